"""CPU: the C-ABI surface of the scaffold analytics (include/diffspectra_scaffold.h) and its argument checks (fake pointers: nothing that would
pass every check is ever passed), the bindings' refusals, and the mirror of tests/scaffold_mirror.py on the hand-stated table of molecules - the
pin of the definitions, since RDKit cannot run here - under renumbering, with the hydrogens stripped, and on the derived set whose coverage the
GPU comparison relies on.  (The kernel is checked on the GPU against the same mirror: tests/test_scaffold_gpu.py.)"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import graph_mirror as GM, scaffold_mirror as K, structure_mirror as SM, valence_mirror as VM

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


@pytest.fixture(scope="module")
def table():
    """The hand-stated molecules with their records and the mirror's rows, computed once."""
    rows = K.hand_table()
    rec, n = SM.records([mol for _, mol, _, _, _ in rows])
    return rows, rec, n, K.analyse_table(rec, n)


def one(mol):
    rec, n = SM.records([mol])
    return K.analyse(rec[0], n[0])


def bits(atoms):
    return sum(1 << i for i in atoms)


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

def test_header_declares_and_library_exports_the_scaffold_function(lib):
    names = ["rec", "n", "P", "scaffold_mask", "ring_mask", "summary", "status", "stream"]
    kinds = ["*", "*", "int64_t", "*", "*", "*", "*", "*"]
    assert abi.SCAFFOLD.exports("dsk_") == list(abi.SCAFFOLD.prototypes) == ["dsk_scaffold_masks"]
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.SCAFFOLD.path).read(), flags=re.S)
    assert hasattr(lib, "dsk_scaffold_masks")
    args = re.search(r"int\s+dsk_scaffold_masks\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
    proto = abi.SCAFFOLD.prototypes["dsk_scaffold_masks"]
    assert proto.params == list(zip(names, kinds)) and proto.ret == "int"
    fn = lib.dsk_scaffold_masks
    assert fn.restype is C.c_int and list(fn.argtypes) == proto.argtypes                                          # bound from the header
    consts = abi.SCAFFOLD.consts
    assert (consts["DSK_OK"], consts["DSK_UNUSABLE"]) == (0, 3) and 1 <= consts["DSK_WAVES"] <= 16
    assert (E.SCAFFOLD_OK, E.SCAFFOLD_UNUSABLE) == (0, 3) == (K.OK, K.UNUSABLE) and E.SCAFFOLD_CONSTS is consts
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.TILES):
        assert not other.exports("dsk_")


def test_library_without_the_symbol_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dsk_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dsk_"):
        abi.SCAFFOLD.bind(Hollow())


def _masks(lib, P=1, rec=FAKE, n=FAKE, outputs=None):
    return lib.dsk_scaffold_masks(rec, n, P, *([FAKE] * 4 if outputs is None else outputs), None)


def test_empty_call_launches_nothing(lib):
    assert _masks(lib, P=0, rec=None, n=None, outputs=[None] * 4) == OK
    assert _masks(lib, P=0, rec=FAKE + 1) == OK                                                       # whatever the pointers


def test_argument_errors_in_the_stated_order(lib):
    """Every pointer here is fake or NULL: a call that got past its checks would fault, so each line also shows that the check comes first."""
    for P in (-1, 2 ** 31, -2 ** 40):                                           # the size, before "an empty call launches nothing" and before any pointer
        assert _masks(lib, P=P) == ERR_ARG and _masks(lib, P=P, rec=None, n=None, outputs=[None] * 4) == ERR_ARG
    assert _masks(lib, rec=None) == ERR_ARG and _masks(lib, n=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _masks(lib, rec=FAKE + off) == ERR_ARG
    for k in range(4):
        out = [FAKE] * 4
        out[k] = None
        assert _masks(lib, outputs=out) == ERR_ARG, f"output {k}"


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    for masks in (E.scaffold_masks, E.DmtEngine.scaffold_masks.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            masks(rec.int(), n)
        with pytest.raises(TypeError, match="n must"):
            masks(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            masks(rec[:, :1000].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            masks(rec, n[:3])
        with pytest.raises(ValueError, match="contiguous"):
            masks(torch.zeros(E.RECORD_BYTES, 4, dtype=torch.uint8).t(), n)
        with pytest.raises(TypeError, match="tensor"):
            masks(rec.numpy(), n)
        with pytest.raises(RuntimeError, match="no CPU path"):
            masks(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.scaffolds(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.scaffold_records(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.scaffold_identity_batch((rec, n), (rec, n))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.get_scaffold_metric((rec, n), unique=False)


# ------------------------------------------------------------------------------------------------------------------ the mirror, pinned by hand

def test_mirror_on_the_hand_stated_table(table):
    rows, rec, n, got = table
    assert len(rows) == 19 and len({name for name, *_ in rows}) == 19
    for (name, mol, scaffold, ring, rings), g in zip(rows, got):
        heavy = int((np.asarray(mol["type"]) != 0).sum())
        assert g == dict(scaffold_mask=bits(scaffold), ring_mask=bits(ring), summary=(heavy, len(scaffold), rings, len(ring)), status=K.OK), (name, g)
    by_name = {name: k for k, (name, *_) in enumerate(rows)}
    # the ring N+ keeps its charge in the scaffold record and loses its methyl; the exocyclic O- of the N-oxide is single-bonded and goes
    k = by_name["1-methylaziridinium (ring N+)"]
    sc = K.scaffold_mol(rec[k], n[k])
    assert sc["type"].tolist() == [2, 1, 1] and sc["fc"].tolist() == [1, 0, 0]
    k = by_name["pyridine N-oxide (N+, O-)"]
    sc = K.scaffold_mol(rec[k], n[k])
    assert sc["type"].tolist() == [2, 1, 1, 1, 1, 1] and sc["fc"].tolist() == [1, 0, 0, 0, 0, 0] and sorted(np.triu(sc["bond"]).ravel().tolist())[-6:] == [1, 1, 1, 2, 2, 2]
    # the parts behind the masks: linkers and exocyclic atoms of the two-ring ketone
    p = K.parts(rec[by_name["dicyclopropyl ketone"]], n[by_name["dicyclopropyl ketone"]])
    assert p["linker"] == {6} and p["exocyclic"] == {7} and p["core"] == set(range(7))
    flat = K.scaffold_mol(rec[by_name["cyclohexanone"]], n[by_name["cyclohexanone"]], bond_orders=False)
    assert len(flat["type"]) == 7 and int(flat["bond"].max()) == 1              # =O became -O


def test_table_under_renumbering_and_without_hydrogens(table):
    rows, rec, n, got = table
    rng = np.random.default_rng(17)
    for (name, mol, scaffold, ring, rings), g in zip(rows, got):
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))                            # new atom i is old atom perm[i]
            new = dict(pos=mol["pos"][perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())
            h = one(new)
            assert h["scaffold_mask"] == bits(i for i in range(len(perm)) if int(perm[i]) in scaffold), name
            assert h["ring_mask"] == bits(i for i in range(len(perm)) if int(perm[i]) in ring) and h["summary"] == g["summary"] and h["status"] == K.OK, name
        assert GM.same_graph(GM.permuted(mol, rng), mol)                        # what the GPU test renumbers with keeps the graph
        bare = one(K.stripped(mol))
        assert bare == g, name                                                  # the heavy atoms come first, so the masks stay as they are


def test_mirror_on_unusable_and_malformed_records(table):
    rows, rec, n, got = table
    zero = dict(scaffold_mask=0, ring_mask=0, summary=(0, 0, 0, 0), status=K.UNUSABLE)
    k = [name for name, *_ in rows].index("cyclohexanone")
    base, count = rec[k], int(n[k])
    assert K.analyse(base, 0) == zero and K.analyse(base, -2) == zero
    bad = base.copy()
    bad[SM.TYPE + 3] = 5
    assert K.analyse(bad, count) == zero
    bad = base.copy()
    bad[SM.BOND + 2 * 29 + 9] = 4
    assert K.analyse(bad, count) == zero
    fine = base.copy()                                                          # the lower triangle, the diagonal, atoms >= n and the pad are not looked at
    fine[SM.BOND + 9 * 29 + 2] = fine[SM.BOND + 4 * 29 + 4] = fine[SM.TYPE + count] = fine[SM.FC + count + 1] = fine[SM.BOND + 1 * 29 + count] = 200
    fine[SM.BOND_END:] = 0xEE
    assert K.analyse(fine, count) == got[k]
    dense = K.analyse(*[x[0] for x in SM.records([GM.k29()])])
    assert dense == dict(scaffold_mask=(1 << 29) - 1, ring_mask=(1 << 29) - 1, summary=(29, 29, 29 * 28 // 2 - 29 + 1, 29), status=K.OK) and dense["summary"][2] == 378


def test_derived_set_covers_the_ground_the_gpu_comparison_stands_on():
    mols = K.derived_set()
    assert 250 <= len(mols) <= 350 and max(len(m["type"]) for m in mols) <= 29
    rec, n = SM.records(mols)
    got = K.analyse_table(rec, n)
    parts = [K.parts(r, k) for r, k in zip(rec, n)]
    assert all(g["status"] == K.OK for g in got)
    assert sum(g["scaffold_mask"] == 0 for g in got) >= 40 and sum(g["summary"][2] >= 2 for g in got) >= 40
    assert sum(bool(p["linker"]) for p in parts) >= 20 and sum(bool(p["exocyclic"]) for p in parts) >= 20
    assert {g["summary"][2] for g in got} >= {0, 1, 2, 3}
    assert all(np.array_equal(a["bond"], b["bond"]) and np.array_equal(a["type"], b["type"]) for a, b in zip(mols, K.derived_set()))      # fixed by the seed


def test_scaf_of_the_mirror(table):
    assert K.cosine({"A": 2, "B": 1}, {"A": 2, "B": 1}) == 1.0 and K.cosine({"A": 3}, {"A": 7}) == 1.0
    assert K.cosine({"A": 2, "B": 1}, {"C": 1, "D": 5}) == 0.0
    assert K.cosine({"A": 2, "B": 1}, {"A": 1, "C": 2}) == 2 / math.sqrt(5 * 5) == 0.4
    assert math.isnan(K.cosine({}, {"A": 1})) and math.isnan(K.cosine({"A": 1}, {})) and math.isnan(K.cosine({}, {}))
    # the same on records: A = dicyclopropyl ketone, B = spiropentane, C = cubane; hexane and toluene have no scaffold at min_rings = 2
    rows, rec, n, got = table
    names = [name for name, *_ in rows]
    pick = lambda *ns: (rec[[names.index(x) for x in ns]], n[[names.index(x) for x in ns]])
    A, B, Cu = "dicyclopropyl ketone", "spiropentane", "cubane"
    gen, test = pick(A, A, B, "hexane", "toluene"), pick(A, Cu, Cu, "toluene")
    assert K.scaf(gen, test, 2) == 2 / math.sqrt(5 * 5) and K.scaf(gen, gen, 2) == 1.0 and K.scaf(pick(B), pick(Cu, A), 2) == 0.0
    assert math.isnan(K.scaf(pick("hexane", "toluene"), test, 2)) and math.isnan(K.scaf(gen, pick("hexane"), 2))
    full = K.scaffold_metric(gen, test, 2)
    assert (full["with_scaffold_generated"], full["with_scaffold_test"], full["distinct_generated"], full["distinct_test"], full["shared"]) == (3, 3, 2, 2, 1)
    assert full["scaffold_class"][3:] == [-1, -1] and full["scaffold_class"][0] == full["scaffold_class"][1] != full["scaffold_class"][2]
    assert full["mean_rings"] == (2 + 2 + 2 + 0 + 1) / 5
    assert K.scaf(gen, test, 1) == (2 + 1) / math.sqrt((4 + 1 + 1) * (1 + 4 + 1))     # toluene's ring enters at min_rings = 1, on both sides
    for name, a, b, same in K.hand_pairs():
        (ra, na), (rb, nb) = SM.records([a]), SM.records([b])
        assert K.same_scaffold((ra[0], na[0]), (rb[0], nb[0])) == (same, K.OK), name
    # Kekule drawings.  Toluene's two are mirror images of each other (atom 1 <-> atom 5), so they are one labelled graph and one scaffold
    # whatever bond_orders says; the two of 2-cyclopropylpyridine are two scaffolds with the orders and one without
    (ra, na), (rb, nb) = SM.records([K.named("toluene")]), SM.records([K.other_kekule_toluene()])
    assert not np.array_equal(ra, rb) and GM.same_graph(K.named("toluene"), K.other_kekule_toluene())
    assert K.same_scaffold((ra[0], na[0]), (rb[0], nb[0]))[0] and K.same_scaffold((ra[0], na[0]), (rb[0], nb[0]), bond_orders=False)[0]
    (ra, na), (rb, nb) = (SM.records([m]) for m in K.kekule_pair())
    assert K.analyse(ra[0], na[0]) == K.analyse(rb[0], nb[0]) == dict(scaffold_mask=511, ring_mask=511, summary=(9, 9, 2, 9), status=K.OK)
    assert not K.same_scaffold((ra[0], na[0]), (rb[0], nb[0]))[0] and K.same_scaffold((ra[0], na[0]), (rb[0], nb[0]), bond_orders=False)[0]


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine:
    """An engine that answers from the mirrors: what ``structure_metrics`` does around the kernels, without them."""

    def scaffold_masks(self, rec, n):
        rows = K.analyse_table(rec.numpy(), n.numpy())
        return (torch.tensor([r["scaffold_mask"] for r in rows], dtype=torch.int32), torch.tensor([r["ring_mask"] for r in rows], dtype=torch.int32),
                torch.tensor([r["summary"] for r in rows], dtype=torch.int32).reshape(len(rows), 4), torch.tensor([r["status"] for r in rows], dtype=torch.uint8))

    def fragment_records(self, rec, n, keep, bonds_from=0, charge_rule=True):
        out, m = VM.fragment_table(rec.numpy(), n.numpy(), keep.numpy(), bonds_from, charge_rule)
        return torch.from_numpy(out), torch.from_numpy(m)

    def graph_hash_records(self, rec, n):
        hashes = [GM.graph_hash(SM.mol_from_record(r, k)) for r, k in zip(rec.numpy(), n.numpy())]
        return torch.tensor([h - ((h >> 63) << 64) for h in hashes], dtype=torch.int64).reshape(-1)          # the 64 bits as int64

    def graph_identity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes=4096):
        verdict = []
        for p in range(prb_n.shape[0]):
            r = p if ref_index is None else int(ref_index[p])
            inside = 0 <= r < ref_n.shape[0]
            verdict.append(3 if not inside else int(GM.same_graph(SM.mol_from_record(prb_rec[p].numpy(), int(prb_n[p])), SM.mol_from_record(ref_rec[r].numpy(), int(ref_n[r])))))
        P = len(verdict)
        return torch.tensor(verdict, dtype=torch.uint8), torch.zeros(P, dtype=torch.int32), torch.full((P, 29), -1, dtype=torch.int32)


def same_partition(got, want):
    """Two class labellings of the same rows, -1 = no class, name the same partition."""
    pairs = set(zip(got, want))
    return len(pairs) == len({g for g, _ in pairs}) == len({w for _, w in pairs}) and all((g == -1) == (w == -1) for g, w in pairs)


def test_public_interface_on_the_mirror_engine(table):
    rows, rec, n, got = table
    names = [name for name, *_ in rows]
    eng = MirrorEngine()
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    found = S.scaffolds(t_rec, t_n.tolist(), engine=eng)
    assert isinstance(found, S.Scaffolds) and found.usable.all() and found.rings.tolist() == [r[4] for r in rows]
    assert found.has_scaffold().tolist() == [r[4] >= 2 for r in rows] and found.has_scaffold(1).tolist() == [r[4] >= 1 for r in rows]
    assert not hasattr(found, "core_mask")
    for orders in (True, False):
        s_rec, s_n = S.scaffold_records(t_rec, t_n, bond_orders=orders, engine=eng)
        assert s_n.tolist() == [len(r[2]) for r in rows] and s_rec.dtype == torch.uint8 and s_rec.shape == t_rec.shape
        for k in range(len(rows)):
            want = K.scaffold_mol(rec[k], n[k], orders)
            mine = SM.mol_from_record(s_rec[k].numpy(), int(s_n[k]))
            assert all(np.array_equal(mine[f], want[f]) for f in ("type", "fc", "bond")), names[k]
    # pairs: the hand pairs, an unusable record, rows outside the table
    pairs = K.hand_pairs()
    a_rec, a_n = (torch.from_numpy(x) for x in SM.records([a for _, a, _, _ in pairs] + [K.named("cubane")] * 3))
    b_rec, b_n = (torch.from_numpy(x) for x in SM.records([b for _, _, b, _ in pairs] + [K.named("cubane")]))
    a_n[5] = 0
    out = S.scaffold_identity_batch((b_rec, b_n), (a_rec, a_n), ref_index=torch.tensor([0, 1, 2, 3, 4, 4, 5]), engine=eng)
    assert isinstance(out, S.ScaffoldIdentity) and out.same.tolist() == [True, False, True, False, True, False, False]
    assert out.status.tolist() == [0, 0, 0, 0, 0, 3, 3] and int(out.undecided) == 0
    # the set metric against the mirror, with and without the molecules made unique
    mols = K.derived_set()
    gen, test = SM.records(mols[30:190:3] + mols[200:210]), SM.records(mols[31:190:3] + mols[30:60:3] + mols[210:215])
    for min_rings in (1, 2):
        want = K.scaffold_metric(gen, test, min_rings)
        assert 0.0 < want["scaf"] < 1.0 and want["shared"] >= 3
        fn = S.get_scaffold_metric((torch.from_numpy(test[0]), test[1]), min_rings=min_rings, unique=False, engine=eng)
        mine = fn((torch.from_numpy(gen[0]), gen[1]))
        assert set(mine) == set(want) and all(mine[k] == want[k] for k in want if k != "scaffold_class"), (mine, want)
        assert isinstance(mine["scaf"], float) and same_partition(mine["scaffold_class"].tolist(), want["scaffold_class"])
    gu, tu = K.unique_rows(*gen), K.unique_rows(*test)
    want = K.scaffold_metric((gen[0][gu], gen[1][gu]), (test[0][tu], test[1][tu]), 2)
    mine = S.get_scaffold_metric((torch.from_numpy(test[0]), test[1]), engine=eng)((torch.from_numpy(gen[0]), gen[1]))
    assert all(mine[k] == want[k] for k in want if k != "scaffold_class") and len(tu) < len(test[1])
    trees = S.get_scaffold_metric((torch.from_numpy(test[0]), test[1]), engine=eng)((torch.from_numpy(gen[0][:1]), gen[1][:1]), keep=torch.tensor([False]))
    assert math.isnan(trees["scaf"]) and math.isnan(trees["mean_rings"]) and trees["n_generated"] == 0


def test_evaluate_adds_the_entry_only_with_the_flag(monkeypatch, tmp_path, table):
    """``metrics['structure']['scaffold']`` under ``config.eval.scaffold`` only (the sampling and the other structure metrics are stubbed: this
    is about the wiring and the host arithmetic, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rows, rec, n, got = table
    names = [name for name, *_ in rows]
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    slots = [names.index(x) for x in ("toluene", "hexane", "dicyclopropyl ketone", "cubane")]
    gen_n = t_n[slots].clone()
    gen_n[3] = 0                                                                # the fourth generated record is unusable
    run = SimpleNamespace(records_by_slot=t_rec[slots].contiguous(), n_atoms=gen_n.tolist(), eng=MirrorEngine(), advance=lambda: None,
                          finish=lambda: ([], None, None), slot_ds=torch.tensor([names.index("cyclohexane")] * 2 + [names.index("dicyclopropyl ketone")] * 2))
    cfg = qm9s_config("ir")
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 1, 1, "", 2
    (tmp_path / "checkpoints").mkdir()
    (tmp_path / "checkpoints" / "checkpoint_1.pth").write_bytes(b"")
    monkeypatch.setattr(EV, "create_model", lambda config: torch.nn.Linear(1, 1))
    monkeypatch.setattr(EV, "restore_checkpoint", lambda path, state, device: state)
    monkeypatch.setattr(EV, "get_cond_sampling_eval_fn", lambda *a, **k: SimpleNamespace(start=lambda model: run))
    monkeypatch.setattr(EV, "_structure_summary", lambda run, table, top_k: dict(success_rate=1.0))
    ds = SimpleNamespace(gt_records=t_rec, num_atom=t_n)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(plain) == {"success_rate"}
    cfg.eval.scaffold = True
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "scaffold"}
    sc = st["scaffold"]
    assert set(sc) == {"scaf", "n_generated", "n_test", "with_scaffold_generated", "with_scaffold_test", "distinct_generated", "distinct_test", "shared",
                       "scaffold_class", "mean_rings", "same_scaffold", "min_rings"}
    # the table has six distinct scaffolds with two rings or more, each once but the two-cyclopropyl linkers' (ketone and propane differ: =O);
    # the generated side has the ketone's once
    want = K.scaffold_metric((rec[slots], gen_n.numpy()), (rec, n), 2)
    assert sc["min_rings"] == 2 and all(sc[k] == want[k] for k in want if k != "scaffold_class") and sc["with_scaffold_generated"] == 1 and sc["shared"] == 1
    assert sc["scaf"] == 1 / math.sqrt(1 * want["with_scaffold_test"]) and sc["mean_rings"] == (1 + 0 + 2) / 3
    same = sc["same_scaffold"]
    assert set(same) == {"same", "status", "rate", "undecided", "top_k"}
    assert same["same"].tolist() == [False, False, True, False] and same["status"].tolist() == [0, 0, 0, 3] and same["rate"] == 1 / 3 and same["undecided"] == 0
    assert same["top_k"]["hit"].tolist() == [False, True] and same["top_k"]["first_hit"].tolist() == [-1, 0] and float(same["top_k"]["acc_at_k"]) == 0.5
    cfg.eval.top_k, cfg.eval.scaffold_min_rings = 1, 1
    sc = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]["scaffold"]
    assert "top_k" not in sc["same_scaffold"] and sc["min_rings"] == 1 and sc["with_scaffold_generated"] == 2
