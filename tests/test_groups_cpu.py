"""CPU: the C-ABI surface of the functional-group analytics (include/diffspectra_groups.h) and its argument checks (fake pointers: nothing that
would pass every check is ever passed), the bindings' refusals, and the mirror of tests/groups_mirror.py on the hand-stated table of molecules -
the pin of the definitions, since RDKit cannot run here - on both Kekule drawings, with hydrogens left implicit, under renumbering, and on the
derived set whose coverage the GPU comparison relies on.  (The kernel is checked on the GPU against the same mirror: tests/test_groups_gpu.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM

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
    rows = G.hand_table()
    rec, n = G.records_of([mol for _, mol, _, _ in rows])
    return rows, rec, n, G.analyse_table(rec, n)


def one(mol):
    rec, n = G.records_of([mol])
    return G.analyse(rec[0], n[0])


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

def test_header_declares_and_library_exports_the_group_functions(lib):
    want = {
        "dsg_group_records": (["rec", "n", "P", "groups", "aromatic_mask", "status", "stream"], ["*", "*", "int64_t", "*", "*", "*", "*"]),
        "dsg_group_similarity_records": (["prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "common", "either", "groups", "status", "stream"],
                                         ["*", "*", "int64_t", "*", "*", "int64_t", "*", "*", "*", "*", "*", "*"]),
    }
    assert abi.GROUPS.exports("dsg_") == list(abi.GROUPS.prototypes) == list(want)
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.GROUPS.path).read(), flags=re.S)
    for name, (names, kinds) in want.items():
        assert hasattr(lib, name)
        args = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
        assert abi.GROUPS.prototypes[name].params == list(zip(names, kinds)) and abi.GROUPS.prototypes[name].ret == "int"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == abi.GROUPS.prototypes[name].argtypes               # bound from the header
    K = abi.GROUPS.consts
    assert (K["DSG_OK"], K["DSG_UNUSABLE"], K["DSG_INVALID"], K["DSG_NUM_GROUPS"]) == (0, 2, 3, 17) and 1 <= K["DSG_WAVES"] <= 16
    assert (E.GROUPS_OK, E.GROUPS_UNUSABLE, E.GROUPS_INVALID, E.NUM_GROUPS) == (0, 2, 3, 17)
    assert S.FUNCTIONAL_GROUP_NAMES == G.NAMES and len(G.NAMES) == 17
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE):
        assert not other.exports("dsg_")


def test_library_without_a_declared_symbol_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dsg_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dsg_"):
        abi.GROUPS.bind(Hollow())


def _groups(lib, P=1, rec=FAKE, n=FAKE, outputs=None):
    return lib.dsg_group_records(rec, n, P, *([FAKE] * 3 if outputs is None else outputs), None)


def _pairs(lib, P=1, M=1, prb_rec=FAKE, prb_n=FAKE, ref_rec=FAKE, ref_n=FAKE, ref_index=FAKE, outputs=None):
    return lib.dsg_group_similarity_records(prb_rec, prb_n, P, ref_rec, ref_n, M, ref_index, *([FAKE] * 4 if outputs is None else outputs), None)


def test_empty_calls_launch_nothing(lib):
    assert _groups(lib, P=0, rec=None, n=None, outputs=[None] * 3) == OK
    assert _groups(lib, P=0, rec=FAKE + 1) == OK                                                      # whatever the pointers
    assert _pairs(lib, P=0, M=0, prb_rec=None, prb_n=None, ref_rec=None, ref_n=None, ref_index=None, outputs=[None] * 4) == OK
    assert _pairs(lib, P=0, M=5, prb_rec=FAKE + 2, ref_rec=FAKE + 3) == OK


def test_argument_errors_in_the_stated_order(lib):
    """Every pointer here is fake or NULL: a call that got past its checks would fault, so each line also shows that the check comes first."""
    # the sizes, before "an empty call launches nothing" and before any pointer
    for P in (-1, 2 ** 31, -2 ** 40):
        assert _groups(lib, P=P) == ERR_ARG and _groups(lib, P=P, rec=None, n=None, outputs=[None] * 3) == ERR_ARG
        assert _pairs(lib, P=P) == ERR_ARG
    for P in (0, 1):
        assert _pairs(lib, P=P, M=-1) == ERR_ARG and _pairs(lib, P=P, M=-1, prb_rec=None) == ERR_ARG
    # then the table: rec, n, the alignment of rec, every output
    assert _groups(lib, rec=None) == ERR_ARG and _groups(lib, n=None) == ERR_ARG
    assert _pairs(lib, prb_rec=None) == ERR_ARG and _pairs(lib, prb_n=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _groups(lib, rec=FAKE + off) == ERR_ARG and _pairs(lib, prb_rec=FAKE + off) == ERR_ARG and _pairs(lib, ref_rec=FAKE + off) == ERR_ARG
    for k in range(3):
        out = [FAKE] * 3
        out[k] = None
        assert _groups(lib, outputs=out) == ERR_ARG, f"output {k}"
    for k in range(4):
        out = [FAKE] * 4
        out[k] = None
        assert _pairs(lib, outputs=out) == ERR_ARG, f"output {k}"
    # then the ground-truth table and the pairing rule
    assert _pairs(lib, ref_rec=None) == ERR_ARG and _pairs(lib, ref_n=None) == ERR_ARG
    assert _pairs(lib, P=3, M=2, ref_index=None) == ERR_ARG and _pairs(lib, P=1, M=0, ref_index=None, ref_rec=None, ref_n=None) == ERR_ARG


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    for groups, pairs in ((E.group_records, E.group_similarity_records),
                          (E.DmtEngine.group_records.__get__(object()), E.DmtEngine.group_similarity_records.__get__(object()))):
        with pytest.raises(TypeError, match="rec"):
            groups(rec.int(), n)
        with pytest.raises(TypeError, match="n must"):
            groups(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            groups(rec[:, :1000].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            groups(rec, n[:3])
        with pytest.raises(ValueError, match="contiguous"):
            groups(torch.zeros(E.RECORD_BYTES, 4, dtype=torch.uint8).t(), n)
        with pytest.raises(TypeError, match="tensor"):
            groups(rec.numpy(), n)
        with pytest.raises(RuntimeError, match="no CPU path"):
            groups(rec, n)
        with pytest.raises(TypeError, match="ref_index"):
            pairs(rec, n, rec, n, torch.zeros(4, dtype=torch.int32))
        with pytest.raises(ValueError, match="ref_index"):
            pairs(rec, n, rec, n, torch.zeros(3, dtype=torch.int64))
        with pytest.raises(ValueError, match="ground-truth row"):
            pairs(rec, n, rec[:2].contiguous(), n[:2].contiguous())
        with pytest.raises(TypeError, match="ref_n"):
            pairs(rec, n, rec, n.long())
        with pytest.raises(RuntimeError, match="no CPU path"):
            pairs(rec, n, rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.functional_groups(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.functional_group_similarity_batch((rec, n), (rec, n))


# ------------------------------------------------------------------------------------------------------------------ the mirror, pinned by hand

def test_mirror_on_the_hand_stated_table(table):
    rows, rec, n, got = table
    assert len(rows) == 40 and len({name for name, _, _, _ in rows}) == 40
    for (name, mol, groups, aromatic), g in zip(rows, got):
        assert g["status"] == G.OK, name
        assert G.names_of(g["groups"]) == groups, (name, G.names_of(g["groups"]), groups)
        assert g["aromatic_mask"] == sum(1 << i for i in aromatic), (name, bin(g["aromatic_mask"]), aromatic)      # heavy atoms come first
    assert all(g["groups"] < 1 << 15 for g in got)                              # sulfide and thiol are never set


def test_both_kekule_drawings_give_identical_outputs(table):
    rows, rec, n, got = table
    by_name = {name: g for (name, _, _, _), g in zip(rows, got)}
    others = G.other_kekule_drawings()
    assert set(others) == {"benzene", "toluene", "pyridine", "naphthalene"}
    for name, mol in others.items():
        first = [m for nm, m, _, _ in rows if nm == name][0]
        assert not np.array_equal(first["bond"], mol["bond"]) and np.array_equal(first["type"], mol["type"]), name     # another drawing of the same atoms
        assert one(mol) == by_name[name], name


def test_implicit_hydrogens_give_the_same_groups(table):
    rows, rec, n, got = table
    by_name = {name: g for (name, _, _, _), g in zip(rows, got)}
    cases = G.implicit_hydrogen_cases()
    assert {name for name, _ in cases} >= {"ethanol", "methane"}
    for name, mol in cases:
        assert one(mol)["groups"] == by_name[name]["groups"], name
    big = one(G.quaterphenyl_29())
    assert G.names_of(big["groups"]) == {"arene", "haloalkane", "alcohol", "amine", "alkane"} and big["aromatic_mask"] == (1 << 24) - 1


def test_similarity_of_hand_stated_pairs(table):
    rows, rec, n, got = table
    by_name = {name: g for (name, _, _, _), g in zip(rows, got)}
    sim = lambda a, b: G.jaccard(G.similarity_pair(by_name[a], by_name[b]))
    assert sim("water", "formamide") == 1.0 and sim("ethanol", "dimethyl ether") == 1 / 3 and sim("benzene", "benzene") == 1.0
    assert sim("acetic acid", "ethanol") == 2 / 3 and sim("benzene", "methane") == 0.0
    pair = G.similarity_pair(by_name["ethanol"], by_name["dimethyl ether"])
    assert (pair["common"], pair["either"], pair["status"]) == (1, 3, G.OK)
    assert G.names_of(pair["groups"][0]) == {"alkane", "alcohol"} and G.names_of(pair["groups"][1]) == {"alkane", "ether"}
    # an unusable record on either side, and a row outside the table
    unusable = G.similarity_table(rec[:2], np.array([0, 5], np.int32), rec[:2], n[:2])
    assert unusable[0] == dict(common=-1, either=-1, groups=(0, 0), status=G.UNUSABLE) and unusable[1]["status"] == G.OK
    outside = G.similarity_table(rec[:3], n[:3], rec[:2], n[:2], ref_index=[1, 2, -1])
    assert [r["status"] for r in outside] == [G.OK, G.INVALID, G.INVALID] and outside[1] == dict(common=-1, either=-1, groups=(0, 0), status=G.INVALID)


def test_mirror_on_unusable_and_malformed_records(table):
    rows, rec, n, got = table
    zero = dict(groups=0, aromatic_mask=0, status=G.UNUSABLE)
    toluene = [k for k, (name, _, _, _) in enumerate(rows) if name == "toluene"][0]
    base, k = rec[toluene], int(n[toluene])
    assert G.analyse(base, 0) == zero and G.analyse(base, -2) == zero
    bad = base.copy()
    bad[SM.TYPE + 3] = 5
    assert G.analyse(bad, k) == zero
    bad = base.copy()
    bad[SM.BOND + 2 * 29 + 9] = 4
    assert G.analyse(bad, k) == zero
    fine = base.copy()                                                          # the lower triangle, the diagonal, atoms >= n and the pad are not looked at
    fine[SM.BOND + 9 * 29 + 2] = fine[SM.BOND + 4 * 29 + 4] = fine[SM.TYPE + k] = fine[SM.FC + k + 1] = fine[SM.BOND + 1 * 29 + k] = 200
    fine[SM.BOND_END:] = 0xEE
    assert G.analyse(fine, k) == got[toluene]
    # every loop is bounded whatever the bytes: the complete graph on 29 carbons has no candidate and no group
    dense = G.analyse(*[x[0] for x in SM.records([GM.k29()])])
    assert dense == dict(groups=0, aromatic_mask=0, status=G.OK)


def test_mirror_is_invariant_under_renumbering(table):
    rows, rec, n, got = table
    rng = np.random.default_rng(17)
    for (name, mol, _, _), g in zip(rows, got):
        for _ in range(2):
            perm = rng.permutation(len(mol["type"]))
            new = dict(pos=mol["pos"][perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())
            h = one(new)
            assert h["groups"] == g["groups"] and h["status"] == G.OK, name
            assert h["aromatic_mask"] == sum(1 << i for i in range(len(perm)) if (g["aromatic_mask"] >> int(perm[i])) & 1), name


def test_derived_set_covers_every_group_both_ways():
    """What the GPU comparison stands on: about 300 molecules, every one of bits 0..14 set in at least five and clear in at least five, at
    least 40 with an aromatic atom and at least 40 with a ring that is not aromatic."""
    mols = G.derived_set()
    assert 250 <= len(mols) <= 350 and max(len(m["type"]) for m in mols) <= 29
    rec, n = G.records_of(mols)
    got = G.analyse_table(rec, n)
    assert all(g["status"] == G.OK for g in got)
    for bit in range(15):
        have = sum((g["groups"] >> bit) & 1 for g in got)
        assert have >= 5 and len(got) - have >= 5, (G.NAMES[bit], have)
    assert sum(g["aromatic_mask"] != 0 for g in got) >= 40
    assert sum(G.has_plain_ring(r, k) for r, k in zip(rec, n)) >= 40
    assert G.derived_set() and all(np.array_equal(a["bond"], b["bond"]) for a, b in zip(mols, G.derived_set()))        # fixed by the seed


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine:
    """An engine that answers the two group calls from the mirror: what ``structure_metrics`` does around the kernel, without it."""

    def group_records(self, rec, n):
        rows = G.analyse_table(rec.numpy(), n.numpy())
        return (torch.tensor([r["groups"] for r in rows], dtype=torch.int32), torch.tensor([r["aromatic_mask"] for r in rows], dtype=torch.int32),
                torch.tensor([r["status"] for r in rows], dtype=torch.uint8))

    def group_similarity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None):
        rows = G.similarity_table(prb_rec.numpy(), prb_n.numpy(), ref_rec.numpy(), ref_n.numpy(), None if ref_index is None else ref_index.tolist())
        return (torch.tensor([r["common"] for r in rows], dtype=torch.int32), torch.tensor([r["either"] for r in rows], dtype=torch.int32),
                torch.tensor([r["groups"] for r in rows], dtype=torch.int32).reshape(len(rows), 2), torch.tensor([r["status"] for r in rows], dtype=torch.uint8))


def test_public_interface_on_the_mirror_engine(table):
    rows, rec, n, got = table
    names = [name for name, _, _, _ in rows]
    eng = MirrorEngine()
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    fg = S.functional_groups(t_rec, t_n.tolist(), engine=eng)
    assert isinstance(fg, S.FunctionalGroups) and fg.usable.all()
    assert fg.names(names.index("anisole")) == ("alkane", "arene", "ether") and fg.names(names.index("water")) == ()
    assert fg.present("arene").tolist() == ["arene" in groups for _, _, groups, _ in rows]
    with pytest.raises(ValueError, match="sulfone"):
        fg.present("sulfone")
    # four candidates for each of two targets: ethanol against (ethanol, dimethyl ether, a row outside, water), benzene against (methane, n = 0, ...)
    pick = lambda *ns: [names.index(x) for x in ns]
    prb_rows = pick("ethanol", "dimethyl ether", "water", "water", "methane", "benzene", "toluene", "phenol")
    prb_n = t_n[prb_rows].clone()
    prb_n[5] = 0
    ref_index = torch.tensor(pick("ethanol", "ethanol") + [-1] + pick("ethanol") + pick("benzene", "benzene", "benzene") + [len(rows)])
    out = S.functional_group_similarity_batch((t_rec, t_n), (t_rec[prb_rows].contiguous(), prb_n), ref_index=ref_index, engine=eng)
    assert isinstance(out, S.GroupSimilarity) and out.similarity.dtype == torch.float64
    assert out.status.tolist() == [0, 0, 3, 0, 0, 2, 0, 3] and out.valid.tolist() == [True, True, False, True, True, False, True, False]
    sim = out.similarity.tolist()
    assert sim[0] == 1.0 and sim[1] == 1 / 3 and sim[2] != sim[2] and sim[3] == 0.0 and sim[4] == 0.0 and sim[5] != sim[5] and sim[6] == 0.5 and sim[7] != sim[7]
    assert out.common.tolist() == [2, 1, -1, 0, 0, -1, 1, -1] and out.either.tolist() == [2, 3, -1, 2, 2, -1, 2, -1]
    top = S.topk_groups(out.similarity, out.status, 4)
    assert top["best"].tolist() == [1.0, 0.5] and top["best_index"].tolist() == [0, 2] and float(top["mean_best"]) == 0.75
    none = S.topk_groups(out.similarity[[2, 5]], out.status[[2, 5]], 2)
    assert none["best"].isnan().all() and none["best_index"].tolist() == [-1] and float(none["mean_best"]) != float(none["mean_best"])
    with pytest.raises(ValueError, match="top_k"):
        S.topk_groups(out.similarity, out.status, 3)
    # neither molecule has a group: 1.0
    both = S.functional_group_similarity_batch((t_rec, t_n), (t_rec, t_n), ref_index=torch.tensor([names.index("formamide")] * len(rows)), engine=eng)
    assert float(both.similarity[names.index("water")]) == 1.0 and int(both.either[names.index("water")]) == 0


def test_evaluate_adds_the_entry_only_with_the_flag(monkeypatch, tmp_path, table):
    """``metrics['structure']['functional_groups']`` under ``config.eval.functional_groups`` only (the sampling and the other structure metrics
    are stubbed: this is about the wiring and the host arithmetic, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rows, rec, n, got = table
    names = [name for name, _, _, _ in rows]
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    slots = [names.index(x) for x in ("ethanol", "dimethyl ether", "benzene", "toluene")]
    gen_n = t_n[slots].clone()
    gen_n[3] = 0                                                                # the fourth generated record is unusable
    run = SimpleNamespace(records_by_slot=t_rec[slots].contiguous(), n_atoms=gen_n.tolist(), eng=MirrorEngine(), advance=lambda: None,
                          finish=lambda: ([], None, None), slot_ds=torch.tensor([names.index("ethanol")] * 2 + [names.index("benzene")] * 2))
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
    cfg.eval.functional_groups = True
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "functional_groups"}
    fg = st["functional_groups"]
    assert set(fg) == {"similarity", "status", "mean", "undefined", "presence_rate", "top_k"}
    assert fg["status"].tolist() == [0, 0, 0, 2] and fg["undefined"] == 1 and fg["mean"] == (1.0 + 1 / 3 + 1.0) / 3
    assert list(fg["presence_rate"]) == list(G.NAMES)
    assert fg["presence_rate"]["alkane"] == 0.5 and fg["presence_rate"]["arene"] == 0.25 and fg["presence_rate"]["thiol"] == 0.0
    assert fg["top_k"]["best"].tolist() == [1.0, 1.0] and fg["top_k"]["best_index"].tolist() == [0, 0]
    cfg.eval.top_k = 1
    assert "top_k" not in EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]["functional_groups"]
