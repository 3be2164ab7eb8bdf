"""CPU: the definition of include/diffspectra_smiles.h as the plain-Python mirror of tests/smiles_mirror.py restates it - the strings that the
definition forces, the round trip through the mirror's own parser, invariance under renaming, agreement with ``graph_mirror.same_graph`` on the
seeded pairs, the grammar, the budget and the certification cap - and the C-ABI surface, the bindings' refusals and the ``evaluate`` flag on an
engine that answers from the mirror.  (The kernel is checked on the GPU against the same mirror: tests/test_smiles_gpu.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import graph_mirror as GM, smiles_mirror as L, structure_mirror as SM

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory
NODE_CAP = 256                       # a condition of the certification check, not a measurement (the worst case here is 160)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def graph_of(mol):
    return {k: mol[k] for k in ("type", "fc", "bond")}


def round_trips(mol, row):
    back = L.parse(row["text"].decode("ascii"))
    return GM.same_graph(graph_of(back), mol) and GM.is_isomorphism(mol, back, L.expanded_order(mol, row["atom_order"]))


def every_molecule():
    ref, prb, _ = GM.seeded_pairs(2000)
    return [m for _, m in L.forced_table()] + [m for _, m in L.property_molecules()] + list(ref) + list(prb)


@pytest.fixture(scope="module")
def rows():
    """The mirror's row of every molecule of the checks, computed once: the forced table, the property molecules, both sides of the seeded pairs."""
    ref, prb = L.seeded_rows(2000)
    return [L.write(m) for _, m in L.forced_table()] + [L.write(m) for _, m in L.property_molecules()] + ref + prb


# ------------------------------------------------------------------------------------------------------------------ the definition

def test_forced_strings_come_out_exactly():
    table = L.forced_table()
    assert [s for s, _ in table] == ["C", "O", "F", "N", "[NH4+]", "[OH-]", "[CH3]", "[CH2]", "[H][H]", "[H]", "[H+]", "CC", "C=C", "C#C", "N#N", "O=C=O", "FF",
                                     "O.O", "C1CC1"]
    for want, mol in table:
        row = L.write(mol)
        assert row["text"] == want.encode() and row["length"] == len(want) and row["status"] == L.OK, (want, row)
        assert row["atom_order"][len(mol["type"]):] == [-1] * (L.W - len(mol["type"]))
    # folded hydrogens have no place in the string; the written atoms have the places 0 .. m-1
    methane = L.write(table[0][1])
    assert methane["atom_order"][:5] == [0, -1, -1, -1, -1]
    assert sorted(L.write(table[8][1])["atom_order"][:2]) == [0, 1]             # H2: both hydrogens are written atoms
    # the written graph of the molecules that the header names
    atoms, label, _ = L.written_graph(L.bridging_hydrogen())
    assert atoms == [0, 1, 2] and label[2] == (0, 0, 0) and label[0] == (1, 0, 2)
    atoms, label, _ = L.written_graph(L.glycine_zwitterion())
    assert atoms == [0, 1, 2, 3, 4] and label[0] == (2, 1, 3) and label[4] == (3, 255, 0)
    assert L.smiles(L.glycine_zwitterion()) in ("[O-]C(=O)C[NH3+]", "O=C([O-])C[NH3+]")


def test_every_string_parses_back_to_its_molecule(rows):
    mols = every_molecule()
    assert len(mols) == len(rows) > 4000
    for mol, row in zip(mols, rows):
        if row["status"] in (L.OK, L.UNCERTIFIED):
            assert round_trips(mol, row), row
    assert [r["status"] for r in rows].count(L.OVERFLOW) == 1


def test_strings_do_not_depend_on_the_atom_numbering():
    rng = np.random.default_rng(20261021)
    ref, _, _ = GM.seeded_pairs(2000)
    for mol in [m for _, m in L.forced_table()] + [m for _, m in L.property_molecules()] + list(ref[:150]):
        want = L.write(mol)
        for _ in range(8):
            got = L.write(GM.permuted(mol, rng))
            assert (got["text"], got["status"], got["nodes"]) == (want["text"], want["status"], want["nodes"])
    # (the twins of a cell are classes of an equivalence, so the count does not depend on who is tried first either); the Kekule drawings:
    # benzene's are one string, 2-methylpyridine's two
    assert L.smiles(L.benzene(0)) == L.smiles(L.benzene(1)) == "C1=CC=CC=C1"
    assert L.smiles(L.methylpyridine(0)) != L.smiles(L.methylpyridine(1))


def test_equal_strings_iff_same_graph_on_the_seeded_pairs():
    ref, prb = L.seeded_rows(2000)
    labels = GM.seeded_labels(2000)
    assert all(r["status"] == L.OK for r in ref + prb)
    assert [a["text"] == b["text"] for a, b in zip(prb, ref)] == labels.tolist() and 400 < int(labels.sum()) < 1600
    for name, a, b in GM.hard_pairs():
        ra, rb = L.write(a), L.write(b)
        assert ra["status"] == rb["status"] == L.OK and ra["text"] != rb["text"], name


def test_grammar(rows):
    allowed = set(b"HCNOF[]()=#+-.%0123456789")
    for row in rows:
        text = row["text"]
        assert row["length"] == len(text) <= L.TEXT_BYTES and set(text) <= allowed
        if row["status"] in (L.OVERFLOW, L.UNUSABLE):
            assert text == b"" and row["atom_order"] == [-1] * L.W
            continue
        depth, open_numbers, at, s = 0, set(), 0, text.decode()
        while at < len(s):
            ch = s[at]
            if ch == "[":
                at = s.index("]", at)
            elif ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
                assert depth >= 0
            elif ch == "%" or ch.isdigit():
                k, at = (int(s[at + 1:at + 3]), at + 2) if ch == "%" else (int(ch), at)
                assert 1 <= k <= L.MAX_RINGS
                open_numbers ^= {k}
            at += 1
        assert depth == 0 and not open_numbers, s
        places = sorted(x for x in row["atom_order"] if x >= 0)
        assert places == list(range(len(places))) and len(places) == len(re.findall(r"\[[^\]]*\]|[CNOF]", s))


def test_budget_and_certification(rows):
    stopped = L.write(L.cubane(), max_nodes=0)
    assert stopped["status"] == L.UNCERTIFIED and 0 < stopped["nodes"] <= 8 and round_trips(L.cubane(), stopped)
    assert L.write(L.cubane())["status"] == L.OK and L.write(L.cubane())["nodes"] > stopped["nodes"]
    easy = L.write(L.propane(), max_nodes=0)
    assert (easy["text"], easy["status"], easy["nodes"]) == (b"C(C)C", L.OK, 1)            # the second end is a twin of the first
    names = [n for n, _ in L.property_molecules()]
    start = len(L.forced_table())
    for k, row in enumerate(rows):
        if start <= k < start + len(names) and names[k - start] == "k29":
            assert (row["status"], row["nodes"], row["length"]) == (L.OVERFLOW, 28, 0)      # one tried atom per level: the others are its twins
        else:
            assert row["status"] == L.OK and row["nodes"] <= NODE_CAP, (k, row)
    by_name = dict(zip(names, rows[start:]))
    assert by_name["hexagon / two triangles / a"]["nodes"] == 18 and by_name["cube / cuneane / a"]["nodes"] == 80 and by_name["29-ring"]["nodes"] == 87
    assert by_name["stacked 10-rings"]["nodes"] == 60 and by_name["29 carbons"]["nodes"] == 28


def test_unusable_and_ignored_bytes():
    rec, n = SM.records([L.glycine_zwitterion()] * 6)
    want = L.write(L.glycine_zwitterion())
    count = int(n[0])
    rec[0, SM.TYPE + 2] = 5
    rec[1, SM.BOND + 1 * 29 + 4] = 4
    n[2] = 0
    rec[3, SM.BOND + 4 * 29 + 1] = 4                                            # lower triangle, diagonal, atoms >= n, pad, positions: not looked at
    rec[3, SM.BOND + 3 * 29 + 3] = rec[3, SM.TYPE + count] = rec[3, SM.BOND + 2 * 29 + count] = 200
    rec[3, SM.BOND_END:] = 0xEE
    rec[3, :SM.TYPE] = 0xFF
    n[4] = -5
    got = L.write_table(rec, n)
    none = dict(text=b"", length=0, status=L.UNUSABLE, nodes=0, atom_order=[-1] * L.W)
    assert got[0] == got[1] == got[2] == got[4] == none and got[3] == got[5] == want


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

def test_header_parses_and_its_constants_are_the_mirrors(lib):
    names = ["rec", "n", "P", "max_nodes", "text", "length", "status", "nodes", "atom_order", "stream"]
    kinds = ["*", "*", "int64_t", "int32_t", "*", "*", "*", "*", "*", "*"]
    assert abi.SMILES.exports("dsl_") == list(abi.SMILES.prototypes) == ["dsl_smiles_records"]
    proto = abi.SMILES.prototypes["dsl_smiles_records"]
    assert proto.params == list(zip(names, kinds)) and proto.ret == "int"
    fn = lib.dsl_smiles_records
    assert fn.restype is C.c_int and list(fn.argtypes) == proto.argtypes
    c = abi.SMILES.consts
    assert (c["DSL_OK"], c["DSL_UNCERTIFIED"], c["DSL_OVERFLOW"], c["DSL_UNUSABLE"]) == (L.OK, L.UNCERTIFIED, L.OVERFLOW, L.UNUSABLE) == (0, 1, 2, 3)
    assert c["DSL_TEXT_BYTES"] == L.TEXT_BYTES == 384 and c["DSL_MAX_RINGS"] == L.MAX_RINGS == 99 and 1 <= c["DSL_WAVES"] <= 16
    assert (E.SMILES_OK, E.SMILES_UNCERTIFIED, E.SMILES_OVERFLOW, E.SMILES_UNUSABLE, E.SMILES_TEXT_BYTES) == (0, 1, 2, 3, 384) and E.SMILES_CONSTS is c
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.SCAFFOLD, abi.TILES):
        assert not other.exports("dsl_")


def _call(lib, P=1, rec=FAKE, n=FAKE, max_nodes=4096, outputs=None):
    return lib.dsl_smiles_records(rec, n, P, max_nodes, *([FAKE] * 5 if outputs is None else outputs), None)


def test_argument_errors_in_the_stated_order(lib):
    """Every pointer here is fake or NULL: a call that got past its checks would fault, so each line also shows that the check comes first."""
    assert _call(lib, P=0, rec=None, n=None, outputs=[None] * 5) == OK and _call(lib, P=0, rec=FAKE + 1) == OK
    for bad in (-1, E.GRAPH_MAX_NODES + 1):
        assert _call(lib, max_nodes=bad) == ERR_ARG and _call(lib, P=0, max_nodes=bad, rec=None, n=None, outputs=[None] * 5) == ERR_ARG
    for P in (-1, 2 ** 31, -2 ** 40):
        assert _call(lib, P=P) == ERR_ARG and _call(lib, P=P, rec=None, n=None, outputs=[None] * 5) == ERR_ARG
    assert _call(lib, rec=None) == ERR_ARG and _call(lib, n=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _call(lib, rec=FAKE + off) == ERR_ARG
        assert _call(lib, outputs=[FAKE + off] + [FAKE] * 4) == ERR_ARG
    for k in range(5):
        out = [FAKE] * 5
        out[k] = None
        assert _call(lib, outputs=out) == ERR_ARG, f"output {k}"


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    for call in (E.smiles_records, E.DmtEngine.smiles_records.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            call(rec.int(), n)
        with pytest.raises(TypeError, match="n must"):
            call(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            call(rec[:, :1000].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            call(rec, n[:3])
        with pytest.raises(TypeError, match="max_nodes"):
            call(rec, n, 3.0)
        with pytest.raises(TypeError, match="max_nodes"):
            call(rec, n, True)
        for bad in (-1, E.GRAPH_MAX_NODES + 1):
            with pytest.raises(ValueError, match="max_nodes"):
                call(rec, n, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.smiles(rec, n)
    with pytest.raises(ValueError, match="max_nodes"):
        S.smiles(rec, n, max_nodes=-2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.smiles_exact_match((rec, n), (rec, n))
    assert S.Smiles._fields == ("text", "length", "status", "nodes", "atom_order")


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine:
    """An engine that answers from the mirror: what ``structure_metrics`` and ``evaluate`` do around the kernel, without it."""

    def smiles_records(self, rec, n, max_nodes=4096):
        rows = L.write_table(rec.numpy(), n.numpy(), max_nodes)
        text = np.zeros((len(rows), L.TEXT_BYTES), np.uint8)
        for p, r in enumerate(rows):
            text[p, :r["length"]] = np.frombuffer(r["text"], np.uint8)
        i32 = lambda key, *shape: torch.tensor([r[key] for r in rows], dtype=torch.int32).reshape(len(rows), *shape)
        return torch.from_numpy(text), i32("length"), torch.tensor([r["status"] for r in rows], dtype=torch.uint8), i32("nodes"), i32("atom_order", L.W)


def _table():
    """Propane, its renumbering, propene, K29, glycine, methane: records and counts as tensors."""
    rng = np.random.default_rng(3)
    propene = GM.saturated(GM.carbons(3, [(0, 1), (1, 2)]))
    propene["bond"][0, 1] = propene["bond"][1, 0] = 2
    rec, n = SM.records([L.propane(), GM.permuted(L.propane(), rng), propene, GM.k29(), L.glycine_zwitterion(), L.forced_table()[0][1]])
    return torch.from_numpy(rec), torch.from_numpy(n)


def test_public_interface_on_the_mirror_engine():
    eng = MirrorEngine()
    rec, n = _table()
    found = S.smiles(rec, n.tolist(), engine=eng)
    assert isinstance(found, S.Smiles) and found.text.shape == (6, 384) and found.text.dtype == torch.uint8
    strings = S.smiles_strings(found)
    assert strings[:3] == ["C(C)C", "C(C)C", strings[2]] and strings[3] is None and strings[5] == "C" and strings[2] not in (None, "C(C)C")
    assert found.certified.tolist() == [True, True, True, False, True, True] and found.has_text.tolist() == found.certified.tolist()
    stopped = S.smiles(rec[:1], n[:1], max_nodes=0, engine=eng)
    assert stopped.status.tolist() == [0] and S.smiles(*[torch.from_numpy(x) for x in SM.records([L.cubane()])], max_nodes=0, engine=eng).status.tolist() == [1]
    # pairs: the same molecule, another one, an overflow row, rows outside the table, an uncertified side
    match = S.smiles_exact_match((rec, n), (rec, n), ref_index=torch.tensor([1, 2, 0, 3, -1, 6]), engine=eng)
    assert isinstance(match, S.SmilesMatch) and match.same.tolist() == [True, False, False, False, False, False]
    assert match.status.tolist() == [0, 0, 0, 2, 3, 3]
    assert S.smiles_exact_match((rec, n), found, engine=eng).same.tolist() == [True, True, True, False, True, True]
    c_rec, c_n = (torch.from_numpy(x) for x in SM.records([L.cubane()]))
    loose = S.smiles_exact_match((c_rec, c_n), (c_rec, c_n), max_nodes=0, engine=eng)
    assert loose.same.tolist() == [False] and loose.status.tolist() == [1]
    with pytest.raises(ValueError, match="ref_index"):
        S.smiles_exact_match((rec[:2], n[:2]), (rec, n), engine=eng)


def test_evaluate_adds_the_entry_only_with_the_flag(monkeypatch, tmp_path):
    """``metrics['structure']['smiles']`` under ``config.eval.smiles`` only, and the file of ``config.eval.smiles_path`` (the sampling and the other
    structure metrics are stubbed: this is about the wiring and the host arithmetic, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rec, n = _table()
    gen_n = n[[0, 2, 3, 1]].clone()
    gen_n[3] = 0                                                                # the fourth generated record is unusable
    run = SimpleNamespace(records_by_slot=rec[[0, 2, 3, 1]].contiguous(), n_atoms=gen_n.tolist(), eng=MirrorEngine(), advance=lambda: None,
                          finish=lambda: ([], None, None), slot_ds=torch.tensor([1, 1, 4, 4]))
    cfg = qm9s_config("ir")
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 1, 1, "", 2
    (tmp_path / "checkpoints").mkdir()
    (tmp_path / "checkpoints" / "checkpoint_1.pth").write_bytes(b"")
    monkeypatch.setattr(EV, "create_model", lambda config: torch.nn.Linear(1, 1))
    monkeypatch.setattr(EV, "restore_checkpoint", lambda path, state, device: state)
    monkeypatch.setattr(EV, "get_cond_sampling_eval_fn", lambda *a, **k: SimpleNamespace(start=lambda model: run))
    monkeypatch.setattr(EV, "_structure_summary", lambda run, table, top_k: dict(success_rate=1.0))
    ds = SimpleNamespace(gt_records=rec, num_atom=n)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(plain) == {"success_rate"}
    cfg.eval.smiles = True
    cfg.eval.smiles_path = str(tmp_path / "out" / "smiles.tsv")
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "smiles"}
    sm = st["smiles"]
    assert set(sm) == {"generated", "ground_truth", "same", "status", "pair_status", "exact_match", "unique", "distinct", "certified", "uncertified",
                       "overflow", "unusable", "top_k"}
    glycine = L.smiles(L.glycine_zwitterion())
    assert sm["generated"][0] == "C(C)C" and sm["generated"][2:] == [None, None] and sm["ground_truth"] == ["C(C)C", "C(C)C", glycine, glycine]
    assert sm["same"].tolist() == [True, False, False, False] and sm["status"].tolist() == [0, 0, 2, 3] and sm["pair_status"].tolist() == [0, 0, 2, 3]
    assert sm["exact_match"] == 0.5 and sm["unique"] == 1.0 and (sm["distinct"], sm["certified"], sm["uncertified"], sm["overflow"], sm["unusable"]) == (2, 2, 0, 1, 1)
    assert sm["top_k"]["hit"].tolist() == [True, False] and sm["top_k"]["first_hit"].tolist() == [0, -1] and float(sm["top_k"]["acc_at_k"]) == 0.5
    lines = open(cfg.eval.smiles_path).read().split("\n")
    assert lines == ["0\tC(C)C\tC(C)C", f"1\t{sm['generated'][1]}\tC(C)C", f"2\t\t{glycine}", f"3\t\t{glycine}", ""]
    cfg.eval.top_k, cfg.eval.smiles_path = 1, None
    sm = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]["smiles"]
    assert "top_k" not in sm and sm["exact_match"] == 0.5
