"""CPU: the C-ABI surface of the valence analytics (include/diffspectra_valence.h) and its argument checks (fake pointers: nothing that would
pass every check is ever passed), the bindings' refusals, the mirror of tests/valence_mirror.py against the reference's recorded results
(tests/golden/g19_stability2d.npz) and on hand-written cases, and the host arithmetic of ``get_edm_metric_2d`` / ``get_edm_metric_3d`` on CPU
tensors with an engine that answers from the mirror.  (The kernels are checked on the GPU against the same mirror: tests/test_valence_gpu.py.)"""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import graph_mirror as GM, structure_mirror as SM, valence_mirror as VM
from tests.test_set_similarity_cpu import MirrorEngine as SetsMirrorEngine

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_stability2d.npz")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def golden():
    z = np.load(GOLDEN)
    return json.loads(str(z["molecules"])), json.loads(str(z["eval_rdmol"])), json.loads(str(z["atom_fc_num"]))


def golden_molecule(row):
    return VM.molecule(row["types"], [tuple(b) for b in row["bonds"]], fc=row["charges"])


def table(mols):
    rec, n = SM.records(mols)
    return torch.from_numpy(rec), torch.from_numpy(n)


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

def test_header_declares_and_library_exports_the_valence_functions(lib):
    want = {
        "dsv_valence_records": (["rec", "n", "P", "bonds_from", "valence", "stable_mask", "valid_mask", "summary", "largest_mask", "status", "stream"],
                                ["*", "*", "int64_t", "int32_t", "*", "*", "*", "*", "*", "*", "*"]),
        "dsv_fragment_records": (["rec", "n", "P", "bonds_from", "keep", "charge_rule", "out_rec", "out_n", "stream"],
                                 ["*", "*", "int64_t", "int32_t", "*", "int32_t", "*", "*", "*"]),
    }
    assert abi.VALENCE.exports("dsv_") == list(abi.VALENCE.prototypes) == list(want)
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.VALENCE.path).read(), flags=re.S)
    for name, (names, kinds) in want.items():
        assert hasattr(lib, name)
        args = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
        assert abi.VALENCE.prototypes[name].params == list(zip(names, kinds)) and abi.VALENCE.prototypes[name].ret == "int"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == abi.VALENCE.prototypes[name].argtypes            # bound from the header
    K = abi.VALENCE.consts
    assert (K["DSV_BONDS_RECORD"], K["DSV_BONDS_DISTANCE"], K["DSV_OK"], K["DSV_UNUSABLE"]) == (0, 1, 0, 3)
    assert (E.BONDS_RECORD, E.BONDS_DISTANCE, E.VALENCE_OK, E.VALENCE_UNUSABLE) == (0, 1, 0, 3) and 1 <= K["DSV_WAVES"] <= 16


def test_the_three_existing_headers_keep_their_prototypes():
    assert (len(abi.SAMPLING.exports("ds_")), len(abi.TRAINING.exports("dst_")), len(abi.SETS.exports("dss_"))) == (31, 50, 3)
    assert (len(abi.SAMPLING.prototypes), len(abi.TRAINING.prototypes), len(abi.SETS.prototypes)) == (31, 50, 3)
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS):
        assert not other.exports("dsv_")


def test_library_without_a_declared_symbol_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dsv_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dsv_"):
        abi.VALENCE.bind(Hollow())


def _valence(lib, P=1, bonds_from=0, rec=FAKE, n=FAKE, outputs=None):
    return lib.dsv_valence_records(rec, n, P, bonds_from, *([FAKE] * 6 if outputs is None else outputs), None)


def _fragment(lib, P=1, bonds_from=0, charge_rule=1, rec=FAKE, n=FAKE, keep=FAKE, out_rec=FAKE, out_n=FAKE):
    return lib.dsv_fragment_records(rec, n, P, bonds_from, keep, charge_rule, out_rec, out_n, None)


def test_empty_calls_launch_nothing(lib):
    for mode in (0, 1):
        assert _valence(lib, P=0, bonds_from=mode, rec=None, n=None, outputs=[None] * 6) == OK
        assert _valence(lib, P=0, bonds_from=mode, rec=FAKE + 1) == OK                              # whatever the pointers
        for rule in (0, 1):
            assert _fragment(lib, P=0, bonds_from=mode, charge_rule=rule, rec=None, n=None, keep=None, out_rec=None, out_n=None) == OK
            assert _fragment(lib, P=0, bonds_from=mode, charge_rule=rule, out_rec=FAKE + 2) == OK


def test_bad_scalars_are_refused_first(lib):
    """... before "an empty call launches nothing" and before any pointer is looked at: every pointer here is fake or NULL."""
    for P in (0, 1):
        for bad in (-1, 2, 3, 256, 1 << 30):
            assert _valence(lib, P=P, bonds_from=bad) == ERR_ARG and _valence(lib, P=P, bonds_from=bad, rec=None) == ERR_ARG
            assert _fragment(lib, P=P, bonds_from=bad) == ERR_ARG and _fragment(lib, P=P, charge_rule=bad) == ERR_ARG
            assert _fragment(lib, P=P, charge_rule=bad, keep=None) == ERR_ARG
    for P in (-1, 2 ** 31, -2 ** 40):
        assert _valence(lib, P=P) == ERR_ARG and _fragment(lib, P=P) == ERR_ARG
        assert _valence(lib, P=P, rec=None, n=None, outputs=[None] * 6) == ERR_ARG


def test_every_pointer_is_required_and_alignment_is_checked(lib):
    assert _valence(lib, rec=None) == ERR_ARG and _valence(lib, n=None) == ERR_ARG
    for k in range(6):
        out = [FAKE] * 6
        out[k] = None
        assert _valence(lib, outputs=out) == ERR_ARG, f"output {k}"
    for key in ("rec", "n", "keep", "out_rec", "out_n"):
        assert _fragment(lib, **{key: None}) == ERR_ARG, key
    for off in (1, 2, 3):
        assert _valence(lib, rec=FAKE + off) == ERR_ARG and _fragment(lib, rec=FAKE + off) == ERR_ARG and _fragment(lib, out_rec=FAKE + off) == ERR_ARG


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    keep = torch.full((4,), 7, dtype=torch.int32)
    for valence, fragment in ((E.valence_records, E.fragment_records),
                              (E.DmtEngine.valence_records.__get__(object()), E.DmtEngine.fragment_records.__get__(object()))):
        with pytest.raises(TypeError, match="rec"):
            valence(rec.int(), n)
        with pytest.raises(TypeError, match="n must"):
            valence(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            valence(rec[:, :1000].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            valence(rec, n[:3])
        with pytest.raises(ValueError, match="contiguous"):
            valence(torch.zeros(E.RECORD_BYTES, 4, dtype=torch.uint8).t(), n)
        with pytest.raises(TypeError, match="tensor"):
            valence(rec.numpy(), n)
        for bad in (True, 1.0, "record"):
            with pytest.raises(TypeError, match="bonds_from"):
                valence(rec, n, bad)
            with pytest.raises(TypeError, match="bonds_from"):
                fragment(rec, n, keep, bad)
        for bad in (-1, 2):
            with pytest.raises(ValueError, match="bonds_from"):
                valence(rec, n, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            valence(rec, n)
        with pytest.raises(TypeError, match="keep"):
            fragment(rec, n, keep.long())
        with pytest.raises(ValueError, match="keep"):
            fragment(rec, n, keep[:3])
        with pytest.raises(ValueError, match="contiguous"):
            fragment(rec, n, torch.zeros(4, 2, dtype=torch.int32)[:, 0])
        with pytest.raises(TypeError, match="rec"):
            fragment(rec.float(), n, keep)
        with pytest.raises(TypeError, match="charge_rule"):
            fragment(rec, n, keep, 0, 1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fragment(rec, n, keep)
    with pytest.raises(ValueError, match="bonds"):
        S.valence_batch(rec, n, bonds="both")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.valence_batch(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.largest_fragment_records(rec, n, bonds="distance")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.get_edm_metric_2d()(rec, n)


# ------------------------------------------------------------------------------------------------------------------ the mirror against the reference

def test_mirror_reproduces_the_reference_on_g19():
    rows, _, fc_num = golden()
    assert len(rows) >= 40
    # the applied-charge table is the data set's atom_fc_num
    assert sorted("HCNOF"[t] + str(c) for t, c in VM.APPLIED) == fc_num
    for row in rows:
        mol = golden_molecule(row)
        rec, n = SM.records([mol])
        got = VM.analyse(rec[0], n[0])
        name = row["name"]
        assert got["status"] == VM.OK and got["summary"][0] == row["ref_atom_num"], name
        assert got["summary"][1] == row["ref_nr_stable"] and VM.flags(got)[0] == row["ref_stable"], name
        assert [VM.applied_charge(t, c) for t, c in zip(row["types"], row["charges"])] == row["ref_applied"], name
        # the extractor with a full mask writes the charges the reference set
        out, m = VM.fragment(rec[0], n[0], (1 << len(row["types"])) - 1)
        assert m == len(row["types"]) and SM.mol_from_record(out, m)["fc"].tolist() == row["ref_applied"], name
    by_name = {row["name"]: VM.flags(VM.analyse(*[x[0] for x in SM.records([golden_molecule(row)])])) for row in rows}
    assert by_name["NH (valid, unstable)"] == (False, True, True) and by_name["OH3 fc +1 (stable, invalid)"] == (True, False, False)
    assert by_name["F fc -1 beside H fc +1"] == (True, True, False) and by_name["CH3 fc +2 and an H fc +1"] == (True, True, False)
    assert by_name["NH4 fc +1"] == (True, True, True) and by_name["nitromethane, charges separated"] == (True, True, True)
    assert by_name["five-valent carbon"] == (False, False, False) and by_name["lone carbon"] == (False, True, True)


def test_mirror_reproduces_the_reference_aggregation_on_g19():
    """``eval_rdmol``'s denominators, ``set`` and ``- {None}``: its sanitisation, fragments and SMILES were the generator's stand-in."""
    rows, cases, _ = golden()
    mols = [golden_molecule(row) for row in rows]
    assert {c["name"] for c in cases} >= {"all", "all, with known", "nothing valid", "fragments"}
    for case in cases:
        rec, n = SM.records([mols[k] for k in case["rows"]])
        known = None if case["known"] is None else [mols[k] for k in case["known"]]
        got = VM.edm_metric(rec, n, VM.RECORD, known)
        assert {k: got[k] for k in case["result"]} == case["result"], case["name"]


# ------------------------------------------------------------------------------------------------------------------ the mirror, by hand

def test_mirror_on_hand_written_cases():
    H, Cc, N, O, F = range(5)
    one = lambda mol, mode=VM.RECORD: VM.analyse(*[x[0] for x in SM.records([mol])], mode)
    water = VM.molecule([O, H, H], [(0, 1, 1), (0, 2, 1)])
    assert one(water) == dict(valence=[2, 1, 1] + [0] * 26, stable_mask=7, valid_mask=7, summary=(3, 3, 1, 3), largest_mask=7, status=0)
    # two fragments of equal size: the one with the lowest atom wins; an isolated atom is a fragment
    mixed = VM.molecule([H, O, H, O, H, H, Cc], [(1, 4, 1), (1, 5, 1), (3, 0, 1), (3, 2, 1)])
    got = one(mixed)
    assert got["summary"] == (7, 6, 3, 3) and got["largest_mask"] == 0b0001101 and got["stable_mask"] == 0b0111111 and got["valid_mask"] == 0b1111111
    assert VM.flags(got) == (False, True, False)
    # the raw charge decides stability, the applied charge validity: O+ with three bonds is stable (raw +1) and invalid (no charge applied)
    oxonium = VM.molecule([O, H, H, H], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], fc=[1, 0, 0, 0])
    assert one(oxonium)["stable_mask"] == 0b1111 and one(oxonium)["valid_mask"] == 0b1110
    ammonium = VM.molecule([N, H, H, H, H], [(0, k, 1) for k in range(1, 5)], fc=[1, 0, 0, 0, 0])
    assert VM.flags(one(ammonium)) == (True, True, True)
    # unusable: n = 0, a type byte 5, a bond byte 4; a bond byte 4 between atoms >= n, in the lower triangle or on the diagonal is not looked at
    zero = dict(valence=[0] * 29, stable_mask=0, valid_mask=0, summary=(0, 0, 0, 0), largest_mask=0, status=3)
    rec, n = SM.records([water])
    assert VM.analyse(rec[0], 0) == zero and VM.analyse(rec[0], -3) == zero
    bad = rec[0].copy()
    bad[VM.TYPE + 2] = 5
    assert VM.analyse(bad, 3) == zero and VM.analyse(bad, 2)["status"] == 0 and VM.fragment(bad, 3, 7)[1] == 0 and not VM.fragment(bad, 3, 7)[0].any()
    bad = rec[0].copy()
    bad[VM.BOND + 0 * 29 + 2] = 4
    assert VM.analyse(bad, 3) == zero and VM.analyse(bad, 2)["status"] == 0
    fine = rec[0].copy()
    fine[VM.BOND + 1 * 29 + 0] = fine[VM.BOND + 3 * 29 + 4] = fine[VM.BOND + 1 * 29 + 1] = fine[VM.TYPE + 3] = 200
    fine[VM.BOND_END:] = 0xEE
    assert VM.analyse(fine, 3) == one(water) and VM.analyse(fine, 40)["status"] == 3
    # the extractor: heavy atoms of ethanol in ascending order, symmetric bonds, zeros elsewhere; charge rule on and off
    ethanol = VM.molecule([H, Cc, H, Cc, O, H, H, H, H], [(1, 3, 1), (3, 4, 1), (0, 1, 1), (2, 1, 1), (5, 1, 1), (6, 3, 1), (7, 3, 1), (8, 4, 1)],
                          fc=[1, 0, 0, 2, -1, 0, 0, 0, 0], pos=np.arange(27).reshape(9, 3))
    rec, n = SM.records([ethanol])
    out, m = VM.fragment(rec[0], 9, 0b000011010 | (1 << 20), charge_rule=True)
    heavy = SM.mol_from_record(out, m)
    assert m == 3 and heavy["type"].tolist() == [Cc, Cc, O] and heavy["fc"].tolist() == [0, 0, -1] and heavy["pos"][:, 0].tolist() == [3.0, 9.0, 12.0]
    assert heavy["bond"].tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    assert np.array_equal(out, SM.records([heavy])[0][0])                                                     # nothing else in the record
    raw = SM.mol_from_record(*VM.fragment(rec[0], 9, 0b000011011, charge_rule=False))
    assert raw["fc"].tolist() == [1, 0, 2, -1]
    again, m2 = VM.fragment(out, m, (1 << 29) - 1)
    assert m2 == m and np.array_equal(again, out)


def test_mirror_on_a_29_atom_chain_under_three_numberings():
    for seed in (None, 1, 2):
        mol = VM.chain(29, None if seed is None else np.random.default_rng(seed))
        rec, n = SM.records([mol])
        got = VM.analyse(rec[0], 29)
        assert got["summary"] == (29, 0, 1, 29) and got["largest_mask"] == (1 << 29) - 1 and got["valid_mask"] == (1 << 29) - 1
        assert sorted(got["valence"]) == [1, 1] + [2] * 27
    two = GM.permuted(VM.molecule([1] * 29, [(i, i + 1, 1) for i in range(28) if i != 13]), np.random.default_rng(3))
    got = VM.analyse(*[x[0] for x in SM.records([two])])
    assert got["summary"][2:] == (2, 15) and bin(got["largest_mask"]).count("1") == 15


def test_mirror_distance_orders():
    H, Cc, N, O, F = range(5)
    # methane at 1.09 A: four single C-H bonds; the hydrogens are 1.78 A apart: no H-H bond (74 + 10 pm)
    t = 1.09 / math.sqrt(3.0)
    methane = VM.molecule([Cc, H, H, H, H], [], pos=[[0, 0, 0], [t, t, t], [t, -t, -t], [-t, t, -t], [-t, -t, t]])
    rec, n = SM.records([methane])
    got = VM.analyse(rec[0], 5, VM.DISTANCE)
    assert got["valence"][:5] == [4, 1, 1, 1, 1] and got["summary"] == (5, 5, 1, 5) and VM.flags(got) == (True, True, True)
    out, m = VM.fragment(rec[0], 5, 31, VM.DISTANCE)
    assert SM.mol_from_record(out, m)["bond"][0].tolist() == [0, 1, 1, 1, 1] and VM.analyse(out, m, VM.RECORD)["summary"] == (5, 5, 1, 5)
    # C-C at 1.50 / 1.36 / 1.21 A: single, double, triple (154 + 10, 134 + 5, 120 + 3 pm); the record's bonds and charges are ignored
    for d, order in ((1.70, 0), (1.50, 1), (1.36, 2), (1.21, 3)):
        pair = VM.molecule([Cc, Cc], [(0, 1, 3)], fc=[1, -1], pos=[[0, 0, 0], [0, d, 0]])
        rec, n = SM.records([pair])
        assert VM.analyse(rec[0], 2, VM.DISTANCE)["valence"][:2] == [order, order]
        out, m = VM.fragment(rec[0], 2, 3, VM.DISTANCE, charge_rule=False)
        assert SM.mol_from_record(out, m)["fc"].tolist() == [0, 0] and SM.mol_from_record(out, m)["bond"][0, 1] == order
    assert VM.near_threshold(164.005) and not VM.near_threshold(164.02) and 164 in VM.THRESHOLDS and 123 in VM.THRESHOLDS and 139 in VM.THRESHOLDS


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine(SetsMirrorEngine):
    """The CPU engine of tests/test_set_similarity_cpu.py (graph hash and identity from the mirrors) with the two valence calls from this
    module's mirror: what ``structure_metrics`` does around the kernels, without them."""

    def valence_records(self, rec, n, bonds_from=0):
        rows = VM.analyse_table(rec.numpy(), n.numpy(), bonds_from)
        col = lambda key, dt: torch.tensor([r[key] for r in rows], dtype=dt).reshape(len(rows), *{"valence": [VM.W], "summary": [4]}.get(key, []))
        return (col("valence", torch.uint8), col("stable_mask", torch.int32), col("valid_mask", torch.int32), col("summary", torch.int32),
                col("largest_mask", torch.int32), col("status", torch.uint8))

    def fragment_records(self, rec, n, keep, bonds_from=0, charge_rule=True):
        out, m = VM.fragment_table(rec.numpy(), n.numpy(), keep.numpy(), bonds_from, charge_rule)
        return torch.from_numpy(out), torch.from_numpy(m)


def _hand_table():
    H, Cc, N, O, F = range(5)
    rng = np.random.default_rng(11)
    water = VM.molecule([O, H, H], [(0, 1, 1), (0, 2, 1)])
    methane = VM.molecule([Cc, H, H, H, H], [(0, k, 1) for k in range(1, 5)])
    both = VM.molecule([Cc, H, H, H, H, O, H, H], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (5, 6, 1), (5, 7, 1)])      # largest: methane
    oxonium = VM.molecule([O, H, H, H], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], fc=[1, 0, 0, 0])                               # stable, invalid
    imine = VM.molecule([N, H], [(0, 1, 1)])                                                                              # valid, unstable
    mols = [water, methane, both, oxonium, imine, GM.permuted(water, rng), GM.permuted(methane, rng), VM.molecule([Cc], [])]
    rec, n = SM.records(mols)
    rec = np.concatenate([rec, rec[:2]])                                       # two unusable rows: a type byte 5, and n = 0
    n = np.concatenate([n, np.array([3, 0], np.int32)])
    rec[8, VM.TYPE + 1] = 5
    return torch.from_numpy(rec), torch.from_numpy(n), [water, methane]


def test_edm_metric_denominators_on_a_hand_made_table():
    eng = MirrorEngine()
    rec, n, known = _hand_table()
    out = S.get_edm_metric_2d(engine=eng)(rec, n)
    assert set(out) == {"mol_stable", "atom_stable", "Validity", "Complete", "Unique", "Novelty", "valence", "valid", "largest"}
    # 10 rows, 3+5+8+4+2+3+5+1 + 3 + 0 = 34 atoms; stable molecules: water, methane, both, oxonium, water, methane = 6;
    # stable atoms 3+5+8+4+1+3+5+0 = 29; valid: all usable but oxonium = 7; complete: those but `both` = 6;
    # distinct largest fragments of the valid: water, methane, NH, C = 4
    assert (out["mol_stable"], out["atom_stable"], out["Validity"], out["Complete"], out["Unique"], out["Novelty"]) == (6 / 10, 29 / 34, 7 / 10, 6 / 10, 4 / 10, -1)
    assert isinstance(out["valence"], S.Valence) and out["valid"].tolist() == [True, True, True, False, True, True, True, True, False, False]
    assert out["valence"].mol_stable.tolist() == [True, True, True, True, False, True, True, False, False, False]
    assert out["valence"].complete.tolist() == [True, True, False, False, True, True, True, True, False, False]
    assert out["valence"].status.tolist() == [0] * 8 + [3, 3] and out["largest"][1].tolist() == [3, 5, 5, 4, 2, 3, 5, 1, 0, 0]
    want = VM.edm_metric(rec.numpy(), n.numpy(), VM.RECORD, None)
    assert {k: out[k] for k in want} == want
    # novelty against known molecules: NH and the lone carbon are new; unusable and invalid rows enter no numerator
    with_known = S.get_edm_metric_2d(known=table(known), engine=eng)(rec, n)
    assert with_known["Novelty"] == 2 / 10 and with_known["Unique"] == 4 / 10
    assert {k: with_known[k] for k in want} == VM.edm_metric(rec.numpy(), n.numpy(), VM.RECORD, known)
    # the wrappers
    v = S.valence_batch(rec, n.tolist(), engine=eng)
    assert isinstance(v, S.Valence) and torch.equal(v.summary, out["valence"].summary)
    f_rec, f_n = S.largest_fragment_records(rec, n, engine=eng)
    assert torch.equal(f_rec, out["largest"][0]) and torch.equal(f_n, out["largest"][1])
    # nothing valid: Unique 0 as the reference sets it, Novelty 0 of nothing; no rows at all: NaN
    none = S.get_edm_metric_2d(known=table(known), engine=eng)(rec[[3, 8, 9]].contiguous(), n[[3, 8, 9]].contiguous())
    assert (none["Validity"], none["Complete"], none["Unique"], none["Novelty"], none["mol_stable"], none["atom_stable"]) == (0.0, 0.0, 0.0, 0.0, 1 / 3, 4 / 7)
    empty = S.get_edm_metric_2d(engine=eng)(rec[:0], n[:0])
    assert all(math.isnan(empty[k]) for k in ("mol_stable", "atom_stable", "Validity", "Complete", "Unique")) and empty["Novelty"] == -1


def test_edm_metric_on_the_reference_aggregation():
    rows, cases, _ = golden()
    mols = [golden_molecule(row) for row in rows]
    eng = MirrorEngine()
    for case in cases:
        known = None if case["known"] is None else table([mols[k] for k in case["known"]])
        got = S.get_edm_metric_2d(known=known, engine=eng)(*table([mols[k] for k in case["rows"]]))
        assert {k: got[k] for k in case["result"]} == case["result"], case["name"]
    stable = sum(row["ref_stable"] for row in rows) / len(rows)
    atoms = sum(row["ref_nr_stable"] for row in rows) / sum(row["ref_atom_num"] for row in rows)
    got = S.get_edm_metric_2d(engine=eng)(*table(mols))
    assert (got["mol_stable"], got["atom_stable"]) == (stable, atoms)                 # get_2D_edm_metric's own two fractions


def test_edm_metric_3d_uses_the_distances():
    eng = MirrorEngine()
    t = 1.09 / math.sqrt(3.0)
    methane = VM.molecule([1, 0, 0, 0, 0], [], fc=[1, 0, 0, 0, 0], pos=[[0, 0, 0], [t, t, t], [t, -t, -t], [-t, t, -t], [-t, -t, t]])
    apart = VM.molecule([1, 0], [(0, 1, 1)], pos=[[0, 0, 0], [0, 0, 3.0]])
    rec, n = table([methane, apart])
    out = S.get_edm_metric_3d(engine=eng)(rec, n)
    assert (out["mol_stable"], out["atom_stable"], out["Validity"], out["Complete"], out["Unique"]) == (0.5, 5 / 7, 1.0, 0.5, 1.0)
    flat = S.get_edm_metric_2d(engine=eng)(rec, n)                                    # the same records by their (absent / present) bond bytes
    assert (flat["mol_stable"], flat["Complete"]) == (0.0, 0.5)
    assert SM.mol_from_record(out["largest"][0][0].numpy(), 5)["bond"][0].tolist() == [0, 1, 1, 1, 1] and out["largest"][1].tolist() == [5, 1]


def test_evaluate_without_the_flag_has_no_edm_keys(monkeypatch, tmp_path):
    """The driver adds ``metric_2d`` / ``metric_3d`` under ``config.eval.edm_metrics`` only (the sampling and the other structure metrics are
    stubbed: this is about the wiring, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rec, n, known = _hand_table()
    eng = MirrorEngine()
    run = SimpleNamespace(records_by_slot=rec, n_atoms=n.tolist(), eng=eng, advance=lambda: None, finish=lambda: ([], None, None))
    cfg = qm9s_config("ir")
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts = 1, 1, ""
    (tmp_path / "checkpoints").mkdir()
    (tmp_path / "checkpoints" / "checkpoint_1.pth").write_bytes(b"")
    monkeypatch.setattr(EV, "create_model", lambda config: torch.nn.Linear(1, 1))
    monkeypatch.setattr(EV, "restore_checkpoint", lambda path, state, device: state)
    monkeypatch.setattr(EV, "get_cond_sampling_eval_fn", lambda *a, **k: SimpleNamespace(start=lambda model: run))
    monkeypatch.setattr(EV, "_structure_summary", lambda run, table, top_k: dict(success_rate=1.0))
    ds = SimpleNamespace(gt_records=rec, num_atom=n)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(plain) == {"success_rate"}
    cfg.eval.edm_metrics = True
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True, known_records=table(known))[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "metric_2d", "metric_3d"}
    want = S.get_edm_metric_2d(known=table(known), engine=eng)(rec, n)
    assert {k: st["metric_2d"][k] for k in ("mol_stable", "atom_stable", "Validity", "Complete", "Unique", "Novelty")} == \
        {k: want[k] for k in ("mol_stable", "atom_stable", "Validity", "Complete", "Unique", "Novelty")}
    assert st["metric_2d"]["Novelty"] == 2 / 10 and st["metric_3d"]["Novelty"] >= 0
