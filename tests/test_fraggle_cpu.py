"""CPU: the Fraggle rule of include/diffspectra_fraggle.h as tests/fraggle_mirror.py restates it, pinned to the hand-stated table of fragmentations
and to the properties the rule must have (invariance under renumbering, one fingerprint for both Kekule drawings, fraggle(X, X), fraggle >=
plain, a budget verdict that does not depend on the enumeration); the ground the GPU comparison of tests/test_fraggle_gpu.py stands on; and
the CPU-loadable surface of the three entry points."""
import math

import numpy as np
import pytest
import torch

from tests import brics_mirror as B, fraggle_mirror as F, groups_mirror as G, structure_mirror as SM


@pytest.fixture(scope="module")
def table():
    rows = F.hand_table()
    rec, n = SM.records([mol for _, mol, _ in rows])
    return rows, rec, n


@pytest.fixture(scope="module")
def derived():
    prb, ref = F.derived_pairs()
    (pr, pn), (rr, rn) = SM.records(prb), SM.records(ref)
    return dict(prb=(pr, pn), ref=(rr, rn), rows=F.similarity_table(pr, pn, rr, rn))


def moved_mask(mask, perm):
    new = {int(old): i for i, old in enumerate(perm)}
    return sum(1 << new[a] for a in range(29) if (mask >> a) & 1)


# ------------------------------------------------------------------------------------------------------------------ the rule

def test_the_hand_table(table):
    rows, rec, n = table
    assert len(rows) >= 20
    kinds = set()
    for (name, mol, stated), r, k in zip(rows, rec, n):
        got = F.fragmentation_row(r, k)
        want = F.stated_rows(mol, stated)
        assert got["status"] == F.OK and [row[:3] for row in got["rows"]] == want[:F.MAX_FRAGMENTATIONS], name
        assert got["summary"][3] == len(want) | (F.TRUNCATED if len(want) > F.MAX_FRAGMENTATIONS else 0), name
        kinds |= {kind for kind, _, _ in stated}
    assert kinds == {0, 1, 2, 3}
    by_name = {name: F.fragmentation_row(r, k) for (name, _, _), r, k in zip(rows, rec, n)}
    assert by_name["n-hexane"]["summary"] == (6, 5, 0, 11) and by_name["cubane"]["summary"] == (8, 0, 12, 0)
    assert by_name["29-atom chain"]["summary"][3] & F.TRUNCATED and len(by_name["29-atom chain"]["rows"]) == F.MAX_FRAGMENTATIONS
    assert by_name["pentane and ethanol"]["summary"][0] == 8 and by_name["ethanol whose hydroxyl hydrogen bridges to ethyl"]["summary"][0] == 6


def test_every_output_moves_with_a_renumbering(table):
    rows, rec, n = table
    rng = np.random.default_rng(5)
    for (name, mol, stated), r, k in zip(rows, rec, n):
        perm = rng.permutation(len(mol["type"]))
        m_rec, m_n = SM.records([B.renumbered(mol, perm)])
        got = F.fragmentation_row(m_rec[0], m_n[0])
        if not got["summary"][3] & F.TRUNCATED:
            assert F.unpacked_rows(got["rows"]) == F.moved_rows(stated, perm), name
        assert got["summary"] == F.fragmentation_row(r, k)["summary"], name
        a, b = F.Mol(r, k).fingerprint(F.DEFAULT_NODES), F.Mol(m_rec[0], m_n[0]).fingerprint(F.DEFAULT_NODES)
        new = {int(old): i for i, old in enumerate(perm)}
        assert a.fp == b.fp and a.count == b.count and {new[x]: bits for x, bits in a.atom_bits.items()} == b.atom_bits, name


def test_similarity_is_invariant_under_renumbering_either_record(derived):
    rng = np.random.default_rng(6)
    (pr, pn), (rr, rn), rows = derived["prb"], derived["ref"], derived["rows"]
    for p in range(0, len(pn), 9):
        prb, ref = SM.mol_from_record(pr[p], pn[p]), SM.mol_from_record(rr[p], rn[p])
        perm_r, perm_q = rng.permutation(len(prb["type"])), rng.permutation(len(ref["type"]))
        moved = F.similarity_pair(tuple(x[0] for x in SM.records([B.renumbered(prb, perm_r)])), tuple(x[0] for x in SM.records([B.renumbered(ref, perm_q)])))
        want = rows[p]
        # the order of the fragmentations within a kind moves with the numbering, so the winner of a tie may be another: the values stay
        assert (moved["plain"], moved["n_fragmentations"], moved["status"]) == (want["plain"], want["n_fragmentations"], want["status"]), p
        assert F.ratio(moved["modified"]) == F.ratio(want["modified"]) and F.fraggle(moved) == F.fraggle(want), p
        if want["n_fragmentations"] == 1:                                         # no tie to break: the masks move with the permutations
            assert moved["marked"] == (moved_mask(want["marked"][0], perm_q), moved_mask(want["marked"][1], perm_r)), p


def test_both_kekule_drawings_of_o_xylene_give_one_fingerprint():
    tail, hydrogens = [(0, 6, 1), (1, 7, 1)], [0, 0, 1, 1, 1, 1, 3, 3]
    one, other = (G.molecule("C" * 8, G._ring(first) + tail, hydrogens) for first in (True, False))
    rec, n = SM.records([one, other])
    assert not np.array_equal(rec[0], rec[1])
    a, b = (F.Mol(r, k) for r, k in zip(rec, n))
    assert a.aromatic == b.aromatic == set(range(6)) and {c for _, _, c in a.bonds} == {0, 3}
    fa, fb = a.fingerprint(F.DEFAULT_NODES), b.fingerprint(F.DEFAULT_NODES)
    assert fa.fp == fb.fp and fa.atom_bits == fb.atom_bits and fa.count == fb.count > 0
    assert F.fragmentation_row(rec[0], n[0]) == F.fragmentation_row(rec[1], n[1])
    row = F.similarity_pair((rec[0], n[0]), (rec[1], n[1]))
    assert row["plain"][0] == row["plain"][1] and F.fraggle(row) == 1.0


def test_self_similarity_is_one_iff_there_is_a_fragmentation(table):
    rows, rec, n = table
    seen = set()
    for (name, _, stated), r, k in zip(rows, rec, n):
        if name == "29-atom chain":                                              # 291 fragmentations: the GPU test has it
            continue
        row = F.similarity_pair((r, k), (r, k))
        assert row["status"] == F.OK and row["plain"][0] == row["plain"][1] and row["n_fragmentations"] == len(stated), name
        assert F.fraggle(row) == (1.0 if stated else 0.0), name
        seen.add(bool(stated))
    assert seen == {True, False}


def test_fraggle_is_at_least_plain_and_the_float_is_defined(derived):
    for row in derived["rows"]:
        value = F.fraggle(row)
        if row["n_fragmentations"]:
            assert value >= F.ratio(row["plain"]) and value >= F.ratio(row["modified"]) and 0.0 <= value <= 1.0
        else:
            assert value == 0.0 and row["modified"] == (-1, -1) and row["best_index"] == -1 and row["marked"] == (0, 0)
    assert math.isnan(F.fraggle(dict(F.NOT_OK, status=F.UNUSABLE)))


def test_the_ground_the_gpu_comparison_stands_on(derived):
    rows = derived["rows"]
    ok = [r for r in rows if r["status"] == F.OK]
    assert len(ok) >= 200
    assert sum(r["n_fragmentations"] == 0 for r in ok) >= 40
    assert sum(r["n_fragmentations"] > 0 and F.better(r["modified"], r["plain"]) for r in ok) >= 40
    assert sum(r["best_kind"] in (2, 3) for r in ok) >= 20
    assert sum(r["ring_step"] for r in ok) >= 20
    rr, rn = derived["ref"]
    molecules = {q.tobytes(): (q, k) for q, k in zip(rr, rn)}
    kinds = [{f[0] for f in F.Mol(q, k).fragmentations()} for q, k in molecules.values()]
    assert all(sum(kind in found for found in kinds) >= 20 for kind in range(4))


def test_the_budget_verdict_does_not_depend_on_where_the_enumeration_starts(table):
    rows, rec, n = table
    rng = np.random.default_rng(7)
    for name in ("cubane", "1-propylindane", "norbornane", "n-hexane"):
        k = [nm for nm, _, _ in rows].index(name)
        m = F.Mol(rec[k], n[k])
        ends = [(a, b) for a, b, _ in m.bonds]
        count = len(F.bond_sets(ends, F.MAX_NODES))
        assert count == m.fingerprint(F.DEFAULT_NODES).count
        for _ in range(4):
            roots = [int(e) for e in rng.permutation(len(ends))]
            assert sorted(map(sorted, F.bond_sets(ends, count, roots))) == sorted(map(sorted, F.bond_sets(ends, count)))
            with pytest.raises(F.Over):
                F.bond_sets(ends, count - 1, roots)
            relabel = [ends[int(e)] for e in rng.permutation(len(ends))]          # the bonds numbered otherwise: the same count
            assert len(F.bond_sets(relabel, F.MAX_NODES)) == count
        assert F.fragmentation_row(rec[k], n[k], count)["status"] == F.OK and F.fragmentation_row(rec[k], n[k], count - 1)["status"] == F.UNDECIDED
        row = F.similarity_pair((rec[k], n[k]), (rec[0], n[0]), count - 1)
        assert row == dict(F.NOT_OK, status=F.UNDECIDED)
    # every connected set once: a triangle has 3 + 3 + 1 sets, a chain of k bonds k + (k - 1) + ... down to sets of five
    assert len(F.bond_sets([(0, 1), (1, 2), (0, 2)], 100)) == 7 and len(F.bond_sets([(i, i + 1) for i in range(7)], 100)) == 7 + 6 + 5 + 4 + 3
    star = F.bond_sets([(0, k) for k in range(1, 7)], 100)                         # six bonds at one atom: every subset of 1..5
    assert len(star) == 6 + 15 + 20 + 15 + 6 and len(set(map(frozenset, star))) == len(star)


def test_the_hash_is_the_headers():
    # h = k, then mix2 over the ascending codes; propane: two C-C bonds; alone (C deg 1, C deg 1), together (C deg 1, C deg 2) twice
    alone, together = ((2 * 8 + 1) << 9) | ((2 * 8 + 1) << 2), ((2 * 8 + 1) << 9) | ((2 * 8 + 2) << 2)
    h1 = F.mix2(1, alone)
    h2 = F.mix2(F.mix2(2, together), together)
    want = 0
    for h in (h1, h2):
        want |= (1 << (h & 1023)) | (1 << ((h >> 32) & 1023))
    rec, n = SM.records([G.molecule("CCC", [(0, 1, 1), (1, 2, 1)], [3, 2, 3])])
    f = F.Mol(rec[0], n[0]).fingerprint(10)
    assert f.fp == want and f.count == 3 and f.atom_bits[1] == want and f.atom_bits[0] == f.atom_bits[2] == want
    assert F.mix2(0, 0) == F.fmix(0x9e3779b97f4a7c15)


# ------------------------------------------------------------------------------------------------------------------ the surface

def test_header_constants_and_prototypes():
    from diffspectra_amd import abi, engine as E
    c = abi.FRAGGLE.consts
    assert (c["DSF_OK"], c["DSF_UNDECIDED"], c["DSF_UNUSABLE"], c["DSF_INVALID"]) == (F.OK, F.UNDECIDED, F.UNUSABLE, F.INVALID)
    assert (c["DSF_MAX_NODES"], c["DSF_DEFAULT_NODES"], c["DSF_MAX_BONDS"], c["DSF_MAX_PATH"]) == (F.MAX_NODES, F.DEFAULT_NODES, F.MAX_BONDS, F.MAX_PATH)
    assert (c["DSF_FP_BITS"], c["DSF_FP_WORDS"]) == (F.FP_BITS, F.FP_WORDS) and c["DSF_FP_BITS"] == 32 * c["DSF_FP_WORDS"]
    assert (c["DSF_CODE_ATTACH"], c["DSF_CODE_WILD"], c["DSF_CODE_WILD_AROMATIC"]) == (F.CODE_ATTACH, F.CODE_WILD, F.CODE_WILD_AROMATIC)
    assert (c["DSF_NO_CUT"], c["DSF_MAX_FRAGMENTATIONS"], c["DSF_TRUNCATED"]) == (F.NO_CUT, F.MAX_FRAGMENTATIONS, F.TRUNCATED)
    assert c["DSF_WAVES"] >= 1 and c["DSF_CODE_ATTACH"] > 2 * 4 + 1, "the extra codes lie above (element, aromatic)"
    assert (E.FRAGGLE_OK, E.FRAGGLE_UNDECIDED, E.FRAGGLE_UNUSABLE, E.FRAGGLE_INVALID) == (F.OK, F.UNDECIDED, F.UNUSABLE, F.INVALID)
    assert (E.FRAGGLE_MAX_NODES, E.FRAGGLE_DEFAULT_NODES, E.FRAGGLE_MAX_FRAGMENTATIONS, E.FRAGGLE_TRUNCATED, E.FRAGGLE_NO_CUT, E.FRAGGLE_FP_WORDS) == \
        (F.MAX_NODES, F.DEFAULT_NODES, F.MAX_FRAGMENTATIONS, F.TRUNCATED, F.NO_CUT, F.FP_WORDS)
    assert abi.FRAGGLE.exports("dsf_") == ["dsf_fraggle_fragmentations", "dsf_path_fingerprints", "dsf_fraggle_similarity_records"]
    protos = abi.FRAGGLE.prototypes
    assert [t for _, t in protos["dsf_fraggle_fragmentations"].params] == ["*", "*", "int64_t", "int32_t"] + ["*"] * 4
    assert [t for _, t in protos["dsf_path_fingerprints"].params] == ["*", "*", "int64_t", "int32_t"] + ["*"] * 5
    assert [t for _, t in protos["dsf_fraggle_similarity_records"].params] == ["*", "*", "int64_t", "*", "*", "int64_t", "*", "int32_t"] + ["*"] * 7
    assert [nm for nm, _ in protos["dsf_fraggle_similarity_records"].params] == [
        "prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "max_nodes", "plain", "modified", "best_index", "n_fragmentations", "marked",
        "status", "stream"]


@pytest.mark.parametrize("call", ["fraggle_fragmentations", "path_fingerprints", "fraggle_similarity_records"])
def test_argument_errors_that_need_no_device(call):
    from diffspectra_amd import engine as E
    pairs = call == "fraggle_similarity_records"
    rec, n = torch.zeros(3, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)

    def fn(rec, n, max_nodes=None, **kw):
        return getattr(E, call)(rec, n, rec, n, max_nodes=max_nodes, **kw) if pairs else getattr(E, call)(rec, n, max_nodes)
    for bad in (0, -1, E.FRAGGLE_MAX_NODES + 1):
        with pytest.raises(ValueError, match="max_nodes"):
            fn(rec, n, bad)
    for bad in (True, 4.0, "7"):
        with pytest.raises(TypeError, match="max_nodes"):
            fn(rec, n, bad)
    with pytest.raises(TypeError, match="rec"):
        fn(rec.to(torch.int8), n)
    with pytest.raises(ValueError, match="rec"):
        fn(rec[:, :-1], n)
    with pytest.raises(TypeError, match="n must"):
        fn(rec, n.to(torch.int64))
    with pytest.raises(ValueError, match="n must"):
        fn(rec, n[:2])
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(E.RECORD_BYTES, 3, dtype=torch.uint8).t(), n)
    if pairs:
        with pytest.raises(TypeError, match="ref_index"):
            fn(rec, n, ref_index=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(ValueError, match="ref_index"):
            fn(rec, n, ref_index=torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="ground-truth row"):
            E.fraggle_similarity_records(rec, n, rec[:2], n[:2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(rec, n)


def test_topk_and_the_float_on_the_cpu():
    from diffspectra_amd import structure_metrics as S
    value = torch.tensor([0.5, float("nan"), 0.75, 0.25, 0.0, 1.0], dtype=torch.float64)
    status = torch.tensor([0, 2, 0, 0, 0, 1], dtype=torch.uint8)
    top = S.topk_fraggle(value, status, 3)
    assert top["best"].tolist() == [0.75, 0.25] and top["best_index"].tolist() == [2, 0] and float(top["mean_best"]) == 0.5
    with pytest.raises(ValueError, match="top_k"):
        S.topk_fraggle(value, status, 4)
