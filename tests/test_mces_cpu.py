"""CPU: the C-ABI surface of the MCES distance and its argument checks, the two yardsticks of tests/mces_mirror.py against each other and
against graphs whose answer is known, and the Top-K reduction.  (The kernel is checked on the GPU against the same mirror:
tests/test_mces_gpu.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from tests import graph_mirror as GM, mces_mirror as MM


def test_header_declares_and_library_exports_mces():
    import __graft_entry__ as g
    g.build()
    lib = E.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(E.HEADER_PATH).read(), flags=re.S)
    assert "ds_mces_records" in E.EXPORTS and hasattr(lib, "ds_mces_records")
    args = re.search(r"int\s+ds_mces_records\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "drop_h", "max_nodes",
                                                                    "dist", "lower", "status", "nodes", "map", "stream"]
    assert (E.MCES_EXACT, E.MCES_UNDECIDED, E.MCES_INVALID) == (0, 2, 3) and E.MCES_MAX_NODES == 1 << 22
    null = C.c_void_p(None)
    call = lambda drop_h, max_nodes, P=0: lib.ds_mces_records(null, null, C.c_int64(P), null, null, C.c_int64(0), null, C.c_int32(drop_h),
                                                              C.c_int32(max_nodes), null, null, null, null, null, null)
    assert call(1, 0) == 0 and call(0, 1 << 22) == 0                   # P = 0 launches nothing
    for bad in (-1, (1 << 22) + 1):
        assert call(1, bad) == -1                                      # DS_ERR_ARG before anything else: no device is touched
    for bad in (-1, 2):
        assert call(bad, 16) == -1
    assert call(1, 16, P=-1) == -1


def test_mces_functions_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec = torch.zeros(4, shard.RECORD_BYTES, dtype=torch.uint8)
    n = torch.full((4,), 3, dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int64)
    for fn in (E.mces_records, E.DmtEngine.mces_records.__get__(object())):
        with pytest.raises(TypeError, match="prb_rec"):
            fn(rec.float(), n, rec, n)
        with pytest.raises(TypeError, match="prb_n"):
            fn(rec, n.long(), rec, n)
        with pytest.raises(TypeError, match="ref_n"):
            fn(rec, n, rec, n.long())
        with pytest.raises(TypeError, match="ref_index"):
            fn(rec, n, rec, n, idx.int())
        with pytest.raises(ValueError, match="ref_rec"):
            fn(rec, n, rec[:, :1247].contiguous(), n)
        with pytest.raises(ValueError, match="prb_n"):
            fn(rec, n[:3], rec, n)
        with pytest.raises(ValueError, match="ref_index"):
            fn(rec, n, rec, n, idx[:2])
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(shard.RECORD_BYTES, 4, dtype=torch.uint8).t(), n, rec, n)
        with pytest.raises(ValueError, match="rows"):
            fn(rec, n, rec[:2], n[:2])
        for bad in (-1, (1 << 22) + 1):
            with pytest.raises(ValueError, match="max_nodes"):
                fn(rec, n, rec, n, None, True, bad)
        with pytest.raises(TypeError, match="max_nodes"):
            fn(rec, n, rec, n, None, True, 16.0)
        with pytest.raises(TypeError, match="drop_h"):
            fn(rec, n, rec, n, None, 1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(rec, n, rec, n, idx)
    from diffspectra_amd.structure_metrics import mces_batch
    with pytest.raises(RuntimeError, match="no CPU path"):
        mces_batch((rec, n), (rec, n))


# ------------------------------------------------------------------------------------------------------------------ the mirror

SMALL = dict(count=300, seed=20261103, heavy=(1, 6))


def test_milp_agrees_with_enumeration_on_small_seeded_pairs():
    ref, prb, kind = MM.seeded_pairs(**SMALL)
    assert len(ref) == 300 and max(int((m["type"] != 0).sum()) for m in ref + prb) <= 6
    milp = MM.seeded_distances(**SMALL)
    brute = np.array([MM.mces_exhaustive(a, b) for a, b in zip(prb, ref)])
    assert np.array_equal(milp, brute), np.nonzero(milp != brute)[0][:10]
    assert (milp[kind == 0] == 0).all() and (milp > 0).sum() > 100      # the set discriminates
    few = [p for p in range(300) if len(ref[p]["type"]) <= 7 and len(prb[p]["type"]) <= 7][:40]
    assert len(few) >= 20
    for p in few:                                                       # with the hydrogens kept
        assert MM.mces_milp(prb[p], ref[p], False) == MM.mces_exhaustive(prb[p], ref[p], False), p


def test_hand_table():
    for name, a, b, want in MM.hand_table():
        for drop_h in (True, False):
            assert MM.mces_milp(a, b, drop_h) == want == MM.mces_exhaustive(a, b, drop_h), name
            assert MM.mces_milp(b, a, drop_h) == want, name
    # with its hydrogens methane has four bonds and water two, and nothing in common: 6 apart once they count, 0 on the heavy atoms
    methane, water = GM.molecule([1, 0, 0, 0, 0], [(0, k) for k in range(1, 5)]), GM.molecule([3, 0, 0], [(0, 1), (0, 2)])
    assert MM.mces_milp(methane, water, True) == 0 and MM.mces_milp(methane, water, False) == 6 == MM.mces_exhaustive(methane, water, False)


def test_symmetry():
    ref, prb, _ = MM.seeded_pairs(**SMALL)
    forward = MM.seeded_distances(**SMALL)
    assert np.array_equal(forward, [MM.mces_milp(b, a) for a, b in zip(prb, ref)])


def _stripped(mol, bonded_only):
    """The heavy atoms with their charges zeroed; ``bonded_only`` also sets aside the heavy atoms without a bond to another heavy atom."""
    t, w, keep = MM.kept_graph(mol, True)
    sel = np.nonzero(w.sum(1) > 0)[0] if bonded_only else np.arange(len(t))
    return dict(pos=np.zeros((len(sel), 3)), type=t[sel], fc=np.zeros(len(sel), np.int64), bond=w[np.ix_(sel, sel)])


def test_zero_distance_is_graph_identity():
    """dist = 0 exactly when graph_mirror.same_graph holds on the hydrogen-stripped, charge-zeroed molecules.  One amendment the definition
    forces: an atom without a bond has no edge to lose (the hand table's methane / water is 0), so where a side has such atoms the comparison
    sets them aside; on every pair without them the statement is checked as it stands."""
    ref, prb, _ = MM.seeded_pairs()
    dist = MM.seeded_distances()
    plain = 0
    for p, (a, b) in enumerate(zip(prb, ref)):
        charged = dict(a, fc=np.where(np.arange(len(a["fc"])) % 2 == 0, 1, -1))       # the charge byte is not compared
        assert GM.same_graph(_stripped(charged, True), _stripped(b, True)) == (dist[p] == 0), p
        whole_a, whole_b = _stripped(a, False), _stripped(b, False)
        if len(whole_a["type"]) == len(_stripped(a, True)["type"]) and len(whole_b["type"]) == len(_stripped(b, True)["type"]):
            plain += 1
            assert GM.same_graph(whole_a, whole_b) == (dist[p] == 0), p
    assert plain > 500 and 100 < int((dist == 0).sum()) < 400


def test_score_of_map_refuses_bad_maps():
    name, a, b, want = MM.hand_table()[2]                               # ethanol C C O / dimethyl ether C O C
    assert MM.score_of_map(a, b, [0, -1, -1]) == 0 and MM.score_of_map(a, b, [-1, 0, 1]) == 1
    for bad in ([0, 0, -1], [1, -1, -1], [0, 2, 5]):
        with pytest.raises((AssertionError, IndexError, KeyError)):
            MM.score_of_map(a, b, bad)


# ------------------------------------------------------------------------------------------------------------------ Top-K

def test_topk_mces():
    from diffspectra_amd.structure_metrics import Mces, topk_mces
    dist = torch.tensor([4, 0, 0,   7, 3, 5,   9, 9, 2,   -1, -1, -1,   -1, 6, 6], dtype=torch.int32)
    status = torch.tensor([0, 0, 0,   2, 2, 2,   0, 2, 0,   3, 3, 3,   3, 2, 0], dtype=torch.uint8)
    s = topk_mces(dist, status, 3)
    assert s["best"].tolist() == [0, 3, 2, -1, 6] and s["best_index"].tolist() == [1, 1, 2, -1, 1]
    assert float(s["mean_best"]) == (0 + 3 + 2 + 6) / 4 and int(s["undecided"]) == 5      # an all-undecided group keeps its upper bounds
    one = topk_mces(dist, status, 1)
    assert one["best"].tolist() == dist.tolist() and one["best_index"].tolist() == [0 if v != 3 else -1 for v in status.tolist()]
    assert float(one["mean_best"]) == float(dist[status != 3].double().mean())
    for bad in (0, -1, 4):
        with pytest.raises(ValueError):
            topk_mces(dist, status, bad)
    with pytest.raises(ValueError):
        topk_mces(dist, status[:6], 3)
    empty = topk_mces(dist[:0], status[:0], 3)
    assert empty["best"].shape == (0,) and int(empty["undecided"]) == 0 and float(empty["mean_best"]) != float(empty["mean_best"])
    m = Mces(dist, dist, status, torch.zeros(15, dtype=torch.int32), torch.full((15, 29), -1, dtype=torch.int32))
    assert m.exact.tolist() == (status == 0).tolist() and m.undecided.tolist() == (status == 2).tolist()
