"""CPU: the C-ABI surface of graph identity and the graph hash, their argument checks, the Python mirror on graphs whose answer is known
(and against networkx where it exists), and the Top-K reduction.  (The kernels are checked on the GPU against the same mirror:
tests/test_graph_identity_gpu.py.)"""
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from tests import graph_mirror as GM, structure_mirror as SM


def test_header_declares_and_library_exports_graph_entry_points():
    import __graft_entry__ as g
    g.build()
    lib = E.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(E.HEADER_PATH).read(), flags=re.S)
    for name, names in (("ds_graph_identity_records", ["prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "max_nodes", "verdict", "nodes",
                                                       "map", "stream"]),
                        ("ds_graph_hash_records", ["rec", "n", "P", "hash", "stream"])):
        assert name in E.EXPORTS and hasattr(lib, name)
        args = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
    assert (E.GRAPH_DIFFERENT, E.GRAPH_IDENTICAL, E.GRAPH_UNDECIDED, E.GRAPH_INVALID) == (0, 1, 2, 3) and E.GRAPH_MAX_NODES == 1 << 20
    # the C entry points refuse a budget outside [0, 1 << 20] before anything else (no device is touched: status DS_ERR_ARG = -1)
    import ctypes as C
    null = C.c_void_p(None)
    for bad in (-1, (1 << 20) + 1):
        assert lib.ds_graph_identity_records(null, null, C.c_int64(0), null, null, C.c_int64(0), null, C.c_int32(bad), null, null, null, null) == -1
    assert lib.ds_graph_identity_records(null, null, C.c_int64(0), null, null, C.c_int64(0), null, C.c_int32(0), null, null, null, null) == 0
    assert lib.ds_graph_hash_records(null, null, C.c_int64(0), null, null) == 0 and lib.ds_graph_hash_records(null, null, C.c_int64(-1), null, null) == -1


def test_graph_functions_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec = torch.zeros(4, shard.RECORD_BYTES, dtype=torch.uint8)
    n = torch.full((4,), 3, dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int64)
    for fn in (E.graph_identity_records, E.DmtEngine.graph_identity_records.__get__(object())):
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
        for bad in (-1, (1 << 20) + 1):
            with pytest.raises(ValueError, match="max_nodes"):
                fn(rec, n, rec, n, None, bad)
        with pytest.raises(TypeError, match="max_nodes"):
            fn(rec, n, rec, n, None, 16.0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(rec, n, rec, n, idx)
    for fn in (E.graph_hash_records, E.DmtEngine.graph_hash_records.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            fn(rec.float(), n)
        with pytest.raises(TypeError, match="n must"):
            fn(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            fn(rec[:, :1247].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            fn(rec, n[:3])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(rec, n)
    from diffspectra_amd.structure_metrics import graph_classes, graph_identity_batch
    with pytest.raises(RuntimeError, match="no CPU path"):
        graph_identity_batch((rec, n), (rec, n))
    with pytest.raises(RuntimeError, match="no CPU path"):
        graph_classes(rec, n)


# ------------------------------------------------------------------------------------------------------------------ the mirror

def test_mirror_answers_the_hard_pairs():
    rng = np.random.default_rng(4)
    for name, a, b in GM.hard_pairs():
        assert sorted((a["bond"] > 0).sum(1)) == sorted((b["bond"] > 0).sum(1)), name        # equal degree sequences: nothing cheap separates them
        assert not GM.same_graph(a, b) and not GM.same_graph(b, a), name
        for m in (a, b):
            moved = GM.permuted(m, rng)
            ok, image = GM.same_graph(moved, m, want_map=True)
            assert ok and GM.is_isomorphism(moved, m, image), name
            assert not GM.is_isomorphism(moved, b if m is a else a, image), name
        assert GM.graph_hash(a) == GM.graph_hash(b), name                                    # colour refinement cannot tell them apart
    k29 = GM.carbons(29, [(i, j) for i in range(29) for j in range(i + 1, 29)])
    none = GM.carbons(29, [])
    c9 = GM.nonane()
    assert len(c9["type"]) == 29 and int((c9["type"] == 0).sum()) == 20
    for m in (k29, none, c9):
        assert GM.same_graph(GM.permuted(m, rng), m)
    assert not GM.same_graph(k29, none) and not GM.same_graph(GM.carbons(28, []), none)
    charged = dict(c9, fc=c9["fc"].copy())
    charged["fc"][3] = -1
    assert not GM.same_graph(charged, c9) and GM.graph_hash(charged) != GM.graph_hash(c9)
    empty = GM.molecule([], [])
    assert GM.same_graph(empty, empty, want_map=True) == (True, []) and GM.graph_hash(empty) == GM.mix(0, 0)


def test_mirror_agrees_with_networkx_on_the_seeded_pairs():
    nx = pytest.importorskip("networkx")
    ref, prb, kind = GM.seeded_pairs()
    mine = GM.seeded_labels()

    def graph(m):
        g = nx.Graph()
        for i in range(len(m["type"])):
            g.add_node(i, label=(int(m["type"][i]), int(m["fc"][i])))
        for i, j in np.argwhere(np.triu(m["bond"], 1) > 0):
            g.add_edge(int(i), int(j), order=int(m["bond"][i, j]))
        return g
    theirs = np.array([nx.is_isomorphic(graph(a), graph(b), node_match=lambda x, y: x["label"] == y["label"],
                                        edge_match=lambda x, y: x["order"] == y["order"]) for a, b in zip(prb, ref)])
    assert np.array_equal(mine, theirs), np.nonzero(mine != theirs)[0][:10]
    for name, a, b in GM.hard_pairs():
        assert not nx.is_isomorphic(graph(a), graph(b)), name


def test_seeded_pairs_discriminate_and_records_match_the_packer():
    ref, prb, kind = GM.seeded_pairs()
    same = GM.seeded_labels()
    assert same[kind == 0].all()
    for k in (1, 3):                                                  # the bond switch and the type swap leave both answers well populated
        share = same[kind == k].mean()
        assert 0.05 <= share <= 0.95, (k, share)
    rec, n = SM.records(ref[:40] + prb[:40])
    for k, m in enumerate(ref[:40] + prb[:40]):
        assert np.array_equal(rec[k], SM.record_from_mol(m["pos"], m["type"], m["fc"], m["bond"])) and n[k] == len(m["type"])
        back = SM.mol_from_record(rec[k], n[k])
        assert GM.same_graph(back, m) and GM.graph_hash(back) == GM.graph_hash(m)


def test_mirror_hash_is_permutation_invariant():
    ref, prb, kind = GM.seeded_pairs()
    hits = 0
    for a, b, s in list(zip(prb, ref, GM.seeded_labels()))[:200]:
        if s:
            assert GM.graph_hash(a) == GM.graph_hash(b)
        hits += GM.graph_hash(a) == GM.graph_hash(b)
    assert hits < 200                                                 # and it does tell most different graphs apart


# ------------------------------------------------------------------------------------------------------------------ Top-K

def test_topk_identity():
    from diffspectra_amd.structure_metrics import GraphIdentity, topk_identity
    verdict = torch.tensor([0, 1, 1,   0, 0, 0,   2, 0, 0,   0, 2, 1], dtype=torch.uint8)
    s = topk_identity(verdict, 3)
    assert s["hit"].tolist() == [True, False, False, True] and s["first_hit"].tolist() == [1, -1, -1, 2]
    assert float(s["acc_at_k"]) == 0.5 and int(s["undecided"]) == 2                           # an undecided pair is a miss, and is reported
    one = topk_identity(verdict, 1)
    assert one["hit"].tolist() == (verdict == 1).tolist() and float(one["acc_at_k"]) == 3 / 12
    assert one["first_hit"].tolist() == [0 if v == 1 else -1 for v in verdict.tolist()]
    with pytest.raises(ValueError):
        topk_identity(verdict, 5)                                     # a ragged size
    with pytest.raises(ValueError):
        topk_identity(verdict, 0)
    empty = topk_identity(verdict[:0], 3)
    assert empty["hit"].shape == (0,) and float(empty["acc_at_k"]) == 0.0 and int(empty["undecided"]) == 0
    g = GraphIdentity(verdict, torch.zeros(12, dtype=torch.int32), torch.full((12, 29), -1, dtype=torch.int32))
    assert g.identical.tolist() == (verdict == 1).tolist() and g.undecided.tolist() == (verdict == 2).tolist()
