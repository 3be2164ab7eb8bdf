"""GPU: the ORDER of the pair search (csrc/ds_refine.h, run by ``k_graph_identity`` and ``k_stereo_identity``) pinned bit for bit.  The mirrors
decide verdicts and check that a map is an isomorphism; they say nothing about which isomorphism is met first or how many nodes that took.
``tests/golden/pair_search_parent.npz`` holds every output of both entry points - verdict, nodes, map, and found and sites for stereo - as the
commit before the search moved into ds_refine.h computed them, on inputs that reach depth >= 2 with backtracking, 29 open levels, a budget
that ends in the middle of a level and enumeration past the first leaf.  Integers only: equality, no tolerance.

Recording (on a GPU, from a built library; only when the search order is MEANT to change): ``python -m tests.test_pair_search_pinned_gpu [PATH]``."""
import hashlib
import os

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E
from diffspectra_amd.structure_metrics import GraphIdentity, StereoIdentity
from tests import graph_mirror as GM, stereo_mirror as K, structure_mirror as SM
from tests.helpers import run_records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_search_parent.npz")
ENTRY = {"graph": (E.graph_identity_records, GraphIdentity), "stereo": (E.stereo_identity_records, StereoIdentity)}


def _sets():
    """[(name, entry, ground truths, generated molecules, scalars)] - built the same way every time, the generators seeded."""
    sets = []
    ref, prb, _ = GM.seeded_pairs()
    sets.append(("graph.seeded", "graph", list(ref[:400]), list(prb[:400]), {}))
    rng = np.random.default_rng(8)                                        # the cross and self pairs of test_graph_identity_gpu.test_hard_pairs
    hard = GM.hard_pairs()
    cross_prb = [GM.permuted(a, rng) for _, a, b in hard] + [GM.permuted(b, rng) for _, a, b in hard]
    cross_ref = [b for _, a, b in hard] + [a for _, a, b in hard]
    own = [m for _, a, b in hard for m in (a, b)] + [GM.k29(), GM.carbons(29, []), GM.nonane()]
    moved = [GM.permuted(m, rng) for m in own]
    for tag, kw in (("default", {}), ("0", dict(max_nodes=0)), ("1", dict(max_nodes=1)), ("64", dict(max_nodes=64))):
        sets.append((f"graph.cross.{tag}", "graph", cross_ref, cross_prb, kw))
        sets.append((f"graph.self.{tag}", "graph", own, moved, kw))
    table = K.hand_table()
    s_prb, s_ref, _ = K.seeded_pairs()
    rng = np.random.default_rng(32)
    cube, k29 = K.cubane(), GM.k29()
    turned, shuffled = K.renumbered(cube, rng), GM.permuted(k29, rng)
    for exhaustive in (0, 1):
        sets.append((f"stereo.hand.{exhaustive}", "stereo", [t[2] for t in table], [t[1] for t in table], dict(exhaustive=bool(exhaustive))))
        sets.append((f"stereo.seeded.{exhaustive}", "stereo", list(s_ref[:100]), list(s_prb[:100]), dict(exhaustive=bool(exhaustive))))
        sets.append((f"stereo.cubane.{exhaustive}", "stereo", [cube], [turned], dict(exhaustive=bool(exhaustive))))
        sets.append((f"stereo.k29.64.{exhaustive}", "stereo", [k29], [shuffled], dict(max_nodes=64, exhaustive=bool(exhaustive))))
    return sets


def _compute(dev):
    """{"<set>.<output>": array} of every set, and "inputs" = the SHA-1 of every record and atom count that went in."""
    out, digest = {}, hashlib.sha1()
    for name, entry, ref, prb, kw in _sets():
        packed = SM.records(ref), SM.records(prb)
        for rec, n in packed:
            digest.update(np.ascontiguousarray(rec).tobytes() + np.ascontiguousarray(n).tobytes())
        fn, result_type = ENTRY[entry]
        got = run_records(fn, result_type, dev, *packed, **kw)
        for field, value in zip(result_type._fields, got):
            out[f"{name}.{field}"] = value
    out["inputs"] = np.frombuffer(digest.digest(), np.uint8)
    return out


def test_search_order_is_the_parents(gpu_device):
    want = np.load(GOLDEN)
    got = _compute(gpu_device)
    assert sorted(got) == sorted(want.files)
    assert got["inputs"].tobytes() == want["inputs"].tobytes(), "the generators built other inputs than were recorded: nothing is compared"
    nodes = {k[:-len(".nodes")]: int(v.sum()) for k, v in got.items() if k.endswith(".nodes")}
    print(f"[pinned] {len(got) - 1} arrays of {len(nodes)} sets; search nodes per set {nodes}")
    # what the sets are there to reach
    assert got["graph.self.default.nodes"][-3] >= 28 and got["graph.seeded.nodes"].max() >= 2             # 29 open levels; depth >= 2
    assert (got["graph.self.1.verdict"] == 2).any() and got["stereo.k29.64.1.nodes"].tolist() == [64]      # a budget that ends mid-level
    assert got["stereo.cubane.1.found"].tolist() == [[48, 24, 24]]                                         # enumeration past the first leaf
    for key in want.files:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), (key, np.argwhere(got[key] != want[key])[:5].tolist())


if __name__ == "__main__":
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(path, **_compute(torch.device("cuda:0")))
    print(f"recorded {path}: {os.path.getsize(path)} bytes")
