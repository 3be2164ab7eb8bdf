"""GPU: the ORDER of the pair search (csrc/ds_refine.h, run by ``k_graph_identity`` and ``k_stereo_identity``) pinned bit for bit.  The mirrors
decide verdicts and check that a map is an isomorphism; they say nothing about which isomorphism is met first or how many nodes that took.
``tests/golden/pair_search_parent.npz`` holds every output of both entry points - verdict, nodes, map, and found and sites for stereo - as the
commit before the search moved into ds_refine.h computed them, on inputs that reach depth >= 2 with backtracking, 29 open levels, a budget
that ends in the middle of a level and enumeration past the first leaf.  Integers only: equality, no tolerance.

``tests/golden/site_search_parent.npz`` does the same for the key level (``k_key_sites``, ``k_key_identity``) and ``k_stereo_sites``: see below.

Recording (on a GPU, from a built library; only when the search order is MEANT to change): ``python -m tests.test_pair_search_pinned_gpu [PATH]``."""
import hashlib
import os

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E
from diffspectra_amd.structure_metrics import GraphIdentity, StereoIdentity
from tests import graph_mirror as GM, key_mirror as KM, stereo_mirror as K, structure_mirror as SM
from tests.helpers import run_records, to_dev

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


# ------------------------------------------------------------------------------------------------------------------ the site kernels
# The key level (csrc/ds_key.hip) and the fp64 site geometry of both levels, pinned the same way before the search, the leaf test and the
# geometry moved into csrc/ds_sites.h.  Recording: ``python -m tests.test_pair_search_pinned_gpu --sites [PATH]``.

SITE_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "site_search_parent.npz")
HAND = 51                                 # the hand pairs and the pairs of the stereo table stand first
KEY_SITES = ("site", "masks", "volume", "nodes", "status")
KEY_PAIRS = ("verdict", "nodes", "found", "sites", "map")
STEREO_SITES = ("masks", "volume", "status")


def _site_table():
    """(generated molecules, ground truths) of the ``table`` fixture of tests/test_key_identity_gpu.py, built the same way, without the mirror."""
    mols = KM.hand_molecules()
    prb = [mols[a] for a, _, _, _ in KM.hand_pairs()] + [a for _, a, _, _ in KM.stereo_table_pairs()]
    ref = [mols[b] for _, b, _, _ in KM.hand_pairs()] + [b for _, _, b, _ in KM.stereo_table_pairs()]
    assert len(prb) == HAND
    a, b, _ = KM.law2_pairs()
    prb, ref = prb + list(a), ref + list(b)
    for i, (_, _, m, s) in enumerate(KM.shifted_forms()):
        prb, ref = prb + [s] + ([KM.reflected(s)] if i % 3 == 0 else []), ref + [m] + ([m] if i % 3 == 0 else [])
    a, b, _ = K.seeded_pairs(K.SEEDS[:1])
    return prb + list(a), ref + list(b)


def _compute_sites(dev):
    """{"<set>.<output>": array} of the key-level and stereo-level site kernels and of the key-level pair search; "inputs" = the SHA-1 of every
    record and atom count that went in, "forms" = that of the normal forms the pair search ran on (csrc/ds_mobile.hip: not what is pinned)."""
    prb, ref = _site_table()
    distinct, seen = [], set()
    for m in prb + ref:
        if id(m) not in seen:
            seen.add(id(m))
            distinct.append(m)
    out, digest, forms_digest = {}, hashlib.sha1(), hashlib.sha1()
    packed = [SM.records(x) for x in (prb, ref, distinct)]
    for rec, n in packed:
        digest.update(np.ascontiguousarray(rec).tobytes() + np.ascontiguousarray(n).tobytes())
    (p_rec, p_n), (r_rec, r_n), (d_rec, d_n) = ((to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)) for rec, n in packed)
    for tag, budget in (("default", None), ("1", 1)):
        for field, value in zip(KEY_SITES, E.key_sites(d_rec, d_n, budget)):
            out[f"key.sites.{tag}.{field}"] = value.cpu().numpy()
    for field, value in zip(STEREO_SITES, E.stereo_sites(d_rec, d_n)):
        out[f"stereo.sites.{field}"] = value.cpu().numpy()
    p_form, r_form = E.normal_records(p_rec, p_n), E.normal_records(r_rec, r_n)
    for t in (*p_form, *r_form):
        forms_digest.update(t.cpu().numpy().tobytes())
    p_site, r_site = E.key_sites(p_rec, p_n)[0], E.key_sites(r_rec, r_n)[0]
    out["key.pairs.prb_site"] = p_site.cpu().numpy()

    def pairs(rows, max_nodes, exhaustive):
        s = slice(0, rows)
        return E.key_identity_records(p_form[0][s], p_form[1][s], p_site[s], r_form[0][s], r_form[1][s], r_site[s], None, max_nodes, exhaustive)
    for exhaustive in (0, 1):
        for field, value in zip(KEY_PAIRS, pairs(len(prb), 4096, bool(exhaustive))):
            out[f"key.pairs.{exhaustive}.{field}"] = value.cpu().numpy()
    for budget in (0, 1, 3):
        for field, value in zip(KEY_PAIRS, pairs(HAND, budget, True)):
            out[f"key.hand.{budget}.1.{field}"] = value.cpu().numpy()
    torch.cuda.synchronize()
    out["inputs"] = np.frombuffer(digest.digest(), np.uint8)
    out["forms"] = np.frombuffer(forms_digest.digest(), np.uint8)
    return out


def test_site_search_is_the_parents(gpu_device):
    want = np.load(SITE_GOLDEN)
    got = _compute_sites(gpu_device)
    assert sorted(got) == sorted(want.files)
    assert got["inputs"].tobytes() == want["inputs"].tobytes(), "the generators built other inputs than were recorded: nothing is compared"
    assert got["forms"].tobytes() == want["forms"].tobytes(), "the normal forms are not the recorded ones: the pair search ran on other records"
    assert got["key.pairs.1.verdict"].shape == (483,) and got["key.sites.default.status"].shape == (648,) and not got["key.sites.default.status"].any()
    # what the sets are there to reach
    verdict, found = got["key.pairs.1.verdict"], got["key.pairs.1.found"]
    assert np.bincount(verdict, minlength=7).tolist() == [33, 321, 0, 0, 9, 12, 108]                       # what the mirror says of these pairs
    assert all((verdict == v).any() for v in (4, 5, 6))                                                     # mirror, stereoisomer, unassigned
    assert (found[:, 0] > found[:, 1] + found[:, 2]).any() and found[:, 0].max() == 48                     # isomorphisms of neither kind; enumeration
    assert any((got[f"key.hand.{b}.1.verdict"] == 2).any() for b in (0, 1, 3))                              # a budget that ends the search
    flags = got["key.pairs.prb_site"][:, :, 0]
    assert ((flags & KM.HSLOT != 0) & (flags & 3 != 0)).any(1)[got["key.pairs.0.verdict"] == 1].any()       # a site on a hydrogen slot, in an identical pair
    worst = 0.0
    for key in want.files:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if key.endswith(".volume"):                                       # fp64: NaN where the parent has NaN, and within 1e-12 of it elsewhere
            nan = np.isnan(want[key])
            assert (np.isnan(got[key]) == nan).all(), key
            diff = float(np.abs(np.where(nan, 0.0, got[key] - want[key])).max())
            print(f"[pinned] {key}: max |V - parent| {diff:.3e}")
            worst = max(worst, diff)
        else:
            assert got[key].tobytes() == want[key].tobytes(), (key, np.argwhere(got[key] != want[key])[:5].tolist())
    print(f"[pinned] {len(want.files) - 2} arrays; key-level search nodes {int(got['key.pairs.1.nodes'].sum())} exhaustive, "
          f"{int(got['key.pairs.0.nodes'].sum())} to the first same map; max |V - parent| {worst:.3e}")
    assert worst <= 1e-12


if __name__ == "__main__":
    import sys
    argv = [a for a in sys.argv[1:] if a != "--sites"]
    sites = len(argv) != len(sys.argv) - 1
    path = argv[0] if argv else SITE_GOLDEN if sites else GOLDEN
    np.savez_compressed(path, **(_compute_sites if sites else _compute)(torch.device("cuda:0")))
    print(f"recorded {path}: {os.path.getsize(path)} bytes")
