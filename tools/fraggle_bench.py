"""Time dsf_fraggle_similarity_records (Fraggle similarity of record pairs; csrc/ds_fraggle.hip), dsf_path_fingerprints and
dsf_fraggle_fragmentations beside dsq_match_records with a single pattern and dsb_brics_records on the same records, and beside the CPU
mirror.

    python tools/fraggle_bench.py [--pairs 10000] [--launches 20] [--mirror 200] [--out profiles/fraggle_bench.json]

Two tables: the derived pairs of tests/fraggle_mirror.py (ground truths of 3 to 28 atoms, a seventh of them without a fragmentation) tiled to
`pairs` rows, and a QM9-sized table - seeded random molecules of 9 heavy atoms drawn without hydrogens, each against itself with one atom
changed.  Prints one JSON line (and writes it to --out): the median, minimum and maximum time of one call of each binding (HIP events around
the call, after three warm-up calls; a call is one kernel launch and the allocation of its outputs), the similarity kernel once more at the
end so that a drift of the clocks shows, pairs per second from the medians, and the wall time of tests/fraggle_mirror.similarity_table on the
first `mirror` pairs as pairs per second.  There is no gate on any of these times.

Run it from the repository root: the molecules and the mirror are the test suite's own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E, smarts                              # noqa: E402
from tests import fraggle_mirror as F, structure_mirror as SM, valence_mirror as VM      # noqa: E402
from record_bench import kernel_ms                                           # noqa: E402  (this directory: the script's own)


def qm9_like(rng, heavy=9):
    """A random molecule of ``heavy`` C / N / O atoms without drawn hydrogens: a random tree with degrees within the valences, up to two
    ring closures, a few double bonds where both ends have room."""
    valence = {1: 4, 2: 3, 3: 2}
    while True:
        types = [int(t) for t in rng.choice([1, 1, 1, 1, 2, 3], size=heavy)]
        used, bonds = [0] * heavy, {}
        ok = True
        for b in range(1, heavy):
            room = [a for a in range(b) if used[a] < valence[types[a]] - (1 if a else 0)]
            if not room:
                ok = False
                break
            a = int(rng.choice(room))
            bonds[a, b] = 1
            used[a] += 1
            used[b] += 1
        if not ok:
            continue
        for _ in range(int(rng.integers(0, 3))):
            a, b = sorted(int(v) for v in rng.choice(heavy, size=2, replace=False))
            if (a, b) not in bonds and b - a > 1 and used[a] < valence[types[a]] and used[b] < valence[types[b]]:
                bonds[a, b] = 1
                used[a] += 1
                used[b] += 1
        for (a, b) in list(bonds):
            if rng.random() < 0.15 and used[a] < valence[types[a]] and used[b] < valence[types[b]]:
                bonds[a, b] = 2
                used[a] += 1
                used[b] += 1
        return VM.molecule(types, [(a, b, o) for (a, b), o in bonds.items()])


def changed(mol, rng):
    out = dict(mol, type=np.asarray(mol["type"]).copy())
    leaves = [i for i in range(len(out["type"])) if (np.asarray(mol["bond"])[i] > 0).sum() == 1]
    a = int(rng.choice(leaves))
    out["type"][a] = 3 if out["type"][a] != 3 else 1
    return out


def time_table(name, prb, ref, a, out, dev):
    rows = np.arange(a.pairs) % len(prb[1])
    prb_d = [torch.as_tensor(x[rows]).to(dev) for x in prb]
    ref_d = [torch.as_tensor(x[rows]).to(dev) for x in ref]
    one_pattern = torch.as_tensor(np.asarray(smarts.compile_patterns(["[#6]-[#8]"]), dtype=np.int32)).to(dev)
    t = {}
    t["fraggle_similarity_records_ms"] = kernel_ms(E.fraggle_similarity_records, (*prb_d, *ref_d), a.launches)
    t["path_fingerprints_ms"] = kernel_ms(E.path_fingerprints, tuple(ref_d), a.launches)
    t["fraggle_fragmentations_ms"] = kernel_ms(E.fraggle_fragmentations, tuple(ref_d), a.launches)
    t["match_records_one_pattern_ms"] = kernel_ms(E.substructure_records, (*ref_d, one_pattern), a.launches)
    t["brics_records_ms"] = kernel_ms(E.brics_records, tuple(ref_d), a.launches)
    t["fraggle_similarity_records_ms_again"] = kernel_ms(E.fraggle_similarity_records, (*prb_d, *ref_d), a.launches)
    for key in ("fraggle_similarity_records_ms", "match_records_one_pattern_ms", "brics_records_ms"):
        t[key.replace("_ms", "_per_s")] = a.pairs / (t[key]["median"] * 1e-3)
    found = E.fraggle_similarity_records(*prb_d, *ref_d)
    t["distinct_pairs"] = int(len(prb[1]))
    t["mean_atoms"] = float(ref[1][rows].mean())
    t["mean_fragmentations"] = float(found[3].double().mean())
    t["ok_pairs"] = int((found[5] == 0).sum())
    if a.mirror:
        k = min(a.mirror, len(prb[1]))
        t0 = time.time()
        want = F.as_arrays(F.similarity_table(prb[0][:k], prb[1][:k], ref[0][:k], ref[1][:k]))
        t["mirror_pairs"] = k
        t["mirror_pairs_per_s"] = k / (time.time() - t0)
        got = [x[:k].cpu().numpy() for x in found]
        t["mirror_rows_equal"] = int(np.all([(g == w).reshape(k, -1).all(1) for g, w in zip(got, want)], axis=0).sum())
    out[name] = t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mirror", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    dev = torch.device("cuda:0")
    out = {"pairs": a.pairs, "launches": a.launches}
    prb, ref = F.derived_pairs()
    time_table("derived", SM.records(prb), SM.records(ref), a, out, dev)
    rng = np.random.default_rng(9)
    mols = [qm9_like(rng) for _ in range(500)]
    time_table("qm9_sized", SM.records([changed(m, rng) for m in mols]), SM.records(mols), a, out, dev)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
