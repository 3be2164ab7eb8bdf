"""Time ds_morgan_records and ds_morgan_similarity_records (Morgan fingerprints, csrc/ds_morgan.hip) on the evaluation-like mix of
tools/graph_bench.py, beside ds_graph_hash_records on the same records in the same session, and the CPU mirror.

    python tools/morgan_bench.py [--pairs 10000] [--launches 20] [--mirror-pairs 1000] [--out profiles/morgan_bench.json]

The pairs: ground truths of tests/graph_mirror.random_molecule at the QM9 size mix; one third of the generated molecules are the ground
truth under another atom order (identical), the rest carry a degree-preserving bond switch on top.  Prints one JSON line (and writes it to
--out): the median kernel time (HIP events around one launch, after warm-up) of the fingerprint kernel and of the similarity kernel at
radius 2, hydrogens dropped and kept, and of the hash kernel, for `pairs` and 10 x `pairs` pairs (the same records tiled); the mean feature
count and the mean Tanimoto similarity; and the host time of tests/morgan_mirror.similarity_counts on the first `mirror-pairs` pairs with
how many of them the kernel's counts equal.  Compare with one denoise iteration of the same number of molecules: bench.py's samples /
(value * denoise_steps) seconds.

Run it from the repository root: the pair generator and the mirror are the test suite's own (tests/graph_mirror.py, tests/morgan_mirror.py)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E                      # noqa: E402
from diffspectra_amd.structure_metrics import MorganSimilarity   # noqa: E402
from tests import graph_mirror as GM, morgan_mirror as FM, structure_mirror as SM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mirror-pairs", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(7)
    sizes = qm9_sizes(rng, a.pairs)
    t0 = time.time()
    ref, prb, _ = GM.seeded_pairs(a.pairs, 20261018, sizes=tuple(int(s) for s in sizes), kinds=(0, 1, 1))
    (ref_rec, ref_n), (prb_rec, prb_n) = SM.records(ref), SM.records(prb)
    gen_s = time.time() - t0
    dev = torch.device("cuda:0")
    t = lambda x, rep=1: torch.as_tensor(np.tile(x, (rep,) + (1,) * (x.ndim - 1))).to(dev)
    out = {"pairs": a.pairs, "mean_atoms": float(sizes.mean()), "mean_heavy_atoms": float(np.mean([(m["type"] != 0).sum() for m in ref])),
           "generate_s": gen_s, "launches": a.launches, "radius": 2, "n_bits": 2048}
    for rep in (1, 10):
        args = (t(prb_rec, rep), t(prb_n, rep), t(ref_rec, rep), t(ref_n, rep))
        for drop_h in (True, False):
            tag = f"drop_h{int(drop_h)}_{a.pairs * rep}"
            out["features_ms_" + tag] = kernel_ms(functools.partial(E.morgan_records, drop_h=drop_h), args[:2], a.launches)
            out["similarity_ms_" + tag] = kernel_ms(functools.partial(E.morgan_similarity_records, drop_h=drop_h), args, a.launches)
        out[f"hash_ms_{a.pairs * rep}"] = kernel_ms(E.graph_hash_records, args[:2], a.launches)
    sim = MorganSimilarity(*E.morgan_similarity_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n)))
    count = E.morgan_records(t(prb_rec), t(prb_n))[1]
    out.update(features_mean=float(count.double().mean()), features_max=int(count.max()), tanimoto_mean=float(sim.tanimoto.mean()),
               cosine_mean=float(sim.cosine.mean()), tanimoto_one=int((sim.tanimoto == 1).sum()))
    if a.mirror_pairs > 0:
        m = min(a.mirror_pairs, a.pairs)
        got = torch.stack([sim.common, sim.n_prb, sim.n_ref], 1)[:m].cpu().numpy()
        t0 = time.time()
        want = np.array([FM.similarity_counts(x, y, True, 2, 2048) for x, y in zip(prb[:m], ref[:m])])
        out["mirror_pairs"] = m
        out["mirror_s"] = time.time() - t0
        out["counts_equal"] = int((want == got).all(1).sum())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
