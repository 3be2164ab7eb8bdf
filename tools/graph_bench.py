"""Time ds_graph_identity_records (graph identity, csrc/ds_graph.hip) on an evaluation-like mix at the QM9 size mix, beside
ds_match_records on the same pairs and the CPU mirror.

    python tools/graph_bench.py [--pairs 10000] [--launches 20] [--no-mirror] [--out profiles/graph_identity_bench.json]

The pairs: ground truths of tests/graph_mirror.random_molecule at the QM9 size mix; one third of the generated molecules are the ground
truth under another atom order with unrelated coordinates (identical), the rest carry a degree-preserving bond switch on top.  Prints one
JSON line (and writes it to --out): the median kernel time (HIP events around one launch, after warm-up) of the identity kernel, of the hash
kernel and of ds_match_records for `pairs` and 10 x `pairs` pairs (the same records tiled), the mean and maximum of the search nodes, and the
wall time of tests/graph_mirror.same_graph on the `pairs` set.  Compare with one denoise iteration of the same number of molecules:
bench.py's samples / (value * denoise_steps) seconds.

Run it from the repository root: the pair generator and the mirror are the test suite's own (tests/graph_mirror.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E                      # noqa: E402
from tests import graph_mirror as GM, structure_mirror as SM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-mirror", action="store_true")
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
    out = {"pairs": a.pairs, "mean_atoms": float(sizes.mean()), "generate_s": gen_s, "launches": a.launches, "max_nodes": 4096}
    for rep in (1, 10):
        args = (t(prb_rec, rep), t(prb_n, rep), t(ref_rec, rep), t(ref_n, rep))
        out[f"identity_ms_{a.pairs * rep}"] = kernel_ms(E.graph_identity_records, args, a.launches)
        out[f"hash_ms_{a.pairs * rep}"] = kernel_ms(E.graph_hash_records, args[:2], a.launches)
        out[f"match_ms_{a.pairs * rep}"] = kernel_ms(E.match_records, args, a.launches)
    verdict, nodes, _ = E.graph_identity_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n))
    verdict, nodes = verdict.cpu().numpy(), nodes.cpu().numpy()
    out.update(identical=int((verdict == 1).sum()), different=int((verdict == 0).sum()), undecided=int((verdict == 2).sum()),
               nodes_mean=float(nodes.mean()), nodes_max=int(nodes.max()),
               match_exact=int(E.match_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n))[4].sum()))
    if not a.no_mirror:
        t0 = time.time()
        want = np.array([GM.same_graph(x, y) for x, y in zip(prb, ref)])
        out["mirror_s"] = time.time() - t0
        out["mirror_identical"] = int(want.sum())
        out["verdicts_equal"] = int((want == (verdict == 1)).sum())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
