"""Time ds_mces_records (the MCES distance, csrc/ds_mces.hip) on an evaluation-like mix at the QM9 size mix, beside ds_match_records and
ds_graph_identity_records on the same pairs in the same session, and the CPU mirror.

    python tools/mces_bench.py [--pairs 10000] [--launches 20] [--mirror-pairs 1000] [--out profiles/mces_bench.json]

The pairs: ground truths of tests/mces_mirror.random_molecule whose TOTAL atom counts (hydrogens included) follow the QM9 size mix of
tools/match_bench.py; one third of the generated molecules are the ground truth under another atom order (identical), the rest carry one
of the perturbations of tests/mces_mirror.treated (a bond moved, a bond order changed, a heavy type changed, an unrelated molecule).  Prints
one JSON line (and writes it to --out): the median kernel time (HIP events around one launch, after warm-up) of the three kernels for
`pairs` and 10 x `pairs` pairs (the same records tiled), the distribution of the search nodes (mean, percentiles, maximum and a
power-of-two histogram), the mean distance, and the host time of the mirror's integer program on the first `mirror-pairs` pairs.  Compare with
one denoise iteration of the same number of molecules: bench.py's samples / (value * denoise_steps) seconds.

Run it from the repository root: the pair generator and the mirror are the test suite's own (tests/mces_mirror.py)."""
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
from tests import graph_mirror as GM, mces_mirror as MM, structure_mirror as SM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)


def molecule_of_size(rng, n_atoms):
    """A molecule-like graph with ``n_atoms`` atoms in all where the valences allow it: the heavy-atom count is drawn until the hydrogens fit."""
    for _ in range(64):
        heavy = int(rng.integers(max(1, (n_atoms + 3) // 5), min(9, n_atoms) + 1))
        mol = MM.random_molecule(rng, heavy, max_atoms=n_atoms)
        if len(mol["type"]) == n_atoms:
            return mol
    return mol


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
    ref = [molecule_of_size(rng, int(s)) for s in sizes]
    prb = [MM.treated(m, (0, 1 + p // 3 % 4, 1 + (p // 3 + 2) % 4)[p % 3], rng, (1, 9), GM.W) for p, m in enumerate(ref)]
    (ref_rec, ref_n), (prb_rec, prb_n) = SM.records(ref), SM.records(prb)
    gen_s = time.time() - t0
    dev = torch.device("cuda:0")
    t = lambda x, rep=1: torch.as_tensor(np.tile(x, (rep,) + (1,) * (x.ndim - 1))).to(dev)
    out = {"pairs": a.pairs, "mean_atoms": float(ref_n.mean()), "mean_heavy_atoms": float(np.mean([(m["type"] != 0).sum() for m in ref])),
           "generate_s": gen_s, "launches": a.launches, "max_nodes": 1 << 18, "drop_h": 1}
    for rep in (1, 10):
        args = (t(prb_rec, rep), t(prb_n, rep), t(ref_rec, rep), t(ref_n, rep))
        out[f"mces_ms_{a.pairs * rep}"] = kernel_ms(E.mces_records, args, a.launches)
        out[f"identity_ms_{a.pairs * rep}"] = kernel_ms(E.graph_identity_records, args, a.launches)
        out[f"match_ms_{a.pairs * rep}"] = kernel_ms(E.match_records, args, a.launches)
    dist, lower, status, nodes, _ = (x.cpu().numpy() for x in E.mces_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n)))
    hist = np.bincount(np.where(nodes > 0, np.floor(np.log2(np.maximum(nodes, 1))).astype(int) + 1, 0))
    out.update(exact=int((status == 0).sum()), undecided=int((status == 2).sum()), zero=int((dist == 0).sum()), dist_mean=float(dist.mean()),
               nodes_mean=float(nodes.mean()), nodes_p50=float(np.percentile(nodes, 50)), nodes_p99=float(np.percentile(nodes, 99)),
               nodes_max=int(nodes.max()), nodes_sum=int(nodes.sum()),
               nodes_hist_pow2={("0" if k == 0 else f"<{1 << k}"): int(c) for k, c in enumerate(hist) if c},
               identity_identical=int((E.graph_identity_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n))[0] == 1).sum()))
    if a.mirror_pairs > 0:
        m = min(a.mirror_pairs, a.pairs)
        t0 = time.time()
        want = np.array([MM.mces_milp(x, y) for x, y in zip(prb[:m], ref[:m])])
        out["mirror_pairs"] = m
        out["mirror_s"] = time.time() - t0
        out["dist_equal"] = int((want == dist[:m]).sum())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
