"""Time dsr_best_rmsd_records (the symmetry-corrected Kabsch RMSD, csrc/ds_bestrmsd.hip) on synthetic pairs at the QM9 size mix, in both
modes, beside ds_match_records on the same pairs in the same session.

    python tools/best_rmsd_bench.py [--pairs 10000] [--launches 20]

Prints one JSON line: per mode the median kernel time (HIP events around one launch, after warm-up), the verdict counts and the mean / max
search nodes and isomorphisms; the median time of ds_match_records as the comparator.  There is no gate.

Run it from the repository root: the pair generator is the test suite's own (tests/structure_mirror.py, the pairs of tools/match_bench.py:
three fifths of them noised copies of the ground truth, the rest with substituted types or dropped atoms, which refinement alone refuses)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E                      # noqa: E402
from tests import structure_mirror as SM                      # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(7)
    sizes = qm9_sizes(rng, a.pairs)
    ref_rec, ref_n, prb_rec, prb_n = SM.synthetic_pairs(a.pairs, 20261017, sizes=sizes)
    dev = torch.device("cuda:0")
    args = tuple(torch.as_tensor(x).to(dev) for x in (prb_rec, prb_n, ref_rec, ref_n))
    out = {"pairs": a.pairs, "mean_atoms": float(sizes.mean()), "launches": a.launches}
    for atoms in ("heavy", "all"):
        fn = lambda *t, atoms=atoms: E.best_rmsd_records(*t, None, 4096, atoms)
        res = fn(*args)
        verdict, nodes, found = res[0].cpu().numpy(), res[3].cpu().numpy(), res[4].cpu().numpy()
        hit = verdict == 1
        out[atoms] = {"kernel_ms": kernel_ms(fn, args, a.launches), "verdicts": np.bincount(verdict, minlength=4).tolist(),
                      "nodes_mean": float(nodes.mean()), "nodes_max": int(nodes.max()), "nodes_mean_of_hits": float(nodes[hit].mean()) if hit.any() else None,
                      "found_mean_of_hits": float(found[hit].mean()) if hit.any() else None, "found_max": int(found.max()),
                      "median_rmsd_of_hits": float(np.nanmedian(res[1].cpu().numpy()[hit, 0])) if hit.any() else None}
    out["match_records_kernel_ms"] = kernel_ms(E.match_records, args, a.launches)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
