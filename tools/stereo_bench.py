"""Time dsc_stereo_identity_records (stereo-aware identity, csrc/ds_stereo.hip) beside ds_graph_identity_records on the same pairs.

    python tools/stereo_bench.py [--pairs 10000] [--launches 20] [--out profiles/stereo_bench.json]

The pairs: the synthetic table of tests/structure_mirror.synthetic_pairs (2 000 ground-truth trees of 3-29 atoms with one candidate each:
rotated, shifted, renumbered, noised, a fifth with substituted types, a fifth with dropped atoms), tiled to `pairs`.  Prints one JSON line
(and writes it to --out): the median kernel time (HIP events around one launch, after warm-up) of the stereo kernel with exhaustive = 0 and
1, of dsc_stereo_sites on the generated records and of the graph-identity kernel, the ratio of the first to the last, the verdict counts and
the search nodes.  The ratio depends on how many isomorphisms the table's molecules have; it is a record, not a gate.

Run it from the repository root: the pair generator is the test suite's own (tests/structure_mirror.py)."""
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
from record_bench import kernel_ms                            # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    base = 2000
    ref_rec, ref_n, prb_rec, prb_n = SM.synthetic_pairs(base, 20261017)
    rows = np.arange(a.pairs) % base
    dev = torch.device("cuda:0")
    args = tuple(torch.as_tensor(np.ascontiguousarray(x[rows])).to(dev) for x in (prb_rec, prb_n, ref_rec, ref_n))
    out = {"pairs": a.pairs, "distinct_pairs": base, "mean_atoms": float(ref_n.mean()), "launches": a.launches, "max_nodes": 4096}
    out["stereo_ms"] = kernel_ms(E.stereo_identity_records, args, a.launches)
    out["stereo_exhaustive_ms"] = kernel_ms(lambda *x: E.stereo_identity_records(*x, exhaustive=True), args, a.launches)
    out["sites_ms"] = kernel_ms(E.stereo_sites, args[:2], a.launches)
    out["graph_identity_ms"] = kernel_ms(E.graph_identity_records, args, a.launches)
    out["stereo_over_graph"] = out["stereo_ms"]["median"] / out["graph_identity_ms"]["median"]
    for name, exhaustive in (("first_same", False), ("exhaustive", True)):
        verdict, nodes, found, sites, _ = E.stereo_identity_records(*args, exhaustive=exhaustive)
        out[name] = {"verdicts": np.bincount(verdict.cpu().numpy(), minlength=7).tolist(), "nodes_mean": float(nodes.double().mean()),
                     "nodes_max": int(nodes.max()), "isomorphisms_max": int(found[:, 0].max())}
    out["with_sites"] = int(((sites[:, 0] + sites[:, 1]) > 0).sum())
    graph = E.graph_identity_records(*args)
    out["graph_identical"] = int((graph[0] == 1).sum())
    out["graph_nodes_mean"] = float(graph[1].double().mean())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
