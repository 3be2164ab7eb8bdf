"""Time dsi_key_sites and dsi_key_identity_records (key-level identity, csrc/ds_key.hip) beside dsm_normal_records +
ds_graph_identity_records (the mobile level) and beside dsc_stereo_identity_records (the stereo level) on the same pairs.

    python tools/key_bench.py [--pairs 10000] [--launches 20] [--out profiles/key_bench.json]

The pairs: the synthetic table of tests/structure_mirror.synthetic_pairs (2 000 ground-truth trees of 3-29 atoms with one candidate each:
rotated, shifted, renumbered, noised, a fifth with substituted types, a fifth with dropped atoms), tiled to `pairs` - the input of
tools/stereo_bench.py.  Prints one JSON line (and writes it to --out): the median kernel time (HIP events around one launch, after warm-up)
of every kernel, the ratios of the key level to the two levels it combines, the verdict histogram of the key level (so that a reader sees
the unassigned share), of the stereo level and of the mobile level, and the search nodes.  The ratios depend on how many isomorphisms the
normal forms of the table's molecules have; they are a record, not a gate.

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
    prb_rec, prb_n, ref_rec, ref_n = (torch.as_tensor(np.ascontiguousarray(x[rows])).to(dev) for x in (prb_rec, prb_n, ref_rec, ref_n))
    out = {"pairs": a.pairs, "distinct_pairs": base, "mean_atoms": float(ref_n.double().mean()), "launches": a.launches, "max_nodes": 4096}
    p_form, r_form = E.normal_records(prb_rec, prb_n), E.normal_records(ref_rec, ref_n)
    p_site, r_site = E.key_sites(prb_rec, prb_n), E.key_sites(ref_rec, ref_n)
    key_args = (p_form[0], p_form[1], p_site[0], r_form[0], r_form[1], r_site[0])
    out["key_sites_ms"] = kernel_ms(E.key_sites, (prb_rec, prb_n), a.launches)
    out["key_identity_ms"] = kernel_ms(E.key_identity_records, key_args, a.launches)
    out["key_identity_exhaustive_ms"] = kernel_ms(lambda *x: E.key_identity_records(*x, exhaustive=True), key_args, a.launches)
    out["normal_ms"] = kernel_ms(E.normal_records, (prb_rec, prb_n), a.launches)
    out["graph_identity_normal_ms"] = kernel_ms(E.graph_identity_records, (p_form[0], p_form[1], r_form[0], r_form[1]), a.launches)
    out["stereo_ms"] = kernel_ms(E.stereo_identity_records, (prb_rec, prb_n, ref_rec, ref_n), a.launches)
    med = lambda k: out[k]["median"]
    # one side's records per pair on both levels: the ground-truth side of an evaluation is normalised once per table, not per pair
    out["key_over_mobile"] = (med("key_sites_ms") + med("normal_ms") + med("key_identity_ms")) / (med("normal_ms") + med("graph_identity_normal_ms"))
    out["key_identity_over_stereo"] = med("key_identity_ms") / med("stereo_ms")
    out["key_sites_over_normal"] = med("key_sites_ms") / med("normal_ms")
    for name, exhaustive in (("first_same", False), ("exhaustive", True)):
        verdict, nodes, found, sites, _ = E.key_identity_records(*key_args, exhaustive=exhaustive)
        out[name] = {"verdicts": np.bincount(verdict.cpu().numpy(), minlength=7).tolist(), "nodes_mean": float(nodes.double().mean()),
                     "nodes_max": int(nodes.max()), "isomorphisms_max": int(found[:, 0].max())}
    out["with_sites"] = int(((sites[:, 0] + sites[:, 1]) > 0).sum())
    out["site_status"] = np.bincount(p_site[4].cpu().numpy(), minlength=5).tolist()
    out["site_nodes_max"] = int(p_site[3].max())
    out["stereo_verdicts"] = np.bincount(E.stereo_identity_records(prb_rec, prb_n, ref_rec, ref_n)[0].cpu().numpy(), minlength=7).tolist()
    out["mobile_verdicts"] = np.bincount(E.graph_identity_records(p_form[0], p_form[1], r_form[0], r_form[1])[0].cpu().numpy(), minlength=4).tolist()
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
