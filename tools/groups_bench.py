"""Time dsg_group_similarity_records and dsg_group_records (functional groups, csrc/ds_groups.hip) beside ds_morgan_similarity_records on
the same pairs, and beside the CPU mirror.

    python tools/groups_bench.py [--pairs 10000] [--launches 50] [--mirror 300] [--out profiles/groups_bench.json]

The pairs: the hand-stated table and the derived set of tests/groups_mirror.py (organic molecules of 3 to 24 atoms with explicit hydrogens,
a third of them aromatic), tiled to `pairs` rows; pair p reads ground-truth row ref_index[p], a fixed permutation.  Prints one JSON line (and
writes it to --out): the median, minimum and maximum time of one call of each binding (HIP events around the call, after three warm-up calls;
a call is one kernel launch and the allocation of its outputs), the mean similarity, and the wall time of tests/groups_mirror.analyse on the
first `mirror` records scaled to 2 x `pairs` records - a plain-Python loop per molecule, as the reference's is (the reference itself needs
RDKit and is not timed here).

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

from diffspectra_amd import engine as E, structure_metrics as S               # noqa: E402
from tests import groups_mirror as G, structure_mirror as SM                  # noqa: E402
from record_bench import kernel_ms                                            # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rec, n = SM.records([mol for _, mol, _, _ in G.hand_table()] + G.derived_set())
    rows = np.arange(a.pairs) % len(n)
    rng = np.random.default_rng(7)
    dev = torch.device("cuda:0")
    rec_d, n_d = torch.as_tensor(rec[rows]).to(dev), torch.as_tensor(n[rows]).to(dev)
    index = torch.as_tensor(rng.permutation(a.pairs)).to(dev)
    out = {"pairs": a.pairs, "distinct_molecules": int(len(n)), "mean_atoms": float(n[rows].mean()), "launches": a.launches}
    out["group_similarity_ms"] = kernel_ms(E.group_similarity_records, (rec_d, n_d, rec_d, n_d, index), a.launches)
    out["morgan_similarity_ms"] = kernel_ms(E.morgan_similarity_records, (rec_d, n_d, rec_d, n_d, index), a.launches)
    out["group_records_ms"] = kernel_ms(E.group_records, (rec_d, n_d), a.launches)
    # once more in the other order: the two pair kernels alternate, so a drift of the clocks shows
    out["morgan_similarity_ms_again"] = kernel_ms(E.morgan_similarity_records, (rec_d, n_d, rec_d, n_d, index), a.launches)
    out["group_similarity_ms_again"] = kernel_ms(E.group_similarity_records, (rec_d, n_d, rec_d, n_d, index), a.launches)
    alike = S.functional_group_similarity_batch((rec_d, n_d), (rec_d, n_d), ref_index=index)
    out["ok_pairs"] = int(alike.valid.sum())
    out["mean_similarity"] = float(alike.similarity[alike.valid].cpu().mean())
    if a.mirror:
        k = min(a.mirror, len(n))
        t0 = time.time()
        want = G.analyse_table(rec[:k], n[:k])
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * 2 * a.pairs / k
        got = [x[:k].cpu().tolist() for x in E.group_records(rec_d, n_d)]
        out["mirror_rows_equal"] = sum(w["groups"] == got[0][p] and w["aromatic_mask"] == got[1][p] and w["status"] == got[2][p] for p, w in enumerate(want))
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
