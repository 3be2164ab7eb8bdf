"""Time dsb_brics_records and dsb_brics_fragment_records (BRICS cuts, labels and fragments; csrc/ds_brics.hip) beside dsq_match_records with a
single pattern and dsk_scaffold_masks on the same records, and beside the CPU mirror.

    python tools/brics_bench.py [--records 10000] [--launches 50] [--mirror 300] [--out profiles/brics_bench.json]

The records: the hand-stated table and the derived set of tests/brics_mirror.py (molecules of 3 to 29 atoms, a third of them without a cut),
tiled to `records` rows.  Prints one JSON line (and writes it to --out): the median, minimum and maximum time of one call of each binding
(HIP events around the call, after three warm-up calls; a call is one kernel launch and the allocation of its outputs), the first two
kernels once more in the other order so that a drift of the clocks shows, the time of `brics_fragment_records` of structure_metrics (two
launches, a cumsum and one read of the total), of one `get_fragment_metric` evaluation of the first half of the records against the second,
and the wall time of tests/brics_mirror.analyse on the first `mirror` records scaled to `records` records.  There is no gate on any of these
times.

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

from diffspectra_amd import engine as E, smarts, structure_metrics as S      # noqa: E402
from tests import brics_mirror as B, structure_mirror as SM                  # noqa: E402
from record_bench import kernel_ms                                           # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rec, n = SM.records([mol for _, mol, _ in B.hand_table()] + B.derived_set())
    rows = np.arange(a.records) % len(n)
    dev = torch.device("cuda:0")
    rec_d, n_d = torch.as_tensor(rec[rows]).to(dev), torch.as_tensor(n[rows]).to(dev)
    one_pattern = torch.as_tensor(np.asarray(smarts.compile_patterns(["[#6]-[#8]"]), dtype=np.int32)).to(dev)
    out = {"records": a.records, "distinct_molecules": int(len(n)), "mean_atoms": float(n[rows].mean()), "launches": a.launches}
    found = S.brics(rec_d, n_d)
    counts = found.n_fragments.to(torch.int64)
    first, total = (torch.cumsum(counts, 0) - counts).contiguous(), int(counts.sum())
    out["brics_records_ms"] = kernel_ms(E.brics_records, (rec_d, n_d), a.launches)
    out["match_records_one_pattern_ms"] = kernel_ms(E.substructure_records, (rec_d, n_d, one_pattern), a.launches)
    out["scaffold_masks_ms"] = kernel_ms(E.scaffold_masks, (rec_d, n_d), a.launches)
    out["match_records_one_pattern_ms_again"] = kernel_ms(E.substructure_records, (rec_d, n_d, one_pattern), a.launches)
    out["brics_records_ms_again"] = kernel_ms(E.brics_records, (rec_d, n_d), a.launches)
    out["brics_fragment_records_kernel_ms"] = kernel_ms(E.brics_fragment_records, (rec_d, n_d, first, total), a.launches)
    out["brics_fragment_records_ms"] = kernel_ms(S.brics_fragment_records, (rec_d, n_d), a.launches)
    out["fragments"] = total
    out["mean_cuts"] = float(found.n_cuts.double().mean())
    out["without_a_cut"] = int((found.n_cuts == 0).sum())
    half = a.records // 2
    torch.cuda.synchronize()
    t0 = time.time()
    metric = S.get_fragment_metric((rec_d[half:].contiguous(), n_d[half:].contiguous()))((rec_d[:half].contiguous(), n_d[:half].contiguous()))
    torch.cuda.synchronize()
    out["fragment_metric_s"] = time.time() - t0
    out["frag"] = metric["frag"]
    out["distinct_fragments"] = metric["distinct_generated"]
    if a.mirror:
        k = min(a.mirror, len(n))
        t0 = time.time()
        want = B.as_arrays(B.analyse_table(rec[:k], n[:k]))
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * a.records / k
        got = [x[:k].cpu().numpy() for x in E.brics_records(rec_d, n_d)]
        out["mirror_rows_equal"] = int(np.all([(g == w).reshape(k, -1).all(1) for g, w in zip(got, want)], axis=0).sum())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
