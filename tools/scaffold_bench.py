"""Time dsk_scaffold_masks (Murcko scaffold atoms, ring atoms, ring counts; csrc/ds_scaffold.hip) beside dsv_valence_records and dsg_group_records
on the same records, and beside the CPU mirror.

    python tools/scaffold_bench.py [--records 10000] [--launches 50] [--mirror 300] [--out profiles/scaffold_bench.json]

The records: the hand-stated table and the derived set of tests/scaffold_mirror.py (molecules of 3 to 29 atoms, a third of them without a
ring), tiled to `records` rows.  Prints one JSON line (and writes it to --out): the median, minimum and maximum time of one call of each
binding (HIP events around the call, after three warm-up calls; a call is one kernel launch and the allocation of its outputs), the three
kernels once more in the other order so that a drift of the clocks shows, the time of `scaffold_records` (two launches) and of one
`get_scaffold_metric` evaluation of the first half of the records against the second, and the wall time of
tests/scaffold_mirror.analyse on the first `mirror` records scaled to `records` records.  There is no gate on any of these times.

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
from tests import scaffold_mirror as K, structure_mirror as SM                # noqa: E402
from record_bench import kernel_ms                                            # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rec, n = SM.records([mol for _, mol, _, _, _ in K.hand_table()] + K.derived_set())
    rows = np.arange(a.records) % len(n)
    dev = torch.device("cuda:0")
    rec_d, n_d = torch.as_tensor(rec[rows]).to(dev), torch.as_tensor(n[rows]).to(dev)
    out = {"records": a.records, "distinct_molecules": int(len(n)), "mean_atoms": float(n[rows].mean()), "launches": a.launches}
    out["scaffold_masks_ms"] = kernel_ms(E.scaffold_masks, (rec_d, n_d), a.launches)
    out["valence_records_ms"] = kernel_ms(E.valence_records, (rec_d, n_d), a.launches)
    out["group_records_ms"] = kernel_ms(E.group_records, (rec_d, n_d), a.launches)
    out["valence_records_ms_again"] = kernel_ms(E.valence_records, (rec_d, n_d), a.launches)
    out["scaffold_masks_ms_again"] = kernel_ms(E.scaffold_masks, (rec_d, n_d), a.launches)
    out["scaffold_records_ms"] = kernel_ms(S.scaffold_records, (rec_d, n_d), a.launches)
    found = S.scaffolds(rec_d, n_d)
    out["with_scaffold"] = int(found.has_scaffold().sum())
    out["mean_rings"] = float(found.rings.double().mean())
    half = a.records // 2
    torch.cuda.synchronize()
    t0 = time.time()
    metric = S.get_scaffold_metric((rec_d[half:].contiguous(), n_d[half:].contiguous()))((rec_d[:half].contiguous(), n_d[:half].contiguous()))
    torch.cuda.synchronize()
    out["scaffold_metric_s"] = time.time() - t0
    out["scaf"] = metric["scaf"]
    if a.mirror:
        k = min(a.mirror, len(n))
        t0 = time.time()
        want = K.analyse_table(rec[:k], n[:k])
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * a.records / k
        got = [x[:k].cpu().tolist() for x in E.scaffold_masks(rec_d, n_d)]
        out["mirror_rows_equal"] = sum(w["scaffold_mask"] == got[0][p] and w["ring_mask"] == got[1][p] and list(w["summary"]) == got[2][p]
                                       and w["status"] == got[3][p] for p, w in enumerate(want))
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
