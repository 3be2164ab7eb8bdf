"""Time dsm_mobile_records and dsm_normal_records (mobile-hydrogen groups and the normal form; csrc/ds_mobile.hip) beside dsb_brics_records on
the same records, and beside the CPU mirror.

    python tools/mobile_bench.py [--records 10000] [--launches 50] [--mirror 500] [--out profiles/mobile_bench.json]

The records: the hand-stated table and the seeded corpus of tests/mobile_mirror.py (molecules of 2 to 9 heavy atoms with explicit hydrogens, a
quarter of them with a mobile group), tiled to `records` rows.  Prints one JSON line (and writes it to --out): the median, minimum and maximum
time of one call of each binding (HIP events around the call, after three warm-up calls; a call is one kernel launch and the allocation of
its outputs), the first kernel once more at the end so that a drift of the clocks shows, the time of one `mobile_identity_batch` of the
records against themselves shifted by one row, and the wall time of the mirror's analysis and normal form on the first `mirror` records,
scaled to `records` records.  There is no gate on any of these times.

Run it from the repository root, after the library has been built: the molecules and the mirror are the test suite's own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E, structure_metrics as S              # noqa: E402
from tests import mobile_mirror as M, structure_mirror as SM                 # noqa: E402
from record_bench import kernel_ms                                           # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    E.load_library()
    rec, n = SM.records([mol for _, mol, _ in M.hand_table()] + M.corpus())
    rows = np.arange(a.records) % len(n)
    dev = torch.device("cuda:0")
    rec_d, n_d = torch.as_tensor(rec[rows]).to(dev), torch.as_tensor(n[rows]).to(dev)
    out = {"records": a.records, "distinct_molecules": int(len(n)), "mean_atoms": float(n[rows].mean()), "launches": a.launches}
    found = S.mobile_hydrogens(rec_d, n_d)
    out["with_a_group"] = int((found.n_groups > 0).sum())
    out["mean_nodes"] = float(found.nodes.double().mean())
    out["max_nodes"] = int(found.nodes.max())
    out["mobile_records_ms"] = kernel_ms(E.mobile_records, (rec_d, n_d), a.launches)
    out["normal_records_ms"] = kernel_ms(E.normal_records, (rec_d, n_d), a.launches)
    out["brics_records_ms"] = kernel_ms(E.brics_records, (rec_d, n_d), a.launches)
    out["mobile_records_ms_again"] = kernel_ms(E.mobile_records, (rec_d, n_d), a.launches)
    other = (torch.roll(rec_d, 1, 0).contiguous(), torch.roll(n_d, 1, 0).contiguous())
    torch.cuda.synchronize()
    t0 = time.time()
    same = S.mobile_identity_batch(other, (rec_d, n_d))
    torch.cuda.synchronize()
    out["mobile_identity_batch_s"] = time.time() - t0
    out["identical"] = int(same.identical.sum())
    out["layer_1"] = int((same.layer == 1).sum())
    if a.mirror:
        k = min(a.mirror, a.records)
        t0 = time.time()
        want = M.as_arrays(M.analyse_table(rec[rows[:k]], n[rows[:k]]))
        forms = M.normal_table(rec[rows[:k]], n[rows[:k]])
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * a.records / k
        got = [x[:k].cpu().numpy() for x in E.mobile_records(rec_d, n_d)] + [x[:k].cpu().numpy() for x in E.normal_records(rec_d, n_d)]
        out["mirror_rows_equal"] = int(np.all([(g == w).reshape(k, -1).all(1) for g, w in zip(got, list(want) + list(forms))], axis=0).sum())
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
