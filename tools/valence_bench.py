"""Time dsv_valence_records and dsv_fragment_records (valence analytics, csrc/ds_valence.hip) at the QM9 size mix, beside the CPU mirror.

    python tools/valence_bench.py [--records 10000] [--launches 20] [--mirror 500] [--out profiles/valence_bench.json]

The records: tests/graph_mirror.random_molecule at the QM9 size mix (trees with ring closures, random coordinates).  Prints one JSON line
(and writes it to --out): the median kernel time (HIP events around one launch, after warm-up) of both entry points with the bond orders
from the record and from the distances, for `records` and 10 x `records` records (the same records tiled); the wall time of the closure of
get_edm_metric_2d on `records` records (both launches, graph_classes, the device-to-host syncs); and the wall time of
tests/valence_mirror.analyse on the first `mirror` records, scaled to `records` - a plain-Python loop per molecule, which is what the
reference's check_2D_stability is too (the reference itself needs RDKit and is not timed here).

Run it from the repository root: the molecule generator and the mirror are the test suite's own."""
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
from tests import graph_mirror as GM, structure_mirror as SM, valence_mirror as VM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                                 # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mirror", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(7)
    sizes = qm9_sizes(rng, a.records)
    t0 = time.time()
    rec, n = SM.records([GM.random_molecule(rng, int(s)) for s in sizes])
    gen_s = time.time() - t0
    dev = torch.device("cuda:0")
    t = lambda x, rep=1: torch.as_tensor(np.tile(x, (rep,) + (1,) * (x.ndim - 1))).to(dev)
    out = {"records": a.records, "mean_atoms": float(sizes.mean()), "generate_s": gen_s, "launches": a.launches}
    for rep in (1, 10):
        rec_d, n_d = t(rec, rep), t(n, rep)
        for mode, name in ((E.BONDS_RECORD, "record"), (E.BONDS_DISTANCE, "distance")):
            keep = E.valence_records(rec_d, n_d, mode)[4]
            out[f"valence_{name}_ms_{a.records * rep}"] = kernel_ms(E.valence_records, (rec_d, n_d, mode), a.launches)
            out[f"fragment_{name}_ms_{a.records * rep}"] = kernel_ms(E.fragment_records, (rec_d, n_d, keep, mode), a.launches)
    rec_d, n_d = t(rec), t(n)
    fn = S.get_edm_metric_2d()
    try:                                                      # graph_classes raises when a comparison runs out of its search budget
        fn(rec_d, n_d)
        torch.cuda.synchronize()
        t0 = time.time()
        numbers = fn(rec_d, n_d)
        torch.cuda.synchronize()
        out["edm_metric_2d_s"] = time.time() - t0
        out["edm_metric_2d"] = {k: v for k, v in numbers.items() if isinstance(v, (int, float))}
    except RuntimeError as err:
        out["edm_metric_2d_error"] = str(err)
    if a.mirror:
        k = min(a.mirror, a.records)
        t0 = time.time()
        want = VM.analyse_table(rec[:k], n[:k])
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * a.records / k
        got = [x[:k].cpu().tolist() for x in E.valence_records(rec_d, n_d)]
        out["mirror_rows_equal"] = sum(w["valence"] == got[0][p] and w["stable_mask"] == got[1][p] and w["valid_mask"] == got[2][p]
                                       and list(w["summary"]) == got[3][p] and w["largest_mask"] == got[4][p] and w["status"] == got[5][p]
                                       for p, w in enumerate(want))
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
