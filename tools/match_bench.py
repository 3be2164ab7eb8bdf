"""Time ds_match_records (the structure metric, csrc/ds_match.hip) on synthetic pairs at the QM9 size mix, beside the CPU mirror.

    python tools/match_bench.py [--pairs 10000] [--launches 20] [--no-mirror]

Prints one JSON line: the median kernel time (HIP events around one launch, after warm-up) for `pairs` and for 10 x `pairs` pairs (the
same records tiled), and the wall time of tests/structure_mirror.py on the `pairs` set.  Compare with one denoise iteration of the same
number of molecules: bench.py's samples / (value * denoise_steps) seconds.

Run it from the repository root: the pair generator and the mirror are the test suite's own (tests/structure_mirror.py), imported from
there so that the measurement and the parity test time and check one and the same recipe."""
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
from tests import structure_mirror as SM                      # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-mirror", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(7)
    sizes = qm9_sizes(rng, a.pairs)
    t0 = time.time()
    ref_rec, ref_n, prb_rec, prb_n = SM.synthetic_pairs(a.pairs, 20261017, sizes=sizes)
    gen_s = time.time() - t0
    dev = torch.device("cuda:0")
    t = lambda x, rep=1: torch.as_tensor(np.tile(x, (rep,) + (1,) * (x.ndim - 1))).to(dev)
    out = {"pairs": a.pairs, "mean_atoms": float(sizes.mean()), "generate_s": gen_s, "launches": a.launches}
    for rep in (1, 10):
        args = (t(prb_rec, rep), t(prb_n, rep), t(ref_rec, rep), t(ref_n, rep))
        out[f"kernel_ms_{a.pairs * rep}"] = kernel_ms(E.match_records, args, a.launches)
    res = E.match_records(t(prb_rec), t(prb_n), t(ref_rec), t(ref_n))
    out["valid"] = int((~torch.isnan(res[0])).sum())
    out["exact"] = int(res[4].sum())
    if not a.no_mirror:
        t0 = time.time()
        want = SM.match_batch(prb_rec, prb_n, ref_rec, ref_n)
        out["mirror_s"] = time.time() - t0
        out["mirror_valid"] = sum(w["valid"] for w in want)
        out["maps_equal"] = int(sum(np.array_equal(w["map"], m) for w, m in zip(want, res[5].cpu().numpy())))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
