"""Time dsp_read_smiles (records from SMILES strings; csrc/ds_reader.hip) on a table of generator strings, beside the CPU mirror.

    python tools/reader_bench.py [--rows 100000] [--launches 20] [--warmup 5] [--mirror 5000] [--out profiles/reader_bench.json]

The strings: `rows` strings of tests/smiles_reader_mirror.generated (random trees with ring closures, charges, brackets and lower-case rings,
never more than 29 atoms with their hydrogens).  Prints one JSON line (and writes it to --out): the time of `launches` calls of the binding
between two HIP events after `warmup` calls (a call is one kernel launch and the allocation of its outputs), strings per second from it, the
statuses, and the rate of tests/smiles_reader_mirror.read on the first `mirror` of the same strings.  There is no gate on any of these.

Run it from the repository root, with the library built: the strings and the mirror are the test suite's own."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E, structure_metrics as S               # noqa: E402
from tests import smiles_reader_mirror as R                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mirror", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    strings = list(R.generated(a.rows, seed=20261025))
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    text, length = S.pack_smiles(strings, dev)
    torch.cuda.synchronize()
    out = {"rows": a.rows, "distinct_strings": len(set(strings)), "mean_length": float(length.float().mean()), "launches": a.launches,
           "warmup": a.warmup, "pack_and_copy_s": time.perf_counter() - t0}
    for _ in range(a.warmup):
        got = E.read_smiles(text, length)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(a.launches):
        got = E.read_smiles(text, length)
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / a.launches
    status = got[2].cpu()
    out.update(ms_per_launch=ms, strings_per_s=a.rows / (ms * 1e-3), statuses=[int((status == k).sum()) for k in range(8)],
               mean_atoms=float(got[1].float().mean()), mean_nodes=float(got[8].float().mean()))
    if a.mirror:
        k = min(a.mirror, a.rows)
        t0 = time.perf_counter()
        want = [R.read(s) for s in strings[:k]]
        out["mirror_rows"] = k
        out["mirror_strings_per_s"] = k / (time.perf_counter() - t0)
        rec, n = got[0][:k].cpu().numpy(), got[1][:k].cpu().tolist()
        out["mirror_rows_equal"] = sum(w["rec"] == rec[p].tobytes() and w["n"] == n[p] for p, w in enumerate(want))
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
