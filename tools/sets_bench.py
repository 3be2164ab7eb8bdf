"""Time the set-against-set scan of the evaluation path: dss_tanimoto_nn (csrc/ds_sets.hip) alone on synthetic bit rows, the same numbers
computed the MOSES way with torch on the same GPU, and the whole closure of structure_metrics.get_set_similarity_metric on records.

    python tools/sets_bench.py [--rows 10000] [--columns 10000,100000] [--bits 1024] [--density 0.05] [--launches 20] [--records 10000]
                               [--out profiles/sets_bench.json]

The rows: seeded random bits at `density`.  The kernel: the median time of one call (HIP events around it, after warm-up, tools/record_bench.py)
with a caller-owned workspace, and the pairs per second next to the instruction-count estimate of the issue that asked for the kernel - one
v_and_b32 and one v_bcnt_u32_b32 per dword of a pair, 4 cycles per wave64 instruction and SIMD, 4 SIMDs x 256 CUs at 2.4 GHz - which counts
neither the fp64 division nor the nearest-neighbour comparison of every pair.  The yardstick: MOSES's formulation (average_agg_tanimoto,
restated from the package as remembered) - the bit rows as a float matrix, one matmul per batch of columns for the intersections,
tp / (|a| + |b| - tp) with NaN -> 1, a running max and a running sum - in fp32 as MOSES runs it and with fp16 operands (exact: the products
are 0 or 1 and the matmul accumulates in fp32), batched so that it fits in memory.  Its nearest neighbour is a float maximum and its sum a
float sum in torch's order: close to, not bit for bit, the kernel's outputs; the largest differences are printed.  The closure: `records`
generated records against a test table of `records` records (tests/graph_mirror.seeded_pairs at the QM9 size mix), uniqueness filter, bit
rows, SNN, IntDiv; first call (builds nothing: the test side is prepared before) and the median of three.

Run it from the repository root: the record generator is the test suite's own (tests/graph_mirror.py)."""
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
from diffspectra_amd import structure_metrics as S           # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)

VALU_LANES_PER_S = 64 / 4 * 4 * 256 * 2.4e9                 # lanes of one-wave-per-SIMD VALU issue per second of the card


def random_rows(rng, n, n_bits, density, dev):
    bits = rng.random((n, n_bits)) < density
    words = np.packbits(bits, axis=1, bitorder="little").view(np.int64).reshape(n, n_bits // 64)
    return torch.as_tensor(words).to(dev), torch.as_tensor(bits.sum(1).astype(np.int32)).to(dev), torch.as_tensor(bits).to(dev)


def torch_way(a_bits, b_bits, dtype, batch):
    """(nearest similarity [Na], sum of similarities [Na]) as MOSES computes them: float rows, a matmul per column batch."""
    a = a_bits.to(dtype)
    a_n = a_bits.sum(1, keepdim=True).float()
    best = torch.full((a.shape[0],), -1.0, device=a.device)
    total = torch.zeros(a.shape[0], dtype=torch.float64, device=a.device)
    for lo in range(0, b_bits.shape[0], batch):
        b = b_bits[lo:lo + batch].to(dtype)
        tp = torch.mm(a, b.t()).float()
        jac = tp / (a_n + b_bits[lo:lo + batch].sum(1).float().unsqueeze(0) - tp)
        jac[torch.isnan(jac)] = 1.0
        best = torch.maximum(best, jac.max(1).values)
        total += jac.sum(1, dtype=torch.float64)
    return best, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--columns", default="10000,100000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    out = {"rows": a.rows, "bits": a.bits, "density": a.density, "launches": a.launches, "estimate_pairs_per_s": VALU_LANES_PER_S / (2 * a.bits / 32),
           "shapes": []}
    aw, ap_, ab = random_rows(rng, a.rows, a.bits, a.density, dev)
    for nb in (int(x) for x in a.columns.split(",")):
        bw, bp, bb = random_rows(rng, nb, a.bits, a.density, dev)
        ws = torch.empty(E.tanimoto_nn_workspace_bytes(a.rows, nb), dtype=torch.uint8, device=dev)
        shape = {"columns": nb, "pairs": a.rows * nb, "workspace_bytes": ws.shape[0]}
        shape["kernel_ms"] = kernel_ms(lambda: E.tanimoto_nn(aw, ap_, bw, bp, a.bits, False, ws), (), a.launches)
        shape["pairs_per_s"] = shape["pairs"] / (shape["kernel_ms"]["median"] * 1e-3)
        shape["share_of_estimate"] = shape["pairs_per_s"] / out["estimate_pairs_per_s"]
        near = S.SetSimilarity(*E.tanimoto_nn(aw, ap_, bw, bp, a.bits, False, ws))
        for name, dtype in (("torch_fp32", torch.float32), ("torch_fp16", torch.float16)):
            shape[name + "_ms"] = kernel_ms(torch_way, (ab, bb, dtype, a.batch), max(3, a.launches // 4))
            shape[name + "_over_kernel"] = shape[name + "_ms"]["median"] / shape["kernel_ms"]["median"]
            best, total = torch_way(ab, bb, dtype, a.batch)
            shape[name + "_max_nearest_diff"] = float((best.double() - near.nearest).abs().max())
            shape[name + "_max_sum_diff"] = float((total - near.sum).abs().max())
        out["shapes"].append(shape)
        del bw, bp, bb, ws
    if a.records > 0:
        from tests import graph_mirror as GM, structure_mirror as SM
        sizes = tuple(int(s) for s in qm9_sizes(rng, a.records))
        t0 = time.time()
        ref, prb, _ = GM.seeded_pairs(a.records, 20261018, sizes=sizes, kinds=(0, 1, 2, 3))
        table = lambda mols: tuple(torch.as_tensor(x).to(dev) for x in SM.records(mols))
        test, gen = table(ref), table(prb)
        out["generate_s"] = time.time() - t0
        t0 = time.time()
        fn = S.get_set_similarity_metric(test)
        torch.cuda.synchronize()
        out["prepare_test_side_s"] = time.time() - t0
        times = []
        for _ in range(4):
            t0 = time.time()
            res = fn(gen)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        out.update(records=a.records, closure_first_s=times[0], closure_median_s=float(np.median(times[1:])), snn=res["snn"], int_div=res["int_div"],
                   n_generated=res["n_generated"], n_test=res["n_test"])
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
