"""Time the substructure-geometry MMD of the evaluation path: the extraction kernels (ds_geometry_count_records / ds_geometry_fill_records,
csrc/ds_subgeom.hip) on evaluation-like records and the 24-class MMD (ds_mmd_1d_segments, csrc/ds_mmd.hip) at the reference's sample cap.

    python tools/geometry_bench.py [--records 10000] [--samples 20000] [--launches 20] [--host-samples 4000] [--out profiles/geometry_bench.json]

The records: the generated side of tests/graph_mirror.seeded_pairs at the QM9 size mix (molecule-like graphs with random coordinates), against
the 24 QM9 substructure classes.  The MMD: 24 classes of `samples` + `samples` seeded normal samples (bond-length-like, angle-like and
dihedral-like spreads), kernel_mul 2, kernel_num 5 - the reference's call.  Prints one JSON line (and writes it to --out): the median time
(HIP events around one call, after warm-up) of the count kernel, the fill kernel and the MMD launch sequence; the entries extracted; the
pairs x bandwidths per second of the MMD (over the ns^2 + nt^2 + ns nt pairs of the definition; the kernel visits the upper triangle of XX
and YY, `evaluated_pairs`), next to the card's v_exp_f32 rate (8 cycles per wave64 instruction and SIMD, 4 SIMDs x 256 CUs at 2.4 GHz: the
kernel spends one v_exp_f32 per evaluated pair with kernel_mul 2 and at most 5 bandwidths, one per pair and bandwidth otherwise); and, for scale, the host time of
the same formula restated in fp32 torch on `host-samples` + `host-samples` samples of one class.

Run it from the repository root: the record generator is the test suite's own (tests/graph_mirror.py)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffspectra_amd import engine as E                      # noqa: E402
from diffspectra_amd.structure_metrics import geometry_classes, sub_geometry   # noqa: E402
from tests import graph_mirror as GM, structure_mirror as SM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                 # noqa: E402  (this directory: the script's own)

V_EXP_PER_S = 64 / 8 * 4 * 256 * 2.4e9                      # v_exp_f32 lanes per second of the card


def host_mmd(source, target, kernel_mul=2.0, kernel_num=5):
    """compute_mmd's formula in fp32 torch on the host, one block (the sizes here fit)."""
    z = torch.cat([source, target])
    ns, n = source.shape[0], z.shape[0]
    d2 = (z.unsqueeze(0) - z.unsqueeze(1)) ** 2
    bw = d2.sum() / (n * n - n) / kernel_mul ** (kernel_num // 2)
    k = sum(torch.exp(-d2 / (bw * kernel_mul ** i)) for i in range(kernel_num))
    return float(k[:ns, :ns].mean() + k[ns:, ns:].mean() - 2 * k[:ns, ns:].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-samples", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(7)
    sizes = qm9_sizes(rng, a.records)
    t0 = time.time()
    _, prb, _ = GM.seeded_pairs(a.records, 20261018, sizes=tuple(int(s) for s in sizes), kinds=(0,))
    rec, n = SM.records(prb)
    gen_s = time.time() - t0
    dev = torch.device("cuda:0")
    rec, n = torch.as_tensor(rec).to(dev), torch.as_tensor(n).to(dev)
    classes = geometry_classes()
    tabs = [torch.tensor(list(c), dtype=torch.int32, device=dev) for c in classes.codes]
    out = {"records": a.records, "mean_atoms": float(sizes.mean()), "generate_s": gen_s, "launches": a.launches}
    out["count_ms"] = kernel_ms(E.geometry_count_records, (rec, n, *tabs), a.launches)
    counts, skipped = E.geometry_count_records(rec, n, *tabs)
    ends = counts.to(torch.int64).cumsum(0)
    totals = ends[-1].tolist()
    out["fill_ms"] = kernel_ms(E.geometry_fill_records, (rec, n, *tabs, (ends - counts).contiguous(), totals), a.launches)
    t0 = time.time()
    found = sub_geometry(rec, n, classes)
    torch.cuda.synchronize()
    out.update(sub_geometry_s=time.time() - t0, entries=dict(zip(("bonds", "angles", "dihedrals"), totals)), skipped=int(skipped.sum()),
               samples_per_symbol={s: int(v.shape[0]) for s, v in found.values.items()})
    # the MMD of 24 classes at the sample cap
    C_, S_ = 24, a.samples
    centre = np.repeat([1.3, 110.0, 0.0], 8) + np.tile(np.arange(8), 3) * 0.05
    spread = np.repeat([0.03, 5.0, 60.0], 8)
    x = torch.as_tensor((rng.normal(size=(C_, S_)) * spread[:, None] + centre[:, None]).astype(np.float32).reshape(-1)).to(dev)
    y = torch.as_tensor((rng.normal(size=(C_, S_)) * spread[:, None] * 1.2 + centre[:, None]).astype(np.float32).reshape(-1)).to(dev)
    off = (torch.arange(C_ + 1, dtype=torch.int64) * S_).to(dev)
    ws = torch.empty(E.mmd_workspace_bytes(C_), dtype=torch.uint8, device=dev)
    out["mmd_ms"] = kernel_ms(functools.partial(E.mmd_1d_segments, workspace=ws), (x, off, y, off), a.launches)
    pairs = C_ * 3 * S_ * S_
    tiles = -(-S_ // E.MMD_TILE)
    evaluated = C_ * (tiles * (tiles + 1) + tiles * tiles) * E.MMD_TILE ** 2
    sec = out["mmd_ms"]["median"] * 1e-3
    out.update(mmd_classes=C_, mmd_samples=S_, kernel_num=5, pairs=pairs, evaluated_pairs=evaluated,
               pair_bandwidths_per_s=pairs * 5 / sec, evaluated_pairs_per_s=evaluated / sec, v_exp_f32_per_s=V_EXP_PER_S,
               v_exp_share=evaluated / sec / V_EXP_PER_S)
    res, status = E.mmd_1d_segments(x, off, y, off, workspace=ws)
    out.update(mmd_mean=float(res[:, 0].mean()), mmd_ok=int((status == E.MMD_OK).sum()))
    if a.host_samples > 0:
        h = min(a.host_samples, S_)
        xs, ys = x[:h].contiguous(), y[:h].contiguous()
        one = torch.tensor([0, h], dtype=torch.int64, device=dev)
        on_gpu = float(E.mmd_1d_segments(xs, one, ys, one)[0][0, 0])
        xs, ys = xs.cpu(), ys.cpu()
        t0 = time.time()
        host = host_mmd(xs, ys)
        out.update(host_samples=h, host_torch_s=time.time() - t0, host_threads=torch.get_num_threads(), host_minus_gpu=host - on_gpu)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
