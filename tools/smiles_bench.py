"""Time dsl_smiles_records (canonical SMILES of result records; csrc/ds_smiles.hip) beside ds_graph_hash_records and graph_classes on the same
records, and beside the CPU mirror.

    python tools/smiles_bench.py [--records 10000] [--distinct 2000] [--launches 50] [--mirror 300] [--out profiles/smiles_bench.json]

The records: `distinct` molecules of tests/graph_mirror.random_molecule (trees with 0-3 ring closures over H, C, N, O, F) at the QM9 size
mix of the evaluation half, tiled to `records` rows.  Prints one JSON line (and writes it to --out): the median, minimum and maximum time of
one call of each binding (HIP events around the call, after three warm-up calls; a call is one kernel launch and the allocation of its
outputs), the two kernels once more in the other order so that a drift of the clocks shows, the wall time of one `graph_classes` (several
launches and host synchronisations) and of one `smiles_strings` (the device-to-host copy and the Python strings), the share of rows with
`nodes > 0`, the statuses, and the wall time of tests/smiles_mirror.write on the first `mirror` records scaled to `records` records.  There
is no gate on any of these times.

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
from tests import graph_mirror as GM, smiles_mirror as L, structure_mirror as SM   # noqa: E402
from record_bench import kernel_ms, qm9_sizes                                 # noqa: E402  (this directory: the script's own)


def wall_ms(fn, repeats=5):
    """Median wall time in ms of ``fn()`` between two device synchronisations, after one warm-up call."""
    fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--distinct", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    rng = np.random.default_rng(11)
    mols = [GM.random_molecule(rng, int(k)) for k in qm9_sizes(rng, a.distinct)]
    rec, n = SM.records(mols)
    rows = np.arange(a.records) % len(n)
    dev = torch.device("cuda:0")
    rec_d, n_d = torch.as_tensor(rec[rows]).to(dev), torch.as_tensor(n[rows]).to(dev)
    out = {"records": a.records, "distinct_molecules": int(len(n)), "mean_atoms": float(n[rows].mean()), "launches": a.launches}
    out["smiles_ms"] = kernel_ms(E.smiles_records, (rec_d, n_d), a.launches)
    out["graph_hash_ms"] = kernel_ms(E.graph_hash_records, (rec_d, n_d), a.launches)
    out["graph_hash_ms_again"] = kernel_ms(E.graph_hash_records, (rec_d, n_d), a.launches)
    out["smiles_ms_again"] = kernel_ms(E.smiles_records, (rec_d, n_d), a.launches)
    out["graph_classes_wall_ms"] = wall_ms(lambda: S.graph_classes(rec_d, n_d))
    found = S.smiles(rec_d, n_d)
    out["smiles_strings_wall_ms"] = wall_ms(lambda: S.smiles_strings(found))
    out["smiles_then_unique_wall_ms"] = wall_ms(lambda: len(set(S.smiles_strings(S.smiles(rec_d, n_d)))))
    nodes, status = found.nodes.cpu().numpy(), found.status.cpu().numpy()
    out["rows_with_nodes"] = float((nodes > 0).mean())
    out["max_nodes"] = int(nodes.max())
    out["statuses"] = [int((status == k).sum()) for k in range(4)]
    out["mean_length"] = float(found.length.float().mean())
    strings = S.smiles_strings(found)
    out["distinct_strings"] = len(set(strings))
    out["graph_classes"] = int(S.graph_classes(rec_d, n_d).unique().numel())
    if a.mirror:
        k = min(a.mirror, len(n))
        t0 = time.time()
        want = L.write_table(rec[:k], n[:k])
        out["mirror_records"] = k
        out["mirror_s_scaled"] = (time.time() - t0) * a.records / k
        out["mirror_rows_equal"] = sum(w["text"].decode() == strings[p] and w["nodes"] == int(nodes[p]) for p, w in enumerate(want))
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
