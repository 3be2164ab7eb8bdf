"""What the record bench tools (match_bench.py, graph_bench.py, mces_bench.py, morgan_bench.py) share: the event-timed launch loop and the draw
of molecule sizes at the QM9 size mix.  Imported by them as scripts (their directory is on ``sys.path``), after the repository root has been added."""
import numpy as np
import torch

from diffspectra_amd.config import QM9_SECOND_HALF_N_NODES


def kernel_ms(fn, args, launches):
    """{"median", "min", "max"} in ms of ``launches`` calls ``fn(*args)``, each between two HIP events, after three warm-up calls."""
    for _ in range(3):
        fn(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def qm9_sizes(rng, count):
    """``count`` atom counts drawn from the QM9 size census of the evaluation half."""
    sizes, counts = zip(*sorted(QM9_SECOND_HALF_N_NODES.items()))
    return rng.choice(sizes, size=count, p=np.array(counts) / sum(counts))
