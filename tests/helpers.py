"""Shared test helpers: procedural state dicts without instantiating the GPU model, error measures, the fp64 evaluation of the oracle,
checkpoint-like weight statistics, the packed-pair <-> oracle-edge maps, and the record-pair runner of the evaluation kernels' GPU tests."""
from __future__ import annotations

import functools

import numpy as np
import torch

from diffspectra_amd import filler
from diffspectra_amd.config import qm9s_config
from diffspectra_amd.params import build_dmt_tree, Holder


@functools.lru_cache(maxsize=4)
def procedural_state_dict(version: str):
    """Reference-named state dict (no ``module.`` prefix) with procedural weights."""
    cfg = qm9s_config(spectra_version=version)
    tree = Holder()
    build_dmt_tree(tree, cfg)
    return cfg, filler.fill_state_dict(tree.state_dict())


def max_abs_diff(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).abs().max())


def relerr(a: torch.Tensor, b: torch.Tensor) -> float:
    """The suite's error measure of a kernel against its high-precision reference: max |a - b| / max |b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(a: torch.Tensor, b: torch.Tensor, tol: float, what: str) -> float:
    e = relerr(a, b)
    assert e <= tol, f"{what}: max |diff| / max |ref| = {e:.3e} (tol {tol:g})"
    return e


def to_dev(dev, a, dtype) -> torch.Tensor:
    """numpy array (any strides) -> contiguous tensor of ``dtype`` on ``dev``."""
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def run_records(fn, result_type, dev, ref, prb, ref_index=None, **kw):
    """``fn`` - a record-pair binding of ``engine`` - on ``ref`` and ``prb``, each a ``(records, n_atoms)`` pair of arrays or a list of molecule
    dicts (packed by ``structure_mirror.records``); ``kw``: the binding's scalars by name.  Synchronised; ``result_type`` of numpy arrays."""
    from tests.structure_mirror import records
    (rr, rn), (pr, pn) = (records(x) if isinstance(x, list) else x for x in (ref, prb))
    idx = None if ref_index is None else to_dev(dev, ref_index, torch.int64)
    out = fn(to_dev(dev, pr, torch.uint8), to_dev(dev, pn, torch.int32), to_dev(dev, rr, torch.uint8), to_dev(dev, rn, torch.int32), idx, **kw)
    torch.cuda.synchronize()
    return result_type(*(o.cpu().numpy() for o in out))


def oracle_forward_f64(sd, cfg, a, return_debug=False):
    """The oracle in fp64 (same code, default dtype switched): the truth both fp32 evaluations are measured against."""
    import oracle
    torch.set_default_dtype(torch.float64)
    try:
        dd = lambda t: None if t is None else ([x.double() for x in t] if isinstance(t, (list, tuple)) else t.double())
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        return oracle.dmt_forward(sd64, cfg, dd(a["xh"]), dd(a["node_mask"]), dd(a["edge_mask"]), dd(a["edge_x"]), dd(a["noise_level"]),
                                  dd(a["cond_x"]), dd(a["cond_edge_x"]), context=dd(a["context"]), return_debug=return_debug)
    finally:
        torch.set_default_dtype(torch.float32)


def checkpoint_like(sd):
    """Weight statistics a trained checkpoint can have and the U(+-1/sqrt(fan_in)) filler never does: adaLN scale / shift / gate
    outputs 30x larger (every block's node / edge / equi / dist time_mlp), a few residual-stream channels at 1e4 magnitude,
    weights with 1e-6 entries.  (The top-level 17 -> 1024 time MLP is left alone: scaling it as well makes the forward
    ill-conditioned - the fp32 CPU oracle itself is then 10 % away from fp64.)"""
    import re
    out = dict(sd)
    for key, v in sd.items():
        k = key[7:] if key.startswith("module.") else key
        if re.match(r"e_block_\d+\.(node_time_mlp|edge_time_mlp|equi_update\.time_mlp|dist_layer\.time_mlp)\.1\.", k):
            out[key] = v * 30.0
        elif k == "node_emb.weight":
            w = v.clone()
            w[[3, 77, 200]] *= 1e4                                      # three residual-stream channels ~1e4
            out[key] = w
        elif re.match(r"e_block_\d+\.(ff_linear1|ff_linear3|equi_update\.coord_mlp\.0)\.weight", k):
            w = v.clone()
            w[::3] *= 1e-5                                              # rows of ~1e-6 entries next to ordinary ones
            out[key] = w
    return out


def oracle_edge_maps(valid, node_dense, pair_a, pair_b):
    """Packed pair rows <-> the oracle's directed edge list (row-major nonzero order of the [B, N, N] mask).  ``valid`` [B, N] bool, ``node_dense``
    [Nn], ``pair_a`` / ``pair_b`` [Pp] (packed node rows).  Returns ``(fwd, bwd, node_dense)``: the oracle edge of every packed pair in direction
    a -> b and b -> a (so ``oracle_edges[fwd]`` is in packed order, and ``packed[inverse]`` with ``inverse[fwd] = p`` goes back)."""
    valid = torch.as_tensor(valid).bool()
    N = valid.shape[1]
    nd = torch.as_tensor(node_dense).cpu().long()
    pa, pb = nd[torch.as_tensor(pair_a).cpu().long()], nd[torch.as_tensor(pair_b).cpu().long()]
    adj = (valid.unsqueeze(1) & valid.unsqueeze(2)) & ~torch.eye(N, dtype=torch.bool).unsqueeze(0)
    eid = torch.full(adj.shape, -1, dtype=torch.long)
    eid[adj] = torch.arange(int(adj.sum()))
    b = pa // N
    return eid[b, pa % N, pb % N], eid[b, pb % N, pa % N], nd
