"""Shared test helpers: procedural state dicts without instantiating the GPU model, error measures, and the record-pair runner of the
evaluation kernels' GPU tests."""
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
