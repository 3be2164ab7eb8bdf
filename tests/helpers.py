"""Shared test helpers: procedural state dicts without instantiating the GPU model."""
from __future__ import annotations

import functools

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
