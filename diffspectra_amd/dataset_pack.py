"""Device-resident conditioning table for the sampler (conditioning side).

The reference assembles every sampling round in Python, one ``test_ds[i]`` at a time: PyG ``Data`` item → transform →
``torch.stack`` of 30.8 kB of spectra per molecule → host→device copy of the batch (``sampling.py:391-420``,
``datasets/qm9s_dataset.py:357-361``).  ``PackedSpectraTable`` walks the dataset ONCE, keeps the three spectra as
contiguous ``[M, 1, L]`` fp32 tensors and ``num_atom`` as ``int64[M]`` in HBM (10 000 molecules = 308 MB of 288 GB),
and hands a round its context with one ``index_select`` per spectrum: no Python per molecule, no PCIe per round.

It is a drop-in for the ``ds`` argument of ``get_cond_sampling_eval_fn`` / ``get_sampling_fn``: ``len()`` and
``[i]`` behave like the dataset it was built from (items expose ``uv / ir / raman / num_atom / pos / rdmol``), and the
sampling loop uses ``batch(ids)`` when the object has it.  ``normalize=True`` applies the reference transform's
``log10(x + 1)`` (``datasets/build_dataset.py:141-148``) for datasets that hold raw intensities.

``gt_records`` (optional): the ground-truth molecules as ``[M, 1248] u8`` records in the layout of ``shard.pack_records_u8``, resident on
the table's device - what ``structure_metrics`` scores sampled molecules against without RDKit.  ``None`` when the source carries no graph.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Sequence

import torch

from .config import SPECTRUM_LENGTHS, used_spectra

_NAMES = ("uv", "ir", "raman")
# A source carries the ground-truth graph only when it has ALL of these (qm9s_dataset.py:267-268); from_dataset and
# ProcessedQM9S.packed_table build gt_records under this one rule and leave it None otherwise (no charges are invented).
GRAPH_FIELDS = ("atom_type", "edge_index", "edge_type", "fc", "pos")


class PackedSpectraTable:
    def __init__(self, spectra: Sequence[Optional[torch.Tensor]], num_atom: torch.Tensor, pos: Optional[List] = None,
                 rdmol: Optional[List] = None, device="cpu", *, gt_records: Optional[torch.Tensor] = None):
        if len(spectra) != 3:
            raise ValueError("spectra = (uv, ir, raman); use None for a spectrum the model does not read")
        self.device = torch.device(device)
        self.num_atom = num_atom.to(torch.int64).reshape(-1).cpu()
        M = self.num_atom.numel()
        self.spectra = []
        for name, L, t in zip(_NAMES, SPECTRUM_LENGTHS, spectra):
            if t is None:
                self.spectra.append(None)
                continue
            t = t.to(torch.float32).reshape(M, 1, -1)
            if t.shape[-1] != L:
                raise ValueError(f"{name} spectra must have {L} points, got {t.shape[-1]}")
            self.spectra.append(t.contiguous().to(self.device))
        self.pos = list(pos) if pos is not None else [None] * M
        self.rdmol = list(rdmol) if rdmol is not None else [None] * M
        if len(self.pos) != M or len(self.rdmol) != M:
            raise ValueError("pos / rdmol lists must have one entry per molecule")
        self.gt_records = None
        if gt_records is not None:
            from .shard import RECORD_BYTES
            if gt_records.dtype != torch.uint8 or tuple(gt_records.shape) != (M, RECORD_BYTES):
                raise ValueError(f"gt_records must be uint8 [{M}, {RECORD_BYTES}], got {gt_records.dtype} {list(gt_records.shape)}")
            self.gt_records = gt_records.contiguous().to(self.device)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_dataset(cls, ds, spectra_version: str, device="cpu", normalize: bool = False) -> "PackedSpectraTable":
        """One pass over ``ds`` (items with ``uv/ir/raman [1, L]``, ``num_atom``, optional ``pos``, ``rdmol``); items that also carry
        every one of ``GRAPH_FIELDS`` (the reference's PyG items, ``qm9s_dataset.py:267-268``) fill ``gt_records``."""
        used = used_spectra(spectra_version)
        cols = [[] if k in used else None for k in range(3)]
        n_atoms, pos, mols, graphs = [], [], [], []
        for i in range(len(ds)):
            it = ds[i]
            for k in used:
                cols[k].append(torch.as_tensor(getattr(it, _NAMES[k]), dtype=torch.float32).reshape(1, -1))
            na = it.num_atom
            n_atoms.append(int(na.item()) if hasattr(na, "item") else int(na))
            pos.append(getattr(it, "pos", None))
            mols.append(getattr(it, "rdmol", None))
            if graphs is not None and all(getattr(it, f, None) is not None for f in GRAPH_FIELDS):
                graphs.append(it)
            else:
                graphs = None
        spectra = [torch.stack(c) if c is not None else None for c in cols]
        if normalize:
            spectra = [torch.log10(t + 1) if t is not None else None for t in spectra]    # build_dataset.py:141-148
        gt = None
        if graphs:
            from .structure_metrics import records_from_graph
            cum = lambda sizes: torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
            cat = lambda name, dim=0: torch.cat([torch.as_tensor(getattr(it, name)) for it in graphs], dim)
            gt = records_from_graph(cat("atom_type"), cat("pos"), cat("fc"), cat("edge_index", 1), cat("edge_type"),
                                    cum([int(torch.as_tensor(it.atom_type).numel()) for it in graphs]),
                                    cum([int(torch.as_tensor(it.edge_type).numel()) for it in graphs]))
        return cls(spectra, torch.tensor(n_atoms, dtype=torch.int64), pos, mols, device, gt_records=gt)

    # ------------------------------------------------------------------ dataset surface
    def __len__(self) -> int:
        return self.num_atom.numel()

    def __getitem__(self, i: int):
        i = int(i)
        item = SimpleNamespace(num_atom=self.num_atom[i], pos=self.pos[i], rdmol=self.rdmol[i])
        for name, t in zip(_NAMES, self.spectra):
            if t is not None:
                setattr(item, name, t[i])
        return item

    # ------------------------------------------------------------------ the sampler's fast path
    def batch(self, ids, spectra_version: str):
        """Context, n_nodes, ground-truth positions and molecules of one sampling round (``sampling.py:391-420``)."""
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        used = used_spectra(spectra_version)
        for k in used:
            if self.spectra[k] is None:
                raise ValueError(f"the table holds no {_NAMES[k]} spectra (built for another spectra_version)")
        dev_ids = ids.to(self.device)
        ctx = [self.spectra[k].index_select(0, dev_ids) for k in used]
        context = ctx if spectra_version == "allspectra" else ctx[0]
        idl = ids.tolist()
        return context, self.num_atom[ids].tolist(), [self.pos[i] for i in idl], [self.rdmol[i] for i in idl]
