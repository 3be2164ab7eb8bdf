"""Evaluation driver + checkpoint contract ("next" row N2 of SURVEY §8f).

Mirror of the sampling half of reference ``run_lib.diffspectra_evaluate`` (``run_lib.py:297-370``) and of the
checkpoint helpers (``utils.py:7-30``, ``models/ema.py``): build the model through the factory, restore
``checkpoints/checkpoint_{k}.pth`` (``{'optimizer', 'model', 'ema', 'step'}``, ``model`` keys ``module.``-prefixed,
``ema['shadow_params']`` a list in ``parameters()`` order), copy the EMA weights into the model and run the
conditional sampling function.  The reference's RDKit / MOSES / FCD metric stack (``run_lib.py:371-441``) is host-side
analytics outside this path; callers plug metrics in as callbacks that receive ``processed_mols`` in the reference's
tuple format.  (The reference's own ``run_lib`` cannot be imported as shipped: ``import visualize`` has no module.)
"""
from __future__ import annotations

import logging
import os
from typing import Callable, Dict, Optional

import torch

from .ema import ExponentialMovingAverage  # noqa: F401  (re-exported: the checkpoint contract's EMA holder)
from .noise_schedule import NoiseScheduleVP
from .registry import create_model
from .sampling import get_cond_sampling_eval_fn
from .scalers import get_data_inverse_scaler


def restore_checkpoint(ckpt_path: str, state: Dict, device) -> Dict:
    """utils.py:7-20: strict model load, EMA + step restored; the optimizer entry is optional on the inference path."""
    if not os.path.exists(ckpt_path):
        os.makedirs(os.path.dirname(ckpt_path) or ".", exist_ok=True)
        logging.warning("No checkpoint found at %s. Returned the same state as input", ckpt_path)
        return state
    loaded = torch.load(ckpt_path, map_location=device)
    if state.get("optimizer") is not None and "optimizer" in loaded:
        state["optimizer"].load_state_dict(loaded["optimizer"])
    state["model"].load_state_dict(loaded["model"], strict=True)
    state["ema"].load_state_dict(loaded["ema"])
    state["step"] = loaded["step"]
    return state


def save_checkpoint(ckpt_path: str, state: Dict) -> None:
    """utils.py:23-30.  In a multi-rank job EVERY rank calls this (the sharded optimizer / EMA state is gathered by collectives
    inside ``state_dict()``); rank 0 writes the file."""
    saved = {}
    if state.get("optimizer") is not None:            # same key order as the reference's file
        saved["optimizer"] = state["optimizer"].state_dict()
    saved.update(model=state["model"].state_dict(), ema=state["ema"].state_dict(), step=state["step"])
    from .shard import world_info
    if world_info()[0] == 0:
        torch.save(saved, ckpt_path)


def checkpoint_ids(config):
    """run_lib.py:326-331: explicit comma list or the inclusive begin..end range."""
    ckpts = getattr(config.eval, "ckpts", "")
    if ckpts != "":
        return [int(c) for c in str(ckpts).split(",")]
    return list(range(config.eval.begin_ckpt, config.eval.end_ckpt + 1))


def _structure_summary(run, table, top_k: int) -> Dict:
    """The structure metric of one finished sharded run: every sample slot's record against the ground-truth record of its dataset item."""
    from .structure_metrics import (graph_classes, graph_identity_batch, hungarian_rmsd_batch, mces_batch, morgan_similarity_batch, topk_identity,
                                    topk_mces, topk_morgan, topk_summary)
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    per_pair = hungarian_rmsd_batch(ref, prb, engine=run.eng, ref_index=run.slot_ds, raw=True)
    ok = per_pair.valid
    n_ok, P = int(ok.sum()), ok.numel()
    mean = lambda t: float(t[ok].double().mean()) if n_ok else None
    rmsd = per_pair.rmsd.cpu()
    out = dict(rmsd_list=[None if v != v else v for v in rmsd.tolist()], success_rate=n_ok / P if P else 0.0, mean_rmsd=mean(per_pair.rmsd),
               mean_atom_type_accuracy=mean(per_pair.type_acc), mean_bond_accuracy=mean(per_pair.bond_acc),
               exact_rate=float(per_pair.exact.double().mean()) if P else 0.0, per_pair=per_pair)
    if top_k > 1:
        out["top_k"] = topk_summary(per_pair, top_k)
    # graph identity: the conformation-independent decision behind Top-1 / Top-K accuracy, and the uniqueness of what was generated
    same = graph_identity_batch(ref, prb, ref_index=run.slot_ds, engine=run.eng)
    classes = graph_classes(prb[0], prb[1], engine=run.eng)
    graph = dict(verdict=same.verdict, identity_rate=float(same.identical.double().mean()) if P else 0.0, undecided=int(same.undecided.sum()),
                 unique_fraction=classes.unique().numel() / P if P else 0.0)
    if top_k > 1:
        graph["top_k"] = topk_identity(same.verdict, top_k)
    out["graph"] = graph
    # MCES distance: how far a wrong molecule is from the right one (hydrogens left out, as in the reference's SMILES route)
    far = mces_batch(ref, prb, ref_index=run.slot_ds, engine=run.eng)
    valid = far.status != 3
    n_valid = int(valid.sum())
    mces = dict(dist=far.dist, status=far.status, mean=float(far.dist[valid].double().mean()) if n_valid else None,
                zero_rate=float((far.dist[valid] == 0).double().mean()) if n_valid else 0.0, undecided=int(far.undecided.sum()))
    if top_k > 1:
        mces["top_k"] = topk_mces(far.dist, far.status, top_k)
    out["mces"] = mces
    # Morgan fingerprints: the graded similarity next to the identity verdict (radius 2, 2048 bits, heavy atoms, as the reference)
    alike = morgan_similarity_batch(ref, prb, ref_index=run.slot_ds, engine=run.eng)
    valid = alike.valid
    n_valid = int(valid.sum())
    tanimoto, cosine = alike.tanimoto, alike.cosine
    mean = lambda t: float(t[valid].cpu().mean()) if n_valid else None          # (summed on the host: one order of summation everywhere)
    fingerprint = dict(tanimoto=tanimoto, cosine=cosine, status=alike.status, mean_tanimoto=mean(tanimoto), mean_cosine=mean(cosine))
    if top_k > 1:
        fingerprint["top_k"] = topk_morgan(tanimoto, top_k)
    out["fingerprint"] = fingerprint
    return out


def _functional_group_summary(run, table, top_k: int) -> Dict:
    """The reference's "Functional Group Similarity" line of one finished run (the pairs of ``_structure_summary``), and how often each group
    occurs among the generated molecules."""
    from .structure_metrics import FUNCTIONAL_GROUP_NAMES, _host_sum, functional_group_similarity_batch, topk_groups
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    alike = functional_group_similarity_batch(ref, prb, ref_index=run.slot_ds, engine=run.eng)
    ok = alike.valid
    n_ok, P = int(ok.sum()), ok.numel()
    mine = alike.groups[:, 0]
    rate = lambda g: float((torch.bitwise_and(mine, 1 << g) != 0).sum()) / P if P else 0.0
    entry = dict(similarity=alike.similarity, status=alike.status, mean=_host_sum(alike.similarity[ok]) / n_ok if n_ok else None,
                 undefined=P - n_ok, presence_rate={name: rate(g) for g, name in enumerate(FUNCTIONAL_GROUP_NAMES)})
    if top_k > 1:
        entry["top_k"] = topk_groups(alike.similarity, alike.status, top_k)
    return entry


def _maccs_summary(run, table, top_k: int, max_nodes: Optional[int] = None) -> Dict:
    """The reference's "Tanimoto Similarity (MACCS)" line of one finished run (the pairs of ``_structure_summary``); ``max_nodes``: the search
    budget per start atom, ``None`` for the header's default."""
    from .structure_metrics import _host_sum, maccs_similarity_batch, topk_maccs
    dev = run.records_by_slot.device
    alike = maccs_similarity_batch(run.records_by_slot, torch.tensor(run.n_atoms), table.gt_records.to(dev), table.num_atom, ref_index=run.slot_ds,
                                   max_nodes=max_nodes, engine=run.eng)
    ok = alike.valid
    n_ok = int(ok.sum())
    entry = dict(tanimoto=alike.tanimoto, status=alike.status, mean=_host_sum(alike.tanimoto[ok]) / n_ok if n_ok else None, scored=n_ok,
                 truncated=int((alike.truncated & ok).sum()))
    if top_k > 1:
        entry["top_k"] = topk_maccs(alike.tanimoto, alike.status, top_k)
    return entry


def _fraggle_summary(run, table, top_k: int, max_nodes: Optional[int] = None) -> Dict:
    """The reference's "Fraggle similarity" line of one finished run (the pairs of ``_structure_summary``; the ground truth is the molecule
    that is fragmented); ``max_nodes``: the bond sets one fingerprint may have, ``None`` for the header's default."""
    from .structure_metrics import _host_sum, fraggle_similarity_batch, topk_fraggle
    dev = run.records_by_slot.device
    alike = fraggle_similarity_batch(run.records_by_slot, torch.tensor(run.n_atoms), table.gt_records.to(dev), table.num_atom, ref_index=run.slot_ds,
                                     max_nodes=max_nodes, engine=run.eng)
    ok = alike.valid
    n_ok = int(ok.sum())
    entry = dict(fraggle=alike.fraggle, status=alike.status, mean=_host_sum(alike.fraggle[ok]) / n_ok if n_ok else None, scored=n_ok,
                 undecided=int((alike.status == 1).sum()), unusable=int((alike.status == 2).sum()),
                 no_fragmentation=int((ok & (alike.n_fragmentations == 0)).sum()))
    if top_k > 1:
        entry["top_k"] = topk_fraggle(alike.fraggle, alike.status, top_k)
    return entry


def _stereo_summary(run, table, top_k: int, min_volume: Optional[float] = None, min_planarity: Optional[float] = None) -> Dict:
    """The stereo-aware Top-1 / Top-K of one finished run (the pairs of ``_structure_summary``): ``dsc_stereo_identity_records`` per slot, and
    how many of the slots' ground truths are chiral.  The thresholds: ``None`` for the header's defaults."""
    from .structure_metrics import chirality, stereo_identity_batch, topk_identity
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    same = stereo_identity_batch(ref, prb, ref_index=run.slot_ds, min_volume=min_volume, min_planarity=min_planarity, engine=run.eng)
    P = same.verdict.numel()
    rate = lambda hit: float(hit.double().mean()) if P else 0.0
    slot_rows = torch.as_tensor(run.slot_ds).to(device=dev, dtype=torch.int64)
    targets = chirality(ref[0], ref[1], min_volume=min_volume, min_planarity=min_planarity, engine=run.eng).chiral[slot_rows]
    entry = dict(verdict=same.verdict, identity_rate=rate(same.identical), constitution_rate=rate(same.same_constitution),
                 enantiomer_rate=rate(same.mirror), stereoisomer_rate=rate(same.stereoisomer), unassigned=int(same.unassigned.sum()),
                 undecided=int(same.undecided.sum()), sites=same.sites, chiral_targets=rate(targets == 1))
    if top_k > 1:
        entry["top_k"] = topk_identity(same.verdict, top_k)
    return entry


def _mobile_summary(run, table, top_k: int, max_nodes: int = 4096) -> Dict:
    """Top-1 / Top-K up to mobile hydrogens, acid / base forms and Kekule drawings of one finished run (the pairs of ``_structure_summary``):
    ``mobile_identity_batch`` per slot."""
    from .structure_metrics import mobile_identity_batch, topk_identity
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    same = mobile_identity_batch(ref, prb, ref_index=run.slot_ds, max_nodes=max_nodes, engine=run.eng)
    P = same.verdict.numel()
    rate = lambda hit: float(hit.double().mean()) if P else 0.0
    entry = dict(verdict=same.verdict, layer=same.layer, identity_rate=rate(same.identical), strict_rate=rate(same.strict == 1),
                 normalised_hits=int((same.layer == 1).sum()), undecided=int(same.undecided.sum()), invalid=int((same.verdict == 3).sum()))
    if top_k > 1:
        entry["top_k"] = topk_identity(same.verdict, top_k)
    return entry


def _key_summary(run, table, top_k: int, max_nodes: int = 4096, min_volume: Optional[float] = None, min_planarity: Optional[float] = None) -> Dict:
    """Top-1 / Top-K at the level of an InChIKey of one finished run (the pairs of ``_structure_summary``): ``key_identity_batch`` per slot -
    the normal form of ``_mobile_summary`` and the stereo verdicts of ``_stereo_summary`` at once.  Unpinned against InChI."""
    from .structure_metrics import key_identity_batch, topk_identity
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    same = key_identity_batch(ref, prb, ref_index=run.slot_ds, max_nodes=max_nodes, min_volume=min_volume, min_planarity=min_planarity, engine=run.eng)
    P = same.verdict.numel()
    rate = lambda hit: float(hit.double().mean()) if P else 0.0
    entry = dict(verdict=same.verdict, layer=same.layer, identity_rate=rate(same.identical), strict_rate=rate(same.strict == 1),
                 normalised_hits=int((same.layer == 1).sum()), mirror=int(same.mirror.sum()), stereoisomer=int(same.stereoisomer.sum()),
                 unassigned=int(same.unassigned.sum()), undecided=int(same.undecided.sum()), invalid=int((same.verdict == 3).sum()),
                 sites=same.sites)
    if top_k > 1:
        entry["top_k"] = topk_identity(same.verdict, top_k)
    return entry


BEST_RMSD_THRESHOLDS = (0.1, 0.25, 0.5, 1.0)      # Angstrom; definitions of "close", not measurements


def _best_rmsd_summary(run, table, top_k: int, atoms: str = "heavy", max_nodes: int = 4096, thresholds=BEST_RMSD_THRESHOLDS) -> Dict:
    """How good the geometry of every hit of one finished run is (the pairs of ``_structure_summary``): ``best_rmsd_batch`` per slot, the
    smallest Kabsch RMSD over all graph isomorphisms.  A HIT is a slot with verdict 1; ``mean`` / ``median`` / ``within`` are over the hits
    with a finite value (``None`` / empty shares without any).  The ``thresholds`` of ``within`` are definitions, not measurements: nobody
    has measured where the values of generated molecules fall."""
    from .structure_metrics import best_rmsd_batch, topk_best_rmsd
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    best = best_rmsd_batch(ref, prb, ref_index=run.slot_ds, atoms=atoms, max_nodes=max_nodes, engine=run.eng)
    hit = best.verdict == 1
    proper = best.rmsd[:, 0]
    values = proper[hit & torch.isfinite(proper)].cpu()                # (summed on the host: one order of summation everywhere)
    n = values.numel()
    entry = dict(verdict=best.verdict, rmsd=best.rmsd, hits=int(hit.sum()), undecided=int((best.verdict == 2).sum()),
                 invalid=int((best.verdict == 3).sum()), mean=float(values.mean()) if n else None, median=float(values.median()) if n else None,
                 mirror_better=int(best.mirror_better.sum()),
                 within={float(t): float((values < float(t)).double().mean()) if n else None for t in thresholds})
    if top_k > 1:
        entry["top_k"] = topk_best_rmsd(best, top_k)
    return entry


def _scaffold_summary(run, table, top_k: int, scaffold_fn, min_rings: int) -> Dict:
    """The "Scaf" number of one finished run against the test table (``scaffold_fn``: ``get_scaffold_metric`` of its records) and, over the
    pairs of ``_structure_summary``, whether every generated molecule shares the scaffold of its ground truth."""
    from .structure_metrics import scaffold_identity_batch, topk_identity
    dev = run.records_by_slot.device
    ref, prb = (table.gt_records.to(dev), table.num_atom), (run.records_by_slot, torch.tensor(run.n_atoms))
    entry = dict(scaffold_fn(prb))
    alike = scaffold_identity_batch(ref, prb, ref_index=run.slot_ds, min_rings=1, engine=run.eng)
    ok = alike.status == 0
    n_ok = int(ok.sum())
    same = dict(same=alike.same, status=alike.status, rate=int(alike.same[ok].sum()) / n_ok if n_ok else None, undecided=int(alike.undecided))
    if top_k > 1:
        top = topk_identity(alike.same.to(torch.uint8), top_k)                   # 1 = same scaffold; a pair that is not ok is a miss
        same["top_k"] = dict(hit=top["hit"], first_hit=top["first_hit"], acc_at_k=top["acc_at_k"])
    entry["same_scaffold"] = same
    entry["min_rings"] = min_rings
    return entry


def _smiles_summary(run, table, top_k: int, path: Optional[str] = None) -> Dict:
    """The molecules of one finished run as text (``structure_metrics.smiles``): the generated strings by slot, the ground-truth strings of the
    same slots, the reference's "Exact Match (SMILES)" over the pairs of ``_structure_summary``, and the file of ``config.eval.smiles_path``."""
    from .shard import world_info
    from .structure_metrics import smiles, smiles_exact_match, smiles_strings, topk_identity
    dev = run.records_by_slot.device
    gen = smiles(run.records_by_slot, torch.tensor(run.n_atoms), engine=run.eng)
    truth = smiles(table.gt_records.to(dev), table.num_atom, engine=run.eng)
    match = smiles_exact_match(truth, gen, ref_index=run.slot_ds)
    generated, table_strings = smiles_strings(gen), smiles_strings(truth)
    ground_truth = [table_strings[r] if 0 <= r < len(table_strings) else None for r in torch.as_tensor(run.slot_ds).reshape(-1).tolist()]
    status = gen.status.cpu().tolist()
    certified = [s for s, st in zip(generated, status) if st == 0]
    ok = match.status == 0
    n_ok = int(ok.sum())
    entry = dict(generated=generated, ground_truth=ground_truth, same=match.same, status=gen.status, pair_status=match.status,
                 exact_match=int(match.same.sum()) / n_ok if n_ok else None, unique=len(set(certified)) / len(certified) if certified else None,
                 distinct=len(set(certified)), certified=len(certified), uncertified=status.count(1), overflow=status.count(2), unusable=status.count(3))
    if top_k > 1:
        top = topk_identity(match.same.to(torch.uint8), top_k)                   # 1 = the same string; a pair that is not certified is a miss
        entry["top_k"] = dict(hit=top["hit"], first_hit=top["first_hit"], acc_at_k=top["acc_at_k"])
    if path and world_info()[0] == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            for slot, (g, t) in enumerate(zip(generated, ground_truth)):
                f.write(f"{slot}\t{'' if g is None else g}\t{'' if t is None else t}\n")
    return entry


def diffspectra_evaluate(config, workdir: str, test_ds=None, eval_folder: str = "eval",
                         metric_fns: Optional[Dict[str, Callable]] = None, structure_metrics: bool = False, known_records=None):
    """Sampling evaluation over the configured checkpoints; returns ``{ckpt: {'processed_mols', 'gt_pos', 'gt_rdmols',
    'metrics'}}``.  ``metric_fns[name](processed_mols, gt_pos, gt_rdmols)`` are optional host-side callbacks.

    ``structure_metrics=True`` (needs a table with ``gt_records`` and the philox noise source) adds ``metrics['structure']``, computed on the
    GPU from the run's ``records_by_slot`` (``structure_metrics.py``; no RDKit): ``rmsd_list, success_rate, mean_rmsd,
    mean_atom_type_accuracy`` of ``eval_sampled_mols/rmsd.py:232-273``, ``mean_bond_accuracy``, ``exact_rate`` and the raw ``per_pair``
    device tensors; with ``config.eval.top_k`` = K > 1 the run draws K candidates per spectrum and ``'top_k'`` holds ``topk_summary``.
    ``metrics['structure']['graph']`` is the reference's headline number without RDKit: ``verdict`` (device tensor of
    ``ds_graph_identity_records``: 1 = the generated molecule IS the ground-truth graph, in any conformation), ``identity_rate`` (Top-1
    accuracy over all slots), ``undecided`` (pairs whose search ran out of budget; they count as misses), ``unique_fraction`` of the
    generated records (``graph_classes``) and, with K > 1, ``top_k = topk_identity(...)`` whose ``acc_at_k`` is the Top-K accuracy.  Identity
    is constitution-level (atom type, formal charge, bond order): unlike the reference's InChIKey comparison (``compute_metrics.py:222-230``)
    it has no stereo layer and no InChI normalisation of tautomers or charges (``config.eval.mobile_identity`` below adds the latter).
    ``metrics['structure']['mces']`` grades the misses: ``dist`` / ``status`` (device tensors of ``ds_mces_records``: the exact
    maximum-common-edge-subgraph distance of every slot's molecule from its ground truth on heavy atoms, bond weight = bond order; status 0
    exact, 2 undecided = ``dist`` is an upper bound, 3 invalid), ``mean`` over the valid pairs (the reference's "MCES (Average)",
    ``compute_metrics.py:235-243``), ``zero_rate``, ``undecided`` and, with K > 1, ``top_k = topk_mces(...)``.  Two deviations from the
    reference's number: the records hold Kekule orders 1..3, not RDKit's aromatic 1.5 (two Kekule drawings of o-xylene are 2 apart), and
    parity with the ``myopic_mces`` package itself is unpinned, because it cannot be run here.
    ``metrics['structure']['fingerprint']`` is the similarity of radius-2 Morgan fingerprints folded to 2048 bits, hydrogens left out
    (``ds_morgan_similarity_records``; the reference's "Tanimoto (Morgan)" and "Cosine (Morgan)", ``compute_metrics.py:246-253``):
    ``tanimoto`` / ``cosine`` (f64 device tensors, one per slot; NaN for an invalid row), ``status`` (0 ok, 3 invalid), ``mean_tanimoto`` /
    ``mean_cosine`` over the valid pairs (``None`` without any) and, with K > 1, ``top_k = topk_morgan(...)``.  Deviations from the
    reference's number: Kekule orders 1..3 instead of aromatic bonds (the two Kekule drawings of o-xylene share 5 of 10 + 10 features),
    RDKit's own invariant hash and fold are not reproduced (values differ where 2048-bit collisions differ), and the hydrogens enter as a
    count in the atom invariant, the reference's SMILES route.

    With ``config.eval.sub_geometry`` true (the reference's ``evaluate.sub_geometry``, ``configs/diffspectra_qm9s.py:145``)
    ``metrics['structure']['sub_geometry']`` is the reference's "Metric-Align" dict (``run_lib.py:392-411``): the bond-length, bond-angle and
    dihedral-angle MMD between the generated records and ALL records of the test table for every QM9 substructure symbol, and
    ``bond_length_mean`` / ``bond_angle_mean`` / ``dihedral_angle_mean`` (``structure_metrics.get_sub_geometry_metric``, which states the
    deviations: every angle counts once, RDKit parity unpinned, a seeded sample cap).  Without the flag the dict has no such key.

    With ``config.eval.set_similarity`` true ``metrics['structure']['set_similarity']`` holds the set-level numbers of the reference's
    "Metric-2D" line that need no RDKit model (``run_lib.py:346-390``): ``snn`` and ``int_div`` of the generated records against ALL records of
    the test table, ``nearest`` / ``nearest_index`` (device tensors: every kept generated molecule's similarity to, and the table row of, its
    nearest test molecule), ``n_generated`` / ``n_test`` and, when ``known_records = (records [*, 1248] u8, n_atoms [*])`` of the training
    molecules is given, ``novelty`` (``structure_metrics.get_set_similarity_metric``, which states the deviations: the MOSES definitions are
    restated and unpinned, one representative per constitution-level class stands for ``set(smiles)``, no RDKit sanitisation filter; FCD is
    not computed (Scaf: ``get_scaffold_metric``, Frag: ``get_fragment_metric``)).  Without the flag the dict has no such key.

    With ``config.eval.scaffold`` true ``metrics['structure']['scaffold']`` is the "Scaf" number of the same line
    (``evaluation/mose_metric.py:111-113``): the dict of ``structure_metrics.get_scaffold_metric`` of the generated records against ALL records
    of the test table (``scaf``, the cosine similarity of the Bemis-Murcko scaffold counts; ``n_generated`` / ``n_test``, ``with_scaffold_*``,
    ``distinct_*``, ``shared``, ``scaffold_class``, ``mean_rings``), with ``min_rings`` = ``config.eval.scaffold_min_rings`` when present, else
    MOSES's 2, reported as ``min_rings``; and ``same_scaffold``: per slot, does the generated molecule share the scaffold of its ground truth
    (``scaffold_identity_batch`` with ``min_rings=1``: ``same`` and ``status`` device tensors, ``rate`` over the ok pairs - ``None`` without
    any -, ``undecided`` and, with K > 1, ``top_k`` with ``hit`` / ``first_hit`` / ``acc_at_k`` as ``topk_identity`` shapes them: a hit is any
    candidate of the target that shares its scaffold).  The scaffold rule restates RDKit's and MOSES's as remembered and is unpinned against
    both (``include/diffspectra_scaffold.h``).  Without the flag the dict has no such key.

    With ``config.eval.fragments`` true ``metrics['structure']['fragments']`` is the "Frag" number of the same line
    (``evaluation/mose_metric.py:88-128``): the dict of ``structure_metrics.get_fragment_metric`` of the generated records against ALL records of
    the test table (``frag``, the cosine similarity of the BRICS fragment counts; ``n_generated`` / ``n_test``, ``fragments_*``, ``distinct_*``,
    ``shared``, ``mean_cuts``, ``fragment_class`` with ``owner``).  The BRICS rules restate RDKit's and MOSES's as remembered and are unpinned against
    both; the project's aromaticity, labelled-graph identity, no sanitisation filter (``include/diffspectra_brics.h``).  Without the flag the dict
    has no such key.

    With ``config.eval.edm_metrics`` true ``metrics['structure']['metric_2d']`` and ``['metric_3d']`` are the reference's first two evaluation
    lines (``run_lib.py:371-387``): ``mol_stable``, ``atom_stable``, ``Validity``, ``Complete``, ``Unique`` and ``Novelty`` (against
    ``known_records``; -1 without) of the generated records, from the predicted bonds and charges and from the distance-derived bonds, plus
    the per-record device tensors ``valence``, ``valid`` and ``largest`` (``structure_metrics.get_edm_metric_2d`` / ``get_edm_metric_3d``, which
    state the deviations: RDKit's valence check restated and unpinned, constitution-level identity, Kekule orders only, ``n = 0`` counted as
    unusable).  Without the flag the dict has no such keys.  ``set_similarity`` stays as it is with both flags set - the reference filters its
    set metrics by RDKit sanitisation, and a caller who wants that passes the mask on:
    ``get_set_similarity_metric(test)(generated, keep=metrics['structure']['metric_2d']['valid'])``.

    With ``config.eval.functional_groups`` true ``metrics['structure']['functional_groups']`` is the reference's "Functional Group Similarity"
    (``compute_metrics.py:117-144``, ``dsg_group_similarity_records``): ``similarity`` (f64 device tensor, one per slot: the Jaccard index of the
    groups present in the generated molecule and in its ground truth, 1.0 when neither has one, NaN for a pair that is not ok), ``status`` (0
    ok, 2 a record of the pair is unusable, 3 invalid), ``mean`` over the ok pairs (summed on the host; ``None`` without any), ``undefined`` (the
    pairs that are not ok), ``presence_rate`` (group name -> fraction of the generated molecules that have it) and, with K > 1, ``top_k =
    topk_groups(...)`` (``structure_metrics.functional_group_similarity_batch``, which states the deviations: the project's own aromaticity
    rule, unpinned against RDKit; every usable pair is scored, with no RDKit filter).  Without the flag the dict has no such key.

    With ``config.eval.maccs`` true ``metrics['structure']['maccs']`` is the reference's "Tanimoto Similarity (MACCS)" (``compute_metrics.py:248-252``;
    ``dsq_match_records`` with the key table of ``maccs.py``): ``tanimoto`` (f64 device tensor, one per slot: common / either of the 166 keys of
    the generated molecule and of its ground truth, 1.0 when neither sets a key, NaN for a pair that is not ok), ``status`` (0 ok, 2 a record
    of the pair is unusable, 3 invalid), ``mean`` over the ok pairs (summed on the host; ``None`` without any), ``scored`` (the ok pairs), ``truncated``
    (the ok pairs with a search that stopped at its budget - ``config.eval.maccs_max_nodes`` assignments per start atom, the header's
    default when absent; such keys are a lower bound) and, with K > 1, ``top_k = topk_maccs(...)``.  The key table restates RDKit's as remembered: parity with RDKit is unpinned
    (``structure_metrics.maccs_similarity_batch``).  Without the flag the dict has no such key.

    With ``config.eval.fraggle`` true ``metrics['structure']['fraggle']`` is the reference's "Fraggle similarity" (``compute_metrics.py:273-291``,
    ``GetFraggleSimilarity(true_mol, pred_mol)``; ``dsf_fraggle_similarity_records``): ``fraggle`` (f64 device tensor, one per slot: 0 when the
    ground truth has no fragmentation, else the larger of the plain path-fingerprint Tanimoto and the best Tanimoto of the marked molecules over
    all fragmentations; NaN for a pair that is not ok), ``status`` (0 ok, 1 undecided, 2 a record of the pair is unusable, 3 invalid), ``mean``
    over the ok pairs (summed on the host; ``None`` without any), ``scored`` (the ok pairs), ``undecided`` (a fingerprint needed more than
    ``config.eval.fraggle_max_nodes`` bond sets, the header's default when absent), ``unusable``, ``no_fragmentation`` (the ok pairs scored 0
    for that reason) and, with K > 1, ``top_k = topk_fraggle(...)``.  The rule restates RDKit's Fraggle as remembered, with the project's own
    fingerprint hash and aromaticity: parity with RDKit is unpinned (``include/diffspectra_fraggle.h`` names every deviation).  Without the
    flag the dict has no such key.

    With ``config.eval.stereo`` true ``metrics['structure']['stereo']`` is the stereo-aware Top-1 (``dsc_stereo_identity_records``; the reference's
    Top-1 compares InChIKeys, ``compute_metrics.py:222-230``, which ``metrics['structure']['graph']`` does at constitution level only): ``verdict``
    (u8 device tensor, one per slot: 0 different, 1 identical, 2 undecided, 3 invalid, 4 mirror image, 5 another stereoisomer, 6 a site too
    flat to tell), ``identity_rate`` (verdict 1 over all slots), ``constitution_rate`` (1, 4, 5 or 6: what ``graph`` calls identical),
    ``enantiomer_rate`` (4), ``stereoisomer_rate`` (5), ``unassigned`` and ``undecided`` (counts: how much hangs on the two thresholds and on the
    budget), ``sites`` (i32 device tensor [slots, 4]: tetrahedral and E/Z sites of the generated molecule, unassigned sites of it and of its
    ground truth), ``chiral_targets`` (the fraction of the slots whose ground truth is chiral: a tetrahedral site and no mirror automorphism) and,
    with K > 1, ``top_k = topk_identity(verdict, K)``.  ``config.eval.stereo_min_volume`` / ``stereo_min_planarity`` replace the header's 0.5 /
    0.5; they are definitions, nobody has measured how generated molecules distribute around them.  Four-coordinate centres and double bonds
    only, no InChI normalisation, parity with RDKit / InChI unpinned (``include/diffspectra_stereo.h``).  Without the flag the dict has no such key.

    With ``config.eval.mobile_identity`` true ``metrics['structure']['mobile']`` is Top-1 up to mobile hydrogens (tautomers), acid / base forms
    and Kekule drawings (``structure_metrics.mobile_identity_batch``: ``graph_identity_batch`` on the normal forms of ``dsm_normal_records``;
    the level of the main layer of the standard InChI behind the reference's Top-1, ``compute_metrics.py:222-230``): ``verdict`` (u8 device
    tensor, one per slot: 0 different, 1 identical, 2 undecided, 3 invalid), ``layer`` (i8: 0 identical as drawn, 1 identical only after the
    normalisation, -1 not identical), ``identity_rate`` (verdict 1 over all slots), ``strict_rate`` (what ``graph`` calls identical),
    ``normalised_hits`` (the slots with layer 1), ``undecided`` and ``invalid`` (counts) and, with K > 1, ``top_k = topk_identity(verdict, K)``.
    ``config.eval.mobile_max_nodes`` replaces the budget of 4096.  The rule restates InChI's as remembered and is unpinned against it; the
    stereo layer is not combined with it there (``include/diffspectra_mobile.h``); ``config.eval.key_identity`` below combines the two.
    Without the flag the dict has no such key.

    With ``config.eval.key_identity`` true ``metrics['structure']['key']`` is Top-1 at the level of an InChIKey - the normal form above AND
    the stereo verdicts, at once (``structure_metrics.key_identity_batch``; ``include/diffspectra_key.h``): ``verdict`` (u8 device tensor, one
    per slot, the codes of ``stereo`` above), ``layer``, ``identity_rate`` (the Top-1), ``strict_rate`` (the stereo-aware Top-1 on the records
    as drawn), ``normalised_hits`` (hits with layer 1), ``mirror``, ``stereoisomer``, ``unassigned``, ``undecided`` and ``invalid`` (counts),
    ``sites`` and, with K > 1, ``top_k``.  ``config.eval.key_max_nodes`` replaces the budget of 4096; the thresholds are those of ``stereo``.
    Every rule restates InChI as remembered: the number is unpinned against InChI.  Without the flag the dict has no such key.

    With ``config.eval.best_rmsd`` true ``metrics['structure']['best_rmsd']`` says how good the geometry of every hit is: the smallest Kabsch
    RMSD over ALL graph isomorphisms between the generated molecule and its ground truth (``structure_metrics.best_rmsd_batch``;
    ``include/diffspectra_rmsd.h``; what RDKit's ``GetBestRMS`` and ``spyrmsd`` compute, where ``rmsd_list`` above is the reference's Hungarian
    match): ``verdict`` (u8 device tensor, one per slot: 0 no isomorphism, 1 a hit with its values, 2 undecided, 3 invalid), ``rmsd`` (f64 device
    tensor [slots, 2]: the best fit by a rotation and the best fit of the mirror image, NaN unless verdict 1), ``hits``, ``undecided`` and
    ``invalid`` (counts, which with the slots of verdict 0 add up to the slots), ``mean`` and ``median`` (of the proper value over the hits with a
    finite one, ``None`` without any), ``mirror_better`` (hits whose mirror image fits better), ``within`` (``{threshold: share of those hits
    below it}`` for ``config.eval.best_rmsd_thresholds``, default 0.1, 0.25, 0.5 and 1.0 Angstrom: definitions of "close", not measurements -
    nobody has measured where generated molecules fall) and, with K > 1, ``top_k = topk_best_rmsd(...)``.  ``config.eval.best_rmsd_atoms``
    (``'heavy'``, the default, or ``'all'``) and ``config.eval.best_rmsd_max_nodes`` (4096) pass through.  Unpinned against RDKit / spyrmsd, no
    mass weighting, the ``'all'`` mode is bound by the budget.  Without the flag the dict has no such key.

    With ``config.eval.smiles`` true ``metrics['structure']['smiles']`` holds the molecules as text, where the reference calls ``Chem.MolToSmiles``
    (``run_lib.py:111-112``, ``compute_metrics.py:73-78,209-220``; ``dsl_smiles_records``): ``generated`` (one canonical SMILES string per slot,
    ``None`` for an overflow or unusable record), ``ground_truth`` (the string of every slot's ground truth), ``same`` / ``status`` / ``pair_status``
    (device tensors: the strings are certified and equal; the generated row's status 0 ok, 1 uncertified, 2 overflow, 3 unusable; the pair's),
    ``exact_match`` (the reference's "Exact Match (SMILES)": the rate of ``same`` over the pairs with both sides certified, ``None`` without
    any), ``unique`` (distinct strings over the certified generated rows, ``None`` without any; ``distinct`` and ``certified`` are the two
    counts), ``uncertified`` / ``overflow`` / ``unusable`` (counts of generated rows) and, with K > 1, ``top_k`` with ``hit`` / ``first_hit`` /
    ``acc_at_k`` as ``topk_identity`` shapes them.  With ``config.eval.smiles_path`` set, rank 0 also writes one ``slot<TAB>generated<TAB>ground
    truth`` line per slot there (an empty field for ``None``).  The strings are canonical for this project, not RDKit's canonical form
    (``include/diffspectra_smiles.h`` states the deviations).  Without the flag the dict has no such key.

    ``test_ds=None`` reads the reference's processed files under ``config.data.root`` (``run_lib.py:313`` ->
    ``build_dataset.py:31-42``: the 'test' entry of ``split_dict_diffspectra_qm9.pt``) into the device-resident table of
    ``qm9s_reader.ProcessedQM9S.packed_table`` - no PyG, no per-molecule Python."""
    os.makedirs(os.path.join(workdir, eval_folder), exist_ok=True)
    if test_ds is None:
        from .qm9s_reader import ProcessedQM9S
        test_ds = ProcessedQM9S(config.data.root).packed_table(
            config.data.spectra_version, split="test", device=config.device, normalize=getattr(config.data, "use_normalize", True))
    model = create_model(config)
    ema = ExponentialMovingAverage(model.parameters(), decay=config.model.ema_decay)
    state = dict(optimizer=None, model=model, ema=ema, step=0)
    logging.info("model size: %.1fMB", sum(p.numel() for p in model.parameters()) * 4 / 2 ** 20)
    noise_scheduler = NoiseScheduleVP(config.sde.schedule, continuous_beta_0=config.sde.continuous_beta_0,
                                      continuous_beta_1=config.sde.continuous_beta_1)
    inverse_scaler = get_data_inverse_scaler(config)
    top_k = int(getattr(config.eval, "top_k", 1)) if structure_metrics else 1
    if structure_metrics and getattr(test_ds, "gt_records", None) is None:
        raise ValueError("structure_metrics=True needs a test_ds with gt_records (PackedSpectraTable built from a source that holds the "
                         "molecular graphs: atom_type, edge_index, edge_type, fc, pos)")
    sampling_fn = get_cond_sampling_eval_fn(config, noise_scheduler, config.eval.batch_size, config.eval.num_samples,
                                            inverse_scaler, test_ds, top_k=top_k)
    results = {}
    geometry_fn = None                            # the test side of the geometry MMD is extracted once, at the first checkpoint
    set_fn = None                                 # and so are the bit rows of the test molecules
    edm_fns = None
    scaffold_fn = None                            # and the scaffolds of the test molecules
    fragment_fn = None                            # and their BRICS fragments
    for ckpt in checkpoint_ids(config):
        ckpt_path = os.path.join(workdir, "checkpoints", "checkpoint_{}.pth".format(ckpt))
        if not os.path.exists(ckpt_path):
            raise FileNotFoundError("Checkpoint path error: " + ckpt_path)
        logging.info("load checkpoint: %s", ckpt_path)
        state = restore_checkpoint(ckpt_path, state, device=config.device)
        ema.copy_to(model.parameters())          # eval uses EMA weights; BatchNorm buffers stay the model's (run_lib.py:361-362)
        if structure_metrics:
            run = sampling_fn.start(model)
            with torch.no_grad():
                run.advance()
                processed_mols, gt_pos, gt_rdmols = run.finish()
        else:
            processed_mols, gt_pos, gt_rdmols = sampling_fn(model)
        metrics = {name: fn(processed_mols, gt_pos, gt_rdmols) for name, fn in (metric_fns or {}).items()}
        if structure_metrics:
            metrics["structure"] = _structure_summary(run, test_ds, top_k)
            if getattr(config.eval, "functional_groups", False):
                metrics["structure"]["functional_groups"] = _functional_group_summary(run, test_ds, top_k)
            if getattr(config.eval, "maccs", False):
                metrics["structure"]["maccs"] = _maccs_summary(run, test_ds, top_k, getattr(config.eval, "maccs_max_nodes", None))
            if getattr(config.eval, "fraggle", False):
                metrics["structure"]["fraggle"] = _fraggle_summary(run, test_ds, top_k, getattr(config.eval, "fraggle_max_nodes", None))
            if getattr(config.eval, "stereo", False):
                metrics["structure"]["stereo"] = _stereo_summary(run, test_ds, top_k, getattr(config.eval, "stereo_min_volume", None),
                                                                 getattr(config.eval, "stereo_min_planarity", None))
            if getattr(config.eval, "mobile_identity", False):
                metrics["structure"]["mobile"] = _mobile_summary(run, test_ds, top_k, int(getattr(config.eval, "mobile_max_nodes", 4096)))
            if getattr(config.eval, "key_identity", False):
                metrics["structure"]["key"] = _key_summary(run, test_ds, top_k, int(getattr(config.eval, "key_max_nodes", 4096)),
                                                           getattr(config.eval, "stereo_min_volume", None),
                                                           getattr(config.eval, "stereo_min_planarity", None))
            if getattr(config.eval, "best_rmsd", False):
                metrics["structure"]["best_rmsd"] = _best_rmsd_summary(run, test_ds, top_k, getattr(config.eval, "best_rmsd_atoms", "heavy"),
                                                                       int(getattr(config.eval, "best_rmsd_max_nodes", 4096)),
                                                                       tuple(getattr(config.eval, "best_rmsd_thresholds", BEST_RMSD_THRESHOLDS)))
            if getattr(config.eval, "sub_geometry", False):
                from .structure_metrics import get_sub_geometry_metric
                if geometry_fn is None:
                    geometry_fn = get_sub_geometry_metric((test_ds.gt_records.to(run.records_by_slot.device), test_ds.num_atom), engine=run.eng)
                metrics["structure"]["sub_geometry"] = geometry_fn((run.records_by_slot, torch.tensor(run.n_atoms)))
            if getattr(config.eval, "set_similarity", False):
                from .structure_metrics import get_set_similarity_metric
                if set_fn is None:
                    dev = run.records_by_slot.device
                    known = None if known_records is None else (known_records[0].to(dev), known_records[1])
                    set_fn = get_set_similarity_metric((test_ds.gt_records.to(dev), test_ds.num_atom), known=known, engine=run.eng)
                metrics["structure"]["set_similarity"] = set_fn((run.records_by_slot, torch.tensor(run.n_atoms)))
            if getattr(config.eval, "scaffold", False):
                from .structure_metrics import get_scaffold_metric
                min_rings = int(getattr(config.eval, "scaffold_min_rings", 2))
                if scaffold_fn is None:
                    scaffold_fn = get_scaffold_metric((test_ds.gt_records.to(run.records_by_slot.device), test_ds.num_atom), min_rings=min_rings,
                                                      engine=run.eng)
                metrics["structure"]["scaffold"] = _scaffold_summary(run, test_ds, top_k, scaffold_fn, min_rings)
            if getattr(config.eval, "fragments", False):
                from .structure_metrics import get_fragment_metric
                if fragment_fn is None:
                    fragment_fn = get_fragment_metric((test_ds.gt_records.to(run.records_by_slot.device), test_ds.num_atom), engine=run.eng)
                metrics["structure"]["fragments"] = fragment_fn((run.records_by_slot, torch.tensor(run.n_atoms)))
            if getattr(config.eval, "smiles", False):
                metrics["structure"]["smiles"] = _smiles_summary(run, test_ds, top_k, getattr(config.eval, "smiles_path", None))
            if getattr(config.eval, "edm_metrics", False):
                from .structure_metrics import get_edm_metric_2d, get_edm_metric_3d
                if edm_fns is None:
                    dev = run.records_by_slot.device
                    known = None if known_records is None else (known_records[0].to(dev), known_records[1])
                    edm_fns = dict(metric_2d=get_edm_metric_2d(known=known, engine=run.eng), metric_3d=get_edm_metric_3d(known=known, engine=run.eng))
                for key, fn in edm_fns.items():
                    metrics["structure"][key] = fn(run.records_by_slot, torch.tensor(run.n_atoms))
        results[ckpt] = dict(processed_mols=processed_mols, gt_pos=gt_pos, gt_rdmols=gt_rdmols, metrics=metrics, step=state["step"])
    return results
