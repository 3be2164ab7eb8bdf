"""Structural quality of sampled molecules without RDKit: Hungarian-matched RMSD, atom-type accuracy and certified Top-K hits.

The reference scores structures with ``eval_sampled_mols/rmsd.py``: largest fragment of each RDKit molecule, a Hungarian atom match with
atom-type penalties, a Kabsch fit on that match, a second, distance-clipped match, then the RMSD and the atom-type accuracy of the final
map (``rmsd.py:12-73``) - one pair at a time, with a Python double loop per cost matrix.  Here the same five steps run in ONE launch of
``ds_match_records`` (one wave per pair, fp64, ``csrc/ds_match.hip``; semantics in ``include/diffspectra_hip.h``) on the 1 248-byte records
the sampler already holds on the GPU (``shard.pack_records_u8``), against ground-truth records built from the processed file's plain
tensors (``records_from_graph``).  Two outputs go beyond the reference: ``bond_acc`` and ``exact`` - the kernel's atom map either is or is
not a graph isomorphism, so ``exact = 1`` is a *certified* hit.  ``exact = 0`` proves nothing (a correct graph in another conformation can
be matched atom-for-atom differently), so hit@K computed from it is a LOWER bound on Top-K accuracy.

The accuracy itself - is a generated molecule THE ground-truth molecule - is ``graph_identity_batch`` / ``topk_identity``: a
conformation-independent decision per pair by ``ds_graph_identity_records`` (``csrc/ds_graph.hip``), and ``graph_classes`` gives the
uniqueness figure of ``evaluation/rdkit_metric.py`` from a permutation-invariant hash plus the same decision.  Identity here is
constitution-level (atom type, formal charge, bond order under a bijection, whole molecules): it is NOT InChIKey identity - no stereo
layer, no InChI normalisation of tautomers or charges (``mobile_identity_batch`` compares at that level).

How far a wrong molecule is from the right one is ``mces_batch`` / ``topk_mces``: the exact maximum-common-edge-subgraph distance per pair by
``ds_mces_records`` (``csrc/ds_mces.hip``), the reference's "MCES (Average)" (``compute_metrics.py:235-243``: one ``myopic_mces`` ILP per
pair).  It deviates from that number in two stated ways: Kekule bond orders 1..3 instead of RDKit's aromatic 1.5, and parity with the
``myopic_mces`` package itself is unpinned (it cannot be run here).

How similar it is in the field's most quoted number is ``morgan_similarity_batch`` / ``topk_morgan``: Tanimoto and cosine similarity of
radius-2 Morgan fingerprints (``ds_morgan_similarity_records``, ``csrc/ds_morgan.hip``), the reference's "Tanimoto (Morgan)" and "Cosine
(Morgan)" (``compute_metrics.py:246-253``); ``morgan_fingerprints`` gives the per-molecule fingerprint.  Deviations from that number:
Kekule orders instead of aromatic bonds, RDKit's own invariant hash and fold are not reproduced (bit-for-bit parity is unpinned), and
``drop_h`` is the reference's SMILES route.

Whether the 3-D conformations are right as a DISTRIBUTION is ``get_sub_geometry_metric``: the reference's bond-length, bond-angle and
dihedral-angle MMD between generated and test molecules per substructure symbol (``evaluation/cal_geometry.py``, ``evaluation/mmd.py``; its
"Metric-Align" line).  ``sub_geometry`` extracts the samples (``ds_geometry_count_records`` / ``ds_geometry_fill_records``,
``csrc/ds_subgeom.hip``), ``mmd_1d`` / ``ds_mmd_1d_segments`` (``csrc/ds_mmd.hip``) is ``compute_mmd``.  Deviations: every angle counts once
(the reference counts it 0, 1 or 2 times depending on the atom numbering), parity with RDKit's angle functions is unpinned, and the
20 000-sample cap is a seeded ``torch.randperm``.

How a generated SET stands against another set is ``get_set_similarity_metric``: the SNN, IntDiv and novelty of the reference's "Metric-2D"
line (``run_lib.py:346-390``, ``evaluation/mose_metric.py``, ``evaluation/rdkit_metric.py:45-65,113-122``).  ``morgan_bit_rows`` packs the
fingerprints into bit rows (``dss_fold_bits``), ``nearest_neighbour_similarity`` scans every generated row against every test row
(``dss_tanimoto_nn``, ``csrc/ds_sets.hip``; the nearest neighbour is decided in integers, the sums have one fixed order), ``snn`` and
``internal_diversity`` reduce it, ``novelty`` is ``graph_classes`` on the known and the generated molecules together.  The MOSES definitions
(``SNNMetric``; ``internal_diversity`` with p = 1, self-pairs included; 1024-bit radius-2 Morgan fingerprints) are restated from the package as
remembered - MOSES is neither vendored by the reference nor runnable here, so parity with it is unpinned - and the fingerprints carry the
deviations of ``morgan_similarity_batch``.  FCD is not computed (Scaf: ``get_scaffold_metric``, Frag: ``get_fragment_metric``).

How the ring systems of a generated set stand against the test set's is ``get_scaffold_metric``: the "Scaf" number of the same line
(``evaluation/mose_metric.py:111-113``), the cosine similarity of the Bemis-Murcko scaffold counts.  ``scaffolds`` gives the per-molecule
scaffold atoms, ring atoms and ring count (``dsk_scaffold_masks``, ``csrc/ds_scaffold.hip``; every definition in
``include/diffspectra_scaffold.h``), ``scaffold_records`` the scaffold as a record of its own, ``scaffold_identity_batch`` the per-pair agreement.
Deviations: the scaffold rule (the 2-core of the heavy graph plus the atoms multiply bonded to it) restates RDKit's ``GetScaffoldForMol`` and
MOSES's ``compute_scaffolds`` as remembered and is unpinned against both; scaffold identity is constitution-level on Kekule orders unless
``bond_orders=False``; there is no RDKit sanitisation filter.

How the building blocks of a generated set stand against the test set's is ``get_fragment_metric``: the "Frag" number of the same line
(``evaluation/mose_metric.py:88-128``), the cosine similarity of the BRICS fragment counts.  ``brics`` gives the per-molecule environments,
cut bonds with their labels and fragments (``dsb_brics_records``, ``csrc/ds_brics.hip``; every definition in ``include/diffspectra_brics.h``),
``brics_fragment_records`` every fragment as a record of its own with its attachment points.  Deviations: the environments and rules restate
RDKit's ``BRICS.py`` and MOSES's ``compute_fragments`` as remembered and are unpinned against both; the project's aromaticity rule is used;
fragment identity is that of the labelled graph, not of a SMILES string; there is no RDKit sanitisation filter; sulfur never occurs; a bond
that fits a rule in both orientations gives both ends the rule's first label.

Whether the generated molecules are chemically sound is ``get_edm_metric_2d`` / ``get_edm_metric_3d``: the reference's first two evaluation lines,
"Metric-3D || atom stability, mol stability, validity, complete" and "Metric-2D || ..., unique & valid, unique & valid & novelty"
(``run_lib.py:371-387``; ``evaluation/stability.py:76-230``, ``evaluation/rdkit_metric.py:86-129``).  ``valence_batch`` gives the per-record
valences, stability, validity and fragments (``dsv_valence_records``, ``csrc/ds_valence.hip``; definitions in ``include/diffspectra_valence.h``) from
the predicted bond orders and charges (2-D) or from bond orders derived from the distances with ``ds_check_stability``'s arithmetic (3-D);
``largest_fragment_records`` turns every molecule's largest fragment into a record of its own (``dsv_fragment_records``), which is what lets
``graph_classes``, ``novelty``, ``morgan_bit_rows`` and the set metrics run on largest fragments and on distance-derived graphs.  Deviations: the
validity restates RDKit's valence check (no aromatic bonds exist in a record, so nothing else of ``Chem.SanitizeMol`` can fail) and is
unpinned against RDKit; ``Unique`` / ``Novelty`` count constitution-level classes of the explicit graph where the reference counts canonical
SMILES; the records hold Kekule orders only; a record with ``n = 0`` (or with a byte outside the alphabet) is UNUSABLE: it counts in every
denominator and in no numerator, where the reference would count an empty molecule as stable and valid.

Whether a generated molecule carries the ground truth's chemistry is ``functional_group_similarity_batch`` / ``topk_groups``: the reference's
"Functional Group Similarity" (``compute_metrics.py:117-144``: the Jaccard index of the sets of functional groups present, 17 patterns,
``compute_metrics.py:38-56``).  ``functional_groups`` gives the per-molecule group word and the aromatic atoms (``dsg_group_records``,
``csrc/ds_groups.hip``; every definition in ``include/diffspectra_groups.h``).  Unlike every metric above it does not take the Kekule orders at
face value: it perceives aromatic atoms by the project's own, order-free rule (C, N, O; simple cycles of 5 and 6 atoms; six electrons), so
both Kekule drawings of a ring give the same groups.  Deviations: that rule restates RDKit's default model as remembered and is unpinned
against RDKit (fused perimeters, other ring sizes, O+ and S are not perceived); the predicates restate the reference's patterns on the record
graph with implicit hydrogens filled to the valence table of ``valence_batch``; sulfide and thiol are never present (no sulfur among the five
types); and every usable pair is scored, where the reference sees only molecules that survived RDKit - ``valence_batch(...).valid`` filters.

What the molecules are as TEXT is ``smiles`` / ``smiles_strings``: one canonical SMILES string per record (``dsl_smiles_records``,
``csrc/ds_smiles.hip``; every definition in ``include/diffspectra_smiles.h``), which is what the reference gets from ``Chem.MolToSmiles``
(``run_lib.py:111-112``, ``compute_metrics.py:73-78``, ``evaluation/mose_metric.py:12-21``); ``smiles_exact_match`` is its ``true_smi == pred_smi``
(``compute_metrics.py:209-220``).  Deviations: the strings are canonical for THIS project, not RDKit's canonical form (compare them as
molecules, never as text, with strings from elsewhere); the graph is the constitution-level one of ``graph_identity_batch`` with raw charge
bytes; Kekule orders only, so two drawings of a ring give one string only where a symmetry maps one onto the other; any SMILES reader reads them.

The way in FROM text is ``read_smiles`` / ``records_from_smiles`` / ``pack_smiles``: one result record per SMILES string (``dsp_read_smiles``,
``csrc/ds_reader.hip``; every definition in ``include/diffspectra_reader.h``), which is what the reference gets from ``Chem.MolFromSmiles``
(``compute_metrics.py:96-114,147-317``, ``evaluation/rdkit_metric.py:86``); ``text_metrics`` builds the reference's metric table for text pairs on
it.  Deviations: an OpenSMILES subset over H, C, N, O, F, not RDKit's reader (parity unpinned); no sanitisation (``valence_batch`` checks the
record); stereo marks, isotopes and classes are read and dropped with a flag; lower-case input gets the first Kekule structure of a stated
search; positions are zero, so nothing that reads geometry applies to a read record.

Whether a molecule contains a substructure, how many times and on which atoms is ``substructure_search`` (``dsq_match_records``,
``csrc/ds_substructure.hip``; every definition in ``include/diffspectra_substructure.h``): patterns are data, a SMARTS subset compiled by
``smarts.py``.  On top of it ``maccs_keys`` / ``maccs_similarity_batch`` / ``topk_maccs`` give the 166 MACCS keys and the reference's "Tanimoto
Similarity (MACCS)" (``compute_metrics.py:248-252``) from the key table of ``maccs.py``, which restates RDKit's as remembered: parity with RDKit
is unpinned.

The reference's "Fraggle Similarity" (``compute_metrics.py:273-291``) is ``fraggle_similarity_batch`` / ``topk_fraggle``
(``dsf_fraggle_similarity_records``, ``csrc/ds_fraggle.hip``; every definition in ``include/diffspectra_fraggle.h``): the ground truth is
fragmented by one to three cuts, every fragmentation marks the atoms of both molecules that it does not explain, and the best Tanimoto of the
marked pair's path fingerprints, or the plain one if larger, is the similarity; ``fraggle_fragmentations`` and ``path_fingerprints`` show the
parts.  The rule restates RDKit's Fraggle as remembered with the project's own fingerprint hash: parity with RDKit is unpinned.

How good the geometry of a hit is says ``best_rmsd_batch`` / ``topk_best_rmsd`` (``dsr_best_rmsd_records``, ``csrc/ds_bestrmsd.hip``; every
definition in ``include/diffspectra_rmsd.h``): the smallest Kabsch RMSD over all graph isomorphisms of the pair, what RDKit's ``GetBestRMS``
and ``spyrmsd`` compute, with the best fit of the mirror image beside it.  Unlike the Hungarian-matched RMSD above it is rotation invariant
and bond consistent, and symmetry cannot inflate it.  Unpinned against RDKit / spyrmsd, no mass weighting.

One rule restates RDKit behaviour that cannot be executed here (RDKit is absent): among equally large fragments the one holding the lowest
atom index wins (``Chem.GetMolFrags`` lists fragments by their first atom, Python's ``max`` keeps the first maximum, ``rmsd.py:84-86``).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence

import torch

from . import shard


class PairMetrics(NamedTuple):
    """Per-pair device tensors of ``ds_match_records``."""
    rmsd: torch.Tensor        # [P] f64, NaN for an invalid pair
    n_matched: torch.Tensor   # [P] i32
    type_acc: torch.Tensor    # [P] f32
    bond_acc: torch.Tensor    # [P] f32
    exact: torch.Tensor       # [P] u8
    map: torch.Tensor         # [P, 29] i32, -1 where unmatched

    @property
    def valid(self) -> torch.Tensor:
        return ~torch.isnan(self.rmsd)


def records_from_graph(atom_type: torch.Tensor, pos: torch.Tensor, fc: torch.Tensor, edge_index: torch.Tensor,
                       edge_type: torch.Tensor, node_slices: torch.Tensor, edge_slices: torch.Tensor, ids=None,
                       atom_type_list: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Ground-truth records ``[len(ids), 1248] u8`` from the collated tensors of the processed file (``qm9s_dataset.py:267-268``), in the
    conventions of ``train_data.edge_com_transform``: an atom's type is its position in ``atom_type_list`` (QM9: H, C, N, O, F), bond code 4
    (aromatic) counts as no bond, and the directed edge list is summed into the dense ``[n, n]`` matrix.  ``node_slices`` / ``edge_slices`` are
    the cumulative offsets of the molecules along ``atom_type`` / ``edge_type``; ``edge_index`` is ``[2, E]`` with molecule-local atom indices.
    No Python per molecule."""
    from .train_data import QM9_ATOM_TYPES
    W = shard.RECORD_ATOMS
    types = torch.tensor(list(QM9_ATOM_TYPES if atom_type_list is None else atom_type_list), dtype=torch.int64)
    node_slices, edge_slices = node_slices.to(torch.int64).cpu(), edge_slices.to(torch.int64).cpu()
    n_mol = node_slices.numel() - 1
    ids = torch.arange(n_mol) if ids is None else torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()
    n, ne = node_slices[1:] - node_slices[:-1], edge_slices[1:] - edge_slices[:-1]
    if ids.numel() and int(n[ids].max()) > W:
        raise ValueError(f"records hold at most {W} atoms")
    # one record per DISTINCT molecule of ids, then the rows of ids are gathered (Top-K tables repeat molecules)
    uniq = torch.unique(ids)
    row = torch.full((n_mol,), -1, dtype=torch.int64)
    row[uniq] = torch.arange(uniq.numel())
    K = uniq.numel()
    mol_n = torch.repeat_interleave(torch.arange(n_mol), n)           # molecule and local index of every atom of the collated tensors
    loc_n = torch.arange(mol_n.numel()) - node_slices[:-1][mol_n]
    mol_e = torch.repeat_interleave(torch.arange(n_mol), ne)
    keep_n, keep_e = row[mol_n] >= 0, row[mol_e] >= 0
    rn, ln = row[mol_n][keep_n], loc_n[keep_n]
    one_hot = atom_type.reshape(-1, 1).to(torch.int64).cpu()[keep_n] == types.unsqueeze(0)      # build_dataset.py:111-114
    if not bool(one_hot.any(1).all()):
        raise ValueError("atom_type outside atom_type_list")
    pos_d, at_d, fc_d = torch.zeros(K, W, 3), torch.zeros(K, W, dtype=torch.int64), torch.zeros(K, W, dtype=torch.int64)
    pos_d[rn, ln] = pos.reshape(-1, 3).to(torch.float32).cpu()[keep_n]
    at_d[rn, ln] = one_hot.to(torch.int64).argmax(1)
    fc_d[rn, ln] = fc.reshape(-1).to(torch.int64).cpu()[keep_n]
    bond = edge_type.reshape(-1).to(torch.float32).cpu()[keep_e]
    bond[bond == 4] = 0                                               # build_dataset.py:118-119
    ei = edge_index.to(torch.int64).cpu()[:, keep_e]
    if ei.numel() and (int(ei.min()) < 0 or bool((ei >= n[mol_e][keep_e].unsqueeze(0)).any())):
        raise ValueError("edge_index outside its molecule")
    et_d = torch.zeros(K * W * W)
    et_d.scatter_add_(0, row[mol_e][keep_e] * (W * W) + ei[0] * W + ei[1], bond)               # build_dataset.py:128-131
    et_d = et_d.round().clamp_(0, 255).reshape(K, W, W)
    return shard.pack_records_u8(pos_d, at_d, fc_d, et_d)[row[ids]].contiguous()


def _pair_call(name, engine, ref, prb, ref_index, *scalars):
    """``engine.<name>`` (the module's function without an engine) on ``(records, n_atoms)`` pairs, ground truth first: the counts and
    ``ref_index`` are converted to the device and dtype the binding wants, the records are passed as they are."""
    from . import engine as E
    (ref_rec, ref_n), (prb_rec, prb_n) = ref, prb
    i32 = lambda t: torch.as_tensor(t).to(device=prb_rec.device, dtype=torch.int32).contiguous()
    idx = None if ref_index is None else torch.as_tensor(ref_index).to(device=prb_rec.device, dtype=torch.int64).contiguous()
    return getattr(engine if engine is not None else E, name)(prb_rec, i32(prb_n), ref_rec, i32(ref_n), idx, *scalars)


def hungarian_rmsd_batch(ref, prb, max_distance: float = 5.0, min_atoms: int = 3, engine=None, ref_index=None, raw: bool = False):
    """``hungarian_rmsd_batch`` of ``eval_sampled_mols/rmsd.py:232-273`` on record tensors.  ``ref`` and ``prb`` are ``(records [*, 1248] u8,
    n_atoms [*])`` pairs on the GPU (ground truth first, as in the reference's signature); ``ref_index [P]`` names the ground-truth row of
    every generated molecule (``None``: row p for pair p), so the K candidates of a spectrum share one row.

    Returns ``(rmsd_list, success_rate, mean_rmsd, mean_atom_type_accuracy)``: ``None`` for an invalid pair, the success rate over all
    pairs, the means over the valid pairs (``None`` without any).  ``raw=True`` returns the ``PairMetrics`` of device tensors instead and
    does not synchronise."""
    out = PairMetrics(*_pair_call("match_records", engine, ref, prb, ref_index, max_distance, min_atoms))
    if raw:
        return out
    rmsd = out.rmsd.cpu()
    ok = ~torch.isnan(rmsd)
    n_ok, P = int(ok.sum()), rmsd.numel()
    rmsd_list = [float(v) if k else None for v, k in zip(rmsd.tolist(), ok.tolist())]
    success_rate = n_ok / P if P else 0.0
    mean_rmsd = float(rmsd[ok].mean()) if n_ok else None
    mean_acc = float(out.type_acc.cpu()[ok].double().mean()) if n_ok else None
    return rmsd_list, success_rate, mean_rmsd, mean_acc


def topk_summary(per_pair, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions over the K consecutive candidates of every spectrum (``processed_mols[i*K:(i+1)*K]``).  ``per_pair``: a
    ``PairMetrics`` or any object / dict with ``rmsd [S*K]`` (NaN = invalid) and ``exact [S*K]``.  Plain torch reductions on the tensors'
    device: ``best_rmsd [S] f64`` (NaN when all K candidates are invalid), ``best_index [S] i64`` (candidate with the lowest RMSD, -1 when
    all are invalid), ``hit [S] bool`` (any candidate certified exact) and ``hit_at_k`` (their mean, a 0-dim f64 tensor; a lower bound on
    Top-K accuracy)."""
    get = (lambda k: per_pair[k]) if isinstance(per_pair, dict) else (lambda k: getattr(per_pair, k))
    rmsd, exact = get("rmsd"), get("exact")
    if top_k < 1 or rmsd.numel() % top_k:
        raise ValueError(f"{rmsd.numel()} pairs are not a whole number of top_k = {top_k} groups")
    r = rmsd.reshape(-1, top_k).to(torch.float64)
    bad = torch.isnan(r)
    filled = torch.where(bad, torch.full_like(r, float("inf")), r)
    best, arg = filled.min(dim=1)
    none = bad.all(dim=1)
    best = torch.where(none, torch.full_like(best, float("nan")), best)
    arg = torch.where(none, torch.full_like(arg, -1), arg)
    hit = exact.reshape(-1, top_k).bool().any(dim=1)
    hit_at_k = hit.double().mean() if hit.numel() else torch.zeros((), dtype=torch.float64, device=hit.device)
    return dict(best_rmsd=best, best_index=arg, hit=hit, hit_at_k=hit_at_k)


# ------------------------------------------------------------------------------------------------------------------ graph identity

class GraphIdentity(NamedTuple):
    """Per-pair device tensors of ``ds_graph_identity_records``."""
    verdict: torch.Tensor     # [P] u8: 1 identical (map is a checked isomorphism), 0 different (proven), 2 undecided (budget), 3 invalid row
    nodes: torch.Tensor       # [P] i32 search nodes used
    map: torch.Tensor         # [P, 29] i32 ground-truth atom of every generated atom when identical, else -1

    @property
    def identical(self) -> torch.Tensor:
        return self.verdict == 1

    @property
    def undecided(self) -> torch.Tensor:
        return self.verdict == 2


def graph_identity_batch(ref, prb, ref_index=None, max_nodes: int = 4096, engine=None) -> GraphIdentity:
    """Constitution-level identity (atom type, formal charge, bond order; no stereo - ``stereo_identity_batch`` -, no tautomer / charge
    normalisation - ``mobile_identity_batch`` -: not InChIKey identity) of every generated molecule with its ground truth, independent of the conformation.  ``ref`` and ``prb`` are ``(records
    [*, 1248] u8, n_atoms [*])`` pairs on the GPU, ground truth first as in ``hungarian_rmsd_batch``; ``ref_index [P]`` names the ground-truth
    row of every generated molecule (``None``: row p).  Device tensors, no synchronisation."""
    return GraphIdentity(*_pair_call("graph_identity_records", engine, ref, prb, ref_index, max_nodes))


def topk_identity(verdict: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Top-K accuracy over the K consecutive candidates of every spectrum from the verdicts of ``graph_identity_batch``: ``hit [S] bool`` (a
    candidate is the ground-truth graph), ``first_hit [S] i64`` (index of the first such candidate, -1 if none), ``acc_at_k`` (mean of ``hit``, a
    0-dim f64 tensor) and ``undecided`` (0-dim i64 count).  An undecided pair counts as a miss, so with ``undecided > 0`` the accuracy is a
    lower bound, short by at most ``undecided / S``.  The accuracy is over constitution-level identity, not InChIKeys."""
    if top_k < 1 or verdict.numel() % top_k:
        raise ValueError(f"{verdict.numel()} pairs are not a whole number of top_k = {top_k} groups")
    same = (verdict == 1).reshape(-1, top_k)
    hit = same.any(dim=1)
    first = torch.where(hit, same.to(torch.uint8).argmax(dim=1), torch.full_like(hit, -1, dtype=torch.int64))
    acc = hit.double().mean() if hit.numel() else torch.zeros((), dtype=torch.float64, device=hit.device)
    return dict(hit=hit, first_hit=first, acc_at_k=acc, undecided=(verdict == 2).sum())


def graph_classes(records: torch.Tensor, n_atoms, engine=None) -> torch.Tensor:
    """``class_id [P] i64``: the lowest row whose molecule is the same labelled graph as row p's (``unique_fraction = class_id.unique().numel()
    / P``, the uniqueness of ``evaluation/rdkit_metric.py`` at constitution level).  Rows are bucketed by ``ds_graph_hash_records``; inside a
    bucket every row is compared with the bucket's lowest unassigned row by ``ds_graph_identity_records`` (the table is its own ground
    truth), and the rows that differ go round again - as many launches as the fullest bucket has classes, no Python per molecule.  An
    undecided comparison raises."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    hash_fn, same_fn = (engine.graph_hash_records, engine.graph_identity_records) if engine is not None else (E.graph_hash_records, E.graph_identity_records)
    P = records.shape[0]
    rows = torch.arange(P, device=records.device)
    _, bucket = torch.unique(hash_fn(records, n), return_inverse=True)
    class_id = torch.full((P,), -1, dtype=torch.int64, device=records.device)
    pending = rows
    while pending.numel():
        lowest = torch.full((P,), P, dtype=torch.int64, device=records.device).scatter_reduce_(0, bucket[pending], pending, "amin")
        rep = lowest[bucket[pending]]                                 # the lowest unassigned row of each pending row's bucket
        verdict = same_fn(records[pending].contiguous(), n[pending].contiguous(), records, n, rep)[0]
        if bool((verdict > 1).any()):
            raise RuntimeError("graph_classes: a comparison ran out of its search budget (verdict 2); the classes are not known")
        same = verdict == 1
        class_id[pending[same]] = rep[same]
        pending = pending[~same]
    return class_id


# ------------------------------------------------------------------------------------------------------------------ MCES distance

class Mces(NamedTuple):
    """Per-pair device tensors of ``ds_mces_records``."""
    dist: torch.Tensor        # [P] i32: W_A + W_B - 2 best, an upper bound that ``map`` achieves (the distance when exact); -1 for an invalid row
    lower: torch.Tensor       # [P] i32: a lower bound on the distance (= dist when exact)
    status: torch.Tensor      # [P] u8: 0 exact, 2 undecided (budget), 3 invalid row
    nodes: torch.Tensor       # [P] i32 tries used
    map: torch.Tensor         # [P, 29] i32 ground-truth atom of every generated atom in the best map, -1 where unmapped or dropped

    @property
    def exact(self) -> torch.Tensor:
        return self.status == 0

    @property
    def undecided(self) -> torch.Tensor:
        return self.status == 2


def mces_batch(ref, prb, ref_index=None, drop_h: bool = True, max_nodes: int = 1 << 18, engine=None) -> Mces:
    """Exact maximum-common-edge-subgraph distance of every generated molecule from its ground truth (``ds_mces_records``,
    ``csrc/ds_mces.hip``): ``W_A + W_B - 2 max score`` over the type-preserving partial atom maps, bond weight = bond order, formal charges
    not compared, hydrogens left out with ``drop_h`` - the graded number next to ``graph_identity_batch``'s verdict, standing in for the
    reference's "MCES (Average)" (``compute_metrics.py:235-243``).  Two deviations from that number: the records hold Kekule orders 1..3, not
    RDKit's aromatic 1.5, so two Kekule drawings of one substituted ring are a non-zero distance apart (o-xylene: 2); and parity with the
    ``myopic_mces`` package itself is unpinned, because it cannot be run here.  Arguments as ``graph_identity_batch``.  Device tensors, no
    synchronisation."""
    return Mces(*_pair_call("mces_records", engine, ref, prb, ref_index, drop_h, max_nodes))


def topk_mces(dist: torch.Tensor, status: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions of ``mces_batch`` over the K consecutive candidates of every spectrum: ``best [S] i32`` (the smallest distance
    among the valid candidates, -1 when all K are invalid), ``best_index [S] i64`` (the first candidate with it, -1 when all are invalid),
    ``mean_best`` (mean of ``best`` over the spectra that have one, a 0-dim f64 tensor; NaN without any) and ``undecided`` (0-dim i64 count).
    An undecided pair keeps its upper bound ``dist``, so with ``undecided > 0`` ``best`` and ``mean_best`` are upper bounds.  Plain torch
    reductions on the tensors' device."""
    if top_k < 1 or dist.numel() % top_k or status.shape != dist.shape:
        raise ValueError(f"{dist.numel()} pairs (status: {status.numel()}) are not a whole number of top_k = {top_k} groups")
    d, bad = dist.reshape(-1, top_k), (status == 3).reshape(-1, top_k)
    filled = torch.where(bad, torch.full_like(d, torch.iinfo(d.dtype).max), d)
    best = filled.min(dim=1).values
    arg = (filled == best.unsqueeze(1)).to(torch.uint8).argmax(dim=1)             # the first candidate that reaches the minimum
    none = bad.all(dim=1)
    best = torch.where(none, torch.full_like(best, -1), best)
    arg = torch.where(none, torch.full_like(arg, -1), arg)
    mean_best = torch.where(none, torch.zeros_like(best), best).double().sum() / (~none).sum()      # 0 / 0 = NaN without any spectrum
    return dict(best=best, best_index=arg, mean_best=mean_best, undecided=(status == 2).sum())


# ------------------------------------------------------------------------------------------------------------------ Morgan fingerprints

class MorganSimilarity(NamedTuple):
    """Per-pair device tensors of ``ds_morgan_similarity_records``."""
    common: torch.Tensor      # [P] i32: size of the intersection of the two (folded) feature sets; -1 for an invalid row
    n_prb: torch.Tensor       # [P] i32: size of the generated molecule's set; -1 for an invalid row
    n_ref: torch.Tensor       # [P] i32: size of the ground truth's set; -1 for an invalid row
    status: torch.Tensor      # [P] u8: 0 ok, 3 invalid row

    @property
    def valid(self) -> torch.Tensor:
        return self.status == 0

    @property
    def tanimoto(self) -> torch.Tensor:
        """``common / (n_prb + n_ref - common)`` as f64: 1.0 when both sets are empty, NaN for an invalid row."""
        c, union = self.common.double(), (self.n_prb + self.n_ref - self.common).double()
        out = torch.where(union == 0, torch.ones_like(c), c / union)
        return torch.where(self.valid, out, torch.full_like(out, float("nan")))

    @property
    def cosine(self) -> torch.Tensor:
        """``common / sqrt(n_prb * n_ref)`` as f64: 1.0 when both sets are empty, 0.0 when exactly one is, NaN for an invalid row."""
        c, a, b = self.common.double(), self.n_prb.double(), self.n_ref.double()
        none = (self.n_prb == 0) | (self.n_ref == 0)
        out = torch.where(none, ((self.n_prb == 0) & (self.n_ref == 0)).double(), c / torch.sqrt(torch.where(none, torch.ones_like(a), a * b)))
        return torch.where(self.valid, out, torch.full_like(out, float("nan")))


def morgan_similarity_batch(ref, prb, ref_index=None, drop_h: bool = True, radius: int = 2, n_bits: int = 2048, engine=None) -> MorganSimilarity:
    """Tanimoto / cosine similarity of the Morgan fingerprints of every generated molecule and its ground truth
    (``ds_morgan_similarity_records``, ``csrc/ds_morgan.hip``): the set sizes, and ``.tanimoto`` / ``.cosine`` from them - the reference's
    ``GetMorganFingerprintAsBitVect(mol, 2, nBits=2048)`` with ``TanimotoSimilarity`` / ``CosineSimilarity`` (``compute_metrics.py:246-253``).
    Deviations from that number: the records hold Kekule orders 1..3 instead of aromatic bonds (the two Kekule drawings of o-xylene share 5 of
    10 + 10 features at radius 2); RDKit's own invariant hash and fold are not reproduced, so values differ where 2048-bit collisions differ
    (bit-for-bit parity is unpinned, RDKit cannot be run here); ``drop_h`` is the reference's SMILES route (heavy atoms, hydrogen count in the
    invariant).  ``n_bits`` 0 compares the unfolded sets.  Arguments as ``graph_identity_batch``.  Device tensors, no synchronisation."""
    return MorganSimilarity(*_pair_call("morgan_similarity_records", engine, ref, prb, ref_index, drop_h, radius, n_bits))


def morgan_fingerprints(records: torch.Tensor, n_atoms, drop_h: bool = True, radius: int = 2, n_bits: Optional[int] = None, engine=None):
    """The Morgan fingerprint of every record (``ds_morgan_records``; definition in the header).  ``n_bits=None``: ``(ids [P, 116] i64 bit
    patterns in ascending unsigned order, count [P] i32)``.  Otherwise a ``[P, n_bits]`` bool tensor, bit ``f mod n_bits`` set for every
    feature f (``n_bits`` a power of two in [64, 4096], as the pair entry point folds) - what diversity and nearest-neighbour analytics
    take.  Plain torch ops on the records' device, no Python per molecule."""
    from . import engine as E
    if n_bits is not None and (isinstance(n_bits, bool) or not isinstance(n_bits, int)):
        raise TypeError(f"n_bits must be an int or None, got {type(n_bits).__name__}")
    if n_bits is not None and not (64 <= n_bits <= E.MORGAN_MAX_BITS and n_bits & (n_bits - 1) == 0):
        raise ValueError(f"n_bits must be a power of two in [64, {E.MORGAN_MAX_BITS}], got {n_bits}")
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    ids, count = (engine if engine is not None else E).morgan_records(records, n, drop_h, radius)
    if n_bits is None:
        return ids, count
    held = torch.arange(ids.shape[1], device=ids.device).unsqueeze(0) < count.unsqueeze(1)
    bits = torch.zeros(ids.shape[0], n_bits + 1, dtype=torch.bool, device=ids.device)          # column n_bits takes the empty slots
    bits.scatter_(1, torch.where(held, ids & (n_bits - 1), torch.full_like(ids, n_bits)), True)
    return bits[:, :n_bits].contiguous()


def topk_morgan(tanimoto: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions of ``MorganSimilarity.tanimoto`` over the K consecutive candidates of every spectrum, NaN (an invalid pair)
    treated as ``topk_summary`` treats it: ``best [S] f64`` (the largest similarity among the valid candidates, NaN when all K are invalid),
    ``best_index [S] i64`` (the first candidate with it, -1 when all are invalid) and ``mean_best`` (mean of ``best`` over the spectra that
    have one, a 0-dim f64 tensor; NaN without any).  Plain torch reductions on the tensor's device."""
    if top_k < 1 or tanimoto.numel() % top_k:
        raise ValueError(f"{tanimoto.numel()} pairs are not a whole number of top_k = {top_k} groups")
    t = tanimoto.reshape(-1, top_k).to(torch.float64)
    bad = torch.isnan(t)
    filled = torch.where(bad, torch.full_like(t, float("-inf")), t)
    best = filled.max(dim=1).values
    arg = (filled == best.unsqueeze(1)).to(torch.uint8).argmax(dim=1)             # the first candidate that reaches the maximum
    none = bad.all(dim=1)
    mean_best = torch.where(none, torch.zeros_like(best), best).sum() / (~none).sum()             # 0 / 0 = NaN without any spectrum
    best = torch.where(none, torch.full_like(best, float("nan")), best)
    arg = torch.where(none, torch.full_like(arg, -1), arg)
    return dict(best=best, best_index=arg, mean_best=mean_best)


# ------------------------------------------------------------------------------------------------------------------ substructure geometry MMD

class GeometryClasses(NamedTuple):
    """The substructure classes of the geometry metric: per kind (bonds, angles, dihedrals) the reference's symbols and their codes."""
    symbols: tuple            # three tuples of symbols such as 'C1H', 'C1C-C1O', 'H1C-C1C-C1N'
    codes: tuple              # three tuples of ints: the fields (type, order, type, ...) in 4-bit groups, first field lowest (the header's encoding)


class SubGeometry(NamedTuple):
    """What ``sub_geometry`` extracts from a record table."""
    values: Dict[str, torch.Tensor]   # symbol -> device f32 tensor: lengths (units of the positions), angles [0, 180] or dihedrals (-180, 180] in degrees
    skipped: torch.Tensor             # [P] i32: entries of a listed class whose value is undefined (coincident atoms, a collinear dihedral)
    classes: GeometryClasses


_GEOMETRY_KINDS = (("top_bond_sym", "bond_length_mean"), ("top_angle_sym", "bond_angle_mean"), ("top_dihedral_sym", "dihedral_angle_mean"))


def _symbol_fields(symbol: str, parts: int, decoder) -> tuple:
    """'H1C-C1N-N1C' -> (0, 1, 1, 1, 2, 1, 1): element, order, element of every part, adjacent parts chained on the shared atom."""
    import re
    pieces = symbol.split("-")
    if len(pieces) != parts:
        raise ValueError(f"{symbol!r}: {parts} bond(s) expected, {len(pieces)} given")
    fields = []
    for k, piece in enumerate(pieces):
        m = re.fullmatch(r"([A-Z][a-z]?)(\d+)([A-Z][a-z]?)", piece)
        if m is None:
            raise ValueError(f"{symbol!r}: {piece!r} is not <element><bond order><element>")
        left, order, right = m.group(1), int(m.group(2)), m.group(3)
        for el in (left, right):
            if el not in decoder or decoder.index(el) > 15:
                raise ValueError(f"{symbol!r}: element {el!r} is not one of the first 16 of the atom decoder {list(decoder)}")
        if not 1 <= order <= 15:
            raise ValueError(f"{symbol!r}: bond order {order} outside 1..15")
        if k and decoder.index(left) != fields[-1]:
            raise ValueError(f"{symbol!r}: {pieces[k - 1]!r} and {piece!r} do not chain on the same atom")
        fields += ([decoder.index(left)] if not k else []) + [order, decoder.index(right)]
    return tuple(fields)


def geometry_classes(dataset_info: Optional[Dict] = None) -> GeometryClasses:
    """The class tables of ``ds_geometry_*_records`` from the reference's symbol lists: ``dataset_info['top_bond_sym' | 'top_angle_sym' |
    'top_dihedral_sym']`` and ``dataset_info['atom_decoder']`` (``datasets/datasets_config.py:19-35``); ``None``: the QM9 lists of ``config``.
    A symbol is ``<element><order><element>``, chained with '-' on the shared atom ('H1C-C1N-N1C').  ``ValueError`` on an unknown element, on
    parts that do not chain, on a list that names a class twice (a class equals its own reverse) and on more than 32 classes of a kind."""
    from . import config as K
    info = dataset_info or dict(atom_decoder=K.QM9_ATOM_DECODER, top_bond_sym=K.QM9_TOP_BOND_SYM, top_angle_sym=K.QM9_TOP_ANGLE_SYM,
                                top_dihedral_sym=K.QM9_TOP_DIHEDRAL_SYM)
    decoder = list(info["atom_decoder"])
    symbols, codes = [], []
    for parts, (key, _) in enumerate(_GEOMETRY_KINDS, start=1):
        names = tuple(info[key])
        if len(names) > 32:
            raise ValueError(f"{key}: {len(names)} classes, at most 32 fit a table")
        seen, row = {}, []
        for name in names:
            fields = _symbol_fields(name, parts, decoder)
            canon = min(fields, fields[::-1])
            if canon in seen:
                raise ValueError(f"{key}: {name!r} names the class of {seen[canon]!r} again (a class is its symbol read in either direction)")
            seen[canon] = name
            row.append(sum(f << (4 * k) for k, f in enumerate(fields)))
        symbols.append(names)
        codes.append(tuple(row))
    return GeometryClasses(tuple(symbols), tuple(codes))


def sub_geometry(records: torch.Tensor, n_atoms, classes: Optional[GeometryClasses] = None, engine=None) -> SubGeometry:
    """Bond lengths, bond angles and dihedral angles of every record of ``records [P, 1248] u8`` (GPU), by substructure symbol - the sample
    lists of ``cal_bond_distance`` / ``cal_bond_angle`` / ``cal_dihedral_angle`` (``evaluation/cal_geometry.py``) on the unsanitised molecules
    of ``check_2D_stability``: every atom and fragment, bonds of any order > 0, positions as they are.  Two kernels
    (``ds_geometry_count_records``, then ``ds_geometry_fill_records`` at the prefix sum of the counts; the totals cross to the host once, to
    size the outputs), then a stable sort by class.  Two stated deviations from the reference: every angle counts once (the reference counts
    it 0, 1 or 2 times depending on atom numbering and on RDKit's begin / end of a bond), and parity with RDKit's ``GetAngleDeg`` /
    ``GetDihedralDeg`` is unpinned (RDKit cannot be run here; the dihedral's global sign cancels in the MMD)."""
    from . import engine as E
    eng = engine if engine is not None else E
    classes = classes if classes is not None else geometry_classes()
    dev = records.device
    n = torch.as_tensor(n_atoms).to(device=dev, dtype=torch.int32).contiguous()
    tables = [torch.tensor(list(c), dtype=torch.int32, device=dev) for c in classes.codes]
    counts, skipped = eng.geometry_count_records(records, n, *tables)
    ends = counts.to(torch.int64).cumsum(0)
    totals = ends[-1].tolist() if ends.shape[0] else [0, 0, 0]
    filled = eng.geometry_fill_records(records, n, *tables, (ends - counts).contiguous(), totals)
    values = {}
    for names, (value, cls) in zip(classes.symbols, filled):
        by_class = torch.sort(cls, stable=True).indices
        sizes = torch.bincount(cls.to(torch.int64), minlength=len(names))[:len(names)].tolist()
        for name, part in zip(names, torch.split(value[by_class], sizes)):
            values[name] = part
    return SubGeometry(values, skipped, classes)


def mmd_1d(source: torch.Tensor, target: torch.Tensor, kernel_mul: float = 2.0, kernel_num: int = 5, fix_sigma: Optional[float] = None,
           engine=None) -> float:
    """``compute_mmd`` of ``evaluation/mmd.py:6-63`` for two 1-D f32 sample tensors on the GPU (``ds_mmd_1d_segments`` with one class): a
    Python float, NaN when a side is empty or all samples are identical.  At most 2^20 samples per side."""
    from . import engine as E
    eng = engine if engine is not None else E
    for t, name in ((source, "source"), (target, "target")):
        E._want(t, name, torch.float32, (None,))
        if t.shape[0] > E.MMD_MAX_SAMPLES:
            raise ValueError(f"{name} holds {t.shape[0]} samples, at most {E.MMD_MAX_SAMPLES} fit")
    off = lambda t: torch.tensor([0, t.shape[0]], dtype=torch.int64, device=t.device)
    out, _ = eng.mmd_1d_segments(source, off(source), target, off(target), kernel_mul, kernel_num, fix_sigma)
    return float(out[0, 0])


def _capped(t: torch.Tensor, max_samples: Optional[int], gen: torch.Generator) -> torch.Tensor:
    if max_samples is None or t.shape[0] <= max_samples:
        return t
    return t[torch.randperm(t.shape[0], generator=gen)[:max_samples].to(t.device)]


def get_sub_geometry_metric(test, dataset_info: Optional[Dict] = None, max_samples: Optional[int] = 20000, seed: int = 0, engine=None):
    """``get_sub_geometry_metric`` of ``evaluation/cal_geometry.py:287-301`` on record tensors: ``test`` is ``(records [*, 1248] u8 on the
    GPU, n_atoms [*])`` of the test molecules, whose geometry is extracted once, here.  Returns ``fn(generated)``, ``generated`` another such
    pair, which gives the reference's dict: the MMD of every symbol of the three lists (NaN where a side has no sample,
    ``cal_geometry.py:273-275``) and ``bond_length_mean``, ``bond_angle_mean``, ``dihedral_angle_mean``, the NaN-ignoring means of their
    kinds - Python floats, all classes through one ``ds_mmd_1d_segments`` launch sequence.

    Deviations from the reference: its ``random.sample`` cap of 20 000 samples per symbol and side is a seeded ``torch.randperm`` on the host
    here (the target side drawn once with ``seed``, the generated side with ``seed + 1`` on every call, so a call is reproducible;
    ``max_samples=None`` uses every sample, up to 2^20 per symbol and side); its ``target_geometry_stat.pk`` cache is not kept; and the two of
    ``sub_geometry``: every angle counts once, parity with RDKit's angle functions is unpinned."""
    from . import engine as E
    eng = engine if engine is not None else E
    classes = geometry_classes(dataset_info)
    names = [s for kind in classes.symbols for s in kind]
    target = sub_geometry(test[0], test[1], classes, engine).values
    gen = torch.Generator().manual_seed(int(seed))
    dev = test[0].device

    def packed(values, gen):
        parts = [_capped(values[s], max_samples, gen) for s in names]
        sizes = torch.tensor([0] + [p.shape[0] for p in parts], dtype=torch.int64)
        return torch.cat(parts).contiguous(), sizes.cumsum(0).to(dev)
    y, y_off = packed(target, gen)

    def sub_geometry_metric(generated):
        x, x_off = packed(sub_geometry(generated[0], generated[1], classes, engine).values, torch.Generator().manual_seed(int(seed) + 1))
        out, _ = eng.mmd_1d_segments(x, x_off, y, y_off)
        mmd = dict(zip(names, out[:, 0].tolist()))
        result = {}
        for kind, (_, mean_name) in zip(classes.symbols, _GEOMETRY_KINDS):
            seen = [mmd[s] for s in kind if mmd[s] == mmd[s]]
            result.update({s: mmd[s] for s in kind})
            result[mean_name] = sum(seen) / len(seen) if seen else float("nan")
        return result
    return sub_geometry_metric


# ------------------------------------------------------------------------------------------------------------------ set against set

class SetSimilarity(NamedTuple):
    """Per-row device tensors of ``dss_tanimoto_nn``: every row of a set against all rows of another."""
    best_common: torch.Tensor     # [Na] i32: |a & b| of the most similar row b; -1 when no row was compared
    best_union: torch.Tensor      # [Na] i32: |a | b| of that pair (0 with 0 common: two empty rows, similarity 1); -1 when no row was compared
    best_index: torch.Tensor      # [Na] i64: its row, the lowest among equally similar ones; -1 when no row was compared
    sum: torch.Tensor             # [Na] f64: the sum of the Tanimoto similarity over the compared rows
    compared: torch.Tensor        # [Na] i64: how many rows were compared

    @property
    def nearest(self) -> torch.Tensor:
        """Tanimoto similarity to the nearest neighbour as f64: 1.0 for two empty rows, NaN when no row was compared."""
        c, u = self.best_common.double(), self.best_union.double()
        out = torch.where(self.best_union == 0, torch.ones_like(c), c / u)
        return torch.where(self.best_index >= 0, out, torch.full_like(out, float("nan")))

    @property
    def mean(self) -> torch.Tensor:
        """Mean Tanimoto similarity to the compared rows as f64, NaN when no row was compared."""
        return self.sum / self.compared.double()                                   # 0.0 / 0 = NaN


class Novelty(NamedTuple):
    """What ``novelty`` returns."""
    novel: torch.Tensor                   # [P] bool: no known molecule is the same labelled graph
    novel_fraction_of_unique: float       # distinct novel graphs / distinct generated graphs (``rdkit_metric.py:45-52,63-65``); NaN without any
    novel_over_all: float                 # distinct novel graphs / generated rows (``eval_rdmol``, ``rdkit_metric.py:120-122``); NaN without any


def morgan_bit_rows(records: torch.Tensor, n_atoms, drop_h: bool = True, radius: int = 2, n_bits: int = 1024, engine=None):
    """The Morgan fingerprint of every record as a packed bit row: ``(words [P, n_bits / 64] i64 bit patterns, popcount [P] i32)`` on the
    records' device (``ds_morgan_records``, then ``dss_fold_bits``) - the operands of ``nearest_neighbour_similarity``.  Bit ``f mod n_bits`` is
    set for every feature f, as ``morgan_fingerprints(..., n_bits=...)`` sets it; bit b is bit ``b % 64`` of word ``b // 64``.  The default of
    1024 bits is MOSES's Morgan setting (restated from the package as remembered); the per-pair metric keeps the reference's 2048.  The
    fingerprint is not RDKit's bit for bit (``morgan_similarity_batch`` lists the deviations).  No Python per molecule."""
    from . import engine as E
    eng = engine if engine is not None else E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    ids, count = eng.morgan_records(records, n, drop_h, radius)
    return eng.fold_bits(ids, count, n_bits)


def nearest_neighbour_similarity(gen, ref, skip_same_index: bool = False, engine=None) -> SetSimilarity:
    """Every bit row of ``gen`` against every bit row of ``ref`` (both ``(words, popcount)`` of ``morgan_bit_rows``, of one width): the
    nearest neighbour of each generated row and the sum of its Tanimoto similarities (``dss_tanimoto_nn``).  ``skip_same_index`` leaves out row
    i of ``ref`` for row i of ``gen`` (a set against itself without the self-pairs).  Device tensors, no synchronisation."""
    from . import engine as E
    eng = engine if engine is not None else E
    n_bits = 64 * gen[0].shape[-1] if gen[0].dim() == 2 else 0                         # a wrong shape is the binding's to refuse
    return SetSimilarity(*eng.tanimoto_nn(gen[0], gen[1], ref[0], ref[1], n_bits, skip_same_index))


def _host_sum(t: torch.Tensor) -> float:
    """Sum of a vector on the host, in index order (the evaluate driver's rule: one order of summation everywhere)."""
    acc = 0.0
    for v in t.detach().to("cpu", torch.float64).tolist():
        acc += v
    return acc


def snn(gen, ref, skip_same_index: bool = False, engine=None) -> float:
    """MOSES's SNN (``SNNMetric``, restated from the package as remembered; parity unpinned): the mean over the generated rows of the
    Tanimoto similarity to the nearest row of ``ref``, over the rows that have one; NaN without any.  Arguments as
    ``nearest_neighbour_similarity``.  A Python float (synchronises)."""
    near = nearest_neighbour_similarity(gen, ref, skip_same_index, engine).nearest.cpu()
    have = ~torch.isnan(near)
    n = int(have.sum())
    return _host_sum(near[have]) / n if n else float("nan")


def internal_diversity(gen, engine=None) -> float:
    """MOSES's IntDiv (``internal_diversity`` with p = 1, restated from the package as remembered; parity unpinned): one minus the mean
    Tanimoto similarity over all ordered pairs of the set, self-pairs included as MOSES includes them - ``1 - sum_i sum_i / sum_i compared_i``,
    the row sums added on the host in index order.  ``gen``: ``(words, popcount)`` of ``morgan_bit_rows``.  NaN for an empty set.  A Python
    float (synchronises)."""
    out = nearest_neighbour_similarity(gen, gen, False, engine)
    pairs = int(out.compared.sum())
    return 1.0 - _host_sum(out.sum) / pairs if pairs else float("nan")


def novelty(generated, known, engine=None) -> Novelty:
    """Which generated molecules are no known molecule: ``generated`` and ``known`` are ``(records [*, 1248] u8 on the GPU, n_atoms [*])``
    pairs; ``graph_classes`` runs on the concatenation known + generated, and a generated row is novel iff the lowest row of its class lies
    in the generated part.  Returns ``Novelty(novel [P] bool on the device, novel_fraction_of_unique, novel_over_all)``: distinct novel graphs
    over distinct generated graphs (``compute_novelty`` on the unique list, ``evaluation/rdkit_metric.py:45-52,63-65``) and over all generated
    rows (``eval_rdmol``, ``rdkit_metric.py:120-122``); NaN without a generated row.  Identity is constitution-level (atom type, formal charge,
    bond order under a bijection, whole molecules): unlike the reference's canonical SMILES it has no stereo and no tautomer / charge
    normalisation, and the reference's RDKit sanitisation filter is not reproduced."""
    (g_rec, g_n), (k_rec, k_n) = generated, known
    dev = g_rec.device
    i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).reshape(-1)
    K, P = k_rec.shape[0], g_rec.shape[0]
    cls = graph_classes(torch.cat([k_rec.to(dev), g_rec]).contiguous(), torch.cat([i32(k_n), i32(g_n)]), engine)[K:]
    novel = cls >= K
    if P == 0:
        return Novelty(novel, float("nan"), float("nan"))
    n_novel = int(cls[novel].unique().numel())
    return Novelty(novel, n_novel / int(cls.unique().numel()), n_novel / P)


def _class_representatives(records, n, engine):
    """Rows of the lowest member of every ``graph_classes`` class, ascending."""
    cls = graph_classes(records, n, engine)
    return torch.nonzero(cls == torch.arange(cls.shape[0], device=cls.device)).reshape(-1)


def get_set_similarity_metric(test, known=None, n_bits: int = 1024, unique: bool = True, engine=None):
    """The set-level numbers of the reference's "Metric-2D" line that need no RDKit model (``get_moses_metrics``, ``evaluation/mose_metric.py``;
    ``run_lib.py:346-390``) on record tensors: ``test`` is ``(records [*, 1248] u8 on the GPU, n_atoms [*])`` of the test molecules, whose bit
    rows are made once, here; ``known``, optional, is such a pair of the training molecules.  Returns ``fn(generated, keep=None)``,
    ``generated`` another such pair, which gives a dict: ``snn`` and ``int_div`` (Python floats: ``snn`` of the generated against the test
    set, ``internal_diversity`` of the generated set), ``nearest`` (f64 device tensor: every compared generated row's similarity to its
    nearest test molecule) and ``nearest_index`` (i64: that molecule's row in the CALLER's test table), ``n_generated`` / ``n_test`` (rows that
    entered) and, with ``known``, ``novelty`` (the ``Novelty`` of the rows that entered).

    ``unique=True`` keeps one representative - the lowest row - of every ``graph_classes`` class on both sides, where the reference takes
    ``list(set(smiles))``.  ``keep`` is an optional bool mask over the generated rows (the device-side stability mask, say): the reference's own
    filter is RDKit sanitisation, which is not reproduced.  FCD is not computed (Scaf: ``get_scaffold_metric``, Frag: ``get_fragment_metric``).  The MOSES definitions are restated from the
    package as remembered and parity with MOSES is unpinned; identity is constitution-level (``graph_identity_batch``)."""
    from . import engine as E
    dev = test[0].device
    i32 = lambda t, d: torch.as_tensor(t).to(device=d, dtype=torch.int32).reshape(-1).contiguous()
    t_rec, t_n = test[0], i32(test[1], dev)
    t_rows = _class_representatives(t_rec, t_n, engine) if unique else torch.arange(t_rec.shape[0], device=dev)
    ref = morgan_bit_rows(t_rec[t_rows].contiguous(), t_n[t_rows], n_bits=n_bits, engine=engine)

    def set_similarity_metric(generated, keep=None):
        g_rec, g_n = generated[0], i32(generated[1], generated[0].device)
        if keep is not None:
            rows = torch.nonzero(torch.as_tensor(keep).to(g_rec.device).bool().reshape(-1)).reshape(-1)
            g_rec, g_n = g_rec[rows].contiguous(), g_n[rows].contiguous()
        if unique:
            rows = _class_representatives(g_rec, g_n, engine)
            g_rec, g_n = g_rec[rows].contiguous(), g_n[rows].contiguous()
        gen = morgan_bit_rows(g_rec, g_n, n_bits=n_bits, engine=engine)
        near = nearest_neighbour_similarity(gen, ref, engine=engine)
        nearest = near.nearest
        have = near.best_index >= 0
        n_have = int(have.sum())
        out = dict(snn=_host_sum(nearest[have]) / n_have if n_have else float("nan"), int_div=internal_diversity(gen, engine),
                   nearest=nearest, nearest_index=torch.where(have, t_rows[near.best_index.clamp(min=0)], near.best_index) if n_have else near.best_index,
                   n_generated=int(g_rec.shape[0]), n_test=int(t_rows.shape[0]))
        if known is not None:
            out["novelty"] = novelty((g_rec, g_n), known, engine)
        return out
    return set_similarity_metric


# ------------------------------------------------------------------------------------------------------------------ stability, validity, fragments

class Valence(NamedTuple):
    """Per-record device tensors of ``dsv_valence_records``."""
    valence: torch.Tensor         # [P, 29] u8: the valence of every atom < n, 0 elsewhere
    stable_mask: torch.Tensor     # [P] i32: bit i = atom i is stable
    valid_mask: torch.Tensor      # [P] i32: bit i = atom i passes the (restated) RDKit valence check
    summary: torch.Tensor         # [P, 4] i32: n, stable atoms, fragments, atoms of the largest fragment
    largest_mask: torch.Tensor    # [P] i32: bit i = atom i belongs to the largest fragment (ties: the one with the lowest atom)
    status: torch.Tensor          # [P] u8: 0 ok, 3 unusable (n = 0, a type above 4, a bond byte above 3): every other output of the row is 0

    @property
    def usable(self) -> torch.Tensor:
        return self.status == 0

    @property
    def mol_stable(self) -> torch.Tensor:
        """Every atom of the molecule is stable (``stability.py:160``); False for an unusable record."""
        return self.usable & (self.summary[:, 1] == self.summary[:, 0])

    @property
    def valid(self) -> torch.Tensor:
        """Every atom passes the valence check - the ``Chem.SanitizeMol`` of ``mol2smiles``, restated; False for an unusable record."""
        return self.usable & (self.valid_mask == torch.bitwise_left_shift(torch.ones_like(self.valid_mask), self.summary[:, 0]) - 1)

    @property
    def complete(self) -> torch.Tensor:
        """Valid and in one piece (``rdkit_metric.py:99-100``)."""
        return self.valid & (self.summary[:, 2] == 1)


def _bonds_from(bonds: str) -> int:
    from . import engine as E
    if bonds not in ("record", "distance"):
        raise ValueError(f"bonds must be 'record' or 'distance', got {bonds!r}")
    return E.BONDS_RECORD if bonds == "record" else E.BONDS_DISTANCE


def valence_batch(records: torch.Tensor, n_atoms, bonds: str = "record", engine=None) -> Valence:
    """Valences, stability, validity and fragments of every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsv_valence_records``.
    ``bonds="record"``: the predicted bond orders and the raw charge bytes with ``allowed_fc_bonds`` - the reference's ``check_2D_stability``;
    ``bonds="distance"``: orders from the fp32 positions by ``get_bond_order`` with the arithmetic of ``ds_check_stability``, charges 0,
    ``allowed_bonds`` - its ``check_stability``.  The validity restates RDKit's valence check with the charges the reference applies (N+1, N-1,
    C+1, O-1, C-1) and is unpinned against RDKit.  Device tensors, no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return Valence(*(engine if engine is not None else E).valence_records(records, n, _bonds_from(bonds)))


def largest_fragment_records(records: torch.Tensor, n_atoms, bonds: str = "record", engine=None):
    """``(records [P, 1248] u8, n_atoms [P] i32)`` of the largest fragment of every molecule (connected components over all atoms, bonds of
    order > 0; among equally large fragments the one with the lowest atom), atoms in their original order, with the charges the reference
    applies to its RDKit atoms and, for ``bonds="distance"``, the derived bond orders and no charges - the ``largest_mol`` of ``eval_rdmol``.
    An unusable record gives 0 atoms.  Two launches (``dsv_valence_records``, ``dsv_fragment_records``), no synchronisation."""
    from . import engine as E
    eng = engine if engine is not None else E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    mode = _bonds_from(bonds)
    return eng.fragment_records(records, n, eng.valence_records(records, n, mode)[4], mode, True)


def _edm_metric(bonds: str, known, engine):
    def edm_metric(records, n_atoms):
        from . import engine as E
        eng = engine if engine is not None else E
        dev = records.device
        n = torch.as_tensor(n_atoms).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        mode = _bonds_from(bonds)
        v = Valence(*eng.valence_records(records, n, mode))
        frag_rec, frag_n = eng.fragment_records(records, n, v.largest_mask, mode, True)
        valid = v.valid
        P, atoms = int(n.shape[0]), int(n.clamp(0, shard.RECORD_ATOMS).sum())
        rows = torch.nonzero(valid).reshape(-1)
        g_rec, g_n = frag_rec[rows].contiguous(), frag_n[rows].contiguous()
        K = 0
        if known is not None:
            K = known[0].shape[0]
            k_n = torch.as_tensor(known[1]).to(device=dev, dtype=torch.int32).reshape(-1)
            g_rec, g_n = torch.cat([known[0].to(dev), g_rec]).contiguous(), torch.cat([k_n, g_n]).contiguous()
        cls = graph_classes(g_rec, g_n, engine)[K:]
        over = lambda count, total: count / total if total else float("nan")
        return dict(mol_stable=over(int(v.mol_stable.sum()), P), atom_stable=over(int(v.summary[:, 1].sum()), atoms),
                    Validity=over(int(valid.sum()), P), Complete=over(int(v.complete.sum()), P), Unique=over(int(cls.unique().numel()), P),
                    Novelty=-1 if known is None else over(int(cls[cls >= K].unique().numel()), P),
                    valence=v, valid=valid, largest=(frag_rec, frag_n))
    return edm_metric


def get_edm_metric_2d(known=None, engine=None):
    """``get_2D_edm_metric`` of ``evaluation/stability.py:199-230`` with ``eval_rdmol`` (``rdkit_metric.py:86-129``) on record tensors - the
    reference's "Metric-2D" line.  ``known``, optional, is ``(records [*, 1248] u8, n_atoms [*])`` of the training molecules.  Returns
    ``fn(records, n_atoms)`` (records on the GPU), which gives the reference's two dicts merged, as Python numbers: ``mol_stable`` (stable
    molecules / P), ``atom_stable`` (stable atoms / all atoms), ``Validity`` (valid / P), ``Complete`` (valid and one fragment / P), ``Unique``
    (distinct ``graph_classes`` classes of the largest fragments of the VALID molecules / P - over all generated molecules, as the reference
    divides), ``Novelty`` (those classes that are no known molecule / P; -1 without ``known``); NaN where a denominator is 0.  Next to them the
    device tensors: ``valence`` (the ``Valence`` of ``valence_batch``), ``valid`` (``[P] bool``, the mask that ``get_set_similarity_metric``'s
    ``keep=`` takes) and ``largest`` (``(records, n_atoms)`` of every molecule's largest fragment).

    Deviations from the reference: the validity restates RDKit's valence check and is unpinned against RDKit; identity is constitution-level
    on the explicit graph (what a SMILES of an all-explicit, stereo-free RDKit molecule distinguishes), with Kekule orders only; an unusable
    record (``n = 0``, a byte outside the alphabet) counts in every denominator and in no numerator."""
    return _edm_metric("record", known, engine)


def get_edm_metric_3d(known=None, engine=None):
    """``get_edm_metric`` of ``evaluation/stability.py:164-196`` on record tensors - the reference's "Metric-3D" line: as
    ``get_edm_metric_2d``, with the bond orders derived from the distances (``get_bond_order``, the arithmetic of ``ds_check_stability``),
    no charges and ``allowed_bonds``; the largest fragments carry the derived orders.  The same deviations apply."""
    return _edm_metric("distance", known, engine)


# ------------------------------------------------------------------------------------------------------------------ functional groups

FUNCTIONAL_GROUP_NAMES = ("alkane", "alkene", "alkyne", "arene", "alcohol", "ether", "aldehyde", "ketone", "carboxylic acid", "ester", "haloalkane",
                          "acyl halide", "amine", "amide", "nitrile", "sulfide", "thiol")         # bit order of include/diffspectra_groups.h


class FunctionalGroups(NamedTuple):
    """Per-record device tensors of ``dsg_group_records``."""
    groups: torch.Tensor          # [P] i32: bit g = group ``FUNCTIONAL_GROUP_NAMES[g]`` is present
    aromatic_mask: torch.Tensor   # [P] i32: bit i = atom i is aromatic (the project's rule; unpinned against RDKit)
    status: torch.Tensor          # [P] u8: 0 ok, 2 unusable (n = 0, a type above 4, a bond byte above 3): the row is 0

    @property
    def usable(self) -> torch.Tensor:
        return self.status == 0

    def present(self, name: str) -> torch.Tensor:
        """``[P] bool``: the molecule has the group ``name`` (False for an unusable record)."""
        if name not in FUNCTIONAL_GROUP_NAMES:
            raise ValueError(f"{name!r} is none of {list(FUNCTIONAL_GROUP_NAMES)}")
        return torch.bitwise_and(self.groups, 1 << FUNCTIONAL_GROUP_NAMES.index(name)) != 0

    def names(self, p: int) -> tuple:
        """The names of the groups of row ``p``, in bit order (a host helper: synchronises)."""
        word = int(self.groups[p])
        return tuple(name for g, name in enumerate(FUNCTIONAL_GROUP_NAMES) if (word >> g) & 1)


class GroupSimilarity(NamedTuple):
    """Per-pair tensors of ``functional_group_similarity_batch``."""
    similarity: torch.Tensor      # [P] f64: common / either, 1.0 when neither molecule has a group, NaN for a pair that is not ok
    common: torch.Tensor          # [P] i32: groups both molecules have; -1 for a pair that is not ok
    either: torch.Tensor          # [P] i32: groups at least one of them has; -1 for a pair that is not ok
    groups: torch.Tensor          # [P, 2] i32: the group words of the generated molecule and of its ground truth; 0 for a pair that is not ok
    status: torch.Tensor          # [P] u8: 0 ok, 2 a record of the pair is unusable, 3 invalid row

    @property
    def valid(self) -> torch.Tensor:
        return self.status == 0


def functional_groups(records: torch.Tensor, n_atoms, engine=None) -> FunctionalGroups:
    """The functional groups and the aromatic atoms of every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsg_group_records``:
    the 17 groups of the reference's ``compute_metrics.py:38-56`` as predicates on the record graph (``include/diffspectra_groups.h`` states
    them), with aromaticity perceived by the project's own order-free rule - unpinned against RDKit, which cannot be run here.  Device tensors,
    no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return FunctionalGroups(*(engine if engine is not None else E).group_records(records, n))


def functional_group_similarity_batch(ref, prb, ref_index=None, engine=None) -> GroupSimilarity:
    """The reference's "Functional Group Similarity" (``compute_metrics.py:117-144``) of every generated molecule and its ground truth
    (``dsg_group_similarity_records``, ``csrc/ds_groups.hip``): the Jaccard index of the two sets of groups present, 1.0 when both are empty.
    Every usable pair is scored; the reference scores only molecules that survived RDKit, and ``valence_batch(...).valid`` is the filter for
    that.  Deviations are those of ``functional_groups``.  Arguments as ``graph_identity_batch``.  Device tensors, no synchronisation."""
    common, either, groups, status = _pair_call("group_similarity_records", engine, ref, prb, ref_index)
    c, u = common.double(), either.double()
    sim = torch.where(either == 0, torch.ones_like(c), c / torch.where(either == 0, torch.ones_like(u), u))
    sim = torch.where(status == 0, sim, torch.full_like(sim, float("nan")))
    return GroupSimilarity(sim, common, either, groups, status)


def topk_groups(similarity: torch.Tensor, status: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions of ``functional_group_similarity_batch`` over the K consecutive candidates of every spectrum, shaped like
    ``topk_morgan``: ``best [S] f64`` (the largest similarity among the ok candidates, NaN when none of the K is ok), ``best_index [S] i64`` (the
    first candidate with it, -1 when none is ok) and ``mean_best`` (mean of ``best`` over the spectra that have one, a 0-dim f64 tensor; NaN
    without any).  Plain torch reductions on the tensors' device."""
    if top_k < 1 or similarity.numel() % top_k or status.shape != similarity.shape:
        raise ValueError(f"{similarity.numel()} pairs (status: {status.numel()}) are not a whole number of top_k = {top_k} groups")
    return topk_morgan(torch.where(status == 0, similarity.to(torch.float64), torch.full_like(similarity, float("nan"), dtype=torch.float64)), top_k)


# ------------------------------------------------------------------------------------------------------------------ scaffolds

class Scaffolds(NamedTuple):
    """Per-record device tensors of ``dsk_scaffold_masks``.  There is no ``core_mask``: the core is the scaffold without its exocyclic atoms,
    and which scaffold atoms are exocyclic (outside the core) cannot be told from these four outputs without reading the record again; the
    ring atoms are the part of the core that the outputs do name."""
    scaffold_mask: torch.Tensor   # [P] i32: bit i = atom i belongs to the scaffold (the 2-core of the heavy graph plus its exocyclic atoms)
    ring_mask: torch.Tensor       # [P] i32: bit i = atom i is a ring atom
    summary: torch.Tensor         # [P, 4] i32: heavy atoms, scaffold atoms, rings, ring atoms
    status: torch.Tensor          # [P] u8: 0 ok, 3 unusable (n = 0, a type above 4, a bond byte above 3): every other output of the row is 0

    @property
    def usable(self) -> torch.Tensor:
        return self.status == 0

    @property
    def rings(self) -> torch.Tensor:
        """``[P] i32``: the cyclomatic number of the core - RDKit's ``RingInfo.NumRings()`` of a molecule."""
        return self.summary[:, 2]

    def has_scaffold(self, min_rings: int = 2) -> torch.Tensor:
        """``[P] bool``: the scaffold is non-empty and has at least ``min_rings`` rings (MOSES's ``compute_scaffold``; its default is 2)."""
        return self.usable & (self.scaffold_mask != 0) & (self.rings >= min_rings)


class ScaffoldIdentity(NamedTuple):
    """What ``scaffold_identity_batch`` returns."""
    same: torch.Tensor            # [P] bool: both molecules have no scaffold, or both have one and they are the same labelled graph
    status: torch.Tensor          # [P] u8: 0 ok, 3 a record of the pair is unusable (``DSK_UNUSABLE``) or the row is invalid (``ref_index`` outside)
    undecided: torch.Tensor       # 0-dim i64: the pairs whose scaffold comparison ran out of its budget; they count as different


def scaffolds(records: torch.Tensor, n_atoms, engine=None) -> Scaffolds:
    """The Bemis-Murcko scaffold atoms, the ring atoms and the ring count of every record of ``records [P, 1248] u8`` (GPU) in one launch of
    ``dsk_scaffold_masks`` (``csrc/ds_scaffold.hip``; every definition in ``include/diffspectra_scaffold.h``): the scaffold is the 2-core of the
    heavy graph plus the atoms multiply bonded to it - RDKit's ``GetScaffoldForMol`` restated, unpinned against RDKit, which cannot be run
    here.  Device tensors, no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return Scaffolds(*(engine if engine is not None else E).scaffold_masks(records, n))


def _scaffold_side(records, n, bond_orders, engine):
    """``(Scaffolds, scaffold records, their atom counts)`` of a record table with ``n`` already ``[P] i32`` on the device: two launches."""
    from . import engine as E
    eng = engine if engine is not None else E
    found = Scaffolds(*eng.scaffold_masks(records, n))
    rec, count = eng.fragment_records(records, n, found.scaffold_mask, E.BONDS_RECORD, True)
    if not bond_orders:
        rec[:, shard._BOND].clamp_(max=1)
    return found, rec, count


def scaffold_records(records: torch.Tensor, n_atoms, bond_orders: bool = True, engine=None):
    """``(records [P, 1248] u8, n_atoms [P] i32)`` of the scaffold of every molecule: its scaffold atoms (``scaffolds``) as a record of their own
    (``dsv_fragment_records``) - heavy atoms only, in their original order, with the charges the reference applies to its RDKit atoms.
    ``bond_orders=False`` sets every non-zero bond byte of the result to 1: the order-free framework, under which all Kekule drawings of a
    ring system are one scaffold and an exocyclic ``=O`` becomes ``-O``.  An unusable or acyclic record gives 0 atoms.  No synchronisation."""
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return _scaffold_side(records, n, bond_orders, engine)[1:]


def scaffold_identity_batch(ref, prb, ref_index=None, min_rings: int = 1, bond_orders: bool = True, engine=None) -> ScaffoldIdentity:
    """Does every generated molecule share the scaffold of its ground truth?  Arguments as ``graph_identity_batch``.  A molecule has a scaffold
    iff ``Scaffolds.has_scaffold(min_rings)``.  Both molecules without one: same; exactly one without: different; otherwise the verdict of
    ``graph_identity_batch`` on the two scaffold records (``scaffold_records(..., bond_orders)``), where an undecided verdict counts as
    different and is counted in ``undecided``.  ``status`` is 0 for an ok pair and 3 for a pair with an unusable record (``DSK_UNUSABLE``) or
    with ``ref_index`` outside the table (invalid); ``same`` is False there.  Device tensors, no synchronisation."""
    (ref_rec, ref_n), (prb_rec, prb_n) = ref, prb
    dev = prb_rec.device
    i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    P, M = prb_rec.shape[0], ref_rec.shape[0]
    idx = torch.arange(P, device=dev) if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    r_found, r_rec, r_count = _scaffold_side(ref_rec, i32(ref_n), bond_orders, engine)
    p_found, p_rec, p_count = _scaffold_side(prb_rec, i32(prb_n), bond_orders, engine)
    inside = (idx >= 0) & (idx < M)
    row = torch.where(inside, idx, torch.zeros_like(idx))
    at = lambda t: t[row] if M else torch.zeros(P, dtype=t.dtype, device=dev)
    ok = inside & at(r_found.usable) & p_found.usable
    r_has, p_has = at(r_found.has_scaffold(min_rings)) & ok, p_found.has_scaffold(min_rings) & ok
    verdict = graph_identity_batch((r_rec, r_count), (p_rec, p_count), ref_index=idx, engine=engine).verdict
    both = r_has & p_has
    same = ok & ((~r_has & ~p_has) | (both & (verdict == 1)))
    from . import engine as E
    status = torch.where(ok, torch.zeros_like(p_found.status), torch.full_like(p_found.status, E.SCAFFOLD_UNUSABLE))
    return ScaffoldIdentity(same, status, (both & (verdict == 2)).sum())


def get_scaffold_metric(test, min_rings: int = 2, unique: bool = True, bond_orders: bool = True, engine=None):
    """The "Scaf" number of the reference's set metrics (``evaluation/mose_metric.py:111-113``; MOSES's ``compute_scaffolds``, ``ScafMetric`` and
    ``cos_similarity``, restated from the package as remembered - parity with MOSES is unpinned) on record tensors: the cosine similarity of
    the Bemis-Murcko scaffold counts of the generated and of the test molecules.  ``test`` is ``(records [*, 1248] u8 on the GPU, n_atoms [*])``
    of the test molecules, analysed once, here.  Returns ``fn(generated, keep=None)``, ``generated`` another such pair; ``keep`` and ``unique``
    mean what they mean in ``get_set_similarity_metric`` (one representative per ``graph_classes`` class of the MOLECULES).  ``fn`` gives a
    dict: ``scaf`` (a Python float: with g_k and t_k the numbers of generated and of test molecules with scaffold k, ``sum g_k t_k /
    sqrt(sum g_k^2 * sum t_k^2)`` from exact integers; NaN when either side has no scaffold), ``n_generated`` / ``n_test`` (molecules that
    entered), ``with_scaffold_generated`` / ``with_scaffold_test`` (those that have a scaffold: non-empty, ``rings >= min_rings``),
    ``distinct_generated`` / ``distinct_test`` / ``shared`` (numbers of scaffold classes), ``scaffold_class`` (i64 device tensor over the generated
    rows that entered: the row of the class's lowest member in the table "test scaffolds, then generated scaffolds", -1 without a scaffold)
    and ``mean_rings`` (a Python float over the usable generated rows that entered; NaN without any).

    Deviations: two scaffolds are the same when ``graph_classes`` says so (atom type, applied charge, bond order), so two Kekule drawings of
    a scaffold that no symmetry maps onto each other (2-cyclopropylpyridine) are two scaffolds - ``bond_orders=False`` compares order-free
    frameworks instead, under which an exocyclic ``=O`` also equals ``-O``; there is no RDKit sanitisation
    filter (``keep=`` takes the caller's mask); a record with several fragments contributes the scaffold of all of them together."""
    import math
    dev = test[0].device
    i32 = lambda t, d: torch.as_tensor(t).to(device=d, dtype=torch.int32).reshape(-1).contiguous()

    def side(rec, n):
        """The rows that enter, what was found in them, and the scaffold records of those that have a scaffold."""
        if unique:
            rows = _class_representatives(rec, n, engine)
            rec, n = rec[rows].contiguous(), n[rows].contiguous()
        found, s_rec, s_n = _scaffold_side(rec, n, bond_orders, engine)
        has = found.has_scaffold(min_rings)
        rows = torch.nonzero(has).reshape(-1)
        return found, has, s_rec[rows].contiguous(), s_n[rows].contiguous()

    t_found, t_has, t_rec, t_n = side(test[0], i32(test[1], dev))
    T = int(t_rec.shape[0])

    def scaffold_metric(generated, keep=None):
        g_rec, g_n = generated[0], i32(generated[1], generated[0].device)
        if keep is not None:
            rows = torch.nonzero(torch.as_tensor(keep).to(g_rec.device).bool().reshape(-1)).reshape(-1)
            g_rec, g_n = g_rec[rows].contiguous(), g_n[rows].contiguous()
        g_found, g_has, s_rec, s_n = side(g_rec, g_n)
        G = int(s_rec.shape[0])
        cls = graph_classes(torch.cat([t_rec.to(s_rec.device), s_rec]).contiguous(), torch.cat([t_n.to(s_n.device), s_n]).contiguous(), engine)

        def count(ids):                                                          # molecules per scaffold class, at the class's own row
            classes, members = torch.unique(ids, return_counts=True)
            return torch.zeros(T + G, dtype=torch.int64, device=cls.device).index_put_((classes,), members)
        t_count, g_count = count(cls[:T]), count(cls[T:])
        dot, gg, tt = int((g_count * t_count).sum()), int((g_count * g_count).sum()), int((t_count * t_count).sum())
        scaffold_class = torch.full((g_has.shape[0],), -1, dtype=torch.int64, device=cls.device)
        scaffold_class[g_has] = cls[T:]
        usable = g_found.usable
        n_usable = int(usable.sum())
        return dict(scaf=dot / math.sqrt(gg * tt) if gg and tt else float("nan"), n_generated=int(g_has.shape[0]), n_test=int(t_has.shape[0]),
                    with_scaffold_generated=G, with_scaffold_test=T, distinct_generated=int((g_count > 0).sum()), distinct_test=int((t_count > 0).sum()),
                    shared=int(((g_count > 0) & (t_count > 0)).sum()), scaffold_class=scaffold_class,
                    mean_rings=int(g_found.rings[usable].to(torch.int64).sum()) / n_usable if n_usable else float("nan"))
    return scaffold_metric


# ------------------------------------------------------------------------------------------------------------------ BRICS fragments

# The labels and the rules of include/diffspectra_brics.h: (x, y, bond order), in the order in which a bond takes its labels.  The sulfur
# environments L11 and L12 and their six rules are left out: a record holds no sulfur.
BRICS_LABELS = (1, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16)
BRICS_RULES = ((1, 3, 1), (1, 5, 1), (1, 10, 1),
               (3, 4, 1), (3, 13, 1), (3, 14, 1), (3, 15, 1), (3, 16, 1),
               (4, 5, 1),
               (5, 14, 1), (5, 16, 1), (5, 13, 1), (5, 15, 1),
               (6, 13, 1), (6, 14, 1), (6, 15, 1), (6, 16, 1),
               (7, 7, 2),
               (8, 9, 1), (8, 10, 1), (8, 13, 1), (8, 14, 1), (8, 15, 1), (8, 16, 1),
               (9, 13, 1), (9, 14, 1), (9, 15, 1), (9, 16, 1),
               (10, 13, 1), (10, 14, 1), (10, 15, 1), (10, 16, 1),
               (13, 14, 1), (13, 15, 1), (13, 16, 1),
               (14, 14, 1), (14, 15, 1), (14, 16, 1),
               (15, 16, 1),
               (16, 16, 1))


class Brics(NamedTuple):
    """Per-record device tensors of ``dsb_brics_records``."""
    env: torch.Tensor             # [P, 29] i32: bit e = the atom is in BRICS environment L_e; 0 for a folded hydrogen and for atoms >= n
    cuts: torch.Tensor            # [P, 28, 4] u8: (a, b, label of a, label of b) with a < b, ascending; unused rows 0xff
    fragment_of: torch.Tensor     # [P, 29] u8: the fragment of every atom, 0xff for atoms >= n
    summary: torch.Tensor         # [P, 4] i32: matchable atoms, cuts, fragments, atoms of the largest fragment with its hydrogens
    status: torch.Tensor          # [P] u8: 0 ok, 3 unusable (n = 0, a type above 4, a bond byte above 3): cuts and fragment_of 0xff, the rest 0

    @property
    def usable(self) -> torch.Tensor:
        return self.status == 0

    @property
    def n_cuts(self) -> torch.Tensor:
        return self.summary[:, 1]

    @property
    def n_fragments(self) -> torch.Tensor:
        return self.summary[:, 2]


def brics(records: torch.Tensor, n_atoms, engine=None) -> Brics:
    """The BRICS environments, cut bonds with their labels and fragments of every record of ``records [P, 1248] u8`` (GPU) in one launch of
    ``dsb_brics_records`` (``csrc/ds_brics.hip``; every definition in ``include/diffspectra_brics.h``).  The environments and the rules restate
    RDKit's ``BRICS.py`` as remembered and are unpinned against RDKit, which cannot be run here; they run on the hydrogen-folded graph of
    ``substructure_search`` with the project's aromaticity; sulfur never occurs; a bond that fits a rule in both orientations gives both ends
    the rule's first label.  Device tensors, no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return Brics(*(engine if engine is not None else E).brics_records(records, n))


def _brics_side(records, n, aromatic, engine):
    """``(Brics, fragment records, their atom counts, owner, source)`` of a record table with ``n`` already ``[P] i32`` on the device: two
    launches, a ``torch.cumsum`` on the device and one read of the total between them."""
    from . import engine as E
    eng = engine if engine is not None else E
    found = Brics(*eng.brics_records(records, n))
    counts = found.n_fragments.to(torch.int64)
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1]) if counts.numel() else 0
    return (found, *eng.brics_fragment_records(records, n, (ends - counts).contiguous(), total, aromatic))


def brics_fragment_records(records: torch.Tensor, n_atoms, aromatic: bool = True, engine=None):
    """``(frag_rec [F, 1248] u8, frag_n [F] i32, owner [F] i64, source [F, 29] u8)``: every BRICS fragment of every record as a record of its
    own (``dsb_brics_fragment_records``), the fragments of record 0 first.  A fragment record holds the fragment's atoms in their original
    order, hydrogens included, with applied charges, and then one attachment point per cut end: type byte 5, the BRICS label of the atom it
    is attached to in the charge byte, the position of the atom across the cut.  ``aromatic=True`` writes aromatic bonds as order 4, so both
    Kekule drawings of a ring give one fragment; ``False`` keeps the Kekule orders.  ``owner`` is the record a fragment comes from, ``source``
    the original atom of every atom of the row (0xff beyond ``frag_n``).  Such records are outside the alphabet of the other analytics, which
    call them unusable; ``graph_classes`` compares raw bytes and decides their identity.  One read of the fragment total sizes the output."""
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return _brics_side(records, n, aromatic, engine)[1:]


def get_fragment_metric(test, unique: bool = True, aromatic: bool = True, engine=None):
    """The "Frag" number of the reference's set metrics (``evaluation/mose_metric.py:88-128``; MOSES's ``compute_fragments``, ``FragMetric`` and
    ``cos_similarity``, restated from the package as remembered - parity with MOSES is unpinned) on record tensors: the cosine similarity of
    the BRICS fragment counts of the generated and of the test molecules.  ``test`` is ``(records [*, 1248] u8 on the GPU, n_atoms [*])`` of the
    test molecules, analysed once, here.  Returns ``fn(generated, keep=None)``, ``generated`` another such pair; ``keep`` and ``unique`` mean what
    they mean in ``get_set_similarity_metric`` (one representative per ``graph_classes`` class of the MOLECULES).  ``fn`` gives a dict: ``frag`` (a
    Python float: with g_k and t_k the numbers of FRAGMENTS of class k on each side - every occurrence counts, a molecule without a cut
    contributes itself - ``sum g_k t_k / sqrt(sum g_k^2 * sum t_k^2)`` from exact integers; NaN when a side has no fragment), ``n_generated`` /
    ``n_test`` (molecules that entered), ``fragments_generated`` / ``fragments_test``, ``distinct_generated`` / ``distinct_test`` / ``shared`` (numbers
    of fragment classes), ``mean_cuts`` (a Python float over the usable generated rows that entered; NaN without any), ``fragment_class`` (i64
    device tensor over the generated fragments: the row of the class's lowest member in the table "test fragments, then generated fragments")
    and ``owner`` (i64: the generated row, among those that entered, that each of these fragments comes from).

    Deviations: the BRICS rules are as remembered and unpinned against RDKit and MOSES; aromaticity is the project's rule; two fragments are the
    same when ``graph_classes`` says so (the labelled graph with its attachment labels, not the SMILES) - with ``aromatic=False`` on Kekule
    orders, so that two drawings of a ring are two fragments; there is no RDKit sanitisation filter (``keep=`` takes the caller's mask);
    sulfur never occurs; a bond that fits a rule in both orientations gives both ends the rule's first label."""
    import math
    dev = test[0].device
    i32 = lambda t, d: torch.as_tensor(t).to(device=d, dtype=torch.int32).reshape(-1).contiguous()

    def side(rec, n):
        """What was found in the rows that enter, and their fragment records."""
        if unique:
            rows = _class_representatives(rec, n, engine)
            rec, n = rec[rows].contiguous(), n[rows].contiguous()
        return _brics_side(rec, n, aromatic, engine)[:4]

    t_found, t_rec, t_n, _ = side(test[0], i32(test[1], dev))
    T = int(t_rec.shape[0])

    def fragment_metric(generated, keep=None):
        g_rec, g_n = generated[0], i32(generated[1], generated[0].device)
        if keep is not None:
            rows = torch.nonzero(torch.as_tensor(keep).to(g_rec.device).bool().reshape(-1)).reshape(-1)
            g_rec, g_n = g_rec[rows].contiguous(), g_n[rows].contiguous()
        g_found, f_rec, f_n, owner = side(g_rec, g_n)
        G = int(f_rec.shape[0])
        cls = graph_classes(torch.cat([t_rec.to(f_rec.device), f_rec]).contiguous(), torch.cat([t_n.to(f_n.device), f_n]).contiguous(), engine)

        def count(ids):                                                          # fragments per class, at the class's own row
            classes, members = torch.unique(ids, return_counts=True)
            return torch.zeros(T + G, dtype=torch.int64, device=cls.device).index_put_((classes,), members)
        t_count, g_count = count(cls[:T]), count(cls[T:])
        dot, gg, tt = int((g_count * t_count).sum()), int((g_count * g_count).sum()), int((t_count * t_count).sum())
        usable = g_found.usable
        n_usable = int(usable.sum())
        return dict(frag=dot / math.sqrt(gg * tt) if gg and tt else float("nan"), n_generated=int(g_found.status.shape[0]),
                    n_test=int(t_found.status.shape[0]), fragments_generated=G, fragments_test=T, distinct_generated=int((g_count > 0).sum()),
                    distinct_test=int((t_count > 0).sum()), shared=int(((g_count > 0) & (t_count > 0)).sum()),
                    mean_cuts=int(g_found.n_cuts[usable].to(torch.int64).sum()) / n_usable if n_usable else float("nan"),
                    fragment_class=cls[T:], owner=owner)
    return fragment_metric


# ------------------------------------------------------------------------------------------------------------------ canonical SMILES

class Smiles(NamedTuple):
    """Per-record device tensors of ``dsl_smiles_records``."""
    text: torch.Tensor            # [P, 384] u8: ASCII, zero after ``length``
    length: torch.Tensor          # [P] i32
    status: torch.Tensor          # [P] u8: 0 ok, 1 uncertified (valid string, not canonical: the search hit ``max_nodes``), 2 overflow, 3 unusable
    nodes: torch.Tensor           # [P] i32 individualisations of the search (0: colour refinement alone ordered the atoms)
    atom_order: torch.Tensor      # [P, 29] i32: position of every record atom among the atoms of the string, -1 for folded hydrogens and atoms >= n

    @property
    def certified(self) -> torch.Tensor:
        return self.status == 0

    @property
    def has_text(self) -> torch.Tensor:
        return self.status <= 1


class SmilesMatch(NamedTuple):
    """What ``smiles_exact_match`` returns."""
    same: torch.Tensor            # [P] bool: both strings certified and equal byte for byte
    status: torch.Tensor          # [P] u8: 0 both sides certified, else the larger of the two sides' statuses; 3 also for ``ref_index`` outside


def smiles(records: torch.Tensor, n_atoms, max_nodes: int = 4096, engine=None) -> Smiles:
    """The canonical SMILES string of every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsl_smiles_records``
    (``csrc/ds_smiles.hip``; every definition in ``include/diffspectra_smiles.h``): plain hydrogens folded into their neighbours, the atoms ordered
    by colour refinement with individualisation (at most ``max_nodes`` individualisations after the first leaf), a Kekule OpenSMILES subset
    that any SMILES reader reads.  Canonical for this project - two usable records get the same certified string iff ``graph_identity_batch``
    calls them identical - and NOT RDKit's canonical form.  Device tensors, no synchronisation; ``smiles_strings`` makes Python strings."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    return Smiles(*(engine if engine is not None else E).smiles_records(records, n, max_nodes))


def smiles_strings(result: Smiles) -> list:
    """One ``str`` per row of a ``Smiles``, ``None`` for an overflow or unusable row: the one device-to-host copy of the text."""
    text, length, status = result.text.cpu().numpy(), result.length.cpu().tolist(), result.status.cpu().tolist()
    return [text[p, :length[p]].tobytes().decode("ascii") if status[p] <= 1 else None for p in range(len(status))]


def smiles_exact_match(ref, prb, ref_index=None, max_nodes: int = 4096, engine=None) -> SmilesMatch:
    """The reference's "Exact Match (SMILES)" (``true_smi == pred_smi``, ``compute_metrics.py:209-220``) per pair: ``ref`` and ``prb`` are ``(records
    [*, 1248] u8, n_atoms [*])`` pairs on the GPU or ``Smiles`` results, ground truth first; ``ref_index [P]`` names the ground-truth row of every
    generated molecule (``None``: row p).  ``same`` holds where both strings are certified (status 0) and equal byte for byte - for such pairs it
    is the verdict of ``graph_identity_batch``; ``status`` is 0 there, else the larger status of the two sides, and 3 for a row outside the
    table.  Device tensors, no synchronisation."""
    side = lambda x: x if isinstance(x, Smiles) else smiles(x[0], x[1], max_nodes=max_nodes, engine=engine)
    r, g = side(ref), side(prb)
    dev = g.text.device
    P, M = g.text.shape[0], r.text.shape[0]
    if ref_index is None and M < P:
        raise ValueError(f"without ref_index pair p reads ground-truth row p: {M} rows for {P} pairs")
    idx = torch.arange(P, device=dev) if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).reshape(-1)
    if idx.numel() != P:
        raise ValueError(f"ref_index must name one ground-truth row per pair: {idx.numel()} for {P}")
    inside = (idx >= 0) & (idx < M)
    row = torch.where(inside, idx, torch.zeros_like(idx))
    if M:
        r_text, r_status = r.text.to(dev)[row], r.status.to(dev)[row]
    else:
        r_text, r_status = torch.zeros_like(g.text), torch.full_like(g.status, 3)
    status = torch.where(inside, torch.maximum(r_status, g.status), torch.full_like(g.status, 3))
    same = (status == 0) & (r_text == g.text).all(dim=1)
    return SmilesMatch(same, status)


# ------------------------------------------------------------------------------------------------------------------ SMILES reader

READER_STATUS_NAMES = ("ok", "empty", "syntax", "element", "kekule", "too large", "undecided", "too long")      # by DSP_* status


class SmilesRecords(NamedTuple):
    """Per-string device tensors of ``dsp_read_smiles``."""
    records: torch.Tensor         # [P, 1248] u8: the record; zero unless status 0
    n_atoms: torch.Tensor         # [P] i32: atoms of the record; 0 unless status 0
    status: torch.Tensor          # [P] u8: index into ``READER_STATUS_NAMES``
    where: torch.Tensor           # [P] i32: offset of the first offending byte (syntax, element, kekule), else -1
    string_atoms: torch.Tensor    # [P] i32: atoms written in the string (ok, too large, kekule, undecided; else 0)
    flags: torch.Tensor           # [P] i32: bit 0 isotope, 1 '@', 2 '/' '\', 3 atom class (read and ignored), 4 lower-case atoms
    aromatic: torch.Tensor        # [P] i32: bit i = record atom i was written in lower case
    atom_pos: torch.Tensor        # [P, 29] i32: offset of record atom i's symbol; -1 for appended hydrogens and atoms >= n
    nodes: torch.Tensor           # [P] i32: tries of the Kekule search

    @property
    def ok(self) -> torch.Tensor:
        return self.status == 0


def pack_smiles(strings: Sequence[str], device=None):
    """``(text [P, 384] u8, length [P] i32)`` of Python strings, packed on the host in one numpy pass: surrounding whitespace is stripped, a
    string longer than 384 bytes keeps its true length (the kernel reports it as too long) and a non-ASCII character becomes byte 0xFF
    (which the kernel reports as a syntax error)."""
    import numpy as np
    from . import engine as E
    width = E.READER_TEXT_BYTES
    rows = [(t if t.isascii() else "".join(c if c.isascii() else "\xff" for c in t)).encode("latin-1") for t in (s.strip() for s in strings)]
    length = np.fromiter((len(r) for r in rows), np.int32, len(rows))
    flat = np.frombuffer(b"".join(r[:width].ljust(width, b"\0") for r in rows), np.uint8)
    text = torch.from_numpy(flat.reshape(len(rows), width).copy())
    out = text, torch.from_numpy(length)
    return out if device is None else tuple(t.to(device) for t in out)


def read_smiles(strings_or_tensor, max_nodes: int = 4096, engine=None, device=None) -> SmilesRecords:
    """The result record of every SMILES string in one launch of ``dsp_read_smiles`` (``csrc/ds_reader.hip``; every definition in
    ``include/diffspectra_reader.h``): an OpenSMILES subset over H, C, N, O, F with aromatic symbols resolved to the first Kekule structure of a
    stated search, implied hydrogens appended behind the atoms of the string, positions zero.  ``strings_or_tensor``: a list of ``str``
    (``pack_smiles`` packs it on the host; ``device`` defaults to ``cuda``), a ``Smiles`` result, or a ``(text [P, stride] u8, length [P] i32)``
    pair of GPU tensors.  NOT RDKit's reader: no sanitisation (``valence_batch`` checks the record), stereo marks, isotopes and classes are read
    and dropped with a flag.  Device tensors, no synchronisation."""
    from . import engine as E
    if isinstance(strings_or_tensor, Smiles):
        text, length = strings_or_tensor.text, strings_or_tensor.length
    elif isinstance(strings_or_tensor, (tuple, list)) and len(strings_or_tensor) == 2 and torch.is_tensor(strings_or_tensor[0]):
        text, length = strings_or_tensor
    else:
        text, length = pack_smiles(list(strings_or_tensor), device if device is not None else "cuda")
    length = torch.as_tensor(length).to(device=text.device, dtype=torch.int32).contiguous()
    return SmilesRecords(*(engine if engine is not None else E).read_smiles(text, length, max_nodes))


def records_from_smiles(strings, max_nodes: int = 4096, engine=None, device=None):
    """``(records, n_atoms)`` of the strings that read ok, for ``known_records=`` of ``diffspectra_evaluate``, ``novelty`` and
    ``get_edm_metric_2d(known=...)``: a ``train_smiles`` list becomes a record table in one launch.  The strings that do not read are dropped
    (``read_smiles`` says why)."""
    got = read_smiles(strings, max_nodes=max_nodes, engine=engine, device=device)
    keep = got.ok
    return got.records[keep].contiguous(), got.n_atoms[keep].contiguous()


# ------------------------------------------------------------------------------------------------------------------ substructure queries, MACCS

class SubstructureMatches(NamedTuple):
    """Per-record device tensors of ``dsq_match_records``; K patterns."""
    count: torch.Tensor           # [P, K] u8: distinct atom sets over the embeddings (RDKit's uniquified match count), saturating at 4
    truncated: torch.Tensor       # [P, K] bool: a search stopped at ``max_nodes``; the entry holds what was found before
    anchors: torch.Tensor         # [P, K] i32: bit i = record atom i takes pattern atom 0 in some embedding
    cover: torch.Tensor           # [P, K] i32: bit i = record atom i takes part in some embedding
    aromatic_mask: torch.Tensor   # [P] i32: bit i = atom i is aromatic (the project's rule; unpinned against RDKit)
    aromatic_rings: torch.Tensor  # [P] i32: distinct aromatic cycles (atom sets), saturating at 4
    fragments: torch.Tensor       # [P] i32: connected components
    status: torch.Tensor          # [P] u8: 0 ok, 2 unusable (n = 0, a type above 4, a bond byte above 3): the row is 0

    def has(self, i: int) -> torch.Tensor:
        """``[P] bool``: the record contains pattern ``i`` (False for an unusable record)."""
        return self.count[:, i] > 0


class MaccsKeys(NamedTuple):
    """What ``maccs_keys`` returns."""
    bits: torch.Tensor            # [P, 167] bool: column k = MACCS key k; column 0 is unused and False; an unusable row is all False
    status: torch.Tensor          # [P] u8: 0 ok, 2 unusable
    truncated: torch.Tensor       # [P] bool: some pattern's search stopped at the budget (the keys are then a lower bound)


class MaccsSimilarity(NamedTuple):
    """Per-pair tensors of ``maccs_similarity_batch``."""
    common: torch.Tensor          # [P] i32: keys both molecules set; -1 for a pair that is not ok
    either: torch.Tensor          # [P] i32: keys at least one of them sets; -1 for a pair that is not ok
    tanimoto: torch.Tensor        # [P] f64: common / either, 1.0 when either = 0, NaN for a pair that is not ok
    status: torch.Tensor          # [P] u8: 0 ok, 2 a record of the pair is unusable, 3 invalid row
    truncated: torch.Tensor       # [P] bool: a search of either molecule stopped at the budget (its keys are a lower bound); False for an invalid row

    @property
    def valid(self) -> torch.Tensor:
        return self.status == 0


def _pattern_tensor(patterns, device) -> torch.Tensor:
    """``[K, 32] i32`` on ``device`` from pattern texts (compiled by ``smarts.compile_patterns``), a numpy array or a tensor of compiled rows."""
    from . import smarts
    if isinstance(patterns, str):
        patterns = [patterns]
    if torch.is_tensor(patterns):
        out = patterns
    elif hasattr(patterns, "dtype"):
        out = torch.from_numpy(patterns)
    else:
        out = torch.from_numpy(smarts.compile_patterns(list(patterns)))
    if out.dtype != torch.int32 or out.dim() != 2 or out.shape[1] != smarts.WORDS:
        raise ValueError(f"compiled patterns are int32 [K, {smarts.WORDS}], got {out.dtype} {list(out.shape)}")
    return out.to(device).contiguous()


def substructure_search(records: torch.Tensor, n_atoms, patterns, max_nodes: Optional[int] = None, engine=None) -> SubstructureMatches:
    """Every pattern against every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsq_match_records`` (``csrc/ds_substructure.hip``;
    every definition in ``include/diffspectra_substructure.h``).  ``patterns``: texts of the SMARTS subset of ``smarts.py``, or rows already
    compiled by it (``int32 [K, 32]``); at most 256 per call.  ``max_nodes``: the assignments one start atom's search may make (``None``:
    ``DSQ_DEFAULT_NODES``).  Matching runs on the hydrogen-folded graph with the project's aromaticity rule, unpinned against RDKit.  Device
    tensors, no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    words = _pattern_tensor(patterns, records.device)
    budget = E.SUBSTRUCTURE_DEFAULT_NODES if max_nodes is None else max_nodes
    count, anchors, cover, aromatic, rings, fragments, status = (engine if engine is not None else E).substructure_records(records, n, words, budget)
    flag = E.SUBSTRUCTURE_TRUNCATED
    return SubstructureMatches(torch.bitwise_and(count, flag - 1), torch.bitwise_and(count, flag) != 0, anchors, cover, aromatic, rings, fragments, status)


_MACCS_TABLE = None


def _maccs_table():
    """The compiled MACCS patterns and how the keys read them, built once."""
    global _MACCS_TABLE
    if _MACCS_TABLE is None:
        from . import maccs, smarts
        texts, single, anchored = maccs.pattern_table()
        _MACCS_TABLE = (torch.from_numpy(smarts.compile_patterns(texts)), single, anchored)
    return _MACCS_TABLE


def _popcount29(x: torch.Tensor) -> torch.Tensor:
    """Set bits of atom masks (bits 0..28) as i64, by plain tensor ops."""
    shifts = torch.arange(29, device=x.device, dtype=torch.int32)
    return torch.bitwise_and(torch.bitwise_right_shift(x.to(torch.int32).unsqueeze(-1), shifts), 1).sum(dim=-1)


def maccs_keys(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None) -> MaccsKeys:
    """The 166 MACCS keys of every record of ``records [P, 1248] u8`` (GPU): one ``substructure_search`` with the table of ``maccs.py`` and plain
    tensor ops on its outputs.  Key k is column k of ``bits [P, 167]`` (column 0 unused), set iff the key's matches exceed its threshold: the
    uniquified match count of a single pattern, the number of anchor atoms of a key that RDKit writes as one recursive atom, ``aromatic_rings >
    1`` for key 125 and ``fragments > 1`` for key 166.  The table restates RDKit's ``MACCSkeys.smartsPatts`` as remembered: parity with RDKit is
    UNPINNED (``maccs.py`` lists the deviations).  Device tensors, no synchronisation."""
    from . import maccs
    words, single, anchored = _maccs_table()
    found = substructure_search(records, n_atoms, words, max_nodes=max_nodes, engine=engine)
    dev = found.count.device
    bits = torch.zeros(found.count.shape[0], maccs.NUM_KEYS + 1, dtype=torch.bool, device=dev)
    keys = torch.tensor([k for k, _, _ in single], dtype=torch.int64, device=dev)
    cols = torch.tensor([c for _, c, _ in single], dtype=torch.int64, device=dev)
    more = torch.tensor([t for _, _, t in single], dtype=torch.int32, device=dev)
    bits[:, keys] = found.count[:, cols].to(torch.int32) > more.unsqueeze(0)
    for key, columns, threshold in anchored:
        atoms = found.anchors[:, columns[0]]
        for c in columns[1:]:
            atoms = torch.bitwise_or(atoms, found.anchors[:, c])
        bits[:, key] = _popcount29(atoms) > threshold
    bits[:, 125] = found.aromatic_rings > 1
    bits[:, 166] = found.fragments > 1
    return MaccsKeys(bits, found.status, found.truncated.any(dim=1))


def maccs_similarity_batch(prb, prb_n, ref, ref_n, ref_index=None, max_nodes: Optional[int] = None, engine=None) -> MaccsSimilarity:
    """The reference's "Tanimoto Similarity (MACCS)" (``compute_metrics.py:248-252``) of every generated record ``prb [P, 1248] u8`` and its ground
    truth among ``ref [M, 1248] u8`` (both on the GPU; ``ref_index [P]`` names the row, ``None``: row p for pair p - the record-pairs contract):
    ``maccs_keys`` once per table, then tensor ops.  ``tanimoto`` = common / either as f64, 1.0 when neither molecule sets a key (the
    convention of the functional-group line); a row outside the table is invalid (status 3) and reads nothing; a pair with an unusable record
    has status 2.  Parity with RDKit's MACCS keys is UNPINNED (``maccs.py``).  Device tensors, no synchronisation."""
    mine, theirs = maccs_keys(prb, prb_n, max_nodes=max_nodes, engine=engine), maccs_keys(ref, ref_n, max_nodes=max_nodes, engine=engine)
    dev = mine.bits.device
    P, M = mine.bits.shape[0], theirs.bits.shape[0]
    if ref_index is None and M < P:
        raise ValueError(f"without ref_index pair p reads ground-truth row p: {M} rows for {P} pairs")
    idx = torch.arange(P, device=dev) if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).reshape(-1)
    if idx.numel() != P:
        raise ValueError(f"ref_index must name one ground-truth row per pair: {idx.numel()} for {P}")
    inside = (idx >= 0) & (idx < M)
    row = torch.where(inside, idx, torch.zeros_like(idx))
    if M:
        r_bits, r_status, r_cut = theirs.bits.to(dev)[row], theirs.status.to(dev)[row], theirs.truncated.to(dev)[row]
    else:
        r_bits, r_status, r_cut = torch.zeros_like(mine.bits), torch.zeros_like(mine.status), torch.zeros_like(mine.truncated)
    status = torch.where(inside, torch.maximum(mine.status, r_status), torch.full_like(mine.status, 3))
    ok = status == 0
    minus = torch.full((P,), -1, dtype=torch.int32, device=dev)
    common = torch.where(ok, (mine.bits & r_bits).sum(dim=1).to(torch.int32), minus)
    either = torch.where(ok, (mine.bits | r_bits).sum(dim=1).to(torch.int32), minus)
    c, u = common.double(), either.double()
    sim = torch.where(either == 0, torch.ones_like(c), c / torch.where(either == 0, torch.ones_like(u), u))
    return MaccsSimilarity(common, either, torch.where(ok, sim, torch.full_like(sim, float("nan"))), status, inside & (mine.truncated | r_cut))


def topk_maccs(tanimoto: torch.Tensor, status: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions of ``maccs_similarity_batch`` over the K consecutive candidates of every spectrum, shaped like ``topk_morgan``: ``best
    [S] f64`` (the largest similarity among the ok candidates, NaN when none of the K is ok), ``best_index [S] i64`` (the first candidate with it,
    -1 when none is ok) and ``mean_best`` (a 0-dim f64 tensor; NaN without any).  Plain torch reductions on the tensors' device."""
    if top_k < 1 or tanimoto.numel() % top_k or status.shape != tanimoto.shape:
        raise ValueError(f"{tanimoto.numel()} pairs (status: {status.numel()}) are not a whole number of top_k = {top_k} groups")
    return topk_morgan(torch.where(status == 0, tanimoto.to(torch.float64), torch.full_like(tanimoto, float("nan"), dtype=torch.float64)), top_k)


# ------------------------------------------------------------------------------------------------------------------ Fraggle similarity

class FraggleFragmentations(NamedTuple):
    """Per-record device tensors of ``dsf_fraggle_fragmentations``."""
    rows: torch.Tensor            # [P, 256, 4] i32: (kept-atom mask, cuts packed, kind, sum of the kept sizes) in the header's order; unused rows -1
    summary: torch.Tensor         # [P, 4] i32: matchable atoms, chain cut bonds, ring cut bonds, fragmentations (all of them)
    truncated: torch.Tensor       # [P] bool: there are more fragmentations than rows
    status: torch.Tensor          # [P] u8: 0 ok, 1 undecided, 2 unusable

    @property
    def n_fragmentations(self) -> torch.Tensor:
        return self.summary[:, 3]


class PathFingerprints(NamedTuple):
    """Per-record device tensors of ``dsf_path_fingerprints``."""
    fp: torch.Tensor              # [P, 32] i32: 1024 bits
    atom_bits: torch.Tensor       # [P, 29, 32] i32: the bits of every atom
    count: torch.Tensor           # [P] i32: connected bond sets; -1 undecided, 0 unusable
    status: torch.Tensor          # [P] u8: 0 ok, 1 undecided, 2 unusable


class FraggleSimilarity(NamedTuple):
    """Per-pair device tensors of ``fraggle_similarity_batch``."""
    plain: torch.Tensor           # [P] f64: Tanimoto of the plain path fingerprints; NaN for a pair that is not ok
    modified: torch.Tensor        # [P] f64: the best Tanimoto of the marked molecules over the fragmentations; NaN without one or when not ok
    fraggle: torch.Tensor         # [P] f64: 0 without a fragmentation, else max(plain, modified); NaN for a pair that is not ok
    best_index: torch.Tensor      # [P] i32: the fragmentation behind ``modified``, -1 without one
    n_fragmentations: torch.Tensor  # [P] i32: the fragmentations of the ground truth
    marked: torch.Tensor          # [P, 2] i32: the marked-atom masks of the ground truth and of the generated molecule for that fragmentation
    status: torch.Tensor          # [P] u8: 0 ok, 1 undecided, 2 a record of the pair is unusable, 3 invalid row
    counts: torch.Tensor          # [P, 4] i32: (common, either) of plain and of modified, as the kernel gives them

    @property
    def valid(self) -> torch.Tensor:
        return self.status == 0


def fraggle_fragmentations(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None) -> FraggleFragmentations:
    """The Fraggle fragmentations of every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsf_fraggle_fragmentations``
    (``csrc/ds_fraggle.hip``; every definition in ``include/diffspectra_fraggle.h``, a restatement of RDKit's Fraggle as remembered and
    unpinned against it).  Device tensors, no synchronisation."""
    from . import engine as E
    rows, summary, status = (engine if engine is not None else E).fraggle_fragmentations(records, _i32_on(records, n_atoms), max_nodes)
    flag = E.FRAGGLE_TRUNCATED
    return FraggleFragmentations(rows, torch.bitwise_and(summary, torch.tensor([-1, -1, -1, flag - 1], dtype=torch.int32, device=summary.device)),
                                 torch.bitwise_and(summary[:, 3], flag) != 0, status)


def path_fingerprints(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None) -> PathFingerprints:
    """The branched path fingerprint (1..5 bonds, 1024 bits, 2 bits per bond set; the project's own hash) of every record of ``records
    [P, 1248] u8`` (GPU) with the bits of every atom, in one launch of ``dsf_path_fingerprints``.  Device tensors, no synchronisation."""
    from . import engine as E
    return PathFingerprints(*(engine if engine is not None else E).path_fingerprints(records, _i32_on(records, n_atoms), max_nodes))


def fraggle_similarity_batch(prb, prb_n, ref, ref_n, ref_index=None, max_nodes: Optional[int] = None, engine=None) -> FraggleSimilarity:
    """The reference's "Fraggle similarity" (``compute_metrics.py:273-291``: ``GetFraggleSimilarity(true_mol, pred_mol)``) of every generated
    record ``prb [P, 1248] u8`` and its ground truth among ``ref [M, 1248] u8`` (both on the GPU; ``ref_index [P]`` names the row, ``None``: row p
    for pair p - the record-pairs contract) in one launch of ``dsf_fraggle_similarity_records``; the floats are one division per pair on its
    integers.  ``fraggle`` is 0 when the ground truth has no fragmentation (as RDKit gives it, even for identical molecules), else the larger
    of ``plain`` and ``modified``.  ``max_nodes``: the connected bond sets one fingerprint may have (``None``: ``DSF_DEFAULT_NODES``); a pair
    beyond it is undecided (status 1).  Stated deviations (``include/diffspectra_fraggle.h``): the rule is as remembered and unpinned against
    RDKit; the fingerprint hash and the aromaticity are the project's; ring cuts and the ring step of the marking are order-free restatements
    of RDKit's SSSR-based ones; both valid pieces of a ring cut count.  Device tensors, no synchronisation."""
    from . import engine as E
    dev = prb.device
    idx = None if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).contiguous()
    plain, modified, best, found, marked, status = (engine if engine is not None else E).fraggle_similarity_records(
        prb, _i32_on(prb, prb_n), ref, _i32_on(ref, ref_n), idx, max_nodes)
    nan = torch.full((prb.shape[0],), float("nan"), dtype=torch.float64, device=dev)

    def ratio(pair, defined):
        c, e = pair[:, 0].double(), pair[:, 1].double()
        return torch.where(defined, torch.where(pair[:, 1] == 0, torch.ones_like(c), c / torch.where(pair[:, 1] == 0, torch.ones_like(e), e)), nan)
    ok = status == 0
    has = ok & (found > 0)
    t_plain, t_modified = ratio(plain, ok), ratio(modified, has)
    fraggle = torch.where(ok, torch.where(has, torch.maximum(t_plain, torch.where(has, t_modified, t_plain)), torch.zeros_like(nan)), nan)
    return FraggleSimilarity(t_plain, t_modified, fraggle, best, found, marked, status, torch.cat([plain, modified], dim=1))


def topk_fraggle(fraggle: torch.Tensor, status: torch.Tensor, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions of ``fraggle_similarity_batch`` over the K consecutive candidates of every spectrum, shaped like ``topk_maccs``:
    ``best [S] f64`` (the largest similarity among the ok candidates, NaN when none of the K is ok), ``best_index [S] i64`` (the first candidate
    with it, -1 when none is ok) and ``mean_best`` (a 0-dim f64 tensor; NaN without any).  Plain torch reductions on the tensors' device."""
    if top_k < 1 or fraggle.numel() % top_k or status.shape != fraggle.shape:
        raise ValueError(f"{fraggle.numel()} pairs (status: {status.numel()}) are not a whole number of top_k = {top_k} groups")
    return topk_morgan(torch.where(status == 0, fraggle.to(torch.float64), torch.full_like(fraggle, float("nan"), dtype=torch.float64)), top_k)


# ------------------------------------------------------------------------------------------------------------------ stereo-aware identity

class StereoIdentity(NamedTuple):
    """Per-pair device tensors of ``dsc_stereo_identity_records``."""
    verdict: torch.Tensor     # [P] u8: 0 different, 1 identical, 2 undecided, 3 invalid row (as ``GraphIdentity``), 4 mirror image, 5 another stereoisomer, 6 unassigned
    nodes: torch.Tensor       # [P] i32 search nodes used
    found: torch.Tensor       # [P, 3] i32 isomorphisms, same, mirror met until the search stopped
    sites: torch.Tensor       # [P, 4] i32 tetrahedral sites and E/Z sites of the generated molecule, unassigned sites of it and of the ground truth
    map: torch.Tensor         # [P, 29] i32 the isomorphism behind verdict 1, 4, 5 or 6 (ground-truth atom of every generated atom), else -1

    @property
    def identical(self) -> torch.Tensor:
        return self.verdict == 1

    @property
    def mirror(self) -> torch.Tensor:
        return self.verdict == 4

    @property
    def stereoisomer(self) -> torch.Tensor:
        return self.verdict == 5

    @property
    def unassigned(self) -> torch.Tensor:
        return self.verdict == 6

    @property
    def undecided(self) -> torch.Tensor:
        return self.verdict == 2

    @property
    def same_constitution(self) -> torch.Tensor:
        """An isomorphism of the labelled graphs was found: what ``graph_identity_batch`` calls identical."""
        return (self.verdict == 1) | (self.verdict >= 4)


class StereoSites(NamedTuple):
    """Per-record device tensors of ``dsc_stereo_sites``; every mask holds a bit per atom."""
    tetra_site: torch.Tensor      # [P] i32 four-coordinate centres without twin neighbours
    tetra_assigned: torch.Tensor  # [P] i32 ... whose |V| reaches ``min_volume``
    tetra_positive: torch.Tensor  # [P] i32 ... with V > 0
    ez_site: torch.Tensor         # [P] i32 both ends of every E/Z double bond
    ez_assigned: torch.Tensor     # [P] i32 ... that is planar enough
    ez_cis: torch.Tensor          # [P] i32 ... whose lowest substituents are cis
    twin: torch.Tensor            # [P] i32 atoms with a twin
    volume: torch.Tensor          # [P, 29] f64 V of every tetrahedral site, NaN elsewhere
    status: torch.Tensor          # [P] u8 0 ok, 3 unusable (masks 0)


class Chirality(NamedTuple):
    """What ``chirality`` returns, per record."""
    chiral: torch.Tensor          # [P] u8: 1 a tetrahedral site and no mirror automorphism, 0 achiral or without such a site, 2 unassigned or undecided
    automorphisms: torch.Tensor   # [P] i32 automorphisms of the ordinal-labelled graph, -1 where the search ran out of its budget


def stereo_identity_batch(ref, prb, ref_index=None, max_nodes: int = 4096, min_volume: Optional[float] = None, min_planarity: Optional[float] = None,
                          exhaustive: bool = False, engine=None) -> StereoIdentity:
    """Identity of every generated molecule with its ground truth as a labelled graph AND as a stereoisomer, read from the positions of the
    records (``dsc_stereo_identity_records``; every definition in ``include/diffspectra_stereo.h``): tetrahedral centres by the sign of a
    volume, double bonds by cis / trans, ``min_volume`` / ``min_planarity`` (``None``: the header's 0.5 / 0.5) below which a site is unassigned.
    Closer to the InChIKey comparison of the reference's Top-1 than ``graph_identity_batch``, with stated deviations: no tautomer / charge
    normalisation, four-coordinate centres only (no three-coordinate N, no allenes, no helicity), perception by twins, parity with RDKit /
    InChI unpinned.  ``ref`` and ``prb`` are ``(records [*, 1248] u8, n_atoms [*])`` pairs on the GPU, ground truth first as in
    ``graph_identity_batch``; ``ref_index [P]`` names the ground-truth row of every generated molecule (``None``: row p).  ``topk_identity`` works
    on the verdict unchanged.  Device tensors, no synchronisation."""
    return StereoIdentity(*_pair_call("stereo_identity_records", engine, ref, prb, ref_index, max_nodes, min_volume, min_planarity, exhaustive))


def stereo_sites(records: torch.Tensor, n_atoms, min_volume: Optional[float] = None, min_planarity: Optional[float] = None, engine=None) -> StereoSites:
    """The twins and the stereo sites of every record of ``records [P, 1248] u8`` (GPU) in one launch of ``dsc_stereo_sites``.  Device tensors,
    no synchronisation."""
    from . import engine as E
    n = torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()
    masks, volume, status = (engine if engine is not None else E).stereo_sites(records, n, min_volume, min_planarity)
    return StereoSites(*masks.unbind(dim=1), volume, status)


def chirality(records: torch.Tensor, n_atoms, max_nodes: int = 4096, min_volume: Optional[float] = None, min_planarity: Optional[float] = None,
              engine=None) -> Chirality:
    """Is every molecule of ``records`` chiral in the sense of ``include/diffspectra_stereo.h``: it has a tetrahedral site and none of its
    automorphisms is a mirror (every record against itself, all automorphisms enumerated).  A meso compound is achiral; a molecule whose
    only stereo sites are double bonds is achiral.  Device tensors, no synchronisation."""
    own = stereo_identity_batch((records, n_atoms), (records, n_atoms), None, max_nodes, min_volume, min_planarity, True, engine)
    decided = own.verdict == 1
    chiral = torch.where(decided, ((own.sites[:, 0] > 0) & (own.found[:, 2] == 0)).to(torch.uint8), torch.full_like(own.verdict, 2))
    return Chirality(chiral, torch.where(own.verdict == 2, torch.full_like(own.found[:, 0], -1), own.found[:, 0]))


# ------------------------------------------------------------------------------------------------------------------ mobile hydrogens, the normal form

class MobileHydrogens(NamedTuple):
    """Per-record device tensors of ``dsm_mobile_records``."""
    fixed_h: torch.Tensor         # [P, 29] u8: fixed H of every kept atom (0 for a group member); 0xff for a folded hydrogen and for atoms >= n
    q_res: torch.Tensor           # [P, 29] i8: residual charge after the (de)protonation rule
    group_of: torch.Tensor        # [P, 29] u8: the mobile group of every member, 0xff elsewhere
    group_h: torch.Tensor         # [P, 14] u8: mobile H of every group, 0xff where unused
    summary: torch.Tensor         # [P, 4] i32: kept atoms, groups, mobile H in all, proton balance
    nodes: torch.Tensor           # [P] i32 search nodes used
    status: torch.Tensor          # [P] u8: 0 ok, 2 undecided (budget), 3 unusable: the byte outputs 0xff, the rest 0

    @property
    def ok(self) -> torch.Tensor:
        return self.status == 0

    @property
    def n_groups(self) -> torch.Tensor:
        return self.summary[:, 1]

    @property
    def proton_balance(self) -> torch.Tensor:
        return self.summary[:, 3]


class MobileIdentity(NamedTuple):
    """Per-pair device tensors of ``mobile_identity_batch``."""
    verdict: torch.Tensor         # [P] u8: 1 identical in the normal form, 0 different, 2 undecided (a budget, or a normal form over 29 nodes), 3 invalid
    strict: torch.Tensor          # [P] u8: the verdict of ``graph_identity_batch`` on the records as drawn
    layer: torch.Tensor           # [P] i8: 0 identical as drawn, 1 identical only in the normal form, -1 not identical
    map: torch.Tensor             # [P, 29] i32: ground-truth kept atom of every generated kept atom when identical, else -1
    prb_status: torch.Tensor      # [P] u8 status of the generated record's normal form (0 ok, 2 undecided, 3 unusable, 4 overflow)
    ref_status: torch.Tensor      # [P] u8 the same of its ground truth (3 for an invalid row)
    nodes: torch.Tensor           # [P] i32 search nodes of the comparison of the normal forms

    @property
    def identical(self) -> torch.Tensor:
        return self.verdict == 1

    @property
    def undecided(self) -> torch.Tensor:
        return self.verdict == 2


def _i32_on(records, n_atoms):
    return torch.as_tensor(n_atoms).to(device=records.device, dtype=torch.int32).contiguous()


def mobile_hydrogens(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None) -> MobileHydrogens:
    """The mobile-hydrogen groups (tautomers), fixed hydrogens, residual charges and proton balance of every record of ``records [P, 1248] u8``
    (GPU) in one launch of ``dsm_mobile_records`` (``csrc/ds_mobile.hip``; every definition in ``include/diffspectra_mobile.h``).  The rule
    restates InChI's mobile-H and (de)protonation normalisation as remembered and is unpinned against InChI, which cannot be run here.
    ``max_nodes``: the budget of the path search per record (``None``: 4096).  Device tensors, no synchronisation."""
    from . import engine as E
    return MobileHydrogens(*(engine if engine is not None else E).mobile_records(records, _i32_on(records, n_atoms), max_nodes))


def normal_form_records(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None):
    """``(out_rec [P, 1248] u8, out_n [P] i32, out_source [P, 29] u8, status [P] u8)``: every record in the normal form of
    ``include/diffspectra_mobile.h`` (``dsm_normal_records``), row p for record p: the kept atoms with their fixed hydrogens and residual
    charge in the charge byte, every bond as byte 1, a group node per mobile group, a proton node for a balance that is not 0.  ``out_source``
    is the original atom of every kept atom of the row.  Such records are outside the alphabet of the other analytics; ``graph_classes`` and
    ``graph_identity_batch`` compare raw bytes and decide their identity.  A row whose status is not 0 is empty.  No synchronisation."""
    from . import engine as E
    return (engine if engine is not None else E).normal_records(records, _i32_on(records, n_atoms), max_nodes)


def mobile_identity_batch(ref, prb, ref_index=None, max_nodes: int = 4096, engine=None) -> MobileIdentity:
    """Identity of every generated molecule with its ground truth up to mobile hydrogens (tautomers), acid / base forms and Kekule drawings:
    ``graph_identity_batch`` on the normal forms of ``normal_form_records`` - the level of the main layer of the standard InChI behind the
    reference's Top-1 (``compute_metrics.py:222-230``), with the deviations ``include/diffspectra_mobile.h`` states (the rule is unpinned
    against InChI; the stereo layer of ``stereo_identity_batch`` is not combined with it).  ``ref`` and ``prb`` are ``(records [*, 1248] u8,
    n_atoms [*])`` pairs on the GPU, ground truth first; ``ref_index [P]`` names the ground-truth row of every generated molecule (``None``:
    row p); ``max_nodes`` is the budget of the path searches and of both graph comparisons.  A pair with an unusable side is invalid (3), a
    pair with a side whose search ran out of its budget or whose normal form has more than 29 nodes is undecided (2).  ``topk_identity``
    works on ``verdict`` unchanged.  Device tensors, no synchronisation."""
    from . import engine as E
    eng = engine if engine is not None else E
    (ref_rec, ref_n), (prb_rec, prb_n) = ref, prb
    dev = prb_rec.device
    ref_n, prb_n = _i32_on(ref_rec, ref_n), _i32_on(prb_rec, prb_n)
    P, M = prb_rec.shape[0], ref_rec.shape[0]
    idx = None if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).contiguous()
    compare = min(max_nodes, E.GRAPH_MAX_NODES) if isinstance(max_nodes, int) else max_nodes      # (the bindings check the type)
    strict = eng.graph_identity_records(prb_rec, prb_n, ref_rec, ref_n, idx, compare)[0]
    p_rec, p_n, p_src, p_st = eng.normal_records(prb_rec, prb_n, max_nodes)
    r_rec, r_n, r_src, r_st = eng.normal_records(ref_rec, ref_n, max_nodes)
    verdict, nodes, image = eng.graph_identity_records(p_rec, p_n, r_rec, r_n, idx, compare)
    rows = torch.arange(P, device=dev) if idx is None else idx
    inside = (rows >= 0) & (rows < M)
    safe = torch.where(inside, rows, torch.zeros_like(rows))
    unusable, ok = E.MOBILE_UNUSABLE, E.MOBILE_OK
    ref_status = torch.where(inside, r_st[safe] if M else torch.zeros_like(p_st), torch.full_like(p_st, unusable))
    not_ok = (p_st != ok) | (ref_status != ok)
    invalid = (verdict == E.GRAPH_INVALID) | (p_st == unusable) | (ref_status == unusable)
    verdict = torch.where(invalid, torch.full_like(verdict, E.GRAPH_INVALID), torch.where(not_ok, torch.full_like(verdict, E.GRAPH_UNDECIDED), verdict))
    same = verdict == E.GRAPH_IDENTICAL
    layer = torch.where(same, (strict != E.GRAPH_IDENTICAL).to(torch.int8), torch.full((P,), -1, dtype=torch.int8, device=dev))
    # the map between normal-form rows, translated to original kept atoms on both sides
    out = torch.full((P, p_src.shape[1]), -1, dtype=torch.int32, device=dev)
    if P and M:
        target = r_src[safe].gather(1, image.clamp(min=0).to(torch.int64)).to(torch.int32)       # the original ground-truth atom of every row atom
        kept = same.unsqueeze(1) & (p_src != 0xff)
        p_at, slot = kept.nonzero(as_tuple=True)
        out[p_at, p_src[p_at, slot].to(torch.int64)] = target[p_at, slot]
    return MobileIdentity(verdict, strict, layer, out, p_st, ref_status, nodes)


def mobile_classes(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, engine=None) -> torch.Tensor:
    """``class_id [P] i64``: the lowest row whose molecule has the same normal form as row p's - ``graph_classes`` on the normal forms, for
    uniqueness and novelty up to tautomers, acid / base forms and Kekule drawings.  A row without a normal form (unusable, undecided or
    over 29 nodes) is a class of its own.  One read of the statuses."""
    out_rec, out_n, _, status = normal_form_records(records, n_atoms, max_nodes, engine)
    class_id = torch.arange(records.shape[0], dtype=torch.int64, device=records.device)
    rows = (status == 0).nonzero(as_tuple=True)[0]
    if rows.numel():
        class_id[rows] = rows[graph_classes(out_rec[rows].contiguous(), out_n[rows].contiguous(), engine)]
    return class_id


# ------------------------------------------------------------------------------------------------------------------ key-level identity

class KeySites(NamedTuple):
    """Per-record device tensors of ``dsi_key_sites``, in normal-form numbering (row p lines up with row p of ``normal_form_records``)."""
    site: torch.Tensor            # [P, 29, 2] u8: (flags, partner) of every node - kind 0 / 1 centre / 2 end in bits 0..1, 4 assigned, 8 sign or cis, 16 hydrogen slot; partner 255 off an E/Z site
    masks: torch.Tensor           # [P, 9] i32, a bit per node: the seven rows of ``StereoSites``, the ends of the double bonds on a shift path, the ends of the ring double bonds
    volume: torch.Tensor          # [P, 29] f64 V of every centre, 0 elsewhere
    nodes: torch.Tensor           # [P] i32 nodes of the exhaustive shift-path search
    status: torch.Tensor          # [P] u8: 0 ok, 2 undecided (budget), 3 unusable, 4 a normal form over 29 nodes: flags 0, partner 255, zeros

    @property
    def flags(self) -> torch.Tensor:
        return self.site[..., 0]

    @property
    def partner(self) -> torch.Tensor:
        return self.site[..., 1]

    @property
    def mobile_bond(self) -> torch.Tensor:
        return self.masks[:, 7]

    @property
    def ring_bond(self) -> torch.Tensor:
        return self.masks[:, 8]


class KeyIdentity(NamedTuple):
    """Per-pair device tensors of ``key_identity_batch``."""
    verdict: torch.Tensor         # [P] u8: the codes of ``StereoIdentity`` at the level of the normal form
    nodes: torch.Tensor           # [P] i32 search nodes of the comparison of the normal forms
    found: torch.Tensor           # [P, 3] i32 isomorphisms of the normal forms, same, mirror met until the search stopped
    sites: torch.Tensor           # [P, 4] i32 centres and E/Z sites of the generated molecule, unassigned sites of it and of the ground truth
    map: torch.Tensor             # [P, 29] i32: ground-truth kept atom of every generated kept atom behind verdict 1, 4, 5 or 6, else -1 (original atoms)
    strict: torch.Tensor          # [P] u8: the verdict of ``stereo_identity_batch`` on the records as drawn
    layer: torch.Tensor           # [P] i8: 0 identical as drawn, 1 identical only at this level, -1 not identical
    prb_status: torch.Tensor      # [P] u8 status of the generated record's sites (0 ok, 2 undecided, 3 unusable, 4 overflow)
    ref_status: torch.Tensor      # [P] u8 the same of its ground truth (3 for an invalid row)

    @property
    def identical(self) -> torch.Tensor:
        return self.verdict == 1

    @property
    def mirror(self) -> torch.Tensor:
        return self.verdict == 4

    @property
    def stereoisomer(self) -> torch.Tensor:
        return self.verdict == 5

    @property
    def unassigned(self) -> torch.Tensor:
        return self.verdict == 6

    @property
    def undecided(self) -> torch.Tensor:
        return self.verdict == 2


def key_sites(records: torch.Tensor, n_atoms, max_nodes: Optional[int] = None, min_volume: Optional[float] = None,
              min_planarity: Optional[float] = None, engine=None) -> KeySites:
    """The stereo sites of every record of ``records [P, 1248] u8`` (GPU) at the level of its normal form, in one launch of ``dsi_key_sites``
    (``csrc/ds_key.hip``; every definition in ``include/diffspectra_key.h``, which restates InChI as remembered and is unpinned against it).
    ``max_nodes``: the budget of the shift-path search per record (``None``: 4096).  Device tensors, no synchronisation."""
    from . import engine as E
    return KeySites(*(engine if engine is not None else E).key_sites(records, _i32_on(records, n_atoms), max_nodes, min_volume, min_planarity))


def key_identity_batch(ref, prb, ref_index=None, max_nodes: int = 4096, min_volume: Optional[float] = None, min_planarity: Optional[float] = None,
                       exhaustive: bool = False, engine=None) -> KeyIdentity:
    """Identity of every generated molecule with its ground truth at the level of an InChIKey: up to mobile hydrogens, acid / base forms and
    Kekule drawings (``mobile_identity_batch``) AND in the arrangement of its centres and double bonds (``stereo_identity_batch``), both at
    once - the comparison behind the reference's Top-1 (``compute_metrics.py:222-230``), with the deviations ``include/diffspectra_key.h``
    states: the rules restate InChI as remembered and the number is UNPINNED against InChI.  ``ref`` and ``prb`` are ``(records [*, 1248] u8,
    n_atoms [*])`` pairs on the GPU, ground truth first; ``ref_index [P]`` names the ground-truth row of every generated molecule (``None``:
    row p); ``max_nodes`` is the budget of the path searches and of the comparisons.  A pair with an unusable side is invalid (3), a pair with
    a side over a budget or over 29 nodes is undecided (2).  ``topk_identity`` works on ``verdict`` unchanged.  Device tensors, no
    synchronisation."""
    from . import engine as E
    eng = engine if engine is not None else E
    (ref_rec, ref_n), (prb_rec, prb_n) = ref, prb
    dev = prb_rec.device
    ref_n, prb_n = _i32_on(ref_rec, ref_n), _i32_on(prb_rec, prb_n)
    P, M = prb_rec.shape[0], ref_rec.shape[0]
    idx = None if ref_index is None else torch.as_tensor(ref_index).to(device=dev, dtype=torch.int64).contiguous()
    compare = min(max_nodes, E.GRAPH_MAX_NODES) if isinstance(max_nodes, int) else max_nodes      # (the bindings check the type)
    strict = eng.stereo_identity_records(prb_rec, prb_n, ref_rec, ref_n, idx, compare, min_volume, min_planarity, exhaustive)[0]
    p_rec, p_n, p_src, _ = eng.normal_records(prb_rec, prb_n, max_nodes)
    r_rec, r_n, r_src, _ = eng.normal_records(ref_rec, ref_n, max_nodes)
    p_site, _, _, _, p_st = eng.key_sites(prb_rec, prb_n, max_nodes, min_volume, min_planarity)
    r_site, _, _, _, r_st = eng.key_sites(ref_rec, ref_n, max_nodes, min_volume, min_planarity)
    verdict, nodes, found, sites, image = eng.key_identity_records(p_rec, p_n, p_site, r_rec, r_n, r_site, idx, compare, exhaustive)
    rows = torch.arange(P, device=dev) if idx is None else idx
    inside = (rows >= 0) & (rows < M)
    safe = torch.where(inside, rows, torch.zeros_like(rows))
    unusable, ok = E.MOBILE_UNUSABLE, E.MOBILE_OK
    ref_status = torch.where(inside, r_st[safe] if M else torch.zeros_like(p_st), torch.full_like(p_st, unusable))
    not_ok = (p_st != ok) | (ref_status != ok)
    invalid = (verdict == E.STEREO_INVALID) | (p_st == unusable) | (ref_status == unusable)
    verdict = torch.where(invalid, torch.full_like(verdict, E.STEREO_INVALID), torch.where(not_ok, torch.full_like(verdict, E.STEREO_UNDECIDED), verdict))
    same = verdict == E.STEREO_IDENTICAL
    layer = torch.where(same, (strict != E.STEREO_IDENTICAL).to(torch.int8), torch.full((P,), -1, dtype=torch.int8, device=dev))
    # the map between normal-form rows, translated to original kept atoms on both sides
    out = torch.full((P, p_src.shape[1]), -1, dtype=torch.int32, device=dev)
    if P and M:
        target = r_src[safe].gather(1, image.clamp(min=0).to(torch.int64)).to(torch.int32)       # the original ground-truth atom of every row atom
        mapped = (same | (verdict >= E.STEREO_MIRROR)).unsqueeze(1) & (p_src != 0xff) & (image >= 0)
        p_at, slot = mapped.nonzero(as_tuple=True)
        out[p_at, p_src[p_at, slot].to(torch.int64)] = target[p_at, slot]
    return KeyIdentity(verdict, nodes, found, sites, out, strict, layer, p_st, ref_status)


# ------------------------------------------------------------------------------------------------------------------ symmetry-corrected Kabsch RMSD

class BestRmsd(NamedTuple):
    """Per-pair device tensors of ``dsr_best_rmsd_records``."""
    verdict: torch.Tensor     # [P] u8: 0 no isomorphism (proven), 1 decided, 2 undecided (budget), 3 invalid row (as ``GraphIdentity``)
    rmsd: torch.Tensor        # [P, 2] f64 the smallest proper / improper (mirror image) Kabsch RMSD over every isomorphism; NaN unless verdict 1
    count: torch.Tensor       # [P] i32 selected atoms of the generated molecule
    nodes: torch.Tensor       # [P] i32 search nodes used
    found: torch.Tensor       # [P] i32 isomorphisms met
    map: torch.Tensor         # [P, 2, 29] i32 the isomorphisms behind the two values (ground-truth atom of every generated atom), else -1

    @property
    def decided(self) -> torch.Tensor:
        return self.verdict == 1

    @property
    def undecided(self) -> torch.Tensor:
        return self.verdict == 2

    @property
    def mirror_better(self) -> torch.Tensor:
        """The mirror image of the generated molecule fits the ground truth better than the molecule itself."""
        return (self.verdict == 1) & (self.rmsd[:, 1] < self.rmsd[:, 0])


def best_rmsd_batch(ref, prb, ref_index=None, atoms: str = "heavy", max_nodes: int = 4096, engine=None) -> BestRmsd:
    """How good the geometry of every hit is: the smallest Kabsch RMSD over ALL graph isomorphisms between every generated molecule and its
    ground truth (``dsr_best_rmsd_records``; every definition in ``include/diffspectra_rmsd.h``), what RDKit's ``GetBestRMS`` and ``spyrmsd``
    compute - rotation invariant, bond consistent, and symmetry (methyl groups, CF2, benzene, cubane) cannot inflate it - with the value of the
    best fit of the mirror image beside it.  ``atoms``: ``'heavy'`` (type not 0; twin hydrogens are not permuted) or ``'all'`` (every
    isomorphism is enumerated: ``max_nodes`` decides).  Stated deviations: unpinned against RDKit / spyrmsd, no mass weighting.  ``ref`` and
    ``prb`` are ``(records [*, 1248] u8, n_atoms [*])`` pairs on the GPU, ground truth first as in ``graph_identity_batch``; ``ref_index [P]``
    names the ground-truth row of every generated molecule (``None``: row p).  Device tensors, no synchronisation."""
    return BestRmsd(*_pair_call("best_rmsd_records", engine, ref, prb, ref_index, max_nodes, atoms))


def topk_best_rmsd(best, top_k: int) -> Dict[str, torch.Tensor]:
    """Best-of-K reductions over the K consecutive candidates of every spectrum from a ``BestRmsd`` (or any object / dict with ``verdict [S*K]``
    and ``rmsd [S*K, 2]``): ``hit [S] bool`` (a candidate is the ground-truth graph: verdict 1), ``best_rmsd [S] f64`` (the lowest proper RMSD
    among the spectrum's hits with a value, NaN if none), ``best_index [S] i64`` (that candidate, -1 if none) and ``undecided`` (0-dim i64
    count).  Plain torch reductions on the tensors' device."""
    get = (lambda k: best[k]) if isinstance(best, dict) else (lambda k: getattr(best, k))
    verdict, rmsd = get("verdict"), get("rmsd")
    if top_k < 1 or verdict.numel() % top_k:
        raise ValueError(f"{verdict.numel()} pairs are not a whole number of top_k = {top_k} groups")
    same = (verdict == 1).reshape(-1, top_k)
    r = rmsd[:, 0].reshape(-1, top_k).to(torch.float64)
    bad = torch.isnan(r) | ~same
    filled = torch.where(bad, torch.full_like(r, float("inf")), r)
    value, arg = filled.min(dim=1)
    none = bad.all(dim=1)
    value = torch.where(none, torch.full_like(value, float("nan")), value)
    arg = torch.where(none, torch.full_like(arg, -1), arg)
    return dict(hit=same.any(dim=1), best_rmsd=value, best_index=arg, undecided=(verdict == 2).sum())
