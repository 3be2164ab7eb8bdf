"""The reference's metric table for TEXT pairs (``compute_metrics.py:96-114,147-317``): predicted and true SMILES strings in, the seven-line
table out - Top-1, MCES, Tanimoto / cosine (Morgan), Tanimoto (MACCS), Fraggle, functional groups - with every molecule read and scored on the
GPU: ``structure_metrics.read_smiles`` (``dsp_read_smiles``, one launch for all strings) and then the record-level calls the rest of the
evaluation uses.  No per-molecule Python.

Stated deviations from the reference.
  * Conversion.  A pair is CONVERTED iff both strings read ok (``include/diffspectra_reader.h``) and both records pass
    ``valence_batch(...).valid`` - the project's stand-in for ``MolFromSmiles(...) is not None``.  Parity with RDKit's reader is UNPINNED (RDKit
    is not available to the tests); the reader is pinned by hand tables and by the round trip with the project's writer.
  * Tautomers.  The reference canonicalises the tautomer of both molecules before EVERY metric; here only Top-1 is tautomer-aware.
  * Top-1 is ``mobile_identity_batch``: the level of an InChI main layer.  The text's stereo marks are not read and read records have no
    coordinates, so ``key_identity_batch`` does not apply - nor does any other geometry-reading call (``hungarian_rmsd_batch``,
    ``best_rmsd_batch``, ``stereo_*``, ``key_*``, ``sub_geometry``); the evaluator never calls them.
  * ``smiles_exact_match`` (the reference's unused ``true_smi == pred_smi`` count) is reported as an extra number.
  * Each metric's deviations from RDKit's number are those of its own call (Kekule orders in the Morgan invariant, the restated MACCS and
    Fraggle definitions, the project's aromaticity in the functional groups).
Means are taken over the converted pairs; for a line whose call leaves some of them undecided or invalid, over the pairs it decided."""
from __future__ import annotations

import csv
import json
from typing import Dict, List, Sequence, Tuple

import torch

from . import structure_metrics as S

PREFIX = "##SMILES: "
METRIC_NAMES = ("Top-1 Accuracy", "MCES", "Tanimoto Similarity (Morgan)", "Cosine Similarity (Morgan)", "Tanimoto Similarity (MACCS)",
                "Fraggle Similarity", "Functional Group Similarity")


def load_smiles_from_jsonl(jsonl_path: str) -> List[Tuple[str, str]]:
    """``[(predicted, true)]`` of a JSONL file of ``{"predict": "##SMILES: ...", "label": "##SMILES: ..."}`` lines (blank lines skipped)."""
    pairs = []
    with open(jsonl_path, "r", encoding="utf-8") as f:
        for line in f:
            if line.strip():
                data = json.loads(line)
                pairs.append((data["predict"].replace(PREFIX, ""), data["label"].replace(PREFIX, "")))
    return pairs


def load_smiles_from_tsv(tsv_path: str) -> List[Tuple[str, str]]:
    """``[(generated, ground truth)]`` of the ``slot<TAB>generated<TAB>ground truth`` file that ``diffspectra_evaluate`` writes with
    ``config.eval.smiles_path`` (an empty field - a record without a string - stays an empty string and reads as ``empty``)."""
    pairs = []
    with open(tsv_path, "r", encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if line:
                fields = line.split("\t")
                if len(fields) != 3:
                    raise ValueError(f"{tsv_path}: expected slot<TAB>generated<TAB>ground truth, got {line!r}")
                pairs.append((fields[1], fields[2]))
    return pairs


def _mean(values: torch.Tensor, keep: torch.Tensor):
    picked = values.double()[keep]
    return float(picked.mean()) if picked.numel() else None


def evaluate_smiles_pairs(pred: Sequence[str], true: Sequence[str], engine=None, device=None) -> Dict:
    """The metric table of ``len(pred)`` (predicted, true) string pairs.  Returns a dict with the seven ``METRIC_NAMES`` (means over the
    converted pairs, ``None`` without any), ``smiles_exact_match``, the counts ``pairs`` / ``converted`` / ``invalid`` (``invalid``: a dict
    with the total, the pairs lost to the valence check and the unread strings by reader status on each side), ``converted_mask`` (a list of
    bools) and ``detailed`` ({metric name: one value per converted pair})."""
    if len(pred) != len(true):
        raise ValueError(f"one true string per predicted string: {len(true)} for {len(pred)}")
    P = len(pred)
    got = S.read_smiles(list(pred) + list(true), engine=engine, device=device)
    valid = got.ok & S.valence_batch(got.records, got.n_atoms, engine=engine).valid
    converted = valid[:P] & valid[P:]
    status = got.status.cpu()
    by_status = lambda side: {name: int((side == k).sum()) for k, name in enumerate(S.READER_STATUS_NAMES) if k and int((side == k).sum())}
    unread = (got.status[:P] != 0) | (got.status[P:] != 0)
    out: Dict = dict(pairs=P, converted=int(converted.sum()),
                     invalid=dict(total=P - int(converted.sum()), valence=int((~converted & ~unread).sum()), predicted=by_status(status[:P]),
                                  true=by_status(status[P:])),
                     converted_mask=converted.cpu().tolist())
    keep = converted.nonzero().reshape(-1)
    prb = (got.records[:P][keep].contiguous(), got.n_atoms[:P][keep].contiguous())
    ref = (got.records[P:][keep].contiguous(), got.n_atoms[P:][keep].contiguous())
    if keep.numel() == 0:
        out.update({name: None for name in METRIC_NAMES}, smiles_exact_match=None, detailed={name: [] for name in METRIC_NAMES})
        return out
    top1 = S.mobile_identity_batch(ref, prb, engine=engine)
    mces = S.mces_batch(ref, prb, engine=engine)
    morgan = S.morgan_similarity_batch(ref, prb, engine=engine)
    maccs = S.maccs_similarity_batch(prb[0], prb[1], ref[0], ref[1], engine=engine)
    fraggle = S.fraggle_similarity_batch(prb[0], prb[1], ref[0], ref[1], engine=engine)
    groups = S.functional_group_similarity_batch(ref, prb, engine=engine)
    exact = S.smiles_exact_match(ref, prb, engine=engine)
    every = torch.ones_like(converted[keep])
    columns = (("Top-1 Accuracy", top1.identical, every), ("MCES", mces.dist, mces.status != 3),
               ("Tanimoto Similarity (Morgan)", morgan.tanimoto, morgan.valid), ("Cosine Similarity (Morgan)", morgan.cosine, morgan.valid),
               ("Tanimoto Similarity (MACCS)", maccs.tanimoto, maccs.valid), ("Fraggle Similarity", fraggle.fraggle, fraggle.valid),
               ("Functional Group Similarity", groups.similarity, groups.valid))
    detailed = {}
    for name, values, decided in columns:
        out[name] = _mean(values, decided)
        host, ok = values.cpu().tolist(), decided.cpu().tolist()
        detailed[name] = [(bool(v) if name == "Top-1 Accuracy" else v) if k else None for v, k in zip(host, ok)]
    out["smiles_exact_match"] = _mean(exact.same, every)
    out["detailed"] = detailed
    return out


def _pairs_of(input_data) -> Tuple[List[str], List[str]]:
    if isinstance(input_data, str):
        pairs = load_smiles_from_jsonl(input_data) if input_data.endswith((".jsonl", ".json")) else load_smiles_from_tsv(input_data)
        return [p for p, _ in pairs], [t for _, t in pairs]
    true, pred = input_data                                          # the reference's order: (true_mols, pred_mols)
    return [p[0] if isinstance(p, (list, tuple)) else p for p in pred], list(true)


def write_tables(result: Dict, output_csv: str) -> Tuple[str, str, str]:
    """The reference's three files of a result: the two-column ``Evaluation Metric,Value`` CSV with four decimals, ``_detailed_scores.csv``
    (a column per metric, a row per converted pair) and ``_detailed_scores.json``; ``utf-8-sig`` for the CSVs.  Returns the three paths."""
    detailed_csv, detailed_json = output_csv.replace(".csv", "_detailed_scores.csv"), output_csv.replace(".csv", "_detailed_scores.json")
    with open(output_csv, "w", newline="", encoding="utf-8-sig") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["Evaluation Metric", "Value"])
        for name in METRIC_NAMES:
            w.writerow([name, "nan" if result[name] is None else f"{result[name]:.4f}"])
    detailed = result["detailed"]
    with open(detailed_csv, "w", newline="", encoding="utf-8-sig") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(METRIC_NAMES)
        for row in zip(*(detailed[name] for name in METRIC_NAMES)):
            w.writerow(["" if v is None else v for v in row])
    with open(detailed_json, "w", encoding="utf-8") as f:
        json.dump({name: detailed[name] for name in METRIC_NAMES}, f, ensure_ascii=False, indent=2)
    return output_csv, detailed_csv, detailed_json


def evaluate_jsonl_predictions(input_data, output_csv: str = None, engine=None, device=None) -> Dict:
    """``compute_metrics.evaluate_jsonl_predictions`` on text.  ``input_data``: a JSONL path (``*.jsonl`` / ``*.json``: ``predict`` / ``label``
    keys), any other path (the ``slot<TAB>generated<TAB>ground truth`` file of ``config.eval.smiles_path``), or a ``(true, pred)`` pair of
    string lists (an inner list stands for its first string, as in the reference).  Returns the dict of ``evaluate_smiles_pairs``; with
    ``output_csv`` it also writes the three files of ``write_tables``."""
    pred, true = _pairs_of(input_data)
    result = evaluate_smiles_pairs(pred, true, engine=engine, device=device)
    if output_csv is not None:
        write_tables(result, output_csv)
    return result
