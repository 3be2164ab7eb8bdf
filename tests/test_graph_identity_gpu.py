"""GPU: ``ds_graph_identity_records`` and ``ds_graph_hash_records`` (one wave per pair / molecule) against the plain-Python mirror of
tests/graph_mirror.py - every verdict equal, every returned map checked here to be an isomorphism, no tolerance anywhere - plus the hard
pairs, the edges of the shape, conformation independence, batch independence, the classes and the evaluation driver end to end."""
import functools

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from diffspectra_amd.structure_metrics import GraphIdentity, graph_classes, graph_identity_batch, topk_identity
from tests import graph_mirror as GM, structure_mirror as SM
from tests.helpers import run_records, to_dev

pytestmark = pytest.mark.gpu

_run = functools.partial(run_records, E.graph_identity_records, GraphIdentity)       # (dev, ref, prb, ref_index=None, **scalars) -> GraphIdentity of numpy arrays


def _check_maps(got, ref, prb, what=""):
    """verdict 1: the map is checked here, independently, to be a type-, charge- and bond-preserving bijection; any other verdict: all -1."""
    assert got.map.shape == (len(prb), SM.W)
    for p, (a, b) in enumerate(zip(prb, ref)):
        if got.verdict[p] == 1:
            n = len(a["type"])
            assert (got.map[p, n:] == -1).all() and GM.is_isomorphism(a, b, got.map[p]), f"{what} pair {p}: the map is no isomorphism"
        else:
            assert (got.map[p] == -1).all(), f"{what} pair {p}: verdict {got.verdict[p]} with a map"


def test_parity_on_seeded_pairs(gpu_device):
    ref, prb, kind = GM.seeded_pairs()
    want = GM.seeded_labels()
    assert len(ref) == 2000 and want[kind == 0].all()
    for k in (1, 3):                                                  # the set discriminates: both answers occur among the bond switches and type swaps
        assert 0.05 <= want[kind == k].mean() <= 0.95, (k, want[kind == k].mean())
    got = _run(gpu_device, ref, prb)
    print(f"[graph] 2000 pairs: {int(want.sum())} identical; nodes mean {got.nodes.mean():.3f} max {got.nodes.max()}; "
          f"disagreements {int((got.verdict != want).sum())}, undecided {int((got.verdict == 2).sum())}")
    assert (got.verdict != 2).all(), np.nonzero(got.verdict == 2)[0][:10]
    assert np.array_equal(got.verdict, want.astype(np.uint8)), np.nonzero(got.verdict != want)[0][:10]
    _check_maps(got, ref, prb, "seeded")
    assert (got.nodes >= 0).all() and (got.nodes <= 4096).all()


def test_hard_pairs(gpu_device):
    rng = np.random.default_rng(8)
    hard = GM.hard_pairs()
    cross_prb, cross_ref = [GM.permuted(a, rng) for _, a, b in hard] + [GM.permuted(b, rng) for _, a, b in hard], [b for _, a, b in hard] + [a for _, a, b in hard]
    got = _run(gpu_device, cross_ref, cross_prb)
    print(f"[graph] hard cross pairs: nodes {got.nodes.tolist()}")
    assert got.verdict.tolist() == [0] * len(cross_prb)              # proven different at the default budget
    _check_maps(got, cross_ref, cross_prb, "cross")
    plain = _run(gpu_device, cross_ref, cross_prb, max_nodes=0)  # refinement alone cannot separate them: the budget path, no fault
    assert plain.verdict.tolist() == [2] * len(cross_prb) and (plain.nodes == 0).all() and (plain.map == -1).all()
    one = _run(gpu_device, cross_ref, cross_prb, max_nodes=1)    # a budget is a cap: never more nodes than allowed, never a wrong answer
    assert (one.nodes <= 1).all() and set(one.verdict.tolist()) <= {0, 2}
    # every molecule against a permuted copy of itself; the deepest stacks; a saturated C9H20
    own = [m for _, a, b in hard for m in (a, b)] + [GM.k29(), GM.carbons(29, []), GM.nonane()]
    moved = [GM.permuted(m, rng) for m in own]
    got = _run(gpu_device, own, moved)
    print(f"[graph] self pairs: nodes {got.nodes.tolist()}")
    assert got.verdict.tolist() == [1] * len(own)
    _check_maps(got, own, moved, "self")
    assert got.nodes[-3] >= 1 and got.nodes[-2] >= 1                  # K29 and the bondless molecule cannot be decided without the search
    tight = _run(gpu_device, own[-3:], moved[-3:], max_nodes=int(got.nodes[-3:].max()))
    assert tight.verdict.tolist() == [1, 1, 1]                        # exactly the nodes a search used are enough for it
    short = _run(gpu_device, own[-3:-1], moved[-3:-1], max_nodes=int(got.nodes[-3:-1].min()) - 1)
    assert short.verdict.tolist() == [2, 2] and (short.map == -1).all()


def test_edges_of_the_shape(gpu_device):
    rng = np.random.default_rng(9)
    ref, prb, _ = GM.seeded_pairs()
    big = next(m for m in ref if len(m["type"]) == 29)
    empty = GM.molecule([], [])
    one_c, one_n = GM.molecule([1], []), GM.molecule([2], [])
    two = GM.molecule([1, 3], [(0, 1)], orders=[2])
    two_single, two_apart = GM.molecule([1, 3], [(0, 1)]), GM.molecule([3, 1], [])
    less = dict(pos=big["pos"][:28], type=big["type"][:28], fc=big["fc"][:28], bond=big["bond"][:28, :28])
    charged = dict(big, fc=big["fc"].copy())
    charged["fc"][11] = (charged["fc"][11] + 2) % 3 - 1               # one formal charge differs
    i, j = np.argwhere(np.triu(big["bond"]) > 0)[0]
    loud = dict(big, bond=big["bond"].copy())
    loud["bond"][i, j] = loud["bond"][j, i] = 255                      # a bond byte of 255 is a label like any other
    cases = [(empty, empty, 1), (one_c, one_c, 1), (one_c, one_n, 0), (empty, one_c, 0),
             (GM.permuted(two, rng), two, 1), (two_single, two, 0), (two_apart, two, 0),
             (big, less, 0), (less, big, 0), (GM.permuted(charged, rng), big, 0), (GM.permuted(charged, rng), charged, 1),
             (GM.permuted(loud, rng), loud, 1), (GM.permuted(loud, rng), big, 0), (GM.permuted(big, rng), loud, 0)]
    prb_m, ref_m, want = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    assert [int(GM.same_graph(a, b)) for a, b in zip(prb_m, ref_m)] == want
    got = _run(gpu_device, ref_m, prb_m)
    assert got.verdict.tolist() == want
    _check_maps(got, ref_m, prb_m, "edge")
    assert got.nodes[0] == 0 and (got.map[0] == -1).all() and got.map[1].tolist() == [0] + [-1] * 28
    # n is clamped to 0..29, as in ds_match_records: a count of 40 reads 29 atoms, a negative one none
    (rr, rn), (pr, pn) = SM.records([big, empty]), SM.records([GM.permuted(big, rng), empty])
    clamped = _run(gpu_device, (rr, np.array([40, -3], np.int32)), (pr, np.array([29, 0], np.int32)))
    assert clamped.verdict.tolist() == [1, 1]
    # the lower triangle and the diagonal of a record's bond matrix are not read
    noisy = pr.copy()
    m = noisy[0, 406:406 + 841].reshape(29, 29)
    m[np.tril_indices(29)] = 77
    assert _run(gpu_device, (rr, rn), (noisy, pn)).verdict.tolist() == [1, 1]
    # ref_index: several candidates share a ground-truth row; a row outside the table is verdict 3 and nothing else changes
    S, K = 20, 4
    rows = np.repeat(np.arange(S), K)
    cand = [prb[s] if k == 0 else (GM.permuted(ref[s], rng) if k == 2 else prb[(s + 7 * k) % 100]) for s in range(S) for k in range(K)]
    want = np.array([int(GM.same_graph(c, ref[r])) for c, r in zip(cand, rows)], np.uint8)
    (rr, rn), (pr, pn) = SM.records(ref[:S]), SM.records(cand)
    got = _run(gpu_device, (rr, rn), (pr, pn), ref_index=rows)
    assert np.array_equal(got.verdict, want) and want.reshape(S, K)[:, 2].all()
    _check_maps(got, [ref[r] for r in rows], cand, "ref_index")
    bad_rows = rows.copy()
    bad_rows[[3, 50]] = [S, -1]
    bad = _run(gpu_device, (rr, rn), (pr, pn), ref_index=bad_rows)
    assert bad.verdict[[3, 50]].tolist() == [3, 3] and (bad.map[[3, 50]] == -1).all() and (bad.nodes[[3, 50]] == 0).all()
    keep = np.ones(S * K, bool)
    keep[[3, 50]] = False
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(bad, got))
    top = topk_identity(torch.as_tensor(got.verdict), K)
    assert top["hit"].tolist() == want.reshape(S, K).any(1).tolist() and int(top["undecided"]) == 0
    # P = 0
    none = _run(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert none.verdict.shape == (0,) and none.nodes.shape == (0,) and none.map.shape == (0, SM.W)
    assert _run(gpu_device, (rr[:0], rn[:0]), (pr[:0], pn[:0])).verdict.shape == (0,)
    assert E.graph_hash_records(to_dev(gpu_device, pr[:0], torch.uint8), to_dev(gpu_device, pn[:0], torch.int32)).shape == (0,)


@pytest.fixture(scope="module")
def synthetic():
    return SM.synthetic_pairs(3000, 20261017)


def test_conformation_independence(gpu_device, synthetic):
    """The point of the feature: the ground truth under another atom order with unrelated coordinates is not certified by the geometric match
    of ds_match_records, and is by ds_graph_identity_records."""
    ref_rec, ref_n, prb_rec, prb_n = synthetic
    rng = np.random.default_rng(10)
    count = 200
    truth = [SM.mol_from_record(ref_rec[p], ref_n[p]) for p in range(count)]
    moved = [GM.permuted(m, rng) for m in truth]
    pr, pn = SM.records(moved)
    dev = lambda a, dt: to_dev(gpu_device, a, dt)
    exact = E.match_records(dev(pr, torch.uint8), dev(pn, torch.int32), dev(ref_rec[:count], torch.uint8), dev(ref_n[:count], torch.int32))[4].cpu().numpy()
    got = _run(gpu_device, (ref_rec[:count], ref_n[:count]), (pr, pn))
    print(f"[graph] {count} re-embedded ground truths: ds_match_records certifies {int(exact.sum())}, ds_graph_identity_records {int((got.verdict == 1).sum())}")
    assert (exact == 0).any() and (got.verdict == 1).all()
    _check_maps(got, truth, moved, "re-embedded")
    # whatever the geometric match certifies on the unmodified pairs is identical here too
    exact = E.match_records(dev(prb_rec, torch.uint8), dev(prb_n, torch.int32), dev(ref_rec, torch.uint8), dev(ref_n, torch.int32))[4].cpu().numpy()
    got = _run(gpu_device, (ref_rec, ref_n), (prb_rec, prb_n))
    assert exact.sum() > 0 and (got.verdict[exact == 1] == 1).all() and (got.verdict <= 1).all()
    batch = graph_identity_batch((dev(ref_rec, torch.uint8), dev(ref_n, torch.int32)), (dev(prb_rec, torch.uint8), torch.as_tensor(prb_n)))
    assert np.array_equal(batch.verdict.cpu().numpy(), got.verdict) and np.array_equal(batch.identical.cpu().numpy(), got.verdict == 1)


def test_batch_independence(gpu_device):
    """A pair's verdict, nodes and map are bit-identical alone, first, last and in the middle of 10 000."""
    ref, prb, _ = GM.seeded_pairs()
    hard = GM.hard_pairs()
    probes = [(prb[5], ref[5]), (prb[1001], ref[1001]), (hard[7][1], hard[7][2]), (GM.permuted(GM.k29(), np.random.default_rng(11)), GM.k29())]
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    rep = np.arange(10000) % 2000
    R, N, Pr, Pn = rr[rep], rn[rep], pr[rep], pn[rep]
    places = [0, 4321, 9999]
    for a, b in probes:
        (r1, n1), (p1, m1) = SM.records([b]), SM.records([a])
        alone = _run(gpu_device, (r1, n1), (p1, m1))
        R[places], N[places], Pr[places], Pn[places] = r1[0], n1[0], p1[0], m1[0]
        full = _run(gpu_device, (R, N), (Pr, Pn))
        for x, y in zip(alone, full):
            for where in places:
                assert x[0].tobytes() == y[where].tobytes(), where
    assert len({int(_run(gpu_device, SM.records([b]), SM.records([a])).verdict[0]) for a, b in probes}) == 2     # both answers were probed


def test_hash_and_classes(gpu_device):
    rng = np.random.default_rng(12)
    ref, prb, _ = GM.seeded_pairs()
    mols = list(ref[:260])
    planted = [int(k) for k in rng.integers(0, 260, size=40)]
    mols += [GM.permuted(mols[k], rng) for k in planted]             # permuted duplicates ...
    for _, a, b in GM.hard_pairs():                                   # ... and graphs that collide in the hash without being equal
        mols += [a, GM.permuted(b, rng), GM.permuted(a, rng)]
    mols += [GM.molecule([], []), GM.molecule([], []), GM.k29(), GM.permuted(GM.k29(), rng)]
    order = rng.permutation(len(mols))
    mols = [mols[k] for k in order]
    rec, n = SM.records(mols)
    got = E.graph_hash_records(to_dev(gpu_device, rec, torch.uint8), to_dev(gpu_device, n, torch.int32))
    assert got.dtype == torch.int64 and got.shape == (len(mols),)
    got = [int(v) & GM.MASK for v in got.cpu().tolist()]
    want = [GM.graph_hash(m) for m in mols]
    assert got == want                                                # bit-equal to the restated formula, hence equal on permuted copies
    # the partition, by the mirror alone: every row against the earlier class representatives
    reps, want_class = [], []
    for k, m in enumerate(mols):
        found = next((r for r in reps if GM.same_graph(m, mols[r])), None)
        if found is None:
            reps.append(k)
        want_class.append(k if found is None else found)
    buckets = {}
    for k, h in enumerate(want):
        buckets.setdefault(h, set()).add(want_class[k])
    assert max(len(v) for v in buckets.values()) >= 2                 # buckets with several classes do occur
    classes = graph_classes(to_dev(gpu_device, rec, torch.uint8), torch.as_tensor(n))
    assert classes.dtype == torch.int64 and classes.tolist() == want_class
    assert classes.unique().numel() == len(reps) < len(mols)
    assert graph_classes(to_dev(gpu_device, rec[:0], torch.uint8), torch.as_tensor(n[:0])).shape == (0,)


def test_evaluate_reports_graph_identity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 3: one slot's record is replaced by its ground truth
    under another atom order with unrelated coordinates; metrics['structure']['graph'] certifies it, its Top-K hits are the mirror's, and
    everything the structure metric reported before is still there."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K, S = 3, 5
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=S)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:S].repeat_interleave(K)
    planted = 1 * K + 1
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    truth = SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])])
    moved = GM.permuted(truth, np.random.default_rng(13))
    assert not np.array_equal(moved["type"], truth["type"]) or not np.array_equal(moved["bond"], truth["bond"])
    gather = shard.gather_by_slot

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    mols, st = res[40]["processed_mols"], res[40]["metrics"]["structure"]
    for key in ("rmsd_list", "success_rate", "mean_rmsd", "mean_atom_type_accuracy", "mean_bond_accuracy", "exact_rate", "per_pair", "top_k"):
        assert key in st, key
    assert set(st["top_k"]) == {"best_rmsd", "best_index", "hit", "hit_at_k"}
    graph = st["graph"]
    assert set(graph) == {"verdict", "identity_rate", "undecided", "unique_fraction", "top_k"}
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in mols]
    want = np.array([GM.same_graph(m, SM.mol_from_record(gt_rec[int(j)], gt_n[int(j)])) for m, j in zip(made, slot_ds)])
    assert GM.same_graph(made[planted], truth) and want[planted]
    verdict = graph["verdict"].cpu().numpy()
    assert verdict.dtype == np.uint8 and np.array_equal(verdict, want.astype(np.uint8)) and verdict[planted] == 1
    assert graph["undecided"] == 0 and graph["identity_rate"] == want.mean()
    top = {k: v.cpu() for k, v in graph["top_k"].items()}
    assert top["hit"].tolist() == want.reshape(S, K).any(1).tolist() and bool(top["hit"][1]) and int(top["undecided"]) == 0
    assert float(top["acc_at_k"]) == want.reshape(S, K).any(1).mean()
    assert top["first_hit"].tolist() == [int(np.argmax(g)) if g.any() else -1 for g in want.reshape(S, K)]
    reps = []
    for k, m in enumerate(made):
        if not any(GM.same_graph(m, made[r]) for r in reps):
            reps.append(k)
    assert graph["unique_fraction"] == len(reps) / len(made)
    # the default call returns what it returned before: no structure entry
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table)
    assert "structure" not in plain[40]["metrics"] and len(plain[40]["processed_mols"]) == S
