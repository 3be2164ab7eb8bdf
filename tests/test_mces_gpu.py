"""GPU: ``ds_mces_records`` (one wave per pair, branch-and-bound) against the integer program of tests/mces_mirror.py - every distance
equal, every returned map rescored here from the records, no tolerance anywhere - plus the budget, the edges of the shape, batch
independence, the agreement with ``ds_graph_identity_records`` and the evaluation driver end to end."""
import functools

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from diffspectra_amd.structure_metrics import Mces, mces_batch, topk_mces
from tests import graph_mirror as GM, mces_mirror as MM, structure_mirror as SM
from tests.helpers import run_records, to_dev

pytestmark = pytest.mark.gpu

_run = functools.partial(run_records, E.mces_records, Mces)       # (dev, ref, prb, ref_index=None, **scalars) -> Mces of numpy arrays

DEFAULT_NODES = 1 << 18
LARGE = dict(count=40, seed=20261102, heavy=(10, 12))


def _check_maps(got, ref, prb, drop_h=True, what=""):
    """The map is rescored here from the molecules: injective, type-preserving, nothing dropped mapped, and W_A + W_B - 2 score(map) = dist."""
    assert got.map.shape == (len(prb), SM.W)
    for p, (a, b) in enumerate(zip(prb, ref)):
        score = MM.score_of_map(a, b, got.map[p], drop_h)
        assert MM.total_weight(a, drop_h) + MM.total_weight(b, drop_h) - 2 * score == got.dist[p], f"{what} pair {p}: the map does not achieve dist"


@pytest.fixture(scope="module")
def seeded():
    ref, prb, kind = MM.seeded_pairs()
    return ref, prb, kind, MM.seeded_distances()


def test_parity_on_seeded_pairs(gpu_device, seeded):
    ref, prb, kind, want = seeded
    assert len(ref) == 600 and max(int((m["type"] != 0).sum()) for m in ref + prb) <= 9 and (want[kind == 0] == 0).all()
    assert (want > 0).sum() > 300                                       # the set discriminates
    got = _run(gpu_device, ref, prb)
    print(f"[mces] 600 pairs, drop_h = 1: dist mean {want.mean():.3f}; nodes mean {got.nodes.mean():.2f} max {got.nodes.max()}; "
          f"disagreements {int((got.dist != want).sum())}, undecided {int((got.status == 2).sum())}")
    assert (got.status == 0).all(), np.nonzero(got.status != 0)[0][:10]
    assert np.array_equal(got.dist, want), np.nonzero(got.dist != want)[0][:10]
    assert np.array_equal(got.lower, got.dist) and (got.nodes >= 0).all() and (got.nodes <= DEFAULT_NODES).all()
    _check_maps(got, ref, prb, True, "seeded")
    # with the hydrogens kept: 100 of the pairs, at most 12 atoms a side so that the hydrogens do not blow up the search
    few = [p for p in range(600) if len(ref[p]["type"]) <= 12 and len(prb[p]["type"]) <= 12][:100]
    assert len(few) == 100
    ref_h, prb_h = [ref[p] for p in few], [prb[p] for p in few]
    want_h = np.array([MM.mces_milp(a, b, False) for a, b in zip(prb_h, ref_h)])
    got_h = _run(gpu_device, ref_h, prb_h, drop_h=False)
    print(f"[mces] 100 pairs, drop_h = 0: nodes mean {got_h.nodes.mean():.2f} max {got_h.nodes.max()}")
    assert (got_h.status == 0).all() and np.array_equal(got_h.dist, want_h) and (want_h != want[few]).any()
    _check_maps(got_h, ref_h, prb_h, False, "with hydrogens")


def test_larger_molecules(gpu_device):
    ref, prb, _ = MM.seeded_pairs(**LARGE)
    want = MM.seeded_distances(**LARGE)
    heavy = [int((m["type"] != 0).sum()) for m in ref]
    assert min(heavy) >= 10 and max(heavy) <= 12
    got = _run(gpu_device, ref, prb, max_nodes=E.MCES_MAX_NODES)
    print(f"[mces] 40 pairs of 10-12 heavy atoms: nodes mean {got.nodes.mean():.1f} max {got.nodes.max()}")
    assert (got.status == 0).all() and np.array_equal(got.dist, want), np.nonzero(got.dist != want)[0][:10]
    _check_maps(got, ref, prb, True, "large")


@pytest.mark.parametrize("budget", [0, 64])
def test_budget(gpu_device, seeded, budget):
    ref, prb, _, want = seeded
    got = _run(gpu_device, ref, prb, max_nodes=budget)
    undecided = got.status == 2
    print(f"[mces] budget {budget}: {int(undecided.sum())} of 600 undecided")
    assert set(got.status.tolist()) <= {0, 2}
    assert (got.lower <= want).all() and (want <= got.dist).all()
    assert np.array_equal(got.status == 0, got.lower == got.dist) and np.array_equal(got.dist[~undecided], want[~undecided])
    assert (got.nodes <= budget).all() and (got.nodes >= 0).all()
    assert undecided.any()                                              # otherwise this test shows nothing
    _check_maps(got, ref, prb, True, f"budget {budget}")                # dist is what the returned map achieves, decided or not


def test_edges_of_the_shape(gpu_device, seeded):
    rng = np.random.default_rng(31)
    ref, prb, _, want = seeded
    table = MM.hand_table()
    for drop_h in (True, False):
        got = _run(gpu_device, [b for _, a, b, _ in table], [a for _, a, b, _ in table], drop_h=drop_h)
        assert got.dist.tolist() == [d for *_, d in table] and (got.status == 0).all(), [(row[0], int(d)) for row, d in zip(table, got.dist) if d != row[3]]
        back = _run(gpu_device, [a for _, a, b, _ in table], [b for _, a, b, _ in table], drop_h=drop_h)
        assert back.dist.tolist() == got.dist.tolist()
        _check_maps(got, [b for _, a, b, _ in table], [a for _, a, b, _ in table], drop_h, "hand")
    empty = GM.molecule([], [])
    ethanol = GM.saturated(GM.molecule([1, 1, 3], [(0, 1), (1, 2)]))       # (valence 4 on the oxygen too: a graph like any other)
    h4 = GM.molecule([0, 0, 0, 0], [(0, 1), (2, 3)])
    bondless, bondless_b = GM.molecule([1, 2, 3, 1], []), GM.molecule([3, 1], [])
    cases = [(empty, empty), (empty, ethanol), (ethanol, empty), (h4, h4), (h4, ethanol), (bondless, bondless_b), (bondless, ethanol), (ethanol, bondless)]
    prb_m, ref_m = [c[0] for c in cases], [c[1] for c in cases]
    for drop_h in (True, False):
        got = _run(gpu_device, ref_m, prb_m, drop_h=drop_h)
        assert got.dist.tolist() == [MM.mces_milp(a, b, drop_h) for a, b in cases] and (got.status == 0).all()
        _check_maps(got, ref_m, prb_m, drop_h, "edge")
        if drop_h:      # hydrogens only: both W are 0, dist 0, exact, nothing mapped
            assert got.dist[3] == 0 and got.nodes[3] == 0 and (got.map[3] == -1).all() and got.dist[0] == 0
            assert got.dist[1] == got.dist[2] == MM.total_weight(ethanol) == 2
    # n is clamped to 0..29 and the lower triangle of a record's bond matrix is not read
    big = max((p for p in range(600) if want[p] > 0), key=lambda p: len(ref[p]["type"]))      # (the atoms beyond its n are bondless hydrogens)
    (rr, rn), (pr, pn) = SM.records([ref[big], empty]), SM.records([prb[big], empty])
    noisy = pr.copy()
    noisy[0, 406:406 + 841].reshape(29, 29)[np.tril_indices(29)] = 77
    got = _run(gpu_device, (rr, np.array([40, -3], np.int32)), (noisy, pn))
    assert got.dist.tolist() == [want[big], 0] and (got.status == 0).all()
    # ref_index: K candidates share one ground-truth row; a row outside the table is invalid and nothing else changes
    S, K = 20, 4
    rows = np.repeat(np.arange(S), K)
    cand = [prb[s] if k == 0 else (GM.permuted(ref[s], rng) if k == 2 else prb[(s + 7 * k) % 100]) for s in range(S) for k in range(K)]
    wanted = np.array([MM.mces_milp(c, ref[r]) for c, r in zip(cand, rows)])
    (rr, rn), (pr, pn) = SM.records(ref[:S]), SM.records(cand)
    got = _run(gpu_device, (rr, rn), (pr, pn), ref_index=rows)
    assert np.array_equal(got.dist, wanted) and (got.status == 0).all() and (wanted.reshape(S, K)[:, 2] == 0).all()
    _check_maps(got, [ref[r] for r in rows], cand, True, "ref_index")
    top = topk_mces(torch.as_tensor(got.dist), torch.as_tensor(got.status), K)
    assert top["best"].tolist() == [0] * S and int(top["undecided"]) == 0
    bad_rows = rows.copy()
    bad_rows[[3, 50]] = [S, -1]
    bad = _run(gpu_device, (rr, rn), (pr, pn), ref_index=bad_rows)
    assert bad.status[[3, 50]].tolist() == [3, 3] and bad.dist[[3, 50]].tolist() == [-1, -1] and bad.lower[[3, 50]].tolist() == [-1, -1]
    assert (bad.map[[3, 50]] == -1).all() and (bad.nodes[[3, 50]] == 0).all()
    keep = np.ones(S * K, bool)
    keep[[3, 50]] = False
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(bad, got))
    # P = 0
    none = _run(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert none.dist.shape == (0,) and none.status.shape == (0,) and none.map.shape == (0, SM.W)
    # the deepest stack: K29 of one type against itself, hydrogens (there are none) kept - it ends, within its budget
    k29 = GM.k29()
    moved = GM.permuted(k29, rng)
    for budget in (16, 4096):
        got = _run(gpu_device, [k29, k29], [k29, moved], drop_h=False, max_nodes=budget)
        assert set(got.status.tolist()) <= {0, 2} and (got.nodes <= budget).all() and (got.lower == 0).all()
        assert np.array_equal(got.status == 0, got.dist == 0)
        _check_maps(got, [k29, k29], [k29, moved], False, "K29")
    assert (got.status == 0).all()                                      # 29 tries find an isomorphism, and the root bound certifies it


def test_batch_independence(gpu_device, seeded):
    """A pair's five outputs are bit-identical alone, first, last and in the middle of 10 000."""
    ref, prb, _, want = seeded
    at64 = _run(gpu_device, ref, prb, max_nodes=64)
    hard, easy = int(np.argmax(at64.nodes * (at64.status == 2))), int(np.argmax(want == 0))
    far = int(np.argmax(want))
    probes = [(hard, 64), (hard, DEFAULT_NODES), (easy, 64), (far, DEFAULT_NODES)]
    assert at64.status[hard] == 2
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    rep = np.arange(10000) % 600
    places = [0, 4321, 9999]
    for which, budget in probes:
        alone = _run(gpu_device, (rr[which:which + 1], rn[which:which + 1]), (pr[which:which + 1], pn[which:which + 1]), max_nodes=budget)
        R, N, Pr, Pn = rr[rep], rn[rep], pr[rep], pn[rep]
        R[places], N[places], Pr[places], Pn[places] = rr[which], rn[which], pr[which], pn[which]
        full = _run(gpu_device, (R, N), (Pr, Pn), max_nodes=budget)
        for x, y in zip(alone, full):
            for where in places:
                assert x[0].tobytes() == y[where].tobytes(), (which, budget, where)
        if budget == DEFAULT_NODES:
            assert np.array_equal(full.dist[600:1200], want)


def test_identical_graphs_are_zero_apart(gpu_device, seeded):
    """Cross-kernel: whatever ds_graph_identity_records calls identical (whole molecules, hydrogens included) is 0 apart on the heavy atoms."""
    ref, prb, _, want = seeded
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    dev = lambda a, dt: to_dev(gpu_device, a, dt)
    args = (dev(pr, torch.uint8), dev(pn, torch.int32), dev(rr, torch.uint8), dev(rn, torch.int32))
    verdict = E.graph_identity_records(*args)[0].cpu().numpy()
    same = verdict == 1
    assert same.sum() >= 100 and (verdict <= 1).all()
    heavy = _run(gpu_device, (rr, rn), (pr, pn))
    assert (heavy.dist[same] == 0).all() and (heavy.status == 0).all()
    # with the hydrogens kept the many equivalent hydrogens can exhaust a budget even on identical graphs: then the root bound still says 0
    whole = _run(gpu_device, (rr, rn), (pr, pn), drop_h=False, max_nodes=4096)
    assert (whole.lower[same] == 0).all() and (whole.dist[same & (whole.status == 0)] == 0).all() and (same & (whole.status == 0)).sum() >= 50
    batch = mces_batch((args[2], args[3]), (args[0], torch.as_tensor(pn)))
    assert np.array_equal(batch.dist.cpu().numpy(), heavy.dist) and np.array_equal(batch.exact.cpu().numpy(), heavy.status == 0)


def test_evaluate_reports_mces(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 3: one slot's record is replaced by its ground truth under
    another atom order; metrics['structure']['mces'] has dist 0 there, its mean and Top-K are the mirror's on the run's records, and
    metrics['structure']['graph'] is what it was."""
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
    gather = shard.gather_by_slot

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    mols, st = res[40]["processed_mols"], res[40]["metrics"]["structure"]
    for key in ("rmsd_list", "success_rate", "mean_rmsd", "mean_atom_type_accuracy", "mean_bond_accuracy", "exact_rate", "per_pair", "top_k", "graph"):
        assert key in st, key
    mces = st["mces"]
    assert set(mces) == {"dist", "status", "mean", "zero_rate", "undecided", "top_k"}
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in mols]
    truths = [SM.mol_from_record(gt_rec[int(j)], gt_n[int(j)]) for j in slot_ds]
    want = np.array([MM.mces_milp(m, t) for m, t in zip(made, truths)])
    dist, status = mces["dist"].cpu().numpy(), mces["status"].cpu().numpy()
    assert dist.dtype == np.int32 and status.dtype == np.uint8 and (status == 0).all() and mces["undecided"] == 0
    assert np.array_equal(dist, want) and dist[planted] == 0
    assert mces["mean"] == want.mean() and mces["zero_rate"] == (want == 0).mean()
    top = {k: v.cpu() for k, v in mces["top_k"].items()}
    assert set(top) == {"best", "best_index", "mean_best", "undecided"}
    assert top["best"].tolist() == want.reshape(S, K).min(1).tolist() and int(top["best"][1]) == 0 and int(top["undecided"]) == 0
    assert top["best_index"].tolist() == want.reshape(S, K).argmin(1).tolist() and float(top["mean_best"]) == want.reshape(S, K).min(1).mean()
    # the graph entry is what it was: same keys, the mirror's verdicts
    graph = st["graph"]
    assert set(graph) == {"verdict", "identity_rate", "undecided", "unique_fraction", "top_k"}
    same = np.array([GM.same_graph(m, t) for m, t in zip(made, truths)])
    assert np.array_equal(graph["verdict"].cpu().numpy(), same.astype(np.uint8)) and graph["identity_rate"] == same.mean() and graph["undecided"] == 0
    assert (dist[same] == 0).all()
