"""GPU: ``ds_morgan_records`` and ``ds_morgan_similarity_records`` (one wave per molecule / per pair) against the plain-Python definition of
tests/morgan_mirror.py - every feature and every count equal, no tolerance anywhere - plus the full width, the edges of the shape, batch and
atom-order independence and the evaluation driver end to end."""
import functools

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from diffspectra_amd.structure_metrics import MorganSimilarity, morgan_fingerprints, morgan_similarity_batch, topk_morgan
from tests import graph_mirror as GM, mces_mirror as MM, morgan_mirror as FM, structure_mirror as SM
from tests.helpers import run_records, to_dev

pytestmark = pytest.mark.gpu

_pairs = functools.partial(run_records, E.morgan_similarity_records, MorganSimilarity)      # (dev, ref, prb, ref_index=None, **scalars)
LARGE = dict(count=40, seed=20261102, heavy=(10, 12))
WIDTH = E.MORGAN_MAX_FEATURES


def _features(dev, mols, drop_h=True, radius=2):
    """``ds_morgan_records`` on molecule dicts or on a ``(records, n)`` pair -> (ids [P, 116] uint64, count [P])."""
    rec, n = SM.records(mols) if isinstance(mols, list) else mols
    ids, count = E.morgan_records(to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32), drop_h, radius)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and count.dtype == torch.int32 and ids.shape == (len(n), WIDTH) and count.shape == (len(n),)
    return ids.cpu().numpy().view(np.uint64), count.cpu().numpy()


@functools.lru_cache(maxsize=16)
def _mirror_sets(drop_h, radius, large=False):
    """The mirror's fingerprint of every molecule of the seeded set, generated molecules first, computed once per process."""
    ref, prb, _ = MM.seeded_pairs(**LARGE) if large else MM.seeded_pairs()
    return [FM.fingerprint(m, drop_h, radius) for m in prb + ref]


def _mirror_counts(drop_h, radius, n_bits, large=False):
    sets = _mirror_sets(drop_h, radius, large)
    half = len(sets) // 2
    out = []
    for a, b in zip(sets[:half], sets[half:]):
        fa, fb = FM.fold(a, n_bits), FM.fold(b, n_bits)
        out.append((len(fa & fb), len(fa), len(fb)))
    return np.array(out, np.int64)


def _check_features(ids, count, sets, what):
    assert len(sets) == len(count)
    for p, want in enumerate(sets):
        assert count[p] == len(want), f"{what} molecule {p}: {count[p]} features, the mirror has {len(want)}"
        assert ids[p, :count[p]].tolist() == sorted(want), f"{what} molecule {p}"
    assert all(not ids[p, count[p]:].any() for p in range(len(sets))), f"{what}: padding"


def _triple(got):
    return np.stack([got.common, got.n_prb, got.n_ref], 1).astype(np.int64)


def _tanimoto(counts):
    return np.array([FM.tanimoto(*row) for row in counts.tolist()])


@pytest.mark.parametrize("drop_h,radius", [(True, 0), (True, 1), (True, 2), (True, 3), (False, 2)])
def test_feature_parity(gpu_device, drop_h, radius):
    ref, prb, _ = MM.seeded_pairs()
    mols = prb + ref
    assert len(mols) == 1200 and max(int((m["type"] != 0).sum()) for m in mols) <= 9 and max(len(m["type"]) for m in mols) <= 23
    ids, count = _features(gpu_device, mols, drop_h, radius)
    sets = _mirror_sets(drop_h, radius)
    print(f"[morgan] 1200 molecules, drop_h = {int(drop_h)}, R = {radius}: features mean {count.mean():.2f} max {count.max()}; "
          f"count disagreements {int((count != [len(s) for s in sets]).sum())}")
    _check_features(ids, count, sets, f"drop_h {drop_h} R {radius}")


def test_pair_parity(gpu_device):
    ref, prb, kind = MM.seeded_pairs()
    assert len(ref) == 600
    got = {}
    for n_bits in (0, 64, 2048):
        out = _pairs(gpu_device, ref, prb, drop_h=True, radius=2, n_bits=n_bits)
        want = _mirror_counts(True, 2, n_bits)
        differ = np.nonzero((_triple(out) != want).any(1))[0]
        print(f"[morgan] 600 pairs, n_bits = {n_bits}: disagreements {len(differ)}")
        assert out.common.dtype == out.n_prb.dtype == out.n_ref.dtype == np.int32 and out.status.dtype == np.uint8
        assert (out.status == 0).all() and len(differ) == 0, differ[:10]
        got[n_bits] = want
    # the set shows something
    unfolded = got[0]
    tan = _tanimoto(unfolded)
    layer1 = _mirror_counts(True, 1, 0)
    print(f"[morgan] Tanimoto < 1: {int((tan < 1).sum())}; kind 0 not 1: {int((tan[kind == 0] != 1).sum())}; 64 bits change "
          f"{int((got[64] != unfolded).any(1).sum())}; R = 1 differs from R = 2 on {int((layer1 != unfolded).any(1).sum())}")
    assert (tan < 1).sum() > 300 and (tan[kind == 0] == 1).all()
    assert (got[64] != unfolded).any(1).sum() > 100 and (layer1 != unfolded).any(1).sum() > 100
    one = _pairs(gpu_device, ref, prb, drop_h=True, radius=1, n_bits=0)
    assert np.array_equal(_triple(one), layer1)
    # the properties of the binding's result type, against the mirror's plain formulas
    dev = lambda a, dt: to_dev(gpu_device, a, dt)
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    batch = morgan_similarity_batch((dev(rr, torch.uint8), torch.as_tensor(rn)), (dev(pr, torch.uint8), torch.as_tensor(pn)))
    folded = got[2048]
    assert np.array_equal(_triple(MorganSimilarity(*(t.cpu().numpy() for t in batch))), folded) and bool(batch.valid.all())
    assert batch.tanimoto.cpu().tolist() == _tanimoto(folded).tolist()
    assert batch.cosine.cpu().tolist() == [FM.cosine(*row) for row in folded.tolist()]


def test_full_width(gpu_device):
    ref, prb, _ = MM.seeded_pairs(**LARGE)
    assert max(len(m["type"]) for m in ref + prb) == SM.W                  # a molecule on every lane of a half
    sets = _mirror_sets(False, 3, True)
    ids, count = _features(gpu_device, prb + ref, False, 3)
    print(f"[morgan] 80 molecules of 10-12 heavy atoms, hydrogens kept, R = 3: features mean {count.mean():.1f} max {count.max()}")
    _check_features(ids, count, sets, "full width")
    for n_bits in (0, 2048, 4096):
        out = _pairs(gpu_device, ref, prb, drop_h=False, radius=3, n_bits=n_bits)
        assert np.array_equal(_triple(out), _mirror_counts(False, 3, n_bits, True)) and (out.status == 0).all()


def test_edges_of_the_shape(gpu_device):
    rng = np.random.default_rng(41)
    ref, prb, _ = MM.seeded_pairs()
    empty, carbon, h2 = GM.molecule([], []), GM.molecule([1], []), GM.molecule([0, 0], [(0, 1)])
    ethanol = GM.saturated(GM.molecule([1, 1, 3], [(0, 1), (1, 2)]))
    charged = GM.molecule([2, 1, 3], [(0, 1), (1, 2)], fc=[1, 0, -1])
    cases = [(empty, empty), (empty, ethanol), (ethanol, empty), (carbon, carbon), (carbon, ethanol), (h2, h2), (h2, ethanol), (charged, ethanol),
             (charged, charged)]
    prb_m, ref_m = [c[0] for c in cases], [c[1] for c in cases]
    for drop_h in (True, False):
        for n_bits in (0, 2048):
            got = _pairs(gpu_device, ref_m, prb_m, drop_h=drop_h, radius=2, n_bits=n_bits)
            want = [FM.similarity_counts(a, b, drop_h, 2, n_bits) for a, b in cases]
            assert _triple(got).tolist() == [list(w) for w in want] and (got.status == 0).all(), (drop_h, n_bits)
        ids, count = _features(gpu_device, prb_m, drop_h, 2)
        _check_features(ids, count, [FM.fingerprint(m, drop_h, 2) for m in prb_m], f"edge, drop_h {drop_h}")
        if drop_h:
            assert _triple(got)[0].tolist() == [0, 0, 0] and _triple(got)[5].tolist() == [0, 0, 0] and count[5] == 0      # H2 is the empty set
            assert _triple(got)[1].tolist() == [0, 0, len(FM.fold(FM.fingerprint(ethanol), 2048))] and count[3] == 1
    # the hand table
    names = list(FM.HAND_COUNTS)
    for radius in range(4):
        ids, count = _features(gpu_device, [FM.MOLECULES[k] for k in names], True, radius)
        assert count.tolist() == [FM.HAND_COUNTS[k][radius] for k in names]
    hand = _pairs(gpu_device, [FM.MOLECULES[b] for _, b, _ in FM.HAND_PAIRS], [FM.MOLECULES[a] for a, _, _ in FM.HAND_PAIRS], radius=2, n_bits=0)
    assert _triple(hand).tolist() == [list(w) for *_, w in FM.HAND_PAIRS]
    # n is clamped to 0..29, the atoms beyond n are not read, and neither is the lower triangle of the bond matrix
    big = max(range(600), key=lambda p: len(ref[p]["type"]))
    (rr, rn), (pr, pn) = SM.records([ref[big], empty, ref[big]]), SM.records([prb[big], empty, prb[big]])
    noisy = pr.copy()
    noisy[0, SM.BOND:SM.BOND_END].reshape(SM.W, SM.W)[np.tril_indices(SM.W)] = 77
    cut = len(prb[big]["type"]) - 3                                       # the third pair: its generated molecule without its last atoms
    noisy[2, SM.TYPE + cut:SM.TYPE + SM.W] = 1
    want = [FM.similarity_counts(prb[big], ref[big]), (0, 0, 0), FM.similarity_counts(SM.mol_from_record(noisy[2], cut), ref[big])]
    got = _pairs(gpu_device, (rr, np.array([40, -3, rn[2]], np.int32)), (noisy, np.array([pn[0], -7, cut], np.int32)))
    assert _triple(got).tolist() == [list(w) for w in want] and (got.status == 0).all()
    # a dense record: 29 atoms, every bond byte 255, garbage in the lower triangle
    dense_rec, dense_n, dense = FM.dense_record()
    for radius, size in enumerate((1, 2, 3, 3)):
        ids, count = _features(gpu_device, (dense_rec, np.array([64], np.int32)), True, radius)
        assert count.tolist() == [size]
        _check_features(ids, count, [FM.fingerprint(dense, True, radius)], f"dense R {radius}")
    got = _pairs(gpu_device, (dense_rec, dense_n), (dense_rec, dense_n), drop_h=False, radius=3, n_bits=64)
    assert _triple(got).tolist() == [list(FM.similarity_counts(dense, dense, False, 3, 64))] and got.common[0] == got.n_prb[0] == got.n_ref[0] > 0
    # ref_index: K candidates share one ground-truth row; a row outside the table is invalid and nothing else changes
    S, K = 20, 4
    rows = np.repeat(np.arange(S), K)
    cand = [prb[s] if k == 0 else (GM.permuted(ref[s], rng) if k == 2 else prb[(s + 7 * k) % 100]) for s in range(S) for k in range(K)]
    wanted = np.array([FM.similarity_counts(c, ref[r]) for c, r in zip(cand, rows)])
    (rr, rn), (pr, pn) = SM.records(ref[:S]), SM.records(cand)
    got = _pairs(gpu_device, (rr, rn), (pr, pn), ref_index=rows)
    assert np.array_equal(_triple(got), wanted) and (got.status == 0).all()
    tan = MorganSimilarity(*(torch.as_tensor(x) for x in got)).tanimoto
    assert (tan.reshape(S, K)[:, 2] == 1).all()
    top = topk_morgan(tan, K)
    assert top["best"].tolist() == [1.0] * S and float(top["mean_best"]) == 1.0
    bad_rows = rows.copy()
    bad_rows[[3, 50]] = [S, -1]
    bad = _pairs(gpu_device, (rr, rn), (pr, pn), ref_index=bad_rows)
    assert bad.status[[3, 50]].tolist() == [3, 3] and (_triple(bad)[[3, 50]] == -1).all()
    keep = np.ones(S * K, bool)
    keep[[3, 50]] = False
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(bad, got))
    sim = MorganSimilarity(*(torch.as_tensor(x) for x in bad))
    assert torch.isnan(sim.tanimoto[[3, 50]]).all() and torch.isnan(sim.cosine[[3, 50]]).all() and int(sim.valid.sum()) == S * K - 2
    # M = 0 with a ref_index: every pair is invalid and nothing is read
    none = _pairs(gpu_device, (rr[:0], rn[:0]), (pr[:3], pn[:3]), ref_index=np.zeros(3, np.int64))
    assert none.status.tolist() == [3, 3, 3] and (_triple(none) == -1).all()
    # P = 0
    none = _pairs(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert none.common.shape == (0,) and none.n_prb.shape == (0,) and none.n_ref.shape == (0,) and none.status.shape == (0,)
    ids, count = _features(gpu_device, (pr[:0], pn[:0]))
    assert ids.shape == (0, WIDTH) and count.shape == (0,)


def test_independence(gpu_device):
    """A pair alone gives what it gives inside the batch; renamed atoms give identical ids."""
    ref, prb, _ = MM.seeded_pairs()
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    full = _pairs(gpu_device, (rr, rn), (pr, pn))
    ids_full, count_full = _features(gpu_device, (pr, pn))
    for p in (0, 299, 599, int(np.argmax(pn))):
        alone = _pairs(gpu_device, (rr[p:p + 1], rn[p:p + 1]), (pr[p:p + 1], pn[p:p + 1]))
        for x, y in zip(alone, full):
            assert x[0].tobytes() == y[p].tobytes(), p
        ids, count = _features(gpu_device, (pr[p:p + 1], pn[p:p + 1]))
        assert ids[0].tobytes() == ids_full[p].tobytes() and count[0] == count_full[p]
    rng = np.random.default_rng(20261105)
    for drop_h, radius in ((True, 2), (False, 3)):
        ids, count = _features(gpu_device, prb[:100], drop_h, radius)
        moved, count_moved = _features(gpu_device, [GM.permuted(m, rng) for m in prb[:100]], drop_h, radius)
        assert np.array_equal(ids, moved) and np.array_equal(count, count_moved)
    # the folded bit vectors are the mirror's folded sets
    bits = morgan_fingerprints(to_dev(gpu_device, pr, torch.uint8), pn, n_bits=2048)
    assert bits.dtype == torch.bool and bits.shape == (600, 2048)
    sets = _mirror_sets(True, 2)[:600]
    bits = bits.cpu().numpy()
    assert all(set(np.nonzero(bits[p])[0].tolist()) == FM.fold(sets[p], 2048) for p in range(600))
    ids2, count2 = morgan_fingerprints(to_dev(gpu_device, pr, torch.uint8), pn)
    assert np.array_equal(ids2.cpu().numpy().view(np.uint64), ids_full) and np.array_equal(count2.cpu().numpy(), count_full)


def test_evaluate_reports_fingerprint_similarity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 3: one slot's record is replaced by its ground truth under
    another atom order; metrics['structure']['fingerprint'] is the mirror's on the run's records, Tanimoto 1 wherever the graph verdict is 1."""
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
    for key in ("rmsd_list", "success_rate", "mean_rmsd", "mean_atom_type_accuracy", "mean_bond_accuracy", "exact_rate", "per_pair", "top_k", "graph", "mces"):
        assert key in st, key
    fp = st["fingerprint"]
    assert set(fp) == {"tanimoto", "cosine", "status", "mean_tanimoto", "mean_cosine", "top_k"}
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in mols]
    truths = [SM.mol_from_record(gt_rec[int(j)], gt_n[int(j)]) for j in slot_ds]
    counts = [FM.similarity_counts(m, t, True, 2, 2048) for m, t in zip(made, truths)]
    want_t, want_c = np.array([FM.tanimoto(*c) for c in counts]), np.array([FM.cosine(*c) for c in counts])
    tan, cos, status = fp["tanimoto"].cpu().numpy(), fp["cosine"].cpu().numpy(), fp["status"].cpu().numpy()
    assert tan.dtype == np.float64 and cos.dtype == np.float64 and status.dtype == np.uint8 and (status == 0).all()
    assert np.array_equal(tan, want_t) and np.array_equal(cos, want_c) and tan[planted] == 1.0 and cos[planted] == 1.0
    assert fp["mean_tanimoto"] == float(torch.as_tensor(want_t).mean()) and fp["mean_cosine"] == float(torch.as_tensor(want_c).mean())
    top = {k: v.cpu() for k, v in fp["top_k"].items()}
    again = topk_morgan(torch.as_tensor(want_t), K)
    assert set(top) == set(again) == {"best", "best_index", "mean_best"}
    assert top["best"].tolist() == again["best"].tolist() == want_t.reshape(S, K).max(1).tolist() and float(top["best"][1]) == 1.0
    assert top["best_index"].tolist() == again["best_index"].tolist() == want_t.reshape(S, K).argmax(1).tolist()
    assert float(top["mean_best"]) == float(again["mean_best"])
    # every slot whose graph verdict is 1 has Tanimoto 1; the other entries are what they were
    verdict = st["graph"]["verdict"].cpu().numpy()
    assert verdict[planted] == 1 and (tan[verdict == 1] == 1.0).all() and (cos[verdict == 1] == 1.0).all()
    assert set(st["graph"]) == {"verdict", "identity_rate", "undecided", "unique_fraction", "top_k"}
    assert set(st["mces"]) == {"dist", "status", "mean", "zero_rate", "undecided", "top_k"}
