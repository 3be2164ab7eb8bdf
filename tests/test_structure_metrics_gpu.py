"""GPU: ``ds_match_records`` (one wave per pair, fp64) against the CPU mirror of tests/structure_mirror.py - assignment decisions exact, RMSD
within 1e-9 A - plus edge cases, batch independence and the evaluation driver end to end."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from diffspectra_amd.structure_metrics import PairMetrics, hungarian_rmsd_batch, topk_summary
from tests import structure_mirror as SM
from tests.helpers import run_records

pytestmark = pytest.mark.gpu

_run = functools.partial(run_records, E.match_records, PairMetrics)       # (dev, ref, prb, ref_index=None, **scalars) -> PairMetrics of numpy arrays

# fp64 sums of at most 29 terms of order 10 on both sides: ~1e-13 of rounding; the gate sits four orders above that and about six orders
# below the fp32 spacing of the input coordinates
RMSD_TOL = 1e-9


def _compare(got, want, tie_budget=0.0, what=""):
    """got: PairMetrics of numpy arrays; want: the mirror's list.  Invalid sets identical; map / n_matched / exact / type_acc / bond_acc exact;
    rmsd within RMSD_TOL.  A pair may carry another map only when the mirror scores both maps within 1e-9 of each other (a genuine tie of the
    second assignment), and only ``tie_budget`` of the pairs may."""
    P = len(want)
    assert got.rmsd.shape == (P,) and got.map.shape == (P, SM.W)
    ties, worst = 0, 0.0
    for p, w in enumerate(want):
        tag = f"{what} pair {p}"
        assert bool(np.isnan(got.rmsd[p])) == (not w["valid"]), tag
        if not np.array_equal(got.map[p], w["map"]):
            own = SM.second_match_score(w["internals"], w["map"]) if "internals" in w else None
            other = SM.second_match_score(w["internals"], got.map[p]) if "internals" in w else None
            assert own is not None and abs(own - other) <= 1e-9, f"{tag}: map differs and is no tie (mirror {own}, kernel's map {other})"
            ties += 1
            continue
        assert got.n_matched[p] == w["n_matched"] and got.exact[p] == w["exact"], tag
        assert got.type_acc[p] == w["type_acc"] and got.bond_acc[p] == w["bond_acc"], tag
        if w["valid"]:
            worst = max(worst, abs(got.rmsd[p] - w["rmsd"]))
            assert abs(got.rmsd[p] - w["rmsd"]) <= RMSD_TOL, f"{tag}: rmsd {got.rmsd[p]!r} vs {w['rmsd']!r}"
        else:
            assert got.type_acc[p] == 0 and got.bond_acc[p] == 0 and got.exact[p] == 0 and (got.map[p] == -1).all(), tag
    assert ties <= tie_budget * P, f"{what}: {ties} of {P} pairs sit on a tie"
    return ties, worst


@pytest.fixture(scope="module")
def synthetic():
    return SM.synthetic_pairs(3000, 20261017)


def test_parity_on_seeded_synthetic_pairs(gpu_device, synthetic):
    ref_rec, ref_n, prb_rec, prb_n = synthetic
    want = SM.match_batch(prb_rec, prb_n, ref_rec, ref_n, want_internals=True)
    invalid = sum(not w["valid"] for w in want)
    assert invalid <= 0.10 * len(want), f"{invalid} invalid pairs: the recipe no longer exercises the metric"
    jittered = SM.match_batch(prb_rec, prb_n, ref_rec, ref_n, jitter=np.random.default_rng(1))
    moved = sum(not np.array_equal(a["map"], b["map"]) for a, b in zip(want, jittered))
    assert moved == 0, f"{moved} maps change under a 1e-7 cost jitter: those pairs sit on ties two correct solvers may break differently"
    got = _run(gpu_device, (ref_rec, ref_n), (prb_rec, prb_n))
    ties, worst = _compare(got, want, tie_budget=0.001, what="synthetic")
    print(f"[structure] {len(want)} pairs: {invalid} invalid, {int(got.exact.sum())} exact, {ties} tie pairs, max |rmsd - mirror| = {worst:.3e}")
    # the same pairs without clipping and with a looser floor
    sub = slice(0, 400)
    for kw in (dict(max_distance=float("inf")), dict(max_distance=2.5, min_atoms=5), dict(min_atoms=1)):
        w = SM.match_batch(prb_rec[sub], prb_n[sub], ref_rec[sub], ref_n[sub], want_internals=True, **kw)
        j = SM.match_batch(prb_rec[sub], prb_n[sub], ref_rec[sub], ref_n[sub], jitter=np.random.default_rng(1), **kw)
        assert all(np.array_equal(a["map"], b["map"]) for a, b in zip(w, j)), f"{kw}: a map moves under the 1e-7 jitter"
        _compare(_run(gpu_device, (ref_rec[sub], ref_n[sub]), (prb_rec[sub], prb_n[sub]), **kw), w, tie_budget=0.001, what=str(kw))
    # the list interface of the reference (rmsd.py:232-273)
    dev = lambda a: torch.as_tensor(a).to(gpu_device)
    rl, rate, mean_rmsd, mean_acc = hungarian_rmsd_batch((dev(ref_rec), dev(ref_n)), (dev(prb_rec), dev(prb_n)))
    ok = [w for w in want if w["valid"]]
    assert [r is None for r in rl] == [not w["valid"] for w in want] and rate == len(ok) / len(want)
    assert abs(mean_rmsd - np.mean([w["rmsd"] for w in ok])) < 1e-9 and abs(mean_acc - np.mean([float(w["type_acc"]) for w in ok])) < 1e-6


def _rec(pos, types, bond, fc=None):
    n = len(types)
    return SM.record_from_mol(np.asarray(pos, np.float64), np.asarray(types), np.zeros(n, np.int64) if fc is None else fc, np.asarray(bond))


def _chain(n):
    b = np.zeros((n, n), np.int64)
    for i in range(n - 1):
        b[i, i + 1] = b[i + 1, i] = 1
    return b


def test_edge_cases(gpu_device, synthetic):
    ref_rec, ref_n, prb_rec, prb_n = synthetic
    rng = np.random.default_rng(3)
    big = int(np.argmax(ref_n))
    cases = []                                                      # (prb_rec, prb_n, ref_rec, ref_n)
    for n in (1, 2):                                                # fewer than three atoms
        pos = rng.normal(size=(n, 3))
        r = _rec(pos, [1] * n, _chain(n))
        cases += [(r, n, ref_rec[big], ref_n[big]), (prb_rec[big], prb_n[big], r, n), (r, n, r, n)]
    n_small = 6
    nobond = _rec(rng.normal(size=(n_small, 3)) * 2, [1, 1, 3, 0, 0, 0], np.zeros((n_small, n_small), np.int64))
    cases += [(nobond, n_small, ref_rec[big], ref_n[big]), (prb_rec[big], prb_n[big], nobond, n_small)]      # no bonds: one-atom fragment
    cases += [(prb_rec[big], 0, ref_rec[big], ref_n[big]), (prb_rec[big], prb_n[big], ref_rec[big], 0)]      # an atom count of zero
    for bad_value, role in ((np.nan, 0), (np.inf, 0), (np.nan, 1), (-np.inf, 1)):      # a non-finite coordinate: no cost matrix, no map
        mol = SM.mol_from_record((prb_rec if role == 0 else ref_rec)[big], (prb_n if role == 0 else ref_n)[big])
        mol["pos"][5, 1] = bad_value
        broken = _rec(mol["pos"], mol["type"], mol["bond"], mol["fc"])
        cases.append((broken, len(mol["type"]), ref_rec[big], ref_n[big]) if role == 0 else (prb_rec[big], prb_n[big], broken, len(mol["type"])))
    n_invalid = len(cases)
    # two equally large fragments: the one that holds atom 0 is the molecule, in the generated and in the ground-truth role
    tri = np.array([[0.0, 0.0, 0.0], [1.2, 0.1, 0.0], [1.9, 1.1, 0.3]])
    six = np.zeros((6, 3))
    six[[0, 2, 4]], six[[1, 3, 5]] = tri, tri @ SM._rotation(rng) + 6.0
    sb = np.zeros((6, 6), np.int64)
    for half in ([0, 2, 4], [1, 3, 5]):
        sb[np.ix_(half, half)] = _chain(3)
    two_frag, one_frag = _rec(six, [1, 0, 1, 0, 3, 0], sb), _rec(tri + 0.5, [1, 1, 3], _chain(3))
    first_frag = len(cases)
    cases += [(two_frag, 6, one_frag, 3), (one_frag, 3, two_frag, 6)]
    drop = 9                                                        # a pair whose candidate lost atoms: fewer generated than true atoms ...
    assert prb_n[drop] < ref_n[drop]
    cases += [(prb_rec[drop], prb_n[drop], ref_rec[drop], ref_n[drop]), (ref_rec[drop], ref_n[drop], prb_rec[drop], prb_n[drop])]   # ... and the reverse
    first_invalid_free = len(cases)
    # planar (a distorted ring in z = 0) and collinear molecules: a rank-deficient Kabsch matrix
    ang = np.linspace(0, 2 * np.pi, 7)[:-1] + rng.normal(size=6) * 0.05
    ring = np.stack([1.4 * np.cos(ang), 1.4 * np.sin(ang) * 1.1, np.zeros(6)], 1)
    rb = _chain(6)
    rb[0, 5] = rb[5, 0] = 2
    planar = _rec(ring, [1, 1, 2, 1, 3, 1], rb)
    c, s = np.cos(0.05), np.sin(0.05)
    planar_moved = _rec(ring @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) + rng.normal(size=(6, 3)) * [0.02, 0.02, 0.0] + 1.0, [1, 1, 2, 1, 3, 1], rb)
    line = np.array([[0, 0, 0], [1.16, 0, 0], [2.40, 0, 0]], np.float64)
    co2 = _rec(line, [3, 1, 3], _chain(3) * 2)
    co2_moved = _rec(line * 1.02 + 0.5, [3, 1, 3], _chain(3) * 2)
    cases += [(planar_moved, 6, planar, 6), (planar, 6, planar, 6), (co2_moved, 3, co2, 3), (co2, 3, co2, 3), (planar, 6, co2, 3), (co2, 3, planar, 6)]
    pr, pn, rr, rn = (np.stack([c[0] for c in cases]), np.array([c[1] for c in cases], np.int32), np.stack([c[2] for c in cases]),
                      np.array([c[3] for c in cases], np.int32))
    got = _run(gpu_device, (rr, rn), (pr, pn))
    want = SM.match_batch(pr, pn, rr, rn, want_internals=True)
    # where the answer does not hang on the completion of a rank-deficient SVD (which LAPACK and a Jacobi sweep choose differently) the mirror decides
    _compare(PairMetrics(*(a[:first_invalid_free] for a in got)), want[:first_invalid_free], what="edge")
    assert np.isnan(got.rmsd[:n_invalid]).all() and (got.n_matched[:n_invalid] == 0).all() and (got.map[:n_invalid] == -1).all()
    assert got.map[first_frag][:6].tolist() == [0, -1, 1, -1, 2, -1] and got.map[first_frag + 1][:3].tolist() == [0, 2, 4]
    assert (got.rmsd[first_frag:first_frag + 2] < 1e-6).all() and got.exact[first_frag:first_frag + 2].tolist() == [0, 0]
    # planar / collinear: finite everywhere, NaN only where the pair is invalid; identical molecules are exact hits with zero RMSD
    tail = slice(first_invalid_free, None)
    assert np.isfinite(got.type_acc[tail]).all() and np.isfinite(got.bond_acc[tail]).all() and not np.isinf(got.rmsd[tail]).any()
    assert (np.isnan(got.rmsd[tail]) == (got.n_matched[tail] < 3)).all()
    assert got.n_matched[tail][:4].tolist() == [6, 6, 3, 3] and got.exact[tail].tolist() == [1, 1, 1, 1, 0, 0]
    assert got.rmsd[first_invalid_free + 1] < 1e-12 and got.rmsd[first_invalid_free + 3] < 1e-12
    assert got.rmsd[first_invalid_free] < 0.1 and got.rmsd[first_invalid_free + 2] < 0.1
    _compare(PairMetrics(*(a[first_invalid_free:first_invalid_free + 2] for a in got)), want[first_invalid_free:first_invalid_free + 2], what="planar")
    # P = 0
    empty = _run(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert empty.rmsd.shape == (0,) and empty.map.shape == (0, SM.W)
    assert _run(gpu_device, (rr[:0], rn[:0]), (pr[:0], pn[:0])).exact.shape == (0,)
    # ref_index: K candidates share one ground-truth row; a row outside the table is an invalid pair, not a read
    K, S = 4, 25
    idx = np.repeat(np.arange(S), K)
    cand = np.stack([prb_rec[(s + k * 7) % 100] if k else prb_rec[s] for s in range(S) for k in range(K)])
    cand_n = np.array([prb_n[(s + k * 7) % 100] if k else prb_n[s] for s in range(S) for k in range(K)], np.int32)
    got = _run(gpu_device, (ref_rec[:S], ref_n[:S]), (cand, cand_n), ref_index=idx)
    want = SM.match_batch(cand, cand_n, ref_rec[:S], ref_n[:S], ref_index=idx, want_internals=True)
    # the same precondition as the parity test: a pair whose mirror map moves under a 1e-7 cost jitter sits on a tie and is left out (foreign
    # candidates are not derived from their ground truth, so the seeded recipe's check does not cover them); no tie allowance beyond that
    jittered = SM.match_batch(cand, cand_n, ref_rec[:S], ref_n[:S], ref_index=idx, jitter=np.random.default_rng(2))
    firm = np.array([np.array_equal(a["map"], b["map"]) and a["valid"] == b["valid"] for a, b in zip(want, jittered)])
    assert firm.sum() >= 0.9 * len(want), f"only {int(firm.sum())} of {len(want)} shared-row pairs are free of ties"
    _compare(PairMetrics(*(a[firm] for a in got)), [w for w, f in zip(want, firm) if f], tie_budget=0.0, what="ref_index")
    idx_bad = idx.copy()
    idx_bad[[3, 50]] = [S, -1]
    bad = _run(gpu_device, (ref_rec[:S], ref_n[:S]), (cand, cand_n), ref_index=idx_bad)
    assert np.isnan(bad.rmsd[[3, 50]]).all() and (bad.map[[3, 50]] == -1).all() and (bad.n_matched[[3, 50]] == 0).all()
    keep = np.ones(S * K, bool)
    keep[[3, 50]] = False
    assert all(np.array_equal(a[keep], b[keep], equal_nan=True) for a, b in zip(bad, got))
    s = topk_summary(dict(rmsd=torch.as_tensor(got.rmsd), exact=torch.as_tensor(got.exact)), K)
    assert s["best_rmsd"].shape == (S,) and int(s["hit"].sum()) >= int(got.exact[::K].sum())


def test_batch_independence(gpu_device, synthetic):
    """A pair's outputs are bit-identical alone, first, last and among 10 000."""
    ref_rec, ref_n, prb_rec, prb_n = synthetic
    rep = np.arange(10000) % 3000
    big = _run(gpu_device, (ref_rec[rep], ref_n[rep]), (prb_rec[rep], prb_n[rep]))
    base = _run(gpu_device, (ref_rec, ref_n), (prb_rec, prb_n))
    for a, b in zip(big, base):
        for lo in range(0, 10000, 3000):
            part = a[lo:lo + 3000]
            assert np.array_equal(part.view(np.uint8) if part.dtype.kind == "f" else part, (b[:len(part)].view(np.uint8) if b.dtype.kind == "f" else b[:len(part)]))
    for p in (0, 17, 1234, 2999):
        alone = _run(gpu_device, (ref_rec[p:p + 1], ref_n[p:p + 1]), (prb_rec[p:p + 1], prb_n[p:p + 1]))
        order = np.r_[p, np.arange(200)]                              # first
        first = _run(gpu_device, (ref_rec[order], ref_n[order]), (prb_rec[order], prb_n[order]))
        order = np.r_[np.arange(200), p]                              # last
        last = _run(gpu_device, (ref_rec[order], ref_n[order]), (prb_rec[order], prb_n[order]))
        for x, f, l, b in zip(alone, first, last, base):
            bits = lambda v: np.ascontiguousarray(v).view(np.uint8).tobytes()
            assert bits(x[0]) == bits(f[0]) == bits(l[-1]) == bits(b[p])


def _graph_dataset(count, seed):
    from diffspectra_amd import filler
    rng = np.random.default_rng(seed)
    items = []
    for i in range(count):
        n = int(rng.integers(4, 13))
        pos, types, fc, bond = SM.random_tree_molecule(rng, n)
        src, dst = np.nonzero(bond)
        items.append(SimpleNamespace(ir=torch.log10(1.0 + filler.uniform(f"smg.ir{i}", (1, 3501)).abs()), num_atom=torch.tensor(n),
                                     pos=torch.tensor(pos - pos.mean(0), dtype=torch.float32), rdmol=None, atom_type=torch.tensor(types),
                                     fc=torch.tensor(fc), edge_index=torch.tensor(np.stack([src, dst])), edge_type=torch.tensor(bond[src, dst])))
    return items


def test_evaluate_with_structure_metrics(gpu_device, tmp_path, monkeypatch):
    """get_cond_sampling_eval_fn(top_k=3) on filler weights through diffspectra_evaluate(structure_metrics=True): exactly what the mirror
    computes from the returned processed_mols and the table's ground truth; one planted slot (its record overwritten with its ground
    truth) is a certified hit for its spectrum."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    import diffspectra_amd.dmt  # noqa: F401
    K, S = 3, 5
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=S)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K
    items = _graph_dataset(8, seed=21)
    table = PackedSpectraTable.from_dataset(items, "ir", device=gpu_device)
    assert table.gt_records.device.type == "cuda" and table.gt_records.shape == (8, shard.RECORD_BYTES)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:S].repeat_interleave(K)
    planted = 1 * K + 1                                               # second candidate of the second spectrum
    gather = shard.gather_by_slot

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = table.gt_records[slot_ds[planted]]
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    mols, st = res[40]["processed_mols"], res[40]["metrics"]["structure"]
    assert len(mols) == S * K
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    want = []
    for p, (pos, atom, edge, fc) in enumerate(mols):
        prb = SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom))
        j = int(slot_ds[p])
        assert len(atom) == gt_n[j]
        want.append(SM.match_pair(prb, SM.mol_from_record(gt_rec[j], gt_n[j]), want_internals=True))
    got = PairMetrics(*(t.cpu().numpy() for t in st["per_pair"]))
    _compare(got, want, what="pipeline")
    ok = [w for w in want if w["valid"]]
    print(f"[structure] pipeline: {len(ok)} of {len(want)} pairs valid, n_matched {got.n_matched.tolist()}")
    assert st["rmsd_list"] == [float(r) if v else None for r, v in zip(got.rmsd, ~np.isnan(got.rmsd))]
    assert st["success_rate"] == len(ok) / len(want)
    assert abs(st["mean_rmsd"] - np.mean([w["rmsd"] for w in ok])) < 1e-9
    assert abs(st["mean_atom_type_accuracy"] - np.mean([float(w["type_acc"]) for w in ok])) < 1e-6
    assert abs(st["mean_bond_accuracy"] - np.mean([float(w["bond_acc"]) for w in ok])) < 1e-6
    assert st["exact_rate"] == sum(w["exact"] for w in want) / len(want)
    # the planted slot: a certified hit with zero RMSD, best of its spectrum
    assert want[planted]["exact"] == 1 and got.exact[planted] == 1 and got.rmsd[planted] < 1e-6
    top = {k: v.cpu() for k, v in st["top_k"].items()}
    assert bool(top["hit"][1]) and int(top["best_index"][1]) == 1 and float(top["best_rmsd"][1]) == got.rmsd[planted]
    r = np.where(np.isnan(got.rmsd), np.inf, got.rmsd).reshape(S, K)
    assert top["hit"].tolist() == got.exact.reshape(S, K).any(1).tolist() and float(top["hit_at_k"]) == got.exact.reshape(S, K).any(1).mean()
    assert np.array_equal(np.where(np.isinf(r.min(1)), -1, r.argmin(1)), top["best_index"].numpy())
    # the default call returns what it returned before: no structure entry, K = 1
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table)
    assert "structure" not in plain[40]["metrics"] and len(plain[40]["processed_mols"]) == S
