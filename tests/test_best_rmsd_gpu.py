"""GPU: ``dsr_best_rmsd_records`` (one wave per pair) against the plain-numpy mirror of tests/best_rmsd_mirror.py - verdict, count and found
exactly, the values on their squares within the rounding bound of the trace formula, every returned map checked here to be an isomorphism
and to be the map behind its value - plus the laws of the definition, the budget, batch independence and the evaluation driver end to end.

The bound: |got^2 - want^2| <= 256 * 2^-53 * G / count per pair (``best_rmsd_mirror.BOUND_FACTOR``).  Every test prints the largest ratio
|got^2 - want^2| / bound that it saw."""
import functools

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E
from diffspectra_amd.structure_metrics import BestRmsd, GraphIdentity, best_rmsd_batch, topk_best_rmsd
from tests import best_rmsd_mirror as R, stereo_mirror as K, structure_mirror as SM
from tests.helpers import run_records, to_dev

pytestmark = pytest.mark.gpu

_run = functools.partial(run_records, E.best_rmsd_records, BestRmsd)     # (dev, ref, prb, ref_index=None, **scalars) -> BestRmsd of numpy arrays
_graph = functools.partial(run_records, E.graph_identity_records, GraphIdentity)


def _ratio(got_value, want_value, bound):
    diff = abs(got_value ** 2 - want_value ** 2)
    return 0.0 if diff == 0.0 else diff / bound


def _against_mirror(got, want, prb, ref, atoms, what):
    """``got`` of searches that ended against the mirror's ``compare`` results.  Returns (largest ratio to the bound, pairs whose maps were
    compared with the mirror's optimal set, pairs with a value)."""
    worst, compared, valued = 0.0, 0, 0
    for p, (w, a, b) in enumerate(zip(want, prb, ref)):
        where = f"{what} pair {p} ({atoms})"
        assert got.verdict[p] == w["verdict"] and got.count[p] == w["count"] and got.found[p] == w["found"], \
            (where, got.verdict[p], w["verdict"], got.count[p], w["count"], got.found[p], w["found"])
        if w["verdict"] != R.DECIDED:
            assert np.isnan(got.rmsd[p]).all() and (got.map[p] == -1).all(), where
            continue
        bound = R.bound_of(a, b, atoms)
        for kind in (0, 1):
            image = got.map[p, kind]
            assert R.is_isomorphism(a, b, image, atoms), (where, kind, image)
            if not w["count"]:
                assert np.isnan(got.rmsd[p, kind]), where
                continue
            ratio = _ratio(got.rmsd[p, kind], w["best"][kind], bound)
            assert ratio <= 1.0, (where, kind, got.rmsd[p, kind], w["best"][kind], ratio)
            own = R.values_of_map(a, b, image, atoms)[kind]                # the returned map is the phi behind the value
            back = _ratio(got.rmsd[p, kind], own, bound)
            assert back <= 1.0, (where, kind, got.rmsd[p, kind], own, back)
            worst = max(worst, ratio, back)
            if w["runner_up"][kind] - w["best"][kind] >= 1e-6:
                assert tuple(int(image[i]) for i in w["selected"]) in w["optimal"][kind], (where, kind, image)
                compared += kind == 0
        valued += bool(w["count"])
    return worst, compared, valued


def test_hand_table(gpu_device):
    table = R.hand_pairs()
    worst = 0.0
    for atoms in ("heavy", "all"):
        rows = [t for t in table if t[3] == atoms]
        prb, ref = [t[1] for t in rows], [t[2] for t in rows]
        want = [R.compare(a, b, atoms) for a, b in zip(prb, ref)]
        got = _run(gpu_device, ref, prb, atoms=atoms)
        print(f"[best_rmsd] hand table, {atoms}: verdict {got.verdict.tolist()} count {got.count.tolist()} found {got.found.tolist()} nodes {got.nodes.tolist()}\n"
              f"            proper {np.round(got.rmsd[:, 0], 6).tolist()}\n            improper {np.round(got.rmsd[:, 1], 6).tolist()}")
        worst = max(worst, _against_mirror(got, want, prb, ref, atoms, "hand")[0])
        named = {t[0]: k for k, t in enumerate(rows)}
        if atoms == "heavy":
            assert got.found[[named[n] for n, _, _ in R.skeletons()]].tolist() == [48, 24, 6, 12, 72]
            k = named["H2, heavy"]
            assert got.verdict[k] == 1 and got.count[k] == 0 and np.isnan(got.rmsd[k]).all() and got.map[k, 0, :2].tolist() in ([0, 1], [1, 0])
            k = named["one heavy atom"]
            assert got.rmsd[k].tolist() == [0.0, 0.0] and got.map[k, :, 0].tolist() == [0, 0] and (got.map[k, :, 1:] == -1).all() and got.nodes[k] == 0
            k = named["four heavy substituents / mirror image"]
            assert got.rmsd[k, 1] < 1e-6 and got.rmsd[k, 0] > 0.5
            assert got.verdict[[named["one atom against two"], named["a changed bond byte"]]].tolist() == [0, 0]
            # ref_index out of range: verdict 3, every row defined, the other rows unchanged
            rows_idx = np.arange(len(rows), dtype=np.int64)
            rows_idx[[1, 4]] = [-1, len(rows)]
            bad = _run(gpu_device, ref, prb, ref_index=rows_idx, atoms=atoms)
            assert bad.verdict[[1, 4]].tolist() == [3, 3] and np.isnan(bad.rmsd[[1, 4]]).all() and (bad.map[[1, 4]] == -1).all()
            assert not bad.count[[1, 4]].any() and not bad.nodes[[1, 4]].any() and not bad.found[[1, 4]].any()
            keep = np.ones(len(rows), bool)
            keep[[1, 4]] = False
            assert all(x[keep].tobytes() == y[keep].tobytes() for x, y in zip(bad, got))
        else:
            assert got.found[named["ethane, all"]] == 72 and got.found[named["CF2H2, F swapped, all"]] == 4
            assert got.rmsd[named["water, H renumbered, all"], 0] < 1e-6
    print(f"[best_rmsd] hand table: largest |got^2 - want^2| / bound = {worst:.3f}")


@pytest.mark.parametrize("atoms", ["heavy", "all"])
def test_seeded_set(gpu_device, atoms):
    prb, ref, _ = R.seeded_pairs()
    want = R.seeded_results(atoms)
    keep = [p for p, w in enumerate(want) if w is not None]
    prb, ref, want = [prb[p] for p in keep], [ref[p] for p in keep], [want[p] for p in keep]
    got = _run(gpu_device, ref, prb, atoms=atoms)
    assert (got.verdict != R.UNDECIDED).all()
    worst, compared, valued = _against_mirror(got, want, prb, ref, atoms, "seeded")
    full = [p for p, m in enumerate(ref) if len(m["type"]) == SM.W]
    print(f"[best_rmsd] {len(prb)} seeded pairs, {atoms}: verdict counts {np.bincount(got.verdict, minlength=4).tolist()}, {len(full)} with 29 atoms, "
          f"nodes mean {got.nodes.mean():.2f} max {got.nodes.max()}, found max {got.found.max()}, maps compared on {compared} of {valued} valued pairs, "
          f"largest |got^2 - want^2| / bound = {worst:.3f}")
    assert len(full) >= 40 and (got.verdict[full] == 1).sum() >= 20
    assert valued - compared <= 0.05 * valued                             # the share left out of the map comparison


def _on_grid(mol):
    """Positions rounded to multiples of 2^-10: sums and differences of such numbers below 32 are exact in fp32."""
    return dict(mol, pos=np.round(np.asarray(mol["pos"]) * 1024.0) / 1024.0)


def _moved_exactly(mol, rng):
    """A quarter-turn rotation (x, y, z) -> (y, -x, z) composed with a cyclic change of axes, a shift on the grid and a renumbering: a rigid
    motion that fp32 holds exactly for positions on the grid."""
    n = len(mol["type"])
    perm = rng.permutation(n)
    pos = np.asarray(mol["pos"])[:, [1, 0, 2]] * (1.0, -1.0, 1.0)
    pos = np.roll(pos, int(rng.integers(3)), axis=1) + rng.integers(-2048, 2049, size=(1, 3)) / 1024.0
    assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
    return dict(pos=pos[perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=np.asarray(mol["bond"])[np.ix_(perm, perm)].copy())


def test_laws(gpu_device):
    prb, ref, kinds = R.seeded_pairs()
    rng = np.random.default_rng(51)
    prb, ref = [_on_grid(m) for m in prb[:300]], [_on_grid(m) for m in ref[:300]]
    base = _run(gpu_device, ref, prb)
    # the verdict is that of the graph identity
    graph = _graph(gpu_device, ref, prb)
    assert (graph.verdict <= 1).all() and np.array_equal(base.verdict, graph.verdict) and (base.verdict == 1).sum() > 150
    # a rigid motion and a renumbering of A change neither value beyond twice the bound (each run is within one bound of the truth)
    again = _run(gpu_device, ref, [_moved_exactly(m, rng) for m in prb])
    turned = _run(gpu_device, ref, [R.reflected(m) for m in prb])
    assert np.array_equal(again.verdict, base.verdict) and np.array_equal(again.found, base.found) and np.array_equal(again.count, base.count)
    assert np.array_equal(turned.verdict, base.verdict) and np.array_equal(turned.found, base.found)
    worst_move, worst_turn, exact_turn = 0.0, 0.0, 0
    for p in np.flatnonzero((base.verdict == 1) & (base.count > 0)):
        bound = R.bound_of(prb[p], ref[p], "heavy")
        for kind in (0, 1):
            worst_move = max(worst_move, _ratio(again.rmsd[p, kind], base.rmsd[p, kind], bound))
            worst_turn = max(worst_turn, _ratio(turned.rmsd[p, 1 - kind], base.rmsd[p, kind], bound))      # reflecting A swaps the two columns
        exact_turn += turned.rmsd[p, ::-1].tobytes() == base.rmsd[p].tobytes()
    print(f"[best_rmsd] laws on {(base.verdict == 1).sum()} decided pairs: moved A {worst_move:.3f}, reflected A {worst_turn:.3f} of the bound "
          f"({exact_turn} reflected pairs swap bit for bit)")
    assert worst_move <= 2.0 and worst_turn <= 2.0
    # the values recomputed from the returned maps and the maps as isomorphisms: _against_mirror does both
    want = [R.compare(a, b) for a, b in zip(prb, ref)]
    _against_mirror(base, want, prb, ref, "heavy", "laws")
    batch = best_rmsd_batch((to_dev(gpu_device, SM.records(ref)[0], torch.uint8), SM.records(ref)[1]),
                            (to_dev(gpu_device, SM.records(prb)[0], torch.uint8), SM.records(prb)[1]))
    assert all(np.array_equal(x.cpu().numpy(), y, equal_nan=True) for x, y in zip(batch, base))
    top = topk_best_rmsd(batch, 4)
    assert top["hit"].cpu().tolist() == (base.verdict == 1).reshape(-1, 4).any(1).tolist() and int(top["undecided"]) == 0
    filled = np.where((base.verdict == 1) & ~np.isnan(base.rmsd[:, 0]), base.rmsd[:, 0], np.inf).reshape(-1, 4)
    assert np.array_equal(top["best_rmsd"].cpu().numpy(), np.where(np.isinf(filled.min(1)), np.nan, filled.min(1)), equal_nan=True)


def test_edges_of_the_shape(gpu_device):
    """Bytes past n are never read, nothing is written outside the output rows, a position that is not finite gives NaN values and no map,
    and the empty shapes (P = 0; M = 0 with ``ref_index``) are defined."""
    rows = [t for t in R.hand_pairs() if t[3] == "heavy"]
    prb, ref = [t[1] for t in rows], [t[2] for t in rows]
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    clean = _run(gpu_device, (rr, rn), (pr, pn))
    dirty_r, dirty_p = rr.copy(), pr.copy()
    for rec, counts in ((dirty_r, rn), (dirty_p, pn)):
        for p, n in enumerate(counts):
            rec[p, SM.POS:SM.TYPE].reshape(SM.W, 12)[n:] = 0xFF
            rec[p, SM.TYPE + n:SM.FC] = 0xFF
            rec[p, SM.FC + n:SM.BOND] = 0xFF
            bond = rec[p, SM.BOND:SM.BOND_END].reshape(SM.W, SM.W)
            bond[n:, :] = 0xFF
            bond[:, n:] = 0xFF
            bond[np.tril_indices(SM.W)] = 0xFF
            rec[p, SM.BOND_END:] = 0xFF
    dirty = _run(gpu_device, (dirty_r, rn), (dirty_p, pn))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    # guard rows around every output
    P, G = len(rows), 3
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    dev = lambda a, dt: to_dev(gpu_device, a, dt)

    def guarded(width, dtype):
        raw = torch.full((P + 2 * G, width), 0x5A, dtype=torch.uint8, device=gpu_device)
        return raw, raw[G:G + P].view(dtype) if dtype != torch.uint8 else raw[G:G + P]
    bufs = [guarded(1, torch.uint8), guarded(16, torch.float64), guarded(4, torch.int32), guarded(4, torch.int32), guarded(4, torch.int32),
            guarded(8 * SM.W, torch.int32)]
    pr_d, pn_d, rr_d, rn_d = dev(pr, torch.uint8), dev(pn, torch.int32), dev(rr, torch.uint8), dev(rn, torch.int32)
    st = lib.dsr_best_rmsd_records(pr_d.data_ptr(), pn_d.data_ptr(), P, rr_d.data_ptr(), rn_d.data_ptr(), P, None, 4096, 0,
                                   *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0
    for (raw, view), want_arr in zip(bufs, clean):
        assert bool((raw[:G] == 0x5A).all()) and bool((raw[-G:] == 0x5A).all())
        assert view.cpu().numpy().tobytes() == want_arr.tobytes()
    assert lib.dsr_best_rmsd_records(pr_d.data_ptr(), pn_d.data_ptr(), P, rr_d.data_ptr(), rn_d.data_ptr(), P, None, 4096, 2,
                                     *(view.data_ptr() for _, view in bufs), stream) == E.CONSTS["DS_ERR_ARG"]
    # a position that is not finite: an isomorphism exists, no value, no map
    neo = K.neopentane()
    hurt = dict(neo, pos=neo["pos"].copy())
    hurt["pos"][1, 2] = np.nan
    got = _run(gpu_device, [neo, hurt], [hurt, neo])
    assert got.verdict.tolist() == [1, 1] and got.found.tolist() == [24, 24] and np.isnan(got.rmsd).all() and (got.map == -1).all()
    # the empty shapes
    none = _run(gpu_device, (rr[:0], rn[:0]), (pr, pn), ref_index=np.arange(P, dtype=np.int64))
    assert (none.verdict == 3).all() and np.isnan(none.rmsd).all() and (none.map == -1).all() and not none.count.any() and not none.found.any()
    zero = _run(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert zero.verdict.shape == (0,) and zero.rmsd.shape == (0, 2) and zero.map.shape == (0, 2, SM.W)


def test_budget(gpu_device):
    """Neopentane in ALL mode has 24 * 6^4 isomorphisms: undecided at 4096 nodes, with exactly the budget spent and nothing reported.  Ethane
    (72) decides.  ``max_nodes`` = 0 is plain refinement: a colouring that refinement makes discrete is decided without a node, any other
    pair is undecided."""
    rng = np.random.default_rng(52)
    neo, eth, fe = K.neopentane(), R.ethane(), K.fluoroethanol()
    cut = _run(gpu_device, [neo], [R.moved(neo, rng, 0.05)], atoms="all", max_nodes=4096)
    assert cut.verdict.tolist() == [2] and cut.nodes.tolist() == [4096] and np.isnan(cut.rmsd).all() and (cut.map == -1).all() and cut.found[0] >= 1
    assert cut.count.tolist() == [17]
    heavy = _run(gpu_device, [neo], [R.moved(neo, rng, 0.05)])
    assert heavy.verdict.tolist() == [1] and heavy.found.tolist() == [24] and heavy.count.tolist() == [5]
    made = R.moved(eth, rng, 0.05)
    full = _run(gpu_device, [eth], [made], atoms="all")
    need = int(full.nodes[0])
    print(f"[best_rmsd] ethane, all atoms: found {full.found.tolist()} in {need} nodes; neopentane, heavy: {heavy.nodes.tolist()} nodes")
    assert full.verdict.tolist() == [1] and full.found.tolist() == [72] and 72 <= need <= 4096
    short = _run(gpu_device, [eth], [made], atoms="all", max_nodes=need - 1)
    assert short.verdict.tolist() == [2] and short.nodes.tolist() == [need - 1] and np.isnan(short.rmsd).all() and (short.map == -1).all()
    exact = _run(gpu_device, [eth], [made], atoms="all", max_nodes=need)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(exact, full))
    plain = _run(gpu_device, [fe, eth, eth], [R.moved(fe, rng), made, made], max_nodes=0)      # heavy: the hydrogens of a methyl group are ordered
    assert plain.verdict.tolist() == [1, 2, 2] and not plain.nodes.any() and plain.found.tolist() == [1, 0, 0]
    assert plain.rmsd[0, 0] < 1e-5 and np.isnan(plain.rmsd[1:]).all() and (plain.map[1:] == -1).all()
    for kw in (dict(max_nodes=-1), dict(max_nodes=E.GRAPH_MAX_NODES + 1), dict(atoms="some")):
        with pytest.raises(ValueError):
            _run(gpu_device, [eth], [made], **kw)


def test_alone_first_last_and_among_ten_thousand(gpu_device):
    """A pair's outputs are bit-identical alone, first, last and in the middle of 10 000 pairs, and run to run."""
    prb, ref, _ = R.seeded_pairs()
    rng = np.random.default_rng(53)
    cube = K.cubane()
    targets = [(R.moved(cube, rng, 0.1), cube), next((a, b) for a, b in zip(prb, ref) if len(b["type"]) == SM.W and R.compare(a, b)["verdict"] == 1)]
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    reps = -(-10000 // len(ref))
    for atoms in ("heavy", "all"):
        for a, b in targets:
            alone = _run(gpu_device, [b], [a], atoms=atoms)
            assert alone.verdict[0] in (1, 2)
            (tr, tn), (tp, tpn) = SM.records([b]), SM.records([a])
            big_r, big_rn = np.tile(rr, (reps, 1))[:10000].copy(), np.tile(rn, reps)[:10000].copy()
            big_p, big_pn = np.tile(pr, (reps, 1))[:10000].copy(), np.tile(pn, reps)[:10000].copy()
            spots = [0, 4321, 9999]
            for s in spots:
                big_r[s], big_rn[s], big_p[s], big_pn[s] = tr[0], tn[0], tp[0], tpn[0]
            many = _run(gpu_device, (big_r, big_rn), (big_p, big_pn), atoms=atoms)
            twice = _run(gpu_device, (big_r, big_rn), (big_p, big_pn), atoms=atoms)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(many, twice)) and many.verdict.shape == (10000,) and (many.verdict == 1).sum() > 7000
            for s in spots:
                assert all(x[s].tobytes() == y[0].tobytes() for x, y in zip(many, alone)), (atoms, s)


def test_evaluate_reports_best_rmsd(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) with config.eval.best_rmsd on filler weights, 3 steps, K = 2: one slot's record is replaced
    by its ground truth under another atom order after a rigid motion; metrics['structure']['best_rmsd'] equals the mirror's verdicts, its
    counts add up to the slots, and the key is absent without the flag."""
    from diffspectra_amd import filler, evaluate as EV, shard
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    top_k, S = 2, 4
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=S)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", top_k
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:S].repeat_interleave(top_k)
    planted = 1 * top_k + 1
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    truth = SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])])
    moved = K.renumbered(truth, np.random.default_rng(33))
    gather = shard.gather_by_slot

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    cfg.eval.best_rmsd = True
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    mols, st = res[40]["processed_mols"], res[40]["metrics"]["structure"]
    entry = st["best_rmsd"]
    assert set(entry) == {"verdict", "rmsd", "hits", "undecided", "invalid", "mean", "median", "mirror_better", "within", "top_k"}
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in mols]
    targets = [SM.mol_from_record(gt_rec[int(j)], gt_n[int(j)]) for j in slot_ds]
    want = [R.compare(m, t) for m, t in zip(made, targets)]
    verdict, rmsd = entry["verdict"].cpu().numpy(), entry["rmsd"].cpu().numpy()
    P = len(want)
    assert verdict.dtype == np.uint8 and verdict.tolist() == [w["verdict"] for w in want] and rmsd.shape == (P, 2)
    assert verdict[planted] == 1 and rmsd[planted, 0] < 1e-5                             # the planted copy: fp32 rounding of the moved positions
    for p, w in enumerate(want):
        if w["verdict"] == 1 and w["count"]:
            assert _ratio(rmsd[p, 0], w["best"][0], R.bound_of(made[p], targets[p], "heavy")) <= 1.0, p
    assert entry["hits"] == int((verdict == 1).sum()) >= 1 and entry["undecided"] == 0 and entry["invalid"] == 0
    assert entry["hits"] + entry["undecided"] + entry["invalid"] + int((verdict == 0).sum()) == P == S * top_k
    assert np.array_equal(verdict == 1, st["graph"]["verdict"].cpu().numpy() == 1)
    values = rmsd[(verdict == 1) & np.isfinite(rmsd[:, 0]), 0]
    assert abs(entry["mean"] - values.mean()) < 1e-12 and set(entry["within"]) == {0.1, 0.25, 0.5, 1.0}
    assert entry["within"][0.1] == float((values < 0.1).mean()) and entry["mirror_better"] == int(((verdict == 1) & (rmsd[:, 1] < rmsd[:, 0])).sum())
    top = {k: v.cpu() for k, v in entry["top_k"].items()}
    assert top["hit"].tolist() == (verdict == 1).reshape(S, top_k).any(1).tolist() and top["best_index"][1] == 1
    # the mode and the thresholds pass through
    cfg.eval.best_rmsd_atoms, cfg.eval.best_rmsd_thresholds, cfg.eval.best_rmsd_max_nodes = "all", (0.3,), 1 << 16
    again = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    every, same_graph = again["best_rmsd"], again["graph"]["verdict"].cpu().numpy()
    all_verdict, all_rmsd = every["verdict"].cpu().numpy(), every["rmsd"].cpu().numpy()
    assert set(every["within"]) == {0.3} and np.array_equal(all_verdict == 0, same_graph == 0)       # (a hit may run out of the budget in this mode)
    assert every["hits"] + every["undecided"] == int((same_graph == 1).sum())
    assert all_rmsd[planted, 0] < 1e-5 if all_verdict[planted] == 1 else all_verdict[planted] == 2
    # without the flag there is no such key
    cfg.eval.best_rmsd = False
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    assert "best_rmsd" not in plain[40]["metrics"]["structure"]
    assert set(plain[40]["metrics"]["structure"]) == set(st) - {"best_rmsd"}
