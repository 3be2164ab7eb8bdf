"""GPU: ``dsc_stereo_identity_records`` and ``dsc_stereo_sites`` (one wave per pair / record) against the plain-Python mirror of
tests/stereo_mirror.py - verdict, counts and sites equal exactly, every returned map checked here to be an isomorphism with the property its
verdict claims, the volumes within 1e-12 - plus the edges of the shape, the budget, consistency with ``ds_graph_identity_records``, run-to-run
and batch independence, ``chirality`` and the evaluation driver end to end."""
import functools

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E
from diffspectra_amd.structure_metrics import (GraphIdentity, StereoIdentity, chirality, stereo_identity_batch, stereo_sites, topk_identity)
from tests import graph_mirror as GM, stereo_mirror as K, structure_mirror as SM
from tests.helpers import run_records, to_dev

pytestmark = pytest.mark.gpu

_run = functools.partial(run_records, E.stereo_identity_records, StereoIdentity)     # (dev, ref, prb, ref_index=None, **scalars) -> StereoIdentity of numpy arrays
_graph = functools.partial(run_records, E.graph_identity_records, GraphIdentity)
WITH_MAP = (K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED)


def _against_mirror(got, want, prb, ref, exhaustive, what):
    """``got`` of a search that ended (no verdict 2) against the mirror's ``compare`` results."""
    for p, (w, a, b) in enumerate(zip(want, prb, ref)):
        where = f"{what} pair {p}"
        assert got.verdict[p] == w["verdict"], (where, got.verdict[p], w["verdict"], got.found[p], w["found"])
        assert got.sites[p].tolist() == w["sites"], (where, got.sites[p], w["sites"])
        assert K.map_claim(a, b, got.map[p], int(got.verdict[p])), (where, got.verdict[p], got.map[p])
        if exhaustive:
            assert got.found[p].tolist() == w["found"], (where, got.found[p], w["found"])
        else:                                                             # counted until the search stopped: never more than there are
            assert all(g <= f for g, f in zip(got.found[p], w["found"])) and (got.found[p, 0] >= 1) == (w["found"][0] >= 1), (where, got.found[p])
            assert (got.found[p, 1] >= 1) == (w["verdict"] == K.IDENTICAL), (where, got.found[p])


@pytest.mark.parametrize("exhaustive", [False, True])
def test_hand_table(gpu_device, exhaustive):
    table = K.hand_table()
    prb, ref = [t[1] for t in table], [t[2] for t in table]
    want = [K.compare(a, b) for a, b in zip(prb, ref)]
    assert [w["verdict"] for w in want] == [t[4] for t in table]         # the mirror against the stated table (tests/test_stereo_cpu.py has the counts)
    got = _run(gpu_device, ref, prb, exhaustive=exhaustive)
    print(f"[stereo] hand table, exhaustive={exhaustive}: verdicts {got.verdict.tolist()} nodes {got.nodes.tolist()} found {got.found.tolist()}")
    _against_mirror(got, want, prb, ref, exhaustive, "hand")
    if exhaustive:
        for (name, _, _, counts, _), found in zip(table, got.found.tolist()):
            assert counts is None or tuple(found) == counts, (name, found, counts)


@pytest.mark.parametrize("exhaustive", [False, True])
def test_seeded_set(gpu_device, exhaustive):
    prb, ref, names = K.seeded_pairs()
    want = K.seeded_results()
    got = _run(gpu_device, ref, prb, exhaustive=exhaustive)
    print(f"[stereo] {len(prb)} seeded pairs, exhaustive={exhaustive}: verdict counts {np.bincount(got.verdict, minlength=7).tolist()}, "
          f"nodes mean {got.nodes.mean():.3f} max {got.nodes.max()}, mirror margin {min(w['margin'] for w in want):.3e}")
    assert (got.verdict != K.UNDECIDED).all()
    _against_mirror(got, want, prb, ref, exhaustive, "seeded")
    # rigid motion plus renumbering changes nothing but the map
    by_name = {n: k for k, n in enumerate(names)}
    for n, k in by_name.items():
        if n.endswith("/moved"):
            base = by_name[n[:-len("moved")] + "identity"]
            assert got.verdict[k] == got.verdict[base] and got.found[k].tolist() == got.found[base].tolist() and got.sites[k].tolist() == got.sites[base].tolist(), n


def test_sites(gpu_device):
    """The prologue alone: masks exact, volumes within 1e-12 (absolute; |V| <= 3.08), an unusable record zeroed."""
    mols = [t[1] for t in K.hand_table()] + [t[2] for t in K.hand_table()] + K.seeded_pairs()[0][::3]
    loud = dict(mols[0], type=mols[0]["type"].copy())
    loud["type"][1] = 7                                                   # a type above 4: unusable
    heavy = dict(mols[0], bond=np.asarray(mols[0]["bond"]).copy())
    heavy["bond"][0, 1] = heavy["bond"][1, 0] = 4                        # a bond byte above 3: unusable
    mols += [loud, heavy, GM.molecule([], [])]
    rec, n = SM.records(mols)
    got = stereo_sites(to_dev(gpu_device, rec, torch.uint8), n)
    masks = torch.stack(got[:7], dim=1).cpu().numpy()
    volume, status = got.volume.cpu().numpy(), got.status.cpu().numpy()
    worst = 0.0
    for p, m in enumerate(mols):
        w_masks, w_vol, w_status = K.site_masks(m)
        assert status[p] == w_status and masks[p].tolist() == w_masks, (p, status[p], masks[p], w_masks)
        assert np.array_equal(np.isnan(volume[p]), np.isnan(w_vol)), p
        on = ~np.isnan(w_vol)
        if on.any():
            worst = max(worst, float(np.abs(volume[p][on] - w_vol[on]).max()))
    print(f"[stereo] sites of {len(mols)} records: {int((masks[:, 0] != 0).sum())} with centres, {int((masks[:, 3] != 0).sum())} with E/Z bonds, "
          f"max |V - mirror| {worst:.3e}")
    assert worst <= 1e-12
    assert status[-3:].tolist() == [3, 3, 3] and (masks[-3:] == 0).all() and np.isnan(volume[-3:]).all()
    cube = E.stereo_sites(*(to_dev(gpu_device, a, dt) for a, dt in zip(SM.records([K.cubane()]), (torch.uint8, torch.int32))))[1][0, :8].cpu().numpy()
    assert np.allclose(np.abs(cube), 1.0 + np.sqrt(3.0), atol=1e-6) and (cube > 0).sum() == 4       # eight centres of |V| = 2.732, four of each sign
    # other thresholds move the assigned bits only
    strict = stereo_sites(to_dev(gpu_device, rec, torch.uint8), n, min_volume=3.0, min_planarity=0.999)
    for p, m in enumerate(mols):
        assert torch.stack(strict[:7], dim=1)[p].cpu().tolist() == K.site_masks(m, 3.0, 0.999)[0], p
    with pytest.raises(ValueError):
        stereo_sites(to_dev(gpu_device, rec, torch.uint8), n, min_volume=float("nan"))
    with pytest.raises(ValueError):
        stereo_sites(to_dev(gpu_device, rec, torch.uint8), n, min_planarity=-0.1)


def test_edges_of_the_shape(gpu_device):
    rng = np.random.default_rng(31)
    fe, big = K.fluoroethanol(), next(m for m in K.seeded_pairs()[1] if len(m["type"]) == 29)
    empty, one = GM.molecule([], []), GM.molecule([1], [])
    moved_big = K.renumbered(big, rng)
    less = dict(pos=big["pos"][:28], type=big["type"][:28], fc=big["fc"][:28], bond=big["bond"][:28, :28])
    # lane 28 active and decisive: a 29-atom molecule whose last atom is the centre's fourth neighbour
    tail = K.Builder()
    chain = [tail.atom(K.C, (1.5 * k, 0.0, 0.0), k - 1 if k else None) for k in range(25)]
    at = np.array((1.5 * 24, 0.0, 0.0)) + K.T[0] * 1.5
    centre = tail.atom(K.C, at, chain[-1])
    tail.atom(K.F, at - K.T[1] * 1.4, centre)
    tail.atom(K.O, at - K.T[2] * 1.4, centre)
    last = tail.atom(K.H, at - K.T[3] * 1.1, centre)
    tail = tail.done()
    assert len(tail["type"]) == 29 and last == 28
    # a NaN coordinate on a site (-> 6) and on a non-site atom (no effect)
    nan_site, nan_off = dict(fe, pos=fe["pos"].copy()), dict(fe, pos=fe["pos"].copy())
    nan_site["pos"][K.perceive(fe)["tetra"][0]["nbrs"][1], 2] = np.nan
    off = next(i for i in range(len(fe["type"])) if K.perceive(fe)["twin"][i])
    nan_off["pos"][off] = np.nan
    cases = [(empty, empty), (one, one), (one, GM.molecule([2], [])), (empty, one), (moved_big, big), (less, big), (big, less),
             (K.renumbered(tail, rng), tail), (K.renumbered(K.reflected(tail), rng), tail), (nan_site, fe), (fe, nan_site), (nan_off, fe),
             (K.reflected(nan_off), fe)]
    prb, ref = [c[0] for c in cases], [c[1] for c in cases]
    want = [K.compare(a, b) for a, b in zip(prb, ref)]
    assert [w["verdict"] for w in want] == [1, 1, 0, 0, want[4]["verdict"], 0, 0, 1, 4, 6, 6, 1, 4] and want[4]["verdict"] in (1, 6)
    for exhaustive in (False, True):
        got = _run(gpu_device, ref, prb, exhaustive=exhaustive)
        _against_mirror(got, want, prb, ref, exhaustive, "edge")
        assert got.nodes[0] == 0 and (got.map[0] == -1).all() and got.found[0].tolist() == [1, 1, 0] and got.map[1].tolist() == [0] + [-1] * 28
    # record bytes past n filled with 0xFF: types, charges, positions and bonds of the atoms >= n are never read
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    dirty_r, dirty_p = rr.copy(), pr.copy()
    for rec, counts in ((dirty_r, rn), (dirty_p, pn)):
        for p, n in enumerate(counts):
            pos = rec[p, SM.POS:SM.TYPE].reshape(SM.W, 12)
            pos[n:] = 0xFF
            rec[p, SM.TYPE + n:SM.FC] = 0xFF
            rec[p, SM.FC + n:SM.BOND] = 0xFF
            bond = rec[p, SM.BOND:SM.BOND_END].reshape(SM.W, SM.W)
            bond[n:, :] = 0xFF
            bond[:, n:] = 0xFF
            bond[np.tril_indices(SM.W)] = 0xFF
            rec[p, SM.BOND_END:] = 0xFF
    clean, dirty = _run(gpu_device, (rr, rn), (pr, pn), exhaustive=True), _run(gpu_device, (dirty_r, rn), (dirty_p, pn), exhaustive=True)
    assert all(np.array_equal(x, y) for x, y in zip(clean, dirty))
    # ref_index = -1 and = M: verdict 3, zeros, -1, and nothing else changes; M = 0 with ref_index; P = 0
    rows = np.arange(len(cases), dtype=np.int64)
    bad_rows = rows.copy()
    bad_rows[[2, 7]] = [-1, len(cases)]
    bad = _run(gpu_device, (rr, rn), (pr, pn), ref_index=bad_rows, exhaustive=True)
    assert bad.verdict[[2, 7]].tolist() == [3, 3] and (bad.map[[2, 7]] == -1).all() and not bad.nodes[[2, 7]].any() and not bad.found[[2, 7]].any() \
        and not bad.sites[[2, 7]].any()
    keep = np.ones(len(cases), bool)
    keep[[2, 7]] = False
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(bad, clean))
    none = _run(gpu_device, (rr[:0], rn[:0]), (pr, pn), ref_index=rows)
    assert (none.verdict == 3).all() and (none.map == -1).all() and not none.found.any() and not none.sites.any()
    zero = _run(gpu_device, (rr, rn), (pr[:0], pn[:0]))
    assert zero.verdict.shape == (0,) and zero.found.shape == (0, 3) and zero.sites.shape == (0, 4) and zero.map.shape == (0, SM.W)
    # guard rows around every output
    P, G = len(cases), 3
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    dev = lambda a, dt: to_dev(gpu_device, a, dt)

    def guarded(width, dtype):
        raw = torch.full((P + 2 * G, width), 0x5A, dtype=torch.uint8, device=gpu_device)
        return raw, raw[G:G + P].view(dtype) if dtype != torch.uint8 else raw[G:G + P]
    bufs = [guarded(1, torch.uint8), guarded(4, torch.int32), guarded(12, torch.int32), guarded(16, torch.int32), guarded(4 * SM.W, torch.int32)]
    pr_d, pn_d, rr_d, rn_d = dev(pr, torch.uint8), dev(pn, torch.int32), dev(rr, torch.uint8), dev(rn, torch.int32)
    st = lib.dsc_stereo_identity_records(pr_d.data_ptr(), pn_d.data_ptr(), P, rr_d.data_ptr(), rn_d.data_ptr(), P, None, 4096, 0.5, 0.5, 1,
                                         *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0
    for (raw, view), want_arr in zip(bufs, clean):
        assert bool((raw[:G] == 0x5A).all()) and bool((raw[-G:] == 0x5A).all())
        assert np.array_equal(view.cpu().numpy().reshape(want_arr.shape), want_arr)
    sbufs = [guarded(4 * 7, torch.int32), guarded(8 * SM.W, torch.float64), guarded(1, torch.uint8)]
    st = lib.dsc_stereo_sites(pr_d.data_ptr(), pn_d.data_ptr(), P, 0.5, 0.5, *(view.data_ptr() for _, view in sbufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(bool((raw[:G] == 0x5A).all()) and bool((raw[-G:] == 0x5A).all()) for raw, _ in sbufs)
    plain = E.stereo_sites(pr_d, pn_d)
    assert all(np.array_equal(view.cpu().numpy().reshape(t.shape), t.cpu().numpy(), equal_nan=True) for (_, view), t in zip(sbufs, plain))
    # the argument check
    for kw in (dict(min_volume=float("nan")), dict(min_planarity=-1.0), dict(max_nodes=-1), dict(max_nodes=E.GRAPH_MAX_NODES + 1)):
        with pytest.raises(ValueError):
            _run(gpu_device, (rr, rn), (pr, pn), **kw)
    nan = float("nan")
    assert lib.dsc_stereo_identity_records(pr_d.data_ptr(), pn_d.data_ptr(), P, rr_d.data_ptr(), rn_d.data_ptr(), P, None, 4096, nan, 0.5, 0,
                                           *(view.data_ptr() for _, view in bufs), stream) == E.CONSTS["DS_ERR_ARG"]
    assert lib.dsc_stereo_identity_records(pr_d.data_ptr(), pn_d.data_ptr(), P, rr_d.data_ptr(), rn_d.data_ptr(), P, None, 4096, 0.5, 0.5, 2,
                                           *(view.data_ptr() for _, view in bufs), stream) == E.CONSTS["DS_ERR_ARG"]
    assert lib.dsc_stereo_sites(pr_d.data_ptr(), pn_d.data_ptr(), P, 0.5, -0.5, *(view.data_ptr() for _, view in sbufs), stream) == E.CONSTS["DS_ERR_ARG"]


def test_budget(gpu_device):
    """``max_nodes`` = 0 is plain refinement; K29 at 64 nodes and cubane one node short of its need end undecided, with exactly the budget
    spent.  K29 is cut off under ``exhaustive = 1`` (29! automorphisms): without it the search ends at its first leaf after 28 nodes, which
    is a same phi of a molecule without sites, and that is asserted too."""
    rng = np.random.default_rng(32)
    cube, k29 = K.cubane(), GM.k29()
    hard = GM.hard_pairs()
    # max_nodes = 0 is plain refinement: what refinement alone orders is decided, the rest is undecided without a node
    prb, ref = [K.fluoroethanol(), K.renumbered(K.fluoroethanol(), rng), cube, hard[0][1]], [K.fluoroethanol(), K.reflected(K.fluoroethanol()), cube, hard[0][2]]
    plain = _run(gpu_device, ref, prb, max_nodes=0, exhaustive=True)
    assert plain.verdict.tolist() == [1, 4, 2, 2] and not plain.nodes.any() and (plain.map[2:] == -1).all()
    # K29 has 29! automorphisms: the enumeration ends at its budget, exactly; the first same phi needs far fewer nodes
    moved = GM.permuted(k29, rng)
    cut = _run(gpu_device, [k29], [moved], max_nodes=64, exhaustive=True)
    assert cut.verdict.tolist() == [2] and cut.nodes.tolist() == [64] and (cut.map == -1).all() and cut.found[0, 0] >= 1
    first = _run(gpu_device, [k29], [moved], max_nodes=64)
    same = _graph(gpu_device, [k29], [moved], max_nodes=64)
    assert first.verdict.tolist() == [1] and first.nodes.tolist() == same.nodes.tolist() and GM.is_isomorphism(moved, k29, first.map[0])
    # cubane: (48, 24, 24) with the default budget; below its need the enumeration is undecided
    turned = K.renumbered(cube, rng)
    full = _run(gpu_device, [cube], [turned], exhaustive=True)
    need = int(full.nodes[0])
    print(f"[stereo] cubane: found {full.found[0].tolist()} in {need} nodes")
    assert full.verdict.tolist() == [1] and full.found[0].tolist() == [48, 24, 24] and need >= 48
    short = _run(gpu_device, [cube], [turned], max_nodes=need - 1, exhaustive=True)
    assert short.verdict.tolist() == [2] and short.nodes.tolist() == [need - 1] and (short.map == -1).all()
    assert _run(gpu_device, [cube], [turned], max_nodes=need, exhaustive=True).found[0].tolist() == [48, 24, 24]


def test_consistent_with_graph_identity(gpu_device):
    """With the default budget: verdict in {1, 4, 5, 6} exactly where ``ds_graph_identity_records`` says 1, 0 exactly where it says 0."""
    ref, prb, _ = GM.seeded_pairs()
    ref, prb = list(ref[:600]) + K.seeded_pairs()[1], list(prb[:600]) + K.seeded_pairs()[0]
    graph = _graph(gpu_device, ref, prb)
    for exhaustive in (False, True):
        got = _run(gpu_device, ref, prb, exhaustive=exhaustive)
        assert (graph.verdict <= 1).all() and (got.verdict != 2).all()
        assert np.array_equal(np.isin(got.verdict, WITH_MAP), graph.verdict == 1) and np.array_equal(got.verdict == 0, graph.verdict == 0)
    assert (graph.verdict == 1).sum() > 100 and (graph.verdict == 0).sum() > 100
    batch = stereo_identity_batch((to_dev(gpu_device, SM.records(ref)[0], torch.uint8), SM.records(ref)[1]),
                                  (to_dev(gpu_device, SM.records(prb)[0], torch.uint8), SM.records(prb)[1]), exhaustive=True)
    assert np.array_equal(batch.verdict.cpu().numpy(), got.verdict) and np.array_equal(batch.same_constitution.cpu().numpy(), graph.verdict == 1)
    assert np.array_equal(batch.identical.cpu().numpy(), got.verdict == 1) and np.array_equal(batch.mirror.cpu().numpy(), got.verdict == 4)
    assert np.array_equal(batch.stereoisomer.cpu().numpy(), got.verdict == 5) and np.array_equal(batch.unassigned.cpu().numpy(), got.verdict == 6)
    assert not batch.undecided.any()
    top = topk_identity(batch.verdict[:600], 4)                           # the Top-K reduction of the graph verdicts works on these unchanged
    assert top["hit"].cpu().tolist() == (got.verdict[:600] == 1).reshape(-1, 4).any(1).tolist()


def test_twice_and_in_two_splits(gpu_device):
    """Every output is bit-identical run to run and whatever the batch around a pair."""
    table = K.hand_table()
    prb, ref = [t[1] for t in table] + K.seeded_pairs()[0], [t[2] for t in table] + K.seeded_pairs()[1]
    (rr, rn), (pr, pn) = SM.records(ref), SM.records(prb)
    for exhaustive in (False, True):
        a, b = _run(gpu_device, (rr, rn), (pr, pn), exhaustive=exhaustive), _run(gpu_device, (rr, rn), (pr, pn), exhaustive=exhaustive)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        for cut in (1, 131):
            lo, hi = _run(gpu_device, (rr[:cut], rn[:cut]), (pr[:cut], pn[:cut]), exhaustive=exhaustive), \
                _run(gpu_device, (rr[cut:], rn[cut:]), (pr[cut:], pn[cut:]), exhaustive=exhaustive)
            assert all(np.concatenate([x, y]).tobytes() == z.tobytes() for x, y, z in zip(lo, hi, a)), cut


def test_chirality(gpu_device):
    mols = [K.fluoroethanol(), K.difluorobutane(False), K.difluorobutane(True), K.difluorocyclobutane(True), K.difluorocyclobutane(False),
            K.difluoroethene(True), K.acetaldoxime(True), K.methane(), K.neopentane(), K.cubane(), K.difluoroallene(), K.fluoroethanol(flat=True)]
    rec, n = SM.records(mols)
    got = chirality(to_dev(gpu_device, rec, torch.uint8), n)
    assert got.chiral.dtype == torch.uint8 and got.automorphisms.dtype == torch.int32
    assert got.chiral.cpu().tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]     # the allene is chiral in fact: the stated deviation
    assert got.automorphisms.cpu().tolist() == [1, 2, 2, 4, 4, 2, 1, 1, 24, 48, 2, 1]
    assert [K.compare(m, m)["found"][0] for m in mols] == got.automorphisms.cpu().tolist()
    short = chirality(to_dev(gpu_device, rec, torch.uint8), n, max_nodes=3)
    assert short.chiral.cpu().tolist()[9] == 2 and short.automorphisms.cpu().tolist()[9] == -1 and short.chiral.cpu().tolist()[0] == 1


def test_evaluate_reports_stereo_identity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) with config.eval.stereo on filler weights, 3 steps, K = 2: one slot's record is replaced by
    its ground truth under another atom order after a rigid motion; metrics['structure']['stereo'] equals the mirror's verdicts, its rates
    sum as they should, and the key is absent without the flag."""
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
    cfg.eval.stereo = True
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    mols, st = res[40]["processed_mols"], res[40]["metrics"]["structure"]
    stereo = st["stereo"]
    assert set(stereo) == {"verdict", "identity_rate", "constitution_rate", "enantiomer_rate", "stereoisomer_rate", "unassigned", "undecided",
                           "sites", "chiral_targets", "top_k"}
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in mols]
    targets = [SM.mol_from_record(gt_rec[int(j)], gt_n[int(j)]) for j in slot_ds]
    want = [K.compare(m, t) for m, t in zip(made, targets)]
    assert min(w["margin"] for w in want) >= 1e-6
    verdict = stereo["verdict"].cpu().numpy()
    assert verdict.dtype == np.uint8 and verdict.tolist() == [w["verdict"] for w in want]
    assert verdict[planted] in (1, 6) and verdict[planted] == K.compare(truth, truth)["verdict"]
    assert stereo["sites"].cpu().tolist() == [w["sites"] for w in want]
    P = len(want)
    count = lambda *codes: sum(int(v) in codes for v in verdict) / P
    assert stereo["identity_rate"] == count(1) and stereo["enantiomer_rate"] == count(4) and stereo["stereoisomer_rate"] == count(5)
    assert stereo["constitution_rate"] == count(1, 4, 5, 6) and stereo["unassigned"] == int((verdict == 6).sum()) and stereo["undecided"] == 0
    assert abs(stereo["constitution_rate"] - (stereo["identity_rate"] + stereo["enantiomer_rate"] + stereo["stereoisomer_rate"] + stereo["unassigned"] / P)) < 1e-12
    assert stereo["constitution_rate"] == st["graph"]["identity_rate"]
    own = [K.compare(t, t) for t in targets]
    assert stereo["chiral_targets"] == sum(o["verdict"] == 1 and o["sites"][0] > 0 and o["found"][2] == 0 for o in own) / P
    top = {k: v.cpu() for k, v in stereo["top_k"].items()}
    assert top["hit"].tolist() == (verdict == 1).reshape(S, top_k).any(1).tolist()
    # a stricter threshold passes through: every centre of the planted pair is then unassigned or was absent
    cfg.eval.stereo_min_volume = 3.5
    again = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    made = [SM.mol_from_record(SM.record_from_mol(pos.numpy(), atom.numpy(), fc.numpy(), edge.numpy()), len(atom)) for pos, atom, edge, fc in again["processed_mols"]]
    strict = again["metrics"]["structure"]["stereo"]
    assert strict["verdict"].cpu().tolist() == [K.compare(m, t, min_volume=3.5)["verdict"] for m, t in zip(made, targets)]
    assert strict["unassigned"] >= stereo["unassigned"]
    # without the flag there is no such key
    cfg.eval.stereo = False
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    assert "stereo" not in plain[40]["metrics"]["structure"]
