"""GPU: the substructure-geometry MMD against tests/geometry_mirror.py.

Extraction (``ds_geometry_count_records`` / ``ds_geometry_fill_records``): counts, classes, order and ``skipped`` exact, values within one fp32
ulp of the mirror's fp64 value rounded to fp32 (dihedrals compared on the circle).  MMD (``ds_mmd_1d_segments``): |gpu - fp64 mirror| <= 8 D,
D the reference's own |fp32 - fp64| read from tests/golden/g18_geometry.npz - the reference's fp32 number is what users compare with, and
eight times its own deviation leaves room for another ``exp`` and another order of summation and nothing more.  Then
``get_sub_geometry_metric`` and the evaluation driver end to end."""
import functools
import json

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import geometry_mirror as GEO, graph_mirror as GM, mces_mirror as MM, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_geometry_cpu import GOLDEN, mmd_cases, reference_deviation

pytestmark = pytest.mark.gpu

CLASSES = S.geometry_classes()
CODES = [list(c) for c in CLASSES.codes]
TILE = E.MMD_TILE


# ---------------------------------------------------------------------------------------------- extraction

def _extract(dev, mols, codes=CODES):
    """Both kernels on molecule dicts or on a ``(records, n)`` pair -> (counts [P, 3], skipped [P], offsets [P, 3], [(value, cls)] per kind)."""
    rec, n = SM.records(mols) if isinstance(mols, list) else mols
    rec, n = to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)
    tabs = [torch.tensor(c, dtype=torch.int32, device=dev) for c in codes]
    counts, skipped = E.geometry_count_records(rec, n, *tabs)
    assert counts.dtype == torch.int32 and counts.shape == (len(n), 3) and skipped.dtype == torch.int32 and skipped.shape == (len(n),)
    ends = counts.to(torch.int64).cumsum(0)
    totals = ends[-1].tolist() if len(n) else [0, 0, 0]
    offsets = (ends - counts).contiguous()
    filled = E.geometry_fill_records(rec, n, *tabs, offsets, totals)
    torch.cuda.synchronize()
    for (value, cls), total in zip(filled, totals):
        assert value.dtype == torch.float32 and cls.dtype == torch.uint8 and value.shape == cls.shape == (total,)
    return counts.cpu().numpy(), skipped.cpu().numpy(), offsets.cpu().numpy(), [(v.cpu().numpy(), c.cpu().numpy()) for v, c in filled]


def _ulp_apart(kind, got, want32):
    """|got - want| in units of one fp32 ulp of want; dihedrals on the circle."""
    diff = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    if kind == 2:
        diff = np.minimum(diff, 360.0 - diff)
    return diff / np.spacing(np.maximum(np.abs(want32), np.float32(1e-30))).astype(np.float64)


def _check(dev, mols, codes=CODES, what=""):
    """The kernels' output for every molecule is the mirror's: counts, skipped, classes in order; values within one fp32 ulp."""
    if not isinstance(mols, list):
        mols = [SM.mol_from_record(r, k) for r, k in zip(*mols)]
    counts, skipped, offsets, filled = _extract(dev, mols, codes)
    worst = 0.0
    for p, mol in enumerate(mols):
        want, want_skipped = GEO.extract(mol, codes)
        assert skipped[p] == want_skipped, f"{what} molecule {p}: skipped {skipped[p]}, the mirror has {want_skipped}"
        for kind, (v64, v32, cls, _) in enumerate(want):
            assert counts[p, kind] == len(cls), f"{what} molecule {p} {GEO.KINDS[kind]}: {counts[p, kind]} entries, the mirror has {len(cls)}"
            lo = offsets[p, kind]
            got_v, got_c = filled[kind][0][lo:lo + len(cls)], filled[kind][1][lo:lo + len(cls)]
            assert np.array_equal(got_c, cls), f"{what} molecule {p} {GEO.KINDS[kind]}: classes"
            if len(cls):
                apart = _ulp_apart(kind, got_v, v32)
                worst = max(worst, float(apart.max()))
                assert apart.max() <= 1.0, f"{what} molecule {p} {GEO.KINDS[kind]}: {apart.max()} ulp at entry {int(apart.argmax())}"
    return counts, skipped, filled, worst


def _with_pos(mol, pos):
    return dict(pos=np.asarray(pos, np.float64), type=mol["type"], fc=mol["fc"], bond=mol["bond"])


def _renamed(mol, rng):
    """The same molecule, coordinates included, under another atom order."""
    perm = rng.permutation(len(mol["type"]))
    return dict(pos=np.asarray(mol["pos"])[perm].copy(), type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())


def _cyclopropane(rng):
    ring = GM.saturated(GM.carbons(3, [(0, 1), (1, 2), (0, 2)]))        # valence 4: two hydrogens per carbon
    return _with_pos(ring, rng.normal(size=(len(ring["type"]), 3)) * 1.5)


def test_seeded_molecules(gpu_device):
    """The seeded set of tests/mces_mirror.py: the generated side has coordinates, the ground truths have none (every atom at the origin: all
    their listed entries are skipped)."""
    ref, prb, _ = MM.seeded_pairs()
    counts, skipped, _, worst = _check(gpu_device, prb, what="generated")
    print(f"seeded generated: {counts.sum(0).tolist()} entries, worst {worst:.3f} ulp")
    assert counts.sum(0).min() > 500 and skipped.sum() == 0
    counts, skipped, _, _ = _check(gpu_device, ref, what="origin")
    assert counts.sum() == 0 and skipped.sum() > 1000


def test_sizes_and_offsets(gpu_device):
    """n of 0, 1, 2, 3, 4 and 29 on one record (the count cuts the molecule), n outside 0..29 clamped; the fully bonded 29 atoms with their
    406 / 10 962 / 295 974 entries between two ordinary records, which checks the offsets."""
    rng = np.random.default_rng(20261119)
    nonane = _with_pos(GM.nonane(), rng.normal(size=(29, 3)) * 2.0)
    rec, _ = SM.records([nonane] * 8)
    _check(gpu_device, (rec, np.array([0, 1, 2, 3, 4, 29, -5, 77], np.int32)), what="cut")
    k29 = _with_pos(GM.k29(), rng.normal(size=(29, 3)) * 2.0)
    small = _cyclopropane(rng)
    counts, skipped, filled, worst = _check(gpu_device, [small, k29, nonane], what="k29")
    print(f"k29: worst {worst:.3f} ulp")
    assert counts[1].tolist() == [406, 10962, 295974] and skipped[1] == 0
    assert set(filled[2][1][counts[0, 2]:counts[0, 2] + 295974].tolist()) == {CLASSES.symbols[2].index("C1C-C1C-C1C")}


def test_edges_of_the_definition(gpu_device):
    rng = np.random.default_rng(20261120)
    # a == b: the three-ring's dihedrals a - i - j - a are emitted
    ring = _cyclopropane(rng)
    _check(gpu_device, [ring], what="cyclopropane")
    assert any(a[0] == a[3] for a in GEO.extract(ring, CODES)[0][2][3].tolist())
    # four carbons on a line: bonds 1, angles exactly 180, the dihedral has no plane and is skipped
    line = _with_pos(GM.carbons(4, GM._path(0, 1, 2, 3)), [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    counts, skipped, filled, _ = _check(gpu_device, [line], what="line")
    assert counts[0].tolist() == [3, 2, 0] and skipped[0] == 1 and filled[0][0].tolist() == [1.0] * 3 and filled[1][0].tolist() == [180.0] * 2
    # two atoms at one point: their bond, the angles and the dihedrals through it are skipped
    twin = _with_pos(GM.carbons(4, GM._path(0, 1, 2, 3)), [[0, 0, 0], [1, 0.5, 0], [1, 0.5, 0], [2, 0, 1]])
    counts, skipped, _, _ = _check(gpu_device, [twin], what="twin")
    assert counts[0].tolist() == [2, 0, 0] and skipped[0] == 4
    # exactly planar: trans is +180 and never -180, cis is 0 - in both orientations and under every order of the atoms
    trans = _with_pos(GM.carbons(4, GM._path(0, 1, 2, 3)), [[-1, 1, 0], [0, 0, 0], [1, 0, 0], [2, -1, 0]])
    flat = []
    for sign in (1.0, -1.0):
        for cis in (False, True):
            pos = trans["pos"] * np.array([1.0, sign, 1.0])
            if cis:
                pos[3, 1] = pos[0, 1]
            flat += [_renamed(_with_pos(trans, pos), rng) for _ in range(6)]
    counts, skipped, filled, _ = _check(gpu_device, flat, what="planar")
    assert counts[:, 2].tolist() == [1] * 24 and skipped.sum() == 0
    assert filled[2][0].tolist() == [180.0] * 6 + [0.0] * 6 + [180.0] * 6 + [0.0] * 6
    # a bond byte or a type byte above 15 has no code: the entries through it belong to no class; the others stay
    odd = _with_pos(GM.saturated(GM.carbons(4, GM._path(0, 1, 2, 3))), rng.normal(size=(14, 3)) * 1.5)
    plain = _extract(gpu_device, [odd])[0][0]
    high = dict(odd, bond=odd["bond"].copy(), type=odd["type"].copy())
    high["bond"][1, 2] = high["bond"][2, 1] = 17
    high["bond"][0, 1] = high["bond"][1, 0] = 200
    heavy = dict(odd, type=odd["type"].copy())
    heavy["type"][0] = 17                                                            # 17 & 15 = 1 would be carbon
    counts, _, _, _ = _check(gpu_device, [high, heavy], what="above 15")
    assert (counts[0] < plain).all() and (counts[1] < plain).all() and counts[1, 0] > 0
    # a table of its own: one class per kind, written backwards, and an empty table
    mine = [[GEO_code((0, 1, 1))], [], [GEO_code((1, 1, 1, 1, 1, 1, 0))]]
    counts, _, filled, _ = _check(gpu_device, [odd, ring], mine, what="own tables")
    assert counts[:, 1].tolist() == [0, 0] and counts[0, 0] == 10 and counts[0, 2] > 0 and set(filled[2][1].tolist()) == {0}


def GEO_code(fields):
    return sum(f << (4 * k) for k, f in enumerate(fields))


def test_no_records_batch_independence_and_renaming(gpu_device):
    rec, n = SM.records(MM.seeded_pairs()[1][:200])
    counts, skipped, offsets, filled = _extract(gpu_device, (rec[:0], n[:0]))
    assert counts.shape == (0, 3) and skipped.shape == (0,) and all(v.shape == (0,) and c.shape == (0,) for v, c in filled)
    counts, skipped, offsets, filled = _extract(gpu_device, (rec, n))
    again = _extract(gpu_device, (rec, n))
    for (v, c), (v2, c2) in zip(filled, again[3]):
        assert v.tobytes() == v2.tobytes() and c.tobytes() == c2.tobytes()          # bit-identical run to run
    for p in (0, 57, 199, int(np.argmax(n))):
        c1, s1, _, f1 = _extract(gpu_device, (rec[p:p + 1], n[p:p + 1]))
        assert c1[0].tolist() == counts[p].tolist() and s1[0] == skipped[p]
        for kind in range(3):
            lo = offsets[p, kind]
            assert f1[kind][0].tobytes() == filled[kind][0][lo:lo + counts[p, kind]].tobytes(), (p, kind)
            assert f1[kind][1].tobytes() == filled[kind][1][lo:lo + counts[p, kind]].tobytes(), (p, kind)
    # renaming the atoms of a molecule (coordinates carried along) leaves every class's multiset of values as it is, bit for bit: a value
    # does not depend on the direction its entry is read in
    rng = np.random.default_rng(20261121)
    mols = [SM.mol_from_record(r, k) for r, k in zip(rec, n)]
    moved = _extract(gpu_device, [_renamed(m, rng) for m in mols])
    assert np.array_equal(moved[0], counts) and np.array_equal(moved[1], skipped)
    for kind in range(3):
        for p in range(len(mols)):
            lo, cnt = offsets[p, kind], counts[p, kind]
            a = sorted(zip(filled[kind][1][lo:lo + cnt].tolist(), filled[kind][0][lo:lo + cnt].tolist()))
            b = sorted(zip(moved[3][kind][1][lo:lo + cnt].tolist(), moved[3][kind][0][lo:lo + cnt].tolist()))
            assert a == b, (GEO.KINDS[kind], p)


# ---------------------------------------------------------------------------------------------- MMD

@functools.lru_cache(maxsize=1)
def _golden():
    g = np.load(GOLDEN)
    return g, reference_deviation(g)


def _run_mmd(dev, xs, ys, **kw):
    """One ``mmd_1d_segments`` call on lists of per-class sample arrays -> (out [C, 5], status [C]) as numpy."""
    cat = lambda parts: np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts] + [np.zeros(0, np.float32)])
    off = lambda parts: np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
    args = (to_dev(dev, cat(xs), torch.float32), to_dev(dev, off(xs), torch.int64), to_dev(dev, cat(ys), torch.float32), to_dev(dev, off(ys), torch.int64))
    out, status = E.mmd_1d_segments(*args, **kw)
    out2, status2 = E.mmd_1d_segments(*args, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and out.shape == (len(xs), 5) and status.dtype == torch.uint8 and status.shape == (len(xs),)
    assert out.cpu().numpy().tobytes() == out2.cpu().numpy().tobytes() and torch.equal(status, status2)      # bit-identical launches
    return out.cpu().numpy(), status.cpu().numpy()


def _gate(out, status, xs, ys, what, **kw):
    """|gpu - fp64 mirror| <= 8 D on mmd, XX, YY and XY of every class; prints and returns the worst case."""
    _, D = _golden()
    worst = 0.0
    for c, (x, y) in enumerate(zip(xs, ys)):
        want = GEO.mmd(np.asarray(x, np.float32), np.asarray(y, np.float32), **kw)
        if len(x) == 0 or len(y) == 0:
            assert status[c] == E.MMD_EMPTY and np.isnan(out[c]).all(), (what, c)
            continue
        assert status[c] == E.MMD_OK, (what, c)
        if want[0] != want[0]:
            assert np.isnan(out[c, :4]).all() and out[c, 4] == want[4], (what, c)
            continue
        err = np.abs(out[c, :4] - np.array(want[:4]))
        worst = max(worst, float(err.max()))
        assert err.max() <= 8 * D, f"{what} class {c}: |gpu - fp64| = {err.tolist()} (mmd, XX, YY, XY), gate 8 D = {8 * D:.3e}"
        assert abs(out[c, 4] - want[4]) <= 1e-9 * want[4], (what, c, out[c, 4], want[4])
    print(f"{what}: worst |gpu - fp64| = {worst:.3e}, D = {D:.3e}, gate {8 * D:.3e}")
    return worst


def test_mmd_golden_cases(gpu_device):
    g, D = _golden()
    names = mmd_cases(g)
    xs, ys = [g[k + ".x"] for k in names], [g[k + ".y"] for k in names]
    out, status = _run_mmd(gpu_device, xs, ys)
    _gate(out, status, xs, ys, "golden, one call")
    for k, name in enumerate(names):                                                 # and against the reference's own fp32 numbers: 8 D + D
        for key in (".ref_b97", ".ref_b1000"):
            ref = float(g[name + key])
            assert (ref != ref and out[k, 0] != out[k, 0]) or abs(out[k, 0] - ref) <= 9 * D, (name, key)
    for k in (0, 4):                                                                  # a class alone gives the bits it gives in the batch
        alone, _ = _run_mmd(gpu_device, xs[k:k + 1], ys[k:k + 1])
        assert alone[0].tobytes() == out[k].tobytes()
        assert S.mmd_1d(to_dev(gpu_device, xs[k], torch.float32), to_dev(gpu_device, ys[k], torch.float32)) == out[k, 0]
    nan = S.mmd_1d(to_dev(gpu_device, xs[-1], torch.float32), to_dev(gpu_device, ys[-1], torch.float32))
    assert nan != nan


def test_mmd_tile_edges_and_kernels(gpu_device):
    rng = np.random.default_rng(20261122)
    sizes = [(TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (2 * TILE + 1, 3), (1, 2 * TILE)]
    xs = [rng.normal(109.5, 4.0, a) for a, _ in sizes]
    ys = [rng.normal(111.0, 6.0, b) for _, b in sizes]
    _gate(*_run_mmd(gpu_device, xs, ys), xs, ys, "tile edges")
    for kw in (dict(kernel_num=1), dict(kernel_num=8), dict(kernel_num=4, kernel_mul=3.0), dict(fix_sigma=20.0), dict(kernel_num=2, fix_sigma=0.5)):
        _gate(*_run_mmd(gpu_device, xs, ys, **kw), xs, ys, f"tile edges {kw}", **kw)


def test_mmd_many_classes(gpu_device):
    """24 classes in one call, an empty source class and an empty target class among them; then offsets that cannot be used."""
    rng = np.random.default_rng(20261123)
    xs = [rng.normal(1.0 + 0.1 * c, 0.05, int(rng.integers(1, 700))) for c in range(24)]
    ys = [rng.normal(1.0 + 0.1 * c, 0.08, int(rng.integers(1, 700))) for c in range(24)]
    xs[5], ys[17] = xs[5][:0], ys[17][:0]
    out, status = _run_mmd(gpu_device, xs, ys)
    _gate(out, status, xs, ys, "24 classes")
    assert status.tolist() == [E.MMD_EMPTY if c in (5, 17) else E.MMD_OK for c in range(24)]
    dev = gpu_device
    x = to_dev(dev, rng.normal(size=40), torch.float32)
    bad = torch.tensor([0, 30, 20, 41, 40], dtype=torch.int64, device=dev)            # decreasing; beyond the end
    good = torch.tensor([0, 10, 20, 30, 40], dtype=torch.int64, device=dev)
    out, status = E.mmd_1d_segments(x, bad, x, good)
    assert status.tolist() == [E.MMD_OK, E.MMD_INVALID, E.MMD_INVALID, E.MMD_INVALID]
    assert bool(torch.isnan(out[1:]).all()) and not bool(torch.isnan(out[0]).any())
    with pytest.raises(ValueError):
        S.mmd_1d(torch.zeros(E.MMD_MAX_SAMPLES + 1, device=dev), x)
    ws = torch.empty(E.mmd_workspace_bytes(4), dtype=torch.uint8, device=dev)        # a caller-owned workspace gives the same bits
    a, _ = E.mmd_1d_segments(x, good, x.flip(0).contiguous(), good)
    b, _ = E.mmd_1d_segments(x, good, x.flip(0).contiguous(), good, workspace=ws)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- end to end

REFERENCE_KEYS = [*CLASSES.symbols[0], "bond_length_mean", *CLASSES.symbols[1], "bond_angle_mean", *CLASSES.symbols[2], "dihedral_angle_mean"]


def _mirror_samples(mols):
    """symbol -> the mirror's fp32 samples over all molecules, in the order ``sub_geometry`` returns them (by record, then the header's)."""
    found = {s: [] for kind in CLASSES.symbols for s in kind}
    for mol in mols:
        for names, (_, v32, cls, _) in zip(CLASSES.symbols, GEO.extract(mol, CODES)[0]):
            for k, name in enumerate(names):
                found[name].append(v32[cls == k])
    return {s: np.concatenate(v + [np.zeros(0, np.float32)]) for s, v in found.items()}


def test_sub_geometry_metric(gpu_device):
    _, D = _golden()
    prb = MM.seeded_pairs()[1]
    test, made = prb[:300], prb[300:420]
    pack = lambda mols: (to_dev(gpu_device, SM.records(mols)[0], torch.uint8), SM.records(mols)[1])
    got_samples = S.sub_geometry(*pack(test))
    want_test, want_made = _mirror_samples(test), _mirror_samples(made)
    assert list(got_samples.values) == [s for kind in CLASSES.symbols for s in kind] and got_samples.skipped.shape == (300,)
    for s, v in got_samples.values.items():
        assert v.dtype == torch.float32 and v.shape == want_test[s].shape, s
    for cap, seed in ((None, 0), (40, 5)):
        result = S.get_sub_geometry_metric(pack(test), max_samples=cap, seed=seed)(pack(made))
        assert list(result) == REFERENCE_KEYS and all(isinstance(v, float) for v in result.values())
        gens = [torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 1)]
        worst = 0.0
        for names, mean_name in zip(CLASSES.symbols, ("bond_length_mean", "bond_angle_mean", "dihedral_angle_mean")):
            wants = []
            for s in names:
                sides = []
                for values, gen in zip((want_test, want_made), gens):                 # the seeded cap, drawn in the metric's order
                    v = values[s]
                    sides.append(v if cap is None or len(v) <= cap else v[torch.randperm(len(v), generator=gen)[:cap].numpy()])
                want = GEO.mmd(sides[1], sides[0])[0]
                wants.append(want)
                if want != want:
                    assert result[s] != result[s], s
                else:
                    worst = max(worst, abs(result[s] - want))
                    assert abs(result[s] - want) <= 8 * D, (s, result[s], want)
            seen = [w for w in wants if w == w]
            assert seen and abs(result[mean_name] - sum(seen) / len(seen)) <= 8 * D, mean_name
        print(f"metric (cap {cap}): worst |gpu - mirror| = {worst:.3e}")
    empty = S.get_sub_geometry_metric(pack(test))(pack(MM.seeded_pairs()[0][:20]))     # generated molecules without geometry: all NaN
    assert list(empty) == REFERENCE_KEYS and all(v != v for v in empty.values())


def test_evaluate_reports_sub_geometry(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps: with ``cfg.eval.sub_geometry`` the 'structure' dict holds the
    reference's keys and the values of a direct call on ``records_by_slot``; without the flag it has no new key."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=6)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts = 40, 40, ""
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    gather, kept = shard.gather_by_slot, []

    def gather_and_keep(rec, n_atoms):
        kept.append(gather(rec, n_atoms))
        return kept[-1]
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_keep)
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert "sub_geometry" not in plain
    cfg.eval.sub_geometry = True
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"sub_geometry"}
    geo = st["sub_geometry"]
    assert list(geo) == REFERENCE_KEYS and all(isinstance(v, float) for v in geo.values())
    n_atoms = [len(atom) for _, atom, _, _ in res["processed_mols"]]
    direct = S.get_sub_geometry_metric((table.gt_records.to(gpu_device), table.num_atom))((kept[-1], torch.tensor(n_atoms)))
    assert json.dumps(geo) == json.dumps(direct)                                      # NaN for NaN, bit for bit otherwise
