"""GPU: ``dsk_scaffold_masks`` (csrc/ds_scaffold.hip) and what ``structure_metrics`` and ``evaluate`` build on it against the plain-Python mirror of
tests/scaffold_mirror.py, which is written from include/diffspectra_scaffold.h and pinned to hand-stated expectations by
tests/test_scaffold_cpu.py.  Every output is an integer or a byte and is compared exactly; the one float, ``scaf``, is the same Python
expression on the same integers on both sides and is compared with ``==``."""
import math

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, scaffold_mirror as K, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_scaffold_cpu import same_partition
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_rows(dev, rec, n):
    """``scaffold_masks`` as the mirror's list of row dicts."""
    out = [t.cpu() for t in E.scaffold_masks(*on(dev, rec, n))]
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(len(n),), (len(n),), (len(n), 4), (len(n),)]
    scaffold, ring, summary, status = (t.tolist() for t in out)
    return [dict(scaffold_mask=scaffold[p], ring_mask=ring[p], summary=tuple(summary[p]), status=status[p]) for p in range(len(status))]


def same_rows(got, want):
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (p, {k: (g[k], w[k]) for k in K.KEYS if g[k] != w[k]})
    assert len(got) == len(want)


def bits(atoms):
    return sum(1 << i for i in atoms)


@pytest.fixture(scope="module")
def molecules():
    """The table, three renumberings of each of its molecules (with the permutations), the table without hydrogens, the Kekule drawings and
    the derived set as one record table, with the mirror's rows: computed once, shared, never changed."""
    rows = K.hand_table()
    rng = np.random.default_rng(23)
    table = [mol for _, mol, _, _, _ in rows]
    perms, renumbered = [], []
    for mol in table:
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))                            # new atom i is old atom perm[i]
            perms.append(perm)
            renumbered.append(dict(pos=mol["pos"][perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy()))
    extra = [K.stripped(mol) for mol in table] + [K.other_kekule_toluene()] + list(K.kekule_pair())
    derived = K.derived_set()
    rec, n = SM.records(table + renumbered + extra + derived)
    return dict(rows=rows, perms=perms, rec=rec, n=n, want=K.analyse_table(rec, n), bare=len(table) * 4, kekule=len(table) * 5,
                derived=slice(len(n) - len(derived), len(n)))


# ------------------------------------------------------------------------------------------------------------------ the kernel

def test_table_renumberings_and_derived_set_against_the_mirror(gpu_device, molecules):
    rows, perms, rec, n, want = (molecules[k] for k in ("rows", "perms", "rec", "n", "want"))
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    # ... and so the hand-stated table holds for the kernel, under renumbering and without hydrogens
    T = len(rows)
    for k, (name, mol, scaffold, ring, rings) in enumerate(rows):
        heavy = int((np.asarray(mol["type"]) != 0).sum())
        stated = dict(scaffold_mask=bits(scaffold), ring_mask=bits(ring), summary=(heavy, len(scaffold), rings, len(ring)), status=0)
        assert got[k] == stated and got[molecules["bare"] + k] == stated, name
        for j in range(3):
            perm, g = perms[3 * k + j], got[T + 3 * k + j]
            assert g["scaffold_mask"] == bits(i for i in range(len(perm)) if int(perm[i]) in scaffold), name
            assert g["ring_mask"] == bits(i for i in range(len(perm)) if int(perm[i]) in ring) and g["summary"] == stated["summary"], name
    # the ground the comparison stands on (asserted on the mirror in tests/test_scaffold_cpu.py)
    part = got[molecules["derived"]]
    assert len(part) >= 250 and sum(g["scaffold_mask"] == 0 for g in part) >= 40 and sum(g["summary"][2] >= 2 for g in part) >= 40
    assert sum(g["summary"][1] > g["summary"][3] for g in part) >= 40 and {g["summary"][2] for g in part} >= {0, 1, 2, 3}      # linker or exocyclic atoms


def ring_of(k, start=0):
    return [(start + i, start + (i + 1) % k) for i in range(k)]


def test_sizes_garbage_and_the_hard_shapes(gpu_device):
    rng = np.random.default_rng(20261020)
    sizes = np.array([1, 2, 28, 29, 28, 29, 40, -3] * 40, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    want = K.analyse_table(rec, n)
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    assert {w["status"] for w in want} == {K.OK, K.UNUSABLE} and sum(w["summary"][2] > 0 for w in want) > 50
    assert gpu_rows(gpu_device, clean, n) == got                                 # what is ignored is ignored
    every = (1 << 29) - 1
    chain = GM.carbons(29, [(i, i + 1) for i in range(28)])
    tailed = GM.carbons(29, ring_of(3) + [(2, 3)] + [(i, i + 1) for i in range(3, 28)])            # the round-bound case: 26 rounds
    big_ring = GM.carbons(29, ring_of(29))                                                       # the longest reach test
    two_rings = GM.carbons(29, ring_of(14) + ring_of(14, 14) + [(0, 28), (28, 14)])
    sparse = [GM.random_molecule(rng, 29) for _ in range(20)]
    hard = [GM.k29(), chain, tailed, big_ring, two_rings, GM.permuted(tailed, rng), GM.permuted(two_rings, rng), GM.permuted(chain, rng)]
    rec, n = SM.records(hard + sparse)
    rec[0, SM.BOND_END:] = 0xEE
    rec[0, SM.BOND:SM.BOND_END].reshape(29, 29)[np.tril_indices(29)] = 0xEE      # garbage in the lower triangle and on the diagonal
    want = K.analyse_table(rec, n)
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    assert got[0] == dict(scaffold_mask=every, ring_mask=every, summary=(29, 29, 378, 29), status=0)
    assert got[1] == dict(scaffold_mask=0, ring_mask=0, summary=(29, 0, 0, 0), status=0) == got[7]
    assert got[2] == dict(scaffold_mask=7, ring_mask=7, summary=(29, 3, 1, 3), status=0) and got[5]["summary"] == (29, 3, 1, 3)
    assert got[3] == dict(scaffold_mask=every, ring_mask=every, summary=(29, 29, 1, 29), status=0)
    assert got[4] == dict(scaffold_mask=every, ring_mask=every & ~(1 << 28), summary=(29, 29, 2, 28), status=0) and got[6]["summary"] == (29, 29, 2, 28)


def test_every_kind_of_unusable_record(gpu_device, molecules):
    names = [name for name, *_ in molecules["rows"]]
    k = names.index("1-cyclohexylethanone")                                      # 9 heavy atoms and 14 hydrogens
    count = int(molecules["n"][k])
    assert count == 23
    base, n = np.repeat(molecules["rec"][k:k + 1], 7, axis=0), np.full(7, count, np.int32)
    n[2] = 0
    base[0, SM.TYPE + count - 1] = 5                                            # a type byte above 4 (the last atom)
    base[1, SM.BOND + 3 * 29 + 12] = 4                                          # a bond byte above 3, upper triangle
    n[3] = -7                                                                   # clamped to 0
    base[4, SM.BOND + 12 * 29 + 3] = 4                                          # the same pair in the lower triangle: not looked at
    base[5, SM.BOND + 28 * 29 + 28] = 9                                         # the diagonal: not looked at
    base[6, SM.TYPE + count] = 77                                               # an atom >= n: not looked at
    base[6, SM.BOND + 2 * 29 + count + 1] = 200
    got = gpu_rows(gpu_device, base, n)
    zero = dict(scaffold_mask=0, ring_mask=0, summary=(0, 0, 0, 0), status=K.UNUSABLE)
    assert got[:4] == [zero] * 4 and got[4:] == [molecules["want"][k]] * 3 and got == K.analyse_table(base, n)


def test_guarded_outputs_repeat_runs_and_batch_independence(gpu_device, molecules):
    """Every output between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record); two runs
    bit-identical; a row's outputs do not depend on the batch around it."""
    rng = np.random.default_rng(9)
    P = 65
    rows = rng.permutation(len(molecules["n"]))[:P]
    rec_d, n_d = on(gpu_device, molecules["rec"][rows], molecules["n"][rows])
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(width, dtype):
        raw = torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + P]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    bufs = [guarded(4, torch.int32), guarded(4, torch.int32), guarded(16, torch.int32), guarded(1, torch.uint8)]
    st = lib.dsk_scaffold_masks(rec_d.data_ptr(), n_d.data_ptr(), P, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    plain, again = E.scaffold_masks(rec_d, n_d), E.scaffold_masks(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
    assert [p["scaffold_mask"] for p in [molecules["want"][r] for r in rows]] == plain[0].cpu().tolist()
    for sub in ([64], [5], [17, 64, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        alone = E.scaffold_masks(rec_d[idx].contiguous(), n_d[idx].contiguous())
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
    assert gpu_rows(gpu_device, molecules["rec"][:0], molecules["n"][:0]) == []


# ------------------------------------------------------------------------------------------------------------------ the public interface

def test_scaffolds_scaffold_records_and_kekule_drawings(gpu_device, molecules):
    rows, rec, n, want = (molecules[k] for k in ("rows", "rec", "n", "want"))
    rec_d, n_d = on(gpu_device, rec, n)
    found = S.scaffolds(rec_d, n.tolist())
    assert isinstance(found, S.Scaffolds) and found.scaffold_mask.device.type == gpu_device.type and bool(found.usable.all())
    assert found.scaffold_mask.cpu().tolist() == [w["scaffold_mask"] for w in want] and found.rings.cpu().tolist() == [w["summary"][2] for w in want]
    for min_rings in (1, 2):
        assert found.has_scaffold(min_rings).cpu().tolist() == [K.has_scaffold(w, min_rings) for w in want]
    for orders in (True, False):
        s_rec, s_n = S.scaffold_records(rec_d, n_d, bond_orders=orders)
        assert s_rec.dtype == torch.uint8 and s_rec.shape == rec_d.shape and s_n.dtype == torch.int32
        assert s_n.cpu().tolist() == [w["summary"][1] for w in want]
        out = s_rec.cpu().numpy()
        for p in range(0, len(n), 3):
            mine, stated = SM.mol_from_record(out[p], want[p]["summary"][1]), K.scaffold_mol(rec[p], n[p], orders, want[p])
            assert all(np.array_equal(mine[f], stated[f]) for f in ("type", "fc", "bond")), p
        assert not out[:, SM.BOND_END:].any() and (orders or int(out[:, SM.BOND:SM.BOND_END].max()) == 1)
        # a fixed point once the exocyclic atoms are accounted for: every atom of a scaffold record is in its own scaffold mask - with the
        # orders; without them an exocyclic =O has become -O, and the scaffold of the framework is the core alone
        twice = S.scaffolds(s_rec, s_n)
        full = torch.bitwise_left_shift(torch.ones_like(s_n), s_n) - 1
        have = s_n > 0
        assert bool((twice.status[~have] == K.UNUSABLE).all()) and torch.equal(twice.rings[have], found.rings[have])
        if orders:
            assert torch.equal(twice.scaffold_mask[have], full[have])
        else:
            core = to_dev(gpu_device, [len(K.parts(r, k)["core"]) for r, k in zip(rec, n)], torch.int32)
            assert torch.equal(twice.summary[:, 1][have], core[have]) and torch.equal(twice.summary[:, 3][have], found.summary[:, 3][have])
        if orders:
            k = [name for name, *_ in rows].index("1-methylaziridinium (ring N+)")
            assert out[k, SM.FC:SM.FC + 3].view(np.int8).tolist() == [1, 0, 0] and out[k, SM.TYPE:SM.TYPE + 4].tolist() == [2, 1, 1, 0]
    # Kekule drawings: toluene's two are mirror images, one graph and one scaffold either way; 2-cyclopropylpyridine's are two scaffolds with
    # the orders and one without
    names = [name for name, *_ in rows]
    tol, kek = [names.index("toluene"), molecules["kekule"]], [molecules["kekule"] + 1, molecules["kekule"] + 2]
    for pair, with_orders in ((tol, 1), (kek, 2)):
        idx = to_dev(gpu_device, pair, torch.int64)
        for orders, classes in ((True, with_orders), (False, 1)):
            s_rec, s_n = S.scaffold_records(rec_d[idx].contiguous(), n_d[idx], bond_orders=orders)
            assert S.graph_classes(s_rec, s_n).unique().numel() == classes, (pair, orders)


def test_scaffold_identity_batch_against_the_mirror(gpu_device, molecules):
    rec, n = molecules["rec"], molecules["n"]
    K_, T = 4, 30
    rng = np.random.default_rng(37)
    pairs = K.hand_pairs()
    h_rec, h_n = SM.records([a for _, a, _, _ in pairs] + [b for _, _, b, _ in pairs])
    ref = (np.concatenate([rec, h_rec[4:]]), np.concatenate([n, h_n[4:]]))
    cand = rng.permutation(len(n))[:T * K_]
    prb = (np.concatenate([h_rec[:4], rec[cand][4:]]), np.concatenate([h_n[:4], n[cand][4:]]))
    targets = np.repeat(rng.integers(0, len(n), size=T), K_).astype(np.int64)
    # half of the candidates are the target itself with another substituent pattern: a neighbour in the derived set
    grown, start = rng.integers(0, 190, size=T * K_), molecules["derived"].start           # ten grown molecules per molecule of the table
    take = rng.random(T * K_) < 0.5
    targets[take] = start + grown[take] // 10 * 10 + rng.integers(0, 10, size=int(take.sum()))
    prb[0][take], prb[1][take] = rec[start + grown[take]], n[start + grown[take]]
    prb[0][:4], prb[1][:4] = h_rec[:4], h_n[:4]
    targets[:4] = len(n) + np.arange(4)
    prb[1][6] = 0                                                               # one unusable candidate
    targets[[9, 40]] = [-1, len(ref[1])]                                        # two rows outside the table
    out = S.scaffold_identity_batch(on(gpu_device, *ref), on(gpu_device, *prb), ref_index=targets)
    assert isinstance(out, S.ScaffoldIdentity) and out.same.dtype == torch.bool and out.status.dtype == torch.uint8 and out.same.device.type == gpu_device.type
    stated = []
    for p in range(T * K_):
        r = int(targets[p])
        stated.append((False, 3) if not 0 <= r < len(ref[1]) else K.same_scaffold((prb[0][p], prb[1][p]), (ref[0][r], ref[1][r])))
    assert out.same.cpu().tolist() == [s for s, _ in stated] and out.status.cpu().tolist() == [st for _, st in stated] and int(out.undecided) == 0
    assert out.same.cpu().tolist()[:4] == [same for _, _, _, same in pairs] == [True, False, True, False]
    assert out.status.cpu().tolist()[6] == 3 and [stated[p] for p in (9, 40)] == [(False, 3)] * 2
    assert 20 <= sum(s for s, _ in stated) <= T * K_ - 20                        # both verdicts are well represented
    flat = S.scaffold_identity_batch(on(gpu_device, *ref), on(gpu_device, *prb), ref_index=targets, bond_orders=False, min_rings=2)
    for p in range(0, T * K_, 5):
        r = int(targets[p])
        if 0 <= r < len(ref[1]):
            assert (bool(flat.same[p]), int(flat.status[p])) == K.same_scaffold((prb[0][p], prb[1][p]), (ref[0][r], ref[1][r]), 2, False), p


@pytest.fixture(scope="module")
def two_sets(molecules):
    """Two disjoint halves of the derived set plus 30 molecules that both get."""
    rec, n = molecules["rec"][molecules["derived"]], molecules["n"][molecules["derived"]]
    shared = np.arange(5, 305, 10)
    rest = np.setdiff1d(np.arange(len(n)), shared)
    gen, test = np.concatenate([rest[0::2], shared]), np.concatenate([rest[1::2], shared])
    return (rec[gen], n[gen]), (rec[test], n[test])


@pytest.mark.parametrize("min_rings", [1, 2])
def test_scaffold_metric_against_the_mirror(gpu_device, two_sets, min_rings):
    gen, test = two_sets
    gen_d, test_d = on(gpu_device, *gen), on(gpu_device, *test)
    want = K.scaffold_metric(gen, test, min_rings)
    assert want["distinct_generated"] >= 10 and want["distinct_test"] >= 10 and want["shared"] >= 3 and 0.0 < want["scaf"] < 1.0
    fn = S.get_scaffold_metric(test_d, min_rings=min_rings, unique=False)
    mine = fn(gen_d)
    assert set(mine) == set(want) and isinstance(mine["scaf"], float) and mine["scaffold_class"].dtype == torch.int64
    assert {k: mine[k] for k in want if k != "scaffold_class"} == {k: want[k] for k in want if k != "scaffold_class"}
    assert same_partition(mine["scaffold_class"].cpu().tolist(), want["scaffold_class"])
    # a keep mask, with the same test side
    keep = np.arange(len(gen[1])) % 3 != 0
    want = K.scaffold_metric((gen[0][keep], gen[1][keep]), test, min_rings)
    mine = fn(gen_d, keep=to_dev(gpu_device, keep, torch.bool))
    assert {k: mine[k] for k in want if k != "scaffold_class"} == {k: want[k] for k in want if k != "scaffold_class"} and mine["n_generated"] == int(keep.sum())
    # one representative per class of molecules on both sides
    gu, tu = K.unique_rows(*gen), K.unique_rows(*test)
    want = K.scaffold_metric((gen[0][gu], gen[1][gu]), (test[0][tu], test[1][tu]), min_rings)
    mine = S.get_scaffold_metric(test_d, min_rings=min_rings)(gen_d)
    assert {k: mine[k] for k in want if k != "scaffold_class"} == {k: want[k] for k in want if k != "scaffold_class"}
    assert mine["n_generated"] == len(gu) < len(gen[1]) and 0.0 < mine["scaf"] < 1.0
    # order-free frameworks
    want = K.scaffold_metric(gen, test, min_rings, bond_orders=False)
    mine = S.get_scaffold_metric(test_d, min_rings=min_rings, unique=False, bond_orders=False)(gen_d)
    assert {k: mine[k] for k in want if k != "scaffold_class"} == {k: want[k] for k in want if k != "scaffold_class"}
    # a generated set of trees only
    trees = [dict(pos=p, type=t, fc=f, bond=b) for p, t, f, b in (SM.random_tree_molecule(np.random.default_rng(5), k) for k in (4, 9, 17))]
    none = fn(on(gpu_device, *SM.records(trees)))
    assert math.isnan(none["scaf"]) and none["with_scaffold_generated"] == 0 and none["scaffold_class"].cpu().tolist() == [-1] * 3 and none["mean_rings"] == 0.0


# ------------------------------------------------------------------------------------------------------------------ evaluation

def test_evaluate_reports_the_scaffolds(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.scaffold`` the 'structure' dict holds the
    entry, equal to the mirror on the run's records (one slot's record is replaced by its ground truth under another atom order: the same
    scaffold there); without the flag it has no such key."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K_, T = 2, 3
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=T)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K_
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:T].repeat_interleave(K_)
    planted = 1 * K_ + 1
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    moved = GM.permuted(SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])]), np.random.default_rng(13))
    gather, kept = shard.gather_by_slot, []

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        kept.append(by_slot)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert "scaffold" not in plain
    cfg.eval.scaffold = True
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"scaffold"}
    sc = st["scaffold"]
    assert set(sc) == {"scaf", "n_generated", "n_test", "with_scaffold_generated", "with_scaffold_test", "distinct_generated", "distinct_test", "shared",
                       "scaffold_class", "mean_rings", "same_scaffold", "min_rings"} and sc["min_rings"] == 2
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    gu, tu = K.unique_rows(gen_rec, gen_n), K.unique_rows(gt_rec, gt_n)
    want = K.scaffold_metric((gen_rec[gu], gen_n[gu]), (gt_rec[tu], gt_n[tu]), 2)
    same_float = lambda a, b: a == b or (a != a and b != b)
    assert all(sc[k] == want[k] for k in want if k not in ("scaffold_class", "scaf", "mean_rings")), (sc, want)
    assert same_float(sc["scaf"], want["scaf"]) and same_float(sc["mean_rings"], want["mean_rings"])
    assert same_partition(sc["scaffold_class"].cpu().tolist(), want["scaffold_class"])
    stated = [K.same_scaffold((gen_rec[p], gen_n[p]), (gt_rec[int(slot_ds[p])], gt_n[int(slot_ds[p])])) for p in range(T * K_)]
    same = sc["same_scaffold"]
    assert set(same) == {"same", "status", "rate", "undecided", "top_k"}
    assert same["same"].cpu().tolist() == [s for s, _ in stated] and same["status"].cpu().tolist() == [s for _, s in stated] and same["undecided"] == 0
    assert stated[planted] == (True, 0) and bool(same["same"][planted])
    n_ok = sum(s == 0 for _, s in stated)
    assert same["rate"] == (sum(v for v, s in stated if s == 0) / n_ok if n_ok else None)
    hits = [any(v for v, _ in stated[t * K_:(t + 1) * K_]) for t in range(T)]
    assert same["top_k"]["hit"].cpu().tolist() == hits and hits[1] and float(same["top_k"]["acc_at_k"]) == sum(hits) / T
