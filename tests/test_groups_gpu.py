"""GPU: ``dsg_group_records`` and ``dsg_group_similarity_records`` (csrc/ds_groups.hip) against the plain-Python mirror of tests/groups_mirror.py,
which is written from include/diffspectra_groups.h and pinned to hand-stated expectations by tests/test_groups_cpu.py.  Every output is an
integer or a byte and is compared exactly; there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

KEYS = ("groups", "aromatic_mask", "status")
PAIR_KEYS = ("common", "either", "groups", "status")
GUARD_ROWS = 3


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_rows(dev, rec, n):
    """``group_records`` as the mirror's list of row dicts."""
    out = [t.cpu() for t in E.group_records(*on(dev, rec, n))]
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.uint8] and all(t.shape == (len(n),) for t in out)
    groups, aromatic, status = (t.tolist() for t in out)
    return [dict(groups=groups[p], aromatic_mask=aromatic[p], status=status[p]) for p in range(len(status))]


def gpu_pairs(dev, prb, ref, ref_index=None):
    """``group_similarity_records`` as the mirror's list of row dicts; ``prb`` and ``ref`` are (rec, n) pairs of arrays."""
    idx = None if ref_index is None else to_dev(dev, ref_index, torch.int64)
    out = [t.cpu() for t in E.group_similarity_records(*on(dev, *prb), *on(dev, *ref), idx)]
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.uint8] and out[2].shape == (len(prb[1]), 2)
    common, either, groups, status = (t.tolist() for t in out)
    return [dict(common=common[p], either=either[p], groups=tuple(groups[p]), status=status[p]) for p in range(len(status))]


def same_rows(got, want, keys=KEYS):
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (p, {k: (g[k], w[k]) for k in keys if g[k] != w[k]})
    assert len(got) == len(want)


@pytest.fixture(scope="module")
def molecules():
    """The table, three renumberings of each of its molecules, the second Kekule drawings, the implicit-hydrogen cases, the 29-heavy-atom
    record and the derived set as one record table, with the mirror's rows: computed once, shared, never changed."""
    rows = G.hand_table()
    rng = np.random.default_rng(23)
    table = [mol for _, mol, _, _ in rows]
    renumbered = [GM.permuted(mol, rng) for mol in table for _ in range(3)]
    extra = list(G.other_kekule_drawings().values()) + [mol for _, mol in G.implicit_hydrogen_cases()] + [G.quaterphenyl_29()]
    derived = G.derived_set()
    rec, n = G.records_of(table)
    rec2, n2 = SM.records(renumbered + extra + derived)
    rec, n = np.concatenate([rec, rec2]), np.concatenate([n, n2])
    return dict(rows=rows, rec=rec, n=n, want=G.analyse_table(rec, n), derived=slice(len(n) - len(derived), len(n)))


# ------------------------------------------------------------------------------------------------------------------ molecules

def test_table_renumberings_and_derived_set_against_the_mirror(gpu_device, molecules):
    rows, rec, n, want = (molecules[k] for k in ("rows", "rec", "n", "want"))
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    # ... and so the hand-stated table holds for the kernel; a renumbering keeps the groups
    for k, (name, _, groups, aromatic) in enumerate(rows):
        assert G.names_of(got[k]["groups"]) == groups and got[k]["aromatic_mask"] == sum(1 << i for i in aromatic) and got[k]["status"] == 0, name
        assert all(got[len(rows) + 3 * k + j]["groups"] == got[k]["groups"] for j in range(3)), name
    # the ground the comparison stands on (asserted on the mirror in tests/test_groups_cpu.py)
    part = got[molecules["derived"]]
    assert len(part) >= 250 and sum(g["aromatic_mask"] != 0 for g in part) >= 40
    assert all(5 <= sum((g["groups"] >> bit) & 1 for g in part) <= len(part) - 5 for bit in range(15))


def test_sizes_malformed_and_dense_records(gpu_device):
    """n in {1, 2, 28, 29} and two clamped values, garbage in everything the contract says is ignored; the complete graph on 29 atoms with
    order-1 bytes and with random orders; a 29-atom chain; 29 heavy atoms without a hydrogen."""
    rng = np.random.default_rng(20261020)
    sizes = np.array([1, 2, 28, 29, 28, 29, 40, -3] * 40, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    want = G.analyse_table(rec, n)
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    assert {w["status"] for w in want} == {G.OK, G.UNUSABLE} and sum(w["groups"] != 0 for w in want) > 50
    assert gpu_rows(gpu_device, clean, n) == got                                 # what is ignored is ignored
    dense = GM.k29()
    heavy = dict(dense, bond=np.triu(rng.integers(1, 4, size=(29, 29)), 1))
    heavy["bond"] = heavy["bond"] + heavy["bond"].T
    sparse = [GM.random_molecule(rng, 29) for _ in range(20)]
    chain = GM.carbons(29, [(i, i + 1) for i in range(28)])
    rec, n = SM.records([dense, heavy, chain, G.quaterphenyl_29()] + sparse)
    rec[0, SM.BOND_END:] = 0xEE
    rec[0, SM.BOND:SM.BOND_END].reshape(29, 29)[np.tril_indices(29)] = 0xEE      # garbage in the lower triangle and on the diagonal
    want = G.analyse_table(rec, n)
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    assert got[0] == dict(groups=0, aromatic_mask=0, status=0) and got[1]["status"] == 0
    assert G.names_of(got[2]["groups"]) == {"alkane"} and got[3]["aromatic_mask"] == (1 << 24) - 1


def test_every_kind_of_unusable_record(gpu_device, molecules):
    names = [name for name, _, _, _ in molecules["rows"]]
    k = names.index("anisole")
    base, n = np.repeat(molecules["rec"][k:k + 1], 7, axis=0), np.full(7, molecules["n"][k], np.int32)
    n[2] = 0
    base[0, SM.TYPE + 15] = 5                                                   # a type byte above 4 (the last atom)
    base[1, SM.BOND + 3 * 29 + 12] = 4                                          # a bond byte above 3, upper triangle
    n[3] = -7                                                                   # clamped to 0
    base[4, SM.BOND + 12 * 29 + 3] = 4                                          # the same pair in the lower triangle: not looked at
    base[5, SM.BOND + 28 * 29 + 28] = 9                                         # the diagonal: not looked at
    base[6, SM.TYPE + 16] = 77                                                  # an atom >= n: not looked at
    base[6, SM.BOND + 2 * 29 + 20] = 200
    got = gpu_rows(gpu_device, base, n)
    zero = dict(groups=0, aromatic_mask=0, status=G.UNUSABLE)
    assert got[:4] == [zero] * 4 and got[4:] == [molecules["want"][k]] * 3 and got == G.analyse_table(base, n)


# ------------------------------------------------------------------------------------------------------------------ pairs

def test_pairs_identity_repeats_and_rows_outside_the_table(gpu_device, molecules):
    rec, n, want = (molecules[k] for k in ("rec", "n", "want"))
    P = 200
    rng = np.random.default_rng(31)
    prb_rows, ref_rows = rng.permutation(len(n))[:P], rng.permutation(len(n))[:P]
    prb, ref = (rec[prb_rows].copy(), n[prb_rows].copy()), (rec[ref_rows].copy(), n[ref_rows].copy())
    prb[1][[5, 77]] = 0                                                          # unusable on one side, on the other, on both
    ref[1][[9, 77]] = 0
    pair = lambda p, r: G.similarity_pair(G.analyse(prb[0][p], prb[1][p]), G.analyse(ref[0][r], ref[1][r]))
    # identity pairing: pair p reads ground-truth row p
    got = gpu_pairs(gpu_device, prb, ref)
    same_rows(got, [pair(p, p) for p in range(P)], PAIR_KEYS)
    assert [got[p]["status"] for p in (5, 9, 77)] == [G.UNUSABLE] * 3 and got[5] == dict(common=-1, either=-1, groups=(0, 0), status=G.UNUSABLE)
    assert len({g["either"] for g in got}) > 4 and any(g["common"] == g["either"] > 0 for g in got) and any(g["common"] == 0 < g["either"] for g in got)
    # ref_index with repeats (K candidates share a row) against a shorter table, and rows outside it: the ground-truth table lies between
    # guard rows of 0xFF bytes with guard counts of 29 - a read of a neighbouring row would find type bytes above 4 and answer UNUSABLE
    M = 50
    index = np.repeat(rng.integers(0, M, size=P // 4), 4).astype(np.int64)
    index[[3, 50, 51, 120]] = [-1, M, 2 ** 40, -2 ** 33]
    g_rec = np.full((M + 2, SM.RECORD_BYTES), 0xFF, np.uint8)
    g_n = np.full(M + 2, 29, np.int32)
    g_rec[1:M + 1], g_n[1:M + 1] = ref[0][:M], ref[1][:M]
    rec_d, n_d = on(gpu_device, g_rec, g_n)
    out = [t.cpu() for t in E.group_similarity_records(*on(gpu_device, *prb), rec_d[1:M + 1], n_d[1:M + 1], to_dev(gpu_device, index, torch.int64))]
    got = [dict(common=int(out[0][p]), either=int(out[1][p]), groups=tuple(out[2][p].tolist()), status=int(out[3][p])) for p in range(P)]
    want_rows = G.similarity_table(prb[0], prb[1], ref[0][:M], ref[1][:M], index)
    same_rows(got, want_rows, PAIR_KEYS)
    assert [got[p] for p in (3, 50, 51, 120)] == [dict(common=-1, either=-1, groups=(0, 0), status=G.INVALID)] * 4
    # M = 0 with a ref_index: every pair is invalid and nothing is read; P = 0
    none = gpu_pairs(gpu_device, (prb[0][:3], prb[1][:3]), (ref[0][:0], ref[1][:0]), np.zeros(3, np.int64))
    assert [g["status"] for g in none] == [G.INVALID] * 3 and all(g["common"] == g["either"] == -1 for g in none)
    assert gpu_pairs(gpu_device, (prb[0][:0], prb[1][:0]), ref) == [] and gpu_rows(gpu_device, rec[:0], n[:0]) == []


def test_guarded_outputs_repeat_runs_and_batch_independence(gpu_device, molecules):
    """Every output between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record); two runs
    bit-identical; a row's outputs do not depend on the batch around it."""
    rng = np.random.default_rng(9)
    P = 65
    rows = rng.permutation(len(molecules["n"]))[:P]
    rec_d, n_d = on(gpu_device, molecules["rec"][rows], molecules["n"][rows])
    ref_d, m_d = on(gpu_device, molecules["rec"][rows[::-1]], molecules["n"][rows[::-1]])
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(width, dtype):
        raw = torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + P]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    bufs = [guarded(4, torch.int32), guarded(4, torch.int32), guarded(1, torch.uint8)]
    st = lib.dsg_group_records(rec_d.data_ptr(), n_d.data_ptr(), P, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    plain, again = E.group_records(rec_d, n_d), E.group_records(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
    bufs = [guarded(4, torch.int32), guarded(4, torch.int32), guarded(8, torch.int32), guarded(1, torch.uint8)]
    st = lib.dsg_group_similarity_records(rec_d.data_ptr(), n_d.data_ptr(), P, ref_d.data_ptr(), m_d.data_ptr(), P, None,
                                          *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    p_plain, p_again = E.group_similarity_records(rec_d, n_d, ref_d, m_d), E.group_similarity_records(rec_d, n_d, ref_d, m_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, p_plain, p_again))
    assert torch.equal(p_plain[2][:, 0], plain[0]) and int((p_plain[3] == 0).sum()) == P
    # rows 64, 5 and 17 alone, and in another order
    for sub in ([64], [5], [17, 64, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        alone = E.group_records(rec_d[idx].contiguous(), n_d[idx].contiguous())
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
        alone = E.group_similarity_records(rec_d[idx].contiguous(), n_d[idx].contiguous(), ref_d, m_d, idx)
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, p_plain))


# ------------------------------------------------------------------------------------------------------------------ the public interface

def test_public_interface_against_the_mirror(gpu_device, molecules):
    rows, rec, n, want = (molecules[k] for k in ("rows", "rec", "n", "want"))
    names = [name for name, _, _, _ in rows]
    rec_d, n_d = on(gpu_device, rec, n)
    fg = S.functional_groups(rec_d, n.tolist())
    assert isinstance(fg, S.FunctionalGroups) and fg.groups.device.type == "cuda" and bool(fg.usable.all())
    assert fg.groups.cpu().tolist() == [w["groups"] for w in want] and fg.aromatic_mask.cpu().tolist() == [w["aromatic_mask"] for w in want]
    assert fg.names(names.index("methyl acetate")) == ("alkane", "ether", "ester")
    for name in ("arene", "amide", "thiol"):
        assert fg.present(name).cpu().tolist() == [name in G.names_of(w["groups"]) for w in want]
    # K = 4 candidates for each of 30 targets, one candidate unusable and one row outside the table
    K, T = 4, 30
    rng = np.random.default_rng(37)
    cand = rng.permutation(len(n))[:T * K]
    targets = np.repeat(rng.integers(0, len(rows), size=T), K).astype(np.int64)
    prb_n = n[cand].copy()
    prb_n[6] = 0
    targets[[9, 40, 41, 42, 43]] = [-1, len(n)] + [-5] * 3                       # the eleventh target has no valid candidate
    out = S.functional_group_similarity_batch((rec_d, n_d), (rec_d[to_dev(gpu_device, cand, torch.int64)].contiguous(), prb_n), ref_index=targets)
    assert isinstance(out, S.GroupSimilarity) and out.similarity.dtype == torch.float64 and out.similarity.device.type == "cuda"
    want_rows = G.similarity_table(rec[cand], prb_n, rec, n, targets)
    got = [dict(common=c, either=e, groups=tuple(g), status=s) for c, e, g, s in zip(out.common.tolist(), out.either.tolist(), out.groups.tolist(), out.status.tolist())]
    same_rows(got, want_rows, PAIR_KEYS)
    sim = out.similarity.cpu().numpy()
    ok = np.array([w["status"] == 0 for w in want_rows])
    assert np.array_equal(sim[ok], np.array([G.jaccard(w) for w in want_rows])[ok]) and np.isnan(sim[~ok]).all() and (~ok).sum() == 6
    assert out.valid.cpu().tolist() == ok.tolist()
    top = S.topk_groups(out.similarity, out.status, K)
    filled = np.where(ok, sim, -np.inf).reshape(T, K)
    best = filled.max(1)
    assert np.array_equal(top["best"].cpu().numpy()[best > -np.inf], best[best > -np.inf]) and np.isnan(top["best"].cpu().numpy()[10])
    assert top["best_index"].cpu().tolist() == [int(np.argmax(r)) if np.isfinite(r.max()) else -1 for r in filled]
    assert abs(float(top["mean_best"]) - float(best[best > -np.inf].sum()) / (T - 1)) <= 1e-12      # a torch fp64 sum of 29 values in [0, 1]: its order is torch's
    # hand-stated: water against formamide, ethanol against dimethyl ether, benzene against benzene
    pick = lambda *ns: to_dev(gpu_device, [names.index(x) for x in ns], torch.int64)
    hand = S.functional_group_similarity_batch((rec_d, n_d), (rec_d[pick("water", "ethanol", "benzene")].contiguous(), n_d[pick("water", "ethanol", "benzene")]),
                                               ref_index=pick("formamide", "dimethyl ether", "benzene"))
    assert hand.similarity.cpu().tolist() == [1.0, 1 / 3, 1.0]


def test_evaluate_reports_the_functional_groups(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.functional_groups`` the 'structure' dict
    holds the entry, equal to the mirror on the run's records (one slot's record is replaced by its ground truth under another atom order:
    similarity 1 there); without the flag it has no such key."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K, T = 2, 3
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=T)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:T].repeat_interleave(K)
    planted = 1 * K + 1
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
    assert "functional_groups" not in plain
    cfg.eval.functional_groups = True
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"functional_groups"}
    fg = st["functional_groups"]
    assert set(fg) == {"similarity", "status", "mean", "undefined", "presence_rate", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    want = G.similarity_table(gen_rec, gen_n, gt_rec, gt_n, slot_ds.numpy())
    ok = np.array([w["status"] == 0 for w in want])
    sim = fg["similarity"].cpu().numpy()
    assert fg["status"].cpu().tolist() == [w["status"] for w in want] and fg["undefined"] == int((~ok).sum())
    assert np.array_equal(sim[ok], np.array([G.jaccard(w) for w in want])[ok]) and np.isnan(sim[~ok]).all()
    assert bool(ok[planted]) and sim[planted] == 1.0
    total = 0.0
    for v in sim[ok].tolist():
        total += v
    assert fg["mean"] == total / int(ok.sum())
    assert fg["presence_rate"] == {name: sum((w["groups"][0] >> g) & 1 for w in want) / (T * K) for g, name in enumerate(G.NAMES)}
    direct = S.topk_groups(fg["similarity"], fg["status"], K)
    same = lambda a, b: torch.allclose(a.double(), b.double(), rtol=0.0, atol=0.0, equal_nan=True)      # NaN where a target has no ok candidate
    assert all(same(fg["top_k"][k], direct[k]) for k in ("best", "best_index", "mean_best"))
    assert float(fg["top_k"]["best"][1]) == 1.0
