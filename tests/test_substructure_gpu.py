"""GPU: ``dsq_match_records`` (csrc/ds_substructure.hip) against the plain-Python mirror of tests/substructure_mirror.py, which is written from
include/diffspectra_substructure.h and pinned to hand-stated expectations by tests/test_substructure_cpu.py.  Every output is an integer or a
byte and is compared exactly, truncated entries included; there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, maccs, shard, smarts, structure_metrics as S
from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM, substructure_mirror as M
from tests.helpers import to_dev
from tests.test_substructure_cpu import GROUP_PATTERNS
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
WAVES = E.SUBSTRUCTURE_CONSTS["DSQ_WAVES"]
SMALL = list(GROUP_PATTERNS.values()) + ["*", "*~*", "[#1]", "*@*", "*!@*", "[!+0]", "*1~*~*~1", "*~*(~*)~*", "[#7,#8;!H0]~*=*", "*:*"]


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_arrays(dev, rec, n, words, max_nodes=M.DEFAULT_NODES):
    """``substructure_records`` as the seven numpy arrays of ``substructure_mirror.as_arrays``."""
    out = [t.cpu() for t in E.substructure_records(*on(dev, rec, n), to_dev(dev, words, torch.int32), max_nodes)]
    P, K = len(n), len(words)
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(P, K)] * 3 + [(P,)] * 4
    return tuple(t.numpy() for t in out)


NAMES = ("count", "anchors", "cover", "aromatic_mask", "aromatic_rings", "fragments", "status")


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert bad.size == 0, (name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.fixture(scope="module")
def molecules():
    """The hand-stated MACCS table, the functional-group table, the second Kekule drawings, the implicit-hydrogen cases, the 29-heavy-atom
    record and the derived set as one record table, with the mirror's arrays over the whole MACCS table: computed once, shared, never changed."""
    rows = M.maccs_table()
    extra = [mol for _, mol, _, _ in G.hand_table()] + list(G.other_kekule_drawings().values()) + [mol for _, mol in G.implicit_hydrogen_cases()]
    extra += list(M.oxygen_cases()) + [G.quaterphenyl_29()]
    derived = G.derived_set()
    rec, n = G.records_of([mol for _, mol, _ in rows])
    rec2, n2 = SM.records(extra + derived)
    rec, n = np.concatenate([rec, rec2]), np.concatenate([n, n2])
    want = M.analyse_table(rec, n, M.MACCS_WORDS)
    return dict(rows=rows, rec=rec, n=n, want_rows=want, want=M.as_arrays(want, len(M.MACCS_WORDS)), big=len(rows) + len(extra) - 1)


# ------------------------------------------------------------------------------------------------------------------ kernel = mirror

def test_tables_and_derived_set_against_the_mirror(gpu_device, molecules):
    rows, rec, n, want = (molecules[k] for k in ("rows", "rec", "n", "want"))
    got = gpu_arrays(gpu_device, rec, n, M.MACCS_WORDS)
    same(got, want)
    assert len(n) >= 350 and not (got[0] & M.TRUNCATED).any() and (got[6] == 0).all()
    # ... and so the hand-stated MACCS sets hold for the kernel
    for p, (name, _, keys) in enumerate(rows):
        row = dict(count=got[0][p].tolist(), anchors=got[1][p].tolist(), aromatic_rings=int(got[4][p]), fragments=int(got[5][p]))
        assert M.maccs_of(row)[0] == keys, name
    assert got[3][molecules["big"]] == (1 << 24) - 1 and got[4][molecules["big"]] == 4                       # quaterphenyl: 24 aromatic atoms, 4 rings
    assert len(np.unique(got[0])) == 5 and (got[0] > 0).any(axis=0).sum() >= 100                               # every count 0..4; most patterns occur


def test_k29_truncated_results_are_bit_identical(gpu_device):
    """The budget case of the CPU test: the complete graph on 29 carbons, the 14-atom and the 8-atom cycle, budgets 12, 13 and 500."""
    rec, n = SM.records([GM.k29(), G.quaterphenyl_29()])
    words = smarts.compile_patterns([maccs._cycle(14), "[#7]", maccs._cycle(8), "*~*~*~*~*~*"])
    everyone = (1 << 29) - 1
    for budget in (12, 13, 500):
        got = gpu_arrays(gpu_device, rec, n, words, budget)
        same(got, M.as_arrays(M.analyse_table(rec, n, words, budget), len(words)))
        assert got[0][0].tolist()[:3] == [M.TRUNCATED | (0 if budget == 12 else 4), 0, M.TRUNCATED | 4]
        assert got[1][0][0] == got[2][0][0] == (0 if budget == 12 else everyone)
    one = gpu_arrays(gpu_device, rec, n, words, 1)
    same(one, M.as_arrays(M.analyse_table(rec, n, words, 1), len(words)))


def test_sizes_malformed_and_dense_records(gpu_device):
    """n in {1, 2, 28, 29} and two clamped values, random types, charges and bond bytes at three densities, garbage in everything the contract
    says is ignored; small patterns under a small budget, so truncated entries are compared too."""
    rng = np.random.default_rng(20261020)
    sizes = np.array([1, 2, 28, 29, 28, 29, 40, -3] * 12, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    words = smarts.compile_patterns(SMALL)
    want = M.as_arrays(M.analyse_table(rec, n, words, 300), len(words))
    got = gpu_arrays(gpu_device, rec, n, words, 300)
    same(got, want)
    assert set(want[6].tolist()) == {M.OK, M.UNUSABLE} and (want[0] & M.TRUNCATED).any() and ((want[0] & M.TRUNCATED) == 0).any()
    same(gpu_arrays(gpu_device, clean, n, words, 300), got)                       # what is ignored is ignored


def test_every_kind_of_unusable_record(gpu_device, molecules):
    names = [name for name, _, _ in molecules["rows"]]
    k = names.index("fluorene")
    base, n = np.repeat(molecules["rec"][k:k + 1], 7, axis=0), np.full(7, molecules["n"][k], np.int32)
    n[2] = 0
    base[0, SM.TYPE + 15] = 5                                                   # a type byte above 4
    base[1, SM.BOND + 3 * 29 + 12] = 4                                          # a bond byte above 3, upper triangle
    n[3] = -7                                                                   # clamped to 0
    base[4, SM.BOND + 12 * 29 + 3] = 4                                          # the same pair in the lower triangle: not looked at
    base[5, SM.BOND + 28 * 29 + 28] = 9                                         # the diagonal: not looked at
    base[6, SM.TYPE + 24] = 77                                                  # an atom >= n: not looked at
    base[6, SM.BOND + 2 * 29 + 25] = 200
    got = gpu_arrays(gpu_device, base, n, M.MACCS_WORDS)
    same(got, M.as_arrays(M.analyse_table(base, n, M.MACCS_WORDS), len(M.MACCS_WORDS)))
    assert all((a[:4] == 0).all() for a in got[:6]) and got[6].tolist() == [2, 2, 2, 2, 0, 0, 0]
    for a, w in zip(got, molecules["want"]):
        assert all(np.array_equal(a[p], w[k]) for p in (4, 5, 6))


def test_malformed_patterns_match_nothing(gpu_device, molecules):
    good = smarts.compile_pattern("*1~*~*~*~*~*~1").astype(np.int64)
    cases = [good]
    for word, value in ((0, 0), (0, 15), (0, 6 | (3 << 8)), (0, 255 | (255 << 8)), (17, 2 | 0xFF00), (17, 200 | 0xFF00), (29, 5 | (5 << 8) | (0xFF << 16)),
                        (29, 3 | (2 << 8) | (0xFF << 16)), (29, 0 | (6 << 8) | (0xFF << 16)), (29, 0 | (77 << 8) | (0xFF << 16))):
        w = good.copy()
        w[word] = value
        cases.append(w)
    cases += [np.full(32, -1, np.int64), np.zeros(32, np.int64), good]
    words = np.stack(cases).astype(np.int32)
    rec, n = molecules["rec"][:40], molecules["n"][:40]
    got = gpu_arrays(gpu_device, rec, n, words)
    same(got, M.as_arrays(M.analyse_table(rec, n, words), len(words)))
    assert (got[0][:, 1:-1] == 0).all() and (got[1][:, 1:-1] == 0).all() and (got[2][:, 1:-1] == 0).all()
    assert np.array_equal(got[0][:, 0], got[0][:, -1]) and got[0][:, 0].sum() >= 5                          # the well-formed one before and after them


def test_table_sizes_guards_and_batch_independence(gpu_device, molecules):
    """P = 1, 5 and 4 w + 1 (w waves per workgroup: the last workgroup has w - 1 waves without a record): every output lies between guard rows
    that stay untouched, and every row equals the same record run alone."""
    rng = np.random.default_rng(9)
    words = to_dev(gpu_device, M.MACCS_WORDS, torch.int32)
    K = words.shape[0]
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    alone = {}
    for P in (1, 5, 4 * WAVES + 1):
        pick = rng.permutation(len(molecules["n"]))[:P]
        rec_d, n_d = on(gpu_device, molecules["rec"][pick], molecules["n"][pick])

        def guarded(width, dtype):
            raw = torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
            return raw, raw[GUARD_ROWS:GUARD_ROWS + P]
        bufs = [guarded(K, torch.uint8), guarded(4 * K, torch.int32), guarded(4 * K, torch.int32), guarded(4, torch.int32), guarded(4, torch.int32),
                guarded(4, torch.int32), guarded(1, torch.uint8)]
        st = lib.dsq_match_records(rec_d.data_ptr(), n_d.data_ptr(), P, words.data_ptr(), K, M.DEFAULT_NODES, *(view.data_ptr() for _, view in bufs), stream)
        torch.cuda.synchronize()
        assert st == 0
        for raw, _ in bufs:
            b = raw.view(torch.uint8)
            assert bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
        for name, (_, view), w in zip(NAMES, bufs, molecules["want"]):
            assert np.array_equal(view.cpu().numpy().reshape(w[pick].shape), w[pick]), (P, name)
        for p in pick[:3]:                                                       # the same record alone
            if int(p) not in alone:
                alone[int(p)] = gpu_arrays(gpu_device, molecules["rec"][p:p + 1], molecules["n"][p:p + 1], M.MACCS_WORDS)
            for a, w in zip(alone[int(p)], molecules["want"]):
                assert np.array_equal(a[0], w[p])


def test_pattern_counts_0_1_and_256(gpu_device, molecules):
    rec, n = molecules["rec"][:60], molecules["n"][:60]
    none = gpu_arrays(gpu_device, rec, n, np.zeros((0, 32), np.int32))
    for a, w in zip(none[3:], molecules["want"][3:]):
        assert np.array_equal(a, w[:60])                                         # K = 0: the per-record outputs are still written
    single = gpu_arrays(gpu_device, rec, n, M.MACCS_WORDS[7:8])
    assert all(np.array_equal(a[:, 0], w[:60, 7]) for a, w in zip(single[:3], molecules["want"][:3]))
    many = np.concatenate([M.MACCS_WORDS, M.MACCS_WORDS])[:256]
    assert len(many) == 256 and len(M.MACCS_WORDS) >= 128
    full = gpu_arrays(gpu_device, rec, n, many)
    K = len(M.MACCS_WORDS)
    for a, w in zip(full[:3], molecules["want"][:3]):
        assert np.array_equal(a[:, :K], w[:60]) and np.array_equal(a[:, K:], w[:60, :256 - K])
    with pytest.raises(ValueError, match="at most 256"):
        E.substructure_records(*on(gpu_device, rec, n), to_dev(gpu_device, np.concatenate([many, many[:1]]), torch.int32))
    assert all(t.shape[0] == 0 for t in E.substructure_records(*on(gpu_device, rec[:0], n[:0]), to_dev(gpu_device, many, torch.int32)))


# ------------------------------------------------------------------------------------------------------------------ cross-checks

def test_aromatic_atoms_and_fragments_agree_with_the_other_kernels(gpu_device, molecules):
    """On every test record - the tables, the derived set, random records with garbage, the dense ones - ``aromatic_mask`` is that of
    ``dsg_group_records`` and ``fragments`` the fragment count of ``valence_batch``."""
    rng = np.random.default_rng(5)
    r2, n2, _ = random_records(rng, 96, garbage=True)
    r3, n3 = SM.records([GM.k29(), GM.carbons(29, [(i, i + 1) for i in range(28)])] + [GM.random_molecule(rng, 29) for _ in range(10)])
    rec, n = np.concatenate([molecules["rec"], r2, r3]), np.concatenate([molecules["n"], n2, n3])
    rec_d, n_d = on(gpu_device, rec, n)
    found = S.substructure_search(rec_d, n_d, [])
    groups = S.functional_groups(rec_d, n_d)
    assert torch.equal(found.aromatic_mask, groups.aromatic_mask) and int((found.aromatic_mask != 0).sum()) >= 60
    usable = found.status == 0
    assert torch.equal(usable, groups.status == 0) and 0 < int(usable.sum()) < len(n)
    valence = S.valence_batch(rec_d, n_d)
    assert torch.equal(found.fragments[usable], valence.summary[usable][:, 2]) and int((found.fragments > 1).sum()) >= 20
    assert bool((found.fragments[~usable] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ similarity, interface

def test_maccs_similarity_with_and_without_ref_index(gpu_device, molecules):
    rec, n, want_rows = (molecules[k] for k in ("rec", "n", "want_rows"))
    keys = [M.maccs_of(row)[0] for row in want_rows]
    rec_d, n_d = on(gpu_device, rec, n)
    mk = S.maccs_keys(rec_d, n.tolist())
    assert isinstance(mk, S.MaccsKeys) and mk.bits.device.type == "cuda" and mk.bits.shape == (len(n), 167) and not bool(mk.truncated.any())
    assert [set(np.nonzero(row)[0].tolist()) for row in mk.bits.cpu().numpy()] == keys
    P = 120
    rng = np.random.default_rng(31)
    prb_rows, ref_rows = rng.permutation(len(n))[:P], rng.permutation(len(n))[:P]
    prb_n, ref_n = n[prb_rows].copy(), n[ref_rows].copy()
    prb_n[[5, 77]] = 0
    ref_n[[9, 77]] = 0
    prb_d, ref_d = on(gpu_device, rec[prb_rows], prb_n), on(gpu_device, rec[ref_rows], ref_n)

    def check(out, index, M_rows):
        assert isinstance(out, S.MaccsSimilarity) and out.tanimoto.dtype == torch.float64 and out.tanimoto.device.type == "cuda"
        common, either, sim, status, cut = (t.cpu().tolist() for t in out)
        assert not any(cut)
        for p in range(P):
            r = int(index[p])
            if not 0 <= r < M_rows:
                assert (common[p], either[p], status[p]) == (-1, -1, M.INVALID) and sim[p] != sim[p], p
            elif prb_n[p] == 0 or ref_n[r] == 0:
                assert (common[p], either[p], status[p]) == (-1, -1, M.UNUSABLE) and sim[p] != sim[p], p
            else:
                a, b = keys[prb_rows[p]], keys[ref_rows[r]]
                assert (common[p], either[p], status[p]) == (len(a & b), len(a | b), M.OK), p
                assert sim[p] == (1.0 if not a | b else len(a & b) / len(a | b)), p                          # Python's division
    check(S.maccs_similarity_batch(*prb_d, *ref_d), np.arange(P), P)
    Mr = 50
    index = np.repeat(rng.integers(0, Mr, size=P // 4), 4).astype(np.int64)
    index[[3, 50, 51, 110]] = [-1, Mr, 2 ** 40, -2 ** 33]
    out = S.maccs_similarity_batch(*prb_d, ref_d[0][:Mr].contiguous(), ref_d[1][:Mr].contiguous(), ref_index=index)
    check(out, index, Mr)
    assert len(set(out.either.cpu().tolist())) > 6 and int((out.status == 3).sum()) == 4
    top = S.topk_maccs(out.tanimoto, out.status, 4)
    sim = out.tanimoto.cpu().numpy().reshape(-1, 4)
    best = np.where(np.isnan(sim), -np.inf, sim).max(axis=1)                                                 # a target may have no ok candidate: NaN
    assert np.array_equal(top["best"].cpu().numpy(), np.where(best == -np.inf, np.nan, best), equal_nan=True)
    none = S.maccs_similarity_batch(prb_d[0][:3].contiguous(), prb_d[1][:3].contiguous(), ref_d[0][:0].contiguous(), ref_d[1][:0].contiguous(), ref_index=np.zeros(3, np.int64))
    assert none.status.cpu().tolist() == [3, 3, 3] and none.common.cpu().tolist() == [-1] * 3                # M = 0: nothing is read


def test_public_search_from_text(gpu_device, molecules):
    rows = molecules["rows"]
    names = [name for name, _, _ in rows]
    rec_d, n_d = on(gpu_device, molecules["rec"][:len(rows)], molecules["n"][:len(rows)])
    found = S.substructure_search(rec_d, n_d, ["c-c", "c-@c", "[OH]", "[#8]"])
    assert found.has(0).cpu().tolist() == [name in ("biphenyl", "fluorene") for name in names]
    assert found.has(1).cpu().tolist() == [name == "fluorene" for name in names]
    assert found.count[names.index("ethylene glycol")].cpu().tolist() == [0, 0, 2, 2] and found.anchors[names.index("ethanol"), 3].item() == 0b100
    assert not bool(found.truncated.any()) and found.cover[names.index("biphenyl"), 0].item() == (1 << 0) | (1 << 6)


def test_two_launches_give_identical_bytes(gpu_device, molecules):
    rec_d, n_d = on(gpu_device, molecules["rec"], molecules["n"])
    words = to_dev(gpu_device, M.MACCS_WORDS, torch.int32)
    first, second = E.substructure_records(rec_d, n_d, words), E.substructure_records(rec_d, n_d, words)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    k29 = on(gpu_device, *SM.records([GM.k29()] * 5))
    cut = smarts.compile_patterns([maccs._cycle(14), maccs._cycle(9)])
    first, second = (E.substructure_records(*k29, to_dev(gpu_device, cut, torch.int32), 500) for _ in range(2))
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(bool((a == a[:1]).all()) for a in first)


def test_evaluate_reports_the_maccs_similarity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.maccs`` the 'structure' dict holds the
    entry, equal to the mirror on the run's records (one slot's record is replaced by its ground truth under another atom order: similarity 1
    there).  One run: that the key is absent without the flag is checked on the CPU."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K, T, BUDGET = 2, 3, 256
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
    cfg.eval.maccs, cfg.eval.maccs_max_nodes = True, BUDGET                     # filler weights draw dense graphs: a small budget keeps the mirror quick
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert "maccs" in st and "functional_groups" not in st                      # (absent without its flag: tests/test_substructure_cpu.py)
    mk = st["maccs"]
    assert set(mk) == {"tanimoto", "status", "mean", "scored", "truncated", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    mine = [M.maccs_row(r, k, BUDGET) for r, k in zip(gen_rec, gen_n)]
    theirs = [M.maccs_row(gt_rec[int(s)], gt_n[int(s)], BUDGET) for s in slot_ds]
    ok = np.array([a["status"] == 0 and b["status"] == 0 for a, b in zip(mine, theirs)])
    sim = mk["tanimoto"].cpu().numpy()
    assert mk["status"].cpu().tolist() == [0 if k else 2 for k in ok] and mk["scored"] == int(ok.sum())
    assert np.array_equal(sim[ok], np.array([M.tanimoto(a["keys"], b["keys"]) for a, b in zip(mine, theirs)])[ok]) and np.isnan(sim[~ok]).all()
    assert bool(ok[planted]) and sim[planted] == 1.0
    assert mk["truncated"] == sum(1 for a, b, k in zip(mine, theirs, ok) if k and (a["truncated"] or b["truncated"]))
    total = 0.0
    for v in sim[ok].tolist():
        total += v
    assert mk["mean"] == total / int(ok.sum())
    direct = S.topk_maccs(mk["tanimoto"], mk["status"], K)
    equal = lambda a, b: torch.allclose(a.double(), b.double(), rtol=0.0, atol=0.0, equal_nan=True)
    assert all(equal(mk["top_k"][k], direct[k]) for k in ("best", "best_index", "mean_best"))
    assert float(mk["top_k"]["best"][1]) == 1.0
