"""GPU: ``dsf_fraggle_fragmentations``, ``dsf_path_fingerprints`` and ``dsf_fraggle_similarity_records`` (csrc/ds_fraggle.hip) and what
``structure_metrics`` and ``evaluate`` build on them against the plain-Python mirror of tests/fraggle_mirror.py, which is written from
include/diffspectra_fraggle.h and pinned to hand-stated expectations by tests/test_fraggle_cpu.py.  Every output of the kernels is an integer
and is compared exactly; the one float, ``fraggle``, is the same Python expression on the same integers on both sides and is compared with
``==``."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import brics_mirror as B, fraggle_mirror as F, graph_mirror as GM, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
SMALL_BUDGET = 1500                       # for random records: bounds what the mirror enumerates


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def same_arrays(got, want, keys):
    assert len(got) == len(want) == len(keys)
    for key, g, w in zip(keys, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (key, g.shape, w.shape, g.dtype, w.dtype)
        rows = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert rows.size == 0, (key, rows[:5].tolist(), g[rows[0]].tolist()[:12], w[rows[0]].tolist()[:12])


FRAG_KEYS, FP_KEYS = ("rows", "summary", "status"), ("fp", "atom_bits", "count", "status")


def gpu_fragmentations(dev, rec, n, max_nodes=None):
    out = [t.cpu() for t in E.fraggle_fragmentations(*on(dev, rec, n), max_nodes)]
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(len(n), F.MAX_FRAGMENTATIONS, 4), (len(n), 4), (len(n),)]
    return [t.numpy() for t in out]


def gpu_fingerprints(dev, rec, n, max_nodes=None):
    out = [t.cpu() for t in E.path_fingerprints(*on(dev, rec, n), max_nodes)]
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(len(n), 32), (len(n), 29, 32), (len(n),), (len(n),)]
    return [t.numpy() for t in out]


def gpu_similarity(dev, prb, ref, ref_index=None, max_nodes=None):
    idx = None if ref_index is None else to_dev(dev, ref_index, torch.int64)
    out = [t.cpu() for t in E.fraggle_similarity_records(*on(dev, *prb), *on(dev, *ref), idx, max_nodes)]
    P = len(prb[1])
    assert [t.dtype for t in out] == [torch.int32] * 5 + [torch.uint8]
    assert [tuple(t.shape) for t in out] == [(P, 2), (P, 2), (P,), (P,), (P, 2), (P,)]
    return [t.numpy() for t in out]


@pytest.fixture(scope="module")
def molecules():
    """The table, three renumberings of each of its molecules (with the permutations) and the derived pairs as record tables, with the
    mirror's rows: computed once, shared, never changed."""
    rows = F.hand_table()
    rng = np.random.default_rng(29)
    table = [mol for _, mol, _ in rows]
    perms, renumbered = [], []
    for mol in table:
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))                            # new atom i is old atom perm[i]
            perms.append(perm)
            renumbered.append(B.renumbered(mol, perm))
    prb, ref = F.derived_pairs()
    t_rec, t_n = SM.records(table + renumbered)
    (p_rec, p_n), (r_rec, r_n) = SM.records(prb), SM.records(ref)
    return dict(rows=rows, perms=perms, table=(t_rec, t_n), prb=(p_rec, p_n), ref=(r_rec, r_n), want=F.similarity_table(p_rec, p_n, r_rec, r_n))


# ------------------------------------------------------------------------------------------------------------------ the kernels

def test_fragmentations_of_the_table_and_the_derived_set_against_the_mirror(gpu_device, molecules):
    rows, perms = molecules["rows"], molecules["perms"]
    rec, n = (np.concatenate([a, b]) for a, b in zip(molecules["table"], molecules["ref"]))
    got = gpu_fragmentations(gpu_device, rec, n)
    same_arrays(got, F.fragmentation_arrays(rec, n), FRAG_KEYS)
    # ... and so the hand-stated table holds for the kernel, under renumbering too
    T = len(rows)
    listed = lambda p: [tuple(r) for r in got[0][p].tolist() if r != [-1] * 4]
    for k, (name, mol, stated) in enumerate(rows):
        want = F.stated_rows(mol, stated)
        assert [r[:3] for r in listed(k)] == want[:F.MAX_FRAGMENTATIONS] and got[2][k] == F.OK, name
        assert got[1][k, 3] == len(want) | (F.TRUNCATED if len(want) > F.MAX_FRAGMENTATIONS else 0), name
        for j in range(3):
            p = T + 3 * k + j
            assert got[1][p].tolist() == got[1][k].tolist(), name
            if len(want) <= F.MAX_FRAGMENTATIONS:
                assert F.unpacked_rows(listed(p)) == F.moved_rows(stated, perms[3 * k + j]), name
    found = S.fraggle_fragmentations(*on(gpu_device, rec, n))
    assert isinstance(found, S.FraggleFragmentations) and found.rows.device.type == gpu_device.type
    assert found.n_fragmentations.cpu().tolist() == [int(v) & (F.TRUNCATED - 1) for v in got[1][:, 3]]
    assert found.truncated.cpu().tolist() == [bool(v & F.TRUNCATED) for v in got[1][:, 3]] and int(found.truncated.sum()) == 4


def test_fingerprints_of_the_table_and_the_derived_set_against_the_mirror(gpu_device, molecules):
    rec, n = (np.concatenate([a, b, c]) for a, b, c in zip(molecules["table"], molecules["prb"], molecules["ref"]))
    got = gpu_fingerprints(gpu_device, rec, n)
    same_arrays(got, F.fingerprint_arrays(rec, n), FP_KEYS)
    assert int(got[2].min()) >= 0 and int(got[2].max()) > 300 and not got[3].any()
    # a renumbering keeps the fingerprint and the count and moves the atom rows
    T = len(molecules["rows"])
    for k in range(T):
        for j in range(3):
            p, perm = T + 3 * k + j, molecules["perms"][3 * k + j]
            assert np.array_equal(got[0][p], got[0][k]) and got[2][p] == got[2][k]
            assert np.array_equal(got[1][p][:len(perm)], got[1][k][perm])
    found = S.path_fingerprints(*on(gpu_device, rec[:5], n[:5]))
    assert isinstance(found, S.PathFingerprints) and np.array_equal(found.fp.cpu().numpy(), got[0][:5])


def test_similarity_of_the_derived_pairs_and_the_table_against_the_mirror(gpu_device, molecules):
    want = molecules["want"]
    got = gpu_similarity(gpu_device, molecules["prb"], molecules["ref"])
    same_arrays(got, F.as_arrays(want), F.KEYS)
    # the ground the comparison stands on (asserted on the mirror in tests/test_fraggle_cpu.py)
    ok = got[5] == F.OK
    assert int(ok.sum()) >= 200 and int((got[3][ok] == 0).sum()) >= 40
    assert sum(F.better(tuple(m), tuple(p)) for m, p, f in zip(got[1].tolist(), got[0].tolist(), got[3]) if f > 0) >= 40
    assert sum(w["best_kind"] in (2, 3) for w in want) >= 20 and sum(w["ring_step"] for w in want) >= 20
    # every molecule of the table against itself and against its renumberings: 1 iff it has a fragmentation; the 29-atom chain has 291
    t_rec, t_n = molecules["table"]
    T = len(molecules["rows"])
    prb = (np.concatenate([t_rec[:T], t_rec[T:]]), np.concatenate([t_n[:T], t_n[T:]]))
    idx = np.concatenate([np.arange(T), np.repeat(np.arange(T), 3)])
    got = gpu_similarity(gpu_device, prb, (t_rec[:T], t_n[:T]), idx)
    rows = F.similarity_table(*prb, t_rec[:T], t_n[:T], idx)
    same_arrays(got, F.as_arrays(rows), F.KEYS)
    for p, row in enumerate(rows):
        stated = molecules["rows"][idx[p]][2]
        assert row["n_fragmentations"] == len(stated) and F.fraggle(row) == (1.0 if stated else 0.0)
    assert max(r["n_fragmentations"] for r in rows) == 291


def test_random_records_every_size_unusable_rows_and_rows_outside_the_table(gpu_device):
    rng = np.random.default_rng(20261021)
    sizes = np.array([0, 1, 3, 28, 29, 2, 40, -3, 9, 14] * 12, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    rec[7::10, SM.TYPE] = 9                                                       # a type byte above 4 in rows that are usable otherwise
    clean[7::10, SM.TYPE] = 9
    n[7::10] = 5
    frag = gpu_fragmentations(gpu_device, rec, n, SMALL_BUDGET)
    same_arrays(frag, F.fragmentation_arrays(rec, n, SMALL_BUDGET), FRAG_KEYS)
    same_arrays(gpu_fragmentations(gpu_device, clean, n, SMALL_BUDGET), frag, FRAG_KEYS)      # what is ignored is ignored
    fps = gpu_fingerprints(gpu_device, rec, n, SMALL_BUDGET)
    same_arrays(fps, F.fingerprint_arrays(rec, n, SMALL_BUDGET), FP_KEYS)
    same_arrays(gpu_fingerprints(gpu_device, clean, n, SMALL_BUDGET), fps, FP_KEYS)
    assert set(fps[3].tolist()) == {F.OK, F.UNDECIDED, F.UNUSABLE} and int((fps[3] == F.OK).sum()) >= 30
    assert (fps[2][fps[3] == F.UNDECIDED] == -1).all() and not fps[0][fps[3] != F.OK].any() and not fps[1][fps[3] != F.OK].any()
    assert (frag[0][frag[2] != F.OK] == -1).all() and not frag[1][frag[2] != F.OK].any() and np.array_equal(frag[2], fps[3])
    # pairs: every generated row against a row of a second table, some outside it, some through the same row
    M = 40
    ref_rec, ref_n, _ = random_records(rng, M, garbage=True, sizes=np.resize(np.array([9, 14, 3, 29, 1, 28, 12, 0], np.int32), M))
    idx = rng.integers(0, M, size=len(n)).astype(np.int64)
    idx[::11] = [-1, M, M + 5, -(2 ** 40), 2 ** 40, -1, M, -7, M + 1, M, -1][:len(idx[::11])]
    got = gpu_similarity(gpu_device, (rec, n), (ref_rec, ref_n), idx, SMALL_BUDGET)
    want = F.similarity_table(rec, n, ref_rec, ref_n, idx, SMALL_BUDGET)
    same_arrays(got, F.as_arrays(want), F.KEYS)
    assert set(got[5].tolist()) == {F.OK, F.UNDECIDED, F.UNUSABLE, F.INVALID} and int((got[5] == F.OK).sum()) >= 15
    bad = got[5] != F.OK
    assert (got[0][bad] == -1).all() and (got[1][bad] == -1).all() and (got[2][bad] == -1).all() and not got[3][bad].any() and not got[4][bad].any()
    same_arrays(gpu_similarity(gpu_device, (clean, n), (ref_rec, ref_n), idx, SMALL_BUDGET), got, F.KEYS)
    assert sum(w["n_fragmentations"] > 0 for w in want) >= 3
    # sparse molecules of 28 and 29 atoms with ring closures and charges, every other one with its hydrogens turned into carbons: against
    # themselves renumbered and against one another, 400 to 1100 bond sets each
    mols = []
    for k in range(5):
        mol = GM.random_molecule(rng, 28 + k % 2)
        if k % 2:
            mol["type"] = np.where(mol["type"] == 0, 1, mol["type"])
        mols.append(mol)
    ref = SM.records(mols)
    prb = SM.records([GM.permuted(m, rng) for m in mols] + mols[1:] + mols[:1])
    idx = np.concatenate([np.arange(5), np.arange(5)])
    got = gpu_similarity(gpu_device, prb, ref, idx)
    want = F.similarity_table(*prb, *ref, idx)
    same_arrays(got, F.as_arrays(want), F.KEYS)
    assert not got[5].any() and int(got[3].min()) >= 5 and [F.fraggle(w) for w in want[:5]] == [1.0] * 5 and max(F.fraggle(w) for w in want[5:]) < 1.0
    same_arrays(gpu_fingerprints(gpu_device, *ref), F.fingerprint_arrays(*ref), FP_KEYS)
    same_arrays(gpu_fragmentations(gpu_device, *ref), F.fragmentation_arrays(*ref), FRAG_KEYS)


def test_a_budget_one_below_the_count_makes_the_row_undecided_and_leaves_its_neighbours(gpu_device, molecules):
    names = [name for name, _, _ in molecules["rows"]]
    pick = [names.index(name) for name in ("n-hexane", "cubane", "1-propylindane", "toluene", "decalin")]
    rec, n = molecules["table"][0][pick], molecules["table"][1][pick]
    counts = gpu_fingerprints(gpu_device, rec, n)[2]
    assert counts.tolist() == [F.Mol(r, k).fingerprint(F.DEFAULT_NODES).count for r, k in zip(rec, n)] and counts[1] == counts.max()
    full = dict(frag=gpu_fragmentations(gpu_device, rec, n), fp=gpu_fingerprints(gpu_device, rec, n), sim=gpu_similarity(gpu_device, (rec, n), (rec, n)))
    exact, below = int(counts[1]), int(counts[1]) - 1
    for budget, status in ((exact, F.OK), (below, F.UNDECIDED)):
        frag, fp = gpu_fragmentations(gpu_device, rec, n, budget), gpu_fingerprints(gpu_device, rec, n, budget)
        sim = gpu_similarity(gpu_device, (rec, n), (rec, n), None, budget)
        same_arrays(frag, F.fragmentation_arrays(rec, n, budget), FRAG_KEYS)
        same_arrays(fp, F.fingerprint_arrays(rec, n, budget), FP_KEYS)
        same_arrays(sim, F.as_arrays(F.similarity_table(rec, n, rec, n, None, budget)), F.KEYS)
        assert frag[2].tolist() == fp[3].tolist() == sim[5].tolist() == [F.OK, status, F.OK, F.OK, F.OK]
        others = [0, 2, 3, 4]
        for got, whole in ((frag, full["frag"]), (fp, full["fp"]), (sim, full["sim"])):
            assert all(np.array_equal(g[others], w[others]) for g, w in zip(got, whole))
    assert (frag[0][1] == -1).all() and not frag[1][1].any() and fp[2][1] == -1 and not fp[0][1].any() and not fp[1][1].any()
    assert [a[1].tolist() for a in sim[:5]] == [[-1, -1], [-1, -1], -1, 0, [0, 0]]
    # the budget of the pair is that of its larger fingerprint, whichever side it is on
    small, large = (rec[3:4], n[3:4]), (rec[1:2], n[1:2])
    assert gpu_similarity(gpu_device, small, large, None, below)[5].tolist() == [F.UNDECIDED] == gpu_similarity(gpu_device, large, small, None, below)[5].tolist()
    assert gpu_similarity(gpu_device, small, large, None, exact)[5].tolist() == [F.OK]


def guarded(dev, count, width, dtype):
    raw = torch.full((count + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=dev).view(dtype)
    return raw, raw[GUARD_ROWS:GUARD_ROWS + count]


def intact(raw):
    b = raw.view(torch.uint8)
    return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())


def test_guarded_outputs_repeat_runs_and_batch_independence(gpu_device, molecules):
    """Every output of the three entry points between guard rows filled with a pattern; two runs bit-identical; a pair alone, first, last and
    among a few hundred gives the same row."""
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    (p_rec, p_n), (r_rec, r_n) = molecules["prb"], molecules["ref"]
    P = len(p_n)
    prb_d, ref_d = on(gpu_device, p_rec, p_n), on(gpu_device, r_rec, r_n)
    bufs = [guarded(gpu_device, P, 8, torch.int32), guarded(gpu_device, P, 8, torch.int32), guarded(gpu_device, P, 4, torch.int32),
            guarded(gpu_device, P, 4, torch.int32), guarded(gpu_device, P, 8, torch.int32), guarded(gpu_device, P, 1, torch.uint8)]
    st = lib.dsf_fraggle_similarity_records(prb_d[0].data_ptr(), prb_d[1].data_ptr(), P, ref_d[0].data_ptr(), ref_d[1].data_ptr(), P, None, F.DEFAULT_NODES,
                                            *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    plain, again = E.fraggle_similarity_records(*prb_d, *ref_d), E.fraggle_similarity_records(*prb_d, *ref_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
    same_arrays([t.cpu().numpy() for t in plain], F.as_arrays(molecules["want"]), F.KEYS)
    busy = int(plain[3].argmax())                                                 # the pair with the most fragmentations
    for sub in ([busy], [0], [P - 1], [busy, 0, P - 1], [P - 1, busy, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        alone = E.fraggle_similarity_records(prb_d[0][idx].contiguous(), prb_d[1][idx].contiguous(), ref_d[0][idx].contiguous(), ref_d[1][idx].contiguous())
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
    # the two single-table entry points: P = 65 records
    rec_d, n_d = ref_d[0][:65].contiguous(), ref_d[1][:65].contiguous()
    bufs = [guarded(gpu_device, 65, F.MAX_FRAGMENTATIONS * 16, torch.int32), guarded(gpu_device, 65, 16, torch.int32), guarded(gpu_device, 65, 1, torch.uint8)]
    st = lib.dsf_fraggle_fragmentations(rec_d.data_ptr(), n_d.data_ptr(), 65, F.DEFAULT_NODES, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    frag, frag_again = E.fraggle_fragmentations(rec_d, n_d), E.fraggle_fragmentations(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, frag, frag_again))
    bufs = [guarded(gpu_device, 65, 128, torch.int32), guarded(gpu_device, 65, 29 * 128, torch.int32), guarded(gpu_device, 65, 4, torch.int32),
            guarded(gpu_device, 65, 1, torch.uint8)]
    st = lib.dsf_path_fingerprints(rec_d.data_ptr(), n_d.data_ptr(), 65, F.DEFAULT_NODES, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    fp, fp_again = E.path_fingerprints(rec_d, n_d), E.path_fingerprints(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, fp, fp_again))
    for sub in ([64], [0], [17, 64, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        assert all(torch.equal(s, t[idx]) for s, t in zip(E.fraggle_fragmentations(rec_d[idx].contiguous(), n_d[idx].contiguous()), frag))
        assert all(torch.equal(s, t[idx]) for s, t in zip(E.path_fingerprints(rec_d[idx].contiguous(), n_d[idx].contiguous()), fp))
    # P = 0 launches nothing; the argument errors of the C entry points
    assert [t.shape[0] for t in E.fraggle_similarity_records(prb_d[0][:0], prb_d[1][:0], *ref_d)] == [0] * 6
    assert [t.shape[0] for t in E.fraggle_fragmentations(rec_d[:0], n_d[:0])] == [0] * 3 and [t.shape[0] for t in E.path_fingerprints(rec_d[:0], n_d[:0])] == [0] * 4
    out = [view.data_ptr() for _, view in bufs]
    assert lib.dsf_path_fingerprints(rec_d.data_ptr(), n_d.data_ptr(), 65, 0, *out, stream) == -1
    assert lib.dsf_path_fingerprints(rec_d.data_ptr(), n_d.data_ptr(), 65, F.MAX_NODES + 1, *out, stream) == -1
    assert lib.dsf_path_fingerprints(rec_d.data_ptr(), n_d.data_ptr(), -1, 10, *out, stream) == -1
    assert lib.dsf_path_fingerprints(None, None, 0, 10, None, None, None, None, stream) == 0
    assert lib.dsf_path_fingerprints(rec_d.data_ptr(), None, 65, 10, *out, stream) == -1
    assert lib.dsf_path_fingerprints(rec_d.data_ptr() + 1, n_d.data_ptr(), 64, 10, *out, stream) == -1
    assert lib.dsf_path_fingerprints(rec_d.data_ptr(), n_d.data_ptr(), 65, 10, out[0], None, out[2], out[3], stream) == -1
    torch.cuda.synchronize()
    assert all(intact(raw) for raw, _ in bufs) and all(torch.equal(view.reshape(t.shape), t) for (_, view), t in zip(bufs, fp))


def test_a_shared_ground_truth_row_with_three_candidates(gpu_device, molecules):
    (p_rec, p_n), (r_rec, r_n) = molecules["prb"], molecules["ref"]
    # derived_pairs lists three generated molecules per ground truth for the first groups: keep one ground-truth row per group
    groups = 40
    rows = np.arange(0, 3 * groups, 3)
    assert all(np.array_equal(r_rec[r], r_rec[r + 1]) and np.array_equal(r_rec[r], r_rec[r + 2]) for r in rows)
    idx = np.repeat(np.arange(groups), 3).astype(np.int64)
    got = gpu_similarity(gpu_device, (p_rec[:3 * groups], p_n[:3 * groups]), (r_rec[rows], r_n[rows]), idx)
    same_arrays(got, F.as_arrays(molecules["want"][:3 * groups]), F.KEYS)


# ------------------------------------------------------------------------------------------------------------------ the public interface

def test_similarity_batch_and_topk_against_the_mirror(gpu_device, molecules):
    (p_rec, p_n), (r_rec, r_n), want = molecules["prb"], molecules["ref"], molecules["want"]
    K, groups = 3, 60
    rows = np.arange(0, K * groups, K)
    idx = np.repeat(np.arange(groups), K).astype(np.int64)
    idx[7] = groups + 3                                                           # one candidate without a ground truth
    prb_d = to_dev(gpu_device, p_rec[:K * groups], torch.uint8)
    alike = S.fraggle_similarity_batch(prb_d, p_n[:K * groups].tolist(), to_dev(gpu_device, r_rec[rows], torch.uint8), r_n[rows], ref_index=idx)
    assert isinstance(alike, S.FraggleSimilarity) and alike.fraggle.dtype == torch.float64 and alike.fraggle.device.type == gpu_device.type
    stated = [dict(F.NOT_OK, status=F.INVALID) if p == 7 else want[p] for p in range(K * groups)]
    same_float = lambda a, b: a == b or (a != a and b != b)
    value = [F.fraggle(r) for r in stated]
    assert all(same_float(a, b) for a, b in zip(alike.fraggle.cpu().tolist(), value))
    assert all(same_float(a, F.ratio(r["plain"]) if r["status"] == F.OK else float("nan")) for a, r in zip(alike.plain.cpu().tolist(), stated))
    assert all(same_float(a, F.ratio(r["modified"]) if r["n_fragmentations"] else float("nan")) for a, r in zip(alike.modified.cpu().tolist(), stated))
    assert alike.status.cpu().tolist() == [r["status"] for r in stated] and alike.valid.cpu().tolist() == [r["status"] == F.OK for r in stated]
    assert alike.best_index.cpu().tolist() == [r["best_index"] for r in stated] and alike.n_fragmentations.cpu().tolist() == [r["n_fragmentations"] for r in stated]
    assert alike.marked.cpu().tolist() == [list(r["marked"]) for r in stated]
    assert alike.counts.cpu().tolist() == [list(r["plain"]) + list(r["modified"]) for r in stated]
    top = S.topk_fraggle(alike.fraggle, alike.status, K)
    best = [max((v for v in value[g * K:(g + 1) * K] if v == v), default=float("nan")) for g in range(groups)]
    assert top["best"].cpu().tolist() == best
    assert top["best_index"].cpu().tolist() == [[v for v in value[g * K:(g + 1) * K]].index(b) for g, b in enumerate(best)]
    assert float(top["mean_best"]) == float(torch.tensor(best, dtype=torch.float64).sum() / groups)
    assert 0 < sum(v == 0.0 for v in value) and 0 < sum(v == 1.0 for v in value) < len(value)
    # an engine object gives the same
    other = S.fraggle_similarity_batch(prb_d, p_n[:K * groups].tolist(), to_dev(gpu_device, r_rec[rows], torch.uint8), r_n[rows], ref_index=idx,
                                       max_nodes=F.DEFAULT_NODES)
    assert torch.equal(other.counts, alike.counts) and torch.equal(other.status, alike.status)


# ------------------------------------------------------------------------------------------------------------------ evaluation

def test_evaluate_reports_the_fraggle_similarity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.fraggle`` the 'structure' dict holds the
    entry, equal to the mirror on the run's records (one slot's record is replaced by its ground truth under another atom order); without the
    flag it has no such key."""
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
    truth = SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])])
    moved = B.renumbered(truth, np.random.default_rng(13).permutation(len(truth["type"])))
    gather, kept = shard.gather_by_slot, []

    def gather_and_keep(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        kept.append(by_slot)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_keep)
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert "fraggle" not in plain
    cfg.eval.fraggle, cfg.eval.fraggle_max_nodes = True, SMALL_BUDGET
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"fraggle"}
    fr = st["fraggle"]
    assert set(fr) == {"fraggle", "status", "mean", "scored", "undecided", "unusable", "no_fragmentation", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    rows = F.similarity_table(gen_rec, gen_n, gt_rec, gt_n, slot_ds.numpy(), SMALL_BUDGET)
    assert rows[planted]["status"] == F.OK and rows[planted]["plain"][0] == rows[planted]["plain"][1]
    value = [F.fraggle(r) for r in rows]
    same_float = lambda a, b: a == b or (a != a and b != b)
    assert len(value) == T * K_ and all(same_float(a, b) for a, b in zip(fr["fraggle"].cpu().tolist(), value))
    assert fr["status"].cpu().tolist() == [r["status"] for r in rows]
    scored = [v for v in value if v == v]
    assert fr["scored"] == len(scored) and fr["undecided"] == sum(r["status"] == F.UNDECIDED for r in rows) and fr["unusable"] == sum(r["status"] == F.UNUSABLE for r in rows)
    assert fr["no_fragmentation"] == sum(r["status"] == F.OK and r["n_fragmentations"] == 0 for r in rows)
    total = 0.0
    for v in scored:
        total += v
    assert fr["mean"] == (total / len(scored) if scored else None)
    best = [max((v for v in value[g * K_:(g + 1) * K_] if v == v), default=float("nan")) for g in range(T)]
    assert all(same_float(a, b) for a, b in zip(fr["top_k"]["best"].cpu().tolist(), best))
