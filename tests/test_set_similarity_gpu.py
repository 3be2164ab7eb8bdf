"""GPU: ``dss_fold_bits`` and ``dss_tanimoto_nn`` against the plain-Python definition of tests/sets_mirror.py - every bit, count, nearest
neighbour and index equal, no tolerance on any integer - on molecules and on synthetic rows sized from the header's tile constants; the
fp64 sums within the bound derived below; guarded buffers, determinism, the edges of the shape, the set-level numbers (SNN, IntDiv, novelty)
and the evaluation driver end to end.

The one tolerance.  ``sum`` adds Nb correctly rounded quotients in [0, 1] in a fixed order in fp64; the mirror's ``math.fsum`` of the same
quotients is exact before its one rounding.  Nb - 1 additions of partial sums that stay <= Nb each lose at most Nb * 2^-53, so
|sum_gpu - sum_mirror| <= (Nb - 1) * Nb * 2^-53 <= Nb^2 * 2^-53: derived, not measured."""
import functools
import math

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, mces_mirror as MM, sets_mirror as XM, structure_mirror as SM
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu

TILE_A, TILE_B, CHUNKS = E.SETS_TILE_A, E.SETS_TILE_B, E.SETS_CHUNKS
WIDTHS = (64, 1024, 4096)
# column counts: one row; one column tile plus one row; 2 CHUNKS tiles, so that chunk g takes tiles g and g + CHUNKS and the last chunk's second
# tile is partial
NB_SIZES = (1, TILE_B + 1, (2 * CHUNKS - 1) * TILE_B + TILE_B // 2 + 1)
NA_SIZES = (1, TILE_A - 1, TILE_A + 3)


def _sum_bound(Nb):
    return Nb * Nb * 2.0 ** -53


def _int_div_bound(N):
    """IntDiv of N rows against the mirror's.  Every row sum is within N^2 eps of the mirror's (eps = 2^-53, ``_sum_bound``); adding N such
    sums in index order rounds N - 1 times at partial sums <= N^2 on either side, so the two totals differ by at most N * N^2 eps + 2 (N - 1)
    N^2 eps <= 3 N^3 eps, which the division by the N^2 pairs turns into 3 N eps; the division and the subtraction from 1 round once each on
    either side: 4 eps."""
    return (3 * N + 4) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------ the numpy path of the mirror

_bitcount = getattr(np, "bitwise_count", None)


def _popcount64(x):
    if _bitcount is not None:
        return _bitcount(x).astype(np.int64)
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0f0f0f0f0f0f0f0f)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def numpy_nearest(a, b, skip_same_index=False):
    """``sets_mirror.nearest`` on ``uint64`` word matrices ``a [Na, W]``, ``b [Nb, W]``, for the sizes at which Fractions take too long: the
    common bits by popcounts of the ANDed words, the nearest neighbour by integer cross-multiplication (a strictly larger similarity
    replaces the best, so the lowest index wins a tie; u = 0 stands as 1 / 1), the sum by ``math.fsum`` of numpy's correctly rounded
    quotients.  Returns int64 arrays ``common, union, index``, a float64 array ``sum`` and an int64 array ``compared``."""
    Na, Nb = a.shape[0], b.shape[0]
    pa, pb = _popcount64(a).sum(1), _popcount64(b).sum(1)
    c = np.zeros((Na, Nb), np.int64)
    for lo in range(0, Na, 32):
        c[lo:lo + 32] = _popcount64(a[lo:lo + 32, None, :] & b[None, :, :]).sum(2)
    u = pa[:, None] + pb[None, :] - c
    empty = (u == 0).astype(np.int64)
    cq, uq = c + empty, u + empty
    take = np.ones((Na, Nb), bool)
    if skip_same_index:
        k = np.arange(min(Na, Nb))
        take[k, k] = False
    bc, bu, bj = np.zeros(Na, np.int64), np.ones(Na, np.int64), np.full(Na, -1, np.int64)
    for j in range(Nb):
        better = take[:, j] & ((bj < 0) | (cq[:, j] * bu > bc * uq[:, j]))
        bc, bu, bj = np.where(better, cq[:, j], bc), np.where(better, uq[:, j], bu), np.where(better, j, bj)
    q = np.where(take, cq / uq, 0.0)
    total = np.array([math.fsum(row) for row in q], np.float64).reshape(Na)
    found = bj >= 0
    pick = lambda m: np.where(found, np.take_along_axis(np.pad(m, ((0, 0), (0, 1))), np.maximum(bj, 0)[:, None], 1)[:, 0], -1)
    return pick(c), pick(u), bj, total, take.sum(1).astype(np.int64)


def _mirror_as_arrays(rows):
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    return col(0, np.int64), col(1, np.int64), col(2, np.int64), col(3, np.float64), col(4, np.int64)


def _words_of(rows, n_bits):
    return np.array([XM.words(r, n_bits) for r in rows], np.uint64).reshape(len(rows), n_bits // 64)


def test_numpy_path_is_the_mirror():
    """The fast path of the synthetic cases, pinned once against the Fractions of ``sets_mirror`` (no GPU in this test)."""
    rng = np.random.default_rng(7)
    for n_bits in (64, 128):
        ints = lambda n: [int.from_bytes(rng.bytes(n_bits // 8), "little") & int.from_bytes(rng.bytes(n_bits // 8), "little") for _ in range(n)]
        a_rows, b_rows = ints(7) + [0, (1 << n_bits) - 1], ints(40) + [0, 0, (1 << n_bits) - 1]
        b_rows[11] = b_rows[30] = a_rows[2]
        for skip in (False, True):
            want = _mirror_as_arrays(XM.nearest(a_rows, b_rows, skip))
            got = numpy_nearest(_words_of(a_rows, n_bits), _words_of(b_rows, n_bits), skip)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (n_bits, skip)
        assert numpy_nearest(_words_of(a_rows, n_bits), _words_of(b_rows, n_bits))[2][2] == 11
    none = numpy_nearest(_words_of([5], 64), _words_of([], 64))
    assert [x.tolist() for x in none] == [[-1], [-1], [-1], [0.0], [0]]


# ------------------------------------------------------------------------------------------------------------------ running the kernels

def _dev_rows(dev, words_u64, pop=None):
    """uint64 word matrix -> the binding's operands ``(words i64, popcount i32)`` on the device."""
    pop = _popcount64(words_u64).sum(1) if pop is None else pop
    return to_dev(dev, words_u64.view(np.int64), torch.int64), to_dev(dev, pop, torch.int32)


def _run(dev, a, b, n_bits, skip=False):
    out = E.tanimoto_nn(*_dev_rows(dev, a), *_dev_rows(dev, b), n_bits, skip)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int64, torch.float64, torch.int64]
    assert all(t.shape == (a.shape[0],) for t in out)
    return [t.cpu().numpy() for t in out]


def _compare(got, want, Nb, what):
    for name, x, y in zip(("best_common", "best_union", "best_index"), got[:3], want[:3]):
        assert np.array_equal(x.astype(np.int64), y), f"{what}: {name} differs on rows {np.nonzero(x != y)[0][:10]}"
    assert np.array_equal(got[4], want[4]), f"{what}: compared"
    err = float(np.abs(got[3] - want[3]).max()) if len(want[3]) else 0.0
    print(f"[sets] {what}: max |sum - fsum| = {err:.3e} (bound {_sum_bound(Nb):.3e})")
    assert err <= _sum_bound(Nb), f"{what}: sum off by {err:.3e}, bound {_sum_bound(Nb):.3e}"


def _molecule_rows(n_bits):
    """Bit rows (Python ints) of the 1200 seeded molecules, generated molecules first; the fingerprints are shared with test_morgan_gpu."""
    from tests.test_morgan_gpu import _mirror_sets
    return [XM.bit_row(f, n_bits) for f in _mirror_sets(True, 2)]


@functools.lru_cache(maxsize=1)
def _molecule_nearest():
    """The mirror's answer for the 600 generated molecules against the 600 ground truths at 1024 bits, computed once per process."""
    rows = _molecule_rows(1024)
    return _mirror_as_arrays(XM.nearest(rows[:600], rows[600:]))


def _molecule_records(dev):
    ref, prb, _ = MM.seeded_pairs()
    rec, n = SM.records(prb + ref)
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


@pytest.mark.parametrize("n_bits", WIDTHS)
def test_fold_parity(gpu_device, n_bits):
    rec, n = _molecule_records(gpu_device)
    assert rec.shape[0] == 1200
    ids, count = E.morgan_records(rec, n, True, 2)
    words, pop = E.fold_bits(ids, count, n_bits)
    torch.cuda.synchronize()
    assert words.dtype == torch.int64 and pop.dtype == torch.int32 and words.shape == (1200, n_bits // 64) and pop.shape == (1200,)
    rows = _molecule_rows(n_bits)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), _words_of(rows, n_bits))
    assert pop.cpu().tolist() == [XM.popcount(r) for r in rows]
    via_metrics = S.morgan_bit_rows(rec, n.cpu(), n_bits=n_bits)
    assert torch.equal(via_metrics[0], words) and torch.equal(via_metrics[1], pop)
    if n_bits == 1024:                                                               # the same bits as the bool fingerprint of the per-pair metric
        bits = S.morgan_fingerprints(rec, n, n_bits=n_bits).cpu().numpy()
        assert np.array_equal(np.packbits(bits, axis=1, bitorder="little").view(np.uint64), words.cpu().numpy().view(np.uint64))


def test_fold_clamps_the_count(gpu_device):
    """A count outside [0, 116] is clamped: every slot of the row, or none - never a slot of the next row."""
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1 << 63, size=(4, E.MORGAN_MAX_FEATURES), dtype=np.int64)
    count = np.array([500, -5, 116, 0], np.int32)
    words, pop = E.fold_bits(to_dev(gpu_device, ids, torch.int64), to_dev(gpu_device, count, torch.int32), 256)
    torch.cuda.synchronize()
    rows = [XM.bit_row(ids[p, :k].view(np.uint64).tolist(), 256) for p, k in enumerate((116, 0, 116, 0))]
    assert np.array_equal(words.cpu().numpy().view(np.uint64), _words_of(rows, 256)) and pop.cpu().tolist() == [XM.popcount(r) for r in rows]
    assert pop.cpu().tolist()[1] == 0 and pop.cpu().tolist()[0] > 50


def test_molecule_sets(gpu_device):
    """The 600 generated molecules against the 600 ground truths at 1024 bits, and determinism: a second call is bit-identical."""
    rows = _molecule_rows(1024)
    a_rows, b_rows = rows[:600], rows[600:]
    want = _molecule_nearest()
    a, b = _words_of(a_rows, 1024), _words_of(b_rows, 1024)
    got = _run(gpu_device, a, b, 1024)
    _compare(got, want, 600, "600 x 600 molecules")
    assert (want[2] == np.arange(600)).sum() > 100 and len(set(want[2].tolist())) > 100 and (want[0] == want[1]).sum() > 100      # the set shows something
    ops = (*_dev_rows(gpu_device, a), *_dev_rows(gpu_device, b))
    one, two = E.tanimoto_nn(*ops, 1024), E.tanimoto_nn(*ops, 1024)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    near = S.SetSimilarity(*one)
    assert near.nearest.cpu().tolist() == [XM.tanimoto(c, u) for c, u in zip(want[0].tolist(), want[1].tolist())]
    assert np.array_equal(near.mean.cpu().numpy(), got[3] / 600)


def _synthetic(rng, N, n_bits, specials):
    """``N`` random rows whose bit density cycles through 1 %, 10 % and 50 %; ``specials``: {row: words} written over them."""
    density = np.array([0.01, 0.10, 0.50])[np.arange(N) % 3]
    bits = rng.random((N, n_bits)) < density[:, None]
    words = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(N, n_bits // 64).copy()
    for row, value in specials.items():
        words[row] = value
    return words


@pytest.mark.parametrize("n_bits", WIDTHS)
def test_synthetic_rows(gpu_device, n_bits):
    rng = np.random.default_rng(20261120 + n_bits)
    W = n_bits // 64
    twin = _synthetic(rng, 3, n_bits, {})[2]                                          # the row B holds three times: 50 % dense, so no random row equals it
    zeros, ones = np.zeros(W, np.uint64), np.full(W, np.uint64(2 ** 64 - 1))
    for Nb in NB_SIZES:
        tiles = -(-Nb // TILE_B)
        # the twins sit in different column tiles; in the largest case the lowest of them is in a chunk that is merged AFTER the chunk of the next
        twins = {1: [], 2: [3, 10, TILE_B]}.get(tiles, [2 * TILE_B + 9, (CHUNKS + 1) * TILE_B + 5, Nb - 1])
        specials = {j: twin for j in twins}
        if Nb > 16:
            specials.update({1: zeros, 2: ones})
        b = _synthetic(rng, Nb, n_bits, specials)
        if tiles > CHUNKS:
            assert tiles == 2 * CHUNKS and Nb % TILE_B not in (0,) and (twins[0] // TILE_B) % CHUNKS > (twins[1] // TILE_B) % CHUNKS
        for Na in NA_SIZES:
            a = _synthetic(rng, Na, n_bits, {0: twin} if Na < 4 else {0: twin, 1: zeros, 2: ones})
            want = numpy_nearest(a, b)
            got = _run(gpu_device, a, b, n_bits)
            _compare(got, want, Nb, f"{n_bits} bits, {Na} x {Nb}")
            if twins:
                assert got[2][0] == min(twins) and got[0][0] == got[1][0] == _popcount64(twin).sum()           # the tie goes to the lowest index
            if Na >= 4 and Nb > 16:                                                  # two empty rows are similarity 1: the first empty row of B
                assert (got[0][1], got[1][1], got[2][1]) == (0, 0, np.nonzero(~b.any(1))[0][0]) and (got[0][2], got[1][2], got[2][2]) == (n_bits, n_bits, 2)
    # a set against itself without the self-pairs, across a row tile and a column tile
    N = TILE_A + 3
    a = _synthetic(rng, N, n_bits, {0: twin, 1: zeros, 2: ones, TILE_A + 1: twin, 7: zeros})
    want = numpy_nearest(a, a, True)
    got = _run(gpu_device, a, a, n_bits, skip=True)
    _compare(got, want, N, f"{n_bits} bits, {N} rows against themselves")
    assert (got[2] != np.arange(N)).all() and (got[4] == N - 1).all() and got[2][0] == TILE_A + 1 and got[2][TILE_A + 1] == 0
    assert got[2][1] == [j for j in np.nonzero(~a.any(1))[0] if j != 1][0] <= 7 and got[0][1] == got[1][1] == 0


def test_edges_of_the_shape(gpu_device):
    rng = np.random.default_rng(11)
    a = _synthetic(rng, 5, 1024, {})
    none = _run(gpu_device, a, a[:0], 1024)                                           # Nb = 0: no row compared
    assert [x.tolist() for x in none] == [[-1] * 5, [-1] * 5, [-1] * 5, [0.0] * 5, [0] * 5]
    near = S.SetSimilarity(*(torch.as_tensor(x) for x in none))
    assert torch.isnan(near.nearest).all() and torch.isnan(near.mean).all()
    empty = _run(gpu_device, a[:0], a, 1024)                                          # Na = 0: empty outputs
    assert all(x.shape == (0,) for x in empty)
    both = _run(gpu_device, a[:0], a[:0], 1024, skip=True)
    assert all(x.shape == (0,) for x in both)
    alone = _run(gpu_device, a[:1], a[:1], 1024, skip=True)                           # N = 1 against itself: no row
    assert [x.tolist() for x in alone] == [[-1], [-1], [-1], [0.0], [0]]
    wider = _run(gpu_device, a, a[:2], 1024, skip=True)                               # rows beyond Nb leave nothing out
    assert wider[4].tolist() == [1, 1, 2, 2, 2] and wider[2].tolist()[:2] == [1, 0]
    _compare(wider, numpy_nearest(a, a[:2], True), 2, "5 x 2, skip")
    # the workspace may be the caller's, and larger than needed
    ops = (*_dev_rows(gpu_device, a), *_dev_rows(gpu_device, a))
    ws = torch.empty(E.tanimoto_nn_workspace_bytes(5, 5) + 64, dtype=torch.uint8, device=gpu_device)
    mine, theirs = E.tanimoto_nn(*ops, 1024, False, ws), E.tanimoto_nn(*ops, 1024)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(mine, theirs)) and mine[2].tolist() == [0, 1, 2, 3, 4]


GUARD = 256                 # bytes on both sides of every buffer


def _guarded(n, dtype, dev):
    """``n`` elements of ``dtype`` between two guard regions of GUARD bytes filled with 0xA5: (whole buffer as bytes, the owned view).  (The
    helper of tests/test_block_stages_gpu.py does not fit: it makes fp32 buffers with a guard behind them only; these outputs are int32, int64,
    float64 and bytes, and are guarded on both sides.)"""
    size = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((2 * GUARD + n * size,), 0xA5, dtype=torch.uint8, device=dev)
    return raw, raw[GUARD:GUARD + n * size].view(dtype)


def _guards_intact(raw):
    return bool((raw[:GUARD] == 0xA5).all()) and bool((raw[-GUARD:] == 0xA5).all())


@pytest.mark.parametrize("n_bits", WIDTHS)
def test_guarded_buffers(gpu_device, n_bits):
    """Outputs and workspace of exactly the stated sizes between guard regions: the guards survive, the results are those of the binding."""
    rng = np.random.default_rng(5 + n_bits)
    Na, Nb = TILE_A + 3, CHUNKS * TILE_B + 7
    a, b = _synthetic(rng, Na, n_bits, {}), _synthetic(rng, Nb, n_bits, {})
    (aw, ap), (bw, bp) = _dev_rows(gpu_device, a), _dev_rows(gpu_device, b)
    need = E.tanimoto_nn_workspace_bytes(Na, Nb)
    bufs = [_guarded(Na, dt, gpu_device) for dt in (torch.int32, torch.int32, torch.int64, torch.float64, torch.int64)]
    ws_raw, ws = _guarded(need, torch.uint8, gpu_device)
    lib = E.load_library()
    st = lib.dss_tanimoto_nn(aw.data_ptr(), ap.data_ptr(), Na, bw.data_ptr(), bp.data_ptr(), Nb, n_bits, 0, ws.data_ptr(), need,
                             *(view.data_ptr() for _, view in bufs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and _guards_intact(ws_raw) and all(_guards_intact(raw) for raw, _ in bufs)
    plain = E.tanimoto_nn(aw, ap, bw, bp, n_bits)
    torch.cuda.synchronize()
    assert all(torch.equal(view, t) for (_, view), t in zip(bufs, plain))
    # the fold, the same way
    ids = to_dev(gpu_device, rng.integers(0, 1 << 63, size=(67, E.MORGAN_MAX_FEATURES), dtype=np.int64), torch.int64)
    count = to_dev(gpu_device, rng.integers(0, E.MORGAN_MAX_FEATURES + 1, size=67), torch.int32)
    (w_raw, words), (p_raw, pop) = _guarded(67 * (n_bits // 64), torch.int64, gpu_device), _guarded(67, torch.int32, gpu_device)
    st = lib.dss_fold_bits(ids.data_ptr(), count.data_ptr(), 67, n_bits, words.data_ptr(), pop.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and _guards_intact(w_raw) and _guards_intact(p_raw)
    want = E.fold_bits(ids, count, n_bits)
    assert torch.equal(words.reshape(67, -1), want[0]) and torch.equal(pop, want[1])


# ------------------------------------------------------------------------------------------------------------------ the set-level numbers

def test_snn_and_internal_diversity_on_molecules(gpu_device):
    rec, n = _molecule_records(gpu_device)
    gen, ref = S.morgan_bit_rows(rec[:600].contiguous(), n[:600]), S.morgan_bit_rows(rec[600:].contiguous(), n[600:])
    assert S.snn(gen, gen) == 1.0
    rows = _molecule_rows(1024)
    want = _molecule_nearest()
    assert S.snn(gen, ref) == XM.ordered_mean([XM.tanimoto(c, u) for c, u in zip(want[0].tolist(), want[1].tolist())])
    # IntDiv of a set of identical molecules is exactly 0; of 40 molecules, the mirror's within the bound of the sums
    same = S.morgan_bit_rows(rec[5:6].expand(50, -1).contiguous(), n[5:6].expand(50).contiguous())
    assert S.internal_diversity(same) == 0.0
    some = (gen[0][:40].contiguous(), gen[1][:40].contiguous())
    got, mirror = S.internal_diversity(some), XM.internal_diversity(rows[:40])
    print(f"[sets] IntDiv of 40 molecules: {got!r}, mirror {mirror!r}")
    assert 0.0 < mirror < 1.0 and abs(got - mirror) <= _int_div_bound(40)
    assert math.isnan(S.internal_diversity((gen[0][:0], gen[1][:0]))) and math.isnan(S.snn(gen, (ref[0][:0], ref[1][:0])))


def _novelty_case():
    """(generated molecules, known molecules): 60 distinct graphs, then ten of them again under another numbering; the known table holds
    every second of the 60 under a random numbering."""
    ref, prb, _ = MM.seeded_pairs()
    rng = np.random.default_rng(20261121)
    cls = XM.classes(prb[:200])
    distinct = [prb[p] for p in range(200) if cls[p] == p][:60]
    assert len(distinct) == 60
    generated = distinct + [GM.permuted(m, rng) for m in distinct[:10]]
    known = [GM.permuted(m, rng) for m in distinct[::2]]
    return generated, known


def test_novelty_on_molecules(gpu_device):
    generated, known = _novelty_case()
    dev = lambda mols: tuple(to_dev(gpu_device, x, dt) for x, dt in zip(SM.records(mols), (torch.uint8, torch.int32)))
    got = S.novelty(dev(generated), dev(known))
    assert got.novel.dtype == torch.bool and got.novel.device.type == "cuda"
    expect = [p % 2 == 1 for p in range(60)] + [p % 2 == 1 for p in range(10)]       # exactly the rows whose graph is in the known table are not novel
    assert got.novel.cpu().tolist() == expect
    novel, of_unique, over_all = XM.novelty(generated, known)
    assert novel == expect and (got.novel_fraction_of_unique, got.novel_over_all) == (of_unique, over_all) == (30 / 60, 30 / 70)


def test_set_similarity_metric_on_molecules(gpu_device):
    generated, known = _novelty_case()
    ref, _, _ = MM.seeded_pairs()
    test = ref[:80] + [generated[4], generated[4]]
    dev = lambda mols: tuple(to_dev(gpu_device, x, dt) for x, dt in zip(SM.records(mols), (torch.uint8, torch.int32)))
    fn = S.get_set_similarity_metric(dev(test), known=dev(known))
    out = fn(dev(generated))
    assert set(out) == {"snn", "int_div", "nearest", "nearest_index", "n_generated", "n_test", "novelty"}
    t_cls = XM.classes(test)
    t_rows = [p for p in range(len(test)) if t_cls[p] == p]
    assert out["n_generated"] == 60 and out["n_test"] == len(t_rows) < len(test)
    a_rows, b_rows = XM.molecule_rows(generated[:60], 1024), XM.molecule_rows([test[p] for p in t_rows], 1024)
    near = XM.nearest(a_rows, b_rows)
    assert out["nearest_index"].cpu().tolist() == [t_rows[j] for _, _, j, *_ in near]
    assert out["nearest"].cpu().tolist() == [XM.tanimoto(c, u) for c, u, *_ in near] and out["nearest"].cpu().tolist()[4] == 1.0
    assert out["snn"] == XM.snn(a_rows, b_rows) and isinstance(out["snn"], float) and isinstance(out["int_div"], float)
    assert abs(out["int_div"] - XM.internal_diversity(a_rows)) <= _int_div_bound(60)
    assert out["novelty"].novel.cpu().tolist() == [p % 2 == 1 for p in range(60)] and out["novelty"].novel_fraction_of_unique == 0.5
    keep = torch.zeros(70, dtype=torch.bool)
    keep[[1, 3, 61]] = True                                                           # row 61 is row 1 again
    masked = fn(dev(generated), keep=keep.to(gpu_device))
    assert masked["n_generated"] == 2 and masked["nearest"].shape == (2,) and masked["novelty"].novel.cpu().tolist() == [True, True]


# ------------------------------------------------------------------------------------------------------------------ the driver

def _graph_dataset(count, seed):
    """The small synthetic table of the driver tests (tests/test_structure_metrics_gpu.py): random tree molecules with spectra."""
    from types import SimpleNamespace
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


def test_evaluate_reports_set_similarity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps: with ``cfg.eval.set_similarity`` the 'structure' dict holds the
    set-level numbers of a direct call on ``records_by_slot``; without the flag it has no new key."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
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
    assert "set_similarity" not in plain
    cfg.eval.set_similarity = True
    known = (table.gt_records[:3].clone(), table.num_atom[:3].clone())
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True, known_records=known)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"set_similarity"}
    sets = st["set_similarity"]
    assert set(sets) == {"snn", "int_div", "nearest", "nearest_index", "n_generated", "n_test", "novelty"}
    assert 0.0 <= sets["snn"] <= 1.0 and 0.0 <= sets["int_div"] <= 1.0 and 1 <= sets["n_generated"] <= 6 and 1 <= sets["n_test"] <= 8
    index = sets["nearest_index"].cpu()
    assert index.dtype == torch.int64 and index.shape == (sets["n_generated"],) and bool(((index >= 0) & (index < 8)).all())
    assert sets["nearest"].dtype == torch.float64 and sets["nearest"].device.type == "cuda" and sets["novelty"].novel.shape == index.shape
    n_atoms = [len(atom) for _, atom, _, _ in res["processed_mols"]]
    direct = S.get_set_similarity_metric((table.gt_records.to(gpu_device), table.num_atom), known=(known[0].to(gpu_device), known[1]))(
        (kept[-1], torch.tensor(n_atoms)))
    assert (sets["snn"], sets["int_div"], sets["n_generated"], sets["n_test"]) == (direct["snn"], direct["int_div"], direct["n_generated"], direct["n_test"])
    assert torch.equal(sets["nearest"], direct["nearest"]) and torch.equal(sets["nearest_index"], direct["nearest_index"])
    assert torch.equal(sets["novelty"].novel, direct["novelty"].novel) and sets["novelty"][1:] == direct["novelty"][1:]
