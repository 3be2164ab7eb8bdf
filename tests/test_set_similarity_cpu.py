"""CPU: the C-ABI surface of the set analytics (include/diffspectra_sets.h) and its argument checks (fake pointers: nothing that would pass
every check is ever passed), the binding's refusals, the mirror of tests/sets_mirror.py on hand-worked rows, and the host arithmetic of
``snn`` / ``internal_diversity`` / ``novelty`` on CPU tensors with a stub engine.  (The kernels are checked on the GPU against the same mirror:
tests/test_set_similarity_gpu.py.)"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import graph_mirror as GM, sets_mirror as XM, structure_mirror as SM

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory
K = abi.SETS.consts


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def _fold(lib, P=1, n_bits=1024, ids=FAKE, count=FAKE, words=FAKE, popcount=FAKE):
    return lib.dss_fold_bits(ids, count, P, n_bits, words, popcount, None)


def _nn(lib, Na=1, Nb=1, n_bits=1024, skip=0, workspace=FAKE, workspace_bytes=1 << 40, outputs=None, **pointers):
    p = lambda key: pointers.get(key, FAKE)
    out = [FAKE] * 5 if outputs is None else outputs
    return lib.dss_tanimoto_nn(p("a_words"), p("a_pop"), Na, p("b_words"), p("b_pop"), Nb, n_bits, skip, workspace, workspace_bytes, *out, None)


def _bytes(lib, Na, Nb):
    size = C.c_int64(-1)
    assert lib.dss_tanimoto_nn_workspace_bytes(Na, Nb, C.byref(size)) == OK
    return size.value


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

def test_header_declares_and_library_exports_the_set_functions(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.SETS.path).read(), flags=re.S)
    want = {
        "dss_fold_bits": ["ids", "count", "P", "n_bits", "words", "popcount", "stream"],
        "dss_tanimoto_nn_workspace_bytes": ["Na", "Nb", "bytes"],
        "dss_tanimoto_nn": ["a_words", "a_pop", "Na", "b_words", "b_pop", "Nb", "n_bits", "skip_same_index", "workspace", "workspace_bytes",
                            "best_common", "best_union", "best_index", "sum", "compared", "stream"],
    }
    assert abi.SETS.exports("dss_") == list(abi.SETS.prototypes) == list(want)
    for name, names in want.items():
        assert hasattr(lib, name)
        args = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
        assert [n for n, _ in abi.SETS.prototypes[name].params] == names
    types = lambda name: [t for _, t in abi.SETS.prototypes[name].params]
    assert types("dss_fold_bits") == ["*", "*", "int64_t", "int32_t", "*", "*", "*"]
    assert types("dss_tanimoto_nn_workspace_bytes") == ["int64_t", "int64_t", "*"]
    assert types("dss_tanimoto_nn") == ["*", "*", "int64_t", "*", "*", "int64_t", "int32_t", "int32_t", "*", "int64_t", "*", "*", "*", "*", "*", "*"]
    # bound on the loaded library, from the header
    for name, proto in abi.SETS.prototypes.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == proto.argtypes, name
    # the tile constants reach Python through the parser, not through copies
    assert (K["DSS_TILE_A"], K["DSS_TILE_B"], K["DSS_CHUNKS"]) == (E.SETS_TILE_A, E.SETS_TILE_B, E.SETS_CHUNKS)
    assert E.SETS_TILE_A % 64 == 0 and E.SETS_TILE_B >= 1 and E.SETS_CHUNKS >= 2
    # two workgroups share a CU's 160 KiB of LDS at the widest row
    assert E.SETS_TILE_B * (E.MORGAN_MAX_BITS // 8 + 4) <= 80 * 1024


def test_the_two_existing_headers_keep_their_prototypes():
    assert len(abi.SAMPLING.prototypes) == 31 and len(abi.TRAINING.prototypes) == 50
    assert E.EXPORTS == abi.SAMPLING.exports("ds_") and not abi.SAMPLING.exports("dss_") and not abi.TRAINING.exports("dss_")


def test_library_without_a_declared_symbol_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dss_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dss_"):
        abi.SETS.bind(Hollow())


def test_workspace_bytes(lib):
    for Na in (1, 5, E.SETS_TILE_A + 3, 10_000):
        sizes = [_bytes(lib, Na, Nb) for Nb in (0, 1, E.SETS_TILE_B, E.SETS_TILE_B + 1, 3 * E.SETS_TILE_B, E.SETS_CHUNKS * E.SETS_TILE_B,
                                                E.SETS_CHUNKS * E.SETS_TILE_B + 1, 100_000, 2 ** 31 - 1)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (Na, sizes)
        assert sizes[-1] == sizes[-2]                                              # the number of chunks is capped
    assert _bytes(lib, 0, 10) == 0 and E.tanimoto_nn_workspace_bytes(7, 100) == _bytes(lib, 7, 100)
    size = C.c_int64(0)
    for Na, Nb in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert lib.dss_tanimoto_nn_workspace_bytes(Na, Nb, C.byref(size)) == ERR_ARG
    assert lib.dss_tanimoto_nn_workspace_bytes(1, 1, None) == ERR_ARG


BAD_BITS = (-1, 0, 1, 32, 63, 65, 96, 1023, 1025, 3072, 8192, 1 << 30, -1024)


def test_empty_calls_launch_nothing(lib):
    for n_bits in (64, 1024, 4096):
        assert _fold(lib, P=0, n_bits=n_bits, ids=None, count=None, words=None, popcount=None) == OK
        nulls = {key: None for key in ("a_words", "a_pop", "b_words", "b_pop")}
        assert _nn(lib, Na=0, Nb=0, n_bits=n_bits, workspace=None, workspace_bytes=0, outputs=[None] * 5, **nulls) == OK
        assert _nn(lib, Na=0, Nb=5, n_bits=n_bits, skip=1, workspace=None, workspace_bytes=0, outputs=[None] * 5, **nulls) == OK


def test_bad_scalars_are_refused(lib):
    """... before "an empty call launches nothing", and before anything is launched: every pointer here is fake."""
    for P in (0, 1):
        for n_bits in BAD_BITS:
            assert _fold(lib, P=P, n_bits=n_bits) == ERR_ARG, n_bits
            assert _nn(lib, Na=P, n_bits=n_bits) == ERR_ARG, n_bits
        for skip in (-1, 2, 256):
            assert _nn(lib, Na=P, skip=skip) == ERR_ARG, skip
    for P in (-1, 2 ** 31):
        assert _fold(lib, P=P) == ERR_ARG
        assert _nn(lib, Na=P) == ERR_ARG and _nn(lib, Nb=P) == ERR_ARG and _nn(lib, Na=0, Nb=P) == ERR_ARG


def test_every_required_pointer_is_required(lib):
    for key in ("ids", "count", "words", "popcount"):
        assert _fold(lib, **{key: None}) == ERR_ARG, key
    for key in ("a_words", "a_pop", "b_words", "b_pop"):
        assert _nn(lib, **{key: None}) == ERR_ARG, key
    for k in range(5):
        out = [FAKE] * 5
        out[k] = None
        assert _nn(lib, outputs=out) == ERR_ARG and _nn(lib, Nb=0, outputs=out) == ERR_ARG, f"output {k}"


def test_workspace_and_alignment_are_checked(lib):
    need = _bytes(lib, 3, 200)
    assert _nn(lib, Na=3, Nb=200, workspace=None) == ERR_ARG
    assert _nn(lib, Na=3, Nb=200, workspace_bytes=need - 1) == ERR_ARG and _nn(lib, Na=3, Nb=200, workspace_bytes=0) == ERR_ARG
    assert _nn(lib, Na=3, Nb=200, workspace=FAKE + 4, workspace_bytes=need) == ERR_ARG
    for key in ("a_words", "b_words"):
        assert _nn(lib, **{key: FAKE + 8}) == ERR_ARG and _nn(lib, n_bits=64, **{key: FAKE + 4}) == ERR_ARG, key


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    ids = torch.zeros(4, E.MORGAN_MAX_FEATURES, dtype=torch.int64)
    count = torch.zeros(4, dtype=torch.int32)
    words, pop = torch.zeros(4, 16, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    for fold, nn in ((E.fold_bits, E.tanimoto_nn), (E.DmtEngine.fold_bits.__get__(object()), E.DmtEngine.tanimoto_nn.__get__(object()))):
        with pytest.raises(TypeError, match="ids"):
            fold(ids.int(), count, 1024)
        with pytest.raises(TypeError, match="count"):
            fold(ids, count.long(), 1024)
        with pytest.raises(ValueError, match="ids"):
            fold(ids[:, :100].contiguous(), count, 1024)
        with pytest.raises(ValueError, match="count"):
            fold(ids, count[:3], 1024)
        with pytest.raises(ValueError, match="contiguous"):
            fold(torch.zeros(E.MORGAN_MAX_FEATURES, 4, dtype=torch.int64).t(), count, 1024)
        with pytest.raises(TypeError, match="n_bits"):
            fold(ids, count, 1024.0)
        with pytest.raises(TypeError, match="n_bits"):
            fold(ids, count, True)
        for bad in (0, 32, 100, 8192):
            with pytest.raises(ValueError, match="n_bits"):
                fold(ids, count, bad)
            with pytest.raises(ValueError, match="n_bits"):
                nn(words, pop, words, pop, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fold(ids, count, 1024)
        with pytest.raises(TypeError, match="a_words"):
            nn(words.int(), pop, words, pop, 1024)
        with pytest.raises(TypeError, match="b_pop"):
            nn(words, pop, words, pop.long(), 1024)
        with pytest.raises(ValueError, match="a_words"):
            nn(words, pop, words, pop, 2048)                                       # 16 words are 1024 bits
        with pytest.raises(ValueError, match="b_words"):
            nn(words, pop, words[:, :8].contiguous(), pop, 1024)
        with pytest.raises(ValueError, match="a_pop"):
            nn(words, pop[:3], words, pop, 1024)
        with pytest.raises(ValueError, match="contiguous"):
            nn(words, pop, torch.zeros(16, 4, dtype=torch.int64).t(), pop, 1024)
        with pytest.raises(TypeError, match="skip_same_index"):
            nn(words, pop, words, pop, 1024, 1)
        with pytest.raises(TypeError, match="workspace"):
            nn(words, pop, words, pop, 1024, False, torch.zeros(1 << 16))
        with pytest.raises(ValueError, match="workspace"):
            nn(words, pop, words, pop, 1024, False, torch.zeros(E.tanimoto_nn_workspace_bytes(4, 4) - 1, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="no CPU path"):
            nn(words, pop, words, pop, 1024)
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.morgan_bit_rows(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.nearest_neighbour_similarity((words, pop), (words, pop))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.get_set_similarity_metric((rec, n))


# ------------------------------------------------------------------------------------------------------------------ the mirror, by hand

def _row(*bits):
    return sum(1 << b for b in bits)


def test_mirror_on_hand_worked_rows():
    a = _row(0, 1, 2, 70)
    # disjoint rows -> 0, identical rows -> 1
    assert XM.similarity(a, _row(3, 4, 900)) == (0, 7, 0) and XM.similarity(a, a) == (4, 4, 1)
    assert XM.nearest([a], [_row(3, 4), a, a]) == [(4, 4, 1, 2.0, 3)]
    # both empty -> 1, and it wins ties by index
    assert XM.similarity(0, 0) == (0, 0, 1)
    assert XM.nearest([0], [_row(5), 0, 0]) == [(0, 0, 1, 2.0, 3)]
    assert XM.nearest([0], [_row(5), _row(6)]) == [(0, 1, 0, 0.0, 2)]                 # every similarity 0: the first row is the nearest
    # 3/4 against 6/8 is a tie.  As two pairs the fractions are equal ...
    a4, a8 = _row(0, 1, 2, 3), _row(*range(6), 100, 101)
    b34, b68 = _row(0, 1, 2), _row(*range(6))
    assert XM.similarity(a4, b34)[:2] == (3, 4) and XM.similarity(a8, b68)[:2] == (6, 8) and XM.similarity(a4, b34)[2] == XM.similarity(a8, b68)[2]
    # ... and ONE row of A (u >= |a| >= c, so it cannot see 3/4 and 6/8 literally) sees the same tie as 9/12 against 12/16: the lower index wins
    a12 = _row(*range(12))
    b1, b2 = _row(*range(9)), _row(*range(200, 204), *range(12))
    assert XM.similarity(a12, b1)[:2] == (9, 12) and XM.similarity(a12, b2)[:2] == (12, 16) and 9 * 16 == 12 * 12
    assert XM.nearest([a12], [b1, b2])[0][:3] == (9, 12, 0) and XM.nearest([a12], [b2, b1])[0][:3] == (12, 16, 0)
    # 5/7 against 7/10: 50 > 49
    a7 = _row(*range(7))
    b57 = _row(*range(5))                                                              # c = 5, u = 7
    b710 = _row(*range(7), 300, 301, 302)                                              # c = 7, u = 10
    assert XM.similarity(a7, b57)[:2] == (5, 7) and XM.similarity(a7, b710)[:2] == (7, 10) and 5 * 10 > 7 * 7
    assert XM.nearest([a7], [b710, b57])[0][:3] == (5, 7, 1) and XM.nearest([a7], [b57, b710])[0][:3] == (5, 7, 0)
    # skip_same_index, and no row at all
    assert XM.nearest([a, a4], [a, a4], skip_same_index=True) == [(3, 5, 1, 0.6, 1), (3, 5, 0, 0.6, 1)]
    assert XM.nearest([a], [a], skip_same_index=True) == [(-1, -1, -1, 0.0, 0)] and XM.nearest([a, 0], []) == [(-1, -1, -1, 0.0, 0)] * 2
    # the sum is fsum of correctly rounded quotients
    assert XM.nearest([a7], [b57, b710, a7, 0])[0][3:] == (math.fsum([5 / 7, 7 / 10, 1.0, 0.0]), 4)
    # words and popcounts
    assert XM.words(_row(0, 63, 64, 130), 256) == [1 | 1 << 63, 1, 4, 0] and XM.popcount(_row(0, 63, 64, 130)) == 4
    assert XM.bit_row({5, 1024 + 5, 2048 + 7, (1 << 64) - 1}, 1024) == _row(5, 7, 1023)
    assert XM.snn([a7, a], [b57, a]) == (5 / 7 + 1.0) / 2 and math.isnan(XM.snn([a7], []))
    assert XM.internal_diversity([a, a, a]) == 0.0 and XM.internal_diversity([a, _row(500)]) == 0.5 and math.isnan(XM.internal_diversity([]))


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine:
    """An engine of CPU tensors that answers from the mirrors: what ``structure_metrics`` does around the kernels, without them."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _mols(rec, n):
        return [SM.mol_from_record(r, int(k)) for r, k in zip(rec.numpy(), n.numpy())]

    def morgan_records(self, rec, n, drop_h=True, radius=2):
        from tests import morgan_mirror as FM
        self.calls.append("morgan_records")
        ids = np.zeros((rec.shape[0], E.MORGAN_MAX_FEATURES), np.uint64)
        count = np.zeros(rec.shape[0], np.int32)
        for p, mol in enumerate(self._mols(rec, n)):
            f = sorted(FM.fingerprint(mol, drop_h, radius))
            ids[p, :len(f)], count[p] = f, len(f)
        return torch.from_numpy(ids.view(np.int64)), torch.from_numpy(count)

    def fold_bits(self, ids, count, n_bits=1024):
        self.calls.append("fold_bits")
        rows = [XM.bit_row(row[:k].tolist(), n_bits) for row, k in zip(ids.numpy().view(np.uint64), count.numpy())]
        words = np.array([XM.words(r, n_bits) for r in rows], np.uint64).reshape(len(rows), n_bits // 64)
        return torch.from_numpy(words.view(np.int64)), torch.tensor([XM.popcount(r) for r in rows], dtype=torch.int32)

    def tanimoto_nn(self, a_words, a_pop, b_words, b_pop, n_bits, skip_same_index=False, workspace=None):
        self.calls.append("tanimoto_nn")
        ints = lambda w: [sum(int(v) << (64 * k) for k, v in enumerate(row)) for row in w.numpy().view(np.uint64).tolist()]
        out = XM.nearest(ints(a_words), ints(b_words), skip_same_index)
        col = lambda k, dt: torch.tensor([r[k] for r in out], dtype=dt)
        return col(0, torch.int32), col(1, torch.int32), col(2, torch.int64), col(3, torch.float64), col(4, torch.int64)

    def graph_hash_records(self, rec, n):
        return torch.tensor([GM.graph_hash(m) - (1 << 64) if GM.graph_hash(m) >> 63 else GM.graph_hash(m) for m in self._mols(rec, n)], dtype=torch.int64)

    def graph_identity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes=4096):
        prb, ref = self._mols(prb_rec, prb_n), self._mols(ref_rec, ref_n)
        verdict = [int(GM.same_graph(m, ref[int(j)])) for m, j in zip(prb, ref_index)]
        return torch.tensor(verdict, dtype=torch.uint8), torch.zeros(len(prb), dtype=torch.int32), torch.zeros(len(prb), 29, dtype=torch.int32)


def _nn_result(rows):
    col = lambda k, dt: torch.tensor([r[k] for r in rows], dtype=dt)
    return S.SetSimilarity(col(0, torch.int32), col(1, torch.int32), col(2, torch.int64), col(3, torch.float64), col(4, torch.int64))


def test_set_similarity_properties():
    m = _nn_result([(3, 4, 7, 1.5, 2), (0, 0, 0, 3.0, 3), (-1, -1, -1, 0.0, 0), (0, 5, 2, 0.0, 4)])
    near, mean = m.nearest, m.mean
    assert near.dtype == mean.dtype == torch.float64
    assert near[[0, 1, 3]].tolist() == [0.75, 1.0, 0.0] and math.isnan(float(near[2]))
    assert mean[[0, 1, 3]].tolist() == [0.75, 1.0, 0.0] and math.isnan(float(mean[2]))
    none = _nn_result([])
    assert none.nearest.shape == (0,) and none.mean.shape == (0,)


def _molecules():
    ethane, propane = GM.molecule([1, 1], [(0, 1)]), GM.molecule([1, 1, 1], [(0, 1), (1, 2)])
    ethanol, ether = GM.molecule([1, 1, 3], [(0, 1), (1, 2)]), GM.molecule([1, 3, 1], [(0, 1), (1, 2)])
    ring = GM.molecule([1, 1, 1], [(0, 1), (1, 2), (0, 2)])
    return ethane, propane, ethanol, ether, ring


def _table(mols):
    rec, n = SM.records(mols)
    return torch.from_numpy(rec), torch.from_numpy(n)


def test_snn_and_internal_diversity_host_arithmetic():
    eng = MirrorEngine()
    ethane, propane, ethanol, ether, ring = _molecules()
    gen_m, ref_m = [ethanol, propane, ring, ethane], [ether, ethane, propane]
    gen, ref = S.morgan_bit_rows(*_table(gen_m), n_bits=64, engine=eng), S.morgan_bit_rows(*_table(ref_m), n_bits=64, engine=eng)
    assert eng.calls == ["morgan_records", "fold_bits"] * 2
    assert gen[0].shape == (4, 1) and gen[0].dtype == torch.int64 and gen[1].dtype == torch.int32
    a_rows, b_rows = XM.molecule_rows(gen_m, 64), XM.molecule_rows(ref_m, 64)
    assert gen[1].tolist() == [XM.popcount(r) for r in a_rows]
    out = S.nearest_neighbour_similarity(gen, ref, engine=eng)
    assert isinstance(out, S.SetSimilarity) and [tuple(t[k].item() for t in out) for k in range(4)] == XM.nearest(a_rows, b_rows)
    assert out.best_index.tolist()[1] == 2 and out.best_index.tolist()[3] == 1 and out.nearest.tolist()[1] == 1.0        # propane, ethane are in the table
    assert S.snn(gen, ref, engine=eng) == XM.snn(a_rows, b_rows)
    assert S.internal_diversity(gen, engine=eng) == XM.internal_diversity(a_rows) and 0.0 < XM.internal_diversity(a_rows) < 1.0
    same = S.morgan_bit_rows(*_table([ethanol] * 3), n_bits=64, engine=eng)
    assert S.internal_diversity(same, engine=eng) == 0.0 and S.snn(same, same, engine=eng) == 1.0
    # a set against itself without the self-pairs; one row alone has no neighbour
    assert S.snn(gen, gen, skip_same_index=True, engine=eng) == XM.ordered_mean([XM.tanimoto(c, u) for c, u, *_ in XM.nearest(a_rows, a_rows, True)])
    one = (gen[0][:1], gen[1][:1])
    assert math.isnan(S.snn(one, one, skip_same_index=True, engine=eng))
    empty = (gen[0][:0], gen[1][:0])
    assert math.isnan(S.snn(gen, empty, engine=eng)) and math.isnan(S.snn(empty, ref, engine=eng)) and math.isnan(S.internal_diversity(empty, engine=eng))


def test_novelty_host_arithmetic():
    eng = MirrorEngine()
    rng = np.random.default_rng(5)
    ethane, propane, ethanol, ether, ring = _molecules()
    known_m = [ethane, ethanol, ethane]
    gen_m = [GM.permuted(ethanol, rng), ring, propane, GM.permuted(ring, rng), ethane, ether, ring]
    got = S.novelty(_table(gen_m), _table(known_m), engine=eng)
    assert isinstance(got, S.Novelty) and got.novel.dtype == torch.bool
    assert got.novel.tolist() == [False, True, True, True, False, True, True]
    # distinct generated graphs: ethanol, ring, propane, ethane, ether = 5; novel ones: ring, propane, ether = 3
    assert got.novel_fraction_of_unique == 3 / 5 and got.novel_over_all == 3 / 7
    want = XM.novelty(gen_m, known_m)
    assert (got.novel.tolist(), got.novel_fraction_of_unique, got.novel_over_all) == want
    nothing = S.novelty(_table(gen_m), (torch.zeros(0, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(0, dtype=torch.int32)), engine=eng)
    assert nothing.novel.all() and nothing.novel_fraction_of_unique == 1.0 and nothing.novel_over_all == 5 / 7
    none = S.novelty((torch.zeros(0, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(0, dtype=torch.int32)), _table(known_m), engine=eng)
    assert none.novel.shape == (0,) and math.isnan(none.novel_fraction_of_unique) and math.isnan(none.novel_over_all)


def test_set_similarity_metric_closure():
    eng = MirrorEngine()
    rng = np.random.default_rng(6)
    ethane, propane, ethanol, ether, ring = _molecules()
    test_m = [propane, ethane, GM.permuted(propane, rng), ether]                       # row 2 repeats row 0
    gen_m = [ethanol, ring, GM.permuted(ethanol, rng), propane, ethane]                # row 2 repeats row 0
    fn = S.get_set_similarity_metric(_table(test_m), known=_table([ethanol]), n_bits=64, engine=eng)
    n_calls = len(eng.calls)
    out = fn(_table(gen_m))
    assert set(out) == {"snn", "int_div", "nearest", "nearest_index", "n_generated", "n_test", "novelty"}
    assert (out["n_generated"], out["n_test"]) == (4, 3) and "morgan_records" in eng.calls[n_calls:]
    kept_gen, kept_test = [gen_m[k] for k in (0, 1, 3, 4)], [test_m[k] for k in (0, 1, 3)]
    a_rows, b_rows = XM.molecule_rows(kept_gen, 64), XM.molecule_rows(kept_test, 64)
    assert out["snn"] == XM.snn(a_rows, b_rows) and out["int_div"] == XM.internal_diversity(a_rows)
    near = XM.nearest(a_rows, b_rows)
    assert out["nearest"].tolist() == [XM.tanimoto(c, u) for c, u, *_ in near]
    assert out["nearest_index"].tolist() == [(0, 1, 3)[j] for _, _, j, *_ in near]   # rows of the caller's table
    assert out["nearest_index"].tolist()[2:] == [0, 1] and out["nearest"].tolist()[2:] == [1.0, 1.0]
    assert out["novelty"].novel.tolist() == [False, True, True, True] and out["novelty"].novel_fraction_of_unique == 0.75
    # keep: a mask over the generated rows; unique=False keeps every row; no `known`, no novelty
    keep = torch.tensor([False, True, True, True, False])
    masked = fn(_table(gen_m), keep=keep)
    assert masked["n_generated"] == 3 and masked["snn"] == XM.snn(XM.molecule_rows([ring, ethanol, propane], 64), b_rows)
    every = S.get_set_similarity_metric(_table(test_m), n_bits=64, unique=False, engine=eng)(_table(gen_m))
    assert (every["n_generated"], every["n_test"]) == (5, 4) and "novelty" not in every
    assert every["int_div"] == XM.internal_diversity(XM.molecule_rows(gen_m, 64)) and every["nearest_index"].tolist()[3] == 0
    nobody = fn(_table(gen_m), keep=torch.zeros(5, dtype=torch.bool))
    assert nobody["n_generated"] == 0 and math.isnan(nobody["snn"]) and math.isnan(nobody["int_div"]) and nobody["nearest"].shape == (0,)
