"""CPU: the C-ABI surface of the Morgan fingerprints and its argument checks (fake pointers: nothing that would pass every check is ever
passed), the binding's refusals, the mirror of tests/morgan_mirror.py against the hand table of the definition, and the host reductions.
(The kernels are checked on the GPU against the same mirror: tests/test_morgan_gpu.py.)"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from tests import graph_mirror as GM, mces_mirror as MM, morgan_mirror as FM

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 4-byte aligned address that is nobody's memory


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def _records(lib, P=1, drop_h=1, radius=2, rec=FAKE, n=FAKE, ids=FAKE, count=FAKE):
    p = C.c_void_p
    return lib.ds_morgan_records(p(rec), p(n), C.c_int64(P), C.c_int32(drop_h), C.c_int32(radius), p(ids), p(count), p(None))


def _pairs(lib, P=1, M=1, drop_h=1, radius=2, n_bits=2048, outputs=None, **pointers):
    ptr = lambda key: C.c_void_p(pointers.get(key, FAKE))
    out = [FAKE] * 4 if outputs is None else outputs
    return lib.ds_morgan_similarity_records(ptr("prb_rec"), ptr("prb_n"), C.c_int64(P), ptr("ref_rec"), ptr("ref_n"), C.c_int64(M), ptr("ref_index"),
                                            C.c_int32(drop_h), C.c_int32(radius), C.c_int32(n_bits), *(C.c_void_p(o) for o in out), C.c_void_p(None))


def test_header_declares_and_library_exports_morgan(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(E.HEADER_PATH).read(), flags=re.S)
    want = {
        "ds_morgan_records": ["rec", "n", "P", "drop_h", "radius", "ids", "count", "stream"],
        "ds_morgan_similarity_records": ["prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "drop_h", "radius", "n_bits", "common", "n_prb",
                                         "n_ref", "status", "stream"],
    }
    for name, names in want.items():
        assert name in E.EXPORTS and hasattr(lib, name)
        args = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
    K = E.CONSTS
    assert (K["DS_MORGAN_MAX_RADIUS"], K["DS_MORGAN_MAX_FEATURES"], K["DS_MORGAN_MAX_BITS"], K["DS_MORGAN_OK"], K["DS_MORGAN_INVALID"]) == (3, 116, 4096, 0, 3)
    assert (E.MORGAN_MAX_RADIUS, E.MORGAN_MAX_FEATURES, E.MORGAN_MAX_BITS, E.MORGAN_OK, E.MORGAN_INVALID) == (3, 116, 4096, 0, 3)
    assert E.MORGAN_MAX_FEATURES == E.MAX_ATOMS * (E.MORGAN_MAX_RADIUS + 1) and FM.MAX_RADIUS == E.MORGAN_MAX_RADIUS


def test_no_pairs_launch_nothing(lib):
    assert _records(lib, P=0, rec=None, n=None, ids=None, count=None) == OK
    nulls = {key: None for key in ("prb_rec", "prb_n", "ref_rec", "ref_n", "ref_index")}
    for n_bits in (0, 64, 2048, 4096):
        assert _pairs(lib, P=0, M=0, n_bits=n_bits, outputs=[None] * 4, **nulls) == OK
    for radius in (0, 3):
        assert _records(lib, P=0, radius=radius, drop_h=0, rec=None, n=None, ids=None, count=None) == OK


def test_bad_scalars_are_refused(lib):
    """... with the sizes, before "P = 0 launches nothing"."""
    for P in (0, 1):
        for drop_h in (-1, 2):
            assert _records(lib, P=P, drop_h=drop_h) == ERR_ARG and _pairs(lib, P=P, drop_h=drop_h) == ERR_ARG
        for radius in (-1, 4):
            assert _records(lib, P=P, radius=radius) == ERR_ARG and _pairs(lib, P=P, radius=radius) == ERR_ARG
        for n_bits in (-1, 1, 32, 63, 65, 96, 2047, 2049, 3072, 8192, 1 << 30, -2048):
            assert _pairs(lib, P=P, n_bits=n_bits) == ERR_ARG, n_bits


def test_sizes_out_of_range_are_refused(lib):
    assert _records(lib, P=-1) == ERR_ARG and _records(lib, P=2 ** 31) == ERR_ARG
    assert _pairs(lib, P=-1) == ERR_ARG and _pairs(lib, P=2 ** 31, M=2 ** 31) == ERR_ARG
    assert _pairs(lib, P=1, M=-1) == ERR_ARG and _pairs(lib, P=0, M=-1) == ERR_ARG


def test_every_required_pointer_is_required(lib):
    for key in ("rec", "n", "ids", "count"):
        assert _records(lib, **{key: None}) == ERR_ARG, key
    for key in ("prb_rec", "prb_n", "ref_rec", "ref_n"):
        assert _pairs(lib, **{key: None}) == ERR_ARG, key
    for k in range(4):
        out = [FAKE] * 4
        out[k] = None
        assert _pairs(lib, outputs=out) == ERR_ARG, f"output {k}"


def test_misaligned_tables_and_short_identity_pairing_are_refused(lib):
    assert _records(lib, rec=FAKE + 1) == ERR_ARG
    for key in ("prb_rec", "ref_rec"):
        assert _pairs(lib, **{key: FAKE + 2}) == ERR_ARG, key
    assert _pairs(lib, P=2, M=1, ref_index=None) == ERR_ARG


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec = torch.zeros(4, shard.RECORD_BYTES, dtype=torch.uint8)
    n = torch.full((4,), 3, dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int64)
    for one, two in ((E.morgan_records, E.morgan_similarity_records),
                     (E.DmtEngine.morgan_records.__get__(object()), E.DmtEngine.morgan_similarity_records.__get__(object()))):
        with pytest.raises(TypeError, match="rec"):
            one(rec.float(), n)
        with pytest.raises(TypeError, match="n must"):
            one(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            one(rec[:, :1247].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            one(rec, n[:3])
        with pytest.raises(TypeError, match="drop_h"):
            one(rec, n, 1)
        with pytest.raises(TypeError, match="radius"):
            one(rec, n, True, 2.0)
        with pytest.raises(TypeError, match="radius"):
            one(rec, n, True, True)
        for bad in (-1, 4):
            with pytest.raises(ValueError, match="radius"):
                one(rec, n, True, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            one(rec, n)
        with pytest.raises(TypeError, match="prb_rec"):
            two(rec.float(), n, rec, n)
        with pytest.raises(TypeError, match="ref_n"):
            two(rec, n, rec, n.long())
        with pytest.raises(TypeError, match="ref_index"):
            two(rec, n, rec, n, idx.int())
        with pytest.raises(ValueError, match="ref_rec"):
            two(rec, n, rec[:, :1247].contiguous(), n)
        with pytest.raises(ValueError, match="ref_index"):
            two(rec, n, rec, n, idx[:2])
        with pytest.raises(ValueError, match="contiguous"):
            two(torch.zeros(shard.RECORD_BYTES, 4, dtype=torch.uint8).t(), n, rec, n)
        with pytest.raises(ValueError, match="rows"):
            two(rec, n, rec[:2], n[:2])
        with pytest.raises(TypeError, match="drop_h"):
            two(rec, n, rec, n, None, 0)
        with pytest.raises(TypeError, match="radius"):
            two(rec, n, rec, n, None, True, 2.0)
        for bad in (-1, 4):
            with pytest.raises(ValueError, match="radius"):
                two(rec, n, rec, n, None, True, bad)
        with pytest.raises(TypeError, match="n_bits"):
            two(rec, n, rec, n, None, True, 2, 2048.0)
        for bad in (-1, 1, 32, 96, 2047, 8192):
            with pytest.raises(ValueError, match="n_bits"):
                two(rec, n, rec, n, None, True, 2, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            two(rec, n, rec, n, idx)
    from diffspectra_amd.structure_metrics import morgan_fingerprints, morgan_similarity_batch
    with pytest.raises(RuntimeError, match="no CPU path"):
        morgan_similarity_batch((rec, n), (rec, n))
    with pytest.raises(RuntimeError, match="no CPU path"):
        morgan_fingerprints(rec, n)
    for bad in (0, 32, 100, 8192):
        with pytest.raises(ValueError, match="n_bits"):
            morgan_fingerprints(rec, n, n_bits=bad)


# ------------------------------------------------------------------------------------------------------------------ the mirror

def test_hand_table():
    assert set(FM.HAND_COUNTS) == {"methane", "ethane", "propane", "cyclopropane", "Kekule benzene", "ethanol", "dimethyl ether"}
    for name, want in FM.HAND_COUNTS.items():
        sets = [FM.fingerprint(FM.MOLECULES[name], True, r) for r in range(4)]
        assert tuple(len(s) for s in sets) == want, name
        assert all(a <= b for a, b in zip(sets[:-1], sets[1:])), name                 # F_0 u ... u F_R grows with R
        assert all(0 <= f < 1 << 64 for f in sets[-1])
        assert [len(FM.fingerprint(FM.MOLECULES[name], False, r)) for r in range(4)] == list(want), name      # there are no hydrogens to drop


def test_hand_pairs():
    for a, b, want in FM.HAND_PAIRS:
        assert FM.similarity_counts(FM.MOLECULES[a], FM.MOLECULES[b], True, 2, 0) == want, (a, b)
        assert FM.similarity_counts(FM.MOLECULES[b], FM.MOLECULES[a], True, 2, 0) == (want[0], want[2], want[1]), (a, b)
    assert [p[2] for p in FM.HAND_PAIRS] == [(0, 4, 3), (1, 2, 4), (1, 6, 4), (5, 10, 10)]
    # the hydrogens count: ethane and ethene differ at every layer once the hydrogen count is in the invariant
    ethane, ethene = GM.saturated(FM.MOLECULES["ethane"]), GM.molecule([1, 1, 0, 0, 0, 0], [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5)], orders=[2, 1, 1, 1, 1])
    assert FM.similarity_counts(ethane, ethene, True, 2, 0) == (0, 2, 2)
    assert len(FM.fingerprint(ethane, False, 2)) > 2


def test_dense_record_and_empty_sets():
    _, _, dense = FM.dense_record()
    assert [len(FM.fingerprint(dense, True, r)) for r in range(4)] == [1, 2, 3, 3]
    h2 = GM.molecule([0, 0], [(0, 1)])
    assert FM.fingerprint(h2, True, 2) == set() and len(FM.fingerprint(h2, False, 2)) == 2
    assert FM.fingerprint(GM.molecule([], []), True, 3) == set()
    assert FM.similarity_counts(h2, h2, True, 2, 2048) == (0, 0, 0)


def test_permutation_invariance():
    ref, _, _ = MM.seeded_pairs()
    rng = np.random.default_rng(20261104)
    sizes = set()
    for mol in ref[:100]:
        moved = GM.permuted(mol, rng)
        for drop_h, radius in ((True, 2), (False, 3)):
            want = FM.fingerprint(mol, drop_h, radius)
            assert FM.fingerprint(moved, drop_h, radius) == want
            sizes.add(len(want))
    assert len(sizes) > 10                                                          # the set of molecules shows something


def test_fold():
    ref, prb, _ = MM.seeded_pairs()
    for a, b in zip(prb[:50], ref[:50]):
        fa, fb = FM.fingerprint(a), FM.fingerprint(b)
        for n_bits in (64, 2048):
            c, na, nb = FM.similarity_counts(a, b, True, 2, n_bits)
            assert na == len({f & (n_bits - 1) for f in fa}) <= len(fa) and nb <= len(fb)
            assert len({f & (n_bits - 1) for f in fa & fb}) <= c <= min(na, nb)         # every common feature folds to a common bit


# ------------------------------------------------------------------------------------------------------------------ host reductions

def _similarity(rows):
    from diffspectra_amd.structure_metrics import MorganSimilarity
    i32 = lambda k: torch.tensor([r[k] for r in rows], dtype=torch.int32)
    return MorganSimilarity(i32(0), i32(1), i32(2), torch.tensor([r[3] for r in rows], dtype=torch.uint8))


def test_similarity_edge_values():
    m = _similarity([(0, 0, 0, 0), (3, 4, 6, 0), (0, 0, 3, 0), (0, 5, 0, 0), (-1, -1, -1, 3), (2, 2, 2, 0), (0, 2, 3, 0)])
    tan, cos = m.tanimoto, m.cosine
    assert tan.dtype == cos.dtype == torch.float64 and m.valid.tolist() == [True, True, True, True, False, True, True]
    assert tan[[0, 1, 2, 3, 5, 6]].tolist() == [1.0, 3 / 7, 0.0, 0.0, 1.0, 0.0] and math.isnan(float(tan[4]))
    assert cos[[0, 1, 2, 3, 5, 6]].tolist() == [1.0, 3 / math.sqrt(24.0), 0.0, 0.0, 1.0, 0.0] and math.isnan(float(cos[4]))
    for (c, a, b, _), t, s in zip([(3, 4, 6, 0), (0, 0, 0, 0), (0, 0, 3, 0)], tan[[1, 0, 2]].tolist(), cos[[1, 0, 2]].tolist()):
        assert t == FM.tanimoto(c, a, b) and s == FM.cosine(c, a, b)
    none = _similarity([])
    assert none.tanimoto.shape == (0,) and none.cosine.shape == (0,)


def test_topk_morgan():
    from diffspectra_amd.structure_metrics import topk_morgan
    nan = float("nan")
    tan = torch.tensor([0.25, 1.0, 1.0,   0.5, nan, 0.75,   nan, nan, nan,   nan, 0.0, 0.0,   0.125, 0.125, nan], dtype=torch.float64)
    s = topk_morgan(tan, 3)
    assert set(s) == {"best", "best_index", "mean_best"}
    best = s["best"].tolist()
    assert best[:2] == [1.0, 0.75] and math.isnan(best[2]) and best[3:] == [0.0, 0.125] and s["best"].dtype == torch.float64
    assert s["best_index"].tolist() == [1, 2, -1, 1, 0] and s["best_index"].dtype == torch.int64
    assert float(s["mean_best"]) == (1.0 + 0.75 + 0.0 + 0.125) / 4
    one = topk_morgan(tan, 1)
    assert one["best_index"].tolist() == [-1 if v != v else 0 for v in tan.tolist()]
    assert float(one["mean_best"]) == float(tan[~torch.isnan(tan)].mean())
    for bad in (0, -1, 4):
        with pytest.raises(ValueError):
            topk_morgan(tan, bad)
    empty = topk_morgan(tan[:0], 3)
    assert empty["best"].shape == (0,) and math.isnan(float(empty["mean_best"]))
    assert math.isnan(float(topk_morgan(tan[6:9], 3)["mean_best"]))
