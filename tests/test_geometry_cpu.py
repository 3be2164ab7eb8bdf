"""No GPU: the substructure-geometry MMD (``ds_geometry_*_records``, ``ds_mmd_1d_segments``) up to the device's edge.

- tests/geometry_mirror.py - the yardstick of the GPU tests - against the reference's own numbers in tests/golden/g18_geometry.npz: its MMD
  equals the reference's ``compute_mmd`` run in fp64 and agrees with the reference's fp32 result within the reference's own recorded
  deviation; its bonds and dihedrals are the reference's enumeration as multisets, its angles the reference's as a set, and the reference's
  angle multiplicities are exactly "neighbours that are the begin atom of their bond to the centre";
- the symbol parser on the three shipped lists and its refusals;
- the argument checks of the C entry points through ctypes (every call is refused or launches nothing: the pointers are fake addresses that
  are never dereferenced) and of the Python bindings."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from diffspectra_amd import config as K, engine as E, structure_metrics as S
from tests import geometry_mirror as GEO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_geometry.npz")
OK, ERR_ARG = 0, -1
FAKE = 0x1000


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def mmd_cases(golden):
    return json.loads(str(golden["mmd_cases"]))


def reference_deviation(golden):
    """D: the largest |reference fp32 - reference fp64| over the stored cases and both batch sizes."""
    worst = 0.0
    for name in mmd_cases(golden):
        f64 = float(golden[name + ".f64"])
        if f64 == f64:
            worst = max(worst, abs(float(golden[name + ".ref_b97"]) - f64), abs(float(golden[name + ".ref_b1000"]) - f64))
    return worst


# ---------------------------------------------------------------------------------------------- the mirror against the reference's numbers

def test_mirror_mmd_is_the_reference_in_fp64(golden):
    for name in mmd_cases(golden):
        got = GEO.mmd(golden[name + ".x"], golden[name + ".y"])[0]
        want = float(golden[name + ".f64"])
        if want != want:
            assert got != got, name
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (name, got, want)


def test_mirror_mmd_agrees_with_the_reference_fp32(golden):
    D = reference_deviation(golden)
    assert 1e-8 < D < 1e-5, D
    for name in mmd_cases(golden):
        got = GEO.mmd(golden[name + ".x"], golden[name + ".y"])[0]
        for key in (".ref_b97", ".ref_b1000"):
            ref = float(golden[name + key])
            # D, plus the 1e-12 by which the mirror may differ from the stored fp64 value
            assert (got != got and ref != ref) or abs(got - ref) <= D + 1e-12 * abs(ref), (name, key, got, ref)


def test_closed_form_bandwidth(golden):
    """The header's 2 sum (z - mean)^2 / (N - 1) is the pairwise sum / (N^2 - N)."""
    for name in mmd_cases(golden):
        z = np.concatenate([golden[name + ".x"], golden[name + ".y"]]).astype(np.float64)
        pairwise = GEO.mmd(golden[name + ".x"], golden[name + ".y"])[4]
        closed = 2.0 * ((z - z.mean()) ** 2).sum() / (len(z) - 1)
        assert abs(closed - pairwise) <= 1e-9 * max(pairwise, 1e-300) + 1e-30, name


def _mol(case):
    n = len(case["types"])
    bond = np.zeros((n, n), np.int64)
    for b, e, o in case["bonds"]:
        bond[b, e] = bond[e, b] = o
    return dict(pos=np.zeros((n, 3)), type=np.array(case["types"], np.int64), fc=np.zeros(n, np.int64), bond=bond)


def _key(sym, rev, atoms):
    atoms = tuple(atoms)
    return tuple(sorted((sym, rev))), min(atoms, atoms[::-1])


def _mirror_keys(found):
    return [_key(GEO.symbol(f), GEO.symbol(f[::-1]), a) for f, a in found]


def test_enumeration_is_the_reference(golden):
    cases = json.loads(str(golden["enumeration"]))
    assert len(cases) >= 10 and {"ethane", "ethene", "propyne", "cyclopropane", "lone atom"} <= {c["name"] for c in cases}
    seen_multiplicity = set()
    for case in cases:
        bonds, angles, dihedrals = GEO.entries(_mol(case))
        count = collections.Counter
        assert count(_mirror_keys(bonds)) == count(_key(*e) for e in case["ref_bonds"]), case["name"]
        assert count(_mirror_keys(dihedrals)) == count(_key(*e) for e in case["ref_dihedrals"]), case["name"]
        mine, theirs = count(_mirror_keys(angles)), count(_key(*e) for e in case["ref_angles"])
        assert max(mine.values(), default=1) == 1
        begin_of = {(b, e) for b, e, _ in case["bonds"]}                      # (begin, end) of every bond
        for key in mine:
            a, c, b = key[1]
            want = ((a, c) in begin_of) + ((b, c) in begin_of)                # neighbours that are the begin atom of their bond to c
            assert theirs.get(key, 0) == want, (case["name"], key)
            seen_multiplicity.add(want)
        assert set(theirs) <= set(mine), case["name"]
    assert seen_multiplicity == {0, 1, 2}
    three_ring = next(c for c in cases if c["name"] == "cyclopropane")
    assert any(a[0] == a[3] for _, a in GEO.entries(_mol(three_ring))[2])     # a == b is enumerated, as the reference does


# ---------------------------------------------------------------------------------------------- the symbol parser

def test_shipped_symbol_lists_parse():
    cls = S.geometry_classes()
    assert cls.symbols == (K.QM9_TOP_BOND_SYM, K.QM9_TOP_ANGLE_SYM, K.QM9_TOP_DIHEDRAL_SYM) and [len(c) for c in cls.codes] == [8, 8, 8]
    for groups, names, codes in zip((3, 5, 7), cls.symbols, cls.codes):
        for name, code in zip(names, codes):
            assert GEO.symbol(GEO.code_fields(code, groups)) == name and 0 <= code < 1 << (4 * groups)
    assert cls.codes[0][0] == 1 | 1 << 4 | 0 << 8                             # 'C1H': C = 1, order 1, H = 0, first field lowest
    info = dict(atom_decoder=["H", "C", "N", "O", "F"], top_bond_sym=["C1H"], top_angle_sym=[], top_dihedral_sym=["H1C-C2N-N1H"])
    assert S.geometry_classes(info).codes == ((17,), (), (0 | 1 << 4 | 1 << 8 | 2 << 12 | 2 << 16 | 1 << 20 | 0 << 24,))


@pytest.mark.parametrize("change", [
    dict(top_bond_sym=["C1X"]),                                               # unknown element
    dict(top_bond_sym=["C1H", "H1C"]),                                        # a symbol and its own reverse
    dict(top_angle_sym=["C1C-C1H", "H1C-C1C"]),
    dict(top_angle_sym=["C1C-N1H"]),                                          # parts that do not chain
    dict(top_dihedral_sym=["H1C-C1C"]),                                       # too few parts
    dict(top_bond_sym=["C0H"]),
    dict(top_bond_sym=["C16H"]),
    dict(top_bond_sym=["C1"]),
    dict(top_bond_sym=[f"C{o}{e}" for o in range(1, 10) for e in "HCNO"]),    # 36 classes
])
def test_symbol_lists_are_refused(change):
    info = dict(atom_decoder=list(K.QM9_ATOM_DECODER), top_bond_sym=[], top_angle_sym=[], top_dihedral_sym=[])
    info.update(change)
    with pytest.raises(ValueError):
        S.geometry_classes(info)


# ---------------------------------------------------------------------------------------------- the C entry points refuse before the device

def _count(lib, P=1, rec=FAKE, n=FAKE, tables=(FAKE, 8, FAKE, 8, FAKE, 8), outputs=(FAKE, FAKE)):
    t = [C.c_void_p(v) if k % 2 == 0 else C.c_int32(v) for k, v in enumerate(tables)]
    return lib.ds_geometry_count_records(C.c_void_p(rec), C.c_void_p(n), C.c_int64(P), *t, *(C.c_void_p(o) for o in outputs), C.c_void_p(None))


def _fill(lib, P=1, rec=FAKE, n=FAKE, tables=(FAKE, 8, FAKE, 8, FAKE, 8), totals=(1, 1, 1), offsets=FAKE, outputs=(FAKE,) * 6):
    t = [C.c_void_p(v) if k % 2 == 0 else C.c_int32(v) for k, v in enumerate(tables)]
    return lib.ds_geometry_fill_records(C.c_void_p(rec), C.c_void_p(n), C.c_int64(P), *t, *(C.c_int64(v) for v in totals), C.c_void_p(offsets),
                                        *(C.c_void_p(o) for o in outputs), C.c_void_p(None))


@pytest.mark.parametrize("call", [_count, _fill])
def test_geometry_entry_points_refuse(lib, call):
    assert call(lib, P=0, rec=None, n=None, tables=(None, 0, None, 0, None, 0)) == OK          # no record launches nothing
    assert call(lib, P=-1) == ERR_ARG and call(lib, P=2 ** 31) == ERR_ARG
    for k in (1, 3, 5):
        for bad in (-1, 33):
            tables = [FAKE, 8, FAKE, 8, FAKE, 8]
            tables[k] = bad
            assert call(lib, tables=tuple(tables)) == ERR_ARG, (k, bad)
            assert call(lib, P=0, tables=tuple(tables)) == ERR_ARG                              # the sizes come before "P = 0"
        tables = [FAKE, 8, FAKE, 8, FAKE, 8]
        tables[k - 1] = None
        assert call(lib, tables=tuple(tables)) == ERR_ARG, k
    assert call(lib, rec=None) == ERR_ARG and call(lib, n=None) == ERR_ARG and call(lib, rec=FAKE + 2) == ERR_ARG


def test_geometry_outputs_are_required(lib):
    assert _count(lib, outputs=(None, FAKE)) == ERR_ARG and _count(lib, outputs=(FAKE, None)) == ERR_ARG
    assert _fill(lib, offsets=None) == ERR_ARG
    assert _fill(lib, totals=(-1, 1, 1)) == ERR_ARG and _fill(lib, P=0, totals=(1, 1, -1)) == ERR_ARG
    for k in range(6):
        out = [FAKE] * 6
        out[k] = None
        assert _fill(lib, outputs=tuple(out)) == ERR_ARG, k


def _mmd(lib, C_=1, Nx=4, Ny=4, x=FAKE, x_off=FAKE, y=FAKE, y_off=FAKE, mul=2.0, num=5, sigma=0.0, ws=FAKE, ws_bytes=1 << 30, out=FAKE, status=FAKE):
    p = C.c_void_p
    return lib.ds_mmd_1d_segments(p(x), p(x_off), C.c_int64(Nx), p(y), p(y_off), C.c_int64(Ny), C.c_int64(C_), C.c_double(mul), C.c_int32(num),
                                  C.c_double(sigma), p(ws), C.c_int64(ws_bytes), p(out), p(status), p(None))


def test_mmd_entry_point_refuses(lib):
    nan, inf = float("nan"), float("inf")
    assert _mmd(lib, C_=0, x=None, x_off=None, y=None, y_off=None, ws=None, out=None, status=None) == OK
    for bad in (dict(C_=-1), dict(C_=65536), dict(Nx=-1), dict(Ny=2 ** 31), dict(num=0), dict(num=9), dict(mul=0.0), dict(mul=-2.0), dict(mul=nan),
                dict(mul=inf), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf)):
        assert _mmd(lib, **bad) == ERR_ARG, bad
        if "C_" not in bad:
            assert _mmd(lib, C_=0, **bad) == ERR_ARG, bad                                      # the scalars come before "C = 0"
    for key in ("x", "x_off", "y", "y_off", "ws", "out", "status"):
        assert _mmd(lib, **{key: None}) == ERR_ARG, key
    need = E.mmd_workspace_bytes(3)
    assert need > 0 and need % 8 == 0 and E.mmd_workspace_bytes(0) == 0 and E.mmd_workspace_bytes(6) == 2 * need
    assert _mmd(lib, C_=3, ws_bytes=need - 1) == ERR_ARG and _mmd(lib, ws=FAKE + 4) == ERR_ARG
    size = C.c_int64(0)
    assert lib.ds_mmd_1d_workspace_bytes(C.c_int64(-1), C.byref(size)) == ERR_ARG
    assert lib.ds_mmd_1d_workspace_bytes(C.c_int64(1), None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- the Python bindings check, never convert

def test_python_bindings_refuse():
    rec, n = torch.zeros(2, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    tab = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.geometry_count_records(rec, n, tab, tab, tab)                      # no CPU path
    with pytest.raises(TypeError):
        E.geometry_count_records(rec, n, tab.long(), tab, tab)
    with pytest.raises(TypeError):
        E.geometry_count_records(rec.int(), n, tab, tab, tab)
    with pytest.raises(ValueError):
        E.geometry_count_records(rec, n, torch.zeros(33, dtype=torch.int32), tab, tab)
    with pytest.raises(ValueError):
        E.geometry_count_records(rec, n[:1], tab, tab, tab)
    with pytest.raises(ValueError):
        E.geometry_count_records(rec, n, torch.zeros(16, dtype=torch.int32)[::2], tab, tab)
    off = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.geometry_fill_records(rec, n, tab, tab, tab, off, (0, 0, 0))
    with pytest.raises(TypeError):
        E.geometry_fill_records(rec, n, tab, tab, tab, off.int(), (0, 0, 0))
    with pytest.raises(ValueError):
        E.geometry_fill_records(rec, n, tab, tab, tab, off[:1], (0, 0, 0))
    with pytest.raises(ValueError):
        E.geometry_fill_records(rec, n, tab, tab, tab, off, (0, -1, 0))
    x, xo = torch.zeros(4), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="HIP device"):
        E.mmd_1d_segments(x, xo, x, xo)
    with pytest.raises(TypeError):
        E.mmd_1d_segments(x.double(), xo, x, xo)
    with pytest.raises(TypeError):
        E.mmd_1d_segments(x, xo.int(), x, xo)
    with pytest.raises(ValueError):
        E.mmd_1d_segments(x, xo, x, torch.tensor([0, 2, 4]))
    with pytest.raises(ValueError):
        E.mmd_1d_segments(x.reshape(2, 2), xo, x, xo)
    with pytest.raises(ValueError):
        E.mmd_1d_segments(torch.zeros(8)[::2], xo, x, xo)
    for bad in (dict(kernel_num=0), dict(kernel_num=9), dict(kernel_mul=0.0), dict(kernel_mul=float("nan")), dict(fix_sigma=-1.0),
                dict(workspace=torch.zeros(8, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            E.mmd_1d_segments(x, xo, x, xo, **bad)
    with pytest.raises(TypeError):
        E.mmd_1d_segments(x, xo, x, xo, kernel_num=5.0)
    with pytest.raises(TypeError):
        S.mmd_1d(x.double(), x)
    with pytest.raises(RuntimeError, match="HIP device"):
        S.mmd_1d(x, x)
    assert {"geometry_count_records", "geometry_fill_records", "mmd_1d_segments"} <= set(dir(E.DmtEngine))
