"""dst_gemm's dispatcher without a device: ``dst_gemm_route`` reports the launch ``dst_gemm`` would make (the same plan function computes
both), from fake addresses.  Runs wherever the library loads.

* every case of tests/gemm_route_cases.py still takes the kernel, tile, split, operand orders and epilogue bits it was built for;
* the cases cover every route the dispatcher can produce with no ``DST_GEMM_*`` knob set (found by sweeping the plan function over its own
  thresholds), each tile kernel with and without ``k_tr_gemm_reduce`` where both exist, each epilogue form;
* every product of a training step (tools/train_gemm_bench.py) runs on a route that some GPU case has;
* the thresholds, from both sides; the argument checks of ``dst_gemm`` and ``dst_gemm_route`` agree."""
import itertools
import math

import pytest

from tests import gemm_route_cases as G
from tests.gemm_route_cases import BF16, BIG, SKINNY, SKINNY4, WS, Case, FakeMV, FakeTensor


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    G.assert_no_knob()
    from diffspectra_amd import train_engine
    return train_engine


class RouteOps:
    """``Ops`` without a device: the library, an invented scratch and the arithmetic mode - all that ``Ops.gemm_route`` reads."""

    def __new__(cls, T, scratch, bf16):
        o = object.__new__(T.Ops)
        o.lib, o.scratch, o.bf16 = T.load_train_library(), scratch, bf16
        return o


def route_of(T, c: Case):
    scratch, args, kw = G.fake_call(c)
    return RouteOps(T, scratch, c.bf16).gemm_route(*args, **kw)


def key(T, r):
    """(kernel, BM, BN, threads, split, A row-fast, B row-fast) of a reported route, the kernel by its header name."""
    names = {T.abi.TRAINING.consts[n]: n for n in (WS, SKINNY, SKINNY4, BF16, BIG, "DST_ROUTE_NONE")}
    return (names[r.kernel], r.BM, r.BN, r.threads, r.slices > 1, r.a_rfast, r.b_rfast)


def test_route_constants_and_field_count(T):
    c = T.abi.TRAINING.consts
    assert [c[n] for n in ("DST_ROUTE_NONE", WS, SKINNY, SKINNY4, BF16, BIG)] == [0, 1, 2, 3, 4, 5] and c["DST_ROUTE_FIELDS"] == 11
    assert len(T.GemmRoute._fields) == 11
    import ctypes
    scratch, args, kw = G.fake_call(G.BASE[0])
    o = RouteOps(T, scratch, True)
    packed = o._gemm_args(*args, **kw)
    short = (ctypes.c_int32 * 10)()
    assert o.lib.dst_gemm_route(packed, short, 10) == T.E.CONSTS["DS_ERR_ARG"] and o.lib.dst_gemm_route(packed, None, 11) == T.E.CONSTS["DS_ERR_ARG"]


@pytest.mark.parametrize("c", G.ALL, ids=lambda c: c.name)
def test_case_takes_the_route_it_was_built_for(T, c):
    r = route_of(T, c)
    assert key(T, r) == c.route, f"{c.name}: built for {c.route}, dispatched to {key(T, r)}: change the SHAPE of the case, not the expectation"
    assert r.epilogue == G.epi_bits(c), (c.name, r.epilogue)
    assert r.bf16 == int(c.bf16 and r.kernel not in (T.abi.TRAINING.consts[SKINNY], T.abi.TRAINING.consts[SKINNY4]))
    assert r.workgroups >= 1 and (r.slices - 1) * r.k_per_slice < max(c.K, 1) <= r.slices * max(r.k_per_slice, 1)


def test_details_the_cases_are_named_for(T):
    """Slice counts, k per slice, chunks and tiles that the case names promise."""
    r = {c.name: route_of(T, c) for c in G.BASE}
    assert (r["t128x64 split5"].slices, r["t128x64 split5"].k_per_slice) == (5, 224)
    assert (r["t128x64 split cap2"].slices, r["t128x64 split cap2"].k_per_slice) == (2, 544)           # partial_cap = 2 M N
    assert r["t128x64 unsplit"].workgroups == 8 * 13 * 8                                                 # 97 m-tiles (padded to 104) x 8 n-tiles
    for n in ("wide64 tm1", "wide128 tm1", "wide256 tm1 tn2"):
        assert r[n].k_per_slice % 32 == 0 and 16392 % r[n].k_per_slice != 0                             # a ragged last slice
    assert r["wide256 tm1 tn2"].workgroups == r["wide256 tm1 tn2"].slices * 2 + (-r["wide256 tm1 tn2"].slices % 8) * 2   # tn = 2
    assert r["wide256 tm2 tn2"].workgroups // ((r["wide256 tm2 tn2"].slices + 7) // 8 * 8) == 4           # tm = tn = 2
    # ws: BN = 32 nct; workgroups = groups (<= 256 / chunks, rounded up to 8) x chunks
    assert r["ws4 fwd 2 chunks"].workgroups == 128 * 2 and r["ws4 dx 2 chunks"].workgroups == 128 * 2
    assert r["ws2 minimum N"].workgroups == 256 and r["ws2 K512 2 chunks"].workgroups == 128 * 2


def _fused(c):
    return c.epi.fused


def test_cases_cover_every_reachable_route_and_epilogue_form(T):
    """Sweep the plan function over both sides of its own thresholds, every operand order, aligned and misaligned operands, with and
    without a row sum and scratch, both arithmetic modes: the routes it produces are exactly those of the case table, plus nothing.
    ``k_tr_gemm_bf16<64,128>`` is compiled but not reachable without DST_GEMM_BM / DST_GEMM_BN (BN = 128 needs K >= 4096, BM = 64 needs
    K < 1024): it never shows up in the sweep and is the one instantiation deliberately without a case."""
    Ms = (1, 96, 160, 1024, 1025, 12300, 65536)
    Ns = (1, 16, 64, 65, 129, 512, 1025)
    Ks = (0, 8, 9, 256, 500, 512, 1023, 1024, 4096, 16384)
    swept = set()
    for M, N, K, kind, rowsum, scratch, bf16, a_off in itertools.product(Ms, Ns, Ks, ("fwd", "dx", "dw"), (False, True),
                                                                         ("normal", "empty", "null"), (True, False), (0, 1)):
        lda, ldb = G.r4(M if kind == "dw" else K) + 4, G.r4(K if kind == "fwd" else N) + 4
        c = Case("sweep", "", M, N, K, kind, lda, ldb, (), bf16=bf16, rowsum=rowsum, scratch=scratch, a_off=a_off)
        swept.add(key(T, route_of(T, c))[:5])
    covered = {c.route[:5] for c in G.ALL}
    assert not {k for k in swept if k[:4] in G.NOT_COVERED}, "k_tr_gemm_bf16<64,128> has become reachable: give it a case"
    assert swept == covered, f"routes without a case: {sorted(swept - covered)}; cases on routes the sweep never found: {sorted(covered - swept)}"
    # every instantiation of the kernel file
    inst = {k[:4] for k in covered}
    assert inst == {(WS, 32, 128, 512), (WS, 32, 64, 512), (SKINNY, 1, 1, 256), (SKINNY4, 1, 4, 256), (BF16, 256, 256, 512),
                    (BF16, 256, 128, 512), (BF16, 256, 64, 512), (BF16, 128, 128, 256), (BF16, 128, 64, 256), (BF16, 64, 64, 256),
                    (BIG, 128, 64, 256), (BIG, 64, 64, 256)}
    big_modes = {(c.route[1], c.bf16, c.route[4]) for c in G.ALL if c.route[0] == BIG}
    assert big_modes == set(itertools.product((128, 64), (True, False), (True, False)))                  # k_tr_gemm_big<{128,64},64,{bf16,fp32}>, +- reduce
    # each tile kernel with and without k_tr_gemm_reduce; BM = 64 needs K < 1024 and a split K >= 1024: bf16<64,64> is never split
    for k in inst:
        if k[0] in (BF16, BIG) and k != (BF16, 64, 64, 256):
            assert {k + (False,), k + (True,)} <= covered, k
    assert (BF16, 64, 64, 256, True) not in swept
    # each epilogue form on each kernel family that has it
    forms = {}
    for c in G.ALL:
        forms.setdefault(c.route[:4], set()).add(G.epilogue_form(c.route[0], c.route[4], G.epi_bits(c), _fused(c)))
    four = {"plain direct", "plain staged-vector", "fused scalar", "fused vector"}
    for k in ((BF16, 64, 64, 256), (WS, 32, 64, 512), (BIG, 64, 64, 256)):
        assert forms[k] >= four, (k, forms[k])
    assert forms[(BF16, 128, 64, 256)] >= {"reduce", "plain staged-vector"} and "reduce" in forms[(BF16, 256, 128, 512)]
    assert forms[(SKINNY, 1, 1, 256)] == {"plain direct", "fused scalar"} and forms[(SKINNY4, 1, 4, 256)] == {"fused vector"}
    # the reduce kernel's own epilogue with every fused form, a row sum included
    red = {(c.epi.name, c.rowsum) for c in G.EPILOGUES if c.route[4]}
    assert {(f.name, False) for f in G.FORMS} <= red and {(f.name, True) for f in G.ROWSUM_FORMS} <= red
    # activations: GELU as act and dact, the residual add, on every family
    for fam in G.EPI_HOSTS:
        names = {c.epi.name for c in G.EPILOGUES if c.family == fam}
        assert {f.name for f in G.FORMS} == names, fam


def test_production_shapes_run_on_routes_the_gpu_cases_have(T):
    """The 31 products of tools/train_gemm_bench.py (aligned contiguous operands, bf16 mode, the 48 Mi-float scratch, a row sum on the
    weight gradients as lin_bwd_w passes it)."""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_gemm_bench.py")).read()
    env = dict(Nn=4600, Pp=40400, D=80800, B=256, Ls=256 * 347)
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "SHAPES")
    shapes = [tuple(s[1:6]) for s in eval(compile(ast.Expression(node.value), "shapes", "eval"), {}, env)]
    assert shapes == G.PRODUCTION and len(shapes) == 31, "tools/train_gemm_bench.py's SHAPES and the copy in tests/gemm_route_cases.py differ"
    have = {c.route for c in G.BASE + G.EPILOGUES}
    missing = []
    for M, N, K, ta, tb in G.PRODUCTION:
        kind = "dw" if ta else "fwd" if tb else "dx"
        c = Case("production", "", M, N, K, kind, M if ta else K, K if tb else N, (), rowsum=ta)
        k = key(T, route_of(T, c))
        if k not in have:
            missing.append(((M, N, K, ta, tb), k))
    assert not missing, f"production shapes on routes without a GPU case (shape, route): {missing}"


def _k(T, **kw):
    base = dict(name="threshold", family="", M=2000, N=128, K=256, kind="fwd", lda=None, ldb=None, route=())
    base.update(kw)
    if base["lda"] is None:
        base["lda"] = G.r4(base["M"] if base["kind"] == "dw" else base["K"])
    if base["ldb"] is None:
        base["ldb"] = G.r4(base["K"] if base["kind"] == "fwd" else base["N"])
    return key(T, route_of(T, Case(**base)))


def test_thresholds_from_both_sides(T):
    # ws: M >= 65536, 256 <= K <= 512, K % 128 == 0; nct 4 -> 2 at K = 512
    assert _k(T, M=65535)[:4] == (BF16, 128, 64, 256) and _k(T, M=65536)[:4] == (WS, 32, 128, 512)
    assert _k(T, M=65536, K=320)[:4] == (BF16, 128, 64, 256) and _k(T, M=65536, K=384)[:4] == (WS, 32, 128, 512)       # K % 128
    assert _k(T, M=65536, K=128)[0] == BF16 and _k(T, M=65536, K=640)[0] == BF16
    assert _k(T, M=65536, K=384)[2] == 128 and _k(T, M=65536, K=512)[:4] == (WS, 32, 64, 512)                           # LDS: nct 4 -> 2
    assert _k(T, M=65536, N=15)[0] == BF16 and _k(T, M=65536, N=16)[:3] == (WS, 32, 64) and _k(T, M=65536, N=65)[:3] == (WS, 32, 128)
    assert _k(T, M=65536, kind="dw", K=256)[0] == BF16                                                                   # A must be k-fast
    # skinny: K <= 8 and M >= 1024 (bf16 mode only)
    assert _k(T, K=8, kind="dx")[0] == SKINNY4 and _k(T, K=9, kind="dx")[:4] == (BF16, 64, 64, 256)
    assert _k(T, K=8, kind="dx", M=1023)[:4] == (BF16, 64, 64, 256) and _k(T, K=8, kind="dx", M=1024)[0] == SKINNY4
    assert _k(T, K=8, kind="dx", M=1024, N=126)[0] == SKINNY and _k(T, K=8, kind="fwd", M=1024)[0] == SKINNY          # N % 4, B not n-fast
    assert _k(T, K=8, kind="dx", bf16=False)[0] == BIG and _k(T, K=7, kind="dx", M=1023)[0] == BIG                     # K < 8: no vector kernel
    # wide: K >= 16384, 160 <= M <= 1024, scratch given
    w = dict(kind="dw", N=200)
    assert _k(T, M=256, K=16383, **w) == (BF16, 128, 128, 256, True, 1, 1) and _k(T, M=256, K=16384, **w) == (BF16, 256, 256, 512, True, 1, 1)
    assert _k(T, M=159, K=16384, **w)[:4] == (BF16, 128, 128, 256) and _k(T, M=160, K=16384, **w)[:4] == (BF16, 256, 256, 512)
    assert _k(T, M=1024, K=16384, **w)[:4] == (BF16, 256, 256, 512) and _k(T, M=1025, K=16384, **w)[:4] == (BF16, 128, 128, 256)
    assert _k(T, M=256, K=16384, scratch="null", **w) == (BF16, 128, 128, 256, False, 1, 1)
    assert [_k(T, M=256, K=16384, kind="dw", N=n)[2] for n in (64, 65, 128, 129)] == [64, 128, 128, 256]
    assert [_k(T, M=256, K=16384, kind="dw", N=n, rowsum=True)[2] for n in (63, 64, 127, 128)] == [64, 128, 128, 256]   # the row sum is a column
    # split: K >= 1024 and fewer than 512 tiles; the tile: BM = 64 below 768 tiles with K < 1024, BN = 128 from K = 4096
    assert _k(T, M=130, N=68, K=1023) == (BF16, 64, 64, 256, False, 0, 0) and _k(T, M=130, N=68, K=1024) == (BF16, 128, 64, 256, True, 0, 0)
    assert _k(T, M=130, N=68, K=4095)[:5] == (BF16, 128, 64, 256, True) and _k(T, M=130, N=68, K=4096)[:5] == (BF16, 128, 128, 256, True)
    assert _k(T, M=128 * 95, N=512, K=16)[:4] == (BF16, 64, 64, 256) and _k(T, M=128 * 95 + 1, N=512, K=16)[:4] == (BF16, 128, 64, 256)   # 760 / 768 tiles
    assert _k(T, M=128 * 64, N=512, K=1024)[:5] == (BF16, 128, 64, 256, False)                                           # 512 tiles: unsplit
    assert _k(T, M=128 * 64 - 1, N=512 - 64, K=1024)[:5] == (BF16, 128, 64, 256, True)
    # big: BM = 128 from M = 96
    assert _k(T, M=95, bf16=False)[:4] == (BIG, 64, 64, 256) and _k(T, M=96, bf16=False)[:4] == (BIG, 128, 64, 256)


@pytest.mark.parametrize("M,K", [(65536, 256), (2000, 256), (256, 16384), (130, 1030)])
def test_operands_the_vector_kernels_refuse_fall_back_to_big(T, M, K):
    """vec_ok from both sides, for A and for B, at shapes that take the ws, the tile, the wide and the split kernel when aligned: a pointer
    off the 16-byte grid, a leading stride that is no multiple of 4, a leading stride of 0, a leading stride below the rounded extent -
    always k_tr_gemm_big, never a vector kernel."""
    kind = "dw" if K == 16384 else "fwd"
    ext = M if kind == "dw" else K
    good = _k(T, M=M, K=K, kind=kind)
    assert good[0] in (WS, BF16)
    lib_route = lambda **kw: _k(T, M=M, K=K, kind=kind, **kw)
    assert lib_route(a_off=1)[0] == BIG and lib_route(a_off=4)[0] == good[0]
    assert lib_route(lda=G.r4(ext) + 1)[0] == BIG and lib_route(lda=G.r4(ext) + 2)[0] == BIG and lib_route(lda=G.r4(ext) + 4)[0] == good[0]
    assert lib_route(a_bcast=True)[0] == BIG
    ragged = dict(M=M - 1, K=K) if kind == "dw" else dict(M=M, K=K - 1)
    rext = ext - 1                                                                # extent 4 n - 1: the stride must still reach 4 n
    if not (good[0] == WS):
        assert _k(T, kind=kind, lda=G.r4(rext), **ragged)[0] == BF16 and _k(T, kind=kind, lda=G.r4(rext) - 4, **ragged)[0] == BIG
    assert _k(T, kind=kind, lda=ext - 4, M=M, K=K)[0] == BIG                       # overlapping rows
    extb = G.r4(K) if kind == "fwd" else 128
    assert lib_route(ldb=extb + 1)[0] == BIG and lib_route(ldb=extb - 4)[0] == BIG and lib_route(ldb=0)[0] == BIG and lib_route(ldb=extb + 4)[0] == good[0]
    big = lib_route(a_off=1)
    assert big[:4] == (BIG, 128 if M >= 96 else 64, 64, 256) and big[4] == (K >= 1024)


def test_argument_checks_of_gemm_and_route_agree(T):
    """DS_ERR_ARG before any launch (this machine may have no device: a launch would fail differently), DS_OK for the empty products; the
    query answers the same, with DST_ROUTE_NONE for the empty ones."""
    import ctypes
    OK, ERR = T.E.CONSTS["DS_OK"], T.E.CONSTS["DS_ERR_ARG"]
    base = G.BASE[0]
    scratch, args, kw = G.fake_call(base)
    o = RouteOps(T, scratch, True)
    A, Bm, Cm, ta, tb = args
    ref = FakeMV(1 << 30, base.M, base.N, base.N)

    def both(packed):
        out = (ctypes.c_int32 * 11)(*([-7] * 11))
        return o.lib.dst_gemm(packed, None), o.lib.dst_gemm_route(packed, out, 11), list(out)

    def packed(A=A, Bm=Bm, Cm=Cm, **k):
        return o._gemm_args(A, Bm, Cm, ta, tb, **k)

    def mv(m, rows=None, cols=None, ptr=None):
        return FakeMV(m.ptr if ptr is None else ptr, m.rows if rows is None else rows, m.cols if cols is None else cols, m.ld)

    bad = {"act with accumulate": packed(act=1, acc=True), "dact without ref": packed(dact=1), "act = 4": packed(act=4),
           "dact = 5": packed(dact=5, ref=ref), "act = -1": packed(act=-1), "drop_p = 1": packed(drop=(1.0, 1, 1, 64)),
           "NULL C": packed(Cm=mv(Cm, ptr=0)), "NULL A, K > 0": packed(A=mv(A, ptr=0)),
           "NULL B, K > 0": packed(Bm=mv(Bm, ptr=0))}
    # what Ops.gemm's own checks keep from the library: negative extents and a negative drop_p, patched into the packed struct
    fields = [n for n, _ in T.header_structs()["dst_gemm_args"]]
    good = list(T.STRUCTS["dst_gemm_args"].unpack(packed()))
    for name, value in (("M", -1), ("N", -1), ("K", -1), ("drop_p", -0.5), ("drop_p", math.nan)):
        v = list(good)
        v[fields.index(name)] = value
        bad[f"{name} = {value}"] = T.STRUCTS["dst_gemm_args"].pack(*v)
    for what, p in bad.items():
        st, rt, out = both(p)
        assert (st, rt) == (ERR, ERR), what
    assert o.lib.dst_gemm(None, None) == ERR and o.lib.dst_gemm_route(None, (ctypes.c_int32 * 11)(), 11) == ERR
    empty = {"M = 0": packed(A=mv(A, rows=0), Cm=mv(Cm, rows=0)), "N = 0, no row sum": packed(Bm=mv(Bm, rows=0), Cm=mv(Cm, cols=0))}
    for what, p in empty.items():
        st, rt, out = both(p)
        assert (st, rt) == (OK, OK) and out[0] == T.abi.TRAINING.consts["DST_ROUTE_NONE"] and out[9] == 0, what
    # N = 0 WITH a row sum is a launch (the sums of A's rows)
    st_route = o.gemm_route(A, mv(Bm, rows=0), mv(Cm, cols=0), ta, tb, rowsum=FakeTensor(1 << 31, base.M))
    assert st_route.kernel == T.abi.TRAINING.consts[BIG] and st_route.workgroups >= 1
