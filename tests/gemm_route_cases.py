"""The case table of the dst_gemm route tests.  TEST INFRASTRUCTURE ONLY: imported by tests/test_train_gemm_routes_cpu.py (which asks
``dst_gemm_route`` - no device - whether every case still takes the kernel it was built for) and tests/test_train_gemm_routes_gpu.py (which
runs every case on the GPU against float64).

A case fixes the shape, the storage of the operands (leading strides, offsets from the 16-byte grid), the scratch it gets and the route it
was BUILT FOR: ``(kernel, BM, BN, threads, split, A row-fast, B row-fast)`` as ``dst_gemm_route`` reports them (``out[0..3]``,
``out[4] > 1``, ``out[6..7]``).  When a retune of the dispatcher moves a case to another kernel the CPU test fails: the SHAPE is then
changed until the case selects its kernel again, never the expectation.

Storage.  ``kind`` is the training product: ``fwd`` Y = X W^T (A = X [M, K], B = W [N, K]), ``dx`` dX = dY W (A [M, K], B [K, N]),
``dw`` dW = dY^T X (A stored [K, M], B stored [K, N]).  Every operand and every output is a window of a wider tensor: ``operand_layout``
and ``output_layout`` say where, in floats from a 16-byte aligned base, so that fake addresses (CPU) and real allocations (GPU) give the
dispatcher the same strides and alignments."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional, Tuple

WS, SKINNY, SKINNY4, BF16, BIG = "DST_ROUTE_WS", "DST_ROUTE_SKINNY", "DST_ROUTE_SKINNY4", "DST_ROUTE_BF16", "DST_ROUTE_BIG"
SILU, GELU, TANH, ADDREF = 1, 2, 3, 4
SCRATCH_FLOATS = 48 * 1024 * 1024          # Ops.scratch
GUARD_ROWS = 32                            # NaN / sentinel rows behind every window
DROP_SEED, DROP_STREAM = (1 << 40) + 77, 9

# every DST_GEMM_* knob of csrc/ds_train_gemm.hip: read once per process, so a test run with one of them set would test another dispatcher
KNOBS = ("DST_GEMM_VEC_EPI", "DST_GEMM_VEC_PLAIN", "DST_GEMM_OLD", "DST_GEMM_BN", "DST_GEMM_BM", "DST_GEMM_SPLIT_WGS", "DST_GEMM_WGS",
         "DST_GEMM_WS", "DST_GEMM_WS_MIN_M", "DST_GEMM_SKINNY", "DST_GEMM_WIDE")


def assert_no_knob():
    import os
    on = [k for k in KNOBS if k in os.environ]
    assert not on, f"the route tests describe the dispatcher with no knob set; unset {on} (they are read once per process)"


@dataclass(frozen=True)
class Epi:
    """One epilogue form.  ``vec``: laid out so that the vector epilogue is allowed where N % 4 == 0 (every window on the 16-byte grid, every
    stride a multiple of 4); else the scalar form is forced: C one column off the grid, or - dropout forms - ``drop_ld`` odd."""
    name: str = "plain"
    bias: bool = False
    acc: bool = False
    act: int = 0
    c2: bool = False
    dact: int = 0
    p: float = 0.0
    vec: bool = True

    @property
    def fused(self):
        return bool(self.act or self.dact or self.p > 0.0)


@dataclass(frozen=True)
class Case:
    name: str
    family: str                     # tile | tile+reduce | wide | wide+reduce | ws | big_bf16 | big_fp32 | skinny | skinny4
    M: int
    N: int
    K: int
    kind: str                       # fwd | dx | dw
    lda: int                        # leading stride of A as stored
    ldb: int
    route: Tuple                    # (kernel, BM, BN, threads, split, a_rfast, b_rfast)
    bf16: bool = True
    rowsum: bool = False
    scratch: str = "normal"         # normal | cap2 (2 * M * Nx floats) | empty (non-NULL, 0 floats) | null
    a_off: int = 0                  # floats from the 16-byte grid to A's first element
    a_bcast: bool = False           # A is ONE row read by every m (a_rs = 0)
    epi: Epi = Epi()

    @property
    def ta(self):
        return self.kind == "dw"

    @property
    def tb(self):
        return self.kind == "fwd"

    @property
    def Nx(self):
        return self.N + (1 if self.rowsum else 0)

    def with_epi(self, e: Epi) -> "Case":
        return replace(self, name=f"{self.name}/{e.name}/{'vec' if e.vec else 'scalar'}", epi=e)


def r4(n):
    return (n + 3) // 4 * 4


def operand_layout(c: Case):
    """``{"A": (rows, cols, ld, off), "B": ...}``: the stored matrix (as Ops.gemm's MV takes it, before ``ta`` / ``tb``) and the float offset of
    its first element inside a tensor of ``off + (rows + GUARD_ROWS) * ld`` floats (one row of ``ld`` for a broadcast A)."""
    a = (c.K, c.M) if c.ta else (c.M, c.K)
    b = (c.N, c.K) if c.tb else (c.K, c.N)
    return {"A": (a[0], a[1], 0 if c.a_bcast else c.lda, c.a_off), "B": (b[0], b[1], c.ldb, 0)}


def output_layout(c: Case):
    """``{"C": (ld, col0), "C2": ..., "ref": ..., "drop_ld": n}``: windows of [M + GUARD_ROWS, ld] tensors starting at column ``col0``."""
    e = c.epi
    off_grid = not e.vec and not e.p > 0.0           # scalar form by an unaligned C ...
    col0 = 1 if off_grid else 4
    ldc = r4(col0 + c.N) + 4
    return {"C": (ldc, col0), "C2": (ldc + 4, col0), "ref": (r4(c.N) + 8, 4),
            "drop_ld": c.N + (4 if e.vec else 1)}     # ... or by an odd drop_ld


def epi_bits(c: Case) -> int:
    """``dst_gemm_args._pad`` the case is built for: bit 0 the vector epilogue, bit 1 the staged vector form of a plain epilogue."""
    ok = c.epi.vec and c.N % 4 == 0 and not c.rowsum
    return (1 | (0 if c.epi.fused else 2)) if ok else 0


def epilogue_form(kernel, split, epi, fused) -> str:
    """The one of the five epilogue forms a launch ends in (k_tr_gemm_skinny4 always runs the vector form)."""
    if split:
        return "reduce"
    if kernel == SKINNY4:
        return "fused vector"
    if kernel == SKINNY:
        return "fused scalar" if fused else "plain direct"
    if fused:
        return "fused vector" if epi & 1 else "fused scalar"
    return "plain staged-vector" if epi & 2 else "plain direct"


def _c(name, family, M, N, K, kind, lda, ldb, route, **kw):
    return Case(name, family, M, N, K, kind, lda, ldb, route, **kw)


# ---------------------------------------------------------------------------------------------------------------- the products
# (the smallest shapes that still select the route; K ragged inside a vec4 and across the k-step wherever the kernel allows it)
_WS_ROWS = 65573                     # 2049 full 32-row tiles and one of 5 rows
WS_LDA = 512                         # the one A of the ws cases: [65573, 512], used as column windows

BASE = [
    # bf16<64,64>: K = 42 inside a stride of 48
    _c("t64 fwd", "tile", 70, 36, 42, "fwd", 48, 48, (BF16, 64, 64, 256, False, 0, 0)),
    _c("t64 dx", "tile", 70, 36, 42, "dx", 48, 40, (BF16, 64, 64, 256, False, 0, 1)),
    _c("t64 dw+rowsum", "tile", 70, 36, 42, "dw", 72, 40, (BF16, 64, 64, 256, False, 1, 1), rowsum=True),
    # bf16<128,64>: 97 x 8 tiles >= 768
    _c("t128x64 unsplit", "tile", 12300, 512, 16, "fwd", 16, 16, (BF16, 128, 64, 256, False, 0, 0)),
    _c("t128x64 unsplit dx", "tile", 12300, 512, 16, "dx", 16, 512, (BF16, 128, 64, 256, False, 0, 1)),
    _c("t128x64 unsplit dw", "tile", 12300, 512, 16, "dw", 12300, 512, (BF16, 128, 64, 256, False, 1, 1), rowsum=True),
    _c("t128x64 split5", "tile+reduce", 130, 68, 1030, "fwd", 1032, 1032, (BF16, 128, 64, 256, True, 0, 0)),
    _c("t128x64 split cap2", "tile+reduce", 130, 68, 1030, "fwd", 1032, 1032, (BF16, 128, 64, 256, True, 0, 0), scratch="cap2"),
    _c("t128x64 long-K empty scratch", "tile", 130, 68, 1030, "fwd", 1032, 1032, (BF16, 128, 64, 256, False, 0, 0), scratch="empty"),
    _c("t128x64 long-K NULL scratch", "tile", 130, 68, 1030, "fwd", 1032, 1032, (BF16, 128, 64, 256, False, 0, 0), scratch="null"),
    # bf16<128,128>: K >= 4096
    _c("t128x128 split", "tile+reduce", 130, 132, 4100, "dw", 132, 132, (BF16, 128, 128, 256, True, 1, 1), rowsum=True),
    _c("t128x128 unsplit", "tile", 130, 132, 4100, "dw", 132, 132, (BF16, 128, 128, 256, False, 1, 1), rowsum=True, scratch="empty"),
    # wide: K = 16392 = 512 k-steps and a quarter
    _c("wide64 tm1", "wide+reduce", 161, 63, 16392, "dw", 164, 64, (BF16, 256, 64, 512, True, 1, 1), rowsum=True),
    _c("wide128 tm1", "wide+reduce", 161, 68, 16392, "dw", 164, 68, (BF16, 256, 128, 512, True, 1, 1)),
    _c("wide256 tm1 tn2", "wide+reduce", 161, 260, 16392, "dw", 164, 260, (BF16, 256, 256, 512, True, 1, 1), rowsum=True),
    _c("wide64 tm2", "wide+reduce", 300, 63, 16392, "dw", 300, 64, (BF16, 256, 64, 512, True, 1, 1), rowsum=True),
    _c("wide128 tm2", "wide+reduce", 300, 68, 16392, "dw", 300, 68, (BF16, 256, 128, 512, True, 1, 1)),
    _c("wide256 tm2 tn2", "wide+reduce", 300, 260, 16392, "dw", 300, 260, (BF16, 256, 256, 512, True, 1, 1), rowsum=True),
    _c("wide256 dx", "wide+reduce", 161, 260, 16392, "dx", 16392, 260, (BF16, 256, 256, 512, True, 0, 1)),
    _c("wide256 fwd", "wide+reduce", 161, 260, 16392, "fwd", 16392, 16392, (BF16, 256, 256, 512, True, 0, 0)),
    _c("wide64 unsplit", "wide", 161, 63, 16392, "dw", 164, 64, (BF16, 256, 64, 512, False, 1, 1), rowsum=True, scratch="empty"),
    _c("wide128 unsplit", "wide", 161, 68, 16392, "dw", 164, 68, (BF16, 256, 128, 512, False, 1, 1), scratch="empty"),
    _c("wide256 unsplit", "wide", 161, 260, 16392, "dw", 164, 260, (BF16, 256, 256, 512, False, 1, 1), rowsum=True, scratch="empty"),
    # ws
    _c("ws4 fwd 2 chunks", "ws", _WS_ROWS, 256, 256, "fwd", WS_LDA, 256, (WS, 32, 128, 512, False, 0, 0)),
    _c("ws4 dx 2 chunks", "ws", _WS_ROWS, 132, 384, "dx", WS_LDA, 132, (WS, 32, 128, 512, False, 0, 1)),
    _c("ws4 dx staging edge", "ws", _WS_ROWS, 130, 256, "dx", WS_LDA, 132, (WS, 32, 128, 512, False, 0, 1)),
    _c("ws2 minimum N", "ws", _WS_ROWS, 16, 256, "fwd", WS_LDA, 256, (WS, 32, 64, 512, False, 0, 0)),
    _c("ws2 K512 2 chunks", "ws", _WS_ROWS, 96, 512, "fwd", WS_LDA, 512, (WS, 32, 64, 512, False, 0, 0)),
    # big, bf16: what the vector kernels refuse
    _c("big64 off grid", "big_bf16", 70, 36, 42, "fwd", 48, 48, (BIG, 64, 64, 256, False, 0, 0), a_off=1),
    _c("big64 odd stride", "big_bf16", 70, 36, 42, "fwd", 43, 48, (BIG, 64, 64, 256, False, 0, 0)),
    _c("big64 broadcast A", "big_bf16", 70, 36, 42, "fwd", 48, 48, (BIG, 64, 64, 256, False, 0, 0), a_bcast=True),
    _c("big128 off grid split", "big_bf16", 130, 68, 1030, "fwd", 1032, 1032, (BIG, 128, 64, 256, True, 0, 0), a_off=1),
    _c("big128 odd stride split", "big_bf16", 130, 68, 1030, "fwd", 1031, 1032, (BIG, 128, 64, 256, True, 0, 0)),
    _c("big128 off grid unsplit", "big_bf16", 130, 68, 1030, "fwd", 1032, 1032, (BIG, 128, 64, 256, False, 0, 0), a_off=1, scratch="empty"),
    _c("big64 off grid split", "big_bf16", 70, 36, 1030, "fwd", 1032, 1032, (BIG, 64, 64, 256, True, 0, 0), a_off=1),
    # big, fp32
    _c("f32 64", "big_fp32", 70, 36, 42, "fwd", 48, 48, (BIG, 64, 64, 256, False, 0, 0), bf16=False),
    _c("f32 128 split", "big_fp32", 130, 68, 1030, "fwd", 1032, 1032, (BIG, 128, 64, 256, True, 0, 0), bf16=False),
    _c("f32 128 unsplit", "big_fp32", 130, 68, 1030, "fwd", 1032, 1032, (BIG, 128, 64, 256, False, 0, 0), bf16=False, scratch="empty"),
    _c("f32 64 split", "big_fp32", 70, 36, 1030, "fwd", 1032, 1032, (BIG, 64, 64, 256, True, 0, 0), bf16=False),
    _c("f32 dw rowsum", "big_fp32", 70, 36, 42, "dw", 72, 40, (BIG, 64, 64, 256, False, 1, 1), bf16=False, rowsum=True),
    # skinny
    _c("skinny4", "skinny4", 1024, 256, 8, "dx", 8, 256, (SKINNY4, 1, 4, 256, False, 0, 1)),
    _c("skinny", "skinny", 1024, 7, 3, "dx", 4, 8, (SKINNY, 1, 1, 256, False, 0, 1)),
]

# K = 0 (fp32 mode): C = bias, row sum 0; both ADDED when accumulating
K0 = [
    _c("K0 bias", "big_fp32", 70, 36, 0, "fwd", 4, 4, (BIG, 64, 64, 256, False, 0, 0), bf16=False, epi=Epi("bias", bias=True)),
    _c("K0 bias acc", "big_fp32", 70, 36, 0, "fwd", 4, 4, (BIG, 64, 64, 256, False, 0, 0), bf16=False, epi=Epi("bias+acc", bias=True, acc=True)),
    _c("K0 rowsum", "big_fp32", 70, 36, 0, "dw", 72, 40, (BIG, 64, 64, 256, False, 1, 1), bf16=False, rowsum=True),
    _c("K0 rowsum acc", "big_fp32", 70, 36, 0, "dw", 72, 40, (BIG, 64, 64, 256, False, 1, 1), bf16=False, rowsum=True, epi=Epi("acc", acc=True)),
]

# ---------------------------------------------------------------------------------------------------------------- the epilogue forms
FORMS = ([Epi("bias", bias=True), Epi("acc", acc=True), Epi("bias+acc", bias=True, acc=True),
          Epi("silu", act=SILU), Epi("gelu", act=GELU, bias=True), Epi("tanh", act=TANH),
          Epi("silu+C2", act=SILU, c2=True, bias=True), Epi("gelu+C2+drop", act=GELU, c2=True, bias=True, p=0.1),
          Epi("tanh+C2+drop", act=TANH, c2=True, p=0.1), Epi("drop", bias=True, p=0.1)]
         + [Epi(f"dact{k}{'+drop' if p else ''}{'+acc' if acc else ''}", dact=k, p=p, acc=acc)
            for k in (SILU, GELU, TANH) for p in (0.0, 0.1) for acc in (False, True)]
         + [Epi("addref", dact=ADDREF, bias=True), Epi("addref+acc", dact=ADDREF, acc=True)])

# the smallest case of every kernel family; families without a vector form (N % 4 != 0) run the scalar form only, k_tr_gemm_skinny4 IS the vector form
EPI_HOSTS = {"tile": ("t64 fwd", (True, False)), "tile+reduce": ("t128x64 split5", (True, False)), "wide+reduce": ("wide128 tm1", (True, False)),
             "ws": ("ws2 minimum N", (True, False)), "big_bf16": ("big64 off grid", (True, False)), "big_fp32": ("f32 64", (True, False)),
             "skinny4": ("skinny4", (True,)), "skinny": ("skinny", (False,))}
# fused forms together with a fused row sum (column N takes the plain epilogue inside the staged loop / the reduce kernel): tile kernels
ROWSUM_HOSTS = ("t64 dw+rowsum", "t128x128 split", "wide64 tm1")
ROWSUM_FORMS = [f for f in FORMS if f.name in ("drop", "dact1+drop+acc", "dact2", "addref+acc", "silu+C2", "gelu+C2+drop")]


def by_name(name) -> Case:
    return next(c for c in BASE if c.name == name)


def epilogue_cases():
    out = []
    for family, (host, variants) in EPI_HOSTS.items():
        for f in FORMS:
            for vec in variants:
                out.append(by_name(host).with_epi(replace(f, vec=vec)))
    for host in ROWSUM_HOSTS:
        for f in ROWSUM_FORMS:
            out.append(by_name(host).with_epi(replace(f, vec=False)))
    return out


EPILOGUES = epilogue_cases()
ALL = BASE + K0 + EPILOGUES

# the one instantiation no case selects: BN = 128 needs K >= 4096, BM = 64 needs K < 1024 - only DST_GEMM_BM / DST_GEMM_BN reach it
NOT_COVERED = {(BF16, 64, 128, 256)}

# (M, N, K, ta, tb) of tools/train_gemm_bench.py's SHAPES: the products of one config-5 training step (data, copied: 31 rows)
_Nn, _Pp, _D, _B, _Ls = 4600, 40400, 80800, 256, 256 * 347
PRODUCTION = [
    (_Nn, 252, 256, False, True), (_Nn, 512, 256, False, True), (_Nn, 256, 512, False, True), (_Pp, 256, 64, False, True),
    (_Pp, 64, 128, False, True), (_Pp, 128, 64, False, True), (_Pp, 64, 128, False, True), (_Pp, 256, 128, False, True),
    (_D, 256, 256, False, True), (_D, 3, 256, False, True), (_D, 256, 256, False, False), (256, 256, _D, True, False),
    (_Pp, 64, 256, False, False), (256, 128, _Pp, True, False), (_Pp, 64, 256, False, False), (256, 64, _Pp, True, False),
    (128, 64, _Pp, True, False), (64, 128, _Pp, True, False), (_Nn, 256, 512, False, False), (512, 256, _Nn, True, False),
    (252, 256, _Nn, True, False), (_B, 19744, 1024, False, True), (19744, 1024, _B, True, False), (_B, 1024, 19744, False, False),
    (_Ls, 128, 128, False, True), (_Ls, 256, 128, False, True), (128, 128, _Ls, True, False), (_Ls, 128, 128, False, False),
    (_B, 256, 44416, False, True), (256, 44416, _B, True, False), (_B, 44416, 256, False, False),
]


# ---------------------------------------------------------------------------------------------------------------- fake operands (no device)
class FakeTensor:
    """What Ops.gemm asks of a bias / row-sum / scratch tensor: an address and a length."""

    def __init__(self, ptr, numel):
        self._ptr, self._n = ptr, numel

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


class FakeMV:
    """An MV with an invented address (dst_gemm_route inspects pointers, never reads through them)."""

    def __init__(self, ptr, rows, cols, ld):
        self.ptr, self.rows, self.cols, self.ld = ptr, rows, cols, ld


_FAKE = {k: (i + 1) << 36 for i, k in enumerate(("A", "B", "C", "C2", "ref", "bias", "rowsum", "scratch"))}    # 16-byte aligned, far apart


def scratch_floats(c: Case) -> Optional[int]:
    return {"normal": SCRATCH_FLOATS, "cap2": 2 * c.M * c.Nx, "empty": 0, "null": None}[c.scratch]


def fake_call(c: Case):
    """(scratch, args, kwargs) of ``Ops.gemm`` / ``Ops.gemm_route`` for the case with invented addresses."""
    lay, out, e = operand_layout(c), output_layout(c), c.epi
    mvs = {k: FakeMV(_FAKE[k] + 4 * off, rows, cols, ld) for k, (rows, cols, ld, off) in lay.items()}
    win = lambda k: FakeMV(_FAKE[k] + 4 * out[k][1], c.M, c.N, out[k][0])
    n = scratch_floats(c)
    scratch = FakeTensor(0 if n is None else _FAKE["scratch"], n or 0)
    kw = dict(bias=FakeTensor(_FAKE["bias"], c.N) if e.bias else None, acc=e.acc, rowsum=FakeTensor(_FAKE["rowsum"] + 32, c.M) if c.rowsum else None,
              act=e.act, dact=e.dact, ref=win("ref") if e.dact else None, out2=win("C2") if e.c2 else None,
              drop=(e.p, DROP_SEED, DROP_STREAM, out["drop_ld"]) if e.p > 0.0 else None)
    return scratch, (mvs["A"], mvs["B"], win("C"), c.ta, c.tb), kw
