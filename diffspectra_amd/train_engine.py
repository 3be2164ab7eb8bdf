"""Training graph of the DMT on the HIP training library: forward tape + hand-written backward.

The reference trains through ``torch.autograd`` over ``models/dmt.py``; here every operation of that graph has an explicit forward
and backward kernel in ``csrc/ds_train.hip`` (C-ABI ``include/diffspectra_train.h``) over the packed-ragged layout, and this module
strings them together: ``DmtTrainGraph.forward`` records the activations a backward needs, ``backward`` walks the tape in
reverse and writes the gradient of every parameter.  PyTorch allocates the buffers, slices / concatenates them and owns the
parameters; no arithmetic of the model runs in PyTorch, and there is no CPU path (``engine.load_library`` raises without the .so).

Same de-duplicated formulation as the sampling kernels (exactly result-preserving): adaLN / time MLPs once per
molecule, ``input_lin`` split into row / column / edge parts, ``node2edge_lin`` per node, edge-side tensors once per unordered
pair (a pair row's gradient is the sum over its two directed edges - every backward operation is linear in the incoming gradient).
Dropout is the identity (stage A: the reference's p = 0 arithmetic, pinned by golden G13).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import abi, engine as E
from .abi import ptr

ADA, ADA_STRIDE, ADA_TOP = E.ADA_COLS, E.ADA_STRIDE, E.CONSTS["DS_ADA_TOP"]
NODE_OFF, EDGE_OFF, EQUI_OFF, DIST_OFF = (E.CONSTS[k] for k in ("DS_ADA_NODE", "DS_ADA_EDGE", "DS_ADA_EQUI", "DS_ADA_DIST"))
NB = E.NB
SILU, GELU, TANH = 1, 2, 3
ADDREF = 4                 # dst_gemm `dact` code: the epilogue adds ref (a residual operand) instead of multiplying by f'(ref)
DW_STREAMS = 2             # weight-gradient streams (1: 19.2 ms per step, 2: 17.9, 3: 18.2; profiles/r05_train_ab_final.txt)


# ---- the argument structs of the C-ABI, read from include/diffspectra_train.h by abi.py (the one description of their layouts; the library
#      reports its sizes, load_train_library compares)
# the order in which dst_struct_sizes reports them
STRUCT_NAMES = ("dst_gemm_args", "dst_layout", "dst_piece", "dst_pair_chain_args", "dst_pair_front_args", "dst_dir_chain_args",
                "dst_node_chain_args", "dst_dir_bwd_args", "dst_pair_bwd_args", "dst_node_bwd_args")


def train_exports() -> List[str]:
    return abi.TRAINING.exports("dst_")


def header_structs() -> Dict[str, List[Tuple[str, str]]]:
    """``{struct name: [(field, struct code)]}`` of every ``typedef struct dst_* { ... }`` of the header."""
    return abi.TRAINING.structs


# Call sites pack positionally: keyword packing or a ctypes Structure built field by field costs ~10 us per call, and a step makes ~600 products
STRUCTS = {n: abi.TRAINING.packer(n) for n in header_structs()}
_GEMM_PACK = STRUCTS["dst_gemm_args"].pack
_CHAIN_PACK = STRUCTS["dst_pair_chain_args"].pack
_FRONT_PACK = STRUCTS["dst_pair_front_args"].pack
_DIR_PACK = STRUCTS["dst_dir_chain_args"].pack
_NODE_PACK = STRUCTS["dst_node_chain_args"].pack
_DIRB_PACK = STRUCTS["dst_dir_bwd_args"].pack
_PAIRB_PACK = STRUCTS["dst_pair_bwd_args"].pack
_NODEB_PACK = STRUCTS["dst_node_bwd_args"].pack


class GemmRoute(NamedTuple):
    """What ``dst_gemm_route`` reports, in the order of its ``out`` array (``kernel``: a ``DST_ROUTE_*`` constant of the header)."""
    kernel: int
    BM: int
    BN: int
    threads: int
    slices: int
    k_per_slice: int
    a_rfast: int
    b_rfast: int
    epilogue: int
    workgroups: int
    bf16: int


assert len(GemmRoute._fields) == abi.TRAINING.consts["DST_ROUTE_FIELDS"]

DstPiece = abi.TRAINING.ctypes_struct("dst_piece")
DstLayout = abi.TRAINING.ctypes_struct("dst_layout")


def _piece_table(dev, dst: List[torch.Tensor], src: List[torch.Tensor], cache: dict, key: str, row):
    """(device pointer, length) of the ``dst_piece`` table with the rows ``row(i, dst[i], src[i])``.  The table is rebuilt only when a pointer
    changed (parameters live in the optimizer's flat buffer, the concatenated buffers are persistent)."""
    sig = tuple(t.data_ptr() for t in dst) + tuple(t.data_ptr() for t in src)
    ent = cache.get(key)
    if ent is None or ent[0] != sig:
        arr = (DstPiece * len(dst))(*(row(i, d, s_) for i, (d, s_) in enumerate(zip(dst, src))))
        ent = cache[key] = (sig, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(dst))
    return ent[1].data_ptr(), ent[2]


def copy_pieces(lib, dev, dst: List[torch.Tensor], src: List[torch.Tensor], cache: dict, key: str, stream=None):
    """``dst[i].copy_(src[i])`` for many small (<= 2-D, last dimension contiguous) fp32 pieces in ONE ``dst_copy_pieces`` launch."""
    def row(i, d, s_):
        assert d.shape == s_.shape and d.dtype == torch.float32 and s_.dtype == torch.float32 and d.dim() <= 2
        rows, cols = (1, d.numel()) if d.dim() < 2 else (d.shape[0], d.shape[1])
        assert rows * cols < 2 ** 31                              # the kernel's index arithmetic is 32-bit
        ld = lambda t: (t.stride(0) if t.dim() == 2 and t.shape[0] > 1 else cols)
        assert (d.dim() < 2 or d.stride(-1) == 1 or cols == 1) and (s_.dim() < 2 or s_.stride(-1) == 1 or cols == 1)
        assert d.dim() >= 1 and (d.dim() == 2 or d.is_contiguous()) and (s_.dim() == 2 or s_.is_contiguous())
        return DstPiece(src=s_.data_ptr(), dst=d.data_ptr(), rows=rows, cols=cols, src_ld=ld(s_), dst_ld=ld(d))
    table, n = _piece_table(dev, dst, src, cache, key, row)
    E._check(lib.dst_copy_pieces(table, n, stream if stream is not None else E._stream()), "dst_copy_pieces")


def pack_bf16_pieces(lib, dev, dst: List[torch.Tensor], src: List[torch.Tensor], cache: dict, key: str, stream=None, key_t=None):
    """``dst[i].copy_(src[i])`` with ``dst`` in bfloat16 (round to nearest even) for many small 2-D pieces in ONE ``dst_pack_bf16_pieces`` launch:
    the weights of the fused row chains, once per step.  ``key_t``: the indices of the pieces that are stored TRANSPOSED."""
    def row(i, d, s_):
        assert d.dtype == torch.bfloat16 and s_.dtype == torch.float32 and d.dim() == 2 and d.stride(1) == 1 and s_.stride(1) == 1 and d.numel() < 2 ** 31
        transposed = key_t is not None and i in key_t           # dst = src^T (dst_ld < 0 in the table)
        assert tuple(d.shape) == (tuple(s_.shape)[::-1] if transposed else tuple(s_.shape))
        return DstPiece(src=s_.data_ptr(), dst=d.data_ptr(), rows=s_.shape[0], cols=s_.shape[1], src_ld=s_.stride(0),
                        dst_ld=-d.stride(0) if transposed else d.stride(0))
    table, n = _piece_table(dev, dst, src, cache, key, row)
    E._check(lib.dst_pack_bf16_pieces(table, n, stream if stream is not None else E._stream()), "dst_pack_bf16_pieces")


_lib = None


def load_train_library() -> C.CDLL:
    """The training entry points live in the same shared library as the sampling path (``engine.load_library`` binds both headers and fails
    loudly if an entry point is missing); here the training argument structs are compared with the library's."""
    global _lib
    if _lib is None:
        lib = E.load_library()
        sizes = (C.c_int64 * len(STRUCT_NAMES))()
        E._check(lib.dst_struct_sizes(sizes, len(sizes)), "dst_struct_sizes")
        bad = [(n, lib_n, STRUCTS[n].size) for n, lib_n in zip(STRUCT_NAMES, sizes) if STRUCTS[n].size != lib_n]
        if bad:
            raise RuntimeError(f"C-ABI struct layout mismatch (training): (struct, library, binding) {bad}")
        _lib = lib
    return _lib


class MV:
    """A row-major matrix view into a device tensor: ``rows x cols`` at element offset ``off`` with row stride ``ld``."""
    __slots__ = ("t", "rows", "cols", "ld", "off")

    def __init__(self, t: torch.Tensor, rows: int, cols: int, ld: int, off: int = 0):
        self.t, self.rows, self.cols, self.ld, self.off = t, rows, cols, ld, off

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * self.off


def mv(t: torch.Tensor, c0: Optional[int] = None, c1: Optional[int] = None, r0: int = 0, r1: Optional[int] = None) -> MV:
    """View of a contiguous 2-D (or 1-D as one row) fp32 tensor, optionally restricted to columns c0:c1 / rows r0:r1.
    (Called ~1 500 times per training step: kept free of numpy and of asserts that cost more than the launch they guard.)"""
    shp = t.shape
    if len(shp) == 1:
        t2r, t2c = 1, shp[0]
    else:
        t2r = shp[0]
        t2c = shp[1] if len(shp) == 2 else (t.numel() // t2r if t2r else 0)
    if not t.is_contiguous() or t.dtype is not torch.float32:
        raise ValueError("mv() needs a contiguous fp32 tensor")
    if c0 is None:
        c0 = 0
    if c1 is None:
        c1 = t2c
    if r1 is None:
        r1 = t2r
    return MV(t, r1 - r0, c1 - c0, t2c, r0 * t2c + c0)


def _need_bf16(*weights):
    """The fused row chains stream their weights as bf16 (dst_pack_bf16_pieces / .to(torch.bfloat16): nearest even)."""
    assert all(w_.dtype == torch.bfloat16 for w_ in weights)


class Ops:
    """ctypes wrappers over the dst_* entry points, issued on torch's current stream."""

    def __init__(self, device):
        self.lib = load_train_library()
        self.dev = torch.device(device)
        self.scratch = torch.empty(48 * 1024 * 1024, dtype=torch.float32, device=self.dev)     # split-K partials / column sums
        self.bf16 = False      # config.training.precision == 'bf16': every GEMM rounds its operands to bf16 (fp32 accumulate, fp32 storage)
        # Weight-gradient products on a SIDE stream (a backward pass switches it on, stream_modes()): nothing downstream of a backward pass reads
        # dW, so the ~200 split-K products of a step need not sit in the dependent chain of input-gradient kernels - they fill the CUs the
        # small kernels of that chain leave idle.  The side stream has its own split-K scratch; operands are kept alive until join_dw().
        self.async_dw = False
        self.main_stream = None    # torch's current stream between begin() and end()
        self.stream_ptr = None     # the HIP stream launches go to (main, or the node / a weight-gradient stream inside _OnStream)
        self.cur_stream = None     # the torch stream of stream_ptr inside a node section or a weight-gradient product, else None (main)
        self._node = None          # the node stream (_OnStream), created by the first node section
        self._sides = []           # the weight-gradient streams (_OnStream, DW_STREAMS of them, round-robin)
        self._side_of = {}         # output pointer -> stream index: products that accumulate into the same gradient stay on one stream, in order
        self._side_next = 0
        self._dw_keep = []
        self._parts = {}           # scratch of the fused backward kernels' column sums, grown on demand

    def _s(self):
        """The HIP stream the kernels are issued on.  ``torch.cuda.current_stream()`` costs ~8 us and a step makes ~1 200 calls: the training
        entry points fetch it once (``begin``) and every launch of the step reuses the handle (``end`` drops it)."""
        return self.stream_ptr if self.stream_ptr is not None else E._stream()

    def begin(self):
        self.main_stream = torch.cuda.current_stream(self.dev)
        self.stream_ptr = self.main_stream.cuda_stream

    def end(self):
        self.stream_ptr = None
        self.main_stream = None
        self.cur_stream = None

    def stream_modes(self) -> Tuple[bool, bool]:
        """(node stream, weight-gradient streams) as the environment asks for them NOW: every forward / backward reads them, so a caller
        may flip them between two steps.  The node stream needs the stream handle of ``begin``."""
        return (bool(int(os.environ.get("DIFFSPECTRA_NODE_STREAM", "1"))) and self.main_stream is not None,
                bool(int(os.environ.get("DIFFSPECTRA_ASYNC_DW", "1"))))

    def _gemm_args(self, A: MV, Bm: MV, Cm: MV, ta: bool, tb: bool, bias=None, acc=False, rowsum=None, act=0, dact=0, ref=None, out2=None,
                   drop=None) -> bytes:
        """The packed ``dst_gemm_args`` of one product (``gemm`` and ``gemm_route`` pass the same struct)."""
        M, K = (A.cols, A.rows) if ta else (A.rows, A.cols)
        a_rs, a_cs = (1, A.ld) if ta else (A.ld, 1)
        K2, N = (Bm.cols, Bm.rows) if tb else (Bm.rows, Bm.cols)
        b_rs, b_cs = (1, Bm.ld) if tb else (Bm.ld, 1)
        assert K == K2 and Cm.rows == M and Cm.cols == N, (M, K, K2, N, Cm.rows, Cm.cols)
        if bias is not None:
            assert bias.numel() == N
        if rowsum is not None:
            assert rowsum.numel() == M and rowsum.is_contiguous()
        dp = drop[0] if drop and drop[0] > 0 else 0.0
        args = _GEMM_PACK(A.ptr, a_rs, a_cs, Bm.ptr, b_rs, b_cs, Cm.ptr, Cm.ld, 0 if bias is None else bias.data_ptr(), M, N, K, int(acc),
                          self.scratch.data_ptr(), self.scratch.numel(), int(self.bf16), 0, 0 if rowsum is None else rowsum.data_ptr(), act, dact,
                          0 if ref is None else ref.ptr, 0 if ref is None else ref.ld, 0 if out2 is None else out2.ptr, 0 if out2 is None else out2.ld,
                          float(dp), int(drop[2]) if drop else 0, int(drop[1]) if drop else 0, int(drop[3]) if drop else 0)
        if ref is not None:
            assert ref.rows == M and ref.cols == N
        if out2 is not None:
            assert out2.rows == M and out2.cols == N
        return args

    def gemm(self, A: MV, Bm: MV, Cm: MV, ta: bool, tb: bool, bias: Optional[torch.Tensor] = None, acc: bool = False,
             rowsum: Optional[torch.Tensor] = None, act: int = 0, dact: int = 0, ref: Optional[MV] = None, out2: Optional[MV] = None,
             drop=None):
        """``drop = (p, seed, stream_id, row_length)``: the Philox dropout mask of element (m, n) is taken at index m * row_length + n."""
        st = self.lib.dst_gemm(self._gemm_args(A, Bm, Cm, ta, tb, bias, acc, rowsum, act, dact, ref, out2, drop), self._s())
        if st:                                        # ~650 calls per step and no scalar argument to convert: the status is tested here,
            E._check(st, "dst_gemm")                  # _check is the error path only

    def gemm_route(self, A: MV, Bm: MV, Cm: MV, ta: bool, tb: bool, bias: Optional[torch.Tensor] = None, acc: bool = False,
                   rowsum: Optional[torch.Tensor] = None, act: int = 0, dact: int = 0, ref: Optional[MV] = None, out2: Optional[MV] = None,
                   drop=None) -> "GemmRoute":
        """The launch ``gemm`` would make for the same arguments (``dst_gemm_route``: kernel, tile, slices, operand orders, epilogue bits),
        without making it.  Nothing is read through the pointers and no device is touched."""
        out = (C.c_int32 * len(GemmRoute._fields))()
        E._check(self.lib.dst_gemm_route(self._gemm_args(A, Bm, Cm, ta, tb, bias, acc, rowsum, act, dact, ref, out2, drop), out, len(out)), "dst_gemm_route")
        return GemmRoute(*out)

    def colsum(self, X: MV, out: torch.Tensor, acc: bool = False, param_grad: bool = False):
        """``param_grad``: the sums are a parameter gradient (nothing downstream of the pass reads them) - with the weight-gradient stream on
        they go there, like ``lin_bwd_w``; X must then not be overwritten before ``join_dw``."""
        assert out.numel() == X.cols
        if param_grad and self.async_dw:
            with self._to_side(X.t, out, out=out):
                return self.colsum(X, out, acc)
        E._check(self.lib.dst_colsum(X.ptr, X.ld, X.rows, X.cols, ptr(out), int(acc),
                                     ptr(self.scratch), self.scratch.numel(), self._s()), "dst_colsum")

    def _to_side(self, *keep, out=None):
        """Pick the weight-gradient stream of this product (``out``: its output tensor - the same output always goes to the same stream) and let
        it wait for the stream the operands were produced on (main, or the node stream inside a node section).  Several streams: a weight
        gradient is a split-K product plus its reduction, two dependent launches that fill a fraction of the chip - on one stream they ran one
        after the other and that stream, not the main one, ended the backward (leaving every weight gradient out shortened the step by 3.9 ms)."""
        if not self._sides:
            self._sides = [_OnStream(self, torch.cuda.Stream(device=self.dev), torch.empty_like(self.scratch)) for _ in range(DW_STREAMS)]
        key = None if out is None else out.data_ptr()
        k = self._side_of.get(key) if key is not None else None
        if k is None:
            k = self._side_next
            self._side_next = (k + 1) % len(self._sides)
            if key is not None:
                self._side_of[key] = k
        side = self._sides[k]
        side.stream.wait_stream(self.cur_stream if self.cur_stream is not None else self._main())
        self._dw_keep.append(keep)
        return side

    def _main(self):
        return self.main_stream if self.main_stream is not None else torch.cuda.current_stream(self.dev)

    # y = x W^T + b ; dx (+)= dy W ; dW = dy^T x ; db = colsum(dy)
    def lin_fwd(self, x: MV, W: MV, b, y: MV, act: int = 0, out2: Optional[MV] = None, drop=None):
        """``act`` + ``out2``: y keeps the pre-activation (the backward's reference), out2 = drop(f(y)); ``act`` alone: y = drop(f(.))."""
        self.gemm(x, W, y, False, True, bias=b, act=act, out2=out2, drop=drop)

    def lin_bwd_x(self, dy: MV, W: MV, dx: MV, acc: bool = False, dact: int = 0, ref: Optional[MV] = None, drop=None):
        """``dact`` + ``ref``: dx = (dy W) * f'(ref) (* the dropout mask ``drop`` of the activated tensor): the gradient in front of
        ``drop(f(.))`` in one product."""
        self.gemm(dy, W, dx, False, False, acc=acc, dact=dact, ref=ref, drop=drop)

    def lin_bwd_w(self, dy: MV, x: MV, dW: MV, db: Optional[torch.Tensor] = None, acc: bool = False):
        if not self.async_dw:
            self.gemm(dy, x, dW, True, False, acc=acc, rowsum=db)       # db = column sums of dy = row sums of dy^T, fused into the product
            return
        with self._to_side(dy.t, x.t, dW.t, db, out=dW.t):              # dy (and x) are complete on their stream at this point
            self.gemm(dy, x, dW, True, False, acc=acc, rowsum=db)

    # ---- node stream (forward): the node-row chain of a block (4 600 rows: ten launches, each shorter than its launch latency) runs beside
    #      the pair-row chain instead of in front of it.  Rules that make it safe with torch's caching allocator (all tensors come from
    #      the MAIN stream's pool): every node section starts by waiting for everything the main stream has been given so far (whatever
    #      memory the section allocates was freed before that point, so its earlier users are covered), and nothing a section touches is
    #      freed before the join at the end of the pass (the graph holds the references).
    def node_section(self):
        if self._node is None:
            self._node = _OnStream(self, torch.cuda.Stream(device=self.dev), torch.empty(4 * 1024 * 1024, dtype=torch.float32, device=self.dev))
        self._node.stream.wait_stream(self.main_stream)
        return self._node

    def node_event(self):
        ev = torch.cuda.Event()
        ev.record(self._node.stream)
        return ev

    def main_wait(self, ev=None):
        """The main stream waits for the node stream (as of now) or for one recorded event."""
        if ev is None:
            self.main_stream.wait_stream(self._node.stream)
        else:
            self.main_stream.wait_event(ev)

    def join_dw(self):
        """The main stream waits for every weight-gradient product issued so far; their operands may be reused after it."""
        if self._sides and self._dw_keep:
            main = self._main()
            for side in self._sides:
                main.wait_stream(side.stream)
        self._side_of = {}
        self._dw_keep = []

    def act_fwd(self, x, y, kind):
        E._check(self.lib.dst_act_fwd(ptr(x), ptr(y), x.numel(), kind, self._s()), "dst_act_fwd")

    def act_bwd(self, dy, ref, dx, kind):
        E._check(self.lib.dst_act_bwd(ptr(dy), ptr(ref), ptr(dx), dy.numel(), kind, self._s()), "dst_act_bwd")

    def dropout(self, x, p, seed, stream_id):
        """In place; the same (seed, stream_id) on the gradient is the backward."""
        if p > 0.0:
            E._check(self.lib.dst_dropout(ptr(x), ptr(x), x.numel(), p, seed, stream_id, self._s()),
                     "dst_dropout")

    def axpy(self, a, x, y):
        E._check(self.lib.dst_axpy(a, ptr(x), ptr(y), x.numel(), self._s()), "dst_axpy")

    def lnmod_fwd(self, x, Cc, seg, mul, B, ada, sh, sc, y, stats):
        E._check(self.lib.dst_lnmod_fwd(ptr(x), Cc, ptr(seg), mul, B, ptr(ada), ADA, sh,
                                        sc, ptr(y), ptr(stats), self._s()), "dst_lnmod_fwd")

    def lnmod_bwd(self, dy, x, stats, Cc, seg, mul, B, ada, d_ada, sh, sc, dx, acc):
        E._check(self.lib.dst_lnmod_bwd(ptr(dy), ptr(x), ptr(stats), Cc, ptr(seg), mul, B, ptr(ada),
                                        ptr(d_ada), ADA, sh, sc, ptr(dx), int(acc), ptr(self.scratch),
                                        self.scratch.numel(), self._s()), "dst_lnmod_bwd")

    def gate_add_fwd(self, r, z, Cc, seg, mul, B, ada, g, out):
        E._check(self.lib.dst_gate_add_fwd(ptr(r), ptr(z), Cc, ptr(seg), mul, B, ptr(ada), ADA,
                                           g, ptr(out), self._s()), "dst_gate_add_fwd")

    def pair_chain_fwd(self, TL, u, n2e_bias, e_in, feat, ld_feat, ada, g1, sh, sc, g2, W3, b3, W4, b4, Wed, ld_wed, bed, Wro, bro, drop, out):
        """The pair rows of a block behind the attention as one kernel (``dst_pair_chain_fwd``, bf16 products).  ``drop = (p, seed, stream3,
        stream4)``; ``out``: the block's tape, holding e_out, ed, re_ and - when the tape is kept - he, xe1, st_e2, ye1, f3, s3, f4, X2."""
        _need_bf16(W3, W4, Wed, Wro)
        args = _CHAIN_PACK(*TL.pair_tables, ptr(u), ptr(n2e_bias), ptr(e_in), ptr(feat), ld_feat, ptr(ada), ADA, g1, sh, sc, g2, ptr(W3), ptr(b3), ptr(W4), ptr(b4),
                           ptr(Wed), ld_wed, ptr(bed), ptr(Wro), ptr(bro), float(drop[0]), int(drop[2]), int(drop[3]), 0, int(drop[1]),
                           *(ptr(out.get(k)) for k in ("he", "xe1", "st_e2", "ye1", "f3", "s3", "f4", "e_out", "X2", "ed", "re_")))
        E._check(self.lib.dst_pair_chain_fwd(C.byref(TL.c), args, self._s()), "dst_pair_chain_fwd")

    def node_chain_fwd(self, TL, h_in, attn, ada, g1, sh, sc, g2, W1, b1, W2, b2, Wac, Wn, bn, drop, out):
        """The node rows of a block behind the attention as one kernel (``dst_node_chain_fwd``, bf16 products).  ``drop = (p, seed, stream1,
        stream2)``; ``out``: the block's tape, holding h_out, ac, rn and - when the tape is kept - x1, st_n2, y1, f1, s1, f2."""
        _need_bf16(W1, W2, Wac, Wn)
        args = _NODE_PACK(TL.node_mol_ptr, ptr(h_in), ptr(attn), ptr(ada), ADA, g1, sh, sc, g2, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(Wac), ptr(Wn), ptr(bn),
                          float(drop[0]), int(drop[2]), int(drop[3]), 0, int(drop[1]),
                          *(ptr(out.get(k)) for k in ("x1", "st_n2", "y1", "f1", "s1", "f2", "h_out", "ac", "rn")))
        E._check(self.lib.dst_node_chain_fwd(C.byref(TL.c), args, self._s()), "dst_node_chain_fwd")

    def dir_chain_fwd(self, TL, ac, ed, ada, sh, sc, W0, b0, W2, out):
        """The directed rows of a block as one kernel (``dst_dir_chain_fwd``, bf16 products).  ``out``: the block's tape, holding c2 and - when the tape is
        kept - zz, st_z, zn, c0, sc0."""
        _need_bf16(W0, W2)
        args = _DIR_PACK(*TL.pair_tables, ptr(ac), ptr(ed), ptr(ada), ADA, sh, sc, ptr(W0), ptr(b0), ptr(W2), *(ptr(out.get(k)) for k in ("zz", "st_z", "zn", "c0", "sc0", "c2")))
        E._check(self.lib.dst_dir_chain_fwd(C.byref(TL.c), args, self._s()), "dst_dir_chain_fwd")

    def _part(self, kernel: str, n: int) -> int:
        """Data pointer of the column-sum scratch of fused backward kernel ``kernel`` (at least ``n`` floats; one buffer per kernel, kept and
        grown on demand)."""
        t = self._parts.get(kernel)
        if t is None or t.numel() < n:
            t = self._parts[kernel] = torch.empty(max(n, 1), dtype=torch.float32, device=self.dev)
        return t.data_ptr()

    def pair_chain_bwd(self, TL, de, dro, ld_dro, ded, f4, f3, xe1, st, he, ada, d_ada, g1, sh, sc, g2, WedT, WroT, W4T, W3T, drop, dfeat, df4, df3, de_in, dhe):
        """Backward of the pair rows of a block behind the attention as one kernel + its finishing kernel (``dst_pair_chain_bwd``).  ``dro``: a
        data pointer (the read-out slice's gradient is a column window of a wider tensor) with row stride ``ld_dro``; ``drop = (p, seed, stream3,
        stream4)``."""
        _need_bf16(WedT, WroT, W4T, W3T)
        tt = TL.pair_tiles
        args = _PAIRB_PACK(tt[0], tt[1], tt[2], tt[3], tt[4], ptr(de), int(dro), ld_dro, ptr(ded), ptr(f4), ptr(f3), ptr(xe1), ptr(st), ptr(he), ptr(ada), ptr(d_ada), ADA,
                           g1, sh, sc, g2, ptr(WedT), ptr(WroT), ptr(W4T), ptr(W3T), float(drop[0]), int(drop[2]), int(drop[3]), 0, int(drop[1]),
                           ptr(dfeat), ptr(df4), ptr(df3), ptr(de_in), ptr(dhe), self._part("pair", tt[4] * 256))
        E._check(self.lib.dst_pair_chain_bwd(C.byref(TL.c), args, self._s()), "dst_pair_chain_bwd")

    def node_chain_bwd(self, TL, dh, drn, ld_drn, dac, f2, f1, x1, st, attn, ada, d_ada, g1, sh, sc, g2, WacT, WnT, W2T, W1T, drop, df2, df1, dh_in, dattn):
        """Backward of the node rows of a block behind the attention as one kernel + its finishing kernel (``dst_node_chain_bwd``).  ``drn``: a data
        pointer with row stride ``ld_drn``; ``drop = (p, seed, stream1, stream2)``."""
        _need_bf16(WacT, WnT, W2T, W1T)
        tt = TL.node_tiles
        args = _NODEB_PACK(tt[0], tt[1], tt[2], tt[3], tt[4], ptr(dh), int(drn), ld_drn, ptr(dac), ptr(f2), ptr(f1), ptr(x1), ptr(st), ptr(attn), ptr(ada), ptr(d_ada), ADA,
                           g1, sh, sc, g2, ptr(WacT), ptr(WnT), ptr(W2T), ptr(W1T), float(drop[0]), int(drop[2]), int(drop[3]), 0, int(drop[1]),
                           ptr(df2), ptr(df1), ptr(dh_in), ptr(dattn), self._part("node", tt[4] * 1024))
        E._check(self.lib.dst_node_chain_bwd(C.byref(TL.c), args, self._s()), "dst_node_chain_bwd")

    def dir_chain_bwd(self, TL, dc2, c0, zz, st, ada, d_ada, sh, sc, W2, W0T, dc0, dz):
        """Backward of the directed rows of a block as one kernel + its finishing kernel (``dst_dir_chain_bwd``)."""
        _need_bf16(W0T)
        assert W2.dtype == torch.float32
        tt = TL.dir_tiles
        args = _DIRB_PACK(tt[0], tt[1], tt[2], tt[3], tt[4], dc2.data_ptr(), c0.data_ptr(), zz.data_ptr(), st.data_ptr(), ada.data_ptr(), d_ada.data_ptr(), ADA, sh, sc,
                          W2.data_ptr(), W0T.data_ptr(), dc0.data_ptr(), dz.data_ptr(), self._part("dir", tt[4] * 512))
        E._check(self.lib.dst_dir_chain_bwd(C.byref(TL.c), args, self._s()), "dst_dir_chain_bwd")

    def pair_front_fwd(self, TL, pos, ada, dist_off, sh, sc, means, stds, e_in, Wee, bee, Wte, out):
        """The pair rows of a block in front of the attention as one kernel (``dst_pair_front_fwd``, bf16 products).  ``out``: the block's tape, holding X1, te
        and - when the tape is kept - xs, d2, e1, st_e1, en."""
        _need_bf16(Wee, Wte)
        args = _FRONT_PACK(*TL.pair_tables, ptr(pos), ptr(ada), ADA, dist_off, sh, sc, 0, ptr(means), ptr(stds), ptr(e_in), ptr(Wee), ptr(bee), ptr(Wte),
                           *(ptr(out.get(k)) for k in ("X1", "xs", "d2", "e1", "st_e1", "en", "te")))
        E._check(self.lib.dst_pair_front_fwd(C.byref(TL.c), args, self._s()), "dst_pair_front_fwd")

    def geom_fwd(self, TL, pos, ada, dist_off, means, stds, X, ldx, col0, xs, d2s):
        E._check(self.lib.dst_geom_fwd(C.byref(TL.c), ptr(pos), ptr(ada), ADA, dist_off, ptr(means), ptr(stds),
                                       X.data_ptr() + 4 * col0, ldx, ptr(xs), ptr(d2s), self._s()), "dst_geom_fwd")

    def geom_bwd(self, TL, pos, ada, d_ada, dist_off, means, stds, xs, d2s, g1, g2, dms, dd2, dpos):
        E._check(self.lib.dst_geom_bwd(C.byref(TL.c), ptr(pos), ptr(ada), ptr(d_ada), ADA, dist_off, ptr(means),
                                       ptr(stds), ptr(xs), ptr(d2s), ptr(g1), g1.shape[1], ptr(g2),
                                       0 if g2 is None else g2.shape[1], ptr(dms), ptr(dd2), ptr(dpos), self._s()), "dst_geom_bwd")

    def gate_add_bwd(self, dout, z, Cc, seg, mul, B, ada, d_ada, g, dr, acc_r, dz, drop=None):
        """``drop = (p, seed, stream_id)``: ``z`` was a dropout's output; ``dz`` is then the gradient in FRONT of that dropout."""
        p_, seed, stream = drop if drop and drop[0] > 0 else (0.0, 0, 0)
        E._check(self.lib.dst_gate_add_bwd(ptr(dout), ptr(z), Cc, ptr(seg), mul, B, ptr(ada), ptr(d_ada),
                                           ADA, g, ptr(dr), int(acc_r), ptr(dz), p_, seed,
                                           stream, self._s()), "dst_gate_add_bwd")


class _OnStream:
    """A stream of its own with its own scratch: inside ``with``, the launches of ``Ops`` go to it.  One object per stream, entered by one
    ``with`` at a time (the node stream and each weight-gradient stream; a weight-gradient product may be issued from inside a node section)."""
    __slots__ = ("o", "stream", "ptr", "scratch", "saved")

    def __init__(self, ops, stream, scratch):
        self.o, self.stream, self.ptr, self.scratch = ops, stream, stream.cuda_stream, scratch

    def __enter__(self):
        o = self.o
        self.saved = (o.stream_ptr, o.scratch, o.cur_stream)
        o.stream_ptr, o.scratch, o.cur_stream = self.ptr, self.scratch, self.stream
        return self

    def __exit__(self, *exc):
        self.o.stream_ptr, self.o.scratch, self.o.cur_stream = self.saved
        return False


class TrainLayout:
    """The packed-ragged tables of ``engine.Layout`` plus what the training kernels need (dense <-> packed index tensors)."""

    def __init__(self, node_mask: torch.Tensor, device):
        self.L = E.Layout(node_mask, device)
        L = self.L
        self.B, self.N, self.Nn, self.Pp = L.B, L.N, L.Nn, L.Pp
        self.c = DstLayout(B=L.B, Nn=L.Nn, Pp=L.Pp, _pad=0, node_off=L.t["node_off"].data_ptr(), pair_off=L.t["pair_off"].data_ptr())
        nd = L.t["node_dense"].long()
        a, b = L.t["pair_a"].long(), L.t["pair_b"].long()
        self.node_dense = nd                                              # [Nn] -> row of the dense [B*N] node arrays
        self.pair_dense = nd[a] * L.N + (nd[b] % L.N)                     # [Pp] -> row (b, i, j) of the dense [B*N*N] edge arrays, i < j
        self.pair_dense_t = nd[b] * L.N + (nd[a] % L.N)                   # the transposed cell (b, j, i)
        self.node_mol = L.t["node_mol"].long()
        self.pair_mol = L.t["pair_mol"].long()
        self.node_off, self.pair_off = L.t["node_off"], L.t["pair_off"]
        # device tables of the flat-tile kernels (dst_pair_*_fwd, dst_dir_chain_fwd): node rows of a pair's atoms, its molecule
        self.pair_tables = (L.t["pair_a"].data_ptr(), L.t["pair_b"].data_ptr(), L.t["pair_mol"].data_ptr())
        self.node_mol_ptr = L.t["node_mol"].data_ptr()                     # [Nn] int32: molecule of a node row (dst_node_chain_fwd)
        # molecule-aligned 32-row tiles of the pair rows, the DIRECTED rows and the node rows (dst_pair_chain_bwd / dst_dir_chain_bwd /
        # dst_node_chain_bwd: their adaLN sums are per molecule): (first row, row count, molecule) per tile, first tile per molecule, number of tiles
        po = L.t["pair_off"].cpu().numpy().astype(np.int64)
        i32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=device)
        self._tile_tensors = []
        no = L.t["node_off"].cpu().numpy().astype(np.int64)
        for mul, name in ((1, "pair_tiles"), (2, "dir_tiles"), (0, "node_tiles")):
            row0, rows, mol, off = [], [], [], [0]
            for m in range(L.B):
                nr, r0 = (mul * int(po[m + 1] - po[m]), mul * int(po[m])) if mul else (int(no[m + 1] - no[m]), int(no[m]))
                for k in range(0, nr, 32):
                    row0.append(r0 + k); rows.append(min(32, nr - k)); mol.append(m)
                off.append(len(row0))
            tens = (i32(row0), i32(rows), i32(mol), i32(off))
            self._tile_tensors.append(tens)
            setattr(self, name, tuple(t.data_ptr() for t in tens) + (len(row0),))

    def pack_nodes(self, dense: torch.Tensor) -> torch.Tensor:
        return dense.reshape(self.B * self.N, -1).index_select(0, self.node_dense).contiguous()

    def pack_pairs(self, dense: torch.Tensor) -> torch.Tensor:
        return dense.reshape(self.B * self.N * self.N, -1).index_select(0, self.pair_dense).contiguous()

    def unpack_nodes(self, packed: torch.Tensor) -> torch.Tensor:
        out = torch.zeros(self.B * self.N, packed.shape[1], dtype=packed.dtype, device=packed.device)
        out[self.node_dense] = packed
        return out.reshape(self.B, self.N, -1)

    def unpack_pairs(self, packed: torch.Tensor) -> torch.Tensor:
        out = torch.zeros(self.B * self.N * self.N, packed.shape[1], dtype=packed.dtype, device=packed.device)
        out[self.pair_dense] = packed
        out[self.pair_dense_t] = packed
        return out.reshape(self.B, self.N, self.N, -1)


ADA_PARTS = (("node_time_mlp.1", NODE_OFF, 1536), ("edge_time_mlp.1", EDGE_OFF, 384), ("equi_update.time_mlp.1", EQUI_OFF, 512),
             ("dist_layer.time_mlp.1", DIST_OFF, 2))

DROP_ROW = (512, 256, 128, 64)     # row length of a block's four dropout masks: behind ff_linear1, ff_linear2 (node rows), ff_linear3, ff_linear4 (pair rows)


def _row_slots(base: int, width: int) -> SimpleNamespace:
    """adaLN columns of the node or the pair rows of a block: ``ln1 = (shift, scale)`` in front of the attention and ``gate1`` behind it,
    ``ln2`` / ``gate2`` around the FF; ``width`` columns each, in the order the *time_mlp produces them."""
    return SimpleNamespace(ln1=(base, base + width), gate1=base + 2 * width, ln2=(base + 3 * width, base + 4 * width), gate2=base + 5 * width)


class BlockSlots:
    """What block ``i`` is called by: its parameter prefix, its columns of the adaLN table and its Philox dropout streams."""
    __slots__ = ("i", "bp", "node", "edge", "equi_ln", "dist")

    def __init__(self, i: int):
        a0 = i * ADA_STRIDE
        self.i, self.bp = i, f"e_block_{i}."
        self.node, self.edge = _row_slots(a0 + NODE_OFF, 256), _row_slots(a0 + EDGE_OFF, 64)
        self.equi_ln = (a0 + EQUI_OFF, a0 + EQUI_OFF + 256)        # (shift, scale) of the directed rows
        self.dist = a0 + DIST_OFF                                  # (scale, shift) pair of the distance features

    def drop(self, k: int) -> Tuple[int, int]:
        """(stream id, row length) of dropout ``k`` of the block (``DROP_ROW``)."""
        return 4 * self.i + k, DROP_ROW[k]


BLOCKS = tuple(BlockSlots(i) for i in range(NB))

# bf16 copies of a block's weights for the fused row chains (leading dimension NB): (name, shape, source, transposed).  Source: a parameter
# name ({i} = block), (parameter name, first column, end column), or "cat.X" = block i of the concatenated buffer X.  The transposed copies
# ([in][out]) are the B operands of the input-gradient products of the fused backward kernels.  The order is the order of the device table.
_BP = "e_block_{i}."
BF16_WEIGHTS = (
    ("W3", (128, 64), _BP + "ff_linear3.weight", False), ("W4", (64, 128), _BP + "ff_linear4.weight", False),
    ("Wed", (256, 128), (_BP + "equi_update.input_lin.weight", 512, 640), False), ("Wro", (16, 64), "edge_{i}.weight", False),
    ("Wee", (64, 128), _BP + "edge_emb.weight", False), ("Wte", (512, 64), "cat.Wte", False),
    ("W0", (256, 256), _BP + "equi_update.coord_mlp.0.weight", False), ("W2", (3, 256), _BP + "equi_update.coord_mlp.2.weight", False),
    ("F1", (512, 256), _BP + "ff_linear1.weight", False), ("F2", (256, 512), _BP + "ff_linear2.weight", False),
    ("Wac", (512, 256), "cat.Wac", False), ("Wn", (64, 256), "node_{i}.weight", False),
    ("W0T", (256, 256), _BP + "equi_update.coord_mlp.0.weight", True), ("WedT", (128, 256), (_BP + "equi_update.input_lin.weight", 512, 640), True),
    ("WroT", (64, 16), "edge_{i}.weight", True), ("W4T", (128, 64), _BP + "ff_linear4.weight", True),
    ("W3T", (64, 128), _BP + "ff_linear3.weight", True), ("WacT", (256, 512), "cat.Wac", True), ("WnT", (256, 64), "node_{i}.weight", True),
    ("F2T", (512, 256), _BP + "ff_linear2.weight", True), ("F1T", (256, 512), _BP + "ff_linear1.weight", True))


def _bf16_source(src, i: int, p, cat) -> torch.Tensor:
    if isinstance(src, tuple):
        return p[src[0].format(i=i)][:, src[1]:src[2]]
    return cat[src[4:]][i] if src.startswith("cat.") else p[src.format(i=i)]


class DmtTrainGraph:
    """Forward tape and backward of one DMT evaluation (conditioning embedding given) on packed tensors.

    ``params``: name -> fp32 device tensor (reference names, no ``module.`` prefix).  ``backward`` returns the gradients under the same
    names: views of the gradient stage given to ``bind``, or - stand-alone - fresh tensors.  ``ops``: the caller's ``Ops`` (a trainer shares
    one between its graphs); None makes one."""

    def __init__(self, params: Dict[str, torch.Tensor], config, device, ops: Optional[Ops] = None):
        self.cfg = config
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("the training graph runs on an MI355X only; diffspectra_amd has no CPU path")
        self.ops = ops if ops is not None else Ops(self.dev)
        self.lib = self.ops.lib
        self.edge_th = float(config.model.edge_quan_th)
        self.cutoff = float(config.model.spatial_cut_off)
        self.p, self.gbuf = params, None       # bind()
        self.cat = self.dcat = self.wb = None  # prepare_weights(): concatenated weights, their gradients, the bf16 copies of the fused chains
        self._cat_cache: dict = {}             # those buffers and the device tables of their piece copies, kept over the calls
        self.t = None                          # the tape of the last forward(save=True), consumed by backward
        # FF dropout of the training forward (dmt.py:114-120): probability and the seed of this evaluation's Philox streams; 0 = identity
        self.dropout_p = 0.0
        self.dropout_seed = 0

    def bind(self, params: Dict[str, torch.Tensor], gbuf: Optional[Dict[str, torch.Tensor]] = None):
        """This call's parameter storage and the views of the gradient stage its backward writes into (None: fresh tensors).  A forward
        keeps its binding in its tape and ``backward`` returns to it, so a backward may follow a later forward of the same graph (whoever
        wants that keeps the tape: a new binding drops it)."""
        self.p, self.gbuf, self.t = params, gbuf, None

    # ------------------------------------------------------------------ helpers
    def f(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def z(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.dev)

    # ---- concatenated weights: Linears that read the same input are evaluated as ONE product (q | k | v; lin_edge0 | lin_edge1; the row | col
    #      parts of input_lin; every *time_mlp as the adaLN table) from per-step copies of the parameters in one buffer each.  The copies are
    #      two multi-tensor launches per step (torch._foreach_copy_), the gradients of the concatenated buffers are scattered back the same way.
    @staticmethod
    def cat_plan():
        """[(buffer name, shape)], [(buffer name, index expression, parameter name)] - where every parameter piece lives in its buffer."""
        bufs = [("Wada", (ADA, 1024)), ("bada", (ADA,)), ("Wqkv", (NB, 768, 256)), ("bqkv", (NB, 768)), ("Wte", (NB, 512, 64)), ("Wac", (NB, 512, 256))]
        pieces = []
        for blk in range(NB):
            bp = f"e_block_{blk}."
            for name, off, rows in ADA_PARTS:
                o = blk * ADA_STRIDE + off
                pieces.append(("Wada", (slice(o, o + rows),), bp + name + ".weight"))
                pieces.append(("bada", (slice(o, o + rows),), bp + name + ".bias"))
            for k, nm in enumerate(("lin_query", "lin_key", "lin_value")):
                rows = 252 if k < 2 else 256
                pieces.append(("Wqkv", (blk, slice(256 * k, 256 * k + rows)), bp + f"attn_mpnn.{nm}.weight"))
                pieces.append(("bqkv", (blk, slice(256 * k, 256 * k + rows)), bp + f"attn_mpnn.{nm}.bias"))
            pieces.append(("Wte", (blk, slice(0, 252)), bp + "attn_mpnn.lin_edge0.weight"))
            pieces.append(("Wte", (blk, slice(256, 512)), bp + "attn_mpnn.lin_edge1.weight"))
            pieces.append(("Wac", (blk, slice(0, 256)), (bp + "equi_update.input_lin.weight", slice(0, 256))))      # h_row part (columns 0..255)
            pieces.append(("Wac", (blk, slice(256, 512)), (bp + "equi_update.input_lin.weight", slice(256, 512))))  # h_col part
        pieces.append(("Wada", (slice(ADA_TOP, ADA_TOP + 2),), "dist_layer.time_mlp.1.weight"))
        pieces.append(("bada", (slice(ADA_TOP, ADA_TOP + 2),), "dist_layer.time_mlp.1.bias"))
        return bufs, pieces

    def _piece_views(self, bufs, tensors):
        """(views into the concatenated buffers, the matching parameter(-shaped) tensors) in plan order."""
        _, pieces = self.cat_plan()
        dst, src = [], []
        for bname, idx, pname in pieces:
            dst.append(bufs[bname][idx])
            if isinstance(pname, tuple):
                src.append(tensors[pname[0]][:, pname[1]])
            else:
                src.append(tensors[pname])
        return dst, src

    def prepare_weights(self):
        """Fill the concatenated weight buffers from the current parameters (once per step: both forwards of a step share them)."""
        cache = self._cat_cache
        if "bufs" not in cache:
            shapes, _ = self.cat_plan()
            cache["bufs"] = {n: self.z(*shape) for n, shape in shapes}          # padding rows (252..255 of q / k / lin_edge0) stay zero
            cache["grads"] = {n: self.z(*shape) for n, shape in shapes}
        dst, src = self._piece_views(cache["bufs"], self.p)
        copy_pieces(self.lib, self.dev, dst, src, cache, "table_fwd", self.ops._s())
        self.cat, self.dcat = cache["bufs"], cache["grads"]
        if self.ops.bf16:
            # the fused row chains take their weights as bf16 (csrc/ds_train_chain.hip: the per-tile weight stream from L2 bounds them)
            if "wb" not in cache:
                cache["wb"] = {n: torch.zeros(NB, *sh, dtype=torch.bfloat16, device=self.dev) for n, sh, _, _ in BF16_WEIGHTS}
            wb = cache["wb"]
            dst = [wb[n][i] for i in range(NB) for n, _, _, _ in BF16_WEIGHTS]
            src = [_bf16_source(s_, i, self.p, cache["bufs"]) for i in range(NB) for _, _, s_, _ in BF16_WEIGHTS]
            tset = {j for j in range(len(dst)) if BF16_WEIGHTS[j % len(BF16_WEIGHTS)][3]}
            pack_bf16_pieces(self.lib, self.dev, dst, src, cache, "table_bf16", self.ops._s(), key_t=tset)
            self.wb = wb

    def scatter_cat_grads(self, g, gw):
        """Gradients of the concatenated buffers -> the parameters' gradient buffers (input_lin's edge part and bias are written directly).
        ``g``: the gradients the backward has handed out so far, ``gw``: its way to the buffer of one it has not."""
        _, pieces = self.cat_plan()
        tgt = {}
        for _, _, pname in pieces:
            name = pname[0] if isinstance(pname, tuple) else pname
            if name not in tgt:
                tgt[name] = g[name] if name in g else gw(name)
        src, dst = self._piece_views(self.dcat, tgt)
        copy_pieces(self.lib, self.dev, dst, src, self._cat_cache, "table_bwd", self.ops._s())

    # ------------------------------------------------------------------ forward
    def forward(self, TL: TrainLayout, xn, ex, noise_level, ctx_emb, cond_n=None, cond_e=None, save: bool = True):
        """``xn [Nn,9]`` / ``ex [Pp,2]`` packed noisy state, ``noise_level [B]``, ``ctx_emb [B,1024]`` = cond_lin(SpecFormer(context)),
        ``cond_n`` / ``cond_e`` packed self-conditioning prediction or None (dmt.py:332-345).  Returns (pos [Nn,3], atom_pred [Nn,6],
        edge_pred [Pp,2]) and keeps the tape in ``self.t`` when ``save``."""
        o, p, lib = self.ops, self.p, self.lib
        B, Nn, Pp = TL.B, TL.Nn, TL.Pp
        t: Dict[str, object] = dict(TL=TL, first=cond_n is None, drop=(self.dropout_p, self.dropout_seed), bound=(self.p, self.gbuf))
        s = self.ops._s
        # ---- time embedding + adaLN table (dmt.py:249-257,353-357; every *time_mlp)
        tf = self.f(B, 17)
        E._check(lib.dst_time_feat_fwd(ptr(noise_level), ptr(p["time_mlp.0.weights"]), B, ptr(tf), s()), "dst_time_feat_fwd")
        tm1, tg, temb, st = self.f(B, 1024), self.f(B, 1024), self.f(B, 1024), self.f(B, 1024)
        o.lin_fwd(mv(tf), mv(p["time_mlp.1.weight"]), p["time_mlp.1.bias"], mv(tm1), act=GELU, out2=mv(tg))
        o.lin_fwd(mv(tg), mv(p["time_mlp.3.weight"]), p["time_mlp.3.bias"], mv(temb))
        o.axpy(1.0, ctx_emb, temb)                                                       # time_emb = time_mlp(noise_level) + context
        o.act_fwd(temb, st, SILU)
        if self.cat is None:
            self.prepare_weights()
        cat = self.cat
        ada = self.f(B, ADA)
        o.lin_fwd(mv(st), mv(cat["Wada"]), cat["bada"], mv(ada))
        t.update(noise_level=noise_level, tf=tf, tm1=tm1, tg=tg, temb=temb, st=st, ada=ada)
        # ---- inputs (dmt.py:323-377)
        pos = xn[:, 0:3].contiguous()
        X0n = torch.cat([xn[:, 3:9], cond_n[:, 3:9] if cond_n is not None else torch.zeros_like(xn[:, 3:9])], dim=1).contiguous()
        h = self.f(Nn, 256)
        o.lin_fwd(mv(X0n), mv(p["node_emb.weight"]), p["node_emb.bias"], mv(h))
        X0p = self.z(Pp, 68)
        X0p[:, 0:2] = ex
        xs0 = d2c = None
        if cond_n is not None:
            X0p[:, 2:4] = cond_e
            cpos = cond_n[:, 0:3].contiguous()
            xs0, d2c = self.f(Pp), self.f(Pp)
            o.geom_fwd(TL, cpos, ada, ADA_TOP, p["dist_layer.means.weight"], p["dist_layer.stds.weight"], X0p, 68, 4, xs0, d2c)
            adj = torch.empty(Pp, dtype=torch.int32, device=self.dev)
            E._check(lib.dst_adj_bits(ptr(cond_e), cond_e.shape[1], ptr(d2c), self.edge_th, self.cutoff, Pp,
                                      ptr(adj), s()), "dst_adj_bits")
            t.update(cpos=cpos)
        else:
            adj = torch.full((Pp,), 3, dtype=torch.int32, device=self.dev)
        e = self.f(Pp, 64)
        o.lin_fwd(mv(X0p), mv(p["edge_emb.weight"]), p["edge_emb.bias"], mv(e))
        t.update(X0n=X0n, X0p=X0p, xs0=xs0, d2c=d2c, adj=adj, h0=h, e0=e)
        node_hids, edge_hids = [h], [e]
        blocks = []
        ns, _ = o.stream_modes()
        # fused row chains: bf16 mode only (their products are bf16 MFMAs; the fp32 mode keeps the per-operation kernels golden G13 / G17 pin)
        fused_chain = bool(o.bf16) and Pp > 0 and os.environ.get("DIFFSPECTRA_FUSED_CHAIN", "1") != "0"
        t.update(node_stream=ns, fused_chain=fused_chain)        # the backward walks this tape with the same choices
        for k in BLOCKS:
            # (the tape of a block is kept in every mode: with the node stream nothing a block touched may be freed - and handed out
            # again - before the join below)
            bt: Dict[str, object] = dict(pos_in=pos, h_in=h, e_in=e)
            pos = self._block_fwd(t, k, bt, save)
            h, e = bt["h_out"], bt["e_out"]
            node_hids.append(bt["rn"])
            edge_hids.append(bt["re_"])
            blocks.append(bt)
        if ns:
            o.main_wait()                                            # join: the last block's node rows and read-out slices
        # ---- read-out MLPs (dmt.py:391-394)
        AH = torch.cat(node_hids, dim=1).contiguous()
        EH = torch.cat(edge_hids, dim=1).contiguous()
        n1, n1s, n2, n2s, atom_pred = self.f(Nn, 256), self.f(Nn, 256), self.f(Nn, 128), self.f(Nn, 128), self.f(Nn, 6)
        o.lin_fwd(mv(AH), mv(p["node_pred_mlp.0.weight"]), p["node_pred_mlp.0.bias"], mv(n1), act=SILU, out2=mv(n1s))
        o.lin_fwd(mv(n1s), mv(p["node_pred_mlp.2.weight"]), p["node_pred_mlp.2.bias"], mv(n2), act=SILU, out2=mv(n2s))
        o.lin_fwd(mv(n2s), mv(p["node_pred_mlp.4.weight"]), p["node_pred_mlp.4.bias"], mv(atom_pred))
        edge_pred = self.f(Pp, 2)
        ro = {}
        for col, name in ((0, "edge_exist_mlp"), (1, "edge_type_mlp")):
            a1, a1s, a2, a2s = self.f(Pp, 64), self.f(Pp, 64), self.f(Pp, 32), self.f(Pp, 32)
            o.lin_fwd(mv(EH), mv(p[name + ".0.weight"]), p[name + ".0.bias"], mv(a1), act=SILU, out2=mv(a1s))
            o.lin_fwd(mv(a1s), mv(p[name + ".2.weight"]), p[name + ".2.bias"], mv(a2), act=SILU, out2=mv(a2s))
            o.lin_fwd(mv(a2s), mv(p[name + ".4.weight"]), p[name + ".4.bias"], mv(edge_pred, col, col + 1))
            ro[name] = (a1, a1s, a2, a2s)
        if save:
            t.update(blocks=blocks, AH=AH, EH=EH, n1=n1, n1s=n1s, n2=n2, n2s=n2s, ro=ro, pos_final=pos)
            self.t = t
        return pos, atom_pred, edge_pred

    # ---- one block, forward.  ``t``: the pass so far (layout, adaLN table, adjacency bits, stream and chain choices), ``k``: the block's slots,
    #      ``bt``: its tape, holding pos_in / h_in / e_in on entry and every tensor the block made on return.  The stream choreography is here
    #      and only here; the row chains it orders follow in their two forms - ``_fused``: one dst_*_chain_* launch (csrc/ds_train_chain.hip),
    #      ``_ops``: the per-operation kernels - which read and write the same entries of ``bt``.  A fused chain without ``save`` (the
    #      self-conditioning pass) writes only what the rest of the forward reads; the tape-only entries are then absent.
    def _block_fwd(self, t, k: BlockSlots, bt, save: bool):
        o, p, lib, s = self.ops, self.p, self.lib, self.ops._s
        TL, ada, adj, ns, drop = t["TL"], t["ada"], t["adj"], t["node_stream"], t["drop"]
        Nn, D = TL.Nn, 2 * TL.Pp
        sec = o.node_section if ns else contextlib.nullcontext
        pair_front, node_rear, pair_rear, dir_rows = ((self._pair_front_fwd_fused, self._node_rear_fwd_fused, self._pair_rear_fwd_fused, self._dir_fwd_fused)
                                                      if t["fused_chain"] else
                                                      (self._pair_front_fwd_ops, self._node_rear_fwd_ops, self._pair_rear_fwd_ops, self._dir_fwd_ops))
        # node rows in front of the attention on the node stream, beside the pair rows' geometry and embedding
        with sec():
            self._node_front_fwd(TL, ada, k, bt)
        pair_front(TL, ada, k, bt, save)
        te = bt["te"]
        # attention (layers.py:131-186)
        if ns:
            o.main_wait()                                        # q | k | v
        attn, alpha = self.f(Nn, 256), self.f(max(D, 1), 16)
        E._check(lib.dst_attn_fwd(C.byref(TL.c), ptr(bt["qkv"]), ptr(te[:, 0:256]), ptr(te[:, 256:512]), 512, ptr(adj), ptr(attn),
                                  ptr(alpha), s()), "dst_attn_fwd")
        bt.update(attn=attn, alpha=alpha)
        # node stream (dmt.py:156-163): node2edge per node first (the pair rows wait for it), then the node rows behind the attention (the
        # directed rows wait for their `ac`, not for the read-out slice behind it)
        with sec():
            u = bt["u"] = self.f(Nn, 64)
            o.lin_fwd(mv(attn), mv(p[k.bp + "node2edge_lin.weight"]), None, mv(u))
            ev_u = o.node_event() if ns else None
            ev_ac = node_rear(TL, ada, k, bt, drop, save, o.node_event if ns else (lambda: None))
        # edge stream (dmt.py:156-157,165-169)
        if ns:
            o.main_wait(ev_u)
        pair_rear(TL, ada, k, bt, drop, save)
        if ns:
            o.main_wait(ev_ac)
        dir_rows(TL, ada, k, bt, save)
        pos_out = self.f(Nn, 3)
        E._check(lib.dst_coord_fwd(C.byref(TL.c), ptr(bt["pos_in"]), ptr(bt["c2"]), ptr(adj), ptr(p[k.bp + "equi_update.coord_norm.scale"]),
                                   ptr(pos_out), s()), "dst_coord_fwd")
        return pos_out

    def _node_front_fwd(self, TL, ada, k, bt):
        """Node rows in front of the attention (dmt.py:148; layers.py:131-140): adaLN modulate, q | k | v as one product (the padding columns
        come out as exact zeros).  Tape: hn, st_n1, qkv."""
        o, cat, i = self.ops, self.cat, k.i
        hn, st_n1 = self.f(TL.Nn, 256), self.f(TL.Nn, 2)
        o.lnmod_fwd(bt["h_in"], 256, TL.node_off, 1, TL.B, ada, *k.node.ln1, hn, st_n1)
        qkv = self.f(TL.Nn, 768)
        o.lin_fwd(mv(hn), mv(cat["Wqkv"][i]), cat["bqkv"][i], mv(qkv))
        bt.update(hn=hn, st_n1=st_n1, qkv=qkv)

    # pair rows in front of the attention: distances + CondGaussian features, edge embedding, adaLN modulate, both lin_edge projections
    # (dmt.py:136-139,145-149).  Tape: X1, te and xs, d2, e1, st_e1, en.
    def _pair_front_fwd_fused(self, TL, ada, k, bt, save):
        p, bp, i, Pp = self.p, k.bp, k.i, TL.Pp
        bt.update(X1=self.f(Pp, 128), te=self.f(Pp, 512))
        if save:
            bt.update(xs=self.f(Pp), d2=self.f(Pp), e1=self.f(Pp, 64), st_e1=self.f(Pp, 2), en=self.f(Pp, 64))
        self.ops.pair_front_fwd(TL, bt["pos_in"], ada, k.dist, *k.edge.ln1, p[bp + "dist_layer.means.weight"], p[bp + "dist_layer.stds.weight"], bt["e_in"],
                                self.wb["Wee"][i], p[bp + "edge_emb.bias"], self.wb["Wte"][i], bt)

    def _pair_front_fwd_ops(self, TL, ada, k, bt, save):
        o, p, bp, Pp = self.ops, self.p, k.bp, TL.Pp
        X1, xs, d2 = self.f(Pp, 128), self.f(Pp), self.f(Pp)
        o.geom_fwd(TL, bt["pos_in"], ada, k.dist, p[bp + "dist_layer.means.weight"], p[bp + "dist_layer.stds.weight"], X1, 128, 0, xs, d2)
        X1[:, 64:128] = bt["e_in"]
        e1 = self.f(Pp, 64)
        o.lin_fwd(mv(X1), mv(p[bp + "edge_emb.weight"]), p[bp + "edge_emb.bias"], mv(e1))
        en, st_e1 = self.f(Pp, 64), self.f(Pp, 2)
        o.lnmod_fwd(e1, 64, TL.pair_off, 1, TL.B, ada, *k.edge.ln1, en, st_e1)
        te = self.f(Pp, 512)                                     # tanh(lin_edge0 e) | tanh(lin_edge1 e) as one product; columns 252..255 = tanh(0)
        o.lin_fwd(mv(en), mv(self.cat["Wte"][k.i]), None, mv(te), act=TANH)
        bt.update(X1=X1, te=te, xs=xs, d2=d2, e1=e1, st_e1=st_e1, en=en)

    # node rows behind the attention: gated residual, LayerNorm + modulate, the FF with its two dropouts, gated residual, the node parts of
    # input_lin and the read-out slice (dmt.py:113-116,158-163,387).  ``drop = (p, seed)``; returns ``ac_ready()``, called once `ac` is in the
    # stream (the node stream's event for it).  Tape: h_out, ac, rn and x1, st_n2, y1, f1, s1, f2.
    def _node_rear_fwd_fused(self, TL, ada, k, bt, drop, save, ac_ready):
        p, wb, bp, i, Nn = self.p, self.wb, k.bp, k.i, TL.Nn
        bt.update(h_out=self.f(Nn, 256), ac=self.f(Nn, 512), rn=self.f(Nn, 64))
        if save:
            bt.update(x1=self.f(Nn, 256), st_n2=self.f(Nn, 2), y1=self.f(Nn, 256), f1=self.f(Nn, 512), s1=self.f(Nn, 512), f2=self.f(Nn, 256))
        self.ops.node_chain_fwd(TL, bt["h_in"], bt["attn"], ada, k.node.gate1, *k.node.ln2, k.node.gate2, wb["F1"][i], p[bp + "ff_linear1.bias"],
                                wb["F2"][i], p[bp + "ff_linear2.bias"], wb["Wac"][i], wb["Wn"][i], p[f"node_{i}.bias"],
                                (*drop, k.drop(0)[0], k.drop(1)[0]), bt)
        return ac_ready()

    def _node_rear_fwd_ops(self, TL, ada, k, bt, drop, save, ac_ready):
        o, p, bp, i, B, Nn = self.ops, self.p, k.bp, k.i, TL.B, TL.Nn
        x1, y1, st_n2 = self.f(Nn, 256), self.f(Nn, 256), self.f(Nn, 2)
        o.gate_add_fwd(bt["h_in"], bt["attn"], 256, TL.node_off, 1, B, ada, k.node.gate1, x1)
        o.lnmod_fwd(x1, 256, TL.node_off, 1, B, ada, *k.node.ln2, y1, st_n2)
        f1, s1, f2, h_out = self.f(Nn, 512), self.f(Nn, 512), self.f(Nn, 256), self.f(Nn, 256)
        # dmt.py:114-116: dropout(act(ff_linear1)) and dropout(ff_linear2) where the GEMMs produce them (f1 = pre-activation, kept)
        o.lin_fwd(mv(y1), mv(p[bp + "ff_linear1.weight"]), p[bp + "ff_linear1.bias"], mv(f1), act=SILU, out2=mv(s1), drop=(*drop, *k.drop(0)))
        o.lin_fwd(mv(s1), mv(p[bp + "ff_linear2.weight"]), p[bp + "ff_linear2.bias"], mv(f2), drop=(*drop, *k.drop(1)))
        o.gate_add_fwd(y1, f2, 256, TL.node_off, 1, B, ada, k.node.gate2, h_out)
        ac = self.f(Nn, 512)                                 # h_row | h_col parts of input_lin as one product
        o.lin_fwd(mv(h_out), mv(self.cat["Wac"][i]), None, mv(ac))
        ev_ac = ac_ready()
        rn = self.f(Nn, 64)                                  # per-block read-out features (dmt.py:387)
        o.lin_fwd(mv(h_out), mv(p[f"node_{i}.weight"]), p[f"node_{i}.bias"], mv(rn))
        bt.update(h_out=h_out, ac=ac, rn=rn, x1=x1, st_n2=st_n2, y1=y1, f1=f1, s1=s1, f2=f2)
        return ev_ac

    # pair rows behind the attention: node2edge sum, gated residual, LayerNorm + modulate, the FF with its two dropouts, gated residual, the
    # edge part of input_lin and the read-out slice (dmt.py:156-157,165-169,388).  Tape: e_out, ed, re_ and he, xe1, st_e2, ye1, f3, s3, f4, X2.
    def _pair_rear_fwd_fused(self, TL, ada, k, bt, drop, save):
        p, wb, bp, i, Pp = self.p, self.wb, k.bp, k.i, TL.Pp
        bt.update(e_out=self.f(Pp, 64), ed=self.f(Pp, 256), re_=self.f(Pp, 16))
        if save:
            bt.update(he=self.f(Pp, 64), xe1=self.f(Pp, 64), st_e2=self.f(Pp, 2), ye1=self.f(Pp, 64), f3=self.f(Pp, 128), s3=self.f(Pp, 128),
                      f4=self.f(Pp, 64), X2=self.f(Pp, 128))
        self.ops.pair_chain_fwd(TL, bt["u"], p[bp + "node2edge_lin.bias"], bt["e_in"], bt["X1"], 128, ada, k.edge.gate1, *k.edge.ln2, k.edge.gate2,
                                wb["W3"][i], p[bp + "ff_linear3.bias"], wb["W4"][i], p[bp + "ff_linear4.bias"], wb["Wed"][i], 128,
                                p[bp + "equi_update.input_lin.bias"], wb["Wro"][i], p[f"edge_{i}.bias"], (*drop, k.drop(2)[0], k.drop(3)[0]), bt)

    def _pair_rear_fwd_ops(self, TL, ada, k, bt, drop, save):
        o, p, bp, i, B, Pp = self.ops, self.p, k.bp, k.i, TL.B, TL.Pp
        he = self.f(Pp, 64)
        E._check(self.lib.dst_pair_sum_fwd(C.byref(TL.c), ptr(bt["u"]), 64, ptr(p[bp + "node2edge_lin.bias"]), ptr(he), o._s()),
                 "dst_pair_sum_fwd")
        xe1, ye1, st_e2 = self.f(Pp, 64), self.f(Pp, 64), self.f(Pp, 2)
        o.gate_add_fwd(bt["e_in"], he, 64, TL.pair_off, 1, B, ada, k.edge.gate1, xe1)
        o.lnmod_fwd(xe1, 64, TL.pair_off, 1, B, ada, *k.edge.ln2, ye1, st_e2)
        f3, s3, f4, e_out = self.f(Pp, 128), self.f(Pp, 128), self.f(Pp, 64), self.f(Pp, 64)
        o.lin_fwd(mv(ye1), mv(p[bp + "ff_linear3.weight"]), p[bp + "ff_linear3.bias"], mv(f3), act=SILU, out2=mv(s3), drop=(*drop, *k.drop(2)))
        o.lin_fwd(mv(s3), mv(p[bp + "ff_linear4.weight"]), p[bp + "ff_linear4.bias"], mv(f4), drop=(*drop, *k.drop(3)))
        o.gate_add_fwd(ye1, f4, 64, TL.pair_off, 1, B, ada, k.edge.gate2, e_out)
        # the input of the equivariant update (dmt.py:37-60): e_out | distance features
        X2 = self.f(Pp, 128)
        X2[:, 0:64] = e_out
        X2[:, 64:128] = bt["X1"][:, 0:64]
        ed = self.f(Pp, 256)
        Win = p[bp + "equi_update.input_lin.weight"]                       # [256, 640] = [h_row | h_col | e | dist]
        o.lin_fwd(mv(X2), mv(Win, 512, 640), p[bp + "equi_update.input_lin.bias"], mv(ed))
        re_ = self.f(Pp, 16)                                     # per-block read-out features (dmt.py:388)
        o.lin_fwd(mv(e_out), mv(p[f"edge_{i}.weight"]), p[f"edge_{i}.bias"], mv(re_))
        bt.update(e_out=e_out, ed=ed, re_=re_, he=he, xe1=xe1, st_e2=st_e2, ye1=ye1, f3=f3, s3=s3, f4=f4, X2=X2)

    # directed rows (dmt.py:37-48): z of both directions, LayerNorm + modulate, coord_mlp.  Tape: c2 and zz, st_z, zn, c0, sc0.
    def _dir_fwd_fused(self, TL, ada, k, bt, save):
        D = 2 * TL.Pp
        bt["c2"] = self.f(max(D, 1), 3)
        if save:
            bt.update(zz=self.f(D, 256), st_z=self.f(D, 2), zn=self.f(D, 256), c0=self.f(D, 256), sc0=self.f(D, 256))
        self.ops.dir_chain_fwd(TL, bt["ac"], bt["ed"], ada, *k.equi_ln, self.wb["W0"][k.i], self.p[k.bp + "equi_update.coord_mlp.0.bias"],
                               self.wb["W2"][k.i], bt)

    def _dir_fwd_ops(self, TL, ada, k, bt, save):
        o, p, bp = self.ops, self.p, k.bp
        D = 2 * TL.Pp
        zz, zn, st_z = self.f(max(D, 1), 256), self.f(max(D, 1), 256), self.f(max(D, 1), 2)
        E._check(self.lib.dst_zbuild_fwd(C.byref(TL.c), ptr(bt["ac"]), ptr(bt["ed"]), ptr(zz), o._s()), "dst_zbuild_fwd")
        o.lnmod_fwd(zz, 256, TL.pair_off, 2, TL.B, ada, *k.equi_ln, zn, st_z)
        c0, sc0, c2 = self.f(max(D, 1), 256), self.f(max(D, 1), 256), self.f(max(D, 1), 3)
        o.lin_fwd(mv(zn, r1=D), mv(p[bp + "equi_update.coord_mlp.0.weight"]), p[bp + "equi_update.coord_mlp.0.bias"], mv(c0, r1=D), act=SILU,
                  out2=mv(sc0, r1=D))
        o.lin_fwd(mv(sc0, r1=D), mv(p[bp + "equi_update.coord_mlp.2.weight"]), None, mv(c2, r1=D))
        bt.update(c2=c2, zz=zz, st_z=st_z, zn=zn, c0=c0, sc0=sc0)

    # ------------------------------------------------------------------ backward
    def backward(self, dpos, datom, dedge) -> Dict[str, torch.Tensor]:
        """Gradients of every DMT parameter (and ``ctx_emb`` under the key ``'@ctx_emb'``) given the gradients of the three outputs."""
        t = self.t
        self.bind(*t["bound"])                              # the parameters and the stage of the forward that wrote this tape
        o, p, lib, gbuf = self.ops, self.p, self.lib, self.gbuf
        TL: TrainLayout = t["TL"]
        B, Nn, Pp = TL.B, TL.Nn, TL.Pp
        s = self.ops._s
        ada = t["ada"]
        g: Dict[str, torch.Tensor] = {}
        cat, dcat = self.cat, self.dcat

        def gw(name):                                       # gradient buffer of a parameter: a view of the trainer's flat stage (zeroed once
            g[name] = gbuf[name] if gbuf is not None else torch.zeros_like(p[name])   # per backward) or, stand-alone, a fresh zero tensor
            return g[name]

        d_ada = self.z(B, ADA)
        _, o.async_dw = o.stream_modes()
        # ---- read-out MLPs
        dAH, dEH = self.f(Nn, 768), self.f(Pp, 192)

        def mlp3_bwd(name, x, acts, dy: MV, dx, acc):
            a1, a1s, a2, a2s = acts
            o.lin_bwd_w(dy, mv(a2s), mv(gw(name + ".4.weight")), gw(name + ".4.bias"))
            d2 = torch.empty_like(a2)
            o.lin_bwd_x(dy, mv(p[name + ".4.weight"]), mv(d2), dact=SILU, ref=mv(a2))
            o.lin_bwd_w(mv(d2), mv(a1s), mv(gw(name + ".2.weight")), gw(name + ".2.bias"))
            d1 = torch.empty_like(a1)
            o.lin_bwd_x(mv(d2), mv(p[name + ".2.weight"]), mv(d1), dact=SILU, ref=mv(a1))
            o.lin_bwd_w(mv(d1), mv(x), mv(gw(name + ".0.weight")), gw(name + ".0.bias"))
            o.lin_bwd_x(mv(d1), mv(p[name + ".0.weight"]), mv(dx), acc=acc)

        mlp3_bwd("node_pred_mlp", t["AH"], (t["n1"], t["n1s"], t["n2"], t["n2s"]), mv(datom), dAH, False)
        mlp3_bwd("edge_exist_mlp", t["EH"], t["ro"]["edge_exist_mlp"], mv(dedge, 0, 1), dEH, False)
        mlp3_bwd("edge_type_mlp", t["EH"], t["ro"]["edge_type_mlp"], mv(dedge, 1, 2), dEH, True)
        # ---- blocks, last to first
        dh = self.z(Nn, 256)             # gradient of the block output h (later: block input of the next one)
        de = self.z(Pp, 64)
        dd2_buf = self.f(max(Pp, 1))
        for k in reversed(BLOCKS):
            dh, de, dpos = self._block_bwd(t, k, gw, d_ada, dAH, dEH, dd2_buf, dh, de, dpos)
        # ---- input embeddings
        o.lin_bwd_w(mv(dh), mv(t["X0n"]), mv(gw("node_emb.weight")), gw("node_emb.bias"))
        o.lin_bwd_w(mv(dAH, 0, 256), mv(t["X0n"]), mv(g["node_emb.weight"]), g["node_emb.bias"], acc=True)
        o.lin_bwd_w(mv(de), mv(t["X0p"]), mv(gw("edge_emb.weight")), gw("edge_emb.bias"))
        o.lin_bwd_w(mv(dEH, 0, 64), mv(t["X0p"]), mv(g["edge_emb.weight"]), g["edge_emb.bias"], acc=True)
        for nm in ("dist_layer.means.weight", "dist_layer.stds.weight"):
            gw(nm)
        if not t["first"]:
            dfeat0 = self.f(Pp, 64)
            o.lin_bwd_x(mv(de), mv(p["edge_emb.weight"], 4, 68), mv(dfeat0))
            o.lin_bwd_x(mv(dEH, 0, 64), mv(p["edge_emb.weight"], 4, 68), mv(dfeat0), acc=True)
            dms_top = self.f(B, 128)                         # (block 0's buffer may still be feeding its column sums on the side stream)
            o.geom_bwd(TL, t["cpos"], ada, d_ada, ADA_TOP, p["dist_layer.means.weight"], p["dist_layer.stds.weight"], t["xs0"], t["d2c"], dfeat0, None,
                       dms_top, dd2_buf, None)
            o.colsum(mv(dms_top, 1, 64), g["dist_layer.means.weight"].view(-1))
            o.colsum(mv(dms_top, 65, 128), g["dist_layer.stds.weight"].view(-1))
        # ---- adaLN table + time embedding
        o.lin_bwd_w(mv(d_ada), mv(t["st"]), mv(dcat["Wada"]), dcat["bada"])
        dtemb = self.f(B, 1024)
        o.lin_bwd_x(mv(d_ada), mv(cat["Wada"]), mv(dtemb), dact=SILU, ref=mv(t["temb"]))
        g["@ctx_emb"] = dtemb
        o.lin_bwd_w(mv(dtemb), mv(t["tg"]), mv(gw("time_mlp.3.weight")), gw("time_mlp.3.bias"))
        dtg = self.f(B, 1024)
        o.lin_bwd_x(mv(dtemb), mv(p["time_mlp.3.weight"]), mv(dtg), dact=GELU, ref=mv(t["tm1"]))
        o.lin_bwd_w(mv(dtg), mv(t["tf"]), mv(gw("time_mlp.1.weight")), gw("time_mlp.1.bias"))
        dtf = self.f(B, 17)
        o.lin_bwd_x(mv(dtg), mv(p["time_mlp.1.weight"]), mv(dtf))
        E._check(lib.dst_time_feat_bwd(ptr(t["noise_level"]), ptr(p["time_mlp.0.weights"]), ptr(dtf), B,
                                       ptr(gw("time_mlp.0.weights")), s()), "dst_time_feat_bwd")
        o.join_dw()                                          # the concatenated gradients are read right here, on the main stream
        o.async_dw = False
        self.scatter_cat_grads(g, gw)
        self.t = None
        return g

    # ---- one block, backward: (dh, de, dpos_out) of its outputs -> the gradients of its inputs; ``dAH`` / ``dEH`` hold the gradients of its
    #      read-out slices.  As in the forward, the streams are ordered here and the row chains follow in their two forms; the fused
    #      forward's tape feeds the fused backward kernels (the pair- and directed-row kernels take a CU's LDS alone, csrc/ds_train_chain.hip
    #      CHAIN_BWD_LDS: sharing a CU with a weight-gradient product they were not bit-reproducible).  Node rows run on the node stream.
    def _block_bwd(self, t, k: BlockSlots, gw, d_ada, dAH, dEH, dd2_buf, dh, de, dpos_out):
        o, p, lib, s = self.ops, self.p, self.lib, self.ops._s
        cat, dcat, bp, i = self.cat, self.dcat, k.bp, k.i
        TL, ada, ns, fused, drop, bt = t["TL"], t["ada"], t["node_stream"], t["fused_chain"], t["drop"], t["blocks"][k.i]
        B, Nn, Pp = TL.B, TL.Nn, TL.Pp
        D = 2 * Pp
        sec = o.node_section if ns else contextlib.nullcontext
        keep: list = []                                  # what only a node section touched: not freed before the closing wait of the block
        dir_rows, node_rear, pair_rear = ((self._dir_bwd_fused, self._node_rear_bwd_fused, self._pair_rear_bwd_fused) if fused else
                                          (self._dir_bwd_ops, self._node_rear_bwd_ops, self._pair_rear_bwd_ops))
        # read-out features of this block: their weight gradients here; their input gradients are part of the fused chains, the
        # per-operation chains find them added to dh / de
        drn, dre = mv(dAH, 256 + 64 * i, 256 + 64 * (i + 1)), mv(dEH, 64 + 16 * i, 64 + 16 * (i + 1))
        with sec():
            o.lin_bwd_w(drn, mv(bt["h_out"]), mv(gw(f"node_{i}.weight")), gw(f"node_{i}.bias"))
            if not fused:
                o.lin_bwd_x(drn, mv(p[f"node_{i}.weight"]), mv(dh), acc=True)
        o.lin_bwd_w(dre, mv(bt["e_out"]), mv(gw(f"edge_{i}.weight")), gw(f"edge_{i}.bias"))
        if not fused:
            o.lin_bwd_x(dre, mv(p[f"edge_{i}.weight"]), mv(de), acc=True)
        # equivariant update
        dpos_in, dc2 = self.f(Nn, 3), self.f(max(D, 1), 3)
        dsp, dms_buf = self.f(B), self.f(B, 128)          # per block: their column sums (parameter gradients) run on the side stream
        E._check(lib.dst_coord_bwd(C.byref(TL.c), ptr(bt["pos_in"]), ptr(bt["c2"]), ptr(t["adj"]), ptr(p[bp + "equi_update.coord_norm.scale"]),
                                   ptr(dpos_out), ptr(dpos_in), ptr(dc2), ptr(dsp), s()), "dst_coord_bwd")
        o.colsum(mv(dsp.view(B, 1)), gw(bp + "equi_update.coord_norm.scale"), param_grad=True)
        dWin = gw(bp + "equi_update.input_lin.weight")
        o.lin_bwd_w(mv(dc2, r1=D), mv(bt["sc0"], r1=D), mv(gw(bp + "equi_update.coord_mlp.2.weight")))
        dz = dir_rows(TL, ada, d_ada, k, bt, gw, dc2)
        dac, ded = self.f(Nn, 512), self.f(Pp, 256)
        E._check(lib.dst_zbuild_bwd(C.byref(TL.c), ptr(dz), ptr(dac), ptr(ded), s()), "dst_zbuild_bwd")
        # node stream (the section waits for dac)
        with sec():
            o.lin_bwd_w(mv(dac), mv(bt["h_out"]), mv(dcat["Wac"][i]))           # both node parts at once; scattered into dWin[:, 0:512] at the end
            dh_in, dattn = node_rear(TL, ada, d_ada, k, bt, gw, drop, dh, dAH.data_ptr() + 4 * (256 + 64 * i), dac, keep)
        # edge stream
        o.lin_bwd_w(mv(ded), mv(bt["X2"]), mv(dWin, 512, 640), gw(bp + "equi_update.input_lin.bias"))
        dfeat2, de_in, dhe = pair_rear(TL, ada, d_ada, k, bt, gw, drop, de, dEH.data_ptr() + 4 * (64 + 16 * i), ded)
        # node2edge
        du = self.f(Nn, 64)
        E._check(lib.dst_pair_sum_bwd(C.byref(TL.c), ptr(dhe), 64, ptr(du), 0, s()), "dst_pair_sum_bwd")
        o.colsum(mv(dhe), gw(bp + "node2edge_lin.bias"), param_grad=True)
        with sec():                                                              # (waits for du)
            o.lin_bwd_w(mv(du), mv(bt["attn"]), mv(gw(bp + "node2edge_lin.weight")))
            o.lin_bwd_x(mv(du), mv(p[bp + "node2edge_lin.weight"]), mv(dattn), acc=True)
        if ns:
            o.main_wait()                                                        # dattn
        # attention
        dqkv, dte = self.f(Nn, 768), self.f(Pp, 512)
        te = bt["te"]
        E._check(lib.dst_attn_bwd(C.byref(TL.c), ptr(bt["qkv"]), ptr(te[:, 0:256]), ptr(te[:, 256:512]), 512, ptr(bt["alpha"]),
                                  ptr(dattn), ptr(dqkv), ptr(dte[:, 0:256]), ptr(dte[:, 256:512]), 1, ptr(o.scratch),
                                  o.scratch.numel(), s()), "dst_attn_bwd")
        with sec():                                                              # (waits for dqkv) q | k | v and the adaLN modulate of the block input
            dhn = self.f(Nn, 256)
            o.lin_bwd_w(mv(dqkv), mv(bt["hn"]), mv(dcat["Wqkv"][i]), dcat["bqkv"][i])
            o.lin_bwd_x(mv(dqkv), mv(cat["Wqkv"][i]), mv(dhn))
            o.lnmod_bwd(dhn, bt["h_in"], bt["st_n1"], 256, TL.node_off, 1, B, ada, d_ada, *k.node.ln1, dh_in, True)
        self._pair_front_bwd(TL, ada, d_ada, k, bt, gw, dte, dfeat2, de_in, dms_buf, dd2_buf, dpos_in)
        if ns:
            o.main_wait()           # end of the block: everything the node stream was given precedes what the main stream does next, so this
                                    # block's temporaries (the locals here, ``keep``) may be released - and handed out again - on return
        return dh_in, de_in, dpos_in

    def _pair_front_bwd(self, TL, ada, d_ada, k, bt, gw, dte, dfeat2, de_in, dms_buf, dd2_buf, dpos_in):
        """Pair rows in front of the attention (one form: both forwards leave the same tape): lin_edge0 | lin_edge1, adaLN modulate, edge
        embedding (its e part adds to ``de_in``), distance features (``dfeat2``: the gradient of the copy the equivariant update read;
        adds to ``dpos_in``)."""
        o, p, bp, Pp = self.ops, self.p, k.bp, TL.Pp
        o.lin_bwd_w(mv(dte), mv(bt["en"]), mv(self.dcat["Wte"][k.i]))          # lin_edge0 | lin_edge1; dte is already in front of the tanh (te_is_tanh)
        den = self.f(Pp, 64)
        o.lin_bwd_x(mv(dte), mv(self.cat["Wte"][k.i]), mv(den))
        de1 = self.f(Pp, 64)
        o.lnmod_bwd(den, bt["e1"], bt["st_e1"], 64, TL.pair_off, 1, TL.B, ada, d_ada, *k.edge.ln1, de1, False)
        # edge embedding + distance features
        o.lin_bwd_w(mv(de1), mv(bt["X1"]), mv(gw(bp + "edge_emb.weight")), gw(bp + "edge_emb.bias"))
        dfeat1 = self.f(Pp, 64)
        Wee = p[bp + "edge_emb.weight"]
        o.lin_bwd_x(mv(de1), mv(Wee, 0, 64), mv(dfeat1))
        o.lin_bwd_x(mv(de1), mv(Wee, 64, 128), mv(de_in), acc=True)
        o.geom_bwd(TL, bt["pos_in"], ada, d_ada, k.dist, p[bp + "dist_layer.means.weight"], p[bp + "dist_layer.stds.weight"], bt["xs"], bt["d2"], dfeat1,
                   dfeat2, dms_buf, dd2_buf, dpos_in)
        o.colsum(mv(dms_buf, 1, 64), gw(bp + "dist_layer.means.weight").view(-1), param_grad=True)      # lane k of the kernel = feature k = Gaussian k - 1
        o.colsum(mv(dms_buf, 65, 128), gw(bp + "dist_layer.stds.weight").view(-1), param_grad=True)

    # directed rows: ``dc2`` -> dz, the gradient of z of both directions; coord_mlp.0's weight gradient
    def _dir_bwd_fused(self, TL, ada, d_ada, k, bt, gw, dc2):
        o, bp, D = self.ops, k.bp, 2 * TL.Pp
        dc0 = self.f(max(D, 1), 256)
        dz = self.f(max(D, 1), 256)                      # (not dc0: the coord_mlp.0 weight gradient may still be reading it on the side stream)
        # coord_mlp.2's and coord_mlp.0's input gradients and the LayerNorm backward as ONE kernel
        o.dir_chain_bwd(TL, dc2, bt["c0"], bt["zz"], bt["st_z"], ada, d_ada, *k.equi_ln, self.p[bp + "equi_update.coord_mlp.2.weight"],
                        self.wb["W0T"][k.i], dc0, dz)
        o.lin_bwd_w(mv(dc0, r1=D), mv(bt["zn"], r1=D), mv(gw(bp + "equi_update.coord_mlp.0.weight")), gw(bp + "equi_update.coord_mlp.0.bias"))
        return dz

    def _dir_bwd_ops(self, TL, ada, d_ada, k, bt, gw, dc2):
        o, p, bp, D = self.ops, self.p, k.bp, 2 * TL.Pp
        dc0 = self.f(max(D, 1), 256)
        dz = self.f(max(D, 1), 256)                      # (not dc0: the coord_mlp.0 weight gradient may still be reading it on the side stream)
        o.lin_bwd_x(mv(dc2, r1=D), mv(p[bp + "equi_update.coord_mlp.2.weight"]), mv(dc0, r1=D), dact=SILU, ref=mv(bt["c0"], r1=D))
        o.lin_bwd_w(mv(dc0, r1=D), mv(bt["zn"], r1=D), mv(gw(bp + "equi_update.coord_mlp.0.weight")), gw(bp + "equi_update.coord_mlp.0.bias"))
        dzn = self.f(max(D, 1), 256)
        o.lin_bwd_x(mv(dc0, r1=D), mv(p[bp + "equi_update.coord_mlp.0.weight"]), mv(dzn, r1=D))
        o.lnmod_bwd(dzn, bt["zz"], bt["st_z"], 256, TL.pair_off, 2, TL.B, ada, d_ada, *k.equi_ln, dz, False)
        return dz

    # node rows behind the attention: ``dh`` (block output), ``drn`` (data pointer of the read-out slice's gradient, row stride 768) and
    # ``dac`` (node parts of input_lin) -> (dh_in, dattn); the FF weight gradients.  Runs on the node stream: its temporaries go to ``keep``
    def _node_rear_bwd_fused(self, TL, ada, d_ada, k, bt, gw, drop, dh, drn, dac, keep):
        o, wb, bp, i, Nn = self.ops, self.wb, k.bp, k.i, TL.Nn
        # the five input gradients, both gated residuals and the LayerNorm backward of the node chain as ONE kernel
        df2, df1, dh_in, dattn = self.f(Nn, 256), self.f(Nn, 512), self.f(Nn, 256), self.f(Nn, 256)
        o.node_chain_bwd(TL, dh, drn, 768, dac, bt["f2"], bt["f1"], bt["x1"], bt["st_n2"], bt["attn"], ada, d_ada, k.node.gate1, *k.node.ln2, k.node.gate2,
                         wb["WacT"][i], wb["WnT"][i], wb["F2T"][i], wb["F1T"][i], (*drop, k.drop(0)[0], k.drop(1)[0]), df2, df1, dh_in, dattn)
        o.lin_bwd_w(mv(df2), mv(bt["s1"]), mv(gw(bp + "ff_linear2.weight")), gw(bp + "ff_linear2.bias"))
        o.lin_bwd_w(mv(df1), mv(bt["y1"]), mv(gw(bp + "ff_linear1.weight")), gw(bp + "ff_linear1.bias"))
        keep += (df2, df1)
        return dh_in, dattn

    def _node_rear_bwd_ops(self, TL, ada, d_ada, k, bt, gw, drop, dh, drn, dac, keep):
        o, p, bp, B, Nn = self.ops, self.p, k.bp, TL.B, TL.Nn                  # (drn: the block has added its input gradient to dh)
        o.lin_bwd_x(mv(dac), mv(self.cat["Wac"][k.i]), mv(dh), acc=True)
        dy1, df2 = self.f(Nn, 256), self.f(Nn, 256)
        o.gate_add_bwd(dh, bt["f2"], 256, TL.node_off, 1, B, ada, d_ada, k.node.gate2, dy1, False, df2, drop=(*drop, k.drop(1)[0]))
        o.lin_bwd_w(mv(df2), mv(bt["s1"]), mv(gw(bp + "ff_linear2.weight")), gw(bp + "ff_linear2.bias"))
        df1 = self.f(Nn, 512)
        o.lin_bwd_x(mv(df2), mv(p[bp + "ff_linear2.weight"]), mv(df1), dact=SILU, ref=mv(bt["f1"]), drop=(*drop, *k.drop(0)))
        o.lin_bwd_w(mv(df1), mv(bt["y1"]), mv(gw(bp + "ff_linear1.weight")), gw(bp + "ff_linear1.bias"))
        o.lin_bwd_x(mv(df1), mv(p[bp + "ff_linear1.weight"]), mv(dy1), acc=True)
        dx1 = self.f(Nn, 256)
        o.lnmod_bwd(dy1, bt["x1"], bt["st_n2"], 256, TL.node_off, 1, B, ada, d_ada, *k.node.ln2, dx1, False)
        dh_in, dattn = self.f(Nn, 256), self.f(Nn, 256)
        o.gate_add_bwd(dx1, bt["attn"], 256, TL.node_off, 1, B, ada, d_ada, k.node.gate1, dh_in, False, dattn)
        keep += (dy1, df2, df1, dx1)
        return dh_in, dattn

    # pair rows behind the attention: ``de`` (block output), ``dre`` (data pointer of the read-out slice's gradient, row stride 192) and
    # ``ded`` (edge part of input_lin) -> (dfeat2, de_in, dhe); the FF weight gradients
    def _pair_rear_bwd_fused(self, TL, ada, d_ada, k, bt, gw, drop, de, dre, ded):
        o, wb, bp, i, Pp = self.ops, self.wb, k.bp, k.i, TL.Pp
        # the five input gradients, both gated residuals and the LayerNorm backward of the rear chain as ONE kernel
        dfeat2, df4, df3, de_in, dhe = self.f(Pp, 64), self.f(Pp, 64), self.f(Pp, 128), self.f(Pp, 64), self.f(Pp, 64)
        o.pair_chain_bwd(TL, de, dre, 192, ded, bt["f4"], bt["f3"], bt["xe1"], bt["st_e2"], bt["he"], ada, d_ada, k.edge.gate1, *k.edge.ln2, k.edge.gate2,
                         wb["WedT"][i], wb["WroT"][i], wb["W4T"][i], wb["W3T"][i], (*drop, k.drop(2)[0], k.drop(3)[0]), dfeat2, df4, df3, de_in, dhe)
        o.lin_bwd_w(mv(df4), mv(bt["s3"]), mv(gw(bp + "ff_linear4.weight")), gw(bp + "ff_linear4.bias"))
        o.lin_bwd_w(mv(df3), mv(bt["ye1"]), mv(gw(bp + "ff_linear3.weight")), gw(bp + "ff_linear3.bias"))
        return dfeat2, de_in, dhe

    def _pair_rear_bwd_ops(self, TL, ada, d_ada, k, bt, gw, drop, de, dre, ded):
        o, p, bp, B, Pp = self.ops, self.p, k.bp, TL.B, TL.Pp                  # (dre: the block has added its input gradient to de)
        Win = p[bp + "equi_update.input_lin.weight"]
        o.lin_bwd_x(mv(ded), mv(Win, 512, 576), mv(de), acc=True)
        dfeat2 = self.f(Pp, 64)
        o.lin_bwd_x(mv(ded), mv(Win, 576, 640), mv(dfeat2))
        dye1, df4 = self.f(Pp, 64), self.f(Pp, 64)
        o.gate_add_bwd(de, bt["f4"], 64, TL.pair_off, 1, B, ada, d_ada, k.edge.gate2, dye1, False, df4, drop=(*drop, k.drop(3)[0]))
        o.lin_bwd_w(mv(df4), mv(bt["s3"]), mv(gw(bp + "ff_linear4.weight")), gw(bp + "ff_linear4.bias"))
        df3 = self.f(Pp, 128)
        o.lin_bwd_x(mv(df4), mv(p[bp + "ff_linear4.weight"]), mv(df3), dact=SILU, ref=mv(bt["f3"]), drop=(*drop, *k.drop(2)))
        o.lin_bwd_w(mv(df3), mv(bt["ye1"]), mv(gw(bp + "ff_linear3.weight")), gw(bp + "ff_linear3.bias"))
        o.lin_bwd_x(mv(df3), mv(p[bp + "ff_linear3.weight"]), mv(dye1), acc=True)
        dxe1 = self.f(Pp, 64)
        o.lnmod_bwd(dye1, bt["xe1"], bt["st_e2"], 64, TL.pair_off, 1, B, ada, d_ada, *k.edge.ln2, dxe1, False)
        de_in, dhe = self.f(Pp, 64), self.f(Pp, 64)
        o.gate_add_bwd(dxe1, bt["he"], 64, TL.pair_off, 1, B, ada, d_ada, k.edge.gate1, de_in, False, dhe)
        return dfeat2, de_in, dhe

    # ------------------------------------------------------------------ loss
    def loss(self, TL: TrainLayout, pos, atom_pred, edge_pred, tpos, tfeat, tedge, wm, weights=(1.0, 0.25, 0.1)):
        """losses.py:359-394 on packed predictions: (per-molecule loss [B], dpos, datom, dedge)."""
        loss_m, dpos, dfeat, dedge = self.f(TL.B), self.f(TL.Nn, 3), self.f(TL.Nn, 6), self.f(max(TL.Pp, 1), 2)
        E._check(self.lib.dst_loss(C.byref(TL.c), ptr(pos), ptr(atom_pred), ptr(edge_pred), ptr(tpos), ptr(tfeat), ptr(tedge),
                                   ptr(wm), weights[0], weights[1], weights[2], ptr(loss_m), ptr(dpos),
                                   ptr(dfeat), ptr(dedge), self.ops._s()), "dst_loss")
        return loss_m, dpos, dfeat, dedge
