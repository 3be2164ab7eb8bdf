"""ctypes binding to ``libdiffspectra_hip.so`` + the host plumbing around it.

Everything arithmetic happens in the HIP library (``csrc/ds_forward.hip``, ``ds_gemm.hip``, ``ds_sampler.hip``, ``ds_spec.hip``); this module packs the
reference-named parameters into the library's MFMA-operand layout once, builds the packed-ragged index
tables from ``node_mask``, owns the (torch-allocated) device workspace and issues the C-ABI calls on
torch's current HIP stream.  There is NO fallback: if the library is missing or no GPU is visible the
calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import abi
from .abi import ptr

_ptr = ptr      # the name under which the tests and tools that call the library directly know the pointer helper

LIB_PATH = os.environ.get("DIFFSPECTRA_HIP_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdiffspectra_hip.so"))

# constants, weight slots, entry points and argument structs as include/diffspectra_hip.h declares them (abi.py reads it)
_HDR = abi.SAMPLING
HEADER_PATH = _HDR.path
CONSTS = _HDR.consts
BLOCK_SLOTS, GLOBAL_SLOTS = _HDR.enums["ds_block_slot"], _HDR.enums["ds_global_slot"]      # the last enumerator of each is its count
EXPORTS = _HDR.exports("ds_")
NB = CONSTS["DS_NBLOCKS"]
W_BLOCK_SLOTS, W_GLOBAL_SLOTS, W_NUM_SLOTS = CONSTS["DS_W_BLOCK_SLOTS"], CONSTS["DS_W_GLOBAL_SLOTS"], CONSTS["DS_W_NUM_SLOTS"]
ADA_COLS = CONSTS["DS_ADA_COLS"]
ADA_STRIDE = CONSTS["DS_ADA_BLOCK_STRIDE"]
MAX_ATOMS = CONSTS["DS_MAX_ATOMS"]

DsWeights = _HDR.ctypes_struct("ds_weights")
DsLayout = _HDR.ctypes_struct("ds_layout")
DsWorkspace = _HDR.ctypes_struct("ds_workspace")
DsGemmArgs = _HDR.ctypes_struct("ds_gemm_args")
_WS_FIELDS = [f for f, _ in _HDR.structs["ds_workspace"]]

_lib = None


def load_library() -> C.CDLL:
    """Load the HIP library; fail loudly if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                           "diffspectra_amd has no CPU/PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    abi.SAMPLING.bind(lib)               # restype and argtypes of every export, as the headers declare them; AttributeError if the
    abi.TRAINING.bind(lib)               # headers declare something the .so lacks
    abi.SETS.bind(lib)
    abi.VALENCE.bind(lib)
    abi.GROUPS.bind(lib)
    abi.SCAFFOLD.bind(lib)
    abi.SMILES.bind(lib)
    abi.SUBSTRUCTURE.bind(lib)
    abi.STEREO.bind(lib)
    abi.BRICS.bind(lib)
    abi.MOBILE.bind(lib)
    abi.KEY.bind(lib)
    abi.FRAGGLE.bind(lib)
    abi.RMSD.bind(lib)
    abi.READER.bind(lib)
    abi.TILES.bind(lib)
    abi.STEP.bind(lib)
    abi.SOLVER.bind(lib)
    sizes = (C.c_int64 * 4)()
    lib.ds_struct_sizes(sizes)
    mine = [C.sizeof(t) for t in (DsWeights, DsLayout, DsWorkspace, DsGemmArgs)]
    if list(sizes) != mine:
        raise RuntimeError(f"C-ABI struct layout mismatch: library {list(sizes)} vs binding {mine}")
    _lib = lib
    return lib


def _check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed with status {status} "
                           f"({ {-1: 'bad argument', -2: 'HIP launch error'}.get(status, 'unknown')})")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


# ----------------------------------------------------------------------------------------- weight packing

def pack_linear(weight: torch.Tensor, n_pad_to: int = 32) -> torch.Tensor:
    """torch Linear weight [N_out, K_in] → MFMA-B packed [Kp/8][2][Np][4] with k = 8*kg + 4*half + s."""
    w = weight.detach().to(torch.float32).cpu()
    N, K = w.shape
    Kp, Np = (K + 7) // 8 * 8, (N + n_pad_to - 1) // n_pad_to * n_pad_to
    b = torch.zeros(Kp, Np)
    b[:K, :N] = w.t()
    return b.view(Kp // 8, 2, 4, Np).permute(0, 1, 3, 2).contiguous().reshape(-1)


SPLIT_SCALE = 2048.0   # 2^11: the low fp16 plane of a split operand is stored scaled so that it keeps 11 significant bits
TANH_PRESCALE = 2.8853900817779268     # 2 log2(e), ds_device.h ds_tanh2_prescaled
F16_MAX = 65504.0      # a split value has fp16's exponent range: |w| must stay below this (activations saturate in the kernels)


def _check_split_range(w: torch.Tensor, what: str) -> None:
    """A weight at or beyond fp16's largest finite value cannot be carried as two fp16 planes (its high plane would be inf and
    every product NaN).  No trained DMT comes near it (random-init |w| < 1); refuse loudly instead of computing garbage."""
    m = float(w.abs().max()) if w.numel() else 0.0
    if not (m < F16_MAX):
        raise ValueError(f"{what}: max |w| = {m:.4g} is outside the split-fp16 range (|w| < {F16_MAX:g}); "
                         "this weight cannot run on the f16 matrix pipe")



def pack_linear_f16_split(weight: torch.Tensor) -> torch.Tensor:
    """torch Linear weight [N_out, K_in] (K % 16 == 0, N % 32 == 0) → two fp16 planes with w ≈ w1 + w2 / 2048 (|error| ≤
    2^-23 |w|), in the A-operand order of v_mfma_f32_32x32x16_f16: halves [plane][K/16][k-half][N][8], k = 16 kb + 8 h + j;
    returned as the fp32 view of those bits (the packed weight buffer is fp32)."""
    w = weight.detach().to(torch.float32).cpu()
    _check_split_range(w, "pack_linear_f16_split")
    if w.shape[0] % 32:                                               # zero rows up to the MFMA tile width
        w = torch.cat([w, torch.zeros(32 - w.shape[0] % 32, w.shape[1])], 0)
    N, K = w.shape
    assert K % 16 == 0
    w1 = w.half()
    w2 = ((w - w1.float()) * SPLIT_SCALE).half()
    planes = torch.stack([w1, w2])                                   # [2, N, K]
    t = planes.view(2, N, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()   # [plane, kb, h, N, 8]
    return t.reshape(-1).view(torch.float32).clone()


def pack_ff4_chain(weight: torch.Tensor) -> torch.Tensor:
    """ff_linear4 [64, 128] for the accumulator-as-operand chain of k_edge_update: the SiLU'd 32 x 32 accumulator tile hc of
    ff_linear3 (lane = row, register i = hidden feature hc*32 + (i&3) + 8(i>>2) + 4h) is used, registers 8s .. 8s+7 at a time,
    as the B fragment of a 32x32x16 f16 MFMA; the A fragment of lane (r, h) must hold, in element j, the weight of output
    ft*32 + r for exactly that hidden feature.  Two fp16 planes (w = w1 + w2/2048); returned as the fp32 view of the bits."""
    w = weight.detach().to(torch.float32).cpu()
    _check_split_range(w, "pack_ff4_chain")
    n_out, k_in = w.shape                                                        # ff_linear4: (64, 128); edge readout .2: (32, 64)
    assert n_out % 32 == 0 and k_in % 32 == 0
    w1 = w.half()
    planes = torch.stack([w1, ((w - w1.float()) * SPLIT_SCALE).half()])          # [2, N, K]
    hc, s_, ft, h, r, j = torch.meshgrid(torch.arange(k_in // 32), torch.arange(2), torch.arange(n_out // 32), torch.arange(2),
                                          torch.arange(32), torch.arange(8), indexing="ij")
    k = hc * 32 + 16 * s_ + 8 * (j >> 2) + 4 * h + (j & 3)
    out = planes[:, ft * 32 + r, k]                                              # [2, K/32, 2, N/32, 2, 32, 8]
    return out.contiguous().reshape(-1).view(torch.float32).clone()


def split_rows_f16(a: torch.Tensor) -> torch.Tensor:
    """fp32 [M, K] → the A-operand layout of ``ds_gemm_split``: halves [M][2][K] (a = a1 + a2/2048), returned as float16."""
    a = a.detach().to(torch.float32)
    fin = torch.isfinite(a)
    sat = lambda t: torch.where(fin, t.clamp(-F16_MAX, F16_MAX), t)                    # the kernels' saturating conversion
    a1 = sat(a).half()
    a2 = sat(((a.double() - a1.double()) * SPLIT_SCALE).float()).half()               # fused on the device: no fp32 overflow in between
    return torch.stack([a1, a2], dim=1).contiguous()


def gemm_split(lib, a_split: torch.Tensor, w_split: torch.Tensor, bias, out: torch.Tensor, M: int, K: int, N: int):
    """C = A W + bias through ``ds_gemm_split`` (operands prepared by ``split_rows_f16`` / ``pack_linear_f16_split``)."""
    _check(lib.ds_gemm_split(ptr(a_split), ptr(w_split), ptr(bias), ptr(out), out.stride(0), M, K, N, _stream()), "ds_gemm_split")


def pad_vec(v: torch.Tensor, to: int = 32) -> torch.Tensor:
    v = v.detach().to(torch.float32).cpu().reshape(-1)
    out = torch.zeros((v.numel() + to - 1) // to * to)
    out[:v.numel()] = v
    return out


def _rbf_tables(sd, name):
    """CondGaussianLayer tables padded 63 → 64 (entry 63 is never read; kept at 1 so it is harmless)."""
    mean = sd[name + ".means.weight"].float().view(-1)
    std = sd[name + ".stds.weight"].float().view(-1).abs() + 1e-5          # layers.py:333
    a = (2 * 3.14159) ** 0.5                                               # layers.py:293-294 (truncated pi)
    astd = a * std                                                         # fp32 product, as torch evaluates it
    one = torch.ones(1)
    return torch.cat([mean, one]), torch.cat([std, one]), torch.cat([astd, one])


def pack_dmt_weights(sd: Dict[str, torch.Tensor]):
    """Reference-named DMT state dict (no ``module.`` prefix) → (flat fp32 tensor, slot offsets)."""
    sd = {k: v.detach().float().cpu() for k, v in sd.items() if not k.startswith("cond_encoder.")}
    chunks: List[torch.Tensor] = []
    offsets = [0] * W_NUM_SLOTS
    cursor = 0

    def put(slot_index, t):
        nonlocal cursor
        pad = (-cursor) % 64                     # 256-byte alignment of every slot
        if pad:
            chunks.append(torch.zeros(pad))
            cursor += pad
        offsets[slot_index] = cursor
        chunks.append(t.reshape(-1).float())
        cursor += t.numel()

    def bslot(b, name):
        return b * W_BLOCK_SLOTS + BLOCK_SLOTS.index(name)

    def gslot(name):
        return NB * W_BLOCK_SLOTS + GLOBAL_SLOTS.index(name)

    def cat_pad_rows(ws, pads):
        rows = []
        for w, p in zip(ws, pads):
            rows.append(w)
            if p > w.shape[0]:
                rows.append(torch.zeros(p - w.shape[0], w.shape[1]))
        return torch.cat(rows, 0)

    ada_rows, ada_bias = [], []
    for b in range(NB):
        p = f"e_block_{b}."
        put(bslot(b, "DS_BW_EDGE_EMB_W"), pack_linear(sd[p + "edge_emb.weight"]))
        put(bslot(b, "DS_BW_EDGE_EMB_B"), pad_vec(sd[p + "edge_emb.bias"]))
        put(bslot(b, "DS_BW_E0_W"), pack_linear(sd[p + "attn_mpnn.lin_edge0.weight"]))
        put(bslot(b, "DS_BW_E1_W"), pack_linear(sd[p + "attn_mpnn.lin_edge1.weight"]))
        wq, wk, wv = (sd[p + f"attn_mpnn.lin_{n}.weight"] for n in ("query", "key", "value"))
        bq, bk, bv = (sd[p + f"attn_mpnn.lin_{n}.bias"] for n in ("query", "key", "value"))
        put(bslot(b, "DS_BW_QKV_W"), pack_linear(cat_pad_rows([wq, wk, wv], [256, 256, 256])))
        put(bslot(b, "DS_BW_QKV_H"), pack_linear_f16_split(cat_pad_rows([wq, wk, wv], [256, 256, 256])))
        put(bslot(b, "DS_BW_QKV_B"), torch.cat([pad_vec(bq, 256), pad_vec(bk, 256), pad_vec(bv, 256)]))
        put(bslot(b, "DS_BW_N2E_W"), pack_linear(sd[p + "node2edge_lin.weight"]))
        put(bslot(b, "DS_BW_N2E_B"), pad_vec(sd[p + "node2edge_lin.bias"]))
        for i, nm in ((1, "FF1"), (2, "FF2"), (3, "FF3"), (4, "FF4")):
            put(bslot(b, f"DS_BW_{nm}_W"), pack_linear(sd[p + f"ff_linear{i}.weight"]))
            put(bslot(b, f"DS_BW_{nm}_B"), pad_vec(sd[p + f"ff_linear{i}.bias"]))
        put(bslot(b, "DS_BW_NODE_RO_W"), pack_linear(sd[f"node_{b}.weight"]))
        put(bslot(b, "DS_BW_NODE_RO_B"), pad_vec(sd[f"node_{b}.bias"]))
        put(bslot(b, "DS_BW_EDGE_RO_W"), pack_linear(sd[f"edge_{b}.weight"]))
        put(bslot(b, "DS_BW_EDGE_RO_B"), pad_vec(sd[f"edge_{b}.bias"]))
        win = sd[p + "equi_update.input_lin.weight"]                       # [256, 640] = [h_row | h_col | e | dist]
        put(bslot(b, "DS_BW_AC_W"), pack_linear(torch.cat([win[:, 0:256], win[:, 256:512]], 0)))
        put(bslot(b, "DS_BW_ED_W"), pack_linear(win[:, 512:640]))
        put(bslot(b, "DS_BW_ED_B"), pad_vec(sd[p + "equi_update.input_lin.bias"]))
        put(bslot(b, "DS_BW_CM0_W"), pack_linear(sd[p + "equi_update.coord_mlp.0.weight"]))
        put(bslot(b, "DS_BW_CM0_B"), pad_vec(sd[p + "equi_update.coord_mlp.0.bias"]))
        put(bslot(b, "DS_BW_CM2_W"), pack_linear(sd[p + "equi_update.coord_mlp.2.weight"]))
        put(bslot(b, "DS_BW_CM0_H"), pack_linear_f16_split(sd[p + "equi_update.coord_mlp.0.weight"]))
        put(bslot(b, "DS_BW_FF3_H"), pack_linear_f16_split(sd[p + "ff_linear3.weight"]))
        put(bslot(b, "DS_BW_FF4_C"), pack_ff4_chain(sd[p + "ff_linear4.weight"]))
        put(bslot(b, "DS_BW_N2E_H"), pack_linear_f16_split(sd[p + "node2edge_lin.weight"]))
        put(bslot(b, "DS_BW_FF1_H"), pack_linear_f16_split(sd[p + "ff_linear1.weight"]))
        put(bslot(b, "DS_BW_FF2_H"), pack_linear_f16_split(sd[p + "ff_linear2.weight"]))
        put(bslot(b, "DS_BW_NODE_RO_H"), pack_linear_f16_split(sd[f"node_{b}.weight"]))
        put(bslot(b, "DS_BW_AC_H"), pack_linear_f16_split(torch.cat([win[:, 0:256], win[:, 256:512]], 0)))
        # k_attn_fused evaluates tanh(x) as 1 - 2 / (1 + exp2(2 log2(e) x)): the factor rides in the packed weights
        put(bslot(b, "DS_BW_E0_H"), pack_linear_f16_split((sd[p + "attn_mpnn.lin_edge0.weight"].double() * TANH_PRESCALE).float()))
        put(bslot(b, "DS_BW_E1_H"), pack_linear_f16_split((sd[p + "attn_mpnn.lin_edge1.weight"].double() * TANH_PRESCALE).float()))
        put(bslot(b, "DS_BW_ED_H"), pack_linear_f16_split(win[:, 512:640]))
        put(bslot(b, "DS_BW_EDGE_EMB_H"), pack_linear_f16_split(sd[p + "edge_emb.weight"]))
        mean, std, astd = _rbf_tables(sd, p + "dist_layer")
        put(bslot(b, "DS_BW_RBF_MEAN"), mean)
        put(bslot(b, "DS_BW_RBF_STD"), std)
        put(bslot(b, "DS_BW_RBF_ASTD"), astd)
        put(bslot(b, "DS_BW_COORD_SCALE"), pad_vec(sd[p + "equi_update.coord_norm.scale"]))
        ws = [sd[p + "node_time_mlp.1.weight"], sd[p + "edge_time_mlp.1.weight"],
              sd[p + "equi_update.time_mlp.1.weight"], sd[p + "dist_layer.time_mlp.1.weight"]]
        bs = [sd[p + "node_time_mlp.1.bias"], sd[p + "edge_time_mlp.1.bias"],
              sd[p + "equi_update.time_mlp.1.bias"], sd[p + "dist_layer.time_mlp.1.bias"]]
        ada_rows.append(cat_pad_rows(ws, [1536, 384, 512, 32]))
        ada_bias.append(torch.cat([pad_vec(x, p_) for x, p_ in zip(bs, [1536, 384, 512, 32])]))
    ada_rows.append(cat_pad_rows([sd["dist_layer.time_mlp.1.weight"]], [32]))
    ada_bias.append(pad_vec(sd["dist_layer.time_mlp.1.bias"], 32))
    ada_w, ada_b = torch.cat(ada_rows, 0), torch.cat(ada_bias)
    assert ada_w.shape == (ADA_COLS, 1024) and ada_b.numel() == ADA_COLS and ada_rows[0].shape[0] == ADA_STRIDE
    put(gslot("DS_GW_SIN_W"), pad_vec(sd["time_mlp.0.weights"]))
    put(gslot("DS_GW_TM1_W"), pack_linear(sd["time_mlp.1.weight"]))
    put(gslot("DS_GW_TM1_B"), pad_vec(sd["time_mlp.1.bias"]))
    put(gslot("DS_GW_TM3_W"), pack_linear(sd["time_mlp.3.weight"]))
    put(gslot("DS_GW_TM3_B"), pad_vec(sd["time_mlp.3.bias"]))
    put(gslot("DS_GW_ADA_W"), pack_linear_f16_split(ada_w))
    put(gslot("DS_GW_ADA_B"), ada_b)
    put(gslot("DS_GW_NODE_EMB_W"), pack_linear(sd["node_emb.weight"]))
    put(gslot("DS_GW_NODE_EMB_B"), pad_vec(sd["node_emb.bias"]))
    put(gslot("DS_GW_EDGE_EMB_W"), pack_linear(sd["edge_emb.weight"]))
    put(gslot("DS_GW_EDGE_EMB_B"), pad_vec(sd["edge_emb.bias"]))
    mean, std, astd = _rbf_tables(sd, "dist_layer")
    put(gslot("DS_GW_RBF_MEAN"), mean)
    put(gslot("DS_GW_RBF_STD"), std)
    put(gslot("DS_GW_RBF_ASTD"), astd)
    for mlp, tag in (("node_pred_mlp", "NP"), ("edge_exist_mlp", "EX"), ("edge_type_mlp", "ET")):
        for i in (0, 2, 4):
            put(gslot(f"DS_GW_{tag}{i}_W"), pack_linear(sd[f"{mlp}.{i}.weight"]))
            put(gslot(f"DS_GW_{tag}{i}_B"), pad_vec(sd[f"{mlp}.{i}.bias"]))
    put(gslot("DS_GW_NP0_H"), pack_linear_f16_split(sd["node_pred_mlp.0.weight"]))
    put(gslot("DS_GW_NP2_H"), pack_linear_f16_split(sd["node_pred_mlp.2.weight"]))
    put(gslot("DS_GW_EX0_H"), pack_linear_f16_split(sd["edge_exist_mlp.0.weight"]))
    put(gslot("DS_GW_ET0_H"), pack_linear_f16_split(sd["edge_type_mlp.0.weight"]))
    put(gslot("DS_GW_EX2_C"), pack_ff4_chain(sd["edge_exist_mlp.2.weight"]))
    put(gslot("DS_GW_ET2_C"), pack_ff4_chain(sd["edge_type_mlp.2.weight"]))
    return torch.cat(chunks), offsets


# ----------------------------------------------------------------------------------------- layout

class Layout:
    """Packed-ragged index tables for one (node_mask) batch structure."""

    def __init__(self, node_mask: torch.Tensor, device):
        nm = node_mask.detach().reshape(node_mask.shape[0], node_mask.shape[1]).to("cpu")
        valid = (nm != 0).numpy()
        B, N = valid.shape
        n_atoms = valid.sum(1).astype(np.int64)
        if n_atoms.max(initial=0) > MAX_ATOMS:
            raise ValueError(f"molecule with {int(n_atoms.max())} atoms exceeds DS_MAX_ATOMS={MAX_ATOMS}")
        node_off = np.zeros(B + 1, np.int64)
        node_off[1:] = np.cumsum(n_atoms)
        pair_cnt = n_atoms * (n_atoms - 1) // 2
        pair_off = np.zeros(B + 1, np.int64)
        pair_off[1:] = np.cumsum(pair_cnt)
        bb, ii = np.nonzero(valid)                                   # row-major → molecule-major, index-ascending
        node_dense = (bb * N + ii).astype(np.int32)
        node_mol = bb.astype(np.int32)
        pa, pb, pm = [], [], []
        tri_cache = {}
        for m in range(B):
            n = int(n_atoms[m])
            if n < 2:
                continue
            if n not in tri_cache:
                tri_cache[n] = np.triu_indices(n, 1)                 # (a asc, b asc): p = a(2n-a-1)/2 + (b-a-1)
            a, b = tri_cache[n]
            pa.append(a + node_off[m]); pb.append(b + node_off[m]); pm.append(np.full(a.shape, m))
        cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
        self.B, self.N, self.Nn, self.Pp = B, N, int(node_off[-1]), int(pair_off[-1])
        self.max_n = int(n_atoms.max(initial=0))
        self.n_atoms = n_atoms
        self.valid = valid
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.t = dict(node_off=dev(node_off.astype(np.int32)), pair_off=dev(pair_off.astype(np.int32)),
                      node_dense=dev(node_dense), node_mol=dev(node_mol), pair_a=dev(cat(pa)), pair_b=dev(cat(pb)),
                      pair_mol=dev(cat(pm)),
                      mol_by_size=dev(np.stack([node_off[:-1], n_atoms, pair_off[:-1], pair_cnt], 1)[
                          np.argsort(-n_atoms.astype(np.int64), kind="stable")].astype(np.int32)))
        self.c = DsLayout(B=B, N=N, Nn=self.Nn, Pp=self.Pp, max_n=self.max_n, _pad=0,
                          **{k: v.data_ptr() for k, v in self.t.items()})

    def check_edge_mask(self, edge_mask: torch.Tensor):
        """The path assumes edge_mask = outer(node_mask) minus the diagonal, as every reference caller builds it."""
        ok = getattr(self, "_mask_ok", None)
        # the SAME tensor object, unmodified since it was checked (a B*N*N device->host copy saved).  The cache holds the tensor
        # itself: an address is not an identity - the caching allocator hands a freed mask's address to the next same-shape mask
        if ok is not None and ok[0] is edge_mask and ok[1] == edge_mask._version:
            return
        v = torch.from_numpy(self.valid)
        want = (v.unsqueeze(1) & v.unsqueeze(2)) & ~torch.eye(self.N, dtype=torch.bool).unsqueeze(0)
        got = edge_mask.detach().reshape(self.B, self.N, self.N).cpu() != 0
        if not torch.equal(want, got):
            raise ValueError("edge_mask is not node_mask ⊗ node_mask minus the diagonal; unsupported graph structure")
        self._mask_ok = (edge_mask, edge_mask._version)

    def check_edge_symmetry(self, edge: torch.Tensor, name: str = "edge_x"):
        """The pair layout stores one value per unordered pair: ``edge[b,i,j,:] == edge[b,j,i,:]`` must hold on valid pairs."""
        ok = getattr(self, "_sym_ok", {}).get(name)
        if ok is not None and ok[0] is edge and ok[1] == edge._version:   # the same tensor object, unmodified (a blocking .any() saved)
            return
        e = edge.detach().reshape(self.B, self.N, self.N, -1)
        v = torch.from_numpy(self.valid).to(e.device)
        m = (v.unsqueeze(1) & v.unsqueeze(2)).unsqueeze(-1)
        if bool(((e != e.transpose(1, 2)) & m).any()):
            raise ValueError(f"{name} is not symmetric in its two atom indices; the MI355X path stores edge features per "
                             "unordered pair and does not support directed edge inputs")
        if not hasattr(self, "_sym_ok"):
            self._sym_ok = {}
        self._sym_ok[name] = (edge, edge._version)


class Workspace:
    def __init__(self, L: Layout, device):
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
        Nn, Pp, B = max(L.Nn, 1), max(L.Pp, 1), L.B
        self.t = dict(pos=f(Nn, 4), h=f(Nn, 256), e=f(Pp, 64), atom_hids=f(Nn, 768), edge_hids=f(Pp, 192),
                      tfeat=f(B, 24), tmid=f(B, 1024), temb_silu=f(B, 1024), ada=f(B, ADA_COLS), qkv=f(Nn, 768),
                      ye=f(Pp, 64), dist=f(Pp), attn=f(Nn, 256), u=f(Nn, 64), ac=f(Nn, 512),
                      ed=f(Pp, 256), lg=f(Pp, 32), tr=f(Pp, 8),
                      adj=torch.zeros(Pp, dtype=torch.int32, device=device),
                      flags=torch.zeros(64, dtype=torch.int32, device=device))
        # a buffer is added in the header AND here: one without the other fails now instead of leaving a NULL pointer in the struct
        assert list(self.t) == _WS_FIELDS, (list(self.t), _WS_FIELDS)
        self.c = DsWorkspace(**{k: v.data_ptr() for k, v in self.t.items()})


# ----------------------------------------------------------------------------------------- structure metric

RECORD_BYTES = CONSTS["DS_RECORD_BYTES"]


def _want(t, name, dtype, shape):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        raise ValueError(f"{name} must have shape {list(shape)} (None = any), got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _record_call(name, tables, ref_index, scalars, outputs, prefix="ds_", also=()):
    """The binding of an entry point on result records.  ``tables``: ``[(rec, n)]`` (``ds_graph_hash_records``, ``ds_morgan_records``; ``ref_index`` unused) or
    ``[(prb_rec, prb_n), (ref_rec, ref_n)]`` with ``ref_index`` (the record pairs of the header).  Checks the tensors (never converts them),
    the pairing rule and the one-device rule, allocates ``outputs`` - ``[(dtype, trailing shape)]``, one row per pair - and issues ``ds_<name>``
    with the C ``scalars`` between the tables and the outputs, on the current stream of the tensors' device.  Returns the output tensors.
    ``prefix`` names the header's family when it is not ``ds_``; ``also`` are further input tensors, already checked by the caller and passed
    among the ``scalars`` as addresses, that the one-device rule covers."""
    pairs = len(tables) == 2
    tensors, args = [], []
    for (rec, n), (rec_name, n_name) in zip(tables, (("prb_rec", "prb_n"), ("ref_rec", "ref_n")) if pairs else (("rec", "n"),)):
        _want(rec, rec_name, torch.uint8, (None, RECORD_BYTES))
        _want(n, n_name, torch.int32, (rec.shape[0],))
        tensors += [rec, n]
        args += [ptr(rec), ptr(n), rec.shape[0]]
    P = tensors[0].shape[0]
    if pairs:
        if ref_index is not None:
            _want(ref_index, "ref_index", torch.int64, (P,))
            tensors.append(ref_index)
        elif tensors[2].shape[0] < P:
            raise ValueError(f"without ref_index pair p reads ground-truth row p: {tensors[2].shape[0]} rows for {P} pairs")
        args.append(ptr(ref_index))
    tensors += list(also)
    dev = tensors[0].device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError(f"{name} needs all its tensors on one HIP device (torch device type 'cuda'); there is no CPU path")
    lib = load_library()
    out = tuple(torch.empty(P, *shape, dtype=dtype, device=dev) for dtype, shape in outputs)
    with torch.cuda.device(dev):
        st = getattr(lib, prefix + name)(*args, *scalars, *(ptr(t) for t in out), _stream())
    _check(st, prefix + name)
    return out


def _node_budget(max_nodes, most):
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, int):
        raise TypeError(f"max_nodes must be an int, got {type(max_nodes).__name__}")
    if not 0 <= max_nodes <= most:
        raise ValueError(f"max_nodes must lie in [0, {most}], got {max_nodes}")
    return max_nodes


_MAP = (torch.int32, (MAX_ATOMS,))        # the atom map that every record-pair entry point returns last


def match_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                  ref_index: Optional[torch.Tensor] = None, max_distance: float = 5.0, min_atoms: int = 3):
    """``ds_match_records``: Hungarian-matched RMSD, type / bond accuracy and the exact-graph flag of P (generated, ground-truth) pairs.

    ``prb_rec [P, 1248] u8`` / ``ref_rec [M, 1248] u8``: records in the layout of ``shard.pack_records_u8``; ``prb_n [P] i32`` / ``ref_n [M] i32``:
    atom counts; ``ref_index [P] i64``: ground-truth row of every pair (``None``: pair p uses row p).  Returns the six device tensors
    ``(rmsd [P] f64, n_matched [P] i32, type_acc [P] f32, bond_acc [P] f32, exact [P] u8, map [P, 29] i32)``, enqueued on the current stream
    without synchronising.  The arguments are checked, never converted: a wrong dtype, shape or a non-contiguous tensor raises."""
    max_distance, min_atoms = float(max_distance), int(min_atoms)
    if max_distance != max_distance:
        raise ValueError("max_distance must not be NaN")
    return _record_call("match_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, [max_distance, min_atoms],
                        [(torch.float64, ()), (torch.int32, ()), (torch.float32, ()), (torch.float32, ()), (torch.uint8, ()), _MAP])


# ----------------------------------------------------------------------------------------- graph identity

GRAPH_MAX_NODES = CONSTS["DS_GRAPH_MAX_NODES"]
GRAPH_DIFFERENT, GRAPH_IDENTICAL, GRAPH_UNDECIDED, GRAPH_INVALID = (CONSTS["DS_GRAPH_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID"))


def graph_identity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                           ref_index: Optional[torch.Tensor] = None, max_nodes: int = 4096):
    """``ds_graph_identity_records``: is the generated molecule of each of P pairs the SAME labelled graph (atom type, formal charge, bond
    order) as its ground truth, whatever the conformation - constitution-level identity, not InChIKey identity (no stereo layer, no
    tautomer / charge normalisation: ``normal_records`` rewrites the records for that; see the header).

    The tensors are those of ``match_records``.  Returns the device tensors ``(verdict [P] u8, nodes [P] i32, map [P, 29] i32)``, enqueued on
    the current stream without synchronising: verdict ``GRAPH_IDENTICAL`` (1: ``map`` is a checked isomorphism), ``GRAPH_DIFFERENT`` (0: proven),
    ``GRAPH_UNDECIDED`` (2: the search needed more than ``max_nodes`` tries; 0 = colour refinement alone) or ``GRAPH_INVALID`` (3: ``ref_index``
    outside the table).  The arguments are checked, never converted."""
    return _record_call("graph_identity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, [_node_budget(max_nodes, GRAPH_MAX_NODES)],
                        [(torch.uint8, ()), (torch.int32, ()), _MAP])


def graph_hash_records(rec: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """``ds_graph_hash_records``: the permutation-invariant 64-bit hash of the labelled graph of every record (formula in the header).
    ``rec [P, 1248] u8``, ``n [P] i32`` -> ``[P] i64`` holding the hash's 64 bits (torch sorts and buckets int64; read them as unsigned with
    ``& (2**64 - 1)``), on the current stream.  Equal hashes do not prove identity - ``graph_identity_records`` decides."""
    return _record_call("graph_hash_records", [(rec, n)], None, [], [(torch.int64, ())])[0]


# ----------------------------------------------------------------------------------------- MCES distance

MCES_MAX_NODES = CONSTS["DS_MCES_MAX_NODES"]
MCES_EXACT, MCES_UNDECIDED, MCES_INVALID = (CONSTS["DS_MCES_" + k] for k in ("EXACT", "UNDECIDED", "INVALID"))


def mces_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                 ref_index: Optional[torch.Tensor] = None, drop_h: bool = True, max_nodes: int = 1 << 18):
    """``ds_mces_records``: the exact maximum-common-edge-subgraph distance of each of P (generated, ground-truth) pairs as labelled graphs
    (atom type and bond order; the formal charge is not compared; ``drop_h`` leaves the hydrogens out) - ``W_A + W_B - 2 max score``, an
    integer, by branch-and-bound (definition and soundness in the header).  It stands in for the reference's "MCES (Average)" with two
    stated deviations: the records hold Kekule orders 1..3 and not RDKit's aromatic 1.5 (two Kekule drawings of o-xylene are 2 apart), and
    parity with the ``myopic_mces`` package itself is unpinned (it cannot be run here).

    The tensors are those of ``match_records``.  Returns the device tensors ``(dist [P] i32, lower [P] i32, status [P] u8, nodes [P] i32,
    map [P, 29] i32)``, enqueued on the current stream without synchronising: status ``MCES_EXACT`` (0: ``dist`` is the distance),
    ``MCES_UNDECIDED`` (2: the search needed more than ``max_nodes`` tries; ``lower <= distance <= dist``, and ``map`` still achieves ``dist``)
    or ``MCES_INVALID`` (3: ``ref_index`` outside the table, ``dist = lower = -1``).  The arguments are checked, never converted."""
    if not isinstance(drop_h, bool):
        raise TypeError(f"drop_h must be a bool, got {type(drop_h).__name__}")
    return _record_call("mces_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, [int(drop_h), _node_budget(max_nodes, MCES_MAX_NODES)],
                        [(torch.int32, ()), (torch.int32, ()), (torch.uint8, ()), (torch.int32, ()), _MAP])


# ----------------------------------------------------------------------------------------- Morgan fingerprints

MORGAN_MAX_RADIUS, MORGAN_MAX_FEATURES, MORGAN_MAX_BITS = (CONSTS["DS_MORGAN_MAX_" + k] for k in ("RADIUS", "FEATURES", "BITS"))
MORGAN_OK, MORGAN_INVALID = CONSTS["DS_MORGAN_OK"], CONSTS["DS_MORGAN_INVALID"]


def _morgan_shape(drop_h, radius):
    if not isinstance(drop_h, bool):
        raise TypeError(f"drop_h must be a bool, got {type(drop_h).__name__}")
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise TypeError(f"radius must be an int, got {type(radius).__name__}")
    if not 0 <= radius <= MORGAN_MAX_RADIUS:
        raise ValueError(f"radius must lie in [0, {MORGAN_MAX_RADIUS}], got {radius}")
    return [int(drop_h), radius]


def morgan_records(rec: torch.Tensor, n: torch.Tensor, drop_h: bool = True, radius: int = 2):
    """``ds_morgan_records``: the Morgan (ECFP-like) fingerprint of the labelled graph of every record as its set of 64-bit features -
    atom invariant (type, charge, kept degree, hydrogen count, cycle flag), ``radius`` rounds over the kept neighbours, one feature per
    distinct new bond environment (definition in the header; invariant under renaming atoms).  ``drop_h`` leaves the hydrogens out and
    counts them in the invariant, as the reference's SMILES route does.  It is not RDKit's fingerprint bit for bit: Kekule orders 1..3
    instead of aromatic bonds, and RDKit's own invariant hash is not reproduced.

    ``rec [P, 1248] u8``, ``n [P] i32`` -> ``(ids [P, 116] i64, count [P] i32)`` on the current stream: ``ids[p, :count[p]]`` are the distinct
    features in ascending UNSIGNED order as int64 bit patterns (read them as unsigned with ``& (2**64 - 1)``), the remaining slots are 0.
    The arguments are checked, never converted."""
    return _record_call("morgan_records", [(rec, n)], None, _morgan_shape(drop_h, radius), [(torch.int64, (MORGAN_MAX_FEATURES,)), (torch.int32, ())])


def morgan_similarity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                              ref_index: Optional[torch.Tensor] = None, drop_h: bool = True, radius: int = 2, n_bits: int = 2048):
    """``ds_morgan_similarity_records``: the sizes behind the Tanimoto and the cosine similarity of the Morgan fingerprints
    (``morgan_records``) of each of P (generated, ground-truth) pairs, folded to ``n_bits`` (0: unfolded; else a power of two in
    [64, 4096]) - the reference's ``GetMorganFingerprintAsBitVect(mol, 2, nBits=2048)`` with ``TanimotoSimilarity`` / ``CosineSimilarity``
    (``compute_metrics.py:246-253``), with the stated deviations: Kekule orders 1..3 instead of aromatic bonds (the two Kekule drawings of
    o-xylene share 5 of 10 + 10 features), RDKit's own hash and fold are not reproduced, and ``drop_h`` is the reference's SMILES route.

    The tensors are those of ``match_records``.  Returns the device tensors ``(common [P] i32, n_prb [P] i32, n_ref [P] i32, status [P] u8)``,
    enqueued on the current stream without synchronising: the sizes of the intersection and of the two sets, status ``MORGAN_OK`` (0) or
    ``MORGAN_INVALID`` (3: ``ref_index`` outside the table, the three counts are -1).  The arguments are checked, never converted."""
    scalars = _morgan_shape(drop_h, radius)
    if isinstance(n_bits, bool) or not isinstance(n_bits, int):
        raise TypeError(f"n_bits must be an int, got {type(n_bits).__name__}")
    if n_bits != 0 and not (64 <= n_bits <= MORGAN_MAX_BITS and n_bits & (n_bits - 1) == 0):
        raise ValueError(f"n_bits must be 0 (unfolded) or a power of two in [64, {MORGAN_MAX_BITS}], got {n_bits}")
    return _record_call("morgan_similarity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, scalars + [n_bits],
                        [(torch.int32, ()), (torch.int32, ()), (torch.int32, ()), (torch.uint8, ())])


# ----------------------------------------------------------------------------------------- substructure geometry and its MMD

GEOM_MAX_CLASSES = CONSTS["DS_GEOM_MAX_CLASSES"]
MMD_TILE, MMD_MAX_SAMPLES, MMD_MAX_KERNELS, MMD_MAX_CLASSES = (CONSTS["DS_MMD_" + k] for k in ("TILE", "MAX_SAMPLES", "MAX_KERNELS", "MAX_CLASSES"))
MMD_OK, MMD_EMPTY, MMD_INVALID = (CONSTS["DS_MMD_" + k] for k in ("OK", "EMPTY", "INVALID"))


def _class_tables(rec, bond_cls, angle_cls, dihedral_cls):
    """The three class tables as C arguments (pointer, count each): int32 device vectors of at most 32 codes on the records' device."""
    args = []
    for t, name in ((bond_cls, "bond_cls"), (angle_cls, "angle_cls"), (dihedral_cls, "dihedral_cls")):
        _want(t, name, torch.int32, (None,))
        if t.shape[0] > GEOM_MAX_CLASSES:
            raise ValueError(f"{name} holds {t.shape[0]} classes, at most {GEOM_MAX_CLASSES} fit")
        if torch.is_tensor(rec) and t.device != rec.device:
            raise RuntimeError(f"{name} must be on the records' device {rec.device}, got {t.device}")
        args += [ptr(t) if t.shape[0] else None, t.shape[0]]
    return args


def geometry_count_records(rec: torch.Tensor, n: torch.Tensor, bond_cls: torch.Tensor, angle_cls: torch.Tensor, dihedral_cls: torch.Tensor):
    """``ds_geometry_count_records``: how many bond lengths, bond angles and dihedral angles of each record fall into the listed classes.

    ``rec [P, 1248] u8``, ``n [P] i32``; the class tables are int32 device vectors of at most 32 codes each, the fields of a class in 4-bit
    groups (first field in bits 0..3; ``structure_metrics.geometry_classes`` builds them from the reference's symbols).  Returns ``(counts
    [P, 3] i32, skipped [P] i32)`` on the current stream without synchronising: entries emitted per kind, and entries of a listed class whose
    value is undefined (coincident atoms, a collinear dihedral).  Every angle counts once - the reference counts it 0, 1 or 2 times depending
    on the atom numbering - and parity with RDKit's angle functions is unpinned (see the header).  Checked, never converted."""
    return _record_call("geometry_count_records", [(rec, n)], None, _class_tables(rec, bond_cls, angle_cls, dihedral_cls),
                        [(torch.int32, (3,)), (torch.int32, ())])


def geometry_fill_records(rec: torch.Tensor, n: torch.Tensor, bond_cls: torch.Tensor, angle_cls: torch.Tensor, dihedral_cls: torch.Tensor,
                          offsets: torch.Tensor, totals):
    """``ds_geometry_fill_records``: the values and classes that ``geometry_count_records`` counted.  ``offsets [P, 3] i64``: where each record's
    entries of each kind start (the exclusive prefix sum of ``counts`` over the records); ``totals``: three ints, the length of each kind's
    output.  Returns ``((bond_value [T0] f32, bond_class [T0] u8), (angle_value, angle_class), (dihedral_value, dihedral_class))`` on the current
    stream without synchronising: lengths in the units of the record's positions, angles in degrees in [0, 180], dihedrals in degrees in
    (-180, 180]; within a record in the header's fixed order, so bit-identical from run to run.  An index at or beyond a total is never
    written.  The deviations from the reference are those of ``geometry_count_records``.  Checked, never converted."""
    tables = _class_tables(rec, bond_cls, angle_cls, dihedral_cls)
    totals = [int(t) for t in totals]
    if len(totals) != 3 or min(totals) < 0:
        raise ValueError(f"totals must be three non-negative ints, got {totals}")
    _want(rec, "rec", torch.uint8, (None, RECORD_BYTES))
    _want(offsets, "offsets", torch.int64, (rec.shape[0], 3))
    if offsets.device != rec.device:
        raise RuntimeError(f"offsets must be on the records' device {rec.device}, got {offsets.device}")
    out = tuple((torch.empty(t, dtype=torch.float32, device=rec.device), torch.empty(t, dtype=torch.uint8, device=rec.device)) for t in totals)
    _record_call("geometry_fill_records", [(rec, n)], None,
                 tables + totals + [ptr(offsets)] + [ptr(t) if t.numel() else None for pair in out for t in pair], [])
    return out


def mmd_workspace_bytes(n_classes: int) -> int:
    """``ds_mmd_1d_workspace_bytes``: the device bytes ``mmd_1d_segments`` needs for ``n_classes`` classes (a pure host function)."""
    size = C.c_int64(0)
    _check(load_library().ds_mmd_1d_workspace_bytes(int(n_classes), C.byref(size)), "ds_mmd_1d_workspace_bytes")
    return int(size.value)


def mmd_1d_segments(x: torch.Tensor, x_off: torch.Tensor, y: torch.Tensor, y_off: torch.Tensor, kernel_mul: float = 2.0, kernel_num: int = 5,
                    fix_sigma: Optional[float] = None, workspace: Optional[torch.Tensor] = None):
    """``ds_mmd_1d_segments``: the reference's ``compute_mmd`` (``evaluation/mmd.py:6-63``; a sum of ``kernel_num`` Gaussian kernels whose
    bandwidths are ``kernel_mul`` apart around the mean squared distance of the pooled samples, or around ``fix_sigma``) of C classes of 1-D
    samples in one launch sequence.  ``x [Nx] f32`` / ``y [Ny] f32``: source / target samples, class c in ``x[x_off[c]:x_off[c+1]]`` and
    ``y[y_off[c]:y_off[c+1]]`` (``x_off``, ``y_off`` ``[C+1] i64`` on the device).  ``workspace``: a ``uint8`` device tensor of at least
    ``mmd_workspace_bytes(C)`` bytes, allocated here when ``None``.

    Returns ``(out [C, 5] f64 = (mmd, XX, YY, XY, bandwidth), status [C] u8)`` on the current stream without synchronising: status ``MMD_OK``,
    ``MMD_EMPTY`` (no source or no target sample: NaN) or ``MMD_INVALID`` (unusable offsets, or more than 2^20 samples on a side: NaN).  All
    samples identical gives NaN, as the reference does.  Bit-identical from run to run.  Checked, never converted; no CPU path."""
    _want(x, "x", torch.float32, (None,))
    _want(y, "y", torch.float32, (None,))
    _want(x_off, "x_off", torch.int64, (None,))
    _want(y_off, "y_off", torch.int64, (x_off.shape[0],))
    if x_off.shape[0] < 1:
        raise ValueError("x_off and y_off hold C + 1 offsets: at least one")
    n_cls = x_off.shape[0] - 1
    if n_cls > MMD_MAX_CLASSES:
        raise ValueError(f"at most {MMD_MAX_CLASSES} classes per call, got {n_cls}")
    if isinstance(kernel_num, bool) or not isinstance(kernel_num, int):
        raise TypeError(f"kernel_num must be an int, got {type(kernel_num).__name__}")
    if not 1 <= kernel_num <= MMD_MAX_KERNELS:
        raise ValueError(f"kernel_num must lie in [1, {MMD_MAX_KERNELS}], got {kernel_num}")
    kernel_mul, sigma = float(kernel_mul), float(fix_sigma) if fix_sigma else 0.0          # the reference's `if fix_sigma:`
    if not (0.0 < kernel_mul < float("inf")):
        raise ValueError(f"kernel_mul must be finite and > 0, got {kernel_mul}")
    if not (0.0 <= sigma < float("inf")):
        raise ValueError(f"fix_sigma must be finite and >= 0, got {fix_sigma}")
    tensors = [x, x_off, y, y_off]
    need = mmd_workspace_bytes(n_cls)
    dev = x.device
    if workspace is not None:
        _want(workspace, "workspace", torch.uint8, (None,))
        if workspace.shape[0] < need:
            raise ValueError(f"workspace holds {workspace.shape[0]} bytes, {need} are needed for {n_cls} classes")
        tensors.append(workspace)
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError("mmd_1d_segments needs all its tensors on one HIP device (torch device type 'cuda'); there is no CPU path")
    lib = load_library()
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    out = torch.empty(n_cls, 5, dtype=torch.float64, device=dev)
    status = torch.empty(n_cls, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = lib.ds_mmd_1d_segments(ptr(x) if x.numel() else None, ptr(x_off), x.shape[0], ptr(y) if y.numel() else None, ptr(y_off),
                                    y.shape[0], n_cls, kernel_mul, kernel_num, sigma, ptr(workspace), workspace.shape[0], ptr(out),
                                    ptr(status), _stream())
    _check(st, "ds_mmd_1d_segments")
    return out, status


# ----------------------------------------------------------------------------------------- bit rows: nearest neighbour and mean similarity of sets

SETS_CONSTS = abi.SETS.consts             # include/diffspectra_sets.h
SETS_TILE_A, SETS_TILE_B, SETS_CHUNKS = (SETS_CONSTS["DSS_" + k] for k in ("TILE_A", "TILE_B", "CHUNKS"))


def _fold_width(n_bits):
    if isinstance(n_bits, bool) or not isinstance(n_bits, int):
        raise TypeError(f"n_bits must be an int, got {type(n_bits).__name__}")
    if not (64 <= n_bits <= MORGAN_MAX_BITS and n_bits & (n_bits - 1) == 0):
        raise ValueError(f"n_bits must be a power of two in [64, {MORGAN_MAX_BITS}], got {n_bits}")
    return n_bits


def _one_device(name, tensors):
    dev = tensors[0].device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError(f"{name} needs all its tensors on one HIP device (torch device type 'cuda'); there is no CPU path")
    return dev


def fold_bits(ids: torch.Tensor, count: torch.Tensor, n_bits: int = 1024):
    """``dss_fold_bits``: the feature lists of ``morgan_records`` (``ids [P, 116] i64`` bit patterns, ``count [P] i32``) folded to packed bit rows:
    ``(words [P, n_bits / 64] i64, popcount [P] i32)`` on the current stream without synchronising.  Bit ``f mod n_bits`` is set for every
    feature f; bit b lives in word ``b // 64`` at position ``b % 64`` (int64 bit patterns: read them as unsigned with ``& (2**64 - 1)``).
    ``n_bits`` is a power of two in [64, 4096].  A count outside [0, 116] is clamped.  Checked, never converted; no CPU path."""
    n_bits = _fold_width(n_bits)
    _want(ids, "ids", torch.int64, (None, MORGAN_MAX_FEATURES))
    _want(count, "count", torch.int32, (ids.shape[0],))
    dev = _one_device("fold_bits", [ids, count])
    lib = load_library()
    P = ids.shape[0]
    words = torch.empty(P, n_bits // 64, dtype=torch.int64, device=dev)
    popcount = torch.empty(P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = lib.dss_fold_bits(ptr(ids), ptr(count), P, n_bits, ptr(words), ptr(popcount), _stream())
    _check(st, "dss_fold_bits")
    return words, popcount


def tanimoto_nn_workspace_bytes(Na: int, Nb: int) -> int:
    """``dss_tanimoto_nn_workspace_bytes``: the device bytes ``tanimoto_nn`` needs for ``Na`` rows against ``Nb`` (a pure host function)."""
    size = C.c_int64(0)
    _check(load_library().dss_tanimoto_nn_workspace_bytes(int(Na), int(Nb), C.byref(size)), "dss_tanimoto_nn_workspace_bytes")
    return int(size.value)


def tanimoto_nn(a_words: torch.Tensor, a_pop: torch.Tensor, b_words: torch.Tensor, b_pop: torch.Tensor, n_bits: int, skip_same_index: bool = False,
                workspace: Optional[torch.Tensor] = None):
    """``dss_tanimoto_nn``: every bit row of A against every bit row of B (``fold_bits`` makes them: ``a_words [Na, n_bits / 64] i64``, ``a_pop
    [Na] i32``, ``b_words [Nb, n_bits / 64] i64``, ``b_pop [Nb] i32``); with ``skip_same_index`` row i of A leaves out row i of B (A against
    itself without the self-pairs).  Tanimoto ``T = c / u``, ``c = popcount(a & b)``, ``u = |a| + |b| - c``, and ``T = 1`` for two empty rows.

    Returns the device tensors ``(best_common [Na] i32, best_union [Na] i32, best_index [Na] i64, sum [Na] f64, compared [Na] i64)`` on the
    current stream without synchronising: c, u and the row of the most similar row of B (decided in integers; among equals the lowest row;
    -1 / -1 / -1 when nothing was compared), the fp64 sum of T over the compared rows and their number.  Bit-identical from run to run.
    ``workspace``: a ``uint8`` device tensor of at least ``tanimoto_nn_workspace_bytes(Na, Nb)`` bytes, allocated here when ``None``.  Checked,
    never converted; no CPU path."""
    n_bits = _fold_width(n_bits)
    if not isinstance(skip_same_index, bool):
        raise TypeError(f"skip_same_index must be a bool, got {type(skip_same_index).__name__}")
    _want(a_words, "a_words", torch.int64, (None, n_bits // 64))
    _want(a_pop, "a_pop", torch.int32, (a_words.shape[0],))
    _want(b_words, "b_words", torch.int64, (None, n_bits // 64))
    _want(b_pop, "b_pop", torch.int32, (b_words.shape[0],))
    Na, Nb = a_words.shape[0], b_words.shape[0]
    tensors = [a_words, a_pop, b_words, b_pop]
    need = tanimoto_nn_workspace_bytes(Na, Nb)
    if workspace is not None:
        _want(workspace, "workspace", torch.uint8, (None,))
        if workspace.shape[0] < need:
            raise ValueError(f"workspace holds {workspace.shape[0]} bytes, {need} are needed for {Na} rows against {Nb}")
        tensors.append(workspace)
    dev = _one_device("tanimoto_nn", tensors)
    lib = load_library()
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    i32 = lambda: torch.empty(Na, dtype=torch.int32, device=dev)
    out = (i32(), i32(), torch.empty(Na, dtype=torch.int64, device=dev), torch.empty(Na, dtype=torch.float64, device=dev),
           torch.empty(Na, dtype=torch.int64, device=dev))
    with torch.cuda.device(dev):
        st = lib.dss_tanimoto_nn(ptr(a_words), ptr(a_pop), Na, ptr(b_words) if Nb else None, ptr(b_pop) if Nb else None, Nb, n_bits,
                                 int(skip_same_index), ptr(workspace), workspace.shape[0], *(ptr(t) for t in out), _stream())
    _check(st, "dss_tanimoto_nn")
    return out


# ----------------------------------------------------------------------------------------- valence analytics: stability, validity, fragments

VALENCE_CONSTS = abi.VALENCE.consts       # include/diffspectra_valence.h
BONDS_RECORD, BONDS_DISTANCE = VALENCE_CONSTS["DSV_BONDS_RECORD"], VALENCE_CONSTS["DSV_BONDS_DISTANCE"]
VALENCE_OK, VALENCE_UNUSABLE = VALENCE_CONSTS["DSV_OK"], VALENCE_CONSTS["DSV_UNUSABLE"]


def _bonds_from(bonds_from):
    if isinstance(bonds_from, bool) or not isinstance(bonds_from, int):
        raise TypeError(f"bonds_from must be an int, got {type(bonds_from).__name__}")
    if bonds_from not in (BONDS_RECORD, BONDS_DISTANCE):
        raise ValueError(f"bonds_from must be BONDS_RECORD ({BONDS_RECORD}) or BONDS_DISTANCE ({BONDS_DISTANCE}), got {bonds_from}")
    return bonds_from


def valence_records(rec: torch.Tensor, n: torch.Tensor, bonds_from: int = 0):
    """``dsv_valence_records``: valences, stability, validity and fragments of every record (definitions in ``include/diffspectra_valence.h``).
    ``bonds_from``: ``BONDS_RECORD`` (0: the record's bond bytes, the 2-D tables with the raw charge bytes) or ``BONDS_DISTANCE`` (1: orders from
    the fp32 positions with the arithmetic of ``ds_check_stability``, every charge 0).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(valence [P, 29] u8, stable_mask [P] i32, valid_mask [P] i32, summary [P, 4] i32,
    largest_mask [P] i32, status [P] u8)`` on the current stream without synchronising: the masks hold a bit per atom, ``summary`` is (n, stable
    atoms, fragments, atoms of the largest fragment), status ``VALENCE_UNUSABLE`` (3: n = 0, a type above 4, a bond byte above 3) zeroes the row.
    The validity restates RDKit's valence check and is unpinned against RDKit.  Checked, never converted; no CPU path."""
    i32 = (torch.int32, ())
    return _record_call("valence_records", [(rec, n)], None, [_bonds_from(bonds_from)],
                        [(torch.uint8, (MAX_ATOMS,)), i32, i32, (torch.int32, (4,)), i32, (torch.uint8, ())], prefix="dsv_")


def fragment_records(rec: torch.Tensor, n: torch.Tensor, keep: torch.Tensor, bonds_from: int = 0, charge_rule: bool = True):
    """``dsv_fragment_records``: the atoms of ``keep [P] i32`` (bit i = keep atom i; bits at and above n are ignored) of every record as a
    well-formed record of their own, atoms in ascending original order: ``(out_rec [P, 1248] u8, out_n [P] i32)`` on the current stream without
    synchronising.  ``charge_rule`` writes the charge the reference applies to its RDKit atom (N+1, N-1, C+1, O-1, C-1; else 0) instead of the
    raw byte; with ``BONDS_DISTANCE`` the bonds written are the derived orders and every charge is 0.  An unusable record gives ``out_n = 0`` and
    zeros.  With ``valence_records``' ``largest_mask`` this is the largest fragment.  Checked, never converted; no CPU path."""
    if not isinstance(charge_rule, bool):
        raise TypeError(f"charge_rule must be a bool, got {type(charge_rule).__name__}")
    _want(rec, "rec", torch.uint8, (None, RECORD_BYTES))
    _want(keep, "keep", torch.int32, (rec.shape[0],))
    return _record_call("fragment_records", [(rec, n)], None, [_bonds_from(bonds_from), ptr(keep), int(charge_rule)],
                        [(torch.uint8, (RECORD_BYTES,)), (torch.int32, ())], prefix="dsv_", also=[keep])


# ----------------------------------------------------------------------------------------- functional groups and aromaticity

GROUPS_CONSTS = abi.GROUPS.consts         # include/diffspectra_groups.h
GROUPS_OK, GROUPS_UNUSABLE, GROUPS_INVALID = (GROUPS_CONSTS["DSG_" + k] for k in ("OK", "UNUSABLE", "INVALID"))
NUM_GROUPS = GROUPS_CONSTS["DSG_NUM_GROUPS"]


def group_records(rec: torch.Tensor, n: torch.Tensor):
    """``dsg_group_records``: the functional groups and the aromatic atoms of every record (definitions in ``include/diffspectra_groups.h``: the
    17 groups of the reference's ``compute_metrics.py:38-56`` as predicates on the record graph, on top of the project's own, order-free
    aromaticity rule, whose parity with RDKit is unpinned).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(groups [P] i32, aromatic_mask [P] i32, status [P] u8)`` on the current stream
    without synchronising: bit g of ``groups`` = group g is present, bit i of ``aromatic_mask`` = atom i is aromatic, status ``GROUPS_UNUSABLE``
    (2: n = 0, a type above 4, a bond byte above 3) zeroes the row.  Checked, never converted; no CPU path."""
    i32 = (torch.int32, ())
    return _record_call("group_records", [(rec, n)], None, [], [i32, i32, (torch.uint8, ())], prefix="dsg_")


def group_similarity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                             ref_index: Optional[torch.Tensor] = None):
    """``dsg_group_similarity_records``: the functional groups of both molecules of each of P (generated, ground-truth) pairs and the two
    counts behind their Jaccard similarity - the reference's "Functional Group Similarity" (``compute_metrics.py:117-144``).

    The tensors are those of ``match_records``.  Returns the device tensors ``(common [P] i32, either [P] i32, groups [P, 2] i32, status [P] u8)``,
    enqueued on the current stream without synchronising: the sizes of the intersection and of the union of the two group sets, the group
    words (generated, ground truth), status ``GROUPS_OK`` (0), ``GROUPS_UNUSABLE`` (2: a record of the pair is unusable) or ``GROUPS_INVALID`` (3:
    ``ref_index`` outside the table); a pair that is not ok has ``common = either = -1`` and ``groups = 0``.  Checked, never converted."""
    i32 = (torch.int32, ())
    return _record_call("group_similarity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, [], [i32, i32, (torch.int32, (2,)), (torch.uint8, ())],
                        prefix="dsg_")


# ----------------------------------------------------------------------------------------- scaffolds, ring atoms, ring counts

SCAFFOLD_CONSTS = abi.SCAFFOLD.consts     # include/diffspectra_scaffold.h
SCAFFOLD_OK, SCAFFOLD_UNUSABLE = SCAFFOLD_CONSTS["DSK_OK"], SCAFFOLD_CONSTS["DSK_UNUSABLE"]


def scaffold_masks(rec: torch.Tensor, n: torch.Tensor):
    """``dsk_scaffold_masks``: the Bemis-Murcko scaffold atoms, the ring atoms and the ring count of every record (definitions in
    ``include/diffspectra_scaffold.h``: the 2-core of the heavy graph plus its exocyclic atoms, ring bonds by reachability, the cyclomatic
    number of the core; the scaffold rule restates RDKit's ``GetScaffoldForMol`` and is unpinned against RDKit).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(scaffold_mask [P] i32, ring_mask [P] i32, summary [P, 4] i32, status [P] u8)`` on
    the current stream without synchronising: the masks hold a bit per atom, ``summary`` is (heavy atoms, scaffold atoms, rings, ring atoms),
    status ``SCAFFOLD_UNUSABLE`` (3: n = 0, a type above 4, a bond byte above 3) zeroes the row.  Checked, never converted; no CPU path."""
    i32 = (torch.int32, ())
    return _record_call("scaffold_masks", [(rec, n)], None, [], [i32, i32, (torch.int32, (4,)), (torch.uint8, ())], prefix="dsk_")


# ----------------------------------------------------------------------------------------- BRICS cuts and fragments

BRICS_CONSTS = abi.BRICS.consts           # include/diffspectra_brics.h
BRICS_OK, BRICS_UNUSABLE = BRICS_CONSTS["DSB_OK"], BRICS_CONSTS["DSB_UNUSABLE"]
BRICS_MAX_CUTS, BRICS_ATTACH_TYPE, BRICS_AROMATIC_ORDER = (BRICS_CONSTS["DSB_" + k] for k in ("MAX_CUTS", "ATTACH_TYPE", "AROMATIC_ORDER"))


def brics_records(rec: torch.Tensor, n: torch.Tensor):
    """``dsb_brics_records``: the BRICS environments of every atom, the cut bonds with their labels and the fragment of every atom (every
    definition in ``include/diffspectra_brics.h``: thirteen environments and forty rules on the hydrogen-folded graph of the substructure
    matcher, restated from RDKit's ``BRICS.py`` as remembered and unpinned against RDKit).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(env [P, 29] i32, cuts [P, 28, 4] u8, fragment_of [P, 29] u8, summary [P, 4] i32,
    status [P] u8)`` on the current stream without synchronising: bit e of ``env`` = the atom is in L_e; a row of ``cuts`` is (a, b, label of a,
    label of b) with a < b, ascending, 0xff where unused; ``fragment_of`` is 0xff for atoms >= n; ``summary`` is (matchable atoms, cuts,
    fragments, atoms of the largest fragment); status ``BRICS_UNUSABLE`` (3: n = 0, a type above 4, a bond byte above 3) zeroes the row
    (``cuts`` and ``fragment_of``: 0xff).  Checked, never converted; no CPU path."""
    return _record_call("brics_records", [(rec, n)], None, [],
                        [(torch.int32, (MAX_ATOMS,)), (torch.uint8, (BRICS_MAX_CUTS, 4)), (torch.uint8, (MAX_ATOMS,)), (torch.int32, (4,)), (torch.uint8, ())],
                        prefix="dsb_")


def brics_fragment_records(rec: torch.Tensor, n: torch.Tensor, first: torch.Tensor, rows: int, aromatic: bool = True):
    """``dsb_brics_fragment_records``: every BRICS fragment as a record of its own, with its attachment points (type byte 5, the label in the
    charge byte).  ``first [P] i64``: the exclusive prefix sum of ``brics_records(...)[3][:, 2]``; ``rows``: the number of output rows F, the
    total of that column (a row outside [0, F) is never written).  ``aromatic`` writes aromatic bonds as order 4 instead of their Kekule order.

    -> the device tensors ``(out_rec [F, 1248] u8, out_n [F] i32, out_owner [F] i64, out_source [F, 29] u8)`` on the current stream without
    synchronising; rows that no fragment is written to are zero (``out_source``: 0xff).  Checked, never converted; no CPU path."""
    if not isinstance(aromatic, bool):
        raise TypeError(f"aromatic must be a bool, got {type(aromatic).__name__}")
    if isinstance(rows, bool) or not isinstance(rows, int):
        raise TypeError(f"rows must be an int, got {type(rows).__name__}")
    if rows < 0:
        raise ValueError(f"rows must not be negative, got {rows}")
    _want(rec, "rec", torch.uint8, (None, RECORD_BYTES))
    _want(n, "n", torch.int32, (rec.shape[0],))
    _want(first, "first", torch.int64, (rec.shape[0],))
    tensors = [rec, n, first]
    dev = rec.device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError("brics_fragment_records needs all its tensors on one HIP device (torch device type 'cuda'); there is no CPU path")
    lib = load_library()
    out = (torch.zeros(rows, RECORD_BYTES, dtype=torch.uint8, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev),
           torch.zeros(rows, dtype=torch.int64, device=dev), torch.full((rows, MAX_ATOMS), 0xff, dtype=torch.uint8, device=dev))
    if rows and rec.shape[0]:                                                   # nothing to write otherwise, and an empty tensor has no address
        with torch.cuda.device(dev):
            st = lib.dsb_brics_fragment_records(ptr(rec), ptr(n), rec.shape[0], ptr(first), rows, int(aromatic), *(ptr(t) for t in out), _stream())
        _check(st, "dsb_brics_fragment_records")
    return out


# ----------------------------------------------------------------------------------------- mobile hydrogens and the normal form

MOBILE_CONSTS = abi.MOBILE.consts         # include/diffspectra_mobile.h
MOBILE_OK, MOBILE_UNDECIDED, MOBILE_UNUSABLE, MOBILE_OVERFLOW = (MOBILE_CONSTS["DSM_" + k] for k in ("OK", "UNDECIDED", "UNUSABLE", "OVERFLOW"))
MOBILE_MAX_NODES, MOBILE_MAX_GROUPS = MOBILE_CONSTS["DSM_MAX_NODES"], MOBILE_CONSTS["DSM_MAX_GROUPS"]
MOBILE_GROUP_TYPE, MOBILE_PROTON_TYPE = MOBILE_CONSTS["DSM_GROUP_TYPE"], MOBILE_CONSTS["DSM_PROTON_TYPE"]
MOBILE_DEFAULT_NODES = 4096               # far above what a molecule of 29 atoms spends


def _mobile_budget(max_nodes):
    if max_nodes is None:
        return MOBILE_DEFAULT_NODES
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, int):
        raise TypeError(f"max_nodes must be an int, got {type(max_nodes).__name__}")
    if not 1 <= max_nodes <= MOBILE_MAX_NODES:
        raise ValueError(f"max_nodes must lie in [1, {MOBILE_MAX_NODES}], got {max_nodes}")
    return max_nodes


def mobile_records(rec: torch.Tensor, n: torch.Tensor, max_nodes: Optional[int] = None):
    """``dsm_mobile_records``: the mobile-hydrogen groups, fixed hydrogens, residual charges and proton balance of every record (every
    definition in ``include/diffspectra_mobile.h``: a restatement of InChI's mobile-H and (de)protonation normalisation as remembered, unpinned
    against InChI).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(fixed_h [P, 29] u8, q_res [P, 29] i8, group_of [P, 29] u8, group_h [P, 14] u8,
    summary [P, 4] i32, nodes [P] i32, status [P] u8)`` on the current stream without synchronising: ``fixed_h`` is 0xff for a folded hydrogen
    and for atoms >= n and 0 for a group member; ``group_of`` and ``group_h`` are 0xff where there is no group; ``summary`` is (kept atoms, groups,
    mobile H in all, proton balance); status ``MOBILE_UNUSABLE`` (3) or ``MOBILE_UNDECIDED`` (2: the path search needed more than ``max_nodes``,
    default 4096) makes the three byte outputs 0xff and zeroes the rest.  Checked, never converted; no CPU path."""
    i8 = (torch.uint8, (MAX_ATOMS,))
    return _record_call("mobile_records", [(rec, n)], None, [_mobile_budget(max_nodes)],
                        [i8, (torch.int8, (MAX_ATOMS,)), i8, (torch.uint8, (MOBILE_MAX_GROUPS,)), (torch.int32, (4,)), (torch.int32, ()), (torch.uint8, ())],
                        prefix="dsm_")


def normal_records(rec: torch.Tensor, n: torch.Tensor, max_nodes: Optional[int] = None):
    """``dsm_normal_records``: every record in the normal form of ``include/diffspectra_mobile.h`` - kept atoms with charge byte ``fixed H +
    16 * (q_res + 1)``, every bond as byte 1, one group node (type byte 6, the mobile H in the charge byte) bonded to the members of every
    mobile group and a proton node (type byte 7, the balance in the charge byte) when the balance is not 0 - so that ``graph_identity_records``
    and ``graph_hash_records`` on the rows decide identity up to tautomers, acid / base forms and Kekule drawings.

    -> the device tensors ``(out_rec [P, 1248] u8, out_n [P] i32, out_source [P, 29] u8, status [P] u8)`` on the current stream without
    synchronising; a row whose status is not ``MOBILE_OK`` (``MOBILE_OVERFLOW`` = 4: more than 29 nodes) is zero with ``out_n`` 0 and
    ``out_source`` 0xff.  Checked, never converted; no CPU path."""
    return _record_call("normal_records", [(rec, n)], None, [_mobile_budget(max_nodes)],
                        [(torch.uint8, (RECORD_BYTES,)), (torch.int32, ()), (torch.uint8, (MAX_ATOMS,)), (torch.uint8, ())], prefix="dsm_")


# ----------------------------------------------------------------------------------------- Fraggle similarity

FRAGGLE_CONSTS = abi.FRAGGLE.consts       # include/diffspectra_fraggle.h
FRAGGLE_OK, FRAGGLE_UNDECIDED, FRAGGLE_UNUSABLE, FRAGGLE_INVALID = (FRAGGLE_CONSTS["DSF_" + k] for k in ("OK", "UNDECIDED", "UNUSABLE", "INVALID"))
FRAGGLE_MAX_NODES, FRAGGLE_DEFAULT_NODES = FRAGGLE_CONSTS["DSF_MAX_NODES"], FRAGGLE_CONSTS["DSF_DEFAULT_NODES"]
FRAGGLE_MAX_FRAGMENTATIONS, FRAGGLE_TRUNCATED, FRAGGLE_NO_CUT = (FRAGGLE_CONSTS["DSF_" + k] for k in ("MAX_FRAGMENTATIONS", "TRUNCATED", "NO_CUT"))
FRAGGLE_FP_WORDS = FRAGGLE_CONSTS["DSF_FP_WORDS"]


def _fraggle_budget(max_nodes):
    if max_nodes is None:
        return FRAGGLE_DEFAULT_NODES
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, int):
        raise TypeError(f"max_nodes must be an int, got {type(max_nodes).__name__}")
    if not 1 <= max_nodes <= FRAGGLE_MAX_NODES:
        raise ValueError(f"max_nodes must lie in [1, {FRAGGLE_MAX_NODES}], got {max_nodes}")
    return max_nodes


def fraggle_fragmentations(rec: torch.Tensor, n: torch.Tensor, max_nodes: Optional[int] = None):
    """``dsf_fraggle_fragmentations``: the Fraggle fragmentations of every record - one or two chain cuts, two ring cuts, two ring cuts and a
    chain cut - in the order and under the size rules of ``include/diffspectra_fraggle.h`` (a restatement of RDKit's Fraggle as remembered,
    unpinned against RDKit).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(rows [P, 256, 4] i32, summary [P, 4] i32, status [P] u8)`` on the current stream
    without synchronising: a row is (kept-atom mask, cuts packed ten bits each as lower atom | higher atom << 5 with ``FRAGGLE_NO_CUT`` for an
    unused one, kind, sum of the kept sizes), unused rows are -1; ``summary`` is (matchable atoms, chain cut bonds, ring cut bonds, fragmentations
    with ``FRAGGLE_TRUNCATED`` set when there are more than rows).  Status ``FRAGGLE_UNUSABLE`` (2) or ``FRAGGLE_UNDECIDED`` (1: the graph has more
    than ``max_nodes`` connected bond sets, default 32768) gives rows of -1 and a zero summary.  Checked, never converted; no CPU path."""
    return _record_call("fraggle_fragmentations", [(rec, n)], None, [_fraggle_budget(max_nodes)],
                        [(torch.int32, (FRAGGLE_MAX_FRAGMENTATIONS, 4)), (torch.int32, (4,)), (torch.uint8, ())], prefix="dsf_")


def path_fingerprints(rec: torch.Tensor, n: torch.Tensor, max_nodes: Optional[int] = None):
    """``dsf_path_fingerprints``: the branched path fingerprint of every record (every connected set of 1..5 bonds sets 2 of 1024 bits; the
    project's own hash, stated in ``include/diffspectra_fraggle.h``) with the bits of every atom.

    -> the device tensors ``(fp [P, 32] i32, atom_bits [P, 29, 32] i32, count [P] i32, status [P] u8)`` on the current stream without
    synchronising; ``count`` is the number of bond sets, -1 for ``FRAGGLE_UNDECIDED`` (more than ``max_nodes``), 0 for ``FRAGGLE_UNUSABLE``; a row
    that is not ok has ``fp = atom_bits = 0``.  Checked, never converted; no CPU path."""
    return _record_call("path_fingerprints", [(rec, n)], None, [_fraggle_budget(max_nodes)],
                        [(torch.int32, (FRAGGLE_FP_WORDS,)), (torch.int32, (MAX_ATOMS, FRAGGLE_FP_WORDS)), (torch.int32, ()), (torch.uint8, ())], prefix="dsf_")


def fraggle_similarity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                               ref_index: Optional[torch.Tensor] = None, max_nodes: Optional[int] = None):
    """``dsf_fraggle_similarity_records``: the Fraggle similarity of P (generated, ground-truth) pairs as integers - the ground truth is the
    query that is fragmented, as in the reference's ``GetFraggleSimilarity(true_mol, pred_mol)``.

    The tensors are those of ``match_records``.  Returns the device tensors ``(plain [P, 2] i32, modified [P, 2] i32, best_index [P] i32,
    n_fragmentations [P] i32, marked [P, 2] i32, status [P] u8)``, enqueued on the current stream without synchronising: ``plain`` and ``modified``
    are (common, either) bit counts of the plain fingerprints and of the best marked pair over all fragmentations (-1, -1 without one),
    ``marked`` the marked-atom masks of the ground truth and of the generated molecule for that fragmentation; status ``FRAGGLE_OK`` (0),
    ``FRAGGLE_UNDECIDED`` (1: a fingerprint needed more than ``max_nodes`` bond sets), ``FRAGGLE_UNUSABLE`` (2) or ``FRAGGLE_INVALID`` (3:
    ``ref_index`` outside the table); a pair that is not ok has -1 in ``plain``, ``modified`` and ``best_index`` and 0 elsewhere.  Checked, never
    converted."""
    i32, two = (torch.int32, ()), (torch.int32, (2,))
    return _record_call("fraggle_similarity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index, [_fraggle_budget(max_nodes)],
                        [two, two, i32, i32, two, (torch.uint8, ())], prefix="dsf_")


# ----------------------------------------------------------------------------------------- canonical SMILES

SMILES_CONSTS = abi.SMILES.consts         # include/diffspectra_smiles.h
SMILES_OK, SMILES_UNCERTIFIED, SMILES_OVERFLOW, SMILES_UNUSABLE = (SMILES_CONSTS["DSL_" + k] for k in ("OK", "UNCERTIFIED", "OVERFLOW", "UNUSABLE"))
SMILES_TEXT_BYTES = SMILES_CONSTS["DSL_TEXT_BYTES"]


def smiles_records(rec: torch.Tensor, n: torch.Tensor, max_nodes: int = 4096):
    """``dsl_smiles_records``: the canonical SMILES string of every record (every definition in ``include/diffspectra_smiles.h``: hydrogens
    folded into their neighbours, colour refinement with individualisation, the smallest certificate, a Kekule OpenSMILES subset; not
    RDKit's canonical form).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(text [P, 384] u8, length [P] i32, status [P] u8, nodes [P] i32, atom_order
    [P, 29] i32)`` on the current stream without synchronising: ``text`` is ASCII, zero after ``length``; status ``SMILES_OK`` (0),
    ``SMILES_UNCERTIFIED`` (1: the search stopped at ``max_nodes`` individualisations; the string is valid, not canonical), ``SMILES_OVERFLOW``
    (2: more than 99 ring numbers open or more than 384 bytes) or ``SMILES_UNUSABLE`` (3: n = 0, a type above 4, a bond byte above 3) - for 2
    and 3 the row is empty; ``atom_order`` is the position of every record atom among the atoms of the string, -1 for folded hydrogens.
    Checked, never converted; no CPU path."""
    return _record_call("smiles_records", [(rec, n)], None, [_node_budget(max_nodes, GRAPH_MAX_NODES)],
                        [(torch.uint8, (SMILES_TEXT_BYTES,)), (torch.int32, ()), (torch.uint8, ()), (torch.int32, ()), _MAP], prefix="dsl_")


# ----------------------------------------------------------------------------------------- SMILES reader

READER_CONSTS = abi.READER.consts         # include/diffspectra_reader.h
READER_STATUSES = ("OK", "EMPTY", "SYNTAX", "ELEMENT", "KEKULE", "TOO_LARGE", "UNDECIDED", "TOO_LONG")
READER_OK, READER_EMPTY, READER_SYNTAX, READER_ELEMENT, READER_KEKULE, READER_TOO_LARGE, READER_UNDECIDED, READER_TOO_LONG = \
    (READER_CONSTS["DSP_" + k] for k in READER_STATUSES)
READER_TEXT_BYTES, READER_WAVES = READER_CONSTS["DSP_TEXT_BYTES"], READER_CONSTS["DSP_WAVES"]


def read_smiles(text: torch.Tensor, length: torch.Tensor, max_nodes: int = 4096):
    """``dsp_read_smiles``: the result record of every SMILES string (every definition in ``include/diffspectra_reader.h``: the accepted
    OpenSMILES subset, the first error and its offset, aromatic bonds as ring bonds between lower-case atoms, the first Kekule structure of a
    stated depth-first order, implied hydrogens appended behind the atoms of the string; not RDKit's reader).

    ``text [P, stride] u8`` (ASCII rows; the stride a multiple of 4 in [4, 384]), ``length [P] i32`` -> the device tensors ``(rec [P, 1248] u8,
    n [P] i32, status [P] u8, where [P] i32, string_atoms [P] i32, flags [P] u32-as-i32, aromatic [P] u32-as-i32, atom_pos [P, 29] i32, nodes
    [P] i32)`` on the current stream without synchronising; status ``READER_OK`` (0) .. ``READER_TOO_LONG`` (7); unless it is 0 the record is
    zero and ``n`` is 0.  Checked, never converted; no CPU path."""
    _want(text, "text", torch.uint8, (None, None))
    P, stride = text.shape
    if stride % 4 or not 4 <= stride <= READER_TEXT_BYTES:
        raise ValueError(f"text must have a stride that is a multiple of 4 in [4, {READER_TEXT_BYTES}], got {stride}")
    _want(length, "length", torch.int32, (P,))
    max_nodes = _node_budget(max_nodes, GRAPH_MAX_NODES)
    dev = text.device
    if dev.type != "cuda" or length.device != dev:
        raise RuntimeError("read_smiles needs all its tensors on one HIP device (torch device type 'cuda'); there is no CPU path")
    lib = load_library()
    i32 = lambda *shape: torch.empty(P, *shape, dtype=torch.int32, device=dev)
    out = (torch.empty(P, RECORD_BYTES, dtype=torch.uint8, device=dev), i32(), torch.empty(P, dtype=torch.uint8, device=dev), i32(), i32(), i32(),
           i32(), i32(MAX_ATOMS), i32())
    with torch.cuda.device(dev):
        st = lib.dsp_read_smiles(ptr(text), stride, ptr(length), P, max_nodes, *(ptr(t) for t in out), _stream())
    _check(st, "dsp_read_smiles")
    return out


# ----------------------------------------------------------------------------------------- substructure queries

SUBSTRUCTURE_CONSTS = abi.SUBSTRUCTURE.consts       # include/diffspectra_substructure.h
SUBSTRUCTURE_OK, SUBSTRUCTURE_UNUSABLE = SUBSTRUCTURE_CONSTS["DSQ_OK"], SUBSTRUCTURE_CONSTS["DSQ_UNUSABLE"]
SUBSTRUCTURE_TRUNCATED, SUBSTRUCTURE_COUNT_CAP = SUBSTRUCTURE_CONSTS["DSQ_TRUNCATED"], SUBSTRUCTURE_CONSTS["DSQ_COUNT_CAP"]
PATTERN_WORDS, MAX_PATTERNS = SUBSTRUCTURE_CONSTS["DSQ_PATTERN_WORDS"], SUBSTRUCTURE_CONSTS["DSQ_MAX_PATTERNS"]
SUBSTRUCTURE_MAX_NODES, SUBSTRUCTURE_DEFAULT_NODES = SUBSTRUCTURE_CONSTS["DSQ_MAX_NODES"], SUBSTRUCTURE_CONSTS["DSQ_DEFAULT_NODES"]


def substructure_records(rec: torch.Tensor, n: torch.Tensor, patterns: torch.Tensor, max_nodes: int = SUBSTRUCTURE_DEFAULT_NODES):
    """``dsq_match_records``: every pattern of ``patterns [K, 32] i32`` (``smarts.compile_patterns``; K <= 256, K = 0 is legal) against every
    record (every definition in ``include/diffspectra_substructure.h``: the hydrogen-folded matched graph, the per-atom properties, the eight
    bond classes, the defined depth-first search with ``max_nodes`` assignments per start atom, in [1, 2^24]).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(count [P, K] u8, anchors [P, K] i32, cover [P, K] i32, aromatic_mask [P] i32,
    aromatic_rings [P] i32, fragments [P] i32, status [P] u8)`` on the current stream without synchronising: ``count`` is the number of distinct
    atom sets over the embeddings, saturating at 4, with bit 7 (``SUBSTRUCTURE_TRUNCATED``) set where a search stopped at its budget; ``anchors``
    and ``cover`` hold a bit per record atom (the images of pattern atom 0, of any pattern atom); status ``SUBSTRUCTURE_UNUSABLE`` (2: n = 0, a type
    above 4, a bond byte above 3) zeroes the row.  Checked, never converted; no CPU path."""
    _want(patterns, "patterns", torch.int32, (None, PATTERN_WORDS))
    K = patterns.shape[0]
    if K > MAX_PATTERNS:
        raise ValueError(f"patterns holds {K} patterns, at most {MAX_PATTERNS} go into one call")
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, int):
        raise TypeError(f"max_nodes must be an int, got {type(max_nodes).__name__}")
    if not 1 <= max_nodes <= SUBSTRUCTURE_MAX_NODES:
        raise ValueError(f"max_nodes must lie in [1, {SUBSTRUCTURE_MAX_NODES}], got {max_nodes}")
    i32 = (torch.int32, ())
    return _record_call("match_records", [(rec, n)], None, [ptr(patterns) if K else None, K, max_nodes],
                        [(torch.uint8, (K,)), (torch.int32, (K,)), (torch.int32, (K,)), i32, i32, i32, (torch.uint8, ())], prefix="dsq_", also=[patterns])


# ----------------------------------------------------------------------------------------- stereo-aware identity

STEREO_CONSTS = abi.STEREO.consts         # include/diffspectra_stereo.h
STEREO_DIFFERENT, STEREO_IDENTICAL, STEREO_UNDECIDED, STEREO_INVALID, STEREO_MIRROR, STEREO_STEREOISOMER, STEREO_UNASSIGNED = (
    STEREO_CONSTS["DSC_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID", "MIRROR", "STEREOISOMER", "UNASSIGNED"))
STEREO_MIN_VOLUME, STEREO_MIN_PLANARITY = abi.STEREO.reals["DSC_MIN_VOLUME"], abi.STEREO.reals["DSC_MIN_PLANARITY"]
STEREO_OK, STEREO_UNUSABLE, STEREO_NUM_MASKS = STEREO_CONSTS["DSC_OK"], STEREO_CONSTS["DSC_UNUSABLE"], STEREO_CONSTS["DSC_NUM_MASKS"]


def _stereo_thresholds(min_volume, min_planarity):
    """The two thresholds as floats, ``None`` = the header's default; a NaN or a negative one raises."""
    out = []
    for name, value, default in (("min_volume", min_volume, STEREO_MIN_VOLUME), ("min_planarity", min_planarity, STEREO_MIN_PLANARITY)):
        value = default if value is None else float(value)
        if not value >= 0.0:
            raise ValueError(f"{name} must be a number >= 0, got {value}")
        out.append(value)
    return out


def stereo_identity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                            ref_index: Optional[torch.Tensor] = None, max_nodes: int = 4096, min_volume: Optional[float] = None,
                            min_planarity: Optional[float] = None, exhaustive: bool = False):
    """``dsc_stereo_identity_records``: is the generated molecule of each of P pairs the same labelled graph as its ground truth AND the same
    stereoisomer, read from the records' positions (every definition in ``include/diffspectra_stereo.h``: twins and ordinals, tetrahedral
    and E/Z sites with the thresholds ``min_volume`` / ``min_planarity`` - ``None``: the header's 0.5 / 0.5 -, same and mirror isomorphisms).

    The tensors are those of ``match_records``.  Returns the device tensors ``(verdict [P] u8, nodes [P] i32, found [P, 3] i32, sites [P, 4]
    i32, map [P, 29] i32)``, enqueued on the current stream without synchronising: verdict ``STEREO_DIFFERENT`` (0), ``STEREO_IDENTICAL`` (1),
    ``STEREO_UNDECIDED`` (2: the search needed more than ``max_nodes`` tries), ``STEREO_INVALID`` (3), ``STEREO_MIRROR`` (4: an enantiomer),
    ``STEREO_STEREOISOMER`` (5: a diastereomer or E/Z isomer) or ``STEREO_UNASSIGNED`` (6: same constitution, a site too flat to tell);
    ``found`` = isomorphisms, same, mirror met until the search stopped (``exhaustive=True``: it stops only when none is left); ``sites`` =
    tetrahedral and E/Z sites of the generated molecule, unassigned sites of it and of the ground truth; ``map`` = the isomorphism behind the
    verdict.  The arguments are checked, never converted."""
    if not isinstance(exhaustive, (bool, int)) or exhaustive not in (0, 1):
        raise TypeError(f"exhaustive must be a bool, got {exhaustive!r}")
    return _record_call("stereo_identity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index,
                        [_node_budget(max_nodes, GRAPH_MAX_NODES), *_stereo_thresholds(min_volume, min_planarity), int(exhaustive)],
                        [(torch.uint8, ()), (torch.int32, ()), (torch.int32, (3,)), (torch.int32, (4,)), _MAP], prefix="dsc_")


def stereo_sites(rec: torch.Tensor, n: torch.Tensor, min_volume: Optional[float] = None, min_planarity: Optional[float] = None):
    """``dsc_stereo_sites``: the twins and the stereo sites of every record (definitions in ``include/diffspectra_stereo.h``).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(masks [P, 7] i32, volume [P, 29] f64, status [P] u8)`` on the current stream
    without synchronising: the rows of ``masks`` hold a bit per atom (tetrahedral site, assigned, V > 0; end of an E/Z site, assigned, cis;
    twin - the header's ``DSC_MASK_*`` order), ``volume`` is V of every tetrahedral site and NaN elsewhere, status ``STEREO_UNUSABLE`` (3: n = 0,
    a type above 4, a bond byte above 3) zeroes the masks.  Checked, never converted; no CPU path."""
    return _record_call("stereo_sites", [(rec, n)], None, _stereo_thresholds(min_volume, min_planarity),
                        [(torch.int32, (STEREO_NUM_MASKS,)), (torch.float64, (MAX_ATOMS,)), (torch.uint8, ())], prefix="dsc_")


# ----------------------------------------------------------------------------------------- key-level identity: normal form and stereo at once

KEY_CONSTS = abi.KEY.consts               # include/diffspectra_key.h
KEY_KIND_MASK, KEY_KIND_CENTRE, KEY_KIND_END = (KEY_CONSTS["DSI_KIND_" + k] for k in ("MASK", "CENTRE", "END"))
KEY_FLAG_ASSIGNED, KEY_FLAG_SIGN, KEY_FLAG_HSLOT = (KEY_CONSTS["DSI_FLAG_" + k] for k in ("ASSIGNED", "SIGN", "HSLOT"))
KEY_NO_PARTNER, KEY_NUM_MASKS = KEY_CONSTS["DSI_NO_PARTNER"], KEY_CONSTS["DSI_NUM_MASKS"]
_KEY_SITE = (torch.uint8, (MAX_ATOMS, 2))


def key_sites(rec: torch.Tensor, n: torch.Tensor, max_nodes: Optional[int] = None, min_volume: Optional[float] = None,
              min_planarity: Optional[float] = None):
    """``dsi_key_sites``: the stereo sites of every ORIGINAL record at the level of its normal form (every definition in
    ``include/diffspectra_key.h``: excluded atoms, the hydrogen slot, centres, E/Z sites off every shift path and off every ring; a
    restatement of InChI as remembered, unpinned against it).

    ``rec [P, 1248] u8``, ``n [P] i32`` -> the device tensors ``(site [P, 29, 2] u8, masks [P, 9] i32, volume [P, 29] f64, nodes [P] i32,
    status [P] u8)`` on the current stream without synchronising, all in normal-form numbering (row p lines up with row p of
    ``normal_records`` with the same ``max_nodes``): ``site`` = (flags, partner) of every node; ``masks`` = the seven ``DSC_MASK_*`` rows, the
    ends of the double bonds on a shift path, the ends of the ring double bonds; ``volume`` = V of every centre, 0 elsewhere; a row whose
    status is not ``MOBILE_OK`` (undecided, unusable, overflow) is flags 0, partner 255, zeros.  Checked, never converted; no CPU path."""
    return _record_call("key_sites", [(rec, n)], None, [_mobile_budget(max_nodes), *_stereo_thresholds(min_volume, min_planarity)],
                        [_KEY_SITE, (torch.int32, (KEY_NUM_MASKS,)), (torch.float64, (MAX_ATOMS,)), (torch.int32, ()), (torch.uint8, ())],
                        prefix="dsi_")


def key_identity_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, prb_site: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                         ref_site: torch.Tensor, ref_index: Optional[torch.Tensor] = None, max_nodes: int = 4096, exhaustive: bool = False):
    """``dsi_key_identity_records``: the verdicts of ``stereo_identity_records`` for P pairs of NORMAL-FORM records (``normal_records``) with
    the site rows of ``key_sites`` beside them (``prb_site [P, 29, 2] u8``, ``ref_site [M, 29, 2] u8``): every isomorphism of the normal forms
    is tested against the sites (``include/diffspectra_key.h``).  Returns ``(verdict [P] u8, nodes [P] i32, found [P, 3] i32, sites [P, 4]
    i32, map [P, 29] i32)`` as there, the map in normal-form indices, on the current stream without synchronising.  Checked, never
    converted."""
    if not isinstance(exhaustive, (bool, int)) or exhaustive not in (0, 1):
        raise TypeError(f"exhaustive must be a bool, got {exhaustive!r}")
    _want(prb_site, "prb_site", torch.uint8, (prb_rec.shape[0], MAX_ATOMS, 2))
    _want(ref_site, "ref_site", torch.uint8, (ref_rec.shape[0], MAX_ATOMS, 2))
    return _record_call("key_identity_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index,
                        [ptr(prb_site), ptr(ref_site), _node_budget(max_nodes, GRAPH_MAX_NODES), int(exhaustive)],
                        [(torch.uint8, ()), (torch.int32, ()), (torch.int32, (3,)), (torch.int32, (4,)), _MAP], prefix="dsi_",
                        also=(prb_site, ref_site))


# ----------------------------------------------------------------------------------------- symmetry-corrected Kabsch RMSD

RMSD_CONSTS = abi.RMSD.consts             # include/diffspectra_rmsd.h
RMSD_DIFFERENT, RMSD_DECIDED, RMSD_UNDECIDED, RMSD_INVALID = (RMSD_CONSTS["DSR_" + k] for k in ("DIFFERENT", "DECIDED", "UNDECIDED", "INVALID"))
RMSD_ATOMS = {"heavy": RMSD_CONSTS["DSR_ATOMS_HEAVY"], "all": RMSD_CONSTS["DSR_ATOMS_ALL"]}


def _rmsd_atoms(atoms) -> int:
    """``'heavy'`` / ``'all'`` as the header's ``DSR_ATOMS_*`` number."""
    if not isinstance(atoms, str) or atoms not in RMSD_ATOMS:
        raise ValueError(f"atoms must be 'heavy' or 'all', got {atoms!r}")
    return RMSD_ATOMS[atoms]


def best_rmsd_records(prb_rec: torch.Tensor, prb_n: torch.Tensor, ref_rec: torch.Tensor, ref_n: torch.Tensor,
                      ref_index: Optional[torch.Tensor] = None, max_nodes: int = 4096, atoms="heavy"):
    """``dsr_best_rmsd_records``: the smallest Kabsch RMSD over ALL graph isomorphisms between the generated molecule and its ground truth of
    each of P pairs, for a rotation and for the mirror image (every definition in ``include/diffspectra_rmsd.h``: the selection ``atoms`` -
    ``'heavy'``: type byte not 0, ``'all'`` -, the trace formula, the twins of hydrogen leaves, the verdicts).

    The tensors are those of ``match_records``.  Returns the device tensors ``(verdict [P] u8, rmsd [P, 2] f64, count [P] i32, nodes [P] i32,
    found [P] i32, map [P, 2, 29] i32)``, enqueued on the current stream without synchronising: verdict ``RMSD_DIFFERENT`` (0: no isomorphism,
    proven), ``RMSD_DECIDED`` (1: ``rmsd[:, 0]`` / ``rmsd[:, 1]`` are the minima of the proper / improper fit over every isomorphism and ``map``
    holds the two isomorphisms that attain them), ``RMSD_UNDECIDED`` (2: the search needed more than ``max_nodes`` tries) or ``RMSD_INVALID`` (3);
    for every verdict but 1 ``rmsd`` is NaN and ``map`` -1.  ``count`` = selected atoms of the generated molecule, ``found`` = isomorphisms met.
    An exact copy scores around 1e-7, not 0 (the trace formula).  The arguments are checked, never converted."""
    return _record_call("best_rmsd_records", [(prb_rec, prb_n), (ref_rec, ref_n)], ref_index,
                        [_node_budget(max_nodes, GRAPH_MAX_NODES), _rmsd_atoms(atoms)],
                        [(torch.uint8, ()), (torch.float64, (2,)), (torch.int32, ()), (torch.int32, ()), (torch.int32, ()), (torch.int32, (2, MAX_ATOMS))],
                        prefix="dsr_")


# ----------------------------------------------------------------------------------------- engine

class DmtEngine:
    """Owns packed weights on one GPU and runs the C-ABI stages."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DmtEngine needs a HIP device (torch device type 'cuda'); there is no CPU path")
        self.lib = load_library()
        self.cfg = config
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        flat, offsets = pack_dmt_weights(sd)
        self.wflat = flat.to(self.device)
        self.woff = torch.tensor(offsets, dtype=torch.int64, device=self.device)
        self.w = DsWeights(base=self.wflat.data_ptr(), off_dev=self.woff.data_ptr(),
                           off=(C.c_int64 * W_NUM_SLOTS)(*offsets), edge_th=float(config.model.edge_quan_th),
                           spatial_cut_off=float(config.model.spatial_cut_off))
        from .spec_engine import SpecEngine
        self.spec = SpecEngine(sd, config, self.device, self.lib)
        self._layouts: Dict[tuple, tuple] = {}

    # layout/workspace cache: keyed on the mask's bytes (cheap: B*N bytes) so equal structures share tables
    def layout_for(self, node_mask: torch.Tensor, edge_mask: Optional[torch.Tensor] = None, validate: bool = False):
        last = getattr(self, "_last_layout", None)
        # the same mask TENSOR again (object identity + version; the cache keeps the tensor alive, so its address cannot be
        # re-issued to another mask while it is the key): no device->host copy
        if last is not None and last[0] is node_mask and last[1] == node_mask._version and last[2] in self._layouts:
            hit = self._layouts[last[2]]
            if validate and edge_mask is not None:
                hit[0].check_edge_mask(edge_mask)
            return hit
        key_t = (node_mask.detach().reshape(node_mask.shape[0], -1) != 0).to("cpu")
        key = (tuple(key_t.shape), key_t.numpy().tobytes())
        self._last_layout = (node_mask, node_mask._version, key)
        hit = self._layouts.get(key)
        if hit is None:
            L = Layout(node_mask, self.device)
            if len(self._layouts) >= 4:
                self._layouts.pop(next(iter(self._layouts)))
            hit = (L, Workspace(L, self.device))
            self._layouts[key] = hit
        if validate and edge_mask is not None:
            hit[0].check_edge_mask(edge_mask)
        return hit

    def context_embedding(self, context) -> Optional[torch.Tensor]:
        """cond_lin(SpecFormer(context)) [B,1024] (dmt.py:348-350)."""
        if context is None:
            return None
        return self.spec.encode(context)

    def forward(self, L: Layout, ws: Workspace, xh, edge_x, noise_level, cond_x, cond_edge_x, ctx_emb,
                out_xh=None, out_edge=None, uniform_noise_level: bool = False):
        """``uniform_noise_level``: the caller guarantees that all ``B`` noise levels are equal (a sampler's are: one noise level per
        step), so the time MLP runs once on ``noise_level[0]`` instead of on ``B`` identical rows (``ds_forward_uniform``); same bits."""
        dev = self.device
        xh, edge_x, noise_level = _f32c(xh, dev), _f32c(edge_x, dev), _f32c(noise_level, dev)
        cond_x = None if cond_x is None else _f32c(cond_x, dev)
        cond_edge_x = None if cond_edge_x is None else _f32c(cond_edge_x, dev)
        ctx_emb = None if ctx_emb is None else _f32c(ctx_emb, dev)
        if out_xh is None:
            out_xh = torch.empty(L.B, L.N, 9, dtype=torch.float32, device=dev)
        if out_edge is None:
            out_edge = torch.empty(L.B, L.N, L.N, 2, dtype=torch.float32, device=dev)
        entry = self.lib.ds_forward_uniform if uniform_noise_level else self.lib.ds_forward
        st = entry(C.byref(self.w), C.byref(L.c), C.byref(ws.c), ptr(xh), ptr(edge_x), ptr(cond_x), ptr(cond_edge_x),
                   ptr(noise_level), ptr(ctx_emb), ptr(out_xh), ptr(out_edge), _stream())
        _check(st, "ds_forward_uniform" if uniform_noise_level else "ds_forward")
        return out_xh, out_edge

    # stage-level calls for the parity tests
    def stage_time(self, L, ws, noise_level, ctx_emb):
        _check(self.lib.ds_stage_time(C.byref(self.w), C.byref(L.c), C.byref(ws.c), ptr(noise_level), ptr(ctx_emb),
                                      _stream()), "ds_stage_time")

    def stage_time_uniform(self, L, ws, noise_level, ctx_emb):
        _check(self.lib.ds_stage_time_uniform(C.byref(self.w), C.byref(L.c), C.byref(ws.c), ptr(noise_level), ptr(ctx_emb),
                                              _stream()), "ds_stage_time_uniform")

    def stage_init(self, L, ws, xh, edge_x, cond_x, cond_edge_x):
        _check(self.lib.ds_stage_init(C.byref(self.w), C.byref(L.c), C.byref(ws.c), ptr(xh), ptr(edge_x),
                                      ptr(cond_x), ptr(cond_edge_x), _stream()), "ds_stage_init")

    def stage_block(self, L, ws, blk, last=False):
        _check(self.lib.ds_stage_block(C.byref(self.w), C.byref(L.c), C.byref(ws.c), blk, int(last),
                                       _stream()), "ds_stage_block")

    def stage_readout(self, L, ws, out_xh, out_edge):
        _check(self.lib.ds_stage_readout(C.byref(self.w), C.byref(L.c), C.byref(ws.c), ptr(out_xh), ptr(out_edge),
                                         _stream()), "ds_stage_readout")

    def sampler_step(self, L, c_x, c_pred, sigma, temperature, x, edge_x, pred, edge_pred, raw_pos, raw_feat, raw_edge,
                     x_mean, edge_mean):
        st = self.lib.ds_sampler_step(C.byref(L.c), c_x, c_pred, sigma, temperature, ptr(x), ptr(edge_x), ptr(pred), ptr(edge_pred),
                                      ptr(raw_pos), ptr(raw_feat), ptr(raw_edge), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_sampler_step")

    def initial_noise_philox(self, L, seed: int, mol_id: torch.Tensor):
        """z_T, edge_z_T of sampling.py:442-447 from the per-molecule Philox streams (``ds_initial_noise``)."""
        dev = self.device
        x = torch.empty(L.B, L.N, 9, dtype=torch.float32, device=dev)
        edge_x = torch.empty(L.B, L.N, L.N, 2, dtype=torch.float32, device=dev)
        _check(self.lib.ds_initial_noise(C.byref(L.c), seed, ptr(mol_id), ptr(x), ptr(edge_x), _stream()),
               "ds_initial_noise")
        return x, edge_x

    def sampler_step_philox(self, L, c_x, c_pred, sigma, temperature, seed: int, step: int, mol_id, x, edge_x, pred, edge_pred,
                            x_mean, edge_mean):
        st = self.lib.ds_sampler_step_philox(C.byref(L.c), c_x, c_pred, sigma, temperature, seed, step, ptr(mol_id), ptr(x),
                                             ptr(edge_x), ptr(pred), ptr(edge_pred), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_sampler_step_philox")

    def step_begin(self, table, n_steps: int, step_dev, B: int, noise_level):
        _check(self.lib.ds_step_begin(ptr(table), n_steps, ptr(step_dev), B, ptr(noise_level), _stream()),
               "ds_step_begin")

    def sampler_step_philox_dev(self, L, table, step_dev, temperature, seed: int, mol_id, x, edge_x, pred, edge_pred, x_mean,
                                edge_mean):
        st = self.lib.ds_sampler_step_philox_dev(C.byref(L.c), ptr(table), ptr(step_dev), temperature, seed, ptr(mol_id), ptr(x),
                                                 ptr(edge_x), ptr(pred), ptr(edge_pred), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_sampler_step_philox_dev")

    # multistep solver update (include/diffspectra_solver.h): row (a, b, c, d); hist / edge_hist may be None when c == 0, raw_* when d == 0
    def solver_step(self, L, a, b, c, d, temperature, x, edge_x, pred, edge_pred, hist, edge_hist, raw_pos, raw_feat, raw_edge,
                    x_mean, edge_mean):
        st = self.lib.ds_solver_step(C.byref(L.c), a, b, c, d, temperature, ptr(x), ptr(edge_x), ptr(pred), ptr(edge_pred), ptr(hist),
                                     ptr(edge_hist), ptr(raw_pos), ptr(raw_feat), ptr(raw_edge), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_solver_step")

    def solver_step_philox(self, L, a, b, c, d, temperature, seed: int, step: int, mol_id, x, edge_x, pred, edge_pred, hist, edge_hist,
                           x_mean, edge_mean):
        st = self.lib.ds_solver_step_philox(C.byref(L.c), a, b, c, d, temperature, seed, step, ptr(mol_id), ptr(x), ptr(edge_x), ptr(pred),
                                            ptr(edge_pred), ptr(hist), ptr(edge_hist), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_solver_step_philox")

    def solver_step_begin(self, table, n_steps: int, step_dev, B: int, noise_level):
        _check(self.lib.ds_solver_step_begin(ptr(table), n_steps, ptr(step_dev), B, ptr(noise_level), _stream()),
               "ds_solver_step_begin")

    def solver_step_philox_dev(self, L, table, step_dev, temperature, seed: int, mol_id, x, edge_x, pred, edge_pred, hist, edge_hist,
                               x_mean, edge_mean):
        st = self.lib.ds_solver_step_philox_dev(C.byref(L.c), ptr(table), ptr(step_dev), temperature, seed, ptr(mol_id), ptr(x), ptr(edge_x),
                                                ptr(pred), ptr(edge_pred), ptr(hist), ptr(edge_hist), ptr(x_mean), ptr(edge_mean), _stream())
        _check(st, "ds_solver_step_philox_dev")

    def check_stability(self, L, pos, atom_type, want_orders: bool = True):
        """``ds_check_stability`` on the tensors ``post_process`` left on the GPU: (mol_stable [B] bool, nr_stable [B],
        n_atoms [B], bond_order [B,N,N] int64 or None)."""
        dev = self.device
        pos = _f32c(pos, dev)
        at = atom_type.detach().to(device=dev, dtype=torch.int32).contiguous()
        order = torch.empty(L.B, L.N, L.N, dtype=torch.int32, device=dev) if want_orders else None
        nr = torch.empty(L.B, dtype=torch.int32, device=dev)
        ok = torch.empty(L.B, dtype=torch.int32, device=dev)
        _check(self.lib.ds_check_stability(C.byref(L.c), ptr(pos), ptr(at), ptr(order), ptr(nr), ptr(ok), _stream()),
               "ds_check_stability")
        n_atoms = torch.as_tensor(L.n_atoms, device=dev)
        return ok.bool(), nr.long(), n_atoms, (order.long() if want_orders else None)

    def match_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_distance: float = 5.0, min_atoms: int = 3):
        """``engine.match_records`` on this engine's library (the structure metric needs no weights)."""
        return match_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, max_distance, min_atoms)

    def graph_identity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes: int = 4096):
        """``engine.graph_identity_records`` on this engine's library (graph identity needs no weights)."""
        return graph_identity_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, max_nodes)

    def graph_hash_records(self, rec, n):
        """``engine.graph_hash_records`` on this engine's library."""
        return graph_hash_records(rec, n)

    def mces_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, drop_h: bool = True, max_nodes: int = 1 << 18):
        """``engine.mces_records`` on this engine's library (the MCES distance needs no weights)."""
        return mces_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, drop_h, max_nodes)

    def morgan_records(self, rec, n, drop_h: bool = True, radius: int = 2):
        """``engine.morgan_records`` on this engine's library."""
        return morgan_records(rec, n, drop_h, radius)

    def morgan_similarity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, drop_h: bool = True, radius: int = 2, n_bits: int = 2048):
        """``engine.morgan_similarity_records`` on this engine's library (the fingerprints need no weights)."""
        return morgan_similarity_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, drop_h, radius, n_bits)

    def geometry_count_records(self, rec, n, bond_cls, angle_cls, dihedral_cls):
        """``engine.geometry_count_records`` on this engine's library."""
        return geometry_count_records(rec, n, bond_cls, angle_cls, dihedral_cls)

    def geometry_fill_records(self, rec, n, bond_cls, angle_cls, dihedral_cls, offsets, totals):
        """``engine.geometry_fill_records`` on this engine's library."""
        return geometry_fill_records(rec, n, bond_cls, angle_cls, dihedral_cls, offsets, totals)

    def mmd_1d_segments(self, x, x_off, y, y_off, kernel_mul: float = 2.0, kernel_num: int = 5, fix_sigma=None, workspace=None):
        """``engine.mmd_1d_segments`` on this engine's library (the MMD needs no weights)."""
        return mmd_1d_segments(x, x_off, y, y_off, kernel_mul, kernel_num, fix_sigma, workspace)

    def fold_bits(self, ids, count, n_bits: int = 1024):
        """``engine.fold_bits`` on this engine's library."""
        return fold_bits(ids, count, n_bits)

    def tanimoto_nn_workspace_bytes(self, Na: int, Nb: int) -> int:
        """``engine.tanimoto_nn_workspace_bytes`` on this engine's library."""
        return tanimoto_nn_workspace_bytes(Na, Nb)

    def tanimoto_nn(self, a_words, a_pop, b_words, b_pop, n_bits: int, skip_same_index: bool = False, workspace=None):
        """``engine.tanimoto_nn`` on this engine's library (the set similarities need no weights)."""
        return tanimoto_nn(a_words, a_pop, b_words, b_pop, n_bits, skip_same_index, workspace)

    def valence_records(self, rec, n, bonds_from: int = 0):
        """``engine.valence_records`` on this engine's library (the valence analytics need no weights)."""
        return valence_records(rec, n, bonds_from)

    def fragment_records(self, rec, n, keep, bonds_from: int = 0, charge_rule: bool = True):
        """``engine.fragment_records`` on this engine's library."""
        return fragment_records(rec, n, keep, bonds_from, charge_rule)

    def group_records(self, rec, n):
        """``engine.group_records`` on this engine's library (the functional groups need no weights)."""
        return group_records(rec, n)

    def group_similarity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None):
        """``engine.group_similarity_records`` on this engine's library."""
        return group_similarity_records(prb_rec, prb_n, ref_rec, ref_n, ref_index)

    def scaffold_masks(self, rec, n):
        """``engine.scaffold_masks`` on this engine's library (the scaffolds need no weights)."""
        return scaffold_masks(rec, n)

    def brics_records(self, rec, n):
        """``engine.brics_records`` on this engine's library (the BRICS analysis needs no weights)."""
        return brics_records(rec, n)

    def brics_fragment_records(self, rec, n, first, rows: int, aromatic: bool = True):
        """``engine.brics_fragment_records`` on this engine's library."""
        return brics_fragment_records(rec, n, first, rows, aromatic)

    def fraggle_fragmentations(self, rec, n, max_nodes=None):
        """``engine.fraggle_fragmentations`` on this engine's library (the Fraggle analysis needs no weights)."""
        return fraggle_fragmentations(rec, n, max_nodes)

    def path_fingerprints(self, rec, n, max_nodes=None):
        """``engine.path_fingerprints`` on this engine's library."""
        return path_fingerprints(rec, n, max_nodes)

    def fraggle_similarity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes=None):
        """``engine.fraggle_similarity_records`` on this engine's library."""
        return fraggle_similarity_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, max_nodes)

    def mobile_records(self, rec, n, max_nodes: Optional[int] = None):
        """``engine.mobile_records`` on this engine's library (the mobile-hydrogen analysis needs no weights)."""
        return mobile_records(rec, n, max_nodes)

    def normal_records(self, rec, n, max_nodes: Optional[int] = None):
        """``engine.normal_records`` on this engine's library."""
        return normal_records(rec, n, max_nodes)

    def key_sites(self, rec, n, max_nodes: Optional[int] = None, min_volume=None, min_planarity=None):
        """``engine.key_sites`` on this engine's library (the perception needs no weights)."""
        return key_sites(rec, n, max_nodes, min_volume, min_planarity)

    def key_identity_records(self, prb_rec, prb_n, prb_site, ref_rec, ref_n, ref_site, ref_index=None, max_nodes: int = 4096,
                             exhaustive: bool = False):
        """``engine.key_identity_records`` on this engine's library (the comparison needs no weights)."""
        return key_identity_records(prb_rec, prb_n, prb_site, ref_rec, ref_n, ref_site, ref_index, max_nodes, exhaustive)

    def smiles_records(self, rec, n, max_nodes: int = 4096):
        """``engine.smiles_records`` on this engine's library (the strings need no weights)."""
        return smiles_records(rec, n, max_nodes)

    def read_smiles(self, text, length, max_nodes: int = 4096):
        """``engine.read_smiles`` on this engine's library (the reader needs no weights)."""
        return read_smiles(text, length, max_nodes)

    def substructure_records(self, rec, n, patterns, max_nodes: int = SUBSTRUCTURE_DEFAULT_NODES):
        """``engine.substructure_records`` on this engine's library (the matcher needs no weights)."""
        return substructure_records(rec, n, patterns, max_nodes)

    def stereo_identity_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes: int = 4096, min_volume=None,
                                min_planarity=None, exhaustive: bool = False):
        """``engine.stereo_identity_records`` on this engine's library (the comparison needs no weights)."""
        return stereo_identity_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, max_nodes, min_volume, min_planarity, exhaustive)

    def best_rmsd_records(self, prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes: int = 4096, atoms="heavy"):
        """``engine.best_rmsd_records`` on this engine's library (the fit needs no weights)."""
        return best_rmsd_records(prb_rec, prb_n, ref_rec, ref_n, ref_index, max_nodes, atoms)

    def stereo_sites(self, rec, n, min_volume=None, min_planarity=None):
        """``engine.stereo_sites`` on this engine's library (the perception needs no weights)."""
        return stereo_sites(rec, n, min_volume, min_planarity)

    def post_process(self, L, xh, edge_x):
        dev = self.device
        pos = torch.empty(L.B, L.N, 3, dtype=torch.float32, device=dev)
        atom = torch.empty(L.B, L.N, dtype=torch.int32, device=dev)
        fc = torch.empty(L.B, L.N, dtype=torch.int32, device=dev)
        et = torch.empty(L.B, L.N, L.N, dtype=torch.float32, device=dev)
        st = self.lib.ds_post_process(C.byref(L.c), ptr(_f32c(xh, dev)), ptr(_f32c(edge_x, dev)), ptr(pos), ptr(atom),
                                      ptr(fc), ptr(et), _stream())
        _check(st, "ds_post_process")
        return pos, atom, fc, et


def gemm(lib, A, lda, Wp, bias, Cout, ldc, M, K, N, act=0, R=None, ldr=0, r_grp_rows=0, col_scale=None, col_shift=None,
         a_silu=0, a_grp=(0, 0), c_grp=(0, 0)):
    """Raw ds_gemm call; A / Wp / C etc. are tensors or integer device addresses."""
    addr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    args = DsGemmArgs(A=addr(A), lda=lda, a_grp_rows=a_grp[0], _p0=0, a_grp_stride=a_grp[1], Wp=addr(Wp), bias=addr(bias),
                      C=addr(Cout), ldc=ldc, c_grp_rows=c_grp[0], _p1=0, c_grp_stride=c_grp[1], M=M, K=K, N=N, act=act,
                      R=addr(R), ldr=ldr, r_grp_rows=r_grp_rows, a_silu=a_silu, col_scale=addr(col_scale),
                      col_shift=addr(col_shift))
    _check(lib.ds_gemm(C.byref(args), _stream()), "ds_gemm")
