"""Float64 yardstick of the sampling block kernels (csrc/ds_forward.hip; buffers: ``ds_workspace`` in include/diffspectra_hip.h), plain
torch / numpy on the CPU.  TEST INFRASTRUCTURE ONLY; pinned without a GPU by tests/test_block_mirror_cpu.py, used by
tests/test_block_stages_gpu.py.

It restates ``oracle/dmt.py`` (``dmt_forward`` init and readout, ``_mix_block``, ``_trans_mix``, ``_equi_update``) in the packed layout of
the kernels, NOT the kernels: node rows ``[Nn]`` molecule-major, pair rows ``[Pp]`` = the pairs a < b of every molecule (a-major), direction 0 =
source / row a -> target / column b, direction 1 = b -> a.  Like ``chain_mirror`` it keeps plain layout numbers (256, 64, 252 = 14 x 18, the adaLN
column offsets) on purpose: they are the contract under test.

STAGE-WISE USE.  One function per stage, every input explicit, so a caller feeds either the mirror's own previous outputs (``forward``: the
free run that tests/test_block_mirror_cpu.py holds to the fp64 oracle) or tensors read back from the GPU (teacher forcing: both sides then
start from the same fp32 values and one stage's arithmetic separates them).  A stage returns ``{name: Ref(ref, bound, tol, mol)}``: the
float64 value of a workspace buffer, the per-element bound carried from the matrix products in front of it, and the ``relerr`` figure of what
lies behind the last product.  ``allowance`` turns that into the per-element limit ``bound + tol * max |ref| over the rows of the molecule``.

ARITHMETIC PER PRODUCT (read from the kernels: ``*_H`` / ``*_C`` weight slots are split-fp16, plain ``*_W`` slots the fp32 path):
  init        node_emb 12 -> 256 fp32 VALU; edge_emb 68 -> 64 fp32 MFMA (DS_GW_*_W)
  edge_geom   edge_emb 128 -> 64 split (EDGE_EMB_H)
  node_qkv    q|k|v 256 -> 768 split (QKV_H)
  attention   lin_edge0 / lin_edge1 64 -> 256 split (E0_H / E1_H, weights times 2 log2 e: one more fp32 rounding of every weight, counted
              as 2^-24 |A||W|); the 18-wide logit sums and the <= 28-source aggregation are fp32 VALU
  node_update node2edge 256 -> 64, ff_linear1 256 -> 512, ff_linear2 512 -> 256, node_i 256 -> 64, input_lin node parts 256 -> 512: all split
  edge_update ff_linear3 64 -> 128 split (FF3_H), ff_linear4 128 -> 64 split in accumulator-chain order (FF4_C), edge_i 64 -> 16 fp32 MFMA
              (EDGE_RO_W), input_lin edge | dist part 128 -> 256 split (ED_H)
  equi_pairs  coord_mlp.0 256 -> 256 split (CM0_H); coord_mlp.2 256 -> 3 fp32 VALU (CM2_W)
  readout     node_pred_mlp.0 768 -> 256 and .2 256 -> 128 split (NP0_H, NP2_H), .4 128 -> 6 fp32; edge_*_mlp.0 192 -> 64 split (EX0_H / ET0_H),
              .2 64 -> 32 split chain (EX2_C / ET2_C), .4 32 -> 1 fp32 VALU

BOUNDS.  fp32 path: ``chain_mirror.product_bound``, 2 (K + 2) 2^-24 (|A||W|^T + |bias|) - twice the worst case of K + 2 fp32 additions in any
order.  Split-fp16 (``split_bound``): every operand travels as a = a1 + a2 / 2048, a1 = fp16(a), a2 = fp16((a - a1) 2048), both round to
nearest.  a - a1 is exact in fp32 and at most 2^-11 |a|; rounding it to fp16's 11 significant bits leaves |a - a1 - a2/2048| <= 2^-22 |a| while
(a - a1) 2048 is a NORMAL fp16 number; below that (|a - a1| 2048 < 2^-14) the absolute error is at most half a subnormal step, 2^-25 / 2048
= 2^-36 - the subnormal floor, kept as its own term 2^-36 (sum_k |a_k| + sum_k |w_k|).  The kernel sums a1 w1 + (a1 w2 + a2 w1) / 2048 (three
f16 MFMAs per k-block; every fp16 x fp16 product is exact in fp32), so against the exact product it lacks
  eps_a w + a eps_w  <= 2 * 2^-22 |a||w|      the two representation errors
  a2 w2 / 2048^2     <= 2^-22 (1 + 2^-10) |a||w|   the dropped term (|a2| / 2048 <= 2^-11 (1 + 2^-11) |a|)
and adds the fp32 accumulation of 3 K products: K of them (+ bias) in the high accumulator, 2 K of relative size 2^-11 (1 + 2^-11) in the low one,
one fused multiply-add joins them.  With the same factor two as the fp32 path:
  bound = [2 (K + 2) 2^-24 + 2 (2 K + 2) 2^-24 2^-10 + 3 * 2^-22 (1 + 2^-9)] |A||W|^T + 2 (K + 2) 2^-24 |bias| + floor.
The constant is pinned by the numpy emulation of tests/test_block_mirror_cpu.py (both planes rounded, the three-product form, fp32
accumulation in a shuffled order), never by a GPU measurement.

CARRYING.  A product whose result the kernel does not write out hands its bound to what follows: ``dA |W|^T`` is added to the next product's
bound; SiLU has Lipschitz constant < 1.1 and tanh 1; the LayerNorm is carried to first order (``ln_carry``: |d yhat| <= (|dy| + mean |dy| +
|yhat| mean(|yhat||dy|)) / sigma), then times |1 + scale|; a gate multiplies by |gate|; the 18-wide logit sum carries sum |q k| d(tanh) / 4
plus its own fp32 sum 2 (18 + 2) 2^-24 sum |q k tanh| / 4; the softmax weights are held to 2 max d(logit) + 3e-6 absolute (the max over the
sources of the target and head: |d softmax| <= 2 max |d logit| for any logit shift); coord_mlp.0 -> SiLU -> coord_mlp.2 -> tanh -> mean over
the (1 + adjacency bits) heads / 3 carries through both products, 1.1, 1 and the mean.  Every epilogue behind a product (gate / residual 2e-6,
modulated LayerNorm 3e-6, Gaussian features / x' 3e-6, SiLU / tanh / exp 3e-6: ``TOL`` of tests/test_train_chain_kernels.py) adds its figure
times the tensor's largest magnitude over the molecule, to the carried input error where the tensor feeds a product and to ``tol`` where it is
the stage's output."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from tests.chain_mirror import U, PI, LN_EPS, tables  # noqa: F401  (tables: the packed-ragged index tables, re-exported)

T_GATE, T_LN, T_RBF, T_ACT = 2e-6, 3e-6, 3e-6, 3e-6       # tests/test_train_chain_kernels.py TOL: gate / residual, modulated LN, features, epilogues
ADA_STRIDE, ADA_NODE, ADA_EDGE, ADA_EQUI, ADA_DIST, ADA_TOP = 2464, 0, 1536, 1920, 2432, 8 * 2464
ADA_COLS = ADA_TOP + 32
NB = 8
SPLIT = 2048.0
F16_FLOOR = 2.0 ** -36
TANH_PRESCALE = 2.8853900817779268

Ref = namedtuple("Ref", "ref bound tol mol")          # mol: molecule of every row (None: one group)


def dbl(x):
    return torch.as_tensor(x).detach().double().cpu()


# ------------------------------------------------------------------------------------------------ inputs of the stage tests
# the smallest layouts that reach every tile edge (32 | 64 | 128-row tiles, 32-row attention chunks, pairless molecules); (Nn, Pp) in COUNTS
LAYOUTS = {"ragged": [3, 1, 9, 2, 12, 1, 4, 15], "big": [29, 28, 29], "single": [1], "one_pair": [2]}
COUNTS = {"ragged": (47, 217), "big": (86, 1190), "single": (1, 0), "one_pair": (2, 1)}
CLEARED = {"ragged": [(2, 4), (7, 0)], "big": [(0, 5), (1, 27)]}      # (molecule, atom) whose incoming cond_adj_2d bits are all made 0


def stage_inputs(layout, first, version="ir", n_atoms=None):
    """``cases.forward_inputs`` of a layout.  The procedural general-step inputs have no atom all of whose neighbours lie below the bond
    threshold, so for the atoms of ``CLEARED`` channel 0 of ``cond_edge_x`` is set to -1 towards every neighbour (symmetrically): all extra-head
    logits of such a target are -1e10 and its softmax is uniform, 1 / (n - 1)."""
    from tests.golden import cases
    a = cases.forward_inputs(version, first, n_atoms=n_atoms or LAYOUTS[layout])
    if not first:
        ce = a["cond_edge_x"].clone()
        for m, i in CLEARED.get(layout, []):
            ce[m, i, :, 0] = -1.0
            ce[m, :, i, 0] = -1.0
        a["cond_edge_x"] = ce * (a["edge_mask"].reshape(ce.shape[:3] + (1,)) != 0)
    return a


def adjacency_patterns(n_atoms, adj):
    """Per target atom: (all incoming bit-0 clear, bit 0 mixed, bit 1 mixed) over the atoms with at least two incoming edges."""
    tb = tables(n_atoms)
    adj = torch.as_tensor(adj).long()
    tgt = torch.cat([tb["pair_b"], tb["pair_a"]])
    bits = torch.cat([adj, adj])
    cnt = torch.zeros(tb["Nn"]).index_add_(0, tgt, torch.ones(len(tgt)))
    s0 = torch.zeros(tb["Nn"]).index_add_(0, tgt, (bits & 1).float())
    s1 = torch.zeros(tb["Nn"]).index_add_(0, tgt, ((bits >> 1) & 1).float())
    many = cnt >= 2
    return bool((many & (s0 == 0)).any()), bool((many & (s0 > 0) & (s0 < cnt)).any()), bool((many & (s1 > 0) & (s1 < cnt)).any())


# ------------------------------------------------------------------------------------------------ bounds
def fp32_bound(A, W, bias=None, dA=None):
    """``chain_mirror.product_bound`` on fp32 operands (nothing is rounded to bf16 here) plus the carried input error ``dA |W|^T``."""
    A, W = dbl(A), dbl(W)
    m = A.abs() @ W.abs().T
    if bias is not None:
        m = m + dbl(bias).abs()
    b = 2.0 * (A.shape[1] + 2) * U * m
    return b if dA is None else b + dbl(dA) @ W.abs().T


def split_bound(A, W, bias=None, dA=None, prescaled=False):
    """The split-fp16 product bound of the module docstring, per element of ``A W^T + bias``."""
    A, W = dbl(A), dbl(W)
    K = A.shape[1]
    m = A.abs() @ W.abs().T
    rel = 2.0 * (K + 2) * U + 2.0 * (2 * K + 2) * U * 2.0 ** -10 + 3.0 * 2.0 ** -22 * (1.0 + 2.0 ** -9) + (U if prescaled else 0.0)
    b = rel * m + F16_FLOOR * (A.abs().sum(1, keepdim=True) + W.abs().sum(1)[None, :])
    if bias is not None:
        b = b + 2.0 * (K + 2) * U * dbl(bias).abs()
    return b if dA is None else b + dbl(dA) @ W.abs().T


def molmax(t, mol):
    """max |t| over all rows of the row's molecule (and all columns), as a column."""
    if t.shape[0] == 0:
        return torch.zeros(0, 1, dtype=torch.float64)
    t = dbl(t).abs().reshape(t.shape[0], -1)
    r = t.max(1).values
    if mol is None:
        return r.max().expand(t.shape[0]).reshape(-1, 1)
    B = int(mol.max()) + 1
    mx = torch.zeros(B, dtype=torch.float64).scatter_reduce(0, mol, r, "amax", include_self=True)
    return mx[mol].reshape(-1, 1)


def allowance(r: Ref):
    """Per-element limit of |got - ref|: the carried product bound + the ``relerr`` figure times the molecule's largest |ref|."""
    a = r.bound + r.tol * molmax(r.ref, r.mol).reshape([-1] + [1] * (r.ref.dim() - 1))
    return a


def ln(x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS)


def ln_carry(x, dx):
    """First-order |d LayerNorm(x)| for an input error of at most ``dx`` per element."""
    mu = x.mean(-1, keepdim=True)
    sig = torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + LN_EPS)
    yh = ((x - mu) / sig).abs()
    return (dx + dx.mean(-1, keepdim=True) + yh * (yh * dx).mean(-1, keepdim=True)) / sig


def silu(x):
    return x * torch.sigmoid(x)


def lin(sd, name, x):
    y = x @ dbl(sd[name + ".weight"]).T
    b = sd.get(name + ".bias")
    return y if b is None else y + dbl(b)


def rbf_tables(sd, name):
    """means, |stds| + 1e-5 and a * std as the reference forms them: in fp32 (layers.py:291-295,332-334; engine._rbf_tables)."""
    mean = sd[name + ".means.weight"].float().view(-1)
    std = sd[name + ".stds.weight"].float().view(-1).abs() + 1e-5
    astd = (2 * PI) ** 0.5 * std
    return mean.double(), std.double(), astd.double()


def cond_gaussian(sd, name, x, scale, shift):
    """[x', 63 Gaussian features of x'] with x' = x (scale + 1) + shift (layers.py:328-334).  x, scale, shift: columns."""
    xp = x * (scale + 1.0) + shift
    return xp, torch.cat([xp, rbf_features(sd, name, xp)], 1)


def rbf_features(sd, name, xp):
    mean, std, astd = rbf_tables(sd, name)
    return torch.exp(-0.5 * ((xp - mean) / std) ** 2) / astd


def gate_mod_ff(x_in, add, gate1, shift, scale, gate2, W1, b1, W2, b2, mol, d_add=None):
    """The residual -> LayerNorm -> FF -> residual chain both row kinds share (dmt.py:159-163,165-169): r = x_in + gate1 add, x = LN(r) (1 +
    scale) + shift, out = x + gate2 (W2 SiLU(W1 x + b1) + b2), with the carried bound of ``out`` (both products split-fp16, neither written)."""
    r = x_in + gate1 * add
    dr = T_GATE * molmax(r, mol) + (0.0 if d_add is None else gate1.abs() * d_add)
    x = ln(r) * (1.0 + scale) + shift
    dx = (1.0 + scale).abs() * ln_carry(r, dr.expand_as(r)) + (T_LN + 2.0 ** -22) * molmax(x, mol)     # + the split-fp16 tile the kernel keeps x in
    f1 = x @ W1.T + b1
    d1 = split_bound(x, W1, b1, dx)
    s = silu(f1)
    ds_ = 1.1 * d1 + T_ACT * molmax(s, mol)
    f2 = s @ W2.T + b2
    d2 = split_bound(s, W2, b2, ds_)
    out = x + gate2 * f2
    return out, dx + gate2.abs() * d2


# ------------------------------------------------------------------------------------------------ adaLN table
def ada_table(sd, temb):
    """[B, ADA_COLS] in the kernels' column layout from the time embedding [B, 1024] (every ``*time_mlp`` Linear, SiLU first)."""
    s = silu(dbl(temb))
    out = torch.zeros(s.shape[0], ADA_COLS, dtype=torch.float64)
    for b in range(NB):
        base, p = b * ADA_STRIDE, f"e_block_{b}."
        for name, off in (("node_time_mlp", ADA_NODE), ("edge_time_mlp", ADA_EDGE), ("equi_update.time_mlp", ADA_EQUI), ("dist_layer.time_mlp", ADA_DIST)):
            y = lin(sd, p + name + ".1", s)
            out[:, base + off: base + off + y.shape[1]] = y
    out[:, ADA_TOP: ADA_TOP + 2] = lin(sd, "dist_layer.time_mlp.1", s)
    return out


def _node_ada(ada, blk, tb):
    a = dbl(ada)[tb["node_mol"], blk * ADA_STRIDE + ADA_NODE:][:, :1536]
    return [a[:, 256 * i: 256 * (i + 1)] for i in range(6)]       # shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp


def _edge_ada(ada, blk, tb):
    a = dbl(ada)[tb["pair_mol"], blk * ADA_STRIDE + ADA_EDGE:][:, :384]
    return [a[:, 64 * i: 64 * (i + 1)] for i in range(6)]


# ------------------------------------------------------------------------------------------------ stages
def dense_tables(tb, N):
    """Dense rows b * N + i of the packed nodes (prefix masks) and (molecule, local a, local b) of the packed pairs."""
    nm = tb["node_mol"]
    local = torch.arange(tb["Nn"]) - torch.as_tensor(tb["node_off"])[nm]
    pm = tb["pair_mol"]
    off = torch.as_tensor(tb["node_off"])[pm] if tb["Pp"] else pm
    return nm * N + local, pm, tb["pair_a"] - off, tb["pair_b"] - off


def init(sd, cfg, tb, xh, edge_x, cond_x, cond_edge_x, ada):
    """dmt.py:323-345,363-377: pos, h = node_emb, e = edge_emb, the adjacency bits and the 'any non-zero conditioning distance' flag."""
    N = xh.shape[1]
    nd, pm, la, lb = dense_tables(tb, N)
    xf = dbl(xh).reshape(-1, 9)[nd]
    first = cond_x is None
    cf = torch.zeros_like(xf) if first else dbl(cond_x).reshape(-1, 9)[nd]
    hin = torch.cat([xf[:, 3:], cf[:, 3:]], 1)
    Wn, bn = dbl(sd["node_emb.weight"]), dbl(sd["node_emb.bias"])
    h = hin @ Wn.T + bn
    ex = dbl(edge_x)[pm, la, lb]
    mol_p = tb["pair_mol"]
    if first:
        ce = torch.zeros_like(ex)
        adj = torch.full((tb["Pp"],), 3, dtype=torch.int32)
        feat, dfeat, flag = torch.zeros(tb["Pp"], 64, dtype=torch.float64), None, 0
    else:
        ce = dbl(cond_edge_x)[pm, la, lb]
        cp32 = cond_x.float().reshape(-1, 9)[nd][:, :3]                               # the two comparisons are made on fp32 values (dmt.py:338-340, utils.py:118-126)
        d32 = ((cp32[tb["pair_a"]] - cp32[tb["pair_b"]]) ** 2).sum(1)
        bit0 = cond_edge_x.float()[pm, la, lb][:, 0] >= float(cfg.model.edge_quan_th)
        adj = (bit0.int() | ((d32 <= float(cfg.model.spatial_cut_off)).int() << 1)).int()
        d2 = ((cf[tb["pair_a"], :3] - cf[tb["pair_b"], :3]) ** 2).sum(1, keepdim=True)
        flag = int(bool((d32 != 0).any()))
        if flag:
            top = dbl(ada)[mol_p, ADA_TOP: ADA_TOP + 2]
            _, feat = cond_gaussian(sd, "dist_layer", d2, top[:, 0:1], top[:, 1:2])
            dfeat = T_RBF * molmax(feat, mol_p).expand_as(feat)
        else:
            feat, dfeat = d2.repeat(1, 64), None
    ein = torch.cat([ex, ce, feat], 1)
    We, be = dbl(sd["edge_emb.weight"]), dbl(sd["edge_emb.bias"])
    e = ein @ We.T + be
    dein = None if dfeat is None else torch.cat([torch.zeros(tb["Pp"], 4, dtype=torch.float64), dfeat], 1)
    return dict(pos=Ref(xf[:, :3], torch.zeros(tb["Nn"], 3, dtype=torch.float64), 0.0, tb["node_mol"]),
                h=Ref(h, fp32_bound(hin, Wn, bn), 0.0, tb["node_mol"]),
                e=Ref(e, fp32_bound(ein, We, be, dein), 0.0, mol_p)), adj, flag


def edge_geom(sd, blk, tb, pos, e_in, ada):
    """dmt.py:136-139,145-149: x' (``dist``) and the LayerNorm'd, modulated edge features ``ye``."""
    p = f"e_block_{blk}."
    pos, e_in, mol = dbl(pos)[:, :3], dbl(e_in), tb["pair_mol"]
    d2 = ((pos[tb["pair_a"]] - pos[tb["pair_b"]]) ** 2).sum(1, keepdim=True)
    ds = dbl(ada)[mol, blk * ADA_STRIDE + ADA_DIST:][:, :2]
    xp, feat = cond_gaussian(sd, p + "dist_layer", d2, ds[:, 0:1], ds[:, 1:2])
    W, b = dbl(sd[p + "edge_emb.weight"]), dbl(sd[p + "edge_emb.bias"])
    xin = torch.cat([feat, e_in], 1)
    y = xin @ W.T + b
    dfeat = T_RBF * molmax(feat, mol).expand_as(feat)
    dy = split_bound(xin, W, b, torch.cat([dfeat, torch.zeros_like(e_in)], 1))
    sh, sc = _edge_ada(ada, blk, tb)[:2]
    ye = ln(y) * (1.0 + sc) + sh
    z = torch.zeros_like(xp)
    return dict(dist=Ref(xp, z, T_RBF, mol), ye=Ref(ye, (1.0 + sc).abs() * ln_carry(y, dy) + 2.0 ** -22 * ye.abs(), T_LN, mol)), feat


def node_qkv(sd, blk, tb, h, ada):
    """dmt.py:148, layers.py:147-149: q (252 of 256) | k (252 of 256) | v (256); the pad columns are zero."""
    p, mol = f"e_block_{blk}.attn_mpnn.", tb["node_mol"]
    sh, sc = _node_ada(ada, blk, tb)[:2]
    x = ln(dbl(h)) * (1.0 + sc) + sh
    dx = (T_LN + 2.0 ** -22) * molmax(x, mol).expand_as(x)
    out = torch.zeros(tb["Nn"], 768, dtype=torch.float64)
    bd = torch.zeros_like(out)
    for name, c0 in (("lin_query", 0), ("lin_key", 256), ("lin_value", 512)):
        W, b = dbl(sd[p + name + ".weight"]), dbl(sd[p + name + ".bias"])
        out[:, c0: c0 + W.shape[0]] = x @ W.T + b
        bd[:, c0: c0 + W.shape[0]] = split_bound(x, W, b, dx)
    return dict(qkv=Ref(out, bd, 0.0, mol))


def _directed(tb):
    """(source, target) node rows of the directed edge [p][dir]."""
    a, b = tb["pair_a"], tb["pair_b"]
    return torch.stack([a, b], 1), torch.stack([b, a], 1)


def _edge_tanh(sd, name, ye, mol):
    W = dbl(sd[name + ".weight"])
    pre = ye @ W.T
    t = torch.tanh(pre)
    return t, split_bound(ye, W, None, None, prescaled=True) + T_ACT


def attn_alpha(sd, blk, tb, qkv, ye, adj):
    """layers.py:165-176 + PyG softmax: the softmax weights [Pp][2][16], the two adjacency heads first."""
    p = f"e_block_{blk}.attn_mpnn."
    qkv, ye = dbl(qkv), dbl(ye)
    Pp, Nn = tb["Pp"], tb["Nn"]
    src, tgt = _directed(tb)
    q = qkv[:, :252].reshape(Nn, 14, 18)
    k = qkv[:, 256:508].reshape(Nn, 14, 18)
    te0, dte = _edge_tanh(sd, p + "lin_edge0", ye, tb["pair_mol"])
    te0, dte = te0.reshape(Pp, 1, 14, 18), dte.reshape(Pp, 1, 14, 18)
    qk = q[tgt] * k[src]                                                   # [Pp, 2, 14, 18]
    logit = (qk * te0).sum(-1) / 4.0
    dlog = ((qk.abs() * dte).sum(-1) + 2.0 * 20 * U * (qk * te0).abs().sum(-1)) / 4.0 + 2.0 * U * logit.abs()
    adj = torch.as_tensor(adj).long().cpu()
    ex = torch.stack([(adj & 1).double(), ((adj >> 1) & 1).double()], 1)
    ex = torch.where(ex == 0, torch.full_like(ex, -1e10), ex).reshape(Pp, 1, 2).expand(Pp, 2, 2)
    lg = torch.cat([ex, logit], -1)                                        # [Pp, 2, 16]
    dl = torch.cat([torch.zeros(Pp, 2, 2, dtype=torch.float64), dlog], -1)
    idx = tgt.reshape(-1, 1).expand(-1, 16)
    flat = lg.reshape(-1, 16)
    mx = torch.full((Nn, 16), -math.inf, dtype=torch.float64).scatter_reduce(0, idx, flat, "amax", include_self=True)
    ev = torch.exp(flat - mx[tgt.reshape(-1)])
    den = torch.zeros(Nn, 16, dtype=torch.float64).index_add_(0, tgt.reshape(-1), ev) + 1e-16
    alpha = (ev / den[tgt.reshape(-1)]).reshape(Pp, 2, 16)
    dmax = torch.zeros(Nn, 16, dtype=torch.float64).scatter_reduce(0, idx, dl.reshape(-1, 16), "amax", include_self=True)
    bound = (2.0 * dmax[tgt.reshape(-1)]).reshape(Pp, 2, 16) + T_ACT                 # absolute: 2 max d(logit) + 3e-6
    return dict(alpha=Ref(alpha, bound, 0.0, None))


def attn_out(sd, blk, tb, alpha, qkv, ye):
    """layers.py:178-186: attn[t] = sum over the sources of v_s tanh(lin_edge1 e) alpha."""
    p = f"e_block_{blk}.attn_mpnn."
    qkv, ye, alpha = dbl(qkv), dbl(ye), dbl(alpha).reshape(-1, 2, 16)
    Pp, Nn = tb["Pp"], tb["Nn"]
    src, tgt = _directed(tb)
    v = qkv[:, 512:].reshape(Nn, 16, 16)
    te1, dte = _edge_tanh(sd, p + "lin_edge1", ye, tb["pair_mol"])
    te1, dte = te1.reshape(Pp, 1, 16, 16), dte.reshape(Pp, 1, 16, 16)
    a = alpha.reshape(Pp, 2, 16, 1)
    msg = v[src] * te1 * a
    dmsg = v[src].abs() * a * dte + 4.0 * U * msg.abs()
    t = tgt.reshape(-1)
    out = torch.zeros(Nn, 16, 16, dtype=torch.float64).index_add_(0, t, msg.reshape(-1, 16, 16))
    mag = torch.zeros_like(out).index_add_(0, t, msg.abs().reshape(-1, 16, 16))
    bd = torch.zeros_like(out).index_add_(0, t, dmsg.reshape(-1, 16, 16)) + 2.0 * 30 * U * mag      # fp32 sum of at most 28 messages
    return dict(attn=Ref(out.reshape(Nn, 256), bd.reshape(Nn, 256), 0.0, tb["node_mol"]))


def node_u(sd, blk, tb, attn):
    W = dbl(sd[f"e_block_{blk}.node2edge_lin.weight"])
    attn = dbl(attn)
    return dict(u=Ref(attn @ W.T, split_bound(attn, W), 0.0, tb["node_mol"]))


def node_update(sd, blk, tb, h_in, attn, ada):
    """dmt.py:159-163: h_out from the block's input h and the attention output."""
    p, mol = f"e_block_{blk}.", tb["node_mol"]
    _, _, g1, sh, sc, g2 = _node_ada(ada, blk, tb)
    out, bd = gate_mod_ff(dbl(h_in), dbl(attn), g1, sh, sc, g2, dbl(sd[p + "ff_linear1.weight"]), dbl(sd[p + "ff_linear1.bias"]),
                          dbl(sd[p + "ff_linear2.weight"]), dbl(sd[p + "ff_linear2.bias"]), mol)
    return dict(h=Ref(out, bd, T_GATE, mol))


def node_tail(sd, blk, tb, h_out):
    """dmt.py:387 and the node parts of equi_update.input_lin (dmt.py:39,45): the readout slice and ``ac`` = [row part | column part]."""
    h, mol = dbl(h_out), tb["node_mol"]
    Wr, br = dbl(sd[f"node_{blk}.weight"]), dbl(sd[f"node_{blk}.bias"])
    Wac = dbl(sd[f"e_block_{blk}.equi_update.input_lin.weight"])[:, :512]
    Wac = torch.cat([Wac[:, :256], Wac[:, 256:]], 0)
    return dict(atom_hids=Ref(h @ Wr.T + br, split_bound(h, Wr, br), 0.0, mol), ac=Ref(h @ Wac.T, split_bound(h, Wac), 0.0, mol))


def edge_update(sd, blk, tb, e_in, u, ada):
    """dmt.py:156-157,165-169: e_out from the block's input e and the per-node node2edge rows ``u``."""
    p, mol = f"e_block_{blk}.", tb["pair_mol"]
    _, _, g1, sh, sc, g2 = _edge_ada(ada, blk, tb)
    u = dbl(u)
    add = (u[tb["pair_a"]] + u[tb["pair_b"]]) + dbl(sd[p + "node2edge_lin.bias"])
    out, bd = gate_mod_ff(dbl(e_in), add, g1, sh, sc, g2, dbl(sd[p + "ff_linear3.weight"]), dbl(sd[p + "ff_linear3.bias"]),
                          dbl(sd[p + "ff_linear4.weight"]), dbl(sd[p + "ff_linear4.bias"]), mol)
    return dict(e=Ref(out, bd, T_GATE, mol))


def edge_tail(sd, blk, tb, e_out, dist):
    """dmt.py:388 (fp32 path) and the edge | dist part of equi_update.input_lin + bias (``ed``), its Gaussian features recomputed from ``dist``."""
    e, xp, mol = dbl(e_out), dbl(dist).reshape(-1, 1), tb["pair_mol"]
    Wr, br = dbl(sd[f"edge_{blk}.weight"]), dbl(sd[f"edge_{blk}.bias"])
    feat = torch.cat([xp, rbf_features(sd, f"e_block_{blk}.dist_layer", xp)], 1)
    Wd = dbl(sd[f"e_block_{blk}.equi_update.input_lin.weight"])[:, 512:]
    bd_ = dbl(sd[f"e_block_{blk}.equi_update.input_lin.bias"])
    xin = torch.cat([e, feat], 1)
    dx = torch.cat([2.0 ** -22 * e.abs(), (T_RBF + 2.0 ** -22) * molmax(feat, mol).expand_as(feat)], 1)
    return dict(edge_hids=Ref(e @ Wr.T + br, fp32_bound(e, Wr, br), 0.0, mol), ed=Ref(xin @ Wd.T + bd_, split_bound(xin, Wd, bd_, dx), 0.0, mol))


def equi_pairs(sd, blk, tb, ac, ed, pos, adj, ada):
    """dmt.py:37-56: the per-edge translation ``tr`` [Pp][2][4] = unit coord_diff * coord_norm.scale * mean of the tanh heads; lane 3 is zero."""
    p = f"e_block_{blk}.equi_update."
    ac, ed, pos = dbl(ac), dbl(ed), dbl(pos)[:, :3]
    Pp = tb["Pp"]
    row, col = _directed(tb)                                              # direction 0: row a, column b
    mol2 = tb["pair_mol"].repeat_interleave(2)
    x = (ac[row.reshape(-1), :256] + ac[col.reshape(-1), 256:]) + ed.repeat_interleave(2, 0)
    dx = T_GATE * molmax(x, mol2).expand_as(x)
    eq = dbl(ada)[mol2, blk * ADA_STRIDE + ADA_EQUI:][:, :512]
    sh, sc = eq[:, :256], eq[:, 256:]
    y = ln(x) * (1.0 + sc) + sh
    dy = (1.0 + sc).abs() * ln_carry(x, dx) + (T_LN + 2.0 ** -22) * molmax(y, mol2)
    W0, b0, W2 = dbl(sd[p + "coord_mlp.0.weight"]), dbl(sd[p + "coord_mlp.0.bias"]), dbl(sd[p + "coord_mlp.2.weight"])
    f0 = y @ W0.T + b0
    s = silu(f0)
    ds_ = 1.1 * split_bound(y, W0, b0, dy) + T_ACT * molmax(s, mol2)
    f2 = s @ W2.T
    inv = torch.tanh(f2)
    dinv = fp32_bound(s, W2, None, ds_) + T_ACT
    adj = torch.as_tensor(adj).long().cpu().repeat_interleave(2)
    heads = torch.stack([torch.ones_like(adj), adj & 1, (adj >> 1) & 1], 1).double()
    w = (inv * heads).sum(1, keepdim=True) / 3.0
    dw = (dinv * heads).sum(1, keepdim=True) / 3.0 + 4.0 * U * (inv.abs() * heads).sum(1, keepdim=True) / 3.0
    d = pos[row.reshape(-1)] - pos[col.reshape(-1)]
    unit = d / d.norm(dim=1, keepdim=True).clamp(min=1e-8) * dbl(sd[p + "coord_norm.scale"])
    tr = torch.cat([unit * w, torch.zeros(2 * Pp, 1, dtype=torch.float64)], 1)
    bd = torch.cat([unit.abs() * dw + T_ACT * unit.abs() * w.abs(), torch.zeros(2 * Pp, 1, dtype=torch.float64)], 1)
    return dict(tr=Ref(tr.reshape(Pp, 2, 4), bd.reshape(Pp, 2, 4), 0.0, tb["pair_mol"]))


def pos_update(tb, pos, tr):
    """dmt.py:57-58 + the per-layer CoM removal (dmt.py:385-386): pos_r + sum_c tr(r -> c), minus the molecule's mean."""
    pos, tr = dbl(pos)[:, :3], dbl(tr).reshape(-1, 2, 4)[:, :, :3]
    row, _ = _directed(tb)
    mol, B = tb["node_mol"], tb["B"]
    agg = torch.zeros_like(pos).index_add_(0, row.reshape(-1), tr.reshape(-1, 3))
    mag = pos.abs() + torch.zeros_like(pos).index_add_(0, row.reshape(-1), tr.abs().reshape(-1, 3))
    x = pos + agg
    n = torch.zeros(B, dtype=torch.float64).index_add_(0, mol, torch.ones(tb["Nn"], dtype=torch.float64)).clamp(min=1).reshape(-1, 1)
    mean = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, mol, x) / n
    summag = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, mol, mag)
    bd = 2.0 * 32 * U * mag + (2.0 * 32 * U * summag / n)[mol] + 2.0 * 32 * U * (summag / n)[mol]     # <= 29 terms per sum, the mean's sum, the division
    return dict(pos=Ref(x - mean[mol], bd, T_GATE, mol))


def _mlp3_bound(sd, name, x, kinds, mol, dx=None):
    y, d = dbl(x), dx
    for i, kind in zip((0, 2, 4), kinds):
        W, b = dbl(sd[f"{name}.{i}.weight"]), dbl(sd[f"{name}.{i}.bias"])
        pre = y @ W.T + b
        dpre = (split_bound if kind == "split" else fp32_bound)(y, W, b, d)
        if i == 4:
            return pre, dpre
        y = silu(pre)
        d = 1.1 * dpre + (T_ACT + 2.0 ** -22) * molmax(y, mol)


def readout(sd, tb, N, atom_hids, edge_hids, pos, nan_flag=0):
    """dmt.py:391-412: out_xh [B, N, 9] (positions masked, NaN-guarded, CoM-free; node_pred_mlp) and the symmetric out_edge [B, N, N, 2]."""
    B, mol, molp = tb["B"], tb["node_mol"], tb["pair_mol"]
    nd, pm, la, lb = dense_tables(tb, N)
    ah, eh = dbl(atom_hids), dbl(edge_hids)
    np_, dnp = _mlp3_bound(sd, "node_pred_mlp", ah, ("split", "split", "fp32"), mol, 2.0 ** -22 * ah.abs())
    pos = torch.zeros(tb["Nn"], 3, dtype=torch.float64) if nan_flag else dbl(pos)[:, :3]
    n = torch.zeros(B, dtype=torch.float64).index_add_(0, mol, torch.ones(tb["Nn"], dtype=torch.float64)).clamp(min=1).reshape(-1, 1)
    sm = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, mol, pos)
    sa = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, mol, pos.abs())
    out = torch.zeros(B * N, 9, dtype=torch.float64)
    bd = torch.zeros_like(out)
    out[nd] = torch.cat([pos - (sm / n)[mol], np_], 1)
    bd[nd] = torch.cat([(2.0 * 32 * U * sa / n)[mol] + 4.0 * U * (pos.abs() + (sa / n)[mol]), dnp], 1)
    oe = torch.zeros(B, N, N, 2, dtype=torch.float64)
    be = torch.zeros_like(oe)
    for ch, name in enumerate(("edge_exist_mlp", "edge_type_mlp")):
        v, dv = _mlp3_bound(sd, name, eh, ("split", "split", "fp32"), molp, 2.0 ** -22 * eh.abs())
        oe[pm, la, lb, ch] = oe[pm, lb, la, ch] = v[:, 0]
        be[pm, la, lb, ch] = be[pm, lb, la, ch] = dv[:, 0]
    return dict(out_xh=Ref(out.reshape(B, N, 9), bd.reshape(B, N, 9), 0.0, None), out_edge=Ref(oe, be, 0.0, None))


# ------------------------------------------------------------------------------------------------ the free run
def block(sd, blk, tb, h, e, pos, adj, ada):
    """One EquivariantMixBlock (dmt.py:122-174) + CoM removal, every stage fed by the mirror's own previous stage.  Returns every buffer."""
    o = {}
    g, _ = edge_geom(sd, blk, tb, pos, e, ada)
    o.update(g)
    o.update(node_qkv(sd, blk, tb, h, ada))
    o.update(attn_alpha(sd, blk, tb, o["qkv"].ref, o["ye"].ref, adj))
    o.update(attn_out(sd, blk, tb, o["alpha"].ref, o["qkv"].ref, o["ye"].ref))
    o.update(node_u(sd, blk, tb, o["attn"].ref))
    o.update(node_update(sd, blk, tb, h, o["attn"].ref, ada))
    o.update(node_tail(sd, blk, tb, o["h"].ref))
    o.update(edge_update(sd, blk, tb, e, o["u"].ref, ada))
    o.update(edge_tail(sd, blk, tb, o["e"].ref, o["dist"].ref))
    o.update(equi_pairs(sd, blk, tb, o["ac"].ref, o["ed"].ref, pos, adj, ada))
    o.update(pos_update(tb, pos, o["tr"].ref))
    return o


def forward(sd, cfg, n_atoms, xh, edge_x, cond_x, cond_edge_x, temb):
    """The whole denoiser from the time embedding [B, 1024] on: ``(blocks, out)`` with blocks[k] = {buffer: float64 value} of block k."""
    tb = tables(n_atoms)
    ada = ada_table(sd, temb)
    i0, adj, _ = init(sd, cfg, tb, xh, edge_x, cond_x, cond_edge_x, ada)
    h, e, pos = i0["h"].ref, i0["e"].ref, i0["pos"].ref
    ah, eh, blocks = [h], [e], []
    for blk in range(NB):
        o = block(sd, blk, tb, h, e, pos, adj, ada)
        h, e, pos = o["h"].ref, o["e"].ref, o["pos"].ref
        ah.append(o["atom_hids"].ref)
        eh.append(o["edge_hids"].ref)
        blocks.append({k: v.ref for k, v in o.items()})
    out = readout(sd, tb, xh.shape[1], torch.cat(ah, 1), torch.cat(eh, 1), pos, int(bool(torch.isnan(pos).any())))
    return blocks, out, adj


# ------------------------------------------------------------------------------------------------ the numpy split-fp16 emulation
def split_planes_np(x, truncate=False):
    """fp32 array -> (a1, a2) fp16 planes with a = a1 + a2 / 2048, both rounded to nearest (``truncate``: plane 1 cut towards zero while
    plane 2 still refers to the rounded plane 1 - the defect of a converting kernel that rounds in the wrong mode)."""
    x = np.asarray(x, np.float32)
    a1 = x.astype(np.float16)
    a2 = ((x - a1.astype(np.float32)) * np.float32(SPLIT)).astype(np.float16)
    if truncate:
        over = np.abs(a1.astype(np.float32)) > np.abs(x)
        a1 = np.where(over, np.nextafter(a1, np.float16(0)), a1).astype(np.float16)
    return a1, a2


def emulate_split_product(A, W, bias, rng, drop_cross=False, truncate=False):
    """``A W^T + bias`` as the kernels form it, in numpy: fp16 planes, a1 w1 into a high fp32 accumulator that starts at the bias, a1 w2 and
    a2 w1 into a low one, every addition rounded to fp32, the k order shuffled by ``rng``, joined by one fused multiply-add."""
    a1, a2 = (p.astype(np.float32) for p in split_planes_np(A, truncate))
    w1, w2 = (p.astype(np.float32) for p in split_planes_np(W))
    M, K = a1.shape
    hi = np.broadcast_to(np.zeros(W.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32), (M, W.shape[0])).copy()
    lo = np.zeros_like(hi)
    for k in rng.permutation(K):
        hi = (hi + np.outer(a1[:, k], w1[:, k])).astype(np.float32)        # an fp16 x fp16 product is exact in fp32
    for j in rng.permutation(2 * K):
        k = j >> 1
        if j & 1:
            lo = (lo + np.outer(a1[:, k], w2[:, k])).astype(np.float32)
        elif not drop_cross:
            lo = (lo + np.outer(a2[:, k], w1[:, k])).astype(np.float32)
    return (lo.astype(np.float64) / SPLIT + hi.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ teacher forcing
BLOCK_BUFFERS = ("dist", "ye", "qkv", "alpha", "attn", "u", "h", "atom_hids", "ac", "e", "edge_hids", "ed", "tr", "pos")


def teacher_forced_block(sd, blk, tb, h_in, e_in, pos_in, adj, ada, obs):
    """Every stage of block ``blk`` evaluated FROM THE OBSERVED TENSORS of the stage in front of it (``obs``: the buffers of ``BLOCK_BUFFERS`` as
    they stand after the block, ``ye`` reconstructed from its planes, ``alpha`` = the contents of ``lg``; ``h_in`` / ``e_in`` / ``pos_in``: the
    snapshot taken before the block).  Returns ``{buffer: Ref}``."""
    o = {}
    o.update(edge_geom(sd, blk, tb, pos_in, e_in, ada)[0])
    o.update(node_qkv(sd, blk, tb, h_in, ada))
    o.update(attn_alpha(sd, blk, tb, obs["qkv"], obs["ye"], adj))
    o.update(attn_out(sd, blk, tb, obs["alpha"], obs["qkv"], obs["ye"]))
    o.update(node_u(sd, blk, tb, obs["attn"]))
    o.update(node_update(sd, blk, tb, h_in, obs["attn"], ada))
    o.update(node_tail(sd, blk, tb, obs["h"]))
    o.update(edge_update(sd, blk, tb, e_in, obs["u"], ada))
    o.update(edge_tail(sd, blk, tb, obs["e"], obs["dist"]))
    o.update(equi_pairs(sd, blk, tb, obs["ac"], obs["ed"], pos_in, adj, ada))
    o.update(pos_update(tb, pos_in, obs["tr"]))
    return o


def shares(refs, obs, names=None):
    """``[(name, max |got - ref|, largest |got - ref| / allowance, index of that element)]`` for the buffers of ``refs`` (an empty buffer: 0, 0)."""
    rows = []
    for name in (names or refs):
        r, got = refs[name], dbl(obs[name]).reshape(refs[name].ref.shape)
        if r.ref.numel() == 0:
            rows.append((name, 0.0, 0.0, ()))
            continue
        dev = (got - r.ref).abs()
        al = allowance(r).expand_as(dev)
        sh = torch.where(dev == 0, torch.zeros_like(dev), dev / al)           # an exact element never fails, whatever its allowance
        sh = torch.where(torch.isnan(got) | torch.isinf(got), torch.full_like(sh, math.inf), sh)
        i = int(sh.reshape(-1).argmax())
        rows.append((name, float(dev.max()), float(sh.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(sh.shape)))))
    return rows
