"""Float64 yardstick of SpecFormer's residual-score attention in its three hand-written forms - ``dst_spec_attn_flash_fwd / _bwd``
(csrc/ds_train_attn.hip), ``dst_spec_attn_fwd / _bwd`` (csrc/ds_train.hip), ``ds_spec_attention`` (csrc/ds_spec.hip) - plain torch on the CPU.
TEST INFRASTRUCTURE ONLY; pinned without a GPU by tests/test_spec_attn_mirror_cpu.py, used by tests/test_spec_attn_gpu.py.  Written from
include/diffspectra_train.h and specformer.py:385-425, not from the kernels; ``rb`` and ``U`` are tests/chain_mirror.py's, the accumulation
bound is its ``product_bound`` figure written out for batched [B, H, ., .] operands.

LAYOUT.  ``qkv_layers``: one [B, L, 3 H dk] tensor (q | k | v) per layer; ``dout_layers``: one [B, L, H dk] per layer.  Scores, probabilities
and score gradients are [B, H, query, key]; outputs and gradients come back in the layout of the inputs.

``exact``.  scores_l = scale q_l k_l^T + scores_{l-1} (``prev`` in front of layer 0, if given), P_l = softmax over the keys, out_l = P_l v_l.
With G_l = P_l (dO_l v_l^T - D_l), D_l = rowsum(dO_l * out_l) the softmax gradient of layer l alone:  dv_l = P_l^T dO_l;  the gradient of
scores_l is the CHAIN dscores_l = G_l + dscores_{l+1} (scores_l is layer l + 1's addend), dq_l = scale dscores_l k_l, dk_l = scale
dscores_l^T q_l.  Unrolled, dscores_j = sum_{l >= j} G_l: layer l contributes scale G_l k_j to dq_j and scale G_l^T q_j to dk_j for every
j <= l - the DECOMPOSITION the flash form computes (``contrib_q[l][j]``, ``contrib_k[l][j]``).  Row maximum and row sum are returned in both
conventions: natural-log domain (max of scores, sum of exp(scores - max): the fp32 form's stats) and log2 domain (max of scores * log2 e;
the sum is the same number: the flash form's stats).

``flash_emulation``.  ONE call of the flash kernels with n_layers = len(qkv_layers), their roundings applied in float64 arithmetic:
forward   q^ = bf16(fp32(q * fp32(scale * log2 e))), k^ = bf16(k), v^ = bf16(v); s = [q^_0 | ..] [k^_0 | ..]^T; online softmax over tiles of 32
          keys: m_t = running maximum behind tile t, p = exp2(s - m_t) for the keys of tile t, P^ = bf16(p) (rounded RELATIVE TO THE RUNNING
          maximum: bf16 rounding does not commute with the later rescaling), w = exp2(m_t - m); l = sum p w (from the UNROUNDED p),
          out = (sum P^ w v^) / l;  stats = (m, l);
backward  TEACHER-FORCED: from the (m, l) and ``out`` it is given (the kernel's own, as the kernel's backward takes them), else from its own.
          D = dO . out from the unrounded dO (fp32); x = m + log2 l; -x and -D as hi + lo bf16 (``split2``: hi = bf16(y), lo = bf16(y - hi));
          s' = [q^ | -x_hi | -x_lo] [k^ | 1 | 1]^T, p = exp2(s'), dP' = [bf16(dO) | -D_hi | -D_lo] [v^ | 1 | 1]^T, dS = p dP', dS^ = bf16(dS),
          P^ = bf16(p); dq_j = fp32(scale) dS^ k^_j, dk_j = fp32(ln 2) dS^^T q^_j (q^ carries scale * log2 e), dv = P^^T bf16(dO).
``round_operands=False`` switches every rounding off: the result is ``exact``'s.

BOUNDS, per element, returned with every result (``bound[name]`` = (a) + (b), ``bound[name + "_b"]`` = (b) alone).  Products of two bf16 numbers
are exact in fp32, so what separates a kernel from this emulation is
(a) fp32 ACCUMULATION and the elementary functions.  An observed sum of K exact products: twice gamma_K, ``2 (K + 2) 2^-24 sum |a| |b|``, for ANY
    order (``product_bound``'s figure) - the scores (K = 8 n, + 2 spare columns in the backward), dP' (K = 10), and with the number of keys or
    queries as K the sums over P^ and dS^.  The scores are not observed: an error ds of a score and dm of its (running) maximum reach p =
    exp2(s - m) as p (2^(ds + dm) - 1) = ln 2 (ds + dm) p to first order (``expm1`` here), plus ``EXP_ULPS`` 2^-24 p for v_exp_f32 and the
    multiply, plus 2^-24 ln 2 |s - m| p for the rounded subtraction; a rescaling weight w is a product of up to NT such exponentials.  A
    (running) maximum of the kernel's scores lies in [s* - bs*, max (s + bs)], s* the emulation's largest score so far and bs* its bound.
    With ``max_obs`` - the kernel's stats[.., 0] - the FINAL maximum is known exactly, and so is the running maximum of every tile behind a
    key that wins clearly (``_clear``): there the error of the maximum is 0 and w = 1 exactly.  l: the sum of those
    errors over the row plus twice gamma_L l.  out = num / l: (error of num) / l + |out| (error of l) / l + 3 ulp.  dS = p dP': |dP'| (error of
    p) + p (error of dP') + one ulp.  D is an fp32 sum of 8 products of fp32 numbers: gamma_8 sum |dO| |out|, twice.  x = m + log2 l in fp32
    from OBSERVED m, l: 2 ulp of |log2 l| for v_log_f32 plus an ulp of the sum.
(b) ROUNDING RISK.  P^, dS^ and the halves of split2(-x), split2(-D) are bf16 roundings of fp32 values the test cannot observe.  The kernel's
    value lies within its bound (a) of the emulation's float64 value, so both round to the SAME bf16 number unless the float64 value is
    within (a) of a rounding boundary (a bf16 midpoint); then the kernel may hold the neighbour: one bf16 ulp of that entry (where (a)
    itself exceeds half an ulp - a difference that cancels, dS of a one-key row - any grid point within (a) + one ulp: ``flip``).  For exactly
    those entries - ``share_at_risk`` of them - one ulp times |other operand| is added to the sums they enter; every other entry contributes
    NOTHING, although it is rounded with a relative step of 2^-8.  For a split2 pair: hi and lo both safe - the pair is bit-identical, error
    0; lo at risk - one ulp of lo; hi at risk - (a) + 2^-16 |y| (each pair represents its own y to 2^-17 |y|).
Second-order terms (error times error) are carried where they are cheap - expm1, (1 + rel) factors - and are otherwise below 2^-40 of
the bound.  exp2 results below 2^-120 (flushed or denormal, a different bf16 grid) get an absolute allowance of 2^-120: ``TINY``.

If the derived bound did not hold on the GPU, that would be a finding - a kernel bug or a term missing above - to be resolved as such, not
scaled away.  So far, both found while this file was written and both errors of the derivation, not of the kernels: (1) the CPU fp32
emulation at L = 1 left the bound by a factor 2 - dS = p (dP - D) cancels to rounding noise there, so (a) is many ulps of dS and "the
neighbour" was too little: ``flip``; (2) on the GPU, 9 of 270 000 dq / dk elements at L = 352 and 384, one layer, were up to 3.7 times their
bound: each traced (offline, from the kernel's saved results) to ONE dS entry rounded to the other neighbour in a row whose split2(-x) had
its hi half at risk - the pair's residual had been written as 2^-18 |y| instead of 2^-17 |y| (``split2``).  With both corrected every case
holds; the first green table is in profiles/HISTORY.md."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.chain_mirror import U, rb

H, DK = 16, 8
LOG2E = 1.4426950408889634                       # the kernels' constants, as written there; they are rounded to fp32 where the kernel holds them in fp32
LN2 = 0.6931471805599453
LOG2E_F32 = float(np.float32(LOG2E))
LN2_F32 = float(np.float32(LN2))
EXP_ULPS = 4.0                                   # v_exp_f32 (1 ulp) + one multiply or subtraction + slack, in units of 2^-24 relative
TINY = 2.0 ** -120
BF16_MIN = 2.0 ** -133                           # the smallest positive bf16 (denormal)
TILE = 32


# ------------------------------------------------------------------------------------------------ layout
def heads(x, n_heads=H):
    """[B, L, n_heads dk] -> [B, n_heads, L, dk]."""
    B, L, D = x.shape
    return x.reshape(B, L, n_heads, D // n_heads).permute(0, 2, 1, 3)


def merge(x):
    """[B, n_heads, L, dk] -> [B, L, n_heads dk]."""
    B, Hh, L, dk = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, Hh * dk)


def parts(qkv, n_heads=H):
    """(q, k, v) of one layer's [B, L, 3 D] buffer, each [B, n_heads, L, dk], dtype kept."""
    D = qkv.shape[-1] // 3
    return tuple(heads(qkv[..., i * D:(i + 1) * D], n_heads) for i in range(3))


def random_inputs(B, L, n_layers, seed, n_heads=H, dk=DK, qk_mul=1.0):
    """fp32 inputs of order 1 (tests/chain_mirror.random_inputs' style: one seeded generator per case): (qkv_layers, dout_layers)."""
    g = torch.Generator().manual_seed(seed)
    D = n_heads * dk
    qkv = [torch.randn(B, L, 3 * D, generator=g) for _ in range(n_layers)]
    for x in qkv:
        x[..., :2 * D] *= qk_mul
    dout = [torch.randn(B, L, D, generator=g) for _ in range(n_layers)]
    return qkv, dout


def dot_bound(absA, absB, K, scale=1.0, addend=None):
    """``product_bound``'s figure for UNROUNDED operands: 2 (K + 2) 2^-24 (|scale| |A| |B|^T + |addend|) for a K-term fp32 dot product that is
    then scaled and added to ``addend``."""
    m = abs(scale) * (absA @ absB.transpose(-1, -2))
    if addend is not None:
        m = m + addend.abs()
    return 2.0 * (K + 2) * U * m


# ------------------------------------------------------------------------------------------------ exact
def exact(qkv_layers, scale, dout_layers=None, prev=None, n_heads=H):
    """The attention of 1 .. 3 chained layers and, with ``dout_layers``, its gradients in closed form, in float64 (module docstring).
    ``prev`` [B, H, query, key]: scores in front of layer 0 (the inference form's has_prev)."""
    n = len(qkv_layers)
    scale = float(scale)
    q, k, v = zip(*(parts(x.double(), n_heads) for x in qkv_layers))
    r = dict(scores=[], max_ln=[], sum_ln=[], max_log2=[], sum_log2=[], P=[], out=[])
    s = 0.0 if prev is None else prev.double()
    outs = []
    for l in range(n):
        s = scale * (q[l] @ k[l].transpose(-1, -2)) + s
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        z = e.sum(-1, keepdim=True)
        P = e / z
        o = P @ v[l]
        outs.append(o)
        r["scores"].append(s); r["P"].append(P); r["out"].append(merge(o))
        r["max_ln"].append(m.squeeze(-1)); r["sum_ln"].append(z.squeeze(-1))
        r["max_log2"].append(m.squeeze(-1) * LOG2E); r["sum_log2"].append(z.squeeze(-1))     # exp2(s log2 e - m log2 e) = exp(s - m)
    if dout_layers is None:
        return r
    G, dv = [], []
    for l in range(n):
        dO = heads(dout_layers[l].double(), n_heads)
        D = (dO * outs[l]).sum(-1, keepdim=True)
        G.append(r["P"][l] * (dO @ v[l].transpose(-1, -2) - D))
        dv.append(r["P"][l].transpose(-1, -2) @ dO)
    ds = [None] * n
    for l in range(n - 1, -1, -1):
        ds[l] = G[l] if l == n - 1 else G[l] + ds[l + 1]
    r["G"], r["dscores"] = G, ds
    r["dq"] = [merge(scale * (ds[l] @ k[l])) for l in range(n)]
    r["dk"] = [merge(scale * (ds[l].transpose(-1, -2) @ q[l])) for l in range(n)]
    r["dv"] = [merge(x) for x in dv]
    r["dqkv"] = [torch.cat([r["dq"][l], r["dk"][l], r["dv"][l]], -1) for l in range(n)]
    r["contrib_q"] = [[merge(scale * (G[l] @ k[j])) for j in range(l + 1)] for l in range(n)]
    r["contrib_k"] = [[merge(scale * (G[l].transpose(-1, -2) @ q[j])) for j in range(l + 1)] for l in range(n)]
    return r


# ------------------------------------------------------------------------------------------------ bf16 rounding with its risk
def bf16_margin(x):
    """(r, margin, ulp) of float64 ``x``: r = bf16(x); ulp = the spacing of bf16 at r; margin = the distance of x from the nearer boundary of
    r's rounding interval (half an ulp to either side; a quarter below a power of two).  r = 0: margin = inf, ulp = 0 (``TINY`` covers it)."""
    r = rb(x)
    man, e = torch.frexp(r)
    ulp = torch.ldexp(torch.ones_like(r), e - 8)
    inward = (man.abs() == 0.5) & (x.abs() < r.abs())
    margin = torch.where(inward, ulp / 4, ulp / 2) - (x - r).abs()
    zero = r == 0
    return r, torch.where(zero, BF16_MIN / 2 - x.abs(), margin), torch.where(zero, torch.full_like(r, BF16_MIN), ulp)


def flip(margin, ulp, err):
    """What bf16(kernel's value) may differ from bf16(x) by when the kernel's value lies within ``err`` of x: nothing if x is further than
    ``err`` from a rounding boundary; else the neighbour (one ulp) - or, where ``err`` itself exceeds half an ulp (a difference that
    cancels: dS of a one-key row is 0 +- rounding), any grid point up to err + half an ulp of either side away: err (1 + 2^-8) + ulp."""
    return torch.where(margin <= err, torch.where(err <= ulp / 2, ulp, err * (1.0 + 2.0 ** -8) + ulp), torch.zeros_like(ulp))


def round_with_risk(x, err, on=True):
    """(bf16(x), allowance): ``flip`` of x."""
    if not on:
        return x, torch.zeros_like(x)
    r, margin, ulp = bf16_margin(x)
    return r, flip(margin, ulp, err)


def split2(y, err, on=True, drop_lo=False):
    """``y`` (float64, known to ``err``) as the kernels' hi + lo bf16 pair of its fp32 value: (hi + lo, |hi| + |lo|, what the kernel's pair may
    differ by).  ``drop_lo``: the deliberately broken form of the CPU tests."""
    if not on:
        return y, y.abs(), torch.zeros_like(y)
    y32 = y.float().double()
    err = err + U * y32.abs()                                            # (this float64 -> fp32 rounding)
    hi, mar_h, _ = bf16_margin(y32)
    lo, mar_l, ulp_l = bf16_margin(y32 - hi)
    if drop_lo:
        lo = torch.zeros_like(lo)
    whole = err + 2.0 ** -16 * y32.abs()                                   # |y - hi| <= 2^-8 |y|, lo within 2^-9 |y - hi| of it: 2^-17 |y| per pair
    b = torch.where(mar_h <= err, whole, torch.minimum(flip(mar_l, ulp_l, err), whole))
    return hi + lo, hi.abs() + lo.abs(), b


def _running(x, L):
    """Per key: the maximum of ``x`` [.., L keys] over all keys of the tiles up to and including the key's own."""
    NT = (L + TILE - 1) // TILE
    pad = torch.full(x.shape[:-1] + (NT * TILE - L,), -math.inf, dtype=x.dtype)
    t = torch.cat([x, pad], -1).reshape(x.shape[:-1] + (NT, TILE)).amax(-1)
    return torch.cummax(t, -1).values.repeat_interleave(TILE, -1)[..., :L]


def _clear(s, bs, L):
    """Per key: whether the largest score s* of the tiles up to and including the key's own is a CLEAR winner there - s* - bs* above s + bs
    of every other key so far - so that whatever the kernel's scores are within their bounds, its running maximum is that key's score."""
    NT = (L + TILE - 1) // TILE
    up, lo, res = s + bs, s - bs, []
    for t in range(NT):
        e = min(L, TILE * (t + 1))
        if e == 1:
            res.append(torch.ones(s.shape[:-1], dtype=torch.bool))
            continue
        top = up[..., :e].topk(2, -1)
        star = s[..., :e].argmax(-1, keepdim=True)
        res.append((top.indices[..., :1] == star).squeeze(-1) & (lo.gather(-1, star).squeeze(-1) > top.values[..., 1]))
    return torch.stack(res, -1).repeat_interleave(TILE, -1)[..., :L]


# ------------------------------------------------------------------------------------------------ the flash form
def flash_operands(qkv_layers, scale, on=True, n_heads=H):
    """([q^_0 | ..], [k^_0 | ..], v^ of the last layer, q^ per layer, k^ per layer), float64 [B, H, L, .]."""
    qs, ks, v = [], [], None
    qmul32 = float(np.float32(scale) * np.float32(LOG2E))
    for x in qkv_layers:
        q, k, v = parts(torch.as_tensor(x), n_heads)
        qs.append(rb(q.float() * qmul32) if on else q.double() * (float(scale) * LOG2E))      # fp32 multiply, then bf16: as the kernel converts
        ks.append(rb(k, on))
    return torch.cat(qs, -1), torch.cat(ks, -1), rb(v, on), qs, ks


def flash_emulation(qkv_layers, scale, dout=None, stats=None, out=None, round_operands=True, n_heads=H, drop_lo=False, max_obs=None):
    """One call of dst_spec_attn_flash_fwd and - with ``dout`` [B, L, D] - of dst_spec_attn_flash_bwd with n_layers = len(qkv_layers) (module
    docstring).  ``stats`` [B, H, L, 2] and ``out`` [B, L, D]: the forward results the backward starts from (default: its own).
    Returns dict(scores, max, sum, out; dq[j], dk[j] for j < n_layers, dv; bound = {...}; share_at_risk, share_zero_allowance = {...})."""
    on = round_operands
    n = len(qkv_layers)
    B, L, _ = qkv_layers[0].shape
    NT = (L + TILE - 1) // TILE
    Q, K, V, qs, ks = flash_operands(qkv_layers, scale, on, n_heads)
    KT, aV = K.transpose(-1, -2), V.abs()
    Kd = Q.shape[-1]
    u = U if on else 0.0
    s = Q @ KT
    bs = 2.0 * (Kd + 2) * u * (Q.abs() @ KT.abs())
    m_run = _running(s, L)
    # a running maximum of the kernel's scores lies in [s* - bs*, max (s + bs)] (s* = the emulation's largest score so far, bs* its bound)
    bm_run = torch.maximum(_running(s + bs, L) - m_run, _running(torch.where(s == m_run, bs, torch.zeros_like(bs)), L))
    m, bm = m_run[..., -1:], bm_run[..., -1:]
    m_use, bm_use, m_fin, bm_fin, pinned = m_run, bm_run, m, bm, torch.zeros_like(s, dtype=torch.bool)
    if on and max_obs is not None:
        # The kernel's final maximum is OBSERVED (stats[.., 0]; compared with m separately): it takes m's place with no error.  Where one key
        # is the clear winner so far (_clear) the kernel's running maximum is that key's score; if it is also the row's clear winner, that
        # score is the observed maximum: the tile's p is exp2(s - observed) with the error of s alone, its rescaling weight exactly 1.
        clear = _clear(s, bs, L)
        pinned = clear & clear[..., -1:] & (m_run == m)
        m_fin, bm_fin = torch.as_tensor(max_obs).double().reshape(m.shape), torch.zeros_like(bm)
        m_use, bm_use = torch.where(pinned, m_fin, m_run), torch.where(pinned, bm_fin, bm_run)
    p, w = torch.exp2(s - m_use), torch.exp2(m_use - m_fin)
    rel_p = torch.expm1(LN2 * (bs + bm_use)) + u * (EXP_ULPS + LN2 * (m_use - s).abs())
    rel_w = torch.where(pinned, torch.zeros_like(w), torch.expm1(LN2 * (bm_use + bm_fin)) + u * (NT * EXP_ULPS + LN2 * (m_fin - m_use).abs()))
    l = (p * w).sum(-1, keepdim=True)
    b_l = (p * w * (rel_p + rel_w + rel_p * rel_w)).sum(-1, keepdim=True) + 2.0 * (L + 2) * u * l + (TINY if on else 0.0)
    Ph, allow = round_with_risk(p, p * rel_p + TINY, on)
    num = (Ph * w) @ V
    b_num_a = (Ph * w * (rel_w + 2.0 * (L + NT + 2) * u)) @ aV
    b_num_b = (allow * w * (1.0 + rel_w)) @ aV
    o = num / l
    grow = 1.0 + b_l / l
    b_out_a = (b_num_a / l + o.abs() * (b_l / l + 3.0 * u)) * grow
    b_out_b = b_num_b / l * grow
    r = dict(scores=s, max=m.squeeze(-1), sum=l.squeeze(-1), out=merge(o),
             bound=dict(scores=bs, max=bm.squeeze(-1), sum=b_l.squeeze(-1), out=merge(b_out_a + b_out_b), out_b=merge(b_out_b)),
             share_at_risk=dict(P=float((allow > 0).double().mean())), share_zero_allowance=dict(out=float((b_out_b == 0).double().mean())))
    if dout is None:
        return r

    # ---- backward, from the forward results it is handed
    st = torch.stack([r["max"], r["sum"]], -1) if stats is None else torch.as_tensor(stats).double().reshape(B, n_heads, L, 2)
    oo = o if out is None else heads(torch.as_tensor(out).double(), n_heads)
    dO = heads(torch.as_tensor(dout).double(), n_heads)
    dOh = rb(dO, on)
    D = (dO * oo).sum(-1, keepdim=True)
    bD = 2.0 * (DK + 2) * u * (dO.abs() * oo.abs()).sum(-1, keepdim=True)
    lg = torch.log2(st[..., 1:2])
    x = st[..., 0:1] + lg
    bx = 2.0 * u * (lg.abs() + x.abs())
    nx, ax, bnx = split2(-x, bx, on, drop_lo)
    nD, aD, bnD = split2(-D, bD, on, drop_lo)
    sp = s + nx
    bsp = 2.0 * (Kd + 4) * u * (Q.abs() @ KT.abs() + ax) + bnx
    pb = torch.exp2(sp)
    rel_pb = torch.expm1(LN2 * bsp) + EXP_ULPS * u
    dP = dOh @ V.transpose(-1, -2) + nD
    b_dP = 2.0 * (DK + 4) * u * (dOh.abs() @ aV.transpose(-1, -2) + aD) + bnD
    dS = pb * dP
    b_dS = dP.abs() * pb * rel_pb + pb * (1.0 + rel_pb) * b_dP + u * dS.abs() + (TINY if on else 0.0)
    dSh, allow_s = round_with_risk(dS, b_dS, on)
    Pbh, allow_p = round_with_risk(pb, pb * rel_pb + TINY, on)
    acc = 2.0 * (L + 2) * u
    f_q, f_k = (float(np.float32(scale)), LN2_F32) if on else (float(scale), LN2)
    r["dq"], r["dk"] = [], []
    bq, bqb, bk, bkb = [], [], [], []
    for j in range(n):
        kj, qj = ks[j], qs[j]
        g = f_q * (dSh @ kj)
        bb = abs(f_q) * (allow_s @ kj.abs())
        r["dq"].append(merge(g)); bqb.append(merge(bb))
        bq.append(merge(abs(f_q) * acc * (dSh.abs() @ kj.abs()) + 2.0 * u * g.abs() + bb))
        g = f_k * (dSh.transpose(-1, -2) @ qj)
        bb = abs(f_k) * (allow_s.transpose(-1, -2) @ qj.abs())
        r["dk"].append(merge(g)); bkb.append(merge(bb))
        bk.append(merge(abs(f_k) * acc * (dSh.abs().transpose(-1, -2) @ qj.abs()) + 2.0 * u * g.abs() + bb))
    dv = Pbh.transpose(-1, -2) @ dOh
    b_dv_b = allow_p.transpose(-1, -2) @ dOh.abs()
    r["dv"] = merge(dv)
    r["bound"].update(dq=bq, dq_b=bqb, dk=bk, dk_b=bkb, dv=merge(acc * (Pbh.transpose(-1, -2) @ dOh.abs()) + b_dv_b), dv_b=merge(b_dv_b))
    r["share_at_risk"].update(dS=float((allow_s > 0).double().mean()), P_bwd=float((allow_p > 0).double().mean()),
                              split2_x=float((bnx > 0).double().mean()), split2_D=float((bnD > 0).double().mean()))
    zero = lambda t: float((t == 0).double().mean())
    r["share_zero_allowance"].update(dq=min(zero(t) for t in bqb), dk=min(zero(t) for t in bkb), dv=zero(r["bound"]["dv_b"]))
    return r
