"""CPU yardstick of the small kernels of the training library (``csrc/ds_train.hip``): batch preparation, noising, Kabsch alignment, the
loss, the time features, the adjacency bits, BatchNorm / LayerNorm of the SpecFormer, the AdamW + EMA step and the bf16 rounding.

numpy / torch float64 only: no GPU, nothing of ``diffspectra_amd``.  One plain function per operation, RESTATED from the reference's
formulas, each with the lines it stands for (as ``oracle/`` does for the model and ``structure_mirror.py`` for the structure metric);
nothing of the reference's text is copied.  ``tests/test_train_mirror_cpu.py`` pins every function: the loss side to golden G13 (the
reference's own tensors), the norms and the optimizer to torch's float64 implementations, the rounding to ``Tensor.bfloat16()``.

Everything is PACKED as ``TrainLayout`` packs it: a batch is its list ``n_atoms``; node arrays are ``[Nn, .]`` with the atoms of molecule
0 first; pair arrays are ``[Pp, .]`` with the unordered pairs (a < b) of molecule 0 first, a ascending, then b ascending
(``p = a (2 n - a - 1) / 2 + (b - a - 1)``).

Also here: the seeded generator of Kabsch cases the GPU test runs (rank-deficient, degenerate, mirrored and ill-conditioned covariances).
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = np.float64


# ------------------------------------------------------------------------------------------------ the packed layout
def offsets(n_atoms):
    """(node_off [B+1], pair_off [B+1]) of the packed layout."""
    n = np.asarray(n_atoms, dtype=np.int64)
    node_off, pair_off = np.zeros(len(n) + 1, np.int64), np.zeros(len(n) + 1, np.int64)
    node_off[1:], pair_off[1:] = np.cumsum(n), np.cumsum(n * (n - 1) // 2)
    return node_off, pair_off


def node_molecule(n_atoms):
    """[Nn] molecule of every node row."""
    return np.repeat(np.arange(len(n_atoms)), np.asarray(n_atoms, dtype=np.int64))


def pair_tables(n_atoms):
    """(a [Pp], b [Pp], molecule [Pp]): the atoms of every pair row as indices INSIDE their molecule, and the molecule."""
    pa, pb, pm = [], [], []
    for m, n in enumerate(n_atoms):
        a, b = np.triu_indices(int(n), 1)
        pa.append(a); pb.append(b); pm.append(np.full(a.shape, m))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)
    return cat(pa), cat(pb), cat(pm)


def pack_nodes(dense, n_atoms):
    """Dense ``[B, N, c]`` -> packed ``[Nn, c]``."""
    dense = np.asarray(dense)
    return np.concatenate([dense[m, :int(n)] for m, n in enumerate(n_atoms)], axis=0)


def pack_pairs(dense, n_atoms, lower: bool = False):
    """Dense ``[B, N, N, c]`` -> packed ``[Pp, c]``: cell (a, b) of every pair a < b, or the transposed cell (b, a) with ``lower``."""
    dense = np.asarray(dense)
    a, b, m = pair_tables(n_atoms)
    return dense[m, b, a] if lower else dense[m, a, b]


def unpack_nodes(packed, n_atoms, n_max=None):
    packed = np.asarray(packed)
    N = int(max(n_atoms)) if n_max is None else int(n_max)
    out = np.zeros((len(n_atoms), N) + packed.shape[1:], dtype=packed.dtype)
    off, _ = offsets(n_atoms)
    for m, n in enumerate(n_atoms):
        out[m, :int(n)] = packed[off[m]:off[m + 1]]
    return out


def unpack_pairs(packed, n_atoms, n_max=None):
    """Packed ``[Pp, c]`` -> dense symmetric ``[B, N, N, c]`` (both cells of a pair, zero diagonal and padding)."""
    packed = np.asarray(packed)
    N = int(max(n_atoms)) if n_max is None else int(n_max)
    out = np.zeros((len(n_atoms), N, N) + packed.shape[1:], dtype=packed.dtype)
    a, b, m = pair_tables(n_atoms)
    out[m, a, b] = packed
    out[m, b, a] = packed
    return out


def _molecule_mean(x, n_atoms):
    """[Nn, c] per-atom copy of the mean over the atoms of the atom's molecule."""
    mol = node_molecule(n_atoms)
    s = np.zeros((len(n_atoms), x.shape[1]), F64)
    np.add.at(s, mol, x)
    return (s / np.asarray(n_atoms, F64)[:, None])[mol]


# ------------------------------------------------------------------------------------------------ batch preparation, noising
def prepare_batch(n_atoms, pos, one_hot, fc, edge, factors):
    """``process_edge_batch`` + ``get_data_scaler`` for centered data with formal charges (losses.py:498-529, utils.py:33-68): positions
    without their molecule's centre of mass over ``pos_norm``; one-hot types as +-1 over ``type_norm``; charges over ``charge_norm``;
    pair features as +-1 over ``edge_norm``.  ``pos [Nn,3]``, ``one_hot [Nn,5]``, ``fc [Nn]``, ``edge [Pp,2]``,
    ``factors = (pos, type, charge, edge)`` -> ``(x [Nn,9], ex [Pp,2])``."""
    pos, one_hot, fc, edge = (np.asarray(v, F64) for v in (pos, one_hot, fc, edge))
    pn, tn, cn, en = (float(v) for v in factors)
    x = np.concatenate([(pos - _molecule_mean(pos, n_atoms)) / pn, (one_hot * 2.0 - 1.0) / tn, fc.reshape(-1, 1) / cn], axis=1)
    return x, (edge * 2.0 - 1.0) / en


def noising(n_atoms, alpha, sigma, x, raw, ex, eraw):
    """``z_t = alpha_t x + sigma_t eps`` (losses.py:318-326) with the noise of models/utils.py:67-106: the three position columns of the
    node noise lose their molecule's mean, the six feature columns are taken as drawn; ``eraw`` is the pair's value of the symmetric
    edge noise (the lower-triangle draw).  ``alpha, sigma [B]`` -> ``(z [Nn,9], ez [Pp,2])``."""
    alpha, sigma, x, raw, ex, eraw = (np.asarray(v, F64) for v in (alpha, sigma, x, raw, ex, eraw))
    eps = raw.copy()
    eps[:, :3] -= _molecule_mean(raw[:, :3], n_atoms)
    mol, pm = node_molecule(n_atoms), pair_tables(n_atoms)[2]
    return alpha[mol, None] * x + sigma[mol, None] * eps, alpha[pm, None] * ex + sigma[pm, None] * eraw


# ------------------------------------------------------------------------------------------------ Kabsch alignment
def kabsch_align(n_atoms, pred, tar):
    """``get_align_position`` / ``kabsch_batch`` (losses.py:414-452) per molecule: ``A = pred^T tar``, ``A = U S V^T``,
    ``R = U diag(1, 1, sign det A) V^T``, aligned target ``= tar R^T``.  Returns ``(rot [B,3,3], aligned [Nn,3], S [B,3])``."""
    pred, tar = np.asarray(pred, F64), np.asarray(tar, F64)
    off, _ = offsets(n_atoms)
    B = len(n_atoms)
    rot, aligned, sing = np.zeros((B, 3, 3)), np.zeros_like(tar), np.zeros((B, 3))
    for m in range(B):
        p, t = pred[off[m]:off[m + 1]], tar[off[m]:off[m + 1]]
        A = p.T @ t
        U, S, Vt = np.linalg.svd(A)
        rot[m] = (U * np.array([1.0, 1.0, np.sign(np.linalg.det(A))])) @ Vt
        aligned[off[m]:off[m + 1]] = t @ rot[m].T
        sing[m] = S
    return rot, aligned, sing


def proper_rotation(pred, tar):
    """The rotation (determinant +1) of the Kabsch fit of ONE molecule: ``U diag(1, 1, det U det V^T) V^T``.  It is ``kabsch_align``'s
    wherever the covariance has full rank, and it is still unique where the rank is 2 (three atoms, planar molecules), where
    ``sign det A`` is rounding noise."""
    U, _, Vt = np.linalg.svd(np.asarray(pred, F64).T @ np.asarray(tar, F64))
    return (U * np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])) @ Vt


def det_sign(pred, tar):
    """sign det(pred^T tar) of ONE molecule (the factor ``kabsch_align`` puts on the smallest singular value)."""
    return float(np.sign(np.linalg.det(np.asarray(pred, F64).T @ np.asarray(tar, F64))))


def _random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1.0
    return q


def kabsch_cases(seed: int = 0):
    """``[(name, pred [n,3] f32, tar [n,3] f32)]``: the covariances a QM9 batch brings (single atoms, diatomics, linear and planar
    molecules: rank 0, 1, 2), a three-fold degenerate one, the identity, a reflection, the two ends of the noise schedule at the maximum
    size, and 20 random ``pred = a tar + sqrt(1 - a^2) noise`` with a in [0.003, 1].  Centred like the trainer's inputs."""
    rng = np.random.default_rng(seed)
    cen = lambda v: (v - v.mean(0)).astype(np.float32)
    out = [("n1", np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))]
    t = cen(rng.normal(size=(2, 3)))
    out.append(("n2", cen(0.3 * t + 0.9 * rng.normal(size=(2, 3))), t))
    t = cen(np.outer([-1.1, 0.0, 1.3], rng.normal(size=3)))
    out.append(("collinear3", cen(0.5 * t + 0.8 * rng.normal(size=(3, 3))), t))
    t = cen(rng.normal(size=(3, 3)))
    out.append(("bent3", cen(0.5 * t + 0.8 * rng.normal(size=(3, 3))), t))
    ang, rad = np.arange(12) * math.pi / 6.0, 1.0 + 0.7 * (np.arange(12) % 2)
    t = cen(np.stack([np.cos(ang) * rad, np.sin(ang) * rad, np.zeros(12)], 1) @ _random_rotation(rng).T)
    out.append(("planar12", cen(0.7 * t + 0.7 * rng.normal(size=(12, 3))), t))
    t = cen(np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F64) * 0.63)       # centred tetrahedron: t^T t = c I
    out.append(("tetrahedron_rotated", cen(t.astype(F64) @ _random_rotation(rng).T), t))
    t = cen(rng.normal(size=(9, 3)))
    out.append(("identical", t.copy(), t))
    out.append(("mirror_image", cen(t * np.array([1.0, 1.0, -1.0])), t))
    t = cen(rng.normal(size=(29, 3)) * 1.5)
    out.append(("n29_pure_noise", cen(0.003 * t + math.sqrt(1.0 - 0.003 ** 2) * rng.normal(size=(29, 3))), t))
    out.append(("n29_no_noise", cen(0.99999 * t + math.sqrt(1.0 - 0.99999 ** 2) * rng.normal(size=(29, 3))), t))
    for s in range(20):
        n = int(rng.integers(3, 30))
        t = cen(rng.normal(size=(n, 3)) * 1.2)
        a = float(rng.uniform(0.003, 1.0))
        out.append((f"random{s}_n{n}", cen(a * t + math.sqrt(1.0 - a * a) * rng.normal(size=(n, 3))), t))
    return out


# ------------------------------------------------------------------------------------------------ loss
def loss_and_grads(n_atoms, pos, feat, edge, tpos, tfeat, tedge, wm, weights=(1.0, 0.25, 0.1)):
    """losses.py:359-394 (pred_data, reduce_mean False) per molecule on packed predictions, gradients by float64 autograd:
    ``loss_m = wm (w0 sum_atoms mean_3 d^2 + w1 sum_atoms mean_6 d^2 + w2 sum_cells mean_2 d^2)``; a pair fills two cells of the dense
    edge tensor.  ``wm [B]`` is the caller's ``sqrt(alpha_t / sigma_t) / B``.  Returns ``(loss_m [B], dpos, dfeat, dedge)`` of
    ``loss_m.sum()``."""
    T = lambda v: torch.as_tensor(np.asarray(v, F64))
    pos, feat, edge = (T(v).clone().requires_grad_(True) for v in (pos, feat, edge))
    mol, pm = torch.as_tensor(node_molecule(n_atoms)), torch.as_tensor(pair_tables(n_atoms)[2])
    B = len(n_atoms)
    per_mol = lambda v, idx: torch.zeros(B, dtype=torch.float64).index_add(0, idx, v)
    l_pos = per_mol(torch.square(pos - T(tpos)).mean(-1), mol)
    l_type = per_mol(torch.square(feat - T(tfeat)).mean(-1), mol)
    l_edge = per_mol(2.0 * torch.square(T(tedge) - edge).mean(-1), pm)
    loss_m = T(wm) * (weights[0] * l_pos + weights[1] * l_type + weights[2] * l_edge)
    loss_m.sum().backward()
    return loss_m.detach().numpy(), pos.grad.numpy(), feat.grad.numpy(), edge.grad.numpy()


# ------------------------------------------------------------------------------------------------ time features, adjacency bits
def time_feat_argument(noise_level, w):
    """``((x w) 2) pi`` formed in float32 in that order, as torch evaluates ``x * weights * 2 * math.pi`` on float32 tensors
    (layers.py:283-288): [B, 8] float32."""
    x, w = np.asarray(noise_level, np.float32).reshape(-1, 1), np.asarray(w, np.float32).reshape(1, -1)
    return ((x * w) * np.float32(2.0)) * np.float32(math.pi)


def time_feat(noise_level, w):
    """Learned sinusoidal features (layers.py:283-288): ``[x, sin(2 pi x w), cos(2 pi x w)]`` -> [B, 17].  The argument is the float32 one
    (``time_feat_argument``), sine and cosine are taken in float64."""
    fr = time_feat_argument(noise_level, w).astype(F64)
    return np.concatenate([np.asarray(noise_level, np.float32).astype(F64).reshape(-1, 1), np.sin(fr), np.cos(fr)], axis=1)


def time_feat_weight_grad(noise_level, w, df):
    """Gradient of the frequencies: ``dw_i = sum_b (df_sin cos(fr) - df_cos sin(fr)) 2 pi x_b`` -> [8]."""
    fr = time_feat_argument(noise_level, w).astype(F64)
    x, df = np.asarray(noise_level, np.float32).astype(F64).reshape(-1, 1), np.asarray(df, F64)
    return ((df[:, 1:9] * np.cos(fr) - df[:, 9:17] * np.sin(fr)) * (2.0 * math.pi * x)).sum(0)


def adj_bits(cond_edge0, d2, edge_th, cutoff):
    """Adjacency of the self-conditioning prediction (dmt.py:338-361): bit 0 = predicted edge-existence channel >= ``edge_quan_th``,
    bit 1 = squared distance of the predicted positions <= the spatial cut-off (both float32 comparisons) -> int32 [Pp]."""
    e, d = np.asarray(cond_edge0, np.float32), np.asarray(d2, np.float32)
    return ((e >= np.float32(edge_th)).astype(np.int32) | ((d <= np.float32(cutoff)).astype(np.int32) << 1)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ BatchNorm / LayerNorm
def batch_norm_train(x, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1):
    """``nn.BatchNorm1d`` in training mode over the rows of ``x [R, C]`` (specformer.py:247,260): batch mean, biased variance for the
    output, unbiased variance into the running statistic.  Returns ``(y, mean, rstd, unbiased variance, running_mean', running_var')``
    (the last two None without running statistics)."""
    x, gamma, beta = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(beta, F64)
    R = x.shape[0]
    mean = x.mean(0)
    var = np.square(x - mean).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    unbiased = var * R / (R - 1)
    rm = rv = None
    if running_mean is not None:
        rm = (1.0 - momentum) * np.asarray(running_mean, F64) + momentum * mean
        rv = (1.0 - momentum) * np.asarray(running_var, F64) + momentum * unbiased
    return (x - mean) * rstd * gamma + beta, mean, rstd, unbiased, rm, rv


def batch_norm_backward(dy, x, mean, rstd, gamma):
    """Backward of ``batch_norm_train`` through the batch statistics: ``(dx, dgamma, dbeta)``."""
    dy, x, gamma = np.asarray(dy, F64), np.asarray(x, F64), np.asarray(gamma, F64)
    R = x.shape[0]
    xh = (x - mean) * rstd
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    return gamma * rstd * (dy - dbeta / R - xh * dgamma / R), dgamma, dbeta


def layer_norm_affine(x, gamma, beta, eps):
    """``nn.LayerNorm`` over the last dimension of ``x [R, C]`` (the SpecFormer's ``out_norm``): ``(y, mean [R], rstd [R])``."""
    x, gamma, beta = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(beta, F64)
    mean = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(np.square(x - mean).mean(1, keepdims=True) + eps)
    return (x - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def layer_norm_backward(dy, x, mean, rstd, gamma):
    """Backward of ``layer_norm_affine``: ``(dx, dgamma, dbeta)``."""
    dy, x, gamma = np.asarray(dy, F64), np.asarray(x, F64), np.asarray(gamma, F64)
    mean, rstd = np.asarray(mean, F64).reshape(-1, 1), np.asarray(rstd, F64).reshape(-1, 1)
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


# ------------------------------------------------------------------------------------------------ optimizer
def adamw_amsgrad_ema_step(p, g, m, v, vmax, ema, step, lr, betas, eps, weight_decay, clip=1.0, ema_one_minus_decay=0.0):
    """One step of ``torch.optim.AdamW(amsgrad=True)`` on the clipped gradient ``clip g`` followed by the EMA of the parameters
    (``s -= (1 - decay) (s - p)``, ema.py): ``step`` counts from 1.  Returns the new ``(p, m, v, vmax, ema)``; ``ema`` may be None."""
    p, g, m, v, vmax = (np.asarray(a, F64) for a in (p, g, m, v, vmax))
    b1, b2 = betas
    g = g * clip
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    vmax = np.maximum(vmax, v)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(vmax) / math.sqrt(bc2) + eps))
    if ema is not None:
        ema = np.asarray(ema, F64)
        ema = ema - ema_one_minus_decay * (ema - p)
    return p, m, v, vmax, ema


# ------------------------------------------------------------------------------------------------ bf16
def bf16_rne(bits):
    """float32 bit patterns (uint32) -> bfloat16 bit patterns (uint16), round to nearest, ties to even - the bits of
    ``torch.Tensor.bfloat16()``.  A NaN becomes the quiet NaN 0x7FC0 (torch writes that one or 0xFFFF, depending on the code path: NaNs are
    compared as NaNs, not bit for bit)."""
    b = np.asarray(bits, np.uint32).astype(np.uint64)
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def bf16_value_bits():
    """The float32 bit patterns the rounding tests feed: exact ties in both directions (tail 0x8000 behind an even and an odd kept bit),
    their neighbours, signed zeros and infinities, the largest finite float32 (rounds to inf), values around 1 and around 1e-30, and a
    seeded random fill.  No NaN and no subnormal: see ``bf16_nan_bits`` / ``bf16_subnormal_bits``."""
    spec = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,               # ties: even kept bit (down), odd kept bit (up), both signs
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,               # one ulp beside the ties
            0x3F7F8000, 0x3FFF8000, 0x7F7F8000,                           # ties that carry into the exponent; the last one rounds to inf
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,               # +-0, +-inf
            0x7F7FFFFF, 0xFF7FFFFF,                                       # largest finite float32 -> +-inf
            0x3F800000, 0x3F800001, 0x3F7FFFFF, 0x3F80FFFF, 0x3F810000,   # around 1
            0x00800000, 0x00808000, 0x00818000]                           # smallest normal and ties just above it
    around = np.concatenate([np.float32(1.0) + np.arange(-300, 300, dtype=np.float32) * np.float32(2.0 ** -17),
                             np.float32(1e-30) * (np.float32(1.0) + np.arange(-300, 300, dtype=np.float32) * np.float32(2.0 ** -17))])
    rng = np.random.default_rng(16)
    rand = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)
    rand = rand[((rand >> 23) & 0xFF != 0xFF) & ((rand >> 23) & 0xFF != 0)]                  # finite, normal
    ties = (rand & np.uint32(0xFFFF0000)) | np.uint32(0x8000)                                # random exact ties
    return np.concatenate([np.array(spec, np.uint32), around.astype(np.float32).view(np.uint32), rand, ties])


def bf16_nan_bits():
    return np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF, 0xFF808000], np.uint32)


def bf16_subnormal_bits():
    return np.array([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008000, 0x007F8000], np.uint32)
