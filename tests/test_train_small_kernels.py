"""GPU parity of the SMALL kernels of the training library, one entry point at a time, against the float64 yardstick of
tests/train_mirror.py (pinned on the CPU by tests/test_train_mirror_cpu.py): batch preparation, noising, Kabsch alignment and the loss;
time features and adjacency bits; BatchNorm and LayerNorm of the SpecFormer; sum of squares, AdamW + EMA and axpy of the optimizer; the
multi-piece copy and the bf16 packing of the weights.  tests/test_train_hip.py does the same for the block kernels; the whole-step tests
reach the kernels here with one batch, aligned padded buffers and a few hundred rows only, so every branch they cannot enter has a case
below: more than 64 BatchNorm chunks, the scratch clamp, B > 64, the scalar and the unaligned arms, tails that are no multiple of four,
rank-deficient covariances, batches with no pair or one pair.

The error measure is the suite's own (``tests.helpers.check``): max |got - ref| / max |ref|."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import train as otrain
from tests import train_mirror as M
from tests.helpers import check, relerr

pytestmark = pytest.mark.gpu

LAYOUTS = {"L_A": [3, 1, 7, 12, 29, 2],
           "L_B": [1],                                     # no pair at all
           "L_C": [1, 1, 2],                               # one pair
           "L_D": [1 + i % 29 for i in range(70)]}         # B > 64

BIG = float(np.float32(9e9))                               # fills outputs before a launch: what is still BIG was not written
_KEEP = []


def _dev(a, d, dtype=torch.float32):
    """``a`` (numpy or torch) on the device, kept alive until the module is done with it: a temporary passed as ``E._ptr(x.to(d))`` is freed
    as soon as ``_ptr`` returns and the caching allocator may hand its block to the next temporary before the kernel has read it."""
    x = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dtype).to(d).contiguous()
    _KEEP.append(x)
    if len(_KEEP) > 256:
        del _KEEP[:128]
    return x


def _np(t):
    return t.detach().cpu().double().numpy()


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _offset_view(n, d, fill=None, lead=1, guard=8):
    """A length-``n`` fp32 view that starts ``lead`` elements into a 16-byte aligned buffer (lead = 1: off the 16-byte grid), with ``guard``
    sentinel elements on both sides: (buffer, view)."""
    buf = torch.full((lead + n + guard + (4 - lead % 4),), -7.5, device=d)
    view = buf[lead:lead + n]
    if fill is not None:
        view.copy_(torch.as_tensor(fill, dtype=torch.float32))
    assert buf.data_ptr() % 16 == 0 and (n == 0 or (lead % 4 == 0) == (view.data_ptr() % 16 == 0))
    return buf, view


def _guards_intact(buf, view, lead=1):
    n = view.numel()
    b = buf.cpu()
    return bool((b[:lead] == -7.5).all()) and bool((b[lead + n:] == -7.5).all())


@pytest.fixture(scope="module")
def ops(gpu_device):
    from diffspectra_amd import engine as E, train_engine as T
    return E, T, T.Ops(gpu_device)


def _layout(T, d, n_atoms):
    from diffspectra_amd import filler
    node_mask, _ = filler.masks_from_n_atoms(n_atoms)
    return T.TrainLayout(node_mask, d)


def _schedule_ends(B, rng):
    """alpha_t, sigma_t of ``NoiseScheduleVP.marginal_prob`` at B times in [1e-5, 1], the two ends included where B allows."""
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    t = rng.uniform(0.02, 0.98, B).astype(np.float32)
    t[0] = 1e-5
    if B > 1:
        # t = 1 itself is no value of the float32 schedule: cos of the float32 pi / 2 is negative and marginal_prob(1.0) is NaN; the
        # trainer's t = rand (1 - 1e-5) + 1e-5 ends one ulp below it, at alpha = 1.9e-7, sigma = 1
        t[-1] = np.nextafter(np.float32(1.0), np.float32(0.0))
    a, s = NoiseScheduleVP("cosine").marginal_prob(torch.from_numpy(t))
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(s).all())
    return a.to(torch.float32).numpy(), s.to(torch.float32).numpy()


# ------------------------------------------------------------------------------------------------ batch preparation
def _raw_batch(n_atoms, rng):
    Nn = int(sum(n_atoms))
    Pp = int(sum(n * (n - 1) // 2 for n in n_atoms))
    pos = (rng.normal(size=(Nn, 3)) * 1.3 + np.array([37.5, -12.0, 3.0])).astype(np.float32)
    one_hot = np.eye(5, dtype=np.float32)[rng.integers(0, 5, Nn)]
    fc = rng.integers(-1, 2, Nn).astype(np.float32)
    order = rng.choice([0.0, 1.0, 2.0, 3.0], size=max(Pp, 1), p=[0.6, 0.2, 0.13, 0.07])
    edge = np.stack([(order > 0).astype(np.float32), (order / 3.0).astype(np.float32)], axis=1)
    return Nn, Pp, pos, one_hot, fc, edge


@pytest.mark.parametrize("factors", ["config", (2.5, 4.0, 8.0, 0.5)])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_prepare_batch(ops, gpu_device, name, factors):
    """dst_prepare_batch on positions far from the origin: x, ex within 3e-6 and the centre of mass of every molecule removed to 1e-6 of
    the position scale."""
    E, T, o = ops
    d = gpu_device
    if factors == "config":
        from diffspectra_amd.config import qm9s_config
        from diffspectra_amd.losses import _factors
        factors = tuple(float(v) for v in _factors(qm9s_config("ir")))
    n_atoms = LAYOUTS[name]
    TL = _layout(T, d, n_atoms)
    Nn, Pp, pos, one_hot, fc, edge = _raw_batch(n_atoms, np.random.default_rng(11))
    assert (TL.Nn, TL.Pp) == (Nn, Pp)
    x, ex = torch.full((Nn, 9), BIG, device=d), torch.full((max(Pp, 1), 2), BIG, device=d)
    E._check(o.lib.dst_prepare_batch(C.byref(TL.c), E._ptr(_dev(pos, d)), E._ptr(_dev(one_hot, d)), E._ptr(_dev(fc, d)), E._ptr(_dev(edge, d)),
                                     *(C.c_float(f) for f in factors), E._ptr(x), E._ptr(ex), E._stream()), "dst_prepare_batch")
    rx, rex = M.prepare_batch(n_atoms, pos, one_hot, fc, edge[:Pp], factors)
    worst = max(check(x[:, :3], _t(rx[:, :3]), 3e-6, "positions"), check(x[:, 3:], _t(rx[:, 3:]), 3e-6, "types and charges"))
    if Pp:
        worst = max(worst, check(ex[:Pp], _t(rex), 3e-6, "pair features"))
    else:
        assert float(ex.min()) == BIG                                     # no pair: nothing written
    scale = np.abs(rx[:, :3]).max()
    got = _np(x[:, :3])
    off, _ = M.offsets(n_atoms)
    com = max(np.abs(got[off[m]:off[m + 1]].mean(0)).max() for m in range(len(n_atoms)))
    print(f"[prepare_batch {name} {factors}] worst deviation {worst:.2e}; worst |centre of mass| / position scale {com / max(scale, 1e-30):.2e}")
    assert com <= 1e-6 * scale, (com, scale)


# ------------------------------------------------------------------------------------------------ noising
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_noising(ops, gpu_device, name):
    """dst_noising with alpha, sigma of both ends of the schedule: z, ez within 3e-6; the position noise free of its centre of mass (per
    molecule |mean over atoms of (z - alpha x)[:, :3]| <= 1e-6 sigma); the six feature columns taken as drawn.

    The centre-of-mass bound is held literally on a second launch with x = 0, where z IS sigma * noise.  With x != 0 the stored z carries
    its own float32 rounding, up to 2^-24 max |z| per element whatever the kernel does (at t = 1e-5, sigma = 6e-4, that alone is 400 x
    the bound), so there the bound is 1e-6 sigma plus that half ulp."""
    E, T, o = ops
    d = gpu_device
    n_atoms = LAYOUTS[name]
    B = len(n_atoms)
    TL = _layout(T, d, n_atoms)
    rng = np.random.default_rng(12)
    Nn, Pp, pos, one_hot, fc, edge = _raw_batch(n_atoms, rng)
    x, ex = M.prepare_batch(n_atoms, pos, one_hot, fc, edge[:Pp], (1.0, 4.0, 4.0, 1.0))
    x, ex = x.astype(np.float32), np.concatenate([ex, np.zeros((max(Pp, 1) - Pp, 2))]).astype(np.float32)
    raw = rng.normal(size=(Nn, 9)).astype(np.float32)
    raw[:, :3] += np.float32(0.75)                                        # a mean worth removing, also in a one-atom molecule
    eraw = rng.normal(size=(max(Pp, 1), 2)).astype(np.float32)
    alpha, sigma = _schedule_ends(B, rng)
    off, _ = M.offsets(n_atoms)
    mol = M.node_molecule(n_atoms)

    def run(xd):
        z, ez = torch.full((Nn, 9), BIG, device=d), torch.full((max(Pp, 1), 2), BIG, device=d)
        E._check(o.lib.dst_noising(C.byref(TL.c), E._ptr(_dev(alpha, d)), E._ptr(_dev(sigma, d)), E._ptr(_dev(xd, d)), E._ptr(_dev(raw, d)), E._ptr(z),
                                   E._ptr(_dev(ex, d)), E._ptr(_dev(eraw, d)), E._ptr(ez), E._stream()), "dst_noising")
        return z, ez

    def com(z, xd):                                                       # per molecule: max |mean over atoms of the position noise| / sigma
        e = _np(z)[:, :3] - alpha.astype(np.float64)[mol, None] * xd.astype(np.float64)[:, :3]
        return np.array([np.abs(e[off[m]:off[m + 1]].mean(0)).max() for m in range(B)]) / sigma.astype(np.float64)

    z, ez = run(x)
    rz, rez = M.noising(n_atoms, alpha, sigma, x, raw, ex[:Pp], eraw[:Pp])
    worst = check(z, _t(rz), 3e-6, "z")
    if Pp:
        worst = max(worst, check(ez[:Pp], _t(rez), 3e-6, "ez"))
    else:
        assert float(ez.min()) == BIG
    zmax = np.array([np.abs(_np(z)[off[m]:off[m + 1], :3]).max() for m in range(B)])
    c1 = com(z, x)
    assert (c1 <= 1e-6 + 2.0 ** -24 * zmax / sigma).all(), c1
    z0, _ = run(np.zeros_like(x))
    c0 = com(z0, np.zeros_like(x))
    assert (c0 <= 1e-6).all(), c0
    # the feature columns are not centred: sigma * raw as drawn (a centred one-atom molecule would have no feature noise at all)
    e6 = _np(z0)[:, 3:] / sigma.astype(np.float64)[mol, None]
    assert np.abs(e6 - raw[:, 3:].astype(np.float64)).max() <= 3e-6 * np.abs(raw[:, 3:]).max()
    feat_mean = np.array([np.abs(e6[off[m]:off[m + 1]].mean(0)).max() for m in range(B)])
    assert (feat_mean > 1e-3).all(), feat_mean
    print(f"[noising {name}] worst deviation {worst:.2e}; noise centre of mass / sigma {c0.max():.2e} (x = 0), {c1.max():.2e} (x != 0)")


# ------------------------------------------------------------------------------------------------ Kabsch
@pytest.mark.parametrize("ld", [9, 3])
def test_kabsch(ops, gpu_device, ld):
    """dst_kabsch on one batch that holds every case class of ``train_mirror.kabsch_cases`` (rank 0, 1, 2 covariances, three equal
    singular values, identity, reflection, both ends of the schedule at n = 29, 20 random), with the trainer's 9-column operands and
    with 3-column ones.  The aligned target is compared in EVERY case at 1e-6 of max |tar| (it is unique even where the rotation is not:
    the target then lies in the span of the leading right singular vectors).  The rotation is compared, and must be orthonormal with
    determinant +1, to 1e-6 where the mirror's s3 >= 1e-6 s1 (below that sign det A is rounding noise in any precision; where the rank is 2
    the kernel must still return the one proper rotation of the fit, ``train_mirror.proper_rotation``); before it
    compares, the test asserts that the case determines its rotation well: (s2 + sign(det) s3) / s1 >= 0.05, so an SVD in float64 plus
    the float32 rounding of the nine entries stays far below 1e-6."""
    E, T, o = ops
    d = gpu_device
    cs = M.kabsch_cases()
    n_atoms = [len(t) for _, _, t in cs]
    TL = _layout(T, d, n_atoms)
    pred, tar = np.concatenate([p for _, p, _ in cs]), np.concatenate([t for _, _, t in cs])
    rng = np.random.default_rng(13)
    wide = lambda a: np.concatenate([a, rng.normal(size=(len(a), ld - 3)).astype(np.float32)], axis=1) if ld > 3 else a
    rot, aligned = torch.full((len(cs), 9), BIG, device=d), torch.full((TL.Nn, 3), BIG, device=d)
    E._check(o.lib.dst_kabsch(C.byref(TL.c), E._ptr(_dev(wide(pred), d)), C.c_int64(ld), E._ptr(_dev(wide(tar), d)), C.c_int64(ld), E._ptr(rot),
                              E._ptr(aligned), E._stream()), "dst_kabsch")
    r_rot, r_al, S = M.kabsch_align(n_atoms, pred, tar)
    rot, aligned = _np(rot).reshape(-1, 3, 3), _np(aligned)
    off, _ = M.offsets(n_atoms)
    worst_al = worst_rot = 0.0
    compared, rank2, gap_min = 0, 0, np.inf
    for m, (name, p, t) in enumerate(cs):
        sl = slice(off[m], off[m + 1])
        e_al = np.abs(aligned[sl] - r_al[sl]).max()
        assert e_al <= 1e-6 * np.abs(t).max(), (name, e_al)
        worst_al = max(worst_al, e_al / (np.abs(t).max() + 1e-30))
        if S[m, 0] > 0 and S[m, 2] >= 1e-6 * S[m, 0]:
            gap = (S[m, 1] + M.det_sign(p, t) * S[m, 2]) / S[m, 0]
            assert gap >= 0.05, (name, S[m])
            gap_min = min(gap_min, gap)
            e_rot = np.abs(rot[m] - r_rot[m]).max()
            assert e_rot <= 1e-6, (name, e_rot)
            assert np.abs(rot[m] @ rot[m].T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(rot[m]) - 1.0) <= 1e-6, name
            worst_rot = max(worst_rot, e_rot)
            compared += 1
        elif S[m, 0] > 0 and S[m, 1] >= 0.05 * S[m, 0]:
            # rank 2 (three atoms, a planar ring): sign det A is noise, but the fit still has ONE proper rotation and the kernel returns it
            e_rot = np.abs(rot[m] - M.proper_rotation(p, t)).max()
            assert e_rot <= 1e-6 and abs(np.linalg.det(rot[m]) - 1.0) <= 1e-6, (name, e_rot)
            worst_rot = max(worst_rot, e_rot)
            rank2 += 1
    assert compared >= 24 and rank2 >= 3                                  # full rank: tetrahedron, identical, mirror image, 2 x n29, 19 random
    print(f"[kabsch ld={ld}] aligned: worst |diff| / max |tar| {worst_al:.2e}; rotation: worst |diff| {worst_rot:.2e} over {compared} cases, "
          f"smallest (s2 +- s3) / s1 {gap_min:.3f}")


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("weights", [(1.0, 0.25, 0.1), (0.3, 2.0, 1.7)])
@pytest.mark.parametrize("name", ["L_A", "L_C", "L_D"])
def test_loss(ops, gpu_device, name, weights):
    """dst_loss against float64 autograd of the mirror: loss per molecule to rtol 1e-5, the three gradients to 2e-5; on L_A the sum over
    the molecules equals ``oracle.train.loss_from_predictions`` on the unpacked dense tensors (packed and dense conventions agree)."""
    E, T, o = ops
    d = gpu_device
    n_atoms = LAYOUTS[name]
    B = len(n_atoms)
    TL = _layout(T, d, n_atoms)
    Nn, Pp = TL.Nn, TL.Pp
    rng = np.random.default_rng(14)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    pos, feat, edge, tpos, tfeat, tedge = f(Nn, 3), f(Nn, 6) * 0.4, f(Pp, 2), f(Nn, 3), f(Nn, 6) * 0.4, f(Pp, 2)
    alpha, sigma = _schedule_ends(B, rng)
    wm = (np.sqrt(alpha / sigma) / np.float32(B)).astype(np.float32)      # a different weight per molecule, as the trainer forms it
    loss_m, dpos, dfeat, dedge = (torch.full(s, BIG, device=d) for s in ((B,), (Nn, 3), (Nn, 6), (Pp, 2)))
    E._check(o.lib.dst_loss(C.byref(TL.c), *(E._ptr(_dev(a, d)) for a in (pos, feat, edge, tpos, tfeat, tedge, wm)),
                            *(C.c_float(w) for w in weights), E._ptr(loss_m), E._ptr(dpos), E._ptr(dfeat), E._ptr(dedge), E._stream()), "dst_loss")
    r_loss, r_dpos, r_dfeat, r_dedge = M.loss_and_grads(n_atoms, pos, feat, edge, tpos, tfeat, tedge, wm, weights)
    e_loss = np.abs(_np(loss_m) - r_loss) / np.abs(r_loss)
    assert (e_loss <= 1e-5).all(), e_loss.max()
    worst = max(check(dpos, _t(r_dpos), 2e-5, "dpos"), check(dfeat, _t(r_dfeat), 2e-5, "dfeat"), check(dedge, _t(r_dedge), 2e-5, "dedge"))
    print(f"[loss {name} {weights}] loss per molecule: worst relative deviation {e_loss.max():.2e}; gradients {worst:.2e}")
    if name == "L_A":
        pred = _t(M.unpack_nodes(np.concatenate([pos, feat], 1), n_atoms))
        xh = _t(M.unpack_nodes(np.concatenate([tpos, tfeat], 1), n_atoms))
        dense = otrain.loss_from_predictions(pred, _t(M.unpack_pairs(edge, n_atoms)), xh, _t(M.unpack_pairs(tedge, n_atoms)),
                                             _t(M.unpack_nodes(tpos, n_atoms)), _t(alpha), _t(sigma), weights)
        assert abs(float(loss_m.double().sum()) - float(dense)) <= 1e-5 * abs(float(dense))


# ------------------------------------------------------------------------------------------------ time features
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_time_feat(ops, gpu_device, B):
    """dst_time_feat_fwd / _bwd at noise levels in [-12, 12] and the frequencies' shipped scale; the mirror forms the argument
    ((x w) 2) pi in float32 in the kernel's order and takes sine and cosine in float64, so the comparison measures the kernel and not the
    rounding of an argument of size 100.  Features 3e-6 (the noise-level column bit for bit), dw 2e-5."""
    from diffspectra_amd import filler
    E, T, o = ops
    d = gpu_device
    rng = np.random.default_rng(15 + B)
    nl = rng.uniform(-12.0, 12.0, B).astype(np.float32)
    nl[0] = 12.0
    nl[-1] = -12.0 if B > 1 else 12.0
    w = filler.fill_tensor("time_mlp.0.weights", (8,)).numpy()
    df = rng.normal(size=(B, 17)).astype(np.float32)
    f, dw = torch.full((B, 17), BIG, device=d), torch.full((8,), BIG, device=d)
    nld, wd = _dev(nl, d), _dev(w, d)
    E._check(o.lib.dst_time_feat_fwd(E._ptr(nld), E._ptr(wd), C.c_int32(B), E._ptr(f), E._stream()), "dst_time_feat_fwd")
    E._check(o.lib.dst_time_feat_bwd(E._ptr(nld), E._ptr(wd), E._ptr(_dev(df, d)), C.c_int32(B), E._ptr(dw), E._stream()), "dst_time_feat_bwd")
    rf = M.time_feat(nl, w)
    assert np.array_equal(_np(f)[:, 0], rf[:, 0])
    e_f = check(f[:, 1:], _t(rf[:, 1:]), 3e-6, "sin / cos features")
    e_w = check(dw, _t(M.time_feat_weight_grad(nl, w, df)), 2e-5, "dw")
    print(f"[time_feat B={B}] features {e_f:.2e}, dw {e_w:.2e}")


# ------------------------------------------------------------------------------------------------ adjacency bits
@pytest.mark.parametrize("Pp", [1, 255, 256, 257, 1000])
def test_adj_bits(ops, gpu_device, Pp):
    """dst_adj_bits with ld = 2 on values exactly at edge_th and at the cut-off, one ulp below and one ulp above: integer equality."""
    E, T, o = ops
    d = gpu_device
    rng = np.random.default_rng(16 + Pp)
    for th, cut in ((0.0, 2.0), (0.5, 1.7)):                              # the configuration's thresholds, and a pair off the float32 grid
        th32, cut32 = np.float32(th), np.float32(cut)
        edges = np.array([th32, np.nextafter(th32, np.float32(-9)), np.nextafter(th32, np.float32(9)), -th32 if th else np.float32(-0.0)], np.float32)
        dists = np.array([cut32, np.nextafter(cut32, np.float32(0)), np.nextafter(cut32, np.float32(9)), 0.0], np.float32)
        ce = rng.normal(size=(Pp, 2)).astype(np.float32)
        d2 = rng.uniform(0.0, 4.0, Pp).astype(np.float32)
        k = np.arange(Pp)
        sel = rng.random(Pp) < 0.5 if Pp > 1 else np.array([True])
        ce[sel, 0] = edges[k[sel] % 4]
        d2[sel] = dists[(k[sel] // 4) % 4]
        ce[:, 1] = np.where(ce[:, 0] >= th32, -5.0, 5.0)                  # column 1 says the opposite: a wrong stride shows
        adj = torch.full((Pp + 3,), -9, dtype=torch.int32, device=d)
        E._check(o.lib.dst_adj_bits(E._ptr(_dev(ce, d)), C.c_int64(2), E._ptr(_dev(d2, d)), C.c_float(th), C.c_float(cut), C.c_int32(Pp), E._ptr(adj),
                                    E._stream()), "dst_adj_bits")
        got = adj.cpu().numpy()
        assert np.array_equal(got[:Pp], M.adj_bits(ce[:, 0], d2, th, cut)) and (got[Pp:] == -9).all(), (Pp, th, cut)
    print(f"[adj_bits Pp={Pp}] equal")


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_run(E, o, d, x, dy, gamma, beta, rm0, rv0, cap_f=None, cap_b=None):
    """dst_bn_fwd + dst_bn_running_again + dst_bn_bwd on scratch buffers of exactly the stated capacity (guarded): every output on the CPU."""
    R, Cc = x.shape
    cap_f, cap_b = cap_f or 4096 * Cc, cap_b or 2 * 4096 * Cc
    scratch = torch.full((max(cap_f, cap_b) + 64,), -7.5, device=d)
    xd, dyd, gd, bd = _dev(x, d), _dev(dy, d), _dev(gamma, d), _dev(beta, d)
    y, stats = torch.full((R, Cc), BIG, device=d), torch.full((3, Cc), BIG, device=d)
    rm, rv = (None, None) if rm0 is None else (_dev(rm0, d).clone(), _dev(rv0, d).clone())
    E._check(o.lib.dst_bn_fwd(E._ptr(xd), C.c_int32(R), C.c_int32(Cc), E._ptr(gd), E._ptr(bd), C.c_float(1e-5), E._ptr(y), E._ptr(stats), E._ptr(rm),
                              E._ptr(rv), E._ptr(scratch), C.c_int64(cap_f), E._stream()), "dst_bn_fwd")
    assert bool((scratch[cap_f:] == -7.5).all())
    if rm is not None:
        E._check(o.lib.dst_bn_running_again(E._ptr(stats), C.c_int32(Cc), E._ptr(rm), E._ptr(rv), E._stream()), "dst_bn_running_again")
    scratch.fill_(-7.5)
    dx, dgamma, dbeta = torch.full((R, Cc), BIG, device=d), torch.full((Cc,), BIG, device=d), torch.full((Cc,), BIG, device=d)
    E._check(o.lib.dst_bn_bwd(E._ptr(dyd), E._ptr(xd), E._ptr(stats), C.c_int32(R), C.c_int32(Cc), E._ptr(gd), E._ptr(dx), E._ptr(dgamma), E._ptr(dbeta),
                              E._ptr(scratch), C.c_int64(cap_b), E._stream()), "dst_bn_bwd")
    assert bool((scratch[cap_b:] == -7.5).all())
    return dict(y=y, mean=stats[0], rstd=stats[1], unbiased=stats[2], rm=rm, rv=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _bn_reference(x, dy, gamma, beta, rm0, rv0):
    y, mean, rstd, unb, rm1, rv1 = M.batch_norm_train(x, gamma, beta, 1e-5, rm0, rv0)
    rm2 = rv2 = None
    if rm0 is not None:
        _, _, _, _, rm2, rv2 = M.batch_norm_train(x, gamma, beta, 1e-5, rm1, rv1)      # the second training-mode pass over the same batch
    dx, dgamma, dbeta = M.batch_norm_backward(dy, x, mean, rstd, gamma)
    return dict(y=y, mean=mean, rstd=rstd, unbiased=unb, rm=rm2, rv=rv2, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _bn_data(R, Cc, seed, mean=None, std=None):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-1.0, 1.0, Cc) if mean is None else np.full(Cc, mean)
    sd = rng.uniform(0.5, 2.0, Cc) if std is None else np.full(Cc, std)
    x = (rng.normal(size=(R, Cc)) * sd + mu).astype(np.float32)
    if R == 2:
        # Two rows x = mu +- d: y and dx depend on d alone, but the kernel (like any BatchNorm that keeps float32 statistics) takes d from
        # x - fl(mean), and fl(mean) is off by up to t = 2^-24 |mean|.  y feels that as t eps / (d^2 + eps)^1.5, and dx, a cancellation that
        # keeps eps / (d^2 + eps) of its terms, as (t / d) (d^2 + eps) / eps of its value - at best 632 t, at d = sqrt(eps).  Measured on plain
        # draws with |mean| <= 1: y 5.3e-6 where one channel had d = 0.003; dx 2.9e-3 with every d >= 0.5 (1e-5 of its terms left) and
        # 3.9e-5 with d from [0.01, 2].  So the bounds of this file can hold only for small means: |mean| <= 0.1 (t <= 3.7e-9), d drawn
        # log-uniformly from [0.01, 2] with channel 0 at 0.01, which gives 3e-8 on y and 4e-6 on dx in the worst channel.
        mu = rng.uniform(-0.1, 0.1, Cc)
        half = np.exp(rng.uniform(np.log(0.01), np.log(2.0), Cc))
        half[0] = 0.01
        x = (mu + np.stack([half, -half]) * rng.choice([-1.0, 1.0], Cc)).astype(np.float32)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return x, f(R, Cc), rng.uniform(0.8, 1.2, Cc).astype(np.float32), f(Cc) * 0.1, f(Cc), rng.uniform(0.5, 2.0, Cc).astype(np.float32)


BN_TOL = dict(y=3e-6, mean=3e-6, rstd=3e-6, unbiased=3e-6, rm=3e-6, rv=3e-6, dx=2e-5, dgamma=1e-5, dbeta=1e-5)


@pytest.mark.parametrize("R,Cc,clamp,running", [(2, 128, False, True), (130, 128, False, True), (130, 128, False, False), (300, 70, False, True),
                                                 (8321, 128, False, True),      # 66 chunks: more than one pass of the 64-lane chunk sum
                                                 (1000, 128, True, True)])      # scratch for 3 chunks: the clamp arm
def test_batch_norm(ops, gpu_device, R, Cc, clamp, running):
    """dst_bn_fwd -> dst_bn_running_again -> dst_bn_bwd: y, mean, rstd, unbiased variance, both running statistics (started from random
    values, after the two updates) to 3e-6, dx to 2e-5, dgamma and dbeta to 1e-5; once without running statistics."""
    E, T, o = ops
    x, dy, gamma, beta, rm0, rv0 = _bn_data(R, Cc, 17 + R)
    if not running:
        rm0 = rv0 = None
    got = _bn_run(E, o, gpu_device, x, dy, gamma, beta, rm0, rv0, *((3 * Cc, 6 * Cc) if clamp else ()))
    ref = _bn_reference(x, dy, gamma, beta, rm0, rv0)
    errs = {k: check(got[k], _t(ref[k]), BN_TOL[k], k) for k in BN_TOL if ref[k] is not None}
    print(f"[batch_norm {R}x{Cc}{' clamp' if clamp else ''}] " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))


def test_batch_norm_large_mean(ops, gpu_device):
    """(130, 128) with mean 50 and standard deviation 0.1 per channel: the variance is 4e-6 of the second moment.  No bound is fixed in
    advance: per quantity, torch's own float32 CPU batch_norm (and its backward) is measured against the float64 mirror on the same input
    and the kernel is allowed four times that (another summation order), but never less than one float32 ulp of the largest reference
    value.  Measured on an MI355X: y torch 1.3e-05, kernel 1.6e-05; dx torch 3.6e-06, kernel 4.4e-06; dgamma torch 1.6e-05, kernel 2.6e-05
    (every other quantity at 1e-7 on both sides)."""
    E, T, o = ops
    R, Cc = 130, 128
    x, dy, gamma, beta, rm0, rv0 = _bn_data(R, Cc, 18, mean=50.0, std=0.1)
    got = _bn_run(E, o, gpu_device, x, dy, gamma, beta, rm0, rv0)
    ref = _bn_reference(x, dy, gamma, beta, rm0, rv0)
    t = lambda a: torch.from_numpy(a.copy())
    rm, rv = t(rm0), t(rv0)
    ty, tmean, trstd = torch.native_batch_norm(t(x), t(gamma), t(beta), rm, rv, True, 0.1, 1e-5)
    torch.native_batch_norm(t(x), t(gamma), t(beta), rm, rv, True, 0.1, 1e-5)
    tdx, tdg, tdb = torch.ops.aten.native_batch_norm_backward(t(dy), t(x), t(gamma), rm, rv, tmean, trstd, True, 1e-5, [True, True, True])
    own = dict(y=ty, mean=tmean, rstd=trstd, rm=rm, rv=rv, dx=tdx, dgamma=tdg, dbeta=tdb)
    line = []
    for k, tv in own.items():
        e_torch = relerr(tv, _t(ref[k]))
        e = check(got[k], _t(ref[k]), max(4.0 * e_torch, 2.0 ** -23), k)
        line.append(f"{k} torch {e_torch:.1e} kernel {e:.1e}")
    print("[batch_norm mean 50, std 0.1] " + "; ".join(line))


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("R,Cc", [(1, 256), (6, 256), (300, 256), (5, 70), (3, 64), (7, 100)])
def test_layer_norm_affine(ops, gpu_device, R, Cc):
    """dst_ln_affine_fwd / _bwd with the eps spec_train.py passes: y, mean, rstd 3e-6, dx 2e-5, dgamma and dbeta 1e-5."""
    E, T, o = ops
    d = gpu_device
    rng = np.random.default_rng(19 + R + Cc)
    x = (rng.normal(size=(R, Cc)) * 2.0 + rng.uniform(-1, 1, (R, 1))).astype(np.float32)
    dy = rng.normal(size=(R, Cc)).astype(np.float32)
    gamma, beta = rng.uniform(0.8, 1.2, Cc).astype(np.float32), (rng.normal(size=Cc) * 0.1).astype(np.float32)
    xd, dyd, gd = _dev(x, d), _dev(dy, d), _dev(gamma, d)
    y, stats = torch.full((R, Cc), BIG, device=d), torch.full((R, 2), BIG, device=d)
    E._check(o.lib.dst_ln_affine_fwd(E._ptr(xd), C.c_int32(R), C.c_int32(Cc), E._ptr(gd), E._ptr(_dev(beta, d)), C.c_float(1e-5), E._ptr(y),
                                     E._ptr(stats), E._stream()), "dst_ln_affine_fwd")
    dx, dgamma, dbeta = torch.full((R, Cc), BIG, device=d), torch.full((Cc,), BIG, device=d), torch.full((Cc,), BIG, device=d)
    E._check(o.lib.dst_ln_affine_bwd(E._ptr(dyd), E._ptr(xd), E._ptr(stats), C.c_int32(R), C.c_int32(Cc), E._ptr(gd), E._ptr(dx), E._ptr(dgamma),
                                     E._ptr(dbeta), E._stream()), "dst_ln_affine_bwd")
    ry, rmean, rrstd = M.layer_norm_affine(x, gamma, beta, 1e-5)
    rdx, rdg, rdb = M.layer_norm_backward(dy, x, rmean, rrstd, gamma)
    e = [check(y, _t(ry), 3e-6, "y"), check(stats[:, 0], _t(rmean), 3e-6, "mean"), check(stats[:, 1], _t(rrstd), 3e-6, "rstd"),
         check(dx, _t(rdx), 2e-5, "dx"), check(dgamma, _t(rdg), 1e-5, "dgamma"), check(dbeta, _t(rdb), 1e-5, "dbeta")]
    print(f"[layer_norm {R}x{Cc}] y {e[0]:.1e}, mean {e[1]:.1e}, rstd {e[2]:.1e}, dx {e[3]:.1e}, dgamma {e[4]:.1e}, dbeta {e[5]:.1e}")


# ------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("n,lead", [(0, 0), (1, 0), (3, 0), (255, 0), (262149, 0), (1000003, 0), (262149, 1), (1000003, 1)])
def test_sumsq(ops, gpu_device, n, lead):
    """dst_sumsq, overwrite and accumulate, to 2e-6: lengths with a tail behind the last full quad, more than one grid pass (262 149 =
    256 x 256 x 4 + 5), and a view one element into the buffer (the unaligned arm)."""
    E, T, o = ops
    d = gpu_device
    x = np.random.default_rng(20 + n).normal(size=n).astype(np.float32)
    buf, view = _offset_view(n, d, x, lead=lead)
    assert n == 0 or (view.data_ptr() % 16 != 0) == bool(lead)              # (an empty tensor has no address at all: n = 0 passes NULL)
    scratch = torch.zeros(1024, device=d)
    ref = float(np.square(x.astype(np.float64)).sum())
    worst = 0.0
    for acc, start in ((0, 123.0), (1, 2.5)):
        out = torch.full((3,), start, device=d)
        E._check(o.lib.dst_sumsq(E._ptr(view), C.c_int64(n), E._ptr(out[1:]), C.c_int32(acc), E._ptr(scratch), C.c_int64(scratch.numel()), E._stream()),
                 "dst_sumsq")
        got = out.cpu().double()
        want = ref + (start if acc else 0.0)
        assert float(got[0]) == start and float(got[2]) == start
        assert abs(float(got[1]) - want) <= 2e-6 * want if n else float(got[1]) == want, (n, lead, acc, float(got[1]), want)
        worst = max(worst, abs(float(got[1]) - want) / max(want, 1e-30))
    print(f"[sumsq n={n} lead={lead}] worst relative deviation {worst:.2e}")


@pytest.mark.parametrize("n,lead", [(1, 0), (5, 0), (1024, 0), (1024, 1), (1027, 0)])
def test_adamw_ema(ops, gpu_device, n, lead):
    """dst_adamw_ema, three consecutive steps with fresh gradients, weight decay and betas (0.9, 0.999): p, m, v, vmax and ema within 2e-6
    of the float64 mirror after every step - on aligned buffers (the float4 kernel where n is a multiple of four), on views one element
    off the 16-byte grid and on lengths with a tail (the scalar kernel); with and without EMA; with the clip coefficient from the host
    alone and times a device scalar."""
    E, T, o = ops
    d = gpu_device
    lr, b1, b2, eps, wd, omd = 2e-3, 0.9, 0.999, 1e-8, 0.03, 0.004
    worst = 0.0
    for with_ema in (True, False):
        for dev_clip in (False, True):
            rng = np.random.default_rng(21 + n + lead)
            start = [rng.normal(size=n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32),
                     rng.normal(size=n).astype(np.float32)]
            bufs = [_offset_view(n, d, a, lead=lead) for a in start]
            gbuf, gview = _offset_view(n, d, lead=lead)
            ref = [a.astype(np.float64) for a in start]
            if not with_ema:
                ref[4] = None
            clip_dev = torch.tensor([0.37], device=d) if dev_clip else None
            for step in (1, 2, 3):
                g = (rng.normal(size=n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
                gview.copy_(torch.from_numpy(g))
                host_clip = 0.5 if step == 2 else 1.0
                E._check(o.lib.dst_adamw_ema(E._ptr(bufs[0][1]), E._ptr(gview), E._ptr(bufs[1][1]), E._ptr(bufs[2][1]), E._ptr(bufs[3][1]),
                                             E._ptr(bufs[4][1]) if with_ema else None, C.c_int64(n), C.c_float(lr), C.c_double(b1), C.c_double(b2),
                                             C.c_float(eps), C.c_float(wd), C.c_float(1.0 - b1 ** step), C.c_float(1.0 - b2 ** step), C.c_float(host_clip),
                                             E._ptr(clip_dev), C.c_float(omd), E._stream()), "dst_adamw_ema")
                clip = host_clip * (float(np.float32(0.37)) if dev_clip else 1.0)
                ref = list(M.adamw_amsgrad_ema_step(ref[0], g, *ref[1:], step, lr, (b1, b2), eps, wd, clip, omd))
                for k, what in enumerate(("p", "m", "v", "vmax", "ema")):
                    if ref[k] is not None:
                        worst = max(worst, check(bufs[k][1], _t(ref[k]), 2e-6, f"{what} after step {step} (ema {with_ema}, device clip {dev_clip})"))
            if not with_ema:
                assert torch.equal(bufs[4][1].cpu(), torch.from_numpy(start[4]))                 # no EMA pointer: nothing of it is touched
            assert all(_guards_intact(b, v, lead) for b, v in bufs + [(gbuf, gview)])
    print(f"[adamw_ema n={n} lead={lead}] worst deviation {worst:.2e}")


@pytest.mark.parametrize("n,lead", [(0, 0), (1, 0), (5, 0), (1024, 0), (1024, 1), (1027, 0)])
def test_axpy(ops, gpu_device, n, lead):
    """dst_axpy (through Ops.axpy) on the same aligned / offset / tail cases plus the empty one, to 1e-6."""
    E, T, o = ops
    d = gpu_device
    rng = np.random.default_rng(22 + n)
    x, y = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    (xb, xv), (yb, yv) = _offset_view(n, d, x, lead=lead), _offset_view(n, d, y, lead=lead)
    o.axpy(-1.75, xv, yv)
    assert _guards_intact(yb, yv, lead) and _guards_intact(xb, xv, lead)
    if n:
        e = check(yv, _t(y.astype(np.float64) - 1.75 * x.astype(np.float64)), 1e-6, "y")
        print(f"[axpy n={n} lead={lead}] {e:.2e}")


# ------------------------------------------------------------------------------------------------ weight staging
SENTINEL = -12345.0


def _guarded(shape, d, window=None):
    """A destination of ``shape`` inside a sentinel-filled buffer: contiguous (32 guard elements on both sides, 16-byte aligned) or, with
    ``window = (total columns, first column)``, a column window of a wider matrix with a guard row above and below."""
    if window is None:
        n = int(np.prod(shape))
        buf = torch.full((n + 64,), SENTINEL, device=d)
        return buf, buf[32:32 + n].view(*shape)
    buf = torch.full((shape[0] + 2, window[0]), SENTINEL, device=d)
    return buf, buf[1:-1, window[1]:window[1] + shape[1]]


def test_copy_pieces(ops, gpu_device):
    """dst_copy_pieces through ``train_engine.copy_pieces``: one launch whose pieces take different arms - 16-byte pieces, odd widths,
    column windows of wider tensors in both directions, a vector, a single element.  Exact, and no byte outside a destination changes."""
    E, T, o = ops
    d = gpu_device
    g = torch.Generator().manual_seed(23)
    r = lambda *s: torch.randn(*s, generator=g).to(d)
    wide70, wide72 = r(300, 70), r(40, 72)
    src = [r(64, 1024), r(300, 257), wide70[:, 3:67], r(300, 64), wide72[:, 4:68], r(5), r(1, 1)]
    spec = [((64, 1024), None), ((300, 257), None), ((300, 64), None), ((300, 64), (70, 3)), ((40, 64), (72, 4)), ((5,), None), ((1, 1), None)]
    made = [_guarded(shape, d, window) for shape, window in spec]
    dst = [v for _, v in made]
    T.copy_pieces(o.lib, d, dst, src, {}, "test")
    torch.cuda.synchronize()
    for k, ((buf, v), s) in enumerate(zip(made, src)):
        assert torch.equal(v, s), k
        mask = torch.ones_like(buf, dtype=torch.bool)
        if spec[k][1] is None:
            mask[32:32 + v.numel()] = False
        else:
            mask[1:-1, spec[k][1][1]:spec[k][1][1] + v.shape[1]] = False
        assert bool((buf[mask] == SENTINEL).all()), k
    print("[copy_pieces] 7 pieces equal, surroundings untouched")


def test_pack_bf16_pieces(ops, gpu_device):
    """dst_pack_bf16_pieces through ``train_engine.pack_bf16_pieces``, plain and transposed destinations in one launch: bit for bit the
    round-to-nearest-even of ``train_mirror.bf16_rne`` on exact ties in both directions, signed zeros and infinities, the largest finite
    float32, values around 1 and around 1e-30; a NaN stays a NaN; float32 subnormals are printed, not asserted (whether a conversion
    flushes them is the hardware's choice)."""
    E, T, o = ops
    d = gpu_device
    vals, nans, subs = M.bf16_value_bits(), M.bf16_nan_bits(), M.bf16_subnormal_bits()
    shapes = [(64, 256), (3, 5), (257, 70)]
    src_bits, kinds = [], []
    for k, (R, Cc) in enumerate(shapes):
        n = R * Cc
        bits = np.resize(np.roll(vals, -37 * k), n).copy()               # the value list, cycled; every piece starts elsewhere in it
        kind = np.zeros(n, np.int8)
        if n > 64:                                                       # NaNs and subnormals at known places, not in the first or last row only
            at = np.linspace(1, n - 2, len(nans) + len(subs)).astype(np.int64)
            bits[at[:len(nans)]], kind[at[:len(nans)]] = nans, 1
            bits[at[len(nans):]], kind[at[len(nans):]] = subs, 2
        src_bits.append(bits.reshape(R, Cc))
        kinds.append(kind.reshape(R, Cc))
    srcs = [torch.from_numpy(b.view(np.float32).copy()).to(d) for b in src_bits]
    src, made, key_t = [], [], set()
    sent = torch.tensor(SENTINEL).bfloat16()
    for k, (R, Cc) in enumerate(shapes):
        for transposed in (False, True):
            rows, cols = (Cc, R) if transposed else (R, Cc)
            buf = torch.full((rows + 2, cols + 6), float(sent), dtype=torch.bfloat16, device=d)
            if transposed:
                key_t.add(len(src))
            src.append(srcs[k])
            made.append((buf, buf[1:-1, 3:3 + cols], k, transposed))
    T.pack_bf16_pieces(o.lib, d, [m[1] for m in made], src, {}, "test", key_t=key_t)
    torch.cuda.synchronize()
    is_nan = lambda h: ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)
    seen_sub = {}
    for buf, view, k, transposed in made:
        got = view.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
        got = got.T if transposed else got
        want, kind = M.bf16_rne(src_bits[k]), kinds[k]
        plain = kind == 0
        assert np.array_equal(got[plain], want[plain]), (k, transposed, [(hex(s), hex(a), hex(b)) for s, a, b in
                                                                         zip(src_bits[k][plain & (got != want)][:6], got[plain & (got != want)][:6],
                                                                             want[plain & (got != want)][:6])])
        assert is_nan(got[kind == 1]).all(), (k, transposed)
        for s, a, b in zip(src_bits[k][kind == 2], got[kind == 2], want[kind == 2]):
            seen_sub[hex(s)] = (hex(a), hex(b))
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[1:-1, 3:3 + view.shape[1]] = False
        assert bool((buf[mask] == sent.to(d)).all()), (k, transposed)
    print(f"[pack_bf16_pieces] {sum(int((k == 0).sum()) for k in kinds) * 2} values bit-exact, NaNs stay NaN; subnormal inputs "
          f"(input: (kernel, round-to-nearest-even)): {seen_sub}")
