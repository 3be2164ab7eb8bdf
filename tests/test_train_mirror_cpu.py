"""The yardstick of the small training kernels (tests/train_mirror.py) pinned on the CPU, so that the GPU tests do not compare the kernels
with a second opinion nobody checked: the loss side reproduces golden G13 (the reference's own tensors of one ``loss_fn`` call), the norms
and the optimizer agree with torch's float64 implementations, the bf16 rounding with ``Tensor.bfloat16()`` bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import schedule
from oracle import train as otrain
from tests import train_mirror as M
from tests.golden import cases

TAG = "ir_selfcond"


def _g13_packed():
    """The G13 batch and draws, packed: what the trainer hands its kernels."""
    n_atoms = cases.TRAIN_ATOMS
    batch, draws = cases.training_batch("ir"), cases.training_draws()
    pos, oh = M.pack_nodes(batch["positions"].numpy(), n_atoms), M.pack_nodes(batch["atom_one_hot"].numpy(), n_atoms)
    fc = M.pack_nodes(batch["formal_charges"].numpy(), n_atoms).reshape(-1)
    edge = M.pack_pairs(batch["edge_one_hot"].numpy(), n_atoms)
    raw = M.pack_nodes(np.concatenate([draws["randn"][0].numpy(), draws["randn"][1].numpy()], axis=2), n_atoms)
    eraw = M.pack_pairs(draws["randn"][2].permute(0, 2, 3, 1).numpy(), n_atoms, lower=True)      # the tril(-1) draw of the pair
    t = draws["t_raw"] * (1.0 - 1e-5) + 1e-5
    alpha, sigma = schedule.marginal_prob(t)
    return n_atoms, pos, oh, fc, edge, raw, eraw, alpha.numpy(), sigma.numpy()


def test_loss_side_reproduces_golden_g13():
    """prepare_batch -> noising -> kabsch_align -> loss_and_grads on the G13 batch against the reference's stored xh, edge_x, z_t,
    edge_z_t, align_pos, rotations (n >= 3) and loss, at the tolerances tests/test_train_oracle.py holds the oracle to."""
    g = cases.load_npz("g13_training.npz")
    n_atoms, pos, oh, fc, edge, raw, eraw, alpha, sigma = _g13_packed()
    x, ex = M.prepare_batch(n_atoms, pos, oh, fc, edge, (1.0, 4.0, 4.0, 1.0))
    z, ez = M.noising(n_atoms, alpha, sigma, x, raw, ex, eraw)
    rot, aligned, sing = M.kabsch_align(n_atoms, z[:, :3], x[:, :3])
    gold = lambda k: g[f"{TAG}_{k}"].double().numpy()
    close = lambda a, b: np.allclose(a, b, rtol=1e-5, atol=2e-6)
    assert close(M.unpack_nodes(x, n_atoms), gold("xh"))
    assert close(M.unpack_pairs(ex, n_atoms), gold("edge_x"))
    assert close(M.unpack_nodes(z, n_atoms), gold("z_t"))
    assert close(M.unpack_pairs(ez, n_atoms), gold("edge_z_t"))
    assert np.allclose(M.unpack_nodes(aligned, n_atoms), gold("align_pos"), rtol=0.0, atol=1e-5)
    node_off, _ = M.offsets(n_atoms)
    for b, n in enumerate(n_atoms):
        if n < 3:                                      # with fewer atoms the rotation is not unique (rank-deficient covariance)
            continue
        want = gold("rotations")[b]
        if sing[b, 2] >= 1e-6 * sing[b, 0]:
            assert np.allclose(rot[b], want, rtol=0.0, atol=1e-4), b
        else:
            # three centred atoms span a plane: s3 = 0 up to rounding and sign(det A) is rounding noise in any precision (the reference's
            # float32 SVD and this float64 one may draw different signs), so the rotation is fixed up to that one factor on u3 v3^T
            A = z[node_off[b]:node_off[b + 1], :3].T @ x[node_off[b]:node_off[b + 1], :3]
            U, _, Vt = np.linalg.svd(A)
            both = [(U * np.array([1.0, 1.0, s])) @ Vt for s in (1.0, -1.0)]
            assert min(np.abs(r - rot[b]).max() for r in both) <= 1e-12
            assert min(np.abs(r - want).max() for r in both) <= 1e-4, b
        # the reference's rotations are proper ones, the rank-2 one included: U diag(1, 1, det U det V^T) V^T names them without the noise
        proper = M.proper_rotation(z[node_off[b]:node_off[b + 1], :3], x[node_off[b]:node_off[b + 1], :3])
        assert np.allclose(proper, want, rtol=0.0, atol=1e-4), b
    pred, epred = M.pack_nodes(gold("pred"), n_atoms), M.pack_pairs(gold("edge_pred"), n_atoms)
    wm = np.sqrt(alpha.astype(np.float64) / sigma.astype(np.float64)) / len(n_atoms)
    loss_m, dpos, dfeat, dedge = M.loss_and_grads(n_atoms, pred[:, :3], pred[:, 3:], epred, aligned, x[:, 3:], ex, wm)
    want = float(g[TAG + "_loss"])
    assert abs(float(loss_m.sum()) - want) <= 1e-5 * abs(want), (float(loss_m.sum()), want)
    # the gradients of the packed loss are those of the dense loss (both cells of a pair add up)
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    pd, ed = T(gold("pred")).requires_grad_(True), T(gold("edge_pred")).requires_grad_(True)
    dense = otrain.loss_from_predictions(pd, ed, T(M.unpack_nodes(x, n_atoms)), T(M.unpack_pairs(ex, n_atoms)),
                                         T(M.unpack_nodes(aligned, n_atoms)), T(alpha), T(sigma))
    dense.backward()
    assert abs(float(dense.detach()) - float(loss_m.sum())) <= 1e-12 * abs(float(dense.detach()))
    gp = M.pack_nodes(pd.grad.numpy(), n_atoms)
    ge = M.pack_pairs(ed.grad.numpy(), n_atoms) + M.pack_pairs(ed.grad.numpy(), n_atoms, lower=True)
    for got, ref in ((dpos, gp[:, :3]), (dfeat, gp[:, 3:]), (dedge, ge)):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_pack_and_unpack_are_inverse_and_follow_pair_index_order():
    n_atoms = [3, 1, 4, 2]
    a, b, m = M.pair_tables(n_atoms)
    _, pair_off = M.offsets(n_atoms)
    for r in range(len(a)):
        n = n_atoms[m[r]]
        assert r - pair_off[m[r]] == a[r] * (2 * n - a[r] - 1) // 2 + (b[r] - a[r] - 1)
    rng = np.random.default_rng(0)
    pk = rng.normal(size=(len(a), 2))
    assert np.array_equal(M.pack_pairs(M.unpack_pairs(pk, n_atoms), n_atoms), pk)
    assert np.array_equal(M.pack_pairs(M.unpack_pairs(pk, n_atoms), n_atoms, lower=True), pk)
    nd = rng.normal(size=(sum(n_atoms), 5))
    assert np.array_equal(M.pack_nodes(M.unpack_nodes(nd, n_atoms), n_atoms), nd)


def test_kabsch_cases_are_well_posed():
    """Every generated case whose covariance has full rank determines its rotation well: (s2 + sign(det) s3) / s1 >= 0.05, the margin the
    GPU test asserts before it compares rotations."""
    for name, pred, tar in M.kabsch_cases():
        _, _, S = M.kabsch_align([len(tar)], pred, tar)
        s = S[0]
        if s[2] >= 1e-6 * s[0] and s[0] > 0:
            assert (s[1] + M.det_sign(pred, tar) * s[2]) / s[0] >= 0.05, (name, s)


def test_time_features_match_torch_and_autograd():
    rng = np.random.default_rng(1)
    x, w = rng.uniform(-12, 12, 33).astype(np.float32), rng.uniform(-1.5, 1.5, 8).astype(np.float32)
    fr = torch.from_numpy(M.time_feat_argument(x, w)).double()
    xt = torch.from_numpy(x).double().unsqueeze(-1)
    assert np.abs(M.time_feat(x, w) - torch.cat((xt, fr.sin(), fr.cos()), dim=-1).numpy()).max() <= 1e-15
    # float32 argument vs the float64 product: it differs by the argument's rounding only
    wt = torch.from_numpy(w).double().requires_grad_(True)
    fr64 = xt * wt.unsqueeze(0) * 2 * np.pi
    assert float((fr - fr64.detach()).abs().max()) <= 4 * 2.0 ** -24 * float(fr64.detach().abs().max())
    df = rng.normal(size=(33, 17))
    (torch.cat((xt, fr64.sin(), fr64.cos()), dim=-1) * torch.from_numpy(df)).sum().backward()
    dw = M.time_feat_weight_grad(x, w, df)
    assert np.abs(dw - wt.grad.numpy()).max() <= 2e-5 * np.abs(wt.grad.numpy()).max()      # the fp32 argument again, times |df| 2 pi |x|


def test_adj_bits():
    th, cut = 0.0, 2.0
    e = np.array([-1.0, -0.0, 0.0, np.nextafter(np.float32(0), np.float32(-1)), 0.5], np.float32)
    d = np.array([2.0, np.nextafter(np.float32(2), np.float32(3)), np.nextafter(np.float32(2), np.float32(0)), 0.0, 9.0], np.float32)
    assert M.adj_bits(e, d, th, cut).tolist() == [2, 1, 3, 2, 1]


def test_batch_norm_matches_torch_float64():
    """y, batch statistics, running statistics after two calls and the three gradients against F.batch_norm + autograd in float64."""
    rng = np.random.default_rng(2)
    for R, C in ((2, 5), (130, 17), (300, 70)):
        x, dy = rng.normal(size=(R, C)) * 1.7 + 0.3, rng.normal(size=(R, C))
        gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(size=C)
        rm0, rv0 = rng.normal(size=C), rng.uniform(0.5, 2.0, C)
        xt = torch.from_numpy(x).requires_grad_(True)
        gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
        rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
        yt = F.batch_norm(xt, rm, rv, gt, bt, True, 0.1, 1e-5)
        (yt * torch.from_numpy(dy)).sum().backward()
        with torch.no_grad():
            F.batch_norm(xt, rm, rv, gt, bt, True, 0.1, 1e-5)
        y, mean, rstd, unb, rm1, rv1 = M.batch_norm_train(x, gamma, beta, 1e-5, rm0, rv0)
        _, _, _, _, rm2, rv2 = M.batch_norm_train(x, gamma, beta, 1e-5, rm1, rv1)
        dx, dgamma, dbeta = M.batch_norm_backward(dy, x, mean, rstd, gamma)
        assert np.abs(mean - x.mean(0)).max() <= 1e-12 and np.abs(unb - x.var(0, ddof=1)).max() <= 1e-12
        assert np.abs(rstd - 1.0 / np.sqrt(x.var(0) + 1e-5)).max() <= 1e-12 * rstd.max()
        for got, ref in ((y, yt.detach()), (rm2, rm), (rv2, rv), (dx, xt.grad), (dgamma, gt.grad), (dbeta, bt.grad)):
            ref = ref.numpy()
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (R, C)
        assert M.batch_norm_train(x, gamma, beta, 1e-5)[4] is None


def test_layer_norm_matches_torch_float64():
    rng = np.random.default_rng(3)
    for R, C in ((1, 256), (6, 256), (5, 70), (7, 100)):
        x, dy = rng.normal(size=(R, C)) * 2.0 - 0.7, rng.normal(size=(R, C))
        gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(size=C)
        xt = torch.from_numpy(x).requires_grad_(True)
        gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
        yt = F.layer_norm(xt, (C,), gt, bt, 1e-5)
        (yt * torch.from_numpy(dy)).sum().backward()
        y, mean, rstd = M.layer_norm_affine(x, gamma, beta, 1e-5)
        dx, dgamma, dbeta = M.layer_norm_backward(dy, x, mean, rstd, gamma)
        assert np.abs(mean - x.mean(1)).max() <= 1e-12
        for got, ref in ((y, yt.detach()), (dx, xt.grad), (dgamma, gt.grad), (dbeta, bt.grad)):
            ref = ref.numpy()
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (R, C)


def test_adamw_amsgrad_matches_torch_float64():
    """Three steps against torch.optim.AdamW(amsgrad=True) in float64, with the EMA of ema.py folded in."""
    rng = np.random.default_rng(4)
    n, lr, betas, eps, wd, omd = 257, 3e-3, (0.9, 0.999), 1e-8, 0.05, 0.01
    p0 = rng.normal(size=n)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([pt], lr=lr, betas=betas, eps=eps, weight_decay=wd, amsgrad=True)
    p, m, v, vmax, ema = p0.copy(), np.zeros(n), np.zeros(n), np.zeros(n), p0.copy()
    ema_t = torch.from_numpy(p0.copy())
    for step in (1, 2, 3):
        g = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 1, n)
        clip = 0.5 if step == 2 else 1.0
        pt.grad = torch.from_numpy(g * clip)
        opt.step()
        ema_t.sub_(omd * (ema_t - pt.detach()))
        p, m, v, vmax, ema = M.adamw_amsgrad_ema_step(p, g, m, v, vmax, ema, step, lr, betas, eps, wd, clip, omd)
        st = opt.state[pt]
        for got, ref in ((p, pt.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"]), (vmax, st["max_exp_avg_sq"]), (ema, ema_t)):
            ref = ref.numpy()
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), step
    assert M.adamw_amsgrad_ema_step(p, g, m, v, vmax, None, 4, lr, betas, eps, wd)[4] is None


def test_bf16_rne_is_torch_bfloat16_bit_for_bit():
    to_bf16 = lambda b: torch.from_numpy(b.view(np.float32).copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    bits = np.concatenate([M.bf16_value_bits(), M.bf16_subnormal_bits()])
    want, got = to_bf16(bits), M.bf16_rne(bits)
    assert np.array_equal(got, want), [hex(b) for b in bits[got != want][:8]]
    # a NaN stays a NaN on both sides; WHICH NaN torch writes depends on the code path it takes (0x7FC0 scalar, 0xFFFF vectorised)
    is_nan = lambda h: ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)
    assert is_nan(to_bf16(M.bf16_nan_bits())).all() and is_nan(M.bf16_rne(M.bf16_nan_bits())).all()
    # the list holds what it promises: ties behind an even and an odd kept bit, a carry to inf, signed zeros
    assert M.bf16_rne(np.array([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x80000000], np.uint32)).tolist() == [0x3F80, 0x3F82, 0x7F80, 0x8000]
