"""fp64 mirror of the multistep solver update (``ds_solver_step*``, include/diffspectra_solver.h) and the closed forms that pin the
solvers without a converged checkpoint: a Gaussian data distribution N(mu, s^2), whose ideal denoiser, probability-flow ODE and
marginals are known exactly.  Test infrastructure only; torch on the CPU."""
from __future__ import annotations

import torch


def mirror_step(row, temp, x, edge_x, pred, edge_pred, hist, edge_hist, noise_x, noise_e, node_mask, edge_mask):
    """One update in fp64: ``row`` = (a, b, c, d); x [B,N,9], edge_x [B,N,N,2]; ``noise_*`` are the transformed draws (masked,
    CoM-projected, symmetric) or None.  With c == 0 the history does not enter at all (it may hold NaN), with d == 0 no noise does.
    Returns (x_mean, x_new, edge_mean, edge_new); masked entries are those of the inputs ``x`` / ``edge_x`` (the kernel does not write
    them) - for the means they are NaN here, so a caller has to select the valid ones."""
    a, b, c, d = (float(v) for v in row)
    f = lambda t: None if t is None else t.detach().cpu().double()
    x, edge_x, pred, edge_pred, hist, edge_hist, noise_x, noise_e = map(f, (x, edge_x, pred, edge_pred, hist, edge_hist, noise_x, noise_e))
    nm = node_mask.detach().cpu().bool().reshape(x.shape[0], x.shape[1], 1).expand_as(x)
    em = edge_mask.detach().cpu().bool().reshape(edge_x.shape[0], edge_x.shape[1], edge_x.shape[2], 1).expand_as(edge_x)
    out = []
    for s, p, h, nz, mask in ((x, pred, hist, noise_x, nm), (edge_x, edge_pred, edge_hist, noise_e, em)):
        mean = a * s + b * p
        if c != 0.0:
            mean = mean + c * h
        new = mean + (d * nz) * float(temp) if d != 0.0 else mean
        nan = torch.full_like(s, float("nan"))
        out += [torch.where(mask, mean, nan), torch.where(mask, new, s)]
    return tuple(out)


def gaussian_denoiser(x, alpha, sigma, mu, s):
    """E[x_0 | x_t = x] for x_0 ~ N(mu, s^2), x_t = alpha x_0 + sigma eps: (alpha s^2 x + sigma^2 mu) / (alpha^2 s^2 + sigma^2)."""
    return (alpha * s * s * x + sigma * sigma * mu) / (alpha * alpha * s * s + sigma * sigma)


def gaussian_flow(x_T, alpha_T, sigma_T, alpha, sigma, mu, s):
    """The probability-flow ODE of that distribution carries x_T at (alpha_T, sigma_T) to
    mu alpha + (x_T - mu alpha_T) sqrt((alpha^2 s^2 + sigma^2) / (alpha_T^2 s^2 + sigma_T^2)): it maps marginal onto marginal."""
    return mu * alpha + (x_T - mu * alpha_T) * ((alpha * alpha * s * s + sigma * sigma) / (alpha_T * alpha_T * s * s + sigma_T * sigma_T)) ** 0.5


def propagate_moments(rows, alpha, sigma, mu, s):
    """Mean and variance of x after rows 0 .. S-2 under the linear denoiser of N(mu, s^2), exactly: x is affine in (x_T, eps_0, ...), so the
    mean and the 2x2 covariance of z = (x, p_prev) follow z' = M z + v + (d eps, 0) with p_i = g x + f,
    M = [[a + b g, c], [g, 0]], v = (b f, f).  x_T ~ the true marginal at t_0, temperature 1.  ``rows``, ``alpha``, ``sigma``: fp64."""
    dd = torch.float64
    m = torch.tensor([alpha[0] * mu, 0.0], dtype=dd)
    C = torch.zeros(2, 2, dtype=dd)
    C[0, 0] = alpha[0] ** 2 * s * s + sigma[0] ** 2
    for i in range(rows.shape[0] - 1):
        a, b, c, d = (rows[i, j] for j in range(4))
        den = alpha[i] ** 2 * s * s + sigma[i] ** 2
        g, f = alpha[i] * s * s / den, sigma[i] ** 2 * mu / den
        M = torch.stack([torch.stack([a + b * g, c]), torch.stack([g, torch.zeros((), dtype=dd)])])
        v = torch.stack([b * f, f])
        m = M @ m + v
        C = M @ C @ M.T
        C[0, 0] = C[0, 0] + d * d
    return m[0], C[0, 0]
