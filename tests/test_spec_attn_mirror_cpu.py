"""tests/spec_attn_mirror.py pinned without a GPU: ``exact`` against torch autograd in fp64 and against the oracle's residual attention; the
closed-form decomposition of the chained score gradient; ``flash_emulation`` without roundings == ``exact``; and the derived bound (a) + (b)
against an fp32 emulation of the flash arithmetic in numpy, in two summation orders - which also shows what the bound catches: each of
three deliberately broken arithmetics (one key too few masked, the lo half of split2 dropped, l summed from the rounded p) leaves it by
orders of magnitude."""
import numpy as np
import pytest
import torch

from tests import spec_attn_mirror as SM

SCALE = SM.DK ** -0.5
CASES = [(69, 1, 3), (33, 3, 2), (32, 2, 2), (1, 2, 2)]          # (L, n_layers, B); the first is the committed case of the allowance test
SEED = 20250


def inputs(L, n, B):
    return SM.random_inputs(B, L, n, SEED + 1000 * L + n)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("L,n,B", [(37, 3, 2), (1, 3, 1)])
def test_exact_vs_autograd_fp64(L, n, B):
    qkv, dout = inputs(L, n, B)
    prev = torch.randn(B, SM.H, L, L, generator=torch.Generator().manual_seed(3)).double()
    r = SM.exact(qkv, SCALE, dout, prev=prev)
    x = [t.double().clone().requires_grad_(True) for t in qkv]
    s, loss = prev, 0.0
    for l in range(n):
        q, k, v = SM.parts(x[l])
        s = SCALE * q @ k.transpose(-1, -2) + s
        o = SM.merge(torch.softmax(s, -1) @ v)
        assert float((o.detach() - r["out"][l]).abs().max()) <= 1e-13
        assert float((s.detach() - r["scores"][l]).abs().max()) <= 1e-13
        s.retain_grad()
        r.setdefault("_s", []).append(s)
        loss = loss + (o * dout[l].double()).sum()
    loss.backward()
    for l in range(n):
        assert float((x[l].grad - r["dqkv"][l]).abs().max()) <= 1e-11 * max(1.0, float(x[l].grad.abs().max())), l
        assert float((r["_s"][l].grad - r["dscores"][l]).abs().max()) <= 1e-12, l
        lse = torch.logsumexp(r["scores"][l], -1)
        assert float((r["max_ln"][l] + torch.log(r["sum_ln"][l]) - lse).abs().max()) <= 1e-12
        assert float((r["max_log2"][l] + torch.log2(r["sum_log2"][l]) - lse * SM.LOG2E).abs().max()) <= 1e-11


def test_exact_vs_oracle_attention():
    """The oracle's residual attention (oracle/specformer.py, the function its SpecFormer forward runs), evaluated in fp64."""
    from oracle.specformer import residual_attention
    L, n, B = 41, 3, 2
    qkv, _ = inputs(L, n, B)
    r = SM.exact(qkv, SCALE)
    prev = None
    for l in range(n):
        q, k, v = SM.parts(qkv[l].double())
        o, prev = residual_attention(q.contiguous(), k.transpose(-1, -2).contiguous(), v.contiguous(), SCALE, prev)
        assert float((o - r["out"][l]).abs().max()) <= 1e-13
        assert float((prev - r["scores"][l]).abs().max()) <= 1e-13


def test_decomposition_equals_chain():
    L, n, B = 37, 3, 2
    qkv, dout = inputs(L, n, B)
    r = SM.exact(qkv, SCALE, dout)
    for j in range(n):
        for name, contrib in (("dq", r["contrib_q"]), ("dk", r["contrib_k"])):
            tot = sum(contrib[l][j] for l in range(j, n))
            assert float((tot - r[name][j]).abs().max()) <= 1e-11, (name, j)


@pytest.mark.parametrize("L,n,B", [(37, 3, 2), (32, 1, 1), (1, 2, 1)])
def test_unrounded_emulation_equals_exact(L, n, B):
    qkv, dout = inputs(L, n, B)
    r = SM.exact(qkv, SCALE, dout)
    for l in range(n):
        e = SM.flash_emulation(qkv[:l + 1], SCALE, dout[l], round_operands=False)
        close = lambda a, b, what: float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())) or pytest.fail(f"{what}, layer {l}")
        close(e["scores"], r["scores"][l] * SM.LOG2E, "scores")
        close(e["max"], r["max_log2"][l], "max"); close(e["sum"], r["sum_log2"][l], "sum"); close(e["out"], r["out"][l], "out")
        close(e["dv"], r["dv"][l], "dv")
        for j in range(l + 1):
            close(e["dq"][j], r["contrib_q"][l][j], f"dq {j}"); close(e["dk"][j], r["contrib_k"][l][j], f"dk {j}")
        assert all(float(torch.as_tensor(b).abs().max()) == 0.0 for b in (e["bound"]["out"], e["bound"]["dv"], *e["bound"]["dq"], *e["bound"]["dk"]))


# ------------------------------------------------------------------------------------------------ the flash arithmetic in fp32 (numpy)
f32 = np.float32


def bf(x):
    """fp32 array -> bf16 (nearest even) -> fp32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).bfloat16().float().numpy()


def dot32(A, Bm, order):
    """sum_c A[.., i, c] B[.., j, c] accumulated in fp32 in the column order ``order``: [.., i, j]."""
    acc = np.zeros(A.shape[:-1] + (Bm.shape[-2],), f32)
    for c in order:
        acc = acc + A[..., :, None, c] * Bm[..., None, :, c]
    return acc


def over32(Wt, X, order):
    """sum_k Wt[.., i, k] X[.., k, :] accumulated in fp32 over k in ``order``: [.., i, d]."""
    acc = np.zeros(Wt.shape[:-1] + (X.shape[-1],), f32)
    for k in order:
        acc = acc + Wt[..., :, k, None] * X[..., None, k, :]
    return acc


def seq(n, rev):
    return list(range(n))[::-1] if rev else list(range(n))


def fp32_flash(qkv_layers, scale, dout, rev, brk=None):
    """The flash kernels' arithmetic in fp32: same operands, same tiles of 32 keys and running maximum, every sum in ascending (``rev`` =
    False) or descending order.  ``brk``: "mask" (the first padded key takes part), "no_lo" (split2 without its lo half), "l_rounded" (l summed
    from the bf16 p)."""
    Q, K, V, qs, ks = SM.flash_operands(qkv_layers, scale)
    Q, K, V = (t.numpy().astype(f32) for t in (Q, K, V))
    qs, ks = [t.numpy().astype(f32) for t in qs], [t.numpy().astype(f32) for t in ks]
    B, Hh, L, Kd = Q.shape
    NT = (L + 31) // 32
    LP = NT * 32
    pad = lambda x: np.concatenate([x, np.zeros(x.shape[:2] + (LP - L,) + x.shape[3:], f32)], 2)
    Kp, Vp = pad(K), pad(V)
    s = dot32(Q, Kp, seq(Kd, rev))
    live = L + 1 if brk == "mask" else L
    s[..., min(live, LP):] = -np.inf
    m = np.full(s.shape[:-1], -np.inf, f32)
    l = np.zeros_like(m)
    o = np.zeros(s.shape[:-1] + (8,), f32)
    with np.errstate(invalid="ignore"):
        for t in range(NT):
            st = s[..., 32 * t:32 * t + 32]
            mn = np.maximum(m, st.max(-1))
            alpha = np.exp2(m - mn).astype(f32)
            p = np.exp2(st - mn[..., None]).astype(f32)
            ph = bf(p)
            rs = np.zeros_like(m)
            for k in seq(32, rev):
                rs = rs + (ph if brk == "l_rounded" else p)[..., k]
            l = l * alpha + rs
            o = o * alpha[..., None] + over32(ph, Vp[..., 32 * t:32 * t + 32, :], seq(32, rev))
            m = mn
    out = o * (f32(1.0) / l)[..., None]
    res = dict(max=m, sum=l, out=SM.merge(torch.from_numpy(out)), stats=torch.from_numpy(np.stack([m, l], -1)))
    if dout is None:
        return res
    dO = SM.heads(dout).numpy().astype(f32)
    D = np.zeros_like(m)
    for e in seq(8, rev):
        D = D + dO[..., e] * out[..., e]
    x = m + np.log2(l).astype(f32)

    def split(y):
        hi = bf(y)
        return hi, (np.zeros_like(hi) if brk == "no_lo" else bf(y - hi))
    one = np.ones((B, Hh, L, 2), f32)
    Qx = np.concatenate([Q, np.stack(split(-x), -1)], -1)
    Kx = np.concatenate([K, one], -1)
    dOx = np.concatenate([bf(dO), np.stack(split(-D), -1)], -1)
    Vx = np.concatenate([V, one], -1)
    pb = np.exp2(dot32(Qx, Kx, seq(Kd + 2, rev))).astype(f32)
    dS = bf(pb * dot32(dOx, Vx, seq(10, rev)))
    Ph = bf(pb)
    sc, ln2 = f32(scale), f32(SM.LN2)
    tr = lambda a: np.swapaxes(a, -1, -2)
    res["dq"] = [SM.merge(torch.from_numpy(sc * over32(dS, kj, seq(L, rev)))) for kj in ks]
    res["dk"] = [SM.merge(torch.from_numpy(ln2 * over32(tr(dS), qj, seq(L, rev)))) for qj in qs]
    res["dv"] = SM.merge(torch.from_numpy(over32(tr(Ph), bf(dO), seq(L, rev))))
    return res


def shares(got, emu):
    """{name: max |got - emulation| / bound} of one call (0 / 0 = 0)."""
    def share(g, e, b):
        d = (torch.as_tensor(g).double() - e).abs()
        assert bool(torch.isfinite(d).all())
        return float(torch.where(d > 0, d / b.clamp_min(1e-300), d).max())
    r = dict(max=share(got["max"], emu["max"], emu["bound"]["max"]), sum=share(got["sum"], emu["sum"], emu["bound"]["sum"]),
             out=share(got["out"], emu["out"], emu["bound"]["out"]))
    if "dv" in got:
        r["dv"] = share(got["dv"], emu["dv"], emu["bound"]["dv"])
        r["dq"] = max(share(g, e, b) for g, e, b in zip(got["dq"], emu["dq"], emu["bound"]["dq"]))
        r["dk"] = max(share(g, e, b) for g, e, b in zip(got["dk"], emu["dk"], emu["bound"]["dk"]))
    return r


_RUNS = {}


def run(L, n, B, rev, brk=None):
    key = (L, n, B, rev, brk)
    if key not in _RUNS:
        qkv, dout = inputs(L, n, B)
        got = fp32_flash(qkv, SCALE, dout[n - 1], rev, brk)
        emu = SM.flash_emulation(qkv, SCALE, dout[n - 1], stats=got["stats"], out=got["out"], max_obs=got["max"])
        _RUNS[key] = (got, emu)
    return _RUNS[key]


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("L,n,B", CASES)
def test_fp32_arithmetic_stays_inside_the_bound(L, n, B, rev):
    got, emu = run(L, n, B, rev)
    sh = shares(got, emu)
    print(f"[flash fp32 emulation, L = {L}, layers = {n}, B = {B}, {'descending' if rev else 'ascending'}] deviation / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sh.items()) + "; at risk: " + ", ".join(f"{k} {v:.2%}" for k, v in emu["share_at_risk"].items())
          + "; zero allowance: " + ", ".join(f"{k} {v:.1%}" for k, v in emu["share_zero_allowance"].items()))
    assert max(sh.values()) <= 1.0, sh


def test_the_two_orders_differ():
    """... so the bound is exercised: the two fp32 runs are not the same numbers."""
    a, b = run(69, 1, 3, False)[0], run(69, 1, 3, True)[0]
    assert not torch.equal(a["out"], b["out"]) and not torch.equal(a["dq"][0], b["dq"][0])


def test_allowance_does_not_swallow_the_test():
    """Committed seed of the smallest case (L = 69, one layer, B = 3, inputs of order 1): at least 90 % of the output elements carry NO
    rounding-risk allowance, i.e. are held to the fp32 accumulation bound alone."""
    _, emu = run(69, 1, 3, False)
    print(f"[allowance, L = 69] at risk {emu['share_at_risk']}, zero allowance {emu['share_zero_allowance']}")
    assert emu["share_zero_allowance"]["out"] >= 0.90, emu["share_zero_allowance"]
    assert emu["share_at_risk"]["P"] <= 0.01, emu["share_at_risk"]


@pytest.mark.parametrize("brk,names,floor", [("mask", ("sum", "out"), 100.0), ("l_rounded", ("sum", "out"), 10.0), ("no_lo", ("dq", "dk", "dv"), 100.0)])
def test_broken_arithmetic_leaves_the_bound(brk, names, floor):
    """What a GPU comparison would do with a subtly wrong kernel, tried on the fp32 emulation (L = 69, one layer): the share deviation / bound
    of the named results goes from <= 1 to >= ``floor``.  A padded key that takes part adds exp2(0 - m) to l and a lost lo half shifts every
    exponent by up to 2^-9 |m + log2 l|: per cent, against a bound of 1e-5 - floor 100 (seen: 1.5e3 / 5.6e2 and, no_lo, above 1e3).  l from the
    rounded p is off by the MEAN of some tens of bf16 rounding errors of random sign, 2^-9 / sqrt(keys that matter) or a few 1e-4 relative,
    against 5e-6 - floor 10 (seen: 85 for l, 34 for out)."""
    got, emu = run(69, 1, 3, False, brk)
    sh = shares(got, emu)
    print(f"[broken: {brk}] deviation / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sh.items()))
    for k in names:
        assert sh[k] >= floor, (brk, k, sh[k])
