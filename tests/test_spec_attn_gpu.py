"""GPU parity of SpecFormer's residual-score attention in its three hand-written forms, every entry point called directly and compared PER ELEMENT
(flash form) or per molecule-head (fp32 forms) with the float64 yardstick of tests/spec_attn_mirror.py (pinned on the CPU by
tests/test_spec_attn_mirror_cpu.py):

* ``dst_spec_attn_flash_fwd / _bwd`` (csrc/ds_train_attn.hip) against ``flash_emulation``: stats[.., 0] to the score bound, stats[.., 1] and
  ``out`` to the derived bound (a) + (b); the backward TEACHER-FORCED from the kernel's own stats and out: dq_j, dk_j (j <= l), dv_l per
  element; the calling contract (accumulate 0 / 1, part 0 / 1 / 2), the argument limit L <= 384 at both entry points;
* ``dst_spec_attn_fwd / _bwd`` (csrc/ds_train.hip) over three chained layers against ``exact``: scores, (row max, row sum), out at the suite's
  exp-epilogue figure 3e-6, dqkv and dscores at 2e-5 (tests/test_train_hip.py's figure for every fp32 backward), both as
  max |got - ref| / max |ref| over the rows of a molecule-head; the pad columns L .. Lp-1 of scores and dscores keep their sentinel;
* ``ds_spec_attention`` (csrc/ds_spec.hip) with the 16 heads of production against ``exact``: the key-major scores written in place to a
  dot-product bound, ``out`` at 3e-6 per molecule-head.

In every test: 32 sentinel guard rows behind every buffer, inputs included, which must survive bit for bit; owned rows hold no sentinel,
no NaN, no Inf; every call twice, bit-identical; the same molecules in reversed batch order give bit-identical rows per molecule.  Every
test prints one line per case: the largest deviation as a share of its bound (or tolerance), the share of elements without rounding-risk
allowance, and the distance of kernel and of emulation from ``exact`` (max |a - b| / max |b|)."""
import pytest
import torch

from tests import spec_attn_mirror as SM
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

Hh, DK, DM = SM.H, SM.DK, SM.H * SM.DK
SCALE = DK ** -0.5
SENT = -7.5
GUARD = 32
TOL = dict(act=3e-6, bwd=2e-5)
ERR_ARG = -1                                    # DS_ERR_ARG


class Ctx:
    """The library and a list that keeps every operand alive until the synchronise (``_dev`` in tests/test_train_hip.py)."""

    def __init__(self, d):
        from diffspectra_amd import engine as E, train_engine as T
        self.E, self.d, self.lib, self.keep = E, d, T.load_train_library(), []

    def rows(self, t):
        """A host tensor [.., C] as device rows [R + GUARD, C], the guard rows full of the sentinel."""
        t = t.reshape(-1, t.shape[-1]).float()
        x = torch.cat([t, torch.full((GUARD, t.shape[1]), SENT)]).to(self.d).contiguous()
        self.keep.append(x)
        return x

    def buf(self, rows, cols, fill=SENT):
        x = torch.full((rows + GUARD, cols), SENT, device=self.d)
        x[:rows] = fill
        self.keep.append(x)
        return x

    def sync(self):
        torch.cuda.synchronize()
        self.keep.clear()

    def s(self):
        return self.E._stream()


_CTX = {}


def ctx(gpu_device):
    if "c" not in _CTX:
        _CTX["c"] = Ctx(gpu_device)
    return _CTX["c"]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guard_ok(t, rows, what):
    assert bool((t[rows:] == SENT).all()) and t.shape[0] == rows + GUARD, f"{what}: guard rows overwritten"


def owned_ok(t, rows, what, cols=None):
    """Guard rows intact; the owned rows (columns ``cols``) finite and free of the sentinel."""
    guard_ok(t, rows, what)
    o = t[:rows] if cols is None else t[:rows, cols[0]:cols[1]]
    assert bool(torch.isfinite(o).all()), f"{what}: NaN / Inf in owned rows"
    assert not bool((o == SENT).any()), f"{what}: sentinel left in owned rows"


def share(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0)."""
    d = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    return float(torch.where(d > 0, d / bound.clamp_min(1e-300), d).max())


REF_ERR = 1e-13                                 # the float64 reference's own rounding on inputs of order 1 (dscores of a one-key row: exactly 0, ref 1e-17)


def per_head(got, ref):
    """max over the molecule-heads of max |got - ref| / max |ref| (``relerr`` per molecule-head); both [B, H, ...]."""
    d = ((got.double() - ref).abs().flatten(2).amax(-1) - REF_ERR).clamp_min(0.0)
    return float((d / (ref.abs().flatten(2).amax(-1) + 1e-30)).max())


# ================================================================================================ flash form
FLASH_L = [1, 31, 32, 33, 69, 352, 384]          # one partial tile, one full tile, a tail of 1, 3 tiles, 11 and 12 full tiles (384: the largest L)
_FLASH_IN, _EXACT = {}, {}


def flash_B(L):
    return 1 if L == 384 else 2                  # B = 2: 32 workgroups, the XCD remap branch; B = 1: 16, the plain one


def flash_inputs(L, qk_mul=1.0):
    key = (L, qk_mul)
    if key not in _FLASH_IN:
        qkv, dout = _FLASH_IN[key] = SM.random_inputs(flash_B(L), L, 3, 7000 + L, qk_mul=qk_mul)
        _EXACT[key] = SM.exact(qkv, SCALE, dout)
    return _FLASH_IN[key] + (_EXACT[key],)


def flash_fwd(c, qd, n, B, L):
    st, out = c.buf(B * Hh * L, 2), c.buf(B * L, DM)
    p = [c.E._ptr(x) for x in qd[:n]] + [0] * (3 - n)
    rc = c.lib.dst_spec_attn_flash_fwd(p[0], p[1], p[2], n, c.E._ptr(st), c.E._ptr(out), B, L, Hh, DK, SCALE, c.s())
    return rc, st, out


def flash_bwd(c, qd, n, st, out, dd, grads, B, L, part, accumulate):
    p = [c.E._ptr(x) for x in qd[:n]] + [0] * (3 - n)
    g = [c.E._ptr(x) for x in grads[:n]] + [0] * (3 - n)
    return c.lib.dst_spec_attn_flash_bwd(p[0], p[1], p[2], n, c.E._ptr(st), c.E._ptr(out), c.E._ptr(dd), g[0], g[1], g[2], B, L, Hh, DK, SCALE, part,
                                         accumulate, c.s())


def nan_grads(c, n, R):
    return [c.buf(R, 3 * DM, float("nan")) for _ in range(n)]


def flash_case(c, L, n, qk_mul=1.0):
    """Forward and backward of one call with n_layers = n: everything but the comparison with ``exact`` is asserted here."""
    B = flash_B(L)
    qkv, dout, ex = flash_inputs(L, qk_mul)
    R = B * L
    qd, dd = [c.rows(x) for x in qkv[:n]], c.rows(dout[n - 1])
    rc, st, out = flash_fwd(c, qd, n, B, L)
    rc2, st2, out2 = flash_fwd(c, qd, n, B, L)
    assert rc == 0 and rc2 == 0
    g0, g0b = nan_grads(c, n, R), nan_grads(c, n, R)
    assert flash_bwd(c, qd, n, st, out, dd, g0, B, L, 0, 0) == 0 and flash_bwd(c, qd, n, st, out, dd, g0b, B, L, 0, 0) == 0
    torch.cuda.synchronize()
    assert same_bits(st, st2) and same_bits(out, out2), "forward: two runs differ"
    owned_ok(st, B * Hh * L, "stats"); owned_ok(out, R, "out")
    for x, h in zip(qd + [dd], list(qkv[:n]) + [dout[n - 1]]):
        assert same_bits(x[:R].cpu(), h.reshape(R, -1)) and bool((x[R:] == SENT).all()), "an input was written"
    # accumulate = 0 on NaN-filled buffers: q and k columns of layers 0 .. n-1 and the v columns of layer n-1 are assigned, nothing else
    for j in range(n):
        assert same_bits(g0[j], g0b[j]), "backward: two runs differ"
        owned_ok(g0[j], R, f"dqkv{j} q | k", (0, 2 * DM))
        if j == n - 1:
            owned_ok(g0[j], R, f"dqkv{j} v", (2 * DM, 3 * DM))
        else:
            assert bool(torch.isnan(g0[j][:R, 2 * DM:]).all()), f"dqkv{j}: v columns of a lower layer written"

    # ---- against the emulation, per element; the backward from the kernel's own stats and out
    st_k, out_k = st[:B * Hh * L].cpu().reshape(B, Hh, L, 2), out[:R].cpu().reshape(B, L, DM)
    e = SM.flash_emulation(qkv[:n], SCALE, dout[n - 1], stats=st_k, out=out_k, max_obs=st_k[..., 0])
    b = e["bound"]
    got = dict(max=st_k[..., 0], sum=st_k[..., 1], out=out_k, dv=g0[n - 1][:R, 2 * DM:].cpu().reshape(B, L, DM))
    sh = {k: share(got[k], e[k], b[k]) for k in ("max", "sum", "out", "dv")}
    dq = [g0[j][:R, :DM].cpu().reshape(B, L, DM) for j in range(n)]
    dk = [g0[j][:R, DM:2 * DM].cpu().reshape(B, L, DM) for j in range(n)]
    sh["dq"] = max(share(dq[j], e["dq"][j], b["dq"][j]) for j in range(n))
    sh["dk"] = max(share(dk[j], e["dk"][j], b["dk"][j]) for j in range(n))
    l = n - 1
    ref = dict(out=ex["out"][l], dv=ex["dv"][l], dq=torch.stack(ex["contrib_q"][l]), dk=torch.stack(ex["contrib_k"][l]))
    kern = dict(out=out_k, dv=got["dv"], dq=torch.stack(dq), dk=torch.stack(dk))
    emul = dict(out=e["out"], dv=e["dv"], dq=torch.stack(e["dq"]), dk=torch.stack(e["dk"]))
    print(f"[flash, L = {L}, B = {B}, layers = {n}{', q k x ' + str(qk_mul) if qk_mul != 1.0 else ''}] deviation / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sh.items())
          + "; at risk: " + ", ".join(f"{k} {v:.2%}" for k, v in e["share_at_risk"].items())
          + "; zero allowance: " + ", ".join(f"{k} {v:.1%}" for k, v in e["share_zero_allowance"].items())
          + "; kernel - exact: " + ", ".join(f"{k} {relerr(kern[k], ref[k]):.2e}" for k in ref)
          + "; emulation - exact: " + ", ".join(f"{k} {relerr(emul[k], ref[k]):.2e}" for k in ref)
          + f"; max |score| {float(ex['scores'][l].abs().max()):.0f}")
    assert max(sh.values()) <= 1.0, sh
    return dict(B=B, R=R, qkv=qkv, dout=dout, qd=qd, dd=dd, st=st, out=out, g0=g0)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("L", FLASH_L)
def test_flash_vs_emulation_and_calling_contract(gpu_device, L, n):
    c = ctx(gpu_device)
    k = flash_case(c, L, n)
    B, R, qd, dd, st, out, g0 = k["B"], k["R"], k["qd"], k["dd"], k["st"], k["out"], k["g0"]
    # accumulate = 1 onto preset buffers: the kernel adds ONE fp32 value to the loaded one - bit-equal to fp32(preset + result of accumulate = 0)
    # in the q and k columns; the v columns of layer n-1 are assigned, those of the lower layers not touched
    gen = torch.Generator().manual_seed(L + n)
    preset = [torch.randn(R, 3 * DM, generator=gen) for _ in range(n)]
    g1 = [c.rows(x) for x in preset]
    assert flash_bwd(c, qd, n, st, out, dd, g1, B, L, 0, 1) == 0
    # part 1 then 2, and 2 then 1, == part 0; each part leaves the other's columns alone
    orders = []
    for first, second in ((1, 2), (2, 1)):
        g = nan_grads(c, n, R)
        assert flash_bwd(c, qd, n, st, out, dd, g, B, L, first, 0) == 0
        torch.cuda.synchronize()
        for j in range(n):
            other = g[j][:R, DM:] if first == 1 else g[j][:R, :DM]
            assert bool(torch.isnan(other).all()), f"part {first} wrote columns of part {second}"
        assert flash_bwd(c, qd, n, st, out, dd, g, B, L, second, 0) == 0
        orders.append(g)
    torch.cuda.synchronize()
    for j in range(n):
        guard_ok(g1[j], R, f"accumulated dqkv{j}")
        want = preset[j].to(gpu_device).clone()
        want[:, :2 * DM] = preset[j].to(gpu_device)[:, :2 * DM] + g0[j][:R, :2 * DM]
        if j == n - 1:
            want[:, 2 * DM:] = g0[j][:R, 2 * DM:]
        assert same_bits(g1[j][:R], want), f"accumulate = 1, dqkv{j}"
        for g in orders:
            assert same_bits(g[j], g0[j]), f"part 1 + part 2 != part 0, dqkv{j}"
    # the same molecules in reversed batch order
    if B > 1:
        qr = [c.rows(x.flip(0)) for x in k["qkv"][:n]]
        dr = c.rows(k["dout"][n - 1].flip(0))
        rc, st_r, out_r = flash_fwd(c, qr, n, B, L)
        gr = nan_grads(c, n, R)
        assert rc == 0 and flash_bwd(c, qr, n, st_r, out_r, dr, gr, B, L, 0, 0) == 0
        torch.cuda.synchronize()
        flip = lambda t, rows: t[:rows * B].reshape(B, rows, -1).flip(0).reshape(rows * B, -1)
        assert same_bits(flip(st_r, Hh * L), st[:B * Hh * L]) and same_bits(flip(out_r, L), out[:R]), "batch order changes the forward"
        for j in range(n):
            assert same_bits(flip(gr[j], L), g0[j][:R]), "batch order changes the backward"
    c.sync()


def test_flash_peaked_scores(gpu_device):
    """q and k scaled by 4: |scores| beyond 100, most probabilities underflow, the row offsets m + log2 l are large numbers - the same
    emulation bound holds.  The distance from ``exact`` (printed) is the bf16 design's own and not a gate."""
    c = ctx(gpu_device)
    flash_case(c, 352, 3, qk_mul=4.0)
    c.sync()


def test_flash_argument_limit(gpu_device):
    """L = 384 is the largest length the backward's LDS tables fit in 64 KB; at 385 BOTH entry points return DS_ERR_ARG and write nothing - a
    tape the backward could not consume is never produced."""
    c = ctx(gpu_device)
    for L, want in ((384, 0), (385, ERR_ARG)):
        qkv, dout = SM.random_inputs(1, L, 1, 9000 + L)
        qd, dd = [c.rows(qkv[0])], c.rows(dout[0])
        rc, st, out = flash_fwd(c, qd, 1, 1, L)
        assert rc == want, ("forward", L, rc)
        g = nan_grads(c, 1, L)
        if want:                                                         # the backward's own check, on a tape of plausible numbers
            torch.cuda.synchronize()
            assert bool((st == SENT).all()) and bool((out == SENT).all()), "the refused forward wrote"
            st[:Hh * L] = 1.0; out[:L] = 0.5
            torch.cuda.synchronize()
        assert flash_bwd(c, qd, 1, st, out, dd, g, 1, L, 0, 0) == want, ("backward", L)
        torch.cuda.synchronize()
        if want:
            assert bool((st[:Hh * L] == 1.0).all()) and bool((out[:L] == 0.5).all()) and bool(torch.isnan(g[0][:L]).all()), "a refused call wrote"
        else:
            owned_ok(st, Hh * L, "stats"); owned_ok(out, L, "out"); owned_ok(g[0], L, "dqkv")
        guard_ok(st, Hh * L, "stats"); guard_ok(out, L, "out"); guard_ok(g[0], L, "dqkv")
    c.sync()


# ================================================================================================ fp32 materialised form
def mat_run(c, qkv, dout, B, L):
    """Three chained layers forward (scores of layer l = prev of layer l + 1), then the backward last to first (dscores_in = NULL for the last)."""
    Lp, R, RS = (L + 31) // 32 * 32, B * L, B * Hh * L
    qd, dd = [c.rows(x) for x in qkv], [c.rows(x) for x in dout]
    sc, st, out = ([c.buf(rows, cols) for _ in range(3)] for rows, cols in ((RS, Lp), (RS, 2), (R, DM)))
    dqkv, dsc = ([c.buf(rows, cols) for _ in range(3)] for rows, cols in ((R, 3 * DM), (RS, Lp)))
    P = c.E._ptr
    for l in range(3):
        assert c.lib.dst_spec_attn_fwd(P(qd[l]), P(sc[l - 1]) if l else 0, P(sc[l]), P(st[l]), P(out[l]), B, L, Hh, DK, SCALE, c.s()) == 0
    for l in (2, 1, 0):
        assert c.lib.dst_spec_attn_bwd(P(qd[l]), P(sc[l]), P(st[l]), P(dd[l]), P(dsc[l + 1]) if l < 2 else 0, P(dqkv[l]), P(dsc[l]), B, L, Hh, DK, SCALE,
                                       c.s()) == 0
    return dict(scores=sc, stats=st, out=out, dqkv=dqkv, dscores=dsc)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129, 347, 512])
def test_materialised_fp32_vs_exact(gpu_device, L):
    c = ctx(gpu_device)
    B = 1 if L == 512 else 2
    Lp, R, RS = (L + 31) // 32 * 32, B * L, B * Hh * L
    qkv, dout = SM.random_inputs(B, L, 3, 8000 + L)
    a, a2 = mat_run(c, qkv, dout, B, L), mat_run(c, qkv, dout, B, L)
    torch.cuda.synchronize()
    rows = dict(scores=RS, stats=RS, out=R, dqkv=R, dscores=RS)
    for k in a:
        for l in range(3):
            assert same_bits(a[k][l], a2[k][l]), f"{k}{l}: two runs differ"
            cols = (0, L) if k in ("scores", "dscores") else None
            owned_ok(a[k][l], rows[k], f"{k}{l}", cols)
            if cols and Lp > L:
                assert bool((a[k][l][:, L:] == SENT).all()), f"{k}{l}: pad columns L .. Lp-1 touched"
    if B > 1:
        r = mat_run(c, [x.flip(0) for x in qkv], [x.flip(0) for x in dout], B, L)
        torch.cuda.synchronize()
        for k in a:
            for l in range(3):
                n = rows[k] // B
                assert same_bits(r[k][l][:rows[k]].reshape(B, n, -1).flip(0).reshape(rows[k], -1), a[k][l][:rows[k]]), f"{k}{l}: batch order matters"
    ex = SM.exact(qkv, SCALE, dout)
    worst = {}
    for l in range(3):
        g = {k: a[k][l][:rows[k]].cpu() for k in a}
        sc, dsc = (g[k].reshape(B, Hh, L, Lp)[..., :L] for k in ("scores", "dscores"))
        st = g["stats"].reshape(B, Hh, L, 2)
        dq, dk, dv = SM.parts(g["dqkv"].reshape(B, L, 3 * DM))
        rq, rk, rv = SM.parts(ex["dqkv"][l])
        e = dict(scores=per_head(sc, ex["scores"][l]) / TOL["act"], max=per_head(st[..., 0], ex["max_ln"][l]) / TOL["act"],
                 sum=per_head(st[..., 1], ex["sum_ln"][l]) / TOL["act"], out=per_head(SM.heads(g["out"].reshape(B, L, DM)), SM.heads(ex["out"][l])) / TOL["act"],
                 dq=per_head(dq, rq) / TOL["bwd"], dk=per_head(dk, rk) / TOL["bwd"], dv=per_head(dv, rv) / TOL["bwd"],
                 dscores=per_head(dsc, ex["dscores"][l]) / TOL["bwd"])
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    print(f"[fp32 materialised, L = {L}, B = {B}, 3 chained layers] deviation / tolerance (3e-6: scores, max, sum, out; 2e-5: gradients): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    c.sync()


# ================================================================================================ inference form
@pytest.mark.parametrize("has_prev", [0, 1])
@pytest.mark.parametrize("L,B,heads", [(L, 2, 16) for L in (1, 7, 8, 9, 63, 64, 65, 139, 347)] + [(1024, 1, 1), (1025, 1, 1)])
def test_inference_attention_vs_exact(gpu_device, L, B, heads, has_prev):
    c = ctx(gpu_device)
    D = heads * DK
    qkv, _ = SM.random_inputs(B, L, 1, 6000 + 2 * L + has_prev, n_heads=heads)
    prev = 0.5 * torch.randn(B, heads, L, L, generator=torch.Generator().manual_seed(L))          # [b][h][key][query]

    def run(x, pv):
        qd = c.rows(x)
        sc = c.rows(pv) if has_prev else c.buf(B * heads * L, L)                                  # has_prev = 0: written only - a read would meet the sentinel
        out = c.buf(B * L, D)
        assert c.lib.ds_spec_attention(c.E._ptr(qd), c.E._ptr(sc), c.E._ptr(out), B, L, heads, DK, SCALE, has_prev, c.s()) == 0
        return sc, out
    (sc, out), (sc2, out2) = run(qkv[0], prev), run(qkv[0], prev)
    torch.cuda.synchronize()
    RS, R = B * heads * L, B * L
    assert same_bits(sc, sc2) and same_bits(out, out2), "two runs differ"
    owned_ok(sc, RS, "scores"); owned_ok(out, R, "out")
    if B > 1:
        sr, orr = run(qkv[0].flip(0), prev.flip(0))
        torch.cuda.synchronize()
        assert same_bits(sr[:RS].reshape(B, -1).flip(0), sc[:RS].reshape(B, -1)) and same_bits(orr[:R].reshape(B, -1).flip(0), out[:R].reshape(B, -1)), "batch order matters"
    pq = prev.transpose(-1, -2) if has_prev else None
    ex = SM.exact(qkv, SCALE, prev=pq, n_heads=heads)
    q, k, _ = SM.parts(qkv[0].double(), heads)
    bound = SM.dot_bound(q.abs(), k.abs(), DK, SCALE, pq)
    got_s = sc[:RS].cpu().reshape(B, heads, L, L).transpose(-1, -2)
    sh = dict(scores=share(got_s, ex["scores"][0], bound),
              out=per_head(SM.heads(out[:R].cpu().reshape(B, L, D), heads), SM.heads(ex["out"][0], heads)) / TOL["act"])
    print(f"[inference, L = {L}, B = {B}, heads = {heads}, has_prev = {has_prev}] scores deviation / bound {sh['scores']:.3f}, out deviation / 3e-6 {sh['out']:.3f}")
    assert max(sh.values()) <= 1.0, sh
    c.sync()
