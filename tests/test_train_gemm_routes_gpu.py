"""dst_gemm route by route against float64: every case of tests/gemm_route_cases.py runs through ``Ops.gemm`` and is compared with the
product of the (bf16-rounded, where the kernel rounds) operands accumulated in float64 on the CPU.  tests/test_train_gemm_routes_cpu.py
holds every case on the kernel it was built for; here ``Ops.gemm_route`` confirms it once more with the real addresses.

BOUND (derived, not measured), per element:  ``|got - ref| <= 2 (K + 3) 2^-24 (|A| |B| + |bias| + |C_old| + |ref|)`` - ``|ref|`` for the
residual add (dact 4), ``|C_old|`` when accumulating, operands rounded where the kernel rounds.  gamma_{K+3} bounds an fp32 sum of K exact
products, a bias and an old value in ANY order with one more rounding per product for the fp32 MFMA; the factor two leaves room for the
roundings behind the sum (slices and the reduce kernel add nothing: they are another order of the same sum).  A dropout survivor is scaled
by 1 / (1 - p): so is its allowance.  The row sum is the same product with B = ones.

Activation stages are teacher-forced like the chain tests': C2 against ``f(C_kernel) * keep`` in float64 from the kernel's own C, limit 3e-6
of the largest reference value (``TOL["act"]`` of tests/test_train_chain_kernels.py).  Where the kernel writes no pre-activation (``act``
without C2, ``dact`` 1..3) the product bound is carried through the activation - times sup |f'| (``chain_mirror.LIPSCHITZ``), respectively
times ``|f'(ref)|`` - plus those 3e-6.  Dropout masks are exact: the zeroed positions are ``oracle.philox`` at index ``m * drop_ld + n``
(an element without allowance must be exact, so a dropped element is an exact zero and a survivor is not - except where the reference
itself is zero, or, behind an activation, below the activation's tolerance: fp32 GELU of a pre-activation below -5.5 is -0.0).

BUFFERS.  A and B are windows of NaN-filled tensors (the columns between extent and leading stride, GUARD_ROWS rows behind the last, an
offset in front): INTEGRATION.md only asks for those locations to be readable, the vector kernels do load them and select them away, and
a NaN in any output is a leak.  C, C2, the row sum and the split-K scratch are windows of sentinel-filled tensors: everything outside
the window stays bit-unchanged.  Every case runs twice from the same initial state: bit-identical (a fixed summation order is promised).

Every case prints ``deviation/share`` = the largest error over its allowance; the fixture's teardown prints the largest per route."""
import zlib

import pytest
import torch

from tests import chain_mirror as CM
from tests import gemm_route_cases as G
from tests.gemm_route_cases import ADDREF, GELU, SILU, TANH

pytestmark = pytest.mark.gpu

SENT = -123456.75                 # what surrounds every output window
TOL_ACT = 3e-6
U2 = lambda K: 2.0 * (K + 3) * CM.U
ACT = {SILU: (CM.silu, CM.dsilu, CM.LIPSCHITZ["silu"]), GELU: (CM.gelu, CM.dgelu, CM.LIPSCHITZ["gelu"]),
       TANH: (torch.tanh, CM.dtanh_of_output, CM.LIPSCHITZ["tanh"])}
_SCRATCH_GUARD = 4096


class Env:
    def __init__(self, d):
        import __graft_entry__ as g
        g.build()
        G.assert_no_knob()
        from diffspectra_amd import train_engine as T
        self.T, self.d, self.o = T, d, T.Ops(d)
        self.own_scratch = self.o.scratch
        self.S = torch.full((_SCRATCH_GUARD + G.SCRATCH_FLOATS + _SCRATCH_GUARD,), SENT, device=d)
        self.names = {T.abi.TRAINING.consts[n]: n for n in (G.WS, G.SKINNY, G.SKINNY4, G.BF16, G.BIG)}
        self.operands, self.products, self.keeps, self.shares = {}, {}, {}, {}


@pytest.fixture(scope="module")
def env(gpu_device):
    e = Env(gpu_device)
    yield e
    torch.cuda.synchronize()
    e.o.scratch = e.own_scratch
    for route, (share, name) in sorted(e.shares.items(), key=str):
        print(f"[dst_gemm routes] largest deviation/share {share:.4f} on {route} ({name})")
    e.operands.clear(), e.products.clear(), e.keeps.clear()


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _window(rows, cols, ld, off, data):
    """``data`` [rows, cols] inside a NaN tensor: ``off`` floats in front, rows of ``ld``, GUARD_ROWS rows behind."""
    full = torch.full((off + (rows + G.GUARD_ROWS) * ld,), float("nan"))
    full[off:].view(rows + G.GUARD_ROWS, ld)[:rows, :cols] = data
    return full


def _operands(env, c):
    """(A values [M, K], B values [K, N], MV of A, MV of B) of the case's product; epilogue variants of one product share them, the ws cases
    share ONE A of 65573 x 512 (plus NaN guard rows) as column windows.  The device tensors stay referenced by ``env`` to the end."""
    base = c.name.split("/")[0]
    if base in env.operands:
        return env.operands[base]
    T, d, lay = env.T, env.d, G.operand_layout(c)
    g = _gen(base)
    if c.family == "ws":
        if "ws A" not in env.operands:
            a = torch.randn(c.M, G.WS_LDA, generator=_gen("ws A"))
            env.operands["ws A"] = (a, _window(c.M, G.WS_LDA, G.WS_LDA, 0, a).to(d))
        a_all, a_dev = env.operands["ws A"]
        a_val, mvA = a_all[:, :c.K], T.MV(a_dev, c.M, c.K, G.WS_LDA, 0)
    else:
        rows, cols, ld, off = lay["A"]
        if c.a_bcast:                                                          # one row of K values, read by every m
            row = torch.randn(1, cols, generator=g)
            full = torch.full((off + G.r4(cols) + 8,), float("nan"))
            full[off:off + cols] = row[0]
            stored = row.expand(rows, cols)
        else:
            stored = torch.randn(rows, cols, generator=g)
            full = _window(rows, cols, ld, off, stored)
        a_val, mvA = (stored.t() if c.ta else stored), T.MV(full.to(d), rows, cols, ld, off)
    rows, cols, ld, off = lay["B"]
    stored = torch.randn(rows, cols, generator=g) * 0.25
    b_val, mvB = (stored.t() if c.tb else stored), T.MV(_window(rows, cols, ld, off, stored).to(d), rows, cols, ld, off)
    env.operands[base] = (a_val, b_val, mvA, mvB)
    return env.operands[base]


def _product(env, c, a_val, b_val, rounded):
    """float64: (A B, |A| |B|, row sums of A, of |A|) from the operands as the kernel sees them; blocked over rows."""
    key = (c.name.split("/")[0], rounded)
    if key not in env.products:
        b = CM.rb(b_val, rounded)
        P, Q = torch.empty(c.M, c.N, dtype=torch.float64), torch.empty(c.M, c.N, dtype=torch.float64)
        rs, rq = torch.empty(c.M, dtype=torch.float64), torch.empty(c.M, dtype=torch.float64)
        for r0 in range(0, c.M, 16384):
            a = CM.rb(a_val[r0:r0 + 16384], rounded)
            P[r0:r0 + 16384], Q[r0:r0 + 16384] = a @ b, a.abs() @ b.abs()
            rs[r0:r0 + 16384], rq[r0:r0 + 16384] = a.sum(1), a.abs().sum(1)
        env.products[key] = (P, Q, rs, rq)
    return env.products[key]


def _keep(env, M, ld, N, p):
    key = (M, ld, p)
    if key not in env.keeps:
        env.keeps[key] = CM.keep_scaled(G.DROP_SEED, G.DROP_STREAM, M, ld, p)
    k, ks = env.keeps[key]
    return k[:, :N], ks[:, :N]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _share(err, allow, what, name):
    """Largest error over its allowance; an element without allowance (a dropped one, an empty sum) must be exact."""
    assert not torch.isnan(err).any(), f"{name}: NaN in {what}: a padding or guard element leaked through a clamped load (or an element was not written)"
    exact = allow == 0
    assert bool((err[exact] == 0).all()), f"{name}: {what} differs where the reference is exact ({int((err[exact] != 0).sum())} elements)"
    return float((err[~exact] / allow[~exact]).max()) if bool((~exact).any()) else 0.0


def run_case(env, c):
    T, d, o, e = env.T, env.d, env.o, c.epi
    M, N, K = c.M, c.N, c.K
    a_val, b_val, mvA, mvB = _operands(env, c)
    out = G.output_layout(c)
    g = _gen(c.name + " outputs")
    # ---- outputs: windows of sentinel tensors; inside the window the old value (accumulate) or NaN (every element must be written)
    def out_tensor(key, old):
        ld, col0 = out[key]
        full = torch.full((M + G.GUARD_ROWS, ld), SENT)
        full[:M, col0:col0 + N] = old if old is not None else float("nan")
        return full, T.MV(full.to(d, copy=True), M, N, ld, col0)
    c_old = torch.randn(M, N, generator=g) if e.acc else None
    C0, mvC = out_tensor("C", c_old)
    C20, mvC2 = out_tensor("C2", None) if e.c2 else (None, None)
    r_old = torch.randn(M, generator=g) if (c.rowsum and e.acc) else None
    R0 = torch.full((8 + M + G.GUARD_ROWS,), SENT)
    R0[8:8 + M] = r_old if r_old is not None else float("nan")
    Rd = R0.to(d, copy=True)
    ref_val = mvRef = None
    if e.dact:
        ref_val = torch.randn(M, N, generator=g)
        if e.dact == TANH:
            ref_val = torch.tanh(ref_val)                                      # tanh' takes the activated value
        ld, col0 = out["ref"]
        full = torch.full((M + G.GUARD_ROWS, ld), float("nan"))
        full[:M, col0:col0 + N] = ref_val
        mvRef = T.MV(full.to(d), M, N, ld, col0)
    bias = torch.randn(N, generator=g) if e.bias else None
    bias_d = bias.to(d) if e.bias else None
    drop = (e.p, G.DROP_SEED, G.DROP_STREAM, out["drop_ld"]) if e.p > 0.0 else None
    # ---- scratch: a slice of the sentinel tensor, or NULL
    n = G.scratch_floats(c)
    env.S.fill_(SENT)
    # (an address and a length: a zero-length slice of a tensor reports a NULL data pointer, and the empty scratch must not be NULL)
    o.scratch = G.FakeTensor(0, 0) if n is None else G.FakeTensor(env.S.data_ptr() + 4 * _SCRATCH_GUARD, n)
    o.bf16 = c.bf16
    args = (mvA, mvB, mvC, c.ta, c.tb)
    kw = dict(bias=bias_d, acc=e.acc, rowsum=Rd[8:8 + M] if c.rowsum else None, act=e.act, dact=e.dact, ref=mvRef, out2=mvC2, drop=drop)
    r = o.gemm_route(*args, **kw)
    route = (env.names[r.kernel], r.BM, r.BN, r.threads, r.slices > 1, r.a_rfast, r.b_rfast)
    assert route == c.route and r.epilogue == G.epi_bits(c), f"{c.name}: built for {c.route} / epilogue bits {G.epi_bits(c)}, runs {route} / {r.epilogue}"
    # ---- twice from the same initial state
    got = []
    for _ in range(2):
        mvC.t.copy_(C0)
        if e.c2:
            mvC2.t.copy_(C20)
        Rd.copy_(R0)
        o.gemm(*args, **kw)
        got.append((mvC.t.clone(), mvC2.t.clone() if e.c2 else None, Rd.clone()))
    torch.cuda.synchronize()                                                   # every operand above is still referenced here
    for x, y in zip(got[0], got[1]):
        assert x is None or torch.equal(_bits(x), _bits(y)), f"{c.name}: two runs differ"
    assert bool((env.S[:_SCRATCH_GUARD] == SENT).all()) and bool((env.S[_SCRATCH_GUARD + (n or 0):] == SENT).all()), f"{c.name}: scratch written outside partial_cap"
    Cg, C2g, Rg = (None if x is None else x.cpu() for x in got[0])
    # ---- nothing outside the windows
    def outside_unchanged(full, init, key):
        ld, col0 = out[key]
        a, b = full.clone(), init.clone()
        a[:M, col0:col0 + N], b[:M, col0:col0 + N] = 0.0, 0.0
        assert torch.equal(_bits(a), _bits(b)), f"{c.name}: {key} written outside its window"
        return full[:M, col0:col0 + N].double()
    Cw = outside_unchanged(Cg, C0, "C")
    C2w = outside_unchanged(C2g, C20, "C2") if e.c2 else None
    if c.rowsum:
        assert torch.equal(_bits(Rg[:8]), _bits(R0[:8])) and torch.equal(_bits(Rg[8 + M:]), _bits(R0[8 + M:])), f"{c.name}: row sum written outside its window"
    else:
        assert torch.equal(_bits(Rg), _bits(R0))
    # ---- reference and allowance
    rounded = bool(r.bf16)
    P, Q, rs, rq = _product(env, c, a_val, b_val, rounded)
    u2 = U2(K)
    v, mag = P.clone(), Q.clone()
    if e.bias:
        v, mag = v + bias.double(), mag + bias.double().abs()
    extra = 0.0
    if e.dact == ADDREF:
        v, mag = v + ref_val.double(), mag + ref_val.double().abs()
    elif e.dact:
        dv = ACT[e.dact][1](ref_val.double())
        v, mag, extra = v * dv, mag * dv.abs(), TOL_ACT
    keep, ks = _keep(env, M, out["drop_ld"], N, e.p) if e.p > 0.0 else (torch.ones(M, N, dtype=torch.bool), torch.ones(M, N, dtype=torch.float64))
    shares = {}
    if e.act:
        f, _, lip = ACT[e.act]
        if e.c2:
            shares["C"] = _share((Cw - v).abs(), u2 * mag, "C", c.name)
            want2 = f(Cw) * ks                                                  # teacher-forced: from the kernel's own pre-activation
            err2 = (C2w - want2).abs()
            assert not torch.isnan(err2).any(), f"{c.name}: NaN in C2"
            shares["C2"] = float(err2.max() / (TOL_ACT * want2.abs().max()))
            if e.p > 0.0:
                # every dropped position is an exact zero; a survivor is zero only where the activation itself vanishes within its tolerance
                # (fp32 GELU of a pre-activation below -5.5 is -0.0: erff has reached -1)
                tiny = want2.abs() <= TOL_ACT * want2.abs().max()
                assert bool((C2w[~keep] == 0).all()) and bool((C2w[keep & ~tiny] != 0).all()), \
                    f"{c.name}: the zeroed positions of C2 are not the Philox mask at m * {out['drop_ld']} + n"
        else:
            want = f(v) * ks
            shares["C"] = _share((Cw - want).abs(), (lip * u2 * mag * ks + TOL_ACT * want.abs().max()) * keep, "C", c.name)
    else:
        want = v * ks + (c_old.double() if e.acc else 0.0)
        allow = u2 * (mag * ks + (c_old.double().abs() if e.acc else 0.0)) + (extra * want.abs().max()) * (keep | e.acc)
        shares["C"] = _share((Cw - want).abs(), allow, "C", c.name)
        if e.p > 0.0 and not e.acc:
            assert torch.equal(Cw == 0, ~keep | (v == 0)), f"{c.name}: the zeroed positions of C are not the Philox mask at m * {out['drop_ld']} + n"
    if c.rowsum:
        wantr = rs + (r_old.double() if r_old is not None else 0.0)
        shares["rowsum"] = _share((Rg[8:8 + M].double() - wantr).abs(), u2 * (rq + (r_old.double().abs() if r_old is not None else 0.0)), "row sum", c.name)
    share = max(shares.values())
    print(f"{c.name}: route {route} slices {r.slices} x k {r.k_per_slice}, epilogue bits {r.epilogue}: deviation/share "
          + ", ".join(f"{k} {s:.4f}" for k, s in shares.items()))
    rk = route[:5] + (("bf16" if r.bf16 else "fp32"),)
    if share > env.shares.get(rk, (-1.0, ""))[0]:
        env.shares[rk] = (share, c.name)
    assert share <= 1.0, f"{c.name}: error {share:.3f} x its allowance ({shares})"


@pytest.mark.parametrize("c", G.BASE + G.K0, ids=lambda c: c.name)
def test_product(env, c):
    run_case(env, c)


@pytest.mark.parametrize("c", G.EPILOGUES, ids=lambda c: c.name)
def test_epilogue(env, c):
    run_case(env, c)
