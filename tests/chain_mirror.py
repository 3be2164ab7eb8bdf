"""Float64 yardstick of the fused bf16 row chains (csrc/ds_train_chain.hip; C-ABI and formulas: include/diffspectra_train.h), plain torch
on the CPU.  TEST INFRASTRUCTURE ONLY; pinned without a GPU by tests/test_chain_mirror_cpu.py, used by tests/test_train_chain_kernels.py.

One function per chain - ``pair_front_fwd``, ``pair_chain_fwd``, ``dir_chain_fwd``, ``node_chain_fwd``, ``dir_chain_bwd``,
``pair_chain_bwd``, ``node_chain_bwd`` - written from the header's formulas (dmt.py:37-48,113-116,136-169, layers.py:291-295,328-334), not
from the kernels and not from train_engine.py.  Arithmetic: the two operands of every product are rounded to bf16 (nearest even:
``Tensor.bfloat16()``, which the suite holds bit-equal to ``dst_pack_bf16_pieces``) - ``round_operands=False`` turns that off -, the
accumulation and everything else run in float64; dropout is ``oracle.philox.dropout_keep`` with the survivors scaled by 1 / (1 - p);
the Gaussian features use the project's constants (pi = 3.14159, std = |stds| + 1e-5); LayerNorm has eps 1e-6 and no affine.

STAGE-WISE USE.  Every function takes ``tape``: a dict of tensors of the chain's own stages.  A stage whose predecessor is in ``tape`` is
evaluated FROM THAT TENSOR and not from the mirror's own value of it: given a kernel's tape, f3 comes from the kernel's ye1, f4 from the
kernel's s3, ed from the kernel's X2, c2 from the kernel's sc0, df3 from the kernel's df4, ...  Both sides then round bit-identical fp32
values to bf16 and only the fp32 accumulation separates them.  Without a tape the stages chain through the mirror's own values (and,
with ``round_operands=False``, stay differentiable: the CPU tests run torch.autograd through the forward functions).

BOUNDS.  The product of two bf16 numbers is exact in fp32, so a product stage differs from this mirror by its accumulation error only:
per element at most gamma_K (|A| |W|^T + |bias|) for ANY summation order; ``out["bound"][stage]`` holds TWICE that with K + 2 terms,
``2 (K + 2) 2^-24 (|A| |W|^T + |bias|)``, from the rounded operands in float64.  Where a product's result is not written by the kernel
(the tanh pre-activation; de_tot, dye1, dzn, dh_tot, dy1 of the backward) the bound is carried through what follows it: times the
Lipschitz constant of tanh (1), times |gate| and the dropout scale, through the LayerNorm backward (``ln_bwd_bound``: it is linear in the
incoming gradient) and into the per-molecule sums."""
from __future__ import annotations

import numpy as np
import torch

from oracle import philox

U = 2.0 ** -24                      # unit roundoff of fp32
PI = 3.14159                        # the reference's truncated pi (layers.py:291-295)
LN_EPS = 1e-6


# ------------------------------------------------------------------------------------------------ layout
def tables(n_atoms):
    """The packed-ragged tables of a batch (include/diffspectra_hip.h): node rows molecule-major; pair rows = the pairs a < b of every
    molecule, molecule-major, a-major; directed row 2 p + dir (dir 0 = (row a, col b), dir 1 = (row b, col a))."""
    n = [int(v) for v in n_atoms]
    node_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    pa, pb, pm = [], [], []
    for m, k in enumerate(n):
        for a in range(k):
            for b in range(a + 1, k):
                pa.append(node_off[m] + a); pb.append(node_off[m] + b); pm.append(m)
    lt = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int64))
    pair_off = np.concatenate([[0], np.cumsum([k * (k - 1) // 2 for k in n])]).astype(np.int64)
    pa, pb, pm = lt(pa), lt(pb), lt(pm)
    dirs = torch.arange(2 * len(pa)) % 2
    rep = lambda t: t.repeat_interleave(2)
    return dict(B=len(n), Nn=int(node_off[-1]), Pp=int(pair_off[-1]), node_off=node_off, pair_off=pair_off,
                node_mol=lt(np.repeat(np.arange(len(n)), n)), pair_a=pa, pair_b=pb, pair_mol=pm,
                dir_row=torch.where(dirs == 0, rep(pa), rep(pb)), dir_col=torch.where(dirs == 0, rep(pb), rep(pa)), dir_pair=rep(torch.arange(len(pa))),
                dir_mol=rep(pm))


# ------------------------------------------------------------------------------------------------ random cases
# adaLN column offsets of the test cases: non-zero, distinct multiples of 4, the slices disjoint and in no particular order (dist_off is
# read as two scalars and may be odd)
OFFS = dict(node=dict(gate1_off=1032, shift_off=4, scale_off=520, gate2_off=264),
            pair=dict(gate1_off=1300, shift_off=1436, scale_off=1368, gate2_off=1504),
            dir=dict(shift_off=1572, scale_off=1832),
            front=dict(dist_off=2093, shift_off=2100, scale_off=2168))
ADA_MIN = 2240


def random_inputs(chain, tb, seed, ada_cols=ADA_MIN, p=0.1, block=3, drop_seed=20240917):
    """fp32 inputs of one chain (``front``, ``pair``, ``dir``, ``node``) and the gradients that arrive at its backward: inputs of order 1,
    weights of order 1 / sqrt(K), the adaLN table of order 0.3 over its full width, dropout streams 4 * block + site."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    w = lambda n, k: r(n, k) / k ** 0.5
    Nn, Pp, B = tb["Nn"], tb["Pp"], tb["B"]
    i = dict(OFFS[chain], ada=0.3 * r(B, ada_cols))
    drop = dict(p=float(p), seed=int(drop_seed))
    if chain == "front":
        i.update(pos=1.2 * r(Nn, 3), means=6.0 * torch.rand(63, generator=g), stds=(0.3 + torch.rand(63, generator=g)) * torch.sign(r(63)),
                 e_in=r(Pp, 64), Wee=w(64, 128), bee=0.3 * r(64), Wte=w(512, 64))
    elif chain == "pair":
        i.update(drop, stream3=4 * block + 2, stream4=4 * block + 3, u=r(Nn, 64), n2e_bias=0.3 * r(64), e_in=r(Pp, 64), feat=r(Pp, 64),
                 W3=w(128, 64), b3=0.3 * r(128), W4=w(64, 128), b4=0.3 * r(64), Wed=w(256, 128), bed=0.3 * r(256), Wro=w(16, 64), bro=0.3 * r(16),
                 de=r(Pp, 64), dro=r(Pp, 16), ded=r(Pp, 256))
    elif chain == "dir":
        i.update(ac=r(Nn, 512), ed=r(Pp, 256), W0=w(256, 256), b0=0.3 * r(256), W2=w(3, 256), dc2=r(2 * Pp, 3))
    elif chain == "node":
        i.update(drop, stream1=4 * block, stream2=4 * block + 1, h_in=r(Nn, 256), attn=r(Nn, 256), W1=w(512, 256), b1=0.3 * r(512), W2=w(256, 512),
                 b2=0.3 * r(256), Wac=w(512, 256), Wn=w(64, 256), bn=0.3 * r(64), dh=r(Nn, 256), drn=r(Nn, 64), dac=r(Nn, 512))
    else:
        raise KeyError(chain)
    return i


# ------------------------------------------------------------------------------------------------ pieces
def rb(x, on=True):
    """``x`` as float64, through bf16 (round to nearest even) when ``on``."""
    x = torch.as_tensor(x)
    return x.bfloat16().double() if on else x.double()


def product(A, W, bias=None, round_operands=True):
    """``A W^T + bias`` (W in torch Linear layout [out, in]): operands rounded to bf16, accumulated in float64."""
    y = rb(A, round_operands) @ rb(W, round_operands).T
    return y if bias is None else y + torch.as_tensor(bias).double()


def product_bound(terms, addend=None):
    """``2 (K + 2) 2^-24 (sum_i |A_i| |W_i|^T + |addend|)`` for a sum of products ``A_i W_i^T`` accumulated in fp32 onto ``addend`` (a bias, a
    residual gradient), K = the total number of products per element."""
    K = sum(int(A.shape[1]) for A, _ in terms)
    m = sum(rb(A).abs() @ rb(W).abs().T for A, W in terms)
    if addend is not None:
        m = m + torch.as_tensor(addend).double().abs()
    return 2.0 * (K + 2) * U * m


def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def gelu(x):
    """GELU in its erf form (torch's default)."""
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * np.pi) ** 0.5


def dtanh_of_output(y):
    """tanh'(x) from y = tanh(x): the backward keeps the activated tensor."""
    return 1.0 - y * y


# sup |f'| of the three activations (SiLU: 1.09984 at x = 2.3994, GELU: 1.12899 at x = sqrt 2, tanh: 1), rounded up: what an error in front
# of the activation can grow to behind it
LIPSCHITZ = dict(silu=1.1, gelu=1.13, tanh=1.0)


def ln_stats(x):
    """(mean, rstd) of every row: biased variance, eps 1e-6."""
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + LN_EPS)


def ln_bwd(dy, x, mean, rstd, scale):
    """Backward of ``y = xhat (1 + scale) + shift``, ``xhat = (x - mean) rstd``, from the SAVED statistics: (dx, xhat)."""
    xh = (x - mean) * rstd
    g = dy * (1.0 + scale)
    return rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)), xh


def ln_bwd_bound(b, xh, rstd, scale):
    """What a per-element perturbation of at most ``b`` of the incoming gradient can do to ``ln_bwd``'s dx (the map is linear in dy)."""
    gb = b * (1.0 + scale).abs()
    return rstd.abs() * (gb + gb.mean(1, keepdim=True) + xh.abs() * (gb * xh.abs()).mean(1, keepdim=True))


def keep_scaled(seed, stream, rows, cols, p):
    """The dropout mask of the contiguous [rows, cols] tensor under Philox stream ``stream``: element (row, col) has index row * cols + col;
    (bool keep, float64 keep / (1 - p)).  The kernels hold p as fp32: 1 - p is taken from that value."""
    if not p > 0.0:
        keep = torch.ones(rows, cols, dtype=torch.bool)
        return keep, keep.double()
    keep = torch.from_numpy(np.ascontiguousarray(philox.dropout_keep(seed, stream, rows * cols, p))).reshape(rows, cols)
    return keep, keep.double() / (1.0 - float(np.float32(p)))


def seg_sum(x, mol, B):
    """[B, C]: the sum of the rows of every molecule (zero for a molecule without rows)."""
    return torch.zeros(B, x.shape[1], dtype=torch.float64).index_add_(0, mol, x)


def _cols(ada, mol, off, C):
    return ada[mol, off:off + C]


class _Run:
    """The stages of one evaluation: ``prev(k)`` = the tape's tensor of stage ``k`` if there is one, else the mirror's own."""

    def __init__(self, tape, round_operands):
        self.tape, self.r, self.out, self.bound = tape or {}, round_operands, {}, {}

    def prev(self, k):
        t = self.tape.get(k)
        return self.out[k] if t is None else torch.as_tensor(t).double()

    def done(self, **extra):
        self.out.update(extra)
        self.out["bound"] = self.bound
        return self.out


# ------------------------------------------------------------------------------------------------ forward chains
def pair_front_fwd(tb, i, tape=None, round_operands=True):
    """dst_pair_front_fwd.  ``i``: pos [Nn,3], ada [B,ADA], dist_off, shift_off, scale_off, means, stds [63], e_in [Pp,64], Wee [64,128], bee,
    Wte [512,64].  Stages: d2, xs, X1 = [x', 63 Gaussians | e_in], e1, st, en, te."""
    R = _Run(tape, round_operands)
    o, pm, ada = R.out, tb["pair_mol"], i["ada"].double()
    d = i["pos"].double()[tb["pair_a"]] - i["pos"].double()[tb["pair_b"]]
    o["d2"] = (d * d).sum(1)
    o["xs"] = R.prev("d2").reshape(-1) * (1.0 + ada[pm, i["dist_off"]]) + ada[pm, i["dist_off"] + 1]
    sd = i["stds"].double().abs() + 1e-5
    x = R.prev("xs").reshape(-1, 1)
    gauss = torch.exp(-0.5 * ((x - i["means"].double()) / sd) ** 2) / ((2.0 * PI) ** 0.5 * sd)
    o["X1"] = torch.cat([x, gauss, i["e_in"].double()], 1)
    X1 = R.prev("X1")
    o["e1"] = product(X1, i["Wee"], i["bee"], R.r)
    e1 = R.prev("e1")
    mean, rstd = ln_stats(e1)
    o["st"] = torch.cat([mean, rstd], 1)
    o["en"] = (e1 - mean) * rstd * (1.0 + _cols(ada, pm, i["scale_off"], 64)) + _cols(ada, pm, i["shift_off"], 64)
    en = R.prev("en")
    o["te_pre"] = product(en, i["Wte"], None, R.r)
    o["te"] = torch.tanh(o["te_pre"])
    if R.r:
        R.bound["e1"] = product_bound([(X1, i["Wee"])], i["bee"])
        R.bound["te"] = product_bound([(en, i["Wte"])])                  # |tanh'| <= 1
    return R.done()


def pair_chain_fwd(tb, i, tape=None, round_operands=True):
    """dst_pair_chain_fwd.  ``i``: u [Nn,64], n2e_bias, e_in [Pp,64], feat [Pp,64], ada, gate1_off, shift_off, scale_off, gate2_off, W3 [128,64],
    b3, W4 [64,128], b4, Wed [256,128] (e | dist), bed, Wro [16,64], bro, p, seed, stream3, stream4.  Stages: he, xe1, st, ye1, f3, s3, f4,
    e_out, X2, ed, ro (+ f4_pre: ff_linear4's output in front of its dropout)."""
    R = _Run(tape, round_operands)
    o, pm, ada, Pp = R.out, tb["pair_mol"], i["ada"].double(), tb["Pp"]
    col = lambda k: _cols(ada, pm, i[k], 64)
    k3, m3 = keep_scaled(i["seed"], i["stream3"], Pp, 128, i["p"])
    k4, m4 = keep_scaled(i["seed"], i["stream4"], Pp, 64, i["p"])
    u = i["u"].double()
    o["he"] = u[tb["pair_a"]] + u[tb["pair_b"]] + i["n2e_bias"].double()
    o["xe1"] = i["e_in"].double() + col("gate1_off") * R.prev("he")
    xe1 = R.prev("xe1")
    mean, rstd = ln_stats(xe1)
    o["st"] = torch.cat([mean, rstd], 1)
    o["ye1"] = (xe1 - mean) * rstd * (1.0 + col("scale_off")) + col("shift_off")
    ye1 = R.prev("ye1")
    o["f3"] = product(ye1, i["W3"], i["b3"], R.r)
    o["s3"] = silu(R.prev("f3")) * m3
    s3 = R.prev("s3")
    o["f4_pre"] = product(s3, i["W4"], i["b4"], R.r)
    o["f4"] = o["f4_pre"] * m4
    o["e_out"] = ye1 + col("gate2_off") * R.prev("f4")
    e_out = R.prev("e_out")
    o["X2"] = torch.cat([e_out, i["feat"].double()], 1)
    X2 = R.prev("X2")
    o["ed"] = product(X2, i["Wed"], i["bed"], R.r)
    o["ro"] = product(e_out, i["Wro"], i["bro"], R.r)
    if R.r:
        R.bound.update(f3=product_bound([(ye1, i["W3"])], i["b3"]), f4=product_bound([(s3, i["W4"])], i["b4"]) * m4,
                       ed=product_bound([(X2, i["Wed"])], i["bed"]), ro=product_bound([(e_out, i["Wro"])], i["bro"]))
    return R.done(keep3=k3, keep4=k4)


def dir_chain_fwd(tb, i, tape=None, round_operands=True):
    """dst_dir_chain_fwd.  ``i``: ac [Nn,512], ed [Pp,256], ada, shift_off, scale_off, W0 [256,256], b0, W2 [3,256].  Stages: zz, st, zn, c0, sc0, c2."""
    R = _Run(tape, round_operands)
    o, dm, ada = R.out, tb["dir_mol"], i["ada"].double()
    ac = i["ac"].double()
    o["zz"] = ac[tb["dir_row"], :256] + ac[tb["dir_col"], 256:] + i["ed"].double()[tb["dir_pair"]]
    zz = R.prev("zz")
    mean, rstd = ln_stats(zz)
    o["st"] = torch.cat([mean, rstd], 1)
    o["zn"] = (zz - mean) * rstd * (1.0 + _cols(ada, dm, i["scale_off"], 256)) + _cols(ada, dm, i["shift_off"], 256)
    zn = R.prev("zn")
    o["c0"] = product(zn, i["W0"], i["b0"], R.r)
    o["sc0"] = silu(R.prev("c0"))
    sc0 = R.prev("sc0")
    o["c2"] = product(sc0, i["W2"], None, R.r)
    if R.r:
        R.bound.update(c0=product_bound([(zn, i["W0"])], i["b0"]), c2=product_bound([(sc0, i["W2"])]))
    return R.done()


def node_chain_fwd(tb, i, tape=None, round_operands=True):
    """dst_node_chain_fwd.  ``i``: h_in, attn [Nn,256], ada, gate1_off, shift_off, scale_off, gate2_off, W1 [512,256], b1, W2 [256,512], b2,
    Wac [512,256], Wn [64,256], bn, p, seed, stream1, stream2.  Stages: x1, st, y1, f1, s1, f2, h_out, ac, rn (+ f2_pre)."""
    R = _Run(tape, round_operands)
    o, nm, ada, Nn = R.out, tb["node_mol"], i["ada"].double(), tb["Nn"]
    col = lambda k: _cols(ada, nm, i[k], 256)
    k1, m1 = keep_scaled(i["seed"], i["stream1"], Nn, 512, i["p"])
    k2, m2 = keep_scaled(i["seed"], i["stream2"], Nn, 256, i["p"])
    o["x1"] = i["h_in"].double() + col("gate1_off") * i["attn"].double()
    x1 = R.prev("x1")
    mean, rstd = ln_stats(x1)
    o["st"] = torch.cat([mean, rstd], 1)
    o["y1"] = (x1 - mean) * rstd * (1.0 + col("scale_off")) + col("shift_off")
    y1 = R.prev("y1")
    o["f1"] = product(y1, i["W1"], i["b1"], R.r)
    o["s1"] = silu(R.prev("f1")) * m1
    s1 = R.prev("s1")
    o["f2_pre"] = product(s1, i["W2"], i["b2"], R.r)
    o["f2"] = o["f2_pre"] * m2
    o["h_out"] = y1 + col("gate2_off") * R.prev("f2")
    h_out = R.prev("h_out")
    o["ac"] = product(h_out, i["Wac"], None, R.r)
    o["rn"] = product(h_out, i["Wn"], i["bn"], R.r)
    if R.r:
        R.bound.update(f1=product_bound([(y1, i["W1"])], i["b1"]), f2=product_bound([(s1, i["W2"])], i["b2"]) * m2,
                       ac=product_bound([(h_out, i["Wac"])]), rn=product_bound([(h_out, i["Wn"])], i["bn"]))
    return R.done(keep1=k1, keep2=k2)


# ------------------------------------------------------------------------------------------------ backward chains
def dir_chain_bwd(tb, i, tape=None, round_operands=True):
    """dst_dir_chain_bwd.  ``i``: dc2 [2 Pp,3], c0, zz [2 Pp,256], st [2 Pp,2] (the forward's tape), ada, shift_off, scale_off, W2 [3,256] (fp32: a
    K = 3 product of plain FMAs, no rounding), W0 [256,256].  Stages: dc0, dz; d_ada = {shift, scale} [B,256].  dzn is not written."""
    R = _Run(tape, round_operands)
    o, dm, ada, B = R.out, tb["dir_mol"], i["ada"].double(), tb["B"]
    sc = _cols(ada, dm, i["scale_off"], 256)
    o["dc0"] = (i["dc2"].double() @ i["W2"].double()) * dsilu(i["c0"].double())
    dc0 = R.prev("dc0")
    o["dzn"] = product(dc0, i["W0"].T, None, R.r)
    st = i["st"].double()
    o["dz"], xh = ln_bwd(o["dzn"], i["zz"].double(), st[:, :1], st[:, 1:2], sc)
    d_ada = dict(shift=seg_sum(o["dzn"], dm, B), scale=seg_sum(o["dzn"] * xh, dm, B))
    if R.r:
        b = product_bound([(dc0, i["W0"].T)])
        R.bound.update(dz=ln_bwd_bound(b, xh, st[:, 1:2], sc), d_ada=dict(shift=seg_sum(b, dm, B), scale=seg_sum(b * xh.abs(), dm, B)))
    return R.done(d_ada=d_ada)


def _rear_bwd(R, i, mol, B, C, names, grads, tapes, weights, keeps):
    """The common shape of the pair- and node-row backward behind the attention (header: dst_pair_bwd_args / dst_node_bwd_args).
    ``names`` = (d_ffout, d_ffpre, d_in, d_gated), ``grads`` = (d_out, [(gradient, weight)] of the products that add to it),
    ``tapes`` = (ff_out, ff_pre, x, st, gated), ``weights`` = (W_ffout, W_ffpre), ``keeps`` = (mask of ff_out, mask of ff_pre)."""
    o, ada = R.out, i["ada"].double()
    n_ffout, n_ffpre, n_in, n_gated = names
    d_out, adds = grads
    ff_out, ff_pre, x, st, gated = (t.double() for t in tapes)
    W_ffout, W_ffpre = weights
    m_out, m_pre = keeps
    col = lambda k: _cols(ada, mol, i[k], C)
    terms = [(g, W.T) for g, W in adds]
    tot = d_out.double() + sum(product(g, Wt, None, R.r) for g, Wt in terms)                  # de_tot / dh_tot: not written
    o[n_ffout] = col("gate2_off") * tot * m_out
    dff = R.prev(n_ffout)
    o[n_ffpre] = product(dff, W_ffout.T, None, R.r) * dsilu(ff_pre) * m_pre
    dpre = R.prev(n_ffpre)
    dy = tot + product(dpre, W_ffpre.T, None, R.r)                                             # dye1 / dy1: not written
    sc = col("scale_off")
    dx, xh = ln_bwd(dy, x, st[:, :1], st[:, 1:2], sc)
    o[n_in], o[n_gated] = dx, col("gate1_off") * dx
    d_ada = dict(gate2=seg_sum(tot * ff_out, mol, B), shift=seg_sum(dy, mol, B), scale=seg_sum(dy * xh, mol, B), gate1=seg_sum(dx * gated, mol, B))
    if R.r:
        b_tot = product_bound(terms, d_out)
        b_dy = product_bound(terms + [(dpre, W_ffpre.T)], d_out)
        b_dx = ln_bwd_bound(b_dy, xh, st[:, 1:2], sc)
        R.bound.update({n_ffout: col("gate2_off").abs() * b_tot * m_out, n_ffpre: product_bound([(dff, W_ffout.T)]) * dsilu(ff_pre).abs() * m_pre,
                        n_in: b_dx, n_gated: col("gate1_off").abs() * b_dx,
                        "d_ada": dict(gate2=seg_sum(b_tot * ff_out.abs(), mol, B), shift=seg_sum(b_dy, mol, B), scale=seg_sum(b_dy * xh.abs(), mol, B),
                                      gate1=seg_sum(b_dx * gated.abs(), mol, B))})
    return tot, dy, d_ada


def pair_chain_bwd(tb, i, tape=None, round_operands=True):
    """dst_pair_chain_bwd.  ``i``: de [Pp,64], dro [Pp,16], ded [Pp,256], the forward's tape f4, f3, xe1, st, he, ada and the four offsets, Wed
    [256,128], Wro [16,64], W4 [64,128], W3 [128,64] (torch Linear layout: the mirror transposes), p, seed, stream3, stream4.  Stages: dfeat, df4,
    df3, de_in, dhe; d_ada = {gate1, shift, scale, gate2} [B,64].  de_tot and dye1 are not written."""
    R = _Run(tape, round_operands)
    Pp, B = tb["Pp"], tb["B"]
    _, m3 = keep_scaled(i["seed"], i["stream3"], Pp, 128, i["p"])
    _, m4 = keep_scaled(i["seed"], i["stream4"], Pp, 64, i["p"])
    Wed = torch.as_tensor(i["Wed"])
    R.out["dfeat"] = product(i["ded"], Wed[:, 64:128].T, None, R.r)
    if R.r:
        R.bound["dfeat"] = product_bound([(i["ded"], Wed[:, 64:128].T)])
    tot, dy, d_ada = _rear_bwd(R, i, tb["pair_mol"], B, 64, ("df4", "df3", "de_in", "dhe"),
                               (i["de"], [(i["ded"], Wed[:, :64]), (i["dro"], i["Wro"])]), (i["f4"], i["f3"], i["xe1"], i["st"], i["he"]),
                               (i["W4"], i["W3"]), (m4, m3))
    return R.done(d_ada=d_ada, de_tot=tot, dye1=dy)


def node_chain_bwd(tb, i, tape=None, round_operands=True):
    """dst_node_chain_bwd.  ``i``: dh [Nn,256], drn [Nn,64], dac [Nn,512], the forward's tape f2, f1, x1, st, attn, ada and the four offsets, Wac
    [512,256], Wn [64,256], W2 [256,512], W1 [512,256], p, seed, stream1, stream2.  Stages: df2, df1, dh_in, dattn; d_ada = {gate1, shift, scale,
    gate2} [B,256].  dh_tot and dy1 are not written."""
    R = _Run(tape, round_operands)
    Nn, B = tb["Nn"], tb["B"]
    _, m1 = keep_scaled(i["seed"], i["stream1"], Nn, 512, i["p"])
    _, m2 = keep_scaled(i["seed"], i["stream2"], Nn, 256, i["p"])
    tot, dy, d_ada = _rear_bwd(R, i, tb["node_mol"], B, 256, ("df2", "df1", "dh_in", "dattn"),
                               (i["dh"], [(i["dac"], i["Wac"]), (i["drn"], i["Wn"])]), (i["f2"], i["f1"], i["x1"], i["st"], i["attn"]),
                               (i["W2"], i["W1"]), (m2, m1))
    return R.done(d_ada=d_ada, dh_tot=tot, dy1=dy)
