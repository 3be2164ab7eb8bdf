"""Pins tests/chain_mirror.py - the float64 yardstick the fused row chains of csrc/ds_train_chain.hip are held to by
tests/test_train_chain_kernels.py - WITHOUT a GPU:

* with ``round_operands=False`` every forward mirror equals the same block piece written with ``torch.nn.functional`` (layer_norm, linear,
  silu, tanh) in float64, to 1e-12;
* with ``round_operands=False`` every backward mirror equals ``torch.autograd`` through that forward, to 1e-10: every output and every
  ``d_ada`` slice, with dropout 0.1 (the Philox masks are constants of the graph);
* with the rounding on, the product stages equal ``F.linear`` on ``.bfloat16().double()`` operands to 1e-12, and a stage whose predecessor
  is in the tape is evaluated from the tape;
* the mask convention - element ``row * N + col`` of stream ``4 * block + site`` - is the one ``oracle.train.dropout_masks`` injects into
  the reference (golden G17).

The error measure is the suite's own (``tests.helpers.relerr``): max |a - b| / max |b|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train as otrain
from tests import chain_mirror as CM
from tests.helpers import relerr

N_ATOMS = [3, 1, 9, 2, 5, 1]          # two molecules without a pair, one in the middle and one last
P = 0.1


def _case(chain, seed=3, grad=False):
    tb = CM.tables(N_ATOMS)
    i = CM.random_inputs(chain, tb, seed, p=P)
    i = {k: (v.double().requires_grad_(grad) if torch.is_tensor(v) else v) for k, v in i.items()}
    return tb, i


def _ada(i, mol, key, C):
    return i["ada"][mol, i[key]:i[key] + C]


# ------------------------------------------------------------------------------------------------ the chains written with torch.nn.functional
def _front_functional(tb, i):
    pm = tb["pair_mol"]
    d2 = ((i["pos"][tb["pair_a"]] - i["pos"][tb["pair_b"]]) ** 2).sum(1)
    xs = d2 * (1 + i["ada"][pm, i["dist_off"]]) + i["ada"][pm, i["dist_off"] + 1]
    std = i["stds"].abs() + 1e-5
    gauss = torch.exp(-0.5 * ((xs[:, None] - i["means"]) / std) ** 2) / ((2 * 3.14159) ** 0.5 * std)       # layers.py:291-295
    X1 = torch.cat([xs[:, None], gauss, i["e_in"]], 1)
    e1 = F.linear(X1, i["Wee"], i["bee"])
    en = F.layer_norm(e1, (64,), eps=1e-6) * (1 + _ada(i, pm, "scale_off", 64)) + _ada(i, pm, "shift_off", 64)
    return dict(d2=d2, xs=xs, X1=X1, e1=e1, en=en, te=torch.tanh(F.linear(en, i["Wte"])))


def _pair_functional(tb, i, m3, m4):
    pm = tb["pair_mol"]
    he = i["u"][tb["pair_a"]] + i["u"][tb["pair_b"]] + i["n2e_bias"]
    xe1 = i["e_in"] + _ada(i, pm, "gate1_off", 64) * he
    ye1 = F.layer_norm(xe1, (64,), eps=1e-6) * (1 + _ada(i, pm, "scale_off", 64)) + _ada(i, pm, "shift_off", 64)
    f3 = F.linear(ye1, i["W3"], i["b3"])
    s3 = F.silu(f3) * m3
    f4 = F.linear(s3, i["W4"], i["b4"]) * m4
    e_out = ye1 + _ada(i, pm, "gate2_off", 64) * f4
    X2 = torch.cat([e_out, i["feat"]], 1)
    return dict(he=he, xe1=xe1, ye1=ye1, f3=f3, s3=s3, f4=f4, e_out=e_out, X2=X2, ed=F.linear(X2, i["Wed"], i["bed"]), ro=F.linear(e_out, i["Wro"], i["bro"]))


def _dir_functional(tb, i):
    zz = i["ac"][tb["dir_row"], :256] + i["ac"][tb["dir_col"], 256:] + i["ed"][tb["dir_pair"]]
    zn = F.layer_norm(zz, (256,), eps=1e-6) * (1 + _ada(i, tb["dir_mol"], "scale_off", 256)) + _ada(i, tb["dir_mol"], "shift_off", 256)
    c0 = F.linear(zn, i["W0"], i["b0"])
    sc0 = F.silu(c0)
    return dict(zz=zz, zn=zn, c0=c0, sc0=sc0, c2=F.linear(sc0, i["W2"]))


def _node_functional(tb, i, m1, m2):
    nm = tb["node_mol"]
    x1 = i["h_in"] + _ada(i, nm, "gate1_off", 256) * i["attn"]
    y1 = F.layer_norm(x1, (256,), eps=1e-6) * (1 + _ada(i, nm, "scale_off", 256)) + _ada(i, nm, "shift_off", 256)
    f1 = F.linear(y1, i["W1"], i["b1"])
    s1 = F.silu(f1) * m1
    f2 = F.linear(s1, i["W2"], i["b2"]) * m2
    h_out = y1 + _ada(i, nm, "gate2_off", 256) * f2
    return dict(x1=x1, y1=y1, f1=f1, s1=s1, f2=f2, h_out=h_out, ac=F.linear(h_out, i["Wac"]), rn=F.linear(h_out, i["Wn"], i["bn"]))


def _mask(i, site_key, rows, cols):
    keep, m = CM.keep_scaled(i["seed"], i[site_key], rows, cols, i["p"])
    assert 0.8 < float(keep.double().mean()) < 0.97                           # p = 0.1 really drops
    assert relerr(m[keep], torch.full((int(keep.sum()),), 1.0 / 0.9, dtype=torch.float64)) < 1e-7
    return m


@pytest.mark.parametrize("chain", ["front", "pair", "dir", "node"])
def test_forward_mirror_equals_the_functional_form(chain):
    tb, i = _case(chain)
    if chain == "front":
        got, ref = CM.pair_front_fwd(tb, i, round_operands=False), _front_functional(tb, i)
    elif chain == "pair":
        got = CM.pair_chain_fwd(tb, i, round_operands=False)
        ref = _pair_functional(tb, i, _mask(i, "stream3", tb["Pp"], 128), _mask(i, "stream4", tb["Pp"], 64))
    elif chain == "dir":
        got, ref = CM.dir_chain_fwd(tb, i, round_operands=False), _dir_functional(tb, i)
    else:
        got = CM.node_chain_fwd(tb, i, round_operands=False)
        ref = _node_functional(tb, i, _mask(i, "stream1", tb["Nn"], 512), _mask(i, "stream2", tb["Nn"], 256))
    for k, v in ref.items():
        assert got[k].shape == v.shape, k
        assert relerr(got[k], v) <= 1e-12, (k, relerr(got[k], v))
    # (mean, rstd) of the LayerNorm in front of the products: the biased variance and eps 1e-6 of F.layer_norm
    x = ref[dict(front="e1", pair="xe1", dir="zz", node="x1")[chain]]
    assert relerr(got["st"][:, 0], x.mean(1)) <= 1e-12
    assert relerr(got["st"][:, 1], 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-6)) <= 1e-12


# ------------------------------------------------------------------------------------------------ backward vs autograd
def _grads(loss, wrt):
    return torch.autograd.grad(loss, wrt, allow_unused=False)


def _ada_slices(g_ada, i, keys, C):
    return {k: g_ada[:, i[k + "_off"]:i[k + "_off"] + C] for k in keys}


def _outside_is_zero(g_ada, i, keys, C):
    m = torch.ones(g_ada.shape[1], dtype=torch.bool)
    for k in keys:
        m[i[k + "_off"]:i[k + "_off"] + C] = False
    return bool((g_ada[:, m] == 0).all())


def test_dir_backward_mirror_equals_autograd():
    tb, i = _case("dir", grad=True)
    f = CM.dir_chain_fwd(tb, i, round_operands=False)
    gc0, gzz, gada = _grads((f["c2"] * i["dc2"].detach()).sum(), [f["c0"], f["zz"], i["ada"]])
    j = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in i.items()}
    b = CM.dir_chain_bwd(tb, dict(j, c0=f["c0"].detach(), zz=f["zz"].detach(), st=f["st"].detach()), round_operands=False)
    assert relerr(b["dc0"], gc0) <= 1e-10 and relerr(b["dz"], gzz) <= 1e-10
    for k, v in _ada_slices(gada, i, ("shift", "scale"), 256).items():
        assert relerr(b["d_ada"][k], v) <= 1e-10, k
        assert bool((b["d_ada"][k][[1, 5]] == 0).all())                       # the molecules without a pair
    assert _outside_is_zero(gada, i, ("shift", "scale"), 256)


@pytest.mark.parametrize("chain", ["pair", "node"])
def test_rear_backward_mirror_equals_autograd(chain):
    tb, i = _case(chain, grad=True)
    j = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in i.items()}
    if chain == "pair":
        f = CM.pair_chain_fwd(tb, i, round_operands=False)
        loss = (f["e_out"] * j["de"]).sum() + (f["ro"] * j["dro"]).sum() + (f["ed"] * j["ded"]).sum()
        names, C = ("df4", "df3", "de_in", "dhe", "dfeat"), 64
        auto = _grads(loss, [f["f4_pre"], f["f3"], f["xe1"], f["he"], i["feat"], i["ada"], i["e_in"]])
        tape = dict(f4=f["f4"], f3=f["f3"], xe1=f["xe1"], st=f["st"], he=f["he"])
        b = CM.pair_chain_bwd(tb, dict(j, **{k: v.detach() for k, v in tape.items()}), round_operands=False)
    else:
        f = CM.node_chain_fwd(tb, i, round_operands=False)
        loss = (f["h_out"] * j["dh"]).sum() + (f["rn"] * j["drn"]).sum() + (f["ac"] * j["dac"]).sum()
        names, C = ("df2", "df1", "dh_in", "dattn"), 256
        auto = _grads(loss, [f["f2_pre"], f["f1"], f["x1"], i["attn"], i["ada"], i["h_in"]])
        tape = dict(f2=f["f2"], f1=f["f1"], x1=f["x1"], st=f["st"])
        b = CM.node_chain_bwd(tb, dict(j, **{k: v.detach() for k, v in tape.items()}), round_operands=False)
    for k, g in zip(names, auto):
        assert relerr(b[k], g) <= 1e-10, (k, relerr(b[k], g))
    assert relerr(b[names[2]], auto[-1]) <= 1e-10                             # de_in / dh_in is also the gradient of the chain's residual input
    gada = auto[len(names)]
    for k, v in _ada_slices(gada, i, ("gate1", "shift", "scale", "gate2"), C).items():
        assert relerr(b["d_ada"][k], v) <= 1e-10, (k, relerr(b["d_ada"][k], v))
    assert _outside_is_zero(gada, i, ("gate1", "shift", "scale", "gate2"), C)
    # a dropped element carries no gradient; a kept one carries the 1 / (1 - p) scale (checked through autograd above)
    f_keys = (("df4", "keep4"), ("df3", "keep3")) if chain == "pair" else (("df2", "keep2"), ("df1", "keep1"))
    for k, m in f_keys:
        assert bool((b[k][~f[m]] == 0).all()) and int((~f[m]).sum()) > 0


# ------------------------------------------------------------------------------------------------ rounding and teacher forcing
PRODUCTS = dict(front=[("e1", "X1", "Wee", "bee"), ("te_pre", "en", "Wte", None)],
                pair=[("f3", "ye1", "W3", "b3"), ("f4_pre", "s3", "W4", "b4"), ("ed", "X2", "Wed", "bed"), ("ro", "e_out", "Wro", "bro")],
                dir=[("c0", "zn", "W0", "b0"), ("c2", "sc0", "W2", None)],
                node=[("f1", "y1", "W1", "b1"), ("f2_pre", "s1", "W2", "b2"), ("ac", "h_out", "Wac", None), ("rn", "h_out", "Wn", "bn")])
FWD = dict(front=CM.pair_front_fwd, pair=CM.pair_chain_fwd, dir=CM.dir_chain_fwd, node=CM.node_chain_fwd)


@pytest.mark.parametrize("chain", ["front", "pair", "dir", "node"])
def test_rounded_product_stages_are_linear_on_bf16_operands(chain):
    tb, i = _case(chain)
    got = FWD[chain](tb, i)
    exact = FWD[chain](tb, i, round_operands=False)
    for out, a, w, b in PRODUCTS[chain]:
        ref = F.linear(got[a].bfloat16().double(), i[w].bfloat16().double(), None if b is None else i[b])
        assert relerr(got[out], ref) <= 1e-12, out
        assert 1e-5 < relerr(got[out], exact[out]) < 5e-2, out                # the rounding is really on, and is bf16-sized
        bound = got["bound"][out.replace("_pre", "")]
        assert bound.shape == ref.shape and float(bound.min()) >= 0.0
        K = i[w].shape[1]
        lim = 2 * (K + 2) * 2.0 ** -24 * (got[a].bfloat16().double().abs() @ i[w].bfloat16().double().abs().T + (0 if b is None else i[b].abs()))
        if out in ("f4_pre", "f2_pre"):                                       # the bound of the stage behind the dropout carries its mask and scale
            lim = lim * CM.keep_scaled(i["seed"], i["stream4" if chain == "pair" else "stream2"], ref.shape[0], ref.shape[1], i["p"])[1]
        assert relerr(bound, lim) <= 1e-12, out


def test_a_stage_is_evaluated_from_the_tape_tensor_in_front_of_it():
    tb, i = _case("pair")
    base = CM.pair_chain_fwd(tb, i)
    ye1 = torch.zeros_like(base["ye1"])
    forced = CM.pair_chain_fwd(tb, i, tape=dict(ye1=ye1.float()))
    assert relerr(forced["f3"], i["b3"].expand_as(forced["f3"])) <= 1e-15      # f3 from the tape's ye1 ...
    assert torch.equal(forced["ye1"], base["ye1"])                            # ... while the stage itself is still the mirror's own
    assert torch.equal(forced["s3"], base["s3"]) is False
    s3 = base["s3"].float()
    forced = CM.pair_chain_fwd(tb, i, tape=dict(s3=s3))
    assert torch.equal(forced["f3"], base["f3"])
    assert relerr(forced["f4_pre"], F.linear(s3.bfloat16().double(), i["W4"].bfloat16().double(), i["b4"])) <= 1e-12
    tb, i = _case("pair")
    fw = CM.pair_chain_fwd(tb, i)
    j = dict(i, f4=fw["f4"], f3=fw["f3"], xe1=fw["xe1"], st=fw["st"], he=fw["he"])
    b0 = CM.pair_chain_bwd(tb, j)
    b1 = CM.pair_chain_bwd(tb, j, tape=dict(df4=torch.zeros_like(b0["df4"])))
    assert float(b1["df3"].abs().max()) == 0.0 and torch.equal(b1["df4"], b0["df4"])


# ------------------------------------------------------------------------------------------------ the mask convention
@pytest.mark.parametrize("block", [0, 2])
def test_mask_convention_is_the_oracles(block):
    """``oracle.train.dropout_masks`` (what golden G17 injects into the reference's nn.Dropout) against ``keep_scaled``: node sites 0, 1 on
    the packed node rows, pair sites 2, 3 on the packed pair rows (both directed edges of a pair carry the pair's mask), stream
    4 * block + site, element row * C + col."""
    n_atoms, seed, N = [3, 1, 4, 2], 987654321, 5
    tb = CM.tables(n_atoms)
    fn = otrain.dropout_masks(n_atoms, N, P, seed)
    valid = torch.tensor([a < n for n in n_atoms for a in range(N)])
    for site, C in ((0, 512), (1, 256)):
        dense = fn(block, site, torch.ones(len(n_atoms) * N, C)).double()
        keep, m = CM.keep_scaled(seed, 4 * block + site, tb["Nn"], C, P)
        assert torch.equal(dense[valid] != 0, keep) and relerr(dense[valid], m) < 1e-7
        assert not torch.equal(keep, CM.keep_scaled(seed, 4 * block + site + 1, tb["Nn"], C, P)[0])
    # directed edges in dense_to_sparse order: per molecule, (i, j) row-major with i != j
    pair_index = {(int(m), int(a), int(b)): p for p, (m, a, b) in enumerate(zip(tb["pair_mol"], tb["pair_a"], tb["pair_b"]))}
    rows = [pair_index[(m, tb["node_off"][m] + min(a, b), tb["node_off"][m] + max(a, b))]
            for m, n in enumerate(n_atoms) for a in range(n) for b in range(n) if a != b]
    for site, C in ((2, 128), (3, 64)):
        dense = fn(block, site, torch.ones(len(rows), C)).double()
        keep, m = CM.keep_scaled(seed, 4 * block + site, tb["Pp"], C, P)
        assert torch.equal(dense != 0, keep[rows]) and relerr(dense, m[rows]) < 1e-7
    # the element order: flat index row * C + col of ONE stream (not a stream per row)
    flat = CM.keep_scaled(seed, 4 * block + 3, 1, tb["Pp"] * 64, P)[0]
    assert torch.equal(flat.reshape(tb["Pp"], 64), CM.keep_scaled(seed, 4 * block + 3, tb["Pp"], 64, P)[0])
    # and the mirrors use their stream arguments: pair sites 2, 3
    i = CM.random_inputs("pair", tb, 1, p=P, block=block, drop_seed=seed)
    f = CM.pair_chain_fwd(tb, i)
    assert torch.equal(f["keep3"], CM.keep_scaled(seed, 4 * block + 2, tb["Pp"], 128, P)[0])
    assert torch.equal(f["keep4"], CM.keep_scaled(seed, 4 * block + 3, tb["Pp"], 64, P)[0])
    assert bool((f["s3"][~f["keep3"]] == 0).all()) and bool((f["f4"][~f["keep4"]] == 0).all())


# ------------------------------------------------------------------------------------------------ the activations of the GEMM epilogue
def test_activations_and_their_derivatives_are_torchs():
    """``silu`` / ``gelu`` / their derivatives and ``dtanh_of_output`` against torch in float64 (values) and torch.autograd (derivatives), and
    ``LIPSCHITZ`` against the largest |f'| on a grid that holds the maxima (SiLU' peaks at 2.3994, GELU' at sqrt 2)."""
    x = torch.linspace(-12.0, 12.0, 48001, dtype=torch.float64)
    for f, df, ref, name in ((CM.silu, CM.dsilu, F.silu, "silu"), (CM.gelu, CM.dgelu, F.gelu, "gelu")):
        xr = x.clone().requires_grad_(True)
        y = ref(xr)
        y.sum().backward()
        assert relerr(f(x), y) <= 1e-15 and relerr(df(x), xr.grad) <= 1e-14, name
        peak = float(df(x).abs().max())
        assert peak <= CM.LIPSCHITZ[name] <= 1.01 * peak, (name, peak)
    xr = x.clone().requires_grad_(True)
    y = torch.tanh(xr)
    y.sum().backward()
    assert relerr(CM.dtanh_of_output(y.detach()), xr.grad) <= 1e-15 and float(xr.grad.max()) <= CM.LIPSCHITZ["tanh"] == 1.0
    assert relerr(CM.dgelu(torch.tensor([2.0 ** 0.5], dtype=torch.float64)), torch.tensor([1.1289], dtype=torch.float64)) < 1e-4
