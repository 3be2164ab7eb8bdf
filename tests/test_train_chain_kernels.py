"""GPU parity of the fused bf16 row chains (csrc/ds_train_chain.hip: dst_pair_front_fwd, dst_pair_chain_fwd, dst_dir_chain_fwd,
dst_node_chain_fwd, dst_dir_chain_bwd, dst_pair_chain_bwd, dst_node_chain_bwd), each entry point called directly and compared STAGE BY
STAGE with the float64 yardstick of tests/chain_mirror.py (pinned on the CPU by tests/test_chain_mirror_cpu.py).

Teacher forcing: every stage's reference is evaluated from the KERNEL'S OWN tape tensor of the stage in front of it (f3 from the kernel's
ye1, f4 from its s3, ed from its X2, c2 from its sc0, df3 from its df4, ...), so both sides round bit-identical fp32 values to bf16 and only
the fp32 accumulation separates them.  Tolerances (derived, not measured):

* a product stage, per element: |got - ref| <= 2 (K + 2) 2^-24 (|A| |W|^T + |bias|) - twice the gamma_K bound of an fp32 sum of K exact
  products in ANY order (chain_mirror.product_bound);
* everything else with the suite's measure max |got - ref| / max |ref| (tests.helpers.relerr), per molecule's rows as well as per tensor,
  at what the unfused kernels are held to: gate / residual 2e-6; modulated LayerNorm and (mean, rstd) 3e-6; Gaussian features, x', d2 3e-6;
  SiLU / tanh epilogues 3e-6 (hardware exp2 / rcp forms, documented absolute error 1e-7); LayerNorm backward rows 2e-5; d_ada slices 1e-5;
* a stage behind a product the kernel does not write (the tanh pre-activation; de_tot, dye1, dzn, dh_tot, dy1) gets that product's bound,
  carried through the stage (chain_mirror's docstring), ADDED to its tolerance.

Interface edges, in every test: all tape pointers NULL against all set (the always-written outputs bit-identical), every kernel twice
(bit-identical: a fixed summation order is promised), ``feat`` / ``dro`` / ``drn`` as column windows of wider tensors, ``Wed`` with a leading
stride of 136, adaLN offsets that are non-zero and distinct, a d_ada table full of a sentinel (only the assigned slices may change), one
guard tile of sentinel rows behind every output, dropout 0.1 and 0 on streams 4 * block + site of block 3, molecules without a pair,
Pp = 0 and a single pair.  Every test prints ``stage deviation/share`` with share = the largest |got - ref| over what the stage is allowed
(for a product stage: the error-to-bound ratio)."""
import pytest
import torch

from tests import chain_mirror as CM

pytestmark = pytest.mark.gpu

LAYOUTS = {"ragged": [3, 1, 9, 2, 12, 1],      # Nn = 28 (one partial node tile); Pp = 106: flat tiles 32 | 32 | 32 | 10, each across a molecule boundary;
                                               # two molecules without a pair; aligned pair tiles 3 | 32 4 | 1 | 32 32 2, directed 6 | 32 32 8 | 2 | 32 x 4, 4
           "split": [29, 29, 5],               # Nn = 63: flat node tiles 32 | 31 split a molecule; Pp = 822: many tiles per molecule, a 22-row tail
           "single": [1],                      # Pp = 0
           "one_pair": [2]}                    # one pair row, two directed rows, two node rows
CASES = [(name, p) for name in LAYOUTS for p in (0.1, 0.0)]
SENT = -7.5                                    # fills every output and the d_ada table before a launch
GUARD = 32                                     # one tile of sentinel rows behind every output
BLOCK = 3                                      # dropout streams 4 * BLOCK + site
TOL = dict(gate=2e-6, ln=3e-6, feat=3e-6, act=3e-6, ln_bwd=2e-5, d_ada=1e-5)

FWD = dict(
    front=dict(rows="pair", always=("X1", "te"), tape=("xs", "d2", "e1", "st", "en"), names=dict(st="st_e1"),
               width=dict(X1=128, te=512, xs=1, d2=1, e1=64, st=2, en=64)),
    pair=dict(rows="pair", always=("e_out", "ed", "ro"), tape=("he", "xe1", "st", "ye1", "f3", "s3", "f4", "X2"), names=dict(st="st_e2", ro="re_"),
              width=dict(he=64, xe1=64, st=2, ye1=64, f3=128, s3=128, f4=64, e_out=64, X2=128, ed=256, ro=16)),
    dir=dict(rows="dir", always=("c2",), tape=("zz", "st", "zn", "c0", "sc0"), names=dict(st="st_z"),
             width=dict(zz=256, st=2, zn=256, c0=256, sc0=256, c2=3)),
    node=dict(rows="node", always=("h_out", "ac", "rn"), tape=("x1", "st", "y1", "f1", "s1", "f2"), names=dict(st="st_n2"),
              width=dict(x1=256, st=2, y1=256, f1=512, s1=512, f2=256, h_out=256, ac=512, rn=64)))
BWD = dict(dir=dict(rows="dir", out=dict(dc0=256, dz=256), slices=("shift", "scale"), C=256),
           pair=dict(rows="pair", out=dict(dfeat=64, df4=64, df3=128, de_in=64, dhe=64), slices=("gate1", "shift", "scale", "gate2"), C=64),
           node=dict(rows="node", out=dict(df2=256, df1=512, dh_in=256, dattn=256), slices=("gate1", "shift", "scale", "gate2"), C=256))


class Ctx:
    """One layout on the device: the library, the layout tables, and a list that keeps every operand alive until the synchronise (a temporary
    handed to a launch as a bare pointer may be freed and reused before the kernel has read it; ``_dev`` in tests/test_train_hip.py)."""

    def __init__(self, gpu_device, name):
        from diffspectra_amd import engine as E, filler, train_engine as T
        self.E, self.T, self.d, self.name = E, T, gpu_device, name
        if "ops" not in _CTX:
            _CTX["ops"] = T.Ops(gpu_device)                                  # (one scratch buffer for all layouts)
        self.o = _CTX["ops"]
        self.n_atoms = LAYOUTS[name]
        self.tb = CM.tables(self.n_atoms)
        self.TL = T.TrainLayout(filler.masks_from_n_atoms(self.n_atoms)[0], gpu_device)
        assert (self.TL.B, self.TL.Nn, self.TL.Pp) == (self.tb["B"], self.tb["Nn"], self.tb["Pp"])
        self.keep = []
        if self.TL.Pp == 0:
            # no pair: the layout's pair tables are empty tensors (NULL pointers), which the entry points reject like any NULL operand
            # before they look at Pp; a raw caller passes any valid address
            ph = self.dev(torch.zeros(4, dtype=torch.int32))
            self.TL.pair_tables = (ph.data_ptr(),) * 3
        self.rows = dict(pair=self.tb["Pp"], dir=2 * self.tb["Pp"], node=self.tb["Nn"])
        off = dict(pair=self.tb["pair_off"], dir=2 * self.tb["pair_off"], node=self.tb["node_off"])
        self.segs = {k: [("all", 0, self.rows[k])] + [(f"molecule {m}", int(v[m]), int(v[m + 1])) for m in range(self.tb["B"])] for k, v in off.items()}
        self.mol_segs = [("all", 0, self.tb["B"])] + [(f"molecule {m}", m, m + 1) for m in range(self.tb["B"])]

    def dev(self, t):
        x = t.to(self.d).contiguous()
        self.keep.append(x)
        return x

    def out(self, rows, cols):
        x = torch.full((rows + GUARD, cols), SENT, device=self.d)
        self.keep.append(x)
        return x

    def window(self, t, lead, ld):
        """``t`` [rows, c] as columns lead .. lead + c of a wider [max(rows, 1), ld] tensor: the view the kernel gets a pointer into."""
        wide = torch.full((max(t.shape[0], 1), ld), 3.25)
        wide[:t.shape[0], lead:lead + t.shape[1]] = t
        return self.dev(wide)[:, lead:lead + t.shape[1]]

    def inputs(self, i, keys):
        return {k: self.dev(i[k] if i[k].shape[0] else torch.zeros(1, *i[k].shape[1:])) for k in keys}

    def pack(self, i, plan):
        """bf16 copies of the weights ``plan = {name: (key, transposed, leading stride or None, slice or None)}`` with dst_pack_bf16_pieces."""
        dst, src, key_t, res = [], [], set(), {}
        for n, (key, transposed, ld, cols) in plan.items():
            w = i[key] if cols is None else i[key][:, cols[0]:cols[1]]
            w = self.dev(w.contiguous())
            shape = tuple(w.shape)[::-1] if transposed else tuple(w.shape)
            buf = torch.full((shape[0], ld or shape[1]), 2.5, dtype=torch.bfloat16, device=self.d)
            self.keep.append(buf)
            res[n] = buf[:, :shape[1]]
            if transposed:
                key_t.add(len(dst))
            dst.append(res[n]); src.append(w)
        cache = {}
        self.keep.append(cache)                                            # (holds the device table of the launch)
        self.T.pack_bf16_pieces(self.o.lib, self.d, dst, src, cache, "w", key_t=key_t)
        torch.cuda.synchronize()
        for n, (key, transposed, ld, cols) in plan.items():               # the packing the mirror assumes (Tensor.bfloat16(): nearest even)
            w = i[key] if cols is None else i[key][:, cols[0]:cols[1]]
            assert torch.equal(res[n].cpu(), (w.T if transposed else w).bfloat16()), n
        return res


_CTX, _FWD_RUNS = {}, {}


def ctx_of(gpu_device, name):
    if name not in _CTX:
        _CTX[name] = Ctx(gpu_device, name)
    return _CTX[name]


def case_inputs(c, chain, p):
    return CM.random_inputs(chain, c.tb, seed=11 + len(chain), ada_cols=c.T.ADA, p=p, block=BLOCK)


# ------------------------------------------------------------------------------------------------ comparison
def check_stage(rep, name, got, ref, segs, tol=0.0, bound=None):
    """``got`` against ``ref`` on every segment of rows: |got - ref| <= bound (per element) + tol * max |ref of the segment|."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    diff = (got - ref).abs()
    for label, r0, r1 in segs:
        if r1 <= r0:
            continue
        allow = tol * float(ref[r0:r1].abs().max())
        allow = allow if bound is None else bound[r0:r1] + allow
        over = diff[r0:r1] - allow
        if bool((over > 0).any()):
            at = int(over.argmax())
            r, col = at // diff.shape[1], at % diff.shape[1]
            raise AssertionError(f"{name}, {label}: row {r0 + r} column {col}: got {float(got[r0 + r, col])!r}, reference {float(ref[r0 + r, col])!r}, "
                                 f"|diff| {float(diff[r0 + r, col]):.3e} > allowed {float(allow if bound is None else allow[r, col]):.3e}")
    if diff.numel():
        scale = float(ref.abs().max())
        allow = tol * scale if bound is None else bound + tol * scale
        share = diff / allow
        share = float(share[torch.isfinite(share)].max()) if bool(torch.isfinite(share).any()) else 0.0
        old = rep.get(name, (0.0, 0.0))
        rep[name] = (max(old[0], float(diff.max()) / (scale + 1e-30)), max(old[1], share))


def report(tag, rep):
    print(f"[{tag}] " + ", ".join(f"{k} {v[0]:.1e}/{v[1]:.3f}" for k, v in rep.items()))


def check_untouched(c, outs, rows):
    for k, t in outs.items():
        assert bool((t[rows:] == SENT).all()), f"{k}: rows beyond {rows} were written"


def check_dropped(name, got, keep):
    got = got.cpu()
    assert bool((got[~keep] == 0).all()), f"{name}: a dropped element is not zero"
    if keep.numel() > 256 and not bool(keep.all()):
        assert float((got[keep] != 0).double().mean()) > 0.99, f"{name}: kept elements are zero"


# ------------------------------------------------------------------------------------------------ forward launches
def launch_fwd(c, chain, i, tapes=True):
    """One launch of a forward chain into fresh sentinel-filled outputs: {stage: tensor with its guard rows}."""
    spec, o, TL, T = FWD[chain], c.o, c.TL, c.T
    rows = c.rows[spec["rows"]]
    outs = {k: c.out(rows, spec["width"][k]) for k in spec["always"] + (spec["tape"] if tapes else ())}
    out = {spec["names"].get(k, k): v for k, v in outs.items()}
    ada = c.dev(i["ada"])
    if chain == "front":
        t = c.inputs(i, ("pos", "means", "stds", "e_in", "bee"))
        w = c.pack(i, dict(Wee=("Wee", False, None, None), Wte=("Wte", False, None, None)))
        o.pair_front_fwd(TL, t["pos"], ada, i["dist_off"], i["shift_off"], i["scale_off"], t["means"], t["stds"], t["e_in"], w["Wee"], t["bee"], w["Wte"], out)
    elif chain == "pair":
        t = c.inputs(i, ("u", "n2e_bias", "e_in", "b3", "b4", "bed", "bro"))
        feat = c.window(i["feat"], 32, 128)                               # ld_feat = 128
        w = c.pack(i, dict(W3=("W3", False, None, None), W4=("W4", False, None, None), Wed=("Wed", False, 136, None), Wro=("Wro", False, None, None)))
        o.pair_chain_fwd(TL, t["u"], t["n2e_bias"], t["e_in"], feat, 128, ada, i["gate1_off"], i["shift_off"], i["scale_off"], i["gate2_off"],
                         w["W3"], t["b3"], w["W4"], t["b4"], w["Wed"], 136, t["bed"], w["Wro"], t["bro"], (i["p"], i["seed"], i["stream3"], i["stream4"]), out)
    elif chain == "dir":
        t = c.inputs(i, ("ac", "ed", "b0"))
        w = c.pack(i, dict(W0=("W0", False, None, None), W2=("W2", False, None, None)))
        o.dir_chain_fwd(TL, t["ac"], t["ed"], ada, i["shift_off"], i["scale_off"], w["W0"], t["b0"], w["W2"], out)
    else:
        t = c.inputs(i, ("h_in", "attn", "b1", "b2", "bn"))
        w = c.pack(i, dict(W1=("W1", False, None, None), W2=("W2", False, None, None), Wac=("Wac", False, None, None), Wn=("Wn", False, None, None)))
        o.node_chain_fwd(TL, t["h_in"], t["attn"], ada, i["gate1_off"], i["shift_off"], i["scale_off"], i["gate2_off"], w["W1"], t["b1"], w["W2"], t["b2"],
                         w["Wac"], w["Wn"], t["bn"], (i["p"], i["seed"], i["stream1"], i["stream2"]), out)
    torch.cuda.synchronize()
    return outs


def forward(c, chain, p):
    """The forward of a case, run once and shared: (inputs, outputs of the first launch with its guard rows, the tape trimmed and on the CPU).
    Also checked here: a second launch and a launch without tape pointers give the same bits; rows beyond the layout's are untouched."""
    key = (c.name, chain, p)
    if key not in _FWD_RUNS:
        spec, i = FWD[chain], case_inputs(c, chain, p)
        rows = c.rows[spec["rows"]]
        outs = launch_fwd(c, chain, i)
        again = launch_fwd(c, chain, i)
        bare = launch_fwd(c, chain, i, tapes=False)
        for k in outs:
            assert torch.equal(outs[k], again[k]), f"{chain} {k}: two launches on the same inputs differ"
        for k in spec["always"]:
            assert torch.equal(outs[k], bare[k]), f"{chain} {k}: differs when the tape pointers are NULL"
        check_untouched(c, outs, rows)
        _FWD_RUNS[key] = (i, outs, {k: v[:rows].cpu() for k, v in outs.items()})
    return _FWD_RUNS[key]


def nothing_written(outs):
    return all(bool((t == SENT).all()) for t in outs.values())


# ------------------------------------------------------------------------------------------------ forward tests
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pair_front_fwd(gpu_device, name):
    c = ctx_of(gpu_device, name)
    i, outs, k = forward(c, "front", 0.0)
    if c.tb["Pp"] == 0:
        assert nothing_written(outs)
        return
    m, rep, segs = CM.pair_front_fwd(c.tb, i, tape=k), {}, c.segs["pair"]
    check_stage(rep, "d2", k["d2"], m["d2"][:, None], segs, TOL["feat"])
    check_stage(rep, "xs", k["xs"], m["xs"][:, None], segs, TOL["feat"])
    check_stage(rep, "x' column", k["X1"][:, :1], m["X1"][:, :1], segs, TOL["feat"])
    check_stage(rep, "gaussians", k["X1"][:, 1:64], m["X1"][:, 1:64], segs, TOL["feat"])
    assert torch.equal(k["X1"][:, :1], k["xs"]) and torch.equal(k["X1"][:, 64:], i["e_in"])
    check_stage(rep, "e1", k["e1"], m["e1"], segs, bound=m["bound"]["e1"])
    check_stage(rep, "st", k["st"], m["st"], segs, TOL["ln"])
    check_stage(rep, "en", k["en"], m["en"], segs, TOL["ln"])
    check_stage(rep, "te", k["te"], m["te"], segs, TOL["act"], bound=m["bound"]["te"])
    report(f"pair_front_fwd {name}", rep)


@pytest.mark.parametrize("name,p", CASES)
def test_pair_chain_fwd(gpu_device, name, p):
    c = ctx_of(gpu_device, name)
    i, outs, k = forward(c, "pair", p)
    if c.tb["Pp"] == 0:
        assert nothing_written(outs)
        return
    m, rep, segs = CM.pair_chain_fwd(c.tb, i, tape=k), {}, c.segs["pair"]
    for s in ("he", "xe1"):
        check_stage(rep, s, k[s], m[s], segs, TOL["gate"])
    for s in ("st", "ye1"):
        check_stage(rep, s, k[s], m[s], segs, TOL["ln"])
    check_stage(rep, "f3", k["f3"], m["f3"], segs, bound=m["bound"]["f3"])
    check_stage(rep, "s3", k["s3"], m["s3"], segs, TOL["act"])
    check_stage(rep, "f4", k["f4"], m["f4"], segs, bound=m["bound"]["f4"])
    check_stage(rep, "e_out", k["e_out"], m["e_out"], segs, TOL["gate"])
    assert torch.equal(k["X2"][:, :64], k["e_out"]) and torch.equal(k["X2"][:, 64:], i["feat"])
    check_stage(rep, "ed", k["ed"], m["ed"], segs, bound=m["bound"]["ed"])
    check_stage(rep, "ro", k["ro"], m["ro"], segs, bound=m["bound"]["ro"])
    check_dropped("s3", k["s3"], m["keep3"])
    check_dropped("f4", k["f4"], m["keep4"])
    assert bool(m["keep3"].all()) == (p == 0.0 or m["keep3"].numel() < 64)
    report(f"pair_chain_fwd {name} p={p}", rep)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_dir_chain_fwd(gpu_device, name):
    c = ctx_of(gpu_device, name)
    i, outs, k = forward(c, "dir", 0.0)
    if c.tb["Pp"] == 0:
        assert nothing_written(outs)
        return
    m, rep, segs = CM.dir_chain_fwd(c.tb, i, tape=k), {}, c.segs["dir"]
    check_stage(rep, "zz", k["zz"], m["zz"], segs, TOL["gate"])
    for s in ("st", "zn"):
        check_stage(rep, s, k[s], m[s], segs, TOL["ln"])
    check_stage(rep, "c0", k["c0"], m["c0"], segs, bound=m["bound"]["c0"])
    check_stage(rep, "sc0", k["sc0"], m["sc0"], segs, TOL["act"])
    check_stage(rep, "c2", k["c2"], m["c2"], segs, bound=m["bound"]["c2"])
    report(f"dir_chain_fwd {name}", rep)


@pytest.mark.parametrize("name,p", CASES)
def test_node_chain_fwd(gpu_device, name, p):
    c = ctx_of(gpu_device, name)
    i, outs, k = forward(c, "node", p)
    m, rep, segs = CM.node_chain_fwd(c.tb, i, tape=k), {}, c.segs["node"]
    check_stage(rep, "x1", k["x1"], m["x1"], segs, TOL["gate"])
    for s in ("st", "y1"):
        check_stage(rep, s, k[s], m[s], segs, TOL["ln"])
    check_stage(rep, "f1", k["f1"], m["f1"], segs, bound=m["bound"]["f1"])
    check_stage(rep, "s1", k["s1"], m["s1"], segs, TOL["act"])
    check_stage(rep, "f2", k["f2"], m["f2"], segs, bound=m["bound"]["f2"])
    check_stage(rep, "h_out", k["h_out"], m["h_out"], segs, TOL["gate"])
    check_stage(rep, "ac", k["ac"], m["ac"], segs, bound=m["bound"]["ac"])
    check_stage(rep, "rn", k["rn"], m["rn"], segs, bound=m["bound"]["rn"])
    check_dropped("s1", k["s1"], m["keep1"])
    check_dropped("f2", k["f2"], m["keep2"])
    report(f"node_chain_fwd {name} p={p}", rep)


# ------------------------------------------------------------------------------------------------ backward launches
def launch_bwd(c, chain, i, tape):
    """One launch of a backward chain on the forward's tape (device tensors, guard rows and all) into fresh sentinel-filled outputs and a
    sentinel-filled d_ada table: (outputs, d_ada)."""
    spec, o, TL = BWD[chain], c.o, c.TL
    rows = c.rows[spec["rows"]]
    outs = {k: c.out(rows, w) for k, w in spec["out"].items()}
    ada = c.dev(i["ada"])
    d_ada = c.dev(torch.full((c.tb["B"], c.T.ADA), SENT))
    if chain == "dir":
        t = c.inputs(i, ("dc2", "W2"))                                    # coord_mlp.2 stays fp32 in the backward (K = 3)
        w = c.pack(i, dict(W0T=("W0", True, None, None)))
        o.dir_chain_bwd(TL, t["dc2"], tape["c0"], tape["zz"], tape["st"], ada, d_ada, i["shift_off"], i["scale_off"], t["W2"], w["W0T"], outs["dc0"], outs["dz"])
    elif chain == "pair":
        t = c.inputs(i, ("de", "ded"))
        dro = c.window(i["dro"], 8, 40)                                   # ld_dro = 40
        w = c.pack(i, dict(WedT=("Wed", True, None, None), WroT=("Wro", True, None, None), W4T=("W4", True, None, None), W3T=("W3", True, None, None)))
        o.pair_chain_bwd(TL, t["de"], dro.data_ptr(), 40, t["ded"], tape["f4"], tape["f3"], tape["xe1"], tape["st"], tape["he"], ada, d_ada,
                         i["gate1_off"], i["shift_off"], i["scale_off"], i["gate2_off"], w["WedT"], w["WroT"], w["W4T"], w["W3T"],
                         (i["p"], i["seed"], i["stream3"], i["stream4"]), outs["dfeat"], outs["df4"], outs["df3"], outs["de_in"], outs["dhe"])
    else:
        t = c.inputs(i, ("dh", "dac", "attn"))
        drn = c.window(i["drn"], 16, 96)                                  # ld_drn = 96
        w = c.pack(i, dict(WacT=("Wac", True, None, None), WnT=("Wn", True, None, None), W2T=("W2", True, None, None), W1T=("W1", True, None, None)))
        o.node_chain_bwd(TL, t["dh"], drn.data_ptr(), 96, t["dac"], tape["f2"], tape["f1"], tape["x1"], tape["st"], t["attn"], ada, d_ada,
                         i["gate1_off"], i["shift_off"], i["scale_off"], i["gate2_off"], w["WacT"], w["WnT"], w["W2T"], w["W1T"],
                         (i["p"], i["seed"], i["stream1"], i["stream2"]), outs["df2"], outs["df1"], outs["dh_in"], outs["dattn"])
    torch.cuda.synchronize()
    return outs, d_ada


def backward(c, chain, p):
    """The backward of a case on its forward's tape, launched twice (same bits); the trimmed outputs, the d_ada slices, the mirror inputs."""
    spec = BWD[chain]
    rows = c.rows[spec["rows"]]
    i, f_outs, k = forward(c, chain, p)
    outs, d_ada = launch_bwd(c, chain, i, f_outs)
    again, d_again = launch_bwd(c, chain, i, f_outs)
    for n in outs:
        assert torch.equal(outs[n], again[n]), f"{chain} {n}: two launches on the same inputs differ"
    assert torch.equal(d_ada, d_again), f"{chain} d_ada: two launches on the same inputs differ"
    check_untouched(c, outs, rows)
    d_ada = d_ada.cpu()
    assigned = torch.zeros(d_ada.shape[1], dtype=torch.bool)
    slices = {}
    for s in spec["slices"]:
        off = i[s + "_off"]
        assigned[off:off + spec["C"]] = True
        slices[s] = d_ada[:, off:off + spec["C"]]
    assert bool((d_ada[:, ~assigned] == SENT).all()), f"{chain}: d_ada columns outside the assigned slices were written"
    assert not bool((d_ada[:, assigned] == SENT).any()), f"{chain}: an assigned d_ada slice still holds the sentinel"
    return i, k, {n: v[:rows].cpu() for n, v in outs.items()}, slices


def check_d_ada(c, rep, spec, got, m):
    for s in spec["slices"]:
        check_stage(rep, f"d_ada[{s}]", got[s], m["d_ada"][s], c.mol_segs, TOL["d_ada"], bound=m["bound"]["d_ada"][s])


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_dir_chain_bwd(gpu_device, name):
    c = ctx_of(gpu_device, name)
    i, k, g, d_ada = backward(c, "dir", 0.0)
    m = CM.dir_chain_bwd(c.tb, dict(i, c0=k["c0"], zz=k["zz"], st=k["st"]), tape=g)
    rep, segs = {}, c.segs["dir"]
    check_stage(rep, "dc0", g["dc0"], m["dc0"], segs, TOL["act"])
    check_stage(rep, "dz", g["dz"], m["dz"], segs, TOL["ln_bwd"], bound=m["bound"]["dz"])
    check_d_ada(c, rep, BWD["dir"], d_ada, m)
    report(f"dir_chain_bwd {name}", rep)


@pytest.mark.parametrize("name,p", CASES)
def test_pair_chain_bwd(gpu_device, name, p):
    c = ctx_of(gpu_device, name)
    i, k, g, d_ada = backward(c, "pair", p)
    m = CM.pair_chain_bwd(c.tb, dict(i, f4=k["f4"], f3=k["f3"], xe1=k["xe1"], st=k["st"], he=k["he"]), tape=g)
    rep, segs, b = {}, c.segs["pair"], m["bound"]
    check_stage(rep, "dfeat", g["dfeat"], m["dfeat"], segs, bound=b["dfeat"])
    check_stage(rep, "df4", g["df4"], m["df4"], segs, TOL["gate"], bound=b["df4"])
    check_stage(rep, "df3", g["df3"], m["df3"], segs, TOL["act"], bound=b["df3"])
    check_stage(rep, "de_in", g["de_in"], m["de_in"], segs, TOL["ln_bwd"], bound=b["de_in"])
    check_stage(rep, "dhe", g["dhe"], m["dhe"], segs, TOL["ln_bwd"], bound=b["dhe"])
    check_d_ada(c, rep, BWD["pair"], d_ada, m)
    f = CM.pair_chain_fwd(c.tb, i, tape=k)                                # the forward's masks: the same elements are dropped in both directions
    check_dropped("df4", g["df4"], f["keep4"])
    check_dropped("df3", g["df3"], f["keep3"])
    assert torch.equal((k["f4"] == 0) & ~f["keep4"], ~f["keep4"]) and torch.equal((k["s3"] == 0) & ~f["keep3"], ~f["keep3"])
    report(f"pair_chain_bwd {name} p={p}", rep)


@pytest.mark.parametrize("name,p", CASES)
def test_node_chain_bwd(gpu_device, name, p):
    c = ctx_of(gpu_device, name)
    i, k, g, d_ada = backward(c, "node", p)
    m = CM.node_chain_bwd(c.tb, dict(i, f2=k["f2"], f1=k["f1"], x1=k["x1"], st=k["st"]), tape=g)
    rep, segs, b = {}, c.segs["node"], m["bound"]
    check_stage(rep, "df2", g["df2"], m["df2"], segs, TOL["gate"], bound=b["df2"])
    check_stage(rep, "df1", g["df1"], m["df1"], segs, TOL["act"], bound=b["df1"])
    check_stage(rep, "dh_in", g["dh_in"], m["dh_in"], segs, TOL["ln_bwd"], bound=b["dh_in"])
    check_stage(rep, "dattn", g["dattn"], m["dattn"], segs, TOL["ln_bwd"], bound=b["dattn"])
    check_d_ada(c, rep, BWD["node"], d_ada, m)
    f = CM.node_chain_fwd(c.tb, i, tape=k)
    check_dropped("df2", g["df2"], f["keep2"])
    check_dropped("df1", g["df1"], f["keep1"])
    report(f"node_chain_bwd {name} p={p}", rep)


def test_molecule_aligned_tiles_are_the_ones_the_cases_are_built_for(gpu_device):
    """The tile tables the backward kernels are given for the ragged layout: pair tiles 3 | 32 4 | 1 | 32 32 2, directed tiles 6 | 32 32 8 | 2 |
    32 x 4, 4, one partial node tile per molecule; the molecules without a pair own no tile."""
    c = ctx_of(gpu_device, "ragged")
    pair, dirs, node = ([t.cpu().tolist() for t in tens] for tens in c.TL._tile_tensors)
    assert pair[1] == [3, 32, 4, 1, 32, 32, 2] and pair[2] == [0, 2, 2, 3, 4, 4, 4] and pair[3] == [0, 1, 1, 3, 4, 7, 7]
    assert dirs[1] == [6, 32, 32, 8, 2, 32, 32, 32, 32, 4] and dirs[3] == [0, 1, 1, 4, 5, 10, 10]
    assert node[1] == [3, 1, 9, 2, 12, 1]
    assert (c.tb["Nn"], c.tb["Pp"]) == (28, 106)
    s = ctx_of(gpu_device, "split")
    assert (s.tb["Nn"], s.tb["Pp"], s.tb["Pp"] % 32) == (63, 822, 22)
