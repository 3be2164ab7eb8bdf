"""GPU: the multistep solver update (``ds_solver_step*``, include/diffspectra_solver.h) and ``sampling.MultistepSampler`` - the kernels against
the fp64 mirror (tests/solver_mirror.py) and ``oracle/philox.py``, the order of convergence through the kernels on a Gaussian data
distribution, graph replay against the eager launch sequence, and the evaluation path end to end.  No sample-quality claim is tested."""
import pytest
import torch

from tests.golden import cases
from tests.solver_mirror import gaussian_denoiser, gaussian_flow, mirror_step
from tests.test_hip_parity import (_philox_sampling_setup, _same_molecules, assert_close, gpu_model, swapped_weights, to_dev)

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
SEED = (3 << 32) + 42


def _masks():
    """B = 5, N = 29: n = 4, 29, 1, 11 and a non-prefix mask of 5 atoms (the layout of test_philox_noise_kernels_vs_oracle)."""
    node_mask = torch.zeros(5, 29, 1)
    for b, n in enumerate([4, 29, 1, 11]):
        node_mask[b, :n] = 1
    node_mask[4, [0, 2, 3, 7, 8]] = 1
    nm2 = node_mask.squeeze(-1)
    edge_mask = ((nm2.unsqueeze(1) * nm2.unsqueeze(2)) * (~torch.eye(29, dtype=torch.bool)).unsqueeze(0)).reshape(-1, 1)
    return node_mask, edge_mask


def _state(name, node_mask, edge_mask):
    """A masked, CoM-free, edge-symmetric state on any mask (filler.synthetic_state knows prefix masks only)."""
    from diffspectra_amd import filler
    B, N, _ = node_mask.shape
    pos = filler.normal(name + ".pos", (B, N, 3)) * node_mask
    pos = pos - (pos.sum(1, keepdim=True) / node_mask.sum(1, keepdim=True)) * node_mask
    feat = filler.normal(name + ".feat", (B, N, 6)) * node_mask
    e = torch.tril(filler.normal(name + ".edge", (B, 2, N, N)), -1)
    e = (e + e.transpose(-1, -2)).permute(0, 2, 3, 1) * edge_mask.reshape(B, N, N, 1)
    return torch.cat([pos, feat], dim=2), e.contiguous()


def _philox_noise(node_mask, mol, draw):
    from oracle import philox as P
    B, N, _ = node_mask.shape
    nm2 = node_mask.squeeze(-1)
    wx, we = torch.zeros(B, N, 9), torch.zeros(B, N, N, 2)
    for b in range(B):
        idx = torch.nonzero(nm2[b]).reshape(-1)
        pos, feat, edge = P.molecule_noise(SEED, draw, int(mol[b]), len(idx))
        wx[b, idx, :3], wx[b, idx, 3:] = torch.from_numpy(pos), torch.from_numpy(feat)
        we[b, idx.unsqueeze(1), idx.unsqueeze(0)] = torch.from_numpy(edge)
    return wx, we


ROWS = {  # (a, b, c, d)
    "second_order_sde": (0.8125, 0.31, -0.12, 0.27),
    "first_order_sde": (0.8125, 0.31, 0.0, 0.27),       # c == 0: the history holds NaN
    "second_order_ode": (0.8125, 0.4, -0.09, 0.0),      # d == 0: raw_* are NULL
    "last_row": (0.0, 1.0, 0.0, 0.0),                   # both
}


@pytest.fixture(scope="module")
def kernel_case(gpu_device):
    """Inputs of the kernel tests, made once and never modified (every test works on clones)."""
    import oracle
    from diffspectra_amd import filler
    cfg, model = gpu_model("allspectra", gpu_device)
    eng = model.module.engine()
    node_mask, edge_mask = _masks()
    L, _ = eng.layout_for(node_mask, edge_mask, validate=True)
    c = dict(eng=eng, L=L, node_mask=node_mask, edge_mask=edge_mask, B=5, N=29)
    for name in ("x", "p", "h"):
        c[name], c["e" + name] = _state("sv." + name, node_mask, edge_mask)
    c["raw"] = (filler.normal("sv.rp", (5, 29, 3)), filler.normal("sv.rf", (5, 29, 6)), filler.normal("sv.re", (5, 2, 29, 29)))
    c["noise_x"] = oracle.combined_noise(c["raw"][0].double(), c["raw"][1].double(), node_mask.double())
    c["noise_e"] = oracle.symmetric_edge_noise(c["raw"][2].double(), edge_mask.double())
    c["mol"] = torch.tensor([7, (1 << 33) + 5, 0, 123456789, 99], dtype=torch.int64)
    return c


def _device_operands(c, d, row):
    """Fresh device operands: masked entries of the in-place state and the whole of the mean outputs carry the sentinel; with c == 0
    the history is NaN everywhere."""
    nm = c["node_mask"].bool().expand(-1, -1, 9)
    em = c["edge_mask"].reshape(5, 29, 29, 1).bool().expand(-1, -1, -1, 2)
    x = torch.where(nm, c["x"], torch.full_like(c["x"], SENTINEL)).to(d)
    ex = torch.where(em, c["ex"], torch.full_like(c["ex"], SENTINEL)).to(d)
    xm, em_out = torch.full((5, 29, 9), SENTINEL, device=d), torch.full((5, 29, 29, 2), SENTINEL, device=d)
    if row[2] != 0.0:
        h, eh = c["h"].to(d), c["eh"].to(d)
    else:
        h, eh = torch.full((5, 29, 9), float("nan"), device=d), torch.full((5, 29, 29, 2), float("nan"), device=d)
    return x, ex, c["p"].to(d), c["ep"].to(d), h, eh, xm, em_out, nm, em


def _check_outputs(c, row, temp, got, noise_x, noise_e, gate, tag):
    x, ex, xm, em_out, nm, em = got
    want = mirror_step(row, temp, c["x"], c["ex"], c["p"], c["ep"], c["h"], c["eh"], noise_x, noise_e, c["node_mask"], c["edge_mask"])
    for t, w, mask, name in ((xm, want[0], nm, "x_mean"), (x, want[1], nm, "x"), (em_out, want[2], em, "edge_mean"), (ex, want[3], em, "edge_x")):
        t = t.cpu()
        assert bool(torch.isfinite(t).all()), f"{tag}: {name} not finite"
        assert_close(t[mask], w[mask], gate, f"{tag}: {name}")
        assert bool((t[~mask] == SENTINEL).all()), f"{tag}: {name} wrote a masked entry"
    assert torch.equal(ex, ex.transpose(1, 2)) and torch.equal(em_out, em_out.transpose(1, 2)), f"{tag}: edges not symmetric bit for bit"
    pos = torch.where(nm[:, :, :3], x.cpu()[:, :, :3], torch.zeros(()))
    assert float((pos.sum(1) / c["node_mask"].sum(1)).abs().max()) <= 1e-5, f"{tag}: centre of mass"


@pytest.mark.parametrize("kind", list(ROWS))
def test_solver_step_host_noise_vs_mirror(gpu_device, kernel_case, kind):
    c, d, row, temp = kernel_case, gpu_device, ROWS[kind], 0.9
    x, ex, p, ep, h, eh, xm, em_out, nm, em = _device_operands(c, d, row)
    raw = to_dev(c["raw"], d) if row[3] != 0.0 else (None, None, None)
    hist = (h, eh) if kind != "last_row" else (None, None)                # c == 0: NaN history or none at all, the same result
    c["eng"].solver_step(c["L"], *row, temp, x, ex, p, ep, hist[0], hist[1], raw[0], raw[1], raw[2], xm, em_out)
    torch.cuda.synchronize()
    _check_outputs(c, row, temp, (x, ex, xm, em_out, nm, em), c["noise_x"], c["noise_e"], 2e-6, kind)


@pytest.mark.parametrize("kind", list(ROWS))
def test_solver_step_philox_vs_oracle_and_device_row(gpu_device, kernel_case, kind):
    """The Philox variant against oracle/philox.py at draw = step + 1, and the device-row variant bit for bit against it: it reads row and
    draw index from device memory, and leaves this step's prediction in the history (valid entries only) after reading the old one."""
    from diffspectra_amd.sampling import SOLVER_ROW
    c, d, row, temp, step = kernel_case, gpu_device, ROWS[kind], 0.9, 17
    mol = c["mol"].to(d)
    x, ex, p, ep, h, eh, xm, em_out, nm, em = _device_operands(c, d, row)
    c["eng"].solver_step_philox(c["L"], *row, temp, SEED, step, mol, x, ex, p, ep, h, eh, xm, em_out)
    torch.cuda.synchronize()
    noise_x, noise_e = _philox_noise(c["node_mask"], c["mol"], step + 1)
    _check_outputs(c, row, temp, (x, ex, xm, em_out, nm, em), noise_x, noise_e, 1e-5, kind)
    # device row: a table of 32-byte rows with the row at index `step`, every other row poisoned
    table = torch.full((step + 2, SOLVER_ROW), float("nan"))
    table[step, :5] = torch.tensor([*row, -1.25])
    table, step_dev, nl = table.to(d), torch.full((1,), step - 1, dtype=torch.int32, device=d), torch.zeros(5, device=d)
    c["eng"].solver_step_begin(table, step + 2, step_dev, 5, nl)
    assert int(step_dev) == step and nl.tolist() == [-1.25] * 5
    x2, ex2, p2, ep2, h2, eh2, xm2, em2, _, _ = _device_operands(c, d, row)
    h2, eh2 = torch.where(nm.to(d), h2, torch.full_like(h2, SENTINEL)), torch.where(em.to(d), eh2, torch.full_like(eh2, SENTINEL))
    c["eng"].solver_step_philox_dev(c["L"], table, step_dev, temp, SEED, mol, x2, ex2, p2, ep2, h2, eh2, xm2, em2)
    torch.cuda.synchronize()
    for a, b, name in ((x2, x, "x"), (ex2, ex, "edge_x"), (xm2, xm, "x_mean"), (em2, em_out, "edge_mean")):
        assert torch.equal(a, b), f"{kind}: device-row {name} differs from the scalar-argument kernel"
    assert torch.equal(h2.cpu()[nm], c["p"][nm]) and torch.equal(eh2.cpu()[em], c["ep"][em])
    assert bool((h2.cpu()[~nm] == SENTINEL).all()) and bool((eh2.cpu()[~em] == SENTINEL).all())
    # the last step of a table clamps: begin at S-1 stays at S-1
    c["eng"].solver_step_begin(table, step + 1, step_dev, 5, nl)
    assert int(step_dev) == step


def test_solver_step_argument_checks(gpu_device, kernel_case):
    import ctypes as C
    from diffspectra_amd import engine as E
    c, d = kernel_case, gpu_device
    lib, Lc, ERR = c["eng"].lib, C.byref(c["L"].c), E.CONSTS["DS_ERR_ARG"]
    x, ex, p, ep, h, eh, xm, em_out, _, _ = _device_operands(c, d, ROWS["second_order_ode"])
    P = E._ptr
    x0, mol = x.clone(), c["mol"].to(d)
    ok = lambda st: st == 0
    # c != 0 needs both histories
    assert lib.ds_solver_step(Lc, 0.8, 0.3, -0.1, 0.0, 1.0, P(x), P(ex), P(p), P(ep), None, P(eh), None, None, None, P(xm), P(em_out), None) == ERR
    assert lib.ds_solver_step(Lc, 0.8, 0.3, -0.1, 0.0, 1.0, P(x), P(ex), P(p), P(ep), P(h), None, None, None, None, P(xm), P(em_out), None) == ERR
    assert lib.ds_solver_step_philox(Lc, 0.8, 0.3, -0.1, 0.2, 1.0, 1, 0, P(mol), P(x), P(ex), P(p), P(ep), None, None, P(xm), P(em_out),
                                     None) == ERR
    # d != 0 needs the three draws; the device-row form needs its history whatever the row says
    assert lib.ds_solver_step(Lc, 0.8, 0.3, 0.0, 0.2, 1.0, P(x), P(ex), P(p), P(ep), None, None, None, None, None, P(xm), P(em_out), None) == ERR
    tab, stp = torch.zeros(2, 8, device=d), torch.zeros(1, dtype=torch.int32, device=d)
    assert lib.ds_solver_step_philox_dev(Lc, P(tab), P(stp), 1.0, 1, P(mol), P(x), P(ex), P(p), P(ep), None, None, P(xm), P(em_out),
                                         None) == ERR
    # the float2 operands must be 8-byte aligned
    assert lib.ds_solver_step(Lc, 0.8, 0.3, 0.0, 0.0, 1.0, P(x), P(ex) + 4, P(p), P(ep), None, None, None, None, None, P(xm), P(em_out), None) == ERR
    torch.cuda.synchronize()
    assert torch.equal(x, x0)                                            # nothing was launched
    assert ok(lib.ds_solver_step(Lc, 0.8, 0.3, 0.0, 0.0, 1.0, P(x), P(ex), P(p), P(ep), None, None, None, None, None, P(xm), P(em_out),
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ order of convergence

_TRIPLES = ((0.7, 0.5, 1.1), (-1.3, 1.5, -0.4), (0.2, 0.05, 0.9))       # (mu, s, x_T), cycled over the elements


@pytest.fixture(scope="module")
def gaussian_errors(gpu_device):
    """max |x - exact| at t_{S-1} after S-1 deterministic steps through ds_solver_step on molecules of 2, 5 and 29 atoms, the analytic
    denoiser of N(mu, s^2) computed in torch (fp64, rounded to the kernel's fp32 operand) between the launches."""
    from diffspectra_amd import filler, sampling as S
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    d = gpu_device
    cfg, model = gpu_model("allspectra", d)
    eng = model.module.engine()
    node_mask, edge_mask = filler.masks_from_n_atoms([2, 5, 29])
    L, _ = eng.layout_for(node_mask, edge_mask, validate=True)
    B, N = 3, 29
    tri = torch.tensor(_TRIPLES, dtype=torch.float64)
    kx = torch.arange(B * N * 9).reshape(B, N, 9) % 3
    i, j = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    ke = ((torch.minimum(i, j) * 31 + torch.maximum(i, j) * 7).reshape(1, N, N, 1) + torch.arange(2).reshape(1, 1, 1, 2)
          + torch.arange(B).reshape(B, 1, 1, 1)) % 3                     # symmetric in (i, j)
    par = lambda k, col: tri[:, col][k]
    mu_x, s_x, xT = par(kx, 0), par(kx, 1), par(kx, 2).clone()
    mu_e, s_e, eT = par(ke, 0), par(ke, 1), par(ke, 2)
    nm = node_mask.double()
    xT = xT * nm
    xT[:, :, :3] -= (xT[:, :, :3].sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm      # positions: per-molecule mean removed
    em = edge_mask.reshape(B, N, N, 1).double()
    eT = eT * em
    assert torch.equal(eT, eT.transpose(1, 2))
    xT, eT = xT.float().double(), eT.float().double()                   # the fp32 state the kernel starts from
    vx, ve = node_mask.bool().expand(-1, -1, 9), edge_mask.reshape(B, N, N, 1).bool().expand(-1, -1, -1, 2)
    ns = NoiseScheduleVP("cosine")
    errs = {}
    dmu_x, ds_x, dmu_e, ds_e, dnm, dem = (v.to(d) for v in (mu_x, s_x, mu_e, s_e, nm, em))
    for solver in ("ddim", "dpmpp_2m"):
        for steps in (32, 64, 128):
            t = S.time_grid(ns, 1e-3, steps, "logSNR")
            rows = S.solver_table(ns, t, solver).float().tolist()
            alpha, sigma = (v.tolist() for v in ns.marginal_prob(t))
            x, ex = xT.float().to(d), eT.float().to(d)
            xm, emn = torch.zeros(B, N, 9, device=d), torch.zeros(B, N, N, 2, device=d)
            pred = [(torch.zeros_like(x), torch.zeros_like(ex)) for _ in range(2)]
            for k in range(steps - 1):
                a, b, c, dd, _ = rows[k]
                p, pe = pred[k & 1]
                p.copy_((gaussian_denoiser(x.double(), alpha[k], sigma[k], dmu_x, ds_x) * dnm).float())
                pe.copy_((gaussian_denoiser(ex.double(), alpha[k], sigma[k], dmu_e, ds_e) * dem).float())
                h, he = pred[(k & 1) ^ 1] if c != 0.0 else (None, None)
                assert dd == 0.0
                eng.solver_step(L, a, b, c, dd, 1.0, x, ex, p, pe, h, he, None, None, None, xm, emn)
            torch.cuda.synchronize()
            want_x = gaussian_flow(xT, alpha[0], sigma[0], alpha[-1], sigma[-1], mu_x, s_x)
            want_e = gaussian_flow(eT, alpha[0], sigma[0], alpha[-1], sigma[-1], mu_e, s_e)
            assert torch.equal(ex, ex.transpose(1, 2))
            errs[solver, steps] = max(float((x.double().cpu() - want_x)[vx].abs().max()), float((ex.double().cpu() - want_e)[ve].abs().max()))
    return errs


def test_order_of_convergence_through_the_kernels(gaussian_errors):
    """dpmpp_2m is second order (error ratio >= 3 per doubling, theory 4), ddim first order (ratio in [1.8, 2.2], theory 2), and 32 steps
    of the former beat 128 of the latter.  fp64 figures of the same experiment: 2M 3.54e-3, 8.80e-4, 2.19e-4; DDIM 4.4e-2, 2.2e-2, 1.1e-2."""
    e = gaussian_errors
    print("[solver convergence]", {f"{k[0]}@{k[1]}": f"{v:.3e}" for k, v in e.items()})
    for lo, hi in ((32, 64), (64, 128)):
        assert e["dpmpp_2m", lo] / e["dpmpp_2m", hi] >= 3.0, (lo, hi, e)
        assert 1.8 <= e["ddim", lo] / e["ddim", hi] <= 2.2, (lo, hi, e)
    assert e["dpmpp_2m", 32] < e["ddim", 128], e


# ------------------------------------------------------------------------------------------------ the sampler

@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m", "sde_dpmpp_2m"])
def test_solver_graph_replay_equals_eager(gpu_device, solver):
    """hipGraph replay (device-side row, history buffer owned by the sampler) against the eager launch sequence (ping-pong predictions) bit
    for bit: the seven molecules and 13 steps of test_graph_replay_equals_eager, whole, in slices, and switching after three eager steps."""
    from diffspectra_amd import filler, sampling as S
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    cfg, model = gpu_model("allspectra", gpu_device)
    cfg = cfg.clone()
    cfg.sampling.steps, cfg.sampling.method = 13, solver
    d = gpu_device
    n_atoms = [5, 29, 2, 17, 9, 1, 12]
    node_mask, edge_mask = filler.masks_from_n_atoms(n_atoms)
    ctx = to_dev(cases.spectra_for("allspectra", len(n_atoms), salt=9), d)
    ids = torch.arange(100, 100 + len(n_atoms))
    outs = {}
    with swapped_weights(model, lambda sd: cases.readout_diverse(sd, "allspectra_S5")):
        for mode, slices in (("eager", [13]), ("graph", [13]), ("graph_sliced", [1, 1, 4, 7]), ("graph_late", [3, 10])):
            sampler = S._make_sampler(cfg, NoiseScheduleVP("cosine"), 1e-3, 0.9)
            assert isinstance(sampler, S.MultistepSampler)
            sampler.use_graph = mode != "eager"
            st = sampler.begin(model, None, node_mask.to(d), edge_mask.to(d), None, ctx, mol_ids=ids, seed=7)
            if mode == "graph_late":
                sampler.use_graph = False
            for k, n in enumerate(slices):
                if mode == "graph_late" and k == 1:
                    sampler.use_graph = True
                done = sampler.advance(st, n)
            assert done and st.i == 13
            assert (st.graph is not None) == (mode != "eager")
            outs[mode] = (st.x_mean.clone(), st.edge_mean.clone(), st.x.clone())
        anc = cfg.clone()
        anc.sampling.method = "ancestral"
        ref = S._make_sampler(anc, NoiseScheduleVP("cosine"), 1e-3, 0.9)
        x_anc, _ = ref.sampling(model, None, node_mask.to(d), edge_mask.to(d), None, ctx, mol_ids=ids, seed=7)
    for mode in ("graph", "graph_sliced", "graph_late"):
        for a, b in zip(outs["eager"], outs[mode]):
            assert torch.equal(a, b), f"{solver}: {mode} differs from the eager launch sequence"
    assert bool(torch.isfinite(outs["eager"][0]).all()) and float(outs["eager"][0].abs().max()) > 0.1
    assert not torch.equal(outs["eager"][0], x_anc)                      # and it is another sampler than the ancestral one


@pytest.mark.parametrize("self_cond", ["ori", "clamp"])
def test_sampler_steps_follow_the_table(gpu_device, self_cond):
    """The host wiring, step by step (a pass advanced in slices of one, noise injected through ``noise_fn``): every step applies its own
    table row to the state, the prediction the model just wrote and - in the second-order rows - the previous step's prediction, which
    with 'clamp' self-conditioning is the tensor clamped in place; the last row draws no noise."""
    import oracle
    from diffspectra_amd import filler, sampling as S
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    cfg, model = gpu_model("allspectra", gpu_device)
    cfg = cfg.clone()
    cfg.sampling.steps, cfg.sampling.method, cfg.model.self_cond_type = 5, "sde_dpmpp_2m", self_cond
    d, temp = gpu_device, 0.9
    n_atoms = [5, 29, 2]
    B, N = 3, 29
    x0, e0, node_mask, edge_mask = filler.synthetic_state(n_atoms, "hk.x")
    ctx = to_dev(cases.spectra_for("allspectra", B, salt=9), d)
    raws = [(filler.normal(f"hk.rp{i}", (B, N, 3)), filler.normal(f"hk.rf{i}", (B, N, 6)), filler.normal(f"hk.re{i}", (B, 2, N, N)))
            for i in range(5)]
    vx, ve = node_mask.bool().expand(-1, -1, 9), edge_mask.reshape(B, N, N, 1).bool().expand(-1, -1, -1, 2)
    calls = []
    with swapped_weights(model, lambda sd: cases.readout_diverse(sd, "allspectra_S5")):
        sampler = S._make_sampler(cfg, NoiseScheduleVP("cosine"), 1e-3, temp)
        sampler.noise_fn = lambda i: (calls.append(i), raws[i])[1]
        rows = sampler.coefficient_table().tolist()
        assert [r[2] != 0.0 for r in rows] == [False, True, True, False, False]      # first, second, second, lower-order final, last
        st = sampler.begin(model, x0, node_mask.to(d), edge_mask.to(d), e0, ctx)
        prev = None
        for i in range(5):
            xb, eb = st.x.clone(), st.edge_x.clone()
            done = sampler.advance(st, 1)
            assert st.i == i + 1 and done == (i == 4)
            p, pe = st.pred[i & 1], st.edge_pred[i & 1]
            h, he = st.pred[(i & 1) ^ 1], st.edge_pred[(i & 1) ^ 1]
            if prev is not None:
                assert torch.equal(h, prev[0]) and torch.equal(he, prev[1])           # the history is what the previous update used
            if self_cond == "clamp":
                assert float(p[:, :, 3:8].cpu()[vx[:, :, 3:8]].abs().max()) <= 0.25    # clamped in place before the update read it
            second = rows[i][2] != 0.0
            nx = oracle.combined_noise(raws[i][0].double(), raws[i][1].double(), node_mask.double())
            ne = oracle.symmetric_edge_noise(raws[i][2].double(), edge_mask.double())
            want = mirror_step(rows[i][:4], temp, xb, eb, p, pe, h if second else None, he if second else None, nx, ne, node_mask, edge_mask)
            for got, w, mask, name in ((st.x_mean, want[0], vx, "x_mean"), (st.x, want[1], vx, "x"), (st.edge_mean, want[2], ve, "edge_mean"),
                                       (st.edge_x, want[3], ve, "edge_x")):
                assert_close(got.cpu()[mask], w[mask], 2e-6, f"{self_cond} step {i}: {name}")
            prev = (p.clone(), pe.clone())
    assert calls == [0, 1, 2, 3]                                                       # d == 0 in the last row: no draw is asked for
    assert torch.equal(st.x_mean.cpu()[vx], prev[0].cpu()[vx])                        # row S-1 returns the prediction


@pytest.mark.parametrize("solver", ["dpmpp_2m", "sde_dpmpp_2m"])
def test_solver_sampling_end_to_end(gpu_device, solver):
    """get_cond_sampling_eval_fn with a multistep method, 6 steps and 9 slots: the molecules do not depend on the micro-batch size, Top-K
    draws distinct candidates with slot 0 shared, another seed gives other molecules, everything is finite."""
    S, cfg, model, ds, n_atoms, ns, inv = _philox_sampling_setup(gpu_device, steps=6)
    cfg.sampling.method = solver
    with swapped_weights(model, lambda sd: cases.readout_diverse(sd, "allspectra_S5")):
        a, gt_pos, gt_mols = S.get_cond_sampling_eval_fn(cfg, ns, 4, 9, inv, ds)(model)
        b, _, _ = S.get_cond_sampling_eval_fn(cfg, ns, 9, 9, inv, ds)(model)
        c, _, _ = S.get_cond_sampling_eval_fn(cfg, ns, 1, 9, inv, ds)(model)
        k3, gt3, mols3 = S.get_cond_sampling_eval_fn(cfg, ns, 5, 3, inv, ds, top_k=3)(model)
        other = cfg.clone()
        other.sampling.seed = 43
        d43, _, _ = S.get_cond_sampling_eval_fn(other, ns, 4, 9, inv, ds)(model)
    torch.manual_seed(42)
    perm = torch.randperm(len(ds)).tolist()
    assert gt_mols == [f"mol{i}" for i in perm[:9]]
    assert [m[0].shape[0] for m in a] == [n_atoms[i] for i in perm[:9]]
    assert _same_molecules(a, b) and _same_molecules(a, c), "molecules depend on the micro-batch size"
    assert not _same_molecules(a, d43)
    assert len(k3) == 9 and mols3 == [f"mol{i}" for i in perm[:3] for _ in range(3)]
    for i in range(3):
        assert float((k3[3 * i][0] - k3[3 * i + 1][0]).abs().max()) > 1e-3
    assert torch.equal(k3[0][0], a[0][0])
    for mols in (a, k3, d43):
        assert all(bool(torch.isfinite(m[0]).all()) and bool(torch.isfinite(m[2]).all()) for m in mols)
