"""CPU: the coefficient algebra of the multistep samplers (``sampling.solver_table``, ``time_grid``, ``NoiseScheduleVP.inverse_lambda``)
in fp64 against the reference's ancestral update and against the closed forms of a Gaussian data distribution (tests/solver_mirror.py).
Parity with the DPM-Solver code base or with ``diffusers`` is not pinned: neither is available to these tests."""
import math

import pytest
import torch

from diffspectra_amd import sampling as S
from diffspectra_amd.config import qm9s_config
from diffspectra_amd.noise_schedule import NoiseScheduleVP
from tests.solver_mirror import propagate_moments

EPS = 1e-3


def _ancestral_rows_f64(ns, t):
    """(c_x, c_pred, sigma) of the reference's ancestral loop (sampling.py:576-580,604-606) in fp64; s_array as sampling.py:558."""
    s = torch.cat([t[1:], torch.zeros(1, dtype=torch.float64)])
    alpha_t, sigma_t = ns.marginal_prob(t)
    alpha_s, sigma_s = ns.marginal_prob(s)
    alpha_ts = alpha_t / alpha_s
    sigma2_ts = sigma_t ** 2 - alpha_ts ** 2 * sigma_s ** 2
    return torch.stack([alpha_ts * sigma_s ** 2 / sigma_t ** 2, alpha_s * sigma2_ts / sigma_t ** 2,
                        torch.sqrt(sigma2_ts) * sigma_s / sigma_t], dim=1)


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
@pytest.mark.parametrize("steps", [50, 1000])
def test_first_order_sde_rows_are_the_ancestral_update(schedule, steps):
    ns = NoiseScheduleVP(schedule)
    t = S.time_grid(ns, EPS, steps).double()                    # the reference's grid (fp32 linspace), every value exact in fp64
    rows = S.solver_table(ns, t, "sde_dpmpp_2m", max_order=1)
    want = _ancestral_rows_f64(ns, t)
    assert rows.dtype == torch.float64 and rows.shape == (steps, 5)
    for col, name in ((0, "a"), (1, "b"), (3, "d")):
        got, ref = rows[:-1, col], want[:-1, {0: 0, 1: 1, 3: 2}[col]]
        rel = float(((got - ref).abs() / ref.abs()).max())
        assert rel <= 1e-12, (name, rel)
    assert float(rows[:, 2].abs().max()) == 0.0                 # first order: no history operand anywhere
    assert rows[-1, :4].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert want[-1].tolist() == [0.0, 1.0, 0.0]                 # and the reference's last step is that row too
    lam = ns.marginal_lambda(t)
    assert float((rows[:, 4] - 2.0 * lam).abs().max()) <= 1e-12


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_tables_are_finite_and_fall_back_to_first_order(solver, spacing):
    ns = NoiseScheduleVP("cosine")
    for steps in (1, 2, 3, 7):
        for lof in (True, False):
            t = S.time_grid(ns, EPS, steps, spacing)
            rows = S.solver_table(ns, t, solver, lower_order_final=lof)
            assert rows.shape == (steps, 5) and bool(torch.isfinite(rows).all()), (steps, lof)
            assert rows[-1, :4].tolist() == [0.0, 1.0, 0.0, 0.0]
            second = [i for i in range(steps) if float(rows[i, 2]) != 0.0]
            want = [] if solver == "ddim" else [i for i in range(1, steps - 1) if not (lof and i == steps - 2)]
            assert second == want, (steps, lof, second)
            noisy = [i for i in range(steps) if float(rows[i, 3]) != 0.0]
            assert noisy == (list(range(steps - 1)) if solver == "sde_dpmpp_2m" else [])
            first = S.solver_table(ns, t, solver, lower_order_final=lof, max_order=1)
            for i in range(steps - 1):                              # b + c = k: a second-order row redistributes the first-order weight
                assert abs(float(rows[i, 1] + rows[i, 2] - first[i, 1])) <= 1e-14 * abs(float(first[i, 1])) + 1e-300
                assert float(rows[i, 0]) == float(first[i, 0]) and float(rows[i, 3]) == float(first[i, 3])
    with pytest.raises(ValueError):
        S.solver_table(ns, S.time_grid(ns, EPS, 4), "unipc")
    with pytest.raises(ValueError):
        S.time_grid(ns, EPS, 4, "quadratic")


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_sde_moments_on_a_gaussian(schedule):
    """sde_dpmpp_2m under the linear denoiser of N(mu, s^2): the mean of x at t_{S-1} is exact (a alpha_i + b + c = alpha_{i+1} row by
    row), the variance converges at second order on the 'logSNR' grid: its error falls by >= 3 per doubling of S from 16 to 128 (theory: 4).

    The variance recursion does not depend on mu; s = 1 is the case in which the marginal N(alpha mu, alpha^2 s^2 + sigma^2) keeps unit
    variance at every t, so the whole error is the solver's and no step of the 16-point grid lies in the stiff region sigma_t << s that a
    narrower distribution has near eps.  Measured (cosine, lower_order_final off): 9.45e-2, 3.12e-2, 8.00e-3, 1.99e-3, ratios 3.03, 3.90,
    4.02.  For s = 0.5 the 16-step grid is not yet asymptotic: 2.31e-2, 7.79e-3, 2.00e-3, 4.97e-4, ratios 2.96, 3.90, 4.02."""
    ns = NoiseScheduleVP(schedule)
    mu, s = 0.7, 1.0
    errs = []
    for steps in (16, 32, 64, 128):
        t = S.time_grid(ns, EPS, steps, "logSNR")
        rows = S.solver_table(ns, t, "sde_dpmpp_2m", lower_order_final=False)
        alpha, sigma = ns.marginal_prob(t)
        mean, var = propagate_moments(rows, alpha, sigma, mu, s)
        assert abs(float(mean - alpha[-1] * mu)) <= 1e-12, steps
        errs.append(abs(float(var - (alpha[-1] ** 2 * s * s + sigma[-1] ** 2))))
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print(f"[sde moments] {schedule}: variance errors {errs}, ratios {ratios}")
    assert all(r >= 3.0 for r in ratios), (errs, ratios)
    # the ODE solvers carry the mean exactly as well, with and without the first-order last step
    for solver in ("ddim", "dpmpp_2m"):
        t = S.time_grid(ns, EPS, 16, "logSNR")
        alpha, sigma = ns.marginal_prob(t)
        mean, _ = propagate_moments(S.solver_table(ns, t, solver), alpha, sigma, mu, s)
        assert abs(float(mean - alpha[-1] * mu)) <= 1e-12, solver


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_inverse_lambda_round_trip_and_logsnr_grid(schedule):
    ns = NoiseScheduleVP(schedule)
    t = torch.linspace(EPS, ns.T, 2001, dtype=torch.float64)
    back = ns.inverse_lambda(ns.marginal_lambda(t))
    assert back.dtype == torch.float64 and float((back - t).abs().max()) <= 1e-9
    for steps in (1, 2, 5, 64):
        g = S.time_grid(ns, EPS, steps, "logSNR")
        assert g.dtype == torch.float64 and g.shape == (steps,)
        assert float(g[0]) == ns.T and (steps == 1 or float(g[-1]) == EPS)           # the end points exactly
        assert bool((g[1:] < g[:-1]).all())
        lam = ns.marginal_lambda(g)
        if steps > 2:
            h = lam[1:] - lam[:-1]
            assert float((h - h.mean()).abs().max()) <= 1e-9 * float(h.mean())     # uniform in lambda
    u = S.time_grid(ns, EPS, 7)
    assert u.dtype == torch.float32 and torch.equal(u, torch.linspace(ns.T, EPS, 7))  # the reference's grid is the default


def test_factory_accepts_the_solvers_and_keeps_the_defaults():
    ns = NoiseScheduleVP("cosine")
    cfg = qm9s_config("ir", steps=9)
    assert (cfg.sampling.method, cfg.sampling.spacing, cfg.sampling.lower_order_final) == ("ancestral", "time_uniform", True)
    anc = S._make_sampler(cfg, ns, EPS, 1.0)
    assert type(anc) is S.AncestralSampler and anc.coefficient_table().shape == (9, 4)
    assert torch.equal(anc.t_array, torch.linspace(ns.T, EPS, 9))
    assert S.SOLVERS == ("ddim", "dpmpp_2m", "sde_dpmpp_2m")
    for method in S.SOLVERS:
        c = cfg.clone()
        c.sampling.method = method
        smp = S._make_sampler(c, ns, EPS, 0.8)
        assert isinstance(smp, S.MultistepSampler) and isinstance(smp, S.AncestralSampler)
        assert (smp.solver, smp.lower_order_final, smp.sampling_temperature, smp.use_graph) == (method, True, 0.8, False)
        tab = smp.coefficient_table()
        assert tab.shape == (9, 5) and tab.dtype == torch.float32
        assert torch.equal(tab, S.solver_table(ns, smp.t_array, method).float())     # fp64, then ONE cast
        assert torch.equal(smp.t_array, torch.linspace(ns.T, EPS, 9))                # 'time_uniform' is the default
        c.sampling.spacing, c.sampling.lower_order_final = "logSNR", False
        smp = S._make_sampler(c, ns, EPS, 1.0)
        assert torch.equal(smp.t_array, S.time_grid(ns, EPS, 9, "logSNR")) and smp.lower_order_final is False
        # an ancestral sampler ignores the spacing: its grid stays the reference's
        c.sampling.method = "ancestral"
        assert torch.equal(S._make_sampler(c, ns, EPS, 1.0).t_array, torch.linspace(ns.T, EPS, 9))
    # a foreign config object without the new fields keeps working
    bare = cfg.clone()
    del bare.sampling.spacing, bare.sampling.lower_order_final
    bare.sampling.method = "dpmpp_2m"
    smp = S._make_sampler(bare, ns, EPS, 1.0)
    assert smp.lower_order_final is True and torch.equal(smp.t_array, torch.linspace(ns.T, EPS, 9))
    for bad in ("ode", "DDIM", "dpmpp_3m", ""):
        c = cfg.clone()
        c.sampling.method = bad
        with pytest.raises(ValueError, match="Invalid sampling method"):
            S._make_sampler(c, ns, EPS, 1.0)
    with pytest.raises(ValueError):
        S.MultistepSampler(ns, torch.linspace(ns.T, EPS, 4), True, True, True, solver="euler")


def test_solver_abi_surface():
    """include/diffspectra_solver.h: four entry points, no structs, one constant; the graph-replayable pair mirrors the ancestral one."""
    import __graft_entry__ as g
    from diffspectra_amd import abi, engine as E
    hdr = abi.SOLVER
    assert list(hdr.prototypes) == hdr.exports("ds_solver_") == ["ds_solver_step", "ds_solver_step_philox", "ds_solver_step_begin",
                                                                 "ds_solver_step_philox_dev"]
    assert not hdr.structs and hdr.consts["DS_SOLVER_ROW"] == S.SOLVER_ROW == 8
    assert hdr.prototypes["ds_solver_step_begin"].params == abi.SAMPLING.prototypes["ds_step_begin"].params
    names = lambda fn: [n for n, _ in hdr.prototypes[fn].params]
    assert names("ds_solver_step") == ["L", "a", "b", "c", "d", "temperature", "x", "edge_x", "pred", "edge_pred", "hist", "edge_hist",
                                       "raw_pos", "raw_feat", "raw_edge", "x_mean", "edge_mean", "stream"]
    anc = [n for n, _ in abi.SAMPLING.prototypes["ds_sampler_step_philox_dev"].params]
    assert [n for n in names("ds_solver_step_philox_dev") if n not in ("hist", "edge_hist")] == anc
    g.build()
    lib = E.load_library()
    for name, proto in hdr.prototypes.items():
        assert list(getattr(lib, name).argtypes) == proto.argtypes, name
    # refused before anything is launched: no layout, and the begin call's own scalars
    assert lib.ds_solver_step(None, 1.0, 1.0, 0.0, 0.0, 1.0, *([None] * 12)) == E.CONSTS["DS_ERR_ARG"]
    assert lib.ds_solver_step_begin(None, 4, None, 2, None, None) == E.CONSTS["DS_ERR_ARG"]
    assert math.isfinite(float(S.solver_table(NoiseScheduleVP("cosine"), S.time_grid(NoiseScheduleVP("cosine"), EPS, 3), "dpmpp_2m").abs().max()))
