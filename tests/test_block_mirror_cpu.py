"""CPU pins of tests/block_mirror.py, the float64 yardstick of the sampling block kernels (no GPU needed):
  * run free (every stage fed by the mirror's own previous stage) it reproduces ``oracle.dmt_forward`` evaluated in fp64 - h, e (both directions)
    and pos of all 8 blocks and the final outputs to 1e-11 of each tensor's largest magnitude;
  * a numpy emulation of the split-fp16 product (both planes rounded to nearest, a1 w1 + (a1 w2 + a2 w1) / 2048, fp32 accumulation in a
    shuffled order) stays inside ``split_bound`` for K = 64 .. 768 on filler and checkpoint-like operands - a condition on the BOUND, shown
    with the reference arithmetic alone - and three defects of that arithmetic exceed it;
  * the general-step inputs of the GPU layouts have the adjacency patterns the GPU tests rely on;
  * the teacher-forced comparison itself passes on the mirror's own fp32-rounded buffers and fails on a displaced pair row."""
import numpy as np
import pytest
import torch

import oracle
from oracle import dmt as odmt
from tests import block_mirror as bm
from tests.golden import cases
from tests.helpers import procedural_state_dict, checkpoint_like, oracle_forward_f64, oracle_edge_maps

LAYOUTS, COUNTS = bm.LAYOUTS, bm.COUNTS
LIMIT = 1e-11


def temb_f64(sd, cfg, a):
    """time_mlp(noise_level) + cond_lin(SpecFormer(context)) in fp64 (dmt.py:348-354): the input of every adaLN Linear."""
    torch.set_default_dtype(torch.float64)
    try:
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        ctx = a["context"]
        ctx = [c.double() for c in ctx] if isinstance(ctx, (list, tuple)) else ctx.double()
        return odmt.time_embedding(sd64, a["noise_level"].double()) + oracle.context_embedding(sd64, ctx, cfg)
    finally:
        torch.set_default_dtype(torch.float32)


def close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= LIMIT * max(scale, 1e-300), f"{what}: {err:.3e} against a scale of {scale:.3e}"
    return err / max(scale, 1e-300)


@pytest.mark.parametrize("version", ["ir", "allspectra"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "general"])
@pytest.mark.parametrize("layout", ["ragged", "one_pair"])
def test_free_run_equals_fp64_oracle(layout, first, version):
    n_atoms = LAYOUTS[layout]
    cfg, sd = procedural_state_dict(version)
    a = bm.stage_inputs(layout, first, version)
    tb = bm.tables(n_atoms)
    assert (tb["Nn"], tb["Pp"]) == COUNTS[layout]
    ref_xh, ref_edge, dbg = oracle_forward_f64(sd, cfg, a, return_debug=True)
    blocks, out, _ = bm.forward(sd, cfg, n_atoms, a["xh"], a["edge_x"], a["cond_x"], a["cond_edge_x"], temb_f64(sd, cfg, a))
    N = a["xh"].shape[1]
    nd = bm.dense_tables(tb, N)[0]
    fwd, bwd, _ = oracle_edge_maps(a["node_mask"].reshape(len(n_atoms), N) != 0, nd, tb["pair_a"], tb["pair_b"])
    worst = 0.0
    for k in range(8):
        worst = max(worst, close(blocks[k]["h"], dbg[f"h_{k}"][nd], f"h_{k}"), close(blocks[k]["pos"], dbg[f"pos_{k}"][nd], f"pos_{k}"),
                    close(blocks[k]["e"], dbg[f"e_{k}"][fwd], f"e_{k} a->b"), close(blocks[k]["e"], dbg[f"e_{k}"][bwd], f"e_{k} b->a"))
    worst = max(worst, close(out["out_xh"].ref, ref_xh, "out_xh"), close(out["out_edge"].ref, ref_edge, "out_edge"))
    print(f"[block mirror vs fp64 oracle] {layout} {'first' if first else 'general'} {version}: worst |diff| / max |ref| = {worst:.2e}")


# ------------------------------------------------------------------------------------------------ the split-fp16 bound
def _operands(stat, M, K, N, rng):
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) * 0.3
    A[:, ::7] *= 1e-3                                   # mixed magnitudes inside a row
    if stat == "checkpoint":
        A *= 30.0                                       # adaLN scale x 30
        A[:, [3, K // 3, K - 5]] *= 300.0               # three channels ~1e4 (inside fp16's range: the kernels saturate beyond it)
        W[::3] *= 1e-5                                  # weight rows ~1e-6
        A[::5] *= 1e-7                                  # rows whose low planes are fp16 subnormals (the floor term)
    return A, W, b


@pytest.mark.parametrize("stat", ["filler", "checkpoint"])
@pytest.mark.parametrize("K", [64, 128, 256, 768])
def test_split_emulation_stays_inside_the_bound(K, stat):
    rng = np.random.default_rng(1000 + K)
    A, W, b = _operands(stat, 24, K, 40, rng)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + b
    bound = bm.split_bound(A, W, b).numpy()
    assert float(np.abs(A).max()) < 65504.0
    worst = 0.0
    for _ in range(3):                                  # three summation orders
        got = bm.emulate_split_product(A, W, b, rng)
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - ref) / bound).max()))
    print(f"[split-fp16 emulation] K {K} {stat}: largest |emulation - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def _coherent(K, rng, frac):
    """Operands on which a defect of the low planes has ONE sign in every term: a = (1 + frac 2^-10) 2^j, w > 0."""
    A = ((1.0 + frac * 2.0 ** -10) * 2.0 ** rng.integers(-2, 3, (16, K))).astype(np.float32)
    W = (rng.uniform(0.5, 1.0, (32, K)) / np.sqrt(K)).astype(np.float32)
    return A, W


@pytest.mark.parametrize("K", [64, 128, 256, 768])
def test_defects_of_the_split_arithmetic_exceed_the_bound(K):
    """The accumulation term of the bound grows with K, so a defect of relative size 2^-11 per term is caught where it does not cancel; these
    operands make it coherent.  The sound emulation stays inside the bound on the same operands."""
    rng = np.random.default_rng(2000 + K)
    for what, frac, kw in (("a2 w1 dropped", 0.45, dict(drop_cross=True)), ("plane 1 truncated", 0.9, dict(truncate=True))):
        A, W = _coherent(K, rng, frac)
        ref = A.astype(np.float64) @ W.astype(np.float64).T
        bound = bm.split_bound(A, W).numpy()
        good = float((np.abs(bm.emulate_split_product(A, W, None, rng) - ref) / bound).max())
        bad = float((np.abs(bm.emulate_split_product(A, W, None, rng, **kw) - ref) / bound).max())
        print(f"[split-fp16 defects] K {K} {what}: sound {good:.3f}, defective {bad:.2f} of the bound")
        assert good <= 1.0 and bad > 1.0, (what, good, bad)
    A, W, b = _operands("filler", 24, K, 40, rng)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + b
    got = bm.emulate_split_product(A, W, b, rng)
    got[[7, 8]] = got[[8, 7]]                            # one row's result lands in its neighbour's place
    bad = float((np.abs(got - ref) / bm.split_bound(A, W, b).numpy()).max())
    print(f"[split-fp16 defects] K {K} row displaced: {bad:.3g} of the bound")
    assert bad > 1.0


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
@pytest.mark.parametrize("layout", ["ragged", "big"])
def test_general_step_inputs_have_the_adjacency_patterns(layout):
    n_atoms = LAYOUTS[layout]
    cfg, sd = procedural_state_dict("ir")
    a = bm.stage_inputs(layout, False)
    tb = bm.tables(n_atoms)
    assert (tb["Nn"], tb["Pp"]) == COUNTS[layout]
    _, adj, flag = bm.init(sd, cfg, tb, a["xh"], a["edge_x"], a["cond_x"], a["cond_edge_x"], torch.zeros(len(n_atoms), bm.ADA_COLS))
    all_clear, mixed0, mixed1 = bm.adjacency_patterns(n_atoms, adj)
    assert flag == 1
    assert all_clear, "no target whose incoming cond_adj_2d bits are all 0 (uniform extra-head softmax)"
    assert mixed0, "no target with mixed cond_adj_2d bits"
    assert mixed1, "no target with mixed cond_adj_spatial bits"
    _, adj1, flag1 = bm.init(sd, cfg, tb, a["xh"], a["edge_x"], None, None, torch.zeros(len(n_atoms), bm.ADA_COLS))
    assert flag1 == 0 and bool((adj1 == 3).all())


# ------------------------------------------------------------------------------------------------ the comparison itself
def test_teacher_forced_comparison_passes_on_the_mirror_and_catches_a_displaced_row():
    n_atoms = LAYOUTS["ragged"]
    cfg, sd = procedural_state_dict("ir")
    sd = checkpoint_like(sd)
    a = bm.stage_inputs("ragged", False)
    tb = bm.tables(n_atoms)
    ada = bm.ada_table(sd, temb_f64(sd, cfg, a)).float()
    i0, adj, _ = bm.init(sd, cfg, tb, a["xh"], a["edge_x"], a["cond_x"], a["cond_edge_x"], ada)
    h, e, pos = (i0[k].ref.float() for k in ("h", "e", "pos"))
    obs = {k: v.ref.float() for k, v in bm.block(sd, 0, tb, h, e, pos, adj, ada).items()}        # what an exact fp32 kernel would leave behind
    refs = bm.teacher_forced_block(sd, 0, tb, h, e, pos, adj, ada, obs)
    for name, dev, share, idx in bm.shares(refs, obs, bm.BLOCK_BUFFERS):
        print(f"[teacher forcing on the mirror] {name:10s} max |diff| {dev:.2e}  share {share:.3f} at {idx}")
        assert share <= 1.0, (name, share, idx)
    for name in ("ed", "tr", "ye", "alpha"):
        bad = dict(obs)
        t = obs[name].clone()
        t[[40, 41]] = t[[41, 40]]
        bad[name] = t
        share = dict((r[0], r[2]) for r in bm.shares(refs, bad, [name]))[name]
        assert share > 1.0, (name, share)
