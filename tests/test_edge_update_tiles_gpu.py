"""k_edge_update at the edges of its 128-row workgroup tile, against the CPU oracle.

Up to the in-place split-fp16 rewrite of ``e_out`` every wave of k_edge_update owns 32 pair rows; behind the kernel's one workgroup barrier
the four wave tiles are one 128-row operand and wave ``w`` computes column chunks ``2w``, ``2w + 1`` of ``ed`` = input_lin's
``[e_out | CondGaussian]`` part for all of them.  A wave whose rows lie wholly behind ``Pp`` therefore still has to reach the barrier, leave
its tile defined and take its chunks.  What the kernel leaves after block 0 and block 1 - ``ws.e``, ``ws.ed`` and the block's 16 columns of
``ws.edge_hids`` - is compared with the same lines of ``oracle.dmt`` (``_mix_block``'s ``h_edge_out``; ``_equi_update``'s ``input_lin`` on the
``[edge_attr | dist]`` columns plus its bias; ``edge_<blk>``).  Tolerance: ``TOL_KERNEL`` with the relative term of tests/test_hip_parity.py,
not one of this file's own.

Batches: ``[2]`` (``Pp`` = 1: one row, three waves without rows); ``[9]`` (36: wave 1 holds 4 rows, waves 2 and 3 none); ``[15]`` (105: the
last wave holds a partial tile); ``[17]`` (136: a second workgroup with 8 rows); ``[29, 12]`` (472: adaLN rows of two molecules inside one
128-row tile, a partial last workgroup); ``[1, 3, 1]`` (molecules without pairs around one with three).  The workspace has a guard tile
behind every buffer; the guard rows of ``e``, ``ed`` and ``edge_hids`` are NaN-filled and must still be NaN: rows at or behind ``Pp`` are
computed but never written.

The forward in one-stream and in two-stream mode (``ds_set_two_stream``) must leave the same bits in ``ws.ed``."""
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import dmt as odmt
from tests.golden import cases
from tests.helpers import oracle_edge_maps
from tests.test_block_stages_gpu import GuardedWorkspace, engine_for, same_bits
from tests.test_hip_parity import TOL_KERNEL, assert_close

pytestmark = pytest.mark.gpu

BATCHES = {"pair1": [2], "pairs36": [9], "pairs105": [15], "pairs136": [17], "pairs472": [29, 12], "lonely": [1, 3, 1]}
PAIRS = {"pair1": 1, "pairs36": 36, "pairs105": 105, "pairs136": 136, "pairs472": 472, "lonely": 3}
GUARDED = ("e", "ed", "edge_hids")


def _oracle_ed(sd, blk, pos, e_out, edge_index, edge_t):
    """The edge part of equi_update.input_lin of block ``blk`` (oracle/dmt.py ``_equi_update``: columns 512-639 of ``h_input``, plus the bias):
    ``e_out`` is the block's edge output, the distance features are those of the positions the block started from."""
    name = f"e_block_{blk}"
    row, col = edge_index
    dvec = pos[row] - pos[col]
    distance = odmt._cond_gaussian(sd, name + ".dist_layer", torch.sum(dvec ** 2, 1).unsqueeze(1), edge_t)
    w = sd[name + ".equi_update.input_lin.weight"]
    return F.linear(torch.cat([e_out, distance], dim=1), w[:, 512:640], sd[name + ".equi_update.input_lin.bias"])


@pytest.mark.parametrize("batch", list(BATCHES))
def test_workgroup_tile_edges_against_the_oracle(gpu_device, batch):
    from diffspectra_amd import engine as E
    n_atoms = BATCHES[batch]
    cpu_cfg, sd, eng = engine_for("filler", gpu_device)
    d = gpu_device
    a = cases.forward_inputs("ir", False, n_atoms=n_atoms, salt=3)
    L = E.Layout(a["node_mask"], d)
    Pp = L.Pp
    assert Pp == PAIRS[batch]
    ws = GuardedWorkspace(L, d)
    ctx = oracle.context_embedding(sd, a["context"], cpu_cfg)
    _, _, dbg = oracle.dmt_forward(sd, cpu_cfg, a["xh"], a["node_mask"], a["edge_mask"], a["edge_x"], a["noise_level"], a["cond_x"],
                                   a["cond_edge_x"], context_emb=ctx, return_debug=True)
    fwd, bwd, nd = oracle_edge_maps(L.valid, L.t["node_dense"], L.t["pair_a"], L.t["pair_b"])
    edge_index = dbg["edge_index"]
    N = a["xh"].shape[1]
    edge_t = (odmt.time_embedding(sd, a["noise_level"]) + ctx)[torch.div(edge_index[0], N, rounding_mode="floor")]
    dv = lambda t: t.to(device=d, dtype=torch.float32).contiguous()
    eng.stage_time(L, ws, dv(a["noise_level"]), dv(ctx))
    eng.stage_init(L, ws, dv(a["xh"]), dv(a["edge_x"]), dv(a["cond_x"]), dv(a["cond_edge_x"]))
    torch.cuda.synchronize()
    for k in GUARDED:                                   # after init: k_pair_init's rows of e and edge_hids[:, 0:64] are in place
        ws.full[k][Pp:] = float("nan")
    pos_prev = a["xh"][:, :, 0:3].reshape(-1, 3)
    for blk in (0, 1):
        e_ref = dbg[f"e_{blk}"]
        ed_ref = _oracle_ed(sd, blk, pos_prev, e_ref, edge_index, edge_t)
        ro_ref = odmt._lin(sd, f"edge_{blk}", e_ref)
        eng.stage_block(L, ws, blk, last=False)
        torch.cuda.synchronize()
        assert ws.t["e"].shape == (Pp, 64) and ws.t["ed"].shape == (Pp, 256)
        ro = ws.t["edge_hids"][:, 64 + 16 * blk: 80 + 16 * blk]
        for way, idx in (("a->b", fwd), ("b->a", bwd)):
            assert_close(ws.t["e"], e_ref[idx], TOL_KERNEL, f"{batch} block {blk}: ws.e ({way})")
            assert_close(ws.t["ed"], ed_ref[idx], TOL_KERNEL, f"{batch} block {blk}: ws.ed ({way})")
            assert_close(ro, ro_ref[idx], TOL_KERNEL, f"{batch} block {blk}: edge_hids slice ({way})")
        for k in GUARDED:
            assert bool(torch.isnan(ws.full[k][Pp:]).all()), f"{batch} block {blk}: a row behind Pp of ws.{k} was written"
        pos_prev = dbg[f"pos_{blk}"]


def test_ed_same_bits_in_one_stream_and_two_stream_mode(gpu_device):
    from diffspectra_amd import engine as E
    n_atoms = BATCHES["pairs472"]
    cpu_cfg, sd, eng = engine_for("filler", gpu_device)
    lib, d = E.load_library(), gpu_device
    a = cases.forward_inputs("ir", False, n_atoms=n_atoms, salt=3)
    L = E.Layout(a["node_mask"], d)
    assert L.Pp == PAIRS["pairs472"]
    ctx = oracle.context_embedding(sd, a["context"], cpu_cfg)
    dv = lambda t: t.to(device=d, dtype=torch.float32).contiguous()
    args = [dv(a[k]) for k in ("xh", "edge_x", "noise_level", "cond_x", "cond_edge_x")] + [dv(ctx)]
    got = {}
    prev = lib.ds_set_two_stream(0)
    try:
        for two in (0, 1):
            lib.ds_set_two_stream(two)
            ws = GuardedWorkspace(L, d)
            out = eng.forward(L, ws, *args)
            torch.cuda.synchronize()
            ws.check_guards(f"two_stream = {two}")
            got[two] = {k: ws.t[k].cpu().clone() for k in GUARDED} | {"out_xh": out[0].cpu().clone(), "out_edge": out[1].cpu().clone()}
    finally:
        lib.ds_set_two_stream(prev)
    assert not bool(torch.isnan(got[0]["ed"]).any()) and float(got[0]["ed"].abs().max()) > 0.0
    for k in got[0]:
        assert same_bits(got[0][k], got[1][k]), f"{k} differs between the one-stream and the two-stream forward"
