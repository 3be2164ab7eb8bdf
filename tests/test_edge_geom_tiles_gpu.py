"""k_pair_init and k_edge_geom at the edges of their 64-row pair tiles, against the CPU oracle.

k_pair_init stages its 68-wide row in 16-byte pieces (a tile row per 16-lane row, four features per lane); k_edge_geom keeps its
``edge_emb`` product in the LDS of its input tile (four workgroups per CU).  What they leave - ``ws.e`` / ``edge_hids[:, 0:64]`` after
``ds_stage_init``; the modulated squared distance ``ws.dist`` and ``ws.ye``, the ``norm1_edge``-modulated ``edge_emb`` output in the split-fp16
layout (``a = a1 + a2 / 2048``), after block 0 and block 1 - is compared with the same lines of ``oracle.dmt`` (``dmt_forward``'s initial
``edge_emb``; ``_mix_block``: ``_cond_gaussian``, ``edge_emb``, ``_ln``, ``_modulate``), evaluated on the oracle's own state ahead of that stage.  Tolerance: ``TOL_KERNEL`` with the relative term of
tests/test_hip_parity.py, which that file applies to the split-fp16 ``temb_silu`` and to every per-stage buffer; not one of this file's own.

Batches: one molecule of 2 atoms (``Pp`` = 1: a tile of one row); ``[12]`` (``Pp`` = 66: one row pair past a full tile); ``[29, 12]`` (``Pp`` = 472: the
tile boundary at row 448 falls inside the second molecule's rows, and tile 6 holds adaLN rows of both molecules); ``[1, 3, 1]`` (molecules
without pairs around one with three).  The workspace has a guard tile behind every buffer; the guard rows of ``ye`` and ``dist`` are
NaN-filled, and must still be NaN: rows behind ``Pp`` in the last tile are computed (as zeros) but never written."""
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import dmt as odmt
from tests.golden import cases
from tests.helpers import oracle_edge_maps
from tests.test_block_stages_gpu import GuardedWorkspace, engine_for
from tests.test_hip_parity import TOL_KERNEL, assert_close

pytestmark = pytest.mark.gpu

BATCHES = {"pair1": [2], "pairs66": [12], "pairs472": [29, 12], "lonely": [1, 3, 1]}
PAIRS = {"pair1": 1, "pairs66": 66, "pairs472": 472, "lonely": 3}


def _oracle_edge_stage(sd, blk, pos, edge_attr, edge_index, edge_t):
    """(modulated squared distance [E], norm1_edge-modulated edge features [E, 64]) of block ``blk``: oracle/dmt.py ``_mix_block``, first lines."""
    name = f"e_block_{blk}"
    row, col = edge_index
    dvec = pos[row] - pos[col]
    distance = odmt._cond_gaussian(sd, name + ".dist_layer", torch.sum(dvec ** 2, 1).unsqueeze(1), edge_t)
    e = odmt._lin(sd, name + ".edge_emb", torch.cat([distance, edge_attr], dim=-1))
    e_sh_a, e_sc_a = odmt._lin(sd, name + ".edge_time_mlp.1", F.silu(edge_t)).chunk(6, dim=1)[:2]
    return distance[:, 0], odmt._modulate(odmt._ln(e), e_sh_a, e_sc_a)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_tile_edges_against_the_oracle(gpu_device, batch):
    from diffspectra_amd import engine as E
    n_atoms = BATCHES[batch]
    cpu_cfg, sd, eng = engine_for("filler", gpu_device)
    d = gpu_device
    a = cases.forward_inputs("ir", False, n_atoms=n_atoms, salt=3)
    L = E.Layout(a["node_mask"], d)
    Pp = L.Pp
    assert Pp == PAIRS[batch]
    ws = GuardedWorkspace(L, d)
    for k in ("ye", "dist"):
        ws.full[k][Pp:] = float("nan")
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
    # the state ahead of block 0, by the oracle's lines (dmt_forward: cond distances -> dist_layer -> edge_emb)
    dense = a["edge_mask"].reshape(len(n_atoms), N, N).nonzero(as_tuple=True)
    cond_pos = a["cond_x"][:, :, 0:3].reshape(-1, 3)
    cdist = torch.sum((cond_pos[edge_index[0]] - cond_pos[edge_index[1]]) ** 2, 1).unsqueeze(1)
    assert float(cdist.sum()) != 0.0
    e_prev = odmt._lin(sd, "edge_emb", torch.cat([a["edge_x"][dense], a["cond_edge_x"][dense], odmt._cond_gaussian(sd, "dist_layer", cdist, edge_t)], dim=-1))
    pos_prev = a["xh"][:, :, 0:3].reshape(-1, 3)
    for way, idx in (("a->b", fwd), ("b->a", bwd)):
        assert_close(ws.t["e"], e_prev[idx], TOL_KERNEL, f"{batch}: ws.e after init ({way})")
        assert_close(ws.t["edge_hids"][:, :64], e_prev[idx], TOL_KERNEL, f"{batch}: edge_hids[:, 0:64] after init ({way})")
    for blk in (0, 1):
        dist_ref, ye_ref = _oracle_edge_stage(sd, blk, pos_prev, e_prev, edge_index, edge_t)
        eng.stage_block(L, ws, blk, last=False)
        torch.cuda.synchronize()
        planes = ws.t["ye"].cpu().view(torch.float16).reshape(-1, 2, 64).float()
        ye = planes[:, 0] + planes[:, 1] / 2048.0
        assert ye.shape == (Pp, 64) and ws.t["dist"].shape[0] == Pp
        for way, idx in (("a->b", fwd), ("b->a", bwd)):
            assert_close(ws.t["dist"][:, 0], dist_ref[idx], TOL_KERNEL, f"{batch} block {blk}: ws.dist ({way})")
            assert_close(ye, ye_ref[idx], TOL_KERNEL, f"{batch} block {blk}: ws.ye ({way})")
        for k in ("ye", "dist"):
            assert bool(torch.isnan(ws.full[k][Pp:]).all()), f"{batch} block {blk}: a row behind Pp of ws.{k} was written"
        e_prev, pos_prev = dbg[f"e_{blk}"], dbg[f"pos_{blk}"]
