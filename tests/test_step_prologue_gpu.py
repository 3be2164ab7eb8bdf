"""The uniform step prologue (include/diffspectra_step.h): ``ds_stage_time_uniform`` / ``ds_forward_uniform`` evaluate the time MLP on
``noise_level[0]`` alone and must leave exactly the bits the per-molecule entry points leave on a noise-level vector filled with that value.

Batch sizes: 1; 3; 65 (a second 64-row GEMM tile of one row); 513 - one above the threshold (512 rows) at which ``Linear(1024 -> 1024)`` of
the per-molecule prologue moves from the 64-row to the 128-row GEMM kernel, so the single row has to follow the batch size, not its own
row count.  Each with and without a context embedding.  The forward runs a 3-molecule batch in both stream modes.

The CPU test pins the C-ABI surface of the header the way tests/test_node_tiles_cpu.py pins ``diffspectra_tiles.h``."""
import ctypes as C

import pytest
import torch


def _library():
    import __graft_entry__ as g
    from diffspectra_amd import engine as E
    g.build()
    return E.load_library()


def test_header_declares_and_library_exports_the_uniform_entry_points():
    from diffspectra_amd import abi
    lib = _library()
    assert list(abi.STEP.prototypes) == abi.STEP.exports("ds_") == ["ds_stage_time_uniform", "ds_forward_uniform"]
    assert not abi.STEP.structs and not abi.STEP.enums
    for name, twin in (("ds_stage_time_uniform", "ds_stage_time"), ("ds_forward_uniform", "ds_forward")):
        assert name not in abi.SAMPLING.prototypes                                    # declared once
        mine, theirs = abi.STEP.prototypes[name], abi.SAMPLING.prototypes[twin]
        assert (mine.ret, mine.params) == (theirs.ret, theirs.params)                 # a drop-in for the per-molecule entry point
        fn = getattr(lib, name)                                                       # exported, and bound from the header
        assert fn.restype is C.c_int and list(fn.argtypes) == mine.argtypes
    for other in (abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.SCAFFOLD, abi.SMILES, abi.TILES):
        assert not any(n.endswith("_uniform") for n in other.prototypes)


def _sizes(B):
    return [(1, 3, 2, 5)[i % 4] for i in range(B)]


@pytest.mark.gpu
@pytest.mark.parametrize("with_ctx", [False, True])
@pytest.mark.parametrize("B", [1, 3, 65, 513])
def test_stage_time_uniform_leaves_the_bits_of_stage_time(gpu_device, B, with_ctx):
    from diffspectra_amd import engine as E, filler
    from tests.test_block_stages_gpu import GuardedWorkspace, engine_for, same_bits
    _, _, eng = engine_for("filler", gpu_device)
    d = gpu_device
    node_mask, _ = filler.masks_from_n_atoms(_sizes(B))
    L = E.Layout(node_mask, d)
    assert L.B == B
    level = float(filler.uniform("sp.nl", (1,), -6.0, 6.0, salt=B)[0])
    ctx = (filler.normal("sp.ctx", (B, 1024), salt=B) * 0.5).to(d) if with_ctx else None
    filled = torch.full((B,), level, device=d)
    first_only = torch.full((B,), float("nan"), device=d)          # the uniform entry may read element 0 and nothing else
    first_only[0] = level
    got = {}
    for name, call, nl in (("rows", eng.stage_time, filled), ("uniform", eng.stage_time_uniform, first_only)):
        ws = GuardedWorkspace(L, d)
        call(L, ws, nl, ctx)
        torch.cuda.synchronize()
        ws.check_guards(f"B = {B} {name}")
        ws.check_written(("temb_silu", "ada"), f"B = {B} {name}")
        got[name] = {k: ws.t[k].cpu().clone() for k in ("temb_silu", "ada")}
    for k in ("temb_silu", "ada"):
        assert not bool(torch.isnan(got["rows"][k]).any())
        assert same_bits(got["uniform"][k], got["rows"][k]), f"B = {B}, ctx = {with_ctx}: ws.{k} differs from the per-molecule prologue"


@pytest.mark.gpu
def test_forward_uniform_equals_forward_in_both_stream_modes(gpu_device):
    from diffspectra_amd import filler
    from tests.test_block_stages_gpu import engine_for, same_bits
    _, _, eng = engine_for("filler", gpu_device)
    lib, d = _library(), gpu_device
    n_atoms = [9, 2, 17]
    x, ex, node_mask, edge_mask = filler.synthetic_state(n_atoms, "sp.x")
    cx, cex, _, _ = filler.synthetic_state(n_atoms, "sp.c")
    nl = torch.full((3,), float(filler.uniform("sp.fnl", (1,), -6.0, 6.0)[0]))
    ctx_emb = filler.normal("sp.fctx", (3, 1024)) * 0.5
    L, ws = eng.layout_for(node_mask, edge_mask, validate=True)
    xd, exd, nld, cxd, cexd, ctxd = (t.to(d) for t in (x, ex, nl, cx, cex, ctx_emb))
    prev = lib.ds_set_two_stream(0)
    try:
        for two in (0, 1):
            lib.ds_set_two_stream(two)
            o, oe = eng.forward(L, ws, xd, exd, nld, cxd, cexd, ctxd)
            ref = (o.clone(), oe.clone())
            o, oe = eng.forward(L, ws, xd, exd, nld, cxd, cexd, ctxd, uniform_noise_level=True)
            assert not bool(torch.isnan(ref[0]).any()) and float(ref[0].abs().max()) > 0.0
            assert same_bits(o, ref[0]) and same_bits(oe, ref[1]), f"two_stream = {two}"
    finally:
        lib.ds_set_two_stream(prev)
