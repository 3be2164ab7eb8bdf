"""The two row-tile forms of the node-row block kernels (``ds_set_node_tile``): 32 rows (k_node_update, the column-split k_node_qkv) and
64 rows per 512-thread workgroup (k_node_update64, k_node_qkv_wide).  A row's value must not depend on its tile, so on every layout both
forms pass the fp64 mirror of tests/test_block_stages_gpu.py within that file's derived bounds (no tolerance of this file's own) AND agree
bit for bit, in the reversed batch order too; the guarded workspace of ``run`` catches a store past a partial tile.

LAYOUTS reach the edges of the 64-row form: a tile of 64 one-atom molecules (64 gate rows: 16 staged ahead of the FF, 48 behind it) followed by a
6-row tile; 32 molecules in a tile; 63 / 64 / 65 rows (a tile short by one row, full, a second tile of one row); 17 rows (the second 32-row
tile of the workgroup is all padding); 129 rows (two full tiles and one row).  Block 0 only, NULL context (a zero context embedding).

The forward test runs the 64-row forms through ``ds_forward`` in both stream modes - the two-stream order uses k_node_update64 without
its node2edge part behind k_node_n2e - against the 32-row single-stream forward, bit for bit."""
import pytest
import torch

from tests import block_mirror as bm
from tests.test_block_stages_gpu import check, check_batch_independence, engine_for, flip_inputs, run, same_bits

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "ones70": [1] * 70,
    "twos33": [2] * 33,
    "rows63": [29, 29, 5],
    "rows64": [29, 29, 6],
    "rows65": [29, 29, 7],
    "rows17": [17],
    "rows129": [29] * 4 + [13],
}
NODE_ROW_BUFFERS = ("qkv", "u", "h", "ac", "atom_hids")


def _library():
    from diffspectra_amd import engine as E
    return E.load_library()


def test_setter_returns_the_previous_value(gpu_device):
    lib = _library()
    prev = lib.ds_set_node_tile(32)
    try:
        assert lib.ds_set_node_tile(64) == 32
        assert lib.ds_set_node_tile(-1) == 64
        assert lib.ds_set_node_tile(32) == -1
    finally:
        lib.ds_set_node_tile(prev)


@pytest.mark.parametrize("weights", ["filler", "checkpoint"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_both_forms_against_the_mirror_and_bit_identical(gpu_device, layout, weights):
    n_atoms = LAYOUTS[layout]
    a = bm.stage_inputs(layout, False, n_atoms=n_atoms)
    lib = _library()
    prev = lib.ds_set_node_tile(32)
    try:
        recs = {}
        for rows, before in ((32, 32), (64, 32)):
            assert lib.ds_set_node_tile(rows) == before
            tag = f"node tiles {layout} {weights} {rows} rows"
            rec = run(weights, a, n_atoms, None, gpu_device, (0,), tag, n_blocks=1, readout=False)      # guards checked inside
            assert rec["tb"]["Nn"] == sum(n_atoms)
            check(weights, a, rec, gpu_device, tag, names=NODE_ROW_BUFFERS)
            rev = run(weights, flip_inputs(a), n_atoms[::-1], None, gpu_device, (0,), tag + " reversed", n_blocks=1, readout=False)
            check_batch_independence(rec, rev, tag)
            recs[rows] = rec["blocks"][0][0]
        for k in NODE_ROW_BUFFERS:
            assert same_bits(recs[32][k], recs[64][k]), f"{layout} {weights}: ws.{k} differs between the 32-row and the 64-row form"
    finally:
        lib.ds_set_node_tile(prev)


def test_forward_64_row_forms_equal_32_row_forms_in_both_stream_modes(gpu_device):
    from diffspectra_amd import filler
    _, _, eng = engine_for("filler", gpu_device)
    lib, d = _library(), gpu_device
    n_atoms = [1] * 40 + [29, 2, 17, 1, 29, 3] + [2] * 20 + [29] * 3
    x, ex, node_mask, edge_mask = filler.synthetic_state(n_atoms, "nt.x")
    cx, cex, _, _ = filler.synthetic_state(n_atoms, "nt.c")
    B = len(n_atoms)
    nl = filler.uniform("nt.nl", (B,), -6, 6)
    ctx_emb = filler.normal("nt.ctx", (B, 1024)) * 0.5
    L, ws = eng.layout_for(node_mask, edge_mask, validate=True)
    xd, exd, nld, cxd, cexd, ctxd = (t.to(d) for t in (x, ex, nl, cx, cex, ctx_emb))
    prev_tile, prev_two = lib.ds_set_node_tile(32), lib.ds_set_two_stream(0)
    try:
        o, oe = eng.forward(L, ws, xd, exd, nld, cxd, cexd, ctxd)
        ref = (o.clone(), oe.clone())
        lib.ds_set_node_tile(64)
        for two in (0, 1):
            lib.ds_set_two_stream(two)
            o, oe = eng.forward(L, ws, xd, exd, nld, cxd, cexd, ctxd)
            assert torch.equal(o, ref[0]) and torch.equal(oe, ref[1]), f"64-row forms, two_stream = {two}"
    finally:
        lib.ds_set_node_tile(prev_tile)
        lib.ds_set_two_stream(prev_two)
