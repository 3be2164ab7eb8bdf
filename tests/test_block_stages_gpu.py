"""Stage-by-stage fp64 parity of the sampling block kernels (csrc/ds_forward.hip) against tests/block_mirror.py: every buffer a block's
seven kernels hand each other through the workspace, plus init and readout.

TEACHER FORCING.  h, e and pos are snapshotted before each ``ds_stage_block``; afterwards every stage's reference is evaluated from the
KERNEL'S OWN tensors of the stage in front of it (``block_mirror.teacher_forced_block``), so both sides start from the same fp32 values and one
stage's arithmetic separates them.  A failure names the block, the buffer and the element.

TOLERANCES.  None is tuned to the kernels: a matrix product is held per element to the bound of its arithmetic (``block_mirror.fp32_bound`` =
``chain_mirror.product_bound``; ``block_mirror.split_bound``, derived in that module's docstring and pinned by the numpy emulation of
tests/test_block_mirror_cpu.py), everything behind a product to the ``relerr`` figures of ``test_train_chain_kernels.TOL`` (gate / residual 2e-6,
modulated LayerNorm 3e-6, Gaussian features / x' 3e-6, SiLU / tanh / exp epilogues 3e-6) over the rows of a molecule, a stage behind an
unobserved product to both (the carried bound), the softmax weights to 2 max d(logit) + 3e-6 absolute.  Integers (adj, flags), the q|k|v pad
columns, the pad lane of tr and masked output entries are compared exactly (their allowance is 0).

INTERFACE EDGES, in every test: the workspace is the test's own, every buffer with a guard tile of 128 extra rows behind it, filled with a
sentinel - guards must survive every stage call bit for bit and the rows a stage owns must hold no sentinel (an out-of-bounds store of a
partial tile is otherwise swallowed by the allocator's padding); every block is run twice from the same snapshot and must reproduce itself
bit for bit; the same molecules in reversed batch order must give bit-identical rows per molecule; no NaN / Inf in a written row.

Every test prints ``buffer: largest deviation / share of its allowance`` (first green run: profiles/HISTORY.md)."""
import math

import pytest
import torch

import oracle
from tests import block_mirror as bm
from tests.helpers import procedural_state_dict, checkpoint_like

pytestmark = pytest.mark.gpu

GUARD = 128                 # one guard tile: the largest row tile of any block kernel (k_edge_update's 4 x 32 rows)
SENT = -7.5
ISENT = -7575
NODE_BUFS = ("pos", "h", "atom_hids", "qkv", "attn", "u", "ac")
PAIR_BUFS = ("e", "edge_hids", "ye", "dist", "ed", "lg", "tr", "adj")
MOL_BUFS = ("tfeat", "tmid", "temb_silu", "ada")
WRITTEN_BY_BLOCK = ("dist", "ye", "qkv", "lg", "attn", "u", "h", "ac", "e", "ed", "tr", "pos")

_ENGINES, _CTX = {}, {}


def engine_for(weights, device):
    """(cfg, CPU state dict, engine) of the procedural ``ir`` weights, as they are (``filler``) or with ``helpers.checkpoint_like`` statistics."""
    if weights not in _ENGINES:
        from diffspectra_amd import engine as E
        from diffspectra_amd.config import qm9s_config
        _, sd = procedural_state_dict("ir")
        if weights == "checkpoint":
            sd = checkpoint_like(sd)
        _ENGINES[weights] = (qm9s_config("ir", device=device), sd, E.DmtEngine(sd, qm9s_config("ir", device=device), device))
    return _ENGINES[weights]


def context_for(weights, key, sd, cfg, a):
    """cond_lin(SpecFormer(context)) on the CPU, once per case: the SpecFormer kernels are not what these tests are about."""
    if (weights, key) not in _CTX:
        _CTX[(weights, key)] = oracle.context_embedding(sd, a["context"], cfg)
    return _CTX[(weights, key)]


class GuardedWorkspace:
    """``engine.Workspace`` with exact row counts and a sentinel guard tile behind every buffer; ``t``: the owned rows, ``full``: with guards."""

    def __init__(self, L, device):
        from diffspectra_amd import engine as E
        Nn, Pp, B = L.Nn, L.Pp, L.B
        shape = dict(pos=(Nn, 4), h=(Nn, 256), e=(Pp, 64), atom_hids=(Nn, 768), edge_hids=(Pp, 192), tfeat=(B, 24), tmid=(B, 1024),
                     temb_silu=(B, 1024), ada=(B, E.ADA_COLS), qkv=(Nn, 768), ye=(Pp, 64), dist=(Pp, 1), attn=(Nn, 256), u=(Nn, 64), ac=(Nn, 512),
                     ed=(Pp, 256), lg=(Pp, 32), tr=(Pp, 8), adj=(Pp, 1), flags=(64, 1))
        assert list(shape) == E._WS_FIELDS, (list(shape), E._WS_FIELDS)
        self.full, self.t, self.rows = {}, {}, {}
        for k, (r, c) in shape.items():
            if k in ("adj", "flags"):                                     # as the engine sets them: zero; the guard rows hold the integer sentinel
                t = torch.full((r + GUARD, c), ISENT, dtype=torch.int32, device=device)
                t[:r] = 0
            else:
                t = torch.full((r + GUARD, c), SENT, dtype=torch.float32, device=device)
            self.full[k], self.t[k], self.rows[k] = t, t[:r], r
        self.c = E.DsWorkspace(**{k: v.data_ptr() for k, v in self.full.items()})

    def check_guards(self, where):
        for k, t in self.full.items():
            g = t[self.rows[k]:]
            assert bool((g == (ISENT if t.dtype == torch.int32 else SENT)).all()), f"{where}: a store went past the last row of ws.{k}"

    def check_written(self, names, where, cols=None):
        for k in names:
            t = self.t[k] if cols is None else self.t[k][:, cols[0]: cols[1]]
            assert not bool((t == SENT).any()), f"{where}: ws.{k} still holds the sentinel in a row the stage owns"

    def snapshot(self):
        return {k: v.clone() for k, v in self.full.items()}

    def restore(self, snap):
        for k, v in snap.items():
            self.full[k].copy_(v)


def guarded(shape, device):
    t = torch.full((shape[0] + GUARD,) + tuple(shape[1:]), SENT, dtype=torch.float32, device=device)
    return t, t[:shape[0]]


def capture(ws, blk):
    """The buffers of ``block_mirror.BLOCK_BUFFERS`` as a block leaves them (CPU): ``raw`` for bit comparisons, ``obs`` as the mirror reads them."""
    raw = {k: ws.t[k].detach().cpu().clone() for k in WRITTEN_BY_BLOCK}
    raw["atom_hids"] = ws.t["atom_hids"][:, 256 + 64 * blk: 320 + 64 * blk].cpu().clone()
    raw["edge_hids"] = ws.t["edge_hids"][:, 64 + 16 * blk: 80 + 16 * blk].cpu().clone()
    raw["flags"] = ws.t["flags"][:2, 0].cpu().clone()
    obs = dict(raw)
    planes = raw["ye"].view(torch.float16).reshape(-1, 2, 64).double()
    obs["ye"] = planes[:, 0] + planes[:, 1] / 2048.0                          # a = a1 + a2 / 2048: exactly the operand of k_attn_fused
    obs["alpha"] = raw["lg"].reshape(-1, 2, 16)
    obs["pos"] = raw["pos"][:, :3]
    assert bool((raw["pos"][:, 3] == 0).all())
    return raw, obs


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def flip_inputs(a):
    f = lambda t: None if t is None else ([x.flip(0) for x in t] if isinstance(t, (list, tuple)) else t.flip(0))
    return {k: f(v) for k, v in a.items()}


def run(weights, a, n_atoms, ctx, device, check_blocks, tag, n_blocks=8, readout=True):
    """time, init, ``n_blocks`` blocks (each of ``check_blocks`` twice from the same snapshot: determinism) and the readout on a guarded
    workspace.  Returns everything the comparisons need, on the CPU."""
    from diffspectra_amd import engine as E
    cfg, sd, eng = engine_for(weights, device)
    L = E.Layout(a["node_mask"], device)
    tb = bm.tables(n_atoms)
    assert (L.Nn, L.Pp) == (tb["Nn"], tb["Pp"])
    ws = GuardedWorkspace(L, device)
    dv = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()
    eng.stage_time(L, ws, dv(a["noise_level"]), dv(ctx))
    torch.cuda.synchronize()
    ws.check_guards(f"{tag} time")
    ws.check_written(MOL_BUFS, f"{tag} time")
    eng.stage_init(L, ws, dv(a["xh"]), dv(a["edge_x"]), dv(a["cond_x"]), dv(a["cond_edge_x"]))
    torch.cuda.synchronize()
    ws.check_guards(f"{tag} init")
    ws.check_written(("pos", "h", "e"), f"{tag} init")
    ws.check_written(("atom_hids",), f"{tag} init", (0, 256))
    ws.check_written(("edge_hids",), f"{tag} init", (0, 64))
    rec = dict(tb=tb, L=L, ada=ws.t["ada"].cpu().clone(), adj=ws.t["adj"][:, 0].cpu().clone(), flags0=ws.t["flags"][:2, 0].cpu().clone(),
               init={k: ws.t[k].cpu().clone() for k in ("pos", "h", "e")}, blocks={}, snaps={})
    assert same_bits(rec["init"]["h"], ws.t["atom_hids"][:, :256].cpu()) and same_bits(rec["init"]["e"], ws.t["edge_hids"][:, :64].cpu())
    for blk in range(n_blocks):
        last = blk == 7
        if blk not in check_blocks:
            eng.stage_block(L, ws, blk, last=last)
            continue
        snap = ws.snapshot()
        rec["snaps"][blk] = {k: snap[k][:ws.rows[k]].cpu().clone() for k in ("h", "e", "pos")}
        eng.stage_block(L, ws, blk, last=last)
        torch.cuda.synchronize()
        where = f"{tag} block {blk}"
        ws.check_guards(where)
        ws.check_written(WRITTEN_BY_BLOCK, where)
        ws.check_written(("atom_hids",), where, (0, 320 + 64 * blk))
        ws.check_written(("edge_hids",), where, (0, 80 + 16 * blk))
        raw, obs = capture(ws, blk)
        ws.restore(snap)
        eng.stage_block(L, ws, blk, last=last)
        torch.cuda.synchronize()
        raw2, _ = capture(ws, blk)
        for k in raw:
            assert same_bits(raw[k], raw2[k]), f"{where}: ws.{k} differs between two runs from the same snapshot"
        if last:                                                              # `last` only arms the NaN flag: the positions are the same bits
            ws.restore(snap)
            eng.stage_block(L, ws, blk, last=False)
            torch.cuda.synchronize()
            assert same_bits(capture(ws, blk)[0]["pos"], raw["pos"]), f"{where}: positions depend on `last`"
            ws.restore(snap)
            eng.stage_block(L, ws, blk, last=True)
            torch.cuda.synchronize()
        rec["blocks"][blk] = (raw, obs)
    if readout:
        B, N = L.B, L.N
        xf, out_xh = guarded((B, N, 9), device)
        ef, out_edge = guarded((B, N, N, 2), device)
        pre = {k: ws.t[k].cpu().clone() for k in ("atom_hids", "edge_hids", "pos", "flags")}
        eng.stage_readout(L, ws, out_xh, out_edge)
        torch.cuda.synchronize()
        ws.check_guards(f"{tag} readout")
        assert bool((xf[B:] == SENT).all()) and bool((ef[B:] == SENT).all()), f"{tag} readout: a store went past the end of an output"
        assert not bool((out_xh == SENT).any()) and not bool((out_edge == SENT).any())
        rec["readout"] = (pre, out_xh.cpu().clone(), out_edge.cpu().clone())
    return rec


def report(tag, rows):
    worst = 0.0
    for name, dev, share, idx in rows:
        print(f"[block stages] {tag:44s} {name:10s} max |got - ref| {dev:.3e}   share of allowance {share:.3f}")
        worst = max(worst, share)
    bad = [(n, f"{s:.3g} x its allowance at {i}") for n, _, s, i in rows if not s <= 1.0]
    assert not bad, f"{tag}: {bad}"
    return worst


def check(weights, a, rec, device, tag, names=bm.BLOCK_BUFFERS):
    """The mirror against every captured stage of ``rec``."""
    cfg, sd, _ = engine_for(weights, device)
    tb, ada, adj = rec["tb"], rec["ada"], rec["adj"]
    refs, ref_adj, ref_flag = bm.init(sd, cfg, tb, a["xh"], a["edge_x"], a["cond_x"], a["cond_edge_x"], ada)
    assert torch.equal(adj, ref_adj), f"{tag}: adjacency bits"
    assert rec["flags0"].tolist() == [ref_flag, 0], f"{tag}: flags {rec['flags0'].tolist()}"
    got = dict(rec["init"], pos=rec["init"]["pos"][:, :3])
    report(f"{tag} init", bm.shares(refs, got))
    for blk, (raw, obs) in rec["blocks"].items():
        s = rec["snaps"][blk]
        refs = bm.teacher_forced_block(sd, blk, tb, s["h"], s["e"], s["pos"], adj, ada, obs)
        report(f"{tag} block {blk}", bm.shares(refs, obs, names))
        assert raw["flags"].tolist() == [ref_flag, 0], f"{tag} block {blk}: flags {raw['flags'].tolist()}"
    if "readout" in rec:
        pre, out_xh, out_edge = rec["readout"]
        N = a["xh"].shape[1]
        refs = bm.readout(sd, tb, N, pre["atom_hids"], pre["edge_hids"], pre["pos"], int(pre["flags"][1, 0]))
        report(f"{tag} readout", bm.shares(refs, dict(out_xh=out_xh, out_edge=out_edge)))
        assert torch.equal(out_edge, out_edge.transpose(1, 2))
        assert float((out_xh * (1 - a["node_mask"])).abs().max()) == 0.0
        assert float((out_edge * (1 - a["edge_mask"].reshape(out_edge.shape[:3] + (1,)))).abs().max()) == 0.0


def check_batch_independence(rec, rev, tag):
    """Molecule m of the batch and molecule B - 1 - m of the reversed batch: bit-identical rows in every buffer."""
    tb, tr_ = rec["tb"], rev["tb"]
    B = tb["B"]
    for m in range(B):
        r = B - 1 - m
        ns, nr = slice(int(tb["node_off"][m]), int(tb["node_off"][m + 1])), slice(int(tr_["node_off"][r]), int(tr_["node_off"][r + 1]))
        ps, pr = slice(int(tb["pair_off"][m]), int(tb["pair_off"][m + 1])), slice(int(tr_["pair_off"][r]), int(tr_["pair_off"][r + 1]))
        assert same_bits(rec["ada"][m], rev["ada"][r]), f"{tag}: adaLN row of molecule {m}"
        assert torch.equal(rec["adj"][ps], rev["adj"][pr])
        for k, v in rec["init"].items():
            sl = (ns, nr) if k in NODE_BUFS else (ps, pr)
            assert same_bits(v[sl[0]], rev["init"][k][sl[1]]), f"{tag} init: ws.{k} of molecule {m} depends on the batch order"
        for blk, (raw, _) in rec["blocks"].items():
            for k, v in raw.items():
                if k == "flags":
                    continue
                sl = (ns, nr) if k in NODE_BUFS else (ps, pr)
                assert same_bits(v[sl[0]], rev["blocks"][blk][0][k][sl[1]]), f"{tag} block {blk}: ws.{k} of molecule {m} depends on the batch order"
        if "readout" in rec:
            assert same_bits(rec["readout"][1][m], rev["readout"][1][r]) and same_bits(rec["readout"][2][m], rev["readout"][2][r]), \
                f"{tag} readout: molecule {m} depends on the batch order"


def stage_case(device, layout, first, weights, check_blocks):
    n_atoms = bm.LAYOUTS[layout]
    a = bm.stage_inputs(layout, first)
    tb = bm.tables(n_atoms)
    assert (tb["Nn"], tb["Pp"]) == bm.COUNTS[layout]
    cfg, sd, _ = engine_for(weights, device)
    ctx = context_for(weights, layout, sd, cfg, a)
    tag = f"{layout} {'first' if first else 'general'} {weights}"
    rec = run(weights, a, n_atoms, ctx, device, check_blocks, tag)
    check(weights, a, rec, device, tag)
    if not first and layout in bm.CLEARED:       # not left to chance: a target with a uniform extra-head softmax, targets with mixed bits of either kind
        assert bm.adjacency_patterns(n_atoms, rec["adj"]) == (True, True, True), f"{tag}: adjacency patterns of the inputs"
    rev = run(weights, flip_inputs(a), n_atoms[::-1], ctx.flip(0), device, check_blocks, tag + " reversed")
    check_batch_independence(rec, rev, tag)
    return rec


@pytest.mark.parametrize("weights", ["filler", "checkpoint"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "general"])
def test_ragged_every_block(gpu_device, first, weights):
    """[3, 1, 9, 2, 12, 1, 4, 15]: two pairless molecules, 1 / 2 / 3 / 4 attention chunks (P = 3 / 36 / 66 / 105), odd and even n, node tiles
    32 | 15, pair tiles cut across molecules at 32, 64 and 128.  Init, all 8 blocks (`last` on block 7) and the readout."""
    stage_case(gpu_device, "ragged", first, weights, range(8))


@pytest.mark.parametrize("weights", ["filler", "checkpoint"])
@pytest.mark.parametrize("layout", ["big", "single", "one_pair"])
def test_layout_edges_blocks_0_and_7(gpu_device, layout, weights):
    """big = [29, 28, 29]: 13 chunks with a 22-row tail, the 15-logits-per-lane softmax at 28 sources, nine full 128-row edge tiles + 38 rows,
    64-row tiles 64 | 22.  single = [1]: no pair row, every pair launch skipped, attn exactly zero.  one_pair = [2]."""
    rec = stage_case(gpu_device, layout, False, weights, (0, 7))
    if layout == "single":
        for blk, (raw, _) in rec["blocks"].items():
            assert float(raw["attn"].abs().max()) == 0.0, f"block {blk}: attention output of a single atom"


@pytest.mark.parametrize("weights", ["filler", "checkpoint"])
def test_persistent_equi_pairs_more_tiles_than_compute_units(gpu_device, weights):
    """[29] x k with ceil(Pp / 32) > compute units: k_equi_pairs workgroups own more than one tile.  Block 0: tr and pos against the mirror, and
    molecule 0's tr bit-identical to the same molecule alone."""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    k = next(k for k in range(1, 4096) if math.ceil(406 * k / 32) > cus)
    n_atoms = [29] * k
    a = bm.stage_inputs("persistent", False, n_atoms=n_atoms)
    tag = f"persistent x{k} {weights}"
    rec = run(weights, a, n_atoms, None, gpu_device, (0,), tag, n_blocks=1, readout=False)      # NULL context: a zero context embedding
    assert math.ceil(rec["tb"]["Pp"] / 32) > cus
    check(weights, a, rec, gpu_device, tag, names=("tr", "pos"))
    one = {key: (None if v is None else ([x[:1] for x in v] if isinstance(v, (list, tuple)) else v[:1])) for key, v in a.items()}
    alone = run(weights, one, [29], None, gpu_device, (0,), tag + " alone", n_blocks=1, readout=False)
    assert same_bits(rec["blocks"][0][0]["tr"][:406], alone["blocks"][0][0]["tr"]), "tr of molecule 0 depends on the batch"
