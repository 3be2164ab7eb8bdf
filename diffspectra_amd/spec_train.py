"""SpecFormer conditioning encoder in TRAINING mode on the HIP training library: forward tape + hand-written backward.

Mirror of reference ``models/specformer.py:77-120`` (patching, ``TSTiEncoder`` ``:167-200``, three post-norm ``TSTEncoderLayer`` s
``:279-309`` with residual attention scores ``:385-425`` and BatchNorm1d over d_model in training mode ``:247,260``, ``Flatten_Head``
``:467-469``, output LayerNorm ``:119``) followed by ``cond_lin`` (``models/dmt.py:350``).  BatchNorm uses batch statistics and
updates its running statistics in place (momentum 0.1, unbiased variance), as ``nn.BatchNorm1d`` does.  All dropouts of the
encoder are 0 in the reference's constructor defaults.  No PyTorch arithmetic: GEMMs, BatchNorm, attention, GELU and LayerNorm are
``dst_*`` kernels; PyTorch slices, tiles and concatenates buffers.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import engine as E
from .abi import ptr
from .config import SPECTRUM_LENGTHS, used_spectra
from .train_engine import ADDREF, GELU, Ops, mv

D_MODEL, N_HEADS, D_K, D_FF, N_LAYERS = 128, 16, 8, 256, 3


class SpecTrainGraph:
    def __init__(self, params: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor], config, ops: Ops):
        """``params``: reference-named trainable tensors (``cond_encoder.*``, ``cond_lin.*``); ``buffers``: the BatchNorm running
        statistics (updated in place by ``forward``)."""
        self.cfg, self.ops = config, ops
        self.p, self.buf, self.gbuf = params, buffers, None      # bind()
        self.t = None                                             # the tape of the last forward(save=True), consumed by backward
        self._bn_last = []                                        # (name, batch statistics) of the BatchNorms of the last forward
        self.lib, self.dev = ops.lib, ops.dev
        self.version = config.data.spectra_version
        self.used = used_spectra(self.version)
        pl, stv = config.model.patch_len, config.model.stride
        self.patch = [(pl[i], stv[i], int((SPECTRUM_LENGTHS[i] - pl[i]) / stv[i] + 1)) for i in self.used]
        self.L = sum(pn for _, _, pn in self.patch)
        self.pos_names = (["W_pos_uv", "W_pos_ir", "W_pos_raman"] if self.version == "allspectra" else ["W_pos"])
        self.flash = None      # None: the score-free flash attention in bf16 mode, the materialised fp32 kernels otherwise; True / False force one

    def bind(self, params: Dict[str, torch.Tensor], gbuf: Optional[Dict[str, torch.Tensor]] = None, buffers: Optional[Dict[str, torch.Tensor]] = None):
        """This call's parameter storage, the views of the gradient stage its backward writes into (None: fresh tensors) and - if given - the
        BatchNorm buffers.  A forward keeps its binding in its tape and ``backward`` returns to it (see ``DmtTrainGraph.bind``)."""
        self.p, self.gbuf, self.t = params, gbuf, None
        if buffers is not None:
            self.buf = buffers

    def f(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def _bn_fwd(self, x, name, y, stats):
        p, b = self.p, self.buf
        o = self.ops
        R, Cc = x.shape
        E._check(self.lib.dst_bn_fwd(ptr(x), R, Cc, ptr(p[name + ".weight"]), ptr(p[name + ".bias"]), 1e-5,
                                     ptr(y), ptr(stats), ptr(b[name + ".running_mean"]), ptr(b[name + ".running_var"]), ptr(o.scratch),
                                     o.scratch.numel(), self.ops._s()), "dst_bn_fwd")
        b[name + ".num_batches_tracked"] += 1
        self._bn_last.append((name, stats))

    def running_stats_again(self):
        """The buffer updates of one more training-mode forward over the batch of the last ``forward`` (same batch statistics, so nothing
        else of that pass would differ): the reference's self-conditioning step evaluates the encoder twice on one input."""
        b = self.buf
        for name, stats in self._bn_last:
            E._check(self.lib.dst_bn_running_again(ptr(stats), stats.shape[1], ptr(b[name + ".running_mean"]),
                                                   ptr(b[name + ".running_var"]), self.ops._s()), "dst_bn_running_again")
            b[name + ".num_batches_tracked"] += 1

    def _bn_bwd(self, dy, x, stats, name, dx, g):
        o = self.ops
        R, Cc = x.shape
        gb = self.gbuf
        g[name + ".weight"], g[name + ".bias"] = (gb[name + ".weight"], gb[name + ".bias"]) if gb is not None else (self.f(Cc), self.f(Cc))
        E._check(self.lib.dst_bn_bwd(ptr(dy), ptr(x), ptr(stats), R, Cc, ptr(self.p[name + ".weight"]), ptr(dx),
                                     ptr(g[name + ".weight"]), ptr(g[name + ".bias"]), ptr(o.scratch), o.scratch.numel(), self.ops._s()),
                 "dst_bn_bwd")

    # ------------------------------------------------------------------ forward
    def forward(self, context, save: bool = True) -> torch.Tensor:
        """``context``: list [uv, ir, raman] of [B,1,L] (allspectra) or one [B,1,L] tensor -> ctx_emb [B,1024] (dmt.py:348-350)."""
        o, p = self.ops, self.p
        pre = "cond_encoder."
        specs = list(context) if self.version == "allspectra" else [context]
        B = specs[0].shape[0]
        L = self.L
        t: Dict[str, object] = dict(B=B, bound=(self.p, self.gbuf, self.buf))
        self._bn_last = []
        toks, Xs = [], []
        for slot, ((pl, stv, pn), spec) in enumerate(zip(self.patch, specs)):
            X = spec.reshape(B, -1).to(torch.float32).unfold(-1, pl, stv).contiguous().reshape(B * pn, pl)       # specformer.py:105
            z = p[pre + "backbone." + self.pos_names[slot]].unsqueeze(0).expand(B, pn, D_MODEL).contiguous().reshape(B * pn, D_MODEL)
            o.gemm(mv(X), mv(p[pre + f"backbone.W_P.{slot}.weight"]), mv(z), False, True, bias=p[pre + f"backbone.W_P.{slot}.bias"], acc=True)
            Xs.append(X)
            toks.append(z.reshape(B, pn, D_MODEL))
        Z = torch.cat(toks, dim=1).contiguous().reshape(B * L, D_MODEL)                                              # :194
        t["Xs"] = Xs
        layers = []
        prev = None
        scale = float(D_K ** -0.5)
        flash = self.ops.bf16 if self.flash is None else bool(self.flash)
        qkvs = []
        for l in range(N_LAYERS):
            base = pre + f"backbone.encoder.layers.{l}."
            qkv = self.f(B * L, 3 * D_MODEL)
            # W_Q | W_K | W_V read the same tokens: one product from a per-call concatenation of the three weights
            Wc = torch.cat([p[base + f"self_attn.{nm}.weight"] for nm in ("W_Q", "W_K", "W_V")], dim=0)
            bc = torch.cat([p[base + f"self_attn.{nm}.bias"] for nm in ("W_Q", "W_K", "W_V")], dim=0)
            o.lin_fwd(mv(Z), mv(Wc), bc, mv(qkv))
            ast, ao = self.f(B, N_HEADS, L, 2), self.f(B * L, D_MODEL)
            qkvs.append(qkv)
            if flash:                                                  # bf16 mode: scores recomputed from the q | k of layers 0 .. l, never stored
                qp = [ptr(q_) for q_ in qkvs] + [None] * (3 - len(qkvs))
                E._check(self.lib.dst_spec_attn_flash_fwd(qp[0], qp[1], qp[2], l + 1, ptr(ast), ptr(ao), B, L,
                                                          N_HEADS, D_K, scale, self.ops._s()), "dst_spec_attn_flash_fwd")
                scores = None
            else:
                Lp = (L + 31) // 32 * 32                               # padded row stride of the [L, L] score matrices
                scores = self.f(B, N_HEADS, L, Lp)
                E._check(self.lib.dst_spec_attn_fwd(ptr(qkv), ptr(prev), ptr(scores), ptr(ast), ptr(ao), B, L,
                                                    N_HEADS, D_K, scale, self.ops._s()), "dst_spec_attn_fwd")
            r1 = self.f(B * L, D_MODEL)                               # Z + to_out(attention): the residual is added in the product's epilogue
            o.gemm(mv(ao), mv(p[base + "self_attn.to_out.0.weight"]), mv(r1), False, True, bias=p[base + "self_attn.to_out.0.bias"], dact=ADDREF, ref=mv(Z))
            z1, st1 = self.f(B * L, D_MODEL), self.f(3, D_MODEL)
            self._bn_fwd(r1, base + "norm_attn.1", z1, st1)
            a = self.f(B * L, D_FF)
            ga = self.f(B * L, D_FF)
            o.lin_fwd(mv(z1), mv(p[base + "ff.0.weight"]), p[base + "ff.0.bias"], mv(a), act=GELU, out2=mv(ga))
            r2 = self.f(B * L, D_MODEL)
            o.gemm(mv(ga), mv(p[base + "ff.3.weight"]), mv(r2), False, True, bias=p[base + "ff.3.bias"], dact=ADDREF, ref=mv(z1))
            z2, st2 = self.f(B * L, D_MODEL), self.f(3, D_MODEL)
            self._bn_fwd(r2, base + "norm_ffn.1", z2, st2)
            if save:
                layers.append(dict(Zin=Z, qkv=qkv, Wqkv=Wc, scores=scores, ast=ast, ao=ao, r1=r1, st1=st1, z1=z1, a=a, ga=ga, r2=r2, st2=st2, has_prev=prev is not None))
            prev = scores
            Z = z2
        flat = Z.reshape(B, L * D_MODEL)
        zh = self.f(B, 256)
        o.lin_fwd(mv(flat), mv(p[pre + "head.linear.weight"]), p[pre + "head.linear.bias"], mv(zh))
        zs, st_ln = self.f(B, 256), self.f(B, 2)
        E._check(self.lib.dst_ln_affine_fwd(ptr(zh), B, 256, ptr(p[pre + "out_norm.weight"]), ptr(p[pre + "out_norm.bias"]),
                                            1e-5, ptr(zs), ptr(st_ln), self.ops._s()), "dst_ln_affine_fwd")
        ctx = self.f(B, 1024)
        o.lin_fwd(mv(zs), mv(p["cond_lin.weight"]), p["cond_lin.bias"], mv(ctx))
        if save:
            t.update(layers=layers, flat=flat, zh=zh, zs=zs, st_ln=st_ln, flash=flash)
            self.t = t
        return ctx

    # ------------------------------------------------------------------ backward
    def backward(self, dctx: torch.Tensor) -> Dict[str, torch.Tensor]:
        t = self.t
        self.bind(*t["bound"])                                         # the parameters and the stage of the forward that wrote this tape
        o, p, gbuf = self.ops, self.p, self.gbuf
        pre = "cond_encoder."
        B, L = t["B"], self.L
        g: Dict[str, torch.Tensor] = {}
        two_streams, o.async_dw = o.stream_modes()                     # weight gradients on the side streams (train_engine.Ops.lin_bwd_w)

        def gw(name):
            g[name] = gbuf[name] if gbuf is not None else torch.empty_like(p[name])
            return g[name]

        o.lin_bwd_w(mv(dctx), mv(t["zs"]), mv(gw("cond_lin.weight")), gw("cond_lin.bias"))
        dzs = self.f(B, 256)
        o.lin_bwd_x(mv(dctx), mv(p["cond_lin.weight"]), mv(dzs))
        dzh = self.f(B, 256)
        E._check(self.lib.dst_ln_affine_bwd(ptr(dzs), ptr(t["zh"]), ptr(t["st_ln"]), B, 256, ptr(p[pre + "out_norm.weight"]),
                                            ptr(dzh), ptr(gw(pre + "out_norm.weight")), ptr(gw(pre + "out_norm.bias")), self.ops._s()),
                 "dst_ln_affine_bwd")
        o.lin_bwd_w(mv(dzh), mv(t["flat"]), mv(gw(pre + "head.linear.weight")), gw(pre + "head.linear.bias"))
        dZ = self.f(B * L, D_MODEL)
        o.lin_bwd_x(mv(dzh), mv(p[pre + "head.linear.weight"]), mv(dZ.view(B, L * D_MODEL)))
        dscores_in = None
        scale = float(D_K ** -0.5)
        cat_dst, cat_src = [], []                                      # gradients of the concatenated W_Q | W_K | W_V, scattered after the side stream has joined
        flash = t["flash"]
        if flash:                                                      # every layer's attention backward adds into the q | k columns of the layers below it
            dqkv_all = [self.f(B * L, 3 * D_MODEL) for _ in range(N_LAYERS)]     # (assigned by the last layer's call: accumulate = 0)
            qkv_all = [lt_["qkv"] for lt_ in t["layers"]]
        for l in reversed(range(N_LAYERS)):
            lt = t["layers"][l]
            base = pre + f"backbone.encoder.layers.{l}."
            dr2 = self.f(B * L, D_MODEL)
            self._bn_bwd(dZ, lt["r2"], lt["st2"], base + "norm_ffn.1", dr2, g)
            o.lin_bwd_w(mv(dr2), mv(lt["ga"]), mv(gw(base + "ff.3.weight")), gw(base + "ff.3.bias"))
            da = self.f(B * L, D_FF)
            o.lin_bwd_x(mv(dr2), mv(p[base + "ff.3.weight"]), mv(da), dact=GELU, ref=mv(lt["a"]))
            o.lin_bwd_w(mv(da), mv(lt["z1"]), mv(gw(base + "ff.0.weight")), gw(base + "ff.0.bias"))
            dz1 = self.f(B * L, D_MODEL)                                                         # dz1 = dr2 (residual) + da W0, in a buffer of its own:
            o.lin_bwd_x(mv(da), mv(p[base + "ff.0.weight"]), mv(dz1), dact=ADDREF, ref=mv(dr2))  # dr2 is an operand of a weight-gradient product that
                                                                                                 # may still be running on the side stream
            dr1 = self.f(B * L, D_MODEL)
            self._bn_bwd(dz1, lt["r1"], lt["st1"], base + "norm_attn.1", dr1, g)
            o.lin_bwd_w(mv(dr1), mv(lt["ao"]), mv(gw(base + "self_attn.to_out.0.weight")), gw(base + "self_attn.to_out.0.bias"))
            dao = self.f(B * L, D_MODEL)
            o.lin_bwd_x(mv(dr1), mv(p[base + "self_attn.to_out.0.weight"]), mv(dao))
            if flash:
                qp = [ptr(q_) for q_ in qkv_all[:l + 1]] + [None] * (2 - l)
                gp = [ptr(q_) for q_ in dqkv_all[:l + 1]] + [None] * (2 - l)
                def flash_bwd(part):
                    E._check(self.lib.dst_spec_attn_flash_bwd(qp[0], qp[1], qp[2], l + 1, ptr(lt["ast"]), ptr(lt["ao"]), ptr(dao), gp[0], gp[1],
                                                              gp[2], B, L, N_HEADS, D_K, scale,
                                                              part, 0 if l == N_LAYERS - 1 else 1, self.ops._s()), "dst_spec_attn_flash_bwd")
                if two_streams:                                        # the key side beside the query side (disjoint columns of dqkv): each kernel
                    with o.node_section():                             # alone keeps two 4-wave workgroups on a CU
                        flash_bwd(2)
                    flash_bwd(1)
                    o.main_wait()
                else:
                    flash_bwd(0)
                dqkv, dscores = dqkv_all[l], None
            else:
                dqkv, dscores = self.f(B * L, 3 * D_MODEL), self.f(B, N_HEADS, L, (L + 31) // 32 * 32)
                E._check(self.lib.dst_spec_attn_bwd(ptr(lt["qkv"]), ptr(lt["scores"]), ptr(lt["ast"]), ptr(dao), ptr(dscores_in), ptr(dqkv), ptr(dscores),
                                                    B, L, N_HEADS, D_K, scale, self.ops._s()),
                         "dst_spec_attn_bwd")
            dzin = self.f(B * L, D_MODEL)                                                        # dZin = dr1 (residual) + dqkv Wqkv (dr1 stays intact, as dr2 above)
            dWc, dbc = self.f(3 * D_MODEL, D_MODEL), self.f(3 * D_MODEL)
            o.lin_bwd_w(mv(dqkv), mv(lt["Zin"]), mv(dWc), dbc)
            o.lin_bwd_x(mv(dqkv), mv(lt["Wqkv"]), mv(dzin), dact=ADDREF, ref=mv(dr1))
            for k, nm in enumerate(("W_Q", "W_K", "W_V")):
                cat_dst += [gw(base + f"self_attn.{nm}.weight"), gw(base + f"self_attn.{nm}.bias")]
                cat_src += [dWc[k * D_MODEL:(k + 1) * D_MODEL], dbc[k * D_MODEL:(k + 1) * D_MODEL]]
            dscores_in = dscores if lt["has_prev"] else None
            dZ = dzin
        dZ3 = dZ.view(B, L, D_MODEL)
        tok0 = 0
        for slot, (pl, stv, pn) in enumerate(self.patch):
            dz = dZ3[:, tok0:tok0 + pn].contiguous().reshape(B * pn, D_MODEL)
            o.lin_bwd_w(mv(dz), mv(t["Xs"][slot]), mv(gw(pre + f"backbone.W_P.{slot}.weight")), gw(pre + f"backbone.W_P.{slot}.bias"))
            o.colsum(mv(dz.view(B, pn * D_MODEL)), gw(pre + "backbone." + self.pos_names[slot]).view(-1))
            tok0 += pn
        o.join_dw()
        o.async_dw = False
        torch._foreach_copy_(cat_dst, cat_src)
        self.t = None
        return g
