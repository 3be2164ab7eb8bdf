"""Training step of the DMT on the MI355X - the surface of reference ``losses.py`` (BASELINE config 5).

Same factories and call conventions: ``get_optimizer(config, params)`` (``losses.py:14-25``), ``optimization_manager(config)`` ->
``optimize_fn(optimizer, params, step)`` with lr warm-up and the adaptive gradient-clipping queue (``:28-94``),
``get_sde_graph_loss_fn(noise_scheduler, train, scaler, config)`` -> ``loss_fn(model, batch)`` (``:286-396``) and
``get_step_fn(...)`` -> ``step_fn(state, batch)`` (``:97-125``: zero_grad, loss, ``loss.backward()``, optimize, EMA).

What runs underneath is not autograd: ``loss_fn`` drives the HIP training library (``train_engine.DmtTrainGraph`` +
``spec_train.SpecTrainGraph``: forward tape and hand-written backward of every operation) and hands the finished gradients to
``loss.backward()`` through a one-node ``torch.autograd.Function``; the optimizer is one fused kernel over a flat parameter
buffer (AdamW-amsgrad + gradient clipping + EMA), and with a process group the gradients are reduce-scattered, every rank
updates its shard, and the parameters are all-gathered (RCCL over xGMI) - no parameter broadcast per call as ``nn.DataParallel``
does (``models/utils.py:27``).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from random import random
from typing import Dict, List

import numpy as np
import torch
import torch.distributed as dist

from . import engine as E
from .abi import ptr
from .ema import ExponentialMovingAverage
from .scalers import _factors, get_self_cond_fn
from .spec_train import SpecTrainGraph
from .train_engine import DmtTrainGraph, Ops, TrainLayout, load_train_library


# ----------------------------------------------------------------------------------------------------------- optimizer
FLAT_ALIGN = 64        # floats: every parameter starts on a 256-byte boundary of the flat buffers (the GEMM kernels load operands 16 bytes at a time)


def flat_offsets(sizes, align: int = FLAT_ALIGN):
    """Start offset of every tensor in a flat buffer that keeps each one ``align``-element aligned, plus the total length (last entry).
    Shared by the optimizer's parameter / gradient buffers and the trainer's gradient stage: equal layouts make ``loss.backward()`` one add."""
    offs, cur = [], 0
    for n in sizes:
        offs.append(cur)
        cur += (int(n) + align - 1) // align * align
    offs.append(cur)
    return offs


class FusedAdamW:
    """``torch.optim.AdamW(params, lr, amsgrad=True, weight_decay)`` (losses.py:20) as ONE kernel over a flat fp32 buffer.

    The parameters are re-pointed to views of one flat buffer (their values are kept), and so are their ``.grad`` s.  ``step``
    optionally folds in the gradient-clipping coefficient and the EMA update (``models/ema.py:24-42``).  With an initialised
    process group of W ranks the step is sharded: reduce-scatter of the flat gradient (mean over ranks), each rank updates 1/W
    of the parameters (and holds 1/W of the optimizer state), all-gather of the parameters.  ``state_dict`` / ``load_state_dict``
    speak ``torch.optim.AdamW``'s format, so checkpoints interchange with the reference's (``utils.py:7-30``)."""

    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-12, amsgrad=True, force_sharded=False):
        if not amsgrad:
            raise ValueError("the fused kernel implements the shipped configuration: AdamW with amsgrad=True")
        self.params: List[torch.nn.Parameter] = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdamW runs on an MI355X only; diffspectra_amd has no CPU path")
        self.lib = load_train_library()
        self.dev = dev
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        # the sharded step (reduce-scatter, shard update, all-gather) runs with more than one rank - or, as a rehearsal of exactly
        # those RCCL calls, on a one-rank group with force_sharded (shard = everything; results equal the unsharded step bit for bit)
        self.sharded = self.world > 1 or (bool(force_sharded) and dist.is_available() and dist.is_initialized())
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=True, params=list(range(len(self.params))))]
        self.sizes = [p.numel() for p in self.params]
        self.offsets = flat_offsets(self.sizes)
        n = self.offsets[-1]
        self.n = n
        unit = 256 * self.world
        self.n_pad = (n + unit - 1) // unit * unit
        self.shard = self.n_pad // self.world
        self.P = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        self.G = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            if p.dtype != torch.float32:
                raise ValueError("FusedAdamW expects fp32 parameters")
            self.P[o:o + p.numel()] = p.data.reshape(-1)
            p.data = self.P[o:o + p.numel()].view(p.shape)
            p.grad = self.G[o:o + p.numel()].view(p.shape)
        lo = self.rank * self.shard
        self.Ps, self.Gs = self.P[lo:lo + self.shard], (torch.zeros(self.shard, device=dev) if self.sharded else self.G[lo:lo + self.shard])
        self.M, self.V, self.Vmax = (torch.zeros(self.shard, dtype=torch.float32, device=dev) for _ in range(3))
        self.steps = 0
        self.scratch = torch.empty(1024, dtype=torch.float32, device=dev)
        self.norm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_state, self._clip_pending = None, False
        self.ema_flat = None

    def unpadded(self, flat: torch.Tensor) -> torch.Tensor:
        """The parameters' elements of a flat buffer in ``parameters()`` order without the alignment gaps (what ``torch.cat`` of the
        flattened tensors gives)."""
        return torch.cat([flat[o:o + n] for o, n in zip(self.offsets, self.sizes)])

    # -- torch.optim surface
    def zero_grad(self, set_to_none: bool = False):
        self.G.zero_()
        for p, o in zip(self.params, self.offsets):                    # keep .grad pointing into the flat buffer
            if p.grad is None or p.grad.data_ptr() != self.G.data_ptr() + 4 * o:
                p.grad = self.G[o:o + p.numel()].view(p.shape)

    def _sync_grads(self):
        """Mean of the gradients over the ranks, scattered: every rank ends with its shard in ``self.Gs``."""
        if not self.sharded:
            return
        if dist.get_backend() == "gloo":                                # rehearsal backend: no reduce_scatter
            dist.all_reduce(self.G)
            self.Gs.copy_(self.G[self.rank * self.shard:(self.rank + 1) * self.shard])
        else:
            dist.reduce_scatter_tensor(self.Gs, self.G, op=dist.ReduceOp.SUM)

    def _norm_sq(self):
        self._sync_grads()
        self._synced = True
        E._check(self.lib.dst_sumsq(ptr(self.Gs), self.shard, ptr(self.norm_sq), 0, ptr(self.scratch),
                                    self.scratch.numel(), E._stream()), "dst_sumsq")
        if self.sharded:
            ns = self.norm_sq if dist.get_backend() != "gloo" else self.norm_sq.cpu()
            dist.all_reduce(ns)
            self.norm_sq.copy_(ns)

    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the (rank-averaged) gradient: what ``clip_grad_norm_`` returns.  Synchronises the gradients."""
        self._norm_sq()
        return torch.sqrt(self.norm_sq[0]) / self.world                 # the shards hold SUMS over ranks; the mean's norm is 1/W of it

    def clip_on_device(self, max_grad: float, first: float = 3000.0) -> torch.Tensor:
        """``gradient_clipping`` (losses.py:28-50) without the reference's ``float(grad_norm)`` round trip: norm, norm history, allowed
        norm and coefficient stay on the device (``dst_clip_update``) and the next ``step`` multiplies the gradient by the coefficient
        it finds there - the host keeps issuing the next step while this one runs.  Returns the state tensor ([51] coefficient,
        [52] norm, [53] allowed norm); reading it is the caller's synchronisation."""
        if self.clip_state is None:
            self.clip_state = torch.zeros(64, dtype=torch.float32, device=self.dev)
            self.clip_state[0] = first                                  # "large value that will be flushed" (losses.py:79)
            self.clip_state[50] = 1.0
        self._norm_sq()
        E._check(self.lib.dst_clip_update(ptr(self.norm_sq), 1.0 / self.world, float(max_grad), ptr(self.clip_state),
                                          E._stream()), "dst_clip_update")
        self._clip_pending = True
        return self.clip_state

    def attach_ema(self, ema: ExponentialMovingAverage):
        """Fold ``ema.update`` into the step kernel: the shadow parameters become views of one flat buffer."""
        flat = torch.zeros(self.n_pad, dtype=torch.float32, device=self.dev)
        trainable = [i for i, p in enumerate(self.params) if p.requires_grad]
        if len(trainable) != len(ema.shadow_params):
            raise ValueError("EMA and optimizer must cover the same trainable parameters")
        flat.copy_(self.P)                                             # frozen parameters: their slots just track the parameter
        for i, s in zip(trainable, ema.shadow_params):
            o = self.offsets[i]
            flat[o:o + s.numel()] = s.reshape(-1).to(self.dev)
        ema.shadow_params = [flat[self.offsets[i]:self.offsets[i] + self.sizes[i]].view(self.params[i].shape) for i in trainable]
        self.ema_flat, self.ema = flat, ema
        self._ema_stale = False
        ema._before_read = self.gather_ema
        ema._after_load = self._ema_loaded

    def _ema_loaded(self):
        self._ema_stale = False                                        # every rank has just loaded the full averages

    def gather_ema(self):
        """All-gather the EMA shards (only when the averages are read: ``ema.copy_to`` / ``ema.state_dict``)."""
        if not self.sharded or self.ema_flat is None or not self._ema_stale:
            return
        lo = self.rank * self.shard
        mine = self.ema_flat[lo:lo + self.shard].clone()
        if dist.get_backend() == "gloo":
            parts = [torch.empty(self.shard) for _ in range(self.world)]
            dist.all_gather(parts, mine.cpu())
            self.ema_flat.copy_(torch.cat(parts).to(self.dev))
        else:
            dist.all_gather_into_tensor(self.ema_flat, mine)
        self._ema_stale = False

    @torch.no_grad()
    def step(self, clip_coef: float = 1.0, ema: ExponentialMovingAverage = None):
        if not getattr(self, "_synced", False):
            self._sync_grads()
        self._synced = False
        g = self.param_groups[0]
        self.steps += 1
        b1, b2 = g["betas"]
        ema_omd = 0.0
        ema_ptr = None
        if ema is not None:
            if self.ema_flat is None or getattr(self, "ema", None) is not ema:
                self.attach_ema(ema)
            ema_omd = 1.0 - ema.effective_decay()
            if ema.num_updates is not None:
                ema.num_updates += 1
            lo = self.rank * self.shard
            ema_ptr = self.ema_flat[lo:lo + self.shard]
        E._check(self.lib.dst_adamw_ema(ptr(self.Ps), ptr(self.Gs), ptr(self.M), ptr(self.V), ptr(self.Vmax), ptr(ema_ptr),
                                        self.shard, float(g["lr"]), b1, b2, g["eps"],
                                        g["weight_decay"], 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps,
                                        float(clip_coef) / self.world, ptr(self.clip_state[51:52]) if self._clip_pending else None,
                                        ema_omd, E._stream()), "dst_adamw_ema")
        self._clip_pending = False
        if self.sharded:
            if dist.get_backend() == "gloo":                           # rehearsal backend: host tensors
                parts = [torch.empty(self.shard) for _ in range(self.world)]
                dist.all_gather(parts, self.Ps.cpu())
                self.P.copy_(torch.cat(parts).to(self.dev))
            else:
                dist.all_gather_into_tensor(self.P, self.Ps.clone())
            if ema_ptr is not None:
                self._ema_stale = True                                  # the other ranks' EMA shards are gathered when the EMA is read

    def _gathered(self, shard_t: torch.Tensor) -> torch.Tensor:
        if not self.sharded:
            return shard_t
        if dist.get_backend() == "gloo":                               # rehearsal backend: host tensors
            parts = [torch.empty(self.shard) for _ in range(self.world)]
            dist.all_gather(parts, shard_t.cpu())
            return torch.cat(parts).to(self.dev)
        full = torch.empty(self.n_pad, dtype=torch.float32, device=self.dev)
        dist.all_gather_into_tensor(full, shard_t.clone())
        return full

    def state_dict(self):
        """``torch.optim.AdamW.state_dict()`` format (what the reference's ``save_checkpoint`` stores, golden G14).

        With more than one rank the optimizer state is sharded (ZeRO-1), so this call is a COLLECTIVE: every rank must make it
        (``evaluate.save_checkpoint`` does, and lets rank 0 write the file); a "rank 0 only" caller would wait for ever."""
        M, V, X = self._gathered(self.M), self._gathered(self.V), self._gathered(self.Vmax)
        state = {}
        if self.steps > 0:
            for i, (o, n, p) in enumerate(zip(self.offsets, self.sizes, self.params)):
                if not p.requires_grad:
                    continue                                          # torch keeps no state for parameters that never received a gradient
                state[i] = dict(step=torch.tensor(float(self.steps)), exp_avg=M[o:o + n].view(p.shape).clone(), exp_avg_sq=V[o:o + n].view(p.shape).clone(),
                                max_exp_avg_sq=X[o:o + n].view(p.shape).clone())
        g = self.param_groups[0]
        group = dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], amsgrad=True, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True, params=list(range(len(self.params))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.param_groups[0].update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"])
        full = [torch.zeros(self.n_pad, dtype=torch.float32, device=self.dev) for _ in range(3)]
        for i, st in sd["state"].items():
            o, n = self.offsets[int(i)], self.sizes[int(i)]
            self.steps = int(float(st["step"]))
            for buf, key in zip(full, ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
                buf[o:o + n] = st[key].reshape(-1).to(self.dev)
        lo = self.rank * self.shard
        for dst, src in zip((self.M, self.V, self.Vmax), full):
            dst.copy_(src[lo:lo + self.shard])


def get_optimizer(config, params):
    """losses.py:14-25.  'AdamW' is the shipped optimizer: AdamW(lr, amsgrad=True, weight_decay=1e-12), here the fused kernel."""
    if config.optim.optimizer == "AdamW":
        return FusedAdamW(params, lr=config.optim.lr, amsgrad=True, weight_decay=1e-12,
                          force_sharded=bool(getattr(config.optim, "force_sharded", False)))
    raise NotImplementedError(f"Optimizer {config.optim.optimizer} not supported yet!")


class Queue:
    """losses.py:53-72 (gradient-norm history of the adaptive clipping)."""

    def __init__(self, max_len=50):
        self.items, self.max_len = [], max_len

    def __len__(self):
        return len(self.items)

    def add(self, item):
        self.items.insert(0, item)
        if len(self) > self.max_len:
            self.items.pop()

    def mean(self):
        return np.mean(self.items)

    def std(self):
        return np.std(self.items)


def clip_coefficient(grad_norm: float, gradnorm_queue: Queue, max_grad: float):
    """The scale ``clip_grad_norm_`` applies inside ``gradient_clipping`` (losses.py:28-50) and the queue update: allowed norm =
    min(1.5 mean + 2 std of the recent history, max_grad); coefficient = min(1, allowed / (norm + 1e-6))."""
    if max_grad <= 1.0:
        return min(1.0, max_grad / (grad_norm + 1e-6)), max_grad
    max_grad_norm = min(1.5 * gradnorm_queue.mean() + 2 * gradnorm_queue.std(), max_grad)
    gradnorm_queue.add(float(max_grad_norm) if grad_norm > max_grad_norm else float(grad_norm))
    return min(1.0, float(max_grad_norm) / (grad_norm + 1e-6)), max_grad_norm


def optimization_manager(config):
    """losses.py:75-94: lr warm-up + adaptive gradient clipping + optimizer step."""
    gradnorm_queue = Queue()
    gradnorm_queue.add(3000)                                            # large value that will be flushed (losses.py:79)

    def optimize_fn(optimizer, params, step, lr=config.optim.lr, warmup=config.optim.warmup, grad_clip=config.optim.grad_clip, ema=None):
        if warmup > 0:
            for g in optimizer.param_groups:
                g["lr"] = lr * np.minimum(step / warmup, 1.0)
        coef = 1.0
        if grad_clip >= 0:
            if hasattr(optimizer, "clip_on_device"):
                # the reference's float(grad_norm) is a device -> host synchronisation in every step; here the clipping (norm history
                # included) runs on the device and the host is free to issue the next step.  last_grad_norm is a 0-dim device tensor
                st = optimizer.clip_on_device(grad_clip)
                optimize_fn.last_grad_norm = st[52]
                optimize_fn.device_state = st
            else:
                norm = float(optimizer.grad_norm())
                coef, _ = clip_coefficient(norm, gradnorm_queue, grad_clip)
                optimize_fn.last_grad_norm = norm
        optimizer.step(clip_coef=coef, ema=ema)

    class _History:
        """``optimize_fn.queue``: the norm history the clipping rule looks at.  Host-side clipping keeps it in ``gradnorm_queue``; with
        the fused optimizer the history lives in ``clip_state`` on the device ([0 .. count) newest first, [50] count) and reading it
        here is a device -> host copy (a synchronisation the step itself never does)."""

        @property
        def items(self):
            st = getattr(optimize_fn, "device_state", None)
            if st is None:
                return list(gradnorm_queue.items)
            host = st.detach().cpu()
            return [float(v) for v in host[:int(host[50])]]                # newest first, like Queue.items

        def mean(self):
            return np.mean(self.items)

        def std(self):
            return np.std(self.items)

        def __len__(self):
            return len(self.items)

    optimize_fn.queue = _History()
    return optimize_fn


# ----------------------------------------------------------------------------------------------------------- loss
class _HipLoss(torch.autograd.Function):
    """One autograd node whose backward hands out gradients the HIP library has already computed."""

    @staticmethod
    def forward(ctx, loss_value, grads, *params):
        ctx.grads = grads
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        live = [g for g in ctx.grads if g is not None]
        torch._foreach_mul_(live, grad_out)                 # one multi-tensor launch instead of one per parameter
        return (None, None) + tuple(ctx.grads)


class _HipLossFlat(torch.autograd.Function):
    """The same hand-over when every ``p.grad`` is a view of ONE flat buffer laid out like the trainer's gradient stage (the fused
    optimizer's arrangement): ``loss.backward()`` is then a single ``G += stage * grad_out`` instead of one accumulation per parameter."""

    @staticmethod
    def forward(ctx, loss_value, stage, target, tr, generation, *params):
        ctx.stage, ctx.target, ctx.tr, ctx.generation = stage, target, tr, generation
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        # the stage is the trainer's ONE shared buffer: a later loss_fn / model(...) backward on the same model rewrites it.  The
        # gradients of this call are then gone - refuse instead of silently adding another batch's gradients
        if ctx.tr.stage_generation != ctx.generation:
            raise RuntimeError("loss.backward() after another loss_fn(model, ...) call on the same model: the gradient stage of this "
                               "loss was overwritten.  Call backward() before the next loss_fn (gradient accumulation: "
                               "loss_fn(b1).backward(); loss_fn(b2).backward())")
        ctx.target.addcmul_(ctx.stage, grad_out.to(ctx.stage.dtype))
        return (None,) * len(ctx.needs_input_grad)


def _deliver_grads(tr, named, g, flat, offs):
    """The hand-over of a finished backward (``g``: its gradients, views of the stage ``flat``) to autograd, as ``(target, grads)``.  When
    every ``p.grad`` is a view of one flat buffer laid out like the stage, ``target`` is that buffer - the caller adds the stage (frozen
    slices cleared here) into it with ONE kernel and its autograd node returns None s - and ``grads`` is None; otherwise ``target`` is None
    and ``grads`` holds per-parameter clones (the stage is overwritten by the next call; None for a frozen parameter)."""
    missing = [n for n, p in named.items() if p.requires_grad and n not in g]
    if missing:
        raise RuntimeError(f"no gradient was produced for {missing[:5]}")
    target = tr.flat_grad_target(named, offs)
    if target is not None:
        zero_frozen(flat, named, offs)
        return target, None
    return None, [g[n].clone() if p.requires_grad else None for n, p in named.items()]


def zero_frozen(flat, named, offs):
    """The backward kernels write a gradient for every parameter; the flat hand-over adds the WHOLE stage into the optimizer's buffer.
    Slices of parameters with ``requires_grad=False`` are cleared first, so a frozen parameter keeps a zero gradient (the per-parameter
    path returns None for it) and the fused AdamW step leaves it where it is."""
    for (name, p), o in zip(named.items(), offs):
        if not p.requires_grad:
            flat[o:o + p.numel()].zero_()


class HipTrainer:
    """Per-model training state: the two graphs, bound to the model's current parameter storage at every call."""

    def __init__(self, module, config):
        self.module, self.cfg = module, config
        self.dev = next(module.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("training runs on an MI355X only (move the model to a 'cuda' device); there is no CPU path")
        self.ops = Ops(self.dev)
        self.lib = self.ops.lib
        self.dmt = DmtTrainGraph({}, config, self.dev, self.ops)      # bound to the parameters' current storage by graphs()
        self.spec = SpecTrainGraph({}, {}, config, self.ops)
        self._registry = None           # (module identity, named parameters, named buffers): the module tree is walked once
        self._layouts: Dict[bytes, TrainLayout] = {}
        self._layout_seen = None        # (mask tensor, its version, key into _layouts) of the last layout() call
        self._flat_ok = None            # (key, base, target) of the last flat gradient buffer flat_grad_target() accepted
        self._stage = None
        self.stage_generation = 0       # bumped whenever the shared gradient stage is rewritten (checked by _HipLossFlat.backward)

    def stage_begin(self, named):
        """Claim the shared stage for a new backward: cleared, generation bumped (a pending flat hand-over of an earlier call notices)."""
        flat, views, offs = self.stage(named)
        self.stage_generation += 1
        flat.zero_()
        return flat, views, offs

    def stage(self, named):
        """One flat fp32 buffer holding every parameter's gradient of the current backward, in ``named_parameters()`` order without
        gaps, and the per-parameter views the backward kernels write into."""
        sizes = [p.numel() for p in named.values()]
        offs = flat_offsets(sizes)
        n = offs[-1]
        if self._stage is None or self._stage[0].numel() != n:
            flat = torch.zeros(n, dtype=torch.float32, device=self.dev)
            views = {name: flat[o:o + p.numel()].view(p.shape) for (name, p), o in zip(named.items(), offs)}
            self._stage = (flat, views, offs)
        return self._stage

    def flat_grad_target(self, named, offs):
        """The flat buffer all ``p.grad`` s are views of, if they are laid out exactly like the stage (``FusedAdamW`` does that), else None."""
        params = list(named.values())
        first = next((i for i, p in enumerate(params) if p.requires_grad), None)
        if first is None or params[first].grad is None:
            return None
        base = params[first].grad._base
        if base is None or base.dim() != 1 or not base.is_contiguous() or base.dtype != torch.float32:
            return None
        key = (base.data_ptr(), tuple(int(p.grad.data_ptr()) if (p.requires_grad and p.grad is not None) else -1 for p in params[::37]))
        cached = self._flat_ok
        if cached is not None and cached[0] == key and cached[1] is base:
            return cached[2]
        b0 = base.data_ptr()
        for p, o in zip(params, offs):
            if not p.requires_grad:
                continue
            gr = p.grad
            if gr is None or gr._base is not base or not gr.is_contiguous() or gr.data_ptr() != b0 + 4 * o:
                return None
        n = offs[-1]
        if base.numel() < n:
            return None
        target = base[:n]
        self._flat_ok = (key, base, target)
        return target

    def layout(self, atom_mask, ident=None) -> TrainLayout:
        # The packed layout is a function of the mask's CONTENT: reading it is a device -> host copy, i.e. the host waits for everything the
        # stream still holds (the previous step's tail) - the one synchronisation of a step.  A mask tensor that was seen in the last call
        # (the same object - held here, so its address cannot be given to another tensor - at the same version counter: an epoch over
        # pre-uploaded batches, bench.py) is recognised without reading it.  ``ident``: the caller's own tensor to recognise the mask by,
        # when ``atom_mask`` is a temporary made from it.
        ident = atom_mask if ident is None else ident
        seen = self._layout_seen
        if seen is not None and seen[0] is ident and seen[1] == ident._version and seen[2] in self._layouts:
            return self._layouts[seen[2]]
        key = (atom_mask != 0).to("cpu").numpy().tobytes() + bytes(atom_mask.shape[1])
        self._layout_seen = (ident, ident._version, key)
        if key not in self._layouts:
            if len(self._layouts) >= 8:
                self._layouts.pop(next(iter(self._layouts)))
            self._layouts[key] = TrainLayout(atom_mask.unsqueeze(2), self.dev)
        return self._layouts[key]

    def graphs(self):
        # (the module tree is walked once: named_parameters() / named_buffers() of ~400 modules cost 2 ms of host time per step)
        reg = self._registry
        if reg is None or reg[0] != (id(self.module), len(self.module._modules)):          # (set tr._registry = None after surgery on the module tree)
            reg = ((id(self.module), len(self.module._modules)), dict(self.module.named_parameters()), {k: v for k, v in self.module.named_buffers()})
            self._registry = reg
        named, bufs = reg[1], reg[2]
        pd = {k: v.data for k, v in named.items()}
        gbuf = self.stage(named)[1]
        self.dmt.bind(pd, gbuf)
        self.spec.bind(pd, gbuf, bufs)
        self.dmt.prepare_weights()                  # concatenated weights of this call's parameters (one multi-tensor copy)
        return named, self.dmt, self.spec


def _trainer(model) -> HipTrainer:
    m = getattr(model, "module", model)
    if not hasattr(m, "engine"):
        raise TypeError(f"diffspectra_amd.losses drives the HIP DMT (diffspectra_amd.dmt.DMT); got {type(m).__name__}")
    tr = getattr(m, "_hip_trainer", None)
    if tr is None or tr.dev != next(m.parameters()).device:
        tr = HipTrainer(m, m.config)
        m._hip_trainer = tr
    return tr


def get_sde_graph_loss_fn(noise_scheduler, train, scaler, config, prop_norm=None):
    """losses.py:286-396 for the shipped mode (DMT, pred_data, self_cond, noise_align, reduce_mean False).  ``scaler`` is accepted
    for signature compatibility; the scaling of ``process_edge_batch`` runs in ``dst_prepare_batch`` with the same factors.
    ``config.model.dropout`` (0.1 as shipped) is the FF dropout of the blocks, with in-kernel Philox masks (``dst_dropout``); golden
    G13 pins the p = 0 arithmetic, the masks themselves cannot agree with torch's generator."""
    if not (config.model.pred_data and config.model.self_cond and config.model.noise_align and config.model.name == "DMT"):
        raise ValueError("the MI355X training step implements the shipped mode: DMT, pred_data, self_cond, noise_align")
    if config.training.reduce_mean:
        raise ValueError("training.reduce_mean=True is not implemented (every shipped config has False)")
    if not config.data.centered or not config.model.include_fc_charge:
        raise ValueError("the batch preparation kernel implements centered data with formal charges")
    dropout_p = float(getattr(config.model, "dropout", 0.0))
    precision = getattr(config.training, "precision", "fp32")
    if precision not in ("fp32", "bf16"):
        raise ValueError("config.training.precision must be 'fp32' or 'bf16'")
    loss_weights = [float(w) for w in config.model.loss_weights.split(",")]
    cond_process_fn = get_self_cond_fn(config)
    pos_norm, type_norm, fc_norm, edge_norm = (float(v) for v in _factors(config))

    def loss_fn(model, batch):
        tr = _trainer(model)
        tr.ops.begin()                                                   # one stream lookup for the ~1 700 launches of the call
        try:
            return _loss_fn(model, batch, tr)
        finally:
            tr.ops.end()

    def _loss_fn(model, batch, tr):
        if model.training != bool(train):                              # (Module.train() walks every sub-module: 1.6 ms per call)
            model.train() if train else model.eval()
        dev, lib = tr.dev, tr.lib
        tr.ops.bf16 = precision == "bf16"          # config 5: bf16 products with fp32 accumulation, fp32 master weights (set BEFORE graphs(): the
        named, dmt, spec = tr.graphs()             # per-step weight copies depend on the mode)
        atom_mask = batch["atom_mask"].to(dev)
        TL = tr.layout(atom_mask)
        B, N = TL.B, TL.N
        f32 = lambda t: t.to(dev, torch.float32)
        pos_p, oh_p = TL.pack_nodes(f32(batch["positions"])), TL.pack_nodes(f32(batch["atom_one_hot"]))
        fc_p, edge_p = TL.pack_nodes(f32(batch["formal_charges"])).reshape(-1).contiguous(), TL.pack_pairs(f32(batch["edge_one_hot"]))
        x, ex = dmt.f(TL.Nn, 9), dmt.f(max(TL.Pp, 1), 2)
        E._check(lib.dst_prepare_batch(C.byref(TL.c), ptr(pos_p), ptr(oh_p), ptr(fc_p), ptr(edge_p), pos_norm, type_norm,
                                       fc_norm, edge_norm, ptr(x), ptr(ex), tr.ops._s()), "dst_prepare_batch")
        context = batch["context"]
        context = [f32(c) for c in context] if isinstance(context, (list, tuple)) else f32(context)
        # the random draws, in the reference's order and shapes (losses.py:314-317, models/utils.py:67-106)
        t = torch.rand(B, device=dev) * (1.0 - 1e-5) + 1e-5
        alpha_t, sigma_t = noise_scheduler.marginal_prob(t)
        raw_pos, raw_feat = torch.randn((B, N, 3), device=dev), torch.randn((B, N, 6), device=dev)
        raw_edge = torch.randn((B, 2, N, N), device=dev)
        raw_n = TL.pack_nodes(torch.cat([raw_pos, raw_feat], dim=2))
        raw_e = raw_edge.permute(0, 2, 3, 1).reshape(B * N * N, 2).index_select(0, TL.pair_dense_t).contiguous()   # tril(-1) value of the pair
        z, ez = dmt.f(TL.Nn, 9), dmt.f(max(TL.Pp, 1), 2)
        alpha_t, sigma_t = alpha_t.to(torch.float32).contiguous(), sigma_t.to(torch.float32).contiguous()
        E._check(lib.dst_noising(C.byref(TL.c), ptr(alpha_t), ptr(sigma_t), ptr(x), ptr(raw_n), ptr(z), ptr(ex), ptr(raw_e), ptr(ez),
                                 tr.ops._s()), "dst_noising")
        rot, aligned = dmt.f(B, 9), dmt.f(TL.Nn, 3)
        E._check(lib.dst_kabsch(C.byref(TL.c), ptr(z), 9, ptr(x), 9, ptr(rot), ptr(aligned), tr.ops._s()), "dst_kabsch")
        noise_level = torch.log(alpha_t ** 2 / sigma_t ** 2).contiguous()
        cond_n = cond_e = None
        # FF dropout (dmt.py:114-120) is active whenever the model is in training mode - in the no-grad self-conditioning forward too
        dmt.dropout_p = dropout_p if train else 0.0
        seeds = torch.randint(0, 2 ** 62, (2,)).tolist() if dmt.dropout_p > 0 else [0, 0]
        # the conditioning encoder sees the same spectra in both forwards of a self-conditioning step (losses.py:344-357): evaluated
        # once, with the running-statistics update of the second pass applied from the saved batch statistics
        ctx = spec.forward(context, save=train) if train else _eval_context(model, context)
        if random() < 0.5:                                              # self-conditioning forward, no gradient (losses.py:344-351)
            dmt.dropout_seed = seeds[0]
            if train:
                spec.running_stats_again()
            pos0, atom0, edge0 = dmt.forward(TL, z, ez, noise_level, ctx, None, None, save=False)
            cond_n, cond_e = torch.cat([pos0, atom0], dim=1).contiguous(), edge0
            if getattr(config.model, "self_cond_type", "ori") != "ori":
                cd, ce = cond_process_fn(TL.unpack_nodes(cond_n), TL.unpack_pairs(cond_e))
                cond_n, cond_e = TL.pack_nodes(cd), TL.pack_pairs(ce)
        dmt.dropout_seed = seeds[1]
        pos, atom, edge = dmt.forward(TL, z, ez, noise_level, ctx, cond_n, cond_e, save=train)
        wm = (torch.sqrt(alpha_t / sigma_t) / B).contiguous()
        tfeat = x[:, 3:9].contiguous()
        loss_m, dpos, dfeat, dedge = dmt.loss(TL, pos, atom, edge, aligned, tfeat, ex, wm, loss_weights)
        loss = loss_m.sum()
        loss_fn.last = dict(t=t, alpha_t=alpha_t, sigma_t=sigma_t, z=z, ez=ez, aligned=aligned, rot=rot, pred=(pos, atom, edge), layout=TL)
        if not (train and torch.is_grad_enabled()):
            return loss
        flat, _, offs = tr.stage_begin(named)                           # zeroed: gradients that a branch does not produce (first-step dist_layer) stay zero
        g = dmt.backward(dpos, dfeat, dedge)
        g.update(spec.backward(g.pop("@ctx_emb")))
        target, grads = _deliver_grads(tr, named, g, flat, offs)
        if target is not None:                                          # the fused optimizer's flat gradient buffer: one accumulation kernel
            return _HipLossFlat.apply(loss, flat, target, tr, tr.stage_generation, *named.values())
        return _HipLoss.apply(loss, grads, *named.values())

    return loss_fn


def _eval_context(model, context):
    """Eval-mode conditioning embedding (BatchNorm running statistics): the sampling engine's SpecFormer."""
    m = getattr(model, "module", model)
    return m.engine().context_embedding(context)


def get_step_fn(noise_scheduler, train, optimize_fn, scaler, config, prop_dist=None):
    """losses.py:97-125."""
    if not config.pred_edge or config.only_2D:
        raise ValueError("the MI355X training step implements the 3-D graph loss (pred_edge, not only_2D)")
    loss_fn = get_sde_graph_loss_fn(noise_scheduler, train, scaler, config, prop_dist)

    def step_fn(state, batch):
        model = state["model"]
        if train:
            optimizer = state["optimizer"]
            optimizer.zero_grad()
            loss = loss_fn(model, batch)
            loss.backward()
            fused = isinstance(optimizer, FusedAdamW) and isinstance(state["ema"], ExponentialMovingAverage)
            if fused:
                optimize_fn(optimizer, model.parameters(), step=state["step"], ema=state["ema"])      # EMA update inside the step kernel
            else:
                optimize_fn(optimizer, model.parameters(), step=state["step"])
            state["step"] += 1
            if not fused:
                state["ema"].update(model.parameters())
            m = getattr(model, "module", model)
            if hasattr(m, "invalidate_engine"):
                m.invalidate_engine()                                   # the sampling engine's packed weights are stale now
        else:
            with torch.no_grad():
                ema = state["ema"]
                ema.store(model.parameters())
                ema.copy_to(model.parameters())
                loss = loss_fn(model, batch)
                ema.restore(model.parameters())
        return loss

    return step_fn
