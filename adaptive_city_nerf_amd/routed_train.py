"""runtime_adapt's update of the ROUTED container on the pair kernels, capturable as one HIP graph.

Reference: pipelines/online_stage/runtime_adapt.py:286-309 with ``active_module=None`` -- the online
stage adapts the whole soft-routed container (models/inr/meta_container.py:275-343): every expert a
sample is routed to renders it, the blend is a weighted index_add_ in expert order, gradients reach
exactly the experts that received samples (the others keep grad None and Adam skips them), then
clip_grad_norm_(1.0) and Adam over every parameter with a gradient.

Here one step is a fixed sequence of launches with no host synchronisation, so it replays as a graph:

    routed_count / routed_scatter   t, routing weights, (sample, expert) pair slots, segments padded
                                    to 128 (routed.hip); jitter = torch.rand(N, S) (the reference's
                                    rand_like draw, graph-safe philox)
    hashgrid_fwd_pairs              h0 of every slot through its expert's table
    mlp_pack_pairs + fwd_pairs      the K expert MLPs on MFMA, per slot
    routed_blend_fwd                (M, 4) = sum_k y_k w_k in expert order
    background + volume_render + MSE under torch autograd (the small shared part)
    routed_blend_bwd / mlp_bwd_dw_pairs / hashgrid_bwd_pairs
                                    per-expert [dW | db] (deterministic order) and table gradients
                                    (float atomics into persistent buffers)
    grad_sumsq_slots + clip_coef + adam_step_slots
                                    clip norm and Adam over the ACTIVE experts only (pair count > 0,
                                    decided on the device) + the shared background head; the table
                                    gradients are cleared by the Adam pass itself.

Buffers are sized for the worst case (every sample routed to every expert), so the step never needs
the pair count on the host.  Parameters keep torch's optimizer state layout: exp_avg / exp_avg_sq are
the FusedAdam state tensors, state['step'] is synchronised from the per-expert device counters.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import AcnError, acn_mlp, check, graph_capture, ptr
from .meta_container import MetaContainer
from .optim import NORM_ELSEWHERE_FLAG, ZERO_GRAD_FLAG, AmpScaler, FusedAdam, SlottedAdam, bump_versions
from .ray_rendering import volume_render
from .train import mse_color_loss

# Optional timing hook (bench.py): when set to a list, an eager step appends recorded HIP events
# bracketing the Adam launch (adam_step_slots) on the current stream.
EVENT_HOOK = None
# Same for the table-gradient scatter (hashgrid_bwd_pairs), the step's second-largest kernel.
BWD_HOOK = None

ALIGN = 128                # pair segment alignment = one MLP round (4 tiles x 32 slots)
# The tables' share of the clip norm from the scatter's returning atomics (acn_hashgrid_bwd_pairs_sumsq)
# instead of a pass over the K x 128 MiB gradient buffers
TELESCOPED_TABLE_NORM = os.environ.get("ACN_TELE_NORM", "1") != "0"
# The background head's forward / backward as two HIP launches (acn_background_fwd / _bwd) instead of the
# ~15 torch launches of its autograd graph
FUSED_BACKGROUND = os.environ.get("ACN_FUSED_BG", "1") != "0"
# Segment maps of the table gradients: the scatter marks the 64-B segments it adds into, and the Adam pass skips
# segments never touched (m = v = g = 0: bit-identical under torch's Adam with weight_decay 0) and reads no
# gradient for segments not touched this step
ADAM_SEGMAP = os.environ.get("ACN_ADAM_SEGMAP", "1") != "0"
# Split segment-mapped Adam: the early pass (segments touched before but not by this step) on a side stream
# beside the step's forward / backward, the late pass after the clip coefficient (the two passes
# contend for HBM with the step's own kernels: C5 1.75 -> 2.0 ms, so it stays off)
ADAM_EARLY = os.environ.get("ACN_ADAM_EARLY", "0") != "0"   # measured slower: off
# The compositing glue of the step in one launch (acn_routed_composite_mse_train: blend, background forward,
# compositing, the linear MSE and the backward of all three down to the pair outputs) instead of eight launches
# and a copy; same arithmetic for every gradient (per-element; tests/test_routed_glue.py compares them bitwise).  The
# loss is a double sum whose order differs (per ray per workgroup here, element-strided in mse_linear_fwd_ws): it is
# equal after the float cast at the tested sizes, not by construction
FUSED_COMPOSITE = os.environ.get("ACN_FUSED_COMPOSITE", "1") != "0"


def draw_jitter(n: int, S: int, device) -> torch.Tensor:
    """The training jitter of one step: stratified_t_vals' rand_like of the (n, S) t grid
    (nerfs/ray_rendering.py:262-287), graph-safe philox under capture."""
    return torch.rand(n, S, device=device)


# the jitter source of jitter='draw' steps (tests substitute a recorded stream)
JITTER = draw_jitter


def _stream(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def check_routed_config(name: str, model, optimizer) -> None:
    """The configuration the routed steps train; ``name``: the class the caller built (its messages)."""
    if not isinstance(model, MetaContainer) or not all(s._fusable for s in model.submodules):
        raise AcnError(f"{name}: a MetaContainer of reference-configuration experts is required")
    if not isinstance(optimizer, FusedAdam):
        raise AcnError(f"{name} needs FusedAdam")
    if not model.use_bg_nerf:
        raise AcnError(f"{name}: the background head is part of the reference configuration")
    encs = [s.xyz_encoder for s in model.submodules]
    e0 = encs[0]
    if any(e._res_host != e0._res_host or e.log2_hashmap_size != e0.log2_hashmap_size
           or e._interp_code != e0._interp_code for e in encs) or e0._interp_code == 0:
        raise AcnError(f"{name}: experts must share one Linear/Smoothstep hash-grid configuration")


class ExpertBank:
    """The training state of the experts ``own`` of a checked container (check_routed_config) -- slot j is expert
    own[j]; range(K) on one GPU, a rank's experts in the expert-parallel step -- and of the shared background
    head (slot E): the persistent gradient buffers behind every parameter's .grad, the ctypes arguments of the
    pair kernels, SlottedAdam's slot_of / flags / grads, and the launches the two routed steps share.
    ``flat_head``: the head's gradients as views of one buffer ``gbg_flat`` (one all-reduce) instead of a tensor
    per parameter."""

    def __init__(self, model, optimizer, own, mlp_precision: str, grad_clip: Optional[float], clear_in_adam: bool,
                 flat_head: bool = False):
        self.model, self.opt, self.own, self.mlp_precision = model, optimizer, list(own), mlp_precision
        subs = [model.submodules[k] for k in self.own]
        encs = [s.xyz_encoder for s in subs]
        self.enc = e0 = encs[0]   # every expert's hash-grid configuration
        E = self.E = len(subs)
        dev = self.device = e0.hash_table.device
        self.tele = TELESCOPED_TABLE_NORM and grad_clip is not None
        # ---- persistent gradients (every parameter's .grad is one of these buffers)
        self.gtables = [torch.zeros_like(e.hash_table) for e in encs]
        self.dw = torch.zeros(E, ops.MLP_DW_FLOATS, device=dev, dtype=torch.float32)
        self.bg_params = list(model.bg_mlp.parameters())
        if flat_head:
            self.gbg_flat = torch.zeros(sum(p.numel() for p in self.bg_params), device=dev, dtype=torch.float32)
            self.gbg = [g.view_as(p) for g, p in zip(self.gbg_flat.split([p.numel() for p in self.bg_params]),
                                                     self.bg_params)]
        else:
            self.gbg = [torch.zeros_like(p) for p in self.bg_params]
        try:   # (acn_background, the tensors it points into)
            self.bg_spec, self._bg_keep = model.background_spec() if FUSED_BACKGROUND else (None, None)
        except AcnError:
            self.bg_spec, self._bg_keep = None, None
        # ---- SlottedAdam's arguments: the tables are cleared by the Adam pass and, telescoped, normed by the scatter
        table_flags = (ZERO_GRAD_FLAG if clear_in_adam else 0) | (NORM_ELSEWHERE_FLAG if self.tele else 0)
        self.slot_of, self.flags = {}, {}
        for j, (sub, enc) in enumerate(zip(subs, encs)):
            enc.hash_table.grad = self.gtables[j]
            self.slot_of[id(enc.hash_table)] = j
            self.flags[id(enc.hash_table)] = table_flags
            views, o = [], 0
            for shp in ops.MLP_DW_SHAPES:
                n = int(np.prod(shp))
                views.append(self.dw[j, o:o + n].view(shp))
                o += n
            for t, g in zip(sub._mlp_tensors(None).values(), views):
                t.grad = g
                self.slot_of[id(t)] = j
        for p, g in zip(self.bg_params, self.gbg):
            p.grad = g
            self.slot_of[id(p)] = E
        self.grads = {id(p): p.grad for p in model.parameters() if id(p) in self.slot_of}
        # ---- the pair kernels' host arguments
        self._mlp_structs = [ops._mlp_struct(list(s._mlp_tensors(None).values())) for s in subs]
        self._mlp_ptrs = (C.POINTER(acn_mlp) * E)(*[C.pointer(w) for w in self._mlp_structs])
        self._tables = (C.c_void_p * E)(*[e.hash_table.data_ptr() for e in encs])
        self._gtables = (C.c_void_p * E)(*[g.data_ptr() for g in self.gtables])
        self._res = (C.c_int32 * len(e0._res_host))(*e0._res_host)
        # (resolutions, levels, log2 table size, interpolation): the hash-grid arguments of every pair kernel
        self.grid = (self._res, len(e0._res_host), e0.log2_hashmap_size, e0._interp_code)
        boxes = [s._host_box() for s in subs]
        self._mins = (C.c_float * (3 * E))(*[float(v) for b in boxes for v in b[0]])
        self._exts = (C.c_float * (3 * E))(*[float(v) for b in boxes for v in b[1]])
        lo = np.float32(1e-6)
        self._lo, self._hi = C.c_float(lo), C.c_float(np.float32(1.0) - lo)
        self.routing = model.routing_spec()

    def slotted_adam(self, **kw) -> SlottedAdam:
        """The clip + Adam pass over the bank's slots (optim.SlottedAdam)."""
        return SlottedAdam(self.opt, self.slot_of, self.grads, self.E, self.E + 1, self.flags, **kw)

    def _mfn(self, name: str):
        return ops.mlp_fn(name, self.mlp_precision)

    def forward(self, x01, pk, seg, sh, h0, out, mws) -> None:
        """h0 of every pair slot through its expert's table, then the E expert MLPs (weights packed from the live
        parameters into ``mws``) -> ``out``; on the current stream."""
        L = _lib.lib()
        s = _stream(self.device)
        check(L.acn_hashgrid_fwd_pairs(ptr(x01), ptr(pk), ptr(seg), self.E, self._tables, *self.grid, ptr(h0), s),
              "acn_hashgrid_fwd_pairs")
        check(self._mfn("acn_mlp_pack_pairs")(self._mlp_ptrs, self.E, ptr(mws), s), "acn_mlp_pack_pairs")
        check(self._mfn("acn_mlp_train_fwd_pairs")(ptr(h0), ptr(sh), ptr(seg), self.E, ptr(mws), ptr(out), s),
              "acn_mlp_train_fwd_pairs")

    def backward_mlp(self, h0, sh, out, gout, seg, mws, gh0) -> None:
        """From dL/d(pair outputs) ``gout``: the experts' [dW | db] into ``dw`` (the MLP .grad views) and dL/dh0
        into ``gh0`` for the caller's table scatter; on the current stream."""
        check(self._mfn("acn_mlp_train_bwd_dw_pairs")(ptr(h0), ptr(sh), ptr(out), ptr(gout), ptr(seg), self.E, ptr(mws),
                                                      ptr(self.dw), ptr(gh0), _stream(self.device)),
              "acn_mlp_train_bwd_dw_pairs")


class RoutedAdaptStep:
    """One runtime_adapt update of a MetaContainer (routed, no active_module) per call.

    ``graph=True``: the first ``warmup`` calls run eagerly -- real updates on the caller's real batches --
    and the step is then captured once (the capture itself runs nothing) and replayed for every later
    full batch of ``n_rays`` rays.  A smaller batch (a loader's ragged last batch) runs eagerly through the
    same buffers.  ``jitter='draw'`` draws the training jitter inside the step like the reference, a
    caller-supplied (n, S) tensor per call otherwise (``jitter='given'``, for fixture replays)."""

    def __init__(self, P, model, n_rays: int, optimizer: FusedAdam, grad_clip: Optional[float] = 1.0,
                 graph: bool = True, warmup: int = 1, max_steps: int = 1 << 16, jitter: str = "draw",
                 clear_in_adam: bool = True):
        check_routed_config("RoutedAdaptStep", model, optimizer)
        self.P, self.model, self.opt = P, model, optimizer
        self.mlp_precision = ops.TRAIN_MLP_PRECISION   # training MLP kernels (ops.set_train_mlp_precision)
        self.grad_clip = grad_clip
        self.jitter_mode = jitter
        # clear_in_adam=False keeps the gradients readable after the step (tests): the table gradients
        # are then zeroed at the start of the next step instead of by the Adam pass
        self.clear_in_adam = bool(clear_in_adam)
        K = len(model.submodules)
        # the experts' gradients, kernel arguments and shared launches: all K experts are differentiated here
        self.bank = bank = ExpertBank(model, optimizer, range(K), self.mlp_precision, grad_clip, self.clear_in_adam)
        self.tele, self.gtables, self.dw = bank.tele, bank.gtables, bank.dw
        dev = self.device = bank.device
        # use_amp (ops.set_train_mlp_precision("amp")): the autocast(fp16) MLP arithmetic plus GradScaler --
        # the loss gradient enters the backward multiplied by the device loss scale, Adam unscales / skips
        self.amp = AmpScaler(dev) if self.mlp_precision == "amp" else None
        S = int(P.ray_samples)
        N = int(n_rays)
        M = N * S
        cap = M * K + K * ALIGN
        self.K, self.N, self.S, self.M, self.cap = K, N, S, M, cap
        f32 = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        L = _lib.lib()
        # ---- static inputs / pair buffers
        self.rays = torch.zeros(N, 8, **f32)
        self.rgbs = torch.zeros(N, 3, **f32)
        self.u = torch.zeros(N, S, **f32)
        self.t = torch.empty(N, S, **f32)
        self.seg = torch.zeros(2 * K + 1, device=dev, dtype=torch.int64)
        self.rws = torch.empty(int(L.acn_routed_workspace_bytes(M, K)), device=dev, dtype=torch.uint8)
        self.pidx = torch.empty(cap, **i32)
        self.pw = torch.empty(cap, **f32)
        self.pk = torch.empty(cap, **i32)
        self.x01 = torch.empty(cap, 3, **f32)
        self.sh = torch.empty(cap, 16, **f32)
        self.pmap = torch.empty(M, K, **i32)
        self.h0 = torch.empty(cap, 32, **f32)
        self.out = torch.empty(cap, 4, **f32)
        self.gh0 = torch.empty(cap, 32, **f32)
        self.mws = torch.empty(int(ops.mlp_fn("acn_mlp_pairs_workspace_bytes", self.mlp_precision)(K)), device=dev,
                               dtype=torch.uint8)
        self.loss = torch.zeros((), **f32)
        self._one = torch.ones((), **f32)          # dL/dL of the explicit loss backward
        self.dirs = torch.zeros(N, 3, **f32)
        self.rgb = torch.zeros(N, 3, **f32)
        self.g_bg = torch.zeros(N, 3, **f32)
        self.gout = torch.zeros(cap, 4, **f32)
        self.cws = torch.zeros(int(L.acn_composite_mse_train_workspace_bytes()), device=dev, dtype=torch.uint8)
        # segment maps: (K, 2, segments) bytes -- [k, 0] touched this step, [k, 1] touched before.  A table whose
        # moments may already be non-zero (optimizer state from earlier steps) starts all "touched before".
        self.segmaps = None
        smap = {}
        if ADAM_SEGMAP:
            tables = [s.xyz_encoder.hash_table for s in model.submodules]
            self.segmaps = torch.zeros(K, 2, tables[0].numel() // 16, device=dev, dtype=torch.uint8)
            for k, table in enumerate(tables):
                st = optimizer.state.get(table)
                if st and float(st.get("step", 0)) > 0:
                    self.segmaps[k, 1].fill_(1)
                smap[id(table)] = (self.segmaps[k, 0], self.segmaps[k, 1])
            self._segnow = (C.c_void_p * K)(*[self.segmaps[k, 0].data_ptr() for k in range(K)])
        # ---- slotted clip + Adam over every parameter of the optimizer's groups (optim.SlottedAdam)
        self.adam = bank.slotted_adam(max_steps=max_steps, segmaps=smap)
        self.rows, self.flags, self.step_dev = self.adam.rows, self.adam.flags, self.adam.step_dev
        self.nslots, self.table_steps, self._step0 = self.adam.nslots, self.adam.table_steps, self.adam.step0
        self.scale = self.adam.scale
        self.table_sumsq = torch.zeros(1, device=dev, dtype=torch.float64)  # reset by grad_sumsq_slots_ex
        # split Adam (ADAM_EARLY): the table segments a step does not touch but earlier steps did (~40-60% of the
        # segment-mapped bytes) are updated on a side stream while the step's forward / backward runs -- their
        # gradient is zero, so they need no clip coefficient; the late pass updates the touched segments and the
        # dense tensors.  Not with use_amp (a found_inf skip is decided after the backward).
        self.early = ADAM_EARLY and self.segmaps is not None and self.amp is None
        if self.early:
            self.side = torch.cuda.Stream(dev)
        self.replays = 0          # graph replays
        self.steps_done = 0       # every update this object ran (eager and replayed): Adam table rows used
        self.graph = None
        self._params = [r[0] for r in self.rows]
        self._eager_left = max(1, int(warmup)) if graph else 0   # eager real steps before the capture

    def _capture(self) -> None:
        """Record the full-batch step into one HIP graph (nothing executes; the static buffers keep their
        contents)."""
        dev = self.device
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with graph_capture(g):
            self._step(self.N)
        torch.cuda.synchronize(dev)
        self.graph = g

    # ------------------------------------------------------------------------------------------
    def _step(self, n: Optional[int] = None) -> None:
        L = _lib.lib()
        dev, K, S, b = self.device, self.K, self.S, self.bank
        N = self.N if n is None else int(n)
        M = N * S
        s = _stream(dev)
        if not self.clear_in_adam:
            for g in self.gtables:
                g.zero_()
        u, t = self.u[:N], self.t[:N]
        if self.jitter_mode == "draw":   # the reference's rand_like(low) draw
            if JITTER is draw_jitter:
                torch.rand(N, S, device=dev, out=u)   # straight into the step's buffer (no copy launch)
            else:
                u.copy_(JITTER(N, S, dev))
        check(L.acn_routed_count(ptr(self.rays), N, S, ptr(u), C.byref(b.routing), ALIGN, ptr(t),
                                 ptr(self.seg), ptr(self.rws), self.rws.numel(), s), "acn_routed_count")
        check(L.acn_routed_scatter(ptr(self.rays), N, S, K, ptr(t), ptr(self.seg), C.cast(b._mins, C.c_void_p),
                                   C.cast(b._exts, C.c_void_p), b._lo, b._hi, ALIGN, ptr(self.rws),
                                   ptr(self.pidx), ptr(self.pw), ptr(self.x01), ptr(self.sh), ptr(self.pmap),
                                   ptr(self.pk), s), "acn_routed_scatter")
        capturing = torch.cuda.is_current_stream_capturing()   # no timing events inside a capture
        det = torch.are_deterministic_algorithms_enabled()
        ev_early = None
        if self.early and not det:
            # fork: the step's now[] marks from its pair list, then Adam's early pass, on the side stream
            main = torch.cuda.current_stream(dev)
            ev0 = torch.cuda.Event()
            ev0.record(main)
            self.side.wait_event(ev0)
            with torch.cuda.stream(self.side):
                self._mark(int(self.side.cuda_stream))
                self.adam.step_early(self.seg, hook=EVENT_HOOK if self.graph is None and not capturing else None)
                ev_early = torch.cuda.Event()
                ev_early.record(self.side)
        b.forward(self.x01, self.pk, self.seg, self.sh, self.h0, self.out, self.mws)
        rays, rgbs, dirs = self.rays[:N], self.rgbs[:N], self.dirs[:N]
        linear = str(self.P.color_space).lower() == "linear"
        if FUSED_COMPOSITE and b.bg_spec is not None and linear and S <= 1024:   # S: the kernel's LDS rows
            check(L.acn_routed_composite_mse_train(
                ptr(rays), N, S, ptr(t), ptr(self.out), ptr(self.pw), ptr(self.pmap), K, ptr(self.pidx), self.cap,
                ptr(self.seg[K:K + 1]), C.byref(b.bg_spec), ptr(rgbs), ptr(self._one if self.amp is None
                                                                         else self.amp.scale),
                ptr(self.rgb), ptr(dirs), ptr(self.g_bg), ptr(self.gout), ptr(self.loss), ptr(self.cws),
                self.cws.numel(), s), "acn_routed_composite_mse_train")
            ops.background_bwd(dirs, b.bg_spec, self.g_bg[:N], b.gbg)
            self._experts_bwd(self.gout, det, capturing, ev_early)
            return
        rs = ops.routed_blend_fwd(self.out, self.pw, self.pmap[:M]).view(N, S, 4).requires_grad_(True)
        # the shared part: compositing, colour transform and MSE under torch autograd (HIP kernels); the
        # background head as its fused HIP forward and backward (writing the persistent .grad buffers), or
        # under autograd when the head is not the HIP-supported SH-4 MLP
        if b.bg_spec is not None and linear:
            # the kernels autograd would run (compositing, the linear-space MSE and their backwards), called
            # directly: no ones-fill for the loss gradient, no autograd bookkeeping launches
            dirs.copy_(rays[:, 3:6])
            rs_ = rs.detach()
            bg = ops.background_fwd(dirs, b.bg_spec)
            rgb = ops.volume_render(rs_, t, bg)[0]
            loss = ops.mse_linear_fwd(rgb, rgbs, out=self.loss)
            g_rgb = ops.mse_linear_bwd(rgb, rgbs, self._one if self.amp is None else self.amp.scale)
            g_rs, g_bg = ops.volume_render_bwd(rs_, t, bg, 1.0, g_rgb, None, None, None)
            ops.background_bwd(dirs, b.bg_spec, g_bg, b.gbg)
        elif b.bg_spec is not None:
            dirs.copy_(rays[:, 3:6])
            bg = ops.background_fwd(dirs, b.bg_spec).requires_grad_(True)
            with torch.enable_grad():
                rgb = volume_render(rs, t, bg_rgb=bg)[0]
                loss = mse_color_loss(rgb, rgbs, self.P.color_space)
                g_rs, g_bg = torch.autograd.grad(loss if self.amp is None else loss * self.amp.scale, [rs, bg])
            ops.background_bwd(dirs, b.bg_spec, g_bg, b.gbg)
        else:
            with torch.enable_grad():
                bg = self.model.background_color(rays[:, 3:6])
                rgb = volume_render(rs, t, bg_rgb=bg)[0]
                loss = mse_color_loss(rgb, rgbs, self.P.color_space)
                grads = torch.autograd.grad(loss if self.amp is None else loss * self.amp.scale, [rs] + b.bg_params)
            g_rs = grads[0]
            for g, buf in zip(grads[1:], b.gbg):
                buf.copy_(g)
        if loss is not self.loss:
            self.loss.copy_(loss.detach())
        gout = ops.routed_blend_bwd(g_rs.reshape(M, 4).contiguous(), self.pidx, self.pw, live=self.seg[K:K + 1])
        self._experts_bwd(gout, det, capturing, ev_early)

    def _mark(self, s: int) -> None:
        """Write the step's now[] segment marks from its pair list, on stream ``s``: for the paths whose table
        backward does not mark them itself (the early Adam pass, the deterministic backward)."""
        check(_lib.lib().acn_hashgrid_pairs_mark(ptr(self.x01), ptr(self.pk), ptr(self.pidx), ptr(self.seg), self.K,
                                                 *self.bank.grid, self._segnow, s), "acn_hashgrid_pairs_mark")

    def _experts_bwd(self, gout: torch.Tensor, det: bool, capturing: bool, ev_early) -> None:
        """From dL/d(pair outputs): the experts' MLP [dW | db] and table gradients, then clip + Adam."""
        L = _lib.lib()
        dev, K, b = self.device, self.K, self.bank
        s = _stream(dev)
        b.backward_mlp(self.h0, self.sh, self.out, gout, self.seg, self.mws, self.gh0)
        bhook = BWD_HOOK if self.graph is None and not capturing else None
        if bhook is not None:
            b0 = torch.cuda.Event(enable_timing=True)
            b0.record()
        if det:
            self._table_bwd_deterministic(b.enc)
            if self.segmaps is not None:   # the sort-based backward marks no segments: the marks on their own
                self._mark(s)
                if self.early:   # the same two passes, in sequence
                    self.adam.step_early(self.seg, hook=EVENT_HOOK if self.graph is None and not capturing else None)
        else:
            # the marks came from the side stream (early) or come with the scatter
            check(L.acn_hashgrid_bwd_pairs_segmap(ptr(self.x01), ptr(self.pk), ptr(self.pidx), ptr(self.seg), K,
                                                  ptr(self.gh0), b._gtables, *b.grid,
                                                  ptr(self.table_sumsq) if self.tele else None,
                                                  self._segnow if self.segmaps is not None and not self.early
                                                  else None, s),
                  "acn_hashgrid_bwd_pairs_segmap")
        if bhook is not None:
            b1 = torch.cuda.Event(enable_timing=True)
            b1.record()
            bhook.append((b0, b1))
        if ev_early is not None:
            torch.cuda.current_stream(dev).wait_event(ev_early)   # join
        self.adam.step(self.seg, self.grad_clip, self.table_sumsq if self.tele else None,
                       hook=EVENT_HOOK if self.graph is None and not capturing else None, amp=self.amp,
                       phase=2 if self.early else 0)

    def _table_bwd_deterministic(self, enc) -> None:
        """Under torch.use_deterministic_algorithms(True): every expert's table gradient by the sort-based
        backward over its live pairs (acn_hashgrid_bwd_det: each row the serial fp32 sum of its contributions
        in pair order = sample order, bitwise reproducible) instead of float atomics, and the tables' share of
        the clip norm by a deterministic double reduction.  Reads the segment table to the host: eager only
        (a graph-replayed step runs this eagerly instead, __call__)."""
        if torch.cuda.is_current_stream_capturing():
            raise AcnError("RoutedAdaptStep: deterministic mode cannot be captured (it reads the pair counts)")
        K = self.K
        seg = self.seg.cpu().tolist()
        for k in range(K):
            s0, n = int(seg[k]), int(seg[K + 1 + k])
            if n:
                ops.hashgrid_bwd(self.x01[s0:s0 + n], self.gh0[s0:s0 + n], enc._res_host, enc.log2_hashmap_size, 2,
                                 enc._interp_code, deterministic=True, out=self.gtables[k])
        if self.tele:
            tot = torch.zeros((), device=self.device, dtype=torch.float64)
            for g in self.gtables:
                tot = tot + (g.double() ** 2).sum()
            self.table_sumsq.copy_(tot.view(1))

    def __call__(self, rays: torch.Tensor, rgbs: torch.Tensor, jitter_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = int(rays.shape[0])
        if rays.dim() != 2 or rays.shape[1] != 8 or tuple(rgbs.shape) != (n, 3) or not 0 < n <= self.N:
            raise AcnError(f"RoutedAdaptStep was built for batches of up to {self.N} rays; got {tuple(rays.shape)}, "
                           f"{tuple(rgbs.shape)}")
        # every update, eager or replayed, consumes one row of the Adam constant table (per-slot device
        # counters never run ahead of the number of updates)
        if self._step0 + self.steps_done + 1 > self.table_steps:
            raise AcnError("RoutedAdaptStep: the Adam constant table is exhausted; build a new step object")
        self.rays[:n].copy_(rays, non_blocking=True)
        self.rgbs[:n].copy_(rgbs, non_blocking=True)
        if self.jitter_mode == "given":
            if jitter_u is None or tuple(jitter_u.shape) != (n, self.S):
                raise AcnError(f"RoutedAdaptStep(jitter='given') needs jitter_u of shape ({n}, {self.S}) per call")
            self.u[:n].copy_(jitter_u, non_blocking=True)
        det = torch.are_deterministic_algorithms_enabled()   # eager: the deterministic table backward
        if n == self.N and self.graph is not None and not det:
            self.graph.replay()
            self.replays += 1
        else:
            self._step(n)
            if n == self.N and self._eager_left > 0 and not det:
                self._eager_left -= 1
                if self._eager_left == 0:
                    self._capture()
        self.steps_done += 1
        bump_versions(self._params)  # the kernels wrote them: packed render images are stale
        return self.loss

    @property
    def last_norm(self) -> torch.Tensor:
        """(total_norm, clip coefficient) of the last step (device), as FusedAdam.last_norm."""
        return self.scale

    def segment_stats(self):
        """(segments touched by the last step's scatter, segments ever updated, segments in all tables), from
        the maps after a step (the last step's marks are in 'ever' once its Adam pass ran).  Host read."""
        if self.segmaps is None:
            return None
        ever = int(self.segmaps[:, 1].sum())
        return ever, int(self.segmaps[:, 1].numel())

    def segment_line_stats(self):
        """128-B lines (two adjacent 64-B segments) of the tables holding at least one ever-updated segment:
        what the segment-mapped Adam's reads fetch if HBM lines are filled whole.  Host read."""
        if self.segmaps is None:
            return None
        ev = self.segmaps[:, 1]
        pairs = ev[:, : ev.shape[1] // 2 * 2].reshape(ev.shape[0], -1, 2)
        return int((pairs.amax(dim=2) != 0).sum())

    def sync_state(self) -> None:
        """Host state['step'] of every parameter from the per-slot device counters (state_dict, or before
        an eager FusedAdam step on the same optimizer)."""
        self.adam.sync_state()

    def load_state(self) -> None:
        """Per-slot device step counters from the optimizer's host state['step'] (after eager FusedAdam
        steps taken on the same optimizer outside this object), and the Adam constants from the current
        group hyper-parameters."""
        before = self.adam.step_dev.cpu().tolist()
        top = self.adam.load_state()
        self.adam.refresh()
        if self.segmaps is not None:
            # an eager step on slot k (runtime_adapt(active_module=k), or the eager routed step) may have moved
            # any row of table k: every segment of a table whose slot counter changed counts as touched, so the
            # segment-mapped Adam keeps decaying its moments
            after = self.adam.step_dev.cpu().tolist()
            for k in range(self.K):
                if after[k] != before[k]:
                    self.segmaps[k, 1].fill_(1)
        self._step0 = top - self.steps_done   # keeps the exhaustion guard exact
