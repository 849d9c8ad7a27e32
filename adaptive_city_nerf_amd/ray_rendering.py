"""Stratified volumetric rendering (reference interface: nerfs/ray_rendering.py:23-345, 564-627).

``render_rays`` / ``render_rays_stratified`` / ``render_image`` / ``volume_render`` keep the
reference's signatures and return values.  Without autograd (eval, rendering, viewer) a whole
``render_rays`` call is ONE fused HIP launch (acn_render_stratified_fwd): t-values -> points ->
routing -> every needed expert's hash grid + MLPs on fp32 MFMA -> soft blend -> background ->
front-to-back compositing; the (N,S,4) field output and the (N*S,6) point table the reference
materialises never exist.  With autograd (training) the call composes the differentiable
per-expert forward (HIP hash grid + fast-weight MetaLinear chain) with the reference's
compositing formulas.

Extensions (not in the reference): ``early_stop_tau`` (default 0 = off) stops a ray once its
transmittance drops below tau; the composite then differs from the reference by at most 2*tau.
``jitter_u`` (N, S) supplies the uniforms of the training-mode jitter (the reference draws them
with torch.rand_like, ray_rendering.py:286) so a training step can be reproduced exactly.
"""
from __future__ import annotations

import os
import threading
import warnings
from contextlib import contextmanager
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import nerfacc, occ_ops, ops
from ._lib import acn_routing
from .encodings import wants_grad
from .meta_container import MetaContainer
from .meta_ngp import MetaNGP
from .ray_sampling import clamp_rays_near_far, get_ray_directions, get_rays  # noqa: F401  (re-export)
from .trunc_exp import trunc_exp

_LINSPACE_CACHE = {}
_GRAPH_MODE = threading.local()


@contextmanager
def second_order(enabled: bool = True):
    """Within this context, differentiable renders build twice-differentiable graphs (second-order
    MAML: meta_core.py:57 takes ``autograd.grad(create_graph=True)`` of the inner loss): the
    compositing runs as torch ops instead of the HIP forward/backward pair, and a hash grid evaluated
    here has a differentiable point gradient.  Thread-local."""
    prev = getattr(_GRAPH_MODE, "second_order", False)
    _GRAPH_MODE.second_order = bool(enabled)
    try:
        yield
    finally:
        _GRAPH_MODE.second_order = prev


def _second_order() -> bool:
    return getattr(_GRAPH_MODE, "second_order", False)


@contextmanager
def encoding_frozen(enabled: bool = True):
    """Within this context, differentiable single-expert renders evaluate the hash grid without autograd:
    for first-order inner loops (FOMAML / Reptile task_adapt, meta_core.py:14-67), which differentiate
    w.r.t. the fast MLP weights only, the encoding's backward branch (dL/dh0, the table scatter) is dead
    work (the values are unchanged).  The shared background head, not a fast weight either, then runs as
    its fused HIP launch (values within fp32 rounding of the torch chain).  Thread-local."""
    prev = getattr(_GRAPH_MODE, "frozen_encoding", False)
    _GRAPH_MODE.frozen_encoding = bool(enabled)
    try:
        yield
    finally:
        _GRAPH_MODE.frozen_encoding = prev


@contextmanager
def inner_loop_background_cache():
    """Within this context (one first-order task_adapt call), frozen-encoding renders reuse the background
    head's output for rays they have already rendered: the head is not a fast weight and the support rays do
    not change between inner steps, so steps 2..n would recompute the same values (a strided-directions
    copy and a background launch per step).  Entries hold their rays tensor (compared by identity) and end
    with the context.  Only the model's background head is cached ('random' backgrounds are re-drawn per
    render, as in the reference).  Thread-local."""
    prev = getattr(_GRAPH_MODE, "bg_cache", None)
    _GRAPH_MODE.bg_cache = {}
    try:
        yield
    finally:
        _GRAPH_MODE.bg_cache = prev


# Training renders (the differentiable single-expert path: meta inner loops and queries, active_module
# adaptation) visit their rays in direction-cell order (ray_order_kernel, the order render_kernel uses for
# C2): the hash grid's gathers and scatter then see spatially coherent 32-sample tiles.  Every per-ray value is
# computed exactly as before and the outputs are returned in the caller's order, so losses are unchanged; only
# the MLP weight-gradient sums run in another order.  Measured slower on the meta step (66.1 -> 69.2 ms: the
# order launch and the permutations cost more than the gathers gain at 4000-ray tasks), so it
# is off by default; ACN_TRAIN_ORDER=1 turns it on.
TRAIN_RAY_ORDER = os.environ.get("ACN_TRAIN_ORDER", "0") != "0"
_ORDER_MAX = 8192   # ray_order_kernel's single-workgroup limit (ACN_ORDER_MAX)


def _train_order(rays: Tensor):
    """(order, inverse) int64 permutations of ``rays`` by direction cell, through the inner-loop cache when open
    (the support rays are rendered at every inner step)."""
    cache = getattr(_GRAPH_MODE, "bg_cache", None)
    key = ("order", id(rays))
    if cache is not None:
        hit = cache.get(key)
        if hit is not None and hit[0] is rays and hit[1] == rays._version:
            return hit[2], hit[3]
    N = rays.shape[0]
    o32 = torch.empty(N, dtype=torch.int32, device=rays.device)
    from ._lib import check, lib, ptr
    r = rays.contiguous()
    check(lib().acn_ray_order(ptr(r), N, ptr(o32), int(torch.cuda.current_stream(rays.device).cuda_stream)),
          "acn_ray_order")
    order = o32.long()
    inv = torch.empty_like(order)
    inv[order] = torch.arange(N, device=rays.device)
    if cache is not None:
        cache[key] = (rays, rays._version, order, inv)
    return order, inv


def _frozen_background(model, rays, params, rgb_sigma, N, bg_color_default):
    """The background of a frozen-encoding render (no autograd), through the inner-loop cache when open."""
    cache = getattr(_GRAPH_MODE, "bg_cache", None)
    if cache is None or not getattr(model, "use_bg_nerf", False):
        return _get_bg_rgb(model, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
    key = (id(model), id(rays))
    hit = cache.get(key)
    if hit is not None and hit[0] is rays and hit[1] == rays._version:
        return hit[2]
    bg = _get_bg_rgb(model, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
    cache[key] = (rays, rays._version, bg)
    return bg


# ============================== BG helpers ===============================
def _get_bg_rgb(model, dirs: Tensor, params, rgb_sigma_or_map, N: int, bg_color_default: str) -> Optional[Tensor]:
    """Background RGB: the model's background head if it has one, else a default colour (:23-45)."""
    if getattr(model, "use_bg_nerf", False):
        return model.background_color(dirs)
    return get_bg_default_color(rgb_sigma_or_map, N, bg_color_default)


def get_bg_default_color(rgb_sigma, N: int, bg_color: str = "white") -> Optional[Tensor]:
    device = None if rgb_sigma is None else rgb_sigma.device
    dtype = None if rgb_sigma is None else rgb_sigma.dtype
    if bg_color == "none":
        return None
    if bg_color == "white":
        return torch.ones(N, 3, device=device, dtype=dtype)
    if bg_color == "black":
        return torch.zeros(N, 3, device=device, dtype=dtype)
    if bg_color == "random":
        return torch.rand(N, 3, device=device, dtype=dtype)
    if bg_color == "last_sample":
        if rgb_sigma is None or rgb_sigma.dim() != 3 or rgb_sigma.size(-1) < 3:
            raise ValueError("bg_color='last_sample' requires rgb_sigma of shape (N,S,4) or (N,S,>=3).")
        return rgb_sigma[:, -1, :3]
    raise ValueError(f"Unknown background policy: {bg_color}")


def apply_bg_mask(rgb_lin: Tensor, mask_invalid: Tensor, policy: str) -> None:
    if not mask_invalid.any():
        return
    policy = str(policy).lower()
    if policy == "white":
        rgb_lin[mask_invalid] = 1.0
    elif policy == "black":
        rgb_lin[mask_invalid] = 0.0
    elif policy == "random":
        n = int(mask_invalid.sum().item())
        rgb_lin[mask_invalid] = torch.rand(n, 3, device=rgb_lin.device, dtype=rgb_lin.dtype)
    elif policy in ("none", "last_sample"):
        pass
    else:
        rgb_lin[mask_invalid] = 1.0


# ============================== Core volume rendering ===============================
def _volume_render_autograd(rgb_sigma, t_vals, bg_rgb, raw_rgb, raw_sigma, sigma_scale):
    """Differentiable compositing, same formulas as ray_rendering.py:137-165 (training path)."""
    rgb = torch.sigmoid(rgb_sigma[..., :3]) if raw_rgb else rgb_sigma[..., :3].clamp(0.0, 1.0)
    sigma = trunc_exp(rgb_sigma[..., 3]) if raw_sigma else rgb_sigma[..., 3].clamp_min(0.0)
    if sigma_scale != 1.0:
        sigma = sigma * float(sigma_scale)
    dists = (t_vals[:, 1:] - t_vals[:, :-1]).clamp_min(1e-4)
    dists = torch.cat([dists, dists[:, -1:]], dim=1)
    alpha = (1.0 - torch.exp(-sigma * dists)).clamp(0.0, 1.0 - 1e-7)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], dim=1), dim=1)[:, :-1]
    weights = alpha * T
    rgb_map = (weights.unsqueeze(-1) * rgb).sum(dim=1)
    depth_map = (weights * t_vals).sum(dim=1)
    acc_map = weights.sum(dim=1)
    if bg_rgb is not None:
        rgb_map = rgb_map + (1.0 - acc_map.unsqueeze(-1)) * bg_rgb.to(rgb_map.device, dtype=rgb_map.dtype)
    return rgb_map, depth_map, weights, acc_map


class _VolumeRenderFn(torch.autograd.Function):
    """volume_render with HIP forward (acn_volume_render_fwd) and backward (acn_volume_render_bwd):
    two kernels instead of the ~40 elementwise/scan/reduction launches of the autograd graph."""

    @staticmethod
    def forward(ctx, rgb_sigma, t_vals, bg_rgb, sigma_scale):
        rgb, depth, w, acc = ops.volume_render(rgb_sigma, t_vals, bg_rgb, sigma_scale=sigma_scale)
        # outputs the loss does not use (depth, weights, acc in training) reach backward as None: the
        # kernel treats a NULL output gradient as zero, so autograd need not zero-fill them (3 launches)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(rgb_sigma, t_vals, bg_rgb)
        ctx.sigma_scale = sigma_scale
        return rgb, depth, w, acc

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_w, g_acc):
        rgb_sigma, t_vals, bg_rgb = ctx.saved_tensors
        g_rs, g_bg = ops.volume_render_bwd(rgb_sigma, t_vals, bg_rgb, ctx.sigma_scale, g_rgb, g_depth, g_w, g_acc)
        return (g_rs if ctx.needs_input_grad[0] else None, None,
                g_bg if (bg_rgb is not None and ctx.needs_input_grad[2]) else None, None)


def volume_render(rgb_sigma: Tensor, t_vals: Tensor, bg_rgb: Optional[Tensor] = None, *, raw_rgb: bool = False,
                  raw_sigma: bool = False, sigma_scale: float = 1.0, **kwargs) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """NeRF compositing: rgb (N,3), depth (N,), weights (N,S), acc (N,) (ray_rendering.py:114-165)."""
    if torch.is_grad_enabled() and (rgb_sigma.requires_grad or (bg_rgb is not None and bg_rgb.requires_grad)):
        if rgb_sigma.is_cuda and not raw_rgb and not raw_sigma and rgb_sigma.dtype == torch.float32 \
                and not _second_order():
            bg = None if bg_rgb is None else bg_rgb.to(rgb_sigma.device, torch.float32)
            return _VolumeRenderFn.apply(rgb_sigma, t_vals, bg, float(sigma_scale))
        return _volume_render_autograd(rgb_sigma, t_vals, bg_rgb, raw_rgb, raw_sigma, sigma_scale)
    out = ops.volume_render(rgb_sigma, t_vals, bg_rgb, raw_rgb=raw_rgb, raw_sigma=raw_sigma, sigma_scale=sigma_scale)
    return tuple(o.to(rgb_sigma.dtype) for o in out)


# ============================== Stratified rendering ===============================
def _t_lin(S: int, device) -> Tensor:
    """torch.linspace(0,1,S) evaluated on the CPU (the reference's device) then moved."""
    key = (S, str(device))
    if key not in _LINSPACE_CACHE:
        _LINSPACE_CACHE[key] = torch.linspace(0.0, 1.0, S).to(device)
    return _LINSPACE_CACHE[key]


@torch.no_grad()
def stratified_t_vals(near: Tensor, far: Tensor, ray_samples: int, randomized: bool = True,
                      u: Optional[Tensor] = None) -> Tensor:
    """S uniform depths in [near, far], jittered within midpoints when randomized (:262-287).
    ``u`` optionally supplies the (N,S) uniforms of the jitter (for reproducible training)."""
    t_lin = _t_lin(ray_samples, near.device).unsqueeze(0)
    t_vals = near.unsqueeze(1) * (1.0 - t_lin) + far.unsqueeze(1) * t_lin
    if randomized:
        mids = 0.5 * (t_vals[:, :-1] + t_vals[:, 1:])
        low = torch.cat([t_vals[:, :1], mids], dim=1)
        high = torch.cat([mids, t_vals[:, -1:]], dim=1)
        t_vals = low + (high - low) * (torch.rand_like(low) if u is None else u)
    return t_vals


FUSED_TRAIN_SAMPLER = True  # tests switch it off to compare with the composed chain
ROUTED_TRAIN = True         # differentiable routed-container renders on the pair kernels (routed.hip)
ENC_EPS = 1e-6  # MetaNGP.enc_eps (a constant fp32 buffer, meta_ngp.py:155-158), known on the host


def _train_expert(model, active_module):
    """The single MetaNGP a differentiable render evaluates (container + active_module, or a bare
    MetaNGP), when it is the fused configuration; else None."""
    sub = model.submodules[active_module] if isinstance(model, MetaContainer) and active_module is not None else (
        model if isinstance(model, MetaNGP) else None)
    return sub if sub is not None and sub._fusable else None


class _BlendFn(torch.autograd.Function):
    """MetaContainer.forward's weighted index_add_ over experts (meta_container.py:300-337) on the
    (sample, expert) pairs: y (P,4) -> (M,4); backward dY_p = dY_m * w_p."""

    @staticmethod
    def forward(ctx, y, pw, pmap, pidx):
        ctx.save_for_backward(pw, pidx)
        return ops.routed_blend_fwd(y, pw, pmap)

    @staticmethod
    def backward(ctx, g):
        pw, pidx = ctx.saved_tensors
        return ops.routed_blend_bwd(g.contiguous(), pidx, pw), None, None, None


def _routed_train_ok(model, rays, active_module) -> bool:
    return (ROUTED_TRAIN and isinstance(model, MetaContainer) and active_module is None and rays.is_cuda
            and rays.dtype == torch.float32 and all(s._fusable for s in model.submodules) and not _second_order())


def _render_routed(model, rays: Tensor, S: int, params, u: Optional[Tensor], bg_color_default: str, sigma_scale,
                   return_t_vals: bool = False):
    """Differentiable render of the routed container (training / runtime_adapt, ray_rendering.py:290-345
    over MetaContainer.forward :275-343): routing + per-expert pair lists on the GPU (routed.hip, one
    host sync for the segment sizes), per expert the HIP hash grid (autograd to its table) and the fused
    MLP, the weighted blend in expert order, HIP compositing.  Experts no sample reaches get no
    gradient at all (grad None), as in the reference's loop."""
    N = rays.shape[0]
    if model.training and u is None:
        u = torch.rand_like(rays.new_empty(N, S))  # the reference's rand_like(low) draw
    boxes = [sub._host_box() for sub in model.submodules]
    t_vals, starts, pidx, pw, x01, sh, pmap = ops.routed_pairs(
        rays.contiguous(), S, u if model.training else None, model.routing_spec(), [b[0] for b in boxes],
        [b[1] for b in boxes], ENC_EPS)
    from .meta_ngp import _FusedMLPFn
    sub_params = model._sub_params(params)
    outs = []
    for k, sub in enumerate(model.submodules):
        a, b = starts[k], starts[k + 1]
        if b == a:
            continue
        h0 = sub.xyz_encoder(x01[a:b])
        ws = [t.contiguous() for t in sub._mlp_tensors(sub_params[k]).values()]
        outs.append(_FusedMLPFn.apply(h0.contiguous(), sh[a:b], *ws))
    y = torch.cat(outs, 0) if len(outs) > 1 else (outs[0] if outs else rays.new_zeros(0, 4))
    rgb_sigma = _BlendFn.apply(y, pw, pmap, pidx).view(N, S, 4)
    bg_rgb = _get_bg_rgb(model, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
    out = volume_render(rgb_sigma, t_vals, bg_rgb=bg_rgb, raw_rgb=False, raw_sigma=False, sigma_scale=sigma_scale)
    return out + (t_vals,) if return_t_vals else out


def _fused_experts(model, params, active_module, render_table: bool = False):
    """(specs, routing, packed weights) for the fused kernels, or None if the model/config is not fusable.
    render_table: the stratified render, which also serves the experts' fp16 render tables
    (set_render_table_dtype); the occupancy renderers keep the fp32 tables."""
    if isinstance(model, MetaContainer):
        if not all(s._fusable for s in model.submodules):
            return None
        if active_module is not None:
            sub = model.submodules[active_module]
            if sub.uses_grad(params):
                return None
            r = acn_routing()
            r.K, r.cluster_2d, r.boundary_margin = 1, 1, 1.0
            spec = sub.expert_spec(params, render_table=render_table)
            return [spec], r, sub.packed_weights(spec, r, params)
        if model.uses_grad(params):
            return None
        specs, routing = model.expert_specs(params, render_table=render_table), model.routing_spec()
        return specs, routing, model.packed_weights(specs, routing, None, params)
    if isinstance(model, MetaNGP):
        if not model._fusable or model.uses_grad(params):
            return None
        r = acn_routing()
        r.K, r.cluster_2d, r.boundary_margin = 1, 1, 1.0
        spec = model.expert_spec(params, render_table=render_table)
        return [spec], r, model.packed_weights(spec, r, params)
    return None


def _fused_background(model, bg_color_default: str, N: int, device):
    """(acn_background, keep) or None when the policy needs the composed path."""
    if getattr(model, "use_bg_nerf", False):
        if torch.is_grad_enabled() and any(p.requires_grad for p in model.bg_mlp.parameters()):
            return None
        return model.background_spec()
    if bg_color_default == "white":
        return ops.make_background("const", color=(1.0, 1.0, 1.0))
    if bg_color_default == "black":
        return ops.make_background("const", color=(0.0, 0.0, 0.0))
    if bg_color_default == "none":
        return ops.make_background("none")
    return None  # "random" / "last_sample": composed path


def render_rays_stratified(model, rays: Tensor, ray_samples: int, params=None, active_module: Optional[int] = None,
                           bg_color_default: str = "white", chunk: int = 1_000_000, sigma_scale=1.0,
                           return_t_vals: bool = False, **kwargs):
    """Stratified renderer: rgb (N,3), depth (N,), weights (N,S), acc (N,) (:290-345).

    ``return_t_vals`` (an extension) appends the (N,S) sample depths the weights belong to, in the caller's ray
    order, as a fifth value: what ``distortion_loss`` needs next to the weights.

    Rays that require grad take the composed path (no fused render, sampler or routed pair kernels): the
    gradient reaches the origins and directions, ``rays[:, :6]``, through the sample points, the field's
    HIP input gradients and the compositing.  ``stratified_t_vals`` is a no-grad function, so the t-values
    are constants: the near / far columns get a zero gradient."""
    diff_rays = wants_grad(rays)
    tau = float(kwargs.get("early_stop_tau", 0.0))
    want_weights = bool(kwargs.get("_want_weights", True))  # render_image drops the (N,S) weights
    N = rays.shape[0]
    if rays.is_cuda and not diff_rays:
        fe = _fused_experts(model, params, active_module, render_table=True)
        fb = _fused_background(model, bg_color_default, N, rays.device) if fe is not None else None
        if fe is not None and fb is not None:
            specs, routing, packed = fe
            bg, keep = fb
            jitter = None
            if model.training:
                ju = kwargs.get("jitter_u")
                jitter = ju.to(rays.device, torch.float32).contiguous() if ju is not None else \
                    torch.rand(N, ray_samples, device=rays.device)
            rgb, depth, w, acc = ops.render_stratified(rays, ray_samples, specs, routing,
                                                       0 if len(specs) == 1 else None, bg,
                                                       sigma_scale=float(sigma_scale), tau=tau, jitter=jitter,
                                                       packed=packed, want_weights=want_weights)
            out = (rgb.to(rays.dtype), depth.to(rays.dtype), None if w is None else w.to(rays.dtype),
                   acc.to(rays.dtype))
            if return_t_vals:   # the kernel keeps its t values in registers: the same jitter through the torch form
                out += (stratified_t_vals(rays[:, 6], rays[:, 7], ray_samples, randomized=model.training, u=jitter),)
            return out
    sub = _train_expert(model, active_module) if FUSED_TRAIN_SAMPLER and not diff_rays else None
    if sub is not None and rays.is_cuda and rays.dtype == torch.float32 and sub._fused_train_ok(rays):
        # differentiable single-expert path (training, inner loops): one sampler launch (t-values,
        # unit-box points, SH), the HIP hash grid under autograd and the fused MLP -- the same values
        # as the composed chain below
        from .meta_ngp import _FusedMLPFn
        u = kwargs.get("jitter_u")
        if model.training and u is None:
            u = torch.rand_like(rays.new_empty(N, ray_samples))  # the reference's rand_like(low) draw
        mn, ext = sub._host_box()
        rays_in = rays
        order = None
        if TRAIN_RAY_ORDER and 1 < N <= _ORDER_MAX:
            order, inv = _train_order(rays)
            rays = rays.index_select(0, order)
            if u is not None:
                u = u.to(rays.device).index_select(0, order)
        t_vals, x01, sh = ops.sample_stratified(rays, ray_samples, u if model.training else None, mn, ext,
                                                ENC_EPS)
        if getattr(_GRAPH_MODE, "frozen_encoding", False):
            with torch.no_grad():
                h0 = sub.xyz_encoder(x01)
        else:
            h0 = sub.xyz_encoder(x01)
        ws = [t.contiguous() for t in sub._mlp_tensors(params).values()]
        rgb_sigma = _FusedMLPFn.apply(h0.contiguous(), sh, *ws).view(N, ray_samples, 4)
        # the background of the caller's rays (cached per rays tensor), then in the visiting order
        if getattr(_GRAPH_MODE, "frozen_encoding", False):
            with torch.no_grad():  # nor is the shared background head a fast weight: one fused HIP launch
                bg_rgb = _frozen_background(model, rays_in, params, rgb_sigma, N, bg_color_default)
        else:
            bg_rgb = _get_bg_rgb(model, rays_in[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
        last_sample = not getattr(model, "use_bg_nerf", False) and bg_color_default == "last_sample"
        if order is not None and not last_sample and bg_rgb is not None and torch.is_tensor(bg_rgb) \
                and bg_rgb.dim() == 2 and bg_rgb.shape[0] == N:
            bg_rgb = bg_rgb.index_select(0, order)   # (last_sample reads the visiting-order samples already)
        out = volume_render(rgb_sigma, t_vals, bg_rgb=bg_rgb, raw_rgb=False, raw_sigma=False,
                            sigma_scale=sigma_scale)
        if return_t_vals:
            out += (t_vals,)
        if order is None:
            return out
        return tuple(None if x is None else x.index_select(0, inv) for x in out)   # the caller's order
    if not diff_rays and _routed_train_ok(model, rays, active_module):
        return _render_routed(model, rays, ray_samples, params, kwargs.get("jitter_u"), bg_color_default,
                              sigma_scale, return_t_vals)
    # composed (differentiable) path -- same structure as the reference
    o, d = rays[:, :3], rays[:, 3:6]
    near, far = rays[:, 6], rays[:, 7]
    t_vals = stratified_t_vals(near, far, ray_samples, randomized=model.training, u=kwargs.get("jitter_u"))
    pts = o.unsqueeze(1) + d.unsqueeze(1) * t_vals.unsqueeze(-1)
    dirs = d.unsqueeze(1).expand_as(pts)
    id6 = torch.cat([pts, dirs], dim=-1).reshape(-1, 6)
    model_eff = model.submodules[active_module] if active_module is not None else model
    outs = [model_eff(id6[s: s + chunk], params=params) for s in range(0, id6.shape[0], chunk)]
    rgb_sigma = torch.cat(outs, dim=0).view(pts.shape[0], pts.shape[1], 4)
    bg_rgb = _get_bg_rgb(model, dirs[:, 0], params, rgb_sigma, N=rgb_sigma.size(0), bg_color_default=bg_color_default)
    out = volume_render(rgb_sigma, t_vals, bg_rgb=bg_rgb, raw_rgb=False, raw_sigma=False, sigma_scale=sigma_scale)
    return out + (t_vals,) if return_t_vals else out


# ============================== Occupancy rendering (Soft MoE) ===============================
@torch.no_grad()
def _intersect_rays_aabb(rays: Tensor, scene_box) -> Tensor:
    """(N,) bool: the ray's [near, far] interval meets the box (ray_rendering.py:170-193)."""
    o, d = rays[:, :3], rays[:, 3:6]
    near, far = rays[:, 6:7], rays[:, 7:8]
    eps = 1e-9
    invd = torch.where(torch.abs(d) > eps, 1.0 / d, torch.full_like(d, 1.0 / eps))
    t0 = (scene_box.min.to(rays.device)[None, :] - o) * invd
    t1 = (scene_box.max.to(rays.device)[None, :] - o) * invd
    tmin = torch.minimum(t0, t1).amax(dim=-1, keepdim=True)
    tmax = torch.maximum(t0, t1).amin(dim=-1, keepdim=True)
    return (torch.minimum(tmax, far) > torch.maximum(tmin, near)).squeeze(-1)


@torch.no_grad()
def _merge_segments_union(ray_indices_list, t0_list, t1_list):
    """Per ray, the sorted distinct boundaries of every expert's segments; consecutive pairs become
    the merged segments (ray_rendering.py:196-258).  One HIP K-way merge per ray."""
    if len(t0_list) == 0:
        dev = torch.device("cpu")
        return (torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev))
    n_rays = int(max(int(r.max().item()) for r in ray_indices_list if r.numel()) + 1) \
        if any(r.numel() for r in ray_indices_list) else 0
    lists = []
    for ri, t0, t1 in zip(ray_indices_list, t0_list, t1_list):
        order = torch.argsort(ri, stable=True)  # each list must be ray-major (marching output already is)
        ri, t0, t1 = ri[order], t0[order], t1[order]
        pi = nerfacc.pack_info(ri, n_rays)
        lists.append((pi[:, 0], pi[:, 1], t0, t1))
    mri, m0, m1, _, _ = occ_ops.union(lists, n_rays)
    return mri, m0, m1


def _bg_or_default(model, d, params, rgb_map, N, bg_color_default):
    return _get_bg_rgb(model, d, params, rgb_map, N, bg_color_default)


def _empty_occ_result(model, rays, d, params, N, bg_color_default):
    acc = rays.new_zeros(N)
    bg_rgb = _get_bg_rgb(model, d, params, None, N, bg_color_default)
    if bg_rgb is not None:
        bg_rgb = bg_rgb.to(rays.device)
    weights = torch.zeros(1, 1, device=rays.device, dtype=rays.dtype)
    return bg_rgb, acc.clone(), weights, acc


def _no_ray_grad(rays: Tensor) -> None:
    if wants_grad(rays):
        raise ops.AcnError("the occupancy renderer has no gradient for its rays (marching is a no-grad step); "
                           "differentiate rays through render_rays_stratified")


def _composite_packed(model, rays, d, params, ri, t0, t1, starts, counts, sigma, rgb, t_mid, N, bg_color_default):
    """nerfacc compositing of packed samples under autograd (training path)."""
    if _second_order():
        raise ops.AcnError("second-order (create_graph) gradients through the occupancy renderer are not "
                           "supported (nerfacc's scan backward is first order too)")
    packed = torch.stack([starts, counts], -1)
    weights = nerfacc.render_weight_from_density(t_starts=t0, t_ends=t1, sigmas=sigma, packed_info=packed)[0][..., None]
    w1 = weights.squeeze(-1)
    rgb_map = nerfacc.accumulate_along_rays(w1, rgb, ri, N)
    depth = nerfacc.accumulate_along_rays(w1, t_mid[:, None], ri, N).squeeze(-1)
    acc = nerfacc.accumulate_along_rays(w1, None, ri, N).squeeze(-1)
    bg_rgb = _get_bg_rgb(model, d, params, rgb_map, N, bg_color_default)
    rgb_map = rgb_map + (1.0 - acc)[..., None] * bg_rgb.to(rgb_map.device, rgb_map.dtype)
    return rgb_map, depth, weights, acc


def render_expert_occ(model, rays: Tensor, *, params=None, bg_color_default: str = "white", chunk: int = 1_000_000,
                      render_step_size=None, alpha_thre=None, cone_angle=None, **kwargs):
    """One expert over its occupancy grid: rgb (N,3), depth (N,), weights (M,1), acc (N,)
    (ray_rendering.py:467-558).  Eval: marching + ONE fused HIP render over the packed samples."""
    _no_ray_grad(rays)
    N = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:6]
    if getattr(model, "occ_grid", None) is None:
        return None
    ri, t0, t1, starts, counts = model._occupancy_marching_packed(
        rays, params=params, render_step_size=render_step_size, alpha_thre=alpha_thre, cone_angle=cone_angle)
    if t0.numel() == 0:
        return _empty_occ_result(model, rays, d, params, N, bg_color_default)
    if rays.is_cuda:
        fe = _fused_experts(model, params, None)
        fb = _fused_background(model, bg_color_default, N, rays.device) if fe is not None else None
        if fe is not None and fb is not None:
            specs, routing, packed = fe
            bg, keep = fb
            rgb, depth, w, acc = occ_ops.render_packed(rays, starts, counts, t0, t1, specs, routing, 0, bg,
                                                       packed=packed)
            return rgb.to(rays.dtype), depth.to(rays.dtype), w.to(rays.dtype)[:, None], acc.to(rays.dtype)
    t_mid = 0.5 * (t0 + t1)
    x = o[ri] + d[ri] * t_mid[:, None]
    ds = d[ri]
    outs = [model(torch.cat([x[s:s + chunk], ds[s:s + chunk]], dim=-1), params=params)
            for s in range(0, x.shape[0], chunk)]
    out = torch.cat(outs, 0)
    return _composite_packed(model, rays, d, params, ri, t0, t1, starts, counts, out[:, 3], out[:, :3], t_mid, N,
                             bg_color_default)


def render_rays_occ(model, rays: Tensor, *, params=None, bg_color_default: str = "white", chunk: int = 1_000_000,
                    render_step_size=None, alpha_thre=None, cone_angle=None, active_module: Optional[int] = None,
                    **kwargs):
    """Occupancy-guided soft Mixture-of-Experts renderer (ray_rendering.py:349-464): per expert,
    AABB prefilter + marching over its grid; per-ray boundary union; experts evaluated at the
    midpoints where their routing weight exceeds 1e-8; sigma and rgb blended BEFORE one nerfacc
    integration.  Eval runs marching (HIP), union (HIP) and ONE fused render launch.

    The reference routes the midpoints with ``model._routing(x_mid.view(1, -1, 3))``, which its own
    ``_routing`` rejects (``assert pts.dim() == 2``, meta_container.py:111), so its container path
    raises AssertionError whenever it runs; this build routes the (M, 3) midpoints, the evident
    intent (documented in DESIGN.md)."""
    _no_ray_grad(rays)
    N = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:6]
    if active_module is not None:
        sub = model.submodules[active_module]
        return render_expert_occ(sub, rays, params=params, bg_color_default=bg_color_default, chunk=chunk,
                                 render_step_size=render_step_size, alpha_thre=alpha_thre, cone_angle=cone_angle)
    K = len(model.submodules)
    training = any(sub.training for sub in model.submodules)
    lists, any_samples = [], False
    for k, expert in enumerate(model.submodules):
        p_k = model.get_subdict(params, f"submodules.{k}") if params is not None else None
        box = [float(v) for v in torch.cat([expert.scene_box.min, expert.scene_box.max]).tolist()]
        if training:  # subset marching, exactly like the reference (the jitter draws one uniform per hit ray)
            hit = _intersect_rays_aabb(rays, expert.scene_box)
            hit_idx = hit.nonzero(as_tuple=False).squeeze(1)
            if hit_idx.numel() == 0:
                continue
            ri_k, t0_k, t1_k, _, _ = expert._occupancy_marching_packed(
                rays[hit_idx], params=p_k, render_step_size=render_step_size, alpha_thre=alpha_thre,
                cone_angle=cone_angle)
            if t0_k.numel() == 0:
                continue
            g = hit_idx[ri_k]
            pi = nerfacc.pack_info(g, N)
            lists.append((pi[:, 0], pi[:, 1], t0_k, t1_k))
        else:  # eval: the prefilter runs inside the traversal kernel over all rays
            ri_k, t0_k, t1_k, st_k, ct_k = expert._occupancy_marching_packed(
                rays, params=p_k, render_step_size=render_step_size, alpha_thre=alpha_thre, cone_angle=cone_angle,
                prefilter_aabb=box)
            if t0_k.numel() == 0:
                continue
            lists.append((st_k, ct_k, t0_k, t1_k))
        any_samples = True
    if not any_samples:
        return _empty_occ_result(model, rays, d, params, N, bg_color_default)
    mri, m0, m1, mst, mct = occ_ops.union(lists, N)
    if m0.numel() == 0:
        return _empty_occ_result(model, rays, d, params, N, bg_color_default)
    if rays.is_cuda:
        fe = _fused_experts(model, params, None)
        fb = _fused_background(model, bg_color_default, N, rays.device) if fe is not None else None
        if fe is not None and fb is not None:
            specs, routing, packed = fe
            bg, keep = fb
            rgb, depth, w, acc = occ_ops.render_packed(rays, mst, mct, m0, m1, specs, routing,
                                                       0 if K == 1 else None, bg, packed=packed)
            return rgb.to(rays.dtype), depth.to(rays.dtype), w.to(rays.dtype)[:, None], acc.to(rays.dtype)
    # composed (differentiable) path -- the reference's structure
    M = m0.numel()
    t_mid = 0.5 * (m0 + m1)
    x_mid = o[mri] + d[mri] * t_mid[:, None]
    d_mid = d[mri]
    with torch.no_grad():
        W, hard = model._routing(x_mid.view(-1, 3))
        if W is None:
            W = x_mid.new_zeros(M, K)
            W[torch.arange(M, device=W.device), hard.view(-1)] = 1.0
    eps = 1e-8
    SIG = x_mid.new_zeros(M, K)
    RGB = x_mid.new_zeros(M, K, 3)
    for k, expert in enumerate(model.submodules):
        mask = W[:, k] > eps
        if not mask.any():
            continue
        idx = torch.nonzero(mask, as_tuple=False).squeeze(1)
        xb, db = x_mid[idx], d_mid[idx]
        p_k = model.get_subdict(params, f"submodules.{k}") if params is not None else None
        sig_l, rgb_l = [], []
        for s in range(0, idx.numel(), chunk):
            out = expert(torch.cat([xb[s:s + chunk], db[s:s + chunk]], dim=-1), params=p_k)
            rgb_l.append(out[..., :3])
            sig_l.append(out[..., 3])
        SIG = SIG.index_put((idx, torch.full_like(idx, k)), torch.cat(sig_l, 0))
        RGB = RGB.index_put((idx, torch.full_like(idx, k)), torch.cat(rgb_l, 0))
    s_num = (W * SIG).sum(dim=1, keepdim=True).clamp_min(1e-12)
    sigma_mix = s_num.squeeze(1)
    rgb_mix = (W[..., None] * SIG[..., None] * RGB).sum(dim=1) / s_num
    return _composite_packed(model, rays, d, params, mri, m0, m1, mst, mct, sigma_mix, rgb_mix, t_mid, N,
                             bg_color_default)


# ============================== Hierarchical (coarse to fine) rendering ===============================
FUSED_RESAMPLE = True   # sample_pdf on acn_resample_pdf; tests switch it off to take the torch chain


def _sample_pdf_torch(t_vals: Tensor, weights: Tensor, n_importance: int, jitter: Optional[Tensor] = None):
    """(t_fine, t_merged) of sample_pdf as torch ops: acn_resample_pdf's definition in float64, every depth rounded to
    fp32 once (CPU tensors, other dtypes, rows beyond the kernel's limits)."""
    N, S = t_vals.shape
    F = int(n_importance)
    t, w = t_vals.detach().double(), weights.detach().double()
    b = (t[:, :-1] + t[:, 1:]) / 2                                        # (N, S-1) edges
    c = torch.cat([t.new_zeros(N, 1), torch.cumsum(w[:, 1:-1] + 1e-5, dim=1)], dim=1)   # (N, S-1), not normalised
    r = 0.5 if jitter is None else jitter.detach().to(t.device, torch.float64)
    v = ((torch.arange(F, device=t.device, dtype=torch.float64)[None, :] + r) / F) * c[:, -1:]
    v = v.expand(N, F).contiguous()
    k = (torch.searchsorted(c[:, :-1].contiguous(), v, right=True) - 1).clamp(0, S - 3)
    c0, c1 = torch.gather(c, 1, k), torch.gather(c, 1, k + 1)
    b0, b1 = torch.gather(b, 1, k), torch.gather(b, 1, k + 1)
    den = c1 - c0
    f = torch.where(den > 0, (v - c0) / den, torch.zeros_like(v)).clamp(0.0, 1.0)
    t_fine = (b0 + f * (b1 - b0)).float().to(t_vals.dtype)
    t_merged = torch.sort(torch.cat([t_vals.detach(), t_fine], dim=1), dim=1, stable=True).values
    return t_fine, t_merged


def _points6(rays: Tensor, t: Tensor) -> Tensor:
    """The (N*S, 6) rows [o + d t, d] the model's forward takes (the composed path's expression)."""
    o, d = rays[:, :3], rays[:, 3:6]
    pts = o.unsqueeze(1) + d.unsqueeze(1) * t.unsqueeze(-1)
    return torch.cat([pts, d.unsqueeze(1).expand_as(pts)], dim=-1).reshape(-1, 6)


@torch.no_grad()
def sample_pdf(t_vals: Tensor, weights: Tensor, n_importance: int, jitter: Optional[Tensor] = None, *,
               return_merged: bool = False, rays: Optional[Tensor] = None):
    """Classic NeRF's importance resampling: ``n_importance`` new depths per ray, (N, F), drawn by the inverse CDF of
    the piecewise-constant density that ``weights[:, 1:-1] + 1e-5`` puts on the bins between the midpoints of
    ``t_vals`` (both (N, S >= 3): the weights and t values of ``render_rays_stratified(..., return_t_vals=True)``), at
    the stratified quantiles (j + jitter[n, j]) / F; ``jitter`` (N, F) in [0, 1), None = 0.5 (deterministic).  The
    depths are non-decreasing along a ray and lie between the first and the last midpoint.

    ``return_merged`` also returns the (N, S + F) sorted union with ``t_vals`` (a coarse sample before an equal fine
    one), what ``volume_render`` and ``distortion_loss`` take; ``rays`` (N, 8), an extension, appends the
    (N * (S + F), 6) rows [o + d t, d] of the merged depths and implies ``return_merged``.

    No gradient: the weights are detached and the outputs are constants, as every t value here.  HIP fp32 tensors with
    S <= 1024 and F <= 1024 take one launch (acn_resample_pdf: float64 arithmetic, one fp32 rounding per depth);
    everything else the same definition as torch ops."""
    if t_vals.dim() != 2 or t_vals.shape[1] < 3 or weights.shape != t_vals.shape:
        raise ops.AcnError(f"sample_pdf: t_vals and weights must both be (N, S >= 3), got {tuple(t_vals.shape)} and "
                           f"{tuple(weights.shape)}")
    F = int(n_importance)
    if F < 1:
        raise ops.AcnError(f"sample_pdf: n_importance must be >= 1, got {n_importance}")
    N, S = t_vals.shape
    if jitter is not None and tuple(jitter.shape) != (N, F):
        raise ops.AcnError(f"sample_pdf: jitter must be ({N}, {F}), got {tuple(jitter.shape)}")
    if rays is not None and (rays.dim() != 2 or rays.shape[0] != N or rays.shape[1] < 8):
        raise ops.AcnError(f"sample_pdf: rays must be ({N}, >=8), got {tuple(rays.shape)}")
    fused = (FUSED_RESAMPLE and t_vals.is_cuda and t_vals.dtype == torch.float32 and weights.dtype == torch.float32
             and S <= ops.RESAMPLE_MAX_S and F <= ops.RESAMPLE_MAX_F and (rays is None or rays.dtype == torch.float32))
    if fused:
        jit = None if jitter is None else jitter.to(t_vals.device)
        t_fine, t_merged, pts6 = ops.resample_pdf(weights, t_vals, F, jitter=jit,
                                                  rays=None if rays is None else rays.detach()[:, :8],
                                                  want_points=rays is not None)
    else:
        t_fine, t_merged = _sample_pdf_torch(t_vals, weights, F, jitter)
        pts6 = None if rays is None else _points6(rays.detach(), t_merged)
    if rays is not None:
        return t_fine, t_merged, pts6
    return (t_fine, t_merged) if return_merged else t_fine


FUSED_FINE_RENDER = True   # render_rays_hierarchical's fine pass on render_rays_at's fused launch;
                           # tests switch it off to take the composed chain


def _f16_render_tables(model) -> bool:
    """An expert of the model renders from an fp16 table (set_render_table_dtype): its no-grad forward then reads
    that table, which the explicit-depth kernels do not."""
    subs = model.submodules if isinstance(model, MetaContainer) else [model]
    return any(getattr(getattr(s, "xyz_encoder", None), "render_table_dtype", torch.float32) == torch.float16
               for s in subs)


def _fused_depths(model, rays: Tensor, t_vals: Tensor, params, active_module, bg_color_default: str):
    """(specs, routing, packed, background, keep) when a render at the depths ``t_vals`` can take the fused launch
    (ops.render_depths), else None: render_rays_stratified's conditions, fp32 depths and fp32 hash tables."""
    if not (rays.is_cuda and t_vals.is_cuda and t_vals.dtype == torch.float32) or wants_grad(rays):
        return None
    if _f16_render_tables(model):
        return None
    fe = _fused_experts(model, params, active_module)
    fb = _fused_background(model, bg_color_default, rays.shape[0], rays.device) if fe is not None else None
    if fe is None or fb is None:
        return None
    return fe + tuple(fb)


def _render_depths_fused(rays: Tensor, t_vals: Tensor, fd, sigma_scale, tau: float):
    specs, routing, packed, bg, keep = fd
    rgb, depth, w, acc = ops.render_depths(rays, t_vals, specs, routing, 0 if len(specs) == 1 else None, bg,
                                           sigma_scale=float(sigma_scale), tau=tau, packed=packed)
    return rgb.to(rays.dtype), depth.to(rays.dtype), w.to(rays.dtype), acc.to(rays.dtype)


def _check_depths(rays: Tensor, t_vals: Tensor, what: str) -> None:
    N = rays.shape[0]
    if t_vals.dim() != 2 or t_vals.shape[0] != N or t_vals.shape[1] < 2:
        raise ops.AcnError(f"{what}: t_vals must be ({N}, S >= 2), got {tuple(t_vals.shape)}")
    if t_vals.device != rays.device:
        raise ops.AcnError(f"{what}: t_vals is on {t_vals.device}, the rays on {rays.device}")


def render_rays_at(model, rays: Tensor, t_vals: Tensor, params=None, active_module: Optional[int] = None,
                   bg_color_default: str = "white", chunk: int = 1_000_000, sigma_scale=1.0,
                   early_stop_tau: float = 0.0):
    """The stratified renderer at the caller's depths (an extension): sample s of ray n at ``t_vals[n, s]``, (N, S >= 2)
    and non-decreasing along a ray, instead of the near..far linspace; near / far of the rays are not used.  Returns
    rgb (N,3), depth (N,), weights (N,S), acc (N,).

    HIP rays that do not require grad, fp32 depths and a model render_rays_stratified would render fused (no fast
    weights that need grad, a background the kernel evaluates, no fp16 render table) take one launch
    (ops.render_depths; ``early_stop_tau`` as in render_rays_stratified).  Everything else is the composed chain --
    the points o + d t, the model's forward in ``chunk`` pieces, the background and ``volume_render`` -- which is also
    the differentiable form (model parameters, fast weights, ray origins and directions).  ``t_vals`` is a constant:
    it never carries a gradient.  The depths are not validated: a NaN or unsorted row spoils that ray only."""
    _check_depths(rays, t_vals, "render_rays_at")
    t_vals = t_vals.detach()
    fd = _fused_depths(model, rays, t_vals, params, active_module, bg_color_default)
    if fd is not None:
        return _render_depths_fused(rays, t_vals, fd, sigma_scale, float(early_stop_tau))
    N, S = t_vals.shape
    id6 = _points6(rays, t_vals)
    model_eff = model.submodules[active_module] if active_module is not None else model
    outs = [model_eff(id6[s: s + chunk], params=params) for s in range(0, id6.shape[0], chunk)]
    rgb_sigma = torch.cat(outs, dim=0).view(N, S, 4)
    bg_rgb = _get_bg_rgb(model, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
    return volume_render(rgb_sigma, t_vals, bg_rgb=bg_rgb, raw_rgb=False, raw_sigma=False, sigma_scale=sigma_scale)


def render_rays_hierarchical(model, rays: Tensor, ray_samples: int, n_importance: int, params=None,
                             active_module: Optional[int] = None, bg_color_default: str = "white", sigma_scale=1.0,
                             return_coarse: bool = False, return_t_vals: bool = False, **kwargs):
    """Coarse-to-fine stratified renderer (classic NeRF): a coarse pass of ``ray_samples`` depths
    (render_rays_stratified), ``n_importance`` further depths per ray where the coarse weights are (sample_pdf), and the
    model evaluated once more on the S + F merged depths.  Returns the fine pass: rgb (N,3), depth (N,), weights
    (N, S+F), acc (N,).

    The coarse pass runs without autograd (in eval mode it is the fused render) unless ``return_coarse``, which
    appends its differentiable (rgb, depth, weights, acc) as one tuple, for the coarse-plus-fine loss.
    ``return_t_vals`` appends the merged (N, S+F) depths last (``distortion_loss(weights, t_merged, rays)``).  The
    resampling carries no gradient.  In training mode the fine quantiles are jittered by ``jitter_fine`` (N, F) or
    torch.rand; in eval mode they are the bin centres.  ``jitter_u``, ``early_stop_tau`` and ``chunk`` go to the coarse
    pass as in render_rays_stratified.  Rays that require grad are differentiated through the fine pass's points.

    A fine pass that needs no gradient (render_rays_at's conditions for its fused launch) is that one launch at the
    merged depths, without a point table, unless FUSED_FINE_RENDER is off; otherwise it is the composed chain."""
    F = int(n_importance)
    if F < 1:
        raise ops.AcnError(f"render_rays_hierarchical: n_importance must be >= 1, got {n_importance}")
    if int(ray_samples) < 3:
        raise ops.AcnError(f"render_rays_hierarchical: the coarse pass needs ray_samples >= 3, got {ray_samples}")
    chunk = int(kwargs.pop("chunk", 1_000_000))
    jitter_fine = kwargs.pop("jitter_fine", None)
    kwargs.pop("_want_weights", None)   # the resampling needs the coarse weights whatever the caller keeps
    N = rays.shape[0]
    with torch.enable_grad() if return_coarse and torch.is_grad_enabled() else torch.no_grad():
        coarse = render_rays_stratified(model, rays, ray_samples, params=params, active_module=active_module,
                                        bg_color_default=bg_color_default, chunk=chunk, sigma_scale=sigma_scale,
                                        return_t_vals=True, **kwargs)
    w_c, t_c = coarse[2].detach(), coarse[4].detach()
    jitter = None
    if model.training:
        jitter = jitter_fine if jitter_fine is not None else torch.rand(N, F, device=rays.device)
    fd = _fused_depths(model, rays, t_c, params, active_module, bg_color_default) if FUSED_FINE_RENDER else None
    if fd is not None:   # the fine pass in one launch at the merged depths: no point table (render_rays_at)
        _, t_merged = sample_pdf(t_c, w_c, F, jitter, return_merged=True)
        out = _render_depths_fused(rays, t_merged, fd, sigma_scale, 0.0)
        if return_coarse:
            out += (tuple(coarse[:4]),)
        return out + (t_merged,) if return_t_vals else out
    if wants_grad(rays):   # the points carry the rays' gradient: the torch expression, not the kernel's constants
        _, t_merged = sample_pdf(t_c, w_c, F, jitter, return_merged=True)
        id6 = _points6(rays, t_merged)
    else:
        _, t_merged, id6 = sample_pdf(t_c, w_c, F, jitter, rays=rays)
    model_eff = model.submodules[active_module] if active_module is not None else model
    outs = [model_eff(id6[s: s + chunk], params=params) for s in range(0, id6.shape[0], chunk)]
    rgb_sigma = torch.cat(outs, dim=0).view(N, t_merged.shape[1], 4)
    bg_rgb = _get_bg_rgb(model, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default=bg_color_default)
    out = volume_render(rgb_sigma, t_merged, bg_rgb=bg_rgb, raw_rgb=False, raw_sigma=False, sigma_scale=sigma_scale)
    if return_coarse:
        out += (tuple(coarse[:4]),)
    return out + (t_merged,) if return_t_vals else out


# ============================== Proposal-guided rendering (mip-NeRF 360) ===============================
FUSED_INTERLEVEL = True   # interlevel_loss on acn_interlevel_loss; tests switch it off to take the
                          # torch chain


def _edges64(t: Tensor) -> Tensor:
    """(N, S + 1) float64 interval edges of (N, S >= 2) depths: e_i = t_i, e_S = t_{S-1} + (t_{S-1} - t_{S-2})."""
    t = t.double()
    return torch.cat([t, t[:, -1:] + (t[:, -1:] - t[:, -2:-1])], dim=1)


def _interlevel_torch(t_vals: Tensor, weights: Tensor, t_prop: Tensor, w_prop: Tensor,
                      ray_scale: Optional[Tensor] = None, eps: float = 2.0 ** -23) -> Tensor:
    """(N,) interlevel loss as torch ops: acn_interlevel_loss's O(S + P) form with float64 scans and searches (CPU
    tensors, other dtypes than fp32, rows beyond the kernel's limits, and inside second_order(): differentiable any
    number of times in ``w_prop``).  A ray whose scale is 0 gets an exact 0 whatever its depths are."""
    t, w, tp = t_vals.detach(), weights.detach().double(), t_prop.detach()
    wp = w_prop.double()
    if ray_scale is not None:
        live = (ray_scale.detach() != 0).unsqueeze(1)
        t, tp = torch.where(live, t, torch.zeros_like(t)), torch.where(live, tp, torch.zeros_like(tp))
        w, wp = torch.where(live, w, torch.zeros_like(w)), torch.where(live, wp, torch.zeros_like(wp))
    P = tp.shape[1]
    a, p = _edges64(t), _edges64(tp).contiguous()
    # proposal intervals [lo, hi) overlapped by fine interval i: lo the largest j with p_j <= a_i (0 if none), hi the
    # smallest j with p_j >= a_{i+1} (P if none), raised to lo
    lo = (torch.searchsorted(p, a[:, :-1].contiguous(), right=True) - 1).clamp_min(0)
    hi = torch.maximum(torch.searchsorted(p, a[:, 1:].contiguous(), right=False).clamp_max(P), lo)
    c = torch.cat([wp.new_zeros(wp.shape[0], 1), torch.cumsum(wp, dim=1)], dim=1)
    # a range of one interval takes its weight itself, not a difference of sums (equal histograms give exactly 0)
    bound = torch.where(hi == lo + 1, torch.gather(wp, 1, lo.clamp_max(P - 1)),
                        torch.gather(c, 1, hi) - torch.gather(c, 1, lo))
    x = (w - bound).clamp_min(0.0)
    loss = (x * x / (w + float(eps))).sum(1)
    if ray_scale is not None:
        loss = torch.where(live.squeeze(1), loss * ray_scale.detach().double(), torch.zeros_like(loss))
    return loss.to(w_prop.dtype)


class _InterlevelFn(torch.autograd.Function):
    """One HIP launch (acn_interlevel_loss) that returns the per-ray loss and keeps d loss / d w_prop for the
    backward, which is g_loss[ray] * grad (the shape of nerfacc._DistortionFn)."""

    @staticmethod
    def forward(ctx, w_prop, t_vals, weights, t_prop, ray_scale, eps, want_grad):
        loss, grad = ops.interlevel_loss(t_vals, weights, t_prop, w_prop, ray_scale, eps=eps, want_grad=want_grad)
        ctx.set_materialize_grads(False)
        if want_grad:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        if g_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        return (g_loss.unsqueeze(1) * ctx.saved_tensors[0],) + (None,) * 6


def _interlevel_fused(t_vals: Tensor, weights: Tensor, t_prop: Tensor, w_prop: Tensor) -> bool:
    return (FUSED_INTERLEVEL and not _second_order()
            and all(x.is_cuda and x.dtype == torch.float32 for x in (t_vals, weights, t_prop, w_prop))
            and t_vals.shape[1] <= ops.INTERLEVEL_MAX_S and t_prop.shape[1] <= ops.INTERLEVEL_MAX_P)


def interlevel_loss(t_vals: Tensor, weights: Tensor, t_prop: Tensor, w_prop: Tensor, rays: Optional[Tensor] = None,
                    reduction: str = "mean", eps: float = 2.0 ** -23) -> Tensor:
    """The mip-NeRF 360 interlevel ("proposal") loss: the proposal's weight histogram along a ray must upper-bound
    the main model's.  ``t_vals`` / ``weights`` (N, S >= 2) are the fine render's depths and weights, ``t_prop`` /
    ``w_prop`` (N, P >= 2) the proposal's (``proposal_weights``).  A row of depths t owns the intervals between the
    edges [t_0 .. t_{S-1}, t_{S-1} + (t_{S-1} - t_{S-2})] (the compositing's own intervals, without volume_render's
    1e-4 clamp); with bound_i the sum of ``w_prop`` over the proposal intervals that overlap fine interval i,

        loss = sum_i max(0, w_i - bound_i)^2 / (w_i + eps)

    per ray.  ``weights`` and all depths are detached: the fine weights are the target, the only gradient is in
    ``w_prop``.  On ties this is deliberately the tight bound: two intervals that only share an edge do not overlap, so
    a fine interval that ends exactly on a proposal edge does not count the next proposal interval (multinerf's
    ``lossfun_outer`` counts it; parity with multinerf is unpinned, the package is not available here).
    ``rays`` (N, >=8) zeroes the rays without far > near (an invalid ray with NaN bounds contributes an exact 0).
    ``reduction``: none (N,) | mean | sum.  HIP fp32 tensors with S, P <= 1024 outside second_order() take one
    launch for loss and gradient (acn_interlevel_loss: float64 arithmetic, one fp32 rounding per output); everything
    else the same definition as float64 torch ops, differentiable any number of times in ``w_prop``."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"interlevel_loss: reduction must be none, mean or sum, got {reduction!r}")
    if (t_vals.dim() != 2 or t_vals.shape[1] < 2 or weights.shape != t_vals.shape or t_prop.dim() != 2
            or t_prop.shape[1] < 2 or w_prop.shape != t_prop.shape or t_prop.shape[0] != t_vals.shape[0]):
        raise ops.AcnError(f"interlevel_loss: t_vals and weights must both be (N, S >= 2), t_prop and w_prop both "
                           f"(N, P >= 2), got {tuple(t_vals.shape)}, {tuple(weights.shape)}, {tuple(t_prop.shape)} "
                           f"and {tuple(w_prop.shape)}")
    if not float(eps) > 0:
        raise ops.AcnError(f"interlevel_loss: eps must be > 0, got {eps}")
    dev = w_prop.device
    t_vals, weights, t_prop = t_vals.detach().to(dev), weights.detach().to(dev), t_prop.detach().to(dev)
    scale = None
    if rays is not None:
        if rays.dim() != 2 or rays.shape[0] != w_prop.shape[0] or rays.shape[1] < 8:
            raise ops.AcnError(f"interlevel_loss: rays must be ({w_prop.shape[0]}, >=8), got {tuple(rays.shape)}")
        near, far = rays.detach()[:, 6].to(dev), rays.detach()[:, 7].to(dev)
        scale = torch.where(far > near, torch.ones_like(far), torch.zeros_like(far))
    if _interlevel_fused(t_vals, weights, t_prop, w_prop):
        loss = _InterlevelFn.apply(w_prop, t_vals, weights, t_prop, scale, float(eps),
                                   torch.is_grad_enabled() and w_prop.requires_grad)
    else:
        loss = _interlevel_torch(t_vals, weights, t_prop, w_prop, ray_scale=scale, eps=eps)
    if reduction == "none":
        return loss
    return loss.mean() if reduction == "mean" else loss.sum()


def _proposal_weights_torch(sigma: Tensor, t: Tensor, sigma_scale) -> Tensor:
    """w = T alpha, alpha_i = 1 - exp(-sigma_i s d_i), T_i = exp(-sum_{j<i} sigma_j s d_j), d the widths of the rows'
    own intervals (_edges64), in float64 and rounded to sigma's dtype."""
    e = _edges64(t)
    tau = sigma.double() * sigma_scale * (e[:, 1:] - e[:, :-1])
    w = torch.exp(-(torch.cumsum(tau, dim=1) - tau)) * (1.0 - torch.exp(-tau))
    return w.to(sigma.dtype)


def proposal_weights(proposal, rays: Tensor, n_proposal: int, params=None, sigma_scale=1.0,
                     jitter_u: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(t_prop (N, P), w_prop (N, P)): the compositing weights of a density-only proposal field along the rays, at
    ``n_proposal`` stratified depths (stratified_t_vals, jittered iff ``proposal.training``, with ``jitter_u`` (N, P)
    as the uniforms).  ``proposal`` is any module with ``density(x (..., 3), params=None) -> (..., 1)``; a small
    MetaNGP of a few coarse hash levels is the intended one (its no-grad density is the fused field kernel, with grad
    it is the HIP hash grid plus the sigma branch).  Sample i owns [e_i, e_{i+1}], e the row's depths and one edge
    synthesised past the last (interlevel_loss's intervals); alpha_i = 1 - exp(-sigma_i sigma_scale d_i), T the
    exclusive product of 1 - alpha, w = T alpha.  On HIP fp32 that is nerfacc.render_weight_from_density on the packed
    view (P samples per ray; forward and backward kernels), elsewhere the formula as float64 torch ops.  Differentiable
    in the proposal's parameters (and fast weights), never in the depths or the rays."""
    P = int(n_proposal)
    if P < 2:
        raise ops.AcnError(f"proposal_weights: n_proposal must be >= 2, got {n_proposal}")
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ops.AcnError(f"proposal_weights: rays must be (N, >=8), got {tuple(rays.shape)}")
    r = rays.detach()
    N = r.shape[0]
    t = stratified_t_vals(r[:, 6], r[:, 7], P, randomized=bool(proposal.training), u=jitter_u)
    pts = r[:, None, :3] + r[:, None, 3:6] * t.unsqueeze(-1)
    sigma = proposal.density(pts.reshape(-1, 3), params=params).reshape(N, P)
    if sigma.is_cuda and sigma.dtype == torch.float32 and t.dtype == torch.float32 and not _second_order():
        t_end = torch.cat([t[:, 1:], t[:, -1:] + (t[:, -1:] - t[:, -2:-1])], dim=1)
        starts = torch.arange(N, dtype=torch.long, device=sigma.device) * P
        info = torch.stack([starts, torch.full_like(starts, P)], dim=-1)
        w, _, _ = nerfacc.render_weight_from_density(t.reshape(-1), t_end.reshape(-1),
                                                     (sigma * sigma_scale).reshape(-1), packed_info=info)
        return t, w.view(N, P)
    return t, _proposal_weights_torch(sigma, t, sigma_scale)


def render_rays_proposal(model, proposal, rays: Tensor, n_proposal: int, n_fine: int, params=None,
                         proposal_params=None, active_module: Optional[int] = None, bg_color_default: str = "white",
                         sigma_scale=1.0, chunk: int = 1_000_000, jitter_u: Optional[Tensor] = None,
                         jitter_fine: Optional[Tensor] = None, return_proposal: bool = False,
                         return_t_vals: bool = False, **kwargs):
    """Proposal-guided stratified renderer (mip-NeRF 360): the density-only ``proposal`` field is evaluated at
    ``n_proposal`` stratified depths (proposal_weights), ``n_fine`` depths per ray are drawn where its weights are
    (sample_pdf on the detached weights), and ``model`` is evaluated at those ``n_fine`` depths only (render_rays_at)
    -- not at the merged depths: evaluating the main model only where the proposal puts mass is the point.  Returns
    the fine pass: rgb (N,3), depth (N,), weights (N, n_fine), acc (N,).

    ``return_proposal`` appends (t_prop, w_prop) as one tuple, ``w_prop`` differentiable in the proposal's parameters
    (``interlevel_loss(t_fine, weights, t_prop, w_prop, rays)`` trains it); ``return_t_vals`` appends the (N, n_fine)
    fine depths last.  The resampling carries no gradient: the image loss never reaches the proposal.  The fine
    quantiles are jittered by ``jitter_fine`` (N, n_fine) or torch.rand when ``model.training`` and are the bin
    centres otherwise; ``jitter_u`` (N, n_proposal) goes to the proposal's depths.  ``params`` are the model's fast
    weights, ``proposal_params`` the proposal's.  One proposal covers the whole scene box of a container.  In eval mode
    without gradients this is the proposal's fused field launch, the weights, the resampling, the ray order and the
    fused render at depths."""
    P, F = int(n_proposal), int(n_fine)
    if P < 3:
        raise ops.AcnError(f"render_rays_proposal: the resampling needs n_proposal >= 3, got {n_proposal}")
    if F < 2:
        raise ops.AcnError(f"render_rays_proposal: the render needs n_fine >= 2, got {n_fine}")
    kwargs.pop("_want_weights", None)   # the caller of the interlevel loss needs the weights whatever render_image keeps
    early_stop_tau = float(kwargs.pop("early_stop_tau", 0.0))
    if kwargs:
        raise TypeError(f"render_rays_proposal: unexpected arguments {sorted(kwargs)}")
    N = rays.shape[0]
    t_prop, w_prop = proposal_weights(proposal, rays, P, params=proposal_params, sigma_scale=sigma_scale,
                                      jitter_u=jitter_u)
    jitter = None
    if model.training:
        jitter = jitter_fine if jitter_fine is not None else torch.rand(N, F, device=rays.device)
    t_fine = sample_pdf(t_prop, w_prop.detach(), F, jitter)
    out = render_rays_at(model, rays, t_fine, params=params, active_module=active_module,
                         bg_color_default=bg_color_default, chunk=chunk, sigma_scale=sigma_scale,
                         early_stop_tau=early_stop_tau)
    if return_proposal:
        out += ((t_prop, w_prop),)
    return out + (t_fine,) if return_t_vals else out


_STRATIFIED_POSITIONALS = ("ray_samples", "params", "active_module", "bg_color_default", "chunk", "sigma_scale",
                           "return_t_vals")


def render_rays(model, rays, *args, **kwargs):
    """Entry point (:564-574): occupancy renderer once the model's grids are ready, else stratified.
    ``n_importance`` = K > 0 (an extension) renders coarse to fine (render_rays_hierarchical) with K further depths
    per ray; it is an error once the occupancy renderer is active, which concentrates its samples by marching.
    ``proposal`` (an extension, with ``n_importance`` = F > 0) renders proposal-guided instead
    (render_rays_proposal): the proposal field at ``ray_samples`` depths, the model at F resampled depths."""
    n_importance = int(kwargs.pop("n_importance", 0) or 0)
    proposal = kwargs.pop("proposal", None)
    if proposal is not None:
        if n_importance <= 0:
            raise ops.AcnError("render_rays(proposal=...): the proposal-guided render needs n_importance > 0, the "
                               "number of depths the model is evaluated at")
        if getattr(model, "use_occ", False) and model.occ_ready:
            raise ops.AcnError("render_rays(proposal=...): the occupancy renderer concentrates its samples by "
                               "marching; a proposal goes with the stratified renderer")
        if len(args) > len(_STRATIFIED_POSITIONALS):
            raise TypeError("render_rays: too many positional arguments")
        kwargs.update(zip(_STRATIFIED_POSITIONALS, args))   # render_rays_stratified's positional order
        return render_rays_proposal(model, proposal, rays, kwargs.pop("ray_samples"), n_importance, **kwargs)
    if n_importance > 0:
        if getattr(model, "use_occ", False) and model.occ_ready:
            raise ops.AcnError("render_rays(n_importance > 0): the occupancy renderer concentrates its samples by "
                               "marching; importance resampling goes with the stratified renderer")
        if len(args) > len(_STRATIFIED_POSITIONALS):
            raise TypeError("render_rays: too many positional arguments")
        kwargs.update(zip(_STRATIFIED_POSITIONALS, args))   # render_rays_stratified's positional order
        return render_rays_hierarchical(model, rays, kwargs.pop("ray_samples"), n_importance, **kwargs)
    if getattr(model, "use_occ", False):
        if not model.occ_ready:
            return render_rays_stratified(model, rays, *args, **kwargs)
        if getattr(model, "warned_occ_ready", False) is False:
            warnings.warn("[OCC] Using nerfacc occupancy renderer (warmup concluded).")
            model.warned_occ_ready = True
        if kwargs.get("return_t_vals"):
            raise ops.AcnError("render_rays(return_t_vals=True): the occupancy renderer has no (N,S) t values; take "
                               "the distortion of its packed samples with nerfacc.distortion")
        kwargs.pop("return_t_vals", None)
        kwargs.pop("ray_samples", None)
        kwargs.pop("_want_weights", None)
        kwargs.pop("sigma_scale", None)
        kwargs.pop("early_stop_tau", None)
        kwargs.pop("jitter_u", None)
        if isinstance(model, MetaNGP):
            return render_expert_occ(model, rays, *args, **kwargs)
        return render_rays_occ(model, rays, *args, **kwargs)
    return render_rays_stratified(model, rays, *args, **kwargs)


@torch.no_grad()
def render_normals(model, rays: Tensor, ray_samples: int, params=None, active_module: Optional[int] = None,
                   bg_color_default: str = "white", min_weight: float = 0.0, chunk_rays: int = 8192,
                   normalize: bool = True):
    """Rendered normals of the stratified (eval) render: normal (N,3), rgb (N,3), depth (N,), acc (N,).

    normal = sum_s w_s * (-grad sigma / |grad sigma|) at the render's own samples, w the compositing weights.  Per
    chunk of ``chunk_rays`` rays: the fused stratified render with weights, the sample points o + d t of
    stratified_t_vals(randomized=False), the model's ``sigma_gradient`` gated by the weights (samples with
    w <= min_weight are not evaluated: each dropped term has norm <= its weight) and ops.normal_composite.
    ``normalize``: the final F.normalize (a zero vector, e.g. a ray that hits nothing, stays zero).  Evaluation
    only: the jittered samples of a model in training mode are not reproducible here, so it raises."""
    if model.training:
        raise ops.AcnError("render_normals renders the evaluation samples (model.eval()); a model in training mode "
                           "draws jittered samples")
    N, S = rays.shape[0], int(ray_samples)
    normal = rays.new_zeros(N, 3, dtype=torch.float32)
    outs = []
    for a in range(0, N, max(1, int(chunk_rays))):
        r = rays[a:a + chunk_rays]
        rgb, depth, w, acc = render_rays_stratified(model, r, S, params=params, active_module=active_module,
                                                    bg_color_default=bg_color_default)
        t = stratified_t_vals(r[:, 6], r[:, 7], S, randomized=False)
        pts = (r[:, None, :3] + r[:, None, 3:6] * t.unsqueeze(-1)).reshape(-1, 3)
        gate = w.reshape(-1)
        if isinstance(model, MetaContainer):
            _, g = model.sigma_gradient(pts, params=params, active_module=active_module, gate=gate, gate_min=min_weight)
        else:
            _, g = model.sigma_gradient(pts, params=params, gate=gate, gate_min=min_weight)
        normal[a:a + r.shape[0]] = ops.normal_composite(g, w) if r.is_cuda else _normal_composite_torch(g, w)
        outs.append((rgb, depth, acc))
    if normalize:
        normal = torch.nn.functional.normalize(normal, dim=-1)
    if len(outs) == 1:
        rgb, depth, acc = outs[0]
    else:
        rgb, depth, acc = (torch.cat([o[i] for o in outs], 0) if outs else rays.new_zeros(0) for i in range(3))
    return normal, rgb, depth, acc


def distortion_loss(weights: Tensor, t_vals: Tensor, rays: Optional[Tensor] = None, reduction: str = "mean") -> Tensor:
    """The mip-NeRF 360 distortion regulariser of a stratified render: per ray
    sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i over the compositing's own intervals (s_i = t_i,
    d_i = volume_render's ``dists``, m_i = s_i + d_i / 2), for the (N,S) ``weights`` and ``t_vals`` of
    ``render_rays_stratified(..., return_t_vals=True)``.  ``rays`` (N, >=8) normalises every ray to unit length
    (the loss times 1 / (far - near); a ray without far > near, e.g. an invalid one with NaN bounds, contributes an
    exact 0).  ``reduction``: none (N,) | mean | sum.  Differentiable in the weights (loss and gradient from one
    HIP launch, acn_distortion_dense); the t values carry no gradient."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"distortion_loss: reduction must be none, mean or sum, got {reduction!r}")
    if weights.dim() != 2 or weights.shape[1] < 2 or t_vals.shape != weights.shape:
        raise ops.AcnError(f"distortion_loss: weights and t_vals must both be (N, S >= 2), got {tuple(weights.shape)} "
                           f"and {tuple(t_vals.shape)}")
    scale = None
    if rays is not None:
        if rays.dim() != 2 or rays.shape[0] != weights.shape[0] or rays.shape[1] < 8:
            raise ops.AcnError(f"distortion_loss: rays must be ({weights.shape[0]}, >=8), got {tuple(rays.shape)}")
        near, far = rays.detach()[:, 6].to(weights.device), rays.detach()[:, 7].to(weights.device)
        scale = torch.where(far > near, 1.0 / (far - near), torch.zeros_like(far))
    if nerfacc._distortion_fused(weights):
        loss = nerfacc._DistortionFn.apply(weights, t_vals.detach(), None, None, None, None, scale,
                                           torch.is_grad_enabled() and weights.requires_grad)
    else:
        loss = nerfacc._distortion_torch(weights, *nerfacc._dense_intervals(t_vals), ray_scale=scale)
    if reduction == "none":
        return loss
    return loss.mean() if reduction == "mean" else loss.sum()


def depth_loss(weights: Tensor, t_vals: Tensor, depths: Tensor, eps, rays: Optional[Tensor] = None,
               depth_weight: float = 1.0, sight_weight: float = 1.0, reduction: str = "mean") -> Tensor:
    """Depth supervision of a stratified render (the expected-depth term of DS-NeRF plus the
    line-of-sight term of Urban Radiance Fields), for the (N,S) ``weights`` and ``t_vals`` of
    ``render_rays(..., return_t_vals=True)``.  Per ray with the target ``depths[r]`` = z (distance along the ray, the
    unit of ``t_vals``; ``ray_sampling.point_depth_targets`` makes them from a point cloud), the half-width ``eps`` (a
    float or (N,)) and sigma = eps / 3, over the compositing's own intervals [t_i, t_i + d_i] (d = volume_render's
    ``dists``):

        depth_weight (c (D - z))^2 + sight_weight sum_{t_i < z + eps} (w_i - k_i)^2,    D = sum_i w_i t_i

    D is the ``depth`` volume_render returns; k_i is the mass the Gaussian N(z, sigma) cut at z +- eps puts into
    interval i, so weight in front of the window pays w^2 (empty space), weight inside it is drawn to the Gaussian,
    and weight behind it is left to occlusion.  ``rays`` (N, >=8) sets c = 1 / (far - near) (c = 1 without): the depth
    error in units of the ray's length, 0 for a ray without far > near.  A ray whose depth or eps is not finite or
    <= 0 (NaN marks a pixel without a target), or whose c is 0, contributes an exact 0 to loss and gradient, whatever
    its t values.  ``reduction``: none (N,) | sum | mean, the mean over the rays that carry a target (at least 1):
    sparse targets cover a small, varying share of a batch, and a mean over all rays would scale the term by that
    share.  The count is taken on the device without a host read.  Differentiable in the weights (loss and gradient
    from one HIP launch, acn_depth_loss_dense; elsewhere the same formula as float64 torch ops, differentiable any
    number of times); the t values, targets and eps carry no gradient."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"depth_loss: reduction must be none, mean or sum, got {reduction!r}")
    if weights.dim() != 2 or weights.shape[1] < 2 or t_vals.shape != weights.shape:
        raise ops.AcnError(f"depth_loss: weights and t_vals must both be (N, S >= 2), got {tuple(weights.shape)} "
                           f"and {tuple(t_vals.shape)}")
    ld, ls = nerfacc._check_depth_weights(depth_weight, sight_weight, "depth_loss")
    dev = weights.device
    z, ep = nerfacc._depth_targets(depths, eps, weights.shape[0], dev, "depth_loss")
    scale = None
    if rays is not None:
        if rays.dim() != 2 or rays.shape[0] != weights.shape[0] or rays.shape[1] < 8:
            raise ops.AcnError(f"depth_loss: rays must be ({weights.shape[0]}, >=8), got {tuple(rays.shape)}")
        near, far = rays.detach()[:, 6].to(dev), rays.detach()[:, 7].to(dev)
        scale = torch.where(far > near, 1.0 / (far - near), torch.zeros_like(far))
    t = t_vals.detach().to(dev)
    if nerfacc._distortion_fused(weights):
        loss = nerfacc._DepthLossFn.apply(weights, t, None, None, None, None, z, ep, scale, ld, ls,
                                          torch.is_grad_enabled() and weights.requires_grad)
    else:
        d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
        d = torch.cat([d, d[:, -1:]], dim=1).double()
        loss = nerfacc._depth_loss_torch(weights, t.double(), t.double() + d, t.double(), z, ep, scale, ld, ls)
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    return loss.sum() / nerfacc._depth_live(z, ep, scale).sum().clamp_min(1).to(loss.dtype)


def _normal_composite_torch(grad: Tensor, weights: Tensor) -> Tensor:
    """ops.normal_composite as torch ops (CPU models): fp32 terms, float64 sum over the samples."""
    N, S = weights.shape
    g = grad.reshape(N, S, 3).float()
    d = g.norm(dim=-1, keepdim=True).clamp_min(1e-9)
    return (weights.float().unsqueeze(-1) * (-g / d)).double().sum(1).float()


@torch.no_grad()
def render_normal_image(model, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float, c2w: Tensor, scene_box,
                        params=None, active_module: Optional[int] = None, ray_samples: int = 64,
                        bg_color_default: str = "white", center_pixels: bool = True, min_weight: float = 0.0,
                        chunk_rays: int = 8192, normalize: bool = True):
    """Full-frame normal map, the companion of render_image: ((H,W,3) normals, (H,W,3) rgb clamped to [0,1],
    depth (H*W,), acc (H*W,)) from the same per-pixel rays."""
    device = next(model.parameters()).device
    rays, _ = ops.get_rays_image(H, W, fx, fy, cx, cy, c2w, scene_box.aabb, device, center_pixels=center_pixels,
                                 near_far_override=(None, None), apply_clamp=True)
    normal, rgb, depth, acc = render_normals(model, rays, ray_samples, params=params, active_module=active_module,
                                             bg_color_default=bg_color_default, min_weight=min_weight,
                                             chunk_rays=chunk_rays, normalize=normalize)
    return normal.view(H, W, 3), rgb.view(H, W, 3).float().clamp_(0, 1), depth.view(-1), acc.view(-1)


@torch.no_grad()
def render_image(model, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float, c2w: Tensor, scene_box,
                 params=None, active_module: Optional[int] = None, ray_samples: int = 64, chunk_points: int = 1 << 16,
                 bg_color_default: str = "white", center_pixels: bool = True, use_amp: bool = False,
                 appearance=None, image_index=None, **kwargs) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """Full frame: per-pixel rays (one fused HIP kernel), render_rays, (H,W,3) clamp (:577-627).
    ``use_amp`` is accepted for interface compatibility; the HIP path computes in fp32.
    ``appearance`` (an appearance.AppearanceAffine) with ``image_index`` corrects the clamped frame
    with that image's matrix and offset (one more launch; the result is not clamped again); an index the model has no
    slot for leaves the frame bit-identical."""
    device = next(model.parameters()).device
    rays, _ = ops.get_rays_image(H, W, fx, fy, cx, cy, c2w, scene_box.aabb, device, center_pixels=center_pixels,
                                 near_far_override=(None, None), apply_clamp=True)
    rgb_lin, depth, _, acc = render_rays(model, rays, ray_samples=ray_samples, params=params,
                                         active_module=active_module, bg_color_default=bg_color_default,
                                         chunk=chunk_points, _want_weights=False, **kwargs)
    rgb_lin = rgb_lin.view(H, W, 3).float().clamp_(0, 1)
    if appearance is not None:
        if image_index is None:
            raise ValueError("render_image: an appearance model needs image_index (the frame's image index)")
        rgb_lin = appearance(rgb_lin, image_index)
    return rgb_lin, (None if depth is None else depth.view(-1)), (None if acc is None else acc.view(-1))
