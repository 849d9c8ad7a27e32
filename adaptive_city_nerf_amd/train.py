"""Online adaptation step (reference: pipelines/online_stage/runtime_adapt.py:213-315 ``runtime_adapt``,
nerfs/losses.py:10-32 ``compute_mse_loss``) on the HIP path.

One step = ``render_rays`` in training mode (stratified jitter) through the differentiable
per-expert forward -> sRGB/linear colour transform -> MSE -> backward (the hash-grid gather
backward is a HIP scatter-add kernel) -> ``clip_grad_norm_`` + Adam as one fused multi-tensor HIP
step (optim.FusedAdam).  The reference wraps the forward in fp16 autocast with a GradScaler; the default
fp16x3 MLP keeps fp32 accuracy, so no scale is needed; the use_amp precision (the reference's fp16
arithmetic, ops.set_train_mlp_precision("amp")) runs under a GradScaler like the reference's.

Expert-parallel use: ``adapt_step(..., group=)`` on the routed container
(active_module None, the online stage's call, runtime_adapt.py:88-90) distributes the experts over the
ranks of ``group`` (expert_parallel.py: all-to-all of per-sample records, complete per-expert
gradients on the owners, all-reduced background head, global clip norm): the update equals the
single-process one.  ``active_module=k`` adapts one expert with the container's background head; the
reference's own runtime_adapt cannot run that configuration (it renders ``base.submodules`` of the
expert itself), so it stays a single-process placement variant and refuses a group.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, Optional

import torch
import torch.nn.functional as F

from . import ops
from ._lib import graph_capture
from .color_space import color_space_transformer
from .optim import FusedAdam
from .ray_rendering import depth_loss, distortion_loss, interlevel_loss, render_rays


class _MSELinearFn(torch.autograd.Function):
    """F.mse_loss(*color_space_transformer(pred, gt, 'linear')) as two HIP launches (loss.hip) instead of
    ~16 elementwise / reduction kernels; same float semantics (clamps pass NaN, powf, float scalars)."""

    @staticmethod
    def forward(ctx, pred, gt):
        ctx.save_for_backward(pred, gt)
        return ops.mse_linear_fwd(pred, gt)

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        return ops.mse_linear_bwd(pred, gt, g.detach()), None


def mse_color_loss(pred_rgb, gt_rgb, color_space: str, reduction: str = "mean"):
    """F.mse_loss(*color_space_transformer(pred, gt, color_space)) (losses.py:10-32)."""
    from .ray_rendering import _second_order
    if (str(color_space).lower() == "linear" and reduction == "mean" and pred_rgb.is_cuda
            and pred_rgb.dtype == torch.float32 and pred_rgb.numel() > 0 and pred_rgb.shape == gt_rgb.shape
            and not _second_order()):
        return _MSELinearFn.apply(pred_rgb, gt_rgb.to(pred_rgb.device, torch.float32))
    pred_rgb, gt_rgb = color_space_transformer(pred_rgb, gt_rgb, color_space=color_space)
    return F.mse_loss(pred_rgb, gt_rgb, reduction=reduction)


class _AppearanceMSEFn(torch.autograd.Function):
    """mse_color_loss(appearance(pred, img), gt, 'linear') as one HIP launch (appearance.hip) that
    returns the loss and keeps its gradients to the prediction, the matrices and the offsets for the backward, which
    multiplies them by the incoming gradient."""

    @staticmethod
    def forward(ctx, pred, gt, slots, A, b):
        want = any(ctx.needs_input_grad)
        loss, g_pred, g_A, g_b = ops.appearance_mse(pred, gt, slots, A, b, want_grad=want)
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(g_pred, g_A, g_b)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 5
        g_pred, g_A, g_b = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (g * g_pred if need[0] else None, None, None, g * g_A if need[3] else None,
                g * g_b if need[4] else None)


def appearance_mse_loss(pred_rgb, gt_rgb, img_indices, appearance, color_space: str, reduction: str = "mean"):
    """mse_color_loss on the per-image corrected prediction ``appearance(pred_rgb, img_indices)``
    (appearance.AppearanceAffine).  In colour space ``linear`` with reduction ``mean``, on fp32 device
    tensors and outside second_order(), the correction, the loss and the gradients to the prediction and to the
    appearance parameters are one HIP launch (ops.appearance_mse); otherwise it is the composed torch chain, which is
    differentiable any number of times and works on CPU tensors."""
    from .ray_rendering import _second_order
    if (str(color_space).lower() == "linear" and reduction == "mean" and pred_rgb.is_cuda
            and pred_rgb.dtype == torch.float32 and pred_rgb.numel() > 0 and pred_rgb.shape == gt_rgb.shape
            and pred_rgb.shape[-1] == 3 and appearance.matrix.is_cuda and appearance.matrix.dtype == torch.float32
            and not _second_order()):
        slots = appearance.slots(img_indices)
        if slots.numel() != pred_rgb.numel() // 3:
            raise ValueError(f"appearance_mse_loss: {slots.numel()} image indices for {pred_rgb.numel() // 3} rays")
        return _AppearanceMSEFn.apply(pred_rgb, gt_rgb.to(pred_rgb.device, torch.float32), slots, appearance.matrix,
                                      appearance.offset)
    from .appearance import _apply_torch
    slots = appearance.slots(img_indices).to(pred_rgb.device)
    corrected = _apply_torch(pred_rgb, slots, appearance.matrix.to(pred_rgb.device),
                             appearance.offset.to(pred_rgb.device))
    return mse_color_loss(corrected, gt_rgb, color_space, reduction)


def _image_loss(pred_rgb, data, P, reduction, appearance, appearance_reg):
    """The image term of compute_loss: mse_color_loss, or with an appearance model appearance_mse_loss on
    ``data["img_indices"]`` plus ``appearance_reg`` times its regulariser."""
    if appearance is None:
        return mse_color_loss(pred_rgb, data["rgbs"], P.color_space, reduction)
    if data.get("img_indices") is None:
        raise ValueError("compute_loss: an appearance model needs data['img_indices'] (one image index per ray)")
    loss = appearance_mse_loss(pred_rgb, data["rgbs"], data["img_indices"], appearance, P.color_space, reduction)
    if appearance_reg:
        loss = loss + float(appearance_reg) * appearance.regulariser()
    return loss


def compute_mse_loss(P, model, data, params=None, active_module=None, reduction: str = "mean", **render_kwargs):
    """losses.py:10-32: MSE between render_rays(...) rgb and data['rgbs'] in P.color_space."""
    gt_rgb = data["rgbs"]
    rays = data["rays"]
    pred_rgb, *_ = render_rays(model, rays, ray_samples=P.ray_samples, params=params, active_module=active_module,
                               chunk=P.chunk_points, **render_kwargs)
    return mse_color_loss(pred_rgb, gt_rgb, P.color_space, reduction)


def compute_loss(P, model, data, params=None, active_module=None, reduction: str = "mean",
                 distortion_weight: float = 0.0, proposal=None, interlevel_weight: float = 1.0,
                 depth_weight: float = 0.0, sight_weight: float = 0.0, depth_eps=None, appearance=None,
                 appearance_reg: float = 0.0, **render_kwargs):
    """compute_mse_loss plus ``distortion_weight`` times the mean distortion loss of the render's weights
    (ray_rendering.distortion_loss, every ray normalised to unit length): the mip-NeRF 360 regulariser against
    semi-transparent fog and floaters between the camera and the surface.  With weight 0 it is compute_mse_loss, from
    the same calls.  The regulariser needs the stratified renderer's (N,S) weights and t values: with the occupancy
    renderer active, render_rays raises (take nerfacc.distortion of the packed samples instead).

    ``proposal`` (a density-only field, ray_rendering.proposal_weights) renders proposal-guided
    (render_rays_proposal; ``n_importance`` in the render kwargs is the number of depths the model is evaluated at,
    ``P.ray_samples`` the proposal's) and adds ``interlevel_weight`` times the mean interlevel loss, which trains the
    proposal and carries no gradient to the model; the image loss carries none to the proposal.

    ``depth_weight`` / ``sight_weight`` > 0 add depth supervision (ray_rendering.depth_loss): that
    multiple of the expected-depth term and of the line-of-sight term, against the targets ``data["depths"]`` (N,)
    (distance along the ray; NaN where a ray has none) with the half-width ``depth_eps`` (a float or (N,)), averaged
    over the rays that carry a target, on the weights of the pass the image loss is taken on.  With both 0 nothing
    changes: the same calls, the same loss.

    ``appearance`` (an appearance.AppearanceAffine) takes the image loss on the per-image corrected
    colour (appearance_mse_loss, with the image index of every ray in ``data["img_indices"]``, the key TaskDataset
    emits) and adds ``appearance_reg`` times its regulariser; the render itself is untouched.  With None nothing
    changes: the same calls, the same loss."""
    geo = {}
    if depth_weight or sight_weight:
        geo = _depth_terms(depth_weight, sight_weight, data.get("depths"), depth_eps, "compute_loss")
    if proposal is not None:
        if not render_kwargs.get("n_importance"):
            raise ValueError("compute_loss: a proposal needs n_importance > 0 in the render arguments (the number of "
                             "depths the model is evaluated at)")
        rays = data["rays"]
        pred_rgb, _, weights, _, (t_prop, w_prop), t_vals = render_rays(
            model, rays, ray_samples=P.ray_samples, params=params, active_module=active_module, chunk=P.chunk_points,
            proposal=proposal, return_proposal=True, return_t_vals=True, **render_kwargs)
        loss = _image_loss(pred_rgb, data, P, reduction, appearance, appearance_reg)
        if distortion_weight:
            loss = loss + float(distortion_weight) * distortion_loss(weights, t_vals, rays=rays, reduction="mean")
        if geo:
            loss = loss + depth_loss(weights, t_vals, data["depths"], depth_eps, rays=rays, reduction="mean", **geo)
        return loss + float(interlevel_weight) * interlevel_loss(t_vals, weights, t_prop, w_prop, rays=rays,
                                                                 reduction="mean")
    if not distortion_weight and not geo and appearance is None:
        return compute_mse_loss(P, model, data, params=params, active_module=active_module, reduction=reduction,
                                **render_kwargs)
    rays = data["rays"]
    if not distortion_weight and not geo:
        pred_rgb, *_ = render_rays(model, rays, ray_samples=P.ray_samples, params=params, active_module=active_module,
                                   chunk=P.chunk_points, **render_kwargs)
        return _image_loss(pred_rgb, data, P, reduction, appearance, appearance_reg)
    pred_rgb, _, weights, _, t_vals = render_rays(model, rays, ray_samples=P.ray_samples, params=params,
                                                  active_module=active_module, chunk=P.chunk_points,
                                                  return_t_vals=True, **render_kwargs)
    loss = _image_loss(pred_rgb, data, P, reduction, appearance, appearance_reg)
    if distortion_weight:
        loss = loss + float(distortion_weight) * distortion_loss(weights, t_vals, rays=rays, reduction="mean")
    if geo:
        loss = loss + depth_loss(weights, t_vals, data["depths"], depth_eps, rays=rays, reduction="mean", **geo)
    return loss


def _depth_terms(depth_weight, sight_weight, depths, depth_eps, what: str) -> dict:
    """{} with both weights 0 (no depth supervision), else depth_loss's two weights, after checking that the targets
    and the half-width are there."""
    if not depth_weight and not sight_weight:
        return {}
    if depths is None or depth_eps is None:
        raise ValueError(f"{what}: depth_weight / sight_weight need the target depths and depth_eps")
    return {"depth_weight": float(depth_weight), "sight_weight": float(sight_weight)}


def adapt_step(P, base, rays, rgbs, optimizer, active_module=None, grad_clip: Optional[float] = 1.0,
               group=None, shared: Optional[list] = None, grad_scaler=None, distortion_weight: float = 0.0,
               proposal=None, interlevel_weight: float = 1.0, depths=None, depth_weight: float = 0.0,
               sight_weight: float = 0.0, depth_eps=None, img_indices=None, appearance=None,
               appearance_reg: float = 0.0, **render_kwargs) -> torch.Tensor:
    """One optimizer update of runtime_adapt (runtime_adapt.py:288-313).  Returns the loss (device).
    ``distortion_weight`` > 0 adds that multiple of the mean distortion loss (compute_loss) to the MSE.
    ``n_importance`` = K > 0 (through ``render_kwargs``, with ``jitter_fine``) trains on the coarse-to-fine render
    (render_rays_hierarchical): the loss is taken on the fine pass.
    ``proposal`` (with ``n_importance``) trains on the proposal-guided render and adds ``interlevel_weight`` times the
    interlevel loss (compute_loss), which trains the proposal: its parameters must be in ``optimizer``.
    ``depth_weight`` / ``sight_weight`` > 0 add depth supervision against ``depths`` (N,) with the half-width
    ``depth_eps`` (compute_loss); with both 0, ``depths`` is not looked at.
    ``appearance`` (an appearance.AppearanceAffine) trains on the per-image corrected colour (compute_loss) with the
    image index of every ray in ``img_indices`` (N,), plus ``appearance_reg`` times its regulariser; some of its
    parameters must be in ``optimizer``.  FusedAdam's folded clip norm is taken over every gradient-carrying tensor of
    the optimizer, so it includes the appearance gradients; without FusedAdam they are clipped with the base's too.
    With None, ``img_indices`` is not looked at.

    ``group`` (expert parallel): ``rays`` / ``rgbs`` are this rank's shard of the global batch, the
    container's experts are distributed over the group (expert_parallel.adapt_step_expert_parallel);
    ``shared`` are the replicated parameters (default: the background head).
    With the use_amp MLP precision (ops.set_train_mlp_precision("amp")) the step runs under a GradScaler as
    the reference's does (runtime_adapt.py:237-268): ``grad_scaler`` (a torch.amp.GradScaler; a fresh one when
    None) scales the loss, unscales, skips a non-finite step and updates its scale."""
    if group is not None and distortion_weight:
        raise ValueError("adapt_step: the expert-parallel step has no distortion loss (distortion_weight must be 0 "
                         "with a group)")
    if group is not None and (depth_weight or sight_weight):
        raise ValueError("adapt_step: the expert-parallel step has no depth supervision (depth_weight and sight_weight "
                         "must be 0 with a group)")
    geo = _depth_terms(depth_weight, sight_weight, depths, depth_eps, "adapt_step")
    if group is not None and render_kwargs.get("n_importance"):
        raise ValueError("adapt_step: the expert-parallel step renders one stratified pass (n_importance must be 0 "
                         "with a group)")
    if group is not None and proposal is not None:
        raise ValueError("adapt_step: the expert-parallel step renders one stratified pass (no proposal with a group)")
    if group is not None and appearance is not None:
        raise ValueError("adapt_step: the expert-parallel step has no appearance model (appearance must be None with "
                         "a group)")
    if proposal is not None:
        held = {id(p) for g in optimizer.param_groups for p in g["params"]}
        if not any(id(p) in held for p in proposal.parameters()):
            raise ValueError("adapt_step: none of the proposal's parameters is in the optimizer; the interlevel loss "
                             "would train nothing")
    if appearance is not None:
        if img_indices is None:
            raise ValueError("adapt_step: an appearance model needs img_indices (one image index per ray)")
        held = {id(p) for g in optimizer.param_groups for p in g["params"]}
        if not any(id(p) in held for p in appearance.parameters()):
            raise ValueError("adapt_step: none of the appearance model's parameters is in the optimizer; the "
                             "correction would train nothing")
    if group is not None and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1:
        from .expert_parallel import HipBackend, adapt_step_expert_parallel
        if active_module is not None:
            raise ValueError("adapt_step: expert-parallel groups adapt the routed container (active_module=None)")
        n = torch.tensor([rays.shape[0]], dtype=torch.int64, device=rays.device)
        torch.distributed.all_reduce(n, group=group)
        shared = list(base.bg_mlp.parameters()) if shared is None else shared
        return adapt_step_expert_parallel(P, HipBackend(base), rays, rgbs, optimizer, len(base.submodules), int(n),
                                          shared, grad_clip=grad_clip, group=group,
                                          u=render_kwargs.get("jitter_u"))
    optimizer.zero_grad()
    data = {"rays": rays, "rgbs": rgbs}
    if geo:
        data["depths"] = depths
        render_kwargs = dict(render_kwargs, depth_eps=depth_eps, **geo)
    if appearance is not None:
        data["img_indices"] = img_indices
        render_kwargs = dict(render_kwargs, appearance=appearance, appearance_reg=appearance_reg)
    loss = compute_loss(P, model=base, data=data, params=None, active_module=active_module,
                        reduction="mean", distortion_weight=distortion_weight, proposal=proposal,
                        interlevel_weight=interlevel_weight, **render_kwargs)
    # without FusedAdam the clip norm is taken over the base's and the proposal's parameters together
    clipped = base.parameters() if proposal is None else list(base.parameters()) + list(proposal.parameters())
    if appearance is not None:
        clipped = list(clipped) + list(appearance.parameters())
    if ops.TRAIN_MLP_PRECISION == "amp":
        scaler = grad_scaler if grad_scaler is not None else torch.amp.GradScaler("cuda")
        scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
        if isinstance(optimizer, FusedAdam):
            scaler.step(optimizer, max_norm=grad_clip)
        else:
            if grad_clip is not None:
                torch.nn.utils.clip_grad_norm_(clipped, grad_clip)
            scaler.step(optimizer)
        scaler.update()
        return loss.detach()
    loss.backward()
    if isinstance(optimizer, FusedAdam):
        optimizer.step(max_norm=grad_clip)  # clip_grad_norm_ folded into the fused step
    else:
        if grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(clipped, grad_clip)
        optimizer.step()
    return loss.detach()


class GraphedAdaptStep:
    """adapt_step captured once into a HIP graph and replayed per batch (the launch-bound inner loop
    of runtime_adapt: ~165 kernels per 1000-ray step).  Same arithmetic as the eager step -- the Adam
    constants come from FusedAdam's device table, the jitter from the graph-safe generator -- with
    the batch copied into static buffers before each replay.  ``warmup`` eager steps run first (they
    are real updates on the first batch).  Only fixed-shape steps are capturable: one expert
    (``active_module``, the C5 / meta-training placement) or a bare MetaNGP -- the routed container's
    per-expert index selection is data-dependent.  Expert-parallel groups are not captured (use
    adapt_step).  ``distortion_weight`` as in adapt_step: the distortion launch and its backward multiply make no
    host synchronisation, so they are captured with the rest.  The proposal-guided step is not captured (use
    adapt_step).  ``depth_weight`` / ``sight_weight`` as in adapt_step: ``depths`` (N,) is copied into a static buffer
    before each replay (pass ``depths=`` per call), ``depth_eps`` is fixed at capture; the depth launch and the count
    of rays with a target make no host synchronisation.  ``appearance`` / ``appearance_reg`` as in adapt_step:
    ``img_indices`` (N,) is kept as a static int32 buffer and copied before each replay (pass ``img_indices=`` per
    call); the slot gather and the fused loss make no host synchronisation."""

    def __init__(self, P, base, rays, rgbs, optimizer, active_module=None, grad_clip: Optional[float] = 1.0,
                 warmup: int = 2, max_steps: int = 1 << 16, distortion_weight: float = 0.0, proposal=None,
                 depths=None, depth_weight: float = 0.0, sight_weight: float = 0.0, depth_eps=None, img_indices=None,
                 appearance=None, appearance_reg: float = 0.0, **render_kwargs):
        from .meta_container import MetaContainer
        if proposal is not None:
            raise ValueError("GraphedAdaptStep: the proposal-guided render is not captured; use adapt_step")
        if render_kwargs.get("n_importance"):
            raise ValueError("GraphedAdaptStep: the hierarchical render (n_importance > 0) is not captured; use "
                             "adapt_step")
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("GraphedAdaptStep needs FusedAdam")
        if isinstance(base, MetaContainer) and active_module is None:
            raise ValueError("GraphedAdaptStep: the routed container step is data-dependent; pass active_module")
        self.static_rays = rays.detach().clone()
        self.static_rgbs = rgbs.detach().clone()
        self.static_u = None
        if render_kwargs.get("jitter_u") is not None:  # caller-supplied jitter: a static input too
            self.static_u = render_kwargs["jitter_u"].detach().clone()
            render_kwargs = dict(render_kwargs, jitter_u=self.static_u)
        if distortion_weight:
            render_kwargs = dict(render_kwargs, distortion_weight=float(distortion_weight))
        self.static_depths = None
        geo = _depth_terms(depth_weight, sight_weight, depths, depth_eps, "GraphedAdaptStep")
        if geo:
            self.static_depths = depths.detach().to(rays.device, torch.float32).reshape(-1).clone()
            if isinstance(depth_eps, torch.Tensor):
                depth_eps = depth_eps.detach().to(rays.device, torch.float32).clone()
            render_kwargs = dict(render_kwargs, depths=self.static_depths, depth_eps=depth_eps, **geo)
        self.static_img = None
        if appearance is not None:
            if img_indices is None:
                raise ValueError("GraphedAdaptStep: an appearance model needs img_indices (one image index per ray)")
            self.static_img = img_indices.detach().to(rays.device, torch.int32).reshape(-1).clone()
            render_kwargs = dict(render_kwargs, img_indices=self.static_img, appearance=appearance,
                                 appearance_reg=appearance_reg)
        self.args = (P, base, optimizer, active_module, grad_clip, render_kwargs)
        side = torch.cuda.Stream(rays.device)
        side.wait_stream(torch.cuda.current_stream(rays.device))
        with torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):
                adapt_step(P, base, self.static_rays, self.static_rgbs, optimizer, active_module=active_module,
                           grad_clip=grad_clip, **render_kwargs)
        torch.cuda.current_stream(rays.device).wait_stream(side)
        torch.cuda.synchronize(rays.device)
        optimizer.graph_begin(max_steps)
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with graph_capture(self.graph):
            self.static_loss = adapt_step(P, base, self.static_rays, self.static_rgbs, optimizer,
                                          active_module=active_module, grad_clip=grad_clip, **render_kwargs)
        optimizer.graph_end_capture()
        self.replays = 0
        self.max_steps = int(max_steps)

    def __call__(self, rays: torch.Tensor, rgbs: torch.Tensor, jitter_u: Optional[torch.Tensor] = None,
                 depths: Optional[torch.Tensor] = None, img_indices: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.replays >= self.max_steps:
            # past the precomputed Adam table the captured update would silently stop
            raise RuntimeError(f"GraphedAdaptStep: {self.max_steps} replays exhausted the Adam constant table; "
                               f"capture a new GraphedAdaptStep (max_steps=...)")
        self.static_rays.copy_(rays, non_blocking=True)
        self.static_rgbs.copy_(rgbs, non_blocking=True)
        if jitter_u is not None:
            self.static_u.copy_(jitter_u, non_blocking=True)
        if depths is not None:
            if self.static_depths is None:
                raise ValueError("GraphedAdaptStep: captured without depth supervision; depths cannot be replayed")
            self.static_depths.copy_(depths.reshape(-1), non_blocking=True)
        if img_indices is not None:
            if self.static_img is None:
                raise ValueError("GraphedAdaptStep: captured without an appearance model; img_indices cannot be "
                                 "replayed")
            self.static_img.copy_(img_indices.reshape(-1), non_blocking=True)
        self.graph.replay()
        self.replays += 1
        from .optim import bump_versions
        bump_versions(self.args[2]._graph["params"])  # the replayed Adam wrote them: packed images are stale
        return self.static_loss

    def sync_state(self) -> None:
        """Write the replay count into the optimizer's host state['step'] entries."""
        self.args[2].graph_sync_steps(self.replays)


def _routed_step_for(P, model, optimizer, n_rays: int, grad_clip):
    """The RoutedAdaptStep cached on ``optimizer`` for ``model`` (built on first use, sized for the first
    batch), or None when the configuration is outside what the routed pair kernels cover (then the eager
    adapt_step runs).  A batch larger than the cached step's capacity rebuilds it (state carried over
    through the optimizer's host state)."""
    from .meta_container import MetaContainer
    from .routed_train import RoutedAdaptStep
    from ._lib import AcnError
    if not (FAST_RUNTIME_ADAPT and isinstance(model, MetaContainer) and isinstance(optimizer, FusedAdam)):
        return None
    cache = optimizer.__dict__.setdefault("_acn_routed_steps", {})
    key = (id(model), grad_clip, int(P.ray_samples), str(P.color_space))
    st = cache.get(key)
    if st is not None and n_rays <= st.N:
        st.load_state()   # eager steps on this optimizer since the last call advanced the host counters
        return st
    if st is not None:
        st.sync_state()
        del cache[key]
    try:
        st = RoutedAdaptStep(P, model, n_rays, optimizer, grad_clip=grad_clip, graph=True, warmup=1)
    except AcnError:
        return None
    cache[key] = st
    return st


# runtime_adapt's full batches through the cached, graph-replayed RoutedAdaptStep (ACN_FAST_ADAPT=0: the
# eager adapt_step for every batch)
FAST_RUNTIME_ADAPT = os.environ.get("ACN_FAST_ADAPT", "1") != "0"


def runtime_adapt(*, P, model, data_loader: Iterable, optimizer, steps: Optional[int] = None,
                  active_module: Optional[int] = None, grad_clip: Optional[float] = 1.0,
                  distortion_weight: float = 0.0, proposal=None, interlevel_weight: float = 1.0,
                  n_importance: int = 0, depth_weight: float = 0.0, sight_weight: float = 0.0,
                  depth_eps=None, appearance=None, appearance_reg: float = 0.0) -> Dict[str, float]:
    """runtime_adapt.py:213-315: adapt in place; one pass over the loader (steps=None) or exactly
    ``steps`` updates cycling over it.

    The online stage's configuration -- the routed container (``active_module=None``) with FusedAdam --
    runs through one RoutedAdaptStep per (model, optimizer): the first full batch is an eager update, the
    step is then captured and every later batch of that size replays one HIP graph with no host
    synchronisation; a smaller (ragged last) batch runs the same kernels eagerly.  The loss is read once,
    at the end (the reference reads it every step).  Other configurations take the eager adapt_step, and so does
    every configuration with ``distortion_weight`` > 0 (adapt_step; the RoutedAdaptStep's fused composite-plus-MSE
    kernel has no regulariser, so none is built), and every configuration with ``n_importance`` > 0 or a
    ``proposal``: the proposal-guided step evaluates the model at ``n_importance`` depths and adds
    ``interlevel_weight`` times the interlevel loss; the proposal, whose parameters must be in ``optimizer``, is put in
    training mode too.  ``depth_weight`` / ``sight_weight`` > 0 add depth supervision (adapt_step) and take the eager
    step as well: the loader then yields (rays, rgbs, depths), ``depth_eps`` is the half-width.  With both 0 the loader
    may yield pairs or triples; the depths are not used.  ``appearance`` (an appearance.AppearanceAffine, some of its
    parameters in ``optimizer``) trains on the per-image corrected colour, plus ``appearance_reg`` times its
    regulariser (adapt_step), and takes the eager step as well: the loader then yields
    (rays, rgbs, depths_or_None, img_indices); the module is put in training mode too."""
    geo = bool(depth_weight or sight_weight)
    if geo and depth_eps is None:
        raise ValueError("runtime_adapt: depth_weight / sight_weight need depth_eps")
    device = next(model.parameters()).device
    model.train()
    if proposal is not None:
        proposal.train()
    if appearance is not None:
        appearance.train()
    # the reference clips base.parameters(); parameters outside base get no gradient from the loss
    # (zero_grad sets them to None), so FusedAdam's norm over gradient-carrying tensors is the same
    base = model.submodules[active_module] if active_module is not None else model
    last_loss, step_count = None, 0
    extra = {}
    if proposal is not None:
        extra.update(proposal=proposal, interlevel_weight=interlevel_weight)
    if n_importance:
        extra["n_importance"] = int(n_importance)
    if geo:
        extra.update(depth_weight=float(depth_weight), sight_weight=float(sight_weight), depth_eps=depth_eps)
    if appearance is not None:
        extra.update(appearance=appearance, appearance_reg=float(appearance_reg))
    fast = [None, active_module is None and not distortion_weight and not extra]   # [RoutedAdaptStep, worth trying]
    # use_amp: a fresh GradScaler per call (runtime_adapt.py:237); the cached RoutedAdaptStep's scaler restarts too
    amp = ops.TRAIN_MLP_PRECISION == "amp"
    scaler = torch.amp.GradScaler("cuda") if amp else None
    reset = set()

    def run(rays, rgbs, depths=None, img_indices=None):
        nonlocal last_loss, step_count
        rays, rgbs = rays.to(device, non_blocking=True), rgbs.to(device, non_blocking=True)
        more = {}
        if geo:
            if depths is None:
                raise ValueError("runtime_adapt: depth_weight / sight_weight need loader items (rays, rgbs, depths)")
            more["depths"] = depths.to(device, non_blocking=True)
        if appearance is not None:
            if img_indices is None:
                raise ValueError("runtime_adapt: an appearance model needs loader items (rays, rgbs, depths_or_None, "
                                 "img_indices)")
            more["img_indices"] = img_indices.to(device, non_blocking=True)
        if fast[1] and (fast[0] is None or rays.shape[0] > fast[0].N):
            fast[0] = _routed_step_for(P, base, optimizer, int(rays.shape[0]), grad_clip)
            fast[1] = fast[0] is not None
        if fast[0] is not None:
            if amp and getattr(fast[0], "amp", None) is not None and id(fast[0]) not in reset:
                fast[0].amp.reset()
                reset.add(id(fast[0]))
            last_loss = fast[0](rays, rgbs)
        else:
            last_loss = adapt_step(P, base, rays, rgbs, optimizer, active_module=active_module, grad_clip=grad_clip,
                                   grad_scaler=scaler, distortion_weight=distortion_weight, **extra, **more)
        step_count += 1

    if steps is None:
        for item in data_loader:
            run(*item)
    else:
        it = iter(data_loader)
        while step_count < int(steps):
            try:
                item = next(it)
            except StopIteration:
                it = iter(data_loader)
                item = next(it)
            run(*item)
    if fast[0] is not None:
        fast[0].sync_state()   # host state['step'] current (state_dict, a later eager step)
    return {"loss": 0.0 if last_loss is None else float(last_loss), "steps": step_count}
