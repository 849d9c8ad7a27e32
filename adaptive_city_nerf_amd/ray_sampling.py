"""Ray generation (reference interface: nerfs/ray_sampling.py:10-176) on HIP kernels.

get_ray_directions / get_rays / clamp_rays_near_far keep the reference's signatures and output
layouts ((H,W,3) dirs; (H,W,8) or (N,8) packed rays [o, d, near, far]); the arithmetic matches
the reference's CPU ops (tests/test_gpu_kernels.py::test_get_rays_vs_reference).
point_depth_targets (an extension) turns a world-space point cloud into per-pixel depth targets for
ray_rendering.depth_loss.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import ops
from .encodings import _first_order_only, wants_grad
from .scene_box import SceneBox


class _RaysFromDirsFn(torch.autograd.Function):
    """ops.rays_from_dirs under autograd: the forward is the same kernel call (identical values); the backward is
    acn_rays_from_dirs_bwd, the gradient of d_w = R . dir, o = t in the pose and the directions.  The near / far
    columns carry no gradient (the t-values are constants of a pose step, as for differentiable rays).  First
    order only.  Gradients come back in the shape, dtype and device of ``c2w`` and ``directions``; the last row
    of a 4x4 pose gets zeros."""

    @staticmethod
    def forward(ctx, directions, c2w, aabb, near_c, far_c, eps, max_bound, invalid_value):
        ctx.save_for_backward(directions, c2w)
        return ops.rays_from_dirs(directions, c2w, aabb, near_c=near_c, far_c=far_c, eps=eps, max_bound=max_bound,
                                  invalid_value=invalid_value)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("get_rays")
        return _RaysFromDirsFn._backward(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g):
        directions, c2w = ctx.saved_tensors
        want_c, want_d = ctx.needs_input_grad[1], ctx.needs_input_grad[0]
        g_c2w, g_dirs = ops.rays_from_dirs_bwd(directions, c2w, g, want_dirs=want_d)
        gc = None
        if want_c:
            gc = torch.zeros(c2w.shape, dtype=torch.float32, device=g_c2w.device)
            gc[:3, :4] = g_c2w
            gc = gc.to(device=c2w.device, dtype=c2w.dtype)
        gd = g_dirs.view(directions.shape).to(directions.dtype) if want_d else None
        return gd, gc, None, None, None, None, None, None


def _rays_from_dirs(directions: Tensor, c2w: Tensor, aabb, **kw) -> Tensor:
    """(N,8) rays; through autograd when the pose or the directions require grad, else exactly ops.rays_from_dirs."""
    if wants_grad(c2w, directions):
        return _RaysFromDirsFn.apply(directions, c2w, aabb, kw.get("near_c", 0.0), kw.get("far_c", 0.0),
                                     kw.get("eps", 1e-8), kw.get("max_bound", 1e10), kw.get("invalid_value", 1e10))
    return ops.rays_from_dirs(directions, c2w, aabb, **kw)


def _rays_cam_to_world(dirs_cam: Tensor, c2w: Tensor) -> Tuple[Tensor, Tensor]:
    """Camera-frame directions -> world-frame origins & directions (ray_sampling.py:10-24)."""
    rays = _rays_from_dirs(dirs_cam, c2w, None)
    shape = dirs_cam.shape
    return rays[:, :3].reshape(*shape), rays[:, 3:6].reshape(*shape)


def pack_rays(rays_o: Tensor, rays_d: Tensor, near: Tensor, far: Tensor) -> Tensor:
    return torch.cat([rays_o, rays_d, near, far], dim=-1)


def unpack_rays(rays: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    assert rays.shape[-1] == 8, "packed rays must be (..., 8)"
    flat = rays.view(-1, 8).contiguous()
    return flat[:, :3], flat[:, 3:6], flat[:, 6:7], flat[:, 7:8]


def get_rays(directions: Tensor, c2w: Tensor, scene_box: Optional[SceneBox] = None, near: Optional[float] = None,
             far: Optional[float] = None, *, aabb_max_bound: float = 1e10, aabb_invalid_value: float = 1e10) -> Tensor:
    """(H,W,3) -> (H,W,8) or (N,3) -> (N,8) rays [o, d, near, far] (ray_sampling.py:50-108).  A ``c2w`` or
    ``directions`` that requires grad receives its gradient (pose refinement): first order, and none through the
    near / far columns."""
    if directions.ndim == 2 and directions.shape[1] == 3:
        out_shape = (directions.shape[0], 8)
    elif directions.ndim == 3 and directions.shape[-1] == 3:
        out_shape = (*directions.shape[:2], 8)
    else:
        raise ValueError(f"directions must be (H, W, 3) or (N, 3), got {tuple(directions.shape)}")
    if scene_box is None and (near is None or far is None):
        raise ValueError("Provide near/far when scene_box is None")
    rays = _rays_from_dirs(directions, c2w, None if scene_box is None else scene_box.aabb,
                           near_c=float(near or 0.0), far_c=float(far or 0.0), eps=1e-8,
                           max_bound=aabb_max_bound, invalid_value=aabb_invalid_value)
    return rays.view(*out_shape)


def get_ray_directions(H: int, W: int, fx: float, fy: float, cx: float, cy: float, center_pixels: bool,
                       device: torch.device) -> Tensor:
    """Unit camera-frame (RUB) directions (H, W, 3) for pinhole intrinsics (ray_sampling.py:111-136)."""
    return ops.ray_directions(H, W, fx, fy, cx, cy, center_pixels, device)


@torch.no_grad()
def clamp_rays_near_far(rays: Tensor, near_far_override: Optional[Tuple[Optional[float], Optional[float]]], *,
                        eps: float = 1e-6, invalid_value: float = float("inf")) -> Tuple[Tensor, Tensor]:
    """(rays', valid): optional near/far overrides; invalid rays get near=far=invalid_value
    (ray_sampling.py:139-176).  With override None the input is returned unchanged."""
    return ops.clamp_rays(rays, near_far_override, eps=eps, invalid_value=invalid_value)


@torch.no_grad()
def point_depth_targets(points: Tensor, c2w: Tensor, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
                        center_pixels: bool) -> Tensor:
    """(H*W,) fp32 depth targets of one view from world points ``points`` (P, 3), e.g. the sparse SfM cloud of a
    COLMAP reconstruction: each pixel (row-major, the order of get_ray_directions / get_rays) gets the smallest
    distance |X - o| over the points that project into it and lie in front of the camera, NaN where there is none
    (ray_rendering.depth_loss skips such a ray).  The camera is get_ray_directions' (RUB: x right, y up, looking
    along -z): pixel (column i, row j) looks along ((i' - cx) / fx, -(j' - cy) / fy, -1) with i' = i + 0.5 under
    ``center_pixels`` and i otherwise, so a point belongs to the pixel whose ray passes nearest to it: i =
    floor(u) with centred pixels, round(u) without.  For X = o + t d on pixel p's own (unit) ray the target at p is t.
    Plain torch ops in float64 on the points' device (once per image: no hot path)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ops.AcnError(f"point_depth_targets: points must be (P, 3), got {tuple(points.shape)}")
    H, W = int(H), int(W)
    dev = points.device
    X = points.detach().double()
    c = c2w.detach().to(dev).double()[:3, :4]
    rel = X - c[:, 3]
    cam = rel @ c[:, :3]                                  # R^T (X - o): camera-frame coordinates
    depth = -cam[:, 2]                                    # along the viewing direction
    front = depth > 0
    safe = torch.where(front, depth, torch.ones_like(depth))
    u = float(cx) + float(fx) * cam[:, 0] / safe
    v = float(cy) - float(fy) * cam[:, 1] / safe
    shift = 0.0 if center_pixels else 0.5
    i, j = torch.floor(u + shift), torch.floor(v + shift)
    ok = front & torch.isfinite(i) & torch.isfinite(j) & (i >= 0) & (i < W) & (j >= 0) & (j < H)
    pix = (j[ok] * W + i[ok]).long()
    out = torch.full((H * W,), float("inf"), dtype=torch.float64, device=dev)
    out = out.scatter_reduce(0, pix, rel[ok].norm(dim=1), reduce="amin", include_self=True)
    return torch.where(torch.isinf(out), torch.full_like(out, float("nan")), out).float()
