"""Image evaluation metrics of the online stage: SSIM and PSNR of a rendered frame against its ground truth.

The reference's ``runtime_evaluate`` (pipelines/online_stage/runtime_adapt.py:111, :152-167) reports PSNR, SSIM and
LPIPS per validation image; its SSIM is ``pytorch_msssim.ssim``, a third-party package that is not vendored in the
reference.  This module restates that function's published definition with the same name, arguments, ``(N, C, H, W)``
layout and return values, so the reference's call reads unchanged:

* ``ssim``: Gaussian window (``win_size`` taps, ``win_sigma``), separable "valid" filtering, ``C1 = (K1 data_range)^2``,
  ``C2 = (K2 data_range)^2``, the mean of the SSIM map per image and channel, then over channels (and images with
  ``size_average``).  fp32 HIP tensors take one fused launch (acn_ssim_fwd): float64 arithmetic on the
  fp32 pixels, one fp32 rounding per image and channel, bitwise reproducible, ``ssim(X, X) == 1`` exactly; it is
  differentiable in both images, so ``1 - ssim`` is a training loss.  CPU tensors, other dtypes, windows above 11 taps
  and calls inside ``ray_rendering.second_order()`` take the same formula as float64 torch ops, differentiable any
  number of times.
* ``ssim_image``: the same metric on ``(H, W, C)`` frames, the layout ``render_image`` returns, read in place.
* ``image_metrics`` / ``evaluate_image``: PSNR (``parallel.psnr_reduce``'s formula) and SSIM of a frame in one of the
  reference's colour spaces; render plus metrics in one call.
* ``depth_metrics``: the absolute relative error and the RMSE of a rendered depth against the entries of a target that
  carry a depth (what depth-supervised training, DESIGN.md §4ab, is read against).

One deviation, on purpose: a spatial dimension smaller than ``win_size`` raises ``AcnError``; pytorch_msssim warns and
skips the filter along that dimension.  MS-SSIM, a caller-supplied window, the 3-D (video) form and LPIPS (which needs
pretrained AlexNet weights) are not provided.

Parity with pytorch_msssim itself is UNPINNED (the package and its fixtures do not exist in this environment); the
kernels and the torch form are checked against a direct float64 evaluation of the definition (tests/ssim_ref.py).
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import ops
from ._lib import AcnError
from .color_space import color_space_transformer

__all__ = ["ssim", "ssim_image", "image_metrics", "evaluate_image", "depth_metrics"]


def _gauss_window(win_size: int, win_sigma: float, device) -> Tensor:
    c = torch.arange(win_size, dtype=torch.float64, device=device) - win_size // 2
    g = torch.exp(-(c * c) / (2.0 * float(win_sigma) ** 2))
    return g / g.sum()


def _ssim_torch(X: Tensor, Y: Tensor, win_size: int, win_sigma: float, c1: float, c2: float) -> Tensor:
    """(N, C) SSIM of (N, C, H, W) images: the kernel's formula as float64 torch ops (conv2d with groups = C),
    differentiable any number of times, returned in X's dtype."""
    x, y = X.double(), Y.double()
    C = x.shape[1]
    g = _gauss_window(win_size, win_sigma, x.device)
    gh, gw = g.view(1, 1, -1, 1).expand(C, 1, -1, 1), g.view(1, 1, 1, -1).expand(C, 1, 1, -1)

    def filt(t):
        return F.conv2d(F.conv2d(t, gw, groups=C), gh, groups=C)

    mu1, mu2 = filt(x), filt(y)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu11, filt(y * y) - mu22, filt(x * y) - mu12
    cs = (2.0 * s12 + c2) / (s1 + s2 + c2)
    smap = (2.0 * mu12 + c1) / (mu11 + mu22 + c1) * cs
    out = smap.flatten(2).mean(-1)
    return out.to(X.dtype) if X.dtype.is_floating_point else out


class _SsimFn(torch.autograd.Function):
    """(N, C) SSIM from acn_ssim_fwd.  The launch that produces the value also produces d ssim[n, c] / d X when X
    requires grad; a Y that requires grad costs a second launch with the images swapped (SSIM is symmetric).  The
    backward is g[n, c] times the kept gradient."""

    @staticmethod
    def forward(ctx, X, Y, channels_last, win_size, win_sigma, c1, c2):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        kw = dict(channels_last=channels_last, win_size=win_size, win_sigma=win_sigma, c1=c1, c2=c2)
        val, gx = ops.ssim_fwd(X, Y, want_grad=need_x, **kw)
        gy = ops.ssim_fwd(Y, X, want_grad=True, **kw)[1] if need_y else None
        ctx.set_materialize_grads(False)
        ctx.channels_last = channels_last
        ctx.have = (need_x, need_y)
        ctx.save_for_backward(*[g for g in (gx, gy) if g is not None])
        return val

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        gb = g[:, None, None, :] if ctx.channels_last else g[:, :, None, None]
        saved = list(ctx.saved_tensors)
        gx = gb * saved.pop(0) if ctx.have[0] else None
        gy = gb * saved.pop(0) if ctx.have[1] else None
        return (gx, gy) + (None,) * 5


def _fused(X: Tensor, Y: Tensor, win_size: int) -> bool:
    from .ray_rendering import _second_order
    return (X.is_cuda and Y.is_cuda and X.dtype == torch.float32 and Y.dtype == torch.float32
            and 3 <= win_size <= ops.SSIM_MAX_WIN and not _second_order())


def _ssim_nc(X: Tensor, Y: Tensor, channels_last: bool, data_range, win_size, win_sigma, K) -> Tensor:
    if X.dim() != 4 or X.shape != Y.shape:
        raise AcnError(f"ssim: the images must share one 4-D shape, got {tuple(X.shape)} and {tuple(Y.shape)}")
    win = int(win_size)
    if win % 2 != 1 or win < 1:
        raise AcnError(f"ssim: win_size must be odd, got {win_size}")
    if not float(win_sigma) > 0:
        raise AcnError(f"ssim: win_sigma must be > 0, got {win_sigma}")
    H, W = (X.shape[1], X.shape[2]) if channels_last else (X.shape[2], X.shape[3])
    if H < win or W < win:
        raise AcnError(f"ssim: both spatial dimensions must be >= win_size = {win}, got {H} x {W} "
                       f"(pytorch_msssim would skip the filter along the short one)")
    c1, c2 = (float(K[0]) * float(data_range)) ** 2, (float(K[1]) * float(data_range)) ** 2
    if _fused(X, Y, win):
        return _SsimFn.apply(X, Y, bool(channels_last), win, float(win_sigma), c1, c2)
    if channels_last:
        X, Y = X.permute(0, 3, 1, 2), Y.permute(0, 3, 1, 2)
    return _ssim_torch(X, Y, win, float(win_sigma), c1, c2)


def _reduce(nc: Tensor, size_average: bool, nonnegative_ssim: bool) -> Tensor:
    if nonnegative_ssim:
        nc = torch.relu(nc)
    return nc.mean() if size_average else nc.mean(1)


def ssim(X: Tensor, Y: Tensor, data_range: float = 1.0, size_average: bool = True, win_size: int = 11,
         win_sigma: float = 1.5, K: Tuple[float, float] = (0.01, 0.03), nonnegative_ssim: bool = False) -> Tensor:
    """Structural similarity of two (N, C, H, W) image batches (pytorch_msssim.ssim): a scalar, or (N,) with
    ``size_average=False``.  Differentiable in ``X`` and ``Y``."""
    return _reduce(_ssim_nc(X, Y, False, data_range, win_size, win_sigma, K), size_average, nonnegative_ssim)


def ssim_image(pred_hw3: Tensor, gt_hw3: Tensor, data_range: float = 1.0, size_average: bool = True,
               win_size: int = 11, win_sigma: float = 1.5, K: Tuple[float, float] = (0.01, 0.03),
               nonnegative_ssim: bool = False) -> Tensor:
    """``ssim`` of two (H, W, C) frames, the layout ``render_image`` returns; the fused path reads them in place."""
    if pred_hw3.dim() != 3 or pred_hw3.shape != gt_hw3.shape:
        raise AcnError(f"ssim_image: the frames must share one (H, W, C) shape, got {tuple(pred_hw3.shape)} and "
                       f"{tuple(gt_hw3.shape)}")
    nc = _ssim_nc(pred_hw3.unsqueeze(0), gt_hw3.unsqueeze(0), True, data_range, win_size, win_sigma, K)
    return _reduce(nc, size_average, nonnegative_ssim)


def image_metrics(pred_lin: Tensor, gt_srgb: Tensor, metrics_space: str = "linear") -> Dict[str, float]:
    """{"psnr", "ssim"} of a rendered (H, W, 3) linear frame against its (H, W, 3) sRGB ground truth, both brought
    into ``metrics_space`` by color_space_transformer: PSNR = -10 log10(clamp_min(mse, 1e-8)) as
    parallel.psnr_reduce computes it, SSIM with data_range 1."""
    if pred_lin.dim() != 3 or pred_lin.shape != gt_srgb.shape:
        raise AcnError(f"image_metrics: the frames must share one (H, W, C) shape, got {tuple(pred_lin.shape)} and "
                       f"{tuple(gt_srgb.shape)}")
    p, g = color_space_transformer(pred_lin.detach(), gt_srgb.detach().to(pred_lin.device), metrics_space)
    d = p.double() - g.double()
    mse = max(float((d * d).sum()) / max(float(d.numel()), 1.0), 1e-8)
    return {"psnr": -10.0 * math.log10(mse), "ssim": float(ssim_image(p, g, data_range=1.0))}


def depth_metrics(pred: Tensor, gt: Tensor) -> Dict[str, float]:
    """{"abs_rel", "rmse"} of a rendered depth against a target of the same shape, over the entries where ``gt`` is
    finite and > 0 (NaN marks a pixel without a target, as ray_sampling.point_depth_targets writes it): abs_rel =
    mean |pred - gt| / gt, rmse = sqrt(mean (pred - gt)^2), in float64.  Without any such entry both are NaN."""
    if pred.shape != gt.shape:
        raise AcnError(f"depth_metrics: pred and gt must share one shape, got {tuple(pred.shape)} and "
                       f"{tuple(gt.shape)}")
    g = gt.detach().double().reshape(-1)
    p = pred.detach().to(g.device).double().reshape(-1)
    keep = torch.isfinite(g) & (g > 0)
    if not bool(keep.any()):
        return {"abs_rel": float("nan"), "rmse": float("nan")}
    d, g = p[keep] - g[keep], g[keep]
    return {"abs_rel": float((d.abs() / g).mean()), "rmse": math.sqrt(float((d * d).mean()))}


@torch.no_grad()
def evaluate_image(model, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float, c2w: Tensor, scene_box,
                   gt_srgb: Tensor, metrics_space: str = "linear", **render_kwargs):
    """``render_image`` followed by ``image_metrics``: (rgb (H, W, 3), depth, acc, {"psnr", "ssim"}) of one validation
    view (the per-image body of the reference's runtime_evaluate, without LPIPS).  ``appearance=`` and
    ``image_index=`` among the render arguments correct the frame with that image's affine colour transform
    (render_image) before the metrics are taken."""
    from .ray_rendering import render_image
    rgb, depth, acc = render_image(model, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, c2w=c2w, scene_box=scene_box,
                                   **render_kwargs)
    return rgb, depth, acc, image_metrics(rgb, gt_srgb.view(H, W, -1), metrics_space)
