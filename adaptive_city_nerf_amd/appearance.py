"""Per-image exposure correction: the per-image affine colour transform of Urban Radiance Fields and
Zip-NeRF.  City captures are taken over hours with auto-exposure and auto white balance on, so the same facade has
another brightness and tint in every image; a field that has to explain all of them with one radiance averages them
and pays the residual as fog.  ``AppearanceAffine`` holds one 3x3 matrix and one offset per training image and
corrects the composited pixel, c = A[s] rgb + b[s] for the ray's image slot s, in linear colour, after compositing
and after the background blend: exposure is multiplicative there, and compositing is linear in colour, so the
correction of the pixel is the correction of every sample.

The module is separate from the field, so the reference's state dicts keep loading unchanged.  The training loss on
the corrected colour and its gradients are one HIP launch (train.appearance_mse_loss, ops.appearance_mse).
"""
from __future__ import annotations

from typing import Sequence, Union

import torch
from torch import Tensor, nn

from . import ops


class AppearanceAffine(nn.Module):
    """``image_ids``: the dataset's image indices that get a slot (need not be contiguous), or an int I for
    ``range(I)``.  ``matrix`` (I, 3, 3) starts at the identity and ``offset`` (I, 3) at zero, so a fresh module
    changes no colour.  An image index without a slot maps to slot -1, the identity."""

    def __init__(self, image_ids: Union[int, Sequence[int]], device=None):
        super().__init__()
        ids = list(range(int(image_ids))) if isinstance(image_ids, int) else [int(i) for i in image_ids]
        if not ids or min(ids) < 0 or len(set(ids)) != len(ids):
            raise ValueError("AppearanceAffine: image_ids must be a non-empty list of distinct indices >= 0 (or their "
                             "number)")
        I = len(ids)
        self.matrix = nn.Parameter(torch.eye(3, dtype=torch.float32, device=device).repeat(I, 1, 1))
        self.offset = nn.Parameter(torch.zeros(I, 3, dtype=torch.float32, device=device))
        lookup = torch.full((max(ids) + 1,), -1, dtype=torch.int32)
        lookup[torch.tensor(ids, dtype=torch.int64)] = torch.arange(I, dtype=torch.int32)
        self.register_buffer("lookup", lookup.to(device))

    @property
    def num_images(self) -> int:
        return int(self.matrix.shape[0])

    def slots(self, img_indices) -> Tensor:
        """(N,) int32 slots of the image indices (a tensor, a list or an int): a device gather without a host read;
        an index outside the table, or without a slot, maps to -1."""
        idx = torch.as_tensor(img_indices, device=self.lookup.device).reshape(-1).to(torch.int64)
        T = self.lookup.shape[0]
        inside = (idx >= 0) & (idx < T)
        s = self.lookup[idx.clamp(0, T - 1)]
        return torch.where(inside, s, torch.full_like(s, -1))

    def forward(self, rgb: Tensor, img_indices) -> Tensor:
        """The corrected colour c_k = sum_j A[s,k,j] rgb_j + b[s,k] of (..., 3) pixels, not clamped; slot -1 leaves
        the pixel as it is.  ``img_indices`` holds one index per pixel, or one for all of them.  One HIP launch
        (ops.appearance_apply) when no gradient is needed, torch ops otherwise."""
        s = self.slots(img_indices)
        n = rgb.numel() // 3
        if s.numel() == 1 and n != 1:
            s = s.expand(n)
        if s.numel() != n:
            raise ValueError(f"AppearanceAffine: {s.numel()} image indices for {n} pixels")
        needs_grad = torch.is_grad_enabled() and (rgb.requires_grad or self.matrix.requires_grad
                                                  or self.offset.requires_grad)
        if rgb.is_cuda and rgb.dtype == torch.float32 and n > 0 and not needs_grad:
            return ops.appearance_apply(rgb, s, self.matrix, self.offset)
        return _apply_torch(rgb, s.to(rgb.device), self.matrix, self.offset)

    def regulariser(self) -> Tensor:
        """mean((A - I)^2) + mean(b^2): keeps the corrections near the identity, so that the field, not the
        per-image terms, explains the scene."""
        eye = torch.eye(3, dtype=self.matrix.dtype, device=self.matrix.device)
        return ((self.matrix - eye) ** 2).mean() + (self.offset ** 2).mean()


def _apply_torch(rgb: Tensor, slots: Tensor, A: Tensor, b: Tensor) -> Tensor:
    """AppearanceAffine.forward as torch ops, differentiable any number of times.  The kernels' arithmetic: the three
    products and three sums in float64, left to right, cast to the colours' dtype once, so that this path and the
    fused one see the same corrected colour."""
    p = rgb.reshape(-1, 3)
    has = (slots >= 0) & (slots < A.shape[0])
    s = slots.clamp(0, A.shape[0] - 1).to(torch.int64)
    p64, A64 = p.double(), A.double()[s]
    c = ((A64[:, :, 0] * p64[:, None, 0] + A64[:, :, 1] * p64[:, None, 1]) + A64[:, :, 2] * p64[:, None, 2]) \
        + b.double()[s]
    return torch.where(has[:, None], c.to(p.dtype), p).view(rgb.shape)
