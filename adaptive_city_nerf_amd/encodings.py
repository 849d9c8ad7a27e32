"""Encoders of the hot path on MI355X (reference interface: models/encodings.py).

HashGridEncoder and SHEncoder keep the reference's constructor arguments, attributes, parameter
names (``hash_table``, state-dict compatible) and forward semantics -- the numerics are those of
the reference's pure-Torch fallback (what the reference runs on ROCm, where tinycudann is
absent), reproduced bit-exactly by the HIP kernels (tests/test_gpu_kernels.py).  Every value of
``implementation`` ("tcnn", "torch", "hip") runs the HIP kernels; there is no CPU path.
"""
from __future__ import annotations

import contextlib
import math
import threading
from typing import Literal, Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import INTERP, AcnError

MAX_SH_DEGREE = 4
INTERPOLATIONS = ["Nearest", "Linear", "Smoothstep"]


def num_sh_bases(degree: int) -> int:
    assert degree <= MAX_SH_DEGREE, f"We don't support degree > {MAX_SH_DEGREE}."
    return (degree + 1) ** 2


def components_from_spherical_harmonics(degree: int, directions: torch.Tensor) -> torch.Tensor:
    """Real SH components of UNIT directions (encodings.py:27-81).  Elementwise utility kept for
    API compatibility; the encoders below use the fused HIP kernel (which also normalises)."""
    assert 0 <= degree <= MAX_SH_DEGREE
    assert directions.shape[-1] == 3
    x, y, z = directions[..., 0], directions[..., 1], directions[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    c = directions.new_zeros((*directions.shape[:-1], num_sh_bases(degree)))
    c[..., 0] = 0.28209479177387814
    if degree > 0:
        c[..., 1] = 0.4886025119029199 * y
        c[..., 2] = 0.4886025119029199 * z
        c[..., 3] = 0.4886025119029199 * x
    if degree > 1:
        c[..., 4] = 1.0925484305920792 * x * y
        c[..., 5] = 1.0925484305920792 * y * z
        c[..., 6] = 0.9461746957575601 * zz - 0.31539156525251999
        c[..., 7] = 1.0925484305920792 * x * z
        c[..., 8] = 0.5462742152960396 * (xx - yy)
    if degree > 2:
        c[..., 9] = 0.5900435899266435 * y * (3 * xx - yy)
        c[..., 10] = 2.890611442640554 * x * y * z
        c[..., 11] = 0.4570457994644658 * y * (5 * zz - 1)
        c[..., 12] = 0.3731763325901154 * z * (5 * zz - 3)
        c[..., 13] = 0.4570457994644658 * x * (5 * zz - 1)
        c[..., 14] = 1.445305721320277 * z * (xx - yy)
        c[..., 15] = 0.5900435899266435 * x * (xx - 3 * yy)
    if degree > 3:
        c[..., 16] = 2.5033429417967046 * x * y * (xx - yy)
        c[..., 17] = 1.7701307697799304 * y * z * (3 * xx - yy)
        c[..., 18] = 0.9461746957575601 * x * y * (7 * zz - 1)
        c[..., 19] = 0.6690465435572892 * y * z * (7 * zz - 3)
        c[..., 20] = 0.10578554691520431 * (35 * zz * zz - 30 * zz + 3)
        c[..., 21] = 0.6690465435572892 * x * z * (7 * zz - 3)
        c[..., 22] = 0.47308734787878004 * (xx - yy) * (7 * zz - 1)
        c[..., 23] = 1.7701307697799304 * x * z * (xx - 3 * yy)
        c[..., 24] = 0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))
    return c


def wants_grad(*ts) -> bool:
    """True when autograd is recording and one of the tensors requires grad.  Every fused or no-grad shortcut of
    the package asks this about its inputs (points, directions, rays) as well as its weights, and takes a
    differentiable path when it holds."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _first_order_only(what: str) -> None:
    """The input-gradient kernels are not differentiable themselves: refuse a backward that records a graph
    (create_graph=True) or runs in a second-order scope, instead of handing back a gradient that autograd would
    treat as constant."""
    from .ray_rendering import _second_order
    if torch.is_grad_enabled() or _second_order():
        raise AcnError(f"{what}: second-order gradients through the input gradient are not implemented on the HIP "
                       "path (create_graph=True / ray_rendering.second_order())")


class _SHFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, levels):
        ctx.save_for_backward(d)
        ctx.levels = levels
        return ops.sh_fwd(d, levels).to(d.dtype)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("SHEncoder")
        return _SHFn._backward(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g):
        (d,) = ctx.saved_tensors
        return ops.sh_bwd(d, g, ctx.levels).to(d.dtype), None


class SHEncoder(nn.Module):
    """Real spherical harmonics of degree levels-1 (encodings.py:84-151) on the HIP kernel."""

    def __init__(self, levels: int = 4, implementation: Literal["tcnn", "torch", "hip"] = "tcnn") -> None:
        super().__init__()
        if levels <= 0 or levels > MAX_SH_DEGREE + 1:
            raise ValueError(f"Supported levels ∈ [1, {MAX_SH_DEGREE + 1}], got {levels}")
        self.levels = int(levels)
        self.degree = self.levels - 1
        self._out_dim = self.levels ** 2
        self.implementation = "hip"

    @property
    def out_dim(self) -> int:
        return self._out_dim

    def forward(self, d: torch.Tensor) -> torch.Tensor:
        assert d.shape[-1] == 3, f"Expected (...,3); got {tuple(d.shape)}"
        if wants_grad(d):
            return _SHFn.apply(d, self.levels)
        return ops.sh_fwd(d, self.levels).to(d.dtype)


_ACC = threading.local()


@contextlib.contextmanager
def accumulate_table_grad():
    """Inside this context a hash-grid backward scatters the table gradient straight into the table's
    existing ``.grad`` buffer (float atomics onto the accumulated values) and hands autograd None for the
    table: no 128 MiB zero-fill for a fresh gradient and no 128 MiB AccumulateGrad add per backward.
    The sum is the same (up to fp32 summation order, which the atomics leave unordered anyway).  Used by
    the graph-replayed meta step, whose persistent .grad buffers are accumulated over its tasks."""
    prev = getattr(_ACC, "on", False)
    _ACC.on = True
    try:
        yield
    finally:
        _ACC.on = prev


class _HashGridFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x01, table, enc):
        if ctx.needs_input_grad[0]:
            # the point gradient reads the table in backward: saved, so that autograd catches an in-place change
            # of it between forward and backward
            ctx.save_for_backward(x01, table)
        else:
            ctx.save_for_backward(x01)
        ctx.enc = enc
        ctx.table = table
        # sampled here: the scope is thread-local and a CUDA backward node runs on autograd's worker thread
        from .ray_rendering import _second_order
        ctx.second_order = _second_order()
        return ops.hashgrid_fwd(x01, table, enc._res_host, enc.log2_hashmap_size, enc.features_per_level,
                                enc._interp_code)

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            if ctx.second_order:
                # the point gradient as an autograd node of its own: differentiable in (x01, g, table) when this
                # backward is recorded, the plain kernel call when not.  The table gradient stays the first-order
                # scatter, a constant of a recorded backward (as in second-order MAML).
                x01, table = ctx.saved_tensors
                gx = _HashGridInputGradFn.apply(x01, g, table, ctx.enc)
                with torch.no_grad():
                    gt = _HashGridFn._backward_table(ctx, g.detach())[1]
                return gx, gt, None
            _first_order_only("HashGridEncoder")
            return _HashGridFn._backward_points(ctx, g)
        return _HashGridFn._backward_table(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward_points(ctx, g):
        x01, table = ctx.saved_tensors
        enc = ctx.enc
        gx = ops.hashgrid_bwd_input(x01, g, table, enc._res_host, enc.log2_hashmap_size, enc.features_per_level,
                                    enc._interp_code).to(x01.dtype)
        return gx, _HashGridFn._backward_table(ctx, g)[1], None

    @staticmethod
    def _backward_table(ctx, g):
        x01 = ctx.saved_tensors[0]
        enc = ctx.enc
        gt = None
        if ctx.needs_input_grad[1]:
            tab = ctx.table
            into = tab.grad if getattr(_ACC, "on", False) and not torch.are_deterministic_algorithms_enabled() else None
            if into is not None and into.shape == tab.shape and into.dtype == torch.float32 and into.is_contiguous():
                ops.hashgrid_bwd(x01, g.contiguous(), enc._res_host, enc.log2_hashmap_size, enc.features_per_level,
                                 enc._interp_code, out=into)
                return None, None, None
            gt = ops.hashgrid_bwd(x01, g.contiguous(), enc._res_host, enc.log2_hashmap_size, enc.features_per_level,
                                  enc._interp_code)
        return None, gt, None


class _HashGridInputGradFn(torch.autograd.Function):
    """grad_x = d sum(out * g) / d x01 of the hash grid as a differentiable function of (x01, g, table): the forward
    is _HashGridFn's point backward (ops.hashgrid_bwd_input, bit for bit), the backward its double backward
    (ops.hashgrid_bwd_input_bwd / _table).  Only reached inside ray_rendering.second_order()."""

    @staticmethod
    def forward(ctx, x01, g, table, enc):
        ctx.save_for_backward(x01, g, table)
        ctx.enc = enc
        return ops.hashgrid_bwd_input(x01, g, table, enc._res_host, enc.log2_hashmap_size, enc.features_per_level,
                                      enc._interp_code).to(x01.dtype)

    @staticmethod
    def backward(ctx, v):
        if torch.is_grad_enabled():
            raise AcnError("HashGridEncoder: third-order gradients (a second-order gradient of the input gradient) "
                           "are not implemented on the HIP path")
        return _HashGridInputGradFn._backward(ctx, v)

    @staticmethod
    @once_differentiable
    def _backward(ctx, v):
        x01, g, table = ctx.saved_tensors
        enc = ctx.enc
        cfg = (enc._res_host, enc.log2_hashmap_size, enc.features_per_level, enc._interp_code)
        need_x, need_g, need_t = ctx.needs_input_grad[:3]
        gg = gx = gt = None
        if need_x or need_g:
            gg, gx = ops.hashgrid_bwd_input_bwd(x01, g, v, table, *cfg, want_gg=need_g, want_gx=need_x)
            gg = gg.to(g.dtype) if need_g else None
            gx = gx.to(x01.dtype) if need_x else None
        if need_t:
            gt = ops.hashgrid_bwd_input_bwd_table(x01, g, v, *cfg).to(table.dtype)
        return gx, gg, gt, None


class HashGridEncoder(nn.Module):
    """Instant-NGP multiresolution hash grid (encodings.py:158-381) on the HIP kernels.

    forward(x: (...,3) in [0,1]) -> (..., levels * features_per_level), level-major.  The table
    is the fp32 parameter ``hash_table`` of shape (levels * 2**log2_hashmap_size, F), initialised
    U(-hash_init_scale, hash_init_scale) as in the reference (:264-268).
    """

    def __init__(self, levels: int = 16, min_res: int = 16, max_res: int = 4096, log2_hashmap_size: int = 19,
                 features_per_level: int = 2, hash_init_scale: float = 1e-3,
                 implementation: Literal["tcnn", "torch", "hip"] = "tcnn",
                 interpolation: Optional[Literal["Nearest", "Linear", "Smoothstep"]] = None) -> None:
        super().__init__()
        self.levels = int(levels)
        self.min_res = int(min_res)
        self.max_res = int(max_res)
        self.features_per_level = int(features_per_level)
        self.log2_hashmap_size = int(log2_hashmap_size)
        self.hash_init_scale = float(hash_init_scale)
        self.hash_table_size = 2 ** self.log2_hashmap_size
        self.interpolation = interpolation
        L = self.levels
        self.growth_factor = 1.0 if L <= 1 else float(math.exp((math.log(self.max_res) - math.log(self.min_res)) / (L - 1)))
        lv = torch.arange(L, dtype=torch.float32)
        scalings = torch.floor(self.min_res * (self.growth_factor ** lv)).to(torch.int32)   # float32 pow, as :211-215
        self.register_buffer("level_resolutions", scalings, persistent=False)
        self.register_buffer("level_offsets", torch.arange(L, dtype=torch.int64) * self.hash_table_size,
                             persistent=False)
        self._res_host = [int(v) for v in scalings.tolist()]
        self._out_dim = self.levels * self.features_per_level
        self.implementation = "hip"
        T = self.hash_table_size * self.levels
        F = self.features_per_level
        self.hash_table = nn.Parameter((torch.rand(T, F) * 2 - 1) * self.hash_init_scale)
        self.register_buffer("hash_primes", torch.tensor([1, 2654435761, 805459861], dtype=torch.int64),
                             persistent=False)
        if self.interpolation is not None and self.interpolation not in INTERPOLATIONS:
            self.interpolation = "Linear"
        self._interp_code = INTERP[self.interpolation or "Linear"]
        self._render_table_dtype = torch.float32

    @property
    def out_dim(self) -> int:
        return self._out_dim

    def get_out_dim(self) -> int:
        return self._out_dim

    def set_render_table_dtype(self, dtype: torch.dtype) -> None:
        """Storage the no-grad field forward and the stratified eval renders gather from: ``torch.float32`` (the
        default: the parameter itself) or ``torch.float16`` (an fp16 copy of it, half the bytes per corner; the
        interpolation and everything after it stay fp32, so the outputs are those of ``hash_table.half().float()``
        bit for bit).  Training, input gradients, the occupancy renderer, the expert-parallel renderer and this
        encoder's own forward keep reading the fp32 parameter, which stays what it is (state-dict key, dtype, shape).
        """
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"render table dtype must be torch.float32 or torch.float16, got {dtype!r}")
        self._render_table_dtype = dtype
        if dtype == torch.float32:
            self.__dict__.pop("_render_shadow", None)

    @property
    def render_table_dtype(self) -> torch.dtype:
        return self.__dict__.get("_render_table_dtype", torch.float32)

    def render_table(self) -> torch.Tensor:
        """The tensor the fused render kernels gather from under set_render_table_dtype: ``hash_table`` itself, or
        its fp16 shadow.  The shadow is a plain attribute (no parameter, no buffer, not in state_dict), converted on
        the current stream by acn_table_to_f16 and refreshed when the parameter's storage or version counter moved
        (optimizer steps, in-place edits and load_state_dict all bump the version) -- the pack cache's rule."""
        tab = self.hash_table
        if self.render_table_dtype == torch.float32:
            return tab
        key = (tab.data_ptr(), tab._version, tab.device)
        shadow = self.__dict__.get("_render_shadow")
        if shadow is None or shadow[0] != key:
            old = shadow[1] if shadow is not None else None
            if old is not None and (old.shape != tab.shape or old.device != tab.device):
                old = None
            shadow = (key, ops.table_to_f16(tab, out=old))
            self.__dict__["_render_shadow"] = shadow
        return shadow[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.shape[-1] == 3, f"Expected (...,3), got {tuple(x.shape)}"
        y = _HashGridFn.apply(x, self.hash_table, self)
        return y.to(x.dtype) if x.dtype != torch.float32 else y


class FrequencyEncoder(nn.Module):
    """NeRF positional encoding (encodings.py:387-444); not on the default hot path
    (dir_encoding='spherical').  Elementwise torch ops, kept for interface completeness."""

    def __init__(self, in_dim: int, pe_dim: int, include_input: bool = True, use_pi: bool = False):
        super().__init__()
        self.in_dim = int(in_dim)
        self.pe_dim = int(pe_dim)
        self.include_input = bool(include_input)
        self.use_pi = bool(use_pi)
        self.register_buffer("bands", 2.0 ** torch.arange(self.pe_dim, dtype=torch.float32), persistent=False)

    @property
    def out_dim(self) -> int:
        return self.in_dim * (2 * self.pe_dim + (1 if self.include_input else 0))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.shape[-1] == self.in_dim, f"Expected (...,{self.in_dim}), got {tuple(x.shape)}"
        fb = self.bands.to(dtype=x.dtype, device=x.device)
        xin = x * (x.new_tensor(math.pi) if self.use_pi else 1)
        xe = xin[..., None] * fb
        pe = torch.cat([torch.cos(xe), torch.sin(xe)], dim=-1).reshape(*x.shape[:-1], -1)
        return torch.cat([x, pe], dim=-1) if self.include_input else pe

    torch_forward = forward
