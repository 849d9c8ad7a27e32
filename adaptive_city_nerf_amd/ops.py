"""Tensor-level wrappers over libacnerf.so (include/acnerf.h).

Each function validates shapes the way the reference's asserts do, makes inputs contiguous fp32
device tensors, allocates outputs with the caching allocator and launches on the current stream.
No CPU path exists: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from ._lib import (ACN_BG_CONST, ACN_BG_MLP, ACN_BG_NONE, AcnError, acn_background, acn_expert,
                   acn_routing, check, ptr, require_hip, stream_of)

MLP_KEYS = (
    ("sig_w0", "sigma_trunk.0.linear.weight"), ("sig_b0", "sigma_trunk.0.linear.bias"),
    ("sig_w1", "sigma_trunk.1.linear.weight"), ("sig_b1", "sigma_trunk.1.linear.bias"),
    ("sigh_w", "sigma_head.weight"), ("sigh_b", "sigma_head.bias"),
    ("geo_w", "geo_head.weight"), ("geo_b", "geo_head.bias"),
    ("col_w0", "color_mlp.0.linear.weight"), ("col_b0", "color_mlp.0.linear.bias"),
    ("col_w1", "color_mlp.1.linear.weight"), ("col_b1", "color_mlp.1.linear.bias"),
    ("col_w2", "color_mlp.2.weight"), ("col_b2", "color_mlp.2.bias"),
)
MLP_SHAPES = {
    "sigma_trunk.0.linear.weight": (64, 32), "sigma_trunk.0.linear.bias": (64,),
    "sigma_trunk.1.linear.weight": (64, 64), "sigma_trunk.1.linear.bias": (64,),
    "sigma_head.weight": (1, 64), "sigma_head.bias": (1,),
    "geo_head.weight": (15, 64), "geo_head.bias": (15,),
    "color_mlp.0.linear.weight": (64, 31), "color_mlp.0.linear.bias": (64,),
    "color_mlp.1.linear.weight": (64, 64), "color_mlp.1.linear.bias": (64,),
    "color_mlp.2.weight": (3, 64), "color_mlp.2.bias": (3,),
}


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------
def hashgrid_fwd(x01: torch.Tensor, table: torch.Tensor, resolutions: Sequence[int], log2T: int,
                 F: int, interp: int) -> torch.Tensor:
    require_hip(x01, "HashGridEncoder")
    assert x01.shape[-1] == 3, f"Expected (...,3), got {tuple(x01.shape)}"
    L = len(resolutions)
    x = _f32(x01).view(-1, 3)
    tab = _f32(table)
    if tab.shape != (L << log2T, F):
        raise AcnError(f"hash table must be ({L << log2T}, {F}), got {tuple(tab.shape)}")
    out = torch.empty(x.shape[0], L * F, device=x.device, dtype=torch.float32)
    res = (C.c_int32 * L)(*[int(r) for r in resolutions])
    check(_lib.lib().acn_hashgrid_fwd(ptr(x), x.shape[0], ptr(tab), res, L, log2T, F, interp, ptr(out),
                                      stream_of(x)), "acn_hashgrid_fwd")
    return out.view(*x01.shape[:-1], L * F)


# workspace cap of the deterministic hash-grid backward (~24 B x 8 x L per point, 3 GB at 1M points)
DET_WS_CAP = 1 << 30


def hashgrid_bwd(x01: torch.Tensor, grad_out: torch.Tensor, resolutions: Sequence[int], log2T: int, F: int,
                 interp: int, deterministic: Optional[bool] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Table gradient (scatter-add).  ``deterministic`` (default: torch.are_deterministic_algorithms_enabled())
    selects the sort-based backward (acn_hashgrid_bwd_det: bitwise reproducible, every row summed in point
    order) over the float-atomic one.  ``out``: an existing (L * 2^log2T, F) fp32 buffer the float-atomic
    scatter adds into (accumulation; the deterministic backward accumulates into it too, each row continuing
    its serial sum).  The deterministic workspace (records + sort buffers, ~3 KB per point at L = 16) is
    bounded by processing the points in chunks of at most DET_WS_CAP bytes: the kernel adds every row's
    contributions, in point order, onto the row's current value, so consecutive chunks give exactly the
    serial sum of one pass."""
    L = len(resolutions)
    x = _f32(x01).view(-1, 3)
    g = _f32(grad_out).view(-1, L * F)
    if out is not None:
        if tuple(out.shape) != (L << log2T, F) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("hashgrid_bwd: out must be a contiguous fp32 (L * 2^log2T, F) buffer")
    gt = out if out is not None else torch.zeros(L << log2T, F, device=x.device, dtype=torch.float32)
    res = (C.c_int32 * L)(*[int(r) for r in resolutions])
    if deterministic is None:
        deterministic = torch.are_deterministic_algorithms_enabled()
    if deterministic and F == 2:
        L_ = _lib.lib()
        M = x.shape[0]
        per = max(1, int(L_.acn_hashgrid_bwd_det_workspace_bytes(1 << 16, L, log2T, interp)) >> 16)
        chunk = max(1, min(M, DET_WS_CAP // per))
        ws = torch.empty(max(int(L_.acn_hashgrid_bwd_det_workspace_bytes(chunk, L, log2T, interp)), 1),
                         dtype=torch.uint8, device=x.device)
        for m0 in range(0, M, chunk):
            n = min(chunk, M - m0)
            check(L_.acn_hashgrid_bwd_det(ptr(x[m0:m0 + n]), n, ptr(g[m0:m0 + n]), res, L, log2T, F, interp, ptr(gt),
                                          ptr(ws), ws.numel(), stream_of(x)), "acn_hashgrid_bwd_det")
        return gt
    check(_lib.lib().acn_hashgrid_bwd(ptr(x), x.shape[0], ptr(g), res, L, log2T, F, interp, ptr(gt),
                                      stream_of(x)), "acn_hashgrid_bwd")
    return gt


def hashgrid_bwd_input(x01: torch.Tensor, grad_out: torch.Tensor, table: torch.Tensor, resolutions: Sequence[int],
                       log2T: int, F: int, interp: int) -> torch.Tensor:
    """Gradient of hashgrid_fwd in the points, (..., 3) fp32 (acn_hashgrid_bwd_input): no atomics, bitwise
    reproducible, each point's result independent of the batch around it.  Nearest gives zeros."""
    require_hip(x01, "HashGridEncoder")
    assert x01.shape[-1] == 3, f"Expected (...,3), got {tuple(x01.shape)}"
    L = len(resolutions)
    x = _f32(x01).view(-1, 3)
    g = _f32(grad_out).view(-1, L * F)
    tab = _f32(table)
    if tab.shape != (L << log2T, F):
        raise AcnError(f"hash table must be ({L << log2T}, {F}), got {tuple(tab.shape)}")
    if g.shape[0] != x.shape[0]:
        raise AcnError(f"grad_out must be ({x.shape[0]}, {L * F}), got {tuple(g.shape)}")
    gx = torch.empty(x.shape[0], 3, device=x.device, dtype=torch.float32)
    res = (C.c_int32 * L)(*[int(r) for r in resolutions])
    check(_lib.lib().acn_hashgrid_bwd_input(ptr(x), x.shape[0], ptr(g), ptr(tab), res, L, log2T, F, interp, ptr(gx),
                                            stream_of(x)), "acn_hashgrid_bwd_input")
    return gx.view(*x01.shape[:-1], 3)


def _bwd_input_bwd_args(x01, grad_out, gg_x, resolutions, F):
    require_hip(x01, "HashGridEncoder")
    assert x01.shape[-1] == 3, f"Expected (...,3), got {tuple(x01.shape)}"
    L = len(resolutions)
    x = _f32(x01).view(-1, 3)
    g = _f32(grad_out).view(-1, L * F)
    v = _f32(gg_x).view(-1, 3)
    if g.shape[0] != x.shape[0]:
        raise AcnError(f"grad_out must be ({x.shape[0]}, {L * F}), got {tuple(g.shape)}")
    if v.shape[0] != x.shape[0]:
        raise AcnError(f"gg_x must be ({x.shape[0]}, 3), got {tuple(v.shape)}")
    return x, g, v, L, (C.c_int32 * L)(*[int(r) for r in resolutions])


def hashgrid_bwd_input_bwd(x01: torch.Tensor, grad_out: torch.Tensor, gg_x: torch.Tensor, table: torch.Tensor,
                           resolutions: Sequence[int], log2T: int, F: int, interp: int, want_gg: bool = True,
                           want_gx: bool = True):
    """Double backward of hashgrid_bwd_input, gather side (acn_hashgrid_bwd_input_bwd): with ``gg_x`` (..., 3) the
    cotangent of the point gradient, returns (gg_out (..., L*F) | None, g_x (..., 3) | None), the derivatives of
    sum(gg_x * hashgrid_bwd_input(x01, grad_out, table)) in ``grad_out`` and in ``x01``.  No atomics, bitwise
    reproducible, each point's result independent of the batch around it.  Nearest gives zeros."""
    x, g, v, L, res = _bwd_input_bwd_args(x01, grad_out, gg_x, resolutions, F)
    tab = _f32(table)
    if tab.shape != (L << log2T, F):
        raise AcnError(f"hash table must be ({L << log2T}, {F}), got {tuple(tab.shape)}")
    M = x.shape[0]
    gg = torch.empty(M, L * F, device=x.device, dtype=torch.float32) if want_gg else None
    gx = torch.empty(M, 3, device=x.device, dtype=torch.float32) if want_gx else None
    check(_lib.lib().acn_hashgrid_bwd_input_bwd(ptr(x), M, ptr(g), ptr(v), ptr(tab), res, L, log2T, F, interp,
                                                ptr(gg) if want_gg else None, ptr(gx) if want_gx else None,
                                                stream_of(x)), "acn_hashgrid_bwd_input_bwd")
    lead = x01.shape[:-1]
    return (gg.view(*lead, L * F) if want_gg else None, gx.view(*lead, 3) if want_gx else None)


def hashgrid_bwd_input_bwd_table(x01: torch.Tensor, grad_out: torch.Tensor, gg_x: torch.Tensor,
                                 resolutions: Sequence[int], log2T: int, F: int, interp: int,
                                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Double backward of hashgrid_bwd_input, table side (acn_hashgrid_bwd_input_bwd_table): the derivative of
    sum(gg_x * hashgrid_bwd_input(x01, grad_out, table)) in the table, (L * 2^log2T, F) fp32, scattered with float
    atomics (into ``out``, accumulating, when given).  The sum order is not fixed and there is no sort-based
    variant: under torch.use_deterministic_algorithms(True) this raises instead of being quietly non-deterministic."""
    if torch.are_deterministic_algorithms_enabled():
        raise AcnError("hashgrid_bwd_input_bwd_table: the table gradient of the second-order point gradient is a "
                       "float-atomic scatter with no deterministic variant (torch.use_deterministic_algorithms)")
    x, g, v, L, res = _bwd_input_bwd_args(x01, grad_out, gg_x, resolutions, F)
    if out is not None:
        if tuple(out.shape) != (L << log2T, F) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("hashgrid_bwd_input_bwd_table: out must be a contiguous fp32 (L * 2^log2T, F) buffer")
    gt = out if out is not None else torch.zeros(L << log2T, F, device=x.device, dtype=torch.float32)
    check(_lib.lib().acn_hashgrid_bwd_input_bwd_table(ptr(x), x.shape[0], ptr(g), ptr(v), res, L, log2T, F, interp,
                                                      ptr(gt), stream_of(x)), "acn_hashgrid_bwd_input_bwd_table")
    return gt


def table_to_f16(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 copy of an fp32 tensor, round to nearest even (acn_table_to_f16), on the current stream; written into
    ``out`` (a contiguous float16 tensor of the same shape and device) when given.  The render-table shadow of
    HashGridEncoder.set_render_table_dtype."""
    require_hip(src, "table_to_f16")
    s = _f32(src)
    if out is None:
        out = torch.empty(s.shape, device=s.device, dtype=torch.float16)
    elif out.dtype != torch.float16 or out.shape != s.shape or out.device != s.device or not out.is_contiguous():
        raise ValueError("table_to_f16: out must be a contiguous float16 tensor of src's shape on src's device")
    check(_lib.lib().acn_table_to_f16(ptr(s), s.numel(), ptr(out), stream_of(s)), "acn_table_to_f16")
    return out


def sh_bwd(d: torch.Tensor, g_out: torch.Tensor, levels: int) -> torch.Tensor:
    """Gradient of sh_fwd in the (unnormalised) directions, (..., 3) fp32 (acn_sh_bwd)."""
    require_hip(d, "SHEncoder")
    assert d.shape[-1] == 3, f"Expected (...,3); got {tuple(d.shape)}"
    x = _f32(d).view(-1, 3)
    g = _f32(g_out).view(-1, levels * levels)
    if g.shape[0] != x.shape[0]:
        raise AcnError(f"g_out must be ({x.shape[0]}, {levels * levels}), got {tuple(g.shape)}")
    gd = torch.empty(x.shape[0], 3, device=x.device, dtype=torch.float32)
    check(_lib.lib().acn_sh_bwd(ptr(x), x.shape[0], levels, ptr(g), ptr(gd), stream_of(x)), "acn_sh_bwd")
    return gd.view(*d.shape[:-1], 3)


def sh_fwd(d: torch.Tensor, levels: int) -> torch.Tensor:
    require_hip(d, "SHEncoder")
    assert d.shape[-1] == 3, f"Expected (...,3); got {tuple(d.shape)}"
    x = _f32(d).view(-1, 3)
    out = torch.empty(x.shape[0], levels * levels, device=x.device, dtype=torch.float32)
    check(_lib.lib().acn_sh_fwd(ptr(x), x.shape[0], levels, ptr(out), stream_of(x)), "acn_sh_fwd")
    return out.view(*d.shape[:-1], levels * levels)


# ---------------------------------------------------------------------------------------------
class ExpertSpec:
    """The device-side description of one MetaNGP expert: hash table + level resolutions + AABB +
    the 14 MLP tensors (module parameters or fast weights from a `params` dict).  ``table_fmt``
    ACN_TABLE_F16: ``table`` is the fp16 copy of the hash table (table_to_f16), for the field forward and the
    stratified renders only; a combination the kernels refuse (acn_expert_table_bytes) raises here, before any
    launch, and so does a table tensor smaller than the kernels will address."""

    def __init__(self, table: torch.Tensor, resolutions: Sequence[int], log2T: int, interp: int,
                 aabb_min: Sequence[float], aabb_extent: Sequence[float], mlp: Dict[str, torch.Tensor],
                 F: int = 2, table_fmt: int = _lib.ACN_TABLE_F32):
        self.keep = []
        s = acn_expert()
        if int(table_fmt) == _lib.ACN_TABLE_F16:
            if table.dtype != torch.float16:
                raise AcnError(f"table_fmt ACN_TABLE_F16 needs a float16 table, got {table.dtype}")
            tab = table.detach().contiguous()
        else:
            tab = _f32(table)
        self.keep.append(tab)
        s.table = ptr(tab)
        s.L = len(resolutions)
        s.log2T = int(log2T)
        s.F = int(F)
        s.interp = int(interp)
        s.table_fmt = int(table_fmt)
        table_bytes = getattr(_lib.lib(), "acn_expert_table_bytes", None)
        if table_bytes is None:   # a developer library (ACNERF_LIB) from before table_fmt: fp32 experts only
            if s.table_fmt != _lib.ACN_TABLE_F32:
                raise AcnError(f"{_lib.LIB_PATH} predates acn_expert.table_fmt: fp32 tables only")
            need = 0
        else:
            need = int(table_bytes(C.byref(s)))
            if need == 0:   # the refusal's message is in acn_last_error
                check(-2, "acn_expert_table_bytes")
        if tab.numel() * tab.element_size() < need:
            raise AcnError(f"hash table holds {tab.numel() * tab.element_size()} bytes, the fused kernels address "
                           f"{need} (L={s.L}, log2T={s.log2T}, F={s.F}, table_fmt={s.table_fmt})")
        for i, r in enumerate(resolutions):
            s.res[i] = int(r)
        s.aabb_min[:] = [float(v) for v in aabb_min]
        s.aabb_extent[:] = [float(v) for v in aabb_extent]
        for field, key in MLP_KEYS:
            if key not in mlp:
                raise AcnError(f"missing MLP tensor {key!r}")
            t = _f32(mlp[key])
            if tuple(t.shape) != MLP_SHAPES[key]:
                raise AcnError(f"the fused HIP field supports the reference architecture (nerf_runner.py:102-121); "
                               f"{key} has shape {tuple(t.shape)}, expected {MLP_SHAPES[key]}")
            self.keep.append(t)
            setattr(s, field, ptr(t))
        self.s = s
        self.device = tab.device


def make_routing(centroids: torch.Tensor, K: int, cluster_2d: bool, boundary_margin: float) -> acn_routing:
    r = acn_routing()
    r.K = int(K)
    r.cluster_2d = int(bool(cluster_2d))
    r.boundary_margin = float(boundary_margin)
    c = centroids.detach().float().cpu()
    for k in range(K):
        for a in range(3):
            r.centroids[k][a] = float(c[k, a])
    return r


def make_background(mode: str, color=None, mlp: Optional[Dict[str, torch.Tensor]] = None):
    b = acn_background()
    keep = []
    if mode == "mlp":
        b.mode = ACN_BG_MLP
        w1 = _f32(mlp["0.weight"]); b1 = _f32(mlp["0.bias"]); w2 = _f32(mlp["2.weight"]); b2 = _f32(mlp["2.bias"])
        if w1.shape[1] != 16 or w2.shape[0] != 3:
            raise AcnError("background MLP must be Linear(16, H) -> Linear(H, 3)")
        keep += [w1, b1, w2, b2]
        b.hidden = int(w1.shape[0])
        b.w1, b.b1, b.w2, b.b2 = ptr(w1), ptr(b1), ptr(w2), ptr(b2)
    elif mode == "const":
        b.mode = ACN_BG_CONST
        b.color[:] = [float(v) for v in color]
    else:
        b.mode = ACN_BG_NONE
    return b, keep


def _experts_array(experts: Sequence[ExpertSpec]):
    return (acn_expert * len(experts))(*[e.s for e in experts])


def pack_experts(experts: Sequence[ExpertSpec], routing: acn_routing, active_module: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MFMA-ordered weight image of the experts the next fused call evaluates (acn_pack_experts)."""
    K = 1 if active_module is not None else routing.K
    nbytes = int(_lib.lib().acn_workspace_bytes(K))
    dev = experts[0].device
    if out is None or out.numel() * 4 < nbytes or out.device != dev:
        out = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    arr = _experts_array(experts)
    check(_lib.lib().acn_pack_experts(arr, C.byref(routing), -1 if active_module is None else int(active_module),
                                      ptr(out), out.numel() * 4, int(torch.cuda.current_stream(dev).cuda_stream)),
          "acn_pack_experts")
    return out


class PackCache:
    """Re-packs only when the (module-owned) weights changed: the key is built from the identity,
    storage and version counter of every packed tensor (in-place updates and load_state_dict bump
    the version).  Fast-weight dicts are never cached (their storage is recycled per step)."""

    def __init__(self):
        self.key = None
        self.ws = None

    def get(self, experts: Sequence[ExpertSpec], routing: acn_routing, active_module: Optional[int], key):
        if key is not None and key == self.key and self.ws is not None:
            return self.ws
        self.ws = pack_experts(experts, routing, active_module, out=self.ws)
        self.key = key
        return self.ws


# Optional timing hook (bench.py): when set to a list, render_stratified / field_fwd append a pair of
# recorded HIP events bracketing exactly the fused kernel on the launch stream.
EVENT_HOOK = None


def field_fwd(x: torch.Tensor, experts: Sequence[ExpertSpec], routing: acn_routing,
              active_module: Optional[int] = None, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    require_hip(x, "MetaContainer.forward")
    assert x.dim() == 2 and x.shape[-1] >= 6, "x must be (N,D>=6)"
    xx = _f32(x)
    M = xx.shape[0]
    out = torch.empty(M, 4, device=xx.device, dtype=torch.float32)
    if M == 0:
        return out
    ws = packed if packed is not None else pack_experts(experts, routing, active_module)
    arr = _experts_array(experts)
    hook = EVENT_HOOK
    if hook is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.lib().acn_field_fwd(ptr(xx), M, xx.shape[1], arr, C.byref(routing),
                                   -1 if active_module is None else int(active_module), ptr(ws),
                                   ws.numel() * 4, ptr(out), stream_of(xx)), "acn_field_fwd")
    if hook is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        hook.append((e0, e1))
    return out



# Default of render_stratified(reorder=None): direction-sorted visiting order for small batches
# (acn_render_stratified_fwd_ordered; outputs are identical either way, only the speed changes).
REORDER = True


def render_stratified(rays: torch.Tensor, S: int, experts: Sequence[ExpertSpec], routing: acn_routing,
                      active_module: Optional[int], background, sigma_scale: float = 1.0, tau: float = 0.0,
                      jitter: Optional[torch.Tensor] = None, want_weights: bool = True,
                      packed: Optional[torch.Tensor] = None, reorder: Optional[bool] = None):
    require_hip(rays, "render_rays")
    assert rays.dim() == 2 and rays.shape[-1] == 8, "rays must be (N,8)"
    r = _f32(rays)
    N = r.shape[0]
    dev = r.device
    rgb = torch.empty(N, 3, device=dev, dtype=torch.float32)
    depth = torch.empty(N, device=dev, dtype=torch.float32)
    acc = torch.empty(N, device=dev, dtype=torch.float32)
    weights = torch.empty(N, S, device=dev, dtype=torch.float32) if want_weights else None
    if N == 0:
        return rgb, depth, weights, acc
    ws = packed if packed is not None else pack_experts(experts, routing, active_module)
    arr = _experts_array(experts)
    jit = None if jitter is None else _f32(jitter)
    # scratch for the ray visiting order (small batches; the outputs do not depend on it)
    obytes = int(_lib.lib().acn_render_order_bytes(N)) if (REORDER if reorder is None else reorder) else 0
    order = torch.empty(obytes // 4, device=dev, dtype=torch.int32) if obytes else None
    hook = EVENT_HOOK
    if hook is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.lib().acn_render_stratified_fwd_ordered(
        ptr(r), N, int(S), ptr(jit), arr, C.byref(routing), -1 if active_module is None else int(active_module),
        C.byref(background), float(sigma_scale), float(tau), ptr(ws), ws.numel() * 4, ptr(rgb), ptr(depth),
        ptr(weights), ptr(acc), ptr(order), obytes, stream_of(r)), "acn_render_stratified_fwd_ordered")
    if hook is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        hook.append((e0, e1))
    return rgb, depth, weights, acc


def _is_f16_expert(e: ExpertSpec) -> bool:
    return int(e.s.table_fmt) == _lib.ACN_TABLE_F16


def render_depths(rays: torch.Tensor, t_vals: torch.Tensor, experts: Sequence[ExpertSpec], routing: acn_routing,
                  active_module: Optional[int], background, sigma_scale: float = 1.0, tau: float = 0.0,
                  want_weights: bool = True, packed: Optional[torch.Tensor] = None, reorder: Optional[bool] = None):
    """render_stratified at the caller's depths: sample s of ray n at ``t_vals[n, s]`` ((N, S >= 2), non-decreasing
    along a ray; near / far of the rays are not read), one fused launch (acn_render_depths_fwd).  The depths are
    not validated: a NaN or unsorted row spoils that ray's outputs only.  fp32 hash tables only."""
    assert rays.dim() == 2 and rays.shape[-1] == 8, "rays must be (N,8)"
    N = rays.shape[0]
    if t_vals.dim() != 2 or t_vals.shape[0] != N or t_vals.shape[1] < 2:
        raise AcnError(f"render_depths: t_vals must be ({N}, S >= 2), got {tuple(t_vals.shape)}")
    require_hip(rays, "render_depths")
    if t_vals.device != rays.device:
        raise AcnError(f"render_depths: t_vals is on {t_vals.device}, the rays on {rays.device}")
    if any(_is_f16_expert(e) for e in experts):
        raise AcnError("render_depths: fp16 hash tables are rendered by render_stratified only; pass the fp32 experts")
    r = _f32(rays)
    t = _f32(t_vals)
    S = t.shape[1]
    dev = r.device
    rgb = torch.empty(N, 3, device=dev, dtype=torch.float32)
    depth = torch.empty(N, device=dev, dtype=torch.float32)
    acc = torch.empty(N, device=dev, dtype=torch.float32)
    weights = torch.empty(N, S, device=dev, dtype=torch.float32) if want_weights else None
    if N == 0:
        return rgb, depth, weights, acc
    ws = packed if packed is not None else pack_experts(experts, routing, active_module)
    arr = _experts_array(experts)
    obytes = int(_lib.lib().acn_render_order_bytes(N)) if (REORDER if reorder is None else reorder) else 0
    order = torch.empty(obytes // 4, device=dev, dtype=torch.int32) if obytes else None
    hook = EVENT_HOOK
    if hook is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.lib().acn_render_depths_fwd(
        ptr(r), N, int(S), ptr(t), arr, C.byref(routing), -1 if active_module is None else int(active_module),
        C.byref(background), float(sigma_scale), float(tau), ptr(ws), ws.numel() * 4, ptr(rgb), ptr(depth),
        ptr(weights), ptr(acc), ptr(order), obytes, stream_of(r)), "acn_render_depths_fwd")
    if hook is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        hook.append((e0, e1))
    return rgb, depth, weights, acc


def volume_render(rgb_sigma: torch.Tensor, t_vals: torch.Tensor, bg_rgb: Optional[torch.Tensor] = None,
                  raw_rgb: bool = False, raw_sigma: bool = False, sigma_scale: float = 1.0):
    require_hip(rgb_sigma, "volume_render")
    rs = _f32(rgb_sigma)
    t = _f32(t_vals)
    N, S = t.shape
    assert rs.shape == (N, S, 4), f"rgb_sigma must be (N,S,4), got {tuple(rs.shape)}"
    dev = rs.device
    bg = None if bg_rgb is None else _f32(bg_rgb.to(dev)).view(N, 3)
    rgb = torch.empty(N, 3, device=dev, dtype=torch.float32)
    depth = torch.empty(N, device=dev, dtype=torch.float32)
    w = torch.empty(N, S, device=dev, dtype=torch.float32)
    acc = torch.empty(N, device=dev, dtype=torch.float32)
    check(_lib.lib().acn_volume_render_fwd(ptr(rs), ptr(t), ptr(bg), N, S, int(raw_rgb), int(raw_sigma),
                                           float(sigma_scale), ptr(rgb), ptr(depth), ptr(w), ptr(acc),
                                           stream_of(rs)), "acn_volume_render_fwd")
    return rgb, depth, w, acc


def volume_render_bwd(rgb_sigma: torch.Tensor, t_vals: torch.Tensor, bg_rgb: Optional[torch.Tensor], sigma_scale: float,
                      g_rgb, g_depth, g_weights, g_acc):
    """dL/d(rgb_sigma), dL/d(bg) of volume_render (raw flags off) for the given output gradients."""
    rs = _f32(rgb_sigma)
    t = _f32(t_vals)
    N, S = t.shape
    dev = rs.device
    bg = None if bg_rgb is None else _f32(bg_rgb.to(dev)).view(N, 3)
    gr = None if g_rgb is None else _f32(g_rgb).view(N, 3)
    gd = None if g_depth is None else _f32(g_depth).view(N)
    gw = None if g_weights is None else _f32(g_weights).view(N, S)
    ga = None if g_acc is None else _f32(g_acc).view(N)
    g_rs = torch.empty(N, S, 4, device=dev, dtype=torch.float32)
    g_bg = torch.empty(N, 3, device=dev, dtype=torch.float32) if bg is not None else None
    check(_lib.lib().acn_volume_render_bwd(ptr(rs), ptr(t), ptr(bg), N, S, float(sigma_scale), ptr(gr), ptr(gd),
                                           ptr(gw), ptr(ga), ptr(g_rs), ptr(g_bg), stream_of(rs)),
          "acn_volume_render_bwd")
    return g_rs, g_bg


def mse_linear_fwd(pred: torch.Tensor, gt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """compute_mse_loss's loss in color_space 'linear' (acn_mse_linear_fwd): a 0-d device tensor (written into
    ``out``, a one-element fp32 tensor on the same device, when given)."""
    p, g = _f32(pred).reshape(-1), _f32(gt).reshape(-1)
    if p.numel() != g.numel() or p.numel() == 0:
        raise ValueError(f"mse_linear: pred / gt sizes {p.numel()} / {g.numel()}")
    if out is None:
        out = torch.empty((), device=p.device, dtype=torch.float32)
    elif out.numel() != 1 or out.dtype != torch.float32 or out.device != p.device:
        raise ValueError("mse_linear_fwd: out must be a one-element fp32 tensor on the inputs' device")
    ws = _mse_ws(p.device)
    check(_lib.lib().acn_mse_linear_fwd_ws(ptr(p), ptr(g), p.numel(), ptr(out), ptr(ws), ws.numel(), stream_of(p)),
          "acn_mse_linear_fwd_ws")
    return out


_MSE_WS = {}


def _mse_ws(device) -> torch.Tensor:
    """Zeroed workspace of acn_mse_linear_fwd_ws per (device, stream): its ticket counter returns to 0
    after every call, so one buffer serves every later call on that stream.  Under stream capture every
    captured call gets a workspace of its own: graphs captured on torch's shared capture stream would
    otherwise share one ticket counter, and two of them replayed concurrently would race on it."""
    if torch.cuda.is_current_stream_capturing():
        ws = torch.zeros(int(_lib.lib().acn_mse_linear_workspace_bytes()), dtype=torch.uint8, device=device)
        return _lib.capture_keepalive(ws)   # lives as long as the graph it is baked into
    key = (device, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _MSE_WS.get(key)
    if ws is None:
        ws = _MSE_WS[key] = torch.zeros(int(_lib.lib().acn_mse_linear_workspace_bytes()), dtype=torch.uint8,
                                        device=device)
    return ws


def mse_linear_bwd(pred: torch.Tensor, gt: torch.Tensor, g_loss: torch.Tensor) -> torch.Tensor:
    p, g = _f32(pred).reshape(-1), _f32(gt).reshape(-1)
    gl = _f32(g_loss.reshape(1))
    out = torch.empty_like(p)
    check(_lib.lib().acn_mse_linear_bwd(ptr(p), ptr(g), p.numel(), ptr(gl), ptr(out), stream_of(p)),
          "acn_mse_linear_bwd")
    return out.view(pred.shape)


_APPEARANCE_WS = {}


def _appearance_ws(device, I: int) -> torch.Tensor:
    """Zeroed workspace of acn_appearance_mse per (device, stream), handled like _mse_ws: the ticket counter returns
    to 0 after every call, and under stream capture every captured call gets a workspace of its own."""
    nbytes = int(_lib.lib().acn_appearance_mse_workspace_bytes(int(I)))
    if torch.cuda.is_current_stream_capturing():
        return _lib.capture_keepalive(torch.zeros(nbytes, dtype=torch.uint8, device=device))
    key = (device, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _APPEARANCE_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _APPEARANCE_WS[key] = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    return ws


def _appearance_args(rgb, slots, A, b, what: str):
    """The (N, 3) colours, (N,) int32 slots, (I, 3, 3) matrices and (I, 3) offsets as contiguous device tensors."""
    require_hip(rgb, what)
    p = _f32(rgb).reshape(-1, 3)
    N = p.shape[0]
    s = slots.detach().reshape(-1)
    if s.dtype != torch.int32:
        s = s.to(torch.int32)
    s = s.contiguous()
    Av, bv = _f32(A), _f32(b)
    if Av.dim() != 3 or Av.shape[1:] != (3, 3) or Av.shape[0] < 1 or bv.shape != (Av.shape[0], 3):
        raise AcnError(f"{what}: A must be (I >= 1, 3, 3) and b (I, 3), got {tuple(A.shape)} and {tuple(b.shape)}")
    if s.numel() != N or any(t.device != p.device for t in (s, Av, bv)):
        raise AcnError(f"{what}: slots must be ({N},) and slots, A, b on the colours' device, got "
                       f"{tuple(slots.shape)} on {slots.device}, A on {A.device}, b on {b.device}")
    return p, s, Av, bv, N, int(Av.shape[0])


def appearance_mse(pred: torch.Tensor, gt: torch.Tensor, slots: torch.Tensor, A: torch.Tensor, b: torch.Tensor,
                   want_grad: bool = True):
    """(loss, g_pred, g_A, g_b) of the linear-colour MSE on the per-image corrected prediction
    c = A[slot] pred + b[slot] (acn_appearance_mse): loss = mean((clamp01(c) - gt_linear(gt))^2) as a
    0-d tensor and, at g_loss = 1, its gradients to ``pred`` (N, 3), ``A`` (I, 3, 3) and ``b`` (I, 3), from one
    launch.  A slot outside [0, I) is the identity and reaches no parameter; a slot no ray has gets exact zeros.
    Sums in float64, one fp32 rounding per output, bitwise reproducible, no host synchronisation.  With
    ``want_grad=False`` the gradients are None and the loss has the same bits."""
    p, s, Av, bv, N, I = _appearance_args(pred, slots, A, b, "appearance_mse")
    g = _f32(gt).reshape(-1, 3)
    if N == 0 or g.shape[0] != N or g.device != p.device:
        raise AcnError(f"appearance_mse: pred / gt must both be (N >= 1, 3) on one device, got {tuple(pred.shape)} "
                       f"and {tuple(gt.shape)}")
    loss = torch.empty((), device=p.device, dtype=torch.float32)
    g_pred = g_A = g_b = None
    if want_grad:
        g_pred, g_A, g_b = torch.empty_like(p), torch.empty_like(Av), torch.empty_like(bv)
    ws = _appearance_ws(p.device, I)
    check(_lib.lib().acn_appearance_mse(ptr(p), ptr(g), ptr(s), N, ptr(Av), ptr(bv), I, ptr(loss), ptr(g_pred),
                                        ptr(g_A), ptr(g_b), ptr(ws), ws.numel(), stream_of(p)), "acn_appearance_mse")
    return loss, (None if g_pred is None else g_pred.view(pred.shape)), g_A, g_b


def appearance_apply(rgb: torch.Tensor, slots: torch.Tensor, A: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """c = A[slot] rgb + b[slot] per pixel (acn_appearance_apply), evaluated in float64 and rounded once, not clamped;
    a slot outside [0, I) returns the input bits.  ``rgb`` is (..., 3) with one slot per pixel."""
    p, s, Av, bv, N, I = _appearance_args(rgb, slots, A, b, "appearance_apply")
    out = torch.empty_like(p)
    check(_lib.lib().acn_appearance_apply(ptr(p), ptr(s), N, ptr(Av), ptr(bv), I, ptr(out), stream_of(p)),
          "acn_appearance_apply")
    return out.view(rgb.shape)


def get_rays_image(H: int, W: int, fx: float, fy: float, cx: float, cy: float, c2w: torch.Tensor,
                   aabb: Optional[torch.Tensor], device, center_pixels: bool = True, near: Optional[float] = None,
                   far: Optional[float] = None, near_far_override=None, apply_clamp: bool = True):
    c = c2w.detach().float().cpu().contiguous()[:3, :4].contiguous()
    c_arr = (C.c_float * 12)(*c.view(-1).tolist())
    a_arr = None
    if aabb is not None:
        a = aabb.detach().float().cpu().contiguous().view(-1)
        a_arr = (C.c_float * 6)(*a.tolist())
    hn = hf = 0
    nv = fv = 0.0
    if near_far_override is not None:
        if near_far_override[0] is not None:
            hn, nv = 1, float(near_far_override[0])
        if near_far_override[1] is not None:
            hf, fv = 1, float(near_far_override[1])
    rays = torch.empty(H * W, 8, device=device, dtype=torch.float32)
    valid = torch.empty(H * W, device=device, dtype=torch.uint8)
    check(_lib.lib().acn_get_rays(int(H), int(W), float(fx), float(fy), float(cx), float(cy), int(center_pixels),
                                  c_arr, a_arr, float(near or 0.0), float(far or 0.0), hn, nv, hf, fv,
                                  int(apply_clamp), ptr(rays), ptr(valid), stream_of(rays)), "acn_get_rays")
    return rays, valid.bool()


def _host_f32(t, n):
    v = t.detach().float().cpu().contiguous().view(-1)
    if v.numel() != n:
        raise AcnError(f"expected {n} values, got {v.numel()}")
    return (C.c_float * n)(*v.tolist())


def ray_directions(H: int, W: int, fx: float, fy: float, cx: float, cy: float, center_pixels: bool, device):
    dirs = torch.empty(H, W, 3, device=device, dtype=torch.float32)
    check(_lib.lib().acn_ray_directions(int(H), int(W), float(fx), float(fy), float(cx), float(cy),
                                        int(center_pixels), ptr(dirs), stream_of(dirs)), "acn_ray_directions")
    return dirs


def rays_from_dirs(dirs: torch.Tensor, c2w: torch.Tensor, aabb: Optional[torch.Tensor], near_c: float = 0.0,
                   far_c: float = 0.0, eps: float = 1e-8, max_bound: float = 1e10, invalid_value: float = 1e10):
    require_hip(dirs, "get_rays")
    d = _f32(dirs).view(-1, 3)
    rays = torch.empty(d.shape[0], 8, device=d.device, dtype=torch.float32)
    c = _host_f32(c2w[:3, :4], 12)
    a = None if aabb is None else _host_f32(aabb, 6)
    check(_lib.lib().acn_rays_from_dirs(ptr(d), d.shape[0], c, a, float(near_c), float(far_c), float(eps),
                                        float(max_bound), float(invalid_value), ptr(rays), stream_of(d)),
          "acn_rays_from_dirs")
    return rays


def rays_from_dirs_bwd(dirs: torch.Tensor, c2w: torch.Tensor, g_rays: torch.Tensor, want_dirs: bool = True):
    """Backward of rays_from_dirs in the pose and the directions (acn_rays_from_dirs_bwd): g_c2w (3,4) fp32 on the
    rays' device and g_dirs (N,3) fp32 (None without ``want_dirs``) from dL/drays (N,8).  Columns 6:8 of g_rays
    (near, far) are ignored: the t-values are constants of a pose step.  Deterministic (double partial sums added
    in a fixed order, no atomics)."""
    require_hip(dirs, "get_rays")
    d = _f32(dirs).view(-1, 3)
    g = _f32(g_rays).view(-1, 8)
    N = d.shape[0]
    if g.shape[0] != N:
        raise AcnError(f"g_rays must be ({N}, 8), got {tuple(g.shape)}")
    c = _host_f32(c2w[:3, :4], 12)
    g_c2w = torch.empty(3, 4, device=d.device, dtype=torch.float32)
    g_dirs = torch.empty(N, 3, device=d.device, dtype=torch.float32) if want_dirs else None
    L = _lib.lib()
    ws = torch.empty(int(L.acn_rays_from_dirs_bwd_workspace_bytes(N)) // 8, dtype=torch.float64, device=d.device)
    check(L.acn_rays_from_dirs_bwd(ptr(d), N, c, ptr(g), ptr(g_c2w), ptr(g_dirs), ptr(ws), ws.numel() * 8,
                                   stream_of(d)), "acn_rays_from_dirs_bwd")
    return g_c2w, g_dirs


def ray_aabb(origins: torch.Tensor, dirs: torch.Tensor, aabb: torch.Tensor, eps: float, max_bound: float,
             invalid_value: float):
    require_hip(origins, "SceneBox.ray_aabb_intersect")
    o = _f32(origins).view(-1, 3)
    d = _f32(dirs.to(o.device)).view(-1, 3)
    tmin = torch.empty(o.shape[0], device=o.device, dtype=torch.float32)
    tmax = torch.empty_like(tmin)
    check(_lib.lib().acn_ray_aabb(ptr(o), ptr(d), o.shape[0], _host_f32(aabb, 6), float(eps), float(max_bound),
                                  float(invalid_value), ptr(tmin), ptr(tmax), stream_of(o)), "acn_ray_aabb")
    return tmin, tmax


def clamp_rays(rays: torch.Tensor, near_far_override, eps: float = 1e-6, invalid_value: float = float("inf")):
    """Returns (rays', valid).  rays' is a new tensor unless override is None (then rays itself)."""
    require_hip(rays, "clamp_rays_near_far")
    apply = near_far_override is not None
    r = _f32(rays).clone() if apply else _f32(rays)
    hn = hf = 0
    nv = fv = 0.0
    if apply:
        if near_far_override[0] is not None:
            hn, nv = 1, float(near_far_override[0])
        if near_far_override[1] is not None:
            hf, fv = 1, float(near_far_override[1])
    valid = torch.empty(r.shape[0], device=r.device, dtype=torch.uint8)
    check(_lib.lib().acn_clamp_rays(ptr(r), r.shape[0], int(apply), hn, nv, hf, fv, float(eps), float(invalid_value),
                                    ptr(valid), stream_of(r)), "acn_clamp_rays")
    return (r if apply else rays), valid.bool()


def routing_fwd(pts: torch.Tensor, routing: acn_routing):
    require_hip(pts, "MetaContainer._routing")
    p = _f32(pts)
    M = p.shape[0]
    if routing.boundary_margin > 1.0:
        W = torch.empty(M, routing.K, device=p.device, dtype=torch.float32)
        check(_lib.lib().acn_routing_fwd(ptr(p), M, p.shape[1], C.byref(routing), ptr(W), None, stream_of(p)),
              "acn_routing_fwd")
        return W, None
    hard = torch.empty(M, device=p.device, dtype=torch.int32)
    check(_lib.lib().acn_routing_fwd(ptr(p), M, p.shape[1], C.byref(routing), None, ptr(hard), stream_of(p)),
          "acn_routing_fwd")
    return None, hard.long()


def background_fwd(dirs: torch.Tensor, background) -> torch.Tensor:
    require_hip(dirs, "MetaContainer.background_color")
    d = _f32(dirs).view(-1, 3)
    out = torch.empty(d.shape[0], 3, device=d.device, dtype=torch.float32)
    check(_lib.lib().acn_background_fwd(ptr(d), d.shape[0], C.byref(background), ptr(out), stream_of(d)),
          "acn_background_fwd")
    return out


def background_bwd(dirs: torch.Tensor, background, g_out: torch.Tensor, grads: Sequence[torch.Tensor]) -> None:
    """Gradients of the MLP background head's four tensors (written into ``grads`` = [gw1, gb1, gw2, gb2],
    overwritten) for dL/d(bg rgb) ``g_out`` (N,3) (acn_background_bwd)."""
    d = _f32(dirs).view(-1, 3)
    g = _f32(g_out).view(-1, 3)
    for t in grads:
        if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == d.device):
            raise AcnError("background_bwd: gradient buffers must be contiguous fp32 on the rays' device")
    L = _lib.lib()
    if torch.cuda.is_current_stream_capturing():   # one workspace per captured call (see _mse_ws)
        ws = _lib.capture_keepalive(torch.empty(int(L.acn_background_bwd_workspace_bytes()), dtype=torch.uint8,
                                                device=d.device))
    else:
        key = (d.device, int(torch.cuda.current_stream(d.device).cuda_stream))
        ws = _BG_WS.get(key)
        if ws is None:
            ws = _BG_WS[key] = torch.empty(int(L.acn_background_bwd_workspace_bytes()), dtype=torch.uint8,
                                           device=d.device)
    check(L.acn_background_bwd(ptr(d), d.shape[0], C.byref(background), ptr(g), *[ptr(t) for t in grads], ptr(ws),
                               ws.numel(), stream_of(d)), "acn_background_bwd")


_BG_WS = {}


# ------------------------------------------------------------------------------------------
# expert MLP of the training path (mlp_train.hip)
MLP_SAVE_COLS, MLP_GRAD_COLS = 325, 275


def _mlp_struct(ws: Sequence[torch.Tensor]):
    from ._lib import acn_mlp
    w = acn_mlp()
    for name, t in zip(("w0", "b0", "w1", "b1", "wsh", "bsh", "wg", "bg", "wc0", "bc0", "wc1", "bc1", "wc2", "bc2"), ws):
        if not (t.is_contiguous() and t.dtype == torch.float32):
            raise AcnError(f"mlp_train: {name} must be a contiguous fp32 tensor")
        setattr(w, name, t.data_ptr())
    return w


MLP_GROUP = 2048


def _mlp_ws(device):
    return torch.empty(int(mlp_fn("acn_mlp_workspace_bytes")()), dtype=torch.uint8, device=device)


def _fm_zeros(M: int, cols: int, device) -> torch.Tensor:
    """(groups, cols, 2048) feature-major buffer; only the last group's tail needs zeros."""
    G = (M + MLP_GROUP - 1) // MLP_GROUP
    t = torch.empty(G, cols, MLP_GROUP, device=device, dtype=torch.float32)
    if M % MLP_GROUP:
        t[-1, :, M % MLP_GROUP:].zero_()
    return t


def mlp_train_fwd(h0: torch.Tensor, sh: torch.Tensor, ws: Sequence[torch.Tensor], save: bool = True,
                  precision: Optional[str] = None, return_img: bool = False):
    """(M,32) hash features + (M,16) SH -> out (M,4) and the feature-major saved layer inputs (or None);
    with ``return_img`` also the call's packed weight image (for mlp_train_bwd_dw(img=...))."""
    require_hip(h0, "MetaNGP MLP (training)")
    M = h0.shape[0]
    out = torch.empty(M, 4, device=h0.device, dtype=torch.float32)
    sv = _fm_zeros(M, MLP_SAVE_COLS, h0.device) if save else None
    w = _mlp_struct(ws)
    img = torch.empty(int(mlp_fn("acn_mlp_workspace_bytes", precision)()), dtype=torch.uint8, device=h0.device)
    check(mlp_fn("acn_mlp_train_fwd", precision)(ptr(h0), ptr(sh), M, C.byref(w), ptr(out),
                                                  ptr(sv) if save else None, ptr(img), stream_of(h0)),
          "acn_mlp_train_fwd")
    if return_img:
        return out, sv, (img if M > 0 else None)
    return out, sv


def mlp_train_bwd(save: torch.Tensor, out: torch.Tensor, gout: torch.Tensor, ws: Sequence[torch.Tensor],
                  want_h0: bool = True):
    M = out.shape[0]
    gs = _fm_zeros(M, MLP_GRAD_COLS, out.device)
    gh = torch.empty(M, 32, device=out.device, dtype=torch.float32) if want_h0 else None
    w = _mlp_struct(ws)
    check(mlp_fn("acn_mlp_train_bwd")(ptr(save), ptr(out), ptr(gout), M, C.byref(w), ptr(gs),
                                       ptr(gh) if want_h0 else None, ptr(_mlp_ws(out.device)), stream_of(out)),
          "acn_mlp_train_bwd")
    return gs, gh


# [dW | db] layout of acn_mlp_train_bwd_dw (include/acnerf.h): the 14 gradients, acn_mlp order
MLP_DW_SHAPES = ((64, 32), (64,), (64, 64), (64,), (1, 64), (1,), (15, 64), (15,), (64, 31), (64,), (64, 64), (64,),
                 (3, 64), (3,))
MLP_DW_FLOATS = 13715
# Precision of the training MLP's layer products: "fp16x3" (default: the fp32-accurate 3-term fp16 split on
# v_mfma_f32_32x32x16_f16), "fp32" (exact fp32 MFMA, the acn_mlp_*_exact entry points) or "amp" (the
# reference's use_amp=True arithmetic: torch.autocast(float16) -- one fp16 product per term, fp16 layer outputs
# and gradients; the acn_mlp_*_amp entry points; pair it with a loss scale, see optim.AmpScaler).  Env ACN_TRAIN_MLP.
TRAIN_MLP_PRECISION = os.environ.get("ACN_TRAIN_MLP", "fp16x3")
_MLP_SUFFIX = {"fp16x3": "", "fp32": "_exact", "amp": "_amp"}


def set_train_mlp_precision(mode: str) -> None:
    """Select the training MLP kernels ("fp16x3", "fp32" or "amp") for later calls; step objects
    (RoutedAdaptStep, ExpertParallelAdaptStep) keep the precision they were built with."""
    global TRAIN_MLP_PRECISION
    if mode not in _MLP_SUFFIX:
        raise ValueError(f"train MLP precision must be one of {sorted(_MLP_SUFFIX)}, got {mode!r}")
    TRAIN_MLP_PRECISION = mode


def mlp_fn(name: str, precision: Optional[str] = None):
    """The training-MLP entry point ``name`` of the selected precision."""
    return getattr(_lib.lib(), name + _MLP_SUFFIX[precision or TRAIN_MLP_PRECISION])
# Optional timing hook (bench.py --workload meta): when set to a list, every acn_mlp_train_bwd_dw call appends
# (start event, end event, M, want_h0) recorded on the current stream around the call (weight pack +
# mlp_bwd_dw_pc_kernel + mlp_dw_reduce_kernel)
DW_HOOK = None
# Algorithmic MACs per sample of the fused MLP backward (SURVEY §8(d) MLP shapes): dW = every weight
# (32x64 + 64x64 + 64x[15|1] + 31x64 + 64x64 + 64x3 = 13,440); dX = the layer-input gradients the chain
# needs (64x3 + 64x64 + 64x15 geo columns + 64x16 heads + 64x64 = 10,368, + 32x64 when dL/dh0 is wanted).
# The in-register forward recompute (13,440 MACs) is extra work of this design, not counted.
MLP_BWD_MACS_DW, MLP_BWD_MACS_DX, MLP_BWD_MACS_DX0, MLP_FWD_MACS = 13440, 10368, 2048, 13440


def mlp_bwd_flops(M: int, want_h0: bool) -> int:
    """Algorithmic FLOPs (2 per MAC) of one fused MLP backward over M samples: dW + dX, no recompute."""
    return 2 * M * (MLP_BWD_MACS_DW + MLP_BWD_MACS_DX + (MLP_BWD_MACS_DX0 if want_h0 else 0))


def mlp_train_bwd_dw(h0: torch.Tensor, sh: torch.Tensor, out: torch.Tensor, gout: torch.Tensor,
                     ws: Sequence[torch.Tensor], want_h0: bool = True, img: Optional[torch.Tensor] = None,
                     precision: Optional[str] = None):
    """Fused backward: the 14 weight / bias gradients (views of one flat buffer, nn.Linear shapes) and
    dL/dh0 (M, 32) or None, from h0 / sh (the forward is re-run in registers) and dL/dout.  ``img``: the
    packed image mlp_train_fwd(return_img=True) returned for the same weights and precision (the
    backward then skips its own pack)."""
    require_hip(h0, "MetaNGP MLP (training)")
    M = out.shape[0]
    dw = torch.empty(MLP_DW_FLOATS, device=out.device, dtype=torch.float32)
    gh = torch.empty(M, 32, device=out.device, dtype=torch.float32) if want_h0 else None
    wsp = torch.empty(int(mlp_fn("acn_mlp_dw_workspace_bytes", precision)()), dtype=torch.uint8, device=out.device)
    hook = DW_HOOK
    if hook is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    if img is not None:
        check(mlp_fn("acn_mlp_train_bwd_dw_img", precision)(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, ptr(img),
                                                             ptr(dw), ptr(gh) if want_h0 else None, ptr(wsp),
                                                             stream_of(out)), "acn_mlp_train_bwd_dw_img")
    else:
        w = _mlp_struct(ws)
        check(mlp_fn("acn_mlp_train_bwd_dw", precision)(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, C.byref(w),
                                                         ptr(dw), ptr(gh) if want_h0 else None, ptr(wsp),
                                                         stream_of(out)), "acn_mlp_train_bwd_dw")
    if hook is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        hook.append((e0, e1, int(M), bool(want_h0)))
    grads, o = [], 0
    for shp in MLP_DW_SHAPES:
        n = 1
        for d in shp:
            n *= d
        grads.append(dw[o:o + n].view(shp))
        o += n
    return grads, gh


def mlp_train_bwd_input(h0: torch.Tensor, sh: torch.Tensor, out: torch.Tensor, gout: torch.Tensor,
                        ws: Sequence[torch.Tensor], want_h0: bool = True, want_sh: bool = True,
                        img: Optional[torch.Tensor] = None, precision: Optional[str] = None):
    """Input gradients of the expert MLP with frozen weights (acn_mlp_train_bwd_input): (dL/dh0 (M,32) or None,
    dL/dsh (M,16) or None) from h0 / sh (the forward is re-run in registers) and dL/dout.  One launch, no weight
    gradients; gh0 is bit-identical to mlp_train_bwd_dw's, every row depends on its own sample only.  ``img``: the
    packed image mlp_train_fwd(return_img=True) returned for the same weights and precision.  "amp" is not
    exposed (differentiated inputs keep the composed chain under AMP)."""
    require_hip(h0, "MetaNGP MLP (input gradients)")
    precision = precision or TRAIN_MLP_PRECISION
    if precision == "amp":
        raise AcnError("mlp_train_bwd_input: precision 'amp' is not supported (fp16x3 or fp32)")
    M = out.shape[0]
    if h0.shape != (M, 32) or sh.shape != (M, 16) or gout.shape != (M, 4):
        raise AcnError(f"mlp_train_bwd_input: h0 (M,32), sh (M,16), out / gout (M,4) expected, got "
                       f"{tuple(h0.shape)}, {tuple(sh.shape)}, {tuple(out.shape)}, {tuple(gout.shape)}")
    for name, t in (("h0", h0), ("sh", sh), ("out", out), ("gout", gout)):
        if not (t.is_contiguous() and t.dtype == torch.float32):
            raise AcnError(f"mlp_train_bwd_input: {name} must be a contiguous fp32 tensor")
    gh = torch.empty(M, 32, device=out.device, dtype=torch.float32) if want_h0 else None
    gs = torch.empty(M, 16, device=out.device, dtype=torch.float32) if want_sh else None
    if img is not None:
        check(mlp_fn("acn_mlp_train_bwd_input_img", precision)(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, ptr(img),
                                                                ptr(gh), ptr(gs), stream_of(out)),
              "acn_mlp_train_bwd_input_img")
    else:
        w = _mlp_struct(ws)
        wsp = torch.empty(int(mlp_fn("acn_mlp_workspace_bytes", precision)()), dtype=torch.uint8, device=out.device)
        check(mlp_fn("acn_mlp_train_bwd_input", precision)(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, C.byref(w),
                                                            ptr(gh), ptr(gs), ptr(wsp), stream_of(out)),
              "acn_mlp_train_bwd_input")
    return gh, gs


def field_sigma_grad(x: torch.Tensor, spec: ExpertSpec, *, gate: Optional[torch.Tensor] = None, gate_min: float = 0.0,
                     precision: Optional[str] = None, eps: float = 1e-6):
    """(sigma (M,), d sigma / d x (M, 3)) of one expert at the world points ``x`` (M, D >= 3; columns 0:3 are read)
    in one launch (acn_field_sigma_grad): hash gather, sigma trunk and head forward and backward on the MFMA and
    the contraction with the corner rows, nothing else written.  Evaluation only (no autograd).  ``gate`` (M,):
    samples with gate <= gate_min return zeros, a tile of 32 such samples is skipped, the others' bits do not
    depend on the gate.  ``precision`` follows TRAIN_MLP_PRECISION ("amp" uses the fp16x3 kernel); ``eps`` is
    MetaNGP.enc_eps.  fp32 table, L = 16, F = 2, Linear / Smoothstep; anything else raises."""
    require_hip(x, "field_sigma_grad")
    if x.dim() != 2 or x.shape[1] < 3:
        raise AcnError(f"field_sigma_grad: x must be (M, D >= 3), got {tuple(x.shape)}")
    s = spec.s
    if s.table_fmt != _lib.ACN_TABLE_F32:
        raise AcnError("field_sigma_grad: fp32 tables only (the spec holds an fp16 render table)")
    precision = precision or TRAIN_MLP_PRECISION
    if precision not in _MLP_SUFFIX:
        raise ValueError(f"train MLP precision must be one of {sorted(_MLP_SUFFIX)}, got {precision!r}")
    if precision == "amp":
        precision = "fp16x3"
    xx = _f32(x)
    M = xx.shape[0]
    g = None
    if gate is not None:
        g = _f32(gate).reshape(-1)
        if g.shape[0] != M or g.device != xx.device:
            raise AcnError(f"field_sigma_grad: gate must hold {M} values on the points' device, got {tuple(gate.shape)}")
    sigma = torch.empty(M, device=xx.device, dtype=torch.float32)
    grad = torch.empty(M, 3, device=xx.device, dtype=torch.float32)
    w = _mlp_struct(spec.keep[1:15])
    wsp = torch.empty(int(mlp_fn("acn_mlp_workspace_bytes", precision)()), dtype=torch.uint8, device=xx.device)
    import numpy as np
    lo = np.float32(eps)
    hi = np.float32(1.0) - lo
    check(mlp_fn("acn_field_sigma_grad", precision)(
        ptr(xx), M, xx.shape[1], s.table, C.cast(s.res, C.c_void_p), s.L, s.log2T, s.F, s.interp,
        C.cast(s.aabb_min, C.c_void_p), C.cast(s.aabb_extent, C.c_void_p), C.c_float(lo), C.c_float(hi), C.byref(w),
        ptr(g), C.c_float(gate_min), ptr(sigma), ptr(grad), ptr(wsp), stream_of(xx)), "acn_field_sigma_grad")
    return sigma, grad


def normal_composite(grad: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """(N, 3) = sum_s weights[n, s] * (-grad[n, s] / max(|grad[n, s]|, 1e-9)) (acn_normal_composite): the weighted
    sum of the samples' unit normals, terms in fp32, accumulated in float64 in sample order.  ``grad`` is (N*S, 3)
    or (N, S, 3), ``weights`` (N, S).  A zero gradient adds exactly 0."""
    require_hip(weights, "normal_composite")
    wv = _f32(weights)
    if wv.dim() != 2 or wv.shape[1] < 1:
        raise AcnError(f"normal_composite: weights must be (N, S >= 1), got {tuple(weights.shape)}")
    N, S = wv.shape
    gv = _f32(grad).reshape(-1, 3)
    if gv.shape[0] != N * S or gv.device != wv.device:
        raise AcnError(f"normal_composite: grad must be ({N * S}, 3) on the weights' device, got {tuple(grad.shape)}")
    out = torch.empty(N, 3, device=wv.device, dtype=torch.float32)
    check(_lib.lib().acn_normal_composite(ptr(gv), ptr(wv), N, int(S), ptr(out), stream_of(wv)),
          "acn_normal_composite")
    return out


def _ray_scale_arg(ray_scale: Optional[torch.Tensor], N: int, device, what: str) -> Optional[torch.Tensor]:
    if ray_scale is None:
        return None
    rs = _f32(ray_scale).reshape(-1)
    if rs.numel() != N or rs.device != device:
        raise AcnError(f"{what}: ray_scale must be ({N},) on the weights' device, got {tuple(ray_scale.shape)} on "
                       f"{ray_scale.device}")
    return rs


def distortion_dense(weights: torch.Tensor, t_vals: torch.Tensor, ray_scale: Optional[torch.Tensor] = None,
                     want_grad: bool = True):
    """(loss (N,), d loss / d weights (N, S) or None) of the mip-NeRF 360 distortion loss over the compositing's own
    intervals (acn_distortion_dense): s_i = t_i, d_i = max(t_{i+1} - t_i, 1e-4) with the last d copied from its
    predecessor (volume_render's ``dists``), m_i = s_i + d_i / 2,
    loss = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i, times ``ray_scale`` (N,) when given.  One launch; prefix
    sums in float64, one fp32 rounding per output; bitwise reproducible.  A ray whose scale is exactly 0 gets zeros and
    its t values are not read."""
    if weights.dim() != 2 or weights.shape[1] < 2 or t_vals.shape != weights.shape:
        raise AcnError(f"distortion_dense: weights and t_vals must both be (N, S >= 2), got {tuple(weights.shape)} and "
                       f"{tuple(t_vals.shape)}")
    require_hip(weights, "distortion_dense")
    wv, tv = _f32(weights), _f32(t_vals)
    if tv.device != wv.device:
        raise AcnError("distortion_dense: t_vals must be on the weights' device")
    N, S = wv.shape
    rs = _ray_scale_arg(ray_scale, N, wv.device, "distortion_dense")
    loss = torch.empty(N, device=wv.device, dtype=torch.float32)
    grad = torch.empty(N, S, device=wv.device, dtype=torch.float32) if want_grad else None
    check(_lib.lib().acn_distortion_dense(ptr(wv), ptr(tv), N, int(S), ptr(rs), ptr(loss), ptr(grad), stream_of(wv)),
          "acn_distortion_dense")
    return loss, grad


def _depth_target_args(depths, eps, depth_weight, sight_weight, N: int, device, what: str):
    """The (N,) fp32 targets and half-widths (``eps`` a float or an (N,) tensor) and the two weights as floats."""
    z = _f32(depths).reshape(-1)
    if z.numel() != N or z.device != device:
        raise AcnError(f"{what}: depths must be ({N},) on the weights' device, got {tuple(depths.shape)} on "
                       f"{depths.device}")
    if isinstance(eps, torch.Tensor):
        e = _f32(eps).reshape(-1)
        if e.numel() == 1 and N != 1:
            e = e.expand(N).contiguous()
        if e.numel() != N or e.device != device:
            raise AcnError(f"{what}: eps must be a float or ({N},) on the weights' device, got {tuple(eps.shape)} on "
                           f"{eps.device}")
    else:
        e = torch.full((N,), float(eps), device=device, dtype=torch.float32)
    ld, ls = float(depth_weight), float(sight_weight)
    if not (ld >= 0.0 and ls >= 0.0):
        raise AcnError(f"{what}: depth_weight and sight_weight must be >= 0, got {depth_weight} and {sight_weight}")
    return z, e, ld, ls


def depth_loss_dense(weights: torch.Tensor, t_vals: torch.Tensor, depths: torch.Tensor, eps,
                     ray_scale: Optional[torch.Tensor] = None, depth_weight: float = 1.0, sight_weight: float = 1.0,
                     want_grad: bool = True):
    """(loss (N,), d loss / d weights (N, S) or None) of the depth supervision over the compositing's own intervals
    (acn_depth_loss_dense): s_i = tau_i = t_i, e_i = t_i + d_i with volume_render's ``dists``; with the
    target z = ``depths[r]``, the half-width ``eps`` (a float or (N,)), sigma = eps / 3 and c = ``ray_scale[r]`` (1),
    k_i the mass of the Gaussian N(z, sigma) cut at z +- eps inside [s_i, e_i],
    loss = depth_weight (c (sum_i w_i t_i - z))^2 + sight_weight sum_{s_i < z + eps} (w_i - k_i)^2.  One launch; float64
    arithmetic, one fp32 rounding per output; bitwise reproducible.  A ray whose target or eps is not finite or <= 0,
    or whose scale is exactly 0, gets zeros and its t values are not read."""
    if weights.dim() != 2 or weights.shape[1] < 2 or t_vals.shape != weights.shape:
        raise AcnError(f"depth_loss_dense: weights and t_vals must both be (N, S >= 2), got {tuple(weights.shape)} and "
                       f"{tuple(t_vals.shape)}")
    require_hip(weights, "depth_loss_dense")
    wv, tv = _f32(weights), _f32(t_vals)
    if tv.device != wv.device:
        raise AcnError("depth_loss_dense: t_vals must be on the weights' device")
    N, S = wv.shape
    z, e, ld, ls = _depth_target_args(depths, eps, depth_weight, sight_weight, N, wv.device, "depth_loss_dense")
    rs = _ray_scale_arg(ray_scale, N, wv.device, "depth_loss_dense")
    loss = torch.empty(N, device=wv.device, dtype=torch.float32)
    grad = torch.empty(N, S, device=wv.device, dtype=torch.float32) if want_grad else None
    check(_lib.lib().acn_depth_loss_dense(ptr(wv), ptr(tv), N, int(S), ptr(z), ptr(e), ptr(rs), ld, ls, ptr(loss),
                                          ptr(grad), stream_of(wv)), "acn_depth_loss_dense")
    return loss, grad


SSIM_TILE_H = SSIM_TILE_W = 32  # ACN_SSIM_TILE: map pixels (forward) / image pixels (gradient) per workgroup
SSIM_MAX_WIN = 11                # the fused path takes odd window sizes 3 .. 11
_SSIM_WS = {}


def _ssim_ws(device, nbytes: int) -> torch.Tensor:
    """Workspace of acn_ssim_fwd per (device, stream), grown on demand; it carries no state between calls.  Under
    stream capture every captured call gets one of its own, as in _mse_ws."""
    if torch.cuda.is_current_stream_capturing():
        return _lib.capture_keepalive(torch.empty(nbytes, dtype=torch.uint8, device=device))
    key = (device, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _SSIM_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _SSIM_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def ssim_fwd(x: torch.Tensor, y: torch.Tensor, *, channels_last: bool = False, win_size: int = 11,
             win_sigma: float = 1.5, c1: float, c2: float, want_grad: bool = False):
    """(ssim (N, C) fp32, d ssim[n, c] / d x in x's layout or None) of pytorch_msssim.ssim's definition
    (acn_ssim_fwd): Gaussian window of ``win_size`` taps (odd, 3 .. 11) and ``win_sigma``, "valid"
    filtering, stabilisers ``c1`` and ``c2``.  ``x`` and ``y`` are (N, C, H, W), or (N, H, W, C) with
    ``channels_last`` (a rendered frame, read with no permute copy).  float64 arithmetic on the fp32 inputs, one fp32
    rounding per output, bitwise reproducible; ssim(x, x) is exactly 1.  The gradient in ``y`` is
    ``ssim_fwd(y, x, want_grad=True)``."""
    if x.dim() != 4 or y.shape != x.shape:
        raise AcnError(f"ssim_fwd: x and y must share one 4-D shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    N, C, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if channels_last else x.shape
    win = int(win_size)
    if win % 2 != 1 or not 3 <= win <= SSIM_MAX_WIN:
        raise AcnError(f"ssim_fwd: win_size must be odd and in 3..{SSIM_MAX_WIN}, got {win_size}")
    if not float(win_sigma) > 0:
        raise AcnError(f"ssim_fwd: win_sigma must be > 0, got {win_sigma}")
    if C < 1 or H < win or W < win:
        raise AcnError(f"ssim_fwd: needs C >= 1 and H, W >= win_size = {win}, got C = {C}, H = {H}, W = {W}")
    require_hip(x, "ssim_fwd")
    xv, yv = _f32(x), _f32(y)
    if yv.device != xv.device:
        raise AcnError("ssim_fwd: y must be on x's device")
    out = torch.empty(N, C, device=xv.device, dtype=torch.float32)
    grad = torch.empty_like(xv) if want_grad else None
    if N == 0:
        return out, grad
    L = _lib.lib()
    ws = _ssim_ws(xv.device, int(L.acn_ssim_workspace_bytes(N, C, H, W, int(want_grad))))
    check(L.acn_ssim_fwd(ptr(xv), ptr(yv), N, C, H, W, int(bool(channels_last)), win, float(win_sigma), float(c1),
                         float(c2), ptr(out), ptr(grad), ptr(ws), ws.numel(), stream_of(xv)), "acn_ssim_fwd")
    return out, grad


RESAMPLE_MAX_S, RESAMPLE_MAX_F = 1024, 1024  # acn_resample_pdf's row limits (its LDS: 16 KB per ray)


def resample_pdf(weights: torch.Tensor, t_vals: torch.Tensor, n_fine: int, jitter: Optional[torch.Tensor] = None,
                 rays: Optional[torch.Tensor] = None, want_points: bool = False):
    """(t_fine (N, F), t_merged (N, S + F), pts6 (N * (S + F), 6) or None) of classic NeRF's importance resampling
    (acn_resample_pdf): F = ``n_fine`` depths per ray by the inverse CDF of the inner weights + 1e-5 over the bins
    between the midpoints of ``t_vals``, at the stratified quantiles (j + jitter[n, j]) / F (0.5 without jitter), the
    row merged with ``t_vals`` (a coarse sample before an equal fine one) and, with ``want_points``, the rows
    [o + d t, d] of ``rays`` (N, 8).  One launch; float64 arithmetic, one fp32 rounding per depth; bitwise reproducible.
    3 <= S <= 1024, 1 <= F <= 1024."""
    if weights.dim() != 2 or weights.shape[1] < 3 or t_vals.shape != weights.shape:
        raise AcnError(f"resample_pdf: weights and t_vals must both be (N, S >= 3), got {tuple(weights.shape)} and "
                       f"{tuple(t_vals.shape)}")
    F = int(n_fine)
    if F < 1:
        raise AcnError(f"resample_pdf: n_fine must be >= 1, got {n_fine}")
    require_hip(weights, "resample_pdf")
    wv, tv = _f32(weights), _f32(t_vals)
    if tv.device != wv.device:
        raise AcnError("resample_pdf: t_vals must be on the weights' device")
    N, S = wv.shape
    jit = None
    if jitter is not None:
        jit = _f32(jitter)
        if jit.shape != (N, F) or jit.device != wv.device:
            raise AcnError(f"resample_pdf: jitter must be ({N}, {F}) on the weights' device, got {tuple(jitter.shape)} "
                           f"on {jitter.device}")
    rv = None
    if want_points:
        if rays is None:
            raise AcnError("resample_pdf: want_points needs the rays")
        rv = _f32(rays)
        if rv.dim() != 2 or rv.shape != (N, 8) or rv.device != wv.device:
            raise AcnError(f"resample_pdf: rays must be ({N}, 8) on the weights' device, got {tuple(rays.shape)} on "
                           f"{rays.device}")
    t_fine = torch.empty(N, F, device=wv.device, dtype=torch.float32)
    t_merged = torch.empty(N, S + F, device=wv.device, dtype=torch.float32)
    pts6 = torch.empty(N * (S + F), 6, device=wv.device, dtype=torch.float32) if want_points else None
    check(_lib.lib().acn_resample_pdf(ptr(wv), ptr(tv), N, int(S), ptr(jit), F, ptr(rv), ptr(t_fine), ptr(t_merged),
                                      ptr(pts6), stream_of(wv)), "acn_resample_pdf")
    return t_fine, t_merged, pts6


INTERLEVEL_MAX_S, INTERLEVEL_MAX_P = 1024, 1024  # acn_interlevel_loss's row limits (its LDS: 12 (S + P + 2) B per ray)


def interlevel_loss(t_fine: torch.Tensor, w_fine: torch.Tensor, t_prop: torch.Tensor, w_prop: torch.Tensor,
                    ray_scale: Optional[torch.Tensor] = None, eps: float = 2.0 ** -23, want_grad: bool = True):
    """(loss (N,), d loss / d w_prop (N, P) or None) of the mip-NeRF 360 interlevel ("proposal") loss
    (acn_interlevel_loss): with the edges of a row of depths E(t) = [t_0 .. t_{S-1},
    t_{S-1} + (t_{S-1} - t_{S-2})], a = E(t_fine) and p = E(t_prop),
    bound_i = the sum of w_prop over the proposal intervals k with p_{k+1} > a_i and p_k < a_{i+1},
    loss = sum_i max(0, w_fine_i - bound_i)^2 / (w_fine_i + eps), times ``ray_scale`` (N,) when given.  The fine
    weights and all depths are constants.  One launch; float64 arithmetic, one fp32 rounding per output; bitwise
    reproducible.  A ray whose scale is exactly 0 gets zeros and its depths are not read.  2 <= S, P <= 1024."""
    if (t_fine.dim() != 2 or w_fine.shape != t_fine.shape or t_prop.dim() != 2 or w_prop.shape != t_prop.shape
            or t_prop.shape[0] != t_fine.shape[0]):
        raise AcnError(f"interlevel_loss: t_fine and w_fine must both be (N, S), t_prop and w_prop both (N, P), got "
                       f"{tuple(t_fine.shape)}, {tuple(w_fine.shape)}, {tuple(t_prop.shape)} and "
                       f"{tuple(w_prop.shape)}")
    N, S = t_fine.shape
    P = t_prop.shape[1]
    if not (2 <= S <= INTERLEVEL_MAX_S and 2 <= P <= INTERLEVEL_MAX_P):
        raise AcnError(f"interlevel_loss: needs 2 <= S <= {INTERLEVEL_MAX_S} fine and 2 <= P <= {INTERLEVEL_MAX_P} "
                       f"proposal samples, got {S} and {P}")
    if not float(eps) > 0:
        raise AcnError(f"interlevel_loss: eps must be > 0, got {eps}")
    require_hip(w_prop, "interlevel_loss")
    wp, tp, tf, wf = _f32(w_prop), _f32(t_prop), _f32(t_fine), _f32(w_fine)
    if not (tp.device == tf.device == wf.device == wp.device):
        raise AcnError("interlevel_loss: the four arrays must be on one device")
    rs = _ray_scale_arg(ray_scale, N, wp.device, "interlevel_loss")
    loss = torch.empty(N, device=wp.device, dtype=torch.float32)
    grad = torch.empty(N, P, device=wp.device, dtype=torch.float32) if want_grad else None
    check(_lib.lib().acn_interlevel_loss(ptr(tf), ptr(wf), int(S), ptr(tp), ptr(wp), int(P), N, ptr(rs), float(eps),
                                         ptr(loss), ptr(grad), stream_of(wp)), "acn_interlevel_loss")
    return loss, grad


def sample_stratified(rays: torch.Tensor, S: int, jitter: Optional[torch.Tensor], aabb_min, aabb_extent,
                      eps: float):
    """Training-path sampler (acn_sample_stratified): t_vals (N,S), x01 (N*S,3) in the expert's unit box
    clamped to [eps, 1 - eps] with eps the fp32 enc_eps buffer (1 - eps evaluated in fp32, as
    MetaNGP._world_to_unit's tensor arithmetic does), SH (N*S,16)."""
    require_hip(rays, "render_rays_stratified sampler")
    rays = rays.contiguous()
    N = rays.shape[0]
    dev = rays.device
    t = torch.empty(N, S, device=dev, dtype=torch.float32)
    x01 = torch.empty(N * S, 3, device=dev, dtype=torch.float32)
    sh = torch.empty(N * S, 16, device=dev, dtype=torch.float32)
    jit = None
    if jitter is not None:
        jitter = jitter.to(dev, torch.float32).contiguous()
        jit = ptr(jitter)
    mn = (C.c_float * 3)(*aabb_min)
    ex = (C.c_float * 3)(*aabb_extent)
    import numpy as np
    lo = np.float32(eps)
    hi = np.float32(1.0) - lo
    check(_lib.lib().acn_sample_stratified(ptr(rays), N, int(S), jit, C.cast(mn, C.c_void_p), C.cast(ex, C.c_void_p),
                                           C.c_float(lo), C.c_float(hi),
                                           ptr(t), ptr(x01), ptr(sh), stream_of(rays)), "acn_sample_stratified")
    return t, x01, sh


# ------------------------------------------------------------------------------------------
# routed container, differentiable path (routed.hip)
def routed_pairs(rays: torch.Tensor, S: int, jitter: Optional[torch.Tensor], routing: acn_routing, aabb_mins,
                 aabb_exts, eps: float):
    """t_vals (N,S) and the (sample, expert) pairs of the routed container: returns (t_vals, starts (K+1
    host ints), pidx (P,) int32, pw (P,), x01 (P,3), sh (P,16), pmap (M,K) int32).  One host
    synchronisation (the segment sizes) sits between the count and the scatter launches."""
    require_hip(rays, "render_rays (routed container)")
    r = _f32(rays)
    N = r.shape[0]
    M = N * int(S)
    K = int(routing.K)
    dev = r.device
    L = _lib.lib()
    ws = torch.empty(int(L.acn_routed_workspace_bytes(M, K)), dtype=torch.uint8, device=dev)
    t = torch.empty(N, int(S), device=dev, dtype=torch.float32)
    starts = torch.empty(2 * K + 1, device=dev, dtype=torch.int64)
    jit = None if jitter is None else _f32(jitter.to(dev))
    check(L.acn_routed_count(ptr(r), N, int(S), ptr(jit), C.byref(routing), 1, ptr(t), ptr(starts), ptr(ws),
                             ws.numel(), stream_of(r)), "acn_routed_count")
    st = [int(v) for v in starts[: K + 1].cpu().tolist()]
    P = st[K]
    pidx = torch.empty(P, device=dev, dtype=torch.int32)
    pw = torch.empty(P, device=dev, dtype=torch.float32)
    x01 = torch.empty(P, 3, device=dev, dtype=torch.float32)
    sh = torch.empty(P, 16, device=dev, dtype=torch.float32)
    pmap = torch.empty(M, K, device=dev, dtype=torch.int32)
    mins = (C.c_float * (3 * K))(*[float(v) for row in aabb_mins for v in row])
    exts = (C.c_float * (3 * K))(*[float(v) for row in aabb_exts for v in row])
    import numpy as np
    lo = np.float32(eps)
    hi = np.float32(1.0) - lo
    check(L.acn_routed_scatter(ptr(r), N, int(S), K, ptr(t), ptr(starts), C.cast(mins, C.c_void_p),
                               C.cast(exts, C.c_void_p), C.c_float(lo), C.c_float(hi), 1, ptr(ws), ptr(pidx),
                               ptr(pw), ptr(x01), ptr(sh), ptr(pmap), None, stream_of(r)), "acn_routed_scatter")
    return t, st, pidx, pw, x01, sh, pmap


def routed_blend_fwd(y: torch.Tensor, pw: torch.Tensor, pmap: torch.Tensor) -> torch.Tensor:
    M, K = pmap.shape
    out = torch.empty(M, 4, device=pmap.device, dtype=torch.float32)
    yy = _f32(y).view(-1, 4) if y.numel() else None
    check(_lib.lib().acn_routed_blend_fwd(ptr(yy), ptr(pw), ptr(pmap), M, K, ptr(out), stream_of(pmap)),
          "acn_routed_blend_fwd")
    return out


def routed_blend_bwd(g: torch.Tensor, pidx: torch.Tensor, pw: torch.Tensor,
                     live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dY per pair slot; ``live``: a device int64 holding the live slot count (capacity-sized buffers),
    slots past it are left unwritten."""
    P = pidx.shape[0]
    gy = torch.empty(P, 4, device=pidx.device, dtype=torch.float32)
    check(_lib.lib().acn_routed_blend_bwd(ptr(_f32(g)), ptr(pidx), ptr(pw), P, ptr(live), ptr(gy), stream_of(pidx)),
          "acn_routed_blend_bwd")
    return gy


def routed_pairs_xd(rays: torch.Tensor, S: int, jitter: Optional[torch.Tensor], routing: acn_routing,
                    tile_rays: int = 0):
    """t_vals (N,S) and the routed pairs as expert-parallel records: (t_vals, counts (K host ints), pidx, pw,
    xd (P,6) world point + direction, pmap (M,K), pk (P,)); pairs grouped by expert, in sample order, or with
    ``tile_rays`` > 0 in depth tiles of that many rays (acn_routed_*_tiled, the ExpertParallelRenderer order)."""
    require_hip(rays, "expert-parallel render")
    r = _f32(rays)
    N = r.shape[0]
    M = N * int(S)
    K = int(routing.K)
    dev = r.device
    L = _lib.lib()
    ws = torch.empty(int(L.acn_routed_workspace_bytes(M, K)), dtype=torch.uint8, device=dev)
    t = torch.empty(N, int(S), device=dev, dtype=torch.float32)
    seg = torch.empty(2 * K + 1, device=dev, dtype=torch.int64)
    jit = None if jitter is None else _f32(jitter.to(dev))
    check(L.acn_routed_count(ptr(r), N, int(S), ptr(jit), C.byref(routing), 1, ptr(t), ptr(seg), ptr(ws),
                             ws.numel(), stream_of(r)), "acn_routed_count")
    sh = [int(v) for v in seg.cpu().tolist()]
    counts = sh[K + 1:]
    P = sh[K]
    pidx = torch.empty(P, device=dev, dtype=torch.int32)
    pw = torch.empty(P, device=dev, dtype=torch.float32)
    xd = torch.empty(P, 6, device=dev, dtype=torch.float32)
    pk = torch.empty(P, device=dev, dtype=torch.int32)
    pmap = torch.empty(M, K, device=dev, dtype=torch.int32)
    if tile_rays:   # the same segments (capacities = the counts), laid out in depth-tile order
        check(L.acn_routed_count_caps_tiled(ptr(r), N, int(S), ptr(jit), C.byref(routing), (C.c_int64 * K)(*counts),
                                            int(tile_rays), ptr(t), ptr(seg), ptr(ws), ws.numel(), stream_of(r)),
              "acn_routed_count_caps_tiled")
    check(L.acn_routed_scatter_xd_tiled(ptr(r), N, int(S), K, int(tile_rays), ptr(t), ptr(seg), ptr(ws), ptr(pidx),
                                        ptr(pw), ptr(xd), ptr(pmap), ptr(pk), stream_of(r)),
          "acn_routed_scatter_xd_tiled")
    return t, counts, pidx, pw, xd, pmap, pk


def xd_unit_sh(xd: torch.Tensor, aabb_min, aabb_extent, eps: float):
    """Owner side: (P,6) records -> x01 (P,3) in the expert's unit box and SH-4 (P,16) of the direction."""
    require_hip(xd, "expert-parallel expert")
    x = _f32(xd)
    P = x.shape[0]
    x01 = torch.empty(P, 3, device=x.device, dtype=torch.float32)
    sh = torch.empty(P, 16, device=x.device, dtype=torch.float32)
    mn = (C.c_float * 3)(*aabb_min)
    ex = (C.c_float * 3)(*aabb_extent)
    import numpy as np
    lo = np.float32(eps)
    hi = np.float32(1.0) - lo
    check(_lib.lib().acn_xd_unit_sh(ptr(x), P, C.cast(mn, C.c_void_p), C.cast(ex, C.c_void_p), C.c_float(lo),
                                    C.c_float(hi), ptr(x01), ptr(sh), stream_of(x)), "acn_xd_unit_sh")
    return x01, sh
