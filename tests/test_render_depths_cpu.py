"""Host-side checks of the render at caller-supplied depths, no GPU needed: render_rays_at on CPU
tensors is the composed chain (points, model forward, background, volume_render) exactly and differentiable in the
model's parameters, the shape errors, and the new entry point's place in the header and the binding."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


class _TinyField(torch.nn.Module):
    """A smooth stand-in for the field on the CPU: (M, 6) rows -> (M, 4) rgb in [0, 1] and sigma >= 0."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(6, 16)
        self.b = torch.nn.Linear(16, 4)

    def forward(self, x, params=None):
        y = self.b(torch.sin(self.a(x)))
        return torch.cat([torch.sigmoid(y[:, :3]), 8.0 * torch.nn.functional.softplus(y[:, 3:] - 1.0)], -1)


def _cpu_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n, 3, generator=g) - 0.5
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    near = 0.1 * torch.rand(n, 1, generator=g)
    return torch.cat([o, d, near, near + 1.0 + torch.rand(n, 1, generator=g)], 1)


def _depths(n, s, seed):
    """Non-decreasing rows that no linspace gives: sorted uniforms, a run of equal neighbours in every row."""
    t = (0.1 + 1.5 * torch.rand(n, s, generator=torch.Generator().manual_seed(seed))).sort(1).values
    t[:, 3] = t[:, 2]
    return t


def test_render_rays_at_is_the_composed_chain_on_cpu():
    from adaptive_city_nerf_amd import render_rays_at
    from adaptive_city_nerf_amd.ray_rendering import volume_render
    m = _TinyField()
    N, S = 24, 13
    rays, t = _cpu_rays(N, 5), _depths(N, S, 6)
    out = render_rays_at(m, rays, t, bg_color_default="white")
    assert len(out) == 4
    rgb, depth, w, acc = out
    assert rgb.shape == (N, 3) and depth.shape == (N,) and w.shape == (N, S) and acc.shape == (N,)
    id6 = torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * t[..., None],
                     rays[:, None, 3:6].expand(N, S, 3)], -1).reshape(-1, 6)
    ref = volume_render(m(id6).view(N, S, 4), t, bg_rgb=torch.ones(N, 3))
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    assert float(acc.detach().max()) > 0
    # the model evaluated in pieces: the same rows (the CPU matmul's blocking depends on the piece: a few ulps)
    assert all(float((a - b).detach().abs().max()) <= 1e-6
               for a, b in zip(render_rays_at(m, rays, t, chunk=50), out))
    # differentiable in the model's parameters; the depths are constants
    tg = t.clone().requires_grad_(True)
    rgb2 = render_rays_at(m, rays, tg)[0]
    assert torch.equal(rgb2, rgb)
    (rgb2 ** 2).mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
               for p in m.parameters())
    assert tg.grad is None
    # and in the rays' origins and directions
    rg = rays.clone().requires_grad_(True)
    render_rays_at(m, rg, t)[0].sum().backward()
    assert bool(torch.isfinite(rg.grad).all()) and float(rg.grad[:, :6].abs().max()) > 0
    assert float(rg.grad[:, 6:].abs().max()) == 0.0          # near / far are not used


def test_shape_errors_raise_without_a_gpu():
    from adaptive_city_nerf_amd import ops, render_rays_at
    from adaptive_city_nerf_amd._lib import AcnError
    m = _TinyField()
    rays = _cpu_rays(4, 1)
    for bad in (torch.rand(4, 1), torch.rand(5, 8), torch.rand(4), torch.rand(4, 2, 2)):
        with pytest.raises(AcnError, match="t_vals"):
            render_rays_at(m, rays, bad)
        with pytest.raises(AcnError, match="t_vals"):
            ops.render_depths(rays, bad, [], None, None, None)
    with pytest.raises(AcnError, match="HIP device"):        # the raw op has no CPU form
        ops.render_depths(rays, torch.rand(4, 8), [], None, None, None)


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    import adaptive_city_nerf_amd as A
    from adaptive_city_nerf_amd import _lib
    text = (REPO / "include" / "acnerf.h").read_text()
    assert "acn_render_depths_fwd" in re.findall(r"^(?:int|size_t)\s+(acn_\w+)\s*\(", text, re.M)
    assert "acn_render_depths_fwd" in _lib.exported_symbols()
    L = _lib.lib()
    assert hasattr(L, "acn_render_depths_fwd")

    def last_error():
        buf = ctypes.create_string_buffer(512)
        L.acn_last_error(buf, 512)
        return buf.value.decode()

    def call(N, S):
        return L.acn_render_depths_fwd(None, N, S, None, None, None, -1, None, 1.0, 0.0, None, 0, None, None, None,
                                       None, None, 0, None)

    assert call(4, 1) == -1 and "S >= 2" in last_error()
    assert call(-1, 8) == -1
    assert call(4, 8) == -1 and "NULL" in last_error()
    assert call(0, 8) == 0                                   # nothing launched
    assert A.render_rays_at is A.ray_rendering.render_rays_at and callable(A.ops.render_depths)
    assert list(inspect.signature(A.render_rays_at).parameters) == [
        "model", "rays", "t_vals", "params", "active_module", "bg_color_default", "chunk", "sigma_scale",
        "early_stop_tau"]
    assert list(inspect.signature(A.ops.render_depths).parameters) == [
        "rays", "t_vals", "experts", "routing", "active_module", "background", "sigma_scale", "tau", "want_weights",
        "packed", "reorder"]
    assert isinstance(A.ray_rendering.FUSED_FINE_RENDER, bool)
