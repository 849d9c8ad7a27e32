"""Host-side checks of the importance resampling, no GPU needed: the package's torch form
(_sample_pdf_torch: CPU tensors, other dtypes, rows beyond the kernel's limits) against the sequential float64 loop of
tests/sample_pdf_ref.py, the argument errors, and the way up on a small CPU model: render_rays_hierarchical equals the
hand-composed chain, render_rays(n_importance=0) is render_rays_stratified.

Bound (sample_pdf_ref.BOUND): |t_fine - ref| <= 2 * 2^-24 * max|t_row| -- the result's own fp32 rounding plus the one
a different float64 summation order of the CDF can flip."""
import inspect

import numpy as np
import pytest
import torch

import sample_pdf_ref as R

SHAPES = [(37, 3, 1), (37, 4, 7), (16, 5, 64), (16, 64, 64), (8, 65, 128), (8, 96, 33), (4, 256, 128), (2, 1024, 1024),
          (2, 1025, 16)]


def _ratio(got, ref, t, keep):
    """Worst |got - ref| over BOUND * max|t_row| among the rows of ``keep``."""
    tmax = t[keep].abs().amax(1, keepdim=True).double()
    return float(((got[keep].double() - ref[keep].double()).abs() / (R.BOUND * tmax)).max())


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_form_matches_the_definition(shape):
    from adaptive_city_nerf_amd.ray_rendering import _sample_pdf_torch, sample_pdf
    N, S, F = shape
    for offset in R.OFFSETS:
        c = R.case(N, S, F, offset)
        keep = R.finite_rows(c)
        for jit in (None, c["jitter"]):
            ref = torch.from_numpy(R.resample(c["w"].numpy(), c["t"].numpy(), F, None if jit is None else jit.numpy()))
            t_fine, t_merged = _sample_pdf_torch(c["t"], c["w"], F, jit)
            assert t_fine.shape == (N, F) and t_fine.dtype == torch.float32 and t_merged.shape == (N, S + F)
            r = _ratio(t_fine, ref, c["t"], keep)
            print(f"{shape}, t offset {offset}, jitter {'given' if jit is not None else 'none'}: {r:.3f} of the bound")
            assert r <= 1
            b = torch.from_numpy(R.edges(c["t"].numpy())).float()      # rounding is monotonic: fl(b_0) <= fl(x) <= ..
            assert bool((t_fine[keep, 1:] >= t_fine[keep, :-1]).all())
            assert bool((t_fine[keep] >= b[keep, :1]).all()) and bool((t_fine[keep] <= b[keep, -1:]).all())
            want = torch.sort(torch.cat([c["t"], t_fine], 1), 1).values
            assert torch.equal(t_merged[keep], want[keep])
            # the public function takes the same path for CPU tensors
            pub = sample_pdf(c["t"], c["w"], F, jit, return_merged=True)
            assert torch.equal(pub[0][keep], t_fine[keep]) and torch.equal(pub[1][keep], t_merged[keep])
            assert torch.equal(sample_pdf(c["t"], c["w"], F, jit)[keep], t_fine[keep])


def test_special_rows_of_the_torch_form():
    from adaptive_city_nerf_amd.ray_rendering import _sample_pdf_torch
    N, S, F = 16, 64, 64
    c = R.case(N, S, F, 100.0)
    rows = c["rows"]
    assert set(rows) == set(R.KINDS)
    t_fine, t_merged = _sample_pdf_torch(c["t"], c["w"], F, c["jitter"])
    z = rows["zero"]
    uni = torch.from_numpy(R.uniform_row(c["t"][z].numpy(), F, c["jitter"][z].numpy()))
    assert float((t_fine[z].double() - uni).abs().max()) <= R.BOUND * float(c["t"][z].abs().max())
    o, m = rows["onehot"], R.onehot_index(S)
    b = torch.from_numpy(R.edges(c["t"].numpy())).float()
    inside = (t_fine[o] >= b[o, m - 1]) & (t_fine[o] <= b[o, m])
    assert int((~inside).sum()) <= R.onehot_outside_max(S, F)
    f = rows["flat"]
    assert bool((t_fine[f] == c["t"][f, 0]).all()) and bool((t_merged[f] == c["t"][f, 0]).all())


def test_other_dtypes_and_the_points():
    from adaptive_city_nerf_amd import sample_pdf
    c = R.case(8, 96, 33, 0.0)
    keep = R.finite_rows(c)
    ref = torch.from_numpy(R.resample(c["w"].numpy(), c["t"].numpy(), 33))
    t_fine, t_merged = sample_pdf(c["t"].double(), c["w"].double(), 33, return_merged=True)
    assert t_fine.dtype == torch.float64 and t_merged.dtype == torch.float64
    assert _ratio(t_fine, ref, c["t"], keep) <= 1
    w = c["w"].clone().requires_grad_(True)
    assert not sample_pdf(c["t"], w, 33).requires_grad                     # the weights are detached
    rays = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
    tf, tm, pts = sample_pdf(c["t"], c["w"], 33, rays=rays)
    assert pts.shape == (8 * (96 + 33), 6)
    want = torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * tm[..., None],
                      rays[:, None, 3:6].expand(8, 96 + 33, 3)], -1).reshape(-1, 6)
    k6 = keep.repeat_interleave(96 + 33)
    assert torch.equal(pts[k6], want[k6])


def test_shape_and_argument_errors():
    import ctypes
    from adaptive_city_nerf_amd import _lib as L
    from adaptive_city_nerf_amd import ops, render_rays, render_rays_hierarchical, sample_pdf, train
    w, t = torch.rand(4, 8), torch.rand(4, 8).sort(1).values
    for bad in (lambda: sample_pdf(t[:, :2], w[:, :2], 4), lambda: sample_pdf(t, w[:, :7], 4),
                lambda: sample_pdf(t[0], w[0], 4), lambda: sample_pdf(t, w, 0),
                lambda: sample_pdf(t, w, 4, jitter=torch.rand(4, 5)), lambda: sample_pdf(t, w, 4, rays=torch.zeros(3, 8)),
                lambda: sample_pdf(t, w, 4, rays=torch.zeros(4, 6)),
                lambda: ops.resample_pdf(w[:, :2], t[:, :2], 4), lambda: ops.resample_pdf(w, t[:, :7], 4),
                lambda: ops.resample_pdf(w[0], t[0], 4), lambda: ops.resample_pdf(w, t, 0),
                lambda: render_rays_hierarchical(None, torch.zeros(4, 8), 8, 0),
                lambda: render_rays_hierarchical(None, torch.zeros(4, 8), 2, 4)):
        with pytest.raises(L.AcnError):
            bad()
    with pytest.raises(L.AcnError, match="HIP device"):      # the raw op has no CPU form
        ops.resample_pdf(w, t, 4)
    lib = L.lib()

    def last_error():
        buf = ctypes.create_string_buffer(512)
        lib.acn_last_error(buf, 512)
        return buf.value.decode()

    none = (None,) * 5
    assert lib.acn_resample_pdf(None, None, -1, 8, None, 4, *none) == -1
    for S, F in ((2, 4), (1025, 4), (8, 0), (8, 1025)):     # outside the kernel's row limits: unsupported
        assert lib.acn_resample_pdf(None, None, 4, S, None, F, *none) == -2 and "1024" in last_error()
    assert lib.acn_resample_pdf(None, None, 4, 8, None, 4, *none) == -1 and "NULL" in last_error()
    assert lib.acn_resample_pdf(None, None, 0, 8, None, 4, *none) == 0            # nothing launched
    # the occupancy renderer marches: no resampling on top of it
    occ_model = type("M", (), {"use_occ": True, "occ_ready": True, "warned_occ_ready": True})()
    with pytest.raises(L.AcnError, match="occupancy"):
        render_rays(occ_model, torch.zeros(4, 8), ray_samples=8, n_importance=4)
    with pytest.raises(ValueError, match="n_importance"):
        train.adapt_step(None, None, None, None, None, group=object(), n_importance=8)
    with pytest.raises(ValueError, match="n_importance"):
        train.GraphedAdaptStep(None, None, None, None, None, active_module=0, n_importance=8)


def test_public_surface():
    import adaptive_city_nerf_amd as A
    assert A.sample_pdf is A.ray_rendering.sample_pdf
    assert A.render_rays_hierarchical is A.ray_rendering.render_rays_hierarchical
    assert list(inspect.signature(A.sample_pdf).parameters)[:5] == ["t_vals", "weights", "n_importance", "jitter",
                                                                    "return_merged"]
    assert list(inspect.signature(A.render_rays_hierarchical).parameters)[:10] == [
        "model", "rays", "ray_samples", "n_importance", "params", "active_module", "bg_color_default", "sigma_scale",
        "return_coarse", "return_t_vals"]
    assert callable(A.ops.resample_pdf) and "acn_resample_pdf" in A._lib.exported_symbols()


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


@pytest.mark.parametrize("training", [False, True])
def test_hierarchical_render_equals_the_hand_composed_chain(training):
    """On CPU tensors the compositing is the autograd form, so the coarse pass is kept differentiable
    (return_coarse); a t value that differs from the reference's by an fp32 rounding moves the smooth field's colour
    by far less than the 1e-5 allowed here."""
    from adaptive_city_nerf_amd import distortion_loss, render_rays, render_rays_hierarchical, render_rays_stratified
    from adaptive_city_nerf_amd.ray_rendering import volume_render
    m = _TinyField().train(training)
    N, S, F = 24, 12, 9
    rays = _cpu_rays(N, 5)
    g = torch.Generator().manual_seed(6)
    u, uf = torch.rand(N, S, generator=g), torch.rand(N, F, generator=g)
    out = render_rays_hierarchical(m, rays, S, F, bg_color_default="white", return_coarse=True, return_t_vals=True,
                                   jitter_u=u, jitter_fine=uf)
    assert len(out) == 6 and len(out[4]) == 4
    rgb, depth, w, acc, coarse, t_merged = out
    c = render_rays_stratified(m, rays, S, bg_color_default="white", return_t_vals=True, jitter_u=u)
    assert all(torch.equal(a, b) for a, b in zip(coarse, c[:4]))
    assert coarse[0].requires_grad and rgb.requires_grad and not t_merged.requires_grad
    t_fine = torch.from_numpy(R.resample(c[2].detach().numpy(), c[4].numpy(), F, uf.numpy() if training else None))
    tm = torch.sort(torch.cat([c[4], t_fine], 1), 1).values
    assert t_merged.shape == (N, S + F) and float((t_merged - tm).abs().max()) <= R.BOUND * float(tm.abs().max())
    id6 = torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * tm[..., None],
                     rays[:, None, 3:6].expand(N, S + F, 3)], -1).reshape(-1, 6)
    ref = volume_render(m(id6).view(N, S + F, 4), tm, bg_rgb=torch.ones(N, 3))
    for name, a, b in zip(("rgb", "depth", "weights", "acc"), (rgb, depth, w, acc), ref):
        a, b = a.detach(), b.detach()
        print(f"{name}: max|got - chain| = {float((a - b).abs().max()):.3e}")
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-5
    assert w.shape == (N, S + F)
    # the classic loss: fine + coarse colour, the regulariser on the fine pass
    loss = (rgb ** 2).mean() + (coarse[0] ** 2).mean() + 0.01 * distortion_loss(w, t_merged, rays=rays)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
               for p in m.parameters())
    # through the entry point, and n_importance = 0 is the stratified render itself
    via = render_rays(m, rays, S, n_importance=F, bg_color_default="white", return_coarse=True, jitter_u=u,
                      jitter_fine=uf)
    assert torch.equal(via[0], rgb) and torch.equal(via[2], w) and len(via) == 5
    plain = render_rays(m, rays, ray_samples=S, n_importance=0, jitter_u=u)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, c[:4]))
    assert all(torch.equal(a, b) for a, b in zip(render_rays(m, rays, ray_samples=S, jitter_u=u), c[:4]))


def test_hierarchical_render_differentiates_its_rays():
    from adaptive_city_nerf_amd import render_rays_hierarchical
    m = _TinyField().train(False)
    rays = _cpu_rays(6, 8).requires_grad_(True)
    rgb = render_rays_hierarchical(m, rays, 8, 5, return_coarse=True)[0]
    rgb.sum().backward()
    assert bool(torch.isfinite(rays.grad).all()) and float(rays.grad[:, :6].abs().max()) > 0
    assert float(rays.grad[:, 6:].abs().max()) == 0.0          # the t values are constants
