"""Host-side checks of the interlevel loss and the proposal-guided render, no GPU needed: the float64
torch form against the O(S P) definition of tests/interlevel_ref.py, its gradient, the exact zeros, the shape and limit
errors, proposal_weights / render_rays_proposal / render_rays(proposal=) on a tiny CPU field against the hand-composed
chain, compute_loss's gradient routing, and the new entry's place in the header, the binding and the Makefile."""
import ctypes
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import interlevel_ref as R

REPO = Path(__file__).resolve().parent.parent
SHAPES = [(37, 2, 2), (5, 64, 64), (3, 65, 63), (8, 33, 96), (4, 192, 64)]


def _f64(c):
    return c["t_fine"], c["w_fine"].double(), c["t_prop"], c["w_prop"].double()


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_form_matches_the_definition(shape):
    from adaptive_city_nerf_amd.ray_rendering import _interlevel_torch
    for offset in R.OFFSETS:
        c = R.case(*shape, offset)
        t, w, tp, wp = _f64(c)
        wp.requires_grad_(True)
        loss = _interlevel_torch(t, w, tp, wp)
        assert loss.dtype == torch.float64
        (g,) = torch.autograd.grad(loss.sum(), wp)
        loss = loss.detach()
        el = np.abs(loss.numpy() - c["loss"]) / np.maximum(np.abs(c["loss"]), 1e-300)
        gmax = np.maximum(np.abs(c["grad"]).max(1, keepdims=True), 1e-300)
        eg = np.abs(g.numpy() - c["grad"]) / gmax
        print(f"{shape}, t offset {offset}: loss {el.max():.2e}, gradient {eg.max():.2e} relative")
        assert float(el.max()) <= 1e-12 and float(eg.max()) <= 1e-12
        if c["rows"]:
            d, z = c["rows"]["dominated"], c["rows"]["zero_prop"]
            assert float(loss[d]) == 0.0 and not bool(g[d].any())
            # all-zero proposal weights: nothing bounds the fine weights
            wz = w[z]
            assert float(loss[z]) == pytest.approx(float((wz * wz / (wz + R.EPS)).sum()), rel=1e-14)


def test_gradcheck_and_double_backward():
    from adaptive_city_nerf_amd.ray_rendering import _interlevel_torch
    c = R.case(8, 33, 96, 0.0)
    t, w, tp, wp = _f64(c)
    # gradcheck's finite differences must not cross the kink of the max, w_i = bound_i (where both are 0 as well):
    # every proposal weight positive, and the test itself checks the distance to the kink
    wp = 0.3 * wp + 0.002
    s = np.stack([w[n].numpy() - (R.overlap(t[n].numpy(), tp[n].numpy()) * wp[n].numpy()[None]).sum(1)
                  for n in range(8)])
    s = s[(w.numpy() > 0) | (s < 0)]                 # w = bound = 0: a fine interval that overlaps nothing
    assert float(np.abs(s).min()) > 1e-5 and 0.2 < float((s > 0).mean()) < 0.8
    wp = wp.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: _interlevel_torch(t, w, tp, v), (wp,), eps=1e-7, atol=1e-6, rtol=1e-4)
    scale = torch.rand(8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.autograd.gradcheck(lambda v: _interlevel_torch(t, w, tp, v, ray_scale=scale), (wp,), eps=1e-7,
                                    atol=1e-6, rtol=1e-4)
    # differentiable twice in w_prop
    (g,) = torch.autograd.grad(_interlevel_torch(t, w, tp, wp).sum(), wp, create_graph=True)
    assert g.requires_grad
    (h,) = torch.autograd.grad((g * g).sum(), wp)
    assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0


def test_identical_histograms_give_exactly_zero():
    from adaptive_city_nerf_amd import interlevel_loss
    for shape in ((5, 64, 64), (3, 65, 63)):
        for offset in R.OFFSETS:
            c = R.case(*shape, offset)
            t, w = c["t_prop"], c["w_prop"]
            for wp in (w, w.double()):
                loss = interlevel_loss(t, w, t, wp.clone().requires_grad_(True), reduction="none")
                assert loss.dtype == wp.dtype and not bool(loss.any())
    # and a proposal that is the fine histogram split in two halves per interval bounds it too
    t = torch.tensor([[1.0, 2.0, 4.0, 5.0]])
    w = torch.tensor([[0.25, 0.5, 0.125, 0.0625]])
    tp = torch.tensor([[1.0, 1.5, 2.0, 3.0, 4.0, 4.5, 5.0, 5.5]])
    wp = torch.tensor([[0.125, 0.125, 0.25, 0.25, 0.0625, 0.0625, 0.03125, 0.03125]])
    assert float(interlevel_loss(t, w, tp, wp, reduction="sum")) == 0.0


def test_ties_are_the_tight_bound():
    """A fine interval that ends exactly on a proposal edge does not count the next proposal interval."""
    from adaptive_city_nerf_amd import interlevel_loss
    t = torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64)          # fine intervals [1,2] [2,3] [3,4]
    w = torch.tensor([[0.5, 0.25, 0.0]], dtype=torch.float64)
    tp = torch.tensor([[0.0, 2.0, 4.0]], dtype=torch.float64)         # proposal intervals [0,2] [2,4] [4,6]
    wp = torch.tensor([[0.125, 1.0, 1.0]], dtype=torch.float64, requires_grad=True)
    out = interlevel_loss(t, w, tp, wp, reduction="none")
    loss = out.detach()
    x0 = 0.5 - 0.125                                                  # [1,2] is bounded by [0,2] alone
    assert float(loss) == pytest.approx(x0 * x0 / (0.5 + R.EPS), rel=1e-15)
    out.sum().backward()
    assert wp.grad.tolist() == [[pytest.approx(-2.0 * x0 / (0.5 + R.EPS), rel=1e-15), 0.0, 0.0]]
    ref = R.definition(t.numpy(), w.numpy(), tp.numpy(), wp.detach().numpy())
    assert float(loss) == pytest.approx(float(ref[0][0]), rel=1e-15)


def test_invalid_rays_contribute_an_exact_zero():
    from adaptive_city_nerf_amd import interlevel_loss
    c = R.case(8, 33, 96, 100.0)
    t, w, tp, wp = (x.clone() for x in (c["t_fine"], c["w_fine"], c["t_prop"], c["w_prop"]))
    rays = torch.zeros(8, 8)
    rays[:, 7] = 1.0
    bad = [6, 7]
    rays[6, 6:] = float("nan")
    rays[7, 6], rays[7, 7] = 2.0, 2.0                                  # far == near
    t[bad], tp[bad] = float("nan"), float("nan")
    wp.requires_grad_(True)
    loss = interlevel_loss(t, w, tp, wp, rays=rays, reduction="none")
    assert bool((loss[bad] == 0).all()) and bool(torch.isfinite(loss).all())
    keep = [i for i in range(8) if i not in bad]
    assert np.allclose(loss[keep].detach().numpy(), c["loss"][keep], rtol=1e-6, atol=1e-12)
    mean = interlevel_loss(t, w, tp, wp, rays=rays)
    assert float(mean.detach()) == pytest.approx(float(loss.detach().sum()) / 8, rel=1e-6)
    mean.backward()
    assert bool((wp.grad[bad] == 0).all()) and bool(torch.isfinite(wp.grad).all())
    assert np.allclose(wp.grad[keep].numpy() * 8, c["grad"][keep], rtol=1e-5, atol=1e-9)


def test_shape_and_limit_errors_raise_without_a_gpu():
    from adaptive_city_nerf_amd import interlevel_loss, ops, proposal_weights, render_rays, render_rays_proposal
    from adaptive_city_nerf_amd._lib import AcnError
    a, b = torch.rand(4, 8), torch.rand(4, 6)
    for args in ((a, b, b, b), (a, a, b, a), (a, a, torch.rand(5, 6), torch.rand(5, 6)),
                 (torch.rand(4, 1), torch.rand(4, 1), b, b), (a, a, torch.rand(4, 1), torch.rand(4, 1)),
                 (torch.rand(4), torch.rand(4), b, b)):
        with pytest.raises(AcnError, match="interlevel_loss"):
            interlevel_loss(*args)
        with pytest.raises(AcnError, match="interlevel_loss"):
            ops.interlevel_loss(*args)
    with pytest.raises(AcnError, match="rays"):
        interlevel_loss(a, a, b, b, rays=torch.rand(3, 8))
    with pytest.raises(ValueError, match="reduction"):
        interlevel_loss(a, a, b, b, reduction="max")
    with pytest.raises(AcnError, match="eps"):
        interlevel_loss(a, a, b, b, eps=0.0)
    assert (ops.INTERLEVEL_MAX_S, ops.INTERLEVEL_MAX_P) == (1024, 1024)
    big = torch.rand(2, 1025).sort(1).values
    with pytest.raises(AcnError, match="1024"):                 # the limits come before the device check
        ops.interlevel_loss(big, big, b[:2], b[:2])
    with pytest.raises(AcnError, match="1024"):
        ops.interlevel_loss(a[:2], a[:2], big, big)
    with pytest.raises(AcnError, match="HIP device"):           # the raw op has no CPU form
        ops.interlevel_loss(a, a, b, b)
    assert interlevel_loss(big, big, b[:2], b[:2], reduction="none").shape == (2,)   # the torch form has no limit
    f, rays = _TinyField(), _cpu_rays(4, 1)
    with pytest.raises(AcnError, match="n_proposal"):
        proposal_weights(f, rays, 1)
    with pytest.raises(AcnError, match="n_proposal"):
        render_rays_proposal(f, f, rays, 2, 8)
    with pytest.raises(AcnError, match="n_fine"):
        render_rays_proposal(f, f, rays, 8, 1)
    with pytest.raises(AcnError, match="n_importance"):
        render_rays(f, rays, ray_samples=8, proposal=f)
    occ_model = type("M", (), {"use_occ": True, "occ_ready": True, "warned_occ_ready": True})()
    with pytest.raises(AcnError, match="occupancy"):
        render_rays(occ_model, rays, ray_samples=8, n_importance=4, proposal=f)
    with pytest.raises(TypeError, match="return_coarse"):
        render_rays(f, rays, ray_samples=8, n_importance=4, proposal=f, return_coarse=True)


# ------------------------------------------------------------------------------------------------ the renders
class _TinyField(torch.nn.Module):
    """A smooth stand-in for a field on the CPU: forward (M, 6) -> (M, 4) rgb in [0, 1] and sigma >= 0, and
    density (..., 3) -> (..., 1)."""

    def __init__(self, seed=3):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(6, 16)
        self.b = torch.nn.Linear(16, 4)
        self.c = torch.nn.Linear(3, 16)
        self.d = torch.nn.Linear(16, 1)

    def forward(self, x, params=None):
        y = self.b(torch.sin(self.a(x)))
        return torch.cat([torch.sigmoid(y[:, :3]), 8.0 * torch.nn.functional.softplus(y[:, 3:] - 1.0)], -1)

    def density(self, x, params=None):
        return 6.0 * torch.nn.functional.softplus(self.d(torch.sin(3.0 * self.c(x))) - 0.5)


def _cpu_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n, 3, generator=g) - 0.5
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    near = 0.1 * torch.rand(n, 1, generator=g)
    return torch.cat([o, d, near, near + 1.0 + torch.rand(n, 1, generator=g)], 1)


def _hand_weights(prop, rays, P, u=None, sigma_scale=1.0):
    """t_prop and w_prop from the formulas of the issue, with nothing of the package but stratified_t_vals."""
    from adaptive_city_nerf_amd import stratified_t_vals
    t = stratified_t_vals(rays[:, 6], rays[:, 7], P, randomized=u is not None, u=u)
    sig = prop.density(rays[:, None, :3] + rays[:, None, 3:6] * t[..., None]).squeeze(-1)
    e = torch.from_numpy(R.edges(t.numpy()))
    tau = sig.double() * sigma_scale * (e[:, 1:] - e[:, :-1])
    T = torch.exp(-(torch.cumsum(tau, 1) - tau))
    return t, (T * (1.0 - torch.exp(-tau))).float()


def test_proposal_render_is_the_hand_composed_chain_on_cpu():
    from adaptive_city_nerf_amd import (proposal_weights, render_rays, render_rays_at, render_rays_proposal,
                                        sample_pdf)
    N, P, F = 24, 12, 9
    m, prop = _TinyField(3).eval(), _TinyField(4).eval()
    rays = _cpu_rays(N, 5)
    t_ref, w_ref = _hand_weights(prop, rays, P, sigma_scale=0.75)
    t_prop, w_prop = proposal_weights(prop, rays, P, sigma_scale=0.75)
    assert torch.equal(t_prop, t_ref) and torch.equal(w_prop, w_ref) and w_prop.requires_grad
    assert float(w_prop.detach().min()) >= 0 and 0 < float(w_prop.detach().sum(1).max()) <= 1 + 1e-6
    t_fine = sample_pdf(t_prop, w_prop.detach(), F)
    ref = render_rays_at(m, rays, t_fine, sigma_scale=0.75)
    out = render_rays_proposal(m, prop, rays, P, F, sigma_scale=0.75, return_proposal=True, return_t_vals=True)
    assert len(out) == 6 and out[2].shape == (N, F)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], ref))
    assert torch.equal(out[4][0], t_prop) and torch.equal(out[4][1], w_prop) and torch.equal(out[5], t_fine)
    assert bool((t_fine[:, 1:] >= t_fine[:, :-1]).all()) and not t_fine.requires_grad
    plain = render_rays(m, rays, ray_samples=P, n_importance=F, proposal=prop, sigma_scale=0.75)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, ref))
    plain = render_rays(m, rays, P, None, None, "white", 1 << 20, 0.75, True, n_importance=F, proposal=prop,
                        _want_weights=False)
    assert len(plain) == 5 and torch.equal(plain[0], ref[0]) and torch.equal(plain[4], t_fine)
    # training mode: both jitters as given, the proposal's depths jittered iff the proposal trains
    g = torch.Generator().manual_seed(8)
    u, uf = torch.rand(N, P, generator=g), torch.rand(N, F, generator=g)
    m.train(), prop.train()
    t_ref, w_ref = _hand_weights(prop, rays, P, u=u)
    out = render_rays_proposal(m, prop, rays, P, F, jitter_u=u, jitter_fine=uf, return_proposal=True,
                               return_t_vals=True)
    assert torch.equal(out[4][0], t_ref) and torch.equal(out[4][1], w_ref)
    t_fine = sample_pdf(t_ref, w_ref.detach(), F, uf)
    assert torch.equal(out[5], t_fine)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], render_rays_at(m, rays, t_fine)))
    # the image never reaches the proposal, the proposal's weights never reach the model
    assert all(x is None for x in torch.autograd.grad(out[0].sum(), list(prop.parameters()), allow_unused=True,
                                                      retain_graph=True))
    assert all(x is None for x in torch.autograd.grad(out[4][1].sum(), list(m.parameters()), allow_unused=True,
                                                      retain_graph=True))
    rg = rays.clone().requires_grad_(True)
    t2, w2 = proposal_weights(prop, rg, P, jitter_u=u)
    assert torch.equal(w2, w_ref)
    w2.sum().backward()
    assert rg.grad is None                                           # never differentiable in the rays


def test_compute_loss_routes_the_gradients():
    from adaptive_city_nerf_amd import interlevel_loss, render_rays
    from adaptive_city_nerf_amd.train import adapt_step, compute_loss, mse_color_loss
    N, S, F = 32, 12, 10
    P = SimpleNamespace(ray_samples=S, chunk_points=1 << 20, color_space="linear")
    m, prop = _TinyField(3).train(), _TinyField(4).train()
    rays = _cpu_rays(N, 6)
    g = torch.Generator().manual_seed(9)
    rgbs, u, uf = torch.rand(N, 3, generator=g), torch.rand(N, S, generator=g), torch.rand(N, F, generator=g)
    kw = dict(n_importance=F, jitter_u=u, jitter_fine=uf)
    rgb, _, w, _, (t_prop, w_prop), t_fine = render_rays(m, rays, ray_samples=S, proposal=prop, return_proposal=True,
                                                         return_t_vals=True, **kw)
    inter = interlevel_loss(t_fine, w, t_prop, w_prop, rays=rays)
    assert float(inter.detach()) > 0
    main = [p for n, p in m.named_parameters() if n[0] in "ab"]
    assert all(x is None for x in torch.autograd.grad(inter, main, allow_unused=True, retain_graph=True))
    gp = torch.autograd.grad(inter, [prop.c.weight, prop.d.weight])
    assert all(bool(torch.isfinite(x).all()) for x in gp) and any(float(x.abs().max()) > 0 for x in gp)
    total = compute_loss(P, m, {"rays": rays, "rgbs": rgbs}, proposal=prop, interlevel_weight=0.5, **kw)
    want = mse_color_loss(rgb, rgbs, "linear") + 0.5 * inter
    assert float(total.detach()) == pytest.approx(float(want.detach()), rel=1e-6)
    with_d = compute_loss(P, m, {"rays": rays, "rgbs": rgbs}, proposal=prop, distortion_weight=0.1, **kw)
    plain = compute_loss(P, m, {"rays": rays, "rgbs": rgbs}, proposal=prop, **kw)
    assert float(with_d.detach()) > float(plain.detach())
    with pytest.raises(ValueError, match="n_importance"):
        compute_loss(P, m, {"rays": rays, "rgbs": rgbs}, proposal=prop)
    # one step with a plain optimizer over both fields moves both; the clip norm covers both
    opt = torch.optim.Adam(list(m.parameters()) + list(prop.parameters()), lr=1e-2)
    before = [p.detach().clone() for p in list(m.parameters()) + list(prop.parameters())]
    loss = adapt_step(P, m, rays, rgbs, opt, proposal=prop, grad_clip=1e-3, **kw)
    assert np.isfinite(float(loss))
    norm = torch.sqrt(sum((p.grad ** 2).sum() for p in list(m.parameters()) + list(prop.parameters())
                          if p.grad is not None))
    assert float(norm) <= 1e-3 * (1 + 1e-4)
    assert not torch.equal(before[0], m.a.weight) and not torch.equal(before[-2], prop.d.weight)
    assert m.c.weight.grad is None and prop.a.weight.grad is None    # the unused halves of the stand-ins
    with pytest.raises(ValueError, match="optimizer"):
        adapt_step(P, m, rays, rgbs, torch.optim.Adam(m.parameters()), proposal=prop, **kw)
    with pytest.raises(ValueError, match="group"):
        adapt_step(P, m, rays, rgbs, opt, proposal=prop, group=object(), **kw)


def test_entry_point_is_declared_bound_and_built():
    import adaptive_city_nerf_amd as A
    from adaptive_city_nerf_amd import _lib
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step, compute_loss, runtime_adapt
    text = (REPO / "include" / "acnerf.h").read_text()
    assert "acn_interlevel_loss" in re.findall(r"^(?:int|size_t)\s+(acn_\w+)\s*\(", text, re.M)
    assert "#define ACN_ABI_VERSION 1" in text or re.search(r"ACN_ABI_VERSION\s+1\b", text)
    assert "acn_interlevel_loss" in _lib.exported_symbols()
    make = (REPO / "adaptive_city_nerf_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\binterlevel\.hip\b", make, re.M)
    assert "interlevel_loss_kernel" in (REPO / "tools" / "spill_guard.py").read_text()
    src = (REPO / "adaptive_city_nerf_amd" / "csrc" / "resample.hip").read_text()
    dev = (REPO / "adaptive_city_nerf_amd" / "csrc" / "acn_device.h").read_text()
    assert "int prefix_count(" in dev and "int prefix_count(" not in src      # moved, not copied
    L = _lib.lib()

    def last_error():
        buf = ctypes.create_string_buffer(512)
        L.acn_last_error(buf, 512)
        return buf.value.decode()

    def call(S, P, N):
        return L.acn_interlevel_loss(None, None, S, None, None, P, N, None, R.EPS, None, None, None)

    for S, P in ((1025, 8), (8, 1025), (1, 8), (8, 1)):          # refused before any HIP call
        assert call(S, P, 4) != 0 and "1024" in last_error()
    assert call(8, 8, -1) != 0
    assert call(8, 8, 4) != 0 and "NULL" in last_error()
    assert call(8, 8, 0) == 0                                    # nothing launched
    for name in ("interlevel_loss", "proposal_weights", "render_rays_proposal"):
        assert getattr(A, name) is getattr(A.ray_rendering, name)
    assert list(inspect.signature(A.ops.interlevel_loss).parameters) == [
        "t_fine", "w_fine", "t_prop", "w_prop", "ray_scale", "eps", "want_grad"]
    assert list(inspect.signature(A.interlevel_loss).parameters)[:6] == [
        "t_vals", "weights", "t_prop", "w_prop", "rays", "reduction"]
    assert list(inspect.signature(A.proposal_weights).parameters) == [
        "proposal", "rays", "n_proposal", "params", "sigma_scale", "jitter_u"]
    assert list(inspect.signature(A.render_rays_proposal).parameters)[:15] == [
        "model", "proposal", "rays", "n_proposal", "n_fine", "params", "proposal_params", "active_module",
        "bg_color_default", "sigma_scale", "chunk", "jitter_u", "jitter_fine", "return_proposal", "return_t_vals"]
    for fn in (compute_loss, adapt_step, runtime_adapt):
        ps = inspect.signature(fn).parameters
        assert ps["proposal"].default is None and ps["interlevel_weight"].default == 1.0
    assert inspect.signature(GraphedAdaptStep.__init__).parameters["proposal"].default is None
    assert isinstance(A.ray_rendering.FUSED_INTERLEVEL, bool)
    assert "multinerf" in A.interlevel_loss.__doc__ and "tight bound" in A.interlevel_loss.__doc__
