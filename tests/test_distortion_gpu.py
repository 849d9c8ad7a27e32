"""The fused distortion loss on the GPU (acn_distortion_packed / acn_distortion_dense) against the O(S^2)
float64 definition of tests/distortion_ref.py, and its way up: autograd through the compositing, nerfacc.distortion on
packed samples, render_rays_stratified(return_t_vals=True), adapt_step / GraphedAdaptStep / runtime_adapt with a
distortion weight.

The kernel carries its sums in float64 and rounds each output to fp32 once, so for every ray
|got - ref| <= 4 * 2^-24 * max|ref| + 1e-30 for the loss and for the gradient (four fp32 roundings against the one the
arithmetic performs); the worst ratio to that bound is printed."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import distortion_ref as R
import goldens as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 4 * 2.0 ** -24
OFFSETS = (0.0, 100.0, 5000.0)
PACKED_COUNTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 300, 17, 0, 91, 200]   # the last four: "a few random ones"
OPAQUE_RAY = 5
DENSE_SHAPES = [(37, 2), (5, 64), (3, 65), (64, 96), (9, 256), (2, 1000)]


def _ratio(got, ref, ray_max):
    """Worst |got - ref| over its bound BOUND * (the ray's largest |ref|) + 1e-30."""
    return float(((got.detach().double().cpu() - ref).abs() / (BOUND * ray_max + 1e-30)).max())


def _ray_max(v, starts, counts):
    per_ray = torch.stack([v[s:s + c].abs().max() if c else v.new_zeros(()) for s, c in zip(starts.tolist(),
                                                                                             counts.tolist())])
    return per_ray, torch.repeat_interleave(per_ray, counts)


@lru_cache(maxsize=None)
def _packed(offset):
    """CPU inputs and the float64 reference, computed once and never modified."""
    gen = torch.Generator().manual_seed(100 + int(offset))
    w, t0, t1, starts, counts = R.packed_case(PACKED_COUNTS, offset, gen, opaque_ray=OPAQUE_RAY)
    assert float((w == 0).float().mean()) > 0.3 and float(w[starts[OPAQUE_RAY]]) == 1.0
    loss, grad = R.packed(w, t0, t1, starts, counts)
    return (w, t0, t1, starts, counts), (loss, grad)


@lru_cache(maxsize=None)
def _dense(shape, offset):
    gen = torch.Generator().manual_seed(200 + 7 * shape[1] + int(offset))
    w, t = R.dense_case(shape[0], shape[1], offset, gen, opaque_ray=0)
    assert float(w[0, 0]) == 1.0 and bool((w[0, 1:] == 0).all())
    return (w, t), R.dense(w, t)


@pytest.mark.parametrize("offset", OFFSETS)
def test_packed_kernel_matches_the_definition(offset):
    from adaptive_city_nerf_amd import occ_ops
    (w, t0, t1, starts, counts), (ref_l, ref_g) = _packed(offset)
    N = len(PACKED_COUNTS)
    args = [x.to(DEV) for x in (w, t0, t1, starts, counts)]
    loss, grad = occ_ops.distortion_packed(*args)
    lmax, (_, gmax) = ref_l.abs(), _ray_max(ref_g, starts, counts)
    r_l, r_g = _ratio(loss, ref_l, lmax), _ratio(grad, ref_g, gmax)
    print(f"packed, t offset {offset}: loss at {r_l:.3f}, gradient at {r_g:.3f} of the bound")
    assert r_l <= 1 and r_g <= 1
    assert float(loss[0]) == 0.0 and float(loss[11]) == 0.0                  # empty rays
    # bitwise reproducible, and the loss does not depend on whether the gradient is written
    loss2, grad2 = occ_ops.distortion_packed(*args)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    loss3, none = occ_ops.distortion_packed(*args, want_grad=False)
    assert none is None and torch.equal(loss, loss3)
    # a power-of-two ray scale is exact; any scale stays within the bound of the scaled definition; scale 0 gives
    # exact zeros although that ray's t values are NaN
    gen = torch.Generator().manual_seed(3)
    p2 = 2.0 ** torch.randint(-3, 4, (N,), generator=gen).float()
    loss_p, grad_p = occ_ops.distortion_packed(*args, ray_scale=p2.to(DEV))
    assert torch.equal(loss_p.cpu(), loss.cpu() * p2)
    assert torch.equal(grad_p.cpu(), grad.cpu() * torch.repeat_interleave(p2, counts))
    scale = torch.rand(N, generator=gen) * 0.2 + 0.01
    dead = 8
    scale[dead] = 0.0
    sl = slice(int(starts[dead]), int(starts[dead] + counts[dead]))
    t0n, t1n = t0.clone(), t1.clone()
    t0n[sl] = t1n[sl] = float("nan")
    loss_s, grad_s = occ_ops.distortion_packed(args[0], t0n.to(DEV), t1n.to(DEV), args[3], args[4],
                                               ray_scale=scale.to(DEV))
    ref_ls, ref_gs = R.packed(w, t0, t1, starts, counts, scale)
    r_l, r_g = _ratio(loss_s, ref_ls, ref_ls.abs()), _ratio(grad_s, ref_gs, _ray_max(ref_gs, starts, counts)[1])
    print(f"packed, t offset {offset}, scaled: loss at {r_l:.3f}, gradient at {r_g:.3f} of the bound")
    assert r_l <= 1 and r_g <= 1
    assert float(loss_s[dead]) == 0.0 and bool((grad_s[sl] == 0).all()) and int(counts[dead]) == 256
    assert bool(torch.isfinite(loss_s).all()) and bool(torch.isfinite(grad_s).all())


@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_kernel_matches_the_definition(shape):
    from adaptive_city_nerf_amd import ops
    N, S = shape
    for offset in OFFSETS:
        (w, t), (ref_l, ref_g) = _dense(shape, offset)
        wd, td = w.to(DEV), t.to(DEV)
        loss, grad = ops.distortion_dense(wd, td)
        r_l = _ratio(loss, ref_l, ref_l.abs())
        r_g = _ratio(grad, ref_g, ref_g.abs().amax(1, keepdim=True))
        print(f"dense {shape}, t offset {offset}: loss at {r_l:.3f}, gradient at {r_g:.3f} of the bound")
        assert r_l <= 1 and r_g <= 1
        loss2, grad2 = ops.distortion_dense(wd, td)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
        loss3, none = ops.distortion_dense(wd, td, want_grad=False)
        assert none is None and torch.equal(loss, loss3)
        p2 = 2.0 ** (torch.arange(N) % 5 - 2).float()
        loss_p, grad_p = ops.distortion_dense(wd, td, ray_scale=p2.to(DEV))
        assert torch.equal(loss_p.cpu(), loss.cpu() * p2) and torch.equal(grad_p.cpu(), grad.cpu() * p2[:, None])
        scale = torch.linspace(0.02, 0.3, N)
        dead = N - 1
        scale[dead] = 0.0
        tn = t.clone()
        tn[dead] = float("nan")
        loss_s, grad_s = ops.distortion_dense(wd, tn.to(DEV), ray_scale=scale.to(DEV))
        ref_ls, ref_gs = R.dense(w, t, scale)
        assert _ratio(loss_s, ref_ls, ref_ls.abs()) <= 1
        assert _ratio(grad_s, ref_gs, ref_gs.abs().amax(1, keepdim=True)) <= 1
        assert float(loss_s[dead]) == 0.0 and bool((grad_s[dead] == 0).all())
        assert bool(torch.isfinite(loss_s).all()) and bool(torch.isfinite(grad_s).all())


def test_distortion_loss_function_and_reductions():
    """ray_rendering.distortion_loss on the GPU: the fused Function's backward is g_loss[r] * grad_w, the ray scale
    comes from the rays' near / far, and the torch form taken inside second_order() agrees with the kernel."""
    from adaptive_city_nerf_amd import distortion_loss, ops
    from adaptive_city_nerf_amd.ray_rendering import second_order
    (w, t), _ = _dense((64, 96), 100.0)
    wd, td = w.to(DEV), t.to(DEV)
    rays = torch.zeros(64, 8, device=DEV)
    rays[:, 6], rays[:, 7] = td[:, 0], td[:, -1]
    rays[5, 6:] = float("nan")
    scale = 1.0 / (rays[:, 7] - rays[:, 6])
    scale[5] = 0.0
    loss_k, grad_k = ops.distortion_dense(wd, td, ray_scale=scale)
    wl = wd.clone().requires_grad_(True)
    loss = distortion_loss(wl, td, rays=rays, reduction="none")
    assert torch.equal(loss.detach(), loss_k)
    g_loss = 2.0 ** (torch.arange(64, device=DEV) % 3).float()
    (loss * g_loss).sum().backward()
    assert torch.equal(wl.grad, grad_k * g_loss[:, None])
    with torch.no_grad():
        assert torch.equal(distortion_loss(wd, td, rays=rays), loss_k.mean())
        assert torch.equal(distortion_loss(wd, td, rays=rays, reduction="sum"), loss_k.sum())
    w2 = wd.clone().requires_grad_(True)
    with second_order():
        loss_t = distortion_loss(w2, td, rays=rays, reduction="none")
        g_t, = torch.autograd.grad(loss_t.sum(), w2, create_graph=True)
    assert g_t.requires_grad
    assert float((loss_t.detach() - loss_k).abs().max()) <= 2.0 ** -23 * float(loss_k.abs().max())
    assert float((g_t.detach() - grad_k).abs().max()) <= 2.0 ** -23 * float(grad_k.abs().max())


def test_gradient_through_the_compositing():
    """volume_render (HIP forward / backward) -> distortion_loss -> rgb_sigma.grad against float64 autograd of the
    reference formulas on the CPU, with test_volume_render_backward_matches_autograd's inputs and tolerance."""
    from adaptive_city_nerf_amd import distortion_loss
    from adaptive_city_nerf_amd.ray_rendering import _volume_render_autograd, volume_render
    d = G.load("volume_render")
    rs = torch.from_numpy(d["rgb_sigma"]).clone()
    t = torch.from_numpy(d["t_vals"]).clone()
    bg = torch.from_numpy(d["bg"]).clone()
    N, S = t.shape
    rs_c = rs.double().requires_grad_(True)
    w_c = _volume_render_autograd(rs_c, t.double(), bg.double(), False, False, 1.0)[2]
    m, dd = R.dense_intervals(t)
    sum(R.ray_loss(w_c[r], m[r], dd[r])[0] for r in range(N)).backward()
    rs_g = rs.to(DEV).requires_grad_(True)
    w_g = volume_render(rs_g, t.to(DEV), bg_rgb=bg.to(DEV))[2]
    loss = distortion_loss(w_g, t.to(DEV), reduction="sum")
    loss.backward()
    ref, got = rs_c.grad.numpy(), rs_g.grad.cpu().numpy()
    assert float(np.abs(ref[..., 3]).max()) > 0
    for c in range(4):
        sc = float(np.abs(ref[..., c]).max()) + 1e-12
        print(f"channel {c}: max|got - ref| = {np.abs(got[..., c] - ref[..., c]).max():.3e}, bound {2e-5 * sc:.3e}")
        np.testing.assert_allclose(got[..., c], ref[..., c], rtol=0, atol=2e-5 * sc)


def test_nerfacc_distortion_on_packed_samples():
    """render_weight_from_density -> nerfacc.distortion -> g_sigmas against float64 autograd of the oracle's formulas,
    within tests/test_occ_gpu.py's tolerance of the packed weights backward."""
    from adaptive_city_nerf_amd import nerfacc
    g = torch.Generator().manual_seed(0)
    counts = torch.randint(0, 200, (64,), generator=g)
    counts[3] = 0
    M = int(counts.sum())
    starts = torch.cumsum(counts, 0) - counts
    ri = torch.repeat_interleave(torch.arange(64), counts)
    dt = torch.rand(M, generator=g) * 0.02 + 1e-4
    t0 = torch.cumsum(dt, 0) - dt + 100.0
    t1 = t0 + dt
    sig = (torch.rand(M, generator=g) * 30 * (torch.rand(M, generator=g) < 0.5)).requires_grad_(True)
    gout = torch.randn(64, generator=g)
    sdt = sig.double() * (t1 - t0).double()
    total = 0.0
    ref_l = torch.zeros(64, dtype=torch.float64)
    for r in range(64):
        s, c = int(starts[r]), int(counts[r])
        if c:
            x = sdt[s:s + c]
            w = torch.exp(-(torch.cumsum(x, 0) - x)) * (1 - torch.exp(-x))
            a, b = t0[s:s + c].double(), t1[s:s + c].double()
            lr = R.ray_loss(w, 0.5 * (a + b), b - a)[0]
            ref_l[r] = lr.detach()
            total = total + lr * gout[r].double()
    total.backward()
    sg = sig.detach().to(DEV).requires_grad_(True)
    w, _, _ = nerfacc.render_weight_from_density(t0.to(DEV), t1.to(DEV), sg, ray_indices=ri.to(DEV), n_rays=64)
    loss = nerfacc.distortion(w, t0.to(DEV), t1.to(DEV), ray_indices=ri.to(DEV), n_rays=64)
    assert loss.shape == (64,)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref_l.numpy(), rtol=1e-4, atol=1e-7)
    (loss * gout.to(DEV)).sum().backward()
    print(f"max|g_sigmas - ref| = {float((sg.grad.cpu() - sig.grad).abs().max()):.3e}, "
          f"max|ref| = {float(sig.grad.abs().max()):.3e}")
    np.testing.assert_allclose(sg.grad.cpu().numpy(), sig.grad.numpy(), rtol=1e-4, atol=1e-5)
    # batched (N, S) rows go through the packed kernel too
    (wv, t), _ = _dense((5, 64), 0.0)
    dd = torch.cat([t[:, 1:] - t[:, :-1], t[:, -1:] - t[:, -2:-1]], 1)
    ref_b, _ = R.packed(wv.reshape(-1), t.reshape(-1), (t + dd).reshape(-1), torch.arange(5) * 64, torch.full((5,), 64))
    wb = wv.to(DEV).requires_grad_(True)
    got_b = nerfacc.distortion(wb, t.to(DEV), (t + dd).to(DEV))
    assert got_b.shape == (5,) and _ratio(got_b, ref_b, ref_b.abs()) <= 1
    got_b.sum().backward()
    assert wb.grad.shape == (5, 64) and bool(torch.isfinite(wb.grad).all())


def _bare_expert():
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    torch.manual_seed(11)
    conf = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": 12, "max_res": 4096, "min_res": 16,
            "interpolation": "Linear"}
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=conf, dir_encoding="spherical")
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    m = m.to(DEV)
    assert m._fusable
    return m


@pytest.mark.parametrize("train_order", [False, True])
def test_render_returns_its_t_vals(train_order):
    from adaptive_city_nerf_amd import ray_rendering as RR
    m = _bare_expert()
    gen = torch.Generator().manual_seed(9)
    o = torch.rand(64, 3, generator=gen) * 1.6 - 0.8
    dirs = torch.nn.functional.normalize(torch.randn(64, 3, generator=gen), dim=-1)
    near = 0.05 * torch.rand(64, generator=gen)
    far = near + 0.5 + torch.rand(64, generator=gen)
    rays_c = torch.cat([o, dirs, near[:, None], far[:, None]], 1)
    u_c = torch.rand(64, 32, generator=gen)
    rays, u = rays_c.to(DEV), u_c.to(DEV)
    prev = RR.TRAIN_RAY_ORDER
    RR.TRAIN_RAY_ORDER = train_order
    try:
        m.train()
        plain = RR.render_rays_stratified(m, rays, 32, jitter_u=u)
        out = RR.render_rays_stratified(m, rays, 32, jitter_u=u, return_t_vals=True)
        assert len(plain) == 4 and len(out) == 5 and out[0].requires_grad
        assert all(torch.equal(a, b) for a, b in zip(plain, out[:4]))
        assert torch.equal(out[4].cpu(), RR.stratified_t_vals(near, far, 32, randomized=True, u=u_c))
        with torch.no_grad():                      # the fused render in training mode: the same jitter
            out_ng = RR.render_rays_stratified(m, rays, 32, jitter_u=u, return_t_vals=True)
            assert torch.equal(out_ng[4].cpu(), out[4].cpu())
        m.eval()
        with torch.no_grad():
            plain = RR.render_rays(m, rays, ray_samples=32)
            out = RR.render_rays(m, rays, ray_samples=32, return_t_vals=True)
        assert len(plain) == 4 and len(out) == 5
        assert all(torch.equal(a, b) for a, b in zip(plain, out[:4]))
        assert torch.equal(out[4].cpu(), RR.stratified_t_vals(near, far, 32, randomized=False))
    finally:
        RR.TRAIN_RAY_ORDER = prev


def _setup():
    from test_graph_gpu import _setup as setup
    return setup()


def test_adapt_step_with_a_distortion_weight():
    from adaptive_city_nerf_amd import distortion_loss, render_rays
    from adaptive_city_nerf_amd.train import adapt_step
    P, m_plain, o_plain, d = _setup()
    _, m_zero, o_zero, _ = _setup()
    _, m_lam, o_lam, _ = _setup()
    _, m_render, _, _ = _setup()
    rays = torch.from_numpy(d["train0:rays"]).to(DEV)
    rgbs = torch.from_numpy(d["train0:rgbs"]).to(DEV)
    u = torch.from_numpy(d["train0:u"]).to(DEV)
    lam = 0.1
    l_plain = adapt_step(P, m_plain, rays, rgbs, o_plain, active_module=0, grad_clip=1.0, jitter_u=u)
    l_zero = adapt_step(P, m_zero, rays, rgbs, o_zero, active_module=0, grad_clip=1.0, jitter_u=u,
                        distortion_weight=0.0)
    assert torch.equal(l_plain, l_zero)
    l_lam = adapt_step(P, m_lam, rays, rgbs, o_lam, active_module=0, grad_clip=1.0, jitter_u=u, distortion_weight=lam)
    _, _, w, _, t = render_rays(m_render, rays, ray_samples=P.ray_samples, active_module=0, chunk=P.chunk_points,
                                jitter_u=u, return_t_vals=True)
    dist = float(distortion_loss(w.detach(), t, rays=rays))
    assert dist > 0
    # loss = fl(mse + fl(lam * dist)) in fp32: the sum is exact to a rounding of the loss itself, so the difference
    # of the two losses is compared relative to the loss
    diff = float(l_lam) - float(l_plain)
    print(f"loss {float(l_lam):.8f}, mse {float(l_plain):.8f}, difference {diff:.6e}, lam * dist {lam * dist:.6e}")
    assert abs(diff - lam * dist) <= 1e-6 * abs(float(l_lam))
    changed = False
    for pa, pb in zip(m_lam.parameters(), m_zero.parameters()):
        assert bool(torch.isfinite(pa).all())
        changed = changed or not torch.equal(pa, pb)
    assert changed


def test_graphed_adapt_step_with_a_distortion_weight_matches_eager():
    """tests/test_graph_gpu.py's comparison of graph replays with eager steps, its batches and tolerances, with the
    regulariser in the captured step."""
    from test_graph_gpu import _batches
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step
    lam, active_module = 0.1, 0
    P, ma, oa, d = _setup()
    _, mb, ob, _ = _setup()
    batches = _batches(d, 6, S=P.ray_samples)
    seq = [batches[0], batches[0]] + batches[1:]
    for rays, rgbs, u in seq:
        la = adapt_step(P, ma, rays, rgbs, oa, active_module=active_module, grad_clip=1.0, jitter_u=u,
                        distortion_weight=lam)
    g = GraphedAdaptStep(P, mb, batches[0][0], batches[0][1], ob, active_module=active_module, grad_clip=1.0,
                         warmup=2, jitter_u=batches[0][2], distortion_weight=lam)
    for rays, rgbs, u in batches[1:]:
        lb = g(rays, rgbs, jitter_u=u)
    torch.cuda.synchronize()
    g.sync_state()
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(la)) + 1e-8
    for (na, pa), (nb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        a, b = pa.detach().cpu().numpy(), pb.detach().cpu().numpy()
        bad = np.abs(a - b) > 1e-5 * np.abs(a) + 1e-7
        if na.endswith("hash_table"):
            assert bad.mean() <= 1e-5 and np.abs(a - b).max() <= 1e-4, (na, int(bad.sum()), np.abs(a - b).max())
        else:
            assert bad.mean() <= 1e-2 and np.abs(a - b).max() <= 2e-6, (na, int(bad.sum()), np.abs(a - b).max())
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        sa, sb = oa.state.get(pa, {}), ob.state.get(pb, {})
        assert ("step" in sa) == ("step" in sb)
        if "step" in sa:
            assert float(sa["step"]) == float(sb["step"]) == 7.0
            np.testing.assert_allclose(sb["exp_avg_sq"].cpu().numpy(), sa["exp_avg_sq"].cpu().numpy(), rtol=1e-4,
                                       atol=1e-12)


def test_runtime_adapt_with_a_distortion_weight_takes_the_eager_step():
    from adaptive_city_nerf_amd import train as T
    P, m, opt, d = _setup()
    rays = torch.from_numpy(d["train0:rays"]).to(DEV)
    rgbs = torch.from_numpy(d["train0:rgbs"]).to(DEV)
    before = [p.detach().clone() for p in m.parameters()]
    out = T.runtime_adapt(P=P, model=m, data_loader=[(rays, rgbs)], optimizer=opt, steps=2, distortion_weight=0.1)
    assert out["steps"] == 2 and np.isfinite(out["loss"]) and out["loss"] > 0
    assert not getattr(opt, "_acn_routed_steps", None)
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
