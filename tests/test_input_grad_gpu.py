"""Input gradients (points, directions, rays) of the HIP encoders and of everything built on them, against the
float64 autograd of the torch restatement (tests/input_grad_ref.py).  Tolerances: the hash-grid kernel within
2e-6 * B elementwise (B: the sum of the absolute terms, ~32 fp32 roundings: 7 difference / lerp steps plus 2L
accumulations); composed quantities within 2e-5 * max(1, max|ref|), the convention of test_hashgrid_bwd_vs_reference;
forward values within the project's RGB 1e-4 / sigma 1e-5 (relative)."""
from functools import lru_cache

import pytest
import torch

import goldens as G
import input_grad_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
GENERIC = "gen_L5_F4_T10"


def _ops():
    from adaptive_city_nerf_amd import ops
    return ops


@lru_cache(maxsize=None)
def _case(name):
    """(x01, g, table, res, log2T, F, interp) on the GPU; shared, never modified."""
    d = G.load("hashgrid")
    x = torch.from_numpy(d["x01"]).to(DEV)
    if name == GENERIC:
        L, log2T, F, interp, seed = 5, 10, 4, 1, 21
        res = O.level_resolutions(5, 16, 256).tolist()
    else:
        L, mn, mx, log2T, seed, interp = [int(v) for v in d[f"{name}:cfg"]]
        F, res = 2, d[f"{name}:resolutions"].tolist()
    from adaptive_city_nerf_amd.synthetic import formula_table
    tab = torch.from_numpy(formula_table(L, log2T, F, seed=seed, scale=0.5)).to(DEV)
    g = torch.randn(x.shape[0], L * F, generator=torch.Generator().manual_seed(seed + 100)).to(DEV)
    return x, g, tab, res, log2T, F, interp


@lru_cache(maxsize=None)
def _full(name):
    x, g, tab, res, log2T, F, interp = _case(name)
    return _ops().hashgrid_bwd_input(x, g, tab, res, log2T, F, interp)


@pytest.mark.parametrize("name", ["smooth_L16_T12", "lin_L8_T14_r2_512", "lin_L4_T19", "lin_L16_T20", GENERIC])
def test_hashgrid_bwd_input_vs_float64_autograd(name):
    x, g, tab, res, log2T, F, interp = _case(name)
    got = _full(name).double()
    ref, B = R.hashgrid_grad(x, g, tab, res, log2T, interp, dtype=torch.float64, weights="fp32")
    err = (got - ref).abs()
    ratio = float((err / B.clamp_min(1e-300)).max())
    print(f"{name}: max|got - ref| / B = {ratio:.3e}, max|ref| = {float(ref.abs().max()):.3e}")
    assert bool((got[B == 0] == 0).all())
    assert bool((err <= 2e-6 * B).all())


@pytest.mark.parametrize("name", ["lin_L16_T20", "smooth_L16_T12"])
def test_ragged_prefixes_equal_the_full_batch(name):
    x, g, tab, res, log2T, F, interp = _case(name)
    full = _full(name)
    for M in (1, 63, 65, 1000):
        assert torch.equal(_ops().hashgrid_bwd_input(x[:M], g[:M], tab, res, log2T, F, interp), full[:M]), M
    e = _ops().hashgrid_bwd_input(x[:0], g[:0], tab, res, log2T, F, interp)
    assert e.shape == (0, 3)


def test_nearest_gives_exact_zeros():
    x, g, tab, res, log2T, F, interp = _case("near_L16_T12")
    assert interp == 0
    got = _ops().hashgrid_bwd_input(x, g, tab, res, log2T, F, interp)
    assert got.shape == x.shape and bool((got == 0).all())


@pytest.mark.parametrize("name", ["smooth_L16_T12", "lin_L16_T20", GENERIC])
def test_run_to_run_bitwise(name):
    x, g, tab, res, log2T, F, interp = _case(name)
    assert torch.equal(_ops().hashgrid_bwd_input(x, g, tab, res, log2T, F, interp), _full(name))


def _encoder(interp="Linear"):
    from adaptive_city_nerf_amd.encodings import HashGridEncoder
    torch.manual_seed(5)
    enc = HashGridEncoder(levels=16, min_res=16, max_res=4096, log2_hashmap_size=12, features_per_level=2,
                          interpolation=interp).to(DEV)
    with torch.no_grad():
        enc.hash_table.uniform_(-0.5, 0.5)
    return enc


def test_autograd_wiring_of_the_hash_grid():
    from adaptive_city_nerf_amd._lib import AcnError
    ops = _ops()
    enc = _encoder("Smoothstep")
    gen = torch.Generator().manual_seed(6)
    x0 = torch.rand(1000, 3, generator=gen).to(DEV)
    g = torch.randn(1000, 32, generator=gen).to(DEV)
    x = x0.clone().requires_grad_()
    enc(x).backward(g)
    want = ops.hashgrid_bwd_input(x0, g, enc.hash_table, enc._res_host, 12, 2, enc._interp_code)
    assert torch.equal(x.grad, want) and float(want.abs().max()) > 0
    # the table gradient does not depend on whether the points are differentiated
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        enc.hash_table.grad = None
        enc(x0.clone().requires_grad_()).backward(g)
        with_x = enc.hash_table.grad.clone()
        enc.hash_table.grad = None
        enc(x0).backward(g)
        assert torch.equal(with_x, enc.hash_table.grad)
    finally:
        torch.use_deterministic_algorithms(prev)
    x = x0.clone().requires_grad_()
    with pytest.raises(AcnError, match="second-order"):
        torch.autograd.grad(enc(x), x, g, create_graph=True)
    # an in-place change of the table between forward and backward is caught by autograd
    x = x0.clone().requires_grad_()
    y = enc(x)
    with torch.no_grad():
        enc.hash_table.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(g)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_sh_bwd_vs_float64_autograd(levels):
    from adaptive_city_nerf_amd.encodings import SHEncoder
    gen = torch.Generator().manual_seed(40 + levels)
    d = torch.randn(2048, 3, generator=gen)
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(2048, 1, generator=gen))
    tiny = torch.tensor([[0.6e-12, -0.64e-12, 0.48e-12]])          # |d| = 1e-12: under the clamp
    d = torch.cat([d, tiny], 0).to(DEV)
    g = torch.randn(2049, levels * levels, generator=gen).to(DEV)
    d64 = d.double().requires_grad_()
    enc64 = R.sh(d64, levels)
    if enc64.requires_grad:
        (ref,) = torch.autograd.grad((enc64 * g.double()).sum(), d64)
    else:                        # levels == 1: the constant component only
        ref = torch.zeros_like(d64)
    got = _ops().sh_bwd(d, g, levels).double()
    err = float((got[:-1] - ref[:-1]).abs().max())
    print(f"levels={levels}: max|got - ref| = {err:.3e}, max|ref| = {float(ref[:-1].abs().max()):.3e}")
    assert err <= 2e-5 * max(1.0, float(ref[:-1].abs().max()))
    if levels == 1:
        assert bool((got == 0).all())
    else:
        torch.testing.assert_close(got[-1], ref[-1], rtol=1e-5, atol=0)
    # the module under autograd is the kernel
    dd = d.clone().requires_grad_()
    SHEncoder(levels)(dd).backward(g)
    assert torch.equal(dd.grad.double(), got)


# ------------------------------------------------------------------------------------------------- field
HASH_CONF = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": 12, "max_res": 4096, "min_res": 16,
             "interpolation": "Linear"}


def _expert():
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    torch.manual_seed(11)
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=HASH_CONF, dir_encoding="spherical").to(DEV)
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    assert m._fusable
    return m


def _torch_encoders(m):
    """Patch the two encoders of ``m`` with the float32 torch restatements (autograd supplies their gradients)."""
    enc = m.xyz_encoder
    enc.forward = lambda x: R.hashgrid(x, enc.hash_table, enc._res_host, enc.log2_hashmap_size, enc._interp_code,
                                       dtype=torch.float32, weights="fp32")
    m.dir_encoder.forward = lambda d: R.sh(d, m.dir_encoder.levels)


def _close(got, ref):
    got, ref = got.detach(), ref.detach()
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"max|got - ref| = {err:.3e} (tolerance {tol:.3e}, max|ref| = {float(ref.abs().max()):.3e})")
    return err <= tol


def _field_inputs(n=500, seed=12):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=gen) * 1.8 - 0.9
    return torch.cat([x, torch.randn(n, 3, generator=gen)], -1).to(DEV)


def test_field_output_is_differentiable_in_its_inputs():
    m = _expert().eval().requires_grad_(False)
    x_d0 = _field_inputs()
    with torch.no_grad():
        fused = m(x_d0)
    x_d = x_d0.clone().requires_grad_()
    y = m(x_d)
    assert y.grad_fn is not None
    y = y.detach()
    assert float((y[:, :3] - fused[:, :3]).abs().max()) <= 1e-4
    assert float(((y[:, 3] - fused[:, 3]).abs() / fused[:, 3].abs().clamp_min(1.0)).max()) <= 1e-5


@pytest.mark.parametrize("variant", ["forward", "density", "params_grad", "train"])
def test_field_input_gradient_vs_torch_encoders(variant):
    m = _expert().eval()
    if variant == "train":
        m.train()
    if variant not in ("params_grad", "train"):
        m.requires_grad_(False)
    x_d0 = _field_inputs()
    wgt = torch.randn(500, 4, generator=torch.Generator().manual_seed(13)).to(DEV)

    def grad_of(model):
        x_d = x_d0.clone().requires_grad_()
        if variant == "density":
            out = (model.density(x_d[:, :3]) * wgt[:, 3:4]).sum()
        else:
            out = (model(x_d) * wgt).sum()
        (gx,) = torch.autograd.grad(out, x_d)
        return gx

    got = grad_of(m)
    _torch_encoders(m)
    ref = grad_of(m)
    assert float(ref[:, :3].abs().max()) > 0
    if variant != "density":
        assert float(ref[:, 3:].abs().max()) > 0
    assert _close(got, ref)


# ------------------------------------------------------------------------------------------------- container
def _container(tag="k4", bm=None):
    from adaptive_city_nerf_amd import MetaContainer, SceneBox
    sc = G.scene()["masks"][G.MASK[tag]]
    K = len(sc["centroids"])
    gbox = SceneBox(aabb=torch.tensor(sc["aabb_global"], dtype=torch.float32))
    boxes = [SceneBox(aabb=torch.tensor([sc["mins"][k], sc["maxs"][k]], dtype=torch.float32)) for k in range(K)]
    torch.manual_seed(0)
    m = MetaContainer(num_submodules=K, centroids=torch.tensor(sc["centroids"]), aabb=gbox.aabb,
                      nerf_variant="instant",
                      boundary_margin=min(max(1.0, 1.05), sc["boundary_margin"]) if bm is None else bm,
                      cluster_2d=sc["cluster_2d"], joint_training=False, use_bg_nerf=True, bg_hidden=32,
                      bg_encoding="spherical", occ_conf={"use_occ": False}, expert_box_list=boxes, hidden=64,
                      sigma_depth=2, color_depth=2, dir_encoding="spherical", color_hidden=64, use_sigmoid_rgb=True,
                      hash_enc_conf=HASH_CONF).to(DEV)
    with torch.no_grad():
        for sub in m.submodules:
            sub.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    return m.eval().requires_grad_(False), gbox


def _container_points(m, gbox, n, seed):
    """n points of the global box, half of them within ~1% of the bisector plane of two centroids."""
    gen = torch.Generator().manual_seed(seed)
    lo, hi = gbox.min.cpu(), gbox.max.cpu()
    x = lo + (hi - lo) * torch.rand(n, 3, generator=gen)
    c = m.centroids.cpu()
    K = c.shape[0]
    cols = list(m._coord_idx)
    h = n // 2
    i = torch.randint(0, K, (h,), generator=gen)
    j = (i + 1 + torch.randint(0, K - 1, (h,), generator=gen)) % K
    ci, cj = c[i][:, cols], c[j][:, cols]
    nrm = cj - ci
    p = 0.5 * (ci + cj) + nrm * ((torch.rand(h, 1, generator=gen) - 0.5) * 0.02)
    if len(cols) == 2:
        perp = torch.stack([-nrm[:, 1], nrm[:, 0]], -1)
        p = p + perp * ((torch.rand(h, 1, generator=gen) - 0.5) * 0.6)
    x[:h, cols] = p
    return x.to(DEV)


def test_container_hard_routing_and_active_module():
    m, gbox = _container(bm=1.0)
    pts = _container_points(m, gbox, 512, seed=30)
    x0 = torch.cat([pts, torch.randn(512, 3, generator=torch.Generator().manual_seed(31)).to(DEV)], -1)
    wgt = torch.randn(512, 4, generator=torch.Generator().manual_seed(32)).to(DEV)
    _, hard = m._routing(pts)
    x = x0.clone().requires_grad_()
    y = m(x)
    assert y.grad_fn is not None
    (gx,) = torch.autograd.grad((y * wgt).sum(), x)
    for k, sub in enumerate(m.submodules):
        sel = (hard == k).nonzero().squeeze(1)
        xk = x0[sel].clone().requires_grad_()
        yk = sub(xk)
        (gk,) = torch.autograd.grad((yk * wgt[sel]).sum(), xk)
        assert _close(y[sel], yk) and _close(gx[sel], gk)
        xa = x0[sel].clone().requires_grad_()
        ya = m(xa, active_module=k)
        (ga,) = torch.autograd.grad((ya * wgt[sel]).sum(), xa)
        assert torch.equal(ya, yk) and torch.equal(ga, gk)


def test_container_soft_routing_weights_and_gradient():
    ops = _ops()
    m, gbox = _container()
    assert m.boundary_margin > 1.0
    pts = _container_points(m, gbox, 4096, seed=33)
    W, _ = ops.routing_fwd(pts, m.routing_spec())
    mask = W > 0
    assert int((mask.sum(-1) > 1).sum()) > 256          # the boundary points do see several experts
    x = pts.clone().requires_grad_()
    w = m._soft_weights(x, mask)
    assert torch.equal(w > 0, mask)
    assert float((w - W).abs().max()) <= 1e-6
    Wr, _ = m._routing(x)
    assert Wr.grad_fn is not None and torch.equal(Wr, w)
    G_ = torch.randn(4096, W.shape[1], generator=torch.Generator().manual_seed(34)).to(DEV)
    (got,) = torch.autograd.grad((w * G_).sum(), x)
    x64 = pts.double().requires_grad_()
    cols = list(m._coord_idx)
    dist = (x64[:, None, cols] - m.centroids.double()[None, :, cols]).pow(2).sum(-1).sqrt().clamp_min(1e-6)
    inv = torch.where(mask, 1.0 / dist, torch.zeros_like(dist))
    w64 = inv / inv.sum(-1, keepdim=True).clamp_min(1e-6)
    (ref,) = torch.autograd.grad((w64 * G_.double()).sum(), x64)
    assert _close(got.double(), ref)
    # the field through the soft blend
    xd = torch.cat([pts, torch.randn(4096, 3, generator=torch.Generator().manual_seed(35)).to(DEV)], -1)
    xd.requires_grad_()
    y = m(xd)
    (gx,) = torch.autograd.grad(y.sum(), xd)
    multi = mask.sum(-1) > 1
    assert bool(torch.isfinite(gx).all()) and bool((gx[multi][:, :3].abs().sum(-1) > 0).all())
    sig = m.density(xd[:, :3])
    assert sig.grad_fn is not None
    rgb = m.color(xd[:, :3], xd[:, 3:])
    assert rgb.grad_fn is not None


# ------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("tag", ["k1", "k4"])
def test_render_rays_gradient(tag):
    from adaptive_city_nerf_amd import render_rays
    from adaptive_city_nerf_amd._lib import AcnError
    from adaptive_city_nerf_amd.ray_rendering import render_rays_occ, stratified_t_vals, volume_render
    m, _ = _container(tag)
    S = 16
    rays0 = torch.from_numpy(G.load(f"render_{tag}")["render:rays"][:64]).to(DEV)
    gen = torch.Generator().manual_seed(50)
    wr, wd = torch.randn(64, 3, generator=gen).to(DEV), torch.randn(64, generator=gen).to(DEV)
    with torch.no_grad():
        fused = render_rays(m, rays0, ray_samples=S)
    rays = rays0.clone().requires_grad_()
    out = render_rays(m, rays, ray_samples=S)
    assert out[0].grad_fn is not None
    assert float((out[0] - fused[0]).abs().max()) <= 1e-4            # rgb
    assert float((out[3] - fused[3]).abs().max()) <= 1e-4            # acc
    assert float((out[1] - fused[1]).abs().max()) <= 1e-4            # depth
    assert float((out[2] - fused[2]).abs().max()) <= 1e-5            # weights
    (got,) = torch.autograd.grad((out[0] * wr).sum() + (out[1] * wd).sum(), rays)
    assert bool((got[:, 6:] == 0).all()) and float(got[:, :3].abs().max()) > 0 and float(got[:, 3:6].abs().max()) > 0
    # the same composition written out: constant t-values, the model call, the compositing
    r2 = rays0.clone().requires_grad_()
    o, d = r2[:, :3], r2[:, 3:6]
    t = stratified_t_vals(r2[:, 6], r2[:, 7], S, randomized=False)
    pts = o.unsqueeze(1) + d.unsqueeze(1) * t.unsqueeze(-1)
    dirs = d.unsqueeze(1).expand_as(pts)
    rgb_sigma = m(torch.cat([pts, dirs], dim=-1).reshape(-1, 6)).view(64, S, 4)
    rgb, depth, _, _ = volume_render(rgb_sigma, t, bg_rgb=m.background_color(dirs[:, 0]))
    (ref,) = torch.autograd.grad((rgb * wr).sum() + (depth * wd).sum(), r2)
    assert torch.equal(got, ref)
    with pytest.raises(AcnError, match="occupancy"):
        render_rays_occ(m, rays0.clone().requires_grad_())
