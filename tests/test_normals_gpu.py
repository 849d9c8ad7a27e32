"""The fused density-gradient kernel (acn_field_sigma_grad) and the rendered normal maps against
the float64 restatement of tests/normal_ref.py and against the four-launch chain of existing kernels it replaces.

Tolerances.  sigma: the project's parity, |got - ref| / max(1, |ref|) <= 1e-5.  The gradient is discontinuous where a
trunk pre-activation crosses zero, so samples whose reference has one with |z| < 1e-5 are set aside (at most 1 % of
them: the point seed was chosen on the CPU so that the reference alone meets this); on the others
max|got - ref| <= tol * max(1, max|ref|) with tol = max(2e-5, 4 e32) for exact-fp32 layer products (e32: the float32
CPU restatement's error in the same measure, §4r's end-to-end rule) and tol = max(2e-5, 4 e_chain) for fp16x3
(e_chain: the error, same run and measure, of hashgrid_fwd -> mlp_train_fwd -> mlp_train_bwd_input -> hashgrid_bwd_input
-> mask / extent, which uses the same layer products)."""
from functools import lru_cache

import pytest
import torch

import input_grad_ref as R
import normal_ref as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 16        # 500 points: 4 (Linear) / 5 (Smoothstep) of them within 1e-5 of a ReLU kink
HASH_CONF = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": 12, "max_res": 4096, "min_res": 16,
             "interpolation": "Linear"}
INTERPS = ["Linear", "Smoothstep"]


def _ops():
    from adaptive_city_nerf_amd import ops
    return ops


@lru_cache(maxsize=None)
def _expert(interp):
    """tests/test_input_grad_gpu.py's _expert() / HASH_CONF (L = 16, F = 2, log2T = 12, table uniform +-0.5) with the
    table drawn on the CPU, so that the reference can be examined without a GPU; shared, never modified."""
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    torch.manual_seed(11)
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=dict(HASH_CONF, interpolation=interp), dir_encoding="spherical")
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    m = m.to(DEV).eval().requires_grad_(False)
    assert m._fusable
    return m


@lru_cache(maxsize=None)
def _points():
    return (torch.rand(500, 3, generator=torch.Generator().manual_seed(SEED)) * 2.2 - 1.1).to(DEV)


def _ref_args(m, params=None):
    enc = m.xyz_encoder
    mn, ext = m._host_box()
    tensors = {k: v.detach().cpu() for k, v in m._mlp_tensors(params).items()}
    return (tensors, enc.hash_table.detach().cpu(), enc._res_host, enc.log2_hashmap_size, enc._interp_code, mn, ext)


@lru_cache(maxsize=None)
def _ref(interp):
    """float64 (sigma, grad, keep mask) and the float32 CPU restatement's gradient, on the CPU."""
    m, x = _expert(interp), _points().cpu()
    sig, grad, pre = N.sigma_grad(x, *_ref_args(m), dtype=torch.float64)
    _, g32, _ = N.sigma_grad(x, *_ref_args(m), dtype=torch.float32)
    keep = ~(pre.abs() < 1e-5).any(-1)
    return sig, grad, keep, g32.double()


def _err(got, ref, keep):
    """max|got - ref| over the kept samples, relative to max(1, max|ref|)."""
    return float((got.double().cpu() - ref)[keep].abs().max()) / max(1.0, float(ref[keep].abs().max()))


def _chain(m, x, precision, params=None):
    """The parent's four launches for (sigma, grad sigma): the route the fused kernel replaces."""
    ops = _ops()
    enc = m.xyz_encoder
    mn = m.scene_box.min.to(x.device)
    ext = m.aabb_extent.to(x.device)
    lo = m.enc_eps
    hi = 1.0 - m.enc_eps
    u = (x - mn) / ext
    x01 = u.clamp(lo, hi)
    h0 = ops.hashgrid_fwd(x01, enc.hash_table, enc._res_host, enc.log2_hashmap_size, 2, enc._interp_code)
    sh = torch.zeros(x.shape[0], 16, device=x.device)
    ws = [t.detach().contiguous() for t in m._mlp_tensors(params).values()]
    out, _ = ops.mlp_train_fwd(h0, sh, ws, save=False, precision=precision)
    gout = torch.zeros_like(out)
    gout[:, 3] = 1.0
    gh, _ = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, want_sh=False, precision=precision)
    gx01 = ops.hashgrid_bwd_input(x01, gh, enc.hash_table, enc._res_host, enc.log2_hashmap_size, 2, enc._interp_code)
    passed = ((u >= lo) & (u <= hi)).float()
    return out[:, 3].contiguous(), gx01 * (passed / ext)


@lru_cache(maxsize=None)
def _full(interp, precision):
    return _ops().field_sigma_grad(_points(), _expert(interp).expert_spec(), precision=precision)


# ------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("interp", INTERPS)
def test_values_against_the_float64_restatement(interp, precision):
    m, x = _expert(interp), _points()
    sig64, g64, keep, g32 = _ref(interp)
    excluded = int((~keep).sum())
    assert excluded <= 5, excluded                       # at most 1 % of the 500 samples sit on a kink
    sig, grad = _full(interp, precision)
    assert sig.shape == (500,) and grad.shape == (500, 3) and sig.dtype == grad.dtype == torch.float32
    es = float(((sig.double().cpu() - sig64).abs() / sig64.abs().clamp_min(1.0)).max())
    eg = _err(grad, g64, keep)
    e32 = _err(g32, g64, keep)
    csig, cgrad = _chain(m, x, precision)
    e_chain = _err(cgrad, g64, keep)
    tol = max(2e-5, 4 * (e32 if precision == "fp32" else e_chain))
    print(f"{interp} {precision}: sigma err {es:.3e}; grad err {eg:.3e} (e32 {e32:.3e}, e_chain {e_chain:.3e}, tol "
          f"{tol:.3e}), max|ref| {float(g64[keep].abs().max()):.3e}, excluded {excluded}, clamped coordinates "
          f"{int((g64 == 0).sum())}")
    assert es <= 1e-5
    assert eg <= tol
    # clamped coordinates (outside the box) have exactly no derivative
    out = ((x < -1.0) | (x > 1.0)).cpu()
    assert bool(out.any()) and bool((grad.cpu()[out] == 0).all())
    # the kernel keeps the chain's layer products and its summation order: the same bits
    assert torch.equal(sig, csig)
    assert torch.equal(grad, cgrad)


@pytest.mark.parametrize("interp", INTERPS)
def test_one_million_points_repeat_and_equal_the_chain(interp):
    """The size at which a gather pass with too many loads in flight showed: with all 64 gathers of
    a pass issued at once, ~8 of the 32768 tiles of a call came back with wrong gradients in rows 16..31, different
    from run to run (Linear, fp16x3, log2T = 20).  500 points have no chance of meeting a 2e-4-per-tile event."""
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    ops = _ops()
    torch.manual_seed(11)
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=dict(HASH_CONF, interpolation=interp, log2_hashmap_size=20),
                dir_encoding="spherical").to(DEV).eval().requires_grad_(False)
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    x = torch.rand(1 << 20, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)) * 2.0 - 1.0
    spec = m.expert_spec()
    s1, g1 = ops.field_sigma_grad(x, spec)
    s2, g2 = ops.field_sigma_grad(x, spec)
    cs, cg = _chain(m, x, None)
    bad_rr = int(((g1 != g2).any(-1) | (s1 != s2)).sum())
    bad_ch = int(((g1 != cg).any(-1) | (s1 != cs)).sum())
    print(f"{interp}: rows differing run to run {bad_rr}, from the chain {bad_ch}")
    assert bad_rr == 0 and bad_ch == 0
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0


# ------------------------------------------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("interp", INTERPS)
def test_prefixes_strides_repeats_and_a_nan_row(interp):
    ops = _ops()
    spec, x = _expert(interp).expert_spec(), _points()
    sig, grad = _full(interp, "fp16x3")
    for M in (1, 31, 32, 33, 65):
        s, g = ops.field_sigma_grad(x[:M], spec)
        assert torch.equal(s, sig[:M]) and torch.equal(g, grad[:M]), M
        s2, g2 = ops.field_sigma_grad(x[:M], spec)
        assert torch.equal(s2, s) and torch.equal(g2, g), M
        wide = torch.cat([x[:M], torch.full((M, 3), 7.0, device=DEV)], -1)      # ld = 6
        s6, g6 = ops.field_sigma_grad(wide, spec)
        assert torch.equal(s6, s) and torch.equal(g6, g), M
        xn = x[:M].clone()
        xn[M // 2, 1] = float("nan")
        sn, gn = ops.field_sigma_grad(xn, spec)
        others = torch.arange(M, device=DEV) != M // 2
        assert torch.equal(sn[others], s[others]) and torch.equal(gn[others], g[others]), M
    s0, g0 = ops.field_sigma_grad(x[:0], spec)
    assert s0.shape == (0,) and g0.shape == (0, 3)


# ------------------------------------------------------------------------------------------------- 3. gate
@pytest.mark.parametrize("interp", INTERPS)
def test_gate(interp):
    ops = _ops()
    spec, x = _expert(interp).expert_spec(), _points()
    sig, grad = _full(interp, "fp16x3")
    idx = torch.arange(500, device=DEV)
    patterns = {"tiles 0 and 2": (idx < 32) | ((idx >= 64) & (idx < 96)), "one sample": idx == 40,
                "nothing": torch.zeros(500, dtype=torch.bool, device=DEV)}
    for name, off in patterns.items():
        gate = torch.where(off, torch.full((500,), 1e-3, device=DEV), torch.full((500,), 0.5, device=DEV))
        s, g = ops.field_sigma_grad(x, spec, gate=gate, gate_min=1e-3)
        assert bool((s[off] == 0).all()) and bool((g[off] == 0).all()), name
        assert torch.equal(s[~off], sig[~off]) and torch.equal(g[~off], grad[~off]), name
    # the gate is "<=": at gate_min = 0 a zero weight is gated, a positive one is not
    gate = torch.where(idx % 2 == 0, torch.zeros(500, device=DEV), torch.full((500,), 1e-30, device=DEV))
    s, g = ops.field_sigma_grad(x, spec, gate=gate)
    assert bool((s[::2] == 0).all()) and torch.equal(s[1::2], sig[1::2]) and torch.equal(g[1::2], grad[1::2])


# ------------------------------------------------------------------------------------------------- 4. modules
def test_module_sigma_gradient_with_fast_weights_and_on_the_cpu():
    m, x = _expert("Linear"), _points()
    gen = torch.Generator().manual_seed(21)
    params = {k: (v.detach().cpu() * (1.0 + 0.1 * torch.randn(v.shape, generator=gen))).to(DEV)
              for k, v in m._mlp_tensors(None).items()}
    sig, grad = m.sigma_gradient(x, params)
    assert sig.shape == (500, 1) and grad.shape == (500, 3) and not sig.requires_grad and not grad.requires_grad
    sig64, g64, pre = N.sigma_grad(x.cpu(), *_ref_args(m, params), dtype=torch.float64)
    keep = ~(pre.abs() < 1e-5).any(-1)
    assert int((~keep).sum()) <= 10
    _, cgrad = _chain(m, x, None, params)
    tol = max(2e-5, 4 * _err(cgrad, g64, keep))
    print(f"fast weights: grad err {_err(grad, g64, keep):.3e} (tol {tol:.3e})")
    assert float(((sig[:, 0].double().cpu() - sig64).abs() / sig64.abs().clamp_min(1.0)).max()) <= 1e-5
    assert _err(grad, g64, keep) <= tol
    assert not torch.equal(sig, m.sigma_gradient(x)[0])          # the fast weights were used
    # leading dimensions and the gate pass through
    s3, g3 = m.sigma_gradient(x.view(5, 100, 3), gate=torch.ones(5, 100, device=DEV))
    assert s3.shape == (5, 100, 1) and g3.shape == (5, 100, 3) and torch.equal(g3.view(-1, 3), m.sigma_gradient(x)[1])
    # the fp32 parameter table, whatever the render table is
    m2 = _expert.__wrapped__("Linear")                           # a second, identical model (same seeds)
    m2.set_render_table_dtype(torch.float16)
    assert torch.equal(m2.sigma_gradient(x)[1], m.sigma_gradient(x)[1])
    # a CPU copy (the encoders as their torch restatements: the HIP ones have no CPU form) takes the autograd route
    mc = _expert.__wrapped__("Linear").cpu()
    enc = mc.xyz_encoder
    enc.forward = lambda p: R.hashgrid(p, enc.hash_table, enc._res_host, enc.log2_hashmap_size, enc._interp_code,
                                       dtype=torch.float32, weights="fp32")
    xc = x.cpu()
    sc, gc = mc.sigma_gradient(xc)
    sd, gd = mc.density_and_gradient(xc, create_graph=False)
    assert torch.equal(sc, sd) and torch.equal(gc, gd) and float(gc.abs().max()) > 0
    gate = torch.rand(500, generator=gen)
    sg, gg = mc.sigma_gradient(xc, gate=gate, gate_min=0.5)
    assert bool((gg[gate <= 0.5] == 0).all()) and torch.equal(gg[gate > 0.5], gd[gate > 0.5])


def _container_chain(m, pts, active_module=None):
    """MetaContainer.sigma_gradient's composition with every expert through the four-launch chain."""
    if active_module is not None:
        return _chain(m.submodules[active_module], pts, None)
    W, hard = m._routing(pts)
    sig = torch.zeros(pts.shape[0], device=DEV)
    grad = torch.zeros(pts.shape[0], 3, device=DEV)
    sig_k = torch.zeros(pts.shape[0], len(m.submodules), device=DEV)
    for k, sub in enumerate(m.submodules):
        sel = ((W[:, k] > 0) if W is not None else (hard == k)).nonzero().squeeze(1)
        if sel.numel() == 0:
            continue
        s, g = _chain(sub, pts[sel], None)
        wk = W[sel, k] if W is not None else torch.ones_like(s)
        sig.index_add_(0, sel, s * wk)
        grad.index_add_(0, sel, g * wk[:, None])
        sig_k[sel, k] = s
    if W is not None:
        x = pts.clone().requires_grad_()
        (gw,) = torch.autograd.grad((m._soft_weights(x, W > 0) * sig_k).sum(), x)
        grad = grad + gw
    return sig, grad


@pytest.mark.parametrize("case", ["hard", "soft", "active"])
def test_container_sigma_gradient_vs_autograd_through_density(case):
    from test_input_grad_gpu import _container, _container_points
    m, gbox = _container("k4", bm=1.0 if case == "hard" else 1.05)
    am = 1 if case == "active" else None
    pts = _container_points(m, gbox, 400, seed=36)
    x = pts.clone().requires_grad_()
    ref_sig = m.density(x, active_module=am)
    assert ref_sig.grad_fn is not None
    (ref_grad,) = torch.autograd.grad(ref_sig.sum(), x)
    sig, grad = m.sigma_gradient(pts, active_module=am)
    assert sig.shape == (400,) and grad.shape == (400, 3) and not grad.requires_grad
    # samples where a live expert's float64 reference sits within 1e-5 of a ReLU kink are set aside: at most 1 % per
    # expert evaluated, and a point near a bisector is evaluated by the (at most 3) experts within the margin
    W, hard = m._routing(pts)
    keep = torch.ones(400, dtype=torch.bool)
    for k, sub in enumerate(m.submodules):
        live = (torch.full((400,), k == am) if am is not None else ((W[:, k] > 0) if W is not None else (hard == k)).cpu())
        _, _, pre = N.sigma_grad(pts.cpu(), *_ref_args(sub), dtype=torch.float64)
        keep &= ~(live & (pre.abs() < 1e-5).any(-1))
    assert int((~keep).sum()) <= 12, int((~keep).sum())
    ref_sig, ref_grad = ref_sig.detach().double().cpu(), ref_grad.double().cpu()
    csig, cgrad = _container_chain(m, pts, am)
    e_chain = _err(cgrad, ref_grad, keep)
    tol = max(2e-5, 4 * e_chain)
    eg = _err(grad, ref_grad, keep)
    es = float(((sig.double().cpu() - ref_sig).abs() / ref_sig.abs().clamp_min(1.0)).max())
    print(f"{case}: sigma err {es:.3e}; grad err {eg:.3e} (e_chain {e_chain:.3e}, tol {tol:.3e}), max|ref| "
          f"{float(ref_grad[keep].abs().max()):.3e}, excluded {int((~keep).sum())}")
    assert es <= 1e-5 and eg <= tol and float(ref_grad.abs().max()) > 0
    if case == "soft":
        assert int(((W > 0).sum(-1) > 1).sum()) > 50          # the blend and its weight gradient are exercised


# ------------------------------------------------------------------------------------------------- 5. normal maps
def test_normal_composite_against_float64():
    gen = torch.Generator().manual_seed(8)
    w = torch.rand(48, 40, generator=gen)
    g = torch.randn(48 * 40, 3, generator=gen) * torch.logspace(-6, 3, 48 * 40).unsqueeze(-1)
    zero = torch.rand(48 * 40, generator=gen) < 0.2
    g[zero] = 0.0
    got = _ops().normal_composite(g.to(DEV), w.to(DEV))
    assert got.shape == (48, 3) and got.dtype == torch.float32
    ref = N.normal_composite(g, w, torch.float64)
    # <= 8 fp32 roundings per term at 2^-24 each, a float64 sum and one final rounding
    bound = 1e-6 * w.double().sum(1, keepdim=True) + 1e-12
    err = (got.double().cpu() - ref).abs()
    print(f"normal_composite: max err / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(_ops().normal_composite(g.view(48, 40, 3).to(DEV), w.to(DEV)), got)
    # zero gradients add exactly nothing
    w0 = w.clone()
    w0.view(-1)[zero] = 0.0
    assert torch.equal(_ops().normal_composite(g.to(DEV), w0.to(DEV)), got)


def _rays(n, seed):
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 2.5]) + 0.2 * torch.randn(n, 3, generator=gen)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.25 * torch.randn(n, 3, generator=gen), dim=-1)
    nf = torch.tensor([[1.0, 4.0]]).expand(n, 2)
    return torch.cat([o, d, nf], -1).to(DEV)


def test_render_normals():
    from adaptive_city_nerf_amd import render_normals, render_rays_stratified, stratified_t_vals
    from adaptive_city_nerf_amd._lib import AcnError
    ops = _ops()
    m = _expert("Linear")
    S, rays = 40, _rays(48, 9)                                   # S is no multiple of 32: tiles straddle rays
    rgb, depth, w, acc = render_rays_stratified(m, rays, S)
    raw, rgb_n, depth_n, acc_n = render_normals(m, rays, S, normalize=False)
    assert raw.shape == (48, 3)
    assert torch.equal(rgb_n, rgb) and torch.equal(depth_n, depth) and torch.equal(acc_n, acc)
    t = stratified_t_vals(rays[:, 6], rays[:, 7], S, randomized=False)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * t.unsqueeze(-1)).reshape(-1, 3)
    _, g = m.sigma_gradient(pts)
    assert float(g.abs().max()) > 0 and float(w.max()) > 1e-3
    assert torch.equal(raw, ops.normal_composite(g, w))
    n1, *_ = render_normals(m, rays, S)
    assert torch.equal(n1, torch.nn.functional.normalize(raw, dim=-1))
    # chunks of rays give the rows of the whole batch
    assert torch.equal(render_normals(m, rays, S, normalize=False, chunk_rays=20)[0], raw)
    # dropping the samples with w <= 1e-3: each dropped unit-normal term has norm <= its weight.  A denser field (fast
    # weights with the sigma head's bias raised) so that the transmittance does fall under 1e-3 along the rays
    dense = dict(m._mlp_tensors(None))
    dense["sigma_head.bias"] = dense["sigma_head.bias"] + 4.0
    wd = render_rays_stratified(m, rays, S, params=dense)[2]
    full, *_ = render_normals(m, rays, S, params=dense, normalize=False)
    cut, *_ = render_normals(m, rays, S, params=dense, min_weight=1e-3, normalize=False)
    dropped = int((wd <= 1e-3).sum())
    print(f"render_normals: {dropped} of {wd.numel()} samples gated, max|cut - full| = "
          f"{float((cut - full).abs().max()):.3e}")
    assert dropped > 32 and float((cut - full).abs().max()) <= 1e-3 * S
    assert not torch.equal(cut, full)
    # a ray that meets nothing keeps a zero normal through the normalisation
    z = torch.nn.functional.normalize(torch.zeros(2, 3, device=DEV), dim=-1)
    assert bool((z == 0).all())
    m.train()
    try:
        with pytest.raises(AcnError, match="training"):
            render_normals(m, rays, S)
    finally:
        m.eval()


def test_render_normal_image():
    from adaptive_city_nerf_amd import render_normal_image, render_normals
    ops = _ops()
    m = _expert("Smoothstep")
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.1], [0.0, 0.0, 1.0, 2.6]])
    kw = dict(H=12, W=16, fx=14.0, fy=14.0, cx=8.0, cy=6.0, c2w=c2w, scene_box=m.scene_box)
    normal, rgb, depth, acc = render_normal_image(m, ray_samples=24, **kw)
    assert normal.shape == (12, 16, 3) and rgb.shape == (12, 16, 3) and depth.shape == (192,) and acc.shape == (192,)
    rays, _ = ops.get_rays_image(12, 16, 14.0, 14.0, 8.0, 6.0, c2w, m.scene_box.aabb, DEV, center_pixels=True,
                                 near_far_override=(None, None), apply_clamp=True)
    n, r, d, a = render_normals(m, rays, 24)
    assert torch.equal(normal.view(-1, 3), n) and torch.equal(rgb.view(-1, 3), r.clamp(0, 1))
    assert torch.equal(depth, d) and torch.equal(acc, a)
    assert float(acc.max()) > 0 and float(normal.abs().max()) > 0
    assert bool(((normal.norm(dim=-1) - 1).abs() < 1e-5).logical_or(normal.norm(dim=-1) == 0).all())
