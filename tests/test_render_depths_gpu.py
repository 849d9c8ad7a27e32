"""The fused render at caller-supplied depths on the GPU (acn_render_depths_fwd): ops.render_depths,
render_rays_at and the fine pass of render_rays_hierarchical.

At the depths the stratified render computes for itself the new kernels must return its bits (the depths are then the
same fp32 numbers, and everything after them is the same instruction sequence); at depths no kernel would generate
they are compared with the composed chain -- points, model forward, background, volume_render -- under the project's
parity tolerances (rgb, acc 1e-4; weights 1e-5; depth 1e-4 * max|t|)."""
from functools import lru_cache

import pytest
import torch

import sample_pdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 2), (37, 31), (37, 33), (16, 65)]   # tile tails on both sides of 32, a lone ray, a partial workgroup,
#                                                   a last ray whose last sample is the tensor's last float


@lru_cache(maxsize=None)
def _model(K, interp="Linear"):
    """Shared between the tests, never modified."""
    import test_f16_table_gpu as T16
    return T16._build(K, interp).eval().requires_grad_(False)


def _rays(m, n, seed):
    import test_f16_table_gpu as T16
    return T16._rays(m, n, seed)


def _points(rays, t):
    N, M = t.shape
    return torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * t[..., None],
                      rays[:, None, 3:6].expand(N, M, 3)], -1).reshape(-1, 6)


def _fused_args(m, active, N):
    """(specs, routing, active_module, background, packed) of the raw ops for this model, as the renderers pass them."""
    from adaptive_city_nerf_amd import ray_rendering as RR
    specs, routing, packed = RR._fused_experts(m, None, active)
    bg, keep = RR._fused_background(m, "white", N, torch.device(DEV))
    return specs, routing, (0 if len(specs) == 1 else None), bg, packed, keep


def _chain(m, rays, t, active=None, sigma_scale=1.0):
    """_points -> model -> _get_bg_rgb -> volume_render (test_resample_gpu._hand_composed's fine pass)."""
    from adaptive_city_nerf_amd import volume_render
    from adaptive_city_nerf_amd.ray_rendering import _get_bg_rgb
    N, S = t.shape
    eff = m.submodules[active] if active is not None else m
    rgb_sigma = eff(_points(rays, t), params=None).view(N, S, 4)
    bg = _get_bg_rgb(m, rays[:, 3:6], None, rgb_sigma, N=N, bg_color_default="white")
    return volume_render(rgb_sigma, t, bg_rgb=bg, sigma_scale=sigma_scale)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _diffs(got, ref):
    return [float((a - b).abs().max()) for a, b in zip(got, ref)]   # rgb, depth, weights, acc


# ------------------------------------------------------------------- 1. the stratified render's own depths: same bits
CONFIGS = [(1, "Linear", None), (1, "Smoothstep", None), (1, "Nearest", None), (2, "Linear", None),
           (2, "Smoothstep", None), (2, "Linear", 0), (2, "Smoothstep", 0), (4, "Linear", None),
           (4, "Smoothstep", None)]


@pytest.mark.parametrize("K,interp,active", CONFIGS)
def test_same_bits_as_the_stratified_render(K, interp, active):
    from adaptive_city_nerf_amd import ops, stratified_t_vals
    m = _model(K, interp)
    for N, S in SHAPES:
        rays = _rays(m, N, 100 + S)
        specs, routing, am, bg, packed, keep = _fused_args(m, active, N)
        jitter = torch.rand(N, S, generator=torch.Generator().manual_seed(S)).to(DEV)
        for jit in (None, jitter):
            t = stratified_t_vals(rays[:, 6], rays[:, 7], S, randomized=jit is not None, u=jit)
            for tau in (0.0, 1e-5):
                with torch.no_grad():
                    ref = ops.render_stratified(rays, S, specs, routing, am, bg, tau=tau, jitter=jit, packed=packed)
                    got = ops.render_depths(rays, t, specs, routing, am, bg, tau=tau, packed=packed)
                if not _same(got, ref):   # which depths differ from the kernels' own, before failing
                    sub = m.submodules[active or 0] if K > 1 else m
                    mn, ext = sub._host_box()
                    tk = ops.sample_stratified(rays, S, jit, mn, ext, 1e-6)[0]
                    bad = (tk != t).nonzero().tolist()
                    print(f"K={K} {interp} active={active} N={N} S={S} jitter={jit is not None} tau={tau}: "
                          f"diffs {_diffs(got, ref)}; torch t differs from the sampler kernel's at {bad[:16]}")
                assert _same(got, ref), (K, interp, active, N, S, jit is not None, tau)


# ------------------------------------------------------------- 2. depths no kernel generates, against the composed chain
def _merged_rows(rays, offset):
    """(N, 32) merged rows: the 16-sample near..far linspace of each ray and 16 fine depths resampled from
    sample_pdf_ref's weights (its special rows: all-zero weights, one opaque sample), row 2 with near == far (every
    depth equal: dist == 0 throughout); t offset by ``offset`` with the origins moved back along the directions, so
    that the points stay where they were."""
    N = rays.shape[0]
    c = R.case(N, 16, 16, 0.0)
    lin = torch.linspace(0.0, 1.0, 16)
    near, far = rays[:, 6:7].cpu(), rays[:, 7:8].cpu()
    t_c = (near * (1.0 - lin) + far * lin).float()
    t_c[2] = near[2]
    t_f = torch.from_numpy(R.resample(c["w"].numpy(), t_c.numpy(), 16))
    t_f[:, 5] = t_c[:, 7]                      # a fine depth equal to a coarse one in every row
    tm = torch.sort(torch.cat([t_c, t_f], 1), 1).values
    assert bool((tm[:, 1:] == tm[:, :-1]).any(1).all()) and bool((tm[2] == tm[2, 0]).all())
    r = rays.clone()
    r[:, :3] -= offset * r[:, 3:6]
    return r, (tm + offset).to(DEV)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_against_the_composed_chain(K):
    from adaptive_city_nerf_amd import ops
    m = _model(K)
    N = 64
    specs, routing, am, bg, packed, keep = _fused_args(m, None, N)
    base = _rays(m, N, 31)
    for offset in (0.0, 100.0):
        rays, t = _merged_rows(base, offset)
        with torch.no_grad():
            ref = _chain(m, rays, t)
            got = ops.render_depths(rays, t, specs, routing, am, bg, packed=packed)
        tmax = float(t.abs().max())
        d = _diffs(got, ref)
        print(f"K={K}, t offset {offset}: rgb {d[0]:.2e}, depth / max|t| {d[1] / tmax:.2e}, weights {d[2]:.2e}, "
              f"acc {d[3]:.2e}")
        assert float(got[3].max()) > 0            # the rays hit something: the comparison is not of empty renders
        assert d[0] <= 1e-4 and d[3] <= 1e-4 and d[2] <= 1e-5 and d[1] <= 1e-4 * tmax
    # for orientation only: the stratified render against the same chain at its own linspace depths
    from adaptive_city_nerf_amd import stratified_t_vals
    with torch.no_grad():
        tl = stratified_t_vals(base[:, 6], base[:, 7], 32, randomized=False)
        d = _diffs(ops.render_stratified(base, 32, specs, routing, am, bg, packed=packed), _chain(m, base, tl))
    print(f"K={K}, render_stratified at the 32-sample linspace: rgb {d[0]:.2e}, depth / max|t| "
          f"{d[1] / float(tl.abs().max()):.2e}, weights {d[2]:.2e}, acc {d[3]:.2e}")


# --------------------------------------------------------------------------------- 3. early termination and the weights
def _saturating_rows(rays, S=128):
    """Rows of four kinds (ray n: n % 4): every sample 0.05 apart from the near plane (opaque inside the first tile under
    the test's sigma_scale), the first 32 / the first 64 samples 1e-4 apart (thin) and 0.05 from there on (the ray
    saturates in the second / third tile), every sample 1e-4 apart (the ray never saturates)."""
    N = rays.shape[0]
    thin = torch.tensor([0, 32, 64, S])[torch.arange(N) % 4]
    step = torch.where(torch.arange(S)[None, :] < thin[:, None], 1e-4, 0.05)
    t = 1.0 + torch.cumsum(step, 1) - step
    return t.float().to(DEV), thin


@pytest.mark.parametrize("K", [1, 4])
def test_early_termination_and_weights(K):
    from adaptive_city_nerf_amd import ops
    m = _model(K)
    N, S, tau, scale = 64, 128, 1e-3, 200.0
    rays = _rays(m, N, 41)
    t, thin = _saturating_rows(rays, S)
    specs, routing, am, bg, packed, keep = _fused_args(m, None, N)
    with torch.no_grad():
        full = ops.render_depths(rays, t, specs, routing, am, bg, sigma_scale=scale, packed=packed)
        cut = ops.render_depths(rays, t, specs, routing, am, bg, sigma_scale=scale, tau=tau, packed=packed)
        bare = ops.render_depths(rays, t, specs, routing, am, bg, sigma_scale=scale, tau=tau, packed=packed,
                                 want_weights=False)
    assert bare[2] is None and all(torch.equal(bare[i], cut[i]) for i in (0, 1, 3))
    # the transmittance behind each 32-sample tile, from the weights of the full render (T = 1 - sum w up to fp32
    # rounding: a tile is counted as below / above tau only when it is so by a factor of 2)
    T = 1.0 - full[2].double().cumsum(1)[:, 31::32]                       # (N, 4)
    below, above = T < 0.5 * tau, T > 2.0 * tau
    clear = (below | above).all(1)
    first = torch.where(below.any(1), below.int().argmax(1), torch.full((N,), 4, device=DEV))   # first tile below tau
    assert int(clear.sum()) >= N // 2
    stops = {k: int(((first == k) & clear).sum()) for k in range(5)}
    print(f"K={K}: rays by the tile behind which they stop (4 = never): {stops}; "
          f"largest T at a stop {float(T[below].max()) if bool(below.any()) else 0.0:.2e}")
    assert stops[0] > 0 and stops[1] + stops[2] > 0 and stops[4] > 0
    s = torch.arange(S, device=DEV)[None, :]
    after = (s >= 32 * (first[:, None] + 1)) & clear[:, None]
    assert int(after.sum()) > 0 and bool((cut[2][after] == 0).all())      # exactly zero behind the stop
    assert torch.equal(cut[2][~after & clear[:, None]], full[2][~after & clear[:, None]])   # untouched before it
    never = clear & (first == 4)
    assert _same([x[never] for x in cut], [x[never] for x in full])
    d = _diffs(cut, full)
    tmax = float(t.abs().max())
    print(f"K={K}, tau {tau} against tau 0: rgb {d[0]:.2e}, depth / max|t| {d[1] / tmax:.2e}, weights {d[2]:.2e}, "
          f"acc {d[3]:.2e}")
    assert d[0] <= 1e-4 and d[3] <= 1e-4 and d[2] <= 1e-5 and d[1] <= 1e-4 * tmax


# -------------------------------------------------------------------------------------------------- 4. row isolation
@pytest.mark.parametrize("K", [1, 2, 4])
def test_rows_are_isolated_and_calls_repeat(K):
    from adaptive_city_nerf_amd import ops
    m = _model(K)
    N, S = 37, 33
    rays = _rays(m, N, 51)
    _, t = _merged_rows(_rays(m, N, 52), 0.0)
    t = torch.cat([t, t[:, -1:] + 0.01], 1)            # S = 33: a one-sample tail tile
    specs, routing, am, bg, packed, keep = _fused_args(m, None, N)
    for tau in (0.0, 1e-3):
        with torch.no_grad():
            a = ops.render_depths(rays, t, specs, routing, am, bg, tau=tau, packed=packed, reorder=True)
            b = ops.render_depths(rays, t, specs, routing, am, bg, tau=tau, packed=packed, reorder=True)
            c = ops.render_depths(rays, t, specs, routing, am, bg, tau=tau, packed=packed, reorder=False)
            t2 = t.clone()
            t2[5] = float("nan")
            t2[N - 1] = t[N - 1].flip(0)                   # descending, in the tensor's last row
            t2[0, 7] = float("inf")
            x = ops.render_depths(rays, t2, specs, routing, am, bg, tau=tau, packed=packed)
        torch.cuda.synchronize()
        assert _same(a, b) and _same(a, c)
        keep_rows = torch.ones(N, dtype=torch.bool, device=DEV)
        keep_rows[[0, 5, N - 1]] = False
        assert _same([v[keep_rows] for v in x], [v[keep_rows] for v in a])
        assert bool(torch.isfinite(a[0]).all()) and float(a[3].max()) > 0


# ---------------------------------------------------------------------------------------------------- 5. public path
@pytest.mark.parametrize("K", [1, 2])
def test_render_rays_at(K):
    from adaptive_city_nerf_amd import ops, render_rays_at
    m = _model(K)
    N = 64
    rays, t = _merged_rows(_rays(m, N, 61), 0.0)
    for active in ((None,) if K == 1 else (None, 0)):
        specs, routing, am, bg, packed, keep = _fused_args(m, active, N)
        with torch.no_grad():
            raw = ops.render_depths(rays, t, specs, routing, am, bg, packed=packed)
            pub = render_rays_at(m, rays, t, active_module=active)
            assert len(pub) == 4 and _same(pub, raw)
            cut = render_rays_at(m, rays, t, active_module=active, sigma_scale=3.0, early_stop_tau=1e-3)
            assert _same(cut, ops.render_depths(rays, t, specs, routing, am, bg, sigma_scale=3.0, tau=1e-3,
                                                packed=packed))
            # depths of another dtype: the chain
            assert _same(render_rays_at(m, rays, t.double(), active_module=active),
                         _chain(m, rays, t.double(), active))
        # rays that require grad: the chain, bit for bit, and a gradient
        rg = rays.clone().requires_grad_(True)
        out = render_rays_at(m, rg, t, active_module=active)
        ref = _chain(m, rays.clone().requires_grad_(True), t, active)
        assert _same([o.detach() for o in out], [r.detach() for r in ref])
        (out[0].sum() + out[1].sum()).backward()
        assert bool(torch.isfinite(rg.grad).all()) and float(rg.grad[:, :6].abs().max()) > 0


def test_render_rays_at_takes_the_chain_for_fp16_render_tables():
    import test_f16_table_gpu as T16
    from adaptive_city_nerf_amd import ops, ray_rendering as RR, render_rays_at
    from adaptive_city_nerf_amd._lib import AcnError
    m = T16._build(1).eval().requires_grad_(False)      # a model of its own: its table mode is changed
    N = 64
    rays, t = _merged_rows(_rays(m, N, 62), 0.0)
    with torch.no_grad():
        fused = render_rays_at(m, rays, t)
        m.set_render_table_dtype(torch.float16)
        assert RR._fused_depths(m, rays, t, None, None, "white") is None
        out = render_rays_at(m, rays, t)
        assert _same(out, _chain(m, rays, t))
        assert not _same(out, fused)              # the fp16 table's values, not the fp32 parameter's
        specs, routing, packed = RR._fused_experts(m, None, None, render_table=True)
        bg, keep = RR._fused_background(m, "white", N, rays.device)
        with pytest.raises(AcnError, match="fp16"):
            ops.render_depths(rays, t, specs, routing, 0, bg, packed=packed)


@pytest.mark.parametrize("config", ["expert", "k2", "k2_a0", "k4"])
def test_hierarchical_fine_pass(config):
    from adaptive_city_nerf_amd import ray_rendering as RR
    from adaptive_city_nerf_amd import render_rays, render_rays_at, render_rays_hierarchical, sample_pdf
    m = _model({"expert": 1, "k2": 2, "k2_a0": 2, "k4": 4}[config])
    active = 0 if config == "k2_a0" else None
    N, S, F = 64, 16, 16
    rays = _rays(m, N, 71)
    prev = RR.FUSED_FINE_RENDER
    try:
        with torch.no_grad():
            RR.FUSED_FINE_RENDER = True
            on = render_rays_hierarchical(m, rays, S, F, active_module=active, return_coarse=True, return_t_vals=True,
                                          early_stop_tau=1e-3)
            assert len(on) == 6 and on[2].shape == (N, S + F)
            at = render_rays_at(m, rays, on[5], active_module=active)    # early_stop_tau: the coarse pass only
            assert _same(on[:4], at)
            via = render_rays(m, rays, ray_samples=S, n_importance=F, active_module=active, early_stop_tau=1e-3)
            assert _same(via, at)
            RR.FUSED_FINE_RENDER = False
            off = render_rays_hierarchical(m, rays, S, F, active_module=active, return_coarse=True, return_t_vals=True,
                                           early_stop_tau=1e-3)
            # the parent's fine pass: the resampling kernel's points, model forward, background, volume_render
            coarse = RR.render_rays_stratified(m, rays, S, active_module=active, return_t_vals=True,
                                               early_stop_tau=1e-3)
            _, tm, id6 = sample_pdf(coarse[4], coarse[2], F, rays=rays)
            eff = m.submodules[active] if active is not None else m
            rgb_sigma = eff(id6, params=None).view(N, S + F, 4)
            bgc = RR._get_bg_rgb(m, rays[:, 3:6], None, rgb_sigma, N=N, bg_color_default="white")
            ref = RR.volume_render(rgb_sigma, tm, bg_rgb=bgc)
    finally:
        RR.FUSED_FINE_RENDER = prev
    assert _same(off[:4], ref) and torch.equal(off[5], tm) and torch.equal(on[5], tm)
    assert _same(on[4], off[4]) and _same(on[4], coarse[:4])
    d = _diffs(on[:4], off[:4])
    far = float(rays[:, 7].max())
    print(f"{config}: fused fine pass against the chain: rgb {d[0]:.2e}, depth / far {d[1] / far:.2e}, weights "
          f"{d[2]:.2e}, acc {d[3]:.2e}")
    assert d[0] <= 1e-4 and d[1] <= 1e-4 * far and d[2] <= 1e-4 and d[3] <= 1e-4   # the eval-mode test's tolerances
    assert float(on[3].max()) > 0
    # a model in training mode under autograd keeps the chain (its parameters need the gradient)


# --------------------------------------------------------------------------------------------------------- 6. errors
def test_errors_and_empty_batches():
    from adaptive_city_nerf_amd import ops, render_rays_at
    from adaptive_city_nerf_amd._lib import AcnError
    m = _model(1)
    N, S = 8, 16
    rays = _rays(m, N, 81)
    t = torch.rand(N, S, device=DEV).sort(1).values + 1.0
    specs, routing, am, bg, packed, keep = _fused_args(m, None, N)
    for bad in (t[:, :1], torch.cat([t, t[:1]], 0), t[0]):
        with pytest.raises(AcnError, match="t_vals"):
            ops.render_depths(rays, bad, specs, routing, am, bg, packed=packed)
        with pytest.raises(AcnError, match="t_vals"):
            render_rays_at(m, rays, bad)
    with pytest.raises(AcnError, match="cpu"):
        ops.render_depths(rays, t.cpu(), specs, routing, am, bg, packed=packed)
    with pytest.raises(AcnError, match="cpu"):
        render_rays_at(m, rays, t.cpu())
    out = ops.render_depths(rays[:0], t[:0], specs, routing, am, bg, packed=packed)
    assert out[0].shape == (0, 3) and out[1].shape == (0,) and out[2].shape == (0, S) and out[3].shape == (0,)
    # non-contiguous and non-fp32 depths go through the fp32 copy
    wide = torch.zeros(N, 2 * S, device=DEV)
    wide[:, ::2] = t
    with torch.no_grad():
        ref = ops.render_depths(rays, t, specs, routing, am, bg, packed=packed)
        assert _same(ops.render_depths(rays, wide[:, ::2], specs, routing, am, bg, packed=packed), ref)
        assert _same(ops.render_depths(rays, t.double(), specs, routing, am, bg, packed=packed), ref)
