"""The fused importance resampling on the GPU (acn_resample_pdf) against the sequential float64
definition of tests/sample_pdf_ref.py, and its way up: sample_pdf, render_rays_hierarchical in eval and training mode,
render_rays / render_image / adapt_step with n_importance.

The kernel works in float64 and rounds each depth to fp32 once; its CDF is a wave scan, the reference's a front-to-back
sum, so for every finite row |t_fine - ref| <= 2 * 2^-24 * max|t_row| (sample_pdf_ref.BOUND: the result's own rounding
plus the one the summation order can flip).  The worst ratio to the bound is printed.  The merged row and the points
are exact functions of t_fine and are compared bit for bit."""
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import pytest
import torch

import sample_pdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(37, 3, 1), (37, 4, 7), (16, 5, 64), (16, 64, 64), (8, 65, 128), (8, 96, 33), (4, 256, 128), (2, 1024, 1024)]


@lru_cache(maxsize=None)
def _case(shape, offset):
    """CPU inputs and the float64 references (without and with jitter), computed once and never modified."""
    N, S, F = shape
    c = R.case(N, S, F, offset)
    refs = {False: torch.from_numpy(R.resample(c["w"].numpy(), c["t"].numpy(), F)),
            True: torch.from_numpy(R.resample(c["w"].numpy(), c["t"].numpy(), F, c["jitter"].numpy()))}
    g = torch.Generator().manual_seed(S + F)
    rays = torch.cat([torch.randn(N, 6, generator=g) * 3.0, c["t"][:, :1], c["t"][:, -1:]], 1)
    return c, refs, rays


def _ratio(got, ref, t, keep):
    tmax = t[keep].abs().amax(1, keepdim=True).double()
    return float(((got.cpu()[keep].double() - ref[keep].double()).abs() / (R.BOUND * tmax)).max())


def _points(rays, t):
    N, M = t.shape
    return torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * t[..., None],
                      rays[:, None, 3:6].expand(N, M, 3)], -1).reshape(-1, 6)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_definition(shape):
    from adaptive_city_nerf_amd import ops
    N, S, F = shape
    for offset in R.OFFSETS:
        c, refs, rays = _case(shape, offset)
        keep = R.finite_rows(c)
        rows = c["rows"]
        w, t, rd = c["w"].to(DEV), c["t"].to(DEV), rays.to(DEV)
        b = torch.from_numpy(R.edges(c["t"].numpy())).float()   # rounding is monotonic: fl(b_0) <= fl(x) <= fl(b_{S-2})
        for given in (False, True):
            jit = c["jitter"].to(DEV) if given else None
            t_fine, t_merged, pts = ops.resample_pdf(w, t, F, jitter=jit, rays=rd, want_points=True)
            torch.cuda.synchronize()
            r = _ratio(t_fine, refs[given], c["t"], keep)
            print(f"{shape}, t offset {offset}, jitter {'given' if given else 'none'}: t_fine at {r:.3f} of the bound")
            assert r <= 1
            tf = t_fine.cpu()
            assert bool((tf[keep, 1:] >= tf[keep, :-1]).all())
            assert bool((tf[keep] >= b[keep, :1]).all()) and bool((tf[keep] <= b[keep, -1:]).all())
            if "zero" in rows:     # every bin weighs the same: uniform over [b_0, b_{S-2}]
                z = rows["zero"]
                uni = torch.from_numpy(R.uniform_row(c["t"][z].numpy(), F, c["jitter"][z].numpy() if given else None))
                assert float((tf[z].double() - uni).abs().max()) <= R.BOUND * float(c["t"][z].abs().max())
            if "onehot" in rows:   # the opaque sample's bin takes all but the few quantiles of the 1e-5 padding
                o, m = rows["onehot"], R.onehot_index(S)
                inside = (tf[o] >= b[o, m - 1]) & (tf[o] <= b[o, m])
                assert int((~inside).sum()) <= R.onehot_outside_max(S, F)
            if "flat" in rows:     # near == far: every depth is that value, every comparison of the merge a tie
                f = rows["flat"]
                assert bool((tf[f] == c["t"][f, 0]).all())
            # the merge and the points: exact functions of the kernel's own t_fine (device torch ops)
            want = torch.sort(torch.cat([t, t_fine], 1), 1).values
            kd = keep.to(DEV)
            assert torch.equal(t_merged[kd], want[kd])
            assert torch.equal(pts.view(N, S + F, 6)[kd], _points(rd, t_merged).view(N, S + F, 6)[kd])
            # repeatable bit for bit, and the outputs do not depend on which optional ones are requested
            again = ops.resample_pdf(w, t, F, jitter=jit, rays=rd, want_points=True)
            bare = ops.resample_pdf(w, t, F, jitter=jit)
            assert bare[2] is None
            for a, bb in zip((t_fine, t_merged, pts, t_fine, t_merged), again + bare[:2]):
                assert torch.equal(a.view(N, -1)[kd], bb.view(N, -1)[kd])
            if "nan" in rows:      # the NaN row returns normally and changes no other row's bits
                n = rows["nan"]
                t2 = c["t"].clone()
                t2[n] = c["t"][N - 1]
                fin = ops.resample_pdf(w, t2.to(DEV), F, jitter=jit, rays=rd, want_points=True)
                assert bool(torch.isfinite(fin[0]).all()) and bool(torch.isfinite(fin[1]).all())
                assert torch.equal(fin[0][kd], t_fine[kd]) and torch.equal(fin[1][kd], t_merged[kd])
                assert torch.equal(fin[2].view(N, S + F, 6)[kd], pts.view(N, S + F, 6)[kd])


def test_sample_pdf_dispatch_and_oversized_rows():
    from adaptive_city_nerf_amd import ops, sample_pdf
    from adaptive_city_nerf_amd import ray_rendering as RR
    from adaptive_city_nerf_amd._lib import AcnError
    c, refs, rays = _case((8, 96, 33), 100.0)
    w, t, jit, rd = (x.to(DEV) for x in (c["w"], c["t"], c["jitter"], rays))
    keep = R.finite_rows(c)
    assert "nan" in c["rows"]
    kd = keep.to(DEV)

    def same(a, b):      # the finite rows (NaN != NaN)
        return torch.equal(a.view(8, -1)[kd], b.view(8, -1)[kd])

    k = ops.resample_pdf(w, t, 33, jitter=jit, rays=rd, want_points=True)
    assert same(sample_pdf(t, w, 33, jit), k[0])
    got = sample_pdf(t, w, 33, jit, return_merged=True)
    assert len(got) == 2 and same(got[0], k[0]) and same(got[1], k[1])
    got = sample_pdf(t, w, 33, jit, rays=rd)
    assert len(got) == 3 and same(got[0], k[0]) and same(got[1], k[1]) and same(got[2], k[2])
    assert not sample_pdf(t, w.clone().requires_grad_(True), 33).requires_grad
    prev = RR.FUSED_RESAMPLE
    RR.FUSED_RESAMPLE = False
    try:       # the torch chain on the device: the same definition
        tt = sample_pdf(t, w, 33, jit, rays=rd)
    finally:
        RR.FUSED_RESAMPLE = prev
    assert _ratio(tt[0], refs[True], c["t"], keep) <= 1
    # S = 1025 is past the kernel's rows: sample_pdf takes the torch chain, the raw op raises
    big = R.case(2, 1025, 16, 100.0)
    ref = torch.from_numpy(R.resample(big["w"].numpy(), big["t"].numpy(), 16, big["jitter"].numpy()))
    wb, tb, jb = (x.to(DEV) for x in (big["w"], big["t"], big["jitter"]))
    t_fine, t_merged = sample_pdf(tb, wb, 16, jb, return_merged=True)
    r = _ratio(t_fine, ref, big["t"], R.finite_rows(big))
    print(f"S = 1025 through the torch chain: t_fine at {r:.3f} of the bound")
    assert r <= 1 and t_merged.shape == (2, 1041)
    with pytest.raises(AcnError, match="1024"):
        ops.resample_pdf(wb, tb, 16, jitter=jb)
    with pytest.raises(AcnError, match="1024"):
        ops.resample_pdf(w, t, 1025)


# ------------------------------------------------------------------------------------------------ the renders
def _expert():
    import test_input_grad_gpu as T
    return T._expert()


def _k2():
    import test_f16_table_gpu as T16
    return T16._k2_container()


def _rays(m, n, seed):
    import test_f16_table_gpu as T16
    return T16._rays(m, n, seed)


def _fast_weights(m):
    g = torch.Generator().manual_seed(2)
    return OrderedDict((n, (p.detach().cpu() + 0.02 * torch.randn(p.shape, generator=g)).to(DEV))
                       for n, p in m.meta_named_parameters())


def _hand_composed(m, rays, S, F, params=None, active_module=None):
    """Coarse render, reference resampling, model forward, volume_render."""
    from adaptive_city_nerf_amd import render_rays_stratified, volume_render
    from adaptive_city_nerf_amd.ray_rendering import _get_bg_rgb
    N = rays.shape[0]
    coarse = render_rays_stratified(m, rays, S, params=params, active_module=active_module, return_t_vals=True)
    t_fine = torch.from_numpy(R.resample(coarse[2].cpu().numpy(), coarse[4].cpu().numpy(), F)).to(DEV)
    tm = torch.sort(torch.cat([coarse[4], t_fine], 1), 1).values
    eff = m.submodules[active_module] if active_module is not None else m
    rgb_sigma = eff(_points(rays, tm), params=params).view(N, S + F, 4)
    bg = _get_bg_rgb(m, rays[:, 3:6], params, rgb_sigma, N=N, bg_color_default="white")
    return volume_render(rgb_sigma, tm, bg_rgb=bg), coarse, tm


@pytest.mark.parametrize("config", ["expert", "expert_fast", "k2", "k2_a0"])
def test_hierarchical_render_in_eval_mode(config):
    from adaptive_city_nerf_amd import render_rays, render_rays_hierarchical
    N, S, F = 64, 16, 16
    if config.startswith("expert"):
        m = _expert().eval().requires_grad_(False)
        params = _fast_weights(m) if config == "expert_fast" else None
        active = None
    else:
        m, params = _k2(), None
        active = 0 if config == "k2_a0" else None
    rays = _rays(m, N, 21)
    far = float(rays[:, 7].max())
    with torch.no_grad():
        ref, coarse, tm = _hand_composed(m, rays, S, F, params=params, active_module=active)
        out = render_rays_hierarchical(m, rays, S, F, params=params, active_module=active, return_coarse=True,
                                       return_t_vals=True)
        plain = render_rays(m, rays, ray_samples=S, n_importance=F, params=params, active_module=active)
    assert len(out) == 6 and len(plain) == 4 and out[2].shape == (N, S + F)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], plain))
    assert all(torch.equal(a, b) for a, b in zip(out[4], coarse[:4]))
    assert float((out[5] - tm).abs().max()) <= R.BOUND * float(tm.abs().max())
    d_rgb, d_depth = float((out[0] - ref[0]).abs().max()), float((out[1] - ref[1]).abs().max())
    d_w, d_acc = float((out[2] - ref[2]).abs().max()), float((out[3] - ref[3]).abs().max())
    print(f"{config}: rgb {d_rgb:.2e}, depth / far {d_depth / far:.2e}, weights {d_w:.2e}, acc {d_acc:.2e}; the fine "
          f"pass moved the colour by {float((out[0] - coarse[0]).abs().max()):.2e}")
    assert d_rgb <= 1e-4 and d_depth <= 1e-4 * far and d_acc <= 1e-4 and d_w <= 1e-4
    assert float(out[3].max()) > 0            # the rays hit something: the comparison is not of empty renders


def test_hierarchical_render_in_training_mode():
    """Fine plus coarse colour plus the regulariser on the fine pass, backward; against the same chain with the
    resampling step as torch ops (FUSED_RESAMPLE off), within test_distortion_gpu's tolerance through the compositing
    (2e-5 of the largest reference gradient per tensor)."""
    from adaptive_city_nerf_amd import distortion_loss, render_rays_hierarchical
    from adaptive_city_nerf_amd import ray_rendering as RR
    m = _expert().train()
    N, S, F = 64, 16, 16
    rays = _rays(m, N, 22)
    g = torch.Generator().manual_seed(4)
    u, uf = torch.rand(N, S, generator=g).to(DEV), torch.rand(N, F, generator=g).to(DEV)

    def step(fused):
        prev = RR.FUSED_RESAMPLE
        RR.FUSED_RESAMPLE = fused
        try:
            m.zero_grad(set_to_none=True)
            rgb, depth, w, acc, coarse, tm = render_rays_hierarchical(m, rays, S, F, return_coarse=True,
                                                                      return_t_vals=True, jitter_u=u, jitter_fine=uf)
            assert rgb.requires_grad and coarse[0].requires_grad and not tm.requires_grad
            loss = ((rgb - 0.25) ** 2).mean() + ((coarse[0] - 0.25) ** 2).mean() + \
                0.05 * distortion_loss(w, tm, rays=rays)
            loss.backward()
        finally:
            RR.FUSED_RESAMPLE = prev
        return float(loss.detach()), OrderedDict((n, p.grad.detach().clone()) for n, p in m.named_parameters()
                                        if p.grad is not None), tm

    loss_f, grads_f, tm_f = step(True)
    loss_t, grads_t, tm_t = step(False)
    assert float((tm_f - tm_t).abs().max()) <= R.BOUND * float(tm_t.abs().max())
    assert abs(loss_f - loss_t) <= 1e-5 * abs(loss_t)
    assert set(grads_f) == set(grads_t) and any(n.endswith("hash_table") for n in grads_f)
    assert any(not n.endswith("hash_table") for n in grads_f)            # the table and the MLP
    for n, gf in grads_f.items():
        gt = grads_t[n]
        sc = float(gt.abs().max())
        assert bool(torch.isfinite(gf).all()) and float(gf.abs().max()) > 0, n
        print(f"{n}: max|fused - torch| = {float((gf - gt).abs().max()):.3e}, bound {2e-5 * sc:.3e}")
        assert float((gf - gt).abs().max()) <= 2e-5 * sc, n


def test_other_entry_points():
    import goldens as G
    import test_input_grad_gpu as T
    from adaptive_city_nerf_amd import render_image, render_rays
    from adaptive_city_nerf_amd._lib import AcnError
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step
    m, gbox = T._container("k4")
    cam = G.scene()["val_cam0"]
    intr = torch.tensor(cam["intrinsics"], dtype=torch.float32)
    s = 16.0 / float(2.0 * intr[2])
    img, depth, acc = render_image(m, H=16, W=16, fx=float(intr[0]) * s, fy=float(intr[1]) * s, cx=8.0, cy=8.0,
                                   c2w=torch.tensor(cam["c2w"]), scene_box=gbox, ray_samples=16, n_importance=8)
    assert img.shape == (16, 16, 3) and bool(torch.isfinite(img).all()) and depth.shape == (256,)
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(acc).all())
    occ_model = type("M", (), {"use_occ": True, "occ_ready": True, "warned_occ_ready": True})()
    with pytest.raises(AcnError, match="occupancy"):
        render_rays(occ_model, torch.zeros(4, 8, device=DEV), ray_samples=8, n_importance=4)
    from test_graph_gpu import _setup
    P, model, opt, d = _setup()
    rays = torch.from_numpy(d["train0:rays"]).to(DEV)[:256].contiguous()
    rgbs = torch.from_numpy(d["train0:rgbs"]).to(DEV)[:256].contiguous()
    before = [p.detach().clone() for p in model.parameters()]
    loss = adapt_step(P, model, rays, rgbs, opt, active_module=0, grad_clip=1.0, n_importance=8)
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    with pytest.raises(ValueError, match="n_importance"):
        GraphedAdaptStep(P, model, rays, rgbs, opt, active_module=0, n_importance=8)
