"""The fused interlevel loss on the GPU (acn_interlevel_loss) against the O(S P) float64 definition
of tests/interlevel_ref.py, and its way up: interlevel_loss, proposal_weights, render_rays_proposal, render_rays /
render_image / adapt_step with a proposal.

The kernel works in float64 and rounds the loss and each gradient element to fp32 once, so per ray
|got - ref| <= 4 * 2^-24 * (largest |ref| of that ray) + floor, with floor = 4 * |definition - prefix form| + 1e-30 taken
from the reference alone (its own sensitivity to float64 summation order).  The worst ratio to the bound is printed.

Measured on an MI355X (worst ratio to the bound over the three offsets, loss / gradient): see DESIGN.md §4aa."""
import numpy as np
import pytest
import torch

import interlevel_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(37, 2, 2), (5, 64, 64), (3, 65, 63), (8, 33, 96), (4, 192, 64), (2, 1024, 1024)]


def _dev(c):
    return tuple(c[k].to(DEV) for k in ("t_fine", "w_fine", "t_prop", "w_prop"))


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_definition(shape):
    from adaptive_city_nerf_amd import ops
    N, S, P = shape
    for offset in R.OFFSETS:
        c = R.case(N, S, P, offset)
        t, w, tp, wp = _dev(c)
        loss, grad = ops.interlevel_loss(t, w, tp, wp)
        torch.cuda.synchronize()
        assert loss.shape == (N,) and grad.shape == (N, P) and loss.dtype == grad.dtype == torch.float32
        rl, rg = R.ratios(c, loss.cpu().numpy(), grad.cpu().numpy())
        print(f"{shape}, t offset {offset}: loss at {rl:.3f}, gradient at {rg:.3f} of the bound "
              f"(floors {c['floor_loss']:.1e}, {c['floor_grad']:.1e})")
        assert rl <= 1 and rg <= 1
        if c["rows"]:
            d = c["rows"]["dominated"]
            assert float(loss[d]) == 0.0 and not bool(grad[d].any())
        # repeatable bit for bit, and the loss does not depend on whether the gradient is written
        again = ops.interlevel_loss(t, w, tp, wp)
        bare = ops.interlevel_loss(t, w, tp, wp, want_grad=False)
        assert torch.equal(again[0], loss) and torch.equal(again[1], grad)
        assert bare[1] is None and torch.equal(bare[0], loss)
        # a power-of-two ray scale is exact; a ray of scale 0 gets exact zeros and its NaN depths are not read
        scale = torch.tensor([4.0, 0.25, 1.0, 0.5], device=DEV).repeat(N // 4 + 1)[:N].contiguous()
        scale[N - 1] = 0.0
        t2, tp2, w2 = t.clone(), tp.clone(), wp.clone()
        t2[N - 1], tp2[N - 1], w2[N - 1] = float("nan"), float("nan"), float("nan")
        ls, gs = ops.interlevel_loss(t2, w, tp2, w2, ray_scale=scale)
        assert torch.equal(ls, loss * scale) and torch.equal(gs, grad * scale[:, None])
        assert float(ls[N - 1]) == 0.0 and not bool(gs[N - 1].any())
        assert torch.equal(ops.interlevel_loss(t2, w, tp2, w2, ray_scale=scale, want_grad=False)[0], ls)


def test_a_bad_row_changes_no_other_ray():
    """A NaN row, a descending row and an infinite depth hold garbage of their own; every other ray keeps its bits."""
    from adaptive_city_nerf_amd import ops
    for shape in ((8, 33, 96), (5, 64, 64)):
        c = R.case(*shape, 100.0)
        N = shape[0]
        t, w, tp, wp = _dev(c)
        loss, grad = ops.interlevel_loss(t, w, tp, wp)
        t2, tp2, w2 = t.clone(), tp.clone(), w.clone()
        t2[0] = float("nan")                         # NaN fine depths
        tp2[1] = tp[1].flip(0)                       # descending proposal depths
        t2[2, -1] = float("inf")                     # an infinite last depth
        w2[N - 1, 0] = float("nan")                  # a NaN weight
        bad = [0, 1, 2, N - 1]
        keep = torch.tensor([i for i in range(N) if i not in bad], device=DEV)
        l2, g2 = ops.interlevel_loss(t2, w2, tp2, wp)
        torch.cuda.synchronize()
        assert torch.equal(l2[keep], loss[keep]) and torch.equal(g2[keep], grad[keep])


def test_limits_are_refused_without_a_launch():
    from adaptive_city_nerf_amd import interlevel_loss, ops
    from adaptive_city_nerf_amd._lib import AcnError, lib
    from adaptive_city_nerf_amd.ops import ptr
    c = R.case(2, 1024, 1024, 0.0)
    t, w, tp, wp = _dev(c)
    big = torch.cat([t, t[:, -1:] + 1.0], 1)
    wbig = torch.cat([w, torch.zeros(2, 1, device=DEV)], 1)
    out = torch.full((2,), 7.0, device=DEV)
    L = lib()
    assert L.acn_interlevel_loss(ptr(big), ptr(wbig), 1025, ptr(tp), ptr(wp), 1024, 2, None, R.EPS, ptr(out), None,
                                 None) != 0
    assert L.acn_interlevel_loss(ptr(t), ptr(w), 1024, ptr(big), ptr(wbig), 1025, 2, None, R.EPS, ptr(out), None,
                                 None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(AcnError, match="1024"):
        ops.interlevel_loss(big, wbig, tp, wp)
    with pytest.raises(AcnError, match="1024"):
        ops.interlevel_loss(t, w, big, wbig)
    # interlevel_loss takes the torch chain past the limits: the extra fine sample has weight 0 and is bounded
    got = interlevel_loss(big, wbig, tp, wp, reduction="none")
    ref = R.definition(big.cpu().numpy(), wbig.cpu().numpy(), c["t_prop"].numpy(), c["w_prop"].numpy())[0]
    assert np.allclose(got.cpu().numpy(), ref, rtol=4 * 2.0 ** -24, atol=0)


def test_autograd_and_the_torch_path():
    from adaptive_city_nerf_amd import interlevel_loss, ops
    from adaptive_city_nerf_amd import ray_rendering as RR
    N, S, P = shape = (8, 33, 96)
    c = R.case(*shape, 100.0)
    t, w, tp, wp = _dev(c)
    loss, grad = ops.interlevel_loss(t, w, tp, wp)
    wl = wp.clone().requires_grad_(True)
    out = interlevel_loss(t.clone().requires_grad_(True), w.clone().requires_grad_(True), tp, wl)
    assert torch.equal(out, loss.mean())
    out.backward()
    assert torch.equal(wl.grad, grad * (torch.ones((), device=DEV) / N))
    none = interlevel_loss(t, w, tp, wp, reduction="none")
    assert torch.equal(none, loss) and not none.requires_grad
    assert torch.equal(interlevel_loss(t, w, tp, wp, reduction="sum"), loss.sum())
    # rays: scale 1 where far > near, an exact 0 otherwise (NaN bounds included)
    rays = torch.zeros(N, 8, device=DEV)
    rays[:, 7] = 1.0
    rays[3, 6:] = float("nan")
    rays[4, 7] = 0.0
    wl = wp.clone().requires_grad_(True)
    lr = interlevel_loss(t, w, tp, wl, rays=rays, reduction="none")
    mask = torch.ones(N, device=DEV)
    mask[3], mask[4] = 0.0, 0.0
    assert torch.equal(lr, loss * mask)
    lr.sum().backward()
    assert torch.equal(wl.grad, grad * mask[:, None])
    # the torch chain on the device is the same definition, within the same bound
    prev = RR.FUSED_INTERLEVEL
    RR.FUSED_INTERLEVEL = False
    try:
        wl = wp.clone().requires_grad_(True)
        lt = interlevel_loss(t, w, tp, wl, reduction="none")
        lt.sum().backward()
    finally:
        RR.FUSED_INTERLEVEL = prev
    rl, rg = R.ratios(c, lt.detach().cpu().numpy(), wl.grad.cpu().numpy())
    print(f"{shape} through the torch chain: loss at {rl:.3f}, gradient at {rg:.3f} of the bound")
    assert rl <= 1 and rg <= 1
    with RR.second_order():      # twice differentiable: the torch chain
        wl = wp.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(interlevel_loss(t, w, tp, wl), wl, create_graph=True)
        assert g.requires_grad


# ------------------------------------------------------------------------------------------------ the renders
def _expert():
    import test_input_grad_gpu as T
    return T._expert()


def _proposal(box, levels):
    """A small density field: ``levels`` coarse hash levels up to resolution 128 (16 levels: the fused field's
    configuration, whose no-grad density is one launch; 4: the intended proposal, hash-grid kernel plus sigma branch)."""
    import test_input_grad_gpu as T
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    conf = dict(T.HASH_CONF, levels=levels, max_res=128)
    torch.manual_seed(5)
    p = MetaNGP(occ_conf={"use_occ": False}, scene_box=box, hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15,
                color_depth=2, use_sigmoid_rgb=True, hash_enc_conf=conf, dir_encoding="spherical").to(DEV)
    with torch.no_grad():
        p.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    assert p._fusable == (levels == 16)
    return p


def _rays(m, n, seed):
    import test_f16_table_gpu as T16
    return T16._rays(m, n, seed)


def _hand_composed(m, prop, rays, P, F, u=None, uf=None):
    """density -> weights -> sample_pdf -> render_rays_at, with the package's own pieces."""
    from adaptive_city_nerf_amd import nerfacc, render_rays_at, sample_pdf, stratified_t_vals
    N = rays.shape[0]
    t = stratified_t_vals(rays[:, 6], rays[:, 7], P, randomized=u is not None, u=u)
    sig = prop.density((rays[:, None, :3] + rays[:, None, 3:6] * t[..., None]).reshape(-1, 3)).reshape(N, P)
    t_end = torch.cat([t[:, 1:], t[:, -1:] + (t[:, -1:] - t[:, -2:-1])], 1)
    starts = torch.arange(N, device=DEV) * P
    w = nerfacc.render_weight_from_density(t.reshape(-1), t_end.reshape(-1), sig.reshape(-1),
                                           packed_info=torch.stack([starts, torch.full_like(starts, P)], -1))[0]
    w = w.view(N, P)
    t_fine = sample_pdf(t, w.detach(), F, uf)
    return render_rays_at(m, rays, t_fine), (t, w), t_fine


@pytest.mark.parametrize("levels", [16, 4])
def test_proposal_render_in_eval_mode(levels):
    from adaptive_city_nerf_amd import render_rays, render_rays_proposal
    N, P, F = 64, 16, 16
    m = _expert().eval().requires_grad_(False)
    prop = _proposal(m.scene_box, levels).eval().requires_grad_(False)
    rays = _rays(m, N, 21)
    with torch.no_grad():
        ref, (t_prop, w_prop), t_fine = _hand_composed(m, prop, rays, P, F)
        out = render_rays_proposal(m, prop, rays, P, F, return_proposal=True, return_t_vals=True)
        plain = render_rays(m, rays, ray_samples=P, n_importance=F, proposal=prop)
    assert len(out) == 6 and len(plain) == 4 and out[2].shape == (N, F)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], ref))
    assert all(torch.equal(a, b) for a, b in zip(plain, ref))
    assert torch.equal(out[4][0], t_prop) and torch.equal(out[4][1], w_prop) and torch.equal(out[5], t_fine)
    assert bool(torch.isfinite(out[0]).all()) and float(out[3].max()) > 0 and float(w_prop.sum(1).max()) > 0
    assert bool((t_fine[:, 1:] >= t_fine[:, :-1]).all())


def test_render_image_with_a_proposal():
    import goldens as G
    import test_input_grad_gpu as T
    from adaptive_city_nerf_amd import ops, render_image, render_rays_proposal
    m, gbox = T._container("k4")
    prop = _proposal(gbox, 4).eval().requires_grad_(False)
    cam = G.scene()["val_cam0"]
    intr = torch.tensor(cam["intrinsics"], dtype=torch.float32)
    s = 16.0 / float(2.0 * intr[2])
    kw = dict(H=16, W=16, fx=float(intr[0]) * s, fy=float(intr[1]) * s, cx=8.0, cy=8.0)
    c2w = torch.tensor(cam["c2w"])
    img, depth, acc = render_image(m, c2w=c2w, scene_box=gbox, ray_samples=16, n_importance=16, proposal=prop, **kw)
    rays, _ = ops.get_rays_image(kw["H"], kw["W"], kw["fx"], kw["fy"], kw["cx"], kw["cy"], c2w, gbox.aabb, DEV,
                                 center_pixels=True, near_far_override=(None, None), apply_clamp=True)
    with torch.no_grad():
        rgb, d, _, a = render_rays_proposal(m, prop, rays, 16, 16)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all()) and bool(torch.isfinite(acc).all())
    assert torch.equal(img, rgb.view(16, 16, 3).float().clamp_(0, 1)) and torch.equal(depth, d) and torch.equal(acc, a)


def _train_setup():
    """test_graph_gpu's training model (the k4 container of the goldens, in training mode) with its scene box."""
    import goldens as G
    from test_module_api import build_model, reference_state_dict
    from test_train import P
    from adaptive_city_nerf_amd import SceneBox
    d = G.load("train_k4")
    m, _ = build_model("k4")
    m.load_state_dict(reference_state_dict(d, len(m.submodules), "w:"))
    sc = G.scene()["masks"][G.MASK["k4"]]
    return P, m.cuda().train(), SceneBox(aabb=torch.tensor(sc["aabb_global"], dtype=torch.float32)), d


def test_adapt_step_trains_the_proposal():
    from adaptive_city_nerf_amd import interlevel_loss, render_rays
    from adaptive_city_nerf_amd.optim import build_optimizer
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step, compute_loss
    P, model, gbox, d = _train_setup()
    prop = _proposal(gbox, 4).train()
    N, S, F = 256, P.ray_samples, 16
    rays = torch.from_numpy(d["train0:rays"]).to(DEV)[:N].contiguous()
    rgbs = torch.from_numpy(d["train0:rgbs"]).to(DEV)[:N].contiguous()
    g = torch.Generator().manual_seed(4)
    u, uf = torch.rand(N, S, generator=g).to(DEV), torch.rand(N, F, generator=g).to(DEV)
    kw = dict(n_importance=F, jitter_u=u, jitter_fine=uf)
    # the interlevel term has no graph to the main model; the image has none to the proposal
    rgb, _, w, _, (t_prop, w_prop), t_fine = render_rays(model, rays, ray_samples=S, active_module=0, proposal=prop,
                                                         return_proposal=True, return_t_vals=True, **kw)
    assert rgb.requires_grad and w_prop.requires_grad and not t_fine.requires_grad and w.shape == (N, F)
    inter = interlevel_loss(t_fine, w, t_prop, w_prop, rays=rays)
    assert float(inter.detach()) > 0
    assert all(x is None for x in torch.autograd.grad(inter, list(model.parameters()), allow_unused=True,
                                                      retain_graph=True))
    assert all(x is None for x in torch.autograd.grad(rgb.sum(), list(prop.parameters()), allow_unused=True,
                                                      retain_graph=True))
    gp = torch.autograd.grad(inter, prop.xyz_encoder.hash_table)[0]
    assert bool(torch.isfinite(gp).all()) and float(gp.abs().max()) > 0
    total = compute_loss(P, model, {"rays": rays, "rgbs": rgbs}, active_module=0, proposal=prop, **kw)
    assert float(total.detach()) > float(inter.detach()) > 0
    # one step over both fields
    opt = build_optimizer(P, model)
    with pytest.raises(ValueError, match="optimizer"):
        adapt_step(P, model, rays, rgbs, opt, active_module=0, proposal=prop, **kw)
    opt.add_param_group({"params": list(prop.parameters()), "lr": 0.01, "name": "proposal"})
    table = prop.xyz_encoder.hash_table.detach().clone()
    before = [p.detach().clone() for p in model.submodules[0].parameters()]
    loss = adapt_step(P, model, rays, rgbs, opt, active_module=0, grad_clip=1.0, proposal=prop, **kw)
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert not torch.equal(table, prop.xyz_encoder.hash_table)
    assert bool(torch.isfinite(prop.xyz_encoder.hash_table).all())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.submodules[0].parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    # the refusals
    with pytest.raises(ValueError, match="n_importance"):
        adapt_step(P, model, rays, rgbs, opt, active_module=0, proposal=prop)
    with pytest.raises(ValueError, match="group"):
        adapt_step(P, model, rays, rgbs, opt, proposal=prop, group=object(), **kw)
    with pytest.raises(ValueError, match="proposal"):
        GraphedAdaptStep(P, model, rays, rgbs, opt, active_module=0, proposal=prop, **kw)
