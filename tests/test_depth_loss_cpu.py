"""Host-side checks of depth supervision, no GPU needed: the float64 reference of
tests/depth_loss_ref.py has the gradient autograd gives it and its inputs exercise both line-of-sight branches; the
package's torch form (CPU tensors, other dtypes, second_order()) agrees with it, on the special rays too; the mean counts
only the rays that carry a target; point_depth_targets, depth_metrics, the refusals and the training entry points'
arguments."""
import ctypes as C
import inspect
import math

import pytest
import torch

import depth_loss_ref as D

# |got - ref| <= 4 * 2^-24 (four fp32 roundings; the torch form rounds its float64 result to fp32 once) of the ray's
# largest reference value, + 1e-30 for a ray whose values are all 0
TOL = 4 * 2.0 ** -24


def _rel(got, ref, per_ray_max):
    return float(((got.double() - ref).abs() / (TOL * per_ray_max + 1e-30)).max())


def _ray_max(v, starts, counts):
    return torch.stack([v[s:s + c].abs().max() if c else v.new_zeros(()) for s, c in zip(starts.tolist(),
                                                                                          counts.tolist())])


def test_reference_gradient_is_autograd_of_its_loss_and_both_sight_branches_are_exercised():
    """The closed-form gradient against float64 autograd of L: the two evaluate the same few products in a different
    order, so they agree to a few float64 roundings of the ray's largest gradient (1e-14 of it allows ~45).  On every
    ray of S >= 64 samples at least 2 samples overlap the window and at least 10 lie wholly in front of it."""
    worst = 0.0
    for shape in D.DENSE_SHAPES:
        for offset in D.OFFSETS:
            w, t, z, eps, c = D.dense_inputs(shape, offset)
            s, e, tau = D.dense_intervals(t)
            for r in range(shape[0]):
                wd = w[r].double().requires_grad_(True)
                loss, grad = D.ray_loss(wd, s[r], e[r], tau[r], float(z[r]), float(eps[r]), float(c[r]))
                auto, = torch.autograd.grad(loss, wd)
                worst = max(worst, float((auto - grad.detach()).abs().max() / grad.detach().abs().max()))
                if shape[1] >= 64:
                    over, front = D.window_counts(s[r], e[r], float(z[r]), float(eps[r]))
                    assert over >= 2 and front >= 10, (shape, offset, r, over, front)
    print(f"closed form against autograd: {worst:.3e} of the ray's largest gradient")
    assert worst <= 1e-14
    for offset in D.OFFSETS:
        w, t0, t1, starts, counts, z, eps, c = D.packed_inputs(offset)
        wd = w.double().requires_grad_(True)
        total = 0.0
        for r, (a, n) in enumerate(zip(starts.tolist(), counts.tolist())):
            sl = slice(a, a + n)
            lo, hi = t0[sl].double(), t1[sl].double()
            total = total + D.ray_loss(wd[sl], lo, hi, 0.5 * (lo + hi), float(z[r]), float(eps[r]), float(c[r]))[0]
        total.backward()
        _, grad = D.packed_reference(offset, (1.0, 1.0))
        gmax = _ray_max(grad, starts, counts)
        assert float(((wd.grad - grad).abs() / (1e-14 * torch.repeat_interleave(gmax, counts) + 1e-300)).max()) <= 1
    # the mass of a window the samples cover is Phi(3) - Phi(-3)
    w, t, z, eps, c = D.dense_inputs((9, 256), 100.0)
    s, e, _ = D.dense_intervals(t)
    k = D.kernel_mass(s[3], e[3], float(z[3]), float(eps[3]))
    assert abs(float(k.sum()) - D.K3) <= 1e-14


@pytest.mark.parametrize("lam", D.LAMBDAS)
def test_torch_form_agrees_with_the_reference(lam):
    from adaptive_city_nerf_amd import depth_loss, nerfacc
    for shape in ((37, 2), (3, 65), (9, 256), (2, 1000)):
        for offset in D.OFFSETS:
            w, t, z, eps, c = D.dense_inputs(shape, offset)
            ref_l, ref_g = D.dense_reference(shape, offset, lam)
            rays = torch.zeros(shape[0], 8)
            rays[:, 6], rays[:, 7] = t[:, 0], t[:, -1]
            assert torch.equal(1.0 / (rays[:, 7] - rays[:, 6]), c)             # c as depth_loss derives it
            ref_c = (ref_l, ref_g)
            wl = w.clone().requires_grad_(True)
            loss = depth_loss(wl, t, z, eps, rays=rays, depth_weight=lam[0], sight_weight=lam[1], reduction="none")
            assert loss.shape == (shape[0],) and loss.dtype == torch.float32
            loss.sum().backward()
            e_l = _rel(loss.detach(), ref_c[0], ref_c[0].abs())
            e_g = _rel(wl.grad, ref_c[1], ref_c[1].abs().amax(1, keepdim=True))
            print(f"dense {shape}, offset {offset}, weights {lam}: loss {e_l:.3f}, grad {e_g:.3f} of the bound")
            assert e_l <= 1 and e_g <= 1
    for offset in D.OFFSETS:
        w, t0, t1, starts, counts, z, eps, c = D.packed_inputs(offset)
        N = len(D.PACKED_COUNTS)
        ri = torch.repeat_interleave(torch.arange(N), counts)
        ref_l, ref_g = D.packed_reference(offset, lam)
        wl = w.clone().requires_grad_(True)
        loss = nerfacc.depth_loss(wl, t0, t1, z, eps, ray_indices=ri, n_rays=N, ray_scale=c, depth_weight=lam[0],
                                  sight_weight=lam[1])
        assert loss.shape == (N,) and loss.dtype == torch.float32
        gsel = 2.0 ** (torch.arange(N) % 5 - 2).float()          # exact factors: g_loss reaches the rays
        (loss * gsel).sum().backward()
        gmax = _ray_max(ref_g, starts, counts)
        e_l = _rel(loss.detach(), ref_l, ref_l.abs())
        e_g = _rel(wl.grad / gsel[ri], ref_g, gmax[ri])
        print(f"packed, offset {offset}, weights {lam}: loss {e_l:.3f}, grad {e_g:.3f} of the bound")
        assert e_l <= 1 and e_g <= 1
        # an empty ray with a target: D = 0, the loss is the depth term of z alone
        assert float(loss.detach()[0]) == pytest.approx(lam[0] * (float(c[0]) * float(z[0])) ** 2, rel=1e-6)
    # batched (n_rays, n_samples) rows are the packed samples as rows
    w, t, z, eps, c = D.dense_inputs((3, 65), 100.0)
    d = torch.cat([t[:, 1:] - t[:, :-1], t[:, -1:] - t[:, -2:-1]], 1)
    st = torch.arange(3) * 65
    ref_b, _ = D.packed(w.reshape(-1), t.reshape(-1), (t + d).reshape(-1), st, torch.full((3,), 65), z, eps, c, *lam)
    got_b = nerfacc.depth_loss(w, t, t + d, z, eps, ray_scale=c, depth_weight=lam[0], sight_weight=lam[1])
    assert got_b.shape == (3,) and _rel(got_b, ref_b, ref_b.abs()) <= 1
    # float64 inputs stay float64; eps as a float
    assert depth_loss(w.double(), t.double(), z.double(), 0.5).dtype == torch.float64
    one = depth_loss(w, t, z, 0.5, reduction="none")
    assert torch.equal(one, depth_loss(w, t, z, torch.full((3,), 0.5), reduction="none"))


def _check_special(loss11, grad11, loss10, grad10, loss01, grad01, rel):
    """The exact expectations of depth_loss_ref.special_rays(), for any implementation: (loss, grad) at the weights
    (1,1), (1,0), (0,1) as CPU tensors; ``rel(got, ref, per_ray_max)`` the worst error over its bound."""
    w, t, z, eps, c = D.special_rays()
    i = {n: k for k, n in enumerate(D.SPECIAL)}
    for loss, grad in ((loss11, grad11), (loss10, grad10), (loss01, grad01)):
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
        for dead in ("no_target", "zero_scale_nan_t"):
            assert float(loss[i[dead]]) == 0.0 and bool((grad[i[dead]] == 0).all())
    for lam, (loss, grad) in zip(D.LAMBDAS, ((loss11, grad11), (loss10, grad10), (loss01, grad01))):
        ref_l, ref_g = D.dense(w, torch.nan_to_num(t), z, eps, c, *lam)
        assert rel(loss, ref_l, ref_l.abs()) <= 1 and rel(grad, ref_g, ref_g.abs().amax(1, keepdim=True)) <= 1
    r = i["window_before"]      # no sample starts before hi: the sight term is exactly 0
    assert float(loss01[r]) == 0.0 and bool((grad01[r] == 0).all())
    assert torch.equal(loss11[r], loss10[r]) and torch.equal(grad11[r], grad10[r]) and float(loss10[r]) > 0
    r = i["window_beyond"]      # every k is 0: the sight term is sum w^2, its gradient 2 w
    assert torch.equal(grad01[r], 2.0 * w[r])
    sw2 = (w[r].double() ** 2).sum()
    assert abs(float(loss01[r]) - float(sw2)) <= TOL * float(sw2)
    r, j = i["narrow_window"], D.NARROW_J    # the window inside interval j alone: k_j = Phi(3) - Phi(-3), others 0
    ref_g = 2.0 * w[r].double()
    ref_g[j] = 2.0 * (float(w[r, j]) - D.K3)
    live = (t[r].double() < float(z[r]) + float(eps[r])).double()
    assert float((grad01[r].double() - ref_g * live).abs().max()) <= TOL * float(ref_g.abs().max())
    r = i["opaque_first"]
    assert float(w[r, 0]) == 1.0 and bool((w[r, 1:] == 0).all())
    d_err = float(c[r]) * (float(t[r, 0]) - float(z[r]))    # D = t_0
    assert abs(float(loss10[r]) - d_err ** 2) <= TOL * d_err ** 2


def test_special_rays_on_the_torch_form():
    from adaptive_city_nerf_amd import nerfacc
    w, t, z, eps, c = D.special_rays()
    s, e, tau = D.dense_intervals(t)
    out = []
    for lam in D.LAMBDAS:
        wl = w.clone().requires_grad_(True)
        loss = nerfacc._depth_loss_torch(wl, s, e, tau, z, eps, c, *lam)
        loss.sum().backward()
        out += [loss.detach(), wl.grad]
    _check_special(*out, _rel)


def test_mean_counts_only_the_rays_that_carry_a_target():
    from adaptive_city_nerf_amd import depth_loss
    w, t, z, eps, c = D.dense_inputs((64, 96), 100.0)
    z = z.clone()
    z[5:60] = float("nan")                       # 9 of 64 rays keep a target
    z[60] = -1.0
    eps = eps.clone()
    eps[61] = 0.0
    rays = torch.zeros(64, 8)
    rays[:, 6], rays[:, 7] = t[:, 0], t[:, -1]
    rays[62, 7] = rays[62, 6]                    # far == near: c = 0
    per_ray = depth_loss(w, t, z, eps, rays=rays, reduction="none")
    live = torch.ones(64, dtype=torch.bool)
    live[5:63] = False
    assert bool((per_ray[~live] == 0).all()) and bool((per_ray[live] > 0).all()) and int(live.sum()) == 6
    assert torch.equal(depth_loss(w, t, z, eps, rays=rays), per_ray.sum() / 6)
    assert torch.equal(depth_loss(w, t, z, eps, rays=rays, reduction="sum"), per_ray.sum())
    # no ray with a target: 0 / max(0, 1), not NaN
    none = depth_loss(w, t, torch.full((64,), float("nan")), eps, rays=rays)
    assert float(none) == 0.0


def test_second_order_takes_the_twice_differentiable_form():
    from adaptive_city_nerf_amd import depth_loss
    from adaptive_city_nerf_amd.ray_rendering import second_order
    w, t, z, eps, c = D.dense_inputs((3, 65), 0.0)
    wl = (w + 0.01).requires_grad_(True)
    with second_order():
        loss = depth_loss(wl, t, z, eps, reduction="sum")
        g, = torch.autograd.grad(loss, wl, create_graph=True)
        assert g.requires_grad
        h, = torch.autograd.grad(g[1, 20], wl)
    # d2 L / dw_20 dw_j = 2 t_20 t_j (+ 2 m_20 at j = 20), c = 1
    ref = 2.0 * t[1, 20].double() * t[1].double()
    ref[20] += 2.0 * float(t[1, 20] < z[1] + eps[1])
    assert float((h[1].double() - ref).abs().max()) <= 1e-6 * float(ref.max())
    assert bool((h[0] == 0).all()) and bool((h[2] == 0).all())


def _pixel_rays(H, W, fx, fy, cx, cy, center, c2w):
    """get_ray_directions and get_rays restated as torch ops (float64): unit RUB directions per pixel, row-major, turned
    into the world frame; origin = the pose's translation."""
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    if center:
        i, j = i + 0.5, j + 0.5
    d = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    d = d.reshape(-1, 3) @ c2w[:3, :3].double().T
    return c2w[:3, 3].double().expand_as(d), d


def _pose():
    a, b = 0.4, -0.3
    rz = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    return torch.cat([rz @ rx, torch.tensor([[3.0], [-2.0], [1.5]])], 1)


@pytest.mark.parametrize("center", [True, False])
def test_point_depth_targets_round_trip(center):
    """For X = o + t d on pixel p's own ray, the target at p is t (to the fp32 rounding of X and of the result: each
    coordinate of X is rounded once, relative 2^-24 of |o| + t, and so is the output)."""
    from adaptive_city_nerf_amd import point_depth_targets
    H, W, fx, fy, cx, cy = 7, 5, 6.0, 6.5, 2.3, 3.6
    c2w = _pose()
    o, d = _pixel_rays(H, W, fx, fy, cx, cy, center, c2w)
    gen = torch.Generator().manual_seed(1)
    tt = 2.0 + 8.0 * torch.rand(H * W, generator=gen, dtype=torch.float64)
    X = (o + tt[:, None] * d).float()
    got = point_depth_targets(X, c2w, H, W, fx, fy, cx, cy, center)
    assert got.shape == (H * W,) and got.dtype == torch.float32
    bound = 8 * 2.0 ** -24 * (float(o[0].norm()) + tt)
    assert bool(((got.double() - tt).abs() <= bound).all()), (got.double() - tt).abs().max()
    # a subset of the pixels: the others stay NaN
    keep = torch.arange(H * W) % 3 == 0
    part = point_depth_targets(X[keep], c2w, H, W, fx, fy, cx, cy, center)
    assert bool(torch.isnan(part[~keep]).all()) and torch.equal(part[keep], got[keep])
    # two points on one pixel keep the nearer; one behind the camera or outside the frame leaves NaN
    p = 17
    two = torch.stack([o[p] + 5.0 * d[p], o[p] + 3.0 * d[p]]).float()
    out = point_depth_targets(two, c2w, H, W, fx, fy, cx, cy, center)
    assert abs(float(out[p]) - 3.0) <= 1e-5 and int(torch.isfinite(out).sum()) == 1
    behind = (o[p] - 4.0 * d[p])[None].float()
    assert bool(torch.isnan(point_depth_targets(behind, c2w, H, W, fx, fy, cx, cy, center)).all())
    cam_x = c2w[:3, 0].double()
    outside = (o[p] + 4.0 * d[p] + 40.0 * cam_x)[None].float()
    assert bool(torch.isnan(point_depth_targets(outside, c2w, H, W, fx, fy, cx, cy, center)).all())
    assert bool(torch.isnan(point_depth_targets(torch.zeros(0, 3), c2w, H, W, fx, fy, cx, cy, center)).all())


def test_depth_metrics_on_a_hand_computed_case():
    from adaptive_city_nerf_amd import depth_metrics
    gt = torch.tensor([2.0, float("nan"), 4.0, 0.0, -1.0, 10.0])
    pred = torch.tensor([1.0, 5.0, 6.0, 7.0, 8.0, 10.0])
    m = depth_metrics(pred, gt)          # entries 0, 2, 5: errors -1, 2, 0
    assert set(m) == {"abs_rel", "rmse"}
    assert m["abs_rel"] == pytest.approx((0.5 + 0.5 + 0.0) / 3, rel=1e-12)
    assert m["rmse"] == pytest.approx(math.sqrt(5.0 / 3), rel=1e-12)
    none = depth_metrics(pred, torch.full((6,), float("nan")))
    assert math.isnan(none["abs_rel"]) and math.isnan(none["rmse"])


def _last_error(L):
    buf = C.create_string_buffer(512)
    L.lib().acn_last_error(buf, 512)
    return buf.value.decode()


def test_bad_arguments_are_refused_before_any_hip_call():
    from adaptive_city_nerf_amd import _lib as L
    from adaptive_city_nerf_amd import depth_loss, depth_metrics, nerfacc, occ_ops, ops, point_depth_targets
    w, t = torch.rand(4, 8), torch.rand(4, 8).sort(1).values
    z, i1 = torch.ones(4), torch.zeros(1, dtype=torch.long)
    for bad in (lambda: ops.depth_loss_dense(w[:, :1], t[:, :1], z, 0.1),
                lambda: ops.depth_loss_dense(w, t[:, :7], z, 0.1),
                lambda: depth_loss(w[:, :1], t[:, :1], z, 0.1), lambda: depth_loss(w, t, z[:3], 0.1),
                lambda: depth_loss(w, t, z, torch.ones(3)), lambda: depth_loss(w, t, z, 0.1, rays=torch.zeros(3, 8)),
                lambda: depth_loss(w, t, z, 0.1, rays=torch.zeros(4, 6)),
                lambda: depth_loss(w, t, z, 0.1, depth_weight=-1.0),
                lambda: depth_loss(w, t, z, 0.1, sight_weight=float("nan")),
                lambda: occ_ops.depth_loss_packed(w, t, t, i1, i1, z[:1], 0.1),
                lambda: occ_ops.depth_loss_packed(w[0], t[0], t[0], torch.zeros(2), torch.zeros(1), z[:2], 0.1),
                lambda: nerfacc.depth_loss(w, t, t[:, :7], z, 0.1),
                lambda: nerfacc.depth_loss(w[None], t[None], t[None], z, 0.1),
                lambda: nerfacc.depth_loss(w, t, t, z, 0.1, ray_indices=torch.zeros(4, dtype=torch.long)),
                lambda: nerfacc.depth_loss(w, t, t, z, 0.1, n_rays=5), lambda: nerfacc.depth_loss(w, t, t, z[:3], 0.1),
                lambda: nerfacc.depth_loss(w[0], t[0], t[0], z[:1], 0.1, ray_indices=torch.zeros(7, dtype=torch.long)),
                lambda: point_depth_targets(torch.zeros(3, 2), torch.eye(4), 4, 4, 1.0, 1.0, 2.0, 2.0, True),
                lambda: depth_metrics(torch.zeros(3), torch.zeros(4))):
        with pytest.raises(L.AcnError) as e:
            bad()
        assert "HIP device" not in str(e.value)
    with pytest.raises(ValueError):
        depth_loss(w, t, z, 0.1, reduction="max")
    with pytest.raises(L.AcnError, match="HIP device"):
        ops.depth_loss_dense(w, t, z, 0.1)
    with pytest.raises(L.AcnError, match="HIP device"):
        occ_ops.depth_loss_packed(w[0], t[0], t[0], i1, torch.full((1,), 8), z[:1], 0.1)
    lib = L.lib()
    n = None
    assert lib.acn_depth_loss_dense(n, n, 4, 1, n, n, n, 1.0, 1.0, n, n, n) == -1 and "S >= 2" in _last_error(L)
    assert lib.acn_depth_loss_dense(n, n, -1, 8, n, n, n, 1.0, 1.0, n, n, n) == -1
    assert lib.acn_depth_loss_dense(n, n, 4, 8, n, n, n, -1.0, 1.0, n, n, n) == -1 and ">= 0" in _last_error(L)
    assert lib.acn_depth_loss_dense(n, n, 4, 8, n, n, n, 1.0, 1.0, n, n, n) == -1 and "NULL" in _last_error(L)
    assert lib.acn_depth_loss_dense(n, n, 0, 8, n, n, n, 1.0, 1.0, n, n, n) == 0        # nothing launched
    assert lib.acn_depth_loss_packed(n, n, n, 0, n, n, -1, n, n, n, 1.0, 1.0, n, n, n) == -1
    assert lib.acn_depth_loss_packed(n, n, n, 8, n, n, 2, n, n, n, 1.0, 1.0, n, n, n) == -1
    assert lib.acn_depth_loss_packed(n, n, n, 8, n, n, 2, n, n, n, 1.0, float("nan"), n, n, n) == -1
    assert lib.acn_depth_loss_packed(n, n, n, 8, n, n, 0, n, n, n, 1.0, 1.0, n, n, n) == 0


class _P:
    ray_samples, chunk_points, color_space = 8, 1 << 20, "linear"


def _stub_render(calls):
    gen = torch.Generator().manual_seed(2)
    rgb = torch.rand(6, 3, generator=gen).requires_grad_(True)
    wts = torch.rand(6, 8, generator=gen) * 0.1
    tv = (1.0 + torch.rand(6, 8, generator=gen).cumsum(1))

    def render_rays(model, rays, **kw):
        calls.append(dict(kw))
        out = (rgb, (wts * tv).sum(1), wts, wts.sum(1))
        return out + (tv,) if kw.get("return_t_vals") else out
    return render_rays, wts, tv


def test_training_entry_points(monkeypatch):
    """The arguments, their defaults and the ValueErrors; compute_loss with both weights 0 makes compute_mse_loss's
    calls and returns its loss bit for bit; with a weight it adds depth_loss of the render's weights and t values."""
    from adaptive_city_nerf_amd import depth_loss, train
    for fn in (train.compute_loss, train.adapt_step, train.GraphedAdaptStep.__init__, train.runtime_adapt):
        p = inspect.signature(fn).parameters
        assert p["depth_weight"].default == 0.0 and p["sight_weight"].default == 0.0 and p["depth_eps"].default is None
    assert inspect.signature(train.adapt_step).parameters["depths"].default is None
    assert inspect.signature(train.GraphedAdaptStep.__call__).parameters["depths"].default is None
    calls = []
    stub, wts, tv = _stub_render(calls)
    monkeypatch.setattr(train, "render_rays", stub)
    gen = torch.Generator().manual_seed(3)
    rays = torch.zeros(6, 8)
    rays[:, 6], rays[:, 7] = 1.0, 9.0
    data = {"rays": rays, "rgbs": torch.rand(6, 3, generator=gen)}
    mse = train.compute_mse_loss(_P, None, data)
    zero = train.compute_loss(_P, None, dict(data, depths=torch.ones(6)), depth_weight=0.0, sight_weight=0.0,
                              depth_eps=0.5)
    assert torch.equal(mse, zero) and calls[0] == calls[1] and "return_t_vals" not in calls[1]
    z = torch.tensor([3.0, float("nan"), 4.0, 5.0, float("nan"), 2.0])
    full = train.compute_loss(_P, None, dict(data, depths=z), depth_weight=0.3, sight_weight=0.2, depth_eps=0.5)
    assert calls[2].get("return_t_vals") is True
    term = depth_loss(wts, tv, z, 0.5, rays=rays, depth_weight=0.3, sight_weight=0.2)
    assert float(term) > 0 and torch.equal(full, mse + term)
    with pytest.raises(ValueError, match="depth"):
        train.compute_loss(_P, None, data, depth_weight=0.3, depth_eps=0.5)              # no data["depths"]
    with pytest.raises(ValueError, match="depth_eps"):
        train.compute_loss(_P, None, dict(data, depths=z), sight_weight=0.3)
    with pytest.raises(ValueError, match="depth"):
        train.adapt_step(_P, None, rays, data["rgbs"], None, depth_weight=0.1, depth_eps=0.5)
    with pytest.raises(ValueError, match="expert-parallel"):
        train.adapt_step(None, None, None, None, None, group=object(), depth_weight=0.1)
    with pytest.raises(ValueError, match="expert-parallel"):
        train.adapt_step(None, None, None, None, None, group=object(), sight_weight=0.1)
    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="depth_eps"):
        train.runtime_adapt(P=_P, model=model, data_loader=[], optimizer=None, depth_weight=0.1)
    with pytest.raises(ValueError, match="rays, rgbs, depths"):
        train.runtime_adapt(P=_P, model=model, data_loader=[(rays, data["rgbs"])], optimizer=None, sight_weight=0.1,
                            depth_eps=0.5)


def test_new_names_are_exported():
    import adaptive_city_nerf_amd as A
    from adaptive_city_nerf_amd import metrics, nerfacc, occ_ops, ops, ray_sampling
    assert A.depth_loss is A.ray_rendering.depth_loss and A.point_depth_targets is ray_sampling.point_depth_targets
    assert A.depth_metrics is metrics.depth_metrics and "depth_metrics" in metrics.__all__
    assert "depth_loss" in nerfacc.__all__
    assert list(inspect.signature(A.depth_loss).parameters) == ["weights", "t_vals", "depths", "eps", "rays",
                                                                "depth_weight", "sight_weight", "reduction"]
    assert list(inspect.signature(nerfacc.depth_loss).parameters)[:7] == ["weights", "t_starts", "t_ends", "depths",
                                                                          "eps", "ray_indices", "n_rays"]
    assert callable(ops.depth_loss_dense) and callable(occ_ops.depth_loss_packed)
    assert list(inspect.signature(ray_sampling.point_depth_targets).parameters) == [
        "points", "c2w", "H", "W", "fx", "fy", "cx", "cy", "center_pixels"]
