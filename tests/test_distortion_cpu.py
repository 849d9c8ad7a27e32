"""Host-side checks of the distortion loss, no GPU needed: the O(S^2) float64 reference of
tests/distortion_ref.py has the gradient autograd gives it; the package's torch form (CPU tensors, other dtypes,
second_order()) agrees with it; a zero ray scale gives exact zeros; bad shapes are refused before any HIP call; the new
names are exported."""
import ctypes as C

import pytest
import torch

import distortion_ref as R

# |got - ref| <= 2.4e-7 (= 4 * 2^-24, four fp32 roundings) of the ray's largest reference value, + 1e-30 for a ray whose
# values are all 0; the torch form rounds its float64 result to fp32 once
TOL = 2.4e-7
COUNTS = [0, 1, 2, 63, 64, 65, 129, 256, 1000]


def test_reference_gradient_is_autograd_of_its_loss():
    gen = torch.Generator().manual_seed(0)
    w, t0, t1, starts, counts = R.packed_case([40, 1, 7], 3.0, gen)
    wd = (w.double() + 0.01 * torch.rand(w.shape, generator=gen, dtype=torch.float64)).requires_grad_(True)
    total = 0.0
    for s, c in zip(starts.tolist(), counts.tolist()):
        sl = slice(s, s + c)
        total = total + R.ray_loss(wd[sl], 0.5 * (t0[sl].double() + t1[sl].double()), (t1[sl] - t0[sl]).double())[0]
    total.backward()
    _, grad = R.packed(wd, t0, t1, starts, counts)
    assert float((wd.grad - grad).abs().max()) <= 1e-13 * float(grad.abs().max())
    # dense layout: the last width is its predecessor's, a step below 1e-4 is 1e-4
    wv, t = R.dense_case(3, 9, 0.0, gen)
    t[1, 4] = t[1, 3] + 1e-6
    m, d = R.dense_intervals(t)
    assert torch.equal(d[:, -1], d[:, -2]) and float(d[1, 3]) == float(torch.tensor(1e-4))
    ww = wv.double().requires_grad_(True)
    sum(R.ray_loss(ww[r], m[r], d[r])[0] for r in range(3)).backward()
    _, gd = R.dense(ww, t)
    assert float((ww.grad - gd).abs().max()) <= 1e-13 * float(gd.abs().max())


def _rel(got, ref, per_ray_max):
    """Worst |got - ref| in units of the bound TOL * (the ray's largest value) + 1e-30."""
    return float(((got.double() - ref).abs() / (TOL * per_ray_max + 1e-30)).max())


def _ray_max(v, starts, counts):
    return torch.stack([v[s:s + c].abs().max() if c else v.new_zeros(()) for s, c in zip(starts.tolist(),
                                                                                          counts.tolist())])


@pytest.mark.parametrize("offset", [0.0, 100.0, 5000.0])
def test_torch_form_agrees_with_the_reference(offset):
    from adaptive_city_nerf_amd import distortion_loss, nerfacc
    gen = torch.Generator().manual_seed(int(offset) + 1)
    # packed, by ray index
    w, t0, t1, starts, counts = R.packed_case(COUNTS, offset, gen, opaque_ray=5)
    ri = torch.repeat_interleave(torch.arange(len(COUNTS)), counts)
    ref_l, ref_g = R.packed(w, t0, t1, starts, counts)
    wl = w.clone().requires_grad_(True)
    loss = nerfacc.distortion(wl, t0, t1, ray_indices=ri, n_rays=len(COUNTS))
    assert loss.shape == (len(COUNTS),) and loss.dtype == torch.float32
    gsel = 2.0 ** torch.randint(-2, 3, (len(COUNTS),), generator=gen).float()   # exact factors: g_loss reaches the rays
    (loss * gsel).sum().backward()
    gmax = _ray_max(ref_g, starts, counts)
    e_l = _rel(loss.detach(), ref_l, ref_l.abs())
    e_g = _rel(wl.grad / gsel[ri], ref_g, gmax[ri])
    print(f"offset {offset}: packed loss {e_l:.3f}, grad {e_g:.3f} of the bound")
    assert e_l <= 1 and e_g <= 1
    assert float(loss.detach()[0]) == 0.0    # the empty ray
    # batched (N, S) without ray indices: the same samples as rows
    wb, tb = R.dense_case(5, 65, offset, gen)
    d = torch.cat([tb[:, 1:] - tb[:, :-1], tb[:, -1:] - tb[:, -2:-1]], 1)
    st = torch.arange(5) * 65
    ref_b, _ = R.packed(wb.reshape(-1), tb.reshape(-1), (tb + d).reshape(-1), st, torch.full((5,), 65))
    got_b = nerfacc.distortion(wb, tb, tb + d)
    assert got_b.shape == (5,) and _rel(got_b, ref_b, ref_b.abs()) <= 1
    # dense: the compositing's own intervals
    for N, S in ((37, 2), (3, 65), (2, 1000)):
        wv, t = R.dense_case(N, S, offset, gen)
        ref_l, ref_g = R.dense(wv, t)
        wl = wv.clone().requires_grad_(True)
        loss = distortion_loss(wl, t, reduction="none")
        loss.sum().backward()
        e_l = _rel(loss.detach(), ref_l, ref_l.abs())
        e_g = _rel(wl.grad, ref_g, ref_g.abs().amax(1, keepdim=True))
        print(f"offset {offset}: dense ({N}, {S}) loss {e_l:.3f}, grad {e_g:.3f} of the bound")
        assert e_l <= 1 and e_g <= 1
    # reductions are torch's
    assert torch.equal(distortion_loss(wv, t, reduction="mean"), distortion_loss(wv, t, reduction="none").mean())
    assert torch.equal(distortion_loss(wv, t, reduction="sum"), distortion_loss(wv, t, reduction="none").sum())
    # float64 inputs stay float64
    assert distortion_loss(wv.double(), t.double()).dtype == torch.float64


def test_zero_ray_scale_gives_exact_zeros_even_with_nan_t():
    from adaptive_city_nerf_amd import distortion_loss
    gen = torch.Generator().manual_seed(4)
    w, t = R.dense_case(6, 40, 100.0, gen)
    rays = torch.zeros(6, 8)
    rays[:, 6], rays[:, 7] = t[:, 0], t[:, -1]
    rays[2, 6:] = float("nan")           # an invalid ray
    rays[4, 7] = rays[4, 6]              # far == near
    t[2] = float("nan")
    wl = w.clone().requires_grad_(True)
    loss = distortion_loss(wl, t, rays=rays, reduction="none")
    loss.sum().backward()
    assert float(loss.detach()[2]) == 0.0 and float(loss.detach()[4]) == 0.0
    assert bool((wl.grad[2] == 0).all()) and bool((wl.grad[4] == 0).all())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(wl.grad).all())
    scale = 1.0 / (rays[:, 7] - rays[:, 6])
    scale[2] = scale[4] = 0.0
    ref_l, ref_g = R.dense(w, torch.nan_to_num(t), scale)
    assert _rel(loss.detach(), ref_l, ref_l.abs()) <= 1
    assert _rel(wl.grad, ref_g, ref_g.abs().amax(1, keepdim=True)) <= 1
    assert float(distortion_loss(w, t, rays=rays)) == float(loss.detach().mean())


def test_second_order_takes_the_twice_differentiable_form():
    from adaptive_city_nerf_amd import distortion_loss
    from adaptive_city_nerf_amd.ray_rendering import second_order
    gen = torch.Generator().manual_seed(6)
    w, t = R.dense_case(2, 12, 0.0, gen)
    wl = (w + 0.05).requires_grad_(True)
    with second_order():
        loss = distortion_loss(wl, t, reduction="sum")
        g, = torch.autograd.grad(loss, wl, create_graph=True)
        h, = torch.autograd.grad(g[0, 3], wl)
    m, d = R.dense_intervals(t)
    ref = 2.0 * (m[0, 3] - m[0]).abs()        # d2 L / dw_3 dw_j = 2 |m_3 - m_j| (+ 2/3 d_3 at j = 3)
    ref[3] += 2.0 * d[0, 3] / 3.0
    assert float((h[0].double() - ref).abs().max()) <= 1e-6 * float(ref.max()) and bool((h[1] == 0).all())


def _last_error(L):
    buf = C.create_string_buffer(512)
    L.lib().acn_last_error(buf, 512)
    return buf.value.decode()


def test_bad_shapes_are_refused_before_any_hip_call():
    """CPU tensors and NULL pointers stand in: a refusal that came after a launch would report a HIP error."""
    from adaptive_city_nerf_amd import _lib as L
    from adaptive_city_nerf_amd import distortion_loss, nerfacc, occ_ops, ops
    from adaptive_city_nerf_amd.ray_rendering import render_rays
    w, t = torch.rand(4, 8), torch.rand(4, 8).sort(1).values
    for bad in (lambda: ops.distortion_dense(w[:, :1], t[:, :1]), lambda: ops.distortion_dense(w, t[:, :7]),
                lambda: ops.distortion_dense(w[0], t[0]), lambda: distortion_loss(w[:, :1], t[:, :1]),
                lambda: distortion_loss(w, t[:3]), lambda: distortion_loss(w, t, rays=torch.zeros(3, 8)),
                lambda: distortion_loss(w, t, rays=torch.zeros(4, 6)),
                lambda: occ_ops.distortion_packed(w, t, t, torch.zeros(1), torch.zeros(1)),
                lambda: occ_ops.distortion_packed(w[0], t[0], t[0, :7], torch.zeros(1), torch.zeros(1)),
                lambda: occ_ops.distortion_packed(w[0], t[0], t[0], torch.zeros(2), torch.zeros(1)),
                lambda: nerfacc.distortion(w, t, t[:, :7]), lambda: nerfacc.distortion(w[None], t[None], t[None]),
                lambda: nerfacc.distortion(w, t, t, ray_indices=torch.zeros(4, dtype=torch.long)),
                lambda: nerfacc.distortion(w, t, t, n_rays=5),
                lambda: nerfacc.distortion(w[0], t[0], t[0], ray_indices=torch.zeros(7, dtype=torch.long))):
        with pytest.raises(L.AcnError) as e:
            bad()
        assert "HIP device" not in str(e.value)
    with pytest.raises(ValueError):
        distortion_loss(w, t, reduction="max")
    # the shape is right, the device is not: the HIP entry itself has no CPU form
    with pytest.raises(L.AcnError, match="HIP device"):
        ops.distortion_dense(w, t)
    with pytest.raises(L.AcnError, match="HIP device"):
        occ_ops.distortion_packed(w[0], t[0], t[0], torch.zeros(1, dtype=torch.long), torch.full((1,), 8))
    lib = L.lib()
    assert lib.acn_distortion_dense(None, None, 4, 1, None, None, None, None) == -1 and "S >= 2" in _last_error(L)
    assert lib.acn_distortion_dense(None, None, -1, 8, None, None, None, None) == -1
    assert lib.acn_distortion_dense(None, None, 4, 8, None, None, None, None) == -1 and "NULL" in _last_error(L)
    assert lib.acn_distortion_dense(None, None, 0, 8, None, None, None, None) == 0       # nothing launched
    assert lib.acn_distortion_packed(None, None, None, 0, None, None, -1, None, None, None, None) == -1
    assert lib.acn_distortion_packed(None, None, None, 8, None, None, 2, None, None, None, None) == -1
    assert lib.acn_distortion_packed(None, None, None, 8, None, None, 0, None, None, None, None) == 0
    # the occupancy renderer has no (N, S) t values
    occ_model = type("M", (), {"use_occ": True, "occ_ready": True, "warned_occ_ready": True})()
    with pytest.raises(L.AcnError, match="nerfacc.distortion"):
        render_rays(occ_model, torch.zeros(2, 8), ray_samples=4, return_t_vals=True)


def test_new_names_are_exported():
    import inspect
    import adaptive_city_nerf_amd as A
    from adaptive_city_nerf_amd import nerfacc, occ_ops, ops, train
    assert callable(A.distortion_loss) and A.distortion_loss is A.ray_rendering.distortion_loss
    assert "distortion" in nerfacc.__all__
    assert list(inspect.signature(nerfacc.distortion).parameters) == ["weights", "t_starts", "t_ends", "ray_indices",
                                                                      "n_rays"]
    assert callable(ops.distortion_dense) and callable(occ_ops.distortion_packed)
    assert "return_t_vals" in inspect.signature(A.render_rays_stratified).parameters
    for fn in (train.compute_loss, train.adapt_step, train.GraphedAdaptStep.__init__, train.runtime_adapt):
        assert inspect.signature(fn).parameters["distortion_weight"].default == 0.0
    with pytest.raises(ValueError, match="expert-parallel"):
        train.adapt_step(None, None, None, None, None, group=object(), distortion_weight=0.1)
