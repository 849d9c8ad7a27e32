"""Host-side checks of the SSIM metric, no GPU needed: the package's float64 torch form agrees with the
direct definition of tests/ssim_ref.py and passes gradcheck; closed forms; reductions and layouts; image_metrics' PSNR is
parallel.psnr_reduce's formula; acn_ssim_fwd refuses bad arguments before any HIP call; the new names are exported."""
import ctypes as C
import math

import pytest
import torch

import ssim_ref as R


def test_torch_form_agrees_with_the_definition_and_the_two_references_agree():
    from adaptive_city_nerf_amd.metrics import _ssim_torch
    for i, shape in enumerate([(1, 3, 11, 11), (2, 3, 43, 75), (1, 1, 64, 53)]):
        X, Y = (t.double() for t in R.images(shape, 10 + i))
        ref = R.ssim_nc(X, Y)
        got = _ssim_torch(X, Y, 11, 1.5, R.C1, R.C2)
        e, e2 = float((got - ref).abs().max()), float((R.ssim_nc_unfold(X, Y) - ref).abs().max())
        print(f"{shape}: |_ssim_torch - definition| = {e:.2e}, |unfold form - definition| = {e2:.2e}")
        assert got.shape == shape[:2] and got.dtype == torch.float64
        assert e <= 1e-12 and e2 <= 1e-13
    # other windows
    X, Y = (t.double() for t in R.images((1, 2, 20, 23), 3))
    for win, sigma in ((3, 0.8), (7, 1.5), (13, 2.0)):
        assert float((_ssim_torch(X, Y, win, sigma, R.C1, R.C2) - R.ssim_nc(X, Y, win, sigma)).abs().max()) <= 1e-12


def test_torch_form_passes_gradcheck_and_is_twice_differentiable():
    from adaptive_city_nerf_amd import ssim
    from adaptive_city_nerf_amd.ray_rendering import second_order
    X, Y = (t.double().requires_grad_(True) for t in R.images((1, 2, 12, 13), 5))
    assert torch.autograd.gradcheck(lambda a, b: ssim(a, b, size_average=False), (X, Y), eps=1e-6, atol=1e-7)
    gx_ref, gy_ref = R.grads(X, Y)
    gx, gy = torch.autograd.grad(ssim(X, Y, size_average=False).sum(), (X, Y))
    assert float((gx - gx_ref / 2).abs().max()) <= 1e-12 and float((gy - gy_ref / 2).abs().max()) <= 1e-12   # mean of C = 2
    with second_order():
        g, = torch.autograd.grad(ssim(X, Y), X, create_graph=True)
        h, = torch.autograd.grad(g.pow(2).sum(), X)
    assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0


def test_closed_forms():
    from adaptive_city_nerf_amd import ssim
    X, _ = R.images((2, 3, 30, 17), 7)
    assert float(ssim(X, X)) == 1.0 and float(ssim(X.double(), X.double())) == 1.0
    assert bool((ssim(X, X, size_average=False) == 1.0).all())
    black, white = torch.zeros(1, 1, 12, 13, dtype=torch.float64), torch.ones(1, 1, 12, 13, dtype=torch.float64)
    v = float(ssim(black, white))
    assert abs(v - R.C1 / (1 + R.C1)) <= 1e-12 and abs(v - 9.999000099990e-5) <= 1e-12
    U = torch.rand(1, 1, 20, 20, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    neg = float(ssim(U, 1 - U))
    print(f"ssim(U, 1 - U) = {neg:.4f}")
    assert neg < 0 and abs(neg - float(R.ssim_nc(U, 1 - U).mean())) <= 1e-12
    assert float(ssim(U, 1 - U, nonnegative_ssim=True)) == 0.0
    # data_range scales C1 and C2: 8-bit images give the value of their [0, 1] form
    X8, Y8 = (t.double() for t in R.images((1, 1, 16, 16), 9))
    assert abs(float(ssim(X8 * 255, Y8 * 255, data_range=255.0)) - float(ssim(X8, Y8))) <= 1e-12


def test_reductions_shapes_and_the_frame_layout():
    from adaptive_city_nerf_amd import ssim, ssim_image
    X, Y = R.images((3, 3, 21, 19), 11)
    ref = R.ssim_nc(X, Y)
    per_image, scalar = ssim(X, Y, size_average=False), ssim(X, Y)
    assert per_image.shape == (3,) and scalar.shape == () and per_image.dtype == torch.float32
    assert float((per_image.double() - ref.mean(1)).abs().max()) <= 2.0 ** -23
    assert abs(float(scalar) - float(ref.mean())) <= 2.0 ** -23
    frame_x, frame_y = X[0].permute(1, 2, 0).contiguous(), Y[0].permute(1, 2, 0).contiguous()
    assert torch.equal(ssim_image(frame_x, frame_y), ssim(X[:1], Y[:1]))
    assert ssim_image(frame_x, frame_y, size_average=False).shape == (1,)
    assert torch.equal(ssim_image(frame_x, frame_y, win_size=7, win_sigma=1.0), ssim(X[:1], Y[:1], win_size=7,
                                                                                     win_sigma=1.0))


def test_bad_arguments_raise():
    from adaptive_city_nerf_amd import image_metrics, ops, ssim, ssim_image
    from adaptive_city_nerf_amd._lib import AcnError
    X = torch.rand(1, 3, 16, 16)
    for bad in (lambda: ssim(X, X[:, :2]), lambda: ssim(X[0], X[0]), lambda: ssim(X, X, win_size=4),
                lambda: ssim(X, X, win_sigma=0.0), lambda: ssim(X[:, :, :10], X[:, :, :10]),
                lambda: ssim(X[..., :10], X[..., :10]), lambda: ssim_image(X, X),
                lambda: ssim_image(X[0, :, :10].permute(1, 2, 0), X[0, :, :10].permute(1, 2, 0)),
                lambda: image_metrics(X[0], X[0, :2]),
                lambda: ops.ssim_fwd(X, X, win_size=13, c1=R.C1, c2=R.C2),
                lambda: ops.ssim_fwd(X, X[:, :2], c1=R.C1, c2=R.C2),
                lambda: ops.ssim_fwd(X[..., :10], X[..., :10], c1=R.C1, c2=R.C2)):
        with pytest.raises(AcnError) as e:
            bad()
        assert "HIP device" not in str(e.value)
    with pytest.raises(AcnError, match="HIP device"):    # the shape is right, the device is not
        ops.ssim_fwd(X, X, c1=R.C1, c2=R.C2)


@pytest.mark.parametrize("space", ["linear", "srgb", "identity"])
def test_image_metrics_psnr_is_psnr_reduce_formula(space):
    from adaptive_city_nerf_amd import image_metrics, ssim_image
    from adaptive_city_nerf_amd.color_space import color_space_transformer, linear_to_srgb, srgb_to_linear
    from adaptive_city_nerf_amd.parallel import local_sse, psnr_reduce
    gen = torch.Generator().manual_seed(13)
    gt = torch.rand(24, 40, 3, generator=gen)
    pred = (srgb_to_linear(gt) + 0.05 * torch.randn(24, 40, 3, generator=gen))   # leaves [0, 1] in places
    if space == "identity":
        pred = pred.clamp(0, 1)
    m = image_metrics(pred, gt, space)
    assert set(m) == {"psnr", "ssim"} and all(isinstance(v, float) for v in m.values())
    assert m["psnr"] == psnr_reduce(*local_sse(pred, gt, space), "cpu")
    p, g = color_space_transformer(pred, gt, space)
    assert m["ssim"] == float(ssim_image(p, g)) and 0 < m["ssim"] < 1
    # identical images: the 1e-8 clamp (80 dB) and an SSIM of exactly 1
    lin = srgb_to_linear(gt)
    same = {"linear": lambda: image_metrics(lin, gt, "linear"), "srgb": lambda: image_metrics(lin, linear_to_srgb(lin), "srgb"),
            "identity": lambda: image_metrics(gt, gt, "identity")}[space]()
    assert same["psnr"] == -10.0 * math.log10(1e-8) and abs(same["psnr"] - 80.0) < 1e-9 and same["ssim"] == 1.0


def _last_error(L):
    buf = C.create_string_buffer(512)
    L.lib().acn_last_error(buf, 512)
    return buf.value.decode()


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """Host buffers stand in for device pointers: a refusal that came after a launch would report a HIP error."""
    from adaptive_city_nerf_amd import _lib as L
    lib = L.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    big = lib.acn_ssim_workspace_bytes(1, 3, 16, 16, 1)

    def call(x=p, y=p, N=1, Cn=3, H=16, W=16, cl=0, win=11, sigma=1.5, out=p, grad=None, ws=p, ws_bytes=big):
        return lib.acn_ssim_fwd(x, y, N, Cn, H, W, cl, win, sigma, R.C1, R.C2, out, grad, ws, ws_bytes, None)

    for kw, word in ((dict(H=10), "H and W"), (dict(W=10), "H and W"), (dict(win=4), "win_size"),
                     (dict(win=13), "win_size"), (dict(win=1), "win_size"), (dict(sigma=0.0), "win_sigma"),
                     (dict(sigma=-1.0), "win_sigma"), (dict(Cn=0), "C >= 1"), (dict(N=-1), "N must be"),
                     (dict(x=None), "NULL"), (dict(y=None), "NULL"), (dict(out=None), "NULL"), (dict(ws=None), "NULL"),
                     (dict(ws_bytes=0), "workspace"), (dict(grad=p, ws_bytes=big // 2), "workspace")):
        assert call(**kw) == -1, kw
        assert word in _last_error(L), (kw, _last_error(L))
    assert call(N=0) == 0 and call(N=0, x=None, y=None, out=None, ws=None, ws_bytes=0) == 0    # nothing launched
    # the workspace: 8 B per tile, 24 B per map pixel more with the gradient; it grows with the image
    no_grad, with_grad = lib.acn_ssim_workspace_bytes(2, 3, 100, 70, 0), lib.acn_ssim_workspace_bytes(2, 3, 100, 70, 1)
    assert 0 < no_grad < with_grad and with_grad - no_grad >= 24 * 6 * 90 * 60
    assert lib.acn_ssim_workspace_bytes(2, 3, 200, 70, 1) > with_grad


def test_new_names_are_exported():
    import inspect
    import adaptive_city_nerf_amd as A
    from adaptive_city_nerf_amd import metrics, ops, parallel
    for n in ("ssim", "ssim_image", "image_metrics", "evaluate_image"):
        assert getattr(A, n) is getattr(metrics, n) and n in metrics.__all__
    assert list(inspect.signature(A.ssim).parameters) == ["X", "Y", "data_range", "size_average", "win_size",
                                                          "win_sigma", "K", "nonnegative_ssim"]
    d = {k: v.default for k, v in inspect.signature(A.ssim).parameters.items()}
    assert (d["data_range"], d["size_average"], d["win_size"], d["win_sigma"], d["K"], d["nonnegative_ssim"]) == \
        (1.0, True, 11, 1.5, (0.01, 0.03), False)
    assert ops.SSIM_TILE_H >= 1 and ops.SSIM_TILE_W >= 1 and callable(ops.ssim_fwd)
    assert "UNPINNED" in metrics.__doc__ and "image_metrics" in parallel.render_image_sharded.__doc__
