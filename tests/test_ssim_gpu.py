"""The fused SSIM on the GPU (acn_ssim_fwd) against the float64 definition of tests/ssim_ref.py, and its
way up: ops.ssim_fwd in both layouts, autograd through metrics.ssim, image_metrics and evaluate_image.

The kernel computes in float64 on the fp32 pixels and rounds each output to fp32 once; its arithmetic differs from the
reference's only in summation order (about 1e-15).  So per image and channel |got - ref| <= 4 * 2^-24 * |ref| + 1e-30 for
the value and, element by element, 4 * 2^-24 * (the plane's largest |ref|) + 1e-30 for the gradient: one fp32 rounding
against a bound of four.  The worst ratio to the bound is printed."""
from functools import lru_cache

import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 4 * 2.0 ** -24


def _tiles():
    from adaptive_city_nerf_amd import ops
    return ops.SSIM_TILE_H, ops.SSIM_TILE_W


def _shapes():
    Th, Tw = _tiles()
    return [(1, 1, 11, 11),                                   # one map pixel
            (1, 3, 11, 12), (1, 3, 12, 11),
            (1, 1, Th + 10, Tw + 10),                         # exactly one tile
            (2, 3, Th + 11, Tw + 10), (2, 3, Th + 10, Tw + 11),   # one row / one column into a second tile
            (1, 3, 2 * Th + 10 + 5, 3 * Tw + 10 + 7),         # whole tiles plus ragged edges both ways
            (3, 1, 13, 75)]


RAGGED = 6   # index of the ragged multi-tile shape


@lru_cache(maxsize=None)
def _case(shape, win=11, sigma=1.5, seed=0):
    """CPU inputs and the float64 reference (value, gradients in X and Y); computed once, never modified."""
    X, Y = R.images(shape, 1000 + seed + sum(shape) + win)
    gx, gy = R.grads(X, Y, win, sigma)
    return X, Y, R.ssim_nc(X, Y, win, sigma), gx, gy


def _value_ratio(got, ref):
    return float(((got.detach().double().cpu() - ref).abs() / (BOUND * ref.abs() + 1e-30)).max())


def _grad_ratio(got, ref):
    plane_max = ref.abs().amax((2, 3), keepdim=True)
    return float(((got.detach().double().cpu() - ref).abs() / (BOUND * plane_max + 1e-30)).max())


def _layout(t, channels_last):
    return t.permute(0, 2, 3, 1).contiguous() if channels_last else t


def _unlayout(t, channels_last):
    return t.permute(0, 3, 1, 2) if channels_last else t


def _leaf(t):
    return t.to(DEV).clone().requires_grad_(True)


def _strided(t):
    """A non-contiguous view with t's values: every other element of the last dimension of a wider tensor."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device, dtype=t.dtype)
    wide[..., ::2] = t
    v = wide[..., ::2]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


@pytest.mark.parametrize("channels_last", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("idx", range(8))
def test_value_and_gradient_match_the_definition(idx, channels_last):
    from adaptive_city_nerf_amd import ops
    shape = _shapes()[idx]
    X, Y, ref, ref_gx, _ = _case(shape)
    x, y = _layout(X.to(DEV), channels_last), _layout(Y.to(DEV), channels_last)
    kw = dict(channels_last=channels_last, c1=R.C1, c2=R.C2)
    val, grad = ops.ssim_fwd(x, y, want_grad=True, **kw)
    assert val.shape == shape[:2] and val.dtype == torch.float32 and grad.shape == x.shape
    r_v, r_g = _value_ratio(val, ref), _grad_ratio(_unlayout(grad, channels_last), ref_gx)
    print(f"{shape} {'channels_last' if channels_last else 'planar'}: value at {r_v:.3f}, gradient at {r_g:.3f} of the "
          f"bound")
    assert r_v <= 1 and r_g <= 1
    # bitwise reproducible; the value does not depend on whether the gradient is written
    val2, grad2 = ops.ssim_fwd(x, y, want_grad=True, **kw)
    val3, none = ops.ssim_fwd(x, y, **kw)
    assert torch.equal(val, val2) and torch.equal(grad, grad2) and torch.equal(val, val3) and none is None
    # a non-contiguous view gives the bits of its contiguous copy
    val4, grad4 = ops.ssim_fwd(_strided(x), _strided(y), want_grad=True, **kw)
    assert torch.equal(val, val4) and torch.equal(grad, grad4)


def test_low_contrast_images_meet_the_same_bound():
    from adaptive_city_nerf_amd import ops
    gen = torch.Generator().manual_seed(40)
    X = 0.5 + 1e-3 * torch.rand(1, 3, 40, 40, generator=gen)
    Y = 0.5 + 1e-3 * torch.rand(1, 3, 40, 40, generator=gen)
    ref = R.ssim_nc(X, Y)
    val, _ = ops.ssim_fwd(X.to(DEV), Y.to(DEV), c1=R.C1, c2=R.C2)
    chain = R.ssim_fp32_conv(X.to(DEV), Y.to(DEV))
    ulps = lambda v: float(((v.double().cpu() - ref).abs() / (2.0 ** -24 * ref.abs())).max())   # noqa: E731
    r = _value_ratio(val, ref)
    print(f"low contrast (amplitude 1e-3 around 0.5): fused at {r:.3f} of the bound ({ulps(val):.2f} x 2^-24 |ref|); the "
          f"fp32 conv2d chain lands {ulps(chain):.1f} x 2^-24 |ref| away (printed only)")
    assert r <= 1


def test_exact_values():
    from adaptive_city_nerf_amd import ops, ssim
    shape = _shapes()[RAGGED]
    X = _case(shape)[0].to(DEV)
    for cl in (False, True):
        val, _ = ops.ssim_fwd(_layout(X, cl), _layout(X, cl), channels_last=cl, c1=R.C1, c2=R.C2)
        assert bool((val == 1.0).all()), val
    assert float(ssim(X, X)) == 1.0
    black, white = torch.zeros(1, 1, 12, 13, device=DEV), torch.ones(1, 1, 12, 13, device=DEV)
    val, _ = ops.ssim_fwd(black, white, c1=R.C1, c2=R.C2)
    ref = torch.tensor([[R.C1 / (1 + R.C1)]], dtype=torch.float64)
    assert _value_ratio(val, ref) <= 1 and _value_ratio(ssim(black, white).view(1, 1), ref) <= 1
    U = torch.rand(1, 1, 20, 20, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert float(ssim(U, 1 - U)) < 0 and float(ssim(U, 1 - U, nonnegative_ssim=True)) == 0.0


def test_autograd_in_both_images_matches_float64_autograd():
    from adaptive_city_nerf_amd import ssim, ssim_image
    shape = _shapes()[4]
    X, Y, ref, ref_gx, ref_gy = _case(shape)
    N, C = shape[:2]
    # the gradient in Y alone: a second launch with the images swapped
    y = _leaf(Y)
    ssim(X.to(DEV), y, size_average=False).sum().backward()
    r = _grad_ratio(y.grad, ref_gy / C)
    print(f"{shape}: d ssim / d Y at {r:.3f} of the bound")
    assert r <= 1
    # a scalar with a non-unit upstream gradient, both images
    x, y = _leaf(X), _leaf(Y)
    val = ssim(x, y)
    (3.0 * val).backward()
    # the fp32 mean of the N * C positive values: N * C - 1 sums and a division on top of the kernel's one rounding,
    # each within 2^-24 of the total, so N * C + 1 roundings where BOUND allows four
    r_v = _value_ratio(val.view(1, 1), ref.mean().view(1, 1)) * 4 / (N * C + 1)
    r_x, r_y = _grad_ratio(x.grad, 3.0 * ref_gx / (N * C)), _grad_ratio(y.grad, 3.0 * ref_gy / (N * C))
    print(f"{shape}: 3 * ssim: value at {r_v:.3f}, d / d X at {r_x:.3f}, d / d Y at {r_y:.3f} of the bound")
    assert r_v <= 1 and r_x <= 1 and r_y <= 1
    # per image, a vector upstream gradient
    up = torch.tensor([2.0, -0.5])   # exact factors: 1 / C, the product with the kept gradient and the kernel round
    x = _leaf(X)
    (ssim(x, Y.to(DEV), size_average=False) * up.to(DEV)).sum().backward()
    r = _grad_ratio(x.grad, ref_gx * (up.double() / C).view(N, 1, 1, 1))
    print(f"{shape}: per-image upstream gradient at {r:.3f} of the bound")
    assert r <= 1
    # (H, W, C) frames: the channels-last path behind autograd
    f = _leaf(_layout(X[:1], True)[0])
    ssim_image(f, _layout(Y[:1], True)[0].to(DEV)).backward()
    assert _grad_ratio(f.grad.permute(2, 0, 1)[None], ref_gx[:1] / C) <= 1


@pytest.mark.parametrize("win,sigma", [(3, 0.8), (7, 1.5)])
def test_smaller_windows(win, sigma):
    from adaptive_city_nerf_amd import ops
    Th, Tw = _tiles()
    shape = (1, 2, Th + win + 4, 2 * Tw + win + 2)
    X, Y, ref, ref_gx, _ = _case(shape, win, sigma)
    for cl in (False, True):
        val, grad = ops.ssim_fwd(_layout(X.to(DEV), cl), _layout(Y.to(DEV), cl), channels_last=cl, win_size=win,
                                 win_sigma=sigma, c1=R.C1, c2=R.C2, want_grad=True)
        r_v, r_g = _value_ratio(val, ref), _grad_ratio(_unlayout(grad, cl), ref_gx)
        print(f"win {win} {shape} {'channels_last' if cl else 'planar'}: value at {r_v:.3f}, gradient at {r_g:.3f} of "
              f"the bound")
        assert r_v <= 1 and r_g <= 1


def test_a_window_above_eleven_takes_the_torch_form():
    from adaptive_city_nerf_amd import ssim
    X, Y = R.images((1, 2, 40, 45), 13)
    ref = R.ssim_nc(X, Y, 13, 2.0)
    x = _leaf(X)
    got = ssim(x, Y.to(DEV), win_size=13, win_sigma=2.0, size_average=False)
    assert got.is_cuda and got.dtype == torch.float32
    assert float((got.detach().double().cpu() - ref.mean(1)).abs().max()) <= 1e-6
    got.sum().backward()
    assert _grad_ratio(x.grad, R.grads(X, Y, 13, 2.0)[0] / 2) <= 1


def test_evaluate_image_is_render_image_plus_image_metrics():
    import goldens as G
    import test_input_grad_gpu as T
    from adaptive_city_nerf_amd import evaluate_image, image_metrics, render_image
    from adaptive_city_nerf_amd.color_space import srgb_to_linear
    m, gbox = T._container("k4")
    cam = G.scene()["val_cam0"]
    intr = torch.tensor(cam["intrinsics"], dtype=torch.float32)
    H, W = 24, 40
    sx, sy = W / float(2.0 * intr[2]), H / float(2.0 * intr[3])
    kw = dict(H=H, W=W, fx=float(intr[0]) * sx, fy=float(intr[1]) * sy, cx=W / 2.0, cy=H / 2.0,
              c2w=torch.tensor(cam["c2w"]), scene_box=gbox, ray_samples=16)
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3))
    rgb, depth, acc, metrics = evaluate_image(m, gt_srgb=gt, **kw)
    rgb0, depth0, acc0 = render_image(m, **kw)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0) and torch.equal(acc, acc0)
    assert metrics == image_metrics(rgb0, gt.to(DEV)) and set(metrics) == {"psnr", "ssim"}
    assert -1.0 <= metrics["ssim"] < 1.0 and 0.0 < metrics["psnr"] < 80.0
    # the SSIM entry is the definition's, on the frame in the metric's colour space
    # (one rounding per channel, two fp32 sums and a division: four roundings of at most the channels' mean magnitude)
    g_lin = srgb_to_linear(gt.to(DEV)).clamp(0, 1)
    ref = R.ssim_nc(rgb0.permute(2, 0, 1)[None], g_lin.permute(2, 0, 1)[None])
    assert abs(metrics["ssim"] - float(ref.mean())) <= 2.0 ** -22 * float(ref.abs().mean()) + 1e-30
    for space in ("linear", "srgb"):
        assert evaluate_image(m, gt_srgb=gt, metrics_space=space, **kw)[3] == image_metrics(rgb0, gt, space)
    same = image_metrics(srgb_to_linear(gt.to(DEV)), gt.to(DEV))
    assert same["ssim"] == 1.0 and abs(same["psnr"] - 80.0) < 1e-9
