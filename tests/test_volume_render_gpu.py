"""volume_render on the GPU (acn_volume_render_fwd / acn_volume_render_bwd: vr_fwd_ray, vr_bwd_ray, composite_tile in
csrc/render.hip) against the float64 reference of tests/volume_render_ref.py, at sample counts below, at and above one
and two 32-sample tiles, on rays that keep weight on every tile and on the last sample.

The tolerances are the project's: rgb and acc 1e-4, weights 1e-5, depth 1e-4 max|t| (README parity contract); per
channel of g_rgb_sigma 2e-5 of the reference channel's maximum, g_bg rtol 1e-5 / atol 1e-6 (tests/test_train.py).
tests/test_volume_render_cpu.py shows that each mistake these tests are there for moves a result by >= 100 of them.
Every test prints its observed maxima, as fractions of the tolerance."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import volume_render_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAW = [(False, False), (True, False), (False, True), (True, True)]
SCALES = (1.0, 2.0)
NAMES = ("rgb", "depth", "weights", "acc")


@lru_cache(maxsize=None)
def _case(shape):
    """CPU inputs of a shape, made once and never modified."""
    (rs, t), (bg, grads) = R.rows(*shape), R.extras(*shape)
    return rs, t, bg, grads


@lru_cache(maxsize=None)
def _inputs(shape, raw_rgb, raw_sigma):
    rs, t, _, _ = _case(shape)
    return R.raw_inputs(rs, t, raw_rgb, raw_sigma) if (raw_rgb or raw_sigma) else rs


@lru_cache(maxsize=None)
def _reference(shape, raw_rgb, raw_sigma, scale, with_bg, subset):
    """(outputs, g_rgb_sigma, g_bg) of the float64 reference, computed once per case."""
    _, t, bg, grads = _case(shape)
    return R.autograd(_inputs(shape, raw_rgb, raw_sigma), t, bg if with_bg else None, raw_rgb, raw_sigma, scale,
                      R.subset(grads, subset))


def _dev(x):
    return None if x is None else x.to(DEV)


def _fmt(worst):
    return ", ".join(f"{k} {v:.4f}" for k, v in worst.items())


def _track(worst, names, values):
    for k, v in zip(names, values):
        worst[k] = max(worst.get(k, 0.0), v)


def _check_backward(worst, got_rs, got_bg, ref_rs, ref_bg, what):
    errs = R.grad_errors(got_rs, ref_rs)
    _track(worst, ("g_r", "g_g", "g_b", "g_sigma"), errs)
    assert max(errs) <= 1.0, (what, errs)
    assert (got_bg is None) == (ref_bg is None), what
    if ref_bg is not None:
        e = R.bg_error(got_bg, ref_bg)
        _track(worst, ("g_bg",), (e,))
        assert e <= 1.0, (what, e)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_forward_matches_the_reference(shape):
    from adaptive_city_nerf_amd import ops
    _, t, bg, _ = _case(shape)
    worst = {}
    for raw_rgb, raw_sigma in RAW:
        x = _dev(_inputs(shape, raw_rgb, raw_sigma))
        for scale in SCALES:
            for with_bg in (True, False):
                got = ops.volume_render(x, _dev(t), _dev(bg) if with_bg else None, raw_rgb=raw_rgb,
                                        raw_sigma=raw_sigma, sigma_scale=scale)
                ref = _reference(shape, raw_rgb, raw_sigma, scale, with_bg, "all")[0]
                assert all(g.dtype == torch.float32 and g.shape == r.shape for g, r in zip(got, ref))
                errs = R.forward_errors(got, ref, t)
                _track(worst, NAMES, errs)
                assert max(errs) <= 1.0, (raw_rgb, raw_sigma, scale, with_bg, dict(zip(NAMES, errs)))
    print(f"forward {shape}, of the tolerance: {_fmt(worst)}")


@pytest.mark.parametrize("shape", R.SHAPES)
def test_backward_matches_the_reference(shape):
    """ops.volume_render_bwd directly and volume_render through autograd (_VolumeRenderFn); the output gradients
    outside the subset are None, which the kernel receives as NULL."""
    from adaptive_city_nerf_amd import ops
    from adaptive_city_nerf_amd.ray_rendering import volume_render
    rs, t, bg, grads = _case(shape)
    rs_d, t_d, bg_d, grads_d = _dev(rs), _dev(t), _dev(bg), tuple(_dev(g) for g in grads)
    worst = {}
    for subset, picked in R.GRAD_SUBSETS.items():
        gs = R.subset(grads_d, subset)
        for scale in SCALES:
            for with_bg in (True, False):
                what = (subset, scale, with_bg)
                _, ref_rs, ref_bg = _reference(shape, False, False, scale, with_bg, subset)
                g_rs, g_bg = ops.volume_render_bwd(rs_d, t_d, bg_d if with_bg else None, scale, *gs)
                _check_backward(worst, g_rs, g_bg, ref_rs, ref_bg, ("direct",) + what)
                x = rs_d.clone().requires_grad_(True)
                b = bg_d.clone().requires_grad_(True) if with_bg else None
                out = volume_render(x, t_d, bg_rgb=b, sigma_scale=scale)
                assert "_VolumeRenderFn" in type(out[0].grad_fn).__name__
                torch.autograd.backward([out[i] for i in picked], [grads_d[i] for i in picked])
                _check_backward(worst, x.grad, None if b is None else b.grad, ref_rs, ref_bg, ("autograd",) + what)
                assert torch.equal(x.grad, g_rs) and (b is None or torch.equal(b.grad, g_bg)), what
    print(f"backward {shape}, of the tolerance: {_fmt(worst)}")


@pytest.mark.parametrize("shape", R.SHAPES)
def test_dispatcher_paths_meet_the_same_bounds(shape):
    """With gradients enabled, raw flags or second_order() send GPU tensors to the composed torch form; float64 inputs
    without grad come back float64 from the kernel."""
    from adaptive_city_nerf_amd import ray_rendering as RR
    _, t, bg, grads = _case(shape)
    t_d, grads_d = _dev(t), [_dev(g) for g in grads]
    worst = {}
    cases = [(raw_rgb, raw_sigma, False) for raw_rgb, raw_sigma in RAW[1:]] + [(False, False, True)]
    for raw_rgb, raw_sigma, second in cases:
        for scale, with_bg in ((2.0, True), (1.0, False)):
            what = (raw_rgb, raw_sigma, second, scale, with_bg)
            ref_out, ref_rs, ref_bg = _reference(shape, raw_rgb, raw_sigma, scale, with_bg, "all")
            x = _dev(_inputs(shape, raw_rgb, raw_sigma)).clone().requires_grad_(True)
            b = _dev(bg).clone().requires_grad_(True) if with_bg else None
            with RR.second_order(second):
                out = RR.volume_render(x, t_d, bg_rgb=b, raw_rgb=raw_rgb, raw_sigma=raw_sigma, sigma_scale=scale)
            assert "_VolumeRenderFn" not in type(out[0].grad_fn).__name__, what
            errs = R.forward_errors([o.detach() for o in out], ref_out, t)
            _track(worst, NAMES, errs)
            assert max(errs) <= 1.0, (what, errs)
            torch.autograd.backward(out, grads_d)
            _check_backward(worst, x.grad, None if b is None else b.grad, ref_rs, ref_bg, what)
    print(f"composed torch path {shape}, of the tolerance: {_fmt(worst)}")
    worst = {}
    for raw_rgb, raw_sigma in RAW:
        x = _dev(_inputs(shape, raw_rgb, raw_sigma)).double()
        with torch.no_grad():
            out = RR.volume_render(x, t_d.double(), bg_rgb=_dev(bg).double(), raw_rgb=raw_rgb, raw_sigma=raw_sigma)
        assert all(o.dtype == torch.float64 and o.is_cuda for o in out)
        errs = R.forward_errors(out, _reference(shape, raw_rgb, raw_sigma, 1.0, True, "all")[0], t)
        _track(worst, NAMES, errs)
        assert max(errs) <= 1.0, (raw_rgb, raw_sigma, errs)
    print(f"float64 in, no grad {shape}, of the tolerance: {_fmt(worst)}")


def test_grid_stride_loops():
    """More rays than one pass of the grid holds: the forward caps at 4096 workgroups of 4 rays, the backward at
    8192.  All rows are compared."""
    from adaptive_city_nerf_amd import ops
    worst = {}
    shape = (16384 + 5, 3)
    rs, t, bg, grads = _case(shape)
    got = ops.volume_render(_dev(rs), _dev(t), _dev(bg))
    errs = R.forward_errors(got, _reference(shape, False, False, 1.0, True, "all")[0], t)
    _track(worst, NAMES, errs)
    assert max(errs) <= 1.0, errs
    shape = (32768 + 5, 3)
    rs, t, bg, grads = _case(shape)
    _, ref_rs, ref_bg = _reference(shape, False, False, 1.0, True, "all")
    g_rs, g_bg = ops.volume_render_bwd(_dev(rs), _dev(t), _dev(bg), 1.0, *[_dev(g) for g in grads])
    _check_backward(worst, g_rs, g_bg, ref_rs, ref_bg, shape)
    assert float(np.abs(ref_rs[32768:, :, 3]).max()) > 0      # the rays of the second pass have something to miss
    print(f"grid-stride, of the tolerance: {_fmt(worst)}")


def test_rays_are_isolated_and_runs_repeat():
    """A NaN density (row 4) and the invalid-ray convention t = +inf (row 9) spoil those rays only: every other row is
    bit-identical to a run without them, forward and backward, and two identical calls return identical bits."""
    from adaptive_city_nerf_amd import ops
    shape = (37, 33)
    rs, t, bg, grads = _case(shape)
    bad_rs, bad_t = rs.clone(), t.clone()
    bad_rs[4, :, 3] = float("nan")
    bad_t[9] = float("inf")
    bg_d, grads_d = _dev(bg), [_dev(g) for g in grads]
    clean_f = ops.volume_render(_dev(rs), _dev(t), bg_d)
    clean_b = ops.volume_render_bwd(_dev(rs), _dev(t), bg_d, 1.0, *grads_d)
    bad_f = ops.volume_render(_dev(bad_rs), _dev(bad_t), bg_d)
    bad_b = ops.volume_render_bwd(_dev(bad_rs), _dev(bad_t), bg_d, 1.0, *grads_d)
    again_f = ops.volume_render(_dev(bad_rs), _dev(bad_t), bg_d)
    again_b = ops.volume_render_bwd(_dev(bad_rs), _dev(bad_t), bg_d, 1.0, *grads_d)
    keep = torch.ones(shape[0], dtype=torch.bool, device=DEV)
    keep[[4, 9]] = False
    for name, a in zip(NAMES, bad_f):
        assert bool(torch.isnan(a[[4, 9]]).all()), name
    for a, b, c in zip(bad_f + bad_b, clean_f + clean_b, again_f + again_b):
        assert torch.equal(a[keep], b[keep]) and bool(torch.isfinite(a[keep]).all())
        assert np.array_equal(a.cpu().numpy(), c.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("shape", [(13, 65), (1, 2)])
def test_c_entries_write_inside_their_outputs(shape):
    """The two C entries on weights / g_rgb_sigma buffers with 64 sentinel floats on either side of the payload."""
    from adaptive_city_nerf_amd import _lib, ops
    from adaptive_city_nerf_amd._lib import check, ptr, stream_of
    N, S = shape
    pad, sentinel = 64, -777.25
    rs, t, bg, grads = _case(shape)
    rs, t, bg, grads = _dev(rs), _dev(t), _dev(bg), [_dev(g) for g in grads]
    ref_f = ops.volume_render(rs, t, bg)
    ref_rs, ref_bg = ops.volume_render_bwd(rs, t, bg, 1.0, *grads)
    L = _lib.lib()
    w = torch.full((pad + N * S + pad,), sentinel, device=DEV)
    rgb, depth, acc = torch.empty(N, 3, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    check(L.acn_volume_render_fwd(ptr(rs), ptr(t), ptr(bg), N, S, 0, 0, 1.0, ptr(rgb), ptr(depth),
                                  w.data_ptr() + 4 * pad, ptr(acc), stream_of(rs)), "acn_volume_render_fwd")
    g = torch.full((pad + N * S * 4 + pad,), sentinel, device=DEV)
    g_bg = torch.empty(N, 3, device=DEV)
    check(L.acn_volume_render_bwd(ptr(rs), ptr(t), ptr(bg), N, S, 1.0, *[ptr(x) for x in grads],
                                  g.data_ptr() + 4 * pad, ptr(g_bg), stream_of(rs)), "acn_volume_render_bwd")
    torch.cuda.synchronize()
    for buf, payload in ((w, ref_f[2]), (g, ref_rs)):
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[-pad:] == sentinel).all())
        assert torch.equal(buf[pad:-pad], payload.reshape(-1))
    assert torch.equal(rgb, ref_f[0]) and torch.equal(depth, ref_f[1]) and torch.equal(acc, ref_f[3])
    assert torch.equal(g_bg, ref_bg)


def test_arguments():
    from adaptive_city_nerf_amd import ops
    from adaptive_city_nerf_amd._lib import AcnError
    S = 5
    out = ops.volume_render(torch.empty(0, S, 4, device=DEV), torch.empty(0, S, device=DEV),
                            torch.empty(0, 3, device=DEV))
    assert [tuple(o.shape) for o in out] == [(0, 3), (0,), (0, S), (0,)]
    g_rs, g_bg = ops.volume_render_bwd(torch.empty(0, S, 4, device=DEV), torch.empty(0, S, device=DEV),
                                       torch.empty(0, 3, device=DEV), 1.0, torch.empty(0, 3, device=DEV), None, None,
                                       None)
    assert tuple(g_rs.shape) == (0, S, 4) and tuple(g_bg.shape) == (0, 3)
    torch.cuda.synchronize()
    rs, t = torch.rand(3, 1, 4, device=DEV), torch.rand(3, 1, device=DEV)
    with pytest.raises(AcnError, match=r"acn_volume_render_fwd: need N >= 0 and S >= 2 \(got S=1\)"):
        ops.volume_render(rs, t)
    with pytest.raises(AcnError, match=r"acn_volume_render_bwd: need N >= 0 and S >= 2 \(got S=1\)"):
        ops.volume_render_bwd(rs, t, None, 1.0, torch.rand(3, 3, device=DEV), None, None, None)
    # the refusals launched nothing and left no error behind
    rs, t, bg, _ = _case((5, 3))
    ops.volume_render(_dev(rs), _dev(t), _dev(bg))
    torch.cuda.synchronize()
