"""Camera-pose gradients and the fused frozen-field input backward on the GPU: acn_mlp_train_bwd_input against the
fused / split backwards it is a part of, the field's input gradient with the switch on against off,
acn_rays_from_dirs_bwd against its three formulas in float64, get_rays under autograd, and a pose step end to end.

Tolerances.  gh0: bit-equal (the same chain in the same order as acn_mlp_train_bwd_dw).  gsh: 2e-5 * max|ref| +
1e-9, the bound test_mlp_train_gpu.py puts on the weight gradients (fp16x3 keeps ~2^-22 per product).  Field:
2e-5 * max(1, max|ref|), the convention of test_input_grad_gpu.py.  rays_from_dirs_bwd: elementwise 1e-6 * B with B
the sum of the absolute terms -- products of two floats are exact in double, the double sum of <= 2^20 terms errs
below 1e-10 * B, the final rounding to float is <= 6e-8 * |result| (g_dirs: three float roundings, <= 2e-7 * B)."""
from contextlib import contextmanager
from functools import lru_cache

import pytest
import torch

import goldens as G
import test_input_grad_gpu as TI

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_BIG = 4200          # every MLP case is a prefix of one batch of this size
SIZES = [1, 31, 33, 4113]


def _ops():
    from adaptive_city_nerf_amd import ops
    return ops


@contextmanager
def _precision(mode):
    ops = _ops()
    old = ops.TRAIN_MLP_PRECISION
    ops.set_train_mlp_precision(mode)
    try:
        yield
    finally:
        ops.set_train_mlp_precision(old)


@contextmanager
def _input_grad_fused(on):
    from adaptive_city_nerf_amd.meta_ngp import _FusedMLPFn
    old = _FusedMLPFn.INPUT_GRAD_FUSED
    _FusedMLPFn.INPUT_GRAD_FUSED = on
    try:
        yield
    finally:
        _FusedMLPFn.INPUT_GRAD_FUSED = old


# ------------------------------------------------------------------------------------------------- MLP kernel
@lru_cache(maxsize=None)
def _mlp_inputs():
    """(ws, h0, sh, gout) of M_BIG rows: the weights and input ranges of test_fused_dw_matches_split_path; shared,
    never modified."""
    from test_mlp_train_gpu import _expert
    sub = _expert()
    ws = [t.detach().contiguous() for t in (
        sub.sigma_trunk[0].linear.weight, sub.sigma_trunk[0].linear.bias, sub.sigma_trunk[1].linear.weight,
        sub.sigma_trunk[1].linear.bias, sub.sigma_head.weight, sub.sigma_head.bias, sub.geo_head.weight,
        sub.geo_head.bias, sub.color_mlp[0].linear.weight, sub.color_mlp[0].linear.bias,
        sub.color_mlp[1].linear.weight, sub.color_mlp[1].linear.bias, sub.color_mlp[2].weight,
        sub.color_mlp[2].bias)]
    g = torch.Generator(device=DEV).manual_seed(4113)
    h0 = (torch.rand(M_BIG, 32, device=DEV, generator=g) - 0.5) * 2
    sh = (torch.rand(M_BIG, 16, device=DEV, generator=g) - 0.5) * 2
    gout = torch.randn(M_BIG, 4, device=DEV, generator=g)
    return ws, h0, sh, gout


@lru_cache(maxsize=None)
def _mlp_case(M, precision):
    """(h0, sh, out, gout, gh0, gsh) of the first M rows: one forward and one acn_mlp_train_bwd_input call."""
    ops = _ops()
    ws, h0, sh, gout = _mlp_inputs()
    h0, sh, gout = h0[:M].contiguous(), sh[:M].contiguous(), gout[:M].contiguous()
    out, _ = ops.mlp_train_fwd(h0, sh, ws, save=False, precision=precision)
    gh, gs = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, precision=precision)
    assert gh.shape == (M, 32) and gs.shape == (M, 16)
    return h0, sh, out, gout, gh, gs


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("M", SIZES)
def test_mlp_bwd_input_gh0_is_the_fused_backwards(M, precision):
    ops = _ops()
    ws = _mlp_inputs()[0]
    h0, sh, out, gout, gh, _ = _mlp_case(M, precision)
    _, gh_dw = ops.mlp_train_bwd_dw(h0, sh, out, gout, ws, want_h0=True, precision=precision)
    assert torch.equal(gh, gh_dw)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("M", SIZES)
def test_mlp_bwd_input_gsh_vs_split_path(M, precision):
    """gsh = dc1 . Wc0[:, 15:31] with dc1 the split path's own colour-layer-0 output gradient, contracted in
    float64.  Measured max|got - ref| / max|ref| (M = 4113): see DESIGN.md 4p."""
    ops = _ops()
    ws = _mlp_inputs()[0]
    h0, sh, _, gout, _, gsh = _mlp_case(M, precision)
    with _precision(precision):   # acn_mlp_train_bwd follows the module's precision
        out, save = ops.mlp_train_fwd(h0, sh, ws, save=True)
        gs, _ = ops.mlp_train_bwd(save, out, gout, ws, want_h0=False)
    dc1 = gs[:, 144:208, :].permute(0, 2, 1).reshape(-1, 64)[:M].double()
    ref = dc1 @ ws[8][:, 15:31].double()
    err = float((gsh.double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"M={M} {precision}: max|gsh - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / max(scale, 1e-30):.3e}")
    assert scale > 0
    assert err <= 2e-5 * scale + 1e-9


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("M", SIZES)
def test_mlp_bwd_input_repeats_and_ignores_the_batch(M, precision):
    ops = _ops()
    ws = _mlp_inputs()[0]
    h0, sh, out, gout, gh, gsh = _mlp_case(M, precision)
    gh2, gsh2 = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, precision=precision)
    assert torch.equal(gh, gh2) and torch.equal(gsh, gsh2)
    _, _, _, _, gh_big, gsh_big = _mlp_case(M_BIG, precision)
    assert torch.equal(gh_big[:M], gh) and torch.equal(gsh_big[:M], gsh)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("M", SIZES)
def test_mlp_bwd_input_null_outputs_and_forward_image(M, precision):
    ops = _ops()
    ws = _mlp_inputs()[0]
    h0, sh, out, gout, gh, gsh = _mlp_case(M, precision)
    a, none = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, want_sh=False, precision=precision)
    assert none is None and torch.equal(a, gh)
    none, b = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, want_h0=False, precision=precision)
    assert none is None and torch.equal(b, gsh)
    assert ops.mlp_train_bwd_input(h0, sh, out, gout, ws, want_h0=False, want_sh=False, precision=precision) == (None, None)
    out2, _, img = ops.mlp_train_fwd(h0, sh, ws, save=False, precision=precision, return_img=True)
    assert torch.equal(out2, out)
    c, d = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, img=img, precision=precision)
    assert torch.equal(c, gh) and torch.equal(d, gsh)


def test_mlp_bwd_input_empty_batch_and_amp():
    ops = _ops()
    ws = _mlp_inputs()[0]
    z = lambda c: torch.zeros(0, c, device=DEV)  # noqa: E731
    gh, gsh = ops.mlp_train_bwd_input(z(32), z(16), z(4), z(4), ws)
    assert gh.shape == (0, 32) and gsh.shape == (0, 16)
    with pytest.raises(ops.AcnError, match="amp"):
        ops.mlp_train_bwd_input(z(32), z(16), z(4), z(4), ws, precision="amp")


# ------------------------------------------------------------------------------------------------- field
def _graph_has(t, name, depth=6):
    seen, todo = set(), [(t.grad_fn, 0)]
    while todo:
        fn, d = todo.pop()
        if fn is None or fn in seen or d > depth:
            continue
        seen.add(fn)
        if name in type(fn).__name__:
            return True
        todo += [(nf, d + 1) for nf, _ in fn.next_functions]
    return False


def test_field_input_gradient_fused_vs_composed():
    m = TI._expert().eval().requires_grad_(False)
    x_d0 = TI._field_inputs()
    wgt = torch.randn(500, 4, generator=torch.Generator().manual_seed(13)).to(DEV)

    def run():
        x_d = x_d0.clone().requires_grad_()
        y = m(x_d)
        (gx,) = torch.autograd.grad((y * wgt).sum(), x_d)
        return y, gx

    y, got = run()
    assert _graph_has(y, "_FusedMLPFn", depth=2)
    with _input_grad_fused(False):
        y_ref, ref = run()
    assert not _graph_has(y_ref, "_FusedMLPFn")
    assert float(ref[:, :3].abs().max()) > 0 and float(ref[:, 3:].abs().max()) > 0
    assert float(got[:, :3].abs().max()) > 0 and float(got[:, 3:].abs().max()) > 0
    assert TI._close(y, y_ref)
    assert TI._close(got, ref)


def test_field_with_trainable_weight_keeps_composed_chain():
    m = TI._expert().eval().requires_grad_(False)
    m.color_mlp[2].weight.requires_grad_(True)
    x_d = TI._field_inputs().requires_grad_()
    y = m(x_d)
    assert y.grad_fn is not None and not _graph_has(y, "_FusedMLPFn")
    gx, gw = torch.autograd.grad(y.sum(), [x_d, m.color_mlp[2].weight])
    assert float(gx[:, 3:].abs().max()) > 0 and float(gw.abs().max()) > 0
    with _precision("amp"):      # AMP with differentiated inputs: the composed chain too
        m.requires_grad_(False)
        assert not _graph_has(m(x_d), "_FusedMLPFn")


def test_field_input_gradient_is_first_order_only():
    from adaptive_city_nerf_amd._lib import AcnError
    from adaptive_city_nerf_amd.ray_rendering import second_order
    m = TI._expert().eval().requires_grad_(False)
    x_d = TI._field_inputs().requires_grad_()
    with pytest.raises(AcnError, match="second-order"):
        torch.autograd.grad(m(x_d).sum(), x_d, create_graph=True)
    with second_order():   # the scope keeps the composed chain; its encoders refuse the same way
        y = m(x_d)
        assert not _graph_has(y, "_FusedMLPFn")
        with pytest.raises(AcnError, match="second-order"):
            torch.autograd.grad(y.sum(), x_d, create_graph=True)


def test_table_gradient_with_frozen_mlp_is_unchanged():
    """Table trainable, MLP frozen: one acn_mlp_train_bwd_input launch instead of the fused backward; the hash
    features' gradient is bit-identical, so the table gradient's inputs are too."""
    m = TI._expert().eval().requires_grad_(False)
    x_d = TI._field_inputs()
    h0 = m._enc_xyz(x_d[:, :3]).detach().requires_grad_()
    with torch.no_grad():
        sh = m._enc_dir(x_d[:, 3:6])
    from adaptive_city_nerf_amd.meta_ngp import _FusedMLPFn
    ws = [t.contiguous() for t in m._mlp_tensors(None).values()]
    wgt = torch.randn(500, 4, generator=torch.Generator().manual_seed(14)).to(DEV)

    def run():
        (g,) = torch.autograd.grad((_FusedMLPFn.apply(h0, sh, *ws) * wgt).sum(), h0)
        return g

    got = run()
    with _input_grad_fused(False):
        ref = run()
    assert float(ref.abs().max()) > 0 and torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------- rays_from_dirs_bwd
@lru_cache(maxsize=None)
def _rays_case(N):
    gen = torch.Generator().manual_seed(1000 + N)
    dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(DEV)
    c2w = torch.randn(3, 4, generator=gen)
    g_rays = torch.randn(N, 8, generator=gen).to(DEV)
    assert float(g_rays[:, 6:].abs().min()) > 0
    g_c2w, g_dirs = _ops().rays_from_dirs_bwd(dirs, c2w, g_rays)
    return dirs, c2w, g_rays, g_c2w, g_dirs


@pytest.mark.parametrize("N", [1, 255, 257, 70001])
def test_rays_from_dirs_bwd_vs_float64(N):
    ops = _ops()
    dirs, c2w, g_rays, g_c2w, g_dirs = _rays_case(N)
    assert g_c2w.shape == (3, 4) and g_dirs.shape == (N, 3) and g_c2w.dtype == g_dirs.dtype == torch.float32
    d, g, R = dirs.double(), g_rays.double(), c2w[:, :3].double().to(DEV)
    ref_c = torch.cat([g[:, 3:6].t() @ d, g[:, :3].sum(0)[:, None]], 1)
    B_c = torch.cat([g[:, 3:6].abs().t() @ d.abs(), g[:, :3].abs().sum(0)[:, None]], 1)
    ref_d = g[:, 3:6] @ R
    B_d = g[:, 3:6].abs() @ R.abs()
    ec, ed = (g_c2w.double() - ref_c).abs(), (g_dirs.double() - ref_d).abs()
    print(f"N={N}: max err/B  g_c2w {float((ec / B_c).max()):.3e}  g_dirs {float((ed / B_d).max()):.3e}")
    assert bool((ec <= 1e-6 * B_c).all())
    assert bool((ed <= 1e-6 * B_d).all())
    # near / far columns are ignored; two calls agree bit for bit; g_dirs is optional
    g2 = g_rays.clone()
    g2[:, 6:] = torch.randn(N, 2, generator=torch.Generator().manual_seed(5)).to(DEV) * 100.0
    a, b = ops.rays_from_dirs_bwd(dirs, c2w, g2)
    assert torch.equal(a, g_c2w) and torch.equal(b, g_dirs)
    a, b = ops.rays_from_dirs_bwd(dirs, c2w, g_rays, want_dirs=False)
    assert torch.equal(a, g_c2w) and b is None


def test_rays_from_dirs_bwd_without_rays_writes_zeros():
    g_c2w, g_dirs = _ops().rays_from_dirs_bwd(torch.zeros(0, 3, device=DEV), torch.eye(4), torch.zeros(0, 8, device=DEV))
    assert g_dirs.shape == (0, 3) and bool((g_c2w == 0).all())


# ------------------------------------------------------------------------------------------------- get_rays
def _box():
    from adaptive_city_nerf_amd import SceneBox
    return SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]))


@pytest.mark.parametrize("with_box", [False, True])
def test_get_rays_autograd(with_box):
    from adaptive_city_nerf_amd.ray_sampling import get_rays
    ops = _ops()
    gen = torch.Generator().manual_seed(77)
    dirs0 = torch.nn.functional.normalize(torch.randn(5, 7, 3, generator=gen), dim=-1).to(DEV)
    c0 = torch.cat([torch.linalg.qr(torch.randn(3, 3, generator=gen))[0], 0.3 * torch.randn(3, 1, generator=gen)], 1)
    kw = dict(scene_box=_box()) if with_box else dict(near=0.1, far=4.0)
    plain = get_rays(dirs0, c0, **kw)
    assert plain.grad_fn is None and not plain.requires_grad and plain.shape == (5, 7, 8)
    wgt = torch.randn(5, 7, 8, generator=gen).to(DEV)
    # 3x4 pose on the device, (H,W,3) directions: both differentiated
    c2w, dirs = c0.to(DEV).requires_grad_(), dirs0.clone().requires_grad_()
    rays = get_rays(dirs, c2w, **kw)
    assert rays.grad_fn is not None and torch.equal(rays.detach(), plain)
    (rays * wgt).sum().backward()
    g_c2w, g_dirs = ops.rays_from_dirs_bwd(dirs0, c0, wgt)
    assert c2w.grad.shape == (3, 4) and c2w.grad.device == c2w.device and torch.equal(c2w.grad, g_c2w)
    assert dirs.grad.shape == (5, 7, 3) and torch.equal(dirs.grad, g_dirs.view(5, 7, 3))
    assert float(c2w.grad.abs().min()) > 0
    # 4x4 float64 pose on the host, (N,3) directions that do not require grad
    c44 = torch.eye(4, dtype=torch.float64)
    c44[:3, :4] = c0.double()
    c44.requires_grad_()
    rays = get_rays(dirs0.view(-1, 3), c44, **kw)
    assert rays.shape == (35, 8) and torch.equal(rays.detach(), plain.view(35, 8))
    (rays * wgt.view(35, 8)).sum().backward()
    assert c44.grad.shape == (4, 4) and c44.grad.dtype == torch.float64 and c44.grad.device.type == "cpu"
    assert torch.equal(c44.grad[:3].float(), g_c2w.cpu()) and bool((c44.grad[3] == 0).all())
    # directions only
    d2 = dirs0.clone().requires_grad_()
    get_rays(d2, c0, **kw).mul(wgt).sum().backward()
    assert torch.equal(d2.grad, g_dirs.view(5, 7, 3))
    from adaptive_city_nerf_amd._lib import AcnError
    c3 = c0.to(DEV).requires_grad_()
    with pytest.raises(AcnError, match="second-order"):
        torch.autograd.grad(get_rays(dirs0, c3, **kw).sum(), c3, create_graph=True)


# ------------------------------------------------------------------------------------------------- end to end
def test_pose_step_end_to_end():
    from adaptive_city_nerf_amd import render_rays
    from adaptive_city_nerf_amd.ray_sampling import get_rays
    ops = _ops()
    m, gbox = TI._container("k1")
    S = 16
    r0 = torch.from_numpy(G.load("render_k1")["render:rays"][:64]).to(DEV)
    # a pose that reproduces the golden rays' neighbourhood: their mean origin, a small rotation of their directions
    a = 0.02
    Rm = torch.tensor([[1.0, -a, a], [a, 1.0, -a], [-a, a, 1.0]])
    c0 = torch.cat([Rm, r0[:, :3].mean(0).cpu()[:, None]], 1).to(DEV)
    dirs = r0[:, 3:6].contiguous()
    gen = torch.Generator().manual_seed(60)
    wr, wd = torch.randn(64, 3, generator=gen).to(DEV), torch.randn(64, generator=gen).to(DEV)

    def loss_of(rays):
        rgb, depth, _, _ = render_rays(m, rays, ray_samples=S)
        return (rgb * wr).sum() + (depth * wd).sum()

    c2w = c0.clone().requires_grad_()
    rays = get_rays(dirs, c2w, scene_box=gbox)
    assert bool(torch.isfinite(rays).all()) and bool((rays[:, 7] > rays[:, 6]).all())
    loss_of(rays).backward()
    assert c2w.grad.shape == (3, 4) and bool(torch.isfinite(c2w.grad).all()) and bool((c2w.grad != 0).all())
    leaf = rays.detach().clone().requires_grad_()
    (g_rays,) = torch.autograd.grad(loss_of(leaf), leaf)
    g_c2w, _ = ops.rays_from_dirs_bwd(dirs, c0, g_rays, want_dirs=False)
    assert torch.equal(c2w.grad, g_c2w)
