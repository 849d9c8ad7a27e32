"""The fused per-image affine colour loss on the GPU (acn_appearance_mse / acn_appearance_apply)
against the definition of tests/appearance_ref.py, and its way up: train.appearance_mse_loss, compute_loss / adapt_step /
GraphedAdaptStep / runtime_adapt with an AppearanceAffine, render_image with a frame's image index.

The kernel evaluates c in float64 in the definition's order and casts once, takes d in fp32 with loss.hip's helpers
(bit-exact while gt_linear stays off powf), and carries everything after d in float64, rounding each output to fp32
once.  So |got - ref| <= 4 * 2^-24 * max|ref| + 1e-30, with the maximum over the ray for g_pred, over the slot for g_A
and g_b, and the loss itself for the loss (four fp32 roundings against the one the arithmetic performs;
tests/test_depth_loss_gpu.py's bound).  The worst ratio to that bound is printed."""
import numpy as np
import pytest
import torch

import appearance_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 4 * 2.0 ** -24


def _up(x, offset=0):
    """``x`` on the device, its storage ``offset`` elements into an allocation (1: unaligned for any vector load)."""
    t = torch.from_numpy(np.array(x, order="C"))   # a copy: the shared inputs are read-only
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    out = buf[offset:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + offset * t.element_size()
    return out


def _run(x, offset=0, want_grad=True):
    from adaptive_city_nerf_amd import ops
    return ops.appearance_mse(*(_up(v, offset) for v in x), want_grad=want_grad)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _ratios(out, ref, extra=None):
    """Worst |got - ref| over its bound, for (loss, g_pred per ray, g_A per slot, g_b per slot).  ``extra``: a further
    absolute allowance per output (the powf term of test_generic_targets)."""
    ex = extra or {"loss": 0.0, "g_pred": 0.0, "g_A": 0.0, "g_b": 0.0}
    loss, g_pred, g_A, g_b = out
    r_l = abs(float(loss) - ref["loss"]) / (BOUND * abs(ref["loss"]) + ex["loss"] + 1e-30)
    m = np.abs(ref["g_pred"]).max(1, keepdims=True)
    r_p = (np.abs(_np(g_pred) - ref["g_pred"]) / (BOUND * m + ex["g_pred"] + 1e-30)).max()
    m = np.abs(ref["g_A"]).max((1, 2), keepdims=True)
    r_A = (np.abs(_np(g_A) - ref["g_A"]) / (BOUND * m + ex["g_A"] + 1e-30)).max()
    m = np.abs(ref["g_b"]).max(1, keepdims=True)
    r_b = (np.abs(_np(g_b) - ref["g_b"]) / (BOUND * m + ex["g_b"] + 1e-30)).max()
    return float(r_l), float(r_p), float(r_A), float(r_b)


@pytest.mark.parametrize("I", R.I_CASES)
@pytest.mark.parametrize("N", R.N_CASES)
def test_kernel_matches_the_definition(N, I):
    """N on every loop boundary of the ray workgroups (wave, workgroup, the 256-workgroup cap at 65536 rays and one
    past it), I from one slot to more slot workgroups than ray workgroups; the layouts: slots mixed with an empty
    slot, -1 and >= I (at aligned and at unaligned storage), every ray in one slot, no ray in any slot.  Targets stay
    off powf (tests/test_appearance_cpu.py checks the inputs' conditions)."""
    for layout in R.LAYOUTS:
        x, ref = R.case(N, I, layout)
        for offset in ((0, 1) if layout == "mixed" else (1,)):
            out = _run(x, offset)
            r = _ratios(out, ref)
            print(f"N {N}, I {I}, {layout}, offset {offset}: loss {r[0]:.3f}, g_pred {r[1]:.3f}, g_A {r[2]:.3f}, "
                  f"g_b {r[3]:.3f} of the bound")
            assert max(r) <= 1
            cnt = np.bincount(x[2][ref["has"]], minlength=I)
            assert bool((out[2].cpu().numpy()[cnt == 0] == 0).all()) and bool((out[3].cpu().numpy()[cnt == 0] == 0).all())
            dead = ~ref["live"] & ~ref["has"][:, None]      # without a slot g_pred is g_c: exact zeros in the dead zone
            assert bool((out[1].cpu().numpy()[dead] == 0).all())


@pytest.mark.parametrize("shape", [(1000, 3), (4099, 70)])
def test_generic_targets(shape):
    """Targets anywhere in [-0.1, 1.1]: gt_linear goes through powf, where the device's result may differ from the
    reference's correctly rounded one by an ulp (at most 2^-24 below 1); d = clamp01(c) - gt_linear is rounded again
    (2^-25 of at most 1 ... its rounding may move by as much as the operand did), so d moves by at most
    delta = 2^-23, about 1e-7, tests/test_loss_gpu.py's term.  Per output, on top of the bound above:
      loss:        sum 2 |d| delta / n + delta^2           = 2 delta mean|d| + delta^2
      g_c:         (2 / n) delta per element, so
      g_pred[r,j]: (2 / n) delta sum_k |A[s,k,j]|          ((2 / n) delta without a slot)
      g_A[i,k,j]:  (2 / n) delta sum_{r in i} |p[r,j]|
      g_b[i,k]:    (2 / n) delta (rays in slot i)."""
    N, I = shape
    x, ref = R.case(N, I, "mixed", "generic")
    pred, gt, slot, A, b = x
    assert float(((gt > 0.04045) & (gt < 1)).mean()) > 0.5
    n, dl, has = 3 * N, R.POW_DELTA, ref["has"]
    e = (2.0 / n) * dl
    sum_p, cnt = np.zeros((I, 3)), np.zeros(I)
    np.add.at(sum_p, slot[has], np.abs(pred[has].astype(np.float64)))
    np.add.at(cnt, slot[has], 1.0)
    extra = {"loss": 2 * dl * float(np.abs(ref["d"].astype(np.float64)).mean()) + dl * dl,
             "g_pred": e * np.where(has[:, None], np.abs(A[np.where(has, slot, 0)].astype(np.float64)).sum(1), 1.0),
             "g_A": e * sum_p[:, None, :], "g_b": e * cnt[:, None]}
    for offset in (0, 1):
        r = _ratios(_run(x, offset), ref, extra)
        print(f"generic targets {shape}, offset {offset}: loss {r[0]:.3f}, g_pred {r[1]:.3f}, g_A {r[2]:.3f}, "
              f"g_b {r[3]:.3f} of the bound plus the powf term")
        assert max(r) <= 1


@pytest.mark.parametrize("shape", [(1024, 3), (4096, 70)])
def test_dyadic_inputs_are_exact_in_any_order(shape):
    """On tests/appearance_ref.py's dyadic inputs every product and sum after d is exact, so the outputs are the
    reference's bit for bit, and stay so when the rays are permuted (another assignment of rays to threads and
    another order of every sum)."""
    N, I = shape
    x = R.dyadic_inputs(N, I)
    ref = R.reference(*x)
    perm = np.random.default_rng(5).permutation(N)
    for order in (np.arange(N), perm, np.arange(N)[::-1]):
        xp = (x[0][order], x[1][order], x[2][order], x[3], x[4])
        loss, g_pred, g_A, g_b = _run(xp, 1)
        assert np.array_equal(g_A.cpu().numpy(), ref["g_A"].astype(np.float32))
        assert np.array_equal(g_b.cpu().numpy(), ref["g_b"].astype(np.float32))
        assert np.array_equal(g_pred.cpu().numpy(), ref["g_pred"][order].astype(np.float32))
        assert abs(float(loss) - ref["loss"]) <= BOUND * ref["loss"]
    assert float(np.abs(ref["g_A"]).max()) > 0


def _loss_inputs(n, seed):
    """tests/test_loss_gpu.py's inputs: out-of-range predictions, values at 0 / 1, targets around the sRGB knee."""
    from test_loss_gpu import _inputs
    return _inputs(n, seed)


@pytest.mark.parametrize("n", [64, 1000])
def test_identity_is_the_existing_loss_kernel(n):
    """With identity A and zero b, or with every slot -1, c is the prediction bit for bit: g_pred is mse_linear_bwd's
    at g_loss = 1 bitwise, the loss is mse_linear_fwd's to the order of the sum, and g_A is sum g (x) p.  With a NaN
    element the loss is NaN and the gradient at that element 0, as in test_fused_linear_mse_nan_like_torch.  (Under
    the identity MATRIX a NaN channel makes all three of its ray's c NaN, 0 * NaN, so that whole ray's gradient is 0;
    with slot -1 only the element's.)"""
    from adaptive_city_nerf_amd import ops
    pred, gt = _loss_inputs(n, 3)
    pd, gd = pred.to(DEV), gt.to(DEV)
    one = torch.ones((), device=DEV)
    I = 5
    A, b = torch.eye(3, device=DEV).repeat(I, 1, 1), torch.zeros(I, 3, device=DEV)
    slots = (torch.arange(n, device=DEV) % I).int()
    minus = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    want = ops.mse_linear_bwd(pd, gd, one)
    want_loss = ops.mse_linear_fwd(pd, gd)
    assert int((want == 0).sum()) > 0 and int(((pred < 0) | (pred > 1)).sum()) > 0
    for s in (slots, minus):
        loss, g_pred, g_A, g_b = ops.appearance_mse(pd, gd, s, A, b)
        assert torch.equal(g_pred, want)
        assert abs(float(loss) - float(want_loss)) <= 2.0 ** -22 * float(want_loss)
        # the definition's sums over g (the existing kernel's own, so that powf does not enter) in float64
        sn, g64 = s.cpu().numpy(), _np(want)
        has = (sn >= 0) & (sn < I)
        gA, gb = np.zeros((I, 3, 3)), np.zeros((I, 3))
        np.add.at(gA, sn[has], g64[has][:, :, None] * pred.numpy().astype(np.float64)[has][:, None, :])
        np.add.at(gb, sn[has], g64[has])
        assert bool((np.abs(_np(g_A) - gA) <= BOUND * np.abs(gA).max((1, 2), keepdims=True) + 1e-30).all())
        assert bool((np.abs(_np(g_b) - gb) <= BOUND * np.abs(gb).max(1, keepdims=True) + 1e-30).all())
        assert s is minus or float(np.abs(gA).max()) > 0
        if s is minus:
            assert int(g_A.count_nonzero()) == 0 and int(g_b.count_nonzero()) == 0
    # a NaN element
    pred = pred.clone()
    pred[5, 1] = float("nan")
    pd = pred.to(DEV)
    want = ops.mse_linear_bwd(pd, gd, one)
    assert float(want[5, 1]) == 0.0
    loss, g_pred, _, _ = ops.appearance_mse(pd, gd, minus, A, b)
    assert bool(torch.isnan(loss)) and float(g_pred[5, 1]) == 0.0 and torch.equal(g_pred, want)
    loss, g_pred, g_A, g_b = ops.appearance_mse(pd, gd, slots, A, b)
    keep = torch.arange(n, device=DEV) != 5
    assert bool(torch.isnan(loss)) and float(g_pred[5, 1]) == 0.0 and torch.equal(g_pred[keep], want[keep])
    assert int(g_pred[5].count_nonzero()) == 0 and int(g_b[5 % I].isnan().sum()) == 0
    other = torch.arange(I, device=DEV) != 5 % I
    assert bool(torch.isfinite(g_A[other]).all())   # the NaN stays in its own slot (0 * NaN in g (x) p)


def test_reproducible_without_gradients_and_under_graph_capture():
    from adaptive_city_nerf_amd import ops
    from adaptive_city_nerf_amd._lib import graph_capture
    xa, _ = R.case(4099, 70, "mixed", "generic")
    xb, _ = R.case(4099, 70, "one", "generic")
    xc = (xa[0][::-1], xb[1], xa[2][::-1], xb[3], xa[4])
    eager = []
    for x in (xa, xb, xc):
        a, b = _run(x), _run(x, 1)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        loss, g_pred, g_A, g_b = _run(x, want_grad=False)
        assert g_pred is None and g_A is None and g_b is None and torch.equal(loss, a[0])
        eager.append(a)
    st = [_up(v).clone() for v in xa]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.appearance_mse(*st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):
        out = ops.appearance_mse(*st)
        out_ng = ops.appearance_mse(*st, want_grad=False)
    for x, want in zip((xa, xb, xc), eager):
        for dst, src in zip(st, x):
            dst.copy_(torch.from_numpy(np.array(src, order="C")))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(out, want)) and torch.equal(out_ng[0], want[0])
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(out, eager[2]))


@pytest.mark.parametrize("shape", [(1, 1), (257, 3), (4099, 300)])
def test_apply(shape):
    from adaptive_city_nerf_amd import AppearanceAffine, ops
    N, I = shape
    (pred, _, slot, A, b), ref = R.case(N, I, "mixed")
    for offset in (0, 1):
        p, s, Ad, bd = (_up(v, offset) for v in (pred, slot, A, b))
        c = ops.appearance_apply(p, s, Ad, bd)
        assert np.array_equal(c.cpu().numpy(), ref["c"])
        none = ~torch.from_numpy(ref["has"])
        assert torch.equal(c.cpu()[none].view(torch.int32), torch.from_numpy(pred)[none].view(torch.int32))
    # the module: no gradient needed -> the kernel; an image shape and one index for the frame
    app = AppearanceAffine(I, device=DEV)
    with torch.no_grad():
        app.matrix.copy_(_up(A))
        app.offset.copy_(_up(b))
        got = app(_up(pred), _up(slot))
        assert np.array_equal(got.cpu().numpy(), ref["c"])
        frame = _up(pred).view(1, N, 3)
        one = app(frame, I - 1)
        want = R.corrected(pred, np.full(N, I - 1, np.int32), A, b)
        assert one.shape == frame.shape and np.array_equal(one.cpu().numpy().reshape(N, 3), want)
        assert torch.equal(app(frame, 10 ** 6), frame)
    # with a gradient: torch ops, equal to a few fp32 roundings
    t = app(_up(pred).requires_grad_(True), _up(slot))
    assert t.requires_grad and float((t.detach() - got).abs().max()) <= 8 * 2.0 ** -24 * 2.0


def _chain(pred, gt, slots, A, b):
    """The composed torch chain on the device: the correction as torch ops, then F.mse_loss of the colour transform."""
    import torch.nn.functional as F
    from adaptive_city_nerf_amd.appearance import _apply_torch
    from adaptive_city_nerf_amd.color_space import color_space_transformer
    pr, gr = color_space_transformer(_apply_torch(pred, slots, A, b), gt, color_space="linear")
    return F.mse_loss(pr, gr, reduction="mean")


def test_loss_function_matches_the_torch_chain():
    """train.appearance_mse_loss under autograd, scaled by 3, against the composed torch chain on the device, with
    tests/test_loss_gpu.py's tolerances: rtol 2e-6 on the loss; rtol 1e-6 and 2 / numel * 3e-7 * 3 absolute on d loss /
    d c of an element (what that file bounds: there c is the prediction), which every gradient here is a sum of, so
    the absolute term carries through the sum: times sum_k |A[s,k,j]| for g_pred[r,j] (1 without a slot), times the
    slot's ray count for g_b and 1.2 times that for g_A (|p| <= 1.2).
    Inside second_order() the Function is not used and the result can be differentiated again."""
    from adaptive_city_nerf_amd import AppearanceAffine
    from adaptive_city_nerf_amd.ray_rendering import second_order
    from adaptive_city_nerf_amd.train import appearance_mse_loss
    N, I = 1000, 70
    (pred, gt, slot, A, b), ref = R.case(N, I, "mixed", "generic")
    ids = list(range(5, 5 + 2 * I, 2))
    app = AppearanceAffine(ids, device=DEV)
    with torch.no_grad():
        app.matrix.copy_(_up(A))
        app.offset.copy_(_up(b))
    img = _up(np.where(ref["has"], 5 + 2 * np.where(ref["has"], slot, 0), np.where(slot < 0, 4, 5 + 2 * I + 7)))
    assert torch.equal(app.slots(img).cpu(), torch.from_numpy(np.where(ref["has"], slot, -1).astype(np.int32)))
    pa, pb, gd = _up(pred).requires_grad_(True), _up(pred).requires_grad_(True), _up(gt)
    la = appearance_mse_loss(pa, gd, img, app, "linear")
    assert type(la.grad_fn).__name__.startswith("_AppearanceMSEFn")
    ga = torch.autograd.grad(la * 3.0, (pa, app.matrix, app.offset))
    A2, b2 = app.matrix.detach().clone().requires_grad_(True), app.offset.detach().clone().requires_grad_(True)
    lb = _chain(pb, gd, app.slots(img), A2, b2)
    gb = torch.autograd.grad(lb * 3.0, (pb, A2, b2))
    print(f"loss {float(la.detach()):.8f} against {float(lb.detach()):.8f}")
    assert torch.allclose(la, lb, rtol=2e-6, atol=0)
    atol = 6e-7 / pred.size * 3.0
    cnt = torch.from_numpy(np.bincount(slot[ref["has"]], minlength=I)).to(DEV).float()
    has = torch.from_numpy(ref["has"]).to(DEV)
    col = torch.where(has[:, None], A2.detach()[app.slots(img).clamp_min(0).long()].abs().sum(1), torch.ones((), device=DEV))
    for name, u, v, k in (("g_pred", ga[0], gb[0], col), ("g_A", ga[1], gb[1], 1.2 * cnt[:, None, None]),
                          ("g_b", ga[2], gb[2], cnt[:, None])):
        over = ((u - v).abs() / (1e-6 * v.abs() + atol * torch.as_tensor(k, device=DEV).clamp_min(1.0))).max()
        print(f"{name}: worst |fused - chain| at {float(over):.3f} of the tolerance")
        assert float(over) <= 1
    assert int((ga[1][cnt == 0] != 0).sum()) == 0
    # the kernel's own numbers under the Function
    k_loss, k_gp, k_gA, k_gb = _run((pred, gt, np.where(ref["has"], slot, -1).astype(np.int32), A, b))
    assert torch.equal(la.detach(), k_loss) and torch.equal(ga[0], 3.0 * k_gp) and torch.equal(ga[1], 3.0 * k_gA)
    with second_order():
        pc = _up(pred).requires_grad_(True)
        lc = appearance_mse_loss(pc, gd, img, app, "linear")
        assert not type(lc.grad_fn).__name__.startswith("_AppearanceMSEFn")
        g_c, = torch.autograd.grad(lc, pc, create_graph=True)
    assert g_c.requires_grad and torch.allclose(lc, lb, rtol=2e-6, atol=0)
    g2, = torch.autograd.grad(g_c.sum(), app.matrix)
    assert bool(torch.isfinite(g2).all()) and float(g2.abs().max()) > 0
    # reduction "none" and another colour space take the chain as well
    assert appearance_mse_loss(pa, gd, img, app, "linear", reduction="none").shape == (N, 3)
    assert float(appearance_mse_loss(pa, gd, img, app, "srgb")) > 0


def _bare_expert():
    """A small MetaNGP: 16 levels of 2^12 rows."""
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    torch.manual_seed(11)
    conf = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": 12, "max_res": 4096, "min_res": 16,
            "interpolation": "Linear"}
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=conf, dir_encoding="spherical")
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    return m.to(DEV).train()


def test_adapt_step_trains_the_field_and_the_touched_slots():
    """One adapt_step on a small MetaNGP, 256 rays x 32 samples with a fixed jitter, with an AppearanceAffine in the
    optimizer: the field and the slots the batch touches change, a slot no ray touched gets an exact zero gradient,
    and the step's loss is the fused loss of the step's own render."""
    from types import SimpleNamespace
    from adaptive_city_nerf_amd import AppearanceAffine, render_rays
    from adaptive_city_nerf_amd.optim import FusedAdam
    from adaptive_city_nerf_amd.train import adapt_step, appearance_mse_loss
    P = SimpleNamespace(ray_samples=32, chunk_points=1 << 20, color_space="linear")
    m = _bare_expert()
    gen = torch.Generator().manual_seed(9)
    N = 256
    o = torch.rand(N, 3, generator=gen) * 1.6 - 0.8
    dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    near = 0.05 * torch.rand(N, generator=gen)
    rays = torch.cat([o, dirs, near[:, None], (near + 0.5 + torch.rand(N, generator=gen))[:, None]], 1).to(DEV)
    u = torch.rand(N, 32, generator=gen).to(DEV)
    rgbs = torch.rand(N, 3, generator=gen).to(DEV)
    app = AppearanceAffine([10, 11, 12, 40], device=DEV)
    img = torch.tensor([10, 12, 99, 11], device=DEV).repeat(N // 4)         # image 40 has no ray; 99 has no slot
    opt = FusedAdam([{"params": list(m.parameters()), "lr": 1e-3},
                     {"params": list(app.parameters()), "lr": 1e-2, "name": "appearance"}])
    pred, *_ = render_rays(m, rays, ray_samples=32, chunk=P.chunk_points, jitter_u=u)   # the step's own path
    with torch.no_grad():
        want = appearance_mse_loss(pred.detach(), rgbs, img, app, "linear")
    before = [p.detach().clone() for p in m.parameters()]
    A0, b0 = app.matrix.detach().clone(), app.offset.detach().clone()
    loss = adapt_step(P, m, rays, rgbs, opt, grad_clip=1.0, jitter_u=u, img_indices=img, appearance=app)
    print(f"adapt_step loss {float(loss):.8f}, the render's fused loss {float(want):.8f}")
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert any(not torch.equal(a, p) for a, p in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in list(m.parameters()) + list(app.parameters()))
    assert int(app.matrix.grad[3].count_nonzero()) == 0 and int(app.offset.grad[3].count_nonzero()) == 0
    for s in range(3):
        assert float(app.matrix.grad[s].abs().max()) > 0 and not torch.equal(app.matrix[s], A0[s])
        assert not torch.equal(app.offset[s], b0[s])
    assert torch.equal(app.matrix[3], A0[3]) and torch.equal(app.offset[3], b0[3])
    # the regulariser pulls back towards the identity: it adds to the loss once the parameters have moved
    l_reg = adapt_step(P, m, rays, rgbs, opt, grad_clip=1.0, jitter_u=u, img_indices=img, appearance=app,
                       appearance_reg=10.0)
    l_plain = adapt_step(P, m, rays, rgbs, opt, grad_clip=1.0, jitter_u=u, img_indices=img, appearance=app)
    assert np.isfinite(float(l_reg)) and np.isfinite(float(l_plain))
    # the refusals
    with pytest.raises(ValueError, match="img_indices"):
        adapt_step(P, m, rays, rgbs, opt, appearance=app)
    with pytest.raises(ValueError, match="optimizer"):
        adapt_step(P, m, rays, rgbs, FusedAdam(list(m.parameters())), appearance=app, img_indices=img)
    with pytest.raises(ValueError, match="expert-parallel"):
        adapt_step(P, m, rays, rgbs, opt, appearance=app, img_indices=img, group=object())


def _setup():
    from test_graph_gpu import _setup as setup
    return setup()


def _with_appearance(opt, I):
    from adaptive_city_nerf_amd import AppearanceAffine
    app = AppearanceAffine(I, device=DEV)
    opt.add_param_group({"params": list(app.parameters()), "lr": 0.01, "name": "appearance"})
    return app


def test_graphed_adapt_step_with_an_appearance_model_matches_eager():
    """tests/test_graph_gpu.py's comparison of graph replays with eager steps, its batches and its tolerance on the
    loss, with the appearance model in the captured step and new image indices on every replay."""
    from test_graph_gpu import _batches
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step
    P, ma, oa, d = _setup()
    _, mb, ob, _ = _setup()
    I = 6
    appa, appb = _with_appearance(oa, I), _with_appearance(ob, I)
    batches = _batches(d, 4, S=P.ray_samples)
    n = batches[0][0].shape[0]
    g = torch.Generator().manual_seed(8)
    imgs = [torch.randint(-1, I + 1, (n,), generator=g).to(DEV) for _ in batches]   # I: no slot
    kw = dict(active_module=0, grad_clip=1.0, appearance_reg=0.01)
    for i in [0, 0, 1, 2, 3]:
        rays, rgbs, u = batches[i]
        la = adapt_step(P, ma, rays, rgbs, oa, jitter_u=u, img_indices=imgs[i], appearance=appa, **kw)
    step = GraphedAdaptStep(P, mb, batches[0][0], batches[0][1], ob, warmup=2, jitter_u=batches[0][2],
                            img_indices=imgs[0], appearance=appb, **kw)
    assert step.static_img.dtype == torch.int32
    for i in (1, 2, 3):
        rays, rgbs, u = batches[i]
        lb = step(rays, rgbs, jitter_u=u, img_indices=imgs[i])
    torch.cuda.synchronize()
    step.sync_state()
    print(f"eager loss {float(la):.8f}, replayed loss {float(lb):.8f}")
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(la)) + 1e-8
    assert not torch.equal(appb.matrix, torch.eye(3, device=DEV).expand(I, 3, 3))
    # five Adam steps of 0.01 each: the two runs' corrections agree far below one step
    assert float((appa.matrix - appb.matrix).abs().max()) <= 1e-3 and float((appa.offset - appb.offset).abs().max()) <= 1e-3


def test_runtime_adapt_with_an_appearance_model_takes_the_eager_step():
    from adaptive_city_nerf_amd import train as T
    P, m, opt, d = _setup()
    app = _with_appearance(opt, 4)
    rays = torch.from_numpy(d["train0:rays"]).to(DEV)
    rgbs = torch.from_numpy(d["train0:rgbs"]).to(DEV)
    img = (torch.arange(rays.shape[0]) % 3).to(DEV)
    before = [p.detach().clone() for p in m.parameters()]
    out = T.runtime_adapt(P=P, model=m, data_loader=[(rays, rgbs, None, img)], optimizer=opt, steps=2, appearance=app,
                          appearance_reg=0.01)
    assert out["steps"] == 2 and np.isfinite(out["loss"]) and out["loss"] > 0
    assert not getattr(opt, "_acn_routed_steps", None)
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
    eye = torch.eye(3, device=DEV)
    assert all(not torch.equal(app.matrix[s], eye) for s in range(3)) and torch.equal(app.matrix[3], eye)
    with pytest.raises(ValueError, match="img_indices"):
        T.runtime_adapt(P=P, model=m, data_loader=[(rays, rgbs)], optimizer=opt, steps=1, appearance=app)


def test_render_image_corrects_the_frame():
    import goldens as G
    from test_interlevel_gpu import _train_setup
    from adaptive_city_nerf_amd import AppearanceAffine, evaluate_image, render_image
    _, m, gbox, _ = _train_setup()
    m = m.eval().requires_grad_(False)
    cam = G.scene()["val_cam0"]
    intr = torch.tensor(cam["intrinsics"], dtype=torch.float32)
    s = 16.0 / float(2.0 * intr[2])
    kw = dict(H=16, W=16, fx=float(intr[0]) * s, fy=float(intr[1]) * s, cx=8.0, cy=8.0, c2w=torch.tensor(cam["c2w"]),
              scene_box=gbox, ray_samples=16)
    app = AppearanceAffine([4, 9], device=DEV)
    with torch.no_grad():
        app.matrix[1] = torch.tensor([[0.5, 0.25, 0.0], [0.0, 1.5, 0.0], [0.125, 0.0, 0.75]], device=DEV)
        app.offset[1] = torch.tensor([0.0625, -0.125, 0.25], device=DEV)
    plain, depth0, acc0 = render_image(m, **kw)
    got, depth, acc = render_image(m, appearance=app, image_index=9, **kw)
    with torch.no_grad():
        want = app(plain, 9)
    assert torch.equal(got, want) and not torch.equal(got, plain) and torch.equal(depth, depth0)
    assert torch.equal(acc, acc0) and got.shape == plain.shape
    by_hand = plain.double() @ app.matrix[1].double().T + app.offset[1].double()
    assert float((got.double() - by_hand).abs().max()) <= 2.0 ** -23 * float(by_hand.abs().max())
    for unknown in (5, 10 ** 6, -3):
        same, _, _ = render_image(m, appearance=app, image_index=unknown, **kw)
        assert torch.equal(same.view(torch.int32), plain.view(torch.int32))
    with pytest.raises(ValueError, match="image_index"):
        render_image(m, appearance=app, **kw)
    gt = torch.rand(16, 16, 3, generator=torch.Generator().manual_seed(3))
    rgb, _, _, metrics = evaluate_image(m, gt_srgb=gt, appearance=app, image_index=9, **kw)
    assert torch.equal(rgb, got) and set(metrics) == {"psnr", "ssim"}
