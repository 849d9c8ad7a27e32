"""Online adaptation step (adaptive_city_nerf_amd/train.py + optim.py) against the reference.

CPU tests cover the host logic (param groups, descriptor plans).  GPU tests compare the fused
HIP optimizer with torch.optim.Adam / clip_grad_norm_ (the reference's own optimizer, CPU fp32),
and two full runtime_adapt steps of the K=4 container with the reference's fixture
(tests/golden/train_k4.npz, made by tests/golden/make_golden.py from the reference itself with the
training jitter injected): loss, clip norm, gradients and parameters after each Adam step.
Tolerances: fp32 sums in a different order (MKL vs rocBLAS / atomics) -> relative 1e-4 on the
loss and gradients; Adam's first steps move every parameter by ~lr * sign(g), so parameters are
compared to 1e-3 * lr plus a 0.1% allowance of sign-ambiguous (|g| ~ 0) elements.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import goldens as G

P = SimpleNamespace(ray_samples=32, chunk_points=1 << 20, color_space="linear", optimizer="adam", lr=1e-4,
                    encoding_lr=0.01, sigma_lr=0.002, color_lr=0.002, bg_lr=0.001, weight_decay=0.0)


def test_build_optimizer_groups_match_reference_config():
    from test_module_api import build_model
    from adaptive_city_nerf_amd.optim import FusedAdam, build_optimizer
    m, _ = build_model("k4")
    opt = build_optimizer(P, m)
    assert isinstance(opt, FusedAdam)
    names = [g["name"] for g in opt.param_groups]
    assert names == ["encoding", "sigma", "color", "background"]
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.002, 0.002, 0.001]
    n = sum(p.numel() for g in opt.param_groups for p in g["params"])
    assert n == sum(p.numel() for p in m.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_matches_torch_adam(wd):
    from adaptive_city_nerf_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(5)
    shapes = [(1 << 18, 2), (64, 32), (64,), (3,), (1, 64), (70001,)]   # chunk tails and tiny tensors
    ref = [torch.randn(s, generator=g) for s in shapes]
    dev = [p.clone().cuda().requires_grad_(True) for p in ref]
    ref = [p.clone().requires_grad_(True) for p in ref]
    groups_r = [{"params": ref[:2], "lr": 0.01}, {"params": ref[2:], "lr": 0.002}]
    groups_d = [{"params": dev[:2], "lr": 0.01}, {"params": dev[2:], "lr": 0.002}]
    opt_r = torch.optim.Adam(groups_r, lr=1e-4, weight_decay=wd, foreach=False)
    opt_d = FusedAdam(groups_d, lr=1e-4, weight_decay=wd)
    for step in range(3):
        for pr, pd in zip(ref, dev):
            gr = torch.randn(pr.shape, generator=g) * (10.0 ** (step - 1))
            if step == 1:
                gr[..., :1] = 0.0
            pr.grad = gr.clone()
            pd.grad = gr.clone().cuda()
        opt_r.step()
        opt_d.step()
        for pr, pd in zip(ref, dev):
            # elements whose (weight-decayed) gradient cancels to ~0 are sign-ambiguous under one
            # rounding difference: allow 1e-5 of them
            assert _close_frac(pd.detach().cpu().numpy(), pr.detach().numpy(), 2e-7, 2e-6) >= 1 - 1e-5
            np.testing.assert_allclose(opt_d.state[pd]["exp_avg_sq"].cpu().numpy(),
                                       opt_r.state[pr]["exp_avg_sq"].numpy(), rtol=2e-6, atol=1e-12)
    # state layout is torch's: the fused optimizer's state dict loads into torch.optim.Adam
    sd = opt_d.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3.0


@pytest.mark.gpu
def test_fused_clip_matches_torch_clip_grad_norm():
    from adaptive_city_nerf_amd.optim import FusedAdam, clip_grad_norm_
    g = torch.Generator().manual_seed(6)
    shapes = [(100000,), (64, 64), (3,)]
    grads = [torch.randn(s, generator=g) for s in shapes]
    ref = [torch.zeros(s, requires_grad=True) for s in shapes]
    for p, gr in zip(ref, grads):
        p.grad = gr.clone()
    tn_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    dev = [torch.zeros(s, device="cuda", requires_grad=True) for s in shapes]
    for p, gr in zip(dev, grads):
        p.grad = gr.clone().cuda()
    tn = clip_grad_norm_(dev, 1.0)
    assert abs(float(tn) - float(tn_ref)) <= 1e-5 * float(tn_ref)
    for pr, pd in zip(ref, dev):
        np.testing.assert_allclose(pd.grad.cpu().numpy(), pr.grad.numpy(), rtol=1e-5, atol=1e-9)
    # fused clip inside the step == clip then step
    a = [torch.ones(s, device="cuda", requires_grad=True) for s in shapes]
    b = [torch.ones(s, device="cuda", requires_grad=True) for s in shapes]
    for x, y, gr in zip(a, b, grads):
        x.grad = gr.clone().cuda()
        y.grad = gr.clone().cuda()
    oa, ob = FusedAdam(a, lr=0.01), FusedAdam(b, lr=0.01)
    oa.step(max_norm=1.0)
    clip_grad_norm_(b, 1.0)
    ob.step()
    for x, y in zip(a, b):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-6, atol=1e-8)


def _close_frac(a, b, atol, rtol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.mean(np.abs(a - b) <= atol + rtol * np.abs(b)))


LRS = {"encoding": 0.01, "sigma": 0.002, "color": 0.002, "background": 0.001}
FIXTURES = {"k4": ("train_k4", 32, 2), "k8": ("train_k8", 96, 3)}   # tag: (fixture, samples, steps)


def check_adapt_fixture(tag, step_fn, make_opt=None, check_grads=True, gtol_later=1e-3, need_later=0.99, stats=None):
    """Replay the reference's runtime_adapt steps of fixture ``tag`` through ``step_fn(P, model, rays,
    rgbs, opt, u) -> loss`` and compare loss, clip norm, gradients (``check_grads``: steps that clear
    the gradients in the Adam pass leave none to compare) and parameters after every step."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd.optim import build_optimizer
    name_, S, nsteps = FIXTURES[tag]
    d = G.load(name_)
    Pk = SimpleNamespace(**{**vars(P), "ray_samples": S, "chunk_points": 4_000_000})
    m, _ = build_model(tag)
    K = len(m.submodules)
    m.load_state_dict(reference_state_dict(d, K, "w:"))
    m = m.cuda().train()
    opt = (make_opt or build_optimizer)(Pk, m)
    rows = d["train:rows"]
    # Adam moves a parameter by ~lr * sign(g) whatever |g| is, so an element whose reference gradient is
    # at the fp32 noise level of its tensor (|g| < 1e-4 max|g|) at some step takes an arbitrary sign
    # under a different summation order; such elements are left out of the parameter comparison
    ambiguous = {}
    for step in range(nsteps):
        pre = f"train{step}:"
        for key in d:
            if key.startswith(pre + "grad:"):
                name = key[len(pre + "grad:"):]
                g = np.abs(d[key])
                amb = g < 1e-4 * (float(g.max()) + 1e-30)
                ambiguous[name] = amb | ambiguous.get(name, np.zeros_like(amb))
        rays = torch.from_numpy(d[pre + "rays"]).cuda()
        rgbs = torch.from_numpy(d[pre + "rgbs"]).cuda()
        u = torch.from_numpy(d[pre + "u"]).cuda()
        loss = step_fn(Pk, m, rays, rgbs, opt, u)
        torch.cuda.synchronize()
        ref_loss = float(d[pre + "loss"])
        assert abs(float(loss) - ref_loss) <= 1e-5 * ref_loss, (float(loss), ref_loss)
        assert abs(float(opt.last_norm[0]) - float(d[pre + "total_norm"])) <= 1e-4 * float(d[pre + "total_norm"])
        named = dict(m.named_parameters())
        for name, p in (named.items() if check_grads else ()):
            gkey = pre + "grad:" + name
            if name.endswith("hash_table"):
                k = int(name.split(".")[1])
                if (pre + f"grad_rows:{k}") not in d:
                    assert p.grad is None or float(p.grad.abs().max()) == 0.0
                    continue
                gt = p.grad.detach()
                np.testing.assert_allclose(gt[torch.from_numpy(rows[k]).cuda()].cpu().numpy(), d[pre + f"grad_rows:{k}"],
                                           rtol=1e-4, atol=1e-9)
                lv = gt.view(16, -1).double()
                np.testing.assert_allclose(lv.sum(1).cpu().numpy(), d[pre + f"grad_level_sum:{k}"], rtol=1e-4,
                                           atol=1e-9)
                np.testing.assert_allclose((lv ** 2).sum(1).cpu().numpy(), d[pre + f"grad_level_sumsq:{k}"],
                                           rtol=1e-4, atol=1e-15)
                assert int((gt != 0).sum()) == int(d[pre + f"grad_nnz:{k}"])
            elif gkey in d:
                ref = d[gkey]
                scale = float(np.abs(ref).max()) + 1e-12
                # from the second step on, the parameters carry the Adam sensitivity described below, so
                # the gradients are evaluated at slightly different points: 1e-3 of scale (measured spread
                # 2.5e-5 with the fp16x3 MLP, 1.6e-4 with exact fp32: profiles/r03_train_parity_spread.json)
                gtol = 1e-4 if step == 0 else gtol_later
                got_g = p.grad.detach().cpu().numpy()
                if stats is not None:
                    stats.setdefault(f"grad_dev_over_scale_step{step}", []).append(
                        float(np.abs(got_g - ref).max() / scale))
                np.testing.assert_allclose(got_g, ref, rtol=0, atol=gtol * scale)
            else:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
        for name, p in named.items():
            group = "encoding" if name.endswith("hash_table") else \
                "background" if name.startswith("bg_mlp") else \
                "color" if ".color_mlp." in name else "sigma"
            lr = LRS[group]
            if name.endswith("hash_table"):
                k = int(name.split(".")[1])
                got = p.detach()[torch.from_numpy(rows[k]).cuda()].cpu().numpy()
                ref = d[pre + f"table_rows:{k}"]
                if (pre + f"table_level_sum:{k}") in d:
                    # every touched row moves by ~lr: level sums over 2^20 rows; last-ulp differences of
                    # the Adam arithmetic random-walk to ~1e-4, one wrong-signed update would add 2 * lr
                    np.testing.assert_allclose(p.detach().view(16, -1).double().sum(1).cpu().numpy(),
                                               d[pre + f"table_level_sum:{k}"], rtol=0, atol=5e-4)
            else:
                got = p.detach().cpu().numpy()
                ref = d[pre + "param:" + name]
                if name in ambiguous:
                    keep = ~ambiguous[name]
                    got, ref = got[keep], ref[keep]
            # Adam's update -lr m / (sqrt(v) + eps) is ~lr sign(g) for |g| >> eps = 1e-8 but proportional to g
            # near it, so a weakly hit expert (K=8: expert 2's gradients are ~1e-6 at most) has elements whose
            # update follows the last bits of a gradient summed in a different order; from the second step on,
            # m / sqrt(v) also mixes steps of different signs.  Emulated with torch.optim.Adam on the fixture
            # gradients: 1e-5 relative gradient noise moves ~5% of such an expert's weights beyond 1e-3 lr after
            # 3 steps.  The gradients themselves are pinned above at 1e-4 of their scale, and the update rule
            # against torch.optim.Adam by test_fused_adam_matches_torch_adam.
            need = 0.99 if step == 0 else need_later
            frac = _close_frac(got, ref, 1e-3 * lr, 1e-6)
            if stats is not None:
                stats.setdefault(f"param_close_frac_step{step}", []).append(frac)
            assert frac >= need, (name, step, frac)
    return m, opt


def _eager_step(Pk, m, rays, rgbs, opt, u):
    from adaptive_city_nerf_amd.train import adapt_step
    return adapt_step(Pk, m, rays, rgbs, opt, grad_clip=1.0, jitter_u=u)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["k4", "k8"])
def test_adapt_steps_match_reference_fixture(tag):
    """runtime_adapt on the routed container (no active_module): K=4 (2 steps, 256 rays x 32) and
    BASELINE C5's K=8 (3 steps, 1000 rays x 96 samples)."""
    check_adapt_fixture(tag, _eager_step)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bg,scale", [(True, 1.0), (False, 2.0)])
def test_volume_render_backward_matches_autograd(with_bg, scale):
    """HIP compositing backward == torch autograd of the reference formulas (ray_rendering.py:137-165),
    evaluated in float64 on the CPU, on the reference's volume_render fixture inputs (incl. saturated
    rays, clamped rgb, sigma < 0 and a sub-1e-4 step).  That fixture (two full tiles, weights below 5e-3 past sample 48, all four
    output gradients) cannot see the second tile, the last sample or the NULL-gradient branches: those are pinned by
    tests/volume_render_ref.py and tests/test_volume_render_gpu.py."""
    from adaptive_city_nerf_amd.ray_rendering import _volume_render_autograd, volume_render
    d = G.load("volume_render")
    rs = torch.from_numpy(d["rgb_sigma"]).clone()
    t = torch.from_numpy(d["t_vals"]).clone()
    bg = torch.from_numpy(d["bg"]).clone() if with_bg else None
    N, S = t.shape
    g = torch.Generator().manual_seed(9)
    gr, gd, gw, ga = torch.randn(N, 3, generator=g), torch.randn(N, generator=g), \
        torch.randn(N, S, generator=g) * 0.1, torch.randn(N, generator=g)
    rs_c = rs.double().requires_grad_(True)
    bg_c = bg.double().requires_grad_(True) if with_bg else None
    out_c = _volume_render_autograd(rs_c, t.double(), bg_c, False, False, scale)
    torch.autograd.backward(out_c, [gr.double(), gd.double(), gw.double(), ga.double()])
    rs_g = rs.cuda().requires_grad_(True)
    bg_g = bg.cuda().requires_grad_(True) if with_bg else None
    out_g = volume_render(rs_g, t.cuda(), bg_rgb=bg_g, sigma_scale=scale)
    torch.autograd.backward(out_g, [gr.cuda(), gd.cuda(), gw.cuda(), ga.cuda()])
    for a, b in zip(out_g, out_c):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=1e-4, atol=1e-5)
    ref = rs_c.grad.numpy()
    got = rs_g.grad.cpu().numpy()
    for c in range(4):
        sc = float(np.abs(ref[..., c]).max()) + 1e-12
        np.testing.assert_allclose(got[..., c], ref[..., c], rtol=0, atol=2e-5 * sc)
    if with_bg:
        np.testing.assert_allclose(bg_g.grad.cpu().numpy(), bg_c.grad.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_render_after_fused_adam_sees_updated_weights(graphed):
    """The fused Adam writes parameters through raw pointers; the packed MLP image the fused render
    caches must be rebuilt after every update (eager step and graph replay), so a render after
    adaptation equals the render of a fresh model holding the updated weights."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd import render_rays
    from adaptive_city_nerf_amd.optim import build_optimizer
    from adaptive_city_nerf_amd.train import GraphedAdaptStep, adapt_step
    d = G.load("train_k4")
    m, _ = build_model("k4")
    m.load_state_dict(reference_state_dict(d, 4, "w:"))
    m = m.cuda()
    rays = torch.from_numpy(d["train0:rays"]).cuda()
    rgbs = torch.from_numpy(d["train0:rgbs"]).cuda()
    am = 0 if graphed else None

    def render(model):
        model.eval()
        with torch.no_grad():
            out = render_rays(model, rays, ray_samples=32, active_module=am)[0].clone()
        model.train()
        return out
    before = render(m)                              # fills the packed-weight cache
    opt = build_optimizer(P, m)
    if graphed:
        g = GraphedAdaptStep(P, m, rays, rgbs, opt, active_module=0, grad_clip=1.0, warmup=1)
        for _ in range(2):
            g(rays, rgbs)
    else:
        for _ in range(2):
            adapt_step(P, m, rays, rgbs, opt, grad_clip=1.0)
    torch.cuda.synchronize()
    after = render(m)
    fresh, _ = build_model("k4")
    fresh.load_state_dict(m.state_dict())
    ref = render(fresh.cuda())
    assert not torch.equal(before, after)
    assert torch.equal(after, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["k4", "k8"])
def test_routed_pairs_path_equals_composed_chain(tag):
    """The routed-container training render on the pair kernels (routed.hip + per-expert hash grid and
    fused MLP + blend) against the composed reference structure (per-expert index_select / index_add_
    through the same expert forward): rgb, loss and every gradient."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd import ray_rendering as RR
    name_, S, _ = FIXTURES[tag]
    d = G.load(name_)
    m, _ = build_model(tag)
    m.load_state_dict(reference_state_dict(d, len(m.submodules), "w:"))
    m = m.cuda().train()
    rays = torch.from_numpy(d["train0:rays"]).cuda()
    rgbs = torch.from_numpy(d["train0:rgbs"]).cuda()
    u = torch.from_numpy(d["train0:u"]).cuda()
    res = []
    for routed in (True, False):
        RR.ROUTED_TRAIN = routed
        try:
            m.zero_grad(set_to_none=True)
            rgb = RR.render_rays(m, rays, ray_samples=S, jitter_u=u)[0]
            loss = ((rgb - rgbs) ** 2).mean()
            loss.backward()
            res.append((rgb.detach().clone(), float(loss),
                        {n: None if p.grad is None else p.grad.detach().clone() for n, p in m.named_parameters()}))
        finally:
            RR.ROUTED_TRAIN = True
    (ra, la, ga), (rb, lb, gb) = res
    # same expert kernels; the composed chain's torch norm / division may round an ulp differently
    torch.testing.assert_close(ra, rb, rtol=0, atol=1e-6)
    assert abs(la - lb) <= 1e-6 * lb
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None), n
        if ga[n] is None:
            continue
        scale = float(gb[n].abs().max()) + 1e-12
        torch.testing.assert_close(ga[n], gb[n], rtol=0, atol=1e-5 * scale, msg=n)


def _routed_step_fn(graph):
    """check_adapt_fixture step through RoutedAdaptStep (the graph-capturable routed-container step),
    built on the first call with the fixture's jitter supplied per call."""
    def fn(Pk, m, rays, rgbs, opt, u):
        from adaptive_city_nerf_amd.routed_train import RoutedAdaptStep
        st = getattr(opt, "_routed_step", None)
        if st is None:
            st = RoutedAdaptStep(Pk, m, rays.shape[0], opt, grad_clip=1.0, graph=False, jitter="given",
                                 clear_in_adam=False)
            opt._routed_step = st
            if graph:
                # one eager warm-up pass (lazy initialisation before the capture), its update undone
                snap = [t.detach().clone() for r in st.rows for t in (r[0], r[2], r[3])] + [st.step_dev.clone()]
                st(rays, rgbs, jitter_u=u)
                torch.cuda.synchronize()
                i = 0
                for r in st.rows:
                    for t in (r[0], r[2], r[3]):
                        t.detach().copy_(snap[i]); i += 1
                st.step_dev.copy_(snap[-1])
                st.replays = 0
                st.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(st.graph):
                    st._step()
                torch.cuda.synchronize()
        loss = st(rays, rgbs, jitter_u=u)
        opt.last_norm = st.last_norm
        return loss
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["k4", "k8"])
@pytest.mark.parametrize("graph", [False, True])
def test_routed_adapt_step_matches_reference_fixture(tag, graph):
    """RoutedAdaptStep (pair kernels, device-side expert activity, slotted Adam; eager and replayed as a
    HIP graph) reproduces the reference's runtime_adapt steps of the routed container."""
    check_adapt_fixture(tag, _routed_step_fn(graph))


@pytest.mark.gpu
def test_routed_step_telescoped_table_norm_equals_full_pass():
    """The tables' share of the clip norm taken from the scatter's returning atomics (sum of new^2 - old^2,
    telescoping per row) equals the sum of squares over the finished gradient buffers: same step, same
    jitter, the two modes' total norms within 1e-6 relative (double sums, different order)."""
    from adaptive_city_nerf_amd import routed_train as RT
    from adaptive_city_nerf_amd.optim import build_optimizer
    from test_module_api import build_model, reference_state_dict
    d = G.load("train_k8")
    Pk = SimpleNamespace(**{**vars(P), "ray_samples": 96, "chunk_points": 4_000_000})
    norms = []
    for tele in (True, False):
        m, _ = build_model("k8")
        m.load_state_dict(reference_state_dict(d, len(m.submodules), "w:"))
        m = m.cuda().train()
        opt = build_optimizer(Pk, m)
        was = RT.TELESCOPED_TABLE_NORM
        RT.TELESCOPED_TABLE_NORM = tele
        try:
            st = RT.RoutedAdaptStep(Pk, m, 1000, opt, grad_clip=1.0, graph=False, jitter="given")
        finally:
            RT.TELESCOPED_TABLE_NORM = was
        assert st.tele == tele
        rays = torch.from_numpy(d["train0:rays"]).cuda()
        rgbs = torch.from_numpy(d["train0:rgbs"]).cuda()
        u = torch.from_numpy(d["train0:u"]).cuda()
        st(rays, rgbs, jitter_u=u)
        st(rays, rgbs, jitter_u=u)   # second step: the Adam pass cleared the tables in between
        torch.cuda.synchronize()
        norms.append(float(st.last_norm[0]))
        assert float(st.table_sumsq[0]) == 0.0   # reset for the next step
    assert abs(norms[0] - norms[1]) <= 1e-6 * norms[1], norms


@pytest.mark.gpu
def test_background_head_backward_matches_autograd():
    """acn_background_bwd (fused re-run forward + backward of the SH-4 background MLP, per-wave sums added
    in wave order) against torch autograd of MetaContainer.background_color's composed chain, including
    directions of mixed length, zero hidden units (ReLU mask) and saturated sigmoids."""
    from adaptive_city_nerf_amd import ops
    from test_module_api import build_model
    m, _ = build_model("k4")
    m = m.cuda()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        m.bg_mlp[0].weight.copy_(torch.randn(m.bg_mlp[0].weight.shape, generator=g))
        m.bg_mlp[0].bias.copy_(torch.randn(m.bg_mlp[0].bias.shape, generator=g))
        m.bg_mlp[2].weight.copy_(torch.randn(m.bg_mlp[2].weight.shape, generator=g) * 3)
    N = 3001
    d = (torch.randn(N, 3, generator=g) * torch.rand(N, 1, generator=g) * 5).cuda()
    go = torch.randn(N, 3, generator=g).cuda()
    params = list(m.bg_mlp.parameters())
    with torch.enable_grad():
        ref = torch.autograd.grad((m.background_color(d) * go).sum(), params)
        spec, _keep = m.background_spec()
    fwd = ops.background_fwd(d, spec)
    with torch.no_grad():
        np.testing.assert_allclose(fwd.cpu().numpy(), m.background_color(d).cpu().numpy(), rtol=0, atol=2e-6)
    got = [torch.full_like(p, float("nan")) for p in params]
    ops.background_bwd(d, spec, go, got)
    for a, b in zip(got, ref):
        scale = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=1e-5 * scale)


def _runtime_adapt_step_fn():
    """check_adapt_fixture step through the drop-in train.runtime_adapt itself (steps=1 per call, one-batch
    loader): the fast path caches a RoutedAdaptStep on the optimizer -- call 1 eager + capture, calls 2..
    replay the graph; the fixture's jitter reaches the step through routed_train.JITTER, filled by the
    loader as it yields the batch."""
    from adaptive_city_nerf_amd import routed_train as RT
    from adaptive_city_nerf_amd import train as T

    def fn(Pk, m, rays, rgbs, opt, u):
        st = getattr(opt, "_u_static", None)
        if st is None:
            st = opt._u_static = torch.zeros_like(u)

        def loader():
            st.copy_(u)
            yield rays, rgbs
        out = T.runtime_adapt(P=Pk, model=m, data_loader=list(loader()), optimizer=opt, steps=1)
        step = next(iter(opt._acn_routed_steps.values()))
        opt.last_norm = step.last_norm
        return out["loss"]
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["k4", "k8"])
def test_runtime_adapt_drop_in_uses_graphed_routed_step(tag, monkeypatch):
    """train.runtime_adapt (the function INTEGRATION.md swaps in for runtime_adapt.py:213-315) goes through
    the cached, graph-replayed RoutedAdaptStep and reproduces the reference's runtime_adapt steps: loss,
    clip norm and parameters after every step."""
    from adaptive_city_nerf_amd import routed_train as RT
    holder = {}
    monkeypatch.setattr(RT, "JITTER", lambda n, S, dev: holder["opt"]._u_static[:n])

    def make_opt(Pk, m):
        from adaptive_city_nerf_amd.optim import build_optimizer
        holder["opt"] = build_optimizer(Pk, m)
        return holder["opt"]
    m, opt = check_adapt_fixture(tag, _runtime_adapt_step_fn(), make_opt=make_opt, check_grads=False)
    st = next(iter(opt._acn_routed_steps.values()))
    nsteps = FIXTURES[tag][2]
    assert st.graph is not None and st.replays == nsteps - 1 and st.steps_done == nsteps
    # runtime_adapt leaves the host optimizer state current (state_dict): the shared head stepped every time
    for p in m.bg_mlp.parameters():
        assert float(opt.state[p]["step"]) == float(nsteps)


@pytest.mark.gpu
def test_runtime_adapt_ragged_batches_match_eager_steps(monkeypatch):
    """A loader whose last batch is short (drop_last=False): full batches replay the graph, the short one
    runs the same kernels eagerly through the step object's buffers; the parameters equal those of the
    eager adapt_step loop on the same batches and jitter (pair kernels vs the same kernels without the
    graph: identical launches, so identical up to float-atomic ordering)."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd import routed_train as RT
    from adaptive_city_nerf_amd import train as T
    from adaptive_city_nerf_amd.optim import build_optimizer
    d = G.load("train_k8")
    Pk = SimpleNamespace(**{**vars(P), "ray_samples": 96, "chunk_points": 4_000_000})
    rays = torch.from_numpy(d["train0:rays"]).cuda()
    rgbs = torch.from_numpy(d["train0:rgbs"]).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    sizes = [1000, 1000, 1000, 600]
    batches = []
    for n in sizes:
        sel = torch.randperm(1000, device="cuda", generator=g)[:n]
        batches.append((rays[sel].contiguous(), rgbs[sel].contiguous(), torch.rand(n, 96, device="cuda", generator=g)))
    results = []
    for fast in (True, False):
        m, _ = build_model("k8")
        m.load_state_dict(reference_state_dict(d, 8, "w:"))
        m = m.cuda().train()
        opt = build_optimizer(Pk, m)
        if fast:
            ustat = torch.zeros(1000, 96, device="cuda")
            monkeypatch.setattr(RT, "JITTER", lambda n, S, dev: ustat[:n])

            def loader():
                for r, c, u in batches:
                    ustat[:u.shape[0]].copy_(u)
                    yield r, c
            out = T.runtime_adapt(P=Pk, model=m, data_loader=loader(), optimizer=opt)
            st = next(iter(opt._acn_routed_steps.values()))
            assert st.replays == 2 and st.steps_done == 4 and out["steps"] == 4
        else:
            for r, c, u in batches:
                T.adapt_step(Pk, m, r, c, opt, grad_clip=1.0, jitter_u=u)
        torch.cuda.synchronize()
        results.append(({n: p.detach().clone() for n, p in m.named_parameters()},
                        {n: float(opt.state[p]["step"]) for n, p in m.named_parameters() if p in opt.state}))
    (pa, sa), (pb, sb) = results
    assert sa == sb   # the same experts stepped the same number of times
    for n in pa:
        lr = 0.01 if n.endswith("hash_table") else 0.001 if n.startswith("bg_mlp") else 0.002
        assert _close_frac(pa[n].cpu().numpy(), pb[n].cpu().numpy(), 1e-3 * lr, 1e-6) >= 0.95, n


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("graph", [False, True])
def test_routed_step_deterministic_at_pre_round_bounds(precision, graph):
    """the reference's K=8 runtime_adapt steps (train_k8.npz, 3 steps at 1000 rays x 96) replayed
    through RoutedAdaptStep under torch.use_deterministic_algorithms(True) -- the table gradients by the
    sort-based backward (every row the serial sum in sample order), the tables' norm share by a double
    reduction; a graph=True object runs such steps eagerly -- pass at the bounds the fixture replay had
    before round 2 loosened them: gradients within 1e-4 of their scale at step 0 and 1e-3 later, >= 99% of
    every parameter tensor within 1e-3 lr at every step.  Both training-MLP precisions; two runs are
    bitwise identical."""
    from adaptive_city_nerf_amd import ops
    from adaptive_city_nerf_amd.routed_train import RoutedAdaptStep
    was = ops.TRAIN_MLP_PRECISION
    ops.set_train_mlp_precision(precision)
    torch.use_deterministic_algorithms(True)
    try:
        finals = []
        for run in range(2):
            def fn(Pk, m, rays, rgbs, opt, u):
                st = getattr(opt, "_det_step", None)
                if st is None:
                    st = opt._det_step = RoutedAdaptStep(Pk, m, rays.shape[0], opt, grad_clip=1.0, graph=graph,
                                                         warmup=1, jitter="given", clear_in_adam=False)
                loss = st(rays, rgbs, jitter_u=u)
                opt.last_norm = st.last_norm
                return loss
            # exact-fp32 layer products land farther from the reference's MKL sums than the fp16x3 split
            # (profiles/r03_train_parity_spread.json: step-2 parameter fraction 0.981 vs 0.9995), so that
            # precision keeps the round-2 bounds
            m, opt = check_adapt_fixture("k8", fn, gtol_later=1e-3 if precision == "fp16x3" else 3e-3,
                                         need_later=0.99 if precision == "fp16x3" else 0.95)
            assert opt._det_step.graph is None and opt._det_step.replays == 0
            finals.append({n: p.detach().clone() for n, p in m.named_parameters()})
        for n in finals[0]:
            assert torch.equal(finals[0][n], finals[1][n]), n
    finally:
        torch.use_deterministic_algorithms(False)
        ops.set_train_mlp_precision(was)


@pytest.mark.gpu
def test_adam_segment_maps_bitwise_equal_dense_over_10_steps(monkeypatch):
    """VERDICT r02 "Next" 6: the segment-mapped Adam (never-touched 64-B table segments skipped, no gradient
    read where this step added nothing) leaves parameters and both moments BITWISE equal to the dense update
    over 10 routed runtime_adapt steps (train_k8.npz's three batches cycled; deterministic table backward so
    the runs see identical gradients), in one pass and split into the early (untouched-now segments, before
    the clip coefficient) and late passes; and it does skip: after step 1 only part of the tables is marked."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd import routed_train as RT
    from adaptive_city_nerf_amd.optim import build_optimizer
    d = G.load("train_k8")
    Pk = SimpleNamespace(**{**vars(P), "ray_samples": 96, "chunk_points": 4_000_000})
    batches = [(torch.from_numpy(d[f"train{s}:rays"]).cuda(), torch.from_numpy(d[f"train{s}:rgbs"]).cuda(),
                torch.from_numpy(d[f"train{s}:u"]).cuda()) for s in range(3)]
    torch.use_deterministic_algorithms(True)
    try:
        out, frac = [], None
        # segment-mapped in one pass, segment-mapped split into the early + late passes (ADAM_EARLY), dense
        for seg_on, early in ((True, False), (True, True), (False, False)):
            monkeypatch.setattr(RT, "ADAM_SEGMAP", seg_on)
            monkeypatch.setattr(RT, "ADAM_EARLY", early)
            m, _ = build_model("k8")
            m.load_state_dict(reference_state_dict(d, 8, "w:"))
            m = m.cuda().train()
            opt = build_optimizer(Pk, m)
            st = RT.RoutedAdaptStep(Pk, m, 1000, opt, grad_clip=1.0, graph=False, jitter="given")
            assert (st.segmaps is not None) == seg_on and (st.adam.segmaps is not None) == seg_on
            assert st.early == early
            for i in range(10):
                r, c, u = batches[i % 3]
                st(r, c, jitter_u=u)
                if seg_on and i == 0:
                    ever, total = st.segment_stats()
                    frac = ever / total
            torch.cuda.synchronize()
            st.sync_state()
            out.append({n: (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                        for n, p in m.named_parameters() if p in opt.state})
        assert 0.0 < frac < 0.5, frac
        for o in out[:2]:
            assert o.keys() == out[2].keys()
            for n in o:
                for a, b in zip(o[n], out[2][n]):
                    assert torch.equal(a, b), n
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.gpu
def test_runtime_adapt_alternating_active_module_keeps_adam_state(monkeypatch):
    """an eager single-expert update (runtime_adapt's active_module path) between routed
    runtime_adapt calls on the same optimizer.  The cached RoutedAdaptStep must pick up that update: the
    expert's step counter, its moments (first-updated parameters included) and -- with the segment-mapped
    Adam -- every table segment the eager step touched, whose moments keep decaying in later routed steps.
    Parameters, moments and step counts equal the all-eager sequence: in particular on the table rows the
    eager step moved (a missed 'ever' mark would leave them un-updated, an lr-sized difference)."""
    from test_module_api import build_model, reference_state_dict
    from adaptive_city_nerf_amd import routed_train as RT
    from adaptive_city_nerf_amd import train as T
    from adaptive_city_nerf_amd.optim import build_optimizer
    d = G.load("train_k8")
    Pk = SimpleNamespace(**{**vars(P), "ray_samples": 96, "chunk_points": 4_000_000})
    rays = torch.from_numpy(d["train0:rays"]).cuda()
    rgbs = torch.from_numpy(d["train0:rgbs"]).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    batches = []
    for _ in range(4):
        sel = torch.randperm(1000, device="cuda", generator=g)
        batches.append((rays[sel].contiguous(), rgbs[sel].contiguous(), torch.rand(1000, 96, device="cuda", generator=g)))
    K_EAGER = 3
    results, moved = [], None
    for fast in (True, False):
        m, _ = build_model("k8")
        m.load_state_dict(reference_state_dict(d, 8, "w:"))
        m = m.cuda().train()
        opt = build_optimizer(Pk, m)
        ustat = torch.zeros(1000, 96, device="cuda")
        monkeypatch.setattr(RT, "JITTER", lambda n, S, dev: ustat[:n])
        tab = m.submodules[K_EAGER].xyz_encoder.hash_table
        for i, (r, c, u) in enumerate(batches):
            if i == 1:      # the eager single-expert update (runtime_adapt.py with active_module)
                before = tab.detach().clone()
                T.adapt_step(Pk, m.submodules[K_EAGER], r, c, opt, active_module=K_EAGER, grad_clip=1.0, jitter_u=u)
                if not fast:
                    moved = (tab.detach() != before).any(dim=1)
            elif fast:
                ustat.copy_(u)
                T.runtime_adapt(P=Pk, model=m, data_loader=[(r, c)], optimizer=opt, steps=1)
            else:
                T.adapt_step(Pk, m, r, c, opt, grad_clip=1.0, jitter_u=u)
        torch.cuda.synchronize()
        if fast:
            assert next(iter(opt._acn_routed_steps.values())).steps_done == 3
        results.append(({n: p.detach().clone() for n, p in m.named_parameters()},
                        {n: float(opt.state[p]["step"]) for n, p in m.named_parameters() if p in opt.state},
                        {n: opt.state[p]["exp_avg"].clone() for n, p in m.named_parameters() if p in opt.state}))
    (pa, sa, ma), (pb, sb, mb) = results
    assert sa == sb
    assert int(moved.sum()) > 1000
    for n in pa:
        lr = 0.01 if n.endswith("hash_table") else 0.001 if n.startswith("bg_mlp") else 0.002
        assert _close_frac(pa[n].cpu().numpy(), pb[n].cpu().numpy(), 1e-3 * lr, 1e-6) >= 0.95, n
    key = f"submodules.{K_EAGER}.xyz_encoder.hash_table"
    a, b = pa[key][moved].cpu().numpy(), pb[key][moved].cpu().numpy()
    assert _close_frac(a, b, 1e-3 * 0.01, 1e-6) >= 0.99, "rows the eager step moved diverge after routed steps"
    a, b = ma[key][moved].cpu().numpy(), mb[key][moved].cpu().numpy()
    assert _close_frac(a, b, 1e-3 * float(np.abs(b).max()), 1e-3) >= 0.99
