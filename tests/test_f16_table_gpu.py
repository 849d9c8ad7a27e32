"""fp16 render tables (HashGridEncoder.set_render_table_dtype) on the GPU.

The oracle is the project's own fp32 path: fp16 -> fp32 widening is exact and the interpolation stays the same fp32
operations, so every output of the fp16 mode must equal, BIT FOR BIT (torch.equal, no tolerance), the fp32 mode of a
model whose table was replaced by ``table.half().float()``.  The reference models are built once per configuration
and never modified."""
from functools import lru_cache

import pytest
import torch

import goldens as G
import test_input_grad_gpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32


def _ops():
    from adaptive_city_nerf_amd import ops
    return ops


def _encoders(m):
    subs = getattr(m, "submodules", None)
    return [s.xyz_encoder for s in subs] if subs is not None else [m.xyz_encoder]


def _k2_container():
    """The first two experts of the k4 scene as a soft-routed container of their own (render_kernel's K == 2 case)."""
    from adaptive_city_nerf_amd import MetaContainer, SceneBox
    sc = G.scene()["masks"][G.MASK["k4"]]
    gbox = SceneBox(aabb=torch.tensor(sc["aabb_global"], dtype=torch.float32))
    boxes = [SceneBox(aabb=torch.tensor([sc["mins"][k], sc["maxs"][k]], dtype=torch.float32)) for k in range(2)]
    torch.manual_seed(0)
    m = MetaContainer(num_submodules=2, centroids=torch.tensor(sc["centroids"][:2]), aabb=gbox.aabb,
                      nerf_variant="instant", boundary_margin=1.05, cluster_2d=sc["cluster_2d"], joint_training=False,
                      use_bg_nerf=True, bg_hidden=32, bg_encoding="spherical", occ_conf={"use_occ": False},
                      expert_box_list=boxes, hidden=64, sigma_depth=2, color_depth=2, dir_encoding="spherical",
                      color_hidden=64, use_sigmoid_rgb=True, hash_enc_conf=T.HASH_CONF).to(DEV)
    return m.eval().requires_grad_(False)


def _build(K, interp="Linear", log2T=12, scale=0.5):
    """The K = 1 expert / K = 4 container of test_input_grad_gpu (same seeds, so two builds hold the same weights),
    with this interpolation and table size, tables U(-scale, scale)."""
    old = dict(T.HASH_CONF)
    T.HASH_CONF.update(interpolation=interp, log2_hashmap_size=log2T)
    try:
        m = T._expert() if K == 1 else (T._container("k4")[0] if K == 4 else _k2_container())
    finally:
        T.HASH_CONF.clear()
        T.HASH_CONF.update(old)
    gen = torch.Generator(device=DEV).manual_seed(1234 + K)
    with torch.no_grad():
        for enc in _encoders(m):
            enc.hash_table.uniform_(-scale, scale, generator=gen)
    return m


def _rounded_copy(m, K, interp, log2T):
    """A second model with m's weights and ``table.half().float()`` as its fp32 table: the oracle's model."""
    ref = _build(K, interp, log2T)
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():
        for enc in _encoders(ref):
            enc.hash_table.copy_(enc.hash_table.half().float())
    return ref


@lru_cache(maxsize=None)
def _pair(K, interp="Linear", log2T=12, scale=0.5):
    """(model in fp16 mode, fp32 model on the rounded table); shared between the tests, never modified."""
    m = _build(K, interp, log2T, scale)
    ref = _rounded_copy(m, K, interp, log2T)
    m.set_render_table_dtype(F16)
    assert all(e.render_table_dtype == F16 for e in _encoders(m))
    assert all(e.render_table_dtype == F32 for e in _encoders(ref))
    return m, ref


def _box(m):
    if hasattr(m, "submodules"):
        v = m.scene_aabb_vec.cpu()
        return v[:3], v[3:]
    return m.scene_box.min.cpu(), m.scene_box.max.cpu()


def _rays(m, n, seed):
    """n rays from above the model's box towards points inside it; far reaches past the box (clamped samples)."""
    lo, hi = _box(m)
    g = torch.Generator().manual_seed(seed)
    c, e = 0.5 * (lo + hi), hi - lo
    o = c + e * (torch.rand(n, 3, generator=g) - 0.5) * 0.4
    o[:, 2] = hi[2] + 0.75 * e[2]
    d = lo + e * torch.rand(n, 3, generator=g) - o
    d = d / d.norm(dim=-1, keepdim=True)
    near = torch.full((n, 1), 0.05)
    far = torch.full((n, 1), float(2.0 * e.norm()))
    return torch.cat([o, d, near, far], 1).float().contiguous().to(DEV)


def _points(m, n, seed):
    """(n, 6) field inputs: random points of the box, plus (n >= 16) points outside it on every side (the clamps
    to 1e-6 and 1 - 1e-6), the box centre and quarter points (exact lattice points of the even resolutions)."""
    lo, hi = _box(m)
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand(n, 3, generator=g)
    if n >= 16:
        e = hi - lo
        x[0], x[1], x[2] = lo - 0.5 * e, hi + 0.5 * e, lo
        x[3], x[4], x[5] = hi, 0.5 * (lo + hi), lo + 0.25 * e
        x[6] = lo + e * torch.tensor([0.75, 0.5, 0.25])
        x[7] = torch.stack([lo[0] - 1.0, 0.5 * (lo[1] + hi[1]), hi[2] + 1.0])
    return torch.cat([x, torch.randn(n, 3, generator=g)], -1).float().contiguous().to(DEV)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ conversion
@pytest.mark.parametrize("n", [1, 3, 7, 4099])
def test_table_to_f16_equals_half_bitwise(n):
    g = torch.Generator().manual_seed(n)
    # 1e-3 scale: about 6 % of the values land among the fp16 subnormals (|v| < 2^-14)
    src = torch.cat([torch.randn(n - n // 2, generator=g) * 1e-3, torch.randn(n // 2, generator=g) * 0.5]).to(DEV)
    got = _ops().table_to_f16(src)
    assert got.dtype == F16 and got.shape == src.shape
    assert torch.equal(got.view(torch.int16), src.half().view(torch.int16))
    assert torch.equal(got.cpu().view(torch.int16), src.cpu().half().view(torch.int16))


def test_table_to_f16_special_values():
    inf, nan = float("inf"), float("nan")
    cases = [                              # (fp32 value, expected fp16 value)
        (0.0, 0.0), (-0.0, -0.0),
        (2.0 ** -24, 2.0 ** -24),                    # smallest fp16 subnormal
        (3 * 2.0 ** -24, 3 * 2.0 ** -24), (-(2.0 ** -15), -(2.0 ** -15)),   # subnormals kept, not flushed
        (1023 * 2.0 ** -24, 1023 * 2.0 ** -24),      # largest subnormal
        (2.0 ** -14, 2.0 ** -14),                    # smallest normal
        (2.0 ** -25, 0.0),                           # tie between 0 and 2^-24: to even
        (3 * 2.0 ** -25, 2.0 ** -23),                # tie between 2^-24 and 2^-23: to even
        (2.0 ** -25 * 1.0000001, 2.0 ** -24),        # just above the tie
        (1.0 + 2.0 ** -11, 1.0),                     # tie: to even (down)
        (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9),     # tie: to even (up)
        (-(1.0 + 2.0 ** -11), -1.0),
        (65504.0, 65504.0), (65519.0, 65504.0),
        (65520.0, inf), (-65520.0, -inf),            # the tie above the largest finite value rounds to inf
        (1e6, inf), (inf, inf), (-inf, -inf), (nan, nan),
    ]
    src = torch.tensor([c[0] for c in cases], dtype=F32)
    want = torch.tensor([c[1] for c in cases], dtype=torch.float64).to(F16)
    assert torch.equal(src[:-1].half().view(torch.int16), want[:-1].view(torch.int16))   # the table above is right
    got = _ops().table_to_f16(src.to(DEV)).cpu()
    assert torch.equal(got[:-1].view(torch.int16), want[:-1].view(torch.int16)), (got, want)
    assert bool(torch.isnan(got[-1]))
    # widening back is exact: the values the kernels interpolate are table.half().float()
    assert torch.equal(got[:-1].float(), src[:-1].half().float())


def test_table_to_f16_writes_into_a_given_buffer():
    src = torch.randn(33, 2, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = torch.zeros(33, 2, dtype=F16, device=DEV)
    assert _ops().table_to_f16(src, out=out) is out and torch.equal(out, src.half())
    with pytest.raises(ValueError):
        _ops().table_to_f16(src, out=torch.zeros(33, 2, device=DEV))


# ------------------------------------------------------------------------------------------------ field forward
FIELD_CASES = [("Linear", 12, 0.5), ("Smoothstep", 12, 0.5), ("Linear", 12, 1e-3), ("Smoothstep", 12, 1e-3),
               ("Linear", 20, 1e-3)]


def _both_parities_on_every_level(m, x):
    enc = _encoders(m)[0]
    sub = m.submodules[0] if hasattr(m, "submodules") else m
    x01 = sub._world_to_unit(x[:, :3])
    for r in enc._res_host:
        x0 = torch.floor(x01[:, 0] * float(r)).long() & 1
        if not (bool((x0 == 0).any()) and bool((x0 == 1).any())):
            return False
    return True


@pytest.mark.parametrize("interp, log2T, scale", FIELD_CASES)
def test_field_forward_single_expert(interp, log2T, scale):
    m, ref = _pair(1, interp, log2T, scale)
    x = _points(m, 1000, seed=40)
    assert _both_parities_on_every_level(m, x)      # the paired gather and the odd-x0 second-row gather both run
    if scale == 1e-3:
        t = _encoders(ref)[0].hash_table
        sub = (t != 0) & (t.abs() < 2.0 ** -14)
        assert 0.03 < float(sub.float().mean()) < 0.09   # fp16 subnormals: a flushing conversion would zero them
    with torch.no_grad():
        for M in (1, 31, 33, 1000):
            got, want = m(x[:M]), ref(x[:M])
            assert got.shape == (M, 4) and torch.equal(got, want), M
        # the mode is on: the unrounded fp32 table gives other bits
        m32 = _build(1, interp, log2T, scale) if log2T == 12 else None
        if m32 is not None:
            assert not torch.equal(m32(x), m(x))


@pytest.mark.parametrize("interp, log2T, scale", FIELD_CASES[:4])
def test_field_forward_container(interp, log2T, scale):
    m, ref = _pair(4, interp, log2T, scale)
    gbox = type("B", (), {"min": _box(m)[0], "max": _box(m)[1]})
    pts = T._container_points(m, gbox, 1000, seed=41)       # half of them near the bisectors: blended experts
    x = _points(m, 1000, seed=42)
    x[16:, :3] = pts[16:]
    ops = _ops()
    with torch.no_grad():
        w, _ = ops.routing_fwd(x[:, :3].contiguous(), m.routing_spec())
        assert bool(((w > 0).sum(-1) > 1).any())            # soft routing blends experts here
        for M in (1, 31, 33, 1000):
            assert torch.equal(m(x[:M]), ref(x[:M])), M                                          # K = 4, soft
            assert torch.equal(m(x[:M], active_module=2), ref(x[:M], active_module=2)), M        # K = 1
        # ops.field_fwd with explicitly built specs
        specs16, specs32 = m.expert_specs(render_table=True), ref.expert_specs()
        assert all(s.s.table_fmt == 1 for s in specs16) and all(s.s.table_fmt == 0 for s in specs32)
        r = m.routing_spec()
        assert torch.equal(ops.field_fwd(x, specs16, r), ops.field_fwd(x, specs32, ref.routing_spec()))


# ------------------------------------------------------------------------------------------------ renders
# (K, tau, sample counts): one case per kernel launch_render can select
RENDER_CASES = {
    "ws_k1": (1, 0.0, (32, 64)),             # render_ws_kernel
    "render_k1_tau": (1, 1e-3, (32, 64)),    # render_kernel, one expert
    "render_k2": (2, 0.0, (32, 64)),         # render_kernel, two routed experts in LDS
    "wss16_k4": (4, 0.0, (32, 64)),          # render_wss_kernel, 16-ray rounds (S <= 128)
    "wss8_k4": (4, 0.0, (160,)),             # render_wss_kernel, 8-ray rounds (128 < S <= 256)
    "slots_k4_tau": (4, 1e-3, (32, 64)),     # render_slots_kernel
}


def _render(model, rays, S, tau, u):
    from adaptive_city_nerf_amd import render_rays
    model.train(u is not None)               # training mode draws the jitter (given here); eval renders without
    try:
        with torch.no_grad():
            return render_rays(model, rays, ray_samples=S, early_stop_tau=tau, jitter_u=u)
    finally:
        model.eval()


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
@pytest.mark.parametrize("case", list(RENDER_CASES))
def test_render_rays_equal_fp32_on_the_rounded_table(case, interp, jitter):
    K, tau, Ss = RENDER_CASES[case]
    m, ref = _pair(K, interp)
    rays = _rays(m, 1000, seed=50 + K)
    for S in Ss:
        u = torch.rand(1000, S, generator=torch.Generator().manual_seed(60 + S)).to(DEV) if jitter else None
        for N in (1, 257, 1000):
            un = None if u is None else u[:N].contiguous()
            got, want = _render(m, rays[:N].contiguous(), S, tau, un), _render(ref, rays[:N].contiguous(), S, tau, un)
            assert got[2].shape == (N, S) and float(got[3].max()) > 0.0
            for name, a, b in zip(("rgb", "depth", "weights", "acc"), got, want):
                assert torch.equal(a, b), (case, S, N, name, float((a - b).abs().max()))


def test_render_default_init_scale_and_run_to_run():
    """The reference's table (log2T = 20, U(-1e-3, 1e-3): fp16 subnormals among the entries), a C2-like small batch."""
    m, ref = _pair(1, "Linear", 20, 1e-3)
    rays = _rays(m, 1000, seed=70)
    a, b, want = _render(m, rays, 64, 0.0, None), _render(m, rays, 64, 0.0, None), _render(ref, rays, 64, 0.0, None)
    assert _same(a, b)
    assert _same(a, want)


# ------------------------------------------------------------------------------------------------ cache
def test_shadow_follows_the_parameter():
    m = _build(1)
    rays = _rays(m, 257, seed=80)
    keys = {k: v.dtype for k, v in m.state_dict().items()}
    ckpt = {k: v.clone() for k, v in m.state_dict().items()}
    first32 = _render(m, rays, 32, 0.0, None)
    m.set_render_table_dtype(F16)
    enc = m.xyz_encoder
    assert _same(_render(m, rays, 32, 0.0, None), _render(_rounded_copy(m, 1, "Linear", 12), rays, 32, 0.0, None))
    # not a parameter, not a buffer, not in the state dict
    assert {k: v.dtype for k, v in m.state_dict().items()} == keys
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in _build(1).named_parameters()]
    assert all(b.dtype != F16 for b in m.buffers())
    shadow = enc.render_table()
    assert shadow.dtype == F16 and shadow.shape == enc.hash_table.shape and enc.render_table() is shadow
    # in-place edit
    with torch.no_grad():
        enc.hash_table.mul_(1.5)
    assert _same(_render(m, rays, 32, 0.0, None), _render(_rounded_copy(m, 1, "Linear", 12), rays, 32, 0.0, None))
    assert torch.equal(enc.render_table(), enc.hash_table.detach().half())
    # optimizer step
    opt = torch.optim.Adam([enc.hash_table], lr=1e-2)
    enc.hash_table.grad = torch.randn(enc.hash_table.shape, generator=torch.Generator().manual_seed(81)).to(DEV)
    opt.step()
    enc.hash_table.grad = None
    assert _same(_render(m, rays, 32, 0.0, None), _render(_rounded_copy(m, 1, "Linear", 12), rays, 32, 0.0, None))
    # a checkpoint from before the switch existed
    m.load_state_dict(ckpt)
    assert torch.equal(enc.render_table(), ckpt["xyz_encoder.hash_table"].half())
    assert _same(_render(m, rays, 32, 0.0, None), _render(_rounded_copy(m, 1, "Linear", 12), rays, 32, 0.0, None))
    # and back: the original fp32 render
    m.set_render_table_dtype(F32)
    assert enc.render_table() is enc.hash_table
    assert _same(_render(m, rays, 32, 0.0, None), first32)
    for bad in (torch.bfloat16, torch.float64, None, "float16"):
        with pytest.raises(ValueError):
            m.set_render_table_dtype(bad)
    assert enc.render_table_dtype == F32


def test_container_switch_reaches_every_expert():
    m = _build(4)
    m.set_render_table_dtype(F16)
    assert all(e.render_table_dtype == F16 for e in _encoders(m))
    m.set_render_table_dtype(F32)
    assert all(e.render_table_dtype == F32 for e in _encoders(m))
    with pytest.raises(ValueError):
        m.set_render_table_dtype(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ training untouched
def _train_pass(m, rays, wr, diff_rays):
    from adaptive_city_nerf_amd import render_rays
    for p in m.parameters():
        p.grad = None
    r = rays.clone().requires_grad_() if diff_rays else rays
    out = render_rays(m, r, ray_samples=16)
    assert out[0].grad_fn is not None
    ((out[0] * wr).sum() + out[1].sum()).backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return [o.detach().clone() for o in out], grads, (r.grad.clone() if diff_rays else None)


@pytest.mark.parametrize("diff_rays", [False, True])
def test_training_path_is_untouched(diff_rays):
    m = _build(1).train(False)
    assert all(p.requires_grad for p in m.parameters())
    rays = _rays(m, 64, seed=90)
    wr = torch.randn(64, 3, generator=torch.Generator().manual_seed(91)).to(DEV)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)   # selects the sorted (bitwise) table backward
    try:
        out0, g0, gr0 = _train_pass(m, rays, wr, diff_rays)
        m.set_render_table_dtype(F16)
        _render(m, rays, 16, 0.0, None)                   # the shadow exists and is in use
        out1, g1, gr1 = _train_pass(m, rays, wr, diff_rays)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert _same(out0, out1)
    assert "xyz_encoder.hash_table" in g0 and len(g0) == 15 and g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert float(g0["xyz_encoder.hash_table"].abs().max()) > 0
    if diff_rays:
        assert torch.equal(gr0, gr1) and float(gr0[:, :6].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_nearest_is_refused_when_the_spec_is_built():
    from adaptive_city_nerf_amd._lib import AcnError
    m = _build(1, interp="Nearest")
    x = _points(m, 33, seed=95)
    with torch.no_grad():
        want = m(x)
        m.set_render_table_dtype(F16)
        with pytest.raises(AcnError, match="Nearest"):
            m.expert_spec(render_table=True)
        with pytest.raises(AcnError, match="Nearest"):
            m(x)
        assert "_render_shadow" not in m.xyz_encoder.__dict__      # refused before anything was converted or launched
        assert m.expert_spec().s.table_fmt == 0                    # the fp32 callers are still served
        m.set_render_table_dtype(F32)
        assert torch.equal(m(x), want)


def test_expert_spec_checks_the_table_size():
    from adaptive_city_nerf_amd._lib import AcnError
    ops = _ops()
    m = _build(1)
    enc = m.xyz_encoder
    mn, ext = m._host_box()
    mlp = m._mlp_tensors(None)
    full = enc.hash_table.detach()
    ok = ops.ExpertSpec(full.half(), enc._res_host, 12, 1, mn, ext, mlp, table_fmt=1)
    assert ok.s.table_fmt == 1
    with pytest.raises(AcnError, match="bytes"):
        ops.ExpertSpec(full.half()[:-1], enc._res_host, 12, 1, mn, ext, mlp, table_fmt=1)
    with pytest.raises(AcnError, match="bytes"):
        ops.ExpertSpec(full[: full.shape[0] // 2], enc._res_host, 12, 1, mn, ext, mlp)
    with pytest.raises(AcnError, match="float16"):
        ops.ExpertSpec(full, enc._res_host, 12, 1, mn, ext, mlp, table_fmt=1)
    with pytest.raises(AcnError, match="table_fmt"):
        ops.ExpertSpec(full, enc._res_host, 12, 1, mn, ext, mlp, table_fmt=7)


def test_occupancy_renderer_keeps_the_fp32_table():
    """The rule for the occupancy renderer: it keeps reading the fp32 parameter, switch on or off (same bits)."""
    from adaptive_city_nerf_amd import render_rays
    from test_occ_gpu import model_from_fixture
    m, d = model_from_fixture("k1")
    rays = torch.from_numpy(d["rays"]).to(DEV)
    with torch.no_grad():
        off = render_rays(m, rays)
        m.set_render_table_dtype(F16)
        on = render_rays(m, rays)
        sig_on = m.submodules[0].density(rays[:, :3]) if hasattr(m, "submodules") else m.density(rays[:, :3])
        m.set_render_table_dtype(F32)
        sig_off = m.submodules[0].density(rays[:, :3]) if hasattr(m, "submodules") else m.density(rays[:, :3])
    assert _same(off, on) and float(off[3].max()) > 0
    assert torch.equal(sig_on, sig_off)          # density (occupancy updates, marching) stays on fp32 too


def test_expert_parallel_renderer_keeps_the_fp32_table():
    """The rule for ExpertParallelRenderer: its specs are the fp32 ones, switch on or off (same bits); the C entry
    point itself refuses an fp16 expert."""
    import ctypes as C
    from adaptive_city_nerf_amd import _lib
    from adaptive_city_nerf_amd.expert_parallel import ExpertParallelRenderer
    m = _build(4)
    rays = _rays(m, 257, seed=97)
    with torch.no_grad():
        off = [x.clone() for x in ExpertParallelRenderer(m, 257, 32, want_weights=True)(rays)]
        fused32 = _render(m, rays, 32, 0.0, None)
        m.set_render_table_dtype(F16)
        on = [x.clone() for x in ExpertParallelRenderer(m, 257, 32, want_weights=True)(rays)]
        fused16 = _render(m, rays, 32, 0.0, None)
    assert _same(off, on) and float(off[3].max()) > 0
    assert not torch.equal(fused16[0], fused32[0])          # while the stratified render did change
    # C ABI: acn_ep_field_fwd with an fp16 expert
    spec = m.submodules[0].expert_spec(render_table=True)
    assert spec.s.table_fmt == 1
    buf = torch.zeros(int(_lib.lib().acn_workspace_bytes(1)) // 4 + 64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = _lib.lib().acn_ep_field_fwd(_lib.ptr(buf), _lib.ptr(cnt), 1, 1, 32, C.byref(spec.s), _lib.ptr(buf),
                                     int(_lib.lib().acn_workspace_bytes(1)), _lib.ptr(buf), None)
    assert st == -2
