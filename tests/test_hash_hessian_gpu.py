"""Second-order point gradients of the hash grid: the double-backward kernels against the float64
formulas of tests/hash_hessian_ref.py, their determinism, the autograd wiring inside ray_rendering.second_order()
and MetaNGP.density_and_gradient end to end.

Tolerances.  Gather kernel: 4e-6 * B elementwise, B the sum of the absolute terms -- the first-order kernel's 2e-6 * B
covers ~32 fp32 roundings; the second-order chains add the v * r * S' products, the three-axis sum, r^2 and S'', which
stays under 64 roundings (64 * 2^-24 = 3.8e-6).  Scatter kernel: (n_row + 16) * 2^-24 * B_row per element, n_row - 1
roundings for the atomic sum of n_row terms and at most 16 per term.  End to end: max(2e-5, 4 * e32) relative to
max(1, max|ref|), e32 the float32-against-float64 error of the same restatement on the CPU."""
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F_

import hash_hessian_ref as H
import input_grad_ref as R
import test_input_grad_gpu as TI
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
GENERIC = TI.GENERIC
F2_LOOP = "f2_L5_T10"            # F == 2 and L no power of two: the per-point level loop of the buffer form
CASES = ["smooth_L16_T12", "lin_L16_T20", "lin_L8_T14_r2_512", GENERIC, F2_LOOP]


def _ops():
    from adaptive_city_nerf_amd import ops
    return ops


@lru_cache(maxsize=None)
def _case(name):
    """(x01, g, v, table, res, log2T, F, interp) on the GPU; shared, never modified."""
    if name == F2_LOOP:
        from adaptive_city_nerf_amd.synthetic import formula_table
        x = TI._case(GENERIC)[0]
        L, log2T, F, interp, seed = 5, 10, 2, 2, 23
        res = O.level_resolutions(5, 16, 256).tolist()
        tab = torch.from_numpy(formula_table(L, log2T, F, seed=seed, scale=0.5)).to(DEV)
        g = torch.randn(x.shape[0], L * F, generator=torch.Generator().manual_seed(seed + 100)).to(DEV)
    else:
        x, g, tab, res, log2T, F, interp = TI._case(name)
        seed = 0
    v = torch.randn(x.shape[0], 3, generator=torch.Generator().manual_seed(seed + 200)).to(DEV)
    return x, g, v, tab, res, log2T, F, interp


@lru_cache(maxsize=None)
def _ref(name):
    x, g, v, tab, res, log2T, F, interp = _case(name)
    return H.double_backward(x, g, v, tab, res, log2T, interp)


@lru_cache(maxsize=None)
def _full(name):
    x, g, v, tab, res, log2T, F, interp = _case(name)
    return _ops().hashgrid_bwd_input_bwd(x, g, v, tab, res, log2T, F, interp)


@pytest.mark.parametrize("name", CASES)
def test_gather_kernel_vs_float64_formulas(name):
    ref = _ref(name)
    for got, val, scale in zip(_full(name), ("gg", "gx2"), ("B_gg", "B_x")):
        got, want, B = got.double(), ref[val], ref[scale]
        err = (got - want).abs()
        ratio = float((err / B.clamp_min(1e-300)).max())
        print(f"{name} {val}: max|got - ref| / B = {ratio:.3e}, max|ref| = {float(want.abs().max()):.3e}")
        assert float(want.abs().max()) > 0
        assert bool((got[B == 0] == 0).all())
        assert bool((err <= 4e-6 * B).all())


@pytest.mark.parametrize("name", ["lin_L16_T20", "smooth_L16_T12", F2_LOOP, GENERIC])
def test_ragged_prefixes_single_outputs_and_repeatability(name):
    x, g, v, tab, res, log2T, F, interp = _case(name)
    ops = _ops()
    gg, gx = _full(name)
    for M in (1, 63, 65, 1000):
        a, b = ops.hashgrid_bwd_input_bwd(x[:M], g[:M], v[:M], tab, res, log2T, F, interp)
        assert torch.equal(a, gg[:M]) and torch.equal(b, gx[:M]), M
    a, b = ops.hashgrid_bwd_input_bwd(x[:0], g[:0], v[:0], tab, res, log2T, F, interp)
    assert a.shape == (0, len(res) * F) and b.shape == (0, 3)
    a, b = ops.hashgrid_bwd_input_bwd(x, g, v, tab, res, log2T, F, interp)
    assert torch.equal(a, gg) and torch.equal(b, gx)
    a, none = ops.hashgrid_bwd_input_bwd(x, g, v, tab, res, log2T, F, interp, want_gx=False)
    assert none is None and torch.equal(a, gg)
    none, b = ops.hashgrid_bwd_input_bwd(x, g, v, tab, res, log2T, F, interp, want_gg=False)
    assert none is None and torch.equal(b, gx)


def test_nearest_gives_exact_zeros_and_leaves_the_table_gradient():
    x, g, v, tab, res, log2T, F, interp = _case("near_L16_T12")
    assert interp == 0
    ops = _ops()
    gg, gx = ops.hashgrid_bwd_input_bwd(x, g, v, tab, res, log2T, F, interp)
    assert gg.shape == g.shape and gx.shape == x.shape
    assert bool((gg == 0).all()) and bool((gx == 0).all())
    sentinel = torch.full_like(tab, 7.25)
    out = ops.hashgrid_bwd_input_bwd_table(x, g, v, res, log2T, F, interp, out=sentinel)
    assert out is sentinel and bool((sentinel == 7.25).all())


@pytest.mark.parametrize("name", CASES)
def test_scatter_kernel_vs_float64_formulas(name):
    """Scattered into a buffer that already holds values.  A row with n contributions starts at B_row / n (about one
    term's size, so an overwrite in place of the accumulation misses the bound by orders of magnitude); the n atomic
    roundings then act on partial sums of at most B_row + B_row / n, which adds one rounding unit of B_row to the
    bound's n - 1 -- inside its 16 per term, of which k_b * g uses about 10.  Untouched rows hold 1.0."""
    x, g, v, tab, res, log2T, F, interp = _case(name)
    ref = _ref(name)
    n = ref["n_row"]
    init = torch.where(n[:, None] > 0, ref["B_row"] / n.clamp_min(1)[:, None], torch.ones_like(ref["B_row"])).float()
    buf = init.clone()
    out = _ops().hashgrid_bwd_input_bwd_table(x, g, v, res, log2T, F, interp, out=buf)
    assert out is buf
    got = buf.double() - init.double()
    err = (got - ref["gT"]).abs()
    bound = (n[:, None] + 16).double() * 2.0 ** -24 * ref["B_row"]
    hit = n > 0
    ratio = float((err[hit] / bound[hit].clamp_min(1e-300)).max())
    print(f"{name}: max|got - ref| / bound = {ratio:.3e}, max n_row = {int(n.max())}, "
          f"max|ref| = {float(ref['gT'].abs().max()):.3e}")
    assert float(ref["gT"].abs().max()) > 0
    assert bool((got[~hit] == 0).all())
    assert bool((err <= bound).all())
    # without out=: a fresh zero-filled gradient
    fresh = _ops().hashgrid_bwd_input_bwd_table(x, g, v, res, log2T, F, interp)
    assert bool(((fresh.double() - ref["gT"]).abs() <= bound).all())


def test_autograd_wiring_inside_the_second_order_scope():
    from adaptive_city_nerf_amd._lib import AcnError
    from adaptive_city_nerf_amd.ray_rendering import second_order
    ops = _ops()
    enc = TI._encoder("Smoothstep")
    cfg = (enc._res_host, 12, 2, enc._interp_code)
    gen = torch.Generator().manual_seed(60)
    x0 = torch.rand(1000, 3, generator=gen).to(DEV)
    g0 = torch.randn(1000, 32, generator=gen).to(DEV)
    v = torch.randn(1000, 3, generator=gen).to(DEV)
    first = ops.hashgrid_bwd_input(x0, g0, enc.hash_table, *cfg)
    with second_order():
        x, g = x0.clone().requires_grad_(), g0.clone().requires_grad_()
        (gx,) = torch.autograd.grad(enc(x), x, g, create_graph=True)
        assert gx.grad_fn is not None and torch.equal(gx, first)
        ax, ag, at = torch.autograd.grad((gx * v).sum(), [x, g, enc.hash_table], retain_graph=True)
        gg, gx2 = ops.hashgrid_bwd_input_bwd(x0, g0, v, enc.hash_table, *cfg)
        assert torch.equal(ax, gx2) and torch.equal(ag, gg)
        # the table side is an atomic sum: two runs agree within twice its rounding bound
        ref = H.double_backward(x0, g0, v, enc.hash_table, *cfg[:2], cfg[3])
        want = ops.hashgrid_bwd_input_bwd_table(x0, g0, v, *cfg)
        bound = 2 * (ref["n_row"][:, None] + 16).double() * 2.0 ** -24 * ref["B_row"]
        assert float(want.abs().max()) > 0 and bool(((at - want).double().abs() <= bound).all())
        with pytest.raises(AcnError, match="third-order"):
            torch.autograd.grad((gx * v).sum(), x, create_graph=True)
        # a plain backward inside the scope is today's first-order gradient
        x = x0.clone().requires_grad_()
        enc(x).backward(g0)
        assert torch.equal(x.grad, first)
        # no deterministic variant of the table side: it refuses instead of being quietly non-deterministic
        x = x0.clone().requires_grad_()
        (gx,) = torch.autograd.grad(enc(x), x, g0, create_graph=True)
        prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            with pytest.raises(AcnError, match="deterministic"):
                torch.autograd.grad((gx * v).sum(), enc.hash_table)
            with pytest.raises(AcnError, match="deterministic"):
                ops.hashgrid_bwd_input_bwd_table(x0, g0, v, *cfg)
        finally:
            torch.use_deterministic_algorithms(prev)
    # outside the scope nothing changed: a recorded backward is refused
    x = x0.clone().requires_grad_()
    with pytest.raises(AcnError, match="second-order"):
        torch.autograd.grad(enc(x), x, g0, create_graph=True)


# ------------------------------------------------------------------------------------------------- end to end
NAMES = ["xyz_encoder.hash_table", "sigma_trunk.0.linear.weight", "sigma_trunk.0.linear.bias",
         "sigma_trunk.1.linear.weight", "sigma_trunk.1.linear.bias", "sigma_head.weight", "sigma_head.bias"]


def _loss(sigma, n, eikonal):
    base = sigma.mean()
    return base + 0.1 * ((n.norm(dim=-1) - 1) ** 2).mean() if eikonal else base


def _restated_grads(m, x, dtype):
    """The density branch of MetaNGP and the eikonal loss in torch ops on the CPU, in ``dtype``."""
    from adaptive_city_nerf_amd.trunc_exp import TruncExp
    enc = m.xyz_encoder
    p = {k: t.detach().cpu().to(dtype).requires_grad_() for k, t in m.named_parameters() if k in NAMES}
    xr = x.detach().cpu().to(dtype).requires_grad_()
    x01 = ((xr - m.scene_box.min.cpu().to(dtype)) / m.aabb_extent.cpu().to(dtype)).clamp(1e-6, 1.0 - 1e-6)
    h = R.hashgrid(x01, p[NAMES[0]], enc._res_host, enc.log2_hashmap_size, enc._interp_code, dtype=dtype,
                   weights="fp32")
    h = F_.relu(F_.linear(h, p[NAMES[1]], p[NAMES[2]]))
    h = F_.relu(F_.linear(h, p[NAMES[3]], p[NAMES[4]]))
    sigma = TruncExp.apply(F_.linear(h, p[NAMES[5]], p[NAMES[6]]))
    (n,) = torch.autograd.grad(sigma.sum(), xr, create_graph=True)
    grads = torch.autograd.grad(_loss(sigma, n, True), [p[k] for k in NAMES])
    return {**dict(zip(NAMES, grads)), "sigma": sigma.detach(), "n": n.detach()}


def test_eikonal_loss_trains_the_table_and_the_density_mlp():
    m = TI._expert()
    assert m.training and all(p.requires_grad for p in m.parameters())
    x = (torch.rand(512, 3, generator=torch.Generator().manual_seed(70)) * 1.8 - 0.9).to(DEV)
    params = dict(m.named_parameters())

    def run(eikonal):
        m.zero_grad(set_to_none=True)
        sigma, n = m.density_and_gradient(x, create_graph=True)
        assert sigma.shape == (512, 1) and n.shape == (512, 3) and n.grad_fn is not None
        _loss(sigma, n, eikonal).backward()
        return {**{k: params[k].grad.detach().clone() for k in NAMES}, "sigma": sigma.detach(), "n": n.detach()}

    got = run(True)
    base = run(False)
    s0, n0 = m.density_and_gradient(x)                       # first order: the same values, no graph
    assert s0.grad_fn is None and n0.grad_fn is None
    assert torch.equal(s0, got["sigma"]) and torch.equal(n0, got["n"])
    ref = _restated_grads(m, x, torch.float64)
    f32 = _restated_grads(m, x, torch.float32)
    for k in ["sigma", "n"] + NAMES:
        scale = max(1.0, float(ref[k].abs().max()))
        e32 = float((f32[k].double() - ref[k]).abs().max()) / scale
        tol = max(2e-5, 4 * e32)
        err = float((got[k].cpu().double() - ref[k]).abs().max()) / scale
        moved = float((got[k] - base[k]).abs().max()) / scale
        print(f"{k}: e32 = {e32:.3e}, GPU error = {err:.3e} (tolerance {tol:.3e}), eikonal term = {moved:.3e}, "
              f"max|ref| = {float(ref[k].abs().max()):.3e}")
        assert err <= tol
        # the eikonal term reaches the table: a gradient that autograd took for a constant would leave the
        # baseline's table gradient, which the comparison above then has to reject
        if k == NAMES[0]:
            assert moved > tol
