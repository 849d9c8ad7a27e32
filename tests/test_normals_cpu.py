"""Host-side checks of the fused density gradient and the normal maps, no GPU needed: the float64
restatement the GPU tests compare with (tests/normal_ref.py) agrees with central finite differences,
acn_field_sigma_grad refuses the configurations its kernel does not implement before any HIP call, and the torch
restatement of acn_normal_composite is consistent with itself."""
import ctypes as C

import pytest
import torch

import normal_ref as N

HASH_CONF = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": 12, "max_res": 4096, "min_res": 16,
             "interpolation": "Linear"}


def _expert(interp):
    from adaptive_city_nerf_amd import SceneBox
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    torch.manual_seed(11)
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=dict(HASH_CONF, interpolation=interp), dir_encoding="spherical")
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    return m


def _ref_args(m):
    enc = m.xyz_encoder
    mn, ext = m._host_box()
    return (m._mlp_tensors(None), enc.hash_table, enc._res_host, enc.log2_hashmap_size, enc._interp_code, mn, ext)


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_float64_restatement_agrees_with_central_differences(interp):
    m = _expert(interp)
    x = torch.rand(64, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2.2 - 1.1
    sig, grad, pre = N.sigma_grad(x, *_ref_args(m), dtype=torch.float64, weights="exact")
    assert sig.shape == (64,) and grad.shape == (64, 3) and pre.shape == (64, 128)
    h = 1e-7
    fd = torch.zeros_like(grad)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        sp, _, _ = N.sigma_grad(x + e, *_ref_args(m), dtype=torch.float64, weights="exact")
        sm, _, _ = N.sigma_grad(x - e, *_ref_args(m), dtype=torch.float64, weights="exact")
        fd[:, a] = (sp - sm) / (2 * h)
    # away from the cell faces, the ReLU kinks and the box faces (a step of 1e-7 crosses one with probability ~1e-2
    # per point) the function is a polynomial per piece: the difference quotient is exact to rounding, ~1e-16 / h
    err = (fd - grad).abs().amax(-1)
    scale = max(1.0, float(grad.abs().max()))
    print(f"{interp}: max|fd - grad| = {float(err.max()):.3e}, median = {float(err.median()):.3e}, "
          f"max|grad| = {float(grad.abs().max()):.3e}")
    assert float(grad.abs().max()) > 0
    assert int((err > 1e-6 * scale).sum()) <= 1           # at most one of the 64 points straddles a kink
    # a coordinate outside the box is clamped: no derivative along it
    out = (x < -1.0) | (x > 1.0)
    assert bool(out.any()) and bool((grad[out] == 0).all())
    # the fp32-cell form the kernel is compared with has the same values up to the float32 rounding of x01
    sig32, grad32, _ = N.sigma_grad(x.float(), *_ref_args(m), dtype=torch.float64, weights="fp32")
    assert float(((sig32 - sig).abs() / sig.abs().clamp_min(1.0)).max()) <= 1e-4


def _last_error(L):
    buf = C.create_string_buffer(512)
    L.lib().acn_last_error(buf, 512)
    return buf.value.decode()


@pytest.mark.parametrize("entry", ["acn_field_sigma_grad", "acn_field_sigma_grad_exact"])
def test_unsupported_configurations_are_refused_before_any_launch(entry):
    """Host memory stands in for every pointer: a refusal that came after a launch would fault or report a HIP
    error instead of ACN_ERR_UNSUPPORTED."""
    import torch  # noqa: F401
    from adaptive_city_nerf_amd import _lib as L
    fn = getattr(L.lib(), entry)
    dummy = C.create_string_buffer(1 << 20)
    p = C.addressof(dummy)
    w = L.acn_mlp()
    for f, _ in L.acn_mlp._fields_:
        setattr(w, f, p)
    res = (C.c_int32 * 32)(*[16 << (i // 2) for i in range(32)])
    box = (C.c_float * 3)(1.0, 1.0, 1.0)

    def call(L_=16, log2T=12, F=2, interp=1, M=4, ld=3):
        return fn(p, M, ld, p, res, L_, log2T, F, interp, C.cast(box, C.c_void_p), C.cast(box, C.c_void_p), 1e-6,
                  1.0 - 1e-6, C.byref(w), None, 0.0, p, p, p, None)

    for kw, word in ((dict(interp=0), "Nearest"), (dict(F=4), "16*2"), (dict(L_=8), "16*2"),
                     (dict(log2T=25), "2 GiB")):
        assert call(**kw) == -2, kw
        assert word in _last_error(L), (kw, _last_error(L))
    assert call(ld=2) == -1 and "ld" in _last_error(L)
    assert call(M=0) == 0                                    # a no-op, nothing launched
    assert not hasattr(L.lib(), "acn_field_sigma_grad_amp")  # evaluation only: compiled out of the AMP object


def test_normal_composite_restatement_is_self_consistent():
    gen = torch.Generator().manual_seed(8)
    w = torch.rand(48, 40, generator=gen)
    g = torch.randn(48 * 40, 3, generator=gen) * torch.logspace(-6, 3, 48 * 40).unsqueeze(-1)
    zero = torch.rand(48 * 40, generator=gen) < 0.2
    g[zero] = 0.0
    n64 = N.normal_composite(g, w, torch.float64)
    n32 = N.normal_composite(g, w, torch.float32)
    assert n64.shape == (48, 3) and n64.dtype == torch.float64
    bound = 1e-6 * w.double().sum(1, keepdim=True) + 1e-12   # <= 8 fp32 roundings per term, a float64 sum
    assert bool(((n32 - n64).abs() <= bound).all())
    # a zero gradient adds exactly nothing, whatever its weight
    w0 = w.clone()
    w0.view(-1)[zero] = 0.0
    assert torch.equal(N.normal_composite(g, w0, torch.float64), n64)
    # unit gradients: the result is minus the weighted mean direction, of norm at most sum w
    assert bool((n64.norm(dim=-1) <= w.double().sum(1) * (1 + 1e-12)).all())
    # the package's own torch form (CPU models) is the float32 restatement
    from adaptive_city_nerf_amd.ray_rendering import _normal_composite_torch
    assert bool(((_normal_composite_torch(g, w).double() - n64).abs() <= bound).all())
