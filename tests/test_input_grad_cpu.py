"""CPU-side checks of the input-gradient feature: the ABI of the two new entry points, and the reference the GPU
tests compare with (tests/input_grad_ref.py) against the golden forward and against finite differences."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import goldens as G
import input_grad_ref as R
from oracle import oracle as O

REPO = Path(__file__).resolve().parent.parent


def test_abi_declares_exports_and_checks_arguments():
    text = (REPO / "include" / "acnerf.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(acn_\w+)\s*\(", text, re.M))
    assert {"acn_hashgrid_bwd_input", "acn_sh_bwd"} <= declared
    from adaptive_city_nerf_amd import _lib
    L = _lib.lib()
    assert {"acn_hashgrid_bwd_input", "acn_sh_bwd"} <= set(_lib.exported_symbols())
    res = (ctypes.c_int32 * 40)()
    buf = ctypes.create_string_buffer(256)
    # argument checks run before any HIP call: no GPU needed
    assert L.acn_hashgrid_bwd_input(None, 10, None, None, res, 40, 20, 2, 1, None, None) == -1
    L.acn_last_error(buf, 256)
    assert b"levels" in buf.value
    assert L.acn_hashgrid_bwd_input(None, 10, None, None, res, 16, 20, 0, 1, None, None) == -1
    assert L.acn_hashgrid_bwd_input(None, 10, None, None, res, 16, 20, 2, 1, None, None) == -1   # NULL with M > 0
    L.acn_last_error(buf, 256)
    assert b"NULL" in buf.value
    assert L.acn_hashgrid_bwd_input(None, 0, None, None, res, 16, 20, 2, 1, None, None) == 0     # M = 0: no-op
    assert L.acn_sh_bwd(None, 4, 7, None, None, None) == -1
    L.acn_last_error(buf, 256)
    assert b"levels" in buf.value
    assert L.acn_sh_bwd(None, 4, 4, None, None, None) == -1
    assert L.acn_sh_bwd(None, 0, 4, None, None, None) == 0


@pytest.mark.parametrize("name", ["near_L16_T12", "smooth_L16_T12", "lin_L8_T14_r2_512", "lin_L4_T19"])
def test_restatement_forward_is_the_golden_forward(name):
    """float32, weights="fp32": bit for bit the reference's forward, edge and lattice points included."""
    d = G.load("hashgrid")
    L, mn, mx, log2T, seed, interp = [int(v) for v in d[f"{name}:cfg"]]
    from adaptive_city_nerf_amd.synthetic import formula_table
    tab = torch.from_numpy(formula_table(L, log2T, 2, seed=seed, scale=0.5))
    y = R.hashgrid(torch.from_numpy(d["x01"]), tab, d[f"{name}:resolutions"].tolist(), log2T, interp,
                   dtype=torch.float32, weights="fp32")
    assert np.array_equal(y.numpy(), d[f"{name}:y"])


def _interior_points(res, n, seed):
    """n points of [0,1]^3 whose weights lie in [0.05, 0.95] on every level and axis."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(400_000, 3, generator=gen, dtype=torch.float64)
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for r in res:
        w = x * float(r)
        w = w - torch.floor(w)
        ok &= ((w >= 0.05) & (w <= 0.95)).all(-1)
    x = x[ok]
    assert x.shape[0] >= n
    return x[:n].contiguous()


@pytest.mark.parametrize("interp,bound", [(1, 1e-8), (2, 1e-3)])
def test_restatement_autograd_matches_central_differences(interp, bound):
    """weights="exact", float64, h = 1e-6.  Linear is affine per axis inside a cell (only rounding remains: 1e-8);
    Smoothstep leaves the h^2 term of a quintic (1e-3)."""
    L, log2T, h = 16, 12, 1e-6
    res = O.level_resolutions(L, 16, 4096).tolist()
    from adaptive_city_nerf_amd.synthetic import formula_table
    tab = torch.from_numpy(formula_table(L, log2T, 2, seed=3, scale=0.5)).double()
    x = _interior_points(res, 256, seed=1)
    g = torch.randn(256, L * 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ref, _ = R.hashgrid_grad(x, g, tab, res, log2T, interp, dtype=torch.float64, weights="exact")

    def loss(xx):
        return (R.hashgrid(xx, tab, res, log2T, interp, dtype=torch.float64, weights="exact") * g).sum(-1)

    fd = torch.empty_like(x)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        fd[:, a] = (loss(x + e) - loss(x - e)) / (2 * h)
    err = float((fd - ref).abs().max() / ref.abs().max())
    print(f"interp={interp}: max|fd - autograd| / max|autograd| = {err:.3e}")
    assert err <= bound
