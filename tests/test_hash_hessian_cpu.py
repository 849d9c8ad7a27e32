"""CPU-side checks of the second-order point gradient of the hash grid: the explicit double-backward formulas the
GPU tests compare with (tests/hash_hessian_ref.py) against float64 autograd taken twice through the torch
restatement of the encoder (tests/input_grad_ref.py), and the ABI of the two new entry points."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import goldens as G
import hash_hessian_ref as H
import input_grad_ref as R
from oracle import oracle as O

REPO = Path(__file__).resolve().parent.parent
NEW = {"acn_hashgrid_bwd_input_bwd", "acn_hashgrid_bwd_input_bwd_table"}


@pytest.mark.parametrize("interp,L,F,log2T", [(1, 16, 2, 12), (2, 16, 2, 12), (1, 5, 4, 10)])
def test_formulas_equal_float64_autograd_taken_twice(interp, L, F, log2T):
    """<= 1e-12 * max|ref| (float64 on both sides: only the summation order differs), and |value| <= B."""
    M = 300
    res = O.level_resolutions(L, 16, 4096 if L == 16 else 256).tolist()
    from adaptive_city_nerf_amd.synthetic import formula_table
    tab = torch.from_numpy(formula_table(L, log2T, F, seed=7, scale=0.5)).double()
    gen = torch.Generator().manual_seed(8)
    # half golden points (edge and lattice points included), half uniform ones
    x = torch.cat([torch.from_numpy(G.load("hashgrid")["x01"][-150:]), torch.rand(150, 3, generator=gen)]).double()
    g = torch.randn(M, L * F, generator=gen, dtype=torch.float64)
    v = torch.randn(M, 3, generator=gen, dtype=torch.float64)
    xr, gr, tr = x.clone().requires_grad_(), g.clone().requires_grad_(), tab.clone().requires_grad_()
    out = R.hashgrid(xr, tr, res, log2T, interp, dtype=torch.float64, weights="fp32")
    (gx,) = torch.autograd.grad((out * gr).sum(), xr, create_graph=True)
    ref = dict(zip(("gg", "gx2", "gT"), torch.autograd.grad((gx * v).sum(), [gr, xr, tr])))
    got = H.double_backward(x, g, v, tab, res, log2T, interp)
    for name, scale in (("gg", "B_gg"), ("gx2", "B_x"), ("gT", "B_row")):
        top = float(ref[name].abs().max())
        err = float((got[name] - ref[name]).abs().max())
        print(f"interp={interp} L={L} F={F} {name}: max|formula - autograd| = {err:.3e}, max|ref| = {top:.3e}")
        assert top > 0 and err <= 1e-12 * top
        assert bool((got[name].abs() <= got[scale] * (1 + 1e-12)).all())
    assert int(got["n_row"].sum()) == M * L * 8
    assert bool((got["gT"][got["n_row"] == 0] == 0).all())


def test_nearest_reference_is_zero():
    res = O.level_resolutions(4, 16, 128).tolist()
    x, g, v = torch.rand(10, 3), torch.randn(10, 8), torch.randn(10, 3)
    got = H.double_backward(x, g, v, torch.randn(4 << 8, 2), res, 8, 0)
    assert all(bool((t == 0).all()) for t in got.values())


def test_abi_declares_exports_and_checks_arguments():
    text = (REPO / "include" / "acnerf.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(acn_\w+)\s*\(", text, re.M))
    assert NEW <= declared
    assert "#define ACN_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", text)
    from adaptive_city_nerf_amd import _lib
    assert NEW <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert NEW <= set(_lib.exported_symbols())
    res = (ctypes.c_int32 * 40)()
    buf = ctypes.create_string_buffer(256)
    # argument checks run before any HIP call: no GPU needed
    for call in (lambda L_, M: L.acn_hashgrid_bwd_input_bwd(None, M, None, None, None, res, L_, 20, 2, 1, None, None, None),
                 lambda L_, M: L.acn_hashgrid_bwd_input_bwd_table(None, M, None, None, res, L_, 20, 2, 1, None, None)):
        assert call(40, 10) == -1
        L.acn_last_error(buf, 256)
        assert b"levels" in buf.value
        assert call(0, 10) == -1
        assert call(16, 0) == 0                                            # M = 0: no-op
    assert L.acn_hashgrid_bwd_input_bwd(None, 10, None, None, None, res, 16, 20, 0, 1, None, None, None) == -1   # F = 0
    assert L.acn_hashgrid_bwd_input_bwd(None, 10, None, None, None, res, 16, 20, 2, 1, None, None, None) == 0    # no output
    assert L.acn_hashgrid_bwd_input_bwd_table(None, 10, None, None, res, 16, 20, 2, 1, None, None) == -1         # NULL, M > 0
    L.acn_last_error(buf, 256)
    assert b"NULL" in buf.value
    assert L.acn_hashgrid_bwd_input_bwd_table(None, 10, None, None, res, 16, 20, 2, 0, None, None) == 0          # Nearest
