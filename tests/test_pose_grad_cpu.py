"""CPU-side checks of the pose-gradient feature: the ABI of the new entry points (acn_mlp_train_bwd_input[_img] in
its default and exact-fp32 builds, acn_rays_from_dirs_bwd).  Argument checks run before any HIP call: no GPU."""
import ctypes
import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

MLP = ["acn_mlp_train_bwd_input", "acn_mlp_train_bwd_input_img"]
RAYS = ["acn_rays_from_dirs_bwd", "acn_rays_from_dirs_bwd_workspace_bytes"]


def _last_error(L):
    buf = ctypes.create_string_buffer(256)
    L.acn_last_error(buf, 256)
    return buf.value


def test_abi_declares_exports_and_checks_arguments():
    text = (REPO / "include" / "acnerf.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(acn_\w+)\s*\(", text, re.M))
    names = set(RAYS) | {n + sfx for n in MLP for sfx in ("", "_exact", "_amp")}
    assert names <= declared
    from adaptive_city_nerf_amd import _lib
    L = _lib.lib()
    assert names <= set(_lib.exported_symbols())
    for n in names:
        assert hasattr(L, n), n

    w = _lib.acn_mlp()          # fourteen NULL tensors: never read by the checks
    one = ctypes.c_float(0.0)   # stands for any non-NULL pointer
    p = ctypes.addressof(one)
    for sfx in ("", "_exact"):
        f, fi = getattr(L, MLP[0] + sfx), getattr(L, MLP[1] + sfx)
        # negative M, NULL weights / workspace / image
        assert f(p, p, p, p, -1, ctypes.byref(w), p, p, p, None) == -1
        assert b"bad arguments" in _last_error(L)
        assert f(p, p, p, p, 4, None, p, p, p, None) == -1
        assert f(p, p, p, p, 4, ctypes.byref(w), p, p, None, None) == -1
        assert fi(p, p, p, p, -1, p, p, p, None) == -1
        assert fi(p, p, p, p, 4, None, p, p, None) == -1
        # NULL inputs with M > 0 and an output wanted
        assert f(None, p, p, p, 4, ctypes.byref(w), p, p, p, None) == -1
        assert b"NULL" in _last_error(L)
        assert f(p, p, p, None, 4, ctypes.byref(w), None, p, p, None) == -1
        assert fi(p, None, p, p, 4, p, p, None, None) == -1
        assert b"NULL" in _last_error(L)
        # no-ops: M == 0, or neither output wanted
        assert f(None, None, None, None, 0, ctypes.byref(w), None, None, p, None) == 0
        assert f(None, None, None, None, 4, ctypes.byref(w), None, None, p, None) == 0
        assert fi(None, None, None, None, 0, p, p, p, None) == 0
        assert fi(None, None, None, None, 4, p, None, None, None) == 0

    r = L.acn_rays_from_dirs_bwd
    c2w = (ctypes.c_float * 12)()
    ws = (ctypes.c_double * 12)()
    wp = ctypes.addressof(ws)
    assert L.acn_rays_from_dirs_bwd_workspace_bytes(0) >= 8
    assert L.acn_rays_from_dirs_bwd_workspace_bytes(1) == 12 * 8
    assert L.acn_rays_from_dirs_bwd_workspace_bytes(70001) % (12 * 8) == 0
    assert r(p, -1, c2w, p, p, p, wp, 96, None) == -1
    assert b"bad arguments" in _last_error(L)
    assert r(p, 4, None, p, p, p, wp, 96, None) == -1
    assert r(None, 4, c2w, p, p, p, wp, 96, None) == -1
    assert b"NULL" in _last_error(L)
    assert r(p, 4, c2w, None, p, p, wp, 96, None) == -1
    assert r(p, 4, c2w, p, None, p, wp, 96, None) == -1
    assert r(p, 4, c2w, p, p, None, None, 96, None) == -1
    assert r(p, 4, c2w, p, p, None, wp, 8, None) == -1           # workspace too small
    assert b"workspace" in _last_error(L)
    assert r(None, 0, c2w, None, None, None, None, 0, None) == 0   # N = 0, nothing to write: no device needed
