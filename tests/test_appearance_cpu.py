"""Per-image exposure correction without a GPU: the definition of tests/appearance_ref.py against
float64 autograd of the same formula, the torch fallback of train.appearance_mse_loss, AppearanceAffine's slots and state
dict, compute_loss with ``appearance=None`` call for call, the argument checks, and the conditions the GPU tests'
inputs have to meet."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import appearance_ref as R


def _torch64(*xs):
    return [torch.from_numpy(np.array(x)).double() for x in xs]


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_reference_gradients_equal_float64_autograd(layout):
    """The analytic g_pred, g_A, g_b of the definition against autograd of mean((clamp01(A[s] p + b[s]) - gt_lin)^2)
    in float64 torch ops.  The definition rounds c, d and g_c to fp32 (relative 2^-24, 2^-25 of at most 1, and 2^-24),
    so g_c differs from the float64 value by at most (2 / n) 2^-22, which carries to the outputs through their sums:
    times sum_k |A[s,k,j]| for g_pred, sum_r |p[r,j]| for g_A, the slot's ray count for g_b."""
    (pred, gt, slot, A, b), ref = R.case(1000, 70, layout, "generic")
    p, Am, bv = (t.requires_grad_(True) for t in _torch64(pred, A, b))
    gl, = _torch64(R.gt_linear(gt))
    loss = R.loss_chain_f64(p, gl, torch.from_numpy(np.array(slot)), Am, bv)
    g_p, g_A, g_b = torch.autograd.grad(loss, (p, Am, bv))
    n, has = 3 * slot.shape[0], ref["has"]
    e = (2.0 / n) * 2.0 ** -22
    assert abs(float(loss.detach()) - ref["loss"]) <= 2.0 ** -22 * ref["loss"]
    absA = np.where(has[:, None], np.abs(A[np.where(has, slot, 0)].astype(np.float64)).sum(1), 1.0)
    assert (np.abs(g_p.numpy() - ref["g_pred"]) <= e * absA + 1e-30).all()
    sum_p, cnt = np.zeros((70, 3)), np.zeros(70)
    np.add.at(sum_p, slot[has], np.abs(pred[has].astype(np.float64)))
    np.add.at(cnt, slot[has], 1.0)
    assert (np.abs(g_A.numpy() - ref["g_A"]) <= e * sum_p[:, None, :] + 1e-30).all()
    assert (np.abs(g_b.numpy() - ref["g_b"]) <= e * cnt[:, None] + 1e-30).all()
    if layout != "none":
        assert float(np.abs(ref["g_A"]).max()) > 0 and float(np.abs(ref["g_b"]).max()) > 0
    assert (ref["g_A"][cnt == 0] == 0).all() and (ref["g_b"][cnt == 0] == 0).all() and (cnt == 0).any()


def _module_from(A, b, ids=None):
    from adaptive_city_nerf_amd import AppearanceAffine
    app = AppearanceAffine(A.shape[0] if ids is None else ids)
    with torch.no_grad():
        app.matrix.copy_(torch.from_numpy(np.array(A)))
        app.offset.copy_(torch.from_numpy(np.array(b)))
    return app


def test_torch_fallback_on_cpu_tensors_matches_the_reference():
    """train.appearance_mse_loss on CPU tensors is the composed fp32 torch chain: its c carries a few fp32 roundings
    (the reference's one), so d moves by a few 2^-24 and every gradient by that times 2 / n times its sum."""
    from adaptive_city_nerf_amd.train import appearance_mse_loss
    (pred, gt, slot, A, b), ref = R.case(1000, 70, "mixed", "generic")
    ids = list(range(5, 5 + 2 * 70, 2))                       # non-contiguous image indices
    app = _module_from(A, b, ids)
    img = torch.from_numpy(np.where(ref["has"], 5 + 2 * np.where(ref["has"], slot, 0),
                                    np.where(slot < 0, 4, 5 + 2 * 70 + 7)))   # 4: inside the table, no slot
    p = torch.from_numpy(np.array(pred)).requires_grad_(True)
    loss = appearance_mse_loss(p, torch.from_numpy(np.array(gt)), img, app, "linear")
    assert abs(float(loss.detach()) - ref["loss"]) <= 2e-6 * ref["loss"]
    g_p, g_A, g_b = torch.autograd.grad(loss, (p, app.matrix, app.offset), create_graph=True)
    assert g_p.requires_grad                                   # differentiable again
    n = 3 * slot.shape[0]
    cnt = np.bincount(slot[ref["has"]], minlength=70)
    e = (2.0 / n) * 8 * 2.0 ** -24
    assert (np.abs(g_p.detach().numpy() - ref["g_pred"]) <= 2 * e + 1e-6 * np.abs(ref["g_pred"])).all()
    assert (np.abs(g_A.detach().numpy() - ref["g_A"]) <= 1.2 * e * cnt[:, None, None] + 1e-6 * np.abs(ref["g_A"])).all()
    assert (np.abs(g_b.detach().numpy() - ref["g_b"]) <= e * cnt[:, None] + 1e-6 * np.abs(ref["g_b"])).all()
    # srgb targets go through the generic chain too
    l_srgb = appearance_mse_loss(p, torch.from_numpy(np.array(gt)), img, app, "srgb")
    assert l_srgb.requires_grad and float(l_srgb.detach()) > 0
    # forward() on CPU tensors is the reference's c
    with torch.no_grad():
        c = app(p, img)
    assert float(np.abs(c.numpy() - ref["c"]).max()) <= 4 * 2.0 ** -24 * 2.0
    assert torch.equal(c[~torch.from_numpy(ref["has"])], p.detach()[~torch.from_numpy(ref["has"])])


def test_slots_state_dict_and_regulariser():
    from adaptive_city_nerf_amd import AppearanceAffine
    app = AppearanceAffine([3, 7, 20])
    assert app.num_images == 3 and tuple(app.matrix.shape) == (3, 3, 3) and tuple(app.offset.shape) == (3, 3)
    assert torch.equal(app.matrix, torch.eye(3).expand(3, 3, 3)) and float(app.offset.abs().max()) == 0.0
    s = app.slots(torch.tensor([3, 7, 20, 0, 19, 21, -1, 10 ** 6, -(10 ** 6)]))
    assert s.dtype == torch.int32 and s.tolist() == [0, 1, 2, -1, -1, -1, -1, -1, -1]
    assert app.slots(7).tolist() == [1] and app.slots([20, 4]).tolist() == [2, -1]
    assert AppearanceAffine(4).slots(torch.arange(-1, 6, dtype=torch.int32)).tolist() == [-1, 0, 1, 2, 3, -1, -1]
    assert float(app.regulariser()) == 0.0
    with torch.no_grad():
        app.matrix[1, 0, 2] = 0.5
        app.offset[2, 1] = -0.25
    assert float(app.regulariser()) == pytest.approx(0.25 / 27 + 0.0625 / 9, rel=1e-6)
    sd = app.state_dict()
    assert set(sd) == {"matrix", "offset", "lookup"}
    other = AppearanceAffine([3, 7, 20])
    other.load_state_dict(sd)
    assert all(torch.equal(sd[k], v) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError):
        AppearanceAffine([3, 7, 21]).load_state_dict(sd)      # another lookup table: a size mismatch, not silence
    x = torch.rand(4, 5, 3)
    assert torch.equal(AppearanceAffine(2)(x, 0), x) and torch.equal(app(x, 99), x)
    for bad in ([], [1, 1], [-2, 3], 0):
        with pytest.raises(ValueError):
            AppearanceAffine(bad)
    with pytest.raises(ValueError, match="image indices"):
        app(x, [3, 7])


class _P:
    ray_samples, chunk_points, color_space = 8, 1 << 20, "linear"


class _Data(dict):
    """A batch that records which keys are read."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.read = []

    def __getitem__(self, k):
        self.read.append(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        self.read.append(k)
        return super().get(k, default)


def test_compute_loss_without_an_appearance_model_is_call_for_call_the_same(monkeypatch):
    from adaptive_city_nerf_amd import AppearanceAffine, train
    for fn in (train.compute_loss, train.adapt_step, train.GraphedAdaptStep.__init__, train.runtime_adapt):
        p = inspect.signature(fn).parameters
        assert p["appearance"].default is None and p["appearance_reg"].default == 0.0
    assert inspect.signature(train.adapt_step).parameters["img_indices"].default is None
    assert inspect.signature(train.GraphedAdaptStep.__call__).parameters["img_indices"].default is None
    calls = []
    gen = torch.Generator().manual_seed(2)
    rgb = torch.rand(6, 3, generator=gen) * 1.4 - 0.2

    def render_rays(model, rays, **kw):
        calls.append(("render_rays", dict(kw)))
        return rgb, None, None, None

    real_mse = train.mse_color_loss

    def mse_color_loss(*a, **k):
        calls.append(("mse_color_loss", len(a), dict(k)))
        return real_mse(*a, **k)

    def appearance_mse_loss(*a, **k):
        calls.append(("appearance_mse_loss",))
        return real_app(*a, **k)

    real_app = train.appearance_mse_loss
    monkeypatch.setattr(train, "render_rays", render_rays)
    monkeypatch.setattr(train, "mse_color_loss", mse_color_loss)
    monkeypatch.setattr(train, "appearance_mse_loss", appearance_mse_loss)
    img = torch.tensor([0, 1, 1, 5, 0, 2])
    base = {"rays": torch.zeros(6, 8), "rgbs": torch.rand(6, 3, generator=gen), "img_indices": img}
    mse = train.compute_mse_loss(_P, None, dict(base))
    first, calls[:] = list(calls), []
    data = _Data(base)
    same = train.compute_loss(_P, None, data, appearance=None, appearance_reg=0.5)
    assert torch.equal(mse, same) and calls == first and "img_indices" not in data.read
    assert [c[0] for c in calls] == ["render_rays", "mse_color_loss"] and "appearance" not in calls[0][1]
    # with a model: one render with the same arguments, then appearance_mse_loss on the batch's image indices
    app = AppearanceAffine(3)
    with torch.no_grad():
        app.matrix.mul_(0.5)
        app.offset.add_(0.125)
    calls[:] = []
    data = _Data(base)
    loss = train.compute_loss(_P, None, data, appearance=app, appearance_reg=0.5)
    assert [c[0] for c in calls][:2] == ["render_rays", "appearance_mse_loss"] and calls[0] == first[0]
    assert "img_indices" in data.read
    want = real_mse(torch.where((img < 3)[:, None], 0.5 * rgb + 0.125, rgb), base["rgbs"], "linear")
    assert torch.allclose(loss, want + 0.5 * app.regulariser(), rtol=1e-6, atol=0)
    assert float(app.regulariser()) > 0
    with pytest.raises(ValueError, match="img_indices"):
        train.compute_loss(_P, None, {"rays": base["rays"], "rgbs": base["rgbs"]}, appearance=app)
    with pytest.raises(ValueError, match="img_indices"):
        train.adapt_step(_P, None, base["rays"], base["rgbs"], None, appearance=app)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])
    with pytest.raises(ValueError, match="appearance model's parameters"):
        train.adapt_step(_P, None, base["rays"], base["rgbs"], opt, appearance=app, img_indices=img)
    with pytest.raises(ValueError, match="expert-parallel"):
        train.adapt_step(None, None, None, None, None, group=object(), appearance=app)
    with pytest.raises(ValueError, match="img_indices"):
        train.runtime_adapt(P=_P, model=torch.nn.Linear(1, 1), data_loader=[(base["rays"], base["rgbs"])],
                            optimizer=None, appearance=app)


def test_bad_arguments_are_refused_before_any_hip_call():
    from adaptive_city_nerf_amd import _lib as L
    from adaptive_city_nerf_amd import ops
    p, s, A, b = torch.rand(4, 3), torch.zeros(4, dtype=torch.int32), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    with pytest.raises(L.AcnError, match="HIP device"):
        ops.appearance_mse(p, p, s, A, b)
    with pytest.raises(L.AcnError, match="HIP device"):
        ops.appearance_apply(p, s, A, b)
    lib, n = L.lib(), None

    def err():
        buf = C.create_string_buffer(512)
        lib.acn_last_error(buf, 512)
        return buf.value.decode()

    one = C.c_void_p(8)   # a non-NULL pointer that is never followed: the checks come before any HIP call
    assert lib.acn_appearance_mse_workspace_bytes(1) == lib.acn_appearance_mse_workspace_bytes(4096) > 0
    assert lib.acn_appearance_mse(n, n, n, 0, n, n, 1, n, n, n, n, n, 0, n) == -1 and ">= 1" in err()
    assert lib.acn_appearance_mse(n, n, n, 4, n, n, 0, n, n, n, n, n, 0, n) == -1 and ">= 1" in err()
    assert lib.acn_appearance_mse(n, n, n, 4, n, n, 2, n, n, n, n, n, 0, n) == -1 and "NULL" in err()
    assert lib.acn_appearance_mse(one, one, one, 4, one, one, 2, one, one, n, n, one, 1 << 20, n) == -1
    assert "together" in err()
    assert lib.acn_appearance_mse(one, one, one, 4, one, one, 2, one, n, n, n, one, 8, n) == -1 and "workspace" in err()
    assert lib.acn_appearance_apply(n, n, -1, n, n, 1, n, n) == -1
    assert lib.acn_appearance_apply(n, n, 4, n, n, 1, n, n) == -1 and "NULL" in err()
    assert lib.acn_appearance_apply(n, n, 0, n, n, 1, n, n) == 0          # nothing launched


@pytest.mark.parametrize("I", R.I_CASES)
@pytest.mark.parametrize("N", R.N_CASES)
def test_the_gpu_cases_meet_their_input_conditions(N, I):
    """What tests/test_appearance_gpu.py's comparison with the definition relies on, asserted on the reference alone,
    for every layout of every case:
    - no c within relative 2^-40 of an fp32 rounding boundary: a round-once float64 evaluation and the reference's
      cast cannot disagree;
    - at least 10 % of the elements in the clamp's dead zone and at least 50 % live;
    - a slot with zero rays and rays with slot -1 in the case (one ray cannot be in a slot and outside, and one slot
      cannot be hit and empty, so this is asked of the case's layouts together, and of the mixed layout alone from
      63 rays and 3 slots on);
    - targets on gt_linear's linear branch or at / above 1."""
    empty = minus = False
    for layout in R.LAYOUTS:
        (pred, gt, slot, A, b), ref = R.case(N, I, layout)
        assert float(R.boundary_margin(pred, slot, A, b).min()) > 2.0 ** -40
        live = float(ref["live"].mean())
        assert live >= 0.5 and 1.0 - live >= 0.1, (layout, live)
        assert bool(((gt <= np.float32(0.04045)) | (gt >= 1)).all())
        cnt = np.bincount(slot[ref["has"]], minlength=I)
        e, m = bool((cnt == 0).any()), bool((slot == -1).any())
        empty, minus = empty or e, minus or m
        if layout == "mixed" and N >= 63 and I >= 3:
            assert e and m and bool((slot >= I).any()) and int((cnt > 0).sum()) >= 2
        if layout == "one":
            assert int(cnt[I - 1]) == N
    assert empty and minus


def test_dyadic_inputs_are_exact():
    """Every product and partial sum of g_A and g_b on the dyadic inputs fits a float64: a sum in another order gives
    the same bits."""
    for N, I in ((1024, 3), (4096, 70)):
        pred, gt, slot, A, b = R.dyadic_inputs(N, I)
        ref = R.reference(pred, gt, slot, A, b)
        perm = np.random.default_rng(1).permutation(N)
        ref_p = R.reference(pred[perm], gt[perm], slot[perm], A, b)
        assert np.array_equal(ref["g_A"], ref_p["g_A"]) and np.array_equal(ref["g_b"], ref_p["g_b"])
        assert np.array_equal(ref["g_pred"][perm], ref_p["g_pred"])
        assert float(np.abs(ref["g_A"]).max()) > 0 and bool((ref["c"] == 0).any() or (ref["c"] == 1).any())
        cnt = np.bincount(slot[ref["has"]], minlength=I)
        assert (cnt == 0).any() or I == 1
        # backwards too: exactness, not luck of one order
        rev = R.reference(pred[::-1], gt[::-1], slot[::-1], A, b)
        assert np.array_equal(ref["g_A"], rev["g_A"]) and np.array_equal(ref["g_b"], rev["g_b"])
