"""The table-gradient scatter's reference (hash_scatter_ref) checked without a GPU: against the golden gtable
fixtures, against the fp32 serial scatter (within the derived bound on generic inputs, bit for bit in any point
order on the exact dyadic inputs), and against mutations of that scatter, every one of which must break the dyadic
equality -- and, applied to the largest contribution of a row, the generic bound too.  That is the evidence that
the GPU tests (test_hash_scatter_gpu), which compare the kernels in the same two ways, fail on a subtly wrong one.
"""
import numpy as np
import pytest

import goldens as G
import hash_scatter_ref as R
from test_hash_det import serial_scatter


def _ref(c, **kw):
    return R.scatter_ref(c.x01, c.gout, c.res, c.log2T, c.F, c.interp, **kw)[0]


def _serial(c, order=None):
    keys, vals, _, _ = R.contributions_f32(c.x01, c.gout, c.res, c.log2T, c.F, c.interp)
    return R.serial_sum(keys, vals, len(c.res) << c.log2T, order)


def _assert_all_exact(c, ref):
    ok = R.exact_rows(ref.A, R.row_granule(c.res, c.B, c.interp, c.log2T))
    assert ok.all(), f"{(~ok).sum()} of {ok.size} rows not provably exact (max A {ref.A.max()})"


def _assert_within(got, ref):
    tol = R.tol_row(ref)
    err = np.abs(got.astype(np.float64) - ref.grad)
    assert np.all(err <= tol), f"worst error / bound {np.max(err[tol > 0] / tol[tol > 0]):.3g}"
    assert np.all(got[ref.A == 0] == 0)
    return float(np.max(err[tol > 0] / tol[tol > 0])) if np.any(tol > 0) else 0.0


# ------------------------------------------------------------------------------------------------------ golden parity
@pytest.mark.parametrize("name", ["near_L16_T12", "smooth_L16_T12", "lin_L8_T14_r2_512"])
def test_reference_reproduces_golden_gtable(name):
    """The golden convention of test_serial_restatement_matches_reference (the fixture is an fp32 scatter), and the
    derived row bound on top of it: the fixture is a float32 scatter of the same contributions in some order."""
    d = G.load("hashgrid")
    L, mn, mx, log2T, seed, interp = [int(v) for v in d[f"{name}:cfg"]]
    ref = R.scatter_ref(d["x01"], d[f"{name}:gy"], d[f"{name}:resolutions"], log2T, 2, interp)[0]
    gold = d[f"{name}:gtable"]
    np.testing.assert_allclose(ref.grad, gold, rtol=0, atol=2e-5 * max(1.0, float(np.abs(gold).max())))
    _assert_within(gold, ref)


@pytest.mark.parametrize("interp", [0, 1, 2])
def test_fp32_restatement_is_serial_scatter(interp):
    """contributions_f32 + serial_sum (what the mutations below are applied to) is test_hash_det.serial_scatter."""
    c = R.generic_case(interp, 700, L=5, log2T=9)
    np.testing.assert_array_equal(_serial(c), serial_scatter(c.x01, c.gout, c.res, 5, 9, interp))


# ------------------------------------------------------------------------------------------------------ generic bound
@pytest.mark.parametrize("kind", ["uniform", "rays", "same"])
@pytest.mark.parametrize("interp", [0, 1, 2])
def test_serial_scatter_within_row_bound(interp, kind):
    c = R.generic_case(interp, 6000, L=8, log2T=12 if kind != "uniform" else 10, kind=kind)
    ref = _ref(c)
    used = _assert_within(serial_scatter(c.x01, c.gout, c.res, 8, c.log2T, interp), ref)
    assert used < 0.5      # the bound is a bound: a serial sum stays well inside it
    rng = np.random.default_rng(3)
    _assert_within(_serial(c, rng.permutation(6000)), ref)


# ---------------------------------------------------------------------------------------------------- dyadic exactness
DYADIC = [(1, 8200, 14, False), (2, 8200, 14, False), (0, 8200, 14, False), (1, 8200, 14, True),
          (2, 8200, 14, True), (1, 4097, 1, False), (2, 4097, 2, False), (1, 300, 3, True), (2, 4097, 4, True)]


@pytest.mark.parametrize("interp,M,log2T,repeat", DYADIC)
def test_dyadic_scatter_exact_in_any_order(interp, M, log2T, repeat):
    c = R.dyadic_case(interp, M, L=8, log2T=log2T, repeat=repeat)
    ref = _ref(c)
    _assert_all_exact(c, ref)
    assert np.array_equal(ref.grad, ref.grad.astype(np.float32).astype(np.float64))
    rng = np.random.default_rng(5)
    for order in (None, np.arange(M)[::-1], rng.permutation(M)):
        np.testing.assert_array_equal(_serial(c, order).astype(np.float64), ref.grad)
    if interp:
        np.testing.assert_array_equal(serial_scatter(c.x01, c.gout, c.res, 8, log2T, interp).astype(np.float64),
                                      ref.grad)


def test_dyadic_inputs_hold_the_edges():
    """(0,0,0), (1,1,1), cell boundaries (zero-weight corners), Nearest's .5 ties and long runs are all there."""
    c = R.dyadic_case(1, 8200)
    x = c.x01
    assert (x == 0).all(1).any() and (x == 1).all(1).any()
    rows, w = R.cells(x, c.res, c.log2T, 1)
    assert (w == 0).all(-1).any() and (w > 0).any()
    s = x[:, None, :] * np.asarray(c.res, np.float32)[None, :, None]
    assert np.any(s - np.floor(s) == 0.5)
    cr = R.dyadic_case(1, 8200, repeat=True)
    same = np.all(cr.x01[1:] == cr.x01[:-1], axis=1)
    run = np.diff(np.flatnonzero(np.concatenate([[True], ~same, [True]])))
    assert run.max() >= 33 and np.any((run > 1) & (run < 16))   # within a lane stretch, and across several
    assert _ref(cr).n.max() >= 64


def test_padding_tail_and_experts_in_the_reference():
    """pidx < 0 and slots past ``live`` add nothing (NaN payloads never reach a sum); experts split by pk."""
    rng = np.random.default_rng(11)
    counts = (17, 0, 15)
    c = R.dyadic_case(1, sum(counts), L=7, log2T=6)
    p = R.pair_list(counts, c.x01, c.gout, rng)
    assert (p.pidx[:p.live] < 0).any() and np.isnan(p.x01[p.live:]).all() and p.x01.shape[0] > p.live
    refs = R.scatter_ref(p.x01, p.gout, c.res, 6, 2, 1, pk=p.pk, pidx=p.pidx, live=p.live, K=3)
    assert all(np.isfinite(r.grad).all() for r in refs) and refs[1].n.sum() == 0 and not refs[1].touched.any()
    for k in (0, 2):
        sel = (p.pk[:p.live] == k) & (p.pidx[:p.live] >= 0)
        one = R.scatter_ref(p.x01[:p.live][sel], p.gout[:p.live][sel], c.res, 6, 2, 1)[0]
        for a, b in zip(refs[k], one):
            np.testing.assert_array_equal(a, b)
    b = int(p.seg[1])
    assert (p.x01[b - 2:b + 2] == p.x01[b]).all() and (p.pidx[b - 2:b + 2] >= 0).all()


# ------------------------------------------------------------------------------------------------------------ mutations
def _largest(keys, vals, nrows, valid):
    """(m, l, c) of a contribution that is the largest of its row, in the row with the most contributions among
    those whose largest one is not a zero-weight corner.  ``valid`` (M, L): the points and levels to choose from."""
    mag = np.abs(vals).max(-1) * valid[..., None]
    flat = keys.reshape(-1)
    top = np.zeros(nrows)
    np.maximum.at(top, flat, mag.reshape(-1))
    cnt = np.bincount(flat, minlength=nrows) * (top > 0)
    row = int(np.argmax(cnt))
    return np.unravel_index(int(np.argmax(np.where(keys == row, mag, -1.0))), keys.shape)


def _mutants(c):
    """name -> (keys, vals) of the fp32 scatter with one contribution (or the weights of one point at one level)
    wrong, at the largest contribution of a crowded row."""
    keys, vals, w, a = R.contributions_f32(c.x01, c.gout, c.res, c.log2T, c.F, c.interp)
    # a point whose w is .5 on every axis has w = 1 - w: nothing to get wrong there
    m, l, cn = _largest(keys, vals, len(c.res) << c.log2T, (w != 0.5).any(-1))
    ax = int(np.argmax(w[m, l] != 0.5))          # 0: x (corner bit 4), 1: y (2), 2: z (1)
    g = np.asarray(c.gout, np.float32).reshape(vals.shape[0], len(c.res), c.F)[m, l]
    out = {}
    v = vals.copy()
    v[m, l, cn] = 0
    out["drop one contribution"] = v
    v = vals.copy()
    other = cn ^ (4 >> ax)
    v[m, l, [cn, other]] = v[m, l, [other, cn]]
    out["swap two corner weights"] = v
    v = vals.copy()
    flipped = (a if cn & (4 >> ax) else w)[m, l, ax]
    v[m, l, cn] = R.corner_value(g, w[m, l], a[m, l], cn, **{("fx", "fy", "fz")[ax]: flipped})
    out["w where 1 - w belongs"] = v
    if c.interp == 2:
        _, raw, _, _ = R.contributions_f32(c.x01, c.gout, c.res, c.log2T, c.F, 2, smooth=False)
        v = vals.copy()
        v[m, l] = raw[m, l]
        out["unsmoothed w"] = v
    return keys, vals, out


@pytest.mark.parametrize("interp", [1, 2])
def test_mutations_break_the_dyadic_equality(interp):
    c = R.dyadic_case(interp, 8200, repeat=True)
    ref = _ref(c)
    _assert_all_exact(c, ref)
    keys, vals, mutants = _mutants(c)
    nrows = len(c.res) << c.log2T
    np.testing.assert_array_equal(R.serial_sum(keys, vals, nrows).astype(np.float64), ref.grad)
    assert len(mutants) == 2 + interp
    for name, v in mutants.items():
        assert not np.array_equal(R.serial_sum(keys, v, nrows).astype(np.float64), ref.grad), name
    # the smallest contribution of the whole scatter (one granule of the finest weights) is seen as well
    mag = np.where(vals == 0, np.inf, np.abs(vals))
    v = vals.copy()
    v[np.unravel_index(int(np.argmin(mag)), vals.shape)] = 0
    assert not np.array_equal(R.serial_sum(keys, v, nrows).astype(np.float64), ref.grad)


@pytest.mark.parametrize("interp", [1, 2])
def test_mutations_break_the_generic_bound(interp):
    c = R.generic_case(interp, 6000, L=8, log2T=10)
    ref = _ref(c)
    keys, vals, mutants = _mutants(c)
    nrows = len(c.res) << c.log2T
    _assert_within(R.serial_sum(keys, vals, nrows), ref)
    assert len(mutants) == 2 + interp
    for name, v in mutants.items():
        err = np.abs(R.serial_sum(keys, v, nrows).astype(np.float64) - ref.grad)
        assert np.any(err > R.tol_row(ref)), name


@pytest.mark.parametrize("interp", [1, 2])
def test_touched_counts_zero_weight_corners(interp):
    """hashgrid_bwd_pairs marks every corner row's segment, also where the weight is 0: a map of the non-zero
    contributions alone differs on the dyadic inputs (cell-boundary points, levels without fraction bits)."""
    c = R.dyadic_case(interp, 8200)
    ref = _ref(c)
    keys, vals, w, a = R.contributions_f32(c.x01, c.gout, c.res, c.log2T, c.F, interp)
    nrows = len(c.res) << c.log2T
    np.testing.assert_array_equal(R.touched_map(keys, nrows), ref.touched)
    weights = np.stack([R.corner_value(np.ones(keys.shape[:2] + (1,), np.float32), w, a, k)[..., 0]
                        for k in range(8)], -1)
    assert not np.array_equal(R.touched_map(keys, nrows, weights != 0), ref.touched)
