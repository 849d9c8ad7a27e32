"""The definition of the fused per-image affine colour loss (acn_appearance_mse / acn_appearance_apply, DESIGN.md
§4ad) in numpy, and the seeded inputs its tests share.

Per ray r with slot s and channel k, n = 3 N:
  c      = fl32(A[s,k,0] p0 + A[s,k,1] p1 + A[s,k,2] p2 + b[s,k])   float64 from the fp32 inputs, left to right, cast once
           (a slot < 0 or >= I: c = p_k, no parameter gradient)
  d      = clamp01(c) - gt_linear(gt)                                 float32: bit-exact against the kernel wherever
                                                                      gt_linear takes no powf (gt <= 0.04045 or >= 1)
  loss   = sum d^2 / n                                                float64 from here on
  g_c    = fl32((2 / n) d) where 0 <= c <= 1, else 0
  g_pred[r,j] = sum_k A[s,k,j] g_c[k]   (g_c[j] without a slot)
  g_A[i,k,j]  = sum_{r: slot = i} g_c[r,k] p[r,j],   g_b[i,k] = sum_{r: slot = i} g_c[r,k]
``reference`` returns the float64 values (the kernel rounds each to fp32 once).
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64

# the ray workgroups' loop boundaries (appearance.hip: 64 lanes, 256 threads, 256 workgroups: one ray per thread up to
# 65536 rays, a second one past it) and the numbers of slots
N_CASES = (1, 63, 64, 65, 257, 1000, 4099, 65536, 65537)
I_CASES = (1, 3, 70, 300)
LAYOUTS = ("mixed", "one", "none")
POW_DELTA = 2.0 ** -23   # how far one ulp of gt_linear's powf moves d (see test_generic_targets)


def clamp01(x):
    """The kernels' clamp: NaN passes."""
    x = np.asarray(x, F32)
    return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


def gt_linear(gt):
    """clamp01(srgb_to_linear(clamp01(gt))) with the kernels' float scalars.  The linear branch is one correctly
    rounded fp32 division: bit-exact.  The powf branch is evaluated in float64 and rounded (correctly rounded up to
    double rounding); the device's powf may differ from it by an ulp."""
    x = clamp01(gt)
    lin = (x / F32(12.92)).astype(F32)
    base = ((x + F32(0.055)).astype(F32) / F32(1.055)).astype(F32)
    with np.errstate(invalid="ignore"):
        pw = np.power(base.astype(F64), F64(F32(2.4))).astype(F32)
    return clamp01(np.where(x <= F32(0.04045), lin, pw))


def corrected64(pred, slot, A, b):
    """(c in float64 before the cast, has-a-slot mask)."""
    I = A.shape[0]
    has = (slot >= 0) & (slot < I)
    s = np.where(has, slot, 0)
    p, As, bs = pred.astype(F64), A[s].astype(F64), b[s].astype(F64)
    c = ((As[:, :, 0] * p[:, None, 0] + As[:, :, 1] * p[:, None, 1]) + As[:, :, 2] * p[:, None, 2]) + bs
    return c, has


def corrected(pred, slot, A, b):
    """c (N, 3) float32: acn_appearance_apply's output."""
    c, has = corrected64(pred, slot, A, b)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(has[:, None], c.astype(F32), pred).astype(F32)


def reference(pred, gt, slot, A, b):
    """dict of c, d, g_c (float32, exact where gt_linear is) and loss, g_pred, g_A, g_b (float64)."""
    N, I = slot.shape[0], A.shape[0]
    n = 3 * N
    _, has = corrected64(pred, slot, A, b)
    c = corrected(pred, slot, A, b)
    d = (clamp01(c) - gt_linear(gt)).astype(F32)
    d64 = d.astype(F64)
    loss = float(np.sum(d64 * d64) / n)
    live = (c >= 0) & (c <= 1)
    g_c = np.where(live, ((2.0 / n) * d64).astype(F32), F32(0)).astype(F32)
    g64, p64 = g_c.astype(F64), pred.astype(F64)
    As = A[np.where(has, slot, 0)].astype(F64)
    g_pred = As[:, 0, :] * g64[:, 0:1] + As[:, 1, :] * g64[:, 1:2] + As[:, 2, :] * g64[:, 2:3]
    g_pred = np.where(has[:, None], g_pred, g64)
    g_A, g_b = np.zeros((I, 3, 3), F64), np.zeros((I, 3), F64)
    np.add.at(g_A, slot[has], g64[has][:, :, None] * p64[has][:, None, :])
    np.add.at(g_b, slot[has], g64[has])
    return {"c": c, "d": d, "g_c": g_c, "live": live, "has": has, "loss": loss, "g_pred": g_pred, "g_A": g_A,
            "g_b": g_b}


def boundary_margin(pred, slot, A, b):
    """Per element with a slot: the distance of the float64 c from the nearest fp32 rounding boundary (the midpoint
    of two neighbouring floats), relative to |c|; inf without a slot."""
    c, has = corrected64(pred, slot, A, b)
    r = c.astype(F32)
    up = (r.astype(F64) + np.nextafter(r, F32(np.inf)).astype(F64)) / 2
    dn = (r.astype(F64) + np.nextafter(r, F32(-np.inf)).astype(F64)) / 2
    dist = np.minimum(np.abs(c - up), np.abs(c - dn)) / np.maximum(np.abs(c), 1e-300)
    return np.where(has[:, None], dist, np.inf)


def _slots(rng, N, I, layout):
    if layout == "none":                       # no ray has a slot: every slot is empty
        r = np.arange(N)
        return np.where(r % 2 == 0, -1, I + r % 3).astype(np.int32)
    if layout == "one":                        # every ray in the last slot: the others are empty
        return np.full(N, I - 1, np.int32)
    s = rng.integers(0, I, N)                  # mixed: slot I // 2 is kept empty when there is another
    if I > 1:
        s = np.where(s == I // 2, (I // 2 + 1) % I, s)
    u = rng.random(N)
    s = np.where(u < 0.1, -1, np.where(u < 0.15, I + rng.integers(0, 5, N), s))
    if N >= 3:
        s[1], s[2] = -1, I
    return s.astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(N, I, layout="mixed", targets="linear", seed=0):
    """(pred (N,3), gt (N,3), slot (N,) int32, A (I,3,3), b (I,3)) float32, seeded.  Predictions in [-0.2, 1.2] (ray 0: -0.3, 0.5, 0.5) and
    matrices near the identity put a good tenth of the corrected colours into the clamp's dead zone on either side.
    ``targets`` "linear": on gt_linear's linear branch (<= 0.04045) or at / above 1, where d is bit-exact; "generic":
    anywhere in [-0.1, 1.1], mostly through powf.  Rays whose c comes within relative 2^-40 of an fp32 rounding
    boundary are drawn again, so that a round-once evaluation in any order casts to the same float."""
    rng = np.random.default_rng([N, I, LAYOUTS.index(layout), seed])
    pred = (rng.random((N, 3)) * 1.4 - 0.2).astype(F32)
    pred[0] = (-0.3, 0.5, 0.5)   # the smallest case, one ray, has a dead and two live channels too
    if targets == "linear":
        u = rng.random((N, 3))
        gt = np.where(u < 0.45, rng.random((N, 3)) * 0.04045, np.where(u < 0.55, 1.0, 1.0 + rng.random((N, 3)) * 0.2))
        gt = gt.astype(F32)
        gt[gt > F32(0.04045)] = np.maximum(gt[gt > F32(0.04045)], F32(1))
    else:
        gt = (rng.random((N, 3)) * 1.2 - 0.1).astype(F32)
    A = (np.eye(3)[None] + 0.15 * rng.standard_normal((I, 3, 3))).astype(F32)
    b = (0.05 * rng.standard_normal((I, 3))).astype(F32)
    slot = _slots(rng, N, I, layout)
    for _ in range(8):
        bad = (boundary_margin(pred, slot, A, b) <= 2.0 ** -40).any(1)
        if not bad.any():
            break
        pred[bad, 1:] = (rng.random((int(bad.sum()), 2)) * 1.4 - 0.2).astype(F32)   # ray 0 keeps its first channel
    for x in (pred, gt, slot, A, b):
        x.setflags(write=False)
    return pred, gt, slot, A, b


@functools.lru_cache(maxsize=None)
def case(N, I, layout="mixed", targets="linear", seed=0):
    """(inputs, reference) of one case, computed once per process and shared read-only."""
    x = inputs(N, I, layout, targets, seed)
    return x, reference(*x)


def dyadic_inputs(N, I, seed=0):
    """Inputs on which every product and sum of the definition is exact in any order: pred multiples of 2^-6 in
    [-0.25, 1.25], A entries from {0, +-1/2, 1, 2}, b multiples of 2^-4, gt in {0, 1}, N a power of two (2 / n times d
    is then one rounding of a dyadic number times 1/3: g_c is the same fp32 for a ray wherever it stands)."""
    assert N & (N - 1) == 0
    rng = np.random.default_rng([N, I, 77, seed])
    pred = (rng.integers(-16, 81, (N, 3)) / 64.0).astype(F32)
    A = rng.choice(np.array([0, 0.5, -0.5, 1, 2], F32), (I, 3, 3)).astype(F32)
    b = (rng.integers(-4, 5, (I, 3)) / 16.0).astype(F32)
    gt = rng.integers(0, 2, (N, 3)).astype(F32)
    slot = rng.integers(-1, I + 1, N).astype(np.int32)
    if I > 1:
        slot[slot == I // 2] = -1   # an empty slot
    return pred, gt, slot, A, b


def loss_chain_f64(pred, gt_lin, slot, A, b):
    """The same formula as float64 torch ops (for autograd): mean((clamp01(A[s] p + b[s]) - gt_lin)^2)."""
    import torch
    I = A.shape[0]
    has = (slot >= 0) & (slot < I)
    s = slot.clamp(0, I - 1).long()
    c = (A[s] * pred[:, None, :]).sum(-1) + b[s]
    c = torch.where(has[:, None], c, pred)
    return ((c.clamp(0, 1) - gt_lin) ** 2).mean()
