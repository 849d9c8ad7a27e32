"""Reference of the hash grid's table-gradient scatter (acn_hashgrid_bwd, acn_hashgrid_bwd_pairs[_sumsq|_segmap],
acn_hashgrid_pairs_mark): numpy, float64, no GPU.

The operation.  For every point m and level l the cell comes from the FLOAT32 product s = x * res_l (part of the
operation's definition, as input_grad_ref's weights="fp32" and test_hash_det.serial_scatter): i0 = floor(s), and
w = s - floor(s), which float32 computes exactly.  Everything after that is float64 here: the smoothstep
w*w*(3 - 2w), the factors w / 1 - w of the three axes, their product with g and the sum over the contributions of a
row.  Nearest takes the one row at rint(s) (half to even) with weight 1.  Hash and corner set are those of
test_hash_det.serial_scatter: row = ((ix + bx) ^ (iy + by) * P1 ^ (iz + bz) * P2) mod 2^log2T, corner c = bx*4 +
by*2 + bz.

scatter_ref returns, per expert, grad (the sums), A (per row and feature, the sum of |g| over the contributions to
it, zero-weight corners included), n (contributions per row) and touched (the byte map of the 64-B segments that
hold a corner row of a live, unpadded slot).

Exact inputs (exact_rows).  Take x = j / 2^B and res_l = 2^p.  Then s = j * 2^(p - B) is exact in float32 and w is a
multiple of 2^-b with b = max(0, B - p) fraction bits (b = 0: all the weight sits on corner 0).
  Linear      w and 1 - w are multiples of 2^-b, so a corner weight (three factors) is a multiple of 2^-3b.
  Smoothstep  w*w is a multiple of 2^-2b and 3 - 2w of 2^-(b-1), so sw = (w*w) * (3 - 2w) and 1 - sw are multiples
              of 2^-(3b-1) (b >= 1; integers for b = 0), and a corner weight of 2^-3(3b-1).  float32 computes w*w
              (2b bits), 3 - 2w (b + 1 bits) and their product (3b + 1 bits) exactly for b <= 7.
  Nearest     the weight is 1.
With integer g every contribution c, and every intermediate product (g * wz), (g * wz) * wy, is a multiple of the
level's granule (2^-3b, 2^-3(3b-1), 1) bounded by |g|.  A partial sum of ANY subset of a row's contributions, in any
order and any grouping (registers, LDS, atomics), is a multiple of the granule bounded by A.  If A / granule < 2^24
it is a float32 number, so no addition ever rounds: every correct kernel returns grad bit for bit, and one lost,
doubled or misplaced contribution of any size changes the result.

Generic inputs (tol_row).  eps = 2^-24 is float32's unit roundoff.  A weight factor is reached from the exact w by
at most 4 roundings (w*w, 3 - 2w, their product, 1 - sw; Linear: one), each of relative error eps on a value whose
contribution to the factor is at most 1, so a factor carries at most 4 eps of absolute error and the product of
three factors (each <= 1) at most 12 eps to first order.  The three multiplications g * wz * wy * wx add 3 eps
relative: a contribution is off by at most 15 eps |g| + O(eps^2).  Adding the n computed contributions of a row in
any order adds at most (n - 1) eps sum|c| + O(eps^2) (each partial sum is bounded by sum|c| <= A).  The bound used is
    tol_row = (16 + n_row) * eps * A_row,
one eps |g| and one eps A more than the first-order terms 15 and n - 1: they cover the second-order terms
(below 120 eps^2 |g| + n^2 eps^2 A, far under eps A for n < 2^20).  No measurement is involved.

Telescoped norm (tele_exact).  acn_hashgrid_bwd_pairs_sumsq adds new^2 - old^2 of every atomic to a double.  On
exact inputs every old and new value of an element is a multiple of its granule q bounded by V = |init| + A, so its
square is a multiple of q^2 bounded by V^2, and a step from old to new changes the square by at most
|new - old| * 2V.  Over a row's steps that is at most 2 A V.  Any partial sum of the differences, in any grouping
(lane, wave, the device double with its starting value s0), is therefore a multiple of qmin^2 bounded by
|s0| + sum 2 A V.  If  |s0| + sum 2 A V + max V^2 < 2^53 qmin^2  every square, difference and partial sum is an exact
double and the device double gains exactly sum(final^2) - sum(init^2).
"""
from collections import namedtuple

import numpy as np

P1, P2 = np.uint32(2654435761), np.uint32(805459861)
EPS = 2.0 ** -24

Ref = namedtuple("Ref", "grad A n touched")


def cells(x01, res, log2T, interp):
    """(rows (M, L, C) int64 within the level, w (M, L, 3) float32 or None): C = 8 corners, Nearest C = 1."""
    x = np.asarray(x01, np.float32).reshape(-1, 3)
    r = np.asarray(res, np.float32)
    mask = np.uint32((1 << log2T) - 1)
    with np.errstate(over="ignore"):
        s = (x[:, None, :] * r[None, :, None]).astype(np.float32)
        if interp == 0:
            i = np.rint(s).astype(np.int64).astype(np.uint32)
            rows = (i[..., 0] ^ (i[..., 1] * P1) ^ (i[..., 2] * P2)) & mask
            return rows.astype(np.int64)[..., None], None
        f = np.floor(s)
        w = (s - f).astype(np.float32)
        i0 = f.astype(np.int64).astype(np.uint32)
        rows = np.empty(s.shape[:2] + (8,), np.int64)
        for c in range(8):
            bx, by, bz = c >> 2, (c >> 1) & 1, c & 1
            rows[..., c] = ((i0[..., 0] + np.uint32(bx)) ^ ((i0[..., 1] + np.uint32(by)) * P1)
                            ^ ((i0[..., 2] + np.uint32(bz)) * P2)) & mask
    return rows, w


def _corner_weights(w, a):
    """(M, L, 8): (z factor * y factor) * x factor of corner c = bx*4 + by*2 + bz, in the dtype of w."""
    out = np.empty(w.shape[:2] + (8,), w.dtype)
    for c in range(8):
        bx, by, bz = c >> 2, (c >> 1) & 1, c & 1
        out[..., c] = ((w[..., 2] if bz else a[..., 2]) * (w[..., 1] if by else a[..., 1])) * \
                      (w[..., 0] if bx else a[..., 0])
    return out


def scatter_ref(x01, gout, res, log2T, F, interp, pk=None, pidx=None, live=None, K=1):
    """List of K Ref(grad (L*T, F) f64, A (L*T, F) f64, n (L*T,) int64, touched (ceil(L*T/8),) uint8), one per
    expert.  Slots at index >= live and slots with pidx < 0 contribute nothing (their payloads are not read)."""
    x = np.asarray(x01, np.float32).reshape(-1, 3)
    cap, L, T = x.shape[0], len(res), 1 << log2T
    g = np.asarray(gout, np.float32).reshape(cap, L, F)
    keep = np.zeros(cap, bool)
    keep[:cap if live is None else int(live)] = True
    if pidx is not None:
        keep &= np.asarray(pidx) >= 0
    idx = np.nonzero(keep)[0]
    k = np.zeros(idx.size, np.int64) if pk is None else np.asarray(pk)[idx].astype(np.int64)
    assert idx.size == 0 or (k.min() >= 0 and k.max() < K)
    rows, w = cells(x[idx], res, log2T, interp)
    g64 = g[idx].astype(np.float64)
    if interp == 0:
        wt = np.ones(rows.shape, np.float64)
    else:
        w = w.astype(np.float64)
        if interp == 2:
            w = (w * w) * (3.0 - 2.0 * w)
        wt = _corner_weights(w, 1.0 - w)
    key = ((k[:, None, None] * L + np.arange(L)[None, :, None]) * T + rows).ravel()
    size = K * L * T
    grad = np.stack([np.bincount(key, (g64[:, :, None, f] * wt).ravel(), size) for f in range(F)], -1)
    A = np.stack([np.bincount(key, np.broadcast_to(np.abs(g64[:, :, None, f]), wt.shape).ravel(), size)
                  for f in range(F)], -1)
    n = np.bincount(key, minlength=size)
    nb = (L * T + 7) // 8
    touched = np.zeros((K, nb), np.uint8)
    touched[key // (L * T), (key % (L * T)) >> 3] = 1
    return [Ref(grad[e * L * T:(e + 1) * L * T], A[e * L * T:(e + 1) * L * T], n[e * L * T:(e + 1) * L * T],
                touched[e]) for e in range(K)]


def tol_row(ref):
    """(L*T, F) bound of |fp32 scatter in any order - grad| for generic inputs (module docstring)."""
    return (16.0 + ref.n)[:, None] * EPS * ref.A


def level_granule(res, B, interp):
    """(L,) float64: the power of two dividing every contribution of the level, for x = j / 2^B, integer g."""
    out = []
    for r in res:
        p = int(r).bit_length() - 1
        assert int(r) == 1 << p and 0 <= B <= 23, "dyadic inputs need power-of-two resolutions"
        b = max(0, B - p)
        if interp == 0:
            e = 0
        elif interp == 1:
            e = 3 * b
        else:
            assert b <= 7, "float32 computes w*w*(3 - 2w) exactly only up to 7 fraction bits"
            e = 3 * (3 * b - 1) if b else 0
        out.append(2.0 ** -e)
    return np.asarray(out)


def row_granule(res, B, interp, log2T):
    """(L*T, 1) granule per row."""
    return np.repeat(level_granule(res, B, interp), 1 << log2T)[:, None]


def exact_rows(A, granule):
    """(rows,) bool: every partial sum of the row's contributions is a float32 number (module docstring)."""
    return np.all(np.asarray(A) / granule < 2.0 ** 24, axis=-1)


def tele_exact(A, init, gmin, s0=0.0):
    """The telescoped sum of squares is exact in doubles (module docstring)."""
    V = np.abs(np.asarray(init, np.float64)) + A
    return abs(s0) + float(np.sum(2.0 * A * V)) + float(V.max() ** 2) < 2.0 ** 53 * gmin * gmin


# ---------------------------------------------------------------------------------------------------- fp32 scatter
def contributions_f32(x01, gout, res, log2T, F, interp, smooth=True):
    """The float32 kernels' contributions: keys (M, L, C) int64 rows of the whole table, vals (M, L, C, F) float32
    = ((g * wz') * wy') * wx', and the factors (w, a = 1 - w) (M, L, 3) float32 (None for Nearest).
    smooth=False leaves the Smoothstep w unsmoothed (a mutation)."""
    L, T = len(res), 1 << log2T
    rows, w = cells(x01, res, log2T, interp)
    M = rows.shape[0]
    g = np.asarray(gout, np.float32).reshape(M, L, 1, F)
    keys = np.arange(L, dtype=np.int64)[None, :, None] * T + rows
    if interp == 0:
        return keys, g.copy(), None, None
    if interp == 2 and smooth:
        w = ((w * w) * (np.float32(3.0) - np.float32(2.0) * w)).astype(np.float32)
    a = (np.float32(1.0) - w).astype(np.float32)
    vals = np.empty((M, L, 8, F), np.float32)
    for c in range(8):
        vals[:, :, c] = corner_value(g[:, :, 0], w, a, c)
    return keys, vals, w, a


def corner_value(g, w, a, c, fz=None, fy=None, fx=None):
    """((g * z factor) * y factor) * x factor of corner c in float32; fz / fy / fx replace a factor."""
    bx, by, bz = c >> 2, (c >> 1) & 1, c & 1
    fz = (w[..., 2] if bz else a[..., 2]) if fz is None else fz
    fy = (w[..., 1] if by else a[..., 1]) if fy is None else fy
    fx = (w[..., 0] if bx else a[..., 0]) if fx is None else fx
    g = np.asarray(g, np.float32)
    return (((g * fz[..., None]).astype(np.float32) * fy[..., None]).astype(np.float32)
            * fx[..., None]).astype(np.float32)


def serial_sum(keys, vals, nrows, order=None):
    """(nrows, F) float32: the contributions added one by one in fp32 (np.add.at is sequential), points in
    ``order`` (a permutation of the points; default: ascending), corners in order within a point and level."""
    tab = np.zeros((nrows, vals.shape[-1]), np.float32)
    if order is not None:
        keys, vals = keys[order], vals[order]
    np.add.at(tab, keys.reshape(-1), vals.reshape(-1, vals.shape[-1]))
    return tab


def touched_map(keys, nrows, select=None):
    """Byte map of the 64-B segments of ``keys`` (those where ``select`` is true)."""
    m = np.zeros((nrows + 7) // 8, np.uint8)
    m[(keys if select is None else keys[select]).reshape(-1) >> 3] = 1
    return m


def chunk_segments(x01, res_l, log2T, interp=1):
    """Distinct 64-B segments (8 rows) that the corners of these points touch at one level."""
    rows, _ = cells(x01, [res_l], log2T, interp)
    return int(np.unique(rows >> 3).size)


# --------------------------------------------------------------------------------------------------- input builders
def dyadic_points(M, B, rng, repeat=False):
    """(M, 3) float32 points j / 2^B, j in [0, 2^B].  Among them (from M >= 2 on, half of M at the most) the corners
    (0,0,0) and (1,1,1), cell-boundary points of every level, the exact .5 ties of Nearest and the smallest
    fractions.  repeat: every point stands a random 1..40 times in a row (runs across the 16-point lane stretch,
    the 64-point wave and expert boundaries)."""
    N = 1 << B
    j = rng.integers(0, N + 1, size=(M, 3))
    special = np.array([[0, 0, 0], [N, N, N], [N // 2, N // 2, N // 2], [N // 4, N // 2, 3 * N // 4], [1, 1, 1],
                        [N - 1, N - 1, N - 1], [0, N, 0], [N, 0, N // 2], [N // 2 + 1, N // 8, 3 * N // 8],
                        [N // 16, N - N // 16, N // 2 - 1], [3, N // 4 + 2, N // 2 + N // 4], [N, N, 0]])
    k = min(len(special), M // 2)
    j[1:1 + k] = special[:k]
    if repeat:
        j = np.repeat(j, rng.integers(1, 41, size=M), axis=0)[:M]
    return (j / float(N)).astype(np.float32)


def int_grads(M, width, gmax, rng):
    """(M, width) float32 integers in [-gmax, gmax]."""
    return rng.integers(-gmax, gmax + 1, size=(M, width)).astype(np.float32)


def int_table(rows, F, vmax, rng):
    """(rows, F) float32 integers in [-vmax, vmax]: a pre-filled gradient table."""
    return rng.integers(-vmax, vmax + 1, size=(rows, F)).astype(np.float32)


DyadicCase = namedtuple("DyadicCase", "x01 gout res B log2T F interp")

# fraction widths b = max(0, B - log2 res): zero (all the weight on corner 0) and several non-zero widths land both
# on levels 0..5 (hashgrid_bwd_merge) and on levels >= 6 (hashgrid_bwd_rle); the lists are not monotonic
_RES = {  # (small table, interp != 2) -> (B, resolutions cycled over the levels, max |g|)
    (False, False): (10, [1024, 512, 256, 128, 64, 64, 128, 2048], 8),
    (False, True): (8, [256, 128, 64, 64, 128, 256, 512, 64], 4),
    # log2T <= 4: a handful of rows takes every contribution, so fewer fraction bits and smaller gradients
    (True, False): (4, [16, 8, 4, 4, 8, 16, 32, 4], 2),
    (True, True): (4, [16, 8, 16, 32, 8, 8, 16, 8], 2),
}


def dyadic_case(interp, M, L=8, log2T=14, F=2, repeat=False, seed=0, B=None):
    """Dyadic points, power-of-two resolutions and small integer gradients on which the scatter is exact.
    ``B`` below the default leaves fewer fraction bits (a coarser granule: the telescoped norm needs it)."""
    B0, base, gmax = _RES[log2T <= 4, interp == 2]
    B = B0 if B is None else B
    rng = np.random.default_rng([seed, interp, M, L, log2T, F, int(repeat), B])
    res = [base[l % len(base)] for l in range(L)]
    return DyadicCase(dyadic_points(M, B, rng, repeat), int_grads(M, L * F, gmax, rng), res, B, log2T, F, interp)


def generic_case(interp, M, L=8, log2T=12, F=2, seed=0, kind="uniform"):
    """Generic float inputs: uniform points, points clustered along a few rays, or all points identical; the
    resolutions grow geometrically from 16 to 1024 and the gradients are normal."""
    rng = np.random.default_rng([seed, interp, M, L, log2T, F])
    res = np.floor(16 * np.exp(np.arange(L) * (np.log(1024 / 16) / max(1, L - 1))) + 0.5).astype(int).tolist()
    if kind == "uniform":
        x = rng.random((M, 3))
    elif kind == "rays":
        R = max(1, M // 150)
        o, d = rng.random((R, 1, 3)) * 0.8 + 0.1, rng.normal(size=(R, 1, 3))
        d = d / np.linalg.norm(d, axis=-1, keepdims=True) * 0.08
        t = np.linspace(0, 1, (M + R - 1) // R)[None, :, None]
        x = np.clip((o + d * t).reshape(-1, 3)[:M], 1e-6, 1 - 1e-6)
    else:
        x = np.broadcast_to(rng.random((1, 3)), (M, 3))
    g = rng.normal(size=(M, L * F)) * rng.choice([1e-3, 1.0, 30.0], size=(M, 1))
    return DyadicCase(np.ascontiguousarray(x, np.float32), g.astype(np.float32), res, None, log2T, F, interp)


PairList = namedtuple("PairList", "x01 gout pk pidx seg live K")


def pair_list(counts, x_live, g_live, rng, tail=37, pad_frac=0.2):
    """The routed pair list of ``counts`` live slots per expert from (sum(counts), 3) points and (sum(counts), W)
    gradients.  The buffers are ``tail`` slots longer than seg[K]; the tail holds NaN x01, NaN gout, a valid pk and
    pidx >= 0, so a kernel that reads it fails the comparison and faults nothing.  A random ``pad_frac`` of the
    live slots is padding (pidx = -1) with NaN payloads and a valid pk.  Around every expert boundary the four
    slots (two on either side, where the experts have them) hold the same point and are not padding: the same
    cell, and a lane's run, repeated across the boundary."""
    K, live = len(counts), int(sum(counts))
    cap = live + tail
    x = np.full((cap, 3), np.nan, np.float32)
    g = np.full((cap, g_live.shape[1]), np.nan, np.float32)
    x[:live], g[:live] = x_live, g_live
    pk = np.zeros(cap, np.int32)
    pk[:live] = np.repeat(np.arange(K, dtype=np.int32), counts)
    pk[live:] = K - 1
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pad = np.zeros(cap, bool)
    pad[:live] = rng.random(live) < pad_frac
    for b in seg[1:-1]:
        lo, hi = max(0, int(b) - 2), min(live, int(b) + 2)
        if lo < b < hi:
            x[lo:hi] = x[lo]
            pad[lo:hi] = False
    x[pad], g[pad] = np.nan, np.nan
    pidx = np.arange(cap, dtype=np.int32)
    pidx[pad] = -1
    return PairList(x, g, pk, pidx, seg, live, K)
