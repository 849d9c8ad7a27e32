"""Importance resampling by its definition, the reference of tests/test_resample_*.py: a plain
sequential float64 evaluation per ray on the fp32 inputs, widened exactly; nothing here is shared with the package.

    edges       b_i = (t_i + t_{i+1}) / 2                  i = 0 .. S-2
    bin masses  p_i = w_{i+1} + 1e-5                       i = 0 .. S-3
    CDF         c_0 = 0, c_k = p_0 + .. + p_{k-1}, C = c_{S-2}      (summed front to back, not normalised)
    quantiles   v_j = (j + r_j) / F * C                    r_j the jitter, or 0.5
    k the largest index in [0, S-3] with c_k <= v_j; f = clamp((v_j - c_k) / (c_{k+1} - c_k), 0, 1), 0 for a
    non-positive denominator; t_fine_j = b_k + f (b_{k+1} - b_k), rounded to fp32 once.

Also the test inputs: t values near (1 - lin) + far lin, weights from real compositing of a sparse density (about 70 %
of them exactly 0), and the special rows."""
import math

import numpy as np
import torch

OFFSETS = (0.0, 100.0, 5000.0)
KINDS = ("zero", "onehot", "flat", "nan")
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # the largest fp32 below 1
BOUND = 2 * 2.0 ** -24   # |t_fine - ref| <= BOUND * max|t_row|: the result's own fp32 rounding, and the one a
#                          different float64 summation order of the CDF can flip


def edges(t_vals):
    """float64 (N, S-1) bin edges."""
    t = np.asarray(t_vals, dtype=np.float64)
    return (t[:, :-1] + t[:, 1:]) / 2


def resample(weights, t_vals, n_fine, jitter=None):
    """t_fine (N, F) float32 by the definition; a row with NaN t values comes out as NaN or garbage, like the
    kernel's."""
    w = np.asarray(weights, dtype=np.float64)
    b = edges(t_vals)
    N, S = w.shape
    F = int(n_fine)
    out = np.empty((N, F), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in range(N):
            c = np.zeros(S - 1)
            for i in range(S - 2):          # front to back
                c[i + 1] = c[i] + (w[n, i + 1] + 1e-5)
            r = 0.5 if jitter is None else np.asarray(jitter[n], dtype=np.float64)
            v = (np.arange(F, dtype=np.float64) + r) / F * c[-1]
            k = np.clip(np.searchsorted(c[:-1], v, side="right") - 1, 0, S - 3)
            den = c[k + 1] - c[k]
            f = np.clip(np.where(den > 0, (v - c[k]) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
            out[n] = (b[n, k] + f * (b[n, k + 1] - b[n, k])).astype(np.float32)
    return out


def uniform_row(t_row, n_fine, jitter_row=None):
    """float64 (F,) resampling of a ray whose bins all weigh the same (every weight 0): bin k = floor(u (S-2)), the
    rest of u (S-2) the position in it -- written without the CDF, so independent of how it is summed."""
    t = np.asarray(t_row, dtype=np.float64)
    b = (t[:-1] + t[1:]) / 2
    F, nb = int(n_fine), t.shape[0] - 2
    r = 0.5 if jitter_row is None else np.asarray(jitter_row, dtype=np.float64)
    pos = (np.arange(F) + r) / F * nb
    k = np.clip(np.floor(pos).astype(np.int64), 0, nb - 1)
    return b[k] + (pos - k) * (b[k + 1] - b[k])


def onehot_outside_max(S, F):
    """How many of the F samples of a ray with one weight 1 (all others 0) may fall outside that weight's bin: the
    other S-3 bins hold 1e-5 each of C = 1 + (S-2) 1e-5, so F (S-3) 1e-5 / C quantiles on average, at most that
    rounded up plus one (the stratified quantiles are 1 / F apart)."""
    C = 1.0 + (S - 2) * 1e-5
    return math.ceil(F * (S - 3) * 1e-5 / C) + 1


def composite(sigma, dt):
    """Front-to-back weights alpha_i T_i of one ray's densities and step lengths (fp32 in, fp32 out)."""
    alpha = 1.0 - torch.exp(-sigma.double() * dt.double())
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha]), 0)[:-1]
    return (alpha * T).float()


def case(N, S, F, offset, seed=0):
    """A test case: dict with fp32 CPU tensors ``w``, ``t`` (N, S), ``jitter`` (N, F), and ``rows`` = {kind: row index}
    of the special rows present.  t = near (1 - lin) + far lin with near in [offset + 2, offset + 3); about 70 % of the
    densities behind the weights are exactly 0.  Special rows (as many as fit next to one ordinary row, rotating with
    the offset so that small N still meets each kind): ``zero`` all weights 0, ``onehot`` one inner weight 1 and the
    rest 0 (an opaque sample), ``flat`` near == far (every edge equal: all ties in the merge), ``nan`` NaN t values.
    Even jitter rows start with exactly 0.0, odd rows end with the largest fp32 below 1 (both in one row when
    F >= 2)."""
    gen = torch.Generator().manual_seed(1000 * S + 10 * F + OFFSETS.index(offset) + seed)
    near = offset + 2.0 + torch.rand(N, generator=gen)
    far = near + 5.0 + 45.0 * torch.rand(N, generator=gen)
    lin = torch.linspace(0.0, 1.0, S)
    t = (near[:, None] * (1.0 - lin) + far[:, None] * lin).float()
    rows = {}
    q = OFFSETS.index(offset)
    for i in range(min(len(KINDS), N - 1)):
        rows[KINDS[(q + i) % len(KINDS)]] = i
    if "flat" in rows:
        t[rows["flat"]] = t[rows["flat"], 0]
    d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1)
    w = torch.empty(N, S)
    for n in range(N):
        sig = torch.rand(S, generator=gen) * 4.0 * (torch.rand(S, generator=gen) < 0.3)
        w[n] = composite(sig, d[n])
    if "zero" in rows:
        w[rows["zero"]] = 0.0
    if "onehot" in rows:
        w[rows["onehot"]] = 0.0
        w[rows["onehot"], onehot_index(S)] = 1.0
    if "nan" in rows:
        t[rows["nan"]] = float("nan")
    jitter = torch.rand(N, F, generator=gen)
    jitter[0::2, 0] = 0.0
    jitter[1::2, -1] = ONE_BELOW
    if F >= 2:
        jitter[0::2, -1] = ONE_BELOW
    assert float(jitter.max()) < 1.0 and float(jitter.min()) == 0.0
    return {"w": w, "t": t, "jitter": jitter, "rows": rows}


def onehot_index(S):
    """The sample that carries the opaque ray's weight: an inner one (its bin is onehot_index - 1)."""
    return max(1, S // 2) if S > 3 else 1


def finite_rows(c):
    keep = torch.ones(c["t"].shape[0], dtype=torch.bool)
    if "nan" in c["rows"]:
        keep[c["rows"]["nan"]] = False
    return keep
