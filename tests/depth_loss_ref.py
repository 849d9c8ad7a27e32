"""Depth supervision by its definition in float64, the reference of tests/test_depth_loss_*.py.  For one
ray with weights w_i over the intervals [s_i, e_i], per-sample depths tau_i, a target z, a half-width eps, a scale c:

    sigma = eps / 3, lo = z - eps, hi = z + eps, Phi the standard normal CDF
    k_i      = Phi((min(e_i, hi) - z) / sigma) - Phi((max(s_i, lo) - z) / sigma) if min(e_i, hi) > max(s_i, lo) else 0
    m_i      = 1 if s_i < hi else 0
    L        = l_d (c (sum_i w_i tau_i - z))^2 + l_s sum_i m_i (w_i - k_i)^2
    dL/dw_i  = 2 l_d c^2 (sum_j w_j tau_j - z) tau_i + 2 l_s m_i (w_i - k_i)

and an exact 0 for a ray whose z or eps is not finite or <= 0, or whose c is 0.  Dense (N, S) layout: s = tau = t,
e = t + d with volume_render's ``dists``; packed: s = t0, e = t1, tau = (t0 + t1) / 2.  The inputs are taken as they are
(fp32 values widened exactly); nothing here is shared with the package's code.

Also the test inputs, computed once and never modified: distortion_ref's composited weights, and per ray a target inside
a drawn interval (kidx = randint(S // 4, 3 S // 4), z = t[kidx] + rand * d[kidx] in fp32), eps = 1.5 mean spacings,
c = 1 / (t_last - t_first)."""
import math
from functools import lru_cache

import torch

import distortion_ref as R

OFFSETS = (0.0, 100.0, 5000.0)
DENSE_SHAPES = [(37, 2), (5, 64), (3, 65), (64, 96), (9, 256), (2, 1000)]
PACKED_COUNTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 300, 17, 0, 91, 200]
OPAQUE_RAY = 5
LAMBDAS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0))
K3 = math.erf(3.0 / math.sqrt(2.0))   # Phi(3) - Phi(-3)


def phi(x):
    return 0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def kernel_mass(s, e, z, eps):
    """k (float64) of the intervals [s, e] for the target z and half-width eps (python floats)."""
    sigma, lo, hi = eps / 3.0, z - eps, z + eps
    x0, x1 = torch.clamp(s, min=lo), torch.clamp(e, max=hi)
    return torch.where(x1 > x0, phi((x1 - z) / sigma) - phi((x0 - z) / sigma), torch.zeros_like(s))


def dead(z, eps, c):
    return not (math.isfinite(z) and z > 0 and math.isfinite(eps) and eps > 0) or c == 0.0


def ray_loss(w, s, e, tau, z, eps, c=1.0, ld=1.0, ls=1.0):
    """(L, dL/dw) of one ray: float64 (S,) weights (may require grad), interval starts, ends and depths; z, eps, c
    python floats (the fp32 inputs widened)."""
    if dead(z, eps, c):
        return w.sum() * 0.0, torch.zeros_like(w)
    k = kernel_mass(s, e, z, eps)
    m = (s < z + eps).double()
    D = (w * tau).sum()
    loss = ld * (c * (D - z)) ** 2 + ls * (m * (w - k) ** 2).sum()
    grad = 2.0 * ld * c * c * (D - z) * tau + 2.0 * ls * m * (w - k)
    return loss, grad


def dense_intervals(t_vals):
    """float64 (s, e, tau) of (N, S) t values: dists in the precision of t, widened before the sum."""
    d = (t_vals[:, 1:] - t_vals[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1).double()
    t = t_vals.double()
    return t, t + d, t


def _c(ray_scale, r):
    return 1.0 if ray_scale is None else float(ray_scale[r])


def dense(weights, t_vals, z, eps, ray_scale=None, ld=1.0, ls=1.0):
    """(loss (N,), grad (N, S)) float64."""
    w = weights.detach().double()
    N, S = w.shape
    loss, grad = torch.zeros(N, dtype=torch.float64), torch.zeros(N, S, dtype=torch.float64)
    for r in range(N):
        zr, er, cr = float(z[r]), float(eps[r]), _c(ray_scale, r)
        if dead(zr, er, cr):
            continue   # before any look at the ray's t values
        s, e, tau = dense_intervals(t_vals[r:r + 1])
        loss[r], grad[r] = ray_loss(w[r], s[0], e[0], tau[0], zr, er, cr, ld, ls)
    return loss, grad


def packed(weights, t0, t1, starts, counts, z, eps, ray_scale=None, ld=1.0, ls=1.0):
    """(loss (N,), grad (M,)) float64; an empty ray has D = 0."""
    w, a, b = weights.detach().double(), t0.double(), t1.double()
    N = starts.numel()
    loss, grad = torch.zeros(N, dtype=torch.float64), torch.zeros_like(w)
    for r in range(N):
        zr, er, cr = float(z[r]), float(eps[r]), _c(ray_scale, r)
        if dead(zr, er, cr):
            continue
        sl = slice(int(starts[r]), int(starts[r]) + int(counts[r]))
        loss[r], grad[sl] = ray_loss(w[sl], a[sl], b[sl], 0.5 * (a[sl] + b[sl]), zr, er, cr, ld, ls)
    return loss, grad


def window_counts(s, e, z, eps):
    """(samples overlapping the window, samples wholly in front of it) of one ray."""
    lo, hi = z - eps, z + eps
    over = (torch.clamp(e, max=hi) > torch.clamp(s, min=lo))
    return int(over.sum()), int((e <= lo).sum())


@lru_cache(maxsize=None)
def dense_inputs(shape, offset):
    """(w, t, z, eps, c) fp32 on the CPU for one dense shape and t offset."""
    N, S = shape
    gen = torch.Generator().manual_seed(300 + 7 * S + int(offset))
    w, t = R.dense_case(N, S, offset, gen, opaque_ray=0)
    assert float(w[0, 0]) == 1.0 and bool((w[0, 1:] == 0).all())          # the opaque-first ray
    d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1)
    kidx = torch.randint(S // 4, max(3 * S // 4, S // 4 + 1), (N,), generator=gen)
    frac = torch.rand(N, generator=gen)
    rows = torch.arange(N)
    z = (t[rows, kidx] + frac * d[rows, kidx]).float()
    length = t[:, -1] - t[:, 0]
    eps = (1.5 * length / (S - 1)).float()
    c = (1.0 / length).float()
    return w, t, z, eps, c


@lru_cache(maxsize=None)
def dense_reference(shape, offset, lam):
    w, t, z, eps, c = dense_inputs(shape, offset)
    return dense(w, t, z, eps, c, *lam)


@lru_cache(maxsize=None)
def packed_inputs(offset):
    """(w, t0, t1, starts, counts, z, eps, c) for PACKED_COUNTS; an empty ray keeps a live target (its D is 0)."""
    gen = torch.Generator().manual_seed(300 + int(offset))
    w, t0, t1, starts, counts = R.packed_case(PACKED_COUNTS, offset, gen, opaque_ray=OPAQUE_RAY)
    N = len(PACKED_COUNTS)
    z, eps, c = torch.zeros(N), torch.zeros(N), torch.zeros(N)
    for r, (s, n) in enumerate(zip(starts.tolist(), counts.tolist())):
        frac = float(torch.rand(1, generator=gen))
        if n == 0:
            z[r], eps[r], c[r] = offset + 10.0 + 30.0 * frac, 1.0, 1.0 / 50.0
            continue
        kidx = s + int(torch.randint(n // 4, max(3 * n // 4, n // 4 + 1), (1,), generator=gen))
        z[r] = t0[kidx] + frac * (t1[kidx] - t0[kidx])
        length = t1[s + n - 1] - t0[s]
        eps[r] = 1.5 * length / max(n - 1, 1)
        c[r] = 1.0 / length
    return w, t0, t1, starts, counts, z, eps, c


@lru_cache(maxsize=None)
def packed_reference(offset, lam):
    w, t0, t1, starts, counts, z, eps, c = packed_inputs(offset)
    return packed(w, t0, t1, starts, counts, z, eps, c, *lam)


SPECIAL = ("no_target", "zero_scale_nan_t", "window_before", "window_beyond", "narrow_window", "opaque_first")
NARROW_J = 7   # the interval the narrow window lies in


@lru_cache(maxsize=None)
def special_rays():
    """(w, t, z, eps, c) of six (S = 16) rays, in the order of SPECIAL:
    z = NaN; c = 0 with NaN t; the window wholly before the first sample; the window beyond the last interval; a
    window inside interval NARROW_J alone; the opaque-first ray."""
    gen = torch.Generator().manual_seed(77)
    n, S = len(SPECIAL), 16
    w, t = R.dense_case(n, S, 100.0, gen, opaque_ray=SPECIAL.index("opaque_first"))
    w = w.clone()
    w[SPECIAL.index("narrow_window"), NARROW_J] = 0.25      # a weight of its own against k = Phi(3) - Phi(-3)
    t = t.clone()
    d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1)
    z = (t[:, S // 2] + 0.5 * d[:, S // 2]).float()
    eps = (1.5 * (t[:, -1] - t[:, 0]) / (S - 1)).float()
    c = (1.0 / (t[:, -1] - t[:, 0])).float()
    z[0] = float("nan")
    c[1] = 0.0
    t[1] = float("nan")
    z[2], eps[2] = 50.0, 10.0                                # hi = 60 < t_0 >= 102
    z[3], eps[3] = t[3, -1] + d[3, -1] + 2.0, 1.0            # lo beyond the last interval's end
    z[4] = t[4, NARROW_J] + 0.5 * d[4, NARROW_J]
    eps[4] = 0.125 * d[4, NARROW_J]
    return w, t, z, eps, c
