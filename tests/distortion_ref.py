"""The distortion loss by its O(S^2) definition in float64, the reference of tests/test_distortion_*.py:

    L       = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i
    dL/dw_i = 2 sum_j w_j |m_i - m_j| + 2/3 w_i d_i

per ray, for packed samples [t0_i, t1_i] (m = (t0 + t1) / 2, d = t1 - t0) and for the dense (N, S) layout with the
compositing's own intervals (s_i = t_i, d_i = volume_render's ``dists``, m_i = s_i + d_i / 2).  The inputs are taken as
they are (fp32 values widened exactly); nothing here is shared with the package's code.  Also the test inputs: weights
from real compositing of a sparse density, so that many are exactly 0."""
import torch


def ray_loss(w, m, d):
    """(L, dL/dw) of one ray: float64 (S,) weights (may require grad), midpoints and widths."""
    a = (m[:, None] - m[None, :]).abs()
    loss = (w[:, None] * w[None, :] * a).sum() + (w * w * d).sum() / 3.0
    grad = 2.0 * (w[None, :] * a).sum(1) + 2.0 * w * d / 3.0
    return loss, grad


def dense_intervals(t_vals):
    """float64 (m, d) of (N, S) t values: dists in the precision of t (ray_rendering.py:187-188), widened."""
    d = (t_vals[:, 1:] - t_vals[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1).double()
    return t_vals.double() + 0.5 * d, d


def dense(weights, t_vals, ray_scale=None):
    """(loss (N,), grad (N, S)) float64."""
    m, d = dense_intervals(t_vals)
    w = weights.detach().double()
    N, S = w.shape
    loss, grad = torch.zeros(N, dtype=torch.float64), torch.zeros(N, S, dtype=torch.float64)
    for r in range(N):
        if ray_scale is not None and float(ray_scale[r]) == 0.0:
            continue
        loss[r], grad[r] = ray_loss(w[r], m[r], d[r])
        if ray_scale is not None:
            loss[r] *= float(ray_scale[r])
            grad[r] *= float(ray_scale[r])
    return loss, grad


def packed(weights, t0, t1, starts, counts, ray_scale=None):
    """(loss (N,), grad (M,)) float64."""
    w, a, b = weights.detach().double(), t0.double(), t1.double()
    N = starts.numel()
    loss, grad = torch.zeros(N, dtype=torch.float64), torch.zeros_like(w)
    for r in range(N):
        s, c = int(starts[r]), int(counts[r])
        if c == 0 or (ray_scale is not None and float(ray_scale[r]) == 0.0):
            continue
        sl = slice(s, s + c)
        loss[r], grad[sl] = ray_loss(w[sl], 0.5 * (a[sl] + b[sl]), b[sl] - a[sl])
        if ray_scale is not None:
            loss[r] *= float(ray_scale[r])
            grad[sl] *= float(ray_scale[r])
    return loss, grad


def composite(sigma, dt):
    """Front-to-back weights alpha_i T_i of one ray's densities and step lengths (fp32 in, fp32 out)."""
    alpha = 1.0 - torch.exp(-sigma.double() * dt.double())
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha]), 0)[:-1]
    return (alpha * T).float()


def sparse_sigma(n, gen, keep=0.3, opaque_first=False):
    """n densities of which about 1 - keep are exactly 0; opaque_first: the first sample absorbs everything."""
    sig = torch.rand(n, generator=gen) * 4.0 * (torch.rand(n, generator=gen) < keep)
    if opaque_first and n:
        sig[0] = 1e6
    return sig


def packed_case(counts, offset, gen, opaque_ray=None):
    """Packed fp32 samples of len(counts) rays: sorted boundaries in [offset, offset + 50), weights composited from a
    sparse density.  Returns (w, t0, t1, starts, counts)."""
    counts = torch.as_tensor(counts, dtype=torch.long)
    starts = torch.cumsum(counts, 0) - counts
    ws, t0s, t1s = [], [], []
    for r, c in enumerate(counts.tolist()):
        t = (torch.sort(torch.rand(c + 1, generator=gen) * 50.0).values + offset).float()
        t0, t1 = t[:-1], t[1:]
        ws.append(composite(sparse_sigma(c, gen, opaque_first=(r == opaque_ray)), t1 - t0))
        t0s.append(t0)
        t1s.append(t1)
    return torch.cat(ws), torch.cat(t0s), torch.cat(t1s), starts, counts


def dense_case(N, S, offset, gen, opaque_ray=0):
    """(weights, t_vals) fp32 (N, S): jittered depths in [offset + 2, offset + 2 + len) per ray, weights composited
    over volume_render's dists from a sparse density."""
    near = offset + 2.0 + torch.rand(N, generator=gen)
    length = 5.0 + 45.0 * torch.rand(N, generator=gen)
    u = (torch.arange(S).float()[None, :] + torch.rand(N, S, generator=gen)) / S
    t = (near[:, None] + length[:, None] * u).float()
    d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    d = torch.cat([d, d[:, -1:]], dim=1)
    w = torch.stack([composite(sparse_sigma(S, gen, opaque_first=(r == opaque_ray)), d[r]) for r in range(N)])
    return w, t
