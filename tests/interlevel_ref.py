"""Float64 numpy reference of the interlevel ("proposal") loss and the cases its tests share.

For a row of S >= 2 non-decreasing fp32 depths t the interval edges are e_i = t_i (i < S) and
e_S = t_{S-1} + (t_{S-1} - t_{S-2}), in float64.  With a = E(t_fine), p = E(t_prop):

    O(i,k)  = (p_{k+1} > a_i) and (p_k < a_{i+1})
    bound_i = sum_k O(i,k) w_prop_k,  x_i = max(0, w_i - bound_i)
    loss    = sum_i x_i^2 / (w_i + eps),  d loss / d w_prop_k = -sum_i O(i,k) 2 x_i / (w_i + eps)

``definition`` evaluates exactly that, O(S P) per ray.  ``prefix_form`` is the O(S + P) form through prefix differences;
it is used only to size the tests' floor: the two differ by float64 summation order alone, and four times their
difference (per case) is what the tests allow on top of the output's own fp32 rounding."""
from functools import lru_cache

import numpy as np
import torch

EPS = 2.0 ** -23
OFFSETS = (0.0, 100.0, 5000.0)
REL = 4.0 * 2.0 ** -24          # the output's one fp32 rounding, with margin (the convention of §4t and §4y)


def edges(t):
    t = np.asarray(t, dtype=np.float64)
    return np.concatenate([t, t[..., -1:] + (t[..., -1:] - t[..., -2:-1])], axis=-1)


def overlap(t_fine_row, t_prop_row):
    """(S, P) bool O(i, k) of one ray."""
    a, p = edges(t_fine_row), edges(t_prop_row)
    return (p[None, 1:] > a[:-1, None]) & (p[None, :-1] < a[1:, None])


def definition(t_fine, w_fine, t_prop, w_prop, eps=EPS):
    """(loss (N,), grad (N, P), x (N, S)) by the O(S P) definition, float64."""
    N, S = t_fine.shape
    P = t_prop.shape[1]
    loss, grad, xs = np.zeros(N), np.zeros((N, P)), np.zeros((N, S))
    for n in range(N):
        O = overlap(t_fine[n], t_prop[n])
        w, wp = w_fine[n].astype(np.float64), w_prop[n].astype(np.float64)
        bound = (O * wp[None, :]).sum(1)
        x = np.maximum(0.0, w - bound)
        loss[n] = (x * x / (w + eps)).sum()
        grad[n] = -(O * (2.0 * x / (w + eps))[:, None]).sum(0)
        xs[n] = x
    return loss, grad, xs


def prefix_form(t_fine, w_fine, t_prop, w_prop, eps=EPS):
    """(loss, grad) through the exclusive prefix sums of w_prop and of 2 x / (w + eps)."""
    N, S = t_fine.shape
    P = t_prop.shape[1]
    loss, grad = np.zeros(N), np.zeros((N, P))
    for n in range(N):
        a, p = edges(t_fine[n]), edges(t_prop[n])
        w, wp = w_fine[n].astype(np.float64), w_prop[n].astype(np.float64)
        lo = np.maximum(np.searchsorted(p, a[:-1], side="right") - 1, 0)
        hi = np.maximum(np.minimum(np.searchsorted(p, a[1:], side="left"), P), lo)
        c = np.concatenate([[0.0], np.cumsum(wp)])
        x = np.maximum(0.0, w - (c[hi] - c[lo]))
        loss[n] = (x * x / (w + eps)).sum()
        R = np.concatenate([[0.0], np.cumsum(2.0 * x / (w + eps))])
        n_lo = np.searchsorted(a[:-1], p[1:], side="left")      # #{i : a_i < p_{k+1}}
        n_hi = np.searchsorted(a[1:], p[:-1], side="right")     # #{i : a_{i+1} <= p_k}
        grad[n] = -(R[np.maximum(n_lo, n_hi)] - R[n_hi])
    return loss, grad


def composite(sigma, t):
    """fp32 compositing weights of densities over the rows' own intervals (float64 arithmetic)."""
    e = edges(t)
    tau = sigma.astype(np.float64) * (e[..., 1:] - e[..., :-1])
    T = np.exp(-(np.cumsum(tau, -1) - tau))
    return (T * (1.0 - np.exp(-tau))).astype(np.float32)


def _depths(rng, n, s, offset):
    return (offset + 4.0 * np.sort(rng.random((n, s)), axis=1)).astype(np.float32)


def _sparse_sigma(rng, n, s, keep, depth=3.0):
    """Densities that are exactly 0 at a share 1 - keep of the samples and add up to an optical depth of about
    ``depth`` over the row's span of 4: the weights are spread over the whole ray at every row length."""
    return np.where(rng.random((n, s)) < keep, rng.exponential(1.0, (n, s)) * depth / (4.0 * keep), 0.0)


def dominate(t_fine_row, w_fine_row, t_prop_row):
    """(w_fine_row', w_prop_row) with bound_i >= 2 w_i for every i: each proposal interval takes twice the weight of
    all fine intervals it overlaps (rounded up to fp32), and a fine interval that overlaps none gets weight 0."""
    O = overlap(t_fine_row, t_prop_row)
    w = np.where(O.any(1), w_fine_row, np.float32(0.0)).astype(np.float32)
    wp = (2.0 * (O * w.astype(np.float64)[:, None]).sum(0)).astype(np.float32)
    wp = np.where(wp > 0, np.nextafter(wp, np.float32(np.inf)), wp).astype(np.float32)
    return w, wp


@lru_cache(maxsize=None)
def case(N, S, P, offset, seed=0):
    """fp32 inputs (torch, CPU), the float64 reference and the floor of one case; computed once, never modified.

    Depths are sorted uniforms shifted by ``offset``; weights are composited from a sparse random density, so a good
    share are exactly 0.  With N >= 4 the first rows are special (``rows``): ties (the fine row copies proposal
    depths), a run of equal neighbours in both rows, a row with all depths equal, an opaque one-hot fine ray, a ray of
    all-zero proposal weights and a dominated ray (bound_i >= 2 w_i for every i); with 4 <= N < 7 they share four
    rows."""
    rng = np.random.default_rng(1000 * S + P + 7 * N + int(offset) + seed)
    tf, tp = _depths(rng, N, S, offset), _depths(rng, N, P, offset)
    rows = {}
    if N >= 4:
        names = ("ties", "equal", "flat", "onehot", "zero_prop", "dominated")
        rows = dict(zip(names, range(6))) if N >= 7 else dict(ties=0, equal=0, flat=1, onehot=2, zero_prop=2,
                                                              dominated=3)
        m = min(S, P)
        tf[rows["ties"]] = np.sort(np.concatenate([tp[rows["ties"], :m], tf[rows["ties"], m:]]))
        e = rows["equal"]
        if S >= 4:
            tf[e, 2] = tf[e, 1]
            tf[e, S // 2:S // 2 + 2] = tf[e, S // 2]
        else:
            tf[e, 1] = tf[e, 0]
        if P >= 4:
            tp[e, 2] = tp[e, 1]
        else:
            tp[e, 1] = tp[e, 0]
        tf[e], tp[e] = np.sort(tf[e]), np.sort(tp[e])
        tf[rows["flat"]] = tp[rows["flat"], P // 2]
    wf = composite(_sparse_sigma(rng, N, S, 0.35), tf)
    wp = composite(_sparse_sigma(rng, N, P, 0.5), tp)
    if N >= 4:
        if rows["flat"] != rows["equal"]:
            wf[rows["flat"]] = (rng.random(S) * (rng.random(S) < 0.5) / S).astype(np.float32)   # zero widths: any w
        wf[rows["onehot"]] = 0.0
        wf[rows["onehot"], S // 2] = 1.0
        wp[rows["zero_prop"]] = 0.0
        d = rows["dominated"]
        wf[d], wp[d] = dominate(tf[d], wf[d], tp[d])
    loss, grad, x = definition(tf, wf, tp, wp)
    loss2, grad2 = prefix_form(tf, wf, tp, wp)
    if S >= 33:      # both branches of the max carry weight
        pos = wf > 0
        share = float(((x > 0) & pos).sum()) / float(pos.sum())
        assert 0.15 <= share <= 0.9, (N, S, P, offset, share)
    if rows:
        d = rows["dominated"]
        assert float(x[d].max()) == 0.0 and float(loss[d]) == 0.0 and not grad[d].any()
        O = overlap(tf[d], tp[d])
        assert bool(((O * wp[d].astype(np.float64)[None]).sum(1) >= 2.0 * wf[d]).all())
    return dict(t_fine=torch.from_numpy(tf), w_fine=torch.from_numpy(wf), t_prop=torch.from_numpy(tp),
                w_prop=torch.from_numpy(wp), loss=loss, grad=grad, x=x, rows=rows,
                floor_loss=4.0 * float(np.abs(loss - loss2).max()) + 1e-30,
                floor_grad=4.0 * float(np.abs(grad - grad2).max()) + 1e-30)


def ratios(case_, loss, grad):
    """Worst ratio of |got - ref| to REL * (largest |ref| of that ray) + floor, for the loss and for the gradient."""
    ref_l, ref_g = case_["loss"], case_["grad"]
    rl = np.abs(np.asarray(loss, dtype=np.float64) - ref_l) / (REL * np.abs(ref_l) + case_["floor_loss"])
    out = [float(rl.max())]
    if grad is not None:
        gmax = np.abs(ref_g).max(1, keepdims=True)
        rg = np.abs(np.asarray(grad, dtype=np.float64) - ref_g) / (REL * gmax + case_["floor_grad"])
        out.append(float(rg.max()))
    return out
