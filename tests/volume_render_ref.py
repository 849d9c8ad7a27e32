"""volume_render by its formula in float64 (ray_rendering.py:137-165), the reference of tests/test_volume_render_*.py,
and the inputs those tests composite.  Nothing here is shared with the package's code.

    rgb    = clamp(c, 0, 1)                 or sigmoid(c)
    sigma  = clamp_min(s, 0) * sigma_scale  or exp(clamp(s, -88.722839111, 88.722839111)) * sigma_scale
    dist_i = max(t_{i+1} - t_i, 1e-4),  dist_{S-1} = dist_{S-2}
    alpha  = clamp(1 - exp(-sigma dist), 0, 1 - 1e-7)
    x_i    = 1 - alpha_i + 1e-10,  T_i = prod_{k<i} x_k,  w_i = alpha_i T_i
    rgb_map = sum w c (+ (1 - acc) bg),  depth = sum w t,  acc = sum w

``forward`` is that in torch (gradients: float64 autograd of it); ``forward_analytic`` / ``backward_analytic`` are the
same and its hand-derived backward in numpy (the comment above vr_bwd_ray, csrc/render.hip):

    g_k = G_rgb.(c_k - bg) + G_depth t_k + G_acc + G_w,k                       (= dL/dw_k)
    dL/dalpha_i = g_i T_i - (sum_{k>i} g_k w_k) / x_i
    dL/dsigma_i = [0 <= a_i <= 1 - 1e-7] dL/dalpha_i dist_i exp(-sigma_i dist_i) sigma_scale [s_i >= 0]
    dL/dc_i     = [0 <= c_i <= 1] w_i G_rgb,   dL/dbg = (1 - acc) G_rgb

(the masks pass the gradient at exactly the bounds, as torch's clamp does).  ``mutate`` plants one mistake into the
analytic pair; tests/test_volume_render_cpu.py shows that each would be seen at >= 100 times the GPU tolerances."""
import numpy as np
import torch

EXP_MAX_F32 = 88.722839111      # trunc_exp's clamp for fp32 inputs (models/trunc_exp.py)
ALPHA_MAX = 1.0 - 1e-7

# every (N, S) the tests composite: below, at and above one and two 32-sample tiles, S = 2, many carries
SHAPES = [(1, 2), (5, 3), (37, 31), (36, 32), (37, 33), (13, 63), (12, 64), (13, 65), (7, 257), (6, 1025)]
KINDS = ("thin", "late", "saturated", "empty", "golden", "degenerate")
THIN_MIN_T = 0.1                # every thin row ends with at least this transmittance
LATE_MIN_W = 0.25               # every late row has at least this weight on its last two samples

MUTATIONS = ("last_dist", "tile_carry", "dist_clamp", "suffix_inclusive", "clamp_masks", "g_weights", "g_bg_acc")


def _d(x):
    return None if x is None else (x if x.dtype == torch.float64 else x.double())


def forward(rgb_sigma, t_vals, bg=None, raw_rgb=False, raw_sigma=False, sigma_scale=1.0):
    """(rgb (N,3), depth (N,), weights (N,S), acc (N,)) float64; differentiable in rgb_sigma and bg."""
    rs, t, bg = _d(rgb_sigma), _d(t_vals), _d(bg)
    c = torch.sigmoid(rs[..., :3]) if raw_rgb else rs[..., :3].clamp(0.0, 1.0)
    sigma = torch.exp(rs[..., 3].clamp(-EXP_MAX_F32, EXP_MAX_F32)) if raw_sigma else rs[..., 3].clamp_min(0.0)
    sigma = sigma * float(sigma_scale)
    dists = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    dists = torch.cat([dists, dists[:, -1:]], dim=1)
    alpha = (1.0 - torch.exp(-sigma * dists)).clamp(0.0, ALPHA_MAX)
    x = 1.0 - alpha + 1e-10
    T = torch.cat([torch.ones_like(x[:, :1]), torch.cumprod(x, dim=1)[:, :-1]], dim=1)
    w = alpha * T
    acc = w.sum(1)
    rgb = (w[..., None] * c).sum(1)
    if bg is not None:
        rgb = rgb + (1.0 - acc)[:, None] * bg
    return rgb, (w * t).sum(1), w, acc


def autograd(rgb_sigma, t_vals, bg, raw_rgb, raw_sigma, sigma_scale, grads):
    """(outputs, g_rgb_sigma, g_bg) float64 numpy: float64 autograd of ``forward`` for the output gradients ``grads`` =
    (g_rgb, g_depth, g_weights, g_acc), each a tensor or None (= not used by the loss)."""
    rs = _d(rgb_sigma).detach().clone().requires_grad_(True)
    b = None if bg is None else _d(bg).detach().clone().requires_grad_(True)
    out = forward(rs, t_vals, b, raw_rgb, raw_sigma, sigma_scale)
    loss = sum((o * _d(g)).sum() for o, g in zip(out, grads) if g is not None)
    loss.backward()
    return (tuple(o.detach().numpy() for o in out), rs.grad.numpy(),
            None if b is None else (b.grad.numpy() if b.grad is not None else np.zeros(tuple(b.shape))))


def _np(x):
    return None if x is None else np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)


def _composite_np(rs, t, sigma_scale, mutate):
    """The forward's intermediates in numpy float64 (raw flags off)."""
    N, S = t.shape
    c = np.clip(rs[..., :3], 0.0, 1.0)
    s_in = rs[..., 3]
    sigma = np.maximum(s_in, 0.0) * float(sigma_scale)
    dists = t[:, 1:] - t[:, :-1]
    if mutate != "dist_clamp":
        dists = np.maximum(dists, 1e-4)
    last = np.full((N, 1), 1e-4) if mutate == "last_dist" else dists[:, -1:]
    dists = np.concatenate([dists, last], axis=1)
    e = np.exp(-sigma * dists)
    a = 1.0 - e
    alpha = np.clip(a, 0.0, ALPHA_MAX)
    x = 1.0 - alpha + 1e-10
    T = np.ones((N, S))
    for i in range(1, S):
        restart = mutate == "tile_carry" and i % 32 == 0
        T[:, i] = 1.0 if restart else T[:, i - 1] * x[:, i - 1]
    return c, s_in, dists, e, a, alpha, x, T, alpha * T


def forward_analytic(rgb_sigma, t_vals, bg=None, sigma_scale=1.0, mutate=None):
    """(rgb, depth, weights, acc) float64 numpy, raw flags off."""
    assert mutate is None or mutate in MUTATIONS
    rs, t, bg = _np(rgb_sigma), _np(t_vals), _np(bg)
    c, _, _, _, _, _, _, _, w = _composite_np(rs, t, sigma_scale, mutate)
    acc = w.sum(1)
    rgb = (w[..., None] * c).sum(1)
    if bg is not None:
        rgb = rgb + (1.0 - acc)[:, None] * bg
    return rgb, (w * t).sum(1), w, acc


def backward_analytic(rgb_sigma, t_vals, bg, sigma_scale, g_rgb, g_depth, g_weights, g_acc, mutate=None):
    """(g_rgb_sigma (N,S,4), g_bg (N,3) or None) float64 numpy, raw flags off; a missing output gradient is zero."""
    assert mutate is None or mutate in MUTATIONS
    rs, t, bg = _np(rgb_sigma), _np(t_vals), _np(bg)
    N, S = t.shape
    G_rgb = np.zeros((N, 3)) if g_rgb is None else _np(g_rgb)
    G_d = np.zeros(N) if g_depth is None else _np(g_depth)
    G_a = np.zeros(N) if g_acc is None else _np(g_acc)
    G_w = np.zeros((N, S)) if (g_weights is None or mutate == "g_weights") else _np(g_weights)
    c, s_in, dists, e, a, alpha, x, T, w = _composite_np(rs, t, sigma_scale, mutate)
    b = np.zeros((N, 3)) if bg is None else bg
    g = ((c - b[:, None, :]) * G_rgb[:, None, :]).sum(-1) + G_d[:, None] * t + G_a[:, None] + G_w
    gw = g * w
    incl = np.cumsum(gw[:, ::-1], axis=1)[:, ::-1]          # sum_{k >= i} g_k w_k
    suffix = incl if mutate == "suffix_inclusive" else np.concatenate([incl[:, 1:], np.zeros((N, 1))], axis=1)
    dalpha = g * T - suffix / x
    masks = mutate != "clamp_masks"
    m_alpha = ((a >= 0.0) & (a <= ALPHA_MAX)) if masks else True
    m_sigma = (s_in >= 0.0) if masks else True
    m_rgb = ((rs[..., :3] >= 0.0) & (rs[..., :3] <= 1.0)) if masks else True
    g_rs = np.empty((N, S, 4))
    g_rs[..., :3] = np.where(m_rgb, w[..., None] * G_rgb[:, None, :], 0.0)
    g_rs[..., 3] = np.where(m_sigma, np.where(m_alpha, dalpha * dists * e, 0.0) * float(sigma_scale), 0.0)
    if bg is None:
        return g_rs, None
    om = np.ones(N) if mutate == "g_bg_acc" else 1.0 - w.sum(1)
    return g_rs, om[:, None] * G_rgb


# ------------------------------------------------------------------------------------------ inputs
def kinds(N):
    return torch.arange(N) % 6


def _gen(N, S, seed, salt):
    return torch.Generator().manual_seed(1_000_003 * int(seed) + 7919 * int(S) + 31 * int(N) + salt)


def _dists32(t):
    d = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    return torch.cat([d, d[:, -1:]], dim=1)


def check_rows(rgb_sigma, t_vals, raw_sigma=False):
    """The two conditions the row kinds exist for, on the float64 reference: every thin row (kind 0) keeps a
    transmittance >= THIN_MIN_T behind its last sample, so that every sample of every tile carries weight, and every
    late row (kind 1) puts >= LATE_MIN_W of weight on its last two samples, so that the tail tile and the last dist
    carry the result.  Returns (smallest thin transmittance, smallest late weight)."""
    N, S = t_vals.shape
    k = kinds(N)
    _, _, w, acc = forward(rgb_sigma, t_vals, None, False, raw_sigma, 1.0)
    # 1 - acc telescopes to prod x_i up to the 1e-10 terms
    thin_T = float((1.0 - acc[k == 0]).min()) if bool((k == 0).any()) else float("inf")
    late_w = float(w[k == 1][:, -2:].sum(1).min()) if bool((k == 1).any()) else float("inf")
    assert thin_T >= THIN_MIN_T, f"rows({N}, {S}): a thin row ends with transmittance {thin_T}"
    assert late_w >= LATE_MIN_W, f"rows({N}, {S}): a late row has {late_w} of weight on its last two samples"
    return thin_T, late_w


def rows(N, S, seed=0):
    """Deterministic fp32 (rgb_sigma (N,S,4), t_vals (N,S)); ray n has kind n % 6 (KINDS):

    0 thin        total optical depth U(0.2, 1.8) spread over all S samples
    1 late        sigma 1e-3, 150 on the last two samples
    2 saturated   sigma 1e5
    3 empty       sigma 0
    4 golden      the golden fixture's exp(U 14 - 7) - 0.01 (some sigma < 0)
    5 degenerate  depths: rows 5, 17, .. all t equal; rows 11, 23, .. one descending pair and a last step of 1e-6

    rgb is U(-0.2, 1.2), steps are U(1e-3, 1.1e-2); rgb_sigma[0, 0, :3] = (0, 1, 0.5) and rgb_sigma[0, 1, 3] = 0 sit
    exactly on the clamps' bounds.  check_rows() holds for the result."""
    assert N >= 1 and S >= 2
    g = _gen(N, S, seed, 0)
    k = kinds(N)
    rgb = torch.rand(N, S, 3, generator=g) * 1.4 - 0.2
    near = torch.rand(N, 1, generator=g) * 0.1
    steps = torch.rand(N, S, generator=g) * 1e-2 + 1e-3
    u_sig = torch.rand(N, S, generator=g)
    tau = torch.rand(N, 1, generator=g) * 1.6 + 0.2
    steps[:, 0] = 0.0
    flat = (k == 5) & ((torch.arange(N) // 6) % 2 == 0)
    bent = (k == 5) & ~flat
    steps[flat] = 0.0
    steps[bent, 1 + (S - 2) // 3] = -2e-3
    steps[bent, S - 1] = 1e-6
    t = (near + torch.cumsum(steps, 1)).float()
    d = _dists32(t).double()
    sig = torch.zeros(N, S, dtype=torch.float64)
    shape = u_sig.double() + 0.5
    sig[k == 0] = (tau.double() * shape / (shape * d).sum(1, keepdim=True))[k == 0]
    sig[k == 1] = 1e-3
    sig[k == 1, -2:] = 150.0
    sig[k == 2] = 1e5
    sig[k == 4] = (torch.exp(u_sig.double() * 14.0 - 7.0) - 0.01)[k == 4]
    sig[k == 5] = (100.0 + 1900.0 * u_sig.double())[k == 5]
    rs = torch.cat([rgb, sig.float()[..., None]], -1)
    rs[0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    rs[0, 1, 3] = 0.0
    check_rows(rs, t)
    return rs, t


def raw_inputs(rgb_sigma, t_vals, raw_rgb, raw_sigma):
    """What the raw-flag cases feed: a channel its flag covers is ``x * 3 - 1`` as in the golden's ``b:`` case, except
    sigma on thin and late rows, which becomes log(sigma) so that exp() keeps the row's optical depth (log(0) = -inf
    meets the lower clamp).  check_rows() is asserted again for raw sigma."""
    x = rgb_sigma.clone()
    if raw_rgb:
        x[..., :3] = rgb_sigma[..., :3] * 3.0 - 1.0
    if raw_sigma:
        k = kinds(x.shape[0])
        keep = (k == 0) | (k == 1)
        sig = rgb_sigma[..., 3]
        x[..., 3] = torch.where(keep[:, None], torch.log(sig.double()).float(), sig * 3.0 - 1.0)
        check_rows(x, t_vals, raw_sigma=True)
    return x


def extras(N, S, seed=0):
    """fp32 (bg (N,3), (g_rgb (N,3), g_depth (N,), g_weights (N,S), g_acc (N,))) for rows(N, S, seed)."""
    g = _gen(N, S, seed, 1)
    bg = torch.rand(N, 3, generator=g)
    return bg, (torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, S, generator=g) * 0.1,
                torch.randn(N, generator=g))


GRAD_SUBSETS = {"rgb": (0,), "depth": (1,), "weights": (2,), "acc": (3,), "all": (0, 1, 2, 3)}


def subset(grads, name):
    """``grads`` with the output gradients outside the subset replaced by None."""
    return tuple(g if i in GRAD_SUBSETS[name] else None for i, g in enumerate(grads))


# ------------------------------------------------------------------------------------------ tolerances
# the project's: README parity contract / tests/test_render_depths_gpu.py (forward), tests/test_train.py (gradients)
TOL_RGB = TOL_ACC = 1e-4
TOL_W = 1e-5
TOL_DEPTH = 1e-4        # times max|t|
TOL_GRAD = 2e-5         # times the reference channel's max
BG_RTOL, BG_ATOL = 1e-5, 1e-6


def forward_errors(got, ref, t_vals):
    """Each output's max|got - ref| over its tolerance, in (rgb, depth, weights, acc) order; <= 1 passes."""
    tmax = float(np.abs(_np(t_vals)).max())
    tol = (TOL_RGB, TOL_DEPTH * tmax, TOL_W, TOL_ACC)
    return tuple(float(np.abs(_np(a) - _np(b)).max()) / s if _np(b).size else 0.0 for a, b, s in zip(got, ref, tol))


def grad_errors(got, ref):
    """Per channel of g_rgb_sigma, max|got - ref| over TOL_GRAD * max|ref channel| (+ 1e-12, as test_train.py)."""
    got, ref = _np(got), _np(ref)
    return tuple(float(np.abs(got[..., c] - ref[..., c]).max())
                 / (TOL_GRAD * (float(np.abs(ref[..., c]).max()) + 1e-12)) for c in range(4))


def bg_error(got, ref):
    """max of |got - ref| / (BG_ATOL + BG_RTOL |ref|); <= 1 passes."""
    got, ref = _np(got), _np(ref)
    return float((np.abs(got - ref) / (BG_ATOL + BG_RTOL * np.abs(ref))).max())
