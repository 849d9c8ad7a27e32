"""Float64 reference of the expert MLP (MetaNGP.forward, as tests/test_amp.py::torch_chain restates it) with a
hand-written backward, its pair-list form, the routed slot layout and the backward kernels' index arithmetic.

Plain numpy, no autograd, nothing from the package: tests/test_mlp_pairs_cpu.py holds this module to torch.autograd
in float64, tests/test_mlp_pairs_gpu.py holds the pair-list kernels of csrc/mlp_train.hip to it.

    a1 = relu(W0 h0 + b0)         a2 = relu(W1 a1 + b1)
    sigma = exp(clamp(Wsh a2 + bsh, +-88.722839111))      (trunc_exp.py; backward d sigma / d s = sigma, clamped or not)
    geo = Wg a2 + bg              cin = [geo | sh]
    c1 = relu(Wc0 cin + bc0)      c2 = relu(Wc1 c1 + bc1)     rgb = sigmoid(Wc2 c2 + bc2)
    out = [rgb, sigma]
"""
import numpy as np

WNAMES = ("w0", "b0", "w1", "b1", "wsh", "bsh", "wg", "bg", "wc0", "bc0", "wc1", "bc1", "wc2", "bc2")
MLP_DW_SHAPES = ((64, 32), (64,), (64, 64), (64,), (1, 64), (1,), (15, 64), (15,), (64, 31), (64,), (64, 64), (64,),
                 (3, 64), (3,))                                  # ops.MLP_DW_SHAPES (asserted equal by the GPU tests)
MLP_DW_FLOATS = int(sum(np.prod(s) for s in MLP_DW_SHAPES))     # 13715
CLAMP = float(np.float32(88.722839111))                          # trunc_exp.py's fp32 limit
ROUND = 128                                                      # slots per round: 4 tiles of 32 rows, one expert
PAIR_DW_BLOCKS = 256                                             # workgroups (partial copies) of the pair-list backward
FWD_GRID = 512                                                   # workgroups of the pair-list forward


def make_weights(seed, scale=0.4):
    """The 14 float32 tensors of one expert, uniform in +-scale / 2 (test_amp._weights' distribution)."""
    g = np.random.default_rng(seed)
    return [((g.random(s) - 0.5) * scale).astype(np.float32) for s in MLP_DW_SHAPES]


def forward(h0, sh, ws):
    """out (n, 4) = [rgb, sigma] and the activations the backward needs, all float64."""
    w = {n: np.asarray(t, np.float64) for n, t in zip(WNAMES, ws)}
    h0, sh = np.asarray(h0, np.float64), np.asarray(sh, np.float64)
    a1 = np.maximum(h0 @ w["w0"].T + w["b0"], 0.0)
    a2 = np.maximum(a1 @ w["w1"].T + w["b1"], 0.0)
    sigma = np.exp(np.clip(a2 @ w["wsh"].T + w["bsh"], -CLAMP, CLAMP))
    cin = np.concatenate([a2 @ w["wg"].T + w["bg"], sh], -1)
    c1 = np.maximum(cin @ w["wc0"].T + w["bc0"], 0.0)
    c2 = np.maximum(c1 @ w["wc1"].T + w["bc1"], 0.0)
    rgb = 0.5 * (1.0 + np.tanh(0.5 * (c2 @ w["wc2"].T + w["bc2"])))      # sigmoid, without exp's overflow
    return np.concatenate([rgb, sigma], -1), dict(w=w, h0=h0, a1=a1, a2=a2, cin=cin, c1=c1, c2=c2)


def backward(h0, sh, gout, ws, factors=None):
    """(out, the 14 [dW | db] in MLP_DW_SHAPES order, dL/dh0 (n, 32), dL/dsh (n, 16)) for dL/dout = gout.  A list
    passed as ``factors`` receives, per tensor, the (dY, X) whose product over the rows it is (X None for a bias)."""
    out, s = forward(h0, sh, ws)
    fac = []
    w, g = s["w"], np.asarray(gout, np.float64)
    rgb = out[:, :3]
    dz = g[:, :3] * rgb * (1.0 - rgb)
    d_wc2, d_bc2 = dz.T @ s["c2"], dz.sum(0)
    fac += [(dz, s["c2"]), (dz, None)]
    dz = (dz @ w["wc2"]) * (s["c2"] > 0)
    d_wc1, d_bc1 = dz.T @ s["c1"], dz.sum(0)
    fac += [(dz, s["c1"]), (dz, None)]
    dz = (dz @ w["wc1"]) * (s["c1"] > 0)
    d_wc0, d_bc0 = dz.T @ s["cin"], dz.sum(0)
    fac += [(dz, s["cin"]), (dz, None)]
    dcin = dz @ w["wc0"]
    dgeo, dsh = dcin[:, :15], dcin[:, 15:]
    ds = g[:, 3:4] * out[:, 3:4]                    # TruncExp: grad * exp(clamped input), no clamp mask
    d_wsh, d_bsh = ds.T @ s["a2"], ds.sum(0)
    d_wg, d_bg = dgeo.T @ s["a2"], dgeo.sum(0)
    fac += [(dgeo, s["a2"]), (dgeo, None), (ds, s["a2"]), (ds, None)]
    dz = (ds @ w["wsh"] + dgeo @ w["wg"]) * (s["a2"] > 0)
    d_w1, d_b1 = dz.T @ s["a1"], dz.sum(0)
    fac += [(dz, s["a1"]), (dz, None)]
    dz = (dz @ w["w1"]) * (s["a1"] > 0)
    d_w0, d_b0 = dz.T @ s["h0"], dz.sum(0)
    fac += [(dz, s["h0"]), (dz, None)]
    if factors is not None:      # collected colour branch first: reorder to MLP_DW_SHAPES order
        factors[:] = [fac[i] for i in (12, 13, 10, 11, 8, 9, 6, 7, 4, 5, 2, 3, 0, 1)]
    grads = [d_w0, d_b0, d_w1, d_b1, d_wsh, d_bsh, d_wg, d_bg, d_wc0, d_bc0, d_wc1, d_bc1, d_wc2, d_bc2]
    assert tuple(x.shape for x in grads) == MLP_DW_SHAPES
    return out, grads, dz @ w["w0"], dsh


def flat_dw(grads):
    """The 14 tensors as the flat [dW | db] row the kernels write (row-major, MLP_DW_SHAPES order)."""
    return np.concatenate([np.asarray(x, np.float64).ravel() for x in grads])


def split_dw(row):
    """Views of one flat [dW | db] row as the 14 tensors."""
    res, o = [], 0
    for shp in MLP_DW_SHAPES:
        n = int(np.prod(shp))
        res.append(row[o:o + n].reshape(shp))
        o += n
    assert o == row.shape[0] == MLP_DW_FLOATS
    return res


def pairs_ref(h0, sh, gout, seg, weights_per_expert):
    """Rows [seg[k], seg[k+1]) through expert k: out (seg[K], 4), gh0 (seg[K], 32), dw (K, MLP_DW_FLOATS); the dw row
    of an expert without rows is zero."""
    seg = [int(x) for x in seg]
    K, n = len(seg) - 1, seg[-1]
    assert K == len(weights_per_expert)
    out, gh0, dw = np.zeros((n, 4)), np.zeros((n, 32)), np.zeros((K, MLP_DW_FLOATS))
    for k in range(K):
        a, b = seg[k], seg[k + 1]
        if b > a:
            out[a:b], grads, gh0[a:b], _ = backward(h0[a:b], sh[a:b], gout[a:b], weights_per_expert[k])
            dw[k] = flat_dw(grads)
    return out, gh0, dw


def make_pairs(rounds, live, seed, gout_scale=1e-4, pad_seed=None, gout_gain=None, gout_mean=3.0):
    """The routed slot layout (routed.hip): expert k's segment is rounds[k] * 128 slots, its first live[k] rows real,
    the rest padding with gout == 0 and finite random h0 / sh (pad_seed redraws the padding values only).  gout is an
    MSE gradient's size (test_amp._data: normal, 1e-4), times gout_gain[k] for expert k; every column has a mean
    of gout_mean / sqrt(live[k]) standard deviations, with the sign of that column's drawn sum over the expert's live
    rows.  That mean keeps the one-element dL/dbsh (and the three of dL/dbc2)
    away from cancellation: with zero-mean gradients such a sum is a single draw of a random walk around 0, and an error relative to it measures how
    close to 0 the draw fell, not the arithmetic (cancellation() and tests/test_mlp_pairs_cpu.py hold the layouts to
    that); it is small enough for one round's rows to stay visible in the sums.  Returns seg (int64, K + 1), h0 (n, 32),
    sh (n, 16), gout (n, 4) as float32 and the live-row mask (n,)."""
    K = len(rounds)
    assert len(live) == K and all(0 <= l <= r * ROUND and (l > 0) == (r > 0) for r, l in zip(rounds, live))
    seg = np.zeros(K + 1, np.int64)
    seg[1:] = np.cumsum(np.asarray(rounds, np.int64) * ROUND)
    n = int(seg[-1])
    g = np.random.default_rng(seed)
    h0 = ((g.random((n, 32)) - 0.5) * 2).astype(np.float32)
    sh = ((g.random((n, 16)) - 0.5) * 2).astype(np.float32)
    gout = g.standard_normal((n, 4))
    for k in range(K):
        drawn = gout[seg[k]:seg[k] + live[k]].sum(0)
        gout[seg[k]:seg[k + 1]] += np.where(drawn < 0, -1.0, 1.0) * gout_mean / np.sqrt(max(live[k], 1))
    gout = (gout * gout_scale).astype(np.float32)
    mask = np.zeros(n, bool)
    for k in range(K):
        mask[seg[k]:seg[k] + live[k]] = True
        if gout_gain is not None:
            gout[seg[k]:seg[k + 1]] *= np.float32(gout_gain[k])
    gp = np.random.default_rng(seed + 7919 if pad_seed is None else pad_seed)
    pad = ~mask
    h0[pad] = ((gp.random((int(pad.sum()), 32)) - 0.5) * 2).astype(np.float32)
    sh[pad] = ((gp.random((int(pad.sum()), 16)) - 0.5) * 2).astype(np.float32)
    gout[pad] = 0.0
    return seg, h0, sh, gout, mask


def cancellation(h0, sh, gout, ws):
    """Per [dW | db] tensor, |sum_r t_r| / sqrt(sum_r t_r^2) of its largest element's terms over the rows: an
    evaluation that rounds every term to relative u lands about u / this from the reference, relative to max |ref|."""
    fac = []
    _, grads, _, _ = backward(h0, sh, gout, ws, fac)
    res = []
    for g, (dy, x) in zip(grads, fac):
        idx = np.unravel_index(np.abs(g).argmax(), g.shape)
        t = dy[:, idx[0]] * (x[:, idx[1]] if x is not None else 1.0)
        assert abs(t.sum() - g[idx]) <= 1e-9 * max(abs(g[idx]), 1e-300)
        res.append(float(abs(t.sum()) / max(np.sqrt((t * t).sum()), 1e-300)))
    return res


def seg_expert(seg, K, p):
    """mlp_train.hip's seg_expert: the last expert whose segment starts at or before slot p (skips empty ones)."""
    k = 0
    while k + 1 < K and seg[k + 1] <= p:
        k += 1
    return k


def round_ranges(seg, G=PAIR_DW_BLOCKS):
    """Per backward workgroup b, its runs [(expert, first round, end round), ...] over the rounds [b R / G, (b+1) R / G)
    (mlp_bwd_dw_pairs_pc_kernel: one run per maximal stretch of one expert, one copy written per run)."""
    seg = [int(x) for x in seg]
    K, R = len(seg) - 1, seg[-1] // ROUND
    res = []
    for b in range(G):
        rd, r1, runs = b * R // G, (b + 1) * R // G, []
        while rd < r1:
            k, a = seg_expert(seg, K, rd * ROUND), rd
            while rd < r1 and seg_expert(seg, K, rd * ROUND) == k:
                rd += 1
            runs.append((k, a, rd))
        res.append(runs)
    return res


def copies_written(seg, G=PAIR_DW_BLOCKS):
    """The partial copies (b, k) the backward kernel writes."""
    return {(b, k) for b, runs in enumerate(round_ranges(seg, G)) for k, _, _ in runs}


def copies_read(seg, G=PAIR_DW_BLOCKS):
    """The partial copies (b, k) mlp_dw_reduce_pairs_kernel adds, from seg alone: its 8 thread rows start at
    bf = k0 G / R - 1 (clamped at 0, rounded down to a multiple of 8) + row, step 8, stop at the first range that
    begins at or past k1, and add a copy when the range is not empty and ends past k0."""
    seg = [int(x) for x in seg]
    K, R = len(seg) - 1, seg[-1] // ROUND
    res = set()
    for k in range(K):
        k0, k1 = seg[k] // ROUND, seg[k + 1] // ROUND
        if not k1 > k0:
            continue
        bf = (k0 * G) // R - 1 if R > 0 else 0
        for row in range(8):
            b = (max(bf, 0) & ~7) + row
            while b < G:
                lo, hi = b * R // G, (b + 1) * R // G
                if lo >= k1:
                    break
                if lo < hi and hi > k0:
                    assert (b, k) not in res
                    res.add((b, k))
                b += 8
    return res


def forward_rounds(seg, grid=FWD_GRID):
    """Per forward workgroup, the experts of the rounds it strides over (mlp_fwd_pairs_kernel)."""
    seg = [int(x) for x in seg]
    K, R = len(seg) - 1, seg[-1] // ROUND
    return [[seg_expert(seg, K, rd * ROUND) for rd in range(b, R, grid)] for b in range(grid)]


# name -> (rounds per expert, live rows per expert); what each reaches is asserted by tests/test_mlp_pairs_cpu.py
LAYOUTS = {
    "one": ([1], [1]),
    "none": ([0], [0]),
    "thin": ([1] * 16, [1 if i == 5 else (31 if i % 2 else 128) for i in range(16)]),
    "holes": ([0, 1, 0, 3, 0], [0, 128, 0, 3 * 128 - 97, 0]),
    "edge255": ([255], [255 * 128 - 97]),
    "edge256": ([256], [256 * 128]),
    "edge257": ([257], [257 * 128 - 97]),
    "cross": ([6, 201, 93], [6 * 128 - 97, 201 * 128, 93 * 128 - 33]),
    "big": ([3, 0, 1, 1, 1, 594, 0, 5], [3 * 128 - 97, 0, 128, 1, 128 - 97, 594 * 128 - 97, 0, 5 * 128]),
}
# (workgroups with an empty range, most distinct experts in one range, an expert strictly inside one range)
LAYOUT_FACTS = {
    "one": (255, 1, False), "none": (256, 0, False), "thin": (240, 1, False), "holes": (252, 1, False),
    "edge255": (1, 1, False), "edge256": (0, 1, False), "edge257": (0, 1, False), "cross": (0, 2, False),
    "big": (0, 3, True),
}
TOL_FLOOR = {"fp16x3": 2e-5, "fp32": 2e-5, "amp": 1e-3}
# per layout, a gain on the output gradients of experts whose few rows would otherwise be lost in a tolerance: none is
# needed, every round of `big` moves its expert's dW by >= 10 tolerances as drawn (tests/test_mlp_pairs_cpu.py)
GOUT_GAIN = {}


def layout_weights(name, scale=0.4):
    """Every expert of a layout from its own seed."""
    return [make_weights(1000 + 37 * k + sum(map(ord, name)), scale) for k in range(len(LAYOUTS[name][0]))]


def layout_pairs(name, pad_seed=None):
    rounds, live = LAYOUTS[name]
    return make_pairs(rounds, live, seed=sum(map(ord, name)), pad_seed=pad_seed, gout_gain=GOUT_GAIN.get(name))


def dev(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
