"""Host-side checks of tests/mlp_ref.py, no GPU needed: the hand-written float64 backward is torch.autograd's over the
same chain; the Python restatement of the pair-list backward's round ranges and of the reduce kernel's copy selection
agree on every layout tried; the layouts of tests/test_mlp_pairs_gpu.py reach the paths they are there for; and the
mistakes those tests are there to catch (an expert's rows through another expert's weights, one round missing from an
expert's dW) move the compared quantities by many tolerances, on the reference alone."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_ref as R

G = R.PAIR_DW_BLOCKS


class _TruncExp(torch.autograd.Function):
    """trunc_exp.py: exp of the input clamped at fp32's limit; backward grad * exp(clamped), no clamp mask."""

    @staticmethod
    def forward(ctx, x):
        y = torch.exp(x.clamp(-R.CLAMP, R.CLAMP))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def torch_chain(h0, sh, ws):
    """test_amp.torch_chain without its casts of the outputs to float32 (that one serves fp32 and autocast)."""
    w = dict(zip(R.WNAMES, ws))
    a1 = F.relu(F.linear(h0, w["w0"], w["b0"]))
    a2 = F.relu(F.linear(a1, w["w1"], w["b1"]))
    sig = _TruncExp.apply(F.linear(a2, w["wsh"], w["bsh"]))
    cin = torch.cat([F.linear(a2, w["wg"], w["bg"]), sh], -1)
    c1 = F.relu(F.linear(cin, w["wc0"], w["bc0"]))
    c2 = F.relu(F.linear(c1, w["wc1"], w["bc1"]))
    return torch.cat([torch.sigmoid(F.linear(c2, w["wc2"], w["bc2"])), sig], -1)


def _autograd(h0, sh, gout, ws):
    t =[torch.tensor(np.asarray(x, np.float64)) for x in (h0, sh, gout)]
    h, s = t[0].requires_grad_(True), t[1].requires_grad_(True)
    wr = [torch.tensor(np.asarray(w, np.float64)).requires_grad_(True) for w in ws]
    out = torch_chain(h, s, wr)
    gr = torch.autograd.grad(out, [h, s] + wr, grad_outputs=t[2])
    return out.detach().numpy(), [x.numpy() for x in gr[2:]], gr[0].numpy(), gr[1].numpy()


@pytest.mark.parametrize("scale", [0.4, 12.0])
@pytest.mark.parametrize("n", [1, 33, 300])
def test_reference_backward_is_autograd_in_float64(n, scale):
    """All 14 [dW | db], dL/dh0 and dL/dsh within 1e-12 of max |ref| (both float64, another summation order).  At scale
    12 the ReLU masks are mixed and the sigma head passes the clamp, where TruncExp's gradient stays sigma."""
    ws = R.make_weights(11 + n, scale)
    g = np.random.default_rng(n)
    h0, sh, gout = (g.random((n, 32)) - 0.5) * 2, (g.random((n, 16)) - 0.5) * 2, g.standard_normal((n, 4))
    out, grads, dh0, dsh = R.backward(h0, sh, gout, ws)
    o_t, g_t, h_t, s_t = _autograd(h0, sh, gout, ws)
    if scale > 1 and n > 1:
        pre = np.log(out[:, 3])
        assert (np.abs(pre) >= R.CLAMP * (1 - 1e-12)).any() and (np.abs(pre) < R.CLAMP * 0.99).any()
        _, st = R.forward(h0, sh, ws)
        for a in ("a1", "a2", "c1", "c2"):
            assert 0.05 < float((st[a] > 0).mean()) < 0.95
        assert all(np.abs(grads[i]).max() > 0 for i in range(6)) and np.abs(dh0).max() > 0
    for name, a, b in zip(("out", "dh0", "dsh") + R.WNAMES, [out, dh0, dsh] + grads, [o_t, h_t, s_t] + g_t):
        assert a.shape == b.shape, name
        # (at scale 12 the colour sigmoid saturates to exactly 0 / 1, so the colour branch's gradients are zero there)
        assert np.isfinite(a).all() and (float(np.abs(b).max()) > 0 or scale > 1), name
        assert R.dev(a, b) <= 1e-12, (name, R.dev(a, b))


def test_pairs_ref_is_the_reference_per_segment():
    seg, h0, sh, gout, mask = R.layout_pairs("holes")
    ws = R.layout_weights("holes")
    out, gh0, dw = R.pairs_ref(h0, sh, gout, seg, ws)
    assert out.shape == (4 * 128, 4) and gh0.shape == (4 * 128, 32) and dw.shape == (5, R.MLP_DW_FLOATS) == (5, 13715)
    assert not dw[[0, 2, 4]].any() and dw[1].any() and dw[3].any()
    o3, g3, h3, _ = R.backward(h0[128:], sh[128:], gout[128:], ws[3])
    assert np.array_equal(out[128:], o3) and np.array_equal(gh0[128:], h3) and np.array_equal(dw[3], R.flat_dw(g3))
    assert all(np.array_equal(a, b) for a, b in zip(R.split_dw(dw[3]), g3))
    # padding: zero output gradients, finite values that are not zero, redrawn by pad_seed alone
    assert not gout[~mask].any() and not gh0[~mask].any() and np.abs(h0[~mask]).min() > 0
    seg2, h02, sh2, gout2, mask2 = R.layout_pairs("holes", pad_seed=5)
    assert np.array_equal(h0[mask], h02[mask2]) and np.array_equal(gout, gout2) and not np.array_equal(h0, h02)


def _random_seg(rng, R_, K):
    if K == 1:
        return np.array([0, R_ * R.ROUND], np.int64)
    cuts = np.sort(rng.integers(0, R_ + 1, K - 1))
    if rng.random() < 0.5:                       # force empty experts at either end and in the middle
        cuts[rng.integers(0, K - 1, max(1, (K - 1) // 3))] = rng.choice([0, R_, cuts[0]])
        cuts = np.sort(cuts)
    return np.concatenate([[0], cuts, [R_]]).astype(np.int64) * R.ROUND


def test_reduce_reads_exactly_the_copies_written():
    """copies_read == copies_written at G = 256 for every layout of the GPU tests and, for every R in 0..1200, two
    random splits into K in 1..16 experts (2402 layouts, empty experts included)."""
    for name, (rounds, live) in R.LAYOUTS.items():
        seg = R.make_pairs(rounds, live, 0)[0]
        assert R.copies_read(seg, G) == R.copies_written(seg, G), name
    rng = np.random.default_rng(2024)
    empties = 0
    for R_ in range(1201):
        for _ in range(2):
            K = int(rng.integers(1, 17))
            seg = _random_seg(rng, R_, K)
            assert len(seg) == K + 1 and seg[-1] == R_ * R.ROUND and (np.diff(seg) >= 0).all()
            empties += int((np.diff(seg) == 0).sum() > 0)
            w = R.copies_written(seg, G)
            assert R.copies_read(seg, G) == w, seg.tolist()
            assert {k for _, k in w} == {k for k in range(K) if seg[k + 1] > seg[k]}
    assert empties > 300


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_layouts_reach_what_they_claim(name):
    rounds, live = R.LAYOUTS[name]
    seg = R.make_pairs(rounds, live, 0)[0]
    ranges = R.round_ranges(seg, G)
    empty = sum(not r for r in ranges)
    most = max(len({k for k, _, _ in r}) for r in ranges)
    inside = any(len(r) >= 3 for r in ranges)       # a run that neither starts nor ends its range
    assert (empty, most, inside) == R.LAYOUT_FACTS[name]
    assert all(len({k for k, _, _ in r}) == len(r) for r in ranges)           # one copy per (b, expert)
    assert sorted(rd for r in ranges for _, a, b in r for rd in range(a, b)) == list(range(sum(rounds)))
    if name == "one":
        assert ranges[255] == [(0, 0, 1)]
    if name == "holes":
        assert {k for r in ranges for k, _, _ in r} == {1, 3}
    if name == "thin":
        assert len(rounds) == 16
    if name == "cross":
        assert {len(r) for r in ranges} == {1, 2} and {b - a for r in ranges for _, a, b in r} == {1, 2}
    if name == "big":
        assert int(seg[-1]) == 77440 and ranges[2] == [(3, 4, 5), (4, 5, 6), (5, 6, 7)]
        assert {sum(b - a for _, a, b in r) for r in ranges} == {2, 3}
        fw = R.forward_rounds(seg)
        assert max(len(f) for f in fw) == 2 and fw[0] == [0, 5] and fw[92] == [5, 7] and fw[93] == [5]
    if name.startswith("edge"):
        assert {sum(b - a for _, a, b in r) for r in ranges} == {"edge255": {0, 1}, "edge256": {1},
                                                                  "edge257": {1, 2}}[name]
    assert sum(1 for l in live if l == 1) == (1 if name in ("one", "thin", "big") else 0)
    if len(rounds) > 2:                    # full segments and segments that end mid-tile side by side
        assert any(l == r * 128 for r, l in zip(rounds, live) if r) and any(l % 32 for l in live)


@functools.lru_cache(maxsize=None)
def _big():
    seg, h0, sh, gout, mask = R.layout_pairs("big")
    ws = R.layout_weights("big")
    return seg, h0, sh, gout, mask, ws, R.pairs_ref(h0, sh, gout, seg, ws)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32", "amp"])
def test_wrong_expert_moves_out_by_100_tolerances(precision):
    """Expert k's rows through expert (k + 1) mod K's weights, on the reference at `big`: max |delta out| / max |out|
    over that expert's rows exceeds 100 tolerances (2e-5 for the fp32 paths, amp's absolute term 1e-3)."""
    seg, h0, sh, gout, mask, ws, (out, _, _) = _big()
    K, tol = len(ws), R.TOL_FLOOR[precision]
    for k in range(K):
        a, b = int(seg[k]), int(seg[k + 1])
        if b > a:
            wrong, _ = R.forward(h0[a:b], sh[a:b], ws[(k + 1) % K])
            d = float(np.abs(wrong - out[a:b]).max() / np.abs(out).max())
            assert d > 100 * tol, (k, d)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32", "amp"])
def test_a_dropped_round_moves_dw_by_10_tolerances(precision):
    """Leaving any single round out of its expert's [dW | db] moves at least one of the 14 tensors by more than 10
    tolerances in max |delta| / max |ref|: the contribution a lost or unread partial copy would take away."""
    seg, h0, sh, gout, mask, ws, (_, _, dw) = _big()
    tol, worst = R.TOL_FLOOR[precision], np.inf
    for k in range(len(ws)):
        ref = R.split_dw(dw[k])
        for a in range(int(seg[k]), int(seg[k + 1]), R.ROUND):
            _, part, _, _ = R.backward(h0[a:a + 128], sh[a:a + 128], gout[a:a + 128], ws[k])
            d = max(float(np.abs(p).max() / np.abs(r).max()) for p, r in zip(part, ref))
            worst = min(worst, d)
            assert d > 10 * tol, (k, a // 128, d)
    print(f"dropped round at big: smallest move {worst:.3e} = {worst / tol:.0f} tolerances ({precision})")


@pytest.mark.parametrize("name", [n for n in R.LAYOUTS if n != "none"])
def test_no_reference_value_is_a_near_cancellation(name):
    """For every expert and each of its 14 tensors, the largest reference element is at least one standard deviation
    of its own terms' random walk away from 0 (ratio >= 1), so rounding every term to fp16 (2^-11) moves it by about
    5e-4 of itself at most and the relative measure of the GPU tests measures arithmetic.  With zero-mean output
    gradients the one-element dL/dbsh of `cross`, expert 1, had ratio 0.11 (see make_pairs)."""
    seg, h0, sh, gout, mask = R.layout_pairs(name)
    ws = R.layout_weights(name)
    worst = np.inf
    for k in range(len(ws)):
        a, b = int(seg[k]), int(seg[k + 1])
        if b > a:
            c = R.cancellation(h0[a:b], sh[a:b], gout[a:b], ws[k])
            worst = min(worst, min(c))
            assert min(c) >= 1.0 - 1e-9, (k, R.WNAMES[int(np.argmin(c))], min(c))
    print(f"{name}: smallest |sum| / sqrt(sum of squares) {worst:.2f}")
