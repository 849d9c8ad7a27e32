"""The routed pair-list entry points of csrc/mlp_train.hip (acn_mlp_pack_pairs, acn_mlp_train_fwd_pairs,
acn_mlp_train_bwd_dw_pairs -> mlp_bwd_dw_pairs_pc_kernel + mlp_dw_reduce_pairs_kernel) called directly, in the three
builds (fp16x3, fp32, amp), against the float64 reference of tests/mlp_ref.py at segment layouts chosen for the index
arithmetic: R = seg[K] / 128 rounds against the backward's G = 256 workgroups and the forward's 512 (mlp_ref.LAYOUTS;
what each reaches is asserted in tests/test_mlp_pairs_cpu.py).

Measure: max |got - ref| / max |ref|, per tensor and per expert.  Bound: not fixed in advance -- the plain torch chain
(test_amp.torch_chain, F.linear per layer) runs on the same rows in the same test, in float32 for fp16x3 / fp32 and
under torch.autocast(float16) for amp, and its error e_chain against the same float64 reference sets
max(2e-5, 4 e_chain) (fp16x3 / fp32, the rule of test_normals_gpu.py) or 2 e_chain + 1e-3 (amp, the rule of
test_amp.py).  amp runs with the output gradient scaled by 2^16 as GradScaler does.  Every buffer the kernels write
is followed by 256 canary rows that must come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_ref as R

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp16x3", "fp32", "amp")
SENTINEL = -7777.0
CANARY = 256
AMP_SCALE = 2.0 ** 16


def _ops():
    from adaptive_city_nerf_amd import ops
    assert tuple(ops.MLP_DW_SHAPES) == R.MLP_DW_SHAPES and ops.MLP_DW_FLOATS == R.MLP_DW_FLOATS
    return ops


class Buffers:
    """Workspace (zeroed) and outputs for up to K experts and n slots; out / gh0 end in canary rows."""

    def __init__(self, K, n, precision):
        ops = _ops()
        self.floats = int(ops.mlp_fn("acn_mlp_pairs_workspace_bytes", precision)(K)) // 4
        self.img_floats = int(ops.mlp_fn("acn_mlp_workspace_bytes", precision)()) // 4
        assert self.floats == K * self.img_floats + R.PAIR_DW_BLOCKS * K * R.MLP_DW_FLOATS
        self.mws = torch.zeros(self.floats, device="cuda")
        self.out = torch.full((n + CANARY, 4), SENTINEL, device="cuda")
        self.gh0 = torch.full((n + CANARY, 32), SENTINEL, device="cuda")
        self.dw = torch.zeros(K, R.MLP_DW_FLOATS, device="cuda")


@functools.lru_cache(maxsize=None)
def _weights(name):
    return [[torch.from_numpy(w).cuda() for w in ws] for ws in R.layout_weights(name)]


@functools.lru_cache(maxsize=None)
def _inputs(name, precision, pad_seed=None):
    """Device rows of a layout (+128 slack rows so that no pointer is NULL at seg[K] = 0); amp: gout scaled by 2^16."""
    seg, h0, sh, gout, mask = R.layout_pairs(name, pad_seed)
    g = np.random.default_rng(1)
    slack = [((g.random((128, c)) - 0.5) * 2).astype(np.float32) for c in (32, 16, 4)]
    dev = [torch.from_numpy(np.concatenate([a, s])).cuda() for a, s in zip((h0, sh, gout), slack)]
    if precision == "amp":
        dev[2] *= AMP_SCALE
    return torch.from_numpy(seg).cuda(), dev[0], dev[1], dev[2], mask


def run_pairs(name, precision, bufs=None, pad_seed=None, poison=False):
    """pack + forward + backward as RoutedAdaptStep issues them; returns clones of out (n, 4), gh0 (n, 32), dw (K, NDW).
    poison: after the pack, NaN over the workspace's partial copies, dw and gh0."""
    ops = _ops()
    from adaptive_city_nerf_amd._lib import acn_mlp, check, ptr, stream_of
    seg, h0, sh, gout, _ = _inputs(name, precision, pad_seed)
    ws = _weights(name)
    K, n = len(ws), h0.shape[0] - 128
    bufs = bufs or Buffers(K, n, precision)
    assert bufs.floats >= K * bufs.img_floats + R.PAIR_DW_BLOCKS * K * R.MLP_DW_FLOATS and bufs.out.shape[0] >= n + CANARY
    structs = [ops._mlp_struct(w) for w in ws]
    ptrs = (C.POINTER(acn_mlp) * K)(*[C.pointer(s) for s in structs])
    tails = [bufs.out[n:].clone(), bufs.gh0[n:].clone(), bufs.dw[K:].clone()]
    fn, s = (lambda f: ops.mlp_fn(f, precision)), stream_of(h0)
    check(fn("acn_mlp_pack_pairs")(ptrs, K, ptr(bufs.mws), s), "acn_mlp_pack_pairs")
    check(fn("acn_mlp_train_fwd_pairs")(ptr(h0), ptr(sh), ptr(seg), K, ptr(bufs.mws), ptr(bufs.out), s),
          "acn_mlp_train_fwd_pairs")
    torch.cuda.synchronize()
    assert torch.equal(bufs.out[n:], tails[0]), "forward wrote past seg[K]"
    if poison:
        bufs.mws[K * bufs.img_floats:].fill_(float("nan"))
        bufs.dw[:K].fill_(float("nan"))
        bufs.gh0[:n].fill_(float("nan"))
    check(fn("acn_mlp_train_bwd_dw_pairs")(ptr(h0), ptr(sh), ptr(bufs.out), ptr(gout), ptr(seg), K, ptr(bufs.mws),
                                           ptr(bufs.dw), ptr(bufs.gh0), s), "acn_mlp_train_bwd_dw_pairs")
    torch.cuda.synchronize()
    assert torch.equal(bufs.out[n:], tails[0]) and torch.equal(bufs.gh0[n:], tails[1]), "backward wrote past seg[K]"
    assert torch.equal(bufs.dw[K:], tails[2])
    return bufs.out[:n].clone(), bufs.gh0[:n].clone(), bufs.dw[:K].clone()


@functools.lru_cache(maxsize=None)
def _base(name, precision):
    """One run in fresh buffers, shared (read-only) by the tests below."""
    return run_pairs(name, precision)


@functools.lru_cache(maxsize=None)
def _ref(name, pad_seed=None):
    """pairs_ref of the layout (unscaled gout; gh0 and dw are linear in gout, so amp's are these times 2^16 exactly)."""
    seg, h0, sh, gout, mask = R.layout_pairs(name, pad_seed)
    return R.pairs_ref(h0, sh, gout, seg, R.layout_weights(name))


def _ref_for(name, precision, pad_seed=None):
    out, gh0, dw = _ref(name, pad_seed)
    s = AMP_SCALE if precision == "amp" else 1.0
    return out, gh0 * s, dw * s


@functools.lru_cache(maxsize=None)
def _chain(name, amp, pad_seed=None):
    """The plain torch chain per segment: out, dL/dh0 and [dW | db] rows as float64 numpy (float32 arithmetic, or
    autocast(float16) with the 2^16 loss scale)."""
    from test_amp import torch_chain
    seg, h0, sh, gout, _ = _inputs(name, "amp" if amp else "fp32", pad_seed)
    ws = _weights(name)
    K, n = len(ws), h0.shape[0] - 128
    out, gh0, dw = np.zeros((n, 4)), np.zeros((n, 32)), np.zeros((K, R.MLP_DW_FLOATS))
    seg = seg.cpu().tolist()
    for k in range(K):
        a, b = seg[k], seg[k + 1]
        if b > a:
            h = h0[a:b].clone().requires_grad_(True)
            wr = [w.clone().requires_grad_(True) for w in ws[k]]
            o = torch_chain(h, sh[a:b], wr, amp)
            gr = torch.autograd.grad(o, [h] + wr, grad_outputs=gout[a:b])
            out[a:b], gh0[a:b] = o.detach().double().cpu().numpy(), gr[0].double().cpu().numpy()
            dw[k] = R.flat_dw([g.double().cpu().numpy() for g in gr[1:]])
    return out, gh0, dw


def _bounds(name, precision, pad_seed=None):
    """{(expert, tensor): bound} from the chain's own error against the float64 reference, and those errors."""
    ref, chain = _ref_for(name, precision, pad_seed), _chain(name, precision == "amp", pad_seed)
    seg = R.layout_pairs(name)[0].tolist()
    bound, e_chain = {}, {}
    for k in range(len(seg) - 1):
        a, b = seg[k], seg[k + 1]
        if b == a:
            continue
        items = [("out", chain[0][a:b], ref[0][a:b]), ("gh0", chain[1][a:b], ref[1][a:b])]
        items += list(zip(R.WNAMES, R.split_dw(chain[2][k]), R.split_dw(ref[2][k])))
        for t, c, r in items:
            e = R.dev(c, r)
            e_chain[k, t] = e
            bound[k, t] = 2 * e + 1e-3 if precision == "amp" else max(2e-5, 4 * e)
    return bound, e_chain


def _errors(name, got, ref):
    """{(expert, tensor): max |got - ref| / max |ref|} of out, gh0 and the 14 [dW | db] per expert with rows."""
    seg = R.layout_pairs(name)[0].tolist()
    got = [x.double().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got]
    err = {}
    for k in range(len(seg) - 1):
        a, b = seg[k], seg[k + 1]
        if b == a:
            continue
        err[k, "out"], err[k, "gh0"] = R.dev(got[0][a:b], ref[0][a:b]), R.dev(got[1][a:b], ref[1][a:b])
        for t, g, r in zip(R.WNAMES, R.split_dw(got[2][k]), R.split_dw(ref[2][k])):
            err[k, t] = R.dev(g, r)
    return err


def _worst(d, only=None):
    ks = [k for k in d if only is None or (k[1] in only)]
    return max((d[k] for k in ks), default=0.0)


def _report(tag, name, precision, err, e_chain, bound):
    groups = (("out", ("out",)), ("gh0", ("gh0",)), ("dw", R.WNAMES))
    msg = "; ".join(f"{g} kernel {_worst(err, t):.2e} chain {_worst(e_chain, t):.2e} bound>={min([bound[k] for k in bound if k[1] in t], default=0):.2e}"
                    for g, t in groups)
    print(f"PAIRS {tag} {name} {precision}: {msg}")


def _assert_within(name, precision, got, tag, pad_seed=None):
    bound, e_chain = _bounds(name, precision, pad_seed)
    err = _errors(name, got, _ref_for(name, precision, pad_seed))
    _report(tag, name, precision, err, e_chain, bound)
    bad = {k: (err[k], bound[k]) for k in err if not err[k] <= bound[k]}
    assert not bad, bad
    return bound


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_pairs_against_float64(name, precision):
    """(a) out over all seg[K] rows (padding included), gh0 and every expert's 14 [dW | db] within the chain-derived
    bound; (b) what must be exact: zero dw rows of experts without pairs, zero gh0 of padding rows, fp16 values in amp."""
    out, gh0, dw = _base(name, precision)
    seg, _, _, _, mask = R.layout_pairs(name)
    assert torch.isfinite(out).all() and torch.isfinite(gh0).all() and torch.isfinite(dw).all()
    _assert_within(name, precision, (out, gh0, dw), "a")
    for k in range(len(seg) - 1):
        if seg[k + 1] == seg[k]:
            assert int((dw[k] != 0).sum()) == 0, k
        else:
            assert int((dw[k] != 0).sum()) > 0, k
    pad = torch.from_numpy(~mask).cuda()
    assert int((gh0[pad] != 0).sum()) == 0
    if mask.any():
        assert int((gh0[~pad] != 0).sum()) > 0
    if precision == "amp":
        assert torch.equal(out, out.half().float()) and torch.equal(dw, dw.half().float())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_padding_is_inert(name, precision):
    """(c) Other finite h0 / sh in the padding slots (gout = 0 there): dw meets the bound of (a) again, and out / gh0 of
    every 32-row tile of live rows only are bit-equal between the two runs."""
    out1, gh1, dw1 = _base(name, precision)
    out2, gh2, dw2 = run_pairs(name, precision, pad_seed=4242)
    _, h01, _, _, mask = _inputs(name, precision)
    _, h02, _, _, _ = _inputs(name, precision, 4242)
    pad = torch.from_numpy(~mask).cuda()
    n = mask.shape[0]
    assert torch.equal(h01[:n][~pad], h02[:n][~pad])
    _assert_within(name, precision, (out2, gh2, dw2), "c", 4242)
    tiles = torch.from_numpy(mask.reshape(-1, 32).all(1).repeat(32)).cuda()
    if name in ("thin", "holes", "cross", "big"):                 # live rows in mixed tiles exist and are left out
        assert 0 < int(tiles.sum()) < int((~pad).sum())
    assert torch.equal(out1[tiles], out2[tiles]) and torch.equal(gh1[tiles], gh2[tiles])
    if name not in ("none", "edge256"):                           # the padding rows did change
        assert not torch.equal(h01[:n][pad], h02[:n][pad]) and not torch.equal(out1[pad], out2[pad])
    else:
        assert int(pad.sum()) == 0
    assert int((gh2[pad] != 0).sum()) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_stale_workspace_and_outputs(name, precision):
    """(d) NaN in every partial copy of the workspace, in dw and in gh0 before the backward: finite results, bit-equal
    to the run in a fresh zeroed workspace -- the reduce adds no copy that this call did not write, and every dw and
    gh0 element is written."""
    out, gh0, dw = run_pairs(name, precision, poison=True)
    assert torch.isfinite(gh0).all() and torch.isfinite(dw).all()
    base = _base(name, precision)
    assert torch.equal(out, base[0]) and torch.equal(gh0, base[1]) and torch.equal(dw, base[2])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_new_seg_in_the_same_buffers(precision):
    """(d) The graph-replay situation: `big`, then `holes` in the same workspace and buffers with nothing cleared in
    between (copies, images, out, gh0 and dw of the larger layout still there): bit-equal to `holes` run fresh."""
    K, n = len(R.LAYOUTS["big"][0]), int(R.layout_pairs("big")[0][-1])
    bufs = Buffers(K, n, precision)
    big = run_pairs("big", precision, bufs)
    assert all(torch.equal(a, b) for a, b in zip(big, _base("big", precision)))
    got = run_pairs("holes", precision, bufs)
    assert all(torch.equal(a, b) for a, b in zip(got, _base("holes", precision)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_pairs_equal_the_single_expert_entry_points(name, precision):
    """(e) Per segment, acn_mlp_train_fwd / acn_mlp_train_bwd_dw on the slice with that expert's weights: out and gh0
    bit-identical (same tile_forward, same dX chain, segments start at multiples of 128 so the 32-row tiles coincide);
    dw, summed in another order, within the bound of (a)."""
    ops = _ops()
    out, gh0, dw = _base(name, precision)
    seg, h0, sh, gout, _ = _inputs(name, precision)
    ws = _weights(name)
    bound, _ = _bounds(name, precision)
    seg = seg.cpu().tolist()
    worst = 0.0
    for k in range(len(ws)):
        a, b = seg[k], seg[k + 1]
        if b == a:
            continue
        o1, _ = ops.mlp_train_fwd(h0[a:b], sh[a:b], ws[k], save=False, precision=precision)
        g1, h1 = ops.mlp_train_bwd_dw(h0[a:b], sh[a:b], o1, gout[a:b], ws[k], want_h0=True, precision=precision)
        assert torch.equal(out[a:b], o1), (k, "out")
        assert torch.equal(gh0[a:b], h1), (k, "gh0")
        for t, p, s in zip(R.WNAMES, R.split_dw(dw[k].double().cpu().numpy()), g1):
            e = R.dev(p, s.double().cpu().numpy())
            worst = max(worst, e)
            assert e <= bound[k, t], (k, t, e, bound[k, t])
    print(f"PAIRS e {name} {precision}: out, gh0 bit-equal; dw pair-list against single-expert {worst:.2e}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_pairs_are_deterministic(name, precision):
    """(f) Two calls on the same inputs: bit-equal out, gh0 and dw (no atomics on this path)."""
    again = run_pairs(name, precision)
    assert all(torch.equal(a, b) for a, b in zip(again, _base(name, precision)))
