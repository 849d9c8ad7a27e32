"""The optimizer kernels of csrc/optim.hip against the float64 reference of tests/adam_ref.py, driven directly through
FusedAdam, SlottedAdam and AmpScaler on synthetic tensors: every element of p, exp_avg and exp_avg_sq, no excluded
fraction.  Sizes sit on the code's boundaries (256 threads, 4 vectors in flight, 4-float vectors, 16-float segments,
65536-float chunks); parameters, gradients and moments are slices of arenas filled with a sentinel, which must be
intact after every step (a vector store past a tail); storage offsets of 1-3 floats send the kernels down their
scalar paths.  The tolerance is 4 x the error of the float32 emulation (adam_ref.adam_step32) against float64 on the
very inputs of each test, in the units of adam_ref.units(); the measured figures are in DESIGN.md 4x.  Exact zeros,
inactive slots, skipped steps, gradients, maps and counters are held bitwise."""
import functools

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FA5C3E1      # a NaN bit pattern: a read of it poisons whatever uses it
ALIGNED = (0, 0, 0, 0)
MISALIGNED = ([tuple(k if a == b else 0 for b in range(4)) for a in range(4) for k in (1, 2, 3)]
              + [(k,) * 4 for k in (1, 2, 3)])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class Arena:
    """Slices of one buffer pre-filled with SENT, each `off` floats past a 16-byte boundary, 8 floats apart."""

    def __init__(self, sizes, off, dev):
        cur, self.spans = 8, []
        for n in sizes:
            self.spans.append((cur + off, n))
            cur = (cur + off + n + 3) // 4 * 4 + 8
        self.buf = torch.full((cur,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.free = np.ones(cur, bool)
        for s, n in self.spans:
            self.free[s:s + n] = False
        self.views = [self.buf[s:s + n] for s, n in self.spans]

    def host(self):
        """The slices on the host, after checking that nothing outside them was written."""
        h = self.buf.cpu().numpy()
        assert (h.view(np.int32)[self.free] == SENT).all(), "a store landed outside the tensors"
        return [h[s:s + n].copy() for s, n in self.spans]


class Rig:
    """A scenario's tensors on the device: arenas for p / g / m / v, torch Parameters over the p slices, a FusedAdam
    whose state holds the m / v slices (a tensor of a slot that starts at step 0 gets no state when `pending`: the
    SlottedAdam then keeps its moments itself until the slot has stepped)."""

    def __init__(self, sc, dev, mis=ALIGNED, pending=False):
        from adaptive_city_nerf_amd import optim as O
        self.sc, self.dev = sc, dev
        sizes = [s[0] for s in sc.specs]
        self.A = [Arena(sizes, o, dev) for o in mis]
        P, G, M, V = (a.views for a in self.A)
        for i in range(len(sizes)):
            P[i].copy_(torch.from_numpy(sc.p0[i]))
            G[i].zero_()
            M[i].copy_(torch.from_numpy(sc.m0[i]))
            V[i].copy_(torch.from_numpy(sc.v0[i]))
        self.params = [torch.nn.Parameter(v) for v in P]
        for p, v, o in zip(self.params, P, mis[:1] * len(P)):
            assert p.data_ptr() == v.data_ptr() and p.data_ptr() % 16 == 4 * o
        self.opt = O.FusedAdam([dict(params=[p for p, s in zip(self.params, sc.specs) if s[2] == g], lr=hp["lr"],
                                     betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"])
                                for g, hp in enumerate(sc.hps)])
        self.own = []     # tensors whose moments live outside the arenas (pending state)
        for i, (p, s) in enumerate(zip(self.params, sc.specs)):
            if pending and sc.start[s[1]] == 0:
                self.own.append(i)
                continue
            self.opt.state[p] = dict(step=torch.tensor(float(sc.start[s[1]])), exp_avg=M[i], exp_avg_sq=V[i])
        self.maps = {}
        for i, s in enumerate(sc.specs):
            if s[4]:
                nseg = (s[0] + R.SEG - 1) // R.SEG
                self.maps[i] = tuple(torch.zeros(nseg, dtype=torch.uint8, device=dev) for _ in range(2))

    def slotted(self, segmaps=True, **kw):
        from adaptive_city_nerf_amd import optim as O
        assert (O.ZERO_GRAD_FLAG, O.NORM_ELSEWHERE_FLAG) == (R.ZERO_GRAD, R.NORM_ELSEWHERE)
        sc = self.sc
        ps = self.params
        sa = O.SlottedAdam(self.opt, {id(p): s[1] for p, s in zip(ps, sc.specs)},
                           {id(p): g for p, g in zip(ps, self.A[1].views)}, sc.K, sc.nslots,
                           flags={id(p): s[3] for p, s in zip(ps, sc.specs)}, max_steps=sc.max_steps,
                           segmaps={id(ps[i]): mp for i, mp in self.maps.items()} if segmaps and self.maps else None,
                           **kw)
        self.mv = {id(r[0]): (r[2], r[3]) for r in sa.rows}
        assert sa.table_steps == sc.table_steps and sa.step_dev.tolist() == sc.start
        return sa

    def feed(self, j, gmul=1.0):
        """Step j's gradients (times a power of two) and now marks."""
        for i, g in enumerate(self.A[1].views):
            g.copy_(torch.from_numpy(self.sc.grads[i][j] * np.float32(gmul)))
        for i, (now, ever) in self.maps.items():
            tm = self.sc.steps[j].get("touch", {}).get(i)
            now.copy_(torch.from_numpy(np.zeros(now.numel(), np.uint8) if tm is None else tm.astype(np.uint8)))

    def seg(self, j):
        """[starts 0..K-1 | total pairs, < 0: skipped step | pair counts K+1..2K] (routed.hip)."""
        st, K = self.sc.steps[j], self.sc.K
        c = list(st["counts"])
        starts = [sum(c[:k]) for k in range(K)]
        return torch.tensor(starts + [-1 if st.get("skip") else sum(c)] + c, dtype=torch.int64, device=self.dev)

    def snapshot(self):
        torch.cuda.synchronize()
        p, g, m, v = (a.host() for a in self.A)
        for i in self.own:
            mm, vv = self.mv[id(self.params[i])]
            m[i], v[i] = mm.cpu().numpy(), vv.cpu().numpy()
        return dict(p=p, g=g, m=m, v=v, now={i: a.cpu().numpy() for i, (a, b) in self.maps.items()},
                    ever={i: b.cpu().numpy() for i, (a, b) in self.maps.items()})


@functools.lru_cache(maxsize=None)
def _reference(make, *args):
    """(scenario, the float64 model's state after every step, the 4 x yardstick bounds)."""
    sc = getattr(R, make)(*args)
    traj = []

    def snap(j, mdl, total):
        traj.append(dict(t=[dict(p=t.p.copy(), m=t.m.copy(), v=t.v.copy(), g=t.g.copy(), gmax=t.gmax,
                                 ever=None if t.ever is None else t.ever.copy(), mapped=mdl.is_mapped(t))
                            for t in mdl.t], counters=list(mdl.counters), total=total,
                         active=mdl.active(sc.steps[j]["counts"], sc.steps[j].get("skip", False))))
    mdl = sc.run(snapshot=snap)
    assert mdl.floor_ok
    y = sc.yardstick()
    assert y[3] == 0
    return sc, traj, [4.0 * a for a in y[:3]]


class _Ref:   # what adam_ref.errors reads of a model tensor
    def __init__(self, d):
        self.p, self.m, self.v, self.gmax, self.n = d["p"], d["m"], d["v"], d["gmax"], len(d["p"])


def _compare(sc, got, ref, bound, worst, what):
    """Every element of every tensor within `bound` units; elements with an all-zero history bitwise."""
    for i, r in enumerate(ref["t"]):
        e = R.errors((got["p"][i], got["m"][i], got["v"][i]), _Ref(r), sc.hps[sc.specs[i][2]]["lr"])
        for q in range(3):
            worst[q] = max(worst[q], e[q])
            assert e[q] <= bound[q], (what, i, sc.specs[i], "pmv"[q], e[q], bound[q])
        z = R.zero_mask(sc.specs[i][0])
        assert np.array_equal(got["p"][i][z], sc.p0[i][z]) and not got["m"][i][z].any() and not got["v"][i][z].any()


def _ulp_close(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or abs(float(a) - float(b)) <= float(np.spacing(np.abs(b)))


# ------------------------------------------------------------------------------------------------ a. FusedAdam
@pytest.mark.parametrize("max_norm", [None, 30.0])
@pytest.mark.parametrize("mis", [ALIGNED] + MISALIGNED, ids=lambda m: "pgmv=%d%d%d%d" % m)
def test_fused_adam_every_element_against_float64(dev, mis, max_norm):
    """5 steps over the unmapped sizes in two groups (wd 0 / 0.01), each of p, g, m, v in turn (then all) at a
    storage offset of 1-3 floats: a torch Parameter wraps an offset view, so this goes through FusedAdam.step."""
    sc, traj, bound = _reference("plain_scenario", max_norm)
    rig = Rig(sc, dev, mis)
    worst = [0.0, 0.0, 0.0]
    for j in range(len(sc.steps)):
        rig.feed(j)
        for p, g in zip(rig.params, rig.A[1].views):
            p.grad = g
        rig.opt.step(max_norm=max_norm)
        got = rig.snapshot()
        _compare(sc, got, traj[j], bound, worst, f"step {j}")
        for i, g in enumerate(got["g"]):
            assert np.array_equal(g, sc.grads[i][j])          # the clipped gradient is never written back
        if max_norm is not None:
            norm, coef = R.clip_coef32(traj[j]["total"], max_norm)
            ln = rig.opt.last_norm.cpu().numpy()
            assert _ulp_close(ln[0], norm) and _ulp_close(ln[1], coef), (ln, norm, coef)
    assert all(int(rig.opt.state[p]["step"]) == 5 for p in rig.params)
    print(f"FusedAdam {mis} max_norm={max_norm}: worst p {worst[0]:.2f} m {worst[1]:.2f} v {worst[2]:.2f} units "
          f"(bounds {bound[0]:.1f} {bound[1]:.1f} {bound[2]:.1f})")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_grad_sumsq_on_an_offset_gradient(dev, off):
    from adaptive_city_nerf_amd import optim as O
    sc, _, _ = _reference("plain_scenario", None)
    rig = Rig(sc, dev, (0, off, 0, 0))
    rig.feed(2)
    for p, g in zip(rig.params, rig.A[1].views):
        p.grad = g
    total = float(O.grad_sumsq(rig.params, dev).cpu())
    want = R.norm_total([g[2] for g in sc.grads])
    assert abs(total - want) <= 1e-12 * want, (total, want)
    rig.snapshot()


# ------------------------------------------------------------------------------------------------ b. graph mode, eager
def test_fused_adam_table_mode_without_a_capture(dev):
    """Two plain steps, graph_begin(max_steps=4), three table steps (the host step count is put back after each, as
    after a capture): bitwise the five plain steps.  A fourth table step is the table's last row; the fifth finds no
    row, writes nothing, and graph_sync_steps raises."""
    from adaptive_city_nerf_amd._lib import AcnError
    sc, traj, bound = _reference("plain_scenario", 30.0)
    plain, table = Rig(sc, dev), Rig(sc, dev)
    for rig in (plain, table):
        for p, g in zip(rig.params, rig.A[1].views):
            p.grad = g
    for j in range(5):
        for rig in (plain, table):
            rig.feed(j)
        plain.opt.step(max_norm=30.0)
        if j == 2:
            table.opt.graph_begin(max_steps=4)
        table.opt.step(max_norm=30.0)
        if j >= 2:
            table.opt.graph_end_capture()
        a, b = plain.snapshot(), table.snapshot()
        for q in "pmv":
            for x, y in zip(a[q], b[q]):
                assert np.array_equal(x, y), (j, q)
    table.opt.graph_sync_steps(3)
    assert all(int(table.opt.state[p]["step"]) == 5 for p in table.params)
    table.opt.graph_sync_steps(0)
    table.feed(0)
    table.opt.step(max_norm=30.0)      # row 3: the last
    table.opt.graph_end_capture()
    last = table.snapshot()
    assert not np.array_equal(last["p"][5], b["p"][5])
    table.opt.step(max_norm=30.0)      # no row 4
    table.opt.graph_end_capture()
    after = table.snapshot()
    for q in "pmv":
        for x, y in zip(last[q], after[q]):
            assert np.array_equal(x, y), q
    assert int(table.opt._graph["step_dev"]) == 7
    with pytest.raises(AcnError, match="exceeded"):
        table.opt.graph_sync_steps(5)


# ------------------------------------------------------------------------------------------------ c. SlottedAdam
def _run_slotted(rig, sa, split=False, amp=None, gmul=1.0, hook=None):
    """Every step of the rig's scenario; the snapshots, each with the device counters, total and scale."""
    sc = rig.sc
    extra = torch.zeros(1, dtype=torch.float64, device=rig.dev)
    use_extra = any(st.get("extra", 0.0) for st in sc.steps)
    out = []
    for j, st in enumerate(sc.steps):
        rig.feed(j, gmul)
        seg = rig.seg(j)
        extra.fill_(st.get("extra", 0.0) * gmul * gmul)
        if split:
            sa.step_early(seg)
        sa.step(seg, sc.max_norm, extra if use_extra else None, amp=amp, phase=2 if split else 0)
        s = rig.snapshot()
        s.update(counters=sa.step_dev.tolist(), total=float(sa.total.cpu()) if sc.max_norm is not None else None,
                 scale=sa.scale.cpu().numpy().copy(), extra=float(extra.cpu()), seg=seg.cpu().tolist())
        out.append(s)
        if hook:
            hook(j, s)
    return out


def _check_slotted(sc, traj, bound, snaps, what):
    worst = [0.0, 0.0, 0.0]
    prev = dict(p=sc.p0, m=sc.m0, v=sc.v0, counters=sc.start)
    for j, (got, ref) in enumerate(zip(snaps, traj)):
        _compare(sc, got, ref, bound, worst, f"{what} step {j}")
        assert got["counters"] == ref["counters"], (what, j)
        skip = sc.steps[j].get("skip", False)
        for i, (n, slot, group, flags, mapped) in enumerate(sc.specs):
            assert np.array_equal(got["g"][i], ref["t"][i]["g"]), (what, j, i, "gradient")
            if flags & R.ZERO_GRAD and (ref["active"][slot] or skip) and got["counters"][slot] <= sc.table_steps:
                assert not got["g"][i].any()
            elif not flags & R.ZERO_GRAD or not ref["active"][slot]:
                assert np.array_equal(got["g"][i], sc.grads[i][j])
            if skip or not ref["active"][slot]:
                for q in "pmv":
                    assert np.array_equal(got[q][i], prev[q][i]), (what, j, i, q, "moved in an inactive slot")
                assert got["counters"][slot] == prev["counters"][slot]
        prev = got
    return worst


@pytest.mark.parametrize("mis", [ALIGNED, (0, 1, 0, 0), (3, 3, 3, 3), (2, 0, 1, 3)], ids=lambda m: "pgmv=%d%d%d%d" % m)
def test_slotted_adam_dense_against_the_model(dev, mis):
    """K = 3 experts + a shared slot from different start steps; one expert, none, all, a skipped step, all, two.
    The offsets send adam_chunk, adam_chunk_zero and the norm down their scalar paths."""
    sc, traj, bound = _reference("slotted_scenario")
    rig = Rig(sc, dev, mis, pending=True)
    sa = rig.slotted()
    pend = [rig.params[i] for i in rig.own]
    assert pend and all(p not in rig.opt.state for p in pend)

    def hook(j, s):
        if j in (0, 5):
            sa.sync_state()
            for p, spec in zip(rig.params, sc.specs):
                if p in rig.opt.state:
                    assert int(rig.opt.state[p]["step"]) == traj[j]["counters"][spec[1]]
            # slot 2 has not stepped after step 0, and has after step 5
            assert all((p in rig.opt.state) == (j == 5) for p in pend)
    snaps = _run_slotted(rig, sa, hook=hook)
    worst = _check_slotted(sc, traj, bound, snaps, "dense")
    for j, (got, ref) in enumerate(zip(snaps, traj)):
        assert abs(got["total"] - ref["total"]) <= 1e-12 * ref["total"] + 1e-300
        norm, coef = R.clip_coef32(ref["total"], sc.max_norm)
        assert _ulp_close(got["scale"][0], norm) and _ulp_close(got["scale"][1], coef)
    for i in rig.own:
        assert rig.opt.state[rig.params[i]]["exp_avg"] is rig.mv[id(rig.params[i])][0]
    print(f"SlottedAdam {mis}: worst p {worst[0]:.2f} m {worst[1]:.2f} v {worst[2]:.2f} units "
          f"(bounds {bound[0]:.1f} {bound[1]:.1f} {bound[2]:.1f})")


def test_slotted_adam_beyond_its_table(dev):
    """max_steps = 2 from slot 0's step 4: its third activation finds no row; nothing of it is written, the
    counter still advances, and sync_state raises."""
    from adaptive_city_nerf_amd._lib import AcnError
    sc, traj, bound = _reference("slotted_scenario", 2)
    rig = Rig(sc, dev)
    sa = rig.slotted()
    snaps = _run_slotted(rig, sa)
    _check_slotted(sc, traj, bound, snaps, "short table")
    assert snaps[-1]["counters"][0] == 7 > sa.table_steps == 6
    for i, spec in enumerate(sc.specs):
        if spec[1] == 0:
            for q in "pmv":
                assert np.array_equal(snaps[5][q][i], snaps[4][q][i])
            assert np.array_equal(snaps[5]["g"][i], sc.grads[i][5])
    with pytest.raises(AcnError, match="exhausted"):
        sa.sync_state()


def test_slotted_adam_is_repeatable(dev):
    sc, _, _ = _reference("slotted_scenario")
    runs = []
    for _ in range(2):
        rig = Rig(sc, dev)
        runs.append(_run_slotted(rig, rig.slotted()))
    for a, b in zip(*runs):
        for q in "pmvg":
            for x, y in zip(a[q], b[q]):
                assert np.array_equal(x, y)
        assert a["total"] == b["total"] and np.array_equal(a["scale"], b["scale"]) and a["counters"] == b["counters"]


# ------------------------------------------------------------------------------------------------ d. the clip norm
@pytest.mark.parametrize("shape", ["mixed", "300x3", "one"])
def test_clip_norm_total_and_one_launch_equals_three(dev, shape, monkeypatch):
    """The total against the float64 sum (inactive slots and NORM_ELSEWHERE tensors out, table_sumsq in and reset);
    the one-launch clip (FUSED_CLIP) against sumsq + reduce + coefficient, bitwise, on six consecutive calls that
    reuse the ticket counter; 300 chunks (the strided partial sums) and a single one."""
    from adaptive_city_nerf_amd import optim as O
    args = {"mixed": (64, 40.0, True), "300x3": (64, 2.0, False, (3,) * 300), "one": (64, 2.0, True, (48,))}[shape]
    sc, traj, bound = _reference("slotted_scenario", *args)
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(O, "FUSED_CLIP", fused)
        rig = Rig(sc, dev)
        sa = rig.slotted()
        assert sa.nchunks == {"mixed": 16, "300x3": 300, "one": 1}[shape]
        assert (sa.norm_plan is not None) == (shape == "mixed")
        runs[fused] = _run_slotted(rig, sa)
        assert int(sa.ticket) == 0
    for j, (a, b, ref) in enumerate(zip(runs[True], runs[False], traj)):
        assert a["total"] == b["total"] and np.array_equal(a["scale"].view(np.int32), b["scale"].view(np.int32)), j
        for q in "pmv":
            for x, y in zip(a[q], b[q]):
                assert np.array_equal(x, y)
        assert abs(a["total"] - ref["total"]) <= 1e-12 * ref["total"], (j, a["total"], ref["total"])
        assert a["extra"] == 0.0 and b["extra"] == 0.0
    # the reference total is not the all-tensor sum: inactive slots and NORM_ELSEWHERE tensors are really left out
    if shape == "mixed":
        everything = R.norm_total([g[0] for g in sc.grads], sc.steps[0]["extra"])
        assert traj[0]["total"] < 0.9 * everything and sc.steps[0]["extra"] > 0.01 * traj[0]["total"]
    _check_slotted(sc, traj, bound, runs[True], shape)


def test_clip_norm_of_zero_and_nan_gradients(dev):
    sc, _, _ = _reference("slotted_scenario", 64, 2.0, False, (48, 5, 300))
    for bad in (False, True):       # the NaN case on an optimizer of its own
        rig = Rig(sc, dev)
        sa = rig.slotted()
        if bad:
            rig.A[1].views[2][7] = float("nan")
        seg = torch.tensor([0, 1, 2, 3, 1, 1, 1], dtype=torch.int64, device=dev)
        sa.step(seg, 2.0)
        torch.cuda.synchronize()
        total, scale = float(sa.total.cpu()), sa.scale.cpu().numpy()
        if bad:
            assert np.isnan(total) and np.isnan(scale[0]) and np.isnan(scale[1])     # documented passthrough
        else:
            assert total == 0.0 and scale[0] == 0.0 and scale[1] == 1.0


# ------------------------------------------------------------------------------------------------ e. segment maps
def test_segment_maps_one_pass_two_passes_and_dense(dev):
    """Mapped tensors (one whose tail chunk ends in the one-vector loop) beside unmapped ones over 8 steps of
    adam_ref.segmap_scenario's touch patterns, one step skipped: the mapped update in one pass, as step_early +
    step(phase=2), and with segmaps=None are bitwise equal and within the bound of the float64 model; afterwards now
    is clear, ever is the model's, the gradients are zero and never-touched segments hold the initial p, m = v = 0.
    A mapped tensor in the weight-decay group, or with numel % 16 != 0, takes the dense path and still matches."""
    sc, traj, bound = _reference("segmap_scenario")
    runs = {}
    for mode in ("one", "two", "dense"):
        rig = Rig(sc, dev)
        sa = rig.slotted(segmaps=mode != "dense")
        assert (sa.segmaps is not None) == (mode != "dense")
        if mode != "dense":
            host = sa.segmaps.cpu().view(-1, 2)
            for i, spec in enumerate(sc.specs):      # rows are in group order: find each tensor's row by pointer
                row = [r for r, x in enumerate(sa.rows) if x[0] is rig.params[i]][0]
                assert bool(host[row, 0]) == traj[0]["t"][i]["mapped"], (i, spec)
        runs[mode] = _run_slotted(rig, sa, split=mode == "two")
    worst = None
    for mode, snaps in runs.items():
        w = _check_slotted(sc, traj, bound, snaps, mode)
        worst = w if worst is None else [max(a, b) for a, b in zip(worst, w)]
    for j, ref in enumerate(traj):
        a = runs["one"][j]
        for mode in ("two", "dense"):
            for q in "pmvg":
                for i, (x, y) in enumerate(zip(a[q], runs[mode][j][q])):
                    assert np.array_equal(x, y), (mode, j, q, i)
            assert a["total"] == runs[mode][j]["total"]
        for mode in ("one", "two"):
            s = runs[mode][j]
            for i, t in enumerate(ref["t"]):
                if not t["mapped"]:
                    continue
                assert not s["now"][i].any() and np.array_equal(s["ever"][i], t["ever"]), (mode, j, i)
                assert not s["g"][i].any()
                never = np.repeat(t["ever"] == 0, R.SEG)
                assert never.any() or sc.specs[i][0] < 128
                assert np.array_equal(s["p"][i][never], sc.p0[i][never])
                assert not s["m"][i][never].any() and not s["v"][i][never].any()
    print(f"segment maps: worst p {worst[0]:.2f} m {worst[1]:.2f} v {worst[2]:.2f} units "
          f"(bounds {bound[0]:.1f} {bound[1]:.1f} {bound[2]:.1f})")


def test_routed_step_never_splits_the_update_under_amp(monkeypatch):
    """found_inf is known only after the early pass would have run (and bumped the counters): RoutedAdaptStep does
    not take the split update with an AmpScaler, even when the split update is asked for and segment maps exist.
    This is the guard."""
    from test_amp import _c5_step
    from adaptive_city_nerf_amd import routed_train as RT
    monkeypatch.setattr(RT, "ADAM_EARLY", True)
    monkeypatch.setattr(RT, "ADAM_SEGMAP", True)
    _, _, st = _c5_step(True)
    assert st.amp is not None and st.segmaps is not None and st.adam.segmaps is not None and st.early is False


# ------------------------------------------------------------------------------------------------ f. AmpScaler
@pytest.mark.parametrize("case", range(len(R.AMP_CASES)))
def test_amp_unscale_coef_against_the_gradscaler_rule(dev, case):
    from adaptive_city_nerf_amd import optim as O
    c = R.AMP_CASES[case]
    growth, backoff, interval = c.get("growth", 2.0), c.get("backoff", 0.5), c.get("interval", 2000)
    want = R.amp_rule(c["total"], c["max_norm"], c["scale"], c["tracker"], growth, backoff, interval)
    amp = O.AmpScaler(dev, c["scale"], growth, backoff, interval)
    amp.tracker.fill_(c["tracker"])
    K = 2
    seg = torch.tensor([0, 3, 5, 3, 2], dtype=torch.int64, device=dev)
    out = torch.full((2,), -7.0, device=dev)
    amp.unscale_coef(torch.tensor([c["total"]], dtype=torch.float64, device=dev), c["max_norm"], out, seg, K)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for a, b in zip(got, (want["norm"], want["mult"])):
        assert (np.isnan(a) and np.isnan(b)) or a == b, (got, want)
    assert amp.found_inf() == want["found"]
    assert amp.get_scale() == float(want["scale"]) and int(amp.tracker) == want["tracker"]
    assert seg.tolist() == [0, 3, -1 if want["skip"] else 5, 3, 2]


def test_slotted_adam_under_a_power_of_two_loss_scale_is_bitwise_the_unscaled_step(dev):
    """Gradients (and table_sumsq) times 2^10 with an AmpScaler at 2^10 against the plain clipped step: the
    multiplier coef / scale and every product with it are exact, so the result is bitwise the same."""
    from adaptive_city_nerf_amd import optim as O
    sc, traj, bound = _reference("slotted_scenario", 64, 40.0, True)
    rig = Rig(sc, dev)
    plain = _run_slotted(rig, rig.slotted())
    rig = Rig(sc, dev)
    amp = O.AmpScaler(dev, init_scale=2.0 ** 10)
    scaled = _run_slotted(rig, rig.slotted(), amp=amp, gmul=2.0 ** 10)
    for j, (a, b) in enumerate(zip(plain, scaled)):
        for q in "pmv":
            for i, (x, y) in enumerate(zip(a[q], b[q])):
                assert np.array_equal(x, y), (j, q, i)
        assert a["counters"] == b["counters"]
        assert b["seg"][sc.K] == (-1 if sc.steps[j].get("skip") else sum(sc.steps[j]["counts"]))
        assert a["scale"][0] == b["scale"][0] and b["scale"][1] == a["scale"][1] / np.float32(1024.0)
    assert amp.get_scale() == 1024.0 and int(amp.tracker) == len(sc.steps) and not amp.found_inf()
    _check_slotted(sc, traj, bound, [dict(s, g=[g / np.float32(1024.0) for g in s["g"]]) for s in scaled], "amp")
