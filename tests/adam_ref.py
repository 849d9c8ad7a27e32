"""Reference for the optimizer kernels of csrc/optim.hip (numpy only, nothing imported from the package).

adam_step64   torch.optim.Adam's _single_tensor_adam in float64, its scalar constants cast to fp32 exactly where the
              kernels' host code casts them, so it differs from a kernel only by the fp32 rounding of the element
              arithmetic.  The oracle of tests/test_optim_gpu.py.
adam_step32   the kernels' operation order in numpy float32 (each fma a float64 multiply-add rounded once).  No
              oracle: the yardstick that sizes the GPU tolerances (units()), and the place the planted mistakes of
              tests/test_optim_cpu.py are applied.
Model         the slotted optimizer from its documented contract: per-slot activity and step counters, the constant
              table's range, the skipped step and what it clears, ZERO_GRAD / NORM_ELSEWHERE, and the (now, ever)
              segment maps in one pass or as the early / late pair of passes.
norm_total, clip_coef32, amp_rule   the clip norm in float64, clip_grad_norm_'s fp32 coefficient, GradScaler's
              unscale / found_inf / backoff / growth.
make_case, the scenario builders    deterministic inputs whose effective gradients are exactly 0 or >= 1e-3 of the
              step's largest, which is what lets every element be compared with no excluded fraction.
"""
import math

import numpy as np

EPS32 = 2.0 ** -24
CHUNK, SEG = 65536, 16
ZERO_GRAD, NORM_ELSEWHERE = 1 << 16, 1 << 17
FLOOR = 1e-3

UNMAPPED = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 65536 + 4096 + 4 * 256 + 7]
MAPPED = [16, 48, 4096, 4096 + 16, 65536, 65536 + 4096 + 16 * 5]

MISTAKES32 = ("row_off_by_one", "bc2s_not_sqrt", "wd_after_moments", "clip_on_wd")
MISTAKES_MODEL = ("inactive_decays", "ever_not_now_skipped", "tail_vector_not_updated", "grad_not_cleared",
                  "ever_not_set")


def hparams(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


def consts(hp, step, exact=False, mistake=None):
    """The scalars of _single_tensor_adam at `step` (python floats = double), cast to fp32 where they meet tensors
    (exact=True keeps the doubles: torch's own float64 run)."""
    if mistake == "row_off_by_one":
        step = step + 1
    b1, b2 = hp["betas"]
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    c = dict(lr_neg_step=-(hp["lr"] / bc1), w1=1.0 - b1, beta2=b2, one_m_beta2=1.0 - b2,
             bc2s=bc2 if mistake == "bc2s_not_sqrt" else math.sqrt(bc2), eps=hp["eps"], wd=hp["weight_decay"])
    return c if exact else {k: float(np.float32(v)) for k, v in c.items()}


def adam_step64(p, g, m, v, hp, step, scale=1.0, exact=False, mistake=None, stats=None):
    """One Adam step in float64; returns (p, m, v), the inputs untouched.  `scale` multiplies the raw gradient only
    (the clip coefficient, or coefficient / loss scale).  stats (a dict) collects the effective gradient's range."""
    k = consts(hp, step, exact, mistake)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * float(scale)
    if k["wd"] != 0.0:
        g = g + k["wd"] * p
    if stats is not None:
        a = np.abs(g)
        stats["gmax"] = max(stats.get("gmax", 0.0), float(a.max(initial=0.0)))
        nz = a[a != 0]
        if nz.size:
            stats["gmin"] = min(stats.get("gmin", math.inf), float(nz.min()))
    m = m + k["w1"] * (g - m)                      # lerp
    v = v * k["beta2"] + k["one_m_beta2"] * g * g
    denom = np.sqrt(v) / k["bc2s"] + k["eps"]
    p = p + k["lr_neg_step"] * m / denom
    return p, m, v


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam_step32(p, g, m, v, hp, step, scale=1.0, exact=False, mistake=None, stats=None):
    """adam_elem's operation order in float32 (see the module docstring); `mistake` plants one of MISTAKES32."""
    k = {n: np.float32(x) for n, x in consts(hp, step, False, mistake).items()}
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    sc = np.float32(scale)
    if mistake == "clip_on_wd":
        g = _fma32(k["wd"], p, g) * sc if k["wd"] != 0 else g * sc
    else:
        g = g * sc
        if k["wd"] != 0 and mistake != "wd_after_moments":
            g = _fma32(k["wd"], p, g)
    m = _fma32(k["w1"], g - m, m)
    v = v * k["beta2"]
    v = v + (k["one_m_beta2"] * g) * g
    denom = np.sqrt(v) / k["bc2s"] + k["eps"]
    if mistake == "wd_after_moments" and k["wd"] != 0:
        p = _fma32(-k["wd"] * np.float32(hp["lr"]), p, p)
    p = p + (k["lr_neg_step"] * m) / denom
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


# ------------------------------------------------------------------------------------------------ norm and scalers
def norm_total(grads, extra=0.0):
    """Sum of squares in float64 of a list of gradient arrays, plus a sum supplied from elsewhere."""
    return float(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads) + extra)


def clip_coef32(total, max_norm):
    """clip_grad_norm_'s (norm, coefficient) in fp32: max_norm / (norm + 1e-6) clamped to <= 1, NaN passing."""
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(np.float64(total)))
        coef = np.float32(max_norm) / (norm + np.float32(1e-6))
        coef = np.float32(1.0) if coef > 1.0 else coef
    return norm, coef


def amp_rule(total, max_norm, scale, tracker, growth=2.0, backoff=0.5, interval=2000):
    """GradScaler's unscale_ + clip_grad_norm_ + step-skip + update() on the squared norm of the scaled gradients.
    Returns dict(norm, mult, found, scale, tracker, skip): `mult` is what the gradients in memory are multiplied
    by (clip coefficient / scale)."""
    with np.errstate(all="ignore"):
        scale = np.float32(scale)
        inv = np.float32(1.0 / np.float64(scale))
        norm = np.float32(np.sqrt(np.float64(total))) * inv
        found = bool(np.isnan(norm) or np.isinf(norm))
        coef = np.float32(1.0)
        if max_norm is not None and max_norm > 0:
            coef = np.float32(max_norm) / (norm + np.float32(1e-6))
            coef = np.float32(1.0) if coef > 1.0 else coef
        new_scale, new_tracker = scale, tracker
        if found:
            new_scale, new_tracker = scale * np.float32(backoff), 0
        else:
            new_tracker = tracker + 1
            if new_tracker == interval:
                grown = scale * np.float32(growth)
                new_scale = grown if np.isfinite(grown) else scale
                new_tracker = 0
    return dict(norm=norm, mult=np.float32(coef * inv), found=found, scale=np.float32(new_scale), tracker=new_tracker,
                skip=found)


AMP_CASES = [
    # finite, clipped and not; inf and NaN totals; tracker one short of the interval; growth that would overflow
    dict(total=4.0 * 1024 ** 2, max_norm=None, scale=1024.0, tracker=0),
    dict(total=4.0 * 1024 ** 2, max_norm=1.0, scale=1024.0, tracker=0),
    dict(total=1e-4, max_norm=1.0, scale=1024.0, tracker=5),
    dict(total=math.inf, max_norm=1.0, scale=1024.0, tracker=7),
    dict(total=math.nan, max_norm=None, scale=1024.0, tracker=7),
    dict(total=9.0, max_norm=1.0, scale=65536.0, tracker=3, interval=4),
    dict(total=9.0, max_norm=None, scale=2.0 ** 127, tracker=3, interval=4),
    dict(total=9.0, max_norm=None, scale=8.0, tracker=0, interval=1, growth=3.0, backoff=0.25),
    dict(total=math.inf, max_norm=None, scale=8.0, tracker=0, interval=1, growth=3.0, backoff=0.25),
]


# ------------------------------------------------------------------------------------------------ the slotted model
class T:
    """One tensor of the model: arrays p, g, m, v, its slot, group and flag bits, optional (now, ever) byte maps."""

    def __init__(self, p, m, v, slot=0, group=0, flags=0, mapped=False, dtype=np.float64):
        self.n = len(p)
        self.p, self.m, self.v = (np.array(a, dtype) for a in (p, m, v))
        self.g = np.zeros(self.n, dtype)
        self.slot, self.group, self.flags = slot, group, flags
        nseg = (self.n + SEG - 1) // SEG
        self.now = np.zeros(nseg, np.uint8) if mapped else None
        self.ever = np.zeros(nseg, np.uint8) if mapped else None
        self.gmax = 0.0          # largest effective gradient this tensor has seen (the G of units())


class Model:
    """SlottedAdam's contract (adaptive_city_nerf_amd/optim.py, csrc/optim.hip comments).  K expert slots, active
    iff their count is > 0; slots >= K always active.  An inactive slot is untouched: parameters, moments, gradient,
    counter.  An active slot's counter goes up by one, and its tensors step with the constants of that count, unless
    the count is beyond the `table_steps` rows (then nothing is written).  A skipped step (skip=True, seg[K] < 0)
    moves nothing; ZERO_GRAD gradients are cleared (a mapped one only in its segments marked now) and now is reset.
    A tensor is segment-mapped when it has maps, its group has weight_decay 0 and its numel is a multiple of 16;
    otherwise it is updated densely and its maps are ignored.  Mapped: a segment is live when now | ever; a live
    segment not marked now takes a zero gradient; afterwards ever |= now, now = 0.  phase 1 updates only the segments
    with ever and not now (and bumps the counters), phase 2 the segments marked now and every dense tensor (no
    bump); phase 0 is both."""

    def __init__(self, tensors, hps, K, nslots, counters, table_steps, step_fn=adam_step64, use_maps=True,
                 mistake=None):
        self.t, self.hps, self.K, self.nslots = tensors, hps, K, nslots
        self.counters = list(counters)
        self.table_steps = table_steps
        self.step_fn, self.use_maps, self.mistake = step_fn, use_maps, mistake
        self.floor_ok = True

    def active(self, counts, skip):
        return [(not skip) and (s >= self.K or counts[s] > 0) for s in range(self.nslots)]

    def is_mapped(self, t):
        return self.use_maps and t.now is not None and self.hps[t.group]["weight_decay"] == 0.0 and t.n % SEG == 0

    def total(self, counts, skip, extra=0.0):
        act = self.active(counts, skip)
        return norm_total([t.g for t in self.t if act[t.slot] and not t.flags & NORM_ELSEWHERE], extra)

    def _update(self, t, idx, g, scale, step):
        """Adam on the elements idx (a slice or index array) with gradient g."""
        stats = {}
        m32 = self.mistake if self.mistake in MISTAKES32 else None
        p, m, v = self.step_fn(t.p[idx], g, t.m[idx], t.v[idx], self.hps[t.group], step, scale, mistake=m32,
                               stats=stats)
        t.p[idx], t.m[idx], t.v[idx] = p, m, v
        if stats:
            t.gmax = max(t.gmax, stats["gmax"])
            self.step_gmax = max(self.step_gmax, stats["gmax"])
            self.step_gmin = min(self.step_gmin, stats.get("gmin", math.inf))

    def step(self, counts, skip=False, scale=1.0, phase=0):
        self.step_gmax, self.step_gmin = 0.0, math.inf
        if skip:
            if phase != 1:
                for t in self.t:
                    if t.flags & ZERO_GRAD:
                        if self.is_mapped(t):
                            t.g[np.repeat(t.now != 0, SEG)[:t.n]] = 0
                            t.now[:] = 0
                        else:
                            t.g[:] = 0
            return
        act = self.active(counts, skip)
        if phase != 2:
            for s in range(self.nslots):
                if act[s]:
                    self.counters[s] += 1
        for t in self.t:
            if not act[t.slot]:
                if self.mistake == "inactive_decays":
                    self._update(t, slice(None), np.zeros(t.n), scale, max(self.counters[t.slot], 1))
                continue
            step = self.counters[t.slot]
            if step < 1 or step > self.table_steps:
                continue
            if not self.is_mapped(t):
                if phase == 1:
                    continue
                self._update(t, slice(None), t.g, scale, step)
                if t.flags & ZERO_GRAD and self.mistake != "grad_not_cleared":
                    t.g[:] = 0
                continue
            now, ever = t.now != 0, t.ever != 0
            live = {0: now | ever, 1: ever & ~now, 2: now}[phase]
            if self.mistake == "ever_not_now_skipped":
                live = live & now
            el = np.repeat(live, SEG)
            if self.mistake == "tail_vector_not_updated" and t.n % CHUNK:
                el[t.n - 4:] = False
            g = np.where(np.repeat(now, SEG), t.g, 0)
            idx = np.nonzero(el)[0]
            if idx.size:
                self._update(t, idx, g[idx], scale, step)
            if phase != 1:
                if t.flags & ZERO_GRAD and self.mistake != "grad_not_cleared":
                    t.g[np.repeat(now, SEG)] = 0
                if self.mistake != "ever_not_set":
                    t.ever[now] = 1
                t.now[:] = 0
        if self.step_gmin < FLOOR * self.step_gmax:
            self.floor_ok = False


def units(ref, lr):
    """The tolerance units of a reference tensor (float64 arrays): p: eps32 (|p| + lr); m: eps32 G; v: eps32 (v +
    G sqrt(v)), G the largest effective gradient the tensor has seen."""
    return (EPS32 * (np.abs(ref.p) + lr), EPS32 * ref.gmax * np.ones(ref.n),
            EPS32 * (ref.v + ref.gmax * np.sqrt(ref.v)))


def errors(got, ref, lr):
    """max over elements of |got - ref| in units(), for (p, m, v); got = three arrays.  A zero unit admits only a
    zero error."""
    out = []
    for a, r, u in zip(got, (ref.p, ref.m, ref.v), units(ref, lr)):
        e = np.abs(np.asarray(a, np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0, 0.0, e / u)
        out.append(float(q.max(initial=0.0)))
    return out


# ------------------------------------------------------------------------------------------------ inputs
def zero_mask(n):
    """Exact zeros on single lanes inside a live vector, on whole 16-B vectors and on whole 64-B segments."""
    i = np.arange(n)
    return ((i % 4 == 1) & ((i // 4) % 7 == 3)) | ((i // 4) % 5 == 2) | ((i // 16) % 3 == 1)


def make_case(n, scales, seed, wd=False):
    """p0 (float32) and one float32 gradient per entry of `scales`.  |g| / scale is in [0.5, 1] ('large') or
    [0.05, 0.1) ('small'), or exactly 0 on zero_mask(n) -- the same elements every step, so their whole history is
    zero.  With weight decay the zero elements also have p = 0 and every gradient has its parameter's sign (|p| in
    [0.15, 0.4], far more than the steps move it), so wd * p never cancels a gradient: the effective gradient
    g * scale + wd * p stays 0 or >= 1e-3 of the step's largest, which Model.step verifies on the reference."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], n)
    p = sign * rng.uniform(0.15, 0.4, n)
    z = zero_mask(n)
    grads = []
    for s in scales:
        small = rng.random(n) < 0.5
        u = np.where(small, rng.uniform(0.05, 0.1, n), rng.uniform(0.5, 1.0, n))
        sg = sign if wd else rng.choice([-1.0, 1.0], n)
        g = (sg * u * s).astype(np.float32)
        g[z] = 0
        if n >= 256:
            live = ~z
            assert (small & live).any() and (~small & live).any()
            v = z.reshape(-1, 4) if n % 4 == 0 else z[:n - n % 4].reshape(-1, 4)
            assert v.all(1).any() and (v.any(1) & ~v.all(1)).any()       # zero vectors and zero lanes
            if n >= 64:
                assert z[16:32].all()                                    # a zero segment
        grads.append(g)
    if wd:
        p[z] = 0
    return p.astype(np.float32), grads


class Scenario:
    """A list of tensor specs (n, slot, group, flags, mapped), the groups' hyper-parameters, and a list of steps:
    dict(counts, skip, gscale, touch={tensor: bool[nseg]}, extra).  inputs() are the float32 p0 / m0 / v0 and the
    per-step gradients; model() builds a Model over them."""

    def __init__(self, specs, hps, K, nslots, steps, start=None, max_steps=64, max_norm=None, seed=0):
        self.specs, self.hps, self.K, self.nslots, self.steps = specs, hps, K, nslots, steps
        self.start = [s if any(sp[1] == k for sp in specs) else 0      # a slot without tensors starts at 0
                      for k, s in enumerate(start or [0] * nslots)]
        self.table_steps = max(self.start) + max_steps
        self.max_steps, self.max_norm = max_steps, max_norm
        scales = [s["gscale"] for s in steps]
        self.p0, self.m0, self.v0, self.grads = [], [], [], []
        for i, (n, slot, group, flags, mapped) in enumerate(specs):
            wd = hps[group]["weight_decay"] != 0
            p, gs = make_case(n, scales, seed * 1000 + i, wd)
            rng = np.random.default_rng(seed * 1000 + 500 + i)
            if self.start[slot] > 0:   # a slot that has stepped before: moments of a plausible history
                m = (rng.uniform(-0.5, 0.5, n) * scales[0]).astype(np.float32)
                v = (rng.uniform(0.01, 0.3, n) * scales[0] ** 2).astype(np.float32)
                z = zero_mask(n)
                m[z], v[z] = 0, 0
            else:
                m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
            for j, st in enumerate(steps):
                tm = st.get("touch", {}).get(i)
                if mapped:
                    tm = np.zeros((n + SEG - 1) // SEG, bool) if tm is None else tm
                    gs[j] = np.where(np.repeat(tm, SEG)[:n], gs[j], np.float32(0))
            self.p0.append(p), self.m0.append(m), self.v0.append(v), self.grads.append(gs)

    def model(self, step_fn=adam_step64, use_maps=True, mistake=None):
        dt = np.float64 if step_fn is adam_step64 else np.float32
        ts = [T(self.p0[i], self.m0[i], self.v0[i], slot, group, flags, mapped, dt)
              for i, (n, slot, group, flags, mapped) in enumerate(self.specs)]
        for t in ts:
            if self.start[t.slot] > 0:
                t.gmax = self.steps[0]["gscale"]
        return Model(ts, self.hps, self.K, self.nslots, self.start, self.table_steps, step_fn, use_maps, mistake)

    def feed(self, model, j):
        """Step j's inputs into a model: the gradients of every tensor (a ZERO_GRAD buffer must have been cleared
        by the step before -- the caller's scatter adds into it) and the now marks of the mapped ones."""
        for i, t in enumerate(model.t):
            t.g[:] = self.grads[i][j]
            if t.now is not None:
                tm = self.steps[j].get("touch", {}).get(i)
                t.now[:] = 0 if tm is None else tm

    def scale_of(self, model, j):
        """The clip coefficient of step j on the model's current gradients (1.0 without max_norm)."""
        st = self.steps[j]
        if self.max_norm is None:
            return 1.0, None
        total = model.total(st["counts"], st.get("skip", False), st.get("extra", 0.0))
        return float(clip_coef32(total, self.max_norm)[1]), total

    def run(self, step_fn=adam_step64, use_maps=True, mistake=None, split=False, snapshot=None):
        """All steps on a fresh model; snapshot(j, model, total) after each.  split: phase 1 then phase 2."""
        mdl = self.model(step_fn, use_maps, mistake)
        for j, st in enumerate(self.steps):
            self.feed(mdl, j)
            scale, total = self.scale_of(mdl, j)
            skip = st.get("skip", False)
            if split:
                mdl.step(st["counts"], skip, 1.0, 1)
                mdl.step(st["counts"], skip, scale, 2)
            else:
                mdl.step(st["counts"], skip, scale, 0)
            if snapshot:
                snapshot(j, mdl, total)
        return mdl

    def yardstick(self, mistake=None, use_maps=True):
        """Worst error over all steps and tensors of the float32 emulation against the float64 model, in units()
        evaluated on the float64 model: (p, m, v).  With `mistake` planted in the float32 run it measures how far
        that mistake moves the compared quantities."""
        ref = self.model(adam_step64)
        emu = self.model(adam_step32, use_maps, mistake)
        worst = [0.0, 0.0, 0.0]
        extra = 0.0    # a wrong gradient, map or counter, in tolerance-free comparisons: counted as infinite
        for j, st in enumerate(self.steps):
            for mdl in (ref, emu):
                self.feed(mdl, j)
                if mistake == "grad_not_cleared" and mdl is emu and j > 0:
                    for i, t in enumerate(mdl.t):     # a ZERO_GRAD buffer is added into, not overwritten
                        if t.flags & ZERO_GRAD:
                            t.g[:] = self.grads[i][j] + self._left[i]
                scale, _ = self.scale_of(mdl, j)
                mdl.step(st["counts"], st.get("skip", False), scale, 0)
            self._left = [t.g.copy() for t in emu.t]
            lr = [self.hps[t.group]["lr"] for t in ref.t]
            for a, r, l in zip(emu.t, ref.t, lr):
                worst = [max(w, e) for w, e in zip(worst, errors((a.p, a.m, a.v), r, l))]
                if a.ever is not None and not np.array_equal(a.ever, r.ever):
                    extra = math.inf
            if emu.counters != ref.counters:
                extra = math.inf
        assert ref.floor_ok, "an effective gradient of the reference run is below the floor"
        return worst + [extra]


# ------------------------------------------------------------------------------------------------ the GPU scenarios
HPS2 = [hparams(0.01, (0.9, 0.999), 1e-8, 0.0), hparams(0.01, (0.5, 0.9), 1e-8, 0.01)]
GSCALES = [1.0, 0.1, 10.0, 100.0, 1.0, 3.0, 0.3, 30.0]


def plain_scenario(max_norm=None, sizes=None):
    """Case a: FusedAdam over the unmapped sizes, alternating between the two groups, 5 steps."""
    sizes = UNMAPPED if sizes is None else sizes
    specs = [(n, 0, i % 2, 0, False) for i, n in enumerate(sizes)]
    steps = [dict(counts=[], gscale=GSCALES[j]) for j in range(5)]
    return Scenario(specs, HPS2, 0, 1, steps, max_norm=max_norm, seed=1)


def slotted_scenario(max_steps=64, max_norm=40.0, elsewhere=False, sizes=None, nsteps=6):
    """Case c: K = 3 experts + one shared slot, two groups, ZERO_GRAD and plain tensors, slot 0 starting at step 4,
    slot 2 at 0; activity: one expert, none, all, a skipped step, all, two."""
    sizes = UNMAPPED if sizes is None else sizes
    specs = []
    for i, n in enumerate(sizes):
        flags = ZERO_GRAD if i % 3 != 2 else 0
        if elsewhere and i % 5 == 1:
            flags |= NORM_ELSEWHERE
        specs.append((n, i % 4, (i // 4) % 2, flags, False))
    acts = [dict(counts=[0, 1, 0]), dict(counts=[0, 0, 0]), dict(counts=[3, 1, 2]),
            dict(counts=[3, 1, 2], skip=True),
            dict(counts=[1, 1, 1]), dict(counts=[1, 0, 1])][:nsteps]
    steps = [dict(a, gscale=GSCALES[j], extra=(2500.0 * GSCALES[j] ** 2 if elsewhere else 0.0))
             for j, a in enumerate(acts)]
    return Scenario(specs, HPS2, 3, 4, steps, start=[4, 2, 0, 1], max_steps=max_steps, max_norm=max_norm, seed=2)


def segmap_scenario():
    """Case e: mapped tensors (group 0, ZERO_GRAD) beside unmapped ones, a mapped tensor in the weight-decay group
    and one whose numel is no multiple of 16 (both fall back to the dense update), 8 steps, one of them skipped.
    Per mapped tensor the segments are touched: never (s % 8 == 6, and s % 8 == 7 away from the edges); at step 0
    only (s % 8 == 0); at steps 2 and 3
    (s % 8 == 1); at step 7 only (s % 8 == 2); at step 5, after the skipped step 4 that also marked them (s % 8 ==
    3); every step (s % 8 == 4); the first and last segment of every chunk and of the tensor at steps 1 and 6.
    zero_mask puts an all-zero gradient on every third segment, touched or not."""
    specs = [(n, i % 2, 0, ZERO_GRAD, True) for i, n in enumerate(MAPPED)]
    specs += [(4096 + 16, 0, 1, ZERO_GRAD, True), (40, 1, 0, ZERO_GRAD, True), (1025, 2, 1, 0, False),
              (4097, 0, 0, ZERO_GRAD, False)]
    steps = []
    for j in range(8):
        touch = {}
        for i, (n, slot, group, flags, mapped) in enumerate(specs):
            if not mapped:
                continue
            nseg = (n + SEG - 1) // SEG
            s = np.arange(nseg)
            tm = (s % 8 == 4)
            tm |= (s % 8 == 0) & (j == 0)
            tm |= (s % 8 == 1) & (j in (2, 3))
            tm |= (s % 8 == 2) & (j == 7)
            tm |= (s % 8 == 3) & (j in (4, 5))
            if j in (1, 6):
                edge = np.zeros(nseg, bool)
                edge[[0, nseg - 1]] = True
                per = CHUNK // SEG
                edge[per - 1::per] = True
                edge[per::per] = True
                tm |= edge & (s % 8 != 6)
            if group == 1 or n % SEG:
                tm = np.ones(nseg, bool)     # the dense fallback reads the whole gradient
            touch[i] = tm
        steps.append(dict(counts=[1, 1], skip=(j == 4), gscale=GSCALES[j], touch=touch))
    return Scenario(specs, HPS2, 2, 3, steps, max_norm=25.0, seed=3)
