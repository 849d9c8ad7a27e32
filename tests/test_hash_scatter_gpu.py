"""The hash grid's table-gradient scatters against the float64 reference of hash_scatter_ref.

Dyadic inputs (points j / 2^B, power-of-two resolutions, small integer gradients) make every partial sum of a row
an fp32 number in any order and grouping: each such case first asserts from the reference that EVERY row is
provably exact (hash_scatter_ref.exact_rows) and then that the kernel equals the float64 sums bit for bit -- one
lost, doubled or misplaced contribution of any size fails.  Generic float inputs must stay within the derived row
bound tol_row = (16 + n_row) * 2^-24 * A_row, with exact zeros where nothing contributes.  test_hash_scatter_cpu
shows that mutations of an fp32 scatter fail both checks.

Reached here (16 points per lane stretch; the standalone scatter merges 6 levels, the pair list none):
  acn_hashgrid_bwd, F = 2, Linear / Smoothstep: hashgrid_bwd_merge (levels 0..5: chunk edges 2^8..2^12, the item
      loop past 1024 items, the crowded-LDS fallback, zero sums at the flush, 64-B segments spanning levels at
      log2T < 3) and hashgrid_bwd_rle (levels >= 6: runs across the 16-point stretch and the 64-point wave);
  acn_hashgrid_bwd, F != 2 or Nearest: hashgrid_bwd_gen;
  acn_hashgrid_bwd_pairs / _sumsq / _segmap and acn_hashgrid_pairs_mark: hashgrid_bwd_pairs plain, TELE and
      MARK_ONLY (padding, seg[K] below the capacity, runs across expert boundaries, the grid-stride loop, the
      telescoped sum of squares, the segment maps).
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import hash_scatter_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@lru_cache(maxsize=None)
def _dyadic(interp, M, L=8, log2T=14, F=2, repeat=False, B=None):
    """(case, reference) of a dyadic case, every row provably exact (asserted before any kernel runs)."""
    c = R.dyadic_case(interp, M, L=L, log2T=log2T, F=F, repeat=repeat, B=B)
    ref = R.scatter_ref(c.x01, c.gout, c.res, c.log2T, c.F, c.interp)[0]
    _assert_all_exact(c, ref.A)
    return c, ref


def _assert_all_exact(c, A):
    ok = R.exact_rows(A, R.row_granule(c.res, c.B, c.interp, c.log2T))
    assert ok.all(), f"{(~ok).sum()} of {ok.size} rows not provably exact (max A {A.max()})"


def _bwd(c, out=None):
    from adaptive_city_nerf_amd import ops
    got = ops.hashgrid_bwd(_t(c.x01), _t(c.gout), c.res, c.log2T, c.F, c.interp, deterministic=False, out=out)
    return got.cpu().numpy()


def _assert_within(got, ref):
    tol = R.tol_row(ref)
    err = np.abs(got.astype(np.float64) - ref.grad)
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} elements over the row bound, worst error / bound " \
                          f"{np.max(err[bad] / tol[bad]):.3g}"
    assert np.all(got[ref.A == 0] == 0)


# ------------------------------------------------------------------------------------- acn_hashgrid_bwd, F = 2
@pytest.mark.parametrize("M", [1, 15, 17, 63, 65, 255, 257, 4095, 4097, 8200])
@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_dyadic_bit_exact(interp, M):
    """Point counts at the lane stretch (16), the wave (64) and the merge chunks (2^8 .. 2^12)."""
    c, ref = _dyadic(interp, M)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_dyadic_merge_item_loop(interp):
    """M = 100003, L = 8: more merge items than the 1024 workgroups of hashgrid_bwd_merge's grid."""
    c, ref = _dyadic(interp, 100003)
    items = sum(-(-100003 // (1 << lg)) for lg in (12, 11, 10, 9, 8, 8))
    assert items > 1024
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("M", [1000, 8200])
@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_dyadic_repeated_runs(interp, M):
    """Every point repeated 1..40 times in a row: runs inside and across the 16-point stretches and the waves."""
    c, ref = _dyadic(interp, M, repeat=True)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_crowded_chunk_falls_back_to_direct_atomics(interp):
    """Uniform points at a fine level 0: its first 4096-point chunk touches more 64-B segments than the 1024
    entries of the LDS table, so part of the chunk takes hashgrid_bwd_merge's direct-atomic fallback."""
    c, ref = _dyadic(interp, 8200)
    assert R.chunk_segments(c.x01[:4096], c.res[0], c.log2T, interp) > 1024
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("L", [1, 5, 6, 7, 16])
@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_dyadic_level_counts(interp, L):
    """Only merged levels (L <= 6), the first run-merge level (7), and both kernels at the reference's L = 16."""
    c, ref = _dyadic(interp, 1031, L=L, repeat=True)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("log2T", [1, 2, 3])
@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_dyadic_tiny_tables(interp, log2T):
    """Below log2T = 3 a 64-B segment of the merge kernel's LDS table spans levels."""
    c, ref = _dyadic(interp, 4097, log2T=log2T)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)
    c, ref = _dyadic(interp, 300, log2T=log2T, repeat=True)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_accumulates_into_out(interp):
    """out= pre-filled with integers ends as init + grad exactly (the sums stay exact: |init| + A is bounded)."""
    c, ref = _dyadic(interp, 4097, repeat=True)
    init = R.int_table(ref.grad.shape[0], 2, 8, np.random.default_rng(2))
    _assert_all_exact(c, ref.A + np.abs(init))
    out = _t(init)
    got = _bwd(c, out=out)
    np.testing.assert_array_equal(got.astype(np.float64), init + ref.grad)
    np.testing.assert_array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("kind,M,log2T", [("uniform", 8200, 10), ("rays", 8200, 12), ("same", 1000, 12),
                                          ("uniform", 257, 14)])
@pytest.mark.parametrize("interp", [1, 2])
def test_standalone_generic_within_row_bound(interp, kind, M, log2T):
    c = R.generic_case(interp, M, L=8, log2T=log2T, kind=kind)
    ref = R.scatter_ref(c.x01, c.gout, c.res, c.log2T, 2, interp)[0]
    _assert_within(_bwd(c), ref)


# ----------------------------------------------------------------------------------------------- hashgrid_bwd_gen
GEN = [(F, i) for F in (1, 3, 4, 8) for i in (0, 1, 2)] + [(2, 0)]


@pytest.mark.parametrize("F,interp", GEN)
def test_generic_kernel_dyadic_bit_exact(F, interp):
    c, ref = _dyadic(interp, 1031, L=7, log2T=10, F=F, repeat=True)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)
    c, ref = _dyadic(interp, 257, L=3, log2T=14, F=F)
    np.testing.assert_array_equal(_bwd(c).astype(np.float64), ref.grad)


@pytest.mark.parametrize("F,interp", GEN)
def test_generic_kernel_within_row_bound(F, interp):
    c = R.generic_case(interp, 3001, L=7, log2T=10, F=F, kind="rays")
    ref = R.scatter_ref(c.x01, c.gout, c.res, c.log2T, F, interp)[0]
    _assert_within(_bwd(c), ref)


# --------------------------------------------------------------------------------------------------- the pair list
COUNTS = [(700, 0, 1301), (1, 63, 65), (17, 16, 15), (1500,)]
# points j / 2^B of the telescoped-norm cases: Smoothstep keeps one fraction bit (granule 2^-6 instead of 2^-15), so
# that hash_scatter_ref.tele_exact holds; Linear keeps the default widths
TELE_B = {1: None, 2: 7}


@lru_cache(maxsize=None)
def _pairs_case(interp, counts, L=8, log2T=14, B=None, repeat=True):
    """(case, pair list, per-expert references, per-expert integer init tables), every row provably exact when
    the tables start from init."""
    rng = np.random.default_rng([interp, L, log2T, B or 0] + list(counts))
    c = R.dyadic_case(interp, sum(counts), L=L, log2T=log2T, repeat=repeat, B=B)
    p = R.pair_list(counts, c.x01, c.gout, rng)
    assert p.x01.shape[0] > p.live and (p.pidx[:p.live] < 0).any()
    refs = R.scatter_ref(p.x01, p.gout, c.res, log2T, 2, interp, pk=p.pk, pidx=p.pidx, live=p.live, K=p.K)
    inits = [R.int_table(L << log2T, 2, 8, rng) for _ in range(p.K)]
    for ref, init in zip(refs, inits):
        _assert_all_exact(c, ref.A + np.abs(init))
    return c, p, refs, inits


def _call_pairs(entry, c, p, tables, sumsq=None, maps=None):
    from adaptive_city_nerf_amd import _lib
    from adaptive_city_nerf_amd._lib import check, ptr
    L = len(c.res)
    dev = [_t(a) for a in (p.x01, p.pk, p.pidx, p.seg, p.gout)]
    x01, pk, pidx, seg, gout = dev
    rp = (C.c_int32 * L)(*c.res)
    tp = (C.c_void_p * p.K)(*[t.data_ptr() for t in tables]) if tables is not None else None
    mp = (C.c_void_p * p.K)(*[m.data_ptr() for m in maps]) if maps is not None else None
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    head = (ptr(x01), ptr(pk), ptr(pidx), ptr(seg), p.K)
    if entry == "plain":
        rc = lib.acn_hashgrid_bwd_pairs(*head, ptr(gout), tp, rp, L, c.log2T, c.interp, s)
    elif entry == "sumsq":
        rc = lib.acn_hashgrid_bwd_pairs_sumsq(*head, ptr(gout), tp, rp, L, c.log2T, c.interp, ptr(sumsq), s)
    elif entry == "segmap":
        rc = lib.acn_hashgrid_bwd_pairs_segmap(*head, ptr(gout), tp, rp, L, c.log2T, c.interp,
                                               ptr(sumsq) if sumsq is not None else None, mp, s)
    else:
        rc = lib.acn_hashgrid_pairs_mark(*head, rp, L, c.log2T, c.interp, mp, s)
    check(rc, entry)
    torch.cuda.synchronize()


SENTINEL = 0xA5


def _maps(refs, sentinel):
    return [torch.full((r.touched.size,), sentinel, dtype=torch.uint8, device=DEV) for r in refs]


def _assert_maps(maps, refs, sentinel):
    for k, (m, r) in enumerate(zip(maps, refs)):
        np.testing.assert_array_equal(m.cpu().numpy(), np.where(r.touched == 1, 1, sentinel).astype(np.uint8),
                                      err_msg=f"segment map of expert {k}")


@pytest.mark.parametrize("entry", ["plain", "sumsq", "segmap", "segmap_tele"])
@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("interp", [1, 2])
def test_pairs_dyadic_bit_exact(interp, counts, entry):
    """Every expert's table ends as init + grad exactly through acn_hashgrid_bwd_pairs, _sumsq and _segmap
    (without and with the telescoped norm), from integer-filled tables, with a NaN tail past seg[K], NaN padding
    slots and runs across the expert boundaries.  The segment maps, started from a sentinel pattern, hold 1 exactly
    where the reference marks a corner row (zero-weight corners included) and keep the sentinel elsewhere.

    The telescoped double, started at 3.0, gains exactly sum(final^2) - sum(init^2) in float64: the tables are
    pre-filled, so every row telescopes to final^2 - init^2, not to final^2.  hash_scatter_ref.tele_exact confirms
    from the reference that every square, difference and partial sum is an exact double."""
    tele = entry in ("sumsq", "segmap_tele")
    c, p, refs, inits = _pairs_case(interp, counts, B=TELE_B[interp] if tele else None)
    tables = [_t(i) for i in inits]
    sq = torch.full((1,), 3.0, dtype=torch.float64, device=DEV) if tele else None
    maps = _maps(refs, SENTINEL) if entry.startswith("segmap") else None
    if tele:
        gmin = float(R.level_granule(c.res, c.B, interp).min())
        assert R.tele_exact(np.concatenate([r.A for r in refs]), np.concatenate(inits), gmin, s0=3.0)
    _call_pairs(entry.split("_")[0], c, p, tables, sq, maps)
    for k in range(p.K):
        np.testing.assert_array_equal(tables[k].cpu().numpy().astype(np.float64), inits[k] + refs[k].grad,
                                      err_msg=f"expert {k}")
    if tele:
        gain = sum(float(np.sum((i + r.grad) ** 2) - np.sum(i.astype(np.float64) ** 2))
                   for i, r in zip(inits, refs))
        assert float(sq.item()) == 3.0 + gain
    if maps is not None:
        _assert_maps(maps, refs, SENTINEL)


@pytest.mark.parametrize("entry", ["plain", "segmap_tele"])
def test_pairs_grid_stride_loop(entry):
    """L = 16, 33003 live slots: 8256 waves of work for the 8192 waves of the fixed grid."""
    counts = (20001, 13002)
    assert -(-sum(counts) // 64) * 16 > 2048 * 4
    c, p, refs, inits = _pairs_case(1, counts, L=16, log2T=14, B=8, repeat=False)
    tables = [_t(i) for i in inits]
    tele = entry != "plain"
    sq = torch.zeros(1, dtype=torch.float64, device=DEV) if tele else None
    maps = _maps(refs, 0) if tele else None
    if tele:
        gmin = float(R.level_granule(c.res, c.B, 1).min())
        assert R.tele_exact(np.concatenate([r.A for r in refs]), np.concatenate(inits), gmin)
    _call_pairs(entry.split("_")[0], c, p, tables, sq, maps)
    for k in range(p.K):
        np.testing.assert_array_equal(tables[k].cpu().numpy().astype(np.float64), inits[k] + refs[k].grad)
    if tele:
        gain = sum(float(np.sum((i + r.grad) ** 2) - np.sum(i.astype(np.float64) ** 2))
                   for i, r in zip(inits, refs))
        assert float(sq.item()) == gain
        _assert_maps(maps, refs, 0)


@pytest.mark.parametrize("sentinel", [0, SENTINEL])
@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("interp", [1, 2])
def test_pairs_mark_sets_exactly_the_touched_segments(interp, counts, sentinel):
    """acn_hashgrid_pairs_mark from zeroed maps and from a sentinel pattern: 1 where the reference marks, the
    starting byte elsewhere; the gradient tables and a sentinel in table_sumsq stay as they were."""
    c, p, refs, inits = _pairs_case(interp, counts)
    tables = [_t(i) for i in inits]
    sq = torch.full((1,), -7.25, dtype=torch.float64, device=DEV)
    maps = _maps(refs, sentinel)
    _call_pairs("mark", c, p, None, None, maps)
    _assert_maps(maps, refs, sentinel)
    for t, i in zip(tables, inits):
        np.testing.assert_array_equal(t.cpu().numpy(), i)
    assert float(sq.item()) == -7.25


@pytest.mark.parametrize("interp", [1, 2])
def test_pairs_segmap_from_zeros(interp):
    c, p, refs, inits = _pairs_case(interp, COUNTS[0])
    tables = [torch.zeros(i.shape, device=DEV) for i in inits]
    maps = _maps(refs, 0)
    _call_pairs("segmap", c, p, tables, None, maps)
    _assert_maps(maps, refs, 0)
    for k in range(p.K):
        np.testing.assert_array_equal(tables[k].cpu().numpy().astype(np.float64), refs[k].grad)


@pytest.mark.parametrize("interp", [1, 2])
def test_pairs_generic_within_row_bound_and_telescoped_norm(interp):
    """Generic float inputs through acn_hashgrid_bwd_pairs_sumsq from zeroed tables: every row within tol_row,
    exact zeros where nothing contributes, and the telescoped double within sum(2 |ref| tol + tol^2) of the
    float64 sum of squares of the reference (|got^2 - ref^2| <= 2 |ref| |got - ref| + |got - ref|^2 per
    element)."""
    counts = (700, 0, 1301)
    rng = np.random.default_rng(17 + interp)
    c = R.generic_case(interp, sum(counts), L=8, log2T=10, kind="rays")
    p = R.pair_list(counts, c.x01, c.gout, rng)
    refs = R.scatter_ref(p.x01, p.gout, c.res, 10, 2, interp, pk=p.pk, pidx=p.pidx, live=p.live, K=3)
    tables = [torch.zeros(8 << 10, 2, device=DEV) for _ in range(3)]
    sq = torch.zeros(1, dtype=torch.float64, device=DEV)
    _call_pairs("sumsq", c, p, tables, sq)
    want = allowed = 0.0
    for t, ref in zip(tables, refs):
        _assert_within(t.cpu().numpy(), ref)
        tol = R.tol_row(ref)
        want += float(np.sum(ref.grad ** 2))
        allowed += float(np.sum(2.0 * np.abs(ref.grad) * tol + tol * tol))
    assert want > 0 and abs(float(sq.item()) - want) <= allowed


def test_pairs_mark_with_adjacent_maps_across_an_expert_boundary():
    """The experts' maps as the routed step lays them out, one (K, 2, segments) buffer.  acn_hashgrid_pairs_mark has
    no gradient tables to tell its runs apart by, so two consecutive slots of different experts whose rows differ
    by (distance of the maps) / 8 must still count as two runs: the second expert's segment is marked as well."""
    L, log2T, interp = 16, 10, 1
    T = 1 << log2T
    maps = torch.zeros(2, 2, L * T // 8, dtype=torch.uint8, device=DEV)
    D = (maps[1, 0].data_ptr() - maps[0, 0].data_ptr()) // 8
    assert 0 < D < T
    c = R.dyadic_case(interp, 4096, L=L, log2T=log2T)
    rows, _ = R.cells(c.x01, c.res, log2T, interp)
    first = {}
    for i, r in enumerate(rows[:, 0, 0]):
        first.setdefault(int(r), i)
    pick = None
    for i, r in enumerate(rows[:, 0, 0]):        # slot of expert 0 at row r, slot of expert 1 at row r - D
        j = first.get(int(r) - D)
        if j is not None:
            others = np.delete(np.arange(L * 8) // 8 * T + rows[j].reshape(-1), 0) >> 3
            if (int(r) - D) >> 3 not in others:  # no other corner or level of that slot marks the same byte
                pick = (i, j)
                break
    assert pick is not None
    x = np.concatenate([c.x01[:4], c.x01[[pick[0]]], c.x01[[pick[1]]]])
    p = R.pair_list((5, 1), x, np.zeros((6, 2 * L), np.float32), np.random.default_rng(0), pad_frac=0.0)
    x2 = p.x01.copy()
    x2[3:6] = x[3:6]                              # pair_list repeats a point around the boundary: not here
    p = p._replace(x01=x2)
    refs = R.scatter_ref(p.x01, p.gout, c.res, log2T, 2, interp, pk=p.pk, pidx=p.pidx, live=p.live, K=2)
    _call_pairs("mark", c, p, None, None, [maps[0, 0], maps[1, 0]])
    _assert_maps([maps[0, 0], maps[1, 0]], refs, 0)
    assert not maps[:, 1].any()
