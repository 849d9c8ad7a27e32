// encoders.hip -- standalone HashGridEncoder and SHEncoder forward/backward (gfx950).
//
// Replaces models/encodings.py:331-381 (HashGridEncoder._torch_forward, _hash :308-316, _gather
// :318-329) and :133-151 (SHEncoder.forward), and their autograd in the table, the points and the
// directions.  One lane per (point, level): the L lanes of a
// point are adjacent, so the (M, L*F) output row of a point is written as one contiguous
// L*F*4-byte segment (128 B for the reference's L=16, F=2) and the point's x01 is a broadcast.
#include <type_traits>

#include "acn_device.h"
#include "acn_internal.h"

namespace {

struct Res32 {
    int32_t v[ACN_MAX_LEVELS];
};

// Smoothstep (INTERP == 2) replaces each lerp weight by S(w) = w^2 (3 - 2w); in this order, bit for bit
template <int INTERP>
__device__ __forceinline__ void smooth_weights(float& wx, float& wy, float& wz) {
    if (INTERP == 2) {
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
}

// The F == 2 gathers of tables up to 2 GiB go through one buffer resource over the whole table (32-bit offsets)
inline bool table_fits_buffer(int L, int log2T) { return ((uint64_t)L << (log2T + 3)) <= (1ull << 31); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t table_rsrc(const float2* table, int L, int log2T) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)table, (short)0, (int)((uint32_t)L << (log2T + 3)), 0x00020000);
}

template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_fwd_f2(const float* __restrict__ x01, int64_t M,
                                                       const float2* __restrict__ table, Res32 res,
                                                       int L, int log2T, float2* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = gid / L;
    const int l = (int)(gid - m * L);
    if (m >= M) return;
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const float2* tl = table + ((int64_t)l << log2T);
    float o0, o1;
    acn::hash_level_f2<INTERP>(tl, sx, sy, sz, mask, o0, o1);
    out[m * L + l] = make_float2(o0, o1);
}

// Linear / Smoothstep through a buffer resource over the whole table (the renders' gather form):
// 32-bit row offsets, and the x-neighbours of each (y, z) corner pair come from one 16-B block when x0 is even
// (hash_issue_x: 4 dwordx4 gathers, plus 4 dwordx2 only for odd x0).  The same rows and the same lerp chain as
// hash_level_f2, so the outputs are bitwise those of hashgrid_fwd_f2.  Tables up to 2 GiB (table_fits_buffer);
// hashgrid_fwd_f2 serves Nearest and the larger tables.
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_fwd_f2_buf(const float* __restrict__ x01, int64_t M,
                                                           const float2* __restrict__ table, Res32 res, int L,
                                                           int log2T, float2* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = gid / L;
    const int l = (int)(gid - m * L);
    if (m >= M) return;
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const __amdgpu_buffer_rsrc_t rs = table_rsrc(table, L, log2T);
    acn::HashPendingX p;
    acn::hash_issue_x<INTERP>(rs, (uint32_t)l << (log2T + 3), sx, sy, sz, mask, p);
    float o0, o1;
    acn::hash_finish_x<INTERP>(p, o0, o1);
    out[m * L + l] = make_float2(o0, o1);
}

// generic feature count (F != 2)
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_fwd_gen(const float* __restrict__ x01, int64_t M,
                                                        const float* __restrict__ table, Res32 res, int L,
                                                        int log2T, int F, float* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = gid / L;
    const int l = (int)(gid - m * L);
    if (m >= M) return;
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const float* tl = table + ((int64_t)l << log2T) * F;
    float* o = out + (m * L + l) * F;
    if (INTERP == 0) {
        const uint32_t ix = (uint32_t)(int)rintf(sx), iy = (uint32_t)(int)rintf(sy), iz = (uint32_t)(int)rintf(sz);
        const float* e = tl + (int64_t)((ix ^ (iy * acn::kP1) ^ (iz * acn::kP2)) & mask) * F;
        for (int f = 0; f < F; ++f) o[f] = e[f];
        return;
    }
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    smooth_weights<INTERP>(wx, wy, wz);
    const uint32_t x0 = (uint32_t)(int)fx, x1 = x0 + 1u;
    const uint32_t y0 = (uint32_t)(int)fy * acn::kP1, y1 = y0 + acn::kP1;
    const uint32_t z0 = (uint32_t)(int)fz * acn::kP2, z1 = z0 + acn::kP2;
    const float* c[8];
    c[0] = tl + (int64_t)((x0 ^ y0 ^ z0) & mask) * F;  // f000
    c[1] = tl + (int64_t)((x0 ^ y0 ^ z1) & mask) * F;  // f001
    c[2] = tl + (int64_t)((x0 ^ y1 ^ z0) & mask) * F;  // f010
    c[3] = tl + (int64_t)((x0 ^ y1 ^ z1) & mask) * F;  // f011
    c[4] = tl + (int64_t)((x1 ^ y0 ^ z0) & mask) * F;  // f100
    c[5] = tl + (int64_t)((x1 ^ y0 ^ z1) & mask) * F;  // f101
    c[6] = tl + (int64_t)((x1 ^ y1 ^ z0) & mask) * F;  // f110
    c[7] = tl + (int64_t)((x1 ^ y1 ^ z1) & mask) * F;  // f111
    const float ax = 1.0f - wx, ay = 1.0f - wy, az = 1.0f - wz;
    for (int f = 0; f < F; ++f) {
        const float c00 = c[0][f] * ax + c[4][f] * wx;
        const float c01 = c[1][f] * ax + c[5][f] * wx;
        const float c10 = c[2][f] * ax + c[6][f] * wx;
        const float c11 = c[3][f] * ax + c[7][f] * wx;
        const float c0 = c00 * ay + c10 * wy;
        const float c1 = c01 * ay + c11 * wy;
        o[f] = c0 * az + c1 * wz;
    }
}

// Backward: autograd of the 8 gathers + lerps.  The gradient of corner (bx,by,bz) is
// ((g * wz') * wy') * wx' in the chain-rule order of the forward lerps, scatter-added with
// no-return fp32 atomics (global_atomic_add_f32), as torch's index_put_(accumulate=True).
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_gen(const float* __restrict__ x01, int64_t M,
                                                        const float* __restrict__ gout, Res32 res, int L,
                                                        int log2T, int F, float* __restrict__ gtable) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = gid / L;
    const int l = (int)(gid - m * L);
    if (m >= M) return;
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    float* tl = gtable + ((int64_t)l << log2T) * F;
    const float* g = gout + (m * L + l) * F;
    if (INTERP == 0) {
        const uint32_t ix = (uint32_t)(int)rintf(sx), iy = (uint32_t)(int)rintf(sy), iz = (uint32_t)(int)rintf(sz);
        float* e = tl + (int64_t)((ix ^ (iy * acn::kP1) ^ (iz * acn::kP2)) & mask) * F;
        for (int f = 0; f < F; ++f) unsafeAtomicAdd(e + f, g[f]);
        return;
    }
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    smooth_weights<INTERP>(wx, wy, wz);
    const float ax = 1.0f - wx, ay = 1.0f - wy, az = 1.0f - wz;
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * acn::kP1;
    const uint32_t z0 = (uint32_t)(int)fz * acn::kP2;
#pragma unroll
    for (int cidx = 0; cidx < 8; ++cidx) {
        const int bx = cidx >> 2, by = (cidx >> 1) & 1, bz = cidx & 1;
        const uint32_t h = ((x0 + (uint32_t)bx) ^ (y0 + (by ? acn::kP1 : 0u)) ^ (z0 + (bz ? acn::kP2 : 0u))) & mask;
        float* e = tl + (int64_t)h * F;
        for (int f = 0; f < F; ++f) {
            const float gv = ((g[f] * (bz ? wz : az)) * (by ? wy : ay)) * (bx ? wx : ax);
            unsafeAtomicAdd(e + f, gv);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// F == 2, Linear / Smoothstep table scatters: one lane per (point stream, corner, feature).  The 64 lanes of a wave
// are 4 streams x 8 corners x 2 features at ONE level, ordered (stream, y/z corner, x corner, feature), so each
// no-return atomic instruction touches ~16 table row pairs (the x-neighbours of a corner pair share a 128-B line)
// instead of the 64 unrelated rows of a lane-per-(point, level) mapping (MI355X_MICROARCH.md "Global float
// atomics": rate set by distinct rows per instruction).
struct CornerLane {
    int f, bx, by, bz;   // feature; the corner's bit per axis
    __device__ explicit CornerLane(int lane)
        : f(lane & 1), bx((lane >> 1) & 1), by((lane >> 3) & 1), bz((lane >> 2) & 1) {}
    // the hashed row of this corner of the cell whose floor is (fx, fy, fz)
    __device__ __forceinline__ uint32_t row(float fx, float fy, float fz, uint32_t mask) const {
        const uint32_t xi = (uint32_t)(int)fx + (uint32_t)bx;
        const uint32_t yi = (uint32_t)(int)fy * acn::kP1 + (by ? acn::kP1 : 0u);
        const uint32_t zi = (uint32_t)(int)fz * acn::kP2 + (bz ? acn::kP2 : 0u);
        return (xi ^ yi ^ zi) & mask;
    }
};
struct Corner {
    uint32_t row;
    float wx, wy, wz;   // the corner's weight per axis: w or 1 - w
};

// The corner of lane c for point m at a level of resolution r.  Its table gradient is ((g * wz) * wy) * wx, the
// chain-rule order of the forward lerps: every scatter forms it in exactly that order (the file is built with
// -ffp-contract=off, so the kernels agree bit for bit).  The complement is 1 - w of the SMOOTHED
// weight, as in the forward; axis_w (the double backward) takes S(1 - u) instead and must not be used here.
template <int INTERP>
__device__ __forceinline__ Corner lane_corner(const CornerLane& c, const float* __restrict__ x01, int64_t m, float r,
                                              uint32_t mask) {
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    smooth_weights<INTERP>(wx, wy, wz);
    return Corner{c.row(fx, fy, fz, mask), c.bx ? wx : 1.0f - wx, c.by ? wy : 1.0f - wy, c.bz ? wz : 1.0f - wz};
}

// consecutive points per lane in hashgrid_bwd_rle / hashgrid_bwd_pairs
constexpr int kRunPoints = 16;

// Run-length-aggregated scatter: a lane walks kRunPoints consecutive points of its stream (a stretch of one ray:
// the training path lays samples out ray-major) at one level, summing gradients in a register while the target
// row repeats and issuing one atomic per run.  Coarse levels see long runs (several samples per cell), which is
// where the per-row atomic contention was; waves interleave levels (l = wave % L) so concurrent waves spread over
// all levels instead of all hammering level 0's few thousand rows at once.  Sum order within a run is the sample
// order; across runs it is the (unordered) atomic order.
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_rle(const float* __restrict__ x01, int64_t M,
                                                        const float* __restrict__ gout, Res32 res, int L,
                                                        int log2T, float* __restrict__ gtable, int l0) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int l = l0 + (int)(wave % (L - l0));  // levels l0..L-1 (the coarser ones: hashgrid_bwd_merge)
    const int64_t chunk = wave / (L - l0);
    const int64_t m0 = (chunk * 4 + (lane >> 4)) * kRunPoints;
    if (m0 >= M) return;
    const CornerLane c(lane);
    const float r = (float)res.v[l];
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const int64_t base = ((int64_t)l << log2T) * 2 + c.f;
    int64_t cur = -1;
    float acc = 0.0f;
#pragma unroll 4
    for (int i = 0; i < kRunPoints; ++i) {
        const int64_t m = m0 + i;
        if (m >= M) break;
        const Corner k = lane_corner<INTERP>(c, x01, m, r, mask);
        const int64_t a = base + (int64_t)k.row * 2;
        const float gv = ((gout[(m * L + l) * 2 + c.f] * k.wz) * k.wy) * k.wx;
        if (a == cur) {
            acc += gv;
        } else {
            if (cur >= 0) unsafeAtomicAdd(gtable + cur, acc);
            cur = a;
            acc = gv;
        }
    }
    if (cur >= 0) unsafeAtomicAdd(gtable + cur, acc);
}

// ---------------------------------------------------------------------------------------------
// (sample, expert) pair lists of the routed container (routed.hip): slot p belongs to expert pk[p],
// the live slot count is seg[K] on the device (graph-replayable: grids are fixed, loops stride to it).
struct Tables {
    const float2* t[acn::kMaxK];
};
struct GradTables {
    float* t[acn::kMaxK];
};
struct SegMaps {   // per expert: the "touched this step" byte map of its table's 64-B segments (or null)
    uint8_t* t[acn::kMaxK];
};

template <int INTERP, bool BUF = false>
__global__ void __launch_bounds__(256) hashgrid_fwd_pairs(const float* __restrict__ x01, const int32_t* __restrict__ pk,
                                                          const int64_t* __restrict__ seg, int K, Tables tabs,
                                                          Res32 res, int L, int log2T, float2* __restrict__ out) {
    const int64_t n = seg[K] * L;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < n; gid += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = gid / L;
        const int l = (int)(gid - m * L);
        const float r = (float)res.v[l];
        const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
        float o0, o1;
        if (BUF) {
            // buffer gathers (hashgrid_fwd_f2_buf) from the table of the lane's expert: one resource per distinct
            // expert of the wave (a wave's slots normally share one; the loop takes each expert once)
            const int k = pk[m];
            for (;;) {
                const int kw = __builtin_amdgcn_readfirstlane(k);
                if (k == kw) {
                    const __amdgpu_buffer_rsrc_t rs = table_rsrc(tabs.t[kw], L, log2T);
                    acn::HashPendingX p;
                    acn::hash_issue_x<INTERP>(rs, (uint32_t)l << (log2T + 3), sx, sy, sz, mask, p);
                    acn::hash_finish_x<INTERP>(p, o0, o1);
                    break;
                }
            }
        } else {
            const float2* tl = tabs.t[pk[m]] + ((int64_t)l << log2T);
            acn::hash_level_f2<INTERP>(tl, sx, sy, sz, mask, o0, o1);
        }
        out[m * L + l] = make_float2(o0, o1);
    }
}

// hashgrid_bwd_rle over pair slots: the run key is (expert, row), so a stretch may cross an expert
// boundary; padding slots (pidx < 0) add nothing.  MARK_ONLY (acn_hashgrid_pairs_mark) reads neither gout nor gt.
// TELE: returning atomics; every run adds new^2 - old^2 (new = old + run sum, the value the atomic
// leaves) to *sq.  Per row these telescope to (final value)^2 - 0, so *sq gains the squared norm of the
// table-gradient update without a pass over the 128 MiB gradient buffers (clip_grad_norm_'s sum of
// squares, runtime_adapt.py:305-307).  Doubles: new^2 and old^2 are exact, so only the differences and
// their sum round (~1e-16 relative).
template <int INTERP, bool TELE, bool MARK_ONLY = false>
__global__ void __launch_bounds__(256) hashgrid_bwd_pairs(const float* __restrict__ x01, const int32_t* __restrict__ pk,
                                                          const int32_t* __restrict__ pidx,
                                                          const int64_t* __restrict__ seg, int K,
                                                          const float* __restrict__ gout, GradTables gt, Res32 res,
                                                          int L, int log2T, double* __restrict__ sq, SegMaps smaps) {
    const int lane = threadIdx.x & 63;
    const int64_t M = seg[K];
    const int64_t nwaves = ((M + 4 * kRunPoints - 1) / (4 * kRunPoints)) * L;
    const CornerLane c(lane);
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    double tsq = 0.0;
    auto flush = [&](float* a, float v) {
        if (MARK_ONLY) return;   // acn_hashgrid_pairs_mark: segment maps only
        if (TELE) {
            const float o = atomicAdd(a, v);
            const float nv = o + v;
            tsq += (double)nv * (double)nv - (double)o * (double)o;
        } else {
            unsafeAtomicAdd(a, v);
        }
    };
    for (int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wave < nwaves;
         wave += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int l = (int)(wave % L);
        const int64_t chunk = wave / L;
        const int64_t m0 = (chunk * 4 + (lane >> 4)) * kRunPoints;
        const float r = (float)res.v[l];
        const int64_t base = ((int64_t)l << log2T) * 2 + c.f;
        constexpr uint32_t kNoRun = 0xffffffffu;   // rows have at most 30 bits
        uint32_t cur_row = kNoRun;
        int cur_k = 0;
        uint8_t* cseg = nullptr;   // the segment-map byte of the run's 64-B segment (segment maps on)
        float acc = 0.0f;
        auto end_run = [&]() {
            if (cur_row == kNoRun) return;
            flush(gt.t[cur_k] + base + (int64_t)cur_row * 2, acc);
            if (cseg && c.f == 0) *cseg = 1;   // idempotent plain byte store (feature 1 shares the row)
        };
        for (int i = 0; i < kRunPoints; ++i) {
            const int64_t m = m0 + i;
            if (m >= M) break;
            if (pidx[m] < 0) continue;
            const Corner k = lane_corner<INTERP>(c, x01, m, r, mask);
            const int kk = pk[m];
            const float gv = MARK_ONLY ? 0.0f : ((gout[(m * L + l) * 2 + c.f] * k.wz) * k.wy) * k.wx;
            if (k.row == cur_row && kk == cur_k) {
                acc += gv;
            } else {
                end_run();
                cur_row = k.row;
                cur_k = kk;
                cseg = smaps.t[kk] ? smaps.t[kk] + ((((int64_t)l << log2T) + k.row) >> 3) : nullptr;
                acc = gv;
            }
        }
        end_run();
    }
    if (TELE) {  // one double atomic per wave
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tsq += __shfl_xor(tsq, off);
        if (lane == 0 && tsq != 0.0) atomicAdd(sq, tsq);
    }
}

// ---------------------------------------------------------------------------------------------
// Coarse levels of the standalone table-gradient scatter (acn_hashgrid_bwd), merged per workgroup.
// At the coarse levels many samples -- of one ray and of neighbouring rays -- add into the same rows, but a lane's
// run merge only sees one corner of one sample stream.  Here a workgroup takes a chunk of C_l consecutive points at
// one level, accumulates every (point, corner) contribution into an LDS hash table keyed by the row's 64-B
// segment with LDS float atomics, then flushes each touched segment as 16 consecutive floats (4 segments per
// wave-instruction = the full-rate shape of MI355X_MICROARCH.md 'Global float atomics').  Memory-side requests fall
// from one per (run, corner pair) to one per distinct segment of the chunk.  A full table (more distinct segments
// than kMergeNE) falls back to direct atomics for the overflowing contributions.  Sums stay fp32; their order is as
// unordered as the atomics they replace.
// The pair-list scatter (hashgrid_bwd_pairs) keeps every level on the run merge: merged coarse levels measured
// slower on the C5 step (hash backward 0.36 -> 0.76 / 0.79 / 0.89 ms merging 3 / 6 / 8 levels) -- a
// coarse chunk is one workgroup's serial work (few items in flight) and the runs of neighbouring lanes collide on
// the same LDS entries -- and they can neither telescope the clip norm nor mark the segment maps.
constexpr int kMergeLogNE = 10, kMergeNE = 1 << kMergeLogNE;
constexpr uint32_t kMergeEmpty = 0xffffffffu;
// merged levels of the standalone scatter (the meta-training query step, whose batch is ~6x C5's): 6 cut the
// scatter 855 -> 795 us and the meta step 1.1%
constexpr int kMergeLevels = 6;
struct MergeCfg {
    int LM;                   // levels 0 .. LM-1 are merged here
    int clog2[ACN_MAX_LEVELS];  // chunk of 2^clog2[l] points per workgroup item at level l
};

template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_merge(const float* __restrict__ x01, int64_t M,
                                                          const float* __restrict__ gout,
                                                          float* __restrict__ gtable, Res32 res, int L, int log2T,
                                                          MergeCfg cfg) {
    __shared__ uint32_t keys[kMergeNE];
    __shared__ __attribute__((aligned(16))) float vals[kMergeNE * 16];
    int64_t items = 0;
    for (int l = 0; l < cfg.LM; ++l) items += (M + (1ll << cfg.clog2[l]) - 1) >> cfg.clog2[l];
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        int l = 0;
        int64_t rem = it;
        for (; l < cfg.LM - 1; ++l) {
            const int64_t n = (M + (1ll << cfg.clog2[l]) - 1) >> cfg.clog2[l];
            if (rem < n) break;
            rem -= n;
        }
        const int64_t m0 = rem << cfg.clog2[l], m1 = min(M, m0 + (1ll << cfg.clog2[l]));
        for (int i = threadIdx.x; i < kMergeNE; i += blockDim.x) keys[i] = kMergeEmpty;
        for (int i = threadIdx.x; i < kMergeNE * 4; i += blockDim.x)
            reinterpret_cast<float4*>(vals)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        __syncthreads();
        const float r = (float)res.v[l];
        float* tl = gtable + ((int64_t)l << log2T) * 2;
        // lanes as in hashgrid_bwd_rle; a lane run-merges 16 consecutive points of its stream and adds each
        // finished run into the LDS table (LDS atomics on runs, not on every contribution: coarse cells repeat
        // along a ray)
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        const CornerLane c(lane);
        auto add_run = [&](uint32_t row, float v) {
            const uint32_t key = row >> 3;   // the row's 64-B segment: 24 bits (merge_cfg), never kMergeEmpty
            uint32_t h = (key * 2654435761u) >> (32 - kMergeLogNE);
            for (int probe = 0; probe < 32; ++probe) {
                uint32_t cur = keys[h];
                if (cur == kMergeEmpty) cur = atomicCAS(&keys[h], kMergeEmpty, key);
                if (cur == kMergeEmpty || cur == key) {
                    atomicAdd(&vals[h * 16 + (row & 7) * 2 + c.f], v);
                    return;
                }
                h = (h + 1) & (kMergeNE - 1);
            }
            unsafeAtomicAdd(tl + (int64_t)row * 2 + c.f, v);  // table crowded
        };
        for (int64_t sb = m0 + (int64_t)w * 64; sb < m1; sb += (int64_t)nw * 64) {
            const int64_t mb = sb + (lane >> 4) * 16;
            uint32_t cur_row = 0xffffffffu;
            float acc = 0.0f;
            for (int i = 0; i < 16; ++i) {
                const int64_t m = mb + i;
                if (m >= m1) break;
                const Corner k = lane_corner<INTERP>(c, x01, m, r, mask);
                const float gv = ((gout[(m * L + l) * 2 + c.f] * k.wz) * k.wy) * k.wx;
                if (k.row == cur_row) {
                    acc += gv;
                } else {
                    if (cur_row != 0xffffffffu) add_run(cur_row, acc);
                    cur_row = k.row;
                    acc = gv;
                }
            }
            if (cur_row != 0xffffffffu) add_run(cur_row, acc);
        }
        __syncthreads();
        // flush: 16 consecutive lanes per segment
        for (int i = threadIdx.x; i < kMergeNE * 16; i += blockDim.x) {
            const uint32_t key = keys[i >> 4];
            const float v = vals[i];
            if (key != kMergeEmpty && v != 0.0f) unsafeAtomicAdd(tl + (int64_t)key * 16 + (i & 15), v);
        }
        __syncthreads();
    }
}

MergeCfg merge_cfg(int L, int log2T, int levels) {
    MergeCfg c{};
    c.LM = levels < L ? levels : L;
    if (log2T > 27) c.LM = 0;  // the LDS key holds a 24-bit segment index
    // chunks sized so a chunk's distinct segments stay well under kMergeNE at the reference grid
    // (tools/hash_bwd_analysis.py on the C5 batch: level 0 ~13k segments per 104k slots ... level 5 ~230k)
    const int lg[8] = {12, 11, 10, 9, 8, 8, 7, 7};
    for (int l = 0; l < ACN_MAX_LEVELS; ++l) c.clog2[l] = l < 8 ? lg[l] : 7;
    return c;
}

// ---------------------------------------------------------------------------------------------
// Input gradient: grad_x (M,3) of sum(out * grad_out), the autograd of encodings.py:331-381 in x.  Per level the
// forward is out_f = interp(rows_f; w(x * res)), so
//   grad_x[a] = sum_l res_l * dw_a * sum_f grad_out[l,f] * d/dw_a interp(rows_f; w)
// with dw = 1 (Linear) or 6 w (1 - w) (Smoothstep, the lerps on the smoothed w).  interp is linear in the rows, so
// the features are folded first (v_corner = sum_f g_f * row_f) and one scalar trilinear form is differentiated:
// d/dw_z is the difference of the two z-planes, d/dw_y the z-lerp of the y-differences of the x-lerps, d/dw_x the
// y -> z lerp of the four x-differences.  Nearest has a zero gradient (acn_hashgrid_bwd_input writes zeros).
//
// Gather forms: F == 2 with a table of at most 2 GiB reads the rows through a buffer resource over the whole table
// with 32-bit offsets (hash_issue_x, exactly the forward's gathers; hashgrid_bwd_input_f2).  Larger tables and
// F != 2 use the 64-bit pointer form, as hashgrid_fwd_f2 / hashgrid_fwd_gen do (hashgrid_bwd_input_gen).
//
// No atomics: a point's level terms are summed in a fixed order that depends on nothing but L -- an xor-shuffle
// tree over the point's L adjacent lanes when L is a power of two (TREE: one lane per (point, level), as the
// forward), else one lane per point adding levels 0 .. L-1 in turn.
// level_grad (acn_device.h) differentiates one level's trilinear form; field_sigma_grad_kernel (mlp_train.hip) shares it.
using acn::LevelGrad;
using acn::level_grad;

template <int INTERP>
__device__ __forceinline__ LevelGrad level_grad_f2(__amdgpu_buffer_rsrc_t rs, int l, int log2T, uint32_t mask,
                                                   float r, float px, float py, float pz, float2 g) {
    const float sx = px * r, sy = py * r, sz = pz * r;
    acn::HashPendingX p;
    acn::hash_issue_x<INTERP>(rs, (uint32_t)l << (log2T + 3), sx, sy, sz, mask, p);
    float2 f[8];
    acn::hash_rows_x(p, f);
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = g.x * f[c].x + g.y * f[c].y;
    return level_grad<INTERP>(v, sx - floorf(sx), sy - floorf(sy), sz - floorf(sz), r);
}

template <int INTERP, bool TREE>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_f2(const float* __restrict__ x01, int64_t M,
                                                             const float2* __restrict__ gout,
                                                             const float2* __restrict__ table, Res32 res, int L,
                                                             int log2T, float* __restrict__ gx) {
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const __amdgpu_buffer_rsrc_t rs = table_rsrc(table, L, log2T);
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (TREE) {
        // L is a power of two <= 32: a point's lanes are one aligned group of a wave, live or idle together
        const int64_t m = gid / L;
        const int l = (int)(gid - m * L);
        LevelGrad a{0.0f, 0.0f, 0.0f};
        if (m < M)
            a = level_grad_f2<INTERP>(rs, l, log2T, mask, (float)res.v[l], x01[3 * m], x01[3 * m + 1], x01[3 * m + 2],
                                      gout[m * L + l]);
        for (int off = 1; off < L; off <<= 1) {
            a.x += __shfl_xor(a.x, off);
            a.y += __shfl_xor(a.y, off);
            a.z += __shfl_xor(a.z, off);
        }
        if (m < M && l == 0) {
            gx[3 * m] = a.x;
            gx[3 * m + 1] = a.y;
            gx[3 * m + 2] = a.z;
        }
    } else {
        const int64_t m = gid;
        if (m >= M) return;
        const float px = x01[3 * m], py = x01[3 * m + 1], pz = x01[3 * m + 2];
        LevelGrad a{0.0f, 0.0f, 0.0f};
        for (int l = 0; l < L; ++l) {
            const LevelGrad t = level_grad_f2<INTERP>(rs, l, log2T, mask, (float)res.v[l], px, py, pz, gout[m * L + l]);
            a.x += t.x;
            a.y += t.y;
            a.z += t.z;
        }
        gx[3 * m] = a.x;
        gx[3 * m + 1] = a.y;
        gx[3 * m + 2] = a.z;
    }
}

// any F, any table size: 64-bit row addresses, one lane per point
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_gen(const float* __restrict__ x01, int64_t M,
                                                              const float* __restrict__ gout,
                                                              const float* __restrict__ table, Res32 res, int L,
                                                              int log2T, int F, float* __restrict__ gx) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const float px = x01[3 * m], py = x01[3 * m + 1], pz = x01[3 * m + 2];
    LevelGrad a{0.0f, 0.0f, 0.0f};
    for (int l = 0; l < L; ++l) {
        const float r = (float)res.v[l];
        const float sx = px * r, sy = py * r, sz = pz * r;
        const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
        const uint32_t x0 = (uint32_t)(int)fx, x1 = x0 + 1u;
        const uint32_t y0 = (uint32_t)(int)fy * acn::kP1, y1 = y0 + acn::kP1;
        const uint32_t z0 = (uint32_t)(int)fz * acn::kP2, z1 = z0 + acn::kP2;
        const uint32_t rows[8] = {x0 ^ y0 ^ z0, x1 ^ y0 ^ z0, x0 ^ y0 ^ z1, x1 ^ y0 ^ z1,
                                  x0 ^ y1 ^ z0, x1 ^ y1 ^ z0, x0 ^ y1 ^ z1, x1 ^ y1 ^ z1};
        const float* tl = table + ((int64_t)l << log2T) * F;
        const float* g = gout + (m * L + l) * F;
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float* e = tl + (int64_t)(rows[c] & mask) * F;
            float s = 0.0f;
            for (int f = 0; f < F; ++f) s += g[f] * e[f];
            v[c] = s;
        }
        const LevelGrad t = level_grad<INTERP>(v, sx - fx, sy - fy, sz - fz, r);
        a.x += t.x;
        a.y += t.y;
        a.z += t.z;
    }
    gx[3 * m] = a.x;
    gx[3 * m + 1] = a.y;
    gx[3 * m + 2] = a.z;
}

// ---------------------------------------------------------------------------------------------
// Double backward of the input gradient: with t = gg_x (M,3) the cotangent of grad_x, the
// derivatives of sum_a t_a grad_x[a] in grad_out (gather), in the points (gather) and in the table (scatter).  Per
// level, u the raw weights, w = S(u), X/Y/Z(b) the corner's weight per axis (w or 1 - w), sgn(b) = +-1:
//   p_a     = (t_a * res) * S'(u_a)
//   k_b     = p_x sgn_x Y Z + p_y X sgn_y Z + p_z X Y sgn_z                   (replaces the trilinear weight)
//   gg[f]   = sum_b k_b row_b[f],      grad_table[row_b, f] += k_b * g[f]
//   g_x[e]  = res^2 (S'(u_e) sum_{a != e} t_a S'(u_a) H_ae + t_e S''(u_e) G_e)
// G_e the first and H_ae the mixed second differences of the folded corner values V_b = sum_f g[f] row_b[f] (the
// trilinear form has no pure second derivative, so Linear keeps the H terms only).
struct AxisW {
    float w, a, d1, d2;   // S(u), 1 - S(u), S'(u), S''(u)
};

// Every member keeps its relative accuracy: 1 - u and 1 - 2u are exact where they cancel, and the complement of
// the smoothed weight is S(1 - u), not 1 - S(u) (whose rounding is absolute: as the weight of a single corner in
// the table scatter it would miss the per-row bound next to w = 1).
template <int INTERP>
__device__ __forceinline__ AxisW axis_w(float u) {
    const float q = 1.0f - u;
    if (INTERP == 2)
        return AxisW{(u * u) * (3.0f - 2.0f * u), (q * q) * (3.0f - 2.0f * q), (6.0f * u) * q, 6.0f * (1.0f - 2.0f * u)};
    return AxisW{u, q, 1.0f, 0.0f};
}

// k_b of one corner: X, Y, Z its weights per axis, bx / by / bz its bits
__device__ __forceinline__ float corner_k(float px, float py, float pz, float X, float Y, float Z, bool bx, bool by,
                                          bool bz) {
    const float tx = px * (Y * Z), ty = py * (X * Z), tz = pz * (X * Y);
    return ((bx ? tx : -tx) + (by ? ty : -ty)) + (bz ? tz : -tz);
}

// k[] in hash_issue's order (bit0 = x1, bit1 = z1, bit2 = y1)
__device__ __forceinline__ void corner_ks(const AxisW& X, const AxisW& Y, const AxisW& Z, float r, float tx, float ty,
                                          float tz, float (&k)[8]) {
    const float px = (tx * r) * X.d1, py = (ty * r) * Y.d1, pz = (tz * r) * Z.d1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool bx = (c & 1) != 0, bz = (c & 2) != 0, by = (c & 4) != 0;
        k[c] = corner_k(px, py, pz, bx ? X.w : X.a, by ? Y.w : Y.a, bz ? Z.w : Z.a, bx, by, bz);
    }
}

// v[]: the folded corner values in hash_issue's order
template <int INTERP>
__device__ __forceinline__ LevelGrad level_hess(const float (&v)[8], const AxisW& X, const AxisW& Y, const AxisW& Z,
                                                float r, float tx, float ty, float tz) {
    const float wx = X.w, wy = Y.w, wz = Z.w;
    const float ax = X.a, ay = Y.a, az = Z.a;
    const float c00 = v[0] * ax + v[1] * wx, c01 = v[2] * ax + v[3] * wx;   // c{y}{z}: the forward's x-lerps
    const float c10 = v[4] * ax + v[5] * wx, c11 = v[6] * ax + v[7] * wx;
    const float d00 = v[1] - v[0], d01 = v[3] - v[2], d10 = v[5] - v[4], d11 = v[7] - v[6];
    const float hxy = (d10 - d00) * az + (d11 - d01) * wz;
    const float hxz = (d01 - d00) * ay + (d11 - d10) * wy;
    const float hyz = (c11 - c01) - (c10 - c00);
    const float px = tx * X.d1, py = ty * Y.d1, pz = tz * Z.d1;
    float ex = X.d1 * (py * hxy + pz * hxz);
    float ey = Y.d1 * (px * hxy + pz * hyz);
    float ez = Z.d1 * (px * hxz + py * hyz);
    if (INTERP == 2) {
        const float gx = (d00 * ay + d10 * wy) * az + (d01 * ay + d11 * wy) * wz;
        const float gy = (c10 - c00) * az + (c11 - c01) * wz;
        const float gz = (c01 * ay + c11 * wy) - (c00 * ay + c10 * wy);
        ex += (tx * X.d2) * gx;
        ey += (ty * Y.d2) * gy;
        ez += (tz * Z.d2) * gz;
    }
    const float r2 = r * r;
    return LevelGrad{r2 * ex, r2 * ey, r2 * ez};
}

// one level of the F == 2 buffer form: gg (when want_gg) and the level's g_x term (when want_gx, else zeros)
template <int INTERP>
__device__ __forceinline__ LevelGrad level_hess_f2(__amdgpu_buffer_rsrc_t rs, int l, int log2T, uint32_t mask,
                                                   float r, float px, float py, float pz, float2 g, float tx,
                                                   float ty, float tz, bool want_gg, bool want_gx, float2& gg) {
    const float sx = px * r, sy = py * r, sz = pz * r;
    acn::HashPendingX p;
    acn::hash_issue_x<INTERP>(rs, (uint32_t)l << (log2T + 3), sx, sy, sz, mask, p);
    float2 f[8];
    acn::hash_rows_x(p, f);
    const AxisW X = axis_w<INTERP>(sx - floorf(sx)), Y = axis_w<INTERP>(sy - floorf(sy)),
                Z = axis_w<INTERP>(sz - floorf(sz));
    if (want_gg) {
        float k[8];
        corner_ks(X, Y, Z, r, tx, ty, tz, k);
        float s0 = k[0] * f[0].x, s1 = k[0] * f[0].y;
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            s0 += k[c] * f[c].x;
            s1 += k[c] * f[c].y;
        }
        gg = make_float2(s0, s1);
    }
    if (!want_gx) return LevelGrad{0.0f, 0.0f, 0.0f};
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = g.x * f[c].x + g.y * f[c].y;
    return level_hess<INTERP>(v, X, Y, Z, r, tx, ty, tz);
}

// ggout / gx2: either may be null (uniform)
template <int INTERP, bool TREE>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_bwd_f2(const float* __restrict__ x01, int64_t M,
                                                                 const float2* __restrict__ gout,
                                                                 const float* __restrict__ ggx,
                                                                 const float2* __restrict__ table, Res32 res, int L,
                                                                 int log2T, float2* __restrict__ ggout,
                                                                 float* __restrict__ gx2) {
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const __amdgpu_buffer_rsrc_t rs = table_rsrc(table, L, log2T);
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool want_gg = ggout != nullptr, want_gx = gx2 != nullptr;
    if (TREE) {
        // one lane per (point, level), as hashgrid_bwd_input_f2: gg is the lane's own, the g_x terms take the tree
        const int64_t m = gid / L;
        const int l = (int)(gid - m * L);
        LevelGrad a{0.0f, 0.0f, 0.0f};
        if (m < M) {
            float2 gg;
            a = level_hess_f2<INTERP>(rs, l, log2T, mask, (float)res.v[l], x01[3 * m], x01[3 * m + 1], x01[3 * m + 2],
                                      gout[m * L + l], ggx[3 * m], ggx[3 * m + 1], ggx[3 * m + 2], want_gg, want_gx, gg);
            if (want_gg) ggout[m * L + l] = gg;
        }
        if (!want_gx) return;
        for (int off = 1; off < L; off <<= 1) {
            a.x += __shfl_xor(a.x, off);
            a.y += __shfl_xor(a.y, off);
            a.z += __shfl_xor(a.z, off);
        }
        if (m < M && l == 0) {
            gx2[3 * m] = a.x;
            gx2[3 * m + 1] = a.y;
            gx2[3 * m + 2] = a.z;
        }
    } else {
        const int64_t m = gid;
        if (m >= M) return;
        const float px = x01[3 * m], py = x01[3 * m + 1], pz = x01[3 * m + 2];
        const float tx = ggx[3 * m], ty = ggx[3 * m + 1], tz = ggx[3 * m + 2];
        LevelGrad a{0.0f, 0.0f, 0.0f};
        for (int l = 0; l < L; ++l) {
            float2 gg;
            const LevelGrad t = level_hess_f2<INTERP>(rs, l, log2T, mask, (float)res.v[l], px, py, pz, gout[m * L + l],
                                                      tx, ty, tz, want_gg, want_gx, gg);
            if (want_gg) ggout[m * L + l] = gg;
            a.x += t.x;
            a.y += t.y;
            a.z += t.z;
        }
        if (want_gx) {
            gx2[3 * m] = a.x;
            gx2[3 * m + 1] = a.y;
            gx2[3 * m + 2] = a.z;
        }
    }
}

// any F, any table size: 64-bit row addresses, one lane per point
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_bwd_gen(const float* __restrict__ x01, int64_t M,
                                                                  const float* __restrict__ gout,
                                                                  const float* __restrict__ ggx,
                                                                  const float* __restrict__ table, Res32 res, int L,
                                                                  int log2T, int F, float* __restrict__ ggout,
                                                                  float* __restrict__ gx2) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const float px = x01[3 * m], py = x01[3 * m + 1], pz = x01[3 * m + 2];
    const float tx = ggx[3 * m], ty = ggx[3 * m + 1], tz = ggx[3 * m + 2];
    LevelGrad a{0.0f, 0.0f, 0.0f};
    for (int l = 0; l < L; ++l) {
        const float r = (float)res.v[l];
        const float sx = px * r, sy = py * r, sz = pz * r;
        const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
        const uint32_t x0 = (uint32_t)(int)fx, x1 = x0 + 1u;
        const uint32_t y0 = (uint32_t)(int)fy * acn::kP1, y1 = y0 + acn::kP1;
        const uint32_t z0 = (uint32_t)(int)fz * acn::kP2, z1 = z0 + acn::kP2;
        const uint32_t rows[8] = {x0 ^ y0 ^ z0, x1 ^ y0 ^ z0, x0 ^ y0 ^ z1, x1 ^ y0 ^ z1,
                                  x0 ^ y1 ^ z0, x1 ^ y1 ^ z0, x0 ^ y1 ^ z1, x1 ^ y1 ^ z1};
        const float* tl = table + ((int64_t)l << log2T) * F;
        const float* g = gout + (m * L + l) * F;
        const AxisW X = axis_w<INTERP>(sx - fx), Y = axis_w<INTERP>(sy - fy), Z = axis_w<INTERP>(sz - fz);
        if (ggout) {
            float k[8];
            corner_ks(X, Y, Z, r, tx, ty, tz, k);
            float* o = ggout + (m * L + l) * F;
            for (int f = 0; f < F; ++f) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < 8; ++c) s += k[c] * tl[(int64_t)(rows[c] & mask) * F + f];
                o[f] = s;
            }
        }
        if (gx2) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float* e = tl + (int64_t)(rows[c] & mask) * F;
                float s = 0.0f;
                for (int f = 0; f < F; ++f) s += g[f] * e[f];
                v[c] = s;
            }
            const LevelGrad t = level_hess<INTERP>(v, X, Y, Z, r, tx, ty, tz);
            a.x += t.x;
            a.y += t.y;
            a.z += t.z;
        }
    }
    if (gx2) {
        gx2[3 * m] = a.x;
        gx2[3 * m + 1] = a.y;
        gx2[3 * m + 2] = a.z;
    }
}

// The table side, F == 2: one lane per (point, corner, feature), no run merge.  A wave is 4 consecutive points x
// CornerLane's 8 corners x 2 features at one level; waves go level by level over the groups of 4 points.  k_b in
// place of the trilinear weight (its weights are axis_w's, not lane_corner's).
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_bwd_table_f2(const float* __restrict__ x01, int64_t M,
                                                                       const float* __restrict__ gout,
                                                                       const float* __restrict__ ggx, Res32 res, int L,
                                                                       int log2T, float* __restrict__ gtable) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t groups = (M + 3) >> 2;               // groups of 4 points
    const int l = (int)(wave / groups);
    const int64_t m = (wave - (int64_t)l * groups) * 4 + (lane >> 4);
    if (l >= L || m >= M) return;
    const CornerLane c(lane);
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    const AxisW X = axis_w<INTERP>(sx - fx), Y = axis_w<INTERP>(sy - fy), Z = axis_w<INTERP>(sz - fz);
    const uint32_t h = c.row(fx, fy, fz, mask);
    const float k = corner_k((ggx[3 * m] * r) * X.d1, (ggx[3 * m + 1] * r) * Y.d1, (ggx[3 * m + 2] * r) * Z.d1,
                             c.bx ? X.w : X.a, c.by ? Y.w : Y.a, c.bz ? Z.w : Z.a, c.bx, c.by, c.bz);
    unsafeAtomicAdd(gtable + (((int64_t)l << log2T) + h) * 2 + c.f, k * gout[(m * L + l) * 2 + c.f]);
}

// generic F: hashgrid_bwd_gen's mapping, one lane per (point, level)
template <int INTERP>
__global__ void __launch_bounds__(256) hashgrid_bwd_input_bwd_table_gen(const float* __restrict__ x01, int64_t M,
                                                                        const float* __restrict__ gout,
                                                                        const float* __restrict__ ggx, Res32 res,
                                                                        int L, int log2T, int F,
                                                                        float* __restrict__ gtable) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = gid / L;
    const int l = (int)(gid - m * L);
    if (m >= M) return;
    const float r = (float)res.v[l];
    const float sx = x01[3 * m] * r, sy = x01[3 * m + 1] * r, sz = x01[3 * m + 2] * r;
    const uint32_t mask = (uint32_t)((1ull << log2T) - 1ull);
    float* tl = gtable + ((int64_t)l << log2T) * F;
    const float* g = gout + (m * L + l) * F;
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    const AxisW X = axis_w<INTERP>(sx - fx), Y = axis_w<INTERP>(sy - fy), Z = axis_w<INTERP>(sz - fz);
    float k[8];
    corner_ks(X, Y, Z, r, ggx[3 * m], ggx[3 * m + 1], ggx[3 * m + 2], k);
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * acn::kP1;
    const uint32_t z0 = (uint32_t)(int)fz * acn::kP2;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t h = ((x0 + ((c & 1) ? 1u : 0u)) ^ (y0 + ((c & 4) ? acn::kP1 : 0u)) ^ (z0 + ((c & 2) ? acn::kP2 : 0u))) & mask;
        float* e = tl + (int64_t)h * F;
        for (int f = 0; f < F; ++f) unsafeAtomicAdd(e + f, k[c] * g[f]);
    }
}

__global__ void __launch_bounds__(256) zero_f32(float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

// Backward of sh_encode (acn_device.h) in the unnormalised direction: g_n through the polynomials, then through
// n = d / max(|d|, 1e-9) as torch differentiates norm and clamp_min (the clamp passes no gradient below 1e-9).
template <int DEGREE>
__global__ void __launch_bounds__(256) sh_bwd_kernel(const float* __restrict__ d, int64_t M,
                                                     const float* __restrict__ gout, float* __restrict__ gd) {
    constexpr int C = (DEGREE + 1) * (DEGREE + 1);
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const float dx = d[3 * m], dy = d[3 * m + 1], dz = d[3 * m + 2];
    const float nrm = acn::norm3(dx, dy, dz);
    const float n = acn::clamp_min_nan(nrm, 1e-9f);
    const float x = dx / n, y = dy / n, z = dz / n;
    float g[C];
#pragma unroll
    for (int i = 0; i < C; ++i) g[i] = gout[m * C + i];
    float gx, gy, gz;
    acn::sh_components_bwd<DEGREE>(x, y, z, g, gx, gy, gz);
    if (nrm >= 1e-9f) {
        const float dot = (x * gx + y * gy) + z * gz;
        gx = gx - x * dot;
        gy = gy - y * dot;
        gz = gz - z * dot;
    }
    gd[3 * m] = gx / n;
    gd[3 * m + 1] = gy / n;
    gd[3 * m + 2] = gz / n;
}

template <int DEGREE>
__global__ void __launch_bounds__(256) sh_fwd_kernel(const float* __restrict__ d, int64_t M,
                                                     float* __restrict__ out) {
    constexpr int C = (DEGREE + 1) * (DEGREE + 1);
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float c[C];
    acn::sh_encode<DEGREE>(d[3 * m], d[3 * m + 1], d[3 * m + 2], c);
#pragma unroll
    for (int i = 0; i < C; ++i) out[m * C + i] = c[i];
}

// ---------------------------------------------------------------------------------------------
// Host side.  The runtime interpolation mode (and a flag) become template arguments through generic lambdas:
// with_interp(interp, [&](auto i) { constexpr int I = decltype(i)::value; ... kernel<I> ... }).
template <class Fn>
void with_lerp(int interp, Fn&& fn) {   // Linear / Smoothstep: the caller has handled or rejected Nearest
    if (interp == 1) fn(std::integral_constant<int, 1>{});
    else fn(std::integral_constant<int, 2>{});
}
template <class Fn>
void with_interp(int interp, Fn&& fn) {
    if (interp == 0) fn(std::integral_constant<int, 0>{});
    else with_lerp(interp, fn);
}
template <class Fn>
void with_bool(bool b, Fn&& fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}

inline dim3 blocks(int64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

Res32 pack_res(const int32_t* res, int L) {
    Res32 r{};
    for (int i = 0; i < L; ++i) r.v[i] = res[i];
    return r;
}

// The arguments common to the grid entry points, reported under the entry point's name fn; packs res into r.
// fmax: the entry's cap on features_per_level, 0 for none (the input-gradient entries take any F >= 1).
int check_grid(const char* fn, int64_t M, int L, int log2T, int F, int fmax, int interp, const int32_t* res,
               Res32& r) {
    ACN_REQUIRE(M >= 0, "%s: M must be >= 0", fn);
    ACN_REQUIRE(L >= 1 && L <= ACN_MAX_LEVELS, "%s: levels must be in [1, %d], got %d", fn, ACN_MAX_LEVELS, L);
    ACN_REQUIRE(log2T >= 1 && log2T <= 30, "%s: log2_hashmap_size must be in [1, 30], got %d", fn, log2T);
    if (fmax) ACN_REQUIRE(F >= 1 && F <= fmax, "%s: features_per_level must be in [1, %d], got %d", fn, fmax, F);
    else ACN_REQUIRE(F >= 1, "%s: features_per_level must be >= 1, got %d", fn, F);
    ACN_REQUIRE(interp >= 0 && interp <= 2, "%s: bad interpolation %d", fn, interp);
    ACN_REQUIRE(res != nullptr, "%s: res is NULL", fn);
    r = pack_res(res, L);
    return ACN_OK;
}

}  // namespace

extern "C" int acn_hashgrid_fwd(const float* x01, int64_t M, const float* table, const int32_t* res, int L,
                                int log2T, int F, int interp, float* out, void* stream) {
    Res32 r;
    if (const int rc = check_grid("acn_hashgrid_fwd", M, L, log2T, F, 64, interp, res, r)) return rc;
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(x01 && table && out, "acn_hashgrid_fwd: NULL pointer");
    const dim3 grid = blocks(M * L), block(256);
    hipStream_t s = (hipStream_t)stream;
    with_interp(interp, [&](auto i) {
        constexpr int I = decltype(i)::value;
        const float2* t2 = (const float2*)table;
        float2* o2 = (float2*)out;
        if (F != 2) {
            hipLaunchKernelGGL(hashgrid_fwd_gen<I>, grid, block, 0, s, x01, M, table, r, L, log2T, F, out);
            return;
        }
        if constexpr (I != 0) {
            if (table_fits_buffer(L, log2T)) {
                hipLaunchKernelGGL(hashgrid_fwd_f2_buf<I>, grid, block, 0, s, x01, M, t2, r, L, log2T, o2);
                return;
            }
        }
        hipLaunchKernelGGL(hashgrid_fwd_f2<I>, grid, block, 0, s, x01, M, t2, r, L, log2T, o2);
    });
    return acn_check_launch("acn_hashgrid_fwd");
}

extern "C" int acn_hashgrid_bwd(const float* x01, int64_t M, const float* grad_out, const int32_t* res, int L,
                                int log2T, int F, int interp, float* grad_table, void* stream) {
    Res32 r;
    if (const int rc = check_grid("acn_hashgrid_bwd", M, L, log2T, F, 64, interp, res, r)) return rc;
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(x01 && grad_out && grad_table, "acn_hashgrid_bwd: NULL pointer");
    const dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
    if (F == 2 && interp != 0) {  // the coarse levels merged per workgroup, the others on the run merge
        const MergeCfg mc = merge_cfg(L, log2T, kMergeLevels);
        with_lerp(interp, [&](auto i) {
            constexpr int I = decltype(i)::value;
            if (mc.LM > 0) {
                int64_t items = 0;
                for (int l = 0; l < mc.LM; ++l) items += (M + (1ll << mc.clog2[l]) - 1) >> mc.clog2[l];
                const dim3 mgrid((unsigned)(items < 1024 ? items : 1024));
                hipLaunchKernelGGL(hashgrid_bwd_merge<I>, mgrid, block, 0, s, x01, M, grad_out, grad_table, r, L, log2T, mc);
            }
            if (mc.LM < L) {
                const int64_t waves = ((M + 4 * kRunPoints - 1) / (4 * kRunPoints)) * (L - mc.LM);
                hipLaunchKernelGGL(hashgrid_bwd_rle<I>, blocks(waves * 64), block, 0, s, x01, M, grad_out, r, L, log2T, grad_table, mc.LM);
            }
        });
    } else {
        with_interp(interp, [&](auto i) {
            hipLaunchKernelGGL(hashgrid_bwd_gen<decltype(i)::value>, blocks(M * L), block, 0, s, x01, M, grad_out, r, L, log2T, F, grad_table);
        });
    }
    return acn_check_launch("acn_hashgrid_bwd");
}

extern "C" int acn_sh_fwd(const float* d, int64_t M, int levels, float* out, void* stream) {
    ACN_REQUIRE(levels >= 1 && levels <= 5, "acn_sh_fwd: Supported levels in [1, 5], got %d", levels);
    ACN_REQUIRE(M >= 0, "acn_sh_fwd: M must be >= 0");
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(d && out, "acn_sh_fwd: NULL pointer");
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (levels) {
        case 1: hipLaunchKernelGGL(sh_fwd_kernel<0>, grid, block, 0, s, d, M, out); break;
        case 2: hipLaunchKernelGGL(sh_fwd_kernel<1>, grid, block, 0, s, d, M, out); break;
        case 3: hipLaunchKernelGGL(sh_fwd_kernel<2>, grid, block, 0, s, d, M, out); break;
        case 4: hipLaunchKernelGGL(sh_fwd_kernel<3>, grid, block, 0, s, d, M, out); break;
        default: hipLaunchKernelGGL(sh_fwd_kernel<4>, grid, block, 0, s, d, M, out); break;
    }
    return acn_check_launch("acn_sh_fwd");
}

extern "C" int acn_hashgrid_bwd_input(const float* x01, int64_t M, const float* grad_out, const float* table,
                                      const int32_t* res, int L, int log2T, int F, int interp, float* grad_x,
                                      void* stream) {
    Res32 r;
    if (const int rc = check_grid("acn_hashgrid_bwd_input", M, L, log2T, F, 0, interp, res, r)) return rc;
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(x01 && grad_out && table && grad_x, "acn_hashgrid_bwd_input: NULL pointer");
    const dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
    if (interp == 0) {  // rint() is piecewise constant: the gradient is exactly 0
        hipLaunchKernelGGL(zero_f32, blocks(3 * M), block, 0, s, grad_x, 3 * M);
    } else with_lerp(interp, [&](auto i) {
        constexpr int I = decltype(i)::value;
        if (F == 2 && table_fits_buffer(L, log2T)) {
            with_bool((L & (L - 1)) == 0, [&](auto tree) {
                constexpr bool TREE = decltype(tree)::value;
                hipLaunchKernelGGL((hashgrid_bwd_input_f2<I, TREE>), blocks(TREE ? M * L : M), block, 0, s, x01, M,
                                   (const float2*)grad_out, (const float2*)table, r, L, log2T, grad_x);
            });
        } else {
            hipLaunchKernelGGL(hashgrid_bwd_input_gen<I>, blocks(M), block, 0, s, x01, M, grad_out, table, r, L, log2T, F, grad_x);
        }
    });
    return acn_check_launch("acn_hashgrid_bwd_input");
}

extern "C" int acn_hashgrid_bwd_input_bwd(const float* x01, int64_t M, const float* grad_out, const float* gg_x,
                                          const float* table, const int32_t* res, int L, int log2T, int F, int interp,
                                          float* gg_out, float* g_x, void* stream) {
    Res32 r;
    if (const int rc = check_grid("acn_hashgrid_bwd_input_bwd", M, L, log2T, F, 0, interp, res, r)) return rc;
    if (M == 0 || (!gg_out && !g_x)) return ACN_OK;
    ACN_REQUIRE(x01 && grad_out && gg_x && table, "acn_hashgrid_bwd_input_bwd: NULL pointer");
    const dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
    if (interp == 0) {  // the input gradient is identically 0: so are its derivatives
        if (gg_out) hipLaunchKernelGGL(zero_f32, blocks(M * L * F), block, 0, s, gg_out, M * L * F);
        if (g_x) hipLaunchKernelGGL(zero_f32, blocks(3 * M), block, 0, s, g_x, 3 * M);
    } else with_lerp(interp, [&](auto i) {
        constexpr int I = decltype(i)::value;
        if (F == 2 && table_fits_buffer(L, log2T)) {
            with_bool((L & (L - 1)) == 0, [&](auto tree) {
                constexpr bool TREE = decltype(tree)::value;
                hipLaunchKernelGGL((hashgrid_bwd_input_bwd_f2<I, TREE>), blocks(TREE ? M * L : M), block, 0, s, x01, M,
                                   (const float2*)grad_out, gg_x, (const float2*)table, r, L, log2T, (float2*)gg_out, g_x);
            });
        } else {
            hipLaunchKernelGGL(hashgrid_bwd_input_bwd_gen<I>, blocks(M), block, 0, s, x01, M, grad_out, gg_x, table, r, L, log2T, F, gg_out, g_x);
        }
    });
    return acn_check_launch("acn_hashgrid_bwd_input_bwd");
}

extern "C" int acn_hashgrid_bwd_input_bwd_table(const float* x01, int64_t M, const float* grad_out, const float* gg_x,
                                                const int32_t* res, int L, int log2T, int F, int interp,
                                                float* grad_table, void* stream) {
    Res32 r;
    if (const int rc = check_grid("acn_hashgrid_bwd_input_bwd_table", M, L, log2T, F, 0, interp, res, r)) return rc;
    if (M == 0 || interp == 0) return ACN_OK;   // Nearest: nothing depends on the table through grad_x
    ACN_REQUIRE(x01 && grad_out && gg_x && grad_table, "acn_hashgrid_bwd_input_bwd_table: NULL pointer");
    const dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
    with_lerp(interp, [&](auto i) {
        constexpr int I = decltype(i)::value;
        if (F == 2) {
            const int64_t waves = ((M + 3) / 4) * L;
            hipLaunchKernelGGL(hashgrid_bwd_input_bwd_table_f2<I>, blocks(waves * 64), block, 0, s, x01, M, grad_out, gg_x, r, L, log2T, grad_table);
        } else {
            hipLaunchKernelGGL(hashgrid_bwd_input_bwd_table_gen<I>, blocks(M * L), block, 0, s, x01, M, grad_out, gg_x, r, L, log2T, F, grad_table);
        }
    });
    return acn_check_launch("acn_hashgrid_bwd_input_bwd_table");
}

extern "C" int acn_sh_bwd(const float* d, int64_t M, int levels, const float* g_out, float* g_d, void* stream) {
    ACN_REQUIRE(levels >= 1 && levels <= 5, "acn_sh_bwd: Supported levels in [1, 5], got %d", levels);
    ACN_REQUIRE(M >= 0, "acn_sh_bwd: M must be >= 0");
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(d && g_out && g_d, "acn_sh_bwd: NULL pointer");
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (levels) {
        case 1: hipLaunchKernelGGL(sh_bwd_kernel<0>, grid, block, 0, s, d, M, g_out, g_d); break;
        case 2: hipLaunchKernelGGL(sh_bwd_kernel<1>, grid, block, 0, s, d, M, g_out, g_d); break;
        case 3: hipLaunchKernelGGL(sh_bwd_kernel<2>, grid, block, 0, s, d, M, g_out, g_d); break;
        case 4: hipLaunchKernelGGL(sh_bwd_kernel<3>, grid, block, 0, s, d, M, g_out, g_d); break;
        default: hipLaunchKernelGGL(sh_bwd_kernel<4>, grid, block, 0, s, d, M, g_out, g_d); break;
    }
    return acn_check_launch("acn_sh_bwd");
}

extern "C" int acn_hashgrid_fwd_pairs(const float* x01, const int32_t* pk, const int64_t* seg, int K,
                                      const float* const* tables, const int32_t* res, int L, int log2T, int interp,
                                      float* out, void* stream) {
    ACN_REQUIRE(K >= 1 && K <= acn::kMaxK && tables && res && seg && x01 && pk && out,
                "acn_hashgrid_fwd_pairs: bad arguments");
    ACN_REQUIRE(L >= 1 && L <= ACN_MAX_LEVELS && log2T >= 1 && log2T <= 30 && interp >= 0 && interp <= 2,
                "acn_hashgrid_fwd_pairs: bad grid configuration");
    const Res32 r = pack_res(res, L);
    Tables t{};
    for (int k = 0; k < K; ++k) t.t[k] = (const float2*)tables[k];
    const dim3 grid(2048), block(256);  // grid-stride to the device slot count
    hipStream_t s = (hipStream_t)stream;
    with_interp(interp, [&](auto i) {
        constexpr int I = decltype(i)::value;
        if constexpr (I != 0) {
            if (table_fits_buffer(L, log2T)) {
                hipLaunchKernelGGL((hashgrid_fwd_pairs<I, true>), grid, block, 0, s, x01, pk, seg, K, t, r, L, log2T, (float2*)out);
                return;
            }
        }
        hipLaunchKernelGGL((hashgrid_fwd_pairs<I, false>), grid, block, 0, s, x01, pk, seg, K, t, r, L, log2T, (float2*)out);
    });
    return acn_check_launch("acn_hashgrid_fwd_pairs");
}

extern "C" int acn_hashgrid_bwd_pairs(const float* x01, const int32_t* pk, const int32_t* pidx, const int64_t* seg,
                                      int K, const float* grad_out, float* const* grad_tables, const int32_t* res,
                                      int L, int log2T, int interp, void* stream) {
    return acn_hashgrid_bwd_pairs_sumsq(x01, pk, pidx, seg, K, grad_out, grad_tables, res, L, log2T, interp, nullptr,
                                        stream);
}

extern "C" int acn_hashgrid_bwd_pairs_sumsq(const float* x01, const int32_t* pk, const int32_t* pidx,
                                            const int64_t* seg, int K, const float* grad_out,
                                            float* const* grad_tables, const int32_t* res, int L, int log2T,
                                            int interp, double* table_sumsq, void* stream) {
    return acn_hashgrid_bwd_pairs_segmap(x01, pk, pidx, seg, K, grad_out, grad_tables, res, L, log2T, interp,
                                         table_sumsq, nullptr, stream);
}

extern "C" int acn_hashgrid_bwd_pairs_segmap(const float* x01, const int32_t* pk, const int32_t* pidx,
                                             const int64_t* seg, int K, const float* grad_out,
                                             float* const* grad_tables, const int32_t* res, int L, int log2T,
                                             int interp, double* table_sumsq, uint8_t* const* seg_now,
                                             void* stream) {
    ACN_REQUIRE(K >= 1 && K <= acn::kMaxK && grad_tables && res && seg && x01 && pk && pidx && grad_out,
                "acn_hashgrid_bwd_pairs: bad arguments");
    ACN_REQUIRE(L >= 1 && L <= ACN_MAX_LEVELS && log2T >= 1 && log2T <= 30 && (interp == 1 || interp == 2),
                "acn_hashgrid_bwd_pairs: Linear / Smoothstep interpolation only");
    const Res32 r = pack_res(res, L);
    GradTables t{};
    for (int k = 0; k < K; ++k) t.t[k] = grad_tables[k];
    SegMaps sm{};
    if (seg_now)
        for (int k = 0; k < K; ++k) sm.t[k] = seg_now[k];
    hipStream_t s = (hipStream_t)stream;
    with_lerp(interp, [&](auto i) {
        with_bool(table_sumsq != nullptr, [&](auto tele) {  // fixed grid (graph-replayable), strided to the slot count
            hipLaunchKernelGGL((hashgrid_bwd_pairs<decltype(i)::value, decltype(tele)::value>), dim3(2048), dim3(256), 0, s,
                               x01, pk, pidx, seg, K, grad_out, t, r, L, log2T, table_sumsq, sm);
        });
    });
    return acn_check_launch("acn_hashgrid_bwd_pairs");
}

extern "C" int acn_hashgrid_pairs_mark(const float* x01, const int32_t* pk, const int32_t* pidx, const int64_t* seg,
                                       int K, const int32_t* res, int L, int log2T, int interp,
                                       uint8_t* const* seg_now, void* stream) {
    ACN_REQUIRE(K >= 1 && K <= acn::kMaxK && res && seg && x01 && pk && pidx && seg_now,
                "acn_hashgrid_pairs_mark: bad arguments");
    ACN_REQUIRE(L >= 1 && L <= ACN_MAX_LEVELS && log2T >= 1 && log2T <= 30 && (interp == 1 || interp == 2),
                "acn_hashgrid_pairs_mark: Linear / Smoothstep interpolation only");
    const Res32 r = pack_res(res, L);
    SegMaps sm{};
    for (int k = 0; k < K; ++k) sm.t[k] = seg_now[k];
    hipStream_t s = (hipStream_t)stream;
    with_lerp(interp, [&](auto i) {
        hipLaunchKernelGGL((hashgrid_bwd_pairs<decltype(i)::value, false, true>), dim3(2048), dim3(256), 0, s, x01, pk,
                           pidx, seg, K, (const float*)nullptr, GradTables{}, r, L, log2T, (double*)nullptr, sm);
    });
    return acn_check_launch("acn_hashgrid_pairs_mark");
}
