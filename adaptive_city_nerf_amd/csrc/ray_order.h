// ray_order.h -- the direction-cell visiting order of a small batch (N <= ACN_ORDER_MAX), shared by
// ray_order_kernel (the whole order, one workgroup) and render_ws_kernel's selection prologue (every render
// workgroup derives the rays of its own windows of that order).  Included by render.hip only.
//
// The order: rays grouped by direction, so that the XCD bands of the render kernels become compact image
// regions (a random pixel batch otherwise spreads every XCD's samples over the whole frame and its 4 MB L2
// serves the hash cells of all of it).  A frame = the batch's mean direction m and an orthonormal pair
// (e1, e2) perpendicular to it; every ray's gnomonic coordinates (d.e1 / d.m, d.e2 / d.m) (for one camera:
// its image-plane position), quantised to a 64 x 64 grid over a bounding box and Z-ordered; rays sorted by
// (cell, ray index).  Only the order changes: each ray is still rendered alone and its outputs written at
// its own index, so results are bit-identical to the given order.  Rays with a non-finite direction or
// d.m <= 0 go to the last cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ACN_ORDER_MAX 8192
#define ACN_ORDER_BINS 4096

// Z-order cell of two 6-bit grid coordinates: both spread in the halves of one register (bit k -> bit 2 k)
__device__ __forceinline__ uint32_t morton6(uint32_t qu, uint32_t qv) {
    uint32_t t = qu | (qv << 16);
    t = (t | (t << 4)) & 0x030F030Fu;
    t = (t | (t << 2)) & 0x03330333u;
    t = (t | (t << 1)) & 0x05550555u;
    return (t | (t >> 15)) & 0xFFFu;
}
// workgroup-wide reductions (1024 threads = 16 waves) of 3 sums / 4 maxima; every thread gets the result
// DPP within each 16-lane row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror), then the
// four row results through scalar readlanes: no LDS round trips (a ds_bpermute shuffle ladder costs six
// dependent LDS latencies per value)
template <int OP>
__device__ __forceinline__ float wave_reduce(float v) {
    auto op = [](float a, float b) { return OP == 0 ? a + b : fmaxf(a, b); };
    v = op(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));
    v = op(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));
    v = op(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));
    v = op(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return op(op(r0, r1), op(r2, r3));
}
// TRAIL: the barrier after the reads, for callers that use red[] again
template <int OP, bool TRAIL = true>
__device__ __forceinline__ void block_reduce3(float& a, float& b, float& c, float* red) {
    a = wave_reduce<OP>(a), b = wave_reduce<OP>(b), c = wave_reduce<OP>(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = a, red[16 + w] = b, red[32 + w] = c;
    __syncthreads();
    a = red[0], b = red[16], c = red[32];
    for (int k = 1; k < 16; ++k) a += red[k], b += red[16 + k], c += red[32 + k];
    if (TRAIL) __syncthreads();  // red[] reuse
}
template <bool TRAIL = true>
__device__ __forceinline__ void block_reduce4max(float& a, float& b, float& c, float& d, float* red) {
    a = wave_reduce<1>(a), b = wave_reduce<1>(b), c = wave_reduce<1>(c), d = wave_reduce<1>(d);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = a, red[16 + w] = b, red[32 + w] = c, red[48 + w] = d;
    __syncthreads();
    for (int k = 0; k < 16; ++k)
        a = fmaxf(a, red[k]), b = fmaxf(b, red[16 + k]), c = fmaxf(c, red[32 + k]), d = fmaxf(d, red[48 + k]);
    if (TRAIL) __syncthreads();
}
// inclusive scan over the 64 lanes (DPP row shifts, then the row broadcasts)
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return v;
}
__device__ __forceinline__ bool dir_ok(float x, float y, float z) {
    const float n2 = x * x + y * y + z * z;
    return n2 > 0.0f && n2 < 3.0e38f;  // finite, non-zero
}

// ---- the per-ray cell: frame, gnomonic coordinates, quantiser (one definition for both kernels; with
// -ffp-contract=off the same inputs give the same cell wherever this is inlined)
struct OrderFrame {
    float mx, my, mz, e1x, e1y, e1z, e2x, e2y, e2z;
};
// These run once per ray in every render workgroup, which is bound by its instruction count there: straight-line
// code, selects instead of branches (a comparison with a NaN is false, so a bad ray drops out by itself).
// a ray's term of the mean direction: its unit direction (+0 for a non-finite or zero one)
__device__ __forceinline__ void order_accum_dir(float x, float y, float z, float& sx, float& sy, float& sz) {
    const float n2 = x * x + y * y + z * z;
    const bool ok = n2 > 0.0f && n2 < 3.0e38f;
    const float r = rsqrtf(ok ? n2 : 1.0f);
    sx += ok ? x * r : 0.0f, sy += ok ? y * r : 0.0f, sz += ok ? z * r : 0.0f;
}
// the frame of a sum of unit directions
__device__ __forceinline__ OrderFrame order_frame(float sx, float sy, float sz) {
    const float mn = sqrtf(sx * sx + sy * sy + sz * sz);
    float mx = 0.0f, my = 0.0f, mz = 1.0f;
    if (mn > 0.0f && mn < 3.0e38f) mx = sx / mn, my = sy / mn, mz = sz / mn;
    // e1 = normalize(m x a) with a the axis least aligned with m; e2 = m x e1
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (fabsf(mx) <= fabsf(my) && fabsf(mx) <= fabsf(mz)) ax = 1.0f;
    else if (fabsf(my) <= fabsf(mz)) ay = 1.0f;
    else az = 1.0f;
    float e1x = my * az - mz * ay, e1y = mz * ax - mx * az, e1z = mx * ay - my * ax;
    const float e1n = rsqrtf(e1x * e1x + e1y * e1y + e1z * e1z);
    e1x *= e1n, e1y *= e1n, e1z *= e1n;
    const float e2x = my * e1z - mz * e1y, e2y = mz * e1x - mx * e1z, e2z = mx * e1y - my * e1x;
    return OrderFrame{mx, my, mz, e1x, e1y, e1z, e2x, e2y, e2z};
}
__device__ __forceinline__ bool order_coords(const OrderFrame& f, float x, float y, float z, float& u, float& v) {
    const float dm = x * f.mx + y * f.my + z * f.mz;
    // one v_rcp_f32 (1 ulp) instead of two correctly rounded divisions: the cell needs 6 bits of each coordinate,
    // and the instruction gives every workgroup the same bits
    const float inv = __builtin_amdgcn_rcpf(dm);
    u = (x * f.e1x + y * f.e1y + z * f.e1z) * inv;
    v = (x * f.e2x + y * f.e2y + z * f.e2z) * inv;
    return dir_ok(x, y, z) && dm > 0.0f && fabsf(u) < 1.0e30f && fabsf(v) < 1.0e30f;
}
struct OrderBox {
    float umin, vmin, su, sv;
};
__device__ __forceinline__ OrderBox order_box(float umin, float vmin, float umax, float vmax) {
    const float su = umax > umin ? 63.999f / (umax - umin) : 0.0f;
    const float sv = vmax > vmin ? 63.999f / (vmax - vmin) : 0.0f;
    return OrderBox{umin, vmin, su, sv};
}
// a ray's coordinates into a running bounding box (nothing for a ray without coordinates)
__device__ __forceinline__ void order_grow_box(bool ok, float u, float v, float& umin, float& vmin, float& umax,
                                               float& vmax) {
    umin = (ok & (u < umin)) ? u : umin, umax = (ok & (u > umax)) ? u : umax;
    vmin = (ok & (v < vmin)) ? v : vmin, vmax = (ok & (v > vmax)) ? v : vmax;
}
// coordinates outside the box clamp to its border cells
__device__ __forceinline__ int order_cell(bool ok, float u, float v, const OrderBox& b) {
    const uint32_t qu = (uint32_t)fminf(fmaxf((u - b.umin) * b.su, 0.0f), 63.0f);
    const uint32_t qv = (uint32_t)fminf(fmaxf((v - b.vmin) * b.sv, 0.0f), 63.0f);
    return ok ? (int)morton6(qu, qv) : ACN_ORDER_BINS - 1;
}

// ------------------------------------------------------------------------------------------
// Selection prologue of render_ws_kernel.  A render workgroup needs the 16 rays of each of its own windows
// [first + k stride, +16) of the order, not the order: every workgroup computes every ray's cell (the same
// code on the same inputs: identical in all workgroups), a histogram and its scan give every cell's first
// position, the rays of the cells that overlap a window become candidates, and a candidate's position is
// its cell's first position plus the number of candidates of that cell with a smaller index.  No scatter,
// no order[] in global memory, no second launch, nothing between workgroups.
//
// Frame (EXACT = false): mean direction and bounding box of 256 rays, every ceil(N / 256)-th, reduced by
// every wave for itself in registers (no barrier; the same 256 loads in every wave).  Rays outside that box
// clamp to its border cells.  EXACT = true: ray_order_kernel's two workgroup reductions over all rays (the
// same partial sums and tree, so the same cells as ray_order_kernel).
//
// A cell holding more than kSelCell rays (many identical directions) leaves the candidate list: every
// workgroup sees the same histogram, so all take the same branch, and the branch ranks a window cell's ray
// by counting the cell's rays below it over all of cell_of[] -- the same positions, slower.
constexpr int kSelRounds = 2;                  // windows per workgroup the slot table holds (8192 rays on 256 CUs)
constexpr int kSelPer = ACN_ORDER_MAX / 1024;  // rays per thread
constexpr int kSelCell = 56;                   // largest cell of the candidate path
// a 16-position window overlaps at most two cells that reach outside it (<= kSelCell rays each, one position
// inside at least) and 14 positions' worth of whole cells
constexpr int kSelCand = kSelRounds * (14 + 2 * kSelCell);
constexpr int kSelFrameRays = 256;

struct SelLds {   // 34 KB, aliases render_ws_kernel's ybuf (free until the first tile is written)
    int start[ACN_ORDER_BINS + 4];   // per cell: count, then first position; start[ACN_ORDER_BINS] = N
    uint16_t cell_of[ACN_ORDER_MAX];
    uint32_t cand[kSelCand];         // cell << 16 | ray index
    int wsum[16];
    float red3[48], red4[64];        // the exact frame's two reductions, an array each: no barrier for reuse
    int ncand, big;
};
struct SelRays {   // a thread's directions: rays tid + 1024 q, and (sampled frame) frame rays (lane + 64 q) step
    float x[kSelPer], y[kSelPer], z[kSelPer];
    float fx[kSelFrameRays / 64], fy[kSelFrameRays / 64], fz[kSelFrameRays / 64];
};

// Issue the direction loads and clear the histogram.  A barrier (the weight staging's) must follow before
// ws_select_finish.
template <bool EXACT>
__device__ __forceinline__ void ws_select_begin(const float* __restrict__ rays, int N, SelRays& r, SelLds& l) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kSelPer; ++q) {
        const int i = tid + q * 1024;
        r.x[q] = r.y[q] = r.z[q] = 0.0f;
        if (i < N) {
            const float* rp = rays + (int64_t)i * 8;
            r.x[q] = rp[3], r.y[q] = rp[4], r.z[q] = rp[5];
        }
    }
    if (!EXACT) {
        const int fstep = (N + kSelFrameRays - 1) / kSelFrameRays;
#pragma unroll
        for (int q = 0; q < kSelFrameRays / 64; ++q) {
            const int i = ((tid & 63) + 64 * q) * fstep;
            r.fx[q] = r.fy[q] = r.fz[q] = 0.0f;   // a zero direction counts for nothing
            if (i < N) {
                const float* rp = rays + (int64_t)i * 8;
                r.fx[q] = rp[3], r.fy[q] = rp[4], r.fz[q] = rp[5];
            }
        }
    }
    reinterpret_cast<int4*>(l.start)[tid] = make_int4(0, 0, 0, 0);
    if (tid == 0) l.start[ACN_ORDER_BINS] = N, l.ncand = 0, l.big = 0;
}

// Fill tab[k * 16 + s] = the ray at position first + k stride + s, for the workgroup's windows k < kSelRounds
// below hi (xcd_band's first / hi / stride with 16 positions per round).  Ends with a barrier.
template <bool EXACT>
__device__ __forceinline__ void ws_select_finish(const SelRays& r, int N, int first, int hi, int stride, SelLds& l,
                                                 uint16_t* tab) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // rays per thread that exist at all (workgroup-uniform: the passes below skip the rest with a scalar branch);
    // a ray past N was loaded as a zero direction, which is no direction: it adds nothing and has no coordinates
    const int nq = min(kSelPer, (N + 1023) >> 10);
    // ---- frame and bounding box
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    float umin = 3.0e38f, vmin = 3.0e38f, umax = -3.0e38f, vmax = -3.0e38f;
    OrderFrame f;
    float cu[kSelPer], cv[kSelPer];
    bool cok[kSelPer];
    if (EXACT) {
#pragma unroll
        for (int q = 0; q < kSelPer; ++q)
            if (q < nq) order_accum_dir(r.x[q], r.y[q], r.z[q], sx, sy, sz);
        block_reduce3<0, false>(sx, sy, sz, l.red3);
        f = order_frame(sx, sy, sz);
    } else {
#pragma unroll
        for (int q = 0; q < kSelFrameRays / 64; ++q) order_accum_dir(r.fx[q], r.fy[q], r.fz[q], sx, sy, sz);
        sx = wave_reduce<0>(sx), sy = wave_reduce<0>(sy), sz = wave_reduce<0>(sz);
        f = order_frame(sx, sy, sz);
#pragma unroll
        for (int q = 0; q < kSelFrameRays / 64; ++q) {
            float u, v;
            const bool ok = order_coords(f, r.fx[q], r.fy[q], r.fz[q], u, v);
            order_grow_box(ok, u, v, umin, vmin, umax, vmax);
        }
    }
#pragma unroll
    for (int q = 0; q < kSelPer; ++q) {
        cok[q] = false, cu[q] = cv[q] = 0.0f;
        if (q < nq) {
            cok[q] = order_coords(f, r.x[q], r.y[q], r.z[q], cu[q], cv[q]);
            if (EXACT) order_grow_box(cok[q], cu[q], cv[q], umin, vmin, umax, vmax);
        }
    }
    umin = -umin, vmin = -vmin;  // one max-reduction for all four
    if (EXACT) block_reduce4max<false>(umin, vmin, umax, vmax, l.red4);
    else umin = wave_reduce<1>(umin), vmin = wave_reduce<1>(vmin), umax = wave_reduce<1>(umax), vmax = wave_reduce<1>(vmax);
    const OrderBox box = order_box(-umin, -vmin, umax, vmax);
    // ---- cells and their histogram
    int cq[kSelPer];
#pragma unroll
    for (int q = 0; q < kSelPer; ++q) {
        const int i = tid + q * 1024;
        cq[q] = ACN_ORDER_BINS - 1;
        if (q < nq) {
            cq[q] = order_cell(cok[q], cu[q], cv[q], box);
            if (i < N) {
                l.cell_of[i] = (uint16_t)cq[q];
                atomicAdd(&l.start[cq[q]], 1);
            }
        }
    }
    __syncthreads();
    // ---- scan: thread t owns cells 4 t .. 4 t + 3
    {
        const int4 c = reinterpret_cast<const int4*>(l.start)[tid];
        const int tot = c.x + c.y + c.z + c.w;
        if (max(max(c.x, c.y), max(c.z, c.w)) > kSelCell) l.big = 1;
        const int incl = wave_incl_scan(tot);
        if (lane == 63) l.wsum[w] = incl;
        __syncthreads();
        int b = incl - tot;
#pragma unroll
        for (int k = 0; k < 16; ++k) b += k < w ? l.wsum[k] : 0;   // all 16 reads in flight, not w dependent ones
        reinterpret_cast<int4*>(l.start)[tid] = make_int4(b, b + c.x, b + c.x + c.y, b + c.x + c.y + c.z);
        __syncthreads();
    }
    // the workgroup's windows [wa, wb); one that starts at or past hi is empty (wb = 0: below every position)
    int wa[kSelRounds], wb[kSelRounds];
#pragma unroll
    for (int k = 0; k < kSelRounds; ++k) {
        wa[k] = first + k * stride;
        wb[k] = wa[k] < hi ? min(wa[k] + 16, hi) : 0;
    }
    // does the position range [s0, s1) of a cell meet a window
    auto windows_hit = [&](int s0, int s1) {
        bool m = false;
#pragma unroll
        for (int k = 0; k < kSelRounds; ++k) m |= s0 < wb[k] && s1 > wa[k];
        return m;
    };
    auto place = [&](int pos, int ray) {
#pragma unroll
        for (int k = 0; k < kSelRounds; ++k)
            if (pos >= wa[k] && pos < wb[k]) tab[k * 16 + pos - wa[k]] = (uint16_t)ray;
    };
    if (!l.big) {   // workgroup-uniform, and the same in every workgroup
        bool hit[kSelPer];   // every cell range read first: one LDS latency, not one per ray
#pragma unroll
        for (int q = 0; q < kSelPer; ++q)
            hit[q] = q < nq && tid + q * 1024 < N && windows_hit(l.start[cq[q]], l.start[cq[q] + 1]);
#pragma unroll
        for (int q = 0; q < kSelPer; ++q) {
            const int i = tid + q * 1024;
            if (hit[q]) {
                const int at = atomicAdd(&l.ncand, 1);
                if (at < kSelCand) l.cand[at] = (uint32_t)cq[q] << 16 | (uint32_t)i;
            }
        }
        __syncthreads();
        const int nc = min(l.ncand, kSelCand);
        if (tid < nc) {
            const uint32_t me = l.cand[tid];
            int rk = 0;
            for (int j = 0; j < nc; ++j) {
                const uint32_t o = l.cand[j];
                rk += ((o ^ me) < 65536u && o < me) ? 1 : 0;   // same cell, smaller index
            }
            place(l.start[me >> 16] + rk, (int)(me & 0xFFFFu));
        }
    } else {
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(l.cell_of);
#pragma unroll 1
        for (int q = 0; q < kSelPer; ++q) {
            const int i = tid + q * 1024;
            if (i >= N) break;
            const uint32_t c = (uint32_t)cq[q];
            const int s0 = l.start[c];
            if (!windows_hit(s0, l.start[c + 1])) continue;
            int rk = 0;
            for (int j = 0; j < (i >> 1); ++j) {
                const uint32_t two = cw[j];
                rk += ((two & 0xFFFFu) == c ? 1 : 0) + ((two >> 16) == c ? 1 : 0);
            }
            if ((i & 1) && l.cell_of[i - 1] == c) ++rk;
            place(s0 + rk, i);
        }
    }
    __syncthreads();
}
