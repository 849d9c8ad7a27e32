// acn_device.h -- device-side building blocks shared by the kernels (gfx950, wave64).
//
// All files are compiled with -ffp-contract=off: every a*b+c here rounds twice unless fmaf() is
// written explicitly, which is what keeps the hash-grid / SH / ray-geometry arithmetic bit-exact
// with the reference's chains of elementwise torch ops.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acn {

constexpr uint32_t kP1 = 2654435761u;  // models/encodings.py:275 hash primes {1, 2654435761, 805459861}
constexpr uint32_t kP2 = 805459861u;

// models/trunc_exp.py:22-41 (float32 clamp +-88.722839111)
__device__ __forceinline__ float trunc_exp(float x) {
    const float m = 88.722839111f;
    x = x < -m ? -m : x;
    x = x > m ? m : x;   // NaN passes through, as torch.clamp
    return expf(x);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch.norm(dim=-1) of a 3-vector on CPU == sqrt(fma(z,z, fma(y,y, x*x)))
__device__ __forceinline__ float norm3(float x, float y, float z) {
    return sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
}

// torch.clamp_min / clamp keeping NaN (torch semantics), unlike fmaxf/fminf
__device__ __forceinline__ float clamp_min_nan(float v, float lo) { return v < lo ? lo : v; }
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// lane l's double (l wave-uniform: two scalar readlanes)
__device__ __forceinline__ double lane_f64(double v, int l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// Inclusive scan and sum of one double per lane over the wave (the segmented per-ray scans of occ.hip and the
// distortion loss of loss.hip: one wave per ray, 64 samples per step).  Fixed order: deterministic; every lane of
// wave_sum_d ends with the same bits (each xor step adds the same two values on both sides).
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(v, off);
        if (lane >= off) v += y;
    }
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// number of leading elements of the ascending a[0..n) for which pred holds (pred true on a prefix): `steps` >=
// floor(log2 n) + 1 halvings.  a[] is read at indices < n only (the searches of resample.hip and interlevel.hip).
template <typename T, typename Pred>
__device__ __forceinline__ int prefix_count(const T* a, int n, int steps, Pred pred) {
    int lo = 0, len = n;
    for (int it = 0; it < steps; ++it) {
        const int half = len >> 1;
        const int mid = lo + half;
        if (len > 0) {
            if (pred(a[mid])) {
                lo = mid + 1;
                len -= half + 1;
            } else {
                len = half;
            }
        }
    }
    return lo;
}

// compute_mse_loss in color_space "linear" (nerfs/losses.py:10-32, color_space.py:13-19, 22-66): pred.clamp(0,1)
// against gt.clamp(0,1) -> srgb_to_linear -> clamp(0,1); float scalars and powf as the torch ops (loss.hip and
// the fused training compositing in render.hip)
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ float srgb_to_linear(float x) {
    return x <= 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f);
}
__device__ __forceinline__ float gt_linear(float g) { return clamp01(srgb_to_linear(clamp01(g))); }

// get_ray_directions (nerfs/ray_sampling.py:122-136) for pixel (i, j)
__device__ __forceinline__ void pixel_dir(int i, int j, float fx, float fy, float cx, float cy, int center,
                                          float& dx, float& dy, float& dz) {
    float fi = (float)i, fj = (float)j;
    if (center) { fi = fi + 0.5f; fj = fj + 0.5f; }
    dx = (fi - cx) / fx;
    dy = -((fj - cy) / fy);
    dz = -1.0f;
    const float n = clamp_min_nan(norm3(dx, dy, dz), 1e-12f);
    dx = dx / n; dy = dy / n; dz = dz / n;
}

// SceneBox.ray_aabb_intersect (scene_box.py:81-107): slab test with eps-signed inverse,
// clamp to [0, max_bound], misses (tmax <= tmin) tagged with invalid_value
__device__ __forceinline__ void slab(const float* o, const float* d, const float* aabb, float eps, float max_bound,
                                     float invalid_value, float& tmin, float& tmax) {
    float t0m = -INFINITY, t1m = INFINITY;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float rd = d[r];
        if (fabsf(rd) < eps) rd = (rd >= 0.0f) ? eps : -eps;
        const float inv = 1.0f / rd;
        const float t0 = (aabb[r] - o[r]) * inv, t1 = (aabb[3 + r] - o[r]) * inv;
        t0m = fmaxf(t0m, fminf(t0, t1));
        t1m = fminf(t1m, fmaxf(t0, t1));
    }
    tmin = fminf(fmaxf(t0m, 0.0f), max_bound);
    tmax = fminf(fmaxf(t1m, 0.0f), max_bound);
    if (tmax <= tmin) { tmin = invalid_value; tmax = invalid_value; }
}

// torch.linspace(0, 1, S)[i] (CPU and GPU kernels: start + step*i below the middle, end - step*(S-1-i)
// above, each evaluated as one fma)
__device__ __forceinline__ float linspace01(int i, int S) {
    if (S == 1) return 0.0f;
    const float step = 1.0f / (float)(S - 1);
    return i < S / 2 ? fmaf(step, (float)i, 0.0f) : fmaf(-step, (float)(S - 1 - i), 1.0f);
}

// torch.lerp(start, end, w) (ATen Lerp.h; the CPU vector kernel and the GPU kernel both end in one fma)
__device__ __forceinline__ float lerp_t(float start, float end, float w) {
    return fabsf(w) < 0.5f ? fmaf(w, end - start, start) : fmaf(w - 1.0f, end - start, end);
}

// models/encodings.py:27-81 components_from_spherical_harmonics, float32 op order of the torch
// expressions (scalar * tensor evaluated left to right).  kz: an opaque +0.0f (c + 0.0f == c for every nonzero
// coefficient) from callers inside a loop, so the coefficient pairs of packed multiplies are formed per call instead
// of being hoisted out of the loop into VGPRs (render_ws_kernel spilled them); 0 elsewhere.
template <int DEGREE>
__device__ __forceinline__ void sh_components(float x, float y, float z, float* c, float kz = 0.0f) {
    const float xx = x * x, yy = y * y, zz = z * z;
    c[0] = (0.28209479177387814f + kz);
    if (DEGREE > 0) {
        c[1] = (0.4886025119029199f + kz) * y;
        c[2] = (0.4886025119029199f + kz) * z;
        c[3] = (0.4886025119029199f + kz) * x;
    }
    if (DEGREE > 1) {
        c[4] = ((1.0925484305920792f + kz) * x) * y;
        c[5] = ((1.0925484305920792f + kz) * y) * z;
        c[6] = (0.9461746957575601f + kz) * zz - (0.31539156525251999f + kz);
        c[7] = ((1.0925484305920792f + kz) * x) * z;
        c[8] = (0.5462742152960396f + kz) * (xx - yy);
    }
    if (DEGREE > 2) {
        c[9] = ((0.5900435899266435f + kz) * y) * (3.0f * xx - yy);
        c[10] = (((2.890611442640554f + kz) * x) * y) * z;
        c[11] = ((0.4570457994644658f + kz) * y) * (5.0f * zz - (1.0f + kz));
        c[12] = ((0.3731763325901154f + kz) * z) * (5.0f * zz - (3.0f + kz));
        c[13] = ((0.4570457994644658f + kz) * x) * (5.0f * zz - (1.0f + kz));
        c[14] = ((1.445305721320277f + kz) * z) * (xx - yy);
        c[15] = ((0.5900435899266435f + kz) * x) * (xx - (3.0f + kz) * yy);
    }
    if (DEGREE > 3) {
        c[16] = (((2.5033429417967046f + kz) * x) * y) * (xx - yy);
        c[17] = (((1.7701307697799304f + kz) * y) * z) * (3.0f * xx - yy);
        c[18] = (((0.9461746957575601f + kz) * x) * y) * (7.0f * zz - (1.0f + kz));
        c[19] = (((0.6690465435572892f + kz) * y) * z) * (7.0f * zz - (3.0f + kz));
        c[20] = (0.10578554691520431f + kz) * (((35.0f * zz) * zz - (30.0f + kz) * zz) + (3.0f + kz));
        c[21] = (((0.6690465435572892f + kz) * x) * z) * (7.0f * zz - (3.0f + kz));
        c[22] = ((0.47308734787878004f + kz) * (xx - yy)) * (7.0f * zz - (1.0f + kz));
        c[23] = (((1.7701307697799304f + kz) * x) * z) * (xx - (3.0f + kz) * yy);
        c[24] = (0.6258357354491761f + kz) * (xx * (xx - (3.0f + kz) * yy) - yy * (3.0f * xx - yy));
    }
}

// SHEncoder.forward (encodings.py:144-151): d / norm(d).clamp_min(1e-9), then components
template <int DEGREE>
__device__ __forceinline__ void sh_encode(float dx, float dy, float dz, float* c, float kz = 0.0f) {
    const float n = clamp_min_nan(norm3(dx, dy, dz), 1e-9f);
    sh_components<DEGREE>(dx / n, dy / n, dz / n, c, kz);
}

// Gradient of sum_c g[c] * Y_c(x, y, z) in the unit vector (x, y, z): the polynomials of sh_components
// differentiated term by term (Y_0 is constant).  Plain mul/add, accumulated in component order.
template <int DEGREE>
__device__ __forceinline__ void sh_components_bwd(float x, float y, float z, const float* g, float& gx, float& gy,
                                                  float& gz) {
    const float xx = x * x, yy = y * y, zz = z * z;
    gx = 0.0f; gy = 0.0f; gz = 0.0f;
    if (DEGREE > 0) {
        gy += 0.4886025119029199f * g[1];
        gz += 0.4886025119029199f * g[2];
        gx += 0.4886025119029199f * g[3];
    }
    if (DEGREE > 1) {
        const float k4 = 1.0925484305920792f, k6 = 0.9461746957575601f, k8 = 0.5462742152960396f;
        gx += (k4 * y) * g[4];  gy += (k4 * x) * g[4];
        gy += (k4 * z) * g[5];  gz += (k4 * y) * g[5];
        gz += ((2.0f * k6) * z) * g[6];
        gx += (k4 * z) * g[7];  gz += (k4 * x) * g[7];
        gx += ((2.0f * k8) * x) * g[8];  gy -= ((2.0f * k8) * y) * g[8];
    }
    if (DEGREE > 2) {
        const float k9 = 0.5900435899266435f, k10 = 2.890611442640554f, k11 = 0.4570457994644658f;
        const float k12 = 0.3731763325901154f, k14 = 1.445305721320277f;
        const float d3 = 3.0f * (xx - yy), z51 = 5.0f * zz - 1.0f;
        gx += ((6.0f * k9) * (x * y)) * g[9];   gy += (k9 * d3) * g[9];
        gx += (k10 * (y * z)) * g[10];  gy += (k10 * (x * z)) * g[10];  gz += (k10 * (x * y)) * g[10];
        gy += (k11 * z51) * g[11];  gz += ((10.0f * k11) * (y * z)) * g[11];
        gz += (k12 * (15.0f * zz - 3.0f)) * g[12];
        gx += (k11 * z51) * g[13];  gz += ((10.0f * k11) * (x * z)) * g[13];
        gx += ((2.0f * k14) * (x * z)) * g[14];  gy -= ((2.0f * k14) * (y * z)) * g[14];  gz += (k14 * (xx - yy)) * g[14];
        gx += (k9 * d3) * g[15];  gy -= ((6.0f * k9) * (x * y)) * g[15];
    }
    if (DEGREE > 3) {
        const float k16 = 2.5033429417967046f, k17 = 1.7701307697799304f, k18 = 0.9461746957575601f;
        const float k19 = 0.6690465435572892f, k20 = 0.10578554691520431f, k22 = 0.47308734787878004f;
        const float k24 = 0.6258357354491761f;
        const float a = 3.0f * xx - yy, b = xx - 3.0f * yy, d3 = 3.0f * (xx - yy);
        const float z71 = 7.0f * zz - 1.0f, z73 = 7.0f * zz - 3.0f, z213 = 21.0f * zz - 3.0f;
        gx += (k16 * (y * a)) * g[16];  gy += (k16 * (x * b)) * g[16];
        gx += ((6.0f * k17) * ((x * y) * z)) * g[17];  gy += (k17 * (z * d3)) * g[17];  gz += (k17 * (y * a)) * g[17];
        gx += (k18 * (y * z71)) * g[18];  gy += (k18 * (x * z71)) * g[18];  gz += ((14.0f * k18) * ((x * y) * z)) * g[18];
        gy += (k19 * (z * z73)) * g[19];  gz += (k19 * (y * z213)) * g[19];
        gz += (k20 * (z * (140.0f * zz - 60.0f))) * g[20];
        gx += (k19 * (z * z73)) * g[21];  gz += (k19 * (x * z213)) * g[21];
        gx += ((2.0f * k22) * (x * z71)) * g[22];  gy -= ((2.0f * k22) * (y * z71)) * g[22];
        gz += ((14.0f * k22) * ((xx - yy) * z)) * g[22];
        gx += (k17 * (z * d3)) * g[23];  gy -= ((6.0f * k17) * ((x * y) * z)) * g[23];  gz += (k17 * (x * b)) * g[23];
        gx += ((4.0f * k24) * (x * b)) * g[24];  gy -= ((4.0f * k24) * (y * a)) * g[24];
    }
}

// One level of HashGridEncoder._torch_forward split in two halves so that callers can keep the
// gathers of several levels in flight: hash_issue computes the 8 corner rows and issues their
// loads, hash_finish interpolates once they have landed.  Same arithmetic as hash_level_f2.
struct HashPending {
    float2 f[8];
    float wx, wy, wz;
};

template <int INTERP>
__device__ __forceinline__ void hash_issue(const float2* __restrict__ tl, float sx, float sy, float sz,
                                           uint32_t mask, HashPending& p) {
    if (INTERP == 0) {
        const uint32_t ix = (uint32_t)(int)rintf(sx), iy = (uint32_t)(int)rintf(sy), iz = (uint32_t)(int)rintf(sz);
        p.f[0] = tl[(ix ^ (iy * kP1) ^ (iz * kP2)) & mask];
        return;
    }
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * kP1, y1 = y0 + kP1;
    const uint32_t z0 = (uint32_t)(int)fz * kP2, z1 = z0 + kP2;
    const uint32_t x1 = x0 + 1u;
    if (INTERP == 2) {
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
    const uint32_t a00 = y0 ^ z0, a01 = y0 ^ z1, a10 = y1 ^ z0, a11 = y1 ^ z1;
    p.f[0] = tl[(x0 ^ a00) & mask];
    p.f[1] = tl[(x1 ^ a00) & mask];
    p.f[2] = tl[(x0 ^ a01) & mask];
    p.f[3] = tl[(x1 ^ a01) & mask];
    p.f[4] = tl[(x0 ^ a10) & mask];
    p.f[5] = tl[(x1 ^ a10) & mask];
    p.f[6] = tl[(x0 ^ a11) & mask];
    p.f[7] = tl[(x1 ^ a11) & mask];
    p.wx = wx;
    p.wy = wy;
    p.wz = wz;
}

// Both features at once on packed fp32 (v_pk_mul_f32 / v_pk_add_f32: per-component IEEE, the reference's
// f0*(1-w) + f1*w roundings), written as vectors so the packing needs no SLP pass.
// f index: bit0 = x1, bit1 = z1, bit2 = y1 (issue order above)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <int INTERP>
__device__ __forceinline__ void hash_finish(const HashPending& p, float& o0, float& o1) {
    if (INTERP == 0) {
        o0 = p.f[0].x;
        o1 = p.f[0].y;
        return;
    }
    const float wx = p.wx, wy = p.wy, wz = p.wz;
    const float ax = 1.0f - wx, ay = 1.0f - wy, az = 1.0f - wz;
    auto v2 = [](float2 f) { return f32x2_t{f.x, f.y}; };
    auto lerp2 = [](f32x2_t a, f32x2_t b, float w, float aw) {
        return a * f32x2_t{aw, aw} + b * f32x2_t{w, w};
    };
    const f32x2_t c00 = lerp2(v2(p.f[0]), v2(p.f[1]), wx, ax);
    const f32x2_t c01 = lerp2(v2(p.f[2]), v2(p.f[3]), wx, ax);
    const f32x2_t c10 = lerp2(v2(p.f[4]), v2(p.f[5]), wx, ax);
    const f32x2_t c11 = lerp2(v2(p.f[6]), v2(p.f[7]), wx, ax);
    const f32x2_t c0 = lerp2(c00, c10, wy, ay);
    const f32x2_t c1 = lerp2(c01, c11, wy, ay);
    const f32x2_t o = lerp2(c0, c1, wz, az);
    o0 = o[0];
    o1 = o[1];
}

// Buffer-resource form of hash_issue/hash_finish (Linear/Smoothstep).  The x-neighbours of a
// (y, z) corner pair hash to rows i0 = x0^a and i1 = x1^a; for even x0, i1 = i0 ^ 1, so ONE
// 16-byte gather of the aligned block holding i0 returns both.  The second gather (8 bytes, row
// i1) is only needed by lanes with odd x0: the other lanes pass an out-of-range offset, which the
// buffer's range check turns into a no-op (no cache access).
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
struct HashPendingX {
    u32x4_t q[4];
    u32x2_t r[4];
    float wx, wy, wz;
    uint32_t sel;  // bit c: row i0 of corner pair c is the odd row of its block; bit 4: x0 odd
};

template <int INTERP>
__device__ __forceinline__ void hash_issue_x(__amdgpu_buffer_rsrc_t rs, uint32_t lvbase, float sx, float sy, float sz,
                                             uint32_t mask, HashPendingX& p) {
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * kP1, y1 = y0 + kP1;
    const uint32_t z0 = (uint32_t)(int)fz * kP2, z1 = z0 + kP2;
    const uint32_t x1 = x0 + 1u;
    if (INTERP == 2) {
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
    const uint32_t aa[4] = {y0 ^ z0, y0 ^ z1, y1 ^ z0, y1 ^ z1};
    const bool xodd = (x0 & 1u) != 0u;
    uint32_t sel = xodd ? 16u : 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t i0 = (x0 ^ aa[c]) & mask;
        sel |= (i0 & 1u) << c;
        p.q[c] = __builtin_amdgcn_raw_buffer_load_b128(rs, lvbase + ((i0 & ~1u) << 3), 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t i1 = (x1 ^ aa[c]) & mask;
        p.r[c] = __builtin_amdgcn_raw_buffer_load_b64(rs, xodd ? lvbase + (i1 << 3) : 0xFFFFFFF0u, 0, 0);
    }
    p.wx = wx;
    p.wy = wy;
    p.wz = wz;
    p.sel = sel;
}

// The 8 corner rows of a landed hash_issue_x, in hash_issue's order (f index: bit0 = x1, bit1 = z1, bit2 = y1), for
// callers that need the rows themselves (the input-gradient kernel, encoders.hip).  The weights are not copied.
__device__ __forceinline__ void hash_rows_x(const HashPendingX& p, float2 (&f)[8]) {
    const bool xodd = (p.sel & 16u) != 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool hi = ((p.sel >> c) & 1u) != 0u;
        const u32x4_t q = p.q[c];
        const uint32_t l0 = hi ? q[2] : q[0], l1 = hi ? q[3] : q[1];
        const uint32_t e0 = hi ? q[0] : q[2], e1 = hi ? q[1] : q[3];
        f[2 * c] = make_float2(__uint_as_float(l0), __uint_as_float(l1));
        f[2 * c + 1] = make_float2(__uint_as_float(xodd ? p.r[c][0] : e0), __uint_as_float(xodd ? p.r[c][1] : e1));
    }
}

template <int INTERP>
__device__ __forceinline__ void hash_finish_x(const HashPendingX& p, float& o0, float& o1) {
    HashPending h;
    const bool xodd = (p.sel & 16u) != 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool hi = ((p.sel >> c) & 1u) != 0u;
        const u32x4_t q = p.q[c];
        const uint32_t l0 = hi ? q[2] : q[0], l1 = hi ? q[3] : q[1];
        const uint32_t e0 = hi ? q[0] : q[2], e1 = hi ? q[1] : q[3];
        h.f[2 * c] = make_float2(__uint_as_float(l0), __uint_as_float(l1));
        h.f[2 * c + 1] = make_float2(__uint_as_float(xodd ? p.r[c][0] : e0), __uint_as_float(xodd ? p.r[c][1] : e1));
    }
    h.wx = p.wx;
    h.wy = p.wy;
    h.wz = p.wz;
    hash_finish<INTERP>(h, o0, o1);
}

// Point derivative of one hash-grid level (the input-gradient kernels of encoders.hip and field_sigma_grad_kernel,
// mlp_train.hip): v[] are the corner values folded over the features (v_corner = sum_f g_f * row_f) in hash_issue's
// order (bit0 = x1, bit1 = z1, bit2 = y1), w the raw (unsmoothed) weights, r the level's resolution.  d/dw_z is the
// difference of the two z-planes, d/dw_y the z-lerp of the y-differences of the x-lerps, d/dw_x the y -> z lerp of the
// four x-differences; dw/dx = r (Linear) or r * 6 w (1 - w) (Smoothstep).
struct LevelGrad {
    float x, y, z;
};

template <int INTERP>
__device__ __forceinline__ LevelGrad level_grad(const float (&v)[8], float wx, float wy, float wz, float r) {
    float dx = r, dy = r, dz = r;
    if (INTERP == 2) {
        dx = r * ((6.0f * wx) * (1.0f - wx));
        dy = r * ((6.0f * wy) * (1.0f - wy));
        dz = r * ((6.0f * wz) * (1.0f - wz));
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
    const float ax = 1.0f - wx, ay = 1.0f - wy, az = 1.0f - wz;
    const float c00 = v[0] * ax + v[1] * wx, c01 = v[2] * ax + v[3] * wx;   // c{y}{z}: the forward's x-lerps
    const float c10 = v[4] * ax + v[5] * wx, c11 = v[6] * ax + v[7] * wx;
    const float c0 = c00 * ay + c10 * wy, c1 = c01 * ay + c11 * wy;
    const float d00 = v[1] - v[0], d01 = v[3] - v[2], d10 = v[5] - v[4], d11 = v[7] - v[6];
    const float gx = (d00 * ay + d10 * wy) * az + (d01 * ay + d11 * wy) * wz;
    const float gy = (c10 - c00) * az + (c11 - c01) * wz;
    const float gz = c1 - c0;
    return LevelGrad{dx * gx, dy * gy, dz * gz};
}

// The INTERP template value of the fused field also carries the table's storage format: 0 nearest, 1 linear,
// 2 smoothstep on the fp32 table; 3 linear, 4 smoothstep on an fp16 copy of it (acn_expert.table_fmt; there is no
// fp16 nearest).  The format is a compile-time property: one gather body per instantiation.
constexpr int kInterpLinearF16 = 3, kInterpSmoothstepF16 = 4;
constexpr bool interp_smooth(int interp) { return interp == 2 || interp == kInterpSmoothstepF16; }
constexpr bool interp_f16(int interp) { return interp >= kInterpLinearF16; }

// fp16 form of hash_issue_x / hash_finish_x: a row is two halves (4 bytes), so the x-paired block of rows
// {i0 & ~1, i0 | 1} is ONE 8-byte gather and the second row of the odd-x0 lanes ONE 4-byte gather (out-of-range offset
// for the others, as above).  Half the bytes in flight per level (12 dwords against 24), twice the rows per 128-B line.
// The landed halves are widened with v_cvt_f32_f16, which is exact (fp16 subnormals included), and go through
// hash_finish unchanged: the result equals, bit for bit, the fp32 gather of table.half().float().
struct HashPendingH {
    u32x2_t q[4];
    uint32_t r[4];
    float wx, wy, wz;
    uint32_t sel;  // as HashPendingX
};

template <int INTERP>
__device__ __forceinline__ void hash_issue_h(__amdgpu_buffer_rsrc_t rs, uint32_t lvbase, float sx, float sy, float sz,
                                             uint32_t mask, HashPendingH& p) {
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * kP1, y1 = y0 + kP1;
    const uint32_t z0 = (uint32_t)(int)fz * kP2, z1 = z0 + kP2;
    const uint32_t x1 = x0 + 1u;
    if (interp_smooth(INTERP)) {
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
    const uint32_t aa[4] = {y0 ^ z0, y0 ^ z1, y1 ^ z0, y1 ^ z1};
    const bool xodd = (x0 & 1u) != 0u;
    uint32_t sel = xodd ? 16u : 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t i0 = (x0 ^ aa[c]) & mask;
        sel |= (i0 & 1u) << c;
        p.q[c] = __builtin_amdgcn_raw_buffer_load_b64(rs, lvbase + ((i0 & ~1u) << 2), 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t i1 = (x1 ^ aa[c]) & mask;
        p.r[c] = __builtin_amdgcn_raw_buffer_load_b32(rs, xodd ? lvbase + (i1 << 2) : 0xFFFFFFF0u, 0, 0);
    }
    p.wx = wx;
    p.wy = wy;
    p.wz = wz;
    p.sel = sel;
}

// one fp16 table row (low half = feature 0, high half = feature 1) widened to fp32
__device__ __forceinline__ float2 row_f16(uint32_t v) {
    return make_float2((float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xFFFFu)),
                       (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)));
}

template <int INTERP>
__device__ __forceinline__ void hash_finish_h(const HashPendingH& p, float& o0, float& o1) {
    HashPending h;
    const bool xodd = (p.sel & 16u) != 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool hi = ((p.sel >> c) & 1u) != 0u;
        const u32x2_t q = p.q[c];
        const uint32_t l = hi ? q[1] : q[0], e = hi ? q[0] : q[1];
        h.f[2 * c] = row_f16(l);
        h.f[2 * c + 1] = row_f16(xodd ? p.r[c] : e);
    }
    h.wx = p.wx;
    h.wy = p.wy;
    h.wz = p.wz;
    hash_finish<INTERP>(h, o0, o1);
}

// One level of HashGridEncoder._torch_forward (encodings.py:331-381) for one point.
// tl: this level's table base (row = F floats).  INTERP: 0 nearest, 1 linear, 2 smoothstep.
// Linear/Smoothstep lerp order x -> y -> z exactly as encodings.py:373-379.
template <int INTERP>
__device__ __forceinline__ void hash_level_f2(const float2* __restrict__ tl, float sx, float sy, float sz,
                                              uint32_t mask, float& o0, float& o1) {
    if (INTERP == 0) {
        const uint32_t ix = (uint32_t)(int)rintf(sx), iy = (uint32_t)(int)rintf(sy), iz = (uint32_t)(int)rintf(sz);
        const float2 e = tl[(ix ^ (iy * kP1) ^ (iz * kP2)) & mask];
        o0 = e.x;
        o1 = e.y;
        return;
    }
    const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
    float wx = sx - fx, wy = sy - fy, wz = sz - fz;
    const uint32_t x0 = (uint32_t)(int)fx;
    const uint32_t y0 = (uint32_t)(int)fy * kP1, y1 = y0 + kP1;   // (iy+1)*P1 == iy*P1 + P1 mod 2^32
    const uint32_t z0 = (uint32_t)(int)fz * kP2, z1 = z0 + kP2;
    const uint32_t x1 = x0 + 1u;
    if (INTERP == 2) {
        wx = (wx * wx) * (3.0f - 2.0f * wx);
        wy = (wy * wy) * (3.0f - 2.0f * wy);
        wz = (wz * wz) * (3.0f - 2.0f * wz);
    }
    const uint32_t a00 = y0 ^ z0, a01 = y0 ^ z1, a10 = y1 ^ z0, a11 = y1 ^ z1;
    const float2 f000 = tl[(x0 ^ a00) & mask];
    const float2 f100 = tl[(x1 ^ a00) & mask];
    const float2 f001 = tl[(x0 ^ a01) & mask];
    const float2 f101 = tl[(x1 ^ a01) & mask];
    const float2 f010 = tl[(x0 ^ a10) & mask];
    const float2 f110 = tl[(x1 ^ a10) & mask];
    const float2 f011 = tl[(x0 ^ a11) & mask];
    const float2 f111 = tl[(x1 ^ a11) & mask];
    const float ax = 1.0f - wx, ay = 1.0f - wy, az = 1.0f - wz;
    {
        const float c00 = f000.x * ax + f100.x * wx;
        const float c01 = f001.x * ax + f101.x * wx;
        const float c10 = f010.x * ax + f110.x * wx;
        const float c11 = f011.x * ax + f111.x * wx;
        const float c0 = c00 * ay + c10 * wy;
        const float c1 = c01 * ay + c11 * wy;
        o0 = c0 * az + c1 * wz;
    }
    {
        const float c00 = f000.y * ax + f100.y * wx;
        const float c01 = f001.y * ax + f101.y * wx;
        const float c10 = f010.y * ax + f110.y * wx;
        const float c11 = f011.y * ax + f111.y * wx;
        const float c0 = c00 * ay + c10 * wy;
        const float c1 = c01 * ay + c11 * wy;
        o1 = c0 * az + c1 * wz;
    }
}

// ------------------------------------------------------------------------------------------
// shared by the fused render (render.hip) and the routed training sampler (routed.hip); Cfg is any
// struct with K, cluster_2d, bm, cent[k][3]
// Routing (meta_container.py:97-134), cdist mm-path restated exactly as in the oracle.
// Computed without per-expert arrays (runtime-indexed arrays would live in scratch): a first
// pass gives min distance / denominator (soft) or argmin (hard), then w_k is recomputed per k.
// squared centroid distance of the cdist mm-path, clamped at 0 (NaN -> 0); route_dist = its square root
template <typename Cfg>
__device__ __forceinline__ float route_dist2(const Cfg& cfg, int k, float px, float py, float pz) {
    float s = 0.0f, xn, cn;
    if (cfg.cluster_2d) {
        const float cy = cfg.cent[k][1], cz = cfg.cent[k][2];
        xn = py * py + pz * pz;
        cn = cy * cy + cz * cz;
        s = fmaf(-2.0f * py, cy, s);
        s = fmaf(-2.0f * pz, cz, s);
    } else {
        const float cx = cfg.cent[k][0], cy = cfg.cent[k][1], cz = cfg.cent[k][2];
        xn = (px * px + py * py) + pz * pz;
        cn = (cx * cx + cy * cy) + cz * cz;
        s = fmaf(-2.0f * px, cx, s);
        s = fmaf(-2.0f * py, cy, s);
        s = fmaf(-2.0f * pz, cz, s);
    }
    s = s + xn;
    s = s + cn;
    return s > 0.0f ? s : 0.0f;
}
template <typename Cfg>
__device__ __forceinline__ float route_dist(const Cfg& cfg, int k, float px, float py, float pz) {
    return sqrtf(route_dist2(cfg, k, px, py, pz));
}

struct RouteState {
    float thr, den;  // soft: bm * min dist, sum of masked inverse distances
    int hard;        // hard: argmin
    float thr2;      // soft: thr^2 (1 + 1e-3); a squared distance above it is outside the margin for sure
};
// A squared distance s > thr^2 (1 + 1e-3) (the products rounded ~1e-7 relative) has fl(sqrt(s)) > thr -- sqrt is
// correctly rounded and monotonic -- so its expert is outside the margin (w = 0 exactly) without the square root.
__device__ __forceinline__ float route_thr2(float thr) { return (thr * thr) * 1.001f; }

template <int ROUTE, typename Cfg>
__device__ __forceinline__ RouteState route_prep(const Cfg& cfg, float px, float py, float pz) {
    RouteState st{0.0f, 0.0f, 0, 0.0f};
    if (ROUTE == 1) {
        // min_k max(sqrt(s_k), 1e-6) = max(sqrt(min_k s_k), 1e-6) (monotonic): one square root, not K
        float mins = INFINITY;
        for (int k = 0; k < cfg.K; ++k) mins = fminf(mins, route_dist2(cfg, k, px, py, pz));
        float mind = sqrtf(mins);
        mind = mind < 1e-6f ? 1e-6f : mind;
        st.thr = cfg.bm * mind;
        st.thr2 = route_thr2(st.thr);
        float den = 0.0f;
        for (int k = 0; k < cfg.K; ++k) {
            const float s2 = route_dist2(cfg, k, px, py, pz);
            if (s2 > st.thr2) continue;   // outside the margin: adds 0
            float d = sqrtf(s2);
            d = d < 1e-6f ? 1e-6f : d;
            den = den + ((d <= st.thr) ? 1.0f / d : 0.0f);
        }
        st.den = den < 1e-6f ? 1e-6f : den;
    } else if (ROUTE == 2) {
        float best = INFINITY;
        for (int k = 0; k < cfg.K; ++k) {
            const float d = route_dist(cfg, k, px, py, pz);
            if (d < best || k == 0) { best = d; st.hard = k; }
        }
    }
    return st;
}

template <typename Cfg>
__device__ __forceinline__ float route_weight(const Cfg& cfg, const RouteState& st, int k, float px, float py,
                                              float pz) {
    const float s2 = route_dist2(cfg, k, px, py, pz);
    if (s2 > st.thr2) return 0.0f;   // = 0 / den
    float d = sqrtf(s2);
    d = d < 1e-6f ? 1e-6f : d;
    return ((d <= st.thr) ? 1.0f / d : 0.0f) / st.den;
}

// colour-branch direction encoding (meta_ngp.py:165-168 then encodings.py:144-151)
__device__ __forceinline__ void dir_sh(float dx, float dy, float dz, float (&sh)[16], float kz = 0.0f) {
    const float n = clamp_min_nan(norm3(dx, dy, dz), 1e-9f);
    sh_encode<3>(dx / n, dy / n, dz / n, sh, kz);
}

// t value of sample s (stratified_t_vals, ray_rendering.py:278-287); linspace as torch CPU
__device__ __forceinline__ float lin01(int i, int S) {
    if (S == 1) return 0.0f;
    const float step = 1.0f / (float)(S - 1);
    return i < S / 2 ? fmaf(step, (float)i, 0.0f) : fmaf(-step, (float)(S - 1 - i), 1.0f);
}
__device__ __forceinline__ float tlin(float near, float far, int i, int S) {
    const float u = lin01(i, S);
    return near * (1.0f - u) + far * u;
}
__device__ __forceinline__ float tval(float near, float far, int s, int S, const float* jit) {
    const float ts = tlin(near, far, s, S);
    if (!jit) return ts;
    const float lo = s == 0 ? ts : 0.5f * (tlin(near, far, s - 1, S) + ts);
    const float hi = s == S - 1 ? ts : 0.5f * (ts + tlin(near, far, s + 1, S));
    return lo + (hi - lo) * jit[s];
}

// fp16 MFMA operand fragment.  Round 5 took rare run-to-run differences of the renders for stale fp16 B operands and
// put every fragment through a VALU -> MFMA operand fence (16 wait states in one asm statement); round 6 found the
// cause in the hash gathers issued as global loads and removed the fence, which cost the meta step 5% and changed
// nothing (hipcc's own padding is audited by tests/test_hazard_audit.py).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

}  // namespace acn
