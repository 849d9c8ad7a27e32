// loss.hip -- the training loss of the adaptation / meta-training steps on gfx950:
//   nerfs/losses.py:10-32 compute_mse_loss = F.mse_loss(*color_space_transformer(pred, gt, "linear"))
//   nerfs/color_space.py:13-19, 22-66 (gt.clamp(0,1) -> srgb_to_linear -> clamp(0,1); pred.clamp(0,1))
// The reference evaluates this as ~11 elementwise / reduction launches forward and ~5 backward per
// render; in a meta-training step (108 renders) those 5-us launches cost more than the MLP forward.
// Here: one single-workgroup launch forward (the batch is thousands of rays; per-thread double partial
// sums, one fixed reduction order: deterministic) and one elementwise launch backward.
// Float semantics follow the torch ops: scalars as float (12.92f, 0.055f, 1.055f, 0.04045f), powf with
// the float exponent, clamps that pass NaN through, and mse_loss_backward's double `2 / numel` factor.
// Also here, as the other small per-ray reduction: acn_normal_composite, the weighted sum of the samples' unit
// normals of a rendered normal map, and the distortion regulariser of the weights along a ray with its
// gradient (acn_distortion_packed / acn_distortion_dense), and depth supervision in the same form
// (acn_depth_loss_packed / acn_depth_loss_dense).
#include "acn_device.h"
#include "acn_internal.h"

namespace {

using acn::clamp01;
using acn::gt_linear;   // gt (sRGB in [0,1] after the clamp) -> linear, clamped again

constexpr int kThreads = 1024;

__global__ void __launch_bounds__(kThreads) mse_linear_fwd_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ gt, int64_t n,
                                                                  float* __restrict__ loss) {
    __shared__ double red[kThreads / 64];
    double acc = 0.0;
    // unrolled: the loads of 8 strides are issued together (same accumulation order per thread)
#pragma unroll 8
    for (int64_t e = threadIdx.x; e < n; e += kThreads) {
        const float d = clamp01(pred[e]) - gt_linear(gt[e]);
        acc += (double)(d * d);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) t += red[i];
        loss[0] = (float)(t / (double)n);
    }
}

// Multi-workgroup form (acn_mse_linear_fwd_ws): G workgroups of 256 threads (G sized for ~2 elements per
// thread, at most 256), thread i of workgroup b sums elements b*256 + i, + G*256, ... in double; the
// workgroup sums in a fixed order into partials[b]; the last workgroup to finish (ticket counter) adds
// partials[0..G) in a fixed tree, writes the loss and resets the counter.  Deterministic (fixed assignment and
// order for a given n).  The time of this launch is memory latency, not arithmetic: a thread's loads are
// issued 4 at a time ahead of the sums (same per-thread order), and the grid is wide enough that a thread
// has one or two such rounds (8 dependent rounds per thread measured 11 us at n = 12000,
// tools/micro/loss_micro.py).
constexpr int kWsThreads = 256;
constexpr int kWsMaxBlocks = 256;
constexpr int kWsPerThread = 2;
__global__ void __launch_bounds__(kWsThreads) mse_linear_fwd_ws_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ gt, int64_t n,
                                                                       double* __restrict__ partials,
                                                                       unsigned int* __restrict__ counter,
                                                                       float* __restrict__ loss) {
    __shared__ double red[kWsThreads / 64];
    __shared__ bool last;
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kWsThreads;
    for (int64_t e = (int64_t)blockIdx.x * kWsThreads + threadIdx.x; e < n; e += 4 * stride) {
        float p[4], q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = e + u * stride;
            p[u] = i < n ? pred[i] : 0.0f;
            q[u] = i < n ? gt[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (e + u * stride < n) {
                const float d = clamp01(p[u]) - gt_linear(q[u]);
                acc += (double)(d * d);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kWsThreads / 64; ++i) t += red[i];
        partials[blockIdx.x] = t;
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    // last workgroup: thread i loads partial i (G <= 256), then a fixed xor tree per wave and the waves in order
    // (deterministic for a given n; a serial in-order sum through one wave measured ~10 us of this launch)
    if (last) {
        __threadfence();
        const unsigned int G = gridDim.x;
        double v = threadIdx.x < G ? __hip_atomic_load(&partials[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                   : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        __syncthreads();   // red[] is reused (thread 0 read it above)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double t = 0.0;
        for (int i = 0; i < kWsThreads / 64; ++i) t += red[i];
        if (threadIdx.x == 0) {
            loss[0] = (float)(t / (double)n);
            counter[0] = 0u;
        }
    }
}

// d loss / d pred: mse_loss_backward (2 / numel * (input - target) * grad_output, in double) through the
// clamp's backward (gradient where 0 <= pred <= 1)
__global__ void __launch_bounds__(256) mse_linear_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             int64_t n, const float* __restrict__ g_loss,
                                                             float* __restrict__ g_pred) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float p = pred[e];
    const float d = clamp01(p) - gt_linear(gt[e]);
    const float g = (float)((2.0 / (double)n) * (double)d * (double)g_loss[0]);
    g_pred[e] = (p >= 0.0f && p <= 1.0f) ? g : 0.0f;
}

// Normal map compositing (acn_normal_composite): n = sum_s w_s * (-g_s / max(|g_s|, 1e-9)) per ray, g_s the density
// gradient of sample s (acn_field_sigma_grad).  One lane per ray; every term in fp32 (norm3, one division and one
// product per component), accumulated in float64 in sample order and rounded once: deterministic, and a zero
// gradient (a gated sample) adds exactly 0.
__global__ void __launch_bounds__(256) normal_composite_kernel(const float* __restrict__ grad,
                                                               const float* __restrict__ weights, int64_t N, int S,
                                                               float* __restrict__ normal) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* g = grad + n * S * 3;
    const float* w = weights + n * S;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int s = 0; s < S; ++s) {
        const float gx = g[3 * s], gy = g[3 * s + 1], gz = g[3 * s + 2], ws = w[s];
        const float d = acn::clamp_min_nan(acn::norm3(gx, gy, gz), 1e-9f);
        ax += (double)(ws * (-gx / d));
        ay += (double)(ws * (-gy / d));
        az += (double)(ws * (-gz / d));
    }
    normal[3 * n] = (float)ax;
    normal[3 * n + 1] = (float)ay;
    normal[3 * n + 2] = (float)az;
}

// Distortion loss (acn_distortion_packed / acn_distortion_dense): for one ray with weights w_i over the
// intervals [s_i, s_i + d_i], midpoints m_i = s_i + d_i / 2 non-decreasing along the ray,
//   L        = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i = sum_i [ 2 w_i (m_i W_<i - WM_<i) + w_i^2 d_i / 3 ]
//   dL/dw_i  = 2 [ (m_i W_<i - WM_<i) + (WM_>i - m_i W_>i) ] + 2/3 w_i d_i
// with W, WM the prefix sums of w and w m.  One wave per ray, 64 samples per step (the shape of
// packed_weights_bwd_kernel): pass 1 sums w and w m over the ray, pass 2 walks front to back with two scans.  m W - WM
// is a difference of nearly equal numbers when t is large against the sample spacing, so the sums, carries and terms
// are double and each output is rounded to fp32 once.  No atomics, no LDS: bitwise reproducible.
// DENSE: w, t (N, S), the compositing's own intervals (s_i = t_i, d_i = max(t_{i+1} - t_i, 1e-4), the last d copied
// from its predecessor: volume_render's dists).  Packed: [t0_i, t1_i] of samples starts[r] .. + counts[r], cut at M.
struct DistortionArgs {
    const float *w, *t0, *t1;        // dense: t0 = t_vals, t1 unused
    const int64_t *starts, *counts;  // packed only
    int64_t M, N;
    int32_t S;                       // dense only
    const float* ray_scale;          // (N) or NULL
    float *loss, *grad_w;            // grad_w may be NULL
};

// midpoint and width of sample k (< n) of the ray whose first sample is b
template <bool DENSE>
__device__ __forceinline__ void distortion_interval(const DistortionArgs& a, int64_t b, int64_t k, int64_t n, double& m,
                                                    double& d) {
    if (DENSE) {
        const int64_t j = k + 1 < n ? k : n - 2;   // the last sample takes its predecessor's width (n >= 2)
        const float df = acn::clamp_min_nan(a.t0[b + j + 1] - a.t0[b + j], 1e-4f);
        d = (double)df;
        m = (double)a.t0[b + k] + 0.5 * d;
    } else {
        const double s = (double)a.t0[b + k], e = (double)a.t1[b + k];
        d = e - s;
        m = 0.5 * (s + e);
    }
}

template <bool DENSE>
__global__ void __launch_bounds__(256) distortion_kernel(DistortionArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < a.N; r += nw) {
        int64_t b, n;
        if (DENSE) {
            b = r * a.S;
            n = a.S;
        } else {
            b = a.starts[r];
            n = a.counts[r];
            if (b < 0 || b > a.M || n < 0) n = 0;   // a range outside the samples is empty, one past M is cut
            if (n > a.M - b) n = a.M - b;
        }
        const double scale = a.ray_scale ? (double)a.ray_scale[r] : 1.0;
        if (scale == 0.0) {   // wave-uniform: zeros, and the ray's t values (NaN for an invalid ray) are not read
            if (a.grad_w)
                for (int64_t k = lane; k < n; k += 64) a.grad_w[b + k] = 0.0f;
            if (lane == 0) a.loss[r] = 0.0f;
            continue;
        }
        double wt = 0.0, wmt = 0.0;   // sum of w and of w m over the ray
        for (int64_t s0 = 0; s0 < n; s0 += 64) {
            const int64_t k = s0 + lane;
            double w = 0.0, wm = 0.0;
            if (k < n) {
                double m, d;
                distortion_interval<DENSE>(a, b, k, n, m, d);
                w = (double)a.w[b + k];
                wm = w * m;
            }
            wt += acn::wave_sum_d(w);
            wmt += acn::wave_sum_d(wm);
        }
        double cw = 0.0, cwm = 0.0;   // sums over the samples before this step
        double acc = 0.0;             // this lane's share of the loss
        for (int64_t s0 = 0; s0 < n; s0 += 64) {
            const int64_t k = s0 + lane;
            const bool v = k < n;
            double w = 0.0, m = 0.0, d = 0.0;
            if (v) {
                distortion_interval<DENSE>(a, b, k, n, m, d);
                w = (double)a.w[b + k];
            }
            const double wm = w * m;
            const double iw = acn::wave_incl_scan(w, lane), iwm = acn::wave_incl_scan(wm, lane);
            if (v) {
                const double w_le = cw + iw, wm_le = cwm + iwm;   // W_<=i, WM_<=i
                const double before = m * (w_le - w) - (wm_le - wm);       // sum_{j<i} w_j (m_i - m_j)
                acc += 2.0 * w * before + w * w * d * (1.0 / 3.0);
                if (a.grad_w) {
                    const double after = (wmt - wm_le) - m * (wt - w_le);  // sum_{j>i} w_j (m_j - m_i)
                    a.grad_w[b + k] = (float)(scale * (2.0 * (before + after) + (2.0 / 3.0) * w * d));
                }
            }
            cw += __shfl(iw, 63);
            cwm += __shfl(iwm, 63);
        }
        acc = acn::wave_sum_d(acc);
        if (lane == 0) a.loss[r] = (float)(scale * acc);
    }
}

template <bool DENSE>
int launch_distortion(const DistortionArgs& a, void* stream, const char* what) {
    const int64_t wgs = (a.N + 3) / 4;   // 4 waves (rays) per 256-thread workgroup, grid-stride past 4096 of them
    hipLaunchKernelGGL(distortion_kernel<DENSE>, dim3((unsigned)(wgs < 4096 ? wgs : 4096)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return acn_check_launch(what);
}

// Depth supervision (acn_depth_loss_packed / acn_depth_loss_dense): for one ray with weights w_i over
// the intervals [s_i, e_i], per-sample depths tau_i, a target depth z, a half-width eps and a length scale c,
//   sigma = eps / 3, lo = z - eps, hi = z + eps, Phi the standard normal CDF
//   k_i      = Phi((min(e_i, hi) - z) / sigma) - Phi((max(s_i, lo) - z) / sigma) if min(e_i, hi) > max(s_i, lo), else 0
//   m_i      = 1 if s_i < hi else 0
//   D        = sum_i w_i tau_i
//   L        = l_d (c (D - z))^2 + l_s sum_i m_i (w_i - k_i)^2
//   dL/dw_i  = 2 l_d c^2 (D - z) tau_i + 2 l_s m_i (w_i - k_i)
// (the expected-depth term of DS-NeRF and the line-of-sight term of Urban Radiance Fields: k is the mass a Gaussian of
// deviation eps / 3 cut at +-eps puts into interval i; samples in front of the window pay w^2, samples behind it
// nothing).  The shape of distortion_kernel: one wave per ray, 64 samples per step; pass 1 sums w tau over the ray,
// pass 2 computes the terms and the gradient.  Everything from the fp32 inputs on is double (z +- eps, the clipping
// and the comparisons are exact there, Phi through erf) and each output is rounded to fp32 once.  No atomics, no LDS:
// bitwise reproducible.  A ray without a target (z or eps not finite or <= 0) or with c exactly 0 gets zeros, and its
// t values are not read.
// DENSE: s_i = tau_i = t_i, e_i = t_i + d_i with volume_render's dists (distortion_interval<true>'s d).  Packed:
// s = t0, e = t1, tau = (t0 + t1) / 2 of samples starts[r] .. + counts[r], cut at M.
struct DepthLossArgs {
    DistortionArgs d;                // w, t0, t1, starts, counts, M, N, S, ray_scale, loss, grad_w
    const float *depth, *eps;        // (N)
    double depth_weight, sight_weight;
};

__device__ __forceinline__ double normal_cdf(double x) { return 0.5 * (1.0 + erf(x * 0.70710678118654752440)); }

// start, end and depth of sample k (< n) of the ray whose first sample is b
template <bool DENSE>
__device__ __forceinline__ void depth_sample(const DistortionArgs& a, int64_t b, int64_t k, int64_t n, double& s,
                                             double& e, double& tau) {
    if (DENSE) {
        double m, d;
        distortion_interval<true>(a, b, k, n, m, d);
        s = (double)a.t0[b + k];
        e = s + d;
        tau = s;
    } else {
        s = (double)a.t0[b + k];
        e = (double)a.t1[b + k];
        tau = 0.5 * (s + e);
    }
}

template <bool DENSE>
__global__ void __launch_bounds__(256) depth_loss_kernel(DepthLossArgs p) {
    const DistortionArgs& a = p.d;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < a.N; r += nw) {
        int64_t b, n;
        if (DENSE) {
            b = r * a.S;
            n = a.S;
        } else {
            b = a.starts[r];
            n = a.counts[r];
            if (b < 0 || b > a.M || n < 0) n = 0;   // a range outside the samples is empty, one past M is cut
            if (n > a.M - b) n = a.M - b;
        }
        const double c = a.ray_scale ? (double)a.ray_scale[r] : 1.0;
        const float zf = p.depth[r], ef = p.eps[r];
        // wave-uniform: zeros, and the ray's t values (NaN for an invalid ray) are not read
        if (!(isfinite(zf) && zf > 0.0f && isfinite(ef) && ef > 0.0f) || c == 0.0) {
            if (a.grad_w)
                for (int64_t k = lane; k < n; k += 64) a.grad_w[b + k] = 0.0f;
            if (lane == 0) a.loss[r] = 0.0f;
            continue;
        }
        const double z = (double)zf, eps = (double)ef;
        const double lo = z - eps, hi = z + eps, sigma = eps / 3.0;
        double wtau = 0.0;   // this lane's share of D
        for (int64_t k = lane; k < n; k += 64) {
            double s, e, tau;
            depth_sample<DENSE>(a, b, k, n, s, e, tau);
            wtau += (double)a.w[b + k] * tau;
        }
        const double diff = acn::wave_sum_d(wtau) - z;   // D - z
        const double gd = 2.0 * p.depth_weight * c * c * diff;
        double acc = 0.0;   // this lane's share of the sight term
        for (int64_t k = lane; k < n; k += 64) {
            double s, e, tau;
            depth_sample<DENSE>(a, b, k, n, s, e, tau);
            const double w = (double)a.w[b + k];
            const double x0 = s > lo ? s : lo, x1 = e < hi ? e : hi;   // the interval clipped to the window
            double kk = 0.0;
            if (x1 > x0) kk = normal_cdf((x1 - z) / sigma) - normal_cdf((x0 - z) / sigma);
            const double u = s < hi ? w - kk : 0.0;
            acc += u * u;
            if (a.grad_w) a.grad_w[b + k] = (float)(gd * tau + 2.0 * p.sight_weight * u);
        }
        acc = acn::wave_sum_d(acc);
        const double cd = c * diff;
        if (lane == 0) a.loss[r] = (float)(p.depth_weight * (cd * cd) + p.sight_weight * acc);
    }
}

template <bool DENSE>
int launch_depth_loss(const DepthLossArgs& p, void* stream, const char* what) {
    const int64_t wgs = (p.d.N + 3) / 4;   // 4 waves (rays) per 256-thread workgroup, grid-stride past 4096 of them
    hipLaunchKernelGGL(depth_loss_kernel<DENSE>, dim3((unsigned)(wgs < 4096 ? wgs : 4096)), dim3(256), 0,
                       (hipStream_t)stream, p);
    return acn_check_launch(what);
}

}  // namespace

extern "C" int acn_depth_loss_packed(const float* weights, const float* t_starts, const float* t_ends, int64_t M,
                                     const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t N,
                                     const float* depth, const float* eps, const float* ray_scale, double depth_weight,
                                     double sight_weight, float* loss, float* grad_w, void* stream) {
    ACN_REQUIRE(N >= 0 && M >= 0, "acn_depth_loss_packed: N and M must be >= 0 (got %lld, %lld)", (long long)N,
                (long long)M);
    ACN_REQUIRE(depth_weight >= 0.0 && sight_weight >= 0.0,
                "acn_depth_loss_packed: depth_weight and sight_weight must be >= 0 (got %g, %g)", depth_weight,
                sight_weight);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(chunk_starts && chunk_cnts && depth && eps && loss, "acn_depth_loss_packed: NULL pointer");
    ACN_REQUIRE(M == 0 || (weights && t_starts && t_ends), "acn_depth_loss_packed: NULL sample array");
    DepthLossArgs p{{weights, t_starts, t_ends, chunk_starts, chunk_cnts, M, N, 0, ray_scale, loss, grad_w},
                    depth, eps, depth_weight, sight_weight};
    return launch_depth_loss<false>(p, stream, "acn_depth_loss_packed");
}

extern "C" int acn_depth_loss_dense(const float* weights, const float* t_vals, int64_t N, int S, const float* depth,
                                    const float* eps, const float* ray_scale, double depth_weight, double sight_weight,
                                    float* loss, float* grad_w, void* stream) {
    ACN_REQUIRE(N >= 0 && S >= 2, "acn_depth_loss_dense: N must be >= 0 and S >= 2 (got %lld, %d)", (long long)N, S);
    ACN_REQUIRE(depth_weight >= 0.0 && sight_weight >= 0.0,
                "acn_depth_loss_dense: depth_weight and sight_weight must be >= 0 (got %g, %g)", depth_weight,
                sight_weight);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(weights && t_vals && depth && eps && loss, "acn_depth_loss_dense: NULL pointer");
    DepthLossArgs p{{weights, t_vals, nullptr, nullptr, nullptr, N * (int64_t)S, N, S, ray_scale, loss, grad_w},
                    depth, eps, depth_weight, sight_weight};
    return launch_depth_loss<true>(p, stream, "acn_depth_loss_dense");
}

extern "C" int acn_distortion_packed(const float* weights, const float* t_starts, const float* t_ends, int64_t M,
                                     const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t N,
                                     const float* ray_scale, float* loss, float* grad_w, void* stream) {
    ACN_REQUIRE(N >= 0 && M >= 0, "acn_distortion_packed: N and M must be >= 0 (got %lld, %lld)", (long long)N,
                (long long)M);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(chunk_starts && chunk_cnts && loss, "acn_distortion_packed: NULL pointer");
    ACN_REQUIRE(M == 0 || (weights && t_starts && t_ends), "acn_distortion_packed: NULL sample array");
    DistortionArgs a{weights, t_starts, t_ends, chunk_starts, chunk_cnts, M, N, 0, ray_scale, loss, grad_w};
    return launch_distortion<false>(a, stream, "acn_distortion_packed");
}

extern "C" int acn_distortion_dense(const float* weights, const float* t_vals, int64_t N, int S,
                                    const float* ray_scale, float* loss, float* grad_w, void* stream) {
    ACN_REQUIRE(N >= 0 && S >= 2, "acn_distortion_dense: N must be >= 0 and S >= 2 (got %lld, %d)", (long long)N, S);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(weights && t_vals && loss, "acn_distortion_dense: NULL pointer");
    DistortionArgs a{weights, t_vals, nullptr, nullptr, nullptr, N * (int64_t)S, N, S, ray_scale, loss, grad_w};
    return launch_distortion<true>(a, stream, "acn_distortion_dense");
}

extern "C" int acn_mse_linear_fwd(const float* pred, const float* gt, int64_t n, float* loss, void* stream) {
    ACN_REQUIRE(n >= 1 && pred && gt && loss, "acn_mse_linear_fwd: bad arguments");
    hipLaunchKernelGGL(mse_linear_fwd_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, pred, gt, n, loss);
    return acn_check_launch("acn_mse_linear_fwd");
}

extern "C" size_t acn_mse_linear_workspace_bytes(void) { return kWsMaxBlocks * sizeof(double) + 16; }

extern "C" int acn_mse_linear_fwd_ws(const float* pred, const float* gt, int64_t n, float* loss, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    ACN_REQUIRE(n >= 1 && pred && gt && loss && workspace, "acn_mse_linear_fwd_ws: bad arguments");
    ACN_REQUIRE(workspace_bytes >= acn_mse_linear_workspace_bytes(), "acn_mse_linear_fwd_ws: workspace too small");
    int64_t g = (n + kWsThreads * kWsPerThread - 1) / (kWsThreads * kWsPerThread);
    g = g < 1 ? 1 : (g > kWsMaxBlocks ? kWsMaxBlocks : g);
    double* partials = (double*)workspace;
    unsigned int* counter = (unsigned int*)((char*)workspace + kWsMaxBlocks * sizeof(double));
    hipLaunchKernelGGL(mse_linear_fwd_ws_kernel, dim3((unsigned)g), dim3(kWsThreads), 0, (hipStream_t)stream, pred, gt,
                       n, partials, counter, loss);
    return acn_check_launch("acn_mse_linear_fwd_ws");
}

extern "C" int acn_mse_linear_bwd(const float* pred, const float* gt, int64_t n, const float* g_loss, float* g_pred,
                                  void* stream) {
    ACN_REQUIRE(n >= 1 && pred && gt && g_loss && g_pred, "acn_mse_linear_bwd: bad arguments");
    hipLaunchKernelGGL(mse_linear_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       pred, gt, n, g_loss, g_pred);
    return acn_check_launch("acn_mse_linear_bwd");
}

extern "C" int acn_normal_composite(const float* grad, const float* weights, int64_t N, int S, float* normal,
                                    void* stream) {
    ACN_REQUIRE(N >= 0 && S >= 1, "acn_normal_composite: N must be >= 0 and S >= 1 (got %lld, %d)", (long long)N, S);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(grad && weights && normal, "acn_normal_composite: NULL pointer");
    hipLaunchKernelGGL(normal_composite_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       grad, weights, N, S, normal);
    return acn_check_launch("acn_normal_composite");
}
