// appearance.hip -- per-image exposure correction on gfx950: the affine colour transform of Urban
// Radiance Fields / Zip-NeRF on the composited pixel, c = A[s] p + b[s] for the ray's image slot s, fused with the
// training loss of loss.hip (clamp01(c) against gt_linear(gt), mean of squares) and with all of its gradients.
//   c[k]        = fl32(A[s,k,0] p0 + A[s,k,1] p1 + A[s,k,2] p2 + b[s,k])     in double, left to right, rounded once
//   d[k]        = clamp01(c[k]) - gt_linear(gt[k])                           fp32, loss.hip's helpers (NaN passes)
//   loss        = fl32(sum d^2 / n), n = 3 N                                 double, fixed order
//   g_c[k]      = fl32((2 / n) d[k]) where 0 <= c[k] <= 1, else 0            mse_linear_bwd_kernel's at g_loss = 1
//   g_pred[r,j] = fl32(sum_k A[s,k,j] g_c[k])                                double
//   g_A[i,k,j]  = fl32(sum_{r: slot = i} g_c[r,k] p[r,j]),  g_b[i,k] = fl32(sum_{r: slot = i} g_c[r,k])   double
// A slot outside [0, I) is the identity (c = p bit for bit, g_pred = g_c) and reaches no parameter.
// One launch.  Workgroups [0, G) own rays, in the layout of mse_linear_fwd_ws_kernel (thread i of workgroup b takes
// rays b*256 + i, + G*256, ...; double partials; a ticket; a fixed final tree): they write g_pred and the loss.
// Workgroups [G, G + I) own one slot each: the workgroup scans the int32 slot column in a fixed per-thread order (the
// column is read I times, coalesced, from L2), recomputes g_c for its own rays, carries 12 double accumulators per
// thread and reduces them with a fixed xor tree per wave and the waves in order.  No sort, no atomics on the outputs,
// every output element written (a slot no ray reached gets zeros): bitwise reproducible, and capturable.
#include "acn_device.h"
#include "acn_internal.h"

namespace {

using acn::clamp01;
using acn::gt_linear;

constexpr int kThreads = 256;
constexpr int kMaxRayBlocks = 256;   // past 65536 rays a thread takes more than one

struct AppearanceArgs {
    const float *pred, *gt;    // (N, 3)
    const int32_t* slot;       // (N)
    int64_t N;
    const float *A, *b;        // (I, 3, 3), (I, 3)
    int I;
    unsigned int G;            // ray workgroups
    float *loss, *g_pred, *g_A, *g_b;   // the three gradients NULL together
    double* partials;          // (kMaxRayBlocks)
    unsigned int* counter;
};

// c of one ray: m = {A (row major), b} of its slot, or the identity when has is false
__device__ __forceinline__ void corrected(const float (&m)[12], bool has, const float (&p)[3], float (&c)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = (double)m[3 * k] * (double)p[0] + (double)m[3 * k + 1] * (double)p[1] +
                         (double)m[3 * k + 2] * (double)p[2] + (double)m[9 + k];
        c[k] = has ? (float)v : p[k];
    }
}

__device__ __forceinline__ void load_slot(const AppearanceArgs& a, int s, float (&m)[12]) {
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] = a.A[(int64_t)s * 9 + q];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[9 + k] = a.b[(int64_t)s * 3 + k];
}

// d loss / d c of one channel at g_loss = 1 (mse_linear_bwd_kernel's expression)
__device__ __forceinline__ float grad_c(float c, float d, double two_over_n) {
    const float g = (float)(two_over_n * (double)d);
    return (c >= 0.0f && c <= 1.0f) ? g : 0.0f;
}

__device__ void ray_workgroup(const AppearanceArgs& a) {
    __shared__ double red[kThreads / 64];
    __shared__ bool last;
    const double two_over_n = 2.0 / (double)(3 * a.N);
    double acc = 0.0;
    const int64_t stride = (int64_t)a.G * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < a.N; r += stride) {
        const int s = a.slot[r];
        const bool has = s >= 0 && s < a.I;
        float p[3], q[3], m[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, c[3], gc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = a.pred[3 * r + k];
            q[k] = a.gt[3 * r + k];
        }
        if (has) load_slot(a, s, m);
        corrected(m, has, p, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d = clamp01(c[k]) - gt_linear(q[k]);
            acc += (double)d * (double)d;
            gc[k] = grad_c(c[k], d, two_over_n);
        }
        if (a.g_pred) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double v = (double)m[j] * (double)gc[0] + (double)m[3 + j] * (double)gc[1] +
                                 (double)m[6 + j] * (double)gc[2];
                a.g_pred[3 * r + j] = has ? (float)v : gc[j];
            }
        }
    }
    acc = acn::wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) t += red[i];
        a.partials[blockIdx.x] = t;
        __threadfence();
        last = atomicAdd(a.counter, 1u) == a.G - 1;
    }
    __syncthreads();
    // last ray workgroup: thread i loads partial i (G <= 256), a fixed xor tree per wave and the waves in order
    if (last) {
        __threadfence();
        double v = threadIdx.x < a.G
                       ? __hip_atomic_load(&a.partials[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       : 0.0;
        v = acn::wave_sum_d(v);
        __syncthreads();   // red[] is reused (thread 0 read it above)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int i = 0; i < kThreads / 64; ++i) t += red[i];
            a.loss[0] = (float)(t / (double)(3 * a.N));
            a.counter[0] = 0u;
        }
    }
}

__device__ void slot_workgroup(const AppearanceArgs& a, int i) {
    __shared__ double red[kThreads / 64][12];
    const double two_over_n = 2.0 / (double)(3 * a.N);
    float m[12];
    load_slot(a, i, m);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    // 4 slot loads in flight per thread; the rays are visited in the same per-thread order either way
    for (int64_t r0 = threadIdx.x; r0 < a.N; r0 += 4 * kThreads) {
        int s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = r0 + (int64_t)u * kThreads;
            s[u] = r < a.N ? a.slot[r] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (s[u] != i) continue;
            const int64_t r = r0 + (int64_t)u * kThreads;
            float p[3], c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = a.pred[3 * r + k];
            corrected(m, true, p, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = clamp01(c[k]) - gt_linear(a.gt[3 * r + k]);
                const double g = (double)grad_c(c[k], d, two_over_n);
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 * k + j] += g * (double)p[j];
                acc[9 + k] += g;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const double v = acn::wave_sum_d(acc[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += red[w][threadIdx.x];
        if (threadIdx.x < 9) a.g_A[(int64_t)i * 9 + threadIdx.x] = (float)t;
        else a.g_b[(int64_t)i * 3 + (threadIdx.x - 9)] = (float)t;
    }
}

__global__ void __launch_bounds__(kThreads) appearance_mse_kernel(AppearanceArgs a) {
    if (blockIdx.x < a.G) ray_workgroup(a);
    else slot_workgroup(a, (int)(blockIdx.x - a.G));
}

__global__ void __launch_bounds__(kThreads) appearance_apply_kernel(const float* __restrict__ rgb,
                                                                    const int32_t* __restrict__ slot, int64_t N,
                                                                    const float* __restrict__ A,
                                                                    const float* __restrict__ b, int I,
                                                                    float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const int s = slot[r];
    const bool has = s >= 0 && s < I;
    float p[3], c[3], m[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = rgb[3 * r + k];
    if (has) {
#pragma unroll
        for (int q = 0; q < 9; ++q) m[q] = A[(int64_t)s * 9 + q];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[9 + k] = b[(int64_t)s * 3 + k];
    }
    corrected(m, has, p, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * r + k] = c[k];
}

}  // namespace

extern "C" size_t acn_appearance_mse_workspace_bytes(int I) {
    (void)I;   // the slot workgroups need none: the loss partials and the ticket
    return kMaxRayBlocks * sizeof(double) + 16;
}

extern "C" int acn_appearance_mse(const float* pred, const float* gt, const int32_t* slot, int64_t N, const float* A,
                                  const float* b, int I, float* loss, float* g_pred, float* g_A, float* g_b,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    ACN_REQUIRE(N >= 1 && I >= 1, "acn_appearance_mse: N and I must be >= 1 (got %lld, %d)", (long long)N, I);
    ACN_REQUIRE(N <= (int64_t)1 << 40, "acn_appearance_mse: N too large (%lld)", (long long)N);
    ACN_REQUIRE(pred && gt && slot && A && b && loss && workspace, "acn_appearance_mse: NULL pointer");
    ACN_REQUIRE((g_pred && g_A && g_b) || (!g_pred && !g_A && !g_b),
                "acn_appearance_mse: g_pred, g_A and g_b must be given or NULL together");
    ACN_REQUIRE(workspace_bytes >= acn_appearance_mse_workspace_bytes(I), "acn_appearance_mse: workspace too small");
    int64_t g = (N + kThreads - 1) / kThreads;
    g = g > kMaxRayBlocks ? kMaxRayBlocks : g;
    AppearanceArgs a{pred, gt, slot, N, A, b, I, (unsigned)g, loss, g_pred, g_A, g_b, (double*)workspace,
                     (unsigned int*)((char*)workspace + kMaxRayBlocks * sizeof(double))};
    const unsigned blocks = (unsigned)g + (g_pred ? (unsigned)I : 0u);
    hipLaunchKernelGGL(appearance_mse_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return acn_check_launch("acn_appearance_mse");
}

extern "C" int acn_appearance_apply(const float* rgb, const int32_t* slot, int64_t N, const float* A, const float* b,
                                    int I, float* out, void* stream) {
    ACN_REQUIRE(N >= 0 && I >= 1, "acn_appearance_apply: N must be >= 0 and I >= 1 (got %lld, %d)", (long long)N, I);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(N <= (int64_t)1 << 38, "acn_appearance_apply: N too large (%lld)", (long long)N);
    ACN_REQUIRE(rgb && slot && A && b && out, "acn_appearance_apply: NULL pointer");
    hipLaunchKernelGGL(appearance_apply_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, rgb, slot, N, A, b, I, out);
    return acn_check_launch("acn_appearance_apply");
}
