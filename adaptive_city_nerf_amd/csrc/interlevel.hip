// interlevel.hip -- the interlevel ("proposal") loss of the mip-NeRF 360 recipe on gfx950: acn_interlevel_loss,
// DESIGN.md 4aa.  The proposal's weight histogram along a ray must upper-bound the main model's; only the proposal's
// weights get a gradient.  The torch form is a chain of cumsum, two searchsorted, gathers and a scatter; here it is one
// launch.
//
// Per ray, in float64 on the fp32 inputs (depths non-decreasing, weights >= 0):
//   edges       E(t)_i = t_i (i < S), E(t)_S = t_{S-1} + (t_{S-1} - t_{S-2});  a = E(t_fine), p = E(t_prop)
//   overlap     O(i,k) = (p_{k+1} > a_i) and (p_k < a_{i+1}): sorted edges make {k : O(i,k)} the range [lo_i, hi_i)
//               lo_i = max(#{j <= P : p_j <= a_i} - 1, 0), hi_i = max(min(#{j <= P : p_j < a_{i+1}}, P), lo_i)
//   bound_i     = c[hi_i] - c[lo_i], c the exclusive prefix sum of w_prop (the one term itself when hi_i = lo_i + 1)
//   x_i         = max(0, w_i - bound_i),  loss = sum_i x_i^2 / (w_i + eps),  r_i = 2 x_i / (w_i + eps)
//   d loss / d w_prop_k = -(R[max(n_lo, n_hi)] - R[n_hi]), R the exclusive prefix sum of r,
//               n_lo = #{i < S : a_i < p_{k+1}}, n_hi = #{i < S : a_{i+1} <= p_k}
// A tie is the tight bound: a fine interval that ends exactly on a proposal edge does not count the next proposal
// interval.
//
// One wave per ray, up to 4 rays per workgroup (fewer at long rows: 64 KB of LDS per workgroup).  A wave's LDS: c
// (P+1 doubles), R (S+1 doubles), the proposal depths (P floats) and the fine depths (S floats); the last edge of a
// row is recomputed in float64 from its last two depths.  Both scans are the distortion loss's wave scan with a
// float64 carry.  Every binary search runs a fixed number of steps over indices that stay inside the wave's own arrays
// whatever the values compare to, so a NaN or unsorted row ends like any other and writes its own row only.  No
// atomics, no scratch: bitwise reproducible.
#include "acn_device.h"
#include "acn_internal.h"

namespace {

constexpr int kMaxS = 1024, kMaxP = 1024;
constexpr int kMaxWaves = 4;            // rays per workgroup at short rows
constexpr size_t kLdsBytes = 65536;     // dynamic LDS a launch gets without raising the limit

struct InterlevelArgs {
    const float *t_fine, *w_fine;   // (N, S)
    const float *t_prop, *w_prop;   // (N, P)
    const float* ray_scale;         // (N) or NULL
    float* loss;                    // (N)
    float* grad;                    // (N, P) or NULL
    double eps;
    int64_t N;
    int32_t S, P;
    int32_t steps_s, steps_p;       // binary-search trip counts over S fine and P proposal depths
    int32_t wave_bytes;             // LDS bytes per wave (a multiple of 8)
};

// #{j <= n : pred(e_j)} over the n + 1 ascending edges e_0 .. e_{n-1} = row[], e_n = last (pred true on a prefix):
// in [0, n + 1]; row[] is read at indices < n only
template <typename Pred>
__device__ __forceinline__ int edge_count(const float* row, int n, double last, int steps, Pred pred) {
    const int c = acn::prefix_count(row, n, steps, [pred](float v) { return pred((double)v); });
    return c + ((c == n && pred(last)) ? 1 : 0);
}

__global__ void __launch_bounds__(kMaxWaves * 64) interlevel_loss_kernel(InterlevelArgs a) {
    extern __shared__ double lds_raw[];   // double: 8-byte alignment of the base
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int S = a.S, P = a.P;
    double* cl = (double*)((char*)lds_raw + (size_t)wave * a.wave_bytes);   // c       [P+1]
    double* rl = cl + (P + 1);                                              // R       [S+1]
    float* pl = (float*)(rl + (S + 1));                                     // t_prop  [P]
    float* al = pl + P;                                                     // t_fine  [S]
    // every wave of the workgroup makes the same number of trips (the barriers below are workgroup barriers)
    for (int64_t base = (int64_t)blockIdx.x * waves; base < a.N; base += (int64_t)gridDim.x * waves) {
        const int64_t r = base + wave;
        const bool in = r < a.N;
        const double scale = in && a.ray_scale ? (double)a.ray_scale[r] : 1.0;
        const bool live = in && scale != 0.0;   // wave-uniform
        const float* wp = a.w_prop + (in ? r : 0) * P;
        if (in && !live) {   // zeros, and the ray's depths (NaN for an invalid ray) are not read
            if (a.grad)
                for (int k = lane; k < P; k += 64) a.grad[r * P + k] = 0.0f;
            if (lane == 0) a.loss[r] = 0.0f;
        }
        if (live) {
            const float* tf = a.t_fine + r * S;
            const float* tp = a.t_prop + r * P;
            for (int i = lane; i < S; i += 64) al[i] = tf[i];
            for (int k = lane; k < P; k += 64) pl[k] = tp[k];
            double carry = 0.0;
            if (lane == 0) cl[0] = 0.0;
            for (int k0 = 0; k0 < P; k0 += 64) {
                const int k = k0 + lane;
                const double v = k < P ? (double)wp[k] : 0.0;
                const double inc = acn::wave_incl_scan(v, lane);
                if (k < P) cl[k + 1] = carry + inc;
                carry += __shfl(inc, 63);
            }
        }
        __syncthreads();
        double a_last = 0.0, p_last = 0.0;
        if (live) {
            a_last = (double)al[S - 1] + ((double)al[S - 1] - (double)al[S - 2]);
            p_last = (double)pl[P - 1] + ((double)pl[P - 1] - (double)pl[P - 2]);
            const float* wf = a.w_fine + r * S;
            double carry = 0.0, acc = 0.0;
            if (lane == 0) rl[0] = 0.0;
            for (int i0 = 0; i0 < S; i0 += 64) {
                const int i = i0 + lane;
                double ri = 0.0;
                if (i < S) {
                    const double a0 = (double)al[i];
                    const double a1 = i + 1 < S ? (double)al[i + 1] : a_last;
                    int lo = edge_count(pl, P, p_last, a.steps_p, [a0](double p) { return p <= a0; }) - 1;
                    lo = lo < 0 ? 0 : lo;                                   // [0, P]
                    int hi = edge_count(pl, P, p_last, a.steps_p, [a1](double p) { return p < a1; });
                    hi = hi > P ? P : hi;
                    hi = hi < lo ? lo : hi;                                 // [lo, P]
                    // one overlapped interval: its weight itself (lo = hi - 1 < P), so that equal histograms give 0
                    const double bound = hi == lo + 1 ? (double)wp[lo] : cl[hi] - cl[lo];
                    const double w = (double)wf[i];
                    double x = w - bound;
                    x = x > 0.0 ? x : 0.0;
                    const double den = w + a.eps;
                    acc += x * x / den;
                    ri = 2.0 * x / den;
                }
                const double inc = acn::wave_incl_scan(ri, lane);
                if (i < S) rl[i + 1] = carry + inc;
                carry += __shfl(inc, 63);
            }
            acc = acn::wave_sum_d(acc);
            if (lane == 0) a.loss[r] = (float)(scale * acc);
        }
        __syncthreads();
        if (live && a.grad) {
            float* g = a.grad + r * P;
            for (int k = lane; k < P; k += 64) {
                const double p0 = (double)pl[k];
                const double p1 = k + 1 < P ? (double)pl[k + 1] : p_last;
                // fine intervals i with a_i < p_{k+1} are [0, n_lo), those with a_{i+1} > p_k are [n_hi, S)
                const int n_lo = acn::prefix_count(al, S, a.steps_s, [p1](float v) { return (double)v < p1; });
                const int n_hi = edge_count(al + 1, S - 1, a_last, a.steps_s, [p0](double v) { return v <= p0; });
                const int top = n_lo > n_hi ? n_lo : n_hi;                  // both in [0, S]
                g[k] = (float)(scale * (rl[n_hi] - rl[top]));
            }
        }
        __syncthreads();   // the next trip overwrites the wave's LDS
    }
}

int search_steps(int n) {   // floor(log2 n) + 1 for n >= 1
    int s = 0;
    while (n > 0) {
        ++s;
        n >>= 1;
    }
    return s < 1 ? 1 : s;
}

}  // namespace

extern "C" int acn_interlevel_loss(const float* t_fine, const float* w_fine, int S, const float* t_prop,
                                   const float* w_prop, int P, int64_t N, const float* ray_scale, double eps,
                                   float* loss, float* grad_w_prop, void* stream) {
    ACN_REQUIRE(N >= 0, "acn_interlevel_loss: N must be >= 0 (got %lld)", (long long)N);
    if (S < 2 || S > kMaxS || P < 2 || P > kMaxP)
        return acn_set_error(ACN_ERR_UNSUPPORTED,
                             "acn_interlevel_loss: needs 2 <= S <= %d fine and 2 <= P <= %d proposal samples (got %d, "
                             "%d)", kMaxS, kMaxP, S, P);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(t_fine && w_fine && t_prop && w_prop && loss, "acn_interlevel_loss: NULL pointer");
    InterlevelArgs a{t_fine, w_fine, t_prop, w_prop, ray_scale, loss, grad_w_prop, eps, N, S, P,
                     search_steps(S), search_steps(P), 0};
    a.wave_bytes = (int32_t)((8 * (size_t)(S + P + 2) + 4 * (size_t)(S + P) + 7) & ~(size_t)7);   // <= 24592
    int waves = (int)(kLdsBytes / (size_t)a.wave_bytes);   // >= 2
    waves = waves > kMaxWaves ? kMaxWaves : waves;
    const size_t lds = (size_t)waves * a.wave_bytes;       // <= 64 KB
    const int64_t wgs = (N + waves - 1) / waves;
    hipLaunchKernelGGL(interlevel_loss_kernel, dim3((unsigned)(wgs < 8192 ? wgs : 8192)), dim3(waves * 64), lds,
                       (hipStream_t)stream, a);
    return acn_check_launch("acn_interlevel_loss");
}
