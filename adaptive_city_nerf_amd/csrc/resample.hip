// resample.hip -- hierarchical importance resampling (classic NeRF sample_pdf, coarse to fine) on gfx950:
// acn_resample_pdf, DESIGN.md 4u.  The torch form is a chain of cumsum, searchsorted, four gathers, cat and a full
// sort of rows that are two sorted lists already (~15 launches); here it is one launch.
//
// Per ray, in float64 on the fp32 inputs (t non-decreasing, w >= 0):
//   edges       b_i = (t_i + t_{i+1}) / 2                      i = 0 .. S-2
//   bin masses  p_i = w_{i+1} + 1e-5                           i = 0 .. S-3   (weights[1:-1] + 1e-5)
//   CDF         c_0 = 0, c_k = p_0 + .. + p_{k-1}, C = c_{S-2}                (not normalised: no division by C)
//   quantiles   v_j = (j + r_j) / F * C, r_j the jitter or 0.5 (stratified: ascending, no sort of u)
//   k the largest index in [0, S-3] with c_k <= v_j, f = clamp((v_j - c_k) / (c_{k+1} - c_k), 0, 1) (0 when the
//   denominator is not positive), t_fine_j = fp32(b_k + f (b_{k+1} - b_k))
// and the stable merge of t with t_fine (a coarse sample before an equal fine one) by rank arithmetic: coarse i goes to
// i + #{fine < t_i}, fine j to j + #{coarse <= x_j}.
//
// One wave per ray, 4 rays per workgroup.  A wave's LDS: its t (S floats), its fine samples (F floats) and one region
// that first holds the CDF (S-1 doubles) and then, the CDF being dead, the merged row (S+F floats): at most 16 KB per
// wave, sized per launch from S and F.  The CDF is a wave scan over 64 bins per step with a carry (the distortion
// loss's scan, loss.hip).  Every binary search runs a fixed number of steps over indices that stay inside the wave's
// own arrays whatever the values compare to, so a NaN row ends like any other and writes its own row only.  The
// merged row and the points leave LDS as contiguous stores.  No atomics, no scratch: bitwise reproducible.
#include "acn_device.h"
#include "acn_internal.h"

namespace {

constexpr int kMaxS = 1024, kMaxF = 1024;
constexpr int kWaves = 4;   // rays per workgroup

struct ResampleArgs {
    const float *w, *t;      // (N, S)
    const float* jitter;     // (N, F) or NULL (0.5)
    const float* rays;       // (N, 8) or NULL
    float *t_fine;           // (N, F) or NULL
    float *t_merged;         // (N, S + F)
    float *pts6;             // (N * (S + F), 6) or NULL
    int64_t N;
    int32_t S, F;
    int32_t steps_c, steps_f, steps_t;   // binary-search trip counts over S-2 CDF entries, F fine and S coarse samples
    int32_t wave_floats;     // LDS floats per wave
    int32_t u_off;           // float offset of the CDF / merged region in a wave's LDS (even: the doubles are aligned)
};

using acn::prefix_count;   // acn_device.h (shared with interlevel.hip)

__global__ void __launch_bounds__(kWaves * 64) resample_pdf_kernel(ResampleArgs a) {
    extern __shared__ double lds_raw[];   // double: 8-byte alignment of the base
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.S, F = a.F, SF = S + F;
    float* tl = (float*)lds_raw + (size_t)wave * a.wave_floats;   // t        [S]
    float* fl = tl + S;                                           // t_fine   [F]
    double* cd = (double*)(tl + a.u_off);                         // CDF      [S-1], then
    float* ml = tl + a.u_off;                                     // t_merged [S+F]
    const int nb = S - 2;                                         // bins
    // every wave of the workgroup makes the same number of trips (the barriers below are workgroup barriers)
    for (int64_t base = (int64_t)blockIdx.x * kWaves; base < a.N; base += (int64_t)gridDim.x * kWaves) {
        const int64_t r = base + wave;
        const bool live = r < a.N;
        if (live) {
            const float* t = a.t + r * S;
            const float* w = a.w + r * S;
            for (int i = lane; i < S; i += 64) tl[i] = t[i];
            double carry = 0.0;
            if (lane == 0) cd[0] = 0.0;
            for (int i0 = 0; i0 < nb; i0 += 64) {
                const int i = i0 + lane;
                const double p = i < nb ? (double)w[i + 1] + 1e-5 : 0.0;
                const double inc = acn::wave_incl_scan(p, lane);
                if (i < nb) cd[i + 1] = carry + inc;
                carry += __shfl(inc, 63);
            }
        }
        __syncthreads();
        if (live) {
            const double C = cd[nb];
            const float* jit = a.jitter ? a.jitter + r * F : nullptr;
            float* tf = a.t_fine ? a.t_fine + r * F : nullptr;
            for (int j = lane; j < F; j += 64) {
                const double rj = jit ? (double)jit[j] : 0.5;
                const double v = (((double)j + rj) / (double)F) * C;
                int k = prefix_count(cd, nb, a.steps_c, [v](double c) { return c <= v; }) - 1;
                k = k < 0 ? 0 : k;   // c_0 = 0 <= v; a NaN v counts nothing
                const double c0 = cd[k], c1 = cd[k + 1];
                const double den = c1 - c0;
                double f = den > 0.0 ? (v - c0) / den : 0.0;
                f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
                const double t0 = (double)tl[k], t1 = (double)tl[k + 1], t2 = (double)tl[k + 2];
                const double b0 = (t0 + t1) * 0.5, b1 = (t1 + t2) * 0.5;
                const float x = (float)(b0 + f * (b1 - b0));
                fl[j] = x;
                if (tf) tf[j] = x;
            }
        }
        __syncthreads();   // the CDF is dead from here: its region takes the merged row
        if (live) {
            for (int i = lane; i < S; i += 64) {
                const float x = tl[i];
                ml[i + prefix_count(fl, F, a.steps_f, [x](float y) { return y < x; })] = x;
            }
            for (int j = lane; j < F; j += 64) {
                const float x = fl[j];
                ml[j + prefix_count(tl, S, a.steps_t, [x](float y) { return y <= x; })] = x;
            }
        }
        __syncthreads();
        if (live) {
            float* tm = a.t_merged + r * SF;
            for (int m = lane; m < SF; m += 64) tm[m] = ml[m];
            if (a.pts6) {
                const float* ray = a.rays + r * 8;
                const float ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];
                // a row is [o + d t, d], 24 bytes: three 8-byte stores, consecutive lanes on consecutive addresses
                float2* p = (float2*)(a.pts6 + r * SF * 6);
                for (int e = lane; e < SF * 3; e += 64) {
                    const int m = e / 3, part = e - 3 * m;
                    const float tv = ml[m];
                    float2 v;
                    if (part == 0) {
                        v = make_float2(ox + dx * tv, oy + dy * tv);
                    } else if (part == 1) {
                        v = make_float2(oz + dz * tv, dx);
                    } else {
                        v = make_float2(dy, dz);
                    }
                    p[e] = v;
                }
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

extern "C" int acn_resample_pdf(const float* weights, const float* t_vals, int64_t N, int S, const float* jitter, int F,
                                const float* rays, float* t_fine, float* t_merged, float* pts6, void* stream) {
    ACN_REQUIRE(N >= 0, "acn_resample_pdf: N must be >= 0 (got %lld)", (long long)N);
    if (S < 3 || S > kMaxS || F < 1 || F > kMaxF)
        return acn_set_error(ACN_ERR_UNSUPPORTED,
                             "acn_resample_pdf: needs 3 <= S <= %d coarse and 1 <= F <= %d fine samples (got %d, %d)",
                             kMaxS, kMaxF, S, F);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(weights && t_vals && t_merged, "acn_resample_pdf: NULL pointer");
    ACN_REQUIRE(!pts6 || rays, "acn_resample_pdf: the points need the rays");
    ResampleArgs a{weights, t_vals, jitter, rays, t_fine, t_merged, pts6, N, S, F,
                   search_steps(S - 2), search_steps(F), search_steps(S), 0, 0};
    a.u_off = (S + F + 1) & ~1;
    const int u_floats = 2 * (S - 1) > S + F ? 2 * (S - 1) : S + F;
    a.wave_floats = (a.u_off + u_floats + 1) & ~1;
    const size_t lds = (size_t)kWaves * a.wave_floats * sizeof(float);   // <= 4 * (2048 + 2048) * 4 = 64 KB
    const int64_t wgs = (N + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(resample_pdf_kernel, dim3((unsigned)(wgs < 8192 ? wgs : 8192)), dim3(kWaves * 64), lds,
                       (hipStream_t)stream, a);
    return acn_check_launch("acn_resample_pdf");
}
