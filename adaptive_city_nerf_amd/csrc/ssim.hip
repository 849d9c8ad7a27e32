// ssim.hip -- the structural similarity index of two images and its gradient on gfx950: the reference's
// second evaluation metric (runtime_adapt.py:152-167 calls pytorch_msssim.ssim) and, as 1 - ssim, a training loss.
// Per image n and channel c, with the normalised Gaussian window g (win taps, host float64, passed by value) and the
// separable "valid" correlation g* (no padding, maps of (H - win + 1) x (W - win + 1) pixels):
//   mu1 = g*X, mu2 = g*Y, s1 = g*X^2 - mu1^2, s2 = g*Y^2 - mu2^2, s12 = g*XY - mu1 mu2
//   cs = (2 s12 + C2) / (s1 + s2 + C2), map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs, ssim[n, c] = mean(map)
// s1, s2 and s12 are differences of nearly equal numbers on a low-contrast image, so everything after the fp32 loads
// is float64 and each output is rounded to fp32 once.  The three second moments are accumulated by one instruction
// sequence in one order (and the build has -ffp-contract=off), so ssim(X, X) is exactly 1.
// Forward: one 256-thread workgroup per 32 x 32 tile of one plane's map.  The (32 + win - 1)^2 halo of X and Y is staged
// in LDS as fp32, the horizontal pass writes the five moments of its rows to LDS as float64, the vertical pass gives each
// thread 4 vertically adjacent map pixels of one column.  The tile's sum goes to the workspace as one float64;
// ssim_mean_kernel adds a plane's tiles in a fixed order: no atomics, bitwise reproducible.
// Gradient: with A = d map / d mu1 (s11 = g*X^2 and s12' = g*XY held fixed), B = d map / d s11, Cm = d map / d s12',
//   d ssim[n, c] / d X[q] = 1 / Np * sum_p g2(p -> q) (A[p] + 2 X[q] B[p] + Y[q] Cm[p]).
// The forward launch writes A, B, Cm as float64 planes into the workspace; ssim_grad_kernel runs the transposed
// ("full") separable correlation of the three maps per 32 x 32 tile of X through the same two LDS passes.
#include "acn_device.h"
#include "acn_internal.h"

#include <math.h>

namespace {

constexpr int kTile = ACN_SSIM_TILE;   // map pixels (forward) / image pixels (gradient) per tile side
constexpr int kThreads = 256;
constexpr int kRows = kTile * kTile / kThreads;   // vertically adjacent outputs per thread
constexpr int kMaxWin = 11;
static_assert(kTile == 32 && kRows == 4, "the thread-to-pixel maps below assume 32 x 32 tiles of 256 threads");

struct SsimWindow {
    double g[kMaxWin];
};

struct SsimArgs {
    const float *x, *y;
    int64_t NC;
    int32_t C, H, W;
    int32_t Hm, Wm;          // map size
    int32_t tiles_x, tiles;  // tiles per row / per plane (of the map forward, of the image in the gradient)
    int32_t channels_last;
    double c1, c2;
    double* partials;        // (NC, tiles) tile sums of the map
    double* maps;            // 3 planes of (NC, Hm, Wm): A, B, Cm; NULL without gradient
    float* grad_x;
    SsimWindow win;
};

// offset of pixel (0, 0) of plane nc, and the strides of a pixel and of a row, in floats
__device__ __forceinline__ void plane_layout(const SsimArgs& a, int64_t nc, int64_t& base, int64_t& ps, int64_t& rs) {
    if (a.channels_last) {
        const int64_t n = nc / a.C, c = nc % a.C;
        base = n * a.H * a.W * a.C + c;
        ps = a.C;
    } else {
        base = nc * a.H * a.W;
        ps = 1;
    }
    rs = ps * a.W;
}

template <int WIN, bool GRAD>
__global__ void __launch_bounds__(kThreads) ssim_fwd_kernel(SsimArgs a) {
    constexpr int R = WIN - 1, HS = kTile + R;   // halo side
    __shared__ float xs[HS][HS];
    __shared__ float ys[HS][HS];
    __shared__ double hm[5][HS][kTile];   // horizontal pass: g*X, g*Y, g*X^2, g*Y^2, g*XY of every halo row
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t nc = blockIdx.x / a.tiles;
    const int tile = (int)(blockIdx.x % a.tiles);
    const int ty0 = (tile / a.tiles_x) * kTile, tx0 = (tile % a.tiles_x) * kTile;
    int64_t base, ps, rs;
    plane_layout(a, nc, base, ps, rs);

    for (int i = tid; i < HS * HS; i += kThreads) {
        const int r = i / HS, c = i % HS;
        const int yy = ty0 + r, xx = tx0 + c;
        const bool in = yy < a.H && xx < a.W;
        const int64_t o = base + yy * rs + xx * ps;
        xs[r][c] = in ? a.x[o] : 0.0f;
        ys[r][c] = in ? a.y[o] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < HS * kTile; i += kThreads) {
        const int r = i / kTile, c = i % kTile;
        double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double g = a.win.g[k];
            const double xv = (double)xs[r][c + k], yv = (double)ys[r][c + k];
            m1 += g * xv;
            m2 += g * yv;
            s11 += g * (xv * xv);
            s22 += g * (yv * yv);
            s12 += g * (xv * yv);
        }
        hm[0][r][c] = m1;
        hm[1][r][c] = m2;
        hm[2][r][c] = s11;
        hm[3][r][c] = s22;
        hm[4][r][c] = s12;
    }
    __syncthreads();
    const int c = tid % kTile, r0 = (tid / kTile) * kRows;
    double acc[kRows][5];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
    for (int j = 0; j < kRows + R; ++j) {
        double v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] = hm[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            const int k = j - o;   // output row r0 + o takes tap k of halo row r0 + j: k ascends with j
            if (k >= 0 && k < WIN) {
                const double g = a.win.g[k];
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[o][m] += g * v[m];
            }
        }
    }
    const int px = tx0 + c;
    const int64_t plane = (int64_t)a.Hm * a.Wm;
    double sum = 0.0;
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int py = ty0 + r0 + o;
        const double mu1 = acc[o][0], mu2 = acc[o][1];
        const double mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
        const double s1 = acc[o][2] - mu11, s2 = acc[o][3] - mu22, s12 = acc[o][4] - mu12;
        const double cd = s1 + s2 + a.c2, ld = mu11 + mu22 + a.c1;
        const double cs = (2.0 * s12 + a.c2) / cd;
        const double l = (2.0 * mu12 + a.c1) / ld;
        const bool in = py < a.Hm && px < a.Wm;
        sum += in ? l * cs : 0.0;
        if (GRAD && in) {
            // d cs / d s1 = -cs / cd, d cs / d s12 = 2 / cd, d l / d mu1 = 2 (mu2 - l mu1) / ld; s1 and s12 carry
            // -mu1^2 and -mu1 mu2
            const double B = -l * cs / cd, Cm = 2.0 * l / cd;
            const double A = 2.0 * cs * (mu2 - l * mu1) / ld - 2.0 * mu1 * B - mu2 * Cm;
            const int64_t p = nc * plane + (int64_t)py * a.Wm + px;
            a.maps[p] = A;
            a.maps[a.NC * plane + p] = B;
            a.maps[2 * a.NC * plane + p] = Cm;
        }
    }
    sum = acn::wave_sum_d(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) t += red[i];
        a.partials[blockIdx.x] = t;
    }
}

// ssim[nc] = (the plane's tile sums, thread i taking tiles i, i + 256, ..., then a fixed tree) / Np, rounded once
__global__ void __launch_bounds__(kThreads) ssim_mean_kernel(const double* __restrict__ partials, int tiles, double np,
                                                             float* __restrict__ out) {
    __shared__ double red[kThreads / 64];
    const double* p = partials + (int64_t)blockIdx.x * tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += kThreads) acc += p[i];
    acc = acn::wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) t += red[i];
        out[blockIdx.x] = (float)(t / np);
    }
}

// The transposed filter: image pixel q = p + k collects g[ky] g[kx] M[p] from the map pixels p = q - k, 0 <= k < WIN.
// Halo row / column h of a tile is map row / column q0 - R + h; a map pixel outside the map is 0.
template <int WIN>
__global__ void __launch_bounds__(kThreads) ssim_grad_kernel(SsimArgs a) {
    constexpr int R = WIN - 1, HS = kTile + R;
    __shared__ double ms[3][HS][HS];
    __shared__ double th[3][HS][kTile];
    const int tid = threadIdx.x;
    const int64_t nc = blockIdx.x / a.tiles;
    const int tile = (int)(blockIdx.x % a.tiles);
    const int qy0 = (tile / a.tiles_x) * kTile, qx0 = (tile % a.tiles_x) * kTile;
    const int64_t plane = (int64_t)a.Hm * a.Wm;

    for (int i = tid; i < HS * HS; i += kThreads) {
        const int r = i / HS, c = i % HS;
        const int py = qy0 - R + r, px = qx0 - R + c;
        const bool in = py >= 0 && py < a.Hm && px >= 0 && px < a.Wm;
        const int64_t p = nc * plane + (int64_t)py * a.Wm + px;
#pragma unroll
        for (int m = 0; m < 3; ++m) ms[m][r][c] = in ? a.maps[m * a.NC * plane + p] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < HS * kTile; i += kThreads) {
        const int r = i / kTile, c = i % kTile;
        double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double g = a.win.g[k];
#pragma unroll
            for (int m = 0; m < 3; ++m) t[m] += g * ms[m][r][c + R - k];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) th[m][r][c] = t[m];
    }
    __syncthreads();
    const int c = tid % kTile, r0 = (tid / kTile) * kRows;
    double acc[kRows][3];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int m = 0; m < 3; ++m) acc[o][m] = 0.0;
#pragma unroll
    for (int j = 0; j < kRows + R; ++j) {
        double v[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) v[m] = th[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            const int k = o + R - j;   // image row r0 + o takes tap k of halo row r0 + o + R - k
            if (k >= 0 && k < WIN) {
                const double g = a.win.g[k];
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[o][m] += g * v[m];
            }
        }
    }
    int64_t base, ps, rs;
    plane_layout(a, nc, base, ps, rs);
    const int qx = qx0 + c;
    const double np = (double)plane;
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int qy = qy0 + r0 + o;
        if (qy < a.H && qx < a.W) {
            const int64_t q = base + qy * rs + qx * ps;
            const double xv = (double)a.x[q], yv = (double)a.y[q];
            a.grad_x[q] = (float)((acc[o][0] + 2.0 * xv * acc[o][1] + yv * acc[o][2]) / np);
        }
    }
}

int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// bytes of the tile sums and of the three gradient maps, each for the largest map an (H, W) image can have (win = 3)
size_t partial_bytes(int64_t NC, int H, int W) {
    const int64_t hm = H > 2 ? H - 2 : 0, wm = W > 2 ? W - 2 : 0;
    return (size_t)(NC * tiles_of(hm) * tiles_of(wm)) * sizeof(double);
}
size_t map_bytes(int64_t NC, int H, int W) {
    const int64_t hm = H > 2 ? H - 2 : 0, wm = W > 2 ? W - 2 : 0;
    return (size_t)(3 * NC * hm * wm) * sizeof(double);
}

template <int WIN>
int launch_ssim(const SsimArgs& fwd, float* ssim_nc, void* stream) {
    const dim3 grid((unsigned)(fwd.NC * fwd.tiles)), block(kThreads);
    if (fwd.grad_x)
        hipLaunchKernelGGL((ssim_fwd_kernel<WIN, true>), grid, block, 0, (hipStream_t)stream, fwd);
    else
        hipLaunchKernelGGL((ssim_fwd_kernel<WIN, false>), grid, block, 0, (hipStream_t)stream, fwd);
    if (int rc = acn_check_launch("acn_ssim_fwd")) return rc;
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)fwd.NC), block, 0, (hipStream_t)stream, fwd.partials, fwd.tiles,
                       (double)fwd.Hm * (double)fwd.Wm, ssim_nc);
    if (int rc = acn_check_launch("acn_ssim_fwd (mean)")) return rc;
    if (!fwd.grad_x) return ACN_OK;
    SsimArgs g = fwd;
    g.tiles_x = (int32_t)tiles_of(fwd.W);
    g.tiles = (int32_t)(tiles_of(fwd.H) * g.tiles_x);
    hipLaunchKernelGGL(ssim_grad_kernel<WIN>, dim3((unsigned)(g.NC * g.tiles)), block, 0, (hipStream_t)stream, g);
    return acn_check_launch("acn_ssim_fwd (gradient)");
}

}  // namespace

extern "C" size_t acn_ssim_workspace_bytes(int64_t N, int C, int H, int W, int want_grad) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return 16;
    const int64_t NC = N * (int64_t)C;
    return 16 + partial_bytes(NC, H, W) + (want_grad ? map_bytes(NC, H, W) : 0);
}

extern "C" int acn_ssim_fwd(const float* x, const float* y, int64_t N, int C, int H, int W, int channels_last,
                            int win_size, double win_sigma, double c1, double c2, float* ssim_nc, float* grad_x,
                            void* workspace, size_t workspace_bytes, void* stream) {
    ACN_REQUIRE(N >= 0 && C >= 1, "acn_ssim_fwd: N must be >= 0 and C >= 1 (got %lld, %d)", (long long)N, C);
    ACN_REQUIRE(win_size >= 3 && win_size <= kMaxWin && (win_size & 1),
                "acn_ssim_fwd: win_size must be odd and in 3..%d (got %d)", kMaxWin, win_size);
    ACN_REQUIRE(win_sigma > 0.0, "acn_ssim_fwd: win_sigma must be > 0 (got %g)", win_sigma);
    ACN_REQUIRE(H >= win_size && W >= win_size, "acn_ssim_fwd: H and W must be >= win_size = %d (got %d, %d)", win_size,
                H, W);
    if (N == 0) return ACN_OK;
    ACN_REQUIRE(x && y && ssim_nc && workspace, "acn_ssim_fwd: NULL pointer");
    ACN_REQUIRE(workspace_bytes >= acn_ssim_workspace_bytes(N, C, H, W, grad_x != nullptr),
                "acn_ssim_fwd: workspace too small (%zu bytes, acn_ssim_workspace_bytes gives %zu)", workspace_bytes,
                acn_ssim_workspace_bytes(N, C, H, W, grad_x != nullptr));
    SsimArgs a{};
    a.x = x;
    a.y = y;
    a.NC = N * (int64_t)C;
    a.C = C;
    a.H = H;
    a.W = W;
    a.Hm = H - win_size + 1;
    a.Wm = W - win_size + 1;
    a.tiles_x = (int32_t)tiles_of(a.Wm);
    a.tiles = (int32_t)(tiles_of(a.Hm) * a.tiles_x);
    a.channels_last = channels_last != 0;
    a.c1 = c1;
    a.c2 = c2;
    ACN_REQUIRE(a.NC * tiles_of(H) * tiles_of(W) <= 0x7fffffffLL,
                "acn_ssim_fwd: N * C * tiles = %lld exceeds the grid limit", (long long)(a.NC * tiles_of(H) * tiles_of(W)));
    a.partials = (double*)workspace;   // 16-byte aligned by the caller's allocator; the maps follow the tile sums
    a.maps = grad_x ? (double*)((char*)workspace + partial_bytes(a.NC, H, W)) : nullptr;
    a.grad_x = grad_x;
    double s = 0.0;
    for (int i = 0; i < win_size; ++i) {
        const double d = (double)(i - win_size / 2);
        a.win.g[i] = exp(-(d * d) / (2.0 * win_sigma * win_sigma));
        s += a.win.g[i];
    }
    for (int i = 0; i < win_size; ++i) a.win.g[i] /= s;
    switch (win_size) {
        case 3: return launch_ssim<3>(a, ssim_nc, stream);
        case 5: return launch_ssim<5>(a, ssim_nc, stream);
        case 7: return launch_ssim<7>(a, ssim_nc, stream);
        case 9: return launch_ssim<9>(a, ssim_nc, stream);
        default: return launch_ssim<11>(a, ssim_nc, stream);
    }
}
