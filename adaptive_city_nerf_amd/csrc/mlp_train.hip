// mlp_train.hip -- the expert MLP of the training path on fp32 MFMA (gfx950).
//
// Replaces the differentiable MetaLinear chain of MetaNGP.density / color (models/inr/meta_ngp.py:
// 171-241, models/metamodule/metamodule.py: F.linear per layer, ReLU blocks, trunc_exp, cat with the SH
// encoding, sigmoid) and its autograd backward: ~11 small GEMMs, ~40 elementwise kernels and the bias
// reductions per call become
//   acn_mlp_train_fwd: one launch -> out (M, 4) = [sigmoid(rgb), trunc_exp(sigma)] and the layer
//                      inputs the weight gradients need, each with a ones column (the bias term);
//   acn_mlp_train_bwd: one launch -> d(hash features) (M, 32) and every layer's output gradient
//                      (after the ReLU / sigmoid / trunc_exp derivative);
// then one GEMM per layer on the caller's side gives [dW | db] = dY^T . [X | 1] (large-K GEMMs);
//   acn_mlp_train_bwd_dw: the fused backward (forward re-run in registers, [dW | db] on MFMA, no saved activations);
//   acn_mlp_train_bwd_input: the input gradients alone (dL/dh0, dL/dsh) for frozen weights, one launch;
//   acn_field_sigma_grad: density and its world-space gradient for evaluation (hash gather, sigma branch forward and
//                      backward, contraction with the corner rows) in one launch, nothing else written.
//
// Execution: one wave per 32-sample tile, lanes (sample j = lane & 31, half h = lane >> 5).  Every
// layer is Y^T = W . X^T on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains) with the layer input in the
// accumulator layout of the previous layer (row rho(r, h) of sample j in register r), so activations
// never leave registers inside a pass; k-step (t, r) pairs input features 32t + rho(r, 0/1), which is
// what each half's lanes hold.  Backward layers are dX^T = W^T . dY^T the same way.  Weights are
// staged in LDS row-major with odd strides (conflict-free for both the row and column access).
// Architecture (the fused paths' reference configuration, nerf_runner.py:102-121): hash features 32
// -> 64 -> 64 (ReLU) -> [geo 15 | sigma 1] ; [geo, SH 16] -> 64 -> 64 (ReLU) -> 3 (sigmoid).
#include "acn_device.h"
#include "acn_internal.h"

// This file is compiled three times into libacnerf.so: the default build (fp16x3 layer products) exports the
// acn_mlp_* entry points, a second object built with -DACN_TRAIN_F16X3=0 -DACN_MLP_SUFFIX=_exact exports
// the exact-fp32 variants as acn_mlp_*_exact, a third built with -DACN_TRAIN_AMP=1 -DACN_MLP_SUFFIX=_amp the
// autocast(float16) arithmetic as acn_mlp_*_amp (a runtime precision switch: ops.set_train_mlp_precision).
// ACN_MLP_SUFFIX, ACN_TRAIN_F16X3 and ACN_TRAIN_AMP are the file's only build parameters.
#ifndef ACN_MLP_SUFFIX
#define ACN_MLP_SUFFIX
#endif
#define ACN_MLP_CAT2(a, b) a##b
#define ACN_MLP_CAT(a, b) ACN_MLP_CAT2(a, b)
#define ACN_MLP_API(name) ACN_MLP_CAT(name, ACN_MLP_SUFFIX)

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// Saved / gradient tensors are feature-major per group of GS samples: element (sample m, feature f) at
// [m / GS][f][m % GS], so a wave's 32 lanes (32 consecutive samples) write 128 contiguous bytes per
// feature, and the weight-gradient GEMM of a layer is a batched (out x GS) . (GS x in) over groups.
constexpr int GS = 2048;
constexpr int SS = 325;                 // saved features: [h0|1 33][a1|1 65][a2|1 65][cin|1 32][c1|1 65][c2|1 65]
constexpr int O_H0 = 0, O_A1 = 33, O_A2 = 98, O_CIN = 163, O_C1 = 195, O_C2 = 260;
constexpr int DS = 275;                 // gradient row: [da1 64][da2 64][dhead 16][dc1 64][dc2 64][drgb 3]
constexpr int G_A1 = 0, G_A2 = 64, G_HD = 128, G_C1 = 144, G_C2 = 208, G_RGB = 272;

#ifndef ACN_TRAIN_F16X3
#define ACN_TRAIN_F16X3 1  // layer products as the fp32-accurate 3-term fp16 split (0: exact fp32 MFMA)
#endif
// ACN_TRAIN_AMP (third object, acn_mlp_*_amp): the reference's use_amp arithmetic -- the chain run under
// torch.autocast(float16) (runtime_adapt.py:249-259, meta_core.py:38, configs/train.json:37).  F.linear casts
// its input and weights to fp16 and addmm returns fp16 (one fp16 x fp16 product per term, fp32 accumulation,
// the bias added, one rounding to fp16); ReLU / sigmoid / trunc_exp (custom_fwd without cast_inputs) run on
// the fp16 tensors and round their results to fp16; the backward mirrors it (the output gradient cast to
// fp16, each dX and [dW | db] rounded to fp16 once).  No per-wave rescaling: values past fp16's range
// overflow / underflow exactly as under autocast -- the loss scale (GradScaler) is the caller's.
#ifndef ACN_TRAIN_AMP
#define ACN_TRAIN_AMP 0
#endif
#if ACN_TRAIN_AMP && !ACN_TRAIN_F16X3
#error "ACN_TRAIN_AMP builds on the fp16 weight image (ACN_TRAIN_F16X3=1)"
#endif
// round to fp16 and back (the identity outside the AMP build)
__device__ __forceinline__ float amp_r(float x) {
#if ACN_TRAIN_AMP
    return (float)(_Float16)x;
#else
    return x;
#endif
}

// LDS weight image: row-major, W0 64x32, W1 64x64, Whead 32x64 (geo rows 0..14, sigma row 15, rows
// 16..31 zero), Wc0 64x31 (col 31 = 0), Wc1 64x64, Wc2 32x64 (rows 3..31 zero), then the biases
// (zero-padded to 32 rows likewise).  Padding every layer to whole 32-row tiles lets the kernels read
// operands unconditionally (no exec-masked LDS loads).  fp32 build: one float per weight, odd strides
// cols + 1 (conflict-free row and column access).  fp16x3 build: each layer region holds a plane of
// hi = f16(w) then a plane of lo = f16(w - hi), row-major f16 with strides cols + 4 halves (a lane's 4
// consecutive k-elements are one 8-B read; rows 2 banks apart); biases stay fp32.
constexpr int S32 = ACN_TRAIN_F16X3 ? 36 : 33, S64 = ACN_TRAIN_F16X3 ? 68 : 65;
constexpr int L_W0 = 0, L_W1 = L_W0 + 64 * S32, L_WH = L_W1 + 64 * S64, L_WC0 = L_WH + 32 * S64, L_WC1 = L_WC0 + 64 * S32,
              L_WC2 = L_WC1 + 64 * S64, L_B0 = L_WC2 + 32 * S64, L_B1 = L_B0 + 64, L_BH = L_B1 + 64, L_BC0 = L_BH + 32,
              L_BC1 = L_BC0 + 64, L_BC2 = L_BC1 + 64, L_FLOATS = L_BC2 + 32;
static_assert(L_FLOATS % 4 == 0, "16-B staging");
static_assert(L_B0 % 4 == 0 && L_B1 % 4 == 0 && L_BH % 4 == 0 && L_BC0 % 4 == 0 && L_BC1 % 4 == 0 && L_BC2 % 4 == 0,
              "16-B bias reads (fwd_layer)");

struct MlpPtrs {
    const float *w0, *b0, *w1, *b1, *wsh, *bsh, *wg, *bg, *wc0, *bc0, *wc1, *bc1, *wc2, *bc2;
};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// values the compiler must treat as unknown per loop iteration, so loop-invariant LDS weight reads and
// lane-address arithmetic are not hoisted out of the tile loop (and then spilled)
__device__ __forceinline__ int opaque_s(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ int opaque_v(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// the heads' activations and the first backward step (torch's derivative chain: sigmoid_backward
// g * (1 - y) * y; trunc_exp backward g * exp(xc) = g * y; threshold_backward (ReLU) g where the output > 0).
// AMP: sigmoid / exp of the fp16 pre-activations rounded to fp16; trunc_exp clamps at fp16(11.089866488) =
// 11.09375 (clamp's scalar is cast to the tensor's dtype; exp(11.09375) > 65504, so the clamped maximum is
// inf, as in the reference); the incoming gradient is cast to fp16 and each product rounded once.
__device__ __forceinline__ float out_rgb(float x) { return amp_r(acn::sigmoidf_(x)); }
__device__ __forceinline__ float out_sigma(float x) {
#if ACN_TRAIN_AMP
    const float m = 11.09375f;
    x = x < -m ? -m : x;
    x = x > m ? m : x;
    return amp_r(expf(x));
#else
    return acn::trunc_exp(x);
#endif
}
__device__ __forceinline__ float grad_rgb(float g, float y) { return amp_r((amp_r(g) * (1.0f - y)) * y); }
__device__ __forceinline__ float grad_sigma(float g, float y) { return amp_r(amp_r(g) * y); }

__device__ __forceinline__ int64_t fm_index(int64_t m, int nfeat, int f) {
    return (m / GS) * ((int64_t)nfeat * GS) + (int64_t)f * GS + (m % GS);
}

// the padded LDS image, built once per call (one element per thread), then copied by every block of
// the MLP kernels with 16-B loads
// weight (row, col) of layer region `layer` (0 W0, 1 W1, 2 head, 3 Wc0, 4 Wc1, 5 Wc2), zero in the padding
__device__ __forceinline__ float layer_w(const MlpPtrs& p, int layer, int r, int c) {
    switch (layer) {
        case 0: return c < 32 ? p.w0[r * 32 + c] : 0.0f;
        case 1: return c < 64 ? p.w1[r * 64 + c] : 0.0f;
        case 2: return c < 64 && r < 16 ? (r < 15 ? p.wg[r * 64 + c] : p.wsh[c]) : 0.0f;
        case 3: return c < 31 ? p.wc0[r * 31 + c] : 0.0f;
        case 4: return c < 64 ? p.wc1[r * 64 + c] : 0.0f;
        default: return c < 64 && r < 3 ? p.wc2[r * 64 + c] : 0.0f;
    }
}

__device__ __forceinline__ float pack_elem(const MlpPtrs& p, int e) {
    if (e < L_B0) {
        int layer, base, rows, ld;
        if (e < L_W1) { layer = 0; base = L_W0; rows = 64; ld = S32; }
        else if (e < L_WH) { layer = 1; base = L_W1; rows = 64; ld = S64; }
        else if (e < L_WC0) { layer = 2; base = L_WH; rows = 32; ld = S64; }
        else if (e < L_WC1) { layer = 3; base = L_WC0; rows = 64; ld = S32; }
        else if (e < L_WC2) { layer = 4; base = L_WC1; rows = 64; ld = S64; }
        else { layer = 5; base = L_WC2; rows = 32; ld = S64; }
        const int q = e - base;
#if ACN_TRAIN_F16X3
        // region = hi plane then lo plane, each rows x ld f16 row-major; this dword = halves (2c, 2c + 1)
        const int plane_dw = rows * ld / 2, part = q / plane_dw, hq = 2 * (q % plane_dw);
        const int r = hq / ld, c = hq % ld;
        uint32_t bits = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float w = layer_w(p, layer, r, c + u);
            const _Float16 hi = (_Float16)w;
            const _Float16 v = part ? (_Float16)(w - (float)hi) : hi;
            bits |= (uint32_t)__builtin_bit_cast(uint16_t, v) << (16 * u);
        }
        return __uint_as_float(bits);
#else
        (void)rows;
        return layer_w(p, layer, q / ld, q % ld);
#endif
    }
    if (e < L_B1) return p.b0[e - L_B0];
    if (e < L_BH) return p.b1[e - L_B1];
    if (e < L_BC0) { const int q = e - L_BH; return q < 15 ? p.bg[q] : (q == 15 ? p.bsh[0] : 0.0f); }
    if (e < L_BC1) return p.bc0[e - L_BC0];
    if (e < L_BC2) return p.bc1[e - L_BC1];
    const int q = e - L_BC2;
    return q < 3 ? p.bc2[q] : 0.0f;
}

__global__ void __launch_bounds__(256) mlp_pack_kernel(MlpPtrs p, float* __restrict__ img) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < L_FLOATS) img[e] = pack_elem(p, e);
}

// the images of K experts at once (routed pair lists): blockIdx.y = expert
struct MlpPtrsK {
    MlpPtrs e[acn::kMaxK];
};
__global__ void __launch_bounds__(256) mlp_pack_multi_kernel(MlpPtrsK p, float* __restrict__ imgs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < L_FLOATS) imgs[(int64_t)blockIdx.y * L_FLOATS + e] = pack_elem(p.e[blockIdx.y], e);
}

__device__ __forceinline__ void stage_weights(const float* __restrict__ img, float* s) {
    const float4* src = reinterpret_cast<const float4*>(img);
    float4* dst = reinterpret_cast<float4*>(s);
    for (int e = threadIdx.x; e < L_FLOATS / 4; e += blockDim.x) dst[e] = src[e];
}

#if ACN_TRAIN_F16X3
// ---- fp16x3 layers: every product as hi*hi + hi*lo + lo*hi of hi = f16(x), lo = f16(x - hi) on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation (dropping lo*lo: ~2^-22 relative, like the fused render,
// DESIGN.md 4).  fp16's range is handled per layer and wave: the layer input (activations, or the
// output gradients in the backward, which sit far below fp16's normal range) is multiplied by a
// wave-uniform power of two that brings its max |x| into [2^13, 2^14) and the accumulator is multiplied
// back -- both exact.  B operand = the input in the accumulator layout of the previous layer: k-element
// e of lane half h at k-step s is register 8 (s & 1) + e of tile s >> 1, i.e. input row xrow(s, h, e).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma_h(const f16x8& a, const f16x8& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int xrow(int s, int h, int e) { return 32 * (s >> 1) + 16 * (s & 1) + 8 * (e >> 2) + 4 * h + (e & 3); }

// wave-uniform exponent k with max |x| * 2^k in [2^13, 2^14) (0 for an all-zero / non-finite tile set)
template <int KT>
__device__ __forceinline__ int tile_scale_exp(const f32x16 (&X)[KT]) {
    // max of |x| as the integer order of the magnitude bits (NaN sorts above inf: the tile then gets k = 0)
    uint32_t m = 0u;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t b = __float_as_uint(X[t][r]) & 0x7fffffffu;
            m = b > m ? b : m;
        }
    // within each row of 16 lanes on DPP (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror),
    // then the four rows through scalar readlanes: no LDS round trip
    auto dmax = [](uint32_t v, uint32_t w) { return v > w ? v : w; };
    m = dmax(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false));
    m = dmax(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));
    m = dmax(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false));
    m = dmax(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, false));
    uint32_t w = dmax(dmax((uint32_t)__builtin_amdgcn_readlane((int)m, 0), (uint32_t)__builtin_amdgcn_readlane((int)m, 16)),
                      dmax((uint32_t)__builtin_amdgcn_readlane((int)m, 32), (uint32_t)__builtin_amdgcn_readlane((int)m, 48)));
    if (w == 0u || w >= 0x7f800000u) return 0;      // all zero, or inf / NaN present
    // max = f * 2^e, f in [0.5, 1): the biased exponent field gives e (subnormals: treat as 2^-126)
    const int be = (int)(w >> 23);
    const int e = (be == 0 ? -126 : be - 127) + 1;
    int k = 14 - e;
    return k > 100 ? 100 : (k < -100 ? -100 : k);
}

template <int KT>
__device__ __forceinline__ void split_tiles(const f32x16 (&X)[KT], int k, f16x8 (&bh)[2 * KT], f16x8 (&bl)[2 * KT]) {
    // hi = f16(x), lo = f16(x - hi) (the difference is exact), both rounded to nearest even; per pair of
    // elements the compiler emits one packed scale (v_pk_mul_f32), two packed conversions
    // (v_cvt_pk_f16_f32), two f16 -> f32 conversions and one packed subtraction -- no inline assembly, so
    // the compiler's hazard tracking sees every instruction.  hi + lo keeps ~22 bits of x (a truncating
    // hi, v_cvt_pkrtz, doubles lo and quadruples the dropped lo*lo term).
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const float sc = ldexpf(1.0f, k);
    const f32x2 sc2 = {sc, sc};
#pragma unroll
    for (int s = 0; s < 2 * KT; ++s) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x2 x = (f32x2){X[s >> 1][8 * (s & 1) + 2 * q], X[s >> 1][8 * (s & 1) + 2 * q + 1]} * sc2;
            const f16x2 h = __builtin_convertvector(x, f16x2);
            const f16x2 l = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), f16x2);
            bh[s][2 * q] = h[0];
            bh[s][2 * q + 1] = h[1];
            bl[s][2 * q] = l[0];
            bl[s][2 * q + 1] = l[1];
        }
    }
}

// AMP: the layer input cast to fp16 as F.linear under autocast does (B operand layout as split_tiles)
template <int KT>
__device__ __forceinline__ void cvt_tiles(const f32x16 (&X)[KT], f16x8 (&bh)[2 * KT]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int s = 0; s < 2 * KT; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f16x2 h = __builtin_convertvector(((f32x2){X[s >> 1][8 * (s & 1) + 2 * q], X[s >> 1][8 * (s & 1) + 2 * q + 1]}), f16x2);
            bh[s][2 * q] = h[0];
            bh[s][2 * q + 1] = h[1];
        }
}

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f16x8 cat44(const f16x4& a, const f16x4& b) {
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Y[to] (rows 32to..) = b + W . X  (W: hi / lo planes of 32*NT padded rows, ld = stride in halves,
// ROWS = rows of the region; X: KT input tiles).  The output tiles run one after the other, each on its own
// MFMA chain (interleaving the tiles' chains per k-step measured slower).
template <int NT, int KT, int ROWS>
__device__ __forceinline__ void fwd_layer(const float* W, int ld, const float* b, const f32x16 (&X)[KT],
                                          f32x16 (&Y)[NT], int lane) {
    const int i = lane & 31, h = lane >> 5;
#if ACN_TRAIN_AMP
    (void)ROWS;
    f16x8 bh[2 * KT];
    cvt_tiles<KT>(X, bh);
    const _Float16* Wh = reinterpret_cast<const _Float16*>(W);
#pragma unroll
    for (int to = 0; to < NT; ++to) {
        const int ro = (32 * to + i) * ld;
        f32x16 acc = 0.0f;
#pragma unroll
        for (int s = 0; s < 2 * KT; ++s) {
            const int c0 = ro + 32 * (s >> 1) + 16 * (s & 1) + 4 * h;
            const f16x8 ahi = cat44(*reinterpret_cast<const f16x4*>(Wh + c0), *reinterpret_cast<const f16x4*>(Wh + c0 + 8));
            acc = mfma_h(ahi, bh[s], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[to][r] = amp_r(acc[r] + amp_r(b[32 * to + rho(r, h)]));
    }
#else
    const int k = tile_scale_exp<KT>(X);
    const float usc = ldexpf(1.0f, -k);
    f16x8 bh[2 * KT], bl[2 * KT];
    split_tiles<KT>(X, k, bh, bl);
    const _Float16* Wh = reinterpret_cast<const _Float16*>(W);
    const _Float16* Wlo = Wh + ROWS * ld;
#pragma unroll
    for (int to = 0; to < NT; ++to) {
        const int ro = (32 * to + i) * ld;
        f32x16 acc = 0.0f;
        // the next k-step's A operands are read while this k-step's MFMAs run (same chain, same order)
        auto lda = [&](int s, f16x8& ahi, f16x8& alo) {
            const int c0 = ro + 32 * (s >> 1) + 16 * (s & 1) + 4 * h;
            ahi = cat44(*reinterpret_cast<const f16x4*>(Wh + c0), *reinterpret_cast<const f16x4*>(Wh + c0 + 8));
            alo = cat44(*reinterpret_cast<const f16x4*>(Wlo + c0), *reinterpret_cast<const f16x4*>(Wlo + c0 + 8));
        };
        f16x8 ahi, alo;
        lda(0, ahi, alo);
#pragma unroll
        for (int s = 0; s < 2 * KT; ++s) {
            f16x8 nhi = ahi, nlo = alo;
            if (s + 1 < 2 * KT) lda(s + 1, nhi, nlo);
            acc = mfma_h(alo, bh[s], acc);
            acc = mfma_h(ahi, bl[s], acc);
            acc = mfma_h(ahi, bh[s], acc);
            ahi = nhi;
            alo = nlo;
        }
        // acc * 2^-k + b in one rounding (the scaling itself is exact); the bias rows rho(4q .. 4q + 3, h) are 4
        // consecutive floats, read as one 16-B vector each (the image's bias regions are 16-B aligned)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            typedef float f32x4b __attribute__((ext_vector_type(4)));
            const f32x4b bv = *reinterpret_cast<const f32x4b*>(b + 32 * to + 8 * q + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) Y[to][4 * q + e] = __builtin_fmaf(acc[4 * q + e], usc, bv[e]);
        }
    }
#endif
}

// the backward layers read W transposed on ds_read_b64_tr_b16
typedef __fp16 hf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) hf16x4 lds_hf16x4;
// ds_read_b64_tr_b16 (gfx950): per 16-lane group, lane 4q + p supplies the address of row q, columns 4p..4p+3
// of a 4 x 16 block of 16-bit elements; lane i of the group receives column i, row q in element q.  The
// address must point into LDS, 8-B aligned; EXEC must be all ones (every caller is wave-uniform).
__device__ __forceinline__ f16x4 ds_read_tr16(const _Float16* p) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_hf16x4*)(p)));
}

// dX[ti] (input features 32ti..) = W^T . dY  (W rows = output features; k-steps whose 16 rows are all
// >= NROW are skipped at compile time, padding rows inside a k-step are zero in the image).  The A operand
// of lane (i, h) at k-step s is column 32 ti + i of W at rows xrow(s, h, 0..7) = base + 4h + 0..3 and
// base + 8 + 4h + 0..3: two 4-row blocks, each one transposed read per plane (lane (g, q, p) of 16-lane
// group g addresses row base [+ 8] + 4h + q, columns 32 ti + 16 (g & 1) + 4p).
template <int NT, int KT, int NROW, int ROWS>
__device__ __forceinline__ void bwd_layer(const float* W, int ld, const f32x16 (&dY)[KT], f32x16 (&dX)[NT],
                                          int lane) {
    const int h = lane >> 5;
#if ACN_TRAIN_AMP
    (void)ROWS;
    f16x8 bh[2 * KT];
    cvt_tiles<KT>(dY, bh);
    const _Float16* Wh = reinterpret_cast<const _Float16*>(W);
    const int trow = 4 * h + ((lane >> 2) & 3), tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        f32x16 acc = 0.0f;
#pragma unroll
        for (int s = 0; s < 2 * KT; ++s) {
            if (32 * (s >> 1) + 16 * (s & 1) >= NROW) continue;
            const int o = (32 * (s >> 1) + 16 * (s & 1) + trow) * ld + 32 * ti + tcol;
            const f16x8 ahi = cat44(ds_read_tr16(Wh + o), ds_read_tr16(Wh + o + 8 * ld));
            acc = mfma_h(ahi, bh[s], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dX[ti][r] = amp_r(acc[r]);
    }
#else
    const int k = tile_scale_exp<KT>(dY);
    const float usc = ldexpf(1.0f, -k);
    f16x8 bh[2 * KT], bl[2 * KT];
    split_tiles<KT>(dY, k, bh, bl);
    const _Float16* Wh = reinterpret_cast<const _Float16*>(W);
    const _Float16* Wlo = Wh + ROWS * ld;
    const int trow = 4 * h + ((lane >> 2) & 3), tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    // as fwd_layer: the next live k-step's A operands are read while this k-step's MFMAs run (same chain, order)
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        auto ldb = [&](int s, f16x8& ahi, f16x8& alo) {
            const int o = (32 * (s >> 1) + 16 * (s & 1) + trow) * ld + 32 * ti + tcol;
            ahi = cat44(ds_read_tr16(Wh + o), ds_read_tr16(Wh + o + 8 * ld));
            alo = cat44(ds_read_tr16(Wlo + o), ds_read_tr16(Wlo + o + 8 * ld));
        };
        f32x16 acc = 0.0f;
        f16x8 ahi, alo;
        ldb(0, ahi, alo);
#pragma unroll
        for (int s = 0; s < 2 * KT; ++s) {
            if (32 * (s >> 1) + 16 * (s & 1) >= NROW) continue;
            f16x8 nhi = ahi, nlo = alo;
            if (s + 1 < 2 * KT && 32 * ((s + 1) >> 1) + 16 * ((s + 1) & 1) < NROW) ldb(s + 1, nhi, nlo);
            acc = mfma_h(alo, bh[s], acc);
            acc = mfma_h(ahi, bl[s], acc);
            acc = mfma_h(ahi, bh[s], acc);
            ahi = nhi;
            alo = nlo;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dX[ti][r] = acc[r] * usc;
    }
#endif
}
#else
// Y[to] (rows 32to..) = b + W . X  (W: 32*NT padded rows, ld = stride; X: KT input tiles).  The A operands
// of an output tile are read into registers before its MFMA chain.
template <int NT, int KT, int ROWS>
__device__ __forceinline__ void fwd_layer(const float* W, int ld, const float* b, const f32x16 (&X)[KT],
                                          f32x16 (&Y)[NT], int lane) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int to = 0; to < NT; ++to) {
        const float* wr = W + (32 * to + i) * ld;
        float a[KT][16];
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[t][r] = wr[32 * t + rho(r, h)];
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[to][r] = b[32 * to + rho(r, h)];
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) Y[to] = mfma32(a[t][r], X[t][r], Y[to]);
    }
}

// dX[ti] (input features 32ti..) = W^T . dY  (W rows = output features; k-steps whose rows are all
// >= NROW are skipped at compile time, the other lane half reads zero padding rows)
template <int NT, int KT, int NROW, int ROWS>
__device__ __forceinline__ void bwd_layer(const float* W, int ld, const f32x16 (&dY)[KT], f32x16 (&dX)[NT],
                                          int lane) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        float a[KT][16];
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (32 * t + rho(r, 0) < NROW) a[t][r] = W[(32 * t + rho(r, h)) * ld + 32 * ti + i];
        dX[ti] = 0.0f;
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (32 * t + rho(r, 0) < NROW) dX[ti] = mfma32(a[t][r], dY[t][r], dX[ti]);
    }
}

#endif

template <int NT>
__device__ __forceinline__ void relu(f32x16 (&Y)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[t][r] = Y[t][r] > 0.0f ? Y[t][r] : 0.0f;
}

// feature-major (GS groups) <-> accumulator tiles of sample m
template <int NT>
__device__ __forceinline__ void load_fm(const float* src, int nall, int off, int nfeat, int64_t m, bool ok, int h,
                                        f32x16 (&X)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * t + rho(r, h);
            X[t][r] = (ok && f < nfeat) ? src[fm_index(m, nall, off + f)] : 0.0f;
        }
}
template <int NT>
__device__ __forceinline__ void store_fm(float* dst, int nall, int off, int nfeat, int64_t m, bool ok, int h,
                                         const f32x16 (&X)[NT]) {
    if (!ok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * t + rho(r, h);
            if (f < nfeat) dst[fm_index(m, nall, off + f)] = amp_r(X[t][r]);
        }
}

// row-major (M, stride) <-> accumulator tiles of sample (base + j)
template <int NT>
__device__ __forceinline__ void load_tiles(const float* src, int64_t stride, int off, int nfeat, int64_t m, bool ok,
                                           int h, f32x16 (&X)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * t + rho(r, h);
            X[t][r] = (ok && f < nfeat) ? src[m * stride + off + f] : 0.0f;
        }
}
template <int NT>
__device__ __forceinline__ void store_tiles(float* dst, int64_t stride, int off, int nfeat, int64_t m, bool ok, int h,
                                            const f32x16 (&X)[NT]) {
    if (!ok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * t + rho(r, h);
            if (f < nfeat) dst[m * stride + off + f] = X[t][r];
        }
}

// forward of one tile: everything the backward needs is recomputable from h0 + sh, but the weight
// gradients need the layer inputs in memory anyway, so they are saved here
__device__ __forceinline__ void tile_forward(const float* Wl, const float* h0, const float* sh, int64_t m, bool ok,
                                             int lane, f32x16 (&X0)[1], f32x16 (&A1)[2], f32x16 (&A2)[2],
                                             f32x16 (&Hd)[1], f32x16 (&Cin)[1], f32x16 (&C1)[2], f32x16 (&C2)[2],
                                             f32x16 (&Rg)[1]) {
    const int h = lane >> 5;
    load_tiles<1>(h0, 32, 0, 32, m, ok, h, X0);
    fwd_layer<2, 1, 64>(Wl + L_W0, S32, Wl + L_B0, X0, A1, lane);
    relu<2>(A1);
    fwd_layer<2, 2, 64>(Wl + L_W1, S64, Wl + L_B1, A1, A2, lane);
    relu<2>(A2);
    fwd_layer<1, 2, 32>(Wl + L_WH, S64, Wl + L_BH, A2, Hd, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = rho(r, h);
        Cin[0][r] = f < 15 ? Hd[0][r] : ((ok && f < 31) ? sh[m * 16 + (f - 15)] : 0.0f);
    }
    fwd_layer<2, 1, 64>(Wl + L_WC0, S32, Wl + L_BC0, Cin, C1, lane);
    relu<2>(C1);
    fwd_layer<2, 2, 64>(Wl + L_WC1, S64, Wl + L_BC1, C1, C2, lane);
    relu<2>(C2);
    fwd_layer<1, 2, 32>(Wl + L_WC2, S64, Wl + L_BC2, C2, Rg, lane);
}

// Prefetched per-sample inputs of the producer waves (mlp_bwd_dw_pc_kernel): whole 16-B vectors at a clamped
// sample index (no per-element exec branches), issued well ahead of their use and masked for samples past the
// end only where they are consumed -- a scheduling barrier after the loads keeps the compiler from sinking them
// to their uses.  The values are those load_tiles / tile_forward and the per-element output / output-gradient
// reads of mlp_bwd_kernel take.
struct X0Raw {
    float4 v[4];   // h0 row elements rho(4q .. 4q + 3, h) = 8q + 4h + 0..3
};
__device__ __forceinline__ void load_x0raw(const float* __restrict__ h0, int64_t m, bool ok, int h, X0Raw& x) {
    const float4* p = reinterpret_cast<const float4*>(h0 + (ok ? m : 0) * 32 + 4 * h);
#pragma unroll
    for (int q = 0; q < 4; ++q) x.v[q] = p[2 * q];
}
__device__ __forceinline__ void x0_tile(const X0Raw& x, bool ok, f32x16 (&X)[1]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        X[0][4 * q] = ok ? x.v[q].x : 0.0f;
        X[0][4 * q + 1] = ok ? x.v[q].y : 0.0f;
        X[0][4 * q + 2] = ok ? x.v[q].z : 0.0f;
        X[0][4 * q + 3] = ok ? x.v[q].w : 0.0f;
    }
}
struct PcIn {      // issued after the forward's first layer (its h0 tile's registers are free by then)
    float s[9];    // SH row value of accumulator row r = 7 .. 15 (rho(r, h) - 15, clamped; rows r < 7 are geo)
    float o[3], g[3];   // outputs / output gradients: h == 0 lanes rgb, h == 1 lanes sigma (in all three)
};
__device__ __forceinline__ void load_pcin(const float* __restrict__ sh, const float* __restrict__ out,
                                          const float* __restrict__ gout, int64_t m, bool ok, int h, PcIn& in) {
    const int64_t mc = ok ? m : 0;
#pragma unroll
    for (int r = 7; r < 16; ++r) {
        const int f = rho(r, h) - 15;
        in.s[r - 7] = sh[mc * 16 + (f < 0 ? 0 : (f > 15 ? 15 : f))];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        in.o[c] = out[mc * 4 + (h ? 3 : c)];
        in.g[c] = gout[mc * 4 + (h ? 3 : c)];
    }
}
__device__ __forceinline__ float opaque_f(float v) {   // pins a prefetched value's first use (and its wait) here
    asm volatile("" : "+v"(v));
    return v;
}
// tile_forward on a prefetched h0 tile, issuing the SH / output loads behind the first layer (bitwise the same
// layers and values)
__device__ __forceinline__ void tile_forward_x(const float* Wl, const X0Raw& x0, const float* __restrict__ sh,
                                               const float* __restrict__ out, const float* __restrict__ gout,
                                               int64_t m, bool ok, int lane, PcIn& in, f32x16 (&A1)[2],
                                               f32x16 (&A2)[2], f32x16 (&Hd)[1], f32x16 (&Cin)[1],
                                               f32x16 (&C1)[2], f32x16 (&C2)[2], f32x16 (&Rg)[1]) {
    const int h = lane >> 5;
    {
        f32x16 X0[1];
        x0_tile(x0, ok, X0);
        fwd_layer<2, 1, 64>(Wl + L_W0, S32, Wl + L_B0, X0, A1, lane);
    }
    relu<2>(A1);
    __builtin_amdgcn_sched_barrier(0);
    load_pcin(sh, out, gout, m, ok, h, in);
    __builtin_amdgcn_sched_barrier(0);
    fwd_layer<2, 2, 64>(Wl + L_W1, S64, Wl + L_B1, A1, A2, lane);
    relu<2>(A2);
    fwd_layer<1, 2, 32>(Wl + L_WH, S64, Wl + L_BH, A2, Hd, lane);
    __builtin_amdgcn_sched_barrier(0);
    float sv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sv[k] = opaque_f(in.s[k]);   // unconditional: selects below, no branches
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = rho(r, h);
        Cin[0][r] = f < 15 ? Hd[0][r] : ((ok && f < 31 && r >= 7) ? sv[r >= 7 ? r - 7 : 0] : 0.0f);
    }
    fwd_layer<2, 1, 64>(Wl + L_WC0, S32, Wl + L_BC0, Cin, C1, lane);
    relu<2>(C1);
    fwd_layer<2, 2, 64>(Wl + L_WC1, S64, Wl + L_BC1, C1, C2, lane);
    relu<2>(C2);
    fwd_layer<1, 2, 32>(Wl + L_WC2, S64, Wl + L_BC2, C2, Rg, lane);
}

// SAVE: write the layer inputs for the split backward (keeps every activation live to the end of the tile:
// ~250 VGPRs, 4-wave blocks).  The no-save instantiation -- every fused-path call -- needs ~124 registers, so it
// runs 8-wave blocks: two blocks (the 72 KB weight image each) = four waves per SIMD.
template <bool SAVE>
__global__ void __launch_bounds__(SAVE ? 256 : 512) mlp_fwd_kernel(const float* __restrict__ img, const float* __restrict__ h0,
                                                      const float* __restrict__ sh, int64_t M,
                                                      float* __restrict__ out, float* __restrict__ save) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    stage_weights(img, Wl);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const int64_t ntiles = (M + 31) / 32;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
        const int64_t m = tile * 32 + j;
        const bool ok = m < M;
        f32x16 X0[1], A1[2], A2[2], Hd[1], Cin[1], C1[2], C2[2], Rg[1];
        // opaque base: the LDS weight reads are re-issued per tile instead of hoisted out of the loop into
        // ~240 held registers (one wave per SIMD; with it the no-save form fits two)
        tile_forward(Wl + opaque_s(0), h0, sh, m, ok, lane, X0, A1, A2, Hd, Cin, C1, C2, Rg);
        if (ok) {
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[m * 4 + c] = out_rgb(Rg[0][c]);
            } else {
                out[m * 4 + 3] = out_sigma(Hd[0][7]);  // row 15 = sigma head (lane half 1, reg 7)
            }
            if (SAVE) {
                // layer inputs (+ ones columns for the bias gradient), feature-major
#pragma unroll
                for (int r = 0; r < 16; ++r) save[fm_index(m, SS, O_H0 + rho(r, h))] = amp_r(h0[m * 32 + rho(r, h)]);
                store_fm<2>(save, SS, O_A1, 64, m, ok, h, A1);
                store_fm<2>(save, SS, O_A2, 64, m, ok, h, A2);
                store_fm<1>(save, SS, O_CIN, 31, m, ok, h, Cin);
                store_fm<2>(save, SS, O_C1, 64, m, ok, h, C1);
                store_fm<2>(save, SS, O_C2, 64, m, ok, h, C2);
                if (h == 0) {
                    save[fm_index(m, SS, O_H0 + 32)] = 1.0f;
                    save[fm_index(m, SS, O_A1 + 64)] = 1.0f;
                    save[fm_index(m, SS, O_A2 + 64)] = 1.0f;
                } else {
                    save[fm_index(m, SS, O_CIN + 31)] = 1.0f;
                    save[fm_index(m, SS, O_C1 + 64)] = 1.0f;
                    save[fm_index(m, SS, O_C2 + 64)] = 1.0f;
                }
            }
        }
    }
}

// torch's derivative chain: sigmoid_backward g * (1 - y) * y; trunc_exp backward g * exp(xc) = g * y;
// threshold_backward (ReLU) g where the saved output > 0
__global__ void __launch_bounds__(256) mlp_bwd_kernel(const float* __restrict__ img, const float* __restrict__ save,
                                                      const float* __restrict__ out, const float* __restrict__ gout,
                                                      int64_t M, float* __restrict__ gsave,
                                                      float* __restrict__ gh0) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    stage_weights(img, Wl);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const int64_t ntiles = (M + 31) / 32;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
        const int64_t m = tile * 32 + j;
        const bool ok = m < M;
        // output-layer gradients (rgb rows 0..2 of the colour head; sigma = head row 15)
        f32x16 dRg[1], dHd[1];
        dRg[0] = 0.0f;
        dHd[0] = 0.0f;
        float dsig = 0.0f;
        if (ok) {
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float y = out[m * 4 + c];
                    dRg[0][c] = grad_rgb(gout[m * 4 + c], y);
                }
            } else {
                dsig = grad_sigma(gout[m * 4 + 3], out[m * 4 + 3]);
            }
        }
        store_fm<1>(gsave, DS, G_RGB, 3, m, ok, h, dRg);
        f32x16 G2[2], G1[2], Gc[1], mask[2];
        bwd_layer<2, 1, 3, 32>(Wl + L_WC2, S64, dRg, G2, lane);
        load_fm<2>(save, SS, O_C2, 64, m, ok, h, mask);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) G2[t][r] = mask[t][r] > 0.0f ? G2[t][r] : 0.0f;
        store_fm<2>(gsave, DS, G_C2, 64, m, ok, h, G2);
        bwd_layer<2, 2, 64, 64>(Wl + L_WC1, S64, G2, G1, lane);
        load_fm<2>(save, SS, O_C1, 64, m, ok, h, mask);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) G1[t][r] = mask[t][r] > 0.0f ? G1[t][r] : 0.0f;
        store_fm<2>(gsave, DS, G_C1, 64, m, ok, h, G1);
        bwd_layer<1, 2, 64, 64>(Wl + L_WC0, S32, G1, Gc, lane);  // d cin: rows 0..14 = d geo (SH rows dropped)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = rho(r, h);
            dHd[0][r] = f < 15 ? Gc[0][r] : (f == 15 ? dsig : 0.0f);
        }
        store_fm<1>(gsave, DS, G_HD, 16, m, ok, h, dHd);
        f32x16 GA2[2], GA1[2], GH[1];
        bwd_layer<2, 1, 16, 32>(Wl + L_WH, S64, dHd, GA2, lane);
        load_fm<2>(save, SS, O_A2, 64, m, ok, h, mask);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) GA2[t][r] = mask[t][r] > 0.0f ? GA2[t][r] : 0.0f;
        store_fm<2>(gsave, DS, G_A2, 64, m, ok, h, GA2);
        bwd_layer<2, 2, 64, 64>(Wl + L_W1, S64, GA2, GA1, lane);
        load_fm<2>(save, SS, O_A1, 64, m, ok, h, mask);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) GA1[t][r] = mask[t][r] > 0.0f ? GA1[t][r] : 0.0f;
        store_fm<2>(gsave, DS, G_A1, 64, m, ok, h, GA1);
        bwd_layer<1, 2, 64, 64>(Wl + L_W0, S32, GA1, GH, lane);
        if (gh0) store_tiles<1>(gh0, 32, 0, 32, m, ok, h, GH);
    }
}

// ---------------------------------------------------------------------------------------------
// Fused backward with the weight gradients (acn_mlp_train_bwd_dw, mlp_bwd_dw_pc_kernel below).  A workgroup
// takes 4 tiles (128 samples) per round.  Its four producer waves each re-run the forward of one tile from
// h0 / sh (the layers of mlp_fwd_kernel, so the activations are bit-identical) instead of reading saved
// activations, and run the backward chain layer by layer.  At each layer they put dY and X of their tiles into
// one shared LDS stage [feature][128 samples]; after a barrier, consumer wave w forms its share of that layer's
// [dW | db] over all 128 samples on v_mfma_f32_16x16x4_f32 (row block w of the 64-row layers, column
// block w of the sigma / colour heads), accumulating in registers that live for the whole kernel:
// every gradient element has exactly one owner wave, so there are no atomics, and a workgroup writes
// its 13,715 partial sums once at the end (mlp_dw_reduce_kernel adds the workgroups' copies).
// Nothing per sample is written except dL/dh0.
constexpr int D_W0 = 0, D_B0 = 2048, D_W1 = 2112, D_B1 = 6208, D_WSH = 6272, D_BSH = 6336, D_WG = 6337,
              D_BG = 7297, D_WC0 = 7312, D_BC0 = 9296, D_WC1 = 9360, D_BC1 = 13456, D_WC2 = 13520, D_BC2 = 13712,
              NDW = 13715;
constexpr int SW = 132;                  // stage row stride (floats): 128 samples + 4, 16-B aligned rows
constexpr int X_ROW = 64;                // stage rows 0..63 = dY, 64..127 = X
constexpr int MAX_DW_BLOCKS = 256;       // partial copies (workgroups) of the fused backward

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int NT>
__device__ __forceinline__ void relu_mask(f32x16 (&G)[NT], const f32x16 (&Y)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) G[t][r] = Y[t][r] > 0.0f ? G[t][r] : 0.0f;
}

// ---- the stage and its contraction.  The default and exact builds stage fp32 values and contract them on
// v_mfma_f32_16x16x4_f32.  (Staging an fp16x3 split instead, by the producers as two f16 planes or by the
// consumers as they read, measured slower both ways: the dW phase is bound by the staging and the LDS traffic,
// not by the fp32 MFMAs that saves; docs/DESIGN_HISTORY.md 4i.)  The AMP build stages one plane of fp16 values:
// its dY and X are fp16 values already, so one v_mfma_f32_16x16x16_f16 product per term is exact (fp32
// accumulation), as autocast's fp16 GEMM computes it -- unscaled, what autocast's GEMM sees.
#if ACN_TRAIN_AMP
// The stage holds one f16 plane of [144 rows][SH halves]: rows 0..63 dY, 64..127 X, row 128 ones (rows
// 129..143 zero) -- the bias sums come out of the MFMA as the contraction with the ones row.  Per round and
// block the 128-sample contraction is 8 k-steps of v_mfma_f32_16x16x16_f16 into a temporary, added to the
// persistent fp32 accumulator.
constexpr int SH = 136;                   // stage row stride (halves): 128 samples + 8, 16-B aligned rows
constexpr int ST_ROWS = 144, ST_ONES = 128;
constexpr int ST_FLOATS = ST_ROWS * SH / 2;
__device__ __forceinline__ f32x4 mfma16h(const f16x4& a, const f16x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
typedef f32x4 BiasAcc;

__device__ __forceinline__ void stage_init(float* st) {  // the ones row (zero elsewhere there)
    _Float16* hp = reinterpret_cast<_Float16*>(st);
    for (int e = threadIdx.x; e < (ST_ROWS - ST_ONES) * SH; e += blockDim.x)
        hp[ST_ONES * SH + e] = (_Float16)(e < SH ? 1.0f : 0.0f);
}

// rows of accumulator-layout tiles -> stage[row0 + feature][32 * w + sample], rounded to fp16
template <int NT>
__device__ __forceinline__ void stage_put(float* st, int row0, const f32x16 (&T)[NT], int w, int lane) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    _Float16* hp = reinterpret_cast<_Float16*>(st);
    const int j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const f16x2 hi = __builtin_convertvector(((f32x2){T[t][r], T[t][r + 1]}), f16x2);
            hp[(row0 + 32 * t + rho(r, h)) * SH + 32 * w + j] = hi[0];
            hp[(row0 + 32 * t + rho(r + 1, h)) * SH + 32 * w + j] = hi[1];
        }
}

// acc[n] += dY[16 rows from arow] . X[16 features from xrow + 16 n]^T over the 128 staged samples,
// bacc (column 0) += the dY rows' sums; lane (i = l & 15, q = l >> 4) supplies k-elements = samples
// 32 q + 4 t + 0..3 of k-step t
template <int NCB, bool PIPE>   // PIPE: the fp32 stage's option (unused here)
__device__ __forceinline__ void dw_blocks(const float* st, int arow, int xrow, f32x4 (&acc)[NCB], BiasAcc& bacc,
                                          int lane) {
    const _Float16* hp = reinterpret_cast<const _Float16*>(st);
    const int i = lane & 15, q = lane >> 4;
    const int oa = (arow + i) * SH + 32 * q, ob = (xrow + i) * SH + 32 * q, oo = (ST_ONES + i) * SH + 32 * q;
    f32x4 tmp[NCB], tb = 0.0f;
#pragma unroll
    for (int n = 0; n < NCB; ++n) tmp[n] = 0.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f16x4 ah = *reinterpret_cast<const f16x4*>(hp + oa + 4 * t);
        const f16x4 on = *reinterpret_cast<const f16x4*>(hp + oo + 4 * t);
        tb = mfma16h(ah, on, tb);
#pragma unroll
        for (int n = 0; n < NCB; ++n) {
            const f16x4 bh = *reinterpret_cast<const f16x4*>(hp + ob + 16 * n * SH + 4 * t);
            tmp[n] = mfma16h(ah, bh, tmp[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[n][r] += tmp[n][r];
#pragma unroll
    for (int r = 0; r < 4; ++r) bacc[r] += tb[r];
}
#else
constexpr int ST_FLOATS = 128 * SW;
typedef float BiasAcc;
__device__ __forceinline__ void stage_init(float*) {}
// rows of accumulator-layout tiles -> stage[row0 + feature][32 * w + sample] (all 32 * NT rows; rows past a
// layer's width hold zeros in the tiles)
template <int NT>
__device__ __forceinline__ void stage_put(float* st, int row0, const f32x16 (&T)[NT], int w, int lane) {
    const int j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[(row0 + 32 * t + rho(r, h)) * SW + 32 * w + j] = T[t][r];
}

// acc[n] += dY[16 rows from arow] . X[16 features from xrow + 16 n]^T over the 128 staged samples;
// lane (i = l & 15, q = l >> 4) supplies k = sample 32 q + kk (4 k-steps per 16-B read).  bsum += this
// lane's share of the bias row sum (the A operand is dY itself).
template <int NCB, bool PIPE>
__device__ __forceinline__ void dw_blocks(const float* st, int arow, int xrow, f32x4 (&acc)[NCB], float& bsum,
                                          int lane) {
    const int i = lane & 15, q = lane >> 4;
    const float* pa = st + (arow + i) * SW + 32 * q;
    const float* pb = st + (xrow + i) * SW + 32 * q;
    if (PIPE) {
    // software-pipelined: the next k-step's A / B vectors are read while this one's MFMAs run, and the MFMAs
    // of the NCB independent blocks alternate (each block's own chain keeps its k order: the same sums bit for
    // bit as the plain loop below)
    f32x4 a = *reinterpret_cast<const f32x4*>(pa);
    f32x4 b[NCB];
#pragma unroll
    for (int n = 0; n < NCB; ++n) b[n] = *reinterpret_cast<const f32x4*>(pb + 16 * n * SW);
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) {
        f32x4 an = a, bn[NCB];
#pragma unroll
        for (int n = 0; n < NCB; ++n) bn[n] = b[n];
        if (k4 < 7) {
            an = *reinterpret_cast<const f32x4*>(pa + 4 * (k4 + 1));
#pragma unroll
            for (int n = 0; n < NCB; ++n) bn[n] = *reinterpret_cast<const f32x4*>(pb + 16 * n * SW + 4 * (k4 + 1));
        }
        bsum += (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < NCB; ++n) acc[n] = mfma16(a[e], b[n][e], acc[n]);
        a = an;
#pragma unroll
        for (int n = 0; n < NCB; ++n) b[n] = bn[n];
    }
    return;
    }
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(pa + 4 * k4);
        bsum += (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
        for (int n = 0; n < NCB; ++n) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(pb + 16 * n * SW + 4 * k4);
            acc[n] = mfma16(a[0], b[0], acc[n]);
            acc[n] = mfma16(a[1], b[1], acc[n]);
            acc[n] = mfma16(a[2], b[2], acc[n]);
            acc[n] = mfma16(a[3], b[3], acc[n]);
        }
    }
}
#endif

// D (16x16x4 layout: lane l, reg r = row 4 (l >> 4) + r, col l & 15) of one block -> dst rows / cols
template <typename Put>
__device__ __forceinline__ void flush_block(const f32x4& d, int lane, Put put) {
#pragma unroll
    for (int r = 0; r < 4; ++r) put(4 * (lane >> 4) + r, lane & 15, d[r]);
}

// expert of pair slot p (segment starts seg[0..K], routed.hip)
__device__ __forceinline__ int seg_expert(const int64_t* seg, int K, int64_t p) {
    int k = 0;
    while (k + 1 < K && seg[k + 1] <= p) ++k;
    return k;
}

// the 14 weight-gradient blocks of one wave (56 accumulator registers) and its bias partial sums
struct DwAcc {
    f32x4 aWC2[1], aWC1[4], aWC0[2], aHD[1], aW1[4], aW0[2];
    BiasAcc bWC2, bWC1, bWC0, bHD, bW1, bW0;
};

__device__ __forceinline__ void dw_zero(DwAcc& a) {
    a.aWC2[0] = 0.0f; a.aHD[0] = 0.0f;
#pragma unroll
    for (int n = 0; n < 4; ++n) { a.aWC1[n] = 0.0f; a.aW1[n] = 0.0f; }
#pragma unroll
    for (int n = 0; n < 2; ++n) { a.aWC0[n] = 0.0f; a.aW0[n] = 0.0f; }
    a.bWC2 = a.bWC1 = a.bWC0 = a.bHD = a.bW1 = a.bW0 = 0.0f;
}

// one copy of the 13,715 partial sums: every element has exactly one owner (wave, lane, register)
__device__ __forceinline__ void dw_flush(DwAcc& a, float* __restrict__ dst, int w, int lane0) {
    const int cw = 16 * w;
    flush_block(a.aWC2[0], lane0, [&](int o, int c, float v) { if (o < 3) dst[D_WC2 + 64 * o + cw + c] = v; });
    flush_block(a.aHD[0], lane0, [&](int o, int c, float v) {
        dst[o < 15 ? D_WG + 64 * o + cw + c : D_WSH + cw + c] = v;
    });
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        flush_block(a.aWC1[n], lane0, [&](int o, int c, float v) { dst[D_WC1 + 64 * (cw + o) + 16 * n + c] = v; });
        flush_block(a.aW1[n], lane0, [&](int o, int c, float v) { dst[D_W1 + 64 * (cw + o) + 16 * n + c] = v; });
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        flush_block(a.aWC0[n], lane0, [&](int o, int c, float v) {
            if (16 * n + c < 31) dst[D_WC0 + 31 * (cw + o) + 16 * n + c] = v;
        });
        flush_block(a.aW0[n], lane0, [&](int o, int c, float v) { dst[D_W0 + 32 * (cw + o) + 16 * n + c] = v; });
    }
#if ACN_TRAIN_AMP
    // bias rows = column 0 of the ones-row contraction blocks: lanes 0, 16, 32, 48 hold rows 4 (l >> 4) + r
    if ((lane0 & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * (lane0 >> 4) + r;
            if (w == 0) {
                if (i < 3) dst[D_BC2 + i] = a.bWC2[r];
                dst[i < 15 ? D_BG + i : D_BSH] = a.bHD[r];
            }
            dst[D_BC1 + cw + i] = a.bWC1[r];
            dst[D_BC0 + cw + i] = a.bWC0[r];
            dst[D_B1 + cw + i] = a.bW1[r];
            dst[D_B0 + cw + i] = a.bW0[r];
        }
    }
#else
    // bias rows: lane (i, q) holds the sum over samples 32 q .. 32 q + 31 of row i of its row block
    auto red = [](float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); };
    const float bWC2 = red(a.bWC2), bHD = red(a.bHD), bWC1 = red(a.bWC1), bWC0 = red(a.bWC0), bW1 = red(a.bW1),
                bW0 = red(a.bW0);
    if (lane0 < 16) {
        const int i = lane0;
        if (w == 0) {
            if (i < 3) dst[D_BC2 + i] = bWC2;
            dst[i < 15 ? D_BG + i : D_BSH] = bHD;
        }
        dst[D_BC1 + cw + i] = bWC1;
        dst[D_BC0 + cw + i] = bWC0;
        dst[D_B1 + cw + i] = bW1;
        dst[D_B0 + cw + i] = bW0;
    }
#endif
}

// The roles (8-wave workgroups, two waves per SIMD).  Waves 0-3 (producers) each take one 32-sample tile of the
// round: forward recompute, the dX chain, ReLU masks; they put each layer's dY / X into the shared stage, tile w
// in stage columns 32 w .. 32 w + 31.  Waves 4-7 (consumers) hold the weight-gradient accumulators: consumer w
// owns row block 16 w .. 16 w + 15 of the 64-row layers and column block 16 w .. of the two heads, and
// contracts the stage over its 128 samples in a fixed k order (dw_blocks: every k-step takes one sample of each
// lane quarter q out of that quarter's samples 32 q .. 32 q + 31, ascending).  Per layer: producers put ->
// barrier -> [producers: dX of the layer | consumers: dW of the layer] -> barrier, so the MFMA-bound
// contraction overlaps the producers' VALU-bound split / ReLU / dX work instead of following it, and neither
// role carries the other's registers.  The barrier
// that frees the stage for the next round sits at the HEAD of the producers' round (after the forward
// recompute), not at the end of the previous one, so the consumers' last layer (sigma trunk 0) runs beside the
// producers' dL/dh0 and their next forward recompute instead of in front of them.  Every wave executes the same
// 12 barriers per round (the head barrier, one after each of the six puts, one after each of the first five
// layers' dX / dW) and the same rounds.  The sums are deterministic: every element of [dW | db] has one owner
// (wave, lane, register), which adds its rounds in order and each round's samples in the fixed k order above;
// the workgroups' copies are added in index order (mlp_dw_reduce_kernel).  No atomics anywhere.
template <int NO, int NI>
__device__ __forceinline__ void pc_put(float* st, const f32x16 (&dY)[NO], const f32x16 (&X)[NI], int w, int lane) {
    stage_put<NO>(st, 0, dY, w, lane);
    stage_put<NI>(st, X_ROW, X, w, lane);
}

// X0n holds this round's h0 tile (loaded during the previous round) and leaves holding the next round's (sample
// mn, okn); the SH row and the output / output-gradient vectors are issued behind the forward's first layer and
// consumed after its later ones
__device__ __forceinline__ void pc_producer_round(const float* W, float* st, const float* __restrict__ h0,
                                                  const float* __restrict__ sh, const float* __restrict__ out,
                                                  const float* __restrict__ gout, int64_t m, bool ok, int w,
                                                  int lane, float* __restrict__ gh0, X0Raw& X0n, int64_t mn,
                                                  bool okn) {
    const int h = lane >> 5;
    f32x16 A1[2], A2[2], Hd[1], Cin[1], C1[2], C2[2], Rg[1];
    PcIn in;
    tile_forward_x(W, X0n, sh, out, gout, m, ok, lane, in, A1, A2, Hd, Cin, C1, C2, Rg);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 dRg[1], dHd[1];
    dRg[0] = 0.0f;
    float dsig = 0.0f;
    {   // selects, not a branch: a branch would let the compiler sink the prefetched loads into it
        const bool rgb = ok && h == 0, sg = ok && h != 0;
        float gv[3], ov[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gv[c] = opaque_f(in.g[c]);
            ov[c] = opaque_f(in.o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dRg[0][c] = rgb ? grad_rgb(gv[c], ov[c]) : 0.0f;
        dsig = sg ? grad_sigma(gv[0], ov[0]) : 0.0f;
    }
    // colour head
    __syncthreads();   // the consumers have finished the previous round's last layer: stage free
    pc_put<1, 2>(st, dRg, C2, w, lane);
    __syncthreads();
    f32x16 G2[2], G1[2], Gc[1];
    bwd_layer<2, 1, 3, 32>(W + L_WC2, S64, dRg, G2, lane);
    relu_mask<2>(G2, C2);
    __syncthreads();
    // colour layer 1
    pc_put<2, 2>(st, G2, C1, w, lane);
    __syncthreads();
    bwd_layer<2, 2, 64, 64>(W + L_WC1, S64, G2, G1, lane);
    relu_mask<2>(G1, C1);
    __syncthreads();
    // colour layer 0
    pc_put<2, 1>(st, G1, Cin, w, lane);
    __syncthreads();
    bwd_layer<1, 2, 64, 64>(W + L_WC0, S32, G1, Gc, lane);  // d cin: rows 0..14 = d geo (SH rows dropped)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = rho(r, h);
        dHd[0][r] = f < 15 ? Gc[0][r] : (f == 15 ? dsig : 0.0f);
    }
    __syncthreads();
    // heads
    pc_put<1, 2>(st, dHd, A2, w, lane);
    __syncthreads();
    f32x16 GA2[2], GA1[2], GH[1];
    bwd_layer<2, 1, 16, 32>(W + L_WH, S64, dHd, GA2, lane);
    relu_mask<2>(GA2, A2);
    __syncthreads();
    // sigma trunk 1
    pc_put<2, 2>(st, GA2, A1, w, lane);
    __syncthreads();
    f32x16 X0[1];
    X0Raw x0c;
    load_x0raw(h0, m, ok, h, x0c);   // reloaded (L2-hot) for the last layer, issued before this layer's dX
    __builtin_amdgcn_sched_barrier(0);
    bwd_layer<2, 2, 64, 64>(W + L_W1, S64, GA2, GA1, lane);
    relu_mask<2>(GA1, A1);
    __builtin_amdgcn_sched_barrier(0);
    x0_tile(x0c, ok, X0);
    __syncthreads();
    // sigma trunk 0
    pc_put<2, 1>(st, GA1, X0, w, lane);
    __syncthreads();
    load_x0raw(h0, mn, okn, h, X0n);   // the next round's h0 tile, behind dL/dh0 and the consumers' last layer
    __builtin_amdgcn_sched_barrier(0);
    if (gh0) {   // overlaps the consumers' last layer (and the next round's forward recompute follows)
        bwd_layer<1, 2, 64, 64>(W + L_W0, S32, GA1, GH, lane);
        store_tiles<1>(gh0, 32, 0, 32, m, ok, h, GH);
    }
}

// PIPE: the software-pipelined contraction of the fp32 stage (dw_blocks)
template <bool PIPE>
__device__ __forceinline__ void pc_consumer_round(const float* st, int w, int lane, DwAcc& a) {
    __syncthreads();   // stage free (the producers' round-head barrier)
    __syncthreads();
    dw_blocks<1, PIPE>(st, 0, X_ROW + 16 * w, a.aWC2, a.bWC2, lane);
    __syncthreads();
    __syncthreads();
    dw_blocks<4, PIPE>(st, 16 * w, X_ROW, a.aWC1, a.bWC1, lane);
    __syncthreads();
    __syncthreads();
    dw_blocks<2, PIPE>(st, 16 * w, X_ROW, a.aWC0, a.bWC0, lane);
    __syncthreads();
    __syncthreads();
    dw_blocks<1, PIPE>(st, 0, X_ROW + 16 * w, a.aHD, a.bHD, lane);
    __syncthreads();
    __syncthreads();
    dw_blocks<4, PIPE>(st, 16 * w, X_ROW, a.aW1, a.bW1, lane);
    __syncthreads();
    __syncthreads();
    dw_blocks<2, PIPE>(st, 16 * w, X_ROW, a.aW0, a.bW0, lane);
}

__global__ void __launch_bounds__(512) mlp_bwd_dw_pc_kernel(const float* __restrict__ img, const float* __restrict__ h0,
                                                            const float* __restrict__ sh, const float* __restrict__ out,
                                                            const float* __restrict__ gout, int64_t M,
                                                            float* __restrict__ gh0, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    __shared__ __attribute__((aligned(16))) float st_base[ST_FLOATS];
    stage_weights(img, Wl);
    stage_init(st_base);   // the fp16 stage's ones row (bias sums); nothing for the fp32 stage
    __syncthreads();
    const int lane0 = threadIdx.x & 63, j = lane0 & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), w = wv & 3;
    const int64_t ntiles = (M + 31) / 32;
    // rounds are uniform over the workgroup (the same 12 barriers per round in both roles): tiles past the end
    // have zero gradients
    if (wv < 4) {
        const int64_t step = (int64_t)gridDim.x * 4;
        X0Raw X0n;
        {
            const int64_t m0 = ((int64_t)blockIdx.x * 4 + w) * 32 + j;
            load_x0raw(h0, m0, m0 < M, lane0 >> 5, X0n);
        }
        for (int64_t base = (int64_t)blockIdx.x * 4; base < ntiles; base += step) {
            const int64_t m = (base + w) * 32 + j, mn = m + step * 32;
            pc_producer_round(Wl + opaque_s(0), st_base + opaque_s(0), h0, sh, out, gout, m, m < M, w,
                              opaque_v(lane0), gh0, X0n, mn, mn < M);
        }
    } else {
        DwAcc a;
        dw_zero(a);
        for (int64_t base = (int64_t)blockIdx.x * 4; base < ntiles; base += (int64_t)gridDim.x * 4)
            pc_consumer_round<true>(st_base + opaque_s(0), w, opaque_v(lane0), a);
        dw_flush(a, partial + (int64_t)blockIdx.x * NDW, w, lane0);
    }
}

// dw[e] = sum over the nblk partial copies: a block sums 32 consecutive elements, its 8 thread rows
// stride over the copies (128-B coalesced rows), then the rows are added in LDS
__global__ void __launch_bounds__(256) mlp_dw_reduce_kernel(const float* __restrict__ partial, int nblk,
                                                            float* __restrict__ dw) {
    __shared__ float red[8][32];
    const int c = threadIdx.x & 31, row = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + c;
    float s = 0.0f;
    if (e < NDW) {
        // same summation order; unrolled so the loads of 8 copies are in flight together (a dependent
        // load per iteration made this a chain of 32 memory latencies: 11.5 us per call)
#pragma unroll 8
        for (int b = row; b < nblk; b += 8) s += partial[(int64_t)b * NDW + e];
    }
    red[row][c] = s;
    __syncthreads();
    if (row == 0 && e < NDW) {
        float t = red[0][c];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[k][c];
        dw[e] = amp_r(t);  // AMP: the fp16 GEMM output rounding of [dW | db]
    }
}


// ---------------------------------------------------------------------------------------------
// Routed pair lists (routed.hip): slots grouped by expert, every expert's segment padded to a multiple
// of 128 (one round = 4 tiles = 128 slots of ONE expert); the slot count seg[K] lives on the device, so
// grids are fixed and the kernels stride to it (HIP-graph replayable).  A workgroup stages the weight
// image of the expert of its current round and restages when the expert changes.

__global__ void __launch_bounds__(256) mlp_fwd_pairs_kernel(const float* __restrict__ imgs, const float* __restrict__ h0,
                                                            const float* __restrict__ sh,
                                                            const int64_t* __restrict__ seg, int K,
                                                            float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31, w = threadIdx.x >> 6;
    const int64_t rounds = seg[K] / 128;
    int cur = -1;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int k = seg_expert(seg, K, rd * 128);
        if (k != cur) {
            __syncthreads();
            stage_weights(imgs + (int64_t)k * L_FLOATS, Wl);
            __syncthreads();
            cur = k;
        }
        const int64_t m = (rd * 4 + w) * 32 + j;
        f32x16 X0[1], A1[2], A2[2], Hd[1], Cin[1], C1[2], C2[2], Rg[1];
        tile_forward(Wl, h0, sh, m, true, lane, X0, A1, A2, Hd, Cin, C1, C2, Rg);
        if (h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[m * 4 + c] = out_rgb(Rg[0][c]);
        } else {
            out[m * 4 + 3] = out_sigma(Hd[0][7]);
        }
    }
}

// The pair-list backward (the routed container's C5 step): mlp_bwd_dw_pc_kernel's roles, barriers and prefetch
// over a contiguous range of rounds per workgroup.  Workgroup b takes the rounds [b R / G, (b+1) R / G) (R =
// seg[K] / 128 from the device, G workgroups); a round is 128 slots of one expert, and padding slots carry zero
// output gradients.  When the expert of the next round differs, both roles pass two barriers around the
// restaging of that expert's image (the consumers first write their running sums to copy (b, expert) and
// restart), so the barrier sequence stays the same in both roles.  Same owners, same stage layout and same k
// order as the single-expert kernel; mlp_dw_reduce_pairs_kernel adds, per expert, the copies of the workgroups
// whose range met that expert's rounds, in b order: deterministic, no atomics.
__global__ void __launch_bounds__(512) mlp_bwd_dw_pairs_pc_kernel(const float* __restrict__ imgs,
                                                                  const float* __restrict__ h0,
                                                                  const float* __restrict__ sh,
                                                                  const float* __restrict__ out,
                                                                  const float* __restrict__ gout,
                                                                  const int64_t* __restrict__ seg, int K,
                                                                  float* __restrict__ gh0, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    __shared__ __attribute__((aligned(16))) float st_base[ST_FLOATS];
    stage_init(st_base);   // published by the staging barriers of the first round
    const int lane0 = threadIdx.x & 63, j = lane0 & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), w = wv & 3;
    const int64_t R = seg[K] / 128, G = gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * R / G, r1 = ((int64_t)blockIdx.x + 1) * R / G;
    // one pass per run of rounds of one expert: both roles restage that expert's image between two barriers, the
    // consumers zero their sums before the run and write copy (b, expert) after it (no accumulator state
    // crosses a run, so the compiler keeps the sums in place)
    int64_t rd = r0;
    if (wv < 4) {
        X0Raw X0n;
        if (r0 < r1) load_x0raw(h0, (r0 * 4 + w) * 32 + j, true, lane0 >> 5, X0n);
        while (rd < r1) {
            const int k = seg_expert(seg, K, rd * 128);
            __syncthreads();
            stage_weights(imgs + (int64_t)k * L_FLOATS, Wl);
            __syncthreads();
            for (; rd < r1 && seg_expert(seg, K, rd * 128) == k; ++rd) {
                const int64_t m = (rd * 4 + w) * 32 + j, mn = m + 128;
                pc_producer_round(Wl + opaque_s(0), st_base + opaque_s(0), h0, sh, out, gout, m, true, w,
                                  opaque_v(lane0), gh0, X0n, mn, rd + 1 < r1);
            }
        }
    } else {
        while (rd < r1) {
            const int k = seg_expert(seg, K, rd * 128);
            __syncthreads();
            stage_weights(imgs + (int64_t)k * L_FLOATS, Wl);
            __syncthreads();
            DwAcc a;
            dw_zero(a);
            for (; rd < r1 && seg_expert(seg, K, rd * 128) == k; ++rd)
                // the unpipelined contraction: the pipelined one's register allocation here leaves a 6-state
                // WAR-on-C gap under tests/test_hazard_audit.py's margin
                pc_consumer_round<false>(st_base + opaque_s(0), w, opaque_v(lane0), a);
            dw_flush(a, partial + ((int64_t)blockIdx.x * K + k) * NDW, w, lane0);
        }
    }
}

// dw[k][e] = sum over the workgroups b whose round range [b R / G, (b+1) R / G) met expert k's rounds of
// copy (b, k); zero for an expert without pairs.  grid (NDW / 32, K)
__global__ void __launch_bounds__(256) mlp_dw_reduce_pairs_kernel(const float* __restrict__ partial,
                                                                  const int64_t* __restrict__ seg, int K, int G,
                                                                  float* __restrict__ dw) {
    __shared__ float red[8][32];
    const int c = threadIdx.x & 31, row = threadIdx.x >> 5;
    const int k = blockIdx.y;
    const int e = blockIdx.x * 32 + c;
    const int64_t R = seg[K] / 128, k0 = seg[k] / 128, k1 = seg[k + 1] / 128;
    float s = 0.0f;
    if (e < NDW && k1 > k0) {
        // only the workgroups whose round range [b R / G, (b+1) R / G) meets [k0, k1) hold a copy (the
        // ranges are monotone in b: stop past k1); same summation order as before, the loads issued
        // unconditionally (every copy slot is allocated) so 8 copies are in flight together -- a
        // load under the condition made this a chain of memory latencies (40 us per step at K = 8)
        // first b whose range can meet [k0, k1): (b + 1) R / G > k0 needs b >= k0 G / R - 1
        const int64_t bf = R > 0 ? (k0 * G) / R - 1 : 0;
        const int b0 = (int)((bf < 0 ? 0 : bf) & ~(int64_t)7) + row;  // same residue mod 8: same order
#pragma unroll 8
        for (int b = b0; b < G; b += 8) {
            const int64_t lo = (int64_t)b * R / G, hi = ((int64_t)b + 1) * R / G;
            if (lo >= k1) break;
            const float v = partial[((int64_t)b * K + k) * NDW + e];
            if (lo < hi && hi > k0) s += v;
        }
    }
    red[row][c] = s;
    __syncthreads();
    if (row == 0 && e < NDW) {
        float t = red[0][c];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += red[q][c];
        dw[(int64_t)k * NDW + e] = amp_r(t);
    }
}

// ---------------------------------------------------------------------------------------------
// Input gradients with frozen weights (acn_mlp_train_bwd_input): dL/d(hash features) and dL/d(SH features) of
// [sigmoid(color_mlp(cat(geo, sh))), trunc_exp(sigma_head)] (MetaNGP.forward, models/inr/meta_ngp.py:226-241, the
// torch.cat of :207-211 included).  One wave per 32-sample tile re-runs the forward (the tile_forward of
// mlp_fwd_kernel, so the activations are the forward's bit for bit) and then the dX chain of mlp_bwd_kernel /
// pc_producer_round with the ReLU masks taken from the live activations; rows 15..30 of d cin, which those kernels drop,
// are the SH gradient.  Nothing is staged, reduced or saved: after the weight staging there is no barrier, no
// LDS write, no atomic, and every output row depends on its own sample only.
__global__ void __launch_bounds__(256) mlp_bwd_input_kernel(const float* __restrict__ img, const float* __restrict__ h0,
                                                            const float* __restrict__ sh, const float* __restrict__ out,
                                                            const float* __restrict__ gout, int64_t M,
                                                            float* __restrict__ gh0, float* __restrict__ gsh) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    stage_weights(img, Wl);
    __syncthreads();
    const int lane0 = threadIdx.x & 63, j = lane0 & 31;
    const int64_t ntiles = (M + 31) / 32;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
        const int64_t m = tile * 32 + j;
        const bool ok = m < M;
        const float* W = Wl + opaque_s(0);   // as mlp_fwd_kernel: the LDS weight reads stay inside the tile loop
        const int lane = opaque_v(lane0), h = lane >> 5;
        f32x16 A1[2], A2[2], Hd[1], Cin[1], C1[2], C2[2], Rg[1];
        {
            f32x16 X0[1];
            tile_forward(W, h0, sh, m, ok, lane, X0, A1, A2, Hd, Cin, C1, C2, Rg);
        }
        f32x16 dRg[1], dHd[1];
        dRg[0] = 0.0f;
        float dsig = 0.0f;
        if (ok) {
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float y = out[m * 4 + c];
                    dRg[0][c] = grad_rgb(gout[m * 4 + c], y);
                }
            } else {
                dsig = grad_sigma(gout[m * 4 + 3], out[m * 4 + 3]);
            }
        }
        f32x16 G2[2], G1[2], Gc[1];
        bwd_layer<2, 1, 3, 32>(W + L_WC2, S64, dRg, G2, lane);
        relu_mask<2>(G2, C2);
        bwd_layer<2, 2, 64, 64>(W + L_WC1, S64, G2, G1, lane);
        relu_mask<2>(G1, C1);
        bwd_layer<1, 2, 64, 64>(W + L_WC0, S32, G1, Gc, lane);  // d cin: rows 0..14 = d geo, 15..30 = d SH
        if (gsh && ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = rho(r, h);
                if (f >= 15 && f < 31) gsh[m * 16 + (f - 15)] = Gc[0][r];
            }
        }
        if (gh0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = rho(r, h);
                dHd[0][r] = f < 15 ? Gc[0][r] : (f == 15 ? dsig : 0.0f);
            }
            f32x16 GA2[2], GA1[2], GH[1];
            bwd_layer<2, 1, 16, 32>(W + L_WH, S64, dHd, GA2, lane);
            relu_mask<2>(GA2, A2);
            bwd_layer<2, 2, 64, 64>(W + L_W1, S64, GA2, GA1, lane);
            relu_mask<2>(GA1, A1);
            bwd_layer<1, 2, 64, 64>(W + L_W0, S32, GA1, GH, lane);
            store_tiles<1>(gh0, 32, 0, 32, m, ok, h, GH);
        }
    }
}

#if !ACN_TRAIN_AMP
// ---------------------------------------------------------------------------------------------
// Density and its world-space gradient in one launch (acn_field_sigma_grad): sigma = trunc_exp(sigma_head(trunk(
// hash(x01)))) and d sigma / d p of MetaNGP.density for p (M, 3), with nothing but (sigma, grad) written.  One wave
// per 32-sample tile.  Lane (j, h) gathers the eight levels whose features it holds in the MFMA operand layout
// (register pair 2i, 2i + 1 = level 4 (i >> 1) + 2h + (i & 1), features rho(2i, h), rho(2i + 1, h)) straight into X0,
// runs the sigma branch forward and backward on the layers of mlp_bwd_input_kernel (the head's 32 padded rows, so
// the sums are those of the fwd -> bwd_input chain with gout = e_sigma), and contracts the returned dL/dh0 of those
// same eight levels with their corner rows, gathered a second time (level_grad, as hashgrid_bwd_input_f2).  The
// sixteen level terms are added in that kernel's xor-tree order -- pairs inside a lane, then across the two lane halves,
// then quads and octets -- so the result equals the four-launch chain bit for bit.  After the weight staging there is
// no barrier, no LDS write and no atomic; every row depends on its own sample only.
struct SigmaGradArgs {
    const float* x;
    int64_t M, ld;
    const float* table;
    int32_t res[16];
    int32_t log2T;
    float amin[3], ext[3];
    float lo, hi;
    const float* gate;
    float gate_min;
    float* sigma;
    float* grad;
};

// Gathers in flight per lane: the renders' depth (ACN_HASH_DEPTH, render.hip), 3 levels = 24 buffer loads, held by
// scheduling barriers.  Left to itself hipcc issued all 64 loads of a gather pass at once, the ceiling of the 6-bit
// vmcnt counter, and at 1 M points a few tiles per call then returned wrong, run-to-run different gradients in rows
// 16..31 (the shape of 4l's wrong gathers).
constexpr int SG_DEPTH = 3;

// gather step i of the lane's point: level 4 (i >> 1) + 2h + (i & 1) (features rho(2i, h), rho(2i + 1, h))
template <int INTERP>
__device__ __forceinline__ float sg_issue(__amdgpu_buffer_rsrc_t rs, const SigmaGradArgs& a, int i, int h, uint32_t mask,
                                          float x0, float x1, float x2, acn::HashPendingX& p) {
    const int l0 = 4 * (i >> 1) + (i & 1);       // the level of half 0; half 1 holds l0 + 2
    const float r = (float)(h ? a.res[l0 + 2] : a.res[l0]);
    acn::hash_issue_x<INTERP>(rs, (uint32_t)(l0 + 2 * h) << (a.log2T + 3), x0 * r, x1 * r, x2 * r, mask, p);
    return r;
}

constexpr int SG_WAVES = 2;   // waves per SIMD the register budget is held to: two 4-wave blocks (72 KB weight image each) per CU
template <int INTERP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SG_WAVES, SG_WAVES)))
field_sigma_grad_kernel(const float* __restrict__ img, SigmaGradArgs a) {
    __shared__ __attribute__((aligned(16))) float Wl[L_FLOATS];
    stage_weights(img, Wl);
    __syncthreads();
    const int lane0 = threadIdx.x & 63, j = lane0 & 31, h0 = lane0 >> 5;
    const uint32_t mask = (1u << a.log2T) - 1u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.table, (short)0, (int)(16u << (a.log2T + 3)), 0x00020000);
    const int64_t ntiles = (a.M + 31) / 32;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
        const int64_t m = tile * 32 + j;
        const bool ok = m < a.M;
        bool gated = false;
        if (a.gate) {
            gated = ok && a.gate[m] <= a.gate_min;
            if (__ballot(ok && !gated) == 0ull) {   // wave-uniform: nothing live in this tile, no gather
                if (ok && h0 == 0) {
                    a.sigma[m] = 0.0f;
                    a.grad[3 * m] = 0.0f;
                    a.grad[3 * m + 1] = 0.0f;
                    a.grad[3 * m + 2] = 0.0f;
                }
                continue;
            }
        }
        const float* W = Wl + opaque_s(0);   // as mlp_fwd_kernel: the LDS weight reads stay inside the tile loop
        const int lane = opaque_v(lane0), h = lane >> 5;
        // unit coordinates (field_tile's division and clamp); a NaN coordinate stays NaN through clamp_nan, so the
        // sample gathers at the box corner instead and enters the tile as zero features
        const float* px = a.x + (ok ? m : 0) * a.ld;
        const float u0 = (px[0] - a.amin[0]) / a.ext[0], u1 = (px[1] - a.amin[1]) / a.ext[1],
                    u2 = (px[2] - a.amin[2]) / a.ext[2];
        float x0 = acn::clamp_nan(u0, a.lo, a.hi), x1 = acn::clamp_nan(u1, a.lo, a.hi), x2 = acn::clamp_nan(u2, a.lo, a.hi);
        const bool fin = x0 == x0 && x1 == x1 && x2 == x2;
        const bool feed = ok && fin;
        if (!fin) { x0 = a.lo; x1 = a.lo; x2 = a.lo; }
        f32x16 A1[2], A2[2];
        float sig;
        {
            f32x16 X0[1], Hd[1];
            {
                acn::HashPendingX p[SG_DEPTH];
#pragma unroll
                for (int i = 0; i < SG_DEPTH - 1; ++i) sg_issue<INTERP>(rs, a, i, h, mask, x0, x1, x2, p[i]);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (i + SG_DEPTH - 1 < 8)
                        sg_issue<INTERP>(rs, a, i + SG_DEPTH - 1, h, mask, x0, x1, x2, p[(i + SG_DEPTH - 1) % SG_DEPTH]);
                    __builtin_amdgcn_sched_barrier(0);
                    float o0, o1;
                    acn::hash_finish_x<INTERP>(p[i % SG_DEPTH], o0, o1);
                    X0[0][2 * i] = feed ? o0 : 0.0f;
                    X0[0][2 * i + 1] = feed ? o1 : 0.0f;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            fwd_layer<2, 1, 64>(W + L_W0, S32, W + L_B0, X0, A1, lane);
            relu<2>(A1);
            fwd_layer<2, 2, 64>(W + L_W1, S64, W + L_B1, A1, A2, lane);
            relu<2>(A2);
            fwd_layer<1, 2, 32>(W + L_WH, S64, W + L_BH, A2, Hd, lane);
            sig = out_sigma(Hd[0][7]);   // row 15 = sigma head (lane half 1, reg 7)
        }
        // d sigma / d s = sigma (TruncExp's rule, also where s was clamped): the head gradient is e_15 * sigma
        f32x16 dHd[1], GH[1];
        dHd[0] = 0.0f;
        dHd[0][7] = (ok && h == 1) ? grad_sigma(1.0f, sig) : 0.0f;
        {
            f32x16 GA2[2], GA1[2];
            bwd_layer<2, 1, 16, 32>(W + L_WH, S64, dHd, GA2, lane);
            relu_mask<2>(GA2, A2);
            bwd_layer<2, 2, 64, 64>(W + L_W1, S64, GA2, GA1, lane);
            relu_mask<2>(GA1, A1);
            bwd_layer<1, 2, 64, 64>(W + L_W0, S32, GA1, GH, lane);
        }
        // contraction: the lane's eight level terms, pairs first (levels 4q + 2h, 4q + 2h + 1)
        float pxs[4], pys[4], pzs[4];
        {
            acn::HashPendingX p[SG_DEPTH];
            float rr[SG_DEPTH];
            acn::LevelGrad tp{0.0f, 0.0f, 0.0f};
            // the same unit point behind an opaque copy: the pass recomputes its cells, weights and row offsets
            // instead of holding the first pass's (~80 registers) across the layers
            float y0 = x0, y1 = x1, y2 = x2;
            asm volatile("" : "+v"(y0), "+v"(y1), "+v"(y2));
            __builtin_amdgcn_sched_barrier(0);   // the second pass's gathers start here, not above the layers
#pragma unroll
            for (int i = 0; i < SG_DEPTH - 1; ++i) rr[i] = sg_issue<INTERP>(rs, a, i, h, mask, y0, y1, y2, p[i]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i + SG_DEPTH - 1 < 8)
                    rr[(i + SG_DEPTH - 1) % SG_DEPTH] =
                        sg_issue<INTERP>(rs, a, i + SG_DEPTH - 1, h, mask, y0, y1, y2, p[(i + SG_DEPTH - 1) % SG_DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                float2 f[8];
                acn::hash_rows_x(p[i % SG_DEPTH], f);
                const float g0 = GH[0][2 * i], g1 = GH[0][2 * i + 1], r = rr[i % SG_DEPTH];
                float v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = g0 * f[c].x + g1 * f[c].y;
                const float sx = y0 * r, sy = y1 * r, sz = y2 * r;
                const acn::LevelGrad t = acn::level_grad<INTERP>(v, sx - floorf(sx), sy - floorf(sy), sz - floorf(sz), r);
                if (i & 1) {
                    pxs[i >> 1] = tp.x + t.x;
                    pys[i >> 1] = tp.y + t.y;
                    pzs[i >> 1] = tp.z + t.z;
                } else {
                    tp = t;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ... then the other lane half's pair (levels 4q .. 4q + 3), the quads and the octets: hashgrid_bwd_input_f2's tree
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pxs[q] += __shfl_xor(pxs[q], 32);
            pys[q] += __shfl_xor(pys[q], 32);
            pzs[q] += __shfl_xor(pzs[q], 32);
        }
        const float gx = (pxs[0] + pxs[1]) + (pxs[2] + pxs[3]);
        const float gy = (pys[0] + pys[1]) + (pys[2] + pys[3]);
        const float gz = (pzs[0] + pzs[1]) + (pzs[2] + pzs[3]);
        const float sg = __shfl_xor(sig, 32);   // half 0 writes; sigma lives in half 1
        if (ok && h == 0) {
            // torch's clamp backward passes the gradient where the unclamped value lies in [lo, hi]
            const float k0 = (u0 >= a.lo && u0 <= a.hi) ? 1.0f / a.ext[0] : 0.0f;
            const float k1 = (u1 >= a.lo && u1 <= a.hi) ? 1.0f / a.ext[1] : 0.0f;
            const float k2 = (u2 >= a.lo && u2 <= a.hi) ? 1.0f / a.ext[2] : 0.0f;
            const float nanv = __builtin_nanf("");
            a.sigma[m] = gated ? 0.0f : (fin ? sg : nanv);
            a.grad[3 * m] = gated ? 0.0f : (fin ? k0 * gx : nanv);
            a.grad[3 * m + 1] = gated ? 0.0f : (fin ? k1 * gy : nanv);
            a.grad[3 * m + 2] = gated ? 0.0f : (fin ? k2 * gz : nanv);
        }
    }
}
#endif

MlpPtrs ptrs(const acn_mlp* w) {
    return MlpPtrs{w->w0, w->b0, w->w1, w->b1, w->wsh, w->bsh, w->wg, w->bg,
                   w->wc0, w->bc0, w->wc1, w->bc1, w->wc2, w->bc2};
}

unsigned grid_for(int64_t M) {  // 4 waves per block, grid-stride over 32-sample tiles, ~2 blocks per CU
    const int64_t tiles = (M + 31) / 32, blocks = (tiles + 3) / 4;
    return (unsigned)(blocks < 512 ? (blocks < 1 ? 1 : blocks) : 512);
}

}  // namespace

extern "C" size_t ACN_MLP_API(acn_mlp_workspace_bytes)(void) { return (size_t)L_FLOATS * sizeof(float); }

extern "C" int ACN_MLP_API(acn_mlp_train_fwd)(const float* h0, const float* sh, int64_t M, const acn_mlp* w, float* out,
                                 float* save, void* workspace, void* stream) {
    ACN_REQUIRE(M >= 0 && w && workspace, "acn_mlp_train_fwd: bad arguments");
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(h0 && sh && out, "acn_mlp_train_fwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((L_FLOATS + 255) / 256), dim3(256), 0, s, ptrs(w), (float*)workspace);
    if (save)
        hipLaunchKernelGGL(mlp_fwd_kernel<true>, dim3(grid_for(M)), dim3(256), 0, s, (const float*)workspace, h0, sh, M,
                           out, save);
    else {
        const int64_t blocks = ((M + 31) / 32 + 7) / 8;
        hipLaunchKernelGGL(mlp_fwd_kernel<false>, dim3((unsigned)(blocks < 512 ? blocks : 512)), dim3(512), 0, s,
                           (const float*)workspace, h0, sh, M, out, save);
    }
    return acn_check_launch("acn_mlp_train_fwd");
}

extern "C" int ACN_MLP_API(acn_mlp_train_bwd)(const float* save, const float* out, const float* gout, int64_t M, const acn_mlp* w,
                                 float* gsave, float* gh0, void* workspace, void* stream) {
    ACN_REQUIRE(M >= 0 && w && workspace, "acn_mlp_train_bwd: bad arguments");
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(save && out && gout && gsave, "acn_mlp_train_bwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((L_FLOATS + 255) / 256), dim3(256), 0, s, ptrs(w), (float*)workspace);
    hipLaunchKernelGGL(mlp_bwd_kernel, dim3(grid_for(M)), dim3(256), 0, s, (const float*)workspace, save, out, gout,
                       M, gsave, gh0);
    return acn_check_launch("acn_mlp_train_bwd");
}

extern "C" size_t ACN_MLP_API(acn_mlp_dw_workspace_bytes)(void) {
    return ((size_t)L_FLOATS + (size_t)MAX_DW_BLOCKS * NDW) * sizeof(float);
}

namespace {
// the fused backward + the copy reduction, on a packed weight image
int bwd_dw_launch(const float* h0, const float* sh, const float* out, const float* gout, int64_t M, const float* img,
                  float* dw, float* gh0, float* partial, hipStream_t s) {
    const int64_t tiles = (M + 31) / 32, want = (tiles + 3) / 4;
    const int nblk = (int)(want < MAX_DW_BLOCKS ? want : MAX_DW_BLOCKS);
    hipLaunchKernelGGL(mlp_bwd_dw_pc_kernel, dim3(nblk), dim3(512), 0, s, img, h0, sh, out, gout, M, gh0, partial);
    hipLaunchKernelGGL(mlp_dw_reduce_kernel, dim3((NDW + 31) / 32), dim3(256), 0, s, (const float*)partial, nblk,
                       dw);
    return acn_check_launch("acn_mlp_train_bwd_dw");
}
}  // namespace

extern "C" int ACN_MLP_API(acn_mlp_train_bwd_dw)(const float* h0, const float* sh, const float* out, const float* gout, int64_t M,
                                    const acn_mlp* w, float* dw, float* gh0, void* workspace, void* stream) {
    ACN_REQUIRE(M >= 0 && w && workspace && dw, "acn_mlp_train_bwd_dw: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        const hipError_t e = hipMemsetAsync(dw, 0, (size_t)NDW * sizeof(float), s);
        return e == hipSuccess ? ACN_OK : acn_set_error((int)e, "acn_mlp_train_bwd_dw: memset failed");
    }
    ACN_REQUIRE(h0 && sh && out && gout, "acn_mlp_train_bwd_dw: NULL pointer");
    float* img = (float*)workspace;
    float* partial = img + L_FLOATS;  // L_FLOATS is a multiple of 4: 16-B aligned
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((L_FLOATS + 255) / 256), dim3(256), 0, s, ptrs(w), img);
    return bwd_dw_launch(h0, sh, out, gout, M, img, dw, gh0, partial, s);
}

// the same backward on the image acn_mlp_train_fwd packed into ITS workspace for the same weights (one
// pack per forward + backward pair instead of two); workspace: acn_mlp_dw_workspace_bytes() as above
extern "C" int ACN_MLP_API(acn_mlp_train_bwd_dw_img)(const float* h0, const float* sh, const float* out, const float* gout,
                                        int64_t M, const float* img, float* dw, float* gh0, void* workspace,
                                        void* stream) {
    ACN_REQUIRE(M >= 0 && img && workspace && dw, "acn_mlp_train_bwd_dw_img: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        const hipError_t e = hipMemsetAsync(dw, 0, (size_t)NDW * sizeof(float), s);
        return e == hipSuccess ? ACN_OK : acn_set_error((int)e, "acn_mlp_train_bwd_dw_img: memset failed");
    }
    ACN_REQUIRE(h0 && sh && out && gout, "acn_mlp_train_bwd_dw_img: NULL pointer");
    return bwd_dw_launch(h0, sh, out, gout, M, img, dw, gh0, (float*)workspace + L_FLOATS, s);
}

// input gradients with frozen weights (mlp_bwd_input_kernel); workspace: acn_mlp_workspace_bytes(), the packed image
extern "C" int ACN_MLP_API(acn_mlp_train_bwd_input)(const float* h0, const float* sh, const float* out, const float* gout,
                                       int64_t M, const acn_mlp* w, float* gh0, float* gsh, void* workspace,
                                       void* stream) {
    ACN_REQUIRE(M >= 0 && w && workspace, "acn_mlp_train_bwd_input: bad arguments");
    if (M == 0 || (!gh0 && !gsh)) return ACN_OK;
    ACN_REQUIRE(h0 && sh && out && gout, "acn_mlp_train_bwd_input: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((L_FLOATS + 255) / 256), dim3(256), 0, s, ptrs(w), (float*)workspace);
    hipLaunchKernelGGL(mlp_bwd_input_kernel, dim3(grid_for(M)), dim3(256), 0, s, (const float*)workspace, h0, sh, out,
                       gout, M, gh0, gsh);
    return acn_check_launch("acn_mlp_train_bwd_input");
}

// the same on the image acn_mlp_train_fwd packed into its workspace for the same weights (no pack, no workspace)
extern "C" int ACN_MLP_API(acn_mlp_train_bwd_input_img)(const float* h0, const float* sh, const float* out,
                                           const float* gout, int64_t M, const float* img, float* gh0, float* gsh,
                                           void* stream) {
    ACN_REQUIRE(M >= 0 && img, "acn_mlp_train_bwd_input_img: bad arguments");
    if (M == 0 || (!gh0 && !gsh)) return ACN_OK;
    ACN_REQUIRE(h0 && sh && out && gout, "acn_mlp_train_bwd_input_img: NULL pointer");
    hipLaunchKernelGGL(mlp_bwd_input_kernel, dim3(grid_for(M)), dim3(256), 0, (hipStream_t)stream, img, h0, sh, out,
                       gout, M, gh0, gsh);
    return acn_check_launch("acn_mlp_train_bwd_input_img");
}

#if !ACN_TRAIN_AMP
// density + world-space density gradient in one launch (field_sigma_grad_kernel); workspace: acn_mlp_workspace_bytes()
extern "C" int ACN_MLP_API(acn_field_sigma_grad)(const float* x, int64_t M, int64_t ld, const float* table,
                                                 const int32_t* res, int L, int log2T, int F, int interp,
                                                 const float* aabb_min, const float* aabb_extent, float lo, float hi,
                                                 const acn_mlp* w, const float* gate, float gate_min, float* sigma,
                                                 float* grad, void* workspace, void* stream) {
    ACN_REQUIRE(M >= 0 && ld >= 3, "acn_field_sigma_grad: M must be >= 0 and ld >= 3 (got %lld, %lld)", (long long)M,
                (long long)ld);
    ACN_REQUIRE(interp >= 0 && interp <= 2, "acn_field_sigma_grad: bad interpolation %d", interp);
    if (interp == 0)
        return acn_set_error(ACN_ERR_UNSUPPORTED, "acn_field_sigma_grad: Nearest interpolation has no point gradient "
                                                  "(Linear or Smoothstep)");
    if (F != 2 || L != 16)
        return acn_set_error(ACN_ERR_UNSUPPORTED, "acn_field_sigma_grad: the fused kernel implements 16*2 hash "
                                                  "features (L = 16, F = 2), got L = %d, F = %d", L, F);
    ACN_REQUIRE(log2T >= 1, "acn_field_sigma_grad: log2_hashmap_size must be >= 1, got %d", log2T);
    if (log2T > 24)
        return acn_set_error(ACN_ERR_UNSUPPORTED, "acn_field_sigma_grad: a table of log2_hashmap_size %d exceeds 2 GiB "
                                                  "(32-bit gather offsets)", log2T);
    ACN_REQUIRE(res && aabb_min && aabb_extent && w && workspace, "acn_field_sigma_grad: NULL argument");
    if (M == 0) return ACN_OK;
    ACN_REQUIRE(x && table && sigma && grad, "acn_field_sigma_grad: NULL pointer");
    SigmaGradArgs a{};
    a.x = x; a.M = M; a.ld = ld; a.table = table; a.log2T = log2T;
    for (int l = 0; l < 16; ++l) a.res[l] = res[l];
    for (int c = 0; c < 3; ++c) { a.amin[c] = aabb_min[c]; a.ext[c] = aabb_extent[c]; }
    a.lo = lo; a.hi = hi; a.gate = gate; a.gate_min = gate_min; a.sigma = sigma; a.grad = grad;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((L_FLOATS + 255) / 256), dim3(256), 0, s, ptrs(w), (float*)workspace);
    if (interp == 1)
        hipLaunchKernelGGL(field_sigma_grad_kernel<1>, dim3(grid_for(M)), dim3(256), 0, s, (const float*)workspace, a);
    else
        hipLaunchKernelGGL(field_sigma_grad_kernel<2>, dim3(grid_for(M)), dim3(256), 0, s, (const float*)workspace, a);
    return acn_check_launch("acn_field_sigma_grad");
}
#endif

// ---------------------------------------------------------------------------------------------
// routed pair lists
constexpr int PAIR_DW_BLOCKS = 256;

extern "C" size_t ACN_MLP_API(acn_mlp_pairs_workspace_bytes)(int K) {
    return ((size_t)K * L_FLOATS + (size_t)PAIR_DW_BLOCKS * K * NDW) * sizeof(float);
}

extern "C" int ACN_MLP_API(acn_mlp_pack_pairs)(const acn_mlp* const* w, int K, void* workspace, void* stream) {
    ACN_REQUIRE(w && workspace && K >= 1 && K <= acn::kMaxK, "acn_mlp_pack_pairs: bad arguments");
    MlpPtrsK pk{};
    for (int k = 0; k < K; ++k) {
        ACN_REQUIRE(w[k], "acn_mlp_pack_pairs: NULL expert %d", k);
        pk.e[k] = ptrs(w[k]);
    }
    hipLaunchKernelGGL(mlp_pack_multi_kernel, dim3((L_FLOATS + 255) / 256, K), dim3(256), 0, (hipStream_t)stream, pk,
                       (float*)workspace);
    return acn_check_launch("acn_mlp_pack_pairs");
}

extern "C" int ACN_MLP_API(acn_mlp_train_fwd_pairs)(const float* h0, const float* sh, const int64_t* seg, int K,
                                       const void* workspace, float* out, void* stream) {
    ACN_REQUIRE(h0 && sh && seg && workspace && out && K >= 1 && K <= acn::kMaxK,
                "acn_mlp_train_fwd_pairs: bad arguments");
    hipLaunchKernelGGL(mlp_fwd_pairs_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, h0,
                       sh, seg, K, out);
    return acn_check_launch("acn_mlp_train_fwd_pairs");
}

extern "C" int ACN_MLP_API(acn_mlp_train_bwd_dw_pairs)(const float* h0, const float* sh, const float* out, const float* gout,
                                          const int64_t* seg, int K, void* workspace, float* dw, float* gh0,
                                          void* stream) {
    ACN_REQUIRE(h0 && sh && out && gout && seg && workspace && dw && K >= 1 && K <= acn::kMaxK,
                "acn_mlp_train_bwd_dw_pairs: bad arguments");
    const float* imgs = (const float*)workspace;
    float* partial = (float*)workspace + (size_t)K * L_FLOATS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_bwd_dw_pairs_pc_kernel, dim3(PAIR_DW_BLOCKS), dim3(512), 0, s, imgs, h0, sh, out, gout, seg, K,
                       gh0, partial);
    hipLaunchKernelGGL(mlp_dw_reduce_pairs_kernel, dim3((NDW + 31) / 32, K), dim3(256), 0, s, (const float*)partial,
                       seg, K, PAIR_DW_BLOCKS, dw);
    return acn_check_launch("acn_mlp_train_bwd_dw_pairs");
}
