// The core of Parakeet's (FastConformer) convolution module (transformers modeling_parakeet.py, ParakeetEncoderConvolutionModule.forward):
//     glu -> depthwise_conv (KW taps, zero SAME padding, optional bias) -> BatchNorm1d in eval mode (running statistics) -> activation
// between the two pointwise convolutions (GEMMs).  KW = 9 (Parakeet) or 32 (LASR / MedASR), C in {256, 512, 768, 1024}, channels-last, fp32.
// An even KW pads as torch's padding="same" does: HL = (KW - 1) / 2 frames on the left, HR = KW - 1 - HL on the right (15 | 16 at 32 taps);
// the data gradient's halo is the mirror image (HR left, HL right).  The two are separate compile-time quantities in every kernel below.
//
//   dyn_convmod_bn_fwd       u [B, T, 2C] -> s [B, T, C] = act((conv - mean_c) * rsqrt(var_c + eps) * weight_c + bias_c),
//                            conv[b, t, c] = cbias_c + sum_j w[c, j] * GLU(u)[b, t - HL + j, c], in ONE launch.
//     Thread = channel.  A thread loads its channel's TT + KW - 1 GLU values ONCE into registers
//     (statically indexed) and forms its TT outputs from them.  BatchNorm with fixed statistics is per channel: no row reduction, so no
//     LDS stage and no barrier.  A GLU value is computed (TT + KW - 1) / TT = 1.5 times at 9 taps (TT = 16), 1.97 times at 32 taps
//     (TT = 32: a 63-float window, 116 VGPRs, 4 waves per SIMD, no scratch).  The other tiling tried at 32 taps, the tile's GLU rows formed
//     once into LDS (63 KB, 2 waves per SIMD) and a thread sliding over its column, gave equal bits and was 16 % / 38 % slower at
//     [5, 509, 512] / [5, 2048, 512] (the LASR section): not kept.
//   dyn_convmod_bn_bwd_act   dc = ds * act'(bn) * weight * rstd and the three column sums (dweight, dbias, dcbias) as per-workgroup
//                            partial rows, rows visited in a fixed order, combined by the fixed-order reducer (reduce.h; deferrable).
//   dyn_glu_dwconv1d_dgrad   du = GLU'(u) * sum_j w[c, j] * dc[t + HL - j]: the register window of the forward over dc (it starts HR frames
//                            to the left), the GLU backward applied to the sum before it is stored; no dgl tensor exists.
// `valid` (device int32 scalar, may be null): GLU rows t >= *valid read as zeros (what SAME padding holds there in the unpadded run) and
// rows >= *valid of every output are exact zeros / left out of the sums.  No float atomics: every result is bit-reproducible.
// The `_lens` entries take one count per batch entry (lens [B], a ragged batch): the same kernels read valid[b * vstride], vstride 0 for
// the scalar entries and 1 for these (transformers' masked_fill in front of the depthwise conv, with the outputs past a row's length zeroed).
#include "common.h"
#include "dwconv_window.h"
#include "reduce.h"

namespace {

constexpr int KW9 = 9, KW32 = 32;
constexpr int TT9 = 16;       // frames per workgroup of the 9-tap forward and dgrad
constexpr int TT32 = 32;      // ... of the 32-tap ones
constexpr int ACT_SILU = 0;

using dyn::silu_f;
using dyn::silu_grad;

// grid (ceil(T / TT), C / 256, B); 256 threads, thread = channel.
template <int KW, int TT>
__global__ __launch_bounds__(256) void convmod_bn_fwd_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                              const float* __restrict__ cbias, const float* __restrict__ mean,
                                                              const float* __restrict__ var, const float* __restrict__ weight,
                                                              const float* __restrict__ bias, float* __restrict__ s,
                                                              float* __restrict__ gl_out, float* __restrict__ c_out,
                                                              const int32_t* __restrict__ valid, int vstride, int64_t T, int C,
                                                              float eps) {
    constexpr int HL = (KW - 1) / 2, HR = KW - 1 - HL, NG = TT + HL + HR;      // frames read left / right of the tile
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t b = blockIdx.z, t0 = (int64_t)blockIdx.x * TT;
    const int64_t vr = dyn::valid_rows(valid, b * vstride, T);
    float wk[KW], g[NG];
    const float cb = dyn::load_glu_window(w, cbias, u + b * T * 2 * C + c, c, C, t0 - HL, vr, wk, g);
    const float mu = mean[c], rs = rsqrtf(var[c] + eps), gw = weight[c], sh = bias[c];
#pragma unroll
    for (int k = 0; k < TT; ++k) {
        const int64_t t = t0 + k;
        if (t >= T) break;
        const int64_t o = (b * T + t) * C + c;
        float cv = 0.f, sv = 0.f;
        if (t < vr) {
            cv = cb;
#pragma unroll
            for (int j = 0; j < KW; ++j) cv += wk[j] * g[k + j];
            sv = silu_f((cv - mu) * rs * gw + sh);
        }
        s[o] = sv;
        if (gl_out) gl_out[o] = g[k + HL];              // rows >= valid hold zeros in the window already
        if (c_out) c_out[o] = cv;
    }
}

// grid (nb, C / 256); thread = channel; workgroup x takes rows x, x + nb, ... of the B * T rows in that order.
__global__ __launch_bounds__(256) void convmod_bn_bwd_act_kernel(const float* __restrict__ c_in, const float* __restrict__ mean,
                                                                  const float* __restrict__ var, const float* __restrict__ weight,
                                                                  const float* __restrict__ bias, const float* ds, float* dc,
                                                                  float* __restrict__ pw, float* __restrict__ pb,
                                                                  float* __restrict__ pc, const int32_t* __restrict__ valid, int vstride,
                                                                  int64_t rows, int64_t T, int C, float eps) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t vr0 = dyn::valid_rows(valid, T);
    const float mu = mean[c], rs = rsqrtf(var[c] + eps), gw = weight[c], sh = bias[c];
    float aw = 0.f, ab = 0.f, ac = 0.f;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        float o = 0.f;
        const int64_t b = r / T;                                   // the quotient of the division r % T needs anyway
        const int64_t vr = vstride ? dyn::valid_rows(valid, b, T) : vr0;
        if (r - b * T < vr) {
            const float xh = (c_in[r * C + c] - mu) * rs;
            const float da = ds[r * C + c] * silu_grad(xh * gw + sh);
            o = da * gw * rs;
            aw += da * xh;
            ab += da;
            ac += o;
        }
        dc[r * C + c] = o;
    }
    const int64_t p = (int64_t)blockIdx.x * C + c;
    if (pw) pw[p] = aw;
    if (pb) pb[p] = ab;
    if (pc) pc[p] = ac;
}

// grid (ceil(T / TT), C / 256, B); 256 threads, thread = channel.
template <int KW, int TT>
__global__ __launch_bounds__(256) void glu_dwconv1d_dgrad_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                                  const float* __restrict__ dc, float* __restrict__ du,
                                                                  const int32_t* __restrict__ valid, int vstride, int64_t T, int C) {
    constexpr int HL = (KW - 1) / 2, HR = KW - 1 - HL;      // the forward's halos
    constexpr int DL = HR, DR = HL, NG = TT + DL + DR;      // the data gradient's: dc[t + HL - j], j = 0 .. KW - 1, reaches HR back and HL ahead
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t b = blockIdx.z, t0 = (int64_t)blockIdx.x * TT;
    const int64_t vr = dyn::valid_rows(valid, b * vstride, T);
    float wk[KW], g[NG];
#pragma unroll
    for (int j = 0; j < KW; ++j) wk[j] = w[(int64_t)c * KW + (KW - 1 - j)];      // flipped: dgl[t] = sum_i wk[i] * dc[t - DL + i]
    const float* gb = dc + b * T * C + c;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int64_t t = t0 - DL + i;
        g[i] = (t >= 0 && t < T) ? gb[t * C] : 0.f;
    }
    const float* ub = u + b * T * 2 * C + c;
    float* ob = du + b * T * 2 * C + c;
#pragma unroll
    for (int k = 0; k < TT; ++k) {
        const int64_t t = t0 + k;
        if (t >= T) break;
        float da = 0.f, db = 0.f;
        if (t < vr) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < KW; ++i) acc += wk[i] * g[k + i];
            const float a = ub[t * 2 * C], sg = dyn::sigmoidf_(ub[t * 2 * C + C]);
            da = acc * sg;
            db = acc * a * sg * (1.f - sg);
        }
        ob[t * 2 * C] = da;
        ob[t * 2 * C + C] = db;
    }
}

inline int bwd_blocks(int64_t rows) { return (int)(rows < 1 ? 1 : rows > 512 ? 512 : rows); }

int check_dims(const char* who, int64_t B, int64_t T, int64_t C, int64_t KW) {
    if (int rc = dyn::check_convmod_dims(who, B, T, C)) return rc;
    DYN_REQUIRE(KW == KW9 || KW == KW32, DYN_E_UNSUPPORTED, "%s: kernel width %lld is not built (9, 32)", who, (long long)KW);
    return DYN_OK;
}

}  // namespace

extern "C" int64_t dyn_convmod_bn_time_tile(void) { return TT9; }

extern "C" int64_t dyn_convmod_bn_time_tile_kw(int64_t KW) { return KW == KW9 ? TT9 : KW == KW32 ? TT32 : 0; }

// `vstride`: 0 = `valid` is one count for the batch (or null), 1 = one count per batch entry.
static int convmod_bn_fwd_impl(const char* who, const float* u, const float* w, const float* cbias, const float* mean, const float* var,
                               const float* weight, const float* bias, float* s, float* gl, float* c, const int32_t* valid, int vstride,
                               int64_t B, int64_t T, int64_t C, int64_t KW, int32_t act, float eps, void* stream) {
    DYN_REQUIRE(u && w && mean && var && weight && bias && s && (valid || !vstride), DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, T, C, KW)) return rc;
    DYN_REQUIRE(act == ACT_SILU, DYN_E_UNSUPPORTED, "%s: act=%d is not built (0 SiLU)", who, (int)act);
    if (B == 0 || T == 0) return DYN_OK;
    const dim3 grid((unsigned)dyn::cdiv(T, KW == KW9 ? TT9 : TT32), (unsigned)(C / 256), (unsigned)B);
#define GO(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, (hipStream_t)stream, u, w, cbias, mean, var, weight, bias, s, gl, c, valid, vstride, T, (int)C, eps)
    if (KW == KW9) GO((convmod_bn_fwd_kernel<KW9, TT9>));
    else GO((convmod_bn_fwd_kernel<KW32, TT32>));
#undef GO
    return dyn::check_launch(who);
}

extern "C" int dyn_convmod_bn_fwd(const float* u, const float* w, const float* cbias, const float* mean, const float* var, const float* weight,
                                  const float* bias, float* s, float* gl, float* c, const int32_t* valid, int64_t B, int64_t T, int64_t C,
                                  int64_t KW, int32_t act, float eps, void* stream) {
    return convmod_bn_fwd_impl("dyn_convmod_bn_fwd", u, w, cbias, mean, var, weight, bias, s, gl, c, valid, 0, B, T, C, KW, act, eps, stream);
}

extern "C" int dyn_convmod_bn_fwd_lens(const float* u, const float* w, const float* cbias, const float* mean, const float* var,
                                       const float* weight, const float* bias, float* s, float* gl, float* c, const int32_t* lens, int64_t B,
                                       int64_t T, int64_t C, int64_t KW, int32_t act, float eps, void* stream) {
    return convmod_bn_fwd_impl("dyn_convmod_bn_fwd_lens", u, w, cbias, mean, var, weight, bias, s, gl, c, lens, 1, B, T, C, KW, act, eps, stream);
}

extern "C" int64_t dyn_convmod_bn_bwd_act_workspace_bytes(int64_t B, int64_t T, int64_t C) {
    return (int64_t)3 * bwd_blocks(B * T) * C * (int64_t)sizeof(float);
}

static int convmod_bn_bwd_act_impl(const char* who, const float* c, const float* mean, const float* var, const float* weight,
                                   const float* bias, const float* ds, float* dc, float* dweight, float* dbias, float* dcbias,
                                   float wgrad_beta, const int32_t* valid, int vstride, int64_t B, int64_t T, int64_t C, int32_t act,
                                   float eps, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(c && mean && var && weight && bias && ds && dc && (valid || !vstride), DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, T, C, KW9)) return rc;
    DYN_REQUIRE(act == ACT_SILU, DYN_E_UNSUPPORTED, "%s: act=%d is not built (0 SiLU)", who, (int)act);
    const int64_t bytes = dyn_convmod_bn_bwd_act_workspace_bytes(B, T, C);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "%s: workspace too small (%lld bytes needed)", who, (long long)bytes);
    if (B == 0 || T == 0) return DYN_OK;
    const int64_t rows = B * T;
    const int nb = bwd_blocks(rows);
    hipStream_t st = (hipStream_t)stream;
    float* pw = dyn::partials_alloc(workspace, bytes);
    float* pb = pw + (int64_t)nb * C;
    float* pc = pb + (int64_t)nb * C;
    hipLaunchKernelGGL(convmod_bn_bwd_act_kernel, dim3((unsigned)nb, (unsigned)(C / 256)), dim3(256), 0, st, c, mean, var, weight, bias, ds, dc,
                       dweight ? pw : nullptr, dbias ? pb : nullptr, dcbias ? pc : nullptr, valid, vstride, rows, T, (int)C, eps);
    if (dweight && dbias) dyn::reduce_pair_or_defer(pw, dweight, pb, dbias, (int64_t)nb, C, wgrad_beta, st);
    else {
        if (dweight) dyn::reduce_or_defer(pw, dweight, (int64_t)nb, C, wgrad_beta, st);
        if (dbias) dyn::reduce_or_defer(pb, dbias, (int64_t)nb, C, wgrad_beta, st);
    }
    if (dcbias) dyn::reduce_or_defer(pc, dcbias, (int64_t)nb, C, wgrad_beta, st);
    return dyn::check_launch(who);
}

extern "C" int dyn_convmod_bn_bwd_act(const float* c, const float* mean, const float* var, const float* weight, const float* bias,
                                      const float* ds, float* dc, float* dweight, float* dbias, float* dcbias, float wgrad_beta,
                                      const int32_t* valid, int64_t B, int64_t T, int64_t C, int32_t act, float eps, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    return convmod_bn_bwd_act_impl("dyn_convmod_bn_bwd_act", c, mean, var, weight, bias, ds, dc, dweight, dbias, dcbias, wgrad_beta, valid, 0, B,
                                   T, C, act, eps, workspace, workspace_bytes, stream);
}

extern "C" int dyn_convmod_bn_bwd_act_lens(const float* c, const float* mean, const float* var, const float* weight, const float* bias,
                                           const float* ds, float* dc, float* dweight, float* dbias, float* dcbias, float wgrad_beta,
                                           const int32_t* lens, int64_t B, int64_t T, int64_t C, int32_t act, float eps, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    return convmod_bn_bwd_act_impl("dyn_convmod_bn_bwd_act_lens", c, mean, var, weight, bias, ds, dc, dweight, dbias, dcbias, wgrad_beta, lens, 1,
                                   B, T, C, act, eps, workspace, workspace_bytes, stream);
}

static int glu_dwconv1d_dgrad_impl(const char* who, const float* u, const float* w, const float* dc, float* du, const int32_t* valid,
                                   int vstride, int64_t B, int64_t T, int64_t C, int64_t KW, void* stream) {
    DYN_REQUIRE(u && w && dc && du && (valid || !vstride), DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, T, C, KW)) return rc;
    DYN_REQUIRE(du != u && du != dc, DYN_E_ARG, "%s: du must not alias u or dc", who);
    if (B == 0 || T == 0) return DYN_OK;
    const dim3 grid((unsigned)dyn::cdiv(T, KW == KW9 ? TT9 : TT32), (unsigned)(C / 256), (unsigned)B);
#define GO(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, (hipStream_t)stream, u, w, dc, du, valid, vstride, T, (int)C)
    if (KW == KW9) GO((glu_dwconv1d_dgrad_kernel<KW9, TT9>));
    else GO((glu_dwconv1d_dgrad_kernel<KW32, TT32>));
#undef GO
    return dyn::check_launch(who);
}

extern "C" int dyn_glu_dwconv1d_dgrad(const float* u, const float* w, const float* dc, float* du, const int32_t* valid, int64_t B, int64_t T,
                                      int64_t C, int64_t KW, void* stream) {
    return glu_dwconv1d_dgrad_impl("dyn_glu_dwconv1d_dgrad", u, w, dc, du, valid, 0, B, T, C, KW, stream);
}

extern "C" int dyn_glu_dwconv1d_dgrad_lens(const float* u, const float* w, const float* dc, float* du, const int32_t* lens, int64_t B,
                                           int64_t T, int64_t C, int64_t KW, void* stream) {
    return glu_dwconv1d_dgrad_impl("dyn_glu_dwconv1d_dgrad_lens", u, w, dc, du, lens, 1, B, T, C, KW, stream);
}
