// The core of a conformer convolution module whose depthwise convolution is CAUSAL, between the two pointwise convolutions (GEMMs):
//     glu -> F.pad(x, (kernel_size - 1, 0)) -> depthwise_conv (optional bias) -> LayerNorm over channels -> activation
// Frame t sees the GLU rows t - (KW - 1) .. t, zeros left of frame 0, nothing to its right.  C in {256, 512, 768, 1024}, channels-last.
// Two entry sets over one set of kernels:
//   dyn_convmod_causal_*      KW = 31, no depthwise bias, SiLU or erf GELU, 8 or 16 frames per workgroup: Wav2Vec2-BERT (transformers
//                             modeling_wav2vec2_bert.py, Wav2Vec2BertConvolutionModule.forward);
//   dyn_convmod_causal_k9_*   KW = 9, depthwise bias `cbias` (may be null), SiLU, 8 frames per workgroup (32 KB of LDS at C = 1024, 16 GLU
//                             values per thread): NemotronAsrStreamingForRNNT (transformers modeling_nemotron_asr_streaming.py,
//                             NemotronAsrStreamingEncoderConvolutionModule.forward).  The bias gradient is the column sum of dy (dyn_colsum).
//
//   dyn_convmod_causal[_k9]_fwd   u [B, T, 2C] -> s [B, T, C] = act(LN_C(cbias[c] + sum_j w[c, j] * GLU(u)[t - (KW - 1) + j, c])) in ONE launch.
//     One workgroup of C threads per (sample, tile of TT frames), thread = channel.  A thread loads its channel's TT + KW - 1 GLU values
//     ONCE into registers (dwconv_window.h: statically indexed, no window shifting) and forms its TT convolution outputs from them; they
//     go to LDS [TT][C]; after one barrier the workgroup's waves take the tile's frames in turn, each holding a whole frame as float4s
//     (layernorm_row.h: centred two-reduction statistics, no second pass over HBM), and write act(LN).  A GLU value is computed
//     (TT + KW - 1) / TT times (2.9 at 31 taps and TT = 16, 4.75 at TT = 8, 2 at 9 taps), its two inputs coming from L2 after the first
//     tile that touched them; the time tile trades that against the number of workgroups (B * ceil(T / TT)): see DESIGN.md for the
//     measured choice.
//   dyn_dwconv1d_causal[_k9]_dgrad / _wgrad   the contracts of dyn_dwconv1d_dgrad / _wgrad with the window shifted (dwconv_window.h's
//     sliding kernels with no left halo / no right halo):
//     dx[t, c] = dx_beta * dx[t, c] + sum_j w[c, j] * dy[t + (KW - 1) - j, c]   (rows past T - 1 are zeros: the gradient of frame t
//     comes from frames t .. t + KW - 1 only)
//     dw[c, j] = beta * dw[c, j] + sum_{b, t} dy[b, t, c] * x[b, t - (KW - 1) + j, c]   per-tile partial sums in the workspace, combined by
//     the fixed-order reducer (reduce.h; deferrable): no atomics, bit-reproducible.
#include "common.h"
#include "dwconv_window.h"
#include "gelu.h"
#include "layernorm_row.h"
#include "reduce.h"

namespace {

using dyn::ld4;
using dyn::st4;

constexpr int ACT_SILU = 0, ACT_GELU = 1;

template <int ACT>
__device__ __forceinline__ float act_f(float x) {
    return ACT == ACT_GELU ? dyn::gelu_f(x) : dyn::silu_f(x);
}

// CB: the entry set has a depthwise bias (cbias may still be null); without it the accumulators start at a literal zero.
template <int KW, int TT, int NV, int ACT, bool CB>
__global__ __launch_bounds__(NV * 256) void convmod_causal_fwd_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                                        const float* __restrict__ cbias, const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, float* __restrict__ s,
                                                                        float* __restrict__ g_out, float* __restrict__ c_out,
                                                                        float* __restrict__ n_out, float* __restrict__ mean_out,
                                                                        float* __restrict__ rstd_out, int64_t T, float eps) {
    constexpr int C = NV * 256, NG = TT + KW - 1, NW = C / 64;
    __shared__ float ys[TT * C];
    const int c = threadIdx.x;
    const int64_t b = blockIdx.y, t0 = (int64_t)blockIdx.x * TT;
    {
        float wk[KW], g[NG];
        const float cb = dyn::load_glu_window(w, CB ? cbias : nullptr, u + b * T * 2 * C + c, c, C, t0 - (KW - 1), T, wk, g);
        if (g_out) {
#pragma unroll
            for (int k = 0; k < TT; ++k)
                if (t0 + k < T) g_out[(b * T + t0 + k) * C + c] = g[KW - 1 + k];
        }
#pragma unroll
        for (int k = 0; k < TT; ++k) {
            float acc = cb;
#pragma unroll
            for (int j = 0; j < KW; ++j) acc += wk[j] * g[k + j];
            ys[k * C + c] = acc;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float4 gm[NV], bt[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        gm[j] = ld4(gamma, lane + 64 * j);
        bt[j] = ld4(beta, lane + 64 * j);
    }
    for (int k = wv; k < TT; k += NW) {
        const int64_t t = t0 + k;
        if (t >= T) break;                              // uniform over the wave
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = ld4(ys + k * C, lane + 64 * j);
        float mean, rstd;
        dyn::row_mean_rstd(v, eps, mean, rstd);
        const int64_t row = b * T + t;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 n = dyn::affine4(v[j], mean, rstd, gm[j], bt[j]);
            if (c_out) st4(c_out + row * C, v[j], lane + 64 * j);
            if (n_out) st4(n_out + row * C, n, lane + 64 * j);
            st4(s + row * C, make_float4(act_f<ACT>(n.x), act_f<ACT>(n.y), act_f<ACT>(n.z), act_f<ACT>(n.w)), lane + 64 * j);
        }
        if (lane == 0) {
            if (mean_out) mean_out[row] = mean;
            if (rstd_out) rstd_out[row] = rstd;
        }
    }
}

template <int KWB>
int check_dims(const char* who, int64_t B, int64_t T, int64_t C, int64_t KW) {
    if (int rc = dyn::check_convmod_dims(who, B, T, C)) return rc;
    DYN_REQUIRE(KW == KWB, DYN_E_UNSUPPORTED, "%s: kernel width %lld is not built (%d)", who, (long long)KW, KWB);
    return DYN_OK;
}

// The checked operands of a forward entry, in the kernel's argument order.
struct FwdArgs {
    const float *u, *w, *cbias, *gamma, *beta;
    float *s, *g, *c, *n, *mean, *rstd;
};

template <int KW>
int check_fwd(const char* who, const FwdArgs& a, int64_t B, int64_t T, int64_t C, int64_t KWin) {
    DYN_REQUIRE(a.u && a.w && a.gamma && a.beta && a.s, DYN_E_ARG, "%s: null pointer", who);
    return check_dims<KW>(who, B, T, C, KWin);
}

int check_fwd_aligned(const char* who, const FwdArgs& a) {
    DYN_REQUIRE(dyn::aligned16(a.u) && dyn::aligned16(a.gamma) && dyn::aligned16(a.beta) && dyn::aligned16(a.s) && dyn::aligned16(a.c) &&
                    dyn::aligned16(a.n),
                DYN_E_ARG, "%s: operands must be 16-byte aligned", who);
    return DYN_OK;
}

template <int KW, int TT, int ACT, bool CB>
int launch_fwd(const char* who, const FwdArgs& a, int64_t B, int64_t T, int64_t C, float eps, void* stream) {
    const dim3 grid((unsigned)dyn::cdiv(T, TT), (unsigned)B);
    dyn::dispatch_nv<1, 2, 3, 4>(C, [&](auto NV) {
        constexpr int nv = decltype(NV)::value;
        hipLaunchKernelGGL((convmod_causal_fwd_kernel<KW, TT, nv, ACT, CB>), grid, dim3(nv * 256), 0, (hipStream_t)stream, a.u, a.w, a.cbias,
                           a.gamma, a.beta, a.s, a.g, a.c, a.n, a.mean, a.rstd, T, eps);
    });
    return dyn::check_launch(who);
}

template <int KW>
int causal_dgrad(const char* who, const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KWin, float dx_beta,
                 void* stream) {
    DYN_REQUIRE(dy && w && dx, DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims<KW>(who, B, T, C, KWin)) return rc;
    if (B == 0 || T == 0) return DYN_OK;
    const dim3 grid((unsigned)dyn::cdiv(T, dyn::DW_TT), (unsigned)dyn::cdiv(C, 256), (unsigned)B);
    hipLaunchKernelGGL((dwconv1d_kernel<KW, 0, true>), grid, dim3(256), 0, (hipStream_t)stream, dy, w, (const float*)nullptr, dx, T, (int)C,
                       dx_beta, 1, (int64_t)0);
    return dyn::check_launch(who);
}

int64_t causal_wgrad_bytes(int64_t B, int64_t T, int64_t C, int64_t KW) {
    int64_t per;
    return dyn::wgrad_tiles(T, &per) * B * C * KW * (int64_t)sizeof(float);
}

template <int KW>
int causal_wgrad(const char* who, const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KWin,
                 void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(x && dy && dw, DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims<KW>(who, B, T, C, KWin)) return rc;
    int64_t per;
    const int64_t chunks = dyn::wgrad_tiles(T, &per), tiles = chunks * B;
    const int64_t bytes = tiles * C * KW * (int64_t)sizeof(float);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "%s: workspace too small (%lld bytes needed)", who, (long long)bytes);
    if (B == 0 || T == 0) return DYN_OK;
    hipStream_t st = (hipStream_t)stream;
    float* pw = dyn::partials_alloc(workspace, bytes);
    const dim3 grid((unsigned)chunks, (unsigned)dyn::cdiv(C, 256), (unsigned)B);
    hipLaunchKernelGGL((dwconv1d_wgrad_kernel<KW, KW - 1, false>), grid, dim3(256), 0, st, x, dy, pw, (float*)nullptr, T, (int)C, per);
    dyn::reduce_or_defer(pw, dw, tiles, C * KW, beta, st);
    return dyn::check_launch(who);
}

}  // namespace

// The default time tile: 16 frames unless that leaves fewer than one workgroup per two CUs (short utterances), then 8.
extern "C" int64_t dyn_convmod_causal_time_tile(int64_t B, int64_t T) { return B * dyn::cdiv(T, 16) >= 128 ? 16 : 8; }

extern "C" int dyn_convmod_causal_fwd(const float* u, const float* w, const float* gamma, const float* beta, float* s, float* g, float* c,
                                      float* n, float* mean, float* rstd, int64_t B, int64_t T, int64_t C, int64_t KW, int32_t act, float eps,
                                      int64_t time_tile, void* stream) {
    const char* who = "dyn_convmod_causal_fwd";
    const FwdArgs a{u, w, nullptr, gamma, beta, s, g, c, n, mean, rstd};
    if (int rc = check_fwd<31>(who, a, B, T, C, KW)) return rc;
    DYN_REQUIRE(act == ACT_SILU || act == ACT_GELU, DYN_E_ARG, "dyn_convmod_causal_fwd: act=%d (0 SiLU, 1 erf GELU)", (int)act);
    DYN_REQUIRE(time_tile == 0 || time_tile == 8 || time_tile == 16, DYN_E_ARG, "dyn_convmod_causal_fwd: time_tile=%lld (0 default, 8, 16)",
                (long long)time_tile);
    if (int rc = check_fwd_aligned(who, a)) return rc;
    if (B == 0 || T == 0) return DYN_OK;
    const int64_t tt = time_tile ? time_tile : dyn_convmod_causal_time_tile(B, T);
    if (tt == 16)
        return act == ACT_GELU ? launch_fwd<31, 16, ACT_GELU, false>(who, a, B, T, C, eps, stream)
                               : launch_fwd<31, 16, ACT_SILU, false>(who, a, B, T, C, eps, stream);
    return act == ACT_GELU ? launch_fwd<31, 8, ACT_GELU, false>(who, a, B, T, C, eps, stream)
                           : launch_fwd<31, 8, ACT_SILU, false>(who, a, B, T, C, eps, stream);
}

extern "C" int dyn_convmod_causal_k9_fwd(const float* u, const float* w, const float* cbias, const float* gamma, const float* beta, float* s,
                                         float* g, float* c, float* n, float* mean, float* rstd, int64_t B, int64_t T, int64_t C, int64_t KW,
                                         float eps, void* stream) {
    const char* who = "dyn_convmod_causal_k9_fwd";
    const FwdArgs a{u, w, cbias, gamma, beta, s, g, c, n, mean, rstd};
    if (int rc = check_fwd<9>(who, a, B, T, C, KW)) return rc;
    if (int rc = check_fwd_aligned(who, a)) return rc;
    if (B == 0 || T == 0) return DYN_OK;
    return launch_fwd<9, 8, ACT_SILU, true>(who, a, B, T, C, eps, stream);
}

extern "C" int dyn_dwconv1d_causal_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                                         void* stream) {
    return causal_dgrad<31>("dyn_dwconv1d_causal_dgrad", dy, w, dx, B, T, C, KW, dx_beta, stream);
}

extern "C" int dyn_dwconv1d_causal_k9_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                                            void* stream) {
    return causal_dgrad<9>("dyn_dwconv1d_causal_k9_dgrad", dy, w, dx, B, T, C, KW, dx_beta, stream);
}

extern "C" int64_t dyn_dwconv1d_causal_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW) { return causal_wgrad_bytes(B, T, C, KW); }

extern "C" int64_t dyn_dwconv1d_causal_k9_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW) {
    return causal_wgrad_bytes(B, T, C, KW);
}

extern "C" int dyn_dwconv1d_causal_wgrad(const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    return causal_wgrad<31>("dyn_dwconv1d_causal_wgrad", x, dy, dw, beta, B, T, C, KW, workspace, workspace_bytes, stream);
}

extern "C" int dyn_dwconv1d_causal_k9_wgrad(const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
    return causal_wgrad<9>("dyn_dwconv1d_causal_k9_wgrad", x, dy, dw, beta, B, T, C, KW, workspace, workspace_bytes, stream);
}
