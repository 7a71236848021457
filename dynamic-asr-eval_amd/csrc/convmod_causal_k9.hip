// The core of NemotronAsrStreamingForRNNT's conformer convolution module (transformers modeling_nemotron_asr_streaming.py,
// NemotronAsrStreamingEncoderConvolutionModule.forward) between its two pointwise convolutions:
//     nn.functional.glu -> depthwise_conv (NemotronAsrStreamingEncoderCausalConv1d: left padding of kernel_size - 1, optional bias)
//     -> self.norm (LayerNorm over channels, affine) -> self.activation (SiLU)
// KW = 9 taps, C in {256, 512, 768, 1024}, channels-last.  The 31-tap, bias-free entries of convmod_causal.hip (Wav2Vec2-BERT) stay as
// they are; these are their siblings at 9 taps with the depthwise bias:
//   dyn_convmod_causal_k9_fwd     u [B, T, 2C] -> s [B, T, C] = silu(LN_C(cbias[c] + sum_j w[c, j] * GLU(u)[t - 8 + j, c])) in ONE launch.
//     One workgroup of C threads per (sample, tile of TT = 8 frames), thread = channel: its TT + 8 GLU values are loaded ONCE into
//     registers, its TT outputs go to LDS [TT][C]; after one barrier the waves take the tile's frames in turn, each holding a whole frame
//     as float4s (layernorm_row.h: centred two-reduction statistics) and write silu(LN).  A GLU value is computed twice.
//   dyn_dwconv1d_causal_k9_dgrad / _wgrad   the contracts of dyn_dwconv1d_causal_dgrad / _wgrad at 9 taps.  The bias gradient is the
//     column sum of dy (dyn_colsum): no entry of its own.
#include "common.h"
#include "layernorm_row.h"

namespace {

using dyn::ld4;
using dyn::st4;

constexpr int KW9 = 9;
constexpr int TT = 8;    // frames per forward workgroup: 32 KB of LDS at C = 1024, 16 GLU values per thread
constexpr int DT = 32;   // frames per dgrad workgroup (dwconv1d_causal_dgrad_kernel's tile)

__device__ __forceinline__ float silu_f(float x) { return x * dyn::sigmoidf_(x); }

template <int KW, int NV>
__global__ __launch_bounds__(NV * 256) void convmod_causal_k_fwd_kernel(const float* __restrict__ u, const float* __restrict__ w,
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
#pragma unroll
        for (int j = 0; j < KW; ++j) wk[j] = w[(int64_t)c * KW + j];
        const float cb = cbias ? cbias[c] : 0.f;
        const float* ub = u + b * T * 2 * C + c;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int64_t t = t0 - (KW - 1) + i;
            g[i] = (t >= 0 && t < T) ? ub[t * 2 * C] * dyn::sigmoidf_(ub[t * 2 * C + C]) : 0.f;
        }
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
            st4(s + row * C, make_float4(silu_f(n.x), silu_f(n.y), silu_f(n.z), silu_f(n.w)), lane + 64 * j);
        }
        if (lane == 0) {
            if (mean_out) mean_out[row] = mean;
            if (rstd_out) rstd_out[row] = rstd;
        }
    }
}

// dx[b, t, c] = beta * dx + sum_i w[c, KW - 1 - i] * dy[b, t + i, c]: the window slides through registers.
template <int KW>
__global__ __launch_bounds__(256) void dwconv1d_causal_k_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                       float* __restrict__ dx, int64_t T, int C, float beta) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t b = blockIdx.z, t0 = (int64_t)blockIdx.x * DT;
    float wk[KW], win[KW];
#pragma unroll
    for (int i = 0; i < KW; ++i) wk[i] = w[(int64_t)c * KW + (KW - 1 - i)];
    const float* gb = dy + b * T * C + c;
    float* xb = dx + b * T * C + c;
#pragma unroll
    for (int i = 0; i < KW - 1; ++i) {
        const int64_t t = t0 + i;
        win[i + 1] = t < T ? gb[t * C] : 0.f;
    }
    for (int k = 0; k < DT; ++k) {
        const int64_t t = t0 + k;
        if (t >= T) break;
#pragma unroll
        for (int i = 0; i < KW - 1; ++i) win[i] = win[i + 1];
        const int64_t tn = t + KW - 1;
        win[KW - 1] = tn < T ? gb[tn * C] : 0.f;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < KW; ++i) acc += wk[i] * win[i];
        xb[t * C] = beta != 0.f ? acc + beta * xb[t * C] : acc;
    }
}

// partial[tile, c, j] = sum_{t in tile} dy[b, t, c] * x[b, t - (KW - 1) + j, c]
template <int KW>
__global__ __launch_bounds__(256) void dwconv1d_causal_k_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                       float* __restrict__ partial_w, int64_t T, int C, int64_t t_per_block) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t b = blockIdx.z;
    const int64_t t0 = (int64_t)blockIdx.x * t_per_block;
    const int64_t t1 = (t0 + t_per_block < T) ? t0 + t_per_block : T;
    const float* xb = x + b * T * C + c;
    const float* gb = dy + b * T * C + c;
    float acc[KW], win[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) acc[j] = 0.f;
#pragma unroll
    for (int j = 0; j < KW - 1; ++j) {
        const int64_t t = t0 - (KW - 1) + j;            // < t0 <= T - 1
        win[j + 1] = t >= 0 ? xb[t * C] : 0.f;
    }
    for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
        for (int j = 0; j < KW - 1; ++j) win[j] = win[j + 1];
        win[KW - 1] = xb[t * C];
        const float g = gb[t * C];
#pragma unroll
        for (int j = 0; j < KW; ++j) acc[j] += g * win[j];
    }
    const int64_t tile = (int64_t)blockIdx.z * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < KW; ++j) partial_w[(tile * C + c) * KW + j] = acc[j];
}

// Rows per wgrad workgroup: wgrad_tiles of convmod_causal.hip
inline int64_t wgrad_tiles(int64_t T, int64_t* per_block) {
    int64_t chunks = dyn::cdiv(T, 8);
    if (chunks > 2048) chunks = 2048;
    if (chunks < 1) chunks = 1;
    *per_block = dyn::cdiv(T > 0 ? T : 1, chunks);
    return dyn::cdiv(T > 0 ? T : 1, *per_block);
}

int check_dims(const char* who, int64_t B, int64_t T, int64_t C, int64_t KW) {
    DYN_REQUIRE(B >= 0 && T >= 0 && B < 65536 && B * T < (1ll << 31), DYN_E_ARG, "%s: bad sizes B=%lld T=%lld", who, (long long)B, (long long)T);
    DYN_REQUIRE(KW == KW9, DYN_E_UNSUPPORTED, "%s: kernel width %lld is not built (9)", who, (long long)KW);
    DYN_REQUIRE(C == 256 || C == 512 || C == 768 || C == 1024, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (256, 512, 768, 1024)", who,
                (long long)C);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_convmod_causal_k9_fwd(const float* u, const float* w, const float* cbias, const float* gamma, const float* beta, float* s,
                                         float* g, float* c, float* n, float* mean, float* rstd, int64_t B, int64_t T, int64_t C, int64_t KW,
                                         float eps, void* stream) {
    DYN_REQUIRE(u && w && gamma && beta && s, DYN_E_ARG, "dyn_convmod_causal_k9_fwd: null pointer");
    if (int rc = check_dims("dyn_convmod_causal_k9_fwd", B, T, C, KW)) return rc;
    DYN_REQUIRE(dyn::aligned16(u) && dyn::aligned16(gamma) && dyn::aligned16(beta) && dyn::aligned16(s) && dyn::aligned16(c) && dyn::aligned16(n),
                DYN_E_ARG, "dyn_convmod_causal_k9_fwd: operands must be 16-byte aligned");
    if (B == 0 || T == 0) return DYN_OK;
    const dim3 grid((unsigned)dyn::cdiv(T, TT), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    dyn::dispatch_nv<1, 2, 3, 4>(C, [&](auto NV) {
        hipLaunchKernelGGL((convmod_causal_k_fwd_kernel<KW9, decltype(NV)::value>), grid, dim3(decltype(NV)::value * 256), 0, st, u, w, cbias, gamma,
                           beta, s, g, c, n, mean, rstd, T, eps);
    });
    return dyn::check_launch("dyn_convmod_causal_k9_fwd");
}

extern "C" int dyn_dwconv1d_causal_k9_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                                            void* stream) {
    DYN_REQUIRE(dy && w && dx, DYN_E_ARG, "dyn_dwconv1d_causal_k9_dgrad: null pointer");
    if (int rc = check_dims("dyn_dwconv1d_causal_k9_dgrad", B, T, C, KW)) return rc;
    if (B == 0 || T == 0) return DYN_OK;
    const dim3 grid((unsigned)dyn::cdiv(T, DT), (unsigned)dyn::cdiv(C, 256), (unsigned)B);
    hipLaunchKernelGGL((dwconv1d_causal_k_dgrad_kernel<KW9>), grid, dim3(256), 0, (hipStream_t)stream, dy, w, dx, T, (int)C, dx_beta);
    return dyn::check_launch("dyn_dwconv1d_causal_k9_dgrad");
}

extern "C" int64_t dyn_dwconv1d_causal_k9_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW) {
    int64_t per;
    return wgrad_tiles(T, &per) * B * C * KW * (int64_t)sizeof(float);
}

extern "C" int dyn_dwconv1d_causal_k9_wgrad(const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(x && dy && dw, DYN_E_ARG, "dyn_dwconv1d_causal_k9_wgrad: null pointer");
    if (int rc = check_dims("dyn_dwconv1d_causal_k9_wgrad", B, T, C, KW)) return rc;
    int64_t per;
    const int64_t chunks = wgrad_tiles(T, &per), tiles = chunks * B;
    const int64_t bytes = tiles * C * KW * (int64_t)sizeof(float);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "dyn_dwconv1d_causal_k9_wgrad: workspace too small (%lld bytes needed)",
                (long long)bytes);
    if (B == 0 || T == 0) return DYN_OK;
    hipStream_t st = (hipStream_t)stream;
    float* pw = dyn::partials_alloc(workspace, bytes);
    const dim3 grid((unsigned)chunks, (unsigned)dyn::cdiv(C, 256), (unsigned)B);
    hipLaunchKernelGGL((dwconv1d_causal_k_wgrad_kernel<KW9>), grid, dim3(256), 0, st, x, dy, pw, T, (int)C, per);
    dyn::reduce_or_defer(pw, dw, tiles, C * KW, beta, st);
    return dyn::check_launch("dyn_dwconv1d_causal_k9_wgrad");
}
