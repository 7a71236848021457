// The causal x8 subsampling of NemotronAsrStreamingForRNNT (transformers modeling_nemotron_asr_streaming.py,
// NemotronAsrStreamingEncoderCausalConv2D.forward: `F.pad(x, freq_pad)`, `F.pad(x, (0, 0, *time_pad))`, `super().forward(x)`): every 3x3
// stride-2 convolution pads (kernel - 1, stride - 1) = (2, 1) on BOTH axes, so one stage maps n -> n / 2 + 1 (80 -> 41 -> 21 -> 11: odd
// widths) and output (to, fo) reads the inputs (2 to + dt - 2, 2 fo + df - 2), dt, df in 0 .. 2.  conv.hip's stages pad (1, 1) and are
// left as they are; these are their causal siblings, channels-last, C % 4 == 0, any T >= 1 and F >= 1:
//   dyn_conv2d_first_causal_fwd / _wgrad          the dense stem, x [B, T, F] -> z [B, To, Fo, C] (pre-activation), w [C, 3, 3]
//   dyn_dwconv2d_s2_causal_fwd_act / _dgrad_act / _wgrad_act   the depthwise stage with the activation of its input fused into the loads:
//                                                 u = bias + dw3x3(act(z)), dz = act'(z) * (the transposed convolution of du)
// The forwards and the dgrad are one thread per four channels of one output element (16-byte accesses, every index checked against the
// tensor); the weight gradients one thread per channel over a tile of output rows, partial sums per tile in the workspace combined by the
// fixed-order reducer (deferrable): no float atomics.  The reference loop freezes this part; it runs once per window.
#include "common.h"
#include "layernorm_row.h"

namespace {

using dyn::ld4;
using dyn::st4;

constexpr int ACT_RELU = 1;    // the `act` codes of conv.hip's _act entries; 0 (SiLU) has no caller here and is not built

__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

// z[b, to, fo, 4 c4 ..] = bias + sum_{dt, df} w[c, dt, df] * x[b, 2 to + dt - 2, 2 fo + df - 2]
__global__ __launch_bounds__(256) void conv2d_first_causal_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, float* __restrict__ z, int64_t total,
                                                                       int64_t T, int F, int64_t To, int Fo, int C4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        const int fo = (int)((e / C4) % Fo);
        const int64_t to = (e / C4 / Fo) % To, b = e / C4 / Fo / To;
        const float* xb = x + b * T * F;
        const float* wc = w + (int64_t)c4 * 36;
        float4 acc = ld4(bias, c4);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int64_t t = 2 * to + dt - 2;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int f = 2 * fo + df - 2;
                const float v = (t >= 0 && t < T && f >= 0 && f < F) ? xb[t * F + f] : 0.f;
                const int j = dt * 3 + df;
                acc.x += wc[j] * v; acc.y += wc[9 + j] * v; acc.z += wc[18 + j] * v; acc.w += wc[27 + j] * v;
            }
        }
        st4(z, acc, e);
    }
}

// u[b, to, fo, c] = bias[c] + sum_{dt, df} w[c, dt, df] * relu(z[b, 2 to + dt - 2, 2 fo + df - 2, c])
__global__ __launch_bounds__(256) void dwconv2d_s2_causal_fwd_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                                      const float* __restrict__ bias, float* __restrict__ u, int64_t total,
                                                                      int64_t T, int F, int64_t To, int Fo, int C4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        const int fo = (int)((e / C4) % Fo);
        const int64_t to = (e / C4 / Fo) % To, b = e / C4 / Fo / To;
        const float* wc = w + (int64_t)c4 * 36;
        float4 acc = ld4(bias, c4);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int64_t t = 2 * to + dt - 2;
            if (t < 0 || t >= T) continue;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int f = 2 * fo + df - 2;
                if (f < 0 || f >= F) continue;
                const float4 v = relu4(ld4(z, ((b * T + t) * F + f) * C4 + c4));
                const int j = dt * 3 + df;
                acc.x += wc[j] * v.x; acc.y += wc[9 + j] * v.y; acc.z += wc[18 + j] * v.z; acc.w += wc[27 + j] * v.w;
            }
        }
        st4(u, acc, e);
    }
}

// dz[b, t, f, c] = [z > 0] * sum_{(to, dt), (fo, df): 2 to + dt - 2 = t, 2 fo + df - 2 = f} w[c, dt, df] * du[b, to, fo, c]
__global__ __launch_bounds__(256) void dwconv2d_s2_causal_dgrad_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                                        const float* __restrict__ du, float* __restrict__ dz, int64_t total,
                                                                        int64_t T, int F, int64_t To, int Fo, int C4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        const int f = (int)((e / C4) % F);
        const int64_t t = (e / C4 / F) % T, b = e / C4 / F / T;
        const float* wc = w + (int64_t)c4 * 36;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int64_t tt = t + 2 - dt;                       // = 2 to, >= 0
            if ((tt & 1) || (tt >> 1) >= To) continue;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int ff = f + 2 - df;                       // = 2 fo, >= 0
                if ((ff & 1) || (ff >> 1) >= Fo) continue;
                const float4 g = ld4(du, ((b * To + (tt >> 1)) * Fo + (ff >> 1)) * C4 + c4);
                const int j = dt * 3 + df;
                acc.x += wc[j] * g.x; acc.y += wc[9 + j] * g.y; acc.z += wc[18 + j] * g.z; acc.w += wc[27 + j] * g.w;
            }
        }
        const float4 zv = ld4(z, e);
        st4(dz, make_float4(zv.x > 0.f ? acc.x : 0.f, zv.y > 0.f ? acc.y : 0.f, zv.z > 0.f ? acc.z : 0.f, zv.w > 0.f ? acc.w : 0.f), e);
    }
}

// partial_w[tile, c, 9], partial_b[tile, c] over the tile's output rows.  FIRST: the input is x [B, T, F] (one channel, no activation),
// else relu(z [B, T, F, C]).
template <bool FIRST>
__global__ __launch_bounds__(256) void conv2d_s2_causal_wgrad_kernel(const float* __restrict__ in, const float* __restrict__ g_out,
                                                                      float* __restrict__ partial_w, float* __restrict__ partial_b, int64_t T,
                                                                      int F, int64_t To, int Fo, int C, int64_t to_per_block) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t b = blockIdx.z;
    if (c >= C) return;
    const int64_t to0 = (int64_t)blockIdx.x * to_per_block;
    const int64_t to1 = (to0 + to_per_block < To) ? to0 + to_per_block : To;
    float acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.f;
    float accb = 0.f;
    const float* ib = FIRST ? in + b * T * F : in + b * T * F * C + c;
    for (int64_t to = to0; to < to1; ++to) {
        const float* gz = g_out + ((b * To + to) * Fo) * C + c;
        for (int fo = 0; fo < Fo; ++fo) {
            const float g = gz[(int64_t)fo * C];
            accb += g;
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) {
                const int64_t t = 2 * to + dt - 2;
                if (t < 0 || t >= T) continue;
#pragma unroll
                for (int df = 0; df < 3; ++df) {
                    const int f = 2 * fo + df - 2;
                    if (f < 0 || f >= F) continue;
                    const float v = FIRST ? ib[t * F + f] : fmaxf(ib[(t * F + f) * C], 0.f);
                    acc[dt * 3 + df] += g * v;
                }
            }
        }
    }
    const int64_t tile = (int64_t)blockIdx.z * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < 9; ++j) partial_w[(tile * C + c) * 9 + j] = acc[j];
    partial_b[tile * C + c] = accb;
}

// Output rows per weight-gradient workgroup: wgrad_tiles2d of conv.hip (up to 4096 tiles per sample).
inline int64_t wgrad_tiles(int64_t To, int64_t* per_block) {
    int64_t chunks = To < 4096 ? To : 4096;
    if (chunks < 1) chunks = 1;
    *per_block = dyn::cdiv(To > 0 ? To : 1, chunks);
    return dyn::cdiv(To > 0 ? To : 1, *per_block);
}

int check_dims(const char* who, int64_t B, int64_t T, int64_t F, int64_t C) {
    DYN_REQUIRE(B >= 0 && B < 65536 && T >= 1 && F >= 1 && F < (1 << 20) && C >= 4 && C <= 65536, DYN_E_ARG,
                "%s: bad sizes B=%lld T=%lld F=%lld C=%lld", who, (long long)B, (long long)T, (long long)F, (long long)C);
    DYN_REQUIRE(C % 4 == 0, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (a multiple of 4)", who, (long long)C);
    DYN_REQUIRE(B * T * F * C < (1ll << 40), DYN_E_ARG, "%s: too many elements for one launch", who);
    return DYN_OK;
}

int check_act(const char* who, int32_t act) {
    DYN_REQUIRE(act == ACT_RELU, DYN_E_UNSUPPORTED, "%s: act=%d is not built (1 ReLU)", who, (int)act);
    return DYN_OK;
}

inline unsigned flat_grid(int64_t total) {
    const int64_t g = dyn::cdiv(total, 256);
    return (unsigned)(g < 65536 ? g : 65536);
}

template <bool FIRST>
int wgrad_impl(const char* who, const float* in, const float* g, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F, int64_t C,
               void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(in && g && dw && dbias, DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, T, F, C)) return rc;
    const int64_t To = T / 2 + 1, Fo = F / 2 + 1;
    int64_t per;
    const int64_t chunks = wgrad_tiles(To, &per), tiles = chunks * B;
    const int64_t bytes = tiles * C * 10 * (int64_t)sizeof(float);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "%s: workspace too small (%lld bytes needed)", who, (long long)bytes);
    if (B == 0) return DYN_OK;
    hipStream_t st = (hipStream_t)stream;
    float* pw = dyn::partials_alloc(workspace, bytes);
    float* pb = pw + tiles * C * 9;
    const dim3 grid((unsigned)chunks, (unsigned)dyn::cdiv(C, 256), (unsigned)B);
    hipLaunchKernelGGL(conv2d_s2_causal_wgrad_kernel<FIRST>, grid, dim3(256), 0, st, in, g, pw, pb, T, (int)F, To, (int)Fo, (int)C, per);
    if (int rc = dyn::check_launch(who)) return rc;
    dyn::reduce_or_defer(pw, dw, tiles, C * 9, beta, st);
    dyn::reduce_or_defer(pb, dbias, tiles, C, beta, st);
    return dyn::check_launch(who);
}

}  // namespace

extern "C" int dyn_conv2d_first_causal_fwd(const float* x, const float* w, const float* bias, float* z, int64_t B, int64_t T, int64_t F, int64_t C,
                                           void* stream) {
    DYN_REQUIRE(x && w && bias && z, DYN_E_ARG, "dyn_conv2d_first_causal_fwd: null pointer");
    if (int rc = check_dims("dyn_conv2d_first_causal_fwd", B, T, F, C)) return rc;
    DYN_REQUIRE(dyn::aligned16(bias) && dyn::aligned16(z), DYN_E_ARG, "dyn_conv2d_first_causal_fwd: bias and z must be 16-byte aligned");
    if (B == 0) return DYN_OK;
    const int64_t To = T / 2 + 1, Fo = F / 2 + 1, total = B * To * Fo * (C / 4);
    hipLaunchKernelGGL(conv2d_first_causal_fwd_kernel, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, x, w, bias, z, total, T, (int)F,
                       To, (int)Fo, (int)(C / 4));
    return dyn::check_launch("dyn_conv2d_first_causal_fwd");
}

extern "C" int64_t dyn_conv2d_causal_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C) {
    if (B < 0 || T < 1 || C < 1) return 0;
    int64_t per;
    return wgrad_tiles(T / 2 + 1, &per) * B * C * 10 * (int64_t)sizeof(float);
}

extern "C" int dyn_conv2d_first_causal_wgrad(const float* x, const float* dz, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                                             int64_t C, void* workspace, int64_t workspace_bytes, void* stream) {
    return wgrad_impl<true>("dyn_conv2d_first_causal_wgrad", x, dz, dw, dbias, beta, B, T, F, C, workspace, workspace_bytes, stream);
}

extern "C" int dyn_dwconv2d_s2_causal_fwd_act(const float* z, const float* w, const float* bias, float* u, int64_t B, int64_t T, int64_t F,
                                              int64_t C, int32_t act, void* stream) {
    DYN_REQUIRE(z && w && bias && u, DYN_E_ARG, "dyn_dwconv2d_s2_causal_fwd_act: null pointer");
    if (int rc = check_act("dyn_dwconv2d_s2_causal_fwd_act", act)) return rc;
    if (int rc = check_dims("dyn_dwconv2d_s2_causal_fwd_act", B, T, F, C)) return rc;
    DYN_REQUIRE(dyn::aligned16(z) && dyn::aligned16(bias) && dyn::aligned16(u), DYN_E_ARG,
                "dyn_dwconv2d_s2_causal_fwd_act: z, bias and u must be 16-byte aligned");
    if (B == 0) return DYN_OK;
    const int64_t To = T / 2 + 1, Fo = F / 2 + 1, total = B * To * Fo * (C / 4);
    hipLaunchKernelGGL(dwconv2d_s2_causal_fwd_kernel, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, z, w, bias, u, total, T, (int)F, To,
                       (int)Fo, (int)(C / 4));
    return dyn::check_launch("dyn_dwconv2d_s2_causal_fwd_act");
}

extern "C" int dyn_dwconv2d_s2_causal_dgrad_act(const float* z, const float* w, const float* du, float* dz, int64_t B, int64_t T, int64_t F,
                                                int64_t C, int32_t act, void* stream) {
    DYN_REQUIRE(z && w && du && dz, DYN_E_ARG, "dyn_dwconv2d_s2_causal_dgrad_act: null pointer");
    if (int rc = check_act("dyn_dwconv2d_s2_causal_dgrad_act", act)) return rc;
    if (int rc = check_dims("dyn_dwconv2d_s2_causal_dgrad_act", B, T, F, C)) return rc;
    DYN_REQUIRE(dyn::aligned16(z) && dyn::aligned16(du) && dyn::aligned16(dz), DYN_E_ARG,
                "dyn_dwconv2d_s2_causal_dgrad_act: z, du and dz must be 16-byte aligned");
    if (B == 0) return DYN_OK;
    const int64_t To = T / 2 + 1, Fo = F / 2 + 1, total = B * T * F * (C / 4);
    hipLaunchKernelGGL(dwconv2d_s2_causal_dgrad_kernel, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, z, w, du, dz, total, T, (int)F,
                       To, (int)Fo, (int)(C / 4));
    return dyn::check_launch("dyn_dwconv2d_s2_causal_dgrad_act");
}

extern "C" int dyn_dwconv2d_s2_causal_wgrad_act(const float* z, const float* du, float* dw, float* dbias, float beta, int64_t B, int64_t T,
                                                int64_t F, int64_t C, int32_t act, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_act("dyn_dwconv2d_s2_causal_wgrad_act", act)) return rc;
    return wgrad_impl<false>("dyn_dwconv2d_s2_causal_wgrad_act", z, du, dw, dbias, beta, B, T, F, C, workspace, workspace_bytes, stream);
}
