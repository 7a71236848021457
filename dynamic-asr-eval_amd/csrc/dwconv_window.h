// The register window of the depthwise Conv1d kernels, thread = channel, for conv.hip, convmod_bn.hip, convmod_brn.hip and
// convmod_causal.hip.  Two shapes of it:
//   * the SLIDING window (dwconv1d_kernel, dwconv1d_wgrad_kernel): win[KW] shifts one frame per step, every input element is loaded once
//     per workgroup.  HL frames of halo to the left of t and HR = KW - 1 - HL to the right are compile-time: 'same' padding is
//     HL = (KW - 1) / 2 (15 | 16 at 32 taps, as torch pads), a causal convolution is HL = KW - 1 and its data gradient HL = 0.
//   * the STATIC window of the fused conv-module forwards (load_glu_window): the tile's TT + KW - 1 GLU values formed once into a
//     statically indexed array, the tile's TT outputs correlated from it; what follows (eval BatchNorm, Welford partials, LDS and a wave
//     per LayerNorm row) stays in the kernels.
// No float atomics: the wgrad kernel leaves per-tile partial sums for the fixed-order reducer (reduce.h).  The kernels live in an
// anonymous namespace, one copy per translation unit that instantiates them.
#pragma once
#include "common.h"

namespace dyn {

constexpr int DW_TT = 32;   // time steps per workgroup of the sliding forward / dgrad kernel

// The taps wk[j] = w[c, j] and the window g[i] = GLU(u)[t_first + i, c] of a channel whose column of u [T, 2C] starts at ub; rows outside
// [0, t_end) read as zeros (t_end: T, or the valid row count of a length bucket).  Returns the channel's depthwise bias (cbias may be null: 0).
template <int KW, int NG>
__device__ __forceinline__ float load_glu_window(const float* w, const float* cbias, const float* ub, int c, int C, int64_t t_first,
                                                 int64_t t_end, float (&wk)[KW], float (&g)[NG]) {
#pragma unroll
    for (int j = 0; j < KW; ++j) wk[j] = w[(int64_t)c * KW + j];
    const float cb = cbias ? cbias[c] : 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int64_t t = t_first + i;
        g[i] = (t >= 0 && t < t_end) ? ub[t * 2 * C] * sigmoidf_(ub[t * 2 * C + C]) : 0.f;
    }
    return cb;
}

// Rows (time steps) per wgrad workgroup: short serial chains and up to 2048 workgroups per sample; the partial sums are combined
// afterwards by the fixed-order 2-D reducer (reduce.h).  Returns the tiles per sample.
inline int64_t wgrad_tiles(int64_t T, int64_t* per_block) {
    int64_t chunks = cdiv(T, 8);
    if (chunks > 2048) chunks = 2048;
    if (chunks < 1) chunks = 1;
    *per_block = cdiv(T > 0 ? T : 1, chunks);
    return cdiv(T > 0 ? T : 1, *per_block);
}

// The sizes every fused conv-module entry accepts; the kernel width is the entry's own check.
inline int check_convmod_dims(const char* who, int64_t B, int64_t T, int64_t C) {
    DYN_REQUIRE(B >= 0 && T >= 0 && B < 65536 && B * T < (1ll << 31), DYN_E_ARG, "%s: bad sizes B=%lld T=%lld", who, (long long)B, (long long)T);
    DYN_REQUIRE(C == 256 || C == 512 || C == 768 || C == 1024, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (256, 512, 768, 1024)", who,
                (long long)C);
    return DYN_OK;
}

}  // namespace dyn

namespace {

// y[b, t, c] = beta * y + bias[c] + sum_j w[c, j] * x[b, t + j - HL, c].   FLIP => dgrad (w index reversed).
// grid (ceil(T / DW_TT), ceil(C / 256), B).
template <int KW, int HL, bool FLIP>
__global__ __launch_bounds__(256) void dwconv1d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int64_t T,
                                                        int C, float beta, int ngroups, int64_t pstride) {
    constexpr int HR = KW - 1 - HL, TT = dyn::DW_TT;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t b = blockIdx.z;
    {   // lockstep group: sample b convolves with the filters of replica b % ngroups (ngroups = 1: plain launch)
        const int64_t poff = (int64_t)(blockIdx.z % ngroups) * pstride;
        w += poff;
        if (bias) bias += poff;
    }
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    float wk[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) wk[j] = w[(int64_t)c * KW + (FLIP ? KW - 1 - j : j)];
    const float bv = bias ? bias[c] : 0.f;
    const float* xb = x + b * T * C + c;
    float* yb = y + b * T * C + c;
    float win[KW];
#pragma unroll
    for (int j = 0; j < KW - 1; ++j) {
        const int64_t t = t0 + j - HL;                      // t0 < T: with no halo on a side, that side needs no test
        win[j + 1] = ((HL == 0 || t >= 0) && (HR == 0 || t < T)) ? xb[t * C] : 0.f;
    }
    for (int k = 0; k < TT; ++k) {
        const int64_t t = t0 + k;
        if (t >= T) break;
#pragma unroll
        for (int j = 0; j < KW - 1; ++j) win[j] = win[j + 1];
        const int64_t tn = t + HR;
        win[KW - 1] = (HR == 0 || tn < T) ? xb[tn * C] : 0.f;
        float acc = bv;
#pragma unroll
        for (int j = 0; j < KW; ++j) acc += wk[j] * win[j];
        yb[t * C] = beta != 0.f ? acc + beta * yb[t * C] : acc;
    }
}

// partial_w[tile, c, j] = sum_{t in tile} dy[b, t, c] * x[b, t + j - HL, c], j = 0 .. KW - 1;   BIAS: partial_b[tile, c] = sum dy.
// grid (wgrad_tiles(T), ceil(C / 256), B), tile = b * gridDim.x + blockIdx.x.
template <int KW, int HL, bool BIAS>
__global__ __launch_bounds__(256) void dwconv1d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ partial_w, float* __restrict__ partial_b,
                                                              int64_t T, int C, int64_t t_per_block) {
    constexpr int HR = KW - 1 - HL;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t b = blockIdx.z;
    const int64_t t0 = (int64_t)blockIdx.x * t_per_block;
    const int64_t t1 = (t0 + t_per_block < T) ? t0 + t_per_block : T;
    const float* xb = x + b * T * C + c;
    const float* gb = dy + b * T * C + c;
    float acc[KW], win[KW];
    float accb = 0.f;
#pragma unroll
    for (int j = 0; j < KW; ++j) acc[j] = 0.f;
#pragma unroll
    for (int j = 0; j < KW - 1; ++j) {
        const int64_t t = t0 + j - HL;
        win[j + 1] = ((HL == 0 || t >= 0) && (HR == 0 || t < T)) ? xb[t * C] : 0.f;
    }
    for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
        for (int j = 0; j < KW - 1; ++j) win[j] = win[j + 1];
        const int64_t tn = t + HR;
        win[KW - 1] = (HR == 0 || tn < T) ? xb[tn * C] : 0.f;
        const float g = gb[t * C];
        if (BIAS) accb += g;
#pragma unroll
        for (int j = 0; j < KW; ++j) acc[j] += g * win[j];
    }
    const int64_t tile = (int64_t)blockIdx.z * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < KW; ++j) partial_w[(tile * C + c) * KW + j] = acc[j];
    if (BIAS) partial_b[tile * C + c] = accb;
}

}  // namespace
