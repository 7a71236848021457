// Conv bias + LayerNorm over channels + exact GELU in one pass each way: the feature-extractor layer of the layer-norm wav2vec2
// layout (`feat_extract_norm: "layer"`, `conv_bias: true`; transformers Wav2Vec2LayerNormConvLayer.forward: conv -> transpose ->
// LayerNorm(C) -> transpose -> GELU), which runs on all seven layers and so on the largest activations of the model.
//   forward:  act = gelu(LN(z + conv_bias));  mean / rstd [rows] kept for the backward; z (the raw conv output) is left alone
//   backward: xhat and n = xhat * gamma + beta are RECOMPUTED from z, mean, rstd (the normalised tensor is never stored),
//             dn = dact * gelu'(n), dz = LayerNorm backward of dn, dgamma = sum dn * xhat, dbeta = sum dn, dconv_bias = sum dz.
// The row kernels are layernorm_row.h's (one wave64 per row, NV = C / 256 float4 per lane and tensor); the three column sums are
// accumulated per workgroup in registers, written as partial rows and summed by the fixed-order reducers.  Nothing here synchronises or allocates.
// Registers at C = 512 (NV = 2): the backward holds z, dact (16 floats), three accumulators (24) and gamma, beta, bias (24) per lane,
// 117 VGPRs = 4 waves per SIMD; its LDS is the 4 KiB combine buffer.  HBM-bound, so the backward spreads the rows over up to 1024
// workgroups of 4 rows in flight (4 waves on every SIMD at the 52428-row layer) at 3 partial rows of C floats per workgroup.
#include "common.h"
#include "gelu.h"
#include "layernorm_row.h"
#include "reduce.h"

namespace {

using dyn::aligned16;
using dyn::ld4;
using dyn::st4;
constexpr int WPB = dyn::ROW_WPB;
constexpr int MAX_BWD_BLOCKS = 1024;

template <int NV>
__global__ __launch_bounds__(256) void blg_fwd_kernel(const float* __restrict__ z, const float* __restrict__ cbias,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ act, float* __restrict__ mean_out,
                                                       float* __restrict__ rstd_out, int64_t rows, float eps) {
    constexpr int C = NV * 256;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 g[NV], b[NV], cb[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        g[j] = ld4(gamma, lane + 64 * j);
        b[j] = ld4(beta, lane + 64 * j);
        cb[j] = cbias ? ld4(cbias, lane + 64 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < rows; row += (int64_t)gridDim.x * WPB) {
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = ld4(z + row * C, lane + 64 * j);
            dyn::add4(v[j], cb[j]);
            s += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        float mean, rstd;
        dyn::row_mean_rstd(v, s, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o;
            o.x = dyn::gelu_f((v[j].x - mean) * rstd * g[j].x + b[j].x);
            o.y = dyn::gelu_f((v[j].y - mean) * rstd * g[j].y + b[j].y);
            o.z = dyn::gelu_f((v[j].z - mean) * rstd * g[j].z + b[j].z);
            o.w = dyn::gelu_f((v[j].w - mean) * rstd * g[j].w + b[j].w);
            st4(act + row * C, o, lane + 64 * j);
        }
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
    }
}

// partial_g / partial_b / partial_c [gridDim.x, C]: this workgroup's sums of dn * xhat, dn and dz (a null pointer: not wanted).
// dz may be dact itself: a lane reads exactly the elements it later writes.
template <int NV>
__global__ __launch_bounds__(256) void blg_bwd_kernel(const float* __restrict__ z, const float* __restrict__ cbias,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                       const float* dact, float* dz, float* __restrict__ partial_g,
                                                       float* __restrict__ partial_b, float* __restrict__ partial_c, int64_t rows) {
    constexpr int C = NV * 256;
    __shared__ float4 red[WPB][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 g[NV], b[NV], cb[NV], ag[NV], ab[NV], ac[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        g[j] = ld4(gamma, lane + 64 * j);
        b[j] = ld4(beta, lane + 64 * j);
        cb[j] = cbias ? ld4(cbias, lane + 64 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        ag[j] = ab[j] = ac[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < rows; row += (int64_t)gridDim.x * WPB) {
        const float mean = mean_in[row], rstd = rstd_in[row];
        float4 xh[NV], gy[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 v = ld4(z + row * C, lane + 64 * j);
            const float4 d = ld4(dact + row * C, lane + 64 * j);
            xh[j].x = (v.x + cb[j].x - mean) * rstd; xh[j].y = (v.y + cb[j].y - mean) * rstd;
            xh[j].z = (v.z + cb[j].z - mean) * rstd; xh[j].w = (v.w + cb[j].w - mean) * rstd;
            float4 dn;
            dn.x = d.x * dyn::gelu_grad(xh[j].x * g[j].x + b[j].x);
            dn.y = d.y * dyn::gelu_grad(xh[j].y * g[j].y + b[j].y);
            dn.z = d.z * dyn::gelu_grad(xh[j].z * g[j].z + b[j].z);
            dn.w = d.w * dyn::gelu_grad(xh[j].w * g[j].w + b[j].w);
            ag[j].x += dn.x * xh[j].x; ag[j].y += dn.y * xh[j].y; ag[j].z += dn.z * xh[j].z; ag[j].w += dn.w * xh[j].w;
            ab[j].x += dn.x; ab[j].y += dn.y; ab[j].z += dn.z; ab[j].w += dn.w;
            gy[j].x = dn.x * g[j].x; gy[j].y = dn.y * g[j].y; gy[j].z = dn.z * g[j].z; gy[j].w = dn.w * g[j].w;
            dyn::bwd_lane_sums(gy[j], xh[j], s1, s2);
        }
        dyn::bwd_row_means<NV>(s1, s2);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 o = dyn::bwd4(gy[j], xh[j], rstd, s1, s2);
            dyn::add4(ac[j], o);
            st4(dz + row * C, o, lane + 64 * j);
        }
    }
    if (partial_g) dyn::combine_waves(ag, red, partial_g + (int64_t)blockIdx.x * C);     // null or not: uniform over the grid
    if (partial_b) dyn::combine_waves(ab, red, partial_b + (int64_t)blockIdx.x * C);
    if (partial_c) dyn::combine_waves(ac, red, partial_c + (int64_t)blockIdx.x * C);
}

// The same two passes for the narrow extractors (SEW: conv_dim 64 and 128): C = 4 * LPR channels, a row on LPR = 16 or 32 lanes (one float4
// each), so a wave64 holds RPW = 64 / LPR rows at a time and the row statistics are reductions over an aligned group of LPR lanes.  The
// column sums: per lane over its rows, then over the wave's RPW row groups (xor 32, then 16: a fixed order), then over the 4 waves through
// LDS in wave order, one partial row of C floats per workgroup.  A lane whose row is past the end loads nothing and stores nothing.
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int LPR>
__device__ __forceinline__ float4 across_groups(float4 v) {
#pragma unroll
    for (int o = 32; o >= LPR; o >>= 1) {
        v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64); v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
    }
    return v;
}

template <int LPR>
__global__ __launch_bounds__(256) void blg_fwd_narrow_kernel(const float* __restrict__ z, const float* __restrict__ cbias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ act, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out, int64_t rows, float eps) {
    constexpr int C = 4 * LPR, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, cl = lane % LPR, sub = lane / LPR;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g = ld4(gamma, cl), b = ld4(beta, cl), cb = cbias ? ld4(cbias, cl) : zero;
    for (int64_t base = ((int64_t)blockIdx.x * WPB + w) * RPW; base < rows; base += (int64_t)gridDim.x * WPB * RPW) {
        const int64_t row = base + sub;
        const bool live = row < rows;
        float4 v = live ? ld4(z + row * C, cl) : zero;
        v.x += cb.x; v.y += cb.y; v.z += cb.z; v.w += cb.w;
        const float mean = group_sum<LPR>(v.x + v.y + v.z + v.w) / C;
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        const float rstd = rsqrtf(group_sum<LPR>(a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3) / C + eps);
        if (!live) continue;
        float4 o;
        o.x = dyn::gelu_f(a0 * rstd * g.x + b.x); o.y = dyn::gelu_f(a1 * rstd * g.y + b.y);
        o.z = dyn::gelu_f(a2 * rstd * g.z + b.z); o.w = dyn::gelu_f(a3 * rstd * g.w + b.w);
        reinterpret_cast<float4*>(act + row * C)[cl] = o;
        if (cl == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
    }
}

// dz may be dact itself: a lane reads exactly the elements it later writes.
template <int LPR>
__global__ __launch_bounds__(256) void blg_bwd_narrow_kernel(const float* __restrict__ z, const float* __restrict__ cbias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                              const float* dact, float* dz, float* __restrict__ partial_g,
                                                              float* __restrict__ partial_b, float* __restrict__ partial_c, int64_t rows) {
    constexpr int C = 4 * LPR, RPW = 64 / LPR;
    __shared__ float4 red[WPB][LPR];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, cl = lane % LPR, sub = lane / LPR;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g = ld4(gamma, cl), b = ld4(beta, cl), cb = cbias ? ld4(cbias, cl) : zero;
    float4 ag = zero, ab = zero, ac = zero;
    for (int64_t base = ((int64_t)blockIdx.x * WPB + w) * RPW; base < rows; base += (int64_t)gridDim.x * WPB * RPW) {
        const int64_t row = base + sub;
        const bool live = row < rows;
        const float mean = live ? mean_in[row] : 0.f, rstd = live ? rstd_in[row] : 0.f;
        const float4 v = live ? ld4(z + row * C, cl) : zero, d = live ? ld4(dact + row * C, cl) : zero;
        float4 xh, dn, gy;
        xh.x = (v.x + cb.x - mean) * rstd; xh.y = (v.y + cb.y - mean) * rstd; xh.z = (v.z + cb.z - mean) * rstd; xh.w = (v.w + cb.w - mean) * rstd;
        dn.x = d.x * dyn::gelu_grad(xh.x * g.x + b.x); dn.y = d.y * dyn::gelu_grad(xh.y * g.y + b.y);
        dn.z = d.z * dyn::gelu_grad(xh.z * g.z + b.z); dn.w = d.w * dyn::gelu_grad(xh.w * g.w + b.w);
        gy.x = dn.x * g.x; gy.y = dn.y * g.y; gy.z = dn.z * g.z; gy.w = dn.w * g.w;
        const float s1 = group_sum<LPR>(gy.x + gy.y + gy.z + gy.w) / C;
        const float s2 = group_sum<LPR>(gy.x * xh.x + gy.y * xh.y + gy.z * xh.z + gy.w * xh.w) / C;
        if (!live) continue;     // (d = 0 there: nothing to add)
        ag.x += dn.x * xh.x; ag.y += dn.y * xh.y; ag.z += dn.z * xh.z; ag.w += dn.w * xh.w;
        ab.x += dn.x; ab.y += dn.y; ab.z += dn.z; ab.w += dn.w;
        float4 o;
        o.x = rstd * (gy.x - s1 - xh.x * s2); o.y = rstd * (gy.y - s1 - xh.y * s2);
        o.z = rstd * (gy.z - s1 - xh.z * s2); o.w = rstd * (gy.w - s1 - xh.w * s2);
        ac.x += o.x; ac.y += o.y; ac.z += o.z; ac.w += o.w;
        reinterpret_cast<float4*>(dz + row * C)[cl] = o;
    }
    for (int pass = 0; pass < 3; ++pass) {
        float* partial = pass == 0 ? partial_g : pass == 1 ? partial_b : partial_c;
        if (!partial) continue;                                      // uniform over the grid
        const float4 t0 = across_groups<LPR>(pass == 0 ? ag : pass == 1 ? ab : ac);
        __syncthreads();
        if (lane < LPR) red[w][lane] = t0;
        __syncthreads();
        if (w == 0 && lane < LPR) {
            float4 t = red[0][lane];
#pragma unroll
            for (int k = 1; k < WPB; ++k) { t.x += red[k][lane].x; t.y += red[k][lane].y; t.z += red[k][lane].z; t.w += red[k][lane].w; }
            reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * C)[lane] = t;
        }
    }
}

}  // namespace

extern "C" int dyn_bias_layernorm_gelu_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float* act,
                                           float* mean, float* rstd, int64_t rows, int64_t C, float eps, void* stream) {
    DYN_REQUIRE(z && gamma && beta && act && mean && rstd && rows >= 0 && C > 0 && (C % 256 == 0 || C == 64 || C == 128), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_fwd: bad arguments (C=%lld must be a multiple of 256, or 64 or 128)", (long long)C);
    DYN_REQUIRE(aligned16(z) && aligned16(conv_bias) && aligned16(gamma) && aligned16(beta) && aligned16(act), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_fwd: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    dim3 grid(dyn::row_blocks(rows, WPB, 2048)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    if (C < 256) {               // 64 / 128 channels: several rows per wave
        dim3 gn(dyn::row_blocks(rows, WPB * (C == 64 ? 4 : 2), 2048));
        if (C == 64) hipLaunchKernelGGL(blg_fwd_narrow_kernel<16>, gn, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps);
        else hipLaunchKernelGGL(blg_fwd_narrow_kernel<32>, gn, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps);
    } else if (!dyn::dispatch_nv<1, 2, 3, 4>(C, [&](auto nv) {
                   hipLaunchKernelGGL(blg_fwd_kernel<decltype(nv)::value>, grid, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps);
               })) {
        dyn::set_error("dyn_bias_layernorm_gelu_fwd: unsupported C=%lld (need C in {256,512,768,1024})", (long long)C);
        return DYN_E_UNSUPPORTED;
    }
    return dyn::check_launch("dyn_bias_layernorm_gelu_fwd");
}

extern "C" int64_t dyn_bias_layernorm_gelu_bwd_workspace_bytes(int64_t rows, int64_t C) {
    return (int64_t)3 * dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS) * C * (int64_t)sizeof(float);
}

extern "C" int dyn_bias_layernorm_gelu_bwd(const float* z, const float* conv_bias, const float* gamma, const float* beta,
                                           const float* mean, const float* rstd, const float* dact, float* dz, float* dgamma,
                                           float* dbeta, float* dconv_bias, float wgrad_beta, int64_t rows, int64_t C,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(z && gamma && beta && mean && rstd && dact && dz && rows >= 0 && C > 0 && (C % 256 == 0 || C == 64 || C == 128), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_bwd: bad arguments (C=%lld must be a multiple of 256, or 64 or 128)", (long long)C);
    DYN_REQUIRE(aligned16(z) && aligned16(conv_bias) && aligned16(gamma) && aligned16(beta) && aligned16(dact) && aligned16(dz), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_bwd: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    const int nb = dyn::row_blocks(C < 256 ? dyn::cdiv(rows, C == 64 ? 4 : 2) : rows, WPB, MAX_BWD_BLOCKS);     // narrow: 4 or 2 rows per wave, so fewer workgroups
    const int64_t need = dyn_bias_layernorm_gelu_bwd_workspace_bytes(rows, C);
    DYN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need, DYN_E_WORKSPACE,
                "dyn_bias_layernorm_gelu_bwd: workspace too small");
    float* pg = dyn::partials_alloc(workspace, need);       // the workspace, or the open deferral context's arena
    float* pb = pg + (int64_t)nb * C;
    float* pc = pb + (int64_t)nb * C;
    float* wg = dgamma ? pg : nullptr;
    float* wb = dbeta ? pb : nullptr;
    float* wc = dconv_bias ? pc : nullptr;
    dim3 grid(nb), blk(256);
    hipStream_t st = (hipStream_t)stream;
    if (C == 64) hipLaunchKernelGGL(blg_bwd_narrow_kernel<16>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows);
    else if (C == 128) hipLaunchKernelGGL(blg_bwd_narrow_kernel<32>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows);
    else if (!dyn::dispatch_nv<1, 2, 3, 4>(C, [&](auto nv) {
                 hipLaunchKernelGGL(blg_bwd_kernel<decltype(nv)::value>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows);
             })) {
        dyn::set_error("dyn_bias_layernorm_gelu_bwd: unsupported C=%lld (need C in {256,512,768,1024})", (long long)C);
        return DYN_E_UNSUPPORTED;
    }
    if (dgamma && dbeta) dyn::reduce_pair_or_defer(pg, dgamma, pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    else {
        if (dgamma) dyn::reduce_or_defer(pg, dgamma, (int64_t)nb, C, wgrad_beta, st);
        if (dbeta) dyn::reduce_or_defer(pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    }
    if (dconv_bias) dyn::reduce_or_defer(pc, dconv_bias, (int64_t)nb, C, wgrad_beta, st);
    return dyn::check_launch("dyn_bias_layernorm_gelu_bwd");
}
