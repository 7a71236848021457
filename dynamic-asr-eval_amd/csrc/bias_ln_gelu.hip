// Conv bias + LayerNorm over channels + exact GELU in one pass each way: the feature-extractor layer of the layer-norm wav2vec2
// layout (`feat_extract_norm: "layer"`, `conv_bias: true`; transformers Wav2Vec2LayerNormConvLayer.forward: conv -> transpose ->
// LayerNorm(C) -> transpose -> GELU), which runs on all seven layers and so on the largest activations of the model.
//   forward:  act = gelu(LN(z + conv_bias));  mean / rstd [rows] kept for the backward; z (the raw conv output) is left alone
//   backward: xhat and n = xhat * gamma + beta are RECOMPUTED from z, mean, rstd (the normalised tensor is never stored),
//             dn = dact * gelu'(n), dz = LayerNorm backward of dn, dgamma = sum dn * xhat, dbeta = sum dn, dconv_bias = sum dz.
// As in norm.hip: one wave64 per row, 16-B accesses, the row in registers (NV = C / 256 float4 per lane and tensor), row statistics
// by wavefront reductions; the three column sums are accumulated per workgroup in registers, written as partial rows and summed
// by the fixed-order reducers (reduce.h; deferrable): no atomics, bit-reproducible.  Nothing here synchronises or allocates.
// Registers at C = 512 (NV = 2): the backward holds z, dact (16 floats), three accumulators (24) and gamma, beta, bias (24) per lane,
// 117 VGPRs = 4 waves per SIMD; its LDS is the 4 KiB combine buffer.  HBM-bound, so the backward spreads the rows over up to 1024
// workgroups of 4 rows in flight (4 waves on every SIMD at the 52428-row layer) at 3 partial rows of C floats per workgroup.
#include "common.h"
#include "gelu.h"
#include "reduce.h"

namespace {

constexpr int WPB = 4;           // waves (rows in flight) per workgroup
constexpr int MAX_BWD_BLOCKS = 1024;

__device__ __forceinline__ float4 ld4(const float* p, int i) { return reinterpret_cast<const float4*>(p)[i]; }

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
            v[j].x += cb[j].x; v[j].y += cb[j].y; v[j].z += cb[j].z; v[j].w += cb[j].w;
            s += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        const float mean = dyn::wave_sum(s) / C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
            q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        }
        const float rstd = rsqrtf(dyn::wave_sum(q) / C + eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o;
            o.x = dyn::gelu_f((v[j].x - mean) * rstd * g[j].x + b[j].x);
            o.y = dyn::gelu_f((v[j].y - mean) * rstd * g[j].y + b[j].y);
            o.z = dyn::gelu_f((v[j].z - mean) * rstd * g[j].z + b[j].z);
            o.w = dyn::gelu_f((v[j].w - mean) * rstd * g[j].w + b[j].w);
            reinterpret_cast<float4*>(act + row * C)[lane + 64 * j] = o;
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
            s1 += gy[j].x + gy[j].y + gy[j].z + gy[j].w;
            s2 += gy[j].x * xh[j].x + gy[j].y * xh[j].y + gy[j].z * xh[j].z + gy[j].w * xh[j].w;
        }
        s1 = dyn::wave_sum(s1) / C;
        s2 = dyn::wave_sum(s2) / C;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o;
            o.x = rstd * (gy[j].x - s1 - xh[j].x * s2);
            o.y = rstd * (gy[j].y - s1 - xh[j].y * s2);
            o.z = rstd * (gy[j].z - s1 - xh[j].z * s2);
            o.w = rstd * (gy[j].w - s1 - xh[j].w * s2);
            ac[j].x += o.x; ac[j].y += o.y; ac[j].z += o.z; ac[j].w += o.w;
            reinterpret_cast<float4*>(dz + row * C)[lane + 64 * j] = o;
        }
    }
    // Combine the 4 waves' column sums in wave order, then write this workgroup's partial rows.
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        for (int pass = 0; pass < 3; ++pass) {
            float* partial = pass == 0 ? partial_g : pass == 1 ? partial_b : partial_c;
            if (!partial) continue;                                  // uniform over the grid
            __syncthreads();
            red[w][lane] = pass == 0 ? ag[j] : pass == 1 ? ab[j] : ac[j];
            __syncthreads();
            if (w == 0) {
                float4 t = red[0][lane];
#pragma unroll
                for (int k = 1; k < WPB; ++k) { t.x += red[k][lane].x; t.y += red[k][lane].y; t.z += red[k][lane].z; t.w += red[k][lane].w; }
                reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * C)[lane + 64 * j] = t;
            }
        }
    }
}

inline int bwd_blocks(int64_t rows) {
    int64_t g = dyn::cdiv(rows, WPB);
    if (g > MAX_BWD_BLOCKS) g = MAX_BWD_BLOCKS;
    if (g < 1) g = 1;
    return (int)g;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" int dyn_bias_layernorm_gelu_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float* act,
                                           float* mean, float* rstd, int64_t rows, int64_t C, float eps, void* stream) {
    DYN_REQUIRE(z && gamma && beta && act && mean && rstd && rows >= 0 && C > 0 && C % 256 == 0, DYN_E_ARG,
                "dyn_bias_layernorm_gelu_fwd: bad arguments (C=%lld must be a multiple of 256)", (long long)C);
    DYN_REQUIRE(aligned16(z) && aligned16(conv_bias) && aligned16(gamma) && aligned16(beta) && aligned16(act), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_fwd: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    int64_t gq = dyn::cdiv(rows, WPB);
    if (gq > 2048) gq = 2048;
    dim3 grid((unsigned)gq), blk(256);
    hipStream_t st = (hipStream_t)stream;
    switch (C / 256) {
        case 1: hipLaunchKernelGGL(blg_fwd_kernel<1>, grid, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps); break;
        case 2: hipLaunchKernelGGL(blg_fwd_kernel<2>, grid, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps); break;
        case 3: hipLaunchKernelGGL(blg_fwd_kernel<3>, grid, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps); break;
        case 4: hipLaunchKernelGGL(blg_fwd_kernel<4>, grid, blk, 0, st, z, conv_bias, gamma, beta, act, mean, rstd, rows, eps); break;
        default: dyn::set_error("dyn_bias_layernorm_gelu_fwd: unsupported C=%lld (need C in {256,512,768,1024})", (long long)C); return DYN_E_UNSUPPORTED;
    }
    return dyn::check_launch("dyn_bias_layernorm_gelu_fwd");
}

extern "C" int64_t dyn_bias_layernorm_gelu_bwd_workspace_bytes(int64_t rows, int64_t C) {
    return (int64_t)3 * bwd_blocks(rows) * C * (int64_t)sizeof(float);
}

extern "C" int dyn_bias_layernorm_gelu_bwd(const float* z, const float* conv_bias, const float* gamma, const float* beta,
                                           const float* mean, const float* rstd, const float* dact, float* dz, float* dgamma,
                                           float* dbeta, float* dconv_bias, float wgrad_beta, int64_t rows, int64_t C,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(z && gamma && beta && mean && rstd && dact && dz && rows >= 0 && C > 0 && C % 256 == 0, DYN_E_ARG,
                "dyn_bias_layernorm_gelu_bwd: bad arguments (C=%lld must be a multiple of 256)", (long long)C);
    DYN_REQUIRE(aligned16(z) && aligned16(conv_bias) && aligned16(gamma) && aligned16(beta) && aligned16(dact) && aligned16(dz), DYN_E_ARG,
                "dyn_bias_layernorm_gelu_bwd: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    const int nb = bwd_blocks(rows);
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
    switch (C / 256) {
        case 1: hipLaunchKernelGGL(blg_bwd_kernel<1>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows); break;
        case 2: hipLaunchKernelGGL(blg_bwd_kernel<2>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows); break;
        case 3: hipLaunchKernelGGL(blg_bwd_kernel<3>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows); break;
        case 4: hipLaunchKernelGGL(blg_bwd_kernel<4>, grid, blk, 0, st, z, conv_bias, gamma, beta, mean, rstd, dact, dz, wg, wb, wc, rows); break;
        default: dyn::set_error("dyn_bias_layernorm_gelu_bwd: unsupported C=%lld (need C in {256,512,768,1024})", (long long)C); return DYN_E_UNSUPPORTED;
    }
    if (dgamma && dbeta) dyn::reduce_pair_or_defer(pg, dgamma, pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    else {
        if (dgamma) dyn::reduce_or_defer(pg, dgamma, (int64_t)nb, C, wgrad_beta, st);
        if (dbeta) dyn::reduce_or_defer(pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    }
    if (dconv_bias) dyn::reduce_or_defer(pc, dconv_bias, (int64_t)nb, C, wgrad_beta, st);
    return dyn::check_launch("dyn_bias_layernorm_gelu_bwd");
}
