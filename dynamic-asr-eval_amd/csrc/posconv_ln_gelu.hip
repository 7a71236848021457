// One layer of Data2Vec-Audio's positional conv stack after its grouped GEMM (transformers Data2VecAudioPositionalConvLayer.forward:
// conv -> transpose -> LayerNorm(H, elementwise_affine=False) -> transpose -> GELU), in one pass each way, reading and writing the
// GROUP-MAJOR layouts the grouped GEMMs work in so that no pack / unpack launch stands between two layers:
//   forward:  row (b, t) = the G segments yg[b, g, t, 0:cg] side by side + conv bias; act = gelu((row - mean) * rstd).  Written as the
//             token-major activation [B, T, H] and / or as the NEXT layer's packed input [B, G, T + 2 pad, cg], whose 2 pad zero rows per
//             (b, g) this kernel writes as well (no memset, no group_pack).  mean / rstd [B T] kept for the backward; yg is left alone.
//   backward: xhat is RECOMPUTED from yg, bias, mean, rstd; dn = dact * gelu'(xhat); dyg = rstd * (dn - mean(dn) - xhat * mean(dn * xhat))
//             written in the [B, G, T, cg] layout the weight- and data-gradient GEMMs read; dbias = column sums of dyg.
// Rows t >= *valid (a zero-padded length bucket; device scalar read when the kernel runs) are zeros in every output: the rows just past
// the utterance see valid rows through the conv, so they are NOT zero on their own, and the next layer must see its zero padding there.
// The row kernels are layernorm_row.h's (one wave64 per row, NV = H / 256 float4 per lane; cg % 4 == 0: a float4 never straddles two
// segments); the column sum is accumulated per workgroup in registers, written as one partial row and summed by the fixed-order reducer.
// Nothing here synchronises or allocates.
#include "common.h"
#include "gelu.h"
#include "layernorm_row.h"
#include "reduce.h"

namespace {

using dyn::aligned16;
using dyn::ld4;
using dyn::st4;
using dyn::valid_rows;
constexpr int WPB = dyn::ROW_WPB;
constexpr int MAX_BWD_BLOCKS = 1024;

// Rows walked: B * (T + 2 pad) when the packed output is wanted (the pad rows are written as zeros), else B * T.
template <int NV>
__global__ __launch_bounds__(256) void pclg_fwd_kernel(const float* __restrict__ yg, const float* __restrict__ bias, float* __restrict__ act,
                                                        float* __restrict__ xg_next, float* __restrict__ mean_out,
                                                        float* __restrict__ rstd_out, int64_t B, int64_t T, int64_t Tg, int G, int cg,
                                                        int64_t pad, float eps, const int32_t* __restrict__ valid) {
    constexpr int H = NV * 256;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t Tv = valid_rows(valid, T);
    const int64_t p0 = xg_next ? pad : 0, Tw = T + 2 * p0, Tp = T + 2 * pad;
    float4 cb[NV];
    int gi[NV], ci[NV];          // this lane's float4 j: group and channel inside the group
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int ch = 4 * (lane + 64 * j);
        cb[j] = ld4(bias + ch);
        gi[j] = ch / cg;
        ci[j] = ch % cg;
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < B * Tw; row += (int64_t)gridDim.x * WPB) {
        const int64_t b = row / Tw, tp = row % Tw, t = tp - p0;
        if (t < 0 || t >= T) {   // a padding row of the packed output (only walked when xg_next is given)
#pragma unroll
            for (int j = 0; j < NV; ++j) st4(xg_next + ((b * G + gi[j]) * Tp + tp) * cg + ci[j], zero);
            continue;
        }
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = ld4(yg + ((b * G + gi[j]) * Tg + t) * cg + ci[j]);
            dyn::add4(v[j], cb[j]);
            s += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        float mean, rstd;
        dyn::row_mean_rstd(v, s, eps, mean, rstd);
        const bool live = t < Tv;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o = zero;
            if (live) {
                o.x = dyn::gelu_f((v[j].x - mean) * rstd);
                o.y = dyn::gelu_f((v[j].y - mean) * rstd);
                o.z = dyn::gelu_f((v[j].z - mean) * rstd);
                o.w = dyn::gelu_f((v[j].w - mean) * rstd);
            }
            if (act) st4(act + (b * T + t) * H + 4 * (lane + 64 * j), o);
            if (xg_next) st4(xg_next + ((b * G + gi[j]) * Tp + tp) * cg + ci[j], o);
        }
        if (lane == 0) {
            mean_out[b * T + t] = mean;
            rstd_out[b * T + t] = rstd;
        }
    }
}

// partial [gridDim.x, H]: this workgroup's column sums of dyg (a null pointer: not wanted).
template <int NV>
__global__ __launch_bounds__(256) void pclg_bwd_kernel(const float* __restrict__ yg, const float* __restrict__ bias,
                                                        const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                        const float* __restrict__ dact, float* __restrict__ dyg, float* __restrict__ partial,
                                                        int64_t B, int64_t T, int64_t Tg, int G, int cg, const int32_t* __restrict__ valid) {
    constexpr int H = NV * 256;
    __shared__ float4 red[WPB][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t Tv = valid_rows(valid, T);
    float4 cb[NV], ac[NV];
    int gi[NV], ci[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int ch = 4 * (lane + 64 * j);
        cb[j] = ld4(bias + ch);
        gi[j] = ch / cg;
        ci[j] = ch % cg;
        ac[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < B * T; row += (int64_t)gridDim.x * WPB) {
        const int64_t b = row / T, t = row % T;
        if (t >= Tv) {           // past the utterance: no gradient
#pragma unroll
            for (int j = 0; j < NV; ++j) st4(dyg + ((b * G + gi[j]) * T + t) * cg + ci[j], make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const float mean = mean_in[row], rstd = rstd_in[row];
        float4 xh[NV], dn[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 v = ld4(yg + ((b * G + gi[j]) * Tg + t) * cg + ci[j]);
            const float4 d = ld4(dact + row * H + 4 * (lane + 64 * j));
            dyn::add4(v, cb[j]);
            xh[j] = dyn::xhat4(v, mean, rstd);
            dn[j].x = d.x * dyn::gelu_grad(xh[j].x); dn[j].y = d.y * dyn::gelu_grad(xh[j].y);
            dn[j].z = d.z * dyn::gelu_grad(xh[j].z); dn[j].w = d.w * dyn::gelu_grad(xh[j].w);
            dyn::bwd_lane_sums(dn[j], xh[j], s1, s2);
        }
        dyn::bwd_row_means<NV>(s1, s2);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 o = dyn::bwd4(dn[j], xh[j], rstd, s1, s2);
            dyn::add4(ac[j], o);
            st4(dyg + ((b * G + gi[j]) * T + t) * cg + ci[j], o);
        }
    }
    if (partial) dyn::combine_waves(ac, red, partial + (int64_t)blockIdx.x * H);     // null or not: uniform over the grid
}

// The shape rules both entries share; `who` names the entry in the message.
inline int check_shape(const char* who, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G) {
    DYN_REQUIRE(B >= 0 && T >= 0 && Tg >= T, DYN_E_ARG, "%s: bad dimensions (B=%lld, T=%lld, Tg=%lld; need Tg >= T)", who, (long long)B,
                (long long)T, (long long)Tg);
    DYN_REQUIRE(H > 0 && H % 256 == 0 && H <= 1024, DYN_E_ARG, "%s: H=%lld must be a multiple of 256 up to 1024", who, (long long)H);
    DYN_REQUIRE(G > 0 && H % G == 0 && (H / G) % 4 == 0, DYN_E_ARG, "%s: H / G = %lld / %lld channels per group must be a whole multiple of 4",
                who, (long long)H, (long long)G);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_posconv_ln_gelu_fwd(const float* yg, const float* bias, float* act, float* xg_next, float* mean, float* rstd, int64_t B,
                                       int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t pad, float eps, const int32_t* valid_rows,
                                       void* stream) {
    DYN_REQUIRE(yg && bias && mean && rstd && (act || xg_next), DYN_E_ARG,
                "dyn_posconv_ln_gelu_fwd: null argument (yg, bias, mean, rstd and at least one of act / xg_next are required)");
    const int rc = check_shape("dyn_posconv_ln_gelu_fwd", B, T, Tg, H, G);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(pad >= 0, DYN_E_ARG, "dyn_posconv_ln_gelu_fwd: pad=%lld must not be negative", (long long)pad);
    DYN_REQUIRE(aligned16(yg) && aligned16(bias) && aligned16(act) && aligned16(xg_next), DYN_E_ARG,
                "dyn_posconv_ln_gelu_fwd: operands must be 16-byte aligned");
    const int64_t rows = B * (T + (xg_next ? 2 * pad : 0));
    if (rows == 0) return DYN_OK;
    dim3 grid(dyn::row_blocks(rows, WPB, 2048)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G);
    dyn::dispatch_nv<1, 2, 3, 4>(H, [&](auto nv) {           // check_shape admits no other H
        hipLaunchKernelGGL(pclg_fwd_kernel<decltype(nv)::value>, grid, blk, 0, st, yg, bias, act, xg_next, mean, rstd, B, T, Tg, g, cg, pad, eps, valid_rows);
    });
    return dyn::check_launch("dyn_posconv_ln_gelu_fwd");
}

extern "C" int64_t dyn_posconv_ln_gelu_bwd_workspace_bytes(int64_t rows, int64_t H) {
    return (int64_t)dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS) * H * (int64_t)sizeof(float);
}

extern "C" int dyn_posconv_ln_gelu_bwd(const float* yg, const float* bias, const float* mean, const float* rstd, const float* dact, float* dyg,
                                       float* dbias, float wgrad_beta, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G,
                                       const int32_t* valid_rows, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(yg && bias && mean && rstd && dact && dyg, DYN_E_ARG,
                "dyn_posconv_ln_gelu_bwd: null argument (yg, bias, mean, rstd, dact and dyg are required; only dbias may be null)");
    const int rc = check_shape("dyn_posconv_ln_gelu_bwd", B, T, Tg, H, G);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(yg) && aligned16(bias) && aligned16(dact) && aligned16(dyg), DYN_E_ARG,
                "dyn_posconv_ln_gelu_bwd: operands must be 16-byte aligned");
    const int64_t rows = B * T;
    if (rows == 0) return DYN_OK;
    const int nb = dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS);
    float* partial = nullptr;
    if (dbias) {
        const int64_t need = dyn_posconv_ln_gelu_bwd_workspace_bytes(rows, H);
        DYN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need, DYN_E_WORKSPACE,
                    "dyn_posconv_ln_gelu_bwd: workspace too small");
        partial = dyn::partials_alloc(workspace, need);          // the workspace, or the open deferral context's arena
    }
    dim3 grid(nb), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G);
    dyn::dispatch_nv<1, 2, 3, 4>(H, [&](auto nv) {           // check_shape admits no other H
        hipLaunchKernelGGL(pclg_bwd_kernel<decltype(nv)::value>, grid, blk, 0, st, yg, bias, mean, rstd, dact, dyg, partial, B, T, Tg, g, cg, valid_rows);
    });
    if (dbias) dyn::reduce_or_defer(partial, dbias, (int64_t)nb, H, wgrad_beta, st);
    return dyn::check_launch("dyn_posconv_ln_gelu_bwd");
}
