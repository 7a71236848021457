// LayerNorm over a NARROW row (rows x C, C % 4 == 0, C <= 256): Wav2Vec2-BERT's `feature_projection.layer_norm` over the 160 stacked
// filter-bank channels (transformers modeling_wav2vec2_bert.py, Wav2Vec2BertFeatureProjection.forward: `self.layer_norm(hidden_states)`
// and its autograd).  Every other LayerNorm entry of the library holds NV * 256 channels per wave (layernorm_row.h); here one wave64 holds
// one row as well, but only its first C / 4 lanes own a float4 (40 of 64 at C = 160), the others carry zeros through the reductions.
// The statistics are the centred two-reduction form of layernorm_row.h (mean first, then the mean of (x - mean)^2): a row of filter-bank
// features far from zero does not cancel.  Backward: dgamma / dbeta are added per lane over the rows of a workgroup, its waves are added in
// wave order into ONE partial row, and the fixed-order reducers (reduce.h; deferrable) sum the partial rows: no atomics, bit-reproducible.
// dx is optional: the row is data (filter-bank features), nothing upstream needs its gradient.
#include "common.h"
#include "layernorm_row.h"
#include "reduce.h"

namespace {

using dyn::ld4;
using dyn::st4;
constexpr int WPB = dyn::ROW_WPB;
constexpr int MAX_BWD_BLOCKS = 256;

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__global__ __launch_bounds__(256) void narrow_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ y,
                                                             float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows,
                                                             int C, float eps) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool own = lane < C / 4;
    const float4 g = own ? ld4(gamma, lane) : zero4();
    const float4 b = (own && beta) ? ld4(beta, lane) : zero4();
    const float inv = 1.f / (float)C;
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < rows; row += (int64_t)gridDim.x * WPB) {
        const float4 v = own ? ld4(x + row * C, lane) : zero4();
        const float mean = dyn::wave_sum(v.x + v.y + v.z + v.w) * inv;
        float q = 0.f;
        if (own) {
            const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
            q = a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        }
        const float rstd = rsqrtf(dyn::wave_sum(q) * inv + eps);
        if (own) st4(y + row * C, dyn::affine4(v, mean, rstd, g, b), lane);
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
    }
}

// partial_g / partial_b [gridDim.x, C]: this workgroup's sums of dy * xhat and dy over its rows; dx (may be null) = rstd * (gy - mean(gy) - xhat mean(gy xhat))
__global__ __launch_bounds__(256) void narrow_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                             const float* __restrict__ dy, float* __restrict__ dx,
                                                             float* __restrict__ partial_g, float* __restrict__ partial_b, int64_t rows, int C) {
    __shared__ float4 red[2][WPB][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool own = lane < C / 4;
    const float4 g = own ? ld4(gamma, lane) : zero4();
    const float inv = 1.f / (float)C;
    float4 ag = zero4(), ab = zero4();
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < rows; row += (int64_t)gridDim.x * WPB) {
        const float mean = mean_in[row], rstd = rstd_in[row];
        float4 d = zero4(), xh = zero4();
        if (own) {
            d = ld4(dy + row * C, lane);
            xh = dyn::xhat4(ld4(x + row * C, lane), mean, rstd);
        }
        dyn::addmul4(ag, d, xh);
        dyn::add4(ab, d);
        if (dx) {                                  // uniform over the launch
            const float4 gy = dyn::mul4(d, g);
            float s1 = 0.f, s2 = 0.f;
            dyn::bwd_lane_sums(gy, xh, s1, s2);
            s1 = dyn::wave_sum(s1) * inv;
            s2 = dyn::wave_sum(s2) * inv;
            if (own) st4(dx + row * C, dyn::bwd4(gy, xh, rstd, s1, s2), lane);
        }
    }
    red[0][w][lane] = ag;
    red[1][w][lane] = ab;
    __syncthreads();
    if (w == 0 && own) {
        float4 tg = red[0][0][lane], tb = red[1][0][lane];
#pragma unroll
        for (int k = 1; k < WPB; ++k) {
            dyn::add4(tg, red[0][k][lane]);
            dyn::add4(tb, red[1][k][lane]);
        }
        st4(partial_g + (int64_t)blockIdx.x * C, tg, lane);
        st4(partial_b + (int64_t)blockIdx.x * C, tb, lane);
    }
}

int check_c(const char* who, int64_t rows, int64_t C) {
    DYN_REQUIRE(rows >= 0, DYN_E_ARG, "%s: rows=%lld", who, (long long)rows);
    DYN_REQUIRE(C >= 4 && C <= 256 && C % 4 == 0, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (a multiple of 4 from 4 to 256; wider rows: dyn_layernorm_*)",
                who, (long long)C);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_narrow_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                        int64_t rows, int64_t C, float eps, void* stream) {
    DYN_REQUIRE(x && gamma && y && mean && rstd, DYN_E_ARG, "dyn_narrow_layernorm_fwd: null pointer");
    if (int rc = check_c("dyn_narrow_layernorm_fwd", rows, C)) return rc;
    DYN_REQUIRE(dyn::aligned16(x) && dyn::aligned16(gamma) && dyn::aligned16(beta) && dyn::aligned16(y), DYN_E_ARG,
                "dyn_narrow_layernorm_fwd: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    hipLaunchKernelGGL(narrow_ln_fwd_kernel, dim3(dyn::row_blocks(rows, WPB, 2048)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, mean,
                       rstd, rows, (int)C, eps);
    return dyn::check_launch("dyn_narrow_layernorm_fwd");
}

extern "C" int64_t dyn_narrow_layernorm_bwd_workspace_bytes(int64_t rows, int64_t C) {
    return (int64_t)2 * dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS) * C * (int64_t)sizeof(float);
}

extern "C" int dyn_narrow_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                                        float* dgamma, float* dbeta, float wgrad_beta, int64_t rows, int64_t C, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(x && gamma && mean && rstd && dy, DYN_E_ARG, "dyn_narrow_layernorm_bwd: null pointer");
    DYN_REQUIRE(dx || dgamma || dbeta, DYN_E_ARG, "dyn_narrow_layernorm_bwd: no output is wanted");
    if (int rc = check_c("dyn_narrow_layernorm_bwd", rows, C)) return rc;
    DYN_REQUIRE(dyn::aligned16(x) && dyn::aligned16(gamma) && dyn::aligned16(dy) && dyn::aligned16(dx), DYN_E_ARG,
                "dyn_narrow_layernorm_bwd: operands must be 16-byte aligned");
    const int nb = dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS);
    const int64_t bytes = (int64_t)2 * nb * C * (int64_t)sizeof(float);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "dyn_narrow_layernorm_bwd: workspace too small (%lld bytes needed)",
                (long long)bytes);
    if (rows == 0) return DYN_OK;                  // no row: nothing to add to the gradients
    hipStream_t st = (hipStream_t)stream;
    float* pg = dyn::partials_alloc(workspace, bytes);
    float* pb = pg + (int64_t)nb * C;
    hipLaunchKernelGGL(narrow_ln_bwd_kernel, dim3(nb), dim3(256), 0, st, x, gamma, mean, rstd, dy, dx, pg, pb, rows, (int)C);
    if (dgamma && dbeta) dyn::reduce_pair_or_defer(pg, dgamma, pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    else {
        if (dgamma) dyn::reduce_or_defer(pg, dgamma, (int64_t)nb, C, wgrad_beta, st);
        if (dbeta) dyn::reduce_or_defer(pb, dbeta, (int64_t)nb, C, wgrad_beta, st);
    }
    return dyn::check_launch("dyn_narrow_layernorm_bwd");
}
