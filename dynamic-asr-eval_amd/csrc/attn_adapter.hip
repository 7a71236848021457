// The bottleneck adapter MMS puts behind every encoder layer (transformers Wav2Vec2AttnAdapterLayer), one launch forward and two backward:
//   forward:   y = x + W2 relu(W1 LayerNorm(x) + b1) + b2, x [M, H], W1 [A, H], W2 [H, A].  The normalised row lives in registers only;
//              mean / rstd [M] and the post-ReLU bottleneck a [M, A] are written when the caller wants them for the backward.  y may be x.
//   backward:  stage 1 (one wave per row): da = W2^T dy, du = da where a > 0 (else 0), dn = W1^T du, dx = dy + LayerNorm'(dn) out of
//              place; du [M, A] goes to the workspace; the column sums dgamma = sum dn xhat, dbeta = sum dn, db2 = sum dy, db1 = sum du are
//              accumulated per workgroup in registers and written as partial rows.
//              stage 2 (one launch): the two outer-product sums dW1[a, c] = sum_r du[r, a] n[r, c] (n recomputed from x, mean, rstd, gamma,
//              beta) and dW2[c, a] = sum_r dy[r, c] a[r, a], every output element owned by ONE thread group: a workgroup holds 256 columns x
//              4 bottleneck units, its 16 waves walk the rows r = w, w + 16, ... in order and are combined through LDS in wave order; further
//              workgroups of the same launch sum the partial rows of the four vectors in the order reduce.h uses.  No atomics: the same call
//              twice gives the same bits, and a row whose dy is all zeros adds exact zeros to every sum and gets an exact-zero dx.
// Staging: neither W1 nor W2 is staged in LDS.  Both are read through the vector L1 / L2 with 16-B loads: the 4 waves of a workgroup work
// on 4 neighbouring rows and read the same weight addresses at nearly the same time, and at the M of one utterance (a few hundred rows over
// 256 CUs) a workgroup sees a handful of rows, too few to pay for filling 80 KiB of LDS first.  LDS holds the cross-wave combines only.
// The LayerNorm of the two row kernels is layernorm_row.h's (the row in registers, NV = H / 256 float4 per lane).
// Nothing here synchronises or allocates.
#include "common.h"
#include "layernorm_row.h"

namespace {

using dyn::aligned16;
using dyn::dot4;
using dyn::ld4;
using dyn::st4;
constexpr int WPB = dyn::ROW_WPB;    // waves (rows in flight) per workgroup of the two row kernels
constexpr int MAX_BWD_BLOCKS = 512;  // partial rows of the backward's column sums
constexpr int GW = 16;               // waves per workgroup of the second backward stage
constexpr int DB1_COLS = 64;         // columns the db1 partials take in a partial row (A <= 64)

// x and y may be the same buffer: a wave holds its whole row before it writes it.
template <int NV>
__global__ __launch_bounds__(256) void adapter_fwd_kernel(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ W1, const float* __restrict__ b1,
                                                           const float* __restrict__ W2, const float* __restrict__ b2, float* y,
                                                           float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                           float* __restrict__ a_out, int64_t M, int A, float eps) {
    constexpr int H = NV * 256;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float bias1 = lane < A ? b1[lane] : 0.f;
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < M; row += (int64_t)gridDim.x * WPB) {
        float4 v[NV], n[NV];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = ld4(x + row * H + 4 * (lane + 64 * j));
            sum += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        // dyn::row_mean_rstd(v, sum, eps, mean, rstd), spelt out: through the call the compiler fuses other multiply-adds of the NV = 3 and 5
        // instances, which changes the bits of y there
        const float mean = dyn::wave_sum(sum) / H;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
            q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        }
        const float rstd = rsqrtf(dyn::wave_sum(q) / H + eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 gm = ld4(gamma + 4 * (lane + 64 * j)), bt = ld4(beta + 4 * (lane + 64 * j));
            n[j].x = (v[j].x - mean) * rstd * gm.x + bt.x; n[j].y = (v[j].y - mean) * rstd * gm.y + bt.y;
            n[j].z = (v[j].z - mean) * rstd * gm.z + bt.z; n[j].w = (v[j].w - mean) * rstd * gm.w + bt.w;
        }
        // down-projection: lane a ends up with unit a (A <= 64), four units per step so their reductions overlap
        float ua = 0.f;
        for (int a0 = 0; a0 < A; a0 += 4) {
            float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* wr = W1 + (int64_t)(a0 + i) * H + 4 * lane;
#pragma unroll
                for (int j = 0; j < NV; ++j) p[i] += dot4(n[j], ld4(wr + 256 * j));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[i] = dyn::wave_sum(p[i]);
                if (lane == a0 + i) ua = fmaxf(p[i] + bias1, 0.f);
            }
        }
        if (a_out && lane < A) a_out[row * A + lane] = ua;
        // up-projection: this lane's 4 NV columns, rows of W2 (A contiguous floats each)
        float4 acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int a0 = 0; a0 < A; a0 += 4) {
            const float4 u = make_float4(__shfl(ua, a0, 64), __shfl(ua, a0 + 1, 64), __shfl(ua, a0 + 2, 64), __shfl(ua, a0 + 3, 64));
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float* wr = W2 + (int64_t)(4 * (lane + 64 * j)) * A + a0;
                acc[j].x += dot4(ld4(wr), u); acc[j].y += dot4(ld4(wr + A), u);
                acc[j].z += dot4(ld4(wr + 2 * A), u); acc[j].w += dot4(ld4(wr + 3 * A), u);
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 b = ld4(b2 + 4 * (lane + 64 * j));
            float4 o;
            o.x = v[j].x + (acc[j].x + b.x); o.y = v[j].y + (acc[j].y + b.y);
            o.z = v[j].z + (acc[j].z + b.z); o.w = v[j].w + (acc[j].w + b.w);
            st4(y + row * H + 4 * (lane + 64 * j), o);
        }
        if (lane == 0) {
            if (mean_out) mean_out[row] = mean;
            if (rstd_out) rstd_out[row] = rstd;
        }
    }
}

// partial [gridDim.x, 3 H + DB1_COLS]: this workgroup's sums of dn * xhat | dn | dy | du (null: no vector gradient is wanted).
// du_out [M, A] (null: dW1 is not wanted).
template <int NV>
__global__ __launch_bounds__(256) void adapter_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ W1, const float* __restrict__ W2,
                                                           const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                           const float* __restrict__ act, const float* __restrict__ dy,
                                                           float* __restrict__ dx, float* __restrict__ du_out, float* __restrict__ partial,
                                                           int64_t M, int A) {
    constexpr int H = NV * 256;
    __shared__ float4 red[WPB][64];
    __shared__ float redu[WPB][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ag[NV], ab[NV], ac[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) ag[j] = ab[j] = ac[j] = zero;
    float au = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < M; row += (int64_t)gridDim.x * WPB) {
        const float mean = mean_in[row], rstd = rstd_in[row];
        float4 d[NV], xh[NV], dn[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            d[j] = ld4(dy + row * H + 4 * (lane + 64 * j));
            const float4 v = ld4(x + row * H + 4 * (lane + 64 * j));
            xh[j].x = (v.x - mean) * rstd; xh[j].y = (v.y - mean) * rstd; xh[j].z = (v.z - mean) * rstd; xh[j].w = (v.w - mean) * rstd;
            dn[j] = zero;
        }
        // da = W2^T dy: lane a ends up with unit a, then the ReLU mask from the saved activation (a > 0; at exactly 0 no gradient)
        float dua = 0.f;
        for (int a0 = 0; a0 < A; a0 += 4) {
            float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float* wr = W2 + (int64_t)(4 * (lane + 64 * j)) * A + a0;
                const float4 w0 = ld4(wr), w1 = ld4(wr + A), w2 = ld4(wr + 2 * A), w3 = ld4(wr + 3 * A);
                p[0] += d[j].x * w0.x + d[j].y * w1.x + d[j].z * w2.x + d[j].w * w3.x;
                p[1] += d[j].x * w0.y + d[j].y * w1.y + d[j].z * w2.y + d[j].w * w3.y;
                p[2] += d[j].x * w0.z + d[j].y * w1.z + d[j].z * w2.z + d[j].w * w3.z;
                p[3] += d[j].x * w0.w + d[j].y * w1.w + d[j].z * w2.w + d[j].w * w3.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[i] = dyn::wave_sum(p[i]);
                if (lane == a0 + i) dua = p[i];
            }
        }
        if (lane < A) {
            if (!(act[row * A + lane] > 0.f)) dua = 0.f;
            if (du_out) du_out[row * A + lane] = dua;
        }
        au += dua;
        for (int a = 0; a < A; ++a) {
            const float s = __shfl(dua, a, 64);
            const float* wr = W1 + (int64_t)a * H + 4 * lane;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float4 w4 = ld4(wr + 256 * j);
                dn[j].x += s * w4.x; dn[j].y += s * w4.y; dn[j].z += s * w4.z; dn[j].w += s * w4.w;
            }
        }
        float s1 = 0.f, s2 = 0.f;
        float4 g[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 gm = ld4(gamma + 4 * (lane + 64 * j));
            ag[j].x += dn[j].x * xh[j].x; ag[j].y += dn[j].y * xh[j].y; ag[j].z += dn[j].z * xh[j].z; ag[j].w += dn[j].w * xh[j].w;
            ab[j].x += dn[j].x; ab[j].y += dn[j].y; ab[j].z += dn[j].z; ab[j].w += dn[j].w;
            ac[j].x += d[j].x; ac[j].y += d[j].y; ac[j].z += d[j].z; ac[j].w += d[j].w;
            g[j].x = dn[j].x * gm.x; g[j].y = dn[j].y * gm.y; g[j].z = dn[j].z * gm.z; g[j].w = dn[j].w * gm.w;
            dyn::bwd_lane_sums(g[j], xh[j], s1, s2);
        }
        dyn::bwd_row_means<NV>(s1, s2);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o;                // dy + dyn::bwd4(): the residual is the addend of bwd4's last multiply, so the expression is spelt out here
            o.x = d[j].x + rstd * (g[j].x - s1 - xh[j].x * s2); o.y = d[j].y + rstd * (g[j].y - s1 - xh[j].y * s2);
            o.z = d[j].z + rstd * (g[j].z - s1 - xh[j].z * s2); o.w = d[j].w + rstd * (g[j].w - s1 - xh[j].w * s2);
            st4(dx + row * H + 4 * (lane + 64 * j), o);
        }
    }
    if (!partial) return;                                            // uniform over the grid
    // The 4 waves' column sums in wave order into this workgroup's partial row.
    float* prow = partial + (int64_t)blockIdx.x * (3 * H + DB1_COLS);
    dyn::combine_waves(ag, red, prow);
    dyn::combine_waves(ab, red, prow + H);
    dyn::combine_waves(ac, red, prow + 2 * H);
    redu[w][lane] = au;
    __syncthreads();
    if (w == 0) {
        float t = redu[0][lane];
#pragma unroll
        for (int k = 1; k < WPB; ++k) t += redu[k][lane];
        prow[3 * H + lane] = t;
    }
}

// Second stage.  Workgroups [0, n_gemm): (column chunk cb of 256, unit chunk ub of 4) of dW1 / dW2; workgroups after them: 64 columns each of
// the partial rows [P, 3 H + DB1_COLS] -> dgamma | dbeta | db2 | db1.  Every output = old + sum (beta = 1).
__global__ __launch_bounds__(1024) void adapter_bwd_sums_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mean_in,
                                                                 const float* __restrict__ rstd_in, const float* __restrict__ act,
                                                                 const float* __restrict__ dy, const float* __restrict__ du,
                                                                 const float* __restrict__ partial, float* dW1, float* dW2, float* dgamma,
                                                                 float* dbeta, float* db2, float* db1, int64_t M, int H, int A, int P,
                                                                 int n_gemm) {
    __shared__ float4 red[GW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x >= n_gemm) {
        const int PW = 3 * H + DB1_COLS;
        const int col = ((int)blockIdx.x - n_gemm) * 64 + lane;       // H % 64 == 0: a workgroup never straddles two outputs
        const int seg = col / H;
        float* out = seg == 0 ? dgamma : seg == 1 ? dbeta : seg == 2 ? db2 : db1;
        const int o = col - seg * H;
        const bool live = out != nullptr && (seg < 3 || o < A);
        float* redf = reinterpret_cast<float*>(&red[0][0]);
        float s = 0.f;
        if (live)
            for (int p = w; p < P; p += GW) s += partial[(int64_t)p * PW + col];
        redf[w * 64 + lane] = s;
        __syncthreads();
        if (w == 0 && live) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < GW; ++k) t += redf[k * 64 + lane];
            out[o] += t;
        }
        return;
    }
    const int ncb = H / 256;
    const int cb = (int)blockIdx.x % ncb, ub = (int)blockIdx.x / ncb;
    const int c0 = 256 * cb + 4 * lane, u0 = 4 * ub;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a1[4] = {zero, zero, zero, zero};      // a1[i] = dW1[u0 + i, c0 .. c0 + 3]
    float4 a2[4] = {zero, zero, zero, zero};      // a2[k] = dW2[c0 + k, u0 .. u0 + 3]
    if (dW1) {
        const float4 gm = ld4(gamma + c0), bt = ld4(beta + c0);
#pragma unroll 4
        for (int64_t r = w; r < M; r += GW) {
            const float4 v = ld4(x + r * H + c0), g = ld4(du + r * A + u0);
            const float mean = mean_in[r], rstd = rstd_in[r];
            float4 n;
            n.x = (v.x - mean) * rstd * gm.x + bt.x; n.y = (v.y - mean) * rstd * gm.y + bt.y;
            n.z = (v.z - mean) * rstd * gm.z + bt.z; n.w = (v.w - mean) * rstd * gm.w + bt.w;
            a1[0].x += g.x * n.x; a1[0].y += g.x * n.y; a1[0].z += g.x * n.z; a1[0].w += g.x * n.w;
            a1[1].x += g.y * n.x; a1[1].y += g.y * n.y; a1[1].z += g.y * n.z; a1[1].w += g.y * n.w;
            a1[2].x += g.z * n.x; a1[2].y += g.z * n.y; a1[2].z += g.z * n.z; a1[2].w += g.z * n.w;
            a1[3].x += g.w * n.x; a1[3].y += g.w * n.y; a1[3].z += g.w * n.z; a1[3].w += g.w * n.w;
        }
    }
    if (dW2) {
#pragma unroll 4
        for (int64_t r = w; r < M; r += GW) {
            const float4 d = ld4(dy + r * H + c0), u = ld4(act + r * A + u0);
            a2[0].x += d.x * u.x; a2[0].y += d.x * u.y; a2[0].z += d.x * u.z; a2[0].w += d.x * u.w;
            a2[1].x += d.y * u.x; a2[1].y += d.y * u.y; a2[1].z += d.y * u.z; a2[1].w += d.y * u.w;
            a2[2].x += d.z * u.x; a2[2].y += d.z * u.y; a2[2].z += d.z * u.z; a2[2].w += d.z * u.w;
            a2[3].x += d.w * u.x; a2[3].y += d.w * u.y; a2[3].z += d.w * u.z; a2[3].w += d.w * u.w;
        }
    }
    // the 16 waves' sums in wave order, one float4 of the 8 per pass
    for (int pass = 0; pass < 8; ++pass) {
        float* out = pass < 4 ? dW1 : dW2;
        if (!out) continue;                                          // uniform
        __syncthreads();
        red[w][lane] = pass < 4 ? a1[pass & 3] : a2[pass & 3];
        __syncthreads();
        if (w == 0) {
            float4 t = red[0][lane];
#pragma unroll
            for (int k = 1; k < GW; ++k) { t.x += red[k][lane].x; t.y += red[k][lane].y; t.z += red[k][lane].z; t.w += red[k][lane].w; }
            float* o = pass < 4 ? dW1 + (int64_t)(u0 + pass) * H + c0 : dW2 + (int64_t)(c0 + (pass & 3)) * A + u0;
            const float4 old = ld4(o);
            t.x += old.x; t.y += old.y; t.z += old.z; t.w += old.w;
            st4(o, t);
        }
    }
}

inline int64_t du_floats(int64_t M, int64_t A) { return (M * A + 63) / 64 * 64; }

inline int check_shape(const char* who, int64_t M, int64_t H, int64_t A) {
    DYN_REQUIRE(M >= 0, DYN_E_ARG, "%s: bad row count M=%lld", who, (long long)M);
    DYN_REQUIRE(H > 0 && H % 256 == 0 && H <= 2048, DYN_E_ARG, "%s: H=%lld must be a multiple of 256 up to 2048", who, (long long)H);
    DYN_REQUIRE(A >= 4 && A % 4 == 0 && A <= 64, DYN_E_ARG, "%s: A=%lld must be a multiple of 4 from 4 to 64", who, (long long)A);
    return DYN_OK;
}

// The built instances: NV = H / 256 in {1 .. 8}; check_shape admits no other H.
template <class Go>
void dispatch(int64_t H, Go go) { dyn::dispatch_nv<1, 2, 3, 4, 5, 6, 7, 8>(H, go); }

}  // namespace

extern "C" int dyn_attn_adapter_fwd(const float* x, const float* gamma, const float* beta, const float* W1, const float* b1, const float* W2,
                                    const float* b2, float* y, float* mean, float* rstd, float* a, int64_t M, int64_t H, int64_t A, float eps,
                                    void* stream) {
    DYN_REQUIRE(x && gamma && beta && W1 && b1 && W2 && b2 && y, DYN_E_ARG, "dyn_attn_adapter_fwd: null argument (only mean, rstd and a may be null)");
    const int rc = check_shape("dyn_attn_adapter_fwd", M, H, A);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(W1) && aligned16(W2) && aligned16(b2) && aligned16(y), DYN_E_ARG,
                "dyn_attn_adapter_fwd: operands must be 16-byte aligned");
    if (M == 0) return DYN_OK;
    dim3 grid(dyn::row_blocks(M, WPB, 2048)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL(adapter_fwd_kernel<decltype(nv)::value>, grid, blk, 0, st, x, gamma, beta, W1, b1, W2, b2, y, mean, rstd, a, M, (int)A, eps);
    });
    return dyn::check_launch("dyn_attn_adapter_fwd");
}

extern "C" int64_t dyn_attn_adapter_bwd_workspace_bytes(int64_t M, int64_t H, int64_t A) {
    if (M < 0 || H <= 0 || A <= 0) return 0;
    return (du_floats(M, A) + (int64_t)dyn::row_blocks(M, WPB, MAX_BWD_BLOCKS) * (3 * H + DB1_COLS)) * (int64_t)sizeof(float);
}

extern "C" int dyn_attn_adapter_bwd(const float* x, const float* gamma, const float* beta, const float* W1, const float* W2, const float* mean,
                                    const float* rstd, const float* a, const float* dy, float* dx, float* dgamma, float* dbeta, float* dW1,
                                    float* db1, float* dW2, float* db2, int64_t M, int64_t H, int64_t A, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(x && gamma && beta && W1 && W2 && mean && rstd && a && dy && dx, DYN_E_ARG,
                "dyn_attn_adapter_bwd: null argument (only the six gradient outputs may be null)");
    const int rc = check_shape("dyn_attn_adapter_bwd", M, H, A);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(dx != dy && dx != x, DYN_E_ARG, "dyn_attn_adapter_bwd: dx must not alias dy or x (it is written out of place)");
    DYN_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(W1) && aligned16(W2) && aligned16(a) && aligned16(dy) &&
                    aligned16(dx) && aligned16(dgamma) && aligned16(dbeta) && aligned16(dW1) && aligned16(dW2) && aligned16(db2),
                DYN_E_ARG, "dyn_attn_adapter_bwd: operands must be 16-byte aligned");
    if (M == 0) return DYN_OK;
    const bool vec = dgamma || dbeta || db1 || db2;
    const int nb = dyn::row_blocks(M, WPB, MAX_BWD_BLOCKS);
    float *du = nullptr, *partial = nullptr;
    if (vec || dW1 || dW2) {
        DYN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= dyn_attn_adapter_bwd_workspace_bytes(M, H, A), DYN_E_WORKSPACE,
                    "dyn_attn_adapter_bwd: workspace too small");
        if (dW1) du = (float*)workspace;
        if (vec) partial = (float*)workspace + du_floats(M, A);
    }
    hipStream_t st = (hipStream_t)stream;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL(adapter_bwd_kernel<decltype(nv)::value>, dim3(nb), dim3(256), 0, st, x, gamma, W1, W2, mean, rstd, a, dy, dx, du, partial, M, (int)A);
    });
    if (vec || dW1 || dW2) {
        // The six outputs are written by no other entry, so nothing a deferral context has recorded can be overtaken here.
        const int n_gemm = (dW1 || dW2) ? (int)((H / 256) * (A / 4)) : 0;
        const int n_red = vec ? (int)((3 * H + DB1_COLS) / 64) : 0;
        hipLaunchKernelGGL(adapter_bwd_sums_kernel, dim3(n_gemm + n_red), dim3(64 * GW), 0, st, x, gamma, beta, mean, rstd, a, dy, du, partial, dW1,
                           dW2, dgamma, dbeta, db2, db1, M, (int)H, (int)A, nb, n_gemm);
    }
    return dyn::check_launch("dyn_attn_adapter_bwd");
}
