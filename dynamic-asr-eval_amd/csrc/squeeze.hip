// The two ends of SEW's squeezed encoder (transformers SEWEncoder.forward), one pass each way.  The encoder runs at T2 = T / s frames
// (s = squeeze_factor): in front of its layers the input h [B, T, H] is average-pooled over s frames and a strided positional conv of h is
// added, behind them a projection to s H channels is cut back into s frames of H channels and padded with zero rows to T frames.
//   squeeze forward:  row (b, t), t < T2 = mean_j h[b, s t + j] + gelu(the G segments yg[b, g, t, 0:cg] side by side + conv bias);
//                     z = LayerNorm_H(row) * gamma + beta; mean / rstd [B T2] kept for the backward.  yg (the grouped GEMM's output, group-major)
//                     and h are read once and left alone.  Replaces a group unpack, a GELU, a pool, an add and a LayerNorm over [B, T, H].
//   squeeze backward: the pre-LN row is RECOMPUTED from h, yg, bias; dsum = LayerNorm backward of dz; dh rows s t + j = dsum[t] / s (rows
//                     >= s T2: zeros); dyg [B, G, T2, cg] = dsum * gelu'(yg + bias) in the layout the weight- and data-gradient GEMMs read;
//                     dgamma, dbeta, dbias = column sums.
//   unsqueeze forward / backward: out [B, T, H] rows t < s T2 = gelu(u[b, t / s, (t % s) H ..]) (u [B, T2, s H]: the same floats, another
//                     batch stride when s T2 < T), zero rows after; du = d * gelu'(u).
//   dyn_squeeze_fwd / _bwd (SEW-D): the squeeze pair with the LayerNorm compiled out of the same two kernel templates (LN = false): the sum
//                     itself is the layers' input, dsum = dz, and of the three column sums only the conv bias's remains.
// `valid` (device int32 scalar, in SQUEEZED frames, read when the kernel runs: a zero-padded length bucket) cuts every output: rows >= valid
// of z and dyg, rows >= s valid of dh, of the upsampled output and of du are exact zeros, and no input row at or past them is read by the
// two backwards.
// The row kernels are layernorm_row.h's (one wave64 per row, NV = H / 256 float4 per lane; cg % 4 == 0: a float4 never straddles two
// segments); the three column sums are accumulated per workgroup in registers, written as partial rows and summed by the fixed-order
// reducer.  Nothing here synchronises or allocates.
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

// The pre-LayerNorm row element: the pool of the s frames + gelu(a), a = yg + bias.
__device__ __forceinline__ float4 pooled(const float* __restrict__ h, int64_t at, int64_t H, int s) {
    float4 p = ld4(h + at);
    for (int k = 1; k < s; ++k) {
        const float4 q = ld4(h + at + k * H);
        p.x += q.x; p.y += q.y; p.z += q.z; p.w += q.w;
    }
    const float fs = (float)s;
    p.x /= fs; p.y /= fs; p.z /= fs; p.w /= fs;
    return p;
}

// LN false (SEW-D, dyn_squeeze_fwd): the row itself is the output, no statistics; gamma, beta, mean_out, rstd_out are not touched.
template <int NV, bool LN = true>
__global__ __launch_bounds__(256) void sq_fwd_kernel(const float* __restrict__ h, const float* __restrict__ yg, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ z,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t B, int64_t T,
                                                      int64_t T2, int64_t Tg, int G, int cg, int s, float eps,
                                                      const int32_t* __restrict__ valid) {
    constexpr int H = NV * 256;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t Tv = valid_rows(valid, T2);
    float4 cb[NV];
    int gi[NV], ci[NV];          // this lane's float4 j: group and channel inside the group
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int ch = 4 * (lane + 64 * j);
        cb[j] = ld4(bias + ch);
        gi[j] = ch / cg;
        ci[j] = ch % cg;
    }
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < B * T2; row += (int64_t)gridDim.x * WPB) {
        const int64_t b = row / T2, t = row % T2;
        float4 v[NV];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 a = ld4(yg + ((b * G + gi[j]) * Tg + t) * cg + ci[j]);
            const float4 p = pooled(h, (b * T + s * t) * H + 4 * (lane + 64 * j), H, s);
            v[j].x = p.x + dyn::gelu_f(a.x + cb[j].x); v[j].y = p.y + dyn::gelu_f(a.y + cb[j].y);
            v[j].z = p.z + dyn::gelu_f(a.z + cb[j].z); v[j].w = p.w + dyn::gelu_f(a.w + cb[j].w);
            sum += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        const bool live = t < Tv;
        if constexpr (!LN) {
#pragma unroll
            for (int j = 0; j < NV; ++j) st4(z + row * H + 4 * (lane + 64 * j), live ? v[j] : make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        float mean, rstd;
        dyn::row_mean_rstd(v, sum, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                const float4 gm = ld4(gamma + 4 * (lane + 64 * j)), bt = ld4(beta + 4 * (lane + 64 * j));
                o.x = (v[j].x - mean) * rstd * gm.x + bt.x; o.y = (v[j].y - mean) * rstd * gm.y + bt.y;
                o.z = (v[j].z - mean) * rstd * gm.z + bt.z; o.w = (v[j].w - mean) * rstd * gm.w + bt.w;
            }
            st4(z + row * H + 4 * (lane + 64 * j), o);
        }
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
    }
}

// Rows walked: B * (T2 + 1); the extra row of every batch entry writes the zeros of the T - s T2 frames no squeezed frame pools.
// partial_g / partial_b / partial_c [gridDim.x, H]: this workgroup's sums of dz * xhat, dz and dyg (a null pointer: not wanted).
// LN false (SEW-D, dyn_squeeze_bwd): dsum = dz; h, gamma, mean_in, rstd_in, partial_g, partial_b are not touched (null).
template <int NV, bool LN = true>
__global__ __launch_bounds__(256) void sq_bwd_kernel(const float* __restrict__ h, const float* __restrict__ yg, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean_in,
                                                      const float* __restrict__ rstd_in, const float* __restrict__ dz, float* __restrict__ dh,
                                                      float* __restrict__ dyg, float* __restrict__ partial_g, float* __restrict__ partial_b,
                                                      float* __restrict__ partial_c, int64_t B, int64_t T, int64_t T2, int64_t Tg, int G, int cg,
                                                      int s, const int32_t* __restrict__ valid) {
    constexpr int H = NV * 256;
    __shared__ float4 red[WPB][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t Tv = valid_rows(valid, T2);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cb[NV], ag[NV], ab[NV], ac[NV];
    int gi[NV], ci[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int ch = 4 * (lane + 64 * j);
        cb[j] = ld4(bias + ch);
        gi[j] = ch / cg;
        ci[j] = ch % cg;
        ag[j] = ab[j] = ac[j] = zero;
    }
    const float fs = (float)s;
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < B * (T2 + 1); row += (int64_t)gridDim.x * WPB) {
        const int64_t b = row / (T2 + 1), t = row % (T2 + 1);
        if (t == T2) {           // the frames past the last whole pool window: no gradient
            for (int64_t r = s * T2; r < T; ++r)
#pragma unroll
                for (int j = 0; j < NV; ++j) st4(dh + (b * T + r) * H + 4 * (lane + 64 * j), zero);
            continue;
        }
        if (t >= Tv) {           // past the utterance: no gradient, nothing read
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                st4(dyg + ((b * G + gi[j]) * T2 + t) * cg + ci[j], zero);
                for (int k = 0; k < s; ++k) st4(dh + (b * T + s * t + k) * H + 4 * (lane + 64 * j), zero);
            }
            continue;
        }
        const int64_t r2 = b * T2 + t;
        if constexpr (!LN) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float4 y = ld4(yg + ((b * G + gi[j]) * Tg + t) * cg + ci[j]);
                const float4 d = ld4(dz + r2 * H + 4 * (lane + 64 * j));
                float4 o, dp;
                o.x = d.x * dyn::gelu_grad(y.x + cb[j].x); o.y = d.y * dyn::gelu_grad(y.y + cb[j].y);
                o.z = d.z * dyn::gelu_grad(y.z + cb[j].z); o.w = d.w * dyn::gelu_grad(y.w + cb[j].w);
                ac[j].x += o.x; ac[j].y += o.y; ac[j].z += o.z; ac[j].w += o.w;
                st4(dyg + ((b * G + gi[j]) * T2 + t) * cg + ci[j], o);
                dp.x = d.x / fs; dp.y = d.y / fs; dp.z = d.z / fs; dp.w = d.w / fs;
                for (int k = 0; k < s; ++k) st4(dh + (b * T + s * t + k) * H + 4 * (lane + 64 * j), dp);
            }
            continue;
        }
        const float mean = mean_in[r2], rstd = rstd_in[r2];
        float4 a[NV], xh[NV], dn[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 y = ld4(yg + ((b * G + gi[j]) * Tg + t) * cg + ci[j]);
            const float4 p = pooled(h, (b * T + s * t) * H + 4 * (lane + 64 * j), H, s);
            const float4 d = ld4(dz + r2 * H + 4 * (lane + 64 * j));
            const float4 gm = ld4(gamma + 4 * (lane + 64 * j));
            a[j].x = y.x + cb[j].x; a[j].y = y.y + cb[j].y; a[j].z = y.z + cb[j].z; a[j].w = y.w + cb[j].w;
            xh[j].x = (p.x + dyn::gelu_f(a[j].x) - mean) * rstd; xh[j].y = (p.y + dyn::gelu_f(a[j].y) - mean) * rstd;
            xh[j].z = (p.z + dyn::gelu_f(a[j].z) - mean) * rstd; xh[j].w = (p.w + dyn::gelu_f(a[j].w) - mean) * rstd;
            ag[j].x += d.x * xh[j].x; ag[j].y += d.y * xh[j].y; ag[j].z += d.z * xh[j].z; ag[j].w += d.w * xh[j].w;
            ab[j].x += d.x; ab[j].y += d.y; ab[j].z += d.z; ab[j].w += d.w;
            dn[j].x = d.x * gm.x; dn[j].y = d.y * gm.y; dn[j].z = d.z * gm.z; dn[j].w = d.w * gm.w;
            dyn::bwd_lane_sums(dn[j], xh[j], s1, s2);
        }
        dyn::bwd_row_means<NV>(s1, s2);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 ds = dyn::bwd4(dn[j], xh[j], rstd, s1, s2);
            float4 o, dp;
            o.x = ds.x * dyn::gelu_grad(a[j].x); o.y = ds.y * dyn::gelu_grad(a[j].y);
            o.z = ds.z * dyn::gelu_grad(a[j].z); o.w = ds.w * dyn::gelu_grad(a[j].w);
            ac[j].x += o.x; ac[j].y += o.y; ac[j].z += o.z; ac[j].w += o.w;
            st4(dyg + ((b * G + gi[j]) * T2 + t) * cg + ci[j], o);
            dp.x = ds.x / fs; dp.y = ds.y / fs; dp.z = ds.z / fs; dp.w = ds.w / fs;
            for (int k = 0; k < s; ++k) st4(dh + (b * T + s * t + k) * H + 4 * (lane + 64 * j), dp);
        }
    }
    if (partial_g) dyn::combine_waves(ag, red, partial_g + (int64_t)blockIdx.x * H);     // null or not: uniform over the grid
    if (partial_b) dyn::combine_waves(ab, red, partial_b + (int64_t)blockIdx.x * H);
    if (partial_c) dyn::combine_waves(ac, red, partial_c + (int64_t)blockIdx.x * H);
}

// One float4 per thread and step: n4 = B * T * H / 4 elements of the output; a row t of it is live when t < s * valid.
__global__ __launch_bounds__(256) void unsq_fwd_kernel(const float* __restrict__ u, float* __restrict__ out, int64_t n4, int64_t T, int64_t T2,
                                                        int64_t H4, int s, const int32_t* __restrict__ valid) {
    const int64_t live = s * valid_rows(valid, T2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c4 = i % H4, t = (i / H4) % T, b = i / (H4 * T);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < live) {
            const float4 v = ld4(u + ((b * T2 * s + t) * H4 + c4) * 4);
            o.x = dyn::gelu_f(v.x); o.y = dyn::gelu_f(v.y); o.z = dyn::gelu_f(v.z); o.w = dyn::gelu_f(v.w);
        }
        st4(out + i * 4, o);
    }
}

// n4 = B * s T2 * H / 4 elements of du (u's own layout); d [B, T, H] is read on live rows only.
__global__ __launch_bounds__(256) void unsq_bwd_kernel(const float* __restrict__ u, const float* __restrict__ d, float* __restrict__ du,
                                                        int64_t n4, int64_t T, int64_t T2, int64_t H4, int s,
                                                        const int32_t* __restrict__ valid) {
    const int64_t live = s * valid_rows(valid, T2), Ts = s * T2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c4 = i % H4, t = (i / H4) % Ts, b = i / (H4 * Ts);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < live) {
            const float4 v = ld4(u + i * 4), g = ld4(d + ((b * T + t) * H4 + c4) * 4);
            o.x = g.x * dyn::gelu_grad(v.x); o.y = g.y * dyn::gelu_grad(v.y); o.z = g.z * dyn::gelu_grad(v.z); o.w = g.w * dyn::gelu_grad(v.w);
        }
        st4(du + i * 4, o);
    }
}

// The built instances: NV = H / 256 in {1, 2, 3, 4}; check_shape admits no other H.
template <class Go>
void dispatch(int64_t H, Go go) { dyn::dispatch_nv<1, 2, 3, 4>(H, go); }

inline int check_factor(const char* who, int64_t s) {
    DYN_REQUIRE(s >= 1 && s <= 4, DYN_E_ARG, "%s: squeeze factor s=%lld must be 1, 2, 3 or 4", who, (long long)s);
    return DYN_OK;
}

// The shape rules the two squeeze entries share; `who` names the entry in the message.
inline int check_shape(const char* who, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s) {
    const int rc = check_factor(who, s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(B >= 0 && T >= 0 && Tg >= T / s, DYN_E_ARG, "%s: bad dimensions (B=%lld, T=%lld, Tg=%lld; need Tg >= T / s)", who, (long long)B,
                (long long)T, (long long)Tg);
    DYN_REQUIRE(H > 0 && H % 256 == 0 && H <= 1024, DYN_E_ARG, "%s: H=%lld must be a multiple of 256 up to 1024", who, (long long)H);
    DYN_REQUIRE(G > 0 && H % G == 0 && (H / G) % 4 == 0, DYN_E_ARG, "%s: H / G = %lld / %lld channels per group must be a whole multiple of 4",
                who, (long long)H, (long long)G);
    return DYN_OK;
}

inline int64_t grid_for(int64_t n4) {
    int64_t g = dyn::cdiv(n4, 256);
    return g > 4096 ? 4096 : (g < 1 ? 1 : g);
}

}  // namespace

extern "C" int dyn_squeeze_ln_fwd(const float* h, const float* yg, const float* bias, const float* gamma, const float* beta, float* z, float* mean,
                                  float* rstd, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, float eps,
                                  const int32_t* valid_rows, void* stream) {
    DYN_REQUIRE(h && yg && bias && gamma && beta && z && mean && rstd, DYN_E_ARG, "dyn_squeeze_ln_fwd: null argument");
    const int rc = check_shape("dyn_squeeze_ln_fwd", B, T, Tg, H, G, s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(h) && aligned16(yg) && aligned16(bias) && aligned16(gamma) && aligned16(beta) && aligned16(z), DYN_E_ARG,
                "dyn_squeeze_ln_fwd: operands must be 16-byte aligned");
    const int64_t T2 = T / s, rows = B * T2;
    if (rows == 0) return DYN_OK;
    dim3 grid(dyn::row_blocks(rows, WPB, 2048)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G), f = (int)s;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL(sq_fwd_kernel<decltype(nv)::value>, grid, blk, 0, st, h, yg, bias, gamma, beta, z, mean, rstd, B, T, T2, Tg, g, cg, f, eps, valid_rows);
    });
    return dyn::check_launch("dyn_squeeze_ln_fwd");
}

extern "C" int64_t dyn_squeeze_ln_bwd_workspace_bytes(int64_t rows, int64_t H) {
    return (int64_t)3 * dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS) * H * (int64_t)sizeof(float);
}

extern "C" int dyn_squeeze_ln_bwd(const float* h, const float* yg, const float* bias, const float* gamma, const float* mean, const float* rstd,
                                  const float* dz, float* dh, float* dyg, float* dgamma, float* dbeta, float* dbias, float wgrad_beta, int64_t B,
                                  int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, const int32_t* valid_rows, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(h && yg && bias && gamma && mean && rstd && dz && dh && dyg, DYN_E_ARG,
                "dyn_squeeze_ln_bwd: null argument (only dgamma, dbeta and dbias may be null)");
    const int rc = check_shape("dyn_squeeze_ln_bwd", B, T, Tg, H, G, s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(h) && aligned16(yg) && aligned16(bias) && aligned16(gamma) && aligned16(dz) && aligned16(dh) && aligned16(dyg),
                DYN_E_ARG, "dyn_squeeze_ln_bwd: operands must be 16-byte aligned");
    const int64_t T2 = T / s, rows = B * (T2 + 1);
    if (B * T == 0) return DYN_OK;
    const int nb = dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS);
    float *pg = nullptr, *pb = nullptr, *pc = nullptr;
    if (dgamma || dbeta || dbias) {
        const int64_t need = dyn_squeeze_ln_bwd_workspace_bytes(rows, H);
        DYN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need, DYN_E_WORKSPACE, "dyn_squeeze_ln_bwd: workspace too small");
        float* p = dyn::partials_alloc(workspace, need);            // the workspace, or the open deferral context's arena
        pg = dgamma ? p : nullptr;
        pb = dbeta ? p + (int64_t)nb * H : nullptr;
        pc = dbias ? p + (int64_t)2 * nb * H : nullptr;
    }
    dim3 grid(nb), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G), f = (int)s;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL(sq_bwd_kernel<decltype(nv)::value>, grid, blk, 0, st, h, yg, bias, gamma, mean, rstd, dz, dh, dyg, pg, pb, pc, B, T, T2, Tg, g, cg, f, valid_rows);
    });
    if (dgamma && dbeta) dyn::reduce_pair_or_defer(pg, dgamma, pb, dbeta, (int64_t)nb, H, wgrad_beta, st);
    else {
        if (dgamma) dyn::reduce_or_defer(pg, dgamma, (int64_t)nb, H, wgrad_beta, st);
        if (dbeta) dyn::reduce_or_defer(pb, dbeta, (int64_t)nb, H, wgrad_beta, st);
    }
    if (dbias) dyn::reduce_or_defer(pc, dbias, (int64_t)nb, H, wgrad_beta, st);
    return dyn::check_launch("dyn_squeeze_ln_bwd");
}

extern "C" int dyn_unsqueeze_act_fwd(const float* u, float* out, int64_t B, int64_t T, int64_t H, int64_t s, const int32_t* valid_rows,
                                     void* stream) {
    DYN_REQUIRE(u && out, DYN_E_ARG, "dyn_unsqueeze_act_fwd: null argument");
    const int rc = check_factor("dyn_unsqueeze_act_fwd", s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(B >= 0 && T >= 0 && H > 0 && H % 4 == 0, DYN_E_ARG, "dyn_unsqueeze_act_fwd: bad dimensions (B=%lld, T=%lld, H=%lld; H must be a multiple of 4)",
                (long long)B, (long long)T, (long long)H);
    DYN_REQUIRE(aligned16(u) && aligned16(out), DYN_E_ARG, "dyn_unsqueeze_act_fwd: operands must be 16-byte aligned");
    const int64_t n4 = B * T * (H / 4);
    if (n4 == 0) return DYN_OK;
    hipLaunchKernelGGL(unsq_fwd_kernel, dim3((unsigned)grid_for(n4)), dim3(256), 0, (hipStream_t)stream, u, out, n4, T, T / s, H / 4, (int)s,
                       valid_rows);
    return dyn::check_launch("dyn_unsqueeze_act_fwd");
}

extern "C" int dyn_unsqueeze_act_bwd(const float* u, const float* d, float* du, int64_t B, int64_t T, int64_t H, int64_t s,
                                     const int32_t* valid_rows, void* stream) {
    DYN_REQUIRE(u && d && du, DYN_E_ARG, "dyn_unsqueeze_act_bwd: null argument");
    const int rc = check_factor("dyn_unsqueeze_act_bwd", s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(B >= 0 && T >= 0 && H > 0 && H % 4 == 0, DYN_E_ARG, "dyn_unsqueeze_act_bwd: bad dimensions (B=%lld, T=%lld, H=%lld; H must be a multiple of 4)",
                (long long)B, (long long)T, (long long)H);
    DYN_REQUIRE(aligned16(u) && aligned16(d) && aligned16(du), DYN_E_ARG, "dyn_unsqueeze_act_bwd: operands must be 16-byte aligned");
    const int64_t T2 = T / s, n4 = B * s * T2 * (H / 4);
    if (n4 == 0) return DYN_OK;
    hipLaunchKernelGGL(unsq_bwd_kernel, dim3((unsigned)grid_for(n4)), dim3(256), 0, (hipStream_t)stream, u, d, du, n4, T, T2, H / 4, (int)s,
                       valid_rows);
    return dyn::check_launch("dyn_unsqueeze_act_bwd");
}

// The same two kernels without the LayerNorm (SEW-D: SEWDEncoder.forward hands the sum to its layers as it is).
extern "C" int dyn_squeeze_fwd(const float* h, const float* yg, const float* bias, float* z, int64_t B, int64_t T, int64_t Tg, int64_t H,
                               int64_t G, int64_t s, const int32_t* valid_rows, void* stream) {
    DYN_REQUIRE(h && yg && bias && z, DYN_E_ARG, "dyn_squeeze_fwd: null argument");
    const int rc = check_shape("dyn_squeeze_fwd", B, T, Tg, H, G, s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(h) && aligned16(yg) && aligned16(bias) && aligned16(z), DYN_E_ARG, "dyn_squeeze_fwd: operands must be 16-byte aligned");
    const int64_t T2 = T / s, rows = B * T2;
    if (rows == 0) return DYN_OK;
    dim3 grid(dyn::row_blocks(rows, WPB, 2048)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G), f = (int)s;
    const float* none = nullptr;
    float* nout = nullptr;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL((sq_fwd_kernel<decltype(nv)::value, false>), grid, blk, 0, st, h, yg, bias, none, none, z, nout, nout, B, T, T2, Tg, g, cg, f, 0.f, valid_rows);
    });
    return dyn::check_launch("dyn_squeeze_fwd");
}

extern "C" int64_t dyn_squeeze_bwd_workspace_bytes(int64_t rows, int64_t H) {
    return (int64_t)dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS) * H * (int64_t)sizeof(float);
}

extern "C" int dyn_squeeze_bwd(const float* yg, const float* bias, const float* dz, float* dh, float* dyg, float* dbias, float wgrad_beta,
                               int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, const int32_t* valid_rows, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(yg && bias && dz && dh && dyg, DYN_E_ARG, "dyn_squeeze_bwd: null argument (only dbias may be null)");
    const int rc = check_shape("dyn_squeeze_bwd", B, T, Tg, H, G, s);
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(aligned16(yg) && aligned16(bias) && aligned16(dz) && aligned16(dh) && aligned16(dyg), DYN_E_ARG,
                "dyn_squeeze_bwd: operands must be 16-byte aligned");
    const int64_t T2 = T / s, rows = B * (T2 + 1);
    if (B * T == 0) return DYN_OK;
    const int nb = dyn::row_blocks(rows, WPB, MAX_BWD_BLOCKS);
    float* pc = nullptr;
    if (dbias) {
        const int64_t need = dyn_squeeze_bwd_workspace_bytes(rows, H);
        DYN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need, DYN_E_WORKSPACE, "dyn_squeeze_bwd: workspace too small");
        pc = dyn::partials_alloc(workspace, need);                   // the workspace, or the open deferral context's arena
    }
    dim3 grid(nb), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int g = (int)G, cg = (int)(H / G), f = (int)s;
    const float* none = nullptr;
    float* nout = nullptr;
    dispatch(H, [&](auto nv) {
        hipLaunchKernelGGL((sq_bwd_kernel<decltype(nv)::value, false>), grid, blk, 0, st, none, yg, bias, none, none, none, dz, dh, dyg, nout, nout, pc, B, T, T2, Tg, g, cg, f, valid_rows);
    });
    if (dbias) dyn::reduce_or_defer(pc, dbias, (int64_t)nb, H, wgrad_beta, st);
    return dyn::check_launch("dyn_squeeze_bwd");
}
