// The conv-module core of csrc/convmod_bn.hip with the norm the reference's third loop actually runs (reference nvidia_ctc/lib.py:74,89-102:
// the conv modules' BatchNorm1d is REPLACED by a fresh BatchRenorm1d, which is in training mode):
//     glu -> depthwise_conv (KW taps, SAME) -> BatchRenorm1d in training mode (statistics of the batch, corrected towards the running
//     statistics by the detached factors r and d; the running statistics move) -> activation.
// The BatchRenorm1d definition is the widely used `batchrenorm` package form (eps added to the deviation, running_std kept instead of
// running_var); parity unpinned against upstream `lcasr`.  Per channel over the n = B * valid valid rows of x = the depthwise output:
//     mu = mean(x), std = sqrt(mean((x - mu)^2)), sig = std + eps, r = clamp(sig / running_std, 1 / rmax, rmax),
//     d = clamp((mu - running_mean) / running_std, -dmax, dmax), s = act(weight * ((x - mu) / sig * r + d) + bias),
//     running_mean += momentum * (mu - running_mean), running_std += momentum * (sig - running_std).
//
//   dyn_convmod_brn_fwd   three launches.
//     (a) the thread-per-channel GLU + depthwise forward of convmod_bn.hip (the same register window), writing gl and c; each workgroup
//         also leaves, per channel, the CENTRED statistic of its time tile: count, tile mean, sum of squared deviations from the tile mean
//         (Welford's update over the tile's valid rows, which are a prefix of the tile, so the reciprocal counts are compile-time constants
//         and no value has to be kept: no register beyond the eval-mode kernel's window).  A tile without a valid row leaves count 0.
//     (b) one thread per channel combines the partials in tile order by the pairwise update (Chan et al.), skipping count 0, forms the seven
//         per-channel rows of `stats` and moves the running statistics in place (momentum > 0).
//     (c) s = act((c - mu) * scale + shift), 16 bytes per lane, rows >= *valid exact zeros.
//   dyn_convmod_brn_bwd   three launches.
//     (1) g = ds * act'(y) written over dc (dc may be ds) and the column sums of g and g * x0 as per-workgroup partial rows, the rows
//         visited in convmod_bn_bwd_act_kernel's fixed order; (2) one thread per channel adds the partials in workgroup order, writes
//         dweight / dbias and the two means; (3) dc = scale * (g - mean(g) - xt * mean(g * x0)) in place.
// No float atomics, no E[x^2] - E[x]^2: every result is bit-reproducible.  A channel whose batch variance is exactly zero is outside the
// contract (xt = (x - mu) / std is 0 / 0 there).
#include "common.h"
#include "dwconv_window.h"

namespace {

constexpr int KW9 = 9, KW32 = 32;
constexpr int TT9 = 16, TT32 = 32;      // frames per workgroup: convmod_bn.hip's tiles
constexpr int ACT_SILU = 0;
constexpr int FIN_BATCH = 16;           // partials a finalise thread has in flight at once (it is latency-bound: one thread per channel)
constexpr int STATS_ROWS = 7;          // mu, 1 / sig, r, d, scale = weight * r / sig, shift = weight * d + bias, 1 / std
enum { S_MU = 0, S_ISIG, S_R, S_D, S_SCALE, S_SHIFT, S_ISTD };

using dyn::silu_f;
using dyn::silu_grad;

// grid (ceil(T / TT), C / 256, B); 256 threads, thread = channel.  part [B * tiles][3][C]: count, mean, M2 of the tile.
template <int KW, int TT>
__global__ __launch_bounds__(256) void convmod_brn_conv_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                                const float* __restrict__ cbias, float* __restrict__ gl_out,
                                                                float* __restrict__ c_out, float* __restrict__ part,
                                                                const int32_t* __restrict__ valid, int64_t T, int C) {
    constexpr int HL = (KW - 1) / 2, HR = KW - 1 - HL, NG = TT + HL + HR;
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t b = blockIdx.z, t0 = (int64_t)blockIdx.x * TT;
    const int64_t vr = dyn::valid_rows(valid, T);
    float wk[KW], g[NG];
    const float cb = dyn::load_glu_window(w, cbias, u + b * T * 2 * C + c, c, C, t0 - HL, vr, wk, g);
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < TT; ++k) {
        const int64_t t = t0 + k;
        if (t >= T) break;
        const int64_t o = (b * T + t) * C + c;
        float cv = 0.f;
        if (t < vr) {                                   // the valid rows of a tile are its first ones: this is its (k + 1)-th value
            cv = cb;
#pragma unroll
            for (int j = 0; j < KW; ++j) cv += wk[j] * g[k + j];
            const float dl = cv - mean;
            mean += dl * (1.f / (float)(k + 1));
            m2 += dl * (cv - mean);
            cnt = (float)(k + 1);
        }
        gl_out[o] = g[k + HL];
        c_out[o] = cv;
    }
    float* pp = part + ((int64_t)b * gridDim.x + blockIdx.x) * 3 * C + c;
    pp[0] = cnt;
    pp[C] = mean;
    pp[2 * C] = m2;
}

// grid (C / 64), one wave per workgroup; thread = channel.
__global__ __launch_bounds__(64) void convmod_brn_stats_kernel(const float* __restrict__ part, int64_t nparts, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias, float* running_mean, float* running_std,
                                                                 float* __restrict__ stats, int C, float eps, float rmax, float dmax,
                                                                 float momentum) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int64_t p0 = 0; p0 < nparts; p0 += FIN_BATCH) {          // FIN_BATCH partials' loads in flight, then combined one after the other
        float nb[FIN_BATCH], mb[FIN_BATCH], qb[FIN_BATCH];
#pragma unroll
        for (int i = 0; i < FIN_BATCH; ++i) {
            const bool in = p0 + i < nparts;
            const float* pp = part + (in ? p0 + i : p0) * 3 * C + c;
            nb[i] = in ? pp[0] : 0.f;
            mb[i] = pp[C];
            qb[i] = pp[2 * C];
        }
#pragma unroll
        for (int i = 0; i < FIN_BATCH; ++i)
            if (nb[i] > 0.f) {                                    // the count is the same in every channel: a wave-uniform branch
                const float nn = n + nb[i], dl = mb[i] - mean;
                mean += dl * (nb[i] / nn);
                m2 += qb[i] + dl * dl * (n * nb[i] / nn);
                n = nn;
            }
    }
    const float sd = n > 0.f ? sqrtf(m2 / n) : 0.f, sig = sd + eps;
    const float rm = running_mean[c], rs = running_std[c], gw = weight[c];
    const float r = fminf(fmaxf(sig / rs, 1.f / rmax), rmax);
    const float d = fminf(fmaxf((mean - rm) / rs, -dmax), dmax);
    stats[S_MU * C + c] = mean;
    stats[S_ISIG * C + c] = 1.f / sig;
    stats[S_R * C + c] = r;
    stats[S_D * C + c] = d;
    stats[S_SCALE * C + c] = gw * r / sig;
    stats[S_SHIFT * C + c] = gw * d + bias[c];
    stats[S_ISTD * C + c] = 1.f / sd;
    if (momentum > 0.f && n > 0.f) {
        running_mean[c] = rm + momentum * (mean - rm);
        running_std[c] = rs + momentum * (sig - rs);
    }
}

// grid-stride over rows * C / 4 float4s.
__global__ __launch_bounds__(256) void convmod_brn_apply_kernel(const float4* __restrict__ c_in, const float4* __restrict__ stats,
                                                                 float4* __restrict__ s, const int32_t* __restrict__ valid, int64_t rows,
                                                                 int64_t T, int C4) {
    const int64_t vr = dyn::valid_rows(valid, T);
    const int64_t total = rows * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int q = (int)(i - row * C4);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row % T < vr) {
            const float4 x = c_in[i], mu = stats[S_MU * C4 + q], sc = stats[S_SCALE * C4 + q], sh = stats[S_SHIFT * C4 + q];
            o.x = silu_f((x.x - mu.x) * sc.x + sh.x);
            o.y = silu_f((x.y - mu.y) * sc.y + sh.y);
            o.z = silu_f((x.z - mu.z) * sc.z + sh.z);
            o.w = silu_f((x.w - mu.w) * sc.w + sh.w);
        }
        s[i] = o;
    }
}

// grid (nb, C / 256); thread = channel; workgroup x takes rows x, x + nb, ... of the B * T rows in that order (convmod_bn_bwd_act_kernel's).
__global__ __launch_bounds__(256) void convmod_brn_bwd_act_kernel(const float* __restrict__ c_in, const float* __restrict__ stats, const float* ds,
                                                                   float* g_out, float* __restrict__ pg, float* __restrict__ px,
                                                                   const int32_t* __restrict__ valid, int64_t rows, int64_t T, int C) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t vr = dyn::valid_rows(valid, T);
    const float mu = stats[S_MU * C + c], isig = stats[S_ISIG * C + c], sc = stats[S_SCALE * C + c], sh = stats[S_SHIFT * C + c];
    float ag = 0.f, ax = 0.f;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        float o = 0.f;
        if (r % T < vr) {
            const float xc = c_in[r * C + c] - mu;
            o = ds[r * C + c] * silu_grad(xc * sc + sh);
            ag += o;
            ax += o * (xc * isig);
        }
        g_out[r * C + c] = o;
    }
    const int64_t p = (int64_t)blockIdx.x * C + c;
    pg[p] = ag;
    px[p] = ax;
}

// grid (C / 64), one wave per workgroup; thread = channel.  means [2][C]: mean(g), mean(g * x0) over the n = B * valid rows.
__global__ __launch_bounds__(64) void convmod_brn_bwd_sums_kernel(const float* __restrict__ pg, const float* __restrict__ px, int nb,
                                                                    const float* __restrict__ stats, float* dweight, float* dbias,
                                                                    float* dcbias, float beta, float* __restrict__ means,
                                                                    const int32_t* __restrict__ valid, int64_t B, int64_t T, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    float ag = 0.f, ax = 0.f;
    for (int p0 = 0; p0 < nb; p0 += FIN_BATCH) {                  // FIN_BATCH partial rows' loads in flight, added in workgroup order
        float vg[FIN_BATCH], vx[FIN_BATCH];
#pragma unroll
        for (int i = 0; i < FIN_BATCH; ++i) {
            const bool in = p0 + i < nb;
            const int64_t o = (int64_t)(in ? p0 + i : p0) * C + c;
            vg[i] = in ? pg[o] : 0.f;
            vx[i] = in ? px[o] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < FIN_BATCH; ++i) {
            ag += vg[i];
            ax += vx[i];
        }
    }
    const float n = (float)(B * dyn::valid_rows(valid, T));
    const float inv = n > 0.f ? 1.f / n : 0.f;
    means[c] = ag * inv;
    means[C + c] = ax * inv;
    if (dweight) dweight[c] = (beta != 0.f ? beta * dweight[c] : 0.f) + (stats[S_R * C + c] * ax + stats[S_D * C + c] * ag);
    if (dbias) dbias[c] = (beta != 0.f ? beta * dbias[c] : 0.f) + ag;
    if (dcbias && beta != 1.f) dcbias[c] = beta != 0.f ? beta * dcbias[c] : 0.f;      // its gradient is identically zero in this mode
}

// grid-stride over rows * C / 4 float4s; in place over g.
__global__ __launch_bounds__(256) void convmod_brn_bwd_dx_kernel(const float4* __restrict__ c_in, const float4* __restrict__ stats,
                                                                  const float4* __restrict__ means, float4* g, const int32_t* __restrict__ valid,
                                                                  int64_t rows, int64_t T, int C4) {
    const int64_t vr = dyn::valid_rows(valid, T);
    const int64_t total = rows * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int q = (int)(i - row * C4);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row % T < vr) {
            const float4 x = c_in[i], gv = g[i], mu = stats[S_MU * C4 + q], sc = stats[S_SCALE * C4 + q], is = stats[S_ISTD * C4 + q];
            const float4 mg = means[q], mx = means[C4 + q];
            o.x = sc.x * (gv.x - mg.x - (x.x - mu.x) * is.x * mx.x);
            o.y = sc.y * (gv.y - mg.y - (x.y - mu.y) * is.y * mx.y);
            o.z = sc.z * (gv.z - mg.z - (x.z - mu.z) * is.z * mx.z);
            o.w = sc.w * (gv.w - mg.w - (x.w - mu.w) * is.w * mx.w);
        }
        g[i] = o;
    }
}

inline int bwd_blocks(int64_t rows) { return (int)(rows < 1 ? 1 : rows > 512 ? 512 : rows); }
inline unsigned flat_blocks(int64_t n4) { return (unsigned)(n4 < 256 ? 1 : dyn::cdiv(n4, 256) > 4096 ? 4096 : dyn::cdiv(n4, 256)); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_dims(const char* who, int64_t B, int64_t T, int64_t C, int64_t KW) {
    if (int rc = dyn::check_convmod_dims(who, B, T, C)) return rc;
    DYN_REQUIRE(B * T >= 2, DYN_E_ARG, "%s: B * T = %lld rows: a batch statistic needs at least 2", who, (long long)(B * T));
    DYN_REQUIRE(KW == KW9 || KW == KW32, DYN_E_UNSUPPORTED, "%s: kernel width %lld is not built (9, 32)", who, (long long)KW);
    return DYN_OK;
}

inline int64_t tiles(int64_t T, int64_t KW) { return dyn::cdiv(T, KW == KW9 ? TT9 : TT32); }

}  // namespace

extern "C" int64_t dyn_convmod_brn_stats_rows(void) { return STATS_ROWS; }

extern "C" int64_t dyn_convmod_brn_fwd_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW) {
    if (KW != KW9 && KW != KW32) return 0;
    return (int64_t)3 * B * tiles(T, KW) * C * (int64_t)sizeof(float);
}

extern "C" int dyn_convmod_brn_fwd(const float* u, const float* w, const float* cbias, float* running_mean, float* running_std,
                                   const float* weight, const float* bias, float* s, float* gl, float* c, float* stats, const int32_t* valid,
                                   int64_t B, int64_t T, int64_t C, int64_t KW, int32_t act, float eps, float rmax, float dmax, float momentum,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(u && w && running_mean && running_std && weight && bias && s && gl && c && stats, DYN_E_ARG, "dyn_convmod_brn_fwd: null pointer");
    if (int rc = check_dims("dyn_convmod_brn_fwd", B, T, C, KW)) return rc;
    DYN_REQUIRE(act == ACT_SILU, DYN_E_UNSUPPORTED, "dyn_convmod_brn_fwd: act=%d is not built (0 SiLU)", (int)act);
    DYN_REQUIRE(rmax >= 1.f && dmax >= 0.f && momentum >= 0.f && momentum <= 1.f && eps >= 0.f, DYN_E_ARG,
                "dyn_convmod_brn_fwd: rmax=%g must be >= 1, dmax=%g >= 0, momentum=%g in [0, 1], eps=%g >= 0", rmax, dmax, momentum, eps);
    DYN_REQUIRE(aligned16(s) && aligned16(c) && aligned16(stats), DYN_E_ARG, "dyn_convmod_brn_fwd: s, c and stats must be 16-byte aligned");
    const int64_t bytes = dyn_convmod_brn_fwd_workspace_bytes(B, T, C, KW);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "dyn_convmod_brn_fwd: workspace too small (%lld bytes needed)",
                (long long)bytes);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int64_t nt = tiles(T, KW);
    const dim3 grid((unsigned)nt, (unsigned)(C / 256), (unsigned)B);
#define GO(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, st, u, w, cbias, gl, c, part, valid, T, (int)C)
    if (KW == KW9) GO((convmod_brn_conv_kernel<KW9, TT9>));
    else GO((convmod_brn_conv_kernel<KW32, TT32>));
#undef GO
    hipLaunchKernelGGL(convmod_brn_stats_kernel, dim3((unsigned)(C / 64)), dim3(64), 0, st, part, B * nt, weight, bias, running_mean, running_std,
                       stats, (int)C, eps, rmax, dmax, momentum);
    hipLaunchKernelGGL(convmod_brn_apply_kernel, dim3(flat_blocks(B * T * (C / 4))), dim3(256), 0, st, (const float4*)c, (const float4*)stats,
                       (float4*)s, valid, B * T, T, (int)(C / 4));
    return dyn::check_launch("dyn_convmod_brn_fwd");
}

extern "C" int64_t dyn_convmod_brn_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C) {
    return (int64_t)(2 * bwd_blocks(B * T) + 2) * C * (int64_t)sizeof(float);
}

extern "C" int dyn_convmod_brn_bwd(const float* c, const float* stats, const float* ds, float* dc, float* dweight, float* dbias, float* dcbias,
                                   float wgrad_beta, const int32_t* valid, int64_t B, int64_t T, int64_t C, int32_t act, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(c && stats && ds && dc, DYN_E_ARG, "dyn_convmod_brn_bwd: null pointer");
    if (int rc = check_dims("dyn_convmod_brn_bwd", B, T, C, KW9)) return rc;
    DYN_REQUIRE(act == ACT_SILU, DYN_E_UNSUPPORTED, "dyn_convmod_brn_bwd: act=%d is not built (0 SiLU)", (int)act);
    DYN_REQUIRE(aligned16(c) && aligned16(dc) && aligned16(stats) && aligned16(workspace), DYN_E_ARG,
                "dyn_convmod_brn_bwd: c, dc, stats and the workspace must be 16-byte aligned");
    const int64_t bytes = dyn_convmod_brn_bwd_workspace_bytes(B, T, C);
    DYN_REQUIRE(workspace && workspace_bytes >= bytes, DYN_E_WORKSPACE, "dyn_convmod_brn_bwd: workspace too small (%lld bytes needed)",
                (long long)bytes);
    const int64_t rows = B * T;
    const int nb = bwd_blocks(rows);
    hipStream_t st = (hipStream_t)stream;
    float* pg = (float*)workspace;
    float* px = pg + (int64_t)nb * C;
    float* means = px + (int64_t)nb * C;
    hipLaunchKernelGGL(convmod_brn_bwd_act_kernel, dim3((unsigned)nb, (unsigned)(C / 256)), dim3(256), 0, st, c, stats, ds, dc, pg, px, valid, rows,
                       T, (int)C);
    dyn::ordered_before_launch(st);      // recorded (deferred) reductions into dweight / dbias go first: recording order is execution order
    hipLaunchKernelGGL(convmod_brn_bwd_sums_kernel, dim3((unsigned)(C / 64)), dim3(64), 0, st, pg, px, nb, stats, dweight, dbias, dcbias,
                       wgrad_beta, means, valid, B, T, (int)C);
    hipLaunchKernelGGL(convmod_brn_bwd_dx_kernel, dim3(flat_blocks(rows * (C / 4))), dim3(256), 0, st, (const float4*)c, (const float4*)stats,
                       (const float4*)means, (float4*)dc, valid, rows, T, (int)(C / 4));
    return dyn::check_launch("dyn_convmod_brn_bwd");
}
