// The transducer head of ParakeetForTDT (transformers modeling_parakeet.py: ParakeetRNNTDecoder, ParakeetTDTJointNetwork,
// transformers.loss.loss_tdt.tdt_loss, generation_parakeet.py: ParakeetTDTGenerationMixin) on the MI355X.  Replaces, around the
// existing GEMM (the LSTM's input and recurrent products, the joint head):
//   * torch.nn.LSTM's cell, forward and backward           dyn_lstm_cell_fwd / dyn_lstm_cell_bwd (pointwise, gate order i, f, g, o)
//   * ACT2FN["relu"](encoder + decoder) and its autograd    dyn_joint_fwd / dyn_joint_bwd (the broadcast sum over [B, T, U + 1, Hd])
//   * tdt_loss: log_softmax of the token and duration logits, the gather of the blank / label columns, the anti-diagonal lattice and,
//     through autograd, its gradient                        dyn_tdt_loss (arc log-probs, alpha / beta, arc posteriors -> dlogits)
//     The same three passes for a joint that is never whole: dyn_tdt_arcs_chunk (the arc log-probs of the frames [t0, t0 + Tc) into a
//     caller-owned lattice state), dyn_tdt_lattice_run (alpha / beta and the reduction on that state), dyn_tdt_grad_chunk (dlogits of
//     a chunk), and dyn_joint_bwd_chunk (de of a chunk's frames, dp accumulated over the chunks in launch order).  One set of
//     kernels: the whole forms are the chunk forms at t0 = 0, Tc = T, so every output is bit-equal whatever the chunking.
//   * ParakeetTDTGenerationMixin's greedy loop              dyn_tdt_greedy_steps (all state on the device, no host round trip per token)
// and the plain RNN-T head of ParakeetForRNNT and the Nemotron models (dyn_rnnt_*): the same code without the duration head.  One
// LatticeDims / state layout / host path; the arcs and gradient kernels are templates on DUR (a duration head or none), the only
// compile-time switch; the lattice and the greedy pick keep one kernel per head (see the RNN-T section below).
//
// fp32 throughout, every sum in a fixed order, no float atomics; argument errors come back as codes before any launch.
//
// The lattice.  alpha(t, u) of a 300 x 40 lattice is a few hundred nats below zero: kept as such, every addition would round at
// ulp(|alpha|) ~ 3e-5 and the posteriors exp(alpha + lp + beta - ll) would carry that error.  Each anti-diagonal n = t + u is
// therefore stored relative to an INTEGER base: base(n) = base(n - 1) + rint(max of the stored values of diagonal n - 1), so stored values
// near the diagonal's maximum are O(1), differences of bases are exact in fp32 (integers below 2^24) and the log-likelihood is kept as
// (integer part, fraction).  The diagonal's maximum travels through LDS in front of the one barrier the diagonal needs anyway: every
// thread reads the wave maxima of the previous diagonal after that barrier.  Diagonals are strided across the workgroup's threads; one
// workgroup per batch row and direction (blockIdx.y = 0: alpha, 1: beta), both directions in one launch.  Stored alpha / beta live in
// global memory ([B, T, U + 1], the gradient kernel reads them); a diagonal reads cells of up to 2 * D earlier diagonals, written by
// other threads of the same workgroup before earlier barriers (__syncthreads orders global memory at workgroup scope).
#include "common.h"

namespace {

constexpr int MAX_DUR = 8;
constexpr int LATTICE_T = 256;   // threads of a lattice workgroup at most: a longer diagonal is strided over them (the barrier of a small workgroup is the cheaper one)
constexpr int WPB = 4;          // waves per workgroup of the row kernels (one row per wave, layernorm_row.h's pattern)

struct Durs { int32_t n; int32_t d[MAX_DUR]; };

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- LSTM cell ------------------------------------------------------------------------------------------------------------
// gates = xg + hg ([Bd, 4 Hd] each, i | f | g | o), c = f * c_prev + i * g, h = o * tanh(c).
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(const float* __restrict__ xg, const float* __restrict__ hg,
                                                            const float* __restrict__ c_prev, float* __restrict__ c, float* __restrict__ h,
                                                            float* __restrict__ gates, int64_t Bd, int64_t Hd) {
    const int64_t n = Bd * Hd;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = idx / Hd, j = idx - b * Hd;
        const float* xr = xg + b * 4 * Hd;
        const float* hr = hg + b * 4 * Hd;
        const float gi = sigm(xr[j] + hr[j]);
        const float gf = sigm(xr[Hd + j] + hr[Hd + j]);
        const float gg = tanhf(xr[2 * Hd + j] + hr[2 * Hd + j]);
        const float go = sigm(xr[3 * Hd + j] + hr[3 * Hd + j]);
        const float cp = c_prev ? c_prev[idx] : 0.f;
        const float cn = gf * cp + gi * gg;
        c[idx] = cn;
        h[idx] = go * tanhf(cn);
        if (gates) {
            float* gr = gates + b * 4 * Hd;
            gr[j] = gi; gr[Hd + j] = gf; gr[2 * Hd + j] = gg; gr[3 * Hd + j] = go;
        }
    }
}

// From dh, dc_next (null: zeros), the saved gate activations, c_prev (null: zeros) and c: the gate pre-activation gradients
// dgates [Bd, 4 Hd] and dc_prev.
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ dc_next,
                                                            const float* __restrict__ gates, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c, float* __restrict__ dgates,
                                                            float* __restrict__ dc_prev, int64_t Bd, int64_t Hd) {
    const int64_t n = Bd * Hd;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = idx / Hd, j = idx - b * Hd;
        const float* gr = gates + b * 4 * Hd;
        const float gi = gr[j], gf = gr[Hd + j], gg = gr[2 * Hd + j], go = gr[3 * Hd + j];
        const float tc = tanhf(c[idx]);
        const float d_h = dh[idx];
        const float dc = (dc_next ? dc_next[idx] : 0.f) + d_h * go * (1.f - tc * tc);
        const float cp = c_prev ? c_prev[idx] : 0.f;
        float* dg = dgates + b * 4 * Hd;
        dg[j] = dc * gg * gi * (1.f - gi);
        dg[Hd + j] = dc * cp * gf * (1.f - gf);
        dg[2 * Hd + j] = dc * gi * (1.f - gg * gg);
        dg[3 * Hd + j] = d_h * tc * go * (1.f - go);
        dc_prev[idx] = dc * gf;
    }
}

// ---- joint input ----------------------------------------------------------------------------------------------------------
// z[b, t, u, :] = relu(e[b, t, :] + p[b, u, :]); p_sb = 0: one p shared by every batch row.  float4 per thread.
__global__ __launch_bounds__(256) void joint_fwd_kernel(const float* __restrict__ e, const float* __restrict__ p, float* __restrict__ z,
                                                        int64_t B, int64_t T, int64_t U1, int64_t H4, int64_t p_sb, int64_t p_su) {
    const int64_t n = B * T * U1 * H4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t h = idx % H4, r = idx / H4, u = r % U1, bt = r / U1, b = bt / T;
        const float4 a = reinterpret_cast<const float4*>(e)[bt * H4 + h];
        const float4 q = reinterpret_cast<const float4*>(p + b * p_sb + u * p_su)[h];
        reinterpret_cast<float4*>(z)[idx] = make_float4(fmaxf(a.x + q.x, 0.f), fmaxf(a.y + q.y, 0.f), fmaxf(a.z + q.z, 0.f), fmaxf(a.w + q.w, 0.f));
    }
}

__device__ __forceinline__ void acc_masked(float4& s, const float4 g, const float4 zz) {
    s.x += zz.x > 0.f ? g.x : 0.f; s.y += zz.y > 0.f ? g.y : 0.f; s.z += zz.z > 0.f ? g.z : 0.f; s.w += zz.w > 0.f ? g.w : 0.f;
}

// de[b, t, :] = sum_u dz * [z > 0], u ascending; de rows of one b are contiguous, batch rows de_sb4 float4 apart (T * H4: the whole
// tensor; more: the frames [t0, t0 + T) of a longer one, the chunk form)
__global__ __launch_bounds__(256) void joint_bwd_e_kernel(const float* __restrict__ dz, const float* __restrict__ z, float* __restrict__ de,
                                                          int64_t B, int64_t T, int64_t U1, int64_t H4, int64_t de_sb4) {
    const int64_t n = B * T * H4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t h = idx % H4, bt = idx / H4, b = bt / T, t = bt - b * T;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t u = 0; u < U1; ++u) {
            const int64_t o = (bt * U1 + u) * H4 + h;
            acc_masked(s, reinterpret_cast<const float4*>(dz)[o], reinterpret_cast<const float4*>(z)[o]);
        }
        reinterpret_cast<float4*>(de)[b * de_sb4 + t * H4 + h] = s;
    }
}

// dp[b, u, :] = sum_t dz * [z > 0], t ascending; shared: one dp row set, summed over b (ascending, outer) as well.  accumulate: the
// sum of these frames is added to what dp holds (the chunk form: one launch per chunk of frames, in stream order)
__global__ __launch_bounds__(256) void joint_bwd_p_kernel(const float* __restrict__ dz, const float* __restrict__ z, float* __restrict__ dp,
                                                          int64_t B, int64_t T, int64_t U1, int64_t H4, int shared, int64_t dp_sb, int64_t dp_su,
                                                          int accumulate) {
    const int64_t Bo = shared ? 1 : B, n = Bo * U1 * H4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t h = idx % H4, r = idx / H4, u = r % U1, bo = r / U1;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        const int64_t b0 = shared ? 0 : bo, b1 = shared ? B : bo + 1;
        for (int64_t b = b0; b < b1; ++b)
            for (int64_t t = 0; t < T; ++t) {
                const int64_t o = ((b * T + t) * U1 + u) * H4 + h;
                acc_masked(s, reinterpret_cast<const float4*>(dz)[o], reinterpret_cast<const float4*>(z)[o]);
            }
        float4* out = reinterpret_cast<float4*>(dp + bo * dp_sb + u * dp_su) + h;
        if (accumulate) {
            const float4 was = *out;
            s = make_float4(was.x + s.x, was.y + s.y, was.z + s.z, was.w + s.w);
        }
        *out = s;
    }
}

// ---- arc log-probabilities -------------------------------------------------------------------------------------------------
// One set of dimensions for both transducer heads.  durs.n == 0: a plain RNN-T lattice (ParakeetForRNNT), N == V1, sigma unused.
struct LatticeDims {
    int64_t B, T, U1;       // the lattice [B, T, U1]
    int64_t t0, Tc;         // the row kernels' logits [B, Tc, U1, N] hold the frames [t0, t0 + Tc) (0, T: the whole lattice; a chunk may overhang T)
    int64_t V1, N;          // V1 = V + 1 token classes (the blank among them), N = V1 + D
    int64_t S;              // targets [B, S]
    int32_t blank;
    float sigma;
    Durs durs;
};

__device__ __forceinline__ int row_T(const int32_t* ilen, int64_t b, const LatticeDims& d) { return clampi(ilen[b], 0, (int)d.T); }
__device__ __forceinline__ int row_U(const int32_t* tlen, int64_t b, const LatticeDims& d) {
    return clampi(tlen[b], 0, (int)(d.U1 - 1 < d.S ? d.U1 - 1 : d.S));
}
__device__ __forceinline__ int target_of(const int32_t* targets, int64_t b, int u, const LatticeDims& d) {
    const int k = targets[b * d.S + u];
    return k < 0 ? 0 : (k >= d.V1 ? (int)d.V1 - 1 : k);               // ids are validated on the host; never read outside the row
}

// One wave per logits row (b, tc, u) of the frames [t0, t0 + Tc): lp[cell] = (blank, label) log-probs (label -inf at u >= U_b),
// lse[cell] = the token log-sum-exp of the lattice cell (b, t0 + tc, u).  DUR (a duration head, TDT): the D duration log-probs behind
// lp's two, the duration log-sum-exp behind lse's one, sigma taken off the token log-probs.  Rows of a chunk past the lattice's last
// frame are skipped.
template <bool DUR>
__global__ __launch_bounds__(64 * WPB) void arcs_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                        const int32_t* __restrict__ tlen, float* __restrict__ lp, float* __restrict__ lse,
                                                        LatticeDims d) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t rows = d.B * d.Tc * d.U1;
    for (int64_t crow = (int64_t)blockIdx.x * WPB + w; crow < rows; crow += (int64_t)gridDim.x * WPB) {
        const int64_t u = crow % d.U1, b = crow / (d.U1 * d.Tc), t = d.t0 + (crow / d.U1) % d.Tc;
        if (t >= d.T) continue;                                       // wave-uniform
        const int64_t row = (b * d.T + t) * d.U1 + u;                 // the lattice cell
        const float* x = logits + crow * d.N;
        float m = -INFINITY;
        for (int c = lane; c < d.V1; c += 64) m = fmaxf(m, x[c]);
        m = dyn::wave_max(m);
        float s = 0.f;
        for (int c = lane; c < d.V1; c += 64) s += expf(x[c] - m);
        s = dyn::wave_sum(s);
        const float lt = m + logf(s);
        if constexpr (DUR) {
            // durations: D <= 8 values, one lane each
            const int D = d.durs.n;
            const float dv = lane < D ? x[d.V1 + lane] : -INFINITY;
            const float dm = dyn::wave_max(dv);
            const float ds = dyn::wave_sum(lane < D ? expf(dv - dm) : 0.f);
            const float ld = dm + logf(ds);
            float* o = lp + row * (2 + D);
            if (lane == 0) {
                o[0] = x[d.blank] - lt - d.sigma;
                o[1] = u < row_U(tlen, b, d) ? x[target_of(targets, b, (int)u, d)] - lt - d.sigma : -INFINITY;
                lse[2 * row] = lt;
                lse[2 * row + 1] = ld;
            }
            if (lane < D) o[2 + lane] = dv - ld;
        } else if (lane == 0) {
            lp[2 * row] = x[d.blank] - lt;
            lp[2 * row + 1] = u < row_U(tlen, b, d) ? x[target_of(targets, b, (int)u, d)] - lt : -INFINITY;
            lse[row] = lt;
        }
    }
}

// ---- lattice ---------------------------------------------------------------------------------------------------------------
// State per row b: lp [T, U1, 2 + D], lse [T, U1, 2] (D == 0: [T, U1]), alpha, beta [T, U1] (stored relative to the bases), abase, bbase
// [T + U1] (floats holding integers), ll [2] = (integer part, fraction) of the row's log-likelihood, -inf fraction when the terminal is
// unreachable, nll.  Per cell 20 bytes without a duration head, 44 at D = 5.
struct LatticeWs { float* lp; float* lse; float* alpha; float* beta; float* abase; float* bbase; float* ll; float* nll; int64_t total; };

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

LatticeWs carve(void* ws, int64_t B, int64_t T, int64_t U1, int64_t D) {
    LatticeWs w;
    char* p = (char*)ws;
    int64_t off = 0;
    const int64_t cells = B * T * U1;
    w.lp = (float*)(p + off); off += align_up(cells * (2 + D) * 4, 256);
    w.lse = (float*)(p + off); off += align_up(cells * (D > 0 ? 2 : 1) * 4, 256);
    w.alpha = (float*)(p + off); off += align_up(cells * 4, 256);
    w.beta = (float*)(p + off); off += align_up(cells * 4, 256);
    w.abase = (float*)(p + off); off += align_up(B * (T + U1) * 4, 256);
    w.bbase = (float*)(p + off); off += align_up(B * (T + U1) * 4, 256);
    w.ll = (float*)(p + off); off += align_up(B * 2 * 4, 256);
    w.nll = (float*)(p + off); off += align_up(B * 4, 256);
    w.total = off;
    return w;
}

// the workgroup's maximum of diagonal `n`: wave maxima into wmax[n & 1][.] BEFORE the diagonal's barrier, read by everyone AFTER it
__device__ __forceinline__ void publish_max(float v, float (*wmax)[16], int n) {
    v = dyn::wave_max(v);
    if ((threadIdx.x & 63) == 0) wmax[n & 1][threadIdx.x >> 6] = v;
}
__device__ __forceinline__ float read_max(float (*wmax)[16], int n) {
    float m = -INFINITY;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) m = fmaxf(m, wmax[n & 1][i]);
    return m;
}

__device__ __forceinline__ float lse_of(const float* c, int k) {
    float m = -INFINITY;
    for (int i = 0; i < k; ++i) m = fmaxf(m, c[i]);
    if (m == -INFINITY) return -INFINITY;
    float s = 0.f;
    for (int i = 0; i < k; ++i) s += expf(c[i] - m);
    return m + logf(s);
}

__global__ __launch_bounds__(LATTICE_T) void tdt_lattice_kernel(const float* __restrict__ lp, const int32_t* __restrict__ ilen,
                                                           const int32_t* __restrict__ tlen, float* alpha, float* beta, float* abase,
                                                           float* bbase, float* ll_out, float* __restrict__ nll, LatticeDims d) {
    __shared__ float wmax[2][16];       // LATTICE_T / 64 wave maxima per diagonal, double-buffered
    const int64_t b = blockIdx.x;
    const int U1 = (int)d.U1, D = d.durs.n, C = 2 + D;
    const int T = row_T(ilen, b, d), U = row_U(tlen, b, d);      // lengths are device data: clamped into the tensor
    const float* lpb = lp + b * d.T * d.U1 * C;
    const int ND = T + U;                       // diagonals 0 .. T + U - 1
    float cand[2 * MAX_DUR];
    if (blockIdx.y == 0) {
        float* al = alpha + b * d.T * d.U1;
        float* bs = abase + b * (d.T + d.U1);
        float base = 0.f;
        for (int n = 0; n < ND; ++n) {
            if (n > 0) {
                const float mx = read_max(wmax, n - 1);
                if (mx > -INFINITY) base += rintf(mx);
            }
            if (threadIdx.x == 0) bs[n] = base;
            float off_b[MAX_DUR], off_l[MAX_DUR];     // base of the source diagonal minus this one's (blank arcs: n - dur; label arcs: n - dur - 1)
            for (int i = 0; i < D; ++i) {
                const int nb_ = n - d.durs.d[i];
                off_b[i] = d.durs.d[i] > 0 && nb_ >= 0 ? bs[nb_] - base : 0.f;
                off_l[i] = nb_ - 1 >= 0 ? bs[nb_ - 1] - base : 0.f;
            }
            float tmax = -INFINITY;
            const int u_lo = n - T + 1 > 0 ? n - T + 1 : 0, u_hi = n < U ? n : U;
            for (int u = u_lo + (int)threadIdx.x; u <= u_hi; u += blockDim.x) {
                const int t = n - u;
                float v = 0.f;
                if (n > 0) {
                    int k = 0;
                    for (int i = 0; i < D; ++i) {
                        const int dur = d.durs.d[i], tp = t - dur;
                        if (tp < 0) continue;
                        if (dur > 0) {
                            const int64_t s = (int64_t)tp * U1 + u;
                            cand[k++] = al[s] + off_b[i] + lpb[s * C] + lpb[s * C + 2 + i];
                        }
                        if (u > 0) {
                            const int64_t s = (int64_t)tp * U1 + u - 1;
                            cand[k++] = al[s] + off_l[i] + lpb[s * C + 1] + lpb[s * C + 2 + i];
                        }
                    }
                    v = lse_of(cand, k);
                }
                al[(int64_t)t * U1 + u] = v;
                tmax = fmaxf(tmax, v);
            }
            publish_max(tmax, wmax, n);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            // terminal: blank arcs (dur > 0) from (T - dur, U); the integer part is the base of the largest term's diagonal
            float li = 0.f, lf = -INFINITY;
            int k = 0;
            float tb[MAX_DUR];
            for (int i = 0; i < D; ++i) {
                const int dur = d.durs.d[i], t = T - dur;
                if (dur <= 0 || t < 0 || T <= 0) continue;
                const int64_t s = (int64_t)t * U1 + U;
                cand[k] = al[s] + lpb[s * C] + lpb[s * C + 2 + i];
                tb[k] = bs[t + U];
                ++k;
            }
            int best = -1;
            for (int i = 0; i < k; ++i)
                if (cand[i] > -INFINITY && (best < 0 || cand[i] + tb[i] > cand[best] + tb[best])) best = i;
            if (best >= 0) {
                li = tb[best];
                for (int i = 0; i < k; ++i) cand[i] += tb[i] - li;
                lf = lse_of(cand, k);
            }
            ll_out[2 * b] = li;
            ll_out[2 * b + 1] = lf;
            nll[b] = lf > -INFINITY ? -(li + lf) : INFINITY;
        }
    } else {
        float* be = beta + b * d.T * d.U1;
        float* bs = bbase + b * (d.T + d.U1);
        float base = 0.f;
        for (int n = ND - 1; n >= 0; --n) {
            if (n < ND - 1) {
                const float mx = read_max(wmax, n + 1);
                if (mx > -INFINITY) base += rintf(mx);
            }
            if (threadIdx.x == 0) bs[n] = base;
            float off_b[MAX_DUR], off_l[MAX_DUR];     // blank arcs land on diagonal n + dur, label arcs on n + dur + 1
            for (int i = 0; i < D; ++i) {
                const int nb_ = n + d.durs.d[i];
                off_b[i] = d.durs.d[i] > 0 && nb_ < ND ? bs[nb_] - base : 0.f;
                off_l[i] = nb_ + 1 < ND ? bs[nb_ + 1] - base : 0.f;
            }
            float tmax = -INFINITY;
            const int u_lo = n - T + 1 > 0 ? n - T + 1 : 0, u_hi = n < U ? n : U;
            for (int u = u_lo + (int)threadIdx.x; u <= u_hi; u += blockDim.x) {
                const int t = n - u;
                const int64_t s = (int64_t)t * U1 + u;
                const float lb = lpb[s * C], ll = lpb[s * C + 1];
                int k = 0;
                for (int i = 0; i < D; ++i) {
                    const int dur = d.durs.d[i], tn = t + dur;
                    const float ld = lpb[s * C + 2 + i];
                    if (dur > 0) {
                        if (tn == T && u == U) cand[k++] = lb + ld - base;                      // the terminal, absolute 0
                        else if (tn < T) cand[k++] = lb + ld + be[(int64_t)tn * U1 + u] + off_b[i];
                    }
                    if (u < U && tn < T) cand[k++] = ll + ld + be[(int64_t)tn * U1 + u + 1] + off_l[i];
                }
                const float v = lse_of(cand, k);
                be[s] = v;
                tmax = fmaxf(tmax, v);
            }
            publish_max(tmax, wmax, n);
            __syncthreads();
        }
    }
}

// ==== RNN-T (ParakeetForRNNT, `model_type: "parakeet_rnnt"`) =================================================================
// The plain transducer lattice of transformers.loss.loss_rnnt.rnnt_loss (a wrapper around torchaudio.functional.rnnt_loss): no
// duration head (durs.n == 0, N == V1), from (t, u) a blank arc to (t + 1, u) and a label arc to (t, u + 1), the terminal
// alpha(T - 1, U) + lp_blank(T - 1, U).  Every arc advances the anti-diagonal by exactly one, so a diagonal reads only the one before it
// and the base difference it needs is the rint() it has just taken: the integer-base scheme of the TDT lattice above with one source
// diagonal, its offset kept in a register where tdt_lattice_kernel reads up to 2 * D bases from memory.  That is why this lattice has a
// body of its own; everything around it (dimensions, state layout, arcs and gradient kernels, reduction, host path, the greedy LSTM /
// projector / joint kernels) is the TDT head's code at D = 0.

// log(exp(a) + exp(b)), -inf when both are
__device__ __forceinline__ float lse2(float a, float b) {
    const float c[2] = {a, b};
    return lse_of(c, 2);
}

__global__ __launch_bounds__(LATTICE_T) void rnnt_lattice_kernel(const float* __restrict__ lp, const int32_t* __restrict__ ilen,
                                                                 const int32_t* __restrict__ tlen, float* alpha, float* beta, float* abase,
                                                                 float* bbase, float* ll_out, float* __restrict__ nll, LatticeDims d) {
    __shared__ float wmax[2][16];
    const int64_t b = blockIdx.x;
    const int U1 = (int)d.U1;
    const int T = row_T(ilen, b, d), U = row_U(tlen, b, d);
    const float* lpb = lp + b * d.T * d.U1 * 2;
    const int ND = T > 0 ? T + U : 0;           // diagonals 0 .. T + U - 1; T_b == 0: no cell, no terminal
    if (blockIdx.y == 0) {
        float* al = alpha + b * d.T * d.U1;
        float* bs = abase + b * (d.T + d.U1);
        float base = 0.f;
        for (int n = 0; n < ND; ++n) {
            float off = 0.f;                    // base of diagonal n - 1 minus this one's
            if (n > 0) {
                const float mx = read_max(wmax, n - 1);
                if (mx > -INFINITY) off = -rintf(mx);
            }
            base -= off;
            if (threadIdx.x == 0) bs[n] = base;
            float tmax = -INFINITY;
            const int u_lo = n - T + 1 > 0 ? n - T + 1 : 0, u_hi = n < U ? n : U;
            for (int u = u_lo + (int)threadIdx.x; u <= u_hi; u += blockDim.x) {
                const int t = n - u;
                float v = 0.f;
                if (n > 0) {
                    float cb = -INFINITY, cl = -INFINITY;
                    if (t > 0) {
                        const int64_t s = (int64_t)(t - 1) * U1 + u;
                        cb = al[s] + off + lpb[2 * s];
                    }
                    if (u > 0) {
                        const int64_t s = (int64_t)t * U1 + u - 1;
                        cl = al[s] + off + lpb[2 * s + 1];
                    }
                    v = lse2(cb, cl);
                }
                al[(int64_t)t * U1 + u] = v;
                tmax = fmaxf(tmax, v);
            }
            publish_max(tmax, wmax, n);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            float lf = -INFINITY;
            if (T > 0) {
                const int64_t s = (int64_t)(T - 1) * U1 + U;
                lf = al[s] + lpb[2 * s];
            }
            ll_out[2 * b] = base;
            ll_out[2 * b + 1] = lf;
            nll[b] = lf > -INFINITY ? -(base + lf) : INFINITY;
        }
    } else {
        float* be = beta + b * d.T * d.U1;
        float* bs = bbase + b * (d.T + d.U1);
        float base = 0.f;
        for (int n = ND - 1; n >= 0; --n) {
            float off = 0.f;                    // base of diagonal n + 1 minus this one's
            if (n < ND - 1) {
                const float mx = read_max(wmax, n + 1);
                if (mx > -INFINITY) off = -rintf(mx);
            }
            base -= off;
            if (threadIdx.x == 0) bs[n] = base;
            float tmax = -INFINITY;
            const int u_lo = n - T + 1 > 0 ? n - T + 1 : 0, u_hi = n < U ? n : U;
            for (int u = u_lo + (int)threadIdx.x; u <= u_hi; u += blockDim.x) {
                const int t = n - u;
                const int64_t s = (int64_t)t * U1 + u;
                float v;
                if (t == T - 1 && u == U) {
                    v = lpb[2 * s];                                   // the terminal, absolute 0 behind it (base is 0 here)
                } else {
                    float cb = -INFINITY, cl = -INFINITY;
                    if (t + 1 < T) cb = lpb[2 * s] + be[s + U1] + off;
                    if (u < U) cl = lpb[2 * s + 1] + be[s + 1] + off;
                    v = lse2(cb, cl);
                }
                be[s] = v;
                tmax = fmaxf(tmax, v);
            }
            publish_max(tmax, wmax, n);
            __syncthreads();
        }
    }
}

// d loss / d nll_b of the reduction (tdt_loss's five; "none" as "sum")
__device__ __forceinline__ float row_weight(int reduction, const int32_t* tlen, int64_t B, int64_t b) {
    if (reduction == 1) return 1.f / (float)B;                                   // mean_batch
    if (reduction == 2) return 1.f / ((float)tlen[b] * (float)B);                // mean
    if (reduction == 3) {                                                        // mean_volume
        float s = 0.f;
        for (int64_t i = 0; i < B; ++i) s += (float)tlen[i];
        return 1.f / s;
    }
    return 1.f;
}

__global__ void tdt_loss_reduce_kernel(const float* __restrict__ nll, const int32_t* __restrict__ tlen, float* loss, int64_t B, int reduction) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.f, vol = 0.f;
    for (int64_t b = 0; b < B; ++b) {
        s += reduction == 2 ? nll[b] / (float)tlen[b] : nll[b];
        vol += (float)tlen[b];
    }
    *loss = reduction == 1 || reduction == 2 ? s / (float)B : (reduction == 3 ? s / vol : s);
}

// ---- gradient --------------------------------------------------------------------------------------------------------------
// One wave per logits row (b, t, u).  With the arc posteriors g_b[i] (blank arc of duration i), g_l[i] (label arc), Gb = sum g_b,
// Gl = sum g_l: dtoken[v] = softmax_v * (Gb + Gl) - Gb [v = blank] - Gl [v = target], ddur[i] = softmax_i * (Gb + Gl) - g_b[i] - g_l[i],
// times grad_scale * row weight.  Rows at t >= T_b or u > U_b, and every row of an unreachable lattice, are zeros.  grad may be logits.
// logits / grad hold the frames [t0, t0 + Tc) ([B, Tc, U1, N]); lp, lse, alpha, beta are the whole lattice's.
// DUR: lane i < D holds the posteriors of duration i, summed in a fixed order.  Without a duration head there is one blank arc
// (to (t + 1, u); beta = 0 behind the terminal cell (T - 1, U)) and one label arc (to (t, u + 1)): Gb and Gl themselves, wave-uniform.
template <bool DUR>
__global__ __launch_bounds__(64 * WPB) void grad_kernel(const float* logits, const int32_t* __restrict__ targets,
                                                        const int32_t* __restrict__ ilen, const int32_t* __restrict__ tlen,
                                                        const float* __restrict__ lp, const float* __restrict__ lse,
                                                        const float* __restrict__ alpha, const float* __restrict__ beta,
                                                        const float* __restrict__ abase, const float* __restrict__ bbase,
                                                        const float* __restrict__ ll, float* grad, float grad_scale, int reduction, LatticeDims d) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t rows = d.B * d.Tc * d.U1;
    for (int64_t row = (int64_t)blockIdx.x * WPB + w; row < rows; row += (int64_t)gridDim.x * WPB) {
        const int u = (int)(row % d.U1);
        const int64_t b = row / (d.U1 * d.Tc), tt = d.t0 + (row / d.U1) % d.Tc;      // a chunk's frame may lie past the lattice: zeros
        const int t = (int)(tt < d.T ? tt : d.T);
        const int T = row_T(ilen, b, d), U = row_U(tlen, b, d);
        const float* x = logits + row * d.N;
        float* g = grad + row * d.N;
        const float li = ll[2 * b], lf = ll[2 * b + 1];
        if (t >= T || u > U || !(lf > -INFINITY)) {
            for (int c = lane; c < d.N; c += 64) g[c] = 0.f;
            continue;
        }
        const int n = t + u;
        const int64_t cell = (b * d.T + t) * d.U1 + u;
        const float* ab = abase + b * (d.T + d.U1);
        const float* bb = bbase + b * (d.T + d.U1);
        const float a = alpha[cell], abn = ab[n];
        float gb = 0.f, gl = 0.f;        // DUR: this lane's duration; else the row's two arcs, every lane the same
        float Gb = 0.f, Gl = 0.f;
        if constexpr (DUR) {
            const int D = d.durs.n, U1 = (int)d.U1, ND = T + U;
            const float* be = beta + b * d.T * d.U1;
            const float* lpc = lp + cell * (2 + D);
            const float lb = lpc[0], llab = lpc[1];
            // uniform control flow: every lane evaluates its own duration or nothing
            if (lane < D && a > -INFINITY) {
                const int dur = d.durs.d[lane], tn = t + dur;
                const float ld = lpc[2 + lane];
                if (dur > 0) {
                    float e = -INFINITY;
                    if (tn == T && u == U) e = a + lb + ld + ((abn - li) - lf);
                    else if (tn < T) e = a + lb + ld + be[(int64_t)tn * U1 + u] + ((abn + bb[n + dur] - li) - lf);
                    gb = e > -INFINITY ? expf(e) : 0.f;
                }
                if (u < U && tn < T && n + dur + 1 < ND) {
                    const float e = a + llab + ld + be[(int64_t)tn * U1 + u + 1] + ((abn + bb[n + dur + 1] - li) - lf);
                    gl = e > -INFINITY ? expf(e) : 0.f;
                }
            }
            for (int i = 0; i < D; ++i) {        // fixed order: duration 0, 1, ..
                Gb += __shfl(gb, i, 64);
                Gl += __shfl(gl, i, 64);
            }
        } else {
            if (a > -INFINITY) {
                const float lb = lp[2 * cell], llab = lp[2 * cell + 1];
                float e = -INFINITY;
                if (t == T - 1 && u == U) e = a + lb + ((abn - li) - lf);
                else if (t + 1 < T) e = a + lb + beta[cell + d.U1] + ((abn + bb[n + 1] - li) - lf);
                gb = e > -INFINITY ? expf(e) : 0.f;
                if (u < U) {
                    e = a + llab + beta[cell + 1] + ((abn + bb[n + 1] - li) - lf);
                    gl = e > -INFINITY ? expf(e) : 0.f;
                }
            }
            Gb = gb;
            Gl = gl;
        }
        const float G = Gb + Gl;
        const float sc = grad_scale * row_weight(reduction, tlen, d.B, b);
        const float lt = lse[DUR ? 2 * cell : cell];
        const int tgt = u < U ? target_of(targets, b, u, d) : -1;
        for (int c = lane; c < d.V1; c += 64) {
            float v = expf(x[c] - lt) * G;
            if (c == d.blank) v -= Gb;
            if (c == tgt) v -= Gl;
            g[c] = v * sc;
        }
        if constexpr (DUR)
            if (lane < d.durs.n) g[d.V1 + lane] = (expf(x[d.V1 + lane] - lse[2 * cell + 1]) * G - (gb + gl)) * sc;
    }
}

// ---- greedy TDT decode -----------------------------------------------------------------------------------------------------
struct GreedyArgs {
    const float* enc;            // [B, T, Hd] projected encoder states
    const int32_t* valid;        // [B] valid frames per row
    const float* embed;          // [V1, Hd]
    const float* const* lstm;    // device array [4 * L]: w_ih, w_hh, b_ih, b_hh per layer
    const float* proj_w; const float* proj_b;     // [Hd, Hd], [Hd]
    const float* head_w; const float* head_b;     // [N, Hd], [N]
    int32_t* istate;             // [6, B]: frame, last token, emit flag, done flag, count, steps; RNN-T [7, B]: the symbols of the frame
    float* h; float* c; float* h_new;             // [L, B, Hd] each
    float* dec;                  // [B, Hd] cached projector output
    float* logits;               // [B, N]
    int32_t* tokens; int32_t* frames;             // [B, n_max]
    int32_t B, T, Hd, L, V1, N, blank, n_max, max_steps;
    Durs durs;
};

__device__ __forceinline__ int32_t* ist(const GreedyArgs& a, int which) { return a.istate + (int64_t)which * a.B; }
enum { S_FRAME = 0, S_TOKEN = 1, S_EMIT = 2, S_DONE = 3, S_COUNT = 4, S_STEPS = 5, S_SYMBOLS = 6 };

__device__ __forceinline__ float wave_dot(const float* __restrict__ w, const float* __restrict__ x, int K, int lane) {
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s = fmaf(w[k], x[k], s);
    return dyn::wave_sum(s);
}

// LSTM layer `l` of the rows that emitted: one wave per hidden unit j computes its four gate rows over [x ; h] and the cell update.
// x = the embedding of the last token (layer 0) or h_new of the layer below.  c in place (unit j is this wave's alone), h into h_new.
__global__ __launch_bounds__(256) void greedy_lstm_kernel(const GreedyArgs a, int l) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, j = blockIdx.x * 4 + w;
    if (j >= a.Hd || ist(a, S_DONE)[b] || !ist(a, S_EMIT)[b]) return;
    const int Hd = a.Hd;
    int tok = ist(a, S_TOKEN)[b];
    tok = tok < 0 ? 0 : (tok >= a.V1 ? a.V1 - 1 : tok);
    const float* x = l == 0 ? a.embed + (int64_t)tok * Hd : a.h_new + ((int64_t)(l - 1) * a.B + b) * Hd;
    const int64_t so = ((int64_t)l * a.B + b) * Hd;
    const float* hp = a.h + so;
    const float* wi = a.lstm[4 * l], * wh = a.lstm[4 * l + 1], * bi = a.lstm[4 * l + 2], * bh = a.lstm[4 * l + 3];
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = (int64_t)q * Hd + j;
        g[q] = wave_dot(wi + r * Hd, x, Hd, lane) + bi[r] + (wave_dot(wh + r * Hd, hp, Hd, lane) + bh[r]);
    }
    if (lane == 0) {
        const float gi = sigm(g[0]), gf = sigm(g[1]), gg = tanhf(g[2]), go = sigm(g[3]);
        const float cn = gf * a.c[so + j] + gi * gg;
        a.c[so + j] = cn;
        a.h_new[so + j] = go * tanhf(cn);
    }
}

// dec = proj_w . h_new[L - 1] + proj_b of the rows that emitted; workgroup column 0 also commits h_new -> h for every layer (nothing in
// this launch reads h).
__global__ __launch_bounds__(256) void greedy_proj_kernel(const GreedyArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, j = blockIdx.x * 4 + w;
    if (ist(a, S_DONE)[b] || !ist(a, S_EMIT)[b]) return;
    const int Hd = a.Hd;
    if (blockIdx.x == 0)
        for (int l = 0; l < a.L; ++l) {
            const int64_t so = ((int64_t)l * a.B + b) * Hd;
            for (int k = threadIdx.x; k < Hd; k += blockDim.x) a.h[so + k] = a.h_new[so + k];
        }
    if (j >= Hd) return;
    const float* x = a.h_new + ((int64_t)(a.L - 1) * a.B + b) * Hd;
    const float s = wave_dot(a.proj_w + (int64_t)j * Hd, x, Hd, lane);
    if (lane == 0) a.dec[(int64_t)b * Hd + j] = s + a.proj_b[j];
}

// logits[b, n] = head_w[n] . relu(enc[b, frame_b] + dec[b]) + head_b[n]
__global__ __launch_bounds__(256) void greedy_joint_kernel(const GreedyArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, n = blockIdx.x * 4 + w;
    if (n >= a.N || ist(a, S_DONE)[b]) return;
    int f = ist(a, S_FRAME)[b];
    f = f < 0 ? 0 : (f >= a.T ? a.T - 1 : f);
    const float* e = a.enc + ((int64_t)b * a.T + f) * a.Hd;
    const float* dc = a.dec + (int64_t)b * a.Hd;
    const float* wr = a.head_w + (int64_t)n * a.Hd;
    float s = 0.f;
    for (int k = lane; k < a.Hd; k += 64) s = fmaf(wr[k], fmaxf(e[k] + dc[k], 0.f), s);
    s = dyn::wave_sum(s);
    if (lane == 0) a.logits[(int64_t)b * a.N + n] = s + a.head_b[n];
}

// The argmax of a workgroup of 256 over the V1 token logits x (first maximum wins; no finite maximum: the blank).  One barrier; the
// result is thread 0's alone.
__device__ __forceinline__ int token_argmax(const float* x, int V1, int blank) {
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = threadIdx.x; c < V1; c += blockDim.x)
        if (better(x[c], c, bv, bi)) { bv = x[c]; bi = c; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[w] = bv; ri[w] = bi; }
    __syncthreads();
    if (threadIdx.x != 0) return blank;
    for (int i = 1; i < 4; ++i)
        if (better(rv[i], ri[i], bv, bi)) { bv = rv[i]; bi = ri[i]; }
    return bi == 0x7fffffff ? blank : bi;
}

// argmax over the token and the duration logits (first maximum wins), then the step's bookkeeping: one workgroup per row
__global__ __launch_bounds__(256) void greedy_pick_kernel(const GreedyArgs a) {
    const int b = blockIdx.x;
    if (ist(a, S_DONE)[b]) return;                 // uniform: the flag is written after the barrier of token_argmax
    const float* x = a.logits + (int64_t)b * a.N;
    const int tok = token_argmax(x, a.V1, a.blank);
    if (threadIdx.x != 0) return;
    int di = 0;
    float dv = x[a.V1];
    for (int i = 1; i < a.durs.n; ++i)
        if (x[a.V1 + i] > dv) { dv = x[a.V1 + i]; di = i; }
    int adv = a.durs.d[di];
    const int frame = ist(a, S_FRAME)[b];
    const bool is_blank = tok == a.blank;
    if (is_blank && adv == 0) adv = 1;
    int count = ist(a, S_COUNT)[b];
    if (!is_blank && count < a.n_max) {
        a.tokens[(int64_t)b * a.n_max + count] = tok;
        a.frames[(int64_t)b * a.n_max + count] = frame;
        ++count;
    }
    const int steps = ist(a, S_STEPS)[b] + 1;
    ist(a, S_COUNT)[b] = count;
    ist(a, S_STEPS)[b] = steps;
    ist(a, S_EMIT)[b] = is_blank ? 0 : 1;
    ist(a, S_TOKEN)[b] = tok;
    ist(a, S_FRAME)[b] = frame + adv;
    if (frame + adv >= a.valid[b] || steps >= a.max_steps || count >= a.n_max) ist(a, S_DONE)[b] = 1;
}

// argmax over the row (first maximum wins), then ParakeetRNNTGenerationMixin._update_model_kwargs_for_generation: a blank advances the
// frame and resets the per-frame symbol counter; a non-blank is emitted and counted, and when the counter reaches max_symbols the frame
// advances anyway and the counter resets (the forced step's token is still emitted and fed to the prediction network).
// `frame_base`: added to the frame RECORDED with an emitted token (0 offline; the absolute frame of a streamed chunk's frame 0).
__global__ __launch_bounds__(256) void rnnt_greedy_pick_kernel(const GreedyArgs a, int max_symbols, int frame_base) {
    const int b = blockIdx.x;
    if (ist(a, S_DONE)[b]) return;                 // uniform: the flag is written after the barrier of token_argmax
    const int tok = token_argmax(a.logits + (int64_t)b * a.N, a.V1, a.blank);
    if (threadIdx.x != 0) return;
    const bool is_blank = tok == a.blank;
    const int frame = ist(a, S_FRAME)[b];
    const int symbols = is_blank ? 0 : ist(a, S_SYMBOLS)[b] + 1;
    const bool forced = symbols >= max_symbols;
    const int adv = is_blank || forced ? 1 : 0;
    int count = ist(a, S_COUNT)[b];
    if (!is_blank && count < a.n_max) {
        a.tokens[(int64_t)b * a.n_max + count] = tok;
        a.frames[(int64_t)b * a.n_max + count] = frame + frame_base;
        ++count;
    }
    const int steps = ist(a, S_STEPS)[b] + 1;
    ist(a, S_COUNT)[b] = count;
    ist(a, S_STEPS)[b] = steps;
    ist(a, S_EMIT)[b] = is_blank ? 0 : 1;
    ist(a, S_TOKEN)[b] = tok;
    ist(a, S_FRAME)[b] = frame + adv;
    ist(a, S_SYMBOLS)[b] = adv ? 0 : symbols;
    if (frame + adv >= a.valid[b] || steps >= a.max_steps || count >= a.n_max) ist(a, S_DONE)[b] = 1;
}

// A streamed decode moves on to the next chunk of encoder frames: the frame pointer back to 0, the done flags, the per-frame symbol
// counter and the chunk's output count and step count cleared.  h / c, the cached projector output, the last token and the emit flag stay.
__global__ void rnnt_greedy_rebase_kernel(const GreedyArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    ist(a, S_FRAME)[b] = 0;
    ist(a, S_DONE)[b] = 0;
    ist(a, S_COUNT)[b] = 0;
    ist(a, S_STEPS)[b] = 0;
    ist(a, S_SYMBOLS)[b] = 0;
}

int check_durs(const int32_t* durations, int64_t D, Durs& out, const char* who) {
    DYN_REQUIRE(durations && D >= 1 && D <= MAX_DUR, DYN_E_ARG, "%s: %lld durations (1 .. %d)", who, (long long)D, MAX_DUR);
    out.n = (int32_t)D;
    bool positive = false;
    for (int i = 0; i < MAX_DUR; ++i) out.d[i] = 0;
    for (int i = 0; i < D; ++i) {
        DYN_REQUIRE(durations[i] >= 0 && durations[i] < (1 << 20) && (i == 0 || durations[i] > durations[i - 1]), DYN_E_ARG,
                    "%s: durations must be non-negative and strictly ascending", who);
        out.d[i] = durations[i];
        positive = positive || durations[i] > 0;
    }
    DYN_REQUIRE(positive, DYN_E_ARG, "%s: no positive duration (no arc advances the frame)", who);
    return DYN_OK;
}

inline unsigned grid_for(int64_t n, int per_block, int64_t cap = 16384) {
    int64_t g = dyn::cdiv(n, per_block);
    return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int dyn_lstm_cell_fwd(const float* xg, const float* hg, const float* c_prev, float* c, float* h, float* gates, int64_t Bd,
                                 int64_t Hd, void* stream) {
    DYN_REQUIRE(xg && hg && c && h && Bd > 0 && Hd > 0, DYN_E_ARG, "dyn_lstm_cell_fwd: bad arguments");
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(grid_for(Bd * Hd, 256)), dim3(256), 0, (hipStream_t)stream, xg, hg, c_prev, c, h, gates, Bd, Hd);
    return dyn::check_launch("dyn_lstm_cell_fwd");
}

extern "C" int dyn_lstm_cell_bwd(const float* dh, const float* dc_next, const float* gates, const float* c_prev, const float* c,
                                 float* dgates, float* dc_prev, int64_t Bd, int64_t Hd, void* stream) {
    DYN_REQUIRE(dh && gates && c && dgates && dc_prev && Bd > 0 && Hd > 0, DYN_E_ARG, "dyn_lstm_cell_bwd: bad arguments");
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(grid_for(Bd * Hd, 256)), dim3(256), 0, (hipStream_t)stream, dh, dc_next, gates, c_prev, c,
                       dgates, dc_prev, Bd, Hd);
    return dyn::check_launch("dyn_lstm_cell_bwd");
}

extern "C" int dyn_joint_fwd(const float* e, const float* p, float* z, int64_t B, int64_t T, int64_t U1, int64_t Hd, int64_t p_stride_b,
                             int64_t p_stride_u, int32_t act, void* stream) {
    DYN_REQUIRE(act == 0, DYN_E_UNSUPPORTED, "dyn_joint_fwd: hidden_act %d is not built (0 = relu)", act);
    DYN_REQUIRE(e && p && z && B > 0 && T > 0 && U1 > 0 && Hd > 0 && Hd % 4 == 0 && p_stride_b >= 0 && p_stride_b % 4 == 0 &&
                    p_stride_u >= Hd && p_stride_u % 4 == 0, DYN_E_ARG, "dyn_joint_fwd: bad arguments (Hd and the strides are multiples of 4)");
    DYN_REQUIRE(!(((uintptr_t)e | (uintptr_t)p | (uintptr_t)z) & 15), DYN_E_ARG, "dyn_joint_fwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(joint_fwd_kernel, dim3(grid_for(B * T * U1 * (Hd / 4), 256)), dim3(256), 0, (hipStream_t)stream, e, p, z, B, T, U1,
                       Hd / 4, p_stride_b, p_stride_u);
    return dyn::check_launch("dyn_joint_fwd");
}

namespace {

// dyn_joint_bwd (de_stride_b = T * Hd, no accumulation) and dyn_joint_bwd_chunk: the same two launches
int joint_bwd(const char* who, const float* dz, const float* z, float* de, float* dp, int64_t B, int64_t T, int64_t U1, int64_t Hd,
              int32_t shared_p, int64_t de_stride_b, int64_t dp_stride_b, int64_t dp_stride_u, int32_t dp_accumulate, int32_t act, void* stream) {
    DYN_REQUIRE(act == 0, DYN_E_UNSUPPORTED, "%s: hidden_act %d is not built (0 = relu)", who, act);
    DYN_REQUIRE(dz && z && (de || dp) && B > 0 && T > 0 && U1 > 0 && Hd > 0 && Hd % 4 == 0, DYN_E_ARG, "%s: bad arguments", who);
    DYN_REQUIRE(!de || (de_stride_b >= T * Hd && de_stride_b % 4 == 0), DYN_E_ARG,
                "%s: de_stride_b must be a multiple of 4, at least the chunk's frames * Hd", who);
    DYN_REQUIRE(!dp || (dp_stride_b >= 0 && dp_stride_b % 4 == 0 && dp_stride_u >= Hd && dp_stride_u % 4 == 0), DYN_E_ARG,
                "%s: dp strides must be multiples of 4, dp_stride_u >= Hd", who);
    DYN_REQUIRE(dp_accumulate == 0 || dp_accumulate == 1, DYN_E_ARG, "%s: dp_accumulate must be 0 or 1", who);
    DYN_REQUIRE(!(((uintptr_t)dz | (uintptr_t)z | (uintptr_t)de | (uintptr_t)dp) & 15), DYN_E_ARG, "%s: pointers must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    if (de)
        hipLaunchKernelGGL(joint_bwd_e_kernel, dim3(grid_for(B * T * (Hd / 4), 256)), dim3(256), 0, st, dz, z, de, B, T, U1, Hd / 4,
                           de_stride_b / 4);
    if (dp)
        hipLaunchKernelGGL(joint_bwd_p_kernel, dim3(grid_for((shared_p ? 1 : B) * U1 * (Hd / 4), 256)), dim3(256), 0, st, dz, z, dp, B, T, U1,
                           Hd / 4, (int)(shared_p != 0), dp_stride_b, dp_stride_u, (int)dp_accumulate);
    return dyn::check_launch(who);
}

}  // namespace

extern "C" int dyn_joint_bwd(const float* dz, const float* z, float* de, float* dp, int64_t B, int64_t T, int64_t U1, int64_t Hd,
                             int32_t shared_p, int64_t dp_stride_b, int64_t dp_stride_u, int32_t act, void* stream) {
    return joint_bwd("dyn_joint_bwd", dz, z, de, dp, B, T, U1, Hd, shared_p, T * Hd, dp_stride_b, dp_stride_u, 0, act, stream);
}

extern "C" int dyn_joint_bwd_chunk(const float* dz, const float* z, float* de, float* dp, int64_t B, int64_t Tc, int64_t U1, int64_t Hd,
                                   int32_t shared_p, int64_t de_stride_b, int64_t dp_stride_b, int64_t dp_stride_u, int32_t dp_accumulate,
                                   int32_t act, void* stream) {
    return joint_bwd("dyn_joint_bwd_chunk", dz, z, de, dp, B, Tc, U1, Hd, shared_p, de_stride_b, dp_stride_b, dp_stride_u, dp_accumulate, act,
                     stream);
}

// ---- the loss entries: one host path, `tdt` false = no duration head (durations null, D = 0, sigma unused) ------------------------
namespace {

const char* const OVER_STATE = "chunking the lattice state is not built: only the joint streams over frame chunks";

// What every loss entry does before its launches: sizes, the duration list, the lattice state carved out of `state` (refused by name over
// the budget, `over` ends that message), the kernels' dimensions for the whole lattice (t0 = 0, Tc = T).
int setup(const char* who, const char* over, bool tdt, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
          int64_t S, int32_t blank, float sigma, void* state, int64_t state_bytes, int64_t budget_bytes, LatticeDims& d, LatticeWs& w) {
    DYN_REQUIRE(B > 0 && T > 0 && U1 > 0 && V1 > 0 && S >= 1 && blank >= 0 && blank < V1, DYN_E_ARG, "%s: bad arguments", who);
    DYN_REQUIRE(V1 < (1 << 30) && U1 < (1 << 24) && T + U1 < (1 << 24), DYN_E_UNSUPPORTED, "%s: %lld diagonals / %lld classes unsupported", who,
                (long long)(T + U1), (long long)V1);
    d.durs = Durs{};
    if (tdt)
        if (const int rc = check_durs(durations, D, d.durs, who)) return rc;
    w = carve(state, B, T, U1, d.durs.n);
    DYN_REQUIRE(budget_bytes <= 0 || w.total <= budget_bytes, DYN_E_WORKSPACE,
                "%s: the lattice of [%lld, %lld, %lld] needs %lld bytes, over the workspace budget of %lld (%s)", who, (long long)B, (long long)T,
                (long long)U1, (long long)w.total, (long long)budget_bytes, over);
    DYN_REQUIRE(state && state_bytes >= w.total, DYN_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)state_bytes,
                (long long)w.total);
    d.B = B; d.T = T; d.U1 = U1; d.t0 = 0; d.Tc = T; d.V1 = V1; d.N = V1 + d.durs.n; d.S = S; d.blank = blank; d.sigma = sigma;
    return DYN_OK;
}

// the frames [t0, t0 + Tc) of a chunk entry; the rows of one launch are counted in int64, the grid is capped (grid_for)
int chunk(const char* who, int64_t t0, int64_t Tc, LatticeDims& d) {
    DYN_REQUIRE(t0 >= 0 && t0 < d.T && Tc > 0 && Tc < (1 << 24), DYN_E_ARG, "%s: the chunk [%lld, %lld + %lld) must start inside the %lld frames",
                who, (long long)t0, (long long)t0, (long long)Tc, (long long)d.T);
    d.t0 = t0; d.Tc = Tc;
    return DYN_OK;
}

void launch_arcs(const float* logits, const int32_t* targets, const int32_t* tlen, const LatticeWs& w, const LatticeDims& d, hipStream_t st) {
    hipLaunchKernelGGL(d.durs.n ? arcs_kernel<true> : arcs_kernel<false>, dim3(grid_for(d.B * d.Tc * d.U1, WPB)), dim3(64 * WPB), 0, st, logits,
                       targets, tlen, w.lp, w.lse, d);
}

// alpha (and with `both` beta) over the anti-diagonals, the reduction, the per-row nll
int launch_lattice(const char* who, const int32_t* ilen, const int32_t* tlen, int reduction, float* loss, float* nll_per_row, bool both,
                   const LatticeWs& w, const LatticeDims& d, hipStream_t st) {
    const int64_t diag = d.T < d.U1 ? d.T : d.U1;
    int threads = (int)((diag + 63) / 64 * 64);
    if (threads > LATTICE_T) threads = LATTICE_T;
    hipLaunchKernelGGL(d.durs.n ? tdt_lattice_kernel : rnnt_lattice_kernel, dim3((unsigned)d.B, both ? 2u : 1u), dim3(threads), 0, st, w.lp, ilen,
                       tlen, w.alpha, w.beta, w.abase, w.bbase, w.ll, w.nll, d);
    hipLaunchKernelGGL(tdt_loss_reduce_kernel, dim3(1), dim3(64), 0, st, w.nll, tlen, loss, d.B, reduction);
    if (nll_per_row) {
        hipError_t e = hipMemcpyAsync(nll_per_row, w.nll, d.B * sizeof(float), hipMemcpyDeviceToDevice, st);
        DYN_REQUIRE(e == hipSuccess, DYN_E_LAUNCH, "%s: copy of the per-row nll failed", who);
    }
    return DYN_OK;
}

void launch_grad(const float* logits, const int32_t* targets, const int32_t* ilen, const int32_t* tlen, float* grad, float grad_scale,
                 int reduction, const LatticeWs& w, const LatticeDims& d, hipStream_t st) {
    hipLaunchKernelGGL(d.durs.n ? grad_kernel<true> : grad_kernel<false>, dim3(grid_for(d.B * d.Tc * d.U1, WPB)), dim3(64 * WPB), 0, st, logits,
                       targets, ilen, tlen, w.lp, w.lse, w.alpha, w.beta, w.abase, w.bbase, w.ll, grad, grad_scale, reduction, d);
}

int loss(const char* who, const char* over, bool tdt, const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1,
         const int32_t* durations, int64_t D, const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths,
         int32_t blank, float sigma, int32_t reduction, float grad_scale, float* loss_out, float* nll_per_row, float* grad, void* workspace,
         int64_t workspace_bytes, int64_t workspace_budget_bytes, void* stream) {
    DYN_REQUIRE(logits && targets && logit_lengths && target_lengths && loss_out && reduction >= 0 && reduction <= 4, DYN_E_ARG,
                "%s: bad arguments", who);
    LatticeDims d;
    LatticeWs w;
    if (const int rc = setup(who, over, tdt, B, T, U1, V1, durations, D, S, blank, sigma, workspace, workspace_bytes, workspace_budget_bytes, d, w))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_arcs(logits, targets, target_lengths, w, d, st);
    if (const int rc = launch_lattice(who, logit_lengths, target_lengths, (int)reduction, loss_out, nll_per_row, grad != nullptr, w, d, st)) return rc;
    if (grad) launch_grad(logits, targets, logit_lengths, target_lengths, grad, grad_scale, (int)reduction, w, d, st);
    return dyn::check_launch(who);
}

int arcs_chunk(const char* who, bool tdt, const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
               const int32_t* targets, int64_t S, const int32_t* target_lengths, int32_t blank, float sigma, int64_t t0, int64_t Tc, void* state,
               int64_t state_bytes, int64_t state_budget_bytes, void* stream) {
    DYN_REQUIRE(logits && targets && target_lengths, DYN_E_ARG, "%s: bad arguments", who);
    LatticeDims d;
    LatticeWs w;
    if (const int rc = setup(who, OVER_STATE, tdt, B, T, U1, V1, durations, D, S, blank, sigma, state, state_bytes, state_budget_bytes, d, w))
        return rc;
    if (const int rc = chunk(who, t0, Tc, d)) return rc;
    launch_arcs(logits, targets, target_lengths, w, d, (hipStream_t)stream);
    return dyn::check_launch(who);
}

int lattice_run(const char* who, bool tdt, int64_t B, int64_t T, int64_t U1, const int32_t* durations, int64_t D, int64_t S,
                const int32_t* logit_lengths, const int32_t* target_lengths, int32_t reduction, float* loss_out, float* nll_per_row,
                int32_t want_beta, void* state, int64_t state_bytes, int64_t state_budget_bytes, void* stream) {
    DYN_REQUIRE(logit_lengths && target_lengths && loss_out && reduction >= 0 && reduction <= 4, DYN_E_ARG, "%s: bad arguments", who);
    LatticeDims d;
    LatticeWs w;
    // the lattice reads neither the vocabulary nor the blank: one token class stands in for them
    if (const int rc = setup(who, OVER_STATE, tdt, B, T, U1, 1, durations, D, S, 0, 0.f, state, state_bytes, state_budget_bytes, d, w)) return rc;
    if (const int rc = launch_lattice(who, logit_lengths, target_lengths, (int)reduction, loss_out, nll_per_row, want_beta != 0, w, d,
                                      (hipStream_t)stream))
        return rc;
    return dyn::check_launch(who);
}

int grad_chunk(const char* who, bool tdt, const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
               const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank, int32_t reduction,
               float grad_scale, int64_t t0, int64_t Tc, float* grad, const void* state, int64_t state_bytes, void* stream) {
    DYN_REQUIRE(logits && targets && logit_lengths && target_lengths && grad && reduction >= 0 && reduction <= 4, DYN_E_ARG, "%s: bad arguments",
                who);
    LatticeDims d;
    LatticeWs w;
    if (const int rc = setup(who, OVER_STATE, tdt, B, T, U1, V1, durations, D, S, blank, 0.f, const_cast<void*>(state), state_bytes, 0, d, w))
        return rc;
    if (const int rc = chunk(who, t0, Tc, d)) return rc;
    launch_grad(logits, targets, logit_lengths, target_lengths, grad, grad_scale, (int)reduction, w, d, (hipStream_t)stream);
    return dyn::check_launch(who);
}

void layout(int64_t B, int64_t T, int64_t U1, int64_t D, int64_t* offsets8) {
    const LatticeWs w = carve(nullptr, B, T, U1, D);
    const float* ps[8] = {w.lp, w.lse, w.alpha, w.beta, w.abase, w.bbase, w.ll, w.nll};
    for (int i = 0; i < 8; ++i) offsets8[i] = (const char*)ps[i] - (const char*)nullptr;
}

}  // namespace

extern "C" int64_t dyn_tdt_loss_workspace_bytes(int64_t B, int64_t T, int64_t U1, int64_t D) {
    if (B <= 0 || T <= 0 || U1 <= 0 || D <= 0) return -1;
    return carve(nullptr, B, T, U1, D).total;
}

extern "C" int64_t dyn_rnnt_loss_workspace_bytes(int64_t B, int64_t T, int64_t U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return -1;
    return carve(nullptr, B, T, U1, 0).total;
}

extern "C" int dyn_tdt_loss_workspace_layout(int64_t B, int64_t T, int64_t U1, int64_t D, int64_t* offsets8) {
    DYN_REQUIRE(offsets8 && B > 0 && T > 0 && U1 > 0 && D > 0 && D <= MAX_DUR, DYN_E_ARG, "dyn_tdt_loss_workspace_layout: bad arguments");
    layout(B, T, U1, D, offsets8);
    return DYN_OK;
}

extern "C" int dyn_rnnt_loss_workspace_layout(int64_t B, int64_t T, int64_t U1, int64_t* offsets8) {
    DYN_REQUIRE(offsets8 && B > 0 && T > 0 && U1 > 0, DYN_E_ARG, "dyn_rnnt_loss_workspace_layout: bad arguments");
    layout(B, T, U1, 0, offsets8);
    return DYN_OK;
}

extern "C" int dyn_tdt_loss(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                            const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank,
                            float sigma, int32_t reduction, float grad_scale, float* loss, float* nll_per_row, float* grad,
                            void* workspace, int64_t workspace_bytes, int64_t workspace_budget_bytes, void* stream) {
    return ::loss("dyn_tdt_loss", "chunking over t is not built", true, logits, B, T, U1, V1, durations, D, targets, S, logit_lengths,
                  target_lengths, blank, sigma, reduction, grad_scale, loss, nll_per_row, grad, workspace, workspace_bytes, workspace_budget_bytes,
                  stream);
}

extern "C" int dyn_rnnt_loss(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                             const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank, int32_t reduction, float grad_scale,
                             float* loss, float* nll_per_row, float* grad, void* workspace, int64_t workspace_bytes,
                             int64_t workspace_budget_bytes, void* stream) {
    return ::loss("dyn_rnnt_loss", OVER_STATE, false, logits, B, T, U1, V1, nullptr, 0, targets, S, logit_lengths, target_lengths, blank, 0.f,
                  reduction, grad_scale, loss, nll_per_row, grad, workspace, workspace_bytes, workspace_budget_bytes, stream);
}

extern "C" int dyn_tdt_arcs_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                                  const int32_t* targets, int64_t S, const int32_t* target_lengths, int32_t blank, float sigma, int64_t t0,
                                  int64_t Tc, void* state, int64_t state_bytes, int64_t state_budget_bytes, void* stream) {
    return arcs_chunk("dyn_tdt_arcs_chunk", true, logits, B, T, U1, V1, durations, D, targets, S, target_lengths, blank, sigma, t0, Tc, state,
                      state_bytes, state_budget_bytes, stream);
}

extern "C" int dyn_rnnt_arcs_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                                   const int32_t* target_lengths, int32_t blank, int64_t t0, int64_t Tc, void* state, int64_t state_bytes,
                                   int64_t state_budget_bytes, void* stream) {
    return arcs_chunk("dyn_rnnt_arcs_chunk", false, logits, B, T, U1, V1, nullptr, 0, targets, S, target_lengths, blank, 0.f, t0, Tc, state,
                      state_bytes, state_budget_bytes, stream);
}

extern "C" int dyn_tdt_lattice_run(int64_t B, int64_t T, int64_t U1, const int32_t* durations, int64_t D, int64_t S,
                                   const int32_t* logit_lengths, const int32_t* target_lengths, int32_t reduction, float* loss,
                                   float* nll_per_row, int32_t want_beta, void* state, int64_t state_bytes, int64_t state_budget_bytes,
                                   void* stream) {
    return lattice_run("dyn_tdt_lattice_run", true, B, T, U1, durations, D, S, logit_lengths, target_lengths, reduction, loss, nll_per_row,
                       want_beta, state, state_bytes, state_budget_bytes, stream);
}

extern "C" int dyn_rnnt_lattice_run(int64_t B, int64_t T, int64_t U1, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths,
                                    int32_t reduction, float* loss, float* nll_per_row, int32_t want_beta, void* state, int64_t state_bytes,
                                    int64_t state_budget_bytes, void* stream) {
    return lattice_run("dyn_rnnt_lattice_run", false, B, T, U1, nullptr, 0, S, logit_lengths, target_lengths, reduction, loss, nll_per_row,
                       want_beta, state, state_bytes, state_budget_bytes, stream);
}

extern "C" int dyn_tdt_grad_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                                  const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths,
                                  int32_t blank, int32_t reduction, float grad_scale, int64_t t0, int64_t Tc, float* grad, const void* state,
                                  int64_t state_bytes, void* stream) {
    return grad_chunk("dyn_tdt_grad_chunk", true, logits, B, T, U1, V1, durations, D, targets, S, logit_lengths, target_lengths, blank, reduction,
                      grad_scale, t0, Tc, grad, state, state_bytes, stream);
}

extern "C" int dyn_rnnt_grad_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                                   const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank, int32_t reduction,
                                   float grad_scale, int64_t t0, int64_t Tc, float* grad, const void* state, int64_t state_bytes, void* stream) {
    return grad_chunk("dyn_rnnt_grad_chunk", false, logits, B, T, U1, V1, nullptr, 0, targets, S, logit_lengths, target_lengths, blank, reduction,
                      grad_scale, t0, Tc, grad, state, state_bytes, stream);
}

// ---- greedy decode: one launcher, the pick kernel chosen by the head ---------------------------------------------------------------
namespace {

// n_steps greedy steps of every live row.  `tdt`: argmax over the durations as well, greedy_pick_kernel; else max_symbols per frame,
// rnnt_greedy_pick_kernel, frames recorded from frame_base, and with `rebase` the state first moved on to this chunk of frames.
int greedy_launch(const char* who, bool tdt, const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs,
                  const float* proj_w, const float* proj_b, const float* head_w, const float* head_b, int32_t* istate, float* h, float* c,
                  float* h_new, float* dec, float* logits, int32_t* tokens, int32_t* frames, int64_t B, int64_t T, int64_t Hd, int64_t layers,
                  int64_t V1, const int32_t* durations, int64_t D, int32_t blank, int64_t max_symbols, int64_t n_max, int64_t max_steps,
                  int32_t n_steps, int64_t frame_base, bool rebase, void* stream) {
    DYN_REQUIRE(enc && valid && embed && lstm_ptrs && proj_w && proj_b && head_w && head_b && istate && h && c && h_new && dec && logits &&
                    tokens && frames, DYN_E_ARG, "%s: null pointer", who);
    DYN_REQUIRE(B > 0 && B <= 65535 && T > 0 && Hd > 0 && layers > 0 && layers <= 8 && V1 > 0 && V1 < (1 << 30) && blank >= 0 && blank < V1 &&
                    max_symbols > 0 && n_max > 0 && max_steps > 0 && n_steps >= 0 && T < (1 << 30) && n_max < (1 << 30), DYN_E_ARG,
                "%s: bad sizes", who);
    DYN_REQUIRE(frame_base >= 0 && frame_base + T < (1ll << 31), DYN_E_ARG, "%s: frame_base=%lld leaves the int32 frames", who,
                (long long)frame_base);
    GreedyArgs a;
    a.durs = Durs{};
    if (tdt)
        if (const int rc = check_durs(durations, D, a.durs, who)) return rc;
    a.enc = enc; a.valid = valid; a.embed = embed; a.lstm = (const float* const*)lstm_ptrs; a.proj_w = proj_w; a.proj_b = proj_b;
    a.head_w = head_w; a.head_b = head_b; a.istate = istate; a.h = h; a.c = c; a.h_new = h_new; a.dec = dec; a.logits = logits;
    a.tokens = tokens; a.frames = frames;
    a.B = (int32_t)B; a.T = (int32_t)T; a.Hd = (int32_t)Hd; a.L = (int32_t)layers; a.V1 = (int32_t)V1; a.N = (int32_t)V1 + a.durs.n;
    a.blank = blank; a.n_max = (int32_t)n_max; a.max_steps = (int32_t)(max_steps < (1 << 30) ? max_steps : (1 << 30));
    const int ms = (int)(max_symbols < (1 << 30) ? max_symbols : (1 << 30));
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(256), gh((unsigned)dyn::cdiv(Hd, 4), (unsigned)B), gn((unsigned)dyn::cdiv(a.N, 4), (unsigned)B);
    if (rebase) hipLaunchKernelGGL(rnnt_greedy_rebase_kernel, dim3((unsigned)dyn::cdiv(B, 256)), blk, 0, st, a);
    for (int s = 0; s < n_steps; ++s) {
        for (int l = 0; l < layers; ++l) hipLaunchKernelGGL(greedy_lstm_kernel, gh, blk, 0, st, a, l);
        hipLaunchKernelGGL(greedy_proj_kernel, gh, blk, 0, st, a);
        hipLaunchKernelGGL(greedy_joint_kernel, gn, blk, 0, st, a);
        if (tdt) hipLaunchKernelGGL(greedy_pick_kernel, dim3((unsigned)B), blk, 0, st, a);
        else hipLaunchKernelGGL(rnnt_greedy_pick_kernel, dim3((unsigned)B), blk, 0, st, a, ms, (int)frame_base);
    }
    return dyn::check_launch(who);
}

}  // namespace

extern "C" int dyn_tdt_greedy_steps(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs,
                                    const float* proj_w, const float* proj_b, const float* head_w, const float* head_b, int32_t* istate,
                                    float* h, float* c, float* h_new, float* dec, float* logits, int32_t* tokens, int32_t* frames,
                                    int64_t B, int64_t T, int64_t Hd, int64_t layers, int64_t V1, const int32_t* durations, int64_t D,
                                    int32_t blank, int64_t n_max, int64_t max_steps, int32_t n_steps, void* stream) {
    return greedy_launch("dyn_tdt_greedy_steps", true, enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, istate, h, c, h_new, dec,
                         logits, tokens, frames, B, T, Hd, layers, V1, durations, D, blank, 1, n_max, max_steps, n_steps, 0, false, stream);
}

extern "C" int dyn_rnnt_greedy_steps(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs,
                                     const float* proj_w, const float* proj_b, const float* head_w, const float* head_b, int32_t* istate,
                                     float* h, float* c, float* h_new, float* dec, float* logits, int32_t* tokens, int32_t* frames, int64_t B,
                                     int64_t T, int64_t Hd, int64_t layers, int64_t V1, int32_t blank, int64_t max_symbols, int64_t n_max,
                                     int64_t max_steps, int32_t n_steps, void* stream) {
    return greedy_launch("dyn_rnnt_greedy_steps", false, enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, istate, h, c, h_new, dec,
                         logits, tokens, frames, B, T, Hd, layers, V1, nullptr, 0, blank, max_symbols, n_max, max_steps, n_steps, 0, false, stream);
}

extern "C" int dyn_rnnt_greedy_steps_chunk(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs,
                                           const float* proj_w, const float* proj_b, const float* head_w, const float* head_b,
                                           int32_t* istate, float* h, float* c, float* h_new, float* dec, float* logits, int32_t* tokens,
                                           int32_t* frames, int64_t B, int64_t T, int64_t Hd, int64_t layers, int64_t V1, int32_t blank,
                                           int64_t max_symbols, int64_t n_max, int64_t max_steps, int32_t n_steps, int64_t frame_base,
                                           int32_t rebase, void* stream) {
    DYN_REQUIRE(rebase == 0 || rebase == 1, DYN_E_ARG, "dyn_rnnt_greedy_steps_chunk: rebase=%d (0 or 1)", (int)rebase);
    return greedy_launch("dyn_rnnt_greedy_steps_chunk", false, enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, istate, h, c, h_new,
                         dec, logits, tokens, frames, B, T, Hd, layers, V1, nullptr, 0, blank, max_symbols, n_max, max_steps, n_steps, frame_base,
                         rebase != 0, stream);
}

