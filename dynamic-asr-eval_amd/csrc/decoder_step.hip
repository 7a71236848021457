// One-token decoder steps of the autoregressive decode (`model.generate`, reference call sites lcasr/lib.py:1128,1579-1582,1620-1625):
// every product of a step is a [1, K] row times a [N, K] weight, 0.13 - 2 MFLOP, and the whole decoder (2 x 256 by default) is
// ~11 MB of weights that stay in L2 — the step is bound by launches, not by bytes or flops.  So a step is 8 * layers + 2 launches of
// two lean kernels, queued back to back from ONE C call for several tokens:
//   dec_gemv_kernel   y = act(W . f(x) + b) (+ residual): a wave per output row (coalesced 16-byte weight reads, one wave reduction per
//                     row), x held in registers; f = LayerNorm (statistics recomputed per wave from the 1 - 8 KB row: cheaper than a
//                     launch) and, for the first layer, the token-embedding + position gather itself
//   dec_attn_kernel   (dec_attn.h, shared with seq2seq_step.hip)
//                     one query against n cached keys / values, four workgroups per head (a quarter of the keys each): scores into LDS
//                     (16 lanes per key row, four rows in flight), exponentials, weighted sum of the value rows; the four (sum, max,
//                     denominator) triples are merged in the prologue of the projection that consumes them
//   dec_pick_kernel   next token = argmax (or the Gumbel-max draw) over the logits, written straight into the token buffer
// No tile kernel, no split-K reduce, no intermediate [1, n] score matrices in HBM.
// dyn_decoder_steps_batch runs the same step for up to 8 rows (the sampled rollouts of the RL modes) over shared encoder states with
// the same launch count: dec_gemv_rows_kernel applies every weight row it reads to four residual rows held in registers (each row's
// sum in dec_gemv_kernel's order, so a row's logits do not depend on its neighbours), the attention and pick kernels take the row
// from the grid.  A per-row device flag retires a row at eos: no work, no cache write, eos in its later token slots.
#include "common.h"

// No implicit multiply-add fusion in this file: where the compiler fuses depends on the surrounding code, and a row of
// dec_gemv_rows_kernel must round exactly as the same row in dec_gemv_kernel does (dyn_decoder_steps_batch's contract).
#pragma clang fp contract(off)
#include "layernorm_row.h"   // after the pragma: its row statistics are compiled without fusion here as well
#include "dec_attn.h"        // dot4, NSPLIT, dec_attn_kernel, better: shared with seq2seq_step.hip

namespace {

struct GemvArgs {
    const float* x;        // [K] input row (unused with EMBED)
    const int32_t* tok;    // EMBED: the token id of this position
    const float* table;    // EMBED: [vocab, K]
    const float* pos;      // EMBED: positional row [K]
    float* x_out;          // EMBED: the gathered row is written here once (the residual stream)
    int vocab;
    const float* parts;    // MERGE: the key splits of the attention, [heads][NSPLIT][hd + 4] (unnormalised sum | max | denominator)
    int hd;
    const float* gamma;    // LN
    const float* beta;
    float eps;
    const float* W;        // [N, K]
    const float* bias;     // [N] or null
    const float* res;      // [N] or null; may alias y (element n is read and written by the same lane)
    float* y;              // [N]
    int N, rpw;            // rows per wave
};

template <int NV, bool LN, bool SILU, bool EMBED, bool MERGE = false>
__global__ __launch_bounds__(256) void dec_gemv_kernel(const GemvArgs a) {
    constexpr int K = NV * 256;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 xv[NV];
    if (EMBED) {
        int64_t id = a.tok[0];
        id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);       // ids are validated on the host; never read outside the table
        const float4* row = reinterpret_cast<const float4*>(a.table + id * K);
        const float4* pr = reinterpret_cast<const float4*>(a.pos);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 e = row[lane + 64 * j], p = pr[lane + 64 * j];
            xv[j] = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
        }
        if (blockIdx.x == 0 && w == 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(a.x_out)[lane + 64 * j] = xv[j];
        }
    } else if (MERGE) {     // x = softmax-weighted value sum of one head, put together from its NSPLIT key splits
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * (lane + 64 * j), h = c / a.hd, cc = c % a.hd;
            const float* ph = a.parts + (int64_t)h * NSPLIT * (a.hd + 4);      // 16-byte aligned slots: hd | max | denominator | pad
            float m = -INFINITY;
#pragma unroll
            for (int u = 0; u < NSPLIT; ++u) m = fmaxf(m, ph[u * (a.hd + 4) + a.hd]);
            float den = 0.f;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < NSPLIT; ++u) {
                const float* pu = ph + u * (a.hd + 4);
                const float wgt = __expf(pu[a.hd] - m);             // an empty split has max = -inf: weight 0
                const float4 ov = *reinterpret_cast<const float4*>(pu + cc);
                den += wgt * pu[a.hd + 1];
                o.x += wgt * ov.x; o.y += wgt * ov.y; o.z += wgt * ov.z; o.w += wgt * ov.w;
            }
            const float r = 1.f / den;
            xv[j] = make_float4(o.x * r, o.y * r, o.z * r, o.w * r);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) xv[j] = reinterpret_cast<const float4*>(a.x)[lane + 64 * j];
    }
    if (LN) {
        float mean, rstd;
        dyn::row_mean_rstd(xv, a.eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 g = reinterpret_cast<const float4*>(a.gamma)[lane + 64 * j], b = reinterpret_cast<const float4*>(a.beta)[lane + 64 * j];
            xv[j].x = (xv[j].x - mean) * rstd * g.x + b.x;
            xv[j].y = (xv[j].y - mean) * rstd * g.y + b.y;
            xv[j].z = (xv[j].z - mean) * rstd * g.z + b.z;
            xv[j].w = (xv[j].w - mean) * rstd * g.w + b.w;
        }
    }
    const int n_base = (blockIdx.x * 4 + w) * a.rpw;
    for (int r = 0; r < a.rpw; r += 2) {          // two rows in flight per wave
        const int n0 = n_base + r;
        if (n0 >= a.N) break;
        const bool two = r + 1 < a.rpw && n0 + 1 < a.N;
        const float4* w0 = reinterpret_cast<const float4*>(a.W + (int64_t)n0 * K);
        const float4* w1 = two ? w0 + K / 4 : w0;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            s0 += dot4(w0[lane + 64 * j], xv[j]);
            s1 += dot4(w1[lane + 64 * j], xv[j]);
        }
        s0 = dyn::wave_sum(s0);
        s1 = dyn::wave_sum(s1);
        if (lane == 0) {
            float v = s0 + (a.bias ? a.bias[n0] : 0.f);
            if (SILU) v = v * dyn::sigmoidf_(v);
            a.y[n0] = v + (a.res ? a.res[n0] : 0.f);
            if (two) {
                v = s1 + (a.bias ? a.bias[n0 + 1] : 0.f);
                if (SILU) v = v * dyn::sigmoidf_(v);
                a.y[n0 + 1] = v + (a.res ? a.res[n0 + 1] : 0.f);
            }
        }
    }
}

constexpr int RB = 4;   // residual rows per workgroup of dec_gemv_rows_kernel

struct GemvRowsArgs {
    GemvArgs g;                  // row 0
    int rows;
    const int32_t* finished;     // [rows]: a finished row is neither read nor written
    int64_t s_scr;               // floats between rows of x / x_out / parts / res (all in the per-row scratch block)
    int64_t s_y;                 // floats between rows of y
    int64_t s_tok;               // EMBED: entries between rows of tok
};

// dec_gemv_kernel for RB rows at once: blockIdx.y picks the group of rows, the weight rows are read once per group.  Per row the
// prologue and the accumulation `s += dot4(w[lane + 64 j], x[j])`, j ascending, then one wave reduction, are those of dec_gemv_kernel.
template <int NV, bool LN, bool SILU, bool EMBED, bool MERGE = false>
__global__ __launch_bounds__(256) void dec_gemv_rows_kernel(const GemvRowsArgs b) {
    constexpr int K = NV * 256;
    const GemvArgs& a = b.g;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = blockIdx.y * RB;
    bool live[RB];
    bool any = false;
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
        live[rr] = r0 + rr < b.rows && b.finished[r0 + rr] == 0;
        any = any || live[rr];
    }
    if (!any) return;
    float4 xv[RB][NV];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
        const int64_t row = r0 + rr;
        if (!live[rr]) {
#pragma unroll
            for (int j = 0; j < NV; ++j) xv[rr][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        if (EMBED) {
            int64_t id = a.tok[row * b.s_tok];
            id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);
            const float4* trow = reinterpret_cast<const float4*>(a.table + id * K);
            const float4* pr = reinterpret_cast<const float4*>(a.pos);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float4 e = trow[lane + 64 * j], p = pr[lane + 64 * j];
                xv[rr][j] = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
            }
            if (blockIdx.x == 0 && w == 0) {
#pragma unroll
                for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(a.x_out + row * b.s_scr)[lane + 64 * j] = xv[rr][j];
            }
        } else if (MERGE) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = 4 * (lane + 64 * j), h = c / a.hd, cc = c % a.hd;
                const float* ph = a.parts + row * b.s_scr + (int64_t)h * NSPLIT * (a.hd + 4);
                float m = -INFINITY;
#pragma unroll
                for (int u = 0; u < NSPLIT; ++u) m = fmaxf(m, ph[u * (a.hd + 4) + a.hd]);
                float den = 0.f;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < NSPLIT; ++u) {
                    const float* pu = ph + u * (a.hd + 4);
                    const float wgt = __expf(pu[a.hd] - m);
                    const float4 ov = *reinterpret_cast<const float4*>(pu + cc);
                    den += wgt * pu[a.hd + 1];
                    o.x += wgt * ov.x; o.y += wgt * ov.y; o.z += wgt * ov.z; o.w += wgt * ov.w;
                }
                const float r = 1.f / den;
                xv[rr][j] = make_float4(o.x * r, o.y * r, o.z * r, o.w * r);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) xv[rr][j] = reinterpret_cast<const float4*>(a.x + row * b.s_scr)[lane + 64 * j];
        }
        if (LN) {
            float mean, rstd;
            dyn::row_mean_rstd(xv[rr], a.eps, mean, rstd);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float4 g = reinterpret_cast<const float4*>(a.gamma)[lane + 64 * j], bt = reinterpret_cast<const float4*>(a.beta)[lane + 64 * j];
                xv[rr][j].x = (xv[rr][j].x - mean) * rstd * g.x + bt.x;
                xv[rr][j].y = (xv[rr][j].y - mean) * rstd * g.y + bt.y;
                xv[rr][j].z = (xv[rr][j].z - mean) * rstd * g.z + bt.z;
                xv[rr][j].w = (xv[rr][j].w - mean) * rstd * g.w + bt.w;
            }
        }
    }
    const int n_base = (blockIdx.x * 4 + w) * a.rpw;
    for (int r = 0; r < a.rpw; r += 2) {          // two weight rows in flight per wave, each applied to the RB residual rows
        const int n0 = n_base + r;
        if (n0 >= a.N) break;
        const bool two = r + 1 < a.rpw && n0 + 1 < a.N;
        const float4* w0 = reinterpret_cast<const float4*>(a.W + (int64_t)n0 * K);
        const float4* w1 = two ? w0 + K / 4 : w0;
        float s0[RB], s1[RB];
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) s0[rr] = s1[rr] = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 wa = w0[lane + 64 * j], wb = w1[lane + 64 * j];
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                s0[rr] += dot4(wa, xv[rr][j]);
                s1[rr] += dot4(wb, xv[rr][j]);
            }
        }
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) {
            if (!live[rr]) continue;
            const float t0 = dyn::wave_sum(s0[rr]), t1 = dyn::wave_sum(s1[rr]);
            if (lane == 0) {
                const int64_t row = r0 + rr;
                float* y = a.y + row * b.s_y;
                const float* res = a.res ? a.res + row * b.s_scr : nullptr;
                float v = t0 + (a.bias ? a.bias[n0] : 0.f);
                if (SILU) v = v * dyn::sigmoidf_(v);
                y[n0] = v + (res ? res[n0] : 0.f);
                if (two) {
                    v = t1 + (a.bias ? a.bias[n0 + 1] : 0.f);
                    if (SILU) v = v * dyn::sigmoidf_(v);
                    y[n0 + 1] = v + (res ? res[n0 + 1] : 0.f);
                }
            }
        }
    }
}

// tokens_out[0] = argmax_c key(x[c]), first maximum wins; key = x (greedy) or the Gumbel-max key of dyn_gumbel_argmax_rows.
// One workgroup per row (blockIdx.x; seed + row): with `finished`, a finished row's slot receives eos and a live row that picks eos
// is marked finished.
template <bool SAMPLE>
__global__ __launch_bounds__(1024) void dec_pick_kernel(const float* __restrict__ x, int C, float inv_t, uint64_t seed, uint64_t stream,
                                                        int32_t* __restrict__ token_out, int64_t s_tok, int32_t* __restrict__ finished, int eos) {
    __shared__ float rv[16];
    __shared__ int ri[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    x += row * C;
    token_out += row * s_tok;
    seed += (uint64_t)row;
    if (finished && finished[row] != 0) {        // uniform over the workgroup; the flag is only written after the barrier below
        if (threadIdx.x == 0) token_out[0] = eos;
        return;
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = threadIdx.x; c < C; c += 1024) {
        const float v = SAMPLE ? dyn::gumbel_key(x[c], inv_t, seed, stream, (uint64_t)c) : x[c];
        if (better(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[w] = bv; ri[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i)
            if (better(rv[i], ri[i], bv, bi)) { bv = rv[i]; bi = ri[i]; }
        bi = bi == 0x7fffffff ? 0 : bi;
        token_out[0] = bi;
        if (finished && bi == eos) finished[row] = 1;
    }
}

template <bool LN, bool SILU, bool EMBED, bool MERGE = false>
int launch_gemv(const GemvArgs& a, int K, hipStream_t st) {
    const dim3 grid((unsigned)dyn::cdiv(a.N, 4 * a.rpw)), blk(256);
    const bool built = dyn::dispatch_nv<1, 2, 3, 4, 5, 6, 7, 8>(K, [&](auto nv) {
        hipLaunchKernelGGL((dec_gemv_kernel<decltype(nv)::value, LN, SILU, EMBED, MERGE>), grid, blk, 0, st, a);
    });
    return built ? DYN_OK : DYN_E_UNSUPPORTED;
}

template <bool LN, bool SILU, bool EMBED, bool MERGE = false>
int launch_gemv_rows(const GemvRowsArgs& b, int K, hipStream_t st) {
    const dim3 grid((unsigned)dyn::cdiv(b.g.N, 4 * b.g.rpw), (unsigned)dyn::cdiv(b.rows, RB)), blk(256);
    const bool built = dyn::dispatch_nv<1, 2, 3, 4, 5, 6, 7, 8>(K, [&](auto nv) {
        hipLaunchKernelGGL((dec_gemv_rows_kernel<decltype(nv)::value, LN, SILU, EMBED, MERGE>), grid, blk, 0, st, b);
    });
    return built ? DYN_OK : DYN_E_UNSUPPORTED;
}

inline int rows_per_wave(int N) { return N >= 4096 ? 4 : (N >= 512 ? 2 : 1); }

GemvArgs gemv(const float* x, const float* W, const float* bias, const float* res, float* y, int N) {
    GemvArgs a{};
    a.x = x; a.W = W; a.bias = bias; a.res = res; a.y = y; a.N = N; a.rpw = rows_per_wave(N);
    return a;
}

inline int64_t row_scratch(int64_t dd, int64_t ff, int64_t H) { return 2 * dd + ff + H * NSPLIT * (dd / H + 4); }

// the checks dyn_decoder_steps and dyn_decoder_steps_batch share
int check_desc(const dyn_decoder_desc* d, int32_t t0, int32_t n_steps, int32_t sample, float inv_temperature, int64_t rows, const char* who) {
    DYN_REQUIRE(d->embed && d->pos_table && d->norm_out_w && d->norm_out_b && d->head_w && d->head_b && d->layer_ptrs && d->tokens &&
                    d->logits && d->scratch, DYN_E_ARG, "%s: null pointer in the descriptor", who);
    const int dd = d->d_model, ff = d->d_ff, V = d->vocab, L = d->layers, H = d->heads;
    DYN_REQUIRE(dd > 0 && ff > 0 && V > 0 && L > 0 && H > 0 && d->n_enc > 0 && t0 >= 0 && n_steps >= 0, DYN_E_ARG, "%s: bad sizes", who);
    DYN_REQUIRE(dd % 256 == 0 && dd <= 2048 && ff % 256 == 0 && ff <= 2048, DYN_E_UNSUPPORTED,
                "%s: d_model %d / d_ff %d unsupported (multiples of 256 up to 2048)", who, dd, ff);
    DYN_REQUIRE(dd % H == 0, DYN_E_ARG, "%s: d_model %d not divisible by %d heads", who, dd, H);
    const int hd = dd / H;
    DYN_REQUIRE(hd >= 4 && hd <= 256 && (hd & (hd - 1)) == 0, DYN_E_UNSUPPORTED, "%s: head dim %d unsupported (power of two in 4 .. 256)", who, hd);
    DYN_REQUIRE((int64_t)t0 + n_steps <= d->max_positions, DYN_E_ARG, "%s: positions %d .. %d exceed max_positions %d", who, t0,
                t0 + n_steps - 1, d->max_positions);
    DYN_REQUIRE(d->n_enc <= MAX_KEYS && t0 + n_steps <= MAX_KEYS, DYN_E_UNSUPPORTED, "%s: more than %d keys per attention", who, MAX_KEYS);
    const int64_t need = rows * row_scratch(dd, ff, H);
    DYN_REQUIRE(d->scratch_floats >= need, DYN_E_WORKSPACE, "%s: scratch %lld < %lld floats", who, (long long)d->scratch_floats, (long long)need);
    DYN_REQUIRE(!sample || inv_temperature > 0.f, DYN_E_ARG, "%s: sampling needs a positive inverse temperature", who);
    for (int i = 0; i < L * DYN_DEC_PTRS_PER_LAYER; ++i)
        DYN_REQUIRE(d->layer_ptrs[i] != nullptr, DYN_E_ARG, "%s: layer pointer %d is null", who, i);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_decoder_steps(const dyn_decoder_desc* d, int32_t t0, int32_t n_steps, int32_t sample, float inv_temperature,
                                 uint64_t seed, uint64_t step0, void* stream) {
    DYN_REQUIRE(d, DYN_E_ARG, "dyn_decoder_steps: null descriptor");
    if (const int rc = check_desc(d, t0, n_steps, sample, inv_temperature, 1, "dyn_decoder_steps")) return rc;
    const int dd = d->d_model, ff = d->d_ff, V = d->vocab, L = d->layers, H = d->heads, hd = dd / H;
    hipStream_t st = (hipStream_t)stream;
    float* x = d->scratch;            // residual stream [dd]
    float* q2 = x + dd;               // cross-attention query [dd]
    float* act = q2 + dd;             // SiLU(w1 .) [ff]
    float* parts = act + ff;          // key splits of the attention [H][NSPLIT][hd + 4]
    auto merged = [&](const float* W, const float* bias) {      // x += W . attention + bias, the splits merged in the prologue
        GemvArgs m = gemv(nullptr, W, bias, x, x, dd);
        m.parts = parts; m.hd = hd;
        return m;
    };
    const float scale = 1.0f / sqrtf((float)hd);
    int rc = DYN_OK;
    for (int t = t0; t < t0 + n_steps && rc == DYN_OK; ++t) {
        for (int l = 0; l < L && rc == DYN_OK; ++l) {
            const void* const* P = d->layer_ptrs + (size_t)l * DYN_DEC_PTRS_PER_LAYER;
            auto F = [&](int i) { return (const float*)P[i]; };
            float* cache = (float*)P[16];
            const float* ckv = F(17);
            float* row = cache + (int64_t)t * 3 * dd;
            // self-attention: q | k | v of this position into cache row t, then the query against rows 0 .. t
            GemvArgs a = gemv(x, F(2), F(3), nullptr, row, 3 * dd);
            a.gamma = F(0); a.beta = F(1); a.eps = d->eps;
            if (l == 0) {
                a.tok = d->tokens + t; a.table = d->embed; a.pos = d->pos_table + (int64_t)t * dd; a.x_out = x; a.vocab = V;
                rc = launch_gemv<true, false, true>(a, dd, st);
            } else {
                rc = launch_gemv<true, false, false>(a, dd, st);
            }
            if (rc != DYN_OK) break;
            AttnArgs s{row, cache + dd, cache + 2 * dd, parts, t + 1, 3 * dd, hd, scale, 0, 0, 0, nullptr};
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT), dim3(256), (size_t)(dyn::cdiv(t + 1, NSPLIT) + 256) * sizeof(float), st, s);
            rc = launch_gemv<false, false, false, true>(merged(F(4), F(5)), dd, st);
            if (rc != DYN_OK) break;
            // cross-attention over the projected encoder rows
            a = gemv(x, F(8), F(9), nullptr, q2, dd);
            a.gamma = F(6); a.beta = F(7); a.eps = d->eps;
            rc = launch_gemv<true, false, false>(a, dd, st);
            if (rc != DYN_OK) break;
            AttnArgs c{q2, ckv, ckv + dd, parts, d->n_enc, 2 * dd, hd, scale, 0, 0, 0, nullptr};
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT), dim3(256), (size_t)(dyn::cdiv(d->n_enc, NSPLIT) + 256) * sizeof(float), st, c);
            rc = launch_gemv<false, false, false, true>(merged(F(10), F(11)), dd, st);
            if (rc != DYN_OK) break;
            // feed-forward
            a = gemv(x, F(14), nullptr, nullptr, act, ff);
            a.gamma = F(12); a.beta = F(13); a.eps = d->eps;
            rc = launch_gemv<true, true, false>(a, dd, st);
            if (rc != DYN_OK) break;
            rc = launch_gemv<false, false, false>(gemv(act, F(15), nullptr, x, x, dd), ff, st);
        }
        if (rc != DYN_OK) break;
        GemvArgs a = gemv(x, d->head_w, d->head_b, nullptr, d->logits, V);
        a.gamma = d->norm_out_w; a.beta = d->norm_out_b; a.eps = d->eps;
        rc = launch_gemv<true, false, false>(a, dd, st);
        if (rc != DYN_OK) break;
        if (sample)
            hipLaunchKernelGGL((dec_pick_kernel<true>), dim3(1), dim3(1024), 0, st, d->logits, V, inv_temperature, seed, step0 + (uint64_t)t, d->tokens + t + 1,
                               (int64_t)0, (int32_t*)nullptr, 0);
        else
            hipLaunchKernelGGL((dec_pick_kernel<false>), dim3(1), dim3(1024), 0, st, d->logits, V, 1.f, 0ull, 0ull, d->tokens + t + 1,
                               (int64_t)0, (int32_t*)nullptr, 0);
    }
    DYN_REQUIRE(rc == DYN_OK, rc, "dyn_decoder_steps: unsupported row length");
    return dyn::check_launch("dyn_decoder_steps");
}

extern "C" int64_t dyn_decoder_row_scratch_floats(int64_t d_model, int64_t d_ff, int64_t heads) {
    if (d_model <= 0 || d_ff <= 0 || heads <= 0 || d_model % heads) return -1;
    return row_scratch(d_model, d_ff, heads);
}

extern "C" int dyn_decoder_steps_batch(const dyn_decoder_batch_desc* b, int32_t t0, int32_t n_steps, int32_t sample, float inv_temperature,
                                       uint64_t seed, uint64_t step0, void* stream) {
    DYN_REQUIRE(b && b->finished, DYN_E_ARG, "dyn_decoder_steps_batch: null descriptor / finished flags");
    const dyn_decoder_desc* d = &b->base;
    const int R = b->rows;
    DYN_REQUIRE(R >= 1 && R <= 8, DYN_E_ARG, "dyn_decoder_steps_batch: %d rows (1 .. 8)", R);
    if (const int rc = check_desc(d, t0, n_steps, sample, inv_temperature, R, "dyn_decoder_steps_batch")) return rc;
    const int dd = d->d_model, ff = d->d_ff, V = d->vocab, L = d->layers, H = d->heads, hd = dd / H;
    DYN_REQUIRE(b->eos_id >= 0 && b->eos_id < V, DYN_E_ARG, "dyn_decoder_steps_batch: eos id %d outside the vocabulary", b->eos_id);
    DYN_REQUIRE(b->token_stride > (int64_t)t0 + n_steps, DYN_E_ARG, "dyn_decoder_steps_batch: token_stride %lld <= last slot %d",
                (long long)b->token_stride, t0 + n_steps);
    DYN_REQUIRE(b->cache_stride >= ((int64_t)t0 + n_steps) * 3 * dd && b->cache_stride % 4 == 0, DYN_E_ARG,
                "dyn_decoder_steps_batch: cache_stride %lld (>= %lld, multiple of 4)", (long long)b->cache_stride, ((long long)t0 + n_steps) * 3 * dd);
    const int64_t S = d->scratch_floats / R;      // per-row scratch block: x [dd] | q2 [dd] | act [ff] | parts
    DYN_REQUIRE(S % 4 == 0, DYN_E_ARG, "dyn_decoder_steps_batch: per-row scratch of %lld floats is not a multiple of 4", (long long)S);
    hipStream_t st = (hipStream_t)stream;
    float* x = d->scratch;
    float* q2 = x + dd;
    float* act = q2 + dd;
    float* parts = act + ff;
    auto rows = [&](GemvArgs g, int64_t s_y) {
        GemvRowsArgs a{};
        a.g = g; a.rows = R; a.finished = b->finished; a.s_scr = S; a.s_y = s_y; a.s_tok = b->token_stride;
        return a;
    };
    auto merged = [&](const float* W, const float* bias) {
        GemvArgs m = gemv(nullptr, W, bias, x, x, dd);
        m.parts = parts; m.hd = hd;
        return rows(m, S);
    };
    const float scale = 1.0f / sqrtf((float)hd);
    int rc = DYN_OK;
    for (int t = t0; t < t0 + n_steps && rc == DYN_OK; ++t) {
        for (int l = 0; l < L && rc == DYN_OK; ++l) {
            const void* const* P = d->layer_ptrs + (size_t)l * DYN_DEC_PTRS_PER_LAYER;
            auto F = [&](int i) { return (const float*)P[i]; };
            float* cache = (float*)P[16];
            const float* ckv = F(17);
            float* row = cache + (int64_t)t * 3 * dd;
            GemvArgs a = gemv(x, F(2), F(3), nullptr, row, 3 * dd);
            a.gamma = F(0); a.beta = F(1); a.eps = d->eps;
            if (l == 0) {
                a.tok = d->tokens + t; a.table = d->embed; a.pos = d->pos_table + (int64_t)t * dd; a.x_out = x; a.vocab = V;
                rc = launch_gemv_rows<true, false, true>(rows(a, b->cache_stride), dd, st);
            } else {
                rc = launch_gemv_rows<true, false, false>(rows(a, b->cache_stride), dd, st);
            }
            if (rc != DYN_OK) break;
            AttnArgs s{row, cache + dd, cache + 2 * dd, parts, t + 1, 3 * dd, hd, scale, b->cache_stride, b->cache_stride, S, b->finished};
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT, R), dim3(256), (size_t)(dyn::cdiv(t + 1, NSPLIT) + 256) * sizeof(float), st, s);
            rc = launch_gemv_rows<false, false, false, true>(merged(F(4), F(5)), dd, st);
            if (rc != DYN_OK) break;
            a = gemv(x, F(8), F(9), nullptr, q2, dd);
            a.gamma = F(6); a.beta = F(7); a.eps = d->eps;
            rc = launch_gemv_rows<true, false, false>(rows(a, S), dd, st);
            if (rc != DYN_OK) break;
            AttnArgs c{q2, ckv, ckv + dd, parts, d->n_enc, 2 * dd, hd, scale, S, 0, S, b->finished};     // keys / values shared by the rows
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT, R), dim3(256), (size_t)(dyn::cdiv(d->n_enc, NSPLIT) + 256) * sizeof(float), st, c);
            rc = launch_gemv_rows<false, false, false, true>(merged(F(10), F(11)), dd, st);
            if (rc != DYN_OK) break;
            a = gemv(x, F(14), nullptr, nullptr, act, ff);
            a.gamma = F(12); a.beta = F(13); a.eps = d->eps;
            rc = launch_gemv_rows<true, true, false>(rows(a, S), dd, st);
            if (rc != DYN_OK) break;
            rc = launch_gemv_rows<false, false, false>(rows(gemv(act, F(15), nullptr, x, x, dd), S), ff, st);
        }
        if (rc != DYN_OK) break;
        GemvArgs a = gemv(x, d->head_w, d->head_b, nullptr, d->logits, V);
        a.gamma = d->norm_out_w; a.beta = d->norm_out_b; a.eps = d->eps;
        rc = launch_gemv_rows<true, false, false>(rows(a, V), dd, st);
        if (rc != DYN_OK) break;
        if (sample)
            hipLaunchKernelGGL((dec_pick_kernel<true>), dim3(R), dim3(1024), 0, st, d->logits, V, inv_temperature, seed, step0 + (uint64_t)t,
                               d->tokens + t + 1, b->token_stride, b->finished, b->eos_id);
        else
            hipLaunchKernelGGL((dec_pick_kernel<false>), dim3(R), dim3(1024), 0, st, d->logits, V, 1.f, 0ull, 0ull, d->tokens + t + 1,
                               b->token_stride, b->finished, b->eos_id);
    }
    DYN_REQUIRE(rc == DYN_OK, rc, "dyn_decoder_steps_batch: unsupported row length");
    return dyn::check_launch("dyn_decoder_steps_batch");
}
