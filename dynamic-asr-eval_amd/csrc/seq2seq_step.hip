// One-token steps of a checkpoint-sized attention decoder for up to 8 rows (CohereAsrForConditionalGeneration.generate: transformers
// modeling_cohere_asr.py CohereAsrDecoder / CohereAsrDecoderLayer with a cache, GenerationMixin's greedy loop).  decoder_step.hip's
// kernels are written for a 2 x 256 decoder whose weights stay in L2; at 8 x 1024 with d_ff 4096 and a 16384-row head one token reads
// ~538 MB of fp32 weights, the same bytes for every row of the batch: the step is bound by weight streaming.  So:
//   s2s_gemv_kernel   y[r, n] = act(W[n, :] . f(x[r, :]) + b[n]) (+ res[r, n]) for ALL rows r at once.  A workgroup owns a few output rows n
//                     and all of K; its four waves split K by 256-float strips (wave w takes strips w, w + 4, ...), each lane keeps its
//                     float4 of every strip of every row r in registers, so a weight element is read from memory once per step and
//                     applied to all rows.  Four output rows are in flight per wave (4 x strips independent 16-byte loads per lane).
//                     The four waves' partial sums meet in LDS and are added in wave order: no atomics, fixed order.  A projection
//                     with N = d_model = 1024 output rows runs N / 4 = 256 workgroups.
//                     f = plain load | LayerNorm | (layer 0) token-embedding + position gather, embedding LayerNorm, written once as the
//                     residual stream, then the layer's input LayerNorm in the same registers | the merge of the attention's key splits.
//                     A row's statistics and sums never see its neighbours and do not depend on the row-block instance (1, 4 or 8
//                     rows): row r of an R-row call has the bits of the same row decoded alone.
//   dec_attn_kernel   dec_attn.h, shared with decoder_step.hip: one query against t + 1 cached keys (self) or the row's n_enc
//                     precomputed encoder keys (cross), NSPLIT key splits merged in the consumer's prologue.
//   s2s_pick_kernel   first maximum of a live row's logits into its next token slot; a row that picks eos is marked finished, a finished
//                     row receives pad.
// A step is 10 * layers + 2 launches.  For t + 1 < n_forced the next slot already holds the prompt: head and pick are skipped.
#include "common.h"

// No implicit multiply-add fusion in this file: where the compiler fuses depends on the surrounding code (the row-block instance, the
// unrolling), and a row must round the same in every instance and next to every neighbour.  The explicit fmaf of dot4 are the only FMAs.
#pragma clang fp contract(off)
#include "dec_attn.h"

namespace {

constexpr int MAXNV = 16;   // 256-float strips of the longest row (K <= 4096)
constexpr int UF = 4;       // output rows in flight per wave

enum Pro { PLAIN = 0, LNORM = 1, EMBED = 2, MERGE = 3 };

struct S2sArgs {
    const float* x;          // PLAIN / LNORM: input rows, row r at x + r * s_x
    int64_t s_x;
    const int32_t* tok;      // EMBED: token of row r at tok[r * s_tok]
    int64_t s_tok;
    const float* table;      // EMBED: [vocab, K]
    const float* pos;        // EMBED: the position's row [K]
    const float* g0;         // EMBED: embedding LayerNorm
    const float* b0;
    float* x_out;            // EMBED: the residual stream, row r at x_out + r * s_x
    int vocab;
    const float* parts;      // MERGE: [heads][NSPLIT][hd + 4] of row r at parts + r * s_x
    int hd;
    const float* gamma;      // LNORM / EMBED
    const float* beta;
    float eps;
    const float* W;          // [N, K]
    const float* bias;       // [N]
    const float* res;        // rows at res + r * s_x, or null; may alias y (element (r, n) is read and written by one thread)
    float* y;                // row r at y + r * s_y
    int64_t s_y;
    int N, nv, rpw, relu;    // nv = K / 256; rpw: output rows per workgroup (multiple of UF)
    int rows;
    const int32_t* finished; // [rows]: a finished row is neither read nor written
};

// mean and 1 / sqrt(var + eps) of the row t[0 .. nv) (this lane's float4 of every strip): the centred two-reduction form
__device__ __forceinline__ void row_stats(const float4 (&t)[MAXNV], int nv, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXNV; ++j)
        if (j < nv) s += t[j].x + t[j].y + t[j].z + t[j].w;
    const float C = (float)(nv * 256);
    mean = dyn::wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXNV; ++j)
        if (j < nv) {
            const float a0 = t[j].x - mean, a1 = t[j].y - mean, a2 = t[j].z - mean, a3 = t[j].w - mean;
            q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        }
    rstd = rsqrtf(dyn::wave_sum(q) / C + eps);
}

__device__ __forceinline__ float4 affine(float4 v, float mean, float rstd, float4 g, float4 b) {
    return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y, (v.z - mean) * rstd * g.z + b.z,
                       (v.w - mean) * rstd * g.w + b.w);
}

__device__ __forceinline__ float4 ldf4(const float* p, int i) { return reinterpret_cast<const float4*>(p)[i]; }

// JW: strips per wave (ceil(nv / 4)); RB: rows held per workgroup (>= rows); PRO: the prologue f
template <int JW, int RB, int PRO>
__global__ __launch_bounds__(256) void s2s_gemv_kernel(const S2sArgs a) {
    __shared__ float red[4][UF * RB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = a.nv, K = nv * 256;
    bool live[RB];
    bool any = false;
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
        live[rr] = rr < a.rows && a.finished[rr] == 0;
        any = any || live[rr];
    }
    if (!any) return;
    float4 xs[RB][JW];      // this wave's strips w, w + 4, ... of every row
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
#pragma unroll
        for (int jj = 0; jj < JW; ++jj) xs[rr][jj] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!live[rr]) continue;
        if (PRO == PLAIN) {
            const float* xr = a.x + rr * a.s_x;
#pragma unroll
            for (int jj = 0; jj < JW; ++jj)
                if (w + 4 * jj < nv) xs[rr][jj] = ldf4(xr, lane + 64 * (w + 4 * jj));
        } else if (PRO == MERGE) {       // x = softmax-weighted value sum of a head, put together from its NSPLIT key splits
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) {
                const int j = w + 4 * jj;
                if (j >= nv) continue;
                const int c = 4 * (lane + 64 * j), h = c / a.hd, cc = c % a.hd;
                const float* ph = a.parts + rr * a.s_x + (int64_t)h * NSPLIT * (a.hd + 4);
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
                xs[rr][jj] = make_float4(o.x * r, o.y * r, o.z * r, o.w * r);
            }
        } else {                         // LNORM / EMBED: every wave holds the whole row for its statistics, then keeps its strips
            float4 t[MAXNV];
            float mean, rstd;
            if (PRO == EMBED) {
                int64_t id = a.tok[rr * a.s_tok];
                id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);       // ids are validated on the host; never read outside the table
                const float* trow = a.table + id * K;
#pragma unroll
                for (int j = 0; j < MAXNV; ++j)
                    if (j < nv) {
                        const float4 e = ldf4(trow, lane + 64 * j), p = ldf4(a.pos, lane + 64 * j);
                        t[j] = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
                    }
                row_stats(t, nv, a.eps, mean, rstd);
#pragma unroll
                for (int j = 0; j < MAXNV; ++j)
                    if (j < nv) t[j] = affine(t[j], mean, rstd, ldf4(a.g0, lane + 64 * j), ldf4(a.b0, lane + 64 * j));
                if (blockIdx.x == 0 && w == 0) {     // the residual stream, written once (nobody reads x in this launch)
#pragma unroll
                    for (int j = 0; j < MAXNV; ++j)
                        if (j < nv) reinterpret_cast<float4*>(a.x_out + rr * a.s_x)[lane + 64 * j] = t[j];
                }
            } else {
                const float* xr = a.x + rr * a.s_x;
#pragma unroll
                for (int j = 0; j < MAXNV; ++j)
                    if (j < nv) t[j] = ldf4(xr, lane + 64 * j);
            }
            row_stats(t, nv, a.eps, mean, rstd);
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) {
                // t is indexed with compile-time constants only (it has to stay in registers): pick strip w + 4 jj by comparison
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int ww = 0; ww < 4; ++ww)
                    if (ww == w && ww + 4 * jj < MAXNV) v = t[ww + 4 * jj];
                const int j = w + 4 * jj;
                if (j < nv) xs[rr][jj] = affine(v, mean, rstd, ldf4(a.gamma, lane + 64 * j), ldf4(a.beta, lane + 64 * j));
            }
        }
    }
    const int n_base = blockIdx.x * a.rpw;
    for (int g = 0; g < a.rpw; g += UF) {
        const int n0 = n_base + g;
        if (n0 >= a.N) break;                       // uniform over the workgroup
        float s[UF][RB];
#pragma unroll
        for (int u = 0; u < UF; ++u)
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) s[u][rr] = 0.f;
        float4 wv[UF][JW];
#pragma unroll
        for (int u = 0; u < UF; ++u) {              // UF * JW independent 16-byte loads per lane
            const int n = min(n0 + u, a.N - 1);     // a tail row is loaded again, never written
            const float* wr = a.W + (int64_t)n * K;
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) {
                const int j = w + 4 * jj;
                wv[u][jj] = j < nv ? ldf4(wr, lane + 64 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int jj = 0; jj < JW; ++jj)             // per (n, r): strips ascending, then the wave reduction, then the waves in order
#pragma unroll
            for (int u = 0; u < UF; ++u)
#pragma unroll
                for (int rr = 0; rr < RB; ++rr) s[u][rr] += dot4(wv[u][jj], xs[rr][jj]);
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) {
            if (!live[rr]) continue;
#pragma unroll
            for (int u = 0; u < UF; ++u) {
                const float t = dyn::wave_sum(s[u][rr]);
                if (lane == 0) red[w][u * RB + rr] = t;
            }
        }
        __syncthreads();
        if (threadIdx.x < UF * RB) {
            const int u = threadIdx.x / RB, rr = threadIdx.x % RB, n = n0 + u;
            if (n < a.N && rr < a.rows && a.finished[rr] == 0) {
                const int i = threadIdx.x;
                float v = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
                v += a.bias[n];
                if (a.relu) v = fmaxf(v, 0.f);
                if (a.res) v += a.res[rr * a.s_x + n];
                a.y[rr * a.s_y + n] = v;
            }
        }
        __syncthreads();
    }
}

// One workgroup per row.  A finished row's slot receives pad; a live row's slot its first maximum, and eos marks the row finished.
__global__ __launch_bounds__(1024) void s2s_pick_kernel(const float* __restrict__ x, int C, int32_t* __restrict__ token_out, int64_t s_tok,
                                                        int32_t* __restrict__ finished, int eos, int pad) {
    __shared__ float rv[16];
    __shared__ int ri[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    x += row * C;
    token_out += row * s_tok;
    if (finished[row] != 0) {        // uniform over the workgroup; the flag is only written after the barrier below
        if (threadIdx.x == 0) token_out[0] = pad;
        return;
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = threadIdx.x; c < C; c += 1024) {
        const float v = x[c];
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
        if (bi == eos) finished[row] = 1;
    }
}

inline int rows_per_wg(int N) { return N >= 8192 ? 16 : (N >= 2048 ? 8 : 4); }

template <int JW, int PRO>
void launch_rb(const S2sArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)dyn::cdiv(a.N, a.rpw)), blk(256);
    if (a.rows == 1) hipLaunchKernelGGL((s2s_gemv_kernel<JW, 1, PRO>), grid, blk, 0, st, a);
    else if (a.rows <= 4) hipLaunchKernelGGL((s2s_gemv_kernel<JW, 4, PRO>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((s2s_gemv_kernel<JW, 8, PRO>), grid, blk, 0, st, a);
}

template <int PRO>
void launch(S2sArgs a, int K, hipStream_t st) {
    a.nv = K / 256;
    a.rpw = rows_per_wg(a.N);
    switch ((a.nv + 3) / 4) {
        case 1: launch_rb<1, PRO>(a, st); break;
        case 2: launch_rb<2, PRO>(a, st); break;
        case 3: launch_rb<3, PRO>(a, st); break;
        default: launch_rb<4, PRO>(a, st); break;
    }
}

inline int64_t row_scratch(int64_t dd, int64_t ff, int64_t H) { return 2 * dd + ff + H * NSPLIT * (dd / H + 4); }

}  // namespace

extern "C" int64_t dyn_seq2seq_row_scratch_floats(int64_t d_model, int64_t d_ff, int64_t heads) {
    if (d_model <= 0 || d_ff <= 0 || heads <= 0 || d_model % heads) return -1;
    return row_scratch(d_model, d_ff, heads);
}

static int seq2seq_steps_impl(const char* who, const dyn_seq2seq_desc* d, const int32_t* enc_lens, int32_t t0, int32_t n_steps, int32_t n_forced,
                              void* stream);

extern "C" int dyn_seq2seq_steps(const dyn_seq2seq_desc* d, int32_t t0, int32_t n_steps, int32_t n_forced, void* stream) {
    return seq2seq_steps_impl("dyn_seq2seq_steps", d, nullptr, t0, n_steps, n_forced, stream);
}

// The ragged batch: row r's cross-attention sees its first enc_lens[r] (device int32 [rows], clamped into [1, n_enc]) encoder keys.
extern "C" int dyn_seq2seq_steps_len(const dyn_seq2seq_desc* d, const int32_t* enc_lens, int32_t t0, int32_t n_steps, int32_t n_forced,
                                     void* stream) {
    DYN_REQUIRE(enc_lens, DYN_E_ARG, "dyn_seq2seq_steps_len: null enc_lens");
    return seq2seq_steps_impl("dyn_seq2seq_steps_len", d, enc_lens, t0, n_steps, n_forced, stream);
}

static int seq2seq_steps_impl(const char* who, const dyn_seq2seq_desc* d, const int32_t* enc_lens, int32_t t0, int32_t n_steps, int32_t n_forced,
                              void* stream) {
    DYN_REQUIRE(d, DYN_E_ARG, "%s: null descriptor", who);
    DYN_REQUIRE(d->embed && d->pos_emb && d->emb_ln_w && d->emb_ln_b && d->norm_w && d->norm_b && d->head_w && d->head_b && d->layer_ptrs &&
                    d->tokens && d->finished && d->logits && d->scratch, DYN_E_ARG, "%s: null pointer in the descriptor", who);
    const int dd = d->d_model, ff = d->d_ff, V = d->vocab, L = d->layers, H = d->heads, R = d->rows;
    DYN_REQUIRE(dd > 0 && ff > 0 && V > 0 && L > 0 && H > 0 && d->n_enc > 0 && t0 >= 0 && n_steps >= 0 && n_forced >= 0, DYN_E_ARG,
                "%s: bad sizes", who);
    DYN_REQUIRE(R >= 1 && R <= 8, DYN_E_ARG, "%s: %d rows (1 .. 8)", who, R);
    DYN_REQUIRE(dd % 256 == 0 && dd <= 4096 && ff % 256 == 0 && ff <= 4096, DYN_E_UNSUPPORTED,
                "%s: d_model %d / d_ff %d unsupported (multiples of 256 up to 4096)", who, dd, ff);
    DYN_REQUIRE(dd % H == 0, DYN_E_ARG, "%s: d_model %d not divisible by %d heads", who, dd, H);
    const int hd = dd / H;
    DYN_REQUIRE(hd >= 4 && hd <= 256 && (hd & (hd - 1)) == 0, DYN_E_UNSUPPORTED, "%s: head dim %d unsupported (power of two in 4 .. 256)", who, hd);
    DYN_REQUIRE((int64_t)t0 + n_steps <= d->max_positions, DYN_E_ARG, "%s: positions %d .. %d exceed max_positions %d", who, t0,
                t0 + n_steps - 1, d->max_positions);
    DYN_REQUIRE(d->n_enc <= MAX_KEYS && (int64_t)t0 + n_steps <= MAX_KEYS, DYN_E_UNSUPPORTED, "%s: more than %d keys per attention", who, MAX_KEYS);
    DYN_REQUIRE(d->eos_id >= 0 && d->eos_id < V && d->pad_id >= 0 && d->pad_id < V, DYN_E_ARG, "%s: eos id %d / pad id %d outside the vocabulary",
                who, d->eos_id, d->pad_id);
    DYN_REQUIRE(d->token_stride > (int64_t)t0 + n_steps, DYN_E_ARG, "%s: token_stride %lld <= last slot %d", who, (long long)d->token_stride,
                t0 + n_steps);
    DYN_REQUIRE(d->cache_stride >= ((int64_t)t0 + n_steps) * 3 * dd && d->cache_stride % 4 == 0, DYN_E_ARG,
                "%s: cache_stride %lld (>= %lld, multiple of 4)", who, (long long)d->cache_stride, ((long long)t0 + n_steps) * 3 * dd);
    DYN_REQUIRE(d->cross_stride >= (int64_t)d->n_enc * 2 * dd && d->cross_stride % 4 == 0, DYN_E_ARG,
                "%s: cross_stride %lld (>= %lld, multiple of 4)", who, (long long)d->cross_stride, (long long)d->n_enc * 2 * dd);
    const int64_t S = row_scratch(dd, ff, H);
    DYN_REQUIRE(d->scratch_floats >= R * S, DYN_E_WORKSPACE, "%s: scratch %lld < %lld floats", who, (long long)d->scratch_floats, (long long)(R * S));
    auto a16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    DYN_REQUIRE(a16(d->embed) && a16(d->pos_emb) && a16(d->emb_ln_w) && a16(d->emb_ln_b) && a16(d->norm_w) && a16(d->norm_b) && a16(d->head_w) &&
                    a16(d->logits) && a16(d->scratch), DYN_E_ARG, "%s: a pointer of the descriptor is not 16-byte aligned", who);
    for (int i = 0; i < L * DYN_S2S_PTRS_PER_LAYER; ++i)
        DYN_REQUIRE(d->layer_ptrs[i] != nullptr && a16(d->layer_ptrs[i]), DYN_E_ARG, "%s: layer pointer %d is null or not 16-byte aligned", who, i);
    hipStream_t st = (hipStream_t)stream;
    float* x = d->scratch;            // per row: residual stream [dd] | cross-attention query [dd] | relu(fc1 .) [ff] | key splits
    float* q2 = x + dd;
    float* act = q2 + dd;
    float* parts = act + ff;
    auto base = [&](const float* W, const float* bias, float* y, int64_t s_y, int N) {
        S2sArgs a{};
        a.x = x; a.s_x = S; a.W = W; a.bias = bias; a.y = y; a.s_y = s_y; a.N = N; a.rows = R; a.finished = d->finished; a.eps = d->eps;
        return a;
    };
    const float scale = 1.0f / sqrtf((float)hd);
    for (int t = t0; t < t0 + n_steps; ++t) {
        for (int l = 0; l < L; ++l) {
            const void* const* P = d->layer_ptrs + (size_t)l * DYN_S2S_PTRS_PER_LAYER;
            auto F = [&](int i) { return (const float*)P[i]; };
            float* cache = (float*)P[18];
            const float* ckv = F(19);
            float* row = cache + (int64_t)t * 3 * dd;
            // self-attention: q | k | v of this position into cache row t, then the query against rows 0 .. t
            S2sArgs a = base(F(2), F(3), row, d->cache_stride, 3 * dd);
            a.gamma = F(0); a.beta = F(1);
            if (l == 0) {
                a.tok = d->tokens + t; a.s_tok = d->token_stride; a.table = d->embed; a.pos = d->pos_emb + (int64_t)t * dd;
                a.g0 = d->emb_ln_w; a.b0 = d->emb_ln_b; a.x_out = x; a.vocab = V;
                launch<EMBED>(a, dd, st);
            } else {
                launch<LNORM>(a, dd, st);
            }
            AttnArgs s{row, cache + dd, cache + 2 * dd, parts, t + 1, 3 * dd, hd, scale, d->cache_stride, d->cache_stride, S, d->finished};
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT, R), dim3(256), (size_t)(dyn::cdiv(t + 1, NSPLIT) + 256) * sizeof(float), st, s);
            a = base(F(4), F(5), x, S, dd);
            a.parts = parts; a.hd = hd; a.res = x;
            launch<MERGE>(a, dd, st);
            // cross-attention over the row's precomputed encoder keys | values
            a = base(F(8), F(9), q2, S, dd);
            a.gamma = F(6); a.beta = F(7);
            launch<LNORM>(a, dd, st);
            AttnArgs c{q2, ckv, ckv + dd, parts, d->n_enc, 2 * dd, hd, scale, S, d->cross_stride, S, d->finished, enc_lens};
            hipLaunchKernelGGL(dec_attn_kernel, dim3(H, NSPLIT, R), dim3(256), (size_t)(dyn::cdiv(d->n_enc, NSPLIT) + 256) * sizeof(float), st, c);
            a = base(F(10), F(11), x, S, dd);
            a.parts = parts; a.hd = hd; a.res = x;
            launch<MERGE>(a, dd, st);
            // feed-forward
            a = base(F(14), F(15), act, S, ff);
            a.gamma = F(12); a.beta = F(13); a.relu = 1;
            launch<LNORM>(a, dd, st);
            a = base(F(16), F(17), x, S, dd);
            a.x = act; a.res = x;
            launch<PLAIN>(a, ff, st);
        }
        if (t + 1 < n_forced) continue;             // the next slot holds the prompt: no head, no pick
        S2sArgs a = base(d->head_w, d->head_b, d->logits, V, V);
        a.gamma = d->norm_w; a.beta = d->norm_b;
        launch<LNORM>(a, dd, st);
        hipLaunchKernelGGL(s2s_pick_kernel, dim3(R), dim3(1024), 0, st, d->logits, V, d->tokens + t + 1, d->token_stride, d->finished, d->eos_id,
                           d->pad_id);
    }
    return dyn::check_launch(who);
}
