// CTC + transformer-LM beam search on the device (reference lcasr/ctc_beam_search.py:89-319, BeamSearch.step / merge / prune /
// prune_less_than / grab_state / trim_cache, with max_cache_length = 128 as load_beamsearch sets it, lcasr/lib.py:37-72).
//
// The whole search is enqueued from ONE C call (dyn_beam_search): per frame one bookkeeping kernel and the LM step, no host
// synchronisation until the caller reads the final beams back.
//   beam_step_kernel   one workgroup: candidates, CTC prefix rules, exact merge, stable top-k, relative prune, trie insert,
//                      K/V pool mark-and-allocate, compaction of the beams that need LM scores into "rows" (count stays on device)
//   lm_gemv_kernel     y[r] = act(W . f(x[r]) + b) (+ x[r]) for every row r < *nrows: weights are read once per step for all rows
//                      (held in registers, rows staged in LDS); f = LayerNorm, optionally of the embedding + position gather
//   lm_attn_kernel     one query per (row, head) against its own gathered history (<= 128 pool rows) plus itself
//   lm_logsoftmax_kernel  log_softmax of the head's logits into the pool row of the new token (temperature 1)
//
// State.  A beam is (trie node, trailing blank, score, history): the am_sequence is [None] + the path to the node + [blank] when the
// trailing-blank bit is set, so (parent, token, trailing blank) of the node is an exact merge key once the trie is canonical —
// children are deduplicated through a hash on the whole (parent, token) key.  The history is the list of pool slots of the last
// <= 128 tokens the LM has processed for this beam (its K/V cache after grab_state / trim_cache); a pool slot holds one token's
// K/V of every layer and the next-token log-probs computed with it.  Slots are freed by marking from the live beams' lists each
// frame, never by age.  Position index of a new token = history length before the step (it stays at 128 once the cache is trimmed).
//
// Arithmetic follows the reference's fp32 tensor arithmetic with the Python constants rounded to fp32; the merge's log / exp run in
// double (math.log / math.exp).  FMA contraction is off in this file: every a * b + c is two rounded operations, as torch does it.
#pragma clang fp contract(off)
#include "common.h"

namespace {
using dyn::wave_sum;
using dyn::block_max;
using dyn::block_sum;

constexpr int HIST = 128;             // max_cache_length of load_beamsearch
constexpr int MAXC = 2688;            // candidates per frame (width * vocab): 20 * 128 fits
constexpr int HS = 4096;              // LDS merge hash (power of two, >= 1.5 * MAXC)
constexpr int MAXW = 32;
constexpr int MAXMEM = 4;             // candidates per merge key: structurally <= 3 (two beams share a node at most, plus a repeat)
constexpr unsigned long long EMPTY = ~0ull;
constexpr int PTRS_GLOBAL = 6, PTRS_LAYER = 10;

// header words of the workspace
enum { H_NB0 = 0, H_NB1 = 1, H_ERR = 2, H_NODES = 3, H_NROWS = 4, H_WORDS = 16 };

struct Layout {
    int64_t hdr, b_node, b_tb, b_score, b_hlen, b_hist, r_tok, r_pos, r_hlen, r_slot, r_hist, n_parent, n_token, h_key, h_val,
        pool_kv, pool_lp, x, q, att, u, logits, total;
    int64_t max_nodes, hash_size, pool_slots;
};

__host__ __device__ inline int64_t al(int64_t v) { return (v + 255) & ~(int64_t)255; }

Layout make_layout(int W, int64_t T, int L, int D, int F, int V) {
    Layout o;
    o.max_nodes = 1 + (int64_t)W * T;
    int64_t h = 1;
    while (h < 2 * o.max_nodes) h <<= 1;
    o.hash_size = h;
    o.pool_slots = (int64_t)W * (HIST + 1) + 1;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { int64_t r = off; off += al(bytes); return r; };
    o.hdr = take(H_WORDS * 4);
    o.b_node = take(2 * W * 4); o.b_tb = take(2 * W * 4); o.b_score = take(2 * W * 4); o.b_hlen = take(2 * W * 4);
    o.b_hist = take((int64_t)2 * W * HIST * 4);
    o.r_tok = take(W * 4); o.r_pos = take(W * 4); o.r_hlen = take(W * 4); o.r_slot = take(W * 4);
    o.r_hist = take((int64_t)W * HIST * 4);
    o.n_parent = take(o.max_nodes * 4); o.n_token = take(o.max_nodes * 4);
    o.h_key = take(o.hash_size * 8); o.h_val = take(o.hash_size * 4);
    o.pool_kv = take(o.pool_slots * L * 2 * D * 4); o.pool_lp = take(o.pool_slots * V * 4);
    o.x = take((int64_t)W * D * 4); o.q = take((int64_t)W * D * 4); o.att = take((int64_t)W * D * 4);
    o.u = take((int64_t)W * F * 4); o.logits = take((int64_t)W * V * 4);
    o.total = off;
    return o;
}

struct Rows {              // the LM work of one step; the count lives on the device
    const int* nrows;
    const int* tok;
    const int* pos;
    const int* hlen;
    const int* slot;
    const int* hist;       // [W][HIST] pool slots of each row's history (oldest first)
};

struct LM {
    int L, D, H, F, V, maxpos;
    float eps;
    const float *embed, *pos, *nw, *nb, *hw, *hb;
    const float* const* layer;   // PTRS_LAYER per layer (device-side pointer values, host array)
};

// ------------------------------------------------------------------------------------------------ bookkeeping
struct StepArgs {
    const float* lp;       // [T, ld] CTC log-probs
    int64_t ld;
    int V1;                // classes = vocab + 1; blank = V1 - 1
    int W, V;              // width, LM vocab
    float alpha, beta, blank_pen, rep_pen, top_thr, prune_val;
    int use_prune;
    char* ws;
    Layout lo;
};

__device__ __forceinline__ unsigned long long mkey(int parent, int token, int tb) {
    return ((unsigned long long)(unsigned)(parent + 1) << 17) | ((unsigned long long)(unsigned)token << 1) | (unsigned)tb;
}
__device__ __forceinline__ unsigned hash64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k;
}
__device__ __forceinline__ unsigned ordered(float f) {
    unsigned u = __float_as_uint(f == 0.f ? 0.f : f);        // -0 == +0 in Python's comparison
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// BeamSearch._sum_log_scores(s1 = incoming, s2 = kept): fp32 tensor difference, math.exp / math.log in double, the double
// rounded to fp32 and added in fp32 (a Python float meets a float32 tensor)
__device__ __forceinline__ float sum_log(float s1, float s2) {
    if (s1 >= s2) return __fadd_rn(s1, (float)log(1.0 + exp((double)__fsub_rn(s2, s1))));
    return __fadd_rn(s2, (float)log(1.0 + exp((double)__fsub_rn(s1, s2))));
}
__device__ __forceinline__ unsigned long long shfl_max64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(1024) void beam_step_kernel(const StepArgs a, int64_t t) {
    __shared__ unsigned long long hkey[HS];
    __shared__ int hcnt[HS];
    __shared__ short hmem[HS][MAXMEM];
    __shared__ float cscore[MAXC];
    __shared__ int cinfo[MAXC];             // src beam << 17 | token << 1 | kind (1 = new token)
    __shared__ short cslot[MAXC];
    __shared__ int ctok[1024];
    __shared__ int bnode[MAXW], btb[MAXW], blast[MAXW], bpar[MAXW], btk[MAXW], bhlen[MAXW], blp[MAXW];
    __shared__ float bscore[MAXW];
    __shared__ int sel[MAXW], knode[MAXW], kslot[MAXW], krow[MAXW], kfound[MAXW];
    __shared__ unsigned mark[(MAXW * (HIST + 1) + 1 + 31) / 32];
    __shared__ unsigned long long wbest[16];
    __shared__ float red[16];
    __shared__ int s_nc, s_nk, s_new, s_rows, s_err;

    const Layout& lo = a.lo;
    char* ws = a.ws;
    int* hdr = (int*)(ws + lo.hdr);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nthr = blockDim.x;
    const int in = (int)(t & 1), out = in ^ 1, W = a.W;
    const int blank = a.V1 - 1;
    const int nb = hdr[H_NB0 + in];
    if (hdr[H_ERR] != 0 || nb == 0) {
        if (tid == 0) { hdr[H_NB0 + out] = 0; hdr[H_NROWS] = 0; if (hdr[H_ERR] == 0) hdr[H_ERR] = 1; }
        return;
    }
    int* b_node = (int*)(ws + lo.b_node); int* b_tb = (int*)(ws + lo.b_tb); float* b_score = (float*)(ws + lo.b_score);
    int* b_hlen = (int*)(ws + lo.b_hlen); int* b_hist = (int*)(ws + lo.b_hist);
    int* n_parent = (int*)(ws + lo.n_parent); int* n_token = (int*)(ws + lo.n_token);
    const float* lp = a.lp + t * a.ld;

    // 1. candidate tokens: i in [1, V1) with lp[i] > lp[argmax] + top_am_threshold, ascending (token 0 is never proposed)
    const float v = tid < a.V1 ? lp[tid] : -INFINITY;
    const float mx = block_max(v, red);
    const float thr = __fadd_rn(mx, a.top_thr);
    const bool isc = tid >= 1 && tid < a.V1 && v > thr;
    const unsigned long long bal = __ballot(isc);
    __syncthreads();                                  // block_max's readers of `red` are done
    if (lane == 0) red[wv] = __int_as_float(__popcll(bal));
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < nthr / 64; ++i) { const int c = __float_as_int(red[i]); if (i < wv) before += c; total += c; }
    if (isc) ctok[before + __popcll(bal & ((1ull << lane) - 1))] = tid;
    for (int i = tid; i < HS; i += nthr) { hkey[i] = EMPTY; hcnt[i] = 0; }
    if (tid < nb) {
        const int nd = b_node[in * W + tid], tb = b_tb[in * W + tid], hl = b_hlen[in * W + tid];
        bnode[tid] = nd; btb[tid] = tb; bscore[tid] = b_score[in * W + tid]; bhlen[tid] = hl;
        bpar[tid] = n_parent[nd]; btk[tid] = n_token[nd];
        blast[tid] = tb ? blank : (nd == 0 ? -1 : n_token[nd]);        // am_sequence[-1]; the root's is None
        blp[tid] = b_hist[((int64_t)in * W + tid) * HIST + hl - 1];      // the beam's own token's pool slot: next_lm_token_lps
    }
    if (tid == 0) { s_nc = total; s_err = 0; }
    __syncthreads();
    const int nc = s_nc, n = nb * nc;
    const float* pool_lp = (const float*)(ws + lo.pool_lp);

    // 2. candidates in (beam, ascending i) order, keyed into the merge hash
    for (int c = tid; c < n; c += nthr) {
        const int b = c / nc, i = ctok[c % nc];
        const float am = lp[i];
        float s;
        unsigned long long key;
        int kind;
        if (blast[b] == i || i == blank) {           // blank or repeat: no LM score, the penalty of its kind
            s = __fadd_rn(__fadd_rn(am, bscore[b]), i == blank ? a.blank_pen : a.rep_pen);
            key = mkey(bpar[b], btk[b], i == blank ? 1 : btb[b]);
            kind = 0;
        } else {                                     // new token (replaces a trailing blank)
            const float lm = pool_lp[(int64_t)blp[b] * a.V + i];
            s = __fadd_rn(__fadd_rn(am, __fadd_rn(__fmul_rn(lm, a.alpha), a.beta)), bscore[b]);
            key = mkey(bnode[b], i, 0);
            kind = 1;
        }
        cscore[c] = s;
        cinfo[c] = (b << 17) | (i << 1) | kind;
        unsigned h = hash64(key) & (HS - 1);
        for (;;) {
            const unsigned long long prev = atomicCAS(&hkey[h], EMPTY, key);
            if (prev == EMPTY || prev == key) break;
            h = (h + 1) & (HS - 1);
        }
        const int p = atomicAdd(&hcnt[h], 1);
        if (p < MAXMEM) hmem[h][p] = (short)c; else s_err = 2;
        cslot[c] = (short)h;
    }
    __syncthreads();
    // 3. merge: the first occurrence survives; later duplicates fold into it in order
    for (int c = tid; c < n; c += nthr) {
        const int h = cslot[c], m = min(hcnt[h], MAXMEM);
        int mem[MAXMEM];
        for (int j = 0; j < m; ++j) mem[j] = hmem[h][j];
        for (int j = 1; j < m; ++j)
            for (int k = j; k > 0 && mem[k] < mem[k - 1]; --k) { const int x = mem[k]; mem[k] = mem[k - 1]; mem[k - 1] = x; }
        if (mem[0] == c) {
            float acc = cscore[c];
            for (int j = 1; j < m; ++j) acc = sum_log(cscore[mem[j]], acc);
            cscore[c] = acc;
        } else {
            cinfo[c] = -1;
        }
    }
    __syncthreads();
    // 4. stable top-W (heapq.nlargest: equal scores keep candidate order), W rounds of a block-wide max
    constexpr int PER = (MAXC + 1023) / 1024;
    unsigned long long mine[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = tid + j * nthr;
        mine[j] = (c < n && cinfo[c] >= 0) ? (((unsigned long long)ordered(cscore[c]) << 32) | (0xFFFFFFFFu - (unsigned)c)) : 0ull;
    }
    int nk = 0;
    for (; nk < W; ++nk) {
        unsigned long long best = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) best = mine[j] > best ? mine[j] : best;
        best = shfl_max64(best);
        if (lane == 0) wbest[wv] = best;
        __syncthreads();
        best = 0;
        for (int i = 0; i < nthr / 64; ++i) best = wbest[i] > best ? wbest[i] : best;
        __syncthreads();
        if (best == 0) break;
        const int c = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));
#pragma unroll
        for (int j = 0; j < PER; ++j) if (mine[j] == best) mine[j] = 0;
        if (tid == 0) sel[nk] = c;
    }
    __syncthreads();
    // 5. prune_less_than: drop beams scoring below top - prune_less_than_val (a prefix of the sorted list survives)
    if (tid == 0) {
        int k = nk;
        if (a.use_prune && nk > 0) {
            const float cut = __fsub_rn(cscore[sel[0]], a.prune_val);
            k = 0;
            while (k < nk && !(cscore[sel[k]] < cut)) ++k;
        }
        s_nk = k;
        if (k == 0) s_err = 3;                        // no candidate at all (the reference fails on beams[0] here)
    }
    for (int i = tid; i < (int)(sizeof(mark) / 4); i += nthr) mark[i] = 0u;
    __syncthreads();
    nk = s_nk;
    // 6. children of new-token beams: exact lookup of (parent, token) in the trie's hash
    unsigned long long* h_key = (unsigned long long*)(ws + lo.h_key);
    int* h_val = (int*)(ws + lo.h_val);
    const unsigned hmask = (unsigned)(lo.hash_size - 1);
    if (tid < nk) {
        const int ci = cinfo[sel[tid]];
        kfound[tid] = -1;
        if (ci & 1) {
            const int b = ci >> 17, i = (ci >> 1) & 0xFFFF;
            const unsigned long long key = ((unsigned long long)(unsigned)bnode[b] << 16) | (unsigned)i;
            unsigned h = hash64(key) & hmask;
            for (;;) {
                const unsigned long long k = h_key[h];
                if (k == key) { kfound[tid] = h_val[h]; break; }
                if (k == EMPTY) break;
                h = (h + 1) & hmask;
            }
        }
    }
    // mark every pool slot a surviving beam still references (a new-token beam's whole source history: its LM row reads it)
    for (int e = tid; e < nk * HIST; e += nthr) {
        const int k = e / HIST, j = e % HIST, b = cinfo[sel[k]] >> 17;
        if (j < bhlen[b]) {
            const int s = b_hist[((int64_t)in * W + b) * HIST + j];
            atomicOr(&mark[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
    if (tid == 0) {                                   // node ids and pool slots, in beam order (deterministic)
        int nodes = hdr[H_NODES], rows = 0, word = 0;
        for (int k = 0; k < nk; ++k) {
            krow[k] = -1;
            if (!(cinfo[sel[k]] & 1)) continue;
            if (kfound[k] < 0) {
                if (nodes >= lo.max_nodes) { s_err = 4; break; }
                knode[k] = nodes++;
            } else {
                knode[k] = kfound[k];
            }
            int s = -1;
            for (; word < (int)((lo.pool_slots + 31) / 32); ++word) {
                const unsigned fr = ~mark[word];
                if (fr) { s = word * 32 + __ffs(fr) - 1; break; }
            }
            if (s < 0 || s >= lo.pool_slots) { s_err = 5; break; }
            mark[s >> 5] |= 1u << (s & 31);
            kslot[k] = s;
            krow[k] = rows++;
        }
        s_new = nodes;
        s_rows = rows;
    }
    __syncthreads();
    if (s_err) {
        if (tid == 0) { hdr[H_ERR] = s_err; hdr[H_NB0 + out] = 0; hdr[H_NROWS] = 0; }
        return;
    }
    // 7. write the new beams, the rows of the LM step and the new trie nodes
    int* r_tok = (int*)(ws + lo.r_tok); int* r_pos = (int*)(ws + lo.r_pos); int* r_hlen = (int*)(ws + lo.r_hlen);
    int* r_slot = (int*)(ws + lo.r_slot); int* r_hist = (int*)(ws + lo.r_hist);
    if (tid < nk) {
        const int c = sel[tid], ci = cinfo[c], b = ci >> 17, i = (ci >> 1) & 0xFFFF;
        const int o = out * W + tid;
        b_score[o] = cscore[c];
        if (ci & 1) {
            const int hl = bhlen[b];
            b_node[o] = knode[tid]; b_tb[o] = 0; b_hlen[o] = min(hl + 1, HIST);
            const int r = krow[tid];
            r_tok[r] = i; r_pos[r] = hl; r_hlen[r] = hl; r_slot[r] = kslot[tid];
            if (kfound[tid] < 0) {
                n_parent[knode[tid]] = bnode[b];
                n_token[knode[tid]] = i;
                const unsigned long long key = ((unsigned long long)(unsigned)bnode[b] << 16) | (unsigned)i;
                unsigned h = hash64(key) & hmask;
                for (;;) {                                  // keys are distinct among the inserting threads
                    const unsigned long long prev = atomicCAS(&h_key[h], EMPTY, key);
                    if (prev == EMPTY) { h_val[h] = knode[tid]; break; }
                    h = (h + 1) & hmask;
                }
            }
        } else {
            b_node[o] = bnode[b]; b_tb[o] = i == blank ? 1 : btb[b]; b_hlen[o] = bhlen[b];
        }
    }
    // histories: a blank / repeat beam keeps its source's list, a new-token beam appends its slot and drops the oldest past 128
    for (int e = tid; e < nk * HIST; e += nthr) {
        const int k = e / HIST, j = e % HIST, ci = cinfo[sel[k]], b = ci >> 17, hl = bhlen[b];
        const int* src = b_hist + ((int64_t)in * W + b) * HIST;
        int* dst = b_hist + ((int64_t)out * W + k) * HIST;
        if (ci & 1) {
            const int r = krow[k];
            r_hist[r * HIST + j] = j < hl ? src[j] : 0;
            const int drop = hl + 1 > HIST ? 1 : 0, nl = min(hl + 1, HIST);
            if (j < nl) dst[j] = (j + drop < hl) ? src[j + drop] : kslot[k];
        } else if (j < hl) {
            dst[j] = src[j];
        }
    }
    if (tid == 0) { hdr[H_NB0 + out] = nk; hdr[H_NROWS] = s_rows; hdr[H_NODES] = s_new; }
}

__global__ void beam_init_kernel(char* ws, const Layout lo, int W, int bos) {
    int* hdr = (int*)(ws + lo.hdr);
    if (threadIdx.x == 0) {
        for (int i = 0; i < H_WORDS; ++i) hdr[i] = 0;
        hdr[H_NB0] = 1; hdr[H_NODES] = 1; hdr[H_NROWS] = 1;
        ((int*)(ws + lo.n_parent))[0] = -1; ((int*)(ws + lo.n_token))[0] = bos;
        ((int*)(ws + lo.b_node))[0] = 0; ((int*)(ws + lo.b_tb))[0] = 0; ((float*)(ws + lo.b_score))[0] = 0.f;
        ((int*)(ws + lo.b_hlen))[0] = 1; ((int*)(ws + lo.b_hist))[0] = 0;
        ((int*)(ws + lo.r_tok))[0] = bos; ((int*)(ws + lo.r_pos))[0] = 0; ((int*)(ws + lo.r_hlen))[0] = 0;
        ((int*)(ws + lo.r_slot))[0] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ LM step
enum { OUT_PLAIN = 0, OUT_QKV = 1 };

struct GemvArgs {
    const int* nrows;
    int W;
    const float* x; int ldx;               // input rows (ignored with EMBED)
    const int* tok; const int* pos;        // EMBED: ids and positions of the rows
    const float* embed; const float* ptab; int vocab, maxpos;
    float* x_out;                          // EMBED: the gathered rows are written here (the residual stream)
    const float* gamma; const float* beta; float eps;   // LN (null: none)
    const float* Wt; const float* bias; int N;
    int silu, residual;                    // act, y += (residual)
    float* y; int ldy;                     // OUT_PLAIN
    const int* slot; float* pool; int64_t slot_stride, layer_off; int D;   // OUT_QKV: q -> y, k / v -> pool rows
};

constexpr int RPW = 2;                     // output rows per wave
constexpr int LDS_FLOATS = 16384;          // staged input rows (64 KB)

template <int NV, bool EMBED>
__global__ __launch_bounds__(256) void lm_gemv_kernel(const GemvArgs a, int mode) {
    constexpr int K = NV * 256;
    constexpr int RC = LDS_FLOATS / K;     // rows per stage
    __shared__ float4 xs[LDS_FLOATS / 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int R = *a.nrows;
    const int n0 = (blockIdx.x * 4 + w) * RPW;
    float4 wr[RPW][NV];
#pragma unroll
    for (int o = 0; o < RPW; ++o) {
        const int nn = min(n0 + o, a.N - 1);
        const float4* row = reinterpret_cast<const float4*>(a.Wt + (int64_t)nn * K);
#pragma unroll
        for (int j = 0; j < NV; ++j) wr[o][j] = row[lane + 64 * j];
    }
    for (int r0 = 0; r0 < R; r0 += RC) {
        const int rc = min(RC, R - r0);
        __syncthreads();
        for (int rr = w; rr < rc; rr += 4) {          // stage (LayerNorm of) the rows
            const int r = r0 + rr;
            float4 xv[NV];
            if (EMBED) {
                const int id = min(max(a.tok[r], 0), a.vocab - 1), p = min(max(a.pos[r], 0), a.maxpos - 1);
                const float4* e = reinterpret_cast<const float4*>(a.embed + (int64_t)id * K);
                const float4* pp = reinterpret_cast<const float4*>(a.ptab + (int64_t)p * K);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float4 ev = e[lane + 64 * j], pv = pp[lane + 64 * j];
                    xv[j] = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
                }
                if (blockIdx.x == 0) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(a.x_out + (int64_t)r * K)[lane + 64 * j] = xv[j];
                }
            } else {
                const float4* xr = reinterpret_cast<const float4*>(a.x + (int64_t)r * a.ldx);
#pragma unroll
                for (int j = 0; j < NV; ++j) xv[j] = xr[lane + 64 * j];
            }
            if (a.gamma) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) s += xv[j].x + xv[j].y + xv[j].z + xv[j].w;
                const float mean = wave_sum(s) / K;
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float dx = xv[j].x - mean, dy = xv[j].y - mean, dz = xv[j].z - mean, dw = xv[j].w - mean;
                    q += dx * dx + dy * dy + dz * dz + dw * dw;
                }
                const float rs = rsqrtf(wave_sum(q) / K + a.eps);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float4 g = reinterpret_cast<const float4*>(a.gamma)[lane + 64 * j];
                    const float4 bb = reinterpret_cast<const float4*>(a.beta)[lane + 64 * j];
                    xv[j] = make_float4((xv[j].x - mean) * rs * g.x + bb.x, (xv[j].y - mean) * rs * g.y + bb.y,
                                        (xv[j].z - mean) * rs * g.z + bb.z, (xv[j].w - mean) * rs * g.w + bb.w);
                }
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) xs[rr * (K / 4) + lane + 64 * j] = xv[j];
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < RPW; ++o) {
            const int nn = n0 + o;
            if (nn >= a.N) break;
            const float b = a.bias ? a.bias[nn] : 0.f;
            for (int rr = 0; rr < rc; ++rr) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float4 xv = xs[rr * (K / 4) + lane + 64 * j];
                    s += wr[o][j].x * xv.x + wr[o][j].y * xv.y + wr[o][j].z * xv.z + wr[o][j].w * xv.w;
                }
                s = wave_sum(s) + b;
                if (lane != 0) continue;
                const int r = r0 + rr;
                if (a.silu) s = s / (1.f + expf(-s));
                if (mode == OUT_QKV) {
                    if (nn < a.D) a.y[(int64_t)r * a.ldy + nn] = s;
                    else a.pool[(int64_t)a.slot[r] * a.slot_stride + a.layer_off + (nn - a.D)] = s;   // [k | v] of this layer
                } else {
                    float* yp = a.y + (int64_t)r * a.ldy + nn;
                    *yp = a.residual ? *yp + s : s;
                }
            }
        }
    }
}

// one query per (row, head) against the row's history (pool slots, oldest first) plus its own key / value
__global__ __launch_bounds__(256) void lm_attn_kernel(const Rows rows, const float* q, float* att, const float* pool,
                                                      int64_t slot_stride, int64_t layer_off, int D, int hd) {
    __shared__ float sc[HIST + 1];
    __shared__ float red[16];
    __shared__ float part[256];
    const int h = blockIdx.x, r = blockIdx.y;
    if (r >= *rows.nrows) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int hl = rows.hlen[r], nk = hl + 1;
    const float scale = 1.f / sqrtf((float)hd);
    const float* qr = q + (int64_t)r * D + h * hd;
    for (int j = w; j < nk; j += 4) {
        const int s = j < hl ? rows.hist[r * HIST + j] : rows.slot[r];
        const float* kr = pool + (int64_t)s * slot_stride + layer_off + h * hd;
        float acc = 0.f;
        for (int d = lane; d < hd; d += 64) acc += qr[d] * kr[d];
        acc = wave_sum(acc);
        if (lane == 0) sc[j] = acc * scale;
    }
    __syncthreads();
    const float m = block_max(threadIdx.x < nk ? sc[threadIdx.x] : -INFINITY, red);
    float e = 0.f;
    if (threadIdx.x < nk) { e = expf(sc[threadIdx.x] - m); }
    const float den = block_sum(e, red);
    if (threadIdx.x < nk) sc[threadIdx.x] = e;
    __syncthreads();
    const int groups = 256 / hd, d = threadIdx.x % hd, g = threadIdx.x / hd;
    float o = 0.f;
    if (g < groups) {
        for (int j = g; j < nk; j += groups) {
            const int s = j < hl ? rows.hist[r * HIST + j] : rows.slot[r];
            o += sc[j] * pool[(int64_t)s * slot_stride + layer_off + D + h * hd + d];
        }
    }
    part[threadIdx.x] = o;
    __syncthreads();
    if (threadIdx.x < hd) {
        float t = 0.f;
        for (int gg = 0; gg < groups; ++gg) t += part[gg * hd + threadIdx.x];
        att[(int64_t)r * D + h * hd + threadIdx.x] = t / den;
    }
}

__global__ __launch_bounds__(256) void lm_logsoftmax_kernel(const Rows rows, const float* logits, float* pool_lp, int V) {
    __shared__ float red[16];
    const int r = blockIdx.x;
    if (r >= *rows.nrows) return;
    const float* x = logits + (int64_t)r * V;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, x[i]);
    m = block_max(m, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) s += expf(x[i] - m);
    s = block_sum(s, red);
    const float ls = logf(s);
    float* y = pool_lp + (int64_t)rows.slot[r] * V;
    for (int i = threadIdx.x; i < V; i += 256) y[i] = (x[i] - m) - ls;
}

template <bool EMBED>
int launch_gemv(const GemvArgs& a, int K, int mode, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + 4 * RPW - 1) / (4 * RPW)));
#define DYN_GEMV_CASE(nv) case nv: hipLaunchKernelGGL((lm_gemv_kernel<nv, EMBED>), grid, dim3(256), 0, st, a, mode); break;
    switch (K / 256) {
        DYN_GEMV_CASE(1) DYN_GEMV_CASE(2) DYN_GEMV_CASE(3) DYN_GEMV_CASE(4) DYN_GEMV_CASE(6) DYN_GEMV_CASE(8)
        DYN_GEMV_CASE(12) DYN_GEMV_CASE(16)
        default: dyn::set_error("beam LM: width %d has no gemv instance", K); return DYN_E_UNSUPPORTED;
    }
#undef DYN_GEMV_CASE
    return dyn::check_launch("lm_gemv_kernel");
}

bool gemv_width_ok(int K) { return K % 256 == 0 && (K / 256 <= 4 || K / 256 == 6 || K / 256 == 8 || K / 256 == 12 || K / 256 == 16); }

// the LM step for the rows in `rows` (count on the device): K / V of each row's token into its pool slot, its log-probs into the slot
int lm_step(const LM& m, const Rows& rows, int W, char* ws, const Layout& lo, hipStream_t st) {
    const int D = m.D, hd = D / m.H;
    float* x = (float*)(ws + lo.x); float* q = (float*)(ws + lo.q); float* att = (float*)(ws + lo.att);
    float* u = (float*)(ws + lo.u); float* logits = (float*)(ws + lo.logits);
    float* pool = (float*)(ws + lo.pool_kv);
    const int64_t slot_stride = (int64_t)m.L * 2 * D;
    int rc;
    for (int l = 0; l < m.L; ++l) {
        const float* const* P = m.layer + (int64_t)l * PTRS_LAYER;
        const int64_t layer_off = (int64_t)l * 2 * D;
        GemvArgs g = {};
        g.nrows = rows.nrows; g.W = W; g.x = x; g.ldx = D; g.tok = rows.tok; g.pos = rows.pos; g.embed = m.embed; g.ptab = m.pos;
        g.vocab = m.V; g.maxpos = m.maxpos; g.x_out = x; g.gamma = P[0]; g.beta = P[1]; g.eps = m.eps;
        g.Wt = P[2]; g.bias = P[3]; g.N = 3 * D; g.y = q; g.ldy = D; g.slot = rows.slot; g.pool = pool; g.slot_stride = slot_stride;
        g.layer_off = layer_off; g.D = D;
        if ((rc = (l == 0 ? launch_gemv<true>(g, D, OUT_QKV, st) : launch_gemv<false>(g, D, OUT_QKV, st))) != DYN_OK) return rc;
        hipLaunchKernelGGL(lm_attn_kernel, dim3((unsigned)m.H, (unsigned)W), dim3(256), 0, st, rows, q, att, pool, slot_stride,
                           layer_off, D, hd);
        if ((rc = dyn::check_launch("lm_attn_kernel")) != DYN_OK) return rc;
        GemvArgs o = {};
        o.nrows = rows.nrows; o.W = W; o.x = att; o.ldx = D; o.Wt = P[4]; o.bias = P[5]; o.N = D; o.residual = 1; o.y = x; o.ldy = D;
        if ((rc = launch_gemv<false>(o, D, OUT_PLAIN, st)) != DYN_OK) return rc;
        GemvArgs f1 = {};
        f1.nrows = rows.nrows; f1.W = W; f1.x = x; f1.ldx = D; f1.gamma = P[6]; f1.beta = P[7]; f1.eps = m.eps; f1.Wt = P[8];
        f1.N = m.F; f1.silu = 1; f1.y = u; f1.ldy = m.F;
        if ((rc = launch_gemv<false>(f1, D, OUT_PLAIN, st)) != DYN_OK) return rc;
        GemvArgs f2 = {};
        f2.nrows = rows.nrows; f2.W = W; f2.x = u; f2.ldx = m.F; f2.Wt = P[9]; f2.N = D; f2.residual = 1; f2.y = x; f2.ldy = D;
        if ((rc = launch_gemv<false>(f2, m.F, OUT_PLAIN, st)) != DYN_OK) return rc;
    }
    GemvArgs hd_ = {};
    hd_.nrows = rows.nrows; hd_.W = W; hd_.x = x; hd_.ldx = D; hd_.gamma = m.nw; hd_.beta = m.nb; hd_.eps = m.eps; hd_.Wt = m.hw;
    hd_.bias = m.hb; hd_.N = m.V; hd_.y = logits; hd_.ldy = m.V;
    if ((rc = launch_gemv<false>(hd_, D, OUT_PLAIN, st)) != DYN_OK) return rc;
    hipLaunchKernelGGL(lm_logsoftmax_kernel, dim3((unsigned)W), dim3(256), 0, st, rows, logits, (float*)(ws + lo.pool_lp), m.V);
    return dyn::check_launch("lm_logsoftmax_kernel");
}

int make_lm(LM& m, const void* ptrs, int L, int D, int H, int F, int V, int maxpos, float eps, const char* who) {
    const float* const* p = (const float* const*)ptrs;
    if (!p || L < 1 || H < 1 || D % H != 0 || !gemv_width_ok(D) || !gemv_width_ok(F) || V < 2 || V > 65535 || maxpos < HIST + 1 ||
        (D / H) > 256 || (D / H) % 64 != 0 || 256 % (D / H) != 0) {
        dyn::set_error("%s: unsupported LM shape (layers %d, d_model %d, heads %d, d_ff %d, vocab %d, max_positions %d)", who, L, D,
                       H, F, V, maxpos);
        return DYN_E_ARG;
    }
    for (int i = 0; i < PTRS_GLOBAL + PTRS_LAYER * L; ++i)
        if (!p[i]) { dyn::set_error("%s: LM weight pointer %d is null", who, i); return DYN_E_ARG; }
    m.L = L; m.D = D; m.H = H; m.F = F; m.V = V; m.maxpos = maxpos; m.eps = eps;
    m.embed = p[0]; m.pos = p[1]; m.nw = p[2]; m.nb = p[3]; m.hw = p[4]; m.hb = p[5]; m.layer = p + PTRS_GLOBAL;
    return DYN_OK;
}

}  // namespace

extern "C" int64_t dyn_beam_workspace_bytes(int32_t width, int64_t frames, int32_t layers, int32_t d_model, int32_t d_ff,
                                            int32_t vocab) {
    if (width < 1 || frames < 0 || layers < 1 || d_model < 1 || d_ff < 1 || vocab < 1) return -1;
    return make_layout(width, frames, layers, d_model, d_ff, vocab).total;
}

extern "C" int dyn_beam_layout(int32_t width, int64_t frames, int32_t layers, int32_t d_model, int32_t d_ff, int32_t vocab,
                               int64_t* offsets) {
    DYN_REQUIRE(offsets && width >= 1 && frames >= 0, DYN_E_ARG, "dyn_beam_layout: bad arguments");
    const Layout lo = make_layout(width, frames, layers, d_model, d_ff, vocab);
    const int64_t v[] = {lo.hdr, lo.b_node, lo.b_tb, lo.b_score, lo.b_hlen, lo.b_hist, lo.n_parent, lo.n_token, lo.pool_lp,
                         lo.r_tok, lo.r_pos, lo.r_hlen, lo.r_slot, lo.r_hist, lo.pool_kv, lo.max_nodes, lo.pool_slots, lo.total};
    for (int i = 0; i < (int)(sizeof(v) / sizeof(v[0])); ++i) offsets[i] = v[i];
    return DYN_OK;
}

extern "C" int dyn_beam_lm_rows(const void* lm_ptrs, int32_t layers, int32_t d_model, int32_t heads, int32_t d_ff, int32_t vocab,
                                int32_t max_positions, float eps, int32_t width, int64_t frames, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    LM m;
    int rc = make_lm(m, lm_ptrs, layers, d_model, heads, d_ff, vocab, max_positions, eps, "dyn_beam_lm_rows");
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(workspace && width >= 1 && width <= MAXW, DYN_E_ARG, "dyn_beam_lm_rows: bad arguments");
    const Layout lo = make_layout(width, frames, layers, d_model, d_ff, vocab);
    DYN_REQUIRE(workspace_bytes >= lo.total, DYN_E_WORKSPACE, "dyn_beam_lm_rows: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)lo.total);
    char* ws = (char*)workspace;
    const Rows rows = {(const int*)(ws + lo.hdr) + H_NROWS, (const int*)(ws + lo.r_tok), (const int*)(ws + lo.r_pos),
                       (const int*)(ws + lo.r_hlen), (const int*)(ws + lo.r_slot), (const int*)(ws + lo.r_hist)};
    return lm_step(m, rows, width, ws, lo, (hipStream_t)stream);
}

extern "C" int dyn_beam_search(const float* log_probs, int64_t frames, int64_t ld, int32_t n_classes, const void* lm_ptrs,
                               int32_t layers, int32_t d_model, int32_t heads, int32_t d_ff, int32_t vocab, int32_t max_positions,
                               float eps, int32_t bos, int32_t width, float alpha, float beta, float blank_penalty,
                               float repetition_penalty, float top_am_threshold, float prune_less_than, int32_t use_prune,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    LM m;
    int rc = make_lm(m, lm_ptrs, layers, d_model, heads, d_ff, vocab, max_positions, eps, "dyn_beam_search");
    if (rc != DYN_OK) return rc;
    DYN_REQUIRE(log_probs && workspace && frames >= 1 && ld >= n_classes && n_classes >= 2 && n_classes <= 1024 &&
                    n_classes - 1 <= vocab && width >= 1 && width <= MAXW && (int64_t)width * (n_classes - 1) <= MAXC &&
                    bos >= 0 && bos < vocab,
                DYN_E_ARG, "dyn_beam_search: bad arguments (frames %lld, classes %d, width %d, vocab %d, bos %d)",
                (long long)frames, n_classes, width, vocab, bos);
    const Layout lo = make_layout(width, frames, layers, d_model, d_ff, vocab);
    DYN_REQUIRE(workspace_bytes >= lo.total, DYN_E_WORKSPACE, "dyn_beam_search: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)lo.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (hipMemsetAsync(ws + lo.h_key, 0xFF, lo.hash_size * 8, st) != hipSuccess) {
        dyn::set_error("dyn_beam_search: memset failed");
        return DYN_E_LAUNCH;
    }
    hipLaunchKernelGGL(beam_init_kernel, dim3(1), dim3(64), 0, st, ws, lo, width, bos);
    if ((rc = dyn::check_launch("beam_init_kernel")) != DYN_OK) return rc;
    const Rows rows = {(const int*)(ws + lo.hdr) + H_NROWS, (const int*)(ws + lo.r_tok), (const int*)(ws + lo.r_pos),
                       (const int*)(ws + lo.r_hlen), (const int*)(ws + lo.r_slot), (const int*)(ws + lo.r_hist)};
    if ((rc = lm_step(m, rows, width, ws, lo, st)) != DYN_OK) return rc;     // LanguageModel.get_initial_state
    StepArgs a;
    a.lp = log_probs; a.ld = ld; a.V1 = n_classes; a.W = width; a.V = vocab; a.alpha = alpha; a.beta = beta;
    a.blank_pen = blank_penalty; a.rep_pen = repetition_penalty; a.top_thr = top_am_threshold; a.prune_val = prune_less_than;
    a.use_prune = use_prune; a.ws = ws; a.lo = lo;
    for (int64_t t = 0; t < frames; ++t) {
        hipLaunchKernelGGL(beam_step_kernel, dim3(1), dim3(1024), 0, st, a, t);
        if ((rc = dyn::check_launch("beam_step_kernel")) != DYN_OK) return rc;
        if (t + 1 < frames && (rc = lm_step(m, rows, width, ws, lo, st)) != DYN_OK) return rc;   // none after the last frame
    }
    return DYN_OK;
}
