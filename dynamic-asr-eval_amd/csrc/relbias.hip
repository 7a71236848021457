// WavLM attention: the gated relative-position bias (transformers modeling_wavlm.py, WavLMAttention.forward / compute_bias), the one part of
// WavLMForCTC that wav2vec2 does not have.  The reference reaches it through `AutoModelForCTC.from_pretrained(checkpoint)`
// (wav2vec2/lib.py:20-23), `model(x).logits` (:163,413) and `loss.backward()` (:194,437).
//   gate[b,head,t] = a * (c * konst[head] - 1) + 2,  a = sigmoid(p0+p1+p2+p3), c = sigmoid(p4+p5+p6+p7), p = W h[b,t,head*D:(head+1)*D] + bias
//   P[b,head,t,:]  = softmax_s(S[b,head,t,s] + gate[b,head,t] * E[bucket(s - t), head])
// All four entries are bandwidth work: the score-sized ones read and write every element of [B, nh, T, T] once, the gate ones read h once.
// bucket(d) is a host-built int32 table (a float32 log decides the bucket: no log in a kernel).  A workgroup owns ROWS consecutive query rows
// of one (batch, head); the distances those rows can see are the T + ROWS - 1 consecutive table entries it stages in LDS (as uint16: at
// most 1024 buckets) next to the head's column of E, so the per-element cost of the bias is two LDS reads.
// The backward is bit-reproducible: no float atomics anywhere, every sum has a fixed order (see dyn_relbias_bwd below).
#include "softmax_row.h"

namespace {

constexpr int TPB = dyn::ROW_TPB;
constexpr int ROWS = 16;            // query rows per workgroup (staging T + 15 table entries is 1/16 of the rows' own traffic)
constexpr int MAX_BUCKETS = 1024;   // E's column in LDS, bucket ids as uint16
constexpr int GATE_LANES = 16;      // lanes that share one (b, t, head) item of the gate kernels: a float4 each per 64 channels
constexpr int GATE_MAX_D = 256;     // gate backward: <= 4 float4 accumulators per lane and operand
constexpr int GATE_MAX_PARTIALS = 512;

// LDS staging shared by the two score-sized kernels: ecol[k] = E[k, head]; tab[w] = bucket of the distance w - (ROWS - 1) - t0, so that row
// t0 + r finds key column s at tab[s + (ROWS - 1 - r)].  Bucket ids are clamped into [0, nbk) here, once, so a bad table cannot index past ecol.
__device__ __forceinline__ void stage_bias(float* ecol, uint16_t* tab, const float* __restrict__ E, const int32_t* __restrict__ bucket,
                                           int head, int nh, int nbk, int t0, int T, int Tmax) {
    for (int k = threadIdx.x; k < nbk; k += TPB) ecol[k] = E[(int64_t)k * nh + head];
    const int W = T + ROWS - 1;
    for (int w = threadIdx.x; w < W; w += TPB) {
        const int idx = w - (ROWS - 1) - t0 + Tmax - 1;       // outside the table only for rows past T of the last block: never read
        int k = (idx >= 0 && idx < 2 * Tmax - 1) ? bucket[idx] : 0;
        k = k < 0 ? 0 : (k >= nbk ? nbk - 1 : k);
        tab[w] = (uint16_t)k;
    }
}

template <int ITEMS>
__global__ __launch_bounds__(TPB) void softmax_relbias_fwd_kernel(const float* x, float* y, const float* __restrict__ gate,
                                                                   const float* __restrict__ E, const int32_t* __restrict__ bucket, int T,
                                                                   int nh, int Tmax, int nbk, int nblk,
                                                                   const int32_t* __restrict__ valid) {   // y may alias x
    extern __shared__ __align__(16) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);
    float* ecol = red + 16;
    uint16_t* tab = reinterpret_cast<uint16_t*>(ecol + nbk);
    const int blk = blockIdx.x % nblk;
    const int64_t bh = blockIdx.x / nblk;
    const int t0 = blk * ROWS;
    stage_bias(ecol, tab, E, bucket, (int)(bh % nh), nh, nbk, t0, T, Tmax);
    __syncthreads();
    const int Lv = dyn::valid_len(valid, T);
    for (int r = 0; r < ROWS && t0 + r < T; ++r) {
        const int64_t row = bh * T + t0 + r;
        const float g = gate[row];
        const float* xr = x + row * T;
        const uint16_t* tr = tab + (ROWS - 1 - r);                 // this row's window of the staged distances: key column s at tr[s]
        dyn::softmax_row<ITEMS, false>([=](int c) { return xr[c] + g * ecol[tr[c]]; }, y + row * T, T, Lv, red);
    }
}

// Backward, kernel 1 of 3: per row dgate = sum_s dS * E[bucket]; per row block the diagonals of gate (.) dS, rows added in row order into the
// block's LDS vector diag[w] (w = s - r + ROWS - 1: one owner thread per entry and row, a barrier between rows), written to diag_ws once.
template <int ITEMS>
__global__ __launch_bounds__(TPB) void relbias_bwd_rows_kernel(const float* __restrict__ dS, const float* __restrict__ gate,
                                                                const float* __restrict__ E, const int32_t* __restrict__ bucket,
                                                                float* __restrict__ dgate, float* __restrict__ diag_ws, int T, int nh, int Tmax,
                                                                int nbk, int nblk) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int W = T + ROWS - 1;
    float* red = reinterpret_cast<float*>(smem);
    float* ecol = red + 16;
    float* diag = ecol + nbk;
    uint16_t* tab = reinterpret_cast<uint16_t*>(diag + W);
    const int blk = blockIdx.x % nblk;
    const int64_t bh = blockIdx.x / nblk;
    const int t0 = blk * ROWS;
    stage_bias(ecol, tab, E, bucket, (int)(bh % nh), nh, nbk, t0, T, Tmax);
    for (int w = threadIdx.x; w < W; w += TPB) diag[w] = 0.f;
    __syncthreads();
    for (int r = 0; r < ROWS && t0 + r < T; ++r) {
        const int64_t row = bh * T + t0 + r;
        const float g = gate[row];
        const float* gr = dS + row * T;
        const int off = ROWS - 1 - r;
        float gv[ITEMS];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int c = threadIdx.x + j * TPB;
            gv[j] = c < T ? gr[c] : 0.f;
            if (c < T) dot += gv[j] * ecol[tab[c + off]];
        }
        dot = dyn::block_sum(dot, red);                        // (its barriers also order this row's diag updates after the previous row's)
        if (threadIdx.x == 0) dgate[row] = dot;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int c = threadIdx.x + j * TPB;
            if (c < T) diag[c + off] += g * gv[j];
        }
    }
    __syncthreads();
    float* out = diag_ws + (int64_t)blockIdx.x * W;
    for (int w = threadIdx.x; w < W; w += TPB) out[w] = diag[w];
}

// Kernel 2 of 3: dist[head, d + T - 1] = sum over b, then over the row blocks whose window holds distance d, both in index order.
__global__ __launch_bounds__(TPB) void relbias_bwd_dist_kernel(const float* __restrict__ diag_ws, float* __restrict__ dist, int B, int T, int nh,
                                                                int nblk) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    const int head = blockIdx.y;
    if (i >= 2 * T - 1) return;
    const int d = i - (T - 1);
    const int W = T + ROWS - 1;
    const int below = -(d + ROWS - 1);                         // w = d + ROWS - 1 + blk * ROWS must lie in [0, W)
    const int lo = below > 0 ? (below + ROWS - 1) / ROWS : 0;
    int hi = (T - d + ROWS - 1) / ROWS;
    hi = hi < nblk ? hi : nblk;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* base = diag_ws + ((int64_t)b * nh + head) * nblk * W;
        for (int blk = lo; blk < hi; ++blk) s += base[(int64_t)blk * W + d + ROWS - 1 + blk * ROWS];
    }
    dist[(int64_t)head * (2 * T - 1) + i] = s;
}

// Kernel 3 of 3: one workgroup per head folds its 2T - 1 distance sums (LDS) into buckets, each bucket's thread adding in distance order.
__global__ __launch_bounds__(TPB) void relbias_bwd_fold_kernel(const float* __restrict__ dist, const int32_t* __restrict__ bucket, float* dE,
                                                                float beta, int T, int nh, int Tmax, int nbk) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* sd = reinterpret_cast<float*>(smem);
    const int head = blockIdx.x, n = 2 * T - 1;
    for (int i = threadIdx.x; i < n; i += TPB) sd[i] = dist[(int64_t)head * n + i];
    __syncthreads();
    const int32_t* tb = bucket + (Tmax - T);                   // tb[i] = bucket of distance i - (T - 1)
    for (int k = threadIdx.x; k < nbk; k += TPB) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) {
            int kk = tb[i];
            kk = kk < 0 ? 0 : (kk >= nbk ? nbk - 1 : kk);      // the clamp of stage_bias
            if (kk == k) s += sd[i];
        }
        float* o = dE + (int64_t)k * nh + head;
        *o = (beta != 0.f ? beta * *o : 0.f) + s;
    }
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 fma4(const float s, const float4 a, const float4 b) {
    return make_float4(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w));
}
// rows 4 * half .. 4 * half + 3 of W [8, D] summed: the gate only sees p0+p1+p2+p3 and p4+p5+p6+p7
__device__ __forceinline__ float4 wsum4(const float4* __restrict__ W4, int D4, int half, int i) {
    const float4* w = W4 + (int64_t)4 * half * D4 + i;
    return add4(add4(w[0], w[D4]), add4(w[2 * D4], w[3 * D4]));
}

// 16 lanes per (b, t, head) item, items in h's memory order: a wavefront reads 4 x 256 contiguous bytes at D = 64.
__global__ __launch_bounds__(TPB) void relpos_gate_fwd_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                               const float* __restrict__ bias, const float* __restrict__ konst,
                                                               float* __restrict__ gate, float* __restrict__ a, float* __restrict__ c,
                                                               int64_t n_items, int T, int nh, int D) {
    const int sub = threadIdx.x & (GATE_LANES - 1);
    const int64_t item = (int64_t)blockIdx.x * (TPB / GATE_LANES) + (threadIdx.x / GATE_LANES);
    const int64_t it = item < n_items ? item : n_items - 1;    // every lane stays in the shuffles
    const int head = (int)(it % nh);
    const int64_t bt = it / nh;
    const int D4 = D / 4;
    const float4* hp = reinterpret_cast<const float4*>(h + (bt * nh + head) * D);
    const float4* W4 = reinterpret_cast<const float4*>(W);
    float sa = 0.f, sc = 0.f;
    for (int i = sub; i < D4; i += GATE_LANES) {
        const float4 x = hp[i];
        sa += dot4(x, wsum4(W4, D4, 0, i));
        sc += dot4(x, wsum4(W4, D4, 1, i));
    }
#pragma unroll
    for (int o = GATE_LANES / 2; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sc += __shfl_xor(sc, o, 64);
    }
    if (sub == 0 && item < n_items) {
        const float av = dyn::sigmoidf_(sa + ((bias[0] + bias[1]) + (bias[2] + bias[3])));
        const float cv = dyn::sigmoidf_(sc + ((bias[4] + bias[5]) + (bias[6] + bias[7])));
        const int64_t b = bt / T, t = bt % T;
        const int64_t o = (b * nh + head) * T + t;
        a[o] = av;
        c[o] = cv;
        gate[o] = av * (cv * konst[head] - 1.f) + 2.f;
    }
}

// Backward of the gate: a workgroup owns `per_wg` consecutive items; each of its 16 lane groups walks every 16th of them in order, adding
// dpa * h and dpc * h (dpa / dpc: gradients of the two pre-sigmoid sums) into registers, writes dh, and the 16 groups are combined through
// LDS in group order into one partial row [2D + 2] = (dWa [D], dWc [D], dba, dbc) of this workgroup.
__global__ __launch_bounds__(TPB) void relpos_gate_bwd_kernel(const float* __restrict__ dgate, const float* __restrict__ a,
                                                               const float* __restrict__ c, const float* __restrict__ h,
                                                               const float* __restrict__ W, const float* __restrict__ konst, float* dh,
                                                               float beta_dh, float* __restrict__ partial, int64_t n_items, int64_t per_wg,
                                                               int T, int nh, int D) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds = reinterpret_cast<float*>(smem);               // [16][2D + 4]: rows stay 16-byte aligned for the float4 stores
    const int sub = threadIdx.x & (GATE_LANES - 1), grp = threadIdx.x / GATE_LANES;
    const int D4 = D / 4, ncol = 2 * D + 2, ldl = 2 * D + 4;
    const float4* W4 = reinterpret_cast<const float4*>(W);
    float4 wa[4], wc[4], accA[4], accC[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = sub + q * GATE_LANES;
        wa[q] = wc[q] = accA[q] = accC[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < D4) { wa[q] = wsum4(W4, D4, 0, i); wc[q] = wsum4(W4, D4, 1, i); }
    }
    float sA = 0.f, sC = 0.f;
    const int64_t base = (int64_t)blockIdx.x * per_wg;
    const int64_t end = base + per_wg < n_items ? base + per_wg : n_items;
    for (int64_t item = base + grp; item < end; item += TPB / GATE_LANES) {
        const int head = (int)(item % nh);
        const int64_t bt = item / nh;
        const int64_t idx = ((bt / T) * nh + head) * T + bt % T;
        const float g = dgate[idx], av = a[idx], cv = c[idx], k = konst[head];
        const float dpa = g * (cv * k - 1.f) * av * (1.f - av);
        const float dpc = g * av * k * cv * (1.f - cv);
        const float4* hp = reinterpret_cast<const float4*>(h + (bt * nh + head) * D);
        float4* dp = reinterpret_cast<float4*>(dh + (bt * nh + head) * D);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = sub + q * GATE_LANES;
            if (i < D4) {
                const float4 x = hp[i];
                accA[q] = fma4(dpa, x, accA[q]);
                accC[q] = fma4(dpc, x, accC[q]);
                float4 d = make_float4(dpa * wa[q].x + dpc * wc[q].x, dpa * wa[q].y + dpc * wc[q].y, dpa * wa[q].z + dpc * wc[q].z,
                                       dpa * wa[q].w + dpc * wc[q].w);
                if (beta_dh != 0.f) d = fma4(beta_dh, dp[i], d);
                dp[i] = d;
            }
        }
        sA += dpa;
        sC += dpc;
    }
    float* mine = lds + grp * ldl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = sub + q * GATE_LANES;
        if (i < D4) {
            *reinterpret_cast<float4*>(mine + 4 * i) = accA[q];
            *reinterpret_cast<float4*>(mine + D + 4 * i) = accC[q];
        }
    }
    if (sub == 0) { mine[2 * D] = sA; mine[2 * D + 1] = sC; }
    __syncthreads();
    for (int col = threadIdx.x; col < ncol; col += TPB) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < TPB / GATE_LANES; ++g) s += lds[g * ldl + col];
        partial[(int64_t)blockIdx.x * ncol + col] = s;
    }
}

// Ends the gate backward.  Blocks [0, nh): dkonst[head] = beta * old + sum_{b, t} dgate * a * c (d gate / d konst = a * c), per thread in
// (b, t) order, then the block sum.  The other blocks: one thread per column of the partial rows adds them in workgroup order; the four rows
// of W (and of bias) behind one sigmoid share one sum, so each column is written four times.
__global__ __launch_bounds__(TPB) void relpos_gate_bwd_finish_kernel(const float* __restrict__ dgate, const float* __restrict__ a,
                                                                      const float* __restrict__ c, const float* __restrict__ partial,
                                                                      float* dW, float* dbias, float* dkonst, float beta, int B, int T, int nh,
                                                                      int D, int P) {
    __shared__ float red[16];
    auto put = [beta](float* o, float v) { *o = (beta != 0.f ? beta * *o : 0.f) + v; };
    if ((int)blockIdx.x < nh) {
        const int head = blockIdx.x;
        float s = 0.f;
        for (int b = 0; b < B; ++b) {
            const int64_t o = ((int64_t)b * nh + head) * T;
            for (int t = threadIdx.x; t < T; t += TPB) s += dgate[o + t] * a[o + t] * c[o + t];
        }
        s = dyn::block_sum(s, red);
        if (threadIdx.x == 0) put(dkonst + head, s);
        return;
    }
    const int ncol = 2 * D + 2;
    const int col = ((int)blockIdx.x - nh) * TPB + threadIdx.x;
    if (col >= ncol) return;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += partial[(int64_t)p * ncol + col];
    if (col < 2 * D) {
        const int half = col / D, i = col % D;
        for (int j = 0; j < 4; ++j) put(dW + (int64_t)(4 * half + j) * D + i, s);
    } else {
        const int half = col - 2 * D;
        for (int j = 0; j < 4; ++j) put(dbias + 4 * half + j, s);
    }
}

// Argument checks shared by the four entries (host side, before any launch).
int check_dims(const char* who, int64_t B, int64_t T, int64_t H, int64_t nh) {
    DYN_REQUIRE(B >= 0 && T > 0 && H > 0 && nh > 0, DYN_E_ARG, "%s: bad sizes B=%lld T=%lld H=%lld heads=%lld", who, (long long)B, (long long)T,
                (long long)H, (long long)nh);
    DYN_REQUIRE(H % nh == 0, DYN_E_ARG, "%s: hidden size %lld is not a multiple of %lld heads", who, (long long)H, (long long)nh);
    DYN_REQUIRE((H / nh) % 4 == 0, DYN_E_ARG, "%s: head dimension %lld is not a multiple of 4", who, (long long)(H / nh));
    return DYN_OK;
}
int check_table(const char* who, int64_t B, int64_t T, int64_t nh, int64_t Tmax, int64_t num_buckets, int64_t max_T) {
    DYN_REQUIRE(num_buckets >= 2 && num_buckets % 2 == 0 && num_buckets <= MAX_BUCKETS, DYN_E_ARG,
                "%s: num_buckets=%lld must be even and in [2, %d]", who, (long long)num_buckets, MAX_BUCKETS);
    DYN_REQUIRE(T <= max_T, DYN_E_ARG, "%s: row length %lld > %lld unsupported", who, (long long)T, (long long)max_T);
    DYN_REQUIRE(Tmax >= T && Tmax <= (1 << 29), DYN_E_ARG, "%s: the bucket table covers %lld frames, the scores have %lld", who, (long long)Tmax,
                (long long)T);
    DYN_REQUIRE(nh <= 65535 && B * nh * dyn::cdiv(T, ROWS) <= INT32_MAX, DYN_E_ARG, "%s: too many rows for one launch", who);
    return DYN_OK;
}

int64_t gate_bwd_per_wg(int64_t n_items) {       // items per workgroup: a multiple of 16, at most GATE_MAX_PARTIALS workgroups
    const int64_t g = TPB / GATE_LANES;
    int64_t per = dyn::cdiv(n_items, GATE_MAX_PARTIALS);
    if (per < 4 * g) per = 4 * g;
    return dyn::cdiv(per, g) * g;
}

}  // namespace

extern "C" int dyn_relpos_gate_fwd(const float* h, const float* W, const float* bias, const float* konst, float* gate, float* a, float* c,
                                   int64_t B, int64_t T, int64_t H, int64_t nh, void* stream) {
    DYN_REQUIRE(h && W && bias && konst && gate && a && c, DYN_E_ARG, "dyn_relpos_gate_fwd: null pointer");
    if (int rc = check_dims("dyn_relpos_gate_fwd", B, T, H, nh)) return rc;
    const int64_t n = B * T * nh;
    if (n == 0) return DYN_OK;
    const int64_t per = TPB / GATE_LANES;
    DYN_REQUIRE(dyn::cdiv(n, per) <= INT32_MAX, DYN_E_ARG, "dyn_relpos_gate_fwd: too many rows for one launch");
    hipLaunchKernelGGL(relpos_gate_fwd_kernel, dim3((unsigned)dyn::cdiv(n, per)), dim3(TPB), 0, (hipStream_t)stream, h, W, bias, konst, gate, a,
                       c, n, (int)T, (int)nh, (int)(H / nh));
    return dyn::check_launch("dyn_relpos_gate_fwd");
}

extern "C" int dyn_softmax_relbias_fwd_len(const float* x, float* y, const float* gate, const float* E, const int32_t* bucket, int64_t B,
                                           int64_t T, int64_t H, int64_t nh, int64_t Tmax, int64_t num_buckets, const int32_t* valid_cols,
                                           void* stream) {
    DYN_REQUIRE(x && y && gate && E && bucket, DYN_E_ARG, "dyn_softmax_relbias_fwd_len: null pointer");
    if (int rc = check_dims("dyn_softmax_relbias_fwd_len", B, T, H, nh)) return rc;
    if (int rc = check_table("dyn_softmax_relbias_fwd_len", B, T, nh, Tmax, num_buckets, dyn::MAX_ROW_FWD)) return rc;
    if (B == 0) return DYN_OK;
    const int nblk = (int)dyn::cdiv(T, ROWS);
    const dim3 grid((unsigned)(B * nh * nblk)), blk(TPB);
    const size_t lds = (16 + num_buckets) * sizeof(float) + (T + ROWS - 1) * sizeof(uint16_t);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dyn::dispatch_items<dyn::MAX_ROW_FWD>("dyn_softmax_relbias_fwd_len", T, [&](auto I) {
            hipLaunchKernelGGL((softmax_relbias_fwd_kernel<decltype(I)::value>), grid, blk, lds, st, x, y, gate, E, bucket, (int)T, (int)nh, (int)Tmax,
                               (int)num_buckets, nblk, valid_cols);
        })) return rc;
    return dyn::check_launch("dyn_softmax_relbias_fwd_len");
}

// workspace: the row blocks' diagonal vectors [B, nh, ceil(T / 16), T + 15], then the per-head distance sums [nh, 2T - 1]
extern "C" int64_t dyn_relbias_bwd_workspace_bytes(int64_t B, int64_t nh, int64_t T, int64_t num_buckets) {
    (void)num_buckets;
    if (B < 0 || nh <= 0 || T <= 0) return 0;
    return (B * nh * dyn::cdiv(T, ROWS) * (T + ROWS - 1) + nh * (2 * T - 1)) * (int64_t)sizeof(float);
}

extern "C" int dyn_relbias_bwd(const float* dS, const float* gate, const float* E, const int32_t* bucket, float* dgate, float* dE, float beta,
                               int64_t B, int64_t T, int64_t H, int64_t nh, int64_t Tmax, int64_t num_buckets, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(dS && gate && E && bucket && dgate && dE && workspace, DYN_E_ARG, "dyn_relbias_bwd: null pointer");
    if (int rc = check_dims("dyn_relbias_bwd", B, T, H, nh)) return rc;
    if (int rc = check_table("dyn_relbias_bwd", B, T, nh, Tmax, num_buckets, dyn::MAX_ROW_BWD)) return rc;
    DYN_REQUIRE(workspace_bytes >= dyn_relbias_bwd_workspace_bytes(B, nh, T, num_buckets), DYN_E_WORKSPACE,
                "dyn_relbias_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)dyn_relbias_bwd_workspace_bytes(B, nh, T, num_buckets));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)dyn::cdiv(T, ROWS);
    const int64_t W = T + ROWS - 1;
    float* diag_ws = static_cast<float*>(workspace);
    float* dist = diag_ws + B * nh * nblk * W;
    if (B > 0) {
        const dim3 grid((unsigned)(B * nh * nblk)), blk(TPB);
        const size_t lds = (16 + num_buckets + W) * sizeof(float) + W * sizeof(uint16_t);
        if (int rc = dyn::dispatch_items<dyn::MAX_ROW_BWD>("dyn_relbias_bwd", T, [&](auto I) {
                hipLaunchKernelGGL((relbias_bwd_rows_kernel<decltype(I)::value>), grid, blk, lds, st, dS, gate, E, bucket, dgate, diag_ws, (int)T, (int)nh,
                                   (int)Tmax, (int)num_buckets, nblk);
            })) return rc;
        if (int rc = dyn::check_launch("dyn_relbias_bwd")) return rc;
    }
    hipLaunchKernelGGL(relbias_bwd_dist_kernel, dim3((unsigned)dyn::cdiv(2 * T - 1, TPB), (unsigned)nh), dim3(TPB), 0, st, diag_ws, dist, (int)B,
                       (int)T, (int)nh, nblk);
    hipLaunchKernelGGL(relbias_bwd_fold_kernel, dim3((unsigned)nh), dim3(TPB), (size_t)(2 * T - 1) * sizeof(float), st, dist, bucket, dE, beta,
                       (int)T, (int)nh, (int)Tmax, (int)num_buckets);
    return dyn::check_launch("dyn_relbias_bwd");
}

extern "C" int64_t dyn_relpos_gate_bwd_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t nh) {
    if (B < 0 || T <= 0 || H <= 0 || nh <= 0 || H % nh) return 0;
    const int64_t n = B * T * nh;
    return dyn::cdiv(n, gate_bwd_per_wg(n)) * (2 * (H / nh) + 2) * (int64_t)sizeof(float);
}

extern "C" int dyn_relpos_gate_bwd(const float* dgate, const float* a, const float* c, const float* h, const float* W, const float* konst,
                                   float* dh, float beta_dh, float* dW, float* dbias, float* dkonst, float beta, int64_t B, int64_t T,
                                   int64_t H, int64_t nh, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(dgate && a && c && h && W && konst && dh && dW && dbias && dkonst && workspace, DYN_E_ARG, "dyn_relpos_gate_bwd: null pointer");
    if (int rc = check_dims("dyn_relpos_gate_bwd", B, T, H, nh)) return rc;
    const int64_t D = H / nh;
    DYN_REQUIRE(D <= GATE_MAX_D, DYN_E_ARG, "dyn_relpos_gate_bwd: head dimension %lld > %d unsupported", (long long)D, GATE_MAX_D);
    DYN_REQUIRE(T <= INT32_MAX && B <= INT32_MAX && nh <= 65535, DYN_E_ARG, "dyn_relpos_gate_bwd: sizes out of range");
    DYN_REQUIRE(workspace_bytes >= dyn_relpos_gate_bwd_workspace_bytes(B, T, H, nh), DYN_E_WORKSPACE,
                "dyn_relpos_gate_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)dyn_relpos_gate_bwd_workspace_bytes(B, T, H, nh));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = B * T * nh;
    const int64_t per = gate_bwd_per_wg(n);
    const int P = (int)dyn::cdiv(n, per);
    float* partial = static_cast<float*>(workspace);
    if (P > 0) {
        const size_t lds = (size_t)(TPB / GATE_LANES) * (2 * D + 4) * sizeof(float);
        hipLaunchKernelGGL(relpos_gate_bwd_kernel, dim3((unsigned)P), dim3(TPB), lds, st, dgate, a, c, h, W, konst, dh, beta_dh, partial, n, per,
                           (int)T, (int)nh, (int)D);
        if (int rc = dyn::check_launch("dyn_relpos_gate_bwd")) return rc;
    }
    hipLaunchKernelGGL(relpos_gate_bwd_finish_kernel, dim3((unsigned)(nh + dyn::cdiv(2 * D + 2, TPB))), dim3(TPB), 0, st, dgate, a, c, partial, dW,
                       dbias, dkonst, beta, (int)B, (int)T, (int)nh, (int)D, P);
    return dyn::check_launch("dyn_relpos_gate_bwd");
}
