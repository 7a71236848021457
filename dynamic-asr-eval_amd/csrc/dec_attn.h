// The one-query attention of the one-token decoder steps, for both files that run it: decoder_step.hip (dyn_decoder_steps*) and
// seq2seq_step.hip (dyn_seq2seq_steps).  One query against n cached keys / values, NSPLIT workgroups per head (a share of the keys each):
// scores into LDS (16 lanes per key row, four rows in flight), exponentials, weighted sum of the value rows.  The NSPLIT
// (sum, max, denominator) triples of a head are merged in the prologue of the projection that consumes them.
// Both files switch floating-point contraction off and include this header after the pragma: the explicit fmaf below are the only FMAs.
#pragma once
#include "common.h"

namespace {

// explicit fused multiply-adds on the hot sums: with contraction off these are the only FMAs, the same in every kernel
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

constexpr int NSPLIT = 4;   // key splits of the one-query attention (one workgroup each); merged in the consumer's prologue

constexpr int MAX_KEYS = 4 * 12288;   // (n_keys / NSPLIT + 256) floats of LDS <= 50 KB

struct AttnArgs {
    const float* q;    // [heads * hd]
    const float* k;    // row j of head h at k + j * ld + h * hd
    const float* v;
    float* parts;      // [heads][NSPLIT][hd + 4]: unnormalised weighted value sum | score maximum | sum of exponentials of this split's keys
    int n_keys, ld, hd;
    float scale;
    // rows of a batched step (blockIdx.z): floats between rows of q / k and v / parts; a finished row does nothing
    int64_t s_q, s_kv, s_parts;
    const int32_t* finished;
    // a ragged batch (null: every row has n_keys): row z attends to its first row_keys[z] keys, clamped into [1, n_keys]; the launch's
    // LDS stays sized by n_keys.  Row z's splits are those of a launch with n_keys = row_keys[z]: the same chunks, the same bits.
    const int32_t* row_keys;
};

// One query; workgroup (h, s) takes the s-th quarter of the keys of head h.  LDS: the split's scores, then 256 partial sums.
__global__ __launch_bounds__(256) void dec_attn_kernel(const AttnArgs a) {
    extern __shared__ float sc[];
    __shared__ float red[16];
    const int h = blockIdx.x, tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const int hd = a.hd;
    const int64_t z = blockIdx.z;
    if (a.finished && a.finished[z] != 0) return;
    int n_keys = a.n_keys;
    if (a.row_keys) n_keys = max(1, min(a.row_keys[z], n_keys));
    const int chunk = (n_keys + NSPLIT - 1) / NSPLIT;
    const int j_lo = blockIdx.y * chunk;
    const int n = min(chunk, n_keys - j_lo);         // keys of this split (<= 0: none)
    float* out = a.parts + z * a.s_parts + ((int64_t)h * NSPLIT + blockIdx.y) * (hd + 4);
    if (n <= 0) {
        if (tid < hd) out[tid] = 0.f;
        if (tid == 0) { out[hd] = -INFINITY; out[hd + 1] = 0.f; }
        return;
    }
    const float* q = a.q + z * a.s_q + h * hd;
    const float* k = a.k + z * a.s_kv + (int64_t)j_lo * a.ld + h * hd;
    const float* v = a.v + z * a.s_kv + (int64_t)j_lo * a.ld + h * hd;
    float4 qv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = l * 4 + 64 * i;
        qv[i] = c < hd ? *reinterpret_cast<const float4*>(q + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // 16 lanes per key row, four rows in flight per 16-lane group (the loads of a group are independent: one latency per 64 keys)
    for (int j0 = g; j0 < n; j0 += 64) {
        float s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 16 * u;
            const float* kr = k + (int64_t)(j < n ? j : j0) * a.ld;
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = l * 4 + 64 * i;
                if (c < hd) t += dot4(*reinterpret_cast<const float4*>(kr + c), qv[i]);
            }
            s[u] = t;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float t = s[u];
            t += __shfl_xor(t, 8, 64);
            t += __shfl_xor(t, 4, 64);
            t += __shfl_xor(t, 2, 64);
            t += __shfl_xor(t, 1, 64);
            if (l == 0 && j0 + 16 * u < n) sc[j0 + 16 * u] = t * a.scale;
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < n; j += 256) m = fmaxf(m, sc[j]);
    m = dyn::block_max(m, red);
    float sum = 0.f;
    for (int j = tid; j < n; j += 256) {
        const float e = __expf(sc[j] - m);
        sc[j] = e;
        sum += e;
    }
    sum = dyn::block_sum(sum, red);               // its barriers also publish the exponentials
    const int c = tid % hd, kg = tid / hd, ng = 256 / hd;
    float acc = 0.f;
    {   // eight value rows in flight per thread; the summation order (increasing j) does not depend on the unrolling
        int j = kg;
        for (; j + 7 * ng < n; j += 8 * ng) {
            float vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = v[(int64_t)(j + u * ng) * a.ld + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(sc[j + u * ng], vv[u], acc);
        }
        for (; j < n; j += ng) acc = fmaf(sc[j], v[(int64_t)j * a.ld + c], acc);
    }
    float* part = sc + n;
    part[tid] = acc;
    __syncthreads();
    if (tid < hd) {
        float t = 0.f;
        for (int i = 0; i < ng; ++i) t += part[i * hd + tid];
        out[tid] = t;
    }
    if (tid == 0) { out[hd] = m; out[hd + 1] = sum; }
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

}  // namespace
