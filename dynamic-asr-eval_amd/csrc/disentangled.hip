// SEW-D attention (transformers modeling_sew_d.py, DisentangledSelfAttention with `share_att_key`): DeBERTa-v2's disentangled score
//   score[i, j] = (q_i . k_j + q_i . Pk[t(i - j)] + k_j . Pq[t(i - j)]) / sqrt(D f),   Pq / Pk = the layer's query / key projection of the
//   relative embeddings [n_buckets = 2 span, H],   t(d) = clamp(bucket(d) + span, 0, 2 span - 1).
// The three products stay on the GEMM, already scaled: S = q k^T [M, T, T] (M = B * heads), C2P = q Pk^T [M, T, ldp] and the position ->
// content product TRANSPOSED, P2CT = Pq k^T [M, ldp, T]: for a fixed query the keys of one far bucket are then neighbours in memory.
// t depends on i - j only and is monotone non-decreasing in it, so it arrives as ONE host-built table int32 [2T - 1] (t(d) at d + T - 1:
// make_log_bucket_position's ceil(log(..)) never runs on the device) that serves both terms (transformers' p2c index
// clamp(-bucket(j - i) + span) is the same number: bucket is odd), and every bucket is one contiguous run of d, [seg_lo[r], seg_hi[r]]
// (empty when lo > hi).
//   forward:  the gather of both terms happens while softmax_row reads the row of S; nothing is materialised at [T, T].
//   backward: dC2P[i, r] = sum of dS[i, i - d] over the run of r, dP2CT[r, j] = sum of dS[j + d, j] over it: torch.gather's scatter-add
//             as segment sums, each output element ONE sum in ascending key (query) order with a plain accumulator: no float atomics, no
//             zero-fill, bit-reproducible.  Both outputs are written completely (empty buckets and the columns / rows from n_buckets to ldp:
//             exact zeros).
// `valid` (device int32 scalar, read when the kernel runs; clamped into [1, T] as the row softmax does): keys >= valid are masked in the
// forward; in the backward rows and columns >= valid of dS are not read and their rows of dC2P / columns of dP2CT are exact zeros.
// A table entry outside [0, n_buckets) is clamped into it before it is used as an index, so no table can make a kernel leave its buffers.
#include "softmax_row.h"

namespace {

constexpr int TPB = dyn::ROW_TPB;
constexpr int COL_TPB = 64;         // disentangled_p2c_bwd_kernel: one wave owns 64 neighbouring key columns

__device__ __forceinline__ int bucket_of(const int32_t* __restrict__ tab, int k, int nbk) {
    const int r = tab[k];
    return r < 0 ? 0 : (r < nbk ? r : nbk - 1);
}

// One workgroup per row (m, i), as softmax_relshift_fwd_kernel.  Row i reads tab[T - 1 + i - j] for key j: one coalesced (descending) pass.
template <int ITEMS>
__global__ __launch_bounds__(TPB) void softmax_disentangled_fwd_kernel(const float* x, float* y, const float* __restrict__ c2p,
                                                                        const float* __restrict__ p2ct, const int32_t* __restrict__ tab,
                                                                        int64_t rows, int T, int64_t ldp, int nbk,
                                                                        const int32_t* __restrict__ valid) {   // y may alias x
    __shared__ float red[16];
    const int Lv = dyn::valid_len(valid, T);
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row % T);
        const float* xr = x + row * T;
        const float* cr = c2p ? c2p + row * ldp : nullptr;
        const float* pr = p2ct ? p2ct + (row / T) * ldp * T : nullptr;
        const int32_t* tr = tab + (T - 1 + i);
        dyn::softmax_row<ITEMS, false>([=](int c) {
            const int r = bucket_of(tr, -c, nbk);
            float v = xr[c];
            if (cr) v += cr[r];
            if (pr) v += pr[(int64_t)r * T + c];
            return v;
        }, y + row * T, T, Lv, red);
    }
}

// dC2P: one workgroup per row (m, i).  The valid part of the row of dS goes through LDS (one coalesced read); thread k then sums bucket k's
// run of keys, j = i - seg_hi[k] .. i - seg_lo[k] cut to [0, Lv), in ascending j.  srow: T floats of dynamic LDS.
__global__ __launch_bounds__(TPB) void disentangled_c2p_bwd_kernel(const float* __restrict__ dS, float* __restrict__ dC,
                                                                    const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                                    int64_t rows, int T, int64_t ldp, int nbk,
                                                                    const int32_t* __restrict__ valid) {
    extern __shared__ float srow[];
    const int Lv = dyn::valid_len(valid, T);
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row % T);
        float* o = dC + row * ldp;
        if (i >= Lv) {               // a query past the utterance (uniform over the workgroup): no gradient, nothing read
            for (int64_t k = threadIdx.x; k < ldp; k += TPB) o[k] = 0.f;
            continue;
        }
        __syncthreads();             // the previous row's sums have been taken
        for (int c = threadIdx.x; c < Lv; c += TPB) srow[c] = dS[row * T + c];
        __syncthreads();
        for (int64_t k = threadIdx.x; k < ldp; k += TPB) {
            float acc = 0.f;
            if (k < nbk) {
                int64_t j0 = (int64_t)i - seg_hi[k], j1 = (int64_t)i - seg_lo[k];
                if (j0 < 0) j0 = 0;
                if (j1 > Lv - 1) j1 = Lv - 1;
                for (int64_t j = j0; j <= j1; ++j) acc += srow[j];
            }
            o[k] = acc;
        }
    }
}

// dP2CT: thread (m, j) owns key column j and walks the queries i = 0 .. Lv - 1 (a wave reads 64 neighbouring floats of one row of dS per
// step).  t(i - j) is non-decreasing in i: the run of one bucket is summed in a register and written when the bucket changes; the rows of
// the buckets the walk skips, and those past its last one up to ldp, are written as zeros, each exactly once.  (Were the table not
// monotone a run that steps back would be dropped, never written twice or out of bounds; sew_d_model.bucket_table refuses such a table.)
__global__ __launch_bounds__(COL_TPB) void disentangled_p2c_bwd_kernel(const float* __restrict__ dS, float* __restrict__ dPT,
                                                                        const int32_t* __restrict__ tab, int64_t M, int T, int64_t ldp,
                                                                        int nbk, const int32_t* __restrict__ valid) {
    const int Lv = dyn::valid_len(valid, T);
    const int64_t chunks = (T + COL_TPB - 1) / COL_TPB;
    for (int64_t blk = blockIdx.x; blk < M * chunks; blk += gridDim.x) {
        const int64_t m = blk / chunks;
        const int j = (int)(blk % chunks) * COL_TPB + (int)threadIdx.x;
        if (j >= T) continue;
        const float* g = dS + m * T * T + j;
        float* o = dPT + m * ldp * T + j;
        int64_t next = 0;            // the first bucket row of this column not written yet
        if (j < Lv) {
            const int32_t* tr = tab + (T - 1 - j);           // tr[i] = t(i - j)
            int cur = bucket_of(tr, 0, nbk);
            float acc = 0.f;
            for (int i = 0; i < Lv; ++i) {
                const int r = bucket_of(tr, i, nbk);
                if (r != cur) {
                    if (cur >= next) {
                        for (int64_t k = next; k < cur; ++k) o[k * T] = 0.f;
                        o[(int64_t)cur * T] = acc;
                        next = (int64_t)cur + 1;
                    }
                    cur = r;
                    acc = 0.f;
                }
                acc += g[(int64_t)i * T];
            }
            if (cur >= next) {
                for (int64_t k = next; k < cur; ++k) o[k * T] = 0.f;
                o[(int64_t)cur * T] = acc;
                next = (int64_t)cur + 1;
            }
        }
        for (int64_t k = next; k < ldp; ++k) o[k * T] = 0.f;
    }
}

int check_dims(const char* who, int64_t M, int64_t T, int64_t ldp, int64_t nbk, int64_t max_row) {
    DYN_REQUIRE(M >= 0 && T >= 1, DYN_E_ARG, "%s: bad sizes M=%lld T=%lld", who, (long long)M, (long long)T);
    DYN_REQUIRE(T <= max_row, DYN_E_ARG, "%s: row length %lld > %lld unsupported", who, (long long)T, (long long)max_row);
    DYN_REQUIRE(nbk >= 1 && nbk <= (1 << 20), DYN_E_ARG, "%s: n_buckets=%lld must be in 1 .. 2^20", who, (long long)nbk);
    DYN_REQUIRE(ldp >= nbk, DYN_E_ARG, "%s: ldp=%lld is shorter than the n_buckets = %lld relative positions", who, (long long)ldp,
                (long long)nbk);
    DYN_REQUIRE(ldp <= (1 << 20) && M * T <= (1ll << 31), DYN_E_ARG, "%s: too many rows for one launch", who);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_softmax_disentangled_fwd(const float* x, float* y, const float* c2p, const float* p2ct, const int32_t* table, int64_t M,
                                            int64_t T, int64_t ldp, int64_t n_buckets, const int32_t* valid_cols, void* stream) {
    DYN_REQUIRE(x && y && table, DYN_E_ARG, "dyn_softmax_disentangled_fwd: null pointer");
    DYN_REQUIRE(c2p || p2ct, DYN_E_ARG, "dyn_softmax_disentangled_fwd: both position terms are null (a plain row softmax: dyn_softmax_fwd_len)");
    if (int rc = check_dims("dyn_softmax_disentangled_fwd", M, T, ldp, n_buckets, dyn::MAX_ROW_FWD)) return rc;
    DYN_REQUIRE((const void*)y != (const void*)c2p && (const void*)y != (const void*)p2ct, DYN_E_ARG,
                "dyn_softmax_disentangled_fwd: the output may alias the scores, not a position term");
    if (M == 0) return DYN_OK;
    const int64_t rows = M * T;
    const dim3 grid((unsigned)(rows < 65535 * 4 ? rows : 65535 * 4)), blk(TPB);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dyn::dispatch_items<dyn::MAX_ROW_FWD>("dyn_softmax_disentangled_fwd", T, [&](auto I) {
            hipLaunchKernelGGL((softmax_disentangled_fwd_kernel<decltype(I)::value>), grid, blk, 0, st, x, y, c2p, p2ct, table, rows, (int)T,
                               ldp, (int)n_buckets, valid_cols);
        })) return rc;
    return dyn::check_launch("dyn_softmax_disentangled_fwd");
}

extern "C" int dyn_disentangled_bwd(const float* dS, float* dC2P, float* dP2CT, const int32_t* table, const int32_t* seg_lo,
                                    const int32_t* seg_hi, int64_t M, int64_t T, int64_t ldp, int64_t n_buckets, const int32_t* valid,
                                    void* stream) {
    DYN_REQUIRE(dS && table && seg_lo && seg_hi, DYN_E_ARG, "dyn_disentangled_bwd: null pointer");
    DYN_REQUIRE(dC2P || dP2CT, DYN_E_ARG, "dyn_disentangled_bwd: both outputs are null");
    if (int rc = check_dims("dyn_disentangled_bwd", M, T, ldp, n_buckets, dyn::MAX_ROW_BWD)) return rc;
    DYN_REQUIRE((const void*)dS != (const void*)dC2P && (const void*)dS != (const void*)dP2CT && (const void*)dC2P != (const void*)dP2CT,
                DYN_E_ARG, "dyn_disentangled_bwd: the outputs may alias neither dS nor each other");
    if (M == 0) return DYN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (dC2P) {
        const int64_t rows = M * T;
        const int64_t g = rows < 65536 ? rows : 65536;
        hipLaunchKernelGGL(disentangled_c2p_bwd_kernel, dim3((unsigned)g), dim3(TPB), (size_t)T * sizeof(float), st, dS, dC2P, seg_lo, seg_hi,
                           rows, (int)T, ldp, (int)n_buckets, valid);
        if (int rc = dyn::check_launch("dyn_disentangled_bwd")) return rc;
    }
    if (dP2CT) {
        const int64_t blocks = M * dyn::cdiv(T, (int64_t)COL_TPB);
        const int64_t g = blocks < 65536 ? blocks : 65536;
        hipLaunchKernelGGL(disentangled_p2c_bwd_kernel, dim3((unsigned)g), dim3(COL_TPB), 0, st, dS, dP2CT, table, M, (int)T, ldp, (int)n_buckets,
                           valid);
    }
    return dyn::check_launch("dyn_disentangled_bwd");
}
