// Wav2Vec2-Conformer attention with `position_embeddings_type: "relative"` (transformers modeling_wav2vec2_conformer.py,
// Wav2Vec2ConformerSelfAttention._apply_relative_embeddings): the Transformer-XL score
//   score[i, j] = ((q_i + u_h) . k_j + (q_i + v_h) . P_h[T - 1 - i + j]) / sqrt(D),   P = linear_pos(pe), pe [2T - 1, H]
// The two products stay on the GEMM: S = (q + u) k^T [B, nh, T, T] and BD = (q + v) P_h^T [B, nh, T, ld_bd >= 2T - 1], both already scaled.
// transformers' "pad, view, slice" shift of BD reads bd[i, T - 1 - i + j]: row i's window of T floats starts at column T - 1 - i, one float
// earlier on every row.  Nothing is copied for it here: the forward kernel adds the window while it reads S for the softmax, the backward
// kernel writes dS back into the window of a [T, ld_bd] row and zeros around it (the buffer is reused scratch: every column is written).
// The other two entries serve the biases u, v [nh, D] = [H] (head-major, so they are a per-channel vector of the [B, T, H] projections):
// q + u and q + v in one pass over q, and back dq = dQu + dQv with the column sums du, dv in a fixed order (no float atomics).
// All four are bandwidth work with 4-byte accesses where a row's start is not aligned (BD's window) and 16-byte ones where it is.
#include "softmax_row.h"

namespace {

constexpr int TPB = dyn::ROW_TPB;
constexpr int HB_ROWS = 8;          // rows a workgroup of head_bias_bwd sums at least
constexpr int HB_MAX_CHUNKS = 512;

// One workgroup per row, as softmax_fwd_kernel (nothing is shared between rows here, so a row block would only serialise them): the row of
// x and the row's window of bd are read once into registers (ITEMS values per thread, coalesced stride-256 accesses), the result is written once.
// LENS (a ragged batch): `valid` holds one key count per batch entry and rows_per_len = nh * T rows share one; the instances without it
// are the code as it was (the per-row division costs 2 - 8 VGPRs in the row loop, so it is not in them).
template <int ITEMS, bool LENS = false>
__global__ __launch_bounds__(TPB) void softmax_relshift_fwd_kernel(const float* x, float* y, const float* __restrict__ bd, int64_t rows, int T,
                                                                    int64_t ld_bd, const int32_t* __restrict__ valid,
                                                                    int64_t rows_per_len) {   // y may alias x
    __shared__ float red[16];
    const int Lv0 = dyn::valid_len(valid, T);
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int Lv = LENS ? dyn::valid_len_of_row(valid, row, rows_per_len, T) : Lv0;
        const int i = (int)(row % T);                          // query position inside its (batch, head)
        const float* xr = x + row * T;
        const float* br = bd + row * ld_bd + (T - 1 - i);      // the row's window: columns T-1-i .. 2T-2-i, inside [0, 2T-1)
        dyn::softmax_row<ITEMS, false>([=](int c) { return xr[c] + br[c]; }, y + row * T, T, Lv, red);
    }
}

// dBD[m, i, k] = dS[m, i, k - (T - 1) + i] inside the row's window, 0 elsewhere (the columns past 2T - 1 of a padded row included).
__global__ __launch_bounds__(TPB) void relshift_bwd_kernel(const float* __restrict__ dS, float* __restrict__ dBD, int64_t rows, int T,
                                                            int64_t ld_bd) {
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row % T);
        const float* gr = dS + row * T;
        float* o = dBD + row * ld_bd;
        const int lo = T - 1 - i;
        for (int64_t k = threadIdx.x; k < ld_bd; k += TPB) {
            const int64_t c = k - lo;
            o[k] = (c >= 0 && c < T) ? gr[c] : 0.f;
        }
    }
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// qu[r, c] = q[r * ldq + c] + u[c], qv[r, c] = q[r * ldq + c] + v[c]: q is read once.
__global__ __launch_bounds__(TPB) void head_bias_add_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ u,
                                                             const float* __restrict__ v, float* __restrict__ qu, float* __restrict__ qv,
                                                             int64_t rows, int H4) {
    const int64_t total = rows * H4;
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
        const int64_t r = idx / H4;
        const int c4 = (int)(idx % H4);
        const float4 x = reinterpret_cast<const float4*>(q + r * ldq)[c4];
        reinterpret_cast<float4*>(qu)[idx] = add4(x, reinterpret_cast<const float4*>(u)[c4]);
        reinterpret_cast<float4*>(qv)[idx] = add4(x, reinterpret_cast<const float4*>(v)[c4]);
    }
}

// A workgroup owns `per` consecutive rows and 256 channels: dq = dQu + dQv, and the two column sums of its rows, in row order, as one
// partial row each (combined afterwards in workgroup order by the fixed-order reducer).
__global__ __launch_bounds__(TPB) void head_bias_bwd_kernel(const float* __restrict__ dqu, const float* __restrict__ dqv, float* __restrict__ dq,
                                                             int64_t ldq, float* __restrict__ pu, float* __restrict__ pv, int64_t rows,
                                                             int64_t per, int H) {
    const int c = blockIdx.y * TPB + threadIdx.x;
    if (c >= H) return;
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < rows ? r0 + per : rows;
    float su = 0.f, sv = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const float a = dqu[r * H + c], b = dqv[r * H + c];
        dq[r * ldq + c] = a + b;
        su += a;
        sv += b;
    }
    pu[(int64_t)blockIdx.x * H + c] = su;
    pv[(int64_t)blockIdx.x * H + c] = sv;
}

int check_scores(const char* who, int64_t M, int64_t T, int64_t ld_bd) {
    DYN_REQUIRE(M >= 0 && T >= 1, DYN_E_ARG, "%s: bad sizes rows=%lld T=%lld", who, (long long)M, (long long)T);
    DYN_REQUIRE(T <= dyn::MAX_ROW_FWD, DYN_E_ARG, "%s: row length %lld > %d unsupported", who, (long long)T, dyn::MAX_ROW_FWD);
    DYN_REQUIRE(ld_bd >= 2 * T - 1, DYN_E_ARG, "%s: ld_bd=%lld is shorter than the 2T - 1 = %lld relative positions", who, (long long)ld_bd,
                (long long)(2 * T - 1));
    DYN_REQUIRE(ld_bd <= (1 << 20) && M * T <= (1ll << 40), DYN_E_ARG, "%s: too many rows for one launch", who);
    return DYN_OK;
}

int64_t hb_chunks(int64_t rows, int64_t* per) {
    int64_t chunks = dyn::cdiv(rows, HB_ROWS);
    if (chunks > HB_MAX_CHUNKS) chunks = HB_MAX_CHUNKS;
    if (chunks < 1) chunks = 1;
    *per = dyn::cdiv(rows > 0 ? rows : 1, chunks);
    return dyn::cdiv(rows > 0 ? rows : 1, *per);
}

}  // namespace

extern "C" int dyn_softmax_relshift_fwd_len(const float* x, float* y, const float* bd, int64_t M, int64_t T, int64_t ld_bd,
                                            const int32_t* valid_cols, void* stream) {
    DYN_REQUIRE(x && y && bd, DYN_E_ARG, "dyn_softmax_relshift_fwd_len: null pointer");
    if (int rc = check_scores("dyn_softmax_relshift_fwd_len", M, T, ld_bd)) return rc;
    DYN_REQUIRE((const void*)y != (const void*)bd, DYN_E_ARG, "dyn_softmax_relshift_fwd_len: the output may alias the scores, not BD");
    if (M == 0) return DYN_OK;
    const int64_t rows = M * T;
    const dim3 grid((unsigned)(rows < 65535 * 4 ? rows : 65535 * 4)), blk(TPB);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dyn::dispatch_items<dyn::MAX_ROW_FWD>("dyn_softmax_relshift_fwd_len", T, [&](auto I) {
            hipLaunchKernelGGL((softmax_relshift_fwd_kernel<decltype(I)::value, false>), grid, blk, 0, st, x, y, bd, rows, (int)T, ld_bd, valid_cols,
                               (int64_t)0);
        })) return rc;
    return dyn::check_launch("dyn_softmax_relshift_fwd_len");
}

// The ragged batch: x [B, nh, T, T], row m of the B * nh * T rows has lens[m / (nh * T)] keys (clamped into [1, T] by the kernel).
extern "C" int dyn_softmax_relshift_fwd_lens(const float* x, float* y, const float* bd, int64_t B, int64_t nh, int64_t T, int64_t ld_bd,
                                             const int32_t* lens, void* stream) {
    DYN_REQUIRE(x && y && bd && lens, DYN_E_ARG, "dyn_softmax_relshift_fwd_lens: null pointer");
    DYN_REQUIRE(B >= 0 && nh >= 1 && B * nh < (1ll << 31), DYN_E_ARG, "dyn_softmax_relshift_fwd_lens: bad sizes B=%lld nh=%lld", (long long)B,
                (long long)nh);
    if (int rc = check_scores("dyn_softmax_relshift_fwd_lens", B * nh, T, ld_bd)) return rc;
    DYN_REQUIRE((const void*)y != (const void*)bd, DYN_E_ARG, "dyn_softmax_relshift_fwd_lens: the output may alias the scores, not BD");
    if (B == 0) return DYN_OK;
    const int64_t rows = B * nh * T;
    const dim3 grid((unsigned)(rows < 65535 * 4 ? rows : 65535 * 4)), blk(TPB);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dyn::dispatch_items<dyn::MAX_ROW_FWD>("dyn_softmax_relshift_fwd_lens", T, [&](auto I) {
            hipLaunchKernelGGL((softmax_relshift_fwd_kernel<decltype(I)::value, true>), grid, blk, 0, st, x, y, bd, rows, (int)T, ld_bd, lens, nh * T);
        })) return rc;
    return dyn::check_launch("dyn_softmax_relshift_fwd_lens");
}

extern "C" int dyn_relshift_bwd(const float* dS, float* dBD, int64_t M, int64_t T, int64_t ld_bd, void* stream) {
    DYN_REQUIRE(dS && dBD, DYN_E_ARG, "dyn_relshift_bwd: null pointer");
    if (int rc = check_scores("dyn_relshift_bwd", M, T, ld_bd)) return rc;
    DYN_REQUIRE((const void*)dS != (const void*)dBD, DYN_E_ARG, "dyn_relshift_bwd: dBD may not alias dS");
    const int64_t rows = M * T;
    if (rows == 0) return DYN_OK;
    const int64_t g = rows < 65536 ? rows : 65536;
    hipLaunchKernelGGL(relshift_bwd_kernel, dim3((unsigned)g), dim3(TPB), 0, (hipStream_t)stream, dS, dBD, rows, (int)T, ld_bd);
    return dyn::check_launch("dyn_relshift_bwd");
}

extern "C" int dyn_head_bias_add(const float* q, int64_t ldq, const float* u, const float* v, float* qu, float* qv, int64_t rows, int64_t H,
                                 void* stream) {
    DYN_REQUIRE(q && u && v && qu && qv, DYN_E_ARG, "dyn_head_bias_add: null pointer");
    DYN_REQUIRE(rows >= 0 && H > 0 && H <= (1 << 24) && ldq >= H, DYN_E_ARG, "dyn_head_bias_add: bad sizes rows=%lld H=%lld ldq=%lld",
                (long long)rows, (long long)H, (long long)ldq);
    DYN_REQUIRE(H % 4 == 0 && ldq % 4 == 0, DYN_E_ARG, "dyn_head_bias_add: H=%lld and ldq=%lld must be multiples of 4", (long long)H,
                (long long)ldq);
    DYN_REQUIRE((((uintptr_t)q | (uintptr_t)u | (uintptr_t)v | (uintptr_t)qu | (uintptr_t)qv) & 15) == 0, DYN_E_ARG,
                "dyn_head_bias_add: operands must be 16-byte aligned");
    if (rows == 0) return DYN_OK;
    int64_t g = dyn::cdiv(rows * (H / 4), TPB);
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(head_bias_add_kernel, dim3((unsigned)g), dim3(TPB), 0, (hipStream_t)stream, q, ldq, u, v, qu, qv, rows, (int)(H / 4));
    return dyn::check_launch("dyn_head_bias_add");
}

extern "C" int64_t dyn_head_bias_bwd_workspace_bytes(int64_t rows, int64_t H) {
    if (rows < 0 || H <= 0) return 0;
    int64_t per;
    return 2 * hb_chunks(rows, &per) * H * (int64_t)sizeof(float);
}

extern "C" int dyn_head_bias_bwd(const float* dqu, const float* dqv, float* dq, int64_t ldq, float* du, float* dv, float beta, int64_t rows,
                                 int64_t H, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(dqu && dqv && dq && du && dv && workspace, DYN_E_ARG, "dyn_head_bias_bwd: null pointer");
    DYN_REQUIRE(rows >= 0 && H > 0 && H <= (1 << 24) && ldq >= H, DYN_E_ARG, "dyn_head_bias_bwd: bad sizes rows=%lld H=%lld ldq=%lld",
                (long long)rows, (long long)H, (long long)ldq);
    const int64_t need = dyn_head_bias_bwd_workspace_bytes(rows, H);
    DYN_REQUIRE(workspace_bytes >= need, DYN_E_WORKSPACE, "dyn_head_bias_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)need);
    int64_t per;
    const int64_t chunks = hb_chunks(rows, &per);
    hipStream_t st = (hipStream_t)stream;
    float* pu = dyn::partials_alloc(workspace, need);          // the workspace, or the open deferral context's arena
    float* pv = pu + chunks * H;
    // rows == 0: one workgroup per column tile writes a zero partial row, so du / dv still become beta * old
    hipLaunchKernelGGL(head_bias_bwd_kernel, dim3((unsigned)chunks, (unsigned)dyn::cdiv(H, TPB)), dim3(TPB), 0, st, dqu, dqv, dq, ldq, pu, pv, rows,
                       per, (int)H);
    if (int rc = dyn::check_launch("dyn_head_bias_bwd")) return rc;
    dyn::reduce_pair_or_defer(pu, du, pv, dv, chunks, H, beta, st);
    return dyn::check_launch("dyn_head_bias_bwd");
}
