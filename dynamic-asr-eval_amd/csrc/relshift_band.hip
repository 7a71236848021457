// Chunked limited-context attention of NemotronAsrStreamingForRNNT (transformers modeling_nemotron_asr_streaming.py,
// chunked_limited_mask_function + NemotronAsrStreamingEncoderAttention.forward): the Transformer-XL score of relshift.hip under the mask
//   query i sees key j  iff  0 <= i / cs - j / cs <= lc          (cs = lookahead + 1 frames per chunk, lc left chunks; lc < 0: unlimited)
// Row i's keys are the contiguous range [j0, j1) = [max(0, i / cs - lc) * cs, min(T, (i / cs + 1) * cs)), never empty, and j - i lies in
// [-dlo, dhi] with dlo = min(lc * cs + cs - 1, T - 1), dhi = min(cs - 1, T - 1): W = dlo + dhi + 1 relative positions whatever T is.
// So the position term is a BAND buffer BDb [B, nh, T, ld >= W] = (q + v) P_h[r0 .. r0 + W)^T over the W rows r0 = T - 1 - dlo .. of the
// projected position table that any row can touch (one GEMM with N = W), and
//   score[i, j] = S[i, j] + BDb[i, j - i + dlo]                   column origin: relative position -dlo is column 0
// a closed form of (i, j): the row's window starts one column earlier per row inside its chunk and jumps back at a chunk boundary.
// Nothing is copied for the shift in either direction.
//   forward   reads S and BDb over [j0, j1) only, writes the softmax there and exact zeros in every other column of the row (so the
//             context product, softmax_bwd and the score-gradient products of the dense path stay correct, unchanged).
//   backward  writes dS[i, j0 .. j1) into BDb's layout and zeros in every other column of the ld-float row (reused scratch).
// Row layout of relshift.hip: one workgroup per row, stride-256 item loop.  Bandwidth work, 4-byte accesses (the window is unaligned).
#include "softmax_row.h"

namespace {

constexpr int TPB = dyn::ROW_TPB;

// The row's key range; cs in [1, T], lc < 0 or in [0, T] (the entries clamp both: no product here leaves int).
__device__ __forceinline__ void key_range(int i, int T, int cs, int lc, int& j0, int& j1) {
    const int q = i / cs;
    j0 = (lc < 0 || q <= lc) ? 0 : (q - lc) * cs;
    const int e = (q + 1) * cs;                                // <= T + cs - 1 <= 2T
    j1 = e < T ? e : T;
}

template <int ITEMS>
__global__ __launch_bounds__(TPB) void softmax_relshift_band_fwd_kernel(const float* x, float* y, const float* __restrict__ bd, int64_t rows,
                                                                         int T, int64_t ld, int cs, int lc, int dlo) {   // y may alias x
    __shared__ float red[16];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row % T);
        int j0, j1;
        key_range(i, T, cs, lc, j0, j1);
        const float* xr = x + row * T + j0;
        const float* br = bd + row * ld + (j0 - i + dlo);      // columns j0 - i + dlo .. j1 - 1 - i + dlo, inside [0, W)
        float* yr = y + row * T;
        const int n = j1 - j0;
        dyn::softmax_row<ITEMS, false>([=](int c) { return xr[c] + br[c]; }, yr + j0, n, n, red);
        for (int c = threadIdx.x; c < j0; c += TPB) yr[c] = 0.f;       // outside the range nobody reads this row: x may be y
        for (int c = j1 + threadIdx.x; c < T; c += TPB) yr[c] = 0.f;
    }
}

// dBDb[m, i, k] = dS[m, i, k - dlo + i] for k - dlo + i in [j0, j1), 0 written in every other column of the ld-float row.
__global__ __launch_bounds__(TPB) void relshift_band_bwd_kernel(const float* __restrict__ dS, float* __restrict__ dBD, int64_t rows, int T,
                                                                 int64_t ld, int cs, int lc, int dlo) {
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row % T);
        int j0, j1;
        key_range(i, T, cs, lc, j0, j1);
        const float* gr = dS + row * T + j0;
        float* o = dBD + row * ld;
        const int lo = j0 - i + dlo, n = j1 - j0;
        for (int64_t k = threadIdx.x; k < ld; k += TPB) {
            const int64_t c = k - lo;
            o[k] = (c >= 0 && c < n) ? gr[c] : 0.f;
        }
    }
}

struct Band { int cs, lc, dlo; int64_t W, keys; };

// (cs, lc) as given -> clamped into the kernels' range with the same mask: cs >= T is one chunk, lc >= T chunks is every chunk.
int band_of(const char* who, int64_t M, int64_t T, int64_t ld, int64_t cs, int64_t lc, Band* b) {
    DYN_REQUIRE(M >= 0 && T >= 1, DYN_E_ARG, "%s: bad sizes rows=%lld T=%lld", who, (long long)M, (long long)T);
    DYN_REQUIRE(T <= dyn::MAX_ROW_FWD, DYN_E_ARG, "%s: row length %lld > %d unsupported", who, (long long)T, dyn::MAX_ROW_FWD);
    DYN_REQUIRE(cs >= 1, DYN_E_ARG, "%s: chunk size %lld must be positive (lookahead + 1)", who, (long long)cs);
    if (cs > T) cs = T;
    if (lc > T) lc = T;
    const int64_t left = lc < 0 ? T - 1 : lc * cs + cs - 1;    // <= T * T + T
    b->cs = (int)cs;
    b->lc = lc < 0 ? -1 : (int)lc;
    b->dlo = (int)(left < T - 1 ? left : T - 1);
    b->W = b->dlo + (cs - 1 < T - 1 ? cs - 1 : T - 1) + 1;
    const int64_t k = lc < 0 ? T : (lc + 1) * cs;
    b->keys = k < T ? k : T;
    DYN_REQUIRE(ld >= b->W, DYN_E_ARG, "%s: ld_bd=%lld is shorter than the band of %lld relative positions", who, (long long)ld, (long long)b->W);
    DYN_REQUIRE(ld <= (1 << 20) && M * T <= (1ll << 40), DYN_E_ARG, "%s: too many rows for one launch", who);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_softmax_relshift_band_fwd(const float* x, float* y, const float* bd, int64_t M, int64_t T, int64_t ld_bd, int64_t cs,
                                             int64_t lc, void* stream) {
    DYN_REQUIRE(x && y && bd, DYN_E_ARG, "dyn_softmax_relshift_band_fwd: null pointer");
    Band b;
    if (int rc = band_of("dyn_softmax_relshift_band_fwd", M, T, ld_bd, cs, lc, &b)) return rc;
    DYN_REQUIRE((const void*)y != (const void*)bd, DYN_E_ARG, "dyn_softmax_relshift_band_fwd: the output may alias the scores, not the band");
    if (M == 0) return DYN_OK;
    const int64_t rows = M * T;
    const dim3 grid((unsigned)(rows < 65535 * 4 ? rows : 65535 * 4)), blk(TPB);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dyn::dispatch_items<dyn::MAX_ROW_FWD>("dyn_softmax_relshift_band_fwd", b.keys, [&](auto I) {
            hipLaunchKernelGGL((softmax_relshift_band_fwd_kernel<decltype(I)::value>), grid, blk, 0, st, x, y, bd, rows, (int)T, ld_bd, b.cs, b.lc,
                               b.dlo);
        })) return rc;
    return dyn::check_launch("dyn_softmax_relshift_band_fwd");
}

extern "C" int dyn_relshift_band_bwd(const float* dS, float* dBD, int64_t M, int64_t T, int64_t ld_bd, int64_t cs, int64_t lc, void* stream) {
    DYN_REQUIRE(dS && dBD, DYN_E_ARG, "dyn_relshift_band_bwd: null pointer");
    Band b;
    if (int rc = band_of("dyn_relshift_band_bwd", M, T, ld_bd, cs, lc, &b)) return rc;
    DYN_REQUIRE((const void*)dS != (const void*)dBD, DYN_E_ARG, "dyn_relshift_band_bwd: dBD may not alias dS");
    const int64_t rows = M * T;
    if (rows == 0) return DYN_OK;
    const int64_t g = rows < 65536 ? rows : 65536;
    hipLaunchKernelGGL(relshift_band_bwd_kernel, dim3((unsigned)g), dim3(TPB), 0, (hipStream_t)stream, dS, dBD, rows, (int)T, ld_bd, b.cs, b.lc,
                       b.dlo);
    return dyn::check_launch("dyn_relshift_band_bwd");
}
