// Edit-distance counts on the MI355X — replaces the host-side integer dynamic programme behind every WER / CER of the package
// (`wer._align`; the reference computes them with `word_error_rate_detail`, lcasr/lib.py:1348-1349 inside calc_rewards and
// run_dynamic_eval_full.py:112-115 for the corpus WER).
//
// Lattice: cell (i, j) aligns the first i reference tokens with the first j hypothesis tokens and carries (cost, ins, del) as
// int32; sub = cost - ins - del.  Row 0 is (j, j, 0), column 0 is (i, 0, i).  Cell rule, which IS `_align`'s tie rule
// (substitution / match first, then deletion, then insertion, the fewest insertions among insertion chains):
//     diag = (i-1, j-1) + [hyp[j-1] != ref[i-1]],  up = (i-1, j) + 1 (a deletion),  left = (i, j-1) + 1 (an insertion)
//     take diag if diag <= up, else up; keep that unless left is STRICTLY smaller.
//
// MI355X mapping: one workgroup walks the anti-diagonals of a block of the lattice; the three live diagonals of (cost, ins, del)
// and both token strings sit in LDS, a thread owns one cell of the diagonal's active range, one barrier per diagonal (as
// softdtw.hip).  Two regimes share that block scan:
//   resident  one workgroup per pair, the block is the whole lattice and its boundaries are row 0 / column 0;
//   tiled     the lattice is cut into tile x tile blocks; the bottom row and right column of every block go to the workspace
//             (each location is written exactly once) and one launch covers one block anti-diagonal of up to GROUP pairs.  Blocks
//             of a launch are independent; block-to-block progress is the launch order of the stream.  No workgroup waits on another.
#include "common.h"

namespace {

constexpr int64_t LDS_BUDGET = 160 * 1024 - 1024;
constexpr int DEFAULT_TILE = 1024, MIN_TILE = 8, MAX_TILE = 2048;
constexpr int GROUP = 16;                  // tiled pairs whose block diagonals share a launch (they travel as kernel arguments)
constexpr int64_t MAX_LEN = (1 << 30) - 1;  // cost <= n + m stays an int32
// resident LDS: 3 diagonals x 3 fields over the hypothesis positions (36 m bytes) + both token strings (4 m + 4 n bytes)
constexpr int64_t RESIDENT_LIMIT = LDS_BUDGET / 44;
// tiled LDS adds the staged top row and left column: 36 T + 8 T + 2 * 12 (T + 1)
static_assert(68 * (int64_t)MAX_TILE + 24 <= LDS_BUDGET, "MAX_TILE exceeds the LDS");

struct Cell {
    int c, i, d;  // cost, insertions, deletions
};

struct Block {
    const int32_t* hyp;   // tokens of columns j0 + 1 .. j0 + w
    const int32_t* ref;   // tokens of rows i0 + 1 .. i0 + h
    int i0, j0, h, w, n;  // origin, extent, reference length of the pair
    const int32_t* top;   // cells (i0, j0 + jj), jj = 0..w, as [3][ldt]; nullptr: row 0
    const int32_t* left;  // cells (i0 + ii, j0), ii = 0..h, as [3][ldl]; nullptr: column 0
    int32_t* bottom;      // cells (i0 + h, j0 + jj), jj = 1..w, same layout as top; nullptr: not needed
    int32_t* right;       // cells (i0 + ii, j0 + w), ii = 1..h, same layout as left; nullptr: not needed
    int64_t ldt, ldl;
    int32_t* counts;      // (ins, del, sub, n) of the pair when this block holds cell (n, m), else nullptr
};

// lds: 9 w (diagonals) + w + h (tokens) [+ 3 (w + 1) when b.top] [+ 3 (h + 1) when b.left] int32 words.  h, w >= 1.
__device__ void scan_block(const Block& b, int32_t* lds) {
    const int h = b.h, w = b.w, tid = threadIdx.x, nt = blockDim.x;
    int32_t* th = lds + 9 * w;
    int32_t* tr = th + w;
    int32_t* tp = tr + h;
    int32_t* lf = tp + (b.top ? 3 * (w + 1) : 0);
    for (int x = tid; x < w; x += nt) th[x] = b.hyp[x];
    for (int y = tid; y < h; y += nt) tr[y] = b.ref[y];
    if (b.top)
        for (int f = 0; f < 3; ++f)
            for (int x = tid; x <= w; x += nt) tp[f * (w + 1) + x] = b.top[f * b.ldt + x];
    if (b.left)
        for (int f = 0; f < 3; ++f)
            for (int y = tid; y <= h; y += nt) lf[f * (h + 1) + y] = b.left[f * b.ldl + y];
    __syncthreads();
    if (b.top && !b.left && tid == 0) {  // the corner (i0, 0) lies on column 0, which no block stores
        tp[0] = b.i0; tp[w + 1] = 0; tp[2 * (w + 1)] = b.i0;
    }
    __syncthreads();
    auto top_cell = [&](int jj) -> Cell {
        if (b.top) return Cell{tp[jj], tp[w + 1 + jj], tp[2 * (w + 1) + jj]};
        return Cell{b.j0 + jj, b.j0 + jj, 0};
    };
    auto left_cell = [&](int ii) -> Cell {
        if (b.left) return Cell{lf[ii], lf[h + 1 + ii], lf[2 * (h + 1) + ii]};
        return Cell{b.i0 + ii, 0, b.i0 + ii};
    };
    // cell (ii, jj) of diagonal q = ii + jj lives at [jj - 1] of that diagonal's buffer
    int32_t* d2 = lds;
    int32_t* d1 = lds + 3 * w;
    int32_t* d0 = lds + 6 * w;
    for (int q = 2; q <= h + w; ++q) {
        const int lo = max(1, q - h), hi = min(w, q - 1);
        for (int jj = lo + tid; jj <= hi; jj += nt) {
            const int ii = q - jj;
            Cell dg, up, lt;
            if (ii == 1) {
                dg = top_cell(jj - 1);
                up = top_cell(jj);
            } else {
                dg = (jj == 1) ? left_cell(ii - 1) : Cell{d2[jj - 2], d2[w + jj - 2], d2[2 * w + jj - 2]};
                up = Cell{d1[jj - 1], d1[w + jj - 1], d1[2 * w + jj - 1]};
            }
            lt = (jj == 1) ? left_cell(ii) : Cell{d1[jj - 2], d1[w + jj - 2], d1[2 * w + jj - 2]};
            const int dgc = dg.c + (th[jj - 1] != tr[ii - 1] ? 1 : 0), upc = up.c + 1;
            Cell v = (dgc <= upc) ? Cell{dgc, dg.i, dg.d} : Cell{upc, up.i, up.d + 1};
            if (lt.c + 1 < v.c) v = Cell{lt.c + 1, lt.i + 1, lt.d};
            d0[jj - 1] = v.c; d0[w + jj - 1] = v.i; d0[2 * w + jj - 1] = v.d;
            if (ii == h && b.bottom) {
                b.bottom[jj] = v.c; b.bottom[b.ldt + jj] = v.i; b.bottom[2 * b.ldt + jj] = v.d;
            }
            if (jj == w && b.right) {
                b.right[ii] = v.c; b.right[b.ldl + ii] = v.i; b.right[2 * b.ldl + ii] = v.d;
            }
            if (ii == h && jj == w && b.counts) {
                b.counts[0] = v.i; b.counts[1] = v.d; b.counts[2] = v.c - v.i - v.d; b.counts[3] = b.n;
            }
        }
        __syncthreads();
        int32_t* t = d2; d2 = d1; d1 = d0; d0 = t;
    }
}

// off: device copy of the offsets, hyp_off [P + 1] then ref_off [P + 1].  Pairs with a side above `limit` belong to the tiled regime.
__global__ __launch_bounds__(1024) void edit_resident_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ ref,
                                                              const int64_t* __restrict__ off, int32_t* __restrict__ counts, int64_t P,
                                                              int limit) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int64_t p = blockIdx.x;
    const int64_t h0 = off[p], r0 = off[P + 1 + p];
    const int64_t m = off[p + 1] - h0, n = off[P + 2 + p] - r0;
    if (n == 0 || m == 0) {  // `_align`: an empty reference gives (m, 0, 0), an empty hypothesis (0, n, 0)
        if (threadIdx.x == 0) {
            int32_t* c = counts + 4 * p;
            c[0] = (int32_t)(n == 0 ? m : 0); c[1] = (int32_t)(n == 0 ? 0 : n); c[2] = 0; c[3] = (int32_t)n;
        }
        return;
    }
    if (m > limit || n > limit) return;
    Block b;
    b.hyp = hyp + h0; b.ref = ref + r0;
    b.i0 = 0; b.j0 = 0; b.h = (int)n; b.w = (int)m; b.n = (int)n;
    b.top = nullptr; b.left = nullptr; b.bottom = nullptr; b.right = nullptr; b.ldt = 0; b.ldl = 0;
    b.counts = counts + 4 * p;
    scan_block(b, lds);
}

struct TiledPair {
    int64_t hyp_off, ref_off, ws_off;  // ws_off in int32 words
    int32_t n, m, pair, pad_;
};
struct TiledGroup {
    TiledPair pr[GROUP];
};

// a pair with an empty side is answered by the resident kernel whatever the other side's length
inline bool is_tiled(int64_t n, int64_t m, int limit) { return n > 0 && m > 0 && (m > limit || n > limit); }

inline int64_t tiled_words(int64_t n, int64_t m, int64_t tile) {
    const int64_t nbi = (n + tile - 1) / tile, nbj = (m + tile - 1) / tile;
    return 3 * ((nbi - 1) * (m + 1) + (nbj - 1) * (n + 1));
}

// Block anti-diagonal d of every pair of the group: grid (blocks on the longest diagonal, pairs).
// Workspace of a pair: H [nbi - 1][3][m + 1] (rows tile, 2 tile, ...) then V [nbj - 1][3][n + 1] (columns tile, 2 tile, ...).
__global__ __launch_bounds__(1024) void edit_tiled_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ ref,
                                                           const TiledGroup g, int32_t* __restrict__ ws, int32_t* __restrict__ counts,
                                                           int tile, int d) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const TiledPair t = g.pr[blockIdx.y];
    const int nbi = (t.n + tile - 1) / tile, nbj = (t.m + tile - 1) / tile;
    const int bi = max(0, d - (nbj - 1)) + (int)blockIdx.x;
    if (bi > min(nbi - 1, d)) return;
    const int bj = d - bi;
    const int64_t ldt = (int64_t)t.m + 1, ldl = (int64_t)t.n + 1;
    int32_t* H = ws + t.ws_off;
    int32_t* V = H + (int64_t)(nbi - 1) * 3 * ldt;
    Block b;
    b.i0 = bi * tile; b.j0 = bj * tile;
    b.h = min(tile, t.n - b.i0); b.w = min(tile, t.m - b.j0); b.n = t.n;
    b.hyp = hyp + t.hyp_off + b.j0; b.ref = ref + t.ref_off + b.i0;
    b.ldt = ldt; b.ldl = ldl;
    b.top = bi ? H + (int64_t)(bi - 1) * 3 * ldt + b.j0 : nullptr;
    b.bottom = bi + 1 < nbi ? H + (int64_t)bi * 3 * ldt + b.j0 : nullptr;
    b.left = bj ? V + (int64_t)(bj - 1) * 3 * ldl + b.i0 : nullptr;
    b.right = bj + 1 < nbj ? V + (int64_t)bj * 3 * ldl + b.i0 : nullptr;
    b.counts = (bi == nbi - 1 && bj == nbj - 1) ? counts + 4 * (int64_t)t.pair : nullptr;
    scan_block(b, lds);
}

inline int scan_threads(int64_t n) {
    int64_t t = (n + 63) / 64 * 64;
    return (int)(t > 1024 ? 1024 : t < 64 ? 64 : t);
}

// Checks the host offsets and the tile; on success *T is the tile and *limit the largest side of a resident pair.
int plan(const char* who, const int64_t* hyp_off, const int64_t* ref_off, int64_t P, int64_t tile, int* T, int* limit) {
    DYN_REQUIRE(hyp_off && ref_off && P >= 0 && P < ((int64_t)1 << 31), DYN_E_ARG, "%s: bad arguments", who);
    DYN_REQUIRE(tile == 0 || (tile >= MIN_TILE && tile <= MAX_TILE), DYN_E_ARG, "%s: tile %lld outside [%d, %d]", who, (long long)tile,
                MIN_TILE, MAX_TILE);
    DYN_REQUIRE(hyp_off[0] >= 0 && ref_off[0] >= 0, DYN_E_ARG, "%s: negative offset", who);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t m = hyp_off[p + 1] - hyp_off[p], n = ref_off[p + 1] - ref_off[p];
        DYN_REQUIRE(m >= 0 && n >= 0 && m <= MAX_LEN && n <= MAX_LEN, DYN_E_ARG, "%s: pair %lld has lengths %lld, %lld", who, (long long)p,
                    (long long)m, (long long)n);
    }
    // an explicit tile is the test / tuning knob: every pair with a side of at least one tile then takes the tiled regime
    *T = tile ? (int)tile : DEFAULT_TILE;
    *limit = tile ? (int)(tile - 1 < RESIDENT_LIMIT ? tile - 1 : RESIDENT_LIMIT) : (int)RESIDENT_LIMIT;
    return DYN_OK;
}

}  // namespace

extern "C" int64_t dyn_edit_counts_resident_limit(void) { return RESIDENT_LIMIT; }

extern "C" int64_t dyn_edit_counts_workspace_bytes(const int64_t* hyp_off, const int64_t* ref_off, int64_t P, int64_t tile) {
    int T, limit;
    const int rc = plan("dyn_edit_counts_workspace_bytes", hyp_off, ref_off, P, tile, &T, &limit);
    if (rc != DYN_OK) return rc;
    int64_t words = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t m = hyp_off[p + 1] - hyp_off[p], n = ref_off[p + 1] - ref_off[p];
        if (is_tiled(n, m, limit)) words += tiled_words(n, m, T);
    }
    return words * (int64_t)sizeof(int32_t);
}

extern "C" int dyn_edit_counts(const int32_t* hyp, const int32_t* ref, const int64_t* hyp_off, const int64_t* ref_off,
                               const int64_t* dev_off, int32_t* counts, void* ws, int64_t ws_bytes, int64_t P, int64_t tile,
                               void* stream) {
    int T, limit;
    const int rc = plan("dyn_edit_counts", hyp_off, ref_off, P, tile, &T, &limit);
    if (rc != DYN_OK) return rc;
    if (P == 0) return DYN_OK;
    DYN_REQUIRE(hyp && ref && dev_off && counts, DYN_E_ARG, "dyn_edit_counts: null pointer");
    int64_t words = 0, res_lds = 0, res_span = 0, n_tiled = 0;
    bool any_resident = false;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t m = hyp_off[p + 1] - hyp_off[p], n = ref_off[p + 1] - ref_off[p];
        if (is_tiled(n, m, limit)) {
            words += tiled_words(n, m, T);
            ++n_tiled;
        } else {
            any_resident = true;
            if (n == 0 || m == 0) continue;
            if (10 * m + n > res_lds) res_lds = 10 * m + n;
            if ((m < n ? m : n) > res_span) res_span = m < n ? m : n;
        }
    }
    DYN_REQUIRE(words == 0 || (ws && ws_bytes >= words * (int64_t)sizeof(int32_t)), DYN_E_WORKSPACE,
                "dyn_edit_counts: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)(words * 4));
    hipStream_t st = (hipStream_t)stream;
    if (any_resident) {
        const size_t shm = (size_t)res_lds * sizeof(int32_t);
        if (shm > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)edit_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        hipLaunchKernelGGL(edit_resident_kernel, dim3((unsigned)P), dim3(scan_threads(res_span)), shm, st, hyp, ref, dev_off, counts, P,
                           limit);
        const int lrc = dyn::check_launch("dyn_edit_counts (resident)");
        if (lrc != DYN_OK) return lrc;
    }
    if (n_tiled == 0) return DYN_OK;
    const size_t shm = (size_t)(68 * (int64_t)T + 24);
    if (shm > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)edit_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    TiledGroup g;
    int cnt = 0, diags = 0, width = 0;
    int64_t ws_off = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t m = hyp_off[p + 1] - hyp_off[p], n = ref_off[p + 1] - ref_off[p];
        if (is_tiled(n, m, limit)) {
            g.pr[cnt++] = TiledPair{hyp_off[p], ref_off[p], ws_off, (int32_t)n, (int32_t)m, (int32_t)p, 0};
            ws_off += tiled_words(n, m, T);
            const int nbi = (int)dyn::cdiv(n, T), nbj = (int)dyn::cdiv(m, T);
            if (nbi + nbj - 1 > diags) diags = nbi + nbj - 1;
            if ((nbi < nbj ? nbi : nbj) > width) width = nbi < nbj ? nbi : nbj;
        }
        if (cnt == GROUP || (p == P - 1 && cnt > 0)) {
            for (int i = cnt; i < GROUP; ++i) g.pr[i] = g.pr[0];  // never indexed (grid.y = cnt); keeps the argument defined
            for (int d = 0; d < diags; ++d) {
                hipLaunchKernelGGL(edit_tiled_kernel, dim3((unsigned)width, (unsigned)cnt), dim3(scan_threads(T)), shm, st, hyp, ref, g,
                                   (int32_t*)ws, counts, T, d);
                const int lrc = dyn::check_launch("dyn_edit_counts (tiled)");
                if (lrc != DYN_OK) return lrc;
            }
            cnt = 0; diags = 0; width = 0;
        }
    }
    return DYN_OK;
}
