// The row softmax and the ITEMS dispatch of every kernel that holds one row in registers: softmax.hip (plain rows), relbias.hip (WavLM's
// gated relative-position bias added while the row is read), relshift.hip (the Transformer-XL window added while the row is read).
// One 256-thread workgroup per row; thread t owns columns t, t + 256, ... (ITEMS of them, coalesced stride-256 accesses).  The kernels keep
// what is theirs (which rows a workgroup walks, what it stages in LDS, where a row starts) and hand softmax_row() the row as `load(c)`.
#pragma once
#include <type_traits>
#include "common.h"

namespace dyn {

constexpr int ROW_TPB = 256;            // threads per row; the instances are ITEMS = 1, 2, 4, ... columns per thread
constexpr int MAX_ROW_FWD = 16384;      // 64 items per thread: one value each in registers
constexpr int MAX_ROW_BWD = 8192;       // 32 items per thread: two values each (backward kernels)

// `valid` (device scalar, may be null): columns >= *valid are masked keys.  The row's valid length, clamped into [1, L].
__device__ __forceinline__ int valid_len(const int32_t* __restrict__ valid, int L) {
    int Lv = L;
    if (valid) { const int v = *valid; Lv = v < 1 ? 1 : (v < L ? v : L); }
    return Lv;
}

// The valid length of `row` when `valid` holds one count per batch entry and rows_per_len consecutive rows share one (a ragged batch).
__device__ __forceinline__ int valid_len_of_row(const int32_t* __restrict__ valid, int64_t row, int64_t rows_per_len, int L) {
    return valid_len(valid + row / rows_per_len, L);
}

// yr[0 .. L) = softmax (LOG: log-softmax) of load(0 .. Lv); columns in [Lv, L) are outside the max and the sum and written as 0 (-inf for
// LOG).  The row is read ONCE into registers, max and sum are wavefront + LDS reductions (`red`: the block_max / block_sum scratch), the
// result is written once.  The values of the first Lv columns are bit for bit those of a row of length Lv (same per-thread items, same
// reductions).  yr may alias what load() reads: every thread reads its columns before it writes them.
template <int ITEMS, bool LOG, class Load>
__device__ __forceinline__ void softmax_row(Load load, float* yr, int L, int Lv, float* red) {
    float v[ITEMS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int c = threadIdx.x + j * ROW_TPB;
        v[j] = c < Lv ? load(c) : -INFINITY;
        m = fmaxf(m, v[j]);
    }
    m = block_max(m, red);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int c = threadIdx.x + j * ROW_TPB;
        const float e = c < Lv ? __expf(v[j] - m) : 0.f;
        s += e;
        if (!LOG) v[j] = e;
    }
    s = block_sum(s, red);
    if (LOG) {
        const float lse = m + __logf(s);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int c = threadIdx.x + j * ROW_TPB;
            if (c < L) yr[c] = v[j] - lse;
        }
    } else {
        const float inv = 1.f / s;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int c = threadIdx.x + j * ROW_TPB;
            if (c < L) yr[c] = v[j] * inv;
        }
    }
}

template <int I, int MAX_ITEMS, class Go>
bool dispatch_items_from(int items, Go& go) {
    if (items <= I) { go(std::integral_constant<int, I>{}); return true; }
    if constexpr (2 * I <= MAX_ITEMS) return dispatch_items_from<2 * I, MAX_ITEMS>(items, go);
    return false;
}

// Host side: calls go(std::integral_constant<int, ITEMS>) with the smallest ITEMS in 1, 2, 4, ..., MAX_ROW / 256 that holds a row of L
// columns (`go` launches that instance); a longer row is refused.
template <int MAX_ROW, class Go>
int dispatch_items(const char* who, int64_t L, Go go) {
    static_assert(MAX_ROW % ROW_TPB == 0, "the row limit is a whole number of items");
    if (L <= MAX_ROW && dispatch_items_from<1, MAX_ROW / ROW_TPB>((int)cdiv(L, ROW_TPB), go)) return DYN_OK;
    set_error("%s: row length %lld > %d unsupported", who, (long long)L, MAX_ROW);
    return DYN_E_UNSUPPORTED;
}

}  // namespace dyn
