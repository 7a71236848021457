// The LayerNorm of a row that one wave64 holds in registers, for every kernel that normalises over NV * 256 channels: norm.hip,
// bias_ln_gelu.hip, posconv_ln_gelu.hip, squeeze.hip, attn_adapter.hip and the prologues of decoder_step.hip.  Lane l owns the float4s
// l, l + 64, ... (NV of them, 16-B accesses); mean, variance and the two gradient dot-products are wavefront reductions (no LDS, no barrier).
// The backward kernels add their column sums (weight gradients) per lane over the rows of a workgroup, combine_waves() adds the waves of the
// workgroup in wave order and writes ONE partial row, and the fixed-order reducers (reduce.h; deferrable) sum the partial rows: no atomics,
// bit-reproducible.  The kernels keep what is theirs (which rows a workgroup walks, where a row's elements live, what is added before or
// applied after the norm, which column sums they keep) and hand the row over as `float4 (&)[NV]`: by reference into force-inlined
// functions, so the arrays stay in registers.  A file that switches floating-point contraction off includes this header after the pragma.
#pragma once
#include <type_traits>
#include "common.h"

namespace dyn {

constexpr int ROW_WPB = 4;   // waves (rows in flight) per workgroup of every kernel here

// float4 number i counted from the 16-byte aligned p
__device__ __forceinline__ float4 ld4(const float* p, int i = 0) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ void st4(float* p, float4 v, int i = 0) { reinterpret_cast<float4*>(p)[i] = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// Componentwise one-liners.  A kernel uses them where its register count stays at the parent's: the compiler schedules four components
// of one step differently from four steps of one component, which cost bias_ln_gelu's backward 2 - 3 VGPRs at NV >= 2 and squeeze's
// backward sits one register below an occupancy step, so those bodies (and the adapter's, at the 256-register limit) spell the lines out.
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ void add4(float4& a, float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void addmul4(float4& a, float4 b, float4 c) { a.x += b.x * c.x; a.y += b.y * c.y; a.z += b.z * c.z; a.w += b.w * c.w; }
// (v - mean) * rstd, and the same * gamma + beta
__device__ __forceinline__ float4 xhat4(float4 v, float mean, float rstd) {
    return make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
}
__device__ __forceinline__ float4 affine4(float4 v, float mean, float rstd, float4 g, float4 b) {
    return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y, (v.z - mean) * rstd * g.z + b.z,
                       (v.w - mean) * rstd * g.w + b.w);
}

// Mean and 1 / sqrt(variance + eps) of the row v: the centred two-reduction form (the variance is the mean of (v - mean)^2, never
// E[v^2] - mean^2, which cancels for a row far from zero).
// `s`: this lane's sum of its elements, for a kernel that adds them up (in j order) while it puts the row together.
template <int NV>
__device__ __forceinline__ void row_mean_rstd(const float4 (&v)[NV], float s, float eps, float& mean, float& rstd) {
    constexpr int C = NV * 256;
    mean = wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
        q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
    }
    rstd = rsqrtf(wave_sum(q) / C + eps);
}
template <int NV>
__device__ __forceinline__ void row_mean_rstd(const float4 (&v)[NV], float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) s += v[j].x + v[j].y + v[j].z + v[j].w;
    row_mean_rstd(v, s, eps, mean, rstd);
}

// LayerNorm backward of a row, gy = dy * gamma, xh = (x - mean) * rstd: dx = rstd * (gy - s1 - xh * s2) with the row means s1 = mean(gy),
// s2 = mean(gy * xh).  RMS (RMSNorm: nothing was subtracted in the forward) has s1 = 0.  In three pieces, so that a kernel adds up, uses
// and stores each float4 as it makes it: bwd_lane_sums() adds one float4 to this lane's s1 and s2 (both start at 0, j ascending),
// bwd_row_means() turns the lane sums into the row means, bwd4() is the expression for one float4.
__device__ __forceinline__ void bwd_lane_sums(float4 gy, float4 xh, float& s1, float& s2) {
    s1 += gy.x + gy.y + gy.z + gy.w;
    s2 += gy.x * xh.x + gy.y * xh.y + gy.z * xh.z + gy.w * xh.w;
}
template <int NV, bool RMS = false>
__device__ __forceinline__ void bwd_row_means(float& s1, float& s2) {
    constexpr int C = NV * 256;
    s1 = RMS ? 0.f : wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
}
__device__ __forceinline__ float4 bwd4(float4 gy, float4 xh, float rstd, float s1, float s2) {
    float4 o;
    o.x = rstd * (gy.x - s1 - xh.x * s2);
    o.y = rstd * (gy.y - s1 - xh.y * s2);
    o.z = rstd * (gy.z - s1 - xh.z * s2);
    o.w = rstd * (gy.w - s1 - xh.w * s2);
    return o;
}

// The workgroup's column sum: acc of its WPB waves added in wave order through `red`, written as the partial row dst_row[0 .. NV * 256).
// Every thread of the workgroup calls it (two barriers per float4).
template <int NV, int WPB>
__device__ __forceinline__ void combine_waves(const float4 (&acc)[NV], float4 (&red)[WPB][64], float* dst_row) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        __syncthreads();
        red[w][lane] = acc[j];
        __syncthreads();
        if (w == 0) {
            float4 t = red[0][lane];
#pragma unroll
            for (int k = 1; k < WPB; ++k) { t.x += red[k][lane].x; t.y += red[k][lane].y; t.z += red[k][lane].z; t.w += red[k][lane].w; }
            st4(dst_row + 4 * (lane + 64 * j), t);
        }
    }
}

// Host side.  Workgroups for `rows` rows at `wpb` rows in flight each, 1 <= result <= cap.  For a backward kernel the result is the number
// of partial rows, so its cap fixes the summation order of the weight gradients: every file passes its own.  The lower clamp is for that
// count (a workspace size is asked for rows = 0 too); a forward grid never meets it, the entries return before the launch when rows = 0.
inline int row_blocks(int64_t rows, int wpb, int cap) {
    const int64_t g = cdiv(rows, wpb);
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Calls go(std::integral_constant<int, NV>) for NV = C / 256 when that instance is one of the built NVS... (`go` launches it); false otherwise.
template <int... NVS, class Go>
bool dispatch_nv(int64_t C, Go go) {
    return ((C == 256 * NVS ? (go(std::integral_constant<int, NVS>{}), true) : false) || ...);
}

}  // namespace dyn
