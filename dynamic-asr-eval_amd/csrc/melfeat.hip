// Waveform front end of the FastConformer family on the device: what transformers' ParakeetFeatureExtractor, NemotronAsrStreamingFeatureExtractor,
// CohereAsrFeatureExtractor and LasrFeatureExtractor compute on the CPU (feature_extraction_parakeet.py / _nemotron_asr_streaming.py /
// _cohere_asr.py / _lasr.py, `__call__` and `_torch_extract_fbank_features`), for a ragged batch [B, Lmax] with one sample count per row.
//
// MI355X mapping: the STFT stays the ONE strided-row fp32-MFMA GEMM of logmel.hip (frame t = row t of the padded signal at lda = hop = 160, the
// Hann window and the window's offset inside the 512-point frame folded into the basis), followed by dyn_stft_power and the mel GEMM.  Unlike
// Kaldi's per-frame pre-emphasis (fbank.hip: folded into the basis), the extractors here pre-emphasise the WHOLE signal before framing and
// then zero every sample at or past the row's length, sample L included (`masked_fill(~timemask, 0.0)`: 0, not -0.97 x[L-1]) — a frame that
// straddles the row's end sees that zero, so the filter cannot live in the basis.  This file holds the two HBM-bound ends:
//   dyn_melfeat_prep     one pass: dither, pre-emphasis, the length mask and the zero padding of `center=True`, every output element written
//   dyn_melfeat_finish   log (guard added, or clamped at a floor), per-row per-bin (mean, unbiased std) over the row's valid frames,
//                        (x - mean) / (std + eps), exact zeros past the valid count, in [B, T, F] or [B, F, T]
// The statistics follow logmel.hip: a pivoted sum per 256-frame block, the mean in double in a fixed order, a second CENTRED pass for the
// squares, no float atomics — a bin at the log guard with a spread of 1e-3 keeps its std, a constant bin has mean == value and gives zeros.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int ROWS = 256;                       // frames per moment block

// out[b, i], i in [0, W): sample j = i - pad of row b after dither, pre-emphasis and the length mask; zero outside [0, len_b).
// The float operations are the extractor's, one rounding each (no fused multiply-add): x + dither * noise, then x[j] - pre * x[j - 1].
__global__ __launch_bounds__(TPB) void prep_kernel(const float* __restrict__ x, float* __restrict__ out, const int32_t* __restrict__ lens,
                                                   const float* __restrict__ noise, const float* __restrict__ prev, int64_t Lmax, int64_t pad,
                                                   int64_t W, float pre, float dither) {
    const int64_t b = blockIdx.y;
    const int64_t L = dyn::valid_rows(lens, b, Lmax);
    const float* xb = x + b * Lmax;
    const float* nb = noise ? noise + b * Lmax : nullptr;
    float* ob = out + b * W;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < W; i += (int64_t)gridDim.x * TPB) {
        const int64_t j = i - pad;
        float v = 0.f;
        if (j >= 0 && j < L) {
            v = xb[j];
            if (nb) v = __fadd_rn(v, __fmul_rn(dither, nb[j]));
            if (pre != 0.f) {
                if (j > 0) {
                    float p = xb[j - 1];
                    if (nb) p = __fadd_rn(p, __fmul_rn(dither, nb[j - 1]));
                    v = __fsub_rn(v, __fmul_rn(pre, p));
                } else if (prev) {
                    v = __fsub_rn(v, __fmul_rn(pre, prev[b]));
                }
            }
        }
        ob[i] = v;
    }
}

__device__ __forceinline__ float log_rule(float m, float guard, int clamp) { return clamp ? logf(fmaxf(m, guard)) : logf(m + guard); }

// partial [b, block, 2F] = per bin (pivot, sum of v - pivot) over the block's valid frames; an empty block writes zeros
__global__ __launch_bounds__(TPB) void pivot_sum_kernel(const float* __restrict__ mel, float* __restrict__ partial, const int32_t* __restrict__ lens,
                                                        int64_t T, int F, float guard, int clamp) {
    __shared__ float red[TPB];
    const int64_t b = blockIdx.y, nb = gridDim.x;
    const int64_t Tv = dyn::valid_rows(lens, b, T);
    const float* m = mel + b * T * F;
    const int f = threadIdx.x % F, lane_r = threadIdx.x / F, rl = TPB / F;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS;
    const int64_t r1 = (r0 + ROWS < Tv) ? r0 + ROWS : Tv;
    const float p = r0 < r1 ? log_rule(m[r0 * F + f], guard, clamp) : 0.f;
    float s = 0.f;
    if (lane_r < rl)
        for (int64_t t = r0 + lane_r; t < r1; t += rl) s += log_rule(m[t * F + f], guard, clamp) - p;
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < F) {
        float ts = 0.f;
        for (int k = 0; k < rl; ++k) ts += red[k * F + threadIdx.x];
        float* dst = partial + (b * nb + blockIdx.x) * 2 * F;
        dst[threadIdx.x] = p;
        dst[F + threadIdx.x] = ts;
    }
}

// partial [b, block, 2F], first F = per bin sum of (v - mean)^2 over the block's valid frames
__global__ __launch_bounds__(TPB) void centred_sq_kernel(const float* __restrict__ mel, const double* __restrict__ stats, float* __restrict__ partial,
                                                         const int32_t* __restrict__ lens, int64_t T, int F, float guard, int clamp) {
    __shared__ float red[TPB];
    const int64_t b = blockIdx.y, nb = gridDim.x;
    const int64_t Tv = dyn::valid_rows(lens, b, T);
    const float* m = mel + b * T * F;
    const int f = threadIdx.x % F, lane_r = threadIdx.x / F, rl = TPB / F;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS;
    const int64_t r1 = (r0 + ROWS < Tv) ? r0 + ROWS : Tv;
    const double mean = stats[b * 2 * F + f];
    float q = 0.f;
    if (lane_r < rl)
        for (int64_t t = r0 + lane_r; t < r1; t += rl) {
            const float d = (float)((double)log_rule(m[t * F + f], guard, clamp) - mean);
            q += d * d;
        }
    red[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x < F) {
        float tq = 0.f;
        for (int k = 0; k < rl; ++k) tq += red[k * F + threadIdx.x];
        partial[(b * nb + blockIdx.x) * 2 * F + threadIdx.x] = tq;
    }
}

// 64 bins x 16 block lanes, in double: lane l adds the blocks l, l + 16, ..., then the lanes in order (the layout of logmel.hip).
// second == 0: stats[b, f] = mean from the (pivot, sum) pairs; second != 0: stats[b, F + f] = 1 / (unbiased std + eps) from the centred sums.
__global__ __launch_bounds__(1024) void finalise_kernel(const float* __restrict__ partial, double* __restrict__ stats, const int32_t* __restrict__ lens,
                                                        int64_t nb, int64_t T, int F, float eps, int second) {
    __shared__ double red[16][64];
    const int64_t b = blockIdx.y;
    const int64_t Tv = dyn::valid_rows(lens, b, T);
    const int cl = threadIdx.x & 63, bl = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + cl;
    const float* pb = partial + b * nb * 2 * F;
    double s = 0.0;
    if (f < F)
        for (int64_t k = bl; k < nb; k += 16) {
            if (second) {
                s += (double)pb[k * 2 * F + f];
            } else {
                const int64_t left = Tv - k * ROWS;
                const int64_t rows = left >= ROWS ? ROWS : (left > 0 ? left : 0);
                s += (double)rows * (double)pb[k * 2 * F + f] + (double)pb[k * 2 * F + F + f];
            }
        }
    red[bl][cl] = s;
    __syncthreads();
    if (bl == 0 && f < F) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        if (second) {
            const double var = Tv > 1 ? t / (double)(Tv - 1) : 0.0;
            stats[b * 2 * F + F + f] = 1.0 / (sqrt(var) + (double)eps);
        } else {
            stats[b * 2 * F + f] = Tv > 0 ? t / (double)Tv : 0.0;
        }
    }
}

__device__ __forceinline__ float finish_value(float m, const double* __restrict__ st, int F, int f, float guard, int clamp, int normalize) {
    const float v = log_rule(m, guard, clamp);
    return normalize ? (float)(((double)v - st[f]) * st[F + f]) : v;
}

// out [B, T, F]: the value of every valid frame, exact zeros past the row's count
__global__ __launch_bounds__(TPB) void apply_tf_kernel(const float* __restrict__ mel, float* __restrict__ out, const double* __restrict__ stats,
                                                       const int32_t* __restrict__ lens, int64_t T, int F, float guard, int clamp, int normalize) {
    const int64_t b = blockIdx.y;
    const int64_t Tv = dyn::valid_rows(lens, b, T);
    const float* m = mel + b * T * F;
    float* o = out + b * T * F;
    const double* st = stats + b * 2 * F;
    const int64_t total = T * F, live = Tv * F;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB)
        o[i] = i < live ? finish_value(m[i], st, F, (int)(i % F), guard, clamp, normalize) : 0.f;
}

// out [B, F, T]: the same values through a 32 x 32 LDS tile
__global__ __launch_bounds__(TPB) void apply_ft_kernel(const float* __restrict__ mel, float* __restrict__ out, const double* __restrict__ stats,
                                                       const int32_t* __restrict__ lens, int64_t T, int F, float guard, int clamp, int normalize) {
    __shared__ float tile[32][33];
    const int64_t b = blockIdx.z;
    const int64_t Tv = dyn::valid_rows(lens, b, T);
    const float* m = mel + b * T * F;
    float* o = out + b * T * F;
    const double* st = stats + b * 2 * F;
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    const int f0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int64_t t = t0 + j;
        const int f = f0 + tx;
        tile[j][tx] = (t < Tv && f < F) ? finish_value(m[t * F + f], st, F, f, guard, clamp, normalize) : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int f = f0 + j;
        const int64_t t = t0 + tx;
        if (f < F && t < T) o[(int64_t)f * T + t] = tile[tx][j];
    }
}
}  // namespace

extern "C" int dyn_melfeat_prep(const float* x, float* out, const int32_t* lens, const float* noise, const float* prev, int64_t B, int64_t Lmax,
                                int64_t pad, int64_t W, float preemphasis, float dither, void* stream) {
    DYN_REQUIRE(x && out && lens, DYN_E_ARG, "dyn_melfeat_prep: null pointer (x, out and lens are required)");
    DYN_REQUIRE(B >= 0 && B < 65536 && Lmax >= 1 && pad >= 0 && W >= pad + Lmax && W < (1ll << 40), DYN_E_ARG,
                "dyn_melfeat_prep: B=%lld Lmax=%lld pad=%lld W=%lld (need W >= pad + Lmax)", (long long)B, (long long)Lmax, (long long)pad,
                (long long)W);
    DYN_REQUIRE(preemphasis >= 0.f && preemphasis < 1.f && dither >= 0.f, DYN_E_ARG, "dyn_melfeat_prep: preemphasis in [0, 1), dither >= 0");
    if (B == 0) return DYN_OK;
    int64_t g = dyn::cdiv(W, TPB);
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)g, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, x, out, lens, noise, prev, Lmax, pad, W,
                       preemphasis, dither);
    return dyn::check_launch("dyn_melfeat_prep");
}

// [B, blocks, 2F] floats (the per-block partials of either pass) followed by [B, 2F] doubles (mean, 1 / (std + eps))
extern "C" int64_t dyn_melfeat_finish_workspace_bytes(int64_t B, int64_t T, int64_t F) {
    if (B < 0 || T < 0 || F < 0) return 0;
    return B * dyn::cdiv(T, ROWS) * 2 * F * (int64_t)sizeof(float) + B * 2 * F * (int64_t)sizeof(double);
}

extern "C" int dyn_melfeat_finish(const float* mel, float* out, const int32_t* lens, int64_t B, int64_t T, int64_t F, float guard, int32_t clamp,
                                  int32_t normalize, float eps, int32_t layout, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(mel && out && lens, DYN_E_ARG, "dyn_melfeat_finish: null pointer (mel, out and lens are required)");
    DYN_REQUIRE(mel != out, DYN_E_ARG, "dyn_melfeat_finish: out must not alias mel");
    DYN_REQUIRE(B >= 0 && B < 65536 && T >= 1 && T < (1ll << 31) && F >= 1 && F <= TPB, DYN_E_ARG, "dyn_melfeat_finish: B=%lld T=%lld F=%lld (F <= 256)",
                (long long)B, (long long)T, (long long)F);
    DYN_REQUIRE(guard > 0.f && eps >= 0.f, DYN_E_ARG, "dyn_melfeat_finish: the log guard / floor must be positive, eps non-negative");
    DYN_REQUIRE(layout == 0 || layout == 1, DYN_E_ARG, "dyn_melfeat_finish: layout %d (0 = [B, T, F], 1 = [B, F, T])", (int)layout);
    DYN_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= dyn_melfeat_finish_workspace_bytes(B, T, F), DYN_E_WORKSPACE,
                "dyn_melfeat_finish: workspace too small or not 8-byte aligned");
    if (B == 0) return DYN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = dyn::cdiv(T, ROWS);
    float* partial = (float*)workspace;
    double* stats = (double*)(partial + B * nb * 2 * F);        // 2F floats per block: the offset is a multiple of 8 bytes
    if (normalize) {
        const dim3 gp((unsigned)nb, (unsigned)B), gc((unsigned)dyn::cdiv(F, 64), (unsigned)B);
        hipLaunchKernelGGL(pivot_sum_kernel, gp, dim3(TPB), 0, st, mel, partial, lens, T, (int)F, guard, (int)clamp);
        hipLaunchKernelGGL(finalise_kernel, gc, dim3(1024), 0, st, partial, stats, lens, nb, T, (int)F, eps, 0);
        hipLaunchKernelGGL(centred_sq_kernel, gp, dim3(TPB), 0, st, mel, stats, partial, lens, T, (int)F, guard, (int)clamp);
        hipLaunchKernelGGL(finalise_kernel, gc, dim3(1024), 0, st, partial, stats, lens, nb, T, (int)F, eps, 1);
    }
    if (layout == 0) {
        int64_t g = dyn::cdiv(T * F, TPB);
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(apply_tf_kernel, dim3((unsigned)g, (unsigned)B), dim3(TPB), 0, st, mel, out, stats, lens, T, (int)F, guard, (int)clamp,
                           (int)normalize);
    } else {
        hipLaunchKernelGGL(apply_ft_kernel, dim3((unsigned)dyn::cdiv(T, 32), (unsigned)dyn::cdiv(F, 32), (unsigned)B), dim3(TPB), 0, st, mel, out,
                           stats, lens, T, (int)F, guard, (int)clamp, (int)normalize);
    }
    return dyn::check_launch("dyn_melfeat_finish");
}
