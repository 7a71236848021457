// Log-mel front end on device: 16 kHz waveform -> [80, T] log-mel, per-bin normalised (100 frames / s).
// Replaces upstream `lcasr.utils.audio_tools.processing_chain / to_spectogram` as called by the dataset adapters
// (reference lcasr/earnings22/run.py:61, tedlium/run.py:94, chime6/run.py:61-68) — today a CPU step serial with the GPU.
//
// MI355X mapping: the STFT is ONE fp32-MFMA GEMM.  Frames are overlapping rows of the reflect-padded signal, so the
// frame matrix is never materialised: A[t, n] = xpad[t * hop + n] is addressed with lda = hop (160) < K (400) and the
// Hann window and the 56-sample centring offset of the 400-tap window inside the 512-point frame are folded into the
// DFT basis B[n, k] = w[n] * {cos, -sin}(2 pi k (n + 56) / 512)  (dyn_gemm_f32, NN).  The remaining kernels are
// HBM-bound passes: power, mel projection (second GEMM), log + column sums, centred column squares (a second pass over
// [T, 80], only when normalising), normalise + transpose.
#include "common.h"

namespace {
constexpr int TPB = 256;

// out[i] = x[reflect(i - pad)], i in [0, n + 2 pad): torch.stft(center=True, pad_mode='reflect')
__global__ __launch_bounds__(TPB) void reflect_pad_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int64_t pad) {
    const int64_t total = n + 2 * pad;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
        int64_t j = i - pad;
        if (j < 0) j = -j;
        if (j >= n) j = 2 * (n - 1) - j;
        j = j < 0 ? 0 : (j >= n ? n - 1 : j);
        out[i] = x[j];
    }
}

// reim [T, 2*KP] (re in [0,KP), im in [KP, 2KP)) -> P [T, KP] = re^2 + im^2
__global__ __launch_bounds__(TPB) void power_kernel(const float* __restrict__ reim, float* __restrict__ P, int64_t T, int KP) {
    const int64_t total = T * KP;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
        const int64_t t = i / KP;
        const int k = (int)(i % KP);
        const float re = reim[t * 2 * KP + k], im = reim[t * 2 * KP + KP + k];
        P[i] = re * re + im * im;
    }
}

// Per-bin statistics of the normalised output, all CENTRED (the variance is never the difference of two accumulated sums: the log-mel
// of an empty band sits at log(eps) = -13.8 with a spread of 1e-3, where E[v^2] - mean^2 from fp32 sums is rounding noise):
//   1. log_sum_kernel        v = log(mel + eps) in place; per 256-row block and column the pivot (the block's first v) and the fp32
//                            sum of v - pivot (zero, exactly, for a constant column)
//   2. column_mean_kernel    mean = sum_b (rows_b * pivot_b + sum_b) / T in double, in a fixed order
//   3. centred_sq_kernel     per block and column the fp32 sum of (v - mean)^2
//   4. column_rstd_kernel    1 / sqrt(sum_b M2_b / (T - 1)) in double; 0 for a column of zero variance and for T == 1
// Every sum has a fixed order (row lanes, then blocks by 16 lanes of stride 16, lanes in order): two calls are bit-identical.
constexpr int ROWS = 256;                       // rows per moment block

// mel [T, F] -> log(mel + eps) in place; partial [block, 2F] = per column (pivot, sum of v - pivot) over this block's rows
__global__ __launch_bounds__(TPB) void log_sum_kernel(float* __restrict__ mel, float* __restrict__ partial, int64_t T, int F, float eps) {
    __shared__ float red[TPB];
    __shared__ float piv[TPB];
    const int f = threadIdx.x % F;
    const int lane_r = threadIdx.x / F;          // row lane inside the block
    const int rl = TPB / F;                      // row lanes (3 for F = 80)
    const int64_t r0 = (int64_t)blockIdx.x * ROWS;
    const int64_t r1 = (r0 + ROWS < T) ? r0 + ROWS : T;
    if (threadIdx.x < F) piv[threadIdx.x] = logf(mel[r0 * F + threadIdx.x] + eps);   // read before any lane overwrites row r0
    __syncthreads();
    const float p = piv[f];
    float s = 0.f;
    if (lane_r < rl)
        for (int64_t t = r0 + lane_r; t < r1; t += rl) {
            const float v = logf(mel[t * F + f] + eps);
            mel[t * F + f] = v;
            s += v - p;
        }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < F) {
        float ts = 0.f;
        for (int k = 0; k < rl; ++k) ts += red[k * F + threadIdx.x];
        partial[(int64_t)blockIdx.x * 2 * F + threadIdx.x] = p;
        partial[(int64_t)blockIdx.x * 2 * F + F + threadIdx.x] = ts;
    }
}

// partial [block, F] = per column sum of (x - mean)^2 over this block's rows (x is the log left by log_sum_kernel)
__global__ __launch_bounds__(TPB) void centred_sq_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                         float* __restrict__ partial, int64_t T, int F) {
    __shared__ float red[TPB];
    const int f = threadIdx.x % F;
    const int lane_r = threadIdx.x / F;
    const int rl = TPB / F;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS;
    const int64_t r1 = (r0 + ROWS < T) ? r0 + ROWS : T;
    const double mean = stats[f];
    float q = 0.f;
    if (lane_r < rl)
        for (int64_t t = r0 + lane_r; t < r1; t += rl) {
            const float d = (float)((double)x[t * F + f] - mean);
            q += d * d;
        }
    red[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x < F) {
        float tq = 0.f;
        for (int k = 0; k < rl; ++k) tq += red[k * F + threadIdx.x];
        partial[(int64_t)blockIdx.x * F + threadIdx.x] = tq;
    }
}

// 64 columns x 16 block lanes (the layout of reduce.h), accumulated in double: lane l adds the blocks l, l + 16, ..., then the lanes in order.
// stats[f] = mean of column f from the (pivot, sum) pairs of log_sum_kernel
__global__ __launch_bounds__(1024) void column_mean_kernel(const float* __restrict__ partial, double* __restrict__ stats, int64_t nb,
                                                           int64_t T, int F) {
    __shared__ double red[16][64];
    const int cl = threadIdx.x & 63, bl = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + cl;
    double s = 0.0;
    if (f < F)
        for (int64_t b = bl; b < nb; b += 16) {
            const int64_t rows = (b + 1) * ROWS <= T ? ROWS : T - b * ROWS;
            s += (double)rows * (double)partial[b * 2 * F + f] + (double)partial[b * 2 * F + F + f];
        }
    red[bl][cl] = s;
    __syncthreads();
    if (bl == 0 && f < F) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        stats[f] = t / (double)T;
    }
}

// stats[F + f] = 1 / unbiased std of column f from the centred sums of centred_sq_kernel (0 where the variance is 0, and for T == 1)
__global__ __launch_bounds__(1024) void column_rstd_kernel(const float* __restrict__ partial, double* __restrict__ stats, int64_t nb,
                                                           int64_t T, int F) {
    __shared__ double red[16][64];
    const int cl = threadIdx.x & 63, bl = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + cl;
    double s = 0.0;
    if (f < F)
        for (int64_t b = bl; b < nb; b += 16) s += (double)partial[b * F + f];
    red[bl][cl] = s;
    __syncthreads();
    if (bl == 0 && f < F) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        const double var = T > 1 ? t / (double)(T - 1) : 0.0;
        stats[F + f] = var > 0.0 ? 1.0 / sqrt(var) : 0.0;
    }
}

// out[f, t] = (x[t, f] - mean_f) / std_f with the unbiased std over T (stats [2F] = column mean and 1 / std, from the kernels above)
__global__ __launch_bounds__(TPB) void normalize_transpose_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                                  float* __restrict__ out, int64_t T, int F, int normalize) {
    __shared__ float tile[32][33];
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    const int f0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int64_t t = t0 + j;
        const int f = f0 + tx;
        tile[j][tx] = (t < T && f < F) ? x[t * F + f] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int f = f0 + j;
        const int64_t t = t0 + tx;
        if (f < F && t < T) {
            float v = tile[tx][j];
            if (normalize) v = (float)(((double)v - stats[f]) * stats[F + f]);
            out[(int64_t)f * T + t] = v;
        }
    }
}
}  // namespace

// Per-row (mean, unbiased std) normalisation of a [R, T] spectrogram in place or out of place: the renormalisation after
// the CHiME-6 channel average, reference lcasr/chime6/run.py:66-68  (spec - spec.mean(-1)) / spec.std(-1).
// One 1024-thread workgroup per row; two passes (mean, then centred sum of squares) so long rows do not cancel.
namespace {
__global__ __launch_bounds__(1024) void rownorm_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t T) {
    __shared__ float red[16];
    const float* src = x + (int64_t)blockIdx.x * T;
    float* dst = out + (int64_t)blockIdx.x * T;
    float s = 0.f;
    for (int64_t t = threadIdx.x; t < T; t += 1024) s += src[t];
    const float mean = dyn::block_sum(s, red) / (float)T;
    float q = 0.f;
    for (int64_t t = threadIdx.x; t < T; t += 1024) { const float d = src[t] - mean; q += d * d; }
    const float var = dyn::block_sum(q, red) / (float)(T > 1 ? T - 1 : 1);
    const float inv = 1.f / sqrtf(var);
    for (int64_t t = threadIdx.x; t < T; t += 1024) dst[t] = (src[t] - mean) * inv;
}
}  // namespace

extern "C" int dyn_rownorm(const float* x, float* out, int64_t R, int64_t T, void* stream) {
    DYN_REQUIRE(x && out && R >= 0 && T >= 0 && R < (1ll << 31), DYN_E_ARG, "dyn_rownorm: bad arguments");
    if (R == 0 || T == 0) return DYN_OK;
    hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)R), dim3(1024), 0, (hipStream_t)stream, x, out, T);
    return dyn::check_launch("dyn_rownorm");
}

extern "C" int dyn_reflect_pad(const float* x, float* out, int64_t n, int64_t pad, void* stream) {
    DYN_REQUIRE(x && out && n > 1 && pad >= 0 && pad < n, DYN_E_ARG, "dyn_reflect_pad: bad arguments (need pad < n)");
    int64_t g = dyn::cdiv(n + 2 * pad, TPB);
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(reflect_pad_kernel, dim3((unsigned)g), dim3(TPB), 0, (hipStream_t)stream, x, out, n, pad);
    return dyn::check_launch("dyn_reflect_pad");
}

extern "C" int dyn_stft_power(const float* reim, float* power, int64_t T, int64_t KP, void* stream) {
    DYN_REQUIRE(reim && power && T >= 0 && KP > 0, DYN_E_ARG, "dyn_stft_power: bad arguments");
    if (T == 0) return DYN_OK;
    int64_t g = dyn::cdiv(T * KP, TPB);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(power_kernel, dim3((unsigned)g), dim3(TPB), 0, (hipStream_t)stream, reim, power, T, (int)KP);
    return dyn::check_launch("dyn_stft_power");
}

// [blocks, 2F] floats (the per-block partials of either pass) followed by the [2F] doubles (mean, 1 / std) of the columns
extern "C" int64_t dyn_logmel_finish_workspace_bytes(int64_t T, int64_t F) {
    return dyn::cdiv(T, ROWS) * 2 * F * (int64_t)sizeof(float) + 2 * F * (int64_t)sizeof(double);
}

// mel [T, F] (overwritten with its log) -> out [F, T]; normalize != 0 applies the per-bin (mean, unbiased std) over T.
extern "C" int dyn_logmel_finish(float* mel, float* out, int64_t T, int64_t F, float eps, int32_t normalize, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(mel && out && T > 0 && F > 0 && F <= TPB, DYN_E_ARG, "dyn_logmel_finish: bad arguments");
    DYN_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= dyn_logmel_finish_workspace_bytes(T, F), DYN_E_WORKSPACE,
                "dyn_logmel_finish: workspace too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = dyn::cdiv(T, ROWS);
    float* partial = (float*)workspace;
    double* stats = (double*)(partial + nb * 2 * F);            // 2F floats per block: the offset is a multiple of 8 bytes
    hipLaunchKernelGGL(log_sum_kernel, dim3((unsigned)nb), dim3(TPB), 0, st, mel, partial, T, (int)F, eps);
    if (normalize) {
        const unsigned gc = (unsigned)dyn::cdiv(F, 64);
        hipLaunchKernelGGL(column_mean_kernel, dim3(gc), dim3(1024), 0, st, partial, stats, nb, T, (int)F);
        hipLaunchKernelGGL(centred_sq_kernel, dim3((unsigned)nb), dim3(TPB), 0, st, mel, stats, partial, T, (int)F);
        hipLaunchKernelGGL(column_rstd_kernel, dim3(gc), dim3(1024), 0, st, partial, stats, nb, T, (int)F);
    }
    hipLaunchKernelGGL(normalize_transpose_kernel, dim3((unsigned)dyn::cdiv(T, 32), (unsigned)dyn::cdiv(F, 32)), dim3(TPB), 0, st, mel,
                       stats, out, T, (int)F, (int)normalize);
    return dyn::check_launch("dyn_logmel_finish");
}
