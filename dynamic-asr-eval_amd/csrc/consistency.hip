// Kernels of the consistency loop (reference lcasr/lib.py:646-903, lib.dynamic_eval_consistency_ctc_loss):
//   dyn_grad_mix_decay  — the distance-decayed mix of the per-window gradients (reference :817-841), bit for bit
//   dyn_adafactor_step  — torch.optim.Adafactor's single-tensor rule over a flat buffer with a segment table
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ gradient mix
// G[W][stride]: row q = the gradient of window q.  For i = 0 .. W-1, in place and in this order (so rows q < i are already mixed):
//   G[i] <- fl32( ( f64(G[i]) + sum_{q != i, ascending} f64( fl32(fl32(decay[|i-q|]) * G[q]) ) ) / denom[i] )
// which is statement for statement what the reference computes with torch on the host: `decay * q_param.grad` is a float32
// product by the Python double rounded to float32, `.to(float64)` widens it exactly, `cur_grad +=` is a float64 add in ascending
// q, `/ total_sum` one float64 divide, `.to(float32)` the narrowing.  Every one of these is a single correctly rounded IEEE
// operation here as well (the product cannot contract into the add: a conversion sits between them), hence equal bits.
// One thread owns one element: its W values are staged in LDS as column `threadIdx.x` of a [W][MIX_TPB] tile (consecutive lanes
// in consecutive banks), and only that thread ever touches the column, so the recurrence needs no barrier.
constexpr int MIX_TPB = 64;
constexpr int64_t MIX_LDS_STATIC_LIMIT = 64 * 1024;
constexpr int64_t MIX_LDS_LIMIT = 160 * 1024;

__global__ __launch_bounds__(MIX_TPB) void grad_mix_kernel(float* __restrict__ G, int64_t stride, int W, int64_t lo, int64_t hi,
                                                           const double* __restrict__ decay, const double* __restrict__ denom) {
    extern __shared__ float mix_lds[];
    float* col = mix_lds + threadIdx.x;            // element q of this thread's column: col[q * MIX_TPB]
    float* dec = mix_lds + (int64_t)W * MIX_TPB;   // fl32(decay[k]), k = 0 .. W-1
    const int64_t e = lo + (int64_t)blockIdx.x * MIX_TPB + threadIdx.x;
    const bool live = e < hi;
    for (int q = 0; q < W; ++q) col[q * MIX_TPB] = live ? G[(int64_t)q * stride + e] : 0.f;
    for (int k = threadIdx.x; k < W; k += MIX_TPB) dec[k] = (float)decay[k];
    __syncthreads();
    for (int i = 0; i < W; ++i) {
        double acc = (double)col[i * MIX_TPB];
        for (int q = 0; q < i; ++q) acc += (double)__fmul_rn(dec[i - q], col[q * MIX_TPB]);
        for (int q = i + 1; q < W; ++q) acc += (double)__fmul_rn(dec[q - i], col[q * MIX_TPB]);
        col[i * MIX_TPB] = (float)(acc / denom[i]);
    }
    if (live)
        for (int q = 0; q < W; ++q) G[(int64_t)q * stride + e] = col[q * MIX_TPB];
}

// ------------------------------------------------------------------------------------------------ Adafactor
// Segment table (device, int64, SEG_COLS entries per tensor): the tensor's offset in the flat buffer, its shape as batch x rows x cols
// (the last two dimensions, leading ones as batch; a 1-D tensor of n elements is 1 x 1 x n and not factored), the offset of its state
// in the state buffer (factored: row_var [batch * rows] then col_var [batch * cols]; else variance [n]), and where its rows,
// batches and factored columns begin in the launches' index spaces.  Work is spread by ROW (one wave each) or by COLUMN (one thread each) over all tensors in one
// launch: a launch finds its tensor by bisection of the table.
constexpr int SEG_COLS = 9;
enum { S_OFF = 0, S_BATCH, S_ROWS, S_COLS, S_STATE, S_FACTORED, S_ROW0, S_BATCH0, S_COL0 };
constexpr int ADA_TPB = 256;

struct AdaArgs {
    const int64_t* seg;
    int n_seg;
    int64_t n_rows, n_batches, n_cols;   // totals over all tensors (n_cols counts batch * cols of the factored ones only)
    float w;                             // one_minus_beta2_t = step^beta2_decay, the lerp weight
    float eps1, eps1_sq;
    double rho, eps2, d, lr_wd;          // rho_t = min(lr, 1 / sqrt(step)); lr * weight_decay
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch's lerp (ATen/native/Lerp.h) in float32
__device__ __forceinline__ float lerp_f32(float self, float end, float w) {
    const float diff = end - self;
    return fabsf(w) < 0.5f ? self + w * diff : end - diff * (1.f - w);
}

// largest s with table[s * SEG_COLS + key] <= v
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ seg, int n_seg, int key, int64_t v) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid * SEG_COLS + key] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float rsqrt_rn(float x) { return 1.f / sqrtf(x); }

// Pass 1, one wave per row: psq[row] = sum p^2; factored: row_var = lerp(row_var, sum g^2 / cols, w);
// 1-D: variance = lerp(variance, g^2, w) element by element.
__global__ __launch_bounds__(ADA_TPB) void ada_rows_stats_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ state, double* __restrict__ psq, const AdaArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (ADA_TPB / 64) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int64_t* s = a.seg + (int64_t)seg_of(a.seg, a.n_seg, S_ROW0, row) * SEG_COLS;
    const int64_t r = row - s[S_ROW0], cols = s[S_COLS], base = s[S_OFF] + r * cols;
    double sp = 0.0, sg = 0.0;
    if (s[S_FACTORED]) {
        for (int64_t c = lane; c < cols; c += 64) {
            const float pv = p[base + c], gv = g[base + c];
            sp += (double)pv * pv;
            sg += (double)gv * gv;
        }
    } else {
        float* var = state + s[S_STATE];
        for (int64_t c = lane; c < cols; c += 64) {
            const float pv = p[base + c], gv = g[base + c];
            sp += (double)pv * pv;
            var[c] = lerp_f32(var[c], gv * gv, a.w);
        }
    }
    sp = wave_sum_f64(sp);
    sg = wave_sum_f64(sg);
    if (lane == 0) {
        psq[row] = sp;
        if (s[S_FACTORED]) {
            float* rv = state + s[S_STATE] + r;
            // torch: norm(grad, dim=-1).square_().div_(cols)
            const float nrm = (float)sqrt(sg);
            *rv = lerp_f32(*rv, nrm * nrm / (float)cols, a.w);
        }
    }
}

// Pass 2, one thread per (batch, column) of the factored tensors: col_var = lerp(col_var, sum_r g^2 / rows, w).
__global__ __launch_bounds__(ADA_TPB) void ada_cols_stats_kernel(const float* __restrict__ g, float* __restrict__ state, const AdaArgs a) {
    const int64_t t = (int64_t)blockIdx.x * ADA_TPB + threadIdx.x;
    if (t >= a.n_cols) return;
    // a tensor that is not factored has no columns here: among equal starts the bisection takes the last, the factored one
    const int64_t* s = a.seg + (int64_t)seg_of(a.seg, a.n_seg, S_COL0, t) * SEG_COLS;
    const int64_t first = s[S_COL0];
    const int64_t rows = s[S_ROWS], cols = s[S_COLS], k = t - first, b = k / cols, c = k - b * cols;
    const float* gb = g + s[S_OFF] + b * rows * cols + c;
    double acc = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        const float gv = gb[r * cols];
        acc += (double)gv * gv;
    }
    float* cv = state + s[S_STATE] + s[S_BATCH] * rows + k;
    const float nrm = (float)sqrt(acc);
    *cv = lerp_f32(*cv, nrm * nrm / (float)rows, a.w);
}

// Pass 3, one wave per batch of the factored tensors: rmean[batch] = max(mean_r row_var, eps1).
__global__ __launch_bounds__(ADA_TPB) void ada_row_mean_kernel(const float* __restrict__ state, float* __restrict__ rmean, const AdaArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t bt = (int64_t)blockIdx.x * (ADA_TPB / 64) + (threadIdx.x >> 6);
    if (bt >= a.n_batches) return;
    const int64_t* s = a.seg + (int64_t)seg_of(a.seg, a.n_seg, S_BATCH0, bt) * SEG_COLS;
    if (!s[S_FACTORED]) {
        if (lane == 0) rmean[bt] = 1.f;
        return;
    }
    const int64_t b = bt - s[S_BATCH0], rows = s[S_ROWS];
    const float* rv = state + s[S_STATE] + b * rows;
    double acc = 0.0;
    for (int64_t r = lane; r < rows; r += 64) acc += (double)rv[r];
    acc = wave_sum_f64(acc);
    if (lane == 0) rmean[bt] = fmaxf((float)(acc / (double)rows), a.eps1);
}

// update = rsqrt(max(var_estimate, eps1^2)) * g of one element
__device__ __forceinline__ float ada_update(float gv, float rv, float cv, float rm, bool factored, float var, const AdaArgs& a) {
    const float est = factored ? (rv * cv) / rm : var;
    return rsqrt_rn(fmaxf(est, a.eps1_sq)) * gv;
}

// Pass 4 (APPLY = false), one wave per row: usq[row] = sum update^2.
// Pass 6 (APPLY = true): p = p * (1 - lr * wd) + coef[tensor] * update.
template <bool APPLY>
__global__ __launch_bounds__(ADA_TPB) void ada_rows_update_kernel(float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ state,
                                                                  const float* __restrict__ rmean, double* __restrict__ usq,
                                                                  const float* __restrict__ coef, const AdaArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (ADA_TPB / 64) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int si = seg_of(a.seg, a.n_seg, S_ROW0, row);
    const int64_t* s = a.seg + (int64_t)si * SEG_COLS;
    const bool factored = s[S_FACTORED] != 0;
    const int64_t r = row - s[S_ROW0], rows = s[S_ROWS], cols = s[S_COLS], base = s[S_OFF] + r * cols, b = r / rows;
    const float* st = state + s[S_STATE];
    const float rv = factored ? st[r] : 0.f, rm = factored ? rmean[s[S_BATCH0] + b] : 1.f;
    const float* cvp = st + s[S_BATCH] * rows + b * cols;
    const float keep = (float)(1.0 - a.lr_wd), cf = APPLY ? coef[si] : 0.f;
    double su = 0.0;
    for (int64_t c = lane; c < cols; c += 64) {
        const float u = ada_update(g[base + c], rv, factored ? cvp[c] : 0.f, rm, factored, factored ? 0.f : st[c], a);
        if (APPLY) {
            float pv = p[base + c];
            if (a.lr_wd != 0.0) pv *= keep;
            p[base + c] = pv + cf * u;
        } else {
            su += (double)u * u;
        }
    }
    if (!APPLY) {
        su = wave_sum_f64(su);
        if (lane == 0) usq[row] = su;
    }
}

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// Pass 5, one workgroup per tensor: alpha = max(eps2, ||p|| / sqrt(n)) * rho_t, denom = max(1, ||update|| / (sqrt(n) * d)),
// coef = -alpha / denom (the scalars torch takes through .item(), as doubles).
__global__ __launch_bounds__(ADA_TPB) void ada_coef_kernel(const double* __restrict__ psq, const double* __restrict__ usq, float* __restrict__ coef,
                                                           const AdaArgs a) {
    __shared__ double red[16];
    const int64_t* s = a.seg + (int64_t)blockIdx.x * SEG_COLS;
    const int64_t nrows = s[S_BATCH] * s[S_ROWS], row0 = s[S_ROW0];
    double sp = 0.0, su = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += ADA_TPB) {
        sp += psq[row0 + r];
        su += usq[row0 + r];
    }
    sp = block_sum_f64(sp, red);
    su = block_sum_f64(su, red);
    if (threadIdx.x == 0) {
        const double rn = sqrt((double)(nrows * s[S_COLS]));
        const double alpha = fmax(a.eps2, (double)(float)sqrt(sp) / rn) * a.rho;
        const double den = fmax(1.0, (double)(float)sqrt(su) / (rn * a.d));
        coef[blockIdx.x] = (float)(-alpha / den);
    }
}

}  // namespace

extern "C" int64_t dyn_grad_mix_decay_max_windows(void) { return (MIX_LDS_LIMIT / 4) / (MIX_TPB + 1); }

extern "C" int dyn_grad_mix_decay(float* grads, int64_t row_stride, int32_t n_windows, const int64_t* ranges, int32_t n_ranges,
                                  const double* decay, const double* denom, void* stream) {
    DYN_REQUIRE(grads && decay && denom && n_windows >= 1 && n_ranges >= 0 && (ranges || n_ranges == 0) && row_stride >= 0,
                DYN_E_ARG, "dyn_grad_mix_decay: bad arguments");
    const int64_t lds = ((int64_t)n_windows * MIX_TPB + n_windows) * (int64_t)sizeof(float);
    DYN_REQUIRE(lds <= MIX_LDS_LIMIT, DYN_E_ARG, "dyn_grad_mix_decay: %d windows need %lld B of LDS per workgroup, more than the %lld B of a CU (at most %lld windows)",
                (int)n_windows, (long long)lds, (long long)MIX_LDS_LIMIT, (long long)dyn_grad_mix_decay_max_windows());
    for (int r = 0; r < n_ranges; ++r)
        DYN_REQUIRE(ranges[2 * r] >= 0 && ranges[2 * r] <= ranges[2 * r + 1] && (n_windows == 1 || ranges[2 * r + 1] <= row_stride), DYN_E_ARG,
                    "dyn_grad_mix_decay: range %d = [%lld, %lld) outside a row of %lld elements", r, (long long)ranges[2 * r],
                    (long long)ranges[2 * r + 1], (long long)row_stride);
    if (lds > MIX_LDS_STATIC_LIMIT) {
        hipError_t e = hipFuncSetAttribute((const void*)grad_mix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DYN_REQUIRE(e == hipSuccess, DYN_E_LAUNCH, "dyn_grad_mix_decay: %lld B of LDS refused: %s", (long long)lds, hipGetErrorString(e));
    }
    for (int r = 0; r < n_ranges; ++r) {
        const int64_t lo = ranges[2 * r], hi = ranges[2 * r + 1];
        if (hi == lo) continue;
        hipLaunchKernelGGL(grad_mix_kernel, dim3((unsigned)dyn::cdiv(hi - lo, MIX_TPB)), dim3(MIX_TPB), (size_t)lds, (hipStream_t)stream, grads,
                           row_stride, (int)n_windows, lo, hi, decay, denom);
    }
    return dyn::check_launch("dyn_grad_mix_decay");
}

extern "C" int64_t dyn_adafactor_scratch_bytes(int64_t n_rows, int64_t n_batches, int64_t n_segments) {
    return (2 * n_rows) * (int64_t)sizeof(double) + (n_batches + n_segments) * (int64_t)sizeof(float) + 64;
}

extern "C" int dyn_adafactor_step(float* params, const float* grads, float* state, const int64_t* segments, int32_t n_segments,
                                  int64_t n_rows, int64_t n_batches, int64_t n_factored_cols, double lr, double beta2_decay, double eps1,
                                  double eps2, double d, double weight_decay, int64_t step, void* scratch, int64_t scratch_bytes,
                                  void* stream) {
    DYN_REQUIRE(params && grads && state && segments && n_segments >= 1 && n_rows >= 1 && n_batches >= 1 && n_factored_cols >= 0 && step >= 1,
                DYN_E_ARG, "dyn_adafactor_step: bad arguments (step counts from 1)");
    DYN_REQUIRE(lr >= 0.0 && beta2_decay <= 0.0 && eps1 >= 0.0 && eps2 >= 0.0 && d >= 1.0 && weight_decay >= 0.0, DYN_E_ARG,
                "dyn_adafactor_step: hyper-parameter out of torch.optim.Adafactor's range");
    DYN_REQUIRE(scratch && scratch_bytes >= dyn_adafactor_scratch_bytes(n_rows, n_batches, n_segments), DYN_E_WORKSPACE,
                "dyn_adafactor_step: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    AdaArgs a;
    a.seg = segments; a.n_seg = n_segments; a.n_rows = n_rows; a.n_batches = n_batches; a.n_cols = n_factored_cols;
    const double sf = (double)step;
    a.w = (float)pow(sf, beta2_decay);
    a.eps1 = (float)eps1; a.eps1_sq = (float)(eps1 * eps1);
    const double inv = 1.0 / sqrt(sf);
    a.rho = lr < inv ? lr : inv; a.eps2 = eps2; a.d = d; a.lr_wd = lr * weight_decay;
    double* psq = (double*)scratch;
    double* usq = psq + n_rows;
    float* rmean = (float*)(usq + n_rows);
    float* coef = rmean + n_batches;
    const unsigned row_blocks = (unsigned)dyn::cdiv(n_rows, ADA_TPB / 64);
    hipLaunchKernelGGL(ada_rows_stats_kernel, dim3(row_blocks), dim3(ADA_TPB), 0, st, (const float*)params, grads, state, psq, a);
    if (n_factored_cols > 0)
        hipLaunchKernelGGL(ada_cols_stats_kernel, dim3((unsigned)dyn::cdiv(n_factored_cols, ADA_TPB)), dim3(ADA_TPB), 0, st, grads, state, a);
    hipLaunchKernelGGL(ada_row_mean_kernel, dim3((unsigned)dyn::cdiv(n_batches, ADA_TPB / 64)), dim3(ADA_TPB), 0, st, (const float*)state, rmean, a);
    hipLaunchKernelGGL(ada_rows_update_kernel<false>, dim3(row_blocks), dim3(ADA_TPB), 0, st, params, grads, (const float*)state,
                       (const float*)rmean, usq, (const float*)coef, a);
    hipLaunchKernelGGL(ada_coef_kernel, dim3((unsigned)n_segments), dim3(ADA_TPB), 0, st, (const double*)psq, (const double*)usq, coef, a);
    hipLaunchKernelGGL(ada_rows_update_kernel<true>, dim3(row_blocks), dim3(ADA_TPB), 0, st, params, grads, (const float*)state,
                       (const float*)rmean, usq, (const float*)coef, a);
    return dyn::check_launch("dyn_adafactor_step");
}
