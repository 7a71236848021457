/*
 * dyneval.h — C-ABI of libdyneval_hip.so (MI355X / gfx950, hand-written HIP).
 *
 * This is the drop-in boundary UNDER the reference's Python call convention
 *   eval_fn(args, model, spec, seq_len, overlap, tokenizer, ...)      (reference lcasr/lib.py:450-462,640)
 * The reference has no FFI of its own; each entry point below names the reference line(s)
 * whose arithmetic it replaces.  Conventions shared by every entry:
 *   - extern "C", plain pointers + int64 sizes + float scalars, no torch types;
 *   - every pointer is DEVICE memory owned by the caller (PyTorch is only the allocator), row-major, fp32
 *     unless the name says otherwise; the library never allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return 0 (DYN_OK) or a negative DYN_E_* code; dyn_last_error() gives a thread-local message;
 *   - workspaces are caller-provided; their size comes from the matching *_workspace_bytes() query.
 */
#ifndef DYNEVAL_H_
#define DYNEVAL_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYN_OK 0
#define DYN_E_ARG (-1)       /* bad argument (shape, alignment, null pointer) */
#define DYN_E_LAUNCH (-2)    /* hipLaunch reported an error */
#define DYN_E_WORKSPACE (-3) /* workspace too small */
#define DYN_E_UNSUPPORTED (-4)

const char* dyn_last_error(void);
const char* dyn_version(void);
const char* dyn_arch(void); /* "gfx950" */

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on MFMA (v_mfma_f32_32x32x2_f32): the encoder's QKV / FFN / pointwise-conv / CTC-head
 * products and their dgrad / wgrad — replaces the torch.nn.Linear / Conv1d(k=1) calls inside
 * model(audio_signal=...) (reference lcasr/lib.py:550,603) and inside loss.backward() (lib.py:579).
 *
 *   C[z] = alpha * opA(A[z]) @ opB(B[z]) + beta * C[z] (+ bias[n])       z = z1 * nb2 + z2
 * opA(A) is M x K: trans_a == 0 -> A stored [M, K] (row stride lda); trans_a == 1 -> A stored [K, M].
 * opB(B) is K x N: trans_b == 0 -> B stored [K, N] (row stride ldb); trans_b == 1 -> B stored [N, K].
 * Two-level batch: operand offset = z1 * s?1 + z2 * s?2 (elements) — lets attention heads be addressed
 * inside a [B, T, H*D] activation without a transpose copy.
 * split_k > 1 reduces K-slices through `workspace` in a fixed order (deterministic, no atomics).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t trans_a, trans_b;
    int64_t M, N, K;
    float alpha, beta;
    const float* A; int64_t lda, sa1, sa2;
    const float* B; int64_t ldb, sb1, sb2;
    float* C;       int64_t ldc, sc1, sc2;
    const float* bias;      /* [N] or NULL; added once (after alpha/beta) */
    int64_t nb1, nb2;       /* batch = nb1 * nb2 (>= 1 each) */
    int32_t split_k;        /* 0 = let the planner choose, n >= 1 = force n K-slices over the whole problem */
    void* workspace; int64_t workspace_bytes;
    /* optional forced configuration (0 = planner: tuned table for known shapes, cost model otherwise); used by
     * scripts/tune_gemm.py to time candidates: tile 64|128 x 64|128, tail_slices = K-slices of the last partial
     * round of workgroups (1 = off) */
    int32_t tile_m, tile_n, tail_slices, reserved_;
    /* optional residual source: C = alpha*A@B + beta*C_in (+ bias), C_in addressed exactly like C (same ldc / batch
     * strides); NULL = accumulate in place.  Lets `x_new = x + f(x)` keep x intact for the backward without a copy. */
    const float* C_in;
    /* activation fused into the store of C (v = alpha*A@B + beta*C_in + bias):
     *   0 none;  1 C = silu(v) and, if aux != NULL, aux = v (the pre-activation the backward needs);  2 C = v * silu'(aux)
     * aux is addressed exactly like C.  Replaces the separate SiLU kernels around the FFN products (the `F.silu` between the two
     * FFN linears inside model(audio_signal=...) and its autograd backward, reference lcasr/lib.py:550,579). */
    int32_t epilogue, reserved2_;
    float* aux;
    /* grouped launches only (dyn_gemm_f32_grouped, trans_a): a_colsum[m] = a_colsum_beta * a_colsum[m] + sum_k A(k, m), i.e. the bias
     * gradient of the linear layer whose weight gradient this product is, summed from the A panel the product streams anyway. */
    float* a_colsum;
    float a_colsum_beta, reserved3_;
    /* optional: n_counters int32 arrival counters owned by the caller, ZERO before the first call and left zero by every call
     * (do not share them between streams).  With them the K slices of a split / tail-sliced product are combined inside the
     * kernel by the workgroup that arrives last (slices summed in slice order: same bits as the separate reduce pass, which is
     * used when counters == NULL or there are fewer counters than partial tiles). */
    int32_t* counters;
    int64_t n_counters;
    /* batch strides of `bias` in elements (0, 0 = the same [N] row for every batch): a product batched over SEVERAL WEIGHT MATRICES —
     * the lockstep group of recordings, each with its own adapted weights (sb1 / sb2 step through the weights) — adds each weight's own bias. */
    int64_t bias_s1, bias_s2;
} dyn_gemm_desc;

int64_t dyn_gemm_f32_workspace_bytes(const dyn_gemm_desc* d);
int dyn_gemm_f32(const dyn_gemm_desc* d, void* stream);
/* n <= 96 independent products (same trans flags, no batching / split-K / bias / activation) as ONE launch over all their 128x128
 * tiles: the weight-gradient products of a whole backward pass (`loss.backward()`, reference lcasr/lib.py:579), each of which alone
 * has too few tiles to fill 256 CUs.  `descs` is a HOST array; the descriptor table is rebuilt in `workspace` by a kernel taking it
 * as arguments (hipGraph-capturable).  Outputs must not alias each other.  Deterministic (no atomics, fixed summation order). */
int64_t dyn_gemm_f32_grouped_workspace_bytes(int32_t n);
int dyn_gemm_f32_grouped(const dyn_gemm_desc* descs, int32_t n, void* workspace, int64_t workspace_bytes, void* stream);

/* EXPERIMENTAL (not on the product path): C[M, N] = X[M, K] . W[N, K]^T (+ bias[N]) as an fp32-grade product on the bf16
 * matrix cores — every fp32 operand split into three bf16 terms, six v_mfma_f32_32x32x16_bf16 per fp32 product, fp32 accumulation
 * (the nn.Linear products inside model(audio_signal=...), reference lcasr/lib.py:550).  K % 32 == 0, X / W 16-byte aligned, ldx / ldw
 * multiples of 4, finite operands.  First, unpipelined form (end of round 4): tests/test_zz_experimental_bf16x3_gpu.py holds it to float64 next to
 * dyn_gemm_f32; scripts/emulate_bf16x3_kernel.py is the lane-level CPU emulation of its indexing. */
int dyn_gemm_bf16x3_nt(const float* X, const float* W, const float* bias, float* C, int64_t M, int64_t N, int64_t K, int64_t ldx,
                       int64_t ldw, int64_t ldc, void* stream);
/* The same for C[M, N] = op(A) . op(B) with dyn_gemm_f32's transpose flags (trans_a: A stored [K][M]; trans_b: B stored [N][K]): the linear layer's
 * input gradient is (0, 0), its weight gradient (1, 0) (loss.backward(), reference lcasr/lib.py:579).  Only (0, 1) has run on hardware so far. */
int dyn_gemm_bf16x3(int trans_a, int trans_b, const float* A, const float* B, const float* bias, float* C, int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldb, int64_t ldc, void* stream);
/* EXPERIMENTAL, not yet run on hardware: the weight operand split once (planes = unsigned short [3][rows][K], K contiguous: the three bf16 terms of
 * src [rows][K]) instead of by every workgroup that stages it, and X W^T (+ bias) on those planes (rows = N).  The weights change once per
 * optimiser step (reference lcasr/lib.py:580), so the split is one HBM pass per step. */
int dyn_bf16x3_split(const float* src, void* planes, int64_t rows, int64_t K, int64_t ld, void* stream);
int dyn_gemm_bf16x3_presplit(const float* X, const void* w_planes, const float* bias, float* C, int64_t M, int64_t N, int64_t K, int64_t ldx,
                             int64_t ldc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HBM-bound encoder pieces (activations, norms, softmax, convolutions).  All replace ops inside
 * model(audio_signal=...) (reference lcasr/lib.py:550,603) and its autograd backward (lib.py:579);
 * the architecture constants come from earnings_finetune/lcasr160rb1.yaml:1-29.
 * "beta" arguments accumulate into the destination (dst = result + beta * dst), which is how residual
 * gradients and repeated weight-gradient contributions are summed without extra passes.
 * ------------------------------------------------------------------------------------------------ */
int dyn_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int dyn_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* GLU over the last dim: u [rows, 2C] -> y [rows, C] = u[:, :C] * sigmoid(u[:, C:]) */
int dyn_glu_fwd(const float* u, float* y, int64_t rows, int64_t C, void* stream);
int dyn_glu_bwd(const float* u, const float* dy, float* du, int64_t rows, int64_t C, void* stream);
/* y = a * x + b * y */
int dyn_axpby(const float* x, float* y, float a, float b, int64_t n, void* stream);
/* out[C] = beta * out + sum_rows x[rows, C]   (bias gradients; deterministic two-stage) */
int64_t dyn_colsum_workspace_bytes(int64_t rows, int64_t C);
int dyn_colsum(const float* x, float* out, int64_t rows, int64_t C, float beta, void* workspace, int64_t workspace_bytes,
               void* stream);
int dyn_reduce_partials(const float* partial, float* out, int64_t P, int64_t n, float beta, void* stream);
/* Deferred column reductions.  The reductions that end dyn_layernorm_bwd / dyn_layernorm_bwd_res / dyn_rmsnorm_bwd / dyn_chanaffine_bwd (weight gradients) and
 * dyn_colsum (bias gradients) / dyn_dwconv1d_wgrad, dyn_dwconv2d_s2_wgrad, dyn_sub12_bwd (convolution taps) are launch-bound (~7 us for a few hundred KB, ~55 per window of the adapt step) and nothing reads their
 * outputs before the optimiser step (`loss.backward()` ... `optimizer.step()`, reference lcasr/lib.py:579-581).  Between begin and flush
 * (thread-local, not nestable) those entry points keep their partial sums in `arena` (256-byte aligned, untouched by anything else until
 * the flush) and only RECORD the reduction; flush runs the recorded ones as one launch per 96, each with the per-column summation order
 * of the separate launch, reductions into the same output chained in recording order: bit-identical results.  When the arena is full the
 * entry points fall back to reducing at once.  abort drops the context without launching (error paths). */
int dyn_reduce_defer_begin(void* arena, int64_t arena_bytes);
int dyn_reduce_defer_flush(void* stream);
int dyn_reduce_defer_abort(void);
/* [F, T] (row stride ldx) -> [T, F]: a log-mel window enters the encoder channels-last */
int dyn_transpose_ft(const float* x, float* y, int64_t F, int64_t T, int64_t ldx, void* stream);

/* LayerNorm / RMSNorm over C (C % 256 == 0, C <= 2048); mean/rstd [rows] are saved for the backward. */
int64_t dyn_norm_bwd_workspace_bytes(int64_t rows, int64_t C);
int dyn_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                      int64_t rows, int64_t C, float eps, void* stream);
int dyn_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                      float dx_beta, float* dgamma, float* dbeta, float wgrad_beta, int64_t rows, int64_t C,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* same, out of place: dx = norm_bwd(dy) + dx_beta * dx_in.  The residual-stream gradient of a block gets a NEW buffer per module,
 * so the previous one stays intact as the A operand of the weight-gradient products deferred to the end of the backward
 * (dyn_gemm_f32_grouped). */
int dyn_layernorm_bwd_res(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy,
                          const float* dx_in, float* dx, float dx_beta, float* dgamma, float* dbeta, float wgrad_beta,
                          int64_t rows, int64_t C, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_rmsnorm_fwd(const float* x, const float* gamma, float* y, float* rstd, int64_t rows, int64_t C, float eps,
                    void* stream);
int dyn_rmsnorm_bwd(const float* x, const float* gamma, const float* rstd, const float* dy, float* dx, float dx_beta,
                    float* dgamma, float wgrad_beta, int64_t rows, int64_t C, void* workspace, int64_t workspace_bytes,
                    void* stream);
/* Lockstep-group variants (r04).  Several recordings advance through the same window step in ONE batch, each with its own adapted weights
 * (recordings are independent: fresh optimiser and restored weights per eval_fn call, reference lcasr/lib.py:494,636-637).  `rows` =
 * n_samples * rows_per_sample; sample s takes the parameters of group s % n_groups, the groups' parameters lie param_stride elements apart
 * (the group's flat parameter buffer is [n_groups, n_flat]); weight gradients of group g go to dgamma + g * param_stride (a group's second
 * sample accumulates onto its first).  n_groups = 1 is exactly the plain entry; per sample the arithmetic, the partial-sum layout and the
 * reduction order are those of a plain launch over that sample's rows: bit-identical to running the recordings one by one. */
int64_t dyn_norm_bwd_workspace_bytes_g(int64_t rows, int64_t C, int64_t rows_per_sample);
int dyn_layernorm_fwd_g(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int64_t C,
                        float eps, int64_t rows_per_sample, int64_t n_groups, int64_t param_stride, void* stream);
int dyn_layernorm_bwd_g(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, const float* dx_in,
                        float* dx, float dx_beta, float* dgamma, float* dbeta, float wgrad_beta, int64_t rows, int64_t C,
                        int64_t rows_per_sample, int64_t n_groups, int64_t param_stride, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_rmsnorm_bwd_g(const float* x, const float* gamma, const float* rstd, const float* dy, float* dx, float dx_beta, float* dgamma,
                      float wgrad_beta, int64_t rows, int64_t C, int64_t rows_per_sample, int64_t n_groups, int64_t param_stride,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* BatchRenorm1d in eval mode = per-channel affine with the running statistics (the loop calls model.eval(), reference
 * lcasr/lib.py:525, so they are constants):  y = (x - mean_c) * rsqrt(var_c + eps) * weight_c + bias_c;  x, y [rows, C].
 * bwd: dx = dy * rsqrt(var + eps) * weight (+ dx_beta * dx), dweight += sum_r dy * xhat, dbias += sum_r dy (deterministic). */
int dyn_chanaffine_fwd(const float* x, const float* mean, const float* var, const float* weight, const float* bias, float* y,
                       int64_t rows, int64_t C, float eps, void* stream);
int64_t dyn_chanaffine_bwd_workspace_bytes(int64_t rows, int64_t C);
int dyn_chanaffine_bwd(const float* x, const float* mean, const float* var, const float* weight, const float* dy, float* dx,
                       float dx_beta, float* dweight, float* dbias, float wgrad_beta, int64_t rows, int64_t C, float eps,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Row softmax / log-softmax (row length L <= 16384 fwd, <= 8192 bwd).  softmax_bwd: dx = y*(dy - sum(dy*y))*scale;
 * log_softmax_bwd: dx = dy - exp(y)*sum(dy).  F.log_softmax call sites: reference wav2vec2/lib.py:169,417. */
int dyn_softmax_fwd(const float* x, float* y, int64_t rows, int64_t L, int64_t ldx, int64_t ldy, void* stream);
int dyn_softmax_bwd(const float* y, const float* dy, float* dx, int64_t rows, int64_t L, int64_t ld, float scale,
                    void* stream);
/* Key-length masked softmax (the attention of a zero-padded utterance bucket, wav2vec2_model.py; HF passes no attention mask to
 * wav2vec2-base, reference wav2vec2/lib.py:413, so an utterance attends to exactly its own frames): `valid_cols` is a DEVICE int32
 * scalar read when the kernel runs; columns >= *valid_cols are outside the max / sum and get probability 0, the first *valid_cols
 * values are bit for bit those of a row of that length. */
int dyn_softmax_fwd_len(const float* x, float* y, int64_t rows, int64_t L, int64_t ldx, int64_t ldy, const int32_t* valid_cols,
                        void* stream);
int dyn_log_softmax_fwd(const float* x, float* y, int64_t rows, int64_t L, int64_t ldx, int64_t ldy, void* stream);
int dyn_log_softmax_bwd(const float* y, const float* dy, float* dx, int64_t rows, int64_t L, int64_t ld, void* stream);
/* Gradient of the mean categorical entropy w.r.t. the log-probabilities (the `entropy_augmentation` input perturbation,
 * reference lcasr/lib.py:86-99): grad[r, c] = -p (y + H_r) * scale, H_r = -sum p y; entropy_per_row optional. */
int dyn_entropy_grad(const float* log_probs, float* grad, float* entropy_per_row, int64_t rows, int64_t L, int64_t ld,
                     float scale, void* stream);

/* Depthwise Conv1d over time, channels-last x [B, T, C], w [C, KW], 'same' zero padding (conformer conv module,
 * `conv_kernel_size: 9`, yaml:15).  KW in {3,5,7,9,15,31}. */
int dyn_dwconv1d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t T, int64_t C,
                     int64_t KW, void* stream);
int dyn_dwconv1d_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW,
                       float dx_beta, void* stream);
int64_t dyn_dwconv1d_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW);
int dyn_dwconv1d_wgrad(const float* x, const float* dy, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t C,
                       int64_t KW, void* workspace, int64_t workspace_bytes, void* stream);
/* lockstep-group variants (see dyn_layernorm_fwd_g): sample b convolves with / accumulates into the filters of replica b % n_groups */
int dyn_dwconv1d_dgrad_g(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                         int64_t n_groups, int64_t param_stride, void* stream);
int dyn_dwconv1d_wgrad_g(const float* x, const float* dy, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                         int64_t n_groups, int64_t param_stride, void* workspace, int64_t workspace_bytes, void* stream);

/* Fused conformer conv-module core (GLU -> depthwise k=9 -> RMSNorm | LayerNorm over channels -> SiLU), one pass:
 *   u [B, T, 2C] -> s [B, T, C];  optional outputs for the backward: g (GLU), c (conv), nn (norm output), mean, rstd [B*T].
 * C in {256, 512, 768, 1024}, kernel width 9. */
int dyn_convmod_fwd(const float* u, const float* w, const float* bias, const float* gamma, const float* beta, float* s,
                    float* g_out, float* c_out, float* nn_out, float* mean_out, float* rstd_out, int64_t B, int64_t T, int64_t C,
                    int64_t KWIDTH, int32_t layernorm, float eps, void* stream);
/* lockstep-group variant (see dyn_layernorm_fwd_g): sample b of the batch takes w / bias / gamma / beta of replica b % n_groups */
int dyn_convmod_fwd_g(const float* u, const float* w, const float* bias, const float* gamma, const float* beta, float* s, float* g_out,
                      float* c_out, float* nn_out, float* mean_out, float* rstd_out, int64_t B, int64_t T, int64_t C, int64_t KWIDTH,
                      int32_t layernorm, float eps, int64_t n_groups, int64_t param_stride, void* stream);

/* dw_striding x8 subsampling (`subsampling: dw_striding`, `subsampling_conv_channels: 256`, `subsampling_act: silu`,
 * yaml:10-13), channels-last.  Output sizes: To = (T-1)/2+1, Fo = (F-1)/2+1 (3x3, stride 2, pad 1).
 *   conv2d_first: x [B,T,F] (1 channel) -> z [B,To,Fo,C], w [C,3,3]
 *   dwconv2d_s2 : u = bias + dw3x3_s2(silu(z)),  z [B,T,F,C] -> u [B,To,Fo,C]   (SiLU fused into the load)
 * The 1x1 pointwise convs between them are dyn_gemm_f32 calls. */
int dyn_conv2d_first_fwd(const float* x, const float* w, const float* bias, float* z, int64_t B, int64_t T, int64_t F,
                         int64_t C, void* stream);
/* input gradient of conv2d_first (needed only by the entropy-gradient input perturbation, reference lib.py:96) */
int dyn_conv2d_first_dgrad(const float* dz, const float* w, float* dx, int64_t B, int64_t T, int64_t F, int64_t C,
                           void* stream);
int64_t dyn_conv2d_wgrad_workspace_bytes(int64_t B, int64_t To, int64_t C);
int dyn_conv2d_first_wgrad(const float* x, const float* dz, float* dw, float* dbias, float beta, int64_t B, int64_t T,
                           int64_t F, int64_t C, void* workspace, int64_t workspace_bytes, void* stream);
/* The first two subsampling stages FUSED: u2 = bias2 + dw3x3_s2(silu(bias1 + conv3x3_s2(x))), x [B, T, F] one channel ->
 * u2 [B, T2, F2, C] (T1 = (T - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1, same for F).  The [B, T1, F1, C] intermediate (671 MB at B = 2,
 * T = 16384: the largest activation of the model) and its gradient never exist: forward and backward recompute it from x
 * (reference: upstream SCConformerXL `subsampling` reached through model(audio_signal=...) and loss.backward(), lcasr/lib.py:550,579).
 * dyn_sub12_bwd accumulates dw1 [C, 3, 3], db1 [C], dw2 [C, 3, 3], db2 [C] (beta * old + new) from du2; deterministic. */
int dyn_sub12_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* u2, int64_t B, int64_t T,
                  int64_t F, int64_t C, void* stream);
int64_t dyn_sub12_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C);
int dyn_sub12_bwd(const float* x, const float* du2, const float* w1, const float* b1, const float* w2, float* dw1, float* db1, float* dw2,
                  float* db2, float beta, int64_t B, int64_t T, int64_t F, int64_t C, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_dwconv2d_s2_fwd(const float* z, const float* w, const float* bias, float* u, int64_t B, int64_t T, int64_t F,
                        int64_t C, void* stream);
int dyn_dwconv2d_s2_dgrad(const float* z, const float* w, const float* du, float* dz, int64_t B, int64_t T, int64_t F,
                          int64_t C, void* stream);
int dyn_dwconv2d_s2_wgrad(const float* z, const float* du, float* dw, float* dbias, float beta, int64_t B, int64_t T,
                          int64_t F, int64_t C, void* workspace, int64_t workspace_bytes, void* stream);

/* Rotary position embedding, in place on the first n_heads*D floats of each row of x ([B*T] rows of row_stride floats);
 * cos/sin tables are [T, D/2]; inverse != 0 applies the transpose (the backward). yaml:22,28. */
int dyn_rotary(float* x, const float* cos_table, const float* sin_table, int64_t B, int64_t T, int64_t n_heads, int64_t D,
               int64_t row_stride, int32_t inverse, void* stream);

/* SpecAugment frequency masks on a [F, T] log-mel window, in place: rows f0[k] <= f < f0[k]+width[k] := value.
 * Replaces lcasr.utils.augmentation.SpecAugment as called at reference lcasr/lib.py:499,541 (mask positions are
 * drawn on the host so the RNG stream stays the caller's).  value_dev (nullable) overrides `value` with a DEVICE scalar,
 * e.g. the window mean produced by dyn_moments, so the fill value never makes a host round trip. */
int dyn_specaug_freqmask(float* x, int64_t F, int64_t T, const int32_t* f0, const int32_t* width, int64_t n_masks,
                         float value, const float* value_dev, void* stream);
int dyn_specaug_timemask(float* x, int64_t F, int64_t T, const int32_t* t0, const int32_t* width, int64_t n_masks,
                         float value, const float* value_dev, void* stream);

/* Same masking with the (start, width) pairs passed by value as kernel arguments: start_host / width_host are HOST arrays
 * (n_masks <= 32) read at launch time, so the per-window loop has no device index buffer and no blocking
 * host-to-device copy (a pageable copy would make the host wait for the previous window's backward). */
int dyn_specaug_mask_args(float* x, int64_t F, int64_t T, const int32_t* start_host, const int32_t* width_host, int64_t n_masks,
                          int32_t along_time, float value, const float* value_dev, void* stream);

/* Log-mel front end (upstream lcasr.utils.audio_tools.processing_chain, called by the dataset adapters: reference
 * lcasr/earnings22/run.py:61, tedlium/run.py:94, chime6/run.py:61-68).  The STFT itself is a dyn_gemm_f32 call on the
 * reflect-padded signal with lda = hop < K (overlapping rows) and a window-folded DFT basis; these are the passes
 * around it:  reflect pad -> [GEMM: re|im] -> power -> [GEMM: mel] -> log + per-bin (mean, std) -> normalise + transpose.
 *   dyn_stft_power     reim [T, 2*KP] (re | im) -> power [T, KP]
 *   dyn_logmel_finish  mel [T, F] (overwritten by log(mel + eps)) -> out [F, T], optionally per-bin normalised over T: the mean, then the
 *                      centred sum of squares in a second pass (never E[x^2] - mean^2), fixed summation order; a bin of zero variance,
 *                      and T == 1, give zeros.  F <= 256; workspace 8-byte aligned, dyn_logmel_finish_workspace_bytes(T, F) bytes. */
int dyn_reflect_pad(const float* x, float* out, int64_t n, int64_t pad, void* stream);
int dyn_stft_power(const float* reim, float* power, int64_t T, int64_t KP, void* stream);
int64_t dyn_logmel_finish_workspace_bytes(int64_t T, int64_t F);
int dyn_logmel_finish(float* mel, float* out, int64_t T, int64_t F, float eps, int32_t normalize, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* (x - mean_row) / std_row (unbiased) of a [R, T] spectrogram: the renormalisation after the CHiME-6 channel average
 * (reference lcasr/chime6/run.py:66-68).  In place when out == x. */
int dyn_rownorm(const float* x, float* out, int64_t R, int64_t T, void* stream);

/* Optional Loop-A augmentations on a device-resident [F, T] window (random draws stay on the host):
 *   dyn_gather_frames  frame_shuffle (reference lcasr/lib.py:81-84): y = x[:, index] (along_time) or x[index, :]
 *   dyn_moments        (sum, mean, unbiased std) of a buffer — spec.std() of add_random_noise (lib.py:379-382)
 *   dyn_cutout         cutout (lib.py:384-417): rects [n, 4] = (y0, y1, x0, x1); mode 0 zero, 1 own mean, 2 constant */
int dyn_gather_frames(const float* x, const int32_t* index, float* y, int64_t F, int64_t T, int32_t along_time, void* stream);
int64_t dyn_moments_workspace_bytes(void);
int dyn_moments(const float* x, int64_t n, float* out3, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_cutout(float* x, int64_t F, int64_t T, const int32_t* rects, int64_t n_rects, int32_t mode, float value,
               float* means_scratch, void* stream);

/* Device-side delay of `microseconds` on `stream` (one wave polling the 100 MHz realtime counter): starts the recording chains of
 * lib.dynamic_eval_many out of phase.  No reference counterpart (the reference runs one recording at a time,
 * run_dynamic_eval_full.py:84-100); scheduling aid only, computes nothing. */
int dyn_sleep_us(int64_t microseconds, void* stream);
/* A HIP stream restricted to the compute units set in `mask` (bit i of word i / 32 = CU i, hipExtStreamCreateWithCUMask), and its
 * destruction.  lib.dynamic_eval_many can run its recording chains on such streams (DYN_CHAIN_CU_MASK=<hole size>): chain k's kernels
 * then leave a different group of CUs free, on which the short kernels of the other chains can start while a matrix kernel of chain k
 * owns the rest of the chip.  No reference counterpart; scheduling aid only (A/B result in DESIGN.md §5). */
int dyn_stream_create_cu_mask(const uint32_t* mask, int32_t n_words, void** stream_out);
int dyn_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused self-attention forward for no-grad passes (reference lcasr/lib.py:603: the final pass runs model(audio_signal) under
 * torch.no_grad(); also every epochs = 0 evaluation): out = softmax(q k^T * scale) v per (batch, head), fp32, online softmax,
 * K/V tiles staged in LDS — the [T, T] scores never reach HBM.  q / k / v are views of [B, T, .] activations with a common row
 * and batch stride (the packed QKV activation: three base pointers), head h at +h * head_dim; head_dim must be 128.
 * ------------------------------------------------------------------------------------------------ */
int dyn_attention_fwd(const float* q, const float* k, const float* v, float* out, int64_t B, int64_t T, int64_t H,
                      int64_t head_dim, int64_t row_stride, int64_t batch_stride, int64_t out_row_stride,
                      int64_t out_batch_stride, float scale, void* stream);
/* Grad-mode variant (the B = 2 forward of every adapt step, reference lcasr/lib.py:550): same kernel, additionally writes
 * lse [B, H, T] = log sum_j exp(scale * q_i k_j) per query row — all the backward needs to re-form the probabilities. */
int dyn_attention_fwd_lse(const float* q, const float* k, const float* v, float* out, float* lse, int64_t B, int64_t T, int64_t H,
                          int64_t head_dim, int64_t row_stride, int64_t batch_stride, int64_t out_row_stride,
                          int64_t out_batch_stride, float scale, void* stream);
/* The same forward with the KEYS split over `nsplit` workgroups per query block (0 = chosen from the launch size, 1 = no split,
 * at most 8): each split writes a normalised partial output and its log-sum-exp to `workspace`, a second kernel merges them in
 * split order (deterministic).  For launches whose (batch, head, query-block) workgroups do not fill the chip: the B = 4 final-pass
 * launch at T' = 2048 (384 workgroups on 512 slots) and every B = 1 inference.  `lse` may be NULL. */
int64_t dyn_attention_fwd_split_workspace_bytes(int64_t B, int64_t T, int64_t H, int32_t nsplit);
int dyn_attention_fwd_split(const float* q, const float* k, const float* v, float* out, float* lse, int64_t B, int64_t T, int64_t H,
                            int64_t head_dim, int64_t row_stride, int64_t batch_stride, int64_t out_row_stride, int64_t out_batch_stride,
                            float scale, int32_t nsplit, void* workspace, int64_t workspace_bytes, void* stream);
/* Backward of the fused attention (`loss.backward()`, reference lcasr/lib.py:579, through softmax(q k^T) v): dq / dk / dv from
 * (q, k, v, out, dout, lse), recomputing P tile by tile from LDS-staged tiles — no [T, T] matrix is read or written.
 * Deterministic (no float atomics): query-owner workgroups produce dq and delta [B, H, T] (scratch: rowsum(dout * out)), then
 * key-owner workgroups produce dk and dv.  dout / out share (out_row_stride, out_batch_stride); dq / dk / dv share
 * (grad_row_stride, grad_batch_stride) — e.g. the three thirds of a packed [B, T, 3 * H * 128] gradient buffer. */
int dyn_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse,
                      float* delta, float* dq, float* dk, float* dv, int64_t B, int64_t T, int64_t H, int64_t head_dim,
                      int64_t row_stride, int64_t batch_stride, int64_t out_row_stride, int64_t out_batch_stride,
                      int64_t grad_row_stride, int64_t grad_batch_stride, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder-decoder `teacher_ce` adaptation (reference lcasr/lib.py:1228-1322 calc_loss_enc_dec, :1475-1732 enc_dec_dynamic_eval):
 * the decoder's dense work runs on dyn_gemm_f32 and the encoder's norm / softmax kernels; these are the pieces that are new.
 *   dyn_embedding_fwd  out[s] = table[ids[s]] (+ pos[s % pos_period])            token embedding (+ fixed positional table)
 *   dyn_embedding_bwd  dtable[v] = beta * dtable[v] + sum_{s: ids[s] == v} dy[s]  one workgroup per vocabulary row, no atomics
 *   dyn_causal_mask    scores[b, r, c] = -inf for c > r                            decoder self-attention (before dyn_softmax_fwd)
 *   dyn_nll_loss       F.cross_entropy(reduction='sum', ignore_index) on log-softmax rows (lib.py:1290-1296): loss [1], the per-row
 *                      terms, and grad = grad_scale * (exp(logp) - onehot(target)) w.r.t. the LOGITS (0 for ignored rows)
 * ------------------------------------------------------------------------------------------------ */
/* ids[r] = argmax_c x[r, c] (first maximum wins, as torch.argmax), vals[r] = that maximum (may be NULL): the greedy step of the
 * autoregressive decode (`model.generate`, reference lcasr/lib.py:1128,1580) and the teacher's mean max-probability (:1601). */
int dyn_argmax_rows(const float* x, int64_t rows, int64_t C, int64_t ld, int32_t* ids, float* vals, void* stream);
int dyn_embedding_fwd(const int32_t* ids, const float* table, const float* pos, float* out, int64_t S, int64_t d, int64_t vocab,
                      int64_t pos_period, void* stream);
int dyn_embedding_bwd(const int32_t* ids, const float* dy, float* dtable, int64_t S, int64_t d, int64_t vocab, float beta,
                      void* stream);
int dyn_causal_mask(float* scores, int64_t nb, int64_t S, void* stream);
int dyn_nll_loss(const float* log_probs, const int32_t* targets, float* loss, float* row_loss, float* grad, int64_t rows, int64_t C,
                 int32_t ignore_index, float grad_scale, void* stream);
/* Row-weighted form, the policy-gradient loss of the RL modes (update_grpo / update_maxrl, reference lcasr/lib.py:1400-1472, where
 * the weight of a token row of rollout j is A_j / (n_j * R) resp. A_j / sum(mask)): loss = sum_r w[r] * (-logp[r, target[r]]),
 * row_loss[r] = that term, grad[r, :] = w[r] * (exp(logp[r, :]) - onehot(target[r])); fixed reduction order.  A target outside
 * [0, C) is an argument the caller must not pass: such a row contributes nothing. */
int dyn_nll_loss_weighted(const float* log_probs, const int32_t* targets, const float* weights, float* loss, float* row_loss, float* grad,
                          int64_t rows, int64_t C, void* stream);
/* Counter-based randomness of the teacher_ce path (no device RNG state, a draw is a pure function of (seed, stream, index)):
 *   z = splitmix64_finish(seed ^ (stream + 1) * 0x9E3779B97F4A7C15 ^ (index + 1) * 0xC2B2AE3D27D4EB4F)
 *   dropout:  keep element i iff (z >> 40) * 2^-24 >= p;  y = keep ? x * 1 / (1 - p) : 0   (in place allowed; the backward is the same
 *             call on the gradient).  Replaces nn.Dropout of `language_model_decoder.dropout_emb / ff_out_dropout` and the attention
 *             `dropout_p` the reference switches on around the supervised step (lcasr/lib.py:1511-1522,1636-1637,1703-1707).
 *   sampling: ids[r] = argmax_c (x[r, c] * inv_temperature + g), g = -log(-log(u)), u = (2 * (z >> 41) + 1) * 2^-24 with
 *             stream = step0 + r, index = c  (Gumbel-max = a draw from softmax(x / temperature)): `model.generate(sample=True,
 *             temperature=...)` of the decode-agreement filter (lcasr/lib.py:1620-1627). */
int dyn_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
int dyn_gumbel_argmax_rows(const float* x, int64_t rows, int64_t C, int64_t ld, float inv_temperature, uint64_t seed, uint64_t step0,
                           int32_t* ids, void* stream);

/* The autoregressive decode of `model.generate` (reference call sites lcasr/lib.py:1128,1579-1582,1620-1625; the model class itself
 * is un-vendored) one token at a time with cached keys / values: ONE call runs `n_steps` consecutive positions t0 .. t0 + n_steps - 1
 * as 8 * layers + 2 lean launches per token (a row-times-matrix kernel with the LayerNorm / embedding prologue and the bias / SiLU /
 * residual epilogue fused, and a one-query attention kernel per head), instead of ~57 launches of the tile kernels at M = 1.
 * Per position t: x = embed[tokens[t]] + pos_table[t]; per layer: self-attention over cache rows 0 .. t (row t = the packed q | k | v
 * of this position, written here), cross-attention over the n_enc projected encoder rows, SiLU feed-forward; then
 * logits = head(norm_out(x)) and tokens[t + 1] = argmax (sample == 0, first maximum wins) or the Gumbel-max draw of
 * dyn_gumbel_argmax_rows with stream = step0 + t (sample != 0).  Nothing is read back: the caller looks for eos when it likes.
 * layer_ptrs: HOST array of layers * DYN_DEC_PTRS_PER_LAYER device pointers, per layer in this order:
 *   self.norm.weight, self.norm.bias, self.qkv.weight [3d, d], self.qkv.bias, self.out.weight [d, d], self.out.bias,
 *   cross.norm.weight, cross.norm.bias, cross.q.weight [d, d], cross.q.bias, cross.out.weight [d, d], cross.out.bias,
 *   ff.norm.weight, ff.norm.bias, ff.w1.weight [d_ff, d], ff.w2.weight [d, d_ff],
 *   cache [>= t0 + n_steps rows, 3d] (read / written), cross_kv [n_enc, 2d] (keys | values of the encoder states).
 * Limits: d_model % 256 == 0, d_model <= 2048, d_ff % 256 == 0, d_ff <= 2048, head dim a power of two in 4 .. 256,
 * t0 + n_steps <= max_positions, keys per attention <= 49152. */
#define DYN_DEC_PTRS_PER_LAYER 18
typedef struct {
    int32_t d_model, heads, d_ff, vocab, layers, n_enc, max_positions, reserved_;
    float eps, reserved2_;
    const float* embed;        /* [vocab, d] */
    const float* pos_table;    /* [max_positions, d] */
    const float* norm_out_w;
    const float* norm_out_b;
    const float* head_w;       /* [vocab, d] */
    const float* head_b;
    const void* const* layer_ptrs;
    int32_t* tokens;           /* device, >= t0 + n_steps + 1 entries; tokens[t0] must be valid on entry */
    float* logits;             /* device [vocab]: the logits of the last position run */
    float* scratch;            /* device, >= 6 * d_model + d_ff + 16 * heads floats */
    int64_t scratch_floats;
} dyn_decoder_desc;
int dyn_decoder_steps(const dyn_decoder_desc* d, int32_t t0, int32_t n_steps, int32_t sample, float inv_temperature, uint64_t seed,
                      uint64_t step0, void* stream);

/* The same decode for `rows` (1 .. 8) sequences over the SAME encoder states, one position per step for all of them: the sampled
 * rollouts of the RL modes (`generate_enc_dec(sample=4, greedy=False)`, reference lcasr/lib.py:1172-1226,1665-1671).  The launch
 * count per token is that of dyn_decoder_steps; every row-times-matrix kernel reads a weight row ONCE and applies it to all rows of a
 * group of four, each row's dot product accumulated in the single-row kernel's order (a row's logits are bit-identical to
 * dyn_decoder_steps on that row alone).  `base` describes row 0; row r lives at
 *   tokens + r * token_stride, layer cache + r * cache_stride, logits + r * vocab, scratch + r * (scratch_floats / rows);
 * the cross-attention keys / values (layer pointer 17) are shared.  Row r draws with seed + r, stream step0 + t.
 * finished[r] != 0 on entry or set here when row r draws `eos_id`: from then on the row runs no kernel work, writes nothing to its
 * cache and every later token slot of it receives eos_id.  The caller reads `finished` / the tokens back when it likes.
 * base.scratch_floats >= rows * dyn_decoder_row_scratch_floats(d_model, d_ff, heads); token_stride > t0 + n_steps;
 * cache_stride >= (t0 + n_steps) * 3 * d_model; cache_stride and the per-row scratch are multiples of 4 floats. */
typedef struct {
    dyn_decoder_desc base;
    int32_t rows, eos_id;
    int64_t token_stride;      /* int32 entries between the token buffers of consecutive rows */
    int64_t cache_stride;      /* floats between the self-attention caches of consecutive rows (every layer) */
    int32_t* finished;         /* device [rows] */
} dyn_decoder_batch_desc;
int64_t dyn_decoder_row_scratch_floats(int64_t d_model, int64_t d_ff, int64_t heads);
int dyn_decoder_steps_batch(const dyn_decoder_batch_desc* d, int32_t t0, int32_t n_steps, int32_t sample, float inv_temperature,
                            uint64_t seed, uint64_t step0, void* stream);

/* The cached greedy decode of CohereAsrForConditionalGeneration.generate(do_sample=False) (transformers modeling_cohere_asr.py:
 * CohereAsrDecoder.forward with past_key_values, CohereAsrDecoderLayer.forward, CohereAsrSelfAttention / CohereAsrCrossAttention,
 * CohereAsrDecoderMLP, `proj_out`, and GenerationMixin's greedy loop: argmax, eos bookkeeping, pad fill) for `rows` (1 .. 8) sequences,
 * one position per step for all of them, n_steps positions t0 .. t0 + n_steps - 1 per call, 10 * layers + 2 launches per position.
 * Per position t and live row r: x = embedding_layernorm(embed[tokens[r][t]] + pos_emb[t]); per layer the pre-LN blocks
 *   x += o(self-attention of q | k | v(input_layernorm(x)) over cache rows 0 .. t; row t is written here),
 *   x += o(cross-attention of q(post_attention_layernorm(x)) over the row's n_enc precomputed keys | values),
 *   x += fc2(relu(fc1(final_layernorm(x))));
 * logits[r] = head(norm(x)); tokens[r][t + 1] = the first maximum.  A row that picks eos_id is marked in `finished`; a finished row
 * (on entry or marked here) runs no work, writes no cache row and receives pad_id in every later slot.  For t + 1 < n_forced slot
 * t + 1 already holds the forced prompt: it is left alone and the head is not run.
 * Every row-times-matrix kernel reads each weight element once per position and applies it to all rows held in registers, K split over
 * the four waves of a workgroup and merged in wave order (no atomics); row r's numbers do not depend on `rows` or on its neighbours.
 * Row r lives at tokens + r * token_stride, layer cache + r * cache_stride, cross_kv + r * cross_stride, logits + r * vocab,
 * scratch + r * dyn_seq2seq_row_scratch_floats(d_model, d_ff, heads).
 * layer_ptrs: HOST array of layers * DYN_S2S_PTRS_PER_LAYER device pointers (16-byte aligned), per layer in this order:
 *   input_layernorm.weight, .bias, self q | k | v weight [3d, d], bias [3d], self o_proj.weight [d, d], .bias,
 *   post_attention_layernorm.weight, .bias, cross q_proj.weight [d, d], .bias, cross o_proj.weight [d, d], .bias,
 *   final_layernorm.weight, .bias, fc1.weight [d_ff, d], .bias, fc2.weight [d, d_ff], .bias,
 *   cache [>= t0 + n_steps rows, 3d] of row 0 (read / written), cross_kv [n_enc, 2d] of row 0 (keys | values).
 * Limits: d_model and d_ff multiples of 256 up to 4096, head dim a power of two in 4 .. 256, t0 + n_steps <= max_positions, keys per
 * attention <= 49152, token_stride > t0 + n_steps, cache_stride >= (t0 + n_steps) * 3 d, cross_stride >= n_enc * 2 d (both multiples
 * of 4), scratch_floats >= rows * the per-row count.  DYN_E_ARG / DYN_E_UNSUPPORTED / DYN_E_WORKSPACE, nothing launched. */
#define DYN_S2S_PTRS_PER_LAYER 20
typedef struct {
    int32_t d_model, heads, d_ff, vocab, layers, n_enc, max_positions, rows;
    int32_t pad_id, eos_id;
    float eps, reserved_;
    const float* embed;        /* [vocab, d] */
    const float* pos_emb;      /* [max_positions, d] */
    const float* emb_ln_w;     /* embedding_layernorm */
    const float* emb_ln_b;
    const float* norm_w;       /* the final norm */
    const float* norm_b;
    const float* head_w;       /* proj_out [vocab, d] */
    const float* head_b;
    const void* const* layer_ptrs;
    int32_t* tokens;           /* device; row r: >= t0 + n_steps + 1 entries, slot t0 (and the forced prompt) valid on entry */
    int32_t* finished;         /* device [rows] */
    float* logits;             /* device [rows, vocab]: the logits of the last position whose head ran */
    float* scratch;
    int64_t scratch_floats;
    int64_t token_stride;      /* int32 entries between the token buffers of consecutive rows */
    int64_t cache_stride;      /* floats between the self-attention caches of consecutive rows (every layer) */
    int64_t cross_stride;      /* floats between the cross-attention keys | values of consecutive rows (every layer) */
} dyn_seq2seq_desc;
int64_t dyn_seq2seq_row_scratch_floats(int64_t d_model, int64_t d_ff, int64_t heads);
int dyn_seq2seq_steps(const dyn_seq2seq_desc* d, int32_t t0, int32_t n_steps, int32_t n_forced, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC.  dyn_ctc_greedy replaces GreedyCTCDecoder on a CPU copy of the posteriors (reference lcasr/lib.py:498,
 * 559,565; run_dynamic_eval_full.py:53,100): argmax over classes (first maximum), collapse repeats, drop `blank`.
 *   log_probs [B*T rows, C] (row stride ld); argmax_ids [B*T]; out_ids [B, T] (prefix of out_len[b] valid ids).
 * dyn_ctc_loss replaces torch.nn.CTCLoss(blank, reduction) forward + backward (reference lcasr/lib.py:492,575,579;
 * wav2vec2/lib.py:351,434): log_probs[t, b, c] at t*lp_stride_t + b*lp_stride_b + c; targets [B, S_max] int32;
 * reduction 0 = 'sum' (loss = sum_b nll_b, grad scaled by grad_scale), 1 = 'mean' (nll_b / max(S_b,1), mean over B).
 * grad (optional) gets torch's native gradient w.r.t. log_probs, same addressing with g_stride_*.
 * Rounding contract (r04): every exp / log of the lattice and the gradient is glibc's expf / logf bit for bit (csrc/libm_f32.h), every
 * add / subtract one fp32 operation in the order of aten/native/LossCTC.cpp's CPU kernel, the per-class log-sum pairwise in descending
 * lattice position: on identical log_probs the nll, alpha, beta and gradient are bit-identical to torch's CPU CTC.
 * dyn_ctc_loss_workspace_layout: byte offsets of {gathered slab, alpha, beta, nll} inside the workspace and the lattice row length
 * L = 2 * max(S_max, 1) + 1 (alpha / beta are [B, T, L] fp32) — lets a caller or a test read the lattice a dyn_ctc_loss call left behind.
 * dyn_libm_f32: y_exp[i] = expf(x[i]), y_log[i] = logf(x[i]), y_exp_nonpos[i] = the branch-free x <= 0 variant the lattice uses
 * (any output may be NULL): the device build of csrc/libm_f32.h, for comparison with the host's libm.
 * ------------------------------------------------------------------------------------------------ */
int dyn_ctc_greedy(const float* log_probs, int64_t B, int64_t T, int64_t C, int64_t ld, int32_t blank, int32_t* argmax_ids,
                   int32_t* out_ids, int32_t* out_len, void* stream);
int64_t dyn_ctc_loss_workspace_bytes(int64_t T, int64_t B, int64_t S_max);
int dyn_ctc_loss_workspace_layout(int64_t T, int64_t B, int64_t S_max, int64_t* offsets4, int64_t* row_len);
int dyn_libm_f32(const float* x, int64_t n, float* y_exp, float* y_log, float* y_exp_nonpos, void* stream);
int dyn_ctc_loss(const float* log_probs, int64_t T, int64_t B, int64_t C, int64_t lp_stride_t, int64_t lp_stride_b,
                 const int32_t* targets, int64_t S_max, const int32_t* input_lengths, const int32_t* target_lengths,
                 int32_t blank, int32_t reduction, float grad_scale, float* loss, float* nll_per_sample, float* grad,
                 int64_t g_stride_t, int64_t g_stride_b, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused adaptation step over a flat fp32 parameter buffer (`optimizer.step()`, reference lcasr/lib.py:581).
 * `step` is the 0-based count of previous steps; step == 0 initialises the state in-kernel (fresh optimiser per
 * eval_fn call, lib.py:494).  MADGRAD follows facebookresearch/madgrad (lr+eps, cube-root denominator, momentum
 * as an average of the dual-averaged iterate); Adam follows torch.optim.Adam (reference nvidia_ctc/lib.py:43).
 * dyn_clip_grad_norm = torch.nn.utils.clip_grad_norm_ (reference wav2vec2/lib.py:442); norm_and_coef: 2 floats.
 * ------------------------------------------------------------------------------------------------ */
int dyn_madgrad_step(float* params, const float* grads, float* grad_sum, float* grad_sum_sq, float* x0, int64_t n, float lr,
                     float momentum, float weight_decay, float eps, int64_t step, void* stream);
int dyn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, void* stream);
int64_t dyn_clip_grad_norm_workspace_bytes(int64_t n);
int dyn_clip_grad_norm(float* grads, int64_t n, float max_norm, float* norm_and_coef, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The consistency loop (reference lcasr/lib.py:646-903): one parameter set and one gradient per window.
 * dyn_grad_mix_decay: in-place distance-decayed mix of a gradient bank grads[n_windows][row_stride] (reference :817-841), for
 * i = 0 .. n_windows-1 IN THIS ORDER (rows q < i are read already mixed):
 *   grads[i] <- fl32( ( f64(grads[i]) + sum_{q != i, ascending q} f64(fl32(fl32(decay[|i-q|]) * grads[q])) ) / denom[i] )
 * bit-identical to the reference's torch statements.  `ranges`: HOST array of n_ranges [lo, hi) element ranges of a row that are
 * mixed (elements outside are not touched: parameters without a gradient); `decay` / `denom`: DEVICE arrays of n_windows doubles,
 * decay[k] = 0.95 ** k and denom[i] = the reference's `total_sum` of window i, both formed on the host.  The windows of an element
 * are staged in LDS: at most dyn_grad_mix_decay_max_windows() windows, more is DYN_E_ARG.
 * dyn_adafactor_step: torch.optim.Adafactor's single-tensor rule (maximize=False) over a flat buffer.  `segments`: DEVICE table of
 * n_segments x 9 int64 per tensor {offset, batch, rows, cols, state offset, factored, first row, first batch, first factored column}:
 * a tensor of dimension >= 2 is batch x rows x cols (its last two dimensions) with row_var [batch * rows] then col_var [batch * cols] at
 * `state offset` of `state`; a 1-D tensor is 1 x 1 x n, not factored, with variance [n] there.  first row / batch / factored column are
 * the running sums of batch * rows, batch and (factored only) batch * cols over the table; n_rows, n_batches, n_factored_cols their
 * totals.  `step` counts from 1 (torch's step_t after the increment); a fresh state is all zeros.  Six launches whatever the number of
 * tensors; every reduction runs in a fixed order, so a step is reproducible bit for bit.  `scratch`: dyn_adafactor_scratch_bytes().
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_grad_mix_decay_max_windows(void);
int dyn_grad_mix_decay(float* grads, int64_t row_stride, int32_t n_windows, const int64_t* ranges, int32_t n_ranges,
                       const double* decay, const double* denom, void* stream);
int64_t dyn_adafactor_scratch_bytes(int64_t n_rows, int64_t n_batches, int64_t n_segments);
int dyn_adafactor_step(float* params, const float* grads, float* state, const int64_t* segments, int32_t n_segments,
                       int64_t n_rows, int64_t n_batches, int64_t n_factored_cols, double lr, double beta2_decay, double eps1,
                       double eps2, double d, double weight_decay, int64_t step, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Window stitching on device (reference lcasr/lib.py:583-589,604-609,615-629): acc[pos+r, c] += exp(lp[r, c]),
 * count[pos+r] += 1, then out = log(acc / count) over the covered prefix.
 * ------------------------------------------------------------------------------------------------ */
int dyn_stitch_accumulate(const float* log_probs, int64_t ld, float* acc, float* count, int64_t pos, int64_t rows, int64_t C,
                          int64_t acc_rows, void* stream);
int dyn_stitch_finalize(const float* acc, const float* count, float* out, int64_t rows, int64_t C, void* stream);
/* Same for an accumulator whose coverage has gaps (outer leave-one-out stitching, reference
 * lcasr/run_within_recording_loo_eval.py:160-181): out[r] = log(acc[row_index[r]] / count[row_index[r]]), row_index int64 on device. */
int dyn_stitch_finalize_rows(const float* acc, const float* count, const int64_t* row_index, float* out, int64_t rows, int64_t C,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * wav2vec2 encoder pieces (reference wav2vec2/lib.py:20-23 loads HF Wav2Vec2ForCTC; forward at :163,413, backward at
 * :194,437).  The strided Conv1d feature extractor and the grouped positional conv are dyn_gemm_f32 calls over
 * OVERLAPPING rows of channels-last activations (lda = stride * C_in < K = kernel * C_in); these are the passes around
 * them.  Layouts: activations [B, T, C]; conv weights [C_out][kernel][C_in]; positional conv v / w [G * C_out/G][kernel][C/G].
 *   dyn_gelu_*          exact erf GELU
 *   dyn_colnorm_*       GroupNorm(groups == channels): per-(batch, channel) normalisation over time, biased variance
 *   dyn_col2im_1d       input gradient of a strided Conv1d from the dense [B, T_out, kernel*C] gradient of its rows
 *   dyn_group_pack ...  [B, T, C] <-> group-major zero-padded [B, G, T + 2 pad, C/G] (and the gradient counterparts)
 *   dyn_weight_norm_*   w = g[tap] * v / ||v[:, tap, :]||_F  (torch weight_norm with dim = 2) and its backward
 * ------------------------------------------------------------------------------------------------ */
int dyn_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int dyn_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* Feature-extractor layer of the layer-norm layout (`feat_extract_norm: "layer"`, `conv_bias: true`: wav2vec2-large-960h-lv60-self,
 * large-robust, XLSR), which the reference reaches through the same `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23)
 * and `model(input_values).logits` (:163,413) / `loss.backward()` (:194,437).  Replaces, after the bias-free conv GEMM, the rest of
 * transformers' Wav2Vec2LayerNormConvLayer.forward (modeling_wav2vec2.py: `self.conv` bias add, `transpose`, `self.layer_norm`,
 * `transpose`, `self.activation`) and its autograd in one pass each way over rows x C (C % 256 == 0, or C = 64 / 128: SEW's narrow extractor layers, several rows per wave; else DYN_E_ARG; C <= 1024):
 *   fwd: act = gelu(LN(z + conv_bias)), exact erf GELU as dyn_gelu_fwd; writes mean / rstd [rows]; z is not modified; conv_bias may be null.
 *   bwd: recomputes xhat and n = xhat * gamma + beta from z, mean, rstd (the normalised tensor is never stored); dn = dact * gelu'(n);
 *        dz = LayerNorm backward of dn (dz may be dact itself); dgamma = sum dn * xhat, dbeta = sum dn, dconv_bias = sum dz over the rows,
 *        each `= wgrad_beta * old + sum` and each may be null (a frozen parameter).  The column sums go through per-workgroup partial
 *        rows in `workspace` and the fixed-order reducers (bit-reproducible; recorded instead while a dyn_reduce_defer context is open).
 * No call synchronises or allocates: both are captured into the length buckets' hipGraphs. */
int dyn_bias_layernorm_gelu_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float* act, float* mean,
                                float* rstd, int64_t rows, int64_t C, float eps, void* stream);
int64_t dyn_bias_layernorm_gelu_bwd_workspace_bytes(int64_t rows, int64_t C);
int dyn_bias_layernorm_gelu_bwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, const float* mean,
                                const float* rstd, const float* dact, float* dz, float* dgamma, float* dbeta, float* dconv_bias,
                                float wgrad_beta, int64_t rows, int64_t C, void* workspace, int64_t workspace_bytes, void* stream);
int64_t dyn_colnorm_workspace_bytes(int64_t B, int64_t T, int64_t C);
int dyn_colnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t B,
                    int64_t T, int64_t C, float eps, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_colnorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                    float* dgamma, float* dbeta, float wgrad_beta, int64_t B, int64_t T, int64_t C, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* The same with a DEVICE-side row count (`valid_rows`: null = all T rows, else an int32 scalar in HBM read when the kernels run):
 * statistics / sums over the first *valid_rows rows of every batch entry, dx = 0 past them.  With dyn_mask_rows and
 * dyn_softmax_fwd_len this lets one captured launch sequence (hipGraph) serve every utterance length of a zero-padded bucket of the
 * per-utterance loop (reference wav2vec2/lib.py:293-462 runs each utterance at its own length). */
int dyn_colnorm_fwd_len(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t B,
                        int64_t T, int64_t C, float eps, const int32_t* valid_rows, void* workspace, int64_t workspace_bytes,
                        void* stream);
int dyn_colnorm_bwd_len(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                        float* dgamma, float* dbeta, float wgrad_beta, int64_t B, int64_t T, int64_t C, const int32_t* valid_rows,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* x [B, T, C]: rows t >= *valid_rows of every batch entry := 0 (what the positional conv's zero padding holds past the last frame). */
int dyn_mask_rows(float* x, int64_t B, int64_t T, int64_t C, const int32_t* valid_rows, void* stream);
int dyn_col2im_1d(const float* dA, float* dx, int64_t B, int64_t Tin, int64_t Tout, int64_t C, int64_t kw, int64_t stride,
                  void* stream);
int dyn_group_pack(const float* x, float* xg, int64_t B, int64_t T, int64_t C, int64_t G, int64_t pad, void* stream);
int dyn_group_unpack(const float* yg, float* y, const float* bias, int64_t B, int64_t T, int64_t Tg, int64_t C, int64_t G,
                     void* stream);
int dyn_group_pack_grad(const float* dy, float* dyg, int64_t B, int64_t T, int64_t Tg, int64_t C, int64_t G, void* stream);
int dyn_group_unpack_grad(const float* dxg, float* dx, int64_t B, int64_t T, int64_t C, int64_t G, int64_t pad, float beta,
                          void* stream);
int64_t dyn_weight_norm_workspace_bytes(int64_t rows, int64_t kw);
int dyn_weight_norm_fwd(const float* v, const float* g, float* w, int64_t rows, int64_t kw, int64_t cg, void* workspace,
                        int64_t workspace_bytes, void* stream);
int dyn_weight_norm_bwd(const float* v, const float* g, const float* dw, float* dv, float* dg, float beta, int64_t rows,
                        int64_t kw, int64_t cg, void* workspace, int64_t workspace_bytes, void* stream);
/* One layer of Data2Vec-Audio's positional conv stack after its grouped conv GEMM.  The reference's loader,
 * `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23), builds transformers' Data2VecAudioForCTC for such a checkpoint;
 * `model(x).logits` (:163,413) and `loss.backward()` (:194,437) then run, `num_conv_pos_embeddings` times per step,
 * Data2VecAudioPositionalConvLayer.forward (modeling_data2vec_audio.py: `self.conv` bias add, `transpose(1, 2)`, `self.layer_norm`
 * = LayerNorm(H, elementwise_affine=False), `transpose(1, 2)`, `self.activation`) and its autograd.  Both entries work in the group-major
 * layouts of the grouped GEMMs (G groups of cg = H / G channels), so no dyn_group_pack / _unpack launch stands between two layers.
 * H % 256 == 0, H <= 1024, cg % 4 == 0, Tg >= T and non-null required pointers, else DYN_E_ARG:
 *   fwd: row (b, t) = yg[b, g, t, 0:cg] for g = 0..G-1 side by side (yg [B, G, Tg, cg] as dyn_group_unpack takes it; not modified)
 *        + bias [H]; out = gelu((row - mean) / sqrt(var + eps)), centred variance, exact erf GELU as dyn_gelu_fwd.  Written to `act`
 *        [B, T, H] and / or to `xg_next` [B, G, T + 2 pad, cg], the NEXT layer's packed input, including its 2 pad zero rows per (b, g)
 *        (either may be null, not both; both get the same bits).  mean / rstd [B T] are written for every row.  Rows t >= *valid_rows
 *        (null = T; a device int32 scalar read when the kernel runs, as dyn_mask_rows) are zeros in both outputs.
 *   bwd: recomputes xhat from yg, bias, mean, rstd; dn = dact * gelu'(xhat) with dact [B, T, H];
 *        dyg [B, G, T, cg] = rstd * (dn - mean_H(dn) - xhat * mean_H(dn * xhat)): the layout the weight- and data-gradient GEMMs read
 *        (replaces dyn_gelu_bwd + a LayerNorm backward + dyn_colsum + dyn_group_pack_grad); rows t >= *valid_rows are exact zeros.
 *        dbias [H] = wgrad_beta * old + column sums of dyg, may be null (frozen; then no workspace is needed).  The sums go through
 *        per-workgroup partial rows in `workspace` and the fixed-order reducer (bit-reproducible; recorded instead while a
 *        dyn_reduce_defer context is open).
 * No call synchronises or allocates: both are captured into the length buckets' hipGraphs. */
int dyn_posconv_ln_gelu_fwd(const float* yg, const float* bias, float* act, float* xg_next, float* mean, float* rstd, int64_t B, int64_t T,
                            int64_t Tg, int64_t H, int64_t G, int64_t pad, float eps, const int32_t* valid_rows, void* stream);
int64_t dyn_posconv_ln_gelu_bwd_workspace_bytes(int64_t rows, int64_t H);
int dyn_posconv_ln_gelu_bwd(const float* yg, const float* bias, const float* mean, const float* rstd, const float* dact, float* dyg,
                            float* dbias, float wgrad_beta, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G,
                            const int32_t* valid_rows, void* workspace, int64_t workspace_bytes, void* stream);
/* The two ends of SEW's squeezed encoder.  The reference's loader, `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23),
 * builds transformers' SEWForCTC for a SEW checkpoint; `model(x).logits` (:163,413) and `loss.backward()` (:194,437) then run
 * SEWEncoder.forward (modeling_sew.py) and its autograd.  T2 = T / s frames (s = squeeze_factor in 1..4, else DYN_E_ARG naming it), G groups
 * of cg = H / G channels; for the two squeeze entries H % 256 == 0, H <= 1024, cg % 4 == 0, Tg >= T2 and non-null required pointers, for the
 * two unsqueeze entries H % 4 == 0, else DYN_E_ARG.  `valid_rows` (null = T2; a device int32 scalar read when the kernel runs, as
 * dyn_mask_rows) counts SQUEEZED frames.
 *   dyn_squeeze_ln_fwd      SEWEncoder.forward from `position_embeddings = self.pos_conv_embed(hidden_states)` AFTER its conv's product
 *                           (the bias add inside `self.conv`, SEWSamePadLayer, `self.activation`), `self.pool(hidden_states)` =
 *                           AvgPool1d(s, s), `pooled_hidden_states[..., :min_length] + position_embeddings[..., :min_length]`, the two
 *                           transposes and `self.layer_norm`: z [B, T2, H] = LayerNorm_H(mean_j h[b, s t + j] + gelu(yg[b, g, t, 0:cg] for
 *                           g = 0..G-1 side by side + bias)) * gamma + beta, with h [B, T, H] and yg [B, G, Tg, cg] the strided grouped GEMM's
 *                           output (as dyn_group_unpack takes it); neither is modified.  Centred variance, exact erf GELU as dyn_gelu_fwd.
 *                           mean / rstd [B T2] are written for every row; rows t >= *valid_rows of z are zeros.
 *   dyn_squeeze_ln_bwd      its autograd: the pre-LayerNorm row is recomputed from h, yg, bias; dsum = the LayerNorm backward of dz [B, T2, H];
 *                           dh [B, T, H] rows s t + j = dsum[t] / s, rows >= s T2 and rows >= s * *valid_rows exact zeros (fully written);
 *                           dyg [B, G, T2, cg] = dsum * gelu'(yg + bias), the layout the weight- and data-gradient GEMMs read, rows >=
 *                           *valid_rows exact zeros.  dgamma / dbeta / dbias [H] = wgrad_beta * old + column sums of dz * xhat, dz, dyg over the
 *                           valid rows; each may be null (frozen; with all three null no workspace is needed; else dyn_squeeze_ln_bwd_workspace_bytes(B * (T2 + 1), H),
 *                           the rows the kernel walks).  The sums go through
 *                           per-workgroup partial rows in `workspace` and the fixed-order reducer (bit-reproducible; recorded instead while
 *                           a dyn_reduce_defer context is open).
 *   dyn_unsqueeze_act_fwd   SEWUpsampling.forward after `self.projection` (`self.activation`, the two `reshape`s) and SEWEncoder.forward's
 *                           `nn.functional.pad(hidden_states, (0, 0, 0, n_input_timesteps - hidden_states.shape[1]))`: out [B, T, H] rows
 *                           t < s T2 = gelu(u[b, t / s, (t % s) H : (t % s + 1) H]) with u [B, T2, s H] (bias already added), rows >= s T2 and
 *                           rows >= s * *valid_rows exact zeros.
 *   dyn_unsqueeze_act_bwd   du [B, T2, s H] = d * gelu'(u) with d [B, T, H]; rows >= *valid_rows exact zeros, d is read on rows
 *                           < s * *valid_rows only.
 * No call synchronises or allocates: all four are captured into the length buckets' hipGraphs. */
int dyn_squeeze_ln_fwd(const float* h, const float* yg, const float* bias, const float* gamma, const float* beta, float* z, float* mean,
                       float* rstd, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, float eps, const int32_t* valid_rows,
                       void* stream);
int64_t dyn_squeeze_ln_bwd_workspace_bytes(int64_t rows, int64_t H);
int dyn_squeeze_ln_bwd(const float* h, const float* yg, const float* bias, const float* gamma, const float* mean, const float* rstd,
                       const float* dz, float* dh, float* dyg, float* dgamma, float* dbeta, float* dbias, float wgrad_beta, int64_t B,
                       int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, const int32_t* valid_rows, void* workspace,
                       int64_t workspace_bytes, void* stream);
int dyn_unsqueeze_act_fwd(const float* u, float* out, int64_t B, int64_t T, int64_t H, int64_t s, const int32_t* valid_rows, void* stream);
int dyn_unsqueeze_act_bwd(const float* u, const float* d, float* du, int64_t B, int64_t T, int64_t H, int64_t s, const int32_t* valid_rows,
                          void* stream);
/* SEW-D's squeeze: the same pass without the LayerNorm.  transformers' SEWDForCTC (what the reference's loader builds for `model_type:
 * "sew-d"`) runs SEWDEncoder.forward (modeling_sew_d.py:1146-1152): `position_embeddings = self.pos_conv_embed(hidden_states)` after its
 * conv's product, `self.pool(hidden_states)`, `pooled_hidden_states + position_embeddings[..., :pooled_hidden_states.size(-1)]`, the two
 * `transpose(1, 2)`, and hands the sum to SEWDTransformerEncoder as it is.  Shapes, layouts, `valid_rows` and refusals as the two entries
 * above (same kernel templates, LayerNorm compiled out):
 *   dyn_squeeze_fwd   z [B, T2, H] row t = the mean of h rows s t .. s t + s - 1 + gelu(yg row t + bias); rows >= *valid_rows zeros.
 *   dyn_squeeze_bwd   its autograd from dz [B, T2, H]: dh rows s t + j = dz[t] / s (rows >= s T2 and >= s * *valid_rows exact zeros, fully
 *                     written), dyg [B, G, T2, cg] = dz * gelu'(yg + bias) (rows >= *valid_rows exact zeros), dbias [H] = wgrad_beta * old +
 *                     the column sums of dyg (null: frozen, no workspace needed; else dyn_squeeze_bwd_workspace_bytes(B * (T2 + 1), H)),
 *                     through per-workgroup partial rows and the fixed-order reducer (deferrable).  h is not needed and not passed. */
int dyn_squeeze_fwd(const float* h, const float* yg, const float* bias, float* z, int64_t B, int64_t T, int64_t Tg, int64_t H, int64_t G,
                    int64_t s, const int32_t* valid_rows, void* stream);
int64_t dyn_squeeze_bwd_workspace_bytes(int64_t rows, int64_t H);
int dyn_squeeze_bwd(const float* yg, const float* bias, const float* dz, float* dh, float* dyg, float* dbias, float wgrad_beta, int64_t B,
                    int64_t T, int64_t Tg, int64_t H, int64_t G, int64_t s, const int32_t* valid_rows, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SEW-D attention: DeBERTa-v2's disentangled relative-position score (csrc/disentangled.hip).  For `model_type: "sew-d"` the reference's
 * loader builds transformers' SEWDForCTC, whose every layer runs DisentangledSelfAttention.forward (modeling_sew_d.py:680-761) with
 * `share_att_key`.  With M = B * heads, n_buckets = 2 * att_span rows of relative embeddings, and
 *   table [2T - 1] int32 (device), table[d + T - 1] = t(d) = clamp(bucket(d) + att_span, 0, 2 att_span - 1), built ON THE HOST from
 *   build_relative_position / make_log_bucket_position (:159-201; a float32 ceil(log) on integer boundaries: a kernel's rounding would be a
 *   wrong bucket) and monotone non-decreasing in d; seg_lo / seg_hi [n_buckets] int32: bucket r is the run seg_lo[r] <= d <= seg_hi[r]
 *   (lo > hi: empty):
 *   dyn_softmax_disentangled_fwd  disentangled_attention_bias (:763-839: the two `torch.gather`s, `c2p_pos` / `p2c_pos`, the
 *                                 `.transpose(-1, -2)`, both `/ scale`) + `attention_scores + rel_att` (:740) + XSoftmax (:746):
 *                                 y[m, i, :] = softmax_j(x[m, i, j] + c2p[m, i, t(i - j)] + p2ct[m, t(i - j), j]); x [M, T, T] = the scaled
 *                                 content scores, c2p [M, T, ldp] = scaled q Pk^T, p2ct [M, ldp, T] = scaled Pq k^T (position -> content,
 *                                 transposed); either term may be null (`pos_att_type` with one of them), not both.  y may be x.  Columns /
 *                                 rows >= n_buckets of c2p / p2ct are never read.  `valid_cols` as dyn_softmax_fwd_len.  T <= 16384.
 *   dyn_disentangled_bwd          the autograd of the two gathers from dS [M, T, T] (what dyn_softmax_bwd leaves):
 *                                 dC2P[m, i, r] = sum over d in run r of dS[m, i, i - d], dP2CT[m, r, j] = sum over d in run r of
 *                                 dS[m, j + d, j]; each element ONE sum in ascending key (query) order, no float atomics, no zero-fill,
 *                                 bit-reproducible; both outputs ([M, T, ldp] and [M, ldp, T]) are written completely, empty buckets and
 *                                 indices >= n_buckets as exact zeros.  Rows and columns >= *valid of dS are not read; rows >= *valid of
 *                                 dC2P and columns >= *valid of dP2CT are exact zeros.  Either output may be null, not both.  T <= 8192.
 * ldp >= n_buckets >= 1, else DYN_E_ARG.  A table entry outside [0, n_buckets) is clamped before use.  No call synchronises or allocates. */
int dyn_softmax_disentangled_fwd(const float* x, float* y, const float* c2p, const float* p2ct, const int32_t* table, int64_t M, int64_t T,
                                 int64_t ldp, int64_t n_buckets, const int32_t* valid_cols, void* stream);
int dyn_disentangled_bwd(const float* dS, float* dC2P, float* dP2CT, const int32_t* table, const int32_t* seg_lo, const int32_t* seg_hi,
                         int64_t M, int64_t T, int64_t ldp, int64_t n_buckets, const int32_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MMS adapters (csrc/attn_adapter.hip).  For an MMS checkpoint (`adapter_attn_dim: 16`) the reference's loader,
 * `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23), builds transformers' Wav2Vec2ForCTC with a Wav2Vec2AttnAdapterLayer
 * behind every stable-LN encoder layer; `model(x).logits` (:163,413) then runs `hidden_states + self.adapter_layer(hidden_states)` =
 * x + linear_2(relu(linear_1(norm(x)))) per layer and `loss.backward()` its autograd.  x [M, H] row-major, gamma / beta [H] the norm,
 * W1 [A, H] / b1 [A] linear_1, W2 [H, A] / b2 [H] linear_2.  H % 256 == 0 and H <= 2048, A % 4 == 0 and 4 <= A <= 64, non-null required
 * pointers, 16-byte aligned operands, else DYN_E_ARG naming the entry.
 *   dyn_attn_adapter_fwd   y [M, H] = x + W2 relu(W1 LayerNorm(x) + b1) + b2 in one launch (centred variance; the normalised row is never
 *                          written); y may be x.  mean / rstd [M] and a [M, A] (the post-ReLU bottleneck) are written when non-null.
 *   dyn_attn_adapter_bwd   from x, mean, rstd, a, dy [M, H]: dx [M, H] = dy + the adapter path, out of place (dx must alias neither dy nor x,
 *                          both are left unmodified).  dgamma, dbeta, dW1, db1, dW2, db2 += their sums over the M rows (beta = 1); each may be
 *                          null and is then not computed.  The ReLU mask is a > 0.  A row of dy that is all zeros gives an all-zero row of dx
 *                          and adds exact zeros to every sum.  Two launches: the rows, then every sum in a fixed order from du [M, A] and
 *                          per-workgroup partial rows in `workspace` (dyn_attn_adapter_bwd_workspace_bytes(M, H, A), DYN_E_WORKSPACE when
 *                          smaller; not needed with all six null): no atomics, the same call twice gives the same bits.
 * No call synchronises or allocates: all are captured into the length buckets' hipGraphs. */
int dyn_attn_adapter_fwd(const float* x, const float* gamma, const float* beta, const float* W1, const float* b1, const float* W2,
                         const float* b2, float* y, float* mean, float* rstd, float* a, int64_t M, int64_t H, int64_t A, float eps,
                         void* stream);
int64_t dyn_attn_adapter_bwd_workspace_bytes(int64_t M, int64_t H, int64_t A);
int dyn_attn_adapter_bwd(const float* x, const float* gamma, const float* beta, const float* W1, const float* W2, const float* mean,
                         const float* rstd, const float* a, const float* dy, float* dx, float* dgamma, float* dbeta, float* dW1, float* db1,
                         float* dW2, float* db2, int64_t M, int64_t H, int64_t A, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * WavLM attention: gated relative-position bias.  The reference's loader, `AutoModelForCTC.from_pretrained(checkpoint)`
 * (wav2vec2/lib.py:20-23), builds transformers' WavLMForCTC for a WavLM checkpoint; `model(x).logits` (:163,413) and
 * `loss.backward()` (:194,437) then run WavLMAttention.forward (modeling_wavlm.py) in every layer.  With h [B, T, H] the attention's
 * input, nh heads of D = H / nh channels, E = rel_attn_embed.weight [num_buckets, nh] (layer 0's, used by every layer) and
 * bucket[d + Tmax - 1] the int32 table of _relative_positions_bucket(d), d in (-Tmax, Tmax), built ON THE HOST (it depends on a
 * float32 log; a kernel's rounding at a bucket edge would be a wrong bucket) and resident in device memory:
 *   dyn_relpos_gate_fwd          steps 1-3 of WavLMAttention.forward (`gru_rel_pos_linear`, `.view(.., 2, 4).sum(-1)`, sigmoid,
 *                                `gate_a * (gate_b * gru_rel_pos_const - 1.0) + 2.0`): p = W h[b, t, head*D:(head+1)*D] + bias
 *                                (W [8, D], bias [8]), a = sigmoid(p0+p1+p2+p3), c = sigmoid(p4+p5+p6+p7),
 *                                gate = a * (c * konst[head] - 1) + 2; gate, a, c are [B, nh, T].  One pass over h.
 *   dyn_softmax_relbias_fwd_len  compute_bias + step 4 + the softmax inside F.multi_head_attention_forward:
 *                                y[b,head,t,:] = softmax_s(x[b,head,t,s] + gate[b,head,t] * E[bucket[s - t + Tmax - 1], head]);
 *                                x = scale * q k^T [B, nh, T, T], y may be x.  `valid_cols` as dyn_softmax_fwd_len (device int32
 *                                scalar read when the kernel runs; columns >= it are outside max / sum and get probability 0);
 *                                NULL = all T columns.  T <= 16384; num_buckets even and <= 1024; T <= Tmax.
 *   dyn_relbias_bwd              autograd of the bias term from dS [B, nh, T, T], the gradient w.r.t. the pre-softmax sum (what
 *                                dyn_softmax_bwd leaves): dgate[b,head,t] = sum_s dS[b,head,t,s] * E[bucket(s-t), head] and
 *                                dE[k, head] = beta * dE[k, head] + sum_{b,t,s: bucket(s-t) = k} gate[b,head,t] * dS[b,head,t,s].
 *                                No float atomics: row blocks sum the diagonals of gate (.) dS in row order into per-distance
 *                                vectors (workspace), a second kernel adds them over (b, row block) in index order, a third folds
 *                                the 2T-1 distances into buckets in distance order.  Bit-reproducible.  T <= 8192.
 *   dyn_relpos_gate_bwd          autograd of dyn_relpos_gate_fwd: dh = beta_dh * dh + (d gate / d h) dgate (the attention's input
 *                                gradient, accumulated), dW [8, D], dbias [8], dkonst [nh] each = beta * old + sum, through
 *                                per-workgroup partial rows in `workspace` summed in index order.  D <= 256.
 * All four take the attention's (B, T, H, nh): null pointer, H % nh != 0, D % 4 != 0, odd or too large num_buckets, T beyond the row limit -> DYN_E_ARG before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_relpos_gate_fwd(const float* h, const float* W, const float* bias, const float* konst, float* gate, float* a, float* c,
                        int64_t B, int64_t T, int64_t H, int64_t nh, void* stream);
int dyn_softmax_relbias_fwd_len(const float* x, float* y, const float* gate, const float* E, const int32_t* bucket, int64_t B,
                                int64_t T, int64_t H, int64_t nh, int64_t Tmax, int64_t num_buckets, const int32_t* valid_cols,
                                void* stream);
int64_t dyn_relbias_bwd_workspace_bytes(int64_t B, int64_t nh, int64_t T, int64_t num_buckets);
int dyn_relbias_bwd(const float* dS, const float* gate, const float* E, const int32_t* bucket, float* dgate, float* dE, float beta,
                    int64_t B, int64_t T, int64_t H, int64_t nh, int64_t Tmax, int64_t num_buckets, void* workspace, int64_t workspace_bytes,
                    void* stream);
int64_t dyn_relpos_gate_bwd_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t nh);
int dyn_relpos_gate_bwd(const float* dgate, const float* a, const float* c, const float* h, const float* W, const float* konst,
                        float* dh, float beta_dh, float* dW, float* dbias, float* dkonst, float beta, int64_t B, int64_t T, int64_t H,
                        int64_t nh, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wav2Vec2-Conformer attention, `position_embeddings_type: "relative"` (transformers Wav2Vec2ConformerSelfAttention.
 * _apply_relative_embeddings; what `AutoModelForCTC.from_pretrained` builds for wav2vec2-conformer-rel-pos-*): the Transformer-XL score
 * ((q + u) k^T + shift((q + v) P^T)) / sqrt(D), P = linear_pos(pe) with pe [2T - 1, H] (row k = relative position T - 1 - k).  The
 * products are dyn_gemm_f32's; M = B * nh score matrices, x = (q + u) k^T [M, T, T] and bd = (q + v) P_h^T [M, T, ld_bd >= 2T - 1], both
 * already scaled.  transformers' pad / view / slice shift equals bd[i, T - 1 - i + j]: no copy is made of it in either direction.
 *   dyn_softmax_relshift_fwd_len  y[m,i,:] = softmax_j(x[m,i,j] + bd[m, i, T - 1 - i + j]); y may be x (not bd).  `valid_cols` as
 *                                 dyn_softmax_fwd_len.  One pass: x and the window of bd read once, y written once.  T <= 16384.
 *   dyn_relshift_bwd              dBD[m,i,k] = dS[m, i, k - (T - 1) + i] inside the window, 0 WRITTEN in every other column of the
 *                                 ld_bd-float row: the buffer may be uninitialised scratch.
 *   dyn_head_bias_add             u, v [nh, D] = [H]: qu[r,c] = q[r * ldq + c] + u[c], qv likewise (q strided inside a packed
 *                                 projection output, qu / qv [rows, H] contiguous).  H % 4 == 0, ldq % 4 == 0, 16-byte aligned.
 *   dyn_head_bias_bwd             dq[r * ldq + c] = dqu[r,c] + dqv[r,c]; du[c] = beta * du[c] + sum_r dqu[r,c], dv likewise: partial
 *                                 rows per workgroup in `workspace`, added in workgroup order (bit-reproducible, deferrable).
 * Null pointer, T < 1, ld_bd < 2T - 1, T beyond the row limit, unaligned operands -> DYN_E_ARG before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_softmax_relshift_fwd_len(const float* x, float* y, const float* bd, int64_t M, int64_t T, int64_t ld_bd, const int32_t* valid_cols,
                                 void* stream);
int dyn_relshift_bwd(const float* dS, float* dBD, int64_t M, int64_t T, int64_t ld_bd, void* stream);
int dyn_head_bias_add(const float* q, int64_t ldq, const float* u, const float* v, float* qu, float* qv, int64_t rows, int64_t H,
                      void* stream);
int64_t dyn_head_bias_bwd_workspace_bytes(int64_t rows, int64_t H);
int dyn_head_bias_bwd(const float* dqu, const float* dqv, float* dq, int64_t ldq, float* du, float* dv, float beta, int64_t rows, int64_t H,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Soft-DTW — replaces the reference's Numba CUDA kernels compute_softdtw_cuda / compute_softdtw_backward_cuda
 * (reference wav2vec2/soft_dtw_cuda.py:33-111), their autograd wrapper (:114-175) and _euclidean_dist_func (:319-329).
 *   dyn_sqdist       D[b,i,j] = sum_k (x[b,i,k] - y[b,j,k])^2            x [B,N,d], y [B,M,d] -> D [B,N,M]
 *   dyn_sqdist_bwd_x dx[b,i,k] = sum_j 2 G[b,i,j] (x[b,i,k] - y[b,j,k])
 *   dyn_softdtw_fwd  R [B,N+2,M+2] fp64 lattice workspace (written entirely by the kernel; keep it for the backward),
 *                    value[b] = R[b,N,M] (fp32)
 *   dyn_softdtw_bwd  E [B,N,M] = d value / d D  (multiply by grad_output on the caller side, as :173-174)
 * bandwidth <= 0 disables the Sakoe-Chiba pruning.  No 1024 limit on N, M (reference :312-314 falls back to CPU).
 * ------------------------------------------------------------------------------------------------ */
int dyn_sqdist(const float* x, const float* y, float* D, int64_t B, int64_t N, int64_t M, int64_t d, void* stream);
int dyn_sqdist_bwd_x(const float* x, const float* y, const float* G, float* dx, int64_t B, int64_t N, int64_t M, int64_t d,
                     void* stream);
int dyn_softdtw_fwd(const float* D, double* R, float* value, int64_t B, int64_t N, int64_t M, float gamma, float bandwidth,
                    void* stream);
int dyn_softdtw_bwd(const float* D, const double* R, float* E, int64_t B, int64_t N, int64_t M, float gamma, float bandwidth,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edit-distance counts of a ragged batch of P token-id pairs — replaces the host dynamic programme behind every WER / CER
 * (`word_error_rate_detail` at reference lcasr/lib.py:1348-1349 inside calc_rewards and run_dynamic_eval_full.py:112-115).
 *   counts [P, 4] int32 = (insertions, deletions, substitutions, reference length) of the alignment the cell rule
 *   "diagonal if diag <= up, else up; left only when strictly smaller" picks (substitution / match, then deletion, then
 *   insertion); an empty reference gives (m, 0, 0), an empty hypothesis (0, n, 0).
 *   hyp / ref: device int32 ids, pair p at [hyp_off[p], hyp_off[p + 1]) / [ref_off[p], ref_off[p + 1]).
 *   hyp_off / ref_off: HOST arrays of P + 1 offsets (the entry plans its launches from them); dev_off: their DEVICE copy,
 *   hyp_off [P + 1] followed by ref_off [P + 1].
 * Pairs with both sides <= dyn_edit_counts_resident_limit() are scored by one workgroup each with the lattice's live
 * diagonals in LDS; longer pairs are cut into tile x tile blocks whose boundary rows / columns live in the workspace, one
 * launch per block anti-diagonal.  tile = 0 is the default (1024); an explicit tile in [8, 2048] also sends every pair with
 * a side >= tile through the tiled regime (tests, tuning).  dyn_edit_counts_workspace_bytes returns bytes or a negative
 * DYN_E_* code.
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_edit_counts_resident_limit(void);
int64_t dyn_edit_counts_workspace_bytes(const int64_t* hyp_off, const int64_t* ref_off, int64_t P, int64_t tile);
int dyn_edit_counts(const int32_t* hyp, const int32_t* ref, const int64_t* hyp_off, const int64_t* ref_off, const int64_t* dev_off,
                    int32_t* counts, void* workspace, int64_t workspace_bytes, int64_t P, int64_t tile, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC + transformer-LM beam search (reference lcasr/ctc_beam_search.py:89-319 with max_cache_length = 128, lcasr/lib.py:37-72).
 *   dyn_beam_search   the whole search over log_probs [frames, ld] (n_classes = vocab + 1, blank = n_classes - 1), enqueued on
 *                     `stream` without a host synchronisation: per frame one bookkeeping kernel (candidates, CTC prefix rules, exact
 *                     merge, stable top-k, relative prune when use_prune != 0) and one LM step for the new beams.  The final beams
 *                     stay in the workspace (dyn_beam_layout gives the offsets); header word 2 != 0 reports a failed search.
 *   dyn_beam_lm_rows  one LM step for the rows the workspace's row arrays describe (token, position, history slots, output slot)
 *   lm_ptrs: host array of device pointers — embed [vocab, d], positions [max_positions, d], norm_out w / b, head w [vocab, d] / b,
 *            then per layer: self.norm w / b, self.qkv w [3d, d] / b, self.out w / b, ff.norm w / b, ff.w1 [d_ff, d], ff.w2 [d, d_ff].
 *   dyn_beam_layout   offsets[18]: header, beam node / trailing blank / score / history length / history, node parent / token,
 *                     pool log-probs, row token / position / history length / slot / history, pool K/V, node capacity, pool slots,
 *                     total bytes.
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_beam_workspace_bytes(int32_t width, int64_t frames, int32_t layers, int32_t d_model, int32_t d_ff, int32_t vocab);
int dyn_beam_layout(int32_t width, int64_t frames, int32_t layers, int32_t d_model, int32_t d_ff, int32_t vocab, int64_t* offsets);
int dyn_beam_lm_rows(const void* lm_ptrs, int32_t layers, int32_t d_model, int32_t heads, int32_t d_ff, int32_t vocab,
                     int32_t max_positions, float eps, int32_t width, int64_t frames, void* workspace, int64_t workspace_bytes,
                     void* stream);
int dyn_beam_search(const float* log_probs, int64_t frames, int64_t ld, int32_t n_classes, const void* lm_ptrs, int32_t layers,
                    int32_t d_model, int32_t heads, int32_t d_ff, int32_t vocab, int32_t max_positions, float eps, int32_t bos,
                    int32_t width, float alpha, float beta, float blank_penalty, float repetition_penalty, float top_am_threshold,
                    float prune_less_than, int32_t use_prune, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wav2Vec2-BERT (`model_type: "wav2vec2-bert"`, transformers Wav2Vec2BertForCTC; what `AutoModelForCTC.from_pretrained` builds for a
 * w2v-BERT 2.0 fine-tune).  fp32, deterministic, no float atomics.
 *   dyn_convmod_causal_fwd     Wav2Vec2BertConvolutionModule.forward between its two pointwise convolutions: `self.glu`, `F.pad(x,
 *                              (kernel_size - 1, 0))`, `self.depthwise_conv`, `self.depthwise_layer_norm`, `self.activation` in one
 *                              launch.  u [B, T, 2C] -> s [B, T, C] = act(LN_C(sum_j w[c, j] * GLU(u)[t - (KW - 1) + j, c])), zeros left
 *                              of frame 0; w [C, KW]; act 0 = SiLU, 1 = erf GELU.  Optional outputs (null: not written) for the
 *                              backward: g the GLU output, c the convolution output, n the LayerNorm output [B, T, C], mean / rstd
 *                              [B * T] (centred two-pass variance).  time_tile: 0 = dyn_convmod_causal_time_tile(B, T), or 8 / 16 frames
 *                              per workgroup (tests, tuning).  KW = 31, C in {256, 512, 768, 1024}: anything else DYN_E_UNSUPPORTED.
 *   dyn_dwconv1d_causal_dgrad  the autograd of that padded depthwise convolution w.r.t. its input:
 *                              dx[b,t,c] = dx_beta * dx[b,t,c] + sum_j w[c,j] * dy[b, t + (KW - 1) - j, c] (rows >= T are zeros).
 *   dyn_dwconv1d_causal_wgrad  ... w.r.t. its weight: dw[c,j] = beta * dw[c,j] + sum_{b,t} dy[b,t,c] * x[b, t - (KW - 1) + j, c], partial
 *                              sums per time tile in `workspace`, combined in tile order (bit-reproducible, deferrable).
 *   dyn_narrow_layernorm_fwd   Wav2Vec2BertFeatureProjection.forward `self.layer_norm(hidden_states)` over C = 160 stacked filter-bank
 *                              channels: LayerNorm of rows x C for C % 4 == 0, C <= 256 (one wave per row; the other LayerNorm
 *                              entries need C % 256 == 0).  y, mean [rows], rstd [rows]; beta may be null.
 *   dyn_narrow_layernorm_bwd   its autograd: dgamma / dbeta = wgrad_beta * old + column sums (partial rows per workgroup in `workspace`,
 *                              added in workgroup order; either may be null), dx [rows, C] optional (null: the input is data).
 *   dyn_fbank_finish           the tail of SeamlessM4TFeatureExtractor.__call__ after the mel projection (`np.maximum(mel_floor, ..)`,
 *                              log, `(x - x.mean(0)) / sqrt(x.var(0, ddof=1) + 1e-7)`, the reshape to [frames // 2, 2 * bins]):
 *                              mel [B, F, M] -> out [B, F / 2, 2M], per sample.  valid_frames (device int32 scalar, may be null = F; read when the kernel
 *                              runs): the statistics cover the first `valid` frames, rows >= valid / 2 of out are written as zeros.
 * Null pointers, sizes out of range -> DYN_E_ARG, a C / KW that is not built -> DYN_E_UNSUPPORTED, a short workspace -> DYN_E_WORKSPACE, all
 * before any launch.
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_convmod_causal_time_tile(int64_t B, int64_t T);
int dyn_convmod_causal_fwd(const float* u, const float* w, const float* gamma, const float* beta, float* s, float* g, float* c, float* n,
                           float* mean, float* rstd, int64_t B, int64_t T, int64_t C, int64_t KW, int32_t act, float eps, int64_t time_tile,
                           void* stream);
int dyn_dwconv1d_causal_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                              void* stream);
int64_t dyn_dwconv1d_causal_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW);
int dyn_dwconv1d_causal_wgrad(const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                              void* workspace, int64_t workspace_bytes, void* stream);
int dyn_narrow_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                             int64_t C, float eps, void* stream);
int64_t dyn_narrow_layernorm_bwd_workspace_bytes(int64_t rows, int64_t C);
int dyn_narrow_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                             float* dgamma, float* dbeta, float wgrad_beta, int64_t rows, int64_t C, void* workspace,
                             int64_t workspace_bytes, void* stream);
int dyn_fbank_finish(const float* mel, float* out, int64_t B, int64_t F, int64_t M, float mel_floor, float eps, const int32_t* valid_frames,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Parakeet (`model_type: "parakeet_ctc"`, transformers ParakeetForCTC: the FastConformer encoder of the nvidia/parakeet-ctc checkpoints,
 * the model family of the reference's nvidia_ctc/lib.py).  fp32, deterministic, no float atomics.
 *   dyn_convmod_bn_fwd        ParakeetEncoderConvolutionModule.forward between its two pointwise convolutions: `glu`, `depthwise_conv`,
 *                             `norm` (BatchNorm1d in eval mode: running statistics), `activation` in one launch.
 *                             u [B, T, 2C] -> s [B, T, C] = act((conv - mean_c) * rsqrt(var_c + eps) * weight_c + bias_c),
 *                             conv[b,t,c] = cbias_c + sum_j w[c,j] * GLU(u)[b, t - (KW - 1) / 2 + j, c], zero SAME padding; w [C, KW];
 *                             an even KW pads as torch's padding="same": (KW - 1) / 2 = 15 frames left, 16 right at KW = 32;
 *                             cbias [C] may be null (convolution_bias = false); mean / var / weight / bias [C]; act 0 = SiLU.
 *                             valid (device int32 scalar, may be null = T; read when the kernel runs): GLU rows t >= *valid read as
 *                             zeros.  Optional outputs (null: not written) for the backward: gl the masked GLU output, c the
 *                             convolution output before BatchNorm, [B, T, C].  Rows >= *valid of s, gl and c are exact zeros.
 *                             dyn_convmod_bn_time_tile() is the number of frames one workgroup takes at 9 taps,
 *                             dyn_convmod_bn_time_tile_kw(KW) at KW taps (0: KW is not built) (tests).
 *   dyn_convmod_bn_bwd_act    from c, the BatchNorm constants and ds [B, T, C]: dc = ds * act'(bn) * weight * rstd (dc may be ds), and
 *                             dweight = wgrad_beta * old + sum ds * act' * xhat, dbias = .. + sum ds * act', dcbias = .. + sum dc over
 *                             the rows; each of the three may be null (frozen: not computed, nothing written).  Partial rows per
 *                             workgroup in `workspace`, combined in workgroup order (bit-reproducible, deferrable).  Rows >= *valid
 *                             give dc = 0 and are left out of the sums.
 *   dyn_glu_dwconv1d_dgrad    du [B, T, 2C] = GLU'(u) * sum_j w[c,j] * dc[b, t + (KW - 1) / 2 - j, c] (rows of dc outside [0, T) are
 *                             zeros): the depthwise data gradient and the GLU backward in one pass, no dgl tensor.  Its halo mirrors
 *                             the forward's: 16 frames back and 15 ahead at KW = 32.  Rows >= *valid of du are exact zeros.  du must
 *                             not alias u or dc.
 *   The depthwise weight gradient is dyn_dwconv1d_wgrad(gl, dc, ..), built at KW = 32 too (dw[c,j] = sum_t dc[t] * gl[t + j - 15]); the plain
 *   depthwise entries dyn_dwconv1d_fwd / _dgrad / _dgrad_g stay refused at even widths.
 *   dyn_dwconv2d_s2_*_act     dyn_dwconv2d_s2_fwd / _dgrad / _wgrad with the activation fused into the loads chosen by the caller:
 *                             act 0 = SiLU (those entries, bit for bit), 1 = ReLU (Parakeet's dw_striding subsampling; ReLU'(0) = 0).
 *   dyn_relu_fwd / _bwd       y = max(x, 0); dx = x > 0 ? dy : 0 (in place allowed), n elements, 16-byte aligned.
 * KW = 9 (Parakeet) or 32 (LASR: `model_type: "lasr_ctc"`, transformers LasrForCTC, google/medasr), C in {256, 512, 768, 1024}, act as
 * listed: anything else DYN_E_UNSUPPORTED.  Null pointers, sizes out of range -> DYN_E_ARG, a
 * short workspace -> DYN_E_WORKSPACE, all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_convmod_bn_time_tile(void);
int64_t dyn_convmod_bn_time_tile_kw(int64_t KW);
int dyn_convmod_bn_fwd(const float* u, const float* w, const float* cbias, const float* mean, const float* var, const float* weight,
                       const float* bias, float* s, float* gl, float* c, const int32_t* valid, int64_t B, int64_t T, int64_t C, int64_t KW,
                       int32_t act, float eps, void* stream);
int64_t dyn_convmod_bn_bwd_act_workspace_bytes(int64_t B, int64_t T, int64_t C);
int dyn_convmod_bn_bwd_act(const float* c, const float* mean, const float* var, const float* weight, const float* bias, const float* ds,
                           float* dc, float* dweight, float* dbias, float* dcbias, float wgrad_beta, const int32_t* valid, int64_t B,
                           int64_t T, int64_t C, int32_t act, float eps, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_glu_dwconv1d_dgrad(const float* u, const float* w, const float* dc, float* du, const int32_t* valid, int64_t B, int64_t T, int64_t C,
                           int64_t KW, void* stream);
int dyn_dwconv2d_s2_fwd_act(const float* z, const float* w, const float* bias, float* u, int64_t B, int64_t T, int64_t F, int64_t C,
                            int32_t act, void* stream);
int dyn_dwconv2d_s2_dgrad_act(const float* z, const float* w, const float* du, float* dz, int64_t B, int64_t T, int64_t F, int64_t C,
                              int32_t act, void* stream);
int dyn_dwconv2d_s2_wgrad_act(const float* z, const float* du, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                              int64_t C, int32_t act, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int dyn_relu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The conv-module core with the norm the reference's third loop runs (reference nvidia_ctc/lib.py:74,89-102): `model.train()`, the conv
 * module and its batch norm put into eval mode, and that batch norm then REPLACED by a fresh BatchRenorm1d(momentum = 0.001, eps = 1e-5),
 * which is in training mode (num_batches_tracked = 1000000 saturates its clamps at rmax = 3, dmax = 5; running_std = sqrt(running_var)).
 * BatchRenorm1d is the `batchrenorm` package form; parity unpinned against upstream `lcasr`.  Per channel over the n = B * *valid valid
 * rows of x = the depthwise convolution's output:
 *     mu = mean(x), std = sqrt(mean((x - mu)^2)) (biased), sig = std + eps (eps joins the deviation, not the variance),
 *     r = clamp(sig / running_std, 1 / rmax, rmax), d = clamp((mu - running_mean) / running_std, -dmax, dmax)   (both constants of the backward)
 *     s = act(weight * ((x - mu) / sig * r + d) + bias);
 *     running_mean += momentum * (mu - running_mean), running_std += momentum * (sig - running_std)   (in place; momentum = 0: untouched).
 * rmax / dmax come from the caller (the schedule over num_batches_tracked is host arithmetic).  fp32, no float atomics, centred
 * statistics (no E[x^2] - E[x]^2), every result bit-reproducible.  A channel whose batch variance is exactly zero is OUTSIDE the contract
 * (the backward divides by std).
 *   dyn_convmod_brn_fwd     u [B, T, 2C], w [C, KW], cbias [C] or null -> s, gl, c [B, T, C] (all three written; rows >= *valid exact zeros)
 *                           and stats [dyn_convmod_brn_stats_rows() = 7][C]: mu, 1 / sig, r, d, scale = weight * r / sig,
 *                           shift = weight * d + bias, 1 / std (what the backward reads).  Three launches: the GLU + depthwise forward of
 *                           dyn_convmod_bn_fwd leaving one centred partial (count, mean, sum of squared deviations) per time tile and
 *                           channel in `workspace`; one thread per channel combining them in tile order (pairwise update, count 0 skipped);
 *                           the apply.  s, c, stats 16-byte aligned.
 *   dyn_convmod_brn_bwd     from c, stats and ds [B, T, C]: dc = scale * (g - mean(g) - (x - mu) / std * mean(g * x0)), g = ds * act'(y),
 *                           x0 = (x - mu) / sig (dc may be ds); dbias = wgrad_beta * old + sum g, dweight = wgrad_beta * old +
 *                           r * sum(g * x0) + d * sum g (null: frozen, not written); dcbias = wgrad_beta * old: the convolution bias
 *                           cancels in x - mu, its gradient is identically zero and no sum is launched for it.  Three launches (g and the
 *                           per-workgroup partial rows in dyn_convmod_bn_bwd_act's fixed row order; one thread per channel adding them in
 *                           workgroup order; dc in place).  The two sums are needed before dc, so this reduction is never deferred.
 *                           The gradient reaches every row of the batch.  c, dc, stats, workspace 16-byte aligned.
 *   The depthwise weight gradient and the data gradient stay dyn_dwconv1d_wgrad(gl, dc) and dyn_glu_dwconv1d_dgrad.
 * KW in {9, 32}, C in {256, 512, 768, 1024}, act 0 = SiLU: anything else DYN_E_UNSUPPORTED.  Null pointers, rmax < 1, dmax < 0, momentum
 * outside [0, 1], B * T < 2 -> DYN_E_ARG; a short workspace -> DYN_E_WORKSPACE; all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int64_t dyn_convmod_brn_stats_rows(void);
int64_t dyn_convmod_brn_fwd_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW);
int dyn_convmod_brn_fwd(const float* u, const float* w, const float* cbias, float* running_mean, float* running_std, const float* weight,
                        const float* bias, float* s, float* gl, float* c, float* stats, const int32_t* valid, int64_t B, int64_t T,
                        int64_t C, int64_t KW, int32_t act, float eps, float rmax, float dmax, float momentum, void* workspace,
                        int64_t workspace_bytes, void* stream);
int64_t dyn_convmod_brn_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C);
int dyn_convmod_brn_bwd(const float* c, const float* stats, const float* ds, float* dc, float* dweight, float* dbias, float* dcbias,
                        float wgrad_beta, const int32_t* valid, int64_t B, int64_t T, int64_t C, int32_t act, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The transducer head of ParakeetForTDT (`model_type: "parakeet_tdt"`, transformers modeling_parakeet.py / generation_parakeet.py /
 * loss/loss_tdt.py; csrc/transducer.hip).  fp32, fixed-order sums, no float atomics, bit-reproducible.
 *   dyn_lstm_cell_fwd     replaces the cell of torch.nn.LSTM (ParakeetRNNTDecoder.lstm): gates = xg + hg, both [Bd, 4 Hd] pre-activations in
 *                         torch's order i | f | g | o (xg = x W_ih^T + b_ih for all steps from one GEMM, hg = h W_hh^T + b_hh per step);
 *                         c = f * c_prev + i * g, h = o * tanh(c); `gates` (null: not saved) receives the four activations.  c_prev null = zeros.
 *   dyn_lstm_cell_bwd     replaces its autograd: from dh, dc_next (null = zeros), the saved gates, c_prev (null = zeros) and c, the
 *                         pre-activation gradients dgates [Bd, 4 Hd] and dc_prev.  The data and weight gradients are GEMMs of dgates.
 *   dyn_joint_fwd         replaces ACT2FN[hidden_act](encoder[:, :, None] + decoder[:, None]) of ParakeetRNNTJointNetwork.forward:
 *                         z[b, t, u, :] = relu(e[b, t, :] + p[b * p_stride_b + u * p_stride_u + :]); p_stride_b = 0 shares one p among the
 *                         batch rows.  act 0 = relu, anything else DYN_E_UNSUPPORTED.  Hd and the strides multiples of 4, 16-byte aligned.
 *   dyn_joint_bwd         replaces its autograd: de[b, t, :] = sum_u dz * [z > 0] (u ascending), dp[b, u, :] = sum_t the same (t ascending;
 *                         shared_p: one set of rows, summed over b ascending, then t).  de or dp may be null.
 *   dyn_tdt_loss          replaces transformers.loss.loss_tdt.tdt_loss and its autograd.  logits [B, T, U1, V1 + D] (V1 = vocabulary with the
 *                         blank, U1 = longest target + 1), targets int32 [B, S], per-row logit_lengths / target_lengths (clamped into
 *                         the tensor), `durations` a HOST array of 1 .. 8 strictly ascending non-negative values with at least one
 *                         positive.  Arcs from (t, u): a blank arc of every duration d > 0 to (t + d, u), a label arc of every duration
 *                         to (t + d, u + 1); the terminal sums the blank arcs with t + d == T_b at u == U_b; sigma is subtracted from the
 *                         token log-probs.  Four launches: arc log-probs (one wave per logits row: the two log-sum-exps, blank, label and
 *                         duration log-probs), alpha and beta over anti-diagonals (one workgroup per row and direction, a diagonal
 *                         strided over its threads, one barrier per diagonal, each diagonal stored relative to an integer base so that
 *                         the stored values stay O(1)), the reduction, and with `grad` the gradient of grad_scale * loss w.r.t. the
 *                         logits from the arc posteriors (rows at t >= T_b or u > U_b exact zeros; grad may be logits).  An unreachable
 *                         terminal gives nll = +inf and an all-zero gradient for that row.  reduction 0 sum, 1 mean_batch,
 *                         2 mean (nll_b / U_b, then the batch mean), 3 mean_volume, 4 none (loss = the sum; the rows in nll_per_row).
 *                         The whole lattice lives in `workspace`; workspace_budget_bytes > 0 refuses a larger one by name
 *                         (DYN_E_WORKSPACE).  This entry wants the whole logits tensor; the three below stream it over frame chunks.
 *   dyn_tdt_loss_workspace_layout   byte offsets of lp, lse, alpha, beta, abase, bbase, ll, nll in the workspace (tests).
 *   dyn_tdt_arcs_chunk / dyn_tdt_lattice_run / dyn_tdt_grad_chunk   dyn_tdt_loss in three passes, for a joint that is produced, consumed and
 *                         dropped a few frames at a time (and produced once more for the gradient).  `state` is a caller-owned buffer of
 *                         dyn_tdt_loss_workspace_bytes in dyn_tdt_loss_workspace_layout's layout; it must survive from the first arcs
 *                         chunk to the last gradient chunk.  A chunk is logits [B, Tc, U1, V1 + D] of the frames [t0, t0 + Tc) of the
 *                         lattice [B, T, U1] (0 <= t0 < T; it may overhang T: those rows are not read by the arcs pass and come out as
 *                         zeros of the gradient pass).  dyn_tdt_arcs_chunk writes lp and lse of the chunk's cells (every frame of the
 *                         lattice must be covered before the lattice runs); dyn_tdt_lattice_run is the alpha / beta launch (beta only
 *                         with want_beta: the gradient needs it), the reduction into loss and the per-row nll; dyn_tdt_grad_chunk writes
 *                         the chunk's gradient (grad may be its logits).  The same kernels as dyn_tdt_loss, a row's arithmetic depends on
 *                         its own logits and on the lattice state alone: every output is bit-equal to dyn_tdt_loss's on the whole tensor,
 *                         whatever the chunking.  state_budget_bytes > 0 refuses a larger lattice state by name (DYN_E_WORKSPACE):
 *                         only the joint is chunked, not the state.
 *   dyn_joint_bwd_chunk   dyn_joint_bwd on z / dz [B, Tc, U1, Hd] of a chunk of frames: de points at the chunk's first frame inside a
 *                         longer [B, T, Hd] (batch rows de_stride_b floats apart) and receives the same bits as those rows of
 *                         dyn_joint_bwd; with dp_accumulate = 1 the chunk's sum over its frames is ADDED to dp (0: written), so chunks
 *                         launched in ascending order on one stream give a fixed summation order, without float atomics.
 *   dyn_tdt_greedy_steps  replaces ParakeetTDTGenerationMixin's greedy loop, n_steps steps per call with all state on the device, in
 *                         the manner of dyn_decoder_steps.  istate int32 [6, B]: frame pointer, last token, emit flag, done flag, output
 *                         count, steps taken (the caller starts with last token = the start token and emit = 1: the first step then
 *                         primes the prediction network).  A step: if emit, the LSTM layers (one wave per hidden unit over [x ; h]) and
 *                         the projector on the last token; logits = head . relu(enc[frame] + dec); argmax over the V1 token and the D
 *                         duration logits (lowest index on ties); the frame pointer advances by durations[argmax], by 1 for a blank
 *                         with duration 0; a non-blank is appended to tokens / frames [B, n_max] and sets emit.  A row is done when
 *                         its pointer reaches valid[b], after max_steps steps or n_max outputs; a done row launches no work.
 *                         `lstm_ptrs`: DEVICE array of 4 * layers pointers (w_ih, w_hh, b_ih, b_hh per layer).
 *   dyn_rnnt_loss         replaces transformers.loss.loss_rnnt.rnnt_loss (loss/loss_rnnt.py:23-90, a wrapper around
 *                         torchaudio.functional.rnnt_loss) and its autograd, the head of ParakeetForRNNT (`model_type: "parakeet_rnnt"`,
 *                         modeling_parakeet.py:922-1032).  logits [B, T, U1, V1]: no duration columns.  Arcs from (t, u): a blank arc to
 *                         (t + 1, u), a label arc to (t, u + 1); the terminal is alpha(T_b - 1, U_b) + lp_blank(T_b - 1, U_b).  The same four
 *                         launches, integer bases, (integer, fraction) log-likelihood, reductions (0 sum, 1 mean_batch, 2 mean,
 *                         3 mean_volume, 4 none), length clamping, zeros outside [:T_b, :U_b + 1] and workspace budget as dyn_tdt_loss;
 *                         20 bytes of state per cell (lp 8, lse 4, alpha 4, beta 4).  A row with T_b == 0 has no terminal: nll = +inf, zero
 *                         gradient; so has a row whose lattice -inf logits cut.
 *   dyn_rnnt_loss_workspace_bytes / _layout   the state's size and the byte offsets of lp [.., 2], lse [.., 1], alpha, beta, abase, bbase,
 *                         ll, nll in it (tests).
 *   dyn_rnnt_arcs_chunk / dyn_rnnt_lattice_run / dyn_rnnt_grad_chunk   dyn_rnnt_loss in three passes against a caller-owned state, as the
 *                         three dyn_tdt_* chunk entries: the whole form is the chunk form at t0 = 0, Tc = T, every output bit-equal
 *                         whatever the chunking.
 *   dyn_rnnt_greedy_steps replaces ParakeetRNNTGenerationMixin's greedy loop (generation_parakeet.py:141-163,
 *                         _update_model_kwargs_for_generation).  dyn_tdt_greedy_steps's LSTM, projector and joint launches with N = V1;
 *                         istate int32 [7, B]: its six rows plus the symbols emitted at the current frame.  argmax over the row (lowest
 *                         index on ties); a blank advances the frame by one and resets the counter; a non-blank is emitted, feeds the
 *                         prediction network and increments it; when it reaches max_symbols the frame advances anyway and the counter
 *                         resets, the forced step's token still emitted and fed.  Done as in dyn_tdt_greedy_steps.
 * Null pointers and sizes out of range -> DYN_E_ARG, all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_lstm_cell_fwd(const float* xg, const float* hg, const float* c_prev, float* c, float* h, float* gates, int64_t Bd, int64_t Hd,
                      void* stream);
int dyn_lstm_cell_bwd(const float* dh, const float* dc_next, const float* gates, const float* c_prev, const float* c, float* dgates,
                      float* dc_prev, int64_t Bd, int64_t Hd, void* stream);
int dyn_joint_fwd(const float* e, const float* p, float* z, int64_t B, int64_t T, int64_t U1, int64_t Hd, int64_t p_stride_b,
                  int64_t p_stride_u, int32_t act, void* stream);
int dyn_joint_bwd(const float* dz, const float* z, float* de, float* dp, int64_t B, int64_t T, int64_t U1, int64_t Hd, int32_t shared_p,
                  int64_t dp_stride_b, int64_t dp_stride_u, int32_t act, void* stream);
int64_t dyn_tdt_loss_workspace_bytes(int64_t B, int64_t T, int64_t U1, int64_t D);
int dyn_tdt_loss_workspace_layout(int64_t B, int64_t T, int64_t U1, int64_t D, int64_t* offsets8);
int dyn_tdt_loss(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                 const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank,
                 float sigma, int32_t reduction, float grad_scale, float* loss, float* nll_per_row, float* grad, void* workspace,
                 int64_t workspace_bytes, int64_t workspace_budget_bytes, void* stream);
int dyn_tdt_arcs_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                       const int32_t* targets, int64_t S, const int32_t* target_lengths, int32_t blank, float sigma, int64_t t0, int64_t Tc,
                       void* state, int64_t state_bytes, int64_t state_budget_bytes, void* stream);
int dyn_tdt_lattice_run(int64_t B, int64_t T, int64_t U1, const int32_t* durations, int64_t D, int64_t S, const int32_t* logit_lengths,
                        const int32_t* target_lengths, int32_t reduction, float* loss, float* nll_per_row, int32_t want_beta, void* state,
                        int64_t state_bytes, int64_t state_budget_bytes, void* stream);
int dyn_tdt_grad_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* durations, int64_t D,
                       const int32_t* targets, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank,
                       int32_t reduction, float grad_scale, int64_t t0, int64_t Tc, float* grad, const void* state, int64_t state_bytes,
                       void* stream);
int dyn_joint_bwd_chunk(const float* dz, const float* z, float* de, float* dp, int64_t B, int64_t Tc, int64_t U1, int64_t Hd, int32_t shared_p,
                        int64_t de_stride_b, int64_t dp_stride_b, int64_t dp_stride_u, int32_t dp_accumulate, int32_t act, void* stream);
int dyn_tdt_greedy_steps(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs, const float* proj_w,
                         const float* proj_b, const float* head_w, const float* head_b, int32_t* istate, float* h, float* c, float* h_new,
                         float* dec, float* logits, int32_t* tokens, int32_t* frames, int64_t B, int64_t T, int64_t Hd, int64_t layers,
                         int64_t V1, const int32_t* durations, int64_t D, int32_t blank, int64_t n_max, int64_t max_steps,
                         int32_t n_steps, void* stream);
int64_t dyn_rnnt_loss_workspace_bytes(int64_t B, int64_t T, int64_t U1);
int dyn_rnnt_loss_workspace_layout(int64_t B, int64_t T, int64_t U1, int64_t* offsets8);
int dyn_rnnt_loss(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                  const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank, int32_t reduction, float grad_scale, float* loss,
                  float* nll_per_row, float* grad, void* workspace, int64_t workspace_bytes, int64_t workspace_budget_bytes, void* stream);
int dyn_rnnt_arcs_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                        const int32_t* target_lengths, int32_t blank, int64_t t0, int64_t Tc, void* state, int64_t state_bytes,
                        int64_t state_budget_bytes, void* stream);
int dyn_rnnt_lattice_run(int64_t B, int64_t T, int64_t U1, int64_t S, const int32_t* logit_lengths, const int32_t* target_lengths,
                         int32_t reduction, float* loss, float* nll_per_row, int32_t want_beta, void* state, int64_t state_bytes,
                         int64_t state_budget_bytes, void* stream);
int dyn_rnnt_grad_chunk(const float* logits, int64_t B, int64_t T, int64_t U1, int64_t V1, const int32_t* targets, int64_t S,
                        const int32_t* logit_lengths, const int32_t* target_lengths, int32_t blank, int32_t reduction, float grad_scale,
                        int64_t t0, int64_t Tc, float* grad, const void* state, int64_t state_bytes, void* stream);
int dyn_rnnt_greedy_steps(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs, const float* proj_w,
                          const float* proj_b, const float* head_w, const float* head_b, int32_t* istate, float* h, float* c, float* h_new,
                          float* dec, float* logits, int32_t* tokens, int32_t* frames, int64_t B, int64_t T, int64_t Hd, int64_t layers,
                          int64_t V1, int32_t blank, int64_t max_symbols, int64_t n_max, int64_t max_steps, int32_t n_steps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * NemotronAsrStreamingForRNNT (`model_type: "nemotron_asr_streaming"`, transformers modeling_nemotron_asr_streaming.py): the encoder's
 * three differences from Parakeet's.  fp32, deterministic, no float atomics.
 *
 * Chunked limited-context attention (chunked_limited_mask_function, :870-883, applied by NemotronAsrStreamingEncoder.forward :981-988 and
 * NemotronAsrStreamingEncoderAttention.forward :619-628: `_rel_shift`, `masked_fill_(attention_mask.logical_not(), -inf)`, the softmax
 * of eager_attention_forward).  cs = lookahead + 1 frames per chunk, lc left chunks (lc < 0: unlimited); query i sees key j iff
 * 0 <= i / cs - j / cs <= lc, the contiguous range [j0, j1) = [max(0, i / cs - lc) * cs, min(T, (i / cs + 1) * cs)).  With
 * dlo = min(lc * cs + cs - 1, T - 1) and dhi = min(cs - 1, T - 1), j - i lies in [-dlo, dhi]: W = dlo + dhi + 1 relative positions.
 * bd is the BAND product (q + v) P_h[T - 1 - dlo .. T - 1 + dhi]^T [M, T, ld_bd >= W], already scaled; relative position -dlo is column 0.
 *   dyn_softmax_relshift_band_fwd  y[m,i,j] = softmax over [j0, j1) of x[m,i,j] + bd[m, i, j - i + dlo]; 0 WRITTEN in every other column
 *                                  of the row.  y may be x (not bd).  One pass, nothing copied for the shift.  T <= 16384.
 *   dyn_relshift_band_bwd          dBD[m,i,k] = dS[m, i, k - dlo + i] where that key lies in [j0, j1), 0 WRITTEN in every other column of
 *                                  the ld_bd-float row: the buffer may be uninitialised scratch.
 * cs >= T is one chunk and lc >= T every chunk (both are clamped).  Null pointer, T < 1, cs < 1, ld_bd < W, T beyond the row limit
 * -> DYN_E_ARG before any launch.
 *
 * Causal x8 subsampling (NemotronAsrStreamingEncoderCausalConv2D.forward :305-316: padding (kernel - 1, stride - 1) = (2, 1) on both
 * axes; NemotronAsrStreamingEncoderSubsamplingConv2D.forward :718-729).  To = T / 2 + 1, Fo = F / 2 + 1, output (to, fo) reads the inputs
 * (2 to + dt - 2, 2 fo + df - 2).  Channels-last, w [C, 3, 3], C % 4 == 0, any T >= 1 and F >= 1.
 *   dyn_conv2d_first_causal_fwd / _wgrad   `conv_in`: x [B, T, F] -> z [B, To, Fo, C] (pre-activation); dw [C, 9] and dbias [C] as
 *                                          beta * old + the sums, per-tile partials in `workspace` combined in tile order (deferrable).
 *   dyn_dwconv2d_s2_causal_fwd_act / _dgrad_act / _wgrad_act   `layers.{i}.depthwise_conv` with `act_fn` of its input fused into the
 *                                          loads, the contracts of dyn_dwconv2d_s2_*_act: u = bias + dw3x3(act(z)), dz = act'(z) * ...;
 *                                          act 1 = ReLU (0, SiLU, has no caller and is DYN_E_UNSUPPORTED).
 *
 * Conv-module core (NemotronAsrStreamingEncoderConvolutionModule.forward :454-469: `glu`, the left-padded `depthwise_conv` with its
 * optional bias, `self.norm` = LayerNorm(C), `self.activation` = SiLU) at KW = 9, C in {256, 512, 768, 1024}.
 *   dyn_convmod_causal_k9_fwd      u [B, T, 2C] -> s [B, T, C] in one launch; cbias may be null; optional outputs g, c, n [B, T, C] and
 *                                  mean / rstd [B * T] as dyn_convmod_causal_fwd.
 *   dyn_dwconv1d_causal_k9_dgrad / _wgrad   the contracts of dyn_dwconv1d_causal_dgrad / _wgrad at 9 taps (the bias gradient is dyn_colsum
 *                                  of dy).
 * A C / KW / act that is not built -> DYN_E_UNSUPPORTED, a short workspace -> DYN_E_WORKSPACE, all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_softmax_relshift_band_fwd(const float* x, float* y, const float* bd, int64_t M, int64_t T, int64_t ld_bd, int64_t cs, int64_t lc,
                                  void* stream);
int dyn_relshift_band_bwd(const float* dS, float* dBD, int64_t M, int64_t T, int64_t ld_bd, int64_t cs, int64_t lc, void* stream);
int dyn_conv2d_first_causal_fwd(const float* x, const float* w, const float* bias, float* z, int64_t B, int64_t T, int64_t F, int64_t C,
                                void* stream);
int64_t dyn_conv2d_causal_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C);
int dyn_conv2d_first_causal_wgrad(const float* x, const float* dz, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                                  int64_t C, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_dwconv2d_s2_causal_fwd_act(const float* z, const float* w, const float* bias, float* u, int64_t B, int64_t T, int64_t F, int64_t C,
                                   int32_t act, void* stream);
int dyn_dwconv2d_s2_causal_dgrad_act(const float* z, const float* w, const float* du, float* dz, int64_t B, int64_t T, int64_t F, int64_t C,
                                     int32_t act, void* stream);
int dyn_dwconv2d_s2_causal_wgrad_act(const float* z, const float* du, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                                     int64_t C, int32_t act, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_convmod_causal_k9_fwd(const float* u, const float* w, const float* cbias, const float* gamma, const float* beta, float* s, float* g,
                              float* c, float* n, float* mean, float* rstd, int64_t B, int64_t T, int64_t C, int64_t KW, float eps,
                              void* stream);
int dyn_dwconv1d_causal_k9_dgrad(const float* dy, const float* w, float* dx, int64_t B, int64_t T, int64_t C, int64_t KW, float dx_beta,
                                 void* stream);
int64_t dyn_dwconv1d_causal_k9_wgrad_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t KW);
int dyn_dwconv1d_causal_k9_wgrad(const float* x, const float* dy, float* dw, float beta, int64_t B, int64_t T, int64_t C, int64_t KW,
                                 void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * NemotronAsrStreamingForRNNT, cache-aware streaming (transformers modeling_nemotron_asr_streaming.py with `use_cache=True`, and
 * generation_nemotron_asr_streaming.py): one STEP takes cs = lookahead + 1 encoder frames of B streams.  `counter` is a device int32:
 * counter[0] = the chunks consumed so far.  Every kernel reads the ring slot, the warm-up count and the state half from it, so a step's
 * launches have the same arguments every time (csrc/stream.hip).  lc = (sliding_window - 1) / cs cached chunks are visible.
 *   dyn_stream_advance        counter[0] += 1: the last launch of a step.
 *   dyn_stream_attn           replaces, for one layer and chunk, `past_key_values.update` (DynamicSlidingWindowLayer), the two head
 *                             biases, `relative_k_proj`'s product with the query, `_rel_shift`, the chunked mask, eager_attention_forward
 *                             (NemotronAsrStreamingEncoderAttention.forward :599-642).  qkv [B, cs, 3H] packed q | k | v, bias_u / bias_v
 *                             [H], pos [W, H] = relative_k_proj of the W = lc cs + 2 cs - 1 sinusoid rows of the distances
 *                             lc cs + cs - 1 .. -(cs - 1) (the same on every step), k_cache / v_cache [B, lc + 1, cs, H] rings (the chunk
 *                             of step s in slot s % (lc + 1)), out [B, cs, H].  Every query sees the min(s, lc) cs cached frames and the
 *                             whole chunk: softmax(((q + u) K^T + (q + v) P[distance]^T) scale) V, the chunk's k / v stored.  One workgroup
 *                             per (head, stream); dyn_stream_attn_lds_bytes of LDS (-1: bad sizes), over a CU's 160 KiB ->
 *                             DYN_E_UNSUPPORTED.  D % 4 == 0.  lc = 0: no cached keys.
 *   dyn_stream_convmod_k9     dyn_convmod_causal_k9_fwd with the padding cache of NemotronAsrStreamingEncoderCausalConv1dCacheLayer.update
 *                             (:81-104, both branches of `shortfall`): state [2, B, 8, C] GLU frames, half counter & 1 read (the 8 frames
 *                             left of the chunk), the last 8 frames of state + chunk written to the other half.  u [B, T, 2C] -> s [B, T, C].
 *   dyn_stream_conv2d_first / dyn_stream_dwconv2d_s2_act   dyn_conv2d_first_causal_fwd / dyn_dwconv2d_s2_causal_fwd_act under
 *                             NemotronAsrStreamingEncoderCausalConv2dCacheLayer.update (:125-149): carry [2, B, F] / [2, B, F, C] holds the
 *                             last input row of the previous chunk (before the ReLU), no padding on the right in time;
 *                             `first` = 1 puts two zero rows in its place (`left_pad_init`).  To = (T + left - 3) / 2 + 1 with left = 1
 *                             (first: 2), Fo = F / 2 + 1.  The new carry is written to the other half in the same launch.
 *   dyn_rnnt_greedy_steps_chunk   dyn_rnnt_greedy_steps on the frames of one streamed chunk: `rebase` = 1 first points the frame pointer at
 *                             frame 0, clears the done flags, the per-frame symbol counter and the chunk's output and step counts and
 *                             keeps h / c, the projector cache, the last token and the emit flag; emitted frames are recorded as
 *                             frame_base + the frame inside the chunk.
 * Null pointers and sizes out of range -> DYN_E_ARG, a width that is not built -> DYN_E_UNSUPPORTED, all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_stream_advance(int32_t* counter, void* stream);
int64_t dyn_stream_attn_lds_bytes(int64_t cs, int64_t lc, int64_t D);
int dyn_stream_attn(const float* qkv, const float* bias_u, const float* bias_v, const float* pos, float* k_cache, float* v_cache,
                    const int32_t* counter, float* out, int64_t B, int64_t cs, int64_t lc, int64_t nh, int64_t D, float scale, void* stream);
int dyn_stream_convmod_k9(const float* u, const float* w, const float* cbias, const float* gamma, const float* beta, float* state,
                          const int32_t* counter, float* s, int64_t B, int64_t T, int64_t C, int64_t KW, float eps, void* stream);
int dyn_stream_conv2d_first(const float* x, const float* w, const float* bias, float* carry, const int32_t* counter, float* z, int64_t B,
                            int64_t T, int64_t F, int64_t C, int32_t first, void* stream);
int dyn_stream_dwconv2d_s2_act(const float* z, const float* w, const float* bias, float* carry, const int32_t* counter, float* u, int64_t B,
                               int64_t T, int64_t F, int64_t C, int32_t act, int32_t first, void* stream);
int dyn_rnnt_greedy_steps_chunk(const float* enc, const int32_t* valid, const float* embed, const void* const* lstm_ptrs, const float* proj_w,
                                const float* proj_b, const float* head_w, const float* head_b, int32_t* istate, float* h, float* c,
                                float* h_new, float* dec, float* logits, int32_t* tokens, int32_t* frames, int64_t B, int64_t T, int64_t Hd,
                                int64_t layers, int64_t V1, int32_t blank, int64_t max_symbols, int64_t n_max, int64_t max_steps,
                                int32_t n_steps, int64_t frame_base, int32_t rebase, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Nemotron3_5AsrForRNNT, language-prompt fusion (transformers modeling_nemotron3_5_asr.py, Nemotron3_5AsrForRNNT.get_audio_features:
 * `one_hot`, `expand`, `torch.cat`, Nemotron3_5AsrPromptProjector.forward's `linear_1` and `act`) and its autograd, csrc/prompt_fuse.hip.
 * linear_1(cat([h, onehot(p_b)])) = h W1[:, :H]^T + (b1 + W1[:, H + p_b]): the K = H product stays on dyn_gemm_f32 (z [B, T, I], no
 * bias), the prompt is a per-batch-row bias.  w1p [I, Np] is the prompt block W1[:, H:] kept contiguous; prompt_ids int32 [B] in DEVICE
 * memory, read when the kernels run.  The caller validates the ids against [0, Np); no kernel reads outside the table for any id: the
 * gather CLAMPS an id into [0, Np - 1], the backward only compares ids with column numbers (an id outside the table adds to db1 alone).
 *   dyn_prompt_bias_gather   pb[b, j] = b1[j] + w1p[j, p_b], pb [B, I].
 *   dyn_prompt_relu_fwd      a[b, t, j] = max(z[b, t, j] + pb[b, j], 0) in one pass (a may be z): replaces the concat copy, the bias add
 *                            and dyn_relu_fwd.  ReLU'(0) = 0 as dyn_relu_bwd.
 *   dyn_prompt_relu_bwd      one pass over (a, da): dz = a > 0 ? da : 0 (dz may be da), per-(b, row tile) partial column sums in
 *                            `workspace` (tiles of dyn_prompt_relu_bwd_row_tile(T) rows, summed in row order); then s[b, :] = the tiles
 *                            of b in tile order, db1[j] = beta * db1[j] + sum_b s[b, j] (b ascending) and, for every p in 0 .. Np - 1,
 *                            dw1p[j, p] = beta * dw1p[j, p] + sum over the b with p_b = p of s[b, j] (b ascending).  A column of a
 *                            prompt no row used is exactly beta * old: zeros at beta = 0, untouched at beta = 1.  No float atomics,
 *                            bit-reproducible; not deferrable (the segment sum is not dyn_reduce_defer's column sum).  db1 / dw1p may be
 *                            null (frozen); with both null only dz is written and ids and workspace are not needed.  Replaces
 *                            dyn_relu_bwd, dyn_colsum and a weight-gradient GEMM over a [rows, Np] one-hot.
 * fp32, 16-byte aligned operands, I % 4 == 0, 1 <= B <= 65535, else DYN_E_ARG; a short workspace -> DYN_E_WORKSPACE; all before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_prompt_bias_gather(const float* b1, const float* w1p, const int32_t* prompt_ids, float* pb, int64_t B, int64_t I, int64_t Np,
                           void* stream);
int dyn_prompt_relu_fwd(const float* z, const float* pb, float* a, int64_t B, int64_t T, int64_t I, void* stream);
int64_t dyn_prompt_relu_bwd_row_tile(int64_t T);
int64_t dyn_prompt_relu_bwd_workspace_bytes(int64_t B, int64_t T, int64_t I);
int dyn_prompt_relu_bwd(const float* a, const float* da, float* dz, const int32_t* prompt_ids, float* db1, float* dw1p, float beta, int64_t B,
                        int64_t T, int64_t I, int64_t Np, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ragged batches of the FastConformer encoder (transformers modeling_parakeet.py with an `attention_mask`): one frame count per batch
 * entry, `lens` int32 [B] on the device, read when the kernel runs and clamped there as the scalar `valid` of the entries beside them
 * (the softmax into [1, T], the others into [0, T]).  The entries above keep their signatures and their bits.
 *   dyn_conv2d_first_fwd_lens      dyn_conv2d_first_fwd with feature frames t >= lens[b] read as zeros whatever they hold (the extractor's
 *                                  `input_features *= mask`; ParakeetEncoderSubsamplingConv2D.forward reads frame L of an odd length L
 *                                  before it masks anything).  Every row of z is written.
 *   dyn_dwconv2d_s2_fwd_act_lens   dyn_dwconv2d_s2_fwd_act with input rows t >= lens_in[b] read as zeros and output rows to >= lens_out[b]
 *                                  written as zeros: `hidden_states *= channel_mask[:, None, :, None]` after the Conv2d in front of this
 *                                  stage (its rows past the length, the pointwise conv's bias rows included) and after this one
 *                                  (ParakeetEncoderSubsamplingConv2D.forward, "mask the hidden states"), with no pass of their own.
 *   dyn_dwconv2d_s2_dgrad_act_lens its data gradient: dz rows t >= lens_in[b] are zeros, du rows to >= lens_out[b] are not read.
 *   dyn_dwconv2d_s2_wgrad_act_lens / dyn_conv2d_first_wgrad_lens
 *                                  the weight gradients with input rows t >= lens_in[b] (feature frames t >= lens[b]) read as zeros, as
 *                                  the forward read them; the output gradient is zero past the output length already.
 *   dyn_mask_rows_lens             x [B, T, W] in place, rows t >= lens[b] := 0 (the same mask behind the last 1x1 Conv2d, a small tensor).
 *   dyn_convmod_bn_fwd_lens / dyn_convmod_bn_bwd_act_lens / dyn_glu_dwconv1d_dgrad_lens
 *                                  the three conv-module entries with lens[b] in the place of *valid: GLU rows t >= lens[b] read as zeros
 *                                  (ParakeetEncoderConvolutionModule.forward, `hidden_states.masked_fill(all_masked_rows, 0.0)`), rows
 *                                  past it of every output exact zeros and left out of the three column sums.  The kernels are the scalar
 *                                  entries': they read valid[b * vstride], vstride 0 there and 1 here.
 *   dyn_softmax_relshift_fwd_lens  dyn_softmax_relshift_fwd_len on x [B, nh, T, T] with lens[b] keys in every row of batch entry b
 *                                  (ParakeetEncoder.forward's `attention_mask & attention_mask.transpose(1, 2)` for a valid query): columns
 *                                  >= lens[b] are outside max and sum and get probability 0.  A padded query row is a softmax over the
 *                                  row's valid keys: finite, without meaning.
 *   dyn_softmax_fwd_lens           dyn_softmax_fwd_len on x [B, rows_per, L] with lens[b] keys in every row of batch entry b: the teacher-forced
 *                                  cross-attention of CohereAsr (transformers' `encoder_attention_mask` on the scores [B, nh, S, T']); the
 *                                  per-row count is relshift's (softmax_row.h).
 *   dyn_seq2seq_steps_len          dyn_seq2seq_steps with enc_lens[r] (device int32 [rows], clamped into [1, n_enc]) encoder keys in row r's
 *                                  cross-attention; the descriptor keeps its layout, n_enc is the batch's maximum (strides, LDS).  Row r is
 *                                  bit-equal to the same row stepped alone with n_enc = enc_lens[r] at the same cross_stride.
 * The stage entries need C % 4 == 0 and 16-byte aligned tensors (DYN_E_UNSUPPORTED otherwise); a null `lens` is DYN_E_ARG.
 * ------------------------------------------------------------------------------------------------ */
int dyn_conv2d_first_fwd_lens(const float* x, const float* w, const float* bias, float* z, int64_t B, int64_t T, int64_t F, int64_t C,
                              const int32_t* lens, void* stream);
int dyn_dwconv2d_s2_fwd_act_lens(const float* z, const float* w, const float* bias, float* u, int64_t B, int64_t T, int64_t F, int64_t C,
                                 int32_t act, const int32_t* lens_in, const int32_t* lens_out, void* stream);
int dyn_dwconv2d_s2_dgrad_act_lens(const float* z, const float* w, const float* du, float* dz, int64_t B, int64_t T, int64_t F, int64_t C,
                                   int32_t act, const int32_t* lens_in, const int32_t* lens_out, void* stream);
int dyn_dwconv2d_s2_wgrad_act_lens(const float* z, const float* du, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                                   int64_t C, int32_t act, const int32_t* lens_in, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_conv2d_first_wgrad_lens(const float* x, const float* dz, float* dw, float* dbias, float beta, int64_t B, int64_t T, int64_t F,
                                int64_t C, const int32_t* lens, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_mask_rows_lens(float* x, int64_t B, int64_t T, int64_t W, const int32_t* lens, void* stream);
int dyn_convmod_bn_fwd_lens(const float* u, const float* w, const float* cbias, const float* mean, const float* var, const float* weight,
                            const float* bias, float* s, float* gl, float* c, const int32_t* lens, int64_t B, int64_t T, int64_t C,
                            int64_t KW, int32_t act, float eps, void* stream);
int dyn_convmod_bn_bwd_act_lens(const float* c, const float* mean, const float* var, const float* weight, const float* bias, const float* ds,
                                float* dc, float* dweight, float* dbias, float* dcbias, float wgrad_beta, const int32_t* lens, int64_t B,
                                int64_t T, int64_t C, int32_t act, float eps, void* workspace, int64_t workspace_bytes, void* stream);
int dyn_glu_dwconv1d_dgrad_lens(const float* u, const float* w, const float* dc, float* du, const int32_t* lens, int64_t B, int64_t T,
                                int64_t C, int64_t KW, void* stream);
int dyn_softmax_relshift_fwd_lens(const float* x, float* y, const float* bd, int64_t B, int64_t nh, int64_t T, int64_t ld_bd,
                                  const int32_t* lens, void* stream);
int dyn_softmax_fwd_lens(const float* x, float* y, int64_t B, int64_t rows_per, int64_t L, int64_t ldx, int64_t ldy, const int32_t* lens,
                         void* stream);
int dyn_seq2seq_steps_len(const dyn_seq2seq_desc* d, const int32_t* enc_lens, int32_t t0, int32_t n_steps, int32_t n_forced, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Waveform front end of the FastConformer family (csrc/melfeat.hip): the two ends of transformers' ParakeetFeatureExtractor /
 * NemotronAsrStreamingFeatureExtractor / CohereAsrFeatureExtractor / LasrFeatureExtractor `__call__` around the strided-row STFT GEMM,
 * dyn_stft_power and the mel GEMM, for a ragged batch.  The reference's third loop gets its `spec` from `get_spectrogram` / `preprocess`
 * (nvidia_ctc/lib.py:20-28), NeMo's preprocessor on the CPU.
 *   dyn_melfeat_prep     x [B, Lmax], lens int32 [B] on the device (clamped into [0, Lmax]) -> out [B, W], W >= pad + Lmax: element i of row b
 *                        is sample j = i - pad after `waveform[:valid] += dither * noise` (noise [B, Lmax], null: none), the pre-emphasis
 *                        `x[j] - preemphasis * x[j - 1]` over the whole signal (sample 0 kept, or filtered against prev[b] when `prev`
 *                        [B] is given: the last sample of the chunk before, for streams; preemphasis 0: none) and
 *                        `masked_fill(~timemask, 0.0)`: exact zeros for j < 0 and j >= lens[b], sample lens[b] included.  Every element of out
 *                        is written; samples at or past lens[b] are never read.  One rounding per operation, as the extractor's float32.
 *   dyn_melfeat_finish   mel [B, T, F] energies, lens int32 [B] valid frames per row (clamped into [0, T]) -> out [B, T, F] (layout 0) or
 *                        [B, F, T] (layout 1): v = log(mel + guard) (clamp 0) or log(max(mel, guard)) (clamp 1); normalize != 0:
 *                        (v - mean) / (std + eps) with the mean and the UNBIASED std per row and bin over the row's valid frames (the mean
 *                        first, then the centred squares in a second pass, per 256-frame block and then over the blocks in double, in
 *                        a fixed order, no float atomics; a bin of equal values gives exact zeros).  Frames >= lens[b] are exact zeros.
 *                        F <= 256; out must not alias mel; workspace 8-byte aligned, dyn_melfeat_finish_workspace_bytes(B, T, F) bytes.
 * Null pointers and sizes out of range -> DYN_E_ARG, a small or misaligned workspace -> DYN_E_WORKSPACE, before any launch.
 * ------------------------------------------------------------------------------------------------ */
int dyn_melfeat_prep(const float* x, float* out, const int32_t* lens, const float* noise, const float* prev, int64_t B, int64_t Lmax,
                     int64_t pad, int64_t W, float preemphasis, float dither, void* stream);
int64_t dyn_melfeat_finish_workspace_bytes(int64_t B, int64_t T, int64_t F);
int dyn_melfeat_finish(const float* mel, float* out, const int32_t* lens, int64_t B, int64_t T, int64_t F, float guard, int32_t clamp,
                       int32_t normalize, float eps, int32_t layout, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNEVAL_H_ */
