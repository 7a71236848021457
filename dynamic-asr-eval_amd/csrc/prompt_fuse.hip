// Language-prompt fusion of Nemotron3_5AsrForRNNT (transformers modeling_nemotron3_5_asr.py, get_audio_features):
//   fused = linear_2(relu(linear_1(cat([h, one_hot(prompt_id)[:, None, :].expand(T)], -1))))
// rests on   linear_1(cat([h, onehot(p_b)])) = h W1[:, :H]^T + (b1 + W1[:, H + p_b]):
// the one-hot never exists, the main block is an ordinary K = H product on the GEMM, and the prompt is a per-batch-row bias vector pb[b, :]
// of I floats gathered from one column of the prompt block W1p = W1[:, H:] ([I, Np], kept contiguous).  What is left is bandwidth work:
//   gather   pb[b, j] = b1[j] + W1p[j, p_b]                                  (B x I floats, once per call or per streaming session)
//   forward  a[b, t, j] = max(z[b, t, j] + pb[b, j], 0)                      (one pass: z read once, a written once; in place allowed)
//   backward dz = da * [a > 0] (in place over da allowed), and the sums behind db1 and dW1p:
//            s[b, j]      = sum_t dz[b, t, j]      per-(b, row tile) partial rows, row order inside a tile, then tiles in tile order
//            db1[j]       = beta * db1[j]      + sum_b s[b, j]                    b ascending
//            dW1p[j, p]   = beta * dW1p[j, p]  + sum_{b : p_b = p} s[b, j]        b ascending: a segment sum over batch rows by prompt id
// No float atomics, every order fixed: bit-reproducible.  A column of a prompt no row used is exactly beta * old: zeros at beta = 0, the
// old bits at beta = 1 (the column is not touched then, so not even -0 becomes +0).
// The ids are read from device memory when the kernels run (a captured streaming step holds only their address).  The caller validates
// them against [0, Np) on the host; the kernels still never read outside the table: the gather CLAMPS an id into [0, Np - 1], the
// backward compares ids with column numbers and never indexes with them, so a row with an id outside the table adds to db1 only.
// The finalise does not go through the deferred-reduction arena (common.h): its segment sum is not the arena's plain column sum, nothing
// else writes db1 / dW1p, and its partials live in the caller's workspace between three launches on one stream.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int ROW_TILE = 8;           // rows of one batch entry a workgroup of the backward sums at least
constexpr int MAX_TILES = 64;         // row tiles per batch entry at most (longer inputs get longer tiles)

__global__ __launch_bounds__(TPB) void prompt_gather_kernel(const float* __restrict__ b1, const float* __restrict__ w1p,
                                                             const int32_t* __restrict__ ids, float* __restrict__ pb, int64_t B, int I, int Np) {
    const int64_t total = B * I;
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
        const int64_t b = idx / I;
        const int j = (int)(idx % I);
        int p = ids[b];
        p = p < 0 ? 0 : (p >= Np ? Np - 1 : p);                // clamped: never a read outside the table
        pb[idx] = b1[j] + w1p[(int64_t)j * Np + p];
    }
}

// a = max(z + pb[b], 0), four columns per thread; a may be z.
__global__ __launch_bounds__(TPB) void prompt_relu_fwd_kernel(const float* z, const float* __restrict__ pb, float* a, int64_t total4,
                                                               int64_t TI4, int I4) {
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * TPB) {
        const int64_t b = idx / TI4;
        const int c4 = (int)(idx % I4);
        const float4 x = reinterpret_cast<const float4*>(z)[idx];
        const float4 p = reinterpret_cast<const float4*>(pb)[b * I4 + c4];
        float4 y;
        y.x = fmaxf(x.x + p.x, 0.f);
        y.y = fmaxf(x.y + p.y, 0.f);
        y.z = fmaxf(x.z + p.z, 0.f);
        y.w = fmaxf(x.w + p.w, 0.f);
        reinterpret_cast<float4*>(a)[idx] = y;
    }
}

// Workgroup (tile, b, column block): the rows [tile * per, tile * per + per) of batch entry b, four columns per thread.  dz = a > 0 ? da : 0
// (dz may be da), and, with `part` non-null, the tile's column sums in row order as one partial row part[b, tile, :].
__global__ __launch_bounds__(TPB) void prompt_relu_bwd_kernel(const float* __restrict__ a, const float* da, float* dz, float* __restrict__ part,
                                                               int64_t T, int64_t per, int I4) {
    const int c4 = blockIdx.z * TPB + threadIdx.x;
    if (c4 >= I4) return;
    const int64_t b = blockIdx.y, tiles = gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * per;
    const int64_t t1 = t0 + per < T ? t0 + per : T;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t at = (b * T + t) * I4 + c4;
        const float4 y = reinterpret_cast<const float4*>(a)[at];
        float4 g = reinterpret_cast<const float4*>(da)[at];
        g.x = y.x > 0.f ? g.x : 0.f;
        g.y = y.y > 0.f ? g.y : 0.f;
        g.z = y.z > 0.f ? g.z : 0.f;
        g.w = y.w > 0.f ? g.w : 0.f;
        reinterpret_cast<float4*>(dz)[at] = g;
        s.x += g.x;
        s.y += g.y;
        s.z += g.z;
        s.w += g.w;
    }
    if (part) reinterpret_cast<float4*>(part)[(b * tiles + blockIdx.x) * I4 + c4] = s;
}

// s[b, j] = the tiles of b in tile order.
__global__ __launch_bounds__(TPB) void prompt_rows_kernel(const float* __restrict__ part, float* __restrict__ s, int64_t B, int64_t tiles, int I) {
    const int64_t total = B * I;
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
        const int64_t b = idx / I;
        const int j = (int)(idx % I);
        float acc = 0.f;
        for (int64_t k = 0; k < tiles; ++k) acc += part[(b * tiles + k) * I + j];
        s[idx] = acc;
    }
}

// One thread per element (j, p) of dW1p [I, Np], p fastest (coalesced stores); the threads of p == 0 also write db1[j].  Either output may
// be null.
__global__ __launch_bounds__(TPB) void prompt_finalise_kernel(const float* __restrict__ s, const int32_t* __restrict__ ids, float* __restrict__ db1,
                                                               float* __restrict__ dw1p, float beta, int64_t B, int I, int Np) {
    const int64_t total = (int64_t)I * Np;
    for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
        const int j = (int)(idx / Np), p = (int)(idx % Np);
        float all = 0.f, mine = 0.f;
        bool hit = false;
        for (int64_t b = 0; b < B; ++b) {
            const float v = s[b * I + j];
            all += v;
            if (ids[b] == p) {
                mine += v;
                hit = true;
            }
        }
        if (dw1p) {
            if (hit) dw1p[idx] = beta == 0.f ? mine : beta * dw1p[idx] + mine;
            else if (beta != 1.f) dw1p[idx] = beta == 0.f ? 0.f : beta * dw1p[idx];     // beta = 1: the old bits stay
        }
        if (db1 && p == 0) db1[j] = beta == 0.f ? all : beta * db1[j] + all;
    }
}

int64_t row_tiles(int64_t T, int64_t* per) {
    const int64_t rows = T > 0 ? T : 1;
    int64_t tiles = dyn::cdiv(rows, ROW_TILE);
    if (tiles > MAX_TILES) tiles = MAX_TILES;
    *per = dyn::cdiv(rows, tiles);
    return dyn::cdiv(rows, *per);
}

unsigned grid_for(int64_t items) {
    int64_t g = dyn::cdiv(items, TPB);
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_sizes(const char* who, int64_t B, int64_t T, int64_t I) {
    DYN_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1ll << 31) && I >= 4 && I <= (1 << 20), DYN_E_ARG, "%s: bad sizes B=%lld T=%lld I=%lld",
                who, (long long)B, (long long)T, (long long)I);
    DYN_REQUIRE(I % 4 == 0, DYN_E_ARG, "%s: I=%lld must be a multiple of 4 (16-byte rows)", who, (long long)I);
    DYN_REQUIRE(B * T <= (1ll << 40) / I, DYN_E_ARG, "%s: B * T * I too large for one launch", who);
    return DYN_OK;
}

}  // namespace

extern "C" int dyn_prompt_bias_gather(const float* b1, const float* w1p, const int32_t* prompt_ids, float* pb, int64_t B, int64_t I, int64_t Np,
                                      void* stream) {
    DYN_REQUIRE(b1 && w1p && prompt_ids && pb, DYN_E_ARG, "dyn_prompt_bias_gather: null pointer");
    if (int rc = check_sizes("dyn_prompt_bias_gather", B, 1, I)) return rc;
    DYN_REQUIRE(Np >= 1 && Np <= (1 << 20), DYN_E_ARG, "dyn_prompt_bias_gather: num_prompts=%lld out of range", (long long)Np);
    DYN_REQUIRE(aligned16(b1) && aligned16(w1p) && aligned16(pb) && ((uintptr_t)prompt_ids & 3) == 0, DYN_E_ARG,
                "dyn_prompt_bias_gather: b1, w1p and pb must be 16-byte aligned, the ids 4-byte aligned");
    hipLaunchKernelGGL(prompt_gather_kernel, dim3(grid_for(B * I)), dim3(TPB), 0, (hipStream_t)stream, b1, w1p, prompt_ids, pb, B, (int)I, (int)Np);
    return dyn::check_launch("dyn_prompt_bias_gather");
}

extern "C" int dyn_prompt_relu_fwd(const float* z, const float* pb, float* a, int64_t B, int64_t T, int64_t I, void* stream) {
    DYN_REQUIRE(z && pb && a, DYN_E_ARG, "dyn_prompt_relu_fwd: null pointer");
    if (int rc = check_sizes("dyn_prompt_relu_fwd", B, T, I)) return rc;
    DYN_REQUIRE(aligned16(z) && aligned16(pb) && aligned16(a), DYN_E_ARG, "dyn_prompt_relu_fwd: operands must be 16-byte aligned");
    DYN_REQUIRE((const void*)a != (const void*)pb, DYN_E_ARG, "dyn_prompt_relu_fwd: the output may alias z, not pb");
    const int64_t I4 = I / 4;
    hipLaunchKernelGGL(prompt_relu_fwd_kernel, dim3(grid_for(B * T * I4)), dim3(TPB), 0, (hipStream_t)stream, z, pb, a, B * T * I4, T * I4, (int)I4);
    return dyn::check_launch("dyn_prompt_relu_fwd");
}

extern "C" int64_t dyn_prompt_relu_bwd_row_tile(int64_t T) {
    if (T < 1) return -1;
    int64_t per;
    row_tiles(T, &per);
    return per;
}

extern "C" int64_t dyn_prompt_relu_bwd_workspace_bytes(int64_t B, int64_t T, int64_t I) {
    if (B < 1 || T < 1 || I < 1) return 0;
    int64_t per;
    return (row_tiles(T, &per) + 1) * B * I * (int64_t)sizeof(float);      // the partial rows, then s [B, I]
}

extern "C" int dyn_prompt_relu_bwd(const float* a, const float* da, float* dz, const int32_t* prompt_ids, float* db1, float* dw1p, float beta,
                                   int64_t B, int64_t T, int64_t I, int64_t Np, void* workspace, int64_t workspace_bytes, void* stream) {
    DYN_REQUIRE(a && da && dz, DYN_E_ARG, "dyn_prompt_relu_bwd: null pointer");
    if (int rc = check_sizes("dyn_prompt_relu_bwd", B, T, I)) return rc;
    DYN_REQUIRE(aligned16(a) && aligned16(da) && aligned16(dz), DYN_E_ARG, "dyn_prompt_relu_bwd: operands must be 16-byte aligned");
    DYN_REQUIRE((const void*)dz != (const void*)a, DYN_E_ARG, "dyn_prompt_relu_bwd: dz may alias da, not a");
    const bool sums = db1 || dw1p;
    int64_t per;
    const int64_t tiles = row_tiles(T, &per), I4 = I / 4;
    float* part = nullptr;
    if (sums) {
        DYN_REQUIRE(prompt_ids && workspace, DYN_E_ARG, "dyn_prompt_relu_bwd: the sums need the prompt ids and a workspace");
        DYN_REQUIRE(Np >= 1 && Np <= (1 << 20), DYN_E_ARG, "dyn_prompt_relu_bwd: num_prompts=%lld out of range", (long long)Np);
        DYN_REQUIRE(((uintptr_t)prompt_ids & 3) == 0 && aligned16(workspace) && (!db1 || aligned16(db1)) && (!dw1p || aligned16(dw1p)), DYN_E_ARG,
                    "dyn_prompt_relu_bwd: workspace, db1 and dw1p must be 16-byte aligned, the ids 4-byte aligned");
        const int64_t need = dyn_prompt_relu_bwd_workspace_bytes(B, T, I);
        DYN_REQUIRE(workspace_bytes >= need, DYN_E_WORKSPACE, "dyn_prompt_relu_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)need);
        part = (float*)workspace;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(prompt_relu_bwd_kernel, dim3((unsigned)tiles, (unsigned)B, (unsigned)dyn::cdiv(I4, TPB)), dim3(TPB), 0, st, a, da, dz, part, T,
                       per, (int)I4);
    if (int rc = dyn::check_launch("dyn_prompt_relu_bwd")) return rc;
    if (!sums) return DYN_OK;
    float* s = part + B * tiles * I;
    hipLaunchKernelGGL(prompt_rows_kernel, dim3(grid_for(B * I)), dim3(TPB), 0, st, part, s, B, tiles, (int)I);
    if (int rc = dyn::check_launch("dyn_prompt_relu_bwd")) return rc;
    hipLaunchKernelGGL(prompt_finalise_kernel, dim3(grid_for(I * Np)), dim3(TPB), 0, st, s, prompt_ids, db1, dw1p, beta, B, (int)I, (int)Np);
    return dyn::check_launch("dyn_prompt_relu_bwd");
}
