// Cache-aware chunk-by-chunk streaming of NemotronAsrStreamingForRNNT's encoder (transformers modeling_nemotron_asr_streaming.py with
// `use_cache=True, past_key_values=..., padding_cache=...`): the kernels of ONE step, cs = lookahead + 1 encoder frames of B streams.
// A step is bound by launches, not arithmetic (every matrix has B * cs rows), so each kernel here fuses what the offline path spreads
// over several, keeps its state on the device and reads WHERE the stream stands from a per-session int32 counter in device memory
// (`counter[0]` = chunks consumed so far): the launch arguments are the same on every step and a step can be captured and replayed.
//   dyn_stream_attn          the attention core of one layer and chunk in one launch: scores against the cached and the new keys, the
//                            position term, softmax, context, and the chunk's k / v stored into the cache.  The cache is a RING of
//                            lc + 1 chunk slots [B, lc + 1, cs, H]: the chunk of step s lives in slot s % (lc + 1), the n_valid =
//                            min(s, lc) * cs visible cached frames are the slots of steps s - min(s, lc) .. s - 1, and the slot written
//                            by a launch is never one it reads (that is what the + 1 buys: no block can overwrite a key another block
//                            of the same launch still has to load).  Nothing is ever moved.
//   dyn_stream_convmod_k9    dyn_convmod_causal_k9_fwd with the 8 GLU frames left of the chunk taken from a carried state.
//   dyn_stream_conv2d_first / dyn_stream_dwconv2d_s2_act   the causal subsampling stages with a one-row carry in time, no right padding.
//   dyn_stream_advance       counter[0] += 1, the last launch of a step.
// The conv state and the subsampling carries are DOUBLE BUFFERED on the counter's parity ([2, ...]: a step reads half `counter & 1` and
// writes the other), so no launch reads state that the same launch has already overwritten, whatever cs is and however many workgroups
// share a stream.  No float atomics anywhere; every sum runs in a fixed order.
#include "common.h"
#include "layernorm_row.h"

namespace {

using dyn::ld4;
using dyn::st4;

constexpr int64_t LDS_LIMIT = 160 * 1024;         // bytes of LDS of a gfx950 CU: one workgroup may ask for all of it
constexpr int64_t LDS_STATIC = 64 * 1024;         // above this a kernel's dynamic LDS has to be allowed first
constexpr int ATT_PAD = 4;                        // floats added to every LDS row of D: lanes that walk rows do not share a bank

__device__ __forceinline__ int stream_step(const int32_t* counter) {
    const int s = *counter;
    return s < 0 ? 0 : s;
}

__global__ void stream_advance_kernel(int32_t* counter) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counter[0] = stream_step(counter) + 1;
}

// ---- attention ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (head, stream).  LDS: K (then V) [NK][D + 4], the position rows [W][D + 4], q + u and q + v [cs][D + 4], the scores
// [cs][NK]; NK = (lc + 1) cs keys at most, W = NK + cs - 1 distances.  Key j < n_valid is cached frame j (oldest first), key n_valid + i
// is frame i of the chunk; query i and key j are i - j + n_valid frames apart, row dlo - (i - j + n_valid) of `pos` (dlo = NK - 1).
__global__ __launch_bounds__(256) void stream_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias_u,
                                                          const float* __restrict__ bias_v, const float* __restrict__ pos,
                                                          float* __restrict__ k_cache, float* __restrict__ v_cache,
                                                          const int32_t* __restrict__ counter, float* __restrict__ out, int cs, int lc, int nh,
                                                          int D, float scale) {
    extern __shared__ __align__(16) float att_lds[];
    const int h = blockIdx.x, tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int H = nh * D, DP = D + ATT_PAD, D4 = D / 4, S = lc + 1, NK = S * cs, W = NK + cs - 1, dlo = NK - 1;
    const int step = stream_step(counter);
    const int nc = step < lc ? step : lc, nv = nc * cs, nk = nv + cs;
    float* Kb = att_lds;
    float* Pb = Kb + (int64_t)NK * DP;
    float* qu = Pb + (int64_t)W * DP;
    float* qv = qu + (int64_t)cs * DP;
    float* sc = qv + (int64_t)cs * DP;
    const int64_t hcol = (int64_t)h * D;
    const int64_t slot_new = ((b * S + step % S) * cs) * H + hcol;         // the chunk's rows in either cache

    for (int e = tid; e < cs * D4; e += 256) {                             // q + u, q + v, the new keys; k and v go into the ring
        const int i = e / D4, d4 = e % D4;
        const float* row = qkv + (b * cs + i) * 3 * H + hcol;
        const float4 q = ld4(row, d4), k = ld4(row + H, d4), v = ld4(row + 2 * H, d4);
        const float4 u4 = ld4(bias_u + hcol, d4), v4 = ld4(bias_v + hcol, d4);
        st4(qu + i * DP, make_float4(q.x + u4.x, q.y + u4.y, q.z + u4.z, q.w + u4.w), d4);
        st4(qv + i * DP, make_float4(q.x + v4.x, q.y + v4.y, q.z + v4.z, q.w + v4.w), d4);
        st4(Kb + (nv + i) * DP, k, d4);
        st4(k_cache + slot_new + (int64_t)i * H, k, d4);
        st4(v_cache + slot_new + (int64_t)i * H, v, d4);
    }
    for (int e = tid; e < nv * D4; e += 256) {                             // the cached keys, oldest chunk first
        const int j = e / D4, d4 = e % D4;
        const int slot = (step - nc + j / cs) % S;
        st4(Kb + j * DP, ld4(k_cache + ((b * S + slot) * cs + j % cs) * H + hcol, d4), d4);
    }
    const int c0 = (lc - nc) * cs;                                         // the first distance row any pair of this step touches
    for (int e = tid + c0 * D4; e < W * D4; e += 256) {
        const int c = e / D4, d4 = e % D4;
        st4(Pb + c * DP, ld4(pos + (int64_t)c * H + hcol, d4), d4);
    }
    __syncthreads();
    for (int p = tid; p < cs * nk; p += 256) {                             // ((q + u) K^T + (q + v) P[distance]^T) * scale
        const int i = p / nk, j = p % nk;
        const float* a = qu + i * DP;
        const float* bq = qv + i * DP;
        const float* kr = Kb + j * DP;
        const float* pr = Pb + (dlo - i + j - nv) * DP;
        float ac = 0.f, bd = 0.f;
        for (int d4 = 0; d4 < D4; ++d4) {
            ac += dyn::dot4(ld4(a, d4), ld4(kr, d4));
            bd += dyn::dot4(ld4(bq, d4), ld4(pr, d4));
        }
        sc[i * NK + j] = (ac + bd) * scale;
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    for (int i = wv; i < cs; i += 4) {                                     // softmax over the nk keys, one wave per query
        float* r = sc + i * NK;
        float m = -INFINITY;
        for (int j = lane; j < nk; j += 64) m = fmaxf(m, r[j]);
        m = dyn::wave_max(m);
        float s = 0.f;
        for (int j = lane; j < nk; j += 64) {
            const float e = expf(r[j] - m);
            r[j] = e;
            s += e;
        }
        const float inv = 1.f / dyn::wave_sum(s);
        for (int j = lane; j < nk; j += 64) r[j] *= inv;
    }
    for (int e = tid; e < cs * D4; e += 256) {                             // V takes K's place: every score has been formed
        const int i = e / D4, d4 = e % D4;
        st4(Kb + (nv + i) * DP, ld4(qkv + (b * cs + i) * 3 * H + 2 * H + hcol, d4), d4);
    }
    for (int e = tid; e < nv * D4; e += 256) {
        const int j = e / D4, d4 = e % D4;
        const int slot = (step - nc + j / cs) % S;
        st4(Kb + j * DP, ld4(v_cache + ((b * S + slot) * cs + j % cs) * H + hcol, d4), d4);
    }
    __syncthreads();
    for (int e = tid; e < cs * D; e += 256) {                              // context: keys in index order
        const int i = e / D, d = e % D;
        const float* r = sc + i * NK;
        float acc = 0.f;
        for (int j = 0; j < nk; ++j) acc += r[j] * Kb[j * DP + d];
        out[(b * cs + i) * H + hcol + d] = acc;
    }
}

int64_t attn_lds_bytes(int64_t cs, int64_t lc, int64_t D) {
    const int64_t NK = (lc + 1) * cs, W = NK + cs - 1, DP = D + ATT_PAD;
    return ((NK + W + 2 * cs) * DP + cs * NK) * (int64_t)sizeof(float);
}

// ---- conv module --------------------------------------------------------------------------------------------------------------------
// convmod_causal.hip's forward at KW = 9, TT = 8 with the frames left of the chunk read from state[counter & 1] [B, 8, C] (GLU values,
// row r = frame r - 8) and the last 8 GLU frames of state + chunk written to the other half: frame t >= 0 by the workgroup whose tile
// holds it, the carried frames t < 0 (only a chunk shorter than 8 keeps any) by the first.
template <int NV>
__global__ __launch_bounds__(NV * 256) void stream_convmod_k9_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                                     const float* __restrict__ cbias, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ state,
                                                                     const int32_t* __restrict__ counter, float* __restrict__ s, int64_t T,
                                                                     float eps) {
    constexpr int KW = 9, TT = 8, C = NV * 256, NG = TT + KW - 1, NW = C / 64;
    __shared__ float ys[TT * C];
    const int c = threadIdx.x;
    const int64_t b = blockIdx.y, B = gridDim.y, t0 = (int64_t)blockIdx.x * TT;
    const int step = stream_step(counter);
    const float* sin = state + (((int64_t)(step & 1) * B + b) * (KW - 1)) * C + c;
    float* sout = state + (((int64_t)((step + 1) & 1) * B + b) * (KW - 1)) * C + c;
    {
        float wk[KW], g[NG];
#pragma unroll
        for (int j = 0; j < KW; ++j) wk[j] = w[(int64_t)c * KW + j];
        const float cb = cbias ? cbias[c] : 0.f;
        const float* ub = u + b * T * 2 * C + c;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int64_t t = t0 - (KW - 1) + i;
            g[i] = t < 0 ? sin[(t + KW - 1) * C] : (t < T ? ub[t * 2 * C] * dyn::sigmoidf_(ub[t * 2 * C + C]) : 0.f);
            const int64_t r = t - (T - (KW - 1));                         // the new state's row of frame t
            if (t < T && r >= 0 && (i >= KW - 1 || blockIdx.x == 0)) sout[r * C] = g[i];
        }
#pragma unroll
        for (int k = 0; k < TT; ++k) {
            float acc = cb;
#pragma unroll
            for (int j = 0; j < KW; ++j) acc += wk[j] * g[k + j];
            ys[k * C + c] = acc;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float4 gm[NV], bt[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        gm[j] = ld4(gamma, lane + 64 * j);
        bt[j] = ld4(beta, lane + 64 * j);
    }
    for (int k = wv; k < TT; k += NW) {
        const int64_t t = t0 + k;
        if (t >= T) break;                              // uniform over the wave
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = ld4(ys + k * C, lane + 64 * j);
        float mean, rstd;
        dyn::row_mean_rstd(v, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 n = dyn::affine4(v[j], mean, rstd, gm[j], bt[j]);
            st4(s + (b * T + t) * C, make_float4(dyn::silu_f(n.x), dyn::silu_f(n.y), dyn::silu_f(n.z), dyn::silu_f(n.w)), lane + 64 * j);
        }
    }
}

// ---- subsampling --------------------------------------------------------------------------------------------------------------------
// A stage sees [left rows of context | the chunk's T rows], no padding on the right: output `to` reads the chunk rows 2 to + dt - left,
// dt in 0 .. 2.  left = 1: row -1 is the carry (the last input row of the previous chunk); first chunk, left = 2: rows -2, -1 are zeros.
// The frequency axis keeps the offline (2, 1) padding.  The carry holds the stage's INPUT row as it arrived: the stem's features, the
// depthwise stage's row BEFORE the ReLU, which is applied as the row is loaded, like every row of the chunk.
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

__global__ __launch_bounds__(256) void stream_conv2d_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ carry,
                                                                  const int32_t* __restrict__ counter, float* __restrict__ z, int64_t total,
                                                                  int64_t B, int64_t T, int F, int64_t To, int Fo, int C4, int left) {
    const int step = stream_step(counter);
    const float* cin = carry + (int64_t)(step & 1) * B * F;
    float* cout = carry + (int64_t)((step + 1) & 1) * B * F;
    const int64_t stride = (int64_t)gridDim.x * 256, first_e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t e = first_e; e < total; e += stride) {
        const int c4 = (int)(e % C4);
        const int fo = (int)((e / C4) % Fo);
        const int64_t to = (e / C4 / Fo) % To, b = e / C4 / Fo / To;
        const float* wc = w + (int64_t)c4 * 36;
        float4 acc = ld4(bias, c4);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int64_t t = 2 * to + dt - left;
            if (t >= T || t < -1 || (t < 0 && left == 2)) continue;
            const float* row = t < 0 ? cin + b * F : x + (b * T + t) * F;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int f = 2 * fo + df - 2;
                const float v = (f >= 0 && f < F) ? row[f] : 0.f;
                const int j = dt * 3 + df;
                acc.x += wc[j] * v; acc.y += wc[9 + j] * v; acc.z += wc[18 + j] * v; acc.w += wc[27 + j] * v;
            }
        }
        st4(z, acc, e);
    }
    for (int64_t e = first_e; e < B * F; e += stride) cout[e] = x[((e / F) * T + T - 1) * F + e % F];
}

__global__ __launch_bounds__(256) void stream_dwconv2d_s2_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ carry,
                                                                 const int32_t* __restrict__ counter, float* __restrict__ u, int64_t total,
                                                                 int64_t B, int64_t T, int F, int64_t To, int Fo, int C4, int left) {
    const int step = stream_step(counter);
    const int64_t FC4 = (int64_t)F * C4;
    const float* cin = carry + (int64_t)(step & 1) * B * FC4 * 4;
    float* cout = carry + (int64_t)((step + 1) & 1) * B * FC4 * 4;
    const int64_t stride = (int64_t)gridDim.x * 256, first_e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t e = first_e; e < total; e += stride) {
        const int c4 = (int)(e % C4);
        const int fo = (int)((e / C4) % Fo);
        const int64_t to = (e / C4 / Fo) % To, b = e / C4 / Fo / To;
        const float* wc = w + (int64_t)c4 * 36;
        float4 acc = ld4(bias, c4);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int64_t t = 2 * to + dt - left;
            if (t >= T || t < -1 || (t < 0 && left == 2)) continue;
            const float* row = t < 0 ? cin + b * FC4 * 4 : z + (b * T + t) * FC4 * 4;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int f = 2 * fo + df - 2;
                if (f < 0 || f >= F) continue;
                const float4 v = relu4(ld4(row, (int64_t)f * C4 + c4));
                const int j = dt * 3 + df;
                acc.x += wc[j] * v.x; acc.y += wc[9 + j] * v.y; acc.z += wc[18 + j] * v.z; acc.w += wc[27 + j] * v.w;
            }
        }
        st4(u, acc, e);
    }
    for (int64_t e = first_e; e < B * FC4; e += stride) st4(cout, ld4(z, ((e / FC4) * T + T - 1) * FC4 + e % FC4), e);
}

int check_stage(const char* who, int64_t B, int64_t T, int64_t F, int64_t C, int32_t first) {
    DYN_REQUIRE(B >= 1 && B < 65536 && T >= 1 && T < (1 << 24) && F >= 1 && F < (1 << 20) && C >= 4 && C <= 65536, DYN_E_ARG,
                "%s: bad sizes B=%lld T=%lld F=%lld C=%lld", who, (long long)B, (long long)T, (long long)F, (long long)C);
    DYN_REQUIRE(C % 4 == 0, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (a multiple of 4)", who, (long long)C);
    DYN_REQUIRE(first == 0 || first == 1, DYN_E_ARG, "%s: first=%d (0 a later chunk, 1 the first)", who, (int)first);
    DYN_REQUIRE(T + (first ? 2 : 1) >= 3, DYN_E_ARG, "%s: a later chunk needs T >= 2 rows (%lld)", who, (long long)T);
    return DYN_OK;
}

inline unsigned flat_grid(int64_t total) {
    const int64_t g = dyn::cdiv(total, 256);
    return (unsigned)(g < 65536 ? g : 65536);
}

}  // namespace

extern "C" int dyn_stream_advance(int32_t* counter, void* stream) {
    DYN_REQUIRE(counter, DYN_E_ARG, "dyn_stream_advance: null pointer");
    hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter);
    return dyn::check_launch("dyn_stream_advance");
}

extern "C" int64_t dyn_stream_attn_lds_bytes(int64_t cs, int64_t lc, int64_t D) {
    if (cs < 1 || lc < 0 || D < 4 || cs > 4096 || lc > 4096 || D > 4096) return -1;
    return attn_lds_bytes(cs, lc, D);
}

extern "C" int dyn_stream_attn(const float* qkv, const float* bias_u, const float* bias_v, const float* pos, float* k_cache, float* v_cache,
                               const int32_t* counter, float* out, int64_t B, int64_t cs, int64_t lc, int64_t nh, int64_t D, float scale,
                               void* stream) {
    const char* who = "dyn_stream_attn";
    DYN_REQUIRE(qkv && bias_u && bias_v && pos && k_cache && v_cache && counter && out, DYN_E_ARG, "%s: null pointer", who);
    DYN_REQUIRE(B >= 1 && B < 65536 && cs >= 1 && cs <= 4096 && lc >= 0 && lc <= 4096 && nh >= 1 && nh < 65536 && D >= 4 && D <= 4096, DYN_E_ARG,
                "%s: bad sizes B=%lld cs=%lld lc=%lld heads=%lld D=%lld", who, (long long)B, (long long)cs, (long long)lc, (long long)nh,
                (long long)D);
    DYN_REQUIRE(D % 4 == 0, DYN_E_UNSUPPORTED, "%s: head width %lld is not built (a multiple of 4)", who, (long long)D);
    const int64_t lds = attn_lds_bytes(cs, lc, D);
    DYN_REQUIRE(lds <= LDS_LIMIT, DYN_E_UNSUPPORTED, "%s: cs=%lld, lc=%lld, D=%lld need %lld B of LDS per workgroup, more than the %lld B of a CU",
                who, (long long)cs, (long long)lc, (long long)D, (long long)lds, (long long)LDS_LIMIT);
    DYN_REQUIRE(B * (lc + 1) * cs * nh * D < (1ll << 40), DYN_E_ARG, "%s: the cache is too large for one launch", who);
    DYN_REQUIRE(dyn::aligned16(qkv) && dyn::aligned16(bias_u) && dyn::aligned16(bias_v) && dyn::aligned16(pos) && dyn::aligned16(k_cache) &&
                    dyn::aligned16(v_cache) && dyn::aligned16(out),
                DYN_E_ARG, "%s: operands must be 16-byte aligned", who);
    if (lds > LDS_STATIC) {                            // once per device, so a captured step issues nothing but its launches
        static bool allowed[64] = {};
        int dev = 0;
        DYN_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, DYN_E_LAUNCH, "%s: no current device", who);
        if (!allowed[dev]) {
            hipError_t e = hipFuncSetAttribute((const void*)stream_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
            DYN_REQUIRE(e == hipSuccess, DYN_E_LAUNCH, "%s: %lld B of LDS refused: %s", who, (long long)lds, hipGetErrorString(e));
            allowed[dev] = true;
        }
    }
    hipLaunchKernelGGL(stream_attn_kernel, dim3((unsigned)nh, (unsigned)B), dim3(256), (size_t)lds, (hipStream_t)stream, qkv, bias_u, bias_v, pos,
                       k_cache, v_cache, counter, out, (int)cs, (int)lc, (int)nh, (int)D, scale);
    return dyn::check_launch(who);
}

extern "C" int dyn_stream_convmod_k9(const float* u, const float* w, const float* cbias, const float* gamma, const float* beta, float* state,
                                     const int32_t* counter, float* s, int64_t B, int64_t T, int64_t C, int64_t KW, float eps, void* stream) {
    const char* who = "dyn_stream_convmod_k9";
    DYN_REQUIRE(u && w && gamma && beta && state && counter && s, DYN_E_ARG, "%s: null pointer", who);
    DYN_REQUIRE(B >= 1 && B < 65536 && T >= 1 && B * T < (1ll << 31), DYN_E_ARG, "%s: bad sizes B=%lld T=%lld", who, (long long)B, (long long)T);
    DYN_REQUIRE(C == 256 || C == 512 || C == 768 || C == 1024, DYN_E_UNSUPPORTED, "%s: C=%lld is not built (256, 512, 768, 1024)", who,
                (long long)C);
    DYN_REQUIRE(KW == 9, DYN_E_UNSUPPORTED, "%s: kernel width %lld is not built (9)", who, (long long)KW);
    DYN_REQUIRE(dyn::aligned16(u) && dyn::aligned16(gamma) && dyn::aligned16(beta) && dyn::aligned16(s), DYN_E_ARG,
                "%s: operands must be 16-byte aligned", who);
    const dim3 grid((unsigned)dyn::cdiv(T, 8), (unsigned)B);
    dyn::dispatch_nv<1, 2, 3, 4>(C, [&](auto NV) {
        constexpr int nv = decltype(NV)::value;
        hipLaunchKernelGGL((stream_convmod_k9_kernel<nv>), grid, dim3(nv * 256), 0, (hipStream_t)stream, u, w, cbias, gamma, beta, state, counter, s,
                           T, eps);
    });
    return dyn::check_launch(who);
}

extern "C" int dyn_stream_conv2d_first(const float* x, const float* w, const float* bias, float* carry, const int32_t* counter, float* z,
                                       int64_t B, int64_t T, int64_t F, int64_t C, int32_t first, void* stream) {
    const char* who = "dyn_stream_conv2d_first";
    DYN_REQUIRE(x && w && bias && carry && counter && z, DYN_E_ARG, "%s: null pointer", who);
    if (int rc = check_stage(who, B, T, F, C, first)) return rc;
    DYN_REQUIRE(dyn::aligned16(bias) && dyn::aligned16(z), DYN_E_ARG, "%s: bias and z must be 16-byte aligned", who);
    const int left = first ? 2 : 1;
    const int64_t To = (T + left - 3) / 2 + 1, Fo = F / 2 + 1, total = B * To * Fo * (C / 4);
    hipLaunchKernelGGL(stream_conv2d_first_kernel, dim3(flat_grid(total > B * F ? total : B * F)), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                       carry, counter, z, total, B, T, (int)F, To, (int)Fo, (int)(C / 4), left);
    return dyn::check_launch(who);
}

extern "C" int dyn_stream_dwconv2d_s2_act(const float* z, const float* w, const float* bias, float* carry, const int32_t* counter, float* u,
                                          int64_t B, int64_t T, int64_t F, int64_t C, int32_t act, int32_t first, void* stream) {
    const char* who = "dyn_stream_dwconv2d_s2_act";
    DYN_REQUIRE(z && w && bias && carry && counter && u, DYN_E_ARG, "%s: null pointer", who);
    DYN_REQUIRE(act == 1, DYN_E_UNSUPPORTED, "%s: act=%d is not built (1 ReLU)", who, (int)act);
    if (int rc = check_stage(who, B, T, F, C, first)) return rc;
    DYN_REQUIRE(dyn::aligned16(z) && dyn::aligned16(bias) && dyn::aligned16(carry) && dyn::aligned16(u), DYN_E_ARG,
                "%s: z, bias, carry and u must be 16-byte aligned", who);
    const int left = first ? 2 : 1;
    const int64_t To = (T + left - 3) / 2 + 1, Fo = F / 2 + 1, total = B * To * Fo * (C / 4), rowv = B * F * (C / 4);
    hipLaunchKernelGGL(stream_dwconv2d_s2_kernel, dim3(flat_grid(total > rowv ? total : rowv)), dim3(256), 0, (hipStream_t)stream, z, w, bias, carry,
                       counter, u, total, B, T, (int)F, To, (int)Fo, (int)(C / 4), left);
    return dyn::check_launch(who);
}
