// Kaldi-style filter-bank front end of Wav2Vec2-BERT on the device: what transformers' SeamlessM4TFeatureExtractor computes in numpy, one
// Python iteration per frame (feature_extraction_seamless_m4t.py: _extract_fbank_features -> audio_utils.spectrogram, then the per-bin
// normalisation and the stacking of two frames in __call__).
// Everything before the power spectrum is linear in the 400-sample frame (x * 2^15, the frame's mean removed, pre-emphasis 0.97, povey
// window, 512-point DFT), so frontend.KaldiFbank folds it in float64 into the [400, 2 * 260] basis of the strided-row GEMM LogMel already
// uses (frame f = samples 160 f .. 160 f + 399, lda = 160); dyn_stft_power and the mel GEMM follow (logmel.hip).  This file holds the rest:
//   dyn_fbank_finish   mel [B, F, M] energies -> out [B, F / 2, 2 M], every sample on its own:
//       x = log(max(mel, mel_floor));  per bin m: mean and UNBIASED variance of x over the first `valid` frames (device scalar; null: all F);
//       out[t, k M + m] = (x[2 t + k, m] - mean_m) / sqrt(var_m + eps) for t < valid / 2 (an odd last frame is dropped AFTER it has
//       taken part in the statistics, as the extractor does), rows t >= valid / 2 of a zero-padded length bucket are WRITTEN as zeros.
//     One workgroup per bin and sample: three passes over its column (sum -> mean, centred squares -> variance, normalise), each a
//     fixed-order block reduction: no atomics, bit-reproducible, no cancellation for a bin far from zero (log energies sit around
//     10 - 30).  Chosen for simplicity, not for bandwidth: a column's elements are M floats apart, so the loads are uncoalesced, every
//     128-byte line is fetched by the 32 workgroups whose bins share it (L2 absorbs that: [F, M] is 320 KB for 10 s of audio), and the
//     log is taken three times.  The whole front end is 46 us for 10 s; a tile of bins per workgroup would coalesce the reads.
#include "common.h"

namespace {

constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void fbank_finish_kernel(const float* __restrict__ mel, float* __restrict__ out, int64_t F, int M,
                                                            float mel_floor, float eps, const int32_t* __restrict__ valid) {
    __shared__ float red[16];
    const int m = blockIdx.x;
    mel += (int64_t)blockIdx.y * F * M;
    out += (int64_t)blockIdx.y * (F / 2) * 2 * M;
    const int64_t Fv = dyn::valid_rows(valid, F);
    const int64_t Tv = Fv / 2, Tb = F / 2;
    float s = 0.f;
    for (int64_t f = threadIdx.x; f < Fv; f += TPB) s += logf(fmaxf(mel[f * M + m], mel_floor));
    const float mean = dyn::block_sum(s, red) / (float)(Fv > 0 ? Fv : 1);
    float q = 0.f;
    for (int64_t f = threadIdx.x; f < Fv; f += TPB) {
        const float d = logf(fmaxf(mel[f * M + m], mel_floor)) - mean;
        q += d * d;
    }
    const float var = dyn::block_sum(q, red) / (float)(Fv > 1 ? Fv - 1 : 1);
    const float inv = 1.f / sqrtf(var + eps);
    for (int64_t f = threadIdx.x; f < 2 * Tb; f += TPB) {
        const float v = f < 2 * Tv ? (logf(fmaxf(mel[f * M + m], mel_floor)) - mean) * inv : 0.f;
        out[(f >> 1) * 2 * M + (f & 1) * M + m] = v;
    }
}

}  // namespace

extern "C" int dyn_fbank_finish(const float* mel, float* out, int64_t B, int64_t F, int64_t M, float mel_floor, float eps, const int32_t* valid_frames,
                                void* stream) {
    DYN_REQUIRE(mel && out, DYN_E_ARG, "dyn_fbank_finish: null pointer");
    DYN_REQUIRE(B >= 0 && B < 65536 && F >= 2 && F < (1ll << 31) && M >= 1 && M <= 4096, DYN_E_ARG,
                "dyn_fbank_finish: B=%lld F=%lld M=%lld (at least two frames: the unbiased variance)", (long long)B, (long long)F, (long long)M);
    if (B == 0) return DYN_OK;
    DYN_REQUIRE(mel_floor > 0.f && eps >= 0.f, DYN_E_ARG, "dyn_fbank_finish: mel_floor must be positive, eps non-negative");
    hipLaunchKernelGGL(fbank_finish_kernel, dim3((unsigned)M, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, mel, out, F, (int)M, mel_floor, eps,
                       valid_frames);
    return dyn::check_launch("dyn_fbank_finish");
}
