// Exact (erf) GELU and its derivative (HF `hidden_act: gelu`): one definition for dyn_gelu_* (wav2vec2.hip) and the fused
// bias + LayerNorm + GELU of the layer-norm feature extractor (bias_ln_gelu.hip), so both give the same bits.
#pragma once
#include "common.h"

namespace dyn {

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(float x) {
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return cdf + x * pdf;
}

}  // namespace dyn
