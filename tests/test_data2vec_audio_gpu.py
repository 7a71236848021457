"""Data2VecAudioForCTC (data2vec_audio_model.py: Wav2Vec2ForCTC's layer-norm extractor, projection and post-LN encoder + the positional conv
stack on csrc/posconv_ln_gelu.hip) against transformers' Data2VecAudioForCTC on the CPU with the same state dict — logits, every parameter
gradient, the flag combinations, the dynamic-eval loops, bucketed hipGraph replay and the harness — at the bars tests/test_wavlm_gpu.py and
tests/test_wav2vec2_conformer_gpu.py hold their models to.  The shared checks live in tests/ctc_family_cases.py."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_family_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

PF = "data2vec_audio."
TOY = dict(C.TOY, num_conv_pos_embedding_groups=4)
POS_W = PF + "encoder.pos_conv_embed.layers.{}.conv.weight"
POS_B = PF + "encoder.pos_conv_embed.layers.{}.conv.bias"


def _pair(cuda, seed=0, arch=TOY, **over):
    from transformers import Data2VecAudioConfig, Data2VecAudioForCTC as HF
    from dynamic_asr_eval_amd.data2vec_audio_model import Data2VecAudioForCTC
    torch.manual_seed(seed)
    cfg = Data2VecAudioConfig(**dict(arch, **over))
    ref = HF(cfg).eval()
    C.randomise_1d(ref)
    hip = Data2VecAudioForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict(), strict=False)
    return ref, hip


@pytest.mark.parametrize("conv_bias,groups,layers,taps,L", [
    (False, 4, 5, 19, 6000), (True, 16, 5, 19, 6000), (False, 4, 1, 19, 6000), (True, 4, 5, 4, 6000), (False, 16, 5, 19, 30000),
    (True, 4, 1, 4, 30000)],
    ids=["nobias-g4-5x19", "bias-g16-5x19", "nobias-g4-1x19", "bias-g4-5x4", "nobias-g16-5x19-93-frames", "bias-g4-1x4-93-frames"])
def test_forward_backward_matches_transformers(cuda, conv_bias, groups, layers, taps, L):
    """18 frames are fewer than the 19 taps: every frame has the zero padding inside its window on both sides; 93 frames have interior
    frames too.  4 taps: an even kernel, whose conv gives T + 1 frames of which transformers drops the last.  One layer: the kernel's
    token-major output alone; five: the packed output feeds the next GEMM four times."""
    ref, hip = _pair(cuda, conv_bias=conv_bias, num_conv_pos_embedding_groups=groups, num_conv_pos_embeddings=layers, conv_pos_kernel_size=taps)
    c = hip.cfg
    assert (c["feat_extract_norm"], c["conv_bias"], c["do_stable_layer_norm"]) == ("layer", conv_bias, False)
    assert (c["num_conv_pos_embedding_groups"], c["num_conv_pos_embeddings"], c["conv_pos_kernel_size"]) == (groups, layers, taps)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, L, generator=g)
    assert hip.conv_lengths(L)[-1] == (18 if L == 6000 else 93)
    grads, named = C.forward_and_every_gradient(cuda, ref, hip, x, g, PF)
    for i in range(layers):
        assert grads[POS_W.format(i)].abs().max().item() > 0.0 and grads[POS_B.format(i)].abs().max().item() > 0.0, i
    C.state_dict_round_trip(ref, hip)


def test_wide_shape_forward_and_every_gradient(cuda):
    """The base width (768 hidden, 12 x 64 heads, 16 groups of 48 channels: a segment that is no power of two) with one encoder layer."""
    arch = dict(TOY, hidden_size=768, num_attention_heads=12, num_hidden_layers=1, num_conv_pos_embedding_groups=16)
    ref, hip = _pair(cuda, arch=arch)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 6000, generator=g)
    C.forward_and_every_gradient(cuda, ref, hip, x, g, PF)


def test_backward_is_bit_reproducible(cuda):
    C.backward_is_bit_reproducible(cuda, _pair(cuda, seed=1)[1])


def test_active_subset_backward(cuda):
    C.active_subset_backward(cuda, _pair(cuda, seed=3)[1])


def test_frozen_prefixes(cuda):
    C.frozen_prefixes(cuda, _pair(cuda, seed=4)[1], PF, PF + "encoder.pos_conv_embed.layers.2", POS_W.format(3))


def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda):
    """With 10 - 18 valid frames in buckets of 16 / 24 every layer of the stack has valid frames whose 19-tap window reaches past the
    utterance, and the rows just past it are not zero after a conv: the run differs from the unpadded one unless every layer's output is
    masked there, which is the fused kernel's `valid` argument."""
    ref, hip = _pair(cuda, seed=11)
    C.bucketed_graph_replay(cuda, hip, PF, POS_W.format(0))


@pytest.mark.parametrize("seed", [0, 1])
def test_dynamic_eval_su_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed)
    C.dynamic_eval_su_matches_oracle(cuda, ref, hip)


@pytest.mark.parametrize("seed", [2, 4])
def test_chunked_dynamic_eval_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed)
    C.chunked_dynamic_eval_matches_oracle(cuda, ref, hip)


def test_run_wav2vec2_harness_with_a_data2vec_audio_directory(cuda, tmp_path, capsys):
    from transformers import Data2VecAudioConfig, Data2VecAudioForCTC as HF
    torch.manual_seed(0)
    cfg = Data2VecAudioConfig(**TOY)
    C.harness_with_a_directory(tmp_path, capsys, cfg, HF(cfg), "data2vec-audio",
                               dict(TOY, num_conv_pos_embeddings=16, feat_extract_norm="layer", conv_bias=True))
