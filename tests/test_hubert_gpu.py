"""HubertForCTC (hubert_model.py: Wav2Vec2ForCTC under the `hubert.` prefix, with the optional feature-projection LayerNorm) against
transformers' HubertForCTC on the CPU with the same state dict — logits, every parameter gradient, both layouts, `feat_proj_layer_norm`
off, the dynamic-eval loops, bucketed hipGraph replay and the harness — at the bars tests/test_wavlm_gpu.py and
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

PF = "hubert."
POST_GROUP = dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False)      # hubert-base
STABLE_LAYER = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)      # hubert-large-ls960-ft
TOY = dict(C.TOY, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
PROJ_LN = PF + "feature_projection.layer_norm.weight"
POS_V = PF + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"


def _pair(cuda, seed=0, flags=POST_GROUP, **over):
    from transformers import HubertConfig, HubertForCTC as HF
    from dynamic_asr_eval_amd.hubert_model import HubertForCTC
    torch.manual_seed(seed)
    cfg = HubertConfig(**dict(TOY, **over), **flags)
    ref = HF(cfg).eval()
    C.randomise_1d(ref)
    hip = HubertForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict(), strict=False)
    return ref, hip


@pytest.mark.parametrize("flags,proj_ln,L", [(POST_GROUP, True, 6000), (STABLE_LAYER, True, 6000), (POST_GROUP, False, 6000),
                                             (STABLE_LAYER, False, 30000), (POST_GROUP, True, 30000)],
                         ids=["postln-group", "stable-layer", "postln-group-no-proj-ln", "stable-layer-no-proj-ln-93-frames",
                              "postln-group-93-frames"])
def test_forward_backward_matches_transformers(cuda, flags, proj_ln, L):
    ref, hip = _pair(cuda, flags=flags, feat_proj_layer_norm=proj_ln)
    c = hip.cfg
    assert (c["feat_extract_norm"], c["conv_bias"], c["do_stable_layer_norm"], c["feat_proj_layer_norm"]) == \
        (flags["feat_extract_norm"], flags["conv_bias"], flags["do_stable_layer_norm"], proj_ln)
    assert (PROJ_LN in hip.P) == proj_ln
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, L, generator=g)
    assert hip.conv_lengths(L)[-1] == (18 if L == 6000 else 93)
    grads, named = C.forward_and_every_gradient(cuda, ref, hip, x, g, PF)
    assert grads[POS_V].abs().max().item() > 0.0
    C.state_dict_round_trip(ref, hip)


def test_backward_is_bit_reproducible(cuda):
    C.backward_is_bit_reproducible(cuda, _pair(cuda, seed=1, feat_proj_layer_norm=False)[1])


def test_active_subset_backward(cuda):
    C.active_subset_backward(cuda, _pair(cuda, seed=3, feat_proj_layer_norm=False)[1])


def test_frozen_prefixes(cuda):
    C.frozen_prefixes(cuda, _pair(cuda, seed=4)[1], PF, PF + "encoder.layers.0.attention.out_proj", PF + "encoder.layers.1.attention.out_proj.weight")


@pytest.mark.parametrize("flags,proj_ln", [(POST_GROUP, False), (STABLE_LAYER, True)], ids=["postln-group-no-proj-ln", "stable-layer"])
def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda, flags, proj_ln):
    ref, hip = _pair(cuda, seed=11, flags=flags, feat_proj_layer_norm=proj_ln)
    C.bucketed_graph_replay(cuda, hip, PF, POS_V)


@pytest.mark.parametrize("seed", [1, 3])
def test_dynamic_eval_su_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed, flags=STABLE_LAYER)
    C.dynamic_eval_su_matches_oracle(cuda, ref, hip)


@pytest.mark.parametrize("seed", [4])
def test_chunked_dynamic_eval_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed, flags=STABLE_LAYER)
    C.chunked_dynamic_eval_matches_oracle(cuda, ref, hip)


def test_run_wav2vec2_harness_with_a_hubert_directory(cuda, tmp_path, capsys):
    from transformers import HubertConfig, HubertForCTC as HF
    torch.manual_seed(0)
    cfg = HubertConfig(**TOY, **POST_GROUP)
    C.harness_with_a_directory(tmp_path, capsys, cfg, HF(cfg), "hubert", dict(TOY, **POST_GROUP))
