"""Data2Vec-Audio and HuBERT without a GPU: the parameter lists against transformers' `named_parameters()` for every flag combination the
GPU tests run, the configuration readers (Data2Vec-Audio's forced layer-norm extractor and post-LN encoder, HuBERT's `feat_proj_layer_norm`),
each refusal and its message, the new C-ABI entries' host-side argument checks, and the harness's model_type dispatch."""
import pytest
import torch

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7, vocab_size=32)
HF_SHAPE = {None: lambda s: s, "conv": lambda s: (s[0], s[2], s[1]), "g": lambda s: (1, 1, s[0])}
NEW = ("dyn_posconv_ln_gelu_fwd", "dyn_posconv_ln_gelu_bwd", "dyn_posconv_ln_gelu_bwd_workspace_bytes")


def _same_as_transformers(spec, ref, prefix):
    hf = {n: tuple(p.shape) for n, p in ref.named_parameters()}
    assert len(spec) == len({n for n, _, _ in spec})
    assert {n for n, _, _ in spec} == set(hf)
    for n, shape, kind in spec:
        assert HF_SHAPE[kind](tuple(shape)) == hf[n], (n, shape, kind, hf[n])
    assert all(n.startswith(prefix) or n.startswith("lm_head.") for n in hf)
    names = [n for n, _, _ in spec]                                           # the q | k | v slots stay side by side
    i = names.index(prefix + "encoder.layers.1.attention.q_proj.weight")
    assert names[i + 1].endswith("k_proj.weight") and names[i + 2].endswith("v_proj.weight")
    assert names[i + 3].endswith("q_proj.bias") and names[i + 5].endswith("v_proj.bias")


@pytest.mark.parametrize("taps", [19, 4])
@pytest.mark.parametrize("layers", [1, 5])
@pytest.mark.parametrize("groups", [4, 16])
@pytest.mark.parametrize("conv_bias", [False, True])
def test_data2vec_param_spec_is_transformers_named_parameters(conv_bias, groups, layers, taps):
    from transformers import Data2VecAudioConfig, Data2VecAudioForCTC as HF
    from dynamic_asr_eval_amd import data2vec_audio_model as M
    cfg = Data2VecAudioConfig(**TOY, conv_bias=conv_bias, num_conv_pos_embedding_groups=groups, num_conv_pos_embeddings=layers,
                              conv_pos_kernel_size=taps)
    spec = M.param_spec(M.make_config(cfg))
    _same_as_transformers(spec, HF(cfg), "data2vec_audio.")
    kinds = {n: (s, k) for n, s, k in spec}
    for i in range(layers):
        assert kinds[f"data2vec_audio.encoder.pos_conv_embed.layers.{i}.conv.weight"] == ((256, taps, 256 // groups), "conv")
        assert kinds[f"data2vec_audio.encoder.pos_conv_embed.layers.{i}.conv.bias"] == ((256,), None)
    assert not any("parametrizations" in n for n in kinds)                    # no weight norm
    assert ("data2vec_audio.feature_extractor.conv_layers.3.conv.bias" in kinds) == conv_bias
    assert "data2vec_audio.feature_extractor.conv_layers.3.layer_norm.weight" in kinds


@pytest.mark.parametrize("mask_time_prob", [0.05, 0.0])
def test_data2vec_wide_param_spec(mask_time_prob):
    from transformers import Data2VecAudioConfig, Data2VecAudioForCTC as HF
    from dynamic_asr_eval_amd import data2vec_audio_model as M
    cfg = Data2VecAudioConfig(**dict(TOY, hidden_size=768, num_attention_heads=12, num_hidden_layers=2, num_conv_pos_embedding_groups=16),
                              mask_time_prob=mask_time_prob)
    spec = M.param_spec(M.make_config(cfg))
    _same_as_transformers(spec, HF(cfg), "data2vec_audio.")
    assert ("data2vec_audio.masked_spec_embed" in {n for n, _, _ in spec}) == (mask_time_prob > 0.0)   # built only when a masking probability is set


@pytest.mark.parametrize("mask_time_prob", [0.05, 0.0])
@pytest.mark.parametrize("proj_ln", [True, False])
@pytest.mark.parametrize("flags", [dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False),
                                   dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)], ids=["group-postln", "layer-stable"])
def test_hubert_param_spec_is_transformers_named_parameters(flags, proj_ln, mask_time_prob):
    from transformers import HubertConfig, HubertForCTC as HF
    from dynamic_asr_eval_amd import hubert_model as M
    cfg = HubertConfig(**TOY, **flags, feat_proj_layer_norm=proj_ln, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
                       mask_time_prob=mask_time_prob)
    c = M.make_config(cfg)
    assert (c["feat_proj_layer_norm"], c["feat_extract_norm"], c["conv_bias"], c["do_stable_layer_norm"]) == \
        (proj_ln, flags["feat_extract_norm"], flags["conv_bias"], flags["do_stable_layer_norm"])
    spec = M.param_spec(c)
    _same_as_transformers(spec, HF(cfg), "hubert.")
    names = {n for n, _, _ in spec}
    assert ("hubert.feature_projection.layer_norm.weight" in names) == ("hubert.feature_projection.layer_norm.bias" in names) == proj_ln
    assert ("hubert.masked_spec_embed" in names) == (mask_time_prob > 0.0)    # transformers builds it only when a masking probability is set


def test_data2vec_make_config_forces_the_layout_and_refuses_what_is_not_built(tmp_path):
    from transformers import Data2VecAudioConfig
    from dynamic_asr_eval_amd import data2vec_audio_model as M, wav2vec2_model as W2, run_wav2vec2 as R
    from dynamic_asr_eval_amd.ops import DynError
    d, hf = M.make_config(), Data2VecAudioConfig()
    for k in ("conv_pos_kernel_size", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups", "hidden_size", "num_hidden_layers",
              "intermediate_size", "layer_norm_eps", "conv_bias", "conv_dim", "conv_kernel", "conv_stride", "vocab_size"):
        assert d[k] == getattr(hf, k), k                                      # Data2VecAudioConfig()'s defaults
    assert (d["conv_pos_kernel_size"], d["num_conv_pos_embeddings"], d["feat_extract_norm"], d["conv_bias"], d["do_stable_layer_norm"]) == \
        (19, 5, "layer", False, False)
    assert M.POS_LN_EPS == 1e-5 == torch.nn.LayerNorm(8).eps                  # not layer_norm_eps
    # whatever the source says about the extractor's norm and the encoder's layout, transformers ignores it here
    for src in (dict(feat_extract_norm="group", do_stable_layer_norm=True, conv_bias=False),
                dict(feat_extract_norm="group", do_stable_layer_norm=True, conv_bias=True),
                Data2VecAudioConfig(**TOY, feat_extract_norm="group", do_stable_layer_norm=True, conv_bias=True, layer_norm_eps=1e-3)):
        c = M.make_config(src)
        want_bias = src["conv_bias"] if isinstance(src, dict) else src.conv_bias
        assert (c["feat_extract_norm"], c["do_stable_layer_norm"], c["conv_bias"]) == ("layer", False, want_bias)
    assert c["layer_norm_eps"] == 1e-3 and c["hidden_size"] == 256
    with pytest.raises(DynError) as e:                                        # wav2vec2's own reader still refuses that extractor
        W2.make_config(dict(feat_extract_norm="layer", conv_bias=False))
    assert "conv_bias" in str(e.value)
    for bad, key in ((dict(add_adapter=True), "add_adapter"), (dict(num_conv_pos_embeddings=0), "num_conv_pos_embeddings"),
                     (dict(conv_pos_kernel_size=0), "conv_pos_kernel_size")):
        with pytest.raises(DynError) as e:
            M.make_config(bad)
        assert key in str(e.value), (bad, str(e.value))
    assert "conv_pos_kernel_size" not in W2.make_config(dict(conv_pos_kernel_size=4))              # wav2vec2's reader is unchanged
    p = tmp_path / "config.json"
    p.write_text(Data2VecAudioConfig(**TOY, conv_pos_kernel_size=4, num_conv_pos_embeddings=3, conv_bias=True).to_json_string(use_diff=False))
    assert R.model_type(str(p)) == "data2vec-audio"
    c = M.config_from_json(str(p))
    assert (c["conv_pos_kernel_size"], c["num_conv_pos_embeddings"], c["conv_bias"], c["feat_extract_norm"], c["conv_dim"]) == \
        (4, 3, True, "layer", (256,) * 7)
    bad = tmp_path / "adapter.json"
    bad.write_text(Data2VecAudioConfig(**TOY, add_adapter=True).to_json_string(use_diff=False))
    with pytest.raises(DynError) as e:
        M.config_from_json(str(bad))
    assert "add_adapter" in str(e.value)


def test_hubert_make_config_reads_its_keys_and_refuses_the_batch_norm_conv(tmp_path):
    from transformers import HubertConfig
    from dynamic_asr_eval_amd import hubert_model as M, run_wav2vec2 as R
    from dynamic_asr_eval_amd.ops import DynError
    d, hf = M.make_config(), HubertConfig()
    for k in ("feat_proj_layer_norm", "conv_pos_batch_norm", "mask_time_prob", "mask_feature_prob", "num_conv_pos_embeddings", "hidden_size",
              "feat_extract_norm", "conv_bias", "do_stable_layer_norm", "layer_norm_eps"):
        assert d[k] == getattr(hf, k), k                                      # HubertConfig()'s defaults
    assert M.make_config(dict(feat_proj_layer_norm=False))["feat_proj_layer_norm"] is False
    with pytest.raises(DynError) as e:
        M.make_config(dict(conv_pos_batch_norm=True))
    assert "conv_pos_batch_norm" in str(e.value)
    with pytest.raises(DynError) as e:                                        # the parent's refusals still hold
        M.make_config(dict(feat_extract_norm="layer", conv_bias=False))
    assert "conv_bias" in str(e.value)
    p = tmp_path / "config.json"
    p.write_text(HubertConfig(**TOY, feat_proj_layer_norm=False, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
                 .to_json_string(use_diff=False))
    assert R.model_type(str(p)) == "hubert"
    c = M.config_from_json(str(p))
    assert (c["feat_proj_layer_norm"], c["feat_extract_norm"], c["do_stable_layer_norm"], c["hidden_size"]) == (False, "layer", True, 256)
    bad = tmp_path / "bn.json"
    bad.write_text(HubertConfig(**TOY, conv_pos_batch_norm=True).to_json_string(use_diff=False))
    with pytest.raises(DynError) as e:
        M.config_from_json(str(bad))
    assert "conv_pos_batch_norm" in str(e.value)


def test_dispatch_builds_the_model_the_config_names(tmp_path, monkeypatch):
    """load_pretrained_model picks the class by `model_type`, under `--config` (checked here with the constructors replaced: no GPU)."""
    import argparse
    from transformers import Data2VecAudioConfig, HubertConfig, Wav2Vec2Config
    from dynamic_asr_eval_amd import data2vec_audio_model, hubert_model, run_wav2vec2 as R
    built = []

    class Stub:
        _prefix = "stub."

        def __init__(self, cfg, device=None):
            built.append((self.kind, cfg))

        def named_parameters(self):
            return []

    for mod, cls in ((data2vec_audio_model, "Data2VecAudioForCTC"), (hubert_model, "HubertForCTC"), (R, "Wav2Vec2ForCTC")):
        monkeypatch.setattr(mod, cls, type(cls, (Stub,), {"kind": cls}))
    for hf, want, key in ((Data2VecAudioConfig(**TOY), "Data2VecAudioForCTC", "conv_pos_kernel_size"),
                          (HubertConfig(**TOY), "HubertForCTC", "feat_proj_layer_norm"), (Wav2Vec2Config(**TOY), "Wav2Vec2ForCTC", "hidden_size")):
        p = tmp_path / f"{want}.json"
        p.write_text(hf.to_json_string(use_diff=False))
        assert R.model_type(str(p)) == hf.model_type
        R.load_pretrained_model(argparse.Namespace(config=str(p), checkpoint="", seed=0), "cpu")
        assert built[-1][0] == want and key in built[-1][1] and built[-1][1]["hidden_size"] == 256
    assert [k for k, _ in built] == ["Data2VecAudioForCTC", "HubertForCTC", "Wav2Vec2ForCTC"]


def test_the_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    p = 256                                                                   # never dereferenced: every call below fails, or has nothing to do, before a launch
    fwd = lambda B=2, T=5, Tg=5, H=256, G=16, yg=p, bias=p, act=p, xg=0: lib.dyn_posconv_ln_gelu_fwd(yg, bias, act, xg, p, p, B, T, Tg, H, G, 9, 1e-5, None, None)  # noqa: E731
    bwd = lambda B=2, T=5, Tg=5, H=256, G=16, dact=p, dyg=p, ws=p, wsb=1 << 20, db=p: lib.dyn_posconv_ln_gelu_bwd(p, p, p, p, dact, dyg, db, 1.0, B, T, Tg, H, G, None, ws, wsb, None)  # noqa: E731
    for call, name in ((fwd, b"dyn_posconv_ln_gelu_fwd"), (bwd, b"dyn_posconv_ln_gelu_bwd")):
        for kw, word in ((dict(H=320), b"multiple of 256"), (dict(H=1280), b"up to 1024"), (dict(H=768, G=128), b"multiple of 4"),
                         (dict(H=256, G=48), b"multiple of 4"), (dict(Tg=4), b"Tg >= T"), (dict(B=-1), b"bad dimensions")):
            assert call(**kw) == -1, (name, kw)                               # DYN_E_ARG
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(B=0) == 0 and call(T=0) == 0                              # nothing to do
    for kw in (dict(yg=0), dict(bias=0), dict(act=0, xg=0)):
        assert fwd(**kw) == -1 and b"null" in lib.dyn_last_error(), kw
    assert fwd(act=260) == -1 and b"aligned" in lib.dyn_last_error()
    for kw in (dict(dact=0), dict(dyg=0)):
        assert bwd(**kw) == -1 and b"null" in lib.dyn_last_error(), kw
    assert lib.dyn_posconv_ln_gelu_bwd_workspace_bytes(10, 256) == 3 * 256 * 4
    assert bwd(wsb=3 * 256 * 4 - 1) == -3 and bwd(ws=0) == -3                 # DYN_E_WORKSPACE
