"""MMS adapters (`adapter_attn_dim`) without a GPU: the parameter list against transformers' Wav2Vec2ForCTC, the configuration reader, the
refusal by the other models of the family, the adapter-only trainable set against transformers' `_get_adapters()`, `--target-lang` loading
from local files with its tokenizer, and the new C-ABI entries' host-side argument checks.  No MMS checkpoint is on the machine: the oracle
is transformers' own class on the CPU with the same random state dict."""
import argparse
import json

import pytest
import torch

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32)
LAYER_STABLE = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
GROUP_STABLE = dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=True)
LAYER_POSTLN = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=False)
HF_SHAPE = {None: lambda s: tuple(s), "conv": lambda s: (s[0], s[2], s[1]), "g": lambda s: (1, 1, s[0])}
NEW = ("dyn_attn_adapter_fwd", "dyn_attn_adapter_bwd", "dyn_attn_adapter_bwd_workspace_bytes")


@pytest.mark.parametrize("flags", [LAYER_STABLE, GROUP_STABLE], ids=["layer-stable", "group-stable"])
@pytest.mark.parametrize("A", [16, 64])
def test_param_spec_is_transformers_parameter_list(flags, A):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC as HF
    from dynamic_asr_eval_amd.wav2vec2_model import make_config, param_spec
    cfg = Wav2Vec2Config(**TOY, **flags, adapter_attn_dim=A)
    want = {n: tuple(p.shape) for n, p in HF(cfg).named_parameters()}
    spec = param_spec(make_config(cfg))
    names = [n for n, _, _ in spec]
    assert len(names) == len(set(names))
    assert {n: HF_SHAPE[k](s) for n, s, k in spec} == want
    ad = [n for n in names if ".adapter_layer." in n]
    assert len(ad) == 12 and ad == [n for n in want if ".adapter_layer." in n]             # HF's order, layer by layer
    tail = lambda ns: [n for n in ns if ".layers.1." in n][-8:]                               # noqa: E731
    assert tail(names) == tail(list(want)) and tail(names)[1].endswith("final_layer_norm.bias")   # ... and after final_layer_norm
    shapes = {n: s for n, s, _ in spec}
    assert shapes["wav2vec2.encoder.layers.1.adapter_layer.linear_1.weight"] == (A, 256)
    assert shapes["wav2vec2.encoder.layers.1.adapter_layer.linear_2.weight"] == (256, A)


def test_post_ln_encoder_has_no_adapters_and_no_setting_keeps_the_spec():
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC as HF
    from dynamic_asr_eval_amd.wav2vec2_model import make_config, param_spec
    cfg = Wav2Vec2Config(**TOY, **LAYER_POSTLN, adapter_attn_dim=16)
    want = {n: tuple(p.shape) for n, p in HF(cfg).named_parameters()}
    spec = param_spec(make_config(cfg))
    assert not any(".adapter_layer." in n for n in want)
    assert {n: HF_SHAPE[k](s) for n, s, k in spec} == want
    for flags in (LAYER_STABLE, LAYER_POSTLN, {}):
        assert param_spec(make_config(dict(TOY, **flags))) == param_spec(make_config(dict(TOY, **flags, adapter_attn_dim=None)))
        assert not any(".adapter_layer." in n for n, _, _ in param_spec(make_config(dict(TOY, **flags))))


def test_config_reader_carries_adapter_attn_dim(tmp_path):
    from transformers import Wav2Vec2Config
    from dynamic_asr_eval_amd.ops import DynError
    from dynamic_asr_eval_amd.wav2vec2_model import config_from_json, make_config, param_spec
    p = tmp_path / "config.json"
    p.write_text(Wav2Vec2Config(**TOY, **LAYER_STABLE, adapter_attn_dim=16).to_json_string(use_diff=False))
    c = config_from_json(str(p))
    assert c["adapter_attn_dim"] == 16 and make_config(c) == c
    assert sum(".adapter_layer." in n for n, _, _ in param_spec(c)) == 12
    free = param_spec(make_config(dict(TOY, **LAYER_STABLE)))
    src = json.loads(p.read_text())
    src["adapter_attn_dim"] = None                                  # JSON null
    p.write_text(json.dumps(src))
    assert config_from_json(str(p))["adapter_attn_dim"] is None and param_spec(config_from_json(str(p))) == free
    del src["adapter_attn_dim"]
    p.write_text(json.dumps(src))
    assert config_from_json(str(p))["adapter_attn_dim"] is None and param_spec(config_from_json(str(p))) == free
    for bad in (6, 68, 0):
        with pytest.raises(DynError) as e:
            make_config(dict(TOY, **LAYER_STABLE, adapter_attn_dim=bad))
        assert "adapter_attn_dim" in str(e.value)


def test_the_other_models_refuse_adapter_attn_dim_by_name():
    from dynamic_asr_eval_amd import (data2vec_audio_model, hubert_model, sew_d_model, sew_model, wav2vec2_conformer_model, wavlm_model)
    from dynamic_asr_eval_amd.ops import DynError
    for mod in (wavlm_model, wav2vec2_conformer_model, data2vec_audio_model, hubert_model, sew_model, sew_d_model):
        mod.make_config(dict(adapter_attn_dim=None))
        for cfg in (dict(adapter_attn_dim=16), argparse.Namespace(adapter_attn_dim=16)):
            with pytest.raises(DynError) as e:
                mod.make_config(cfg)
            assert "adapter_attn_dim" in str(e.value), (mod.__name__, str(e.value))


class _Shell:
    """Wav2Vec2ForCTC's host-side state without its device buffers: what adapter_only() and trainable() look at."""

    def __init__(self, cfg):
        from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC, adapter_dim, make_config, param_spec
        self.cfg = make_config(cfg)
        self.spec = [(n, s) for n, s, _ in param_spec(self.cfg)]
        self.adapter_dim = adapter_dim(self.cfg)
        self.frozen = set()
        self.adapter_only = Wav2Vec2ForCTC.adapter_only.__get__(self)
        self.trainable = Wav2Vec2ForCTC.trainable.__get__(self)
        self._below_frozen = Wav2Vec2ForCTC._below_frozen.__get__(self)
        self._prefix = "wav2vec2."


def test_adapter_only_trains_what_get_adapters_lists():
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC as HF
    from dynamic_asr_eval_amd import run_wav2vec2 as R
    from dynamic_asr_eval_amd.ops import DynError
    cfg = Wav2Vec2Config(**TOY, **LAYER_STABLE, adapter_attn_dim=16)
    want = set(HF(cfg)._get_adapters())
    m = _Shell(cfg)
    assert not m._below_frozen()
    m.adapter_only()
    assert {n for n, _ in m.spec if m.trainable(n)} == want and len(want) == 14
    assert set(R.adapter_names(cfg)) == want
    assert m._below_frozen()
    for free in (dict(TOY, **LAYER_STABLE), dict(TOY, **LAYER_POSTLN, adapter_attn_dim=16)):
        with pytest.raises(DynError) as e:
            _Shell(free).adapter_only()
        assert "no adapters" in str(e.value)


def _adapter_file(cfg, vocab, seed=0):
    from dynamic_asr_eval_amd import run_wav2vec2 as R
    from dynamic_asr_eval_amd.wav2vec2_model import make_config, param_spec
    g = torch.Generator().manual_seed(seed)
    shapes = {n: s for n, s, _ in param_spec(make_config(dict(cfg, vocab_size=vocab)))}
    return {n: torch.randn(shapes[n], generator=g) for n in R.adapter_names(dict(cfg, vocab_size=vocab))}


def test_target_lang_loads_local_adapter_files_and_the_vocabulary(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from transformers import Wav2Vec2Config
    from dynamic_asr_eval_amd import run_wav2vec2 as R, wav2vec2_lib as W
    from dynamic_asr_eval_amd.wav2vec2_model import make_config, param_spec
    hf = Wav2Vec2Config(**TOY, **LAYER_STABLE, adapter_attn_dim=16)
    d = tmp_path / "mms"
    d.mkdir()
    (d / "config.json").write_text(hf.to_json_string(use_diff=False))
    base = {n: torch.zeros(HF_SHAPE[k](s)) for n, s, k in param_spec(make_config(hf))}       # lm_head [32, 256]: another vocabulary
    torch.save(base, str(d / "pytorch_model.bin"))
    ad = _adapter_file(TOY | LAYER_STABLE | dict(adapter_attn_dim=16), 11)
    save_file(ad, str(d / "adapter.xyz.safetensors"))
    torch.save(_adapter_file(TOY | LAYER_STABLE | dict(adapter_attn_dim=16), 11, seed=1), str(d / "adapter.bin_only.bin"))
    alphabet = ["<pad>", "<s>", "</s>", "<unk>", "|", "a", "b", "c", "d", "e", "'"]
    (d / "vocab.json").write_text(json.dumps({"xyz": {t: i for i, t in enumerate(alphabet)}, "bin_only": {t: i for i, t in enumerate(alphabet)}}))
    built = []

    class Stub:
        _prefix = "wav2vec2."

        def __init__(self, cfg, device=None):
            self.cfg = make_config(cfg)
            self.names = [n for n, _, _ in param_spec(self.cfg)]
            built.append(self)

        def load_state_dict(self, sd, strict=True):
            self.sd = sd
            return argparse.Namespace(missing_keys=[n for n in self.names if n not in sd], unexpected_keys=[k for k in sd if k not in self.names])

        def adapter_only(self):
            self.only = True

    monkeypatch.setattr(R, "Wav2Vec2ForCTC", Stub)
    args = argparse.Namespace(config="", checkpoint=str(d), seed=0, target_lang="xyz", adapter_only=True)
    model, tok = R.load_pretrained_model(args, "cpu")
    assert model.cfg["vocab_size"] == 11 and model.cfg["adapter_attn_dim"] == 16 and model.only
    assert tuple(model.sd["lm_head.weight"].shape) == (11, 256)                # the base's [32, 256] head was dropped, the file's loaded
    for n, t in ad.items():
        assert torch.equal(model.sd[n], t), n
    assert torch.equal(model.sd["wav2vec2.encoder.layers.0.layer_norm.weight"], torch.zeros(256))   # the rest is the base's
    assert isinstance(tok, R.VocabTokenizer) and (tok.vocab_size, tok.blank_id) == (11, 0)
    text = "a bad 'cab bed"
    assert tok.decode(tok(text).input_ids) == text
    assert tok("a z").input_ids == [5, 4, 3] and tok.decode([0, 5, 1, 4, 2, 6]) == "a b"
    model, _ = R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0, target_lang="bin_only"), "cpu")   # the .bin twin
    assert tuple(model.sd["lm_head.bias"].shape) == (11,) and not torch.equal(model.sd["lm_head.weight"], ad["lm_head.weight"])
    # a missing and an extra key are both named
    broken = dict(ad)
    del broken["wav2vec2.encoder.layers.1.adapter_layer.linear_2.bias"]
    broken["wav2vec2.encoder.layers.2.adapter_layer.norm.weight"] = torch.zeros(256)
    save_file(broken, str(d / "adapter.bad.safetensors"))
    with pytest.raises(KeyError) as e:
        R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0, target_lang="bad"), "cpu")
    assert "layers.1.adapter_layer.linear_2.bias" in str(e.value) and "layers.2.adapter_layer.norm.weight" in str(e.value)
    with pytest.raises(FileNotFoundError):
        R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0, target_lang="none"), "cpu")
    # without --target-lang the directory's own weights load; a flat vocab.json is read as it is; without one the CharTokenizer stays
    (d / "vocab.json").write_text(json.dumps({t: i for i, t in enumerate(alphabet)}))
    _, tok = R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0), "cpu")
    assert isinstance(tok, R.VocabTokenizer) and tok.decode(tok("ab e").input_ids) == "ab e"
    (d / "vocab.json").unlink()
    _, tok = R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0), "cpu")
    assert isinstance(tok, W.CharTokenizer)


def test_an_mms_state_dict_is_refused_by_an_adapter_free_configuration(tmp_path, monkeypatch):
    """The silent drop this used to be: adapter tensors in the checkpoint, no adapter_attn_dim in the configuration."""
    from transformers import Wav2Vec2Config
    from dynamic_asr_eval_amd import run_wav2vec2 as R
    from dynamic_asr_eval_amd.wav2vec2_model import make_config, param_spec
    d = tmp_path / "m"
    d.mkdir()
    (d / "config.json").write_text(Wav2Vec2Config(**TOY, **LAYER_STABLE).to_json_string(use_diff=False))
    with_ad = make_config(dict(TOY, **LAYER_STABLE, adapter_attn_dim=16))
    torch.save({n: torch.zeros(HF_SHAPE[k](s)) for n, s, k in param_spec(with_ad)}, str(d / "pytorch_model.bin"))

    class Stub:
        _prefix = "wav2vec2."

        def __init__(self, cfg, device=None):
            self.names = [n for n, _, _ in param_spec(make_config(cfg))]

        def load_state_dict(self, sd, strict=True):
            return argparse.Namespace(missing_keys=[n for n in self.names if n not in sd], unexpected_keys=[k for k in sd if k not in self.names])

    monkeypatch.setattr(R, "Wav2Vec2ForCTC", Stub)
    with pytest.raises(KeyError) as e:
        R.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(d), seed=0), "cpu")
    assert "adapter_layer" in str(e.value) and "12 adapter parameters" in str(e.value)


def test_synthetic_init_starts_the_adapter_norm_at_one():
    from dynamic_asr_eval_amd import run_wav2vec2 as R
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC, make_config, param_spec

    class Model:
        _norm_weight_suffixes = Wav2Vec2ForCTC._norm_weight_suffixes

        def __init__(self):
            self.p = [(n, torch.zeros(s)) for n, s, _ in param_spec(make_config(dict(TOY, **LAYER_STABLE, adapter_attn_dim=16)))]

        def named_parameters(self):
            return self.p

    m = Model()
    R.init_synthetic(m, 0)
    for n, p in m.p:
        if n.endswith("adapter_layer.norm.weight"):
            assert abs(p.mean().item() - 1.0) < 0.02, n
        if n.endswith("adapter_layer.norm.bias") or n.endswith("adapter_layer.linear_2.bias"):
            assert abs(p.mean().item()) < 0.02, n


def test_the_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    p = 256                                                         # never dereferenced: every call below fails, or has nothing to do, before a launch
    fwd = lambda M=3, H=256, A=16, x=p: lib.dyn_attn_adapter_fwd(x, p, p, p, p, p, p, p + 4096, None, None, None, M, H, A, 1e-5, None)  # noqa: E731
    bwd = lambda M=3, H=256, A=16, x=p, ws=p, wsb=1 << 30, dx=p + 8192: lib.dyn_attn_adapter_bwd(  # noqa: E731
        x, p, p, p, p, p, p, p, p + 4096, dx, p, p, p, p, p, p, M, H, A, ws, wsb, None)
    for call, name in ((fwd, b"dyn_attn_adapter_fwd"), (bwd, b"dyn_attn_adapter_bwd")):
        for kw, word in ((dict(H=300), b"H=300"), (dict(H=2304), b"H=2304"), (dict(A=6), b"A=6"), (dict(A=68), b"A=68"), (dict(x=0), b"null"),
                         (dict(M=-1), b"M=-1"), (dict(x=260), b"aligned")):
            assert call(**kw) == -1, (name, kw)                     # DYN_E_ARG
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(M=0) == 0
    assert bwd(dx=p + 4096) == -1 and b"alias" in lib.dyn_last_error()
    need = lib.dyn_attn_adapter_bwd_workspace_bytes(67, 1280, 16)
    assert need >= (67 * 16 + 17 * 3 * 1280) * 4                    # du [M, A] and ceil(67 / 4) partial rows of three H-wide sums
    assert bwd(M=67, H=1280, wsb=need - 1) == -3 and bwd(M=67, H=1280, ws=0) == -3          # DYN_E_WORKSPACE
    assert b"dyn_attn_adapter_bwd" in lib.dyn_last_error()
