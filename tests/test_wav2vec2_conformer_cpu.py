"""Wav2Vec2-Conformer without a GPU: the new C-ABI entries' host-side argument checks, the host-built position tables against transformers'
Wav2Vec2ConformerRelPositionalEmbedding / RotaryPositionalEmbedding, the parameter list against transformers' `named_parameters()` for both
position types and both extractor layouts, the configuration keys and refusals, and the harness's model_type dispatch."""
import pytest
import torch

GROUP = dict(feat_extract_norm="group", conv_bias=False)
LAYER = dict(feat_extract_norm="layer", conv_bias=True)
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32, hidden_act="swish")
NEW = ("dyn_softmax_relshift_fwd_len", "dyn_relshift_bwd", "dyn_head_bias_add", "dyn_head_bias_bwd")


def _calls(lib, p, M, T, ld, rows=74, H=192, ldq=576):
    """The four entries with `p` for every pointer (never dereferenced: the checks fail, or succeed with nothing to do, before any launch)."""
    return {
        "dyn_softmax_relshift_fwd_len": lambda: lib.dyn_softmax_relshift_fwd_len(p, p + 4096 if p else p, p + 8192 if p else p, M, T, ld, None, None),
        "dyn_relshift_bwd": lambda: lib.dyn_relshift_bwd(p, p + 4096 if p else p, M, T, ld, None),
        "dyn_head_bias_add": lambda: lib.dyn_head_bias_add(p, ldq, p, p, p, p, rows, H, None),
        "dyn_head_bias_bwd": lambda: lib.dyn_head_bias_bwd(p, p, p, ldq, p, p, 1.0, rows, H, p, 1 << 20, None),
    }


def test_the_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW + ("dyn_head_bias_bwd_workspace_bytes",):
        assert n in names and hasattr(lib, n), n
    for name, call in _calls(lib, None, 6, 37, 73).items():                  # null pointers
        assert call() == -1, name                                            # DYN_E_ARG
        assert name.encode() in lib.dyn_last_error() and b"null pointer" in lib.dyn_last_error(), (name, lib.dyn_last_error())
    score = ("dyn_softmax_relshift_fwd_len", "dyn_relshift_bwd")
    # T < 1; ld_bd one short of the 2T - 1 relative positions; T beyond the softmax's row limit
    for T, ld, word in ((0, 8, b"bad sizes"), (37, 72, b"ld_bd"), (16385, 2 * 16385 - 1, b"row length")):
        for name in score:
            assert _calls(lib, 256, 6, T, ld)[name]() == -1, (name, T, ld)
            assert name.encode() in lib.dyn_last_error() and word in lib.dyn_last_error(), (name, lib.dyn_last_error())
    assert lib.dyn_softmax_relshift_fwd_len(256, 512, 512, 6, 37, 73, None, None) == -1          # the output may alias the scores, not BD
    assert lib.dyn_relshift_bwd(256, 256, 6, 37, 73, None) == -1
    for name in score:                                                       # an empty batch passes the checks and launches nothing
        assert _calls(lib, 256, 0, 37, 73)[name]() == 0, (name, lib.dyn_last_error())
        assert _calls(lib, 256, 0, 1, 1)[name]() == 0, (name, lib.dyn_last_error())            # T = 1: one relative position
    # head biases: H and ldq multiples of 4, ldq >= H, 16-byte alignment
    for kw in (dict(H=190, ldq=570), dict(H=192, ldq=574), dict(H=192, ldq=188), dict(H=0)):
        assert _calls(lib, 256, 6, 37, 73, **kw)["dyn_head_bias_add"]() == -1, kw
        assert b"dyn_head_bias_add" in lib.dyn_last_error()
    assert lib.dyn_head_bias_add(260, 576, 256, 256, 256, 256, 74, 192, None) == -1 and b"aligned" in lib.dyn_last_error()
    assert lib.dyn_head_bias_add(256, 576, 256, 256, 256, 256, 0, 192, None) == 0
    for kw in (dict(H=192, ldq=188), dict(H=0), dict(rows=-1)):
        assert _calls(lib, 256, 6, 37, 73, **kw)["dyn_head_bias_bwd"]() == -1, kw
        assert b"dyn_head_bias_bwd" in lib.dyn_last_error()
    need = lib.dyn_head_bias_bwd_workspace_bytes(74, 192)
    assert need == 2 * 10 * 192 * 4                                          # ceil(74 / 8) = 10 partial rows for u and for v
    assert lib.dyn_head_bias_bwd_workspace_bytes(10000, 1024) == 2 * 500 * 1024 * 4      # at most 512 chunks: 20 rows each -> 500
    assert lib.dyn_head_bias_bwd(256, 256, 256, 576, 256, 256, 1.0, 74, 192, 256, need - 1, None) == -3       # DYN_E_WORKSPACE


def _hf_cfg(**kw):
    from transformers import Wav2Vec2ConformerConfig
    return Wav2Vec2ConformerConfig(**kw)


@pytest.mark.parametrize("T,H,max_len", [(1, 256, 5000), (2, 256, 5000), (18, 256, 5000), (93, 256, 5000), (300, 256, 5000), (41, 8, 40)])
def test_relative_position_table_is_transformers(T, H, max_len):
    """Also with more frames than max_source_positions, where transformers rebuilds its table at the input's length."""
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerRelPositionalEmbedding as Emb
    from dynamic_asr_eval_amd import ops
    want = Emb(_hf_cfg(hidden_size=H, max_source_positions=max_len))(torch.zeros(1, T, H))[0]
    got = ops.relative_position_table(T, H)
    assert got.dtype == torch.float32 and got.shape == (2 * T - 1, H) and got.is_contiguous()
    assert torch.equal(got, want)
    assert torch.equal(got[T - 1], torch.tensor([0.0, 1.0] * (H // 2)))       # the middle row is relative position 0
    if T > 1:                                                                 # row k is relative position T - 1 - k: positive ones first
        assert got[0, 0].item() == pytest.approx(torch.sin(torch.tensor(float(T - 1))).item(), abs=1e-6)
        assert torch.equal(got[0, 0::2], -got[-1, 0::2]) and torch.equal(got[0, 1::2], got[-1, 1::2])


@pytest.mark.parametrize("T,D,base", [(1, 64, 10000), (93, 64, 10000), (300, 32, 500)])
def test_rotary_tables_are_the_first_half_of_transformers(T, D, base):
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerRotaryPositionalEmbedding as Emb
    from dynamic_asr_eval_amd import ops
    both = Emb(_hf_cfg(hidden_size=4 * D, num_attention_heads=4, rotary_embedding_base=base))(torch.zeros(1, T, 4 * D))   # [2, T, 1, 1, D]
    cos, sin = ops.rotary_tables(T, D, base)
    assert cos.shape == sin.shape == (T, D // 2) and cos.is_contiguous() and sin.is_contiguous()
    assert torch.equal(cos, both[0, :, 0, 0, :D // 2]) and torch.equal(sin, both[1, :, 0, 0, :D // 2])
    assert torch.equal(both[0, :, 0, 0, D // 2:], cos) and torch.equal(both[1, :, 0, 0, D // 2:], sin)     # the second half repeats the first


@pytest.mark.parametrize("pos", ["relative", "rotary"])
@pytest.mark.parametrize("flags", [GROUP, LAYER], ids=["group", "layer"])
def test_param_spec_is_transformers_named_parameters(pos, flags):
    from transformers import Wav2Vec2ConformerForCTC as HF
    from dynamic_asr_eval_amd import wav2vec2_conformer_model as M
    cfg = _hf_cfg(**TOY, **flags, position_embeddings_type=pos)
    ref = HF(cfg)
    hf = {n: tuple(p.shape) for n, p in ref.named_parameters()}
    c = M.make_config(cfg)
    spec = M.param_spec(c)
    assert len(spec) == len({n for n, _, _ in spec})
    assert {n for n, _, _ in spec} == set(hf)
    hf_shape = {None: lambda s: s, "conv": lambda s: (s[0], s[2], s[1]), "g": lambda s: (1, 1, s[0]), "pw": lambda s: s + (1,),
                "dw": lambda s: (s[0], 1, s[1])}
    for n, shape, kind in spec:
        assert hf_shape[kind](tuple(shape)) == hf[n], (n, shape, kind, hf[n])
    assert all(n.startswith("wav2vec2_conformer.") or n.startswith("lm_head.") for n in hf)
    assert any(n.endswith("self_attn.pos_bias_u") for n in hf) == (pos == "relative")
    names = [n for n, _, _ in spec]                                           # the q | k | v slots stay side by side
    i = names.index("wav2vec2_conformer.encoder.layers.1.self_attn.linear_q.weight")
    assert names[i + 1].endswith("linear_k.weight") and names[i + 2].endswith("linear_v.weight")
    assert names[i + 3].endswith("linear_q.bias") and names[i + 5].endswith("linear_v.bias")
    bufs = {n for n, _ in ref.named_buffers() if "batch_norm" in n}           # what state_dict() adds to the parameters
    assert bufs == {f"wav2vec2_conformer.encoder.layers.{l}.conv_module.batch_norm.{b}" for l in range(2) for b in M.BN_BUFFERS}


def test_make_config_reads_the_new_keys_and_refuses_what_is_not_built(tmp_path):
    from dynamic_asr_eval_amd import wav2vec2_conformer_model as M, wav2vec2_model as W2, run_wav2vec2 as R
    from dynamic_asr_eval_amd.ops import DynError
    d, hf = M.make_config(), _hf_cfg()
    for k in ("position_embeddings_type", "rotary_embedding_base", "max_source_positions", "conv_depthwise_kernel_size", "hidden_act",
              "hidden_size", "num_hidden_layers", "intermediate_size", "layer_norm_eps", "feat_extract_norm", "conv_bias"):
        assert d[k] == getattr(hf, k), k                                      # Wav2Vec2ConformerConfig()'s defaults
    assert (d["position_embeddings_type"], d["conv_depthwise_kernel_size"], d["hidden_act"]) == ("relative", 31, "gelu")
    c = M.make_config(_hf_cfg(**TOY, **LAYER, position_embeddings_type="rotary", rotary_embedding_base=500, conv_depthwise_kernel_size=15,
                              layer_norm_eps=1e-3))
    assert (c["position_embeddings_type"], c["rotary_embedding_base"], c["conv_depthwise_kernel_size"], c["hidden_act"], c["layer_norm_eps"],
            c["feat_extract_norm"], c["conv_bias"], c["do_stable_layer_norm"]) == ("rotary", 500, 15, "swish", 1e-3, "layer", True, False)
    for bad, key in ((dict(position_embeddings_type="absolute"), "position_embeddings_type"), (dict(position_embeddings_type=None), "position_embeddings_type"),
                     (dict(add_adapter=True), "add_adapter"), (dict(hidden_act="relu"), "hidden_act"),
                     (dict(conv_depthwise_kernel_size=30), "conv_depthwise_kernel_size"), (dict(conv_depthwise_kernel_size=33), "conv_depthwise_kernel_size"),
                     (dict(position_embeddings_type="rotary", hidden_size=36, num_attention_heads=4), "rotary")):
        with pytest.raises(DynError) as e:
            M.make_config(bad)
        assert key in str(e.value), (bad, str(e.value))
    assert "position_embeddings_type" not in W2.make_config(dict(position_embeddings_type="rotary"))       # wav2vec2's reader is unchanged
    p = tmp_path / "config.json"
    p.write_text(_hf_cfg(**TOY, **GROUP, position_embeddings_type="rotary").to_json_string(use_diff=False))
    assert R.model_type(str(p)) == "wav2vec2-conformer"
    c = M.config_from_json(str(p))
    assert (c["position_embeddings_type"], c["hidden_act"], c["num_hidden_layers"], c["conv_dim"]) == ("rotary", "swish", 2, (256,) * 7)


def test_the_committed_large_config_is_the_published_architecture():
    import os
    from dynamic_asr_eval_amd import wav2vec2_conformer_model as M, run_wav2vec2 as R
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wav2vec2_conformer_rel_pos_large_config.json")
    assert R.model_type(p) == "wav2vec2-conformer"
    c = M.config_from_json(p)
    assert (c["num_hidden_layers"], c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["feat_extract_norm"], c["conv_bias"],
            c["hidden_act"], c["conv_depthwise_kernel_size"], c["position_embeddings_type"]) == (24, 1024, 16, 4096, "layer", True, "swish", 31, "relative")
    spec = M.param_spec(c)
    assert sum(torch.Size(s).numel() for _, s, _ in spec) > 590e6             # the ~0.6 B parameters of the large conformer
