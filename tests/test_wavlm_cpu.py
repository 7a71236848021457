"""WavLM without a GPU: the four new C-ABI entries' host-side argument checks, the host-built bucket table against transformers'
`_relative_positions_bucket`, the parameter list against transformers' `named_parameters()` for both layouts, and the configuration keys."""
import pytest
import torch

POST_GROUP = dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False)
STABLE_LAYER = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32)
NEW = ("dyn_relpos_gate_fwd", "dyn_softmax_relbias_fwd_len", "dyn_relbias_bwd", "dyn_relpos_gate_bwd")


def _calls(lib, p, B, T, H, nh):
    """The four entries with `p` for every pointer (never dereferenced: the checks fail, or succeed with B = 0, before any launch)."""
    return {
        "dyn_relpos_gate_fwd": lambda: lib.dyn_relpos_gate_fwd(p, p, p, p, p, p, p, B, T, H, nh, None),
        "dyn_softmax_relbias_fwd_len": lambda: lib.dyn_softmax_relbias_fwd_len(p, p, p, p, p, B, T, H, nh, T, 8, None, None),
        "dyn_relbias_bwd": lambda: lib.dyn_relbias_bwd(p, p, p, p, p, p, 1.0, B, T, H, nh, T, 8, p, 1 << 20, None),
        "dyn_relpos_gate_bwd": lambda: lib.dyn_relpos_gate_bwd(p, p, p, p, p, p, p, 1.0, p, p, p, 1.0, B, T, H, nh, p, 1 << 20, None),
    }


def test_the_four_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW + ("dyn_relbias_bwd_workspace_bytes", "dyn_relpos_gate_bwd_workspace_bytes"):
        assert n in names and hasattr(lib, n), n
    for name, call in _calls(lib, None, 2, 37, 192, 3).items():             # null pointers
        assert call() == -1, name                                           # DYN_E_ARG
        assert name.encode() in lib.dyn_last_error(), (name, lib.dyn_last_error())
    for name, call in _calls(lib, 256, 2, 37, 186, 3).items():              # D = 62: not a multiple of 4
        assert call() == -1, name
        assert name.encode() in lib.dyn_last_error() and b"multiple of 4" in lib.dyn_last_error(), (name, lib.dyn_last_error())
    for name, call in _calls(lib, 256, 2, 37, 190, 3).items():              # H % nh != 0
        assert call() == -1, name
        assert name.encode() in lib.dyn_last_error(), (name, lib.dyn_last_error())
    # num_buckets odd / beyond the LDS column, T beyond the softmax row limits (16384 forward, 8192 backward), table shorter than the scores
    for nbk, T, Tmax in ((7, 37, 37), (1026, 37, 37), (8, 16385, 16385), (8, 37, 36)):
        assert lib.dyn_softmax_relbias_fwd_len(256, 256, 256, 256, 256, 2, T, 192, 3, Tmax, nbk, None, None) == -1, (nbk, T, Tmax)
        assert b"dyn_softmax_relbias_fwd_len" in lib.dyn_last_error()
    for nbk, T, Tmax in ((7, 37, 37), (1026, 37, 37), (8, 8193, 8193), (8, 37, 36)):
        assert lib.dyn_relbias_bwd(256, 256, 256, 256, 256, 256, 1.0, 2, T, 192, 3, Tmax, nbk, 256, 1 << 40, None) == -1, (nbk, T, Tmax)
        assert b"dyn_relbias_bwd" in lib.dyn_last_error()
    need = lib.dyn_relbias_bwd_workspace_bytes(2, 3, 37, 8)
    assert need == (2 * 3 * 3 * (37 + 15) + 3 * 73) * 4                     # 3 blocks of 16 rows, T + 15 distances each; 2T - 1 per head
    assert lib.dyn_relbias_bwd(256, 256, 256, 256, 256, 256, 1.0, 2, 37, 192, 3, 37, 8, 256, need - 1, None) == -3      # DYN_E_WORKSPACE
    assert lib.dyn_relpos_gate_bwd_workspace_bytes(2, 37, 192, 3) >= (2 * 64 + 2) * 4
    assert lib.dyn_relpos_gate_bwd(256, 256, 256, 256, 256, 256, 256, 1.0, 256, 256, 256, 1.0, 2, 37, 192, 3, 256, 8, None) == -3
    for name, call in _calls(lib, 256, 0, 37, 192, 3).items():              # an empty batch passes the checks and launches nothing
        if name in ("dyn_relpos_gate_fwd", "dyn_softmax_relbias_fwd_len"):
            assert call() == 0, (name, lib.dyn_last_error())


@pytest.mark.parametrize("nbk,maxd,Tmax", [(8, 12, 18), (320, 800, 1500)])
def test_host_bucket_table_is_transformers(nbk, maxd, Tmax):
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    from dynamic_asr_eval_amd import ops
    att = WavLMAttention(embed_dim=16, num_heads=2, num_buckets=nbk, max_distance=maxd)
    want = att._relative_positions_bucket(torch.arange(-(Tmax - 1), Tmax, dtype=torch.long))
    got = ops.relative_position_buckets(Tmax, nbk, maxd)
    assert got.dtype == torch.int32 and got.shape == (2 * Tmax - 1,)
    assert torch.equal(got.long(), want)
    assert int(got.min()) == 0 and int(got.max()) == nbk - 1               # both tables reach the clamped last bucket
    if nbk == 8:                                                            # the exact, logarithmic and clamped branch on both signs
        assert sorted(set(got.tolist())) == [0, 1, 2, 3, 5, 6, 7]
    # the matrix form compute_bias builds: bucket[t, s] = table[s - t + Tmax - 1]
    T = 11
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None]
    assert torch.equal(got.long()[idx + Tmax - 1], att._relative_positions_bucket(idx))


@pytest.mark.parametrize("flags", [POST_GROUP, STABLE_LAYER], ids=["postln-group", "stable-layer"])
def test_param_spec_is_transformers_named_parameters(flags):
    from transformers import WavLMConfig, WavLMForCTC as HF
    from dynamic_asr_eval_amd import wavlm_model as M
    cfg = WavLMConfig(**TOY, **flags, num_buckets=8, max_bucket_distance=12)
    hf = {n: tuple(p.shape) for n, p in HF(cfg).named_parameters()}
    c = M.make_config(cfg)
    spec = M.param_spec(c)
    assert len(spec) == len({n for n, _, _ in spec})
    assert {n for n, _, _ in spec} == set(hf)
    hf_shape = {None: lambda s: s, "conv": lambda s: (s[0], s[2], s[1]), "g": lambda s: (1, 1, s[0]), "heads": lambda s: (1, s[0], 1, 1)}
    for n, shape, kind in spec:
        assert hf_shape[kind](tuple(shape)) == hf[n], (n, shape, kind, hf[n])
    assert [n for n in hf if n.endswith("rel_attn_embed.weight")] == ["wavlm.encoder.layers.0.attention.rel_attn_embed.weight"]
    assert all(n.startswith("wavlm.") or n.startswith("lm_head.") for n in hf)
    # the q | k | v slots stay side by side (one [3H, H] projection), the gate parameters come after the shared list
    names = [n for n, _, _ in spec]
    i = names.index("wavlm.encoder.layers.1.attention.q_proj.weight")
    assert names[i + 1].endswith("k_proj.weight") and names[i + 2].endswith("v_proj.weight")


def test_make_config_reads_the_bucket_keys(tmp_path):
    from transformers import WavLMConfig
    from dynamic_asr_eval_amd import wavlm_model as M, wav2vec2_model as W2
    from dynamic_asr_eval_amd.ops import DynError
    assert (M.make_config()["num_buckets"], M.make_config()["max_bucket_distance"]) == (320, 800)      # WavLMConfig()'s defaults
    assert (WavLMConfig().num_buckets, WavLMConfig().max_bucket_distance) == (320, 800)
    c = M.make_config(dict(num_buckets=8, max_bucket_distance=12, hidden_size=256, do_stable_layer_norm=True))
    assert (c["num_buckets"], c["max_bucket_distance"], c["hidden_size"], c["do_stable_layer_norm"]) == (8, 12, 256, True)
    c = M.make_config(WavLMConfig(**TOY, **STABLE_LAYER, num_buckets=16, max_bucket_distance=100))
    assert (c["num_buckets"], c["max_bucket_distance"], c["feat_extract_norm"], c["conv_bias"]) == (16, 100, "layer", True)
    p = tmp_path / "config.json"
    p.write_text(WavLMConfig(**TOY, **POST_GROUP, num_buckets=8, max_bucket_distance=12).to_json_string(use_diff=False))
    c = M.config_from_json(str(p))
    assert (c["num_buckets"], c["max_bucket_distance"], c["num_hidden_layers"]) == (8, 12, 2)
    from dynamic_asr_eval_amd import run_wav2vec2 as R
    assert R.model_type(str(p)) == "wavlm"
    with pytest.raises(DynError):
        M.make_config(dict(num_buckets=7))
    assert "num_buckets" not in W2.make_config(dict(num_buckets=8))        # wav2vec2's reader is unchanged: it ignores keys it does not know
