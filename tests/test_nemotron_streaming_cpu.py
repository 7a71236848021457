"""What of NemotronAsrStreamingForRNNT (nemotron_asr_streaming_model.py) can be checked without a GPU: the chunked limited-context mask
restated in tests/nemotron_refs.py against the mask transformers hands its attention layers, the band's closed forms, the frame
arithmetic, the configuration reader and its refusals, the parameter list against transformers' state dict, the C-ABI surface and the
decode oracle's conditions."""
import argparse
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import nemotron_refs as NR  # noqa: E402
import rnnt_refs as R  # noqa: E402

ENTRIES = ("dyn_softmax_relshift_band_fwd", "dyn_relshift_band_bwd", "dyn_conv2d_first_causal_fwd", "dyn_conv2d_causal_wgrad_workspace_bytes",
           "dyn_conv2d_first_causal_wgrad", "dyn_dwconv2d_s2_causal_fwd_act", "dyn_dwconv2d_s2_causal_dgrad_act",
           "dyn_dwconv2d_s2_causal_wgrad_act", "dyn_convmod_causal_k9_fwd", "dyn_dwconv1d_causal_k9_dgrad",
           "dyn_dwconv1d_causal_k9_wgrad_workspace_bytes", "dyn_dwconv1d_causal_k9_wgrad")


@pytest.mark.parametrize("sw,look", [(9, 2), (9, 0), (9, 3), (71, 13), (0, 2)])
def test_restated_mask_equals_the_mask_transformers_passes_to_attention(sw, look):
    """T = 259 gives T' = 34 (a multiple of cs only for cs = 1), T = 131 gives T' = 18; the lookahead once from the configuration's default
    and once as the forward's argument."""
    cfg, ref = NR.hf_model(seed=0, arch=dict(NR.TOY, sliding_window=sw, default_num_lookahead_tokens=look))
    for T, Tp in ((259, 34), (131, 18)):
        m = NR.captured_mask(ref, torch.randn(1, T, 80, generator=torch.Generator().manual_seed(T)))
        assert m.shape == (Tp, Tp) and torch.equal(m, NR.chunked_mask(Tp, sw - 1, look)), (sw, look, T)
    other = look + 2
    m = NR.captured_mask(ref, torch.randn(1, 259, 80, generator=torch.Generator().manual_seed(1)), num_lookahead_tokens=other)
    assert torch.equal(m, NR.chunked_mask(34, sw - 1, other)) and not torch.equal(m, NR.chunked_mask(34, sw - 1, look))


@pytest.mark.parametrize("left,look", [(8, 2), (8, 0), (8, 3), (70, 13), (70, 6), (70, 1), (70, 0), (-1, 2), (70, 299), (3, 5)])
def test_band_width_and_key_ranges_equal_the_closed_forms(left, look):
    """ops.chunked_band against the mask: every row's visible keys are the contiguous, never empty closed-form range, every visible
    (i, j) falls on band column j - i + dlo in [0, W), both end columns are reached once T' is large enough, and W is then
    lc cs + 2 cs - 1 (97, 83, 73, 71 for the released sliding_window 71 and the processor's lookaheads)."""
    from dynamic_asr_eval_amd import ops
    for T in (1, 5, 34, 257, 600):
        b = ops.chunked_band(T, left, look)
        mask = NR.chunked_mask(T, left, look)
        cols = set()
        for i in range(T):
            j0, j1 = NR.key_range(i, T, left, look)
            assert 0 <= j0 < j1 <= T and mask[i].nonzero().flatten().tolist() == list(range(j0, j1)), (T, i)
            cols.update((j0 - i + b.dlo, j1 - 1 - i + b.dlo))
        assert min(cols) == 0 and max(cols) == b.W - 1 and b.r0 == T - 1 - b.dlo and b.r0 + b.W <= 2 * T - 1, (T, vars(b))
        W = NR.band_width(left, look)
        if W is None or W >= 2 * T - 1:
            assert b.W <= 2 * T - 1 and (b.W == 2 * T - 1 if (left < 0 and look + 1 >= T) else True)
        elif T - 1 >= b.lc * b.cs + b.cs - 1:
            assert b.W == W, (T, b.W, W)
    assert {k: NR.band_width(70, k) for k in (13, 6, 1, 0)} == {13: 97, 6: 83, 1: 73, 0: 71}
    assert ops.chunked_band(256, 70, 13).W == 97


def test_frames_equal_transformers_output_lengths():
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM
    cfg, ref = NR.hf_model(seed=0)
    Ts = [1, 2, 7, 8, 131, 259]
    assert [NM.frames(T) for T in Ts] == ref.encoder._get_subsampling_output_length(torch.tensor(Ts)).tolist()
    for T in (1, 7, 131):
        with torch.no_grad():
            assert ref.encoder(input_features=torch.zeros(1, T, 80)).last_hidden_state.shape[1] == NM.frames(T)
    assert NM.frames(131) == 18 and NM.frames(259) == 34 and [NM.frames(F) for F in (80, 128)] == [11, 17]


def test_make_config_round_trips_the_default_and_the_toy_configuration(tmp_path):
    from transformers import NemotronAsrStreamingConfig
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM
    want = NemotronAsrStreamingConfig()
    for c in (NM.make_config(), NM.make_config(want), NM.make_config(want.to_dict())):
        for k in ("vocab_size", "decoder_hidden_size", "num_decoder_layers", "max_symbols_per_step", "blank_token_id", "pad_token_id"):
            assert c[k] == getattr(want, k), k
        for k in NM.ENCODER_KEYS:
            if k not in ("num_key_value_heads", "head_dim"):
                assert c[k] == getattr(want.encoder_config, k), k
        assert c["joint_hidden_act"] == "relu" and c["durations"] == () and c["head_dim"] == 128
        assert (c["sliding_window"], c["default_num_lookahead_tokens"], c["vocab_size"], c["blank_token_id"]) == (71, 13, 1025, 1024)
    toy = NR.hf_config()
    p = tmp_path / "config.json"
    p.write_text(toy.to_json_string(use_diff=False))
    assert NM.config_from_json(str(p)) == NM.make_config(toy)
    assert NM.make_config(toy)["sliding_window"] == 9 and NM.make_config(toy)["num_mel_bins"] == 80
    odd = NM.make_config(NR.hf_config(arch=dict(NR.TOY, num_mel_bins=41)))      # no multiple-of-8 rule here
    assert odd["num_mel_bins"] == 41


@pytest.mark.parametrize("word,over,enc", [
    ("subsampling_factor", {}, dict(subsampling_factor=4)), ("subsampling_conv_kernel_size", {}, dict(subsampling_conv_kernel_size=5)),
    ("subsampling_conv_stride", {}, dict(subsampling_conv_stride=1)), ("conv_kernel_size", {}, dict(conv_kernel_size=31)),
    ("hidden_act", {}, dict(hidden_act="gelu")), ("of the joint", dict(hidden_act="tanh"), {}), ("hidden_size", {}, dict(hidden_size=384)),
    ("default_num_lookahead_tokens", {}, dict(default_num_lookahead_tokens=-1)),
    ("default_num_lookahead_tokens", {}, dict(default_num_lookahead_tokens=1.5)), ("sliding_window", {}, dict(sliding_window=0)),
    ("parakeet_rnnt", dict(model_type="parakeet_rnnt"), {}), ("parakeet_tdt", dict(model_type="parakeet_tdt"), {}),
    ("parakeet_ctc", dict(model_type="parakeet_ctc"), {}), ("Parakeet", dict(durations=[0, 1, 2]), {}),
    ("decoder_hidden_size", dict(decoder_hidden_size=66), {}), ("blank_token_id", dict(blank_token_id=40), {}),
    ("subsampling_conv_channels", {}, dict(subsampling_conv_channels=30))], ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(word, over, enc):
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM
    from dynamic_asr_eval_amd.ops import DynError
    base = NR.hf_config().to_dict()
    base["encoder_config"] = dict(base["encoder_config"], **enc)
    with pytest.raises(DynError) as e:
        NM.make_config(dict(base, **over))
    assert word in str(e.value), str(e.value)


def test_call_time_refusals_and_the_waveform_harness(tmp_path):
    """attention_mask, the three streaming caches, a bad lookahead, too many frames and batch_renorm_training() are refused by name before anything
    touches the device (no instance is needed: the checks come first); run_wav2vec2 points a nemotron_asr_streaming config.json to this
    module; a Parakeet RNN-T reader refuses this model_type."""
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM, parakeet_rnnt_model as RM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    M = NM.NemotronAsrStreamingForRNNT
    fake = argparse.Namespace(cfg=NM.make_config(NR.hf_config()), _refuse_caches=lambda kw: M._refuse_caches(None, kw), frames=NM.frames)
    x, ids = torch.zeros(1, 8, 80), torch.zeros(1, 1, dtype=torch.int64)
    with pytest.raises(DynError) as e:
        M.forward(fake, x, decoder_input_ids=ids, attention_mask=torch.ones(1, 8))
    assert "attention_mask" in str(e.value)
    for k, v in (("use_cache", True), ("past_key_values", object()), ("padding_cache", object())):
        for call in (lambda **kw: M.forward(fake, x, decoder_input_ids=ids, **kw), lambda **kw: M.encode(fake, x, **kw)):
            with pytest.raises(DynError) as e:
                call(**{k: v})
            assert k in str(e.value) and "streaming caches" in str(e.value)
    for bad in (-1, 1.5, True):
        with pytest.raises(DynError) as e:
            M.encode(fake, x, num_lookahead_tokens=bad)
        assert "num_lookahead_tokens" in str(e.value)
    with pytest.raises(DynError) as e:
        M.encode(argparse.Namespace(cfg=dict(fake.cfg, max_position_embeddings=4), _refuse_caches=fake._refuse_caches, frames=NM.frames),
                 torch.zeros(1, 64, 80))
    assert "max_position_embeddings" in str(e.value)
    with pytest.raises(DynError) as e:
        M.batch_renorm_training(None)
    assert "batch_renorm_training" in str(e.value)
    with pytest.raises(DynError) as e:
        RM.make_config(NR.hf_config().to_dict())
    assert "nemotron_asr_streaming" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    (d / "config.json").write_text(NR.hf_config().to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "nemotron_asr_streaming"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "nemotron_asr_streaming_model" in str(e.value) and "dynamic_eval_transducer_loss" in str(e.value)


def test_param_spec_equals_transformers_state_dict():
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM
    for arch in (NR.TOY, dict(NR.TOY, convolution_bias=False, attention_bias=False, num_mel_bins=41)):
        cfg, ref = NR.hf_model(seed=0, arch=arch)
        sd = ref.state_dict()
        spec = NM.param_spec(NM.make_config(cfg))
        assert {n for n, _, _ in spec} == set(sd) and len(spec) == len(sd)
        for n, shape, kind in spec:
            hf = tuple(sd[n].shape)
            want = {"dw": shape[:1] + (1,) + shape[1:], "pw": shape + (1,), "pw2": shape + (1, 1)}.get(kind, shape)
            assert hf == want, (n, hf, shape, kind)
        assert not any(n.endswith(("running_mean", "running_var")) for n in sd)


def test_header_entries_are_exported_and_refuse_before_any_launch():
    """The new entries are in include/dyneval.h and in the library; argument errors come back as codes before any launch, so dummy
    pointers are never dereferenced: DYN_E_ARG (-1), DYN_E_WORKSPACE (-3), DYN_E_UNSUPPORTED (-4)."""
    from dynamic_asr_eval_amd import _lib
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    lib = _lib.load()
    for n in _lib.exported_symbols():
        assert hasattr(lib, n), n
    p, q, big = 256, 512, 1 << 40
    assert lib.dyn_softmax_relshift_band_fwd(None, p, q, 4, 34, 97, 14, 5, None) == -1
    assert lib.dyn_softmax_relshift_band_fwd(p, p, q, 4, 34, 97, 0, 5, None) == -1 and b"chunk size" in lib.dyn_last_error()
    assert lib.dyn_softmax_relshift_band_fwd(p, p, q, 4, 256, 96, 14, 5, None) == -1 and b"97" in lib.dyn_last_error()
    assert lib.dyn_softmax_relshift_band_fwd(p, q, q, 4, 34, 97, 14, 5, None) == -1
    assert lib.dyn_softmax_relshift_band_fwd(p, p, q, 4, 20000, 97, 14, 5, None) == -1
    assert lib.dyn_relshift_band_bwd(p, q, 4, 34, 46, 14, -1, None) == -1 and lib.dyn_relshift_band_bwd(p, p, 4, 34, 97, 14, 5, None) == -1
    assert lib.dyn_conv2d_first_causal_fwd(p, p, p, p, 2, 0, 80, 32, None) == -1
    assert lib.dyn_conv2d_first_causal_fwd(p, p, p, p, 2, 8, 80, 30, None) == -4
    assert lib.dyn_dwconv2d_s2_causal_fwd_act(p, p, p, p, 2, 8, 41, 32, 0, None) == -4 and b"ReLU" in lib.dyn_last_error()
    assert lib.dyn_dwconv2d_s2_causal_dgrad_act(p, p, p, None, 2, 8, 41, 32, 1, None) == -1
    need = lib.dyn_conv2d_causal_wgrad_workspace_bytes(2, 8, 32)
    assert need == 2 * 5 * 32 * 10 * 4
    assert lib.dyn_dwconv2d_s2_causal_wgrad_act(p, p, p, p, 1.0, 2, 8, 41, 32, 1, p, need - 1, None) == -3
    assert lib.dyn_conv2d_first_causal_wgrad(p, p, p, p, 1.0, 2, 8, 80, 32, None, big, None) == -3
    assert lib.dyn_convmod_causal_k9_fwd(p, p, None, p, p, p, None, None, None, None, None, 2, 9, 256, 31, 1e-5, None) == -4
    assert lib.dyn_convmod_causal_k9_fwd(p, p, None, p, p, p, None, None, None, None, None, 2, 9, 384, 9, 1e-5, None) == -4
    assert lib.dyn_convmod_causal_k9_fwd(p, p, None, p, p + 4, p, None, None, None, None, None, 2, 9, 256, 9, 1e-5, None) == -1
    assert lib.dyn_dwconv1d_causal_k9_dgrad(p, p, None, 2, 9, 256, 9, 0.0, None) == -1
    need = lib.dyn_dwconv1d_causal_k9_wgrad_workspace_bytes(2, 34, 256, 9)
    assert lib.dyn_dwconv1d_causal_k9_wgrad(p, p, p, 1.0, 2, 34, 256, 9, p, need - 1, None) == -3
    assert lib.dyn_dwconv1d_causal_k9_wgrad(p, p, p, 1.0, 2, 34, 256, 31, p, big, None) == -4


def test_decode_oracle_satisfies_the_gpu_tests_conditions():
    """transformers' greedy decode on the inputs tests/test_nemotron_streaming_gpu.py gives generate() (nemotron_refs.DECODE,
    max_symbols_per_step = 3): the top-two logit gap at every decode step exceeds 1e-3 (rnnt_refs.assert_decode_conditions asks 1e-2),
    blank and non-blank steps, a frame left unforced after two or more symbols, a forced advance; every row reaches the end."""
    cfg, ref = NR.decode_model()
    assert cfg.max_symbols_per_step == 3
    for B in (1, 3):
        rows, Tp, margin = NR.decode_case(B, ref)
        assert margin > 1e-3 and Tp == 39 and all(r["finished"] for r in rows)
        R.assert_decode_conditions(rows, margin, cfg.max_symbols_per_step)
