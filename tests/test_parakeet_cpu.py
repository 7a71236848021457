"""What of ParakeetForCTC (parakeet_model.py), its kernels' host side (csrc/convmod_bn.hip, the `_act` entries of csrc/conv.hip) and the
loop's test-side oracle (tests/parakeet_refs.py) can be checked without a GPU, against transformers' ParakeetForCTC."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as R  # noqa: E402


@pytest.mark.parametrize("over", [{}, dict(attention_bias=False), dict(convolution_bias=False), dict(scale_input=False)],
                         ids=["toy", "no-attention-bias", "no-convolution-bias", "no-scale-input"])
def test_param_spec_and_buffers_are_transformers_state_dict(over):
    from transformers import ParakeetForCTC
    from dynamic_asr_eval_amd import parakeet_model as PM
    cfg = R.hf_config(**over)
    sd = ParakeetForCTC(cfg).state_dict()
    c = PM.make_config(cfg)
    assert (c["attention_bias"], c["convolution_bias"], c["scale_input"]) == tuple(over.get(k, True) for k in ("attention_bias", "convolution_bias", "scale_input"))
    C, F3, H = c["subsampling_conv_channels"], c["num_mel_bins"] // 8, c["hidden_size"]
    hf_shape = {"pw": lambda s: s + (1,), "dw": lambda s: (s[0], 1) + s[1:], "pw2": lambda s: s + (1, 1), "sublin": lambda s: s, None: lambda s: s}
    ours = {n: hf_shape[kind](tuple(shape)) for n, shape, kind in PM.param_spec(c)}
    bufs = {n: tuple(shape) for n, shape, _ in PM.buffer_spec(c)}
    assert not set(ours) & set(bufs)
    assert set(ours) | set(bufs) == set(sd)
    for n, shape in {**ours, **bufs}.items():
        assert tuple(sd[n].shape) == shape, (n, tuple(sd[n].shape), shape)
    assert ours["encoder.subsampling.linear.weight"] == (H, C * F3)
    assert ("encoder.layers.0.self_attn.q_proj.bias" in ours) == over.get("attention_bias", True)
    assert ("encoder.layers.0.conv.depthwise_conv.bias" in ours) == over.get("convolution_bias", True)
    assert PM.make_config(cfg.to_dict()) == c                                        # the nested dict of a config.json reads the same


@pytest.mark.parametrize("H", [256, 1024])
def test_position_table_is_transformers_bit_for_bit(H):
    from transformers.models.parakeet.modeling_parakeet import ParakeetEncoderRelPositionalEncoding
    from dynamic_asr_eval_amd import parakeet_model as PM
    enc = R.hf_config(dict(R.TOY, hidden_size=H)).encoder_config
    theirs = ParakeetEncoderRelPositionalEncoding(enc)
    for T in (1, 2, 9, 256):
        want = theirs(torch.zeros(3, T, H))
        got = PM.position_table(T, H)
        assert got.dtype == torch.float32 and got.shape == (2 * T - 1, H)
        for b in range(3):
            assert torch.equal(got, want[b]), (T, H)
    assert not torch.equal(PM.position_table(9, H)[0], PM.position_table(9, H)[-1])   # positions T - 1 and -(T - 1): sin changes sign


def test_frame_count_is_transformers():
    from transformers import ParakeetForCTC
    from dynamic_asr_eval_amd import parakeet_model as PM
    ref = ParakeetForCTC(R.hf_config(dict(R.TOY, num_hidden_layers=1)))
    want = ref._get_subsampling_output_length(torch.arange(1, 71))
    assert [PM.frames(T) for T in range(1, 71)] == want.tolist()
    assert PM.frames(67) == 9 and PM.frames(131) == 17 and PM.frames(128) == 16 and PM.frames(108) == 14


def test_subsampling_linear_column_permutation_round_trips():
    from dynamic_asr_eval_amd import parakeet_model as PM
    H, C, F3 = 5, 8, 3
    w = torch.randn(H, C * F3, generator=torch.Generator().manual_seed(1))
    native = PM.sublin_from_hf(w, C, F3)
    assert torch.equal(PM.sublin_to_hf(native, C, F3), w) and torch.equal(PM.sublin_from_hf(PM.sublin_to_hf(w, C, F3), C, F3), w)
    assert not torch.equal(native, w)
    # transformers flattens [B, C, T, F] -> (c, f) columns, the channels-last kernels [B, T, F, C] -> (f, c): the same product either way
    a = torch.randn(2, C, 4, F3, generator=torch.Generator().manual_seed(2))
    theirs = a.transpose(1, 2).reshape(2, 4, -1) @ w.t()
    ours = a.permute(0, 2, 3, 1).reshape(2, 4, -1) @ native.t()
    assert torch.allclose(theirs, ours, atol=1e-5)


@pytest.mark.parametrize("key,over", [
    ("subsampling_factor", dict(subsampling_factor=4)), ("subsampling_conv_kernel_size", dict(subsampling_conv_kernel_size=5)),
    ("subsampling_conv_stride", dict(subsampling_conv_stride=1)), ("subsampling_conv_channels", dict(subsampling_conv_channels=250)),
    ("num_mel_bins", dict(num_mel_bins=84)), ("hidden_size", dict(hidden_size=384)), ("hidden_size", dict(hidden_size=1280, num_attention_heads=8)),
    ("conv_kernel_size", dict(conv_kernel_size=31)), ("hidden_act", dict(hidden_act="gelu")), ("num_key_value_heads", dict(num_key_value_heads=2)),
    ("head_dim", dict(head_dim=32))], ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(key, over):
    from dynamic_asr_eval_amd import parakeet_model as PM
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        PM.make_config(dict(vocab_size=R.VOCAB, pad_token_id=R.PAD, encoder_config=dict(R.TOY, **over)))
    assert key in str(e.value), str(e.value)


def test_attention_mask_and_the_waveform_harness_are_refused(tmp_path):
    """forward() refuses an attention mask before it looks at the input (so no GPU is needed to see it); run_wav2vec2.load_pretrained_model
    refuses a parakeet_ctc config.json and names the library that drives this family."""
    from dynamic_asr_eval_amd import parakeet_model as PM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        PM.ParakeetForCTC.forward(None, torch.zeros(1, 8, 80), attention_mask=torch.ones(1, 8))
    assert "attention_mask" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(R.hf_config().to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "parakeet_ctc"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "parakeet_ctc" in str(e.value) and "features" in str(e.value) and "nvidia_ctc_lib" in str(e.value)


def test_new_entries_refuse_what_they_have_no_instance_for():
    """dyn_convmod_bn_fwd / _bwd_act, dyn_glu_dwconv1d_dgrad and the `_act` entries of the depthwise 3x3 stage dispatch on the host: an unbuilt
    C / KW / act is DYN_E_UNSUPPORTED (-4), a null pointer or bad size DYN_E_ARG (-1), a short workspace DYN_E_WORKSPACE, all before any
    launch, so dummy pointers are never dereferenced (tests/test_host_cpu.py::test_conv_entries_refuse_what_they_have_no_instance_for)."""
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    p, big = 256, 1 << 40
    B, T = 2, 8
    assert lib.dyn_convmod_bn_time_tile() >= 1
    for C, KW, act in ((300, 9, 0), (1280, 9, 0), (256, 31, 0), (256, 7, 0), (256, 9, 1)):
        assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, B, T, C, KW, act, 1e-5, None) == -4, (C, KW, act, lib.dyn_last_error())
        assert b"dyn_convmod_bn_fwd" in lib.dyn_last_error()
        if KW == 9:
            assert lib.dyn_convmod_bn_bwd_act(p, p, p, p, p, p, p, p, p, p, 1.0, None, B, T, C, act, 1e-5, p, big, None) == -4, (C, act, lib.dyn_last_error())
            assert b"dyn_convmod_bn_bwd_act" in lib.dyn_last_error()
        if act == 0:
            assert lib.dyn_glu_dwconv1d_dgrad(p, p, 512, 1024, None, B, T, C, KW, None) == -4, (C, KW, lib.dyn_last_error())
            assert b"dyn_glu_dwconv1d_dgrad" in lib.dyn_last_error()
    assert lib.dyn_convmod_bn_fwd(None, p, p, p, p, p, p, p, p, p, None, B, T, 256, 9, 0, 1e-5, None) == -1
    assert lib.dyn_convmod_bn_fwd(p, p, None, p, p, p, p, None, p, p, None, B, T, 256, 9, 0, 1e-5, None) == -1          # s is required, cbias is not
    assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, -1, T, 256, 9, 0, 1e-5, None) == -1
    assert lib.dyn_convmod_bn_bwd_act(p, p, p, p, p, None, p, p, p, p, 1.0, None, B, T, 256, 0, 1e-5, p, big, None) == -1
    need = lib.dyn_convmod_bn_bwd_act_workspace_bytes(B, T, 256)
    assert need == 3 * B * T * 256 * 4
    assert lib.dyn_convmod_bn_bwd_act(p, p, p, p, p, p, p, p, p, p, 1.0, None, B, T, 256, 0, 1e-5, p, need - 1, None) == -3, lib.dyn_last_error()
    assert lib.dyn_convmod_bn_bwd_act(p, p, p, p, p, p, p, p, p, p, 1.0, None, B, T, 256, 0, 1e-5, None, big, None) == -3
    assert lib.dyn_glu_dwconv1d_dgrad(p, p, p, None, None, B, T, 256, 9, None) == -1
    assert lib.dyn_glu_dwconv1d_dgrad(p, p, 512, p, None, B, T, 256, 9, None) == -1                                    # du aliases u
    for act in (2, -1):
        assert lib.dyn_dwconv2d_s2_fwd_act(p, p, p, p, B, T, 8, 8, act, None) == -4, lib.dyn_last_error()
        assert b"dyn_dwconv2d_s2_fwd_act" in lib.dyn_last_error()
        assert lib.dyn_dwconv2d_s2_dgrad_act(p, p, p, p, B, T, 8, 8, act, None) == -4
        assert lib.dyn_dwconv2d_s2_wgrad_act(p, p, p, p, 1.0, B, T, 8, 8, act, p, big, None) == -4
    for act in (0, 1):
        assert lib.dyn_dwconv2d_s2_fwd_act(p, p, None, p, B, T, 8, 8, act, None) == -1
        assert lib.dyn_dwconv2d_s2_wgrad_act(p, p, p, p, 1.0, B, T, 8, 8, act, p, 16, None) == -3
        assert lib.dyn_dwconv2d_s2_fwd_act(p, p, p, p, 0, T, 8, 8, act, None) == 0
    assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, 0, T, 256, 9, 0, 1e-5, None) == 0
    assert lib.dyn_relu_fwd(None, p, 8, None) == -1 and lib.dyn_relu_bwd(p, p, 260, 8, None) == -1 and lib.dyn_relu_fwd(p, p, 0, None) == 0


def test_loop_oracle_has_teeth_on_the_gpu_tests_inputs():
    """The test-side oracle of tests/parakeet_refs.py (reference nvidia_ctc/lib.py:35-193 on transformers' model) on the inputs
    tests/test_parakeet_gpu.py gives the loop: four windows (the last one shorter), every window's pseudo-label sequence non-empty, and an
    adapted result more than 1e-2 away from the unadapted one (at the reference's lr of 1e-8 a step is invisible: the tests use 1e-5, as the
    sibling loops' tests do).  The weights are restored bit for bit."""
    L = R.LOOP
    spec, tok = R.loop_inputs()
    cfg, ref = R.hf_model(seed=L["seed"], blank_bias=L["blank_bias"])
    before = {n: p.detach().clone() for n, p in ref.named_parameters()}
    args = argparse.Namespace(epochs=1, shuffle=False)
    labels = []
    gen = lambda: torch.Generator().manual_seed(L["mask_seed"])                                   # noqa: E731
    adapted = R.dynamic_eval_ref(args, ref, spec, L["seq_len"], L["overlap"], tok, L["num_negatives"], L["lr_args"], generator=gen(), labels_out=labels)
    plain = R.dynamic_eval_ref(args, ref, spec, L["seq_len"], L["overlap"], tok, L["num_negatives"], L["lr_args"], generator=gen(), adapt=False)
    assert len(labels) == 4 and all(len(ids) > 0 for ids in labels), labels
    assert adapted.shape == plain.shape == (16 + 8 + 8 + 6, R.VOCAB) and np.isfinite(adapted).all()
    assert np.abs(adapted - plain).max() > 1e-2, np.abs(adapted - plain).max()
    top2 = np.sort(adapted, -1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 1e-2          # no argmax of the oracle sits on a tie the GPU test's 1e-3 could flip
    for n, p in ref.named_parameters():
        assert torch.equal(p, before[n]) and p.requires_grad, n
