"""What of LasrForCTC (lasr_model.py), the host side of its kernels (the 32-tap instances of csrc/convmod_bn.hip and of dyn_dwconv1d_wgrad), the
loop's constants (nvidia_ctc_lib.loop_constants) and the loop's test-side oracle (tests/lasr_refs.py) can be checked without a GPU, against
transformers' LasrForCTC."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import lasr_refs as R  # noqa: E402


def test_make_config_defaults_are_transformers():
    from transformers import LasrCTCConfig
    from dynamic_asr_eval_amd import lasr_model as LM
    theirs = LasrCTCConfig()
    c = LM.make_config()
    for k in LM.DEFAULT_CONFIG:
        want = getattr(theirs, k) if k in ("vocab_size", "pad_token_id") else getattr(theirs.encoder_config, k, None)
        if k == "head_dim":
            want = theirs.encoder_config.hidden_size // theirs.encoder_config.num_attention_heads
        want = tuple(want) if isinstance(want, (list, tuple)) else want
        assert c[k] == want, (k, c[k], want)
    assert LM.make_config(theirs) == c == LM.make_config(theirs.to_dict())         # the object and the nested dict of a config.json read the same
    flat = dict(theirs.encoder_config.to_dict(), vocab_size=theirs.vocab_size, pad_token_id=theirs.pad_token_id)
    assert LM.make_config(flat) == c


def test_config_from_json(tmp_path):
    from dynamic_asr_eval_amd import lasr_model as LM
    cfg = R.hf_config(attention_bias=True)
    with open(tmp_path / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    c = LM.config_from_json(str(tmp_path / "config.json"))
    assert c == LM.make_config(cfg) and c["attention_bias"] is True and c["vocab_size"] == R.VOCAB and c["hidden_size"] == 256


@pytest.mark.parametrize("key,over", [
    ("conv_kernel_size", dict(conv_kernel_size=31)), ("conv_kernel_size", dict(conv_kernel_size=9)),
    ("subsampling_conv_kernel_size", dict(subsampling_conv_kernel_size=3)), ("subsampling_conv_stride", dict(subsampling_conv_stride=1)),
    ("hidden_size", dict(hidden_size=384)), ("hidden_size", dict(hidden_size=1280, num_attention_heads=8)), ("hidden_act", dict(hidden_act="gelu")),
    ("num_key_value_heads", dict(num_key_value_heads=2)), ("head_dim", dict(hidden_size=768, num_attention_heads=256)),
    ("rope_type", dict(rope_parameters={"rope_type": "linear", "rope_theta": 10000.0, "factor": 2.0})),
    ("feed_forward_residual_weights", dict(feed_forward_residual_weights=[1.0])),
    ("feed_forward_residual_weights", dict(feed_forward_residual_weights=[1.0, 0.5, 0.5])),
    ("conv_residual_weights", dict(conv_residual_weights=[2.0, "1"])), ("conv_residual_weights", dict(conv_residual_weights=1.0)),
    ("subsampling_conv_channels", dict(subsampling_conv_channels=250)), ("num_mel_bins", dict(num_mel_bins=81))],
    ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(key, over):
    """A flat dict, so that no transformers validation stands between the value and make_config."""
    from dynamic_asr_eval_amd import lasr_model as LM
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        LM.make_config(dict(R.TOY, vocab_size=R.VOCAB, pad_token_id=R.PAD, **over))
    assert key in str(e.value), str(e.value)
    with pytest.raises(DynError):                                 # and nested, as a config.json holds it
        LM.make_config(dict(vocab_size=R.VOCAB, pad_token_id=R.PAD, encoder_config=dict(R.TOY, **over)))


def test_attention_mask_short_input_and_the_waveform_harness_are_refused(tmp_path):
    """forward() refuses an attention mask before it looks at the input (so no GPU is needed to see it); run_wav2vec2.load_pretrained_model
    refuses a lasr_ctc config.json with the pointer it gives for parakeet_ctc."""
    from dynamic_asr_eval_amd import lasr_model as LM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        LM.LasrForCTC.forward(None, torch.zeros(1, 16, 128), attention_mask=torch.ones(1, 16))
    assert "attention_mask" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(R.hf_config().to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "lasr_ctc"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "lasr_ctc" in str(e.value) and "features" in str(e.value) and "nvidia_ctc_lib" in str(e.value) and "LasrForCTC" in str(e.value)
    assert LM.MIN_FRAMES == 13 and LM.frames(13) == 1 and LM.frames(12) < 1


def test_frame_count_is_transformers():
    from transformers import LasrForCTC
    from dynamic_asr_eval_amd import lasr_model as LM
    ref = LasrForCTC(R.hf_config(dict(R.TOY, num_hidden_layers=1)))
    want = ref._get_subsampling_output_length(torch.arange(13, 301))
    assert [LM.frames(T) for T in range(13, 301)] == want.tolist()
    assert (LM.frames(13), LM.frames(77), LM.frames(141), LM.frames(2048), LM.frames(128), LM.frames(108)) == (1, 17, 33, 509, 29, 24)


@pytest.mark.parametrize("D", [32, 64])
def test_rotary_table_is_transformers_bit_for_bit(D):
    """The host table against LasrEncoderRotaryEmbedding: bit-equal on this platform (both sides evaluate the same torch expressions on the
    CPU, so the same libm serves both), both halves of transformers' cat((freqs, freqs)) table."""
    from transformers.models.lasr.modeling_lasr import LasrEncoderRotaryEmbedding
    from dynamic_asr_eval_amd import lasr_model as LM
    enc = R.hf_config(dict(R.TOY, hidden_size=256, num_attention_heads=256 // D)).encoder_config
    theirs = LasrEncoderRotaryEmbedding(enc)
    for T in (1, 2, 17, 509):
        cos, sin = theirs(torch.zeros(1, T, 256), torch.arange(T).unsqueeze(0))
        got_cos, got_sin = LM.rotary_table(T, D, enc.rope_parameters["rope_theta"])
        assert got_cos.dtype == torch.float32 and got_cos.shape == got_sin.shape == (T, D // 2) and cos.shape == (1, T, D)
        for half in (slice(0, D // 2), slice(D // 2, D)):
            assert torch.equal(got_cos, cos[0, :, half]) and torch.equal(got_sin, sin[0, :, half]), (T, D)
    assert not torch.equal(LM.rotary_table(17, D)[1][0], LM.rotary_table(17, D)[1][16])


def test_rotary_convention_is_apply_rotary_pos_emb():
    """dyn_rotary's rule (csrc/stitch.hip: (x1 c - x2 s, x2 c + x1 s) on the halves) restated in torch equals transformers'
    x cos + rotate_half(x) sin with the cat((freqs, freqs)) table, bit for bit: the halves are not interleaved."""
    from transformers.models.lasr.modeling_lasr import apply_rotary_pos_emb
    from dynamic_asr_eval_amd import lasr_model as LM
    T, D = 9, 32
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(2, 4, T, D, generator=g), torch.randn(2, 4, T, D, generator=g)
    c, s = LM.rotary_table(T, D)
    want_q, want_k = apply_rotary_pos_emb(q, k, torch.cat((c, c), -1)[None], torch.cat((s, s), -1)[None])
    for x, want in ((q, want_q), (k, want_k)):
        x1, x2 = x[..., :D // 2], x[..., D // 2:]
        assert torch.equal(torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1), want)


def test_conv1d_weight_permutation_round_trips_bit_for_bit():
    from dynamic_asr_eval_amd import wav2vec2_model as W2
    w = torch.randn(6, 4, 5, generator=torch.Generator().manual_seed(1))           # transformers' [Cout, Cin, k]
    native = W2._conv_to_native(w)                                                 # [Cout, k, Cin]: a row of the implicit GEMM's B operand
    assert native.shape == (6, 5, 4) and torch.equal(W2._conv_to_hf(native), w) and not torch.equal(native.reshape(6, -1), w.reshape(6, -1))
    # the implicit GEMM over channels-last rows with the permuted weight is the convolution
    x = torch.randn(2, 13, 4, generator=torch.Generator().manual_seed(2))
    rows = torch.stack([x[:, 2 * t:2 * t + 5].reshape(2, -1) for t in range(5)], 1)
    want = torch.nn.functional.conv1d(x.transpose(1, 2), w, stride=2).transpose(1, 2)
    assert torch.allclose(rows @ native.reshape(6, -1).t(), want, atol=1e-5)


@pytest.mark.parametrize("over", [{}, dict(attention_bias=True), dict(convolution_bias=True)], ids=["toy", "attention-bias", "convolution-bias"])
def test_param_spec_buffers_and_alias_table_cover_transformers_state_dict(over):
    from transformers import LasrForCTC
    from dynamic_asr_eval_amd import lasr_model as LM
    cfg = R.hf_config(**over)
    ref = LasrForCTC(cfg)
    sd = ref.state_dict()
    c = LM.make_config(cfg)
    hf_shape = {"pw": lambda s: s + (1,), "dw": lambda s: (s[0], 1) + s[1:], "conv": lambda s: (s[0], s[2], s[1]), None: lambda s: s}
    ours = {n: hf_shape[kind](tuple(shape)) for n, shape, kind in LM.param_spec(c)}
    bufs = {n: tuple(shape) for n, shape, _ in LM.buffer_spec(c)}
    assert not set(ours) & set(bufs) and set(ours) | set(bufs) == set(sd) and set(ours) == {n for n, _ in ref.named_parameters()}
    for n, shape in {**ours, **bufs}.items():
        assert tuple(sd[n].shape) == shape, (n, tuple(sd[n].shape), shape)
    assert ("encoder.layers.0.self_attn.q_proj.bias" in ours) == over.get("attention_bias", False)
    assert ("encoder.layers.0.conv.depthwise_conv.bias" in ours) == over.get("convolution_bias", False)
    # the alias table: every per-layer parameter of the 2-layer model whose group the shared layer code names differently is reached
    assert c["num_hidden_layers"] == 2
    theirs = {b for _, b in LM.LAYER_NAMES}
    groups = {n.split(".", 3)[3].rsplit(".", 1)[0] for n in ours if n.startswith("encoder.layers.")}
    own = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "norm_conv", "conv.pointwise_conv1", "conv.depthwise_conv", "conv.norm",
           "conv.pointwise_conv2"}                                # read under transformers' own names by lasr_model / the packed q | k | v views
    assert groups == theirs | own, groups ^ (theirs | own)
    assert "self_attn.relative_k_proj" not in theirs and len(LM.LAYER_NAMES) == 9


def test_loop_constants_of_a_parakeet_model_are_the_old_ones():
    from dynamic_asr_eval_amd import lasr_model as LM, nvidia_ctc_lib as N, parakeet_model as PM
    assert N.loop_constants(PM.ParakeetForCTC) == (8, ("encoder.subsampling.", "ctc_head.")) == (8, PM.FROZEN_IN_THE_LOOP)
    assert N.loop_constants(object()) == (8, ("encoder.subsampling.", "ctc_head."))                # a model that does not say: the reference's
    assert N.loop_constants(LM.LasrForCTC) == (4, ("encoder.subsampler.", "ctc_head."))


def test_32_tap_entries_dispatch_on_the_host():
    """32 taps are built beside 9, 31 / 33 / 7 stay DYN_E_UNSUPPORTED (-4), before any launch (B = 0 returns at once, so a built width
    answers 0 without a GPU); the zero-argument tile entry keeps its value."""
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    p = 256
    assert lib.dyn_convmod_bn_time_tile() == 16 and lib.dyn_convmod_bn_time_tile_kw(9) == 16 and lib.dyn_convmod_bn_time_tile_kw(32) >= 1
    assert lib.dyn_convmod_bn_time_tile_kw(31) == 0
    for KW, rc in ((32, 0), (9, 0), (31, -4), (33, -4), (7, -4), (16, -4)):
        assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, 0, 8, 512, KW, 0, 1e-5, None) == rc, (KW, lib.dyn_last_error())
        assert lib.dyn_glu_dwconv1d_dgrad(p, p, 512, 1024, None, 0, 8, 512, KW, None) == rc, (KW, lib.dyn_last_error())
    assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, 2, 8, 300, 32, 0, 1e-5, None) == -4
    assert lib.dyn_dwconv1d_wgrad_workspace_bytes(2, 64, 512, 32) == 2 * 8 * 512 * 33 * 4


def test_loop_oracle_has_teeth_on_the_gpu_tests_inputs():
    """The test-side oracle (tests/lasr_refs.py) on the inputs tests/test_lasr_gpu.py gives the loop: four windows of 128, 128, 128 and 108
    frames -> 29, 29, 29, 24 encoder frames, u_len / ds_len = 4.41 / 4.5 (no integer), overlap_ds = int(64 / ratio) = 14 -> 29 + 15 + 15 + 10 = 69 rows;
    every window's pseudo-label sequence non-empty; the smallest top-2 log-prob margin over all stitched frames at least 1e-2 (ten times the
    GPU test's bar, so no argmax can flip by rounding); at least a quarter of the frames non-blank; an adapted result more than 1e-2 away
    from the unadapted one; the weights restored bit for bit."""
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
    assert adapted.shape == plain.shape == (R.LOOP_ROWS, R.VOCAB) and np.isfinite(adapted).all()
    assert np.abs(adapted - plain).max() > 1e-2, np.abs(adapted - plain).max()
    top2 = np.sort(adapted, -1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() >= 1e-2
    assert (adapted.argmax(-1) != R.PAD).mean() >= 0.25
    for n, p in ref.named_parameters():
        assert torch.equal(p, before[n]) and p.requires_grad, n
