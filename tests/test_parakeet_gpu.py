"""ParakeetForCTC (parakeet_model.py: the FastConformer encoder on the parent's conformer layer code, the x8 ReLU subsampling on
csrc/conv.hip, the conv module on csrc/convmod_bn.hip) against transformers' ParakeetForCTC on the CPU with the same random state dict —
logits, every parameter gradient, the optional-bias and scale_input variants, state-dict round trip, reproducibility, active subsets,
frozen prefixes — and nvidia_ctc_lib.dynamic_eval against the test-side oracle of the reference's loop (tests/parakeet_refs.py)."""
import argparse
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

SUB, HEAD = "encoder.subsampling.", "ctc_head."


def _pair(cuda, arch=R.TOY, seed=0, blank_bias=0.0, **over):
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    cfg, ref = R.hf_model(arch, seed, blank_bias, **over)
    hip = ParakeetForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _forward_and_every_gradient(cuda, ref, hip, x, g, logit_bar):
    out_ref = ref(input_features=x).logits
    res = hip(input_features=x.to(cuda))
    out = res.logits
    assert out.shape == out_ref.shape and res.frames == out.shape[1]
    err = (out.cpu() - out_ref).abs().max().item()
    top = out_ref.abs().max().item()
    print(f"forward err {err:.3e}, max |logit| {top:.3e}, bar {logit_bar * max(1.0, top):.3e}")
    assert err < logit_bar * max(1.0, top), (err, top)
    gl = torch.randn(out_ref.shape, generator=g) / out_ref.numel()
    ref.zero_grad()
    out_ref.backward(gl)
    hip.zero_grad(); hip.backward(gl.to(cuda))
    grads = hip.grads_hf()
    named = dict(ref.named_parameters())
    assert set(grads) == set(named)
    worst = 0.0
    for n, p in named.items():
        assert p.grad is not None, n
        assert grads[n].shape == p.grad.shape, n
        diff = (grads[n].cpu() - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
        assert scale > 0.0, n
    print("worst relative gradient error", worst)
    return grads


def _state_dict_round_trip(ref, hip):
    sd = hip.state_dict()                                   # transformers' names and layouts, bit for bit; parameters + the batch-norm buffers
    want = ref.state_dict()
    bn = {n for n, _ in ref.named_buffers() if ".conv.norm." in n}
    assert len(bn) == 3 * hip.cfg["num_hidden_layers"]
    assert set(sd) == {n for n, _ in ref.named_parameters()} | bn == set(want)
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n
    for n in bn:                                            # outside the flat vector: no optimiser step can move them
        assert n not in hip.P and n in hip.buffers_
    before = hip.flat_params.clone()
    hip.load_state_dict(sd)
    assert torch.equal(hip.flat_params, before)


@pytest.mark.parametrize("shape,over", [((3, 67, 80), {}), ((2, 131, 80), {}), ((3, 67, 80), dict(attention_bias=False)),
                                        ((3, 67, 80), dict(convolution_bias=False)), ((3, 67, 80), dict(scale_input=False))],
                         ids=["9-frames", "17-frames", "no-attention-bias", "no-convolution-bias", "no-scale-input"])
def test_forward_backward_matches_transformers(cuda, shape, over):
    """67 feature frames give 9 encoder frames (= the depthwise kernel's 9 taps: every frame inside its halo), 131 give 17 (a second time tile
    of the conv-module kernels).  Logits within 2e-4 * max(1, max |logit|) (scale_input multiplies the residual stream by 16), every
    parameter's gradient within 3e-3 of its largest entry + 2e-8: the bars tests/test_wav2vec2_conformer_gpu.py gives this layer stack.
    Measured (MI355X): logits within 5.4e-07 .. 8.9e-07 (max |logit| 0.6 .. 0.9), worst relative gradient error 1.1e-06 .. 3.3e-04."""
    ref, hip = _pair(cuda, **over)
    for k, v in over.items():
        assert hip.cfg[k] is v
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    from dynamic_asr_eval_amd.parakeet_model import frames
    assert frames(shape[1]) == (9 if shape[1] == 67 else 17)
    grads = _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    assert ("encoder.layers.0.self_attn.q_proj.bias" in grads) == over.get("attention_bias", True)
    assert ("encoder.layers.0.conv.depthwise_conv.bias" in grads) == over.get("convolution_bias", True)
    _state_dict_round_trip(ref, hip)


def test_wide_shape_forward_and_every_gradient(cuda):
    """The published width (1024 hidden, 8 x 128 heads) without the 24 layers and with a narrow FFN.  Measured (MI355X): logits within 1.1e-06
    (max |logit| 1.5, bar 7.6e-04), worst relative gradient error 4.6e-04."""
    ref, hip = _pair(cuda, arch=R.WIDE)
    g = torch.Generator().manual_seed(11)
    _forward_and_every_gradient(cuda, ref, hip, torch.randn(2, 67, 80, generator=g), g, 5e-4)


def test_backward_is_bit_reproducible(cuda):
    ref, hip = _pair(cuda, seed=1)
    x = torch.randn(2, 131, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert first.abs().max().item() > 0.0


def test_active_subset_backward(cuda):
    """n_active = 2 of 3 equals the full backward with a zero gradient on the third row, to 1e-5 of the largest entry."""
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(3, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out)
    gl[:2] = torch.randn(2, *out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:2].contiguous(), n_active=2)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_frozen_prefixes(cuda, monkeypatch):
    """With `encoder.subsampling.` and `ctc_head.` frozen (the reference loop's freeze): their gradients are exact zeros, every other gradient
    keeps its bits, and no subsampling backward kernel is launched (their wrappers are made to raise)."""
    from dynamic_asr_eval_amd import ops
    ref, hip = _pair(cuda, seed=4)
    x = torch.randn(2, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl)
    free = {n: hip.G[n].clone() for n, _ in hip.spec}
    assert all(free[n].abs().max().item() > 0.0 for n in free if n.startswith((SUB, HEAD)))

    def forbidden(*a, **k):
        raise AssertionError("a subsampling backward kernel was launched although the subsampling is frozen")

    for name in ("dwconv2d_s2_wgrad_act", "dwconv2d_s2_dgrad_act", "conv2d_first_wgrad", "relu_bwd"):
        monkeypatch.setattr(ops, name, forbidden)
    hip.frozen = {SUB, HEAD}
    hip(x); hip.zero_grad(); hip.backward(gl)
    for n, _ in hip.spec:
        if n.startswith((SUB, HEAD)):
            assert hip.G[n].abs().max().item() == 0.0, n
        else:
            assert torch.equal(hip.G[n], free[n]), n
    hip.frozen = {"encoder.layers.0.self_attn.relative_k_proj", "encoder.layers.0.self_attn.bias_", "encoder.layers.1.feed_forward1.linear1.bias"}
    monkeypatch.undo()
    hip(x); hip.zero_grad(); hip.backward(gl)
    for n in ("encoder.layers.0.self_attn.relative_k_proj.weight", "encoder.layers.0.self_attn.bias_u", "encoder.layers.0.self_attn.bias_v",
              "encoder.layers.1.feed_forward1.linear1.bias"):
        assert hip.G[n].abs().max().item() == 0.0, n
        assert free[n].abs().max().item() > 0.0, n
    assert hip.G["encoder.layers.1.self_attn.bias_u"].abs().max().item() > 0.0 and torch.equal(hip.G[SUB + "layers.0.weight"], free[SUB + "layers.0.weight"])
    hip.frozen = set()


def test_input_and_mask_refusals(cuda):
    from dynamic_asr_eval_amd.ops import DynError
    ref, hip = _pair(cuda, arch=dict(R.TOY, num_hidden_layers=1))
    with pytest.raises(DynError) as e:
        hip(input_features=torch.zeros(1, 16, 80, device=cuda), attention_mask=torch.ones(1, 16, device=cuda))
    assert "attention_mask" in str(e.value)
    for bad in (torch.zeros(1, 16, 64, device=cuda), torch.zeros(16, 80, device=cuda), torch.zeros(1, 16, 80)):
        with pytest.raises(DynError):
            hip(input_features=bad)
    assert hip(torch.zeros(1, 1, 80, device=cuda)).logits.shape == (1, 1, R.VOCAB)                 # one feature frame is one encoder frame


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
def test_dynamic_eval_matches_oracle(cuda, shuffle):
    """nvidia_ctc_lib.dynamic_eval against the reference's loop restated on transformers' model (tests/parakeet_refs.py): a [1, 80, 300]
    spectrogram, seq_len 128, overlap 64 (four windows, the last one 108 frames: overlap_ds = int(64 / (108 / 14)) = 8), two augmented copies,
    Adam at 1e-5, once in order and once shuffled under a fixed random.seed.  The project's loop bar: stitched log-probs within 1e-3 with
    equal argmax, identical pseudo-labels at every step, parameters and `frozen` restored bit for bit."""
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.decoding import GreedyCTCDecoder
    L = R.LOOP
    ref, hip = _pair(cuda, seed=L["seed"], blank_bias=L["blank_bias"])
    spec, tok = R.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=shuffle)
    want_labels, got_labels = [], []
    random.seed(17)
    want = R.dynamic_eval_ref(args, ref, spec, L["seq_len"], L["overlap"], tok, L["num_negatives"], L["lr_args"],
                              generator=torch.Generator().manual_seed(L["mask_seed"]), labels_out=want_labels)
    ids = GreedyCTCDecoder.ids

    def recording_ids(self, log_probs):
        out = ids(self, log_probs)
        got_labels.append(list(out))
        return out

    GreedyCTCDecoder.ids = recording_ids
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    try:
        got = N.dynamic_eval(args, hip, spec, L["seq_len"], L["overlap"], tok, use_tqdm=False, num_negatives=L["num_negatives"], lr_args=L["lr_args"],
                             spec_augment_config=R.SPEC_AUGMENT)
    finally:
        GreedyCTCDecoder.ids = ids
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert got_labels == want_labels and len(want_labels) == 4 and all(want_labels)
    assert got.shape == want.shape == (38, R.VOCAB) and np.isfinite(want).all()
    err = np.abs(got - want).max()
    print("stitched log-prob err", err)
    assert err < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))
