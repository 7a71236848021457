"""LasrForCTC (lasr_model.py: the MedASR conformer on the parents' layer code, the Conv1d subsampling on the implicit GEMM, q | k rotary
after the packed projection, weighted residuals, the 32-tap conv module on csrc/convmod_bn.hip) against transformers' LasrForCTC on the CPU
with the same random state dict — logits, every parameter gradient, the bias and residual-weight variants, state-dict round trip,
reproducibility, active subsets, frozen prefixes — nvidia_ctc_lib.dynamic_eval against the test-side oracle of the reference's loop
(tests/lasr_refs.py), and a Parakeet model through the changed loop."""
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

import lasr_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

SUB, HEAD = "encoder.subsampler.", "ctc_head."


def _pair(cuda, arch=R.TOY, seed=0, blank_bias=0.0, **over):
    from dynamic_asr_eval_amd.lasr_model import LasrForCTC
    cfg, ref = R.hf_model(arch, seed, blank_bias, **over)
    hip = LasrForCTC(cfg, device=cuda)
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


ONES = dict(feed_forward_residual_weights=[1.0, 1.0], conv_residual_weights=[1.0, 1.0])


@pytest.mark.parametrize("shape,over", [((3, 77, 128), {}), ((2, 141, 128), {}), ((1, 13, 128), {}), ((3, 77, 128), dict(attention_bias=True)),
                                        ((3, 77, 128), dict(convolution_bias=True)), ((3, 77, 128), ONES)],
                         ids=["17-frames", "33-frames", "1-frame", "attention-bias", "convolution-bias", "unit-residual-weights"])
def test_forward_backward_matches_transformers(cuda, shape, over):
    """77 feature frames give 17 encoder frames (every frame's 32-tap window leaves the sequence on both sides), 141 give 33 (a second time
    tile of the conv-module kernels), 13 give one.  Logits within 2e-4 * max(1, max |logit|), every parameter's gradient within 3e-3 of its
    largest entry + 2e-8: the bars tests/test_parakeet_gpu.py gives this layer stack.
    Measured (MI355X): logits within 2.1e-07 .. 8.9e-07 (max |logit| 0.8 .. 1.0), worst relative gradient error 1.9e-06 .. 3.3e-05."""
    from dynamic_asr_eval_amd.lasr_model import frames
    ref, hip = _pair(cuda, **over)
    for k, v in over.items():
        assert hip.cfg[k] == (tuple(v) if isinstance(v, list) else v)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    assert frames(shape[1]) == {77: 17, 141: 33, 13: 1}[shape[1]]
    grads = _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    assert ("encoder.layers.0.self_attn.q_proj.bias" in grads) == over.get("attention_bias", False)
    assert ("encoder.layers.0.conv.depthwise_conv.bias" in grads) == over.get("convolution_bias", False)
    _state_dict_round_trip(ref, hip)


def test_published_width_forward_and_every_gradient(cuda):
    """MedASR's width (512 hidden, 8 x 64 heads: a second channel block of the conv-module kernels) at one layer.  Measured (MI355X): logits
    within 9.8e-07 (max |logit| 1.7, bar 8.6e-04), worst relative gradient error 3.3e-06."""
    ref, hip = _pair(cuda, arch=R.WIDE)
    g = torch.Generator().manual_seed(11)
    _forward_and_every_gradient(cuda, ref, hip, torch.randn(2, 77, 128, generator=g), g, 5e-4)


def test_backward_is_bit_reproducible(cuda):
    ref, hip = _pair(cuda, seed=1)
    x = torch.randn(2, 141, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert first.abs().max().item() > 0.0


def test_active_subset_backward(cuda):
    """n_active = 2 of 3 equals the full backward with a zero gradient on the third row, to 1e-5 of the largest entry."""
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(3, 77, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out)
    gl[:2] = torch.randn(2, *out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:2].contiguous(), n_active=2)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_frozen_prefixes(cuda, monkeypatch):
    """With `encoder.subsampler.` and `ctc_head.` frozen (the loop's freeze for this family): their gradients are exact zeros, every other
    gradient keeps its bits, and no subsampling backward kernel is launched (their wrappers are made to raise)."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.lasr_model import FROZEN_IN_THE_LOOP
    assert FROZEN_IN_THE_LOOP == (SUB, HEAD)
    ref, hip = _pair(cuda, seed=4)
    x = torch.randn(2, 77, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl)
    free = {n: hip.G[n].clone() for n, _ in hip.spec}
    assert all(free[n].abs().max().item() > 0.0 for n in free if n.startswith((SUB, HEAD)))

    def forbidden(*a, **k):
        raise AssertionError("a subsampling backward kernel was launched although the subsampling is frozen")

    for name in ("conv1d_wgrad", "conv1d_dgrad", "relu_bwd"):
        monkeypatch.setattr(ops, name, forbidden)
    hip.frozen = set(FROZEN_IN_THE_LOOP)
    hip(x); hip.zero_grad(); hip.backward(gl)
    for n, _ in hip.spec:
        if n.startswith((SUB, HEAD)):
            assert hip.G[n].abs().max().item() == 0.0, n
        else:
            assert torch.equal(hip.G[n], free[n]), n
    monkeypatch.undo()
    hip.frozen = {"encoder.layers.0.norm_out", "encoder.layers.1.feed_forward1.linear1.weight", "encoder.out_norm"}
    hip(x); hip.zero_grad(); hip.backward(gl)
    for n in ("encoder.layers.0.norm_out.weight", "encoder.layers.1.feed_forward1.linear1.weight", "encoder.out_norm.weight"):
        assert hip.G[n].abs().max().item() == 0.0 and free[n].abs().max().item() > 0.0, n
    assert torch.equal(hip.G[SUB + "conv_0.weight"], free[SUB + "conv_0.weight"])
    hip.frozen = set()


def test_input_and_mask_refusals(cuda):
    from dynamic_asr_eval_amd.ops import DynError
    ref, hip = _pair(cuda, arch=dict(R.TOY, num_hidden_layers=1))
    with pytest.raises(DynError) as e:
        hip(input_features=torch.zeros(1, 16, 128, device=cuda), attention_mask=torch.ones(1, 16, device=cuda))
    assert "attention_mask" in str(e.value)
    with pytest.raises(DynError) as e:
        hip(input_features=torch.zeros(1, 12, 128, device=cuda))
    assert "13" in str(e.value)
    for bad in (torch.zeros(1, 16, 80, device=cuda), torch.zeros(16, 128, device=cuda), torch.zeros(1, 16, 128)):
        with pytest.raises(DynError):
            hip(input_features=bad)


def _recorded_labels():
    from dynamic_asr_eval_amd.decoding import GreedyCTCDecoder
    ids, got = GreedyCTCDecoder.ids, []

    def recording_ids(self, log_probs):
        out = ids(self, log_probs)
        got.append(list(out))
        return out

    return GreedyCTCDecoder, ids, recording_ids, got


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
def test_dynamic_eval_matches_oracle(cuda, shuffle):
    """nvidia_ctc_lib.dynamic_eval against the reference's loop restated on transformers' model (tests/lasr_refs.py): a [1, 128, 300]
    feature matrix, seq_len 128, overlap 64 (four windows of 128, 128, 128, 108 frames -> 29, 29, 29, 24 encoder frames; u_len / ds_len is
    4.41 and 4.5, no integer: overlap_ds = int(64 / ratio) = 14), two augmented copies, Adam at 1e-5, once in order and once shuffled under a
    fixed random.seed.  The Parakeet loop test's bars: stitched log-probs within 1e-3 with equal argmax, identical pseudo-labels at every
    step, parameters and `frozen` restored bit for bit.  Conditions on the inputs, asserted on the oracle's own output: its smallest top-2
    log-prob margin over all stitched frames is >= 1e-2 (ten times the bar: no argmax can flip by rounding) and at least a quarter of the
    frames are non-blank.  Measured (MI355X): stitched log-probs within 9.5e-07; the oracle's margin 0.026 in order, 0.031 shuffled, every
    frame non-blank."""
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    L = R.LOOP
    ref, hip = _pair(cuda, seed=L["seed"], blank_bias=L["blank_bias"])
    spec, tok = R.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=shuffle)
    want_labels = []
    random.seed(17)
    want = R.dynamic_eval_ref(args, ref, spec, L["seq_len"], L["overlap"], tok, L["num_negatives"], L["lr_args"],
                              generator=torch.Generator().manual_seed(L["mask_seed"]), labels_out=want_labels)
    top2 = np.sort(want, -1)[:, -2:]
    margin, nonblank = (top2[:, 1] - top2[:, 0]).min(), (want.argmax(-1) != R.PAD).mean()
    print(f"oracle: smallest top-2 margin {margin:.4f}, non-blank frames {nonblank:.2f}")
    assert margin >= 1e-2 and nonblank >= 0.25
    D, ids, recording_ids, got_labels = _recorded_labels()
    D.ids = recording_ids
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    try:
        got = N.dynamic_eval(args, hip, spec, L["seq_len"], L["overlap"], tok, use_tqdm=False, num_negatives=L["num_negatives"], lr_args=L["lr_args"],
                             spec_augment_config=R.SPEC_AUGMENT)
    finally:
        D.ids = ids
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert got_labels == want_labels and len(want_labels) == 4 and all(want_labels)
    assert got.shape == want.shape == (R.LOOP_ROWS, R.VOCAB) and np.isfinite(want).all()
    err = np.abs(got - want).max()
    print("stitched log-prob err", err)
    assert err < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))


def test_parakeet_through_the_changed_loop_keeps_its_bits(cuda):
    """A Parakeet model through nvidia_ctc_lib.dynamic_eval: reading `downsampling_factor` / `frozen_in_the_loop` from the model gives the
    bits that passing the loop's former constants (8, parakeet_model.FROZEN_IN_THE_LOOP) gives."""
    import parakeet_refs as PR
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.parakeet_model import FROZEN_IN_THE_LOOP, ParakeetForCTC
    L = PR.LOOP
    cfg, ref = PR.hf_model(seed=L["seed"], blank_bias=L["blank_bias"])
    hip = ParakeetForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    assert N.loop_constants(hip) == (8, FROZEN_IN_THE_LOOP) == (8, ("encoder.subsampling.", "ctc_head."))
    spec, tok = PR.loop_inputs()
    runs = []
    for kw in ({}, dict(downsampling_factor=8, frozen_prefixes=FROZEN_IN_THE_LOOP)):
        args = argparse.Namespace(epochs=1, shuffle=False, spec_augment_generator=torch.Generator().manual_seed(L["mask_seed"]))
        runs.append(N.dynamic_eval(args, hip, spec, L["seq_len"], L["overlap"], tok, use_tqdm=False, num_negatives=L["num_negatives"],
                                   lr_args=L["lr_args"], spec_augment_config=PR.SPEC_AUGMENT))
    assert runs[0].shape == (38, PR.VOCAB) and np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))
    with pytest.raises(AssertionError):                                            # the factor is what the overlap is checked against
        N.dynamic_eval(argparse.Namespace(epochs=1, shuffle=False), hip, spec, L["seq_len"], 60, tok, use_tqdm=False, num_negatives=1)
