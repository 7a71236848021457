"""ParakeetForCTC / LasrForCTC under batch_renorm_training() and nvidia_ctc_lib.dynamic_eval(batch_renorm=True) against transformers' models
on the CPU with the swap reference nvidia_ctc/lib.py:74,89-102 performs (tests/batch_renorm_refs.py): a BatchRenorm1d in training mode in
every conv module.  Running statistics are calibrated so that every clamp is at work (batch_renorm_refs.calibrate)."""
import argparse
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import batch_renorm_refs as BR  # noqa: E402
import kernel_refs as K  # noqa: E402
import lasr_refs as LR  # noqa: E402
import parakeet_refs as PR  # noqa: E402

pytestmark = pytest.mark.gpu

CBIAS = "conv.depthwise_conv.bias"


def _pair(cuda, family, x, seed=0):
    """(ref, hip, share): transformers' model (eval mode, not yet swapped) with calibrated batch-norm buffers and this package's model with
    the same state dict."""
    if family == "parakeet":
        from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC as Model
        R = PR
    else:
        from dynamic_asr_eval_amd.lasr_model import LasrForCTC as Model
        R = LR
    cfg, ref = R.hf_model(R.TOY, seed)
    share = BR.calibrate(ref, x)
    hip = Model(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip, share


def _x(family, T, seed=1):
    n_mels = (PR if family == "parakeet" else LR).TOY["num_mel_bins"]
    return torch.randn(3, T, n_mels, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("family", ["parakeet", "lasr"])
def test_forward_backward_matches_transformers(cuda, family):
    """One forward + backward of a [3, 131, F] batch (17 encoder frames at 9 taps, 30 at 32: 51 / 90 rows in the batch statistic) against
    transformers on the CPU with the swapped-in module.  tests/test_parakeet_gpu.py's bars: logits within 2e-4 x max(1, max |logit|), every
    trainable parameter's gradient within 3e-3 of its largest entry + 2e-8.  The conv bias' gradient is exactly zero here; the fp32 oracle's
    is rounding noise (9.5e-7 / 7.5e-8 against 7.8e-16 / 1.1e-16 in float64) and is the only quantity whose fp32 oracle is further than a
    quarter of its bar from the float64 run, so it is compared with nothing but zero.  The share of (layer, channel) pairs with an active
    clamp is 0.828 on the oracle.
    Measured (MI355X): Parakeet logits within 8.2e-06 (max |logit| 0.96), worst relative gradient error 7.9e-04, 0.54 from the eval-mode logits;
    LASR 1.2e-06 (0.91), 7.8e-06, 0.52."""
    x = _x(family, 131)
    ref, hip, share = _pair(cuda, family, x)
    assert 0.25 <= share <= 0.9, share
    oracle = BR.swap_in(copy.deepcopy(ref))
    out_ref = oracle(input_features=x).logits
    g = torch.Generator().manual_seed(2)
    gl = torch.randn(out_ref.shape, generator=g) / out_ref.numel()
    out_ref.backward(gl)
    with torch.no_grad():
        eval_out = ref(input_features=x).logits
    with hip.batch_renorm_training() as state:
        res = hip(input_features=x.to(cuda))
        hip.zero_grad(); hip.backward(gl.to(cuda))
        assert state.num_batches_tracked == [1000001] * hip.cfg["num_hidden_layers"]
    out = res.logits.cpu()
    err, top = (out - out_ref).abs().max().item(), out_ref.abs().max().item()
    live = (out_ref - eval_out).abs().max().item()
    print(f"{family}: share {share:.3f}, forward err {err:.3e}, max |logit| {top:.3e}, bar {2e-4 * max(1.0, top):.3e}; against the eval-mode logits {live:.3e}")
    assert err < 2e-4 * max(1.0, top), (err, top)
    assert live > 10 * 2e-4 * max(1.0, top)                     # the mode is live: far from the eval-mode model
    grads = hip.grads_hf()
    named = dict(oracle.named_parameters())
    assert set(grads) == set(named)
    worst, n_cb = 0.0, 0
    for n, p in named.items():
        assert p.grad is not None and grads[n].shape == p.grad.shape, n
        if n.endswith(CBIAS):
            n_cb += 1
            assert grads[n].abs().max().item() == 0.0, n
            continue
        diff = (grads[n].cpu() - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
        assert scale > 0.0, n
    assert n_cb == (hip.cfg["num_hidden_layers"] if hip.cfg["convolution_bias"] else 0)
    print(f"{family}: worst relative gradient error {worst:.3e}")


@pytest.mark.parametrize("momentum", [0.001, 0.1])
def test_state_after_three_forwards(cuda, momentum):
    """Three forwards (the second without grad mode) advance the loop-local state as the oracle's modules advance: running_mean / running_std
    within kernel_refs.measured_tol of the float64 oracle (4 x the fp32 oracle's own error + 2e-6), num_batches_tracked equal.
    Measured (MI355X) kernel | fp32 oracle | bound, worst of the two layers: momentum 0.001 running_mean 3.2e-08 | 3.2e-08 | 2.1e-06 (moved by 8e-04),
    running_std 4.5e-09 | 4.5e-09 | 2.0e-06; momentum 0.1 running_mean 2.4e-08 | 2.7e-08 | 2.1e-06 (moved by 7e-02), running_std 7.6e-09 | 7.3e-09."""
    xs = [_x("parakeet", 131, seed) for seed in (1, 2, 3)]
    ref, hip, _ = _pair(cuda, "parakeet", xs[0])
    o32, o64 = (BR.swap_in(copy.deepcopy(ref).to(dt), momentum=momentum) for dt in (torch.float32, torch.float64))
    with torch.no_grad():
        for x in xs:
            o32(input_features=x); o64(input_features=x.double())
    with hip.batch_renorm_training(momentum=momentum) as state:
        assert state.momentum == momentum and state.eps == 1e-5
        for k, x in enumerate(xs):
            with (torch.no_grad() if k == 1 else torch.enable_grad()):
                hip(input_features=x.to(cuda))
        for l, (m32, m64) in enumerate(zip(o32.encoder.layers, o64.encoder.layers)):
            assert state.num_batches_tracked[l] == m32.conv.norm.num_batches_tracked.item() == 1000003
            for name in ("running_mean", "running_std"):
                want, t32 = getattr(m64.conv.norm, name), getattr(m32.conv.norm, name)
                tol, e32 = K.measured_tol(t32, want, 2e-6)
                err = K.max_err(getattr(state, name)[l], want)
                moved = K.max_err(want, (ref.encoder.layers[l].conv.norm.running_var.sqrt() if name == "running_std" else
                                         ref.encoder.layers[l].conv.norm.running_mean))
                print(f"  momentum {momentum} layer {l} {name}: kernel {err:.2e} | fp32 oracle {e32:.2e} | bound {tol:.2e} | moved by {moved:.2e}")
                assert err <= tol, (name, l, err, tol)
                assert moved > 10 * tol or momentum < 0.01


def test_context_refusals_and_restoration(cuda):
    """backward(n_active = B - 1) raises inside the context, naming the reason; a nested context is refused; leaving the context restores the
    eval-mode outputs and gradients bit for bit; the model's buffers never change."""
    from dynamic_asr_eval_amd.ops import DynError
    x = _x("parakeet", 67)
    ref, hip, _ = _pair(cuda, "parakeet", x)
    xd = x.to(cuda)
    buffers = {n: b.clone() for n, b in hip.buffers_.items()}
    before = hip(xd).logits.clone()
    gl = (torch.randn(before.shape, generator=torch.Generator().manual_seed(3)) / before.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl[:2].contiguous(), n_active=2)
    grads_before = hip.flat_grads.clone()
    with hip.batch_renorm_training() as state:
        inside = hip(xd).logits.clone()
        with pytest.raises(DynError) as e:
            hip.backward(gl[:2].contiguous(), n_active=2)
        assert "every row" in str(e.value) and "n_active" in str(e.value)
        with pytest.raises(DynError):
            with hip.batch_renorm_training():
                pass
        hip.zero_grad(); hip.backward(gl, n_active=3)                        # all rows: allowed
        assert len(state.running_mean) == len(state.running_std) == hip.cfg["num_hidden_layers"]
        assert not torch.equal(state.running_mean[0], buffers["encoder.layers.0.conv.norm.running_mean"])
    assert hip._brn is None
    assert (inside - before).abs().max().item() > 1e-3
    after = hip(xd).logits
    assert torch.equal(after, before)
    hip.zero_grad(); hip.backward(gl[:2].contiguous(), n_active=2)            # the eval-mode path takes an active subset as before
    assert torch.equal(hip.flat_grads, grads_before)
    for n, b in buffers.items():
        assert torch.equal(hip.buffers_[n], b), n


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
def test_dynamic_eval_matches_oracle(cuda, shuffle):
    """nvidia_ctc_lib.dynamic_eval(batch_renorm=True) against the loop oracle (batch_renorm_refs.dynamic_eval_ref: parakeet_refs' statements
    with the reference's swap in place of model.eval()) at parakeet_refs.LOOP's constants and model seed 5 (batch_renorm_refs.LOOP_SEED: the
    first from 3 upwards at which the oracle's fp32 and float64 runs agree on every label).  The oracle runs in FLOAT64: in fp32 its conv-bias
    gradient is rounding noise that Adam turns into steps of lr (LOOP_SEED's comment; 1.7e-2 / 7.1e-3 from its own float64 run).  Stitched
    log-probs within 1e-3, equal argmax, equal pseudo-labels at every step, parameters and `frozen` bit-restored, buffers untouched; the result
    differs from batch_renorm=False by more than the bar; False and the keyword omitted give equal bits.
    Measured (MI355X): stitched log-probs within 1.7e-05 in order, 1.6e-05 shuffled; 0.52 / 0.55 from batch_renorm=False; share 0.828."""
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.decoding import GreedyCTCDecoder
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    L = PR.LOOP
    cfg, ref, share = BR.loop_pair()
    assert 0.25 <= share <= 0.9, share
    hip = ParakeetForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    spec, tok = PR.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=shuffle)
    want_labels, got_labels = [], []
    random.seed(17)
    want = BR.dynamic_eval_ref(args, copy.deepcopy(ref).double(), spec.double(), L["seq_len"], L["overlap"], tok, L["num_negatives"], L["lr_args"],
                               generator=torch.Generator().manual_seed(L["mask_seed"]), labels_out=want_labels)
    ids = GreedyCTCDecoder.ids

    def recording_ids(self, log_probs):
        out = ids(self, log_probs)
        got_labels.append(list(out))
        return out

    def run(**kw):
        args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
        random.seed(17)
        return N.dynamic_eval(args, hip, spec, L["seq_len"], L["overlap"], tok, use_tqdm=False, num_negatives=L["num_negatives"], lr_args=L["lr_args"],
                              spec_augment_config=PR.SPEC_AUGMENT, **kw)

    before, frozen_before = hip.flat_params.clone(), hip.frozen
    buffers = {n: b.clone() for n, b in hip.buffers_.items()}
    GreedyCTCDecoder.ids = recording_ids
    try:
        got = run(batch_renorm=True)
    finally:
        GreedyCTCDecoder.ids = ids
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set() and hip._brn is None
    for n, b in buffers.items():
        assert torch.equal(hip.buffers_[n], b), n
    assert got_labels == want_labels and len(want_labels) == 4 and all(want_labels)
    assert got.shape == want.shape == (38, PR.VOCAB) and np.isfinite(want).all()
    err = np.abs(got - want).max()
    print("share", share, "stitched log-prob err", err)
    assert err < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))
    off = run(batch_renorm=False)
    omitted = run()
    assert np.array_equal(off.view(np.int32), omitted.view(np.int32))
    args.batch_renorm = True                                     # the args route: the keyword's None reads args.batch_renorm
    by_args = run()
    del args.batch_renorm
    assert np.array_equal(by_args.view(np.int32), got.view(np.int32))
    live = np.abs(got - off).max()
    print("against batch_renorm=False", live)
    assert live > 1e-3
