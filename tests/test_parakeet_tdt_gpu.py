"""ParakeetForTDT (parakeet_tdt_model.py) against transformers' ParakeetForTDT on the CPU with the same random state dict — joint logits, the
TDT loss, every parameter's gradient, reproducibility, a frozen prediction network, the state-dict round trip — its greedy decode against
transformers' generate, and parakeet_tdt_lib.dynamic_eval_tdt_loss against the test-side oracle (tests/transducer_refs.py)."""
import argparse
import copy
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import transducer_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _pair(cuda, ref_cfg=None, **kw):
    from dynamic_asr_eval_amd.parakeet_tdt_model import ParakeetForTDT
    cfg, ref = R.hf_tdt_model(**kw) if ref_cfg is None else ref_cfg
    hip = ParakeetForTDT(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _labels(B, U, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(3, vocab - 1, (B, U), generator=g)                       # neither the pad id (2) nor the blank
    return lab, torch.cat([torch.full((B, 1), vocab - 1), lab], 1)


@pytest.mark.parametrize("kw,shape,U", [(dict(hidden=64, layers=2, vocab=33), (3, 67, 80), 4), (dict(hidden=640, layers=1, vocab=1030), (2, 67, 80), 3)],
                         ids=["64x2-vocab33", "640x1-vocab1030"])
def test_logits_loss_and_every_gradient_match_transformers(cuda, kw, shape, U):
    """The toy encoder with a 64-wide, 2-layer prediction network at vocab 33 and a 640-wide, 1-layer one at vocab 1030.  Joint logits
    within 2e-4 * max(1, max |logit|), the loss (reduction "mean", sigma 0.05) within 2e-4 relative, every parameter's gradient within
    3e-3 of its largest entry + 2e-8: the bars of tests/test_parakeet_gpu.py.  Then the state dict round-trips and a second backward
    gives equal bits.  Measured (MI355X): 64 x 2, vocab 33: logits within 7.5e-08 (max |logit| 0.42), loss equal as printed, worst relative
    gradient error 1.8e-06; 640 x 1, vocab 1030: 2.5e-07 (0.52), 5.4e-04."""
    ref, hip = _pair(cuda, seed=2, **kw)
    V1 = kw["vocab"]
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    lab, dec_in = _labels(shape[0], U, V1, 5)
    from transformers.loss.loss_tdt import tdt_loss
    out_ref = ref(input_features=x, decoder_input_ids=dec_in).logits
    Tp = out_ref.shape[1]
    loss_ref = tdt_loss(out_ref[..., :V1], out_ref[..., V1:], lab, torch.full((shape[0],), Tp), torch.full((shape[0],), U), V1 - 1, list(R.DURATIONS),
                        0.05, "mean")
    with torch.enable_grad():
        out = hip(input_features=x.to(cuda), decoder_input_ids=dec_in, labels=lab, sigma=0.05)
    assert out.logits.shape == out_ref.shape and out.frames == Tp
    err, top = (out.logits.cpu() - out_ref).abs().max().item(), out_ref.abs().max().item()
    lerr = abs(out.loss.item() - loss_ref.item()) / abs(loss_ref.item())
    print(f"logits err {err:.3e}, max |logit| {top:.3e}; loss {loss_ref.item():.6f}, relative err {lerr:.3e}")
    assert err < 2e-4 * max(1.0, top) and lerr < 2e-4
    ref.zero_grad()
    loss_ref.backward()
    hip.zero_grad(); hip.backward()
    first = hip.flat_grads.clone()
    grads, named = hip.grads_hf(), dict(ref.named_parameters())
    assert set(grads) == set(named)
    worst = 0.0
    for n, p in named.items():
        assert p.grad is not None and grads[n].shape == p.grad.shape, n
        diff, scale = (grads[n].cpu() - p.grad).abs().max().item(), p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
        assert scale > 0.0, n
    print("worst relative gradient error", worst)
    with torch.enable_grad():
        hip(input_features=x.to(cuda), decoder_input_ids=dec_in, labels=lab, sigma=0.05)
    hip.zero_grad(); hip.backward()
    assert torch.equal(hip.flat_grads, first)                                    # bit-reproducible
    sd, want = hip.state_dict(), ref.state_dict()
    assert set(sd) == set(want)
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n
    before = hip.flat_params.clone()
    hip.load_state_dict(sd)
    assert torch.equal(hip.flat_params, before)


def test_shared_decoder_rows_active_subset_and_frozen_decoder(cuda, monkeypatch):
    """decoder_input_ids [1, U + 1] shared by the rows equals the same ids repeated per row (logits bit for bit, gradients to 1e-5 of the
    largest entry: dp sums over the batch in another order); n_active = 2 of 3 leaves the third row out of the loss; with `decoder.`
    frozen the LSTM backward is not run at all (its wrapper is made to raise), those gradients are exact zeros and every other
    gradient keeps its bits."""
    from dynamic_asr_eval_amd import ops
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(3, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    lab, dec_in = _labels(1, 4, R.TDT_VOCAB, 7)
    with torch.enable_grad():
        a = hip(input_features=x, decoder_input_ids=dec_in, labels=lab, reduction="sum", n_active=2)
    assert a.logits.shape[0] == 2
    hip.zero_grad(); hip.backward(); shared = hip.flat_grads.clone()
    with torch.enable_grad():
        b = hip(input_features=x, decoder_input_ids=dec_in.expand(2, -1).contiguous(), labels=lab.expand(2, -1).contiguous(), reduction="sum", n_active=2)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss)
    hip.zero_grad(); hip.backward()
    assert (hip.flat_grads - shared).abs().max().item() <= 1e-5 * shared.abs().max().item()
    free = {n: hip.G[n].clone() for n, _ in hip.spec}
    assert all(free[n].abs().max().item() > 0.0 for n in free if n.startswith("decoder."))

    def forbidden(*args, **kw):
        raise AssertionError("the LSTM backward was launched although the prediction network is frozen")

    monkeypatch.setattr(ops, "lstm_cell_bwd", forbidden)
    hip.frozen = {"decoder."}
    with torch.enable_grad():
        hip(input_features=x, decoder_input_ids=dec_in.expand(2, -1).contiguous(), labels=lab.expand(2, -1).contiguous(), reduction="sum", n_active=2)
    hip.zero_grad(); hip.backward()
    for n, _ in hip.spec:
        if n.startswith("decoder."):
            assert hip.G[n].abs().max().item() == 0.0, n
        else:
            assert torch.equal(hip.G[n], free[n]), n
    hip.frozen = set()


@pytest.mark.parametrize("B", [1, 3])
def test_generate_matches_transformers(cuda, B):
    """generate() against transformers' generate on the decode case of tests/transducer_refs.py (its conditions are asserted on the oracle
    alone, here and in tests/test_parakeet_tdt_cpu.py): the non-blank tokens, their frames (the cumulative sums of transformers'
    durations) and the number of steps per row are equal."""
    ref_cfg = R.decode_model()
    rows, Tp, (mt, md) = R.decode_case(B, ref_cfg[1])
    R.assert_decode_conditions(rows, mt, md)
    ref, hip = _pair(cuda, ref_cfg=ref_cfg)
    out = hip.generate(R.decode_feats(B).to(cuda))
    for b, row in enumerate(rows):
        n = int(out.count[b])
        assert out.tokens[b, :n].tolist() == row["tokens"] and out.frames[b, :n].tolist() == row["frames"], b
        assert int(out.steps[b]) == len(row["steps"]), b


@pytest.mark.parametrize("overlap,shuffle,brn", [(0, False, False), (64, False, False), (64, True, False), (64, False, True)],
                         ids=["overlap0", "overlap64", "overlap64-shuffled", "overlap64-batch-renorm"])
def test_dynamic_eval_matches_oracle(cuda, overlap, shuffle, brn):
    """parakeet_tdt_lib.dynamic_eval_tdt_loss against the loop restated on transformers' model (tests/transducer_refs.py): a [1, 80, 300]
    spectrogram, windows of 128 frames, overlap 0 and 64, in order and shuffled, two augmented copies, Adam at 1e-5: tokens and frames
    equal, the adapted joint logits of a probe after the last step within 1e-3, parameters and `frozen` restored bit for bit.  Once with
    batch_renorm: the oracle then carries the reference's swap (batch_renorm_refs.swap_in: a training-mode BatchRenorm1d in every conv
    module), tokens and frames equal.  The smallest top-2 margin over every argmax the oracle takes is asserted to be at least 1e-2.
    Measured (MI355X): adapted joint logits within 6.1e-05 (max |logit| 607)."""
    from dynamic_asr_eval_amd import parakeet_tdt_lib as N
    L = R.LOOP
    ref, hip = _pair(cuda, ref_cfg=R.decode_model())
    spec, tok = R.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=shuffle)
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    probe_x = torch.randn(1, 67, 80, generator=torch.Generator().manual_seed(9))
    probe_ids = torch.tensor([[R.TDT_BLANK, 5, 9]])
    got_logits = {}
    random.seed(17)
    info = {"probe": (probe_x, probe_ids)}
    want_ids, want_frames = R.dynamic_eval_tdt_ref(args, copy.deepcopy(ref) if brn else ref, spec, L["seq_len"], overlap, tok, L["num_negatives"], L["lr_args"],
                                                   generator=torch.Generator().manual_seed(L["mask_seed"]), logits_out=info, batch_renorm=brn)
    assert info["margin"] >= 1e-2, info["margin"]
    assert len(want_ids) > 0 and any(k != R.TDT_BLANK for k, _ in info["steps"]) and any(k == R.TDT_BLANK for k, _ in info["steps"])
    step = N.Adam.step
    if not brn:      # the adapted logits, taken before the loop restores the weights (under batch renorm a probe would move the running statistics)
        def probing_step(self, *a, **k):
            r = step(self, *a, **k)
            with torch.no_grad():
                got_logits["logits"] = hip(input_features=probe_x.to(cuda), decoder_input_ids=probe_ids).logits.cpu()
            return r

        N.Adam.step = probing_step
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    try:
        ids, frames, text = N.dynamic_eval_tdt_loss(args, hip, spec, L["seq_len"], overlap, tok, use_tqdm=False, num_negatives=L["num_negatives"],
                                                    lr_args=L["lr_args"], spec_augment_config=R.PR.SPEC_AUGMENT, batch_renorm=brn)
    finally:
        N.Adam.step = step
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert text == tok.ids_to_text(ids) and len(ids) == len(frames)
    assert frames == sorted(frames) and all(0 <= f < 38 for f in frames)
    assert ids == want_ids and frames == want_frames
    if brn:
        return
    err = (got_logits["logits"] - info["logits"]).abs().max().item()
    top = info["logits"].abs().max().item()
    print(f"adapted joint logits err {err:.3e} (max |logit| {top:.3e})")
    assert err < 1e-3
