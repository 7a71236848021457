"""ParakeetForRNNT (parakeet_rnnt_model.py) against transformers' ParakeetForRNNT on the CPU with the same random state dict: encode, joint
logits, the RNN-T loss and every parameter's gradient (the oracle of the loss is transformers' logits through the torch recursion of
tests/rnnt_refs.py and autograd: transformers' own rnnt_loss needs torchaudio), the joint streamed over frame chunks, the greedy decode
against transformers' generate, parakeet_tdt_lib.dynamic_eval_transducer_loss against the test-side oracle, and a ParakeetForTDT built in
the same process afterwards."""
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

import kernel_refs as K  # noqa: E402
import rnnt_refs as R  # noqa: E402
import transducer_refs as TR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, U = (3, 67, 80), 4
_ORACLE = {}


def _pair(cuda, ref_cfg=None, **kw):
    from dynamic_asr_eval_amd.parakeet_rnnt_model import ParakeetForRNNT
    cfg, ref = R.hf_rnnt_model(**kw) if ref_cfg is None else ref_cfg
    hip = ParakeetForRNNT(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _labels(B, U, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(3, vocab - 1, (B, U), generator=g)                       # neither the pad id (2) nor the blank
    return lab, torch.cat([torch.full((B, 1), vocab - 1), lab], 1)


def _oracle(reduction):
    """transformers' model, the torch-recursion loss on its logits and every parameter's gradient: computed once on the CPU per reduction,
    shared by the whole and the chunked tests, left alone.  The last label of row 1 is the blank id: transformers counts
    `labels != blank_token_id`, so that row has U - 1 labels."""
    if reduction not in _ORACLE:
        cfg, ref = R.hf_rnnt_model(seed=2)
        x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(1))
        lab, dec_in = _labels(SHAPE[0], U, R.RNNT_VOCAB, 5)
        lab[1, -1] = dec_in[1, -1] = R.RNNT_BLANK
        out = ref(input_features=x, decoder_input_ids=dec_in)
        Tp = out.logits.shape[1]
        U_b = (lab != R.RNNT_BLANK).sum(-1).tolist()
        assert U_b == [U, U - 1, U]
        scale = 0.25 if reduction == "sum" else 1.0
        loss = R.rnnt_loss_torch(out.logits, lab.tolist(), [Tp] * SHAPE[0], U_b, R.RNNT_BLANK, reduction)
        ref.zero_grad()
        (loss * scale).backward()
        _ORACLE[reduction] = dict(cfg=(cfg, ref), x=x, lab=lab, dec_in=dec_in, Tp=Tp, loss=loss.item(), scale=scale, logits=out.logits.detach(),
                                  enc=out.pooler_output.detach(), grads={n: p.grad.clone() for n, p in ref.named_parameters()})
    return _ORACLE[reduction]


def _grads(hip, **kw):
    """One grad-mode forward, zero_grad() BETWEEN forward and backward, backward -> (output, a copy of flat_grads)."""
    with torch.enable_grad():
        out = hip(**kw)
    hip.zero_grad(); hip.backward()
    return out, hip.flat_grads.clone()


def _kw(o, cuda, reduction):
    kw = dict(input_features=o["x"].to(cuda), decoder_input_ids=o["dec_in"], labels=o["lab"])
    if reduction == "sum":
        kw.update(reduction="sum", grad_scale=o["scale"])
    return kw                                                                    # "mean_volume" is the default: not passed


def _assert_grads(hip, o):
    grads = hip.grads_hf()
    assert set(grads) == set(o["grads"])
    worst = 0.0
    for n, want in o["grads"].items():
        assert grads[n].shape == want.shape, n
        diff, scale = (grads[n].cpu() - want).abs().max().item(), want.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
        assert scale > 0.0, n
    return worst


@pytest.mark.parametrize("reduction", ["mean_volume", "sum"])
def test_encode_logits_loss_and_every_gradient_match_transformers(cuda, reduction):
    """The toy encoder with a 64-wide, 2-layer prediction network at vocab 33, B = 3, T' = 9, U = 4 (one row with a blank-padded label:
    its length is counted as transformers does, `labels != blank_token_id`).  The projected encoder states and the joint logits
    [B, T', U + 1, V1] within 2e-4 * max(1, max |value|), the loss within 2e-4 relative, every parameter's gradient within 3e-3 of its
    largest entry + 2e-8: the bars of tests/test_parakeet_tdt_gpu.py.  Reduction "sum" with grad_scale 0.25 (what the loop uses) and the
    default, "mean_volume".  Then a one-row decoder_input_ids shared by the batch gives the logits of the repeated rows, a second
    backward gives equal bits and the state dict round-trips.
    Measured (MI355X): enc within 5.2e-07 (max 0.92), logits within 4.5e-08 (max |logit| 0.19), both losses equal as printed, worst
    relative gradient error 1.3e-04 (mean_volume) and 1.6e-04 (sum)."""
    o = _oracle(reduction)
    ref, hip = _pair(cuda, ref_cfg=o["cfg"])
    out, first = _grads(hip, **_kw(o, cuda, reduction))
    assert out.logits.shape == o["logits"].shape == (3, 9, U + 1, R.RNNT_VOCAB) and out.frames == o["Tp"] == 9
    eerr, etop = (out.enc.cpu() - o["enc"]).abs().max().item(), o["enc"].abs().max().item()
    err, top = (out.logits.cpu() - o["logits"]).abs().max().item(), o["logits"].abs().max().item()
    lerr = abs(out.loss.item() - o["loss"]) / abs(o["loss"])
    print(f"enc err {eerr:.3e} (max {etop:.3e}); logits err {err:.3e}, max |logit| {top:.3e}; loss {o['loss']:.6f}, relative err {lerr:.3e}")
    assert eerr < 2e-4 * max(1.0, etop) and err < 2e-4 * max(1.0, top) and lerr < 2e-4
    print("worst relative gradient error", _assert_grads(hip, o))
    _, second = _grads(hip, **_kw(o, cuda, reduction))
    assert torch.equal(second, first)                                            # bit-reproducible
    with torch.no_grad():
        one = hip(input_features=o["x"].to(cuda), decoder_input_ids=o["dec_in"][:1])
        rep = hip(input_features=o["x"].to(cuda), decoder_input_ids=o["dec_in"][:1].expand(3, -1).contiguous())
    assert torch.equal(one.logits, rep.logits) and torch.equal(one.logits[0], out.logits[0])
    sd, want = hip.state_dict(), ref.state_dict()
    assert set(sd) == set(want)
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n


def test_frozen_decoder_and_frozen_encoder_skip_their_backward(cuda, monkeypatch):
    """With `decoder.` frozen the LSTM backward is not run at all (its wrapper is made to raise), with the encoder and its projector
    frozen the attention backward is not; the frozen gradients are exact zeros and every other gradient keeps its bits."""
    from dynamic_asr_eval_amd import ops
    o = _oracle("sum")
    ref, hip = _pair(cuda, ref_cfg=o["cfg"])
    kw = _kw(o, cuda, "sum")
    _grads(hip, **kw)
    free = {n: hip.G[n].clone() for n, _ in hip.spec}

    def forbidden(*args, **kw):
        raise AssertionError("a backward of a frozen part was launched")

    with monkeypatch.context() as m:
        m.setattr(ops, "lstm_cell_bwd", forbidden)
        hip.frozen = {"decoder."}
        _grads(hip, **kw)
    for n, _ in hip.spec:
        assert (hip.G[n].abs().max().item() == 0.0) if n.startswith("decoder.") else torch.equal(hip.G[n], free[n]), n
    with monkeypatch.context() as m:
        m.setattr(hip, "_layers_bwd", forbidden)
        hip.frozen = {"encoder.", "encoder_projector."}
        _grads(hip, **kw)
    for n, _ in hip.spec:
        assert (hip.G[n].abs().max().item() == 0.0) if n.startswith(("encoder.", "encoder_projector.")) else torch.equal(hip.G[n], free[n]), n
    hip.frozen = set()


@pytest.mark.parametrize("Tc", [1, 4])
def test_chunked_head_is_bit_equal_in_loss_and_within_the_wgrad_rule_in_gradients(cuda, Tc):
    """frames_per_chunk 1 and 4 at T' = 9 (9 chunks; 4, 4 and 1 frames): `logits` is None, loss and nll are bit-equal to the unchunked
    call, every parameter's gradient meets the bars of the whole-joint test against the same CPU oracle and lies within
    kernel_refs.wgrad_tol(5e-4, B T' (U + 1) rows, 531) of the unchunked gradient (sums over frames in another order), and an explicit
    grad_logits is refused by name.
    Measured (MI355X): chunked against unchunked gradients within 3.6e-07 (Tc 1) and 4.8e-07 (Tc 4), largest entry 2.5 | bound 5.0e-04."""
    from dynamic_asr_eval_amd import ops
    o = _oracle("mean_volume")
    ref, hip = _pair(cuda, ref_cfg=o["cfg"])
    kw = _kw(o, cuda, "mean_volume")
    whole_out, whole = _grads(hip, **kw)
    out, chunked = _grads(hip, frames_per_chunk=Tc, **kw)
    assert out.logits is None and whole_out.logits is not None and out.frames == 9
    assert torch.equal(out.loss, whole_out.loss) and torch.equal(out.nll, whole_out.nll)
    _assert_grads(hip, o)
    tol = K.wgrad_tol(5e-4, SHAPE[0] * 9 * (U + 1), 531)
    diff = (chunked - whole).abs().max().item()
    print(f"Tc={Tc}: chunked vs unchunked gradients {diff:.3e} (largest entry {whole.abs().max().item():.3e}) | bound {tol:.1e}")
    assert diff <= tol and whole.abs().max().item() > 0
    with torch.enable_grad():
        hip(frames_per_chunk=Tc, **kw)
    with pytest.raises(ops.DynError) as e:
        hip.backward(torch.zeros(3, 9, U + 1, R.RNNT_VOCAB, device=cuda))
    assert "grad_logits" in str(e.value) and "chunked forward" in str(e.value)
    hip.joint_budget = 1                                                         # the attribute alone: one frame per chunk
    with torch.no_grad():
        small = hip(**kw)
    assert small.logits is None and torch.equal(small.loss, whole_out.loss)


@pytest.mark.parametrize("B", [1, 3])
def test_generate_matches_transformers(cuda, B):
    """generate() against transformers' generate on the decode case of tests/rnnt_refs.py with max_symbols_per_step = 3 (its conditions
    are asserted on the oracle alone, here and in tests/test_parakeet_rnnt_cpu.py): the non-blank tokens, their frames (the cumulative
    sums of transformers' per-step advances), the frames left by the forced advance among them, and the number of steps per row taken
    before the frame pointer reaches the end are equal."""
    ref_cfg = R.decode_model()
    rows, Tp, margin = R.decode_case(B, ref_cfg[1])
    R.assert_decode_conditions(rows, margin, ref_cfg[0].max_symbols_per_step)
    ref, hip = _pair(cuda, ref_cfg=ref_cfg)
    out = hip.generate(R.decode_feats(B).to(cuda))
    for b, row in enumerate(rows):
        n = int(out.count[b])
        assert out.tokens[b, :n].tolist() == row["tokens"] and out.frames[b, :n].tolist() == row["frames"], b
        assert int(out.steps[b]) == len(row["steps"]), b
        forced = [t for k, d, t in row["steps"] if k != R.RNNT_BLANK and d == 1]
        assert forced and all(out.frames[b, :n].tolist().count(t) == 3 for t in forced), b


def test_dynamic_eval_matches_oracle(cuda):
    """parakeet_tdt_lib.dynamic_eval_transducer_loss on a ParakeetForRNNT against the loop restated on transformers' model with the torch
    loss (tests/rnnt_refs.py): a [1, 80, 300] spectrogram, windows of 128 frames, overlap 64, two augmented copies, Adam at 1e-5.  Merged
    ids and frames are equal, the adapted joint logits of a probe after the last step are within 1e-3 (the TDT loop test's bar and method),
    parameters and `frozen` are restored bit for bit.  The smallest top-2 margin over every argmax the oracle takes is at least 1e-2.
    The fp32 oracle's own distance from its float64 run is printed next to ours.
    Measured (MI355X): adapted joint logits within 4.3e-06 of the fp32 oracle (max |logit| 7.1); against the float64 run of the oracle ours
    are 2.7e-06 away, the fp32 oracle itself 3.5e-06: a ratio of 0.78."""
    from dynamic_asr_eval_amd import parakeet_tdt_lib as N
    L = R.LOOP
    ref, hip = _pair(cuda, ref_cfg=R.decode_model())
    spec, tok = R.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=False)
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    probe_x = torch.randn(1, 67, 80, generator=torch.Generator().manual_seed(9))
    probe_ids = torch.tensor([[R.RNNT_BLANK, 5, 9]])
    infos = {}
    for dtype in (torch.float64, torch.float32):
        info = {"probe": (probe_x, probe_ids)}
        random.seed(17)
        model = copy.deepcopy(ref).to(dtype)
        infos[dtype] = (R.dynamic_eval_rnnt_ref(args, model, spec.to(dtype), L["seq_len"], 64, tok, L["num_negatives"], L["lr_args"],
                                                generator=torch.Generator().manual_seed(L["mask_seed"]), logits_out=info, dtype=dtype), info)
    (want_ids, want_frames), info = infos[torch.float32]
    assert infos[torch.float64][0] == (want_ids, want_frames)
    assert info["margin"] >= 1e-2, info["margin"]
    assert len(want_ids) > 0 and any(k != R.RNNT_BLANK for k, _, _ in info["steps"]) and any(k == R.RNNT_BLANK for k, _, _ in info["steps"])
    got_logits = {}
    step = N.Adam.step

    def probing_step(self, *a, **k):
        r = step(self, *a, **k)
        with torch.no_grad():
            got_logits["logits"] = hip(input_features=probe_x.to(cuda), decoder_input_ids=probe_ids).logits.cpu()
        return r

    N.Adam.step = probing_step
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    try:
        ids, frames, text = N.dynamic_eval_transducer_loss(args, hip, spec, L["seq_len"], 64, tok, use_tqdm=False, num_negatives=L["num_negatives"],
                                                           lr_args=L["lr_args"], spec_augment_config=R.PR.SPEC_AUGMENT)
    finally:
        N.Adam.step = step
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert text == tok.ids_to_text(ids) and len(ids) == len(frames)
    assert frames == sorted(frames) and all(0 <= f < 38 for f in frames)
    assert ids == want_ids and frames == want_frames
    want64 = infos[torch.float64][1]["logits"]
    err = (got_logits["logits"].double() - want64).abs().max().item()
    own = (info["logits"].double() - want64).abs().max().item()
    err32 = (got_logits["logits"] - info["logits"]).abs().max().item()
    print(f"adapted joint logits: ours vs fp32 oracle {err32:.3e}, ours vs float64 {err:.3e}, fp32 oracle vs float64 {own:.3e} "
          f"(ratio {err / max(own, 1e-30):.2f}; max |logit| {want64.abs().max().item():.3e})")
    assert err32 < 1e-3


def test_a_tdt_model_built_after_an_rnnt_one_keeps_its_bits(cuda):
    """Shared scratch or state would show here: a ParakeetForTDT's loss and nll on one small case, then a ParakeetForRNNT built and run
    (whole and chunked head, backward, generate) in the same process, then a fresh ParakeetForTDT from the same state dict: equal bits."""
    from dynamic_asr_eval_amd.parakeet_tdt_model import ParakeetForTDT
    cfg, tref = TR.hf_tdt_model(seed=3)
    x = torch.randn(2, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    lab, dec_in = _labels(2, 4, TR.TDT_VOCAB, 8)

    def tdt_run():
        hip = ParakeetForTDT(cfg, device=cuda)
        hip.load_state_dict(tref.state_dict())
        out, g = _grads(hip, input_features=x, decoder_input_ids=dec_in, labels=lab, sigma=0.05)
        return out.loss.clone(), out.nll.clone(), out.logits.clone(), g

    first = tdt_run()
    o = _oracle("mean_volume")
    ref, hip = _pair(cuda, ref_cfg=o["cfg"])
    _grads(hip, **_kw(o, cuda, "mean_volume"))
    _grads(hip, frames_per_chunk=4, **_kw(o, cuda, "mean_volume"))
    hip.generate(o["x"].to(cuda))
    second = tdt_run()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.isfinite(first[0]).all()
