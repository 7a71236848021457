"""ParakeetForTDT with the joint streamed over frame chunks (head(frames_per_chunk=) / joint_budget): the loss and every parameter's
gradient against transformers' ParakeetForTDT on the CPU with the bars of tests/test_parakeet_tdt_gpu.py, the options of the head against
the whole-joint path of the same build, scratch survival between forward and backward, the peak memory, and the loop
(parakeet_tdt_lib.dynamic_eval_tdt_loss) with every window chunked against the test-side oracle."""
import argparse
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

MODELS = {"64x2-vocab33": (dict(hidden=64, layers=2, vocab=33), (3, 67, 80), 4), "640x1-vocab1030": (dict(hidden=640, layers=1, vocab=1030), (2, 67, 80), 3)}
_ORACLE = {}


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


def _oracle(name):
    """transformers' model, its tdt_loss (reduction "mean", sigma 0.05) and every parameter's gradient on the inputs of
    test_logits_loss_and_every_gradient_match_transformers: computed once on the CPU, shared by the chunk sizes, left alone."""
    if name not in _ORACLE:
        from transformers.loss.loss_tdt import tdt_loss
        kw, shape, U = MODELS[name]
        cfg, ref = R.hf_tdt_model(seed=2, **kw)
        V1 = kw["vocab"]
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
        lab, dec_in = _labels(shape[0], U, V1, 5)
        logits = ref(input_features=x, decoder_input_ids=dec_in).logits
        Tp = logits.shape[1]
        loss = tdt_loss(logits[..., :V1], logits[..., V1:], lab, torch.full((shape[0],), Tp), torch.full((shape[0],), U), V1 - 1, list(R.DURATIONS),
                        0.05, "mean")
        ref.zero_grad()
        loss.backward()
        _ORACLE[name] = dict(cfg=(cfg, ref), x=x, lab=lab, dec_in=dec_in, Tp=Tp, loss=loss.item(), grads={n: p.grad.clone() for n, p in ref.named_parameters()})
    return _ORACLE[name]


def _grads(hip, **kw):
    """One grad-mode forward, zero_grad() BETWEEN forward and backward, backward -> (output, a copy of flat_grads)."""
    with torch.enable_grad():
        out = hip(**kw)
    hip.zero_grad(); hip.backward()
    return out, hip.flat_grads.clone()


@pytest.mark.parametrize("Tc", [1, 4])
@pytest.mark.parametrize("name", list(MODELS))
def test_chunked_loss_and_every_gradient_match_transformers(cuda, name, Tc):
    """Both models of test_logits_loss_and_every_gradient_match_transformers at T' = 9 with 1 and 4 frames per chunk (9 chunks; 4, 4 and
    1 frames): the loss within 2e-4 relative of transformers' tdt_loss, every parameter's gradient within 3e-3 of its largest entry +
    2e-8 (that test's bars, against the same CPU oracle), `logits` None, a second forward and backward with equal bits.  Chunked
    against unchunked is printed, not asserted to be equal: the GEMM's plan depends on M.
    Measured (MI355X): loss equal to transformers' as printed, worst relative gradient error 1.8e-06 (64 x 2) and 5.4e-04 (640 x 1) at both
    chunk sizes; chunked against unchunked: loss and nll equal bits, gradients within 1.5e-08 / 2.2e-08 (Tc 1 / 4, largest entry 0.22)
    and 7.5e-08 / 1.0e-07 (largest entry 0.37)."""
    o = _oracle(name)
    ref, hip = _pair(cuda, ref_cfg=o["cfg"])
    kw = dict(input_features=o["x"].to(cuda), decoder_input_ids=o["dec_in"], labels=o["lab"], sigma=0.05)
    out, first = _grads(hip, frames_per_chunk=Tc, **kw)
    assert out.logits is None and out.frames == o["Tp"] == 9 and out.nll.shape == (o["x"].shape[0],)
    lerr = abs(out.loss.item() - o["loss"]) / abs(o["loss"])
    assert lerr < 2e-4, (out.loss.item(), o["loss"])
    grads = hip.grads_hf()
    assert set(grads) == set(o["grads"])
    worst = 0.0
    for n, want in o["grads"].items():
        diff, scale = (grads[n].cpu() - want).abs().max().item(), want.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
    _, second = _grads(hip, frames_per_chunk=Tc, **kw)
    assert torch.equal(second, first)                                            # bit-reproducible
    whole_out, whole = _grads(hip, **kw)
    assert whole_out.logits is not None
    print(f"{name} Tc={Tc}: loss relative err vs transformers {lerr:.3e}, worst relative gradient error {worst:.3e}; chunked vs unchunked: "
          f"loss {abs(out.loss.item() - whole_out.loss.item()):.3e}, nll {(out.nll - whole_out.nll).abs().max().item():.3e}, "
          f"gradients {(first - whole).abs().max().item():.3e} (largest entry {whole.abs().max().item():.3e})")


def _close(chunked, whole, what):
    """The bar test_shared_decoder_rows_active_subset_and_frozen_decoder uses for a changed summation order: 1e-5 of the largest entry."""
    top = whole.abs().max().item()
    assert top > 0 and (chunked - whole).abs().max().item() <= 1e-5 * top, (what, (chunked - whole).abs().max().item(), top)


def test_options_on_the_chunked_path(cuda, monkeypatch):
    """Shared decoder rows with n_active = 2 of 3, per-row labels with label_lengths, a frozen `decoder.` (the LSTM backward's wrapper is
    made to raise; those gradients are exact zeros), a frozen encoder and batch_renorm_training(), each at 4 frames per chunk against
    the whole-joint path of the same build: the loss to 1e-5 relative, the gradients to 1e-5 of the largest entry."""
    from dynamic_asr_eval_amd import ops
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(3, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    lab, dec_in = _labels(1, 4, R.TDT_VOCAB, 7)
    lab3, dec_in3 = _labels(3, 4, R.TDT_VOCAB, 8)

    def both(what, **kw):
        a, ga = _grads(hip, frames_per_chunk=4, **kw)
        b, gb = _grads(hip, **kw)
        assert a.logits is None and b.logits is not None and a.nll.shape == b.nll.shape
        assert abs(a.loss.item() - b.loss.item()) <= 1e-5 * abs(b.loss.item()), what
        _close(ga, gb, what)
        return ga

    shared = dict(input_features=x, decoder_input_ids=dec_in, labels=lab, reduction="sum", n_active=2)
    free = both("shared rows, n_active 2 of 3", **shared)
    assert all(hip.G[n].abs().max().item() > 0.0 for n, _ in hip.spec if n.startswith("decoder."))
    both("label_lengths", input_features=x, decoder_input_ids=dec_in3, labels=lab3, reduction="sum", label_lengths=[4, 2, 3])
    both("mean, per-row labels", input_features=x, decoder_input_ids=dec_in3, labels=lab3, sigma=0.05)
    hip.frozen = {"encoder.", "encoder_projector."}
    enc_frozen = both("frozen encoder", **shared)
    assert all(hip.G[n].abs().max().item() == 0.0 for n, _ in hip.spec if n.startswith(("encoder.", "encoder_projector.")))
    assert enc_frozen.abs().max().item() > 0
    hip.frozen = set()
    with hip.batch_renorm_training():
        with torch.enable_grad():
            a = hip(frames_per_chunk=4, **shared)
        hip.zero_grad(); hip.backward(); ga = hip.flat_grads.clone()
    with hip.batch_renorm_training():                                            # a fresh state: the same running statistics
        with torch.enable_grad():
            b = hip(**shared)
        hip.zero_grad(); hip.backward()
    assert abs(a.loss.item() - b.loss.item()) <= 1e-5 * abs(b.loss.item())
    _close(ga, hip.flat_grads, "batch renorm")

    def forbidden(*args, **kw):
        raise AssertionError("the LSTM backward was launched although the prediction network is frozen")

    monkeypatch.setattr(ops, "lstm_cell_bwd", forbidden)
    hip.frozen = {"decoder."}
    frozen = both("frozen decoder", **shared)
    assert frozen.abs().max().item() > 0
    for n, _ in hip.spec:
        if n.startswith("decoder."):
            assert hip.G[n].abs().max().item() == 0.0, n
    hip.frozen = set()
    _close(frozen[hip.flat_grads != 0], free[hip.flat_grads != 0], "frozen decoder against the free run")


def test_generate_between_a_chunked_forward_and_backward(cuda):
    """What backward() needs of a chunked forward lives in tensors of its own, not in the shared scratch: a greedy decode (an encoder
    pass and the decode kernels, all on the model's scratch) between forward and backward leaves every gradient bit unchanged."""
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(3, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    lab, dec_in = _labels(3, 4, R.TDT_VOCAB, 8)
    kw = dict(input_features=x, decoder_input_ids=dec_in, labels=lab, sigma=0.05, frames_per_chunk=4)
    _, want = _grads(hip, **kw)
    with torch.enable_grad():
        hip(**kw)
    dec = hip.generate(torch.randn(2, 131, 80, generator=torch.Generator().manual_seed(3)).to(cuda))
    assert dec.tokens.shape[0] == 2
    hip.zero_grad(); hip.backward()
    assert want.abs().max().item() > 0 and torch.equal(hip.flat_grads, want)


def test_an_explicit_grad_logits_after_a_chunked_forward_is_refused(cuda):
    from dynamic_asr_eval_amd import ops
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(2, 67, 80, generator=torch.Generator().manual_seed(2)).to(cuda)
    lab, dec_in = _labels(2, 4, R.TDT_VOCAB, 8)
    with torch.enable_grad():
        out = hip(input_features=x, decoder_input_ids=dec_in, labels=lab, frames_per_chunk=2)
    with pytest.raises(ops.DynError) as e:
        hip.backward(torch.zeros(2, out.frames, 5, R.TDT_VOCAB + 5, device=cuda))
    assert "grad_logits" in str(e.value) and "chunked forward" in str(e.value)
    hip.zero_grad(); hip.backward()                                             # the refusal left the forward's state in place
    assert hip.flat_grads.abs().max().item() > 0
    hip.joint_budget = 1                                                         # the attribute alone: one frame per chunk
    with torch.no_grad():
        small = hip(input_features=x, decoder_input_ids=dec_in, labels=lab)
    assert small.logits is None and abs(small.loss.item() - out.loss.item()) <= 1e-5 * abs(out.loss.item())
    with torch.no_grad():                                                        # no labels: nothing to stream, today's path
        assert hip(input_features=x, decoder_input_ids=dec_in).logits is not None


def test_peak_memory_of_the_chunked_path(cuda):
    """The toy encoder with the 640-wide head at vocab 1030, T' = 64, U = 8, B = 2: torch.cuda.max_memory_allocated over forward +
    backward (the output kept alive, the peak reset before each run, after a warm-up of both paths) at 4 frames per chunk and
    unchunked.  The unchunked path holds all logits [2, 64, 9, 1035] (and as much again of their gradient, and z and dz), the chunked
    one a sixteenth: the two peaks must differ by at least half the bytes of the full logits tensor.
    Measured (MI355X): T' = 65, 1402.1 MB unchunked, 1385.8 MB chunked (the model's 1 GiB scratch included), 16.3 MB apart; logits 4.8 MB."""
    ref, hip = _pair(cuda, seed=2, hidden=640, layers=1, vocab=1030)
    B, U = 2, 8
    x = torch.randn(B, 515, 80, generator=torch.Generator().manual_seed(4)).to(cuda)
    lab, dec_in = _labels(B, U, 1030, 6)

    def peak(fpc):
        torch.cuda.synchronize(cuda)
        torch.cuda.reset_peak_memory_stats(cuda)
        with torch.enable_grad():
            out = hip(input_features=x, decoder_input_ids=dec_in, labels=lab, frames_per_chunk=fpc)
        hip.zero_grad(); hip.backward()
        torch.cuda.synchronize(cuda)
        top = torch.cuda.max_memory_allocated(cuda)
        return top, out.frames, out.loss.item()

    peak(4), peak(None)                                                          # the scratch, the position table, the allocator's pools
    chunked, Tp, loss_c = peak(4)
    whole, _, loss_w = peak(None)
    logits_bytes = B * Tp * (U + 1) * (1030 + 5) * 4
    print(f"T' = {Tp}: peak {whole} B unchunked, {chunked} B at 4 frames per chunk, difference {whole - chunked} B; full logits {logits_bytes} B")
    assert 60 <= Tp <= 68 and abs(loss_c - loss_w) <= 1e-5 * abs(loss_w)
    assert whole - chunked >= logits_bytes // 2


def test_dynamic_eval_with_every_window_chunked_matches_oracle(cuda, monkeypatch):
    """The overlap-64 case of test_dynamic_eval_matches_oracle (in order, no batch renorm) with model.joint_budget = 1 byte: every
    window's joint streams frame by frame (ops.tdt_loss is made to raise, the arcs pass is counted).  The oracle's tokens and frames,
    parameters and `frozen` restored bit for bit."""
    from dynamic_asr_eval_amd import ops, parakeet_tdt_lib as N
    L = R.LOOP
    ref, hip = _pair(cuda, ref_cfg=R.decode_model())
    spec, tok = R.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=False)
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    random.seed(17)
    info = {"probe": (torch.randn(1, 67, 80, generator=torch.Generator().manual_seed(9)), torch.tensor([[R.TDT_BLANK, 5, 9]]))}
    want_ids, want_frames = R.dynamic_eval_tdt_ref(args, ref, spec, L["seq_len"], 64, tok, L["num_negatives"], L["lr_args"],
                                                   generator=torch.Generator().manual_seed(L["mask_seed"]), logits_out=info)
    assert info["margin"] >= 1e-2 and len(want_ids) > 0
    calls = {"arcs": 0, "grad": 0}
    arcs, grad = ops.tdt_arcs_chunk, ops.tdt_grad_chunk

    def counted(name, fn):
        def run(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return run

    def forbidden(*a, **k):
        raise AssertionError("the whole-joint loss ran although the budget is one byte")

    monkeypatch.setattr(ops, "tdt_arcs_chunk", counted("arcs", arcs))
    monkeypatch.setattr(ops, "tdt_grad_chunk", counted("grad", grad))
    monkeypatch.setattr(ops, "tdt_loss", forbidden)
    hip.joint_budget = 1
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    ids, frames, text = N.dynamic_eval_tdt_loss(args, hip, spec, L["seq_len"], 64, tok, use_tqdm=False, num_negatives=L["num_negatives"],
                                                lr_args=L["lr_args"], spec_augment_config=R.PR.SPEC_AUGMENT, batch_renorm=False)
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert calls["arcs"] >= 16 and calls["grad"] == calls["arcs"], calls         # a frame per chunk, every window stepped
    assert text == tok.ids_to_text(ids) and ids == want_ids and frames == want_frames
