"""ParakeetForCTC on ragged batches (`input_lengths=`: per-row frame counts through the subsampling, the relative-position softmax and the conv
module) against transformers' ParakeetForCTC with the matching `attention_mask` on the CPU (the default sdpa path; float64 is `want`, the
bar is ragged_refs.tol: 4 x transformers' own fp32 error + 2e-5 * max(1, max |want|)) and against every row run alone by this package:
toy arch, [3, 131, 80], lens (131, 67, 100), (131, 8, 9), (130, 17, 1) — odd and even lengths, rows of 1, 2 and 3 encoder frames.
tests/test_ragged_cpu.py shows on the same inputs that a forgotten mask misses these bars by two orders of magnitude."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as R  # noqa: E402
import ragged_refs as RR  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [str(l) for l in RR.LENS]


@pytest.fixture(scope="module")
def pair(cuda):
    """(transformers fp32, its float64 copy, this package's model): built once, never modified (gradients are zeroed before each use)."""
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    cfg, ref = R.hf_model()
    hip = ParakeetForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, RR.double(ref), hip


@pytest.mark.parametrize("lens", RR.LENS, ids=IDS)
def test_ragged_forward_and_generate(cuda, pair, lens):
    """Logits at valid frames against transformers with the mask and against each row alone by this package; everything finite at padded
    frames; junk in the padding changes no bit; `lengths`; generate ids with the pad tail equal transformers'.
    Measured (MI355X): within 2.3e-07 .. 2.8e-07 of the float64 oracle (transformers fp32: 6.9e-07 .. 7.5e-07, bound 2.3e-05), bit-equal to
    every row run alone."""
    ref, ref64, hip = pair
    x = RR.features()
    l3 = RR.enc_lens(lens)
    tol, e32, want = RR.model_tol(ref, ref64, x, lens)
    with torch.no_grad():
        out = hip(input_features=RR.zero_padded(x, lens).to(cuda), input_lengths=list(lens))
        junk = hip(input_features=RR.junk_padded(x, lens).to(cuda), input_lengths=torch.tensor(lens, device=cuda))
        solo = [hip(input_features=x[b:b + 1, :n].clone().to(cuda)).logits.cpu() for b, n in enumerate(lens)]
    assert out.lengths == l3 and out.lengths_device.dtype == torch.int32 and out.lengths_device.tolist() == l3
    assert out.logits.shape == want.shape and out.frames == want.shape[1]
    assert torch.isfinite(out.logits).all()
    assert torch.equal(out.logits, junk.logits)
    err = (RR.valid_cat(out.logits.cpu().double(), l3) - RR.valid_cat(want, l3)).abs().max().item()
    err_solo = RR.valid_err(out.logits, solo)
    print(f"lens {lens}: vs transformers f64 {err:.2e}, vs solo {err_solo:.2e} | transformers fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, (err, tol)
    assert err_solo <= tol, (err_solo, tol)
    mask = RR.prefix_mask(lens, x.shape[1])
    with torch.no_grad():
        want_ids = ref.generate(input_features=RR.zero_padded(x, lens), attention_mask=mask)
    ids = hip.generate(RR.junk_padded(x, lens).to(cuda), input_lengths=lens)
    assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), want_ids)
    for b, n in enumerate(l3):
        assert (ids[b, n:] == R.PAD).all()
    assert torch.equal(hip.generate(x.to(cuda)).cpu(), ref.generate(input_features=x))                   # without lengths: no pad tail


@pytest.mark.parametrize("lens", RR.LENS, ids=IDS)
def test_ragged_loss_and_every_gradient(cuda, pair, lens):
    """`labels` -> the CTC loss over each row's own frames and every parameter gradient against transformers' backward on the same masked
    batch.  The gradient handed to backward() carries junk at the padded frames: backward() zeroes it there first.  Bar per parameter:
    ragged_refs.tol with the float64 oracle's gradient as `want`, and tests/test_parakeet_gpu.py's relative bar on top.
    Measured (MI355X): losses equal to six decimals, all 88 gradients within 0.06 .. 0.11 of their bound (worst: ctc_head.weight)."""
    from dynamic_asr_eval_amd import ops
    ref, ref64, hip = pair
    x = RR.features()
    l3 = RR.enc_lens(lens)
    g = torch.Generator().manual_seed(5)
    labels = torch.full((3, 4), R.PAD, dtype=torch.int64)
    for b, n in enumerate(l3):                                                                     # as many labels as fit a row's frames without repeats
        k = max(1, min(4, (n + 1) // 2))
        labels[b, :k] = torch.randperm(R.VOCAB - 1, generator=g)[:k]
    mask = RR.prefix_mask(lens, x.shape[1])
    grads = []
    for m in (ref, ref64):
        m.zero_grad()
        o = m(input_features=RR.zero_padded(x, lens).to(next(m.parameters()).dtype), attention_mask=mask, labels=labels)
        o.loss.backward()
        grads.append((o.loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}))
        m.zero_grad()
    (loss32, g32), (loss64, g64) = grads
    out = hip(input_features=RR.junk_padded(x, lens).to(cuda), input_lengths=lens)
    log_p = ops.log_softmax(out.logits)
    tlen = (labels != R.PAD).sum(-1).to(torch.int32).to(cuda)
    loss, nll, g_lp = ops.ctc_loss(log_p, labels.to(torch.int32).to(cuda), out.lengths_device, tlen, R.PAD, reduction=ref.config.ctc_loss_reduction)
    g_logits = ops.log_softmax_bwd(log_p, g_lp)
    keep = RR.prefix_mask(l3, out.frames)[:, :, None].to(cuda)
    g_logits = torch.where(keep, g_logits, torch.full_like(g_logits, 123.0))                      # junk where no frame is
    hip.zero_grad()
    hip.backward(g_logits)
    got = hip.grads_hf()
    ltol = 4 * abs(loss32 - loss64) + 2e-5 * max(1.0, abs(loss64))
    print(f"lens {lens}: loss {loss.item():.6f} vs {loss64:.6f} (bound {ltol:.1e})")
    assert abs(loss.item() - loss64) <= ltol
    assert set(got) == set(g64)
    worst = (0.0, None)
    for n, w in g64.items():
        tol, e32 = RR.tol(g32[n], w)
        err = (got[n].cpu().double() - w).abs().max().item()
        worst = max(worst, (err / tol, n))
        assert torch.isfinite(got[n]).all() and err <= tol, (n, err, tol, e32)
        assert err < 3e-3 * w.abs().max().item() + 2e-8, (n, err)                                # and tests/test_parakeet_gpu.py's relative bar
    print(f"lens {lens}: {len(g64)} gradients, worst err / bound {worst[0]:.2f} at {worst[1]}")


def test_active_subset_and_full_lengths(cuda, pair):
    """n_active = 2 of 3 on a ragged batch equals the full backward with a zero gradient on the third row; full lengths give the logits of the
    call without lengths bit for bit."""
    ref, ref64, hip = pair
    x, lens = RR.features().to(cuda), RR.LENS[0]
    out = hip(x, input_lengths=lens).logits
    gl = torch.zeros_like(out)
    gl[:2] = torch.randn(2, *out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x, input_lengths=lens); hip.zero_grad(); hip.backward(gl[:2].contiguous(), n_active=2)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5
    hip.zero_grad()
    with torch.no_grad():
        assert torch.equal(hip(x, input_lengths=[x.shape[1]] * 3).logits, hip(x).logits)


def test_refusals_on_the_device(cuda, pair):
    from dynamic_asr_eval_amd.lasr_model import LasrForCTC
    from dynamic_asr_eval_amd.ops import DynError
    import lasr_refs as LR
    ref, ref64, hip = pair
    x = RR.features().to(cuda)
    for bad, word in (([131, 67], "2 counts"), ([131, 0, 5], "1 .. T = 131"), ([131, 132, 5], "1 .. T = 131"), (torch.ones(3, device=cuda), "integers")):
        with pytest.raises(DynError) as e:
            hip(x, input_lengths=bad)
        assert "input_lengths" in str(e.value) and word in str(e.value)
    with pytest.raises(DynError) as e:
        hip(x, attention_mask=torch.ones(3, 131), input_lengths=[131, 67, 100])
    assert "attention_mask" in str(e.value)
    with hip.batch_renorm_training():
        with pytest.raises(DynError) as e:
            hip(x, input_lengths=[131, 67, 100])
        assert "batch_renorm_training" in str(e.value)
    cfg, _ = LR.hf_model()
    with pytest.raises(DynError) as e:
        LasrForCTC(cfg, device=cuda)(x, input_lengths=[131, 67, 100])
    assert "LasrForCTC" in str(e.value) and "input_lengths" in str(e.value)


# ----------------------------------------------------------------------------------------------------------- the transducers
def _transducer(kind, cuda, decode=False):
    """(refs module, transformers model, its float64 copy, this package's model, vocab, blank) of ParakeetForTDT / ParakeetForRNNT."""
    import rnnt_refs as NR
    import transducer_refs as TR
    from dynamic_asr_eval_amd.parakeet_rnnt_model import ParakeetForRNNT
    from dynamic_asr_eval_amd.parakeet_tdt_model import ParakeetForTDT
    mod, make, cls = (TR, TR.hf_tdt_model, ParakeetForTDT) if kind == "tdt" else (NR, NR.hf_rnnt_model, ParakeetForRNNT)
    cfg, ref = make(**mod.DECODE) if decode else make(seed=2)
    hip = cls(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return mod, ref, RR.double(ref), hip, cfg.vocab_size, cfg.blank_token_id


def _transducer_loss(kind, mod, logits, lab, T_b, U, V1, blank):
    if kind == "tdt":
        from transformers.loss.loss_tdt import tdt_loss
        return tdt_loss(logits[..., :V1], logits[..., V1:], lab, torch.tensor(T_b), torch.full((len(T_b),), U), blank, list(mod.DURATIONS), 0.0, "mean")
    return mod.rnnt_loss_torch(logits, lab.tolist(), list(T_b), [U] * len(T_b), blank, "mean")


@pytest.mark.parametrize("kind", ["tdt", "rnnt"])
def test_transducer_ragged_loss_and_every_gradient(cuda, kind):
    """ParakeetForTDT / ParakeetForRNNT on the ragged batch (131, 67, 100): the encoder states at valid frames, the loss with the rows' own
    frame counts as logit lengths (reduction "mean") and every parameter's gradient against transformers with the mask: the joint
    logits through transformers' tdt_loss (TDT) or the torch recursion of tests/rnnt_refs.py (RNN-T) with per-row lengths, autograd.
    Bars: ragged_refs.tol with the float64 oracle as `want`, and tests/test_parakeet_tdt_gpu.py's relative bar on the gradients.
    Measured (MI355X): joint logits within 4.5e-08 (TDT) / 3.3e-08 (RNN-T), losses equal to six decimals, all 101 gradients within 0.01 of
    their bound."""
    mod, ref, ref64, hip, V1, blank = _transducer(kind, cuda)
    lens, U = RR.LENS[0], 3
    l3 = RR.enc_lens(lens)
    x = RR.features()
    lab = torch.randint(3, V1 - 1, (3, U), generator=torch.Generator().manual_seed(5))
    dec_in = torch.cat([torch.full((3, 1), blank), lab], 1)
    mask = RR.prefix_mask(lens, x.shape[1])
    runs = []
    for m in (ref, ref64):
        m.zero_grad()
        dt = next(m.parameters()).dtype
        logits = m(input_features=RR.zero_padded(x, lens).to(dt), attention_mask=mask, decoder_input_ids=dec_in).logits
        loss = _transducer_loss(kind, mod, logits, lab, l3, U, V1, blank)
        loss.backward()
        runs.append((loss.item(), logits.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
        m.zero_grad()
    (loss32, logits32, g32), (loss64, logits64, g64) = runs
    with torch.enable_grad():
        out = hip(input_features=RR.junk_padded(x, lens).to(cuda), decoder_input_ids=dec_in, labels=lab, reduction="mean", input_lengths=lens)
    assert out.lengths == l3 and out.lengths_device.tolist() == l3
    tol, e32 = RR.tol(RR.valid_cat(logits32, l3), RR.valid_cat(logits64, l3))
    err = (RR.valid_cat(out.logits.cpu().double(), l3) - RR.valid_cat(logits64, l3)).abs().max().item()
    ltol = 4 * abs(loss32 - loss64) + 2e-5 * max(1.0, abs(loss64))
    print(f"{kind}: logits err {err:.2e} (transformers fp32 {e32:.2e}, bound {tol:.2e}); loss {out.loss.item():.6f} vs {loss64:.6f} (bound {ltol:.1e})")
    assert torch.isfinite(out.logits).all() and err <= tol
    assert abs(out.loss.item() - loss64) <= ltol
    hip.zero_grad(); hip.backward()
    got = hip.grads_hf()
    assert set(got) == set(g64)
    worst = (0.0, None)
    for n, w in g64.items():
        t, _ = RR.tol(g32[n], w)
        e = (got[n].cpu().double() - w).abs().max().item()
        worst = max(worst, (e / t, n))
        assert torch.isfinite(got[n]).all() and e <= t, (n, e, t)
        assert e < 3e-3 * w.abs().max().item() + 2e-8, (n, e)                                    # and tests/test_parakeet_tdt_gpu.py's relative bar
    print(f"{kind}: {len(g64)} gradients, worst err / bound {worst[0]:.2f} at {worst[1]}")


@pytest.mark.parametrize("kind", ["tdt", "rnnt"])
def test_transducer_ragged_generate(cuda, kind):
    """generate() of the ragged batch (300, 150, 228 of the decode case's 300 frames, junk in the padding) equals, row by row, transformers'
    generate of the row alone at its own length (tokens, frames, steps) and this package's decode of the row alone."""
    mod, ref, _, hip, V1, blank = _transducer(kind, cuda, decode=True)
    x = mod.decode_feats(3)
    lens = (300, 150, 228)
    out = hip.generate(RR.junk_padded(x, lens).to(cuda), input_lengths=lens)
    for b, n in enumerate(lens):
        row = mod.hf_greedy(ref, x[b:b + 1, :n].clone())[0][0]
        k = int(out.count[b])
        assert len(row["tokens"]) > 0
        assert out.tokens[b, :k].tolist() == row["tokens"] and out.frames[b, :k].tolist() == row["frames"], b
        assert int(out.steps[b]) == len(row["steps"]), b
        solo = hip.generate(x[b:b + 1, :n].clone().to(cuda))
        assert int(solo.count[0]) == k and solo.tokens[0, :k].tolist() == row["tokens"] and int(solo.steps[0]) == int(out.steps[b])
    enc = hip.encode(RR.zero_padded(x, lens).to(cuda), input_lengths=lens)                        # the split call finds the lengths itself
    again = hip.generate(enc=enc)
    assert torch.equal(again.count, out.count) and torch.equal(again.steps, out.steps)
    given = hip.generate(enc=enc.clone(), enc_lengths=RR.enc_lens(lens))
    assert torch.equal(given.count, out.count) and torch.equal(given.steps, out.steps)
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:                                                            # a copy without lengths would decode the padding
        hip.generate(enc=enc.clone())
    assert "enc_lengths" in str(e.value)


def test_transducer_family_refusals(cuda):
    """The classes without per-row frame counts refuse `input_lengths` by name, before they look at the input."""
    from dynamic_asr_eval_amd.nemotron3_5_asr_model import Nemotron3_5AsrForRNNT
    from dynamic_asr_eval_amd.nemotron_asr_streaming_model import NemotronAsrStreamingForRNNT
    from dynamic_asr_eval_amd.ops import DynError
    for cls in (NemotronAsrStreamingForRNNT, Nemotron3_5AsrForRNNT):
        for call in (lambda: cls.encode(None, None, input_lengths=[1]), lambda: cls.forward(None, None, input_lengths=[1]),
                     lambda: cls.generate(None, None, input_lengths=[1])):
            with pytest.raises(DynError) as e:
                call()
            assert "input_lengths is not built for" in str(e.value)
