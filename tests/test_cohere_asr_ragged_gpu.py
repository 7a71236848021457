"""CohereAsrForConditionalGeneration on ragged batches (`input_lengths=`): the encoder's per-row frame counts (tests/test_parakeet_ragged_gpu.py)
and, behind it, lengths[b] keys in row b's cross-attention, teacher-forced (dyn_softmax_fwd_lens) and in the batched greedy step
(dyn_seq2seq_steps_len).  Against transformers' model with the matching `attention_mask` on the CPU and against every row run alone:
features [3, 131, 80], lens (131, 67, 100), the decode cases of tests/cohere_asr_refs.py at gain 8.  The decoder's logits hardly depend
on the audio with random weights, so the mask is judged on what the cross-attention READS (`decoder.proj` and every layer's keys | values;
tests/test_ragged_cpu.py shows that a forgotten mask misses that bar a hundredfold); ids are compared exactly."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cohere_asr_refs as R  # noqa: E402
import ragged_refs as RR  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = RR.LENS[0]


def _pair(cuda, **kw):
    from dynamic_asr_eval_amd.cohere_asr_model import CohereAsrForConditionalGeneration
    cfg, ref = R.hf_model(R.DEC_A, **kw)
    hip = CohereAsrForConditionalGeneration(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


@pytest.mark.parametrize("seed,prompt", R.DECODE_CASES, ids=["seed5-P2", "seed6-P2", "seed9-P3"])
def test_ragged_generate_matches_transformers_and_each_row_alone(cuda, seed, prompt):
    """generate() of the ragged batch (junk in the padding) equals transformers' generate with the attention_mask, id for id with the pad
    tail, and every row equals the row decoded alone at its own length, by transformers and by this package."""
    ref, hip = _pair(cuda, seed=seed, gain=8.0)
    x, prompt = RR.features(), torch.tensor(prompt)
    mask = RR.prefix_mask(LENS, x.shape[1])
    with torch.no_grad():
        want = ref.generate(input_features=RR.zero_padded(x, LENS), attention_mask=mask, decoder_input_ids=prompt, do_sample=False, max_new_tokens=16)
    got = hip.generate(RR.junk_padded(x, LENS).to(cuda), decoder_input_ids=prompt, max_new_tokens=16, input_lengths=LENS)
    assert got.dtype == torch.int64 and got.tolist() == want.tolist()
    pad, eos = ref.config.pad_token_id, ref.config.eos_token_id

    def trimmed(row):                                                                            # a row's ids up to its eos: the cut is the batch's
        row = row.tolist()
        return row[:row.index(eos) + 1] if eos in row else [t for t in row if t != pad]

    for b, n in enumerate(LENS):
        xb = x[b:b + 1, :n].clone()
        one, _ = R.hf_generate(ref, xb, prompt[b:b + 1])
        alone = hip.generate(xb.to(cuda), decoder_input_ids=prompt[b:b + 1], max_new_tokens=16)
        assert alone.tolist() == one.tolist(), b
        assert trimmed(got[b]) == trimmed(one[0]), b
    enc = hip.encode(RR.zero_padded(x, LENS).to(cuda), input_lengths=LENS)                        # the split call finds the lengths itself
    assert hip.generate(encoder_hidden_states=enc, decoder_input_ids=prompt, max_new_tokens=16).tolist() == want.tolist()
    given = hip.generate(encoder_hidden_states=enc.clone(), decoder_input_ids=prompt, max_new_tokens=16, enc_lengths=RR.enc_lens(LENS))
    assert given.tolist() == want.tolist()
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:                                                            # a copy without lengths would run unmasked
        hip.generate(encoder_hidden_states=enc.clone(), decoder_input_ids=prompt, max_new_tokens=16)
    assert "enc_lengths" in str(e.value)


def test_ragged_teacher_forced_forward_and_every_gradient(cuda):
    """Labels [3, 6] with a -100 tail on one row on the ragged batch: what the cross-attention reads (`decoder.proj`, every layer's keys |
    values) at valid frames within ragged_refs.tol of the float64 oracle, the logits and the loss within the recipe's bound, every
    parameter's gradient within ragged_refs.tol of the float64 oracle's and within tests/test_cohere_asr_gpu.py's relative bar."""
    ref, hip = _pair(cuda, seed=2, gain=8.0)
    ref64 = RR.double(ref)
    x, l3 = RR.features(), RR.enc_lens(LENS)
    lab = torch.randint(5, R.DEC_A["vocab_size"], (3, 6), generator=R.gen(5))
    lab[-1, 4:] = -100
    mask = RR.prefix_mask(LENS, x.shape[1])
    runs = []
    for m in (ref, ref64):
        m.zero_grad()
        o = m(input_features=RR.zero_padded(x, LENS).to(next(m.parameters()).dtype), attention_mask=mask, labels=lab)
        o.loss.backward()
        runs.append((o.loss.item(), o.logits.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
        m.zero_grad()
    (loss32, logits32, g32), (loss64, logits64, g64) = runs
    with torch.no_grad():
        kv32, kv64 = RR.cohere_kv(ref, x, LENS), RR.cohere_kv(ref64, x, LENS)
    with torch.enable_grad():
        out = hip(input_features=RR.junk_padded(x, LENS).to(cuda), labels=lab, input_lengths=LENS)
    assert out.lengths == l3 and out.lengths_device.tolist() == l3
    kv = torch.cat([c["kv"] for c in hip._dec["saved"]["layers"]], -1)
    tol, e32 = RR.tol(RR.valid_cat(kv32, l3), RR.valid_cat(kv64, l3))
    err = (RR.valid_cat(kv.cpu().double(), l3) - RR.valid_cat(kv64, l3)).abs().max().item()
    ltol, le32 = RR.tol(logits32, logits64)
    lerr = (out.logits.cpu().double() - logits64).abs().max().item()
    losstol = 4 * abs(loss32 - loss64) + 2e-5 * max(1.0, abs(loss64))
    print(f"cross K | V err {err:.2e} (transformers fp32 {e32:.2e}, bound {tol:.2e}); logits err {lerr:.2e} (fp32 {le32:.2e}, bound {ltol:.2e}); "
          f"loss {out.loss.item():.6f} vs {loss64:.6f} (bound {losstol:.1e})")
    assert torch.isfinite(out.logits).all() and torch.isfinite(kv).all()
    assert err <= tol and lerr <= ltol and abs(out.loss.item() - loss64) <= losstol
    hip.zero_grad(); hip.backward()
    got = hip.grads_hf()
    assert set(got) == set(g64)
    worst = (0.0, None)
    for n, w in g64.items():
        t, _ = RR.tol(g32[n], w)
        e = (got[n].cpu().double() - w).abs().max().item()
        worst = max(worst, (e / t, n))
        assert torch.isfinite(got[n]).all() and e <= t, (n, e, t)
        assert e < 3e-3 * w.abs().max().item() + 2e-8, (n, e)
    print(f"{len(g64)} gradients, worst err / bound {worst[0]:.2f} at {worst[1]}")


def test_one_row_with_its_full_length_is_the_call_without_lengths(cuda):
    """rows = 1 and input_lengths = [T]: logits, ids and gradients bit for bit those of the call without the keyword."""
    ref, hip = _pair(cuda, seed=5, gain=8.0)
    x = RR.features()[:1].contiguous().to(cuda)
    prompt, lab = torch.tensor(R.P2[:1]), torch.randint(5, 40, (1, 6), generator=R.gen(3))
    runs = []
    for kw in ({}, dict(input_lengths=[x.shape[1]])):
        ids = hip.generate(x, decoder_input_ids=prompt, max_new_tokens=16, **kw)
        with torch.enable_grad():
            out = hip(input_features=x, labels=lab, **kw)
        hip.zero_grad(); hip.backward()
        runs.append((ids, out.logits.clone(), out.loss.clone(), hip.flat_grads.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
