"""Enc-dec RL modes (`training_mode` grpo / maxrl, opt-in through `rl_reward`; reference lcasr/lib.py:1172-1226,1330-1472,1659-1702) on
the HIP path: the batched sampled decode (dyn_decoder_steps_batch) against the single-row decode, `generate_enc_dec`'s sampled
form, `update_grpo` / `update_maxrl` (dyn_nll_loss_weighted, gradients accumulated over rollouts) against autograd on the CPU
oracle, the loop against tests/enc_dec_rl_cpu.py, and the harness.  Smallest decoder of tests/test_enc_dec_gpu.py, 256-frame windows."""
import argparse
import os
import pickle
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from enc_dec_rl_cpu import CFG, VOCAB, enc_dec_dynamic_eval_rl_ref, generate_rows_ref, pair, rl_loss_ref

pytestmark = pytest.mark.gpu
CAP = 12


@pytest.fixture(scope="module")
def decode_case(cuda):
    ref, hip = pair(cuda, seed=5, eos_bias=2.5)
    x = torch.randn(1, 80, 256, generator=torch.Generator().manual_seed(8))
    return ref, hip, x, hip.forward(x.to(cuda))


@pytest.mark.parametrize("rows,seed", [(1, 25), (3, 24), (4, 24)])
def test_batched_sampled_decode_equals_single_row_decodes(cuda, decode_case, rows, seed):
    """Row r of generate_batch(seed=s) holds the ids of generate(sample=True, seed=s + r) — and of the oracle's prefix re-run with
    the same draws.  Seeds 24 .. 27 give, on the oracle, an eos at step 0, a row cut by the cap of 12 and rows of 5 and 3 tokens
    (asserted); check_every = 5 divides none of them.  Caches, logits and scratch start as NaN: a finished row's cache is never
    read, an unwritten row never leaks into a live one."""
    ref, hip, x, enc = decode_case
    margins = []
    want = generate_rows_ref(ref, x, rows, max_generate=CAP, seed=seed, margins=margins)
    assert min(margins) > 1e-3, "fixture: a sampled step is a near-tie on the oracle"
    if rows >= 3:
        assert len(want[0]) == 0 and len(want[1]) == CAP and len(set(map(len, want))) >= 3, want
    else:
        assert len(want[0]) == CAP
    single = [hip.generate(x.to(cuda), encoder_states=enc, sample=True, seed=seed + r, max_tokens=CAP)["text_sequence"] for r in range(rows)]
    assert single == want
    for every in (5, 1, 64):
        got = hip.generate_batch(x.to(cuda), rows, encoder_states=enc, seed=seed, max_tokens=CAP, check_every=every, fill=float("nan"))
        assert got["text_sequences"] == single, (every, got, single)
    t = hip.generate_batch(x.to(cuda), rows, encoder_states=enc, seed=seed, max_tokens=CAP, temperature=0.7)["text_sequences"]
    assert t == [hip.generate(x.to(cuda), encoder_states=enc, sample=True, temperature=0.7, seed=seed + r, max_tokens=CAP)["text_sequence"]
                 for r in range(rows)]


def test_batched_decode_logits_are_bitwise_the_single_row_logits(cuda, decode_case):
    """One step of dyn_decoder_steps_batch on 4 rows with different tokens against dyn_decoder_steps on each row alone: the logits
    and the cache rows are bit-identical (same accumulation order per row), a finished row's cache / logits stay untouched, its next
    token slot receives eos; the tile-kernel fallback (`fused_decode` off) returns the same ids; bad descriptors are refused."""
    import ctypes
    from dynamic_asr_eval_amd import _lib, ops
    from dynamic_asr_eval_amd.enc_dec import DEC
    _, hip, x, enc = decode_case
    h = enc["hidden"][0]
    dd, L, R, T = hip.dec["dec_d_model"], hip.dec["dec_layers"], 4, 3
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    per_row = int(lib.dyn_decoder_row_scratch_floats(dd, dd * hip.dec["dec_ff_mult"], hip.dec["dec_heads"]))
    prefix = torch.tensor([[0, 5, 9, 0, 0], [0, 7, 7, 0, 0], [0, 1, 2, 0, 0], [0, 63, 33, 0, 0]], dtype=torch.int32, device=cuda)
    with torch.no_grad(), ops.use_workspace(hip._scratch()):
        kv = [ops.linear(h, hip.P[f"{DEC}layers.{l}.cross.kv.weight"], hip.P[f"{DEC}layers.{l}.cross.kv.bias"]) for l in range(L)]
        cache = [torch.full((R, T + 1, 3 * dd), float("nan"), device=cuda) for _ in range(L)]
        tok = prefix.clone()
        fin = torch.zeros(R, dtype=torch.int32, device=cuda)
        logits, scratch = torch.full((R, VOCAB), float("nan"), device=cuda), torch.full((R, per_row), float("nan"), device=cuda)
        base, keep = hip._decoder_desc(kv, cache, tok, h.shape[0], logits=logits, scratch=scratch)
        desc = _lib.DecoderBatchDesc(base=base, rows=R, eos_id=0, token_stride=tok.shape[1], cache_stride=(T + 1) * 3 * dd, finished=fin.data_ptr())
        for t in range(T):
            fin.zero_()                                       # a greedy pick of eos must not retire a row of this scripted run
            if t == 2:
                fin[1] = 1                                    # row 1 retires before the last step
            _lib.check(lib.dyn_decoder_steps_batch(ctypes.byref(desc), t, 1, 0, 1.0, 0, 0, st), "dyn_decoder_steps_batch")
            if t < 2:
                tok[:, t + 1] = prefix[:, t + 1]              # keep the scripted prefix
        assert int(tok[1, 3]) == 0 and torch.isnan(cache[0][1, 2]).all() and torch.isfinite(cache[0][1, :2]).all()
        for r in range(R):
            c1 = [torch.zeros(T + 1, 3 * dd, device=cuda) for _ in range(L)]
            t1 = prefix[r].clone()
            d1, k1 = hip._decoder_desc(kv, c1, t1, h.shape[0])
            for t in range(T if r != 1 else 2):
                _lib.check(lib.dyn_decoder_steps(ctypes.byref(d1), t, 1, 0, 1.0, 0, 0, st), "dyn_decoder_steps")
                t1[t + 1] = prefix[r, t + 1] if t < 2 else t1[t + 1]
            n = T if r != 1 else 2
            print("row", r, "max |batched - single| logits", float((logits[r] - k1[1]).abs().max()))
            assert torch.equal(logits[r], k1[1]), r
            for l in range(L):
                assert torch.equal(cache[l][r, :n], c1[l][:n]), (r, l)
            if r != 1:
                assert int(tok[r, 3]) == int(t1[3])
        for bad in (dict(rows=9), dict(rows=0), dict(token_stride=1), dict(cache_stride=4)):
            d2 = _lib.DecoderBatchDesc(base=base, rows=R, eos_id=0, token_stride=tok.shape[1], cache_stride=(T + 1) * 3 * dd, finished=fin.data_ptr())
            for k, v in bad.items():
                setattr(d2, k, v)
            with pytest.raises(_lib.DynError):
                _lib.check(lib.dyn_decoder_steps_batch(ctypes.byref(d2), 0, 1, 0, 1.0, 0, 0, st), "dyn_decoder_steps_batch")
        del keep
    fused = hip.generate_batch(x.to(cuda), 3, encoder_states=enc, seed=24, max_tokens=CAP)["text_sequences"]
    hip.fused_decode = False
    try:
        assert hip.generate_batch(x.to(cuda), 3, encoder_states=enc, seed=24, max_tokens=CAP)["text_sequences"] == fused
    finally:
        hip.fused_decode = True


def test_generate_enc_dec_sampled_form(cuda, decode_case):
    """generate_enc_dec(sample=4, greedy=False) (lib.py:1172-1226): [R, Lmax] long padded with 0, bos removed, the encoder output,
    lengths [R] — rows in row order, cap = max_generate; softmax input is logits * temperature; the greedy form is unchanged."""
    from dynamic_asr_eval_amd.enc_dec import generate_enc_dec
    ref, hip, x, _ = decode_case
    want = generate_rows_ref(ref, x, 4, max_generate=CAP, seed=24)
    seq, enc_out, lens = generate_enc_dec(hip, x.to(cuda), max_generate=CAP, sample=4, greedy=False, temperature=1.0, seed=24)
    assert seq.dtype == torch.long and tuple(seq.shape) == (4, CAP) and lens.tolist() == [len(w) for w in want] == [0, CAP, 5, 3]
    for r, w in enumerate(want):
        assert seq[r, :len(w)].tolist() == w and not seq[r, len(w):].any()
    assert "hidden" in enc_out and "final_posteriors_ctc" in enc_out
    m = []
    want2 = generate_rows_ref(ref, x, 2, max_generate=CAP, temperature=1.3, seed=40, margins=m)
    assert min(m) > 1e-3
    seq2, _, lens2 = generate_enc_dec(hip, x.to(cuda), max_generate=CAP, sample=2, greedy=False, temperature=1.3, seed=40)
    assert [seq2[r, :int(lens2[r])].tolist() for r in range(2)] == want2
    hip.random_seed, hip._draws = 9, 0                         # default seed: a fresh stream block of model.random_seed
    ref.language_model_decoder.random_seed = 9
    ref.language_model_decoder.streams.draws = 0
    seq3, _, lens3 = generate_enc_dec(hip, x.to(cuda), max_generate=CAP, sample=1, greedy=False)
    assert [seq3[0, :int(lens3[0])].tolist()] == generate_rows_ref(ref, x, 1, max_generate=CAP)
    greedy = generate_enc_dec(hip, x.to(cuda))
    assert len(greedy) == 1 and greedy[0].tolist() == hip.generate(x.to(cuda))["text_sequence"]


HYPS = [[5, 9, 33, 2, 17, 40, 8], [], [12, 3, 3], [61, 1, 7, 7, 20]]
REWARDS = [0.15, 0.95, 0.4, 0.62]


@pytest.mark.parametrize("mode,kw", [("grpo", dict(normalize_std=True)), ("grpo", dict(normalize_std=False)), ("maxrl", dict(success_threshold=0.5)),
                                     ("maxrl", dict(success_threshold=0.99))])
def test_update_grpo_maxrl_loss_and_every_gradient(cuda, mode, kw):
    """update_grpo / update_maxrl (lib.py:1400-1472) on fixed hypotheses of 7, 0, 3 and 5 tokens: the loss and the gradient of EVERY
    parameter (decoder gradients accumulated over the rollouts, the encoder's through the summed cross-attention gradient) against
    autograd on the CPU oracle, with the tolerances tests/test_enc_dec_gpu.py applies to calc_loss_enc_dec; MaxRL's skip -> None."""
    from dynamic_asr_eval_amd.enc_dec import policy_forward, update_grpo, update_maxrl
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = pair(cuda)
    tok = SyntheticTokenizer(VOCAB)
    x = torch.randn(1, 80, 256, generator=torch.Generator().manual_seed(0))
    texts = [tok.decode(q) for q in HYPS]
    ref.ctc_loss_weight = hip.ctc_loss_weight = 0.0
    loss_ref = rl_loss_ref(ref, x, HYPS, REWARDS, mode, **kw)
    hip.zero_grad()
    fn = update_grpo if mode == "grpo" else update_maxrl
    loss = fn(hip, x.to(cuda), tok, texts, REWARDS, **kw)
    if loss_ref is None:
        assert loss is None and not bool(hip.flat_grads.any())
        return
    loss_ref.backward()
    assert isinstance(loss, float) and abs(loss - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref)))
    worst = 0.0
    for (n, _), gh, p in zip(hip.named_parameters(), hip.grads(), ref.ordered_parameters()):
        want = p.grad if p.grad is not None else torch.zeros_like(p)             # the CTC head: no gradient at ctc_loss_weight 0
        rel = (gh.cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        if p.grad is None:
            assert not bool(gh.any()), n
            continue
        worst = max(worst, rel)
        assert rel < 2e-3, (n, rel)
    print("enc-dec RL worst relative gradient error", mode, kw, worst)
    lp, mask = policy_forward(hip, x.to(cuda), tok, texts)
    with torch.no_grad():
        from enc_dec_rl_cpu import policy_forward_ref
        lp_ref, mask_ref = policy_forward_ref(ref, x, HYPS)
    assert torch.equal(mask, mask_ref) and (lp - lp_ref).abs().max().item() < 2e-4


class ScriptedReward:
    """(ref, hyps) -> rewards by window: > 0.95 mean (early exit), all equal (skipping), then mixed (update)."""
    TABLE = [[1.0, 1.0, 0.9, 1.0], [0.5, 0.5, 0.5, 0.5], [0.1, 0.95, 0.3, 0.2]]

    def __init__(self):
        self.calls = 0

    def __call__(self, ref, hyps):
        self.calls += 1
        return list(self.TABLE[(self.calls - 1) % 3])


@pytest.mark.parametrize("mode,reward", [("grpo", "wer_cer"), ("maxrl", "wer_cer"), ("grpo", "scripted"), ("maxrl", "scripted")])
def test_enc_dec_dynamic_eval_rl_matches_cpu_restatement(cuda, capsys, mode, reward):
    """The loop with `rl_reward` set over a 3-window recording against tests/enc_dec_rl_cpu.py (lib.py:1659-1702 on EncDecRef with the
    oracle's counter-based sampler): the same rollout ids, rewards and decisions at EVERY window, adapted parameters within 5e-5,
    the same final transcript, weights restored bit for bit.  Every sampled step's top-2 margin on the oracle exceeds 1e-3
    (asserted: a near-tie is a bad fixture).  The scripted reward forces the > 0.95 exit, `skipping` and an update in turn."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import enc_dec as E
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = pair(cuda, seed=7, eos_bias=E2E_EOS_BIAS)
    tok = SyntheticTokenizer(VOCAB)
    spec = torch.randn(1, 80, 700, generator=torch.Generator().manual_seed(4))
    _, keys = R.prepare_chunks(spec, 256, 0)
    mg = torch.Generator().manual_seed(6)
    masks = {k: (R.draw_masks(3, 12, 80, mg), ([], [])) for k in keys}
    thr = 0.9 if reward == "scripted" else E2E_MAXRL_THRESHOLD
    trace, margins = [], []
    ref_reward = ScriptedReward() if reward == "scripted" else (lambda r, h: _quiet(E.calc_rewards, r, h))
    want, p_ref = enc_dec_dynamic_eval_rl_ref(ref, spec, 256, tok, MADGRAD_REF, {'lr': 1e-4}, mode, ref_reward, fixed_masks=masks,
                                              random_seed=E2E_SEED, maxrl_success_threshold=thr, trace=trace, margins=margins)
    assert len(trace) == 3 and min(margins) > 1e-3, f"fixture: sampled near-tie on the oracle ({min(margins):.2e})"
    decisions = [d for _, _, d in trace]
    if reward == "scripted":
        assert decisions == ["early_exit", "skipping", "update"]
    else:
        assert "update" in decisions, decisions
    args = argparse.Namespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 2048, 'overlap': 0}, 'training': {}},
                              optim_lr=1e-4, epochs=1, shuffle=False, training_mode=mode, spec_augment_fixed_masks=masks, random_seed=E2E_SEED,
                              rl_reward=ScriptedReward() if reward == "scripted" else "wer_cer", maxrl_success_threshold=thr)
    seen = []
    real = E.generate_enc_dec

    def spy(*a, **kw):
        out = real(*a, **kw)
        if kw.get("greedy", True):
            return out
        seen.append([out[0][r, :int(out[2][r])].tolist() for r in range(out[0].shape[0])])
        return out

    E.generate_enc_dec = spy
    try:
        before = hip.flat_params.clone()
        w0 = hip.ctc_loss_weight
        got, p = E.enc_dec_dynamic_eval(args, hip, spec, 256, 0, tok, use_tqdm=False, return_params=True)
    finally:
        E.generate_enc_dec = real
    out = capsys.readouterr().out
    assert torch.equal(hip.flat_params, before) and hip.ctc_loss_weight == w0
    assert seen == [r for r, _, _ in trace], "rollout ids"
    printed = [eval(l) for l in out.splitlines() if l.startswith("[") and l.endswith("]") and "w" not in l]
    assert printed == [rw for _, rw, _ in trace], "rewards"
    assert ("\n" + out).count("\nskipping\n") == decisions.count("skipping")
    assert out.count("skipping task") == decisions.count("maxrl_skip")
    assert out.count("loss (maxrl)" if mode == "maxrl" else " loss\n") == decisions.count("update")
    if reward == "wer_cer":
        assert out.startswith("rl_reward='wer_cer'") and "BLEU" in out.splitlines()[0]
    assert got == want
    moved = max((a - b).abs().max().item() for a, b in zip(p_ref, [q.detach() for q in ref.ordered_parameters()]))
    assert moved > 1e-6, "the update must move the parameters"
    for a, b in zip(p, p_ref):
        assert (a - b).abs().max().item() < 5e-5
    assert hip.language_model_decoder.training is False


def _quiet(fn, *a):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


E2E_SEED, E2E_EOS_BIAS, E2E_MAXRL_THRESHOLD = 3, 0.0, 0.2


def test_rl_modes_still_refused_without_rl_reward(cuda):
    from dynamic_asr_eval_amd.enc_dec import enc_dec_dynamic_eval
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    _, hip = pair(cuda)
    args = argparse.Namespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 2048, 'overlap': 0}, 'training': {}},
                              optim_lr=1e-4, training_mode='maxrl')
    with pytest.raises(NotImplementedError, match="only 'teacher_ce' is implemented"):
        enc_dec_dynamic_eval(args, hip, torch.randn(1, 80, 300), 256, 0, SyntheticTokenizer(VOCAB), use_tqdm=False)
    args.rl_reward = 'bleu'
    with pytest.raises(ValueError):
        enc_dec_dynamic_eval(args, hip, torch.randn(1, 80, 300), 256, 0, SyntheticTokenizer(VOCAB), use_tqdm=False)


def test_harness_maxrl_with_rl_reward(cuda, tmp_path, capsys):
    """enc_dec_dynamic_eval_test.py with `--training_mode maxrl -kwargs rl_reward="'wer_cer'"` on synthetic_small: runs to a WER line and
    a pickle; the first line of the RL path states the BLEU deviation."""
    from dynamic_asr_eval_amd import enc_dec_dynamic_eval_test as A, lib
    from dynamic_asr_eval_amd.enc_dec import EncDecSCConformerXL
    from dynamic_asr_eval_amd.synthetic_weights import init_synthetic
    m = EncDecSCConformerXL(CFG, vocab_size=128, device=cuda)
    init_synthetic(m, seed=1, blank_bias=1.0)
    ck = str(tmp_path / "encdec.pt")
    model_cfg = dict(CFG, feat_in=80, subsampling_factor=8, conv_kernel_size=9, self_conditioning=True, rotary_base_freq=1500000)
    torch.save({'config': {'model': model_cfg, 'audio_chunking': {'size': 2048, 'overlap': 0}, 'training': {'max_seq_len': 0}},
                'model': {k: v.cpu() for k, v in m.state_dict().items()}}, ck)
    save = str(tmp_path / "rl.pkl")
    avg = A.main(lib.apply_args(A.build_parser(), ["-d", "synthetic_small", "-s", save, "--training_mode", "maxrl", "--maxrl_success_threshold", "0.1",
                                                   "--breaks", "-c", ck, "-seq", "512", "-o", "0", "-nv", "-kwargs", "optim_lr=1e-5", "vocab_size=128",
                                                   "rl_reward='wer_cer'", "spec_augment_n_freq_masks=2", "spec_augment_freq_mask_param=10"]))
    out = capsys.readouterr().out
    assert "WER: " in out and "Average WER: " in out and "Student rollouts:" in out and "avg reward" in out and "Saved to" in out and avg >= 0
    assert "rl_reward='wer_cer'" in out and "BLEU" in out
    d = pickle.load(open(save.replace(".pkl", "_1.pkl"), "rb"))
    assert len(d["model_output"]) == 1 and d["args_dict"]["training_mode"] == "maxrl" and d["args_dict"]["rl_reward"] == "wer_cer"
