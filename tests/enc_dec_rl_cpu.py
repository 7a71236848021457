"""CPU restatement (plain torch + autograd on oracle/enc_dec_ref.EncDecRef) of the enc-dec RL path the GPU tests compare the HIP
path with: the sampled rollouts of `generate_enc_dec(sample=R, greedy=False)` (reference lcasr/lib.py:1172-1226) with the oracle's
counter-based sampler, `_policy_forward` / `update_grpo` / `update_maxrl` (:1361-1472) and the RL branch of `enc_dec_dynamic_eval`
(:1659-1702).  tests/test_enc_dec_rl_cpu.py holds the loss formulas and the retirement rule to the reference's own functions
(tests/golden/enc_dec_rl_pins.json).  Test infrastructure only."""
import numpy as np
import torch

from oracle.dynamic_eval_ref import apply_masks, draw_masks, prepare_chunks
from oracle.enc_dec_ref import _Streams, enc_dec_inference_ref, mix64

CFG = dict(n_layers=2, d_model=256, n_heads=2, head_dim=128, subsampling_conv_channels=64, dec_d_model=256, dec_layers=2, dec_heads=4,
           ctc_loss_weight=0.3)
VOCAB = 64


def pair(cuda, seed=3, eos_bias=0.0):
    """EncDecRef and the HIP model with the same seeded weights (as tests/test_enc_dec_gpu.py `_pair`); `eos_bias` is added to the
    head's eos logit on both so that sampled rows end at mixed lengths."""
    from oracle.enc_dec_ref import EncDecRef
    from dynamic_asr_eval_amd.enc_dec import EncDecSCConformerXL
    ref = EncDecRef(CFG, vocab_size=VOCAB, seed=seed, blank_bias=1.0)
    with torch.no_grad():
        ref.language_model_decoder.head.bias[0] += eos_bias
    hip = None
    if cuda is not None:
        hip = EncDecSCConformerXL(CFG, vocab_size=VOCAB, device=cuda)
        sd = ref.hip_state_dict()
        assert sorted(sd) == sorted(n for n, _ in hip.spec)
        hip.load_state_dict(sd)
    return ref, hip


def gumbel_keys(logits, inv_t, seed, step):
    """The keys dyn_gumbel_argmax_rows maximises (oracle/enc_dec_ref.gumbel_argmax, with the keys kept): float64 [C]."""
    C = logits.shape[-1]
    u = (np.float64(2.0) * (mix64(seed, step, np.arange(C, dtype=np.uint64)) >> np.uint64(41)).astype(np.float64) + 1.0) * 2.0 ** -24
    return logits.detach().numpy().astype(np.float64) * np.float64(np.float32(inv_t)) - np.log(-np.log(u))


@torch.no_grad()
def sample_row(ref, h, seed, step0, limit, inv_t=1.0, margins=None):
    """One sampled row: draws of (seed, step0 + t), at most `limit` tokens, cut at the first eos (= 0).  `margins` collects the
    top-2 margin of the perturbed keys at every step (a near-tie there is where fp32 summation order could flip an id)."""
    dec = ref.language_model_decoder
    toks = [0]
    while len(toks) <= limit:
        keys = gumbel_keys(dec(torch.LongTensor(toks), h)[-1], inv_t, seed, step0 + len(toks) - 1)
        if margins is not None:
            top = np.sort(keys)[-2:]
            margins.append(float(top[1] - top[0]))
        nxt = int(np.argmax(keys))
        if nxt == 0:
            break
        toks.append(nxt)
    return toks[1:]


def generate_rows_ref(ref, x, rows, max_generate=256, temperature=1.0, seed=None, margins=None, hidden=None):
    """generate_enc_dec(sample=rows, greedy=False) in row order: softmax input logits * temperature (lib.py:1200), a row keeps at most
    min(max_generate, dec_max_positions - 1) tokens; row r draws with seed + r.  seed None: (random_seed, a fresh stream block)."""
    dec = ref.language_model_decoder
    with torch.no_grad():
        h = ref.forward(x)["hidden"][0] if hidden is None else hidden
    seed, step0 = (dec.random_seed, dec.streams.next()) if seed is None else (seed, 0)
    limit = max(1, min(int(max_generate), ref.dec["dec_max_positions"] - 1))
    return [sample_row(ref, h, seed + r, step0, limit, inv_t=temperature, margins=margins) for r in range(rows)]


def policy_forward_ref(ref, x, ids):
    """`_policy_forward` (lib.py:1361-1397) -> (log_probs [R, Lmax] with autograd, mask): one encoder forward, the decoder on each
    bos-prefixed hypothesis, the log-probability of its tokens followed by eos."""
    R, Lmax = len(ids), max(len(q) for q in ids) + 1
    h = ref.forward(x)["hidden"][0]
    rows, mask = [], torch.zeros(R, Lmax, dtype=torch.bool)
    for j, q in enumerate(ids):
        lp = ref.language_model_decoder(torch.LongTensor([0] + list(q)), h).log_softmax(-1)
        lp = lp.gather(-1, torch.LongTensor(list(q) + [0])[:, None])[:, 0]
        rows.append(torch.nn.functional.pad(lp, (0, Lmax - lp.shape[0])))
        mask[j, :len(q) + 1] = True
    return torch.stack(rows), mask


def grpo_loss(log_probs, mask, rewards, normalize_std=True, std_epsilon=1e-7):
    """lib.py:1411-1420"""
    rewards = torch.as_tensor(rewards, dtype=torch.float32)
    advantage = rewards - rewards.mean()
    if normalize_std:
        advantage = advantage / (rewards.std(unbiased=False) + std_epsilon)
    token_counts = mask.sum(dim=-1).clamp_min(1)
    seq_mean_log_probs = (log_probs * mask).sum(dim=-1) / token_counts
    return -(seq_mean_log_probs * advantage).mean()


def maxrl_loss(log_probs, mask, rewards, success_threshold=0.9, epsilon=1e-6):
    """lib.py:1450-1470; None in the two skip cases"""
    rewards_bin = torch.as_tensor([1.0 if r >= success_threshold else 0.0 for r in rewards], dtype=torch.float32)
    mean = rewards_bin.mean()
    if mean.item() <= 0 or mean.item() >= 1:
        return None
    advantage = (rewards_bin - mean) / (mean + epsilon)
    per_token_loss = (-log_probs * advantage.unsqueeze(-1)).masked_fill(~mask, 0)
    return per_token_loss.sum() / mask.sum()


def rl_loss_ref(ref, x, ids, rewards, mode, **kw):
    if mode == 'maxrl' and maxrl_loss(torch.zeros(len(ids), 1), torch.ones(len(ids), 1, dtype=torch.bool), rewards, **kw) is None:
        return None
    lp, mask = policy_forward_ref(ref, x, ids)
    return maxrl_loss(lp, mask, rewards, **kw) if mode == 'maxrl' else grpo_loss(lp, mask, rewards, **kw)


def retire(draws, max_generate, eos_id=0):
    """The retirement rule of generate_enc_dec (lib.py:1193-1217) on scripted draws, rows in ROW order: draws[t][r] is the draw of row
    r at step t.  A row retires when its draw is eos or its length including bos exceeds max_generate; that draw is discarded."""
    rows = [[] for _ in draws[0]]
    live = list(range(len(rows)))
    t = 0
    while live:
        for r in list(live):
            if draws[t][r] == eos_id or len(rows[r]) + 1 > max_generate:
                live.remove(r)
            else:
                rows[r].append(draws[t][r])
        t += 1
    return rows


def enc_dec_dynamic_eval_rl_ref(model, spec, seq_len, tokenizer, optimizer_cls, lr_args, mode, reward_fn, fixed_masks=None, random_seed=0,
                                maxrl_success_threshold=0.9, grpo_normalize_std=True, trace=None, margins=None):
    """reference lcasr/lib.py:1475-1732 with the RL branch (:1659-1702): teacher = greedy decode of the clean copy; 4 rollouts of the
    augmented copy at temperature 1.0; rewards against the teacher's text; > 0.95 mean -> no update; all zero / all equal -> skipping;
    else update_maxrl / update_grpo, zero_grad, backward, step.  `trace` collects per window (rollout ids, rewards, decision)."""
    dec = model.language_model_decoder
    dec.dropout_emb, dec.ff_out_dropout, dec.dropout_attn = 0.0, 0.0, 0.0
    dec.random_seed, dec.streams = random_seed, _Streams()
    original = [p.clone().detach() for p in model.ordered_parameters()]
    optimizer = optimizer_cls(model.ordered_parameters(), **lr_args)
    seq_len = min(seq_len, spec.shape[-1])
    model.eval()
    training_data, training_keys = prepare_chunks(spec, seq_len, 0)
    for key in training_keys:
        audio_chunk = training_data[key].clone().repeat(2, 1, 1)
        masks = fixed_masks[key] if fixed_masks is not None else (draw_masks(0, 1, 80), ([], []))
        apply_masks(audio_chunk[0], masks, False)
        with torch.no_grad():
            enc_states = model.forward(audio_signal=audio_chunk[-1, None])
        teacher_text = tokenizer.decode(model.generate(audio_chunk[-1, None], encoder_states=enc_states)["text_sequence"]).strip()
        original_ctc_loss_weight, model.ctc_loss_weight = model.ctc_loss_weight, 0.0
        rollouts = generate_rows_ref(model, audio_chunk[:1], 4, temperature=1.0, margins=margins)
        texts = [tokenizer.decode(q).strip() for q in rollouts]
        rewards = reward_fn(teacher_text, texts)
        decision = 'update'
        if sum(rewards) / len(rewards) > 0.95:
            decision = 'early_exit'
        elif all(r == 0.0 for r in rewards) or all(r == rewards[0] for r in rewards):
            decision = 'skipping'
        else:
            ids = [tokenizer.encode(t) for t in texts]
            kw = dict(success_threshold=maxrl_success_threshold) if mode == 'maxrl' else dict(normalize_std=grpo_normalize_std)
            loss = rl_loss_ref(model, audio_chunk[:1], ids, rewards, mode, **kw)
            if loss is None:
                decision = 'maxrl_skip'
            else:
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
        model.ctc_loss_weight = original_ctc_loss_weight
        if trace is not None:
            trace.append((rollouts, list(rewards), decision))
    model.eval()
    final_out = enc_dec_inference_ref(model, spec, seq_len, 0, tokenizer)
    updated = [p.clone().detach() for p in model.ordered_parameters()]
    with torch.no_grad():
        for p, po in zip(model.ordered_parameters(), original):
            p.copy_(po)
    return final_out, updated
