"""References for the Nemotron3_5AsrForRNNT tests: plain torch restatements of the prompt-fusion kernels (csrc/prompt_fuse.hip) in the dtype
of their inputs (float64: the reference; float32: the yardstick of kernel_refs.measured_tol), and the transformers Nemotron3_5AsrConfig /
Nemotron3_5AsrForRNNT pair at toy size with its forward, decode, streaming and loop cases, on the pattern of tests/nemotron_refs.py."""
import copy

import torch

import nemotron_refs as NR
import nemotron_stream_refs as SR
import rnnt_refs as R

VOCAB, BLANK, TOY = NR.VOCAB, NR.BLANK, NR.TOY
NUM_PROMPTS, PROMPT_I, DEFAULT_PROMPT = 8, 96, 5
PROMPTS_A, PROMPTS_B = [1, 5, 1], [6, 5, 3]          # A: a duplicated id and the default; B': rows 0 and 2 change, row 1 does not


# ----------------------------------------------------------------------------------------------------------- the kernels
def gather(b1, w1p, ids):
    """pb [B, I] = b1 + the column ids[b] of w1p [I, Np]."""
    return b1[None, :] + w1p[:, ids].t()


def fused_fwd(z, pb):
    return torch.relu(z + pb[:, None, :])


def fused_bwd(a, da, ids, Np):
    """(dz, s [B, I], db1 [I], dW1p [I, Np]) of the forward from its OUTPUT a (mask a > 0), sums in the dtype of da."""
    dz = da * (a > 0).to(da.dtype)
    s = dz.sum(1)
    dw = torch.zeros(a.shape[2], Np, dtype=da.dtype)
    for b, p in enumerate(ids):
        dw[:, p] += s[b]
    return dz, s, s.sum(0), dw


def concat_form(h, w1, b1, ids, Np):
    """transformers' own form: linear_1 on cat([h, one_hot]) -> the pre-activation [B, T, I]."""
    one_hot = torch.nn.functional.one_hot(torch.as_tensor(ids), num_classes=Np).to(h.dtype)[:, None, :].expand(-1, h.shape[1], -1)
    return torch.nn.functional.linear(torch.cat([h, one_hot], -1), w1, b1)


# ----------------------------------------------------------------------------------------------------------- the transformers pair
def hf_config(arch=TOY, vocab=VOCAB, hidden=64, layers=2, **over):
    from transformers import Nemotron3_5AsrConfig
    kw = dict(num_prompts=NUM_PROMPTS, prompt_intermediate_size=PROMPT_I, default_prompt_id=DEFAULT_PROMPT)
    kw.update(over)
    return Nemotron3_5AsrConfig(vocab_size=vocab, decoder_hidden_size=hidden, num_decoder_layers=layers, blank_token_id=vocab - 1,
                                encoder_config=dict(arch), **kw)


def hf_model(seed=0, blank_bias=0.0, head_gain=1.0, sub_gain=1.0, emb_gain=1.0, dec_gain=1.0, prompt_gain=1.0, out_gain=1.0, arch=TOY, **kw):
    """transformers' Nemotron3_5AsrForRNNT in eval mode, randomised by nemotron_refs.hf_model's recipe with two more gains: the prompt
    columns of prompt_projector.linear_1.weight times `prompt_gain` (so that a language moves the states by more than rounding), and
    prompt_projector.linear_2.weight times `out_gain`."""
    from transformers import Nemotron3_5AsrForRNNT
    torch.manual_seed(seed)
    cfg = hf_config(arch=arch, **kw)
    ref = Nemotron3_5AsrForRNNT(cfg).eval()
    H = cfg.encoder_config.hidden_size
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        for n, p in ref.named_parameters():
            if n.startswith("encoder.subsampling.") and n.endswith("weight"):
                p.mul_(sub_gain)
        ref.decoder.embedding.weight.mul_(emb_gain)
        ref.decoder.decoder_projector.weight.mul_(dec_gain)
        ref.joint.head.weight.mul_(head_gain)
        ref.joint.head.bias[cfg.blank_token_id] += blank_bias
        ref.prompt_projector.linear_1.weight[:, H:] *= prompt_gain
        ref.prompt_projector.linear_2.weight *= out_gain
    ref.generation_config.decoder_start_token_id = cfg.blank_token_id        # unset in the config: generate() starts from the blank
    return cfg, ref


def ids_tensor(prompt_ids):
    return None if prompt_ids is None else torch.as_tensor(prompt_ids, dtype=torch.long)


def min_pre_relu(ref, x, prompt_ids, num_lookahead_tokens=None):
    """The smallest |z| over the pre-activations of prompt_projector.linear_1 on features x: how far an fp32 difference is from flipping a
    ReLU mask."""
    with torch.no_grad():
        h = ref.encoder(input_features=x, num_lookahead_tokens=num_lookahead_tokens).last_hidden_state
        pl = ref.prompt_projector.linear_1
        return concat_form(h, pl.weight, pl.bias, prompt_ids, ref.config.num_prompts).abs().min().item()


def hf_encode(ref, x, prompt_ids, num_lookahead_tokens=None):
    with torch.no_grad():
        return ref.get_audio_features(input_features=x, prompt_ids=ids_tensor(prompt_ids), num_lookahead_tokens=num_lookahead_tokens).pooler_output


def hf_greedy(ref, feats, prompt_ids):
    """rnnt_refs.hf_greedy with the languages handed to transformers' generate."""
    cfg = ref.config
    with torch.no_grad():
        out = ref.generate(input_features=feats, prompt_ids=ids_tensor(prompt_ids))
    seq, dur = out.sequences[:, 1:], out.durations[:, 1:]
    Tp = int(ref.encoder._get_subsampling_output_length(torch.tensor([feats.shape[1]])).item())
    rows = []
    for b in range(feats.shape[0]):
        toks, frames, steps, t = [], [], [], 0
        for s in range(seq.shape[1]):
            if t >= Tp:
                break
            k, d = int(seq[b, s]), int(dur[b, s])
            steps.append((k, d, t))
            if k != cfg.blank_token_id:
                toks.append(k)
                frames.append(t)
            t += d
        rows.append(dict(tokens=toks, frames=frames, steps=steps, finished=t >= Tp))
    return rows, Tp


def hf_margins(ref, feats, rows, prompt_ids):
    """rnnt_refs.hf_margins on the states of `prompt_ids`: the smallest top-2 margin over the steps, from a step-by-step replay that must
    take the same steps."""
    cfg = ref.config
    margins = []
    with torch.no_grad():
        enc = hf_encode(ref, feats, prompt_ids)
        for b, row in enumerate(rows):
            _, _, steps = R.greedy_steps_torch(enc[b], ref.decoder.embedding, ref.decoder.lstm, ref.decoder.decoder_projector, ref.joint.head,
                                               cfg.blank_token_id, R.start_token(ref), cfg.max_symbols_per_step, len(row["steps"]),
                                               lambda lg: margins.append(float(lg.topk(2).values.diff().abs())))
            assert steps == row["steps"], (b, steps, row["steps"])
    return min(margins)


def hf_stream_encode(ref, x, lookahead, prompt_ids, dtype=torch.float64):
    """transformers' get_audio_features driven chunk by chunk with its own caches and the languages `prompt_ids` on x [B, T, F], in
    `dtype` -> the projected encoder states [B, T', Hd], one chunk's after the other."""
    m = copy.deepcopy(ref).to(dtype).eval()
    sw = m.config.encoder_config.sliding_window
    pkv = pc = None
    outs = []
    with torch.no_grad():
        for ch in SR.chunks_of(x.to(dtype), sw, lookahead):
            out = m.get_audio_features(input_features=ch, use_cache=True, past_key_values=pkv, padding_cache=pc, num_lookahead_tokens=lookahead,
                                       prompt_ids=ids_tensor(prompt_ids))
            pkv, pc = out.past_key_values, out.padding_cache
            outs.append(out.pooler_output)
    return torch.cat(outs, 1)


# ----------------------------------------------------------------------------------------------------------- the committed cases
# Forward / backward: model seed 2 with the prompt columns times 10.  Measured on the CPU at T = 131, lookahead 2, labels seed 5 (U = 4,
# all non-blank), "mean_volume": the loss gradient of linear_1.weight's prompt columns has its largest entry 4.6e-3 at column 1 and
# 2.2e-3 at column 5 and is exactly 0 at the other six; the smallest pre-ReLU |z| is 6.0e-4; the projected states of PROMPTS_A and
# PROMPTS_B differ by 1.8e-2, 0 and 3.3e-2 on the three rows (max |enc| 0.30).
MODEL = dict(seed=2, prompt_gain=10.0)
MIN_PRE_RELU = 1e-4
# Decode: found by a seeded search on the CPU over seeds 0-9 x blank bias x head gain x out gain, in that order, until transformers'
# decode alone satisfied rnnt_refs.assert_decode_conditions under PROMPTS_A.
DECODE = dict(seed=7, blank_bias=8.0, head_gain=100.0, sub_gain=12.0, emb_gain=30.0, dec_gain=30.0, max_symbols_per_step=3, prompt_gain=10.0,
              out_gain=4.0)
LOOP_PROMPT = 3                                   # the loop runs with default_prompt_id set to a language that is not the configuration's
# Two windows (128 and 96 frames at overlap 64), the decode model; spectrogram seeds searched from 0 on the CPU until the oracle's smallest
# top-2 margin under LOOP_PROMPT was >= 1e-2: seed 0, margin 9.6e-2, 33 non-blank and 19 blank steps.
LOOP = dict(R.LOOP, T=160, spec_seed=0)


def loop_inputs():
    import parakeet_refs
    spec = torch.randn(1, TOY["num_mel_bins"], LOOP["T"], generator=torch.Generator().manual_seed(LOOP["spec_seed"]))
    return spec, parakeet_refs.Tokenizer(VOCAB - 1)


def decode_model():
    return hf_model(**DECODE)


def decode_case(B, prompt_ids, ref=None):
    """(rows of hf_greedy, T', the smallest top-2 margin) of the decode model on the first B rows of nemotron_refs.decode_feats(3)."""
    ref = decode_model()[1] if ref is None else ref
    x = NR.decode_feats(B)
    rows, Tp = hf_greedy(ref, x, prompt_ids[:B])
    return rows, Tp, hf_margins(ref, x, rows, prompt_ids[:B])
