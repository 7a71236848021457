"""References for the CohereAsr tests: a torch restatement (any dtype, CPU) of the decoder of transformers' modeling_cohere_asr.py over
precomputed cross keys | values (the float64 reference of csrc/seq2seq_step.hip and, in fp32, the measure of its bounds), random decoder
weights for the kernel tests, the transformers pair on parakeet_refs.TOY, transformers' greedy decode with the smallest top-2 gap of its
decisions, and the test-side oracle of cohere_asr_lib.dynamic_eval_seq2seq_loss on transformers' model and torch.optim.Adam.

The issue's toy encoder (64 wide, 32 subsampling channels) is one parakeet_model.make_config refuses (widths 256 / 512 / 768 / 1024,
the LayerNorm kernels' C % 256 == 0): the pair uses parakeet_refs.TOY (2 layers x 256, 4 heads), the encoder of every sibling test."""
import random

import torch

import parakeet_refs as PR

EPS = 1e-5
START, PAD, EOS = 4, 2, 3
# configurations A and B of the model tests: the decoder over the TOY encoder
DEC_A = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=40, max_position_embeddings=64)
DEC_B = dict(hidden_size=1024, num_hidden_layers=1, num_attention_heads=8, intermediate_size=4096, vocab_size=1030, max_position_embeddings=64)
LAYER_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "encoder_attn.q_proj", "encoder_attn.k_proj",
                 "encoder_attn.v_proj", "encoder_attn.o_proj", "mlp.fc1", "mlp.fc2")
LAYER_NORMS = ("input_layernorm", "post_attention_layernorm", "final_layernorm")


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------- the decoder, any dtype
def decoder_params(d, ff, vocab, layers, max_positions, seed):
    """Random fp32 decoder weights under transformers' names without the `model.decoder.` prefix (`proj_out.*` as it is): O(1)
    activations everywhere (weights ~ N(0, 1 / K), norm weights around 1, embeddings ~ N(0, 1))."""
    g = gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                                      # noqa: E731
    p = {"embed_tokens.weight": rn(vocab, d), "pos_emb.weight": 0.5 * rn(max_positions, d)}
    for n in ("embedding_layernorm", "norm"):
        p[n + ".weight"], p[n + ".bias"] = 1.0 + 0.1 * rn(d), 0.1 * rn(d)
    for l in range(layers):
        for n in LAYER_NORMS:
            p[f"layers.{l}.{n}.weight"], p[f"layers.{l}.{n}.bias"] = 1.0 + 0.1 * rn(d), 0.1 * rn(d)
        for n in LAYER_LINEARS:
            N, K = (ff, d) if n == "mlp.fc1" else ((d, ff) if n == "mlp.fc2" else (d, d))
            p[f"layers.{l}.{n}.weight"], p[f"layers.{l}.{n}.bias"] = rn(N, K) / K ** 0.5, 0.1 * rn(N)
    p["proj_out.weight"], p["proj_out.bias"] = rn(vocab, d) / d ** 0.5, 0.1 * rn(vocab)
    return p


def cross_kv(layers, rows, n_enc, d, seed, gain=1.0):
    """Random precomputed cross keys | values, per layer [rows, n_enc, 2d]."""
    g = gen(seed + 1000)
    return [gain * torch.randn(rows, n_enc, 2 * d, generator=g) for _ in range(layers)]


def decoder_of(state_dict):
    """transformers' state dict -> decoder_params' naming."""
    out = {k[len("model.decoder."):]: v for k, v in state_dict.items() if k.startswith("model.decoder.")}
    out.update({k: v for k, v in state_dict.items() if k.startswith("proj_out.")})
    return out


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) * w + b


def _attend(q, k, v, heads, causal):
    """q [R, S, d], k / v [R, Tk, d] -> [R, S, d]; softmax(q k^T / sqrt(hd)) v per head."""
    R, S, d = q.shape
    hd = d // heads
    sp = lambda t: t.reshape(R, t.shape[1], heads, hd).transpose(1, 2)                                # noqa: E731
    s = sp(q) @ sp(k).transpose(2, 3) / hd ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(S, k.shape[1], dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(R, S, d)


def decoder_ref(p, ids, ckv, heads, dtype=torch.float64):
    """The decoder over ids [R, S] and the precomputed cross keys | values ckv (per layer [R, n_enc, 2d]) in `dtype`: causal, so position t
    of the result is what the cached one-token step at t computes.  Returns (logits [R, S, V], cache rows per layer [R, S, 3d] = q | k | v
    of every position, x0 [R, S, d] = the residual stream after the embedding LayerNorm)."""
    p = {k: v.to(dtype) for k, v in p.items()}
    ids = torch.as_tensor(ids).long()
    R, S = ids.shape
    d = p["embed_tokens.weight"].shape[1]
    lin = lambda x, n: x @ p[n + ".weight"].T + p[n + ".bias"]                                        # noqa: E731
    x0 = _ln(p["embed_tokens.weight"][ids] + p["pos_emb.weight"][:S], p["embedding_layernorm.weight"], p["embedding_layernorm.bias"])
    x, rows = x0, []
    for l in range(len(ckv)):
        q = f"layers.{l}."
        n1 = _ln(x, p[q + "input_layernorm.weight"], p[q + "input_layernorm.bias"])
        qq, kk, vv = (lin(n1, q + f"self_attn.{c}_proj") for c in "qkv")
        rows.append(torch.cat([qq, kk, vv], -1))
        x = x + lin(_attend(qq, kk, vv, heads, True), q + "self_attn.o_proj")
        n2 = _ln(x, p[q + "post_attention_layernorm.weight"], p[q + "post_attention_layernorm.bias"])
        kv = ckv[l].to(dtype)
        x = x + lin(_attend(lin(n2, q + "encoder_attn.q_proj"), kv[..., :d], kv[..., d:], heads, False), q + "encoder_attn.o_proj")
        n3 = _ln(x, p[q + "final_layernorm.weight"], p[q + "final_layernorm.bias"])
        x = x + lin(torch.relu(lin(n3, q + "mlp.fc1")), q + "mlp.fc2")
    return lin(_ln(x, p["norm.weight"], p["norm.bias"]), "proj_out"), rows, x0


def cross_kv_of(p, enc, layers, dtype=torch.float64):
    """The cross keys | values of encoder states enc [R, T', H_enc]: `proj`, then every layer's k_proj | v_proj."""
    p = {k: v.to(dtype) for k, v in p.items()}
    mem = enc.to(dtype) @ p["proj.weight"].T + p["proj.bias"]
    return [torch.cat([mem @ p[f"layers.{l}.encoder_attn.{c}_proj.weight"].T + p[f"layers.{l}.encoder_attn.{c}_proj.bias"] for c in "kv"], -1)
            for l in range(layers)]


def step_tol(want32, want64):
    """tests/test_decoder_step_kernels_gpu.py's recipe: 4 x the error of the same function in fp32 on the CPU + 2e-5 * max(1, max |want|)."""
    e32 = (want32.double() - want64).abs().max().item()
    return 4.0 * e32 + 2e-5 * max(1.0, want64.abs().max().item()), e32


# ----------------------------------------------------------------------------------------------------------- the transformers pair
def hf_config(dec=DEC_A, arch=PR.TOY, **over):
    from transformers import CohereAsrConfig
    kw = dict(pad_token_id=PAD, eos_token_id=EOS, bos_token_id=START, decoder_start_token_id=START, encoder_config=dict(arch))
    kw.update(dec)
    kw.update(over)
    return CohereAsrConfig(**kw)


def hf_model(dec=DEC_A, seed=0, gain=1.0, arch=PR.TOY, **over):
    """transformers' CohereAsrForConditionalGeneration in eval mode, one-dimensional parameters and the batch norms' running statistics
    randomised as parakeet_refs.hf_model does.  `gain` multiplies embed_tokens, pos_emb and proj_out.weight (the decode tests: with
    transformers' initialisation, std 0.02, every decision is a near tie)."""
    from transformers import CohereAsrForConditionalGeneration
    torch.manual_seed(seed)
    cfg = hf_config(dec, arch, **over)
    ref = CohereAsrForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
        d = ref.model.decoder
        for w in (d.embed_tokens.weight, d.pos_emb.weight, ref.proj_out.weight):
            w.mul_(gain)
    return cfg, ref


# (model seed, forced prompt per row) of the decode tests, gain 8, found by a seeded scan on the CPU (tests/test_cohere_asr_cpu.py
# re-checks them): seed 5 rows end at steps 10 / 11 / 11 (cut before max_new_tokens, pad fill on row 0), seed 6 at 3 / 3 / never, seed 9
# with the 3-token prompts at never / never / 2; smallest top-2 gaps 0.027, 0.050, 0.037 at max |logit| about 8.  The rows hardly depend
# on the audio with random weights, so every row gets its own prompt token.
P2 = [[START, 7], [START, 11], [START, 23]]
P3 = [[START, 7, 9], [START, 11, 30], [START, 23, 5]]
DECODE_CASES = [(5, P2), (6, P2), (9, P3)]


def feats(B=3, T=67, seed=1):
    return torch.randn(B, T, PR.TOY["num_mel_bins"], generator=gen(seed))


def hf_generate(ref, x, prompt, max_new_tokens=16):
    """transformers' greedy decode from the forced prompt [B, P] (start token first) -> (ids [B, P + n], the smallest top-2 logit gap over
    every decision of a live row, recomputed teacher-forced in fp32)."""
    with torch.no_grad():
        seq = ref.generate(input_features=x, decoder_input_ids=prompt, do_sample=False, max_new_tokens=max_new_tokens)
        P = prompt.shape[1]
        assert torch.equal(seq[:, :P], prompt), "transformers changed the forced prompt (it must start with decoder_start_token_id)"
        gap = float("inf")
        if seq.shape[1] > P:
            logits = ref(input_features=x, decoder_input_ids=seq[:, :-1]).logits
            for b in range(seq.shape[0]):
                for t in range(P - 1, seq.shape[1] - 1):
                    top = logits[b, t].topk(2).values
                    assert int(logits[b, t].argmax()) == int(seq[b, t + 1]), "the teacher-forced replay disagrees with generate"
                    gap = min(gap, float(top[0] - top[1]))
                    if int(seq[b, t + 1]) == ref.config.eos_token_id:
                        break
    return seq, gap


# ----------------------------------------------------------------------------------------------------------- the loop's oracle
LOOP = dict(seq_len=128, num_negatives=2, lr_args={'lr': 1e-5}, T=256, spec_seed=8, mask_seed=5, max_new_tokens=8, model_seed=12)     # seed 12: six tokens, then eos; gap 0.18


def loop_inputs():
    spec = torch.randn(1, PR.TOY["num_mel_bins"], LOOP["T"], generator=gen(LOOP["spec_seed"]))
    return spec, PR.Tokenizer(DEC_A["vocab_size"])


def dynamic_eval_seq2seq_ref(args, model, spec, seq_len, overlap, tokenizer, num_negatives, lr_args, spec_augment_config=PR.SPEC_AUGMENT,
                             generator=None, prompt=(START,), max_new_tokens=8, freeze_decoder=True, out=None):
    """cohere_asr_lib.dynamic_eval_seq2seq_loss restated on transformers' model (CPU): per window SpecAugment on the first num_negatives
    copies, one grad-mode encoder pass of all copies, transformers' generate on the clean copy's encoder states from the forced prompt,
    the text hop, the model's own loss (labels -100 under the prompt, ids, eos) on the augmented copies, torch Adam on everything but
    the subsampling, the decoder and proj_out.  Returns the per-window pseudo-labels {start: ids}; `out` collects the logits of a probe
    after the last step, the smallest top-2 gap of the decodes and the number of optimiser steps."""
    from dynamic_asr_eval_amd.augment import SpecAugment
    from oracle.dynamic_eval_ref import apply_masks
    spec_n = spec.shape[-1]
    factor = 8
    original = [p.clone().detach() for p in model.parameters()]
    augmentation = SpecAugment(**spec_augment_config)
    model.eval()
    frozen = []
    for part in (model.model.encoder.subsampling,) + ((model.model.decoder, model.proj_out) if freeze_decoder else ()):
        for p in part.parameters():
            frozen.append((p, p.requires_grad))
            p.requires_grad = False
    optimizer = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], **lr_args)
    if seq_len > spec_n:
        seq_len, overlap = spec_n, 0
    assert overlap % factor == 0
    last_ulen, kill_next, training_data = None, False, {}
    for i in range(0, spec_n, seq_len - overlap):
        chunk = spec[:, :, i:i + seq_len]
        u_len = chunk.shape[-1]
        if kill_next:
            break
        elif last_ulen is not None and u_len < last_ulen:
            kill_next = True
        last_ulen = u_len
        training_data[i] = chunk
    prompt = [int(t) for t in prompt]
    P = len(prompt)
    windows, steps, gap = {}, 0, float("inf")
    for epoch in range(args.__dict__.get('epochs', 1)):
        windows = {}
        keys = list(training_data.keys())
        keys = random.sample(keys, len(keys)) if args.__dict__.get('shuffle', False) else keys
        for i in keys:
            chunk = training_data[i].clone().repeat(num_negatives + 1, 1, 1)
            for j in range(num_negatives):
                apply_masks(chunk[j], augmentation.draw(chunk.shape[1], chunk.shape[2], generator), augmentation.zero_masking)
            eo = model.model.encoder(chunk.transpose(1, 2))
            enc = eo.last_hidden_state                                                                   # [n + 1, T', H]
            with torch.no_grad():
                clean = type(eo)(last_hidden_state=enc[-1:].detach())
                seq = model.generate(encoder_outputs=clean, decoder_input_ids=torch.tensor([prompt]), do_sample=False, max_new_tokens=max_new_tokens)
                if seq.shape[1] > P:
                    lg = model(encoder_outputs=clean, decoder_input_ids=seq[:, :-1]).logits[0]
                    for t in range(P - 1, seq.shape[1] - 1):
                        top = lg[t].topk(2).values
                        gap = min(gap, float(top[0] - top[1]))
                        if int(seq[0, t + 1]) == EOS:
                            break
            toks = [int(t) for t in seq[0, P:].tolist() if int(t) not in (EOS, PAD)]
            windows[i] = toks
            ids = tokenizer.text_to_ids(tokenizer.ids_to_text(toks))
            optimizer.zero_grad()
            if not ids:
                continue
            dec_in = torch.tensor([prompt + ids] * num_negatives)
            labels = torch.tensor([[-100] * (P - 1) + ids + [EOS]] * num_negatives)
            loss = model(encoder_outputs=type(eo)(last_hidden_state=enc[:num_negatives]), decoder_input_ids=dec_in, labels=labels).loss
            if torch.isfinite(loss):
                loss.backward()
                optimizer.step()
                steps += 1
    if out is not None:
        with torch.no_grad():
            x, dec_in = out["probe"]
            out["logits"] = model(input_features=x, decoder_input_ids=dec_in).logits
        out["gap"], out["steps"] = gap, steps
    with torch.no_grad():
        for p, p_orig in zip(model.parameters(), original):
            p.copy_(p_orig)
    for p, rg in frozen:
        p.requires_grad = rg
    model.zero_grad()
    return windows
