"""References for the NemotronAsrStreamingForRNNT tests: plain torch restatements, in the dtype of their inputs (float64: the reference;
float32: the yardstick of kernel_refs.measured_tol), of the three things its encoder does differently from Parakeet's: the softmax of
the Transformer-XL score under the chunked limited-context mask (written from the mask formula, with autograd for the gradient), the
causal 3x3 stride-2 subsampling stages and the conv module's core.  Then the transformers NemotronAsrStreamingConfig /
NemotronAsrStreamingForRNNT pair at toy size and its decode and loop cases, on the pattern of tests/rnnt_refs.py."""
import torch
import torch.nn.functional as Fn

import parakeet_refs as PR
import rnnt_refs as R

# ----------------------------------------------------------------------------------------------------------- the chunked mask
def chunk_params(left_context, lookahead):
    """(cs, lc) of transformers' chunked_limited_mask_function(left_context, lookahead); lc None: unlimited."""
    cs = lookahead + 1
    return cs, (left_context // cs if left_context >= 0 else None)


def chunked_mask(T, left_context, lookahead):
    """bool [T, T]: query i sees key j iff 0 <= i // cs - j // cs <= lc."""
    cs, lc = chunk_params(left_context, lookahead)
    d = torch.arange(T)[:, None] // cs - torch.arange(T)[None, :] // cs
    return (d >= 0) & (d <= lc) if lc is not None else d >= 0


def key_range(i, T, left_context, lookahead):
    """The closed form of row i's keys: [(i // cs - lc) cs, (i // cs + 1) cs) cut to [0, T)."""
    cs, lc = chunk_params(left_context, lookahead)
    return (0 if lc is None else max(0, (i // cs - lc) * cs)), min(T, (i // cs + 1) * cs)


def band_width(left_context, lookahead):
    """W = lc cs + 2 cs - 1 relative positions whatever T is (None: unlimited left context, the band is the table)."""
    cs, lc = chunk_params(left_context, lookahead)
    return None if lc is None else lc * cs + 2 * cs - 1


def band_softmax(S, BD, mask):
    """softmax_j(S[m, i, j] + BD[m, i, T - 1 - i + j]) over the keys `mask` [T, T] leaves, 0 elsewhere; S [M, T, T], BD [M, T, 2T - 1]
    (the FULL position product).  Differentiable."""
    M, T, _ = S.shape
    idx = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]).expand(M, T, T)
    x = (S + torch.gather(BD, 2, idx)).masked_fill(~mask, float("-inf"))
    return torch.softmax(x, -1)


def band_softmax_grads(S, BD, mask, dY, dtype):
    """(y, dS, dBD [M, T, 2T - 1]) of band_softmax in `dtype` for the output gradient dY."""
    s, b = S.to(dtype).clone().requires_grad_(), BD.to(dtype).clone().requires_grad_()
    y = band_softmax(s, b, mask)
    (y * dY.to(dtype)).sum().backward()
    return y.detach(), s.grad, b.grad


# ----------------------------------------------------------------------------------------------------------- causal subsampling stages
def causal_conv(x, w, bias, groups):
    """NemotronAsrStreamingEncoderCausalConv2D.forward on NCHW: pad (2, 1) in frequency and in time, then the 3x3 stride-2 convolution."""
    return Fn.conv2d(Fn.pad(x, (2, 1, 2, 1)), w, bias, stride=2, groups=groups)


def stem(x, w, bias):
    """x [B, T, F], w [C, 3, 3] -> z [B, To, Fo, C] channels-last, pre-activation."""
    return causal_conv(x[:, None], w[:, None], bias, 1).permute(0, 2, 3, 1)


def dw_stage(z, w, bias):
    """z [B, T, F, C] channels-last -> bias + causal depthwise 3x3 stride-2 of relu(z), channels-last."""
    return causal_conv(torch.relu(z).permute(0, 3, 1, 2), w[:, None], bias, w.shape[0]).permute(0, 2, 3, 1)


def grads(fn, inputs, dout, dtype):
    """(output, gradients of sum(output * dout) w.r.t. every input) of fn(*inputs) in `dtype`."""
    xs = [t.to(dtype).clone().requires_grad_() for t in inputs]
    y = fn(*xs)
    (y * dout.to(dtype)).sum().backward()
    return y.detach(), [t.grad for t in xs]


# ----------------------------------------------------------------------------------------------------------- conv-module core
def convmod_core(u, w, cbias, gamma, beta, eps=1e-5):
    """u [B, T, 2C] -> silu(LayerNorm_C(cbias + causal depthwise conv(GLU(u)))), w [C, KW], zeros left of frame 0."""
    C, KW = w.shape
    g = Fn.glu(u, dim=-1).transpose(1, 2)
    c = Fn.conv1d(Fn.pad(g, (KW - 1, 0)), w[:, None], cbias, groups=C).transpose(1, 2)
    return Fn.silu(Fn.layer_norm(c, (C,), gamma, beta, eps))


# ----------------------------------------------------------------------------------------------------------- the transformers pair
VOCAB, BLANK = R.RNNT_VOCAB, R.RNNT_BLANK
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, subsampling_conv_channels=32, num_mel_bins=80,
           sliding_window=9, default_num_lookahead_tokens=2, dropout=0.0, dropout_positions=0.0, layerdrop=0.0, activation_dropout=0.0,
           attention_dropout=0.0)


def hf_config(arch=TOY, vocab=VOCAB, hidden=64, layers=2, **over):
    from transformers import NemotronAsrStreamingConfig
    return NemotronAsrStreamingConfig(vocab_size=vocab, decoder_hidden_size=hidden, num_decoder_layers=layers, blank_token_id=vocab - 1,
                                      encoder_config=dict(arch), **over)


def hf_model(seed=0, blank_bias=0.0, head_gain=1.0, sub_gain=1.0, emb_gain=1.0, dec_gain=1.0, arch=TOY, **kw):
    """transformers' NemotronAsrStreamingForRNNT in eval mode, randomised as rnnt_refs.hf_rnnt_model does (one-dimensional parameters; the
    gains and the blank's bias give the decode tests frames that differ and argmaxes with margins)."""
    from transformers import NemotronAsrStreamingForRNNT
    torch.manual_seed(seed)
    cfg = hf_config(arch=arch, **kw)
    ref = NemotronAsrStreamingForRNNT(cfg).eval()
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
    ref.generation_config.decoder_start_token_id = cfg.blank_token_id        # unset in the config: generate() starts from the blank
    return cfg, ref


def captured_mask(ref, x, num_lookahead_tokens=None):
    """The attention mask transformers' encoder hands its layers' self_attn on features x, as bool [T', T'] (True: visible)."""
    seen = {}
    attn = ref.encoder.layers[0].self_attn
    forward = attn.forward

    def spy(*args, **kw):
        seen["mask"] = kw.get("attention_mask")
        return forward(*args, **kw)

    attn.forward = spy
    try:
        with torch.no_grad():
            ref.encoder(input_features=x, num_lookahead_tokens=num_lookahead_tokens)
    finally:
        del attn.forward
    m = seen["mask"]
    m = m if m.dtype == torch.bool else m == 0
    assert m.shape[0] == 1 or bool((m == m[:1]).all())
    return m[0, 0]


# The decode case: found by a seeded search on the CPU (seeds and gains tried in order until transformers' decode alone satisfied
# rnnt_refs.assert_decode_conditions, whose margin rule of 1e-2 is stricter than the 1e-3 asked of this case: the smallest top-2 margin
# over every decode step is 1.7e-2 at B = 3).
DECODE = dict(seed=4, blank_bias=8.0, head_gain=50.0, sub_gain=12.0, emb_gain=30.0, dec_gain=30.0, max_symbols_per_step=3)
DECODE_FEATS = dict(seed=1, T=300)
LOOP = dict(R.LOOP, T=160, spec_seed=22)    # two windows (128 and 96 frames at overlap 64); seed searched: the oracle's smallest margin is 2.9e-2


def decode_model():
    return hf_model(**DECODE)


def decode_feats(B):
    return torch.randn(3, DECODE_FEATS["T"], TOY["num_mel_bins"], generator=torch.Generator().manual_seed(DECODE_FEATS["seed"]))[:B].contiguous()


def decode_case(B, ref=None):
    """(rows of rnnt_refs.hf_greedy, T', the smallest top-2 margin) of the decode model on its first B feature rows."""
    ref = decode_model()[1] if ref is None else ref
    x = decode_feats(B)
    rows, Tp = R.hf_greedy(ref, x)
    return rows, Tp, R.hf_margins(ref, x, rows)


def loop_inputs():
    spec = torch.randn(1, TOY["num_mel_bins"], LOOP["T"], generator=torch.Generator().manual_seed(LOOP["spec_seed"]))
    return spec, PR.Tokenizer(VOCAB - 1)
