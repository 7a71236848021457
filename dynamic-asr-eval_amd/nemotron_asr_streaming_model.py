"""NemotronAsrStreamingForRNNT on MI355X: the cache-aware streaming FastConformer transducer of `nvidia/nemotron-speech-streaming-en-0.6b`
(`model_type: "nemotron_asr_streaming"`, transformers modeling_nemotron_asr_streaming.py) as transformers builds it in plain torch, run
OFFLINE under its chunked limited-context mask: what cache-aware training makes equal to streaming, and what the dynamic-evaluation
loop (parakeet_tdt_lib.dynamic_eval_transducer_loss) needs.

A subclass of ParakeetForRNNT (parakeet_rnnt_model.py): `encoder_projector`, the LSTM prediction network, the joint (whole or streamed over
frame chunks: `joint_budget`, `frames_per_chunk=`), ops.rnnt_loss with reduction "mean_volume" and label lengths counted as
`labels != blank_token_id`, backward() and the greedy decode are the parent's, as are the encoder layers' FFNs, LayerNorms, flat parameters
and the five attention products.  The class's own `loss_function` is unusable in transformers (it resolves to ForCausalLMLoss), so the
loss follows ParakeetForRNNT.  The encoder differs in three places:
  * attention: transformers applies chunked_limited_mask_function(sliding_window - 1, num_lookahead_tokens) even without an
    attention_mask.  With cs = lookahead + 1 and lc = (sliding_window - 1) // cs (unlimited when sliding_window - 1 < 0), query i sees key
    j iff 0 <= i // cs - j // cs <= lc: a contiguous key range per row, and j - i in [-dlo, dhi] (ops.chunked_band).  The position
    term is therefore a BAND: `relative_k_proj` runs on the W = dlo + dhi + 1 rows of the position table any row can touch, (q + v) P^T is
    one GEMM with N = W (97 at the released sliding_window 71 / lookahead 13, against 2T' - 1 = 511 at T' = 256), the shift, the mask and
    the softmax are one launch that writes exact zeros outside the key range (csrc/relshift_band.hip: ops.softmax_relshift_band), and
    the backward writes dS into the band's layout (ops.relshift_band_bwd): d(q + v) is a K = W product and the position table's gradient
    only has its W band rows.  The score and context GEMMs stay dense over [T', T'].
  * conv module: the depthwise conv is causal (left padding 8) with an optional bias and `conv.norm` is a LayerNorm(H), no batch-norm
    buffers: GLU, conv, bias, LayerNorm and SiLU are one launch (csrc/convmod_causal.hip: ops.convmod_causal_k9); backward by the
    existing SiLU' and LayerNorm kernels, the causal depthwise dgrad / wgrad at 9 taps and ops.colsum for the bias.
  * x8 subsampling (`encoder.subsampling.`: conv_in, layers.{0,1}.depthwise_conv / pointwise_conv, linear): every 3x3 stride-2 conv pads
    (2, 1) on both axes, one stage maps n -> n // 2 + 1, so the widths are odd (80 -> 41 -> 21 -> 11) and `num_mel_bins` need not be a
    multiple of 8 (csrc/subsample_causal.hip).  The linear's columns live in the kernels' (f, c) order, permuted in state_dict() /
    load_state_dict() / grads_hf() as parakeet_model does.
`num_lookahead_tokens=` of forward / encode / generate picks the lookahead of that call (None: `default_num_lookahead_tokens`); head() and
backward() take it too and refuse a value that differs from the encode whose activations they continue.

Streaming is a separate interface: `model.stream(batch_size, num_lookahead_tokens=None, graph=False)` returns a session that owns the K/V
rings, the conv states, the subsampling carries and the greedy decoder's state on the device (encode_chunk / push / reset), and
`generate_streaming()` drives one over a whole stream (nemotron_asr_streaming_stream.py, csrc/stream.hip); a stream is not bounded by
`max_position_embeddings`.
Refused by name before any launch: `attention_mask`; `use_cache`, `past_key_values`, `padding_cache` in the offline calls (the streaming caches
belong to a session);
`subsampling_factor` != 8, subsampling kernel != 3, stride != 2, `conv_kernel_size` != 9, `hidden_act` != "silu", a joint activation
other than relu, `hidden_size` outside 256 / 512 / 768 / 1024; a negative or non-integer lookahead, `sliding_window` = 0, T' >
`max_position_embeddings`; the `model_type` of any Parakeet head and "nemotron3_5_asr" (the multilingual sibling with a language-prompt
projector: nemotron3_5_asr_model.py builds it on this class); `sigma`; batch_renorm_training() (there is no batch norm); and what
the parents refuse of the head.
Out of scope: gradients through a streaming session; ragged batches and rows that join or leave a session; a waveform front end (since built:
feature_extractor() / generate_from_audio(), and push_audio() / flush() of a session; frontend.MelFeatures, MelStream); hipGraph
replay of the offline calls and lockstep groups; the decode inside the captured streaming step;
skipping fully masked tiles in the score and context GEMMs (the band is exploited in the position product and the softmax only).  No hub checkpoint is on the machine: transformers' class on the CPU with the same random state dict is the
oracle in the tests."""
import torch

from . import _attn, ops
from . import parakeet_model as PM
from . import parakeet_rnnt_model as RM
from . import parakeet_tdt_model as TM

ENCODER_KEYS = PM.ENCODER_KEYS + ("sliding_window", "default_num_lookahead_tokens")
DEFAULT_ENCODER = dict(PM.DEFAULT_CONFIG, sliding_window=71, default_num_lookahead_tokens=13)
DEFAULT_HEAD = dict(RM.DEFAULT_HEAD, vocab_size=1025, blank_token_id=1024, pad_token_id=0)
SUB = PM.SUB
FROZEN_IN_THE_LOOP = (SUB, TM.DEC)
PARAKEET_TYPES = ("parakeet_ctc", "parakeet_tdt", "parakeet_rnnt", "parakeet_encoder")
CACHES = ("use_cache", "past_key_values", "padding_cache")


def check_lookahead(v, what="num_lookahead_tokens"):
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ops.DynError(f"{what}={v!r} is not built: a non-negative integer number of encoder frames")
    return v


def encoder_config(cfg=None):
    """parakeet_model.make_config with the two attention-context keys and without its rule on num_mel_bins (any positive width)."""
    out = PM.make_config(cfg, DEFAULT_ENCODER, ENCODER_KEYS, mel_multiple=1)
    sw = out["sliding_window"]
    if isinstance(sw, bool) or not isinstance(sw, int) or sw == 0:
        raise ops.DynError(f"sliding_window={sw!r} is not built: a positive integer (the left attention context is sliding_window - 1 frames; "
                           "a negative one leaves the left context unlimited)")
    check_lookahead(out["default_num_lookahead_tokens"], "default_num_lookahead_tokens")
    out["max_position_embeddings"] = int(out["max_position_embeddings"])
    return out


def make_config(cfg=None):
    """transformers' NemotronAsrStreamingConfig (the object, or the nested dict of a config.json; None: its defaults) -> the flat dict the
    parents' code reads, with `durations` empty, plus `sliding_window` and `default_num_lookahead_tokens`."""
    if cfg is not None:
        get = TM._getter(cfg)
        mt = get("model_type")
        if mt in PARAKEET_TYPES or get("durations") is not None:
            raise ops.DynError(f"model_type={mt!r} is a Parakeet configuration, not built by this module (NemotronAsrStreamingForRNNT): "
                               "parakeet_model / parakeet_tdt_model / parakeet_rnnt_model build those")
        if mt == "nemotron3_5_asr":
            raise ops.DynError("model_type=\"nemotron3_5_asr\" (Nemotron3_5AsrForRNNT: this encoder and head with a language-prompt projector "
                               "in between) is not built by this module: nemotron3_5_asr_model.Nemotron3_5AsrForRNNT builds it")
        if mt is not None and mt != "nemotron_asr_streaming":
            raise ops.DynError(f"model_type={mt!r} is not a NemotronAsrStreamingForRNNT configuration (\"nemotron_asr_streaming\")")
    return TM.head_config(cfg, DEFAULT_HEAD, encoder_config)


def config_from_json(path):
    """An HF `config.json` of a nemotron_asr_streaming checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def frames(T):
    """Encoder frames of T feature frames: three causal stride-2 stages, n -> n // 2 + 1 (transformers' _get_subsampling_output_length)."""
    for _ in range(3):
        T = ops.causal_out_len(T)
    return T


def param_spec(c, pf=""):
    """transformers' state dict of NemotronAsrStreamingForRNNT: the causal subsampling under its own names, then ParakeetForRNNT's layers
    (the same names; `conv.norm` is a LayerNorm's weight and bias) and head."""
    C, H, s = c["subsampling_conv_channels"], c["hidden_size"], pf + SUB
    spec = [(s + "conv_in.weight", (C, 3, 3), "dw"), (s + "conv_in.bias", (C,), None)]
    for i in (0, 1):
        spec += [(s + f"layers.{i}.depthwise_conv.weight", (C, 3, 3), "dw"), (s + f"layers.{i}.depthwise_conv.bias", (C,), None),
                 (s + f"layers.{i}.pointwise_conv.weight", (C, C), "pw2"), (s + f"layers.{i}.pointwise_conv.bias", (C,), None)]
    spec += [(s + "linear.weight", (H, C * frames(c["num_mel_bins"])), "sublin"), (s + "linear.bias", (H,), None)]
    return spec + [e for e in RM.param_spec(c, pf) if not e[0].startswith(s)]


class NemotronAsrStreamingForRNNT(RM.ParakeetForRNNT):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    downsampling_factor = 8
    frozen_in_the_loop = FROZEN_IN_THE_LOOP
    frames = staticmethod(frames)

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        self.F3 = frames(self.cfg["num_mel_bins"])             # the frequency columns the subsampling linear reads per channel
        self._lookahead = self.cfg["default_num_lookahead_tokens"]     # of the encode in flight
        self._ctx_lookahead = None                             # of the encode whose activations self._ctx holds
        self._after_stream = False                             # a streaming session ran since the last encode(): backward() is refused

    def _make_buffers(self):
        return {}                                              # conv.norm is a LayerNorm: no running statistics

    def batch_renorm_training(self, *args, **kw):
        raise ops.DynError("batch_renorm_training() is not built for NemotronAsrStreamingForRNNT: its conv module has a LayerNorm, no batch norm")

    # ------------------------------------------------------------------ the calls that take the lookahead
    def _refuse_caches(self, kw):
        for k in CACHES:
            if kw.pop(k, None) not in (None, False):
                raise ops.DynError(f"{k} is not built here: this call is the offline forward under the chunked limited-context mask; the "
                                   "streaming caches live in a session, model.stream(batch_size) (encode_chunk / push), or generate_streaming()")
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")

    def _same_lookahead(self, who, num_lookahead_tokens):
        if num_lookahead_tokens is not None and self._ctx_lookahead is not None and check_lookahead(num_lookahead_tokens) != self._ctx_lookahead:
            raise ops.DynError(f"{who}(num_lookahead_tokens={num_lookahead_tokens}) continues an encode that ran with "
                               f"num_lookahead_tokens={self._ctx_lookahead}")

    _feature_kind = "nemotron_asr_streaming"                   # NemotronAsrStreamingFeatureExtractor: no normalisation, center=False for chunks
    _ragged = False                                            # the chunked attention mask and the causal subsampling know one length

    def encode(self, input_features, attention_mask=None, num_lookahead_tokens=None, input_lengths=None, **caches):
        """ParakeetForTDT.encode under the chunked mask of `num_lookahead_tokens` (None: the configuration's default)."""
        PM.refuse_input_lengths(type(self).__name__, input_lengths)
        self._refuse_caches(caches)
        c = self.cfg
        self._after_stream = False
        self._lookahead =c["default_num_lookahead_tokens"] if num_lookahead_tokens is None else check_lookahead(num_lookahead_tokens)
        if isinstance(input_features, torch.Tensor) and input_features.dim() == 3 and self.frames(input_features.shape[1]) > c["max_position_embeddings"]:
            raise ops.DynError(f"{self.frames(input_features.shape[1])} encoder frames exceed max_position_embeddings={c['max_position_embeddings']}")
        enc = super().encode(input_features, attention_mask)
        self._ctx_lookahead = self._lookahead if self._ctx is not None else None
        return enc

    def forward(self, input_features, decoder_input_ids=None, labels=None, attention_mask=None, reduction=None, sigma=0.0, grad_scale=1.0,
                n_active=None, label_lengths=None, frames_per_chunk=None, num_lookahead_tokens=None, input_lengths=None, **caches):
        """ParakeetForTDT.forward with `num_lookahead_tokens`."""
        PM.refuse_input_lengths(type(self).__name__, input_lengths)
        self._refuse_caches(caches)
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built: every frame of input_features is taken as valid (ragged batches are out of scope)")
        if decoder_input_ids is None:
            raise ops.DynError("forward() needs decoder_input_ids [B or 1, U + 1] (start token + labels); generate() decodes without them")
        enc = self.encode(input_features, None, num_lookahead_tokens)
        out = self.head(enc, decoder_input_ids, labels, reduction, sigma, grad_scale, n_active, label_lengths, frames_per_chunk)
        out.enc = enc
        return out

    def head(self, enc, decoder_input_ids, labels=None, reduction=None, sigma=0.0, grad_scale=1.0, n_active=None, label_lengths=None,
             frames_per_chunk=None, num_lookahead_tokens=None):
        self._same_lookahead("head", num_lookahead_tokens)
        return super().head(enc, decoder_input_ids, labels, reduction, sigma, grad_scale, n_active, label_lengths, frames_per_chunk)

    def backward(self, grad_logits=None, n_active=None, num_lookahead_tokens=None):
        if self._after_stream:
            raise ops.DynError("backward() after a streaming push / encode_chunk is not built: a session runs under no_grad and keeps no "
                               "activations (gradients through a stream are out of scope); run encode() / forward() first")
        self._same_lookahead("backward", num_lookahead_tokens)
        return super().backward(grad_logits, n_active)

    # ------------------------------------------------------------------ streaming (nemotron_asr_streaming_stream.py)
    def stream(self, batch_size, num_lookahead_tokens=None, graph=False):
        """A cache-aware streaming session of `batch_size` streams: StreamSession (first_chunk_frames, chunk_frames, encode_chunk(feats),
        push(feats), frames_seen, reset()).  graph=True replays the steady-state encoder step as one captured hipGraph."""
        from .nemotron_asr_streaming_stream import StreamSession
        return StreamSession(self, batch_size, num_lookahead_tokens, graph)

    def generate_streaming(self, input_features, num_lookahead_tokens=None, graph=False):
        """generate() chunk by chunk through a session: input_features [B, T, F] with T = first_chunk_frames + k * chunk_frames, or an
        iterable of chunks -> the same fields, concatenated over the chunks."""
        from .nemotron_asr_streaming_stream import generate_streaming
        return generate_streaming(self, input_features, num_lookahead_tokens, graph)

    def generate(self, input_features=None, enc=None, num_lookahead_tokens=None, input_lengths=None):
        """ParakeetForTDT.generate; the encoder pass of `input_features` runs under the mask of `num_lookahead_tokens`."""
        PM.refuse_input_lengths(type(self).__name__, input_lengths)
        if enc is None:
            with torch.no_grad():
                keep = self._ctx, self._tdt, self._ctx_lookahead
                enc = self.encode(input_features, None, num_lookahead_tokens)
                self._ctx, self._tdt, self._ctx_lookahead = keep
        return super().generate(enc=enc)

    def _band(self, T, lookahead):
        return ops.chunked_band(T, self.cfg["sliding_window"] - 1, lookahead)

    # ------------------------------------------------------------------ subsampling
    def _subsample(self, x):
        """x [B, T, F] -> (h [B, T', H], what _subsample_bwd needs, batch-major)."""
        P, s = self.P, SUB
        z1 = ops.conv2d_first_causal(x, P[s + "conv_in.weight"], P[s + "conv_in.bias"])                  # [B, T1, F1, C], pre-activation
        u2 = ops.dwconv2d_s2_causal_act(z1, P[s + "layers.0.depthwise_conv.weight"], P[s + "layers.0.depthwise_conv.bias"], "relu")
        z2 = ops.linear(u2, P[s + "layers.0.pointwise_conv.weight"], P[s + "layers.0.pointwise_conv.bias"])
        u3 = ops.dwconv2d_s2_causal_act(z2, P[s + "layers.1.depthwise_conv.weight"], P[s + "layers.1.depthwise_conv.bias"], "relu")
        z3 = ops.linear(u3, P[s + "layers.1.pointwise_conv.weight"], P[s + "layers.1.pointwise_conv.bias"])
        a3 = ops.relu(z3)
        B, T3, F3, C = a3.shape
        h = ops.linear(a3.view(B, T3, F3 * C), P[s + "linear.weight"], P[s + "linear.bias"])
        if self.input_scale != 1.0:                           # (W a + b) * sqrt(H), as transformers multiplies the linear's output
            raw, h = h, h.clone()
            ops.axpby(raw, h, 0.0, self.input_scale)
        return h, (x, z1, u2, z2, u3, z3, a3)

    def _subsample_bwd(self, kept, dh):
        P, G, s = self.P, self.G, SUB
        x, z1, u2, z2, u3, z3, a3 = kept
        B, T3, F3, C = a3.shape
        if self.input_scale != 1.0:
            d = dh.clone()
            ops.axpby(dh, d, 0.0, self.input_scale)
            dh = d
        da3 = self._lin_bwd(dh, a3.view(B, T3, F3 * C), s + "linear.weight", s + "linear.bias")
        dz3 = ops.relu_bwd(z3, da3.view(z3.shape), out=da3.view(z3.shape))
        du3 = self._lin_bwd(dz3, u3, s + "layers.1.pointwise_conv.weight", s + "layers.1.pointwise_conv.bias")
        ops.dwconv2d_s2_causal_wgrad_act(z2, du3, G[s + "layers.1.depthwise_conv.weight"], G[s + "layers.1.depthwise_conv.bias"], "relu", beta=1.0)
        dz2 = ops.dwconv2d_s2_causal_dgrad_act(z2, P[s + "layers.1.depthwise_conv.weight"], du3, "relu")
        du2 = self._lin_bwd(dz2, u2, s + "layers.0.pointwise_conv.weight", s + "layers.0.pointwise_conv.bias")
        ops.dwconv2d_s2_causal_wgrad_act(z1, du2, G[s + "layers.0.depthwise_conv.weight"], G[s + "layers.0.depthwise_conv.bias"], "relu", beta=1.0)
        dz1 = ops.dwconv2d_s2_causal_dgrad_act(z1, P[s + "layers.0.depthwise_conv.weight"], du2, "relu")
        ops.conv2d_first_causal_wgrad(x, dz1, G[s + "conv_in.weight"], G[s + "conv_in.bias"], beta=1.0)

    # ------------------------------------------------------------------ attention under the chunked mask
    def _attn_fwd(self, x, l, vT, tab, save):
        """x + o_proj(attn(LN(x))): Wav2Vec2ConformerForCTC._attn_fwd's relative branch with the position product and the softmax on the band."""
        c, P = self.cfg, self.P
        B, T, H = x.shape
        nh = c["num_attention_heads"]
        D = H // nh
        scale = D ** -0.5
        p = f"encoder.layers.{l}."
        band = self._band(T, self._lookahead)
        W = band.W
        n, m, s = ops.layernorm(x, P[p + "self_attn_layer_norm.weight"], P[p + "self_attn_layer_norm.bias"], self._layer_eps)
        Wqkv, bqkv = self.Pqkv[l]
        qkv = torch.empty(B, T, 3 * H, device=x.device, dtype=torch.float32)
        S = torch.empty(B, nh, T, T, device=x.device, dtype=torch.float32)
        k, v = _attn.packed(qkv, 1, D), _attn.packed(qkv, 2, D)
        ops.linear(n, Wqkv, bqkv, out=qkv)
        qu, qv = ops.head_bias_add(qkv, P[p + "self_attn.pos_bias_u"], P[p + "self_attn.pos_bias_v"], H=H, ldq=3 * H)
        pos = ops.linear(tab[band.r0:band.r0 + W], P[p + "self_attn.linear_pos.weight"])       # [W, H]: only the rows any query can reach
        _attn.scores(_attn.plain(qu, D), k, S, scale)
        BD = torch.empty(B, nh, T, W, device=x.device, dtype=torch.float32)
        ops.gemm(qv, pos, BD, trans_b=True, M=T, N=W, K=D, lda=H, ldb=H, ldc=W, nb1=B, nb2=nh, sa=(T * H, D), sb=(0, D), sc=(nh * T * W, T * W),
                 alpha=scale)
        ops.softmax_relshift_band(S, BD, band, out=S)
        O = torch.empty(B, T, H, device=x.device, dtype=torch.float32)
        _attn.context(S, v, _attn.plain(O, D))
        r = x.clone() if save else x
        ops.linear(O, P[p + "self_attn.linear_out.weight"], P[p + "self_attn.linear_out.bias"], out=r, beta=1.0)
        return r, (x, m, s, n, qkv, S, O, qu, qv, pos)

    def _attn_bwd(self, dr, kept, pos, l, nb, T, tab, vT=None):
        c, P, G = self.cfg, self.P, self.G
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        sc = D ** -0.5
        p = f"encoder.layers.{l}."
        x, m, s, n, qkv, S, O, qu, qv = kept[:9]
        band = self._band(T, self._ctx_lookahead)
        W = band.W
        Wqkv = self.Pqkv[l][0]
        gW, gb = self.Gqkv[l]
        M = nb * T
        dO = self._lin_bwd(dr, O, p + "self_attn.linear_out.weight", p + "self_attn.linear_out.bias")
        dqkv = torch.empty_like(qkv)
        (_, k, v), (_, dk, dv) = ([_attn.packed(t, j, D) for j in range(3)] for t in (qkv, dqkv))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)                # dS: exact zeros outside every row's key range, since S is zero there
        sB, sO = (nh * T * W, T * W), (T * H, D)
        dqu = torch.empty(nb, T, H, device=dr.device, dtype=torch.float32)
        _attn.grad_qk(dP, _attn.plain(qu, D), k, _attn.plain(dqu, D), dk, sc)
        dBD = ops.relshift_band_bwd(dP, band)                    # dS in the band's layout, zeros written around it
        dqv = torch.empty_like(dqu)
        ops.gemm(dBD, pos, dqv, M=T, N=D, K=W, lda=W, ldb=H, ldc=H, nb1=nb, nb2=nh, sa=sB, sb=(0, D), sc=sO, alpha=sc)
        dpos = torch.empty_like(pos)                             # the W band rows: every other row of the table's gradient is zero
        for b in range(nb):
            ops.gemm(dBD, qv, dpos, trans_a=True, M=W, N=D, K=T, lda=W, ldb=H, ldc=H, nb1=1, nb2=nh, sa=(0, T * W), sb=(0, D), sc=(0, D),
                     a_off=b * nh * T * W, b_off=b * T * H, alpha=sc, beta=0.0 if b == 0 else 1.0)
        self._wgrad(dpos, tab[band.r0:band.r0 + W], G[p + "self_attn.linear_pos.weight"], None)
        ops.head_bias_bwd(dqu, dqv, dqkv, G[p + "self_attn.pos_bias_u"], G[p + "self_attn.pos_bias_v"], beta=1.0, ldq=3 * H)
        self._wgrad(dqkv.view(M, 3 * H), n.view(M, H), gW, gb)
        dn = torch.empty_like(dr)
        ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "self_attn_layer_norm.weight"], m, s, dn, dx, G[p + "self_attn_layer_norm.weight"],
                          G[p + "self_attn_layer_norm.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    # ------------------------------------------------------------------ conv module
    def _causal_conv_spec(self, l):
        p = f"encoder.layers.{l}."
        names = tuple(p + n for n in ("norm_conv", "conv.pointwise_conv1", "conv.depthwise_conv", "conv.norm", "conv.pointwise_conv2"))
        core = lambda u, w, cb, gamma, beta, save: ops.convmod_causal_k9(u, w, cb, gamma, beta, self._layer_eps, save=save)
        return names, core, ops.silu_bwd, ops.dwconv1d_causal_k9_wgrad, ops.dwconv1d_causal_k9_dgrad

    def _conv_fwd(self, x, l, vT, save):
        """x + conv_module(x)."""
        return self._causal_conv_fwd(x, l, save)

    def _conv_bwd(self, dr, kept, l, vT):
        return self._causal_conv_bwd(dr, kept, l)
