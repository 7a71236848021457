"""CohereAsrForConditionalGeneration on MI355X: the attention encoder-decoder of `CohereLabs/cohere-transcribe-03-2026` (`model_type:
"cohere_asr"`, transformers modeling_cohere_asr.py) as transformers builds it in plain torch.  The encoder is ParakeetEncoder, here
ParakeetForCTC's (parakeet_model.py) kernel for kernel without the `ctc_head`; behind it:
  * `model.decoder.proj`: Linear(H_enc -> d) on the encoder's last hidden states (the existing GEMM), the memory of every cross-attention.
  * the decoder (CohereAsrDecoder): embed_tokens[ids] + pos_emb[positions] -> embedding_layernorm -> `num_hidden_layers` pre-LN blocks
    (input_layernorm, causal self-attention with separate biased q / k / v / o projections; post_attention_layernorm, cross-attention
    over the memory; final_layernorm, fc1 -> ReLU -> fc2) -> norm -> `proj_out` (biased, untied).  Teacher-forced over [B, S] decoder
    inputs from ops.linear, ops.layernorm, the five attention products of _attn.py, ops.relu and ops.log_softmax.  q | k | v of the
    self-attention are ONE [3d, d] product and k | v of the cross-attention one [2d, d] product: their slots are adjacent in the flat
    parameter vector (param_spec lists them side by side), so the packed matrices are views and the state dict keeps transformers'
    separate names without a merge or a split.
  * the loss: transformers' ForCausalLMLoss as this class calls it, `shift_labels = labels`: no shift, cross-entropy over labels != -100,
    averaged over their count (dyn_nll_loss on the log-softmax rows).
  * generate: the greedy decode with all state on the device.  The encoder, `decoder.proj` and the cross K | V of every layer run once
    per call through the GEMM; then chunks of one-token steps for up to 8 rows at a time through dyn_seq2seq_steps
    (csrc/seq2seq_step.hip: every weight element read once per step for all rows); the host reads the `finished` flags once per chunk.
    Output as transformers' generate(do_sample=False): [B, P + n], the forced prompt first, pad after a row's eos, cut at the longest row.
Inside the model the encoder keeps the parent's names (`encoder.*`); state_dict() / load_state_dict() / grads_hf() speak transformers'
(`model.encoder.*`), and `frozen` prefixes may be given in either form.

Refused by name before any launch: a `model_type` other than "cohere_asr", num_key_value_heads != num_attention_heads (GQA), a head_dim
other than hidden_size / heads or not a power of two in 4 .. 256, hidden_act other than "relu", hidden_size / intermediate_size not a
multiple of 256 or above 4096, tie_word_embeddings, attention_bias false, `attention_mask` / `decoder_attention_mask`, do_sample,
num_beams > 1, and whatever parakeet_model.make_config refuses of the encoder.  That last includes the released encoder's
hidden_size 1280: the package's FastConformer is built at 256 / 512 / 768 / 1024, so the released checkpoint itself does not load yet;
the decoder and the step are built and measured at the released decoder size.  Out of scope: the waveform front end (since built: feature_extractor() / generate_from_audio(), frontend.MelFeatures; rows longer than
30 s, which the extractor splits at energy-based boundaries, are refused), sampling, beam search, ragged encoder
lengths (since built: `input_lengths=` on encode / forward / generate, lengths[b] keys in row b's cross-attention; DESIGN.md, "Ragged
batches"), hipGraph replay, lockstep groups, bf16.  No hub checkpoint is on the machine: transformers' CohereAsrForConditionalGeneration on
the CPU with the same (random) state dict is the oracle in the tests."""
import ctypes
import math
from types import SimpleNamespace

import torch

from . import _attn, ops
from . import parakeet_model as PM
from ._lib import S2S_PTRS_PER_LAYER, Seq2SeqDesc, check, load

DEC, HEAD, HF_ENC = "model.decoder.", "proj_out.", "model."
# configuration_cohere_asr.py: CohereAsrConfig's fields and its _default_encoder_config_kwargs (the keys parakeet_model reads)
DEFAULT_DECODER = dict(vocab_size=16384, hidden_size=1024, num_hidden_layers=8, num_attention_heads=8, num_key_value_heads=None,
                       intermediate_size=4096, hidden_act="relu", max_position_embeddings=1024, pad_token_id=2, eos_token_id=3, bos_token_id=4,
                       attention_bias=True, decoder_start_token_id=None, tie_word_embeddings=False, head_dim=None)
DEFAULT_ENCODER = dict(hidden_size=1280, num_hidden_layers=48, num_attention_heads=8, intermediate_size=5120, hidden_act="silu",
                       attention_bias=True, convolution_bias=True, conv_kernel_size=9, subsampling_factor=8, subsampling_conv_channels=256,
                       num_mel_bins=128, subsampling_conv_kernel_size=3, subsampling_conv_stride=2, max_position_embeddings=5000,
                       scale_input=False)
FROZEN_IN_THE_LOOP = (HF_ENC + PM.SUB, DEC, HEAD)       # nvidia_ctc/lib.py:81-86: pre_encode and NeMo's `decoder`
MAX_WIDTH = 4096                                        # dyn_seq2seq_steps: K of a row projection
LN_EPS = 1e-5                                           # nn.LayerNorm's default, every norm of the decoder
MAX_ROWS = 8                                            # rows of one dyn_seq2seq_steps call


def _getter(cfg):
    return (lambda k: cfg.get(k)) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k, None))


def make_config(cfg=None):
    """transformers' CohereAsrConfig (the object, or the nested dict of a config.json; None: the released defaults) -> the flat dict this
    module reads: parakeet_model.make_config's encoder keys plus the decoder's as `dec_*`, the token ids and `vocab_size`."""
    get = _getter(cfg) if cfg is not None else (lambda k: None)
    mt = get("model_type")
    if mt is not None and mt != "cohere_asr":
        raise ops.DynError(f"model_type={mt!r} is not a CohereAsrForConditionalGeneration configuration (\"cohere_asr\")")
    d = dict(DEFAULT_DECODER)
    for k in d:
        v = get(k)
        if v is not None:
            d[k] = v
    enc = get("encoder_config")
    if enc is None or isinstance(enc, dict):
        enc = {**DEFAULT_ENCODER, **(enc or {})}
        emt = enc.pop("model_type", None)
    else:
        emt = getattr(enc, "model_type", None)
    if emt is not None and emt != "parakeet_encoder":
        raise ops.DynError(f"encoder_config.model_type={emt!r} is not built: CohereAsrForConditionalGeneration runs a \"parakeet_encoder\"")
    dd, I, nh = (d[k] for k in ("hidden_size", "intermediate_size", "num_attention_heads"))
    for name, v in (("hidden_size", dd), ("intermediate_size", I)):
        if not (isinstance(v, int) and 0 < v <= MAX_WIDTH and v % 256 == 0):
            raise ops.DynError(f"{name}={v!r} of the decoder is not built: a multiple of 256 up to {MAX_WIDTH}")
    if not (isinstance(nh, int) and nh > 0 and dd % nh == 0):
        raise ops.DynError(f"num_attention_heads={nh!r} does not divide hidden_size={dd}")
    kv = d["num_key_value_heads"]
    if kv is not None and kv != nh:
        raise ops.DynError(f"num_key_value_heads={kv} is not built: it must equal num_attention_heads={nh} (no GQA)")
    hd = d["head_dim"]
    if hd is not None and hd != dd // nh:
        raise ops.DynError(f"head_dim={hd} is not built: it must equal hidden_size / num_attention_heads = {dd // nh}")
    hd = dd // nh
    if not (4 <= hd <= 256 and hd & (hd - 1) == 0):
        raise ops.DynError(f"head_dim={hd} is not built: a power of two in 4 .. 256")
    if d["hidden_act"] != "relu":
        raise ops.DynError(f"hidden_act={d['hidden_act']!r} of the decoder is not built (\"relu\")")
    if d["tie_word_embeddings"]:
        raise ops.DynError("tie_word_embeddings=True is not built: proj_out has its own weight")
    if not d["attention_bias"]:
        raise ops.DynError("attention_bias=False is not built: the decoder's q / k / v / o projections carry biases")
    V, L, maxp = (d[k] for k in ("vocab_size", "num_hidden_layers", "max_position_embeddings"))
    if not all(isinstance(v, int) and v > 0 for v in (V, L, maxp)):
        raise ops.DynError(f"vocab_size={V!r}, num_hidden_layers={L!r}, max_position_embeddings={maxp!r} must be positive integers")
    start = d["decoder_start_token_id"] if d["decoder_start_token_id"] is not None else d["bos_token_id"]
    for name, v in (("pad_token_id", d["pad_token_id"]), ("eos_token_id", d["eos_token_id"]), ("decoder_start_token_id (or bos_token_id)", start)):
        if not (isinstance(v, int) and 0 <= v < V):
            raise ops.DynError(f"{name}={v!r} lies outside the vocabulary of {V}")
    out = PM.make_config({"encoder_config": enc, "vocab_size": V, "pad_token_id": d["pad_token_id"]})
    out.update(dec_hidden_size=dd, dec_layers=L, dec_heads=nh, dec_intermediate_size=I, dec_max_positions=maxp, eos_token_id=d["eos_token_id"],
               bos_token_id=d["bos_token_id"], decoder_start_token_id=start)
    return out


def config_from_json(path):
    """An HF `config.json` of a cohere_asr checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def hf_name(n):
    """The model's name of a parameter or buffer -> transformers': the encoder lives under `model.`."""
    return HF_ENC + n if n.startswith("encoder.") else n


def own_name(n):
    return n[len(HF_ENC):] if n.startswith(HF_ENC + "encoder.") else n


def param_spec(c):
    """[(name, shape, kind)]: the encoder's names as the parent keeps them (`encoder.*`; transformers': `model.encoder.*`, hf_name), then
    transformers' own for `model.decoder.*` and `proj_out`.  Within a layer q | k | v (and the cross-attention's k | v) stand side by
    side, weights then biases: adjacent slots, one packed matrix."""
    H, d, I, V = c["hidden_size"], c["dec_hidden_size"], c["dec_intermediate_size"], c["vocab_size"]
    spec = [s for s in PM.param_spec(c) if not s[0].startswith("ctc_head.")]
    lin = lambda p, n, m: [(p + ".weight", (n, m), None), (p + ".bias", (n,), None)]                  # noqa: E731
    ln = lambda p: [(p + ".weight", (d,), None), (p + ".bias", (d,), None)]                          # noqa: E731
    spec += [(DEC + "embed_tokens.weight", (V, d), None), (DEC + "pos_emb.weight", (c["dec_max_positions"], d), None)]
    spec += ln(DEC + "embedding_layernorm") + lin(DEC + "proj", d, H)
    for l in range(c["dec_layers"]):
        p = f"{DEC}layers.{l}."
        spec += ln(p + "input_layernorm")
        spec += [(p + f"self_attn.{n}_proj.weight", (d, d), None) for n in "qkv"] + [(p + f"self_attn.{n}_proj.bias", (d,), None) for n in "qkv"]
        spec += lin(p + "self_attn.o_proj", d, d) + ln(p + "post_attention_layernorm") + lin(p + "encoder_attn.q_proj", d, d)
        spec += [(p + f"encoder_attn.{n}_proj.weight", (d, d), None) for n in "kv"] + [(p + f"encoder_attn.{n}_proj.bias", (d,), None) for n in "kv"]
        spec += lin(p + "encoder_attn.o_proj", d, d) + ln(p + "final_layernorm") + lin(p + "mlp.fc1", I, d) + lin(p + "mlp.fc2", d, I)
    return spec + ln(DEC + "norm") + lin(HEAD[:-1], V, d)


def hf_param_shapes(c):
    """param_spec in transformers' names and shapes: {name: shape}.  The encoder's conv kernels are kept without transformers'
    singleton axes (parakeet_model.param_spec's kinds); they are put back here as ParakeetForCTC._to_hf does."""
    hf = {None: lambda s: s, "sublin": lambda s: s, "pw": lambda s: s + (1,), "pw2": lambda s: s + (1, 1), "dw": lambda s: (s[0], 1) + s[1:]}
    return {hf_name(n): tuple(hf[kind](tuple(shape))) for n, shape, kind in param_spec(c)}


def shift_tokens_right(labels, pad_token_id, decoder_start_token_id):
    """transformers' shift_tokens_right on a host tensor [B, S]: the start token, then labels[:, :-1], -100 replaced by pad."""
    labels = torch.as_tensor(labels).long()
    out = labels.new_zeros(labels.shape)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = decoder_start_token_id
    return out.masked_fill(out == -100, pad_token_id)


def host_prompt(decoder_input_ids, B, start, vocab):
    """The forced prompt of generate(): None -> [B, 1] start tokens; else an integer [B or 1, P] tensor, P >= 1, ids inside the vocabulary."""
    if decoder_input_ids is None:
        return torch.full((B, 1), int(start), dtype=torch.int64)
    t = torch.as_tensor(decoder_input_ids).detach().cpu()
    if t.dim() != 2 or t.dtype not in (torch.int32, torch.int64) or t.shape[0] not in (1, B) or t.shape[1] < 1:
        raise ops.DynError(f"decoder_input_ids must be an integer tensor [{B} or 1, P >= 1], got {tuple(t.shape)} {t.dtype}")
    t = t.long()
    if int(t.min()) < 0 or int(t.max()) >= vocab:
        raise ops.DynError(f"decoder_input_ids: ids must lie in [0, {vocab})")
    return t.expand(B, -1).contiguous()


def finish_sequences(tokens, P, eos, pad):
    """What transformers' greedy loop returns from the device token buffer [B, P + n] (host int64): everything after a row's first eos
    behind the prompt is pad, and the rows are cut where the longest one ends."""
    tokens = tokens.clone()
    B, N = tokens.shape
    longest = P
    for b in range(B):
        hits = (tokens[b, P:] == eos).nonzero()
        end = N if hits.numel() == 0 else P + int(hits[0]) + 1
        tokens[b, end:] = pad
        longest = max(longest, end)
    return tokens[:, :longest]


class CohereAsrForConditionalGeneration(PM.ParakeetForCTC):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(lambda c, pf="": param_spec(c))
    frozen_in_the_loop = FROZEN_IN_THE_LOOP
    greedy_chunk = 16                                    # decode steps queued per host call; the finished flags are read once per chunk
    _feature_kind = "cohere_asr"                         # CohereAsrFeatureExtractor (frontend.MelFeatures): dither, rows of at most 30 s

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self.d, self.I, self.nh, self.V, self.L = (c[k] for k in ("dec_hidden_size", "dec_intermediate_size", "dec_heads", "vocab_size", "dec_layers"))
        self.hd = self.d // self.nh
        self.pad, self.eos, self.start_token = c["pad_token_id"], c["eos_token_id"], c["decoder_start_token_id"]
        self._dec = None
        d = self.d

        def pack(first, last, n):                            # the adjacent slots first .. last as one [n d, d] matrix / [n d] bias, (P, G) each
            out = []
            for leaf, shape in (("weight", (n * d, d)), ("bias", (n * d,))):
                o = self._slots[f"{first}.{leaf}"][0]
                assert self._slots[f"{last}.{leaf}"][0] == o + (n - 1) * math.prod(shape) // n
                out.append(tuple(f[o:o + math.prod(shape)].view(shape) for f in (self.flat_params, self.flat_grads)))
            return out
        self._qkv, self._ckv = [], []
        for l in range(self.L):
            p = f"{DEC}layers.{l}."
            self._qkv.append(pack(p + "self_attn.q_proj", p + "self_attn.v_proj", 3))
            self._ckv.append(pack(p + "encoder_attn.k_proj", p + "encoder_attn.v_proj", 2))

    def __call__(self, x=None, **kw):
        return self.forward(kw.pop(self._input, x), **kw)

    def trainable(self, name):
        name = getattr(self, "_alias", {}).get(name, name)
        fz = tuple(self.frozen)
        return not (fz and (name.startswith(fz) or hf_name(name).startswith(fz)))

    def _decoder_frozen(self):
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith((DEC, HEAD)))

    def _encoder_frozen(self):
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith("encoder."))

    # ------------------------------------------------------------------ state dict: transformers' names outside
    def state_dict(self):
        return {hf_name(n): t for n, t in super().state_dict().items()}

    def grads_hf(self):
        return {hf_name(n): t for n, t in super().grads_hf().items()}

    def load_state_dict(self, sd, strict=True):
        res = super().load_state_dict({own_name(k): v for k, v in sd.items()}, strict)
        return SimpleNamespace(missing_keys=[hf_name(k) for k in res.missing_keys], unexpected_keys=[hf_name(k) for k in res.unexpected_keys])

    # ------------------------------------------------------------------ encoder
    def _encode(self, h, ctx, vT, dims, v0):
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        if ctx is not None:
            ctx["head"] = x
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(x=x, frames=T)

    def encode(self, input_features, input_lengths=None):
        """input_features [B, T, num_mel_bins] -> the encoder's last hidden states [B, T', H_enc].  In grad mode its activations are kept.
        `input_lengths` (ParakeetForCTC.forward): the valid frames per row of a ragged batch; head() and generate() given this call's
        result find the rows' encoder frame counts themselves (else `enc_lengths=`): row b's cross-attention sees lengths[b] keys."""
        self._dec = None
        out = PM.ParakeetForCTC.forward(self, input_features, None, *(() if input_lengths is None else (input_lengths,)))
        self._remember_lengths(out.x, out)
        return out.x

    # ------------------------------------------------------------------ decoder, teacher-forced
    def _kv_view(self, kv, j):
        """Keys (j = 0) or values (j = 1) of a packed cross projection [B, T', 2d]."""
        return _attn.View(kv, j * self.d, 2 * self.d, kv.shape[-2] * 2 * self.d, self.hd)

    def _attend(self, q, k, v, B, Tq, Tk, causal, klens=None):
        """softmax(q k^T / sqrt(hd)) v per head on Views -> (O [B, Tq, d], the probabilities [B, nh, Tq, Tk]).  `klens` (int32 [B] on the
        device): row b has klens[b] keys, probability 0 past them (so the backward needs no mask: dS = P * (..) is 0 there, and with it
        the padded keys' dk and dv)."""
        Pm = torch.empty(B, self.nh, Tq, Tk, device=self.device, dtype=torch.float32)
        _attn.scores(q, k, Pm, 1.0 / math.sqrt(self.hd))
        if causal:
            check(load().dyn_causal_mask(Pm.data_ptr(), B * self.nh, Tq, torch.cuda.current_stream().cuda_stream), "dyn_causal_mask")
        ops.softmax(Pm, out=Pm, lens=klens)
        O = torch.empty(B, Tq, self.d, device=self.device, dtype=torch.float32)
        _attn.context(Pm, v, _attn.plain(O, self.hd))
        return O, Pm

    def _attend_bwd(self, dO, Pm, q, k, v, dq, dk, dv):
        dP = torch.empty_like(Pm)
        _attn.grad_v_dP(Pm, _attn.plain(dO, self.hd), v, dv, dP)
        ops.softmax_bwd(Pm, dP, out=dP, scale=1.0)
        _attn.grad_qk(dP, q, k, dq, dk, 1.0 / math.sqrt(self.hd))

    def _embed(self, ids):
        """ids int64 host [B, S] -> (embedding_layernorm(embed_tokens[ids] + pos_emb[0 .. S)) [B, S, d], what its backward needs)."""
        P, d = self.P, self.d
        B, S = ids.shape
        ids_dev = ids.to(torch.int32).contiguous().view(-1).to(self.device)
        e = torch.empty(B, S, d, device=self.device, dtype=torch.float32)
        check(load().dyn_embedding_fwd(ids_dev.data_ptr(), P[DEC + "embed_tokens.weight"].data_ptr(), P[DEC + "pos_emb.weight"].data_ptr(),
                                       e.data_ptr(), B * S, d, self.V, S, torch.cuda.current_stream().cuda_stream), "dyn_embedding_fwd")
        x, m, r = ops.layernorm(e, P[DEC + "embedding_layernorm.weight"], P[DEC + "embedding_layernorm.bias"], LN_EPS)
        return x, (ids, e, m, r)

    def _decoder_fwd(self, ids, mem, save, klens=None):
        """ids int64 host [B, S], mem [B, T', d] -> (logits [B, S, V], the saved activations or None); `klens`: the rows' valid frames of mem."""
        P, d, hd = self.P, self.d, self.hd
        B, S = ids.shape
        Tk = mem.shape[1]
        x, emb = self._embed(ids)
        layers = []
        for l in range(self.L):
            p = f"{DEC}layers.{l}."
            (Wqkv, _), (bqkv, _) = self._qkv[l]
            (Wkv, _), (bkv, _) = self._ckv[l]
            n1, m1, r1 = ops.layernorm(x, P[p + "input_layernorm.weight"], P[p + "input_layernorm.bias"], LN_EPS)
            qkv = ops.linear(n1, Wqkv, bqkv)
            o1, P1 = self._attend(_attn.packed(qkv, 0, hd), _attn.packed(qkv, 1, hd), _attn.packed(qkv, 2, hd), B, S, S, True)
            x1 = ops.linear(o1, P[p + "self_attn.o_proj.weight"], P[p + "self_attn.o_proj.bias"], beta=1.0, residual=x)
            n2, m2, r2 = ops.layernorm(x1, P[p + "post_attention_layernorm.weight"], P[p + "post_attention_layernorm.bias"], LN_EPS)
            q2 = ops.linear(n2, P[p + "encoder_attn.q_proj.weight"], P[p + "encoder_attn.q_proj.bias"])
            kv = ops.linear(mem, Wkv, bkv)
            o2, P2 = self._attend(_attn.plain(q2, hd), self._kv_view(kv, 0), self._kv_view(kv, 1), B, S, Tk, False, klens)
            x2 = ops.linear(o2, P[p + "encoder_attn.o_proj.weight"], P[p + "encoder_attn.o_proj.bias"], beta=1.0, residual=x1)
            n3, m3, r3 = ops.layernorm(x2, P[p + "final_layernorm.weight"], P[p + "final_layernorm.bias"], LN_EPS)
            u = ops.linear(n3, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])
            a = ops.relu(u)
            x3 = ops.linear(a, P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"], beta=1.0, residual=x2)
            if save:
                layers.append(dict(x=x, n1=n1, m1=m1, r1=r1, qkv=qkv, P1=P1, o1=o1, x1=x1, n2=n2, m2=m2, r2=r2, q2=q2, kv=kv, P2=P2, o2=o2, x2=x2,
                                   n3=n3, m3=m3, r3=r3, u=u, a=a))
            x = x3
        nf, mf, rf = ops.layernorm(x, P[DEC + "norm.weight"], P[DEC + "norm.bias"], LN_EPS)
        logits = ops.linear(nf, P[HEAD + "weight"], P[HEAD + "bias"])
        return logits, (dict(emb=emb, layers=layers, final=(x, nf, mf, rf), mem=mem) if save else None)

    def _dec_wgrad(self, dy, x, dw, db):
        """Every weight-gradient product of the decoder, `decoder.proj` and `proj_out` goes through here (a frozen decoder never calls it)."""
        self._wgrad(dy, x, dw, db)

    def _dec_lin_bwd(self, dy, x, wname, bname, packed=None, need_dx=True):
        """Backward of a decoder linear: its weight and bias gradients unless both are frozen, and the data gradient.  `packed`:
        ((W, dW), (b, db)) of a packed projection whose first member is `wname`."""
        (W, dW), (_, db) = packed if packed is not None else ((self.P[wname], self.G[wname]), (None, self.G[bname]))
        if self.trainable(wname) or self.trainable(bname):
            self._dec_wgrad(dy, x, dW, db)
        return ops.linear_dgrad(dy, W) if need_dx else None

    def _decoder_bwd(self, dlogits, saved, need_mem):
        """dL/dlogits [B, S, V] -> every decoder gradient accumulated; returns dL/dmem [B, T', d] (None unless need_mem)."""
        P, d, hd = self.P, self.d, self.hd
        g = self._g
        x, nf, mf, rf = saved["final"]
        mem = saved["mem"]
        B, S, _ = x.shape
        dn = self._dec_lin_bwd(dlogits, nf, HEAD + "weight", HEAD + "bias")
        dx = torch.empty_like(x)
        ops.layernorm_bwd(x, P[DEC + "norm.weight"], mf, rf, dn, dx, g(DEC + "norm.weight"), g(DEC + "norm.bias"), dx_beta=0.0)
        dmem = torch.zeros_like(mem) if need_mem else None
        for l in reversed(range(self.L)):
            p = f"{DEC}layers.{l}."
            c = saved["layers"][l]
            da = self._dec_lin_bwd(dx, c["a"], p + "mlp.fc2.weight", p + "mlp.fc2.bias")
            du = ops.relu_bwd(c["u"], da)
            dn3 = self._dec_lin_bwd(du, c["n3"], p + "mlp.fc1.weight", p + "mlp.fc1.bias")
            dx2 = torch.empty_like(dx)
            ops.layernorm_bwd(c["x2"], P[p + "final_layernorm.weight"], c["m3"], c["r3"], dn3, dx2, g(p + "final_layernorm.weight"),
                              g(p + "final_layernorm.bias"), dx_beta=1.0, dx_in=dx)
            # cross-attention
            do2 = self._dec_lin_bwd(dx2, c["o2"], p + "encoder_attn.o_proj.weight", p + "encoder_attn.o_proj.bias")
            dq2, dkv, kv = torch.empty_like(c["q2"]), torch.empty_like(c["kv"]), c["kv"]
            self._attend_bwd(do2, c["P2"], _attn.plain(c["q2"], hd), self._kv_view(kv, 0), self._kv_view(kv, 1), _attn.plain(dq2, hd),
                             self._kv_view(dkv, 0), self._kv_view(dkv, 1))
            self._dec_lin_bwd(dkv, mem, p + "encoder_attn.k_proj.weight", p + "encoder_attn.k_proj.bias", self._ckv[l], need_dx=False)
            if need_mem:                                     # every layer's share of dL/dmem is added up in place
                ops.linear_dgrad(dkv, self._ckv[l][0][0], out=dmem, beta=1.0)
            dn2 = self._dec_lin_bwd(dq2, c["n2"], p + "encoder_attn.q_proj.weight", p + "encoder_attn.q_proj.bias")
            dx1 = torch.empty_like(dx)
            ops.layernorm_bwd(c["x1"], P[p + "post_attention_layernorm.weight"], c["m2"], c["r2"], dn2, dx1, g(p + "post_attention_layernorm.weight"),
                              g(p + "post_attention_layernorm.bias"), dx_beta=1.0, dx_in=dx2)
            # causal self-attention
            do1 = self._dec_lin_bwd(dx1, c["o1"], p + "self_attn.o_proj.weight", p + "self_attn.o_proj.bias")
            qkv, dqkv = c["qkv"], torch.empty_like(c["qkv"])
            self._attend_bwd(do1, c["P1"], _attn.packed(qkv, 0, hd), _attn.packed(qkv, 1, hd), _attn.packed(qkv, 2, hd), _attn.packed(dqkv, 0, hd),
                             _attn.packed(dqkv, 1, hd), _attn.packed(dqkv, 2, hd))
            dn1 = self._dec_lin_bwd(dqkv, c["n1"], p + "self_attn.q_proj.weight", p + "self_attn.q_proj.bias", self._qkv[l])
            dx = torch.empty_like(dx)
            ops.layernorm_bwd(c["x"], P[p + "input_layernorm.weight"], c["m1"], c["r1"], dn1, dx, g(p + "input_layernorm.weight"),
                              g(p + "input_layernorm.bias"), dx_beta=1.0, dx_in=dx1)
        ids, e, m, r = saved["emb"]
        tn, pn = DEC + "embed_tokens.weight", DEC + "pos_emb.weight"
        if self.trainable(tn) or self.trainable(pn) or self.trainable(DEC + "embedding_layernorm.weight"):
            de = torch.empty_like(e)
            ops.layernorm_bwd(e, P[DEC + "embedding_layernorm.weight"], m, r, dx, de, g(DEC + "embedding_layernorm.weight"),
                              g(DEC + "embedding_layernorm.bias"), dx_beta=0.0)
            st = torch.cuda.current_stream().cuda_stream
            if self.trainable(tn):                          # nn.Embedding(padding_idx = pad): the pad row receives no gradient (-1 matches no row)
                tid = ids.masked_fill(ids == self.pad, -1).to(torch.int32).contiguous().view(-1).to(self.device)
                check(load().dyn_embedding_bwd(tid.data_ptr(), de.data_ptr(), self.G[tn].data_ptr(), B * S, d, self.V, 1.0, st), "dyn_embedding_bwd")
            if self.trainable(pn):
                pid = torch.arange(S, dtype=torch.int32).repeat(B).to(self.device)
                check(load().dyn_embedding_bwd(pid.data_ptr(), de.data_ptr(), self.G[pn].data_ptr(), B * S, d, self.cfg["dec_max_positions"], 1.0, st),
                      "dyn_embedding_bwd")
        return dmem

    # ------------------------------------------------------------------ forward / backward
    def _ids(self, t, what, rows, allow_ignore=False):
        t = torch.as_tensor(t).detach().cpu()
        if t.dim() != 2 or t.dtype not in (torch.int32, torch.int64) or t.shape[0] not in (1, rows) or t.shape[1] < 1:
            raise ops.DynError(f"{what} must be an integer tensor [{rows} or 1, S >= 1], got {tuple(t.shape)} {t.dtype}")
        t = t.long()
        bad = (t < 0) | (t >= self.V)
        if allow_ignore:
            bad &= t != -100
        if bool(bad.any()):
            raise ops.DynError(f"{what}: ids must lie in [0, {self.V})" + (" or be -100" if allow_ignore else ""))
        return t.expand(rows, -1).contiguous()

    def forward(self, input_features, decoder_input_ids=None, labels=None, n_active=None, attention_mask=None, decoder_attention_mask=None,
                input_lengths=None):
        """The teacher-forced pass (`input_lengths`: encode()): input_features [B, T, num_mel_bins] float32 on the device, decoder_input_ids [n or 1, S] (one row: shared
        by the batch), labels [same rows, S] with -100 for positions outside the loss; n = n_active (default B): the decoder runs on the
        first n rows.  `labels` without `decoder_input_ids` means shift_tokens_right(labels, pad, decoder_start).  Returns
        SimpleNamespace(logits [n, S, V], loss [1] or None, encoder_last_hidden_state [B, T', H_enc], frames = T').  In grad mode the
        loss's gradient is kept for backward()."""
        if attention_mask is not None or decoder_attention_mask is not None:
            raise ops.DynError("attention_mask / decoder_attention_mask are not built: every frame and every decoder position is taken as valid "
                               "(a ragged batch passes input_lengths)")
        if decoder_input_ids is None and labels is None:
            raise ops.DynError("forward() needs decoder_input_ids [B or 1, S] or labels; generate() decodes without them")
        out = self.head(self.encode(input_features, input_lengths), decoder_input_ids, labels, n_active)
        if input_lengths is not None:
            out.lengths, out.lengths_device = self._enc_lengths[1:]
        return out

    def head(self, x, decoder_input_ids=None, labels=None, n_active=None, enc_lengths=None):
        """forward() behind the encoder: `decoder.proj`, the decoder and the loss on the first n_active rows of the encoder states x
        [B, T', H_enc] of the last encode() (the loop encodes all copies once, decodes the clean one and scores the others)."""
        if decoder_input_ids is None and labels is None:
            raise ops.DynError("head() needs decoder_input_ids [B or 1, S] or labels")
        B = x.shape[0]
        nb = B if n_active is None else int(n_active)
        if not 1 <= nb <= B:
            raise ops.DynError(f"n_active={n_active!r} must lie in 1 .. {B}")
        lab = None if labels is None else self._ids(labels, "labels", nb, allow_ignore=True)
        ids = self._ids(decoder_input_ids, "decoder_input_ids", nb) if decoder_input_ids is not None else \
            shift_tokens_right(lab, self.pad, self.start_token)
        S = ids.shape[1]
        if lab is not None and lab.shape[1] != S:
            raise ops.DynError(f"labels {tuple(lab.shape)} must have decoder_input_ids' {S} positions")
        if S > self.cfg["dec_max_positions"]:
            raise ops.DynError(f"{S} decoder positions exceed max_position_embeddings={self.cfg['dec_max_positions']}")
        grad_mode = torch.is_grad_enabled() and self._ctx is not None
        P = self.P
        klens = self._lengths_of(x, enc_lengths, nb)
        with ops.use_workspace(self._scratch()):
            xe = x[:nb].contiguous()
            mem = ops.linear(xe, P[DEC + "proj.weight"], P[DEC + "proj.bias"])
            logits, saved = self._decoder_fwd(ids, mem, grad_mode, klens)
            loss = dlogits = None
            if lab is not None:
                count = int((lab != -100).sum())
                if count == 0:
                    raise ops.DynError("labels hold no position inside the loss (all -100): the mean over their count is undefined")
                logp = ops.log_softmax(logits.view(nb * S, self.V))
                tg = lab.to(torch.int32).view(-1).to(self.device)
                loss = torch.empty(1, device=self.device, dtype=torch.float32)
                row_loss = torch.empty(nb * S, device=self.device, dtype=torch.float32)
                dlogits = torch.empty(nb, S, self.V, device=self.device, dtype=torch.float32) if grad_mode else None
                check(load().dyn_nll_loss(logp.data_ptr(), tg.data_ptr(), loss.data_ptr(), row_loss.data_ptr(), 0 if dlogits is None else dlogits.data_ptr(),
                                          nb * S, self.V, -100, 1.0 / count, torch.cuda.current_stream().cuda_stream), "dyn_nll_loss")
                loss = loss / count
        self._dec = dict(saved=saved, rows=nb, xe=xe, dlogits=dlogits, shape=tuple(logits.shape)) if grad_mode else None
        return SimpleNamespace(logits=logits, loss=loss, encoder_last_hidden_state=x, frames=x.shape[1])

    def backward(self, grad_logits=None, n_active=None):
        """Accumulates every parameter's gradient into flat_grads: of the loss of the last grad-mode forward with labels, or of
        sum(grad_logits * logits) for a given grad_logits [n, S, V]; through `decoder.proj` into the encoder."""
        t = self._dec
        if t is None:
            raise ops.DynError("backward() without a grad-mode forward through the decoder")
        if n_active is not None and int(n_active) != t["rows"]:
            raise ops.DynError(f"backward(n_active={n_active}) after a forward whose decoder ran on {t['rows']} rows")
        g = t["dlogits"] if grad_logits is None else grad_logits
        if g is None:
            raise ops.DynError("backward() needs grad_logits: the last forward had no labels")
        if tuple(g.shape) != t["shape"]:
            raise ops.DynError(f"grad_logits {tuple(g.shape)} does not fit the logits {t['shape']}")
        t["g"] = g.contiguous()
        B = self._ctx["dims"][0]
        nb = B if self._ctx_brn else t["rows"]          # batch renorm: the gradient reaches every row through the batch statistics
        try:                                            # the decoder's gradient waits in self._dec; the placeholder only carries nb
            super().backward(torch.empty(nb, 0, device=self.device), None if nb == B else nb)
        finally:
            self._dec = None

    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        t, P = self._dec, self.P
        v0, vT = ctx["valid"]
        T = ctx["dims"][2]
        rows = t["rows"]
        need_enc = not self._encoder_frozen()
        need_mem = need_enc or self.trainable(DEC + "proj.weight") or self.trainable(DEC + "proj.bias")
        if self._decoder_frozen() and not need_mem:
            return None
        dmem = self._decoder_bwd(t["g"], t["saved"], need_mem)
        if not need_mem:
            return None
        dx = self._dec_lin_bwd(dmem, t["xe"], DEC + "proj.weight", DEC + "proj.bias", need_dx=need_enc)
        if not need_enc:
            return None
        if rows < nb:                                    # batch renorm: zero gradient rows for the copies the loss did not see
            full = torch.zeros(nb, T, dx.shape[-1], device=self.device, dtype=torch.float32)
            full[:rows] = dx
            dx = full
        lens = ctx.get("lens")
        if lens is not None:                             # a ragged batch: no gradient enters at a padded frame (decoder.proj's bias rows)
            vT, lens = vT.cut(nb), lens[:, :nb]
            dx = ops.mask_rows_lens(dx.contiguous(), lens[3])
        dh = self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
        if not self._below_frozen():
            self._subsample_bwd(cut(ctx["sub"]), dh, *(() if lens is None else (lens,)))
        return None

    # ------------------------------------------------------------------ greedy decode
    def _step_desc(self, kv, cache, tokens, finished, logits, scratch, rows, n_enc, cap):
        """dyn_seq2seq_desc of one group of rows (include/dyneval.h): returns (descriptor, the host pointer array it points into)."""
        P, c = self.P, self.cfg
        names = ("input_layernorm.weight", "input_layernorm.bias", None, None, "self_attn.o_proj.weight", "self_attn.o_proj.bias",
                 "post_attention_layernorm.weight", "post_attention_layernorm.bias", "encoder_attn.q_proj.weight", "encoder_attn.q_proj.bias",
                 "encoder_attn.o_proj.weight", "encoder_attn.o_proj.bias", "final_layernorm.weight", "final_layernorm.bias", "mlp.fc1.weight",
                 "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
        ptrs = (ctypes.c_void_p * (self.L * S2S_PTRS_PER_LAYER))()
        for l in range(self.L):
            o = l * S2S_PTRS_PER_LAYER
            for i, nm in enumerate(names):
                if nm is not None:
                    ptrs[o + i] = P[f"{DEC}layers.{l}.{nm}"].data_ptr()
            ptrs[o + 2], ptrs[o + 3] = self._qkv[l][0][0].data_ptr(), self._qkv[l][1][0].data_ptr()
            ptrs[o + 18], ptrs[o + 19] = cache[l].data_ptr(), kv[l].data_ptr()
        d = Seq2SeqDesc(d_model=self.d, heads=self.nh, d_ff=self.I, vocab=self.V, layers=self.L, n_enc=int(n_enc),
                        max_positions=c["dec_max_positions"], rows=int(rows), pad_id=self.pad, eos_id=self.eos, eps=LN_EPS,
                        embed=P[DEC + "embed_tokens.weight"].data_ptr(), pos_emb=P[DEC + "pos_emb.weight"].data_ptr(),
                        emb_ln_w=P[DEC + "embedding_layernorm.weight"].data_ptr(), emb_ln_b=P[DEC + "embedding_layernorm.bias"].data_ptr(),
                        norm_w=P[DEC + "norm.weight"].data_ptr(), norm_b=P[DEC + "norm.bias"].data_ptr(), head_w=P[HEAD + "weight"].data_ptr(),
                        head_b=P[HEAD + "bias"].data_ptr(), layer_ptrs=ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)),
                        tokens=tokens.data_ptr(), finished=finished.data_ptr(), logits=logits.data_ptr(), scratch=scratch.data_ptr(),
                        scratch_floats=scratch.numel(), token_stride=tokens.shape[1], cache_stride=cap * 3 * self.d,
                        cross_stride=int(n_enc) * 2 * self.d)
        return d, ptrs

    def generate(self, input_features=None, decoder_input_ids=None, max_new_tokens=64, encoder_hidden_states=None, do_sample=False, num_beams=1,
                 attention_mask=None, decoder_attention_mask=None, input_lengths=None, enc_lengths=None):
        """Greedy decode of input_features [B, T, num_mel_bins] (or of encoder states `encoder_hidden_states` [B, T', H_enc]) -> int64 host
        tensor [B, P + n] as transformers' generate(do_sample=False): `decoder_input_ids` [B or 1, P] is the whole forced prompt, start
        token included (None: the start token alone); a row that emitted eos is pad afterwards; cut at the longest row.  A ragged batch:
        `input_lengths` with input_features, `enc_lengths` with encoder_hidden_states; row b's step attends to its own encoder frames
        (dyn_seq2seq_steps_len), so it emits what it emits decoded alone."""
        if do_sample or (num_beams is not None and int(num_beams) > 1):
            raise ops.DynError("do_sample / num_beams > 1 are not built: generate() is the greedy decode")
        if attention_mask is not None or decoder_attention_mask is not None:
            raise ops.DynError("attention_mask / decoder_attention_mask are not built: every frame and every decoder position is taken as valid")
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
            raise ops.DynError(f"max_new_tokens={max_new_tokens!r} must be a positive integer")
        c, P, d = self.cfg, self.P, self.d
        with torch.no_grad():
            if encoder_hidden_states is None:
                keep = self._ctx, self._dec
                x = self.encode(input_features, input_lengths)
                self._ctx, self._dec = keep
            else:
                if input_lengths is not None:
                    raise ops.DynError("generate(encoder_hidden_states=..., input_lengths=...): input_lengths counts feature frames; pass "
                                       "enc_lengths with encoder states")
                x = encoder_hidden_states
            klens = self._lengths_of(x, enc_lengths, x.shape[0])
            x = x.detach().contiguous()
            B, Tk, _ = x.shape
            prompt = host_prompt(decoder_input_ids, B, self.start_token, self.V)
            Pn = prompt.shape[1]
            cap = Pn + max_new_tokens - 1                                # positions run: the last one fills slot P + max_new_tokens - 1
            if cap > c["dec_max_positions"]:
                raise ops.DynError(f"prompt of {Pn} + max_new_tokens={max_new_tokens} needs {cap} positions, max_position_embeddings is "
                                   f"{c['dec_max_positions']}")
            new = lambda *shape: torch.empty(*shape, device=self.device, dtype=torch.float32)          # noqa: E731
            st = torch.cuda.current_stream().cuda_stream
            per_row = int(load().dyn_seq2seq_row_scratch_floats(d, self.I, self.nh))
            out = torch.empty(B, cap + 1, dtype=torch.int64)
            with ops.use_workspace(self._scratch()):
                mem = ops.linear(x, P[DEC + "proj.weight"], P[DEC + "proj.bias"])
                for r0 in range(0, B, MAX_ROWS):
                    R = min(MAX_ROWS, B - r0)
                    kv = [ops.linear(mem[r0:r0 + R], self._ckv[l][0][0], self._ckv[l][1][0]) for l in range(self.L)]     # [R, T', 2d]
                    cache = [new(R, cap, 3 * d) for _ in range(self.L)]
                    tokens = torch.full((R, cap + 1), self.pad, dtype=torch.int32)
                    tokens[:, :Pn] = prompt[r0:r0 + R].to(torch.int32)
                    tokens = tokens.to(self.device)
                    finished = torch.zeros(R, dtype=torch.int32, device=self.device)
                    logits, scratch = new(R, self.V), new(R, per_row)
                    desc, keep_ptrs = self._step_desc(kv, cache, tokens, finished, logits, scratch, R, Tk, cap)
                    t = 0
                    while t < cap:
                        n = min(self.greedy_chunk, cap - t)
                        if klens is None:
                            check(load().dyn_seq2seq_steps(ctypes.byref(desc), t, n, Pn, st), "dyn_seq2seq_steps")
                        else:
                            check(load().dyn_seq2seq_steps_len(ctypes.byref(desc), klens[r0:r0 + R].data_ptr(), t, n, Pn, st), "dyn_seq2seq_steps_len")
                        t += n
                        if t >= Pn and bool(finished.all()):             # the one host read of the chunk
                            break
                    got = tokens.cpu().long()
                    got[:, t + 1:] = self.pad                            # slots behind the last step run were never written
                    out[r0:r0 + R] = got
                    del keep_ptrs
        return finish_sequences(out, Pn, self.eos, self.pad)
