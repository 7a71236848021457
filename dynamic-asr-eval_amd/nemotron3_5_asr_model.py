"""Nemotron3_5AsrForRNNT on MI355X: the multilingual sibling of NemotronAsrStreamingForRNNT, `nvidia/nemotron-3.5-asr-streaming-0.6b`
(`model_type: "nemotron3_5_asr"`, transformers modeling_nemotron3_5_asr.py), as transformers builds it in plain torch.

A subclass of NemotronAsrStreamingForRNNT (nemotron_asr_streaming_model.py): the cache-aware FastConformer encoder, `encoder_projector`, the
LSTM prediction network, the joint, the RNN-T loss, backward(), the greedy decode and the streaming session are the parent's, unchanged.
The one thing that is new sits between the encoder's last hidden states h [B, T', H] and `encoder_projector`: language-ID conditioning
through `prompt_projector`,
    fused = linear_2(relu(linear_1(cat([h, one_hot(prompt_id)[:, None, :].expand(T')], -1))))          linear_1 [I, H + Np], linear_2 [H, I]
(released sizes H = 1024, Np = 128, I = 2048).  The concat form is never run.  Since
    linear_1(cat([h, onehot(p_b)])) = h W1[:, :H]^T + (b1 + W1[:, H + p_b]),
the main block is an ordinary K = H product on the GEMM and the prompt is a per-batch-row bias of I floats (csrc/prompt_fuse.hip):
  forward   z = h W1h^T (no bias); pb = ops.prompt_bias_gather; a = ops.prompt_relu(z, pb) in place; fused = linear_2(a); encoder_projector.
  backward  encoder_projector and linear_2 by the existing GEMM paths; ops.prompt_relu_bwd: dz in place over da, db1, and dW1p as a
            fixed-order segment sum over the batch rows grouped by prompt id (a column of a prompt no row used stays exactly zero);
            the main block's weight gradient rides in the backward's grouped launch, its data gradient is one GEMM.  a is kept, z is not
            (the ReLU mask is a > 0).
`prompt_projector.linear_1.weight` therefore lives as TWO flat parameters, W1h [I, H] (`...linear_1.weight.hidden`) and W1p [I, Np]
(`...linear_1.weight.prompt`), both contiguous; state_dict() / load_state_dict() / grads_hf() merge and split them, so the outside sees
transformers' one [I, H + Np] tensor (as the subsampling linear's column permutation is hidden).  named_parameters() and the optimisers
see the two parts; `frozen` prefixes match both through transformers' name.

The language: `prompt_ids=` of encode / forward / generate / generate_streaming / stream is an int tensor or list [B], or one int for
every row; None means `model.default_prompt_id`, a settable attribute initialised from the configuration (no warning is printed).  That
attribute is how parakeet_tdt_lib.dynamic_eval_transducer_loss, which passes no prompt, is pointed at a language.  The ids are checked on
the host (ops.host_prompt_ids); head() and backward() take `prompt_ids` too and refuse a value that differs from the encode they continue.
The prompt projector adapts in the loop (`frozen_in_the_loop` is the parent's) and counts as the encoder's side for _encoder_frozen().

Streaming: `model.stream(batch_size, num_lookahead_tokens=None, graph=False, prompt_ids=None)` returns a PromptStreamSession, the
parent's session plus a device int32 [B] of prompt ids and the gathered pb [B, I].  `reset(prompt_ids=None)` may change the ids in
place (None keeps them) and gathers pb again from the current weights; a captured step holds only the two addresses, so a change of
language needs no recapture.  pb is gathered at stream() and at reset(): weights adapted in between show after the next reset().

Refused by name before any launch: the Parakeet `model_type`s and "nemotron_asr_streaming" (their own modules build them), an
`encoder_config` that is not a "nemotron_asr_streaming_encoder", `num_prompts` < 1, a `prompt_intermediate_size` that is not a positive
multiple of 4, a `default_prompt_id` outside [0, num_prompts), `prompt_ids` of the wrong length or outside the table, `prompt_ids` next
to `enc=` in generate(), and what the parents refuse.  Out of scope: what the parent lists; a language name -> id table (transformers
keeps it in the processor).  No hub checkpoint is on the machine: transformers' class on the CPU with the same random state dict is
the oracle in the tests."""
import torch

from . import ops
from . import nemotron_asr_streaming_model as NM
from . import parakeet_tdt_model as TM
from .nemotron_asr_streaming_stream import StreamSession

DEFAULT_HEAD = dict(NM.DEFAULT_HEAD, vocab_size=13088, blank_token_id=13087, pad_token_id=0)
DEFAULT_PROMPT = dict(num_prompts=128, prompt_intermediate_size=2048, default_prompt_id=101)
PROMPT = "prompt_projector."
W1, B1, W2, B2 = (PROMPT + n for n in ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"))
W1H, W1P = W1 + ".hidden", W1 + ".prompt"      # the two flat parts of linear_1.weight: columns [0, H) and [H, H + Np)


def _int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def make_config(cfg=None):
    """transformers' Nemotron3_5AsrConfig (the object, or the nested dict of a config.json; None: its defaults) -> the parent's flat dict
    plus `num_prompts`, `prompt_intermediate_size` and `default_prompt_id`."""
    prompt = dict(DEFAULT_PROMPT)
    if cfg is not None:
        get = TM._getter(cfg)
        mt = get("model_type")
        if mt in NM.PARAKEET_TYPES or get("durations") is not None:
            raise ops.DynError(f"model_type={mt!r} is a Parakeet configuration, not built by this module (Nemotron3_5AsrForRNNT): "
                               "parakeet_model / parakeet_tdt_model / parakeet_rnnt_model build those")
        if mt == "nemotron_asr_streaming":
            raise ops.DynError("model_type=\"nemotron_asr_streaming\" (no prompt projector) is not built by this module "
                               "(Nemotron3_5AsrForRNNT): nemotron_asr_streaming_model.NemotronAsrStreamingForRNNT builds it")
        if mt is not None and mt != "nemotron3_5_asr":
            raise ops.DynError(f"model_type={mt!r} is not a Nemotron3_5AsrForRNNT configuration (\"nemotron3_5_asr\")")
        enc = get("encoder_config")
        emt = None if enc is None else TM._getter(enc)("model_type")
        if emt is not None and emt != "nemotron_asr_streaming_encoder":
            raise ops.DynError(f"encoder_config.model_type={emt!r} is not built: Nemotron3_5AsrForRNNT runs a \"nemotron_asr_streaming_encoder\"")
        for k in prompt:
            v = get(k)
            if v is not None:
                prompt[k] = v
    out = TM.head_config(cfg, DEFAULT_HEAD, NM.encoder_config)
    Np, I, dp = prompt["num_prompts"], prompt["prompt_intermediate_size"], prompt["default_prompt_id"]
    if not _int(Np) or Np < 1:
        raise ops.DynError(f"num_prompts={Np!r} is not built: a positive integer number of language-prompt slots")
    if not _int(I) or I < 4 or I % 4:
        raise ops.DynError(f"prompt_intermediate_size={I!r} is not built: a positive multiple of 4 (16-byte rows)")
    out.update(num_prompts=Np, prompt_intermediate_size=I, default_prompt_id=check_default_prompt(dp, Np))
    return out


def check_default_prompt(v, num_prompts):
    if not _int(v) or not 0 <= v < num_prompts:
        raise ops.DynError(f"default_prompt_id={v!r} lies outside [0, {num_prompts}) (num_prompts)")
    return v


def config_from_json(path):
    """An HF `config.json` of a nemotron3_5_asr checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def param_spec(c, pf=""):
    """transformers' state dict of Nemotron3_5AsrForRNNT: NemotronAsrStreamingForRNNT's, then `prompt_projector.linear_{1,2}`."""
    H, Np, I = c["hidden_size"], c["num_prompts"], c["prompt_intermediate_size"]
    return NM.param_spec(c, pf) + [(pf + W1, (I, H + Np), None), (pf + B1, (I,), None), (pf + W2, (H, I), None), (pf + B2, (H,), None)]


def flat_spec(c, pf=""):
    """param_spec as the flat buffers hold it: linear_1.weight as its two contiguous parts."""
    H, Np, I = c["hidden_size"], c["num_prompts"], c["prompt_intermediate_size"]
    out = []
    for n, shape, kind in param_spec(c, pf):
        out += [(pf + W1H, (I, H), None), (pf + W1P, (I, Np), None)] if n == pf + W1 else [(n, shape, kind)]
    return out


def split_w1(w, H):
    """linear_1.weight [I, H + Np] (or its gradient) -> (the hidden block [I, H], the prompt block [I, Np]), both contiguous."""
    return w[:, :H].contiguous(), w[:, H:].contiguous()


def merge_w1(hidden, prompt):
    return torch.cat([hidden, prompt], 1)


class Nemotron3_5AsrForRNNT(NM.NemotronAsrStreamingForRNNT):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(flat_spec)

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self.Np, self.I = c["num_prompts"], c["prompt_intermediate_size"]
        self._default_prompt_id = c["default_prompt_id"]
        self._prompts = None                                   # (host ids, device int32 [B]) of the encode in flight
        self._ctx_prompts = None                               # the host ids of the encode whose activations self._ctx holds

    @property
    def default_prompt_id(self):
        """The language of every call that passes no `prompt_ids`."""
        return self._default_prompt_id

    @default_prompt_id.setter
    def default_prompt_id(self, v):
        self._default_prompt_id = check_default_prompt(v, self.Np)

    def _encoder_frozen(self):
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith(("encoder.", TM.PROJ, PROMPT)))

    # ------------------------------------------------------------------ state dict: one linear_1.weight outside, two parts inside
    def _merged(self, d):
        out = {}
        for n, t in d.items():
            if n == W1H:
                out[W1] = merge_w1(t, d[W1P])
            elif n != W1P:
                out[n] = t
        return out

    def state_dict(self):
        return self._merged(super().state_dict())

    def grads_hf(self):
        return self._merged(super().grads_hf())

    def load_state_dict(self, sd, strict=True):
        if W1 in sd:
            H = self.cfg["hidden_size"]
            if tuple(sd[W1].shape) != (self.I, H + self.Np):
                raise ops.DynError(f"{W1}: shape {tuple(sd[W1].shape)} in the state dict does not fit this configuration's {(self.I, H + self.Np)}")
            sd = dict(sd)
            sd[W1H], sd[W1P] = split_w1(sd.pop(W1).to(torch.float32), H)
        return super().load_state_dict(sd, strict)

    # ------------------------------------------------------------------ the language of a call
    def _host_prompts(self, prompt_ids, B):
        return ops.host_prompt_ids(prompt_ids, B, self.Np, self._default_prompt_id)

    def _same_prompts(self, who, prompt_ids):
        if prompt_ids is not None and self._ctx_prompts is not None:
            ids = self._host_prompts(prompt_ids, len(self._ctx_prompts))
            if ids != self._ctx_prompts:
                raise ops.DynError(f"{who}(prompt_ids={ids}) continues an encode that ran with prompt_ids={self._ctx_prompts}")

    def encode(self, input_features, attention_mask=None, num_lookahead_tokens=None, prompt_ids=None, input_lengths=None, **caches):
        """The parent's encode with the language of every row (`prompt_ids`: module docstring) fused in front of `encoder_projector`."""
        NM.PM.refuse_input_lengths(type(self).__name__, input_lengths)
        self._refuse_caches(caches)
        x = input_features
        if isinstance(x, torch.Tensor) and x.dim() == 3 and x.shape[0] >= 1:      # anything else: the parent refuses it
            ids = self._host_prompts(prompt_ids, x.shape[0])
            self._prompts = (ids, torch.tensor(ids, dtype=torch.int32).to(self.device)) if x.is_cuda else None
        enc = super().encode(input_features, attention_mask, num_lookahead_tokens)
        self._ctx_prompts = self._prompts[0] if self._ctx is not None else None
        return enc

    def forward(self, input_features, decoder_input_ids=None, labels=None, attention_mask=None, reduction=None, sigma=0.0, grad_scale=1.0,
                n_active=None, label_lengths=None, frames_per_chunk=None, num_lookahead_tokens=None, prompt_ids=None, input_lengths=None,
                **caches):
        """The parent's forward with `prompt_ids`."""
        NM.PM.refuse_input_lengths(type(self).__name__, input_lengths)
        self._refuse_caches(caches)
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built: every frame of input_features is taken as valid (ragged batches are out of scope)")
        if decoder_input_ids is None:
            raise ops.DynError("forward() needs decoder_input_ids [B or 1, U + 1] (start token + labels); generate() decodes without them")
        enc = self.encode(input_features, None, num_lookahead_tokens, prompt_ids)
        out = self.head(enc, decoder_input_ids, labels, reduction, sigma, grad_scale, n_active, label_lengths, frames_per_chunk)
        out.enc = enc
        return out

    def head(self, enc, decoder_input_ids, labels=None, reduction=None, sigma=0.0, grad_scale=1.0, n_active=None, label_lengths=None,
             frames_per_chunk=None, num_lookahead_tokens=None, prompt_ids=None):
        self._same_prompts("head", prompt_ids)
        return super().head(enc, decoder_input_ids, labels, reduction, sigma, grad_scale, n_active, label_lengths, frames_per_chunk,
                            num_lookahead_tokens)

    def backward(self, grad_logits=None, n_active=None, num_lookahead_tokens=None, prompt_ids=None):
        self._same_prompts("backward", prompt_ids)
        return super().backward(grad_logits, n_active, num_lookahead_tokens)

    def generate(self, input_features=None, enc=None, num_lookahead_tokens=None, prompt_ids=None, input_lengths=None):
        """The parent's generate; the encoder pass of `input_features` runs with the languages `prompt_ids`.  Projected states `enc` are
        already fused: `prompt_ids` next to them is refused."""
        NM.PM.refuse_input_lengths(type(self).__name__, input_lengths)
        if enc is None:
            with torch.no_grad():
                keep = self._ctx, self._tdt, self._ctx_lookahead, self._ctx_prompts
                enc = self.encode(input_features, None, num_lookahead_tokens, prompt_ids)
                self._ctx, self._tdt, self._ctx_lookahead, self._ctx_prompts = keep
        elif prompt_ids is not None:
            raise ops.DynError("generate(enc=..., prompt_ids=...): the projected states already carry their language; pass prompt_ids with "
                               "input_features, or to the encode() that made `enc`")
        return super().generate(enc=enc)

    # ------------------------------------------------------------------ the prompt projector in front of encoder_projector
    def _fuse(self, x, ids_dev, pb, save):
        """x [B, T', H] -> (enc [B, T', Hd], (a, fused, ids) or None).  `pb` [B, I]: a session's gathered bias (None: gathered here)."""
        P = self.P
        z = ops.linear(x, P[W1H])                                                # the K = H block; the bias comes with the prompt
        if pb is None:
            pb = ops.prompt_bias_gather(P[B1], P[W1P], ids_dev)
        a = ops.prompt_relu(z, pb, out=z)
        f = ops.linear(a, P[W2], P[B2])
        enc = ops.linear(f, P[TM.PROJ + "weight"], P[TM.PROJ + "bias"])
        return enc, ((a, f, ids_dev) if save else None)

    def _project_enc(self, x, save):
        ids, ids_dev = self._prompts
        if len(ids) != x.shape[0]:
            raise ops.DynError(f"{len(ids)} prompt ids for {x.shape[0]} rows of encoder states")
        return self._fuse(x, ids_dev, None, save)

    def _project_enc_bwd(self, de, ctx, cut):
        P = self.P
        a, f, ids_dev = cut(ctx["project"])
        df = self._lin_bwd(de, f, TM.PROJ + "weight", TM.PROJ + "bias")
        da = self._lin_bwd(df, a, W2, B2)
        dz = ops.prompt_relu_bwd(a, da, ids_dev, self._g(B1), self._g(W1P), beta=1.0, out=da)
        if self.trainable(W1H):
            self._wgrad(dz, cut(ctx["head"]), self.G[W1H], None)
        return ops.linear_dgrad(dz, P[W1H])

    # ------------------------------------------------------------------ streaming
    def stream(self, batch_size, num_lookahead_tokens=None, graph=False, prompt_ids=None):
        """The parent's session with the languages of its streams: PromptStreamSession (`reset(prompt_ids=None)` changes them)."""
        return PromptStreamSession(self, batch_size, num_lookahead_tokens, graph, prompt_ids)

    def generate_streaming(self, input_features, num_lookahead_tokens=None, graph=False, prompt_ids=None):
        from .nemotron_asr_streaming_stream import generate_streaming
        return generate_streaming(self, input_features, num_lookahead_tokens, graph, prompt_ids=prompt_ids)


class PromptStreamSession(StreamSession):
    """StreamSession + the languages: `prompt_ids` int32 [B] and the gathered bias `pb` [B, I] on the device, allocated once; the step
    reads both through their addresses."""

    def __init__(self, model, batch_size, num_lookahead_tokens=None, graph=False, prompt_ids=None):
        ids = model._host_prompts(prompt_ids, batch_size) if _int(batch_size) and batch_size >= 1 else None     # else: the parent refuses
        super().__init__(model, batch_size, num_lookahead_tokens, graph)
        self.prompt_ids = torch.zeros(self.B, device=model.device, dtype=torch.int32)
        self.pb = torch.zeros(self.B, model.I, device=model.device, dtype=torch.float32)
        self._set_prompts(ids)

    def _set_prompts(self, ids):
        m = self.model
        if ids is not None:
            self.prompt_ids.copy_(torch.tensor(ids, dtype=torch.int32))
        with torch.no_grad():
            ops.prompt_bias_gather(m.P[B1], m.P[W1P], self.prompt_ids, out=self.pb)

    def state_bytes(self):
        return super().state_bytes() + sum(t.numel() * t.element_size() for t in (self.prompt_ids, self.pb))

    def reset(self, prompt_ids=None):
        """The parent's reset; `prompt_ids` (None: unchanged) replaces the languages in place, and pb is gathered again from the current
        weights either way.  A captured step stays valid."""
        ids = None if prompt_ids is None else self.model._host_prompts(prompt_ids, self.B)
        super().reset()
        self._set_prompts(ids)

    def _project(self, x):
        return self.model._fuse(x, self.prompt_ids, self.pb, False)[0]
