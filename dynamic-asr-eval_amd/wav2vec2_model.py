"""Wav2Vec2ForCTC on MI355X: the model the reference's wav2vec2 path loads with
`AutoModelForCTC.from_pretrained("facebook/wav2vec2-base-960h")` (reference wav2vec2/lib.py:20-23) and drives with
`model(input_values).logits` (lib.py:163,413), with explicit forward / backward on the HIP kernels only.

Architecture = HF `Wav2Vec2Config()` defaults (= base-960h: 7 strided Conv1d layers of 512 channels, GroupNorm on the
first, feature projection LN + Linear(512 -> 768), grouped positional conv (k = 128, 16 groups, weight-normed) + GELU,
12 post-LN transformer layers with 12 x 64 heads and GELU FFN 3072, lm_head 768 -> 32); `feat_extract_norm="group"`,
`do_stable_layer_norm=False`, eval mode (no dropout, no SpecAugment masking) as in the reference loop.
The other layout transformers has (wav2vec2-large-960h-lv60-self, large-robust, XLSR) is built too, the two choices independently:
`feat_extract_norm="layer"` + `conv_bias=True` (every extractor layer is conv -> + bias -> LayerNorm(C) -> GELU, the last three in one
kernel each way: ops.bias_layernorm_gelu) and `do_stable_layer_norm=True` (pre-LN encoder: x + attn(LN(x)), x + ffn(LN(x)), the
encoder's LayerNorm after the last layer).
MMS (`facebook/mms-1b-all`, `mms-300m` fine-tunes) is that stable-LN layout plus `adapter_attn_dim: 16`: a bottleneck adapter behind every
encoder layer, x + linear_2(relu(linear_1(LayerNorm(x)))) (transformers Wav2Vec2AttnAdapterLayer), one kernel forward and two backward
(ops.attn_adapter / attn_adapter_bwd); `adapter_only()` freezes everything but the adapters and lm_head, and a backward skips the weight
gradients of frozen parameters and everything below the first encoder layer when nothing there adapts.  No MMS checkpoint is on the machine:
the oracle in the tests is transformers' Wav2Vec2ForCTC on the CPU with the same random state dict.
Parameter NAMES are HF's (state_dict interchange with transformers, which is the oracle in tests); the native HBM layout
of conv kernels is [C_out][kernel][C_in] so each strided Conv1d is one implicit GEMM over overlapping rows of the
channels-last activation (ops.conv1d), converted on load / save.
Attention keeps its scores in memory: the products are _attn.py's on the packed q | k | v projection, the softmax between them is a hook
(_softmax / _softmax_bwd) a model of the family replaces (WavLM's gated relative-position bias)."""
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import _attn, _graphs, ops
from ._flat import FlatModel

DEFAULT_CONFIG = dict(
    conv_dim=(512,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), hidden_size=768,
    num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, num_conv_pos_embeddings=128,
    num_conv_pos_embedding_groups=16, vocab_size=32, layer_norm_eps=1e-5,
    adapter_attn_dim=None,    # MMS: the width A of a bottleneck adapter behind every stable-LN encoder layer (transformers Wav2Vec2AttnAdapterLayer)
)


LAYOUT_FLAGS = dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)     # the base layout
ADAPTER_EPS = 1e-5        # the adapter's nn.LayerNorm is built with torch's default eps as well
EXTRACTOR_EPS = 1e-5      # transformers builds the extractor's GroupNorm / LayerNorm with torch's default eps, not config.layer_norm_eps


def make_config(cfg=None, defaults=DEFAULT_CONFIG):
    """`defaults` (DEFAULT_CONFIG; a model of the family may add keys of its own) + LAYOUT_FLAGS overridden by `cfg` (a dict, or an object with
    those attributes such as transformers' Wav2Vec2Config); keys it does not carry keep the base value, other keys are ignored."""
    out = dict(defaults)
    out.update(LAYOUT_FLAGS)
    if cfg is not None:
        src = cfg if isinstance(cfg, dict) else cfg.__dict__
        for k in defaults:
            if k in src:
                out[k] = tuple(src[k]) if isinstance(src[k], (list, tuple)) else src[k]
        for k in LAYOUT_FLAGS:
            v = src.get(k, None) if isinstance(cfg, dict) else getattr(cfg, k, None)
            if v is not None:
                out[k] = v
    out["do_stable_layer_norm"], out["conv_bias"] = bool(out["do_stable_layer_norm"]), bool(out["conv_bias"])
    A = out.get("adapter_attn_dim", None)
    if A is not None:
        if defaults is not DEFAULT_CONFIG:
            raise ops.DynError(f"adapter_attn_dim={A!r} is not built for this model: the per-layer adapters exist for Wav2Vec2ForCTC only")
        # with the post-LN encoder transformers builds no adapter whatever the value: nothing to check there
        if out["do_stable_layer_norm"] and not (isinstance(A, int) and A % 4 == 0 and 4 <= A <= 64):
            raise ops.DynError(f"adapter_attn_dim={A!r} is not built: the adapter kernels take a multiple of 4 from 4 to 64")
    if (out["feat_extract_norm"], out["conv_bias"]) not in (("group", False), ("layer", True)):
        raise ops.DynError(f"feat_extract_norm={out['feat_extract_norm']!r} with conv_bias={out['conv_bias']} is not built: the feature "
                           "extractor is either (\"group\", conv_bias=False) or (\"layer\", conv_bias=True)")
    return out


def config_dict(cfg, keys):
    """`cfg` (None, a dict, or an object with attributes such as a transformers configuration) as a dict of those of `keys` it carries: what
    the configuration reader of a model of the family looks at before it calls make_config."""
    if cfg is None:
        return {}
    if isinstance(cfg, dict):
        return {k: cfg[k] for k in keys if cfg.get(k, None) is not None}
    return {k: getattr(cfg, k) for k in keys if getattr(cfg, k, None) is not None}


def config_from_json(path, make=make_config):
    """An HF `config.json` as plain JSON -> make_config (only DEFAULT_CONFIG's keys and the three layout flags are read, `adapter_attn_dim`
    among them: JSON null or an absent key means no adapters; `make`: the configuration reader of another model of the family)."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    known = make()
    return make({k: v for k, v in src.items() if k in known})


def _conv_to_native(w):   # HF [Cout, Cin, k] -> native [Cout, k, Cin]
    return w.permute(0, 2, 1).contiguous()


def _conv_to_hf(w):       # native [Cout, k, Cin] -> HF [Cout, Cin, k]
    return w.permute(0, 2, 1).contiguous()


WEIGHT_NORM_MAX_ROW = 6144     # dyn_weight_norm_*: kernel * C/G floats of one (out-channel) row must fit its LDS buffer (128 * 48 at base-960h)


def _wn_parts(K, cg):
    """1 where a row of the positional conv's weight fits dyn_weight_norm_*; else the smallest power of two s dividing cg with K * cg / s floats
    per row that does (2 at the large layout: 128 taps x 64 channels per group)."""
    s = 1
    while K * cg // s > WEIGHT_NORM_MAX_ROW and cg % (2 * s) == 0:
        s *= 2
    return s


def _wn_split(t, s):
    """[H, K, cg] -> [s * H, K, cg / s]: the channel slices of every row become rows of their own.  A tap's norm runs over (rows, channels), so the
    weight norm of the result is the weight norm of `t` (same terms) and existing kernels serve rows wider than their LDS buffer.  Copy only."""
    H, K, cg = t.shape
    return t.view(H, K, s, cg // s).permute(2, 0, 1, 3).contiguous().view(s * H, K, cg // s)


def _wn_join(t, s):
    sH, K, c = t.shape
    return t.view(s, sH // s, K, c).permute(1, 2, 0, 3).contiguous().view(sH // s, K, s * c)


_RELEASED = object()      # Wav2Vec2ForCTC._ctx after a bucket replay whose saved activations are owned by its graphs only


def adapter_dim(c):
    """The adapters' width, or None: transformers builds them in the stable-LN encoder's layers only."""
    return c.get("adapter_attn_dim", None) if c.get("do_stable_layer_norm", False) else None


ADAPTER_PARAMS = ("norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias")


def param_spec(c, pf="wav2vec2."):
    """[(name, shape, kind)] with HF's names (`pf`: the base model's prefix); kind "conv": a conv kernel kept as [C_out][kernel][C_in],
    "g": the weight norm's magnitudes."""
    H = c["hidden_size"]
    spec = [(pf + "masked_spec_embed", (H,), None)]
    fe = pf + "feature_extractor.conv_layers."
    cin = 1
    for i, (co, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
        spec.append((f"{fe}{i}.conv.weight", (co, k, cin), "conv"))
        if c.get("conv_bias", False):
            spec.append((f"{fe}{i}.conv.bias", (co,), None))
        if i == 0 or c.get("feat_extract_norm", "group") == "layer":
            spec += [(f"{fe}{i}.layer_norm.weight", (co,), None), (f"{fe}{i}.layer_norm.bias", (co,), None)]
        cin = co
    fp = pf + "feature_projection."
    spec += [(fp + "layer_norm.weight", (cin,), None), (fp + "layer_norm.bias", (cin,), None),
             (fp + "projection.weight", (H, cin), None), (fp + "projection.bias", (H,), None)]
    pc = pf + "encoder.pos_conv_embed.conv."
    K, G = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    spec += [(pc + "bias", (H,), None), (pc + "parametrizations.weight.original0", (K,), "g"),
             (pc + "parametrizations.weight.original1", (H, K, H // G), "conv")]
    spec += [(pf + "encoder.layer_norm.weight", (H,), None), (pf + "encoder.layer_norm.bias", (H,), None)]
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}."
        # q | k | v weights side by side in the flat buffers (then their biases): one [3H, H] projection instead of three launches
        spec += [(p + f"attention.{n}.weight", (H, H), None) for n in ("q_proj", "k_proj", "v_proj")]
        spec += [(p + f"attention.{n}.bias", (H,), None) for n in ("q_proj", "k_proj", "v_proj")]
        spec += [(p + "attention.out_proj.weight", (H, H), None), (p + "attention.out_proj.bias", (H,), None)]
        spec += [(p + "layer_norm.weight", (H,), None), (p + "layer_norm.bias", (H,), None),
                 (p + "feed_forward.intermediate_dense.weight", (c["intermediate_size"], H), None),
                 (p + "feed_forward.intermediate_dense.bias", (c["intermediate_size"],), None),
                 (p + "feed_forward.output_dense.weight", (H, c["intermediate_size"]), None),
                 (p + "feed_forward.output_dense.bias", (H,), None),
                 (p + "final_layer_norm.weight", (H,), None), (p + "final_layer_norm.bias", (H,), None)]
        A = adapter_dim(c)
        if A:                                                       # HF's order inside Wav2Vec2AttnAdapterLayer: norm, linear_1, linear_2
            ad = p + "adapter_layer."
            spec += [(ad + "norm.weight", (H,), None), (ad + "norm.bias", (H,), None), (ad + "linear_1.weight", (A, H), None),
                     (ad + "linear_1.bias", (A,), None), (ad + "linear_2.weight", (H, A), None), (ad + "linear_2.bias", (H,), None)]
    spec += [("lm_head.weight", (c["vocab_size"], H), None), ("lm_head.bias", (c["vocab_size"],), None)]
    return spec


class Wav2Vec2ForCTC(FlatModel):
    _input = "input_values"
    # what a model of the same family (wavlm_model.WavLMForCTC) replaces: the base model's parameter prefix, its configuration reader and
    # parameter list, and the two attention hooks _softmax / _softmax_bwd; a model with another encoder (wav2vec2_conformer_model) also the
    # names of the q | k | v projections inside a layer and the two encoder hooks _encode / _backward_encoder; a model with another positional
    # embedding (data2vec_audio_model) the pair _pos_embed / _pos_embed_bwd, one with another feature projection (hubert_model) _project / _project_bwd
    # a model whose layers run at another frame rate (sew_model) _project / _project_bwd and _encode / _backward_encoder around the shared
    # _post_ln_layers / _post_ln_layers_bwd and _pos_weight / _pos_weight_bwd, plus _fill_valid for its own valid-length scalar
    # a model whose layers carry other parameter names and another attention (sew_d_model) _qv_names and the pair _attention / _attention_bwd
    _prefix = "wav2vec2."
    _qkv_fmt = "attention.{}_proj"
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    _norm_weight_suffixes = ("adapter_layer.norm.weight",)       # run_wav2vec2.init_synthetic starts these around 1 too
    _conv_extractor = True       # False: a model without the waveform conv stack (wav2vec2_bert_model.py); cfg's conv_kernel / conv_stride are then frame arithmetic only

    def __init__(self, config=None, device="cuda:0"):
        self.cfg = self._make_config(config)
        c, pf = self.cfg, self._prefix
        H = c["hidden_size"]
        assert H % 256 == 0 and (not self._conv_extractor or c["conv_dim"][-1] % 256 == 0), "LayerNorm kernels need C % 256 == 0"
        self.layer_extractor = c["feat_extract_norm"] == "layer"
        self.stable_ln = c["do_stable_layer_norm"]
        self.adapter_dim = adapter_dim(c)
        if self._conv_extractor and self.layer_extractor and any(d % 256 and d not in (64, 128) for d in c["conv_dim"]):
            raise ops.DynError(f"feat_extract_norm=\"layer\" needs every conv_dim to be 64, 128 or a multiple of 256 (got {c['conv_dim']})")
        spec = self._param_spec(c, pf)
        super().__init__([(n, shape) for n, shape, _ in spec], device)
        slots = self._slots
        self._kind = {n: kind for n, _, kind in spec}
        # packed views of the attention input projections: [3H, H] weights / [3H] biases (the slots are contiguous when H % 64 == 0)
        self.packed_qkv = H % 64 == 0
        self.Pqkv, self.Gqkv = [], []
        if self.packed_qkv:
            for l in range(c["num_hidden_layers"]):
                q, v = self._qv_names(l)
                ow = slots[f"{q}.weight"][0]
                assert slots[f"{v}.weight"][0] == ow + 2 * H * H
                if f"{q}.bias" not in slots:                     # a model of the family whose projections may have no bias (parakeet_model.py)
                    self.Pqkv.append((self.flat_params[ow:ow + 3 * H * H].view(3 * H, H), None))
                    self.Gqkv.append((self.flat_grads[ow:ow + 3 * H * H].view(3 * H, H), None))
                    continue
                ob = slots[f"{q}.bias"][0]
                assert slots[f"{v}.bias"][0] == ob + 2 * H
                self.Pqkv.append((self.flat_params[ow:ow + 3 * H * H].view(3 * H, H), self.flat_params[ob:ob + 3 * H]))
                self.Gqkv.append((self.flat_grads[ow:ow + 3 * H * H].view(3 * H, H), self.flat_grads[ob:ob + 3 * H]))
        self.config = SimpleNamespace(**c)
        # hipGraph replay over LENGTH BUCKETS (see forward()): off unless a loop turns it on (wav2vec2_lib: args.use_graphs)
        self.use_graphs = False
        self.bucket_frames = 32                  # an utterance of T' frames runs in the bucket of ceil(T' / 32) * 32 frames (0.64 s of audio)
        self.graph_after = 2                     # a bucket is captured the n-th time it is seen; before that the utterance runs unpadded, eagerly
        self.graph_budget_bytes = 64 << 30       # device memory the buckets' graphs may hold (their shared pool + static buffers); beyond it all are dropped
        self._graphs = OrderedDict()             # bucket key -> {"graph", "in", "out", "ctx", "bwd": {...}, "bytes"}
        self._pool = None                        # ONE private memory pool for all buckets of this model (see _forward_bucketed)
        self._seen = _graphs.Seen()
        # device int32 [n_conv]: valid frames after every conv layer of the utterance in flight
        self._valid = torch.zeros(len(c["conv_kernel"]), dtype=torch.int32, device=self.device)
        self._vl = None                          # = self._valid while a bucketed launch sequence is being issued / captured, else None
        self._ctx, self._ctx_static, self._ctx_key = None, False, None

    def _qv_names(self, l):
        """The names (without `.weight` / `.bias`) of layer l's query and value projections, the two ends of its packed q | k | v slots."""
        p = f"{self._prefix}encoder.layers.{l}."
        return p + self._qkv_fmt.format("q"), p + self._qkv_fmt.format("v")

    # ------------------------------------------------------------------ nn.Module-like surface
    def grads_hf(self):
        """{name: gradient in HF layout} (tests)."""
        return {n: self._to_hf(n, self.G[n]) for n, _ in self.spec}

    def _to_hf(self, name, t):
        kind = self._kind[name]
        if kind == "conv":
            return _conv_to_hf(t)
        if kind == "g":
            return t.reshape(1, 1, -1)
        if kind == "heads":
            return t.reshape(1, -1, 1, 1)
        return t

    def state_dict(self):
        return {n: self._to_hf(n, p).detach().clone() for n, p in self.named_parameters()}

    def load_state_dict(self, sd, strict=True):
        missing = [n for n, _ in self.spec if n not in sd]
        if strict and missing:
            raise KeyError(f"missing {missing[:4]}…")
        for n, _ in self.spec:
            if n not in sd:
                continue
            t = sd[n].to(torch.float32)
            native = tuple(self.P[n].shape)
            want = (native[0], native[2], native[1]) if self._kind[n] == "conv" else native
            if t.numel() != self.P[n].numel() or (self._kind[n] == "conv" and tuple(t.shape) != want):
                raise ops.DynError(f"{n}: shape {tuple(t.shape)} in the state dict does not fit this configuration's {want}")
            if self._kind[n] == "conv":
                t = _conv_to_native(t)
            self.P[n].copy_(t.reshape(self.P[n].shape).to(self.device))
        return SimpleNamespace(missing_keys=missing, unexpected_keys=[k for k in sd if k not in self.P])

    def modules(self):
        return []

    # ------------------------------------------------------------------ forward
    def conv_lengths(self, L):
        """Frames after every layer of the feature extractor for L input samples."""
        out = []
        for k, st in zip(self.cfg["conv_kernel"], self.cfg["conv_stride"]):
            L = (L - k) // st + 1
            out.append(L)
        return out

    def samples_for_frames(self, T):
        """The smallest number of input samples that gives T output frames."""
        L = T
        for k, st in zip(reversed(self.cfg["conv_kernel"]), reversed(self.cfg["conv_stride"])):
            L = (L - 1) * st + k
        return L

    def forward(self, input_values):
        """input_values [B, L] float32 on the device (already zero-mean / unit-variance) -> SimpleNamespace(logits [B, T', V], frames).

        With `use_graphs` the launch sequence of a LENGTH BUCKET is captured once as a hipGraph and replayed for every utterance that
        falls into it (the per-utterance loop, reference wav2vec2/lib.py:293-462, is launch-bound — ~500 launches
        of work for ~10 ms of audio model time, and every utterance has its own length).  The waveform is zero-padded to the bucket's
        sample count; `logits` then has the BUCKET's frame count and `frames` says how many of them belong to the utterance.  The
        utterance's own frame counts live in HBM (`_valid`) and are read by the kernels when the graph runs, so that the valid frames
        are those of the unpadded run: the first layer's GroupNorm takes its statistics over the valid frames only
        (dyn_colnorm_fwd_len), the frames past the end are zeroed before the positional conv (dyn_mask_rows: what its zero padding
        holds there), and attention masks the keys past the end (dyn_softmax_fwd_len).  Everything else is per frame, or (the strided
        convs) looks only backwards from a valid frame.  The backward gets exact zeros on the padded frames (CTC gives them zero
        gradient, every per-frame BACKWARD kernel maps a zero gradient row to a zero gradient row, the masked softmax cuts the
        attention path, dyn_mask_rows / dyn_colnorm_bwd_len cut the other two), so every weight gradient sums the same terms plus
        zeros: equal to the unpadded run up to the summation order of a longer K (tests/test_wav2vec2_gpu.py).
        In the forward the padded rows hold zeros only in the base layout, where every per-frame kernel maps 0 to 0.  With the
        layer-norm extractor they do not (the conv bias and the LayerNorm's beta put finite non-zero values there, the stable encoder's
        LayerNorms likewise): nothing reads them — the statistics of that layout are per row (no ops.colnorm, `_valid[0]` unused),
        dyn_mask_rows zeroes them before the positional conv and the masked softmax drops them as keys — and their gradients are
        still exactly zero because every op that layout adds is per row (tests/test_wav2vec2_layernorm_gpu.py).
        WavLM's attention bias (wavlm_model.py) keeps the argument: a padded query row has dS = 0 (CTC), so its gate gradient, its terms of
        the bias table's gradient and its terms of the gate's input gradient are exact zeros (tests/test_wavlm_gpu.py)."""
        x = input_values
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
            raise ops.DynError("input_values must be a float32 CUDA tensor [B, L]")
        with ops.use_workspace(self._scratch()):
            if self.use_graphs and not ops.GEMM_PROFILE_EAGER():
                return self._forward_bucketed(x)
            self._vl, self._ctx_static = None, False
            return self._forward_eager(x)

    def _bucket(self, L):
        T = self.conv_lengths(L)[-1]
        q = max(1, int(self.bucket_frames))
        Tb = -(-T // q) * q
        return T, Tb, self.samples_for_frames(Tb + 1) - 1       # every L with <= Tb frames fits; the bucket itself has exactly Tb frames

    def graph_bytes(self):
        return sum(e["bytes"] for e in self._graphs.values())

    def drop_graphs(self):
        """Forget every captured bucket (never inside a capture: destroying a graph there aborts the process).  The shared pool goes back to the
        allocator once its last graph is gone."""
        if self._graphs:
            torch.cuda.synchronize(self.device)             # no replay may still be in flight when its graph is destroyed
        for ent in self._graphs.values():
            ent.clear()
        self._graphs.clear()
        self._pool = None
        if self._ctx is _RELEASED:
            self._ctx = None
        self._ctx_static = False

    def _forward_bucketed(self, x):
        B, L = x.shape
        need = self.samples_for_frames(1)
        if L < need:
            raise ops.DynError(f"input of {L} samples is shorter than the feature extractor's receptive field ({need} samples)")
        T, Tb, Lb = self._bucket(L)
        key = (B, Lb, torch.is_grad_enabled())
        ent = self._graphs.get(key)
        if ent is None:
            if not self._seen(key, self.graph_after):
                self._vl, self._ctx_static = None, False
                return self._forward_eager(x)
            if self.graph_bytes() > self.graph_budget_bytes:
                self.drop_graphs()
            # ONE private pool for every bucket of this model, and no Python reference to a bucket's saved activations once its backward graph
            # exists (_backward_graphed): the next bucket's capture then reuses that memory, so the pool grows to the LARGEST bucket's needs,
            # not to their sum (15 buckets of one 5-min talk held 26 GiB with a pool each).  Safe because the graphs of one model replay
            # strictly as forward(b), backward(b) pairs on one stream: a bucket's activations only have to survive from its forward replay to
            # its own backward replay, and no other graph of this model runs in between.  (Not the interleaved case of model.py::_graph_pool.)
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            r0 = torch.cuda.memory_reserved(self.device)
            static_in = torch.zeros(B, Lb, device=self.device, dtype=torch.float32)
            self._vl = self._valid
            try:
                graph, out = _graphs.capture(self._pool, lambda: self._forward_eager(static_in))
            finally:
                self._vl = None
            ent = {"graph": graph, "in": static_in, "out": out.logits, "ctx": self._ctx, "bwd": {}, "len": 0,
                   "bytes": max(0, torch.cuda.memory_reserved(self.device) - r0)}
            self._graphs[key] = ent
        self._graphs.move_to_end(key)
        ent["in"][:, :L].copy_(x)
        if L < ent["len"]:
            ent["in"][:, L:ent["len"]].zero_()
        ent["len"] = L                                   # (beyond the previous utterance's end the buffer is still zero)
        self._fill_valid(self.conv_lengths(L))
        ent["graph"].replay()
        self._ctx, self._ctx_static, self._ctx_key = (ent["ctx"] if ent["ctx"] is not None else _RELEASED), True, key
        return SimpleNamespace(logits=ent["out"], frames=T)

    def _fill_valid(self, cl):
        """The utterance's frame counts `cl` (conv_lengths) into the device scalars the captured kernels read.  A model whose encoder runs at
        another frame rate (sew_model.py) adds its own."""
        self._valid[0:1].fill_(cl[0])                    # (fills, not a pageable upload: that would block the host on this stream and stall the
        self._valid[-1:].fill_(cl[-1])                   #  other chains of wav2vec2_lib.dynamic_eval_su_many)

    def _forward_eager(self, x):
        c, P, pf = self.cfg, self.P, self._prefix
        vl = self._vl
        v0 = vl[0:1] if vl is not None else None             # valid frames after the first conv (its GroupNorm runs over time)
        vT = vl[-1:] if vl is not None else None             # valid frames of the encoder
        save = torch.is_grad_enabled()
        ctx = {"conv": []} if save else None
        B, L = x.shape
        need = 1
        for k, st in zip(reversed(c["conv_kernel"]), reversed(c["conv_stride"])):   # receptive field of the conv stack (400 samples)
            need = (need - 1) * st + k
        if L < need:
            raise ops.DynError(f"input of {L} samples is shorter than the feature extractor's receptive field ({need} samples)")
        fe = pf + "feature_extractor.conv_layers."
        a = x.contiguous().view(B, L, 1)
        for i, (k, s) in enumerate(zip(c["conv_kernel"], c["conv_stride"])):
            w = P[f"{fe}{i}.conv.weight"]
            z = ops.conv1d(a, w.view(w.shape[0], -1), k, s)
            if self.layer_extractor:                                # conv -> + bias -> LayerNorm(C) -> GELU; only (a, z, mean, rstd) are kept
                act, mean, rstd = ops.bias_layernorm_gelu(z, P[f"{fe}{i}.conv.bias"] if c["conv_bias"] else None, P[f"{fe}{i}.layer_norm.weight"],
                                                          P[f"{fe}{i}.layer_norm.bias"], EXTRACTOR_EPS)
                if save:
                    ctx["conv"].append((a, z, (mean, rstd)))
            elif i == 0:
                n0, mean, rstd = ops.colnorm(z, P[fe + "0.layer_norm.weight"], P[fe + "0.layer_norm.bias"], c["layer_norm_eps"], valid=v0)
                act = ops.gelu(n0)
                if save:
                    ctx["conv"].append((a, z, (mean, rstd, n0)))
            else:
                act = ops.gelu(z)
                if save:
                    ctx["conv"].append((a, z, None))
            a = act
        T = a.shape[1]
        h, kept = self._project(a)
        if vT is not None:
            ops.mask_rows(h, vT)                                    # the positional conv must see zeros past the utterance's last frame
        if save:
            ctx["proj"] = kept
        return self._encode(h, ctx, vT, (B, L, T), v0)

    def _project(self, a):
        """The feature projection of the extractor's output a [B, T, C]: returns (h [B, T, H], what _project_bwd needs, batch-major).  A
        model whose projection differs (HuBERT without its LayerNorm) overrides the pair."""
        c, P = self.cfg, self.P
        fp = self._prefix + "feature_projection."
        n, mean, rstd = ops.layernorm(a, P[fp + "layer_norm.weight"], P[fp + "layer_norm.bias"], c["layer_norm_eps"])
        h = ops.linear(n, P[fp + "projection.weight"], P[fp + "projection.bias"])
        return h, (a, mean, rstd, n)

    def _project_bwd(self, kept, dhs):
        """Backward of _project (`kept` already cut to the active samples): accumulates its parameters' gradients, returns dL/da."""
        P, G = self.P, self.G
        a, mean, rstd, n = kept
        fp = self._prefix + "feature_projection."
        dn = self._lin_bwd(dhs, n, fp + "projection.weight", fp + "projection.bias")
        da = torch.empty_like(dn)
        ops.layernorm_bwd(a, P[fp + "layer_norm.weight"], mean, rstd, dn, da, self._g(fp + "layer_norm.weight"), self._g(fp + "layer_norm.bias"), dx_beta=0.0)
        return da

    def _encode(self, h, ctx, vT, dims, v0):
        """The encoder and lm_head from the feature projection's output h [B, T, H] (rows past `vT` zeroed): fills ctx["pos"], ["layers"],
        ["head"], ["dims"], ["valid"] (+ ["final"] in the stable-LN layout) for _backward_encoder, sets self._ctx.  A model of the family
        with another encoder (wav2vec2_conformer_model.py) overrides this together with _backward_encoder."""
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        B, L, T = dims
        # positional conv embedding, residual, LayerNorm
        pos, kept = self._pos_embed(h, vT)
        hs = h.clone() if save else h
        ops.axpby(pos, hs, 1.0, 1.0)
        if self.stable_ln:
            return self._encoder_stable(hs, ctx, kept, vT, (B, L, T), v0)
        h2, mean, rstd = ops.layernorm(hs, P[pf + "encoder.layer_norm.weight"], P[pf + "encoder.layer_norm.bias"], c["layer_norm_eps"])
        if save:
            ctx["pos"] = kept + (hs, mean, rstd)
        h = self._post_ln_layers(h2, ctx, vT)
        logits = ops.linear(h, P["lm_head.weight"], P["lm_head.bias"])
        if save:
            ctx["head"] = h
            ctx["dims"] = (B, L, T)
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    def _post_ln_layers(self, h, ctx, vT):
        """The post-LN transformer layers (transformers Wav2Vec2EncoderLayer) on h [B, T, H], keys past `vT` masked: returns the last layer's
        output and fills ctx["layers"] for _post_ln_layers_bwd.  Shared with a model whose layers run at another frame count (sew_model.py)."""
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        if save:
            ctx["layers"] = []
        for l in range(c["num_hidden_layers"]):
            p = f"{pf}encoder.layers.{l}."
            qkv, S, O = self._attention(h, l, vT)
            r1 = h.clone() if save else h
            ops.linear(O, P[p + "attention.out_proj.weight"], P[p + "attention.out_proj.bias"], out=r1, beta=1.0)
            h1, m1, s1 = ops.layernorm(r1, P[p + "layer_norm.weight"], P[p + "layer_norm.bias"], c["layer_norm_eps"])
            u = ops.linear(h1, P[p + "feed_forward.intermediate_dense.weight"], P[p + "feed_forward.intermediate_dense.bias"])
            ga = ops.gelu(u)
            r2 = h1.clone() if save else h1
            ops.linear(ga, P[p + "feed_forward.output_dense.weight"], P[p + "feed_forward.output_dense.bias"], out=r2, beta=1.0)
            h2, m2, s2 = ops.layernorm(r2, P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"], c["layer_norm_eps"])
            if save:
                ctx["layers"].append((h, qkv, S, O, r1, m1, s1, h1, u, ga, r2, m2, s2))
            h = h2
        return h

    def _pos_embed(self, h, vT):
        """The positional embedding of h [B, T, H] (rows past `vT` are zero): returns (pos [B, T, H], a tuple of what _pos_embed_bwd needs).
        Here wav2vec2's: one grouped, weight-normed conv, then GELU.  A model with another positional embedding (data2vec_audio_model.py)
        overrides the pair."""
        c, P, pf = self.cfg, self.P, self._prefix
        B, T, _ = h.shape
        pc = pf + "encoder.pos_conv_embed.conv."
        H, K, G = c["hidden_size"], c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        cg, pad = H // G, K // 2
        w = self._pos_weight()                                      # [H, K, cg]
        xg = ops.group_pack(h, G, pad)                              # [B, G, T + 2 pad, cg]
        Tp = T + 2 * pad
        yg = torch.empty(B, G, T, cg, device=h.device, dtype=torch.float32)
        ops.gemm(xg, w, yg, trans_b=True, M=T, N=cg, K=K * cg, lda=cg, ldb=K * cg, ldc=cg, nb1=B, nb2=G,
                 sa=(G * Tp * cg, Tp * cg), sb=(0, cg * K * cg), sc=(G * T * cg, T * cg))
        pre = ops.group_unpack(yg, P[pc + "bias"], T, H)
        pos = ops.gelu(pre)
        return pos, (xg, w, pre)

    def _pos_weight(self):
        """The positional conv's weight [H, K, cg] from its weight-norm parameters."""
        c, P = self.cfg, self.P
        pc = self._prefix + "encoder.pos_conv_embed.conv."
        K, cg = c["num_conv_pos_embeddings"], c["hidden_size"] // c["num_conv_pos_embedding_groups"]
        v, g = P[pc + "parametrizations.weight.original1"], P[pc + "parametrizations.weight.original0"]
        parts = _wn_parts(K, cg)
        return ops.weight_norm(v, g) if parts == 1 else _wn_join(ops.weight_norm(_wn_split(v, parts), g), parts)

    def _pos_weight_bwd(self, dw):
        """Backward of _pos_weight: adds the weight-norm parameters' gradients given dw [H, K, cg]."""
        c, P, G = self.cfg, self.P, self.G
        pc = self._prefix + "encoder.pos_conv_embed.conv."
        H, K = c["hidden_size"], c["num_conv_pos_embeddings"]
        cg = H // c["num_conv_pos_embedding_groups"]
        v, g = P[pc + "parametrizations.weight.original1"], P[pc + "parametrizations.weight.original0"]
        parts = _wn_parts(K, cg)
        if parts == 1:
            ops.weight_norm_bwd(v, g, dw, G[pc + "parametrizations.weight.original1"], G[pc + "parametrizations.weight.original0"], beta=1.0)
        else:                                                        # rows wider than the kernel's LDS buffer: see _wn_split
            dv = torch.zeros(parts * H, K, cg // parts, device=dw.device, dtype=torch.float32)
            ops.weight_norm_bwd(_wn_split(v, parts), g, _wn_split(dw, parts), dv, G[pc + "parametrizations.weight.original0"], beta=1.0)
            ops.axpby(_wn_join(dv, parts), G[pc + "parametrizations.weight.original1"], 1.0, 1.0)

    def _attention(self, h, l, vT):
        """Self-attention of layer l on h [B, T, H] up to (not including) the output projection: returns (qkv, S, O)."""
        c, P, pf = self.cfg, self.P, self._prefix
        B, T, H = h.shape
        nh = c["num_attention_heads"]
        D = H // nh
        p = f"{pf}encoder.layers.{l}."
        qkv = torch.empty(B, T, 3 * H, device=h.device, dtype=torch.float32)
        if self.packed_qkv:
            ops.linear(h, self.Pqkv[l][0], self.Pqkv[l][1], out=qkv)
        for j, nm in enumerate(() if self.packed_qkv else ("q_proj", "k_proj", "v_proj")):
            ops.gemm(h, P[p + f"attention.{nm}.weight"], qkv, trans_b=True, M=B * T, N=H, K=H, lda=H, ldb=H, ldc=3 * H,
                     c_off=j * H, bias=P[p + f"attention.{nm}.bias"])
        S = torch.empty(B, nh, T, T, device=h.device, dtype=torch.float32)
        _attn.scores(_attn.packed(qkv, 0, D), _attn.packed(qkv, 1, D), S, D ** -0.5)
        kept = self._softmax(S, h, l, vT)
        O = torch.empty(B, T, H, device=h.device, dtype=torch.float32)
        _attn.context(S, _attn.packed(qkv, 2, D), _attn.plain(O, D))
        return qkv, (S if kept is None else (S,) + tuple(kept)), O

    def _softmax(self, S, h, l, vT):
        """The scores S [B, nh, T, T] of layer l -> probabilities, in place (keys past `vT` masked).  `h` is the attention's input: a model whose
        scores depend on it beyond q k^T (WavLM) overrides this together with _softmax_bwd and returns the tensors its backward needs; they
        travel with S through the saved context (batch-major, so an `n_active` backward cuts them like every other activation)."""
        ops.softmax(S, out=S, valid=vT)
        return None

    def _softmax_bwd(self, dS, kept, h, l, dh):
        """After _attention_bwd: dS is the gradient w.r.t. the pre-softmax scores, `kept` what _softmax returned, dh the gradient of the
        attention's input, to be added to in place.  Nothing here."""

    def _encoder_stable(self, x, ctx, pos, vT, dims, v0):
        """The pre-LN encoder (transformers Wav2Vec2EncoderStableLayerNorm) from x = h + gelu(pos_conv(h)): per layer
        x = x + out_proj(attn(LN1(x))), x = x + ffn(LN2(x)); the encoder's LayerNorm after the last layer; lm_head."""
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        eps = c["layer_norm_eps"]
        if save:
            ctx["pos"] = pos + (None, None, None)
            ctx["layers"] = []
        for l in range(c["num_hidden_layers"]):
            p = f"{pf}encoder.layers.{l}."
            n1, m1, s1 = ops.layernorm(x, P[p + "layer_norm.weight"], P[p + "layer_norm.bias"], eps)
            qkv, S, O = self._attention(n1, l, vT)
            r1 = x.clone() if save else x
            ops.linear(O, P[p + "attention.out_proj.weight"], P[p + "attention.out_proj.bias"], out=r1, beta=1.0)
            n2, m2, s2 = ops.layernorm(r1, P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"], eps)
            u = ops.linear(n2, P[p + "feed_forward.intermediate_dense.weight"], P[p + "feed_forward.intermediate_dense.bias"])
            ga = ops.gelu(u)
            r2 = r1.clone() if save else r1
            ops.linear(ga, P[p + "feed_forward.output_dense.weight"], P[p + "feed_forward.output_dense.bias"], out=r2, beta=1.0)
            kept = ()
            if self.adapter_dim:                                    # x + adapter(x), one launch; in place when nothing is kept
                w = [P[p + "adapter_layer." + n] for n in ADAPTER_PARAMS]
                y, am, ars, aa = ops.attn_adapter(r2, *w, eps=ADAPTER_EPS, out=None if save else r2, save=save)
                kept, r2 = ((r2, am, ars, aa),), y
            if save:
                ctx["layers"].append((x, m1, s1, n1, qkv, S, O, r1, m2, s2, n2, u, ga) + kept)
            x = r2
        h, mean, rstd = ops.layernorm(x, P[pf + "encoder.layer_norm.weight"], P[pf + "encoder.layer_norm.bias"], eps)
        logits = ops.linear(h, P["lm_head.weight"], P["lm_head.bias"])
        if save:
            ctx["final"] = (x, mean, rstd)
            ctx["head"] = h
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=dims[2])

    def _attention_bwd(self, dO, qkv, S, h, l, nb, T, residual):
        """Backward of _attention: queues / accumulates the q | k | v weight gradients and returns d h (+ `residual` when given, out of
        place: it may be a queued operand)."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        p = f"{pf}encoder.layers.{l}."
        S, kept = (S[0], S[1:]) if isinstance(S, tuple) else (S, None)
        dqkv = torch.empty_like(qkv)
        (q, k, v), (dq, dk, dv) = ([_attn.packed(t, j, D) for j in range(3)] for t in (qkv, dqkv))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)                # dP is now dS, the gradient of the pre-softmax scores
        _attn.grad_qk(dP, q, k, dq, dk, D ** -0.5)
        M = nb * T
        if self.packed_qkv:                                      # the three projections as one [3H, H] product each way
            q, v = self._qv_names(l)
            k = q[:-len(self._qkv_fmt.format("q"))] + self._qkv_fmt.format("k")
            if any(self.trainable(n + s) for n in (q, k, v) for s in (".weight", ".bias")):     # all six frozen: no product
                self._wgrad(dqkv.view(M, 3 * H), h.view(M, H), self.Gqkv[l][0], self.Gqkv[l][1])
            dh_in = torch.empty_like(dO)                         # the residual path may be a queued operand: not accumulated in place
            if residual is not None:
                ops.gemm(dqkv, self.Pqkv[l][0], dh_in, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H, beta=1.0, c_in=residual)
            else:
                ops.gemm(dqkv, self.Pqkv[l][0], dh_in, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        elif residual is None:
            dh_in = torch.zeros_like(dO)
        else:
            dh_in = residual.clone() if self._wq is not None else residual
        for j, nm in enumerate(() if self.packed_qkv else ("q_proj", "k_proj", "v_proj")):
            # dW += dqkv_j^T h ; db += colsum ; dh += dqkv_j W      (dqkv_j is a strided [M, H] slice, lda = 3H)
            ops.gemm(dqkv, h, G[p + f"attention.{nm}.weight"], trans_a=True, M=H, N=H, K=M, lda=3 * H, ldb=H, ldc=H, a_off=j * H, beta=1.0)
            dj = dqkv.view(M, 3, H)[:, j, :].contiguous()
            ops.colsum(dj, G[p + f"attention.{nm}.bias"], beta=1.0)
            ops.gemm(dqkv, P[p + f"attention.{nm}.weight"], dh_in, M=M, N=H, K=H, lda=3 * H, ldb=H, ldc=H, a_off=j * H, beta=1.0)
        if kept is not None:
            self._softmax_bwd(dP, kept, h, l, dh_in)
        return dh_in

    # ------------------------------------------------------------------ backward
    def _wgrad(self, dy, x, dw, db):
        """dw += dy^T x, db += column sums of dy: queued for the ONE grouped launch that ends the backward (the products of a short
        utterance are 36 - 144 tiles each: far too few to fill the chip alone), or at once.  Queued operands must stay unmodified."""
        dy = dy.contiguous()
        if self._wq is not None and ops.wgrad_groupable(dy, x, dw):
            self._wq.append(ops.wgrad_desc(dy, x, dw, beta=1.0, colsum=db, colsum_beta=1.0))
            return
        ops.linear_wgrad(dy, x, dw, beta=1.0)
        if db is not None:
            ops.colsum(dy, db, beta=1.0)

    def _g(self, name):
        """The gradient buffer of a parameter, or None when it is frozen: a kernel that takes a null gradient pointer skips that sum."""
        return self.G[name] if self.trainable(name) else None

    def _lin_bwd(self, dy, x, wname, bname, need_dx=True):
        if self.trainable(wname) or (bname is not None and self.trainable(bname)):      # both frozen: no product, no column sum
            self._wgrad(dy, x, self.G[wname], self.G[bname] if bname is not None else None)
        return ops.linear_dgrad(dy, self.P[wname]) if need_dx else None

    def backward(self, grad_logits, n_active=None):
        """Accumulates dL/dparam into flat_grads given dL/dlogits [nb, T', V] for the first nb samples of the batch.  The launch-bound
        column reductions of the norm / bias gradients run as one batched launch at the end (ops.reduce_defer; bit-identical)."""
        with ops.use_workspace(self._scratch()):
            if self._ctx_static and self.use_graphs and self._ctx is not None:
                return self._backward_graphed(grad_logits, n_active)
            self._backward_eager(grad_logits, n_active)

    def _backward_graphed(self, grad_logits, n_active):
        """Replay (first use: capture) of the backward launch sequence of the bucket whose forward graph produced the saved activations."""
        ent = self._graphs[self._ctx_key]
        key = (tuple(grad_logits.shape), n_active, frozenset(self.frozen), self.grouped_wgrad)
        b = ent["bwd"].get(key)
        if b is None and ent["ctx"] is None:
            # another backward variant (other frozen set / active copies) after the bucket's activations were released: recompute them eagerly from
            # the bucket's input buffer (the utterance and its frame counts are still there) and run this backward eagerly
            self._vl = self._valid
            try:
                with torch.enable_grad():
                    self._forward_eager(ent["in"])
            finally:
                self._vl = None
            self._ctx_static = False
            return self._backward_eager(grad_logits, n_active)
        if b is None:
            self._ctx = ent["ctx"]
            r0 = torch.cuda.memory_reserved(self.device)
            static_g = grad_logits.contiguous().clone()
            graph, _ = _graphs.capture(self._pool, lambda: self._backward_eager(static_g, n_active))
            b = ent["bwd"][key] = {"graph": graph, "g": static_g}
            ent["bytes"] += max(0, torch.cuda.memory_reserved(self.device) - r0)
            ent["ctx"] = None                                    # released: both graphs hold the addresses, nobody needs the tensors
        b["g"].copy_(grad_logits)
        b["graph"].replay()
        self._ctx = None

    def _backward_eager(self, grad_logits, n_active):
        # every linear layer's weight gradient (+ bias sums) of this backward: one launch
        with self._reduce_defer(), self._wgrad_queue(self.grouped_wgrad):
            self._backward_layers(grad_logits, n_active)
        for n, _ in self.spec:                      # after the deferred reductions have been queued: they write gradients too
            if not self.trainable(n):
                self.G[n].zero_()

    def _backward_layers(self, grad_logits, n_active=None):
        ctx = self._ctx
        if ctx is None or ctx is _RELEASED:
            raise ops.DynError("backward() without a grad-mode forward (or use_graphs switched off between a bucketed forward and its backward)")
        if self._ctx_static:                        # a graph-owned context must survive the backward (entries are dropped below as they are used)
            ctx = dict(ctx)
            ctx["layers"], ctx["conv"] = list(ctx["layers"]), list(ctx["conv"])
        v0, vT = ctx["valid"]
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        B, L, T = ctx["dims"]
        nb = B if n_active is None else int(n_active)
        assert grad_logits.shape[0] == nb

        def cut(t):
            if isinstance(t, tuple):
                return tuple(cut(x) for x in t)
            if t is None or nb == B:
                return t
            if t.dim() == 1:
                return t[:nb * (t.shape[0] // B)]
            return t[:nb]

        dhs = self._backward_encoder(ctx, grad_logits, nb, cut)
        if dhs is None:                                              # everything below the encoder's layers is frozen
            self._ctx = None
            return
        # feature projection
        da = self._project_bwd(cut(ctx["proj"]), dhs)
        # conv feature extractor
        fe = pf + "feature_extractor.conv_layers."
        for i in reversed(range(len(c["conv_kernel"]))):
            k, s = c["conv_kernel"][i], c["conv_stride"][i]
            a_in, z, norm = cut(ctx["conv"][i])
            wname = f"{fe}{i}.conv.weight"
            wmat = P[wname].view(P[wname].shape[0], -1)
            if self.layer_extractor:                                 # GELU', LayerNorm backward and the three column sums in one pass, dz over da
                mean, rstd = norm
                gw, gb, cb = (f"{fe}{i}.layer_norm.weight", f"{fe}{i}.layer_norm.bias", f"{fe}{i}.conv.bias")
                has = (True, True, c["conv_bias"])                 # a model of the family may have no conv bias here (Data2Vec-Audio)
                dz = ops.bias_layernorm_gelu_bwd(z, P[cb] if has[2] else None, P[gw], P[gb], mean, rstd, da,
                                                 *(G[n] if h and self.trainable(n) else None for n, h in zip((gw, gb, cb), has)), out=da)
            elif i == 0:
                mean, rstd, n0 = norm
                dn0 = ops.gelu_bwd(n0, da)
                dz = ops.colnorm_bwd(z, P[fe + "0.layer_norm.weight"], mean, rstd, dn0, G[fe + "0.layer_norm.weight"], G[fe + "0.layer_norm.bias"],
                                     valid=v0)
            else:
                dz = ops.gelu_bwd(z, da)
            ops.conv1d_wgrad(a_in, dz, G[wname].view(wmat.shape), k, s, beta=1.0)
            if i > 0:
                da = ops.conv1d_dgrad(dz, wmat, a_in.shape[1], a_in.shape[2], k, s)
            ctx["conv"][i] = None
        self._ctx = None

    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        """Backward of _encode from dL/dlogits [nb, T', V]: accumulates the gradients of lm_head and the encoder, returns the gradient of the
        feature projection's output (rows past the utterance's last frame zero).  `ctx` is this backward's own copy of the saved context
        (entries are dropped as they are used), `cut` trims a saved activation to the first nb samples."""
        v0, vT = ctx["valid"]
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        B, L, T = ctx["dims"]
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        eps = c["layer_norm_eps"]
        h_last = cut(ctx["head"])
        dh = self._lin_bwd(grad_logits.contiguous(), h_last, "lm_head.weight", "lm_head.bias")
        if self.stable_ln:
            x, mean, rstd = cut(ctx["final"])
            dx = torch.empty_like(dh)
            ops.layernorm_bwd(x, P[pf + "encoder.layer_norm.weight"], mean, rstd, dh, dx, self._g(pf + "encoder.layer_norm.weight"),
                              self._g(pf + "encoder.layer_norm.bias"), dx_beta=0.0)
        for l in reversed(range(c["num_hidden_layers"]) if self.stable_ln else ()):
            # x -> r1 = x + out_proj(attn(LN1(x))) -> r2 = r1 + ffn(LN2(r1)); dx is dL/dr2.  Each residual sum rides on the LayerNorm
            # backward's dx = grad + dx_in form (out of place: dx / dr1 are queued weight-gradient operands), so no add pass of its own.
            p = f"{pf}encoder.layers.{l}."
            x, m1, s1, n1, qkv, S, O, r1, m2, s2, n2, u, ga, *kept = cut(ctx["layers"][l])
            if kept:                                                 # the adapter behind the layer: dx becomes dL/d(its input), out of place
                r2, am, ars, aa = kept[0]
                ad = p + "adapter_layer."
                dx = ops.attn_adapter_bwd(r2, P[ad + "norm.weight"], P[ad + "norm.bias"], P[ad + "linear_1.weight"], P[ad + "linear_2.weight"],
                                          am, ars, aa, dx, *(self._g(ad + n) for n in ADAPTER_PARAMS))
            dga = self._lin_bwd(dx, ga, p + "feed_forward.output_dense.weight", p + "feed_forward.output_dense.bias")
            du = ops.gelu_bwd(u, dga, out=dga)
            dn2 = self._lin_bwd(du, n2, p + "feed_forward.intermediate_dense.weight", p + "feed_forward.intermediate_dense.bias")
            dr1 = torch.empty_like(dx)
            ops.layernorm_bwd(r1, P[p + "final_layer_norm.weight"], m2, s2, dn2, dr1, self._g(p + "final_layer_norm.weight"),
                              self._g(p + "final_layer_norm.bias"), dx_beta=1.0, dx_in=dx)
            dO = self._lin_bwd(dr1, O, p + "attention.out_proj.weight", p + "attention.out_proj.bias")
            dn1 = self._attention_bwd(dO, qkv, S, n1, l, nb, T, None)
            dx = torch.empty_like(dr1)
            ops.layernorm_bwd(x, P[p + "layer_norm.weight"], m1, s1, dn1, dx, self._g(p + "layer_norm.weight"), self._g(p + "layer_norm.bias"),
                              dx_beta=1.0, dx_in=dr1)
            ctx["layers"][l] = None
        if not self.stable_ln:
            dh = self._post_ln_layers_bwd(ctx, dh, nb, T, cut)
        # encoder LayerNorm, positional embedding
        kept = ctx["pos"][:-3]
        hs, mean, rstd = cut(ctx["pos"][-3:])
        if self.stable_ln:
            dhs = dx                                                 # dL/d(h + pos): no queued product reads it, so the pos path adds in place
        else:
            dhs = torch.empty_like(dh)
            ops.layernorm_bwd(hs, P[pf + "encoder.layer_norm.weight"], mean, rstd, dh, dhs, self._g(pf + "encoder.layer_norm.weight"),
                              self._g(pf + "encoder.layer_norm.bias"), dx_beta=0.0)
        if self._below_frozen():                                    # nothing under the first encoder layer adapts: its backward is not needed
            return None
        return self._pos_embed_bwd(kept, dhs, nb, cut, vT)

    def _below_frozen(self):
        """True when no parameter below the encoder's layers (positional embedding, feature projection, extractor) is trainable."""
        above = (self._prefix + "encoder.layers.", self._prefix + "encoder.layer_norm.", "lm_head.")
        return not any(self.trainable(n) for n, _ in self.spec if not n.startswith(above))

    def adapter_only(self):
        """The MMS recipe: freeze everything but the adapters and lm_head (the keys of transformers' `_get_adapters()`)."""
        if not self.adapter_dim:
            raise ops.DynError("adapter_only(): this model has no adapters (adapter_attn_dim with do_stable_layer_norm)")
        self.frozen = {n for n, _ in self.spec if ".adapter_layer." not in n and not n.startswith("lm_head.")}
        return self

    def _post_ln_layers_bwd(self, ctx, dh, nb, T, cut):
        """Backward of _post_ln_layers from dh [nb, T, H], the gradient of its output: accumulates the layers' gradients, returns the
        gradient of its input.  Entries of ctx["layers"] are dropped as they are used."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        for l in reversed(range(c["num_hidden_layers"])):
            p = f"{pf}encoder.layers.{l}."
            h, qkv, S, O, r1, m1, s1, h1, u, ga, r2, m2, s2 = cut(ctx["layers"][l])
            dr2 = torch.empty_like(dh)
            ops.layernorm_bwd(r2, P[p + "final_layer_norm.weight"], m2, s2, dh, dr2, self._g(p + "final_layer_norm.weight"),
                              self._g(p + "final_layer_norm.bias"), dx_beta=0.0)
            dga = self._lin_bwd(dr2, ga, p + "feed_forward.output_dense.weight", p + "feed_forward.output_dense.bias")
            du = ops.gelu_bwd(u, dga, out=dga)
            dh1 = self._lin_bwd(du, h1, p + "feed_forward.intermediate_dense.weight", p + "feed_forward.intermediate_dense.bias")
            ops.axpby(dr2, dh1, 1.0, 1.0)                            # residual: h1 feeds both the FFN and r2
            dr1 = torch.empty_like(dh1)
            ops.layernorm_bwd(r1, P[p + "layer_norm.weight"], m1, s1, dh1, dr1, self._g(p + "layer_norm.weight"), self._g(p + "layer_norm.bias"),
                              dx_beta=0.0)
            dO = self._lin_bwd(dr1, O, p + "attention.out_proj.weight", p + "attention.out_proj.bias")
            dh_in = self._attention_bwd(dO, qkv, S, h, l, nb, T, dr1)
            dh = dh_in
            ctx["layers"][l] = None
        return dh

    def _pos_embed_bwd(self, kept, dhs, nb, cut, vT):
        """Backward of _pos_embed: dhs [nb, T, H] is dL/d(h + pos); accumulates the embedding's parameter gradients, adds its path to dhs in
        place and returns it = dL/dh (rows past `vT` zero).  `kept` is _pos_embed's tuple, uncut: `cut` trims what is batch-major."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        T, H = dhs.shape[1], dhs.shape[2]
        w = kept[1]                                                  # the normalised weight is not batch-indexed
        xg, _, pre = cut(kept)
        pc = pf + "encoder.pos_conv_embed.conv."
        K, Gn = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        cg, pad = H // Gn, K // 2
        Tp = T + 2 * pad
        dpre = ops.gelu_bwd(pre, dhs)
        ops.colsum(dpre, G[pc + "bias"], beta=1.0)
        dyg = ops.group_pack_grad(dpre, Gn, T)                       # [nb, G, T, cg]
        dw = torch.zeros_like(w)
        for b in range(nb):                                          # dw[g] += dyg[b, g]^T rows(xg[b, g])
            ops.gemm(dyg, xg, dw, trans_a=True, M=cg, N=K * cg, K=T, lda=cg, ldb=cg, ldc=K * cg, nb1=1, nb2=Gn,
                     sa=(0, T * cg), sb=(0, Tp * cg), sc=(0, cg * K * cg), a_off=b * Gn * T * cg, b_off=b * Gn * Tp * cg, beta=1.0)
        self._pos_weight_bwd(dw)
        dA = torch.empty(nb, Gn, T, K * cg, device=dhs.device, dtype=torch.float32)
        ops.gemm(dyg, w, dA, M=T, N=K * cg, K=cg, lda=cg, ldb=K * cg, ldc=K * cg, nb1=nb, nb2=Gn, sa=(Gn * T * cg, T * cg),
                 sb=(0, cg * K * cg), sc=(Gn * T * K * cg, T * K * cg))
        dxg = torch.empty(nb * Gn, Tp, cg, device=dhs.device, dtype=torch.float32)
        ops.col2im_1d(dA, dxg, nb * Gn, Tp, T, cg, K, 1)
        ops.group_unpack_grad(dxg.view(nb, Gn, Tp, cg), dhs, pad, beta=1.0)   # dh (pre-pos) = dhs (residual) + pos-conv path
        if vT is not None:
            ops.mask_rows(dhs, vT)                                   # the windows of the last valid frames reach into the zeroed tail: no gradient there
        return dhs
