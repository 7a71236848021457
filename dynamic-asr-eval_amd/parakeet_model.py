"""ParakeetForCTC on MI355X: the FastConformer encoder + CTC head of the `nvidia/parakeet-ctc-*` checkpoints (`model_type: "parakeet_ctc"`,
transformers modeling_parakeet.py), the model family of the reference's third loop (nvidia_ctc/lib.py: NVIDIA's conformer-CTC models), as
`AutoModelForCTC` builds it in plain torch.  No attention mask, dropout zero.  The conv modules' norm by default reads its running statistics
(the eval-mode model).  That is NOT what the reference loop runs: it calls `model.train()` (nvidia_ctc/lib.py:74), puts `layer.conv` and its
batch norm into eval mode (:92-93) and then replaces that batch norm by a fresh, hence training-mode, BatchRenorm1d (:94-102).
`batch_renorm_training()` runs that norm (csrc/convmod_brn.hip); eval mode remains the default until a maintainer flips it.

A subclass of Wav2Vec2ConformerForCTC: the two half-step FFNs, Transformer-XL attention with per-head `bias_u` / `bias_v` and a bias-free
position projection (csrc/relshift.hip), the five attention products (_attn.py), the layer loop, flat parameters and the backward's deferred
reductions are the parent's, found under the parent's names through an alias table (LAYER_NAMES, as sew_d_model.py does).  What differs:
  * input: `input_features` [B, T, num_mel_bins] log-mel frames, as transformers takes them (the reference computes its spectrogram outside
    the loop, nvidia_ctc/lib.py:20-28); feature_extractor() / generate_from_audio() start at the waveform (frontend.MelFeatures).
  * subsampling (ParakeetEncoderSubsamplingConv2D, x8 `dw_striding`): Conv2d(1 -> C, 3, s2) -> ReLU -> 2 x [depthwise Conv2d(C, 3, s2) -> 1x1
    -> ReLU] -> flatten -> Linear(C F / 8 -> H).  The stage structure of the project's own conformer (csrc/conv.hip) with ReLU fused into
    the depthwise loads (ops.dwconv2d_s2_*_act) and ops.relu in front of the flatten; the unfused stages (the reference freezes this part,
    and its windows are 2048 frames).  The channels-last kernels flatten as (F, C), transformers as (C, F): the linear's weight lives in the
    kernels' order in the flat vector, its columns are permuted in state_dict() / load_state_dict() / grads_hf() (SUBLIN).
  * `scale_input`: the hidden states are multiplied by sqrt(hidden_size) after the subsampling linear, bias included.
  * position table: ParakeetEncoderRelPositionalEncoding.forward restated on the host in its own dtypes and operation order
    (position_table); ops.relative_position_table forms the angles differently and is not used.  Cached per frame count.
  * optional biases: `attention_bias` (q / k / v / o projections and both FFNs) and `convolution_bias` (the conv module's three convs) may
    each be false; the biases are then null pointers and absent from the state dict.
  * conv module: LN -> pointwise_conv1 -> [GLU -> depthwise conv (9 taps, SAME, optional bias) -> BatchNorm1d (eval) -> SiLU] ->
    pointwise_conv2, the bracket one launch forward and two backward (csrc/convmod_bn.hip: ops.convmod_bn, convmod_bn_bwd_act,
    glu_dwconv1d_dgrad) + the existing ops.dwconv1d_wgrad.  A backward keeps u, gl and c of the bracket instead of g, gl, dw, bn.
  * no `encoder.layer_norm`; the head is `ctc_head`, a k = 1 Conv1d = a linear.
  * the batch-norm buffers live outside the flat vector (`buffers_`), as in the parent.
  * ragged batches: `input_lengths=` (the valid feature frames per row) on forward / generate.  The counts behind each stride-2 stage
    (output_lengths) go to the device once; the first conv reads the frames past a row's length as zeros, the depthwise stages read and
    write their rows past it as zeros, the relative-position softmax takes the row's own key count, the conv module zeroes the GLU rows
    past it, backward() zeroes the incoming gradient there (the `_lens` entries of csrc/conv.hip, relshift.hip, convmod_bn.hip).  Valid
    frames equal the row run alone; DESIGN.md, "Ragged batches".

Not built, refused by name before any launch: `subsampling_factor` != 8, `subsampling_conv_kernel_size` != 3, `subsampling_conv_stride` != 2,
`subsampling_conv_channels` not a multiple of 4, `num_mel_bins` not a multiple of 8, `hidden_size` outside 256 / 512 / 768 / 1024,
`conv_kernel_size` != 9, `hidden_act` != "silu", `num_key_value_heads` != `num_attention_heads`, a `head_dim` other than hidden_size / heads,
an `attention_mask` argument.  Bucketed hipGraph replay and lockstep groups are out of scope (ParakeetForTDT and ParakeetForRNNT: since built,
parakeet_tdt_model.py, parakeet_rnnt_model.py).  No hub checkpoint is on
the machine: transformers' ParakeetForCTC on the CPU with the same (random) state dict is the oracle in the tests."""
import contextlib
import math
import weakref
from types import SimpleNamespace

import torch

from . import ops
from . import wav2vec2_conformer_model as WC
from . import wav2vec2_model as W2

ENCODER_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act", "attention_bias",
                "convolution_bias", "conv_kernel_size", "subsampling_factor", "subsampling_conv_channels", "num_mel_bins",
                "subsampling_conv_kernel_size", "subsampling_conv_stride", "max_position_embeddings", "scale_input", "num_key_value_heads",
                "head_dim")
DEFAULT_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=8, intermediate_size=4096, hidden_act="silu",
                      attention_bias=True, convolution_bias=True, conv_kernel_size=9, subsampling_factor=8, subsampling_conv_channels=256,
                      num_mel_bins=80, subsampling_conv_kernel_size=3, subsampling_conv_stride=2, max_position_embeddings=5000,
                      scale_input=True, num_key_value_heads=None, head_dim=None, vocab_size=1025, pad_token_id=1024, layer_norm_eps=1e-5)
WIDTHS = (256, 512, 768, 1024)         # instances of dyn_convmod_bn_* (and of the LayerNorm kernels)
CONV_KERNEL = 9
BN_EPS = 1e-5                          # nn.BatchNorm1d's default; the per-layer LayerNorms have torch's default too (WC.LAYER_EPS)
# the parent's name of a layer's parameter group -> transformers' (ParakeetEncoderBlock)
LAYER_NAMES = (("ffn1_layer_norm", "norm_feed_forward1"), ("ffn1.intermediate_dense", "feed_forward1.linear1"),
               ("ffn1.output_dense", "feed_forward1.linear2"), ("self_attn_layer_norm", "norm_self_att"),
               ("self_attn.linear_out", "self_attn.o_proj"), ("self_attn.linear_pos", "self_attn.relative_k_proj"),
               ("ffn2_layer_norm", "norm_feed_forward2"), ("ffn2.intermediate_dense", "feed_forward2.linear1"),
               ("ffn2.output_dense", "feed_forward2.linear2"), ("final_layer_norm", "norm_out"))
SUB = "encoder.subsampling."
FROZEN_IN_THE_LOOP = (SUB, "ctc_head.")          # nvidia_ctc/lib.py:81-86: pre_encode and the decoder do not adapt


def _flatten(cfg, keys=ENCODER_KEYS):
    """A ParakeetCTCConfig (or its dict, `encoder_config` nested; or a flat dict) -> one flat dict of the keys this module reads (`keys`: the
    encoder keys of another model of the family, lasr_model.py)."""
    if cfg is None:
        return {}
    get = (lambda o, k: o.get(k, None)) if isinstance(cfg, dict) else (lambda o, k: getattr(o, k, None))
    enc = get(cfg, "encoder_config")
    out = {}
    for src in (cfg, enc):
        if src is None:
            continue
        g = (lambda k, s=src: s.get(k, None)) if isinstance(src, dict) else (lambda k, s=src: getattr(s, k, None))
        for k in tuple(keys) + ("vocab_size", "pad_token_id"):
            if src is not cfg and k in ("vocab_size", "pad_token_id"):
                continue
            v = g(k)
            if v is not None:
                out[k] = v
    return out


def make_config(cfg=None, defaults=DEFAULT_CONFIG, keys=ENCODER_KEYS, mel_multiple=8):
    """transformers' ParakeetCTCConfig / ParakeetEncoderConfig keys with their defaults; what this forward does not build is refused by name.
    `defaults`, `keys`, `mel_multiple`: a model of the family with more encoder keys and another subsampling (nemotron_asr_streaming_model.py)."""
    out = W2.make_config(_flatten(cfg, keys), defaults)
    out["do_stable_layer_norm"] = False
    out["position_embeddings_type"] = "relative"             # the parent's switch: Transformer-XL scores
    out["conv_kernel"], out["conv_stride"], out["conv_dim"] = (), (), ()     # no waveform conv stack (_conv_extractor = False)
    if out["subsampling_factor"] != 8:
        raise ops.DynError(f"subsampling_factor={out['subsampling_factor']} is not built (8: three stride-2 stages)")
    if out["subsampling_conv_kernel_size"] != 3:
        raise ops.DynError(f"subsampling_conv_kernel_size={out['subsampling_conv_kernel_size']} is not built (3)")
    if out["subsampling_conv_stride"] != 2:
        raise ops.DynError(f"subsampling_conv_stride={out['subsampling_conv_stride']} is not built (2)")
    C, F = out["subsampling_conv_channels"], out["num_mel_bins"]
    if not (isinstance(C, int) and C > 0 and C % 4 == 0):
        raise ops.DynError(f"subsampling_conv_channels={C!r} is not built: the channels-last conv kernels take a positive multiple of 4")
    if not (isinstance(F, int) and F > 0 and F % mel_multiple == 0):
        raise ops.DynError(f"num_mel_bins={F!r} is not built: a positive multiple of {mel_multiple} (transformers' num_mel_bins // 8 columns "
                           "per channel are the conv stages' only then)")
    H, nh = out["hidden_size"], out["num_attention_heads"]
    if H not in WIDTHS:
        raise ops.DynError(f"hidden_size={H} is not built: one of {WIDTHS}")
    k = out["conv_kernel_size"] = int(out["conv_kernel_size"])
    if k != CONV_KERNEL:
        raise ops.DynError(f"conv_kernel_size={k} is not built ({CONV_KERNEL})")
    if out["hidden_act"] != "silu":
        raise ops.DynError(f"hidden_act={out['hidden_act']!r} is not built (\"silu\")")
    if H % nh:
        raise ops.DynError(f"hidden_size={H} is not a multiple of num_attention_heads={nh}")
    kv = out["num_key_value_heads"]
    if kv is not None and kv != nh:
        raise ops.DynError(f"num_key_value_heads={kv} is not built: it must equal num_attention_heads={nh}")
    hd = out["head_dim"]
    if hd is not None and hd != H // nh:
        raise ops.DynError(f"head_dim={hd} is not built: it must equal hidden_size / num_attention_heads = {H // nh}")
    out["num_key_value_heads"], out["head_dim"] = nh, H // nh
    out["attention_bias"], out["convolution_bias"], out["scale_input"] = (bool(out[k]) for k in ("attention_bias", "convolution_bias", "scale_input"))
    return out


def config_from_json(path):
    """An HF `config.json` of a parakeet_ctc checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def frames(T):
    """Encoder frames of T feature frames: three 3-wide, stride-2, pad-1 stages (transformers' _get_subsampling_output_length)."""
    for _ in range(3):
        T = ops.out_len(T)
    return T


def output_lengths(lens):
    """Valid feature frames per row -> [(frames into stage 1), after stage 1, after stage 2, after stage 3]: four lists, each stride-2 stage
    maps L -> (L - 1) // 2 + 1 (transformers' _get_subsampling_output_length); the last is the encoder's valid frames per row."""
    out = [[int(n) for n in lens]]
    for _ in range(3):
        out.append([ops.out_len(n) for n in out[-1]])
    return out


def lengths_from_mask(mask):
    """The feature extractor's `attention_mask` [B, T] (nonzero = valid frame) -> the list of valid frames per row.  A mask that is not a
    prefix (a valid frame behind an invalid one) or has an empty row is refused: `input_lengths` can only say how many leading frames count."""
    if not (isinstance(mask, torch.Tensor) and mask.dim() == 2 and mask.shape[1] >= 1 and not mask.is_floating_point() and not mask.is_complex()):
        raise ops.DynError("lengths_from_mask: the mask must be an integer or bool tensor [B, T]")
    m = (mask != 0).cpu()
    lens = m.sum(1)
    if not bool((m == (torch.arange(m.shape[1])[None, :] < lens[:, None])).all()):
        raise ops.DynError("lengths_from_mask: the mask is not a prefix mask (a valid frame follows an invalid one); input_lengths cannot express it")
    if int(lens.min()) < 1:
        raise ops.DynError("lengths_from_mask: a row of the mask has no valid frame")
    return [int(n) for n in lens]


def check_input_lengths(input_lengths, B, T):
    """`input_lengths` (a sequence of ints, or an integer tensor [B] on the host or the device: one host copy) -> a list of B ints in 1 .. T."""
    v = input_lengths
    if isinstance(v, torch.Tensor):
        if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ops.DynError(f"input_lengths must hold integers, not {v.dtype}")
        if v.dim() != 1:
            raise ops.DynError(f"input_lengths must be one count per row [B], not a tensor of shape {tuple(v.shape)}")
        v = v.tolist()
    elif isinstance(v, (list, tuple)):
        if not all(isinstance(n, int) and not isinstance(n, bool) for n in v):
            raise ops.DynError("input_lengths must hold integers")
        v = list(v)
    else:
        raise ops.DynError("input_lengths must be a sequence of ints or an integer tensor [B]")
    if len(v) != B:
        raise ops.DynError(f"input_lengths holds {len(v)} counts for a batch of {B} rows")
    if not all(1 <= n <= T for n in v):
        raise ops.DynError(f"input_lengths={v} must lie in 1 .. T = {T}, the frames of input_features")
    return v


def refuse_input_lengths(who, input_lengths):
    """A model of the family without per-row frame counts refuses them by name."""
    if input_lengths is not None:
        raise ops.DynError(f"input_lengths is not built for {who}: per-row frame counts exist for ParakeetForCTC, ParakeetForTDT and "
                           "ParakeetForRNNT; run every utterance at its own length")


def position_table(T, H):
    """ParakeetEncoderRelPositionalEncoding.forward for T frames of width H on the host, in its dtypes and operation order: [2T - 1, H]
    float32, positions T - 1 .. -(T - 1), sin / cos interleaved."""
    if not isinstance(T, int) or T < 1:
        raise ops.DynError(f"position_table: T={T!r} must be a positive integer")
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, H, 2, dtype=torch.float) / H))
    position_ids = torch.arange(T - 1, -T, -1)
    freqs = (inv_freq[None, :, None].float() @ position_ids[None, None, :].float()).transpose(1, 2)
    pe = torch.stack([freqs.sin(), freqs.cos()], dim=-1)
    return pe.reshape(*pe.shape[:-2], -1)[0].contiguous()


def sublin_to_hf(t, C, F3):
    """The subsampling linear's weight (or gradient) from the kernels' column order (f, c) to transformers' (c, f)."""
    return t.reshape(t.shape[0], F3, C).permute(0, 2, 1).reshape(t.shape[0], C * F3).contiguous()


def sublin_from_hf(t, C, F3):
    return t.reshape(t.shape[0], C, F3).permute(0, 2, 1).reshape(t.shape[0], F3 * C).contiguous()


def param_spec(c, pf=""):
    """[(name, shape, kind)] in transformers' names.  kind "pw": a k = 1 Conv1d kernel kept as [C_out, C_in]; "dw": a depthwise kernel kept
    without its singleton input-channel axis ([C, k] / [C, 3, 3]); "pw2": a 1x1 Conv2d kernel kept as [C, C] (all reshapes); "sublin": the
    subsampling linear, columns in the kernels' (f, c) order."""
    H, I, k, nh = c["hidden_size"], c["intermediate_size"], c["conv_kernel_size"], c["num_attention_heads"]
    C, F3 = c["subsampling_conv_channels"], c["num_mel_bins"] // 8
    ab, cb = c["attention_bias"], c["convolution_bias"]
    lin = lambda p, n, m, b=True, kind=None: [(p + ".weight", (n, m), kind)] + ([(p + ".bias", (n,), None)] if b else [])           # noqa: E731
    ln = lambda p: [(p + ".weight", (H,), None), (p + ".bias", (H,), None)]                                                            # noqa: E731
    s = pf + SUB
    spec = [(s + "layers.0.weight", (C, 3, 3), "dw"), (s + "layers.0.bias", (C,), None)]
    for i in (2, 5):
        spec += [(s + f"layers.{i}.weight", (C, 3, 3), "dw"), (s + f"layers.{i}.bias", (C,), None)]
        spec += lin(s + f"layers.{i + 1}", C, C, kind="pw2")
    spec += lin(s + "linear", H, C * F3, kind="sublin")
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}."
        spec += ln(p + "norm_feed_forward1") + lin(p + "feed_forward1.linear1", I, H, ab) + lin(p + "feed_forward1.linear2", H, I, ab)
        spec += ln(p + "norm_self_att")
        spec += [(p + f"self_attn.{n}_proj.weight", (H, H), None) for n in "qkv"]                  # q | k | v side by side
        spec += [(p + f"self_attn.{n}_proj.bias", (H,), None) for n in "qkv"] if ab else []
        spec += lin(p + "self_attn.o_proj", H, H, ab)
        spec += [(p + "self_attn.relative_k_proj.weight", (H, H), None), (p + "self_attn.bias_u", (nh, H // nh), None),
                 (p + "self_attn.bias_v", (nh, H // nh), None)]
        spec += ln(p + "norm_conv") + lin(p + "conv.pointwise_conv1", 2 * H, H, cb, "pw")
        spec += [(p + "conv.depthwise_conv.weight", (H, k), "dw")] + ([(p + "conv.depthwise_conv.bias", (H,), None)] if cb else [])
        spec += ln(p + "conv.norm") + lin(p + "conv.pointwise_conv2", H, H, cb, "pw")
        spec += ln(p + "norm_feed_forward2") + lin(p + "feed_forward2.linear1", I, H, ab) + lin(p + "feed_forward2.linear2", H, I, ab)
        spec += ln(p + "norm_out")
    return spec + [(pf + "ctc_head.weight", (c["vocab_size"], H), "pw"), (pf + "ctc_head.bias", (c["vocab_size"],), None)]


def buffer_spec(c, pf=""):
    """[(name, shape, dtype)] of the batch norms' buffers, in transformers' names."""
    out = []
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}.conv.norm."
        out += [(p + "running_mean", (c["hidden_size"],), torch.float32), (p + "running_var", (c["hidden_size"],), torch.float32),
                (p + "num_batches_tracked", (), torch.int64)]
    return out


class ParakeetForCTC(WC.Wav2Vec2ConformerForCTC):
    _input = "input_features"
    _prefix = ""
    _qkv_fmt = "self_attn.{}_proj"
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    _norm_weight_suffixes = ("norm_feed_forward1.weight", "norm_feed_forward2.weight", "norm_self_att.weight", "norm_conv.weight", "norm_out.weight",
                             "conv.norm.weight")               # run_wav2vec2.init_synthetic starts these around 1
    _conv_extractor = False                                    # log-mel features, no waveform conv stack
    # what a model of the family (lasr_model.py) replaces: the alias tables, and what nvidia_ctc_lib.dynamic_eval reads from its model
    _layer_names = LAYER_NAMES
    _head_bias_names = (("self_attn.pos_bias_u", "self_attn.bias_u"), ("self_attn.pos_bias_v", "self_attn.bias_v"))
    downsampling_factor = 8                                    # nvidia_ctc/lib.py:110: the overlap must be a multiple of it
    frozen_in_the_loop = FROZEN_IN_THE_LOOP
    frames = staticmethod(frames)                              # encoder frames of T feature frames; a model with another subsampling replaces it

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self._alias = {}
        for l in range(c["num_hidden_layers"]):                # the parent's layer code finds every parameter under the name it uses;
            p = f"encoder.layers.{l}."                         # a bias this configuration does not have is None there (a null pointer)
            for theirs, ours in self._layer_names:
                for leaf in ("weight", "bias"):
                    a, b = f"{p}{theirs}.{leaf}", f"{p}{ours}.{leaf}"
                    if theirs == "self_attn.linear_pos" and leaf == "bias":
                        continue
                    self.P[a], self.G[a] = self.P.get(b), self.G.get(b)
                    self._alias[a] = b
            for theirs, ours in self._head_bias_names:
                self.P[p + theirs], self.G[p + theirs] = self.P[p + ours], self.G[p + ours]
                self._alias[p + theirs] = p + ours
        self.n_mels, self.C, self.F3 = c["num_mel_bins"], c["subsampling_conv_channels"], c["num_mel_bins"] // 8
        self.input_scale = math.sqrt(c["hidden_size"]) if c.get("scale_input", False) else 1.0
        self._brn, self._ctx_brn = None, False             # batch_renorm_training()'s state; whether the last forward ran inside it

    def trainable(self, name):
        return super().trainable(getattr(self, "_alias", {}).get(name, name))

    def __call__(self, x=None, **kw):
        more = {"input_lengths": kw["input_lengths"]} if kw.get("input_lengths") is not None else {}
        return self.forward(kw.get(self._input, x), attention_mask=kw.get("attention_mask"), **more)

    def _make_buffers(self):
        return {n: (torch.ones if n.endswith("running_var") else torch.zeros)(shape, device=self.device, dtype=dt)
                for n, shape, dt in buffer_spec(self.cfg)}

    def _bn(self, l):
        p = f"encoder.layers.{l}.conv.norm."
        return self.buffers_[p + "running_mean"], self.buffers_[p + "running_var"]

    def _below_frozen(self):
        """True when nothing of the subsampling adapts: its backward is then not run at all."""
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith(SUB))

    # ------------------------------------------------------------------ training-mode BatchRenorm (the reference loop's conv-module norm)
    @contextlib.contextmanager
    def batch_renorm_training(self, momentum=0.001, eps=1e-5, num_batches_tracked=1_000_000):
        """Inside this context the conv modules' norm is what reference nvidia_ctc/lib.py:74,89-102 leaves in the model: a BatchRenorm1d in
        TRAINING mode (the `batchrenorm` package form; parity unpinned against upstream `lcasr`) with the reference's constants as defaults.
        On entry every layer's `running_mean` and `sqrt(running_var)` (no eps under the root, :101) are copied into loop-local device
        tensors; the returned state exposes them as lists over the layers (`running_mean`, `running_std`) next to `num_batches_tracked` (a
        list too: one counter per replaced module, as in the reference), `momentum` and `eps`.  Every forward, grad mode or not, normalises
        with the statistics of its batch (all rows, the clean copy included), corrects them by the detached r / d clamped at
        ops.batch_renorm_clamps(num_batches_tracked), moves the state's running statistics and advances the counters.  The gradient flows
        through the batch mean and deviation and so reaches every row: backward(n_active < B) is refused.
        Deviation from the reference: it leaves its replaced modules in the model and never restores anything; here the state is dropped
        on exit, and the model's own buffers and its eval-mode path are untouched throughout."""
        if self._brn is not None:
            raise ops.DynError("batch_renorm_training() is already active on this model")
        if not (0.0 <= float(momentum) <= 1.0 and float(eps) >= 0.0 and int(num_batches_tracked) >= 0):
            raise ops.DynError(f"batch_renorm_training: momentum={momentum!r} must lie in [0, 1], eps={eps!r} and "
                               f"num_batches_tracked={num_batches_tracked!r} must not be negative")
        L = self.cfg["num_hidden_layers"]
        stats = [self._bn(l) for l in range(L)]
        state = SimpleNamespace(momentum=float(momentum), eps=float(eps), num_batches_tracked=[int(num_batches_tracked)] * L,
                                running_mean=[m.clone() for m, _ in stats], running_std=[v.sqrt() for _, v in stats])
        self._brn = state
        try:
            yield state
        finally:
            self._brn = None

    def _convmod(self, l, u, w, cb, p, vT, save):
        """The bracket between the two pointwise convolutions in the model's mode: (a, gl, cv, stats); stats is None in eval mode."""
        P = self.P
        self._ctx_brn = self._brn is not None
        if self._brn is None:
            mean, var = self._bn(l)
            return ops.convmod_bn(u, w, cb, mean, var, P[p + "conv.norm.weight"], P[p + "conv.norm.bias"], "silu", BN_EPS, valid=vT, save=save) + (None,)
        st = self._brn
        rmax, dmax = ops.batch_renorm_clamps(st.num_batches_tracked[l])
        out = ops.convmod_brn(u, w, cb, st.running_mean[l], st.running_std[l], P[p + "conv.norm.weight"], P[p + "conv.norm.bias"], rmax, dmax,
                              st.momentum, "silu", st.eps, valid=vT)
        st.num_batches_tracked[l] += 1
        return out

    def _convmod_bwd(self, l, cv, stats, da, p, cbn, has_cb, vT):
        """dc of the bracket's norm and activation (over da), the norm's affine gradients accumulated."""
        P = self.P
        gw, gb, gc = self._g(p + "conv.norm.weight"), self._g(p + "conv.norm.bias"), self._g(cbn) if has_cb else None
        if stats is None:
            mean, var = self._bn(l)
            return ops.convmod_bn_bwd_act(cv, mean, var, P[p + "conv.norm.weight"], P[p + "conv.norm.bias"], da, gw, gb, gc, "silu", BN_EPS,
                                          valid=vT, out=da)
        return ops.convmod_brn_bwd(cv, stats, da, gw, gb, gc, "silu", valid=vT, out=da)

    def backward(self, grad_logits, n_active=None):
        if self._ctx_brn and isinstance(self._ctx, dict) and n_active is not None and int(n_active) < self._ctx["dims"][0]:
            raise ops.DynError(f"backward(n_active={int(n_active)}) of a batch of {self._ctx['dims'][0]} after a forward under batch_renorm_training(): "
                               "the gradient flows through the batch statistics and reaches every row; pass a gradient for all rows "
                               "(zeros where the loss has none)")
        return super().backward(grad_logits, n_active)

    # ------------------------------------------------------------------ state dict
    def _to_hf(self, name, t):
        kind = self._kind[name]
        if kind == "pw2":
            return t.reshape(*t.shape, 1, 1)
        if kind == "sublin":
            return sublin_to_hf(t, self.C, self.F3)
        return super()._to_hf(name, t)                         # "pw" / "dw": the parent's reshapes

    def load_state_dict(self, sd, strict=True):
        n = SUB + "linear.weight"
        if n in sd:
            if tuple(sd[n].shape) != (self.cfg["hidden_size"], self.C * self.F3):
                raise ops.DynError(f"{n}: shape {tuple(sd[n].shape)} in the state dict does not fit this configuration's "
                                   f"{(self.cfg['hidden_size'], self.C * self.F3)}")
            sd = dict(sd)
            sd[n] = sublin_from_hf(sd[n].to(torch.float32), self.C, self.F3)
        return super().load_state_dict(sd, strict)

    # ------------------------------------------------------------------ position table
    def position_table(self, T):
        """pe [2T - 1, H] of T encoder frames on the device; built on the host the first time T is seen, never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the position table of {T} frames has to exist before its launch sequence is captured")
            t = self._tables[T] = position_table(T, self.cfg["hidden_size"]).to(self.device)
        return t

    # ------------------------------------------------------------------ forward
    _ragged = True                                             # a model of the family without per-row frame counts says so (refused by name)
    _enc_lengths = None      # (weak reference to enc, host list, int32 [B] on the device) of the last encode() of a ragged batch

    def _remember_lengths(self, enc, out):
        """encode() of a model whose head runs in a later call: keeps the rows' encoder frame counts next to a weak reference to `enc`."""
        self._enc_lengths = (weakref.ref(enc), out.lengths, out.lengths_device) if hasattr(out, "lengths") else None

    def _lengths_of(self, enc, enc_lengths, rows):
        """The valid encoder frames of the first `rows` rows of enc as int32 on the device, or None (every frame): `enc_lengths` (a
        sequence of ints or an integer tensor [B], 1 .. T'), else what the encode() that returned this very tensor knows.  Another
        tensor of that shape while a ragged encode is remembered (a clone, a detached or contiguous copy) is refused: it would silently
        run at full lengths."""
        if enc_lengths is None:
            k = self._enc_lengths
            if k is None:
                return None
            if k[0]() is enc:
                return k[2][:rows]
            if k[0]() is not None and tuple(k[0]().shape) == tuple(enc.shape):
                raise ops.DynError("the last encode() ran a ragged batch (input_lengths) and these encoder states are another tensor of the "
                                   "same shape: pass enc_lengths (the result's `lengths`) with it")
            return None
        host = check_input_lengths(enc_lengths, enc.shape[0], enc.shape[1])
        return torch.tensor(host + [0] * (-len(host) % 4), dtype=torch.int32).to(self.device, non_blocking=True)[:rows]

    def forward(self, input_features, attention_mask=None, input_lengths=None):
        """input_features [B, T, num_mel_bins] float32 on the device -> SimpleNamespace(logits [B, T', V], frames = T'), T' = frames(T).
        `attention_mask` is refused.  `input_lengths` (None: every frame of every row is valid; else check_input_lengths): the valid
        frames per row of a ragged batch.  Frames >= input_lengths[b] of input_features are never read as data (they count as zeros,
        what the extractor's `input_features *= mask` leaves there), the result gains `lengths` (the valid encoder frames per row,
        output_lengths(..)[3], a host list) and `lengths_device` (the same, int32 [B] on the device): logits at frames < lengths[b] are
        those of the row run alone at its own length, the frames past it are finite and carry no meaning."""
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built: every frame of input_features is taken as valid (the reference loop passes whole "
                               "windows); a ragged batch passes input_lengths (parakeet_model.lengths_from_mask turns a prefix mask into them)")
        x = input_features
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == self.n_mels
                and x.shape[1] >= 1):
            raise ops.DynError(f"input_features must be a float32 CUDA tensor [B, T, {self.n_mels}]")
        B, T, _ = x.shape
        T3 = self.frames(T)
        host = lens = None
        if input_lengths is not None:
            host, lens = self._stage_lengths(input_lengths, B, T)
        self.position_table(T3)
        with ops.use_workspace(self._scratch()):
            self._vl, self._ctx_static = None, False
            ctx = {"conv": []} if torch.is_grad_enabled() else None
            h, kept = self._subsample(x.contiguous()) if lens is None else self._subsample(x.contiguous(), lens)
            if ctx is not None:
                ctx["sub"] = kept
                ctx["lens"] = lens
            out = self._encode(h, ctx, None if lens is None else ops.RowLens(lens[3]), (B, T, T3), None)
        if lens is not None:
            out.lengths, out.lengths_device = host[3], lens[3]
        return out

    def _stage_lengths(self, input_lengths, B, T):
        """(output_lengths as host lists, the same as one int32 tensor [4, B] (a view) on the device: one small copy, no synchronisation) of a ragged
        batch; what is not built with per-row frame counts is refused by name here, before any launch."""
        if not self._ragged:
            refuse_input_lengths(type(self).__name__, input_lengths)
        if self._brn is not None:
            raise ops.DynError("input_lengths inside batch_renorm_training() is not built: the batch statistics would have to leave out every "
                               "row's padded frames")
        if torch.cuda.is_current_stream_capturing():
            raise ops.DynError("input_lengths under hipGraph capture is not built: the frame counts are checked and copied on the host")
        host = output_lengths(check_input_lengths(input_lengths, B, T))
        rows = torch.zeros(4, (B + 3) // 4 * 4, dtype=torch.int32)          # every stage's counts start 16-byte aligned (the loss kernels ask for it)
        rows[:, :B] = torch.tensor(host, dtype=torch.int32)
        return host, rows.to(self.device, non_blocking=True)[:, :B]

    def _subsample(self, x, lens=None):
        """x [B, T, F] -> (h [B, T', H], what _subsample_bwd needs, batch-major).  `lens` (int32 [4, B], _stage_lengths): transformers zeroes
        the rows past a row's length after every Conv2d.  Here the two depthwise stages read their input rows past it as zeros and write
        their output rows past it as zeros (that covers the first conv's output, both large intermediates and the first pointwise conv's
        bias rows without a pass over them), the first conv reads the feature frames past it as zeros, and the small z3 behind the last
        pointwise conv gets ops.mask_rows_lens."""
        P, s = self.P, SUB
        l0, l1, l2, l3 = (None,) * 4 if lens is None else lens                                       # None: the entries without counts
        z1 = ops.conv2d_first(x, P[s + "layers.0.weight"], P[s + "layers.0.bias"], lens=l0)             # [B, T1, F1, C], pre-activation
        u2 = ops.dwconv2d_s2_act(z1, P[s + "layers.2.weight"], P[s + "layers.2.bias"], "relu", lens_in=l1, lens_out=l2)
        z2 = ops.linear(u2, P[s + "layers.3.weight"], P[s + "layers.3.bias"])
        u3 = ops.dwconv2d_s2_act(z2, P[s + "layers.5.weight"], P[s + "layers.5.bias"], "relu", lens_in=l2, lens_out=l3)
        z3 = ops.linear(u3, P[s + "layers.6.weight"], P[s + "layers.6.bias"])
        if lens is not None:
            ops.mask_rows_lens(z3, l3)
        a3 = ops.relu(z3)
        B, T3, F3, C = a3.shape
        h = ops.linear(a3.view(B, T3, F3 * C), P[s + "linear.weight"], P[s + "linear.bias"])
        if self.input_scale != 1.0:                           # (W a + b) * sqrt(H), one rounding, as transformers multiplies the linear's output
            raw, h = h, h.clone()
            ops.axpby(raw, h, 0.0, self.input_scale)
        return h, (x, z1, u2, z2, u3, z3, a3)

    def _subsample_bwd(self, kept, dh, lens=None):
        """Accumulates the subsampling's gradients from dh = dL/dh [nb, T', H]; the features are data, so nothing is returned.  `lens`
        (int32 [4, nb]): the forward's row masks run backwards: dz3 is zeroed past a row's length, each depthwise dgrad writes zeros past
        its input length and reads no du past its output length, the weight gradients read their input rows past the length as zeros."""
        P, G, s = self.P, self.G, SUB
        x, z1, u2, z2, u3, z3, a3 = kept
        B, T3, F3, C = a3.shape
        if self.input_scale != 1.0:
            d = dh.clone()
            ops.axpby(dh, d, 0.0, self.input_scale)
            dh = d
        da3 = self._lin_bwd(dh, a3.view(B, T3, F3 * C), s + "linear.weight", s + "linear.bias")
        dz3 = ops.relu_bwd(z3, da3.view(z3.shape), out=da3.view(z3.shape))
        l0, l1, l2, l3 = (None,) * 4 if lens is None else lens
        if lens is not None:
            ops.mask_rows_lens(dz3, l3)
        du3 = self._lin_bwd(dz3, u3, s + "layers.6.weight", s + "layers.6.bias")
        ops.dwconv2d_s2_wgrad_act(z2, du3, G[s + "layers.5.weight"], G[s + "layers.5.bias"], "relu", beta=1.0, lens_in=l2)
        dz2 = ops.dwconv2d_s2_dgrad_act(z2, P[s + "layers.5.weight"], du3, "relu", lens_in=l2, lens_out=l3)
        du2 = self._lin_bwd(dz2, u2, s + "layers.3.weight", s + "layers.3.bias")
        ops.dwconv2d_s2_wgrad_act(z1, du2, G[s + "layers.2.weight"], G[s + "layers.2.bias"], "relu", beta=1.0, lens_in=l1)
        dz1 = ops.dwconv2d_s2_dgrad_act(z1, P[s + "layers.2.weight"], du2, "relu", lens_in=l1, lens_out=l2)
        ops.conv2d_first_wgrad(x, dz1, G[s + "layers.0.weight"], G[s + "layers.0.bias"], beta=1.0, lens=l0)

    def _conv_fwd(self, x, l, vT, save):
        """x + conv_module(x)."""
        P = self.P
        p = f"encoder.layers.{l}."
        n, m, s = ops.layernorm(x, P[p + "norm_conv.weight"], P[p + "norm_conv.bias"], self._layer_eps)
        u = ops.linear(n, P[p + "conv.pointwise_conv1.weight"], P.get(p + "conv.pointwise_conv1.bias"))
        w, cb = P[p + "conv.depthwise_conv.weight"], P.get(p + "conv.depthwise_conv.bias")
        a, gl, cv, st = self._convmod(l, u, w, cb, p, vT, save)
        r = x.clone() if save else x
        ops.linear(a, P[p + "conv.pointwise_conv2.weight"], P.get(p + "conv.pointwise_conv2.bias"), out=r, beta=1.0)
        return r, (x, m, s, n, u, gl, cv, a, st)

    def _conv_bwd(self, dr, kept, l, vT):
        P, G = self.P, self.G
        p = f"encoder.layers.{l}."
        x, m, s, n, u, gl, cv, a, st = kept
        cbn = p + "conv.depthwise_conv.bias"
        has_cb = cbn in P
        b1, b2 = (p + f"conv.pointwise_conv{i}.bias" if has_cb else None for i in (1, 2))
        da = self._lin_bwd(dr, a, p + "conv.pointwise_conv2.weight", b2)
        w = P[p + "conv.depthwise_conv.weight"]
        dc = self._convmod_bwd(l, cv, st, da, p, cbn, has_cb, vT)
        ops.dwconv1d_wgrad(gl, dc, G[p + "conv.depthwise_conv.weight"], None, beta=1.0)
        du = ops.glu_dwconv1d_dgrad(u, w, dc, valid=vT)
        dn = self._lin_bwd(du, n, p + "conv.pointwise_conv1.weight", b1)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "norm_conv.weight"], m, s, dn, dx, G[p + "norm_conv.weight"], G[p + "norm_conv.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    def _encode(self, h, ctx, vT, dims, v0):
        P = self.P
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        logits = ops.linear(x, P["ctc_head.weight"], P["ctc_head.bias"])
        if ctx is not None:
            ctx["head"] = x
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    # ------------------------------------------------------------------ backward
    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        """ctc_head, the layers and the subsampling; returns None: nothing lies below the subsampling (the features are data)."""
        v0, vT = ctx["valid"]
        T = ctx["dims"][2]
        lens = ctx.get("lens")
        if lens is not None:                                   # a ragged batch: no gradient enters at a padded frame, whatever the caller's loss left there
            vT, lens = vT.cut(nb), lens[:, :nb]
            grad_logits = ops.mask_rows_lens(grad_logits.contiguous().clone(), lens[3])
        dx = self._lin_bwd(grad_logits.contiguous(), cut(ctx["head"]), "ctc_head.weight", "ctc_head.bias")
        dh = self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
        if not self._below_frozen():
            self._subsample_bwd(cut(ctx["sub"]), dh, *(() if lens is None else (lens,)))
        return None

    # ------------------------------------------------------------------ waveform front end (frontend.MelFeatures, csrc/melfeat.hip)
    _feature_kind = "parakeet"                                 # the extractor class of the checkpoint family (frontend.MEL_KINDS)

    def feature_extractor(self):
        """The device form of this family's transformers feature extractor at the configuration's `num_mel_bins`, built once per model."""
        fe = self.__dict__.get("_mel_features")
        if fe is None:
            from . import frontend
            fe = self._mel_features = frontend.MelFeatures(self._feature_kind, self.cfg["num_mel_bins"], self.device)
        return fe

    def features_from_audio(self, waveforms, audio_lengths=None):
        """waveforms [B, Lmax] float32 on the device (+ the valid samples per row) -> (input_features, input_lengths).  Rows with one and the
        same count of VALID FRAMES (what the extractor's mask would show; 16000 and 16100 samples are both 100 frames, so equal sample
        counts are not required):
        the features are cut to their valid frames and input_lengths is None (what a model without per-row frame counts can run);
        otherwise the extractor's [B, T, F] with zeros past each row's count, and the counts."""
        feats, lens = self.feature_extractor()(waveforms, audio_lengths)
        if len(set(lens)) == 1:
            return feats[:, :lens[0]].contiguous(), None
        return feats, lens

    def generate_from_audio(self, waveforms, audio_lengths=None, **generate_kw):
        """generate() from 16 kHz mono waveforms [B, Lmax] on the device; `audio_lengths`: the valid samples per row of a ragged batch
        (a model that refuses `input_lengths` refuses it with its own message).  `generate_kw` goes to generate() unchanged."""
        if "input_lengths" in generate_kw or "input_features" in generate_kw:
            raise ops.DynError("generate_from_audio computes input_features and input_lengths itself: pass waveforms and audio_lengths")
        feats, lens = self.features_from_audio(waveforms, audio_lengths)
        if lens is not None:
            generate_kw["input_lengths"] = lens
        return self.generate(feats, **generate_kw)

    def generate(self, input_features, input_lengths=None):
        """Greedy CTC ids as transformers' ParakeetForCTC.generate returns them: the argmax of every frame's logits [B, T'] (int64, blanks
        and repeats kept), `pad_token_id` at the frames past a row's length of a ragged batch."""
        with torch.no_grad():
            out = self.forward(input_features, input_lengths=input_lengths)
        B, T3, V = out.logits.shape
        ids = ops.argmax_rows(out.logits.view(B * T3, V))[0].view(B, T3).to(torch.int64)
        if input_lengths is not None:
            ids.masked_fill_(torch.arange(T3, device=ids.device)[None, :] >= out.lengths_device[:, None], self.cfg["pad_token_id"])
        return ids
