"""LasrForCTC on MI355X: the conformer encoder + CTC head of google/medasr (`model_type: "lasr_ctc"`, transformers modeling_lasr.py), the
second model family of the reference's third loop (nvidia_ctc/lib.py driven through nvidia_ctc_lib.dynamic_eval), as `AutoModelForCTC`
builds it in plain torch.  No attention mask; the conv modules' norm reads its running statistics by default (eval mode).  The reference loop
itself replaces that norm by a training-mode BatchRenorm1d (nvidia_ctc/lib.py:74,89-102): ParakeetForCTC.batch_renorm_training(), inherited
here at 32 taps, runs it; eval mode remains the default until a maintainer flips it.

transformers derives LasrForCTC from ParakeetForCTC, and so does this module: flat parameters, the batch-norm buffers outside the flat
vector, the alias table that lets Wav2Vec2ConformerForCTC's layer loop find every parameter under the name it uses (LAYER_NAMES), the
deferred reductions and the active-subset backward are the parents'.  What differs from Parakeet:
  * subsampling (LasrEncoderSubsampling, x4): dense_0 -> ReLU -> 2 x [valid Conv1d (5 taps, stride 2) + bias -> ReLU] -> dense_1.  The
    convolutions are the wav2vec2 extractor's implicit GEMM (ops.gemm over overlapping rows) with the bias in the GEMM's epilogue, their
    backward ops.conv1d_wgrad / conv1d_dgrad; a Conv1d weight [Cout, Cin, 5] lives as [Cout, 5, Cin] (channels-last rows) in the flat vector
    and is permuted, bit for bit, in state_dict() / load_state_dict() / grads_hf() (the parent's kind "conv").
  * attention: plain q k^T / sqrt(D) scores with Llama-style rotary applied to q and k AFTER their projections: q | k are the first 2H
    floats of every 3H-float row of the packed projection, so ops.rotary(qkv, cos, sin, B, T, 2 nh, D, 3H) turns both in one launch
    (x cos + rotate_half(x) sin, halves not interleaved: transformers' apply_rotary_pos_emb) and `inverse=True` on dqkv is the backward.
    The (cos, sin) [T, D / 2] table is LasrEncoderRotaryEmbedding's own torch expressions on the host (rotary_table), cached per frame count,
    never built inside a capture.
  * weighted residuals: x <- a x + b branch(x), (a, b) = feed_forward_residual_weights (1.5, 0.5) around both FFNs and
    conv_residual_weights (2, 1) around the conv module; attention keeps 1 + 1.  A bias-free closing projection writes alpha = b, beta = a
    from its GEMM into a copy of x; with a bias (which alpha must not scale) ops.axpby combines.  Backward: the branch's output gradient is
    b dr, the pass-through a dr rides on the LayerNorm backward's dx = grad + dx_beta * dx_in.
  * conv module: the fused core of csrc/convmod_bn.hip at 32 taps (padding="same" of an even kernel: 15 frames left, 16 right; the data
    gradient 16 | 15) + ops.dwconv1d_wgrad at 32 taps.
  * every LayerNorm is bias-free (a null beta / dbeta pointer) with config.layer_norm_eps (1e-6); BatchNorm keeps torch's 1e-5.
  * `encoder.out_norm` closes the encoder in front of `ctc_head`.
  * no `scale_input`, no position projection, no per-head biases.

Not built, refused by name before any launch: `conv_kernel_size` != 32, `subsampling_conv_kernel_size` != 5, `subsampling_conv_stride` != 2,
`hidden_size` outside 256 / 512 / 768 / 1024, `hidden_act` != "silu", `num_key_value_heads` != `num_attention_heads`, an odd head
dimension, a `rope_type` other than "default", residual-weight lists that are not two numbers, `subsampling_conv_channels` / `num_mel_bins`
that are no multiple of 4 (the GEMM's 16-byte operand rows), fewer than 13 feature frames, an `attention_mask` argument.
LasrFeatureExtractor, LasrEncoder as a bare encoder, bucketed hipGraph replay and lockstep groups are out of scope.  No hub checkpoint is on
the machine: transformers' LasrForCTC on the CPU with the same (random) state dict is the oracle in the tests."""
from types import SimpleNamespace

import torch

from . import _attn, ops
from . import parakeet_model as PM
from . import wav2vec2_model as W2

ENCODER_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act", "attention_bias",
                "convolution_bias", "conv_kernel_size", "subsampling_conv_channels", "num_mel_bins", "subsampling_conv_kernel_size",
                "subsampling_conv_stride", "max_position_embeddings", "layer_norm_eps", "feed_forward_residual_weights",
                "conv_residual_weights", "rope_parameters", "num_key_value_heads", "head_dim")
DEFAULT_CONFIG = dict(hidden_size=512, num_hidden_layers=17, num_attention_heads=8, intermediate_size=2048, hidden_act="silu",
                      attention_bias=False, convolution_bias=False, conv_kernel_size=32, subsampling_conv_channels=256, num_mel_bins=128,
                      subsampling_conv_kernel_size=5, subsampling_conv_stride=2, max_position_embeddings=10000, layer_norm_eps=1e-6,
                      feed_forward_residual_weights=(1.5, 0.5), conv_residual_weights=(2.0, 1.0),
                      rope_parameters={"rope_theta": 10000.0, "rope_type": "default"}, num_key_value_heads=None, head_dim=None,
                      vocab_size=512, pad_token_id=0)
WIDTHS = PM.WIDTHS                     # instances of dyn_convmod_bn_* (and of the LayerNorm kernels)
CONV_KERNEL = 32
SUB_KERNEL, SUB_STRIDE = 5, 2
MIN_FRAMES = (SUB_KERNEL - 1) * SUB_STRIDE + SUB_KERNEL          # 13: the two valid convolutions' receptive field
BN_EPS = PM.BN_EPS
# the grandparent's name of a layer's parameter group -> transformers' (LasrEncoderBlock): Parakeet's table without the position projection
LAYER_NAMES = tuple((a, b) for a, b in PM.LAYER_NAMES if a != "self_attn.linear_pos")
SUB = "encoder.subsampler."
FROZEN_IN_THE_LOOP = (SUB, "ctc_head.")          # nvidia_ctc/lib.py:81-86 on this family: the subsampling and the head do not adapt


def _pair_of_numbers(out, key):
    v = out[key]
    if not (isinstance(v, (list, tuple)) and len(v) == 2 and all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v)):
        raise ops.DynError(f"{key}={v!r} is not built: a list of two numbers (residual weight, branch weight)")
    out[key] = (float(v[0]), float(v[1]))


def make_config(cfg=None):
    """transformers' LasrCTCConfig / LasrEncoderConfig keys with their defaults, from the configuration object, its dict (`encoder_config`
    nested) or a flat dict; what this forward does not build is refused by name."""
    out = W2.make_config(PM._flatten(cfg, ENCODER_KEYS), DEFAULT_CONFIG)
    out["do_stable_layer_norm"] = False
    out["position_embeddings_type"] = "rotary"               # the grandparent's switch: no Transformer-XL extras in the layer loop
    out["conv_kernel"], out["conv_stride"], out["conv_dim"] = (), (), ()     # no waveform conv stack (_conv_extractor = False)
    k = out["conv_kernel_size"] = int(out["conv_kernel_size"])
    if k != CONV_KERNEL:
        raise ops.DynError(f"conv_kernel_size={k} is not built ({CONV_KERNEL})")
    if out["subsampling_conv_kernel_size"] != SUB_KERNEL:
        raise ops.DynError(f"subsampling_conv_kernel_size={out['subsampling_conv_kernel_size']} is not built ({SUB_KERNEL})")
    if out["subsampling_conv_stride"] != SUB_STRIDE:
        raise ops.DynError(f"subsampling_conv_stride={out['subsampling_conv_stride']} is not built ({SUB_STRIDE})")
    H, nh = out["hidden_size"], out["num_attention_heads"]
    if H not in WIDTHS:
        raise ops.DynError(f"hidden_size={H} is not built: one of {WIDTHS}")
    if out["hidden_act"] != "silu":
        raise ops.DynError(f"hidden_act={out['hidden_act']!r} is not built (\"silu\")")
    if not (isinstance(nh, int) and nh > 0) or H % nh:
        raise ops.DynError(f"hidden_size={H} is not a multiple of num_attention_heads={nh}")
    kv = out["num_key_value_heads"]
    if kv is not None and kv != nh:
        raise ops.DynError(f"num_key_value_heads={kv} is not built: it must equal num_attention_heads={nh}")
    hd = out["head_dim"]
    if hd is not None and hd != H // nh:
        raise ops.DynError(f"head_dim={hd} is not built: it must equal hidden_size / num_attention_heads = {H // nh}")
    if (H // nh) % 2:
        raise ops.DynError(f"head_dim = hidden_size / num_attention_heads = {H // nh} is not built: rotary embeddings need an even head dimension")
    out["num_key_value_heads"], out["head_dim"] = nh, H // nh
    rp = out["rope_parameters"]
    rp = dict(DEFAULT_CONFIG["rope_parameters"]) if rp is None else dict(rp)
    if rp.get("rope_type", "default") != "default":
        raise ops.DynError(f"rope_parameters: rope_type={rp.get('rope_type')!r} is not built (\"default\")")
    out["rope_parameters"] = {"rope_type": "default", "rope_theta": float(rp.get("rope_theta", 10000.0))}
    _pair_of_numbers(out, "feed_forward_residual_weights")
    _pair_of_numbers(out, "conv_residual_weights")
    for key in ("subsampling_conv_channels", "num_mel_bins"):
        v = out[key]
        if not (isinstance(v, int) and v > 0 and v % 4 == 0):
            raise ops.DynError(f"{key}={v!r} is not built: a positive multiple of 4 (the GEMM reads its operands in 16-byte rows)")
    out["attention_bias"], out["convolution_bias"] = bool(out["attention_bias"]), bool(out["convolution_bias"])
    out["layer_norm_eps"] = float(out["layer_norm_eps"])
    return out


def config_from_json(path):
    """An HF `config.json` of a lasr_ctc checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def frames(T):
    """Encoder frames of T feature frames: two valid 5-wide stride-2 convolutions (transformers' _get_subsampling_output_length)."""
    for _ in range(2):
        T = (T - SUB_KERNEL) // SUB_STRIDE + 1
    return T


def rotary_table(T, D, theta=10000.0):
    """(cos, sin) [T, D / 2] float32 on the host: LasrEncoderRotaryEmbedding (rope_type "default") for positions 0 .. T - 1 in its own dtypes
    and operation order.  transformers returns cat((freqs, freqs)).cos() / .sin() [T, D]; ops.rotary's half-split convention reads the first
    half, which holds the same floats as the second."""
    if not isinstance(T, int) or T < 1:
        raise ops.DynError(f"rotary_table: T={T!r} must be a positive integer")
    inv_freq = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    position_ids = torch.arange(T).unsqueeze(0)
    freqs = (inv_freq[None, :, None].float().expand(1, -1, 1) @ position_ids[:, None, :].float()).transpose(1, 2)
    return freqs.cos()[0].contiguous(), freqs.sin()[0].contiguous()


def param_spec(c, pf=""):
    """[(name, shape, kind)] in transformers' names.  kind "pw": a k = 1 Conv1d kernel kept as [C_out, C_in]; "dw": the depthwise kernel kept
    as [C, k] (both reshapes); "conv": a Conv1d kernel [C_out, C_in, k] kept as [C_out, k, C_in] (a permutation)."""
    H, I, k = c["hidden_size"], c["intermediate_size"], c["conv_kernel_size"]
    C, F = c["subsampling_conv_channels"], c["num_mel_bins"]
    ab, cb = c["attention_bias"], c["convolution_bias"]
    lin = lambda p, n, m, b=True, kind=None: [(p + ".weight", (n, m), kind)] + ([(p + ".bias", (n,), None)] if b else [])           # noqa: E731
    ln = lambda p: [(p + ".weight", (H,), None)]                                                                                       # noqa: E731
    s = pf + SUB
    spec = lin(s + "dense_0", H, F)
    spec += [(s + "conv_0.weight", (H, SUB_KERNEL, H), "conv"), (s + "conv_0.bias", (H,), None)]
    spec += [(s + "conv_1.weight", (C, SUB_KERNEL, H), "conv"), (s + "conv_1.bias", (C,), None)]
    spec += lin(s + "dense_1", H, C)
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}."
        spec += ln(p + "norm_feed_forward1") + lin(p + "feed_forward1.linear1", I, H, ab) + lin(p + "feed_forward1.linear2", H, I, ab)
        spec += ln(p + "norm_self_att")
        spec += [(p + f"self_attn.{n}_proj.weight", (H, H), None) for n in "qkv"]                  # q | k | v side by side
        spec += [(p + f"self_attn.{n}_proj.bias", (H,), None) for n in "qkv"] if ab else []
        spec += lin(p + "self_attn.o_proj", H, H, ab)
        spec += ln(p + "norm_conv") + lin(p + "conv.pointwise_conv1", 2 * H, H, cb, "pw")
        spec += [(p + "conv.depthwise_conv.weight", (H, k), "dw")] + ([(p + "conv.depthwise_conv.bias", (H,), None)] if cb else [])
        spec += [(p + "conv.norm.weight", (H,), None), (p + "conv.norm.bias", (H,), None)] + lin(p + "conv.pointwise_conv2", H, H, cb, "pw")
        spec += ln(p + "norm_feed_forward2") + lin(p + "feed_forward2.linear1", I, H, ab) + lin(p + "feed_forward2.linear2", H, I, ab)
        spec += ln(p + "norm_out")
    spec += ln(pf + "encoder.out_norm")
    return spec + [(pf + "ctc_head.weight", (c["vocab_size"], H), "pw"), (pf + "ctc_head.bias", (c["vocab_size"],), None)]


buffer_spec = PM.buffer_spec           # the batch norms' buffers carry Parakeet's names (`encoder.layers.{l}.conv.norm.*`)


class LasrForCTC(PM.ParakeetForCTC):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    _norm_weight_suffixes = PM.ParakeetForCTC._norm_weight_suffixes + ("out_norm.weight",)
    _layer_names = LAYER_NAMES
    _head_bias_names = ()
    downsampling_factor = 4                                    # two stride-2 stages
    _feature_kind = "lasr"                                     # LasrFeatureExtractor (frontend.MelFeatures)
    frozen_in_the_loop = FROZEN_IN_THE_LOOP
    frames = staticmethod(frames)

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self._layer_eps = c["layer_norm_eps"]                  # every LayerNorm of this family takes the configuration's eps
        self.ffn_weights, self.conv_weights = c["feed_forward_residual_weights"], c["conv_residual_weights"]

    def _below_frozen(self):
        """True when nothing of the subsampling adapts: its backward is then not run at all."""
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith(SUB))

    # ------------------------------------------------------------------ rotary table
    def position_table(self, T):
        """(cos, sin) [T, D / 2] of T encoder frames on the device; built on the host the first time T is seen, never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the rotary table of {T} frames has to exist before its launch sequence is captured")
            c = self.cfg
            t = self._tables[T] = tuple(x.to(self.device) for x in rotary_table(T, c["head_dim"], c["rope_parameters"]["rope_theta"]))
        return t

    # ------------------------------------------------------------------ forward
    _ragged = False

    def forward(self, input_features, attention_mask=None, input_lengths=None):
        """input_features [B, T, num_mel_bins] float32 on the device, T >= 13 -> SimpleNamespace(logits [B, T', V], frames = T'),
        T' = frames(T).  Every row is valid: `attention_mask` and `input_lengths` are refused."""
        PM.refuse_input_lengths("LasrForCTC", input_lengths)
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built: every frame of input_features is taken as valid (the reference loop passes whole windows)")
        x = input_features
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == self.n_mels):
            raise ops.DynError(f"input_features must be a float32 CUDA tensor [B, T, {self.n_mels}]")
        B, T, _ = x.shape
        if T < MIN_FRAMES:
            raise ops.DynError(f"input_features of {T} frames are shorter than the subsampling's receptive field ({MIN_FRAMES} frames)")
        T2 = frames(T)
        self.position_table(T2)
        with ops.use_workspace(self._scratch()):
            self._vl, self._ctx_static = None, False
            ctx = {"conv": []} if torch.is_grad_enabled() else None
            h, kept = self._subsample(x.contiguous())
            if ctx is not None:
                ctx["sub"] = kept
            return self._encode(h, ctx, None, (B, T, T2), None)

    @staticmethod
    def _conv5(x, w, bias):
        """ops.conv1d (valid, 5 taps, stride 2: an implicit GEMM over overlapping rows) with the bias in the GEMM's epilogue."""
        B, T, Cin = x.shape
        Cout, Tout = w.shape[0], ops.conv1d_out_len(T, SUB_KERNEL, SUB_STRIDE)
        y = torch.empty(B, Tout, Cout, device=x.device, dtype=torch.float32)
        ops.gemm(x, w, y, trans_b=True, M=Tout, N=Cout, K=SUB_KERNEL * Cin, lda=SUB_STRIDE * Cin, ldb=SUB_KERNEL * Cin, ldc=Cout, nb1=B,
                 sa=(T * Cin, 0), sc=(Tout * Cout, 0), bias=bias)
        return y

    def _subsample(self, x):
        """x [B, T, F] -> (h [B, T', H], what _subsample_bwd needs, batch-major).  Each ReLU runs in place: its output is its own mask."""
        P, s = self.P, SUB
        w0, w1 = P[s + "conv_0.weight"], P[s + "conv_1.weight"]
        a0 = ops.linear(x, P[s + "dense_0.weight"], P[s + "dense_0.bias"])
        ops.relu(a0, out=a0)
        a1 = self._conv5(a0, w0.view(w0.shape[0], -1), P[s + "conv_0.bias"])
        ops.relu(a1, out=a1)
        a2 = self._conv5(a1, w1.view(w1.shape[0], -1), P[s + "conv_1.bias"])
        ops.relu(a2, out=a2)
        return ops.linear(a2, P[s + "dense_1.weight"], P[s + "dense_1.bias"]), (x, a0, a1, a2)

    def _subsample_bwd(self, kept, dh):
        """Accumulates the subsampling's gradients from dh = dL/dh [nb, T', H]; the features are data, so nothing is returned."""
        P, G, s = self.P, self.G, SUB
        x, a0, a1, a2 = kept
        d = self._lin_bwd(dh, a2, s + "dense_1.weight", s + "dense_1.bias")
        for a_in, a_out, name in ((a1, a2, "conv_1"), (a0, a1, "conv_0")):
            w, gw = P[f"{s}{name}.weight"], G[f"{s}{name}.weight"]
            dz = ops.relu_bwd(a_out, d, out=d)
            ops.conv1d_wgrad(a_in, dz, gw.view(gw.shape[0], -1), SUB_KERNEL, SUB_STRIDE, beta=1.0)
            ops.colsum(dz, G[f"{s}{name}.bias"], beta=1.0)
            d = ops.conv1d_dgrad(dz, w.view(w.shape[0], -1), a_in.shape[1], a_in.shape[2], SUB_KERNEL, SUB_STRIDE)
        dz0 = ops.relu_bwd(a0, d, out=d)
        self._lin_bwd(dz0, x, s + "dense_0.weight", s + "dense_0.bias", need_dx=False)

    def _weighted_out(self, x, a, wname, bname, weights, save):
        """weights[0] * x + weights[1] * (a @ W^T + bias): from the GEMM's alpha / beta where the projection has no bias, else ops.axpby."""
        P = self.P
        ra, rb = weights
        r = x.clone() if save else x
        bias = P.get(bname)
        if bias is None:
            return ops.linear(a, P[wname], None, out=r, alpha=rb, beta=ra)
        return ops.axpby(ops.linear(a, P[wname], bias), r, rb, ra)

    @staticmethod
    def _branch_grad(dr, rb):
        """rb * dr, the gradient of a weighted branch's output (out of place: dr is the pass-through's source)."""
        if rb == 1.0:
            return dr
        d = dr.clone()
        return ops.axpby(dr, d, 0.0, rb)

    def _ffn_fwd(self, x, p, which, save):
        """a x + b ffn(LN(x)), (a, b) = feed_forward_residual_weights; returns (result, saved)."""
        P = self.P
        n, m, s = ops.layernorm(x, P[f"{p}{which}_layer_norm.weight"], None, self._layer_eps)
        u = ops.linear(n, P[f"{p}{which}.intermediate_dense.weight"], P[f"{p}{which}.intermediate_dense.bias"])
        a = self._act(u)
        r = self._weighted_out(x, a, f"{p}{which}.output_dense.weight", f"{p}{which}.output_dense.bias", self.ffn_weights, save)
        return r, (x, m, s, n, u, a)

    def _ffn_bwd(self, dr, kept, p, which):
        P, G = self.P, self.G
        x, m, s, n, u, a = kept
        da = self._lin_bwd(self._branch_grad(dr, self.ffn_weights[1]), a, f"{p}{which}.output_dense.weight", f"{p}{which}.output_dense.bias")
        du = self._act_bwd(u, da, out=da)
        dn = self._lin_bwd(du, n, f"{p}{which}.intermediate_dense.weight", f"{p}{which}.intermediate_dense.bias")
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[f"{p}{which}_layer_norm.weight"], m, s, dn, dx, G[f"{p}{which}_layer_norm.weight"], None,
                          dx_beta=self.ffn_weights[0], dx_in=dr)
        return dx

    def _attn_fwd(self, x, l, vT, tab, save):
        """x + o_proj(attn(LN(x))), rotary on q | k after the packed projection."""
        c, P = self.cfg, self.P
        B, T, H = x.shape
        nh = c["num_attention_heads"]
        D = H // nh
        p = f"encoder.layers.{l}."
        cos, sin = tab
        n, m, s = ops.layernorm(x, P[p + "norm_self_att.weight"], None, self._layer_eps)
        Wqkv, bqkv = self.Pqkv[l]
        qkv = torch.empty(B, T, 3 * H, device=x.device, dtype=torch.float32)
        ops.linear(n, Wqkv, bqkv, out=qkv)
        ops.rotary(qkv, cos, sin, B, T, 2 * nh, D, 3 * H)       # q | k: the first 2H floats of every row, 2 nh heads of D
        q, k, v = (_attn.packed(qkv, j, D) for j in range(3))
        S = torch.empty(B, nh, T, T, device=x.device, dtype=torch.float32)
        _attn.scores(q, k, S, D ** -0.5)
        ops.softmax(S, out=S, valid=vT)
        O = torch.empty(B, T, H, device=x.device, dtype=torch.float32)
        _attn.context(S, v, _attn.plain(O, D))
        r = x.clone() if save else x
        ops.linear(O, P[p + "self_attn.o_proj.weight"], P.get(p + "self_attn.o_proj.bias"), out=r, beta=1.0)
        return r, (x, m, s, n, qkv, S, O)

    def _attn_bwd(self, dr, kept, pos, l, nb, T, tab, vT=None):
        c, P, G = self.cfg, self.P, self.G
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        p = f"encoder.layers.{l}."
        cos, sin = tab
        x, m, s, n, qkv, S, O = kept[:7]
        Wqkv = self.Pqkv[l][0]
        gW, gb = self.Gqkv[l]
        M = nb * T
        dO = self._lin_bwd(dr, O, p + "self_attn.linear_out.weight", p + "self_attn.linear_out.bias")
        dqkv = torch.empty_like(qkv)
        (q, k, v), (dq, dk, dv) = ([_attn.packed(t, j, D) for j in range(3)] for t in (qkv, dqkv))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)                # dP is now dS, the gradient of the pre-softmax sum
        _attn.grad_qk(dP, q, k, dq, dk, D ** -0.5)               # with respect to the ROTATED q | k ...
        ops.rotary(dqkv, cos, sin, nb, T, 2 * nh, D, 3 * H, inverse=True)     # ... and through the rotation's transpose to the projections' outputs
        self._wgrad(dqkv.view(M, 3 * H), n.view(M, H), gW, gb)
        dn = torch.empty_like(dr)
        ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "norm_self_att.weight"], m, s, dn, dx, G[p + "norm_self_att.weight"], None, dx_beta=1.0, dx_in=dr)
        return dx

    def _conv_fwd(self, x, l, vT, save):
        """a x + b conv_module(LN(x)), (a, b) = conv_residual_weights."""
        P = self.P
        p = f"encoder.layers.{l}."
        n, m, s = ops.layernorm(x, P[p + "norm_conv.weight"], None, self._layer_eps)
        u = ops.linear(n, P[p + "conv.pointwise_conv1.weight"], P.get(p + "conv.pointwise_conv1.bias"))
        w, cb = P[p + "conv.depthwise_conv.weight"], P.get(p + "conv.depthwise_conv.bias")
        a, gl, cv, st = self._convmod(l, u, w, cb, p, vT, save)
        r = self._weighted_out(x, a, p + "conv.pointwise_conv2.weight", p + "conv.pointwise_conv2.bias", self.conv_weights, save)
        return r, (x, m, s, n, u, gl, cv, a, st)

    def _conv_bwd(self, dr, kept, l, vT):
        P, G = self.P, self.G
        p = f"encoder.layers.{l}."
        x, m, s, n, u, gl, cv, a, st = kept
        cbn = p + "conv.depthwise_conv.bias"
        has_cb = cbn in P
        b1, b2 = (p + f"conv.pointwise_conv{i}.bias" if has_cb else None for i in (1, 2))
        d = self._branch_grad(dr, self.conv_weights[1])
        da = self._lin_bwd(d, a, p + "conv.pointwise_conv2.weight", b2)
        w = P[p + "conv.depthwise_conv.weight"]
        dc = self._convmod_bwd(l, cv, st, da, p, cbn, has_cb, vT)
        ops.dwconv1d_wgrad(gl, dc, G[p + "conv.depthwise_conv.weight"], None, beta=1.0)
        du = ops.glu_dwconv1d_dgrad(u, w, dc, valid=vT)
        dn = self._lin_bwd(du, n, p + "conv.pointwise_conv1.weight", b1)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "norm_conv.weight"], m, s, dn, dx, G[p + "norm_conv.weight"], None, dx_beta=self.conv_weights[0], dx_in=dr)
        return dx

    def _encode(self, h, ctx, vT, dims, v0):
        P = self.P
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        hN, mean, rstd = ops.layernorm(x, P["encoder.out_norm.weight"], None, self._layer_eps)
        logits = ops.linear(hN, P["ctc_head.weight"], P["ctc_head.bias"])
        if ctx is not None:
            ctx["final"] = (x, mean, rstd)
            ctx["head"] = hN
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    # ------------------------------------------------------------------ backward
    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        """ctc_head, out_norm, the layers and the subsampling; returns None: nothing lies below the subsampling (the features are data)."""
        v0, vT = ctx["valid"]
        P = self.P
        T = ctx["dims"][2]
        dh = self._lin_bwd(grad_logits.contiguous(), cut(ctx["head"]), "ctc_head.weight", "ctc_head.bias")
        x, mean, rstd = cut(ctx["final"])
        dx = torch.empty_like(dh)
        ops.layernorm_bwd(x, P["encoder.out_norm.weight"], mean, rstd, dh, dx, self._g("encoder.out_norm.weight"), None, dx_beta=0.0)
        dh = self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
        if not self._below_frozen():
            self._subsample_bwd(cut(ctx["sub"]), dh)
        return None
