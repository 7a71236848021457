"""Data2VecAudioForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for
a Data2Vec-Audio checkpoint (data2vec-audio-base-960h, -large-960h), driven by the same `model(input_values).logits` (lib.py:163,413).

Data2Vec-Audio is wav2vec2's layer-norm extractor (always: transformers ignores `feat_extract_norm` here; `conv_bias` may be either value),
feature projection, POST-LN encoder (always: `do_stable_layer_norm` is ignored too) and lm_head, with another positional embedding: not one
weight-normed 128-tap grouped conv but a stack of `num_conv_pos_embeddings` (5) layers, each
    Conv1d(H, H, k = conv_pos_kernel_size (19), padding = k // 2, groups = G) -> [drop the last frame when k is even]
    -> LayerNorm(H, elementwise_affine=False, eps = 1e-5) over channels -> GELU
(transformers Data2VecAudioPositionalConvLayer).  This subclass of Wav2Vec2ForCTC replaces the prefix (`data2vec_audio.`), the configuration
reader, the positional conv's entries of the parameter list and the hook pair _pos_embed / _pos_embed_bwd.  Per layer the forward is the
grouped GEMM on the packed input [B, G, T + 2 pad, cg] and ONE kernel (ops.posconv_ln_gelu: bias, LayerNorm, GELU, and the next layer's
packed, zero-padded input written directly; the last layer writes the token-major activation for the residual add); the backward is ONE
kernel (ops.posconv_ln_gelu_bwd: GELU', LayerNorm backward, the bias's column sums, dyg in the GEMMs' layout), the per-sample
weight-gradient GEMMs, the data-gradient GEMM, col2im and the unpack of the input gradient.
Under bucketed hipGraph replay every layer's output is masked past the utterance by the kernel's `valid` argument: the rows just past the
last frame see valid rows through the conv and are not zero on their own, while the next layer must find its zero padding there.  The
backward kernel writes exact zeros on those rows whatever their incoming gradient holds, so only the stack's input gradient is masked.
Eval mode only, as the reference loop: no dropout, layerdrop or SpecAugment masking; no attention_mask (the reference passes none)."""
import torch

from . import ops
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(W2.DEFAULT_CONFIG, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, add_adapter=False, mask_time_prob=0.05,
                      mask_feature_prob=0.0)
POS_LN_EPS = 1e-5          # nn.LayerNorm's default: the positional layers' norm is not built with config.layer_norm_eps


def make_config(cfg=None):
    """wav2vec2_model.make_config with Data2Vec-Audio's keys (`conv_pos_kernel_size`; `num_conv_pos_embeddings` counts LAYERS here), the
    extractor forced to the layer-norm one and the encoder to post-LN whatever the source says, and `conv_bias` free."""
    src = W2.config_dict(cfg, tuple(DEFAULT_CONFIG) + tuple(W2.LAYOUT_FLAGS))
    if src.get("add_adapter", False):
        raise ops.DynError("add_adapter=true is not built: the adapter's strided convs between the encoder and lm_head are missing")
    conv_bias = bool(src.get("conv_bias", False))
    out = W2.make_config(dict(src, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=False), DEFAULT_CONFIG)
    out["conv_bias"] = conv_bias
    n, k = out["num_conv_pos_embeddings"], out["conv_pos_kernel_size"] = int(out["num_conv_pos_embeddings"]), int(out["conv_pos_kernel_size"])
    if n < 1 or k < 1:
        raise ops.DynError(f"num_conv_pos_embeddings={n} layers of conv_pos_kernel_size={k} taps: both must be at least 1")
    out["mask_time_prob"], out["mask_feature_prob"] = float(out["mask_time_prob"]), float(out["mask_feature_prob"])
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def param_spec(c, pf="data2vec_audio."):
    """wav2vec2_model.param_spec under Data2Vec-Audio's prefix with the positional conv's three entries replaced, in place, by
    `encoder.pos_conv_embed.layers.{i}.conv.weight` (kind "conv": kept as [H][k][cg], HF [H, cg, k]) and `.bias` per layer; no weight norm.
    `masked_spec_embed` exists only when a masking probability is positive, as in transformers (never used in eval mode)."""
    H, G, k = c["hidden_size"], c["num_conv_pos_embedding_groups"], c["conv_pos_kernel_size"]
    old = pf + "encoder.pos_conv_embed.conv."
    spec = []
    for entry in W2.param_spec(c, pf):
        if entry[0] == pf + "masked_spec_embed" and not (c["mask_time_prob"] > 0.0 or c["mask_feature_prob"] > 0.0):
            continue
        if not entry[0].startswith(old):
            spec.append(entry)
        elif entry[0] == old + "bias":                         # the first of the three
            for i in range(c["num_conv_pos_embeddings"]):
                p = f"{pf}encoder.pos_conv_embed.layers.{i}.conv."
                spec += [(p + "weight", (H, k, H // G), "conv"), (p + "bias", (H,), None)]
    return spec


class Data2VecAudioForCTC(W2.Wav2Vec2ForCTC):
    _prefix = "data2vec_audio."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)

    def __init__(self, config=None, device="cuda:0"):
        c = self._make_config(config)
        H, G = c["hidden_size"], c["num_conv_pos_embedding_groups"]
        if H % 256 or H > 1024 or G < 1 or H % G or (H // G) % 4:
            raise ops.DynError(f"the positional conv kernels need hidden_size % 256 == 0 up to 1024 and hidden_size / "
                               f"num_conv_pos_embedding_groups a multiple of 4 (got {H} / {G})")
        super().__init__(config, device)

    def _pos_names(self, i):
        p = f"{self._prefix}encoder.pos_conv_embed.layers.{i}.conv."
        return p + "weight", p + "bias"

    def _pos_embed(self, h, vT):
        c, P = self.cfg, self.P
        B, T, H = h.shape
        n, K, G = c["num_conv_pos_embeddings"], c["conv_pos_kernel_size"], c["num_conv_pos_embedding_groups"]
        cg, pad = H // G, K // 2
        Tp = T + 2 * pad                                            # k even: the conv has T + 1 outputs, M = T drops the last one
        xg = ops.group_pack(h, G, pad)                              # [B, G, T + 2 pad, cg]; layers 1.. get theirs from the fused kernel
        kept = []
        for i in range(n):
            wn, bn = self._pos_names(i)
            yg = torch.empty(B, G, T, cg, device=h.device, dtype=torch.float32)
            ops.gemm(xg, P[wn], yg, trans_b=True, M=T, N=cg, K=K * cg, lda=cg, ldb=K * cg, ldc=cg, nb1=B, nb2=G,
                     sa=(G * Tp * cg, Tp * cg), sb=(0, cg * K * cg), sc=(G * T * cg, T * cg))
            last = i == n - 1
            pos, nxt, mean, rstd = ops.posconv_ln_gelu(yg, P[bn], T, pad, POS_LN_EPS, valid=vT, want_act=last, want_packed=not last)
            kept.append((xg, yg, mean, rstd))
            xg = nxt
        return pos, (tuple(kept),)

    def _pos_embed_bwd(self, kept, dhs, nb, cut, vT):
        c, P, G = self.cfg, self.P, self.G
        T, H = dhs.shape[1], dhs.shape[2]
        n, K, Gn = c["num_conv_pos_embeddings"], c["conv_pos_kernel_size"], c["num_conv_pos_embedding_groups"]
        cg, pad = H // Gn, K // 2
        Tp = T + 2 * pad
        layers = cut(kept[0])
        dact = dhs                                                   # dL/d(h + pos) is dL/dpos; read only until layer 0 adds its path to it
        for i in reversed(range(n)):
            xg, yg, mean, rstd = layers[i]
            wn, bn = self._pos_names(i)
            dyg = ops.posconv_ln_gelu_bwd(yg, P[bn], mean, rstd, dact, G[bn] if self.trainable(bn) else None, wgrad_beta=1.0, valid=vT)
            for b in range(nb if self.trainable(wn) else 0):         # dw[g] += dyg[b, g]^T rows(xg[b, g])
                ops.gemm(dyg, xg, G[wn], trans_a=True, M=cg, N=K * cg, K=T, lda=cg, ldb=cg, ldc=K * cg, nb1=1, nb2=Gn,
                         sa=(0, T * cg), sb=(0, Tp * cg), sc=(0, cg * K * cg), a_off=b * Gn * T * cg, b_off=b * Gn * Tp * cg, beta=1.0)
            dA = torch.empty(nb, Gn, T, K * cg, device=dhs.device, dtype=torch.float32)
            ops.gemm(dyg, P[wn], dA, M=T, N=K * cg, K=cg, lda=cg, ldb=K * cg, ldc=K * cg, nb1=nb, nb2=Gn, sa=(Gn * T * cg, T * cg),
                     sb=(0, cg * K * cg), sc=(Gn * T * K * cg, T * K * cg))
            dxg = torch.empty(nb * Gn, Tp, cg, device=dhs.device, dtype=torch.float32)
            ops.col2im_1d(dA, dxg, nb * Gn, Tp, T, cg, K, 1)
            if i > 0:                                                # rows past `vT` of it are never read: the fused backward zeroes them
                dact = ops.group_unpack_grad(dxg.view(nb, Gn, Tp, cg), torch.empty_like(dhs), pad, beta=0.0)
            else:
                ops.group_unpack_grad(dxg.view(nb, Gn, Tp, cg), dhs, pad, beta=1.0)   # dh (pre-pos) = dhs (residual) + the stack's path
        if vT is not None:
            ops.mask_rows(dhs, vT)                                   # the windows of the last valid frames reach into the zeroed tail: no gradient there
        return dhs
