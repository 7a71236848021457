"""SEWForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for a SEW
checkpoint (asapp/sew-small-100k-ft-ls100h, sew-mid-100k-ft-ls100h), driven by the same `model(input_values).logits` (lib.py:163,413).

SEW (transformers SEWForCTC) is wav2vec2's feature extractor (either layout, usually narrower: conv_dim 64 -> 512 with kernel-1 layers),
post-LN transformer layers and lm_head around a SQUEEZED encoder: the layers run at T2 = T // s frames (s = `squeeze_factor`).
    a   = LayerNorm_{conv_dim[-1]}(extractor(x))             `sew.layer_norm`
    h   = Linear(a)                                          `sew.feature_projection`, present only when conv_dim[-1] != hidden_size
    pos = gelu(conv_s(h))                                    the weight-normed grouped conv with STRIDE s, last frame dropped when K is even
    z   = encoder.layer_norm(AvgPool1d(s, s)(h)[:T2] + pos[:T2])
    z   = the post-LN layers at T2 frames
    u   = gelu(upsample.projection(z))                       [B, T2, s H] read as [B, s T2, H], zero rows up to T frames
    logits = lm_head(u)
This subclass of Wav2Vec2ForCTC replaces the prefix (`sew.`), the configuration reader, the parameter list, the projection hooks and the
encoder hooks; the layer loop, the weight norm, the extractor, flat parameters and the length-bucket hipGraphs are the parent's.  The
strided conv's product stays a grouped GEMM on the packed input (lda = s * cg, M = T2, the way ops.conv1d expresses a stride); everything
between that product and the first layer is ONE kernel each way (ops.squeeze_ln / ops.squeeze_ln_bwd: bias, GELU, regroup, pool, sum,
LayerNorm; the hook pair _squeeze / _squeeze_bwd, which SEW-D answers without the LayerNorm), everything between the upsampling
projection and lm_head another (ops.unsqueeze_act / _bwd).  `out.frames` and the logits
stay at T frames, the extractor's count: the loops and CTC work there.

Bucketed hipGraph replay.  The encoder's valid length is v2 = vT // s (vT: the utterance's frames), a device scalar filled next to the
parent's (_fill_valid), read by the attention's key mask and the four kernels.  Wav2Vec2ConformerForCTC.forward's zero-gradient argument
carries over: CTC gives the padded output frames zero gradient, every per-frame backward maps a zero row to a zero row, the masked
softmax cuts the attention path.  Three places look across time here:
  * the positional conv: the parent zeroes h past vT before it (what the unpadded run's zero padding holds there), its output rows >= v2
    are never used (next point), and the conv path's input gradient is masked past vT (the windows of the last valid frames reach there);
  * the pool: squeezed row t pools frames s t .. s t + s - 1, all valid when t < v2.  With vT odd inside an even bucket, squeezed row
    vT // 2 averages the last valid frame with a zero row; the unpadded run has no such row.  It reaches nothing: it is >= v2, so the
    forward kernel writes zeros there, the attention masks it as a key, the backward kernel gives it no gradient (exact zeros in dyg and in
    its s rows of dh, without reading dz) and leaves it out of the three column sums;
  * the unsqueeze: output rows >= s v2 are exact zeros, as the unpadded run's zero padding (row vT - 1 for vT odd: its logits are
    lm_head.bias), and du rows >= v2 are exact zeros whatever the incoming gradient holds.
Eval mode only, as the reference loop: no dropout, layerdrop or SpecAugment masking; no attention_mask (the reference passes none)."""
from types import SimpleNamespace

import torch

from . import ops
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(W2.DEFAULT_CONFIG, conv_dim=(64, 128, 128, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512),
                      conv_stride=(5, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1), conv_kernel=(10, 3, 1, 3, 1, 3, 1, 3, 1, 2, 1, 2, 1),
                      squeeze_factor=2, feat_extract_activation="gelu", hidden_act="gelu")


def make_config(cfg=None):
    """wav2vec2_model.make_config with SEW's keys (`squeeze_factor`, `feat_extract_activation`, `hidden_act`) and transformers' SEWConfig
    defaults, the encoder forced to post-LN (SEW has no other).  What is not built is refused by name."""
    src = W2.config_dict(cfg, tuple(DEFAULT_CONFIG) + tuple(W2.LAYOUT_FLAGS))
    out = W2.make_config(dict(src, do_stable_layer_norm=False), DEFAULT_CONFIG)
    for k in ("feat_extract_activation", "hidden_act"):
        if out[k] != "gelu":
            raise ops.DynError(f"{k}={out[k]!r} is not built: only \"gelu\"")
    s = out["squeeze_factor"]
    if not isinstance(s, int) or isinstance(s, bool) or not 1 <= s <= 4:
        raise ops.DynError(f"squeeze_factor={s!r} is not built: 1, 2, 3 or 4")
    if out["hidden_size"] % 256:
        raise ops.DynError(f"hidden_size={out['hidden_size']} is not built: the row kernels need a multiple of 256")
    if out["conv_dim"][-1] % 256:
        raise ops.DynError(f"conv_dim[-1]={out['conv_dim'][-1]} is not built: the row kernels need a multiple of 256")
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def has_projection(c):
    return c["conv_dim"][-1] != c["hidden_size"]


def param_spec(c, pf="sew."):
    """wav2vec2_model.param_spec under SEW's prefix: `feature_projection.layer_norm.*` becomes `layer_norm.*`, `feature_projection.projection.*`
    becomes `feature_projection.*` and exists only when conv_dim[-1] != hidden_size, `encoder.upsample.projection.*` stands before lm_head."""
    H, s = c["hidden_size"], c["squeeze_factor"]
    fp = pf + "feature_projection."
    spec = []
    for name, shape, kind in W2.param_spec(c, pf):
        if name.startswith(fp + "layer_norm."):
            name = pf + name[len(fp):]
        elif name.startswith(fp + "projection."):
            if not has_projection(c):
                continue
            name = fp + name[len(fp + "projection."):]
        elif name == "lm_head.weight":
            spec += [(pf + "encoder.upsample.projection.weight", (s * H, H), None), (pf + "encoder.upsample.projection.bias", (s * H,), None)]
        spec.append((name, shape, kind))
    return spec


class SEWForCTC(W2.Wav2Vec2ForCTC):
    _prefix = "sew."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)

    def __init__(self, config=None, device="cuda:0"):
        c = self._make_config(config)
        H, G = c["hidden_size"], c["num_conv_pos_embedding_groups"]
        if H > 1024 or G < 1 or H % G or (H // G) % 4:
            raise ops.DynError(f"the squeeze kernels need hidden_size up to 1024 and hidden_size / num_conv_pos_embedding_groups a multiple "
                               f"of 4 (got {H} / {G})")
        super().__init__(config, device)
        self._valid2 = torch.zeros(1, dtype=torch.int32, device=self.device)    # valid SQUEEZED frames of the utterance in flight

    def _fill_valid(self, cl):
        super()._fill_valid(cl)
        self._valid2.fill_(cl[-1] // self.cfg["squeeze_factor"])

    # ------------------------------------------------------------------ projection: sew.layer_norm, then the optional linear
    def _project(self, a):
        c, P, pf = self.cfg, self.P, self._prefix
        n, mean, rstd = ops.layernorm(a, P[pf + "layer_norm.weight"], P[pf + "layer_norm.bias"], c["layer_norm_eps"])
        if not has_projection(c):
            return n, (a, mean, rstd, None)
        return ops.linear(n, P[pf + "feature_projection.weight"], P[pf + "feature_projection.bias"]), (a, mean, rstd, n)

    def _project_bwd(self, kept, dhs):
        P, G, pf = self.P, self.G, self._prefix
        a, mean, rstd, n = kept
        dn = dhs if n is None else self._lin_bwd(dhs, n, pf + "feature_projection.weight", pf + "feature_projection.bias")
        da = torch.empty_like(dn)
        ops.layernorm_bwd(a, P[pf + "layer_norm.weight"], mean, rstd, dn, da, G[pf + "layer_norm.weight"], G[pf + "layer_norm.bias"], dx_beta=0.0)
        return da

    # ------------------------------------------------------------------ encoder
    def _conv_dims(self, T):
        c = self.cfg
        H, K, G, s = c["hidden_size"], c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], c["squeeze_factor"]
        return H, K, G, s, H // G, K // 2, T + 2 * (K // 2), T // s

    def _encode(self, h, ctx, vT, dims, v0):
        """Squeeze (strided positional conv + pool + LayerNorm), the parent's post-LN layers at T2 frames, unsqueeze, lm_head at T frames."""
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        B, L, T = dims
        H, K, G, s, cg, pad, Tp, T2 = self._conv_dims(T)
        if T2 < 1:
            raise ops.DynError(f"{T} frames are fewer than squeeze_factor={s}: the squeezed encoder would have no frame")
        v2 = self._valid2 if vT is not None else None
        pc = pf + "encoder.pos_conv_embed.conv."
        w = self._pos_weight()                                      # [H, K, cg]
        xg = ops.group_pack(h, G, pad)                              # [B, G, T + 2 pad, cg]
        yg = torch.empty(B, G, T2, cg, device=h.device, dtype=torch.float32)
        ops.gemm(xg, w, yg, trans_b=True, M=T2, N=cg, K=K * cg, lda=s * cg, ldb=K * cg, ldc=cg, nb1=B, nb2=G,
                 sa=(G * Tp * cg, Tp * cg), sb=(0, cg * K * cg), sc=(G * T2 * cg, T2 * cg))
        z, stats = self._squeeze(h, yg, v2)
        if save:
            ctx["pos"] = (xg, w, yg, h) + stats
        z = self._post_ln_layers(z, ctx, v2)
        u = ops.linear(z, P[pf + "encoder.upsample.projection.weight"], P[pf + "encoder.upsample.projection.bias"])     # [B, T2, s H]
        up = ops.unsqueeze_act(u, T, s, valid=v2)                   # [B, T, H]
        logits = ops.linear(up, P["lm_head.weight"], P["lm_head.bias"])
        if save:
            ctx["up"] = (z, u)
            ctx["head"] = up
            ctx["dims"] = (B, L, T)
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    def _squeeze(self, h, yg, v2):
        """What stands between the strided conv's product yg and the first layer, one kernel: returns (z [B, T2, H], a tuple of what
        _squeeze_bwd needs besides h and yg, batch-major).  A model without the encoder LayerNorm (sew_d_model.py) overrides the pair."""
        c, P, pf = self.cfg, self.P, self._prefix
        z, mean, rstd = ops.squeeze_ln(h, yg, P[pf + "encoder.pos_conv_embed.conv.bias"], P[pf + "encoder.layer_norm.weight"],
                                       P[pf + "encoder.layer_norm.bias"], c["squeeze_factor"], c["layer_norm_eps"], valid=v2)
        return z, (mean, rstd)

    def _squeeze_bwd(self, h, yg, stats, dz, v2):
        """Backward of _squeeze from dz [nb, T2, H] (`h`, `yg`, `stats` cut to the active samples): accumulates its parameters' gradients,
        returns (dh [nb, T, H]: the pool's path, dyg [nb, G, T2, cg]: the conv product's gradient)."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        mean, rstd = stats
        pc = pf + "encoder.pos_conv_embed.conv."
        names = (pf + "encoder.layer_norm.weight", pf + "encoder.layer_norm.bias", pc + "bias")
        return ops.squeeze_ln_bwd(h, yg, P[pc + "bias"], P[names[0]], mean, rstd, dz, c["squeeze_factor"],
                                  *(G[n] if self.trainable(n) else None for n in names), wgrad_beta=1.0, valid=v2)

    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        v0, vT = ctx["valid"]
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        B, L, T = ctx["dims"]
        H, K, Gn, s, cg, pad, Tp, T2 = self._conv_dims(T)
        v2 = self._valid2 if vT is not None else None
        dup = self._lin_bwd(grad_logits.contiguous(), cut(ctx["head"]), "lm_head.weight", "lm_head.bias")
        z, u = cut(ctx["up"])
        du = ops.unsqueeze_act_bwd(u, dup, s, valid=v2)
        dz = self._lin_bwd(du, z, pf + "encoder.upsample.projection.weight", pf + "encoder.upsample.projection.bias")
        dz = self._post_ln_layers_bwd(ctx, dz, nb, T2, cut)
        # squeeze: LayerNorm, pool and GELU backward in one kernel, then the strided conv's three products
        w = ctx["pos"][1]                                            # the normalised weight is not batch-indexed
        xg, _, yg, h, *stats = cut(ctx["pos"])
        dh, dyg = self._squeeze_bwd(h, yg, stats, dz.contiguous(), v2)
        dw = torch.zeros_like(w)
        for b in range(nb):                                          # dw[g] += dyg[b, g]^T rows(xg[b, g]), rows s frames apart
            ops.gemm(dyg, xg, dw, trans_a=True, M=cg, N=K * cg, K=T2, lda=cg, ldb=s * cg, ldc=K * cg, nb1=1, nb2=Gn,
                     sa=(0, T2 * cg), sb=(0, Tp * cg), sc=(0, cg * K * cg), a_off=b * Gn * T2 * cg, b_off=b * Gn * Tp * cg, beta=1.0)
        self._pos_weight_bwd(dw)
        dA = torch.empty(nb, Gn, T2, K * cg, device=dh.device, dtype=torch.float32)
        ops.gemm(dyg, w, dA, M=T2, N=K * cg, K=cg, lda=cg, ldb=K * cg, ldc=K * cg, nb1=nb, nb2=Gn, sa=(Gn * T2 * cg, T2 * cg),
                 sb=(0, cg * K * cg), sc=(Gn * T2 * K * cg, T2 * K * cg))
        dxg = torch.empty(nb * Gn, Tp, cg, device=dh.device, dtype=torch.float32)
        ops.col2im_1d(dA, dxg, nb * Gn, Tp, T2, cg, K, s)
        ops.group_unpack_grad(dxg.view(nb, Gn, Tp, cg), dh, pad, beta=1.0)   # dh = the pool's path + the conv's path
        if vT is not None:
            ops.mask_rows(dh, vT)                                    # the windows of the last valid frames reach into the zeroed tail: no gradient there
        return dh
