"""Wav2Vec2ConformerForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds
for a wav2vec2-conformer checkpoint (facebook/wav2vec2-conformer-rel-pos-large-960h-ft, ...-rope-large-960h-ft), driven by the same
`model(input_values).logits` (lib.py:163,413).  Eval mode, no attention mask, as the reference loop runs it.

Feature extractor, feature projection, flat parameters, length-bucket hipGraphs and the loops are Wav2Vec2ForCTC's, of which this is a subclass
that replaces the prefix (`wav2vec2_conformer.`), the parameter list and the two encoder hooks (_encode / _backward_encoder).  The encoder is
conformer layers only (transformers modeling_wav2vec2_conformer.py, Wav2Vec2ConformerEncoderLayer):
    x = x + 0.5 ffn1(LN(x));  x = x + linear_out(attn(LN(x)));  x = x + conv_module(x);  x = x + 0.5 ffn2(LN(x));  x = final_layer_norm(x)
    conv_module = LN -> pointwise_conv1 (H -> 2H) -> GLU -> depthwise conv (k taps, SAME) -> BatchNorm1d (eval: running statistics)
                  -> act -> pointwise_conv2, no biases
then `encoder.layer_norm` and lm_head.  `act` = hidden_act (gelu | swish) in the FFNs and the conv module.  The per-layer LayerNorms have
torch's default eps; config.layer_norm_eps reaches feature_projection.layer_norm and encoder.layer_norm only.  `encoder.pos_conv_embed.*`
and `masked_spec_embed` exist in transformers but are never used in this forward: they are parameters here too (state-dict interchange),
with gradients that stay exactly zero.  The batch-norm buffers live OUTSIDE the flat parameter vector (`buffers_`): no optimiser step or
weight restore touches them.
Attention, by `position_embeddings_type`:
  "relative"  Transformer-XL scores ((q + u) k^T + shift((q + v) P^T)) / sqrt(D), P = linear_pos(pe), pe = ops.relative_position_table(T, H);
              the shift and the softmax are one kernel (csrc/relshift.hip), the BD products are ops.gemm.
  "rotary"    the LayerNormed states are rotated per head (ops.rotary: x cos + cat(-x2, x1) sin) before linear_q / linear_k, linear_v reads
              them unrotated; plain q k^T / sqrt(D).
Both schemes differ only in how q, k and the score extras are formed: the five products around the softmax (S, O, dV, dP, dQ | dK) are
_attn.py's, as in every model of the family.
The tables are built on the host with transformers' own torch expressions, once per frame count, resident on the device, never inside a
capture (the rule of WavLMForCTC.bucket_table)."""
from types import SimpleNamespace

import torch

from . import _attn, ops
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(W2.DEFAULT_CONFIG, position_embeddings_type="relative", rotary_embedding_base=10000, max_source_positions=5000,
                      conv_depthwise_kernel_size=31, hidden_act="gelu", add_adapter=False)
LAYER_EPS = 1e-5                       # nn.LayerNorm / nn.BatchNorm1d defaults of the per-layer norms
DWCONV_WIDTHS = (3, 5, 7, 9, 15, 31)   # instances of dyn_dwconv1d_*
ACTS = {"gelu": (ops.gelu, ops.gelu_bwd), "swish": (ops.silu, ops.silu_bwd), "silu": (ops.silu, ops.silu_bwd)}
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def make_config(cfg=None):
    """wav2vec2_model.make_config plus the conformer's keys; what this forward does not build is refused by name."""
    out = W2.make_config(cfg, DEFAULT_CONFIG)
    out["do_stable_layer_norm"] = False                      # the conformer encoder has one layout
    if out["position_embeddings_type"] not in ("relative", "rotary"):
        raise ops.DynError(f"position_embeddings_type={out['position_embeddings_type']!r} is not built (\"relative\" or \"rotary\")")
    if out["add_adapter"]:
        raise ops.DynError("add_adapter=True is not built")
    if out["hidden_act"] not in ACTS:
        raise ops.DynError(f"hidden_act={out['hidden_act']!r} is not built ({sorted(ACTS)})")
    k = out["conv_depthwise_kernel_size"] = int(out["conv_depthwise_kernel_size"])
    if k % 2 == 0 or k not in DWCONV_WIDTHS:
        raise ops.DynError(f"conv_depthwise_kernel_size={k} is not built: odd (SAME padding) and one of {DWCONV_WIDTHS}")
    if out["hidden_size"] % out["num_attention_heads"]:
        raise ops.DynError(f"hidden_size={out['hidden_size']} is not a multiple of num_attention_heads={out['num_attention_heads']}")
    if out["position_embeddings_type"] == "rotary" and (out["hidden_size"] // out["num_attention_heads"]) % 2:
        raise ops.DynError("position_embeddings_type=\"rotary\" needs an even head dimension (hidden_size / num_attention_heads)")
    out["max_source_positions"] = int(out["max_source_positions"])
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def param_spec(c, pf="wav2vec2_conformer."):
    """[(name, shape, kind)] in transformers' names: wav2vec2_model.param_spec's front end (extractor, projection, the unused positional conv,
    encoder.layer_norm) + the conformer layers + lm_head.  kind "pw": a pointwise Conv1d kernel kept as [C_out, C_in] (HF [C_out, C_in, 1]),
    "dw": the depthwise kernel kept as [C, k] (HF [C, 1, k]); both are reshapes.  The q | k | v slots are side by side."""
    H, I, k = c["hidden_size"], c["intermediate_size"], c["conv_depthwise_kernel_size"]
    nh = c["num_attention_heads"]
    front = W2.param_spec(dict(c, num_hidden_layers=0), pf)
    spec, head = front[:-2], front[-2:]
    ln = lambda p: [(p + ".weight", (H,), None), (p + ".bias", (H,), None)]                                                       # noqa: E731
    ffn = lambda p: [(p + ".intermediate_dense.weight", (I, H), None), (p + ".intermediate_dense.bias", (I,), None),              # noqa: E731
                     (p + ".output_dense.weight", (H, I), None), (p + ".output_dense.bias", (H,), None)]
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}."
        spec += ln(p + "ffn1_layer_norm") + ffn(p + "ffn1") + ln(p + "self_attn_layer_norm")
        spec += [(p + f"self_attn.linear_{n}.weight", (H, H), None) for n in "qkv"]
        spec += [(p + f"self_attn.linear_{n}.bias", (H,), None) for n in "qkv"]
        spec += [(p + "self_attn.linear_out.weight", (H, H), None), (p + "self_attn.linear_out.bias", (H,), None)]
        if c["position_embeddings_type"] == "relative":
            spec += [(p + "self_attn.linear_pos.weight", (H, H), None), (p + "self_attn.pos_bias_u", (nh, H // nh), None),
                     (p + "self_attn.pos_bias_v", (nh, H // nh), None)]
        cm = p + "conv_module."
        spec += ln(cm + "layer_norm") + [(cm + "pointwise_conv1.weight", (2 * H, H), "pw"), (cm + "depthwise_conv.weight", (H, k), "dw")]
        spec += ln(cm + "batch_norm") + [(cm + "pointwise_conv2.weight", (H, H), "pw")]
        spec += ln(p + "ffn2_layer_norm") + ffn(p + "ffn2") + ln(p + "final_layer_norm")
    return spec + head


class Wav2Vec2ConformerForCTC(W2.Wav2Vec2ForCTC):
    _prefix = "wav2vec2_conformer."
    _qkv_fmt = "self_attn.linear_{}"
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        assert self.packed_qkv                                 # H % 256 == 0: the q | k | v slots are one [3H, H] matrix
        self.relative = c["position_embeddings_type"] == "relative"
        self._layer_eps = LAYER_EPS                            # the per-layer LayerNorms' eps; a model of the family may carry config.layer_norm_eps here
        self._act, self._act_bwd = ACTS[c["hidden_act"]]
        self.buffers_ = self._make_buffers()                   # BatchNorm1d's buffers: not parameters, not in the flat vector
        self._tables = {}                                      # frame count -> pe [2T - 1, H] (relative) | (cos, sin) [T, D / 2] (rotary)

    def _make_buffers(self):
        """{name: tensor} of the conv modules' batch-norm buffers; a model of the family whose conv module has none returns {}."""
        c, pf, out = self.cfg, self._prefix, {}
        H = c["hidden_size"]
        for l in range(c["num_hidden_layers"]):
            p = f"{pf}encoder.layers.{l}.conv_module.batch_norm."
            out[p + "running_mean"] = torch.zeros(H, device=self.device, dtype=torch.float32)
            out[p + "running_var"] = torch.ones(H, device=self.device, dtype=torch.float32)
            out[p + "num_batches_tracked"] = torch.zeros((), device=self.device, dtype=torch.int64)
        return out

    # ------------------------------------------------------------------ state dict
    def _to_hf(self, name, t):
        kind = self._kind[name]
        if kind == "pw":
            return t.unsqueeze(-1)
        if kind == "dw":
            return t.unsqueeze(1)
        return super()._to_hf(name, t)

    def state_dict(self):
        sd = super().state_dict()
        sd.update({n: b.detach().clone() for n, b in self.buffers_.items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        """As the parent's, + the batch-norm buffers; `encoder.embed_positions.inv_freq` (rope) is accepted and recomputed from the config."""
        skip = self._prefix + "encoder.embed_positions.inv_freq"
        res = super().load_state_dict({k: v for k, v in sd.items() if k not in self.buffers_ and k != skip}, strict)
        missing = [n for n in self.buffers_ if n not in sd and not n.endswith("num_batches_tracked")]
        if strict and missing:
            raise KeyError(f"missing {missing[:4]}…")
        for n, b in self.buffers_.items():
            if n in sd:
                if sd[n].numel() != b.numel():
                    raise ops.DynError(f"{n}: shape {tuple(sd[n].shape)} in the state dict does not fit this configuration's {tuple(b.shape)}")
                b.copy_(sd[n].to(b.dtype).reshape(b.shape).to(self.device))
        res.missing_keys = list(res.missing_keys) + missing
        return res

    def copy_buffers_from(self, other):
        for n, b in self.buffers_.items():
            b.copy_(other.buffers_[n])

    # ------------------------------------------------------------------ position tables
    def position_table(self, T):
        """pe [2T - 1, H] (relative) or (cos, sin) [T, D / 2] (rotary) of T frames on the device; built on the host the first time T is seen,
        never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the position table of {T} frames has to exist before its launch sequence is captured")
            c = self.cfg
            if self.relative:
                t = ops.relative_position_table(T, c["hidden_size"]).to(self.device)
            else:
                t = tuple(x.to(self.device) for x in ops.rotary_tables(T, c["hidden_size"] // c["num_attention_heads"],
                                                                       c["rotary_embedding_base"]))
            self._tables[T] = t
        return t

    def forward(self, input_values):
        """As Wav2Vec2ForCTC.forward.  Under bucketed hipGraph replay the position table is the BUCKET's (relative position i - j and the
        rotation of frame t do not depend on the utterance's length) and the utterance's length stays the device scalar of the masked
        softmax.  One op of this encoder looks across time, the depthwise convolution: the GLU output's rows past the utterance are zeroed
        before it (ops.mask_rows: what SAME padding holds there in the unpadded run) and the rows past it of its input gradient after the
        dgrad; every other op is per frame.  The parent's zero-gradient argument then carries over: a padded query row gets
        dL/dlogits = 0 from CTC, hence dS = 0 for its whole row and zero rows of dBD, d(q + u), d(q + v); a padded KEY column has
        probability 0, so dS = 0 there as well and dk, dv, dP sum the unpadded run's terms plus zeros."""
        x = input_values
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] >= self.samples_for_frames(1):
            T, Tb, _ = self._bucket(x.shape[1])
            self.position_table(T)
            if self.use_graphs:
                self.position_table(Tb)
        return super().forward(input_values)

    # ------------------------------------------------------------------ forward
    def _ffn_fwd(self, x, p, which, save):
        """x + 0.5 ffn(LN(x)); returns (result, saved)."""
        P = self.P
        n, m, s = ops.layernorm(x, P[f"{p}{which}_layer_norm.weight"], P[f"{p}{which}_layer_norm.bias"], self._layer_eps)
        u = ops.linear(n, P[f"{p}{which}.intermediate_dense.weight"], P[f"{p}{which}.intermediate_dense.bias"])
        a = self._act(u)
        f = ops.linear(a, P[f"{p}{which}.output_dense.weight"], P[f"{p}{which}.output_dense.bias"])
        r = x.clone() if save else x
        ops.axpby(f, r, 0.5, 1.0)
        return r, (x, m, s, n, u, a)

    def _ffn_bwd(self, dr, kept, p, which):
        """dr = dL/d(x + 0.5 ffn(LN(x))) -> dL/dx (out of place: dr is a queued operand's source)."""
        P, G = self.P, self.G
        x, m, s, n, u, a = kept
        dhalf = dr.clone()
        ops.axpby(dr, dhalf, 0.0, 0.5)                          # 0.5 dr: the FFN branch's output gradient
        da = self._lin_bwd(dhalf, a, f"{p}{which}.output_dense.weight", f"{p}{which}.output_dense.bias")
        du = self._act_bwd(u, da, out=da)
        dn = self._lin_bwd(du, n, f"{p}{which}.intermediate_dense.weight", f"{p}{which}.intermediate_dense.bias")
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[f"{p}{which}_layer_norm.weight"], m, s, dn, dx, G[f"{p}{which}_layer_norm.weight"],
                          G[f"{p}{which}_layer_norm.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    def _attn_fwd(self, x, l, vT, tab, save):
        """x + linear_out(attn(LN(x)))."""
        c, P, pf = self.cfg, self.P, self._prefix
        B, T, H = x.shape
        nh = c["num_attention_heads"]
        D = H // nh
        scale = D ** -0.5
        p = f"{pf}encoder.layers.{l}."
        n, m, s = ops.layernorm(x, P[p + "self_attn_layer_norm.weight"], P[p + "self_attn_layer_norm.bias"], self._layer_eps)
        Wqkv, bqkv = self.Pqkv[l]
        qkv = torch.empty(B, T, 3 * H, device=x.device, dtype=torch.float32)
        S = torch.empty(B, nh, T, T, device=x.device, dtype=torch.float32)
        q, k, v = (_attn.packed(qkv, j, D) for j in range(3))
        if self.relative:
            ops.linear(n, Wqkv, bqkv, out=qkv)
            qu, qv = ops.head_bias_add(qkv, P[p + "self_attn.pos_bias_u"], P[p + "self_attn.pos_bias_v"], H=H, ldq=3 * H)
            pos = ops.linear(tab, P[p + "self_attn.linear_pos.weight"])                  # [2T - 1, H]: head h's P_h is columns h D .. h D + D
            R = 2 * T - 1
            _attn.scores(_attn.plain(qu, D), k, S, scale)
            BD = torch.empty(B, nh, T, R, device=x.device, dtype=torch.float32)          # all 2T - 1 columns: twice the window's flops, accepted
            ops.gemm(qv, pos, BD, trans_b=True, M=T, N=R, K=D, lda=H, ldb=H, ldc=R, nb1=B, nb2=nh, sa=(T * H, D), sb=(0, D),
                     sc=(nh * T * R, T * R), alpha=scale)
            ops.softmax_relshift(S, BD, out=S, valid=vT)
            extra = (qu, qv, pos)
        else:
            cos, sin = tab
            nrot = n.clone()
            ops.rotary(nrot, cos, sin, B, T, nh, D, H)
            ops.gemm(nrot, Wqkv, qkv, trans_b=True, M=B * T, N=2 * H, K=H, lda=H, ldb=H, ldc=3 * H, bias=bqkv)             # q | k from the rotated
            ops.gemm(n, Wqkv, qkv, trans_b=True, M=B * T, N=H, K=H, lda=H, ldb=H, ldc=3 * H, b_off=2 * H * H, c_off=2 * H,   # v from the plain states
                     bias=bqkv[2 * H:])
            _attn.scores(q, k, S, scale)
            ops.softmax(S, out=S, valid=vT)
            extra = (nrot,)
        O = torch.empty(B, T, H, device=x.device, dtype=torch.float32)
        _attn.context(S, v, _attn.plain(O, D))
        r = x.clone() if save else x
        ops.linear(O, P[p + "self_attn.linear_out.weight"], P[p + "self_attn.linear_out.bias"], out=r, beta=1.0)
        return r, (x, m, s, n, qkv, S, O) + extra

    def _attn_bwd(self, dr, kept, pos, l, nb, T, tab, vT=None):
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        sc = D ** -0.5
        p = f"{pf}encoder.layers.{l}."
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
        if self.relative:
            qu, qv = kept[7], kept[8]
            R = 2 * T - 1
            sB, sO = (nh * T * R, T * R), (T * H, D)
            dqu = torch.empty(nb, T, H, device=dr.device, dtype=torch.float32)
            _attn.grad_qk(dP, _attn.plain(qu, D), k, _attn.plain(dqu, D), dk, sc)    # q + u took q's place: dQ is d(q + u), dK reads q + u
            dBD = ops.relshift_bwd(dP)                           # dS in every row's window, zeros written around it
            dqv = torch.empty_like(dqu)
            ops.gemm(dBD, pos, dqv, M=T, N=D, K=R, lda=R, ldb=H, ldc=H, nb1=nb, nb2=nh, sa=sB, sb=(0, D), sc=sO, alpha=sc)
            dpos = torch.empty_like(pos)
            for b in range(nb):                                  # dP_h = sum_b dBD[b, h]^T (q + v)[b, h], b in index order
                ops.gemm(dBD, qv, dpos, trans_a=True, M=R, N=D, K=T, lda=R, ldb=H, ldc=H, nb1=1, nb2=nh, sa=(0, T * R), sb=(0, D), sc=(0, D),
                         a_off=b * nh * T * R, b_off=b * T * H, alpha=sc, beta=0.0 if b == 0 else 1.0)
            self._wgrad(dpos, tab, G[p + "self_attn.linear_pos.weight"], None)
            ops.head_bias_bwd(dqu, dqv, dqkv, G[p + "self_attn.pos_bias_u"], G[p + "self_attn.pos_bias_v"], beta=1.0, ldq=3 * H)
            self._wgrad(dqkv.view(M, 3 * H), n.view(M, H), gW, gb)
            dn = torch.empty_like(dr)
            ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        else:
            cos, sin = tab
            nrot = kept[7]
            _attn.grad_qk(dP, q, k, dq, dk, sc)
            # q | k read the rotated states, v the plain ones: two weight-gradient products into the packed [3H, H] gradient, one bias sum
            ops.gemm(dqkv, nrot, gW, trans_a=True, M=2 * H, N=H, K=M, lda=3 * H, ldb=H, ldc=H, beta=1.0)
            ops.gemm(dqkv, n, gW, trans_a=True, M=H, N=H, K=M, lda=3 * H, ldb=H, ldc=H, a_off=2 * H, c_off=2 * H * H, beta=1.0)
            ops.colsum(dqkv, gb, beta=1.0)
            dn = torch.empty_like(dr)
            ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=2 * H, lda=3 * H, ldb=H, ldc=H)
            ops.rotary(dn, cos, sin, nb, T, nh, D, H, inverse=True)                      # the rotation's transpose
            ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=H, lda=3 * H, ldb=H, ldc=H, a_off=2 * H, b_off=2 * H * H, beta=1.0)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "self_attn_layer_norm.weight"], m, s, dn, dx, G[p + "self_attn_layer_norm.weight"],
                          G[p + "self_attn_layer_norm.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    def _bn(self, l):
        p = f"{self._prefix}encoder.layers.{l}.conv_module.batch_norm."
        return self.buffers_[p + "running_mean"], self.buffers_[p + "running_var"]

    def _conv_fwd(self, x, l, vT, save):
        """x + conv_module(x)."""
        P = self.P
        p = f"{self._prefix}encoder.layers.{l}.conv_module."
        n, m, s = ops.layernorm(x, P[p + "layer_norm.weight"], P[p + "layer_norm.bias"], self._layer_eps)
        g = ops.linear(n, P[p + "pointwise_conv1.weight"])
        gl = ops.glu(g)
        if vT is not None:
            ops.mask_rows(gl, vT)                               # the depthwise conv must see zeros past the utterance's last frame
        dw = ops.dwconv1d(gl, P[p + "depthwise_conv.weight"], None)
        mean, var = self._bn(l)
        bn = ops.chanaffine(dw, mean, var, P[p + "batch_norm.weight"], P[p + "batch_norm.bias"], LAYER_EPS)
        a = self._act(bn)
        r = x.clone() if save else x
        ops.linear(a, P[p + "pointwise_conv2.weight"], None, out=r, beta=1.0)
        return r, (x, m, s, n, g, gl, dw, bn, a)

    def _conv_bwd(self, dr, kept, l, vT):
        P, G = self.P, self.G
        p = f"{self._prefix}encoder.layers.{l}.conv_module."
        x, m, s, n, g, gl, dw, bn, a = kept
        da = self._lin_bwd(dr, a, p + "pointwise_conv2.weight", None)
        dbn = self._act_bwd(bn, da, out=da)
        mean, var = self._bn(l)
        ddw = torch.empty_like(dbn)
        ops.chanaffine_bwd(dw, mean, var, P[p + "batch_norm.weight"], dbn, ddw, G[p + "batch_norm.weight"], G[p + "batch_norm.bias"], LAYER_EPS)
        ops.dwconv1d_wgrad(gl, ddw, G[p + "depthwise_conv.weight"], None, beta=1.0)
        dgl = ops.dwconv1d_dgrad(ddw, P[p + "depthwise_conv.weight"])
        if vT is not None:
            ops.mask_rows(dgl, vT)                              # the windows of the last valid frames reach into the zeroed tail: no gradient there
        dg = ops.glu_bwd(g, dgl)
        dn = self._lin_bwd(dg, n, p + "pointwise_conv1.weight", None)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "layer_norm.weight"], m, s, dn, dx, G[p + "layer_norm.weight"], G[p + "layer_norm.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    # The conv module of the family's causal members (Wav2Vec2-BERT, Nemotron streaming): LayerNorm -> pointwise conv -> [GLU -> causal
    # depthwise conv -> LayerNorm -> activation in one launch] -> pointwise conv, added to x.  A class says what is its own in
    # _causal_conv_spec(l): the parameter names (without .weight / .bias; the three convolutions' biases are used where they exist) of
    # (layer_norm, pointwise_conv1, depthwise_conv, depthwise_layer_norm, pointwise_conv2), then core(u, w, cbias, gamma, beta, save), the
    # activation's backward and the depthwise wgrad and dgrad ops.
    def _causal_conv_fwd(self, x, l, save):
        P = self.P
        (ln, pw1, dw, dln, pw2), core = self._causal_conv_spec(l)[:2]
        n, m, s = ops.layernorm(x, P[ln + ".weight"], P[ln + ".bias"], self._layer_eps)
        u = ops.linear(n, P[pw1 + ".weight"], P.get(pw1 + ".bias"))
        a, g, cv, nn, mean, rstd = core(u, P[dw + ".weight"], P.get(dw + ".bias"), P[dln + ".weight"], P[dln + ".bias"], save)
        r = x.clone() if save else x
        ops.linear(a, P[pw2 + ".weight"], P.get(pw2 + ".bias"), out=r, beta=1.0)
        return r, (x, m, s, n, u, g, cv, nn, mean, rstd, a)

    def _causal_conv_bwd(self, dr, kept, l):
        P, G = self.P, self.G
        (ln, pw1, dw, dln, pw2), _, act_bwd, wgrad, dgrad = self._causal_conv_spec(l)
        x, m, s, n, u, g, cv, nn, mean, rstd, a = kept
        has_cb = dw + ".bias" in P
        b1, b2 = (pw + ".bias" if has_cb else None for pw in (pw1, pw2))
        da = self._lin_bwd(dr, a, pw2 + ".weight", b2)
        dnn = act_bwd(nn, da, out=da)
        dcv = torch.empty_like(dnn)
        ops.layernorm_bwd(cv, P[dln + ".weight"], mean, rstd, dnn, dcv, G[dln + ".weight"], G[dln + ".bias"], dx_beta=0.0)
        wgrad(g, dcv, G[dw + ".weight"], beta=1.0)
        if has_cb:
            ops.colsum(dcv.view(-1, dcv.shape[-1]), G[dw + ".bias"], beta=1.0)
        dg = dgrad(dcv, P[dw + ".weight"])
        du = ops.glu_bwd(u, dg)
        dn = self._lin_bwd(du, n, pw1 + ".weight", b1)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[ln + ".weight"], m, s, dn, dx, G[ln + ".weight"], G[ln + ".bias"], dx_beta=1.0, dx_in=dr)
        return dx

    def _layers_fwd(self, x, ctx, vT, tab):
        """The conformer layers on x [B, T, H]; fills ctx["layers"] when a context is kept.  Shared with a model of the family whose encoder
        ends differently (wav2vec2_bert_model.py)."""
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        if save:
            ctx["layers"] = []
        for l in range(c["num_hidden_layers"]):
            p = f"{pf}encoder.layers.{l}."
            r1, k1 = self._ffn_fwd(x, p, "ffn1", save)
            r2, k2 = self._attn_fwd(r1, l, vT, tab, save)
            pos = k2[9] if self.relative else None              # [2T - 1, H]: not batch-indexed, kept apart from what an n_active backward cuts
            r3, k3 = self._conv_fwd(r2, l, vT, save)
            r4, k4 = self._ffn_fwd(r3, p, "ffn2", save)
            x, m, s = ops.layernorm(r4, P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"], self._layer_eps)
            if save:
                ctx["layers"].append(((k1, k2[:9], k3, k4, (r4, m, s)), pos))
        return x

    def _encode(self, h, ctx, vT, dims, v0):
        c, P, pf = self.cfg, self.P, self._prefix
        save = ctx is not None
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        hN, mean, rstd = ops.layernorm(x, P[pf + "encoder.layer_norm.weight"], P[pf + "encoder.layer_norm.bias"], c["layer_norm_eps"])
        logits = ops.linear(hN, P["lm_head.weight"], P["lm_head.bias"])
        if save:
            ctx["final"] = (x, mean, rstd)
            ctx["head"] = hN
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    # ------------------------------------------------------------------ backward
    def _layers_bwd(self, ctx, dx, nb, T, tab, vT, cut):
        """Backward of _layers_fwd from dx [nb, T, H], the gradient of its output: returns the gradient of its input."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        for l in reversed(range(c["num_hidden_layers"])):
            p = f"{pf}encoder.layers.{l}."
            kept, pos = ctx["layers"][l]
            k1, k2, k3, k4, (r4, m, s) = cut(kept)
            dr4 = torch.empty_like(dx)
            ops.layernorm_bwd(r4, P[p + "final_layer_norm.weight"], m, s, dx, dr4, G[p + "final_layer_norm.weight"],
                              G[p + "final_layer_norm.bias"], dx_beta=0.0)
            dr3 = self._ffn_bwd(dr4, k4, p, "ffn2")
            dr2 = self._conv_bwd(dr3, k3, l, vT)
            dr1 = self._attn_bwd(dr2, k2, pos, l, nb, T, tab, vT)
            dx = self._ffn_bwd(dr1, k1, p, "ffn1")
            ctx["layers"][l] = None
        return dx

    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        v0, vT = ctx["valid"]
        P, G, pf = self.P, self.G, self._prefix
        T = ctx["dims"][2]
        dh = self._lin_bwd(grad_logits.contiguous(), cut(ctx["head"]), "lm_head.weight", "lm_head.bias")
        x, mean, rstd = cut(ctx["final"])
        dx = torch.empty_like(dh)
        ops.layernorm_bwd(x, P[pf + "encoder.layer_norm.weight"], mean, rstd, dh, dx, G[pf + "encoder.layer_norm.weight"],
                          G[pf + "encoder.layer_norm.bias"], dx_beta=0.0)
        return self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
