"""Wav2Vec2BertForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for
a w2v-BERT 2.0 fine-tune (`model_type: "wav2vec2-bert"`), driven by the same `model(input).logits` (lib.py:163,413).  Eval mode, no
attention mask, as the reference loop runs it.

A subclass of Wav2Vec2ConformerForCTC: the FFN halves, the five attention products (_attn.py), the layer loop, flat parameters,
length-bucket hipGraphs and the loops are the parent's.  What differs (transformers modeling_wav2vec2_bert.py):
  * no waveform convolution stack.  The model reads Kaldi-style filter-bank features, `input_features` [B, T, 160] (80 log-mel bins, two
    frames per row, per-bin normalised); `feature_projection.layer_norm` is over those 160 channels (ops.narrow_layernorm).  forward()
    takes them as transformers does, or a waveform [B, L] as the loops of wav2vec2_lib.py pass it (after normalize_waveform), which goes
    through frontend.KaldiFbank on the device first.  The features do not depend on the waveform's gain except through the mel floor
    (float32 epsilon against energies of 16-bit-scaled samples), so the loops' zero-mean / unit-variance step changes nothing that
    matters; no gradient flows into the features (they are data).
  * frame counts: F = 1 + (L - 400) // 160 filter-bank frames, T = F // 2 encoder frames (the rows SeamlessM4TFeatureExtractor marks valid;
    an odd last frame is dropped).  The parent's frame arithmetic holds them as a two-"layer" front end, kernels (400, 2) and strides
    (160, 2): conv_lengths, samples_for_frames and _bucket report [F, T] unchanged, `_valid` carries both counts.  L < 560 is refused.
  * prefix `wav2vec2_bert.`; no positional conv, no `encoder.layer_norm`, no batch-norm buffers; EVERY LayerNorm has config.layer_norm_eps.
  * the conv module is causal and LayerNormed: LN -> pointwise_conv1 -> [GLU -> left-padded depthwise conv (31 taps) -> LayerNorm ->
    act] -> pointwise_conv2, the bracket one launch (ops.convmod_causal); its backward is act', ops.layernorm_bwd, the causal dgrad /
    wgrad entries and ops.glu_bwd.
  * attention is `position_embeddings_type: "relative_key"` (Shaw): scores += q_i . E[clamp(j - i, -left, right) + left] / sqrt(D),
    E = `distance_embedding.weight` [P = left + right + 1, D], one table for all heads.

Relative key on the disentangled kernels.  With Erev[r] = E[P - 1 - r] and t(d) = clamp(d + right, 0, P - 1) for d = i - j,
E[clamp(j - i, -left, right) + left] = Erev[t(i - j)], and t is non-decreasing in d.  So softmax_j(S + c2p[m, i, t(i - j)]) with
c2p = scale q Erev^T [B, nh, T, ldp] is ops.softmax_disentangled with p2ct = None, and ops.disentangled_bwd returns dC2P with the clipped
ends summed in a fixed order; dq += scale dC2P Erev is one batched product, dE is ops.relkey_embed_grad (four launches whatever B * nh).
relkey_table() builds t and the runs [lo, hi] of every r on the host, once per frame count, never inside a capture; the table of a bucket
serves every length inside it (t depends on i - j only).

Bucketed hipGraph replay.  The parent's zero-gradient argument carries over, and the conformer's `mask_rows` pair is NOT needed here: the
convolution is causal, so a valid frame's window holds valid frames (or the zeros left of frame 0) only, whatever the padded rows hold;
its dgrad at a padded row sums gradient rows of later frames, which are padded too and exactly zero (CTC gives them no gradient, every
per-frame backward maps a zero row to a zero row), and at a valid row the padded rows it reaches add zeros, as the end of the unpadded
run does; its wgrad multiplies the padded rows' (finite) GLU values by those zeros.  The per-bin statistics of the front end run over the
valid filter-bank frames (`_valid[0]`), the rows past the valid encoder frames are written as zeros, attention masks the keys past
`_valid[-1]`.  tests/test_wav2vec2_bert_gpu.py compares a bucketed replay with the unpadded eager run.

Not built, refused by name before any launch: `position_embeddings_type` other than "relative_key", `add_adapter`,
`use_intermediate_ffn_before_adapter`, `feature_projection_input_dim` != 160, `hidden_size` not a multiple of 256 or above 1024 (the
causal conv kernel's instances), `conv_depthwise_kernel_size` != 31, a `hidden_act` outside the parent's, left + right + 1 > 256,
`adapter_attn_dim`.  No hub checkpoint is on the machine: transformers' Wav2Vec2BertForCTC on the CPU with the same (random) state dict
is the oracle in the tests."""
from types import SimpleNamespace

import torch

from . import _attn, ops
from . import wav2vec2_conformer_model as WC
from . import wav2vec2_model as W2
from .frontend import HOP, WIN, FBANK_STACK, N_MELS, KaldiFbank
from .sew_d_model import BucketTable

FRONT_KERNEL, FRONT_STRIDE = (WIN, FBANK_STACK), (HOP, FBANK_STACK)     # framing, then two frames per row: the parent's frame arithmetic
FEATURE_DIM = N_MELS * FBANK_STACK                                      # 160
CAUSAL_KERNELS = (31,)                                                  # instances of dyn_convmod_causal_fwd / dyn_dwconv1d_causal_*
CAUSAL_WIDTHS = (256, 512, 768, 1024)
MAX_POSITIONS = 256

DEFAULT_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, vocab_size=32,
                      layer_norm_eps=1e-5, hidden_act="swish", feature_projection_input_dim=FEATURE_DIM,
                      position_embeddings_type="relative_key", left_max_position_embeddings=64, right_max_position_embeddings=8,
                      conv_depthwise_kernel_size=31, add_adapter=False, use_intermediate_ffn_before_adapter=False, adapter_attn_dim=None)


def make_config(cfg=None):
    """transformers' Wav2Vec2BertConfig keys with its defaults (vocab_size: 32, the loops' CharTokenizer); what this forward does not build
    is refused by name."""
    out = W2.make_config(cfg, DEFAULT_CONFIG)
    out["do_stable_layer_norm"] = False
    if out["position_embeddings_type"] != "relative_key":
        raise ops.DynError(f"position_embeddings_type={out['position_embeddings_type']!r} is not built (\"relative_key\")")
    if out["add_adapter"]:
        raise ops.DynError("add_adapter=True is not built")
    if out["use_intermediate_ffn_before_adapter"]:
        raise ops.DynError("use_intermediate_ffn_before_adapter=True is not built")
    if out["feature_projection_input_dim"] != FEATURE_DIM:
        raise ops.DynError(f"feature_projection_input_dim={out['feature_projection_input_dim']} is not built: the front end gives "
                           f"{N_MELS} bins x {FBANK_STACK} frames = {FEATURE_DIM}")
    H = out["hidden_size"]
    if H not in CAUSAL_WIDTHS:
        raise ops.DynError(f"hidden_size={H} is not built: a multiple of 256 up to 1024 {CAUSAL_WIDTHS}")
    k = out["conv_depthwise_kernel_size"] = int(out["conv_depthwise_kernel_size"])
    if k not in CAUSAL_KERNELS:
        raise ops.DynError(f"conv_depthwise_kernel_size={k} is not built: one of {CAUSAL_KERNELS}")
    if out["hidden_act"] not in WC.ACTS:
        raise ops.DynError(f"hidden_act={out['hidden_act']!r} is not built ({sorted(WC.ACTS)})")
    if H % out["num_attention_heads"]:
        raise ops.DynError(f"hidden_size={H} is not a multiple of num_attention_heads={out['num_attention_heads']}")
    left, right = (out[k] for k in ("left_max_position_embeddings", "right_max_position_embeddings"))
    if not all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in (left, right)):
        raise ops.DynError(f"left_max_position_embeddings={left!r} / right_max_position_embeddings={right!r} must be non-negative integers")
    if left + right + 1 > MAX_POSITIONS:
        raise ops.DynError(f"left_max_position_embeddings + right_max_position_embeddings + 1 = {left + right + 1} is not built (<= {MAX_POSITIONS})")
    out["conv_kernel"], out["conv_stride"] = FRONT_KERNEL, FRONT_STRIDE
    out["conv_dim"] = ()                     # no conv stack exists (Wav2Vec2BertForCTC._conv_extractor = False)
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def relkey_table(T, left, right):
    """(table, lo, hi), int32 CPU tensors, for T frames.  table [2T - 1]: t(d) = clamp(d + right, 0, left + right) at position d + T - 1,
    d = i - j (query minus key): the row of the REVERSED embedding Erev[r] = E[P - 1 - r] that transformers' index
    clamp(j - i, -left, right) + left selects in E.  lo / hi [P]: row r serves the run lo[r] <= d <= hi[r] (lo > hi: no pair of T frames
    falls into it).  t is non-decreasing in d; nothing here depends on a valid length."""
    if not isinstance(T, int) or T < 1:
        raise ops.DynError(f"relkey_table: T={T!r} must be a positive integer")
    P = left + right + 1
    d = torch.arange(-(T - 1), T)
    t = torch.clamp(d + right, 0, P - 1)
    r = torch.arange(P)
    lo = torch.searchsorted(t, r, right=False) - (T - 1)          # the first d with t(d) >= r
    hi = torch.searchsorted(t, r, right=True) - (T - 1) - 1       # the last d with t(d) <= r
    return BucketTable(t.to(torch.int32), lo.to(torch.int32), hi.to(torch.int32))


def param_spec(c, pf="wav2vec2_bert."):
    """[(name, shape, kind)] in transformers' names; kinds as wav2vec2_conformer_model.param_spec ("pw" / "dw": reshapes)."""
    H, I, k = c["hidden_size"], c["intermediate_size"], c["conv_depthwise_kernel_size"]
    D = H // c["num_attention_heads"]
    Pn = c["left_max_position_embeddings"] + c["right_max_position_embeddings"] + 1
    ln = lambda p, n=H: [(p + ".weight", (n,), None), (p + ".bias", (n,), None)]                                                  # noqa: E731
    ffn = lambda p: [(p + ".intermediate_dense.weight", (I, H), None), (p + ".intermediate_dense.bias", (I,), None),              # noqa: E731
                     (p + ".output_dense.weight", (H, I), None), (p + ".output_dense.bias", (H,), None)]
    fp = pf + "feature_projection."
    spec = [(pf + "masked_spec_embed", (H,), None)] + ln(fp + "layer_norm", FEATURE_DIM)
    spec += [(fp + "projection.weight", (H, FEATURE_DIM), None), (fp + "projection.bias", (H,), None)]
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}."
        spec += ln(p + "ffn1_layer_norm") + ffn(p + "ffn1") + ln(p + "self_attn_layer_norm")
        spec += [(p + f"self_attn.linear_{n}.weight", (H, H), None) for n in "qkv"]
        spec += [(p + f"self_attn.linear_{n}.bias", (H,), None) for n in "qkv"]
        spec += [(p + "self_attn.linear_out.weight", (H, H), None), (p + "self_attn.linear_out.bias", (H,), None),
                 (p + "self_attn.distance_embedding.weight", (Pn, D), None)]
        cm = p + "conv_module."
        spec += ln(cm + "layer_norm") + [(cm + "pointwise_conv1.weight", (2 * H, H), "pw"), (cm + "depthwise_conv.weight", (H, k), "dw")]
        spec += ln(cm + "depthwise_layer_norm") + [(cm + "pointwise_conv2.weight", (H, H), "pw")]
        spec += ln(p + "ffn2_layer_norm") + ffn(p + "ffn2") + ln(p + "final_layer_norm")
    return spec + [("lm_head.weight", (c["vocab_size"], H), None), ("lm_head.bias", (c["vocab_size"],), None)]


class Wav2Vec2BertForCTC(WC.Wav2Vec2ConformerForCTC):
    _input = "input_features"
    _prefix = "wav2vec2_bert."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    _norm_weight_suffixes = ()
    _conv_extractor = False                                    # filter-bank features, no waveform conv stack

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self._layer_eps = c["layer_norm_eps"]                  # every LayerNorm of this model
        self._act_name = c["hidden_act"]
        self.left, self.right = c["left_max_position_embeddings"], c["right_max_position_embeddings"]
        self.n_pos = self.left + self.right + 1
        self.ldp = (self.n_pos + 3) // 4 * 4                   # the leading dimension of the position product
        self.frontend = KaldiFbank(self.device)

    def _make_buffers(self):
        return {}                                              # no BatchNorm1d here

    # ------------------------------------------------------------------ position tables
    def position_table(self, T):
        """relkey_table(T) on the device; built on the host the first time T is seen, never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the relative-key table of {T} frames has to exist before its launch sequence is captured")
            t = self._tables[T] = BucketTable(*(x.to(self.device) for x in relkey_table(T, self.left, self.right)))
        return t

    # ------------------------------------------------------------------ forward
    def forward(self, input_features):
        """input_features [B, T, 160] float32 on the device (transformers' own signature: eager, every row valid), or a waveform [B, L] (the
        loops): filter-bank front end on the device, then as Wav2Vec2ForCTC.forward, length buckets included.
        -> SimpleNamespace(logits [B, T', V], frames)."""
        x = input_features
        if isinstance(x, torch.Tensor) and x.dim() == 3:
            if not (x.is_cuda and x.dtype == torch.float32 and x.shape[2] == FEATURE_DIM and x.shape[1] >= 1):
                raise ops.DynError(f"input_features must be a float32 CUDA tensor [B, T, {FEATURE_DIM}]")
            B, T, _ = x.shape
            self.position_table(T)
            with ops.use_workspace(self._scratch()):
                self._vl, self._ctx_static = None, False
                return self._from_features(x.contiguous(), None, None, (B, self.samples_for_frames(T), T))
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] >= self.samples_for_frames(1):
            T, Tb, _ = self._bucket(x.shape[1])
            self.position_table(T)
            if self.use_graphs:
                self.position_table(Tb)
        return W2.Wav2Vec2ForCTC.forward(self, x)

    def _forward_eager(self, x):
        vl = self._vl
        v0 = vl[0:1] if vl is not None else None             # valid filter-bank frames (the per-bin statistics run over them)
        vT = vl[-1:] if vl is not None else None             # valid encoder frames
        B, L = x.shape
        need = self.samples_for_frames(1)
        if L < need:
            raise ops.DynError(f"input of {L} samples is shorter than two filter-bank frames ({need} samples): the unbiased per-bin variance "
                               "of the front end is undefined")
        feats = self.frontend(x.contiguous(), valid=v0)       # [B, F // 2, 160], rows past the utterance zeros
        return self._from_features(feats, v0, vT, (B, L, feats.shape[1]))

    def _from_features(self, feats, v0, vT, dims):
        ctx = {"conv": []} if torch.is_grad_enabled() else None
        h, kept = self._project(feats)
        if ctx is not None:
            ctx["proj"] = kept
        return self._encode(h, ctx, vT, dims, v0)

    def _project(self, a):
        c, P = self.cfg, self.P
        fp = self._prefix + "feature_projection."
        n, mean, rstd = ops.narrow_layernorm(a, P[fp + "layer_norm.weight"], P[fp + "layer_norm.bias"], c["layer_norm_eps"])
        return ops.linear(n, P[fp + "projection.weight"], P[fp + "projection.bias"]), (a, mean, rstd, n)

    def _project_bwd(self, kept, dhs):
        """Accumulates the projection's and its LayerNorm's gradients; the features are data, so nothing is returned."""
        a, mean, rstd, n = kept
        fp = self._prefix + "feature_projection."
        need_dn = self.trainable(fp + "layer_norm.weight") or self.trainable(fp + "layer_norm.bias")
        dn = self._lin_bwd(dhs, n, fp + "projection.weight", fp + "projection.bias", need_dx=need_dn)
        if need_dn:
            ops.narrow_layernorm_bwd(a, self.P[fp + "layer_norm.weight"], mean, rstd, dn, self._g(fp + "layer_norm.weight"),
                                     self._g(fp + "layer_norm.bias"))

    def _attn_fwd(self, x, l, vT, tab, save):
        """x + linear_out(attn(LN(x))) with the relative-key term gathered inside the softmax."""
        c, P, pf = self.cfg, self.P, self._prefix
        B, T, H = x.shape
        nh = c["num_attention_heads"]
        D = H // nh
        scale = D ** -0.5
        Pn, ldp = self.n_pos, self.ldp
        p = f"{pf}encoder.layers.{l}."
        n, m, s = ops.layernorm(x, P[p + "self_attn_layer_norm.weight"], P[p + "self_attn_layer_norm.bias"], self._layer_eps)
        Wqkv, bqkv = self.Pqkv[l]
        qkv = torch.empty(B, T, 3 * H, device=x.device, dtype=torch.float32)
        ops.linear(n, Wqkv, bqkv, out=qkv)
        q, k, v = (_attn.packed(qkv, j, D) for j in range(3))
        S = torch.empty(B, nh, T, T, device=x.device, dtype=torch.float32)
        _attn.scores(q, k, S, scale)
        erev = P[p + "self_attn.distance_embedding.weight"].flip(0)                     # [P, D], a copy: row r = E[P - 1 - r]
        c2p = torch.empty(B, nh, T, ldp, device=x.device, dtype=torch.float32)          # columns >= P are never read
        ops.gemm(q.t, erev, c2p, trans_b=True, M=T, N=Pn, K=D, lda=q.ld, ldb=D, ldc=ldp, nb1=B, nb2=nh, sa=(q.sb, D), sb=(0, 0),
                 sc=(nh * T * ldp, T * ldp), a_off=q.off, alpha=scale)
        ops.softmax_disentangled(S, c2p, None, tab.table, Pn, ldp, out=S, valid=vT)
        O = torch.empty(B, T, H, device=x.device, dtype=torch.float32)
        _attn.context(S, v, _attn.plain(O, D))
        r = x.clone() if save else x
        ops.linear(O, P[p + "self_attn.linear_out.weight"], P[p + "self_attn.linear_out.bias"], out=r, beta=1.0)
        return r, (x, m, s, n, qkv, S, O)

    def _attn_bwd(self, dr, kept, pos, l, nb, T, tab, vT=None):
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        H, nh = c["hidden_size"], c["num_attention_heads"]
        D = H // nh
        sc = D ** -0.5
        Pn, ldp = self.n_pos, self.ldp
        p = f"{pf}encoder.layers.{l}."
        x, m, s, n, qkv, S, O = kept
        Wqkv = self.Pqkv[l][0]
        gW, gb = self.Gqkv[l]
        M = nb * T
        dO = self._lin_bwd(dr, O, p + "self_attn.linear_out.weight", p + "self_attn.linear_out.bias")
        dqkv = torch.empty_like(qkv)
        (q, k, v), (dq, dk, dv) = ([_attn.packed(t, j, D) for j in range(3)] for t in (qkv, dqkv))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)                # dP is now dS, the gradient of the summed pre-softmax score
        _attn.grad_qk(dP, q, k, dq, dk, sc)
        dc, _ = ops.disentangled_bwd(dP, tab.table, tab.lo, tab.hi, ldp, want_c2p=True, want_p2c=False, valid=vT)
        E = p + "self_attn.distance_embedding.weight"
        ops.gemm(dc, P[E].flip(0), dq.t, M=T, N=D, K=Pn, lda=ldp, ldb=D, ldc=dq.ld, nb1=nb, nb2=nh, sa=(nh * T * ldp, T * ldp), sb=(0, 0),
                 sc=(dq.sb, D), c_off=dq.off, alpha=sc, beta=1.0)
        if self.trainable(E):
            ops.relkey_embed_grad(dc, q, G[E], sc, beta=1.0)
        self._wgrad(dqkv.view(M, 3 * H), n.view(M, H), gW, gb)
        dn = torch.empty_like(dr)
        ops.gemm(dqkv, Wqkv, dn, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        dx = torch.empty_like(dr)
        ops.layernorm_bwd(x, P[p + "self_attn_layer_norm.weight"], m, s, dn, dx, G[p + "self_attn_layer_norm.weight"],
                          G[p + "self_attn_layer_norm.bias"], dx_beta=1.0, dx_in=dr)
        return dx

    def _causal_conv_spec(self, l):
        p = f"{self._prefix}encoder.layers.{l}.conv_module."
        names = tuple(p + n for n in ("layer_norm", "pointwise_conv1", "depthwise_conv", "depthwise_layer_norm", "pointwise_conv2"))
        core = lambda u, w, cb, gamma, beta, save: ops.convmod_causal(u, w, gamma, beta, self._act_name, self._layer_eps, save=save)
        return names, core, self._act_bwd, ops.dwconv1d_causal_wgrad, ops.dwconv1d_causal_dgrad

    def _conv_fwd(self, x, l, vT, save):
        """x + conv_module(x).  No row masking under a length bucket: the convolution is causal (see the module docstring)."""
        return self._causal_conv_fwd(x, l, save)

    def _conv_bwd(self, dr, kept, l, vT):
        return self._causal_conv_bwd(dr, kept, l)

    def _encode(self, h, ctx, vT, dims, v0):
        P = self.P
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        logits = ops.linear(x, P["lm_head.weight"], P["lm_head.bias"])
        if ctx is not None:
            ctx["head"] = x
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(logits=logits, frames=T)

    # ------------------------------------------------------------------ backward
    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        """lm_head, the layers and the feature projection; returns None: nothing lies below the projection (the features are data)."""
        v0, vT = ctx["valid"]
        T = ctx["dims"][2]
        dx = self._lin_bwd(grad_logits.contiguous(), cut(ctx["head"]), "lm_head.weight", "lm_head.bias")
        dh = self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
        if not self._below_frozen():
            self._project_bwd(cut(ctx["proj"]), dh)
        return None
