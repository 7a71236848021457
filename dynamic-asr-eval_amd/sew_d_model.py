"""SEWDForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for a SEW-D
checkpoint (asapp/sew-d-*-ft-ls100h, `model_type: "sew-d"`), driven by the same `model(input_values).logits` (lib.py:163,413).

SEW-D (transformers SEWDForCTC) is SEW (sew_model.py: extractor, `sew_d.layer_norm`, the optional projection, the squeezed encoder at
T2 = T // s frames, the upsampling, lm_head) with three differences:
  * no LayerNorm after the squeeze: the layers' input is AvgPool1d(s, s)(h)[:T2] + gelu(conv_s(h))[:T2] (ops.squeeze / ops.squeeze_bwd, the
    squeeze kernels with the LayerNorm compiled out);
  * the layers carry BERT's parameter names (`sew_d.encoder.encoder.layer.{l}.attention.self.query_proj`, `.attention.output.dense`, ...);
    the arithmetic is the parent's post-LN layer, so Wav2Vec2ForCTC._post_ln_layers / _post_ln_layers_bwd run unchanged: self.P / self.G
    carry the parent's name of every layer parameter as a second key for the same view (LAYER_NAMES);
  * the attention is DeBERTa-v2's disentangled attention with `share_att_key` (csrc/disentangled.hip).  With rel = the relative embeddings
    `rel_embeddings.weight` [2 span, H] (through `encoder.encoder.LayerNorm` once per forward when `norm_rel_ebd` has `layer_norm`),
    Pq | Pk = the layer's own query | key projection of rel (one product, the first 2H rows of the packed q | k | v weight) and
    f = 1 + [c2p] + [p2c]:
        score[i, j] = (q_i . k_j + q_i . Pk[t(i - j)] + k_j . Pq[t(i - j)]) / sqrt(D f),    t(d) = clamp(bucket(d) + span, 0, 2 span - 1)
    The three products are strided batched GEMMs (Pq, Pk with batch stride 0), the gather of both terms and the masked softmax one kernel,
    the gathers' backward one entry of segment sums (ops.softmax_disentangled / ops.disentangled_bwd).  t comes from bucket_table() below:
    the project's restatement of transformers' build_relative_position / make_log_bucket_position on the host, in the same dtypes and
    operation order (the ceil(log(..)) sits on integer boundaries), one int32 table per row length, uploaded once.

Index identity.  The position matrix depends on d = i - j only, bucket(d) is odd and monotone non-decreasing, so transformers' p2c index
clamp(-bucket(j - i) + span) IS the c2p index t(i - j), the clamp included, and every bucket is one contiguous run of d (bucket_table
refuses a table that is not monotone; tests/test_sew_d_cpu.py checks the identity against transformers' two index matrices).  One table serves both terms; the backward's scatter-add is a segment sum in a fixed order.

Bucketed hipGraph replay.  The encoder's valid length is SEW's `_valid2`; SEW's zero-gradient argument carries over (sew_model.py), with
one more place that looks across time: the position terms.  t depends on i - j only, so the table built for the bucket's length holds, for
every valid (i, j), exactly the entry the unpadded run's table holds; keys >= v2 are masked, padded queries receive zero gradient from CTC
and the backward entry neither reads them nor gives them any.  Pq, Pk, rel and the table are not batch-indexed: an `n_active` backward
cuts the per-sample tensors only.

Not built, refused by name before any launch: `relative_attention: false`, `share_att_key: false`, a `pos_att_type` that is empty or holds
anything but c2p / p2c, `hidden_size` not a multiple of 256 (the 384-wide tiny checkpoint, as SEW's) and SEW's own refusals.
Eval mode only, as the reference loop: no dropout, layerdrop or SpecAugment masking; no attention_mask (the reference passes none).  No
hub checkpoint is on the machine: transformers' SEWDForCTC on the CPU with the same (random) state dict is the oracle in the tests."""
from collections import namedtuple

import torch

from . import _attn, ops
from . import sew_model as S
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(S.DEFAULT_CONFIG, hidden_act="gelu_python", layer_norm_eps=1e-7, feature_layer_norm_eps=1e-5,
                      max_position_embeddings=512, position_buckets=256, max_relative_positions=-1, relative_attention=True,
                      share_att_key=True, pos_att_type=("p2c", "c2p"), norm_rel_ebd="layer_norm")
OWN_KEYS = ("feature_layer_norm_eps", "max_position_embeddings", "position_buckets", "max_relative_positions", "relative_attention",
            "share_att_key", "pos_att_type", "norm_rel_ebd")

# the parent's name of a layer parameter (wav2vec2_model.param_spec) -> SEW-D's, both without `{prefix}encoder.` in front
LAYER_NAMES = (("attention.q_proj", "attention.self.query_proj"), ("attention.k_proj", "attention.self.key_proj"),
               ("attention.v_proj", "attention.self.value_proj"), ("attention.out_proj", "attention.output.dense"),
               ("layer_norm", "attention.output.LayerNorm"), ("feed_forward.intermediate_dense", "intermediate.dense"),
               ("feed_forward.output_dense", "output.dense"), ("final_layer_norm", "output.LayerNorm"))

BucketTable = namedtuple("BucketTable", "table lo hi")


def att_span(position_buckets, max_position):
    """`pos_ebd_size` of DisentangledSelfAttention: half the rows of the relative embeddings."""
    return position_buckets if position_buckets > 0 else max_position


def _log_bucket(rel, bucket_size, max_position):
    """transformers' make_log_bucket_position, statement by statement, on an int64 tensor (float32 in between, as there)."""
    sign = torch.sign(rel)
    mid = bucket_size // 2
    abs_pos = torch.where((rel < mid) & (rel > -mid), torch.tensor(mid - 1).type_as(rel), torch.abs(rel))
    log_pos = torch.ceil(torch.log(abs_pos / mid) / torch.log(torch.tensor((max_position - 1) / mid)) * (mid - 1)) + mid
    return torch.where(abs_pos <= mid, rel.type_as(log_pos), log_pos * sign)


def bucket_table(T, position_buckets, max_position):
    """(table, lo, hi), int32 CPU tensors.  table [2T - 1]: t(d) = clamp(bucket(d) + span, 0, 2 span - 1) at position d + T - 1, where
    bucket is build_relative_position(T, T, position_buckets, max_position) as a function of d = i - j (log buckets when both are positive,
    else d itself) and span = position_buckets when positive, else max_position.  lo / hi [2 span]: bucket r is the run lo[r] <= d <= hi[r]
    of relative positions (lo > hi: no d in [-(T - 1), T - 1] falls into it).  Nothing here depends on a valid length: the table of a
    padded length serves every length inside it.  A table that is not monotone in d (no configuration gives one) is refused."""
    if not isinstance(T, int) or T < 1:
        raise ops.DynError(f"bucket_table: T={T!r} must be a positive integer")
    span = att_span(position_buckets, max_position)
    if span < 1:
        raise ops.DynError(f"bucket_table: position_buckets={position_buckets} and max_position={max_position} leave no relative position")
    d = torch.arange(-(T - 1), T)
    rel = _log_bucket(d, position_buckets, max_position) if position_buckets > 0 and max_position > 0 else d
    t = torch.clamp(rel.to(torch.long) + span, 0, 2 * span - 1)
    if (t[1:] < t[:-1]).any():
        raise ops.DynError(f"bucket_table: the buckets of T={T}, position_buckets={position_buckets}, max_position={max_position} are not "
                           "monotone in the relative position")
    r = torch.arange(2 * span)
    lo = torch.searchsorted(t, r, right=False) - (T - 1)          # the first d with t(d) >= r
    hi = torch.searchsorted(t, r, right=True) - (T - 1) - 1       # the last d with t(d) <= r
    return BucketTable(t.to(torch.int32), lo.to(torch.int32), hi.to(torch.int32))


def rel_norm(c):
    return "layer_norm" in [x.strip() for x in str(c["norm_rel_ebd"]).lower().split("|")]


def make_config(cfg=None):
    """sew_model.make_config (SEW's keys, defaults and refusals) with SEW-D's own keys and transformers' SEWDConfig defaults.  `hidden_act`
    may be "gelu" or "gelu_python": both are the erf GELU."""
    keys = tuple(DEFAULT_CONFIG) + tuple(W2.LAYOUT_FLAGS)
    src = W2.config_dict(cfg, keys)
    act = src.get("hidden_act", DEFAULT_CONFIG["hidden_act"])
    if act not in ("gelu", "gelu_python"):
        raise ops.DynError(f"hidden_act={act!r} is not built: only \"gelu\" and \"gelu_python\" (the erf GELU)")
    out = S.make_config(dict(src, hidden_act="gelu", layer_norm_eps=src.get("layer_norm_eps", DEFAULT_CONFIG["layer_norm_eps"])))
    out["hidden_act"] = act
    for k in OWN_KEYS:
        v = src.get(k, DEFAULT_CONFIG[k])
        out[k] = tuple(v) if isinstance(v, (list, tuple)) else v
    if not out["relative_attention"]:
        raise ops.DynError("relative_attention=False is not built: SEW-D's layers here are the disentangled attention")
    if not out["share_att_key"]:
        raise ops.DynError("share_att_key=False is not built: the position projections are the layer's own query / key projections")
    pat = out["pos_att_type"]
    pat = tuple(x.strip() for x in pat.split("|")) if isinstance(pat, str) else tuple(pat)
    if not pat or any(x not in ("c2p", "p2c") for x in pat):
        raise ops.DynError(f"pos_att_type={out['pos_att_type']!r} is not built: \"c2p\", \"p2c\" or both")
    out["pos_att_type"] = pat
    for k in ("max_position_embeddings", "position_buckets", "max_relative_positions"):
        if not isinstance(out[k], int) or isinstance(out[k], bool):
            raise ops.DynError(f"{k}={out[k]!r} must be an integer")
    if out["max_relative_positions"] < 1:
        out["max_relative_positions"] = out["max_position_embeddings"]
    if att_span(out["position_buckets"], out["max_relative_positions"]) < 1:
        raise ops.DynError(f"max_position_embeddings={out['max_position_embeddings']} with position_buckets={out['position_buckets']} leaves "
                           "no relative position")
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def param_spec(c, pf="sew_d."):
    """sew_model.param_spec under SEW-D's prefix and names: no `encoder.layer_norm`, the layers as `encoder.encoder.layer.{l}.` with BERT's
    names (LAYER_NAMES; q | k | v still side by side, weights then biases, so the packed projection holds), and behind them
    `encoder.encoder.rel_embeddings.weight` [2 span, H] and, with `norm_rel_ebd: layer_norm`, `encoder.encoder.LayerNorm.*`."""
    H = c["hidden_size"]
    old, new = pf + "encoder.layers.", pf + "encoder.encoder.layer."
    spec = []
    for name, shape, kind in S.param_spec(c, pf):
        if name.startswith(pf + "encoder.layer_norm."):
            continue
        if name == pf + "encoder.upsample.projection.weight":
            spec.append((pf + "encoder.encoder.rel_embeddings.weight", (2 * att_span(c["position_buckets"], c["max_relative_positions"]), H), None))
            if rel_norm(c):
                spec += [(pf + "encoder.encoder.LayerNorm.weight", (H,), None), (pf + "encoder.encoder.LayerNorm.bias", (H,), None)]
        if name.startswith(old):
            l, rest = name[len(old):].split(".", 1)
            stem, leaf = rest.rsplit(".", 1)
            name = f"{new}{l}.{dict(LAYER_NAMES)[stem]}.{leaf}"
        spec.append((name, shape, kind))
    return spec


class SEWDForCTC(S.SEWForCTC):
    _prefix = "sew_d."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    _norm_weight_suffixes = ("LayerNorm.weight",)              # run_wav2vec2.init_synthetic: BERT's spelling of a norm's weight starts at 1 too

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c, pf = self.cfg, self._prefix
        for l in range(c["num_hidden_layers"]):                # the parent's layer loop finds every parameter under the name it uses
            for theirs, ours in LAYER_NAMES:
                for leaf in ("weight", "bias"):
                    a, b = f"{pf}encoder.layers.{l}.{theirs}.{leaf}", f"{pf}encoder.encoder.layer.{l}.{ours}.{leaf}"
                    self.P[a], self.G[a] = self.P[b], self.G[b]
        self.span = att_span(c["position_buckets"], c["max_relative_positions"])
        self.ldp = (2 * self.span + 3) // 4 * 4                # the leading dimension of the position products
        self.c2p, self.p2c = "c2p" in c["pos_att_type"], "p2c" in c["pos_att_type"]
        self.att_scale = float((c["hidden_size"] // c["num_attention_heads"]) * (1 + self.c2p + self.p2c)) ** -0.5
        H, L = c["hidden_size"], c["num_hidden_layers"]
        ow = [self._slots[self._qv_names(l)[0] + ".weight"][0] for l in range(L)]
        self._qkv_stride = ow[1] - ow[0] if L > 1 else 0       # the layers' slots repeat at a constant distance in the flat buffers
        assert all(ow[l] - ow[0] == l * self._qkv_stride for l in range(L))
        self._tables = {}                                      # row length -> BucketTable on the device
        self._rel = None                                       # the forward / backward in flight: see _rel_forward

    def _qv_names(self, l):
        p = f"{self._prefix}encoder.encoder.layer.{l}.attention.self."
        return p + "query_proj", p + "value_proj"

    def _table(self, T):
        """The bucket table of T squeezed frames on the device; built on the host the first time T is seen, never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the bucket table of {T} frames has to exist before its launch sequence is captured")
            c = self.cfg
            t = self._tables[T] = BucketTable(*(x.to(self.device) for x in bucket_table(T, c["position_buckets"], c["max_relative_positions"])))
        return t

    def forward(self, input_values):
        """As SEWForCTC.forward.  The tables of the utterance's own squeezed length and, under bucketed replay, of the bucket's are uploaded
        here, before any capture begins (WavLMForCTC.forward does the same for its table)."""
        x = input_values
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] >= self.samples_for_frames(1):
            s = self.cfg["squeeze_factor"]
            T, Tb, _ = self._bucket(x.shape[1])
            for t in (T, Tb) if self.use_graphs else (T,):
                if t // s >= 1:
                    self._table(t // s)
        return super().forward(input_values)

    # ------------------------------------------------------------------ projection: SEW's, `sew_d.layer_norm` with its own epsilon
    def _project(self, a):
        c, P, pf = self.cfg, self.P, self._prefix
        n, mean, rstd = ops.layernorm(a, P[pf + "layer_norm.weight"], P[pf + "layer_norm.bias"], c["feature_layer_norm_eps"])
        if not S.has_projection(c):
            return n, (a, mean, rstd, None)
        return ops.linear(n, P[pf + "feature_projection.weight"], P[pf + "feature_projection.bias"]), (a, mean, rstd, n)

    # ------------------------------------------------------------------ squeeze: no LayerNorm behind it
    def _squeeze(self, h, yg, v2):
        return ops.squeeze(h, yg, self.P[self._prefix + "encoder.pos_conv_embed.conv.bias"], self.cfg["squeeze_factor"], valid=v2), ()

    def _squeeze_bwd(self, h, yg, stats, dz, v2):
        n = self._prefix + "encoder.pos_conv_embed.conv.bias"
        return ops.squeeze_bwd(yg, self.P[n], dz, h.shape[1], self.cfg["squeeze_factor"], self.G[n] if self.trainable(n) else None,
                               wgrad_beta=1.0, valid=v2)

    # ------------------------------------------------------------------ layers: the parent's, around the relative embeddings
    def _rel_forward(self, T2):
        """The relative embeddings as every layer of this forward reads them, [2 span, H], with the row length's table.  `pqk` collects the
        layers' Pq | Pk [2 span, 2H] for the backward.  None of it is batch-indexed, so it travels in ctx["rel"], not with the layers' tuples."""
        c, P, pf = self.cfg, self.P, self._prefix
        raw = P[pf + "encoder.encoder.rel_embeddings.weight"]
        if not rel_norm(c):
            return dict(table=self._table(T2), rel=raw, stats=None, pqk=[])
        rel, mean, rstd = ops.layernorm(raw, P[pf + "encoder.encoder.LayerNorm.weight"], P[pf + "encoder.encoder.LayerNorm.bias"], c["layer_norm_eps"])
        return dict(table=self._table(T2), rel=rel, stats=(mean, rstd), pqk=[])

    def _post_ln_layers(self, h, ctx, vT):
        self._rel = self._rel_forward(h.shape[1])
        out = super()._post_ln_layers(h, ctx, vT)
        if ctx is not None:
            ctx["rel"] = self._rel
        self._rel = None
        return out

    def _position_operands(self, qkv, pqk):
        """(q, k, Pq, Pk) as _attn views; Pq | Pk [R, 2H] has head h of Pq at column h D, of Pk at column H + h D, and no batch stride."""
        D = self.cfg["hidden_size"] // self.cfg["num_attention_heads"]
        H2 = pqk.shape[-1]
        return (_attn.packed(qkv, 0, D), _attn.packed(qkv, 1, D), _attn.View(pqk, 0, H2, 0, D), _attn.View(pqk, H2 // 2, H2, 0, D))

    def _attention(self, h, l, vT):
        """The parent's _attention with the disentangled score: returns (qkv, S, O).  The two position products are scratch; the backward
        needs the probabilities, qkv and Pq | Pk only."""
        c, rel = self.cfg, self._rel
        B, T, H = h.shape
        nh, R, ldp, a = c["num_attention_heads"], 2 * self.span, self.ldp, self.att_scale
        D = H // nh
        W, bias = self.Pqkv[l]
        qkv = torch.empty(B, T, 3 * H, device=h.device, dtype=torch.float32)
        ops.linear(h, W, bias, out=qkv)
        pqk = ops.linear(rel["rel"], W[:2 * H], bias[:2 * H])            # [R, 2H]: the layer's query | key projection of the embeddings
        rel["pqk"].append(pqk)
        q, k, Pq, Pk = self._position_operands(qkv, pqk)
        S_ = torch.empty(B, nh, T, T, device=h.device, dtype=torch.float32)
        _attn.scores(q, k, S_, a)
        c2p = p2ct = None
        if self.c2p:                                                     # q Pk^T [B, nh, T, ldp]
            c2p = torch.empty(B, nh, T, ldp, device=h.device, dtype=torch.float32)
            ops.gemm(q.t, Pk.t, c2p, trans_b=True, M=T, N=R, K=D, lda=q.ld, ldb=Pk.ld, ldc=ldp, nb1=B, nb2=nh, sa=(q.sb, D), sb=(0, D),
                     sc=(nh * T * ldp, T * ldp), a_off=q.off, b_off=Pk.off, alpha=a)
        if self.p2c:                                                     # Pq k^T [B, nh, ldp, T]: rows >= R are never read
            p2ct = torch.empty(B, nh, ldp, T, device=h.device, dtype=torch.float32)
            ops.gemm(Pq.t, k.t, p2ct, trans_b=True, M=R, N=T, K=D, lda=Pq.ld, ldb=k.ld, ldc=T, nb1=B, nb2=nh, sa=(0, D), sb=(k.sb, D),
                     sc=(nh * ldp * T, ldp * T), a_off=Pq.off, b_off=k.off, alpha=a)
        ops.softmax_disentangled(S_, c2p, p2ct, rel["table"].table, R, ldp, out=S_, valid=vT)
        O = torch.empty(B, T, H, device=h.device, dtype=torch.float32)
        _attn.context(S_, _attn.packed(qkv, 2, D), _attn.plain(O, D))
        return qkv, S_, O

    def _post_ln_layers_bwd(self, ctx, dh, nb, T, cut):
        """The parent's loop, then what all layers owe the relative embeddings.  Every layer leaves dPq | dPk in `dpqk` [layers, R, 2H].  Its
        weight gradient lands in the slot the layer's own QUEUED q | k | v product accumulates into, and the descriptors of a grouped launch
        run side by side, so it does not join that queue: all layers go as ONE strided batched product here, in stream order before the
        flush.  d rel sums the layers in layer order."""
        c, P, G, pf = self.cfg, self.P, self.G, self._prefix
        H, L, R = c["hidden_size"], c["num_hidden_layers"], 2 * self.span
        rel = ctx["rel"]
        self._rel = dict(rel, valid=self._valid2 if ctx["valid"][1] is not None else None,
                         dpqk=torch.zeros(L, R, 2 * H, device=self.device, dtype=torch.float32))
        try:
            dh = super()._post_ln_layers_bwd(ctx, dh, nb, T, cut)
            dpqk = self._rel["dpqk"]
        finally:
            self._rel = None
        ops.gemm(dpqk, rel["rel"], self.Gqkv[0][0], trans_a=True, M=2 * H, N=H, K=R, lda=2 * H, ldb=H, ldc=H, nb1=L, sa=(R * 2 * H, 0),
                 sc=(self._qkv_stride, 0), beta=1.0)
        drel = torch.empty_like(rel["rel"])
        for l in range(L):
            ops.colsum(dpqk[l], self.Gqkv[l][1][:2 * H], beta=1.0)
            ops.gemm(dpqk[l], self.Pqkv[l][0], drel, M=R, N=H, K=2 * H, lda=2 * H, ldb=H, ldc=H, beta=0.0 if l == 0 else 1.0)
        raw = pf + "encoder.encoder.rel_embeddings.weight"
        if rel["stats"] is None:
            ops.axpby(drel, G[raw], 1.0, 1.0)
        else:
            ln = pf + "encoder.encoder.LayerNorm."
            ops.layernorm_bwd(P[raw], P[ln + "weight"], *rel["stats"], drel, G[raw], G[ln + "weight"], G[ln + "bias"], dx_beta=1.0)
        return dh

    def _attention_bwd(self, dO, qkv, S_, h, l, nb, T, residual):
        """The parent's _attention_bwd (packed projections) with the position terms: dQ += a dC2P Pk, dK += a dP2C Pq,
        dPk[head] = a sum_b dC2P^T Q, dPq[head] = a sum_b dP2C^T K (beta = 1, in batch order)."""
        c, rel = self.cfg, self._rel
        H, nh, R, ldp, a = c["hidden_size"], c["num_attention_heads"], 2 * self.span, self.ldp, self.att_scale
        D = H // nh
        pqk, dpqk = rel["pqk"][l], rel["dpqk"][l]
        dqkv = torch.empty_like(qkv)
        q, k, Pq, Pk = self._position_operands(qkv, pqk)
        v, (dq, dk, dv) = _attn.packed(qkv, 2, D), (_attn.packed(dqkv, j, D) for j in range(3))
        dPq, dPk = _attn.View(dpqk, 0, 2 * H, 0, D), _attn.View(dpqk, H, 2 * H, 0, D)
        dP = torch.empty_like(S_)
        _attn.grad_v_dP(S_, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S_, dP, out=dP, scale=1.0)               # dP is now dS, the gradient of the summed pre-softmax score
        _attn.grad_qk(dP, q, k, dq, dk, a)
        tb = rel["table"]
        dc, dpt = ops.disentangled_bwd(dP, tb.table, tb.lo, tb.hi, ldp, want_c2p=self.c2p, want_p2c=self.p2c, valid=rel["valid"])
        if dc is not None:
            ops.gemm(dc, Pk.t, dq.t, M=T, N=D, K=R, lda=ldp, ldb=Pk.ld, ldc=dq.ld, nb1=nb, nb2=nh, sa=(nh * T * ldp, T * ldp), sb=(0, D),
                     sc=(dq.sb, D), b_off=Pk.off, c_off=dq.off, alpha=a, beta=1.0)
            for b in range(nb):
                ops.gemm(dc, q.t, dPk.t, trans_a=True, M=R, N=D, K=T, lda=ldp, ldb=q.ld, ldc=dPk.ld, nb1=1, nb2=nh, sa=(0, T * ldp),
                         sb=(0, D), sc=(0, D), a_off=b * nh * T * ldp, b_off=q.off + b * q.sb, c_off=dPk.off, alpha=a, beta=1.0)
        if dpt is not None:
            ops.gemm(dpt, Pq.t, dk.t, trans_a=True, M=T, N=D, K=R, lda=T, ldb=Pq.ld, ldc=dk.ld, nb1=nb, nb2=nh, sa=(nh * ldp * T, ldp * T),
                     sb=(0, D), sc=(dk.sb, D), b_off=Pq.off, c_off=dk.off, alpha=a, beta=1.0)
            for b in range(nb):
                ops.gemm(dpt, k.t, dPq.t, M=R, N=D, K=T, lda=T, ldb=k.ld, ldc=dPq.ld, nb1=1, nb2=nh, sa=(0, ldp * T), sb=(0, D), sc=(0, D),
                         a_off=b * nh * ldp * T, b_off=k.off + b * k.sb, c_off=dPq.off, alpha=a, beta=1.0)
        M = nb * T
        self._wgrad(dqkv.view(M, 3 * H), h.view(M, H), self.Gqkv[l][0], self.Gqkv[l][1])
        dh_in = torch.empty_like(dO)                             # the residual path may be a queued operand: not accumulated in place
        if residual is not None:
            ops.gemm(dqkv, self.Pqkv[l][0], dh_in, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H, beta=1.0, c_in=residual)
        else:
            ops.gemm(dqkv, self.Pqkv[l][0], dh_in, M=M, N=H, K=3 * H, lda=3 * H, ldb=H, ldc=H)
        return dh_in
