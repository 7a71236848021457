"""WavLMForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for a WavLM
checkpoint (base-plus, large and their CTC fine-tunes), driven by the same `model(input_values).logits` (lib.py:163,413).

WavLM is wav2vec2 with one more term in the attention scores; everything else (feature extractor, feature projection, weight-normed
positional conv, FFN, lm_head, both layouts through the same three flags, flat parameters, length-bucket hipGraphs) is Wav2Vec2ForCTC, of
which this is a subclass that replaces the parameter prefix (`wavlm.`), adds the per-layer gate parameters and layer 0's bias table to the
parameter list, and overrides the two attention hooks.  With h [B, T, H] the attention's input (the layer's input in the post-LN layout,
its LayerNorm in the stable-LN one), nh heads of D channels:
    p    = gru_rel_pos_linear(h[b, t, head*D:(head+1)*D])                      8 values, weight [8, D] shared by the heads of the layer
    a, c = sigmoid(p0+p1+p2+p3), sigmoid(p4+p5+p6+p7)
    gate = a * (c * gru_rel_pos_const[head] - 1) + 2                           [B, nh, T]
    P    = softmax_s(D**-0.5 q_t.k_s + gate[b, head, t] * E[bucket(s - t), head])
E = layers.0.attention.rel_attn_embed.weight [num_buckets, nh]: layer 0 owns it, EVERY layer uses it (so its gradient sums over the layers).
bucket(d) is transformers' _relative_positions_bucket: a table built on the host with the same torch expressions (ops.relative_position_buckets),
once per frame count, resident on the device.  Eval mode only, as the reference loop: no dropout, layerdrop or SpecAugment masking; no
attention_mask (the reference passes none)."""
import torch

from . import ops
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(W2.DEFAULT_CONFIG, num_buckets=320, max_bucket_distance=800)


def make_config(cfg=None):
    """wav2vec2_model.make_config plus WavLM's two keys, `num_buckets` and `max_bucket_distance`."""
    out = W2.make_config(cfg, DEFAULT_CONFIG)
    nbk = out["num_buckets"] = int(out["num_buckets"])
    out["max_bucket_distance"] = int(out["max_bucket_distance"])
    if nbk < 4 or nbk % 2 or out["max_bucket_distance"] <= nbk // 4:
        raise ops.DynError(f"num_buckets={nbk} must be even (half per sign; a quarter are exact distances) with "
                           f"max_bucket_distance={out['max_bucket_distance']} beyond the exact ones")
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def param_spec(c, pf="wavlm."):
    """wav2vec2_model.param_spec under WavLM's prefix + per layer `attention.gru_rel_pos_const` (HF shape (1, nh, 1, 1); kind "heads") and
    `attention.gru_rel_pos_linear.{weight,bias}`, + layer 0's `attention.rel_attn_embed.weight`.  Appended after the shared list: the q | k | v
    slots stay side by side."""
    nh = c["num_attention_heads"]
    spec = W2.param_spec(c, pf)
    head = spec[-2:]                                           # lm_head stays last
    spec = spec[:-2]
    for l in range(c["num_hidden_layers"]):
        p = f"{pf}encoder.layers.{l}.attention."
        spec += [(p + "gru_rel_pos_const", (nh,), "heads"), (p + "gru_rel_pos_linear.weight", (8, c["hidden_size"] // nh), None),
                 (p + "gru_rel_pos_linear.bias", (8,), None)]
    spec.append((f"{pf}encoder.layers.0.attention.rel_attn_embed.weight", (c["num_buckets"], nh), None))
    return spec + head


class WavLMForCTC(W2.Wav2Vec2ForCTC):
    _prefix = "wavlm."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        if (c["hidden_size"] // c["num_attention_heads"]) % 4:
            raise ops.DynError("WavLM's gate kernels need a head dimension that is a multiple of 4")
        self._tables = {}                                      # frame count -> device int32 bucket table [2 T - 1]

    def bucket_table(self, T):
        """The relative-position buckets of T frames on the device; built on the host the first time T is seen, never inside a capture."""
        t = self._tables.get(T)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.DynError(f"the bucket table of {T} frames has to exist before its launch sequence is captured")
            t = self._tables[T] = ops.relative_position_buckets(T, self.cfg["num_buckets"], self.cfg["max_bucket_distance"]).to(self.device)
        return t

    def forward(self, input_values):
        """As Wav2Vec2ForCTC.forward.  Under bucketed hipGraph replay the bias needs nothing new from the host: the table is sized by the
        BUCKET's frame count (distance s - t does not depend on the utterance's length), the utterance's length stays the device scalar the
        masked softmax already reads, and the parent's zero-gradient argument carries over: a padded query row gets dL/dlogits = 0 from CTC,
        hence dS = 0 for its whole row, so its dgate (a sum of dS * E), its terms of dE (gate * dS) and its terms of dh (dgate * ...) are exact
        zeros; a padded KEY column has probability 0, so dS = 0 there as well and dE sums the unpadded run's terms plus zeros."""
        x = input_values
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] >= self.samples_for_frames(1):
            T, Tb, _ = self._bucket(x.shape[1])
            self.bucket_table(T)
            if self.use_graphs:
                self.bucket_table(Tb)
        return super().forward(input_values)

    def _gate_params(self, l, of):
        p = f"{self._prefix}encoder.layers.{l}.attention."
        return of[p + "gru_rel_pos_linear.weight"], of[p + "gru_rel_pos_linear.bias"], of[p + "gru_rel_pos_const"]

    def _softmax(self, S, h, l, vT):
        W, b, k = self._gate_params(l, self.P)
        nh = self.cfg["num_attention_heads"]
        gate, a, c = ops.relpos_gate(h, W, b, k, nh)
        E = self.P[f"{self._prefix}encoder.layers.0.attention.rel_attn_embed.weight"]
        ops.softmax_relbias(S, gate, E, self.bucket_table(S.shape[-1]), h.shape[-1] // nh, out=S, valid=vT)
        return gate, a, c

    def _softmax_bwd(self, dS, kept, h, l, dh):
        gate, a, c = kept
        nh = self.cfg["num_attention_heads"]
        en = f"{self._prefix}encoder.layers.0.attention.rel_attn_embed.weight"
        dgate = ops.relbias_bwd(dS, gate, self.P[en], self.bucket_table(dS.shape[-1]), h.shape[-1] // nh, self.G[en], beta=1.0)
        W, _, k = self._gate_params(l, self.P)
        dW, db, dk = self._gate_params(l, self.G)
        ops.relpos_gate_bwd(dgate, a, c, h.contiguous(), W, k, dh, dW, db, dk, dh_beta=1.0, beta=1.0)
