"""HubertForCTC on MI355X: what the reference's loader `AutoModelForCTC.from_pretrained(checkpoint)` (wav2vec2/lib.py:20-23) builds for a
HuBERT checkpoint (hubert-large-ls960-ft, hubert-xlarge-ls960-ft), driven by the same `model(input_values).logits` (lib.py:163,413).

HuBERT for CTC is wav2vec2 under another parameter prefix (`hubert.`): both extractor layouts, the weight-normed positional conv, both
encoders, lm_head, flat parameters and the length-bucket hipGraphs are Wav2Vec2ForCTC's, of which this is a subclass.  Two things differ:
`feat_proj_layer_norm: false` builds the feature projection without its LayerNorm (the two parameters are then absent; the hook pair
_project / _project_bwd is overridden), and `masked_spec_embed` exists only when `mask_time_prob` or `mask_feature_prob` is positive, as in
transformers (it is never used in eval mode: its gradient is exactly zero).  `conv_pos_batch_norm: true` (a BatchNorm1d instead of the weight
norm on the positional conv) is refused.  Eval mode only, as the reference loop; no attention_mask (the reference passes none)."""
from . import ops
from . import wav2vec2_model as W2

DEFAULT_CONFIG = dict(W2.DEFAULT_CONFIG, feat_proj_layer_norm=True, conv_pos_batch_norm=False, mask_time_prob=0.05, mask_feature_prob=0.0)


def make_config(cfg=None):
    """wav2vec2_model.make_config plus HuBERT's keys: `feat_proj_layer_norm`, `conv_pos_batch_norm` (refused when true) and the two masking
    probabilities that decide whether `masked_spec_embed` exists."""
    out = W2.make_config(cfg, DEFAULT_CONFIG)
    if out["conv_pos_batch_norm"]:
        raise ops.DynError("conv_pos_batch_norm=true is not built: the positional conv is the weight-normed one")
    out["feat_proj_layer_norm"], out["conv_pos_batch_norm"] = bool(out["feat_proj_layer_norm"]), False
    out["mask_time_prob"], out["mask_feature_prob"] = float(out["mask_time_prob"]), float(out["mask_feature_prob"])
    return out


def config_from_json(path):
    return W2.config_from_json(path, make_config)


def param_spec(c, pf="hubert."):
    """wav2vec2_model.param_spec under HuBERT's prefix, without `feature_projection.layer_norm.*` when `feat_proj_layer_norm` is false and
    without `masked_spec_embed` when both masking probabilities are zero."""
    drop = set()
    if not c["feat_proj_layer_norm"]:
        drop |= {pf + "feature_projection.layer_norm.weight", pf + "feature_projection.layer_norm.bias"}
    if not (c["mask_time_prob"] > 0.0 or c["mask_feature_prob"] > 0.0):
        drop.add(pf + "masked_spec_embed")
    return [e for e in W2.param_spec(c, pf) if e[0] not in drop]


class HubertForCTC(W2.Wav2Vec2ForCTC):
    _prefix = "hubert."
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)

    def _project(self, a):
        if self.cfg["feat_proj_layer_norm"]:
            return super()._project(a)
        fp = self._prefix + "feature_projection."
        return ops.linear(a, self.P[fp + "projection.weight"], self.P[fp + "projection.bias"]), (a,)

    def _project_bwd(self, kept, dhs):
        if self.cfg["feat_proj_layer_norm"]:
            return super()._project_bwd(kept, dhs)
        fp = self._prefix + "feature_projection."
        return self._lin_bwd(dhs, kept[0], fp + "projection.weight", fp + "projection.bias")
