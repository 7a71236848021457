"""ParakeetForRNNT on MI355X: the plain RNN transducer of the `nvidia/parakeet-rnnt-0.6b` / `-1.1b` checkpoints (`model_type:
"parakeet_rnnt"`, transformers modeling_parakeet.py: ParakeetForRNNT).  ParakeetForTDT (parakeet_tdt_model.py) is transformers' subclass of
it; here it is the other way round, because the TDT head was built first: ParakeetForRNNT subclasses ParakeetForTDT with an empty duration
list (D = 0) and overrides the handful of methods in which the two heads differ.  Shared, unchanged: the FastConformer encoder,
`encoder_projector`, the LSTM prediction network and its backward, the joint (ops.joint / joint_bwd, head Linear(Hd -> V + 1): no duration
columns), the joint streamed over frame chunks (`joint_budget`, `frames_per_chunk=`, plan_joint_chunk with N = V + 1), backward().
What differs:
  * the loss: ops.rnnt_loss (transformers.loss.loss_rnnt.rnnt_loss, a wrapper around torchaudio.functional.rnnt_loss, and its autograd):
    from (t, u) a blank arc to (t + 1, u) and a label arc to (t, u + 1), the terminal alpha(T' - 1, U) + lp_blank(T' - 1, U); rnnt_loss's
    five reductions with its default "mean_volume" (not "mean" as tdt_loss); no sigma (refused when not 0).  20 bytes of lattice state
    per cell; above ops.RNNT_WORKSPACE_BUDGET the state is refused by name.  The chunked form: ops.rnnt_arcs_chunk / rnnt_lattice_run /
    rnnt_grad_chunk, bit-equal to the whole form in loss and per-logit gradient.
  * label lengths: transformers' RNN-T forward counts `labels != blank_token_id` (TDT: `!= pad_token_id`); `label_lengths` replaces
    the count.
  * generate: ParakeetRNNTGenerationMixin's greedy decode with all state on the device (ops.rnnt_greedy_steps): a blank advances the frame
    by one, a non-blank stays, and after max_symbols_per_step non-blanks at one frame the frame advances anyway (the forced step's token
    is still emitted and fed to the prediction network).  The step cap is max_symbols_per_step * T', the number of steps the all-forced
    worst case needs to walk every frame; transformers' derived `max_length` of the same value also counts the start token and stops
    that one case a step earlier, one forced token short of the last frame.  Every other decode ends at the frame pointer and is
    identical; the tests compare the steps taken before the frame pointer reaches the end.

Refused by name before any launch: `model_type: "parakeet_tdt"` and any config that carries `durations` (parakeet_tdt_model builds
those), `attention_mask`, `sigma != 0`, and what parakeet_tdt_model.make_config refuses of the head and the encoder (a `hidden_act` of the
joint other than "relu", decoder sizes, ids outside the vocabulary).  Out of scope: beam / MAES decoding, ragged batches in the model (the
loss kernel's per-row lengths are built), a waveform front end (since built: ParakeetForCTC.generate_from_audio, frontend.MelFeatures), hipGraph replay, chunking the lattice state, `hidden_act` other than relu.
torchaudio is not needed: the tests' oracle is a plain torch recursion with autograd on transformers' own ParakeetForRNNT logits (CPU, the
same random state dict), a float64 closed form and a brute-force sum over all alignments."""
from . import ops
from . import parakeet_tdt_model as TM

DEFAULT_HEAD = {k: v for k, v in TM.DEFAULT_HEAD.items() if k != "durations"}
FROZEN_IN_THE_LOOP = TM.FROZEN_IN_THE_LOOP
plan_joint_chunk = TM.plan_joint_chunk


def make_config(cfg=None):
    """transformers' ParakeetRNNTConfig (the object, or the nested dict of a config.json; None: its defaults) -> the flat dict
    ParakeetForTDT's code reads, with `durations` empty."""
    if cfg is not None:
        get = TM._getter(cfg)
        mt = get("model_type")
        if mt == "parakeet_tdt" or get("durations") is not None:
            raise ops.DynError("ParakeetForTDT (model_type \"parakeet_tdt\", a config with `durations`) is not built by this module, the RNN-T "
                               "head (ParakeetForRNNT): parakeet_tdt_model.ParakeetForTDT builds it")
        if mt is not None and mt != "parakeet_rnnt":
            raise ops.DynError(f"model_type={mt!r} is not a ParakeetForRNNT configuration (\"parakeet_rnnt\")")
    return TM.head_config(cfg, DEFAULT_HEAD)


def config_from_json(path):
    """An HF `config.json` of a parakeet_rnnt checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def param_spec(c, pf=""):
    """transformers' state dict of ParakeetForRNNT: ParakeetForTDT's names, `joint.head` as [V + 1, Hd] (no durations)."""
    if len(c["durations"]):
        raise ops.DynError("param_spec: an RNN-T configuration has no durations")
    return TM.param_spec(c, pf)


class ParakeetForRNNT(TM.ParakeetForTDT):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    default_reduction = "mean_volume"                    # rnnt_loss's

    def head(self, enc, decoder_input_ids, labels=None, reduction=None, sigma=0.0, *args, **kw):
        """ParakeetForTDT.head with the RNN-T loss: logits [n_active, T', U + 1, V + 1], `reduction` None = "mean_volume", `sigma` must be 0."""
        if float(sigma) != 0.0:
            raise ops.DynError(f"sigma={sigma!r} is not built for ParakeetForRNNT: rnnt_loss has no sigma (it is tdt_loss's)")
        return super().head(enc, decoder_input_ids, labels, reduction, 0.0, *args, **kw)

    def _label_lengths(self, lab):
        """transformers' ParakeetForRNNT.forward counts `labels != blank_token_id`."""
        return (lab != self.blank).sum(-1).to(TM.torch.int32)

    def _loss_whole(self, logits, tg, ilen, tlen, sigma, reduction, grad_scale, want_grad):
        return ops.rnnt_loss(logits, tg, ilen, tlen, self.blank, reduction, grad_scale, want_grad=want_grad)

    def _loss_state(self, nb, T, U1, reduction, sigma):
        if reduction not in ops.TDT_REDUCTIONS:
            raise ops.DynError(f"reduction={reduction!r} is not one of {sorted(ops.TDT_REDUCTIONS)}")
        return ops.rnnt_state(nb, T, U1, self.device)                                            # over RNNT_WORKSPACE_BUDGET: refused by name

    def _loss_arcs_chunk(self, logits, t0, T, tg, tlen, state, sigma):
        ops.rnnt_arcs_chunk(logits, t0, T, tg, tlen, self.blank, state)

    def _loss_lattice_run(self, nb, T, U1, S, ilen, tlen, state, reduction, want_beta):
        return ops.rnnt_lattice_run(nb, T, U1, S, ilen, tlen, state, reduction, want_beta)

    def _loss_grad_chunk(self, logits, t0, T, tg, ilen, tlen, state, reduction, grad_scale):
        return ops.rnnt_grad_chunk(logits, t0, T, tg, ilen, tlen, self.blank, state, reduction, grad_scale, out=logits)

    def _greedy_state(self, B, cap):
        return ops.RnntGreedyState(B, self.Hd, self.cfg["num_decoder_layers"], self.V1, cap, self.start_token, self.device)

    def _greedy_steps(self, enc, valid, st, cap, n):
        P, DEC, JOINT = self.P, TM.DEC, TM.JOINT
        ops.rnnt_greedy_steps(enc, valid, P[DEC + "embedding.weight"], self._lstm_ptrs, P[DEC + "decoder_projector.weight"],
                              P[DEC + "decoder_projector.bias"], P[JOINT + "head.weight"], P[JOINT + "head.bias"], st, self.blank,
                              self.cfg["max_symbols_per_step"], cap, n)
