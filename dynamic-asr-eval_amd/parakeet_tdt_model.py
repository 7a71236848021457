"""ParakeetForTDT on MI355X: the token-and-duration transducer of the `nvidia/parakeet-tdt-*` checkpoints (`model_type: "parakeet_tdt"`,
transformers modeling_parakeet.py: ParakeetForTDT) as transformers builds it in plain torch.  The encoder is ParakeetForCTC's
(parakeet_model.py), kernel for kernel, without the `ctc_head`; behind it:
  * `encoder_projector`: Linear(H -> Hd) on the encoder's last hidden states (the existing GEMM).
  * the prediction network (ParakeetRNNTDecoder): Embedding(V + 1, Hd) -> LSTM(Hd, Hd, layers, batch_first) from a zero state ->
    Linear(Hd, Hd), teacher-forced over the U + 1 decoder inputs.  Per layer x W_ih^T + b_ih of ALL steps is one GEMM, h W_hh^T + b_hh one
    small GEMM per step, the cell is ops.lstm_cell (csrc/transducer.hip, gate order i, f, g, o).  Activations are kept time-major
    ([U + 1, B, .]): a step's rows are contiguous.  Backward: ops.lstm_cell_bwd per step, the recurrent data gradient through
    ops.linear_dgrad accumulated into the step below, the four weight gradients one product each over all steps at the end.
  * the joint (ParakeetTDTJointNetwork): z = relu(enc[:, :, None] + dec[:, None]) (ops.joint), head Linear(Hd -> V + 1 + D) over
    [B, T', U + 1, Hd] by the existing GEMM (M = B T' (U + 1)).  The decoder rows may be ONE row set shared by the batch
    (decoder_input_ids [1, U + 1]: the loop's copies carry identical labels); their gradient then sums over the batch as well.
  * the loss: ops.tdt_loss (transformers.loss.loss_tdt.tdt_loss and its autograd: arc log-probs, lattice, gradient), the five reductions
    of tdt_loss with default "mean", plus sigma.  The lattice STATE (arc log-probs, alpha, beta: 44 bytes per cell at D = 5) is always
    whole; above ops.TDT_WORKSPACE_BUDGET it is refused by name.
  * the joint over frame chunks: z, the logits and dz are 4 (2 Hd + V + 1 + D) bytes per lattice cell, 35 KB at the released head.  When
    a loss is asked for and they do not fit `joint_budget` (ops.TDT_JOINT_BUDGET; plan_joint_chunk picks the frames per chunk, head's
    `frames_per_chunk=` overrides it), nothing of the joint is kept.  Pass 1, per chunk of Tc frames: z_c, logits_c, their arc
    log-probs into the state (ops.tdt_arcs_chunk), then both are dropped.  Pass 2: the lattice and the reduction on the state
    (ops.tdt_lattice_run).  Pass 3, in backward(), chunks ascending: z_c and logits_c once more, the gradient over logits_c
    (ops.tdt_grad_chunk), the head's weight and bias gradients accumulated, dz_c, de of the chunk's frames and dp added to the earlier
    chunks' (ops.joint_bwd_chunk).  The same kernels as the whole path: loss and per-logit gradient are bit-equal, sums over frames (dp,
    the head's gradients) differ by their order.  One more head GEMM per step; `logits` of the output is None, an explicit
    `grad_logits` is refused.  What backward() needs (state, e, p) lives in tensors of the call, never in the shared scratch.
  * generate: the duration-aware greedy decode of ParakeetTDTGenerationMixin with all state on the device (ops.tdt_greedy_steps); the
    host reads the done flags once per chunk of steps.  The frame pointer advances by durations[argmax] (transformers adds the argmax
    INDEX, the same thing for the released checkpoints' durations 0 .. D - 1), by 1 for a blank with duration 0.

Refused by name before any launch: `attention_mask`, a `hidden_act` of the joint other than "relu", more than 8 durations, negative or
unsorted durations, `model_type: "parakeet_rnnt"` (ParakeetForRNNT: no duration head; parakeet_rnnt_model builds it on this class), and whatever
parakeet_model.make_config refuses of the encoder.  Out of scope: beam / MAES decoding, ragged batches in the model (the loss kernel's
per-row lengths are built), a waveform front end (since built: ParakeetForCTC.generate_from_audio, frontend.MelFeatures), hipGraph replay and lockstep groups, chunking the joint over u or the lattice state, a
log-sum-exp in the GEMM's epilogue that never writes the logits.  No hub checkpoint is
on the machine: transformers' ParakeetForTDT on the CPU with the same (random) state dict is the oracle in the tests."""
from types import SimpleNamespace

import torch

from . import ops
from . import parakeet_model as PM
from ._lib import check, load

DEFAULT_HEAD = dict(vocab_size=8193, decoder_hidden_size=640, num_decoder_layers=2, hidden_act="relu", max_symbols_per_step=10, pad_token_id=2,
                    blank_token_id=8192, durations=(0, 1, 2, 3, 4), decoder_start_token_id=None)
DEC, JOINT, PROJ = "decoder.", "joint.", "encoder_projector."
FROZEN_IN_THE_LOOP = (PM.SUB, DEC)          # nvidia_ctc/lib.py:81-86: pre_encode and NeMo's `decoder`, here the prediction network


def make_config(cfg=None):
    """transformers' ParakeetTDTConfig (the object, or the nested dict of a config.json; None: its defaults) -> the flat dict this module
    reads: parakeet_model.make_config's encoder keys plus the head's.  The joint's `hidden_act` is kept as `joint_hidden_act` (the
    encoder has a `hidden_act` of its own)."""
    get = _getter(cfg)
    if cfg is not None:
        mt = get("model_type")
        if mt == "parakeet_rnnt" or (mt is None and get("durations") is None and type(cfg).__name__ == "ParakeetRNNTConfig"):
            raise ops.DynError("ParakeetForRNNT (model_type \"parakeet_rnnt\") is not built by this module, the TDT head (ParakeetForTDT): "
                               "parakeet_rnnt_model.ParakeetForRNNT builds it")
        if mt is not None and mt != "parakeet_tdt":
            raise ops.DynError(f"model_type={mt!r} is not a ParakeetForTDT configuration (\"parakeet_tdt\")")
    return head_config(cfg, DEFAULT_HEAD)


def _getter(cfg):
    return (lambda k: cfg.get(k)) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k, None))


def head_config(cfg, defaults, encoder=PM.make_config):
    """make_config behind the model_type check, for both transducer heads: `defaults` holds the head's keys (with `durations`: TDT;
    without: RNN-T, `durations` of the result is then empty and the joint head is [V + 1, Hd]).  `encoder`: the configuration reader of
    the encoder (a model of the family with another encoder, nemotron_asr_streaming_model.py)."""
    get = _getter(cfg)
    head = dict(defaults)
    if cfg is not None:
        for k in head:
            v = get(k)
            if v is not None:
                head[k] = v
    out = encoder({"encoder_config": None if cfg is None else get("encoder_config"), "vocab_size": head["vocab_size"],
                   "pad_token_id": head["pad_token_id"]})
    if head["hidden_act"] not in ops.JOINT_ACTS:
        raise ops.DynError(f"hidden_act={head['hidden_act']!r} of the joint is not built ({sorted(ops.JOINT_ACTS)})")
    out["joint_hidden_act"] = head["hidden_act"]
    out["durations"] = ops.check_durations(head["durations"]) if "durations" in head else ()
    Hd, L, V1 = (int(head[k]) for k in ("decoder_hidden_size", "num_decoder_layers", "vocab_size"))
    if Hd < 4 or Hd % 4:
        raise ops.DynError(f"decoder_hidden_size={Hd} is not built: a positive multiple of 4 (16-byte rows)")
    if not 1 <= L <= 8:
        raise ops.DynError(f"num_decoder_layers={L} is not built (1 .. 8)")
    blank = int(head["blank_token_id"])
    if not 0 <= blank < V1:
        raise ops.DynError(f"blank_token_id={blank} lies outside the vocabulary of {V1}")
    start = head["decoder_start_token_id"]
    if start is not None and not 0 <= int(start) < V1:
        raise ops.DynError(f"decoder_start_token_id={start} lies outside the vocabulary of {V1}")
    out.update(decoder_hidden_size=Hd, num_decoder_layers=L, blank_token_id=blank, max_symbols_per_step=int(head["max_symbols_per_step"]),
               decoder_start_token_id=None if start is None else int(start))
    if out["max_symbols_per_step"] < 1:
        raise ops.DynError(f"max_symbols_per_step={out['max_symbols_per_step']} must be positive")
    return out


def config_from_json(path):
    """An HF `config.json` of a parakeet_tdt checkpoint -> make_config."""
    import json
    with open(path) as f:
        src = json.load(f)
    if not isinstance(src, dict):
        raise ops.DynError(f"{path}: expected a JSON object")
    return make_config(src)


def param_spec(c, pf=""):
    """transformers' state dict of ParakeetForTDT: the encoder's names (parakeet_model.param_spec without the ctc_head), then
    encoder_projector, decoder.embedding, decoder.lstm.{weight,bias}_{ih,hh}_l{k}, decoder.decoder_projector, joint.head."""
    H, Hd, V1, D = c["hidden_size"], c["decoder_hidden_size"], c["vocab_size"], len(c["durations"])
    spec = [s for s in PM.param_spec(c, pf) if not s[0].startswith(pf + "ctc_head.")]
    spec += [(pf + PROJ + "weight", (Hd, H), None), (pf + PROJ + "bias", (Hd,), None), (pf + DEC + "embedding.weight", (V1, Hd), None)]
    for k in range(c["num_decoder_layers"]):
        spec += [(pf + DEC + f"lstm.weight_ih_l{k}", (4 * Hd, Hd), None), (pf + DEC + f"lstm.weight_hh_l{k}", (4 * Hd, Hd), None),
                 (pf + DEC + f"lstm.bias_ih_l{k}", (4 * Hd,), None), (pf + DEC + f"lstm.bias_hh_l{k}", (4 * Hd,), None)]
    spec += [(pf + DEC + "decoder_projector.weight", (Hd, Hd), None), (pf + DEC + "decoder_projector.bias", (Hd,), None),
             (pf + JOINT + "head.weight", (V1 + D, Hd), None), (pf + JOINT + "head.bias", (V1 + D,), None)]
    return spec


def plan_joint_chunk(B, T, U1, Hd, N, budget):
    """Pure host function: the frames per chunk of the joint.  One frame of z + logits + dz is B * U1 * (2 Hd + N) * 4 bytes; the result
    is the largest Tc in 1 .. T whose chunk fits `budget` bytes (1 when not even one frame does: the head then runs frame by frame,
    over the budget, rather than not at all).  Tc == T means the whole joint fits: unchunked."""
    B, T, U1, Hd, N, budget = (int(v) for v in (B, T, U1, Hd, N, budget))
    if min(B, T, U1, Hd, N) < 1:
        raise ops.DynError(f"plan_joint_chunk: B, T, U1, Hd, N = {(B, T, U1, Hd, N)} must be positive")
    frame = B * U1 * (2 * Hd + N) * 4
    return max(1, min(T, budget // frame))


def _host_ids(t, what, vocab):
    """An integer tensor (host or device) or nested list -> int64 host tensor [rows, n], every id inside the vocabulary."""
    t = torch.as_tensor(t).detach().cpu()
    if t.numel() == 0:
        t = t.to(torch.int64)
    if t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
        raise ops.DynError(f"{what} must be an integer tensor [rows, n], got {tuple(t.shape)} {t.dtype}")
    t = t.long()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= vocab):
        raise ops.DynError(f"{what}: ids must lie in [0, {vocab})")
    return t


class ParakeetForTDT(PM.ParakeetForCTC):
    _make_config = staticmethod(make_config)
    _param_spec = staticmethod(param_spec)
    frozen_in_the_loop = FROZEN_IN_THE_LOOP
    greedy_chunk = 32                                    # greedy steps queued per host call; the done flags are read once per chunk
    default_reduction = "mean"                           # tdt_loss's

    def __init__(self, config=None, device="cuda:0"):
        super().__init__(config, device)
        c = self.cfg
        self.Hd, self.V1, self.D = c["decoder_hidden_size"], c["vocab_size"], len(c["durations"])
        self.blank = c["blank_token_id"]
        self.start_token = c["decoder_start_token_id"] if c["decoder_start_token_id"] is not None else self.blank
        self._tdt = None
        self.joint_budget = ops.TDT_JOINT_BUDGET             # bytes of z + logits + dz held at once; above it the joint streams over frame chunks
        names = [DEC + f"lstm.{n}_l{k}" for k in range(c["num_decoder_layers"]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        self._lstm_ptrs = torch.tensor([self.P[n].data_ptr() for n in names], dtype=torch.int64, device=self.device)

    def __call__(self, x=None, **kw):
        return self.forward(kw.pop(self._input, x), **kw)

    def _decoder_frozen(self):
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith(DEC))

    def _encoder_frozen(self):
        return not any(self.trainable(n) for n, _ in self.spec if n.startswith(("encoder.", PROJ)))

    # ------------------------------------------------------------------ what differs between the transducer heads (ParakeetForRNNT overrides)
    def _label_lengths(self, lab):
        """transformers' ParakeetForTDT.forward counts `labels != pad_token_id`."""
        return (lab != self.cfg["pad_token_id"]).sum(-1).to(torch.int32)

    def _loss_whole(self, logits, tg, ilen, tlen, sigma, reduction, grad_scale, want_grad):
        return ops.tdt_loss(logits, tg, ilen, tlen, self.blank, self.cfg["durations"], sigma, reduction, grad_scale, want_grad=want_grad)

    def _loss_state(self, nb, T, U1, reduction, sigma):
        if reduction not in ops.TDT_REDUCTIONS:
            raise ops.DynError(f"reduction={reduction!r} is not one of {sorted(ops.TDT_REDUCTIONS)}")
        return ops.tdt_state(nb, T, U1, self.cfg["durations"], self.device)                       # over TDT_WORKSPACE_BUDGET: refused by name

    def _loss_arcs_chunk(self, logits, t0, T, tg, tlen, state, sigma):
        ops.tdt_arcs_chunk(logits, t0, T, tg, tlen, self.blank, self.cfg["durations"], state, sigma)

    def _loss_lattice_run(self, nb, T, U1, S, ilen, tlen, state, reduction, want_beta):
        return ops.tdt_lattice_run(nb, T, U1, S, ilen, tlen, self.cfg["durations"], state, reduction, want_beta)

    def _loss_grad_chunk(self, logits, t0, T, tg, ilen, tlen, state, reduction, grad_scale):
        return ops.tdt_grad_chunk(logits, t0, T, tg, ilen, tlen, self.blank, self.cfg["durations"], state, reduction, grad_scale, out=logits)

    def _greedy_state(self, B, cap):
        return ops.TdtGreedyState(B, self.Hd, self.cfg["num_decoder_layers"], self.V1 + self.D, cap, self.start_token, self.device)

    def _greedy_steps(self, enc, valid, st, cap, n):
        P = self.P
        ops.tdt_greedy_steps(enc, valid, P[DEC + "embedding.weight"], self._lstm_ptrs, P[DEC + "decoder_projector.weight"],
                             P[DEC + "decoder_projector.bias"], P[JOINT + "head.weight"], P[JOINT + "head.bias"], st, self.cfg["durations"],
                             self.blank, cap, n)

    # ------------------------------------------------------------------ encoder
    def _project_enc(self, x, save):
        """The encoder's last hidden states x [B, T', H] -> (the projected states [B, T', Hd], what _project_enc_bwd needs besides x, or
        None): `encoder_projector`.  A model with more between the encoder and the projector (nemotron3_5_asr_model.py) overrides the
        pair; a streaming session calls it too.  (Not `_project`: that is the feature projection of the waveform models this family
        inherits from.)"""
        return ops.linear(x, self.P[PROJ + "weight"], self.P[PROJ + "bias"]), None

    def _project_enc_bwd(self, de, ctx, cut):
        """Backward of _project_enc from de [nb, T', Hd]: accumulates its parameters' gradients, returns dL/dx [nb, T', H]."""
        return self._lin_bwd(de, cut(ctx["head"]), PROJ + "weight", PROJ + "bias")

    def _encode(self, h, ctx, vT, dims, v0):
        T = dims[2]
        x = self._layers_fwd(h, ctx, vT, self.position_table(T))
        enc, kept = self._project_enc(x, ctx is not None)
        if ctx is not None:
            ctx["head"] = x
            ctx["project"] = kept
            ctx["dims"] = dims
            ctx["valid"] = (v0, vT)
        self._ctx = ctx
        return SimpleNamespace(enc=enc, frames=T)

    def encode(self, input_features, attention_mask=None, input_lengths=None):
        """input_features [B, T, num_mel_bins] -> the projected encoder states [B, T', Hd] (transformers' `pooler_output`).  In grad mode
        the encoder's activations are kept for a later head() + backward().  `input_lengths` (ParakeetForCTC.forward): the valid
        frames per row of a ragged batch; head() and generate() given this call's result find the rows' encoder frame counts
        (`enc_lengths`) themselves."""
        self._tdt = None
        out = PM.ParakeetForCTC.forward(self, input_features, attention_mask, *(() if input_lengths is None else (input_lengths,)))
        self._remember_lengths(out.enc, out)
        return out.enc

    # ------------------------------------------------------------------ prediction network
    def _decoder_fwd(self, ids, save):
        """ids int64 host [Bd, U1] -> (p [U1, Bd, Hd] time-major, what _decoder_bwd needs or None)."""
        P, c, Hd = self.P, self.cfg, self.Hd
        Bd, U1 = ids.shape
        ids_tm = ids.t().contiguous().to(torch.int32).to(self.device).view(-1)                     # [U1 * Bd], step-major
        x = torch.empty(U1, Bd, Hd, device=self.device, dtype=torch.float32)
        check(load().dyn_embedding_fwd(ids_tm.data_ptr(), P[DEC + "embedding.weight"].data_ptr(), None, x.data_ptr(), U1 * Bd, Hd, self.V1, 1,
                                       torch.cuda.current_stream().cuda_stream), "dyn_embedding_fwd")
        kept = []
        zeros = torch.zeros(Bd, Hd, device=self.device, dtype=torch.float32)
        for k in range(c["num_decoder_layers"]):
            w_ih, w_hh, b_ih, b_hh = (P[DEC + f"lstm.{n}_l{k}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            xg = ops.linear(x.view(U1 * Bd, Hd), w_ih, b_ih).view(U1, Bd, 4 * Hd)                  # every step's input half: one GEMM
            h_all = torch.empty(U1, Bd, Hd, device=self.device, dtype=torch.float32)
            c_all = torch.empty(U1, Bd, Hd, device=self.device, dtype=torch.float32)
            g_all = torch.empty(U1, Bd, 4 * Hd, device=self.device, dtype=torch.float32) if save else None
            for u in range(U1):
                hg = ops.linear(h_all[u - 1] if u else zeros, w_hh, b_hh)
                ops.lstm_cell(xg[u], hg, c_all[u - 1] if u else None, out=(c_all[u], h_all[u], g_all[u] if save else None))
            if save:
                kept.append((x, h_all, c_all, g_all))
            x = h_all
        p = ops.linear(x.view(U1 * Bd, Hd), P[DEC + "decoder_projector.weight"], P[DEC + "decoder_projector.bias"]).view(U1, Bd, Hd)
        return p, ((ids_tm, kept) if save else None)

    def _decoder_bwd(self, dp, saved):
        """dp [U1, Bd, Hd] time-major: accumulates the prediction network's gradients."""
        P, G, c, Hd = self.P, self.G, self.cfg, self.Hd
        ids_tm, kept = saved
        U1, Bd, _ = dp.shape
        top = kept[-1][1]
        d = self._lin_bwd(dp.view(U1 * Bd, Hd), top.view(U1 * Bd, Hd), DEC + "decoder_projector.weight", DEC + "decoder_projector.bias")
        for k in reversed(range(c["num_decoder_layers"])):
            x, h_all, c_all, g_all = kept[k]
            names = [DEC + f"lstm.{n}_l{k}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            w_ih, w_hh = P[names[0]], P[names[1]]
            dh_all = d.view(U1, Bd, Hd)                      # the gradient from above; the recurrent gradient is added step by step
            dg_all = torch.empty_like(g_all)
            dc = None
            for u in reversed(range(U1)):
                _, dc = ops.lstm_cell_bwd(dh_all[u], dc, g_all[u], c_all[u - 1] if u else None, c_all[u], dgates=dg_all[u])
                if u:
                    ops.linear_dgrad(dg_all[u], w_hh, out=dh_all[u - 1], beta=1.0)
            dg = dg_all.view(U1 * Bd, 4 * Hd)
            if any(self.trainable(n) for n in names):
                self._wgrad(dg, x.view(U1 * Bd, Hd), G[names[0]], G[names[2]])
                if U1 > 1:                                   # h_{-1} = 0: step 0 adds nothing to the recurrent weight
                    self._wgrad(dg_all[1:].view((U1 - 1) * Bd, 4 * Hd), h_all[:-1].view((U1 - 1) * Bd, Hd), G[names[1]], None)
                ops.colsum(dg, G[names[3]], beta=1.0)
            d = ops.linear_dgrad(dg, w_ih)
        if self.trainable(DEC + "embedding.weight"):
            check(load().dyn_embedding_bwd(ids_tm.data_ptr(), d.data_ptr(), G[DEC + "embedding.weight"].data_ptr(), U1 * Bd, Hd, self.V1, 1.0,
                                           torch.cuda.current_stream().cuda_stream), "dyn_embedding_bwd")

    # ------------------------------------------------------------------ joint, loss
    def _joint_frames(self, nb, T, U1, frames_per_chunk):
        """Frames per chunk of the joint for a loss on [nb, T, U1]: the override, or plan_joint_chunk under joint_budget.  T: unchunked."""
        if frames_per_chunk is None:
            return plan_joint_chunk(nb, T, U1, self.Hd, self.V1 + self.D, self.joint_budget)
        if isinstance(frames_per_chunk, bool) or not isinstance(frames_per_chunk, int) or frames_per_chunk < 1:
            raise ops.DynError(f"frames_per_chunk={frames_per_chunk!r} must be a positive integer")
        return min(frames_per_chunk, T)

    def _joint_chunk(self, e, p, t0, n, zbuf, lbuf):
        """z and the logits of the frames [t0, t0 + n) into the front of the two chunk buffers: ([nb, n, U1, Hd], [nb, n, U1, V + 1 + D])."""
        P, Hd = self.P, self.Hd
        nb, U1, N = e.shape[0], p.shape[0], self.V1 + self.D
        z = ops.joint(e[:, t0:t0 + n].contiguous(), p.transpose(0, 1), self.cfg["joint_hidden_act"], out=zbuf[:nb * n * U1 * Hd].view(nb, n, U1, Hd))
        return z, ops.linear(z, P[JOINT + "head.weight"], P[JOINT + "head.bias"], out=lbuf[:nb * n * U1 * N].view(nb, n, U1, N))

    def _chunk_buffers(self, nb, Tc, U1, dz):
        n = nb * Tc * U1
        new = lambda k: torch.empty(n * k, device=self.device, dtype=torch.float32)                # noqa: E731
        return new(self.Hd), new(self.V1 + self.D), (new(self.Hd) if dz else None)

    def _head_chunked(self, e, p, Tc, tg, ilen, tlen, reduction, sigma, want_beta):
        """Passes 1 and 2 of the chunked loss: the arcs of every chunk of Tc frames into a lattice state this call owns (the joint of a
        chunk is dropped as soon as its arcs are written), then the lattice -> (loss, nll, state)."""
        nb, T, _ = e.shape
        U1 = p.shape[0]
        state = self._loss_state(nb, T, U1, reduction, sigma)
        zbuf, lbuf, _ = self._chunk_buffers(nb, Tc, U1, False)
        for t0 in range(0, T, Tc):
            _, logits = self._joint_chunk(e, p, t0, min(Tc, T - t0), zbuf, lbuf)
            self._loss_arcs_chunk(logits, t0, T, tg, tlen, state, sigma)
        loss, nll = self._loss_lattice_run(nb, T, U1, tg.shape[1], ilen, tlen, state, reduction, want_beta)
        return loss, nll, state

    def head(self, enc, decoder_input_ids, labels=None, reduction=None, sigma=0.0, grad_scale=1.0, n_active=None, label_lengths=None,
             frames_per_chunk=None, enc_lengths=None):
        """The prediction network, the joint and (with labels) the TDT loss on the first n_active rows of enc [B, T', Hd].
        decoder_input_ids [n_active or 1, U + 1] (one row: shared by every copy); labels [same rows, U], padded with pad_token_id
        (transformers counts `labels != pad_token_id`; `label_lengths`, one per label row, replaces that count: unpadded labels may
        hold the pad id).  `enc_lengths` (_lengths_of): the valid frames per row of enc, the loss's logit lengths; the logits past them
        carry no meaning.
        Returns SimpleNamespace(logits [n_active, T', U + 1, V + 1 + D], loss [1] or None, nll [n_active] or None).  In grad mode the
        loss's gradient w.r.t. the logits, times grad_scale, is kept for backward().
        With labels, when z + logits + dz of the whole joint do not fit `joint_budget` bytes (or `frames_per_chunk` < T' is given), the
        joint streams over chunks of frames (module docstring): `logits` is then None, loss and nll are those of the whole-joint path,
        and backward() recomputes the joint chunk by chunk."""
        c, P, Hd = self.cfg, self.P, self.Hd
        reduction = self.default_reduction if reduction is None else reduction
        B, T, _ = enc.shape
        nb = B if n_active is None else int(n_active)
        if not 1 <= nb <= B:
            raise ops.DynError(f"n_active={n_active!r} must lie in 1 .. {B}")
        ids = _host_ids(decoder_input_ids, "decoder_input_ids", self.V1)
        if ids.shape[0] not in (1, nb) or ids.shape[1] < 1:
            raise ops.DynError(f"decoder_input_ids {tuple(ids.shape)} must be [{nb} or 1, U + 1]")
        U1 = ids.shape[1]
        rows_T = self._lengths_of(enc, enc_lengths, nb)
        Tc = T if labels is None else self._joint_frames(nb, T, U1, frames_per_chunk)
        grad_mode = torch.is_grad_enabled() and self._ctx is not None
        with ops.use_workspace(self._scratch()):
            run_dec_bwd = grad_mode and not self._decoder_frozen()
            p, dec_saved = self._decoder_fwd(ids, run_dec_bwd)
            e = enc[:nb].contiguous()
            z = logits = None
            if Tc >= T:
                z = ops.joint(e, p.transpose(0, 1), c["joint_hidden_act"])
                logits = ops.linear(z, P[JOINT + "head.weight"], P[JOINT + "head.bias"])
            loss = nll = dlogits = chunked = None
            if labels is not None:
                lab = _host_ids(labels, "labels", self.V1)
                if lab.shape[0] != ids.shape[0] or lab.shape[1] != U1 - 1:
                    raise ops.DynError(f"labels {tuple(lab.shape)} must be [{ids.shape[0]}, {U1 - 1}]: one label per decoder input after the start token")
                if lab.shape[0] == 1 and nb > 1:
                    lab = lab.expand(nb, -1)
                if label_lengths is None:
                    tlen = self._label_lengths(lab)
                else:
                    tlen = torch.as_tensor(list(label_lengths), dtype=torch.int32).reshape(-1)
                    if tlen.numel() == 1 and nb > 1:
                        tlen = tlen.expand(nb).contiguous()
                    if tlen.numel() != nb or int(tlen.min()) < 0 or int(tlen.max()) > U1 - 1:
                        raise ops.DynError(f"label_lengths {tlen.tolist()} must be {nb} (or 1) values in 0 .. {U1 - 1}")
                tg = (lab.to(torch.int32).contiguous() if U1 > 1 else torch.zeros(nb, 1, dtype=torch.int32)).to(self.device)
                ilen = torch.full((nb,), T, dtype=torch.int32, device=self.device) if rows_T is None else rows_T
                tlen = tlen.to(self.device)
                if Tc >= T:
                    loss, nll, dlogits = self._loss_whole(logits, tg, ilen, tlen, float(sigma), reduction, float(grad_scale), grad_mode)
                else:
                    loss, nll, state = self._head_chunked(e, p, Tc, tg, ilen, tlen, reduction, float(sigma), grad_mode)
                    # what the gradient pass needs, in tensors of this call's own: nothing of it lives in the shared scratch
                    chunked = dict(frames=Tc, e=e, p=p, state=state, tg=tg, ilen=ilen, tlen=tlen, reduction=reduction, grad_scale=float(grad_scale))
        self._tdt = dict(z=z, p_rows=ids.shape[0], dec=dec_saved, rows=nb, dlogits=dlogits, chunked=chunked) if grad_mode else None
        return SimpleNamespace(logits=logits, loss=loss, nll=nll, frames=T)

    def forward(self, input_features, decoder_input_ids=None, labels=None, attention_mask=None, reduction=None, sigma=0.0, grad_scale=1.0,
                n_active=None, label_lengths=None, frames_per_chunk=None, input_lengths=None):
        """input_features [B, T, num_mel_bins] float32 on the device, decoder_input_ids [B or 1, U + 1] -> SimpleNamespace(logits
        [B, T', U + 1, V + 1 + D] (None when the joint was chunked: head()), loss, nll, frames = T', enc [B, T', Hd]).  `attention_mask`
        is refused.  `input_lengths` (ParakeetForCTC.forward): the valid frames per row of a ragged batch; the rows' encoder frame counts
        become the loss's logit lengths and the result's `lengths` (host list) / `lengths_device`."""
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built: every frame of input_features is taken as valid; a ragged batch passes "
                               "input_lengths (parakeet_model.lengths_from_mask turns a prefix mask into them)")
        if decoder_input_ids is None:
            raise ops.DynError("forward() needs decoder_input_ids [B or 1, U + 1] (start token + labels); generate() decodes without them")
        enc = self.encode(input_features, attention_mask, *(() if input_lengths is None else (input_lengths,)))
        out = self.head(enc, decoder_input_ids, labels, reduction, sigma, grad_scale, n_active, label_lengths, frames_per_chunk)
        out.enc = enc
        if input_lengths is not None:
            out.lengths, out.lengths_device = self._enc_lengths[1:]
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, grad_logits=None, n_active=None):
        """Accumulates every parameter's gradient into flat_grads: of grad_scale * loss of the last grad-mode forward with labels, or of
        sum(grad_logits * logits) for a given grad_logits [n_active, T', U + 1, V + 1 + D].  The joint ran on the first n_active rows of
        the forward; under batch_renorm_training() the encoder's backward still covers every row (zeros for the rest)."""
        t = self._tdt
        if t is None:
            raise ops.DynError("backward() without a grad-mode forward through the joint")
        if n_active is not None and int(n_active) != t["rows"]:
            raise ops.DynError(f"backward(n_active={n_active}) after a forward whose joint ran on {t['rows']} rows")
        if t.get("chunked") is not None:
            if grad_logits is not None:
                raise ops.DynError("backward(grad_logits=...) after a chunked forward is not built: the joint streamed over chunks of "
                                   f"{t['chunked']['frames']} frames and the logits were never whole; backward() without grad_logits takes the "
                                   "loss's own gradient (or run the forward with a joint_budget / frames_per_chunk that keeps the joint whole)")
        else:
            g = t["dlogits"] if grad_logits is None else grad_logits
            if g is None:
                raise ops.DynError("backward() needs grad_logits: the last forward had no labels")
            if tuple(g.shape) != tuple(t["z"].shape[:3]) + (self.V1 + self.D,):
                raise ops.DynError(f"grad_logits {tuple(g.shape)} does not fit the joint logits")
            t["g"] = g.contiguous()
        B = self._ctx["dims"][0]
        nb = B if self._ctx_brn else t["rows"]          # batch renorm: the gradient reaches every row through the batch statistics
        # the parent's surface hands dL/dlogits [nb, ..] down to _backward_encoder; the joint's gradient waits in self._tdt instead
        # (its rows may be fewer than the encoder's), the placeholder only carries nb
        try:
            super().backward(torch.empty(nb, 0, device=self.device), None if nb == B else nb)
        finally:
            self._tdt = None

    def _joint_bwd_chunked(self, t, need_enc, need_dec):
        """Pass 3 of the chunked loss, chunks in ascending order: the joint and the logits of a chunk once more, the loss's gradient written
        over those logits, the head's weight and bias gradients accumulated at once (not through the deferred queue: the chunk buffers are
        reused), dz, then de of the chunk's frames and dp added to the chunks before -> (de [rows, T', Hd] or None, dp time-major or None)."""
        P, G, Hd, N = self.P, self.G, self.Hd, self.V1 + self.D
        k = t["chunked"]
        e, p, Tc = k["e"], k["p"], k["frames"]
        rows, T, _ = e.shape
        U1 = p.shape[0]
        wn, bn = JOINT + "head.weight", JOINT + "head.bias"
        head_grads, need_dz = self.trainable(wn) or self.trainable(bn), need_enc or need_dec
        if not (head_grads or need_dz):
            return None, None
        zbuf, lbuf, dzbuf = self._chunk_buffers(rows, Tc, U1, need_dz)
        de = torch.empty(rows, T, Hd, device=self.device, dtype=torch.float32) if need_enc else None
        dp = torch.empty(U1, t["p_rows"], Hd, device=self.device, dtype=torch.float32) if need_dec else None
        for t0 in range(0, T, Tc):
            z, logits = self._joint_chunk(e, p, t0, min(Tc, T - t0), zbuf, lbuf)
            g = self._loss_grad_chunk(logits, t0, T, k["tg"], k["ilen"], k["tlen"], k["state"], k["reduction"], k["grad_scale"]).view(-1, N)
            if head_grads:                                   # as _lin_bwd: both sums unless both are frozen
                ops.linear_wgrad(g, z.view(-1, Hd), G[wn], beta=1.0)
                ops.colsum(g, G[bn], beta=1.0)
            if need_dz:
                dz = ops.linear_dgrad(g, P[wn], out=dzbuf[:z.numel()].view(-1, Hd)).view(z.shape)
                ops.joint_bwd_chunk(dz, z, de, dp, t0, t0 > 0, self.cfg["joint_hidden_act"], time_major=True)
        return de, dp

    def _backward_encoder(self, ctx, grad_logits, nb, cut):
        t, P = self._tdt, self.P
        v0, vT = ctx["valid"]
        T = ctx["dims"][2]
        rows, Hd = t["rows"], self.Hd
        need_dec, need_enc = t["dec"] is not None, not self._encoder_frozen()
        if t["chunked"] is not None:
            de, dp = self._joint_bwd_chunked(t, need_enc, need_dec)
            if not (need_dec or need_enc):
                return None
        else:
            z, g = t["z"], t["g"]
            U1 = z.shape[2]
            dz = self._lin_bwd(g.view(-1, g.shape[-1]), z.view(-1, Hd), JOINT + "head.weight", JOINT + "head.bias").view(z.shape)
            if not (need_dec or need_enc):
                return None
            de, dp = ops.joint_bwd(dz, z, torch.empty(t["p_rows"], U1, Hd, device="meta"), self.cfg["joint_hidden_act"], want_de=need_enc,
                                   want_dp=need_dec, time_major=True)
        if need_dec:
            self._decoder_bwd(dp, t["dec"])
        if not need_enc:
            return None
        if rows < nb:                                    # batch renorm: zero gradient rows for the copies the loss did not see
            full = torch.zeros(nb, T, Hd, device=self.device, dtype=torch.float32)
            full[:rows] = de
            de = full
        lens = ctx.get("lens")
        if lens is not None:                             # a ragged batch: no gradient enters at a padded frame, whatever the joint left there
            vT, lens = vT.cut(nb), lens[:, :nb]
            de = ops.mask_rows_lens(de.contiguous(), lens[3])
        dx = self._project_enc_bwd(de, ctx, cut)
        dh = self._layers_bwd(ctx, dx, nb, T, self.position_table(T), vT, cut)
        if not self._below_frozen():
            self._subsample_bwd(cut(ctx["sub"]), dh, *(() if lens is None else (lens,)))
        return None

    # ------------------------------------------------------------------ greedy decode
    def generate(self, input_features=None, enc=None, input_lengths=None, enc_lengths=None):
        """Greedy TDT decode of input_features [B, T, num_mel_bins] (or of projected encoder states `enc` [B, T', Hd]) ->
        SimpleNamespace(tokens int32 [B, Nmax], frames int32 [B, Nmax] (the encoder frame at which each non-blank token was emitted),
        count int32 [B], steps int32 [B]).  At most max_symbols_per_step * T' steps per row, transformers' derived max_length.
        A ragged batch: `input_lengths` with input_features, `enc_lengths` (_lengths_of) with enc; every row decodes its own frames."""
        c = self.cfg
        with torch.no_grad():
            if enc is None:
                keep = self._ctx, self._tdt
                enc = self.encode(input_features, None, *(() if input_lengths is None else (input_lengths,)))
                self._ctx, self._tdt = keep
            elif input_lengths is not None:
                raise ops.DynError("generate(enc=..., input_lengths=...): input_lengths counts feature frames; pass enc_lengths with enc")
            rows_T = self._lengths_of(enc, enc_lengths, enc.shape[0])
            enc = enc.detach().contiguous()
            B, T, _ = enc.shape
            cap = c["max_symbols_per_step"] * T
            st = self._greedy_state(B, cap)
            valid = torch.full((B,), T, dtype=torch.int32, device=self.device) if rows_T is None else rows_T
            done = 0
            while done < cap:
                n = min(self.greedy_chunk, cap - done)
                self._greedy_steps(enc, valid, st, cap, n)
                done += n
                if bool(st.istate[3].all()):             # the one host read of the chunk
                    break
        return SimpleNamespace(tokens=st.tokens, frames=st.frames, count=st.istate[4], steps=st.istate[5])
