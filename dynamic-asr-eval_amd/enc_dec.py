"""Encoder-decoder test-time adaptation: mirror of the reference's `calc_loss_enc_dec` (lcasr/lib.py:1228-1322),
`enc_dec_inference` (:1112-1134), `generate_enc_dec` (:1172-1226), `calc_rewards` / `_policy_forward` / `update_grpo` /
`update_maxrl` (:1330-1472) and `enc_dec_dynamic_eval` (:1475-1732), same names / argument meaning / printed lines, on the HIP
kernels.  `training_mode == 'teacher_ce'` runs as is; the RL modes `grpo` / `maxrl` are OPT-IN through `rl_reward` (below).

The reference takes the model from the un-vendored `lcasr` package (`get_model_class(config)`, an SCConformerXL encoder with a
CTC head plus `language_model_decoder`; enc_dec_dynamic_eval_test.py:45-46).  Only its call surface is visible in the reference:
`model.forward(audio_signal[, text_sequence_bos, a_lengths]) -> {'final_posteriors_ctc', 'final_posteriors_lm', 'length'}`,
`model.generate(audio, encoder_states=...)["text_sequence"]`, `model.ctc_loss_weight`, `model.language_model_decoder.{pos_enc,
layers, dropout_emb, ff_out_dropout}`, `model.pos_enc`, `model.ctc_decoder.num_classes`.  The DECODER ARCHITECTURE IS DEFINED BY THIS
BUILD (parity unpinned, like the encoder's internals): token embedding + fixed sinusoidal positions, `dec_layers` pre-norm blocks of
causal self-attention / cross-attention over the encoder states / SiLU FFN, final LayerNorm, linear head over the tokenizer
vocabulary; bos = eos = 0 as in calc_loss_enc_dec's defaults (:1236-1237).  oracle/enc_dec_ref.py holds the same definition in torch.

Scope: `training_mode == 'teacher_ce'` (:1638-1658) with every flag of that path: the teacher filters incl. the sampled-decode
agreement filter (`model.generate(sample=True, temperature=...)`, :1620-1627) and the decoder dropout knobs `dropout_emb /
dropout_post_ff / dropout_attn` (:1511-1522,1636-1637,1703-1707).  Randomness is counter-based (dyn_dropout / dyn_gumbel_argmax_rows:
a draw is a pure function of (seed, stream, index)), so it is reproducible and the oracle restates it exactly.  Decoder parameters
live in the encoder's flat buffers (SCConformerXL(extra_spec=...)), so snapshot / restore / MADGRAD step are the same single
operations as on the CTC path.

RL modes (`training_mode` 'grpo' / 'maxrl', :1659-1702): run only when `args.rl_reward` is set (harness: `-kwargs
rl_reward="'wer_cer'"`); without it they raise NotImplementedError as before.  `rl_reward='wer_cer'` is the reference's
`calc_rewards` WITHOUT ITS BLEU TERM — reward = ((1 - WER) + (1 - CER)) / 2 instead of (1 - WER + 1 - CER + BLEU) / 3, because
`sacrebleu` is not vendored; a callable `(ref, hyps) -> [float]` is accepted in its place, so a site that has sacrebleu can pass the
reference's exact reward.  Per window: 4 sampled rollouts of the augmented copy in ONE batched decode (`generate_batch`:
dyn_decoder_steps_batch, row r draws with seed + r), rewards against the teacher's text, then `update_grpo` / `update_maxrl`: the
rollouts are scored teacher-forced one at a time (causal, padded at the end only: exact), the policy-gradient loss is
dyn_nll_loss_weighted with the per-rollout weight of `rl_row_weights`, and its gradient is ACCUMULATED into the flat gradient buffer
(decoder gradients summed over rollouts, one encoder backward with the summed cross-attention gradient) — there is no autograd graph,
the update functions return the loss as a float.  Rollouts come back in row order (the reference appends them in finishing order;
every consumer pairs hypotheses and rewards by index).  With decoder dropout on, every rollout's scoring pass draws its own masks.
The 'wer_cer' reward's word and character edit counts of a window come from one dyn_edit_counts call on the model's device (the
integers of the host dynamic programme, so the rewards are the same floats); `rl_reward_on_host=True` scores on the host."""
import ctypes
import math
import os
import random
from types import SimpleNamespace

import torch

from . import _attn, ops
from ._lib import DEC_PTRS_PER_LAYER, DecoderBatchDesc, DecoderDesc, check, load
from ._loop import augmented_batch, window_rule
from .augment import SpecAugment
from .decoding import GreedyCTCDecoder
from .enc_dec_teacher_filters import should_skip_faulty_teacher_prediction
from .lib import get_lr_args_from_args, get_specaugment_config_from_args, prepare_chunks
from .model import SCConformerXL
from .optim import MADGRAD
from .wer import _pair_ids, edit_counts, edit_counts_ids, rates_from_counts

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **_):
        return x

DEC = "language_model_decoder."
DEFAULT_DECODER = dict(dec_d_model=256, dec_layers=2, dec_heads=4, dec_ff_mult=4, dec_max_positions=2048, ctc_loss_weight=0.3)


def decoder_spec(dc, d_enc, vocab):
    dd, ff = dc["dec_d_model"], dc["dec_d_model"] * dc["dec_ff_mult"]
    spec = [(DEC + "embed.weight", (vocab, dd))]
    for l in range(dc["dec_layers"]):
        p = f"{DEC}layers.{l}."
        spec += [(p + "self.norm.weight", (dd,)), (p + "self.norm.bias", (dd,)), (p + "self.qkv.weight", (3 * dd, dd)),
                 (p + "self.qkv.bias", (3 * dd,)), (p + "self.out.weight", (dd, dd)), (p + "self.out.bias", (dd,)),
                 (p + "cross.norm.weight", (dd,)), (p + "cross.norm.bias", (dd,)), (p + "cross.q.weight", (dd, dd)),
                 (p + "cross.q.bias", (dd,)), (p + "cross.kv.weight", (2 * dd, d_enc)), (p + "cross.kv.bias", (2 * dd,)),
                 (p + "cross.out.weight", (dd, dd)), (p + "cross.out.bias", (dd,)),
                 (p + "ff.norm.weight", (dd,)), (p + "ff.norm.bias", (dd,)), (p + "ff.w1.weight", (ff, dd)), (p + "ff.w2.weight", (dd, ff))]
    spec += [(DEC + "norm_out.weight", (dd,)), (DEC + "norm_out.bias", (dd,)), (DEC + "head.weight", (vocab, dd)), (DEC + "head.bias", (vocab,))]
    return spec


def sinusoidal_positions(n, d):
    """Fixed positional table [n, d] (float64 -> fp32 once; shared with the oracle).  Frozen: the reference freezes
    `language_model_decoder.pos_enc` (lib.py:1505-1509,1533-1536) — here it is not a parameter at all."""
    pos = torch.arange(n, dtype=torch.float64)[:, None]
    inv = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * (-math.log(10000.0) / d))
    tab = torch.zeros(n, d, dtype=torch.float64)
    tab[:, 0::2] = torch.sin(pos * inv)
    tab[:, 1::2] = torch.cos(pos * inv)
    return tab.float()


class _NoParams:
    def parameters(self):
        return []


class _AttnFn:
    """`layer[0].fn.dropout_p` of the reference's decoder layers (lib.py:1525,1636,1706): the self-attention dropout rate."""

    def __init__(self):
        self.dropout_p = 0.0


class _DecoderKnobs:
    """What the reference touches on `model.language_model_decoder`: `.pos_enc`, `.layers[i][0].fn.dropout_p`, `.dropout_emb`,
    `.ff_out_dropout`, `.train()` / `.eval()` (dropout is applied in training mode only, as nn.Dropout)."""

    def __init__(self, n_layers):
        self.pos_enc = _NoParams()
        self.layers = [[SimpleNamespace(fn=_AttnFn())] for _ in range(n_layers)]
        self.dropout_emb = 0.0
        self.ff_out_dropout = 0.0
        self.training = False

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)


def _check_ids(ids, vocab, what):
    """Token ids are validated on the host before they reach the embedding / loss kernels (an id outside the decoder
    vocabulary, e.g. a tokenizer / vocab_size mismatch, must fail loudly instead of reading out of bounds)."""
    ids = [int(i) for i in ids]
    if ids and (min(ids) < 0 or max(ids) >= vocab):
        raise ops.DynError(f"{what}: token id outside [0, {vocab}) (min {min(ids)}, max {max(ids)}): tokenizer / vocab_size mismatch?")
    return ids


class EncDecSCConformerXL(SCConformerXL):
    """Encoder (this package's SCConformerXL, CTC head = `ctc_decoder`) + autoregressive decoder."""

    def __init__(self, config=None, vocab_size=128, device="cuda:0"):
        config = dict(config or {})
        self.dec = {k: config.pop(k, v) for k, v in DEFAULT_DECODER.items()}
        d_enc = config.get("d_model", 768)
        if self.dec["dec_d_model"] % 256 or self.dec["dec_d_model"] % self.dec["dec_heads"]:
            raise ValueError("dec_d_model must be a multiple of 256 (wave-per-row norm kernels) and of dec_heads")
        super().__init__(config, vocab_size=vocab_size, device=device, extra_spec=decoder_spec(self.dec, d_enc, vocab_size))
        self.vocab = vocab_size
        self.ctc_loss_weight = float(self.dec["ctc_loss_weight"])
        self.ctc_decoder = self.decoder                          # the reference's name for the CTC head (lib.py:1559)
        self.pos_table = sinusoidal_positions(self.dec["dec_max_positions"], self.dec["dec_d_model"]).to(self.device)
        # the attributes the reference's loop sets on `model.language_model_decoder` (lib.py:1519-1522,1636-1637,1703-1707)
        self.language_model_decoder = _DecoderKnobs(self.dec["dec_layers"])
        self.pos_enc = _NoParams()
        self._dctx = None
        # generate(): the lean one-token kernels of dyn_decoder_steps (default) or, with DYN_FUSED_DECODE=0, the tile kernels at M = 1
        hd = self.dec["dec_d_model"] // self.dec["dec_heads"]
        self.fused_decode = (os.environ.get("DYN_FUSED_DECODE", "1") != "0" and self.dec["dec_d_model"] * self.dec["dec_ff_mult"] <= 2048
                             and 4 <= hd <= 256 and hd & (hd - 1) == 0)
        self.random_seed = 0          # seed of the counter-based dropout / sampling draws (args.random_seed in the loop)
        self._draws = 0               # one stream id per random site and call: no draw is ever reused

    # ------------------------------------------------------------------ reference call surface
    def forward(self, audio_signal, text_sequence_bos=None, a_lengths=None):
        with ops.use_workspace(self._scratch()):
            enc = self._forward_eager(audio_signal)
            out = {"final_posteriors_ctc": enc["final_posteriors"], "hidden": self._hidden,
                   "length": torch.full((audio_signal.shape[0],), enc["final_posteriors"].shape[1], dtype=torch.int32, device=self.device)}
            if text_sequence_bos is not None:
                if audio_signal.shape[0] != 1 or text_sequence_bos.shape[0] != 1:
                    raise ops.DynError("enc-dec forward with text: batch size 1 only (num_negatives == 1 in the reference, lib.py:1494)")
                out["final_posteriors_lm"] = self._decoder_forward(text_sequence_bos[0].to(torch.int32), self._hidden[0])[None]
        return out

    __call__ = forward

    def generate(self, audio_signal, encoder_states=None, sample=False, temperature=1.0, max_tokens=None, seed=None, check_every=8, step0=0):
        """Autoregressive decode of ONE window -> {'text_sequence': [ids]} (reference call sites lib.py:1128,1579-1582,1620-1625):
        greedy, or with `sample=True` a draw from softmax(logits / temperature) per step (Gumbel-max on counter-based uniforms:
        dyn_gumbel_argmax_rows; `seed` defaults to a fresh stream of this model's random_seed, an explicit seed draws from stream
        `step0` + t).
        Incremental: every step runs ONE token through the decoder against per-layer caches — the self-attention keys / values of
        the prefix live in a packed [limit + 1, 3 * dd] buffer the QKV projection writes row t of, the cross-attention keys /
        values of the encoder states are projected once.  The chosen id goes straight into the device token buffer; the host
        looks for eos only every `check_every` steps (ids after the first eos are never read), so there is no per-token sync."""
        with torch.no_grad():
            enc = encoder_states if encoder_states is not None else self.forward(audio_signal)
            h = enc["hidden"][0]
            limit = max_tokens if max_tokens is not None else max(1, min(self.dec["dec_max_positions"] - 1, h.shape[0] // 2))
            limit = min(int(limit), self.dec["dec_max_positions"] - 1)       # position t reads pos_table[t]: never past the table
            dc, P = self.dec, self.P
            dd, L = dc["dec_d_model"], dc["dec_layers"]
            if sample:
                if not temperature > 0.0:
                    raise ops.DynError("generate(sample=True): temperature must be > 0")
                if seed is None:
                    seed, step0 = self.random_seed, self._next_stream()
            st = torch.cuda.current_stream().cuda_stream
            with ops.use_workspace(self._scratch()):
                kv = [ops.linear(h, P[f"{DEC}layers.{l}.cross.kv.weight"], P[f"{DEC}layers.{l}.cross.kv.bias"]) for l in range(L)]
                cache = [torch.empty(limit + 1, 3 * dd, device=self.device, dtype=torch.float32) for _ in range(L)]
                tok_dev = torch.zeros(limit + 2, dtype=torch.int32, device=self.device)           # tok_dev[0] = bos
                n_tok, t = None, 0
                fused = self._decoder_desc(kv, cache, tok_dev, h.shape[0]) if self.fused_decode else None
                while t < limit and n_tok is None:
                    n = min(check_every, limit - t)
                    if fused is not None:                                                          # one C call, 8 * layers + 2 launches per token
                        check(load().dyn_decoder_steps(ctypes.byref(fused[0]), t, n, 1 if sample else 0, 1.0 / float(temperature) if sample else 1.0,
                                                       int(seed) if sample else 0, int(step0) if sample else 0, st), "dyn_decoder_steps")
                        t += n
                    for _ in range(0 if fused is not None else n):                                 # the tile-kernel path (DYN_FUSED_DECODE=0)
                        logits = self._decoder_step(tok_dev, t, h, kv, cache)                     # [1, V]
                        nxt = tok_dev[t + 1:]
                        if sample:
                            check(load().dyn_gumbel_argmax_rows(logits.data_ptr(), 1, self.vocab, self.vocab, 1.0 / float(temperature), int(seed),
                                                                int(step0 + t), nxt.data_ptr(), st), "dyn_gumbel_argmax_rows")
                        else:
                            check(load().dyn_argmax_rows(logits.data_ptr(), 1, self.vocab, self.vocab, nxt.data_ptr(), 0, st), "dyn_argmax_rows")
                        t += 1
                    got = tok_dev[1:t + 1].tolist()                                                # one sync per `check_every` tokens
                    if 0 in got:                                                                   # eos
                        n_tok = got.index(0)
                toks = tok_dev[1:t + 1].tolist()[:n_tok] if n_tok is not None else tok_dev[1:t + 1].tolist()
        return {"text_sequence": toks}

    def generate_batch(self, audio_signal, rows, encoder_states=None, temperature=1.0, max_tokens=None, seed=None, check_every=8,
                       bos_id=0, eos_id=0, fill=None):
        """`rows` (1 .. 8) SAMPLED decodes of one window in lockstep -> {'text_sequences': [[ids] per row]}: row r is what
        `generate(sample=True, temperature=..., seed=seed + r, max_tokens=...)` returns, token for token (dyn_decoder_steps_batch:
        every weight row is read once per step for all live rows, each row's sums in the single-row kernel's order).  The
        cross-attention keys / values are projected once and shared; every row has its own self-attention cache, token buffer and
        device-side `finished` flag — a row that drew eos runs no more work and writes nothing.  The host reads the flags every
        `check_every` steps.  `fill`: value the fresh caches / scratch are filled with (tests: NaN exposes a read of a row never written).
        With `fused_decode` off the rows are decoded one after the other through the tile-kernel path of `generate`."""
        rows = int(rows)
        if not 1 <= rows <= 8:
            raise ops.DynError(f"generate_batch: {rows} rows (1 .. 8)")
        if not temperature > 0.0:
            raise ops.DynError("generate_batch: temperature must be > 0")
        with torch.no_grad():
            enc = encoder_states if encoder_states is not None else self.forward(audio_signal)
            h = enc["hidden"][0]
            limit = max_tokens if max_tokens is not None else max(1, min(self.dec["dec_max_positions"] - 1, h.shape[0] // 2))
            limit = min(int(limit), self.dec["dec_max_positions"] - 1)
            seed, step0 = (self.random_seed, self._next_stream()) if seed is None else (seed, 0)
            if not self.fused_decode or bos_id != 0 or eos_id != 0:
                if bos_id != 0 or eos_id != 0:
                    raise ops.DynError("generate_batch: bos = eos = 0 only (calc_loss_enc_dec's defaults, lib.py:1236-1237)")
                return {"text_sequences": [self.generate(audio_signal, encoder_states=enc, sample=True, temperature=temperature, max_tokens=limit,
                                                         seed=int(seed) + r, step0=step0, check_every=check_every)["text_sequence"]
                                           for r in range(rows)]}                                  # the same draws: (seed + r, step0 + t)
            dc, P = self.dec, self.P
            dd, L = dc["dec_d_model"], dc["dec_layers"]
            st = torch.cuda.current_stream().cuda_stream
            new = (lambda *shape: torch.empty(*shape, device=self.device, dtype=torch.float32)) if fill is None else \
                (lambda *shape: torch.full(shape, float(fill), device=self.device, dtype=torch.float32))
            with ops.use_workspace(self._scratch()):
                kv = [ops.linear(h, P[f"{DEC}layers.{l}.cross.kv.weight"], P[f"{DEC}layers.{l}.cross.kv.bias"]) for l in range(L)]
                cache = [new(rows, limit + 1, 3 * dd) for _ in range(L)]
                tok_dev = torch.zeros(rows, limit + 2, dtype=torch.int32, device=self.device)
                tok_dev[:, 0] = bos_id
                finished = torch.zeros(rows, dtype=torch.int32, device=self.device)
                per_row = int(load().dyn_decoder_row_scratch_floats(dd, dd * dc["dec_ff_mult"], dc["dec_heads"]))
                base, keep = self._decoder_desc(kv, cache, tok_dev, h.shape[0], logits=new(rows, self.vocab), scratch=new(rows, per_row))
                desc = DecoderBatchDesc(base=base, rows=rows, eos_id=int(eos_id), token_stride=limit + 2, cache_stride=(limit + 1) * 3 * dd,
                                        finished=finished.data_ptr())
                t = 0
                while t < limit:
                    n = min(check_every, limit - t)
                    check(load().dyn_decoder_steps_batch(ctypes.byref(desc), t, n, 1, 1.0 / float(temperature), int(seed), int(step0), st),
                          "dyn_decoder_steps_batch")
                    t += n
                    if all(finished.tolist()):                                                     # one sync per `check_every` tokens
                        break
                got = tok_dev[:, 1:t + 1].tolist()
            del keep
        return {"text_sequences": [g[:g.index(eos_id)] if eos_id in g else g for g in got]}

    def _decoder_desc(self, kv, cache, tok_dev, n_enc, logits=None, scratch=None):
        """dyn_decoder_desc of one generate() call (include/dyneval.h): returns (descriptor, objects it points into)."""
        P, dc = self.P, self.dec
        dd, L = dc["dec_d_model"], dc["dec_layers"]
        ff = dd * dc["dec_ff_mult"]
        names = ("self.norm.weight", "self.norm.bias", "self.qkv.weight", "self.qkv.bias", "self.out.weight", "self.out.bias",
                 "cross.norm.weight", "cross.norm.bias", "cross.q.weight", "cross.q.bias", "cross.out.weight", "cross.out.bias",
                 "ff.norm.weight", "ff.norm.bias", "ff.w1.weight", "ff.w2.weight")
        ptrs = (ctypes.c_void_p * (L * DEC_PTRS_PER_LAYER))()
        for l in range(L):
            for i, nm in enumerate(names):
                ptrs[l * DEC_PTRS_PER_LAYER + i] = P[f"{DEC}layers.{l}.{nm}"].data_ptr()
            ptrs[l * DEC_PTRS_PER_LAYER + 16] = cache[l].data_ptr()
            ptrs[l * DEC_PTRS_PER_LAYER + 17] = kv[l].data_ptr()
        logits = torch.empty(self.vocab, device=self.device, dtype=torch.float32) if logits is None else logits
        scratch = torch.empty(6 * dd + ff + 16 * dc["dec_heads"], device=self.device, dtype=torch.float32) if scratch is None else scratch
        d = DecoderDesc(d_model=dd, heads=dc["dec_heads"], d_ff=ff, vocab=self.vocab, layers=L, n_enc=int(n_enc),
                        max_positions=dc["dec_max_positions"], eps=float(self.config["norm_eps"]),
                        embed=P[DEC + "embed.weight"].data_ptr(), pos_table=self.pos_table.data_ptr(),
                        norm_out_w=P[DEC + "norm_out.weight"].data_ptr(), norm_out_b=P[DEC + "norm_out.bias"].data_ptr(),
                        head_w=P[DEC + "head.weight"].data_ptr(), head_b=P[DEC + "head.bias"].data_ptr(),
                        layer_ptrs=ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), tokens=tok_dev.data_ptr(), logits=logits.data_ptr(),
                        scratch=scratch.data_ptr(), scratch_floats=scratch.numel())
        return d, (ptrs, logits, scratch)

    def _next_stream(self):
        """A fresh block of 2^20 stream ids for one random site (dropout mask) or one sampled decode (one id per step)."""
        self._draws += 1
        return self._draws << 20

    def _dropout(self, x, p, stream_id, out=None):
        """y = dropout(x) with the mask of (random_seed, stream_id); the backward is the same call on the gradient."""
        out = torch.empty_like(x) if out is None else out
        check(load().dyn_dropout(x.data_ptr(), out.data_ptr(), x.numel(), float(p), int(self.random_seed), int(stream_id),
                                 torch.cuda.current_stream().cuda_stream), "dyn_dropout")
        return out

    def _decoder_step(self, tok_dev, t, h_enc, kv, cache):
        """One token (position t, id tok_dev[t]) through the decoder with cached keys / values -> logits [1, V]."""
        P, dc = self.P, self.dec
        dd, eps = dc["dec_d_model"], self.config["norm_eps"]
        Tk = h_enc.shape[0]
        st = torch.cuda.current_stream().cuda_stream
        x = torch.empty(1, dd, device=self.device, dtype=torch.float32)
        check(load().dyn_embedding_fwd(tok_dev[t:].data_ptr(), P[DEC + "embed.weight"].data_ptr(), self.pos_table[t:].data_ptr(), x.data_ptr(), 1, dd,
                                       self.vocab, 1, st), "dyn_embedding_fwd")
        for l in range(dc["dec_layers"]):
            p = f"{DEC}layers.{l}."
            c = cache[l]
            n1, _, _ = ops.layernorm(x, P[p + "self.norm.weight"], P[p + "self.norm.bias"], eps)
            row = ops.linear(n1, P[p + "self.qkv.weight"], P[p + "self.qkv.bias"], out=c[t:t + 1])          # q | k | v of position t
            o1, _ = self._attend(row, c[:, dd:], c[:, 2 * dd:], 1, t + 1, 3 * dd, 3 * dd, False, False)        # the prefix IS the causal mask
            x1 = ops.linear(o1, P[p + "self.out.weight"], P[p + "self.out.bias"], beta=1.0, residual=x)
            n2, _, _ = ops.layernorm(x1, P[p + "cross.norm.weight"], P[p + "cross.norm.bias"], eps)
            q2 = ops.linear(n2, P[p + "cross.q.weight"], P[p + "cross.q.bias"])
            o2, _ = self._attend(q2, kv[l], kv[l][:, dd:], 1, Tk, dd, 2 * dd, False, False)
            x2 = ops.linear(o2, P[p + "cross.out.weight"], P[p + "cross.out.bias"], beta=1.0, residual=x1)
            n3, _, _ = ops.layernorm(x2, P[p + "ff.norm.weight"], P[p + "ff.norm.bias"], eps)
            a = ops.silu(ops.linear(n3, P[p + "ff.w1.weight"]))
            x = ops.linear(a, P[p + "ff.w2.weight"], beta=1.0, residual=x2)
        nf, _, _ = ops.layernorm(x, P[DEC + "norm_out.weight"], P[DEC + "norm_out.bias"], eps)
        return ops.linear(nf, P[DEC + "head.weight"], P[DEC + "head.bias"])

    # ------------------------------------------------------------------ decoder forward / backward (B = 1)
    def _attend(self, q, k, v, S, Tk, ldq, ldk, causal, save, drop=None):
        """softmax(q k^T / sqrt(hd)) v per head (the products: _attn.py); q rows have leading dimension ldq, k / v rows ldk (views into packed
        projections).
        `drop` = (p, stream id): dropout on the probabilities (training mode); returns (O, P[, dropped P])."""
        Hh, dd = self.dec["dec_heads"], self.dec["dec_d_model"]
        hd = dd // Hh
        Pm = torch.empty(Hh, S, Tk, device=self.device, dtype=torch.float32)
        _attn.scores(_attn.plain(q, hd, ldq), _attn.plain(k, hd, ldk), Pm, 1.0 / math.sqrt(hd))
        if causal:
            check(load().dyn_causal_mask(Pm.data_ptr(), Hh, S, torch.cuda.current_stream().cuda_stream), "dyn_causal_mask")
        ops.softmax(Pm, out=Pm)
        Pd = self._dropout(Pm, drop[0], drop[1]) if drop is not None else Pm
        O = torch.empty(S, dd, device=self.device, dtype=torch.float32)
        _attn.context(Pd, _attn.plain(v, hd, ldk), _attn.plain(O, hd))
        if drop is not None:
            return O, ((Pm, Pd) if save else None)
        return O, (Pm if save else None)

    def _attend_bwd(self, dO, Pm, q, k, v, dq, dk, dv, S, Tk, ldq, ldk, drop=None):
        """Gradients of _attend into the (strided) dq / dk / dv views of the packed projection gradients; each view is written
        exactly once (beta = 0).  With dropout `Pm` = (probabilities, dropped probabilities) and `drop` = (p, stream id)."""
        Hh, dd = self.dec["dec_heads"], self.dec["dec_d_model"]
        hd = dd // Hh
        Pm, Pd = Pm if drop is not None else (Pm, Pm)
        dP = torch.empty_like(Pm)
        _attn.grad_v_dP(Pd, _attn.plain(dO, hd), _attn.plain(v, hd, ldk), _attn.plain(dv, hd, ldk), dP)
        if drop is not None:
            self._dropout(dP, drop[0], drop[1], out=dP)            # same mask, same 1 / (1 - p)
        ops.softmax_bwd(Pm, dP, out=dP, scale=1.0)
        _attn.grad_qk(dP, _attn.plain(q, hd, ldq), _attn.plain(k, hd, ldk), _attn.plain(dq, hd, ldq), _attn.plain(dk, hd, ldk), 1.0 / math.sqrt(hd))

    def _decoder_forward(self, tokens, h_enc, cached_kv=None):
        """tokens int32 [S] (bos first), h_enc [T', d_enc] -> logits [S, V].  Saves activations in grad mode."""
        P, dc = self.P, self.dec
        dd, eps = dc["dec_d_model"], self.config["norm_eps"]
        S, Tk = tokens.shape[0], h_enc.shape[0]
        if S > dc["dec_max_positions"]:
            raise ops.DynError(f"decoder sequence of {S} tokens exceeds dec_max_positions {dc['dec_max_positions']}")
        save = torch.is_grad_enabled() and cached_kv is None
        st = torch.cuda.current_stream().cuda_stream
        x = torch.empty(S, dd, device=self.device, dtype=torch.float32)
        check(load().dyn_embedding_fwd(tokens.data_ptr(), P[DEC + "embed.weight"].data_ptr(), self.pos_table.data_ptr(), x.data_ptr(), S, dd,
                                       self.vocab, self.pos_table.shape[0], st), "dyn_embedding_fwd")
        ctx = {"tokens": tokens, "h_enc": h_enc, "layers": []} if save else None
        # dropout: only in the decoder's training mode (the reference brackets the supervised step with .train() / .eval(),
        # lib.py:1637,1703) and only for a forward that will be differentiated
        knobs = self.language_model_decoder
        train = save and knobs.training
        p_emb = float(knobs.dropout_emb) if train else 0.0
        p_ff = float(knobs.ff_out_dropout) if train else 0.0
        d_emb = (p_emb, self._next_stream()) if p_emb > 0.0 else None
        if d_emb is not None:
            self._dropout(x, *d_emb, out=x)
        if save:
            ctx["d_emb"] = d_emb
        for l in range(dc["dec_layers"]):
            p = f"{DEC}layers.{l}."
            lc = {}
            p_attn = float(knobs.layers[l][0].fn.dropout_p) if train else 0.0
            d_attn = (p_attn, self._next_stream()) if p_attn > 0.0 else None
            d_ff = (p_ff, self._next_stream()) if p_ff > 0.0 else None
            n1, m1, r1 = ops.layernorm(x, P[p + "self.norm.weight"], P[p + "self.norm.bias"], eps)
            qkv = ops.linear(n1, P[p + "self.qkv.weight"], P[p + "self.qkv.bias"])
            o1, P1 = self._attend(qkv, qkv[:, dd:], qkv[:, 2 * dd:], S, S, 3 * dd, 3 * dd, True, save, drop=d_attn)
            x1 = ops.linear(o1, P[p + "self.out.weight"], P[p + "self.out.bias"], beta=1.0, residual=x)
            n2, m2, r2 = ops.layernorm(x1, P[p + "cross.norm.weight"], P[p + "cross.norm.bias"], eps)
            q2 = ops.linear(n2, P[p + "cross.q.weight"], P[p + "cross.q.bias"])
            kv = cached_kv[l] if cached_kv is not None else ops.linear(h_enc, P[p + "cross.kv.weight"], P[p + "cross.kv.bias"])
            o2, P2 = self._attend(q2, kv, kv[:, dd:], S, Tk, dd, 2 * dd, False, save)
            x2 = ops.linear(o2, P[p + "cross.out.weight"], P[p + "cross.out.bias"], beta=1.0, residual=x1)
            n3, m3, r3 = ops.layernorm(x2, P[p + "ff.norm.weight"], P[p + "ff.norm.bias"], eps)
            u = ops.linear(n3, P[p + "ff.w1.weight"])
            a = ops.silu(u)
            if d_ff is None:
                x3 = ops.linear(a, P[p + "ff.w2.weight"], beta=1.0, residual=x2)
            else:                                   # x3 = x2 + dropout(a W2^T)
                x3 = self._dropout(ops.linear(a, P[p + "ff.w2.weight"]), *d_ff)
                ops.axpby(x2, x3, a=1.0, b=1.0)
            if save:
                lc = dict(x=x, n1=n1, m1=m1, r1=r1, qkv=qkv, P1=P1, o1=o1, x1=x1, n2=n2, m2=m2, r2=r2, q2=q2, kv=kv, P2=P2, o2=o2, x2=x2,
                          n3=n3, m3=m3, r3=r3, u=u, a=a, d_attn=d_attn, d_ff=d_ff)
                ctx["layers"].append(lc)
            x = x3
        nf, mf, rf = ops.layernorm(x, P[DEC + "norm_out.weight"], P[DEC + "norm_out.bias"], eps)
        logits = ops.linear(nf, P[DEC + "head.weight"], P[DEC + "head.bias"])
        if save:
            ctx["final"] = (x, nf, mf, rf)
            self._dctx = ctx
        return logits

    def _wb(self, dy, x, name, bias=True):
        """weight (+ bias) gradient of y = x W^T + b, accumulated into the flat gradient buffer."""
        if self.trainable(name + ".weight"):
            ops.linear_wgrad(dy, x, self.G[name + ".weight"], beta=1.0)
        if bias and self.trainable(name + ".bias"):
            ops.colsum(dy, self.G[name + ".bias"], beta=1.0)

    def _decoder_backward(self, dlogits):
        """dL/dlogits [S, V] -> accumulates every decoder parameter gradient; returns dL/dh_enc [T', d_enc]."""
        P, G, dc, ctx = self.P, self.G, self.dec, self._dctx
        dd = dc["dec_d_model"]
        tokens, h_enc = ctx["tokens"], ctx["h_enc"]
        S, Tk = tokens.shape[0], h_enc.shape[0]
        x, nf, mf, rf = ctx["final"]
        self._wb(dlogits, nf, DEC + "head")
        dn = ops.linear_dgrad(dlogits, P[DEC + "head.weight"])
        dx = torch.empty_like(x)
        ops.layernorm_bwd(x, P[DEC + "norm_out.weight"], mf, rf, dn, dx, G[DEC + "norm_out.weight"], G[DEC + "norm_out.bias"], dx_beta=0.0)
        dh_enc = torch.zeros_like(h_enc)
        for l in reversed(range(dc["dec_layers"])):
            p = f"{DEC}layers.{l}."
            c = ctx["layers"][l]
            # FFN
            df = dx if c["d_ff"] is None else self._dropout(dx, *c["d_ff"])          # gradient of the (dropped) FFN branch; dx stays the residual's
            if self.trainable(p + "ff.w2.weight"):
                ops.linear_wgrad(df, c["a"], G[p + "ff.w2.weight"], beta=1.0)
            du = ops.silu_bwd(c["u"], ops.linear_dgrad(df, P[p + "ff.w2.weight"]))
            if self.trainable(p + "ff.w1.weight"):
                ops.linear_wgrad(du, c["n3"], G[p + "ff.w1.weight"], beta=1.0)
            dn3 = ops.linear_dgrad(du, P[p + "ff.w1.weight"])
            ops.layernorm_bwd(c["x2"], P[p + "ff.norm.weight"], c["m3"], c["r3"], dn3, dx, G[p + "ff.norm.weight"], G[p + "ff.norm.bias"], dx_beta=1.0)
            # cross-attention
            self._wb(dx, c["o2"], p + "cross.out")
            do2 = ops.linear_dgrad(dx, P[p + "cross.out.weight"])
            dq2 = torch.empty_like(c["q2"])
            dkv = torch.empty_like(c["kv"])
            self._attend_bwd(do2, c["P2"], c["q2"], c["kv"], c["kv"][:, dd:], dq2, dkv, dkv[:, dd:], S, Tk, dd, 2 * dd)
            self._wb(dkv, h_enc, p + "cross.kv")
            ops.linear_dgrad(dkv, P[p + "cross.kv.weight"], out=dh_enc, beta=1.0)
            self._wb(dq2, c["n2"], p + "cross.q")
            dn2 = ops.linear_dgrad(dq2, P[p + "cross.q.weight"])
            ops.layernorm_bwd(c["x1"], P[p + "cross.norm.weight"], c["m2"], c["r2"], dn2, dx, G[p + "cross.norm.weight"], G[p + "cross.norm.bias"],
                              dx_beta=1.0)
            # causal self-attention
            self._wb(dx, c["o1"], p + "self.out")
            do1 = ops.linear_dgrad(dx, P[p + "self.out.weight"])
            dqkv = torch.empty_like(c["qkv"])
            qkv = c["qkv"]
            self._attend_bwd(do1, c["P1"], qkv, qkv[:, dd:], qkv[:, 2 * dd:], dqkv, dqkv[:, dd:], dqkv[:, 2 * dd:], S, S, 3 * dd, 3 * dd,
                             drop=c["d_attn"])
            self._wb(dqkv, c["n1"], p + "self.qkv")
            dn1 = ops.linear_dgrad(dqkv, P[p + "self.qkv.weight"])
            ops.layernorm_bwd(c["x"], P[p + "self.norm.weight"], c["m1"], c["r1"], dn1, dx, G[p + "self.norm.weight"], G[p + "self.norm.bias"],
                              dx_beta=1.0)
        if ctx["d_emb"] is not None:
            self._dropout(dx, *ctx["d_emb"], out=dx)
        if self.trainable(DEC + "embed.weight"):
            check(load().dyn_embedding_bwd(tokens.data_ptr(), dx.data_ptr(), G[DEC + "embed.weight"].data_ptr(), S, dd, self.vocab, 1.0,
                                           torch.cuda.current_stream().cuda_stream), "dyn_embedding_bwd")
        self._dctx = None
        return dh_enc


# ------------------------------------------------------------------------------------------------ the reference's functions
def calc_loss_enc_dec(model, audio_signal, text_sequence, a_lengths, t_lengths, tokenizer, token_swap_prob=0.0, bos_id=0, eos_id=0,
                      label_smoothing=0.0, backward=True):
    """reference lcasr/lib.py:1228-1322 for one sample (num_negatives == 1): bos-prefixed inputs, targets shifted left with
    eos (= 0) in the last place (:1240-1244,1277), `model.forward(audio, text_bos, a_lengths)` (:1255), CTC term
    F.ctc_loss(sum, blank = C - 1) / (N * B) * 100 (:1258-1272), LM term F.cross_entropy(sum) / (B * S) (:1290-1299), mixed with
    `model.ctc_loss_weight` (:1303).  With `backward` the gradients of that loss are accumulated into the model's flat gradient
    buffer (decoder backward -> encoder backward with the cross-attention's gradient on the encoder states): the reference's
    `loss.backward()` at :1657.  Returns the same dict (loss as a python float, no autograd graph exists here)."""
    if token_swap_prob > 0.0 or label_smoothing > 0.0:
        raise NotImplementedError("token_swap_prob / label_smoothing: defaults only (the teacher_ce path passes neither, lib.py:1645-1652)")
    dev = model.device
    text = text_sequence.to(dev)
    assert text.shape[0] == 1 and audio_signal.shape[0] == 1, "calc_loss_enc_dec: batch of 1 (num_negatives == 1)"
    S = int(t_lengths[0])
    _check_ids(text_sequence[0, :S].tolist(), model.vocab, "calc_loss_enc_dec: text_sequence")
    text_bos = torch.zeros(1, S + 1, dtype=torch.int32, device=dev)
    text_bos[:, 0] = bos_id
    text_bos[:, 1:] = text[:, :S].to(torch.int32)
    targets = torch.zeros(1, S + 1, dtype=torch.int32, device=dev)
    targets[:, :-1] = text_bos[:, 1:]
    targets[:, -1] = eos_id                                      # equal lengths in the batch: `targets[:, -1] = 0` (:1277)
    with torch.enable_grad():
        out = model.forward(audio_signal, text_bos, a_lengths)
    ctc_out, lm_out = out["final_posteriors_ctc"], out["final_posteriors_lm"]
    N, B = ctc_out.shape[1], ctc_out.shape[0]
    w = float(model.ctc_loss_weight)
    st = torch.cuda.current_stream().cuda_stream
    g_ctc, ctc_show, ctc_bwd = None, 0.0, 0.0
    if w > 0.0:
        ilen = torch.full((B,), N, dtype=torch.int32, device=dev)
        tlen = torch.full((B,), S, dtype=torch.int32, device=dev)
        tg = text[:, :max(S, 1)].to(torch.int32).contiguous() if S else torch.zeros(1, 1, dtype=torch.int32, device=dev)
        loss_ctc, _, g_ctc = ops.ctc_loss(ctc_out.contiguous(), tg, ilen, tlen, ctc_out.shape[-1] - 1, reduction="sum",
                                          grad_scale=w * 100.0 / (N * B), want_grad=backward)
        lc = float(loss_ctc.item())
        ctc_show, ctc_bwd = lc / float(a_lengths.sum()) * 100, lc / (N * B) * 100
    rows, V = S + 1, lm_out.shape[-1]
    logp = ops.log_softmax(lm_out[0].contiguous())
    loss_lm = torch.empty(1, device=dev, dtype=torch.float32)
    row_loss = torch.empty(rows, device=dev, dtype=torch.float32)
    g_lm = torch.empty(rows, V, device=dev, dtype=torch.float32) if backward else None
    check(load().dyn_nll_loss(logp.data_ptr(), targets.data_ptr(), loss_lm.data_ptr(), row_loss.data_ptr(), 0 if g_lm is None else g_lm.data_ptr(),
                              rows, V, -100, (1.0 - w) / (1 * rows), st), "dyn_nll_loss")
    ll = float(loss_lm.item())
    lm_show, lm_bwd = ll / max(1, S), ll / (1 * rows)
    if backward:
        with ops.use_workspace(model._scratch()):
            dh = model._decoder_backward(g_lm)
        gp = g_ctc if g_ctc is not None else torch.zeros_like(ctc_out)
        model.backward(gp, grad_hidden=dh[None])
    return {"loss": ctc_bwd * w + lm_bwd * (1 - w),
            "display_losses": {"loss": ctc_show * w + lm_show * (1 - w), "ctc_loss": ctc_show, "lm_loss": lm_show},
            "ctc_posteriors": ctc_out, "lm_posteriors": lm_out, "length": out["length"]}


def generate_enc_dec(model, audio_signal, max_generate=256, bos_id=0, eos_id=0, sample=1, greedy=True, temperature=1.0, seed=None):
    """reference lcasr/lib.py:1172-1226.  `sample=1, greedy=True` (call site :1128, `generate_enc_dec(model, audio_chunk)[0]`):
    [token ids of the greedy decode].  Any other combination is the sampled form (the RL rollouts, :1665-1671): `sample` rows drawn
    in one batched decode -> (text_sequence [R, Lmax] long, padded with 0, bos removed; encoder_out; text_lengths [R]) as :1220-1226.
    Kept from the reference: the softmax input is `logits * temperature` (:1200 multiplies; the one call site passes 1.0); a row
    retires when its draw is `eos_id` or when its length including bos exceeds `max_generate` — the draw made at retirement is
    discarded, so a row holds at most `max_generate` tokens; the decoder's `dec_max_positions` caps a row as well.  Different: rows
    come back in ROW order (the reference appends in finishing order).  `seed`: row r draws with seed + r (default: a fresh stream
    block of `model.random_seed`)."""
    if sample == 1 and greedy:
        return [torch.tensor(model.generate(audio_signal)["text_sequence"], dtype=torch.long)]
    if not temperature > 0.0:
        raise ValueError("generate_enc_dec: temperature must be > 0")
    with torch.no_grad():
        encoder_out = model.forward(audio_signal=audio_signal)
    limit = max(1, min(int(max_generate), model.dec["dec_max_positions"] - 1))
    seqs = model.generate_batch(audio_signal, sample, encoder_states=encoder_out, temperature=1.0 / float(temperature), max_tokens=limit,
                                seed=seed, bos_id=bos_id, eos_id=eos_id)["text_sequences"]
    text_lengths = torch.LongTensor([len(q) for q in seqs])
    text_sequence = torch.zeros(len(seqs), max(len(q) for q in seqs), dtype=torch.long)
    for r, q in enumerate(seqs):
        text_sequence[r, :len(q)] = torch.tensor(q, dtype=torch.long)
    return text_sequence.to(model.device), encoder_out, text_lengths


WER_CER_NOTE = ("rl_reward='wer_cer': reward = ((1 - WER) + (1 - CER)) / 2 - the reference's BLEU term (sacrebleu.corpus_bleu, lib.py:1350) is "
                "dropped: sacrebleu is not available; pass a callable (ref, hyps) -> [float] as rl_reward for another reward")


def calc_rewards(ref, hyps, device=None):
    """reference lcasr/lib.py:1330-1359 WITHOUT THE BLEU TERM (`rl_reward='wer_cer'`): per hypothesis ((1 - WER) + (1 - CER)) / 2
    where the reference averages 1 - WER, 1 - CER and sacrebleu.corpus_bleu / 100 (sacrebleu is not vendored).  The two empty-string
    branches (:1341-1346) are kept as written: both empty -> 1.0, empty reference and a non-empty hypothesis -> -(number of words).
    With a GPU `device` the word and character counts of all remaining hypotheses come from ONE dyn_edit_counts call; the counts are
    the host path's integers and the reward is formed by the same expression, so the floats are identical."""
    rewards = [None] * len(hyps)
    scored = []
    for k, hyp in enumerate(hyps):
        if len(hyp.strip()) == 0 and len(ref.strip()) == 0:
            rewards[k] = 1.0
        elif len(ref.strip()) == 0 and len(hyp.strip()) > 0:
            rewards[k] = len(hyp.strip().split()) * -1.0
        else:
            scored.append(k)
    if device is None:
        counts = [(edit_counts([hyps[k]], [ref]), edit_counts([hyps[k]], [ref], use_cer=True)) for k in scored]
    else:
        ids = [_pair_ids(hyps[k], ref, use_cer) for k in scored for use_cer in (False, True)]
        rows = edit_counts_ids([h for h, _ in ids], [r for _, r in ids], device)
        counts = [(tuple(int(x) for x in rows[2 * q]), tuple(int(x) for x in rows[2 * q + 1])) for q in range(len(scored))]
    for k, (words, chars) in zip(scored, counts):
        wer = rates_from_counts(*words)[0] * -1.0 + 1
        cer = rates_from_counts(*chars)[0] * -1.0 + 1
        rewards[k] = (wer + cer) / 2.0
    print(sum(rewards) / len(rewards), "avg reward")
    return rewards


def _reward_fn(rl_reward, device=None):
    if rl_reward == 'wer_cer':
        return calc_rewards if device is None else (lambda ref, hyps: calc_rewards(ref, hyps, device=device))
    if callable(rl_reward):
        return lambda ref, hyps: [float(r) for r in rl_reward(ref, hyps)]
    raise ValueError(f"rl_reward {rl_reward!r}: 'wer_cer' or a callable (ref: str, hyps: list[str]) -> list[float]")


def rl_row_weights(mode, rewards, lengths, normalize_std=True, std_epsilon=1e-7, success_threshold=0.9, epsilon=1e-6):
    """Per-rollout weight w_j of the policy-gradient loss `sum_j w_j * sum_t (-log p(y_jt))` over the n_j = lengths[j] + 1 scored
    tokens (hypothesis + eos) of rollout j — the reference's losses with their advantages folded in, in its float32 arithmetic:
      'grpo'  (lib.py:1411-1420): A = r - mean(r) [/ (std(r, unbiased=False) + std_epsilon)];  w_j = A_j / (n_j * R)
      'maxrl' (:1450-1470): r binarised at success_threshold, pass rate m; None when m <= 0 or m >= 1 (the skip cases);
                            A = (r - m) / (m + epsilon);  w_j = A_j / sum_j n_j
    Returns (weights [R] float32 tensor, advantage [R]) or None."""
    counts = torch.as_tensor([int(n) + 1 for n in lengths], dtype=torch.float32)
    R = len(rewards)
    assert R == counts.shape[0] and R > 0
    if mode == 'grpo':
        r = torch.as_tensor(rewards, dtype=torch.float32)
        advantage = r - r.mean()
        if normalize_std:
            advantage = advantage / (r.std(unbiased=False) + std_epsilon)
        return advantage / R / counts, advantage
    if mode == 'maxrl':
        r = torch.as_tensor([1.0 if x >= success_threshold else 0.0 for x in rewards], dtype=torch.float32)
        mean = r.mean()
        if mean.item() <= 0 or mean.item() >= 1:
            return None
        advantage = (r - mean) / (mean + epsilon)
        return advantage / counts.sum(), advantage
    raise ValueError(f"rl_row_weights: mode {mode!r}")


def policy_forward(model, audio_signal, tokenizer, hyps, weights=None):
    """reference lcasr/lib.py:1361-1397 (`_policy_forward`): teacher-forced log-probabilities of the rollouts' own tokens ->
    (log_probs [R, Lmax] float32, mask [R, Lmax] bool) on the host, row j valid for len(encode(hyps[j])) + 1 positions (tokens, then
    eos).  The rollouts are causal and padded at the end only, so each runs through the B = 1 decoder at its own length: exact.
    With `weights` [R] it is also the backward of loss = sum_j weights[j] * sum_t (-log_probs[j, t]): one encoder forward in grad
    mode, per rollout decoder forward / dyn_nll_loss_weighted / decoder backward (parameter gradients ACCUMULATE in the flat
    buffer), then one encoder backward with the cross-attention gradients on the encoder states summed over rollouts (the CTC
    head receives a zero gradient).  Returns (log_probs, mask, loss as a python float) then."""
    assert audio_signal.shape[0] == 1, 'Must be bsz of 1 for audio signal'
    dev = model.device
    ids = [_check_ids(tokenizer.encode(t), model.vocab, "policy_forward: hypothesis") for t in hyps]
    R, Lmax = len(ids), max(len(q) for q in ids) + 1
    grad = weights is not None
    st = torch.cuda.current_stream().cuda_stream
    with (torch.enable_grad() if grad else torch.no_grad()):
        enc = model.forward(audio_signal)
        h = enc["hidden"][0]
        log_probs = torch.zeros(R, Lmax, dtype=torch.float32, device=dev)
        mask = torch.zeros(R, Lmax, dtype=torch.bool)
        losses = torch.zeros(R, dtype=torch.float32, device=dev)
        dh = None
        with ops.use_workspace(model._scratch()):
            for j, seq in enumerate(ids):
                S = len(seq) + 1
                tokens = torch.tensor([0] + seq, dtype=torch.int32, device=dev)                      # bos first
                targets = torch.tensor(seq + [0], dtype=torch.int32, device=dev)                     # eos last
                logp = ops.log_softmax(model._decoder_forward(tokens, h))
                log_probs[j, :S] = logp.gather(1, targets.long()[:, None])[:, 0]
                mask[j, :S] = True
                if grad:
                    w = torch.full((S,), float(weights[j]), dtype=torch.float32, device=dev)
                    g, row = torch.empty_like(logp), torch.empty(S, dtype=torch.float32, device=dev)
                    check(load().dyn_nll_loss_weighted(logp.data_ptr(), targets.data_ptr(), w.data_ptr(), losses[j:].data_ptr(), row.data_ptr(),
                                                       g.data_ptr(), S, model.vocab, st), "dyn_nll_loss_weighted")
                    d = model._decoder_backward(g)
                    dh = d if dh is None else ops.axpby(d, dh)
    if not grad:
        return log_probs.cpu(), mask
    model.backward(torch.zeros_like(enc["final_posteriors_ctc"]), grad_hidden=dh[None])
    return log_probs.cpu(), mask, float(sum(losses.tolist()))


def update_grpo(model, audio_signal, tokenizer, hyps, rewards, normalize_std=True, std_epsilon=1e-7):
    """reference lcasr/lib.py:1400-1422: loss = -mean_j(A_j * mean_t log p(y_jt)).  Returns the loss as a python float and accumulates
    its gradient into the model's flat gradient buffer (the reference returns a tensor and the loop calls .backward())."""
    lengths = [len(tokenizer.encode(t)) for t in hyps]
    weights, advantage = rl_row_weights('grpo', rewards, lengths, normalize_std=normalize_std, std_epsilon=std_epsilon)
    print(advantage)
    _, _, loss = policy_forward(model, audio_signal, tokenizer, hyps, weights=weights.tolist())
    print(loss, "loss")
    return loss


def update_maxrl(model, audio_signal, tokenizer, hyps, rewards, success_threshold=0.9, epsilon=1e-6):
    """reference lcasr/lib.py:1425-1472 (Maximum Likelihood RL, on-policy): rewards binarised at `success_threshold`, advantage
    (r - pass rate) / (pass rate + epsilon), loss = sum of -log p * A over the valid tokens / their number.  None (and no gradient)
    when the pass rate is 0 or 1.  Otherwise the loss as a python float, its gradient accumulated as update_grpo does."""
    lengths = [len(tokenizer.encode(t)) for t in hyps]
    out = rl_row_weights('maxrl', rewards, lengths, success_threshold=success_threshold, epsilon=epsilon)
    if out is None:
        if not any(r >= success_threshold for r in rewards):
            print(f'maxrl: pass rate=0 (no rollout >= {success_threshold}), skipping task')
        else:
            print(f'maxrl: pass rate=1 (all rollouts >= {success_threshold}), skipping task (zero advantage)')
        return None
    weights, advantage = out
    mean = sum(1.0 for r in rewards if r >= success_threshold) / len(rewards)
    print(f'maxrl: pass rate={mean:.3f}, advantages={advantage.tolist()}')
    _, _, loss = policy_forward(model, audio_signal, tokenizer, hyps, weights=weights.tolist())
    print(loss, "loss (maxrl)")
    return loss


def enc_dec_inference(model, spec, seq_len, overlap, tokenizer, use_tqdm=True):
    """reference lcasr/lib.py:1112-1134: windows without overlap, greedy generate per window, texts joined by one space."""
    assert overlap == 0, 'Overlap not implemented for encoder-decoder model (yet)'
    spec = spec.to(device=model.device, dtype=torch.float32)
    training_data, training_keys = prepare_chunks(spec, seq_len, overlap)
    output_sequences = [None] * len(training_keys)
    idxs = list(range(len(training_keys)))
    for idx in (tqdm(idxs) if use_tqdm else idxs):
        audio_chunk = training_data[training_keys[idx]].contiguous()
        with torch.no_grad():
            output = generate_enc_dec(model, audio_chunk)[0]
        text = tokenizer.decode(output.tolist()).strip()
        print(f'Generated text: {text}')
        output_sequences[idx] = text
    return " ".join(output_sequences).replace('  ', ' ').strip()


def enc_dec_dynamic_eval(args, model, spec, seq_len, overlap, tokenizer, use_tqdm=True, optim=MADGRAD, optimizer_state=None,
                         return_params=False, **kwargs):
    """reference lcasr/lib.py:1475-1732: per window — augmented + clean copy (:1574-1576), teacher = greedy decode of the clean copy
    from one no-grad encoder pass (:1580-1588), the teacher filters (:1596-1633), then the update.  `training_mode == 'teacher_ce'`:
    one supervised step on the augmented copy with the teacher's tokens as target: calc_loss_enc_dec -> zero_grad / backward / step
    (:1638-1658).  `training_mode` 'grpo' / 'maxrl' WITH `args.rl_reward` set ('wer_cer' = the reference's reward without its BLEU
    term, or a callable (ref, hyps) -> [float]), :1659-1702: ctc_loss_weight zeroed for the step, 4 sampled rollouts of the augmented
    copy at temperature 1.0, rewards against the teacher's text, no update when the mean reward exceeds 0.95, `skipping` when all
    rewards are zero or equal, else update_maxrl (`args.maxrl_success_threshold`) / update_grpo (`args.grpo_normalize_std`) ->
    zero_grad / step.  Without `rl_reward` those modes raise NotImplementedError.  Afterwards the whole recording is decoded with
    the adapted weights (:1714-1722) and the weights restored (:1728-1729)."""
    mode = getattr(args, 'training_mode', 'grpo')
    rl_reward = args.__dict__.get('rl_reward')
    if mode != 'teacher_ce' and (rl_reward is None or mode not in ('grpo', 'maxrl')):
        raise NotImplementedError(f"training_mode {mode!r}: only 'teacher_ce' is implemented (the RL modes grpo / maxrl are out of scope)")
    reward_fn = None
    if mode != 'teacher_ce':
        # 'wer_cer' is scored on the model's device (dyn_edit_counts); `rl_reward_on_host=True` keeps the host dynamic programme
        reward_fn = _reward_fn(rl_reward)                 # an unknown name is refused here, before the model is touched
        if rl_reward == 'wer_cer' and not args.__dict__.get('rl_reward_on_host', False):
            reward_fn = _reward_fn(rl_reward, model.device)
        print(WER_CER_NOTE if rl_reward == 'wer_cer' else f'rl_reward: {getattr(rl_reward, "__name__", rl_reward)!r} (caller-supplied reward)')
    dropout_emb = args.__dict__.get('dropout_emb', 0.0)
    dropout_post_ff = args.__dict__.get('dropout_post_ff', 0.0)
    dropout_attn = args.__dict__.get('dropout_attn', 0.0)
    for k, v in (('dropout_emb', dropout_emb), ('dropout_post_ff', dropout_post_ff), ('dropout_attn', dropout_attn)):
        if not 0.0 <= float(v) < 1.0:
            raise ValueError(f"{k} must be in [0, 1), got {v}")
    # the reference's knobs on the decoder (lib.py:1519-1525): embedding / post-FFN dropout for the whole call, attention dropout
    # only around the supervised step; draws are counter-based and restart with every call (reproducible: `random_seed`)
    model.language_model_decoder.dropout_emb = dropout_emb
    model.language_model_decoder.ff_out_dropout = dropout_post_ff
    for layer in model.language_model_decoder.layers:
        layer[0].fn.dropout_p = 0
    model.random_seed, model._draws = int(args.__dict__.get('random_seed', 0)), 0
    spec_augment_config = get_specaugment_config_from_args(args)
    print(spec_augment_config)
    lr_args = get_lr_args_from_args(args)
    print(lr_args)
    num_negatives = 1
    device = model.device
    spec = spec.to(device=device, dtype=torch.float32)
    spec_n = spec.shape[-1]
    original_flat = model.flat_params.clone()
    optimizer = optim(model.parameters(), **lr_args)
    if optimizer_state is not None:
        optimizer.load_state_dict(optimizer_state)
    augmentation = SpecAugment(**spec_augment_config)
    fixed_masks = args.__dict__.get('spec_augment_fixed_masks', None)
    seq_len, overlap = window_rule(args, spec_n, seq_len, overlap, args.config['model']['subsampling_factor'])
    assert overlap == 0, 'Overlap > 0 not implemented for encoder-decoder model'
    print(f'Using seq_len: {seq_len}')
    ctc_decoder = None
    if args.__dict__.get('teacher_filter_ctc_agreement', False):
        ctc_decoder = GreedyCTCDecoder(tokenizer=tokenizer, blank_id=model.ctc_decoder.num_classes - 1, device=device)
    model.eval()
    training_data, training_keys = prepare_chunks(spec, seq_len, overlap)
    for epoch in range(args.__dict__.get('epochs', 1)):
        print(f'Epoch {epoch + 1} / {args.__dict__.get("epochs", 1)}')
        idxs = list(range(len(training_keys)))
        idxs = random.sample(idxs, len(idxs)) if args.__dict__.get('shuffle', False) else idxs
        for idx in (tqdm(idxs) if use_tqdm else idxs):
            view = training_data[training_keys[idx]][0]                                    # [F, T]
            Fq, u_len = view.shape
            audio_chunk = augmented_batch(
                [view], lambda k: fixed_masks[training_keys[idx]] if fixed_masks is not None else augmentation.draw(Fq, u_len), augmentation)
            with torch.no_grad():
                encoder_out_for_teacher = model.forward(audio_signal=audio_chunk[-1:].contiguous())
            teacher_pred_tokens = _check_ids(model.generate(audio_chunk[-1:], encoder_states=encoder_out_for_teacher)["text_sequence"],
                                             model.vocab, "teacher prediction")
            teacher_pred = torch.tensor(teacher_pred_tokens, dtype=torch.long, device=device)
            teacher_pred_text = tokenizer.decode(teacher_pred_tokens).strip()
            text_lengths = torch.LongTensor([teacher_pred.shape[-1]])
            acoustic_length = torch.LongTensor([audio_chunk.shape[-1]])
            teacher_mean_max_prob, teacher_mean_entropy, ctc_text, agreement_text = None, None, None, None
            if args.__dict__.get('teacher_filter_low_confidence', False) or args.__dict__.get('teacher_filter_ctc_agreement', False):
                teacher_inputs = torch.zeros(1, teacher_pred.shape[-1] + 1, dtype=torch.int32, device=device)
                teacher_inputs[:, 1:] = teacher_pred.to(torch.int32)
                with torch.no_grad():
                    tf = model.forward(audio_chunk[-1:].contiguous(), teacher_inputs, acoustic_length)
                if args.__dict__.get('teacher_filter_low_confidence', False) and teacher_pred.shape[-1] > 0:
                    lp = ops.log_softmax(tf['final_posteriors_lm'][0, :teacher_pred.shape[-1]].contiguous())
                    _, ent = ops.entropy_grad(lp, 1.0)
                    ids_max, vmax = ops.argmax_rows(lp)
                    teacher_mean_max_prob = float(vmax.exp().mean().item())
                    teacher_mean_entropy = float(ent.mean().item())
                if args.__dict__.get('teacher_filter_ctc_agreement', False) and ctc_decoder is not None:
                    ctc_text = ctc_decoder(tf['final_posteriors_ctc'][0]).strip()
            if args.__dict__.get('teacher_filter_decode_agreement', False):             # lib.py:1620-1627: a second, SAMPLED decode
                agreement_gen = model.generate(audio_chunk[-1:], encoder_states=encoder_out_for_teacher, sample=True,
                                               temperature=args.__dict__.get('teacher_decode_agreement_temperature', 0.7))
                agreement_text = tokenizer.decode(agreement_gen["text_sequence"]).strip()
            print(f'Teacher pred: {teacher_pred_text}')
            skip, reason = should_skip_faulty_teacher_prediction(
                args=args, teacher_pred_tokens=teacher_pred_tokens, teacher_pred_text=teacher_pred_text, spec_frames=audio_chunk.shape[-1],
                agreement_text=agreement_text, teacher_mean_max_prob=teacher_mean_max_prob, teacher_mean_entropy=teacher_mean_entropy, ctc_text=ctc_text)
            if skip:
                print(f'Skipping teacher update: {reason}')
                continue
            for layer in model.language_model_decoder.layers:                            # lib.py:1636-1637
                layer[0].fn.dropout_p = dropout_attn
            model.language_model_decoder.train()   # for dropout
            if mode == 'teacher_ce':
                optimizer.zero_grad()
                out = calc_loss_enc_dec(model=model, audio_signal=audio_chunk[:num_negatives].contiguous(), text_sequence=teacher_pred[None, :],
                                        a_lengths=acoustic_length, t_lengths=text_lengths, tokenizer=tokenizer)
                print(out['loss'], "loss (teacher_ce)")
                optimizer.step()
            else:                                                                        # lib.py:1659-1702
                original_ctc_loss_weight = model.ctc_loss_weight
                model.ctc_loss_weight = 0.0
                rl_audio = audio_chunk[:num_negatives].contiguous()
                student_rollouts, _, rollout_lengths = generate_enc_dec(model=model, audio_signal=rl_audio, sample=4, greedy=False, temperature=1.0)
                # the reference decodes the padded rows (`seq.tolist()`, :1673); the padding is cut here: id 0 is a word of the
                # synthetic tokenizer, and `_policy_forward` re-encodes the text, so padding would become tokens of the hypothesis
                student_rollouts_text = [tokenizer.decode(seq[:int(n)].tolist()).strip() for seq, n in zip(student_rollouts, rollout_lengths)]
                print(f'Student rollouts: {student_rollouts_text} \n--------------------------------\n')
                rewards = reward_fn(teacher_pred_text, student_rollouts_text)
                print(rewards)
                if sum(rewards) / len(rewards) > 0.95:                                   # :1679-1682: no update for this window
                    pass
                elif all(r == 0.0 for r in rewards) or all(r == rewards[0] for r in rewards):
                    print('skipping')
                else:
                    optimizer.zero_grad()        # before the update: the gradient is accumulated by update_*, not by a later .backward()
                    if mode == 'maxrl':
                        loss = update_maxrl(model, audio_signal=rl_audio, tokenizer=tokenizer, hyps=student_rollouts_text, rewards=rewards,
                                            success_threshold=getattr(args, 'maxrl_success_threshold', 0.9))
                    else:
                        loss = update_grpo(model, audio_signal=rl_audio, tokenizer=tokenizer, hyps=student_rollouts_text, rewards=rewards,
                                           normalize_std=getattr(args, 'grpo_normalize_std', True))
                    if loss is not None:
                        optimizer.step()
                model.ctc_loss_weight = original_ctc_loss_weight
            model.language_model_decoder.eval()                                          # lib.py:1703-1707
            for layer in model.language_model_decoder.layers:
                layer[0].fn.dropout_p = 0
    model.eval()
    final_out = enc_dec_inference(model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=use_tqdm)
    if return_params:
        updated_model_params = [p.clone().detach().cpu() for p in model.parameters()]
    model.flat_params.copy_(original_flat)
    return final_out if not return_params else (final_out, updated_model_params)
