"""Dynamic evaluation of a transducer on transducer pseudo-labels: the token-and-duration one (parakeet_tdt_model.ParakeetForTDT) or the
plain RNN-T (parakeet_rnnt_model.ParakeetForRNNT, a subclass).  The loop reaches the model only through encode / generate / head /
backward and reads nothing of the head's own (no `durations`): with a ParakeetForRNNT "the TDT loss" below is ops.rnnt_loss and "the
greedy TDT decode" the RNN-T stepping rule.  `dynamic_eval_transducer_loss` is the head-neutral name of `dynamic_eval_tdt_loss`.

The reference has NO transducer loop: this one is DEFINED HERE, on the pattern of its third loop (reference nvidia_ctc/lib.py:35-193) as
nvidia_ctc_lib.dynamic_eval_ctc_loss mirrors it, with the same signature, flags and `apply_args`.  Line by line against that loop:
  :58-64   spectrogram [1, n_mels, T]; the parameters are snapshotted                      -- the same
  :66-72   CTCLoss / GreedyCTCDecoder / SpecAugment                                        -- the TDT loss (ops.tdt_loss), the greedy TDT decode
                                                                                              (model.generate), the same SpecAugment
  :74,89-102 training mode with the conv modules' batch norm replaced by BatchRenorm       -- `batch_renorm=True`, as in the CTC loop: it is the
                                                                                              encoder's (model.batch_renorm_training())
  :81-86   pre_encode and `decoder` frozen                                                 -- `encoder.subsampling.` and `decoder.`: NeMo's
                                                                                              `decoder` of a transducer is the prediction network.
                                                                                              The joint head and `encoder_projector` adapt.
  :105     the optimiser over the trainable parameters                                     -- the same (optim.Adam)
  :110     the overlap is a multiple of the downsampling factor                            -- the same
  :116-125 the windows                                                                     -- the same
  :135-137 num_negatives + 1 copies, SpecAugment on all but the last                       -- the same, by the same RNG rule
  :141-142 one grad-mode forward of all copies                                             -- one grad-mode ENCODER forward of all copies
  :144-146 greedy decode of the clean copy, text hop                                       -- greedy TDT decode of the clean copy's encoder states,
                                                                                              text_to_ids(ids_to_text(tokens))
  :147-152 CTC loss of the augmented copies on the pseudo-labels / (N * B)                 -- TDT loss (reduction "sum") of the augmented copies on
                                                                                              [start] + ids, grad_scale = 1 / (T' * num_negatives).
                                                                                              Empty labels are legal: the all-blank path.  A loss
                                                                                              that is not finite skips the step.
  :155-160 backward, optimiser step                                                        -- the same
  :165-187 stitching of exp(log_p) over the overlaps                                       -- a transducer has no per-frame posteriors to average:
                                                                                              every window keeps the clean copy's decode, taken
                                                                                              BEFORE that window's update, frames made absolute,
                                                                                              and merge_window_tokens cuts the windows at the
                                                                                              midpoints of their overlaps
  :189-191 parameters restored                                                             -- the same, and the `frozen` set
Returns (ids, frames, text)."""
import contextlib
import random

import torch

from . import ops
from ._loop import window_fill_value
from .augment import SpecAugment
from .nvidia_ctc_lib import BATCH_RENORM, SPEC_AUGMENT_CONFIG, SyntheticTokenizer, apply_args, disable_dropout, loop_constants  # noqa: F401
from .optim import MADGRAD, Adam  # noqa: F401

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **_):
        return x


def merge_window_tokens(windows, downsampling_factor):
    """Pure host function.  `windows`: an iterable of (start, length, tokens, frames) in any order: the window's first input frame, its
    length in input frames, and its decode with ABSOLUTE encoder frames.  Consecutive windows (by start) are cut at the midpoint of their
    overlap in input frames, (next start + this start + this length) / 2: with no overlap that is the seam.  A token at encoder frame f
    belongs to the window whose [lo, hi) contains f * downsampling_factor; the first window owns everything before its hi, the last
    everything from its lo.  Returns (ids, frames) in window order."""
    ws = sorted(((int(s), int(n), list(t), list(f)) for s, n, t, f in windows), key=lambda w: w[0])
    factor = int(downsampling_factor)
    if factor < 1:
        raise ops.DynError(f"downsampling_factor={downsampling_factor!r} must be a positive integer")
    ids, frames = [], []
    for k, (s, n, toks, frs) in enumerate(ws):
        if len(toks) != len(frs):
            raise ops.DynError(f"window at {s}: {len(toks)} tokens but {len(frs)} frames")
        if k and s == ws[k - 1][0]:
            raise ops.DynError(f"two windows start at input frame {s}")
        # twice the boundaries, so that the midpoint of an odd overlap stays an integer
        lo2 = None if k == 0 else s + ws[k - 1][0] + ws[k - 1][1]
        hi2 = None if k == len(ws) - 1 else ws[k + 1][0] + s + n
        for t, f in zip(toks, frs):
            x2 = 2 * int(f) * factor
            if (lo2 is None or x2 >= lo2) and (hi2 is None or x2 < hi2):
                ids.append(int(t))
                frames.append(int(f))
    return ids, frames


def dynamic_eval_tdt_loss(args, model, spec, seq_len, overlap, tokenizer, use_tqdm=True, optim=Adam, num_negatives=4, lr_args={'lr': 1e-8},
                          spec_augment_config=SPEC_AUGMENT_CONFIG, return_device=False, downsampling_factor=None, frozen_prefixes=None,
                          batch_renorm=None):
    """See the module docstring.  `tokenizer.vocab_size` counts the labels without the blank (the model has vocab_size + 1 token classes).
    `return_device` is accepted for the shared signature; the outputs are host lists."""
    if batch_renorm is None:
        batch_renorm = bool(args.__dict__.get('batch_renorm', False))
    device = model.device
    spec = spec.to(device=device, dtype=torch.float32)                                           # [1, F, T]
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ops.DynError(f"spec must be [1, n_mels, T], got {tuple(spec.shape)}")
    if num_negatives < 1:
        raise ops.DynError(f"num_negatives={num_negatives} must be positive")
    Fq, spec_n = spec.shape[1], spec.shape[-1]
    factor, frozen = loop_constants(model)
    downsampling_factor = factor if downsampling_factor is None else int(downsampling_factor)
    frozen = frozen if frozen_prefixes is None else tuple(frozen_prefixes)
    model = disable_dropout(model)
    original = model.flat_params.clone()
    was_frozen = model.frozen
    model.frozen = set(was_frozen) | set(frozen)
    mode = contextlib.ExitStack()
    try:
        if batch_renorm:
            mode.enter_context(model.batch_renorm_training(**BATCH_RENORM))
        augmentation = SpecAugment(**spec_augment_config)
        generator = args.__dict__.get('spec_augment_generator', None)
        optimizer = optim(model.parameters(), **lr_args)
        if seq_len > spec_n:
            seq_len, overlap = spec_n, 0
        assert overlap / downsampling_factor == overlap // downsampling_factor, 'Overlap must be a multiple of the downsampling factor'
        last_ulen, kill_next, training_data = None, False, {}
        for i in range(0, spec_n, seq_len - overlap):
            chunk = spec[:, :, i:i + seq_len]
            u_len = chunk.shape[-1]
            if kill_next:
                break
            elif last_ulen is not None and u_len < last_ulen:
                kill_next = True
            last_ulen = u_len
            training_data[i] = chunk
        outputs = {}
        B = num_negatives + 1
        start = model.start_token
        for epoch in range(args.__dict__.get('epochs', 1)):
            outputs = {}
            keys = list(training_data.keys())
            keys = random.sample(keys, len(keys)) if args.__dict__.get('shuffle', False) else keys
            for i in (tqdm(keys) if use_tqdm else keys):
                chunk = training_data[i][0]                                                      # [F, u_len], a view of the recording
                u_len = chunk.shape[-1]
                feats = torch.empty(B, u_len, Fq, device=device, dtype=torch.float32)
                copy = torch.empty(Fq, u_len, device=device, dtype=torch.float32)
                for j in range(B):                                                               # the last copy stays clean
                    if j < num_negatives:
                        copy.copy_(chunk)
                        masks = augmentation.draw(Fq, u_len, generator)
                        if masks[0][0] or masks[1][0]:
                            augmentation.apply(copy, masks, window_fill_value(copy, augmentation.zero_masking))
                        ops.transpose_ft(copy, out=feats[j])
                    else:
                        ops.transpose_ft(chunk, out=feats[j])
                with torch.enable_grad():
                    enc = model.encode(feats)                                                    # one grad-mode encoder pass of all copies
                N = enc.shape[1]
                dec = model.generate(enc=enc[-1:])                                               # the clean copy, before this window's update
                n = int(dec.count[0])
                toks, frs = dec.tokens[0, :n].tolist(), dec.frames[0, :n].tolist()
                outputs[i] = (u_len, toks, [f + i // downsampling_factor for f in frs])
                ids = tokenizer.text_to_ids(tokenizer.ids_to_text(toks))
                with torch.enable_grad():
                    out = model.head(enc, torch.tensor([[start] + ids]), torch.tensor([ids], dtype=torch.int64).reshape(1, len(ids)),
                                     reduction="sum", grad_scale=1.0 / (N * num_negatives), n_active=num_negatives, label_lengths=[len(ids)])
                optimizer.zero_grad()
                if bool(torch.isfinite(out.loss).all()):                                         # an unreachable lattice: no step
                    model.backward()
                    optimizer.step()
        ids, frames = merge_window_tokens([(i, o[0], o[1], o[2]) for i, o in outputs.items()], downsampling_factor)
    finally:
        mode.close()
        model.flat_params.copy_(original)
        model.frozen = was_frozen
    return ids, frames, tokenizer.ids_to_text(ids)


dynamic_eval = dynamic_eval_transducer_loss = dynamic_eval_tdt_loss
