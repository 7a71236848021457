"""Dynamic evaluation of an attention encoder-decoder (cohere_asr_model.CohereAsrForConditionalGeneration) on its own greedy decode: the
third loop with a third kind of head, after the CTC one (nvidia_ctc_lib.py) and the transducers' (parakeet_tdt_lib.py).

The reference has NO seq2seq loop: this one is DEFINED HERE, on the pattern of its third loop (reference nvidia_ctc/lib.py:35-193) as
parakeet_tdt_lib.dynamic_eval_transducer_loss mirrors it, with the same signature, flags and plumbing.  Against that loop:
  :58-64   spectrogram [1, n_mels, T]; the parameters are snapshotted                      -- the same
  :66-72   CTCLoss / GreedyCTCDecoder / SpecAugment                                        -- teacher-forced cross-entropy, model.generate, the same
                                                                                              SpecAugment
  :81-86   pre_encode and `decoder` frozen                                                 -- `model.encoder.subsampling.`, `model.decoder.` and
                                                                                              `proj_out.`; `freeze_decoder=False` adapts the decoder
                                                                                              and the head too
  :105     the optimiser over the trainable parameters                                     -- the same (optim.Adam)
  :110-125 overlap a multiple of the downsampling factor; the windows                      -- the same
  :135-137 num_negatives + 1 copies, SpecAugment on all but the last                       -- the same, by the same RNG rule
  :141-142 one grad-mode forward of all copies                                             -- one grad-mode ENCODER forward of all copies
  :144-146 greedy decode of the clean copy, text hop                                       -- model.generate on the clean copy's encoder states from
                                                                                              the forced prompt; the prompt, eos and pad are dropped;
                                                                                              text_to_ids(ids_to_text(tokens))
  :147-152 CTC loss of the augmented copies on the pseudo-labels                           -- decoder inputs prompt + ids, ONE label row shared by the
                                                                                              copies: -100 under the prompt, then ids, then eos;
                                                                                              the mean cross-entropy over the scored positions.
                                                                                              An empty pseudo-label skips the window's update.
  :155-160 backward, optimiser step                                                        -- the same
  :165-187 stitching of exp(log_p) over the overlaps                                       -- a seq2seq decode has no frames: the tokens of a window
                                                                                              are spread evenly over its encoder frames
                                                                                              (spread_frames) and parakeet_tdt_lib.merge_window_tokens
                                                                                              cuts the windows at the midpoints of their overlaps
  :189-191 parameters restored                                                             -- the same, and the `frozen` set
Returns (ids, frames, text)."""
import random

import torch

from . import ops
from ._loop import window_fill_value
from .augment import SpecAugment
from .nvidia_ctc_lib import SPEC_AUGMENT_CONFIG, disable_dropout, loop_constants
from .optim import Adam
from .parakeet_tdt_lib import merge_window_tokens

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **_):
        return x


def pseudo_label(sequence, prompt_len, eos, pad):
    """Pure host function: one row of generate()'s output -> the tokens behind the prompt without eos and pad."""
    return [int(t) for t in list(sequence)[prompt_len:] if int(t) not in (eos, pad)]


def label_row(prompt, ids, eos):
    """Pure host function: (decoder inputs, labels) of the teacher-forced pass, one row each: inputs prompt + ids; labels -100 under the
    prompt (its last token predicts ids[0]), then ids, then eos."""
    prompt, ids = [int(t) for t in prompt], [int(t) for t in ids]
    return prompt + ids, [-100] * (len(prompt) - 1) + ids + [int(eos)]


def spread_frames(n_tokens, n_frames, first_frame=0):
    """Pure host function: token k of n placed at encoder frame first_frame + floor((2k + 1) n_frames / (2n))."""
    return [first_frame + ((2 * k + 1) * n_frames) // (2 * n_tokens) for k in range(n_tokens)]


def dynamic_eval_seq2seq_loss(args, model, spec, seq_len, overlap, tokenizer, use_tqdm=True, optim=Adam, num_negatives=4, lr_args={'lr': 1e-8},
                              spec_augment_config=SPEC_AUGMENT_CONFIG, return_device=False, downsampling_factor=None, frozen_prefixes=None,
                              freeze_decoder=True, prompt_ids=None, max_new_tokens=64):
    """See the module docstring.  `prompt_ids`: the forced prompt of every decode, start token included (released checkpoints decode from
    several control tokens; None: the start token alone).  `return_device` is accepted for the shared signature; the outputs are host lists."""
    device = model.device
    spec = spec.to(device=device, dtype=torch.float32)                                           # [1, F, T]
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ops.DynError(f"spec must be [1, n_mels, T], got {tuple(spec.shape)}")
    if num_negatives < 1:
        raise ops.DynError(f"num_negatives={num_negatives} must be positive")
    Fq, spec_n = spec.shape[1], spec.shape[-1]
    factor, frozen = loop_constants(model)
    downsampling_factor = factor if downsampling_factor is None else int(downsampling_factor)
    if frozen_prefixes is not None:
        frozen = tuple(frozen_prefixes)
    elif not freeze_decoder:
        frozen = tuple(p for p in frozen if p.startswith("model.encoder."))
    prompt = [model.start_token] if prompt_ids is None else [int(t) for t in prompt_ids]
    model = disable_dropout(model)
    original = model.flat_params.clone()
    was_frozen = model.frozen
    model.frozen = set(was_frozen) | set(frozen)
    try:
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
                seq = model.generate(encoder_hidden_states=enc[-1:], decoder_input_ids=torch.tensor([prompt]), max_new_tokens=max_new_tokens)
                toks = pseudo_label(seq[0].tolist(), len(prompt), model.eos, model.pad)          # the clean copy, before this window's update
                outputs[i] = (u_len, toks, spread_frames(len(toks), N, i // downsampling_factor))
                ids = tokenizer.text_to_ids(tokenizer.ids_to_text(toks))
                optimizer.zero_grad()
                if not ids:                                                                      # nothing to teach: no step
                    continue
                dec_in, labels = label_row(prompt, ids, model.eos)
                with torch.enable_grad():
                    out = model.head(enc, torch.tensor([dec_in]), torch.tensor([labels]), n_active=num_negatives)
                if bool(torch.isfinite(out.loss).all()):
                    model.backward()
                    optimizer.step()
        ids, frames = merge_window_tokens([(i, o[0], o[1], o[2]) for i, o in outputs.items()], downsampling_factor)
    finally:
        model.flat_params.copy_(original)
        model.frozen = was_frozen
    return ids, frames, tokenizer.ids_to_text(ids)


dynamic_eval = dynamic_eval_seq2seq_loss
