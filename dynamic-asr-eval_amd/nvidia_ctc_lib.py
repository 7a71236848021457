"""Drop-in mirror of the reference's third dynamic-eval library (reference nvidia_ctc/lib.py: NVIDIA's conformer-CTC models) on the HIP
path: the chunked `dynamic_eval_ctc_loss` / `dynamic_eval` (:35-193) and `apply_args` (:206-221).

Same call signature; `model` is this package's ParakeetForCTC (parakeet_model.py), the FastConformer-CTC architecture as transformers
restates it, so no NeMo is needed, or a model of its family that says what the loop has to know about it (lasr_model.LasrForCTC: the
attributes `downsampling_factor` and `frozen_in_the_loop`, read by loop_constants below).  The loop follows wav2vec2_lib.dynamic_eval_ctc_loss statement for statement; what differs, as in the
reference:
  * `spec` [1, n_mels, T] is a spectrogram, computed outside the loop (nvidia_ctc/lib.py:20-28; here get_spectrogram / preprocess
    below, on the device), cut into windows along T (:116-125); every
    copy is transposed to [T, n_mels] on the device, the layout transformers' model takes;
  * SpecAugment (augment.SpecAugment, `spec_augment_config`) on the first `num_negatives` copies, one draw per copy in index order from the
    host torch RNG (`args.spec_augment_generator`, a torch.Generator, when given).  The reference's SpecAugment comes from an un-vendored
    package: the draw rule is augment.py's (parity unpinned, as for the other loops);
  * Adam (optim.Adam: one fused launch over the flat vector);
  * `pre_encode` and the decoder do not adapt (:81-86): the model's `frozen_in_the_loop` prefixes (Parakeet: `encoder.subsampling.` and
    `ctc_head.`) are in `model.frozen` for the duration of the call (`pos_enc` has no parameters), so their backward is not run at all;
  * the conv modules' norm.  The reference calls `model.train()` (:74), puts `layer.conv` and its batch norm into eval mode (:92-93) and then
    REPLACES that batch norm by a fresh BatchRenorm1d(momentum=0.001, eps=1e-5) (:94-102), which is in training mode: at every step it
    normalises with the statistics of the batch (augmented copies and the clean one), corrects them towards the running statistics by the
    detached r / d (num_batches_tracked = 1000000 saturates the clamps at 3 / 5, :97; running_std = sqrt(running_var), :101), moves the
    running statistics, and the gradient flows through the batch mean and deviation into every row.  `batch_renorm=True` (or
    `args.batch_renorm`) runs exactly that (model.batch_renorm_training(), csrc/convmod_brn.hip; BatchRenorm1d is un-vendored: the
    `batchrenorm` package form, parity unpinned against upstream `lcasr`).  The DEFAULT is still the eval-mode norm reading its running
    statistics, until a maintainer flips it;
  * blank = `tokenizer.vocab_size`, greedy pseudo-labels from the clean last copy, `CTCLoss(reduction="sum") / (N * B)`, probability-space
    stitching by the window's own ratio of input to output frames (:165-187; the model's `downsampling_factor`, 8 for Parakeet, is what the
    overlap must be a multiple of, :110); parameters and the `frozen` set are restored on exit (:189-191).
The tokenizer is NeMo's surface: `vocab_size` (an attribute), `ids_to_text`, `text_to_ids`; SyntheticTokenizer is the stand-in for seeded
weights."""
import contextlib
import random

import torch

from . import ops
from ._loop import Stitcher, window_fill_value
from .augment import SpecAugment
from .decoding import GreedyCTCDecoder
from .optim import MADGRAD, Adam  # noqa: F401

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **_):
        return x

SPEC_AUGMENT_CONFIG = {'n_time_masks': 3, 'n_freq_masks': 3, 'freq_mask_param': 40, 'time_mask_param': -1, 'min_p': 0.05, 'zero_masking': False}


class SyntheticTokenizer:
    """Stand-in for a NeMo tokenizer with seeded weights: token i <-> the word "w<i>", so ids_to_text -> text_to_ids is an exact identity and
    the pseudo-label text hop of the reference is preserved.  `vocab_size` does not count the CTC blank (the model has vocab_size + 1 classes)."""

    def __init__(self, vocab_size):
        self.vocab_size = int(vocab_size)

    def ids_to_text(self, ids):
        return " ".join(f"w{int(i)}" for i in ids)

    def text_to_ids(self, text):
        return [int(w[1:]) for w in text.split() if len(w) > 1 and w[0] == "w" and w[1:].isdigit() and int(w[1:]) < self.vocab_size]


class SentencePieceAdapter:
    """reference nvidia_ctc/lib.py:196-204."""

    def __init__(self, tokenizer):
        self.tokenizer = tokenizer

    def decode(self, ids):
        return self.tokenizer.ids_to_text(ids)

    def encode(self, text):
        return self.tokenizer.text_to_ids(text)


BATCH_RENORM = dict(momentum=0.001, eps=1e-5, num_batches_tracked=1000000)      # nvidia_ctc/lib.py:94-97
DOWNSAMPLING_FACTOR = 8                                      # nvidia_ctc/lib.py:60, and
FROZEN_IN_THE_LOOP = ("encoder.subsampling.", "ctc_head.")   # :81-86 for the FastConformer the reference drives: the defaults below


def loop_constants(model):
    """(downsampling factor, parameter-name prefixes frozen for the duration of the loop) of `model` (an instance or its class): its
    `downsampling_factor` / `frozen_in_the_loop` attributes, or the reference's own constants for a model that does not say."""
    factor = int(getattr(model, "downsampling_factor", DOWNSAMPLING_FACTOR))
    frozen = tuple(getattr(model, "frozen_in_the_loop", FROZEN_IN_THE_LOOP))
    if factor < 1 or not all(isinstance(p, str) and p for p in frozen):
        raise ops.DynError(f"{type(model).__name__}: downsampling_factor={factor!r} / frozen_in_the_loop={frozen!r} are not a positive integer and "
                           "non-empty parameter-name prefixes")
    return factor, frozen


def get_spectrogram(audio_signal, model, device=None):
    """reference nvidia_ctc/lib.py:20-23: audio_signal [1, L] (16 kHz mono) -> spec [1, n_mels, T] on the device, through the model's own
    front end (model.feature_extractor(): frontend.MelFeatures, csrc/melfeat.hip) in the loop's layout.  NeMo's preprocessor is not a
    dependency, so the layout and the trimming are DEFINED here: the transformers extractor's features of the model's family, transposed,
    cut to the row's valid frames (L // 160 for Parakeet; the extractor's last, masked frame is dropped).  `device` must be the model's
    (None: the model's); anything else, the 'cpu' of the reference's `preprocess` included, is refused by name."""
    if device is not None:
        d, m = torch.device(device), torch.device(model.device)
        if d.type != m.type or (d.index is not None and d.index != m.index):
            raise ops.DynError(f"get_spectrogram: device={device!r} is not the model's ({model.device}): the front end runs where the model "
                               "lives (there is no CPU path)")
    x = torch.as_tensor(audio_signal)
    if x.dim() == 1:
        x = x[None, :]
    if x.dim() != 2 or x.shape[0] != 1:
        raise ops.DynError(f"get_spectrogram: audio_signal must be one mono recording [1, L], not {tuple(x.shape)} (multi-channel input is "
                           "out of scope)")
    x = x.to(device=model.device, dtype=torch.float32).contiguous()
    spec, lens = model.feature_extractor()(x, layout="ft")
    return spec[:, :, :lens[0]].contiguous()


def preprocess(audio, model):
    """reference nvidia_ctc/lib.py:25-28: a recording -> spec [1, n_mels, T] on the model's device.  `audio`: the path of a 16 kHz mono PCM
    `.wav` (read with scipy.io.wavfile; integer PCM is scaled to [-1, 1) as torchaudio.load does), a tensor or an ndarray [L] / [1, L]."""
    if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__"):
        import numpy as np
        from scipy.io import wavfile
        sr, data = wavfile.read(audio)
        if sr != 16000:
            raise ops.DynError(f"{audio}: sampling rate {sr} Hz is not built (16000; resampling is out of scope)")
        if data.ndim != 1:
            raise ops.DynError(f"{audio}: {data.shape[1]} channels; mono only (multi-channel input is out of scope)")
        if np.issubdtype(data.dtype, np.integer):
            if data.dtype == np.uint8:
                data = (data.astype(np.float32) - 128.0) / 128.0
            else:
                data = data.astype(np.float32) / float(1 << (8 * data.dtype.itemsize - 1))
        audio = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))[None, :]
    return get_spectrogram(audio, model, None)


def disable_dropout(model):
    """reference nvidia_ctc/lib.py:30-33 — the model has no dropout modules (eval-mode forward)."""
    return model


def dynamic_eval_ctc_loss(args, model, spec, seq_len, overlap, tokenizer, use_tqdm=True, optim=Adam, num_negatives=4, lr_args={'lr': 1e-8},
                          spec_augment_config=SPEC_AUGMENT_CONFIG, return_device=False, downsampling_factor=None, frozen_prefixes=None,
                          batch_renorm=None):
    """reference nvidia_ctc/lib.py:35-193: spectrogram windows, SpecAugment on the first copies, Adam, stitching of exp(log_p[-1]).
    `downsampling_factor` / `frozen_prefixes`: given, they take the place of what loop_constants reads from the model.
    `batch_renorm` (None: `args.batch_renorm`, False when absent): True runs the loop inside model.batch_renorm_training() with the
    reference's constants (:94-102) and hands the backward a gradient for all B rows, zeros for the clean copy, since the training-mode
    norm carries it into every row.  The state (running statistics, counters) is dropped on exit, so the model's buffers are restored
    trivially: they are never written."""
    if batch_renorm is None:
        batch_renorm = bool(args.__dict__.get('batch_renorm', False))
    device = model.device
    spec = spec.to(device=device, dtype=torch.float32)                                           # [1, F, T]
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ops.DynError(f"spec must be [1, n_mels, T], got {tuple(spec.shape)}")
    Fq, spec_n = spec.shape[1], spec.shape[-1]
    factor, frozen = loop_constants(model)
    downsampling_factor = factor if downsampling_factor is None else int(downsampling_factor)
    frozen = frozen if frozen_prefixes is None else tuple(frozen_prefixes)
    model = disable_dropout(model)
    original = model.flat_params.clone()                                                         # lib.py:63-64
    was_frozen = model.frozen
    model.frozen = set(was_frozen) | set(frozen)                                     # lib.py:81-86
    mode = contextlib.ExitStack()
    try:
        if batch_renorm:
            mode.enter_context(model.batch_renorm_training(**BATCH_RENORM))                      # lib.py:74,89-102
        blank = tokenizer.vocab_size                                                             # lib.py:66,71
        decoder = GreedyCTCDecoder(tokenizer=SentencePieceAdapter(tokenizer), blank_id=blank, device=device)
        augmentation = SpecAugment(**spec_augment_config)
        generator = args.__dict__.get('spec_augment_generator', None)
        optimizer = optim(model.parameters(), **lr_args)                                         # lib.py:105
        if seq_len > spec_n:
            seq_len, overlap = spec_n, 0
        assert overlap / downsampling_factor == overlap // downsampling_factor, 'Overlap must be a multiple of the downsampling factor'
        stitch = Stitcher.for_recording(spec_n, seq_len, tokenizer.vocab_size + 1, device)       # lib.py:113
        last_ulen, kill_next, training_data = None, False, {}
        for i in range(0, spec_n, seq_len - overlap):                                            # lib.py:116-125
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
                for j in range(B):                                                               # lib.py:135-137: the last copy stays clean
                    if j < num_negatives:
                        copy.copy_(chunk)
                        masks = augmentation.draw(Fq, u_len, generator)
                        if masks[0][0] or masks[1][0]:
                            augmentation.apply(copy, masks, window_fill_value(copy, augmentation.zero_masking))
                        ops.transpose_ft(copy, out=feats[j])
                    else:
                        ops.transpose_ft(chunk, out=feats[j])
                with torch.enable_grad():
                    out = model(input_features=feats)                                            # lib.py:141
                log_p = ops.log_softmax(out.logits)
                N = out.frames
                ids = tokenizer.text_to_ids(decoder(log_p[-1, :N]))                              # lib.py:144-146
                S = len(ids)
                targets = torch.tensor([ids if S else [0]] * num_negatives, dtype=torch.int32, device=device)
                aug = log_p[:num_negatives].contiguous()
                nb = aug.shape[0]
                ilen = torch.full((nb,), N, dtype=torch.int32, device=device); tlen = torch.full((nb,), S, dtype=torch.int32, device=device)
                _, _, g_lp = ops.ctc_loss(aug, targets, ilen, tlen, blank, reduction="sum", grad_scale=1.0 / (N * nb))   # lib.py:149-152
                optimizer.zero_grad()
                if batch_renorm:                                                                 # every row takes part in the batch statistics
                    g_all = torch.zeros_like(log_p)
                    g_all[:num_negatives].copy_(g_lp)
                    model.backward(ops.log_softmax_bwd(log_p, g_all), n_active=B)
                else:
                    model.backward(ops.log_softmax_bwd(aug, g_lp), n_active=num_negatives)       # lib.py:155-156
                optimizer.step()                                                                 # lib.py:160
                outputs[i] = (log_p[-1, :N], u_len)                                              # lib.py:165-170
        for i in sorted(outputs):                                                                # lib.py:174-187
            stitch.add(i, *outputs[i], overlap)
        logits = stitch.finalize()
    finally:
        mode.close()
        model.flat_params.copy_(original)                                                        # lib.py:189-191
        model.frozen = was_frozen
    return logits if return_device else logits.cpu().numpy()


dynamic_eval = dynamic_eval_ctc_loss


def apply_args(parser, argv=None):
    """reference nvidia_ctc/lib.py:206-221 (same flags).  The reference falls back to `paths.checkpoints.nvidia_ctc` when -c is empty; no
    paths.yaml exists offline, so an empty -c stays empty (seeded weights)."""
    parser.add_argument('-c', '--checkpoint', type=str, default='', help='path to checkpoint')
    parser.add_argument('-split', '--split', type=str, default='test', help='test or dev split')
    parser.add_argument('-seq', '--seq_len', type=int, default=2048)
    parser.add_argument('-overlap', '--overlap', type=int, default=0)
    parser.add_argument('-nv', '--not_verbose', action='store_true', help='verbose')
    parser.add_argument('-log', '--log', type=str, default='')
    parser.add_argument('-shuffle', '--shuffle', action='store_true', help='shuffle')
    parser.add_argument('-epochs', '--epochs', type=int, default=1, help='epochs')
    parser.add_argument('-dfa', '--disable_flash_attention', action='store_true', help='disable flash attention')
    args = parser.parse_args(argv)
    args.verbose = not args.not_verbose
    return args
