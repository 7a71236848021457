"""References of the FastConformer family's waveform front end (frontend.MelFeatures, csrc/melfeat.hip), all on the CPU:
  * make_extractor: transformers' own feature extractor classes, built WITHOUT their constructors (three of the four import librosa there,
    which is not a dependency): `cls.__new__`, SequenceFeatureExtractor.__init__, the attributes `__call__` reads, and `mel_filters` from
    transformers.audio_utils.mel_filter_bank (the call the extractors' TODO names as librosa's replacement) in float32.  `__call__` then
    runs unchanged.  LasrFeatureExtractor() constructs normally.
  * features_f64: each mode's formula restated in float64 from its definition (zero padding, rfft of the windowed 512-point frame, the
    float32 filter values, log, per-row per-bin normalisation over the valid frames), independent of the device path's strided-row GEMM.
  * chain32: the device path's own chain in float32 torch (strided frames @ basis, power, @ filters, log, torch's two-pass statistics):
    what kernel_refs.measured_tol measures against features_f64 to set the device's bound.
Measured on the CPU (random audio at 0.1 amplitude; 5000 | 3333, 16000 | 801, 48000): features_f64 reproduces the extractors' valid-frame
counts exactly; Parakeet (values up to 5): extractor 2.9e-5 .. 4.8e-5, chain32 1.3e-5 .. 2.1e-5 from features_f64; Nemotron (values up to
16): 1.3e-4 .. 1.4e-4 and 4.3e-5 .. 1.6e-4."""
import math

import numpy as np
import torch

F64 = torch.float64
N_FFT, WIN, HOP, SR = 512, 400, 160, 16000
GUARD = 2.0 ** -24
EPS = 1e-5
MODES = ("parakeet", "nemotron_asr_streaming", "cohere_asr", "lasr")
NORMALISED = ("parakeet", "cohere_asr")


def extractor_class(kind):
    if kind == "parakeet":
        from transformers.models.parakeet.feature_extraction_parakeet import ParakeetFeatureExtractor as C
    elif kind == "nemotron_asr_streaming":
        from transformers.models.nemotron_asr_streaming.feature_extraction_nemotron_asr_streaming import NemotronAsrStreamingFeatureExtractor as C
    elif kind == "cohere_asr":
        from transformers.models.cohere_asr.feature_extraction_cohere_asr import CohereAsrFeatureExtractor as C
    else:
        from transformers.models.lasr.feature_extraction_lasr import LasrFeatureExtractor as C
    return C


def slaney_filters(feature_size):
    """[257, F] float32: mel_filter_bank(slaney scale, slaney norm, 0 - 8000 Hz) rounded to float32."""
    from transformers.audio_utils import mel_filter_bank
    return torch.from_numpy(mel_filter_bank(N_FFT // 2 + 1, feature_size, 0.0, SR / 2, SR, norm="slaney", mel_scale="slaney")).to(torch.float32)


def make_extractor(cls, feature_size, dither=None):
    """transformers' extractor class `cls` without its constructor (see the module docstring)."""
    from transformers.feature_extraction_sequence_utils import SequenceFeatureExtractor
    if cls.__name__ == "LasrFeatureExtractor":
        return cls(feature_size=feature_size)
    fe = cls.__new__(cls)
    SequenceFeatureExtractor.__init__(fe, feature_size=feature_size, sampling_rate=SR, padding_value=0.0)
    fe.hop_length, fe.n_fft, fe.win_length, fe.preemphasis = HOP, N_FFT, WIN, 0.97
    fe.mel_filters = slaney_filters(feature_size).T.contiguous()
    if cls.__name__ == "CohereAsrFeatureExtractor":
        fe.dither = 1e-5 if dither is None else dither
        fe.max_audio_clip_s, fe.overlap_chunk_second, fe.min_energy_window_samples = 35.0, 5.0, 1600
    return fe


def run_extractor(fe, rows, center=True):
    """rows: 1-D float32 tensors -> (input_features [B, T, F] float32, attention_mask [B, T] bool)."""
    kw = {}
    name = type(fe).__name__
    if name == "NemotronAsrStreamingFeatureExtractor":
        kw["center"] = center
    if name == "LasrFeatureExtractor":
        kw["return_attention_mask"] = True
    out = fe([r.numpy().copy() for r in rows], sampling_rate=SR, return_tensors="pt", **kw)
    return out["input_features"], out["attention_mask"].bool()


def valid_frames(kind, L, center=True):
    """Written from the extractors' own expressions (features_lengths / the strided attention mask)."""
    if kind == "lasr":
        return len(range(WIN - 1, L, HOP))
    if center:
        return (L + N_FFT // 2 * 2 - N_FFT) // HOP
    return max(0, (L - N_FFT) // HOP + 1) if L >= N_FFT else 0


def output_frames(kind, Lmax, center=True):
    if kind == "lasr":
        return 1 + (Lmax - WIN) // HOP
    return 1 + Lmax // HOP if center else 1 + (Lmax - N_FFT) // HOP


def dither_noise(rows):
    """CohereAsrFeatureExtractor._apply_dither's noise per row: randn(L) from a CPU generator seeded with L."""
    g = torch.Generator(device="cpu")
    out = []
    for r in rows:
        g.manual_seed(r.numel())
        out.append(torch.randn(r.numel(), dtype=torch.float32, generator=g))
    return out


def signal(kind, rows, dtype, dither=0.0):
    """[B, Lmax] in `dtype`: the padded batch after dither, pre-emphasis over the whole signal (sample 0 kept) and the length mask.  The
    coefficients are the extractor's float32 values."""
    Lmax = max(r.numel() for r in rows)
    x = torch.zeros(len(rows), Lmax, dtype=dtype)
    noise = dither_noise(rows) if (kind == "cohere_asr" and dither > 0) else None
    for b, r in enumerate(rows):
        v = r.to(dtype)
        if noise is not None:
            v = v + torch.tensor(dither, dtype=torch.float32).to(dtype) * noise[b].to(dtype)
        x[b, :r.numel()] = v
    if kind != "lasr":
        pre = torch.tensor(0.97, dtype=torch.float32).to(dtype)
        x = torch.cat([x[:, :1], x[:, 1:] - pre * x[:, :-1]], dim=1)
        for b, r in enumerate(rows):
            x[b, r.numel():] = 0
    return x


def hann(dtype=F64):
    n = torch.arange(WIN, dtype=F64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * n / (WIN - 1))).to(dtype)


def filters64(kind, feature_size):
    if kind == "lasr":
        from transformers.models.lasr.feature_extraction_lasr import linear_to_mel_weight_matrix
        return torch.from_numpy(linear_to_mel_weight_matrix(feature_size, N_FFT // 2 + 1, SR, 125.0, 7500.0, np.float64))
    return slaney_filters(feature_size).to(F64)


def finish(logv, lens, normalise):
    """logv [B, T, F] -> per-row per-bin (x - mean) / (unbiased std + 1e-5) over the valid frames (torch's two-pass mean / std at logv's
    dtype; in float64 the mean is taken around the first frame, so a bin of equal values is exact zeros, as in exact arithmetic), zeros
    past them."""
    out = torch.zeros_like(logv)
    for b, n in enumerate(lens):
        v = logv[b, :n]
        if normalise:
            mean = v.mean(0, keepdim=True)
            if v.dtype == F64:                                  # the exact mean of equal values is the value: centre on the first frame
                mean = v[:1] + (v - v[:1]).mean(0, keepdim=True)
            std = torch.sqrt(((v - mean) ** 2).sum(0, keepdim=True) / (n - 1))
            v = (v - mean) / (std + EPS)
        out[b, :n] = v
    return out


def log_rule(kind, mel):
    return torch.log(mel.clamp(min=1e-5)) if kind == "lasr" else torch.log(mel + GUARD)


def features_f64(kind, rows, feature_size, center=True, dither=0.0):
    """(features [B, T, F] float64, valid frames per row): the mode's formula in float64."""
    x = signal(kind, rows, F64, dither)
    B, Lmax = x.shape
    lens = [valid_frames(kind, r.numel(), center) for r in rows]
    T = output_frames(kind, Lmax, center)
    w = hann()
    if kind == "lasr":
        frames = x.unfold(-1, WIN, HOP)[:, :T] * w
        spec = torch.fft.rfft(frames, n=N_FFT)
    else:
        if center:
            x = torch.nn.functional.pad(x, (N_FFT // 2, N_FFT // 2))
        w512 = torch.zeros(N_FFT, dtype=F64)
        w512[(N_FFT - WIN) // 2:(N_FFT - WIN) // 2 + WIN] = w
        spec = torch.fft.rfft(x.unfold(-1, N_FFT, HOP)[:, :T] * w512)
    power = spec.real ** 2 + spec.imag ** 2
    return finish(log_rule(kind, power @ filters64(kind, feature_size)), lens, kind in NORMALISED), lens


def chain32(kind, rows, basis32, fb32, center=True, dither=0.0):
    """The device path's chain in float32 torch: strided 400-sample frames @ basis [400, 520], power, @ fb [260, F], log, statistics."""
    x = signal(kind, rows, torch.float32, dither)
    B, Lmax = x.shape
    lens = [valid_frames(kind, r.numel(), center) for r in rows]
    T = output_frames(kind, Lmax, center)
    off = 0 if kind == "lasr" else (N_FFT - WIN) // 2
    if kind != "lasr" and center:
        x = torch.nn.functional.pad(x, (N_FFT // 2, N_FFT // 2))
    frames = x[:, off:].unfold(-1, WIN, HOP)[:, :T]
    reim = frames @ basis32
    KP = basis32.shape[1] // 2
    power = reim[..., :KP] ** 2 + reim[..., KP:] ** 2
    return finish(log_rule(kind, power @ fb32), lens, kind in NORMALISED), lens


def audio(L, seed, amplitude=0.1, offset=0.0):
    return amplitude * torch.randn(L, generator=torch.Generator().manual_seed(seed)) + offset
