"""Log-mel front end on the GPU: 16 kHz mono waveform -> spec [1, 80, T] (100 frames / s), the tensor every
`process_fn` of the reference hands to eval_fn (reference lcasr/run_dynamic_eval_full.py:84; adapters call the
un-vendored `lcasr.utils.audio_tools.processing_chain`, e.g. lcasr/earnings22/run.py:61).

Constants DEFINED here (the upstream implementation is absent; parity unpinned, the oracle oracle/logmel_ref.py restates
the same definition with torch.stft): n_fft 512, Hann(400, periodic) centred in the frame, hop 160, center=True with
reflect padding, power spectrum, 80 HTK-mel triangular filters over 0-8000 Hz (torchaudio `melscale_fbanks` rule,
norm=None), log(mel + 1e-6), then per-bin (mean, unbiased std) normalisation over the recording (the std from a second, centred pass:
a bin at the floor log(1e-6) with a spread of 1e-3 keeps its std; a bin of zero variance comes out as zeros).
The STFT is one fp32-MFMA GEMM over overlapping rows of the padded signal (lda = hop); see csrc/logmel.hip."""
import math

import torch

from . import ops
from ._lib import check, load

SAMPLE_RATE, N_FFT, WIN, HOP, N_MELS, KP = 16000, 512, 400, 160, 80, 260   # KP = 257 bins padded to a multiple of 4


def mel_filterbank(n_freqs=N_FFT // 2 + 1, f_min=0.0, f_max=8000.0, n_mels=N_MELS, sample_rate=SAMPLE_RATE):
    """[n_freqs, n_mels] triangular HTK-mel filters (torchaudio.functional.melscale_fbanks, norm=None), float64."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0)


class LogMel:
    def __init__(self, device="cuda:0", eps=1e-6, normalize=True):
        self.device, self.eps, self.normalize = torch.device(device), float(eps), bool(normalize)
        n = torch.arange(WIN, dtype=torch.float64)
        w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / WIN)                      # torch.hann_window(400, periodic=True)
        k = torch.arange(N_FFT // 2 + 1, dtype=torch.float64)
        ang = 2 * math.pi * k[None, :] * (n[:, None] + (N_FFT - WIN) // 2) / N_FFT
        basis = torch.zeros(WIN, 2 * KP, dtype=torch.float64)
        basis[:, :N_FFT // 2 + 1] = w[:, None] * torch.cos(ang)
        basis[:, KP:KP + N_FFT // 2 + 1] = -w[:, None] * torch.sin(ang)
        self.basis = basis.float().to(self.device).contiguous()                # [400, 520]
        fb = torch.zeros(KP, N_MELS, dtype=torch.float64)
        fb[:N_FFT // 2 + 1] = mel_filterbank()
        self.fb = fb.float().to(self.device).contiguous()                      # [260, 80]

    def __call__(self, waveform):
        """waveform: 1-D float tensor (host or device) -> spec [1, 80, T] on the device, T = 1 + len // 160."""
        x = torch.as_tensor(waveform, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        n = x.numel()
        pad = N_FFT // 2
        T = 1 + n // HOP
        st = torch.cuda.current_stream().cuda_stream
        xpad = torch.empty(n + 2 * pad, device=self.device, dtype=torch.float32)
        check(load().dyn_reflect_pad(x.data_ptr(), xpad.data_ptr(), n, pad, st), "dyn_reflect_pad")
        reim = torch.empty(T, 2 * KP, device=self.device, dtype=torch.float32)
        # frame t = xpad[t*160 + 56 : t*160 + 456]  (the 400-tap window sits at offset 56 of the 512-point frame)
        ops.gemm(xpad, self.basis, reim, M=T, N=2 * KP, K=WIN, lda=HOP, ldb=2 * KP, ldc=2 * KP, a_off=(N_FFT - WIN) // 2)
        power = torch.empty(T, KP, device=self.device, dtype=torch.float32)
        check(load().dyn_stft_power(reim.data_ptr(), power.data_ptr(), T, KP, st), "dyn_stft_power")
        mel = torch.empty(T, N_MELS, device=self.device, dtype=torch.float32)
        ops.gemm(power, self.fb, mel, M=T, N=N_MELS, K=KP, lda=KP, ldb=N_MELS, ldc=N_MELS)
        out = torch.empty(1, N_MELS, T, device=self.device, dtype=torch.float32)
        ws = ops.workspace(self.device)
        check(load().dyn_logmel_finish(mel.data_ptr(), out.data_ptr(), T, N_MELS, self.eps, int(self.normalize), ws.data_ptr(),
                                       ws.numel(), st), "dyn_logmel_finish")
        return out


FBANK_STACK = 2                                                              # SeamlessM4TFeatureExtractor.stride: frames stacked per row
FBANK_SCALE, FBANK_PREEMPHASIS, FBANK_MIN_HZ = 2.0 ** 15, 0.97, 20.0


def kaldi_fbank_frames(n_samples):
    """Filter-bank frames of n_samples samples (`center=False`: 1 + (L - 400) // 160) and the rows the extractor keeps of them (an odd last
    frame is dropped by its reshape to two frames per row)."""
    F = 1 + (int(n_samples) - WIN) // HOP if n_samples >= WIN else 0
    return F, F // FBANK_STACK


def kaldi_fbank_matrices():
    """(basis [400, 2 * 260], mel [260, 80]) in float64: what SeamlessM4TFeatureExtractor._extract_fbank_features does to one 400-sample
    frame before its power spectrum, folded into one matrix, and its Kaldi-scale mel filters.
    transformers' audio_utils.spectrogram, per frame, in float64: x * 2^15 (the extractor, before the call), `buffer -= buffer.mean()`
    (remove_dc_offset), `buffer[1:] -= 0.97 * buffer[:-1]; buffer[0] *= 1 - 0.97` (preemphasis), `buffer *= window` (povey, symmetric),
    rfft of the frame zero-padded to 512.  All five are linear in the frame: with A = diag(w) Pre Centre 2^15 the spectrum of frame x is
    x^T (A^T [cos | -sin]), so the whole chain is the strided-row GEMM LogMel runs with another basis.  The filters are
    audio_utils.mel_filter_bank's own values (20 Hz .. 8 kHz, Kaldi mel scale, triangles in mel space): computed, not downloaded."""
    from transformers.audio_utils import mel_filter_bank, window_function
    n = torch.arange(WIN, dtype=torch.float64)
    w = torch.from_numpy(window_function(WIN, "povey", periodic=False)).to(torch.float64)
    centre = torch.eye(WIN, dtype=torch.float64) - 1.0 / WIN
    pre = torch.eye(WIN, dtype=torch.float64)
    pre[0, 0] = 1.0 - FBANK_PREEMPHASIS
    pre[n[1:].long(), n[:-1].long()] = -FBANK_PREEMPHASIS
    A = w[:, None] * (pre @ centre) * FBANK_SCALE                            # y = A x: the windowed frame
    k = torch.arange(N_FFT // 2 + 1, dtype=torch.float64)
    ang = 2 * math.pi * k[None, :] * n[:, None] / N_FFT
    basis = torch.zeros(WIN, 2 * KP, dtype=torch.float64)
    basis[:, :N_FFT // 2 + 1] = A.T @ torch.cos(ang)
    basis[:, KP:KP + N_FFT // 2 + 1] = -(A.T @ torch.sin(ang))
    fb = torch.zeros(KP, N_MELS, dtype=torch.float64)
    fb[:N_FFT // 2 + 1] = torch.from_numpy(mel_filter_bank(num_frequency_bins=N_FFT // 2 + 1, num_mel_filters=N_MELS, min_frequency=FBANK_MIN_HZ,
                                                           max_frequency=SAMPLE_RATE // 2, sampling_rate=SAMPLE_RATE, norm=None, mel_scale="kaldi",
                                                           triangularize_in_mel_space=True)).to(torch.float64)
    return basis, fb


class KaldiFbank:
    """Waveforms [B, L] on the device -> Wav2Vec2-BERT's `input_features` [B, F // 2, 160], F = 1 + (L - 400) // 160: the device form of
    SeamlessM4TFeatureExtractor (which runs in numpy, one Python iteration per frame).  Four launches for the whole batch: the framing +
    DFT GEMM over overlapping rows (lda = 160, no frame matrix), dyn_stft_power, the mel GEMM, dyn_fbank_finish (floor, log, per-bin
    normalisation over the valid frames, two frames per row).  `valid` (device int32 scalar): the utterance's own frame count inside a
    zero-padded length bucket; its rows equal the unpadded call's (a frame never reads past its own 400 samples) and the rows past them
    are zeros.  The features do not depend on the waveform's gain except through the mel floor (log of a scaled energy moves every frame
    of a bin by the same constant, which the per-bin mean removes)."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        basis, fb = kaldi_fbank_matrices()
        self.basis = basis.float().to(self.device).contiguous()                # [400, 520]
        self.fb = fb.float().to(self.device).contiguous()                      # [260, 80]

    def __call__(self, x, valid=None):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()):
            raise ops.DynError("KaldiFbank: expected a contiguous float32 CUDA tensor [B, L]")
        B, L = x.shape
        F, T = kaldi_fbank_frames(L)
        if T < 1:
            raise ops.DynError(f"KaldiFbank: {L} samples give {F} filter-bank frame(s); two are needed ({WIN + HOP} samples): the unbiased "
                               "per-bin variance of one frame is undefined")
        st = torch.cuda.current_stream().cuda_stream
        reim = torch.empty(B, F, 2 * KP, device=self.device, dtype=torch.float32)
        ops.gemm(x, self.basis, reim, M=F, N=2 * KP, K=WIN, lda=HOP, ldb=2 * KP, ldc=2 * KP, nb1=B, sa=(L, 0), sc=(F * 2 * KP, 0))
        power = torch.empty(B * F, KP, device=self.device, dtype=torch.float32)
        check(load().dyn_stft_power(reim.data_ptr(), power.data_ptr(), B * F, KP, st), "dyn_stft_power")
        mel = torch.empty(B, F, N_MELS, device=self.device, dtype=torch.float32)
        ops.gemm(power, self.fb, mel, M=B * F, N=N_MELS, K=KP, lda=KP, ldb=N_MELS, ldc=N_MELS)
        return ops.fbank_finish(mel, valid)


# ------------------------------------------------------------------------------------------ FastConformer family: waveform -> input_features
# What differs between transformers' four extractor classes (feature_extraction_parakeet.py, _nemotron_asr_streaming.py, _cohere_asr.py,
# _lasr.py).  `offset`: where the 400-tap window sits in the 512-point frame (torch.stft centres it; LASR's unfold + rfft(n=512) does not);
# `guard` / `clamp`: log(mel + guard) or log(max(mel, guard)).
MEL_KINDS = {
    "parakeet": dict(preemphasis=0.97, normalize=True, guard=2.0 ** -24, clamp=False, offset=56, centred=True, dither=0.0, feature_size=80),
    "nemotron_asr_streaming": dict(preemphasis=0.97, normalize=False, guard=2.0 ** -24, clamp=False, offset=56, centred=True, dither=0.0,
                                   feature_size=128),
    "cohere_asr": dict(preemphasis=0.97, normalize=True, guard=2.0 ** -24, clamp=False, offset=56, centred=True, dither=1e-5, feature_size=128),
    "lasr": dict(preemphasis=0.0, normalize=False, guard=1e-5, clamp=True, offset=0, centred=False, dither=0.0, feature_size=128),
}
MEL_KIND_OF_CLASS = {"ParakeetFeatureExtractor": "parakeet", "NemotronAsrStreamingFeatureExtractor": "nemotron_asr_streaming",
                     "CohereAsrFeatureExtractor": "cohere_asr", "LasrFeatureExtractor": "lasr"}
MEL_NORM_EPS = 1e-5                        # the extractors' EPSILON: (x - mean) / (std + 1e-5)
COHERE_MAX_SECONDS = 30.0                  # max_audio_clip_s - overlap_chunk_second: longer rows take the extractor's energy-based splitting
LASR_MEL_HZ = (125.0, 7500.0)


def mel_frames(kind, n_samples, center=True):
    """Valid feature frames of a row of n_samples samples, the extractor's `attention_mask.sum(1)`: L // 160 with centring (the frame
    centred past the last whole hop is masked), (L - 512) // 160 + 1 with center=False, 1 + (L - 400) // 160 for LASR; never negative."""
    L = int(n_samples)
    if kind == "lasr":
        return max(0, 1 + (L - WIN) // HOP) if L >= WIN else 0
    if center:
        return L // HOP
    return (L - N_FFT) // HOP + 1 if L >= N_FFT else 0


def mel_output_frames(kind, n_samples, center=True):
    """Frames of the extractor's output for a batch padded to n_samples: 1 + L // 160 when centred."""
    L = int(n_samples)
    if kind == "lasr":
        return 1 + (L - WIN) // HOP if L >= WIN else 0
    if center:
        return 1 + L // HOP
    return (L - N_FFT) // HOP + 1 if L >= N_FFT else 0


def mel_filters(kind, feature_size):
    """[257, F] float64 holding the float32 filter values.  The three librosa classes: transformers.audio_utils.mel_filter_bank(slaney,
    slaney norm, 0 - 8000 Hz) rounded to float32, the call the extractors' own TODO names as their intended replacement (librosa's float32
    filters differ from it in the last bits; librosa is not a dependency here).  LASR: its own linear_to_mel_weight_matrix (float64)."""
    F = int(feature_size)
    if kind == "lasr":
        from transformers.models.lasr.feature_extraction_lasr import linear_to_mel_weight_matrix
        import numpy as np
        return torch.from_numpy(linear_to_mel_weight_matrix(num_mel_bins=F, num_spectrogram_bins=N_FFT // 2 + 1, sample_rate=SAMPLE_RATE,
                                                            lower_edge_hertz=LASR_MEL_HZ[0], upper_edge_hertz=LASR_MEL_HZ[1],
                                                            dtype=np.float64)).to(torch.float64)
    from transformers.audio_utils import mel_filter_bank
    fb = mel_filter_bank(N_FFT // 2 + 1, F, 0.0, SAMPLE_RATE / 2, SAMPLE_RATE, norm="slaney", mel_scale="slaney")
    return torch.from_numpy(fb).to(torch.float32).to(torch.float64)


def mel_basis(offset):
    """[400, 2 * 260] float64: Hann(400, periodic=False) times the 512-point DFT's cos | -sin at sample n + offset of the frame."""
    n = torch.arange(WIN, dtype=torch.float64)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / (WIN - 1))                   # torch.hann_window(400, periodic=False)
    k = torch.arange(N_FFT // 2 + 1, dtype=torch.float64)
    ang = 2 * math.pi * k[None, :] * (n[:, None] + offset) / N_FFT
    basis = torch.zeros(WIN, 2 * KP, dtype=torch.float64)
    basis[:, :N_FFT // 2 + 1] = w[:, None] * torch.cos(ang)
    basis[:, KP:KP + N_FFT // 2 + 1] = -w[:, None] * torch.sin(ang)
    return basis


def cohere_dither_noise(lengths, Lmax):
    """[B, Lmax] float32 on the host: CohereAsrFeatureExtractor._apply_dither's noise, row b = randn(L_b) from a CPU generator seeded with
    L_b (so a row's dither does not depend on the batch it sits in), zeros past L_b."""
    noise = torch.zeros(len(lengths), int(Lmax), dtype=torch.float32)
    g = torch.Generator(device="cpu")
    for b, L in enumerate(lengths):
        L = min(int(L), int(Lmax))
        if L > 0:
            g.manual_seed(L)
            noise[b, :L] = torch.randn(L, dtype=torch.float32, generator=g)
    return noise


def stream_samples_for_frames(n_frames):
    """Samples of a stream that must have arrived before its first n_frames centred feature frames can be extracted: frame t reads the
    samples below 160 t + 200 (the 400-tap window around sample 160 t)."""
    n = int(n_frames)
    return 0 if n <= 0 else HOP * (n - 1) + WIN // 2


def stream_frames_ready(n_samples):
    """Centred feature frames whose window support lies inside the first n_samples samples."""
    S = int(n_samples)
    return 0 if S < WIN // 2 else (S - WIN // 2) // HOP + 1


def stream_samples_for_chunk(k, first_chunk_frames, chunk_frames):
    """Samples that complete chunk k (0-based) of a streaming session: first_chunk_frames, then chunk_frames feature frames a chunk."""
    return stream_samples_for_frames(int(first_chunk_frames) + int(k) * int(chunk_frames))


class MelFeatures:
    """Waveforms [B, Lmax] on the device -> the family's `input_features` [B, T, F] (or the loops' `spec` [B, F, T]) and the valid frames per
    row: the device form of transformers' four extractor classes (`kind`, MEL_KINDS).  Five entry calls for the whole batch (nine kernels where the mode normalises: dyn_melfeat_finish launches five): dyn_melfeat_prep
    (dither, pre-emphasis over the whole signal, the length mask, `center=True`'s zero padding), the framing + DFT GEMM over overlapping
    rows (lda = 160, no frame matrix), dyn_stft_power, the mel GEMM, dyn_melfeat_finish (log, per-row per-bin normalisation over the valid
    frames, zeros past them).  `overrides`: sampling_rate, n_fft, win_length, hop_length (anything but 16000 / 512 / 400 / 160 is refused),
    preemphasis, dither."""

    def __init__(self, kind, feature_size=None, device="cuda:0", **overrides):
        if kind not in MEL_KINDS:
            raise ops.DynError(f"MelFeatures: kind={kind!r} is not built: one of {sorted(MEL_KINDS)}")
        k = dict(MEL_KINDS[kind])
        for name, want in (("sampling_rate", SAMPLE_RATE), ("n_fft", N_FFT), ("win_length", WIN), ("hop_length", HOP)):
            got = overrides.pop(name, want)
            if got != want:
                raise ops.DynError(f"MelFeatures: {name}={got!r} is not built ({want}; resampling and other frame geometries are out of scope)")
        for name in ("preemphasis", "dither"):
            v = overrides.pop(name, None)
            if v is not None:
                k[name] = float(v)
        if overrides:
            raise ops.DynError(f"MelFeatures: unknown option(s) {sorted(overrides)}")
        if kind == "lasr" and k["preemphasis"] != 0.0:
            raise ops.DynError("MelFeatures: LasrFeatureExtractor has no pre-emphasis")
        if not (0.0 <= k["preemphasis"] < 1.0 and k["dither"] >= 0.0):
            raise ops.DynError(f"MelFeatures: preemphasis={k['preemphasis']!r} must lie in [0, 1), dither={k['dither']!r} must not be negative")
        if k["dither"] > 0.0 and kind != "cohere_asr":
            raise ops.DynError(f"MelFeatures: dither is CohereAsrFeatureExtractor's; kind={kind!r} has none")
        F = k["feature_size"] if feature_size is None else feature_size
        if isinstance(F, bool) or not isinstance(F, int) or F < 4 or F > 256 or F % 4:
            raise ops.DynError(f"MelFeatures: feature_size={F!r} is not built: a multiple of 4 in 4 .. 256")
        self.kind, self.feature_size, self.device = kind, F, torch.device(device)
        self.preemphasis, self.dither, self.normalize = k["preemphasis"], k["dither"], k["normalize"]
        self.guard, self.clamp, self.offset, self.centred = k["guard"], k["clamp"], k["offset"], k["centred"]
        self.basis = mel_basis(self.offset).float().to(self.device).contiguous()     # [400, 520]
        fb = torch.zeros(KP, F, dtype=torch.float64)
        fb[:N_FFT // 2 + 1] = mel_filters(kind, F)
        self.fb = fb.float().to(self.device).contiguous()                            # [260, F]

    @classmethod
    def from_preprocessor_config(cls, path_or_dict, device="cuda:0"):
        """A checkpoint's `preprocessor_config.json` (path or dict): `feature_extractor_type` names the class, the geometry fields are
        checked, `feature_size`, `preemphasis` and `dither` are taken."""
        src = path_or_dict
        if not isinstance(src, dict):
            import json
            with open(src) as f:
                src = json.load(f)
            if not isinstance(src, dict):
                raise ops.DynError(f"{path_or_dict}: expected a JSON object")
        name = src.get("feature_extractor_type")
        if name not in MEL_KIND_OF_CLASS:
            raise ops.DynError(f"preprocessor config: feature_extractor_type={name!r} is not built: one of {sorted(MEL_KIND_OF_CLASS)}")
        kind = MEL_KIND_OF_CLASS[name]
        kw = {k: src[k] for k in ("sampling_rate", "n_fft", "win_length", "hop_length", "dither") if src.get(k) is not None}
        if kind != "lasr" and "preemphasis" in src:
            kw["preemphasis"] = 0.0 if src["preemphasis"] is None else src["preemphasis"]
        if kind != "cohere_asr":
            kw.pop("dither", None)
        return cls(kind, src.get("feature_size"), device, **kw)

    # ------------------------------------------------------------------ host checks
    def check_audio_lengths(self, audio_lengths, B, Lmax, center=True):
        """(sample counts, valid frames) per row as host lists; everything that is not built is refused by name here, before any launch."""
        v = audio_lengths
        if v is None:
            v = [Lmax] * B
        elif isinstance(v, torch.Tensor):
            if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool or v.dim() != 1:
                raise ops.DynError("audio_lengths must be a sequence of ints or an integer tensor [B]")
            v = v.tolist()                                                     # the one host copy
        elif isinstance(v, (list, tuple)) and all(isinstance(n, int) and not isinstance(n, bool) for n in v):
            v = list(v)
        else:
            raise ops.DynError("audio_lengths must be a sequence of ints or an integer tensor [B]")
        if len(v) != B:
            raise ops.DynError(f"audio_lengths holds {len(v)} counts for a batch of {B} rows")
        if not all(0 <= n <= Lmax for n in v):
            raise ops.DynError(f"audio_lengths={v} must lie in 0 .. Lmax = {Lmax}, the samples of waveforms")
        if not center and self.kind != "nemotron_asr_streaming":
            raise ops.DynError(f"center=False is NemotronAsrStreamingFeatureExtractor's; kind={self.kind!r} has no such mode")
        frames = [mel_frames(self.kind, n, center) for n in v]
        need = 2 if self.normalize else 1
        for b, (n, f) in enumerate(zip(v, frames)):
            if f < 1:
                raise ops.DynError(f"row {b}: {n} samples give no valid feature frame")
            if f < need:
                raise ops.DynError(f"row {b}: {n} samples give {f} valid feature frame; the per-bin normalisation needs two (320 samples): the "
                                   "unbiased variance of one frame is undefined")
            if self.kind == "cohere_asr" and n > COHERE_MAX_SECONDS * SAMPLE_RATE:
                raise ops.DynError(f"row {b}: {n / SAMPLE_RATE:.2f} s of audio; CohereAsrFeatureExtractor splits rows longer than "
                                   f"{COHERE_MAX_SECONDS:.0f} s at energy-based boundaries, which is not built: split the recording first")
        return v, frames

    # ------------------------------------------------------------------ the launches
    def _features(self, x, lens_dev, frames_dev, T, pad, a_off, layout, normalize, noise=None, prev=None, right=0):
        """x [B, Lmax] -> [B, T, F] | [B, F, T].  Frame t reads the prepared signal at t * 160 + a_off .. + 400; `pad` zeros stand in front of
        sample 0, and the row is long enough for every frame (`right`: zeros wanted behind sample Lmax - 1)."""
        B, Lmax = x.shape
        F = self.feature_size
        need = (T - 1) * HOP + a_off + WIN
        W = (max(pad + Lmax + right, need) + 3) // 4 * 4                       # rows start 16-byte aligned
        st = torch.cuda.current_stream().cuda_stream
        sig = torch.empty(B, W, device=self.device, dtype=torch.float32)
        ops.melfeat_prep(x, lens_dev, sig, pad, self.preemphasis, noise=noise, dither=self.dither, prev=prev)
        reim = torch.empty(B, T, 2 * KP, device=self.device, dtype=torch.float32)
        ops.gemm(sig, self.basis, reim, M=T, N=2 * KP, K=WIN, lda=HOP, ldb=2 * KP, ldc=2 * KP, nb1=B, sa=(W, 0), sc=(T * 2 * KP, 0), a_off=a_off)
        power = torch.empty(B * T, KP, device=self.device, dtype=torch.float32)
        check(load().dyn_stft_power(reim.data_ptr(), power.data_ptr(), B * T, KP, st), "dyn_stft_power")
        mel = torch.empty(B, T, F, device=self.device, dtype=torch.float32)
        ops.gemm(power, self.fb, mel, M=B * T, N=F, K=KP, lda=KP, ldb=F, ldc=F)
        return ops.melfeat_finish(mel, frames_dev, self.guard, self.clamp, normalize, MEL_NORM_EPS, layout)

    def __call__(self, waveforms, audio_lengths=None, center=True, layout="tf"):
        """waveforms: contiguous float32 device tensor [B, Lmax]; audio_lengths: the valid samples per row (None: all) ->
        (input_features [B, T, F] (layout "tf") or [B, F, T] ("ft"), input_lengths: the valid frames per row, a list of ints).
        T is the extractor's: 1 + Lmax // 160 when centred.  Frames past a row's count are exact zeros; samples past a row's length are
        never read."""
        x = waveforms
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.shape[1] >= 1):
            raise ops.DynError("MelFeatures: waveforms must be a contiguous float32 CUDA tensor [B, Lmax]")
        if layout not in ("tf", "ft"):
            raise ops.DynError(f"MelFeatures: layout={layout!r} must be \"tf\" ([B, T, F]) or \"ft\" ([B, F, T])")
        B, Lmax = x.shape
        lens, frames = self.check_audio_lengths(audio_lengths, B, Lmax, center)
        T = mel_output_frames(self.kind, Lmax, center)
        rows = torch.zeros(2, (B + 3) // 4 * 4, dtype=torch.int32)
        rows[0, :B], rows[1, :B] = torch.tensor(lens, dtype=torch.int32), torch.tensor(frames, dtype=torch.int32)
        rows = rows.to(self.device, non_blocking=True)
        noise = cohere_dither_noise(lens, Lmax).to(self.device) if self.dither > 0.0 else None
        pad = N_FFT // 2 if (self.centred and center) else 0
        out = self._features(x, rows[0, :B], rows[1, :B], T, pad, self.offset, layout, self.normalize, noise=noise, right=pad)
        return out, frames


class MelStream:
    """The audio side of a streaming session (nemotron_asr_streaming_stream.StreamSession.push_audio): B streams advancing together, any
    number of samples a call.  Owns the audio tail (the samples a later frame still reads) and the sample before it per row, both on the
    device.  Centred frame t is extracted once the samples below 160 t + 200 have arrived and equals frame t of one offline pass over the
    whole stream: the pre-emphasis is carried across calls by the previous sample, the 256 zeros of `center=True` stand in front of sample 0
    only.  finish() ends the stream: the frames below total // 160 that are still missing, read with zeros behind the last sample."""

    def __init__(self, fe, batch_size):
        if fe.normalize or not fe.centred:
            raise ops.DynError(f"MelStream: kind={fe.kind!r} is not built for streaming (a per-utterance normalisation needs the whole stream)")
        self.fe, self.B = fe, int(batch_size)
        self.prev = torch.zeros(self.B, device=fe.device, dtype=torch.float32)
        self.reset()

    def reset(self):
        self.tail = torch.zeros(self.B, 0, device=self.fe.device, dtype=torch.float32)
        self.start, self.total, self.next_frame = 0, 0, 0                      # absolute sample of tail[:, 0]; samples seen; frames extracted
        self.prev.zero_()

    def _extract(self, upto, final):
        """Frames next_frame .. upto - 1 from the tail -> [B, n, F] (None: nothing new), then the tail is cut to what frame `upto` needs."""
        t0, n = self.next_frame, upto - self.next_frame
        if n <= 0:
            return None
        fe, raw = self.fe, self.tail
        m = raw.shape[1]
        pad = N_FFT // 2 if self.start == 0 else 0
        a_off = HOP * t0 - WIN // 2 - self.start + pad
        lens = torch.full((self.B,), m, device=fe.device, dtype=torch.int32)
        frames = torch.full((self.B,), n, device=fe.device, dtype=torch.int32)
        out = fe._features(raw, lens, frames, n, pad, a_off, "tf", False, prev=self.prev if self.start > 0 else None,
                           right=N_FFT // 2 if final else 0)
        self.next_frame = upto
        keep = HOP * upto - WIN // 2                                            # the first sample frame `upto` reads
        if keep > self.start and not final:
            self.prev = raw[:, keep - self.start - 1].clone()
            self.tail, self.start = raw[:, keep - self.start:].contiguous(), keep
        return out

    def push(self, samples):
        if not (isinstance(samples, torch.Tensor) and samples.is_cuda and samples.dtype == torch.float32 and samples.dim() == 2
                and samples.shape[0] == self.B):
            raise ops.DynError(f"push_audio: samples must be a float32 CUDA tensor [{self.B}, n]")
        if samples.shape[1] == 0:
            return None
        self.tail = torch.cat([self.tail, samples], dim=1).contiguous()
        self.total += samples.shape[1]
        return self._extract(stream_frames_ready(self.total), False)

    def finish(self):
        return self._extract(self.total // HOP, True) if self.tail.shape[1] else None


def processing_chain(waveform, device="cuda:0"):
    """Same role as upstream `lcasr.utils.audio_tools.processing_chain`: waveform -> normalised log-mel [1, 80, T]."""
    return LogMel(device)(waveform)


def total_frames(seconds):
    """Seconds -> spectrogram frames (upstream `audio_tools.total_frames`; 100 frames / s, DEFINED here as int(s * 100))."""
    return int(float(seconds) * 100)


def zero_out_spectogram(spec, remove_timings):
    """TEDLIUM `ignore_time_segment_in_scoring` segments are blanked before eval (reference lcasr/tedlium/run.py:91-96 calls
    the un-vendored `lcasr.eval.utils.zero_out_spectogram`; rule DEFINED here: spec[:, :, frames(start):frames(end)] = 0).
    spec: CUDA [1, F, T], modified in place by the time-mask kernel (segments travel as kernel arguments)."""
    import ctypes
    F, T = spec.shape[-2], spec.shape[-1]
    if spec.dim() != 3 or spec.shape[0] != 1 or not spec.is_cuda or not spec.is_contiguous():
        raise ops.DynError("zero_out_spectogram expects a contiguous CUDA [1, F, T] spectrogram")
    st, wd = [], []
    for seg in remove_timings:
        a, b = min(total_frames(seg['start']), T), min(total_frames(seg['end']), T)
        if b > a:
            st.append(a); wd.append(b - a)
    for i in range(0, len(st), 32):
        a = (ctypes.c_int32 * len(st[i:i + 32]))(*st[i:i + 32])
        b = (ctypes.c_int32 * len(wd[i:i + 32]))(*wd[i:i + 32])
        check(load().dyn_specaug_mask_args(spec.data_ptr(), F, T, ctypes.addressof(a), ctypes.addressof(b), len(a), 1, 0.0, 0,
                                           torch.cuda.current_stream().cuda_stream), "dyn_specaug_mask_args")
    return spec


def combine_channels(waveforms, stime, etime, device="cuda:0"):
    """CHiME-6 array combination (reference lcasr/chime6/run.py:46-70): every channel -> un-normalised log-mel, right-padded
    to the longest channel, trimmed to [frames(stime), frames(etime)), averaged over channels, renormalised per bin
    ((x - mean) / unbiased std over time).  -> CUDA [1, 80, T']"""
    fe = LogMel(device, normalize=False)
    n = max(int(torch.as_tensor(w).numel()) for w in waveforms)
    a, b = total_frames(stime), total_frames(etime)
    acc = None
    for w in waveforms:
        x = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        if x.numel() < n:
            x = torch.nn.functional.pad(x, (0, n - x.numel()))
        spec = fe(x)[:, :, a:b].contiguous()
        if acc is None:
            acc = torch.zeros_like(spec)
        ops.axpby(spec, acc, a=1.0 / len(waveforms), b=1.0)
    check(load().dyn_rownorm(acc.data_ptr(), acc.data_ptr(), acc.shape[1], acc.shape[2], torch.cuda.current_stream().cuda_stream),
          "dyn_rownorm")
    return acc
