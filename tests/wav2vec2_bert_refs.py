"""References shared by the Wav2Vec2-BERT tests: transformers' SeamlessM4TFeatureExtractor itself, and its per-frame formula restated in
float64 numpy.

Why both.  audio_utils.spectrogram works on a float64 buffer per frame but STORES every frame's spectrum as complex64 and returns float32,
and the extractor normalises that float32 array in float32: its features are 8e-6 .. 2e-5 away from its own formula evaluated in float64
(measured: L = 560 .. 48 000, printed by the tests).  A bound tighter than that against the extractor's output says nothing about the code
under test.  fbank_formula_f64 is the same statement sequence (same window and mel filters, taken from the extractor object) without the
float32 stores.  The tests tie it to the real extractor first: the extractor's output must lie within extractor_bound of it, a bound
worked out from the float32 roundings the extractor performs, not from what was measured.  The code under test is then held to the
formula at its own bound, and so to the extractor at the sum of the two."""
import numpy as np
import torch

MEL_FLOOR = 1.192092955078125e-07
_FE = None


def extractor():
    global _FE
    if _FE is None:
        from transformers import SeamlessM4TFeatureExtractor
        _FE = SeamlessM4TFeatureExtractor()
    return _FE


def extractor_rows(x):
    """(input_features [rows, 160] float32, number of valid rows) for one float32 waveform tensor [L]."""
    out = extractor()(x.numpy(), sampling_rate=16000, return_tensors="np")
    return out["input_features"][0], int(out["attention_mask"][0].sum())


def _log_mel_f64(x):
    """[F, 80] float64 log-mel energies: feature_extraction_seamless_m4t.py / audio_utils.spectrogram, statement by statement, in float64."""
    fe = extractor()
    xs = x.numpy().astype(np.float64) * 2 ** 15                                # `np.squeeze(waveform) * (2**15)`
    F = 1 + (xs.shape[0] - 400) // 160
    rows = []
    for f in range(F):
        buf = np.zeros(512)
        buf[:400] = xs[f * 160:f * 160 + 400]
        buf[:400] -= buf[:400].mean()                                          # remove_dc_offset
        buf[1:400] -= 0.97 * buf[:399]                                         # preemphasis
        buf[0] *= 1 - 0.97
        buf[:400] *= fe.window
        spec = np.abs(np.fft.rfft(buf)) ** 2.0
        rows.append(np.log(np.maximum(MEL_FLOOR, fe.mel_filters.T @ spec)))
    return np.stack(rows)


def fbank_formula_f64(x):
    """[F // 2, 160] float64: the extractor's formula in float64 throughout (log-mel, `do_normalize_per_mel_bins`, two frames per row)."""
    r = _log_mel_f64(x)
    n = (r - r.mean(0)) / np.sqrt(r.var(0, ddof=1) + 1e-7)
    T = r.shape[0] // 2
    return n[:2 * T].reshape(T, 160)


EXTRACTOR_ULPS = 8


def extractor_bound(x):
    """[F // 2, 160]: how far the extractor's float32 output may sit from fbank_formula_f64, element by element.  The extractor holds the
    log-mel energies (magnitude up to 32) as float32 and forms mean, x - mean, the variance and the quotient in float32: each is a
    rounding of half an ulp of the log-mel scale or less (store, mean, difference) or of the O(1) result (variance, quotient), 2 - 3 ulp
    of the log-mel scale in x - mean in all, which the division by the bin's standard deviation carries into the feature.  Allowed:
    EXTRACTOR_ULPS = 8 such ulp over the bin's standard deviation (a margin of about 3 over that count), plus 8 ulp of the feature itself.
    The complex64 spectrum adds 1e-7 to a log energy: inside the first rounding."""
    r = _log_mel_f64(x)
    ulp = np.spacing(np.float32(np.abs(r).max())).astype(np.float64)
    std = np.sqrt(r.var(0, ddof=1) + 1e-7)
    n = np.abs((r - r.mean(0)) / std)
    b = EXTRACTOR_ULPS * ulp / std[None, :] + EXTRACTOR_ULPS * 2.0 ** -23 * np.maximum(n, 1.0)
    T = r.shape[0] // 2
    return b[:2 * T].reshape(T, 160)


def fbank_chain(x, basis, fb, dtype):
    """The device chain (folded basis GEMM over strided frames, power, mel GEMM, floor, log, per-bin normalisation, stacking) in torch on the
    CPU at `dtype`: float64 for the identity, float32 for the error a float32 implementation of this chain has."""
    KP = fb.shape[0]
    frames = x.to(dtype).unfold(0, 400, 160)
    reim = frames @ basis.to(dtype)
    mel = (reim[:, :KP] ** 2 + reim[:, KP:] ** 2) @ fb.to(dtype)
    logm = torch.log(torch.clamp(mel, min=MEL_FLOOR))
    n = (logm - logm.mean(0)) / torch.sqrt(logm.var(0, unbiased=True) + 1e-7)
    T = frames.shape[0] // 2
    return n[:2 * T].reshape(T, 160)
