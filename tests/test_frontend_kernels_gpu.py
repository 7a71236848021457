"""Float64 parity of the kernels around the model that only `LogMel(...)` and one-shape augmentation tests used to reach: the log-mel
front end (csrc/logmel.hip), the window augmentations (csrc/augment.hip), the SpecAugment masks and the window transpose
(csrc/elementwise.hip, csrc/specaug_args.hip), called through the C-ABI so no GEMM stands between the input and the kernel.  The
references are tests/kernel_refs.py (held to torch's ops in tests/test_kernel_refs_cpu.py).

Tolerances.  Copies, gathers, fills and masks are bit-exact, with a sentinel after every output.  Arithmetic results are MEASURED
(kernel_refs.measured_tol): 4 x the error of torch's fp32 CPU result of the same op on the same inputs against float64, plus the floor
named at the call.  Every check prints `name: kernel error | torch fp32 error | bound` before it asserts (pytest -s shows them).
The normalised log-mel is checked in log-mel units (|out - ref| * std of the bin, the metric of tests/test_frontend_gpu.py) and by the
property no reference is needed for: every bin of the output has mean 0 and unbiased std 1.  tests/test_kernel_refs_cpu.py shows that the
statistics dyn_logmel_finish formed before they were centred (var = (q - s * mean) / (T - 1) from fp32 sums) miss both bounds."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -12345.678
TAIL = 64
E_ARG, E_WORKSPACE = -1, -3                      # DYN_E_ARG, DYN_E_WORKSPACE of include/dyneval.h


def _L():
    from dynamic_asr_eval_amd import _lib
    return _lib.load()


def _ok(rc, what):
    from dynamic_asr_eval_amd._lib import check
    check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(name, got, want, tol, e32=None, rel=False):
    err = K.max_err(got, want, rel)
    print(f"  {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")
    assert err <= tol, f"{name}: {'rel' if rel else 'abs'} err {err} > {tol} (torch fp32: {e32})"


def _measured(name, got, torch32, want, floor, rel=False):
    tol, e32 = K.measured_tol(torch32, want, floor, rel)
    _check(name, got, want, tol, e32, rel)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guarded(cuda, n):
    """A device buffer of n floats followed by TAIL sentinels; returns (whole buffer, its first n elements)."""
    buf = torch.full((n + TAIL,), SENTINEL, device=cuda, dtype=torch.float32)
    return buf, buf[:n]


def _tail_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all().item())


# ----------------------------------------------------------------------------------------------------------- dyn_reflect_pad
@pytest.mark.parametrize("n,pad", [(2, 1), (257, 256), (800, 256), (16123, 256), (1_050_000, 256), (1000, 0)])
def test_reflect_pad(cuda, n, pad):
    """Bit-exact; (257, 256) is pad = n - 1, the shortest waveform LogMel accepts; 1 050 512 outputs pass the 4096 x 256 grid cap (the stride
    loop runs); pad = 0 is a copy."""
    x = torch.randn(n, generator=K.gen(n + pad))
    buf, out = _guarded(cuda, n + 2 * pad)
    _ok(_L().dyn_reflect_pad(x.to(cuda).data_ptr(), out.data_ptr(), n, pad, _stream()), "dyn_reflect_pad")
    assert _bits_equal(out, K.reflect_pad_ref(x, pad)) and _tail_intact(buf, n + 2 * pad)
    if pad == 0:
        assert _bits_equal(out, x)


@pytest.mark.parametrize("n,pad", [(5, 5), (5, 9), (1, 0), (1, 1)])
def test_reflect_pad_rejects_pad_past_the_signal(cuda, n, pad):
    x = torch.randn(8, generator=K.gen(1)).to(cuda)
    buf, out = _guarded(cuda, n + 2 * pad)
    assert _L().dyn_reflect_pad(x.data_ptr(), out.data_ptr(), n, pad, _stream()) == E_ARG
    torch.cuda.synchronize()
    assert _tail_intact(buf, 0), "an error code must come without a launch"


# ----------------------------------------------------------------------------------------------------------- dyn_stft_power
@pytest.mark.parametrize("T,KP", [(1, 260), (7, 4), (8200, 260)])
def test_stft_power(cuda, T, KP):
    """re^2 + im^2, relative to float64 (floor 0); 8200 x 260 outputs pass the 8192 x 256 grid cap."""
    reim = torch.randn(T, 2 * KP, generator=K.gen(T + KP)) * torch.logspace(-3, 2, 2 * KP)[None, :]
    buf, out = _guarded(cuda, T * KP)
    _ok(_L().dyn_stft_power(reim.to(cuda).data_ptr(), out.data_ptr(), T, KP, _stream()), "dyn_stft_power")
    _measured("power (rel)", out.view(T, KP), reim[:, :KP] * reim[:, :KP] + reim[:, KP:] * reim[:, KP:], K.stft_power_ref(reim, KP), 0.0, rel=True)
    assert _tail_intact(buf, T * KP), "written past T * KP"


# ----------------------------------------------------------------------------------------------------------- dyn_logmel_finish
def _logmel_finish(cuda, mel, normalize, slack=0):
    """dyn_logmel_finish on a copy of mel [T, F] with a workspace of exactly dyn_logmel_finish_workspace_bytes (+ a sentinel tail).
    Returns (out [F, T], the log left in mel [T, F]) on the device."""
    L = _L()
    T, Fq = mel.shape
    need = L.dyn_logmel_finish_workspace_bytes(T, Fq)
    ws = torch.full((need + 256,), 0x5A, device=cuda, dtype=torch.uint8)
    md = mel.to(cuda).contiguous()
    buf, out = _guarded(cuda, T * Fq)
    _ok(L.dyn_logmel_finish(md.data_ptr(), out.data_ptr(), T, Fq, K.LOGMEL_EPS, int(normalize), ws.data_ptr(), need + slack, _stream()),
        "dyn_logmel_finish")
    assert _tail_intact(buf, T * Fq), "written past out"
    assert bool((ws[need:] == 0x5A).all().item()), "written past dyn_logmel_finish_workspace_bytes"
    return out.view(Fq, T), md


def _log_uniform_mel(T, Fq):
    """mel log-uniform in [1e-9, 1e3], with exact zeros."""
    g = K.gen(9000 + 7 * T + Fq)
    mel = torch.exp(torch.rand(T, Fq, generator=g, dtype=F64) * (6.907755 + 20.723266) - 20.723266)
    mel[torch.rand(T, Fq, generator=g) < 0.05] = 0.0
    mel.view(-1)[0] = 0.0
    return mel.float()


@pytest.mark.parametrize("Fq", [1, 33, 80, 128, 256])
def test_logmel_finish_unnormalised(cuda, Fq):
    """log(mel + eps) -> [F, T] and the log left in mel, at the ragged edges of the 32 x 32 transpose tile and of the 256-row moment block."""
    for T in (1, 2, 31, 32, 33, 255, 256, 257, 513):
        mel = _log_uniform_mel(T, Fq)
        out, left = _logmel_finish(cuda, mel, False)
        ref = K.logmel_finish_ref(mel, K.LOGMEL_EPS, False)
        t32 = K.logmel_torch_fp32(mel, K.LOGMEL_EPS, False)
        _measured(f"F={Fq} T={T} out", out, t32, ref, 2e-6)
        _measured(f"F={Fq} T={T} log left in mel", left, t32.t(), ref.t(), 2e-6)
        assert _bits_equal(out, left.t()), "out must be the transpose of the log left in mel"


def test_logmel_finish_rejects_a_small_workspace_and_wide_windows(cuda):
    L = _L()
    T, Fq = 300, 80
    need = L.dyn_logmel_finish_workspace_bytes(T, Fq)
    assert need >= (-(-T // 256) * 2 * Fq) * 4 + 2 * Fq * 4
    mel = torch.ones(T, 257, device=cuda)
    keep = mel.clone()
    buf, out = _guarded(cuda, T * 257)
    ws = torch.empty(1 << 20, device=cuda, dtype=torch.uint8)
    assert L.dyn_logmel_finish(mel.data_ptr(), out.data_ptr(), T, Fq, K.LOGMEL_EPS, 1, ws.data_ptr(), need - 1, _stream()) == E_WORKSPACE
    assert L.dyn_logmel_finish(mel.data_ptr(), out.data_ptr(), T, 257, K.LOGMEL_EPS, 1, ws.data_ptr(), ws.numel(), _stream()) == E_ARG
    torch.cuda.synchronize()
    assert torch.equal(mel, keep) and _tail_intact(buf, 0), "an error code must come without a launch"


@pytest.mark.parametrize("T", K.LOGMEL_NORM_T)
def test_logmel_finish_normalised(cuda, T):
    """Bins cycling through (mu, sd) of log(mel + eps) from (-13.8, 1e-3) — an empty band, at log(1e-6) — to (+4, 1), one bin all zeros.
    Measured on the MI355X (kernel | torch fp32 | bound), the T of the largest kernel figure: out in log-mel units 1.6e-06 | 2.3e-06 | 1.1e-05
    (T = 60001); per-bin |mean| 3.1e-07 | 1.7e-03 | 6.8e-03 (T = 101); per-bin |std - 1| 7.2e-08 | 5.5e-08 | 1.0e-05 (T = 101).  With the
    uncentred statistics this kernel had before (var = (q - s * mean) / (T - 1) from fp32 sums, var <= 0 replaced by 1) the same checks
    measured 3.4e-03 to 2.0e-02 log units and |std - 1| = 1.0 at every T (7 to 11 of the 39 bins at log(1e-6) left un-normalised, the others
    divided by 0.58 to 3.7 x their std), and the all-zero bin came out up to 1.1e-03 from 0."""
    mel = K.logmel_class_inputs(T)
    bd = K.logmel_norm_bounds(mel)
    out, _ = _logmel_finish(cuda, mel, True)
    again, _ = _logmel_finish(cuda, mel, True, slack=128)
    assert _bits_equal(out, again), "two calls must be bit-identical"
    assert torch.isfinite(out).all(), "nan / inf in the normalised output"
    assert torch.equal(out[K.LOGMEL_ZERO_COLUMN].cpu(), torch.zeros(T)), "a bin of zero variance must come out as zeros"
    assert bd["live"] == [f for f in range(80) if f != K.LOGMEL_ZERO_COLUMN]
    worst = ((K.d(out) - bd["ref"]).abs() * bd["std"]).amax(1)
    print(f"  T={T}: per-class worst error in log-mel units {[float(worst[c::6].max()) for c in range(6)]}")
    got_m, got_s = K.unit_stats_err(out, bd["live"])
    print(f"  T={T}: std of the output's first 12 bins {[round(float(v), 6) for v in K.d(out)[:12].std(-1)]}")
    for name, got, (tol, e32) in (("out (log-mel units)", float(worst.max()), bd["out"]), ("per-bin mean", got_m, bd["mean"]),
                                  ("per-bin std - 1", got_s, bd["unit_std"])):
        print(f"  T={T} {name}: kernel {got:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    for name, got, (tol, e32) in (("out (log-mel units)", float(worst.max()), bd["out"]), ("per-bin mean", got_m, bd["mean"]),
                                  ("per-bin std - 1", got_s, bd["unit_std"])):
        assert got <= tol, f"T={T} {name}: {got} > {tol} (torch fp32: {e32})"


def test_logmel_finish_one_frame_normalises_to_zeros(cuda):
    out, _ = _logmel_finish(cuda, _log_uniform_mel(1, 80), True)
    assert torch.equal(out.cpu(), torch.zeros(80, 1))


# ----------------------------------------------------------------------------------------------------------- LogMel, band-limited
@pytest.mark.parametrize("seconds", [1, 60])
def test_logmel_band_limited_waveform(cuda, seconds):
    """Sines at 200, 440 and 1900 Hz plus 1e-4 dither: no component above 2 kHz but the dither, so most bins sit near their floor with a
    small spread.  Every bin of the normalised output has mean 0 and std 1 (bounds: torch's fp32 (x - mean) / std of LogMel's own
    un-normalised output, 4 x + 1e-5), and the output matches the float64 oracle to 1e-3 in log-mel units (tests/test_frontend_gpu.py).
    Measured on the MI355X (kernel | torch fp32 | bound): 1 s: |mean| 1.0e-06 | 7.8e-05 | 3.2e-04, |std - 1| 1.4e-07 | 8.4e-08 | 1.0e-05,
    oracle 4.6e-04; 60 s: |mean| 3.8e-07 | 6.3e-05 | 2.6e-04, |std - 1| 1.8e-07 | 6.5e-08 | 1.0e-05, oracle 4.3e-04.  With the uncentred
    statistics: |std - 1| 2.5e-03 (1 s) and 1.0 (60 s, a bin left un-normalised), oracle 4.6e-04 and 7.1e-02."""
    from dynamic_asr_eval_amd.frontend import LogMel
    from oracle.logmel_ref import logmel_ref
    n = 16000 * seconds
    t = torch.arange(n, dtype=F64) / 16000.0
    wav = (0.3 * torch.sin(2 * torch.pi * 200.0 * t) + 0.2 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * 1900.0 * t)
           + 1e-4 * torch.randn(n, generator=K.gen(seconds), dtype=F64)).float()
    raw = LogMel(cuda, normalize=False)(wav)[0]
    out = LogMel(cuda, normalize=True)(wav)[0]
    assert out.shape == (80, 1 + n // 160) and torch.isfinite(out).all()
    bins = list(range(80))
    e_m, e_s = K.unit_stats_err(K.normalise_fp32(raw), bins)
    got_m, got_s = K.unit_stats_err(out, bins)
    print(f"  {seconds} s per-bin mean: kernel {got_m:.2e} | torch fp32 {e_m:.2e} | bound {4 * e_m + 1e-5:.2e}")
    print(f"  {seconds} s per-bin std - 1: kernel {got_s:.2e} | torch fp32 {e_s:.2e} | bound {4 * e_s + 1e-5:.2e}")
    ref = logmel_ref(wav, normalize=True)[0]
    scale = logmel_ref(wav, normalize=False)[0].std(-1, keepdim=True)
    err = ((K.d(out) - ref).abs() * scale).max().item()
    print(f"  {seconds} s against the oracle: {err:.2e} log-mel units | bound 1e-3; smallest bin std {scale.min().item():.2e}")
    assert got_m <= 4 * e_m + 1e-5, f"per-bin mean {got_m} (torch fp32: {e_m})"
    assert got_s <= 4 * e_s + 1e-5, f"per-bin std - 1 {got_s} (torch fp32: {e_s})"
    assert err < 1e-3, err


# ----------------------------------------------------------------------------------------------------------- dyn_rownorm
@pytest.mark.parametrize("T", [2, 1023, 1024, 1025, 4097])
def test_rownorm(cuda, T):
    """Rows with mean / std of 0, 30 and 1000, in place and out of place; the output is in units of the row's std."""
    x = torch.randn(3, T, generator=K.gen(T)) * 0.7
    x = (x + torch.tensor([[0.0], [30.0 * 0.7], [1000.0 * 0.7]])).float()
    ref = K.rownorm_ref(x)
    t32 = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    buf, out = _guarded(cuda, 3 * T)
    xd = x.to(cuda)
    _ok(_L().dyn_rownorm(xd.data_ptr(), out.data_ptr(), 3, T, _stream()), "dyn_rownorm")
    assert _bits_equal(xd, x) and _tail_intact(buf, 3 * T)
    _ok(_L().dyn_rownorm(xd.data_ptr(), xd.data_ptr(), 3, T, _stream()), "dyn_rownorm")
    assert _bits_equal(xd, out.view(3, T)), "in place and out of place must agree bit for bit"
    for r, ratio in enumerate((0, 30, 1000)):
        _measured(f"T={T} mean/std={ratio}", out.view(3, T)[r], t32[r], ref[r], 2e-6)


# ----------------------------------------------------------------------------------------------------------- dyn_gather_frames
@pytest.mark.parametrize("Fq,T", [(1, 1), (80, 1), (3, 1025), (80, 4099)])
def test_gather_frames(cuda, Fq, T):
    x = torch.randn(Fq, T, generator=K.gen(Fq + T))
    xd = x.to(cuda)
    for along_time, n in ((1, T), (0, Fq)):
        for name, idx in (("identity", torch.arange(n)), ("reversal", torch.arange(n - 1, -1, -1)), ("permutation", torch.randperm(n, generator=K.gen(n)))):
            idx = idx.to(torch.int32)
            buf, y = _guarded(cuda, Fq * T)
            _ok(_L().dyn_gather_frames(xd.data_ptr(), idx.to(cuda).data_ptr(), y.data_ptr(), Fq, T, along_time, _stream()), "dyn_gather_frames")
            assert _bits_equal(y.view(Fq, T), K.gather_frames_ref(x, idx, along_time)), (name, along_time)
            assert _tail_intact(buf, Fq * T) and _bits_equal(xd, x)


# ----------------------------------------------------------------------------------------------------------- dyn_moments
@pytest.mark.parametrize("n", [1, 2, 255, 2049, 2_200_000])
def test_moments(cuda, n):
    """(sum, mean, unbiased std) of a buffer shaped like a normalised window (the only input the product gives it): mean 0.37, std 1.1.
    2 200 000 elements pass the 1024-block cap."""
    from dynamic_asr_eval_amd import ops
    L = _L()
    x = (torch.randn(n, generator=K.gen(n)) * 1.1 + 0.37).float()
    out = torch.full((3 + TAIL,), SENTINEL, device=cuda)
    ws = ops.workspace(cuda)
    assert ws.numel() >= L.dyn_moments_workspace_bytes()
    _ok(L.dyn_moments(x.to(cuda).data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "dyn_moments")
    assert _tail_intact(out, 3)
    want = K.moments_ref(x)
    t32 = (x.sum(), x.mean(), x.std() if n > 1 else torch.tensor(0.0))
    for name, got, w, t in zip(("sum", "mean", "std"), out[:3].cpu().tolist(), want, t32):
        if name == "std" and n == 1:
            assert got == 0.0, "the std of one element is 0"
            continue
        _measured(f"n={n} {name} (rel)", torch.tensor([got], dtype=F64), t.reshape(1), torch.tensor([w], dtype=F64), 2e-6, rel=True)
    assert L.dyn_moments(x.to(cuda).data_ptr(), n, out.data_ptr(), ws.data_ptr(), L.dyn_moments_workspace_bytes() - 1, _stream()) == E_WORKSPACE


# ----------------------------------------------------------------------------------------------------------- dyn_cutout
def _cutout_rects(Fq, T):
    """In order: an overlapping pair (the later wins), one rectangle touching each border, a zero-height and a zero-width one."""
    return [(Fq // 8, Fq // 2, T // 6, T // 2), (Fq // 4, 3 * Fq // 4, T // 3, 2 * T // 3),
            (0, 1, 1, T - 1), (Fq - 1, Fq, 2, T), (1, Fq - 1, 0, 1), (1, 3, T - 2, T),
            (2, 2, 1, T - 1), (0, Fq, T // 2, T // 2)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Fq,T", [(80, 600), (5, 7)])
def test_cutout(cuda, Fq, T, mode):
    """mode 0 zero / 1 each rectangle's own mean (all means before any fill) / 2 a constant.  Every cell takes the fill of the LAST rectangle
    covering it, bit-exact in position; the means are within 2e-6 of float64; cells outside every rectangle keep their bits."""
    L = _L()
    value = float(torch.tensor(1.2345678, dtype=torch.float32))
    x = (torch.randn(Fq, T, generator=K.gen(Fq * T + mode)) * 1.7 + 0.2).float()
    rects = _cutout_rects(Fq, T)
    for name, rs in (("edges and overlaps", rects), ("whole window first", [(0, Fq, 0, T)] + rects[:2]), ("whole window alone", [(0, Fq, 0, T)]),
                     ("no rectangle", [])):
        buf, xd = _guarded(cuda, Fq * T)
        xd.copy_(x.view(-1))
        rd = torch.tensor(rs, dtype=torch.int32).reshape(-1, 4).to(cuda)
        means = torch.full((len(rs) + 1,), SENTINEL, device=cuda)
        _ok(L.dyn_cutout(xd.data_ptr(), Fq, T, rd.data_ptr() if rs else 0, len(rs), mode, value, means.data_ptr(), _stream()), "dyn_cutout")
        got = xd.view(Fq, T).cpu()
        ref, win, m64 = K.cutout_ref(x, rs, mode, value)
        assert _tail_intact(buf, Fq * T), name
        assert _bits_equal(got[win < 0], x[win < 0]), f"{name}: a cell outside every rectangle changed"
        if name == "edges and overlaps":
            assert (win < 0).any() and all((win == k).any() for k in range(6)) and not (win == 6).any() and not (win == 7).any()
        if mode == 0:
            assert torch.equal(got[win >= 0], torch.zeros(int((win >= 0).sum()))), name
        elif mode == 2:
            assert _bits_equal(got[win >= 0], torch.full((int((win >= 0).sum()),), value)), name
        else:
            for k in range(len(rs)):
                cells = got[win == k]
                if cells.numel():
                    assert (cells == cells[0]).all(), f"{name}: rectangle {k} is not filled with one value"
                    err = abs(cells[0].double().item() - m64[k].item())
                    print(f"  [{Fq}, {T}] {name}: rectangle {k} mean error {err:.2e} | bound 2e-06")
                    assert err <= 2e-6, f"{name}: rectangle {k} mean {cells[0].item()} vs {m64[k].item()}"
        _check(f"[{Fq}, {T}] mode {mode} {name}", got, ref, 2e-6 if mode == 1 else 0.0)


# ----------------------------------------------------------------------------------------------------------- SpecAugment masks
def _masks(size):
    """33 (start, width) pairs: at index 0, ending exactly at the edge, of width 0, a wide one where the axis has room; the rest repeat."""
    base = [(0, 1), (size - 1, 1), (size // 2, 0), (size // 3, size // 4), (size - size // 5, size // 5)]
    reps = [(0, 1), (size - 1, 1), (size // 2, 0)]
    return base + [reps[k % 3] for k in range(33 - len(base))]


def _mask_ref(x, masks, along_time, value):
    ref = x.clone()
    for s, w in masks:
        if along_time:
            ref[:, s:s + w] = value
        else:
            ref[s:s + w, :] = value
    return ref


@pytest.mark.parametrize("Fq,T", [(80, 777), (3, 5)])
@pytest.mark.parametrize("along_time", [0, 1])
def test_specaug_masks_match_slice_assignment(cuda, Fq, T, along_time):
    """dyn_specaug_timemask / dyn_specaug_freqmask (mask positions in device memory) and dyn_specaug_mask_args (positions as kernel arguments,
    32 at a time) against plain slice assignment, with a host fill value and a device-resident one."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.augment import SpecAugment
    x = torch.randn(Fq, T, generator=K.gen(Fq + T + along_time))
    masks = _masks(T if along_time else Fq)
    st, wd = [m[0] for m in masks], [m[1] for m in masks]
    assert len(masks) == 33
    for value in (0.0, 1.5, torch.tensor([-3.25])):
        v = float(value) if not isinstance(value, torch.Tensor) else value.item()
        fill = value.to(cuda) if isinstance(value, torch.Tensor) else value
        ref = _mask_ref(x, masks, along_time, v)
        assert not torch.equal(ref, x) and (ref == x).any()
        for api in ("device positions", "argument positions"):
            buf, xd = _guarded(cuda, Fq * T)
            xd.copy_(x.view(-1))
            win = xd.view(Fq, T)
            if api == "device positions":
                sd, wdd = torch.tensor(st, dtype=torch.int32).to(cuda), torch.tensor(wd, dtype=torch.int32).to(cuda)
                (ops.specaug_timemask if along_time else ops.specaug_freqmask)(win, sd, wdd, fill)
            else:
                SpecAugment().apply(win, (([], []), (st, wd)) if along_time else ((st, wd), ([], [])), fill)
            assert _bits_equal(win, ref), (api, value)
            assert _tail_intact(buf, Fq * T), (api, value)


def test_specaug_mask_args_rejects_more_than_32_masks(cuda):
    x = torch.zeros(3, 5, device=cuda)
    a = (ctypes.c_int32 * 33)(*([0] * 33))
    assert _L().dyn_specaug_mask_args(x.data_ptr(), 3, 5, ctypes.addressof(a), ctypes.addressof(a), 33, 1, 1.0, 0, _stream()) == E_ARG


# ----------------------------------------------------------------------------------------------------------- ops.transpose_ft
@pytest.mark.parametrize("Fq,T", [(1, 1), (80, 31), (80, 33), (33, 513)])
def test_transpose_ft_of_a_strided_window(cuda, Fq, T):
    """[F, T] window view of a longer spectrogram (row stride > T, start not 16-byte aligned) -> contiguous [T, F], bit-exact."""
    from dynamic_asr_eval_amd import ops
    spec = torch.randn(Fq, T + 37, generator=K.gen(Fq * T))
    win = spec.to(cuda)[:, 5:5 + T]
    buf, out = _guarded(cuda, Fq * T)
    ops.transpose_ft(win, out=out.view(T, Fq))
    assert _bits_equal(out.view(T, Fq), spec[:, 5:5 + T].t()) and _tail_intact(buf, Fq * T)
    assert _bits_equal(ops.transpose_ft(win), spec[:, 5:5 + T].t())
