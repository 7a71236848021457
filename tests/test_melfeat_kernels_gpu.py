"""The waveform front end of the FastConformer family on the device (frontend.MelFeatures: csrc/melfeat.hip around the strided-row STFT
GEMM, dyn_stft_power and the mel GEMM) against tests/melfeat_refs.py: each mode's formula in float64, and transformers' own extractor.

No tolerance here is a chosen number.  The device is held to the float64 formula at kernel_refs.measured_tol: 4 x the error of the SAME
chain in float32 torch on the CPU on the same inputs, plus a floor of 4 ulp of the reference's largest magnitude.  Against the extractor's
float32 output the bar is that plus the extractor's own measured distance from the float64 formula on the same input.  Every test prints
the distances; the measured figures (MI355X) are in DESIGN.md, "Waveform front end of the FastConformer family"."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import melfeat_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
CASES = {"L320": ((320,), 0.0), "L401": ((401,), 0.0), "L561": ((561,), 0.0), "ragged-5000-3333": ((5000, 3333), 0.0),
         "ragged-16000-801": ((16000, 801), 0.0), "3s": ((48000,), 0.0), "3s-plus-0.5": ((48000,), 0.5)}
_FE, _EXT, _REF = {}, {}, {}


def _size(kind):
    return 80 if kind == "parakeet" else 128


def _dither(kind):
    return 1e-5 if kind == "cohere_asr" else 0.0


def _fe(cuda, kind, dither=None):
    """(the device front end, its float32 basis and filters on the host), built once per (mode, dither)."""
    from dynamic_asr_eval_amd import frontend as FE
    key = (kind, dither)
    if key not in _FE:
        fe = FE.MelFeatures(kind, _size(kind), cuda, **({} if dither is None else {"dither": dither}))
        _FE[key] = (fe, fe.basis.cpu(), fe.fb.cpu())
    return _FE[key]


def _extractor(kind, dither=None):
    from transformers.utils import logging as hf_logging
    hf_logging.set_verbosity_error()
    key = (kind, dither)
    if key not in _EXT:
        _EXT[key] = R.make_extractor(R.extractor_class(kind), _size(kind), dither=dither)
    return _EXT[key]


def _zeros(t):
    return t.numel() == 0 or t.abs().max().item() == 0.0


def _rows(Ls, offset=0.0, amplitude=0.1):
    return [R.audio(L, 100 + L, amplitude, offset) for L in Ls]


def _batch(rows, cuda, fill=0.0):
    x = torch.full((len(rows), max(r.numel() for r in rows)), fill)
    for b, r in enumerate(rows):
        x[b, :r.numel()] = r
    return x.to(cuda).contiguous()


def _refs(cuda, kind, name, rows, dither):
    """(float64 formula, valid frames, the float32 chain, the device's bound), computed once per case and left unchanged."""
    key = (kind, name, dither)
    if key not in _REF:
        _, basis, fb = _fe(cuda, kind, dither if kind == "cohere_asr" else None)
        exact, lens = R.features_f64(kind, rows, _size(kind), dither=dither)
        c32, _ = R.chain32(kind, rows, basis, fb, dither=dither)
        tol, e32 = K.measured_tol(c32, exact, 4 * ULP * exact.abs().max().item())
        _REF[key] = (exact, lens, c32, tol, e32)
    return _REF[key]


def _against_formula_and_extractor(cuda, kind, name, rows, dither):
    fe, _, _ = _fe(cuda, kind, dither if kind == "cohere_asr" else None)
    exact, lens, c32, tol, e32 = _refs(cuda, kind, name, rows, dither)
    got, got_lens = fe(_batch(rows, cuda), [r.numel() for r in rows])
    assert got_lens == lens and tuple(got.shape) == tuple(exact.shape)
    g = got.cpu()
    err = K.max_err(g, exact)
    want, mask = R.run_extractor(_extractor(kind, dither if kind == "cohere_asr" else None), rows)
    assert mask.sum(1).tolist() == lens and want.shape == exact.shape
    own = max((want[b, :n].double() - exact[b, :n]).abs().max().item() for b, n in enumerate(lens))
    against = max((g[b, :n].double() - want[b, :n].double()).abs().max().item() for b, n in enumerate(lens))
    print(f"  {kind} {name}: kernel vs float64 {err:.2e} | float32 chain {e32:.2e} | bound {tol:.2e} | extractor vs float64 {own:.2e} | "
          f"kernel vs extractor {against:.2e}")
    for b, n in enumerate(lens):
        assert _zeros(g[b, n:])                                                    # exact zeros past the row's count
    assert err <= tol, (kind, name, err, tol)
    assert against <= tol + own, (kind, name, against, tol, own)
    return g


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", R.MODES)
def test_features_against_the_formula_and_the_extractor(cuda, kind, name):
    """Every mode at two frames (L = 320), a frame that straddles the row's end (401, 561), two ragged pairs, 3 s, and 3 s on a constant
    0.5 (the pre-emphasis leaves 0.015 of it; LASR, without one, keeps all of it in bin 0, below its 125 Hz filters).  LASR needs 400
    samples for a frame: its L = 320 case is the refusal.  Cohere runs with the extractor's dither 1e-5.
    Measured: DESIGN.md."""
    from dynamic_asr_eval_amd import ops
    Ls, offset = CASES[name]
    rows = _rows(Ls, offset)
    if kind == "lasr" and min(Ls) < 400:
        fe, _, _ = _fe(cuda, kind)
        with pytest.raises(ops.DynError, match="no valid feature frame"):
            fe(_batch(rows, cuda))
        return
    _against_formula_and_extractor(cuda, kind, name, rows, _dither(kind))


@pytest.mark.parametrize("kind", R.MODES)
def test_ragged_batch(cuda, kind):
    """5000 | 3333: each row's valid frames against the same row extracted alone UNDER THE TOLERANCE (the batched and the single DFT GEMM
    may take different plans, M = 32 x 2 against 32 or 21 rows, so bit equality is not guaranteed and not asserted); exact zeros past the
    valid count; a padding region holding 1e3 gives the same bits as zeros; a short batch after a long one leaves nothing behind."""
    fe, _, _ = _fe(cuda, kind, _dither(kind) if kind == "cohere_asr" else None)
    rows = _rows((5000, 3333))
    exact, lens, _, tol, _ = _refs(cuda, kind, "ragged-5000-3333", rows, _dither(kind))
    Ls = [r.numel() for r in rows]
    first, got_lens = fe(_batch(rows, cuda), Ls)
    assert got_lens == lens
    for b, r in enumerate(rows):
        alone, n = fe(r.view(1, -1).to(cuda).contiguous())
        assert n == [lens[b]]
        diff = (alone[0, :lens[b]] - first[b, :lens[b]]).abs().max().item()
        print(f"  {kind} row {b}: batch vs alone {diff:.2e} (bound {tol:.2e})")
        assert diff <= tol, (kind, b, diff, tol)
        assert _zeros(first[b, lens[b]:])
    dirty, _ = fe(_batch(rows, cuda, fill=1e3), Ls)
    assert torch.equal(dirty, first)
    long_rows = _rows((48000, 20000))
    fe(_batch(long_rows, cuda), [48000, 20000])
    again, _ = fe(_batch(rows, cuda), Ls)
    assert torch.equal(again, first)


def _finish_refs(mel32, lens, guard):
    """(float64, float32 torch) of dyn_melfeat_finish's normalised output [B, T, F] for mel [B, T, F] float32."""
    g32 = torch.tensor(guard, dtype=torch.float32)
    exact = R.finish(torch.log(mel32.double() + g32.double()), lens, True)
    c32 = R.finish(torch.log(mel32 + g32), lens, True)
    return exact, c32


def _spread_inputs(T, classes, seed, guard):
    """mel [T, F] as kernel_refs.logmel_class_inputs builds it: column f has log(mel + guard) ~ mu + sd * randn, (mu, sd) = classes[f % n]."""
    z = torch.randn(T, 80, generator=K.gen(9000 + seed + T), dtype=torch.float64)
    mu = torch.tensor([classes[f % len(classes)][0] for f in range(80)], dtype=torch.float64)
    sd = torch.tensor([classes[f % len(classes)][1] for f in range(80)], dtype=torch.float64)
    return (torch.exp(mu + sd * z) - guard).clamp(min=0.0).float().contiguous()


@pytest.mark.parametrize("what", ["at-the-guard", "large-mean"])
def test_finish_keeps_the_std_of_a_narrow_bin(cuda, what):
    """Crafted mel energies straight to dyn_melfeat_finish, two rows of 801 and 300 valid frames (four and two 256-frame blocks).
    at-the-guard: kernel_refs.logmel_class_inputs, whose bins 0, 6, .. sit at log(guard) = -13.8 with a spread of 1e-3 and whose bin 79 is
    all zeros; large-mean: bins at log-energy 10 and 15 with spreads of 1e-3 and 1e-2.  A statistic formed as E[x^2] - mean^2 from float32
    sums loses both.  The output and its per-bin std are held to the float64 value at measured_tol; the all-zero bin is exact zeros."""
    from dynamic_asr_eval_amd import ops
    guard, T, lens = K.LOGMEL_EPS, 801, [801, 300]
    if what == "at-the-guard":
        mel = torch.stack([K.logmel_class_inputs(T, 80, seed=s) for s in (0, 1)])
    else:
        mel = torch.stack([_spread_inputs(T, ((10.0, 1e-3), (15.0, 1e-2), (10.0, 1.0)), s, guard) for s in (0, 1)])
    exact, c32 = _finish_refs(mel, lens, guard)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=cuda)
    got = ops.melfeat_finish(mel.to(cuda), lens_dev, guard, False, True, 1e-5, "tf").cpu()
    tol, e32 = K.measured_tol(c32, exact, 4 * ULP * exact.abs().max().item())
    err = K.max_err(got, exact)
    print(f"  {what}: output kernel {err:.2e} | float32 torch {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, (err, tol)
    for b, n in enumerate(lens):
        s64, s32, sg = exact[b, :n].std(0), c32[b, :n].double().std(0), got[b, :n].double().std(0)
        stol, se32 = K.measured_tol(s32, s64, 4 * ULP)
        serr = (sg - s64).abs().max().item()
        print(f"  {what} row {b}: per-bin std of the output kernel {serr:.2e} | float32 torch {se32:.2e} | bound {stol:.2e}")
        assert serr <= stol, (b, serr, stol)
        assert _zeros(got[b, n:])
        if what == "at-the-guard":
            assert got[b, :, K.LOGMEL_ZERO_COLUMN].abs().max().item() == 0.0 == exact[b, :, K.LOGMEL_ZERO_COLUMN].abs().max().item()


@pytest.mark.parametrize("kind", R.NORMALISED)
def test_an_all_zero_row_gives_exact_zeros(cuda, kind):
    """Silence beside a live row: every bin of the silent row is log(2^-24) at every frame, mean == value, output exact zeros.  The
    yardstick is the float64 formula (zeros too), not the extractor: its float32 mean of equal values can round, and the difference is
    then divided by 1e-5.  (Cohere without dither: dither is what keeps its silence from being one.)"""
    fe, _, _ = _fe(cuda, kind, 0.0 if kind == "cohere_asr" else None)
    rows = [R.audio(5000, 7), torch.zeros(3333)]
    exact, lens = R.features_f64(kind, rows, _size(kind))
    got, got_lens = fe(_batch(rows, cuda), [5000, 3333])
    assert got_lens == lens
    assert exact[1].abs().max().item() == 0.0
    assert got[1].abs().max().item() == 0.0
    assert got[0, :lens[0]].abs().max().item() > 1.0


def test_one_long_row_in_both_layouts(cuda):
    """B = 1, L = 480000: 3000 frames, the statistics cross twelve 256-frame blocks.  [B, F, T] is the transpose of [B, T, F] bit for bit
    (the same value per element, through an LDS tile), and both are held to the float64 formula."""
    kind = "parakeet"
    fe, _, _ = _fe(cuda, kind)
    rows = _rows((480000,))
    exact, lens, _, tol, e32 = _refs(cuda, kind, "30s", rows, 0.0)
    x = _batch(rows, cuda)
    tf, n1 = fe(x, layout="tf")
    ft, n2 = fe(x, layout="ft")
    assert n1 == n2 == lens == [3000] and tuple(tf.shape) == (1, 3001, 80) and tuple(ft.shape) == (1, 80, 3001)
    assert torch.equal(ft, tf.transpose(1, 2))
    err = K.max_err(tf.cpu(), exact)
    print(f"  30 s: kernel vs float64 {err:.2e} | float32 chain {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, (err, tol)
    assert tf[0, 3000].abs().max().item() == 0.0


@pytest.mark.parametrize("dither", [1e-5, 0.0])
def test_cohere_dither_against_the_extractor(cuda, dither):
    """The deterministic dither (randn from a CPU generator seeded with the row's sample count, times 1e-5, added before the pre-emphasis)
    and its absence, on a ragged pair whose second row is quiet enough (amplitude 1e-4) for the dither to matter."""
    rows = [R.audio(5000, 11), R.audio(3333, 12, amplitude=1e-4)]
    _against_formula_and_extractor(cuda, "cohere_asr", f"dither-{dither}", rows, dither)


def test_lasr_against_its_extractor_at_the_clamp(cuda):
    """LasrFeatureExtractor computes in float64 and returns float32.  The second row (amplitude 5e-4) has its quietest bins, 16 % of its
    values in the float64 formula, at the clamp log(1e-5); the first row only the bins whose filter is empty."""
    rows = [R.audio(5000, 21), R.audio(3333, 22, amplitude=5e-4)]
    g = _against_formula_and_extractor(cuda, "lasr", "clamp", rows, 0.0)
    exact = _refs(cuda, "lasr", "clamp", rows, 0.0)[0]
    floor = torch.log(torch.tensor(1e-5, dtype=torch.float64)).item()
    at64, at = (exact[1, :19] - floor).abs() < 1e-9, (g[1, :19].double() - floor).abs() < 4 * ULP * abs(floor)
    loud = ((exact[0, :29] - floor).abs() < 1e-9).float().mean().item()             # only the bins whose filter is empty (below 125 Hz)
    assert 0.1 < at64.float().mean().item() < 0.25 and loud < 0.05
    assert (at == at64).float().mean().item() > 0.99                                  # a bin within rounding of the clamp may fall on either side
