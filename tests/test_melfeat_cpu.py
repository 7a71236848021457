"""What of the FastConformer family's waveform front end (frontend.MelFeatures / MelStream, csrc/melfeat.hip) can be checked without a GPU:
the C-ABI surface and its argument refusals, the frame counts against transformers' extractors, the filter matrices against their sources,
every host-side refusal by name, the streaming sample arithmetic, Cohere's dither noise, and the references of tests/melfeat_refs.py against
the extractors they restate."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import melfeat_refs as R  # noqa: E402

ENTRIES = ("dyn_melfeat_prep", "dyn_melfeat_finish_workspace_bytes", "dyn_melfeat_finish")
LENGTHS = (160, 161, 319, 320, 511, 512, 513, 5000)


def _quiet():
    from transformers.utils import logging as hf_logging
    hf_logging.set_verbosity_error()


def test_header_entries_are_exported_and_refuse_before_any_launch():
    """The three entries are in include/dyneval.h and in the library; argument errors come back as DYN_E_ARG (-1) / DYN_E_WORKSPACE (-3)
    before any launch, so dummy pointers are never dereferenced."""
    from dynamic_asr_eval_amd import _lib
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    lib = _lib.load()
    for n in ENTRIES:
        assert hasattr(lib, n), n
    p, q = 256, 512
    prep = lambda *a: lib.dyn_melfeat_prep(*a, None)                                                          # noqa: E731
    assert prep(None, q, p, None, None, 2, 100, 256, 612, 0.97, 0.0) == -1
    assert prep(p, None, p, None, None, 2, 100, 256, 612, 0.97, 0.0) == -1
    assert prep(p, q, None, None, None, 2, 100, 256, 612, 0.97, 0.0) == -1 and b"lens" in lib.dyn_last_error()
    assert prep(p, q, p, None, None, 2, 100, 256, 355, 0.97, 0.0) == -1 and b"W >= pad + Lmax" in lib.dyn_last_error()
    assert prep(p, q, p, None, None, 2, 0, 256, 612, 0.97, 0.0) == -1
    assert prep(p, q, p, None, None, 2, 100, -1, 612, 0.97, 0.0) == -1
    assert prep(p, q, p, None, None, 2, 100, 256, 612, 1.0, 0.0) == -1
    assert prep(p, q, p, None, None, 2, 100, 256, 612, 0.97, -1.0) == -1
    assert prep(p, q, p, None, None, 0, 100, 256, 612, 0.97, 0.0) == 0                                         # nothing to do
    assert lib.dyn_melfeat_finish_workspace_bytes(2, 300, 80) == 2 * 2 * 160 * 4 + 2 * 160 * 8
    assert lib.dyn_melfeat_finish_workspace_bytes(1, 360000, 128) == 1407 * 256 * 4 + 256 * 8
    ws = lib.dyn_melfeat_finish_workspace_bytes(2, 300, 80)
    fin = lambda *a: lib.dyn_melfeat_finish(*a, None)                                                          # noqa: E731
    assert fin(None, q, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, p, ws) == -1
    assert fin(p, q, None, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, p, ws) == -1
    assert fin(p, p, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, p, ws) == -1 and b"alias" in lib.dyn_last_error()
    assert fin(p, q, p, 2, 300, 257, 1e-6, 0, 1, 1e-5, 0, p, 1 << 20) == -1
    assert fin(p, q, p, 2, 0, 80, 1e-6, 0, 1, 1e-5, 0, p, ws) == -1
    assert fin(p, q, p, 2, 300, 80, 0.0, 0, 1, 1e-5, 0, p, ws) == -1
    assert fin(p, q, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 2, p, ws) == -1 and b"layout" in lib.dyn_last_error()
    assert fin(p, q, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, p, ws - 1) == -3
    assert fin(p, q, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, p + 4, ws) == -3
    assert fin(p, q, p, 2, 300, 80, 1e-6, 0, 1, 1e-5, 0, None, ws) == -3
    assert fin(p, q, p, 0, 300, 80, 1e-6, 0, 1, 1e-5, 0, p, ws) == 0


@pytest.mark.parametrize("kind,center", [(k, True) for k in R.MODES] + [("nemotron_asr_streaming", False)])
def test_frame_counts_equal_the_extractors_attention_mask(kind, center):
    """frontend.mel_frames / mel_output_frames against `attention_mask.sum(1)` and the feature shape of transformers' extractor, each
    length alone and all of them as one ragged batch.  Where the extractor itself cannot run (LASR's unfold below 400 samples, torch.stft
    with center=False below 512) the count is 0, which MelFeatures refuses."""
    from dynamic_asr_eval_amd import frontend as FE
    _quiet()
    F_ = 80 if kind == "parakeet" else 128
    fe = R.make_extractor(R.extractor_class(kind), F_, dither=0.0)
    floor = 400 if kind == "lasr" else (512 if not center else 1)
    ok = [L for L in LENGTHS if L >= floor]
    for L in LENGTHS:
        if L < floor:
            assert FE.mel_frames(kind, L, center) == 0 == R.valid_frames(kind, L, center)
            continue
        feats, mask = R.run_extractor(fe, [R.audio(L, L)], center)
        assert FE.mel_frames(kind, L, center) == int(mask.sum()) == R.valid_frames(kind, L, center), L
        assert FE.mel_output_frames(kind, L, center) == feats.shape[1] == R.output_frames(kind, L, center), L
    feats, mask = R.run_extractor(fe, [R.audio(L, L) for L in ok], center)
    assert mask.sum(1).tolist() == [FE.mel_frames(kind, L, center) for L in ok]
    assert feats.shape[1] == FE.mel_output_frames(kind, max(ok), center)


def test_filter_matrices_equal_their_sources():
    from dynamic_asr_eval_amd import frontend as FE
    from transformers.audio_utils import mel_filter_bank
    from transformers.models.lasr.feature_extraction_lasr import LasrFeatureExtractor
    for F_ in (80, 128):
        want = torch.from_numpy(mel_filter_bank(257, F_, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney")).to(torch.float32)
        for kind in ("parakeet", "nemotron_asr_streaming", "cohere_asr"):
            got = FE.mel_filters(kind, F_)
            assert got.dtype == torch.float64 and torch.equal(got.float(), want) and torch.equal(got, want.double())
        assert torch.equal(R.make_extractor(R.extractor_class("parakeet"), F_).mel_filters, want.T)
    assert torch.equal(FE.mel_filters("lasr", 128), LasrFeatureExtractor().mel_filters)
    fe = FE.MelFeatures("lasr", 128, device="cpu")
    assert fe.fb.shape == (260, 128) and torch.equal(fe.fb[:257], LasrFeatureExtractor().mel_filters.float()) and fe.fb[257:].abs().max() == 0
    w = torch.hann_window(400, periodic=False, dtype=torch.float64)
    assert (FE.mel_basis(0)[:, 0] - w).abs().max().item() < 1e-15                     # bin 0's cosine column is the window itself
    assert FE.MelFeatures("parakeet", 80, device="cpu").basis.shape == (400, 520)


def test_references_restate_the_extractors():
    """tests/melfeat_refs.features_f64 against the extractors it restates (valid frames, shapes, values), so a wrong reference cannot hide
    a wrong kernel.  The bound is loose on purpose (the extractors compute in float32; LASR in float64): the GPU tests measure the
    distance per case and add it to the device's bound."""
    _quiet()
    for kind in R.MODES:
        F_ = 80 if kind == "parakeet" else 128
        dither = 1e-5 if kind == "cohere_asr" else 0.0
        fe = R.make_extractor(R.extractor_class(kind), F_)
        rows = [R.audio(5000, 1), R.audio(3333, 2)]
        want, mask = R.run_extractor(fe, rows)
        exact, lens = R.features_f64(kind, rows, F_, dither=dither)
        assert mask.sum(1).tolist() == lens and want.shape == exact.shape
        for b, n in enumerate(lens):
            assert (want[b, :n].double() - exact[b, :n]).abs().max().item() < (1e-5 if kind == "lasr" else 2e-3), kind
            if kind != "lasr":
                assert want[b, n:].abs().max().item() == 0.0 == exact[b, n:].abs().max().item()


def test_every_refusal_is_raised_by_name():
    from dynamic_asr_eval_amd import frontend as FE
    from dynamic_asr_eval_amd import ops
    for name, v in (("sampling_rate", 8000), ("n_fft", 400), ("win_length", 320), ("hop_length", 128)):
        with pytest.raises(ops.DynError, match=name):
            FE.MelFeatures("parakeet", 80, device="cpu", **{name: v})
        with pytest.raises(ops.DynError, match=name):
            FE.MelFeatures.from_preprocessor_config({"feature_extractor_type": "ParakeetFeatureExtractor", "feature_size": 80, name: v}, device="cpu")
    with pytest.raises(ops.DynError, match="kind"):
        FE.MelFeatures("whisper", 80, device="cpu")
    with pytest.raises(ops.DynError, match="feature_extractor_type"):
        FE.MelFeatures.from_preprocessor_config({"feature_extractor_type": "WhisperFeatureExtractor"}, device="cpu")
    with pytest.raises(ops.DynError, match="feature_size"):
        FE.MelFeatures("parakeet", 258, device="cpu")
    with pytest.raises(ops.DynError, match="unknown option"):
        FE.MelFeatures("parakeet", 80, device="cpu", window="hamming")
    with pytest.raises(ops.DynError, match="dither"):
        FE.MelFeatures("parakeet", 80, device="cpu", dither=1e-5)
    fe = FE.MelFeatures.from_preprocessor_config({"feature_extractor_type": "CohereAsrFeatureExtractor", "feature_size": 128, "sampling_rate": 16000,
                                                  "n_fft": 512, "win_length": 400, "hop_length": 160, "preemphasis": 0.97, "dither": 0.0},
                                                 device="cpu")
    assert (fe.kind, fe.feature_size, fe.dither, fe.normalize) == ("cohere_asr", 128, 0.0, True)
    par, nem, coh, las = (FE.MelFeatures(k, 80 if k == "parakeet" else 128, device="cpu") for k in R.MODES)
    with pytest.raises(ops.DynError, match="no valid feature frame"):
        par.check_audio_lengths([5000, 159], 2, 5000)
    with pytest.raises(ops.DynError, match="no valid feature frame"):
        las.check_audio_lengths([399], 1, 399)
    with pytest.raises(ops.DynError, match="no valid feature frame"):
        nem.check_audio_lengths([511], 1, 511, center=False)
    for fe in (par, coh):
        with pytest.raises(ops.DynError, match="unbiased variance"):
            fe.check_audio_lengths([5000, 319], 2, 5000)
    assert nem.check_audio_lengths([5000, 319], 2, 5000) == ([5000, 319], [31, 1])                          # no normalisation: one frame is a row
    with pytest.raises(ops.DynError, match="energy-based"):
        coh.check_audio_lengths([480001], 1, 480001)
    assert coh.check_audio_lengths([480000], 1, 480000)[1] == [3000]
    assert par.check_audio_lengths([480001], 1, 480001)[1] == [3000]
    for fe in (par, coh, las):
        with pytest.raises(ops.DynError, match="center=False"):
            fe.check_audio_lengths([5000], 1, 5000, center=False)
    with pytest.raises(ops.DynError, match="audio_lengths"):
        par.check_audio_lengths([5000], 2, 5000)
    with pytest.raises(ops.DynError, match="audio_lengths"):
        par.check_audio_lengths([5001, 400], 2, 5000)
    with pytest.raises(ops.DynError, match="audio_lengths"):
        par.check_audio_lengths(torch.tensor([5000.0, 400.0]), 2, 5000)
    assert par.check_audio_lengths(torch.tensor([5000, 400]), 2, 5000) == ([5000, 400], [31, 2])
    assert par.check_audio_lengths(None, 2, 5000) == ([5000, 5000], [31, 31])
    with pytest.raises(ops.DynError, match="CUDA"):
        par(torch.zeros(1, 5000))
    with pytest.raises(ops.DynError, match="streaming"):
        FE.MelStream(par, 2)


@pytest.mark.parametrize("look", [0, 1, 3])
def test_streaming_sample_arithmetic(look):
    """How many samples complete chunk k: centred frame t reads the samples 160 t - 200 .. 160 t + 199, so the first n frames are ready
    once 160 (n - 1) + 200 samples have arrived, not one sooner.  Checked against a brute-force count over the window supports."""
    from dynamic_asr_eval_amd import frontend as FE
    from dynamic_asr_eval_amd import ops
    geo = ops.stream_geometry(9, look)
    first, later = geo.first_frames, geo.frames
    assert (first, later) == (1 + 8 * look, 8 * (look + 1))
    ready = lambda S: sum(1 for t in range(S // 160 + 3) if 160 * t + 199 < S)                                # noqa: E731
    for S in list(range(0, 700)) + [999, 1000, 1001, 15999, 16000, 16040]:
        assert FE.stream_frames_ready(S) == ready(S), S
        assert FE.stream_frames_ready(S) <= S // 160                                    # never a frame the offline pass would mask
    for k in range(5):
        n = first + k * later
        S = FE.stream_samples_for_chunk(k, first, later)
        assert S == 160 * (n - 1) + 200 == FE.stream_samples_for_frames(n)
        assert ready(S) == n and ready(S - 1) == n - 1
    assert FE.stream_samples_for_frames(0) == 0 and FE.stream_samples_for_chunk(0, 1, 8) == 200


def test_cohere_dither_noise_equals_the_extractors():
    from dynamic_asr_eval_amd import frontend as FE
    fe = R.make_extractor(R.extractor_class("cohere_asr"), 128, dither=1.0)
    lens = [5000, 3333, 1]
    want = fe._apply_dither(torch.zeros(3, 5000), torch.tensor(lens))                  # zeros + 1.0 * noise
    got = FE.cohere_dither_noise(lens, 5000)
    assert torch.equal(got, want) and got[1, 3333:].abs().max() == 0
    assert torch.equal(FE.cohere_dither_noise([3333], 4000)[0, :3333], got[1, :3333])     # a row's noise does not depend on its batch
