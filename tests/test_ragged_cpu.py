"""Ragged batches (per-row frame counts, `input_lengths=`) without a GPU: the length arithmetic and lengths_from_mask against transformers,
every refusal by name, the new entries' argument refusals through ctypes, and the oracle facts the GPU tests stand on, re-checked on the
inputs those tests use: transformers' masked batch equals every row run alone within the tolerance, and its unmasked padded batch misses
it by at least ten times the tolerance (so a forgotten mask cannot pass)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as R  # noqa: E402
import ragged_refs as RR  # noqa: E402


def test_length_arithmetic_is_transformers():
    from dynamic_asr_eval_amd import parakeet_model as PM
    _, ref = R.hf_model()
    L = list(range(1, 71))
    stages = PM.output_lengths(L)
    assert stages[0] == L and len(stages) == 4
    assert stages[3] == ref.encoder._get_subsampling_output_length(torch.tensor(L)).tolist() == [PM.frames(n) for n in L] == RR.enc_lens(L)
    sub = ref.encoder.subsampling
    cur = torch.tensor(L)
    for i, layer in enumerate(l for l in sub.layers if isinstance(l, torch.nn.Conv2d) and l.stride != (1, 1)):
        cur = sub._get_output_length(cur, layer)
        assert stages[i + 1] == cur.tolist(), i
    assert stages[3][:3] == [1, 1, 1] and stages[3][8] == 2 and stages[3][16] == 3         # rows of 1, 2 and 3 encoder frames exist


def test_lengths_from_mask():
    from dynamic_asr_eval_amd import parakeet_model as PM
    from dynamic_asr_eval_amd.ops import DynError
    for lens in RR.LENS:
        m = RR.prefix_mask(lens, RR.T_FEAT)
        for mask in (m, m.to(torch.int32), m.to(torch.int64)):
            assert PM.lengths_from_mask(mask) == list(lens)
    hole = RR.prefix_mask((5, 8), 8).clone()
    hole[0, 6] = True
    for bad, word in ((hole, "prefix"), (RR.prefix_mask((0, 8), 8), "no valid frame"), (torch.ones(2, 8), "integer or bool"),
                      (torch.ones(8, dtype=torch.bool), "[B, T]"), ([[1, 1]], "[B, T]")):
        with pytest.raises(DynError) as e:
            PM.lengths_from_mask(bad)
        assert word in str(e.value), str(e.value)


def test_input_lengths_are_checked_by_name():
    from dynamic_asr_eval_amd import parakeet_model as PM
    from dynamic_asr_eval_amd.ops import DynError
    assert PM.check_input_lengths([8, 1, 3], 3, 8) == [8, 1, 3]
    assert PM.check_input_lengths(torch.tensor([8, 1, 3], dtype=torch.int32), 3, 8) == [8, 1, 3]
    assert PM.check_input_lengths((8,), 1, 8) == [8]
    for bad, word in (([8, 1], "2 counts for a batch of 3"), ([8, 0, 3], "1 .. T = 8"), ([9, 1, 3], "1 .. T = 8"), ([8, 1, -3], "1 .. T = 8"),
                      ([8.0, 1, 3], "integers"), ([True, 1, 3], "integers"), (torch.tensor([8.0, 1, 3]), "integers"),
                      (torch.ones(3, dtype=torch.bool), "integers"), (torch.ones(3, 1, dtype=torch.int64), "one count per row"),
                      (8, "sequence of ints"), ("811", "sequence of ints")):
        with pytest.raises(DynError) as e:
            PM.check_input_lengths(bad, 3, 8)
        assert "input_lengths" in str(e.value) and word in str(e.value), str(e.value)


def test_what_is_not_built_with_input_lengths_is_refused_by_name():
    """Before any launch, so no GPU is needed to see it: the classes without per-row counts, batch_renorm_training(), and attention_mask as
    before (its text now points at input_lengths)."""
    from dynamic_asr_eval_amd import lasr_model as LM, parakeet_model as PM
    from dynamic_asr_eval_amd.ops import DynError
    x = torch.zeros(2, 16, 80)
    with pytest.raises(DynError) as e:
        LM.LasrForCTC.forward(None, x, input_lengths=[16, 8])
    assert "input_lengths" in str(e.value) and "LasrForCTC" in str(e.value)
    stage = PM.ParakeetForCTC._stage_lengths
    with pytest.raises(DynError) as e:
        stage(SimpleNamespace(_ragged=True, _brn=object()), [16, 8], 2, 16)
    assert "batch_renorm_training" in str(e.value) and "input_lengths" in str(e.value)
    with pytest.raises(DynError) as e:
        stage(SimpleNamespace(_ragged=False, _brn=None), [16, 8], 2, 16)
    assert "input_lengths is not built for" in str(e.value)
    with pytest.raises(DynError) as e:
        PM.ParakeetForCTC.forward(None, x, attention_mask=torch.ones(2, 16))
    assert "attention_mask" in str(e.value) and "input_lengths" in str(e.value)
    from dynamic_asr_eval_amd.nemotron3_5_asr_model import Nemotron3_5AsrForRNNT
    from dynamic_asr_eval_amd.nemotron_asr_streaming_model import NemotronAsrStreamingForRNNT
    from dynamic_asr_eval_amd.nemotron_asr_streaming_stream import StreamSession
    for cls in (NemotronAsrStreamingForRNNT, Nemotron3_5AsrForRNNT):
        for call in (cls.encode, cls.forward, cls.generate):
            with pytest.raises(DynError) as e:
                call(None, x, input_lengths=[16, 8])
            assert "input_lengths is not built for" in str(e.value), str(e.value)     # (the class name in the text is type(self)'s: None here)
    for call in (lambda: StreamSession._encode(None, x, None, [16, 8]),                         # push() and encode_chunk() hand it down
                 lambda: StreamSession.encode_chunk(SimpleNamespace(_encode=lambda *a: StreamSession._encode(None, *a)), x, None, [16, 8])):
        with pytest.raises(DynError) as e:
            call()
        assert "input_lengths" in str(e.value) and "streaming session" in str(e.value)


def test_capture_and_the_wrappers_refuse_by_name(monkeypatch):
    """hipGraph capture is refused where the counts are checked (the stream's capture state is read, nothing is launched); the ops wrappers
    refuse a `lens` that is no int32 CUDA tensor, `valid` next to `lens`, and one of lens_in / lens_out without the other: all before
    any pointer is taken, so the CPU tensors here are never read.  (A wrong count and a strided `lens` need a CUDA tensor:
    tests/test_ragged_kernels_gpu.py.)"""
    from dynamic_asr_eval_amd import ops, parakeet_model as PM
    from dynamic_asr_eval_amd.ops import DynError
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(DynError) as e:
        PM.ParakeetForCTC._stage_lengths(SimpleNamespace(_ragged=True, _brn=None), [16, 8], 2, 16)
    assert "hipGraph capture" in str(e.value) and "input_lengths" in str(e.value)
    monkeypatch.undo()
    for bad in ([3, 3], torch.tensor([3, 3], dtype=torch.int32), torch.tensor([3, 3]), torch.tensor([3.0, 3.0]), None):
        with pytest.raises(DynError) as e:
            ops._lens_ptr(bad, 2, "who")
        assert "who: lens must be a contiguous int32 CUDA tensor [B]" in str(e.value)
    with pytest.raises(DynError) as e:
        ops._lens_ptr(torch.tensor([3, 3], dtype=torch.int32), 2, "who", valid=torch.tensor([3], dtype=torch.int32))
    assert "not both" in str(e.value)
    for kw in (dict(lens_in=torch.tensor([3], dtype=torch.int32)), dict(lens_out=torch.tensor([3], dtype=torch.int32))):
        with pytest.raises(DynError) as e:
            ops._stage_lens("who", 1, kw.get("lens_in"), kw.get("lens_out"))
        assert "lens_in and lens_out go together" in str(e.value)


def test_cohere_oracle_has_teeth_on_the_gpu_tests_inputs():
    """transformers' CohereAsrForConditionalGeneration (tests/cohere_asr_refs.py, decoder A, the decode cases' seeds, gain 8) on the
    features [3, 131, 80] with lens (131, 67, 100).  The decoder's logits hardly depend on the audio with random weights (a forgotten mask
    moves them by 0.9e-4 .. 4.5e-4 at a tolerance of 1.6e-4, and by 5e-5 at gain 1), so the GPU test compares what the cross-attention
    READS: `decoder.proj` of the encoder states through every layer's k_proj | v_proj.  There the masked batch lies within the tolerance
    of each row alone and the unmasked batch at least ten times the tolerance away.  Measured: tolerance 2.1e-05, masked 2.7e-07 ..
    3.0e-07, unmasked 2.2e-03 .. 2.3e-03."""
    import cohere_asr_refs as CR
    lens, x = RR.LENS[0], RR.features()
    l3 = RR.enc_lens(lens)
    for seed in (2, 5):
        _, ref = CR.hf_model(seed=seed, gain=8.0)
        with torch.no_grad():
            m32, m64, un = RR.cohere_kv(ref, x, lens), RR.cohere_kv(RR.double(ref), x, lens), RR.cohere_kv(ref, x, lens, masked=False)
            solo = RR.cohere_kv_solo(ref, x, lens)
        t, e32 = RR.tol(RR.valid_cat(m32, l3), RR.valid_cat(m64, l3))
        em, eu = RR.valid_err(m32, solo), RR.valid_err(un, solo)
        print(f"seed {seed}: tolerance {t:.2e}, masked vs solo {em:.2e}, unmasked vs solo {eu:.2e}")
        assert torch.isfinite(m32).all() and em <= t and eu >= 10 * t, (em, eu, t)


def test_new_entries_refuse_bad_arguments():
    """The `_lens` entries through ctypes: a null `lens` and every other null pointer DYN_E_ARG (-1), bad sizes -1, an unbuilt C / KW / act or
    a channel count the vectorised stage kernels do not take DYN_E_UNSUPPORTED (-4), a short workspace -3, an empty batch 0: all decided on the
    host, the dummy pointers are never dereferenced."""
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    p, big, B, T = 256, 1 << 40, 2, 8
    fwd = lambda lens, C=256, KW=9, act=0, B=B: lib.dyn_convmod_bn_fwd_lens(p, p, p, p, p, p, p, p, p, p, lens, B, T, C, KW, act, 1e-5, None)  # noqa: E731
    assert fwd(None) == -1 and b"dyn_convmod_bn_fwd_lens" in lib.dyn_last_error()
    assert fwd(p, C=300) == -4 and fwd(p, KW=31) == -4 and fwd(p, act=1) == -4 and fwd(p, B=-1) == -1 and fwd(p, B=0) == 0
    assert lib.dyn_convmod_bn_fwd(p, p, p, p, p, p, p, p, p, p, None, 0, T, 256, 9, 0, 1e-5, None) == 0          # the scalar entry still takes null
    bwd = lambda lens, C=256, ws=p, n=big: lib.dyn_convmod_bn_bwd_act_lens(p, p, p, p, p, p, p, p, p, p, 1.0, lens, B, T, C, 0, 1e-5, ws, n, None)  # noqa: E731
    assert bwd(None) == -1 and b"dyn_convmod_bn_bwd_act_lens" in lib.dyn_last_error()
    assert bwd(p, C=1280) == -4 and bwd(p, n=16) == -3 and bwd(p, ws=None) == -3
    dg = lambda lens, C=256, KW=9, du=1024: lib.dyn_glu_dwconv1d_dgrad_lens(p, p, 512, du, lens, B, T, C, KW, None)  # noqa: E731
    assert dg(None) == -1 and b"dyn_glu_dwconv1d_dgrad_lens" in lib.dyn_last_error()
    assert dg(p, KW=7) == -4 and dg(p, C=300) == -4 and dg(p, du=512) == -1                                        # du aliases dc
    sm = lambda lens, B=B, nh=2, T=T, ld=2 * T - 1, y=512: lib.dyn_softmax_relshift_fwd_lens(p, y, 1024, B, nh, T, ld, lens, None)  # noqa: E731
    assert sm(None) == -1 and b"dyn_softmax_relshift_fwd_lens" in lib.dyn_last_error()
    assert sm(p, ld=2 * T - 2) == -1 and sm(p, T=0) == -1 and sm(p, nh=0) == -1 and sm(p, T=16385, ld=40000) == -1 and sm(p, y=1024) == -1
    assert sm(p, B=0) == 0
    st = lambda f, *tail: f(p, p, p, 512, *tail)                                                                   # noqa: E731
    for C, rc in ((256, None), (6, -4)):
        for act in (0, 1, 2):
            want = -4 if (rc or act == 2) else 0
            assert st(lib.dyn_dwconv2d_s2_fwd_act_lens, 0 if want == 0 else B, T, 8, C, act, p, p, None) == want, (C, act, lib.dyn_last_error())
            assert st(lib.dyn_dwconv2d_s2_dgrad_act_lens, 0 if want == 0 else B, T, 8, C, act, p, p, None) == want
    assert st(lib.dyn_dwconv2d_s2_fwd_act_lens, B, T, 8, 256, 1, None, p, None) == -1 and b"dyn_dwconv2d_s2_fwd_act_lens" in lib.dyn_last_error()
    assert st(lib.dyn_dwconv2d_s2_fwd_act_lens, B, T, 8, 256, 1, p, None, None) == -1
    assert st(lib.dyn_dwconv2d_s2_dgrad_act_lens, B, T, 8, 256, 1, p, None, None) == -1
    assert st(lib.dyn_dwconv2d_s2_fwd_act_lens, B, 0, 8, 256, 1, p, p, None) == -1
    assert lib.dyn_dwconv2d_s2_fwd_act_lens(p, p, p, 516, B, T, 8, 256, 1, p, p, None) == -4                       # u not 16-byte aligned
    assert st(lib.dyn_conv2d_first_fwd_lens, B, T, 8, 256, None, None) == -1 and b"dyn_conv2d_first_fwd_lens" in lib.dyn_last_error()
    assert st(lib.dyn_conv2d_first_fwd_lens, B, T, 8, 6, p, None) == -4 and st(lib.dyn_conv2d_first_fwd_lens, 0, T, 8, 256, p, None) == 0
    assert lib.dyn_dwconv2d_s2_wgrad_act_lens(p, p, p, p, 1.0, B, T, 8, 256, 1, None, p, big, None) == -1
    assert lib.dyn_dwconv2d_s2_wgrad_act_lens(p, p, p, p, 1.0, B, T, 8, 256, 2, p, p, big, None) == -4
    assert lib.dyn_dwconv2d_s2_wgrad_act_lens(p, p, p, p, 1.0, B, T, 8, 6, 1, p, p, big, None) == -4
    assert lib.dyn_dwconv2d_s2_wgrad_act_lens(p, p, p, p, 1.0, B, T, 8, 256, 1, p, p, 16, None) == -3
    assert lib.dyn_conv2d_first_wgrad_lens(p, p, p, p, 1.0, B, T, 8, 256, None, p, big, None) == -1
    assert lib.dyn_conv2d_first_wgrad_lens(p, p, p, p, 1.0, B, T, 8, 6, p, p, big, None) == -4
    assert lib.dyn_conv2d_first_wgrad_lens(p, p, p, p, 1.0, B, T, 8, 256, p, p, 16, None) == -3
    assert lib.dyn_mask_rows_lens(p, B, T, 8, None, None) == -1 and b"dyn_mask_rows_lens" in lib.dyn_last_error()
    assert lib.dyn_mask_rows_lens(p, 65536, T, 8, p, None) == -1 and lib.dyn_mask_rows_lens(p, B, 0, 8, p, None) == -1
    assert lib.dyn_mask_rows_lens(p, 0, T, 8, p, None) == 0
    assert lib.dyn_softmax_fwd_lens(p, 512, B, 4, 8, 8, 8, None, None) == -1 and b"dyn_softmax_fwd_lens" in lib.dyn_last_error()
    assert lib.dyn_softmax_fwd_lens(p, 512, B, 0, 8, 8, 8, p, None) == -1 and lib.dyn_softmax_fwd_lens(p, 512, B, 4, 8, 7, 8, p, None) == -1
    assert lib.dyn_softmax_fwd_lens(p, 512, B, 4, 16385, 16385, 16385, p, None) == -4 and lib.dyn_softmax_fwd_lens(p, 512, 0, 4, 8, 8, 8, p, None) == 0
    desc = _lib.Seq2SeqDesc()
    assert lib.dyn_seq2seq_steps_len(ctypes.byref(desc), None, 0, 1, 0, None) == -1 and b"dyn_seq2seq_steps_len" in lib.dyn_last_error()
    assert lib.dyn_seq2seq_steps_len(None, p, 0, 1, 0, None) == -1
    assert lib.dyn_seq2seq_steps_len(ctypes.byref(desc), p, 0, 1, 0, None) == -1 and b"dyn_seq2seq_steps_len: null pointer" in lib.dyn_last_error()


@pytest.mark.parametrize("lens", RR.LENS, ids=[str(l) for l in RR.LENS])
def test_oracle_has_teeth_on_the_gpu_tests_inputs(lens):
    """transformers' ParakeetForCTC (toy arch, seed 0, default sdpa) on the GPU tests' features [3, 131, 80], zero-padded: on valid frames the
    masked batch lies within the tolerance of every row run alone at its own length, the unmasked batch at least ten times the tolerance
    away, and nothing is NaN.  A condition on the inputs, so that the GPU tests' bar cannot be met without the masks.
    Measured: tolerance 2.2e-05 .. 2.3e-05, masked 5.4e-07 .. 6.0e-07, unmasked 3.1e-03."""
    _, ref = R.hf_model()
    x = RR.features()
    with torch.no_grad():
        t, e32, _ = RR.model_tol(ref, RR.double(ref), x, lens)
        solo = RR.hf_solo(ref, x, lens)
        masked, unmasked = RR.hf_masked(ref, x, lens), RR.hf_unmasked(ref, x, lens)
    assert [s.shape[1] for s in solo] == RR.enc_lens(lens)
    assert torch.isfinite(masked).all() and torch.isfinite(unmasked).all()
    em, eu = RR.valid_err(masked, solo), RR.valid_err(unmasked, solo)
    print(f"lens {lens}: tolerance {t:.2e} (fp32 vs f64 {e32:.2e}), masked vs solo {em:.2e}, unmasked vs solo {eu:.2e}")
    assert em <= t, (em, t)
    assert eu >= 10 * t, (eu, t)
