"""Holds the oracle (CPU tests) and the HIP kernels (-m gpu tests) to tests/golden/reference_pins.{npz,json}: outputs that
the REFERENCE'S OWN functions / statements produced when executed unchanged via ast extraction in the build container
(tests/golden/make_reference_pins.py).  Covered: frame_shuffle / add_random_noise / cutout (lcasr/lib.py:81-84,379-417),
the four arg->config helpers (:102-125,419-428), the stitch statements (lcasr/lib.py:615-629 and run_seq_eval.py:130-144),
the TEDLIUM STM text handling (tedlium/run.py:25-51) and SoftDTW._euclidean_dist_func (wav2vec2/soft_dtw_cuda.py:319-329)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "reference_pins.npz")), json.load(open(os.path.join(GOLD, "reference_pins.json")))


AUG_SHUFFLE = (("t", dict(time_dimension=True)), ("f", dict(freq_dimension=True)), ("tf", dict(time_dimension=True, freq_dimension=True)))


def _stitch_inputs(arr, case, tag, ci):
    flat = torch.from_numpy(arr[f"stitch_{tag}_{ci}_in"])
    mo, row = {}, 0
    for k, ds in zip(case["keys"], case["ds_len"]):
        mo[k] = {"logits": flat[row:row + ds][None], "ds_len": ds, "overlap_ds": case["overlap_ds"]}
        row += ds
    return mo


# ------------------------------------------------------------------------------------------------ CPU: oracle / host logic
def test_oracle_augmentations_reproduce_the_reference_outputs(pins):
    from oracle import augment_ref as R
    arr, meta = pins
    spec = torch.from_numpy(arr["aug_spec"])
    for tag, kw in AUG_SHUFFLE:
        torch.manual_seed(meta["aug_seeds"]["frame_shuffle"])
        assert np.array_equal(R.frame_shuffle(spec.clone(), **kw).numpy(), arr[f"frame_shuffle_{tag}"]), tag
    torch.manual_seed(meta["aug_seeds"]["noise"])
    assert np.array_equal(R.add_random_noise(spec.clone(), 0.3).numpy(), arr["noise_0p3"])
    for val in ("mean", "mean_recording", "zero"):
        torch.manual_seed(meta["aug_seeds"]["cutout"])
        got = R.cutout(spec.clone(), 600, cutout_val=val, num_rectangles=7, max_width=100, max_height=10).numpy()
        assert np.array_equal(got, arr[f"cutout_{val}"]), val
    torch.manual_seed(meta["aug_seeds"]["cutout_short"])
    got = R.cutout(spec[:, :, :250].clone(), 600, cutout_val="mean", num_rectangles=7, max_width=40, max_height=6).numpy()
    assert np.array_equal(got, arr["cutout_short"])


def test_arg_helpers_reproduce_the_reference_dicts(pins):
    from dynamic_asr_eval_amd import lib
    _, meta = pins
    for case in meta["arg_cases"]:
        a = argparse.Namespace(**case["args"])
        assert lib.get_specaugment_config_from_args(a) == case["specaugment"]
        assert lib.get_frame_shuffle_config_from_args(a) == case["frame_shuffle"]
        assert lib.get_lr_args_from_args(a) == case["lr"]
        assert lib.get_cutout_params_from_args(a, 16384) == case["cutout"]


@pytest.mark.parametrize("tag", ["inner", "outer"])
def test_oracle_stitch_reproduces_the_reference_statements(pins, tag):
    from oracle.dynamic_eval_ref import stitch_ref
    arr, meta = pins
    for ci, case in enumerate(meta[f"stitch_{tag}"]):
        mo = _stitch_inputs(arr, case, tag, ci)
        C, rows = case["classes"], case["acc_rows"]
        out = stitch_ref(mo, torch.zeros(1, rows, C), torch.zeros(1, rows, C))[0].numpy()
        want = arr[f"stitch_{tag}_{ci}_out"]
        # equal to the last bit on the machine that made the pins (same CPU model, torch build and thread count as the loop pins' record: both
        # fixture sets were generated in the build container); another CPU's vectorised log may differ in the last place
        assert out.shape == want.shape == (case["out_rows"], C)
        if _generating_machine() and os.environ.get("DYN_PINS_STRICT", "1") == "1":
            assert np.array_equal(out, want), (tag, ci, float(np.abs(out - want).max()))
        else:
            assert np.abs(out - want).max() <= 1e-6 and np.array_equal(out.argmax(-1), want.argmax(-1)), (tag, ci)


def test_fetch_utterances_reproduces_the_reference(pins, tmp_path):
    """wav2vec2/tedlium/run.py:56-83: the utterance list `dynamic_eval_su` is fed (sample ranges, per-utterance text, joined text)."""
    from dynamic_asr_eval_amd.datasets import fetch_utterances
    _, meta = pins
    ref = meta["fetch_utterances"]
    stm = tmp_path / "talk.stm"
    stm.write_text("\n".join(meta["stm"]["lines"]))
    wave = torch.arange(ref["wave_samples"], dtype=torch.float32)[None] * 0.5
    utts, all_text = fetch_utterances(str(stm), wave, ref["sample_rate"])
    assert all_text == ref["all_text"] and len(utts) == len(ref["utterances"])
    for u, r in zip(utts, ref["utterances"]):
        assert (u["start"], u["end"], u["text"], u["start_frame"], u["end_frame"]) == (r["start"], r["end"], r["text"], r["start_frame"], r["end_frame"])
        assert list(u["waveform"].shape) == r["shape"] and float(u["waveform"][0, 0]) == r["first"] and float(u["waveform"][0, -1]) == r["last"]
        assert u["waveform"].data_ptr() == wave[:, r["start_frame"]:].data_ptr()          # a view of the resident talk, not a copy


def test_stm_text_handling_reproduces_the_reference(pins):
    from dynamic_asr_eval_amd.datasets import proc_stm_lines
    _, meta = pins
    text, timings, remove = proc_stm_lines(meta["stm"]["lines"])
    assert text == meta["stm"]["text"] and timings == meta["stm"]["timings"] and remove == meta["stm"]["remove_timings"]


def test_oracle_sqdist_reproduces_the_reference(pins):
    from oracle.softdtw_ref import sqdist
    arr, _ = pins
    for tag in "abc":
        want = arr[f"sqdist_{tag}_d"]
        got = sqdist(arr[f"sqdist_{tag}_x"], arr[f"sqdist_{tag}_y"])
        assert got.shape == want.shape and np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), tag


# ------------------------------------------------------------------------------------------------ GPU: the HIP path
@pytest.mark.gpu
def test_device_augmentations_reproduce_the_reference_outputs(cuda, pins):
    """augment.frame_shuffle / add_random_noise / cutout draw from the caller's torch CPU RNG in the reference's order and move
    the data on the device: same seeds -> the reference's own outputs (shuffles bit-exact; means/noise to fp32 rounding)."""
    from dynamic_asr_eval_amd import augment
    arr, meta = pins
    spec = torch.from_numpy(arr["aug_spec"])

    def dev():
        return spec[0].to(cuda).clone()

    for tag, kw in AUG_SHUFFLE:
        torch.manual_seed(meta["aug_seeds"]["frame_shuffle"])
        assert np.array_equal(augment.frame_shuffle(dev(), **kw).cpu().numpy(), arr[f"frame_shuffle_{tag}"][0]), tag
    torch.manual_seed(meta["aug_seeds"]["noise"])
    got = augment.add_random_noise(dev(), 0.3).cpu().numpy()
    assert np.abs(got - arr["noise_0p3"][0]).max() < 2e-5
    for val in ("mean", "mean_recording", "zero"):
        torch.manual_seed(meta["aug_seeds"]["cutout"])
        got = augment.cutout(dev(), 600, cutout_val=val, num_rectangles=7, max_width=100, max_height=10).cpu().numpy()
        assert np.abs(got - arr[f"cutout_{val}"][0]).max() < 2e-6, val
    torch.manual_seed(meta["aug_seeds"]["cutout_short"])
    got = augment.cutout(spec[0, :, :250].contiguous().to(cuda), 600, cutout_val="mean", num_rectangles=7, max_width=40, max_height=6).cpu().numpy()
    assert np.abs(got - arr["cutout_short"][0]).max() < 2e-6


@pytest.mark.gpu
def test_device_stitch_reproduces_the_reference_statements(cuda, pins):
    """dyn_stitch_accumulate / dyn_stitch_finalize (the loop's accumulators in HBM) and run_seq_eval.outer_stitch against the
    outputs of the reference's stitch statements, short tail windows and a tail that lands inside earlier coverage included."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.run_seq_eval import outer_stitch
    arr, meta = pins
    for ci, case in enumerate(meta["stitch_inner"]):
        mo = _stitch_inputs(arr, case, "inner", ci)
        C, rows = case["classes"], case["acc_rows"]
        acc = torch.zeros(rows, C, device=cuda); cnt = torch.zeros(rows, device=cuda)
        pos = end = 0
        for k in sorted(mo):                                    # the position rule of _loop.Stitcher.add
            pos -= mo[k]["overlap_ds"] if k != 0 else 0
            ops.stitch_accumulate(torch.log(mo[k]["logits"][0]).to(cuda).contiguous(), acc, cnt, pos)
            pos += mo[k]["ds_len"]
            end = max(end, pos)
        got = ops.stitch_finalize(acc, cnt, end).cpu().numpy()
        want = arr[f"stitch_inner_{ci}_out"]
        assert got.shape == want.shape and np.abs(got - want).max() < 5e-6, ci
    for ci, case in enumerate(meta["stitch_outer"]):
        mo = _stitch_inputs(arr, case, "outer", ci)
        # outer_stitch derives overlap_ds = int(overlap / (u_len / ds_len)): u_len = 8 * ds_len, overlap = 8 * overlap_ds
        wins = [(k, torch.log(mo[k]["logits"][0]).to(cuda).contiguous(), 8 * mo[k]["ds_len"]) for k in mo]
        got = outer_stitch(wins, 8 * case["overlap_ds"], case["classes"], cuda).cpu().numpy()
        want = arr[f"stitch_outer_{ci}_out"]
        assert got.shape == want.shape and np.abs(got - want).max() < 5e-6, ci


@pytest.mark.gpu
def test_device_sqdist_reproduces_the_reference(cuda, pins):
    from dynamic_asr_eval_amd.soft_dtw import sqdist
    arr, _ = pins
    for tag in "abc":
        want = arr[f"sqdist_{tag}_d"]
        got = sqdist(torch.from_numpy(arr[f"sqdist_{tag}_x"]).to(cuda), torch.from_numpy(arr[f"sqdist_{tag}_y"]).to(cuda)).cpu().numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), tag


def test_teacher_filters_reproduce_the_reference_decisions(pins):
    """enc_dec_teacher_filters: same flag defaults and, case by case, the same (skip, reason) as the reference's
    should_skip_faulty_teacher_prediction executed unchanged."""
    from dynamic_asr_eval_amd.enc_dec_teacher_filters import add_enc_dec_teacher_filter_args, should_skip_faulty_teacher_prediction
    _, meta = pins
    defaults = vars(add_enc_dec_teacher_filter_args(argparse.ArgumentParser()).parse_args([]))
    assert defaults == meta["teacher_filter_defaults"]
    for case in meta["teacher_filter_cases"]:
        a = argparse.Namespace(**dict(defaults, **case["flags"]))
        skip, reason = should_skip_faulty_teacher_prediction(args=a, teacher_pred_tokens=case["tokens"], teacher_pred_text=case["text"],
                                                             spec_frames=case["frames"], **case["extra"])
        assert (bool(skip), reason) == (case["skip"], case["reason"]), case


# ------------------------------------------------------------------------------------------------ CPU: the loop restatements as a whole
# tests/golden/loop_pins.{npz,json}: outputs of the REFERENCE'S OWN loop functions (lcasr/lib.py:450-640 dynamic_eval_ctc_loss, :206-376 AWMC,
# run_half_concat_eval.py:64-160 adapt_on_concat_only, wav2vec2/lib.py:293-462 dynamic_eval_ctc_loss_su) executed unchanged via ast extraction
# on toy models, with the un-vendored leaf classes bound to the oracle's own (tests/golden/make_loop_pins.py says which).  What is pinned is
# loop order and glue arithmetic: window order / shuffle, which copy is augmented and which gives the labels, the / (N * B) and / (N * B * 2)
# scalings, zero_grad / backward / step order (clip -> step -> zero_grad in the wav2vec2 loop), online vs final pass, epochs under online,
# overlap_ds, the -1 defaults from args.config, the stitch, return_params and the restore.  Same torch, same CPU ops on both sides: the
# comparison is bit-for-bit on the machine that generated the pins and 2e-5 + identical argmax elsewhere (other BLAS code paths).
LOOP_TOL = 2e-5


def _generating_machine():
    """True on the machine class that generated the fixtures (CPU model, torch build, thread count recorded in loop_pins.json)."""
    rec = json.load(open(os.path.join(GOLD, "loop_pins.json")))["machine"]
    cpu = ""
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            cpu = line.split(":", 1)[1].strip()
            break
    return cpu == rec["cpu"] and torch.__version__ == rec["torch"] and torch.get_num_threads() == rec["threads"]


@pytest.fixture(scope="module")
def loop_pins():
    import sys
    sys.path.insert(0, GOLD)
    import loop_pin_cases as C
    arr, meta = np.load(os.path.join(GOLD, "loop_pins.npz")), json.load(open(os.path.join(GOLD, "loop_pins.json")))
    return arr, meta, C, _generating_machine()


def _held(got, want, same_machine, what, argmax=True, tol=LOOP_TOL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if same_machine and os.environ.get("DYN_PINS_STRICT", "1") == "1":
        assert np.array_equal(got, want), f"{what}: not bit-identical on the generating machine (max |d| {np.abs(got - want).max():.3e})"
    else:
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)) and np.abs(got[fin] - want[fin]).max() <= tol, what
        if argmax:
            assert np.array_equal(got.argmax(-1), want.argmax(-1)), what


def _fixed_masks(C, spec, seq_len, overlap):
    from oracle import dynamic_eval_ref as R
    data, keys = R.prepare_chunks(spec, seq_len, overlap)
    return {k: C.content_masks(data[k][0]) for k in keys}


class _CountingTokenizer:
    """Counts the pseudo-label ids the loop trained on (the toy runs must exercise the CTC glue with non-empty targets)."""
    def __init__(self, tok):
        self.tok, self.n = tok, 0

    def vocab_size(self):
        return self.tok.vocab_size()

    def decode(self, ids):
        return self.tok.decode(ids)

    def encode(self, text):
        ids = self.tok.encode(text)
        self.n += len(ids)
        return ids


def _resolve(args, seq_len, overlap, spec_n):
    """seq_len / overlap as the reference resolves them (lcasr/lib.py:466,501-504)."""
    seq_len = seq_len if seq_len != -1 else args.config['audio_chunking']['size']
    if seq_len > spec_n:
        return spec_n, 0
    return seq_len, overlap if overlap != -1 else args.config['audio_chunking']['overlap']


def test_oracle_dynamic_eval_reproduces_the_reference_function(loop_pins):
    import random
    from dynamic_asr_eval_amd import lib
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD
    arr, meta, C, same = loop_pins
    tok = _CountingTokenizer(C.tokenizer_128())
    for tag, (T, seq_len, overlap, kw) in C.DYNEVAL_CASES.items():
        m = meta["dyneval"][tag]
        assert (m["frames"], m["seq_len"], m["overlap"], m["args"]) == (T, seq_len, overlap, kw), f"{tag}: case table and fixture disagree"
        args = C.toy_args(**kw)
        model = C.toy_model(seed=m["model_seed"])
        spec = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(m["spec_seed"]))
        sl, ov = _resolve(args, seq_len, overlap, T)
        random.seed(m["random_seed"]); torch.manual_seed(m["torch_seed"])
        out, params = R.dynamic_eval_ref(model, spec, sl, ov, tok, MADGRAD, lib.get_lr_args_from_args(args),
                                         lib.get_specaugment_config_from_args(args), epochs=kw.get("epochs", 1), shuffle=kw.get("shuffle", False),
                                         online=kw.get("online", False), fixed_masks=_fixed_masks(C, spec, sl, ov), return_params=True)
        _held(out, arr[f"dyneval_{tag}_out"], same, f"dynamic_eval_ctc_loss[{tag}] stitched log-probs")
        digest, psum = C.params_digest(params)
        _held(digest, arr[f"dyneval_{tag}_params"], same, f"dynamic_eval_ctc_loss[{tag}] updated parameters", argmax=False)
        assert abs(psum[1] - m["params_sum"][1]) <= 1e-6 * m["params_sum"][1]
    assert tok.n > 300, f"the toy runs must carry non-empty pseudo-labels, or the CTC glue is not exercised ({tok.n} ids)"


def test_oracle_awmc_reproduces_the_reference_function(loop_pins):
    from dynamic_asr_eval_amd import lib
    from oracle.awmc_ref import awmc_ref
    from oracle.madgrad_ref import MADGRAD
    arr, meta, C, same = loop_pins
    tok = C.tokenizer_128()
    for tag, (T, seq_len, overlap, kw) in C.AWMC_CASES.items():
        m = meta["awmc"][tag]
        args = C.toy_args(**kw)
        model = C.toy_model(seed=m["model_seed"])
        spec = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(m["spec_seed"]))
        out, params = awmc_ref(model, spec, seq_len, overlap, tok, MADGRAD, lib.get_lr_args_from_args(args), lib.get_specaugment_config_from_args(args),
                               epochs=kw["epochs"], ema_decay=kw.get("ema_decay", 0.999), fixed_masks=_fixed_masks(C, spec, seq_len, overlap),
                               return_params=True)
        _held(out, arr[f"awmc_{tag}_out"], same, f"AWMC[{tag}] stitched log-probs")
        _held(C.params_digest(params)[0], arr[f"awmc_{tag}_params"], same, f"AWMC[{tag}] updated parameters", argmax=False)


def test_oracle_adapt_on_concat_only_reproduces_the_reference_function(loop_pins):
    """run_half_concat_eval.py:64-160 = Loop A of dynamic eval (or AWMC with return_params) on the concatenation: the oracle has no separate
    restatement of it, `dynamic_eval_ref(..., return_params=True)` / `awmc_ref` on the concatenated spectrogram IS the claim being pinned."""
    from dynamic_asr_eval_amd import lib
    from oracle import dynamic_eval_ref as R
    from oracle.awmc_ref import awmc_ref
    from oracle.madgrad_ref import MADGRAD
    arr, meta, C, same = loop_pins
    tok = C.tokenizer_128()
    for tag, lens, kw, adapt_overlap in C.CONCAT_CASES:
        m = meta["concat"][tag]
        args = C.toy_args(**kw)
        model = C.toy_model(seed=m["model_seed"])
        g = torch.Generator().manual_seed(m["spec_seed"])
        concat = torch.cat([torch.randn(1, 80, n, generator=g) for n in lens], dim=-1)
        sl, ov = _resolve(args, kw["seq_len"], adapt_overlap, concat.shape[-1])
        masks = _fixed_masks(C, concat, sl, ov)
        if kw["awmc"]:
            _, params = awmc_ref(model, concat, sl, ov, tok, MADGRAD, lib.get_lr_args_from_args(args), {}, epochs=kw["epochs"], fixed_masks=masks,
                                 return_params=True)
        else:
            _, params = R.dynamic_eval_ref(model, concat, sl, ov, tok, MADGRAD, lib.get_lr_args_from_args(args), {}, epochs=kw["epochs"],
                                           fixed_masks=masks, return_params=True)
        _held(C.params_digest(params)[0], arr[f"concat_{tag}_params"], same, f"adapt_on_concat_only[{tag}]", argmax=False)


def test_oracle_wav2vec2_su_loop_reproduces_the_reference_function(loop_pins):
    """wav2vec2/lib.py:293-462 on a toy transformers Wav2Vec2ForCTC.  The reference normalises through the HF feature extractor (numpy),
    the oracle restates the rule in torch: 1e-5 instead of bit-identity, argmax identical."""
    import argparse
    import random
    import sys
    sys.path.insert(0, GOLD)
    import tests_w2v2_toy as toy
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD
    arr, meta, C, same = loop_pins
    for tag, kw, lr in C.SU_CASES:
        m = meta["su"][tag]
        model = toy.model(seed=m["model_seed"])
        utts = toy.utterances(seed=m["utt_seed"])
        random.seed(m["random_seed"])
        out = dynamic_eval_su_ref(argparse.Namespace(**kw), model, utts, toy.CharTokenizer(), MADGRAD, lr_args={'lr': lr})
        assert len(out) == m["n"]
        moved = 0.0
        for k, u in enumerate(out):
            want = arr[f"su_{tag}_probs{k}"]
            got = u['probs'].numpy()
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5, (tag, k, np.abs(got - want).max())
            assert np.array_equal(got.argmax(-1), want.argmax(-1))
            if k:
                moved = max(moved, float(np.abs(want).max()))
        assert moved > 0


def test_oracle_cross_dataset_loop_reproduces_the_reference_statements(loop_pins):
    """BASELINE config 5's outer loop: reference lcasr/run_cross_dataset_eval.py:82-94,96-218 executed unchanged on toy recordings
    (eval_fn = the reference's own dynamic_eval_ctc_loss) against oracle/cross_dataset_ref.py driving oracle.dynamic_eval_ref: every scored
    corpus' hypotheses in scoring order, and the four result entries."""
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.wer import basic_normalize
    from oracle import dynamic_eval_ref as R
    from oracle.cross_dataset_ref import cross_dataset_ref, oracle_eval_fn
    from oracle.madgrad_ref import MADGRAD
    from oracle.wer_ref import word_error_rate_detail
    arr, meta, C, same = loop_pins
    tok = C.tokenizer_128()
    dec = C.OracleGreedyCTCDecoder(tok, C.VOCAB)
    for tag, lens_a, lens_b, kw in C.CROSS_CASES:
        m = meta["cross"][tag]
        assert (m["lens_a"], m["lens_b"], m["args"]) == (list(lens_a), list(lens_b), kw)
        model = C.toy_model(seed=m["model_seed"])
        before = [p.clone() for p in model.parameters()]
        args = C.toy_args(dataset="toy_a", dataset2="toy_b", **kw)
        eval_fn = oracle_eval_fn(MADGRAD, lib.get_lr_args_from_args, lib.get_specaugment_config_from_args,
                                 lambda spec, sl, ov: _fixed_masks(C, spec, sl, ov))
        transcribe = lambda logits: basic_normalize(dec(torch.as_tensor(logits))).lower()   # noqa: E731
        # (1) as the statements evaluate on the CPU, where `.to(p.device)` aliases (oracle/cross_dataset_ref.py docstring): the pin's own mode
        scored = []
        res = cross_dataset_ref(args, model, C.toy_records(lens_a, m["seeds"][0]), C.toy_records(lens_b, m["seeds"][1]), eval_fn, tok,
                                transcribe, word_error_rate_detail, record=scored, device_copies=False)
        assert [h for _, _, h in scored] == m["scored_hypotheses"], f"{tag}: hypotheses differ from the reference's run"
        assert [p for p, _, _ in scored] == ["a_baseline", "b_baseline"] + ["a_to_b", "a_to_a_loo"] * len(lens_a)
        for k in ("a_baseline", "b_baseline", "a_to_b", "a_to_a_loo"):
            assert res[0][k] == m["results"][k], (tag, k)
        # (2) with copies, as on a GPU: the baselines and iteration 0 are the same numbers, and the weights really come back
        model = C.toy_model(seed=m["model_seed"])
        res2 = cross_dataset_ref(args, model, C.toy_records(lens_a, m["seeds"][0]), C.toy_records(lens_b, m["seeds"][1]), eval_fn, tok,
                                 transcribe, word_error_rate_detail, device_copies=True)
        assert res2[0]["a_baseline"] == m["results"]["a_baseline"] and res2[0]["b_baseline"] == m["results"]["b_baseline"]
        assert res2[0]["a_to_b"][0] == m["results"]["a_to_b"][0] and res2[0]["a_to_a_loo"][0] == m["results"]["a_to_a_loo"][0]
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())), "weights restored after the last i (:197-198)"
