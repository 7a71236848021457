"""What of ParakeetForTDT (parakeet_tdt_model.py), its loop (parakeet_tdt_lib.py), the host side of csrc/transducer.hip and the test-side
references (tests/transducer_refs.py) can be checked without a GPU, against transformers' ParakeetForTDT and tdt_loss."""
import argparse
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as PR  # noqa: E402
import transducer_refs as R  # noqa: E402


@pytest.mark.parametrize("layers", [1, 2])
def test_param_spec_is_transformers_state_dict(layers):
    from transformers import ParakeetForTDT
    from dynamic_asr_eval_amd import parakeet_model as PM, parakeet_tdt_model as TM
    cfg = R.hf_tdt_config(layers=layers)
    sd = ParakeetForTDT(cfg).state_dict()
    c = TM.make_config(cfg)
    hf_shape = {"pw": lambda s: s + (1,), "dw": lambda s: (s[0], 1) + s[1:], "pw2": lambda s: s + (1, 1), "sublin": lambda s: s, None: lambda s: s}
    ours = {n: hf_shape[kind](tuple(shape)) for n, shape, kind in TM.param_spec(c)}
    bufs = {n: tuple(shape) for n, shape, _ in PM.buffer_spec(c)}
    assert set(ours) | set(bufs) == set(sd) and not set(ours) & set(bufs)
    for n, shape in {**ours, **bufs}.items():
        assert tuple(sd[n].shape) == shape, (n, tuple(sd[n].shape), shape)
    assert not any(n.startswith("ctc_head.") for n in ours)
    assert ours["joint.head.weight"] == (R.TDT_VOCAB + 5, 64) and ours["decoder.embedding.weight"] == (R.TDT_VOCAB, 64)
    assert (f"decoder.lstm.weight_hh_l{layers - 1}" in ours) and (f"decoder.lstm.weight_hh_l{layers}" not in ours)
    names = [n for n, _, _ in TM.param_spec(c)]
    assert [n for n in names if not n.startswith("encoder.")] == [n for n in sd if not n.startswith("encoder.")]      # transformers' order


def test_make_config_reads_the_object_and_the_nested_dict():
    from dynamic_asr_eval_amd import parakeet_tdt_model as TM
    cfg = R.hf_tdt_config(durations=(0, 1, 2, 4))
    c = TM.make_config(cfg)
    assert TM.make_config(cfg.to_dict()) == c
    assert c["durations"] == (0, 1, 2, 4) and c["decoder_hidden_size"] == 64 and c["num_decoder_layers"] == 2 and c["vocab_size"] == R.TDT_VOCAB
    assert c["blank_token_id"] == R.TDT_BLANK and c["pad_token_id"] == R.TDT_PAD and c["joint_hidden_act"] == "relu" and c["hidden_act"] == "silu"
    assert c["max_symbols_per_step"] == 10 and c["decoder_start_token_id"] is None and c["hidden_size"] == 256
    d = TM.make_config()                                     # transformers' defaults: the released checkpoints' head
    assert (d["decoder_hidden_size"], d["num_decoder_layers"], d["vocab_size"], d["blank_token_id"], d["durations"]) == (640, 2, 8193, 8192, (0, 1, 2, 3, 4))


@pytest.mark.parametrize("word,over", [
    ("hidden_act", dict(hidden_act="gelu")), ("durations", dict(durations=list(range(9)))), ("negative", dict(durations=[-1, 0, 1])),
    ("unsorted", dict(durations=[0, 2, 1])), ("unsorted", dict(durations=[0, 1, 1])), ("positive", dict(durations=[0])),
    ("ParakeetForRNNT", dict(model_type="parakeet_rnnt")), ("decoder_hidden_size", dict(decoder_hidden_size=66)),
    ("blank_token_id", dict(blank_token_id=40))], ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(word, over):
    from dynamic_asr_eval_amd import parakeet_tdt_model as TM
    from dynamic_asr_eval_amd.ops import DynError
    base = R.hf_tdt_config().to_dict()
    with pytest.raises(DynError) as e:
        TM.make_config(dict(base, **over))
    assert word in str(e.value), str(e.value)


def test_rnnt_config_object_attention_mask_and_the_waveform_harness_are_refused(tmp_path):
    from transformers import ParakeetRNNTConfig
    from dynamic_asr_eval_amd import parakeet_tdt_model as TM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        TM.make_config(ParakeetRNNTConfig(vocab_size=33, blank_token_id=32, decoder_hidden_size=64, encoder_config=dict(PR.TOY)))
    assert "ParakeetForRNNT" in str(e.value) and "parakeet_rnnt" in str(e.value)
    with pytest.raises(DynError) as e:
        TM.ParakeetForTDT.forward(None, torch.zeros(1, 8, 80), decoder_input_ids=torch.zeros(1, 1, dtype=torch.int64), attention_mask=torch.ones(1, 8))
    assert "attention_mask" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(R.hf_tdt_config().to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "parakeet_tdt"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "parakeet_tdt" in str(e.value) and "parakeet_tdt_lib" in str(e.value)
    assert TM.config_from_json(str(d / "config.json")) == TM.make_config(R.hf_tdt_config())


RAGGED = [((1, 0), [1], [0], R.DURATIONS), ((1, 1), [1], [1], R.DURATIONS), ((2, 0), [2, 1], [0, 0], (1, 2)), ((5, 3), [5, 4], [3, 1], R.DURATIONS),
          ((9, 5), [9, 7, 4], [5, 0, 3], (0, 1)), ((9, 5), [9, 6, 9], [5, 5, 2], (1, 2)), ((12, 4), [12, 9], [4, 2], (0, 2, 5))]


@pytest.mark.parametrize("shape,T_b,U_b,durs", RAGGED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "")
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_float64_restatement_is_transformers_tdt_loss(shape, T_b, U_b, durs, sigma):
    """Loss per row and the autograd gradient of transformers' tdt_loss (fp32 inside) against the float64 restatement with its closed-form
    gradient, at ragged lengths: 2e-5 relative on the losses, 2e-5 absolute on the gradients (entries up to 1); rows past the lengths
    are exactly zero in both; beta(0, 0) and the alpha terminal agree (the lattice is consistent); the reductions agree."""
    (T, U), B, V1 = shape, len(T_b), 9
    x, tg = R.tdt_inputs(B, T, U, V1, len(durs), 3)
    want = R.tdt_ref(x, tg, T_b, U_b, V1 - 1, durs, sigma, "none")
    loss32, grad32 = R.tdt_torch_fp32(x, tg, T_b, U_b, V1 - 1, durs, sigma, "none")
    assert np.isfinite(want["nll"]).all()
    assert np.abs(loss32.numpy() - want["nll"]).max() <= 2e-5 * np.abs(want["nll"]).max()
    g32 = grad32.numpy()
    fin = np.isfinite(g32)           # torch's logsumexp backward is nan at cells no path reaches (no duration 0: u > t; no duration 1: t = 1)
    assert (fin.all() or tuple(durs[:2]) != (0, 1)) and fin.mean() > 0.5 and np.abs(g32 - want["grad"])[fin].max() <= 2e-5
    for b in range(B):
        row = want["rows"][b]
        assert np.all(want["grad"][b, T_b[b]:] == 0) and np.all(want["grad"][b, :, U_b[b] + 1:] == 0)
        assert np.all(g32[b, T_b[b]:][fin[b, T_b[b]:]] == 0) and np.all(g32[b, :, U_b[b] + 1:][fin[b, :, U_b[b] + 1:]] == 0)
        assert abs(row["beta"][0, 0] + row["nll"]) < 1e-12      # beta(0, 0) is the log-likelihood
        reach = np.isfinite(row["alpha"]) & np.isfinite(row["beta"])
        assert reach[0, 0] and np.all((row["alpha"] + row["beta"])[reach] <= -row["nll"] + 1e-9)      # no cell carries more than all paths
        assert abs(want["grad"][b].sum()) < 1e-9                # every row of a softmax gradient sums to zero
    for red in ("sum", "mean_batch") + (("mean_volume",) if sum(U_b) > 0 else ()) + (("mean",) if min(U_b) > 0 else ()):
        l32, gr32 = R.tdt_torch_fp32(x, tg, T_b, U_b, V1 - 1, durs, sigma, red)
        w = R.tdt_ref(x, tg, T_b, U_b, V1 - 1, durs, sigma, red)
        assert abs(float(l32) - w["loss"]) <= 2e-5 * abs(w["loss"]) and np.abs(gr32.numpy() - w["grad"])[fin].max() <= 2e-5, red


def test_float64_restatement_infeasible_lattice():
    x, tg = R.tdt_inputs(1, 2, 4, 9, 2, 0)
    want = R.tdt_ref(x, tg, [2], [4], 8, (1, 2))
    assert np.isposinf(want["nll"][0]) and np.all(want["grad"] == 0) and np.isfinite(want["grad"]).all()
    assert torch.isposinf(R.tdt_torch_fp32(x, tg, [2], [4], 8, (1, 2), 0.0, "none")[0]).all()


def test_merge_window_tokens():
    from dynamic_asr_eval_amd.parakeet_tdt_lib import merge_window_tokens as merge
    f = 8
    # no overlap: the seam.  Frame 16 * 8 = 128 is the second window's first input frame
    a = (0, 128, [1, 2, 3], [0, 7, 15])
    b = (128, 128, [4, 5], [16, 31])
    assert merge([a, b], f) == ([1, 2, 3, 4, 5], [0, 7, 15, 16, 31])
    # even overlap 64: windows [0, 128) and [64, 192), cut at 96 = frame 12; a token exactly on the boundary belongs to the later window
    a = (0, 128, [1, 2, 3, 9], [0, 11, 12, 15])
    b = (64, 128, [4, 5, 6, 7], [8, 11, 12, 20])
    assert merge([a, b], f) == ([1, 2, 6, 7], [0, 11, 12, 20])
    # odd overlap in frames of the factor: overlap 24 -> cut at 128 - 12 = 116 = frame 14.5: frame 14 stays, frame 15 moves
    a = (0, 128, [1, 2, 3], [13, 14, 15])
    b = (104, 128, [4, 5, 6], [13, 14, 15])
    assert merge([a, b], f) == ([1, 2, 6], [13, 14, 15])
    # a shorter last window, three windows, shuffled insertion order: [0, 128), [64, 192), [128, 236): cuts at 96 and 160
    w0 = (0, 128, [1, 2], [5, 12])
    w1 = (64, 128, [3, 4, 5], [11, 12, 20])
    w2 = (128, 108, [6, 7, 8], [19, 20, 28])
    want = ([1, 4, 7, 8], [5, 12, 20, 28])
    for order in ([w0, w1, w2], [w2, w0, w1], [w1, w2, w0]):
        assert merge(order, f) == want
    assert merge([w1], f) == ([3, 4, 5], [11, 12, 20])          # one window owns everything
    assert merge([], f) == ([], [])
    # the references' independent restatement agrees on random windows
    rng = random.Random(5)
    for _ in range(50):
        n, ov = rng.randint(1, 5), rng.choice([0, 8, 16, 24, 64])
        starts = [k * (128 - ov) for k in range(n)]
        lens = [128] * (n - 1) + [rng.choice([128, 100, 40])]
        wins = [[(rng.randint(0, 30), s // f + rng.randint(0, 15)) for _ in range(rng.randint(0, 6))] for s in starts]
        wins = [sorted(w, key=lambda p: p[1]) for w in wins]
        order = list(range(n))
        rng.shuffle(order)
        got = merge([(starts[i], lens[i], [k for k, _ in wins[i]], [fr for _, fr in wins[i]]) for i in order], f)
        assert got == R.merged_ref(wins, starts, lens, f)


def test_header_entries_are_exported_and_refuse_before_any_launch():
    """The new C-ABI entries are in include/dyneval.h and in the library; argument errors come back as codes before any launch, so dummy
    pointers are never dereferenced: DYN_E_ARG (-1) for null pointers, bad sizes and bad duration lists, DYN_E_UNSUPPORTED (-4) for a joint
    activation other than relu, DYN_E_WORKSPACE (-3) for a short workspace and, by name, for a lattice over the budget."""
    import ctypes
    from dynamic_asr_eval_amd import _lib
    names = ("dyn_lstm_cell_fwd", "dyn_lstm_cell_bwd", "dyn_joint_fwd", "dyn_joint_bwd", "dyn_tdt_loss", "dyn_tdt_loss_workspace_bytes",
             "dyn_tdt_loss_workspace_layout", "dyn_tdt_greedy_steps")
    assert set(names) <= set(_lib.exported_symbols())
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n
    p, big = 256, 1 << 40
    dur = lambda *d: ctypes.cast((ctypes.c_int32 * len(d))(*d), ctypes.c_void_p)                 # noqa: E731
    assert lib.dyn_lstm_cell_fwd(None, p, None, p, p, None, 2, 64, None) == -1 and lib.dyn_lstm_cell_fwd(p, p, None, p, p, None, 0, 64, None) == -1
    assert lib.dyn_lstm_cell_bwd(p, None, None, None, p, p, p, 2, 64, None) == -1
    assert lib.dyn_joint_fwd(p, p, p, 1, 2, 3, 64, 0, 64, 1, None) == -4 and b"hidden_act" in lib.dyn_last_error()
    assert lib.dyn_joint_bwd(p, p, p, p, 1, 2, 3, 64, 0, 192, 64, 1, None) == -4
    assert lib.dyn_joint_fwd(p, p, p, 1, 2, 3, 66, 0, 66, 0, None) == -1 and lib.dyn_joint_fwd(p, p + 4, p, 1, 2, 3, 64, 0, 64, 0, None) == -1
    assert lib.dyn_joint_bwd(p, p, None, None, 1, 2, 3, 64, 0, 192, 64, 0, None) == -1
    need = lib.dyn_tdt_loss_workspace_bytes(2, 9, 6, 5)
    assert need >= 2 * 9 * 6 * (7 + 2 + 1 + 1) * 4 and lib.dyn_tdt_loss_workspace_bytes(0, 9, 6, 5) == -1
    args = lambda d, D, ws=p, wsb=big, budget=0, blank=8, red=0: (p, 2, 9, 6, 9, d, D, p, 5, p, p, blank, 0.0, red, 1.0, p, p, p, ws, wsb, budget, None)   # noqa: E731
    for d, D in ((dur(0, 1, 2, 3, 4, 5, 6, 7, 8), 9), (dur(-1, 1), 2), (dur(0, 2, 1), 3), (dur(1, 1), 2), (dur(0), 1), (None, 2)):
        assert lib.dyn_tdt_loss(*args(d, D)) == -1, lib.dyn_last_error()
        assert b"dyn_tdt_loss" in lib.dyn_last_error()
    assert lib.dyn_tdt_loss(*args(dur(0, 1, 2, 3, 4), 5, blank=9)) == -1 and lib.dyn_tdt_loss(*args(dur(0, 1, 2, 3, 4), 5, red=5)) == -1
    assert lib.dyn_tdt_loss(*args(dur(0, 1, 2, 3, 4), 5, wsb=need - 1)) == -3 and lib.dyn_tdt_loss(*args(dur(0, 1, 2, 3, 4), 5, ws=None)) == -3
    assert lib.dyn_tdt_loss(*args(dur(0, 1, 2, 3, 4), 5, budget=need - 1)) == -3
    assert b"budget" in lib.dyn_last_error() and b"chunking" in lib.dyn_last_error()
    g = lambda d, D, B=2, n_steps=1, blank=32: (p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, B, 17, 64, 2, 33, d, D, blank, 170, 170, n_steps, None)   # noqa: E731
    assert lib.dyn_tdt_greedy_steps(*g(dur(0, 2, 1), 3)) == -1 and lib.dyn_tdt_greedy_steps(*g(dur(0, 1), 2, B=0)) == -1
    assert lib.dyn_tdt_greedy_steps(*g(dur(0, 1), 2, blank=33)) == -1 and lib.dyn_tdt_greedy_steps(*g(dur(0, 1), 2, n_steps=-1)) == -1
    assert lib.dyn_tdt_greedy_steps(*((None,) + g(dur(0, 1), 2)[1:])) == -1


def test_ops_refuse_on_the_host():
    from dynamic_asr_eval_amd import ops
    for bad, word in (([0, 1, 2, 3, 4, 5, 6, 7, 8], "9 durations"), ([-1, 0], "negative"), ([0, 2, 1], "unsorted"), ([0], "positive")):
        with pytest.raises(ops.DynError) as e:
            ops.check_durations(bad)
        assert word in str(e.value)
    assert ops.check_durations([1, 2]) == (1, 2) and ops.check_durations((0, 1, 2, 3, 4, 5, 6, 7)) == tuple(range(8))
    with pytest.raises(ops.DynError) as e:
        ops.joint(torch.zeros(1, 2, 64), torch.zeros(1, 3, 64), act="gelu")
    assert "hidden_act" in str(e.value) and "gelu" in str(e.value)
    with pytest.raises(ops.DynError):
        ops.joint(torch.zeros(1, 2, 64), torch.zeros(1, 3, 64))            # host tensors: there is no CPU path


def test_decode_oracle_satisfies_the_gpu_tests_conditions():
    """transformers' greedy TDT decode on the inputs tests/test_parakeet_tdt_gpu.py gives generate() (transducer_refs.DECODE): the smallest
    top-2 margin over every token and every duration argmax is at least 1e-2, at least a quarter of the steps are non-blank and at least
    one is blank, at least three distinct durations occur, at least one non-blank is emitted with duration 0; no row runs into the step
    cap."""
    ref = R.decode_model()[1]
    for B in (1, 3):
        rows, Tp, (mt, md) = R.decode_case(B, ref)
        R.assert_decode_conditions(rows, mt, md)
        assert Tp == 38 and all(len(r["steps"]) < ref.config.max_symbols_per_step * Tp - 1 for r in rows)
