"""What of ParakeetForRNNT (parakeet_rnnt_model.py), the host side of the RNN-T entries of csrc/transducer.hip and the test-side references
(tests/rnnt_refs.py) can be checked without a GPU.  transformers' rnnt_loss needs torchaudio, which is not a dependency: the references pin
each other instead (float64 lattice with its closed-form gradient, torch recursion with autograd, brute force over all alignments)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parakeet_refs as PR  # noqa: E402
import rnnt_refs as R  # noqa: E402
import transducer_refs as TR  # noqa: E402


@pytest.mark.parametrize("T,U", [(1, 0), (1, 3), (3, 0), (4, 3), (5, 2)])
def test_recursion_closed_form_gradient_and_brute_force_agree(T, U):
    """The float64 lattice with its closed-form gradient, the torch recursion with autograd (float64) and the sum over all C(T - 1 + U, U)
    alignments agree to 1e-12 in the NLL and in every entry of the gradient; the blank is not the last class, the tensor is larger
    than the lattice and the gradient is exactly zero outside [:T, :U + 1]."""
    V1, pad_t, pad_u = 6, 2, 1
    x, tg, blank = R.rnnt_inputs(1, T + pad_t, U + pad_u, V1, 3)
    assert blank == V1 - 2 and not (tg == blank).any()
    want = R.rnnt_ref(x, tg, [T], [U], blank, "none")
    row = want["rows"][0]
    nll_t, g_t = R.rnnt_torch(x, tg, [T], [U], blank, "none", dtype=torch.float64)
    nll_b, g_b = R.rnnt_brute(x[0, :T, :U + 1].double().numpy(), tg[0].numpy(), T, U, blank)
    assert abs(row["nll"] - float(nll_t[0])) <= 1e-12 and abs(row["nll"] - nll_b) <= 1e-12
    assert np.abs(want["grad"][0] - g_t[0].numpy()).max() <= 1e-12
    assert np.abs(want["grad"][0, :T, :U + 1] - g_b).max() <= 1e-12
    assert np.all(want["grad"][0, T:] == 0) and np.all(want["grad"][0, :, U + 1:] == 0)
    assert np.all(g_t[0, T:].numpy() == 0) and np.all(g_t[0, :, U + 1:].numpy() == 0)
    assert np.abs(want["grad"][0, :T, :U + 1]).max() > 0
    assert abs(row["alpha"][T - 1, U] + x[0].double().log_softmax(-1)[T - 1, U, blank].item() + row["nll"]) <= 1e-12      # the alpha terminal
    assert np.abs(want["grad"][0].sum(-1)).max() < 1e-12                        # every row of a softmax gradient sums to zero


def test_reference_ragged_rows_reductions_and_unreachable_lattices():
    """Ragged T_b / U_b: the gradient is zero outside [:T_b, :U_b + 1] row by row; the five reductions of the float64 restatement are those
    of the torch recursion; a T_b == 0 row and a row whose target's logit is -inf at a cell every path crosses are +inf with a zero
    gradient."""
    T_b, U_b = [7, 4, 6], [3, 3, 1]
    x, tg, blank = R.rnnt_inputs(3, 7, 3, 7, 5)
    for red in R.REDUCTIONS:
        want = R.rnnt_ref(x, tg, T_b, U_b, blank, red, grad_scale=0.5)
        l64, g64 = R.rnnt_torch(x, tg, T_b, U_b, blank, red, dtype=torch.float64)
        assert np.abs(np.asarray(want["loss"]) - l64.numpy()).max() <= 1e-12, red
        assert np.abs(want["grad"] - 0.5 * g64.numpy()).max() <= 1e-12, red
    for b in range(3):
        assert np.all(want["grad"][b, T_b[b]:] == 0) and np.all(want["grad"][b, :, U_b[b] + 1:] == 0)
    assert np.isposinf(R.rnnt_ref(x, tg, [0, 4, 6], U_b, blank, "none")["nll"][0])
    cut = x.clone()
    cut[1, :, 1, int(tg[1, 1])] = -float("inf")                                 # label 1 of row 1 has no probability anywhere: no complete path
    w = R.rnnt_ref(cut, tg, T_b, U_b, blank, "none")
    assert np.isposinf(w["nll"][1]) and np.all(w["grad"][1] == 0) and np.isfinite(w["nll"][[0, 2]]).all() and np.isfinite(w["grad"]).all()


@pytest.mark.parametrize("layers", [1, 2])
def test_param_spec_is_transformers_state_dict(layers):
    from transformers import ParakeetForRNNT
    from dynamic_asr_eval_amd import parakeet_model as PM, parakeet_rnnt_model as RM
    cfg = R.hf_rnnt_config(layers=layers)
    sd = ParakeetForRNNT(cfg).state_dict()
    c = RM.make_config(cfg)
    hf_shape = {"pw": lambda s: s + (1,), "dw": lambda s: (s[0], 1) + s[1:], "pw2": lambda s: s + (1, 1), "sublin": lambda s: s, None: lambda s: s}
    ours = {n: hf_shape[kind](tuple(shape)) for n, shape, kind in RM.param_spec(c)}
    bufs = {n: tuple(shape) for n, shape, _ in PM.buffer_spec(c)}
    assert set(ours) | set(bufs) == set(sd) and not set(ours) & set(bufs)
    for n, shape in {**ours, **bufs}.items():
        assert tuple(sd[n].shape) == shape, (n, tuple(sd[n].shape), shape)
    assert ours["joint.head.weight"] == (R.RNNT_VOCAB, 64) and ours["joint.head.bias"] == (R.RNNT_VOCAB,)
    names = [n for n, _, _ in RM.param_spec(c)]
    assert [n for n in names if not n.startswith("encoder.")] == [n for n in sd if not n.startswith("encoder.")]      # transformers' order


def test_make_config_reads_the_object_the_nested_dict_and_the_defaults(tmp_path):
    from dynamic_asr_eval_amd import parakeet_rnnt_model as RM
    cfg = R.hf_rnnt_config(max_symbols_per_step=3)
    c = RM.make_config(cfg)
    assert RM.make_config(cfg.to_dict()) == c
    assert c["durations"] == () and c["decoder_hidden_size"] == 64 and c["num_decoder_layers"] == 2 and c["vocab_size"] == R.RNNT_VOCAB
    assert c["blank_token_id"] == R.RNNT_BLANK and c["pad_token_id"] == R.RNNT_PAD and c["joint_hidden_act"] == "relu" and c["hidden_act"] == "silu"
    assert c["max_symbols_per_step"] == 3 and c["decoder_start_token_id"] is None and c["hidden_size"] == 256
    d = RM.make_config()                                     # transformers' defaults: the released checkpoints' head
    from transformers import ParakeetRNNTConfig
    t = ParakeetRNNTConfig()
    assert (d["decoder_hidden_size"], d["num_decoder_layers"], d["vocab_size"], d["blank_token_id"], d["max_symbols_per_step"], d["durations"]) == \
        (t.decoder_hidden_size, t.num_decoder_layers, t.vocab_size, t.blank_token_id, t.max_symbols_per_step, ()) == (640, 2, 8193, 8192, 10, ())
    assert RM.make_config(t) == d
    with open(tmp_path / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    assert RM.config_from_json(str(tmp_path / "config.json")) == c
    assert RM.ParakeetForRNNT.default_reduction == "mean_volume" and RM.ParakeetForRNNT.__mro__[1].default_reduction == "mean"


@pytest.mark.parametrize("word,over", [
    ("hidden_act", dict(hidden_act="gelu")), ("ParakeetForTDT", dict(model_type="parakeet_tdt")), ("parakeet_tdt_model", dict(durations=[0, 1, 2, 3, 4])),
    ("parakeet_ctc", dict(model_type="parakeet_ctc")), ("decoder_hidden_size", dict(decoder_hidden_size=66)),
    ("num_decoder_layers", dict(num_decoder_layers=9)), ("blank_token_id", dict(blank_token_id=40)),
    ("max_symbols_per_step", dict(max_symbols_per_step=0)), ("decoder_start_token_id", dict(decoder_start_token_id=33))],
    ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(word, over):
    from dynamic_asr_eval_amd import parakeet_rnnt_model as RM
    from dynamic_asr_eval_amd.ops import DynError
    base = R.hf_rnnt_config().to_dict()
    with pytest.raises(DynError) as e:
        RM.make_config(dict(base, **over))
    assert word in str(e.value), str(e.value)


def test_tdt_config_encoder_refusals_attention_mask_and_the_waveform_harness(tmp_path):
    from dynamic_asr_eval_amd import parakeet_rnnt_model as RM, parakeet_tdt_model as TM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    with pytest.raises(DynError) as e:
        RM.make_config(TR.hf_tdt_config())                                      # the object: it carries durations
    assert "ParakeetForTDT" in str(e.value) and "parakeet_tdt_model" in str(e.value)
    with pytest.raises(DynError) as e:
        TM.make_config(R.hf_rnnt_config())
    assert "ParakeetForRNNT" in str(e.value) and "parakeet_rnnt" in str(e.value) and "parakeet_rnnt_model" in str(e.value)
    with pytest.raises(DynError) as e:                                          # what parakeet_model.make_config refuses of the encoder
        RM.make_config(R.hf_rnnt_config(arch=dict(PR.TOY, conv_kernel_size=7)))
    assert "conv_kernel_size" in str(e.value)
    with pytest.raises(DynError) as e:
        RM.ParakeetForRNNT.forward(None, torch.zeros(1, 8, 80), decoder_input_ids=torch.zeros(1, 1, dtype=torch.int64), attention_mask=torch.ones(1, 8))
    assert "attention_mask" in str(e.value)
    with pytest.raises(DynError) as e:
        RM.ParakeetForRNNT.head(None, None, None, sigma=0.05)
    assert "sigma" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(R.hf_rnnt_config().to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "parakeet_rnnt"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "parakeet_rnnt" in str(e.value) and "parakeet_rnnt_model" in str(e.value) and "dynamic_eval_transducer_loss" in str(e.value)


def test_the_loop_has_a_head_neutral_name_and_reads_no_durations():
    import inspect
    from dynamic_asr_eval_amd import parakeet_tdt_lib as N
    assert N.dynamic_eval_transducer_loss is N.dynamic_eval_tdt_loss
    assert "durations" not in inspect.getsource(N.dynamic_eval_tdt_loss)


def test_header_entries_are_exported_and_refuse_before_any_launch():
    """The RNN-T entries are in include/dyneval.h and in the library; argument errors come back as codes before any launch, so dummy
    pointers are never dereferenced: DYN_E_ARG (-1) for null pointers and bad sizes, DYN_E_WORKSPACE (-3) for a short workspace and, by
    name, for a lattice over the budget.  The state is 20 bytes per cell."""
    from dynamic_asr_eval_amd import _lib
    names = ("dyn_rnnt_loss", "dyn_rnnt_loss_workspace_bytes", "dyn_rnnt_loss_workspace_layout", "dyn_rnnt_arcs_chunk", "dyn_rnnt_lattice_run",
             "dyn_rnnt_grad_chunk", "dyn_rnnt_greedy_steps")
    assert set(names) <= set(_lib.exported_symbols())
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n
    p, big = 256, 1 << 40
    cells = 64 * 300 * 41
    need = lib.dyn_rnnt_loss_workspace_bytes(64, 300, 41)
    assert 20 * cells <= need <= 20 * cells + 8 * 64 * 341 + 12 * 64 + 8 * 256 and lib.dyn_rnnt_loss_workspace_bytes(0, 9, 6) == -1
    assert need < lib.dyn_tdt_loss_workspace_bytes(64, 300, 41, 5) * 21 // 44
    need = lib.dyn_rnnt_loss_workspace_bytes(2, 9, 6)
    args = lambda ws=p, wsb=big, budget=0, blank=8, red=3, x=p: (x, 2, 9, 6, 9, p, 5, p, p, blank, red, 1.0, p, p, p, ws, wsb, budget, None)   # noqa: E731
    assert lib.dyn_rnnt_loss(*args(blank=9)) == -1 and b"dyn_rnnt_loss" in lib.dyn_last_error()
    assert lib.dyn_rnnt_loss(*args(red=5)) == -1 and lib.dyn_rnnt_loss(*args(x=None)) == -1
    assert lib.dyn_rnnt_loss(*args(wsb=need - 1)) == -3 and lib.dyn_rnnt_loss(*args(ws=None)) == -3
    assert lib.dyn_rnnt_loss(*args(budget=need - 1)) == -3
    assert b"budget" in lib.dyn_last_error() and b"chunking" in lib.dyn_last_error()
    chunk = lambda t0, Tc, budget=0: (p, 2, 9, 6, 9, p, 5, p, 8, t0, Tc, p, big, budget, None)                                              # noqa: E731
    assert lib.dyn_rnnt_arcs_chunk(*chunk(9, 1)) == -1 and lib.dyn_rnnt_arcs_chunk(*chunk(-1, 1)) == -1 and lib.dyn_rnnt_arcs_chunk(*chunk(0, 0)) == -1
    assert lib.dyn_rnnt_arcs_chunk(*chunk(0, 3, budget=need - 1)) == -3 and b"dyn_rnnt_arcs_chunk" in lib.dyn_last_error()
    assert lib.dyn_rnnt_lattice_run(2, 9, 6, 5, p, p, 3, p, p, 1, p, need - 1, 0, None) == -3
    assert lib.dyn_rnnt_lattice_run(2, 9, 6, 5, None, p, 3, p, p, 1, p, big, 0, None) == -1
    assert lib.dyn_rnnt_grad_chunk(p, 2, 9, 6, 9, p, 5, p, p, 8, 3, 1.0, 9, 2, p, p, big, None) == -1
    assert lib.dyn_rnnt_grad_chunk(p, 2, 9, 6, 9, p, 5, p, p, 8, 3, 1.0, 0, 2, None, p, big, None) == -1
    g = lambda B=2, n_steps=1, blank=32, ms=3: (p,) * 16 + (B, 17, 64, 2, 33, blank, ms, 51, 51, n_steps, None)                            # noqa: E731
    assert lib.dyn_rnnt_greedy_steps(*g(B=0)) == -1 and lib.dyn_rnnt_greedy_steps(*g(blank=33)) == -1
    assert lib.dyn_rnnt_greedy_steps(*g(n_steps=-1)) == -1 and lib.dyn_rnnt_greedy_steps(*g(ms=0)) == -1
    assert lib.dyn_rnnt_greedy_steps(*((None,) + g()[1:])) == -1


def test_ops_refuse_on_the_host():
    from dynamic_asr_eval_amd import ops
    for fn in ("rnnt_loss", "rnnt_state", "rnnt_arcs_chunk", "rnnt_lattice_run", "rnnt_grad_chunk", "RnntGreedyState", "rnnt_greedy_steps"):
        assert hasattr(ops, fn), fn
    with pytest.raises(ops.DynError):
        ops.rnnt_loss(torch.zeros(1, 2, 3, 5), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.int32), 4)                     # host tensors: there is no CPU path
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_state(64, 3000, 400, "cpu")
    assert "budget" in str(e.value) and "chunking the lattice state is not built" in str(e.value)
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_state(2, 9, 6, "cpu", budget=100)
    assert "budget of 100" in str(e.value)


def test_decode_oracle_satisfies_the_gpu_tests_conditions():
    """transformers' greedy RNN-T decode on the inputs tests/test_parakeet_rnnt_gpu.py gives generate() (rnnt_refs.DECODE, with
    max_symbols_per_step = 3): the smallest top-2 margin over every argmax is at least 1e-2; there are blank and non-blank steps,
    neither none nor all; at least one frame emits two or more symbols and is then left by a blank, unforced; at least one frame is
    left by the forced advance, after exactly max_symbols_per_step symbols; every row reaches the end of its frames."""
    cfg, ref = R.decode_model()
    assert cfg.max_symbols_per_step == 3
    for B in (1, 3):
        rows, Tp, margin = R.decode_case(B, ref)
        R.assert_decode_conditions(rows, margin, cfg.max_symbols_per_step)
        assert Tp == 38 and all(r["finished"] and len(r["steps"]) < cfg.max_symbols_per_step * Tp - 1 for r in rows)
