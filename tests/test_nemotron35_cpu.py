"""What of Nemotron3_5AsrForRNNT (nemotron3_5_asr_model.py, csrc/prompt_fuse.hip) can be checked without a GPU: the configuration and its
refusals, the parameter names against transformers' state dict, the split of linear_1.weight, the C-ABI surface, the identity the kernels
rest on (on transformers' own modules, in float64), the host-side checks of `prompt_ids`, and the committed cases' figures on the oracle."""
import argparse
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import nemotron35_refs as PR  # noqa: E402
import nemotron_refs as NR  # noqa: E402
import rnnt_refs as R  # noqa: E402

ENTRIES = ("dyn_prompt_bias_gather", "dyn_prompt_relu_fwd", "dyn_prompt_relu_bwd_row_tile", "dyn_prompt_relu_bwd_workspace_bytes",
           "dyn_prompt_relu_bwd")


def test_make_config_round_trips_the_default_and_the_toy_configuration(tmp_path):
    from transformers import Nemotron3_5AsrConfig
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M, nemotron_asr_streaming_model as NM
    want = Nemotron3_5AsrConfig()
    for c in (M.make_config(), M.make_config(want), M.make_config(want.to_dict())):
        for k in ("vocab_size", "decoder_hidden_size", "num_decoder_layers", "max_symbols_per_step", "blank_token_id", "pad_token_id",
                  "num_prompts", "prompt_intermediate_size", "default_prompt_id"):
            assert c[k] == getattr(want, k), k
        for k in NM.ENCODER_KEYS:
            if k not in ("num_key_value_heads", "head_dim"):
                assert c[k] == getattr(want.encoder_config, k), k
        assert (c["num_prompts"], c["prompt_intermediate_size"], c["default_prompt_id"], c["vocab_size"]) == (128, 2048, 101, 13088)
        assert c["durations"] == () and c["joint_hidden_act"] == "relu"
    toy = PR.hf_config()
    assert toy.model_type == "nemotron3_5_asr" and toy.encoder_config.model_type == "nemotron_asr_streaming_encoder"
    p = tmp_path / "config.json"
    p.write_text(toy.to_json_string(use_diff=False))
    c = M.config_from_json(str(p))
    assert c == M.make_config(toy)
    assert (c["num_prompts"], c["prompt_intermediate_size"], c["default_prompt_id"], c["sliding_window"]) == (8, 96, 5, 9)


@pytest.mark.parametrize("word,over,enc", [
    ("parakeet_rnnt", dict(model_type="parakeet_rnnt"), {}), ("parakeet_tdt", dict(model_type="parakeet_tdt"), {}),
    ("parakeet_ctc", dict(model_type="parakeet_ctc"), {}), ("Parakeet", dict(durations=[0, 1, 2]), {}),
    ("nemotron_asr_streaming_model", dict(model_type="nemotron_asr_streaming"), {}), ("wav2vec2", dict(model_type="wav2vec2"), {}),
    ("nemotron_asr_streaming_encoder", {}, dict(model_type="parakeet_encoder")),
    ("num_prompts", dict(num_prompts=0), {}), ("num_prompts", dict(num_prompts=2.5), {}),
    ("prompt_intermediate_size", dict(prompt_intermediate_size=0), {}), ("prompt_intermediate_size", dict(prompt_intermediate_size=98), {}),
    ("prompt_intermediate_size", dict(prompt_intermediate_size=-4), {}),
    ("default_prompt_id", dict(default_prompt_id=8), {}), ("default_prompt_id", dict(default_prompt_id=-1), {}),
    ("default_prompt_id", dict(default_prompt_id=True), {}),
    ("sliding_window", {}, dict(sliding_window=0)), ("of the joint", dict(hidden_act="tanh"), {}), ("hidden_size", {}, dict(hidden_size=384))],
    ids=lambda v: v if isinstance(v, str) else "")
def test_what_is_not_built_is_refused_by_name(word, over, enc):
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M
    from dynamic_asr_eval_amd.ops import DynError
    base = PR.hf_config().to_dict()
    base["encoder_config"] = dict(base["encoder_config"], **enc)
    with pytest.raises(DynError) as e:
        M.make_config(dict(base, **over))
    assert word in str(e.value), str(e.value)


def test_the_sibling_and_the_waveform_harness_point_here(tmp_path):
    from dynamic_asr_eval_amd import nemotron_asr_streaming_model as NM, parakeet_rnnt_model as RM, run_wav2vec2 as RW
    from dynamic_asr_eval_amd.ops import DynError
    toy = PR.hf_config()
    for make in (NM.make_config, RM.make_config):
        with pytest.raises(DynError) as e:
            make(toy.to_dict())
        assert "nemotron3_5_asr" in str(e.value)
    with pytest.raises(DynError) as e:
        NM.make_config(toy)
    assert "nemotron3_5_asr_model" in str(e.value) and "Nemotron3_5AsrForRNNT" in str(e.value)
    d = tmp_path / "model"
    d.mkdir()
    (d / "config.json").write_text(toy.to_json_string(use_diff=False))
    assert RW.model_type(str(d / "config.json")) == "nemotron3_5_asr"
    with pytest.raises(DynError) as e:
        RW.load_pretrained_model(argparse.Namespace(checkpoint=str(d), config=""), "cuda:0")
    assert "nemotron3_5_asr_model" in str(e.value) and "dynamic_eval_transducer_loss" in str(e.value)


def test_param_spec_equals_transformers_state_dict_and_linear_1_splits_and_merges():
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M
    for arch in (NR.TOY, dict(NR.TOY, convolution_bias=False, attention_bias=False, num_mel_bins=41)):
        cfg, ref = PR.hf_model(seed=0, arch=arch)
        sd = ref.state_dict()
        c = M.make_config(cfg)
        spec = M.param_spec(c)
        assert {n for n, _, _ in spec} == set(sd) and len(spec) == len(sd)
        for n, shape, kind in spec:
            hf = tuple(sd[n].shape)
            want = {"dw": shape[:1] + (1,) + shape[1:], "pw": shape + (1,), "pw2": shape + (1, 1)}.get(kind, shape)
            assert hf == want, (n, hf, shape, kind)
        flat = M.flat_spec(c)
        assert len(flat) == len(spec) + 1 and M.W1 not in {n for n, _, _ in flat}
        shapes = {n: s for n, s, _ in flat}
        assert shapes[M.W1H] == (96, 256) and shapes[M.W1P] == (96, 8)
        assert all(n.startswith(M.W1) and n.startswith(M.PROMPT) for n in (M.W1H, M.W1P))       # a frozen prefix by transformers' name holds both
        w = sd[M.W1]
        hidden, prompt = M.split_w1(w, 256)
        assert hidden.is_contiguous() and prompt.is_contiguous() and hidden.shape == (96, 256) and prompt.shape == (96, 8)
        assert torch.equal(hidden, w[:, :256]) and torch.equal(prompt, w[:, 256:]) and torch.equal(M.merge_w1(hidden, prompt), w)


def test_the_identity_holds_on_transformers_modules_in_float64():
    """linear_1(cat([h, onehot(p_b)])) = h W1[:, :H]^T + (b1 + W1[:, H + p_b]) on transformers' prompt projector in float64, forward (the
    pre-activation, the fused states) and backward (db1 = sum_b s[b], dW1[:, H + p] = the segment sum over the rows with p_b = p, exact
    zeros at unused prompts), with the refs the GPU tests use."""
    cfg, ref = PR.hf_model(**PR.MODEL)
    pp = copy_double(ref.prompt_projector)
    H, Np = cfg.encoder_config.hidden_size, cfg.num_prompts
    g = torch.Generator().manual_seed(0)
    h = torch.randn(3, 7, H, generator=g, dtype=torch.float64)
    ids = PR.PROMPTS_A
    w1, b1 = pp.linear_1.weight, pp.linear_1.bias
    want_z = PR.concat_form(h, w1, b1, ids, Np)
    pb = PR.gather(b1, w1[:, H:], ids)
    z = h @ w1[:, :H].t()
    assert (z + pb[:, None, :] - want_z).abs().max().item() < 1e-13
    one_hot = torch.nn.functional.one_hot(torch.tensor(ids), Np).double()[:, None, :].expand(-1, 7, -1)
    fused = pp(torch.cat([h, one_hot], -1))
    a = PR.fused_fwd(z, pb)
    assert (pp.linear_2(a) - fused).abs().max().item() < 1e-13
    dout = torch.randn(fused.shape, generator=g, dtype=torch.float64)
    pp.zero_grad()
    (fused * dout).sum().backward()
    da = dout @ pp.linear_2.weight.detach()
    dz, s, db1, dw = PR.fused_bwd(a.detach(), da, ids, Np)
    assert (db1 - pp.linear_1.bias.grad).abs().max().item() < 1e-12
    assert (dw - pp.linear_1.weight.grad[:, H:]).abs().max().item() < 1e-12
    assert (dz.reshape(-1, dz.shape[-1]).t() @ h.reshape(-1, H) - pp.linear_1.weight.grad[:, :H]).abs().max().item() < 1e-11
    unused = [p for p in range(Np) if p not in ids]
    assert bool((pp.linear_1.weight.grad[:, H:][:, unused] == 0).all()) and bool((dw[:, unused] == 0).all())
    assert torch.equal(dw[:, 1], s[0] + s[2]) and torch.equal(dw[:, 5], s[1])


def copy_double(module):
    import copy
    return copy.deepcopy(module).double()


def test_header_entries_are_exported_and_refuse_before_any_launch():
    """The prompt-fusion entries are in include/dyneval.h and in the library; argument errors come back as DYN_E_ARG (-1) or
    DYN_E_WORKSPACE (-3) before any launch, so dummy pointers are never dereferenced."""
    from dynamic_asr_eval_amd import _lib
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    lib = _lib.load()
    for n in ENTRIES:
        assert hasattr(lib, n), n
    p = 256
    assert lib.dyn_prompt_bias_gather(None, p, p, p, 3, 96, 8, None) == -1
    assert lib.dyn_prompt_bias_gather(p, p, None, p, 3, 96, 8, None) == -1
    assert lib.dyn_prompt_bias_gather(p, p, p, p, 0, 96, 8, None) == -1
    assert lib.dyn_prompt_bias_gather(p, p, p, p, 3, 98, 8, None) == -1 and b"multiple of 4" in lib.dyn_last_error()
    assert lib.dyn_prompt_bias_gather(p, p, p, p, 3, 96, 0, None) == -1
    assert lib.dyn_prompt_bias_gather(p, p + 4, p, p, 3, 96, 8, None) == -1 and b"aligned" in lib.dyn_last_error()
    assert lib.dyn_prompt_bias_gather(p, p, p + 2, p, 3, 96, 8, None) == -1
    assert lib.dyn_prompt_relu_fwd(None, p, p, 3, 5, 96, None) == -1
    assert lib.dyn_prompt_relu_fwd(p, p, p + 8, 3, 5, 96, None) == -1
    assert lib.dyn_prompt_relu_fwd(p, p, p, 3, 0, 96, None) == -1
    assert lib.dyn_prompt_relu_fwd(p, p, p, 3, 5, 2, None) == -1
    assert lib.dyn_prompt_relu_fwd(p, p, p, 70000, 5, 96, None) == -1
    assert lib.dyn_prompt_relu_fwd(512, p, p, 3, 5, 96, None) == -1 and b"alias" in lib.dyn_last_error()
    assert [lib.dyn_prompt_relu_bwd_row_tile(T) for T in (0, 1, 8, 9, 512, 513, 1024)] == [-1, 1, 8, 5, 8, 9, 16]
    assert lib.dyn_prompt_relu_bwd_workspace_bytes(3, 9, 96) == (2 + 1) * 3 * 96 * 4
    assert lib.dyn_prompt_relu_bwd_workspace_bytes(4, 256, 2048) == (32 + 1) * 4 * 2048 * 4
    assert lib.dyn_prompt_relu_bwd_workspace_bytes(0, 9, 96) == 0
    bwd = lambda *a: lib.dyn_prompt_relu_bwd(*a, None)                                                       # noqa: E731
    q = 512
    assert bwd(None, p, p, p, p, p, 1.0, 3, 5, 96, 8, q, 1 << 20) == -1
    assert bwd(q, p, q, p, p, p, 1.0, 3, 5, 96, 8, q, 1 << 20) == -1 and b"alias" in lib.dyn_last_error()
    assert bwd(q, p, p, None, p, p, 1.0, 3, 5, 96, 8, q, 1 << 20) == -1 and b"ids" in lib.dyn_last_error()
    assert bwd(q, p, p, p, p, p, 1.0, 3, 5, 96, 8, None, 1 << 20) == -1
    assert bwd(q, p, p, p, p, p, 1.0, 3, 5, 96, 0, q, 1 << 20) == -1
    assert bwd(q, p, p, p, p, p + 4, 1.0, 3, 5, 96, 8, q, 1 << 20) == -1
    assert bwd(q, p, p, p, p, p, 1.0, 3, 5, 94, 8, q, 1 << 20) == -1
    assert bwd(q, p, p, p, p, p, 1.0, 3, 5, 96, 8, q, 2 * 3 * 96 * 4 - 1) == -3 and b"workspace" in lib.dyn_last_error()


def test_prompt_ids_are_checked_on_the_host():
    """ops.host_prompt_ids: None is the default for every row, an int is broadcast, a tensor or list must be integer, [B] and inside the
    table; the model's setter of default_prompt_id refuses a value outside it.  No device is touched."""
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M, ops
    f = lambda p, B=3: ops.host_prompt_ids(p, B, 8, 5)                                                       # noqa: E731
    assert f(None) == [5, 5, 5] and f(1) == [1, 1, 1] and f([1, 5, 1]) == [1, 5, 1] and f(torch.tensor([6, 5, 3], dtype=torch.int32)) == [6, 5, 3]
    assert f(torch.tensor([7]), 1) == [7] and f((0, 7), 2) == [0, 7]
    for bad in ([1, 5], [1, 5, 1, 1], 8, -1, [1, 8, 1], [0, -1, 0], True, 1.0, [1.0, 2.0, 3.0], [[1, 5, 1]], torch.tensor(3)):
        with pytest.raises(ops.DynError) as e:
            f(bad)
        assert "prompt_ids" in str(e.value), (bad, str(e.value))
    fake = argparse.Namespace(Np=8, _default_prompt_id=5, _ctx_prompts=[1, 5, 1])
    fake._host_prompts = lambda p, B: M.Nemotron3_5AsrForRNNT._host_prompts(fake, p, B)
    same = lambda who, p: M.Nemotron3_5AsrForRNNT._same_prompts(fake, who, p)                                # noqa: E731
    same("head", None), same("head", [1, 5, 1]), same("backward", torch.tensor([1, 5, 1]))
    for who, bad in (("head", [6, 5, 3]), ("backward", 1), ("backward", [1, 5])):
        with pytest.raises(ops.DynError) as e:
            same(who, bad)
        assert "prompt_ids" in str(e.value)
    prop = M.Nemotron3_5AsrForRNNT.default_prompt_id
    prop.fset(fake, 3)
    assert prop.fget(fake) == 3 and fake._host_prompts(None, 2) == [3, 3]
    for bad in (8, -1, True, 1.5, None):
        with pytest.raises(ops.DynError) as e:
            prop.fset(fake, bad)
        assert "default_prompt_id" in str(e.value)
    assert prop.fget(fake) == 3


def test_committed_cases_hold_on_the_oracle():
    """The figures the GPU tests lean on, on transformers alone: the ReLU masks of the forward / backward case are at least 1e-4 from a
    flip (6.0e-4), the two prompt sets move rows 0 and 2 of the projected states (1.8e-2 and 3.3e-2 at max |enc| 0.30) and leave row 1
    alone, and the decode case satisfies rnnt_refs.assert_decode_conditions under both prompt sets through transformers' own generate
    (margins 1.9e-2 and 1.6e-2, token counts [72, 2, 39] under A), rows 0 and 2 differing between the sets and row 1 equal."""
    cfg, ref = PR.hf_model(**PR.MODEL)
    x = torch.randn(3, 131, 80, generator=torch.Generator().manual_seed(1))
    for look in (2, 0):
        assert PR.min_pre_relu(ref, x, PR.PROMPTS_A, look) > PR.MIN_PRE_RELU
    eA, eB = PR.hf_encode(ref, x, PR.PROMPTS_A, 2), PR.hf_encode(ref, x, PR.PROMPTS_B, 2)
    gap = (eA - eB).abs().amax((1, 2)).tolist()
    assert gap[0] > 1e-2 and gap[1] == 0.0 and gap[2] > 1e-2 and 0.2 < eA.abs().max().item() < 0.4, gap
    assert torch.equal(PR.hf_encode(ref, x, None, 2), PR.hf_encode(ref, x, [5, 5, 5], 2))
    cfg, ref = PR.decode_model()
    rows_a, Tp, margin_a = PR.decode_case(3, PR.PROMPTS_A, ref)
    rows_b, _, margin_b = PR.decode_case(3, PR.PROMPTS_B, ref)
    assert Tp == 39 and margin_a > 1.8e-2 and margin_b > 1.5e-2, (margin_a, margin_b)
    assert [len(r["tokens"]) for r in rows_a] == [72, 2, 39]
    for rows, margin in ((rows_a, margin_a), (rows_b, margin_b)):
        R.assert_decode_conditions(rows, margin, cfg.max_symbols_per_step)
    assert [rows_a[b]["tokens"] == rows_b[b]["tokens"] for b in range(3)] == [False, True, False]
