"""CohereAsrForConditionalGeneration (cohere_asr_model.py) without a GPU: the parameter list against transformers' state dict, every refusal
of make_config by name, config_from_json, the float64 references of tests/cohere_asr_refs.py against transformers (cached generate and the
teacher-forced forward, both in float64), the pure host functions of the model and of cohere_asr_lib, and the conditions the GPU decode
test puts on its fixtures, re-checked here on transformers alone."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cohere_asr_refs as R  # noqa: E402
import parakeet_refs as PR  # noqa: E402

from dynamic_asr_eval_amd import cohere_asr_lib as CL  # noqa: E402
from dynamic_asr_eval_amd import cohere_asr_model as CM  # noqa: E402
from dynamic_asr_eval_amd import ops  # noqa: E402

ENC_1024 = dict(hidden_size=1024, intermediate_size=4096)               # the released encoder at a width the package builds


@pytest.mark.parametrize("dec", [R.DEC_A, R.DEC_B], ids=["A", "B"])
def test_param_spec_is_transformers_state_dict(dec):
    cfg, ref = R.hf_model(dec)
    c = CM.make_config(cfg)
    want = {n: tuple(p.shape) for n, p in ref.named_parameters()}
    got = CM.hf_param_shapes(c)
    assert set(got) == set(want)
    assert all(got[n] == want[n] for n in want), [(n, got[n], want[n]) for n in want if got[n] != want[n]][:4]
    bufs = {CM.hf_name(n) for n, _, _ in CM.PM.buffer_spec(c)}
    assert bufs == {n for n, _ in ref.named_buffers() if "inv_freq" not in n}
    names = [n for n, _, _ in CM.param_spec(c)]
    for l in range(dec["num_hidden_layers"]):            # the packed projections: adjacent slots, weights then biases
        p = f"model.decoder.layers.{l}."
        i = names.index(p + "self_attn.q_proj.weight")
        assert names[i:i + 6] == [p + f"self_attn.{n}_proj.{leaf}" for leaf in ("weight", "bias") for n in "qkv"]
        i = names.index(p + "encoder_attn.k_proj.weight")
        assert names[i:i + 4] == [p + f"encoder_attn.{n}_proj.{leaf}" for leaf in ("weight", "bias") for n in "kv"]


def _cfg(**over):
    enc = over.pop("encoder_config", dict(PR.TOY))
    return {"model_type": "cohere_asr", "encoder_config": enc, **R.DEC_A, **over}


@pytest.mark.parametrize("over,word", [
    (dict(model_type="whisper"), "model_type"), (dict(num_key_value_heads=1), "num_key_value_heads"), (dict(head_dim=64), "head_dim"),
    (dict(hidden_size=768, num_attention_heads=4), "head_dim=192"), (dict(hidden_size=512, num_attention_heads=1), "head_dim=512"),
    (dict(hidden_act="gelu"), "hidden_act"), (dict(hidden_size=320), "hidden_size"), (dict(hidden_size=4352, num_attention_heads=17), "hidden_size"),
    (dict(intermediate_size=1000), "intermediate_size"), (dict(intermediate_size=4352), "intermediate_size"),
    (dict(tie_word_embeddings=True), "tie_word_embeddings"), (dict(attention_bias=False), "attention_bias"),
    (dict(eos_token_id=40), "eos_token_id"), (dict(encoder_config=dict(PR.TOY, model_type="whisper_encoder")), "encoder_config.model_type"),
    (dict(encoder_config=dict(PR.TOY, hidden_size=64, num_attention_heads=4)), "hidden_size=64"),
    (dict(encoder_config=dict(PR.TOY, conv_kernel_size=31)), "conv_kernel_size"),
])
def test_make_config_refuses_by_name(over, word):
    with pytest.raises(ops.DynError, match=word):
        CM.make_config(_cfg(**over))


def test_released_defaults_and_config_from_json(tmp_path):
    """None reads the released defaults of configuration_cohere_asr.py; the released ENCODER width (1280) is one parakeet_model does not
    build and is refused by name.  With an encoder width that is built, config_from_json round-trips the released decoder defaults."""
    from transformers import CohereAsrConfig
    with pytest.raises(ops.DynError, match="hidden_size=1280"):
        CM.make_config(None)
    with pytest.raises(ops.DynError, match="hidden_size=1280"):
        CM.make_config(CohereAsrConfig())
    hf = CohereAsrConfig(encoder_config=dict(ENC_1024))
    path = tmp_path / "config.json"
    path.write_text(json.dumps(hf.to_dict()))
    a, b = CM.config_from_json(str(path)), CM.make_config(hf)
    assert a == b == CM.make_config(dict(encoder_config=dict(ENC_1024)))
    assert (a["dec_hidden_size"], a["dec_layers"], a["dec_heads"], a["dec_intermediate_size"], a["vocab_size"], a["dec_max_positions"]) == \
        (1024, 8, 8, 4096, 16384, 1024)
    assert (a["pad_token_id"], a["eos_token_id"], a["decoder_start_token_id"]) == (2, 3, 4)          # no decoder_start_token_id: bos
    assert a["num_mel_bins"] == 128 and a["scale_input"] is False and a["num_hidden_layers"] == 48
    path.write_text("[1]")
    with pytest.raises(ops.DynError, match="JSON object"):
        CM.config_from_json(str(path))


def test_float64_references_agree_with_transformers():
    """decoder_ref (causal: position t is the cached step at t) against transformers in float64, within 1e-10: the teacher-forced forward,
    and the logits of the cached decode along generate's own sequence.  generate casts its `scores` to float32 whatever the model's
    dtype, so the cached logits are taken from the forward generate calls, with `past_key_values`: the prompt, then one token a step."""
    cfg, ref = R.hf_model(R.DEC_A, seed=5, gain=8.0)
    ref = ref.double()
    x = R.feats().double()
    ids = torch.randint(5, 40, (3, 6), generator=R.gen(3))
    p = R.decoder_of(ref.state_dict())
    with torch.no_grad():
        enc = ref.model.encoder(x).last_hidden_state
        want = ref(input_features=x, decoder_input_ids=ids).logits
        ckv = R.cross_kv_of(p, enc, 2)
        got, rows, x0 = R.decoder_ref(p, ids, ckv, 2)
        assert (got - want).abs().max().item() < 1e-10
        prompt = torch.tensor([[R.START, 7], [R.START, 11], [R.START, 23]])
        seq = ref.generate(input_features=x, decoder_input_ids=prompt, do_sample=False, max_new_tokens=6)
        step, _, _ = R.decoder_ref(p, seq[:, :-1], ckv, 2)
        eo = ref.model.encoder(x)
        o = ref(encoder_outputs=eo, decoder_input_ids=seq[:, :2], use_cache=True)
        assert (step[:, 1] - o.logits[:, -1]).abs().max().item() < 1e-10
        for t in range(2, seq.shape[1] - 1):
            o = ref(encoder_outputs=eo, decoder_input_ids=seq[:, t:t + 1], past_key_values=o.past_key_values, use_cache=True)
            assert (step[:, t] - o.logits[:, -1]).abs().max().item() < 1e-10
            assert torch.equal(o.logits[:, -1].argmax(-1), seq[:, t + 1])


def test_host_functions():
    lab = torch.tensor([[7, 8, 9, -100], [5, -100, -100, -100]])
    from transformers.models.cohere_asr.modeling_cohere_asr import shift_tokens_right
    assert torch.equal(CM.shift_tokens_right(lab, 2, 4), shift_tokens_right(lab, 2, 4))
    assert CM.host_prompt(None, 3, 4, 40).tolist() == [[4]] * 3
    assert CM.host_prompt([[4, 9]], 2, 4, 40).tolist() == [[4, 9]] * 2
    for bad in ([[4, 40]], [[-1]], [4, 5], torch.zeros(1, 0, dtype=torch.int64), torch.zeros(1, 2), [[1], [2], [3]]):
        with pytest.raises(ops.DynError):
            CM.host_prompt(bad, 2, 4, 40)
    buf = torch.tensor([[4, 9, 3, 7, 7, 7], [4, 3, 3, 5, 5, 5], [4, 8, 8, 8, 8, 3]])
    assert CM.finish_sequences(buf, 1, 3, 2).tolist() == [[4, 9, 3, 2, 2, 2], [4, 3, 2, 2, 2, 2], [4, 8, 8, 8, 8, 3]]
    assert CM.finish_sequences(buf[:2], 1, 3, 2).tolist() == [[4, 9, 3], [4, 3, 2]]                    # cut at the longest row
    assert CM.finish_sequences(buf[:, :2], 2, 3, 2).tolist() == [[4, 9], [4, 3], [4, 8]]               # an eos inside the prompt is not one
    assert CM.hf_name("encoder.layers.0.norm_out.weight") == "model.encoder.layers.0.norm_out.weight"
    assert CM.own_name("model.encoder.subsampling.linear.bias") == "encoder.subsampling.linear.bias"
    assert CM.hf_name("proj_out.bias") == CM.own_name("proj_out.bias") == "proj_out.bias"
    assert CL.pseudo_label([4, 9, 7, 8, 3, 2, 2], 2, 3, 2) == [7, 8]
    assert CL.label_row([4, 9], [7, 8], 3) == ([4, 9, 7, 8], [-100, 7, 8, 3])
    assert CL.spread_frames(3, 9, 10) == [11, 14, 17] and CL.spread_frames(0, 9) == []


def test_run_wav2vec2_refuses_cohere_asr_by_name(tmp_path):
    import argparse
    from dynamic_asr_eval_amd import run_wav2vec2
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="cohere_asr")))
    with pytest.raises(ops.DynError, match="cohere_asr_lib.dynamic_eval_seq2seq_loss"):
        run_wav2vec2.load_pretrained_model(argparse.Namespace(config="", checkpoint=str(tmp_path)), "cpu")


@pytest.mark.parametrize("seed,prompt", R.DECODE_CASES)
def test_decode_fixtures_are_not_near_ties(seed, prompt):
    """The conditions tests/test_cohere_asr_gpu.py puts on its decode fixtures, on transformers alone: the smallest top-2 gap of every
    decision is far above fp32 noise (1e-2, the rule of the sibling decode tests), and with the 2-token prompts the rows end at
    different steps, so the pad fill is exercised (seed 6: one row never ends)."""
    cfg, ref = R.hf_model(R.DEC_A, seed=seed, gain=8.0)
    prompt = torch.tensor(prompt)
    seq, gap = R.hf_generate(ref, R.feats(), prompt)
    print(seq.tolist(), gap)
    assert gap > 1e-2
    if prompt.shape[1] == 2:
        ends = [(row[2:] == R.EOS).nonzero() for row in seq]
        assert len({int(e[0]) if e.numel() else -1 for e in ends}) > 1
