"""CPU side of the LM beam search: the CPU restatement of the LM reproduces the fixture's logits, the factory's defaults and
argument checks, and a foreign beam_search_fn is still refused."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_cpu_lm_reproduces_fixture_logits():
    from lm_cpu import CpuLM
    from dynamic_asr_eval_amd.lm import synthetic_state
    meta = json.load(open(os.path.join(GOLD, "beam_pins.json")))
    arr = np.load(os.path.join(GOLD, "beam_pins.npz"))
    m = CpuLM(meta["lm_config"], meta["vocab"], synthetic_state(meta["lm_config"], meta["vocab"], meta["lm_seed"]))
    lp, _, st = m(torch.tensor([[meta["bos_id"]]]), torch.LongTensor([1]))
    np.testing.assert_allclose(lp.log_softmax(-1)[0, 0].numpy(), arr["lm_init"], atol=2e-6, rtol=0)
    assert st["cache_lengths"].tolist() == [1]


def test_factory_defaults_match_reference():
    from dynamic_asr_eval_amd import lib
    sig = inspect.signature(lib.load_beamsearch).parameters
    assert sig["path"].default is None
    assert (sig["alpha"].default, sig["beta"].default, sig["prune_less_than_val"].default, sig["top_am_threshold"].default) == \
        (0.45, 1.53, 3.17, -6)
    from dynamic_asr_eval_amd.lm import DEFAULT_LM_CONFIG, MAX_CACHE_LENGTH, lm_spec
    assert MAX_CACHE_LENGTH == 128 and DEFAULT_LM_CONFIG["max_positions"] >= MAX_CACHE_LENGTH + 1
    n = sum(int(np.prod(s)) for _, s in lm_spec(DEFAULT_LM_CONFIG, 128))
    assert 40e6 < n < 50e6        # 6 x 768 layers, ~170 MB of fp32 weights per LM step


def test_factory_argument_validation():
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(128)
    with pytest.raises(ValueError):
        lib.load_beamsearch(None, prune_less_than_val=-1.0, tokenizer=tok, device="cpu")
    with pytest.raises(ValueError):
        lib.load_beamsearch(None, top_am_threshold=1.0, tokenizer=tok, device="cpu")
    with pytest.raises(TypeError):
        lib.load_beamsearch(None, alpha="0.4", tokenizer=tok, device="cpu")


def test_checkpoint_loader_strips_ddp_and_reports_keys(tmp_path):
    from dynamic_asr_eval_amd.lm import load_checkpoint, synthetic_state
    cfg = dict(n_layers=1, d_model=256, n_heads=2, ff_mult=2, max_positions=129, norm_eps=1e-5)
    st = {"module." + k: torch.from_numpy(v) for k, v in synthetic_state(cfg, 128, 1).items()}
    path = str(tmp_path / "lm.pt")
    torch.save({"model": st, "config": cfg}, path)
    c, w = load_checkpoint(path)
    assert c["n_layers"] == 1 and np.array_equal(w["head.bias"], st["module.head.bias"].numpy())
    del st["module.head.bias"]
    torch.save({"model": st, "config": cfg}, path)
    with pytest.raises(KeyError):
        load_checkpoint(path)
    assert not load_checkpoint(path, allow_missing=True)[1]["head.bias"].any()


def test_foreign_beam_search_fn_refused():
    import argparse
    from dynamic_asr_eval_amd import lib
    args = argparse.Namespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 16384, 'overlap': 0},
                                      'training': {}}, lm_tta_beams=3)
    gen = lib._dynamic_eval_gen(args, None, torch.zeros(1, 80, 10), 512, 256, None, beam_search_fn=object())
    with pytest.raises(NotImplementedError):
        next(gen)
