"""CTC + transformer-LM beam search on the GPU (csrc/beam_search.hip) against tests/golden/beam_pins.*: the reference's own
BeamSearch (lcasr/ctc_beam_search.py) executed unchanged over the CPU restatement of the LM (tests/lm_cpu.py)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pins():
    meta = json.load(open(os.path.join(GOLD, "beam_pins.json")))
    return meta, dict(np.load(os.path.join(GOLD, "beam_pins.npz")))


@pytest.fixture(scope="module")
def setup(cuda, pins):
    import sentencepiece as spm
    from dynamic_asr_eval_amd.lm import TransformerLM, synthetic_state
    meta, _ = pins
    tok = spm.SentencePieceProcessor(model_file=os.path.join(GOLD, "tokenizer_128.model"))
    lm = TransformerLM(meta["lm_config"], meta["vocab"], synthetic_state(meta["lm_config"], meta["vocab"], meta["lm_seed"]), cuda)
    return tok, lm


def _factory(tok, lm, bos, case):
    from dynamic_asr_eval_amd.lib import BeamSearchFactory
    return BeamSearchFactory(lm, tok, bos, blank_id=tok.vocab_size(), alpha=case["alpha"], beta=case["beta"],
                             prune_less_than_val=case["prune"], top_am_threshold=-6)


def test_lm_step_matches_cpu_logits(setup, pins, cuda):
    from dynamic_asr_eval_amd import _lib
    from dynamic_asr_eval_amd.decoding import beam_layout
    tok, lm = setup
    meta, arr = pins
    lib = _lib.load()
    L, D, H, F, V, maxpos, eps = lm.dims()
    W, T = 4, 1
    off = beam_layout(lib, W, T, L, D, F, V)
    ws = torch.zeros(off["total"], dtype=torch.uint8, device=cuda)
    assert off["pool_slots"] >= 150
    import ctypes

    def i32(name, n):
        return ws[off[name]:off[name] + 4 * n].view(torch.int32)

    def step(rows):     # rows: (token, history slots, output slot)
        i32("hdr", 16)[4] = len(rows)
        hist = torch.zeros(W, 128, dtype=torch.int32)
        for r, (t, h, s) in enumerate(rows):
            i32("r_tok", W)[r] = t
            i32("r_pos", W)[r] = len(h)
            i32("r_hlen", W)[r] = len(h)
            i32("r_slot", W)[r] = s
            hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
        i32("r_hist", W * 128).copy_(hist.view(-1).to(cuda))
        _lib.check(lib.dyn_beam_lm_rows(ctypes.cast(lm.ptrs, ctypes.c_void_p), L, D, H, F, V, maxpos, eps, W, T, ws.data_ptr(),
                                        ws.numel(), torch.cuda.current_stream().cuda_stream), "dyn_beam_lm_rows")

    def lp(slot):
        return ws[off["pool_lp"] + 4 * V * slot:off["pool_lp"] + 4 * V * (slot + 1)].view(torch.float32).cpu().numpy()

    bos = meta["bos_id"]
    step([(bos, [], 0)])
    np.testing.assert_allclose(lp(0), arr["lm_init"], atol=2e-5, rtol=0)
    seq = arr["lm_seq"].tolist()
    for n, t in enumerate(seq, start=1):        # slot n = token n; its cache = the last <= 128 slots before it
        step([(t, list(range(max(0, n - 128), n)), n)])
    rows = [(int(t), list(range(max(0, n + 1 - 128), n + 1)), 141 + r) for r, (n, t) in enumerate(arr["lm_rows"].tolist())]
    step(rows)
    got = np.stack([lp(141 + r) for r in range(len(rows))])
    np.testing.assert_allclose(got, arr["lm_batch"], atol=2e-5, rtol=0)


def _run(setup, pins, case, feed):
    tok, lm = setup
    bs = _factory(tok, lm, pins[0]["bos_id"], case)(log_probs=feed, beam_width=case["width"])
    bs.run_search(use_tqdm=False)
    return bs


def _ulp_equal(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, np.float32(np.inf)) == b or np.nextafter(a, np.float32(-np.inf)) == b


@pytest.mark.parametrize("kind", ["a0", "lm"])
def test_search_matches_reference(setup, pins, cuda, kind):
    meta, arr = pins
    cases = [c for c in meta["cases"] if (c["alpha"] == 0.0) == (kind == "a0")]
    assert cases
    for c in cases:
        bs = _run(setup, pins, c, torch.from_numpy(arr["lp_" + c["name"]]).to(cuda))
        assert len(bs.beams) == len(c["beams"]), c["name"]
        for k, (b, ref) in enumerate(zip(bs.beams, c["beams"])):
            assert b.lm_sequence == ref["lm_sequence"], (c["name"], k)
            assert [(-1 if x is None else x) for x in b.am_sequence] == ref["am_sequence"], (c["name"], k)
            if kind == "a0":
                assert _ulp_equal(b.score, ref["score"]), (c["name"], k, b.score, ref["score"])
            else:
                assert abs(b.score - ref["score"]) <= 1e-4 + 1e-6 * abs(ref["score"]), (c["name"], k, b.score, ref["score"])
        assert bs.return_text(0) == c["text"]
    assert max(c["max_emitted"] for c in cases) > 128        # the cache trim is exercised


def test_input_kinds_identical(setup, pins, cuda):
    meta, arr = pins
    c = next(c for c in meta["cases"] if c["name"] == "w20_lm_prune")
    x = arr["lp_" + c["name"]]
    outs = [_run(setup, pins, c, f) for f in (torch.from_numpy(x).to(cuda), torch.from_numpy(x), x)]
    for o in outs[1:]:
        assert [(b.score, b.lm_sequence, b.am_sequence) for b in o.beams] == \
            [(b.score, b.lm_sequence, b.am_sequence) for b in outs[0].beams]


def test_tta_width1_equals_greedy(cuda):
    """dynamic_eval with a width-1, alpha = beta = 0 factory on posteriors where token 0 never wins: the beam search's text equals
    the greedy one, so logits and adapted parameters are bit-identical to the plain greedy run."""
    import argparse
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.model import SCConformerXL
    from dynamic_asr_eval_amd.synthetic_weights import init_synthetic
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    cfg = dict(n_layers=2, d_model=256, n_heads=2, head_dim=128, subsampling_conv_channels=64)
    m = SCConformerXL(cfg, vocab_size=128, device=cuda)
    init_synthetic(m, seed=3, blank_bias=1.5)
    with torch.no_grad():       # token 0 never wins: its CTC-head bias far below the rest
        m.P["decoder.ff.bias"][0] -= 40.0
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 1400, generator=torch.Generator().manual_seed(5))

    def args(**kw):
        return argparse.Namespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 16384, 'overlap': 0},
                                          'training': {}}, optim_lr=1e-4, epochs=1, shuffle=False, quiet=True, **kw)
    fac = lib.load_beamsearch(None, alpha=0.0, beta=0.0, prune_less_than_val=None, tokenizer=tok, device=cuda,
                              lm_config=dict(n_layers=1, d_model=256, n_heads=2, ff_mult=2, max_positions=129, norm_eps=1e-5))
    ref, pref = lib.dynamic_eval(args(), m, spec, 512, 256, tok, use_tqdm=False, return_params=True)
    out, pout = lib.dynamic_eval(args(lm_tta_beams=1), m, spec, 512, 256, tok, use_tqdm=False, beam_search_fn=fac, return_params=True)
    assert np.array_equal(ref, out)
    for a, b in zip(pref, pout):
        assert torch.equal(a, b)


def test_harness_beamsearch(cuda, tmp_path, capsys):
    from dynamic_asr_eval_amd import lib, run_dynamic_eval_full as H
    common = ["-d", "synthetic_small", "-seq", "512", "-o", "256", "-ds", "-nv", "-epochs", "1", "-kwargs", "optim_lr=1e-5",
              "vocab_size=128", "quiet=True", "blank_bias=0.0"]
    greedy = str(tmp_path / "greedy.pkl")
    H.main(lib.apply_args(H.build_parser(), ["-s", greedy] + common))
    beam = str(tmp_path / "beam.pkl")
    H.main(lib.apply_args(H.build_parser(), ["-beamsearch", "-s", beam] + common + ["lm_tta_beams=0", "lm_eval_beams=4", "lm_beta=20.0"]))
    g = pickle.load(open(greedy.replace(".pkl", "_1.pkl"), "rb"))
    b = pickle.load(open(beam.replace(".pkl", "_1.pkl"), "rb"))
    assert b["model_output"] != g["model_output"]
    # the hypotheses are the factory's output on the eval function's logits
    args = lib.apply_args(H.build_parser(), common + ["lm_tta_beams=0"])
    model, tokenizer = H.load_model_and_tokenizer(args, cuda)
    fac = lib.load_beamsearch(None, beta=20.0, tokenizer=tokenizer, device=cuda)
    from dynamic_asr_eval_amd.datasets import datasets_functions
    data = datasets_functions["synthetic_small"]("test")
    by_gold = {gold: hyp for gold, hyp in zip(b["gold"], b["model_output"])}     # the pickle's order is the shard order
    for rec in data:
        spec, gold = rec["process_fn"](rec)
        hyp = by_gold[gold]
        logits = lib.dynamic_eval(args, model, spec, args.seq_len, args.overlap, tokenizer, use_tqdm=False, return_device=True)
        bs = fac(log_probs=logits, beam_width=4)
        bs.run_search(use_tqdm=False)
        assert H.normalize(bs.return_text(0)).lower() == hyp
