"""dyn_edit_counts (csrc/editdist.hip) against `wer._align` on the same ids, integer for integer: (ins, del, sub, n_ref) of every
pair, in both regimes (one workgroup per pair with the lattice's diagonals in LDS; tile x tile blocks with boundary rows / columns in
the workspace), and the callers that take `device=` - calc_rewards, score_texts, the character scoring and the grpo loop."""
import argparse
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def _rand(rng, n, alphabet=5):
    return rng.integers(0, alphabet, n).tolist()


def _check(cuda, hyps, refs, tile=0):
    """One device call for all pairs; every row equals `_align` on the same ids."""
    from dynamic_asr_eval_amd.wer import _align, edit_counts_ids
    got = edit_counts_ids(hyps, refs, cuda, tile=tile)
    assert got.shape == (len(hyps), 4) and got.dtype == np.int32
    for p, (h, r) in enumerate(zip(hyps, refs)):
        assert tuple(int(x) for x in got[p]) == _align(h, r) + (len(r),), (p, len(h), len(r), tile)
    return got


def _ws_bytes(hyps, refs, tile=0):
    from dynamic_asr_eval_amd import _lib
    ho = np.concatenate([[0], np.cumsum([len(h) for h in hyps])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    return int(_lib.load().dyn_edit_counts_workspace_bytes(ho.ctypes.data, ro.ctypes.data, len(hyps), tile))


def test_all_short_sequences_against_each_other_in_one_call(cuda):
    """All 120 sequences of length 1..4 over 3 symbols against each other: 14 400 pairs in ONE call - the ragged batch, the tie rule."""
    seqs = [list(s) for n in range(1, 5) for s in itertools.product(range(3), repeat=n)]
    assert len(seqs) == 120
    _check(cuda, [h for h in seqs for _ in seqs], [r for _ in seqs for r in seqs])


def test_seeded_ragged_batch_with_empty_and_single_token_sides(cuda):
    rng = np.random.default_rng(7)
    lens = [(0, 0), (0, 9), (9, 0), (1, 1), (1, 40), (40, 1), (0, 1), (1, 0)] + [tuple(rng.integers(0, 71, 2)) for _ in range(192)]
    hyps, refs = [_rand(rng, m, 4) for m, _ in lens], [_rand(rng, n, 4) for _, n in lens]
    got = _check(cuda, hyps, refs)
    assert tuple(got[1]) == (0, 9, 0, 9) and tuple(got[2]) == (9, 0, 0, 0) and tuple(got[0]) == (0, 0, 0, 0)


@pytest.mark.parametrize("shapes", [[(m, n) for m in (63, 64, 65) for n in (1, 64, 65)], [(1023, 1000), (1024, 1000), (1025, 1000)],
                                    [(1000, 1023), (1000, 1024), (1000, 1025)], [(1, 300), (300, 1)]],
                         ids=["wave", "workgroup-hyp", "workgroup-ref", "thin"])
def test_lengths_straddling_wave_and_workgroup(cuda, shapes):
    rng = np.random.default_rng(11)
    _check(cuda, [_rand(rng, m) for m, _ in shapes], [_rand(rng, n) for _, n in shapes])


def test_resident_limit_hand_over(cuda):
    """L - 1, L and L + 1 against 50, L from the library's own rule (both sides <= L: one workgroup, no workspace; beyond: tiled)."""
    from dynamic_asr_eval_amd import _lib
    L = int(_lib.load().dyn_edit_counts_resident_limit())
    assert 3 * 3 * 4 * L + 8 * L <= 160 * 1024 - 1024 < 44 * (L + 1)
    rng = np.random.default_rng(13)
    for k in (L - 1, L, L + 1):
        long, short = _rand(rng, k), _rand(rng, 50)
        assert (_ws_bytes([long], [short]) > 0) == (k > L) and (_ws_bytes([short], [long]) > 0) == (k > L)
        _check(cuda, [long, short], [short, long])


@pytest.mark.parametrize("shape", [(200, 130), (64, 64), (65, 129), (129, 65), (300, 63), (63, 300)])
def test_tiled_regime_forced_with_tile_64(cuda, shape):
    """Ragged block edges, a single block, block diagonals that grow and shrink, one block row / one block column."""
    rng = np.random.default_rng(17)
    hyp, ref = _rand(rng, shape[0]), _rand(rng, shape[1])
    assert _ws_bytes([hyp], [ref], 64) > 0 or shape == (64, 64)
    _check(cuda, [hyp], [ref], tile=64)


def test_tiled_and_resident_pairs_mixed_in_one_call(cuda):
    """40 pairs at tile = 64, lengths 0..150: more tiled pairs than one launch group holds, resident and empty pairs between them."""
    rng = np.random.default_rng(19)
    lens = [(0, 120), (120, 0), (64, 3), (3, 64), (63, 63)] + [tuple(rng.integers(0, 151, 2)) for _ in range(35)]
    assert sum(1 for m, n in lens if max(m, n) >= 64 and min(m, n) > 0) > 16 and sum(1 for m, n in lens if max(m, n) < 64) >= 3
    _check(cuda, [_rand(rng, m) for m, _ in lens], [_rand(rng, n) for _, n in lens], tile=64)
    _check(cuda, [_rand(rng, m) for m, _ in lens[:12]], [_rand(rng, n) for _, n in lens[:12]], tile=8)


def test_long_pair_at_the_default_tile(cuda):
    """2300 x 2250 over 40 symbols (resident at the default tile) and 4000 x 3900 (beyond the resident limit: 4 x 4 blocks of 1024)."""
    rng = np.random.default_rng(23)
    _check(cuda, [_rand(rng, 2300, 40)], [_rand(rng, 2250, 40)])
    hyp, ref = _rand(rng, 4000, 40), _rand(rng, 3900, 40)
    assert _ws_bytes([hyp], [ref]) == 3 * 4 * (3 * 4001 + 3 * 3901)
    _check(cuda, [hyp], [ref])


def test_near_identical_and_disjoint_sequences(cuda):
    """Long ties (a copy with about 1 % edits) and none (no common symbol), resident and tiled."""
    rng = np.random.default_rng(29)
    ref = _rand(rng, 2000, 30)
    hyp = []
    for t in ref:
        u = rng.random()
        if u < 0.004:
            continue                                   # deletion
        hyp.append(int(rng.integers(0, 30)) if u < 0.008 else t)
        if u > 0.996:
            hyp.append(int(rng.integers(0, 30)))       # insertion
    assert hyp != ref and abs(len(hyp) - len(ref)) < 40
    a, b = _rand(rng, 500, 5), [5 + t for t in _rand(rng, 700, 5)]
    for tile in (0, 256):
        got = _check(cuda, [hyp, ref, a, b], [ref, ref, b, a], tile=tile)
        assert tuple(got[1]) == (0, 0, 0, 2000) and tuple(got[2]) == (0, 200, 500, 700) and tuple(got[3]) == (200, 0, 500, 500)


REF_TEXT = "the quick brown fox jumps over the lazy dog and keeps on running through the field"
HYP_TEXTS = ["the quick brown fox jumps over the lazy dog and keeps on running through the field",
             "the quick brown fax jumps over lazy dog and and keeps running through the the field",
             "", "   ", "quick", "a completely different sentence with nothing shared at all in it",
             "the  quick brown fox jumps over the lazy dog and keeps on running through the fiel d",
             "thequickbrownfoxjumpsoverthelazydog"]


@pytest.mark.parametrize("ref", [REF_TEXT, "", "  "], ids=["text", "empty-ref", "blank-ref"])
def test_calc_rewards_device_equals_host_as_exact_floats(cuda, capsys, ref):
    from dynamic_asr_eval_amd.enc_dec import calc_rewards
    host = calc_rewards(ref, HYP_TEXTS)
    dev = calc_rewards(ref, HYP_TEXTS, device=cuda)
    assert len(dev) == 8 and dev == host and all(type(a) is type(b) for a, b in zip(dev, host))
    assert [x.hex() if isinstance(x, float) else x for x in dev] == [x.hex() if isinstance(x, float) else x for x in host]
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[0] == out[1] and out[0].endswith("avg reward")


def test_calc_rewards_scores_all_hypotheses_in_one_device_call(cuda, monkeypatch):
    from dynamic_asr_eval_amd import enc_dec as E
    calls = []
    real = E.edit_counts_ids

    def spy(hyp_ids, ref_ids, device, tile=0):
        calls.append(len(hyp_ids))
        return real(hyp_ids, ref_ids, device, tile=tile)
    monkeypatch.setattr(E, "edit_counts_ids", spy)
    E.calc_rewards(REF_TEXT, HYP_TEXTS, device=cuda)
    assert calls == [2 * len(HYP_TEXTS)]                # words and characters of every hypothesis together


def test_score_texts_and_character_scoring_on_the_device(cuda):
    from dynamic_asr_eval_amd import harness_common as H
    from dynamic_asr_eval_amd.wer import edit_counts, edit_counts_pairs, word_error_rate_detail
    preds, golds = HYP_TEXTS + [REF_TEXT], [REF_TEXT] * 8 + [""]
    assert H.score_texts(preds, golds, device=cuda) == H.score_texts(preds, golds)
    try:
        H.set_score_device(cuda)
        assert H.score_texts(preds, golds) == H.score_texts(preds, golds, device=None)
    finally:
        H.set_score_device(None)
    for use_cer in (False, True):
        assert edit_counts_pairs(preds, golds, use_cer=use_cer, device=cuda) == edit_counts_pairs(preds, golds, use_cer=use_cer)
        assert edit_counts(preds, golds, use_cer=use_cer, device=cuda) == edit_counts(preds, golds, use_cer=use_cer)
        assert word_error_rate_detail(preds, golds, use_cer=use_cer, device=cuda) == word_error_rate_detail(preds, golds, use_cer=use_cer)
    assert edit_counts_pairs(["a  b", " "], ["a b", "  "], use_cer=True, device=cuda) == [(1, 0, 0, 3), (0, 1, 0, 2)]


def test_argument_errors_are_codes_not_launches(cuda):
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ids = torch.zeros(400, dtype=torch.int32, device=cuda)
    counts = torch.full((1, 4), -5, dtype=torch.int32, device=cuda)
    off = np.array([0, 200, 0, 200], dtype=np.int64)
    dev_off = torch.from_numpy(off).to(cuda)
    ho, ro = off[:2], off[2:]
    need = lib.dyn_edit_counts_workspace_bytes(ho.ctypes.data, ro.ctypes.data, 1, 64)
    assert need == 2 * 3 * 201 * 3 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    args = (ids.data_ptr(), ids.data_ptr() + 800, ho.ctypes.data, ro.ctypes.data, dev_off.data_ptr(), counts.data_ptr())
    assert lib.dyn_edit_counts(*args, ws.data_ptr(), need - 4, 1, 64, st) == -3              # DYN_E_WORKSPACE
    assert b"workspace" in lib.dyn_last_error()
    assert lib.dyn_edit_counts(*args, None, 0, 1, 64, st) == -3
    bad = np.array([0, -200], dtype=np.int64)
    assert lib.dyn_edit_counts(args[0], args[1], bad.ctypes.data, ro.ctypes.data, *args[4:], ws.data_ptr(), need, 1, 64, st) == -1
    assert lib.dyn_edit_counts(args[0], args[1], ho.ctypes.data, bad.ctypes.data, *args[4:], ws.data_ptr(), need, 1, 64, st) == -1
    assert lib.dyn_edit_counts(*args, ws.data_ptr(), need, 1, 5, st) == -1                   # tile outside [8, 2048]
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [[-5, -5, -5, -5]]                                       # nothing ran
    assert lib.dyn_edit_counts(*args, ws.data_ptr(), need, 1, 64, st) == 0
    assert counts.cpu().tolist() == [[0, 0, 0, 200]]


def test_grpo_loop_with_device_rewards_equals_host_rewards_bit_for_bit(cuda, capsys, monkeypatch):
    """A 3-window grpo adaptation with rl_reward='wer_cer' on the small enc-dec model of tests/test_enc_dec_rl_gpu.py: rewards scored
    by dyn_edit_counts against `rl_reward_on_host=True` - the same printed rewards, the same parameters after the loop, bit for bit."""
    from enc_dec_rl_cpu import VOCAB, pair
    from oracle import dynamic_eval_ref as R
    from dynamic_asr_eval_amd import enc_dec as E
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    _, hip = pair(cuda, seed=7, eos_bias=0.0)
    tok = SyntheticTokenizer(VOCAB)
    spec = torch.randn(1, 80, 700, generator=torch.Generator().manual_seed(4))
    _, keys = R.prepare_chunks(spec, 256, 0)
    mg = torch.Generator().manual_seed(6)
    masks = {k: (R.draw_masks(3, 12, 80, mg), ([], [])) for k in keys}
    device_calls = []
    real = E.edit_counts_ids

    def spy(hyp_ids, ref_ids, device, tile=0):
        device_calls.append(len(hyp_ids))
        return real(hyp_ids, ref_ids, device, tile=tile)
    monkeypatch.setattr(E, "edit_counts_ids", spy)
    runs = {}
    for on_host in (True, False):
        args = argparse.Namespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 2048, 'overlap': 0}, 'training': {}},
                                  optim_lr=1e-4, epochs=1, shuffle=False, training_mode='grpo', spec_augment_fixed_masks=masks, random_seed=3,
                                  rl_reward='wer_cer', rl_reward_on_host=on_host)
        n_before = len(device_calls)
        text, params = E.enc_dec_dynamic_eval(args, hip, spec, 256, 0, tok, use_tqdm=False, return_params=True)
        out = capsys.readouterr().out
        rewards = [eval(l) for l in out.splitlines() if l.startswith("[") and l.endswith("]") and "w" not in l]
        runs[on_host] = (text, [p.detach().clone() for p in params], rewards, out.count(" loss\n"), len(device_calls) - n_before)
    host, dev = runs[True], runs[False]
    assert host[4] == 0 and dev[4] == len(dev[2]) == 3, "one device call per window, none when forced to the host"
    assert host[3] >= 1, "fixture: no window updated the parameters"
    assert dev[2] == host[2] and dev[3] == host[3] and dev[0] == host[0]
    assert len(dev[1]) == len(host[1]) and all(torch.equal(a, b) for a, b in zip(dev[1], host[1]))
