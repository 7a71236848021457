#!/usr/bin/env python3
"""Host `wer._align` against the device path (dyn_edit_counts, upload and download included) in one process on one MI355X, written to
profiles/edit_counts_timing.json:

  per_call   8 pairs of ~1500 characters, 8 pairs of ~250 words, one 9000 x 9000-word pair, eleven 2250-word pairs in one call;
             median of `--repeats` timed calls after a warm-up, host and device alternating, counts asserted equal.
  rl_step    one grpo window (4 sampled rollouts of up to 256 tokens, rl_reward='wer_cer') on the default enc-dec model, the whole
             enc_dec_dynamic_eval call of a one-window recording: rewards scored on the host (`rl_reward_on_host=True`, which is the
             code path of the commit before the device path existed) against on the device, A B A B.
  --config5 1 adds the cross-dataset harness at its stated shapes (scripts/run_config5_full.py's configuration) with every
             score_texts call timed both ways.

  python scripts/time_edit_counts.py [--out profiles/edit_counts_timing.json] [--repeats 7] [--rl 1] [--config5 0]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def noisy_copy(rng, ref, alphabet, rate=0.15):
    """A hypothesis-like copy: `rate` of the tokens substituted, deleted or followed by an insertion."""
    out = []
    for t in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(int(rng.integers(0, alphabet)) if u < 2 * rate / 3 else t)
        if u > 1 - rate / 3:
            out.append(int(rng.integers(0, alphabet)))
    return out


def per_call(dev, repeats):
    from dynamic_asr_eval_amd.wer import _align, edit_counts_ids
    rng = np.random.default_rng(0)
    cases = {}
    for name, pairs, n, alphabet in (("8_pairs_1500_chars", 8, 1500, 28), ("8_pairs_250_words", 8, 250, 4000),
                                     ("1_pair_9000_words", 1, 9000, 4000), ("11_pairs_2250_words", 11, 2250, 4000)):
        refs = [rng.integers(0, alphabet, n).tolist() for _ in range(pairs)]
        cases[name] = ([noisy_copy(rng, r, alphabet) for r in refs], refs)
    out = {}
    for name, (hyps, refs) in cases.items():
        host_reps = repeats if name != "1_pair_9000_words" else min(repeats, 3)
        edit_counts_ids(hyps, refs, dev)                                  # warm-up: code object, pinned and device allocations
        t_host, t_dev, want = [], [], None
        for k in range(repeats):
            if k < host_reps:
                t0 = time.perf_counter()
                want = [_align(h, r) + (len(r),) for h, r in zip(hyps, refs)]
                t_host.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = edit_counts_ids(hyps, refs, dev)                        # ends in a stream synchronise (the download)
            t_dev.append(time.perf_counter() - t0)
            assert [tuple(int(x) for x in row) for row in got] == want, name
        h, d = statistics.median(t_host), statistics.median(t_dev)
        out[name] = {"host_ms": round(h * 1e3, 3), "device_ms": round(d * 1e3, 3), "host_over_device": round(h / d, 1),
                     "device_faster": d < h, "host_ms_all": [round(x * 1e3, 3) for x in t_host],
                     "device_ms_all": [round(x * 1e3, 3) for x in t_dev], "hyp_lengths": [len(x) for x in hyps]}
        print(name, out[name]["host_ms"], "ms host,", out[name]["device_ms"], "ms device", flush=True)
    return out


def rl_step(dev, rounds):
    from dynamic_asr_eval_amd import enc_dec as E, lib
    from dynamic_asr_eval_amd import enc_dec_dynamic_eval_test as T
    args = lib.apply_args(T.build_parser(), ["-seq", "2048", "-nv", "--training_mode", "grpo", "-epochs", "1", "-kwargs", "optim_lr=1e-6",
                                             "vocab_size=4095", "quiet=True", "rl_reward='wer_cer'", "blank_bias=1.34"])
    model, tok = T.load_enc_dec_model(args, dev)
    spec = torch.randn(1, 80, 2048, generator=torch.Generator().manual_seed(1))
    lengths = []
    real = E.calc_rewards

    def recording(ref, hyps, device=None):
        lengths.append({"ref_words": len(ref.split()), "ref_chars": len(ref), "hyp_words": [len(h.split()) for h in hyps],
                        "hyp_chars": [len(h) for h in hyps]})
        t0 = time.perf_counter()
        r = real(ref, hyps, device=device)
        lengths[-1]["reward_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        return r
    E.calc_rewards = recording
    times = {True: [], False: []}
    reward_ms = {True: [], False: []}
    texts = {}
    try:
        for k in range(1 + rounds):                                       # round 0 is the warm-up of both paths
            for on_host in (True, False):
                args.rl_reward_on_host = on_host
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    text = E.enc_dec_dynamic_eval(args, model, spec, 2048, 0, tok, use_tqdm=False)
                torch.cuda.synchronize()
                if k:
                    times[on_host].append(time.perf_counter() - t0)
                    reward_ms[on_host].append(lengths[-1]["reward_ms"])
                texts.setdefault(on_host, text)
                assert texts[on_host] == text
    finally:
        E.calc_rewards = real
    assert texts[True] == texts[False], "host and device rewards must give the same adaptation"
    h, d = times[True], times[False]
    return {"what": "enc_dec_dynamic_eval of a one-window (2048-frame) recording, grpo, 4 rollouts capped at 256 tokens, default enc-dec model, "
                    "vocab 4095; A = rewards on the host (the previous code path), B = rewards on the device, A B A B",
            "host_rewards_s": [round(x, 4) for x in h], "device_rewards_s": [round(x, 4) for x in d],
            "host_rewards_median_s": round(statistics.median(h), 4), "device_rewards_median_s": round(statistics.median(d), 4),
            "host_spread_s": round(max(h) - min(h), 4), "device_spread_s": round(max(d) - min(d), 4),
            "calc_rewards_host_ms": reward_ms[True], "calc_rewards_device_ms": reward_ms[False], "window": lengths[-1]}


def config5(dev):
    """The cross-dataset harness at its stated shapes; every score_texts call is answered by the device path and timed, then the same
    corpus is scored on the host and timed (outside the harness's own flow only in that the host result is compared, not returned)."""
    from dynamic_asr_eval_amd import harness_common as H, lib, run_cross_dataset_eval as X
    import tempfile
    argv = ["-d", "synthetic", "-d2", "synthetic_tedlium", "-split", "test", "-seq", "16384", "-o", "14336", "-ds", "-nv", "-epochs", "1",
            "-kwargs", "optim_lr=9e-5", "spec_augment_n_freq_masks=6", "spec_augment_freq_mask_param=34", "spec_augment_n_time_masks=0",
            "vocab_size=4095", "quiet=True", "blank_bias=1.34"]
    t_dev, t_host, sizes = [], [], []
    real = H.score_texts

    def timed(preds, golds, reduce_over_ranks=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = real(preds, golds, reduce_over_ranks=reduce_over_ranks, device=dev)
        t_dev.append(time.perf_counter() - t0)
        H.set_score_device(None)                                          # device=None must mean the host here
        t0 = time.perf_counter()
        want = real(preds, golds, reduce_over_ranks=reduce_over_ranks, device=None)
        t_host.append(time.perf_counter() - t0)
        H.set_score_device(dev)
        assert r == want
        sizes.append([len(g.split()) for g in golds])
        print(f"score_texts call {len(t_dev)}: {len(golds)} recordings, device {t_dev[-1]:.3f} s, host {t_host[-1]:.3f} s", file=sys.__stdout__, flush=True)
        return r
    X.score_texts = timed
    try:
        with tempfile.TemporaryDirectory() as tmp:
            args = lib.apply_args(X.build_parser(), argv + ["-s", os.path.join(tmp, "c5.pkl")])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                X.main(args)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
    finally:
        X.score_texts = real
        H.set_score_device(None)
    return {"what": "run_cross_dataset_eval, A = 6 x 1 h, B = 11 x 15 min, -seq 16384 -o 14336, one GPU; wall includes BOTH scorings of every corpus",
            "wall_s": round(wall, 2), "score_calls": len(t_dev), "recordings_scored": sum(len(s) for s in sizes),
            "scoring_device_s": round(sum(t_dev), 3), "scoring_host_s": round(sum(t_host), 3),
            "wall_with_host_scoring_only_s": round(wall - sum(t_dev), 2), "wall_with_device_scoring_only_s": round(wall - sum(t_host), 2),
            "host_share_of_wall_with_host_scoring": round(sum(t_host) / (wall - sum(t_dev)), 4), "reference_words_per_call": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_counts_timing.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rl", type=int, default=1)
    ap.add_argument("--rl_rounds", type=int, default=3)
    ap.add_argument("--config5", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "clock": "time.perf_counter around calls that end in a stream synchronise",
           "per_call": per_call(dev, a.repeats)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    save()
    if a.rl:
        rec["rl_step"] = rl_step(dev, a.rl_rounds)
        print("rl_step", rec["rl_step"]["host_rewards_s"], rec["rl_step"]["device_rewards_s"], flush=True)
        save()
    if a.config5:
        rec["cross_dataset"] = config5(dev)
        print("cross_dataset", {k: v for k, v in rec["cross_dataset"].items() if k != "reference_words_per_call"}, flush=True)
        save()
    print(json.dumps({k: (v if k != "cross_dataset" else "...") for k, v in rec.items()})[:2000])


if __name__ == "__main__":
    main()
