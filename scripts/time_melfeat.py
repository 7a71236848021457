"""Timing of the FastConformer family's waveform front end on the MI355X ("Waveform front end of the FastConformer family"),
one JSON line, for the record only: nothing comparable exists before it, no threshold is set.
  melfeat_1h_ms        frontend.MelFeatures("parakeet", 80) on one 1 h recording (B = 1, 57.6 M samples, 360 001 frames)
  melfeat_16x30s_ms    the same front end on 16 rows of 30 s (ragged by a few thousand samples)
  logmel_1h_ms         the existing frontend.LogMel on the same 1 h recording
Each figure: a host clock around `--reps` calls that end in a device synchronise, after a warm-up call of the same shape; the median with
its min and max.  Seeded noise at 0.1 amplitude; the device allocations of a call are part of it (torch's caching allocator, warm).
Usage: python scripts/time_melfeat.py [--reps 10] [--seconds 3600] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _wall_ms(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--seconds", type=int, default=3600)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_melfeat.py measures on the GPU: none found")
    from dynamic_asr_eval_amd import frontend
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    long = (0.1 * torch.randn(1, a.seconds * 16000, generator=g)).to(dev)
    rows = (0.1 * torch.randn(16, 480000, generator=g)).to(dev)
    lens = [480000 - 1234 * b for b in range(16)]
    mel, logmel = frontend.MelFeatures("parakeet", 80, dev), frontend.LogMel(dev)
    res = {"reps": a.reps, "seconds": a.seconds, "columns": ["median_ms", "min_ms", "max_ms"]}
    res["melfeat_1h_ms"] = _wall_ms(lambda: mel(long), a.reps, dev)
    res["melfeat_1h_ft_ms"] = _wall_ms(lambda: mel(long, layout="ft"), a.reps, dev)
    res["melfeat_16x30s_ms"] = _wall_ms(lambda: mel(rows, lens), a.reps, dev)
    res["logmel_1h_ms"] = _wall_ms(lambda: logmel(long[0]), a.reps, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
