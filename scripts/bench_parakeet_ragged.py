"""What the per-row frame counts cost where nothing is masked: one ParakeetForCTC forward (no grad) of [8, 2048, 80] features at the released
size (DEFAULT_CONFIG: 24 layers, 1024 wide), with `input_lengths` = 2048 in every row against the call without them (the launch sequence
from before per-row counts existed: the scalar entries, bit for bit), and with lengths spread over 512 .. 2048 (the same launches: padding
is computed, only masked).  Median of 5 after 2 warm-ups, in ms.

    python scripts/bench_parakeet_ragged.py [--out profiles/parakeet_ragged_forward.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup=2, runs=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2048)
    args = ap.parse_args()
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    dev = torch.device("cuda:0")
    model = ParakeetForCTC(None, device=dev)
    g = torch.Generator().manual_seed(0)
    model.flat_params.copy_((0.02 * torch.randn(model.flat_params.numel(), generator=g)).to(dev))
    B, T = args.batch, args.frames
    x = torch.randn(B, T, model.n_mels, generator=g).to(dev)
    full = [T] * B
    spread = [T - (i * (T - T // 4)) // max(B - 1, 1) for i in range(B)]
    res = {"shape": [B, T, model.n_mels], "layers": model.cfg["num_hidden_layers"], "hidden_size": model.cfg["hidden_size"], "spread_lengths": spread}
    with torch.no_grad():
        assert torch.equal(model(x).logits, model(x, input_lengths=full).logits)
        for name, kw in (("no_lengths_ms", {}), ("full_lengths_ms", {"input_lengths": full}), ("spread_lengths_ms", {"input_lengths": spread}),
                         ("no_lengths_again_ms", {})):
            res[name], res[name + "_runs"] = timed(lambda: model(x, **kw))
    res["full_over_none"] = res["full_lengths_ms"] / res["no_lengths_ms"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
