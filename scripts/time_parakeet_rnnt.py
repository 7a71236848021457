"""Timing of the RNN-T loss on the MI355X, one JSON line: ops.rnnt_loss forward + gradient next to ops.tdt_loss forward +
gradient at the same lattice [B, T', U + 1] with the released head width (V + 1 = 8193; TDT: + 5 duration columns, durations 0 .. 4), the
same token logits and targets.  One process, alternating, HIP events, median of 25 after a warm-up, eager launches; the TDT form is timed
TWICE in the same alternation: the difference of its medians is the run-to-run spread.  A record, not a gate: RNN-T has nothing to compare
against on the parent commit.
Usage: python scripts/time_parakeet_rnnt.py [--shapes B,T,U ...] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _median_us  # noqa: E402

V1, DURATIONS = 8193, (0, 1, 2, 3, 4)


def time_losses(dev, B, T, U, reps=25):
    from dynamic_asr_eval_amd import ops
    g = torch.Generator().manual_seed(100 * T + U)
    D = len(DURATIONS)
    x_tdt = torch.randn(B, T, U + 1, V1 + D, generator=g).to(dev)
    x_rnnt = x_tdt[..., :V1].contiguous()
    tg = torch.randint(0, V1 - 1, (B, U), generator=g, dtype=torch.int32).to(dev)
    il, tl = torch.full((B,), T, dtype=torch.int32, device=dev), torch.full((B,), U, dtype=torch.int32, device=dev)
    g_rnnt, g_tdt = torch.empty_like(x_rnnt), torch.empty_like(x_tdt)

    def rnnt():
        return ops.rnnt_loss(x_rnnt, tg, il, tl, V1 - 1, "sum", 1.0, out=g_rnnt)

    def tdt():
        return ops.tdt_loss(x_tdt, tg, il, tl, V1 - 1, DURATIONS, 0.0, "sum", 1.0, out=g_tdt)

    lr, lt = rnnt()[0].item(), tdt()[0].item()
    assert lr == lr and lt == lt and abs(lr) != float("inf") and abs(lt) != float("inf"), (lr, lt)
    (tr, tr_lo, tr_hi), (tt, tt_lo, tt_hi), (tu, tu_lo, tu_hi) = _median_us([rnnt, tdt, tdt], reps=reps, warm=5)
    return {"shape": [B, T, U + 1], "classes": V1, "rnnt_us": round(tr, 1), "rnnt_us_min_max": [round(tr_lo, 1), round(tr_hi, 1)],
            "tdt_us": round(tt, 1), "tdt_us_min_max": [round(tt_lo, 1), round(tt_hi, 1)], "tdt_again_us": round(tu, 1),
            "tdt_spread_us": round(abs(tt - tu), 1), "time_ratio_rnnt_over_faster_tdt": round(tr / min(tt, tu), 3),
            "state_bytes_rnnt_tdt": [ops._L().dyn_rnnt_loss_workspace_bytes(B, T, U + 1), ops._L().dyn_tdt_loss_workspace_bytes(B, T, U + 1, D)]}


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", nargs="*", default=["2,16,25", "2,64,41"])
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_parakeet_rnnt.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {"rnnt_vs_tdt_loss_fwd_grad": [time_losses(dev, *(int(v) for v in s.split(","))) for s in a.shapes]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
