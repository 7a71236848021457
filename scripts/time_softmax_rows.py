"""Durations of the row-softmax kernels that share csrc/softmax_row.h, for comparing two builds under `rocprofv3 --kernel-trace --stats`
(each build from its own tree: the package is imported from this file's parent directory).
  run        launches ops.softmax (masked), ops.softmax_relbias, ops.softmax_relshift and ops.softmax_bwd on [2 x 16, T, T] scores at T = 500 and
             1500 (the shapes of scripts/time_wav2vec2_conformer.py: the large architecture's 16 heads), WARM launches per kernel and shape first,
             then REPS measured ones, the four kernels alternating.  To be run under the profiler:
               rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o p -- python scripts/time_softmax_rows.py run
  summarise  DIR [DIR ...] -> one JSON object per DIR: per kernel instance the mean / min / max duration in ns of its measured dispatches (the
             first WARM dispatches of every instance dropped), read from the profiler's kernel trace CSV.
Usage: python scripts/time_softmax_rows.py run | summarise DIR [DIR ...]"""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM, REPS = 10, 60
KERNELS = ("softmax_fwd_kernel", "softmax_relbias_fwd_kernel", "softmax_relshift_fwd_kernel", "softmax_bwd_kernel")


def run():
    import torch
    from dynamic_asr_eval_amd import ops
    dev = torch.device("cuda", 0)
    B, nh, D, nbk = 2, 16, 64, 320
    for T in (500, 1500):
        g = torch.Generator().manual_seed(T)
        S = torch.randn(B, nh, T, T, generator=g).to(dev)
        BD = torch.randn(B, nh, T, 2 * T - 1, generator=g).to(dev)
        gate = (1.0 + torch.rand(B, nh, T, generator=g)).to(dev)
        E = torch.randn(nbk, nh, generator=g).to(dev)
        table = ops.relative_position_buckets(T, nbk, 800).to(dev)
        valid = torch.tensor([T - 3], dtype=torch.int32, device=dev)
        out, P = torch.empty_like(S), ops.softmax(S)
        fns = (lambda: ops.softmax(S, out=out, valid=valid), lambda: ops.softmax_relbias(S, gate, E, table, D, out=out, valid=valid),
               lambda: ops.softmax_relshift(S, BD, out=out, valid=valid), lambda: ops.softmax_bwd(P, S, out=out))
        torch.cuda.synchronize(dev)
        for _ in range(WARM + REPS):
            for fn in fns:
                fn()
        torch.cuda.synchronize(dev)


def summarise(d):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"{d}: no kernel trace CSV")
    per = {}
    for path in paths:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if any(k + "<" in name for k in KERNELS):
                    short = name.split("::")[-1].split("(")[0]
                    per.setdefault(short, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    res = {}
    for name, spans in sorted(per.items()):
        ns = [e - s for s, e in sorted(spans)][WARM:]
        res[name] = {"dispatches": len(ns), "mean_ns": round(statistics.mean(ns), 1), "median_ns": statistics.median(ns), "min_ns": min(ns),
                     "max_ns": max(ns)}
    return res


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["summarise"] and len(sys.argv) > 2:
        print(json.dumps({d: summarise(d) for d in sys.argv[2:]}, indent=1))
    else:
        raise SystemExit(__doc__)
