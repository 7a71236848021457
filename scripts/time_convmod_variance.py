"""The fused conv-module kernel (csrc/convmod.hip) on two builds of the library: durations of its LayerNorm instances and digests of its
RMSNorm outputs.  The build is chosen by DYN_LIB_PATH (dynamic_asr_eval_amd/_lib.py); the package is imported from this file's parent directory.
  run        launches ops.convmod_fwd (save on, as the training step does) for the four LayerNorm instances C = 256, 512, 768, 1024 at
             B = 2, T = 2048: WARM launches per instance first, then REPS measured ones, the four instances alternating.  To be run under
             the profiler:  rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o p -- python scripts/time_convmod_variance.py run
  summarise  DIR [DIR ...] -> one JSON object per DIR: per kernel instance the mean / median / min / max duration in ns of its measured
             dispatches (the first WARM dispatches of every instance dropped), read from the profiler's kernel trace CSV.
  digest     SHA-256 over the raw float32 bits of `s` and `rstd` of every RMSNorm case of tests/test_conv_kernels_gpu.py (all four
             instances, T in {1, 13} and 3, 4, 5, 9 at C = 256, NULL bias, the offset cases): one JSON object {case: digest}.  Two builds
             whose RMSNorm instantiations compute the same thing print the same object.
Usage: python scripts/time_convmod_variance.py run | summarise DIR [DIR ...] | digest"""
import csv
import glob
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WARM, REPS = 10, 60
KERNEL = "convmod_fwd_kernel"


def run():
    import torch
    from dynamic_asr_eval_amd import ops
    dev = torch.device("cuda", 0)
    B, T = 2, 2048
    fns = []
    for C in (256, 512, 768, 1024):
        g = torch.Generator().manual_seed(C)
        u, w, bias, gamma, beta = (torch.randn(s_, generator=g).to(dev) for s_ in ((B, T, 2 * C), (C, 9), (C,), (C,), (C,)))
        fns.append(lambda u=u, w=w, bias=bias, gamma=gamma, beta=beta: ops.convmod_fwd(u, w, bias, gamma, beta, True, 1e-5, True))
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
                if KERNEL + "<" in name:
                    short = name.split("::")[-1].split("(")[0]
                    per.setdefault(short, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    res = {}
    for name, spans in sorted(per.items()):
        ns = [e - s for s, e in sorted(spans)][WARM:]
        res[name] = {"dispatches": len(ns), "mean_ns": round(statistics.mean(ns), 1), "median_ns": statistics.median(ns), "min_ns": min(ns),
                     "max_ns": max(ns)}
    return res


def digest():
    import torch
    import kernel_refs as K
    import test_conv_kernels_gpu as TC
    from dynamic_asr_eval_amd import ops
    dev = torch.device("cuda", 0)

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    res = {}
    for C in (256, 512, 768, 1024):
        for T, seed, with_bias in [(T, T, True) for T in (1, 13) + ((3, 4, 5, 9) if C == 256 else ())] + [(13, 77, False)]:
            u, w, bias, gamma, _ = TC._convmod_inputs(2, T, C, seed)
            s, _, _, _, _, rstd = ops.convmod_fwd(u.to(dev), w.to(dev), bias.to(dev) if with_bias else None, gamma.to(dev), None, False, 1e-5, True)
            res[f"C{C}.T{T}.bias{int(with_bias)}.s"], res[f"C{C}.T{T}.bias{int(with_bias)}.rstd"] = sha(s), sha(rstd)
    for C in (256, 1024):
        u, w, _, gamma, _ = TC._convmod_inputs(2, 9, C, seed=9)
        for m in (0.0,) + K.COLNORM_RATIOS:
            bias = (m + 0.1 * torch.randn(C, generator=K.gen(16500 + C))).float()
            s, _, _, _, _, rstd = ops.convmod_fwd(u.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), None, False, 1e-5, True)
            res[f"offset.C{C}.m{m:g}.s"], res[f"offset.C{C}.m{m:g}.rstd"] = sha(s), sha(rstd)
    return res


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["summarise"] and len(sys.argv) > 2:
        print(json.dumps({d: summarise(d) for d in sys.argv[2:]}, indent=1))
    elif sys.argv[1:2] == ["digest"]:
        print(json.dumps(digest(), indent=1, sort_keys=True))
    else:
        raise SystemExit(__doc__)
