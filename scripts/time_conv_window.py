"""Durations of the depthwise Conv1d kernels whose instruction stream changed when they moved onto csrc/dwconv_window.h, for comparing two
builds of the library (DYN_LIB_PATH picks the shared library) under `rocprofv3 --kernel-trace --stats`.
  run        launches, WARM times first and then REPS measured times, the kernels alternating:
               the 31-tap causal core forward (time tiles 8 and 16, SiLU), its dgrad and wgrad at (2, 750, 1024) and the forward at the
               library's tile at (2, 93, 1024) (scripts/time_wav2vec2_bert.py's shapes);
               the 9-tap causal core forward with the depthwise bias, its dgrad and wgrad at (3, 256, 1024) (scripts/time_nemotron_streaming.py's);
               convmod_bn and convmod_brn forward at 9 taps, (1, 2048, 1024), and at 32 taps, (1, 2048, 512) (Parakeet's and LASR's windows).
             To be run under the profiler:
               rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o p -- python scripts/time_conv_window.py run
  compare    PARENT_DIR THIS_DIR PARENT_DIR -> one JSON object, scripts/time_layernorm_rows.py's rule: the three runs (made in that order) side
             by side per kernel instance, the margin (the parent's own spread: the difference of its two run means) and `regression`: this
             build's mean is above the slower parent run by more than that margin.  The content of profiles/dwconv_window_timing.json.
Usage: python scripts/time_conv_window.py run | compare PARENT_DIR THIS_DIR PARENT_DIR"""
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM, REPS = 10, 60
# label -> the kernel's name before | after the move (template arguments included: one label per instance)
NAMES = (("causal31_fwd_tt%s", r"convmod_causal_fwd_kernel<31, (\d+), 4, 0(?:, false)?>"),
         ("causal31_dgrad", r"dwconv1d_causal_dgrad_kernel<31>|dwconv1d_kernel<31, 0, true>"),
         ("causal31_wgrad", r"dwconv1d_causal_wgrad_kernel<31>|dwconv1d_wgrad_kernel<31, 30, false>"),
         ("causal9_fwd", r"convmod_causal_k_fwd_kernel<9, 4>|convmod_causal_fwd_kernel<9, 8, 4, 0, true>"),
         ("causal9_dgrad", r"dwconv1d_causal_k_dgrad_kernel<9>|dwconv1d_kernel<9, 0, true>"),
         ("causal9_wgrad", r"dwconv1d_causal_k_wgrad_kernel<9>|dwconv1d_wgrad_kernel<9, 8, false>"),
         ("convmod_bn_fwd_kw%s", r"convmod_bn_fwd_kernel<(\d+), \d+>"),
         ("convmod_brn_conv_kw%s", r"convmod_brn_conv_kernel<(\d+), \d+>"))


def run():
    import torch
    from dynamic_asr_eval_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)       # noqa: E731
    fns = []

    def causal(B, T, C, KW, fwds, dgrad, wgrad):
        u, dy, w, gamma, beta, cb = rnd(B, T, 2 * C), rnd(B, T, C), rnd(C, KW) / 3, rnd(C), rnd(C), rnd(C)
        gl, dx, dw = rnd(B, T, C), torch.empty(B, T, C, device=dev), torch.zeros(C, KW, device=dev)
        fns.extend(f(u, w, cb, gamma, beta) for f in fwds)
        if dgrad:
            fns.extend([lambda: dgrad(dy, w, out=dx), lambda: wgrad(gl, dy, dw, beta=0.0)])

    tile = lambda tt: lambda u, w, cb, gamma, beta: lambda: ops.convmod_causal(u, w, gamma, beta, "swish", 1e-5, save=True, time_tile=tt)   # noqa: E731
    k9 = lambda u, w, cb, gamma, beta: lambda: ops.convmod_causal_k9(u, w, cb, gamma, beta, 1e-5, save=True)                             # noqa: E731
    causal(2, 750, 1024, 31, (tile(8), tile(16)), ops.dwconv1d_causal_dgrad, ops.dwconv1d_causal_wgrad)
    causal(2, 93, 1024, 31, (tile(0),), None, None)
    causal(3, 256, 1024, 9, (k9,), ops.dwconv1d_causal_k9_dgrad, ops.dwconv1d_causal_k9_wgrad)
    for KW, (B, T, C) in ((9, (1, 2048, 1024)), (32, (1, 2048, 512))):
        u, w, cb, mean, bw, bb = rnd(B, T, 2 * C), rnd(C, KW) / 3, rnd(C), rnd(C), rnd(C), rnd(C)
        var = torch.rand(C, generator=g).to(dev) + 0.5
        fns.append(lambda u=u, w=w, cb=cb, mean=mean, var=var, bw=bw, bb=bb: ops.convmod_bn(u, w, cb, mean, var, bw, bb, save=True))
        fns.append(lambda u=u, w=w, cb=cb, mean=mean, var=var, bw=bw, bb=bb: ops.convmod_brn(u, w, cb, mean.clone(), var.clone(), bw, bb, 3.0, 5.0, 0.0))
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
                for label, pat in NAMES:
                    m = re.search(pat, row["Kernel_Name"])
                    if m:
                        per.setdefault(label % m.groups() if m.groups() else label, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
                        break
    res = {}
    for name, spans in sorted(per.items()):
        ns = [e - s for s, e in sorted(spans)]
        ns = ns[-REPS * (len(ns) // (WARM + REPS)):]              # an instance launched from two shapes: the measured launches of both
        res[name] = {"dispatches": len(ns), "mean_ns": round(statistics.mean(ns), 1), "min_ns": min(ns), "max_ns": max(ns)}
    return res


def compare(parent_1, this, parent_2):
    a, b, c = summarise(parent_1), summarise(this), summarise(parent_2)
    out = {"unit": "ns, [mean, min, max] over the measured dispatches of a run (%d per launch site); runs in the order parent_1, this, parent_2" % REPS,
           "rule": "margin = |parent_1 mean - parent_2 mean|; regression = this mean > the slower parent mean + margin", "kernels": {}}
    for k in sorted(a):
        pm = (a[k]["mean_ns"], c[k]["mean_ns"])
        margin, over = abs(pm[0] - pm[1]), b[k]["mean_ns"] - max(pm)
        out["kernels"][k] = {"parent_1": [a[k][f] for f in ("mean_ns", "min_ns", "max_ns")], "this": [b[k][f] for f in ("mean_ns", "min_ns", "max_ns")],
                             "parent_2": [c[k][f] for f in ("mean_ns", "min_ns", "max_ns")], "margin_ns": round(margin, 1),
                             "this_minus_slower_parent_ns": round(over, 1), "regression": over > margin}
    out["regressions"] = [k for k, v in out["kernels"].items() if v["regression"]]
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 5:
        print(json.dumps(compare(*sys.argv[2:5]), indent=1))
    else:
        raise SystemExit(__doc__)
