"""Durations of the wave-per-row LayerNorm kernels that share csrc/layernorm_row.h, for comparing two builds of the library (DYN_LIB_PATH
picks the shared library) under `rocprofv3 --kernel-trace --stats`.
  run        launches, WARM times first and then REPS measured times, the kernels alternating:
               bias_layernorm_gelu forward + backward at rows = 52428, C = 512 (the layer-norm extractor's largest layer);
               layernorm forward + backward at rows = 8192, C = 768 (the flagship SCConformerXL: a lockstep group of 4 windows of 2048 frames);
               posconv_ln_gelu, squeeze_ln and squeeze forward + backward at B = 1, T = 1500, H = 768 (one utterance; 16 groups, s = 2);
               attn_adapter forward + backward at M = 1500, H = 1280, A = 16.
             To be run under the profiler:
               rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o p -- python scripts/time_layernorm_rows.py run
  summarise  DIR [DIR ...] -> one JSON object per DIR: per kernel instance the mean / min / max duration in ns of its measured dispatches (the
             last REPS dispatches of every instance: what comes before them is set-up and warm-up), read from the profiler's kernel trace CSV.
  compare    PARENT_DIR THIS_DIR PARENT_DIR -> one JSON object: the three runs (made in that order) side by side per kernel instance, the margin
             (the parent's own spread: the difference of its two run means) and `regression`: this build's mean is above the slower parent
             run by more than that margin.  The content of profiles/layernorm_row_timing.json.
Usage: python scripts/time_layernorm_rows.py run | summarise DIR [DIR ...] | compare PARENT_DIR THIS_DIR PARENT_DIR"""
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
KERNELS = ("blg_fwd_kernel", "blg_bwd_kernel", "norm_fwd_kernel", "norm_bwd_kernel", "pclg_fwd_kernel", "pclg_bwd_kernel", "sq_fwd_kernel",
           "sq_bwd_kernel", "adapter_fwd_kernel", "adapter_bwd_kernel")


def run():
    import torch
    from dynamic_asr_eval_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)       # noqa: E731
    fns = []
    # bias + LayerNorm + GELU: the extractor's largest layer
    rows, C = 52428, 512
    z, dact, gamma, beta, cb = rnd(rows, C), rnd(rows, C), rnd(C), rnd(C), rnd(C)
    _, mean, rstd = ops.bias_layernorm_gelu(z, cb, gamma, beta)
    dz, wg = torch.empty_like(z), [torch.zeros(C, device=dev) for _ in range(3)]
    fns += [lambda: ops.bias_layernorm_gelu(z, cb, gamma, beta),
            lambda: ops.bias_layernorm_gelu_bwd(z, cb, gamma, beta, mean, rstd, dact, *wg, out=dz)]
    # LayerNorm: the flagship model
    rows, C = 8192, 768
    x, dy, g7, b7 = rnd(rows, C), rnd(rows, C), rnd(C), rnd(C)
    y, m7, r7 = ops.layernorm(x, g7, b7)
    dx, dg7, db7 = torch.empty_like(x), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    fns += [lambda: ops.layernorm(x, g7, b7, out=y), lambda: ops.layernorm_bwd(x, g7, m7, r7, dy, dx, dg7, db7)]
    # the grouped-layout kernels: one utterance
    B, T, H, G, s = 1, 1500, 768, 16, 2
    yg, bias, gm, bt = rnd(B, G, T, H // G), rnd(H), rnd(H), rnd(H)
    h, dact3, dz2 = rnd(B, T, H), rnd(B, T, H), rnd(B, T // s, H)
    _, _, pm, pr = ops.posconv_ln_gelu(yg, bias, T)
    _, sm, sr = ops.squeeze_ln(h, yg, bias, gm, bt, s)
    dbias, dgm, dbt = (torch.zeros(H, device=dev) for _ in range(3))
    fns += [lambda: ops.posconv_ln_gelu(yg, bias, T), lambda: ops.posconv_ln_gelu_bwd(yg, bias, pm, pr, dact3, dbias),
            lambda: ops.squeeze_ln(h, yg, bias, gm, bt, s), lambda: ops.squeeze_ln_bwd(h, yg, bias, gm, sm, sr, dz2, s, dgm, dbt, dbias),
            lambda: ops.squeeze(h, yg, bias, s), lambda: ops.squeeze_bwd(yg, bias, dz2, T, s, dbias)]
    # the MMS adapter
    M, H, A = 1500, 1280, 16
    xa, dya, ga, ba, b2 = rnd(M, H), rnd(M, H), rnd(H), rnd(H), rnd(H)
    w1, w2, b1 = rnd(A, H) / H ** 0.5, rnd(H, A) / A ** 0.5, rnd(A)
    ya, am, ar, aa = ops.attn_adapter(xa, ga, ba, w1, b1, w2, b2, save=True)
    grads, dxa = [torch.zeros_like(t) for t in (ga, ba, w1, b1, w2, b2)], torch.empty_like(xa)
    fns += [lambda: ops.attn_adapter(xa, ga, ba, w1, b1, w2, b2, out=ya), lambda: ops.attn_adapter_bwd(xa, ga, ba, w1, w2, am, ar, aa, dya, *grads, dx=dxa)]
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
        ns = [e - s for s, e in sorted(spans)][-REPS:]
        res[name] = {"dispatches": len(ns), "mean_ns": round(statistics.mean(ns), 1), "median_ns": statistics.median(ns), "min_ns": min(ns),
                     "max_ns": max(ns)}
    return res


def compare(parent_1, this, parent_2):
    a, b, c = summarise(parent_1), summarise(this), summarise(parent_2)
    out = {"unit": "ns, [mean, min, max] over the %d measured dispatches of a run; runs in the order parent_1, this, parent_2" % REPS,
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
    elif sys.argv[1:2] == ["summarise"] and len(sys.argv) > 2:
        print(json.dumps({d: summarise(d) for d in sys.argv[2:]}, indent=1))
    else:
        raise SystemExit(__doc__)
