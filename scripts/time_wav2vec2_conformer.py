"""Timings of Wav2Vec2-Conformer on the MI355X, one JSON line:
  kernel  dyn_softmax_relshift_fwd_len next to the masked ops.softmax on the same [2 x 16, T, T] scores at T = 500 and 1500 (BD is
          [2 x 16, T, 2T - 1]), in one process, alternating, HIP events, median of 15 after a warm-up; achieved bytes/s over the ALGORITHMIC
          bytes (softmax: read S, write P; relshift: read S, read the T x T window of BD, write P: 1.5 x the plain softmax's traffic).
          A third timing, the plain masked softmax over the first T floats of every BD row (ldx = 2T - 1), shows what reading half of every
          unaligned (2T - 1)-float row costs on its own.
  loop    wav2vec2_lib.dynamic_eval_su at the published large architecture (tests/golden/wav2vec2_conformer_rel_pos_large_config.json, seeded
          weights; the rope variant is the same file with position_embeddings_type "rotary") on the synthetic talk time_wav2vec2_layernorm.py
          uses, eager and with bucket graphs, audio-s/s; for "relative" also the share of an eager pass spent in the BD-side products
          (linear_pos(pe), (q + v) P^T, dBD P, dBD^T (q + v); HIP events around those ops.gemm calls; dW_pos rides in the grouped
          weight-gradient launch and is not separable).
  profile one warm and one measured eager pass of the relative model, to be run under `rocprofv3 --kernel-trace --stats`;
  share   FILE_kernel_stats.csv of such a run -> the share of GPU kernel time spent in the four kernels of csrc/relshift.hip.
Usage: python scripts/time_wav2vec2_conformer.py [kernel] [loop] [profile] [share CSV] [--seconds S] [--out FILE]"""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import time
from contextlib import redirect_stdout

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_KERNELS = ("softmax_relshift_fwd_kernel", "relshift_bwd_kernel", "head_bias_add_kernel", "head_bias_bwd_kernel")


def _median_us(fns, reps=15, warm=3):
    """Median (and min, max) of `reps` HIP-event timings per function, the functions alternating inside every repetition."""
    times = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            if r >= warm:
                times[k].append(a.elapsed_time(b) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def time_kernel(dev, T, B=2, nh=16):
    from dynamic_asr_eval_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    S = torch.randn(B, nh, T, T, generator=g).to(dev)
    BD = torch.randn(B, nh, T, 2 * T - 1, generator=g).to(dev)
    out = torch.empty_like(S)
    valid = torch.tensor([T - 3], dtype=torch.int32, device=dev)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream

    def softmax_of_bd_rows():       # the plain masked softmax over the first T floats of every (2T - 1)-float row of BD: two arrays, strided rows
        _lib.check(lib.dyn_softmax_fwd_len(BD.data_ptr(), out.data_ptr(), B * nh * T, T, 2 * T - 1, T, valid.data_ptr(), st), "dyn_softmax_fwd_len")

    (rs, rs_lo, rs_hi), (sm, sm_lo, sm_hi), (sb, _, _) = _median_us([lambda: ops.softmax_relshift(S, BD, out=out, valid=valid),
                                                                    lambda: ops.softmax(S, out=out, valid=valid), softmax_of_bd_rows])
    nbytes = S.numel() * 4
    return {"shape": [B * nh, T, T], "scores_MB": round(nbytes / 1e6, 1),
            "softmax_relshift_us": round(rs, 1), "softmax_relshift_us_min_max": [round(rs_lo, 1), round(rs_hi, 1)],
            "softmax_relshift_TBps": round(3 * nbytes / rs / 1e6, 2),
            "masked_softmax_us": round(sm, 1), "masked_softmax_us_min_max": [round(sm_lo, 1), round(sm_hi, 1)],
            "masked_softmax_TBps": round(2 * nbytes / sm / 1e6, 2), "masked_softmax_of_bd_rows_us": round(sb, 1),
            "time_ratio": round(rs / sm, 2), "expected_ratio": 1.5}


def _model(dev, pos):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    from dynamic_asr_eval_amd import wav2vec2_conformer_model as M
    cfg = dict(M.config_from_json(os.path.join(ROOT, "tests", "golden", "wav2vec2_conformer_rel_pos_large_config.json")), position_embeddings_type=pos)
    m = M.Wav2Vec2ConformerForCTC(cfg, device=dev)
    RW.init_synthetic(m, 0)
    return m.eval()


def _su(m, utts, dev, **kw):
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    torch.cuda.synchronize(dev)
    t0 = time.time()
    with redirect_stdout(io.StringIO()):
        W.dynamic_eval_su(argparse.Namespace(epochs=1, shuffle=False, **kw), m, [dict(u) for u in utts], 0, 0, W.CharTokenizer(), None,
                          use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-6})
    torch.cuda.synchronize(dev)
    return time.time() - t0


def _bd_gemm_share(m, utts, dev):
    """Share of one eager pass's wall time inside the ops.gemm calls one of whose sizes is the 2T - 1 relative positions of the utterance in
    flight (HIP events around each of them, read after the pass)."""
    from dynamic_asr_eval_amd import ops
    cur, pairs = {"R": -1}, []
    gemm, table = ops.gemm, m.position_table

    def position_table(T):
        cur["R"] = 2 * T - 1
        return table(T)

    def timed(a, b, c, **kw):
        if cur["R"] not in (kw["M"], kw["N"], kw["K"]):
            return gemm(a, b, c, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = gemm(a, b, c, **kw)
        e1.record()
        pairs.append((e0, e1))
        return out

    ops.gemm, m.position_table = timed, position_table
    try:
        wall = _su(m, utts, dev, use_graphs=False)
    finally:
        ops.gemm = gemm
        del m.position_table
    return round(sum(a.elapsed_time(b) for a, b in pairs) / 1e3 / wall, 3), len(pairs)


def time_loop(dev, pos, seconds):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    m = _model(dev, pos)
    utts = RW.fetch_utterances_synthetic(seconds, 7)
    audio_s = sum(u['waveform'].shape[-1] for u in utts) / 16000.0
    _su(m, utts, dev, use_graphs=False)
    eager = min(_su(m, utts, dev, use_graphs=False), _su(m, utts, dev, use_graphs=False))
    res = {"parameters_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 1), "utterances": len(utts), "audio_s": round(audio_s, 1),
           "eager_audio_s_per_s": round(audio_s / eager, 1)}
    if pos == "relative":
        res["bd_side_gemm_share_of_eager_pass"], res["bd_side_gemm_calls"] = _bd_gemm_share(m, utts, dev)
    _su(m, utts, dev); _su(m, utts, dev)                             # a length bucket is captured the second time it is seen
    graphs = min(_su(m, utts, dev), _su(m, utts, dev))
    res.update({"bucket_graphs_audio_s_per_s": round(audio_s / graphs, 1), "buckets": len(m._graphs), "graph_GiB": round(m.graph_bytes() / 2 ** 30, 2)})
    return res


def kernel_share(path):
    """rocprofv3's kernel stats CSV (Name, Calls, TotalDurationNs, ..., Percentage) -> share of GPU kernel time per new kernel."""
    tot, mine = 0.0, {k: 0.0 for k in NEW_KERNELS}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            tot += ns
            for k in NEW_KERNELS:
                if k in row["Name"]:
                    mine[k] += ns
    out = {k: round(v / tot, 4) for k, v in mine.items()}
    out["all_four"] = round(sum(mine.values()) / tot, 4)
    out["gpu_kernel_ms_total"] = round(tot / 1e6, 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "loop"])
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {}
    if "share" in a.what:
        res["relshift_kernels_share_of_gpu_kernel_time"] = kernel_share(a.what[a.what.index("share") + 1])
    else:
        dev = torch.device("cuda", 0)
        if "kernel" in a.what:
            res["softmax_relshift"] = [time_kernel(dev, T) for T in (500, 1500)]
        if "loop" in a.what:
            res["large_dynamic_eval_su"] = {pos: time_loop(dev, pos, a.seconds) for pos in ("relative", "rotary")}
        if "profile" in a.what:
            from dynamic_asr_eval_amd import run_wav2vec2 as RW
            m = _model(dev, "relative")
            utts = RW.fetch_utterances_synthetic(a.seconds, 7)
            _su(m, utts, dev, use_graphs=False)
            res["profiled_eager_pass_s"] = round(_su(m, utts, dev, use_graphs=False), 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
