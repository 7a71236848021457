"""Timings of SEW-D on the MI355X, one JSON line:
  gather   the bucket gather of both position terms + masked softmax forward, and the gathers' backward, at scores [4, 12, 375, 375] with 256
           buckets over 512 positions (span 256, 512 rows): FUSED = dyn_softmax_disentangled_fwd + dyn_disentangled_bwd, next to the
           COMPOSITION of the same result on the GPU from torch.gather / index_add_ over MATERIALISED [T, T] index tensors (built once, not
           timed) and the project's plain masked softmax.  One process, alternating, HIP events, median of 25 after a warm-up, eager
           launches.  The composition is timed TWICE in the same alternation: the difference of its two medians is the run-to-run spread the
           fused form is held against.  The two forms are checked against each other before they are timed; the composition's index_add_
           uses float atomics, so its backward is not bit-reproducible and the fused one is compared to it with a tolerance.
  loop     wav2vec2_lib.dynamic_eval_su with seeded weights at SEWDConfig()'s shape (768 wide, 12 layers, 12 x 64 heads, FFN 3072,
           squeeze_factor 2, 256 buckets over 512 positions) beside SEWForCTC at the shape scripts/time_sew.py times (512 wide) in the same
           run, same synthetic talk, eager and with bucket graphs, audio-s/s: median, min and max of 3 timed passes each.
Usage: python scripts/time_sew_d.py [gather] [loop] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _Counted, _median_us, _su  # noqa: E402


def time_gather(dev, B=4, nh=12, T=375, buckets=256, max_position=512):
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.sew_d_model import att_span, bucket_table
    R = 2 * att_span(buckets, max_position)
    tab = bucket_table(T, buckets, max_position)
    table, lo, hi = (t.to(dev) for t in tab)
    g = torch.Generator().manual_seed(T)
    S = torch.randn(B, nh, T, T, generator=g).to(dev)
    c2p = torch.randn(B, nh, T, R, generator=g).to(dev)
    p2ct = torch.randn(B, nh, R, T, generator=g).to(dev)
    dS = (torch.randn(B, nh, T, T, generator=g) / T).to(dev)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    idx = tab.table.long()[i - j + T - 1].to(dev)                        # [T, T]: t(i - j), materialised as the composition needs it
    idx_c = idx.expand(B, nh, T, T).contiguous()                         # gather index of c2p [.., i, r]
    idx_p = idx.t().expand(B, nh, T, T).contiguous()                     # gather index of p2c [.., j, r] at [j, i]
    p2c = p2ct.transpose(-1, -2).contiguous()                            # the composition's layout, as transformers forms it

    def fused():
        y = ops.softmax_disentangled(S, c2p, p2ct, table, R, R)
        dc, dpt = ops.disentangled_bwd(dS, table, lo, hi, R)
        return y, dc, dpt

    def composed():
        x = S + torch.gather(c2p, -1, idx_c) + torch.gather(p2c, -1, idx_p).transpose(-1, -2)
        y = ops.softmax(x.contiguous())
        dc = torch.zeros_like(c2p).scatter_add_(-1, idx_c, dS)
        dp = torch.zeros_like(p2c).scatter_add_(-1, idx_p, dS.transpose(-1, -2).contiguous())
        return y, dc, dp

    yf, dcf, dpf = fused()
    yc, dcc, dpc = composed()
    agree = {"probabilities": (yf - yc).abs().max().item(), "dC2P": (dcf - dcc).abs().max().item() / dcc.abs().max().item(),
             "dP2C": (dpf.transpose(-1, -2) - dpc).abs().max().item() / dpc.abs().max().item()}
    assert all(v < 1e-4 for v in agree.values()), agree
    again = fused()
    bits = all(torch.equal(a, b) for a, b in zip((yf, dcf, dpf), again))
    with _Counted() as nf:
        fused()
    (tf, tf_lo, tf_hi), (tc, tc_lo, tc_hi), (td, td_lo, td_hi) = _median_us([fused, composed, composed], reps=25, warm=5)
    reach = int(((tab.lo <= tab.hi).sum()).item())
    return {"scores": [B, nh, T, T], "buckets": buckets, "max_position": max_position, "rows_of_embeddings": R, "rows_reached": reach,
            "fused_us": round(tf, 1), "fused_us_min_max": [round(tf_lo, 1), round(tf_hi, 1)], "fused_abi_calls": nf.n,
            "fused_bit_reproducible": bits, "composed_us": round(tc, 1), "composed_us_min_max": [round(tc_lo, 1), round(tc_hi, 1)],
            "composed_again_us": round(td, 1), "composed_again_us_min_max": [round(td_lo, 1), round(td_hi, 1)],
            "composed_spread_us": round(abs(tc - td), 1), "time_ratio_fused_over_composed": round(tf / min(tc, td), 3),
            "max_disagreement": {k: float(f"{v:.2e}") for k, v in agree.items()}}


def time_loop(dev, m, seconds, passes=3):
    """time_data2vec_audio.time_loop with `passes` timed passes per mode and their spread."""
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    RW.init_synthetic(m, 0)
    m.eval()
    utts = RW.fetch_utterances_synthetic(seconds, 7)
    audio_s = sum(u['waveform'].shape[-1] for u in utts) / 16000.0
    _su(m, utts, dev, use_graphs=False)
    eager = [audio_s / _su(m, utts, dev, use_graphs=False) for _ in range(passes)]
    _su(m, utts, dev); _su(m, utts, dev)                             # a length bucket is captured the second time it is seen
    graphs = [audio_s / _su(m, utts, dev) for _ in range(passes)]
    stat = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}  # noqa: E731
    return {"parameters_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 1), "utterances": len(utts), "audio_s": round(audio_s, 1),
            "passes": passes, "eager_audio_s_per_s": stat(eager), "bucket_graphs_audio_s_per_s": stat(graphs), "buckets": len(m._graphs),
            "graph_GiB": round(m.graph_bytes() / 2 ** 30, 2)}


def _commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip()
    except (OSError, subprocess.SubprocessError):
        return ""


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["gather", "loop"])
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="the commit the numbers belong to (default: git's HEAD when there is one)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"commit": a.commit or _commit(), "device": torch.cuda.get_device_name(dev)}
    if "gather" in a.what:
        res["gather_softmax_fwd_bwd"] = time_gather(dev)
    if "loop" in a.what:
        from dynamic_asr_eval_amd.sew_d_model import SEWDForCTC
        from dynamic_asr_eval_amd.sew_model import SEWForCTC
        sew = SEWForCTC(dict(hidden_size=512, num_attention_heads=8, intermediate_size=2048), device=dev)
        res["dynamic_eval_su"] = {"sew_d_768x12": time_loop(dev, SEWDForCTC(None, device=dev), a.seconds), "sew_512x12": time_loop(dev, sew, a.seconds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
