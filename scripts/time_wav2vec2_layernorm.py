"""Timings of the layer-norm wav2vec2 layout on the MI355X, one JSON line:
  kernel  dyn_bias_layernorm_gelu_fwd / _bwd at the first extractor layer of a 131072-sample window with B = 2 ([2 x 26214, 512]) next to the
          same work composed from ops.axpby / ops.layernorm / ops.gelu and their backwards (+ ops.colsum for the bias gradient), in one
          process, alternating, HIP events, median of 15 after a warm-up; achieved bytes/s over the ALGORITHMIC bytes (forward: read z, write
          act; backward: read z and dact, write dz).
  loop    run_wav2vec2's per-utterance loop at the wav2vec2-large-960h-lv60-self architecture (tests/golden/wav2vec2_large_lv60_config.json,
          seeded weights) on the bench's synthetic talk, eager and with bucket graphs, audio-s/s.
Usage: python scripts/time_wav2vec2_layernorm.py [kernel] [loop] [--out FILE]"""
import argparse
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


def _median_us(fns, reps=15, warm=3):
    """Median of `reps` HIP-event timings per function, the functions alternating inside every repetition."""
    times = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            if r >= warm:
                times[k].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in times]


def time_kernel(dev, rows=2 * 26214, C=512):
    from dynamic_asr_eval_amd import ops
    g_ = torch.Generator().manual_seed(0)
    z = torch.randn(rows, C, generator=g_).to(dev)
    dact = torch.randn(rows, C, generator=g_).to(dev)
    cb, gamma, beta = (torch.randn(C, generator=g_).to(dev) for _ in range(3))
    dg, db, dc = (torch.zeros(C, device=dev) for _ in range(3))
    act, mean, rstd = ops.bias_layernorm_gelu(z, cb, gamma, beta)
    dz = torch.empty_like(z)
    cb_rows = cb.expand(rows, C).contiguous()                        # the composition has no broadcast add: z + bias as axpby over a bias tensor
    v, n = z.clone(), torch.empty_like(z)                            # the composition adds the bias in place (its LayerNorm backward needs z + bias)
    state = {}

    def fused_fwd():
        ops.bias_layernorm_gelu(z, cb, gamma, beta)

    def composed_fwd():
        ops.axpby(cb_rows, v, 1.0, 1.0)
        state["n"], state["mean"], state["rstd"] = ops.layernorm(v, gamma, beta, 1e-5, out=n)
        ops.gelu(n)

    def fused_bwd():
        ops.bias_layernorm_gelu_bwd(z, cb, gamma, beta, mean, rstd, dact, dg, db, dc, out=dz)

    def composed_bwd():
        dn = ops.gelu_bwd(n, dact)
        ops.layernorm_bwd(v, gamma, state["mean"], state["rstd"], dn, dz, dg, db, dx_beta=0.0)
        ops.colsum(dz, dc, beta=1.0)

    composed_fwd()
    t_ff, t_cf, t_fb, t_cb = _median_us([fused_fwd, composed_fwd, fused_bwd, composed_bwd])
    nbytes = rows * C * 4
    return {"shape": [rows, C], "tensor_MB": round(nbytes / 1e6, 1),
            "fused_fwd_us": round(t_ff, 1), "fused_fwd_TBps": round(2 * nbytes / t_ff / 1e6, 2),
            "composed_fwd_us": round(t_cf, 1),
            "fused_bwd_us": round(t_fb, 1), "fused_bwd_TBps": round(3 * nbytes / t_fb / 1e6, 2),
            "composed_bwd_us": round(t_cb, 1),
            "note": "composed forward = in-place axpby(bias rows) + layernorm + gelu; composed backward = gelu_bwd + layernorm_bwd + colsum"}


def time_loop(dev, seconds=300.0):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW, wav2vec2_lib as W
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC, config_from_json
    cfg = config_from_json(os.path.join(ROOT, "tests", "golden", "wav2vec2_large_lv60_config.json"))
    m = Wav2Vec2ForCTC(cfg, device=dev)
    RW.init_synthetic(m, 0)
    m.eval()
    utts = RW.fetch_utterances_synthetic(seconds, 7)
    audio_s = sum(u['waveform'].shape[-1] for u in utts) / 16000.0
    tok = W.CharTokenizer()

    def su(**kw):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        with redirect_stdout(io.StringIO()):
            W.dynamic_eval_su(argparse.Namespace(epochs=1, shuffle=False, **kw), m, [dict(u) for u in utts], 0, 0, tok, None, use_tqdm=False,
                              optim=W.MADGRAD, lr_args={'lr': 1e-6})
        torch.cuda.synchronize(dev)
        return time.time() - t0

    su(use_graphs=False)
    eager = min(su(use_graphs=False), su(use_graphs=False))
    su(); su()                                                       # a length bucket is captured the second time it is seen
    graphs = min(su(), su())
    return {"parameters_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 1), "utterances": len(utts), "audio_s": round(audio_s, 1),
            "eager_audio_s_per_s": round(audio_s / eager, 1), "bucket_graphs_audio_s_per_s": round(audio_s / graphs, 1),
            "buckets": len(m._graphs), "graph_GiB": round(m.graph_bytes() / 2 ** 30, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "loop"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    if "kernel" in a.what:
        res["bias_layernorm_gelu"] = time_kernel(dev)
    if "loop" in a.what:
        res["lv60_dynamic_eval_su"] = time_loop(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
