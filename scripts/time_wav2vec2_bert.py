"""Timings of Wav2Vec2-BERT's new pieces on the MI355X, one JSON line:
  core      ops.convmod_causal (one launch; time tiles 8, 16 and the library's choice) next to the existing unfused SAME-padded chain at the
            same shape, which moves the same bytes: ops.glu, ops.dwconv1d, ops.layernorm, ops.silu.  One process, alternating, HIP events
            around 20 back-to-back calls, median of 15 such windows after a warm-up.
  de        ops.relkey_embed_grad (one batched product into per-(b, h) partials + the fixed-order reducer) next to the loop of per-(b, h)
            products with beta = 1 it replaces, checked against each other first.
  frontend  frontend.KaldiFbank on 10 s of audio (the whole chain: two GEMMs, power, finish).
  step      forward + backward of the full 24-layer, 1024-wide model (seeded weights) on a 10 s utterance, two copies, one active in the
            backward, as a dynamic_eval_su step runs it: eager and as a replayed length-bucket hipGraph.
Usage: python scripts/time_wav2vec2_bert.py [core] [de] [frontend] [step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _median_us(fns, reps=15, warm=3, inner=20):
    """Per function: (median, min, max) microseconds per call over `reps` windows of `inner` back-to-back calls, the functions alternating."""
    times = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if r >= warm:
                times[k].append(a.elapsed_time(b) * 1e3 / inner)
    return [[round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)] for t in times]


def time_core(dev, shape):
    from dynamic_asr_eval_amd import ops
    B, T, C = shape
    g = torch.Generator().manual_seed(T)
    u = torch.randn(B, T, 2 * C, generator=g).to(dev)
    w = (torch.randn(C, 31, generator=g) / 31 ** 0.5).to(dev)
    gamma, beta = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)

    def fused(tt, save):
        return lambda: ops.convmod_causal(u, w, gamma, beta, "swish", 1e-5, save=save, time_tile=tt)

    def chain():
        gl = ops.glu(u)
        dw = ops.dwconv1d(gl, w, None)
        n, _, _ = ops.layernorm(dw, gamma, beta, 1e-5)
        return ops.silu(n)

    names = ["fused_tile8", "fused_tile16", "fused_default", "fused_default_saving", "unfused_same_chain"]
    res = _median_us([fused(8, False), fused(16, False), fused(0, False), fused(0, True), chain])
    from dynamic_asr_eval_amd import _lib
    out = {"shape": list(shape), "default_time_tile": int(_lib.load().dyn_convmod_causal_time_tile(B, T))}
    out.update({n: r for n, r in zip(names, res)})
    out["bytes_moved_MB"] = round(4.0 * B * T * C * 3 / 1e6, 2)                # u in (2C), s out (C)
    return out


def time_de(dev, B=2, nh=16, T=750, P=73, D=64):
    from dynamic_asr_eval_amd import _attn, ops
    H, ldp, scale = nh * D, (P + 3) // 4 * 4, D ** -0.5
    g = torch.Generator().manual_seed(1)
    dc = torch.zeros(B, nh, T, ldp)
    dc[..., :P] = torch.randn(B, nh, T, P, generator=g)
    dc = dc.to(dev)
    qkv = torch.randn(B, T, 3 * H, generator=g).to(dev)
    q = _attn.packed(qkv, 0, D)
    out_a, out_b = torch.zeros(P, D, device=dev), torch.zeros(P, D, device=dev)

    def batched():
        return ops.relkey_embed_grad(dc, q, out_a, scale, beta=0.0)

    def loop():
        rev = torch.empty(P, D, device=dev)
        for b in range(B):
            for h in range(nh):
                ops.gemm(dc, qkv, rev, trans_a=True, M=P, N=D, K=T, lda=ldp, ldb=3 * H, ldc=D, a_off=(b * nh + h) * T * ldp,
                         b_off=b * T * 3 * H + h * D, alpha=scale, beta=0.0 if b + h == 0 else 1.0)
        return ops.axpby(rev.flip(0), out_b, 1.0, 0.0)

    batched(); loop()
    agree = (out_a - out_b).abs().max().item() / out_b.abs().max().item()
    assert agree < 1e-5, agree
    res = _median_us([batched, loop], inner=5)
    return {"shape": [B * nh, T, P, D], "reduction_length": B * nh * T, "batched_gemm_plus_reducer_us": res[0], "per_head_gemm_loop_us": res[1],
            "launches": {"batched": 4, "loop": B * nh + 2}, "relative_disagreement": float(f"{agree:.2e}")}


def time_frontend(dev, seconds=10.0):
    from dynamic_asr_eval_amd.frontend import KaldiFbank
    fe = KaldiFbank(dev)
    x = torch.randn(1, int(seconds * 16000), generator=torch.Generator().manual_seed(0)).to(dev)
    res = _median_us([lambda: fe(x)], inner=10)
    return {"audio_s": seconds, "us_per_call": res[0], "audio_s_per_s": round(seconds / (res[0][0] * 1e-6), 0)}


def time_step(dev, seconds=10.0):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    from dynamic_asr_eval_amd.wav2vec2_bert_model import Wav2Vec2BertForCTC
    m = Wav2Vec2BertForCTC(None, device=dev)
    RW.init_synthetic(m, 0)
    m.eval()
    L = int(seconds * 16000)
    x = torch.randn(2, L, generator=torch.Generator().manual_seed(0)).to(dev)
    T = m.conv_lengths(L)[-1]

    def step():
        with torch.enable_grad():
            out = m(x)
        gl = torch.zeros_like(out.logits[:1])
        gl[:, :out.frames] = 1e-3
        m.zero_grad()
        m.backward(gl, n_active=1)

    out = {"parameters_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 1), "audio_s": seconds, "frames": T, "copies": 2}
    m.use_graphs = False
    out["eager_ms"] = [round(v / 1e3, 2) for v in _median_us([step], reps=7, warm=2, inner=1)[0]]
    m.use_graphs, m.graph_after = True, 1
    out["graph_replay_ms"] = [round(v / 1e3, 2) for v in _median_us([step], reps=7, warm=3, inner=1)[0]]
    out["graph_GiB"] = round(m.graph_bytes() / 2 ** 30, 2)
    m.use_graphs = False
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["core", "de", "frontend", "step"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timings need the MI355X"
    dev = torch.device("cuda", 0)
    res = {}
    if "core" in a.what:
        res["causal_core_fwd"] = [time_core(dev, s) for s in ((2, 750, 1024), (2, 93, 1024), (1, 250, 1024), (2, 1500, 1024), (2, 750, 256))]
    if "de" in a.what:
        res["distance_embedding_grad"] = [time_de(dev), time_de(dev, T=93)]
    if "frontend" in a.what:
        res["frontend"] = time_frontend(dev)
    if "step" in a.what:
        res["full_model_step"] = time_step(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
