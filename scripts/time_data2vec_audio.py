"""Timings of Data2Vec-Audio on the MI355X, one JSON line:
  stack   the five-layer positional conv stack (H = 768, 16 groups, 19 taps, B = 1) forward + backward at T = 100, 500, 1500 as
          Data2VecAudioForCTC runs it (per layer: grouped GEMM + dyn_posconv_ln_gelu_fwd; dyn_posconv_ln_gelu_bwd + the weight- and
          data-gradient GEMMs + col2im + unpack) next to the SAME stack composed from the ops that existed before (group_unpack, layernorm
          with unit gamma, gelu, mask_rows, group_pack; gelu_bwd, layernorm_bwd, colsum, group_pack_grad) around the same GEMMs, both
          with a device-side valid length as under bucket replay; one process, alternating, HIP events, median of 15 after a warm-up,
          eager launches (no hipGraph).  The two are checked against each other before they are timed.
  loop    wav2vec2_lib.dynamic_eval_su at the base architecture (Data2VecAudioConfig() defaults = data2vec-audio-base-960h, seeded
          weights) beside Wav2Vec2ForCTC at its base architecture in the same run, on the synthetic talk time_wav2vec2_layernorm.py
          uses, eager and with bucket graphs, audio-s/s.
Usage: python scripts/time_data2vec_audio.py [stack] [loop] [--seconds S] [--out FILE]"""
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


class _Counted:
    """Counts the C-ABI calls (= kernel launch sequences) issued through ops' library handle while active."""

    def __init__(self):
        self.n = 0

    def __enter__(self):
        from dynamic_asr_eval_amd import ops
        self.ops, self.L = ops, ops._L
        lib, me = ops._L(), self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(lib, name)

                def call(*a):
                    me.n += 1
                    return fn(*a)
                return call
        proxy = Proxy()
        ops._L = lambda: proxy
        return self

    def __exit__(self, *exc):
        self.ops._L = self.L


def _composed(m, h, dhs, vT):
    """The stack forward + backward from the ops that existed before the fused kernels, on the model's weights; returns (pos, dh)."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.data2vec_audio_model import POS_LN_EPS
    c, P = m.cfg, m.P
    B, T, H = h.shape
    n, K, G = c["num_conv_pos_embeddings"], c["conv_pos_kernel_size"], c["num_conv_pos_embedding_groups"]
    cg, pad = H // G, K // 2
    Tp = T + 2 * pad
    one, zero = torch.ones(H, device=h.device), torch.zeros(H, device=h.device)
    junk_g, junk_b = torch.zeros(H, device=h.device), torch.zeros(H, device=h.device)
    kept, a = [], h
    for i in range(n):
        wn, bn = m._pos_names(i)
        xg = ops.group_pack(a, G, pad)
        yg = torch.empty(B, G, T, cg, device=h.device, dtype=torch.float32)
        ops.gemm(xg, P[wn], yg, trans_b=True, M=T, N=cg, K=K * cg, lda=cg, ldb=K * cg, ldc=cg, nb1=B, nb2=G,
                 sa=(G * Tp * cg, Tp * cg), sb=(0, cg * K * cg), sc=(G * T * cg, T * cg))
        pre = ops.group_unpack(yg, P[bn], T, H)
        nrm, mean, rstd = ops.layernorm(pre, one, zero, POS_LN_EPS)
        a = ops.mask_rows(ops.gelu(nrm), vT)
        kept.append((xg, pre, nrm, mean, rstd))
    pos, da = a, dhs
    for i in reversed(range(n)):
        xg, pre, nrm, mean, rstd = kept[i]
        wn, bn = m._pos_names(i)
        dn = ops.mask_rows(ops.gelu_bwd(nrm, da), vT)
        dpre = torch.empty_like(dn)
        ops.layernorm_bwd(pre, one, mean, rstd, dn, dpre, junk_g, junk_b, dx_beta=0.0)
        ops.colsum(dpre, m.G[bn], beta=1.0)
        dyg = ops.group_pack_grad(dpre, G, T)
        for b in range(B):
            ops.gemm(dyg, xg, m.G[wn], trans_a=True, M=cg, N=K * cg, K=T, lda=cg, ldb=cg, ldc=K * cg, nb1=1, nb2=G,
                     sa=(0, T * cg), sb=(0, Tp * cg), sc=(0, cg * K * cg), a_off=b * G * T * cg, b_off=b * G * Tp * cg, beta=1.0)
        dA = torch.empty(B, G, T, K * cg, device=h.device, dtype=torch.float32)
        ops.gemm(dyg, P[wn], dA, M=T, N=K * cg, K=cg, lda=cg, ldb=K * cg, ldc=K * cg, nb1=B, nb2=G, sa=(G * T * cg, T * cg),
                 sb=(0, cg * K * cg), sc=(G * T * K * cg, T * K * cg))
        dxg = torch.empty(B * G, Tp, cg, device=h.device, dtype=torch.float32)
        ops.col2im_1d(dA, dxg, B * G, Tp, T, cg, K, 1)
        da = ops.group_unpack_grad(dxg.view(B, G, Tp, cg), torch.empty_like(dhs), pad, beta=0.0)
    return pos, ops.mask_rows(da, vT)


def time_stack(dev, T, B=1):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    from dynamic_asr_eval_amd.data2vec_audio_model import Data2VecAudioForCTC
    m = Data2VecAudioForCTC(dict(num_hidden_layers=0), device=dev)           # the base widths; the encoder layers take no part
    RW.init_synthetic(m, 0)
    c = m.cfg
    H = c["hidden_size"]
    g = torch.Generator().manual_seed(T)
    h = torch.randn(B, T, H, generator=g).to(dev)
    dpos = (torch.randn(B, T, H, generator=g) / T).to(dev)
    vT = torch.tensor([T - 3], dtype=torch.int32, device=dev)
    h[:, T - 3:] = 0.0                                                        # as the model hands it over under bucket replay

    def fused():
        pos, kept = m._pos_embed(h, vT)
        # _pos_embed_bwd adds the stack's input gradient to the residual gradient in place: a fresh copy of dpos each time
        return pos, m._pos_embed_bwd(kept, dpos.clone(), B, lambda t: t, vT)

    def composed():
        return _composed(m, h, dpos, vT)

    m.zero_grad(); pf, df = fused(); gf = m.flat_grads.clone()
    m.zero_grad(); pc, dc = composed(); gc = m.flat_grads.clone()
    dc = dc + torch.where(torch.arange(T, device=dev)[None, :, None] < T - 3, dpos, torch.zeros_like(dpos))   # the residual term fused() carries
    agree = {"pos": (pf - pc).abs().max().item(), "dh": (df - dc).abs().max().item() / dc.abs().max().item(),
             "grads": (gf - gc).abs().max().item() / gc.abs().max().item()}
    assert agree["pos"] < 1e-4 and agree["dh"] < 1e-4 and agree["grads"] < 1e-4, agree
    with _Counted() as nf:
        fused()
    with _Counted() as nc:
        composed()
    (tf, tf_lo, tf_hi), (tc, tc_lo, tc_hi) = _median_us([fused, composed])
    return {"shape": [B, T, H], "layers": c["num_conv_pos_embeddings"], "taps": c["conv_pos_kernel_size"], "groups": c["num_conv_pos_embedding_groups"],
            "fused_us": round(tf, 1), "fused_us_min_max": [round(tf_lo, 1), round(tf_hi, 1)], "fused_abi_calls": nf.n,
            "composed_us": round(tc, 1), "composed_us_min_max": [round(tc_lo, 1), round(tc_hi, 1)], "composed_abi_calls": nc.n,
            "time_ratio_fused_over_composed": round(tf / tc, 3), "max_disagreement": {k: float(f"{v:.2e}") for k, v in agree.items()}}


def _su(m, utts, dev, **kw):
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    torch.cuda.synchronize(dev)
    t0 = time.time()
    with redirect_stdout(io.StringIO()):
        W.dynamic_eval_su(argparse.Namespace(epochs=1, shuffle=False, **kw), m, [dict(u) for u in utts], 0, 0, W.CharTokenizer(), None,
                          use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-6})
    torch.cuda.synchronize(dev)
    return time.time() - t0


def time_loop(dev, m, seconds):
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    RW.init_synthetic(m, 0)
    m.eval()
    utts = RW.fetch_utterances_synthetic(seconds, 7)
    audio_s = sum(u['waveform'].shape[-1] for u in utts) / 16000.0
    _su(m, utts, dev, use_graphs=False)
    eager = min(_su(m, utts, dev, use_graphs=False), _su(m, utts, dev, use_graphs=False))
    _su(m, utts, dev); _su(m, utts, dev)                             # a length bucket is captured the second time it is seen
    graphs = min(_su(m, utts, dev), _su(m, utts, dev))
    return {"parameters_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 1), "utterances": len(utts), "audio_s": round(audio_s, 1),
            "eager_audio_s_per_s": round(audio_s / eager, 1), "bucket_graphs_audio_s_per_s": round(audio_s / graphs, 1),
            "buckets": len(m._graphs), "graph_GiB": round(m.graph_bytes() / 2 ** 30, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["stack", "loop"])
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    if "stack" in a.what:
        res["positional_stack_fwd_bwd"] = [time_stack(dev, T) for T in (100, 500, 1500)]
    if "loop" in a.what:
        from dynamic_asr_eval_amd.data2vec_audio_model import Data2VecAudioForCTC
        from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
        res["base_dynamic_eval_su"] = {"data2vec_audio": time_loop(dev, Data2VecAudioForCTC(None, device=dev), a.seconds),
                                       "wav2vec2": time_loop(dev, Wav2Vec2ForCTC(None, device=dev), a.seconds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
