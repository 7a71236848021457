"""Timings of Parakeet on the MI355X, one JSON line:
  convmod  the conv-module core between the two pointwise convolutions, forward + backward, at [B, T, C] = [5, 256, 1024] (the reference's
           default window of 2048 spectrogram frames at 5 copies) and [5, 2048, 1024]: FUSED = dyn_convmod_bn_fwd + dyn_convmod_bn_bwd_act +
           dyn_dwconv1d_wgrad + dyn_glu_dwconv1d_dgrad, next to the COMPOSITION it replaces, the statements of
           wav2vec2_conformer_model._conv_fwd / _conv_bwd between the same two points: glu, dwconv1d, chanaffine, silu; silu_bwd,
           chanaffine_bwd, dwconv1d_wgrad, dwconv1d_dgrad, glu_bwd.  One process, alternating, HIP events, median of 25 after a warm-up,
           eager launches.  The composition is timed TWICE in the same alternation: the difference of its medians is the run-to-run spread
           the fused form is held against.  The two forms are checked against each other before they are timed.
  loop     nvidia_ctc_lib.dynamic_eval (seq_len 2048, 4 augmented copies + 1 clean, Adam) over a synthetic 10-minute spectrogram
           [1, 80, 60000] with seeded weights at the 0.6b shape (24 layers, 1024 wide, 8 heads, FFN 4096, vocabulary 1025): three passes
           after a warm-up pass over both window shapes, audio-s/s from a host clock around a pass that ends in a device synchronise.
Usage: python scripts/time_parakeet.py [convmod] [loop] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _Counted, _median_us  # noqa: E402

EPS, KW = 1e-5, 9


def time_convmod(dev, B, T, C, reps=25):
    from dynamic_asr_eval_amd import ops
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                                          # noqa: E731
    u, w, cb, mean, var, gamma, beta = r(B, T, 2 * C), r(C, KW) * 0.3, r(C) * 0.2, r(C) * 0.1, (0.5 + torch.rand(C, generator=g)).to(dev), 1 + 0.1 * r(C), r(C) * 0.1
    ds = r(B, T, C) / T
    grads = dict(w=torch.zeros(C, KW, device=dev), cb=torch.zeros(C, device=dev), gamma=torch.zeros(C, device=dev), beta=torch.zeros(C, device=dev))

    def fused():
        s, gl, c = ops.convmod_bn(u, w, cb, mean, var, gamma, beta, "silu", EPS, save=True)
        dc = ops.convmod_bn_bwd_act(c, mean, var, gamma, beta, ds, grads["gamma"], grads["beta"], grads["cb"], "silu", EPS, wgrad_beta=0.0)
        ops.dwconv1d_wgrad(gl, dc, grads["w"], None, beta=0.0)
        return s, ops.glu_dwconv1d_dgrad(u, w, dc)

    def composed():
        gl = ops.glu(u)
        dw = ops.dwconv1d(gl, w, cb)
        bn = ops.chanaffine(dw, mean, var, gamma, beta, EPS)
        s = ops.silu(bn)
        dbn = ops.silu_bwd(bn, ds)
        ddw = torch.empty_like(dbn)
        ops.chanaffine_bwd(dw, mean, var, gamma, dbn, ddw, grads["gamma"], grads["beta"], EPS, wgrad_beta=0.0)
        ops.dwconv1d_wgrad(gl, ddw, grads["w"], grads["cb"], beta=0.0)
        dgl = ops.dwconv1d_dgrad(ddw, w)
        return s, ops.glu_bwd(u, dgl)

    sf, duf = fused(); gf = {k: v.clone() for k, v in grads.items()}
    sc, duc = composed(); gc = {k: v.clone() for k, v in grads.items()}
    agree = {"s": (sf - sc).abs().max().item(), "du": (duf - duc).abs().max().item() / duc.abs().max().item(),
             "wgrads": max(((gf[k] - gc[k]).abs().max() / gc[k].abs().max()).item() for k in grads)}
    assert all(v < 1e-4 for v in agree.values()), agree
    with _Counted() as nf:
        fused()
    with _Counted() as nc:
        composed()
    (tf, tf_lo, tf_hi), (tc, tc_lo, tc_hi), (td, td_lo, td_hi) = _median_us([fused, composed, composed], reps=reps, warm=5)
    return {"shape": [B, T, C], "fused_us": round(tf, 1), "fused_us_min_max": [round(tf_lo, 1), round(tf_hi, 1)], "fused_abi_calls": nf.n,
            "composed_us": round(tc, 1), "composed_us_min_max": [round(tc_lo, 1), round(tc_hi, 1)],
            "composed_again_us": round(td, 1), "composed_again_us_min_max": [round(td_lo, 1), round(td_hi, 1)],
            "composed_abi_calls": nc.n, "composed_spread_us": round(abs(tc - td), 1),
            "time_ratio_fused_over_slower_composed": round(tf / max(tc, td), 3),
            "saved_activation_floats_fused_vs_composed": [3 * B * T * C, 4 * B * T * C],          # gl, c, s | gl, dw, bn, s  (u is kept by both)
            "max_disagreement": {k: float(f"{v:.2e}") for k, v in agree.items()}}


def time_loop(dev, seconds, passes=3):
    import argparse as ap
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    from dynamic_asr_eval_amd.run_wav2vec2 import init_synthetic
    model = ParakeetForCTC(None, device=dev)                                                     # the defaults are the 0.6b shape
    init_synthetic(model, seed=0)
    for n, b in model.buffers_.items():
        if n.endswith("running_var"):
            b.fill_(1.0)
    frames = int(seconds * 100)                                                                  # 10 ms hop
    spec = torch.randn(1, model.n_mels, frames, generator=torch.Generator().manual_seed(7))
    tok = N.SyntheticTokenizer(model.cfg["vocab_size"] - 1)
    args = ap.Namespace(epochs=1, shuffle=False, spec_augment_generator=torch.Generator().manual_seed(1))

    def run(sp):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = N.dynamic_eval(args, model, sp, 2048, 0, tok, use_tqdm=False, return_device=True)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    tail = frames % 2048
    run(spec[:, :, :2048 + tail] if tail else spec[:, :, :4096])                                 # warm-up: every window shape of the timed passes
    times = []
    for _ in range(passes):
        t, out = run(spec)
        assert torch.isfinite(out).all()
        times.append(t)
    n_params = sum(p.numel() for _, p in model.named_parameters())
    return {"shape": {"layers": 24, "hidden": 1024, "heads": 8, "ffn": 4096, "vocab": model.cfg["vocab_size"], "parameters_M": round(n_params / 1e6, 1)},
            "audio_seconds": seconds, "windows": -(-frames // 2048), "copies": 5,
            "pass_s": [round(t, 3) for t in times], "audio_s_per_s": round(seconds / sorted(times)[len(times) // 2], 1)}


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["convmod", "loop"])
    p.add_argument("--seconds", type=float, default=600.0)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_parakeet.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {}
    if "convmod" in a.what:
        res["convmod_core_fwd_bwd"] = [time_convmod(dev, 5, 256, 1024), time_convmod(dev, 5, 2048, 1024)]
    if "loop" in a.what:
        res["dynamic_eval"] = time_loop(dev, a.seconds)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
