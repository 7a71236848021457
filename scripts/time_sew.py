"""Timings of SEW on the MI355X, one JSON line:
  squeeze  the passes between the strided positional conv's grouped GEMM and the first encoder layer, forward + backward, at
           [B, T, H] = [4, 1499, 512], s = 2, G = 16 (K = 128 only sets the GEMM, which both forms share and neither times): FUSED =
           dyn_squeeze_ln_fwd + dyn_squeeze_ln_bwd, next to the COMPOSITION they replace, from the ops that existed before: group_unpack,
           gelu, torch's avg_pool1d, axpby, layernorm; layernorm_bwd, gelu_bwd, colsum, group_pack_grad and the pool's backward in torch.
           One process, alternating, HIP events, median of 25 after a warm-up, eager launches.  The composition is timed TWICE in the same
           alternation (two entries): the difference of their medians is the run-to-run spread the fused form is held against.  The two
           forms are checked against each other before they are timed.
  loop     wav2vec2_lib.dynamic_eval_su with seeded weights at SEW's 512-wide, 12-layer shape (8 x 64 heads, FFN 2048, SEWConfig()'s
           13-layer extractor, squeeze_factor 2) beside Wav2Vec2ForCTC at its base architecture in the same run, same synthetic talk, eager
           and with bucket graphs, audio-s/s (time_data2vec_audio.py's loop).
Usage: python scripts/time_sew.py [squeeze] [loop] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _Counted, _median_us, time_loop  # noqa: E402

EPS = 1e-5


def time_squeeze(dev, B=4, T=1499, H=512, G=16, s=2):
    from dynamic_asr_eval_amd import ops
    T2, cg = T // s, H // G
    g = torch.Generator().manual_seed(T)
    h = torch.randn(B, T, H, generator=g).to(dev)
    yg = torch.randn(B, G, T2, cg, generator=g).to(dev)
    bias, gamma, beta = (torch.randn(H, generator=g).to(dev) for _ in range(3))
    dz = (torch.randn(B, T2, H, generator=g) / T2).to(dev)
    grads = [torch.zeros(H, device=dev) for _ in range(3)]

    def fused():
        z, mean, rstd = ops.squeeze_ln(h, yg, bias, gamma, beta, s, EPS)
        dh, dyg = ops.squeeze_ln_bwd(h, yg, bias, gamma, mean, rstd, dz, s, *grads, wgrad_beta=0.0)
        return z, dh, dyg

    def composed():
        pre = ops.group_unpack(yg, bias, T2, H)
        pos = ops.gelu(pre)
        hs = F.avg_pool1d(h.transpose(1, 2), s, s).transpose(1, 2)[:, :T2].contiguous()
        ops.axpby(pos, hs, 1.0, 1.0)
        z, mean, rstd = ops.layernorm(hs, gamma, beta, EPS)
        dhs = torch.empty_like(hs)
        ops.layernorm_bwd(hs, gamma, mean, rstd, dz, dhs, grads[0], grads[1], dx_beta=0.0, wgrad_beta=0.0)
        dpre = ops.gelu_bwd(pre, dhs)
        ops.colsum(dpre, grads[2], beta=0.0)
        dyg = ops.group_pack_grad(dpre, G, T2)
        dh = torch.zeros(B, T, H, device=dev)                       # the pool's backward: every frame of a window gets dhs / s
        dh[:, :s * T2].view(B, T2, s, H).copy_((dhs / s).unsqueeze(2).expand(-1, -1, s, -1))
        return z, dh, dyg

    zf, dhf, dyf = fused(); gf = [t.clone() for t in grads]
    zc, dhc, dyc = composed(); gc = [t.clone() for t in grads]
    agree = {"z": (zf - zc).abs().max().item(), "dh": (dhf - dhc).abs().max().item() / dhc.abs().max().item(),
             "dyg": (dyf - dyc).abs().max().item() / dyc.abs().max().item(),
             "wgrads": max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gf, gc))}
    assert all(v < 1e-4 for v in agree.values()), agree
    with _Counted() as nf:
        fused()
    with _Counted() as nc:
        composed()
    (tf, tf_lo, tf_hi), (tc, tc_lo, tc_hi), (td, td_lo, td_hi) = _median_us([fused, composed, composed], reps=25, warm=5)
    return {"shape": [B, T, H], "squeeze_factor": s, "groups": G, "fused_us": round(tf, 1), "fused_us_min_max": [round(tf_lo, 1), round(tf_hi, 1)],
            "fused_abi_calls": nf.n, "composed_us": round(tc, 1), "composed_us_min_max": [round(tc_lo, 1), round(tc_hi, 1)],
            "composed_again_us": round(td, 1), "composed_again_us_min_max": [round(td_lo, 1), round(td_hi, 1)],
            "composed_abi_calls_without_torch": nc.n, "composed_spread_us": round(abs(tc - td), 1),
            "time_ratio_fused_over_composed": round(tf / min(tc, td), 3), "max_disagreement": {k: float(f"{v:.2e}") for k, v in agree.items()}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["squeeze", "loop"])
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    if "squeeze" in a.what:
        res["squeeze_stage_fwd_bwd"] = time_squeeze(dev)
    if "loop" in a.what:
        from dynamic_asr_eval_amd.sew_model import SEWForCTC
        from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
        sew = SEWForCTC(dict(hidden_size=512, num_attention_heads=8, intermediate_size=2048), device=dev)
        res["dynamic_eval_su"] = {"sew_512x12": time_loop(dev, sew, a.seconds), "wav2vec2_base": time_loop(dev, Wav2Vec2ForCTC(None, device=dev), a.seconds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
