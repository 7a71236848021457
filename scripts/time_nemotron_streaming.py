"""Timing of NemotronAsrStreamingForRNNT's chunked-context attention on the MI355X, one JSON line.  One encoder layer's attention,
forward + backward, at T' = 256 and H = 1024 (8 heads) under sliding_window 71 and lookahead 13, twice from the same input and weights:
the BAND path the model runs (position product over the W = 97 rows any query can reach, ops.softmax_relshift_band, ops.relshift_band_bwd,
K = W and M = W gradient products) and the DENSE yardstick built here from existing ops (Wav2Vec2ConformerForCTC's attention: the full
[T', 2T' - 1] = 511-column position product, an additive -inf mask added to the scores by ops.axpby, ops.softmax_relshift,
ops.relshift_bwd).  One process, alternating, HIP events, median of 25 after a warm-up, eager launches, weight gradients launched at once;
the dense form is timed TWICE in the same alternation: the difference of its medians is the run-to-run spread.  Then one whole model
step (forward with labels + backward) at the released size.  A record, not a gate.
Usage: python scripts/time_nemotron_streaming.py [--batch B] [--layers L] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _median_us  # noqa: E402

T_FEATS, T_ENC, LOOK = 2040, 256, 13               # 2040 -> 1021 -> 511 -> 256 frames


def _model(dev, layers):
    from dynamic_asr_eval_amd.nemotron_asr_streaming_model import NemotronAsrStreamingForRNNT
    m = NemotronAsrStreamingForRNNT({"encoder_config": {"num_hidden_layers": layers}}, device=dev)       # every other key: the released defaults
    g = torch.Generator().manual_seed(0)
    for n, _ in m.spec:
        p = m.P[n]
        p.copy_((torch.randn(p.shape, generator=g) * (0.02 if p.dim() > 1 else 0.1)).to(dev))
        if n.endswith(m._norm_weight_suffixes):
            p.add_(1.0)
    return m


def time_attention(dev, B, reps=25):
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd import wav2vec2_conformer_model as WC
    m = _model(dev, 1)
    c = m.cfg
    H, nh, T = c["hidden_size"], c["num_attention_heads"], T_ENC
    band = m._band(T, LOOK)
    m._lookahead = m._ctx_lookahead = LOOK
    tab = m.position_table(T)
    g = torch.Generator().manual_seed(1)
    x, dr = (torch.randn(B, T, H, generator=g).to(dev) for _ in range(2))
    d = torch.arange(T)[:, None] // band.cs - torch.arange(T)[None, :] // band.cs
    add = torch.zeros(T, T).masked_fill(~((d >= 0) & (d <= band.lc)), float("-inf")).expand(B, nh, T, T).contiguous().to(dev)
    plain = ops.softmax_relshift

    def masked(S, BD, out=None, valid=None, ld_bd=None):
        ops.axpby(add, S, 1.0, 1.0)
        return plain(S, BD, out=out, valid=valid, ld_bd=ld_bd)

    def banded():
        with ops.use_workspace(m._scratch()):
            r, kept = m._attn_fwd(x, 0, None, tab, True)
            return r, m._attn_bwd(dr, kept[:9], kept[9], 0, B, T, tab)

    def dense():
        ops.softmax_relshift = masked
        try:
            with ops.use_workspace(m._scratch()):
                r, kept = WC.Wav2Vec2ConformerForCTC._attn_fwd(m, x, 0, None, tab, True)
                return r, WC.Wav2Vec2ConformerForCTC._attn_bwd(m, dr, kept[:9], kept[9], 0, B, T, tab)
        finally:
            ops.softmax_relshift = plain

    m.zero_grad()
    (rb, dxb), gb = banded(), m.flat_grads.clone()
    m.zero_grad()
    (rd, dxd), gd = dense(), m.flat_grads.clone()
    diffs = [(a - b).abs().max().item() for a, b in ((rb, rd), (dxb, dxd), (gb, gd))]
    (tb, tb_lo, tb_hi), (td, td_lo, td_hi), (tu, tu_lo, tu_hi) = _median_us([banded, dense, dense], reps=reps, warm=5)
    return {"shape": [B, T, H], "heads": nh, "sliding_window": c["sliding_window"], "lookahead": LOOK, "band_columns": band.W,
            "dense_columns": 2 * T - 1, "band_us": round(tb, 1), "band_us_min_max": [round(tb_lo, 1), round(tb_hi, 1)],
            "dense_us": round(td, 1), "dense_us_min_max": [round(td_lo, 1), round(td_hi, 1)], "dense_again_us": round(tu, 1),
            "dense_spread_us": round(abs(td - tu), 1), "time_ratio_band_over_faster_dense": round(tb / min(td, tu), 3),
            "max_abs_diff_out_dx_grads": diffs}


def time_step(dev, B, layers, U=20, reps=10):
    m = _model(dev, layers)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T_FEATS, m.cfg["num_mel_bins"], generator=g).to(dev)
    lab = torch.randint(0, m.blank, (1, U), generator=g)
    ids = torch.cat([torch.full((1, 1), m.blank), lab], 1)

    def step():
        with torch.enable_grad():
            out = m(input_features=x, decoder_input_ids=ids, labels=lab, num_lookahead_tokens=LOOK)
        m.zero_grad()
        m.backward()
        return out

    loss = step().loss.item()
    assert loss == loss and abs(loss) != float("inf"), loss
    (ts, lo, hi), = _median_us([step], reps=reps, warm=3)
    return {"shape": [B, T_FEATS, m.cfg["num_mel_bins"]], "encoder_frames": m.frames(T_FEATS), "layers": layers, "labels": U,
            "step_ms": round(ts / 1e3, 2), "step_ms_min_max": [round(lo / 1e3, 2), round(hi / 1e3, 2)]}


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=3)
    p.add_argument("--layers", type=int, default=24)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nemotron_streaming.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {"attention_fwd_bwd_band_vs_dense": time_attention(dev, a.batch), "model_step": time_step(dev, a.batch, a.layers)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
