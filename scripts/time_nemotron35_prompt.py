"""Timing of Nemotron3_5AsrForRNNT's prompt projector on the MI355X, one JSON line.  Released sizes: H = 1024, I = 2048,
Np = 128.  Two forms of the block between the encoder's last hidden states and `encoder_projector`, forward and forward + backward:
  fused    what the model runs: K = H product, ops.prompt_bias_gather, ops.prompt_relu in place, linear_2; backward by linear_2's
           products, ops.prompt_relu_bwd (dz, db1, dW1p in one pass + finalise), the hidden block's weight and data gradients.
           `fused_fwd_session` is the forward of a streaming step: pb was gathered when the session was opened.
  concat   the yardstick, transformers' form composed from the ops that existed before: a materialised [B, T', H + Np] one-hot concat,
           K = H + Np products each way, ops.relu / relu_bwd, ops.colsum, a [I, H + Np] weight gradient.
Shapes: T' = 256 at B = 4 (an offline window of the loop) and a 14-frame streaming chunk at B = 1 and 8.  The two forms alternate inside
every repetition; a repetition is `--iters` calls between two device events; reported: the median over `--reps` repetitions with min and
max (the spread).  Both forms' results are compared first.
`--stream` adds the streaming step: encode_chunk per chunk (eager and graph=True) of this model against its parent
NemotronAsrStreamingForRNNT at the released configuration, lookahead 13, alternating the two models' sessions.
A record, not a gate.  Usage: python scripts/time_nemotron35_prompt.py [--reps 9] [--iters 50] [--stream] [--layers 24] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

H, I, NP = 1024, 2048, 128
SHAPES = ((4, 256), (1, 14), (8, 14))


def _events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _ab(fns, reps, iters):
    """{name: [median, min, max] ms per call}: the forms alternate inside every repetition, after one warm-up round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_events_ms(fn, iters))
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}


def block_case(dev, B, T, reps, iters):
    from dynamic_asr_eval_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)                                         # noqa: E731
    x, w1, b1, w2, b2, df = r(B, T, H), r(I, H + NP, k=0.03), r(I, k=0.1), r(H, I, k=0.03), r(H, k=0.1), r(B, T, H)
    w1h, w1p = w1[:, :H].contiguous(), w1[:, H:].contiguous()
    ids_host = [(7 * b + 3) % NP for b in range(B)]
    ids = torch.tensor(ids_host, dtype=torch.int32, device=dev)
    one_hot = torch.nn.functional.one_hot(torch.tensor(ids_host), NP).float().to(dev)[:, None, :].expand(B, T, NP)
    G = {k: torch.zeros_like(v) for k, v in dict(w1=w1, w1h=w1h, w1p=w1p, b1=b1, w2=w2, b2=b2).items()}
    M = B * T

    def fused_fwd():
        z = ops.linear(x, w1h)
        a = ops.prompt_relu(z, ops.prompt_bias_gather(b1, w1p, ids), out=z)
        return a, ops.linear(a, w2, b2)

    pb_session = ops.prompt_bias_gather(b1, w1p, ids)

    def fused_fwd_session():                                   # a streaming step: pb was gathered when the session was opened
        z = ops.linear(x, w1h)
        return ops.linear(ops.prompt_relu(z, pb_session, out=z), w2, b2)

    def fused_both():
        a, f = fused_fwd()
        da = ops.linear_dgrad(df, w2)
        ops.linear_wgrad(df.view(M, H), a.view(M, I), G["w2"], beta=0.0)
        ops.colsum(df, G["b2"], beta=0.0)
        dz = ops.prompt_relu_bwd(a, da, ids, G["b1"], G["w1p"], beta=0.0, out=da)
        ops.linear_wgrad(dz.view(M, I), x.view(M, H), G["w1h"], beta=0.0)
        return f, ops.linear_dgrad(dz, w1h)

    def concat_fwd():
        xc = torch.cat([x, one_hot], -1)                       # the copy transformers makes
        a = ops.relu(ops.linear(xc, w1, b1))
        return xc, a, ops.linear(a, w2, b2)

    def concat_both():
        xc, a, f = concat_fwd()
        da = ops.linear_dgrad(df, w2)
        ops.linear_wgrad(df.view(M, H), a.view(M, I), G["w2"], beta=0.0)
        ops.colsum(df, G["b2"], beta=0.0)
        dz = ops.relu_bwd(a, da, out=da)
        ops.linear_wgrad(dz.view(M, I), xc.view(M, H + NP), G["w1"], beta=0.0)
        ops.colsum(dz, G["b1"], beta=0.0)
        return f, ops.linear_dgrad(dz, w1)[..., :H]

    with torch.no_grad():
        f1, dx1 = fused_both()
        gw = torch.cat([G["w1h"], G["w1p"]], 1).clone()
        gb = G["b1"].clone()
        f2, dx2 = concat_both()
        agree = {"fused_states": (f1 - f2).abs().max().item(), "dx": (dx1 - dx2).abs().max().item(), "dW1": (gw - G["w1"]).abs().max().item(),
                 "db1": (gb - G["b1"]).abs().max().item(), "max_abs_states": f2.abs().max().item(), "max_abs_dW1": G["w1"].abs().max().item()}
        times = _ab({"fused_fwd": fused_fwd, "fused_fwd_session": fused_fwd_session, "concat_fwd": concat_fwd, "fused_fwd_bwd": fused_both, "concat_fwd_bwd": concat_both}, reps, iters)
    # bytes the two ReLU / bias passes move, from the shapes (the GEMMs' operands aside): fused reads z and writes a once each way;
    # concat also writes and reads the [M, H + Np] copy and sums dz in a pass of its own
    traffic = {"fused_elementwise_bytes": 4 * M * I * (2 + 3), "concat_elementwise_bytes": 4 * (M * I * (2 + 3 + 1) + M * (H + NP) * 2 + M * H)}
    return {"B": B, "T": T, "ms_median_min_max": times, "largest_difference_between_the_forms": {k: float(f"{v:.3e}") for k, v in agree.items()}, **traffic}


def _init(m, dev):
    g = torch.Generator().manual_seed(0)
    for n, _ in m.spec:
        p = m.P[n]
        p.copy_((torch.randn(p.shape, generator=g) * (0.02 if p.dim() > 1 else 0.1)).to(dev))
        if n.endswith(m._norm_weight_suffixes):
            p.add_(1.0)
    return m


def stream_models(dev, layers):
    from dynamic_asr_eval_amd.nemotron3_5_asr_model import Nemotron3_5AsrForRNNT
    from dynamic_asr_eval_amd.nemotron_asr_streaming_model import NemotronAsrStreamingForRNNT
    over = {"encoder_config": {"num_hidden_layers": layers}}
    return {"parent": _init(NemotronAsrStreamingForRNNT(over, device=dev), dev), "nemotron3_5": _init(Nemotron3_5AsrForRNNT(over, device=dev), dev)}


def stream_case(dev, models, layers, B, look, n_chunks, reps):
    from dynamic_asr_eval_amd import nemotron_asr_streaming_stream as NS
    sessions = {f"{k}_{mode}": m.stream(B, look, graph=(mode == "graph")) for k, m in models.items() for mode in ("eager", "graph")}
    any_s = next(iter(sessions.values()))
    T = any_s.first_chunk_frames + (n_chunks - 1) * any_s.chunk_frames
    x = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(B + look)).to(dev)
    chunks = [ch.contiguous() for ch in NS.split_chunks(any_s, x)]

    def run(s):
        s.reset()
        for ch in chunks:
            s.encode_chunk(ch)

    for s in sessions.values():
        run(s)
    torch.cuda.synchronize(dev)
    ts = {k: [] for k in sessions}
    for _ in range(reps):
        for k, s in sessions.items():                         # the four sessions alternate inside every repetition
            t0 = time.perf_counter()
            run(s)
            torch.cuda.synchronize(dev)
            ts[k].append((time.perf_counter() - t0) * 1e3 / n_chunks)
    out = {"B": B, "lookahead": look, "chunks": n_chunks, "layers": layers,
           "encode_chunk_ms_median_min_max": {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()},
           "state_bytes": {k: s.state_bytes() for k, s in sessions.items() if k.endswith("eager")}}
    for s in sessions.values():
        s.close()
    return out


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--stream", action="store_true")
    p.add_argument("--layers", type=int, default=24)
    p.add_argument("--chunks", type=int, default=40)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nemotron35_prompt.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {"hidden_size": H, "prompt_intermediate_size": I, "num_prompts": NP, "reps": a.reps, "iters": a.iters,
           "block": [block_case(dev, B, T, a.reps, a.iters) for B, T in SHAPES]}
    if a.stream:
        models = stream_models(dev, a.layers)
        res["stream"] = [stream_case(dev, models, a.layers, B, 13, a.chunks, max(3, a.reps // 2)) for B in (1, 8)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
