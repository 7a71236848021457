"""Timing of NemotronAsrStreamingForRNNT's streaming sessions on the MI355X, one JSON line.  The released configuration
(24 layers, H = 1024, 8 heads, sliding_window 71; seeded random weights), lookahead 13 (chunks of 14 encoder frames = 1.12 s of audio,
5 cached chunks) and 0 (one frame = 80 ms per chunk, 70 cached chunks), B in {1, 8, 32}, a stream of 60 chunks.  Per case:
  encode_chunk   ms per chunk, eager and graph=True: a host clock around the 60 chunks of a warmed session, ended by a device
                 synchronise; the median of `--reps` passes with their min and max (the spread).  The graph pass includes the copy into
                 the static chunk and the copy of the result out of the captured step's buffer.
  push           ms per chunk with the greedy decode (eager encoder), and the tokens the random head emitted per chunk and row.
  launches       C-ABI calls of one steady-state chunk (one kernel launch each; a GEMM whose plan splits K launches its combine too).
  throughput     audio-seconds per second of the whole stream: generate_streaming-style push over the 60 chunks, next to the only thing
                 the offline path offers for the same audio, generate() of the concatenated features.
  latency        what a streaming user pays per chunk without a session: the offline encode() of the whole prefix at chunks 10, 30, 60.
Eager launches are host-bound here, so the host clock is the right clock; nothing is profiled.  A record, not a gate.
Usage: python scripts/time_nemotron_stream_chunks.py [--batches 1,8,32] [--lookaheads 13,0] [--chunks 60] [--reps 5] [--layers 24] [--out FILE]"""
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

from time_nemotron_streaming import _model  # noqa: E402

FRAME_S = 0.08                                   # one encoder frame: 8 feature frames of 10 ms


def _wall_ms(fn, reps, dev):
    """(median, min, max) ms of fn() ended by a device synchronise, after one warm-up pass."""
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


class _Counting:
    """The library with every dyn_* call counted."""

    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("dyn_") or name in ("dyn_last_error",):
            return f

        def counted(*a):
            self.n += 1
            return f(*a)
        return counted


def _launches(session, chunks):
    from dynamic_asr_eval_amd import ops
    session.reset()
    for ch in chunks[:2]:
        session.encode_chunk(ch)
    real = ops._L
    lib = _Counting(real())
    ops._L = lambda: lib
    try:
        session.encode_chunk(chunks[2])
    finally:
        ops._L = real
    return lib.n


def time_case(dev, m, B, look, n_chunks, reps):
    from dynamic_asr_eval_amd import nemotron_asr_streaming_stream as NS
    c = m.cfg
    eager, graphed = m.stream(B, look), m.stream(B, look, graph=True)
    geo = eager.geo
    T = eager.first_chunk_frames + (n_chunks - 1) * eager.chunk_frames
    x = torch.randn(B, T, c["num_mel_bins"], generator=torch.Generator().manual_seed(B + look)).to(dev)
    chunks = [ch.contiguous() for ch in NS.split_chunks(eager, x)]
    audio_s = n_chunks * geo.cs * FRAME_S

    def run(session, call):
        def go():
            session.reset()
            for ch in chunks:
                getattr(session, call)(ch)
        return go

    res = {"batch": B, "lookahead": look, "chunk_encoder_frames": geo.cs, "cached_chunks": geo.lc, "chunks": n_chunks,
           "audio_s_per_row": round(audio_s, 2), "state_bytes": eager.state_bytes(), "launches_per_chunk": _launches(eager, chunks)}
    outs = []
    for session in (eager, graphed):
        session.reset()
        outs.append(torch.cat([session.encode_chunk(ch) for ch in chunks], 1))
    res["graph_bit_equal_to_eager"] = bool(torch.equal(*outs))
    for name, session, call in (("encode_chunk_eager", eager, "encode_chunk"), ("encode_chunk_graph", graphed, "encode_chunk"),
                                ("push_eager", eager, "push")):
        med, lo, hi = _wall_ms(run(session, call), reps, dev)
        res[name + "_ms_per_chunk"] = round(med / n_chunks, 4)
        res[name + "_ms_per_chunk_min_max"] = [round(lo / n_chunks, 4), round(hi / n_chunks, 4)]
        if call == "push":
            res["stream_audio_s_per_s"] = round(B * audio_s / (med / 1e3), 1)
    eager.reset()
    res["tokens_per_chunk_and_row"] = round(sum(float(eager.push(ch).count.float().mean()) for ch in chunks) / n_chunks, 2)
    med, lo, hi = _wall_ms(lambda: m.generate(x, num_lookahead_tokens=look), max(3, reps // 2), dev)
    res["offline_generate_ms"] = round(med, 2)
    res["offline_generate_ms_min_max"] = [round(lo, 2), round(hi, 2)]
    res["offline_audio_s_per_s"] = round(B * audio_s / (med / 1e3), 1)
    res["reencode_prefix_ms"] = {}
    for k in sorted({min(10, n_chunks), min(30, n_chunks), n_chunks}):
        prefix = x[:, :eager.first_chunk_frames + (k - 1) * eager.chunk_frames].contiguous()

        def enc():
            with torch.no_grad():
                m.encode(prefix, num_lookahead_tokens=look)
        med, lo, hi = _wall_ms(enc, max(3, reps // 2), dev)
        res["reencode_prefix_ms"][str(k)] = [round(med, 3), round(lo, 3), round(hi, 3)]
    graphed.close()
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="1,8,32")
    p.add_argument("--lookaheads", default="13,0")
    p.add_argument("--chunks", type=int, default=60)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--layers", type=int, default=24)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nemotron_stream_chunks.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    model = _model(dev, a.layers)
    cases = [time_case(dev, model, B, look, a.chunks, a.reps) for look in map(int, a.lookaheads.split(",")) for B in map(int, a.batches.split(","))]
    line = json.dumps({"layers": a.layers, "hidden_size": model.cfg["hidden_size"], "sliding_window": model.cfg["sliding_window"], "cases": cases})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
