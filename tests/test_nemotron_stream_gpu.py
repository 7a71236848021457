"""Streaming sessions of NemotronAsrStreamingForRNNT (nemotron_asr_streaming_stream.py) against transformers' encoder driven chunk by
chunk with its own caches on the CPU (tests/nemotron_stream_refs.hf_stream_encode, float64; its float32 run is the yardstick of
kernel_refs.measured_tol), on the toy model of tests/nemotron_refs.py with the same random state dict on both sides; the greedy decode
across chunks against transformers' OFFLINE generate on the whole prefix (its streaming generate is not a batch oracle: at B = 3 it
stops emitting once the first chunk's rows run out)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import nemotron_refs as NR  # noqa: E402
import nemotron_stream_refs as SR  # noqa: E402
import rnnt_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

ENC_FLOOR = 2e-4            # test_nemotron_streaming_gpu.py's bar for projected encoder states, times max(1, max |value|)
_CACHE = {}


def _model(sw=9, **arch):
    key = (sw, tuple(sorted(arch.items())))
    if key not in _CACHE:
        _CACHE[key] = NR.hf_model(seed=2, arch=dict(NR.TOY, sliding_window=sw, **arch))
    return _CACHE[key]


def _hip(cuda, ref_cfg):
    from dynamic_asr_eval_amd.nemotron_asr_streaming_model import NemotronAsrStreamingForRNNT
    hip = NemotronAsrStreamingForRNNT(ref_cfg[0], device=cuda)
    hip.load_state_dict(ref_cfg[1].state_dict())
    return hip


def _feats(B, sw, look, n_chunks, seed=1):
    _, _, first, per = SR.geometry(sw, look)
    return torch.randn(B, first + (n_chunks - 1) * per, NR.TOY["num_mel_bins"], generator=torch.Generator().manual_seed(seed))


def _oracle(sw, look, B, n_chunks, **arch):
    """(features, transformers' streamed projected states in float64, in float32): computed once on the CPU, shared, left alone."""
    key = ("enc", sw, look, B, n_chunks, tuple(sorted(arch.items())))
    if key not in _CACHE:
        ref = _model(sw, **arch)[1]
        x = _feats(B, sw, look, n_chunks)
        _CACHE[key] = (x, SR.hf_stream_encode(ref, x, look, torch.float64), SR.hf_stream_encode(ref, x, look, torch.float32))
    return _CACHE[key]


def _stream(session, x, sw, look, call="encode_chunk"):
    return [getattr(session, call)(ch.contiguous()) for ch in SR.chunks_of(x, sw, look)]


def _check(name, got, e32, e64):
    tol, err32 = K.measured_tol(e32.double(), e64, ENC_FLOOR * max(1.0, e64.abs().max().item()))
    err = K.max_err(got.double(), e64)
    print(f"{name}: kernel {err:.2e} | transformers fp32 streaming {err32:.2e} | bound {tol:.2e}")
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("sw,look,B,n_chunks", [(9, 2, 2, 12), (9, 0, 1, 20), (29, 13, 1, 8)])
def test_encode_chunk_matches_transformers_streaming_and_the_offline_encode(cuda, sw, look, B, n_chunks):
    """encode_chunk over the whole stream against transformers' chunk-by-chunk float64 result, and against this project's own offline
    encode() of the concatenated features, both under measured_tol with transformers' fp32 streaming as the yardstick and the 2e-4 *
    max(1, max |value|) floor of the offline model test.  (9, 2): the cache transformers keeps (8) is longer than the mask shows (6);
    (9, 0): one frame per chunk, 8 cached chunks, the conv state's shortfall branch; (29, 13): the released chunk size, two cached chunks,
    two time tiles in the conv core.
    Measured (MI355X), worst over the three cases: stream against transformers 3.3e-07 (transformers' fp32 streaming 3.2e-07, bound
    2.0e-04), own offline encode against transformers 3.2e-07, stream against own offline encode 2.4e-07."""
    x, e64, e32 = _oracle(sw, look, B, n_chunks)
    hip = _hip(cuda, _model(sw))
    s = hip.stream(B, look)
    cs = look + 1
    assert (s.first_chunk_frames, s.chunk_frames) == (1 + 8 * look, 8 * cs) and s.frames_seen == 0
    enc = torch.cat(_stream(s, x.to(cuda), sw, look), 1)
    assert enc.shape == e64.shape == (B, n_chunks * cs, 64) and s.frames_seen == n_chunks * cs
    _check("stream vs transformers", enc.cpu(), e32, e64)
    with torch.no_grad():
        off = hip.encode(x.to(cuda), num_lookahead_tokens=look)
    _check("offline vs transformers", off.cpu(), e32, e64)
    tol, _ = K.measured_tol(e32.double(), e64, ENC_FLOOR * max(1.0, e64.abs().max().item()))
    gap = (enc - off).abs().max().item()
    print(f"stream vs own offline encode: {gap:.2e} (bound {tol:.2e})")
    assert gap <= tol


def test_a_stream_is_not_bounded_by_max_position_embeddings(cuda):
    """30 chunks at (9, 2) are 90 encoder frames under max_position_embeddings = 32: the session runs (9 keys at most are in play) and
    matches transformers' streaming result; the offline encode of the same features still refuses."""
    from dynamic_asr_eval_amd import ops
    x, e64, e32 = _oracle(9, 2, 1, 30, max_position_embeddings=32)
    hip = _hip(cuda, _model(9, max_position_embeddings=32))
    enc = torch.cat(_stream(hip.stream(1, 2), x.to(cuda), 9, 2), 1)
    assert enc.shape[1] == 90
    _check("stream vs transformers", enc.cpu(), e32, e64)
    with pytest.raises(ops.DynError, match="max_position_embeddings"):
        hip.encode(x.to(cuda), num_lookahead_tokens=2)


@pytest.mark.parametrize("nB", [1, 3])
def test_push_decodes_across_chunks_as_transformers_decodes_the_whole_prefix(cuda, nB):
    """nemotron_refs' decode model on the first 281 feature frames (17 + 11 * 24: 12 chunks, 36 encoder frames at lookahead 2).  The
    oracle is transformers' OFFLINE generate on that prefix (rnnt_refs.hf_greedy), whose output alone satisfies
    rnnt_refs.assert_decode_conditions; emissions and forced advances fall on the last frame of a chunk, where the carried decoder state
    matters.  push() over the 12 chunks gives the same tokens, absolute frames and counts per row; generate_streaming() gives what this
    project's own generate() gives."""
    ref_cfg = NR.decode_model()
    x = NR.decode_feats(nB)[:, :281].contiguous()
    rows, Tp = R.hf_greedy(ref_cfg[1], x)
    margin = R.hf_margins(ref_cfg[1], x, rows)
    assert Tp == 36 and margin > 1e-3, (Tp, margin)
    R.assert_decode_conditions(rows, margin, ref_cfg[0].max_symbols_per_step)
    last = [s for r in rows for s in r["steps"] if s[2] % 3 == 2 and s[0] != NR.BLANK]
    assert last, "no emission on the last frame of a chunk"
    hip = _hip(cuda, ref_cfg)
    s = hip.stream(nB, 2)
    outs = _stream(s, x.to(cuda), 9, 2, "push")
    assert len(outs) == 12 and all(o.tokens.shape == (nB, 9) and o.enc.shape == (nB, 3, 64) for o in outs)
    for b, row in enumerate(rows):
        toks = [t for o in outs for t in o.tokens[b, :int(o.count[b])].tolist()]
        frs = [t for o in outs for t in o.frames[b, :int(o.count[b])].tolist()]
        assert toks == row["tokens"] and frs == row["frames"], b
        assert sum(int(o.steps[b]) for o in outs) == len(row["steps"]), b
    own = hip.generate(x.to(cuda), num_lookahead_tokens=2)
    got = hip.generate_streaming(x.to(cuda), num_lookahead_tokens=2)
    assert torch.equal(got.count, own.count) and torch.equal(got.steps, own.steps)
    for b in range(nB):
        n = int(own.count[b])
        assert n == len(rows[b]["tokens"])
        assert torch.equal(got.tokens[b, :n], own.tokens[b, :n]) and torch.equal(got.frames[b, :n], own.frames[b, :n]), b
    chunks = [ch.to(cuda).contiguous() for ch in SR.chunks_of(x, 9, 2)]
    again = hip.generate_streaming(iter(chunks), num_lookahead_tokens=2)
    assert torch.equal(again.tokens, got.tokens) and torch.equal(again.frames, got.frames)


def test_graph_replay_is_bit_equal_to_eager(cuda):
    """graph=True (the steady-state step captured at the third chunk, replayed from then on) against graph=False on the same inputs at
    (9, 2), 6 chunks, B = 2; a second graphed session opened after the first was dropped gives the same bits again."""
    x = _feats(2, 9, 2, 6, seed=3).to(cuda)
    hip = _hip(cuda, _model(9))
    eager = torch.cat(_stream(hip.stream(2, 2), x, 9, 2), 1)
    s = hip.stream(2, 2, graph=True)
    graphed = torch.cat(_stream(s, x, 9, 2), 1)
    assert s._graph is not None and torch.equal(graphed, eager)
    s.close()
    del s
    s2 = hip.stream(2, 2, graph=True)
    assert torch.equal(torch.cat(_stream(s2, x, 9, 2), 1), eager)
    s2.close()


def test_reset_restarts_the_stream(cuda):
    x = _feats(2, 9, 2, 5, seed=4).to(cuda)
    hip = _hip(cuda, NR.decode_model())
    s = hip.stream(2, 2)
    first = _stream(s, x, 9, 2, "push")
    s.reset()
    assert s.frames_seen == 0
    second = _stream(s, x, 9, 2, "push")
    for a, b in zip(first, second):
        assert torch.equal(a.enc, b.enc) and torch.equal(a.tokens, b.tokens) and torch.equal(a.frames, b.frames) and torch.equal(a.count, b.count)


def test_a_bad_chunk_is_refused_and_the_session_stays_usable(cuda):
    from dynamic_asr_eval_amd import ops
    x = _feats(1, 9, 2, 3, seed=5).to(cuda)
    hip = _hip(cuda, _model(9))
    want = torch.cat(_stream(hip.stream(1, 2), x, 9, 2), 1)
    s = hip.stream(1, 2)
    chunks = [c.contiguous() for c in SR.chunks_of(x, 9, 2)]
    with pytest.raises(ops.DynError, match="17.*24.*pad"):
        s.encode_chunk(chunks[1])                                  # 24 frames where the first chunk's 17 are due
    got = [s.encode_chunk(chunks[0])]
    with pytest.raises(ops.DynError, match="17.*24.*pad"):
        s.encode_chunk(chunks[0])                                  # and the other way round
    with pytest.raises(ops.DynError, match="join or leave"):
        s.encode_chunk(torch.cat([chunks[1], chunks[1]]))
    with pytest.raises(ops.DynError, match="attention_mask"):
        s.push(chunks[1], attention_mask=torch.ones(1, 24))
    assert s.frames_seen == 3 and int(s.counter.item()) == 1
    got += [s.encode_chunk(c) for c in chunks[1:]]
    assert torch.equal(torch.cat(got, 1), want)
    with pytest.raises(ops.DynError, match="streaming"):
        hip.backward()
