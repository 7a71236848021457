"""Nemotron3_5AsrForRNNT (nemotron3_5_asr_model.py) against transformers' Nemotron3_5AsrForRNNT on the CPU with the same random state dict,
on the pattern and with the tolerances of tests/test_nemotron_streaming_gpu.py and tests/test_nemotron_stream_gpu.py (the model differs
from its parent only in the prompt projector): logits, loss and every gradient with a language per row, the language told apart rather
than tolerated, the state dict, the greedy decode, streaming sessions with and without a captured step and a change of language under
one, the dynamic-evaluation loop pointed at a language through `default_prompt_id`, and the refusals on the device path."""
import argparse
import copy
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import nemotron35_refs as PR  # noqa: E402
import nemotron_refs as NR  # noqa: E402
import nemotron_stream_refs as SR  # noqa: E402
import rnnt_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, U, H = 3, 4, 256
A, B2 = PR.PROMPTS_A, PR.PROMPTS_B
W1 = "prompt_projector.linear_1.weight"
ENC_FLOOR = 2e-4
_ORACLE = {}


def _pair(cuda, ref_cfg=None, **kw):
    from dynamic_asr_eval_amd.nemotron3_5_asr_model import Nemotron3_5AsrForRNNT
    cfg, ref = PR.hf_model(**kw) if ref_cfg is None else ref_cfg
    hip = Nemotron3_5AsrForRNNT(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _model():
    if "model" not in _ORACLE:
        _ORACLE["model"] = PR.hf_model(**PR.MODEL)
    return _ORACLE["model"]


def _decode_model():
    if "decode" not in _ORACLE:
        _ORACLE["decode"] = PR.decode_model()
    return _ORACLE["decode"]


def _feats(T):
    return torch.randn(B, T, 80, generator=torch.Generator().manual_seed(1))


def _oracle(T, look):
    """transformers' model at B = 3 under the languages A = [1, 5, 1] on T feature frames: the logits, a fixed random scalar of them and
    every parameter's gradient of it, the torch-recursion loss ("mean_volume", U = 4, all labels non-blank) and every parameter's gradient
    of the loss.  The ReLU masks of the prompt projector are at least 1e-4 from a flip.  Computed once on the CPU, shared, left alone."""
    key = (T, look)
    if key not in _ORACLE:
        cfg, ref = _model()
        x = _feats(T)
        assert PR.min_pre_relu(ref, x, A, look) > PR.MIN_PRE_RELU
        lab = torch.randint(3, NR.VOCAB - 1, (B, U), generator=torch.Generator().manual_seed(5))
        dec_in = torch.cat([torch.full((B, 1), NR.BLANK), lab], 1)
        out = ref(input_features=x, decoder_input_ids=dec_in, num_lookahead_tokens=look, prompt_ids=torch.tensor(A))
        Tp = out.logits.shape[1]
        gl = torch.randn(out.logits.shape, generator=torch.Generator().manual_seed(3))
        ref.zero_grad()
        (out.logits * gl).sum().backward(retain_graph=True)
        g_logits = {n: p.grad.clone() for n, p in ref.named_parameters()}
        loss = R.rnnt_loss_torch(out.logits, lab.tolist(), [Tp] * B, [U] * B, NR.BLANK, "mean_volume")
        ref.zero_grad()
        loss.backward()
        _ORACLE[key] = dict(x=x, lab=lab, dec_in=dec_in, Tp=Tp, gl=gl, logits=out.logits.detach(), enc=out.pooler_output.detach(),
                            g_logits=g_logits, loss=loss.item(), g_loss={n: p.grad.clone() for n, p in ref.named_parameters()})
        ref.zero_grad()
    return _ORACLE[key]


def _assert_grads(hip, want):
    grads = hip.grads_hf()
    assert set(grads) == set(want)
    worst = 0.0
    for n, w in want.items():
        assert grads[n].shape == w.shape, n
        diff, scale = (grads[n].cpu() - w).abs().max().item(), w.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
        assert scale > 0.0, n
    unused = [p for p in range(PR.NUM_PROMPTS) if p not in A]
    assert grads[W1][:, H:][:, unused].abs().max().item() == 0.0, "prompts no row used: exactly zero gradient columns"
    assert want[W1][:, H:][:, unused].abs().max().item() == 0.0
    return worst


@pytest.mark.parametrize("T,look", [(131, 2), (131, 0), (259, 2), (259, 0)])
def test_logits_loss_and_every_gradient_match_transformers(cuda, T, look):
    """The toy model of tests/nemotron_refs.py with num_prompts 8, prompt_intermediate_size 96 and the prompt columns of linear_1 times
    10, B = 3 under the languages [1, 5, 1], T' = 18 and 34, lookahead 2 and 0.  The bars of tests/test_nemotron_streaming_gpu.py: projected
    states and joint logits within 2e-4 * max(1, max |value|), the loss within 2e-4 relative, every parameter's gradient, of a random
    scalar of the logits and of the loss, within 3e-3 of its largest entry + 2e-8; the gradient columns of the six unused prompts are exactly
    zero on both sides; a second backward gives equal bits.
    Measured (MI355X), worst over the four cases: enc within 6.3e-08 (max 0.30), logits within 1.5e-08 (max |logit| 0.19), loss relative
    error 1.1e-07, worst relative gradient error 2.6e-06 for the loss and 7.0e-04 for the scalar of the logits."""
    o = _oracle(T, look)
    ref, hip = _pair(cuda, ref_cfg=_model())
    assert set(hip.grads_hf()) == {n for n, _ in ref.named_parameters()}
    kw = dict(input_features=o["x"].to(cuda), decoder_input_ids=o["dec_in"], num_lookahead_tokens=look, prompt_ids=A)
    with torch.enable_grad():
        out = hip(**kw)
    assert out.logits.shape == o["logits"].shape == (B, o["Tp"], U + 1, NR.VOCAB) and out.frames == o["Tp"] == {131: 18, 259: 34}[T]
    eerr, etop = (out.enc.cpu() - o["enc"]).abs().max().item(), o["enc"].abs().max().item()
    err, top = (out.logits.cpu() - o["logits"]).abs().max().item(), o["logits"].abs().max().item()
    print(f"enc err {eerr:.3e} (max {etop:.3e}); logits err {err:.3e}, max |logit| {top:.3e}")
    assert eerr < 2e-4 * max(1.0, etop) and err < 2e-4 * max(1.0, top)
    hip.zero_grad(); hip.backward(o["gl"].to(cuda), num_lookahead_tokens=look, prompt_ids=A)
    print("scalar of the logits: worst relative gradient error", _assert_grads(hip, o["g_logits"]))
    with torch.enable_grad():
        out = hip(labels=o["lab"], **kw)
    hip.zero_grad(); hip.backward()
    first = hip.flat_grads.clone()
    lerr = abs(out.loss.item() - o["loss"]) / abs(o["loss"])
    print(f"loss {o['loss']:.6f}, relative err {lerr:.3e}")
    assert lerr < 2e-4
    print("loss: worst relative gradient error", _assert_grads(hip, o["g_loss"]))
    with torch.enable_grad():
        hip(labels=o["lab"], **kw)
    hip.zero_grad(); hip.backward()
    assert torch.equal(hip.flat_grads, first)


def test_the_language_is_told_apart_and_none_is_the_default(cuda):
    """A = [1, 5, 1] against B' = [6, 5, 3] at T = 131: the oracle's projected states differ by 1.8e-2 and 3.3e-2 on rows 0 and 2 (max
    |enc| 0.30) and not at all on row 1.  Each of our runs lies within 1 / 50 of a row's gap of its own oracle and more than half the gap
    from the other; row 1 is bit-equal between our runs.  None is the configuration's default_prompt_id (5) bit for bit, and setting
    model.default_prompt_id = 1 equals [1, 1, 1]."""
    cfg, ref = _model()
    ref, hip = _pair(cuda, ref_cfg=(cfg, ref))
    x = _feats(131)
    wa, wb = PR.hf_encode(ref, x, A, 2), PR.hf_encode(ref, x, B2, 2)
    xd = x.to(cuda)
    with torch.no_grad():
        ga, gb = hip.encode(xd, num_lookahead_tokens=2, prompt_ids=A).cpu(), hip.encode(xd, num_lookahead_tokens=2, prompt_ids=torch.tensor(B2)).cpu()
    for r in (0, 2):
        gap = (wa[r] - wb[r]).abs().max().item()
        own = max((ga[r] - wa[r]).abs().max().item(), (gb[r] - wb[r]).abs().max().item())
        cross = min((ga[r] - wb[r]).abs().max().item(), (gb[r] - wa[r]).abs().max().item())
        print(f"row {r}: oracle gap {gap:.3e}; ours to its own oracle {own:.3e}, to the other {cross:.3e}")
        assert gap > 1e-2 and own < gap / 50 and cross > gap / 2
    assert torch.equal(wa[1], wb[1]) and torch.equal(ga[1], gb[1])
    assert hip.default_prompt_id == 5
    with torch.no_grad():
        none, fives = hip.encode(xd), hip.encode(xd, prompt_ids=[5, 5, 5])
        assert torch.equal(none, fives) and torch.equal(none, hip.encode(xd, prompt_ids=5)) and not torch.equal(none.cpu(), ga)
        hip.default_prompt_id = 1
        assert torch.equal(hip.encode(xd), hip.encode(xd, prompt_ids=[1, 1, 1])) and not torch.equal(hip.encode(xd), none)
        assert torch.equal(hip.encode(xd)[0].cpu(), ga[0])       # row 0 of A is language 1 as well


def test_state_dict_round_trips_with_transformers_names(cuda):
    ref, hip = _pair(cuda, ref_cfg=_model())
    sd, want = hip.state_dict(), ref.state_dict()
    assert set(sd) == set(want)
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n
    ref2, hip2 = _pair(cuda, seed=9)
    hip2.load_state_dict(sd)
    assert torch.equal(hip2.flat_params, hip.flat_params)
    copy.deepcopy(ref).load_state_dict({n: t.cpu() for n, t in sd.items()})      # and transformers' class takes ours back (strict)


@pytest.mark.parametrize("nB", [1, 3])
def test_generate_matches_transformers(cuda, nB):
    """generate(prompt_ids=) against transformers' generate(prompt_ids=) on nemotron35_refs' decode case (max_symbols_per_step = 3) under
    A: the oracle's three rows alone satisfy rnnt_refs.assert_decode_conditions (margin 1.9e-2, so no step is excluded and a flip is a
    failure; the free advance is on rows 1 and 2, so the conditions are asked of the three rows, also for nB = 1); tokens, frames and
    steps are equal at nB = 1 and 3.  Under B' rows 0 and 2 decode differently, row 1 the same."""
    cfg, ref = _decode_model()
    if "decode_rows" not in _ORACLE:
        _ORACLE["decode_rows"] = PR.decode_case(3, A, ref)
    rows3, _, margin3 = _ORACLE["decode_rows"]
    R.assert_decode_conditions(rows3, margin3, cfg.max_symbols_per_step)
    rows, Tp, margin = _ORACLE["decode_rows"] if nB == 3 else PR.decode_case(nB, A, ref)
    assert margin > 1e-2 and Tp == 39, (margin, Tp)
    ref, hip = _pair(cuda, ref_cfg=(cfg, ref))
    x = NR.decode_feats(nB).to(cuda)
    out = hip.generate(x, prompt_ids=A[:nB])
    for b, row in enumerate(rows):
        n = int(out.count[b])
        assert out.tokens[b, :n].tolist() == row["tokens"] and out.frames[b, :n].tolist() == row["frames"], b
        assert int(out.steps[b]) == len(row["steps"]), b
        forced = [t for k, d, t in row["steps"] if k != NR.BLANK and d == 1]
        assert all(out.frames[b, :n].tolist().count(t) == 3 for t in forced), b
    if nB == 3:
        rows_b, _, margin_b = PR.decode_case(nB, B2, ref)
        assert margin_b > 1e-2
        other = hip.generate(x, prompt_ids=B2)
        same = []
        for b, row in enumerate(rows_b):
            n = int(other.count[b])
            assert other.tokens[b, :n].tolist() == row["tokens"] and other.frames[b, :n].tolist() == row["frames"], b
            same.append(row["tokens"] == rows[b]["tokens"])
        assert same == [False, True, False]


# ----------------------------------------------------------------------------------------------------------- streaming
def _stream_feats(nB, look, n_chunks, seed=1):
    _, _, first, per = SR.geometry(9, look)
    return torch.randn(nB, first + (n_chunks - 1) * per, 80, generator=torch.Generator().manual_seed(seed))


def _stream(session, x, look, call="encode_chunk"):
    return [getattr(session, call)(ch.contiguous()) for ch in SR.chunks_of(x, 9, look)]


def _check(name, got, e32, e64):
    tol, err32 = K.measured_tol(e32.double(), e64, ENC_FLOOR * max(1.0, e64.abs().max().item()))
    err = K.max_err(got.double(), e64)
    print(f"{name}: kernel {err:.2e} | transformers fp32 streaming {err32:.2e} | bound {tol:.2e}")
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("look,ids,n_chunks", [(2, A, 8), (0, [6], 12)])
def test_encode_chunk_matches_transformers_streaming_and_the_offline_encode(cuda, look, ids, n_chunks):
    """encode_chunk over a stream with a language per row against transformers' chunk-by-chunk get_audio_features(use_cache=True, ...,
    prompt_ids=) in float64, and against this project's own offline encode() of the concatenated features, both under measured_tol with
    transformers' fp32 streaming as the yardstick and the 2e-4 * max(1, max |value|) floor, as tests/test_nemotron_stream_gpu.py."""
    cfg, ref = _model()
    nB = len(ids)
    x = _stream_feats(nB, look, n_chunks)
    e64, e32 = PR.hf_stream_encode(ref, x, look, ids, torch.float64), PR.hf_stream_encode(ref, x, look, ids, torch.float32)
    ref, hip = _pair(cuda, ref_cfg=(cfg, ref))
    s = hip.stream(nB, look, prompt_ids=ids)
    parent_bytes = super(type(s), s).state_bytes()
    assert s.state_bytes() == parent_bytes + 4 * nB + 4 * nB * PR.PROMPT_I and s.prompt_ids.tolist() == ids and s.pb.shape == (nB, PR.PROMPT_I)
    enc = torch.cat(_stream(s, x.to(cuda), look), 1)
    assert enc.shape == e64.shape == (nB, n_chunks * (look + 1), 64)
    _check("stream vs transformers", enc.cpu(), e32, e64)
    with torch.no_grad():
        off = hip.encode(x.to(cuda), num_lookahead_tokens=look, prompt_ids=ids)
    _check("offline vs transformers", off.cpu(), e32, e64)
    tol, _ = K.measured_tol(e32.double(), e64, ENC_FLOOR * max(1.0, e64.abs().max().item()))
    gap = (enc - off).abs().max().item()
    print(f"stream vs own offline encode: {gap:.2e} (bound {tol:.2e})")
    assert gap <= tol


def test_push_over_the_stream_equals_the_offline_generate(cuda):
    """The decode model on the first 281 feature frames (12 chunks, 36 encoder frames at lookahead 2) under A: transformers' OFFLINE
    generate on that prefix is the oracle (margin 1.9e-2); push() over the chunks and generate_streaming(prompt_ids=) give the tokens,
    frames, counts and steps of this project's own offline generate(prompt_ids=), which are the oracle's."""
    cfg, ref = _decode_model()
    x = NR.decode_feats(3)[:, :281].contiguous()
    rows, Tp = PR.hf_greedy(ref, x, A)
    margin = PR.hf_margins(ref, x, rows, A)
    assert Tp == 36 and margin > 1e-2, (Tp, margin)
    ref, hip = _pair(cuda, ref_cfg=(cfg, ref))
    xd = x.to(cuda)
    outs = _stream(hip.stream(3, 2, prompt_ids=A), xd, 2, "push")
    assert len(outs) == 12
    own = hip.generate(xd, num_lookahead_tokens=2, prompt_ids=A)
    got = hip.generate_streaming(xd, num_lookahead_tokens=2, prompt_ids=A)
    assert torch.equal(got.count, own.count) and torch.equal(got.steps, own.steps)
    for b, row in enumerate(rows):
        n = int(own.count[b])
        toks = [t for o in outs for t in o.tokens[b, :int(o.count[b])].tolist()]
        frs = [t for o in outs for t in o.frames[b, :int(o.count[b])].tolist()]
        assert toks == row["tokens"] == own.tokens[b, :n].tolist() and frs == row["frames"] == own.frames[b, :n].tolist(), b
        assert sum(int(o.steps[b]) for o in outs) == len(row["steps"]) == int(own.steps[b]), b
        assert torch.equal(got.tokens[b, :n], own.tokens[b, :n]) and torch.equal(got.frames[b, :n], own.frames[b, :n]), b


def test_graph_replay_is_bit_equal_and_a_language_change_needs_no_recapture(cuda):
    """graph=True against graph=False on the same inputs (6 chunks, B = 3, languages A).  Then reset(prompt_ids=B') on the session whose
    step is already captured: the same graph object replays and the outputs equal those of a fresh eager session under B' bit for bit (the
    captured step holds the addresses of the ids and of pb, not their values); rows 0 and 2 differ from A's, row 1 does not."""
    x = _stream_feats(3, 2, 6, seed=3).to(cuda)
    ref, hip = _pair(cuda, ref_cfg=_model())
    eager_a = torch.cat(_stream(hip.stream(3, 2, prompt_ids=A), x, 2), 1)
    eager_b = torch.cat(_stream(hip.stream(3, 2, prompt_ids=B2), x, 2), 1)
    s = hip.stream(3, 2, graph=True, prompt_ids=A)
    graphed = torch.cat(_stream(s, x, 2), 1)
    graph = s._graph
    assert graph is not None and torch.equal(graphed, eager_a)
    s.reset(prompt_ids=B2)
    assert s.frames_seen == 0 and s.prompt_ids.tolist() == B2
    again = torch.cat(_stream(s, x, 2), 1)
    assert s._graph is graph and torch.equal(again, eager_b)
    assert not torch.equal(again[0], graphed[0]) and torch.equal(again[1], graphed[1]) and not torch.equal(again[2], graphed[2])
    s.reset()                                                    # None keeps the languages
    assert s.prompt_ids.tolist() == B2 and torch.equal(torch.cat(_stream(s, x, 2), 1), eager_b) and s._graph is graph
    s.close()


# ----------------------------------------------------------------------------------------------------------- the loop
def test_dynamic_eval_follows_default_prompt_id(cuda):
    """parakeet_tdt_lib.dynamic_eval_transducer_loss drives the model unchanged and passes no prompt: `model.default_prompt_id = 3` (the
    configuration says 5) points it at a language.  A [1, 80, 160] spectrogram, two windows of 128 frames at overlap 64, two augmented
    copies, Adam at 1e-5, against rnnt_refs.dynamic_eval_rnnt_ref on transformers' model with config.default_prompt_id = 3: merged ids and
    frames are equal, the adapted joint logits of a probe after the last step are within 1e-3, and the oracle's smallest top-2 margin is at
    least 1e-2 (9.6e-2).  The oracle under the configuration's own language gives other probe logits by more than ten times that bar, so
    the language is told apart.  After the first update the prompt projector has moved (of linear_1's prompt columns only column 3),
    and parameters and `frozen` are restored at the end."""
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M, parakeet_tdt_lib as N
    L = PR.LOOP
    cfg, ref = _decode_model()
    ref, hip = _pair(cuda, ref_cfg=(cfg, ref))
    assert hip.frozen_in_the_loop == ("encoder.subsampling.", "decoder.") and hip.default_prompt_id == PR.DEFAULT_PROMPT
    spec, tok = PR.loop_inputs()
    args = argparse.Namespace(epochs=1, shuffle=False)
    probe_x = torch.randn(1, 67, 80, generator=torch.Generator().manual_seed(9))
    probe_ids = torch.tensor([[NR.BLANK, 5, 9]])
    infos = {}
    for p in (PR.LOOP_PROMPT, PR.DEFAULT_PROMPT):
        m = copy.deepcopy(ref)
        m.config.default_prompt_id = p
        infos[p] = {"probe": (probe_x, probe_ids)}
        random.seed(17)
        res = R.dynamic_eval_rnnt_ref(args, m, spec, L["seq_len"], 64, tok, L["num_negatives"], L["lr_args"],
                                      generator=torch.Generator().manual_seed(L["mask_seed"]), logits_out=infos[p])
        if p == PR.LOOP_PROMPT:
            want_ids, want_frames = res
    info = infos[PR.LOOP_PROMPT]
    assert info["margin"] >= 1e-2, info["margin"]
    assert len(want_ids) > 0 and any(k != NR.BLANK for k, _, _ in info["steps"]) and any(k == NR.BLANK for k, _, _ in info["steps"])
    apart = (info["logits"] - infos[PR.DEFAULT_PROMPT]["logits"]).abs().max().item()
    assert apart > 1e-2, apart
    hip.default_prompt_id = PR.LOOP_PROMPT
    before, frozen_before = hip.flat_params.clone(), hip.frozen
    start = {n: hip.P[n].clone() for n in (M.W1H, M.W1P, M.B1, M.W2, M.B2)}
    got, steps, moved, step = {}, [], [], N.Adam.step

    def probing_step(self, *a, **k):
        r = step(self, *a, **k)
        steps.append(1)
        if len(steps) == 1:
            moved.append({n: hip.P[n].clone() for n in start})
        with torch.no_grad():
            got["logits"] = hip(input_features=probe_x.to(cuda), decoder_input_ids=probe_ids).logits.cpu()
        return r

    N.Adam.step = probing_step
    args.spec_augment_generator = torch.Generator().manual_seed(L["mask_seed"])
    random.seed(17)
    try:
        ids, frames, text = N.dynamic_eval_transducer_loss(args, hip, spec, L["seq_len"], 64, tok, use_tqdm=False, num_negatives=L["num_negatives"],
                                                           lr_args=L["lr_args"], spec_augment_config=R.PR.SPEC_AUGMENT)
    finally:
        N.Adam.step = step
    assert len(steps) == 2                                                       # two windows, two updates
    for n in start:
        assert not torch.equal(moved[0][n], start[n]), f"{n} did not adapt"
    others = [p for p in range(PR.NUM_PROMPTS) if p != PR.LOOP_PROMPT]
    assert torch.equal(moved[0][M.W1P][:, others], start[M.W1P][:, others]) and not torch.equal(moved[0][M.W1P][:, 3], start[M.W1P][:, 3])
    assert torch.equal(hip.flat_params, before) and hip.frozen is frozen_before and hip.frozen == set()
    assert hip.default_prompt_id == PR.LOOP_PROMPT
    assert text == tok.ids_to_text(ids) and ids == want_ids and frames == want_frames
    err = (got["logits"] - info["logits"]).abs().max().item()
    print(f"adapted joint logits: ours vs fp32 oracle {err:.3e} (max |logit| {info['logits'].abs().max().item():.3e}); other language {apart:.3e}")
    assert err < 1e-3


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_fire_on_the_device_path(cuda):
    from dynamic_asr_eval_amd import nemotron3_5_asr_model as M, nemotron_asr_streaming_model as NM, ops
    o = _oracle(131, 2)
    ref, hip = _pair(cuda, ref_cfg=_model())
    x = o["x"].to(cuda)
    kw = dict(input_features=x, decoder_input_ids=o["dec_in"])
    for bad, word in ((dict(prompt_ids=[1, 5]), "prompt_ids"), (dict(prompt_ids=[1, 5, 8]), "prompt_ids"), (dict(prompt_ids=-1), "prompt_ids"),
                      (dict(prompt_ids=torch.tensor([1.0, 5.0, 1.0])), "prompt_ids"), (dict(prompt_ids=True), "prompt_ids"),
                      (dict(attention_mask=torch.ones(B, 131)), "attention_mask"), (dict(use_cache=True), "use_cache"),
                      (dict(num_lookahead_tokens=-1), "num_lookahead_tokens"), (dict(labels=o["lab"], sigma=0.05), "sigma")):
        with pytest.raises(ops.DynError) as e:
            hip(**kw, **bad)
        assert word in str(e.value), str(e.value)
    for call in (lambda: hip.encode(x, prompt_ids=[9, 0, 0]), lambda: hip.generate(x, prompt_ids=[0, 0]),
                 lambda: hip.stream(3, 2, prompt_ids=[1, 5]), lambda: hip.stream(2, 2, prompt_ids=8),
                 lambda: hip.generate_streaming(x[:, :17], prompt_ids=[0, 0, 8])):
        with pytest.raises(ops.DynError) as e:
            call()
        assert "prompt_ids" in str(e.value), str(e.value)
    with torch.enable_grad():
        out = hip(labels=o["lab"], num_lookahead_tokens=2, prompt_ids=A, **kw)
    for call in (lambda: hip.head(out.enc, o["dec_in"], prompt_ids=B2), lambda: hip.backward(prompt_ids=B2), lambda: hip.backward(prompt_ids=5)):
        with pytest.raises(ops.DynError) as e:
            call()
        assert "prompt_ids" in str(e.value) and "continues an encode" in str(e.value)
    with pytest.raises(ops.DynError) as e:
        hip.backward(num_lookahead_tokens=0)
    assert "num_lookahead_tokens" in str(e.value)
    with torch.enable_grad():
        hip(labels=o["lab"], num_lookahead_tokens=2, prompt_ids=A, **kw)
    hip.zero_grad(); hip.backward(num_lookahead_tokens=2, prompt_ids=torch.tensor(A))
    with pytest.raises(ops.DynError) as e:
        hip.generate(enc=out.enc, prompt_ids=A)
    assert "prompt_ids" in str(e.value) and "enc" in str(e.value)
    s = hip.stream(3, 2, prompt_ids=A)
    with pytest.raises(ops.DynError) as e:
        s.reset(prompt_ids=[1, 5, 1, 1])
    assert "prompt_ids" in str(e.value) and s.prompt_ids.tolist() == A
    with pytest.raises(ops.DynError) as e:
        hip.default_prompt_id = 8
    assert "default_prompt_id" in str(e.value) and hip.default_prompt_id == 5
    for make, cfg in ((M.Nemotron3_5AsrForRNNT, NR.hf_config()), (NM.NemotronAsrStreamingForRNNT, PR.hf_config())):
        with pytest.raises(ops.DynError) as e:
            make(cfg, device=cuda)
        assert "model_type" in str(e.value)
