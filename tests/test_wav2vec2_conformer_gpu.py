"""Wav2Vec2ConformerForCTC (wav2vec2_conformer_model.py: Wav2Vec2ForCTC's front end + conformer layers with Transformer-XL relative-position
or rotary attention, csrc/relshift.hip) against transformers' Wav2Vec2ConformerForCTC on the CPU with the same state dict — logits, every
parameter gradient, both position types and extractor layouts, the dynamic-eval loops, bucketed hipGraph replay and the harness at the bars
tests/test_wavlm_gpu.py holds WavLM to — and the four new kernels against float64 / exact fp32 restatements."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

GROUP = dict(feat_extract_norm="group", conv_bias=False)
LAYER = dict(feat_extract_norm="layer", conv_bias=True)
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32, ctc_loss_reduction="mean", hidden_act="swish")
PF = "wav2vec2_conformer."
UNUSED = {PF + "masked_spec_embed", PF + "encoder.pos_conv_embed.conv.bias", PF + "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
          PF + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
INV_FREQ = PF + "encoder.embed_positions.inv_freq"
POS_W = PF + "encoder.layers.{}.self_attn.linear_pos.weight"
POS_U = PF + "encoder.layers.{}.self_attn.pos_bias_u"
POS_V = PF + "encoder.layers.{}.self_attn.pos_bias_v"


def _pair(cuda, seed=0, pos="relative", flags=GROUP, arch=TOY, **over):
    from transformers import Wav2Vec2ConformerConfig, Wav2Vec2ConformerForCTC as HF
    from dynamic_asr_eval_amd.wav2vec2_conformer_model import Wav2Vec2ConformerForCTC
    torch.manual_seed(seed)
    cfg = Wav2Vec2ConformerConfig(**dict(arch, **over), **flags, position_embeddings_type=pos)
    ref = HF(cfg).eval()
    with torch.no_grad():   # HF initialises biases / norms / running statistics to trivial values: randomise so every path is exercised
        for n, p in ref.named_parameters():
            if p.dim() == 1 or "original0" in n:
                p.add_(0.1 * torch.randn_like(p))
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
    hip = Wav2Vec2ConformerForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict(), strict=False)
    return ref, hip


def _forward_and_every_gradient(cuda, ref, hip, x, g, logit_bar):
    out_ref = ref(x).logits
    out = hip(x.to(cuda)).logits
    assert out.shape == out_ref.shape
    err = (out.cpu() - out_ref).abs().max().item()
    print("forward err", err)
    assert err < logit_bar, err
    gl = torch.randn(out_ref.shape, generator=g) / out_ref.numel()
    ref.zero_grad()
    out_ref.backward(gl)
    hip.zero_grad(); hip.backward(gl.to(cuda))
    grads = hip.grads_hf()
    named = dict(ref.named_parameters())
    assert set(grads) == set(named)
    assert {n for n, p in named.items() if p.grad is None} == UNUSED       # built by transformers, never used in this forward
    worst = 0.0
    for n, p in named.items():
        if p.grad is None:
            assert grads[n].abs().max().item() == 0.0, n
            continue
        assert grads[n].shape == p.grad.shape, n
        diff = (grads[n].cpu() - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
    print("worst relative gradient error", worst)
    return grads, named


def _state_dict_round_trip(ref, hip):
    sd = hip.state_dict()                                   # HF names and layouts, bit for bit; parameters + the batch-norm buffers
    want = {n: t for n, t in ref.state_dict().items() if n != INV_FREQ}
    bn = {n for n, _ in ref.named_buffers() if ".batch_norm." in n}
    assert len(bn) == 3 * hip.cfg["num_hidden_layers"]
    assert set(sd) == {n for n, _ in ref.named_parameters()} | bn == set(want)
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n
    for n in bn:                                            # outside the flat vector: no optimiser step can move them
        assert n not in hip.P and n in hip.buffers_


@pytest.mark.parametrize("pos,flags,L,over", [
    ("relative", GROUP, 6000, {}), ("relative", LAYER, 6000, {}), ("rotary", GROUP, 6000, {}), ("rotary", LAYER, 6000, {}),
    ("relative", LAYER, 30000, {}), ("relative", GROUP, 6000, dict(hidden_act="gelu")), ("rotary", LAYER, 6000, dict(layer_norm_eps=1e-3))],
    ids=["relative-group", "relative-layer", "rotary-group", "rotary-layer", "relative-layer-93-frames", "relative-gelu", "rotary-eps1e-3"])
def test_forward_backward_matches_transformers(cuda, pos, flags, L, over):
    """18 frames are fewer than the 31 taps of the depthwise kernel: every frame is inside its halo on both sides; 93 frames have interior
    frames too and a second row block of the score kernels.  `layer_norm_eps=1e-3` reaches feature_projection.layer_norm and
    encoder.layer_norm only (the per-layer norms keep torch's 1e-5): applied anywhere else the logits would leave the bar."""
    ref, hip = _pair(cuda, pos=pos, flags=flags, **over)
    assert (hip.cfg["feat_extract_norm"], hip.cfg["conv_bias"], hip.cfg["position_embeddings_type"]) == (flags["feat_extract_norm"], flags["conv_bias"], pos)
    assert hip.cfg["hidden_act"] == over.get("hidden_act", "swish") and hip.cfg["layer_norm_eps"] == over.get("layer_norm_eps", 1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, L, generator=g)
    assert hip.conv_lengths(L)[-1] == (18 if L == 6000 else 93)
    grads, named = _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    if pos == "relative":
        for l in range(2):
            for n in (POS_W, POS_U, POS_V):
                assert grads[n.format(l)].abs().max().item() > 0.0, n
    _state_dict_round_trip(ref, hip)


@pytest.mark.parametrize("pos", ["relative", "rotary"])
def test_wide_shape_forward_and_every_gradient(cuda, pos):
    """The published large widths (1024 hidden, 16 x 64 heads, FFN 4096, layer-norm extractor) without the 24 layers."""
    arch = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, conv_dim=(512,) * 7,
                num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, vocab_size=32, ctc_loss_reduction="mean", hidden_act="swish")
    ref, hip = _pair(cuda, pos=pos, flags=LAYER, arch=arch)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16000, generator=g)
    assert hip.conv_lengths(16000)[-1] == 49
    _forward_and_every_gradient(cuda, ref, hip, x, g, 5e-4)


# ----------------------------------------------------------------------------------------------------------- the four kernels
_shift_ref = K.shift_pad_view_slice      # transformers' pad / view / slice: [B, nh, T, 2T - 1] -> [B, nh, T, T]


@pytest.mark.parametrize("shape,valid,pad", [((2, 3, 37, 64), None, 0), ((2, 3, 37, 64), 29, 0), ((1, 2, 300, 32), None, 0),
                                             ((2, 2, 1, 32), None, 0), ((2, 2, 2, 32), None, 0), ((2, 3, 37, 64), 29, 4)],
                         ids=["full", "valid29-of-37", "T300-D32", "T1", "T2", "ld_bd-2T+3"])
def test_kernels_against_float64(cuda, shape, valid, pad):
    """dyn_softmax_relshift_fwd_len / dyn_relshift_bwd / dyn_head_bias_add / dyn_head_bias_bwd.  T = 37 leaves the 16-row blocks ragged (and
    every window start unaligned), T = 300 takes two row items per thread and 19 row blocks, T = 1 and T = 2 have windows that are the whole
    row / all but one element; `ld_bd = 2T + 3` pads BD's rows: the padding holds NaN in the forward (never read) and is written 0 backward.
    Probabilities: kernel_refs.measured_tol, 4 x the error of torch's own fp32 result against float64 + 2e-6.  The backward shift, q + u /
    q + v and dq are copies or single fp32 additions: bit-equal to the fp32 torch restatement, checked on NaN-filled outputs so an element
    the kernel does not write shows.  du / dv sum B T rows of O(1) terms: kernel_refs.wgrad_tol(5e-4, B T, 531)."""
    from dynamic_asr_eval_amd import ops
    B, nh, T, D = shape
    H, R = nh * D, 2 * T - 1
    ld = R + pad
    g = torch.Generator().manual_seed(7)
    S = torch.randn(B, nh, T, T, generator=g)
    BD = torch.full((B, nh, T, ld), float("nan"))
    BD[..., :R] = torch.randn(B, nh, T, R, generator=g)
    dS = torch.randn(B, nh, T, T, generator=g)
    Lv = T if valid is None else valid
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    assert torch.equal(_shift_ref(BD[..., :R]), BD[..., :R].gather(-1, (T - 1 - i + j).expand(B, nh, T, T)))     # the index the kernels use

    def probs(dt):
        s = S.to(dt) + _shift_ref(BD[..., :R].to(dt))
        y = torch.zeros_like(s)
        y[..., :Lv] = torch.softmax(s[..., :Lv], -1)
        return y

    y64, y32 = probs(torch.float64), probs(torch.float32)
    Sd, BDd, dSd = S.to(cuda), BD.to(cuda), dS.to(cuda)
    vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
    got = ops.softmax_relshift(Sd, BDd, valid=vd, ld_bd=ld)
    tol, e32 = K.measured_tol(y32, y64, 2e-6)
    err = K.max_err(got, y64)
    print(f"  probabilities: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, (err, tol)
    given = torch.full_like(Sd, float("nan"))
    assert ops.softmax_relshift(Sd, BDd, out=given, valid=vd, ld_bd=ld) is given and torch.equal(given, got)
    inplace = Sd.clone()
    ops.softmax_relshift(inplace, BDd, out=inplace, valid=vd, ld_bd=ld)
    assert torch.equal(inplace, got)                                                    # the model runs it in place
    if valid is not None:
        assert got[..., Lv:].abs().max().item() == 0.0
    # backward shift: dS in the window, zeros everywhere else of the ld-float row; also what autograd gives through pad / view / slice
    want = torch.zeros(B, nh, T, ld)
    for r in range(T):
        want[:, :, r, T - 1 - r:2 * T - 1 - r] = dS[:, :, r]
    leaf = BD[..., :R].clone().requires_grad_()
    (_shift_ref(leaf) * dS).sum().backward()
    assert torch.equal(leaf.grad, want[..., :R])
    out = torch.full((B, nh, T, ld), float("nan"), device=cuda)
    assert ops.relshift_bwd(dSd, out=out, ld_bd=ld) is out and torch.equal(out.cpu(), want)
    assert torch.equal(ops.relshift_bwd(dSd, ld_bd=ld).cpu(), want)
    # the per-head biases on q inside a packed [B, T, 3H] projection output
    qkv = torch.randn(B, T, 3 * H, generator=g)
    u, v = torch.randn(nh, D, generator=g), torch.randn(nh, D, generator=g)
    qu, qv = ops.head_bias_add(qkv.to(cuda), u.to(cuda), v.to(cuda), H=H, ldq=3 * H)
    assert qu.shape == qv.shape == (B, T, H)
    assert torch.equal(qu.cpu(), qkv[..., :H] + u.view(H)) and torch.equal(qv.cpu(), qkv[..., :H] + v.view(H))
    dqu, dqv = torch.randn(B, T, H, generator=g), torch.randn(B, T, H, generator=g)
    old_u, old_v = torch.randn(nh, D, generator=g), torch.randn(nh, D, generator=g)
    rows_tol = K.wgrad_tol(5e-4, B * T, 531)
    for beta in (0.0, 1.0):
        dq = torch.full((B, T, 3 * H), float("nan"), device=cuda)
        du, dv = old_u.to(cuda), old_v.to(cuda)
        ops.head_bias_bwd(dqu.to(cuda), dqv.to(cuda), dq, du, dv, beta=beta, ldq=3 * H)
        assert torch.equal(dq[..., :H].cpu(), dqu + dqv) and torch.isnan(dq[..., H:]).all()          # k | v columns are not its to write
        for name, gotw, src, old in (("du", du, dqu, old_u), ("dv", dv, dqv, old_v)):
            err = K.max_err(gotw.view(H), src.double().sum((0, 1)) + beta * old.double().view(H))
            print(f"  {name} (beta {beta:g}): kernel {err:.2e} | bound {rows_tol:.2e}")
            assert err <= rows_tol, (name, err, rows_tol)


@pytest.mark.parametrize("pos", ["relative", "rotary"])
def test_backward_is_bit_reproducible(cuda, pos):
    ref, hip = _pair(cuda, seed=1, pos=pos)
    x = torch.randn(2, 6000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert first.abs().max().item() > 0.0


@pytest.mark.parametrize("pos", ["relative", "rotary"])
def test_active_subset_backward(cuda, pos):
    ref, hip = _pair(cuda, seed=3, pos=pos)
    x = torch.randn(2, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out); gl[0] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:1].contiguous(), n_active=1)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_frozen_prefixes(cuda):
    ref, hip = _pair(cuda, seed=4)
    x = torch.randn(1, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {PF + "feature_extractor", PF + "encoder.layers.0.self_attn.linear_pos", PF + "encoder.layers.0.self_attn.pos_bias"}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[PF + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
    for n in (POS_W, POS_U, POS_V):
        assert hip.G[n.format(0)].abs().max().item() == 0.0, n
        assert hip.G[n.format(1)].abs().max().item() > 0.0, n
    assert hip.G[PF + "encoder.layers.0.self_attn.linear_q.weight"].abs().max().item() > 0.0
    hip.frozen = set()


@pytest.mark.parametrize("pos", ["relative", "rotary"])
def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda, pos):
    """The protocol and bars of tests/test_wavlm_gpu.py's test of the same name (logits of the utterance's own frames 2e-5, flat gradient 1e-4
    of its largest entry).  The position table is the BUCKET's (16 / 24 frames); with 10 - 18 valid frames every one of them has padded
    frames inside the 31-tap window of the depthwise conv, so the run differs from the unpadded one unless the GLU output and the dgrad
    are masked.  Two lengths in one bucket and one in another, a shorter utterance replayed after a longer one, and a second backward variant
    (frozen extractor) after the bucket's activations were released."""
    ref, hip = _pair(cuda, seed=11, pos=pos)
    hip.graph_after, hip.bucket_frames = 1, 8
    lengths = [4400, 4000, 6000, 3500, 4400]                    # frames 13, 12, 18, 10, 13 -> buckets 16, 16, 24, 16, 16

    def run(L, graphs, frozen=()):
        x = (torch.randn(2, L, generator=torch.Generator().manual_seed(L)) * 0.3).to(cuda)
        hip.use_graphs, hip.frozen = graphs, set(frozen)
        with torch.enable_grad():
            out = hip(x)
        assert hip._ctx_static == graphs
        T = out.frames
        logits = out.logits[:, :T].clone()
        gl = torch.zeros_like(out.logits[:1])
        gl[:, :T] = (torch.randn(1, T, logits.shape[-1], generator=torch.Generator().manual_seed(L + 1)) / T).to(cuda)   # zero past the utterance, as CTC gives
        hip.zero_grad(); hip.backward(gl.contiguous(), n_active=1)
        return T, out.logits.shape[1], logits, hip.flat_grads.clone()

    assert [hip.conv_lengths(L)[-1] for L in lengths] == [13, 12, 18, 10, 13]
    for k, L in enumerate(lengths):
        fz = (PF + "feature_extractor",) if k == 4 else ()      # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        assert (lo - lo2).abs().max().item() < 2e-5 * max(1.0, lo2.abs().max().item()), (L, (lo - lo2).abs().max().item())
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        assert hip.G[PF + "encoder.layers.0.conv_module.depthwise_conv.weight"].abs().max().item() > 0.0
        if fz:
            assert hip.G[PF + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
            assert hip.G[PF + "feature_projection.layer_norm.weight"].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


@pytest.mark.parametrize("pos,flags,seed", [("relative", LAYER, 1), ("rotary", GROUP, 0)], ids=["relative-layer", "rotary-group"])
def test_dynamic_eval_su_matches_oracle(cuda, pos, flags, seed):
    import argparse
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    # The weights' seed is one at which the ORACLE stays finite: a random model's greedy pseudo-label may hold id 3, which decodes to the text
    # "<unk>" and tokenises back to five ids, more than the frames can emit: CTC loss inf, NaN weights from there on, in transformers as here.
    ref, hip = _pair(cuda, seed=seed, pos=pos, flags=flags)
    tok = W.CharTokenizer()
    g = torch.Generator().manual_seed(9)
    utts_ref = [{'waveform': torch.randn(1, n, generator=g) * 0.1 + 0.01} for n in (4000, 7000, 5200)]
    utts = [{'waveform': u['waveform'].clone()} for u in utts_ref]
    args = argparse.Namespace(epochs=1, shuffle=False)
    before = hip.flat_params.clone()
    dynamic_eval_su_ref(args, ref, utts_ref, tok, MADGRAD_REF, lr_args={'lr': 1e-5})
    W.dynamic_eval_su(args, hip, utts, 0, 0, tok, None, use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-5})
    assert torch.equal(hip.flat_params, before)
    for a, b in zip(utts, utts_ref):
        assert torch.isfinite(b['probs']).all()
        assert a['probs'].shape == b['probs'].shape
        assert (a['probs'] - b['probs']).abs().max().item() < 1e-3
        assert torch.equal(a['probs'].argmax(-1), b['probs'].argmax(-1))


@pytest.mark.parametrize("pos,flags,seed", [("relative", LAYER, 4), ("rotary", GROUP, 2)], ids=["relative-layer", "rotary-group"])
def test_chunked_dynamic_eval_matches_oracle(cuda, pos, flags, seed):
    import argparse
    import numpy as np
    from oracle.wav2vec2_ref import dynamic_eval_chunked_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    seq_len, overlap, L = 6000, 1280, 15000
    ref, hip = _pair(cuda, seed=seed, pos=pos, flags=flags)   # a seed at which the oracle stays finite, see test_dynamic_eval_su_matches_oracle
    tok = W.CharTokenizer()
    wav = torch.randn(1, L, generator=torch.Generator().manual_seed(L + overlap)) * 0.1 + 0.01
    args = argparse.Namespace(epochs=1, shuffle=False)
    before = hip.flat_params.clone()
    np.random.seed(1000 + L)
    want = dynamic_eval_chunked_ref(args, ref, wav, seq_len, overlap, tok, MADGRAD_REF, lr_args={'lr': 1e-5})
    np.random.seed(1000 + L)
    got = W.dynamic_eval(args, hip, wav, seq_len, overlap, tok, None, use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-5})
    assert torch.equal(hip.flat_params, before)
    assert got.shape == want.shape and np.isfinite(want).all(), (got.shape, want.shape)
    assert np.abs(got - want).max() < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))


def test_run_wav2vec2_harness_with_a_conformer_directory(cuda, tmp_path, capsys):
    """`-c DIR` whose config.json says `model_type: wav2vec2-conformer` builds Wav2Vec2ConformerForCTC and runs; `--config` with that file does
    too (seeded weights); the same weights offered with a wav2vec2 config are refused with an error that names a parameter."""
    from transformers import Wav2Vec2Config, Wav2Vec2ConformerConfig, Wav2Vec2ConformerForCTC as HF
    from dynamic_asr_eval_amd import run_wav2vec2 as R, wav2vec2_lib as W
    from dynamic_asr_eval_amd.ops import DynError
    torch.manual_seed(0)
    cfg = Wav2Vec2ConformerConfig(**TOY, **GROUP)
    ref = HF(cfg)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    assert '"model_type": "wav2vec2-conformer"' in open(d / "config.json").read()
    torch.save(ref.state_dict(), str(d / "pytorch_model.bin"))
    n_params = sum(p.numel() for p in ref.parameters())
    R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d), "-nv"]))
    out = capsys.readouterr().out
    assert f"Loaded model from {d}" in out and f"Total number of parameters: {n_params / 1e6:.2f}M" in out and "WER: " in out
    R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "--config", str(d / "config.json"), "-nv"]))
    out = capsys.readouterr().out
    assert f"Total number of parameters: {n_params / 1e6:.2f}M" in out and "WER: " in out
    w2 = tmp_path / "w2.json"
    with open(w2, "w") as f:
        f.write(Wav2Vec2Config(**{k: v for k, v in TOY.items() if k != "hidden_act"}, **GROUP).to_json_string(use_diff=False))
    with pytest.raises((KeyError, DynError)) as e:
        R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "--config", str(w2), "-nv"]))
    assert "wav2vec2." in str(e.value)                          # names the first parameter the checkpoint does not have
