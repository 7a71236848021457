"""WavLMForCTC (wavlm_model.py: Wav2Vec2ForCTC + the gated relative-position bias of csrc/relbias.hip) against transformers' WavLMForCTC on
the CPU with the same state dict — logits, every parameter gradient, both layouts, the dynamic-eval loops, bucketed hipGraph replay and the
harness at the bars tests/test_wav2vec2_layernorm_gpu.py holds wav2vec2 to — and the four new kernels against float64 restatements."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

POST_GROUP = dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False)      # base, base-plus
STABLE_LAYER = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)      # large
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32, ctc_loss_reduction="mean")
SMALL_BUCKETS = dict(num_buckets=8, max_bucket_distance=12)
EMBED = "wavlm.encoder.layers.0.attention.rel_attn_embed.weight"


def _pair(cuda, seed=0, flags=POST_GROUP, arch=TOY, buckets=SMALL_BUCKETS):
    from transformers import WavLMConfig, WavLMForCTC as HF
    from dynamic_asr_eval_amd.wavlm_model import WavLMForCTC
    torch.manual_seed(seed)
    cfg = WavLMConfig(**arch, **flags, **buckets)
    ref = HF(cfg).eval()
    with torch.no_grad():   # HF initialises biases / LN / the gate constant to trivial values: randomise so every gradient path is exercised
        for n, p in ref.named_parameters():
            if p.dim() == 1 or "original0" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif n.endswith("gru_rel_pos_const"):
                p.add_(0.3 * torch.randn_like(p))
            elif n.endswith("rel_attn_embed.weight"):
                p.copy_(0.5 * torch.randn_like(p))
    hip = WavLMForCTC(cfg, device=cuda)
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
    worst = 0.0
    for n, p in named.items():
        if p.grad is None:
            assert n == "wavlm.masked_spec_embed" and grads[n].abs().max().item() == 0.0, n       # unused in eval mode
            continue
        assert grads[n].shape == p.grad.shape, n
        diff = (grads[n].cpu() - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
    print("worst relative gradient error", worst)
    return grads, named


@pytest.mark.parametrize("flags,buckets,L", [(POST_GROUP, SMALL_BUCKETS, 6000), (STABLE_LAYER, SMALL_BUCKETS, 6000),
                                             (POST_GROUP, dict(num_buckets=320, max_bucket_distance=800), 30000)],
                         ids=["postln-group-8x12", "stable-layer-8x12", "postln-group-320x800"])
def test_forward_backward_matches_transformers(cuda, flags, buckets, L):
    """18 frames with (8, 12): distances up to 17 take the exact, the logarithmic and the clamped branch on both signs (buckets 0-3 and 5-7;
    bucket 4 = "distance 0 on the positive side" does not exist).  93 frames with (320, 800): distances cross 80, where the default table
    turns logarithmic.  Two layers share layer 0's table, so its gradient is checked against an oracle that sums both."""
    ref, hip = _pair(cuda, flags=flags, buckets=buckets)
    assert (hip.cfg["feat_extract_norm"], hip.cfg["conv_bias"], hip.cfg["do_stable_layer_norm"]) == \
        (flags["feat_extract_norm"], flags["conv_bias"], flags["do_stable_layer_norm"])
    assert (hip.cfg["num_buckets"], hip.cfg["max_bucket_distance"]) == (buckets["num_buckets"], buckets["max_bucket_distance"])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, L, generator=g)
    T = hip.conv_lengths(L)[-1]
    assert T == (18 if L == 6000 else 93)
    grads, named = _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    used = sorted(set(hip.bucket_table(T).cpu().tolist()))
    if buckets is SMALL_BUCKETS:
        assert used == [0, 1, 2, 3, 5, 6, 7]
    else:
        assert 2 * 80 < len(used) < 2 * T - 1                # past +-80 several distances share a bucket
    ge, want = grads[EMBED].cpu(), named[EMBED].grad
    for k in range(buckets["num_buckets"]):                 # every bucket a distance falls into has a gradient from BOTH layers; the others none
        if k in used:
            assert ge[k].abs().max().item() > 0.0 and want[k].abs().max().item() > 0.0, k
        else:
            assert ge[k].abs().max().item() == 0.0 and want[k].abs().max().item() == 0.0, k
    sd = hip.state_dict()                                   # state_dict round trip keeps HF names and layouts, bit for bit
    for n, p in ref.named_parameters():
        assert sd[n].shape == p.shape and torch.equal(sd[n].cpu(), p.detach()), n
    assert set(sd) == {n for n, _ in ref.named_parameters()}


def test_rel_attn_embed_gradient_sums_over_the_layers(cuda):
    """Layer 0 owns the table and every layer uses it: what layer 0's own backward adds to the table's gradient is recorded on a second,
    bit-identical run, and the full gradient must differ from it by far more than rounding: layer 1's share."""
    ref, hip = _pair(cuda, seed=2)
    x = torch.randn(2, 6000, generator=torch.Generator().manual_seed(4)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(5)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl)
    both = hip.G[EMBED].clone()
    g0 = {}
    orig = hip._softmax_bwd

    def only_layer0(dS, kept, h, l, dh):
        if l == 0:
            before = hip.G[EMBED].clone()
            orig(dS, kept, h, l, dh)
            g0["v"] = hip.G[EMBED] - before
        else:
            orig(dS, kept, h, l, dh)
    hip._softmax_bwd = only_layer0
    try:
        hip(x); hip.zero_grad(); hip.backward(gl)
    finally:
        del hip._softmax_bwd
    assert torch.equal(hip.G[EMBED], both)
    rest = (both - g0["v"]).abs().max().item()
    assert rest > 1e-3 * both.abs().max().item(), rest      # layer 1's share is no rounding residue


def test_wide_shape_forward_and_every_gradient(cuda):
    """WavLM-large's widths (1024 hidden, 16 x 64 heads, FFN 4096, 64 channels per positional-conv group) without its 24 layers."""
    arch = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, conv_dim=(512,) * 7,
                num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, vocab_size=32, ctc_loss_reduction="mean")
    ref, hip = _pair(cuda, flags=STABLE_LAYER, arch=arch, buckets={})
    assert hip.cfg["num_buckets"] == 320 and hip.cfg["max_bucket_distance"] == 800
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16000, generator=g)
    _forward_and_every_gradient(cuda, ref, hip, x, g, 5e-4)


# ----------------------------------------------------------------------------------------------------------- the four kernels in float64
def _gate_ref(h, W, bias, const, nh):
    """gate, a, c [B, nh, T] in the dtype of the operands (WavLMAttention.forward steps 1-3 restated)."""
    B, T, H = h.shape
    p = h.view(B, T, nh, H // nh).permute(0, 2, 1, 3) @ W.t() + bias                    # [B, nh, T, 8]
    a, c = torch.sigmoid(p[..., :4].sum(-1)), torch.sigmoid(p[..., 4:].sum(-1))
    return a * (c * const.view(1, nh, 1) - 1.0) + 2.0, a, c


_bias_ref = K.bias_ref      # gate[b, head, t] * E[bucket(s - t), head] as [B, nh, T, T]


SMALL = (2, 3, 37, 64, 8, 12)          # B, nh, T, D, num_buckets, max_bucket_distance


@pytest.mark.parametrize("shape,valid,Tmax", [(SMALL, None, 37), (SMALL, 29, 40), ((1, 2, 300, 32, 320, 800), None, 300)],
                         ids=["full", "valid29-of-37", "T300-D32-320x800"])
def test_kernels_against_float64(cuda, shape, valid, Tmax):
    """dyn_relpos_gate_fwd / dyn_softmax_relbias_fwd_len / dyn_relbias_bwd / dyn_relpos_gate_bwd at B = 2, nh = 3, T = 37, D = 64, 8 buckets:
    odd T and nh leave the 16-row blocks, the diagonals and the bucket folds ragged; `valid29-of-37` masks keys 29.. and reads a table built
    for more frames than the scores have.  T = 300 takes the paths the small shape cannot: two row items per thread, a last row block of 12
    rows, more distances (599) than one workgroup of the second backward kernel, more buckets (320) than threads in the fold, the
    logarithmic part of the default table, and D = 32 leaves half of a gate item's 16 lanes without channels.
    Bounds, by the rule of tests/test_kernel_parity_f64_gpu.py (kernel_refs.measured_tol): 4 x the error of torch's own fp32 CPU result of
    the same expression on the same inputs against float64, plus the floor the project already uses for that kind of result — 2e-6 for
    elementwise / softmax results (gate, a, c, probabilities), 2e-5 for input gradients that sum a row (dgate: 37 terms, dh: a 64-channel
    product; "ln dx" there).  Parameter gradients are long sums of O(1) terms and take kernel_refs.wgrad_tol: 5e-4 at 531 summed rows,
    growing with sqrt(rows / 531): dW / dbias sum B T nh rows (222 and 600), dconst B T (74 and 300), a bucket of dE the B (T - |d|)
    products of its distances d, counted from the table for the fullest bucket (B T T = 2738 would be the crude count at the small shape:
    1.14e-3).  All inputs are O(1) (randn; gate is in (0, 3))."""
    from dynamic_asr_eval_amd import ops
    B, nh, T, D, nbk, maxd = shape
    H = nh * D
    g = torch.Generator().manual_seed(7)
    h = torch.randn(B, T, H, generator=g)
    W = torch.randn(8, D, generator=g) / 8.0
    bias, const = 0.3 * torch.randn(8, generator=g), 1.0 + 0.3 * torch.randn(nh, generator=g)
    E = torch.randn(nbk, nh, generator=g)
    x = torch.randn(B, nh, T, T, generator=g)
    dS = torch.randn(B, nh, T, T, generator=g)
    dgate_in = torch.randn(B, nh, T, generator=g)
    table = ops.relative_position_buckets(Tmax, nbk, maxd)
    Lv = T if valid is None else valid
    dist = torch.arange(-(T - 1), T)
    fullest = int(torch.zeros(nbk, dtype=torch.long).index_add_(0, table.long()[dist + Tmax - 1], B * (T - dist.abs())).max())

    def run(dt):
        """The whole chain in dtype dt with autograd: forward results and the gradients the two backward entries produce."""
        hh, WW, bb, kk, EE = (t.to(dt).clone().requires_grad_() for t in (h, W, bias, const, E))
        gate, a, c = _gate_ref(hh, WW, bb, kk, nh)
        s = x.to(dt) + _bias_ref(gate.detach(), EE.detach(), table, T, Tmax)
        y = torch.zeros_like(s)
        y[..., :Lv] = torch.softmax(s[..., :Lv], -1)
        gd = gate.detach().clone().requires_grad_()
        (_bias_ref(gd, EE, table, T, Tmax) * dS.to(dt)).sum().backward()               # dyn_relbias_bwd: dgate, dE
        (gate * dgate_in.to(dt)).sum().backward()                                       # dyn_relpos_gate_bwd: dh, dW, dbias, dconst
        return dict(gate=gate, a=a, c=c, y=y, dgate=gd.grad, dE=EE.grad, dh=hh.grad, dW=WW.grad, dbias=bb.grad, dconst=kk.grad)

    r64, r32 = run(torch.float64), run(torch.float32)
    hd, Wd, bd, kd, Ed, xd, dSd, dgd, td = (t.to(cuda) for t in (h, W, bias, const, E, x, dS, dgate_in, table))
    got = {}
    got["gate"], got["a"], got["c"] = ops.relpos_gate(hd, Wd, bd, kd, nh)
    vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
    got["y"] = ops.softmax_relbias(xd, got["gate"], Ed, td, D, valid=vd)
    assert torch.equal(ops.softmax_relbias(xd.clone(), got["gate"], Ed, td, D, out=None, valid=vd), got["y"])
    inplace = xd.clone()
    ops.softmax_relbias(inplace, got["gate"], Ed, td, D, out=inplace, valid=vd)
    assert torch.equal(inplace, got["y"])                                               # the model runs it in place
    if valid is not None:
        assert got["y"][..., Lv:].abs().max().item() == 0.0
    old = dict(dE=torch.full((nbk, nh), 0.75), dW=torch.full((8, D), -1.25), dbias=torch.full((8,), 0.5), dconst=torch.full((nh,), 2.0),
               dh=torch.randn(B, T, H, generator=g))
    for beta in (0.0, 1.0):
        acc = {k: v.to(cuda) for k, v in old.items()}
        got["dgate"] = ops.relbias_bwd(dSd, got["gate"], Ed, td, D, acc["dE"], beta=beta)
        ops.relpos_gate_bwd(dgd, got["a"], got["c"], hd, Wd, kd, acc["dh"], acc["dW"], acc["dbias"], acc["dconst"], dh_beta=beta, beta=beta)
        got.update(acc)
        for name, floor in (("gate", 2e-6), ("a", 2e-6), ("c", 2e-6), ("y", 2e-6), ("dgate", 2e-5), ("dh", 2e-5)):
            want = r64[name] + (beta * old[name].double() if name in old else 0.0)
            tol, e32 = K.measured_tol(r32[name] + (beta * old[name] if name in old else 0.0), want, floor)
            err = K.max_err(got[name], want)
            print(f"  {name} (beta {beta:g}): kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
            assert err <= tol, (name, err, tol)
        for name, rows in (("dE", fullest), ("dW", B * T * nh), ("dbias", B * T * nh), ("dconst", B * T)):
            tol = K.wgrad_tol(5e-4, rows, 531)
            err = K.max_err(got[name], r64[name] + beta * old[name].double())
            print(f"  {name} (beta {beta:g}): kernel {err:.2e} | torch fp32 {K.max_err(r32[name], r64[name]):.2e} | bound {tol:.2e}")
            assert err <= tol, (name, err, tol)


def test_backward_is_bit_reproducible(cuda):
    ref, hip = _pair(cuda, seed=1)
    x = torch.randn(2, 6000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert hip.G[EMBED].abs().max().item() > 0.0


def test_active_subset_backward(cuda):
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(2, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out); gl[0] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:1].contiguous(), n_active=1)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_frozen_prefixes(cuda):
    ref, hip = _pair(cuda, seed=4)
    x = torch.randn(1, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {"wavlm.feature_extractor", "wavlm.encoder.layers.0.attention.gru_rel_pos"}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G["wavlm.feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
    assert hip.G["wavlm.encoder.layers.0.attention.gru_rel_pos_linear.weight"].abs().max().item() == 0.0
    assert hip.G["wavlm.encoder.layers.0.attention.gru_rel_pos_const"].abs().max().item() == 0.0
    assert hip.G["wavlm.encoder.layers.1.attention.gru_rel_pos_linear.weight"].abs().max().item() > 0.0
    assert hip.G[EMBED].abs().max().item() > 0.0
    hip.frozen = set()


def test_dynamic_eval_su_matches_oracle(cuda):
    import argparse
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    # The weights' seed is one at which the ORACLE stays finite: a random model's greedy pseudo-label may hold id 3, which decodes to the text
    # "<unk>" and tokenises back to five ids, more than the frames can emit: CTC loss inf, NaN weights from there on, in transformers as here
    # (seed 5 does that at the second utterance).
    ref, hip = _pair(cuda, seed=6)
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


def test_chunked_dynamic_eval_matches_oracle(cuda):
    import argparse
    import numpy as np
    from oracle.wav2vec2_ref import dynamic_eval_chunked_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    seq_len, overlap, L = 6000, 1280, 15000
    ref, hip = _pair(cuda, seed=8, flags=STABLE_LAYER)       # a seed at which the oracle stays finite, see test_dynamic_eval_su_matches_oracle
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


def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda):
    """One captured launch sequence per length bucket against the unpadded eager run at the bars of the parent's test of the same name (logits
    of the utterance's own frames 2e-5, flat gradient 1e-4 of its largest entry): the bucket table is the BUCKET's (16 / 24 frames), the
    utterance's length the device scalar of the masked softmax; padded query rows and key columns contribute exact zeros to dgate, dE and dh.
    Two lengths in one bucket and one in another, a shorter utterance replayed after a longer one, and a second backward variant (frozen
    extractor) after the bucket's activations were released."""
    ref, hip = _pair(cuda, seed=11)
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
        fz = ("wavlm.feature_extractor",) if k == 4 else ()     # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        assert (lo - lo2).abs().max().item() < 2e-5 * max(1.0, lo2.abs().max().item()), (L, (lo - lo2).abs().max().item())
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        assert hip.G[EMBED].abs().max().item() > 0.0
        if fz:
            assert hip.G["wavlm.feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
            assert hip.G["wavlm.feature_projection.layer_norm.weight"].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


def test_run_wav2vec2_harness_with_a_wavlm_directory(cuda, tmp_path, capsys):
    """`-c DIR` whose config.json says `model_type: wavlm` builds WavLMForCTC and runs; `--config` with that file does too (seeded weights);
    the same weights offered with a wav2vec2 config are refused with an error that names a parameter."""
    from transformers import Wav2Vec2Config, WavLMConfig, WavLMForCTC as HF
    from dynamic_asr_eval_amd import run_wav2vec2 as R, wav2vec2_lib as W
    from dynamic_asr_eval_amd.ops import DynError
    torch.manual_seed(0)
    cfg = WavLMConfig(**TOY, **POST_GROUP, **SMALL_BUCKETS)
    ref = HF(cfg)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    assert '"model_type": "wavlm"' in open(d / "config.json").read()
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
        f.write(Wav2Vec2Config(**TOY, **POST_GROUP).to_json_string(use_diff=False))
    with pytest.raises((KeyError, DynError)) as e:
        R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "--config", str(w2), "-nv"]))
    assert "wav2vec2." in str(e.value)                          # names the first parameter the checkpoint does not have
