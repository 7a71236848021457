"""Wav2Vec2BertForCTC (wav2vec2_bert_model.py: filter-bank front end, narrow feature-projection LayerNorm, conformer layers with the causal
LayerNormed conv module and relative-key attention on the disentangled kernels) against transformers' Wav2Vec2BertForCTC on the CPU with
the same random state dict: logits and every parameter gradient from `input_features`, the state dict, active-subset and frozen
backwards, bucketed hipGraph replay from waveforms, both dynamic-eval loops against the oracle and the harness, at the bars
tests/test_wav2vec2_conformer_gpu.py holds the conformer to.  No hub checkpoint is on the machine."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wav2vec2_bert_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, vocab_size=32, ctc_loss_reduction="mean")
WIDE = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, vocab_size=32, ctc_loss_reduction="mean")
PF = "wav2vec2_bert."
UNUSED = {PF + "masked_spec_embed"}
DIST = PF + "encoder.layers.{}.self_attn.distance_embedding.weight"
DW = PF + "encoder.layers.{}.conv_module.depthwise_conv.weight"
# Weights' seeds at which the ORACLE stays finite: a random model's greedy pseudo-label may hold id 3, which decodes to "<unk>" and tokenises back
# to five ids, more than the frames can emit: CTC loss inf, NaN weights from there on, in transformers as here (see the conformer's loop tests).
SU_SEED, CHUNKED_SEED = 2, 3


def _pair(cuda, seed=0, arch=TOY, **over):
    from transformers import Wav2Vec2BertConfig, Wav2Vec2BertForCTC as HF
    from dynamic_asr_eval_amd.wav2vec2_bert_model import Wav2Vec2BertForCTC
    torch.manual_seed(seed)
    cfg = Wav2Vec2BertConfig(**dict(arch, **over))
    ref = HF(cfg).eval()
    with torch.no_grad():   # HF initialises biases and norms to trivial values: randomise so every path is exercised
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    hip = Wav2Vec2BertForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


class WaveformModel(torch.nn.Module):
    """What the oracle's loops drive: a normalised waveform [B, L] through SeamlessM4TFeatureExtractor (valid rows only; the rows of a batch
    share one length) into transformers' model."""

    def __init__(self, hf):
        super().__init__()
        self.hf = hf

    def forward(self, input_values):
        feats = []
        for row in input_values.detach():
            f, valid = R.extractor_rows(row)
            feats.append(torch.from_numpy(f[:valid]))
        return self.hf(torch.stack(feats))


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
    assert {n for n, p in named.items() if p.grad is None} == UNUSED       # built by transformers, never used in an eval forward
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
    sd, want = hip.state_dict(), ref.state_dict()           # HF names and layouts, bit for bit; this model has no buffers
    assert set(sd) == set(want) == {n for n, _ in ref.named_parameters()}
    for n, t in want.items():
        assert sd[n].shape == t.shape and sd[n].dtype == t.dtype and torch.equal(sd[n].cpu(), t), n
    assert hip.buffers_ == {}


@pytest.mark.parametrize("T,over", [(18, {}), (93, {}), (19, dict(left_max_position_embeddings=5, right_max_position_embeddings=3)),
                                    (18, dict(hidden_act="gelu")), (18, dict(layer_norm_eps=1e-3))],
                         ids=["T18", "T93", "left5-right3-T19", "gelu", "eps1e-3"])
def test_forward_backward_matches_transformers(cuda, T, over):
    """T = 18: every frame inside the 31-tap left halo, and left = 64 is never reached, so dC2P has empty segments; T = 93: interior frames,
    both clips of the default table active (93 > 64), a second row block of the score kernels; left 5 / right 3 at T = 19: both clips on a
    short table; `layer_norm_eps=1e-3` must reach EVERY norm (applied to some only, the logits leave the bar)."""
    ref, hip = _pair(cuda, **over)
    assert hip.cfg["hidden_act"] == over.get("hidden_act", "swish") and hip.cfg["layer_norm_eps"] == over.get("layer_norm_eps", 1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, T, 160, generator=g)
    grads, named = _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    for l in range(2):
        assert grads[DIST.format(l)].abs().max().item() > 0.0 and grads[DW.format(l)].abs().max().item() > 0.0
        if T == 18 and not over.get("left_max_position_embeddings"):      # rows of E no pair of 18 frames selects: exact zeros on both sides
            far = grads[DIST.format(l)][:64 - 17]
            assert far.abs().max().item() == 0.0 and named[DIST.format(l)].grad[:64 - 17].abs().max().item() == 0.0
    _state_dict_round_trip(ref, hip)


def test_wide_shape_forward_and_every_gradient(cuda):
    """The published widths (1024 hidden, 16 x 64 heads, FFN 4096) without the 24 layers."""
    ref, hip = _pair(cuda, arch=WIDE)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 49, 160, generator=g)
    _forward_and_every_gradient(cuda, ref, hip, x, g, 5e-4)


def test_backward_is_bit_reproducible(cuda):
    ref, hip = _pair(cuda, seed=1)
    x = torch.randn(2, 37, 160, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert first.abs().max().item() > 0.0


def test_active_subset_backward(cuda):
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(2, 15, 160, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out); gl[0] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:1].contiguous(), n_active=1)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_frozen_prefixes(cuda):
    ref, hip = _pair(cuda, seed=4)
    x = torch.randn(1, 15, 160, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {PF + "feature_projection", PF + "masked_spec_embed", PF + "encoder.layers.0.self_attn.distance_embedding",
                  PF + "encoder.layers.0.conv_module.depthwise_conv"}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[PF + "feature_projection.projection.weight"].abs().max().item() == 0.0
    assert hip.G[PF + "feature_projection.layer_norm.weight"].abs().max().item() == 0.0
    for n in (DIST, DW):
        assert hip.G[n.format(0)].abs().max().item() == 0.0, n
        assert hip.G[n.format(1)].abs().max().item() > 0.0, n
    assert hip.G[PF + "encoder.layers.0.self_attn.linear_q.weight"].abs().max().item() > 0.0
    hip.frozen = {PF + "feature_projection.layer_norm"}                    # the projection adapts, its LayerNorm does not
    hip(x); hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[PF + "feature_projection.projection.weight"].abs().max().item() > 0.0
    assert hip.G[PF + "feature_projection.layer_norm.weight"].abs().max().item() == 0.0
    hip.frozen = set()


def test_waveform_input_matches_transformers_behind_its_extractor(cuda):
    """A waveform goes through the device front end; transformers gets the extractor's features of the same waveform.  Bars of the
    feature-input test (the front end's 1e-5 distance from the extractor, wav2vec2_bert_refs.py, is inside them)."""
    ref, hip = _pair(cuda, seed=2)
    L = 6000
    x = torch.randn(2, L, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = WaveformModel(ref)(x).logits
        got = hip(x.to(cuda))
    assert got.frames == want.shape[1] == hip.conv_lengths(L)[-1] == 18
    err = (got.logits.cpu() - want).abs().max().item()
    print("waveform forward err", err)
    assert err < 2e-4, err
    with pytest.raises(Exception) as e:
        hip(torch.zeros(1, 559, device=cuda))
    assert "559 samples" in str(e.value)


def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda):
    """The protocol and bars of tests/test_wav2vec2_conformer_gpu.py's test of the same name (logits of the utterance's own frames 2e-5, flat
    gradient 1e-4 of its largest entry), from waveforms.  Buckets of 8 frames: two lengths in one bucket and one in another, a shorter
    utterance replayed after a longer one, and a second backward variant (frozen feature projection) after the bucket's activations were
    released.  The causal conv module runs WITHOUT the conformer's mask_rows pair (wav2vec2_bert_model.py argues why): this test decides."""
    ref, hip = _pair(cuda, seed=11)
    hip.graph_after, hip.bucket_frames = 1, 8
    # frames 13, 12, 18, 10, 13 -> buckets 16, 16, 24, 16, 16; 560 + 320 (t - 1) samples give 2 t filter-bank frames, + 160 an odd one more
    lengths = [560 + 320 * (t - 1) + d for t, d in ((13, 57), (12, 0), (18, 319), (10, 160), (13, 57))]

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
        fz = (PF + "feature_projection",) if k == 4 else ()     # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        assert (lo - lo2).abs().max().item() < 2e-5 * max(1.0, lo2.abs().max().item()), (L, (lo - lo2).abs().max().item())
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        assert hip.G[DW.format(0)].abs().max().item() > 0.0 and hip.G[DIST.format(0)].abs().max().item() > 0.0
        if fz:
            assert hip.G[PF + "feature_projection.projection.weight"].abs().max().item() == 0.0
        else:
            assert hip.G[PF + "feature_projection.layer_norm.weight"].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


def test_dynamic_eval_su_matches_oracle(cuda):
    import argparse
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    # The weights' seed is one at which the ORACLE stays finite (see tests/test_wav2vec2_conformer_gpu.py's test of the same name).
    ref, hip = _pair(cuda, seed=SU_SEED)
    tok = W.CharTokenizer()
    g = torch.Generator().manual_seed(9)
    utts_ref = [{'waveform': torch.randn(1, n, generator=g) * 0.1 + 0.01} for n in (4000, 7000, 5200)]
    utts = [{'waveform': u['waveform'].clone()} for u in utts_ref]
    args = argparse.Namespace(epochs=1, shuffle=False)
    before = hip.flat_params.clone()
    dynamic_eval_su_ref(args, WaveformModel(ref), utts_ref, tok, MADGRAD_REF, lr_args={'lr': 1e-5})
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
    ref, hip = _pair(cuda, seed=CHUNKED_SEED)                  # a seed at which the oracle stays finite
    tok = W.CharTokenizer()
    wav = torch.randn(1, L, generator=torch.Generator().manual_seed(L + overlap)) * 0.1 + 0.01
    args = argparse.Namespace(epochs=1, shuffle=False)
    before = hip.flat_params.clone()
    np.random.seed(1000 + L)
    want = dynamic_eval_chunked_ref(args, WaveformModel(ref), wav, seq_len, overlap, tok, MADGRAD_REF, lr_args={'lr': 1e-5})
    np.random.seed(1000 + L)
    got = W.dynamic_eval(args, hip, wav, seq_len, overlap, tok, None, use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-5})
    assert torch.equal(hip.flat_params, before)
    assert got.shape == want.shape and np.isfinite(want).all(), (got.shape, want.shape)
    assert np.abs(got - want).max() < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))



def test_run_wav2vec2_harness_with_a_wav2vec2_bert_directory(cuda, tmp_path, capsys):
    """`-c DIR` whose config.json says `model_type: wav2vec2-bert` builds Wav2Vec2BertForCTC and runs; `--config` with that file does too
    (seeded weights); the same weights offered with a wav2vec2 config are refused with an error that names a parameter."""
    from transformers import Wav2Vec2BertConfig, Wav2Vec2BertForCTC as HF, Wav2Vec2Config
    from dynamic_asr_eval_amd import run_wav2vec2 as RUN, wav2vec2_lib as W
    from dynamic_asr_eval_amd.ops import DynError
    torch.manual_seed(0)
    cfg = Wav2Vec2BertConfig(**TOY)
    ref = HF(cfg)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    assert '"model_type": "wav2vec2-bert"' in open(d / "config.json").read()
    torch.save(ref.state_dict(), str(d / "pytorch_model.bin"))
    n_params = sum(p.numel() for p in ref.parameters())
    RUN.main(W.apply_args(RUN.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d), "-nv"]))
    out = capsys.readouterr().out
    assert f"Loaded model from {d}" in out and f"Total number of parameters: {n_params / 1e6:.2f}M" in out and "WER: " in out
    RUN.main(W.apply_args(RUN.build_parser(), ["--mode", "su", "--seconds", "6", "--config", str(d / "config.json"), "-nv"]))
    out = capsys.readouterr().out
    assert f"Total number of parameters: {n_params / 1e6:.2f}M" in out and "WER: " in out
    w2 = tmp_path / "w2.json"
    with open(w2, "w") as f:
        f.write(Wav2Vec2Config(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, vocab_size=32, conv_dim=(256,) * 7,
                               num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4).to_json_string(use_diff=False))
    with pytest.raises((KeyError, DynError)) as e:
        RUN.main(W.apply_args(RUN.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "--config", str(w2), "-nv"]))
    assert "wav2vec2." in str(e.value)                          # names the first parameter the checkpoint does not have
