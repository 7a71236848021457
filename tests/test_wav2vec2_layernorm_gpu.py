"""The layer-norm / stable-LN wav2vec2 layout (wav2vec2-large-960h-lv60-self, large-robust, XLSR: `feat_extract_norm="layer"`,
`conv_bias=True`, `do_stable_layer_norm=True`) and the two mixed combinations: HIP Wav2Vec2ForCTC against the transformers CPU model
with the same weights — logits, every parameter gradient, the dynamic-eval loops, bucketed hipGraph replay and the harness — at the
bars tests/test_wav2vec2_gpu.py holds the base layout to."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LAYER_STABLE = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32, ctc_loss_reduction="mean")


def _pair(cuda, seed=0, flags=LAYER_STABLE, arch=TOY):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC as HF
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
    torch.manual_seed(seed)
    cfg = Wav2Vec2Config(**arch, **flags)
    ref = HF(cfg).eval()
    with torch.no_grad():   # HF initialises biases / LN to trivial values: randomise so every gradient path is exercised
        for n, p in ref.named_parameters():
            if p.dim() == 1 or "original0" in n:
                p.add_(0.1 * torch.randn_like(p))
    hip = Wav2Vec2ForCTC(cfg, device=cuda)
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
            assert n == "wav2vec2.masked_spec_embed" and grads[n].abs().max().item() == 0.0, n       # unused in eval mode
            continue
        diff = (grads[n].cpu().reshape(p.grad.shape) - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        worst = max(worst, diff / (scale + 1e-12)) if scale > 1e-7 else worst
        assert diff < 3e-3 * scale + 2e-8, (n, diff, scale)
    print("worst relative gradient error", worst)


@pytest.mark.parametrize("flags", [LAYER_STABLE, dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=True),
                                   dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=False)],
                         ids=["layer-stable", "group-stable", "layer-postln"])
def test_forward_backward_matches_transformers(cuda, flags):
    ref, hip = _pair(cuda, flags=flags)
    assert (hip.cfg["feat_extract_norm"], hip.cfg["conv_bias"], hip.cfg["do_stable_layer_norm"]) == \
        (flags["feat_extract_norm"], flags["conv_bias"], flags["do_stable_layer_norm"])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6000, generator=g)
    _forward_and_every_gradient(cuda, ref, hip, x, g, 2e-4)
    sd = hip.state_dict()                                   # state_dict round trip keeps HF names and layouts, bit for bit
    for n, p in ref.named_parameters():
        assert sd[n].shape == p.shape and torch.equal(sd[n].cpu(), p.detach()), n
    assert set(sd) == {n for n, _ in ref.named_parameters()}


def test_wide_shape_forward_and_every_gradient(cuda):
    """The lv60 group width (1024 / 16 = 64 channels per positional-conv group, 16 x 64 heads, FFN 4096) and LayerNorm row widths
    (512 in the extractor, 1024 in the encoder), without its 24 layers."""
    arch = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, conv_dim=(512,) * 7,
                num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, vocab_size=32, ctc_loss_reduction="mean")
    ref, hip = _pair(cuda, arch=arch)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16000, generator=g)
    _forward_and_every_gradient(cuda, ref, hip, x, g, 5e-4)


def test_active_subset_backward(cuda):
    ref, hip = _pair(cuda, seed=3)
    x = torch.randn(2, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out); gl[0] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:1].contiguous(), n_active=1)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def test_dynamic_eval_su_matches_oracle(cuda):
    import argparse
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    ref, hip = _pair(cuda, seed=5)
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
        assert a['probs'].shape == b['probs'].shape
        assert (a['probs'] - b['probs']).abs().max().item() < 1e-3
        assert torch.equal(a['probs'].argmax(-1), b['probs'].argmax(-1))


@pytest.mark.parametrize("seq_len,overlap,epochs,L", [(6000, 0, 1, 15000), (6000, 1280, 1, 15000)])
def test_chunked_dynamic_eval_matches_oracle(cuda, seq_len, overlap, epochs, L):
    import argparse
    import numpy as np
    from oracle.wav2vec2_ref import dynamic_eval_chunked_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    ref, hip = _pair(cuda, seed=7)
    tok = W.CharTokenizer()
    wav = torch.randn(1, L, generator=torch.Generator().manual_seed(L + overlap)) * 0.1 + 0.01
    args = argparse.Namespace(epochs=epochs, shuffle=False)
    before = hip.flat_params.clone()
    np.random.seed(1000 + L)
    want = dynamic_eval_chunked_ref(args, ref, wav, seq_len, overlap, tok, MADGRAD_REF, lr_args={'lr': 1e-5})
    np.random.seed(1000 + L)
    got = W.dynamic_eval(args, hip, wav, seq_len, overlap, tok, None, use_tqdm=False, optim=W.MADGRAD, lr_args={'lr': 1e-5})
    assert torch.equal(hip.flat_params, before)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() < 1e-3 and np.array_equal(got.argmax(-1), want.argmax(-1))


def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda):
    """One captured launch sequence per length bucket, replayed with the utterance's frame counts in HBM, against the unpadded eager run: the
    bars of the base layout's test of the same name (logits of the utterance's own frames 2e-5, flat gradient 1e-4 of its largest entry).
    The padded rows are NOT zero in this layout's forward (conv bias, LayerNorm beta); their gradients are.  Two lengths in one bucket and
    one in another, a shorter utterance replayed after a longer one, and a second backward variant (frozen extractor) after the bucket's
    activations were released."""
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
        fz = ("wav2vec2.feature_extractor",) if k == 4 else ()  # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        assert (lo - lo2).abs().max().item() < 2e-5 * max(1.0, lo2.abs().max().item()), (L, (lo - lo2).abs().max().item())
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        if fz:
            for n in ("conv_layers.0.conv.weight", "conv_layers.0.conv.bias", "conv_layers.6.layer_norm.weight"):
                assert hip.G["wav2vec2.feature_extractor." + n].abs().max().item() == 0.0
            assert hip.G["wav2vec2.feature_projection.layer_norm.weight"].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


def test_run_wav2vec2_harness_with_a_model_directory(cuda, tmp_path, capsys):
    """`-c DIR` (config.json + pytorch_model.bin, as a local HF model directory holds them) builds that architecture and layout and runs; the same
    state dict as a bare `-c FILE` without `--config` is refused (missing / shape error) instead of running at the base layout; `--config` alone
    gives seeded weights at that architecture."""
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC as HF
    from dynamic_asr_eval_amd import run_wav2vec2 as R, wav2vec2_lib as W
    from dynamic_asr_eval_amd.ops import DynError
    torch.manual_seed(0)
    cfg = Wav2Vec2Config(**TOY, **LAYER_STABLE)
    ref = HF(cfg)
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))             # the full HF file: dozens of keys the reader does not know
    torch.save(ref.state_dict(), str(d / "pytorch_model.bin"))
    n_params = sum(p.numel() for p in ref.parameters())
    R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d), "-nv"]))
    out = capsys.readouterr().out
    assert f"Loaded model from {d}" in out and f"Total number of parameters: {n_params / 1e6:.2f}M" in out and "WER: " in out
    with pytest.raises((KeyError, DynError)) as e:
        R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "-nv"]))
    assert "wav2vec2." in str(e.value)                          # names the first parameter that does not fit
    R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "--config", str(d / "config.json"), "-nv"]))
    R.main(W.apply_args(R.build_parser(), ["--mode", "chunked", "--seconds", "6", "--config", str(d / "config.json"), "-seq", "32000", "-nv"]))
    assert capsys.readouterr().out.count(f"Total number of parameters: {n_params / 1e6:.2f}M") == 2
