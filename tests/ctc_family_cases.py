"""What tests/test_data2vec_audio_gpu.py and tests/test_hubert_gpu.py share: the checks tests/test_wav2vec2_conformer_gpu.py holds a model of
the wav2vec2 family to (transformers on the CPU with the same state dict is the oracle), written once over a `pair(cuda, seed=..., **kw)`
-> (transformers model in eval mode, HIP model) factory and the family's parameter prefix.  Not a test module."""
import argparse

import pytest
import torch

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7, vocab_size=32,
           ctc_loss_reduction="mean")
LOGIT_BAR = 2e-4
REPLAY_LENGTHS = [4400, 4000, 6000, 3500, 4400]                 # frames 13, 12, 18, 10, 13 -> buckets 16, 16, 24, 16, 16


def randomise_1d(ref):
    """HF initialises biases / norms to trivial values: randomise so every gradient path is exercised (as tests/test_wavlm_gpu.py::_pair)."""
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1 or "original0" in n:
                p.add_(0.1 * torch.randn_like(p))


def forward_and_every_gradient(cuda, ref, hip, x, g, pf, logit_bar=LOGIT_BAR):
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
    assert {n for n, p in named.items() if p.grad is None} == {pf + "masked_spec_embed"}       # unused in eval mode
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


def state_dict_round_trip(ref, hip):
    sd = hip.state_dict()                                   # HF names and layouts, bit for bit
    assert set(sd) == {n for n, _ in ref.named_parameters()}
    for n, p in ref.named_parameters():
        assert sd[n].shape == p.shape and sd[n].dtype == p.dtype and torch.equal(sd[n].cpu(), p.detach()), n


def backward_is_bit_reproducible(cuda, hip):
    x = torch.randn(2, 6000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = (torch.randn(out.shape, generator=torch.Generator().manual_seed(3)) / out.numel()).to(cuda)
    hip.zero_grad(); hip.backward(gl); first = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl)
    assert torch.equal(hip.flat_grads, first)
    assert first.abs().max().item() > 0.0


def active_subset_backward(cuda, hip):
    x = torch.randn(2, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = hip(x).logits
    gl = torch.zeros_like(out); gl[0] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(3)).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gl); full = hip.flat_grads.clone()
    hip(x); hip.zero_grad(); hip.backward(gl[:1].contiguous(), n_active=1)
    assert (hip.flat_grads - full).abs().max().item() / full.abs().max().item() < 1e-5


def frozen_prefixes(cuda, hip, pf, frozen_prefix, live_name):
    """The extractor and `frozen_prefix` frozen: their gradients are exact zeros, `live_name` and the projection keep theirs."""
    x = torch.randn(1, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {pf + "feature_extractor", frozen_prefix}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[pf + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
    hit = [n for n in hip.G if n.startswith(frozen_prefix)]
    assert len(hit) >= 2 and not live_name.startswith(frozen_prefix)
    for n in hit:
        assert hip.G[n].abs().max().item() == 0.0, n
    assert hip.G[live_name].abs().max().item() > 0.0
    assert hip.G[pf + "feature_projection.projection.weight"].abs().max().item() > 0.0
    hip.frozen = set()


def bucketed_graph_replay(cuda, hip, pf, live_name):
    """The protocol and bars of tests/test_wavlm_gpu.py's test of the same name (logits of the utterance's own frames 2e-5, flat gradient 1e-4
    of its largest entry): two lengths in one bucket and one in another, a shorter utterance replayed after a longer one, and a second backward
    variant (frozen extractor) after the bucket's activations were released.  Returns the largest logits error seen."""
    hip.graph_after, hip.bucket_frames = 1, 8
    worst = 0.0

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

    assert [hip.conv_lengths(L)[-1] for L in REPLAY_LENGTHS] == [13, 12, 18, 10, 13]
    for k, L in enumerate(REPLAY_LENGTHS):
        fz = (pf + "feature_extractor",) if k == 4 else ()      # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        err = (lo - lo2).abs().max().item()
        worst = max(worst, err)
        print(f"L {L}: logits error against the unpadded eager run {err:.2e}")
        assert err < 2e-5 * max(1.0, lo2.abs().max().item()), (L, err)
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        assert hip.G[live_name].abs().max().item() > 0.0
        if fz:
            assert hip.G[pf + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
            assert hip.G[pf + "feature_projection.projection.weight"].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()
    return worst


def dynamic_eval_su_matches_oracle(cuda, ref, hip):
    """The weights' seed is one at which the ORACLE stays finite: a random model's greedy pseudo-label may hold id 3, which decodes to the
    text "<unk>" and tokenises back to five ids, more than the frames can emit: CTC loss inf, NaN weights from there on."""
    from oracle.wav2vec2_ref import dynamic_eval_su_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
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


def chunked_dynamic_eval_matches_oracle(cuda, ref, hip):
    import numpy as np
    from oracle.wav2vec2_ref import dynamic_eval_chunked_ref
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import wav2vec2_lib as W
    seq_len, overlap, L = 6000, 1280, 15000
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


def harness_with_a_directory(tmp_path, capsys, cfg, ref, model_type, wav2vec2_keys):
    """`-c DIR` whose config.json (as transformers writes it) names `model_type` builds that model and runs; `--config` with that file does too
    (seeded weights); the same weights offered with a wav2vec2 config are refused with an error that names a parameter."""
    from transformers import Wav2Vec2Config
    from dynamic_asr_eval_amd import run_wav2vec2 as R, wav2vec2_lib as W
    from dynamic_asr_eval_amd.ops import DynError
    d = tmp_path / "model"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        f.write(cfg.to_json_string(use_diff=False))
    assert f'"model_type": "{model_type}"' in open(d / "config.json").read()
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
        f.write(Wav2Vec2Config(**wav2vec2_keys).to_json_string(use_diff=False))
    with pytest.raises((KeyError, DynError)) as e:
        R.main(W.apply_args(R.build_parser(), ["--mode", "su", "--seconds", "6", "-c", str(d / "pytorch_model.bin"), "--config", str(w2), "-nv"]))
    assert "wav2vec2." in str(e.value)                          # names the first parameter the checkpoint does not have
