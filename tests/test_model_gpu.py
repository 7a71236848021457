"""Model-level and loop-level parity on the GPU: the HIP SCConformerXL (forward, backward, adaptation step, dynamic
eval) against the CPU oracle (oracle/conformer_ref.py, oracle/dynamic_eval_ref.py) with the SAME seeded weights,
inputs and SpecAugment masks.  Bars from BASELINE.json: CTC argmax token ids bit-exact, adapted logits within 1e-3."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(n_layers=2, d_model=256, n_heads=2, head_dim=128, subsampling_conv_channels=64)


def _pair(cuda, cfg, vocab, seed=3, blank_bias=0.0):
    from oracle.conformer_ref import SCConformerXLRef
    from dynamic_asr_eval_amd.model import SCConformerXL
    ref = SCConformerXLRef(cfg, vocab_size=vocab, seed=seed, blank_bias=blank_bias)
    hip = SCConformerXL(cfg, vocab_size=vocab, device=cuda)
    assert [n for n, _ in ref.named_parameters()] == [n for n, _ in hip.named_parameters()]
    hip.load_state_dict(ref.state_dict())
    return ref, hip


@pytest.mark.parametrize("cfg_over,T", [({}, 256), (dict(conv_norm="layer_norm"), 200), (dict(self_conditioning=False), 77)])
def test_forward_backward_parity(cuda, cfg_over, T):
    cfg = dict(SMALL, **cfg_over)
    ref, hip = _pair(cuda, cfg, vocab=128)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 80, T, generator=g)
    out_ref = ref(audio_signal=x)['final_posteriors']
    out = hip(audio_signal=x.to(cuda))['final_posteriors']
    assert out.shape == out_ref.shape
    err = (out.cpu() - out_ref).abs().max().item()
    assert err < 2e-4, f"forward log-probs differ by {err}"          # fp32 vs fp32, different summation orders
    assert torch.equal(out.cpu().argmax(-1), out_ref.argmax(-1))       # argmax ids bit-exact
    gp = torch.randn(out_ref.shape, generator=g) / out_ref.numel()
    out_ref.backward(gp)
    hip.zero_grad()
    hip.backward(gp.to(cuda))
    worst = 0.0
    for (n, p), gh in zip(ref.named_parameters(), hip.grads()):
        denom = p.grad.abs().max().item() + 1e-12
        rel = (gh.cpu() - p.grad).abs().max().item() / denom
        worst = max(worst, rel)
        assert rel < 2e-3, f"grad {n}: rel err {rel}"
    print("worst relative grad error", worst)


def test_fused_grad_attention_forward_backward_parity(cuda):
    """The whole model with the streaming grad-mode attention (no [B, H, T', T'] scores; forward keeps lse, backward re-forms P):
    log-probs and every parameter gradient vs the CPU oracle, and the n_active backward shortcut on top of it."""
    ref, hip = _pair(cuda, SMALL, vocab=128)
    hip.fused_attention_grad = "1"
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 80, 300, generator=g)
    out_ref = ref(audio_signal=x)['final_posteriors']
    out = hip(audio_signal=x.to(cuda))['final_posteriors']
    assert (out.cpu() - out_ref).abs().max().item() < 2e-4 and torch.equal(out.cpu().argmax(-1), out_ref.argmax(-1))
    gp = torch.zeros(out_ref.shape)
    gp[0] = torch.randn(out_ref.shape[1:], generator=g) / out_ref[0].numel()
    out_ref.backward(gp)
    hip.zero_grad()
    hip.backward(gp[:1].contiguous().to(cuda), n_active=1)
    for (n, p), gh in zip(ref.named_parameters(), hip.grads()):
        rel = (gh.cpu() - p.grad).abs().max().item() / (p.grad.abs().max().item() + 1e-12)
        assert rel < 2e-3, f"grad {n}: rel err {rel}"


def test_backward_active_subset_matches_full(cuda):
    """Skipping the clean copy (zero gradient) must give the same parameter gradients as the full backward."""
    ref, hip = _pair(cuda, SMALL, vocab=128)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 80, 160, generator=g).to(cuda)
    out = hip(audio_signal=x)['final_posteriors']
    gp = torch.zeros_like(out)
    gp[0] = torch.randn(out.shape[1:], generator=g).to(cuda) / out[0].numel()
    hip.zero_grad(); hip.backward(gp)
    full = hip.flat_grads.clone()
    hip(audio_signal=x)
    hip.zero_grad(); hip.backward(gp[:1].contiguous(), n_active=1)
    denom = full.abs().max().item()
    assert (hip.flat_grads - full).abs().max().item() / denom < 1e-5


def _args(**kw):
    a = argparse.Namespace()
    a.config = {'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 16384, 'overlap': 0}, 'training': {}}
    a.__dict__.update(kw)
    return a


def _masks_for(keys, F, u_lens, seed):
    from oracle.dynamic_eval_ref import draw_masks
    g = torch.Generator().manual_seed(seed)
    return {k: (draw_masks(3, 12, F, g), ([], [])) for k in keys}


@pytest.mark.parametrize("online,optim_name", [(True, "madgrad"), (False, "madgrad"), (False, "adam")])
def test_dynamic_eval_parity(cuda, online, optim_name):
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    vocab = 128
    ref, hip = _pair(cuda, SMALL, vocab=vocab, seed=5, blank_bias=1.5)
    tok = SyntheticTokenizer(vocab)
    g = torch.Generator().manual_seed(11)
    spec = torch.randn(1, 80, 1500, generator=g)
    seq_len, overlap = 512, 256
    _, keys = R.prepare_chunks(spec, seq_len, overlap)
    masks = _masks_for(keys, 80, None, seed=2)
    lr = 1e-4
    if optim_name == "madgrad":
        ref_opt, hip_opt, lr_args = MADGRAD_REF, lib.MADGRAD, {'lr': lr}
    else:
        ref_opt, hip_opt, lr_args = torch.optim.Adam, lib.Adam, {'lr': lr}
    before = hip.flat_params.clone()
    out_ref, params_ref = R.dynamic_eval_ref(ref, spec, seq_len, overlap, tok, ref_opt, lr_args, {}, epochs=1, shuffle=False,
                                             online=online, fixed_masks=masks, return_params=True)
    args = _args(optim_lr=lr, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks, quiet=True)
    out, params = lib.dynamic_eval(args, hip, spec, seq_len, overlap, tok, use_tqdm=False, optim=hip_opt, return_params=True)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == out_ref.shape
    assert torch.equal(hip.flat_params, before), "weights must be restored (reference lib.py:636-637)"
    err = np.abs(out - out_ref).max()
    assert err < 1e-3, f"adapted, stitched log-probs differ by {err} (bar: 1e-3 fp32)"
    assert np.array_equal(out.argmax(-1), out_ref.argmax(-1)), "CTC argmax ids must be bit-exact"
    # the adaptation really moved the weights, and by the same amount on both sides
    moved = max((a - b).abs().max().item() for a, b in zip(params_ref, [p.detach() for p in ref.parameters()]))
    assert moved > 1e-6
    for a, b in zip(params, params_ref):
        assert (a - b).abs().max().item() < 5e-5


class _RecordingTokenizer:
    """The reference's own 128-piece SentencePiece model (tests/golden/tokenizer_128.model) with the target lengths of every
    encode() recorded: the text hop ids -> text -> ids of reference lcasr/lib.py:565-569 with a real tokenizer."""

    def __init__(self):
        import os
        from dynamic_asr_eval_amd.tokenizer import load_sentencepiece
        self.sp = load_sentencepiece(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_128.model"))
        self.lengths = []

    def vocab_size(self):
        return self.sp.vocab_size()

    def decode(self, ids):
        return self.sp.decode([int(i) for i in ids])

    def encode(self, text):
        ids = self.sp.encode(text)
        self.lengths.append(len(ids))
        return ids


def test_dynamic_eval_with_the_128_piece_tokenizer_reaches_the_wide_ctc_lattices(cuda):
    """The loop itself at lattice widths L = 2 S + 1 > 1024 and > 2048: with the reference's tokenizer a 164 s window of a model
    that emits a token every other frame carries ~1000 pseudo-label ids (1030 -> ctc_scan_kernel<4>, 1002 -> <2>), the 82 s tail
    window ~500; the stitched, adapted log-probs must match the oracle loop (torch.nn.CTCLoss on the CPU)."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=5, blank_bias=0.0)
    spec = torch.randn(1, 80, 16384 + 8192, generator=torch.Generator().manual_seed(3))
    seq_len, overlap = 16384, 8192
    _, keys = R.prepare_chunks(spec, seq_len, overlap)
    assert len(keys) == 3
    masks = _masks_for(keys, 80, None, seed=4)
    tok_ref, tok_hip = _RecordingTokenizer(), _RecordingTokenizer()
    out_ref = R.dynamic_eval_ref(ref, spec, seq_len, overlap, tok_ref, MADGRAD_REF, {'lr': 2e-6}, {}, epochs=1, shuffle=False,
                                 online=False, fixed_masks=masks)
    args = _args(optim_lr=2e-6, epochs=1, shuffle=False, online=False, spec_augment_fixed_masks=masks, quiet=True)
    out = lib.dynamic_eval(args, hip, spec, seq_len, overlap, tok_hip, use_tqdm=False)
    assert tok_hip.lengths == tok_ref.lengths, (tok_hip.lengths, tok_ref.lengths)
    # S in [512, 1023] -> L in (1024, 2048] -> ctc_scan_kernel<2>; S in [1024, 2047] -> ctc_scan_kernel<4>   (seeded: [1030, 1002, 510])
    assert any(1024 <= n <= 2047 for n in tok_hip.lengths) and any(512 <= n <= 1023 for n in tok_hip.lengths), \
        f"pseudo-label lengths {tok_hip.lengths}: expected one window in [512, 1023] and one in [1024, 2047]"
    err = np.abs(out - out_ref).max()
    assert out.shape == out_ref.shape and err < 1e-3, f"adapted, stitched log-probs differ by {err} (bar: 1e-3 fp32)"
    # argmax ids bit-exact, except at frames whose top-2 margin IN THE ORACLE is below 5e-5 (under the fp32 summation-order noise of
    # either side: this seeded 129-class model emits near-uniform posteriors, margins of 1e-5 occur among its 3072 frames)
    bad = out.argmax(-1) != out_ref.argmax(-1)
    top2 = np.sort(out_ref, -1)[:, -2:]
    assert not (bad & ((top2[:, 1] - top2[:, 0]) >= 5e-5)).any(), "CTC argmax ids differ away from a near-tie"
    assert int(bad.sum()) <= 3, f"{int(bad.sum())} near-tie frames differ"


def test_dynamic_eval_short_recording_and_epochs0(cuda):
    """spec_n <= seq_len -> single window; epochs=0 -> plain forward + stitch (the no-adapt baseline path)."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=7, blank_bias=1.0)
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 300, generator=torch.Generator().manual_seed(4))
    out_ref = R.dynamic_eval_ref(ref, spec, 512, 256, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=0)
    out = lib.dynamic_eval(_args(epochs=0, quiet=True), hip, spec, 512, 256, tok, use_tqdm=False)
    assert out.shape == out_ref.shape
    assert np.abs(out - out_ref).max() < 2e-4
    assert np.array_equal(out.argmax(-1), out_ref.argmax(-1))


def test_awmc_parity(cuda):
    """AWMC (reference lcasr/lib.py:206-376) on the HIP path vs the CPU oracle: 2 epochs so the leader EMA moves."""
    from oracle.awmc_ref import awmc_ref
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=9, blank_bias=1.5)
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 1100, generator=torch.Generator().manual_seed(21))
    seq_len, overlap = 512, 256
    _, keys = R.prepare_chunks(spec, seq_len, overlap)
    masks = _masks_for(keys, 80, None, seed=4)
    before = hip.flat_params.clone()
    out_ref, p_ref = awmc_ref(ref, spec, seq_len, overlap, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=2, ema_decay=0.999,
                              fixed_masks=masks, return_params=True)
    args = _args(optim_lr=1e-4, epochs=2, ema_decay=0.999, spec_augment_fixed_masks=masks, quiet=True)
    out, p = lib.AWMC(args, hip, spec, seq_len, overlap, tok, use_tqdm=False, return_params=True)
    assert torch.equal(hip.flat_params, before)
    assert out.shape == out_ref.shape and np.abs(out - out_ref).max() < 1e-3
    assert np.array_equal(out.argmax(-1), out_ref.argmax(-1))
    for a, b in zip(p, p_ref):
        assert (a - b).abs().max().item() < 5e-5


def test_awmc_bitfit_parity(cuda):
    """`-kwargs bitfit=True` (reference lcasr/lib.py:148-160,234-235): only norm / linear biases move; every other parameter
    comes back bit-identical, and the moved ones match the oracle."""
    from oracle.awmc_ref import awmc_ref
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    cfg = dict(SMALL, conv_norm="layer_norm")
    ref, hip = _pair(cuda, cfg, vocab=128, seed=19, blank_bias=1.5)
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 900, generator=torch.Generator().manual_seed(23))
    _, keys = R.prepare_chunks(spec, 512, 256)
    masks = _masks_for(keys, 80, None, seed=8)
    before = {n: p.clone() for n, p in hip.named_parameters()}
    out_ref, p_ref = awmc_ref(ref, spec, 512, 256, tok, MADGRAD_REF, {'lr': 1e-3}, {}, epochs=1, fixed_masks=masks, return_params=True, bitfit=True)
    args = _args(optim_lr=1e-3, epochs=1, bitfit=True, spec_augment_fixed_masks=masks, quiet=True)
    out, p = lib.AWMC(args, hip, spec, 512, 256, tok, use_tqdm=False, return_params=True)
    assert hip.frozen == set() and all(torch.equal(q, before[n]) for n, q in hip.named_parameters())
    assert out.shape == out_ref.shape and np.abs(out - out_ref).max() < 1e-3 and np.array_equal(out.argmax(-1), out_ref.argmax(-1))
    moved = 0
    for (n, _), a, b in zip(hip.named_parameters(), p, p_ref):
        assert (a - b).abs().max().item() < 5e-5, n
        changed = not torch.equal(a, before[n].cpu())
        is_bitfit_bias = n.endswith(".bias") and ("norm" in n.split(".")[-2] or n.endswith(("qkv.bias", "attn.out.bias", "subsampling.out.bias",
                                                                                                 "decoder.ff.bias", "decoder.reproj.bias")))
        assert changed == is_bitfit_bias or (is_bitfit_bias and not changed and a.abs().max() == 0), (n, changed)
        moved += changed
    assert moved >= 10


def test_chains_replicas_carry_buffers_and_frozen_set(cuda):
    """run_seq_eval.replicate(): the replicas of a batch_renorm model must carry its running statistics (they live outside
    flat_params) and its frozen set; two recordings in flight then reproduce the one-at-a-time outputs bit for bit."""
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.run_seq_eval import replicate
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    cfg = dict(SMALL, conv_norm="batch_renorm")
    ref, hip = _pair(cuda, cfg, vocab=128, seed=4, blank_bias=1.5)
    g = torch.Generator().manual_seed(77)
    for n in hip.buffers:
        hip.buffers[n].copy_((torch.rand(hip.buffers[n].shape, generator=g) * (2.0 if n.endswith("var") else 0.6) + (0.5 if n.endswith("var") else -0.3)).to(cuda))
    hip.frozen = {"subsampling."}
    models = replicate(hip, 2)
    assert all(torch.equal(models[1].buffers[n], hip.buffers[n]) for n in hip.buffers) and models[1].frozen == hip.frozen
    tok = SyntheticTokenizer(128)
    specs = [torch.randn(1, 80, n, generator=g) for n in (1100, 900)]
    args = _args(optim_lr=1e-4, epochs=1, quiet=True, spec_augment_n_freq_masks=0)
    one = [lib.dynamic_eval(args, hip, sp, 512, 256, tok, use_tqdm=False) for sp in specs]
    two = lib.dynamic_eval_many(args, models, specs, 512, 256, tok, use_tqdm=False)
    assert all(np.array_equal(a, b) for a, b in zip(one, two))
    hip.frozen = set()


@pytest.mark.parametrize("epochs", [2, 3])
def test_online_mode_with_several_epochs_stitches_the_last_one(cuda, epochs):
    """online=True with epochs > 1: the reference's loop still runs range(args.epochs) (lcasr/lib.py:527; only the printed count is
    forced to 1, :515) and every epoch overwrites model_outputs[i] (:583-589), so the weights adapt over all epochs and the LAST
    epoch's posteriors are stitched: the output must neither double in length nor overflow the accumulator."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=15, blank_bias=1.5)
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 1100, generator=torch.Generator().manual_seed(5))
    _, keys = R.prepare_chunks(spec, 512, 256)
    masks = _masks_for(keys, 80, None, seed=2)
    out_ref = R.dynamic_eval_ref(ref, spec, 512, 256, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=epochs, online=True, fixed_masks=masks)
    args = _args(optim_lr=1e-4, epochs=epochs, online=True, spec_augment_fixed_masks=masks, quiet=True)
    out = lib.dynamic_eval(args, hip, spec, 512, 256, tok, use_tqdm=False)
    assert out.shape == out_ref.shape and np.abs(out - out_ref).max() < 1e-3 and np.array_equal(out.argmax(-1), out_ref.argmax(-1))


def test_adapt_on_concat_only_matches_loop_a(cuda):
    """run_half_concat_eval.adapt_on_concat_only (reference :64-160) = Loop A of dynamic eval on the concatenation."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd.run_half_concat_eval import adapt_on_concat_only, concatenate_specs
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=13, blank_bias=1.5)
    tok = SyntheticTokenizer(128)
    g = torch.Generator().manual_seed(31)
    specs = [torch.randn(1, 80, n, generator=g) for n in (700, 500, 300)]
    concat = concatenate_specs(specs)
    _, keys = R.prepare_chunks(concat, 512, 256)
    masks = _masks_for(keys, 80, None, seed=6)
    _, p_ref = R.dynamic_eval_ref(ref, concat, 512, 256, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=1, fixed_masks=masks,
                                  return_params=True)
    args = _args(optim_lr=1e-4, epochs=1, shuffle=False, seq_len=512, awmc=False, spec_augment_fixed_masks=masks, quiet=True)
    before = hip.flat_params.clone()
    p = adapt_on_concat_only(args, hip, concat, tok, adapt_overlap=256)
    assert torch.equal(hip.flat_params, before)
    for a, b in zip(p, p_ref):
        assert (a - b).abs().max().item() < 5e-5
    with pytest.raises(ValueError):
        concatenate_specs([])


def test_entropy_augmentation_matches_autograd(cuda):
    """reference lcasr/lib.py:86-99: spec + 0.001 * d mean-entropy / d spec, computed by torch autograd on the oracle."""
    from dynamic_asr_eval_amd import lib
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=17)
    spec = torch.randn(1, 80, 200, generator=torch.Generator().manual_seed(5))
    audio = spec.clone().requires_grad_()
    lp = ref(audio_signal=audio)['final_posteriors']
    entropy = torch.distributions.Categorical(probs=lp.exp()).entropy()
    grad = torch.autograd.grad(outputs=entropy.mean(), inputs=audio, create_graph=False)[0] * 0.001
    expect = (audio + grad).detach()
    got = lib.entropy_augmentation(spec.to(cuda).clone(), hip, enabled=True)
    delta_ref = (expect - spec)
    delta = (got.cpu() - spec)
    assert delta_ref.abs().max() > 0
    rel = (delta - delta_ref).abs().max().item() / delta_ref.abs().max().item()
    assert rel < 2e-3, rel
    assert torch.equal(lib.entropy_augmentation(spec.to(cuda), hip, enabled=False).cpu(), spec)


@pytest.mark.parametrize("conv_norm", ["rms_norm", "layer_norm"])
def test_fused_convmod_matches_unfused(cuda, conv_norm):
    """csrc/convmod.hip (GLU + dwconv k=9 + norm + SiLU in one pass) vs the four separate kernels, forward and backward."""
    cfg = dict(SMALL, conv_norm=conv_norm)
    ref, hip = _pair(cuda, cfg, vocab=128, seed=23)
    x = torch.randn(2, 80, 333, generator=torch.Generator().manual_seed(8)).to(cuda)
    outs, grads = [], []
    for fused in (True, False):
        hip.fused_convmod = fused
        out = hip(audio_signal=x)['final_posteriors']
        gp = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(cuda) / out.numel()
        hip.zero_grad(); hip.backward(gp)
        outs.append(out.clone()); grads.append(hip.flat_grads.clone())
    assert (outs[0] - outs[1]).abs().max().item() < 2e-5
    assert (grads[0] - grads[1]).abs().max().item() / grads[1].abs().max().item() < 1e-4
    with torch.no_grad():
        hip.fused_convmod = True
        a = hip(audio_signal=x)['final_posteriors']
    assert (a - outs[0]).abs().max().item() < 1e-6


def test_chains_and_graphs_are_bit_identical_to_the_sequential_eager_loop(cuda):
    """dynamic_eval_many (recordings interleaved on several streams, hipGraph replay of the encoder) launches the same
    kernels with the same plans as one eager recording after another: results must be bit-identical, every replica's
    weights restored, and the caller's grad mode untouched (no grad-mode context is held across a generator yield)."""
    from oracle.dynamic_eval_ref import prepare_chunks
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.model import SCConformerXL
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    vocab = 128
    _, hip = _pair(cuda, SMALL, vocab=vocab, seed=5, blank_bias=1.5)
    replicas = [hip]
    for _ in range(2):
        m = SCConformerXL(SMALL, vocab_size=vocab, device=cuda)
        m.flat_params.copy_(hip.flat_params)
        replicas.append(m)
    tok = SyntheticTokenizer(vocab)
    g = torch.Generator().manual_seed(21)
    specs = [torch.randn(1, 80, n, generator=g) for n in (1500, 1100, 1500, 700, 1300)]   # ragged, more than chains
    seq_len, overlap = 512, 256
    # SpecAugment draws come from the global CPU RNG in call order, which interleaving changes: pin them per window key
    _, keys = prepare_chunks(specs[0], seq_len, overlap)
    masks = _masks_for(keys, 80, None, seed=9)

    def args(graphs):
        return _args(optim_lr=1e-4, quiet=True, use_graphs=graphs, spec_augment_fixed_masks=masks)

    eager = [lib.dynamic_eval(args(False), hip, s, seq_len, overlap, tok, use_tqdm=False) for s in specs]
    graphed = [lib.dynamic_eval(args(True), hip, s, seq_len, overlap, tok, use_tqdm=False) for s in specs]
    for a_, b_ in zip(eager, graphed):
        assert np.array_equal(a_, b_), "hipGraph replay must not change a single bit"
    before = [m.flat_params.clone() for m in replicas]
    many = lib.dynamic_eval_many(args(True), replicas, specs, seq_len, overlap, tok, use_tqdm=False)
    assert len(many) == len(specs)
    for a_, b_ in zip(eager, many):
        assert a_.shape == b_.shape and np.array_equal(a_, b_), "interleaved chains must match the sequential loop bit for bit"
    for m, b in zip(replicas, before):
        assert torch.equal(m.flat_params, b), "every replica's weights must be restored"
    assert torch.is_grad_enabled()
    # the adaptation did something: the no-adapt pass differs
    plain = lib.dynamic_eval(_args(epochs=0, quiet=True), hip, specs[0], seq_len, overlap, tok, use_tqdm=False)
    assert np.abs(plain - eager[0]).max() > 1e-6


def test_fused_subsampling_matches_the_separate_kernels_through_the_model(cuda):
    """model.fused_subsampling (default): forward bit-identical to the unfused path, every parameter gradient equal up to summation
    order, and the input-gradient path (entropy augmentation: needs dz1 itself) still works from the fused forward."""
    ref, hip = _pair(cuda, SMALL, vocab=128)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 80, 300, generator=g).to(cuda)
    outs, grads, dxs = [], [], []
    for fused in (True, False):
        hip.fused_subsampling = fused
        with torch.enable_grad():
            out = hip(audio_signal=x)['final_posteriors']
        gp = torch.randn(out.shape, generator=torch.Generator().manual_seed(13)).to(cuda) / out[0].numel()
        hip.zero_grad()
        dx = hip.backward(gp, input_grad=True)
        outs.append(out.clone()); grads.append(hip.flat_grads.clone()); dxs.append(dx.clone())
        with torch.enable_grad():
            hip(audio_signal=x)
        hip.zero_grad()
        hip.backward(gp)
        grads.append(hip.flat_grads.clone())
    hip.fused_subsampling = True
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(dxs[0], dxs[1])
    denom = grads[1].abs().max().item()
    assert (grads[0] - grads[2]).abs().max().item() / denom < 1e-5       # input_grad=True runs the separate backward kernels in both modes
    assert (grads[1] - grads[3]).abs().max().item() / denom < 1e-5       # fused backward vs separate backward
    assert (grads[0] - grads[1]).abs().max().item() / denom < 1e-5


@pytest.mark.parametrize("cfg_over", [{}, dict(conv_norm="layer_norm", n_layers=3), dict(self_conditioning=False)])
def test_deferred_reductions_are_bit_identical_through_the_model(cuda, cfg_over):
    """model.defer_reduces (default): the weight-gradient / bias-sum reductions of the backward run as one batched launch at its end
    (dyn_reduce_defer_begin / _flush) — every gradient bit-identical to one launch per reduction, with the shared self-conditioning norm
    (several reductions chained into one output), with frozen parameters (their gradients stay zero), eagerly and through the hipGraph."""
    from dynamic_asr_eval_amd.lib import freeze_subsampling
    ref, hip = _pair(cuda, dict(SMALL, **cfg_over), vocab=128)
    assert hip.defer_reduces
    x = torch.randn(2, 80, 300, generator=torch.Generator().manual_seed(12)).to(cuda)
    for frozen in (False, True):
        if frozen:
            freeze_subsampling(hip)
        for n_active in (None, 1):
            grads = []
            for defer, graphs in ((True, False), (False, False), (True, True), (True, True)):
                hip.defer_reduces, hip.use_graphs = defer, graphs
                with torch.enable_grad():
                    out = hip(audio_signal=x)['final_posteriors']
                nb = out.shape[0] if n_active is None else n_active
                gp = torch.randn(out[:nb].shape, generator=torch.Generator().manual_seed(13)).to(cuda) / out[0].numel()
                hip.zero_grad()
                hip.backward(gp, n_active=n_active)
                grads.append(hip.flat_grads.clone())
            hip.defer_reduces, hip.use_graphs = True, False
            assert grads[0].abs().max().item() > 0
            for g in grads[1:]:
                assert torch.equal(grads[0], g)
            if frozen:
                for name, _ in hip.spec:
                    if not hip.trainable(name):
                        assert float(hip.G[name].abs().max()) == 0.0, name


def test_clean_copy_attention_through_the_fused_kernel(cuda):
    """model.grad_samples = 1 (what lib.dynamic_eval sets: only the augmented copy is differentiated, reference lcasr/lib.py:570-575):
    the clean copy's attention takes the fused no-grad kernel inside the grad-mode batch.  Same posteriors (fp32 summation order
    apart), the same gradients for the augmented copy, and a backward over MORE samples than were kept is refused."""
    from dynamic_asr_eval_amd import ops
    ref, hip = _pair(cuda, SMALL, vocab=128)
    x = torch.randn(2, 80, 4800, generator=torch.Generator().manual_seed(21)).to(cuda)          # T' = 600 >= 512: the fused kernel applies
    res = []
    for gs in (None, 1):
        hip.grad_samples = gs
        with torch.enable_grad():
            out = hip(audio_signal=x)['final_posteriors']
        gp = torch.randn(1, *out.shape[1:], generator=torch.Generator().manual_seed(22)).to(cuda) / out[0].numel()
        hip.zero_grad()
        hip.backward(gp, n_active=1)
        res.append((out.clone(), hip.flat_grads.clone()))
    # the augmented copy runs the same kernels either way, but as a batch of 1 instead of 2: another (tile, K-slice) plan may be
    # chosen for its attention products, so equality is up to fp32 summation order
    assert (res[0][0] - res[1][0]).abs().max().item() < 2e-5
    assert (res[0][1] - res[1][1]).abs().max().item() / res[0][1].abs().max().item() < 1e-5
    with torch.enable_grad():
        out = hip(audio_signal=x)['final_posteriors']
    with pytest.raises(ops.DynError):
        hip.backward(torch.zeros_like(out))
    hip.grad_samples = None


def test_batch_renorm_eval_mode_parity(cuda):
    """conv_norm='batch_renorm': the loop runs the model in eval mode (reference lib.py:525), i.e. a per-channel affine
    with the checkpoint's running statistics.  Non-trivial statistics, forward + every parameter gradient vs the oracle,
    and one adapted dynamic-eval pass."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    from oracle.conformer_ref import SCConformerXLRef
    from dynamic_asr_eval_amd.model import SCConformerXL
    cfg = dict(SMALL, conv_norm="batch_renorm")
    ref = SCConformerXLRef(cfg, vocab_size=128, seed=13, blank_bias=1.5)
    g = torch.Generator().manual_seed(2)
    for name, buf in ref.named_buffers():
        if name.endswith("running_mean"):
            buf.copy_(0.3 * torch.randn(buf.shape, generator=g))
        if name.endswith("running_var"):
            buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
    ref.eval()
    hip = SCConformerXL(cfg, vocab_size=128, device=cuda)
    hip.load_state_dict(ref.state_dict())
    x = torch.randn(2, 80, 200, generator=g)
    out_ref = ref(audio_signal=x)['final_posteriors']
    out = hip(audio_signal=x.to(cuda))['final_posteriors']
    assert (out.cpu() - out_ref).abs().max().item() < 2e-4
    assert torch.equal(out.cpu().argmax(-1), out_ref.argmax(-1))
    gp = torch.randn(out_ref.shape, generator=g) / out_ref.numel()
    out_ref.backward(gp)
    hip.zero_grad(); hip.backward(gp.to(cuda))
    for (n, p), gh in zip(ref.named_parameters(), hip.grads()):
        rel = (gh.cpu() - p.grad).abs().max().item() / (p.grad.abs().max().item() + 1e-12)
        assert rel < 2e-3, f"grad {n}: rel err {rel}"
    ref.zero_grad()
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 1100, generator=g)
    _, keys = R.prepare_chunks(spec, 512, 256)
    masks = _masks_for(keys, 80, None, seed=4)
    o_ref = R.dynamic_eval_ref(ref, spec, 512, 256, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=1, shuffle=False, fixed_masks=masks)
    o = lib.dynamic_eval(_args(optim_lr=1e-4, epochs=1, shuffle=False, spec_augment_fixed_masks=masks, quiet=True), hip, spec, 512, 256, tok,
                         use_tqdm=False)
    assert np.abs(o - o_ref).max() < 1e-3 and np.array_equal(o.argmax(-1), o_ref.argmax(-1))


def test_dynamic_eval_with_empty_pseudo_labels(cuda):
    """A window whose greedy transcript is empty (all blank) still takes its adapt step: CTC against an empty target is
    -sum_t log p(blank) (torch.nn.CTCLoss with target_lengths = 0, what the reference's tokenizer.encode('') leads to,
    lib.py:569-575).  Parity with the oracle on that path, and the weights do move."""
    from oracle import dynamic_eval_ref as R
    from oracle.madgrad_ref import MADGRAD as MADGRAD_REF
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    ref, hip = _pair(cuda, SMALL, vocab=128, seed=9, blank_bias=9.0)
    tok = SyntheticTokenizer(128)
    spec = torch.randn(1, 80, 1100, generator=torch.Generator().manual_seed(6))
    _, keys = R.prepare_chunks(spec, 512, 256)
    masks = _masks_for(keys, 80, None, seed=3)
    out_ref, params_ref = R.dynamic_eval_ref(ref, spec, 512, 256, tok, MADGRAD_REF, {'lr': 1e-4}, {}, epochs=1, shuffle=False,
                                             fixed_masks=masks, return_params=True)
    assert (out_ref.argmax(-1) == 128).all(), "the fixture is meant to decode to nothing"
    out, params = lib.dynamic_eval(_args(optim_lr=1e-4, epochs=1, shuffle=False, spec_augment_fixed_masks=masks, quiet=True), hip, spec,
                                   512, 256, tok, use_tqdm=False, return_params=True)
    assert np.abs(out - out_ref).max() < 1e-3 and np.array_equal(out.argmax(-1), out_ref.argmax(-1))
    moved = max((a - b.detach()).abs().max().item() for a, b in zip(params_ref, ref.parameters()))
    assert moved > 1e-7
    for a, b in zip(params, params_ref):
        assert (a - b).abs().max().item() < 5e-5


def test_lockstep_group_matches_separate_models(cuda):
    """SCConformerXL(group=R): R replicas with DIFFERENT weights in one object, batches ordered sample = chunk * R + replica.  Forward
    log-probs and every replica's parameter gradients against R separate single models on the same inputs (the grouped launches may pick
    other GEMM tiles than the single ones: 2e-5 on log-probs, 1e-4 relative on gradients; row-wise kernels are the same per-sample
    arithmetic), eager and through the hipGraph replay, and with fewer active replicas than the group holds."""
    from dynamic_asr_eval_amd.model import SCConformerXL
    from oracle.conformer_ref import SCConformerXLRef
    R, T = 3, 320          # T' = 40: per-replica slices of the [R, T', 129] head tensors stay 16-byte aligned
    refs = [SCConformerXLRef(SMALL, vocab_size=128, seed=40 + r, blank_bias=0.5) for r in range(R)]
    singles = []
    for ref in refs:
        m = SCConformerXL(SMALL, vocab_size=128, device=cuda)
        m.load_state_dict(ref.state_dict())
        singles.append(m)
    grp = SCConformerXL(SMALL, vocab_size=128, device=cuda, group=R)
    for r, ref in enumerate(refs):
        sd = ref.state_dict()
        for n, _ in grp.spec:
            grp.PR[n][r].copy_(sd[n].to(cuda).reshape(grp.PR[n][r].shape))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2 * R, 80, T, generator=g).to(cuda)             # samples 0..R-1: "augmented" copies, R..2R-1: "clean" copies

    def run_group(active, use_graphs, reps):
        grp.active, grp.use_graphs, grp.grad_samples = active, use_graphs, active
        xa = torch.cat([x[:active], x[R:R + active]]).contiguous()
        for _ in range(reps):
            with torch.enable_grad():
                out = grp(audio_signal=xa)['final_posteriors']
            gp = torch.zeros_like(out[:active])
            gp.copy_(gl[:active])
            grp.zero_grad()
            grp.backward(gp, n_active=active)
        return out.clone(), grp.flat_grads.view(R, grp.n_flat).clone()

    outs, grads = [], []
    Tp = None
    for r, m in enumerate(singles):
        m.grad_samples = 1
        with torch.enable_grad():
            o = m(audio_signal=torch.stack([x[r], x[R + r]]))['final_posteriors']
        Tp = o.shape[1]
        outs.append(o.clone())
    gl = (torch.randn(R, Tp, 129, generator=g) / (Tp * 129)).to(cuda)
    for r, m in enumerate(singles):
        m.zero_grad()
        m.backward(gl[r:r + 1].clone(), n_active=1)          # a fresh (16-byte aligned) buffer: the slice of an odd-sized tensor is not
        grads.append(m.flat_grads.clone())
    for active, use_graphs, reps in ((R, False, 1), (R, True, 3), (2, False, 1), (1, True, 3)):
        og, gg = run_group(active, use_graphs, reps)
        for r in range(active):
            for c, k in ((0, r), (1, active + r)):
                err = (og[k] - outs[r][c]).abs().max().item()
                assert err < 2e-5, f"active {active} graphs {use_graphs}: replica {r} copy {c}: log-probs differ by {err}"
            denom = grads[r].abs().max().item()
            rel = (gg[r] - grads[r]).abs().max().item() / denom
            assert rel < 1e-4, f"active {active} graphs {use_graphs}: replica {r}: gradients differ by {rel} (relative)"
            # per tensor too: a gradient written to the wrong replica or slot shows up here, not in the global maximum
            for n, (o, cnt, shape) in grp._slots.items():
                a, b = gg[r][o:o + cnt], grads[r][o:o + cnt]
                d = b.abs().max().item()
                assert (a - b).abs().max().item() <= 2e-4 * d + 1e-9, (active, use_graphs, r, n)
        for r in range(active, R):
            assert gg[r].abs().max().item() == 0.0, "inactive replicas receive no gradient"
    grp.active, grp.grad_samples = R, None


def test_lockstep_dynamic_eval_matches_one_recording_at_a_time(cuda):
    """lib.dynamic_eval_lockstep (R recordings of equal length advance through every window step together) against lib.dynamic_eval on each
    recording alone, same weights, per-recording stored masks: stitched log-probs within 2e-4 (the weights carry the tile-choice rounding
    through the MADGRAD steps), identical argmax ids, adapted parameters within 5e-5, the group's weights restored; offline and online."""
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.model import SCConformerXL
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    from oracle import dynamic_eval_ref as R_
    from oracle.conformer_ref import SCConformerXLRef
    R, vocab = 3, 128
    ref = SCConformerXLRef(SMALL, vocab_size=vocab, seed=5, blank_bias=1.5)
    single = SCConformerXL(SMALL, vocab_size=vocab, device=cuda)
    single.load_state_dict(ref.state_dict())
    grp = SCConformerXL(SMALL, vocab_size=vocab, device=cuda, group=R)
    grp.load_state_dict(ref.state_dict())
    tok = SyntheticTokenizer(vocab)
    g = torch.Generator().manual_seed(21)
    specs = [torch.randn(1, 80, 1500, generator=g) for _ in range(R)]
    _, keys = R_.prepare_chunks(specs[0], 512, 256)
    masks = [_masks_for(keys, 80, None, seed=30 + r) for r in range(R)]
    for online in (False, True):
        want = []
        for r in range(R):
            a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks[r], quiet=True)
            want.append(lib.dynamic_eval(a, single, specs[r], 512, 256, tok, use_tqdm=False, return_params=True))
        for n_rec in (R, 2):
            a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks[:n_rec], quiet=True)
            before = grp.flat_params.clone()
            got = lib.dynamic_eval_lockstep(a, grp, specs[:n_rec], 512, 256, tok, use_tqdm=False, return_params=True)
            assert torch.equal(grp.flat_params, before), "the group's weights must be restored"
            assert len(got) == n_rec
            for r in range(n_rec):
                (o, p), (ow, pw) = got[r], want[r]
                assert o.shape == ow.shape and np.abs(o - ow).max() < 2e-4, (online, n_rec, r, np.abs(o - ow).max())
                assert np.array_equal(o.argmax(-1), ow.argmax(-1))
                for x, y in zip(p, pw):
                    assert (x - y).abs().max().item() < 1e-3      # MADGRAD's cube root: a gradient element near zero takes a step of ~lr^(2/3) |g|^(1/3) either way
    # recordings of DIFFERENT lengths in one group (given out of length order): the full windows run on the longer ones together, each short
    # last window on its own replica, a finished recording's replica is no longer stepped
    lens = (1100, 1500, 1360)
    specs2 = [torch.randn(1, 80, n, generator=g) for n in lens]
    masks2 = [_masks_for(range(0, 2048, 256), 80, None, seed=50 + r) for r in range(R)]
    for online in (False, True):
        want = []
        for r in range(R):
            a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks2[r], quiet=True)
            want.append(lib.dynamic_eval(a, single, specs2[r], 512, 256, tok, use_tqdm=False, return_params=True))
        a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks2, quiet=True)
        before = grp.flat_params.clone()
        got = lib.dynamic_eval_lockstep(a, grp, specs2, 512, 256, tok, use_tqdm=False, return_params=True)
        assert torch.equal(grp.flat_params, before)
        for r in range(R):
            (o, p), (ow, pw) = got[r], want[r]
            assert o.shape == ow.shape and np.abs(o - ow).max() < 2e-4, (online, r, o.shape, ow.shape, np.abs(o - ow).max())
            assert np.array_equal(o.argmax(-1), ow.argmax(-1))
            for x, y in zip(p, pw):
                assert (x - y).abs().max().item() < 1e-3      # MADGRAD's cube root: a gradient element near zero takes a step of ~lr^(2/3) |g|^(1/3) either way
    # two epochs: the recordings get out of step after the first one (4, 5, 5 windows): every recording keeps its own optimiser step count
    want = []
    for r in range(R):
        a = _args(optim_lr=1e-4, epochs=2, shuffle=False, spec_augment_fixed_masks=masks2[r], quiet=True)
        want.append(lib.dynamic_eval(a, single, specs2[r], 512, 256, tok, use_tqdm=False))
    a = _args(optim_lr=1e-4, epochs=2, shuffle=False, spec_augment_fixed_masks=masks2, quiet=True)
    assert lib.lockstep_supported(a, grp, specs2)
    got = lib.dynamic_eval_lockstep(a, grp, specs2, 512, 256, tok, use_tqdm=False)
    for r in range(R):
        assert got[r].shape == want[r].shape and np.abs(got[r] - want[r]).max() < 5e-4, (r, np.abs(got[r] - want[r]).max())
        assert np.array_equal(got[r].argmax(-1), want[r].argmax(-1))


def test_lockstep_five_shape_classes_in_one_step(cuda):
    """Five recordings whose last windows all sit at key 768 with five different lengths: that window step runs five shape classes, more
    than a 4-slot ring of pinned upload buffers holds, and each class uploads its own targets.  lib.dynamic_eval_lockstep against
    lib.dynamic_eval on each recording alone with per-recording stored masks, offline and online, with the tolerances of
    test_lockstep_dynamic_eval_matches_one_recording_at_a_time."""
    from dynamic_asr_eval_amd import lib
    from dynamic_asr_eval_amd.model import SCConformerXL
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    from oracle import dynamic_eval_ref as R_
    from oracle.conformer_ref import SCConformerXLRef
    R, vocab = 5, 128
    ref = SCConformerXLRef(SMALL, vocab_size=vocab, seed=5, blank_bias=1.5)
    single = SCConformerXL(SMALL, vocab_size=vocab, device=cuda)
    single.load_state_dict(ref.state_dict())
    grp = SCConformerXL(SMALL, vocab_size=vocab, device=cuda, group=R)
    grp.load_state_dict(ref.state_dict())
    tok = SyntheticTokenizer(vocab)
    g = torch.Generator().manual_seed(27)
    lens = (1100, 1150, 1200, 1250, 1270)
    specs = [torch.randn(1, 80, n, generator=g) for n in lens]
    last = [R_.prepare_chunks(sp, 512, 256)[0] for sp in specs]
    assert all(sorted(d) == [0, 256, 512, 768] for d in last) and len({d[768].shape[-1] for d in last}) == R
    masks = [_masks_for(range(0, 1024, 256), 80, None, seed=70 + r) for r in range(R)]
    for online in (False, True):
        want = []
        for r in range(R):
            a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks[r], quiet=True)
            want.append(lib.dynamic_eval(a, single, specs[r], 512, 256, tok, use_tqdm=False, return_params=True))
        a = _args(optim_lr=1e-4, epochs=1, shuffle=False, online=online, spec_augment_fixed_masks=masks, quiet=True)
        before = grp.flat_params.clone()
        got = lib.dynamic_eval_lockstep(a, grp, specs, 512, 256, tok, use_tqdm=False, return_params=True)
        assert torch.equal(grp.flat_params, before), "the group's weights must be restored"
        assert len(got) == R
        for r in range(R):
            (o, p), (ow, pw) = got[r], want[r]
            assert o.shape == ow.shape and np.abs(o - ow).max() < 2e-4, (online, r, np.abs(o - ow).max())
            assert np.array_equal(o.argmax(-1), ow.argmax(-1))
            for x, y in zip(p, pw):
                assert (x - y).abs().max().item() < 1e-3      # MADGRAD's cube root: a gradient element near zero takes a step of ~lr^(2/3) |g|^(1/3) either way
