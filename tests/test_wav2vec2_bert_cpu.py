"""Wav2Vec2-BERT without a GPU: the parameter list against transformers' Wav2Vec2BertForCTC, the configuration reader and each refusal by
name, the harness's model_type dispatch, the relative-key table against transformers' own index, the frame counts and the host-built
front-end matrices against SeamlessM4TFeatureExtractor, and the new C-ABI entries' host-side argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wav2vec2_bert_refs as R  # noqa: E402

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, vocab_size=32, ctc_loss_reduction="mean")
HF_SHAPE = {None: lambda s: s, "pw": lambda s: s + (1,), "dw": lambda s: (s[0], 1, s[1])}
NEW = ("dyn_convmod_causal_fwd", "dyn_convmod_causal_time_tile", "dyn_dwconv1d_causal_dgrad", "dyn_dwconv1d_causal_wgrad",
       "dyn_dwconv1d_causal_wgrad_workspace_bytes", "dyn_narrow_layernorm_fwd", "dyn_narrow_layernorm_bwd",
       "dyn_narrow_layernorm_bwd_workspace_bytes", "dyn_fbank_finish")


@pytest.mark.parametrize("arch", [TOY, dict(num_hidden_layers=2, vocab_size=32), dict(TOY, left_max_position_embeddings=5, right_max_position_embeddings=3)],
                         ids=["toy", "default-widths", "left5-right3"])
def test_param_spec_is_transformers_named_parameters(arch):
    from transformers import Wav2Vec2BertConfig, Wav2Vec2BertForCTC as HF
    from dynamic_asr_eval_amd import wav2vec2_bert_model as M
    cfg = Wav2Vec2BertConfig(**arch)
    c = M.make_config(cfg)
    spec = M.param_spec(c)
    ref = HF(cfg)
    hf = {n: tuple(p.shape) for n, p in ref.named_parameters()}
    names = [n for n, _, _ in spec]
    assert len(names) == len(set(names)) and set(names) == set(hf) == set(ref.state_dict())        # no buffers in this model
    for n, shape, kind in spec:
        assert HF_SHAPE[kind](tuple(shape)) == hf[n], (n, shape, kind, hf[n])
    H, nh = c["hidden_size"], c["num_attention_heads"]
    Pn = c["left_max_position_embeddings"] + c["right_max_position_embeddings"] + 1
    shapes = dict((n, s) for n, s, _ in spec)
    assert shapes["wav2vec2_bert.encoder.layers.1.self_attn.distance_embedding.weight"] == (Pn, H // nh)
    assert shapes["wav2vec2_bert.feature_projection.layer_norm.weight"] == (160,)
    assert shapes["wav2vec2_bert.feature_projection.projection.weight"] == (H, 160)
    assert not any("encoder.layer_norm" in n or "pos_conv_embed" in n or "batch_norm" in n or "feature_extractor" in n for n in names)
    i = names.index("wav2vec2_bert.encoder.layers.1.self_attn.linear_q.weight")                      # the q | k | v slots stay side by side
    assert names[i + 1].endswith("linear_k.weight") and names[i + 2].endswith("linear_v.weight")
    assert names[i + 3].endswith("linear_q.bias") and names[i + 5].endswith("linear_v.bias")


def test_make_config_reads_its_keys_and_refuses_what_is_not_built(tmp_path):
    from transformers import Wav2Vec2BertConfig
    from dynamic_asr_eval_amd import wav2vec2_bert_model as M, run_wav2vec2 as RUN
    from dynamic_asr_eval_amd.ops import DynError
    d, hf = M.make_config(), Wav2Vec2BertConfig(vocab_size=32)
    for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "vocab_size", "layer_norm_eps", "hidden_act",
              "feature_projection_input_dim", "position_embeddings_type", "left_max_position_embeddings", "right_max_position_embeddings",
              "conv_depthwise_kernel_size", "add_adapter", "use_intermediate_ffn_before_adapter"):
        assert d[k] == getattr(hf, k), k                                        # Wav2Vec2BertConfig()'s defaults
    assert M.make_config(hf) == d and M.make_config(d) == d
    c = M.make_config(dict(TOY, hidden_act="gelu", layer_norm_eps=1e-3, left_max_position_embeddings=5, right_max_position_embeddings=3))
    assert (c["hidden_size"], c["hidden_act"], c["layer_norm_eps"], c["left_max_position_embeddings"], c["right_max_position_embeddings"]) == \
        (256, "gelu", 1e-3, 5, 3)
    assert (c["conv_kernel"], c["conv_stride"]) == ((400, 2), (160, 2))         # the front end as the family's frame arithmetic reads it
    for bad, key in ((dict(position_embeddings_type="relative"), "position_embeddings_type"), (dict(position_embeddings_type="rotary"), "position_embeddings_type"),
                     (dict(position_embeddings_type=None), "position_embeddings_type"),
                     (dict(add_adapter=True), "add_adapter"), (dict(use_intermediate_ffn_before_adapter=True), "use_intermediate_ffn_before_adapter"),
                     (dict(feature_projection_input_dim=80), "feature_projection_input_dim"), (dict(hidden_size=384, num_attention_heads=6), "hidden_size=384"),
                     (dict(hidden_size=1280, num_attention_heads=20), "hidden_size=1280"), (dict(conv_depthwise_kernel_size=15), "conv_depthwise_kernel_size=15"),
                     (dict(conv_depthwise_kernel_size=32), "conv_depthwise_kernel_size=32"), (dict(hidden_act="relu"), "hidden_act"),
                     (dict(left_max_position_embeddings=250, right_max_position_embeddings=8), "left_max_position_embeddings"),
                     (dict(num_attention_heads=7), "num_attention_heads"), (dict(adapter_attn_dim=16), "adapter_attn_dim")):
        with pytest.raises(DynError) as e:
            M.make_config(dict(TOY, **bad))
        assert key in str(e.value), (bad, str(e.value))
    p = tmp_path / "config.json"
    p.write_text(Wav2Vec2BertConfig(**dict(TOY, hidden_act="gelu", left_max_position_embeddings=5)).to_json_string(use_diff=False))
    assert RUN.model_type(str(p)) == "wav2vec2-bert"
    c = M.config_from_json(str(p))
    assert (c["hidden_size"], c["num_hidden_layers"], c["hidden_act"], c["left_max_position_embeddings"], c["right_max_position_embeddings"]) == \
        (256, 2, "gelu", 5, 8)
    assert M.make_config(c) == c                                                # a model's own cfg builds its replica
    bad = tmp_path / "rotary.json"
    bad.write_text(Wav2Vec2BertConfig(**dict(TOY, position_embeddings_type="rotary")).to_json_string(use_diff=False))
    with pytest.raises(DynError) as e:
        M.config_from_json(str(bad))
    assert "position_embeddings_type='rotary'" in str(e.value)


def test_dispatch_builds_wav2vec2_bert_for_its_model_type(tmp_path, monkeypatch):
    """load_pretrained_model picks Wav2Vec2BertForCTC for `model_type: wav2vec2-bert` under `--config` (the constructors replaced: no GPU;
    `-c DIR` runs on the GPU in test_wav2vec2_bert_gpu.py); a wav2vec2-conformer config still builds the conformer."""
    import argparse
    from transformers import Wav2Vec2BertConfig, Wav2Vec2ConformerConfig
    from dynamic_asr_eval_amd import wav2vec2_bert_model, wav2vec2_conformer_model, run_wav2vec2 as RUN
    built = []

    class Stub:
        _prefix = "stub."

        def __init__(self, cfg, device=None):
            built.append((self.kind, cfg))

        def named_parameters(self):
            return []

    for mod, cls in ((wav2vec2_bert_model, "Wav2Vec2BertForCTC"), (wav2vec2_conformer_model, "Wav2Vec2ConformerForCTC")):
        monkeypatch.setattr(mod, cls, type(cls, (Stub,), {"kind": cls}))
    conf = dict(TOY, conv_dim=(256,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
    for hf, want in ((Wav2Vec2BertConfig(**TOY), "Wav2Vec2BertForCTC"), (Wav2Vec2ConformerConfig(**conf), "Wav2Vec2ConformerForCTC")):
        p = tmp_path / f"{want}.json"
        p.write_text(hf.to_json_string(use_diff=False))
        assert RUN.model_type(str(p)) == hf.model_type
        RUN.load_pretrained_model(argparse.Namespace(config=str(p), checkpoint="", seed=0), "cpu")
        assert built[-1][0] == want and built[-1][1]["hidden_size"] == 256
    assert [k for k, _ in built] == ["Wav2Vec2BertForCTC", "Wav2Vec2ConformerForCTC"]
    assert built[0][1]["left_max_position_embeddings"] == 64 and "left_max_position_embeddings" not in built[1][1]


@pytest.mark.parametrize("left,right,T", [(5, 3, 19), (64, 8, 18), (64, 8, 93)])
def test_relative_key_table_is_transformers_index_after_the_reversal(left, right, T):
    """table[i - j + T - 1] = r means row r of the reversed embedding, i.e. row P - 1 - r of E: that must be transformers' own
    clamp(j - i, -left, right) + left for every (i, j).  The table is monotone and its segments partition the relative positions."""
    from dynamic_asr_eval_amd.wav2vec2_bert_model import relkey_table
    P = left + right + 1
    table, lo, hi = relkey_table(T, left, right)
    assert table.dtype == lo.dtype == hi.dtype == torch.int32 and table.shape == (2 * T - 1,) and lo.shape == hi.shape == (P,)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    hf = torch.clamp(j - i, -left, right) + left                               # modeling_wav2vec2_bert.py: distance + left_max_position_embeddings
    assert torch.equal(P - 1 - table.long()[i - j + T - 1], hf)
    assert (table[1:] >= table[:-1]).all() and table.min().item() >= 0 and table.max().item() <= P - 1
    seen = torch.zeros(2 * T - 1, dtype=torch.int32)
    for r in range(P):
        l, h = lo[r].item(), hi[r].item()
        if l > h:
            assert not (table == r).any(), r
            continue
        assert -(T - 1) <= l and h <= T - 1 and (table[l + T - 1:h + T].long() == r).all(), r
        seen[l + T - 1:h + T] += 1
    assert (seen == 1).all()
    if T - 1 < left:                                                            # T = 18 with left = 64: the far-left rows are never reached
        assert sum(1 for r in range(P) if lo[r].item() > hi[r].item()) == P - (T - 1) - 1 - min(right, T - 1)
    big = relkey_table(96, left, right).table                                   # a bucket's table holds the table of every length inside it
    assert torch.equal(big[96 - T:96 + T - 1], table)
    # the identity itself, in torch on the CPU: softmax over S + c2p[i, t(i - j)] is transformers' relative-key score
    g = torch.Generator().manual_seed(T)
    q, E = torch.randn(T, 8, generator=g, dtype=torch.float64), torch.randn(P, 8, generator=g, dtype=torch.float64)
    want = torch.einsum("ld,lrd->lr", q, E[hf])
    c2p = q @ E.flip(0).t()
    assert torch.equal(c2p.gather(1, table.long()[i - j + T - 1]), want) or (c2p.gather(1, table.long()[i - j + T - 1]) - want).abs().max() < 1e-12


def test_frame_counts_are_the_extractors_valid_rows():
    """conv_lengths(L)[-1] (through the parent's arithmetic on the (400, 2) / (160, 2) front end) = the rows the extractor marks valid."""
    from dynamic_asr_eval_amd import wav2vec2_bert_model as M
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
    from dynamic_asr_eval_amd.frontend import kaldi_fbank_frames
    from types import SimpleNamespace
    m = SimpleNamespace(cfg=M.make_config(TOY), bucket_frames=32)
    g = torch.Generator().manual_seed(0)
    for L in list(range(560, 560 + 701, 53)) + [48077]:
        F, T = Wav2Vec2ForCTC.conv_lengths(m, L)
        assert (F, T) == (1 + (L - 400) // 160, (1 + (L - 400) // 160) // 2) == kaldi_fbank_frames(L)
        feats, valid = R.extractor_rows(torch.randn(L, generator=g))
        assert valid == T and feats.shape[0] in (T, T + 1), (L, valid, T, feats.shape)   # (the extractor may pad one more, invalid, row)
        assert Wav2Vec2ForCTC.conv_lengths(m, Wav2Vec2ForCTC.samples_for_frames(m, T))[-1] == T
        assert Wav2Vec2ForCTC.conv_lengths(m, Wav2Vec2ForCTC.samples_for_frames(m, T) - 1)[-1] == T - 1
    assert Wav2Vec2ForCTC.samples_for_frames(m, 1) == 560
    assert kaldi_fbank_frames(559) == (1, 0) and kaldi_fbank_frames(399) == (0, 0)


@pytest.mark.parametrize("L,offset", [(560, 0.0), (560 + 160 * 4, 0.0), (16000, 0.0), (16000, 0.5)], ids=["two-frames", "odd-F", "1s", "1s-dc-offset"])
def test_host_built_matrices_reproduce_the_extractor_in_float64(L, offset):
    """The folded basis (scale, mean removal, pre-emphasis, povey window, DFT) and the mel matrix, applied in float64 torch, reproduce the
    extractor's formula to 1e-9 (measured 1e-13 .. 7e-13).  The extractor's OUTPUT is not a float64 quantity (wav2vec2_bert_refs.py: complex64
    spectra, float32 normalisation).  It is first tied to the restated formula: every element within extractor_bound, the float32 roundings
    it performs (measured: 0.06 .. 0.29 of the bound; 1.0e-5 .. 1.6e-5 at most).  The matrices are then within that bound + 1e-9 of the
    extractor's output, element by element."""
    from dynamic_asr_eval_amd.frontend import KP, WIN, kaldi_fbank_frames, kaldi_fbank_matrices
    x = torch.randn(L, generator=torch.Generator().manual_seed(L)) + offset
    want, valid = R.extractor_rows(x)
    basis, fb = kaldi_fbank_matrices()
    assert basis.dtype == fb.dtype == torch.float64 and basis.shape == (WIN, 2 * KP) and fb.shape == (KP, 80)
    F, T = kaldi_fbank_frames(L)
    assert T == valid
    feats = R.fbank_chain(x, basis, fb, torch.float64).numpy()
    exact = R.fbank_formula_f64(x)
    assert feats.shape == exact.shape == (T, 160)
    err = np.abs(feats - exact).max()
    own = np.abs(want[:T].astype(np.float64) - exact).max()
    bound = R.extractor_bound(x)
    ratio = (np.abs(want[:T].astype(np.float64) - exact) / bound).max()
    against = np.abs(feats - want[:T].astype(np.float64))
    print(f"L={L} offset={offset}: matrices vs formula {err:.2e} | extractor vs its formula {own:.2e} = {ratio:.2f} of its bound | "
          f"matrices vs extractor {against.max():.2e}")
    assert err < 1e-9, err
    assert ratio <= 1.0, (ratio, own)                                           # the restated formula IS the extractor's, to float32 rounding
    assert (against <= bound + 1e-9).all(), (against.max(), bound.max())


def test_the_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    p = 256                                                                   # never dereferenced: every call below fails, or has nothing to do, before a launch
    fwd = lambda B=2, T=10, C=256, KW=31, act=0, tt=0, u=p, s=p: lib.dyn_convmod_causal_fwd(u, p, p, p, s, None, None, None, None, None, B, T, C, KW, act, 1e-5, tt, None)  # noqa: E731
    dg = lambda B=2, T=10, C=256, KW=31, dy=p, dx=p + 256: lib.dyn_dwconv1d_causal_dgrad(dy, p, dx, B, T, C, KW, 0.0, None)  # noqa: E731
    wg = lambda B=2, T=10, C=256, KW=31, x=p, ws=p, wsb=1 << 24: lib.dyn_dwconv1d_causal_wgrad(x, p, p, 1.0, B, T, C, KW, ws, wsb, None)  # noqa: E731
    for call, name in ((fwd, b"dyn_convmod_causal_fwd"), (dg, b"dyn_dwconv1d_causal_dgrad"), (wg, b"dyn_dwconv1d_causal_wgrad")):
        for kw, code, word in ((dict(C=384), -4, b"C=384 is not built"), (dict(C=1280), -4, b"C=1280"), (dict(C=160), -4, b"C=160"),
                               (dict(KW=9), -4, b"kernel width 9"), (dict(KW=33), -4, b"kernel width 33"), (dict(B=-1), -1, b"bad sizes"),
                               (dict(T=-1), -1, b"bad sizes")):
            assert call(**kw) == code, (name, kw)
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(B=0) == 0 and call(T=0) == 0
    assert fwd(u=0) == -1 and b"null" in lib.dyn_last_error() and fwd(s=0) == -1
    assert fwd(act=2) == -1 and b"act=2" in lib.dyn_last_error()
    assert fwd(tt=32) == -1 and b"time_tile=32" in lib.dyn_last_error() and fwd(tt=8, B=0) == 0 and fwd(tt=16, B=0) == 0
    assert fwd(u=260) == -1 and b"aligned" in lib.dyn_last_error()
    assert lib.dyn_convmod_causal_time_tile(2, 18) == 8 and lib.dyn_convmod_causal_time_tile(4, 4000) == 16
    assert dg(dy=0) == -1 and b"null" in lib.dyn_last_error()
    assert wg(x=0) == -1 and b"null" in lib.dyn_last_error()
    need = lib.dyn_dwconv1d_causal_wgrad_workspace_bytes(2, 10, 256, 31)
    assert need == 2 * 2 * 256 * 31 * 4                                        # ceil(10 / 8) time tiles per sample
    assert wg(wsb=need - 1) == -3 and wg(ws=0) == -3                           # DYN_E_WORKSPACE
    ln = lambda rows=5, C=160, x=p, beta=p: lib.dyn_narrow_layernorm_fwd(x, p, beta, p, p, p, rows, C, 1e-5, None)  # noqa: E731
    lnb = lambda rows=5, C=160, dy=p, dx=p, dg_=p, db=p, ws=p, wsb=1 << 20: lib.dyn_narrow_layernorm_bwd(p, p, p, p, dy, dx, dg_, db, 1.0, rows, C, ws, wsb, None)  # noqa: E731
    for call, name in ((ln, b"dyn_narrow_layernorm_fwd"), (lnb, b"dyn_narrow_layernorm_bwd")):
        for kw, code, word in ((dict(C=0), -4, b"C=0"), (dict(C=162), -4, b"C=162"), (dict(C=260), -4, b"C=260"), (dict(C=512), -4, b"C=512"),
                               (dict(rows=-1), -1, b"rows=-1")):
            assert call(**kw) == code, (name, kw)
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(rows=0) == 0
    assert ln(x=0) == -1 and b"null" in lib.dyn_last_error() and ln(x=260) == -1 and b"aligned" in lib.dyn_last_error()
    assert ln(beta=0, rows=0) == 0                                             # beta is optional
    assert lnb(dy=0) == -1 and b"null" in lib.dyn_last_error()
    assert lnb(dx=0, dg_=0, db=0) == -1 and b"no output" in lib.dyn_last_error()
    assert lnb(dx=0, rows=0) == 0                                              # dx is optional
    assert lib.dyn_narrow_layernorm_bwd_workspace_bytes(5, 160) == 2 * 2 * 160 * 4      # ceil(5 / 4) partial rows, two sums
    assert lnb(wsb=2 * 2 * 160 * 4 - 1) == -3 and lnb(ws=0) == -3
    fb = lambda B=1, F=10, M=80, mel=p, floor=1e-7, eps=1e-7: lib.dyn_fbank_finish(mel, p, B, F, M, floor, eps, None, None)  # noqa: E731
    for kw, word in ((dict(F=1), b"at least two frames"), (dict(M=0), b"M=0"), (dict(B=-1), b"B=-1"), (dict(mel=0), b"null"),
                     (dict(floor=0.0), b"mel_floor")):
        assert fb(**kw) == -1, kw
        assert b"dyn_fbank_finish" in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
    assert fb(B=0) == 0
