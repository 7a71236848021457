"""SEW-D without a GPU: the host-built bucket table against transformers' build_relative_position mapped through the clamp (and its
segments), the parameter list against transformers' SEWDForCTC state dict, the configuration reader and each refusal by name, config.json
round trips, the harness's model_type dispatch, and the new C-ABI entries' host-side argument checks."""
import pytest
import torch

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), vocab_size=32, num_conv_pos_embeddings=16,
           num_conv_pos_embedding_groups=4, squeeze_factor=2, position_buckets=8, max_position_embeddings=32)
NARROW = dict(TOY, conv_dim=(64, 64, 128, 128, 512), conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1))     # with the projection
HF_SHAPE = {None: lambda s: s, "conv": lambda s: (s[0], s[2], s[1]), "g": lambda s: (1, 1, s[0])}
TABLES = [(9, 8, 32), (19, 8, 32), (46, 8, 32), (48, 4, 8), (40, 16, 16), (375, 256, 512), (600, 256, 512), (30, -1, 16)]   # (T, buckets, max_position)
NEW = ("dyn_softmax_disentangled_fwd", "dyn_disentangled_bwd", "dyn_squeeze_fwd", "dyn_squeeze_bwd", "dyn_squeeze_bwd_workspace_bytes")


@pytest.mark.parametrize("T,b,m", TABLES)
def test_bucket_table_is_build_relative_position_through_the_clamp(T, b, m):
    """table[i - j + T - 1] == clamp(build_relative_position(T, T, b, m)[i, j] + span, 0, 2 span - 1) for every (i, j), which is also
    transformers' p2c index clamp(-rel[j, i] + span); the segments partition [-(T - 1), T - 1] and t is constant on each."""
    from transformers.models.sew_d.modeling_sew_d import build_relative_position
    from dynamic_asr_eval_amd.sew_d_model import att_span, bucket_table
    span = att_span(b, m)
    table, lo, hi = bucket_table(T, b, m)
    assert table.dtype == lo.dtype == hi.dtype == torch.int32
    assert table.shape == (2 * T - 1,) and lo.shape == hi.shape == (2 * span,)
    rel = build_relative_position(T, T, bucket_size=b, max_position=m)[0]
    c2p = torch.clamp(rel + span, 0, 2 * span - 1)
    p2c = torch.clamp(-rel + span, 0, 2 * span - 1)                            # gathered at [j, i], then transposed
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    got = table.long()[i - j + T - 1]
    assert torch.equal(got, c2p) and torch.equal(got, p2c.t())
    if (T, b, m) in ((46, 8, 32), (48, 4, 8), (600, 256, 512), (30, -1, 16)):   # the clamp binds: the unclamped index leaves the table
        assert (rel + span).max().item() > 2 * span - 1
    seen = torch.zeros(2 * T - 1, dtype=torch.int32)
    for r in range(2 * span):
        l, h = lo[r].item(), hi[r].item()
        if l > h:
            assert not (table == r).any(), r
            continue
        assert -(T - 1) <= l and h <= T - 1
        assert (table[l + T - 1:h + T].long() == r).all(), r
        seen[l + T - 1:h + T] += 1
    assert (seen == 1).all()                                                  # every d in exactly one segment
    assert (table[1:] >= table[:-1]).all()


def test_a_table_of_a_longer_row_holds_the_shorter_rows_table():
    """Bucketed replay: the table depends on i - j only, so the centre of the table of a padded length is the table of every length inside."""
    from dynamic_asr_eval_amd.sew_d_model import bucket_table
    for b, m in ((8, 32), (256, 512), (-1, 16)):
        big = bucket_table(48, b, m).table
        for T in (1, 9, 41, 47):
            assert torch.equal(big[48 - T:48 + T - 1], bucket_table(T, b, m).table), (b, m, T)


@pytest.mark.parametrize("arch,over", [(TOY, {}), (NARROW, {}), (TOY, dict(norm_rel_ebd="none", position_buckets=-1, max_position_embeddings=16)),
                                       (None, {})], ids=["toy", "projection", "no-norm-linear", "default"])
def test_param_spec_is_transformers_state_dict(arch, over):
    from transformers import SEWDConfig, SEWDForCTC as HF
    from dynamic_asr_eval_amd import sew_d_model as M
    cfg = SEWDConfig(**dict(arch or {}, **over))
    c = M.make_config(cfg)
    spec = M.param_spec(c)
    hf = {n: tuple(p.shape) for n, p in HF(cfg).state_dict().items()}
    names = [n for n, _, _ in spec]
    assert len(names) == len(set(names)) and set(names) == set(hf)
    for n, shape, kind in spec:
        assert HF_SHAPE[kind](tuple(shape)) == hf[n], (n, shape, kind, hf[n])
    H = c["hidden_size"]
    span = M.att_span(c["position_buckets"], c["max_relative_positions"])
    assert dict((n, s) for n, s, _ in spec)["sew_d.encoder.encoder.rel_embeddings.weight"] == (2 * span, H)
    assert ("sew_d.encoder.encoder.LayerNorm.weight" in names) == M.rel_norm(c) == (over.get("norm_rel_ebd") != "none")
    assert not any(n.startswith("sew_d.encoder.layer_norm") or n.startswith("sew_d.encoder.layers.") for n in names)
    assert ("sew_d.feature_projection.weight" in names) == (arch is not TOY)
    i = names.index("sew_d.encoder.encoder.layer.1.attention.self.query_proj.weight")     # the q | k | v slots stay side by side
    assert names[i + 1].endswith("key_proj.weight") and names[i + 2].endswith("value_proj.weight")
    assert names[i + 3].endswith("query_proj.bias") and names[i + 5].endswith("value_proj.bias")


def test_make_config_reads_its_keys_and_refuses_what_is_not_built(tmp_path):
    from transformers import SEWDConfig
    from dynamic_asr_eval_amd import sew_d_model as M, sew_model, run_wav2vec2 as R
    from dynamic_asr_eval_amd.ops import DynError
    d, hf = M.make_config(), SEWDConfig()
    for k in ("squeeze_factor", "feat_extract_activation", "hidden_act", "conv_dim", "conv_kernel", "conv_stride", "hidden_size",
              "num_hidden_layers", "num_attention_heads", "intermediate_size", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups",
              "vocab_size", "layer_norm_eps", "feature_layer_norm_eps", "feat_extract_norm", "conv_bias", "max_position_embeddings",
              "position_buckets", "share_att_key", "relative_attention", "pos_att_type", "norm_rel_ebd"):
        want = getattr(hf, k)
        assert d[k] == (tuple(want) if isinstance(want, (list, tuple)) else want), k   # SEWDConfig()'s defaults
    assert (d["layer_norm_eps"], d["feature_layer_norm_eps"], d["max_relative_positions"]) == (1e-7, 1e-5, 512)
    assert M.make_config(hf) == d and M.make_config(d) == d
    assert M.make_config(dict(hidden_act="gelu"))["hidden_act"] == "gelu"
    assert M.make_config(dict(pos_att_type="c2p|p2c"))["pos_att_type"] == ("c2p", "p2c")
    assert M.make_config(dict(max_relative_positions=64))["max_relative_positions"] == 64
    for bad, key in ((dict(relative_attention=False), "relative_attention"), (dict(share_att_key=False), "share_att_key"),
                     (dict(pos_att_type=()), "pos_att_type"), (dict(pos_att_type=("c2p", "p2p")), "pos_att_type"),
                     (dict(hidden_size=384), "hidden_size"), (dict(hidden_act="gelu_new"), "hidden_act"),
                     (dict(feat_extract_activation="relu"), "feat_extract_activation"), (dict(squeeze_factor=5), "squeeze_factor"),
                     (dict(conv_dim=(64, 128, 320)), "conv_dim[-1]"), (dict(feat_extract_norm="layer", conv_bias=False), "conv_bias"),
                     (dict(position_buckets=-1, max_position_embeddings=0), "max_position_embeddings")):
        with pytest.raises(DynError) as e:
            M.make_config(bad)
        assert key in str(e.value), (bad, str(e.value))
    assert "position_buckets" not in sew_model.make_config(dict(position_buckets=8))       # SEW's reader is unchanged
    p = tmp_path / "config.json"
    p.write_text(SEWDConfig(**dict(NARROW, squeeze_factor=3, pos_att_type=("c2p",), norm_rel_ebd="none")).to_json_string(use_diff=False))
    assert R.model_type(str(p)) == "sew-d"
    c = M.config_from_json(str(p))
    assert (c["squeeze_factor"], c["conv_dim"], c["hidden_size"], c["position_buckets"], c["max_relative_positions"], c["pos_att_type"],
            c["norm_rel_ebd"], c["hidden_act"]) == (3, (64, 64, 128, 128, 512), 256, 8, 32, ("c2p",), "none", "gelu_python")
    assert M.make_config(c) == c                                              # a model's own cfg builds its replica
    bad = tmp_path / "tiny.json"
    bad.write_text(SEWDConfig(**dict(TOY, hidden_size=384, num_attention_heads=6)).to_json_string(use_diff=False))
    with pytest.raises(DynError) as e:
        M.config_from_json(str(bad))
    assert "hidden_size=384" in str(e.value)


def test_dispatch_builds_sew_d_for_model_type_sew_d(tmp_path, monkeypatch):
    """load_pretrained_model picks SEWDForCTC for `model_type: sew-d` under `--config` (the constructors replaced: no GPU)."""
    import argparse
    from transformers import SEWConfig, SEWDConfig
    from dynamic_asr_eval_amd import sew_d_model, sew_model, run_wav2vec2 as R
    built = []

    class Stub:
        _prefix = "stub."

        def __init__(self, cfg, device=None):
            built.append((self.kind, cfg))

        def named_parameters(self):
            return []

    for mod, cls in ((sew_d_model, "SEWDForCTC"), (sew_model, "SEWForCTC")):
        monkeypatch.setattr(mod, cls, type(cls, (Stub,), {"kind": cls}))
    sew = {k: v for k, v in TOY.items() if k not in ("position_buckets", "max_position_embeddings")}
    for hf, want in ((SEWDConfig(**TOY), "SEWDForCTC"), (SEWConfig(**sew), "SEWForCTC")):
        p = tmp_path / f"{want}.json"
        p.write_text(hf.to_json_string(use_diff=False))
        assert R.model_type(str(p)) == hf.model_type
        R.load_pretrained_model(argparse.Namespace(config=str(p), checkpoint="", seed=0), "cpu")
        assert built[-1][0] == want and built[-1][1]["hidden_size"] == 256 and built[-1][1]["squeeze_factor"] == 2
    assert [k for k, _ in built] == ["SEWDForCTC", "SEWForCTC"]
    assert built[0][1]["position_buckets"] == 8 and "position_buckets" not in built[1][1]


def test_synthetic_init_starts_every_norm_weight_at_one():
    """run_wav2vec2.init_synthetic keys on `layer_norm.weight`; SEW-D's layers spell it `LayerNorm.weight` and name it to the initialiser."""
    from dynamic_asr_eval_amd import run_wav2vec2 as R, sew_d_model as M

    class Model:
        _norm_weight_suffixes = M.SEWDForCTC._norm_weight_suffixes

        def __init__(self):
            self.p = [(n, torch.zeros(shape)) for n, shape, _ in M.param_spec(M.make_config(TOY))]

        def named_parameters(self):
            return self.p

    m = Model()
    R.init_synthetic(m, 0)
    norms = [n for n, _ in m.p if n.endswith("LayerNorm.weight") or n.endswith("layer_norm.weight")]
    assert len(norms) == 2 * 2 + 1 + 1 + 1                                     # two per layer, the rel LayerNorm, sew_d.layer_norm, the extractor's
    for n, p in m.p:
        if p.dim() == 1:
            assert abs(p.mean().item() - (1.0 if n in norms or n.endswith("original0") else 0.0)) < 0.02, n


def test_the_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    names = _lib.exported_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    p = 256                                                                   # never dereferenced: every call below fails, or has nothing to do, before a launch
    fwd = lambda M=2, T=10, ldp=16, nb=16, x=p, y=p + 256, c=p, pt=p: lib.dyn_softmax_disentangled_fwd(x, y, c, pt, p, M, T, ldp, nb, None, None)  # noqa: E731
    bwd = lambda M=2, T=10, ldp=16, nb=16, g=p, dc=p + 256, dp=p + 512, lo=p: lib.dyn_disentangled_bwd(g, dc, dp, p, lo, p, M, T, ldp, nb, None, None)  # noqa: E731
    for call, name in ((fwd, b"dyn_softmax_disentangled_fwd"), (bwd, b"dyn_disentangled_bwd")):
        for kw, word in ((dict(ldp=15), b"ldp=15 is shorter than the n_buckets = 16"), (dict(nb=0), b"n_buckets=0"), (dict(T=0), b"bad sizes"),
                         (dict(M=-1), b"bad sizes"), (dict(T=1 << 20), b"unsupported")):
            assert call(**kw) == -1, (name, kw)                               # DYN_E_ARG
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(M=0) == 0
    assert fwd(x=0) == -1 and b"null" in lib.dyn_last_error()
    assert fwd(c=0, pt=0) == -1 and b"both position terms are null" in lib.dyn_last_error()
    assert fwd(y=p) == -1 and b"alias" in lib.dyn_last_error()                 # y == c2p
    assert fwd(T=16384, M=0) == 0 and bwd(T=8193) == -1 and b"8192" in lib.dyn_last_error()
    assert bwd(g=0) == -1 and bwd(lo=0) == -1 and b"null" in lib.dyn_last_error()
    assert bwd(dc=0, dp=0) == -1 and b"both outputs are null" in lib.dyn_last_error()
    assert bwd(dc=p) == -1 and b"alias" in lib.dyn_last_error()
    sq = lambda B=2, T=10, Tg=5, H=256, G=16, s=2, h=p: lib.dyn_squeeze_fwd(h, p, p, p, B, T, Tg, H, G, s, None, None)  # noqa: E731
    sqb = lambda B=2, T=10, Tg=5, H=256, G=16, s=2, dz=p, db=p, ws=p, wsb=1 << 20: lib.dyn_squeeze_bwd(p, p, dz, p, p, db, 1.0, B, T, Tg, H, G, s, None, ws, wsb, None)  # noqa: E731
    for call, name in ((sq, b"dyn_squeeze_fwd"), (sqb, b"dyn_squeeze_bwd")):
        for kw, word in ((dict(H=384), b"multiple of 256"), (dict(H=1280), b"up to 1024"), (dict(H=768, G=128), b"multiple of 4"),
                         (dict(s=5), b"squeeze factor s=5"), (dict(Tg=4), b"Tg >= T / s"), (dict(B=-1), b"bad dimensions")):
            assert call(**kw) == -1, (name, kw)
            assert name in lib.dyn_last_error() and word in lib.dyn_last_error(), (kw, lib.dyn_last_error())
        assert call(B=0) == 0
    assert sq(h=0) == -1 and b"null" in lib.dyn_last_error() and sq(h=260) == -1 and b"aligned" in lib.dyn_last_error()
    assert sq(T=1) == 0                                                       # no squeezed frame: nothing to do
    assert sqb(dz=0) == -1 and b"null" in lib.dyn_last_error()
    assert lib.dyn_squeeze_bwd_workspace_bytes(10, 256) == 3 * 256 * 4         # ceil(10 / 4) partial rows, one sum
    assert sqb(wsb=3 * 256 * 4 - 1) == -3 and sqb(ws=0) == -3                 # DYN_E_WORKSPACE: 2 * (5 + 1) rows walked
