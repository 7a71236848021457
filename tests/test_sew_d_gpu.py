"""SEWDForCTC (sew_d_model.py: SEW's squeezed encoder without its LayerNorm, BERT-named post-LN layers, DeBERTa-v2's disentangled attention on
csrc/disentangled.hip) against transformers' SEWDForCTC on the CPU with the same state dict — logits, every parameter gradient, both
extractor layouts, with and without the feature projection, each position term alone, with and without the embeddings' LayerNorm, linear
positions, the published width, the dynamic-eval loops, bucketed hipGraph replay and the harness — at the bars tests/test_sew_gpu.py holds
SEW to.  The shared checks live in tests/ctc_family_cases.py; those that name wav2vec2's `feature_projection.projection.weight` are restated
here with SEW-D's names, same protocol, lengths and bars, as test_sew_gpu.py does."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_family_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

PF = "sew_d."
# test_sew_gpu.py's TOY plus the relative positions: 8 buckets over 32 positions, so 46 squeezed frames reach the clamp at both ends
TOY = dict(C.TOY, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), num_conv_pos_embeddings=16,
           num_conv_pos_embedding_groups=4, squeeze_factor=2, position_buckets=8, max_position_embeddings=32)
NARROW = dict(TOY, conv_dim=(64, 64, 128, 128, 512), conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1))   # projection, kernel-1 layers
GROUP = dict(feat_extract_norm="group", conv_bias=False)
LAYER = dict(feat_extract_norm="layer", conv_bias=True)
POS_V = PF + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
UP_W = PF + "encoder.upsample.projection.weight"
REL_W = PF + "encoder.encoder.rel_embeddings.weight"
REL_LN = PF + "encoder.encoder.LayerNorm.weight"
Q_W = PF + "encoder.encoder.layer.0.attention.self.query_proj.weight"


def _pair(cuda, seed=0, arch=TOY, **over):
    from transformers import SEWDConfig, SEWDForCTC as HF
    from dynamic_asr_eval_amd.sew_d_model import SEWDForCTC
    torch.manual_seed(seed)
    cfg = SEWDConfig(**dict(arch, **over))
    ref = HF(cfg).eval()
    C.randomise_1d(ref)
    hip = SEWDForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict(), strict=False)
    return ref, hip


def _check(cuda, ref, hip, L, frames, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, L, generator=g)
    T, s = hip.conv_lengths(L)[-1], hip.cfg["squeeze_factor"]
    assert T == frames
    grads, named = C.forward_and_every_gradient(cuda, ref, hip, x, g, PF)
    for n in (UP_W, POS_V, REL_W, Q_W) + ((REL_LN,) if REL_LN in grads else ()):
        assert grads[n].abs().max().item() > 0.0, n
    out = hip(x.to(cuda))
    assert out.frames == T and out.logits.shape[1] == T
    for t in range(s * (T // s), T):                                            # the zero rows behind the upsampled frames: lm_head.bias, bit for bit
        assert torch.equal(out.logits[:, t], hip.P["lm_head.bias"].expand(2, -1)), t
    C.state_dict_round_trip(ref, hip)


@pytest.mark.parametrize("layout", [GROUP, LAYER], ids=["group", "layer"])
@pytest.mark.parametrize("L,frames", [(6000, 18), (30000, 93)], ids=["18-frames", "93-frames-odd"])
def test_toy_forward_backward_matches_transformers(cuda, layout, L, frames):
    """18 frames: T2 = 9, no relative position reaches the clamp.  93 frames: T2 = 46, bucket +-8 clamps to index 15 / 0; odd, so the last row is
    the zero padding and its logits are lm_head.bias bit for bit."""
    ref, hip = _pair(cuda, **layout)
    assert not any(n.startswith(PF + "feature_projection") for n in hip.P) and REL_LN in hip.P
    _check(cuda, ref, hip, L, frames)


@pytest.mark.parametrize("L,frames", [(380, 18), (1880, 93)], ids=["18-frames", "93-frames-odd"])
def test_narrow_extractor_with_projection_matches_transformers(cuda, L, frames):
    ref, hip = _pair(cuda, arch=NARROW)
    assert PF + "feature_projection.weight" in hip.P
    _check(cuda, ref, hip, L, frames)


@pytest.mark.parametrize("over,L,frames", [(dict(pos_att_type=("c2p",)), 30000, 93), (dict(pos_att_type=("p2c",)), 30000, 93),
                                           (dict(norm_rel_ebd="none"), 6000, 18), (dict(position_buckets=-1, max_position_embeddings=16), 30000, 93),
                                           (dict(squeeze_factor=1), 6000, 18), (dict(squeeze_factor=3), 6300, 19),
                                           (dict(position_buckets=64, max_position_embeddings=128), 6000, 18)],
                         ids=["c2p-only", "p2c-only", "no-rel-layernorm", "linear-positions-16", "s1", "s3-19-frames", "64-buckets-few-reached"])
def test_each_position_term_the_plain_embeddings_linear_positions_and_other_squeeze_factors(cuda, over, L, frames):
    """One position term alone changes the scale (f = 2); `norm_rel_ebd: none` drops the embeddings' LayerNorm and its two parameters; linear
    positions (position_buckets -1, span 16) at 46 squeezed frames clamp from |d| = 16 on; squeeze_factor 1 runs 18 frames, 3 runs 6 with one
    zero row; with 64 buckets 9 squeezed frames reach rows 56 .. 72 of the 128 only: the others' gradient is exactly zero before the LayerNorm."""
    ref, hip = _pair(cuda, **over)
    assert (REL_LN in hip.P) == (over.get("norm_rel_ebd") != "none")
    _check(cuda, ref, hip, L, frames)


def test_published_width_forward_and_every_gradient(cuda):
    """768 wide, 12 x 64 heads, one layer, 256 buckets over 512 positions (the published sew-d-base shape), 19 frames: a [512, 768] table of
    embeddings of which 9 squeezed frames reach a handful of rows; the others' gradient is the LayerNorm's alone."""
    arch = dict(NARROW, conv_dim=(64, 64, 128, 128, 768), hidden_size=768, num_attention_heads=12, num_hidden_layers=1,
                num_conv_pos_embedding_groups=16, position_buckets=256, max_position_embeddings=512)
    ref, hip = _pair(cuda, arch=arch)
    assert hip.P[REL_W].shape == (512, 768)
    _check(cuda, ref, hip, 400, 19, seed=11)


def test_backward_is_bit_reproducible(cuda):
    C.backward_is_bit_reproducible(cuda, _pair(cuda, seed=1)[1])


def test_active_subset_backward(cuda):
    C.active_subset_backward(cuda, _pair(cuda, seed=3)[1])


def test_frozen_prefixes(cuda):
    """ctc_family_cases.frozen_prefixes with SEW-D's names: the extractor and the positional conv frozen, the relative embeddings, their
    LayerNorm, the upsampling projection and `sew_d.layer_norm` keep their gradients."""
    hip = _pair(cuda, seed=4)[1]
    frozen_prefix = PF + "encoder.pos_conv_embed"
    x = torch.randn(1, 5000, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {PF + "feature_extractor", frozen_prefix}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[PF + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
    hit = [n for n in hip.G if n.startswith(frozen_prefix)]
    assert len(hit) >= 2
    for n in hit:
        assert hip.G[n].abs().max().item() == 0.0, n
    for n in (REL_W, REL_LN, UP_W, Q_W, PF + "layer_norm.weight"):
        assert hip.G[n].abs().max().item() > 0.0, n
    hip.frozen = {REL_W}                                                         # and the other way round: the table frozen, its LayerNorm live
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[REL_W].abs().max().item() == 0.0 and hip.G[REL_LN].abs().max().item() > 0.0
    hip.frozen = set()


@pytest.mark.parametrize("over", [dict(), dict(squeeze_factor=3), dict(position_buckets=64, max_position_embeddings=128)],
                         ids=["s2", "s3", "64-buckets-few-reached"])
def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda, over):
    """ctc_family_cases.bucketed_graph_replay with SEW-D's names (test_sew_gpu.py's restatement, the relative embeddings as the live name): the
    bucket's table serves every valid length inside it, padded keys are masked, padded queries give and receive nothing.  With 64 buckets
    the bucket's length reaches more rows of the embeddings than the utterance's own; the valid (i, j) still gather the same ones."""
    ref, hip = _pair(cuda, seed=11, **over)
    pf, live_name, proj = PF, REL_W, PF + "layer_norm.weight"
    s = hip.cfg["squeeze_factor"]
    hip.graph_after, hip.bucket_frames = 1, 8

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

    assert [hip.conv_lengths(L)[-1] for L in C.REPLAY_LENGTHS] == [13, 12, 18, 10, 13]
    for k, L in enumerate(C.REPLAY_LENGTHS):
        fz = (pf + "feature_extractor",) if k == 4 else ()      # bucket 16's backward graph exists by then and its activations are released
        T, Tb, lo, gr = run(L, True, fz)
        T2, Tb2, lo2, gr2 = run(L, False, fz)
        assert T == T2 == Tb2 == hip.conv_lengths(L)[-1] and Tb == -(-T // 8) * 8 and lo.shape == lo2.shape
        err = (lo - lo2).abs().max().item()
        print(f"L {L}: logits error against the unpadded eager run {err:.2e}")
        assert err < 2e-5 * max(1.0, lo2.abs().max().item()), (L, err)
        assert (gr - gr2).abs().max().item() < 1e-4 * gr2.abs().max().item(), (L, (gr - gr2).abs().max().item(), gr2.abs().max().item())
        for t in range(s * (T // s), T):                        # the zero rows of the unpadded run, inside the bucket too
            assert torch.equal(lo[:, t], hip.P["lm_head.bias"].expand(2, -1)) and torch.equal(lo2[:, t], lo[:, t]), (L, t)
        assert hip.G[live_name].abs().max().item() > 0.0 and hip.G[Q_W].abs().max().item() > 0.0
        if fz:
            assert hip.G[pf + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
            assert hip.G[proj].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


@pytest.mark.parametrize("seed", [0, 2])
def test_dynamic_eval_su_matches_oracle(cuda, seed):
    """Seeds at which the oracle stays finite on the CPU (ctc_family_cases.dynamic_eval_su_matches_oracle's docstring)."""
    ref, hip = _pair(cuda, seed=seed)
    C.dynamic_eval_su_matches_oracle(cuda, ref, hip)


@pytest.mark.parametrize("seed", [2, 4])
def test_chunked_dynamic_eval_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed)
    C.chunked_dynamic_eval_matches_oracle(cuda, ref, hip)


def test_run_wav2vec2_harness_with_a_sew_d_directory(cuda, tmp_path, capsys):
    from transformers import SEWDConfig, SEWDForCTC as HF
    torch.manual_seed(0)
    cfg = SEWDConfig(**TOY)
    w2 = {k: v for k, v in TOY.items() if k not in ("squeeze_factor", "position_buckets", "max_position_embeddings")}
    C.harness_with_a_directory(tmp_path, capsys, cfg, HF(cfg), "sew-d", w2)
