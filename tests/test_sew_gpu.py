"""SEWForCTC (sew_model.py: Wav2Vec2ForCTC's extractor, post-LN layers and lm_head around the squeezed encoder on csrc/squeeze.hip) against
transformers' SEWForCTC on the CPU with the same state dict — logits, every parameter gradient, both extractor layouts, with and without the
feature projection, the dynamic-eval loops, bucketed hipGraph replay and the harness — at the bars tests/test_data2vec_audio_gpu.py and
tests/test_hubert_gpu.py hold their models to.  The shared checks live in tests/ctc_family_cases.py; the two of them that name wav2vec2's
`feature_projection.projection.weight` are restated here with SEW's names, same protocol, lengths and bars."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_family_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

PF = "sew."
# C.TOY with wav2vec2's seven kernels and strides spelled out (SEWConfig's defaults have thirteen layers); conv_dim[-1] == hidden_size: no projection
TOY = dict(C.TOY, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), num_conv_pos_embeddings=16,
           num_conv_pos_embedding_groups=4, squeeze_factor=2)
NARROW = dict(TOY, conv_dim=(64, 64, 128, 128, 512), conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1))   # projection, kernel-1 layers
GROUP = dict(feat_extract_norm="group", conv_bias=False)
LAYER = dict(feat_extract_norm="layer", conv_bias=True)
POS_V = PF + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
UP_W = PF + "encoder.upsample.projection.weight"


def _pair(cuda, seed=0, arch=TOY, **over):
    from transformers import SEWConfig, SEWForCTC as HF
    from dynamic_asr_eval_amd.sew_model import SEWForCTC
    torch.manual_seed(seed)
    cfg = SEWConfig(**dict(arch, **over))
    ref = HF(cfg).eval()
    C.randomise_1d(ref)
    hip = SEWForCTC(cfg, device=cuda)
    hip.load_state_dict(ref.state_dict(), strict=False)
    return ref, hip


def _check(cuda, ref, hip, L, frames, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, L, generator=g)
    T, s = hip.conv_lengths(L)[-1], hip.cfg["squeeze_factor"]
    assert T == frames
    grads, named = C.forward_and_every_gradient(cuda, ref, hip, x, g, PF)
    assert grads[UP_W].abs().max().item() > 0.0 and grads[POS_V].abs().max().item() > 0.0
    out = hip(x.to(cuda))
    assert out.frames == T and out.logits.shape[1] == T
    for t in range(s * (T // s), T):                                            # the zero rows behind the upsampled frames: lm_head.bias, bit for bit
        assert torch.equal(out.logits[:, t], hip.P["lm_head.bias"].expand(2, -1)), t
    C.state_dict_round_trip(ref, hip)


@pytest.mark.parametrize("layout", [GROUP, LAYER], ids=["group", "layer"])
@pytest.mark.parametrize("L,frames", [(6000, 18), (30000, 93)], ids=["18-frames", "93-frames-odd"])
def test_toy_forward_backward_matches_transformers(cuda, layout, L, frames):
    """No projection (conv_dim[-1] == hidden_size); K = 16, an even kernel whose conv gives one frame more than the pool at 18 frames.  93 frames:
    odd, the last row is the zero padding and its logits are lm_head.bias bit for bit."""
    ref, hip = _pair(cuda, **layout)
    assert not any(n.startswith(PF + "feature_projection") for n in hip.P)
    _check(cuda, ref, hip, L, frames)


@pytest.mark.parametrize("layout", [GROUP, LAYER], ids=["group", "layer"])
@pytest.mark.parametrize("L,frames", [(380, 18), (1880, 93)], ids=["18-frames", "93-frames-odd"])
def test_narrow_extractor_with_projection_matches_transformers(cuda, layout, L, frames):
    """conv_dim (64, 64, 128, 128, 512) with kernel-1 / stride-1 layers and a 512 -> 256 feature projection, in both extractor layouts: the
    layer-norm one runs its 64- and 128-channel layers on the narrow instances of ops.bias_layernorm_gelu."""
    ref, hip = _pair(cuda, arch=NARROW, **layout)
    assert PF + "feature_projection.weight" in hip.P
    _check(cuda, ref, hip, L, frames)


def test_unbuilt_extractor_width_is_refused_by_name(cuda):
    from transformers import SEWConfig
    from dynamic_asr_eval_amd.ops import DynError
    from dynamic_asr_eval_amd.sew_model import SEWForCTC
    with pytest.raises(DynError) as e:
        SEWForCTC(SEWConfig(**dict(NARROW, conv_dim=(64, 96, 128, 128, 512), **LAYER)), device=cuda)
    assert "conv_dim" in str(e.value) and "96" in str(e.value)


@pytest.mark.parametrize("over,L,frames", [(dict(num_conv_pos_embeddings=15), 6000, 18), (dict(squeeze_factor=3), 6300, 19),
                                           (dict(squeeze_factor=1), 6000, 18)], ids=["K15-odd", "s3-19-frames", "s1"])
def test_odd_kernel_and_other_squeeze_factors(cuda, over, L, frames):
    """K = 15: no frame dropped.  squeeze_factor 3 at 19 frames: 6 squeezed frames and one zero row.  squeeze_factor 1: the degenerate pool."""
    ref, hip = _pair(cuda, **over)
    _check(cuda, ref, hip, L, frames)


def test_wide_shape_forward_and_every_gradient(cuda):
    """512 wide (the published small / mid width), 8 x 64 heads, 16 groups, with the narrow extractor's 512 channels: no projection."""
    arch = dict(NARROW, hidden_size=512, num_attention_heads=8, num_hidden_layers=1, num_conv_pos_embedding_groups=16)
    ref, hip = _pair(cuda, arch=arch)
    _check(cuda, ref, hip, 400, 19, seed=11)


def test_backward_is_bit_reproducible(cuda):
    C.backward_is_bit_reproducible(cuda, _pair(cuda, seed=1)[1])


def test_active_subset_backward(cuda):
    C.active_subset_backward(cuda, _pair(cuda, seed=3)[1])


@pytest.mark.parametrize("arch,proj", [(TOY, PF + "layer_norm.weight"), (NARROW, PF + "feature_projection.weight")], ids=["toy", "narrow"])
def test_frozen_prefixes(cuda, arch, proj):
    """ctc_family_cases.frozen_prefixes with SEW's names: the extractor and the positional conv frozen, the upsampling projection and `proj`
    keep their gradients."""
    hip = _pair(cuda, seed=4, arch=arch)[1]
    frozen_prefix, live_name = PF + "encoder.pos_conv_embed", UP_W
    L = 5000 if arch is TOY else 400
    x = torch.randn(1, L, generator=torch.Generator().manual_seed(2)).to(cuda)
    hip.frozen = {PF + "feature_extractor", frozen_prefix}
    out = hip(x).logits
    hip.zero_grad(); hip.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(6)) / out.numel()).to(cuda))
    assert hip.G[PF + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
    hit = [n for n in hip.G if n.startswith(frozen_prefix)]
    assert len(hit) >= 2 and not live_name.startswith(frozen_prefix)
    for n in hit:
        assert hip.G[n].abs().max().item() == 0.0, n
    assert hip.G[live_name].abs().max().item() > 0.0
    assert hip.G[proj].abs().max().item() > 0.0
    assert hip.G[PF + "encoder.layer_norm.weight"].abs().max().item() > 0.0
    hip.frozen = set()


@pytest.mark.parametrize("over", [dict(), dict(squeeze_factor=3)], ids=["s2", "s3"])
def test_bucketed_graph_replay_matches_the_unpadded_eager_run(cuda, over):
    """ctc_family_cases.bucketed_graph_replay with SEW's names.  13 valid frames in a bucket of 16: squeezed row 6 averages the last valid
    frame with a zero row and must reach nothing, and output row 12 must be exact zero before lm_head (its logits: lm_head.bias)."""
    ref, hip = _pair(cuda, seed=11, **over)
    pf, live_name, proj = PF, POS_V, PF + "layer_norm.weight"
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
        assert hip.G[live_name].abs().max().item() > 0.0
        if fz:
            assert hip.G[pf + "feature_extractor.conv_layers.0.conv.weight"].abs().max().item() == 0.0
            assert hip.G[proj].abs().max().item() > 0.0
    assert len(hip._graphs) == 2
    hip.use_graphs, hip.frozen = False, set()


@pytest.mark.parametrize("seed", [0, 2])
def test_dynamic_eval_su_matches_oracle(cuda, seed):
    """Seeds at which the oracle stays finite on the CPU (ctc_family_cases.dynamic_eval_su_matches_oracle's docstring): with seed 1 the
    transformers model's own loss is inf on these utterances."""
    ref, hip = _pair(cuda, seed=seed)
    C.dynamic_eval_su_matches_oracle(cuda, ref, hip)


@pytest.mark.parametrize("seed", [2, 4])
def test_chunked_dynamic_eval_matches_oracle(cuda, seed):
    ref, hip = _pair(cuda, seed=seed)
    C.chunked_dynamic_eval_matches_oracle(cuda, ref, hip)


def test_run_wav2vec2_harness_with_a_sew_directory(cuda, tmp_path, capsys):
    from transformers import SEWConfig, SEWForCTC as HF
    torch.manual_seed(0)
    cfg = SEWConfig(**TOY)
    w2 = {k: v for k, v in TOY.items() if k != "squeeze_factor"}
    C.harness_with_a_directory(tmp_path, capsys, cfg, HF(cfg), "sew", w2)
