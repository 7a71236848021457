"""The streaming kernels of NemotronAsrStreamingForRNNT (csrc/stream.hip) against the float64 torch restatements of
tests/nemotron_stream_refs.py, the state stepped over several chunks by the device counter (ops.stream_advance after every step, as a
session does).  The bar is test_rnnt_kernels_gpu.py's, constants and code: at most 4 x the error of the float32 torch restatement
against the same float64 result + 2e-6."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import nemotron_stream_refs as SR  # noqa: E402
from test_rnnt_kernels_gpu import _check  # noqa: E402

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _counter(cuda):
    return torch.zeros(1, dtype=torch.int32, device=cuda)


@pytest.mark.parametrize("cs", [1, 3, 8, 14])
def test_conv_core_carries_its_state(cuda, cs):
    """ops.stream_convmod_k9 at C = 256, B = 2 over four chunks of cs frames: cs = 1 and 3 take the shortfall branch (the new state is
    the old state's tail followed by the chunk), 8 is the boundary, 14 has two time tiles per stream (the second never reads the state).
    Every chunk after the first reads a state that the launch before rewrote; the state itself is compared too (GLU values).
    Measured (MI355X), the case with the kernel's largest error, kernel | float32 restatement | bound: output 1.1e-06 | 7.4e-07 | 5.0e-06,
    state 2.8e-07 | 2.8e-07 | 3.1e-06."""
    from dynamic_asr_eval_amd import ops
    B, C, n = 2, 256, 4
    g = _g(31 + cs)
    w, cb, gamma, beta = torch.randn(C, 9, generator=g) / 3, torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    state = torch.zeros(2, B, 8, C, device=cuda)
    cnt = _counter(cuda)
    s64, s32 = torch.zeros(B, 8, C, dtype=torch.float64), torch.zeros(B, 8, C)
    d = lambda t: t.to(cuda)                                                                                  # noqa: E731
    for step in range(n):
        u = torch.randn(B, cs, 2 * C, generator=g)
        y64, s64 = SR.stream_convmod(u.double(), s64, w.double(), cb.double(), gamma.double(), beta.double())
        y32, s32 = SR.stream_convmod(u, s32, w, cb, gamma, beta)
        y = ops.stream_convmod_k9(d(u), d(w), d(cb), d(gamma), d(beta), state, cnt)
        ops.stream_advance(cnt)
        _check(f"chunk {step}", y.cpu(), y32, y64)
        _check(f"state {step}", state[(step + 1) & 1].cpu(), s32, s64)
    assert int(cnt.item()) == n


@pytest.mark.parametrize("F", [80, 41])
def test_subsampling_stages_carry_one_row(cuda, F):
    """ops.stream_conv2d_first and ops.stream_dwconv2d_s2_act at C = 32, B = 2, lookahead 2: the first chunk (17 rows, two zero rows of
    left context) and two later ones (24 rows, the carried row), an even and an odd frequency width.  Output lengths 9, 12, 12; the carry
    written by a step is the last input row, before the ReLU.
    Measured (MI355X), worst, kernel | float32 restatement | bound: stem 8.6e-07 | 5.7e-07 | 4.3e-06, depthwise 7.9e-07 | 4.0e-07 | 3.6e-06."""
    from dynamic_asr_eval_amd import ops
    B, C = 2, 32
    g = _g(5 + F)
    w, bias = torch.randn(C, 3, 3, generator=g) / 3, torch.randn(C, generator=g)
    c_stem, c_dw = torch.zeros(2, B, F, device=cuda), torch.zeros(2, B, F, C, device=cuda)
    cnt = _counter(cuda)
    d = lambda t: t.to(cuda)                                                                                  # noqa: E731
    k64 = k32 = z64 = z32 = None
    for step, n in enumerate((17, 24, 24)):
        first = step == 0
        x, z = torch.randn(B, n, F, generator=g), torch.randn(B, n, F, C, generator=g)
        y64, k64 = SR.stream_stage(x.double(), k64, w.double(), bias.double(), first, True)
        y32, k32 = SR.stream_stage(x, k32, w, bias, first, True)
        u64, z64 = SR.stream_stage(z.double(), z64, w.double(), bias.double(), first, False)
        u32, z32 = SR.stream_stage(z, z32, w, bias, first, False)
        y = ops.stream_conv2d_first(d(x), d(w), d(bias), c_stem, cnt, first)
        u = ops.stream_dwconv2d_s2_act(d(z), d(w), d(bias), c_dw, cnt, "relu", first)
        ops.stream_advance(cnt)
        assert y.shape == u.shape == (B, SR.stage_len(n, first), F // 2 + 1, C) and y.shape[1] == (9 if first else 12)
        _check(f"stem {step}", y.cpu(), y32, y64)
        _check(f"depthwise {step}", u.cpu(), u32, u64)
        assert torch.equal(c_stem[(step + 1) & 1].cpu(), x[:, -1]) and torch.equal(c_dw[(step + 1) & 1].cpu(), z[:, -1])


ATTN_CASES = [(9, 0, 4, 64), (9, 2, 4, 64), (10, 2, 4, 64), (9, 13, 4, 64), (29, 13, 4, 64), (71, 13, 2, 128)]


@pytest.mark.parametrize("sw,R,nh,D", ATTN_CASES)
def test_attention_step_over_two_turns_of_the_ring(cuda, sw, R, nh, D):
    """ops.stream_attn over 2 (lc + 1) + 2 chunks against nemotron_stream_refs.attn_step, which applies the mask formula to the FULL key
    history: the warm-up counts 0 .. lc, then two whole turns of the ring.  (9, 0): cs = 1, lc = 8; (9, 2): transformers keeps 8 frames,
    the mask shows 6; (10, 2): lc = 3; (9, 13): lc = 0, no cached keys; (29, 13): the released chunk size with lc = 2; (71, 13) at
    D = 128, B = 1: the released LDS footprint (84 keys, 97 position rows).  The ring slot of every step is checked to hold the chunk's
    k / v bit for bit.
    Measured (MI355X), the step with the kernel's largest error over the six cases, kernel | float32 restatement | bound:
    1.7e-06 | 1.4e-06 | 7.5e-06."""
    from dynamic_asr_eval_amd import ops
    cs, lc, _, _ = SR.geometry(sw, R)
    B, H = (1 if D == 128 else 2), nh * D
    W = lc * cs + 2 * cs - 1
    assert ops.stream_geometry(sw, R).W == W
    g = _g(sw * 100 + R)
    bu, bv, pos = torch.randn(H, generator=g), torch.randn(H, generator=g), torch.randn(W, H, generator=g)
    kc, vc = (torch.full((B, lc + 1, cs, H), float("nan"), device=cuda) for _ in range(2))
    cnt = _counter(cuda)
    K64, V64 = (torch.zeros(B, 0, H, dtype=torch.float64) for _ in range(2))
    K32, V32 = (torch.zeros(B, 0, H) for _ in range(2))
    d = lambda t: t.to(cuda)                                                                                  # noqa: E731
    worst = 0.0
    for step in range(2 * (lc + 1) + 2):
        qkv = torch.randn(B, cs, 3 * H, generator=g)
        o64, K64, V64 = SR.attn_step(qkv.double(), K64, V64, bu.double(), bv.double(), pos.double(), cs, lc, nh)
        o32, K32, V32 = SR.attn_step(qkv, K32, V32, bu, bv, pos, cs, lc, nh)
        o = ops.stream_attn(d(qkv), d(bu), d(bv), d(pos), kc, vc, cnt, nh, lc)
        ops.stream_advance(cnt)
        worst = max(worst, _check(f"step {step}", o.cpu(), o32, o64)[0])
        slot = step % (lc + 1)
        assert torch.equal(kc[:, slot].cpu(), qkv[..., H:2 * H]) and torch.equal(vc[:, slot].cpu(), qkv[..., 2 * H:])
    print("worst", worst)


def test_arguments_are_refused_before_any_launch(cuda):
    from dynamic_asr_eval_amd import ops
    cnt = _counter(cuda)
    z = lambda *s: torch.zeros(*s, device=cuda)                                                               # noqa: E731
    with pytest.raises(ops.DynError):                       # caches of another ring length
        ops.stream_attn(z(1, 3, 3 * 64), z(64), z(64), z(11, 64), z(1, 2, 3, 64), z(1, 2, 3, 64), cnt, 1, 2)
    with pytest.raises(ops.DynError, match="LDS"):          # 4096 keys of 128 floats do not fit a CU
        ops.stream_attn(z(1, 64, 3 * 128), z(128), z(128), z(64 * 64 + 63, 128), z(1, 64, 64, 128), z(1, 64, 64, 128), cnt, 1, 63)
    with pytest.raises(ops.DynError):                       # a state of the wrong shape
        ops.stream_convmod_k9(z(1, 3, 512), z(256, 9), None, z(256), z(256), z(1, 1, 8, 256), cnt)
    with pytest.raises(ops.DynError):                       # a later chunk of one row has no output
        ops.stream_conv2d_first(z(1, 1, 80), z(32, 3, 3), z(32), z(2, 1, 80), cnt, False)
    assert int(cnt.item()) == 0
