"""Float64 parity of the kernels that only whole-model tests (2e-4 on logits, 3e-3 on gradients) or self-comparisons used to reach: every
HIP kernel here against tests/kernel_refs.py (float64 restatements, themselves held to torch's ops in tests/test_kernel_refs_cpu.py), at
the smallest shapes that take each code path.

Tolerances.  Where tests/test_ops_gpu.py already asserts one for the same kind of result it is used and named (1e-6 elementwise, 2e-6
elementwise backward / softmax, 5e-6 norm forward, 2e-5 norm dx and convolution forward / dgrad, 5e-4 norm weight gradients at 531 rows and
3e-4 conv taps at 400 rows, both scaled by sqrt(rows) past that: kernel_refs.wgrad_tol).  Where the inputs make that tolerance meaningless
(offsets, 1 / sqrt(eps) amplification, long sums) the bound is MEASURED in the test: 4 x the error of torch's fp32 CPU result of the same
op on the same inputs against float64, plus that floor (kernel_refs.measured_tol).  Integer and copy kernels are bit-exact.
Every check prints `name: kernel error | torch fp32 error | bound` before it asserts (pytest -s shows them)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(name, got, want, tol, e32=None, rel=False):
    err = K.max_err(got, want, rel)
    print(f"  {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")
    assert err <= tol, f"{name}: {'rel' if rel else 'abs'} err {err} > {tol} (torch fp32: {e32})"


def _measured(name, got, torch32, want, floor, rel=False):
    tol, e32 = K.measured_tol(torch32, want, floor, rel)
    _check(name, got, want, tol, e32, rel)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------- column norm
def _colnorm_torch_fp32_bwd(x, gamma, beta, dy, eps):
    C = x.shape[2]
    xr, gr, br = (t.clone().requires_grad_() for t in (x, gamma, beta))
    F.group_norm(xr.transpose(1, 2), C, gr, br, eps).transpose(1, 2).backward(dy)
    return xr.grad, gr.grad, br.grad


def _colnorm_case(cuda, x, gamma, beta, dy, eps, valid=None, offset=False):
    """ops.colnorm / ops.colnorm_bwd on x (statistics over the first `valid` rows when given) against float64 on the cut tensor."""
    from dynamic_asr_eval_amd import ops
    B, T, C = x.shape
    n = T if valid is None else valid
    xc, dyc = x[:, :n].contiguous(), dy[:, :n].contiguous()
    y64, mean64, rstd64 = K.colnorm_ref(xc, gamma, beta, eps)
    dx64, dg64, db64 = K.colnorm_bwd_ref(xc, gamma, dyc, eps)
    y32, mean32, rstd32 = K.colnorm_torch_fp32(xc, gamma, beta, eps)
    dx32, _, _ = _colnorm_torch_fp32_bwd(xc, gamma, beta, dyc, eps)
    vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
    xd, gd, bd, dyd = (t.to(cuda) for t in (x, gamma, beta, dy))
    y, mean, rstd = ops.colnorm(xd, gd, bd, eps, valid=vd)
    _measured("y", y[:, :n], y32, y64, 5e-6)                      # 5e-6: the norm-forward tolerance of test_layernorm_rmsnorm
    _measured("mean", mean, mean32, mean64, 5e-6)
    _measured("rstd (rel)", rstd, rstd32, rstd64, 5e-6, rel=True)
    wtol = K.wgrad_tol(5e-4, B * n, 531)                          # 5e-4 at 531 rows: "ln dgamma" / "ln dbeta" there
    gtol = K.wgrad_tol_ill_conditioned(5e-4, B * n) if offset else wtol   # the fp32 mean the backward is GIVEN shifts xhat: see there
    old_g, old_b = torch.full((C,), 0.75), torch.full((C,), -1.25)
    for wb in (0.0, 1.0):
        dgam, dbet = old_g.to(cuda), old_b.to(cuda)
        dx = ops.colnorm_bwd(xd, gd, mean, rstd, dyd, dgam, dbet, wgrad_beta=wb, valid=vd)
        _measured(f"dx (wgrad_beta {wb:g})", dx[:, :n], dx32, dx64, 2e-5)   # 2e-5: "ln dx" there
        _check(f"dgamma (wgrad_beta {wb:g})", dgam, dg64 + wb * old_g.double(), gtol)
        _check(f"dbeta (wgrad_beta {wb:g})", dbet, db64 + wb * old_b.double(), wtol)
    if n < T:
        assert torch.equal(dx[:, n:], torch.zeros_like(dx[:, n:])), "dx past the valid rows must be exactly 0"
        assert torch.isfinite(y[:, n:]).all(), "y past the valid rows must be finite"


# Measured on the MI355X against float64, kernel | torch fp32 CPU (the bound of y, mean, rstd, dx is 4 x the second + its floor).
# `before` is y of the kernel before its statistics were made stable (E[x^2] - mean^2 from fp32 running sums): it missed the bound on every
# offset row; at T = 1 it missed on rstd (relative 3.0e-3 zero-mean, 0.98 offset; y there is beta either way).
#   case                        y                    mean                 rstd (rel)           dx                   dgamma   (its bound)  before
#   (2, 1, 3)       zero-mean   0.0e+00 | 7.2e-06    0.0e+00 | 0.0e+00    5.4e-08 | 4.2e-08    0.0e+00 | 3.1e-05    0.0e+00  (5.0e-04)    rstd
#   (2, 1, 3)       offset      0.0e+00 | 9.6e-03    0.0e+00 | 0.0e+00    5.4e-08 | 4.2e-08    0.0e+00 | 0.0e+00    0.0e+00  (7.1e-04)    rstd
#   (3, 63, 5)      zero-mean   3.3e-06 | 2.3e-07    3.3e-07 | 3.2e-08    8.1e-07 | 8.3e-08    2.5e-06 | 4.3e-07    1.4e-05  (5.0e-04)
#   (3, 63, 5)      offset      2.2e-06 | 8.7e-05    2.7e-05 | 2.7e-05    6.7e-07 | 5.9e-06    1.4e-05 | 3.2e-05    2.4e-04  (6.9e-03)    7.4e-01
#   (2, 64, 257)    zero-mean   4.5e-06 | 7.7e-07    5.1e-07 | 5.1e-08    2.0e-06 | 1.0e-07    4.8e-06 | 9.0e-07    1.4e-05  (5.0e-04)
#   (2, 64, 257)    offset      8.5e-06 | 1.8e-04    3.1e-05 | 9.1e-05    1.5e-06 | 1.7e-05    4.2e-05 | 1.7e-04    5.8e-04  (5.7e-03)    6.7e+00
#   (2, 65, 64)     zero-mean   1.9e-06 | 5.1e-07    2.6e-07 | 4.5e-08    7.2e-07 | 1.2e-07    1.5e-06 | 5.1e-07    6.9e-06  (5.0e-04)
#   (2, 65, 64)     offset      1.2e-06 | 1.4e-04    3.0e-05 | 7.0e-05    3.7e-07 | 1.3e-05    2.6e-05 | 1.0e-04    4.2e-04  (5.7e-03)    5.7e-01
#   (1, 300, 512)   zero-mean   2.1e-06 | 1.1e-06    2.1e-07 | 3.1e-08    4.9e-07 | 1.5e-07    2.3e-06 | 1.1e-06    1.6e-05  (5.0e-04)
#   (1, 300, 512)   offset      2.6e-06 | 2.7e-04    3.1e-05 | 1.1e-04    5.6e-07 | 9.3e-06    1.7e-05 | 1.4e-04    1.2e-03  (8.7e-03)    6.8e-01
#   (1, 16500, 8)   zero-mean   7.1e-07 | 5.5e-07    1.3e-08 | 6.7e-09    7.3e-08 | 9.5e-08    6.8e-07 | 7.6e-07    9.2e-05  (2.8e-03)
#   (1, 16500, 8)   offset      8.0e-07 | 5.5e-06    2.8e-05 | 3.3e-05    5.8e-08 | 3.2e-07    1.5e-06 | 5.8e-05    2.3e-03  (6.4e-02)    5.1e-02
#   (1, 480000, 1)  zero-mean   4.3e-07 | 1.9e-07    2.3e-10 | 2.2e-12    7.2e-08 | 5.0e-09    4.2e-05 | 1.6e-05    5.8e-04  (1.5e-02)
#   (1, 480000, 1)  offset      3.8e-07 | 2.0e-06    8.7e-10 | 5.9e-08    6.5e-08 | 8.8e-08    4.0e-05 | 2.4e-04    4.7e-04  (3.5e-01)    1.3e-03
#   valid 1         offset      0.0e+00 | 2.0e-02    0.0e+00 | 0.0e+00    5.4e-08 | 4.2e-08    0.0e+00 | 6.1e-05    0.0e+00  (7.1e-04)    rstd
#   valid 64        offset      2.2e-06 | 2.0e-04    3.1e-05 | 8.4e-05    6.1e-07 | 1.9e-05    3.4e-05 | 2.4e-04    3.6e-04  (5.7e-03)    1.7e+00
#   valid 65        offset      4.5e-06 | 2.0e-04    2.8e-05 | 8.7e-05    9.6e-07 | 1.3e-05    2.6e-05 | 1.6e-04    6.0e-04  (5.7e-03)    1.4e+00
#   valid 211       offset      5.3e-06 | 9.8e-05    3.0e-05 | 5.6e-05    7.1e-07 | 9.7e-06    2.0e-05 | 8.0e-05    7.8e-04  (1.0e-02)    6.9e-01
#   valid 300       offset      2.1e-06 | 9.5e-05    3.0e-05 | 8.8e-05    4.8e-07 | 7.4e-06    1.6e-05 | 8.7e-05    8.0e-04  (1.2e-02)    5.5e-01
# y: the forward also subtracts what fp32 cannot hold of the mean (csrc/wav2vec2.hip, mean_lo), so y does not carry the mean's rounding
#    times rstd (3e-5 at mean / std = 1000, which torch's y = x * scale + bias form pays on most inputs and happens not to at (1, 16500, 8)).
# mean: 3.05e-05 is ulp(1000) / 2, the most a correctly rounded fp32 mean can be off; the kernel's error stays at or under it and under torch's.
# dgamma on OFFSET inputs: the backward is GIVEN the fp32 mean, so 5e-4 * sqrt(rows / 531) is out of reach of any kernel with this interface
#    (5.8e-4 .. 1.2e-3 above against 5.0e-4 .. 5.3e-4 at the 300-row-and-shorter shapes); the bound is 5e-4 * sqrt(rows) there
#    (kernel_refs.wgrad_tol_ill_conditioned).  torch's fp32 dgamma on these inputs: 7.3e-04 (3, 63, 5), 2.8e-03, 2.0e-03, 9.6e-03, 2.0e-01
#    (1, 16500, 8), 4.3e-01 (1, 480000, 1); valid: 3.5e-02, 2.7e-03, 2.4e-03, 5.2e-03, 1.0e-02 — so "4 x torch + 5e-4" would be the looser bound.
@pytest.mark.parametrize("offset", [False, True], ids=["zero-mean", "offset"])
@pytest.mark.parametrize("shape", K.COLNORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_colnorm(cuda, shape, offset):
    """dyn_colnorm_fwd_len / dyn_colnorm_bwd_len: y, mean, rstd, dx, dgamma, dbeta against float64.  (1, 16500, 8) has more than 256 x 64
    rows (the rows-per-chunk > 64 path), (1, 480000, 1) with eps 1e-7 is the waveform normaliser.  E[x^2] - mean^2 from fp32 running sums
    fails every offset case here (tests/test_kernel_refs_cpu.py replays it)."""
    x, gamma, beta, dy = K.colnorm_inputs(shape, offset)
    _colnorm_case(cuda, x, gamma, beta, dy, K.colnorm_eps(shape), offset=offset)


@pytest.mark.parametrize("valid", [1, 64, 65, 211, 300])
def test_colnorm_valid_rows(cuda, valid):
    """The device-side row count on an offset input: statistics, y[:, :n], dx[:, :n] and the affine gradients against float64 on the cut
    tensor (chunks of 60 rows: 64 and 65 end inside the second chunk, 1 leaves four chunks without a row); dx[:, n:] == 0, y[:, n:] finite."""
    x, gamma, beta, dy = K.colnorm_inputs((2, 300, 64), True, seed=valid)
    _colnorm_case(cuda, x, gamma, beta, dy, 1e-5, valid=valid, offset=True)


# ----------------------------------------------------------------------------------------------------------- gelu
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 300])       # the last is past the 4096-block grid cap: the stride loop
def test_gelu(cuda, n):
    from dynamic_asr_eval_amd import ops
    x, dy = K.gelu_inputs(n)
    _check("gelu", ops.gelu(x.to(cuda)), K.gelu_ref(x), 1e-6)                          # "silu" 1e-6 in test_silu_glu_axpby
    _check("gelu_bwd", ops.gelu_bwd(x.to(cuda), dy.to(cuda)), K.gelu_bwd_ref(x, dy), 2e-6)   # "silu_bwd" 2e-6


# ----------------------------------------------------------------------------------------------------------- weight norm
# Measured on the MI355X, kernel | torch fp32:   w                    dv (beta 0)          dv (beta 1)
#   (5, 3, 4)                                  6.5e-08 | 9.9e-08    7.2e-08 | 5.2e-08    1.3e-07 | 1.3e-07
#   (17, 3, 4)                                 3.8e-08 | 6.7e-08    4.4e-08 | 1.1e-07    1.3e-07 | 1.1e-07
#   (16, 128, 48)                              6.9e-08 | 5.2e-08    7.9e-08 | 5.3e-08    2.3e-07 | 2.3e-07
#   (9, 300, 1)                                3.4e-07 | 4.0e-07    7.6e-07 | 5.3e-07    8.9e-07 | 5.8e-07
#   (2100, 2, 2)                               1.4e-08 | 6.3e-08    1.4e-08 | 8.8e-08    1.2e-07 | 1.4e-07
@pytest.mark.parametrize("rows,kw,cg", [(5, 3, 4), (17, 3, 4), (16, 128, 48), (9, 300, 1), (2100, 2, 2)])
def test_weight_norm(cuda, rows, kw, cg):
    """One block, a ragged last block, kw * cg == WN_MAX, kw > 256 threads, the 256-block cap; beta 0 and 1 onto non-zero dv / dg."""
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(3000 + rows + kw)
    v, g, dw = torch.randn(rows, kw, cg, generator=g_), torch.randn(kw, generator=g_) + 2.0, torch.randn(rows, kw, cg, generator=g_)
    vr, gr = v.clone().requires_grad_(), g.clone().requires_grad_()
    w32 = gr[None, :, None] * vr / vr.pow(2).sum((0, 2), keepdim=True).sqrt()
    w32.backward(dw)
    dv64, dg64 = K.weight_norm_bwd_ref(v, g, dw)
    vd, gd, dwd = v.to(cuda), g.to(cuda), dw.to(cuda)
    _measured("w", ops.weight_norm(vd, gd), w32, K.weight_norm_ref(v, g), 1e-6)       # elementwise floor
    old_v, old_g = torch.randn(rows, kw, cg, generator=g_), torch.randn(kw, generator=g_)
    for beta in (0.0, 1.0):
        dv, dg = old_v.to(cuda), old_g.to(cuda)
        ops.weight_norm_bwd(vd, gd, dwd, dv, dg, beta=beta)
        _measured(f"dv (beta {beta:g})", dv, vr.grad + beta * old_v, dv64 + beta * old_v.double(), 2e-6)   # elementwise backward floor
        _check(f"dg (beta {beta:g})", dg, dg64 + beta * old_g.double(), K.wgrad_tol(5e-4, rows * cg, 531))


def test_weight_norm_rejects_a_tap_row_past_its_lds_buffer(cuda):
    """kw * cg = 6145 > WN_MAX: an argument check, nothing is launched."""
    from dynamic_asr_eval_amd import ops
    v = torch.ones(1, 6145, 1, device=cuda); g = torch.ones(6145, device=cuda)
    with pytest.raises(ops.DynError):
        ops.weight_norm(v, g)
    with pytest.raises(ops.DynError):
        ops.weight_norm_bwd(v, g, v.clone(), torch.zeros_like(v), torch.zeros_like(g))


# ----------------------------------------------------------------------------------------------------------- strided conv1d
# Measured on the MI355X, kernel | torch fp32:   y                    dx
#   (2, 400, 1, 32, 10, 5)                     5.0e-07 | 7.1e-07    1.4e-06 | 2.2e-06
#   (2, 37, 32, 48, 3, 2)                      3.7e-06 | 1.9e-06    2.9e-06 | 2.8e-06
#   (1, 38, 32, 48, 2, 2)                      1.7e-06 | 2.6e-06    1.6e-06 | 1.6e-06
#   (1, 10, 1, 32, 10, 5)                      1.1e-07 | 5.9e-08    1.7e-07 | 4.1e-07
#   (2, 403, 1, 32, 10, 5)                     4.9e-07 | 3.9e-07    1.6e-06 | 2.2e-06
@pytest.mark.parametrize("B,T,Cin,Cout,kw,stride", [(2, 400, 1, 32, 10, 5),      # row stride 5 floats: not 16-byte aligned
                                                    (2, 37, 32, 48, 3, 2), (1, 38, 32, 48, 2, 2),
                                                    (1, 10, 1, 32, 10, 5),       # Tout = 1
                                                    (2, 403, 1, 32, 10, 5)])     # (T - kw) % stride != 0: dx tail rows exactly 0
def test_conv1d(cuda, B, T, Cin, Cout, kw, stride):
    """The implicit GEMM over overlapping rows (forward, weight gradient) and GEMM + dyn_col2im_1d (input gradient)."""
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(4000 + T + kw)
    x, w = torch.randn(B, T, Cin, generator=g_), torch.randn(Cout, kw * Cin, generator=g_) * 0.3
    Tout = (T - kw) // stride + 1
    dy = torch.randn(B, Tout, Cout, generator=g_)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y32 = F.conv1d(xr.transpose(1, 2), K.torch_conv_weight(wr, kw), stride=stride).transpose(1, 2)
    y32.backward(dy)
    xd, wd, dyd = x.to(cuda), w.to(cuda), dy.to(cuda)
    _measured("y", ops.conv1d(xd, wd, kw, stride), y32, K.conv1d_ref(x, w, kw, stride), 2e-5)       # "dwconv1d fwd" 2e-5
    dw64 = K.conv1d_wgrad_ref(x, dy, kw, stride)
    old = torch.randn(Cout, kw * Cin, generator=g_)
    for beta in (0.0, 1.0):
        dw = old.to(cuda)
        ops.conv1d_wgrad(xd, dyd, dw, kw, stride, beta=beta)
        _check(f"dw (beta {beta:g})", dw, dw64 + beta * old.double(), K.wgrad_tol(3e-4, B * Tout, 400))   # "dwconv1d wgrad" 3e-4 at 400 rows
    dx = ops.conv1d_dgrad(dyd, wd, T, Cin, kw, stride)
    _measured("dx", dx, xr.grad, K.conv1d_dgrad_ref(dy, w, T, Cin, kw, stride), 2e-5)               # "dwconv1d dgrad" 2e-5
    covered = (Tout - 1) * stride + kw
    assert torch.equal(dx[:, covered:], torch.zeros_like(dx[:, covered:])), "rows no window covers must be exactly 0"


# ----------------------------------------------------------------------------------------------------------- grouped positional conv
GROUP_SHAPES = [(2, 5, 32, 4, 8), (1, 50, 32, 4, 8), (2, 7, 48, 16, 64)]      # (B, T, C, G, pad); the first has T < pad


@pytest.mark.parametrize("B,T,C,G,pad", GROUP_SHAPES)
def test_group_pack_unpack_are_bit_exact(cuda, B, T, C, G, pad):
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(5000 + T + C)
    cg = C // G
    x = torch.randn(B, T, C, generator=g_)
    assert _bits_equal(ops.group_pack(x.to(cuda), G, pad), K.group_pack_ref(x, G, pad))
    for Tg in (T, T + 1, T + 5):                                   # Tg > T: rows past T are dropped (unpack) / zero (pack_grad)
        yg, bias = torch.randn(B, G, Tg, cg, generator=g_), torch.randn(C, generator=g_)
        assert _bits_equal(ops.group_unpack(yg.to(cuda), None, T, C), K.group_unpack_ref(yg, None, T, C))
        assert _bits_equal(ops.group_unpack(yg.to(cuda), bias.to(cuda), T, C), K.group_unpack_ref(yg, bias, T, C))
        assert _bits_equal(ops.group_pack_grad(x.to(cuda), G, Tg), K.group_pack_grad_ref(x, G, Tg))
    dxg, old = torch.randn(B, G, T + 2 * pad, cg, generator=g_), torch.randn(B, T, C, generator=g_)
    for beta in (0.0, 1.0):
        dx = old.to(cuda)
        ops.group_unpack_grad(dxg.to(cuda), dx, pad, beta=beta)
        assert _bits_equal(dx, K.group_unpack_grad_ref(dxg, old, pad, beta)), f"unpack_grad beta {beta}"


# Measured on the MI355X, kernel | torch fp32:   y                    dx
#   (2, 5, 32, 4, 8)                           5.7e-07 | 7.8e-07    2.8e-07 | 2.5e-07
#   (1, 50, 32, 4, 8)                          1.7e-06 | 3.8e-06    9.8e-07 | 2.6e-06
#   (2, 7, 48, 16, 64)                         6.3e-07 | 3.9e-07    4.2e-07 | 4.2e-07
@pytest.mark.parametrize("B,T,C,G,pad", GROUP_SHAPES)
def test_grouped_conv_composition_drops_the_last_frame(cuda, B, T, C, G, pad):
    """pack -> conv1d per group -> unpack against float64 F.conv1d(groups=G, padding=kw // 2)[..., :-1] (an even kernel: the reference
    model drops the last frame) and pack_grad -> conv1d_dgrad per group -> unpack_grad against its input gradient."""
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(6000 + T + C)
    kw, cg = 2 * pad, C // G
    x, wg, bias = torch.randn(B, T, C, generator=g_), torch.randn(G, cg, kw * cg, generator=g_) * 0.2, torch.randn(C, generator=g_)
    dy = torch.randn(B, T, C, generator=g_)

    def torch_op(x_, wg_, bias_):
        return F.conv1d(x_.transpose(1, 2), K.torch_grouped_weight(wg_, kw), bias_, padding=kw // 2, groups=G)[..., :-1].transpose(1, 2)

    x64 = x.double().requires_grad_()
    y64 = torch_op(x64, wg.double(), bias.double())
    y64.backward(dy.double())
    x32 = x.clone().requires_grad_()
    y32 = torch_op(x32, wg, bias)
    y32.backward(dy)
    xg = ops.group_pack(x.to(cuda), G, pad)
    wd = wg.to(cuda)
    yg = torch.stack([ops.conv1d(xg[:, g].contiguous(), wd[g], kw, 1) for g in range(G)], 1)          # [B, G, T + 1, cg]
    y = ops.group_unpack(yg.contiguous(), bias.to(cuda), T, C)
    _measured("y", y, y32, y64.detach(), 2e-5)                                                       # convolution forward floor
    dyg = ops.group_pack_grad(dy.to(cuda), G, T + 1)
    dxg = torch.stack([ops.conv1d_dgrad(dyg[:, g].contiguous(), wd[g], T + 2 * pad, cg, kw, 1) for g in range(G)], 1)
    dx = ops.group_unpack_grad(dxg.contiguous(), torch.empty(B, T, C, device=cuda), pad, beta=0.0)
    _measured("dx", dx, x32.grad, x64.grad, 2e-5)                                                    # convolution dgrad floor


# ----------------------------------------------------------------------------------------------------------- channel affine
# Measured on the MI355X, kernel | torch fp32 (|y| reaches 1e3 on the var = 1e-9 channels: 316 x |x - mean| x |weight|):
#   (rows, C)     y                    y (bias None)        dx (dx_beta 1)       dweight (wgrad_beta 0)   dweight (wgrad_beta 1)
#   (1, 256)      8.6e-05 | 2.1e-04    6.2e-05 | 2.6e-04    1.1e-04 | 1.1e-04    8.4e-05 | 1.3e-04        5.7e-05 | 1.8e-04
#   (1, 300)      7.3e-05 | 1.4e-04    7.4e-05 | 1.1e-04    7.5e-05 | 7.5e-05    9.7e-05 | 9.7e-05        9.5e-05 | 9.5e-05
#   (513, 256)    5.3e-04 | 3.5e-04    5.2e-04 | 4.0e-04    3.3e-04 | 3.3e-04    4.1e-03 | 2.6e-03        4.7e-03 | 2.7e-03
#   (513, 300)    5.0e-04 | 4.6e-04    4.5e-04 | 5.0e-04    2.1e-04 | 2.1e-04    6.6e-03 | 3.5e-03        6.4e-03 | 2.6e-03
# dweight sums terms of size 316, not O(1), so the plain 5e-4 does not apply to it: 4 x torch + 5e-4 (1.1e-2 .. 1.5e-2 at 513 rows).
@pytest.mark.parametrize("C", [256, 300])                  # 300: the column loop
@pytest.mark.parametrize("rows", [1, 513])                 # 513: more rows than the 512 workgroups
def test_chanaffine(cuda, rows, C):
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(7000 + rows + C)
    eps = 1e-5
    x, w, b, dy = (torch.randn(s_, generator=g_) for s_ in ((rows, C), (C,), (C,), (rows, C)))
    mean, var = torch.randn(C, generator=g_), torch.rand(C, generator=g_) + 0.5
    var[::7] = 1e-9                                            # var near 0: 1 / sqrt(eps) = 316 amplifies every rounding, hence measured bounds
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
    y32 = F.batch_norm(xr, mean, var, wr, br, training=False, eps=eps)
    y32.backward(dy)
    xd, md, vd, wd, bd, dyd = (t.to(cuda) for t in (x, mean, var, w, b, dy))
    _measured("y", ops.chanaffine(xd, md, vd, wd, bd, eps), y32, K.chanaffine_ref(x, mean, var, w, b, eps), 5e-6)
    _measured("y (bias None)", ops.chanaffine(xd, md, vd, wd, None, eps), y32.detach() - b, K.chanaffine_ref(x, mean, var, w, None, eps), 5e-6)
    dx64, dw64, db64 = K.chanaffine_bwd_ref(x, mean, var, w, dy, eps)
    old_x, old_w, old_b = torch.randn(rows, C, generator=g_), torch.randn(C, generator=g_), torch.randn(C, generator=g_)
    wtol = K.wgrad_tol(5e-4, rows, 531)
    for wb in (0.0, 1.0):
        dx, dwt, dbs = old_x.to(cuda), old_w.to(cuda), old_b.to(cuda)
        ops.chanaffine_bwd(xd, md, vd, wd, dyd, dx, dwt, dbs, eps, dx_beta=1.0, wgrad_beta=wb)
        _measured("dx (dx_beta 1)", dx, xr.grad + old_x, dx64 + old_x.double(), 2e-5)
        tol, e32 = K.measured_tol(wr.grad + wb * old_w, dw64 + wb * old_w.double(), wtol)          # terms are O(316), not O(1)
        _check(f"dweight (wgrad_beta {wb:g})", dwt, dw64 + wb * old_w.double(), tol, e32)
        _check(f"dbias (wgrad_beta {wb:g})", dbs, db64 + wb * old_b.double(), wtol)


# ----------------------------------------------------------------------------------------------------------- row norms
# rows: fewer than waves; more than 256 blocks x 4 rows.  C = 1280: the instance between the two, at the row count that idles a wave.
@pytest.mark.parametrize("rows,C", [(r, c) for c in (512, 2048) for r in (1, 3, 1029)] + [(3, 1280)], ids=lambda v: str(v))
def test_layernorm_rmsnorm_row_edges(cuda, rows, C):
    """The tolerances of test_ops_gpu.py::test_layernorm_rmsnorm on its input distribution, at the widths and row counts it does not run;
    plus the residual variant of layernorm_bwd (dx = grad + dx_in, dx_in untouched)."""
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(8000 + rows + C)
    x = torch.randn(rows, C, generator=g_) * 2 + 0.3
    g, b, dy, other = (torch.randn(s_, generator=g_) for s_ in ((C,), (C,), (rows, C), (rows, C)))
    xd, gd, bd, dyd = (t.to(cuda) for t in (x, g, b, dy))
    wtol = K.wgrad_tol(5e-4, rows, 531)
    y64, mean64, rstd64 = K.layernorm_ref(x, g, b, 1e-5)
    dx64, dg64, db64 = K.layernorm_bwd_ref(x, g, dy, 1e-5)
    y, mean, rstd = ops.layernorm(xd, gd, bd, 1e-5)
    _check("ln y", y, y64, 5e-6); _check("ln mean", mean, mean64, 5e-6); _check("ln rstd (rel)", rstd, rstd64, 5e-6, rel=True)
    dx, dgam, dbet = torch.ones(rows, C, device=cuda), torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    ops.layernorm_bwd(xd, gd, mean, rstd, dyd, dx, dgam, dbet, dx_beta=1.0, wgrad_beta=0.0)
    _check("ln dx (dx_beta 1)", dx, dx64 + 1.0, 2e-5); _check("ln dgamma", dgam, dg64, wtol); _check("ln dbeta", dbet, db64, wtol)
    od = other.to(cuda)
    dx, dgam, dbet = torch.full((rows, C), 7.0, device=cuda), torch.ones(C, device=cuda), torch.ones(C, device=cuda)
    ops.layernorm_bwd(xd, gd, mean, rstd, dyd, dx, dgam, dbet, dx_beta=1.0, wgrad_beta=1.0, dx_in=od)
    _check("ln dx (residual)", dx, dx64 + other.double(), 2e-5)
    assert _bits_equal(od, other), "the residual source must be left unchanged"
    _check("ln dgamma (beta 1)", dgam, dg64 + 1.0, wtol); _check("ln dbeta (beta 1)", dbet, db64 + 1.0, wtol)
    y64, rstd64 = K.rmsnorm_ref(x, g, 1e-5)
    dx64, dg64 = K.rmsnorm_bwd_ref(x, g, dy, 1e-5)
    y, rstd = ops.rmsnorm(xd, gd, 1e-5)
    _check("rms y", y, y64, 5e-6); _check("rms rstd (rel)", rstd, rstd64, 5e-6, rel=True)
    dx, dgam = torch.zeros(rows, C, device=cuda), torch.zeros(C, device=cuda)
    ops.rmsnorm_bwd(xd, gd, rstd, dyd, dx, dgam, dx_beta=0.0, wgrad_beta=0.0)
    _check("rms dx", dx, dx64, 2e-5); _check("rms dgamma", dgam, dg64, wtol)


# Measured on the MI355X, kernel | torch fp32: y 2.6e-05 | 2.4e-05, mean 9.7e-06 | 9.9e-06, rstd (rel) 9.6e-08 | 8.4e-08, dx 1.7e-06 | 7.5e-06
# (ulp(100) / 2 = 3.8e-6 in x - mean, times |gamma| up to 3.5: no cancellation of the variance, which would show in rstd).
def test_layernorm_with_a_large_mean(cuda):
    """mean 100, std 1: the in-register two-pass row statistics do not cancel (measured bounds: x - mean alone carries ulp(100) / 2)."""
    from dynamic_asr_eval_amd import ops
    rows, C = 37, 512
    g_ = K.gen(8100)
    x = torch.randn(rows, C, generator=g_) + 100.0
    g, b, dy = torch.randn(C, generator=g_), torch.randn(C, generator=g_), torch.randn(rows, C, generator=g_)
    xr, gr, br = (t.clone().requires_grad_() for t in (x, g, b))
    y32 = F.layer_norm(xr, (C,), gr, br, 1e-5)
    y32.backward(dy)
    y64, mean64, rstd64 = K.layernorm_ref(x, g, b, 1e-5)
    y, mean, rstd = ops.layernorm(x.to(cuda), g.to(cuda), b.to(cuda), 1e-5)
    _measured("y", y, y32, y64, 5e-6)
    _measured("mean", mean, x.mean(-1), mean64, 5e-6)
    _measured("rstd (rel)", rstd, torch.rsqrt(x.var(-1, unbiased=False) + 1e-5), rstd64, 5e-6, rel=True)
    dx, dgam, dbet = torch.zeros(rows, C, device=cuda), torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    ops.layernorm_bwd(x.to(cuda), g.to(cuda), mean, rstd, dy.to(cuda), dx, dgam, dbet, dx_beta=0.0, wgrad_beta=0.0)
    dx64, dg64, db64 = K.layernorm_bwd_ref(x, g, dy, 1e-5)
    _measured("dx", dx, xr.grad, dx64, 2e-5)
    _check("dgamma", dgam, dg64, 5e-4); _check("dbeta", dbet, db64, 5e-4)


# ----------------------------------------------------------------------------------------------------------- masked softmax, entropy
@pytest.mark.parametrize("L", [64, 300, 1100])
def test_softmax_with_valid_columns(cuda, L):
    from dynamic_asr_eval_amd import ops
    x = torch.randn(9, L, generator=K.gen(9000 + L)) * 4
    for valid in (1, L - 1, L):
        y = ops.softmax(x.to(cuda), valid=torch.tensor([valid], dtype=torch.int32, device=cuda))
        _check(f"softmax valid {valid}", y, K.masked_softmax_ref(x, valid), 2e-6)          # "softmax" 2e-6 in test_softmax_family
        assert torch.equal(y[:, valid:], torch.zeros_like(y[:, valid:])), "masked columns must be exactly 0"


# Measured on the MI355X, kernel | torch fp32:   entropy              grad (scale 1 / 7)
#   L = 1                                      0.0e+00 | 0.0e+00    0.0e+00 | 0.0e+00
#   L = 129                                    1.3e-07 | 1.2e-07    9.1e-09 | 8.0e-09
#   L = 300                                    3.1e-07 | 2.1e-07    1.1e-08 | 6.1e-09
#   L = 4096                                   3.0e-07 | 3.5e-07    9.3e-09 | 9.3e-09
@pytest.mark.parametrize("L", [1, 129, 300, 4096])
def test_entropy_grad(cuda, L):
    """dyn_entropy_grad against float64 autograd of (-(p * logp).sum(-1)).mean() through log_softmax (kernel_refs.entropy_grad_ref is held
    to exactly that in the CPU tests); through the wrapper (ld == L) and through the C-ABI with a padded row stride."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    rows = 7
    logp = F.log_softmax(torch.randn(rows, L, generator=K.gen(9100 + L), dtype=torch.float64) * 3, -1).float()
    scale = 1.0 / rows
    g64, H64 = K.entropy_grad_ref(logp, scale)
    p32 = logp.exp()
    H32 = -(p32 * logp).sum(-1)
    g32 = -p32 * (logp + H32[:, None]) * scale
    grad, ent = ops.entropy_grad(logp.to(cuda), scale)
    _measured("entropy", ent, H32, H64, 2e-6)                      # a softmax-family reduction: 2e-6 floor
    _measured("grad", grad, g32, g64, 2e-6 * scale)
    ld = L + 3
    padded = torch.full((rows, ld), float("nan"), device=cuda)
    padded[:, :L] = logp.to(cuda)
    gp, ep = torch.full((rows, ld), 5.0, device=cuda), torch.empty(rows, device=cuda)
    check(load().dyn_entropy_grad(padded.data_ptr(), gp.data_ptr(), ep.data_ptr(), rows, L, ld, scale, _stream()), "dyn_entropy_grad")
    assert torch.equal(gp[:, :L], grad) and torch.equal(ep, ent), "a padded row stride must not change a value"
    assert torch.equal(gp[:, L:], torch.full((rows, 3), 5.0, device=cuda)), "the padding columns must not be written"


# ----------------------------------------------------------------------------------------------------------- encoder-decoder pieces
# Measured on the MI355X, kernel | torch fp32, dtable: d = 256: 1.8e-07 | 1.8e-07 (beta 0), 3.6e-07 | 4.2e-07 (beta 1);
#                                                     d = 300: 2.4e-07 | 2.4e-07 (beta 0), 4.8e-07 | 3.6e-07 (beta 1)
@pytest.mark.parametrize("dm", [256, 300])
def test_embedding_fwd_bwd(cuda, dm):
    from dynamic_asr_eval_amd._lib import check, load
    L = load()
    vocab, S, period = 11, 9, 4
    g_ = K.gen(9200 + dm)
    ids = torch.tensor([3, 3, 0, 10, 7, 3, 0, 1, 10], dtype=torch.int32)      # repeats; rows 2, 4, 5, 6, 8, 9 are never selected
    table, pos, dy, old = (torch.randn(s_, generator=g_) for s_ in ((vocab, dm), (period, dm), (S, dm), (vocab, dm)))
    idd, td, pd, dyd = ids.to(cuda), table.to(cuda), pos.to(cuda), dy.to(cuda)
    out = torch.empty(S, dm, device=cuda)
    check(L.dyn_embedding_fwd(idd.data_ptr(), td.data_ptr(), pd.data_ptr(), out.data_ptr(), S, dm, vocab, period, _stream()), "dyn_embedding_fwd")
    _check("embedding + pos (S > pos_period wraps)", out, K.embedding_ref(ids, table, pos, period), 1e-6)
    assert _bits_equal(out, table[ids.long()] + pos[torch.arange(S) % period]), "one fp32 add per element"
    check(L.dyn_embedding_fwd(idd.data_ptr(), td.data_ptr(), None, out.data_ptr(), S, dm, vocab, 0, _stream()), "dyn_embedding_fwd")
    assert _bits_equal(out, table[ids.long()]), "pos null: a copy"
    unused = [v for v in range(vocab) if v not in ids.tolist()]
    for beta in (0.0, 1.0):
        dt = old.to(cuda)
        check(L.dyn_embedding_bwd(idd.data_ptr(), dyd.data_ptr(), dt.data_ptr(), S, dm, vocab, beta, _stream()), "dyn_embedding_bwd")
        t32 = (beta * old).index_add(0, ids.long(), dy)
        _measured(f"dtable (beta {beta:g})", dt, t32, K.embedding_bwd_ref(ids, dy, old, beta), 1e-6)
        assert _bits_equal(dt[unused], old[unused] if beta else torch.zeros(len(unused), dm)), "a vocabulary row no id selects must be exactly beta * old"
    dt = old.to(cuda)
    check(L.dyn_embedding_bwd(idd.data_ptr(), dyd.data_ptr(), dt.data_ptr(), 0, dm, vocab, 0.0, _stream()), "dyn_embedding_bwd")
    assert torch.equal(dt, torch.zeros_like(dt)), "S = 0 with beta 0 must zero the table"


@pytest.mark.parametrize("S", [1, 7, 65])
def test_causal_mask_is_bit_exact(cuda, S):
    from dynamic_asr_eval_amd._lib import check, load
    s = torch.randn(3, S, S, generator=K.gen(9300 + S))
    sd = s.to(cuda)
    check(load().dyn_causal_mask(sd.data_ptr(), 3, S, _stream()), "dyn_causal_mask")
    assert _bits_equal(sd, K.causal_mask_ref(s))


# Measured on the MI355X, kernel | torch fp32:   loss (rel)           grad                 weighted loss (rel)  weighted grad
#   C = 5                                      2.9e-08 | 2.9e-08    9.5e-09 | 9.5e-09    5.4e-08 | 5.4e-08    1.1e-07 | 1.1e-07
#   C = 4096                                   1.5e-08 | 1.3e-07    6.2e-09 | 6.2e-09    1.3e-08 | 1.3e-08    1.3e-07 | 1.3e-07
@pytest.mark.parametrize("C", [5, 4096])
def test_nll_loss_and_its_weighted_form(cuda, C):
    from dynamic_asr_eval_amd._lib import check, load
    L = load()
    rows, ignore, scale = 9, -100, 0.25
    logp = F.log_softmax(torch.randn(rows, C, generator=K.gen(9400 + C), dtype=torch.float64) * 2, -1).float()
    tgt = torch.tensor([0, C - 1, ignore, 2, 2, ignore, 1, C + 3, 0], dtype=torch.int32)      # ignored rows, one target >= C
    w = torch.tensor([0.5, 0.0, 1.0, -2.0, 1.5, 0.25, 1.0, 1.0, 3.0])                         # a zero and a negative weight
    lpd, td, wd = logp.to(cuda), tgt.to(cuda), w.to(cuda)

    def torch32(weights, ignore_index, sc):
        live = torch.tensor([t != ignore_index and 0 <= t < C for t in tgt.tolist()])
        ww = torch.ones(rows) if weights is None else weights
        rl = torch.zeros(rows)
        rl[live] = -ww[live] * logp[live, tgt.long()[live]]
        g = torch.zeros(rows, C)
        g[live] = ww[live, None] * sc * (logp[live].exp() - F.one_hot(tgt.long()[live], C))
        return rl.sum(), rl, g, [r for r in range(rows) if not live[r]]

    for weights in (None, w):
        ign = ignore if weights is None else None
        sc = scale if weights is None else 1.0
        loss64, rl64, g64 = K.nll_ref(logp, tgt, ign, sc, weights)
        loss32, rl32, g32, dead = torch32(weights, ign, sc)
        name = "nll" if weights is None else "nll_weighted"
        for with_grad in (True, False):
            loss, rl = torch.full((1,), 9.0, device=cuda), torch.full((rows,), 9.0, device=cuda)
            grad = torch.full((rows, C), 9.0, device=cuda)
            gp = grad.data_ptr() if with_grad else None
            if weights is None:
                check(L.dyn_nll_loss(lpd.data_ptr(), td.data_ptr(), loss.data_ptr(), rl.data_ptr(), gp, rows, C, ignore, scale, _stream()), name)
            else:
                check(L.dyn_nll_loss_weighted(lpd.data_ptr(), td.data_ptr(), wd.data_ptr(), loss.data_ptr(), rl.data_ptr(), gp, rows, C, _stream()), name)
            _measured(f"{name} loss (rel)", loss[0], loss32, loss64, 1e-6, rel=True)
            _check(f"{name} row_loss", rl, rl64, 1e-6)                                         # one fp32 product at most: elementwise
            if with_grad:
                _measured(f"{name} grad", grad, g32, g64, 1e-6)
                assert torch.equal(grad[dead], torch.zeros(len(dead), C, device=cuda)), "an ignored / out-of-range row must have a zero gradient row"
                assert rl[7].item() == 0.0, "a target >= C must contribute 0 loss"
            else:
                assert torch.equal(grad, torch.full((rows, C), 9.0, device=cuda)), "grad null: nothing written"
        loss = torch.full((1,), 9.0, device=cuda)
        if weights is None:
            check(L.dyn_nll_loss(lpd.data_ptr(), td.data_ptr(), loss.data_ptr(), rl.data_ptr(), None, 0, C, ignore, scale, _stream()), name)
        else:
            check(L.dyn_nll_loss_weighted(lpd.data_ptr(), td.data_ptr(), wd.data_ptr(), loss.data_ptr(), rl.data_ptr(), None, 0, C, _stream()), name)
        assert loss.item() == 0.0, "rows = 0 must give loss exactly 0"


# ----------------------------------------------------------------------------------------------------------- argmax, stitch
@pytest.mark.parametrize("C", [1, 63, 4096])
def test_argmax_rows_and_stitch_finalize_rows(cuda, C):
    from dynamic_asr_eval_amd import ops
    rows = 11
    g_ = K.gen(9500 + C)
    x = torch.randn(rows, C, generator=g_)
    if C > 1:                                                  # exact ties: the first maximum wins, also across lanes and across the 64-column stride
        x[1, C // 2] = x[1, 5 % C] = x[1].max() + 1.0
        x[2, C - 1] = x[2, 0] = x[2].max() + 1.0
        x[3] = 0.25
        x[4, min(64, C - 1)] = x[4, 0] = x[4].max() + 2.0
    ids, vals = ops.argmax_rows(x.to(cuda))
    want = np.argmax(x.numpy(), axis=-1)                       # numpy documents the first occurrence
    assert ids.cpu().tolist() == want.tolist()
    assert _bits_equal(vals, x.max(-1).values)
    R = 20
    acc, cnt = torch.rand(R, C, generator=g_) + 0.05, torch.randint(1, 4, (R,), generator=g_).float()
    idx = torch.tensor([0, 1, 5, 6, 7, 12, 19, 3])             # coverage with gaps, not monotonic
    out = ops.stitch_finalize_rows(acc.to(cuda), cnt.to(cuda), idx.to(cuda))
    _check("stitch_finalize_rows", out, K.stitch_finalize_rows_ref(acc, cnt, idx), 2e-6)      # "stitch" 2e-6 in test_stitch
