"""The kernels NemotronAsrStreamingForRNNT adds (csrc/relshift_band.hip, subsample_causal.hip, the _k9 entries of convmod_causal.hip) against the float64
torch restatements of tests/nemotron_refs.py on the same inputs.  The bar is test_rnnt_kernels_gpu.py's, constants and code: at most
4 x the error of the float32 torch restatement against the same float64 result + 2e-6."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import nemotron_refs as NR  # noqa: E402
from test_rnnt_kernels_gpu import FLOOR, _check  # noqa: E402

pytestmark = pytest.mark.gpu

M = 4                                                        # B * nh of every band-softmax case
BAND_CASES = ([(T, 70, 13) for T in (1, 5, 34, 257, 600)] + [(T, 70, 0) for T in (1, 5, 34, 257, 600)]
              + [(34, 8, 3), (34, -1, 2), (34, 70, 299), (600, 70, 299)])


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("T,left,look", BAND_CASES)
def test_band_softmax_forward_and_backward(cuda, T, left, look):
    """ops.softmax_relshift_band and ops.relshift_band_bwd (with the existing ops.softmax_bwd between them) at B nh = 4 against
    nemotron_refs.band_softmax and its autograd in float64.  The band buffer holds the W columns r0 .. r0 + W of a random FULL
    [M, T, 2T - 1] position product; the reference reads the full one through transformers' shift.  Outside every row's key range
    the output is exactly zero, and so is every column of the band gradient buffer that no key of its row reaches (the buffer starts as
    NaN: every column is written); the reference's gradient is exactly zero in every table row outside the band.  In place (out = S)
    gives the same bits.  The released pair (70, 13), cs = 1, lc cs != left context, an unlimited left context, one chunk (the band is
    the table), and T' = 1, 5, 257 (a stride-loop edge of the 256-thread rows), 600 (more than 256 items: two per thread).
    Measured (MI355X), the case with the kernel's largest error, kernel | float32 restatement | bound: y 2.7e-07 | 2.5e-07 | 3.0e-06,
    dS 9.8e-07 | 7.5e-07 | 5.0e-06, dBD 9.8e-07 | 7.5e-07 | 5.0e-06."""
    from dynamic_asr_eval_amd import ops
    band = ops.chunked_band(T, left, look)
    mask = NR.chunked_mask(T, left, look)
    S, BD, dY = (torch.randn(M, T, n, generator=_g(7 + T + look)) * s for n, s in ((T, 2.0), (2 * T - 1, 2.0), (T, 1.0)))
    y64, dS64, dBD64 = NR.band_softmax_grads(S, BD, mask, dY, torch.float64)
    y32, dS32, dBD32 = NR.band_softmax_grads(S, BD, mask, dY, torch.float32)
    rows = slice(band.r0, band.r0 + band.W)
    outside = torch.ones(2 * T - 1, dtype=torch.bool)
    outside[rows] = False
    assert dBD64[:, :, outside].abs().sum().item() == 0.0    # the table's gradient has only its band rows
    Sd = S.view(1, M, T, T).to(cuda)
    BDb = BD[:, :, rows].contiguous().view(1, M, T, band.W).to(cuda)
    y = ops.softmax_relshift_band(Sd, BDb, band)
    assert (y.cpu()[0][~mask.expand(M, T, T)] == 0).all()
    _check("y", y.cpu()[0], y32, y64)
    dS = ops.softmax_bwd(y, dY.view(1, M, T, T).to(cuda))
    _check("dS", dS.cpu()[0], dS32, dS64)
    buf = torch.full((1, M, T, band.W), float("nan"), device=cuda)
    dBDb = ops.relshift_band_bwd(dS, band, out=buf).cpu()[0]
    _check("dBD", dBDb, dBD32[:, :, rows], dBD64[:, :, rows])
    i, c = torch.arange(T)[:, None], torch.arange(band.W)[None, :]
    j = c - band.dlo + i                                       # the key a band column belongs to in row i
    unused = ~((j >= 0) & (j < T) & mask[i, j.clamp(0, T - 1)])
    assert (dBDb[unused.expand(M, T, band.W)] == 0).all()
    inplace = Sd.clone()
    ops.softmax_relshift_band(inplace, BDb, band, out=inplace)
    assert torch.equal(inplace, y)


def test_band_arguments_are_refused_before_any_launch(cuda):
    from dynamic_asr_eval_amd import ops
    S = torch.zeros(1, 2, 5, 5, device=cuda)
    band = ops.chunked_band(5, 3, 1)
    with pytest.raises(ops.DynError):
        ops.softmax_relshift_band(S, torch.zeros(1, 2, 5, band.W - 1, device=cuda), band)
    with pytest.raises(ops.DynError):
        ops.relshift_band_bwd(S, band, ld_bd=band.W - 1)
    with pytest.raises(ops.DynError):
        ops.chunked_band(5, 3, -1)


@pytest.mark.parametrize("T,F,C", [(1, 80, 4), (2, 80, 32), (7, 41, 32), (131, 80, 32), (16, 128, 256)])
def test_causal_subsampling_stages(cuda, T, F, C):
    """The causal stem (forward, weight gradient) and the causal depthwise stage with ReLU fused into its loads (forward, data and
    weight gradient) at B = 2 against F.pad (2, 1) + F.conv2d in float64; odd and even widths, T = 1, C = 4 and C = 256 (the released
    channels).  Gradients accumulate: a second call with beta = 1 doubles them.
    Measured (MI355X), the case with the kernel's largest error, kernel | float32 restatement | bound: stem 1.2e-06 | 6.9e-07 | 4.7e-06,
    stem dw 3.4e-05 | 1.2e-04 | 4.9e-04, stem db 2.6e-05 | 8.9e-05 | 3.6e-04, depthwise 5.2e-06 | 4.4e-06 | 2.0e-05, dz 4.0e-07 | 4.0e-07 |
    3.6e-06, depthwise dw 2.4e-05 | 4.0e-05 | 1.6e-04, depthwise db 2.6e-05 | 6.6e-05 | 2.7e-04."""
    from dynamic_asr_eval_amd import ops
    B = 2
    To, Fo = T // 2 + 1, F // 2 + 1
    g = _g(11 + T + F + C)
    x, z = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, C, generator=g)
    w, bias = torch.randn(C, 3, 3, generator=g) / 3, torch.randn(C, generator=g)
    dout = torch.randn(B, To, Fo, C, generator=g)
    d = lambda t: t.to(cuda)                                                                                  # noqa: E731
    # stem
    (y64, g64), (y32, g32) = (NR.grads(NR.stem, (x, w, bias), dout, dt) for dt in (torch.float64, torch.float32))
    y = ops.conv2d_first_causal(d(x), d(w), d(bias))
    assert y.shape == (B, To, Fo, C)
    _check("stem", y.cpu(), y32, y64)
    dw, db = torch.zeros(C, 3, 3, device=cuda), torch.zeros(C, device=cuda)
    ops.conv2d_first_causal_wgrad(d(x), d(dout), dw, db, beta=0.0)
    _check("stem dw", dw.cpu(), g32[1], g64[1]); _check("stem db", db.cpu(), g32[2], g64[2])
    once = dw.clone()
    ops.conv2d_first_causal_wgrad(d(x), d(dout), dw, db, beta=1.0)
    assert torch.allclose(dw, 2 * once, rtol=1e-6, atol=0)
    # depthwise stage
    (y64, g64), (y32, g32) = (NR.grads(NR.dw_stage, (z, w, bias), dout, dt) for dt in (torch.float64, torch.float32))
    u = ops.dwconv2d_s2_causal_act(d(z), d(w), d(bias), "relu")
    assert u.shape == (B, To, Fo, C)
    _check("dw", u.cpu(), y32, y64)
    dz = ops.dwconv2d_s2_causal_dgrad_act(d(z), d(w), d(dout), "relu")
    _check("dw dz", dz.cpu(), g32[0], g64[0])
    dw, db = torch.zeros(C, 3, 3, device=cuda), torch.zeros(C, device=cuda)
    ops.dwconv2d_s2_causal_wgrad_act(d(z), d(dout), dw, db, "relu", beta=0.0)
    _check("dw dw", dw.cpu(), g32[1], g64[1]); _check("dw db", db.cpu(), g32[2], g64[2])
    with pytest.raises(ops.DynError):
        ops.dwconv2d_s2_causal_act(d(z), d(w), d(bias), "silu")


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("B,T,C", [(1, 1, 256), (2, 5, 256), (2, 9, 1024), (3, 34, 512), (1, 17, 768)])
def test_conv_module_core_at_9_taps(cuda, B, T, C, has_bias):
    """ops.convmod_causal_k9 (one launch) and its backward chain (ops.silu_bwd, layernorm_bwd, dwconv1d_causal_k9_wgrad / _dgrad, colsum,
    glu_bwd: what the model runs) against nemotron_refs.convmod_core and its autograd in float64, with and without the depthwise bias;
    T' below the tap count (1, 5), off the 8-frame tile (9, 17, 34), every built width.
    Measured (MI355X), the case with the kernel's largest error, kernel | float32 restatement | bound: s 1.1e-06 | 1.2e-06 | 6.9e-06,
    du 1.7e-06 | 1.2e-06 | 6.7e-06, dgamma 5.8e-06 | 6.6e-06 | 2.9e-05, dbeta 4.2e-06 | 2.6e-06 | 1.2e-05, dcbias 4.5e-06 | 3.3e-06 | 1.5e-05;
    the depthwise taps' gradient stays under its bound in every case."""
    from dynamic_asr_eval_amd import ops
    g = _g(3 + B + T + C)
    u = torch.randn(B, T, 2 * C, generator=g)
    w = torch.randn(C, 9, generator=g) / 3
    cb = torch.randn(C, generator=g) if has_bias else None
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dout = torch.randn(B, T, C, generator=g)
    ins = (u, w, cb, gamma, beta) if has_bias else (u, w, gamma, beta)
    fn = NR.convmod_core if has_bias else (lambda u_, w_, ga, be: NR.convmod_core(u_, w_, None, ga, be))
    (y64, g64), (y32, g32) = (NR.grads(fn, ins, dout, dt) for dt in (torch.float64, torch.float32))
    d = lambda t: None if t is None else t.to(cuda)                                                           # noqa: E731
    s, gl, cv, nn, mean, rstd = ops.convmod_causal_k9(d(u), d(w), d(cb), d(gamma), d(beta), save=True)
    _check("s", s.cpu(), y32, y64)
    s2 = ops.convmod_causal_k9(d(u), d(w), d(cb), d(gamma), d(beta))[0]
    assert torch.equal(s2, s)
    dnn = ops.silu_bwd(nn, d(dout))
    dcv, dgam, dbet = torch.empty_like(dnn), torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    ops.layernorm_bwd(cv, d(gamma), mean, rstd, dnn, dcv, dgam, dbet, dx_beta=0.0)
    dw = torch.zeros(C, 9, device=cuda)
    ops.dwconv1d_causal_k9_wgrad(gl, dcv, dw, beta=0.0)
    du = ops.glu_bwd(d(u), ops.dwconv1d_causal_k9_dgrad(dcv, d(w)))
    k = 1 if has_bias else 0
    _check("du", du.cpu(), g32[0], g64[0]); _check("dw", dw.cpu(), g32[1], g64[1])
    _check("dgamma", dgam.cpu(), g32[2 + k], g64[2 + k]); _check("dbeta", dbet.cpu(), g32[3 + k], g64[3 + k])
    if has_bias:
        dcb = torch.zeros(C, device=cuda)
        ops.colsum(dcv.view(-1, C), dcb, beta=0.0)
        _check("dcbias", dcb.cpu(), g32[2], g64[2])
    with pytest.raises(ops.DynError):
        ops.convmod_causal_k9(d(u), torch.zeros(C, 31, device=cuda), d(cb), d(gamma), d(beta))


@pytest.mark.parametrize("T,left,look", [(34, 8, 2), (257, 70, 13), (34, -1, 2)])
def test_band_attention_equals_the_dense_path_under_an_additive_mask(cuda, T, left, look):
    """One head group's attention, forward and backward, twice from the same q + u, q + v, k, v and projected position table: the band
    path (the W-row position product, ops.softmax_relshift_band, ops.relshift_band_bwd, K = W and M = W gradient products) and the
    existing dense path (the full [T, 2T - 1] product, ops.softmax_relshift on scores + an additive -inf mask built here,
    ops.relshift_bwd).  The context, d(q + u), dk, dv, d(q + v) and the band rows of the position table's gradient differ by no more than
    4 x the float32 torch restatement's error against float64 + 2e-6; the dense table gradient's rows outside the band are exactly zero.
    Measured (MI355X), worst over the three cases: band against dense 7.2e-07 (d(q + v)), band against float64 1.9e-06 (dpos) | float32
    restatement 1.2e-06 | bound 6.9e-06."""
    from dynamic_asr_eval_amd import _attn, ops
    B, nh, D = 2, 2, 64
    H = nh * D
    scale = D ** -0.5
    band = ops.chunked_band(T, left, look)
    W, R = band.W, 2 * T - 1
    mask = NR.chunked_mask(T, left, look)
    g = _g(5 + T)
    qu, qv, k, v, dO = (torch.randn(B, T, H, generator=g) for _ in range(5))
    pos = torch.randn(R, H, generator=g)

    def torch_ref(dt):
        t = [a.to(dt).clone().requires_grad_() for a in (qu, qv, k, v, pos)]
        hd = lambda a: a.view(B, T, nh, D).permute(0, 2, 1, 3)                                                # noqa: E731
        S = hd(t[0]) @ hd(t[2]).transpose(-1, -2) * scale
        BD = hd(t[1]) @ t[4].view(R, nh, D).permute(1, 2, 0) * scale
        P = NR.band_softmax(S.reshape(B * nh, T, T), BD.reshape(B * nh, T, R), mask).view(B, nh, T, T)
        O = (P @ hd(t[3])).permute(0, 2, 1, 3).reshape(B, T, H)
        (O * dO.to(dt)).sum().backward()
        return [O.detach()] + [a.grad for a in t]

    want, t32 = torch_ref(torch.float64), torch_ref(torch.float32)
    d = lambda a: a.to(cuda)                                                                                  # noqa: E731
    quD, qvD, kD, vD, posD, dOD = (d(a) for a in (qu, qv, k, v, pos, dO))
    add = torch.zeros(T, T).masked_fill(~mask, float("-inf")).to(cuda)

    def run(banded):
        n = W if banded else R
        pw = posD[band.r0:band.r0 + W] if banded else posD
        S = torch.empty(B, nh, T, T, device=cuda)
        _attn.scores(_attn.plain(quD, D), _attn.plain(kD, D), S, scale)
        BD = torch.empty(B, nh, T, n, device=cuda)
        ops.gemm(qvD, pw, BD, trans_b=True, M=T, N=n, K=D, lda=H, ldb=H, ldc=n, nb1=B, nb2=nh, sa=(T * H, D), sb=(0, D), sc=(nh * T * n, T * n),
                 alpha=scale)
        if banded:
            ops.softmax_relshift_band(S, BD, band, out=S)
        else:
            S += add
            ops.softmax_relshift(S, BD, out=S)
        O = torch.empty(B, T, H, device=cuda)
        _attn.context(S, _attn.plain(vD, D), _attn.plain(O, D))
        dv, dk, dqu, dqv = (torch.empty(B, T, H, device=cuda) for _ in range(4))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dOD, D), _attn.plain(vD, D), _attn.plain(dv, D), dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)
        _attn.grad_qk(dP, _attn.plain(quD, D), _attn.plain(kD, D), _attn.plain(dqu, D), _attn.plain(dk, D), scale)
        dBD = ops.relshift_band_bwd(dP, band) if banded else ops.relshift_bwd(dP)
        ops.gemm(dBD, pw, dqv, M=T, N=D, K=n, lda=n, ldb=H, ldc=H, nb1=B, nb2=nh, sa=(nh * T * n, T * n), sb=(0, D), sc=(T * H, D), alpha=scale)
        dpos = torch.empty(n, H, device=cuda)
        for b in range(B):
            ops.gemm(dBD, qvD, dpos, trans_a=True, M=n, N=D, K=T, lda=n, ldb=H, ldc=H, nb1=1, nb2=nh, sa=(0, T * n), sb=(0, D), sc=(0, D),
                     a_off=b * nh * T * n, b_off=b * T * H, alpha=scale, beta=0.0 if b == 0 else 1.0)
        return [t.cpu() for t in (O, dqu, dqv, dk, dv, dpos)]

    bandr, dense = run(True), run(False)
    outside = torch.ones(R, dtype=torch.bool)
    outside[band.r0:band.r0 + W] = False
    assert dense[5][outside].abs().sum().item() == 0.0
    dense[5] = dense[5][band.r0:band.r0 + W]
    want[5], t32[5] = want[5][band.r0:band.r0 + W], t32[5][band.r0:band.r0 + W]
    for name, a, b_, w64, w32 in zip(("O", "dqu", "dqv", "dk", "dv", "dpos"), bandr, dense, want, t32):
        tol, e32 = K.measured_tol(w32, w64, FLOOR)
        err, own = K.max_err(a, b_.double()), K.max_err(a, w64)
        print(f"{name}: band vs dense {err:.2e}, band vs float64 {own:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
        assert err <= tol and own <= tol, name
