"""The kernels Wav2Vec2-BERT adds, each alone against float64 torch on the CPU: the fused causal conv-module core and its depthwise dgrad /
wgrad (csrc/convmod_causal.hip), the narrow-row LayerNorm (csrc/featproj_ln.hip), the shared distance embedding's gradient
(ops.relkey_embed_grad) and the filter-bank front end (frontend.KaldiFbank, csrc/fbank.hip).

No tolerance here is a chosen number.  Every bound is tests/kernel_refs.measured_tol: 4 x the error the SAME chain written in fp32 torch on
the CPU has against float64 on the same inputs (another, equally valid fp32 summation order), plus a floor of 4 ulp of the output's
largest magnitude.  The measured figures (MI355X) stand next to each assertion and in DESIGN.md."""
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
import wav2vec2_bert_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
KW = 31


def _check(name, got, f32, f64, rel=False):
    """got within 4 x (torch fp32's error) + 4 ulp of the reference's scale."""
    floor = 4 * ULP * (1.0 if rel else max(1e-30, f64.abs().max().item()))
    tol, e32 = K.measured_tol(f32, f64, floor, rel)
    err = K.max_err(got, f64, rel)
    print(f"  {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, (name, err, tol)
    return err


def _core(u, w, gamma, beta, act, eps):
    """transformers' Wav2Vec2BertConvolutionModule between its pointwise convolutions, at u's dtype: (s, g, c, n, mean, rstd)."""
    C = w.shape[0]
    g = F.glu(u, dim=-1)
    c = F.conv1d(F.pad(g.transpose(1, 2), (KW - 1, 0)), w.unsqueeze(1), groups=C).transpose(1, 2)
    mean = c.mean(-1)
    rstd = 1.0 / torch.sqrt(c.var(-1, unbiased=False) + eps)
    n = F.layer_norm(c, (C,), gamma, beta, eps)
    s = F.silu(n) if act == "swish" else F.gelu(n)
    return s, g, c, n, mean.reshape(-1), rstd.reshape(-1)


@pytest.mark.parametrize("act", ["swish", "gelu"])
@pytest.mark.parametrize("shape", [(2, 18, 256), (2, 93, 1024), (1, 131, 512), (3, 1, 768)], ids=["T18-C256", "T93-C1024", "T131-C512", "T1-C768"])
def test_causal_conv_core_dgrad_wgrad_against_float64(cuda, shape, act):
    """T = 18: every frame inside the 30-frame left halo (zeros left of frame 0 in every window); 93 and 131: ragged last tiles at both
    time tiles, interior frames, more than one workgroup; T = 1.  Both time tiles and the default give the same bits (a frame's sum has one
    order).  Measured, worst case (kernel | torch fp32 | bound): s 2.3e-6 | 3.0e-6 | 1.6e-5, conv output 9.3e-7 | 9.3e-7 | 5.1e-6, rstd 1.1e-7 |
    1.3e-7 | 9.9e-7 (relative), dgrad 1.2e-6 | 1.1e-6 | 7.0e-6, wgrad 7.1e-6 | 5.6e-6 | 3.6e-5."""
    from dynamic_asr_eval_amd import ops
    B, T, C = shape
    gen = torch.Generator().manual_seed(B * 1000 + T)
    u = torch.randn(B, T, 2 * C, generator=gen)
    w = torch.randn(C, KW, generator=gen) / KW ** 0.5
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    eps = 1e-5
    r64 = _core(u.double(), w.double(), gamma.double(), beta.double(), act, eps)
    r32 = _core(u, w, gamma, beta, act, eps)
    ud, wd, gd, bd = (t.to(cuda) for t in (u, w, gamma, beta))
    got = ops.convmod_causal(ud, wd, gd, bd, act, eps, save=True)
    for name, a, b32, b64 in zip(("s", "glu", "conv", "norm", "mean"), got, r32, r64):
        _check(name, a.cpu().reshape(b64.shape), b32, b64)
    _check("rstd", got[5].cpu(), r32[5], r64[5], rel=True)
    free = ops.convmod_causal(ud, wd, gd, bd, act, eps, save=False)                # the grad-free call: null optional outputs
    assert all(t is None for t in free[1:]) and torch.equal(free[0], got[0])
    for tt in (8, 16):
        other = ops.convmod_causal(ud, wd, gd, bd, act, eps, save=True, time_tile=tt)
        for a, b in zip(other, got):
            assert torch.equal(a, b), tt
    # the depthwise convolution's two gradients
    dy = torch.randn(B, T, C, generator=gen)
    x = r64[1].float()                                                             # a GLU output as the convolution's input

    def grads(dt):
        xi, wi = x.to(dt).requires_grad_(), w.to(dt).requires_grad_()
        c = F.conv1d(F.pad(xi.transpose(1, 2), (KW - 1, 0)), wi.unsqueeze(1), groups=C).transpose(1, 2)
        c.backward(dy.to(dt))
        return xi.grad, wi.grad

    (dx64, dw64), (dx32, dw32) = grads(torch.float64), grads(torch.float32)
    xd, dyd = x.to(cuda), dy.to(cuda)
    _check("dgrad", ops.dwconv1d_causal_dgrad(dyd, wd).cpu(), dx32, dx64)
    old = torch.randn(B, T, C, generator=gen)
    acc = old.to(cuda)
    assert ops.dwconv1d_causal_dgrad(dyd, wd, out=acc, beta=0.5) is acc
    _check("dgrad beta=0.5", acc.cpu(), dx32 + 0.5 * old, dx64 + 0.5 * old.double())
    for b_ in (0.0, 1.0):                                                           # beta = 1 onto a non-zero buffer
        oldw = torch.randn(C, KW, generator=gen)
        dw = oldw.to(cuda)
        ops.dwconv1d_causal_wgrad(xd, dyd, dw, beta=b_)
        _check(f"wgrad beta={b_:g}", dw.cpu(), dw32 + b_ * oldw, dw64 + b_ * oldw.double())
    twice = torch.zeros(C, KW, device=cuda)
    ops.dwconv1d_causal_wgrad(xd, dyd, twice, beta=0.0)
    again = torch.full((C, KW), float("nan"), device=cuda)
    ops.dwconv1d_causal_wgrad(xd, dyd, again, beta=0.0)
    assert torch.equal(twice, again)                                               # fixed-order combine


@pytest.mark.parametrize("rows,C,offset", [(1, 160, 0.0), (5, 160, 0.0), (300, 160, 0.0), (300, 160, 1000.0), (1, 4, 0.0), (5, 4, 0.0), (300, 4, 0.0),
                                           (1, 256, 0.0), (5, 256, 0.0), (300, 256, 0.0), (5, 256, 1000.0)])
def test_narrow_layernorm_against_float64(cuda, rows, C, offset):
    """rows {1, 5, 300} x C {160, 4, 256}, and two offset cases.  160 is the case that matters (40 of 64 lanes own a float4), 4 and 256 the ends of the range; 300 rows are more than one workgroup's
    (75 partial rows).  offset = 1000 with unit spread is the cancellation case: the statistics are centred, so the kernel stays at torch's
    fp32 error.  Measured (kernel | torch fp32 | bound): y 6.6e-7 | 6.7e-7 | 5.0e-6, at 300 x 160 with the offset 1.5e-4 | 1.3e-4 | 5.1e-4;
    dgamma 8.5e-6 | 7.9e-6 | 6.1e-5, with the offset 2.4e-3 | 2.4e-3 | 9.7e-3 and, the tightest case, 2.4e-4 | 9.1e-5 | 3.7e-4 at 5 x 256
    (xhat carries the fp32 rounding of a mean of 1000 whatever the kernel does); dx 3.3e-6 | 3.4e-6 | 1.9e-5."""
    from dynamic_asr_eval_amd import ops
    gen = torch.Generator().manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, generator=gen) + offset
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    dy = torch.randn(rows, C, generator=gen)
    eps = 1e-5

    def ref(dt):
        xi, g, b = x.to(dt).requires_grad_(), gamma.to(dt).requires_grad_(), beta.to(dt).requires_grad_()
        y = F.layer_norm(xi, (C,), g, b, eps)
        y.backward(dy.to(dt))
        mean = xi.detach().mean(-1)
        rstd = 1.0 / torch.sqrt(xi.detach().var(-1, unbiased=False) + eps)
        return y.detach(), mean, rstd, g.grad, b.grad, xi.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    xd, gd, bd, dyd = (t.to(cuda) for t in (x, gamma, beta, dy))
    y, mean, rstd = ops.narrow_layernorm(xd, gd, bd, eps)
    _check("y", y.cpu(), r32[0], r64[0])
    _check("mean", mean.cpu(), r32[1], r64[1])
    _check("rstd", rstd.cpu(), r32[2], r64[2], rel=True)
    # the backward from the float64 statistics rounded to fp32 (what the forward hands over, to half an ulp)
    dg, db = torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    dx = torch.full((rows, C), float("nan"), device=cuda)
    assert ops.narrow_layernorm_bwd(xd, gd, mean, rstd, dyd, dg, db, dx=dx, wgrad_beta=0.0) is dx
    _check("dgamma", dg.cpu(), r32[3], r64[3])
    _check("dbeta", db.cpu(), r32[4], r64[4])
    _check("dx", dx.cpu(), r32[5], r64[5])
    old_g, old_b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    dg2, db2 = old_g.to(cuda), old_b.to(cuda)
    assert ops.narrow_layernorm_bwd(xd, gd, mean, rstd, dyd, dg2, db2) is None      # dx is optional: the input is data
    assert torch.equal(dg2, dg + old_g.to(cuda)) and torch.equal(db2, db + old_b.to(cuda))   # same partial rows, beta = 1
    only = torch.zeros(C, device=cuda)
    ops.narrow_layernorm_bwd(xd, gd, mean, rstd, dyd, None, only, wgrad_beta=0.0)    # either gradient alone
    assert torch.equal(only, db)


@pytest.mark.parametrize("B,nh,T,P,D", [(2, 4, 93, 73, 64), (1, 3, 19, 9, 64)], ids=["8x93x73x64", "3x19x9x64"])
def test_distance_embedding_gradient_against_float64(cuda, B, nh, T, P, D):
    """dE[p] = beta dE[p] + scale sum_{b, h, i} dC2P[b, h, i, P - 1 - p] q[b, h, i]: two calls give equal bits, beta accumulates.
    Measured (kernel | torch fp32 | bound): 2.9e-6 | 4.9e-6 | 2.6e-5 at 8 x 93, 4.8e-7 | 6.8e-7 | 5.1e-6 at 3 x 19."""
    from dynamic_asr_eval_amd import _attn, ops
    H, ldp, scale = nh * D, (P + 3) // 4 * 4, D ** -0.5
    gen = torch.Generator().manual_seed(T)
    dc = torch.zeros(B, nh, T, ldp)
    dc[..., :P] = torch.randn(B, nh, T, P, generator=gen)
    qkv = torch.randn(B, T, 3 * H, generator=gen)
    old = torch.randn(P, D, generator=gen)

    def ref(dt, beta):
        q = qkv[..., :H].to(dt).view(B, T, nh, D)
        return scale * torch.einsum("bhip,bihd->pd", dc[..., :P].to(dt).flip(-1), q) + beta * old.to(dt)

    dcd, qd = dc.to(cuda), _attn.packed(qkv.to(cuda), 0, D)
    for beta in (0.0, 1.0):
        first, second = old.to(cuda), old.to(cuda)
        assert ops.relkey_embed_grad(dcd, qd, first, scale, beta=beta) is first
        ops.relkey_embed_grad(dcd, qd, second, scale, beta=beta)
        assert torch.equal(first, second)
        _check(f"dE beta={beta:g}", first.cpu(), ref(torch.float32, beta), ref(torch.float64, beta))


_FRONT = {}


def _front(cuda):
    if not _FRONT:
        from dynamic_asr_eval_amd.frontend import KaldiFbank, kaldi_fbank_matrices
        _FRONT["fe"], _FRONT["mats"] = KaldiFbank(cuda), kaldi_fbank_matrices()
    return _FRONT["fe"], _FRONT["mats"]


@pytest.mark.parametrize("L,offset", [(560, 0.0), (1040, 0.0), (48000, 0.0), (48000, 0.5)], ids=["L560", "odd-F", "3s", "3s-plus-0.5"])
def test_front_end_against_the_extractor(cuda, L, offset):
    """frontend.KaldiFbank against SeamlessM4TFeatureExtractor.  Its float32 output is first tied to the formula restated in float64
    (every element within wav2vec2_bert_refs.extractor_bound, worked out from the extractor's float32 roundings; measured 0.06 .. 0.29 of
    it); the device features are held to that formula at 4 x the fp32 CPU chain's error, and to the extractor's own output at the sum of
    the two bounds.  The constant 0.5 is 16 384 after the 2^15 scale: the mean removal sits INSIDE the fp32 basis product.
    Measured (kernel | torch fp32 chain | extractor vs its formula): L560 1.6e-5 | 1.25e-4 | 1.6e-5, odd-F 1.1e-5 | 1.5e-5 | 2.2e-5,
    3 s 1.3e-5 | 1.25e-5 | 8.6e-6, 3 s + 0.5 1.65e-5 | 2.1e-5 | 8.7e-6: the offset costs no more than the fp32 chain's own error, the
    folded basis stays."""
    fe, (basis, fb) = _front(cuda)
    x = torch.randn(L, generator=torch.Generator().manual_seed(L)) + offset
    exact = torch.from_numpy(R.fbank_formula_f64(x))
    chain32 = R.fbank_chain(x, basis.float(), fb.float(), torch.float32)
    got = fe(x.view(1, L).to(cuda))
    Fr = 1 + (L - 400) // 160
    assert got.shape == (1, Fr // 2, 160)
    err = _check("features", got[0].cpu(), chain32, exact)
    want, valid = R.extractor_rows(x)
    assert valid == Fr // 2
    bound = R.extractor_bound(x)
    own = np.abs(want[:valid].astype(np.float64) - exact.numpy())
    against = np.abs(got[0].cpu().double().numpy() - want[:valid])
    tol, _ = K.measured_tol(chain32, exact, 4 * ULP * exact.abs().max().item())
    print(f"  extractor vs its formula {own.max():.2e} = {(own / bound).max():.2f} of its bound | kernel vs extractor {against.max():.2e}")
    assert (own <= bound).all(), (own / bound).max()                               # the restated formula IS the extractor's, to float32 rounding
    assert (against <= tol + bound).all(), (against.max(), tol, bound.max())


def test_front_end_in_a_padded_bucket(cuda):
    """Two waveforms (the second a gain-and-offset copy) zero-padded to a longer bucket with the valid frame count in a device scalar: the
    valid rows are the unpadded call's, the rows past them exact zeros, and a shorter utterance after a longer one leaves nothing behind."""
    fe, (basis, fb) = _front(cuda)
    Lb = 400 + 160 * 41 - 1                                                        # 41 frames -> 20 rows
    valid = torch.zeros(1, dtype=torch.int32, device=cuda)
    buf = torch.zeros(2, Lb, device=cuda)
    for L in (5000, 3021, 560):
        x = torch.randn(L, generator=torch.Generator().manual_seed(L))
        x2 = torch.stack([x, 0.3 * x + 0.01]).to(cuda)
        Fr = 1 + (L - 400) // 160
        T = Fr // 2
        alone = fe(x2)
        buf.zero_()
        buf[:, :L].copy_(x2)
        valid.fill_(Fr)
        got = fe(buf, valid=valid)
        assert got.shape == (2, 20, 160) and alone.shape == (2, T, 160)
        assert got[:, T:].abs().max().item() == 0.0 if T < 20 else True
        exact = torch.from_numpy(R.fbank_formula_f64(x))
        chain32 = R.fbank_chain(x, basis.float(), fb.float(), torch.float32)
        _check(f"L={L} padded", got[0, :T].cpu(), chain32, exact)
        _check(f"L={L} alone", alone[0].cpu(), chain32, exact)
        diff = (got[:, :T] - alone).abs().max().item()
        print(f"  L={L}: padded vs unpadded call {diff:.2e}")
        assert torch.equal(got[:, :T], alone), diff
        gain = (got[1, :T] - got[0, :T]).abs().max().item()                         # gain-invariant except through the mel floor
        print(f"  L={L}: 0.3 x + 0.01 against x {gain:.2e}")
    with pytest.raises(Exception) as e:
        fe(torch.zeros(1, 559, device=cuda))
    assert "559 samples" in str(e.value)
