"""The 64- and 128-channel instances of dyn_bias_layernorm_gelu_fwd / _bwd (SEW's narrow layer-norm extractor layers: a row on 16 or 32
lanes, 4 or 2 rows per wave) against float64 torch on the CPU — F.gelu(F.layer_norm(z + conv_bias)) and its autograd — in the conventions of
test_bias_layernorm_gelu_gpu.py: forward 5e-6 and dz 2e-5 as floors of kernel_refs.measured_tol (4 x torch's own fp32 error + floor), the
three column sums kernel_refs.wgrad_tol(5e-4, rows, 531).  Every check prints `name: kernel error | torch fp32 error | bound` first."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 1e-5
SHAPES = [(1, 64), (7, 64), (1031, 64), (1, 128), (7, 128), (1031, 128)]       # rows: less than a wave's 4 / 2, a tail, several workgroups + tail


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


def _ref(z, cb, g, b, dact, dtype):
    zr, gr, br = (t.detach().to(dtype).clone().requires_grad_() for t in (z, g, b))
    cr = None if cb is None else cb.detach().to(dtype).clone().requires_grad_()
    v = zr if cr is None else zr + cr
    act = F.gelu(F.layer_norm(v, (z.shape[-1],), gr, br, EPS))
    act.backward(dact.to(dtype))
    vd = v.detach()
    return (act.detach(), vd.mean(-1), torch.rsqrt(vd.var(-1, unbiased=False) + EPS), zr.grad, gr.grad, br.grad, None if cr is None else cr.grad)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rows,C", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_forward_and_backward_against_float64(cuda, rows, C, with_bias):
    from dynamic_asr_eval_amd import ops
    g_ = K.gen(8000 + rows + C)
    z = torch.randn(rows, C, generator=g_) * 2.0 + 0.3
    cb = torch.randn(C, generator=g_) if with_bias else None
    g, b, dact = torch.randn(C, generator=g_), torch.randn(C, generator=g_), torch.randn(rows, C, generator=g_)
    old = torch.randn(3, C, generator=g_)
    r64, r32 = _ref(z, cb, g, b, dact, torch.float64), _ref(z, cb, g, b, dact, torch.float32)
    zd, gd, bd, dd = (t.to(cuda) for t in (z, g, b, dact))
    cd = None if cb is None else cb.to(cuda)
    z_before = zd.clone()
    act, mean, rstd = ops.bias_layernorm_gelu(zd, cd, gd, bd, EPS)
    act2, mean2, rstd2 = ops.bias_layernorm_gelu(zd, cd, gd, bd, EPS)
    assert _bits_equal(act, act2) and _bits_equal(mean, mean2) and _bits_equal(rstd, rstd2) and _bits_equal(zd, z_before)
    _measured("act", act, r32[0], r64[0], 5e-6)
    _check("mean", mean, r64[1], 5e-6)
    _check("rstd rel", rstd, r64[2], 5e-6, rel=True)
    wtol = K.wgrad_tol(5e-4, rows, 531)
    for wbeta in (0.0, 1.0):
        dg, db, dc = (old[k].to(cuda) for k in range(3))
        dz = ops.bias_layernorm_gelu_bwd(zd, cd, gd, bd, mean, rstd, dd, dg, db, dc if with_bias else None, wgrad_beta=wbeta)
        _measured(f"dz (wgrad_beta {wbeta:g})", dz, r32[3], r64[3], 2e-5)
        _check(f"dgamma (wgrad_beta {wbeta:g})", dg, r64[4] + wbeta * old[0].double(), wtol)
        _check(f"dbeta (wgrad_beta {wbeta:g})", db, r64[5] + wbeta * old[1].double(), wtol)
        if with_bias:
            _check(f"dconv_bias (wgrad_beta {wbeta:g})", dc, r64[6] + wbeta * old[2].double(), wtol)
    again = [old[k].to(cuda) for k in range(3)]
    dz2 = ops.bias_layernorm_gelu_bwd(zd, cd, gd, bd, mean, rstd, dd, again[0], again[1], again[2] if with_bias else None, wgrad_beta=1.0)
    assert _bits_equal(dz2, dz) and _bits_equal(again[0], dg) and _bits_equal(again[1], db), "two identical calls must give identical bits"
    frozen = ops.bias_layernorm_gelu_bwd(zd, cd, gd, bd, mean, rstd, dd, None, None, None)
    assert _bits_equal(frozen, dz)
    inplace = dd.clone()
    assert ops.bias_layernorm_gelu_bwd(zd, cd, gd, bd, mean, rstd, inplace, None, None, None, out=inplace) is inplace and _bits_equal(inplace, dz)
    assert _bits_equal(zd, z_before)


def test_identical_under_reduce_defer(cuda):
    from dynamic_asr_eval_amd import ops
    rows, C = 5003, 64
    g_ = K.gen(8100)
    z, cb, g, b, dact = (torch.randn(*s, generator=g_).to(cuda) for s in ((rows, C), (C,), (C,), (C,), (rows, C)))
    old = torch.randn(3, C, generator=g_)
    act, mean, rstd = ops.bias_layernorm_gelu(z, cb, g, b, EPS)

    def bwd(arena):
        w = [old[k].to(cuda) for k in range(3)]
        with ops.reduce_defer(arena):
            dz = ops.bias_layernorm_gelu_bwd(z, cb, g, b, mean, rstd, dact, *w, wgrad_beta=1.0)
        return [dz] + w

    first = bwd(None)
    arena = torch.empty(8 << 20, dtype=torch.uint8, device=cuda)
    deferred = bwd(arena)
    for k, name in enumerate(("dz", "dgamma", "dbeta", "dconv_bias")):
        assert _bits_equal(first[k], deferred[k]), f"{name}: differs under ops.reduce_defer"
    assert not _bits_equal(deferred[3], old[2])
