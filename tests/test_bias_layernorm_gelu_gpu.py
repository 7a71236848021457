"""dyn_bias_layernorm_gelu_fwd / _bwd (the layer-norm wav2vec2 extractor's conv bias + LayerNorm(C) + GELU in one pass each way) against
float64 torch on the CPU — F.gelu(F.layer_norm(z + b, ...)) and its autograd — in the conventions of test_kernel_parity_f64_gpu.py:
forward 5e-6 and dz 2e-5 as floors of kernel_refs.measured_tol (4 x torch's own fp32 error + floor), the three column sums
kernel_refs.wgrad_tol(5e-4, rows, 531), and measured_tol for them as well where a row mean of 50 makes the plain bound meaningless.
Every check prints `name: kernel error | torch fp32 error | bound` before it asserts."""
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


def _torch_ref(z, cb, g, b, dact, dtype):
    """(act, mean, rstd, dz, dgamma, dbeta, dconv_bias) from torch's own ops and autograd in `dtype` on the CPU."""
    zr, gr, br = (t.detach().to(dtype).clone().requires_grad_() for t in (z, g, b))
    cbr = None if cb is None else cb.detach().to(dtype).clone().requires_grad_()
    v = zr if cbr is None else zr + cbr
    act = F.gelu(F.layer_norm(v, (z.shape[-1],), gr, br, EPS))
    act.backward(dact.to(dtype))
    vd = v.detach()
    mean = vd.mean(-1)
    rstd = torch.rsqrt(vd.var(-1, unbiased=False) + EPS)
    return act.detach(), mean, rstd, zr.grad, gr.grad, br.grad, (None if cbr is None else cbr.grad)


def _inputs(rows, C, seed, mean=0.3, std=2.0):
    g_ = K.gen(9000 + seed + rows + C)
    z = torch.randn(rows, C, generator=g_) * std + mean
    cb, g, b = (torch.randn(C, generator=g_) for _ in range(3))
    dact = torch.randn(rows, C, generator=g_)
    old = [torch.randn(C, generator=g_) for _ in range(3)]
    return z, cb, g, b, dact, old


def _run_bwd(ops, cuda, z, cb, g, b, mean, rstd, dact, old, wbeta, skip=None):
    """The fused backward onto copies of the non-zero `old` gradients; `skip` in (None, 0, 1, 2): that weight-gradient pointer is null."""
    outs = [None if k == skip else o.to(cuda) for k, o in enumerate(old)]
    dz = ops.bias_layernorm_gelu_bwd(z.to(cuda), None if cb is None else cb.to(cuda), g.to(cuda), b.to(cuda), mean, rstd, dact.to(cuda),
                                     outs[0], outs[1], None if cb is None else outs[2], wgrad_beta=wbeta)
    return dz, outs


# rows: one row; fewer rows than two workgroups' waves; several workgroups plus a tail.  The two widest instances at the row count that idles a wave.
@pytest.mark.parametrize("rows,C", [(r, c) for c in (256, 512) for r in (1, 7, 1031)] + [(7, 768), (7, 1024)], ids=lambda v: str(v))
def test_forward_and_backward_against_float64(cuda, rows, C):
    from dynamic_asr_eval_amd import ops
    z, cb, g, b, dact, old = _inputs(rows, C, 0)
    wtol = K.wgrad_tol(5e-4, rows, 531)
    for bias in (cb, None):
        tag = "bias" if bias is not None else "no bias"
        r64 = _torch_ref(z, bias, g, b, dact, torch.float64)
        r32 = _torch_ref(z, bias, g, b, dact, torch.float32)
        zd = z.to(cuda)
        z_before = zd.clone()
        act, mean, rstd = ops.bias_layernorm_gelu(zd, None if bias is None else bias.to(cuda), g.to(cuda), b.to(cuda), EPS)
        assert _bits_equal(zd, z_before), "z (the raw conv output) must not be modified"
        _measured(f"act ({tag})", act, r32[0], r64[0], 5e-6)
        _check(f"mean ({tag})", mean, r64[1], 5e-6)                       # the floors of test_layernorm_rmsnorm_row_edges
        _check(f"rstd rel ({tag})", rstd, r64[2], 5e-6, rel=True)
        for wbeta in (0.0, 1.0):
            dz, (dg, db, dc) = _run_bwd(ops, cuda, z, bias, g, b, mean, rstd, dact, old, wbeta)
            _measured(f"dz ({tag}, wgrad_beta {wbeta:g})", dz, r32[3], r64[3], 2e-5)
            _check(f"dgamma ({tag}, wgrad_beta {wbeta:g})", dg, r64[4] + wbeta * old[0].double(), wtol)
            _check(f"dbeta ({tag}, wgrad_beta {wbeta:g})", db, r64[5] + wbeta * old[1].double(), wtol)
            if bias is not None:
                _check(f"dconv_bias (wgrad_beta {wbeta:g})", dc, r64[6] + wbeta * old[2].double(), wtol)
            else:
                assert _bits_equal(dc, old[2]), "no conv bias: its gradient buffer was not passed and must be untouched"
    # each weight-gradient pointer null in turn (a frozen parameter): the other two are what the full call gives, bit for bit
    r64 = _torch_ref(z, cb, g, b, dact, torch.float64)
    _, mean, rstd = ops.bias_layernorm_gelu(z.to(cuda), cb.to(cuda), g.to(cuda), b.to(cuda), EPS)
    dz_full, full = _run_bwd(ops, cuda, z, cb, g, b, mean, rstd, dact, old, 1.0)
    for skip in range(3):
        dz, outs = _run_bwd(ops, cuda, z, cb, g, b, mean, rstd, dact, old, 1.0, skip=skip)
        assert _bits_equal(dz, dz_full)
        for k in range(3):
            if k != skip:
                _check(f"wgrad {k} with pointer {skip} null", outs[k], r64[4 + k] + old[k].double(), wtol)
                assert _bits_equal(outs[k], full[k]), (skip, k)
    # in place: dz over dact
    dd = dact.to(cuda)
    out = ops.bias_layernorm_gelu_bwd(z.to(cuda), cb.to(cuda), g.to(cuda), b.to(cuda), mean, rstd, dd, None, None, None, out=dd)
    assert out.data_ptr() == dd.data_ptr() and _bits_equal(dd, dz_full)


def test_row_mean_of_fifty(cuda):
    """Row mean 50, unit variance: x - mean alone carries ulp(50) / 2 = 1.9e-6, amplified by |gamma| and summed over the rows, so every
    bound is measured (4 x torch's fp32 error + the floor) — the file's rule for inputs that make the plain bounds meaningless."""
    from dynamic_asr_eval_amd import ops
    rows, C = 531, 512
    z, cb, g, b, dact, old = _inputs(rows, C, 1, mean=50.0, std=1.0)
    r64 = _torch_ref(z, cb, g, b, dact, torch.float64)
    r32 = _torch_ref(z, cb, g, b, dact, torch.float32)
    act, mean, rstd = ops.bias_layernorm_gelu(z.to(cuda), cb.to(cuda), g.to(cuda), b.to(cuda), EPS)
    _measured("act", act, r32[0], r64[0], 5e-6)
    _measured("mean", mean, r32[1], r64[1], 5e-6)
    _measured("rstd (rel)", rstd, r32[2], r64[2], 5e-6, rel=True)
    wtol = K.wgrad_tol(5e-4, rows, 531)
    dz, (dg, db, dc) = _run_bwd(ops, cuda, z, cb, g, b, mean, rstd, dact, old, 0.0)
    _measured("dz", dz, r32[3], r64[3], 2e-5)
    _measured("dgamma", dg, r32[4], r64[4], wtol)
    _measured("dbeta", db, r32[5], r64[5], wtol)
    _measured("dconv_bias", dc, r32[6], r64[6], wtol)


def test_bad_width_is_an_argument_error(cuda):
    """C = 100 is refused on the host with DYN_E_ARG (-1) by both entries, before any launch; outputs stay untouched."""
    from dynamic_asr_eval_amd import _lib, ops
    lib = _lib.load()
    rows, C = 3, 100
    z = torch.randn(rows, 128, device=cuda)[:, :C].contiguous()
    g, b, cb = (torch.randn(128, device=cuda)[:C] for _ in range(3))
    act = torch.full((rows, C), 7.0, device=cuda)
    mean, rstd = torch.zeros(rows, device=cuda), torch.zeros(rows, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.dyn_bias_layernorm_gelu_fwd(z.data_ptr(), cb.data_ptr(), g.data_ptr(), b.data_ptr(), act.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), rows, C, EPS, st)
    assert rc == -1 and b"256" in lib.dyn_last_error()
    ws = ops.workspace(cuda)
    dz = torch.full((rows, C), 7.0, device=cuda)
    rc = lib.dyn_bias_layernorm_gelu_bwd(z.data_ptr(), cb.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         act.data_ptr(), dz.data_ptr(), 0, 0, 0, 1.0, rows, C, ws.data_ptr(), ws.numel(), st)
    assert rc == -1
    torch.cuda.synchronize()
    assert (act == 7.0).all() and (dz == 7.0).all()
    with pytest.raises(ops.DynError):
        ops.bias_layernorm_gelu(z, cb.contiguous(), g.contiguous(), b.contiguous(), EPS)


def test_reproducible_and_identical_under_reduce_defer(cuda):
    """Two identical calls give bit-identical outputs (fixed-order column sums, no atomics), and the result with the reductions recorded
    under ops.reduce_defer (as the model's backward runs them) is bit-identical to the direct call."""
    from dynamic_asr_eval_amd import ops
    rows, C = 1031, 512
    z, cb, g, b, dact, old = _inputs(rows, C, 2)
    zd, cbd, gd, bd, dd = (t.to(cuda) for t in (z, cb, g, b, dact))
    a1, m1, s1 = ops.bias_layernorm_gelu(zd, cbd, gd, bd, EPS)
    a2, m2, s2 = ops.bias_layernorm_gelu(zd, cbd, gd, bd, EPS)
    assert _bits_equal(a1, a2) and _bits_equal(m1, m2) and _bits_equal(s1, s2)

    def bwd(arena):
        outs = [o.to(cuda) for o in old]
        with ops.reduce_defer(arena):
            dz = ops.bias_layernorm_gelu_bwd(zd, cbd, gd, bd, m1, s1, dd, *outs, wgrad_beta=1.0)
        return [dz] + outs

    first, second = bwd(None), bwd(None)
    arena = torch.empty(8 << 20, dtype=torch.uint8, device=cuda)
    assert arena.data_ptr() % 256 == 0
    deferred = bwd(arena)
    for k, name in enumerate(("dz", "dgamma", "dbeta", "dconv_bias")):
        assert _bits_equal(first[k], second[k]), f"{name}: two identical calls differ"
        assert _bits_equal(first[k], deferred[k]), f"{name}: differs under ops.reduce_defer"
    assert not _bits_equal(deferred[1], old[0])            # the recorded reductions did run at the flush
