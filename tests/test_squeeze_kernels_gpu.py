"""dyn_squeeze_ln_fwd / _bwd and dyn_unsqueeze_act_fwd / _bwd (csrc/squeeze.hip: the two ends of SEW's squeezed encoder, one pass each way)
against float64 torch on the CPU — F.avg_pool1d, F.gelu, F.layer_norm, reshape, F.pad and autograd — in the conventions of
test_posconv_ln_gelu_gpu.py: forward 5e-6 and dh / dyg / du 2e-5 as floors of kernel_refs.measured_tol (4 x torch's own fp32 error + floor),
the three column sums kernel_refs.wgrad_tol(5e-4, rows, 531), and measured_tol for them as well where a row mean of 50 makes the plain
bound meaningless.  Every check prints `name: kernel error | torch fp32 error | bound` before it asserts."""
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
SHAPES = [(2, 7, 256, 4, 2), (1, 33, 768, 16, 2), (2, 18, 1024, 16, 3), (1, 5, 256, 16, 4), (2, 6, 512, 16, 1)]       # (B, T, H, G, s)
IDS = ["T7-odd-s2-cg64", "H768-cg48-s2", "H1024-s3", "T5-s4-one-row", "s1-degenerate-pool"]
EXTRA = 3                     # yg rows per group beyond T2 (Tg > T2): NaN, never to be read


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


def _grouped(t, G):            # [B, T, H] -> [B, G, T, cg]
    B, T, H = t.shape
    return t.view(B, T, G, H // G).permute(0, 2, 1, 3).contiguous()


def _vt(valid, cuda):
    return None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)


def _valids(T2):
    return (None, T2, max(T2 - 2, 1), 1)


def _inputs(B, T, H, G, s, seed, mean=0.3, std=2.0, extra=EXTRA):
    """h [B, T, H], the conv product y [B, T2, H] token-major and the same numbers as yg [B, G, T2 + extra, cg] (the extra rows hold NaN)."""
    g_ = K.gen(9000 + seed + B * T + H + G + s)
    T2, cg = T // s, H // G
    h = torch.randn(B, T, H, generator=g_) * std + mean
    y = torch.randn(B, T2, H, generator=g_) * std
    yg = torch.full((B, G, T2 + extra, cg), float("nan"))
    yg[:, :, :T2] = _grouped(y, G)
    bias, gamma, beta = (torch.randn(H, generator=g_) for _ in range(3))
    dz = torch.randn(B, T2, H, generator=g_)
    old = torch.randn(3, H, generator=g_)
    return h, y, yg.contiguous(), bias, gamma, beta, dz, old


def _squeeze_ref(h, y, bias, gamma, beta, dz, s, valid, dtype):
    """(z, mean, rstd, dh, dy, dgamma, dbeta, dbias) from torch's own ops and autograd in `dtype`; rows >= valid of z are zeroed after the
    LayerNorm (so they carry no gradient), their statistics are those of the row all the same."""
    hr, yr, br, gr, tr = (t.detach().to(dtype).clone().requires_grad_() for t in (h, y, bias, gamma, beta))
    T2 = h.shape[1] // s
    pl = F.avg_pool1d(hr.transpose(1, 2), s, s).transpose(1, 2)
    pre = pl[:, :T2] + F.gelu(yr + br)
    z = F.layer_norm(pre, (h.shape[-1],), gr, tr, EPS)
    keep = torch.zeros(T2, dtype=dtype)
    keep[:T2 if valid is None else valid] = 1.0
    z = z * keep[None, :, None]
    z.backward(dz.to(dtype))
    pd = pre.detach()
    return (z.detach(), pd.mean(-1).reshape(-1), torch.rsqrt(pd.var(-1, unbiased=False) + EPS).reshape(-1), hr.grad, yr.grad, gr.grad, tr.grad,
            br.grad)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_squeeze_forward_and_backward_against_float64(cuda, shape):
    """Every shape with valid in {None, T2, max(T2 - 2, 1), 1}; Tg = T2 + 3 with NaN in the rows never to be read.  Rows >= valid of z and dyg,
    rows >= s valid and rows >= s T2 of dh are exact zeros; wgrad_beta 0 / 1 and null gradient pointers; h and yg are left unmodified; two
    identical calls give identical bits."""
    from dynamic_asr_eval_amd import ops
    B, T, H, G, s = shape
    T2 = T // s
    h, y, yg, bias, gamma, beta, dz, old = _inputs(B, T, H, G, s, 0)
    hd, ygd, bd, gd, td, dzd = (t.to(cuda) for t in (h, yg, bias, gamma, beta, dz))
    h_before, yg_before = hd.clone(), ygd.clone()
    wtol = K.wgrad_tol(5e-4, B * T2, 531)
    for valid in _valids(T2):
        tag = f"valid {valid}"
        Tv = T2 if valid is None else valid
        r64 = _squeeze_ref(h, y, bias, gamma, beta, dz, s, valid, torch.float64)
        r32 = _squeeze_ref(h, y, bias, gamma, beta, dz, s, valid, torch.float32)
        z, mean, rstd = ops.squeeze_ln(hd, ygd, bd, gd, td, s, EPS, valid=_vt(valid, cuda))
        z2, mean2, rstd2 = ops.squeeze_ln(hd, ygd, bd, gd, td, s, EPS, valid=_vt(valid, cuda))
        assert z.shape == (B, T2, H) and _bits_equal(z, z2) and _bits_equal(mean, mean2) and _bits_equal(rstd, rstd2)
        assert _bits_equal(ygd, yg_before) and _bits_equal(hd, h_before), "h and yg must not be modified"
        assert torch.isfinite(z).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        if Tv < T2:
            assert z[:, Tv:].abs().max().item() == 0.0
        _measured(f"z ({tag})", z, r32[0], r64[0], 5e-6)
        _check(f"mean ({tag})", mean, r64[1], 5e-6)
        _check(f"rstd rel ({tag})", rstd, r64[2], 5e-6, rel=True)
        for wbeta in (0.0, 1.0):
            dg, db, dc = (old[k].to(cuda) for k in range(3))
            dh, dyg = ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dzd, s, dg, db, dc, wgrad_beta=wbeta, valid=_vt(valid, cuda))
            assert dh.shape == (B, T, H) and dyg.shape == (B, G, T2, H // G)
            assert torch.isfinite(dh).all() and torch.isfinite(dyg).all()
            if s * Tv < T:
                assert dh[:, s * Tv:].abs().max().item() == 0.0
            if Tv < T2:
                assert dyg[:, :, Tv:].abs().max().item() == 0.0
            _measured(f"dh ({tag}, wgrad_beta {wbeta:g})", dh, r32[3], r64[3], 2e-5)
            _measured(f"dyg ({tag}, wgrad_beta {wbeta:g})", dyg, _grouped(r32[4], G), _grouped(r64[4], G), 2e-5)
            for k, (name, got) in enumerate((("dgamma", dg), ("dbeta", db), ("dbias", dc))):
                _check(f"{name} ({tag}, wgrad_beta {wbeta:g})", got, r64[5 + k] + wbeta * old[k].double(), wtol)
        again = ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dzd, s, old[0].to(cuda), old[1].to(cuda), old[2].to(cuda), wgrad_beta=1.0,
                                   valid=_vt(valid, cuda))
        frozen = ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dzd, s, None, None, None, valid=_vt(valid, cuda))
        assert _bits_equal(again[0], dh) and _bits_equal(again[1], dyg), "two identical calls must give identical bits"
        assert _bits_equal(frozen[0], dh) and _bits_equal(frozen[1], dyg), "null gradient pointers: the same dh and dyg"
        only = old[2].to(cuda)                                       # one of the three alone: the same sum as with all three
        ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dzd, s, None, None, only, wgrad_beta=1.0, valid=_vt(valid, cuda))
        assert _bits_equal(only, dc)
        assert _bits_equal(ygd, yg_before) and _bits_equal(hd, h_before)


def _unsqueeze_ref(u, d, T, s, valid, dtype):
    ur = u.detach().to(dtype).clone().requires_grad_()
    B, T2, sH = u.shape
    keep = torch.zeros(T2, dtype=dtype)
    keep[:T2 if valid is None else valid] = 1.0
    a = (F.gelu(ur) * keep[None, :, None]).reshape(B, T2, s, sH // s).reshape(B, s * T2, sH // s)
    out = F.pad(a, (0, 0, 0, T - s * T2))
    out.backward(d.to(dtype))
    return out.detach(), ur.grad


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unsqueeze_forward_and_backward_against_float64(cuda, shape):
    """gelu(u) cut into s frames per squeezed frame, exact zero rows from s min(valid, T2) to T; du = d * gelu'(u) with exact zero rows from
    valid on.  The incoming gradient holds NaN in the rows the backward must not read."""
    from dynamic_asr_eval_amd import ops
    B, T, H, G, s = shape
    T2 = T // s
    g_ = K.gen(9500 + B * T + H + s)
    u = torch.randn(B, T2, s * H, generator=g_) * 2.0
    u.view(-1)[:len(K.GELU_EDGES)] = torch.tensor(K.GELU_EDGES)
    d = torch.randn(B, T, H, generator=g_)
    ud = u.to(cuda)
    u_before = ud.clone()
    for valid in _valids(T2):
        tag = f"valid {valid}"
        Tv = T2 if valid is None else valid
        r64, r32 = _unsqueeze_ref(u, d, T, s, valid, torch.float64), _unsqueeze_ref(u, d, T, s, valid, torch.float32)
        out = ops.unsqueeze_act(ud, T, s, valid=_vt(valid, cuda))
        assert out.shape == (B, T, H) and _bits_equal(out, ops.unsqueeze_act(ud, T, s, valid=_vt(valid, cuda)))
        if s * Tv < T:
            assert out[:, s * Tv:].abs().max().item() == 0.0
        _measured(f"out ({tag})", out, r32[0], r64[0], 5e-6)
        dn = d.clone()
        dn[:, s * Tv:] = float("nan")
        du = ops.unsqueeze_act_bwd(ud, dn.to(cuda), s, valid=_vt(valid, cuda))
        assert du.shape == (B, T2, s * H) and torch.isfinite(du).all()
        assert _bits_equal(du, ops.unsqueeze_act_bwd(ud, dn.to(cuda), s, valid=_vt(valid, cuda)))
        if Tv < T2:
            assert du[:, Tv:].abs().max().item() == 0.0
        _measured(f"du ({tag})", du, r32[1], r64[1], 2e-5)
        assert _bits_equal(ud, u_before)


def test_row_mean_of_fifty(cuda):
    """Input mean 50, unit variance: x - mean alone carries ulp(50) / 2 = 1.9e-6, so a sum-of-squares variance would lose five digits and
    every bound is measured (4 x torch's fp32 error + the floor), the sibling file's rule for inputs that make the plain bounds meaningless.
    531 squeezed rows: several workgroups and a tail."""
    from dynamic_asr_eval_amd import ops
    B, T, H, G, s = 3, 355, 512, 16, 2
    T2 = T // s
    h, y, yg, bias, gamma, beta, dz, old = _inputs(B, T, H, G, s, 1, mean=50.0, std=1.0, extra=0)
    r64 = _squeeze_ref(h, y, bias, gamma, beta, dz, s, None, torch.float64)
    r32 = _squeeze_ref(h, y, bias, gamma, beta, dz, s, None, torch.float32)
    hd, ygd, bd, gd, td = (t.to(cuda) for t in (h, yg, bias, gamma, beta))
    z, mean, rstd = ops.squeeze_ln(hd, ygd, bd, gd, td, s, EPS)
    _measured("z", z, r32[0], r64[0], 5e-6)
    _measured("mean", mean, r32[1], r64[1], 5e-6)
    _measured("rstd (rel)", rstd, r32[2], r64[2], 5e-6, rel=True)
    dg, db, dc = (old[k].to(cuda) for k in range(3))
    dh, dyg = ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dz.to(cuda), s, dg, db, dc, wgrad_beta=0.0)
    _measured("dh", dh, r32[3], r64[3], 2e-5)
    _measured("dyg", dyg, _grouped(r32[4], G), _grouped(r64[4], G), 2e-5)
    wtol = K.wgrad_tol(5e-4, B * T2, 531)
    for k, (name, got) in enumerate((("dgamma", dg), ("dbeta", db), ("dbias", dc))):
        _measured(name, got, r32[5 + k], r64[5 + k], wtol)


def test_identical_under_reduce_defer(cuda):
    """The column sums recorded under ops.reduce_defer (as the model's backward runs them) are bit-identical to the direct call's."""
    from dynamic_asr_eval_amd import ops
    B, T, H, G, s = 1, 2062, 768, 16, 2
    h, y, yg, bias, gamma, beta, dz, old = _inputs(B, T, H, G, s, 2, extra=0)
    hd, ygd, bd, gd, td, dzd = (t.to(cuda) for t in (h, yg, bias, gamma, beta, dz))
    valid = _vt(1000, cuda)
    z, mean, rstd = ops.squeeze_ln(hd, ygd, bd, gd, td, s, EPS, valid=valid)

    def bwd(arena):
        w = [old[k].to(cuda) for k in range(3)]
        with ops.reduce_defer(arena):
            dh, dyg = ops.squeeze_ln_bwd(hd, ygd, bd, gd, mean, rstd, dzd, s, *w, wgrad_beta=1.0, valid=valid)
        return [dh, dyg] + w

    first = bwd(None)
    arena = torch.empty(16 << 20, dtype=torch.uint8, device=cuda)
    assert arena.data_ptr() % 256 == 0
    deferred = bwd(arena)
    for k, name in enumerate(("dh", "dyg", "dgamma", "dbeta", "dbias")):
        assert _bits_equal(first[k], deferred[k]), f"{name}: differs under ops.reduce_defer"
    assert not _bits_equal(deferred[4], old[2])             # the recorded reduction did run at the flush
    r64 = _squeeze_ref(h, y, bias, gamma, beta, dz, s, 1000, torch.float64)
    wtol = K.wgrad_tol(5e-4, 1000, 531)
    for k, name in enumerate(("dgamma", "dbeta", "dbias")):
        _check(f"{name} over 1000 rows", first[2 + k], r64[5 + k] + old[k].double(), wtol)


def test_wrappers_refuse_what_is_not_built_before_any_launch(cuda):
    """H = 384, s = 5 and cg % 4 != 0 are refused on the host by the wrappers (DynError naming the constraint) and by the library entries
    (DYN_E_ARG): the outputs stay untouched."""
    from dynamic_asr_eval_amd import _lib, ops

    def args(B, T, H, G, s):
        T2 = max(T // max(s, 1), 1)
        return (torch.randn(B, T, H, device=cuda), torch.randn(B, G, T2, H // G, device=cuda)) + tuple(torch.randn(H, device=cuda) for _ in range(3))

    for (H, G, s), word in (((384, 16, 2), "256"), ((256, 16, 5), "1, 2, 3 or 4"), ((768, 128, 2), "multiple of 4")):
        h, yg, b, g, t = args(1, 10, H, G, s)
        with pytest.raises(ops.DynError) as e:
            ops.squeeze_ln(h, yg, b, g, t, s)
        assert word in str(e.value), str(e.value)
        with pytest.raises(ops.DynError) as e:
            ops.squeeze_ln_bwd(h, yg, b, g, torch.zeros(10, device=cuda), torch.zeros(10, device=cuda), torch.zeros(1, 10 // s, H, device=cuda), s,
                               None, None, None)
        assert word in str(e.value), str(e.value)
    for fn in (lambda: ops.unsqueeze_act(torch.randn(1, 2, 5 * 256, device=cuda), 10, 5),
               lambda: ops.unsqueeze_act_bwd(torch.randn(1, 2, 5 * 256, device=cuda), torch.randn(1, 10, 256, device=cuda), 5)):
        with pytest.raises(ops.DynError) as e:
            fn()
        assert "1, 2, 3 or 4" in str(e.value)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ws = ops.workspace(cuda)
    src = torch.randn(4 * 10 * 1024, device=cuda)
    buf = torch.full((4 * 10 * 1024,), 7.0, device=cuda)
    stat = torch.zeros(64, device=cuda)
    p = src.data_ptr()
    for (H, G, s), word in (((384, 16, 2), b"256"), ((256, 16, 5), b"squeeze factor"), ((768, 128, 2), b"multiple of 4")):
        rc = lib.dyn_squeeze_ln_fwd(p, p, p, p, p, buf.data_ptr(), stat.data_ptr(), stat.data_ptr(), 2, 10, 5, H, G, s, EPS, None, st)
        assert rc == -1 and b"dyn_squeeze_ln_fwd" in lib.dyn_last_error() and word in lib.dyn_last_error(), lib.dyn_last_error()
        rc = lib.dyn_squeeze_ln_bwd(p, p, p, p, stat.data_ptr(), stat.data_ptr(), p, buf.data_ptr(), buf.data_ptr(), 0, 0, 0, 1.0, 2, 10, 5, H, G,
                                    s, None, ws.data_ptr(), ws.numel(), st)
        assert rc == -1 and b"dyn_squeeze_ln_bwd" in lib.dyn_last_error() and word in lib.dyn_last_error(), lib.dyn_last_error()
    rc = lib.dyn_unsqueeze_act_fwd(p, buf.data_ptr(), 2, 10, 256, 5, None, st)
    assert rc == -1 and b"squeeze factor" in lib.dyn_last_error()
    rc = lib.dyn_unsqueeze_act_bwd(p, p, buf.data_ptr(), 2, 10, 256, 0, None, st)
    assert rc == -1 and b"squeeze factor" in lib.dyn_last_error()
    rc = lib.dyn_squeeze_ln_fwd(p, p, p, p, p, buf.data_ptr(), stat.data_ptr(), stat.data_ptr(), 2, 10, 4, 256, 16, 2, EPS, None, st)
    assert rc == -1 and b"Tg" in lib.dyn_last_error()                          # fewer yg rows than T / s
    rc = lib.dyn_squeeze_ln_bwd(p, p, p, p, stat.data_ptr(), stat.data_ptr(), p, buf.data_ptr(), buf.data_ptr(), stat.data_ptr(), 0, 0, 1.0, 2, 10,
                                5, 256, 16, 2, None, ws.data_ptr(), 15, st)
    assert rc == -3                                                            # DYN_E_WORKSPACE
    torch.cuda.synchronize()
    assert (buf == 7.0).all() and (stat == 0.0).all()
