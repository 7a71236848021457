"""dyn_attn_adapter_fwd / _bwd (the MMS bottleneck adapter with its residual, y = x + W2 relu(W1 LayerNorm(x) + b1) + b2, one launch forward and
two backward) against float64 torch on the CPU — x + F.linear(F.relu(F.linear(F.layer_norm(x), W1, b1)), W2, b2) and its autograd — in the
conventions of test_posconv_ln_gelu_gpu.py: y, mean, rstd, a at kernel_refs.measured_tol with the forward floor 5e-6, dx with floor 2e-5, the six
parameter gradients at kernel_refs.wgrad_tol(5e-4, M, 531) relative to each gradient's largest entry.  The ReLU's derivative jumps at 0, so the
backward reference takes its mask from the kernel's saved a > 0; that this mask is the float64 one outside |pre| <= 1e-4, and that the band
holds at most 1 % of the units, is asserted separately.  Every check prints `name: kernel error | torch fp32 error | bound` before it asserts."""
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
SHAPES = [(1, 256, 16), (37, 256, 16), (130, 1024, 16), (67, 1280, 16), (5, 256, 4), (33, 512, 64),       # (M, H, A)
          (37, 768, 16), (37, 1536, 16), (37, 1792, 16), (37, 2048, 16)]                                      # the other built widths
IDS = ["one-row", "partial-row-tile", "H1024-many-tiles", "mms-1b-width", "A4", "A64", "H768", "H1536", "H1792", "H2048"]
PARAMS = ("gamma", "beta", "W1", "b1", "W2", "b2")
_CACHE = {}


def _check(name, got, want, tol, e32=None, scale=1.0):
    err = K.max_err(got, want) / scale
    print(f"  {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _measured(name, got, torch32, want, floor):
    tol, e32 = K.measured_tol(torch32, want, floor)
    _check(name, got, want, tol, e32)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inputs(M, H, A):
    """Rows of mean 0.3 / std 2.0; linear weights randn / sqrt(fan_in) (the adapter's branch as large as the residual); b1 makes unit 0 dead
    and unit 1 alive on every row and leaves the rest mixed."""
    g = K.gen(9000 + M + H + A)
    p = dict(x=torch.randn(M, H, generator=g) * 2.0 + 0.3, gamma=torch.randn(H, generator=g) * 0.5 + 1.0, beta=torch.randn(H, generator=g),
             W1=torch.randn(A, H, generator=g) / H ** 0.5, b1=torch.randn(A, generator=g) * 0.3, W2=torch.randn(H, A, generator=g) / A ** 0.5,
             b2=torch.randn(H, generator=g), dy=torch.randn(M, H, generator=g))
    p["b1"][0], p["b1"][1] = -12.0, 12.0
    p["old"] = {n: torch.randn(p[n].shape, generator=g) for n in PARAMS}
    return p


def _torch_ref(p, dtype, mask=None, dy=None):
    """(y, mean, rstd, pre, a, dx, {six gradients}) from torch's ops and autograd in `dtype`; with `mask` the bottleneck is pre * mask (the
    ReLU with its kink decided by the caller)."""
    t = {n: p[n].detach().to(dtype).clone().requires_grad_() for n in ("x",) + PARAMS}
    H = p["x"].shape[-1]
    n = F.layer_norm(t["x"], (H,), t["gamma"], t["beta"], EPS)
    pre = F.linear(n, t["W1"], t["b1"])
    a = F.relu(pre) if mask is None else pre * mask.to(dtype)
    y = t["x"] + F.linear(a, t["W2"], t["b2"])
    y.backward((p["dy"] if dy is None else dy).to(dtype))
    xd = t["x"].detach()
    return (y.detach(), xd.mean(-1), torch.rsqrt(xd.var(-1, unbiased=False) + EPS), pre.detach(), a.detach(), t["x"].grad,
            {k: t[k].grad for k in PARAMS})


def _case(shape):
    if shape not in _CACHE:                                        # the references are computed once and shared, unchanged
        p = _inputs(*shape)
        _CACHE[shape] = (p, _torch_ref(p, torch.float64), _torch_ref(p, torch.float32))
    return _CACHE[shape]


def _forward(cuda, p, save=True, inplace=False):
    from dynamic_asr_eval_amd import ops
    d = {n: p[n].to(cuda) for n in ("x",) + PARAMS}
    x = d["x"].clone()
    out = ops.attn_adapter(x, d["gamma"], d["beta"], d["W1"], d["b1"], d["W2"], d["b2"], eps=EPS, out=x if inplace else None, save=save)
    return d, out


def _backward(cuda, d, saved, dy, old, skip=()):
    from dynamic_asr_eval_amd import ops
    mean, rstd, a = saved
    grads = {n: (None if n in skip else old[n].to(cuda).clone()) for n in PARAMS}
    dx = ops.attn_adapter_bwd(d["x"], d["gamma"], d["beta"], d["W1"], d["W2"], mean, rstd, a, dy, *(grads[n] for n in PARAMS))
    return dx, grads


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_against_float64(cuda, shape):
    M, H, A = shape
    p, r64, r32 = _case(shape)
    pre = r64[3]
    assert pre[:, 0].max().item() < 0.0 and pre[:, 1].min().item() > 0.0, "unit 0 must be dead and unit 1 alive on every row"
    if M >= 5:
        assert any(pre[:, k].min().item() < 0.0 < pre[:, k].max().item() for k in range(2, A)), "no mixed unit"
    d, (y, mean, rstd, a) = _forward(cuda, p)
    assert y.shape == (M, H) and mean.shape == rstd.shape == (M,) and a.shape == (M, A)
    assert _bits_equal(d["x"], p["x"]), "x must not be modified out of place"
    _measured("y", y, r32[0], r64[0], 5e-6)                        # ReLU is continuous: no element is left out
    _measured("mean", mean, r32[1], r64[1], 5e-6)
    _measured("rstd", rstd, r32[2], r64[2], 5e-6)
    _measured("a", a, r32[4], r64[4], 5e-6)
    assert a[:, 0].abs().max().item() == 0.0 and a.min().item() >= 0.0
    _, (y2, none_m, none_r, none_a) = _forward(cuda, p, save=False)
    assert none_m is None and none_r is None and none_a is None and _bits_equal(y, y2), "with and without the optional outputs: same y bits"
    _, (y3, _, _, _) = _forward(cuda, p, save=False, inplace=True)
    assert _bits_equal(y, y3), "in place (y is x) must give the bits of out of place"
    _, (y4, mean4, rstd4, a4) = _forward(cuda, p, save=True, inplace=True)
    assert _bits_equal(y, y4) and _bits_equal(mean, mean4) and _bits_equal(rstd, rstd4) and _bits_equal(a, a4)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_against_float64(cuda, shape):
    """Accumulation onto non-zero old gradients (beta = 1); the same call twice gives the same bits; x and dy are left unmodified."""
    M, H, A = shape
    p, r64, _ = _case(shape)
    d, (y, mean, rstd, a) = _forward(cuda, p)
    mask = (a > 0).cpu()
    pre = r64[3]
    far = pre.abs() > 1e-4
    assert torch.equal(mask[far], (pre > 0)[far]), "the kernel's ReLU mask differs from float64's outside the band |pre| <= 1e-4"
    share = 1.0 - far.double().mean().item()
    print(f"  units inside the band: {share:.2e}")
    assert share <= 0.01
    m64, m32 = _torch_ref(p, torch.float64, mask), _torch_ref(p, torch.float32, mask)
    dy = p["dy"].to(cuda)
    dx, grads = _backward(cuda, d, (mean, rstd, a), dy, p["old"])
    assert _bits_equal(d["x"], p["x"]) and _bits_equal(dy, p["dy"]), "x and dy must be left unmodified"
    _measured("dx", dx, m32[5], m64[5], 2e-5)
    wtol = K.wgrad_tol(5e-4, M, 531)
    for n in PARAMS:
        want = m64[6][n]
        _check("d" + n, grads[n].cpu().double() - p["old"][n].double(), want, wtol, K.max_err(m32[6][n], want) / want.abs().max().item(),
               scale=want.abs().max().item())
    dx2, grads2 = _backward(cuda, d, (mean, rstd, a), dy, p["old"])
    assert _bits_equal(dx, dx2) and all(_bits_equal(grads[n], grads2[n]) for n in PARAMS), "the same call twice must give the same bits"


def test_null_gradients_and_zero_rows(cuda):
    """M = 37.  Every single null gradient pointer leaves the other outputs' bits unchanged (all six null as well).  With the last 5 rows of
    dy zero, dx has exact-zero rows there and every parameter gradient is BIT-IDENTICAL to the call on the first 32 rows alone: rows map to
    workgroups four at a time from row 0 and to the second stage's waves by row index, so the 32 rows keep their places in every sum and the
    5 rows add exact zeros (the tile boundary does not move)."""
    shape = (37, 256, 16)
    M, H, A = shape
    p, _, _ = _case(shape)
    d, (y, mean, rstd, a) = _forward(cuda, p)
    dy = p["dy"].to(cuda)
    dx, grads = _backward(cuda, d, (mean, rstd, a), dy, p["old"])
    for n in PARAMS:
        dxn, gn = _backward(cuda, d, (mean, rstd, a), dy, p["old"], skip=(n,))
        assert gn[n] is None and _bits_equal(dx, dxn), n
        assert all(_bits_equal(grads[k], gn[k]) for k in PARAMS if k != n), n
    dx0, g0 = _backward(cuda, d, (mean, rstd, a), dy, p["old"], skip=PARAMS)
    assert _bits_equal(dx, dx0) and all(v is None for v in g0.values())
    dyz = dy.clone()
    dyz[32:] = 0.0
    dxz, gz = _backward(cuda, d, (mean, rstd, a), dyz, p["old"])
    assert dxz[32:].abs().max().item() == 0.0 and dxz[:32].abs().max().item() > 0.0
    d32 = dict(d, x=d["x"][:32].contiguous())
    dx32, g32 = _backward(cuda, d32, (mean[:32].contiguous(), rstd[:32].contiguous(), a[:32].contiguous()), dyz[:32].contiguous(), p["old"])
    assert _bits_equal(dxz[:32], dx32)
    for n in PARAMS:
        assert _bits_equal(gz[n], g32[n]), n
    zero_old = {n: torch.zeros_like(v) for n, v in p["old"].items()}
    _, gzero = _backward(cuda, d, (mean, rstd, a), torch.zeros_like(dy), zero_old)
    assert all(gzero[n].abs().max().item() == 0.0 for n in PARAMS), "an all-zero dy must add nothing to any sum"


def test_wrappers_refuse_what_the_kernels_do_not_take(cuda):
    from dynamic_asr_eval_amd import ops
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    for H, A, word in ((300, 16, "H = 300"), (2304, 16, "H = 2304"), (256, 6, "A = 6"), (256, 68, "A = 68")):
        with pytest.raises(ops.DynError) as e:
            ops.attn_adapter(z(3, H), z(H), z(H), z(A, H), z(A), z(H, A), z(H))
        assert word in str(e.value)
    x = z(3, 256)
    with pytest.raises(ops.DynError) as e:
        ops.attn_adapter_bwd(x, z(256), z(256), z(16, 256), z(256, 16), z(3), z(3), z(3, 16), x, None, None, None, None, None, None, dx=x)
    assert "alias" in str(e.value)
