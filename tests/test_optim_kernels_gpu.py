"""Float64 parity of the flat optimiser step (csrc/optim.hip) past the one case tests/test_ops_gpu.py holds (n = 10007, weight_decay 0):
the `n < 4` and `n % 4` scalar tails, the grid-stride loop (one sweep is 256 workgroups x 256 threads x 4 floats = 262144 elements), the
weight-decay line of both optimisers, the in-kernel initialisation of the state at step 0, every state buffer at every step, and the
unclipped / all-zero paths of the gradient-norm clip.

The references are oracle.madgrad_ref.MADGRAD and torch.optim.Adam run on float64 CPU copies of the same fp32 inputs.  The bound of every
compared buffer is MEASURED (kernel_refs.measured_tol): 4 x the error of the same optimiser run in fp32 on the CPU against the float64 run,
plus 2e-6 (the assertion of test_optimizers_match_torch).  Every check prints `name: kernel error | torch fp32 error | bound`."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
SIZES = [1, 3, 4, 5, 262144, 262147, 524295]     # 524295 = two sweeps + a scalar tail of 3
STEPS = 5
SENTINEL = -12345.678
TAIL = 8


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """p0 and the five gradients (0.1 * randn; step 2 scaled x 10), fp32, shared by every case of size n and left unchanged."""
    g = K.gen(3000 + n % 9973)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * (1.0 if k == 2 else 0.1) for k in range(STEPS)]


def _state(cuda, n):
    """NaN-filled state buffer of n floats with a sentinel tail: step 0 must initialise it in-kernel."""
    buf = torch.full((n + TAIL,), SENTINEL, device=cuda)
    buf[:n] = float("nan")
    return buf


def _param(cuda, p0):
    buf = torch.full((p0.numel() + TAIL,), SENTINEL, device=cuda)
    buf[:p0.numel()] = p0.to(cuda)
    return buf


def _compare(what, bufs, n, refs64, refs32):
    for name, buf in bufs.items():
        got = buf[:n]
        assert not torch.isnan(got).any(), f"{what}: nan in {name}"
        assert bool((buf[n:] == SENTINEL).all().item()), f"{what}: {name} written past n"
        tol, e32 = K.measured_tol(refs32[name], refs64[name], 2e-6)
        err = K.max_err(got, refs64[name])
        print(f"  {what} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
        assert err <= tol, f"{what} {name}: err {err} > {tol} (torch fp32: {e32})"


def _madgrad_cpu(p0, grads, dtype, lr, momentum, wd, eps):
    """oracle MADGRAD in `dtype` on the CPU: per step the dict of p, s, nu and x0 (for momentum 0, where the oracle keeps no x0, the value its
    step derives: p + s / (nu^(1/3) + eps) from the state before the update)."""
    from oracle.madgrad_ref import MADGRAD
    p = p0.to(dtype).clone().requires_grad_()
    opt = MADGRAD([p], lr=lr, momentum=momentum, weight_decay=wd, eps=eps)
    out = []
    for g in grads:
        if momentum == 0:
            st = opt.state[p]
            s_b = st["s"].clone() if "s" in st else torch.zeros_like(p.data)
            nu_b = st["grad_sum_sq"].clone() if "s" in st else torch.zeros_like(p.data)
            x0 = p.data + s_b / (nu_b.pow(1 / 3) + eps)
        p.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[p]
        out.append(dict(p=p.data.clone(), s=st["s"].clone(), nu=st["grad_sum_sq"].clone(), x0=x0.clone() if momentum == 0 else st["x0"].clone()))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("n", SIZES)
def test_madgrad_step(cuda, n, momentum, wd):
    from dynamic_asr_eval_amd import ops
    lr, eps = 9e-5, 1e-6
    p0, grads = _inputs(n)
    ref64 = _madgrad_cpu(p0, grads, F64, lr, momentum, wd, eps)
    ref32 = _madgrad_cpu(p0, grads, torch.float32, lr, momentum, wd, eps)
    bufs = dict(p=_param(cuda, p0), s=_state(cuda, n), nu=_state(cuda, n), x0=_state(cuda, n))
    for k, g in enumerate(grads):
        gd = g.to(cuda)
        ops.madgrad_step(bufs["p"][:n], gd, bufs["s"][:n], bufs["nu"][:n], bufs["x0"][:n], lr, momentum, wd, eps, k)
        assert torch.equal(gd.cpu(), g), "the gradient is an input"
        _compare(f"madgrad n={n} m={momentum} wd={wd} step {k}", bufs, n, ref64[k], ref32[k])


def _adam_cpu(p0, grads, dtype, lr, wd):
    p = p0.to(dtype).clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd)
    out = []
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[p]
        out.append(dict(p=p.data.clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone()))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step(cuda, n, wd):
    """weight_decay is L2 (added to the gradient), as in torch.optim.Adam — not AdamW."""
    from dynamic_asr_eval_amd import ops
    lr = 1e-3
    p0, grads = _inputs(n)
    ref64, ref32 = _adam_cpu(p0, grads, F64, lr, wd), _adam_cpu(p0, grads, torch.float32, lr, wd)
    bufs = dict(p=_param(cuda, p0), m=_state(cuda, n), v=_state(cuda, n))
    for k, g in enumerate(grads):
        ops.adam_step(bufs["p"][:n], g.to(cuda), bufs["m"][:n], bufs["v"][:n], lr, 0.9, 0.999, 1e-8, wd, k)
        _compare(f"adam n={n} wd={wd} step {k}", bufs, n, ref64[k], ref32[k])


# ----------------------------------------------------------------------------------------------------------- clip_grad_norm
def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", [1, 5, 262147, 1_050_001])
def test_clip_grad_norm(cuda, n):
    """1 050 001 elements pass the 1024-partial cap.  Clipping: the norm within 1e-6 relative of float64, the gradients within the measured
    bound (floor 1e-6, the "clip" assertion of test_optimizers_match_torch).  Not clipping: coefficient exactly 1 and every gradient
    bit-unchanged.  All zeros: norm 0, unchanged."""
    from dynamic_asr_eval_amd import ops
    g = torch.randn(n, generator=K.gen(4000 + n % 9973)) * 3
    norm64 = torch.sqrt((g.double() ** 2).sum()).item()

    def run(src, max_norm):
        buf = torch.full((n + TAIL,), SENTINEL, device=cuda)
        buf[:n] = src.to(cuda)
        out = ops.clip_grad_norm(buf[:n], max_norm)
        assert bool((buf[n:] == SENTINEL).all().item()), "written past n"
        return buf[:n], out.cpu().double()

    # clipping: max_norm is half the norm
    max_norm = float(torch.tensor(0.5 * norm64, dtype=torch.float32))
    got, nc = run(g, max_norm)
    coef64 = max_norm / (norm64 + 1e-6)
    prm = torch.nn.Parameter(torch.zeros(n))
    prm.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([prm], max_norm)
    tol, e32 = K.measured_tol(prm.grad, g.double() * coef64, 1e-6)
    err = K.max_err(got, g.double() * coef64)
    rel_n, rel_c = abs(nc[0].item() / norm64 - 1), abs(nc[1].item() / coef64 - 1)
    print(f"  clip n={n}: norm rel {rel_n:.2e}, coefficient rel {rel_c:.2e} | bound 1e-06; gradients kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert rel_n <= 1e-6 and rel_c <= 1e-6 and err <= tol, f"n={n}: norm rel {rel_n}, coefficient rel {rel_c}, gradients {err} > {tol} (torch fp32: {e32})"
    # not clipping: the early return
    got, nc = run(g, float(2 * norm64 + 1))
    assert nc[1].item() == 1.0 and _bits_equal(got, g) and abs(nc[0].item() / norm64 - 1) <= 1e-6
    # all zeros
    got, nc = run(torch.zeros(n), 10.0)
    assert nc[0].item() == 0.0 and nc[1].item() == 1.0 and _bits_equal(got, torch.zeros(n))
