"""Per-kernel parity: every HIP op (through the C-ABI) against the torch CPU op the reference path calls,
on the same seeded inputs.  Tolerances are written next to each check; integer outputs are bit-exact."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol, what=""):
    err = (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()
    assert err <= tol, f"{what}: max abs err {err} > {tol}"


def test_silu_glu_axpby(cuda):
    from dynamic_asr_eval_amd import ops
    x = torch.randn(37, 1030, generator=_g(0)) * 3
    dy = torch.randn(37, 1030, generator=_g(1))
    xr = x.clone().requires_grad_()
    F.silu(xr).backward(dy)
    _close(ops.silu(x.to(cuda)), F.silu(x), 1e-6, "silu")
    _close(ops.silu_bwd(x.to(cuda), dy.to(cuda)), xr.grad, 2e-6, "silu_bwd")
    u = torch.randn(50, 2 * 768, generator=_g(2))
    dg = torch.randn(50, 768, generator=_g(3))
    ur = u.clone().requires_grad_()
    F.glu(ur, dim=-1).backward(dg)
    _close(ops.glu(u.to(cuda)), F.glu(u, dim=-1), 1e-6, "glu")
    _close(ops.glu_bwd(u.to(cuda), dg.to(cuda)), ur.grad, 2e-6, "glu_bwd")
    y = torch.randn(1001, generator=_g(4)); x1 = torch.randn(1001, generator=_g(5))
    yc = y.to(cuda)
    ops.axpby(x1.to(cuda), yc, 0.5, 2.0)
    _close(yc, 0.5 * x1 + 2.0 * y, 1e-6, "axpby")


def test_colsum_transpose_specaug(cuda):
    from dynamic_asr_eval_amd import ops
    x = torch.randn(5000, 300, generator=_g(6))
    out = torch.ones(300, device=cuda)
    ops.colsum(x.to(cuda), out, beta=1.0)
    _close(out, 1.0 + x.double().sum(0), 2e-3, "colsum")
    spec = torch.randn(80, 1000, generator=_g(7)).to(cuda)
    win = spec[:, 100:613]
    _close(ops.transpose_ft(win), win.cpu().T.contiguous(), 0.0, "transpose_ft")
    w = win.contiguous()
    f0 = torch.tensor([3, 40, 75], dtype=torch.int32, device=cuda)
    wd = torch.tensor([5, 0, 10], dtype=torch.int32, device=cuda)
    ref = w.cpu().clone(); ref[3:8] = 0; ref[75:80] = 0
    ops.specaug_freqmask(w, f0, wd, 0.0)
    _close(w, ref, 0.0, "specaug")


@pytest.mark.parametrize("C", [256, 768, 1024])
def test_layernorm_rmsnorm(cuda, C):
    from dynamic_asr_eval_amd import ops
    rows = 531
    x = torch.randn(rows, C, generator=_g(8)) * 2 + 0.3
    g = torch.randn(C, generator=_g(9)); b = torch.randn(C, generator=_g(10))
    dy = torch.randn(rows, C, generator=_g(11))
    xr, gr, br = x.clone().requires_grad_(), g.clone().requires_grad_(), b.clone().requires_grad_()
    F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy)
    y, mean, rstd = ops.layernorm(x.to(cuda), g.to(cuda), b.to(cuda), 1e-5)
    _close(y, F.layer_norm(x, (C,), g, b, 1e-5), 5e-6, "ln fwd")
    dx = torch.ones(rows, C, device=cuda)
    dg = torch.zeros(C, device=cuda); db = torch.zeros(C, device=cuda)
    ops.layernorm_bwd(x.to(cuda), g.to(cuda), mean, rstd, dy.to(cuda), dx, dg, db, dx_beta=1.0, wgrad_beta=0.0)
    _close(dx, xr.grad + 1.0, 2e-5, "ln dx")
    _close(dg, gr.grad, 5e-4, "ln dgamma")
    _close(db, br.grad, 5e-4, "ln dbeta")
    # RMSNorm: y = x * rsqrt(mean(x^2) + eps) * g
    xr, gr = x.clone().requires_grad_(), g.clone().requires_grad_()
    (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-5) * gr).backward(dy)
    y, rstd = ops.rmsnorm(x.to(cuda), g.to(cuda), 1e-5)
    _close(y, x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * g, 5e-6, "rms fwd")
    dx = torch.zeros(rows, C, device=cuda); dg = torch.zeros(C, device=cuda)
    ops.rmsnorm_bwd(x.to(cuda), g.to(cuda), rstd, dy.to(cuda), dx, dg, dx_beta=0.0, wgrad_beta=0.0)
    _close(dx, xr.grad, 2e-5, "rms dx")
    _close(dg, gr.grad, 5e-4, "rms dgamma")


@pytest.mark.parametrize("L", [1, 63, 129, 256, 1992, 2048, 4096])
def test_softmax_family(cuda, L):
    """Rows up to 4096 (ITEMS <= 16).  Rows beyond that, both edges of every instance up to the limits (16384 forward, 8192 backward),
    more rows than a grid, padded strides and the masked forms: tests/test_row_kernels_gpu.py."""
    from dynamic_asr_eval_amd import ops
    rows = 77
    x = torch.randn(rows, L, generator=_g(12)) * 4
    dy = torch.randn(rows, L, generator=_g(13))
    xr = x.clone().requires_grad_(); F.softmax(xr, -1).backward(dy)
    y = ops.softmax(x.to(cuda))
    _close(y, F.softmax(x, -1), 2e-6, "softmax")
    _close(ops.softmax_bwd(y, dy.to(cuda), scale=0.5), 0.5 * xr.grad, 5e-6, "softmax_bwd")
    xr = x.clone().requires_grad_(); F.log_softmax(xr, -1).backward(dy)
    y = ops.log_softmax(x.to(cuda))
    _close(y, F.log_softmax(x, -1), 1e-5, "log_softmax")
    # sum(dy) over L N(0,1) terms is O(sqrt(L)) and is rounded differently by the two fp32 summation orders
    _close(ops.log_softmax_bwd(y, dy.to(cuda)), xr.grad, 2e-6 * max(L, 16), "log_softmax_bwd")


@pytest.mark.parametrize("T,C,KW", [(200, 768, 9), (33, 300, 9), (5, 256, 31), (64, 512, 3)])
def test_dwconv1d(cuda, T, C, KW):
    from dynamic_asr_eval_amd import ops
    B = 2
    x = torch.randn(B, T, C, generator=_g(14)); w = torch.randn(C, KW, generator=_g(15)); b = torch.randn(C, generator=_g(16))
    dy = torch.randn(B, T, C, generator=_g(17))
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    ref = F.conv1d(xr.transpose(1, 2), wr.unsqueeze(1), br, padding=(KW - 1) // 2, groups=C).transpose(1, 2)
    ref.backward(dy)
    _close(ops.dwconv1d(x.to(cuda), w.to(cuda), b.to(cuda)), ref, 2e-5, "dwconv1d fwd")
    dx = torch.ones(B, T, C, device=cuda)
    ops.dwconv1d_dgrad(dy.to(cuda), w.to(cuda), dx, beta=1.0)
    _close(dx, xr.grad + 1, 2e-5, "dwconv1d dgrad")
    dw = torch.zeros(C, KW, device=cuda); db = torch.zeros(C, device=cuda)
    ops.dwconv1d_wgrad(x.to(cuda), dy.to(cuda), dw, db, beta=0.0)
    _close(dw, wr.grad, 3e-4, "dwconv1d wgrad")
    _close(db, br.grad, 3e-4, "dwconv1d bgrad")


@pytest.mark.parametrize("T,Fq,C", [(64, 80, 256), (37, 21, 96), (1, 1, 32), (5, 7, 6), (9, 12, 516)])
def test_subsampling_convs(cuda, T, Fq, C):
    from dynamic_asr_eval_amd import ops
    B = 2
    x = torch.randn(B, T, Fq, generator=_g(18))
    w1 = torch.randn(C, 3, 3, generator=_g(19)) * 0.3; b1 = torch.randn(C, generator=_g(20))
    w1r, b1r = w1.clone().requires_grad_(), b1.clone().requires_grad_()
    z_ref = F.conv2d(x.unsqueeze(1), w1r.unsqueeze(1), b1r, stride=2, padding=1)  # [B, C, To, Fo]
    dz = torch.randn(z_ref.shape, generator=_g(21))
    z_ref.backward(dz)
    z = ops.conv2d_first(x.to(cuda), w1.to(cuda), b1.to(cuda))
    _close(z, z_ref.permute(0, 2, 3, 1), 2e-5, "conv2d_first fwd")
    dw = torch.zeros(C, 3, 3, device=cuda); db = torch.zeros(C, device=cuda)
    ops.conv2d_first_wgrad(x.to(cuda), dz.permute(0, 2, 3, 1).contiguous().to(cuda), dw, db, beta=0.0)
    _close(dw, w1r.grad, 1e-3, "conv2d_first wgrad")
    _close(db, b1r.grad, 1e-3, "conv2d_first bgrad")
    # depthwise stride-2 with fused input SiLU
    zc = z_ref.detach().permute(0, 2, 3, 1).contiguous()  # channels-last [B, To, Fo, C]
    w2 = torch.randn(C, 3, 3, generator=_g(22)) * 0.3; b2 = torch.randn(C, generator=_g(23))
    zr, w2r, b2r = z_ref.detach().clone().requires_grad_(), w2.clone().requires_grad_(), b2.clone().requires_grad_()
    u_ref = F.conv2d(F.silu(zr), w2r.unsqueeze(1), b2r, stride=2, padding=1, groups=C)
    du = torch.randn(u_ref.shape, generator=_g(24))
    u_ref.backward(du)
    u = ops.dwconv2d_s2(zc.to(cuda), w2.to(cuda), b2.to(cuda))
    _close(u, u_ref.permute(0, 2, 3, 1), 5e-5, "dwconv2d fwd")
    duc = du.permute(0, 2, 3, 1).contiguous().to(cuda)
    _close(ops.dwconv2d_s2_dgrad(zc.to(cuda), w2.to(cuda), duc), zr.grad.permute(0, 2, 3, 1), 5e-5, "dwconv2d dgrad")
    dw = torch.zeros(C, 3, 3, device=cuda); db = torch.zeros(C, device=cuda)
    ops.dwconv2d_s2_wgrad(zc.to(cuda), duc, dw, db, beta=0.0)
    _close(dw, w2r.grad, 1e-3, "dwconv2d wgrad")
    _close(db, b2r.grad, 1e-3, "dwconv2d bgrad")


@pytest.mark.parametrize("B,T,Fq,C", [(2, 64, 80, 256), (1, 37, 21, 96), (2, 1, 1, 32), (1, 5, 7, 8), (1, 9, 12, 516), (1, 1026, 80, 64)])
def test_fused_first_two_subsampling_stages(cuda, B, T, Fq, C):
    """dyn_sub12_fwd / dyn_sub12_bwd (conv3x3_s2 -> SiLU -> dw3x3_s2 with the intermediate recomputed, never stored) against torch's
    conv2d chain + autograd, and against the unfused HIP kernels: the forward must be bit-identical to conv2d_first + dwconv2d_s2
    (same accumulation order), the four gradients equal up to summation order.  Odd sizes exercise every padding / parity case."""
    from dynamic_asr_eval_amd import ops
    g = _g(300 + T + C)
    x = torch.randn(B, T, Fq, generator=g)
    w1, b1 = torch.randn(C, 3, 3, generator=g) * 0.5, torch.randn(C, generator=g) * 0.3
    w2, b2 = torch.randn(C, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.3
    w1r, b1r, w2r, b2r = (t.clone().requires_grad_() for t in (w1, b1, w2, b2))
    z = F.conv2d(x.unsqueeze(1), w1r.unsqueeze(1), b1r, stride=2, padding=1)
    u_ref = F.conv2d(F.silu(z), w2r.unsqueeze(1), b2r, stride=2, padding=1, groups=C)            # [B, C, T2, F2]
    du = torch.randn(u_ref.shape, generator=g)
    u_ref.backward(du)
    xd, w1d, b1d, w2d, b2d = (t.to(cuda) for t in (x, w1, b1, w2, b2))
    u = ops.sub12_fwd(xd, w1d, b1d, w2d, b2d)
    assert tuple(u.shape) == (B, u_ref.shape[2], u_ref.shape[3], C)
    _close(u, u_ref.permute(0, 2, 3, 1), 1e-4, "fused subsampling fwd")
    unf = ops.dwconv2d_s2(ops.conv2d_first(xd, w1d, b1d), w2d, b2d)
    assert torch.equal(u, unf), "fused forward must be bit-identical to the two separate kernels"
    duc = du.permute(0, 2, 3, 1).contiguous().to(cuda)
    dw1, db1, dw2, db2 = (torch.full(s_, 0.5, device=cuda) for s_ in ((C, 3, 3), (C,), (C, 3, 3), (C,)))
    ops.sub12_bwd(xd, duc, w1d, b1d, w2d, dw1, db1, dw2, db2, beta=2.0)                        # beta: accumulates onto 2 * 0.5
    scale = max(1.0, float(T * Fq) ** 0.5)
    for got, want, name in ((dw1, w1r.grad, "dw1"), (db1, b1r.grad, "db1"), (dw2, w2r.grad, "dw2"), (db2, b2r.grad, "db2")):
        _close(got - 1.0, want, 2e-5 * scale * max(1.0, want.abs().max().item()), "fused subsampling " + name)
    again = [torch.full_like(t, 0.5) for t in (dw1, db1, dw2, db2)]
    ops.sub12_bwd(xd, duc, w1d, b1d, w2d, *again, beta=2.0)
    assert all(torch.equal(a, b) for a, b in zip(again, (dw1, db1, dw2, db2))), "deterministic"


def test_rotary_roundtrip_and_reference(cuda):
    from dynamic_asr_eval_amd import ops
    B, T, H, D = 2, 50, 3, 128
    qkv = torch.randn(B, T, 3 * H * D, generator=_g(25))
    inv = 1.0 / (1.5e6 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
    cos, sin = ang.cos().float(), ang.sin().float()
    x = qkv.to(cuda)
    ops.rotary(x, cos.to(cuda), sin.to(cuda), B, T, 2 * H, D, 3 * H * D)
    qk = qkv.view(B, T, 3 * H, D)[:, :, :2 * H]
    x1, x2 = qk[..., :D // 2], qk[..., D // 2:]
    c, s = cos[None, :, None], sin[None, :, None]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    got = x.view(B, T, 3 * H, D)
    _close(got[:, :, :2 * H], ref, 2e-6, "rotary fwd")
    _close(got[:, :, 2 * H:], qkv.view(B, T, 3 * H, D)[:, :, 2 * H:], 0.0, "rotary leaves v alone")
    ops.rotary(x, cos.to(cuda), sin.to(cuda), B, T, 2 * H, D, 3 * H * D, inverse=True)
    _close(x, qkv, 2e-6, "rotary inverse")


def _collapse(ids, blank):
    out, prev = [], None
    for i in ids:
        if i != blank and i != prev:
            out.append(i)
        prev = i
    return out


@pytest.mark.parametrize("T,C", [(1, 5), (64, 129), (2048, 4096), (3000, 33)])
def test_ctc_greedy_bit_exact(cuda, T, C):
    from dynamic_asr_eval_amd import ops
    B = 2
    lp = torch.randn(B, T, C, generator=_g(26))
    lp[:, :, C - 1] += 2.0  # blank-heavy like a trained model
    if T > 10:
        lp[0, 5:9] = lp[0, 4]  # forced repeats
        lp[1, 3, 7 % C] = lp[1, 3].max()  # exact tie: first maximum must win
    lp = F.log_softmax(lp, -1)
    ids, n = ops.ctc_greedy(lp.to(cuda), C - 1)
    for b in range(B):
        ref = _collapse(lp[b].argmax(-1).tolist(), C - 1)
        assert n[b].item() == len(ref)
        assert ids[b, :len(ref)].cpu().tolist() == ref


# lattice width L = 2 S + 1 selects the scan kernel (csrc/ctc.hip: 1024-thread workgroup, ITEMS = ceil(L / 1024) positions per thread):
# S <= 511 -> ctc_scan_kernel<1>, 512..1023 -> <2>, 1024..2047 -> <4>, 2048..4095 -> <8>.  The last six cases execute <2>, <4>, <8>
# (the prefetch-depth 4 / 2 variants), with repeated labels, a shorter second sample and both reductions.
@pytest.mark.parametrize("T,C,S,reduction", [(64, 129, 10, "sum"), (50, 33, 0, "sum"), (200, 129, 60, "mean"),
                                            (512, 4096, 255, "sum"), (30, 20, 12, "sum"),
                                            (2048, 4096, 600, "sum"), (1300, 129, 600, "mean"),
                                            (2048, 129, 1100, "sum"), (2300, 33, 1100, "mean"),
                                            (4200, 129, 2100, "sum"), (4300, 33, 2100, "mean")])
def test_ctc_loss_and_grad(cuda, T, C, S, reduction):
    from dynamic_asr_eval_amd import ops
    B = 2
    g = _g(27 + T)
    lp = F.log_softmax(torch.randn(B, T, C, generator=g), -1)
    tgt = torch.randint(0, C - 1, (B, max(S, 1)), generator=g)
    if S >= 4:
        tgt[0, 1] = tgt[0, 0]  # repeated label needs a blank between
        tgt[1, 3] = tgt[1, 1]
    if S >= 512:               # repeats across the 1024-position item boundaries of the wide scans, and a run of three
        for k in (511, 512, 1023, 1024, 2047):
            if k + 1 < S:
                tgt[0, k + 1] = tgt[0, k]
        tgt[1, 700 % S] = tgt[1, 700 % S - 1] = tgt[1, 700 % S - 2]
    tl = torch.tensor([S, max(S - S // 3 - 2, 0)]) if S >= 512 else torch.tensor([S, max(S - 2, 0)]) if S else torch.tensor([0, 0])
    il = torch.tensor([T, T - 3])
    lpr = lp.clone().requires_grad_()
    loss_ref = F.ctc_loss(lpr.transpose(0, 1), tgt[:, :max(S, 1)], il, tl, blank=C - 1, reduction=reduction)
    scale = 1.0 / (T * B)
    (loss_ref * scale).backward()
    loss, nll, grad = ops.ctc_loss(lp.to(cuda), tgt.int().to(cuda), il.int().to(cuda), tl.int().to(cuda), C - 1,
                                   reduction=reduction, grad_scale=scale)
    rel = abs(loss.item() - loss_ref.item()) / max(1.0, abs(loss_ref.item()))
    assert rel < 2e-6 * max(1, T // 64), (loss.item(), loss_ref.item())   # fp32 lattice, T serial log-sum-exps
    # |grad| <= scale per element; the fp32 lattice's log-domain error grows with the T serial log-sum-exps and with |alpha| ~ T * |lp|
    # (ulp(20000) = 2e-3 at T = 4200, C = 129: torch's own fp32 lattice is as far from float64 as this one, tests/drift_check.py)
    _close(grad, lpr.grad, scale * max(1.3e-3, 4e-6 * T), "ctc grad")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_device_libm_matches_the_host_libm(cuda):
    """csrc/libm_f32.h on the device against the expf / logf of THIS machine's libm.so.6 — the functions torch's CPU CTC kernel calls
    (aten/native/LossCTC.cpp: std::exp / std::log on float).  Bit for bit, NaN payloads aside."""
    import ctypes
    import numpy as np
    from dynamic_asr_eval_amd import ops
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype = ctypes.c_float; libm.expf.argtypes = [ctypes.c_float]
    libm.logf.restype = ctypes.c_float; libm.logf.argtypes = [ctypes.c_float]
    g = _g(271)
    n = 60000
    xs = torch.cat([
        -torch.rand(n, generator=g) * 110.0,                                  # the lattice's range, into the underflow band
        (torch.rand(n, generator=g) - 0.5) * 180.0,
        torch.randn(n, generator=g).exp() * 3.0,                              # logf arguments around 1 .. 3 (sums of up to three exps)
        torch.rand(n, generator=g) * 2.0 + 0.5,
        (torch.randint(0, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).int()).view(torch.float32),   # any positive bit pattern
        torch.tensor([0.0, -0.0, 1.0, 2.0, 3.0, -87.3, -88.0, -103.0, -103.97, -103.98, -104.0, 88.7, 88.8, 1e-45, 1e-40,
                      float("inf"), float("-inf"), float("nan"), -1.0, 0.5, 1.0000001, 0.99999994]),
    ])
    e, l, enp = (t.cpu().numpy() for t in ops.libm_f32(xs.to(cuda)))
    xn = xs.numpy()
    he = np.array([libm.expf(float(v)) for v in xn], dtype=np.float32)
    hl = np.array([libm.logf(float(v)) for v in xn], dtype=np.float32)

    def same(a, b):
        return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))
    assert same(e, he).all(), f"expf: {(~same(e, he)).sum()} of {len(xn)} differ, first at x = {xn[~same(e, he)][:5]}"
    assert same(l, hl).all(), f"logf: {(~same(l, hl)).sum()} of {len(xn)} differ, first at x = {xn[~same(l, hl)][:5]}"
    neg = (xn <= 0) & ~np.isnan(xn)
    assert same(enp[neg], he[neg]).all(), "the branch-free x <= 0 expf differs from libm"


# (T, C, S per sample, reduction): the BASELINE config-2 shape first (T' = 2048 encoder frames, V + 1 = 4096, a speech-like 450 labels),
# then the wider scan kernels <2>, <4>, an empty target and a short second sample.
@pytest.mark.parametrize("T,C,S,reduction", [(2048, 4096, (450, 431), "sum"), (2048, 129, (1030, 600), "sum"), (700, 33, (340, 0), "mean"),
                                            (2300, 129, (1100, 1024), "mean"), (300, 40, (0, 0), "sum")])
def test_ctc_lattice_is_bitwise_torch_cpu(cuda, T, C, S, reduction):
    """IDENTICAL log-probs into dyn_ctc_loss and into torch's CPU CTC (torch._ctc_loss returns (nll, log_alpha));
    the lattice, the nll and the gradient w.r.t. the log-probs must agree BIT FOR BIT — same libm roundings, same operation order."""
    from dynamic_asr_eval_amd import ops
    B = 2
    g = _g(4242 + T + C)
    logits = torch.randn(B, T, C, generator=g) * 3.0
    logits[:, :, C - 1] += 4.0   # blank-heavy and peaky like a trained model: |alpha| grows to the thousands
    lp = F.log_softmax(logits, -1)
    Sm = max(max(S), 1)
    tgt = torch.randint(0, C - 1, (B, Sm), generator=g)
    for b in range(B):           # repeated labels (no skip transition), a run of three, repeats far apart (prev_same chains)
        if S[b] >= 8:
            tgt[b, 1] = tgt[b, 0]
            tgt[b, 5] = tgt[b, 4] = tgt[b, 3]
            tgt[b, S[b] - 1] = tgt[b, 0]
    tl = torch.tensor(list(S)); il = torch.tensor([T, T - 5])
    nll_ref, alpha_ref = torch._ctc_loss(lp.transpose(0, 1), tgt, il.tolist(), tl.tolist(), C - 1, False)
    lpr = lp.clone().requires_grad_()
    scale = 1.0 / (T * B)
    (F.ctc_loss(lpr.transpose(0, 1), tgt, il, tl, blank=C - 1, reduction=reduction) * scale).backward()
    loss, nll, grad = ops.ctc_loss(lp.to(cuda), tgt.int().to(cuda), il.int().to(cuda), tl.int().to(cuda), C - 1,
                                   reduction=reduction, grad_scale=scale)
    alpha, beta, _ = ops.ctc_lattice(T, B, Sm, cuda)
    alpha = alpha.cpu()
    assert torch.equal(_bits(nll), _bits(nll_ref)), (nll.cpu().tolist(), nll_ref.tolist())
    cells = same_cells = 0
    for b in range(B):
        Tb, Lb = int(il[b]), 2 * int(tl[b]) + 1
        a, r = alpha[b, :Tb, :Lb], alpha_ref[b, :Tb, :Lb]
        cells += a.numel(); same_cells += int((_bits(a) == _bits(r)).sum())
    assert same_cells == cells, f"alpha: {cells - same_cells} of {cells} cells differ from torch's CPU lattice"
    gb, gr = _bits(grad), _bits(lpr.grad)
    assert torch.equal(gb, gr), f"gradient: {(gb != gr).sum().item()} of {gb.numel()} elements differ, max |d| {(grad.cpu() - lpr.grad).abs().max().item():.3e}"


def test_optimizers_match_torch(cuda):
    from dynamic_asr_eval_amd import ops
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from oracle.madgrad_ref import MADGRAD
    n = 10007
    for momentum in (0.9, 0.0):
        p0 = torch.randn(n, generator=_g(40))
        pr = p0.clone().requires_grad_()
        opt = MADGRAD([pr], lr=9e-5, momentum=momentum)
        p = p0.to(cuda); s = torch.empty(n, device=cuda); nu = torch.empty(n, device=cuda); x0 = torch.empty(n, device=cuda)
        for k in range(4):
            g = torch.randn(n, generator=_g(41 + k)) * (0.1 if k != 2 else 10.0)
            pr.grad = g.clone(); opt.step()
            ops.madgrad_step(p, g.to(cuda), s, nu, x0, 9e-5, momentum, 0.0, 1e-6, k)
            _close(p, pr, 2e-6, f"madgrad m={momentum} step {k}")
    p0 = torch.randn(n, generator=_g(50))
    pr = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pr], lr=1e-3)
    p = p0.to(cuda); m = torch.empty(n, device=cuda); v = torch.empty(n, device=cuda)
    for k in range(4):
        g = torch.randn(n, generator=_g(51 + k))
        pr.grad = g.clone(); opt.step()
        ops.adam_step(p, g.to(cuda), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, k)
        _close(p, pr, 2e-6, f"adam step {k}")
    g = torch.randn(n, generator=_g(60)) * 3
    gr = g.clone(); prm = torch.nn.Parameter(torch.zeros(n)); prm.grad = gr
    tn = torch.nn.utils.clip_grad_norm_([prm], 10.0)
    gc = g.to(cuda)
    nc = ops.clip_grad_norm(gc, 10.0)
    assert abs(nc[0].item() - tn.item()) < 1e-3
    _close(gc, prm.grad, 1e-6, "clip")


def test_stitch(cuda):
    from dynamic_asr_eval_amd import ops
    C, rows = 129, 40
    acc = torch.zeros(100, C, device=cuda); cnt = torch.zeros(100, device=cuda)
    ra, rc = torch.zeros(100, C), torch.zeros(100, C)
    pos = 0
    for i in range(3):
        lp = F.log_softmax(torch.randn(rows, C, generator=_g(70 + i)), -1)
        if i:
            pos -= 30
        ops.stitch_accumulate(lp.to(cuda), acc, cnt, pos)
        ra[pos:pos + rows] += lp.exp(); rc[pos:pos + rows] += 1
        pos += rows
    n = int((rc.sum(-1) != 0).sum())
    out = ops.stitch_finalize(acc, cnt, n)
    _close(out, torch.log(ra[:n] / rc[:n]), 2e-6, "stitch")


def test_optional_augmentations_match_reference_functions(cuda):
    """frame_shuffle / add_random_noise / cutout (reference lcasr/lib.py:81-84,379-417) with the same torch RNG stream."""
    from dynamic_asr_eval_amd import augment
    from oracle import augment_ref as R
    spec = torch.randn(1, 80, 600, generator=_g(80)) * 1.7 + 0.2
    for kw in (dict(time_dimension=True), dict(freq_dimension=True), dict(time_dimension=True, freq_dimension=True)):
        torch.manual_seed(5); ref = R.frame_shuffle(spec.clone(), **kw)
        torch.manual_seed(5); got = augment.frame_shuffle(spec[0].to(cuda).clone(), **kw)
        _close(got, ref[0], 0.0, f"frame_shuffle {kw}")
    torch.manual_seed(6); ref = R.add_random_noise(spec.clone(), 0.3)
    torch.manual_seed(6); got = augment.add_random_noise(spec[0].to(cuda).clone(), 0.3)
    _close(got, ref[0], 2e-5, "add_random_noise")
    for val in ("mean", "mean_recording", "zero"):
        torch.manual_seed(7); ref = R.cutout(spec.clone(), 600, cutout_val=val, num_rectangles=7, max_width=100, max_height=10)
        torch.manual_seed(7); got = augment.cutout(spec[0].to(cuda).clone(), 600, cutout_val=val, num_rectangles=7, max_width=100, max_height=10)
        _close(got, ref[0], 2e-6, f"cutout {val}")


def test_specaug_mask_args_matches_device_index_kernels(cuda):
    """dyn_specaug_mask_args (masks as kernel arguments) == dyn_specaug_freqmask / _timemask (masks in device buffers),
    including > 32 masks (chunked), zero-width masks, and a device-resident fill value."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.augment import SpecAugment
    g = torch.Generator().manual_seed(3)
    F, T = 80, 777
    x = torch.randn(F, T, generator=g).to(cuda)
    f0 = torch.randint(0, F - 10, (40,), generator=g).tolist(); fw = torch.randint(0, 10, (40,), generator=g).tolist()
    t0 = torch.randint(0, T - 50, (5,), generator=g).tolist(); tw = torch.randint(0, 50, (5,), generator=g).tolist()
    fill = torch.tensor([0.37], device=cuda)
    a = x.clone(); b = x.clone()
    ops.specaug_freqmask(a, torch.tensor(f0, dtype=torch.int32, device=cuda), torch.tensor(fw, dtype=torch.int32, device=cuda), fill)
    ops.specaug_timemask(a, torch.tensor(t0, dtype=torch.int32, device=cuda), torch.tensor(tw, dtype=torch.int32, device=cuda), fill)
    SpecAugment().apply(b, ((f0, fw), (t0, tw)), fill)
    assert torch.equal(a, b)
    c = x.clone()
    SpecAugment().apply(c, ((f0[:3], fw[:3]), ([], [])), 0.0)
    ref = x.clone()
    for s_, w_ in zip(f0[:3], fw[:3]):
        ref[s_:s_ + w_] = 0.0
    assert torch.equal(c, ref)


@pytest.mark.parametrize("B,T,H", [(1, 128, 1), (2, 100, 3), (1, 33, 2), (2, 2048, 2), (1, 257, 1)])
def test_fused_attention_forward(cuda, B, T, H):
    """dyn_attention_fwd (online softmax, scores never materialised) vs softmax(Q K^T / sqrt(D)) V in float64 on the packed
    QKV activation; ragged T exercises the masked last key tile and the clamped last query block."""
    from dynamic_asr_eval_amd import ops
    D = 128
    g = torch.Generator().manual_seed(B * 1000 + T + H)
    qkv = torch.randn(B, T, 3 * H * D, generator=g) * 1.5
    scale = 1.0 / D ** 0.5
    out = ops.attention_fwd(qkv.to(cuda), B, T, H, D, scale)
    x = qkv.double().view(B, T, 3, H, D)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)     # [B, H, T, D]
    ref = (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(B, T, H * D)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-5, err


@pytest.mark.parametrize("B,T,H,nsplit", [(1, 2048, 6, 0), (4, 2048, 6, 0), (1, 1000, 2, 3), (2, 513, 1, 2), (1, 4096, 1, 8), (1, 640, 3, 2)])
def test_fused_attention_forward_with_key_splits(cuda, B, T, H, nsplit):
    """dyn_attention_fwd_split: the keys of a query block split over several workgroups (normalised partial outputs + log-sum-exp
    per split, merged in split order) — automatic choice (0) and forced counts, ragged T, output AND lse vs float64; identical
    results on a second run; nsplit = 1 is bit-identical to the unsplit entry point."""
    from dynamic_asr_eval_amd import ops
    D = 128
    g = torch.Generator().manual_seed(B * 31 + T + H + nsplit)
    qkv = (torch.randn(B, T, 3 * H * D, generator=g) * 1.5).to(cuda)
    scale = 1.0 / D ** 0.5
    out, lse = ops.attention_fwd(qkv, B, T, H, D, scale, want_lse=True, nsplit=nsplit)
    x = qkv.cpu().double().view(B, T, 3, H, D)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    sc = q @ k.transpose(-1, -2) * scale
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, T, H * D)
    assert (out.cpu().double() - ref).abs().max().item() < 2e-5
    assert (lse.cpu().double() - torch.logsumexp(sc, -1)).abs().max().item() < 2e-5
    out2 = ops.attention_fwd(qkv, B, T, H, D, scale, nsplit=nsplit)
    assert torch.equal(out, out2)
    one, lse1 = ops.attention_fwd(qkv, B, T, H, D, scale, want_lse=True, nsplit=1)
    from dynamic_asr_eval_amd._lib import check, load
    base, HD = qkv.data_ptr(), H * D
    plain = torch.empty_like(one)
    check(load().dyn_attention_fwd(base, base + 4 * HD, base + 8 * HD, plain.data_ptr(), B, T, H, D, 3 * HD, T * 3 * HD, HD, T * HD, scale,
                                   torch.cuda.current_stream().cuda_stream), "dyn_attention_fwd")
    assert torch.equal(one, plain)
    assert (one - out).abs().max().item() < 2e-5


@pytest.mark.parametrize("B,T,H", [(1, 100, 6), (2, 257, 6), (1, 2048, 6), (2, 33, 1), (1, 128, 2)])
def test_fused_attention_grad_mode_forward_and_backward(cuda, B, T, H):
    """Grad-mode streaming attention: dyn_attention_fwd_lse (output + one log-sum-exp per query row) and dyn_attention_bwd (P re-formed
    tile by tile; query-owner workgroups -> dQ and delta, key-owner workgroups -> dK, dV; no atomics) against float64 autograd of
    softmax(Q K^T / sqrt(D)) V on the packed QKV activation.  Ragged T exercises the masked last tile and the clamped last owner block;
    two runs must agree bit for bit (deterministic)."""
    from dynamic_asr_eval_amd import ops
    D = 128
    g = torch.Generator().manual_seed(B * 977 + T + H)
    qkv = (torch.randn(B, T, 3 * H * D, generator=g) * 1.2)
    dout = torch.randn(B, T, H * D, generator=g)
    scale = 1.0 / D ** 0.5
    x = qkv.double().requires_grad_(True)
    xv = x.view(B, T, 3, H, D)
    q, k, v = xv[:, :, 0].transpose(1, 2), xv[:, :, 1].transpose(1, 2), xv[:, :, 2].transpose(1, 2)
    sc = q @ k.transpose(-1, -2) * scale
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, T, H * D)
    ref.backward(dout.double())
    out, lse = ops.attention_fwd(qkv.to(cuda), B, T, H, D, scale, want_lse=True)
    assert (out.cpu().double() - ref.detach()).abs().max().item() < 2e-5
    assert (lse.cpu().double() - torch.logsumexp(sc.detach(), -1)).abs().max().item() < 2e-5
    dqkv = ops.attention_bwd(qkv.to(cuda), out, dout.to(cuda), lse, B, T, H, D, scale)
    err = (dqkv.cpu().double() - x.grad).abs().max().item() / x.grad.abs().max().item()
    assert err < 2e-5, err
    again = ops.attention_bwd(qkv.to(cuda), out, dout.to(cuda), lse, B, T, H, D, scale)
    assert torch.equal(dqkv, again)


def test_deferred_column_reductions_match_the_separate_launches(cuda):
    """dyn_reduce_defer_begin / _flush: LayerNorm / RMSNorm / BatchRenorm weight gradients and bias column sums recorded and reduced in one
    batched launch — bit-identical to reducing at once, including reductions chained into one output (beta = 1, a shared parameter),
    beta = 0 overwrites, more than 96 recorded reductions (two launches), and an arena too small for everything (the rest reduces at once)."""
    from dynamic_asr_eval_amd import ops
    g = torch.Generator().manual_seed(5)
    rows, C = 1100, 768
    xs = [torch.randn(rows, C, generator=g).to(cuda) for _ in range(3)]
    dys = [torch.randn(rows, C, generator=g).to(cuda) for _ in range(3)]
    gam = torch.randn(C, generator=g).to(cuda)
    bet = torch.randn(C, generator=g).to(cuda)
    wide = torch.randn(900, 3072, generator=g).to(cuda)

    def run(arena, repeats):
        out = {}
        dgam, dbet = torch.full((C,), 0.25, device=cuda), torch.full((C,), -0.5, device=cuda)
        drms = torch.zeros(C, device=cuda)
        dw, db = torch.ones(C, device=cuda), torch.ones(C, device=cuda)
        bias_w = torch.full((3072,), 2.0, device=cuda)
        bias_c = torch.zeros(C, device=cuda)
        with ops.reduce_defer(arena):
            for r in range(repeats):
                for x, dy in zip(xs, dys):
                    y, mean, rstd = ops.layernorm(x, gam, bet)
                    ops.layernorm_bwd(x, gam, mean, rstd, dy, torch.empty_like(x), dgam, dbet, wgrad_beta=1.0)      # chained into one output
                    y2, rs = ops.rmsnorm(x, gam)
                    ops.rmsnorm_bwd(x, gam, rs, dy, torch.empty_like(x), drms, wgrad_beta=0.0 if r == 0 and x is xs[0] else 1.0)
                    ops.colsum(dy, bias_c, beta=1.0)
                ops.colsum(wide, bias_w, beta=0.5)
                var = torch.rand(C, generator=torch.Generator().manual_seed(3)).to(cuda) + 0.5
                ops.chanaffine_bwd(xs[0], bet, var, gam, dys[0], torch.empty_like(xs[0]), dw, db, wgrad_beta=1.0)
        out.update(dgam=dgam, dbet=dbet, drms=drms, dw=dw, db=db, bias_w=bias_w, bias_c=bias_c)
        return out

    with ops.use_workspace(torch.empty(ops.WORKSPACE_BYTES // 4, dtype=torch.uint8, device=cuda)):
        for repeats in (1, 9):                      # 9 x 14 = 126 recorded reductions: two batched launches
            want = run(None, repeats)
            for arena_bytes in (ops.DEFER_ARENA_BYTES, 5 << 20):
                got = run(torch.empty(arena_bytes, dtype=torch.uint8, device=cuda), repeats)
                for k in want:
                    assert torch.equal(want[k], got[k]), (k, repeats, arena_bytes)
        assert float(want["dgam"].abs().max()) > 1.0
    # a DIRECT reduction (ops.reduce_partials, as model.py uses for the shared-weight slabs) into an output that a RECORDED one
    # also targets must not overtake it — with a beta = 0 direct writer the recorded term would otherwise be added on top of the overwrite
    slabs = torch.randn(4, C, generator=g).to(cuda)
    def mixed(arena):
        acc = torch.full((C,), 3.0, device=cuda)
        with ops.reduce_defer(arena):
            ops.colsum(dys[0], acc, beta=1.0)            # recorded (deferred) when an arena is open
            ops.reduce_partials(slabs, acc, beta=0.0)    # direct: overwrites — must run AFTER the recorded column sum
            ops.colsum(dys[1], acc, beta=1.0)            # recorded again
        return acc
    with ops.use_workspace(torch.empty(ops.WORKSPACE_BYTES // 4, dtype=torch.uint8, device=cuda)):
        want = mixed(None)
        got = mixed(torch.empty(ops.DEFER_ARENA_BYTES, dtype=torch.uint8, device=cuda))
        assert torch.equal(want, got), "a direct reduction overtook a recorded one"
        # an item produced on ANOTHER stream does not join the batch (it reduces at once on its own stream, after what was recorded so far)
        side = torch.cuda.Stream()
        acc2 = torch.zeros(C, device=cuda); acc3 = torch.zeros(C, device=cuda)
        torch.cuda.synchronize()
        with ops.reduce_defer(torch.empty(ops.DEFER_ARENA_BYTES, dtype=torch.uint8, device=cuda)):
            ops.colsum(dys[0], acc2, beta=0.0)
            with torch.cuda.stream(side):
                ops.colsum(dys[1], acc3, beta=0.0)
            side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(acc2, ops.colsum(dys[0], torch.zeros(C, device=cuda), beta=0.0))
        assert torch.equal(acc3, ops.colsum(dys[1], torch.zeros(C, device=cuda), beta=0.0))
    # a context is per thread and not nestable; an exception inside drops it
    a = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    with pytest.raises(ops.DynError):
        with ops.reduce_defer(a):
            with ops.reduce_defer(a):
                pass
    with ops.reduce_defer(a):
        pass
