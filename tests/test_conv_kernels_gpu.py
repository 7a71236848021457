"""Float64 parity of the conformer encoder's own convolution kernels (csrc/conv.hip, csrc/convmod.hip) on every dispatch path: each C-ABI
entry against tests/kernel_refs.py (float64 restatements by index gathers, held to torch's ops and autograd in tests/test_kernel_refs_cpu.py),
at the smallest shapes that reach each template instance, tile edge, channel block, grid cap, `per` loop and fallback.

Tolerances are the project's (see tests/test_kernel_parity_f64_gpu.py): 2e-5 for a convolution forward / dgrad, kernel_refs.wgrad_tol(3e-4,
rows, 400) for tap and bias gradients summing `rows` terms, 5e-6 for norm statistics (rstd relative), 1e-6 elementwise (the GLU output).
The conv-module outputs behind the norm (nn, s) are the conv output times rstd * gamma = O(1) on these inputs: the convolution forward's
2e-5.  Where the inputs make a fixed floor meaningless (the conv module with a channel offset, sums deeper than 8192 rows, the fused
subsampling backward whose terms are products of two convolutions) the bound is MEASURED: 4 x the error of torch's fp32 CPU result of the
same op on the same inputs against float64, plus that floor (kernel_refs.measured_tol).  The kernel under test is never the yardstick.
Outputs start as NaN (beta = 0 accumulators too: a kernel that reads them fails).  Every check prints
`name: kernel error | torch fp32 error | bound` before it asserts (pytest -s shows them; profiles/conv_kernels_parity.txt is one run).

Before convmod_fwd_kernel's LayerNorm branch centred its variance (E[x^2] - mean^2 from single-pass fp32 sums) the offset cases of
test_convmod_with_a_channel_offset failed on rstd, nn and s for LayerNorm at every m >= 30, at both widths: rstd off by 6.6e-5 / 8.5e-4 /
8.0e-2 relative at m = 30 / 100 / 1000 (C = 256; bounds 5.7e-6 / 7.5e-6 / 2.6e-5), s by 3.3e-4 / 5.2e-3 / 5.3e-1; centred: 1.2e-7 / 3.2e-7 /
2.7e-6 at C = 1024, level with torch's fp32.  Both tables: profiles/conv_kernels_parity.txt.

What the cases catch, from scratch builds that only skip work (each run against this file on the MI355X):
  the `c0 += 256` / `cb += 256` channel loops ended after one pass   test_subsampling_channel_blocks[260], test_subsampling_alignment_fallback[260]
                                                                     (its v4 side), test_sub12_second_channel_pass
  the 2-D `per` loops run for their first row only                   test_subsampling_wgrad_with_two_rows_per_tile[4], [6], test_sub12_bwd_with_three_rows_per_tile
  the 1-D wgrad's row loop capped at 8 steps                         test_dwconv1d_wgrad_tiles at T = 16385 and 16400, both widths
  b / ngroups for b % ngroups                                        test_dwconv1d_lockstep_groups[4-2], [6-3], test_convmod_lockstep_group[rms], [ln]
  conv2d_first_dgrad's element loop ended after one pass             test_conv2d_first_dgrad_past_the_grid_cap
  FLIP dropped                                                       every T > 1 case of test_dwconv1d_every_width (18), test_dwconv1d_lockstep_groups[4-2], [6-3]"""
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

NAN = float("nan")
SENTINEL = -7777.25
KWS = (3, 5, 7, 9, 15, 31)
GRID_T, GRID_F = (1, 2, 3, 4, 5, 8), (1, 2, 3, 4, 7)


def _check(name, got, want, tol, t32=None, rel=False):
    err = K.max_err(got, want, rel)
    e32 = None if t32 is None else K.max_err(t32, want, rel)
    print(f"  {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")
    assert err <= tol, f"{name}: {'rel' if rel else 'abs'} err {err} > {tol} (torch fp32: {e32})"


def _measured(name, got, torch32, want, floor, rel=False):
    tol, _ = K.measured_tol(torch32, want, floor, rel)
    _check(name, got, want, tol, torch32, rel)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


def _cl(t):
    """torch's [B, C, T, F] -> channels-last [B, T, F, C]."""
    return t.detach().permute(0, 2, 3, 1).contiguous()


def _acc(old, beta, dev):
    """An accumulator holding `old` (beta != 0) or NaN (beta == 0: it must not be read)."""
    return old.to(dev) if beta != 0.0 else torch.full_like(old, NAN).to(dev)


def _plus(want, old, beta):
    return want + beta * old.to(want.dtype) if beta != 0.0 else want


# ----------------------------------------------------------------------------------------------------------- depthwise 1-D
def _dw1d_torch32(x, w, bias, dy):
    """torch's fp32 CPU depthwise conv1d and its autograd: y, dx, dw, dbias."""
    KW = w.shape[1]
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, bias))
    y = F.conv1d(xr.transpose(1, 2), wr.unsqueeze(1), br, padding=(KW - 1) // 2, groups=x.shape[2]).transpose(1, 2)
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad, br.grad


def _dw1d_inputs(B, T, C, KW, seed=0):
    g = K.gen(11000 + seed + 31 * T + 7 * C + KW)
    return (torch.randn(B, T, C, generator=g), torch.randn(C, KW, generator=g), torch.randn(C, generator=g), torch.randn(B, T, C, generator=g),
            torch.randn(C, KW, generator=g), torch.randn(C, generator=g), torch.randn(B, T, C, generator=g))


DW1D_CASES = ([(KW, T, C) for KW in KWS for (T, C) in ((1, 5), (33, 257), (65, 256))]          # T < P; two tiles + two channel blocks; a full third tile row
              + [(31, 15, 8), (31, 16, 8)]                                                      # the window is padding on both sides
              + [(9, 31, 8), (9, 32, 8), (9, 33, 1), (9, 33, 300)])                            # the tile edge; one channel; a ragged second channel block


@pytest.mark.parametrize("KW,T,C", DW1D_CASES, ids=lambda v: str(v))
def test_dwconv1d_every_width(cuda, KW, T, C):
    """dwconv1d_kernel<KW, FLIP> and dwconv1d_wgrad_kernel<KW> at all six widths, random asymmetric taps (a missed flip in dgrad shows)."""
    from dynamic_asr_eval_amd import ops
    B = 2
    x, w, bias, dy, old_w, old_b, old_x = _dw1d_inputs(B, T, C, KW)
    y32, dx32, dw32, db32 = _dw1d_torch32(x, w, bias, dy)
    x64, w64, b64, dy64 = x.double(), w.double(), bias.double(), dy.double()
    xd, wd, bd, dyd = (t.to(cuda) for t in (x, w, bias, dy))
    print(f"dwconv1d KW {KW} T {T} C {C}")
    _check("fwd", ops.dwconv1d(xd, wd, bd, out=_nan(B, T, C, dev=cuda)), K.dwconv1d_ref(x64, w64, b64), 2e-5, y32)
    _check("fwd (bias None)", ops.dwconv1d(xd, wd, None, out=_nan(B, T, C, dev=cuda)), K.dwconv1d_ref(x64, w64), 2e-5, y32 - bias)
    dx64 = K.dwconv1d_dgrad_ref(dy64, w64)
    for beta in (0.0, 0.5, 1.0):
        dx = ops.dwconv1d_dgrad(dyd, wd, out=_acc(old_x, beta, cuda), beta=beta)
        _check(f"dgrad (beta {beta:g})", dx, _plus(dx64, old_x, beta), 2e-5, _plus(dx32, old_x, beta))
    dw64, db64 = K.dwconv1d_wgrad_ref(x64, dy64, KW)
    tol = K.wgrad_tol(3e-4, B * T, 400)
    for beta in (0.0, 1.0):
        dw, db = _acc(old_w, beta, cuda), _acc(old_b, beta, cuda)
        ops.dwconv1d_wgrad(xd, dyd, dw, db, beta=beta)
        _check(f"wgrad (beta {beta:g})", dw, _plus(dw64, old_w, beta), tol, _plus(dw32, old_w, beta))
        _check(f"bgrad (beta {beta:g})", db, _plus(db64, old_b, beta), tol, _plus(db32, old_b, beta))
        dw2 = _acc(old_w, beta, cuda)
        ops.dwconv1d_wgrad(xd, dyd, dw2, None, beta=beta)
        assert _bits_equal(dw2, dw), "dbias = None must not change dw"


@pytest.mark.parametrize("KW", [3, 31])
@pytest.mark.parametrize("T", [7, 9, 16385, 16400])
def test_dwconv1d_wgrad_tiles(cuda, T, KW):
    """wgrad_tiles: 8 rows per tile up to T = 16384 (7: one ragged tile, 9: a second tile of one row), 9 rows past it (16385: 1821 tiles, the
    last of 5 rows; 16400: the last of 2), halos crossing every tile boundary.  Past 8192 rows the bound is measured."""
    from dynamic_asr_eval_amd import ops
    B, C = 1, 4
    x, w, bias, dy, old_w, old_b, _ = _dw1d_inputs(B, T, C, KW, seed=1)
    _, _, dw32, db32 = _dw1d_torch32(x, w, bias, dy)
    dw64, db64 = K.dwconv1d_wgrad_ref(x.double(), dy.double(), KW)
    floor = K.wgrad_tol(3e-4, B * T, 400)
    print(f"dwconv1d wgrad tiles KW {KW} T {T}")
    for beta in (0.0, 1.0):
        dw, db = _acc(old_w, beta, cuda), _acc(old_b, beta, cuda)
        ops.dwconv1d_wgrad(x.to(cuda), dy.to(cuda), dw, db, beta=beta)
        if T > 8192:
            _measured(f"wgrad (beta {beta:g})", dw, _plus(dw32, old_w, beta), _plus(dw64, old_w, beta), floor)
            _measured(f"bgrad (beta {beta:g})", db, _plus(db32, old_b, beta), _plus(db64, old_b, beta), floor)
        else:
            _check(f"wgrad (beta {beta:g})", dw, _plus(dw64, old_w, beta), floor, _plus(dw32, old_w, beta))
            _check(f"bgrad (beta {beta:g})", db, _plus(db64, old_b, beta), floor, _plus(db32, old_b, beta))


# ----------------------------------------------------------------------------------------------------------- lockstep groups
class _Flat:
    """Parameters carved from a flat [R, n] buffer as model.py carves them, n larger than what is carved: the gaps hold a sentinel."""

    def __init__(self, R, sizes, dev, gap=12):
        self.R, self.off, n = R, {}, gap
        for name, size in sizes.items():
            self.off[name] = (n, size)
            n += -(-size // 4) * 4 + gap
        self.n = n
        self.buf = torch.full((R, n), SENTINEL, device=dev)
        self.gap = torch.ones(n, dtype=torch.bool)
        for lo, size in self.off.values():
            self.gap[lo:lo + size] = False

    def view(self, name, *shape):
        lo, size = self.off[name]
        return self.buf[:, lo:lo + size].view(self.R, *shape)

    def param(self, name, *shape):
        from dynamic_asr_eval_amd import ops
        return ops.GroupParam(self.view(name, *shape), self.R, self.n)

    def gaps_untouched(self):
        return _bits_equal(self.buf[:, self.gap.to(self.buf.device)], torch.full((self.R, int(self.gap.sum())), SENTINEL))


@pytest.mark.parametrize("B,R", [(4, 2), (6, 3)])
def test_dwconv1d_lockstep_groups(cuda, B, R):
    """dyn_dwconv1d_dgrad_g / dyn_dwconv1d_wgrad_g through ops.GroupParam: sample b uses replica b % R at the flat buffer's stride, the
    weight gradient of replica r is beta * old + the sum over its samples (beta applied once), nothing outside the carved regions is written."""
    from dynamic_asr_eval_amd import ops
    T, C, KW = 33, 257, 9
    g = K.gen(12000 + B)
    dy, x = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    w, old_w, old_b, old_x = (torch.randn(s_, generator=g) for s_ in ((R, C, KW), (R, C, KW), (R, C), (B, T, C)))
    P = _Flat(R, {"w": C * KW, "b": C}, cuda)
    P.view("w", C, KW).copy_(w)
    print(f"dwconv1d groups B {B} R {R}")
    dx64 = K.dwconv1d_dgrad_group_ref(dy.double(), w.double())
    for beta in (0.0, 1.0):
        dx = ops.dwconv1d_dgrad(dy.to(cuda), P.param("w", C, KW), out=_acc(old_x, beta, cuda), beta=beta)
        _check(f"dgrad_g (beta {beta:g})", dx, _plus(dx64, old_x, beta), 2e-5)
    assert P.gaps_untouched() and _bits_equal(P.view("w", C, KW), w)
    tol = K.wgrad_tol(3e-4, (B // R) * T, 400)
    for beta in (0.0, 1.0):
        dw64, db64 = K.dwconv1d_wgrad_group_ref(x.double(), dy.double(), old_w.double(), old_b.double(), beta)
        for with_bias in (True, False):
            G = _Flat(R, {"w": C * KW, "b": C}, cuda)
            G.view("w", C, KW).copy_(_acc(old_w, beta, cuda))
            G.view("b", C).copy_(_acc(old_b, beta, cuda))
            before_b = G.view("b", C).clone()
            ops.dwconv1d_wgrad(x.to(cuda), dy.to(cuda), G.param("w", C, KW), G.view("b", C) if with_bias else None, beta=beta)
            _check(f"wgrad_g (beta {beta:g}, dbias {with_bias})", G.view("w", C, KW), dw64, tol)
            if with_bias:
                _check(f"bgrad_g (beta {beta:g})", G.view("b", C), db64, tol)
            else:
                assert _bits_equal(G.view("b", C), before_b), "dbias = None: the bias gradient must not be written"
            assert G.gaps_untouched(), "the gaps between the carved gradients must keep their sentinel, bit for bit"


def test_one_replica_group_entries_equal_the_plain_entries(cuda):
    """n_groups = 1 through the _g entries: the same bits as the plain entries."""
    from dynamic_asr_eval_amd import ops
    B, T, C, KW = 2, 33, 257, 9
    x, w, bias, dy, old_w, old_b, old_x = (t.to(cuda) for t in _dw1d_inputs(B, T, C, KW, seed=2))
    gp = lambda t: ops.GroupParam(t.view(1, *t.shape), 1, t.numel() + 40)                         # noqa: E731
    assert _bits_equal(ops.dwconv1d_dgrad(dy, gp(w), out=old_x.clone(), beta=0.5), ops.dwconv1d_dgrad(dy, w, out=old_x.clone(), beta=0.5))
    for beta in (0.0, 1.0):
        dw_g, db_g, dw_p, db_p = old_w.clone(), old_b.clone(), old_w.clone(), old_b.clone()
        ops.dwconv1d_wgrad(x, dy, gp(dw_g), db_g, beta=beta)
        ops.dwconv1d_wgrad(x, dy, dw_p, db_p, beta=beta)
        assert _bits_equal(dw_g, dw_p) and _bits_equal(db_g, db_p), f"wgrad_g beta {beta}"
    Cm = 256
    g = K.gen(12100)
    u, wm, bm, gm, tm = (torch.randn(s_, generator=g).to(cuda) for s_ in ((B, 5, 2 * Cm), (Cm, 9), (Cm,), (Cm,), (Cm,)))
    for ln in (False, True):
        got = ops.convmod_fwd(u, gp(wm), bm, gm, tm if ln else None, ln, 1e-5, True)
        want = ops.convmod_fwd(u, wm, bm, gm, tm if ln else None, ln, 1e-5, True)
        assert all(a is None and b is None or _bits_equal(a, b) for a, b in zip(got, want)), f"convmod_fwd_g layernorm {ln}"


# ----------------------------------------------------------------------------------------------------------- 2-D subsampling
def _sub_inputs(B, T, Fq, C, seed=0):
    """x [B, T, F], z [B, T, F, C] (the depthwise conv's input), both filters and biases, and output gradients for both."""
    g = K.gen(13000 + seed + 101 * T + 13 * Fq + C)
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    return dict(x=torch.randn(B, T, Fq, generator=g), z=torch.randn(B, T, Fq, C, generator=g) * 2,
                w1=torch.randn(C, 3, 3, generator=g) * 0.3, b1=torch.randn(C, generator=g), w2=torch.randn(C, 3, 3, generator=g) * 0.3,
                b2=torch.randn(C, generator=g), dz=torch.randn(B, To, Fo, C, generator=g), du=torch.randn(B, To, Fo, C, generator=g),
                old_w=torch.randn(C, 3, 3, generator=g), old_b=torch.randn(C, generator=g))


def _sub_torch32(i):
    """torch's fp32 CPU results of the five operations on the inputs of _sub_inputs."""
    C = i["w1"].shape[0]
    w1r, b1r = i["w1"].clone().requires_grad_(), i["b1"].clone().requires_grad_()
    z = F.conv2d(i["x"].unsqueeze(1), w1r.unsqueeze(1), b1r, stride=2, padding=1)
    z.backward(i["dz"].permute(0, 3, 1, 2))
    zr, w2r, b2r = i["z"].permute(0, 3, 1, 2).clone().requires_grad_(), i["w2"].clone().requires_grad_(), i["b2"].clone().requires_grad_()
    u = F.conv2d(F.silu(zr), w2r.unsqueeze(1), b2r, stride=2, padding=1, groups=C)
    u.backward(i["du"].permute(0, 3, 1, 2))
    return dict(z=_cl(z), dw1=w1r.grad, db1=b1r.grad, u=_cl(u), dzin=_cl(zr.grad), dw2=w2r.grad, db2=b2r.grad)


def _sub_case(cuda, B, T, Fq, C, measured=False, seed=0):
    """conv2d_first fwd / wgrad and dwconv2d_s2 fwd / dgrad / wgrad through ops (16-byte aligned tensors: the v4 kernels when C % 4 == 0,
    the scalar ones otherwise) against float64."""
    from dynamic_asr_eval_amd import ops
    i = _sub_inputs(B, T, Fq, C, seed)
    t32 = _sub_torch32(i)
    d, i64 = {k: v.to(cuda) for k, v in i.items()}, {k: v.double() for k, v in i.items()}
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    floor = K.wgrad_tol(3e-4, B * To * Fo, 400)
    print(f"subsampling B {B} T {T} F {Fq} C {C}")
    _check("conv2d_first fwd", ops.conv2d_first(d["x"], d["w1"], d["b1"], out=_nan(B, To, Fo, C, dev=cuda)),
           K.conv2d_first_ref(i64["x"], i64["w1"], i64["b1"]), 2e-5, t32["z"])
    _check("dwconv2d_s2 fwd", ops.dwconv2d_s2(d["z"], d["w2"], d["b2"], out=_nan(B, To, Fo, C, dev=cuda)),
           K.dwconv2d_s2_ref(i64["z"], i64["w2"], i64["b2"]), 2e-5, t32["u"])
    _check("dwconv2d_s2 dgrad", ops.dwconv2d_s2_dgrad(d["z"], d["w2"], d["du"], out=_nan(B, T, Fq, C, dev=cuda)),
           K.dwconv2d_s2_dgrad_ref(i64["z"], i64["w2"], i64["du"]), 2e-5, t32["dzin"])
    wants = {"conv2d_first": K.conv2d_first_wgrad_ref(i64["x"], i64["dz"]), "dwconv2d_s2": K.dwconv2d_s2_wgrad_ref(i64["z"], i64["du"])}
    for beta in (0.0, 1.0):
        for name, fn, a, b, k32 in (("conv2d_first", ops.conv2d_first_wgrad, "x", "dz", ("dw1", "db1")),
                                    ("dwconv2d_s2", ops.dwconv2d_s2_wgrad, "z", "du", ("dw2", "db2"))):
            dw, db = _acc(i["old_w"], beta, cuda), _acc(i["old_b"], beta, cuda)
            fn(d[a], d[b], dw, db, beta=beta)
            for what, got, want, old, t in (("wgrad", dw, wants[name][0], i["old_w"], t32[k32[0]]), ("bgrad", db, wants[name][1], i["old_b"], t32[k32[1]])):
                if measured:
                    _measured(f"{name} {what} (beta {beta:g})", got, _plus(t, old, beta), _plus(want, old, beta), floor)
                else:
                    _check(f"{name} {what} (beta {beta:g})", got, _plus(want, old, beta), floor, _plus(t, old, beta))


@pytest.mark.parametrize("B", [1, 3])
def test_subsampling_parity_grid(cuda, B):
    """T x F over every parity and the one-row / one-column inputs at C = 4 (one lane of a wave live).  B * To runs through 1, 2,
    3, 4 (B = 1) and 3, 6, 9, 12 (B = 3): the four waves of the last workgroup are partly live; (B, T) = (1, 9) adds five rows."""
    for T in GRID_T + ((9,) if B == 1 else ()):
        for Fq in GRID_F:
            _sub_case(cuda, B, T, Fq, 4)


@pytest.mark.parametrize("C", [6, 256, 258, 260])
def test_subsampling_channel_blocks(cuda, C):
    """6 and 258: the scalar kernels (258: their second blockIdx.y channel block, two channels live); 256 and 260: the v4 kernels (260: the
    channel loop's second pass with one lane live)."""
    _sub_case(cuda, 2, 5, 7, C)


@pytest.mark.parametrize("C", [4, 6])
def test_subsampling_wgrad_with_two_rows_per_tile(cuda, C):
    """T = 8195: To = 4098 > 4096 tiles per sample, so per = 2 and 2049 tiles (tiles % 4 = 1: one live wave in the last workgroup of the v4
    kernel, C = 4; the scalar kernels' to_per_block = 2, C = 6).  8196 summed terms per tap: measured bounds."""
    _sub_case(cuda, 1, 8195, 3, C, measured=True)


def _offset_copy(t, dev):
    """A copy of `t` one float into a larger buffer: 4 bytes past a 16-byte boundary."""
    buf = torch.full((t.numel() + 8,), NAN, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("C", [8, 260])
def test_subsampling_alignment_fallback(cuda, C):
    """C % 4 == 0 but no pointer 16-byte aligned: the C-ABI takes the scalar kernels.  Their forwards accumulate in the v4 kernels' order
    (bias first, taps dt-major), so they equal the v4 results bit for bit; dgrad and wgrad sum in another order and are held to float64."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    L = load()
    B, T, Fq = 2, 5, 7
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    i = _sub_inputs(B, T, Fq, C, seed=3)
    i64 = {k: v.double() for k, v in i.items()}
    d = {k: v.to(cuda) for k, v in i.items()}
    o = {k: _offset_copy(v, cuda) for k, v in i.items()}
    ws = ops.workspace(cuda)
    print(f"subsampling, misaligned pointers, C {C}")
    z = _offset_copy(_nan(B, To, Fo, C, dev=cuda), cuda)
    check(L.dyn_conv2d_first_fwd(o["x"].data_ptr(), o["w1"].data_ptr(), o["b1"].data_ptr(), z.data_ptr(), B, T, Fq, C, _stream()), "conv2d_first_fwd")
    assert _bits_equal(z, ops.conv2d_first(d["x"], d["w1"], d["b1"])), "scalar conv2d_first forward != v4, bit for bit"
    u = _offset_copy(_nan(B, To, Fo, C, dev=cuda), cuda)
    check(L.dyn_dwconv2d_s2_fwd(o["z"].data_ptr(), o["w2"].data_ptr(), o["b2"].data_ptr(), u.data_ptr(), B, T, Fq, C, _stream()), "dwconv2d_s2_fwd")
    assert _bits_equal(u, ops.dwconv2d_s2(d["z"], d["w2"], d["b2"])), "scalar dwconv2d_s2 forward != v4, bit for bit"
    dzin = _offset_copy(_nan(B, T, Fq, C, dev=cuda), cuda)
    check(L.dyn_dwconv2d_s2_dgrad(o["z"].data_ptr(), o["w2"].data_ptr(), o["du"].data_ptr(), dzin.data_ptr(), B, T, Fq, C, _stream()), "dwconv2d_s2_dgrad")
    _check("dwconv2d_s2 dgrad (scalar)", dzin, K.dwconv2d_s2_dgrad_ref(i64["z"], i64["w2"], i64["du"]), 2e-5)
    tol = K.wgrad_tol(3e-4, B * To * Fo, 400)
    for beta in (0.0, 1.0):
        for name, fn, a, b, want in (("conv2d_first", L.dyn_conv2d_first_wgrad, "x", "dz", K.conv2d_first_wgrad_ref(i64["x"], i64["dz"])),
                                     ("dwconv2d_s2", L.dyn_dwconv2d_s2_wgrad, "z", "du", K.dwconv2d_s2_wgrad_ref(i64["z"], i64["du"]))):
            dw, db = _offset_copy(_acc(i["old_w"], beta, cuda), cuda), _offset_copy(_acc(i["old_b"], beta, cuda), cuda)
            check(fn(o[a].data_ptr(), o[b].data_ptr(), dw.data_ptr(), db.data_ptr(), beta, B, T, Fq, C, ws.data_ptr(), ws.numel(), _stream()), name)
            _check(f"{name} wgrad (scalar, beta {beta:g})", dw, _plus(want[0], i["old_w"], beta), tol)
            _check(f"{name} bgrad (scalar, beta {beta:g})", db, _plus(want[1], i["old_b"], beta), tol)


# ----------------------------------------------------------------------------------------------------------- conv2d_first_dgrad
def _first_dgrad_case(cuda, B, T, Fq, C):
    from dynamic_asr_eval_amd._lib import check, load
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    g = K.gen(14000 + 101 * T + 13 * Fq + C)
    dz, w = torch.randn(B, To, Fo, C, generator=g), torch.randn(C, 3, 3, generator=g) * 0.3
    xr = torch.zeros(B, 1, T, Fq, requires_grad=True)
    F.conv2d(xr, w.unsqueeze(1), None, stride=2, padding=1).backward(dz.permute(0, 3, 1, 2))
    dx = _nan(B, T, Fq, dev=cuda)
    dzd, wd = dz.to(cuda), w.to(cuda)
    check(load().dyn_conv2d_first_dgrad(dzd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, T, Fq, C, _stream()), "dyn_conv2d_first_dgrad")
    _check(f"conv2d_first dgrad B {B} T {T} F {Fq} C {C}", dx, K.conv2d_first_dgrad_ref(dz.double(), w.double(), T, Fq), 2e-5, xr.grad[:, 0])


@pytest.mark.parametrize("C", [1, 63, 64, 65, 300])
def test_conv2d_first_dgrad(cuda, C):
    """One wave per input element, lanes striding the channels: one lane live, one short of a wave, a wave, the `c += 64` loop's second
    pass with one lane (65) and its fifth with 44 (300); every parity of T and F."""
    for T in GRID_T:
        for Fq in GRID_F:
            _first_dgrad_case(cuda, 2, T, Fq, C)


def test_conv2d_first_dgrad_past_the_grid_cap(cuda):
    """264000 outputs > 4 x 65536: the element stride loop's second pass."""
    _first_dgrad_case(cuda, 1, 3300, 80, 4)


# ----------------------------------------------------------------------------------------------------------- fused first two stages
def _sub12_case(cuda, B, T, Fq, C):
    from dynamic_asr_eval_amd import ops
    g = K.gen(15000 + 101 * T + 13 * Fq + C)
    x = torch.randn(B, T, Fq, generator=g)
    w1, b1 = torch.randn(C, 3, 3, generator=g) * 0.5, torch.randn(C, generator=g) * 0.3
    w2, b2 = torch.randn(C, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.3
    w1r, b1r, w2r, b2r = (t.clone().requires_grad_() for t in (w1, b1, w2, b2))
    u32 = F.conv2d(F.silu(F.conv2d(x.unsqueeze(1), w1r.unsqueeze(1), b1r, stride=2, padding=1)), w2r.unsqueeze(1), b2r, stride=2, padding=1, groups=C)
    du = torch.randn(_cl(u32).shape, generator=g)
    u32.backward(du.permute(0, 3, 1, 2))
    olds = [torch.randn(s_, generator=g) for s_ in ((C, 3, 3), (C,), (C, 3, 3), (C,))]
    T1, F1 = K.s2_out_len(T), K.s2_out_len(Fq)
    T2, F2 = K.s2_out_len(T1), K.s2_out_len(F1)
    xd, w1d, b1d, w2d, b2d, dud = (t.to(cuda) for t in (x, w1, b1, w2, b2, du))
    print(f"sub12 B {B} T {T} F {Fq} C {C}")
    u = ops.sub12_fwd(xd, w1d, b1d, w2d, b2d, out=_nan(B, T2, F2, C, dev=cuda))
    _check("sub12 fwd", u, K.sub12_ref(x.double(), w1.double(), b1.double(), w2.double(), b2.double()), 2e-5, _cl(u32))
    assert _bits_equal(u, ops.dwconv2d_s2(ops.conv2d_first(xd, w1d, b1d), w2d, b2d)), "the fused forward must equal the two kernels bit for bit"
    wants = K.sub12_bwd_ref(x.double(), du.double(), w1.double(), b1.double(), w2.double())
    rows = (B * T1 * F1, B * T1 * F1, B * T2 * F2, B * T2 * F2)
    for beta in (0.0, 2.0):
        accs = [_acc(o_, beta, cuda) for o_ in olds]
        ops.sub12_bwd(xd, dud, w1d, b1d, w2d, *accs, beta=beta)
        for name, got, want, t, old, n in zip(("dw1", "db1", "dw2", "db2"), accs, wants, (w1r.grad, b1r.grad, w2r.grad, b2r.grad), olds, rows):
            _measured(f"sub12 {name} (beta {beta:g})", got, _plus(t, old, beta), _plus(want, old, beta), K.wgrad_tol(3e-4, n, 400))


@pytest.mark.parametrize("T", [4, 5, 6, 7])
def test_sub12_every_residue(cuda, T):
    """T mod 4 and F mod 4 over {0, 1, 2, 3}: every combination of a padded z1 row / column and a padded x row / column behind it."""
    for Fq in (8, 9, 10, 11):
        _sub12_case(cuda, 2, T, Fq, 8)


def test_sub12_second_channel_pass(cuda):
    """C = 260: the `c0 += 256` / `cb += 256` loops' second pass with one lane live."""
    _sub12_case(cuda, 2, 5, 9, 260)


def test_sub12_bwd_with_three_rows_per_tile(cuda):
    """T = 16389: T1 = 8195 > 4096 tiles per sample, per = 3, 2732 tiles, the last of 2 rows."""
    _sub12_case(cuda, 1, 16389, 5, 8)


# ----------------------------------------------------------------------------------------------------------- fused conv module
def _convmod_inputs(B, T, C, seed=0, R=None):
    g = K.gen(16000 + seed + 17 * T + C)
    lead = () if R is None else (R,)
    u = torch.randn(B, T, 2 * C, generator=g)
    w, bias = torch.randn(*lead, C, 9, generator=g) * 0.3, torch.randn(*lead, C, generator=g) * 0.3
    gamma, beta = torch.randn(*lead, C, generator=g) * 0.5 + 1.0, torch.randn(*lead, C, generator=g)
    return u, w, bias, gamma, beta


def _convmod_torch32(u, w, bias, gamma, beta, layernorm, eps):
    """torch's fp32 CPU GLU -> conv1d -> layer_norm / RMS -> SiLU: the same tuple as kernel_refs.convmod_ref."""
    B, T, C2 = u.shape
    C = C2 // 2
    g = F.glu(u, -1)
    c = F.conv1d(g.transpose(1, 2), w.unsqueeze(1), bias, padding=4, groups=C).transpose(1, 2).contiguous()
    if layernorm:
        nn = F.layer_norm(c, (C,), gamma, beta, eps)
        mean, rstd = c.mean(-1).reshape(-1), torch.rsqrt(c.var(-1, unbiased=False) + eps).reshape(-1)
    else:
        rstd = torch.rsqrt(c.pow(2).mean(-1) + eps).reshape(-1)
        nn, mean = c * rstd.view(B, T, 1) * gamma, None
    return F.silu(nn), g, c, nn, mean, rstd


CONVMOD_FLOORS = (("s", 2e-5, False), ("g", 1e-6, False), ("c", 2e-5, False), ("nn", 2e-5, False), ("mean", 5e-6, False), ("rstd (rel)", 5e-6, True))


def _convmod_compare(got, want, t32, measured):
    """All six outputs are printed before the first miss is raised: a wrong rstd shows next to the s and nn it spoils."""
    missed = []
    for (name, floor, rel), a, b, t in zip(CONVMOD_FLOORS, got, want, t32):
        if b is None:
            assert a is None, name
            continue
        try:
            if measured:
                _measured(name, a, t, b, floor, rel)
            else:
                _check(name, a, b, floor, t, rel)
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, "; ".join(missed)


def _convmod_case(cuda, B, T, C, layernorm, bias, beta, seed=0):
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    eps = 1e-5
    u, w, bs, gamma, bt = _convmod_inputs(B, T, C, seed)
    bs, bt = bs if bias else None, bt if (beta and layernorm) else None
    dd = lambda t: None if t is None else t.double()                                               # noqa: E731
    dv = lambda t: None if t is None else t.to(cuda)                                               # noqa: E731
    want = K.convmod_ref(dd(u), dd(w), dd(bs), dd(gamma), dd(bt), layernorm, eps)
    t32 = _convmod_torch32(u, w, bs, gamma, bt, layernorm, eps)
    print(f"convmod B {B} T {T} C {C} {'LayerNorm' if layernorm else 'RMSNorm'} bias {bias} beta {bt is not None}")
    outs = [_nan(B, T, C, dev=cuda) for _ in range(4)] + [_nan(B * T, dev=cuda), _nan(B * T, dev=cuda)]        # s, g, c, nn, mean, rstd
    ud, wd, bd, gd, td = dv(u), dv(w), dv(bs), dv(gamma), dv(bt)
    p = lambda t: None if t is None else t.data_ptr()                                             # noqa: E731
    check(load().dyn_convmod_fwd(ud.data_ptr(), wd.data_ptr(), p(bd), gd.data_ptr(), p(td), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                 outs[3].data_ptr(), outs[4].data_ptr() if layernorm else None, outs[5].data_ptr(), B, T, C, 9, int(layernorm), eps,
                                 _stream()), "dyn_convmod_fwd")
    got = outs[:4] + [outs[4] if layernorm else None, outs[5]]
    _convmod_compare(got, want, t32, False)
    if not layernorm:
        assert torch.isnan(outs[4]).all(), "RMSNorm must not write mean_out"
    s_only = ops.convmod_fwd(ud, wd, bd, gd, td, layernorm, eps, False)
    assert s_only[1:] == (None,) * 5 and _bits_equal(s_only[0], got[0]), "save = False must give the same s, bit for bit"
    saved = ops.convmod_fwd(ud, wd, bd, gd, td, layernorm, eps, True)
    assert all(a is None and b is None or _bits_equal(a, b) for a, b in zip(saved, got)), "the wrapper's saved outputs"


@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("C", [256, 512, 768, 1024])
def test_convmod_every_instance(cuda, C, layernorm):
    """convmod_fwd_kernel<NV, LAYERNORM>, all eight: T = 1 (a tile of one frame, the window all halo) and 13 (four tiles, the last of one
    frame) at every instance; 3, 4, 5, 9 (the 4-frame tile's edges, T < P and T = 2 P + 1) at C = 256.  All six outputs, save on and off,
    NULL bias, NULL beta."""
    for T in (1, 13) + ((3, 4, 5, 9) if C == 256 else ()):
        _convmod_case(cuda, 2, T, C, layernorm, True, True, seed=T)
    _convmod_case(cuda, 2, 13, C, layernorm, False, False, seed=77)


@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
def test_convmod_lockstep_group(cuda, layernorm):
    """dyn_convmod_fwd_g at (B, R) = (4, 2): filters, bias, gamma and beta of replica b % R, carved from one flat buffer with a padded stride."""
    from dynamic_asr_eval_amd import ops
    B, R, T, C, eps = 4, 2, 5, 256, 1e-5
    u, w, bias, gamma, beta = _convmod_inputs(B, T, C, seed=5, R=R)
    P = _Flat(R, {"w": C * 9, "bias": C, "gamma": C, "beta": C}, cuda)
    for name, t in (("w", w), ("bias", bias), ("gamma", gamma), ("beta", beta)):
        P.view(name, *t.shape[1:]).copy_(t)
    want = K.convmod_group_ref(u.double(), w.double(), bias.double(), gamma.double(), beta.double() if layernorm else None, layernorm, eps)
    print(f"convmod group B {B} R {R} {'LayerNorm' if layernorm else 'RMSNorm'}")
    got = ops.convmod_fwd(u.to(cuda), P.param("w", C, 9), P.view("bias", C), P.view("gamma", C), P.view("beta", C) if layernorm else None,
                          layernorm, eps, True)
    _convmod_compare(got, want, (None,) * 6, False)
    assert P.gaps_untouched()


@pytest.mark.parametrize("m", (0.0,) + K.COLNORM_RATIOS, ids=lambda m: f"m{m:g}")
@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("C", [256, 1024])
def test_convmod_with_a_channel_offset(cuda, C, layernorm, m):
    """A conv bias with a component m common to the channels, m / std in {0, 30, 100, 1000}: the filters are scaled so that the float64 conv
    output has unit spread over the channels (the mean over the frames; see the assertion below), the bias is m + 0.1 N(0, 1).  LayerNorm must centre before it squares:
    E[x^2] - mean^2 from fp32 sums is off by 1e-4 relative in rstd at m = 30 and by 1e-1 at m = 1000.  Bounds measured against torch's fp32."""
    from dynamic_asr_eval_amd import ops
    B, T, eps = 2, 9, 1e-5
    u, w, _, gamma, beta = _convmod_inputs(B, T, C, seed=9)
    g = K.gen(16500 + C)
    c0 = K.convmod_ref(u.double(), w.double(), None, gamma.double(), None, False, eps)[2]
    w = (w.double() / c0.std(-1, unbiased=False).mean()).float()
    spread = K.convmod_ref(u.double(), w.double(), None, gamma.double(), None, False, eps)[2].std(-1, unbiased=False)
    # the mean over the 2 x 9 frames is 1 by construction; single frames lie between 0.79 (the first and last see five of the nine taps)
    # and 1.19 (the middle one sees all nine), so m / std of a frame is m to within a quarter
    assert abs(spread.mean().item() - 1.0) <= 0.2 and 0.75 <= spread.min().item() and spread.max().item() <= 1.25, spread
    bias = (m + 0.1 * torch.randn(C, generator=g)).float()
    bt = beta if layernorm else None
    want = K.convmod_ref(u.double(), w.double(), bias.double(), gamma.double(), None if bt is None else bt.double(), layernorm, eps)
    t32 = _convmod_torch32(u, w, bias, gamma, bt, layernorm, eps)
    print(f"convmod offset m {m:g} C {C} {'LayerNorm' if layernorm else 'RMSNorm'}")
    got = ops.convmod_fwd(u.to(cuda), w.to(cuda), bias.to(cuda), gamma.to(cuda), None if bt is None else bt.to(cuda), layernorm, eps, True)
    _convmod_compare(got, want, t32, True)
