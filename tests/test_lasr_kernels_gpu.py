"""The 32-tap instances LASR (MedASR) adds to csrc/convmod_bn.hip (dyn_convmod_bn_fwd, dyn_glu_dwconv1d_dgrad; dyn_convmod_bn_bwd_act is
tap-independent) and the 32-tap dyn_dwconv1d_wgrad of csrc/conv.hip, against float64 restatements whose depthwise step is torch's own
`conv1d(padding="same")` (tests/lasr_refs.py): an even kernel pads 15 frames left and 16 right, its data gradient reaches 16 back and 15
ahead.  Bars: kernel_refs.measured_tol (4 x torch's own fp32 CPU error against float64 + 2e-6) for activations and data gradients,
kernel_refs.wgrad_tol for column sums (5e-4 at 531 rows) and conv taps (3e-4 at 400 rows)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import lasr_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

KW, EPS, SENTINEL, NAN, B = 32, 1e-5, -7777.25, float("nan"), 2


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guarded(B, T, C, dev):
    """A [B, T, C] view at the head of a buffer that holds two more rows of SENTINEL: (view, the guard rows)."""
    buf = torch.full(((B * T + 2) * C,), SENTINEL, device=dev)
    return buf[:B * T * C].view(B, T, C), buf[B * T * C:]


def _report(name, got, t32, want, floor, worst):
    tol, e32 = K.measured_tol(t32, want, floor)
    err = K.max_err(got, want)
    worst[name] = max(worst.get(name, (0, 0, 0)), (err, e32, tol))
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _inputs(T, C, seed):
    g = K.gen(41000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return dict(u=r(B, T, 2 * C), w=r(C, KW) * 0.2, cbias=r(C) * 0.2, mean=r(C) * 0.1, var=0.5 + torch.rand(C, generator=g), weight=1 + 0.1 * r(C),
                bias=r(C) * 0.1, c=r(B, T, C), ds=r(B, T, C), dc=r(B, T, C), old=[r(C) for _ in range(3)], old_w=r(C, KW))


@pytest.mark.parametrize("C", [256, 512])
def test_convmod_bn_32_taps_against_float64(cuda, C):
    """Forward (s, gl, c), activation / BatchNorm backward, fused GLU + depthwise data gradient and the 32-tap weight gradient at B = 2 and
    T = 1, 15, 16, 17 (around the two halos), 31, 32, 33 (around KW and the 32-frame time tile), 65 (a third tile of one frame); C = 512 is a
    second channel block; valid = null, 0, 1, T - 1, T; with and without the convolution bias.  Rows >= valid are exact zeros, the two guard
    rows behind every output keep their sentinel, a second run gives equal bits.
    Worst measured kernel | torch fp32 | bound over the whole grid (MI355X):
      C 256: s 9.8e-07 | 9.8e-07 | 5.9e-06   gl 2.8e-07 | 2.8e-07 | 3.1e-06   c 7.0e-07 | 5.5e-07 | 4.2e-06   dc 1.0e-06 | 6.6e-07 | 4.7e-06
             du 1.3e-06 | 5.8e-07 | 4.3e-06   dweight 4.5e-06, dbias 3.6e-06, dcbias 4.2e-06 | bound 5.0e-04   dw 7.3e-06 | bound 3.0e-04
      C 512: s 1.2e-06 | 1.2e-06 | 6.8e-06   gl 2.9e-07 | 2.4e-07 | 3.0e-06   c 6.5e-07 | 5.6e-07 | 4.3e-06   dc 1.3e-06 | 8.1e-07 | 5.2e-06
             du 8.6e-07 | 6.3e-07 | 4.5e-06   dweight 6.7e-06, dbias 3.8e-06, dcbias 4.6e-06 | bound 5.0e-04   dw 7.5e-06 | bound 3.0e-04"""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    tile = ops.convmod_bn_time_tile(KW)
    assert ops.convmod_bn_time_tile() == 16                       # the 9-tap path's tile is what it was
    worst = {}
    for T in sorted({1, 15, 16, 17, 31, 32, 33, tile - 1, tile + 1, 2 * tile + 1}):
        i = _inputs(T, C, 7 * T + C)
        i64 = {k: v.double() for k, v in i.items() if k != "old"}
        d = {k: v.to(cuda) for k, v in i.items() if k != "old"}
        for valid in [None] + sorted({0, 1, T - 1, T}):
            vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
            v = T if valid is None else valid
            bn = lambda t: (t["mean"], t["var"], t["weight"], t["bias"])                         # noqa: E731
            for has_cb in (True, False):
                cb = lambda t: t["cbias"] if has_cb else None                                    # noqa: E731
                # ---------------- forward
                want = R.convmod_bn_ref(i64["u"], i64["w"], cb(i64), *bn(i64), EPS, valid)
                t32 = R.convmod_bn_ref(i["u"], i["w"], cb(i), *bn(i), EPS, valid)
                runs = []
                for _ in range(2):
                    outs = [_guarded(B, T, C, cuda) for _ in range(3)]
                    check(load().dyn_convmod_bn_fwd(d["u"].data_ptr(), d["w"].data_ptr(), d["cbias"].data_ptr() if has_cb else None,
                                                    d["mean"].data_ptr(), d["var"].data_ptr(), d["weight"].data_ptr(), d["bias"].data_ptr(),
                                                    outs[0][0].data_ptr(), outs[1][0].data_ptr(), outs[2][0].data_ptr(),
                                                    None if vd is None else vd.data_ptr(), B, T, C, KW, 0, EPS,
                                                    torch.cuda.current_stream().cuda_stream), "fwd")
                    for o, guard in outs:
                        assert (guard == SENTINEL).all(), (T, valid)
                        assert v >= T or o[:, v:].abs().max().item() == 0.0, (T, valid)
                    runs.append([o for o, _ in outs])
                for a, c_ in zip(*runs):
                    assert _bits_equal(a, c_), ("two runs differ", T, valid)
                for name, got, t, w64 in zip(("s", "gl", "c"), runs[0], t32, want):
                    _report(name, got, t, w64, 2e-6, worst)
                s, gl, cv = ops.convmod_bn(d["u"], d["w"], cb(d), *bn(d), "silu", EPS, valid=vd, save=True)
                assert _bits_equal(s, runs[0][0]) and _bits_equal(gl, runs[0][1]) and _bits_equal(cv, runs[0][2])
            # ---------------- activation / BatchNorm backward (the tap-independent kernel, at these shapes)
            want = R.convmod_bn_bwd_act_ref(i64["c"], *bn(i64), i64["ds"], EPS, valid)
            t32 = R.convmod_bn_bwd_act_ref(i["c"], *bn(i), i["ds"], EPS, valid)
            sums_tol = K.wgrad_tol(5e-4, B * T, 531)
            runs = []
            for _ in range(2):
                acc = [o.to(cuda) for o in i["old"]]
                dc, guard = _guarded(B, T, C, cuda)
                assert ops.convmod_bn_bwd_act(d["c"], *bn(d), d["ds"], *acc, "silu", EPS, valid=vd, out=dc) is dc and (guard == SENTINEL).all()
                assert v >= T or dc[:, v:].abs().max().item() == 0.0
                runs.append([dc] + acc)
            assert all(_bits_equal(a, c_) for a, c_ in zip(*runs))
            _report("dc", runs[0][0], t32[0], want[0], 2e-6, worst)
            for k, name in enumerate(("dweight", "dbias", "dcbias")):
                err = K.max_err(runs[0][1 + k], want[1 + k] + i["old"][k].double())
                worst[name] = max(worst.get(name, (0, 0, 0)), (err, 0.0, sums_tol))
                assert err <= sums_tol, (name, err, sums_tol, T, valid)
            # ---------------- GLU' x depthwise data gradient
            want = R.glu_dwconv1d_dgrad_ref(i64["u"], i64["w"], i64["dc"], valid)
            t32 = R.glu_dwconv1d_dgrad_ref(i["u"], i["w"], i["dc"], valid)
            first = None
            for _ in range(2):
                du, guard = _guarded(B, T, 2 * C, cuda)
                assert ops.glu_dwconv1d_dgrad(d["u"], d["w"], d["dc"], valid=vd, out=du) is du and (guard == SENTINEL).all()
                assert v >= T or du[:, v:].abs().max().item() == 0.0
                first = du if first is None else first
                assert _bits_equal(du, first)
            _report("du", first, t32, want, 2e-6, worst)
        # ---------------- 32-tap weight gradient: dw[c, j] = sum_t dc[t] gl[t + j - 15] (valid does not reach it: gl and dc carry their zero rows)
        want = R.dwconv1d_wgrad_ref(i64["c"], i64["dc"])
        taps_tol = K.wgrad_tol(3e-4, B * T, 400)
        for beta in (0.0, 1.0):
            runs = []
            for _ in range(2):
                buf = torch.full(((C + 2) * KW,), SENTINEL, device=cuda)
                dw, guard = buf[:C * KW].view(C, KW), buf[C * KW:]
                dw.copy_(d["old_w"] if beta else torch.full_like(d["old_w"], NAN))
                ops.dwconv1d_wgrad(d["c"], d["dc"], dw, None, beta=beta)
                assert (guard == SENTINEL).all()
                runs.append(dw)
            assert _bits_equal(*runs)
            err = K.max_err(runs[0], want + beta * i64["old_w"])
            worst["dw"] = max(worst.get("dw", (0, 0, 0)), (err, 0.0, taps_tol))
            assert err <= taps_tol, ("dw", err, taps_tol, T, beta)
    for name, (err, e32, tol) in worst.items():
        print(f"  C {C} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")


@pytest.mark.parametrize("t0", [40, 3, 60])
def test_impulse_separates_left_from_right(cuda, t0):
    """T = 64, the GLU input zero except at frame t0, w[c, j] = j + 1.  The saved convolution output is non-zero exactly on t0 - 16 .. t0 + 15
    (clipped to the sequence) with c[t] = w[c, t0 - t + 15] gl[t0]: a frame reads 15 back and 16 ahead.  The data gradient of an impulse in
    dc at t0 reaches exactly t0 - 15 .. t0 + 16 with dgl[t] = w[c, t + 15 - t0].  A kernel with the two halos swapped fails both by one frame.
    Every product has one non-zero term, so the comparison is exact."""
    from dynamic_asr_eval_amd import ops
    T, C = 64, 256
    g = K.gen(42000 + t0)
    u = torch.zeros(B, T, 2 * C)
    u[:, :, C:] = torch.randn(B, T, C, generator=g)
    u[:, t0, :C] = 1.0 + torch.rand(B, C, generator=g)
    w = (torch.arange(KW, dtype=torch.float32) + 1).repeat(C, 1)
    ones, zeros = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    ud, wd = u.to(cuda), w.to(cuda).contiguous()
    s, gl, c = ops.convmod_bn(ud, wd, None, zeros, ones, ones, zeros, "silu", 0.0, save=True)
    gl, c = gl.cpu(), c.cpu()
    assert (gl[:, t0] != 0).all() and (gl[:, :t0] == 0).all() and (gl[:, t0 + 1:] == 0).all()
    want = torch.zeros(B, T, C)
    for t in range(max(0, t0 - 16), min(T, t0 + 16)):
        want[:, t] = w[:, t0 - t + 15] * gl[:, t0]
    assert _bits_equal(c, want), (c - want).abs().max()
    lo, hi = max(0, t0 - 16), min(T, t0 + 16)
    assert (c[:, lo:hi] != 0).all() and (c[:, :lo] == 0).all() and (c[:, hi:] == 0).all()
    # the data gradient: a = 1, gate input 0 => d/da = dgl * sigmoid(0) = dgl / 2 exactly
    u2 = torch.zeros(B, T, 2 * C)
    u2[:, :, :C] = 1.0
    dc = torch.zeros(B, T, C)
    dc[:, t0] = 1.0
    du = ops.glu_dwconv1d_dgrad(u2.to(cuda), wd, dc.to(cuda)).cpu()
    want = torch.zeros(B, T, C)
    for t in range(max(0, t0 - 15), min(T, t0 + 17)):
        want[:, t] = w[:, t + 15 - t0] * 0.5
    assert _bits_equal(du[:, :, :C], want), (du[:, :, :C] - want).abs().max()
    assert _bits_equal(du[:, :, C:], want * 0.5)                  # d/d(gate) = dgl * a * sg * (1 - sg) = dgl / 4
    # and the weight gradient of the same impulse pair: dw[c, j] = sum_t dc[t] gl[t + j - 15] picks gl[t0] at j = 15 when dc's impulse sits at t0
    dw = torch.zeros(C, KW, device=cuda)
    ops.dwconv1d_wgrad(gl.to(cuda), dc.to(cuda), dw, None, beta=0.0)
    want = torch.zeros(C, KW)
    want[:, 15] = gl[0, t0] + gl[1, t0]
    assert _bits_equal(dw, want), (dw.cpu() - want).abs().max()


def test_wrappers_refuse_other_widths(cuda):
    """31 and 33 taps are refused by the fused entries (DYN_E_UNSUPPORTED from the library); an even width by the plain depthwise entries,
    whose symmetric padding and flipped data gradient are wrong there."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.ops import DynError
    i = {k: v.to(cuda) for k, v in _inputs(4, 256, 0).items() if isinstance(v, torch.Tensor)}
    bn = (i["mean"], i["var"], i["weight"], i["bias"])
    for kw in (31, 33):
        w = torch.randn(256, kw, device=cuda)
        with pytest.raises(DynError):
            ops.convmod_bn(i["u"], w, None, *bn)
        with pytest.raises(DynError):
            ops.glu_dwconv1d_dgrad(i["u"], w, i["dc"])
        with pytest.raises(DynError):
            ops.convmod_bn_time_tile(kw)
    for kw in (32, 8):
        w = torch.randn(256, kw, device=cuda)
        with pytest.raises(DynError, match="even"):
            ops.dwconv1d(i["c"], w, None)
        with pytest.raises(DynError, match="even"):
            ops.dwconv1d_dgrad(i["dc"], w)
