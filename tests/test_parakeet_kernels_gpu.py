"""The kernels Parakeet adds — csrc/convmod_bn.hip (dyn_convmod_bn_fwd, dyn_convmod_bn_bwd_act, dyn_glu_dwconv1d_dgrad), the ReLU instances of
the 3x3 stride-2 depthwise stage (csrc/conv.hip, `_act` entries) and dyn_relu_fwd / _bwd — against float64 restatements
(tests/parakeet_refs.py).  Bars: kernel_refs.measured_tol (4 x torch's own fp32 CPU error against float64 + 2e-6) for activations and data
gradients, kernel_refs.wgrad_tol for column sums (5e-4 at 531 rows for norm-like sums, 3e-4 at 400 rows for conv taps)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import parakeet_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

KW, EPS, SENTINEL, NAN = 9, 1e-5, -7777.25, float("nan")
GRID_T, GRID_F = (1, 2, 3, 4, 5, 8), (1, 2, 3, 4, 7)      # tests/test_conv_kernels_gpu.py's grid for the SiLU instances


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(B, T, C, dev):
    """A [B, T, C] view at the head of a buffer that holds two more rows of SENTINEL: (view, the guard rows)."""
    buf = torch.full(((B * T + 2) * C,), SENTINEL, device=dev)
    return buf[:B * T * C].view(B, T, C), buf[B * T * C:]


def _report(name, got, t32, want, floor, worst):
    tol, e32 = K.measured_tol(t32, want, floor)
    err = K.max_err(got, want)
    worst[name] = max(worst.get(name, (0, 0, 0)), (err, e32, tol))
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _inputs(B, T, C, seed):
    g = K.gen(31000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return dict(u=r(B, T, 2 * C), w=r(C, KW) * 0.3, cbias=r(C) * 0.2, mean=r(C) * 0.1, var=0.5 + torch.rand(C, generator=g), weight=1 + 0.1 * r(C),
                bias=r(C) * 0.1, c=r(B, T, C), ds=r(B, T, C), dc=r(B, T, C), old=[r(C) for _ in range(3)])


def _valids(T, tile):
    """None, 1, a value strictly inside a time tile (not on its edge), T."""
    inside = [v for v in (tile + 5, tile // 2 + 1, 2) if 1 < v < T and v % tile]
    return [None, 1] + inside[:1] + [T]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [256, 1024])
def test_convmod_bn_kernels_against_float64(cuda, C, B):
    """Forward, activation / BatchNorm backward and fused GLU + depthwise data gradient at T = 1, 3 (shorter than the half window), 9 (= KW),
    one short of and one past the 16-frame time tile, and 33 (a third tile of one frame); valid = null, 1, strictly inside a tile, T; with and
    without the convolution bias.  Rows >= valid are exact zeros, the two guard rows behind every output keep their sentinel, a second run
    gives equal bits, each null gradient pointer leaves the other sums unchanged bit for bit, dc may be written over ds.
    Worst measured kernel | torch fp32 | bound over the whole grid, the worse of B = 1 and 3 (MI355X):
      C 256:  s 5.7e-07 | 5.7e-07 | 4.3e-06   gl 3.0e-07 | 1.8e-07 | 2.7e-06   c 3.9e-07 | 3.0e-07 | 3.2e-06   dc 7.7e-07 | 5.9e-07 | 4.4e-06
              du 4.4e-07 | 3.8e-07 | 3.5e-06
              dweight 3.5e-06, dbias 3.2e-06, dcbias 3.8e-06 | bound 5.0e-04
      C 1024: s 1.1e-06 | 6.3e-07 | 4.5e-06   gl 3.0e-07 | 3.0e-07 | 3.2e-06   c 4.7e-07 | 4.7e-07 | 3.9e-06   dc 1.4e-06 | 5.8e-07 | 4.3e-06
              du 4.7e-07 | 5.6e-07 | 4.3e-06
              dweight 7.5e-06, dbias 3.9e-06, dcbias 5.4e-06 | bound 5.0e-04"""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    L = load()
    tile = ops.convmod_bn_time_tile()
    assert tile == 16
    worst = {}
    for T in (1, 3, KW, tile - 1, tile + 1, 2 * tile + 1):
        i = _inputs(B, T, C, 7 * T + B + C)
        i64 = {k: v.double() for k, v in i.items() if k != "old"}
        d = {k: v.to(cuda) for k, v in i.items() if k != "old"}
        for valid in _valids(T, tile):
            vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
            v = T if valid is None else valid
            for has_cb in (True, False):
                cb = lambda t: t["cbias"] if has_cb else None                                    # noqa: E731
                # ---------------- forward
                want = R.convmod_bn_ref(i64["u"], i64["w"], cb(i64), i64["mean"], i64["var"], i64["weight"], i64["bias"], EPS, valid)
                t32 = R.convmod_bn_ref(i["u"], i["w"], cb(i), i["mean"], i["var"], i["weight"], i["bias"], EPS, valid)
                runs = []
                for _ in range(2):
                    outs = [_guarded(B, T, C, cuda) for _ in range(3)]
                    check(L.dyn_convmod_bn_fwd(d["u"].data_ptr(), d["w"].data_ptr(), d["cbias"].data_ptr() if has_cb else None,
                                               d["mean"].data_ptr(), d["var"].data_ptr(), d["weight"].data_ptr(), d["bias"].data_ptr(),
                                               outs[0][0].data_ptr(), outs[1][0].data_ptr(), outs[2][0].data_ptr(),
                                               None if vd is None else vd.data_ptr(), B, T, C, KW, 0, EPS, _stream()), "fwd")
                    for o, guard in outs:
                        assert (guard == SENTINEL).all(), (T, valid)
                        assert o[:, v:].abs().max().item() == 0.0 if v < T else True, (T, valid)
                    runs.append([o for o, _ in outs])
                for a, c_ in zip(*runs):
                    assert _bits_equal(a, c_), ("two runs differ", T, valid)
                for name, got, t, w64 in zip(("s", "gl", "c"), runs[0], t32, want):
                    _report(name, got, t, w64, 2e-6, worst)
                s, gl, cv = ops.convmod_bn(d["u"], d["w"], cb(d), d["mean"], d["var"], d["weight"], d["bias"], "silu", EPS, valid=vd, save=True)
                assert _bits_equal(s, runs[0][0]) and _bits_equal(gl, runs[0][1]) and _bits_equal(cv, runs[0][2])
                s_only, none_gl, none_c = ops.convmod_bn(d["u"], d["w"], cb(d), d["mean"], d["var"], d["weight"], d["bias"], valid=vd)
                assert none_gl is None and none_c is None and _bits_equal(s_only, s)
            # ---------------- activation / BatchNorm backward
            want = R.convmod_bn_bwd_act_ref(i64["c"], i64["mean"], i64["var"], i64["weight"], i64["bias"], i64["ds"], EPS, valid)
            t32 = R.convmod_bn_bwd_act_ref(i["c"], i["mean"], i["var"], i["weight"], i["bias"], i["ds"], EPS, valid)
            sums_tol = K.wgrad_tol(5e-4, B * T, 531)
            full = {}
            for beta in (0.0, 1.0):
                for null in (None, 0, 1, 2):
                    acc = [None if k == null else (o.to(cuda) if beta else torch.full_like(o, NAN).to(cuda)) for k, o in enumerate(i["old"])]
                    dc, guard = _guarded(B, T, C, cuda)
                    got = ops.convmod_bn_bwd_act(d["c"], d["mean"], d["var"], d["weight"], d["bias"], d["ds"], *acc, "silu", EPS, valid=vd, out=dc,
                                                 wgrad_beta=beta)
                    assert got is dc and (guard == SENTINEL).all()
                    if v < T:
                        assert dc[:, v:].abs().max().item() == 0.0
                    if null is None:
                        full[beta] = [dc.clone()] + [a.clone() for a in acc]
                        _report("dc", dc, t32[0], want[0], 2e-6, worst)
                        for k, name in enumerate(("dweight", "dbias", "dcbias")):
                            err = K.max_err(acc[k], want[1 + k] + beta * i["old"][k].double())
                            worst[name] = max(worst.get(name, (0, 0, 0)), (err, 0.0, sums_tol))
                            assert err <= sums_tol, (name, err, sums_tol, T, valid, beta)
                    else:
                        assert _bits_equal(dc, full[beta][0])
                        for k in range(3):
                            assert k == null or _bits_equal(acc[k], full[beta][1 + k]), ("a null pointer changed another sum", null, k)
            over = d["ds"].clone()
            assert ops.convmod_bn_bwd_act(d["c"], d["mean"], d["var"], d["weight"], d["bias"], over, None, None, None, valid=vd, out=over) is over
            assert _bits_equal(over, full[1.0][0])
            # ---------------- GLU' x depthwise data gradient
            want = R.glu_dwconv1d_dgrad_ref(i64["u"], i64["w"], i64["dc"], valid)
            t32 = R.glu_dwconv1d_dgrad_ref(i["u"], i["w"], i["dc"], valid)
            first = None
            for _ in range(2):
                du, guard = _guarded(B, T, 2 * C, cuda)
                assert ops.glu_dwconv1d_dgrad(d["u"], d["w"], d["dc"], valid=vd, out=du) is du and (guard == SENTINEL).all()
                if v < T:
                    assert du[:, v:].abs().max().item() == 0.0
                first = du if first is None else first
                assert _bits_equal(du, first)
            _report("du", first, t32, want, 2e-6, worst)
    for name, (err, e32, tol) in worst.items():
        print(f"  C {C} B {B} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")


def test_convmod_bn_wrappers_refuse_bad_operands(cuda):
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.ops import DynError
    i = {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in _inputs(1, 4, 256, 0).items()}
    bn = (i["mean"], i["var"], i["weight"], i["bias"])
    with pytest.raises(DynError):
        ops.convmod_bn(i["u"], i["w"], None, *bn, act="gelu")
    with pytest.raises(DynError):
        ops.convmod_bn(i["u"], i["w"][:, :7].contiguous(), None, *bn)                             # KW = 7: DYN_E_UNSUPPORTED from the library
    with pytest.raises(DynError):
        ops.convmod_bn(i["u"], i["w"], None, i["mean"][:128], *bn[1:])
    with pytest.raises(DynError):
        ops.glu_dwconv1d_dgrad(i["u"], i["w"], i["dc"], out=i["u"])
    with pytest.raises(DynError):
        ops.convmod_bn_bwd_act(i["c"], *bn, i["ds"][:, :2], None, None, None)


def _relu_inputs(B, T, Fq, C, seed=0):
    g = K.gen(32000 + seed + 101 * T + 13 * Fq + C)
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    z = torch.randn(B, T, Fq, C, generator=g) * 2
    z = z + torch.where(z >= 0, 1e-3, -1e-3)                  # none within 1e-3 of zero: ReLU' is well defined against float64
    z.view(-1)[0], z.view(-1)[1] = z.view(-1)[0].abs(), -z.view(-1)[1].abs()     # both sides of zero even in the four-element input
    return dict(z=z, w=torch.randn(C, 3, 3, generator=g) * 0.3, b=torch.randn(C, generator=g), du=torch.randn(B, To, Fo, C, generator=g),
                old_w=torch.randn(C, 3, 3, generator=g), old_b=torch.randn(C, generator=g))


def _relu_case(cuda, B, T, Fq, C, worst):
    from dynamic_asr_eval_amd import ops
    i = _relu_inputs(B, T, Fq, C)
    assert i["z"].abs().min().item() >= 1e-3 and (i["z"] > 0).any() and (i["z"] < 0).any()
    want = R.relu_dwconv2d_s2(*(i[k].double() for k in ("z", "w", "b", "du")))
    t32 = R.relu_dwconv2d_s2(*(i[k] for k in ("z", "w", "b", "du")))
    d = {k: v.to(cuda) for k, v in i.items()}
    To, Fo = K.s2_out_len(T), K.s2_out_len(Fq)
    u = ops.dwconv2d_s2_act(d["z"], d["w"], d["b"], "relu", out=torch.full((B, To, Fo, C), NAN, device=cuda))
    _report("relu fwd", u, t32[0], want[0], 2e-6, worst)
    dz = ops.dwconv2d_s2_dgrad_act(d["z"], d["w"], d["du"], "relu", out=torch.full((B, T, Fq, C), NAN, device=cuda))
    _report("relu dgrad", dz, t32[1], want[1], 2e-6, worst)
    assert (dz[d["z"] < 0] == 0).all()
    tol = K.wgrad_tol(3e-4, B * To * Fo, 400)
    for beta in (0.0, 1.0):
        dw = d["old_w"].clone() if beta else torch.full_like(d["old_w"], NAN)
        db = d["old_b"].clone() if beta else torch.full_like(d["old_b"], NAN)
        ops.dwconv2d_s2_wgrad_act(d["z"], d["du"], dw, db, "relu", beta=beta)
        for name, got, w64, old in (("relu wgrad", dw, want[2], i["old_w"]), ("relu bgrad", db, want[3], i["old_b"])):
            err = K.max_err(got, w64 + beta * old.double())
            worst[name] = max(worst.get(name, (0, 0, 0)), (err, 0.0, tol))
            assert err <= tol, (name, err, tol, B, T, Fq, C, beta)
    # act 0 through the new entries is the SiLU entry, bit for bit
    assert _bits_equal(ops.dwconv2d_s2_act(d["z"], d["w"], d["b"], "silu"), ops.dwconv2d_s2(d["z"], d["w"], d["b"]))
    assert _bits_equal(ops.dwconv2d_s2_dgrad_act(d["z"], d["w"], d["du"], "silu"), ops.dwconv2d_s2_dgrad(d["z"], d["w"], d["du"]))
    a, b = (d["old_w"].clone(), d["old_b"].clone()), (d["old_w"].clone(), d["old_b"].clone())
    ops.dwconv2d_s2_wgrad_act(d["z"], d["du"], *a, "silu", beta=1.0)
    ops.dwconv2d_s2_wgrad(d["z"], d["du"], *b, beta=1.0)
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])


@pytest.mark.parametrize("B", [1, 3])
def test_relu_depthwise_stage_parity_grid(cuda, B):
    """The shapes tests/test_conv_kernels_gpu.py::test_subsampling_parity_grid gives the SiLU instances: T x F over every parity and the
    one-row / one-column inputs at C = 4 (the v4 kernels, one lane live).
    Worst measured kernel | torch fp32 | bound (MI355X): B = 1: fwd 4.7e-07 | 1.1e-07 | 2.4e-06, dgrad 9.8e-08 | 9.8e-08 | 2.4e-06, wgrad 1.3e-06,
    bgrad 6.4e-07 | bound 3.0e-04; B = 3: fwd 2.7e-07 | 3.2e-07 | 3.3e-06, dgrad 1.2e-07 | 1.2e-07 | 2.5e-06, wgrad 1.7e-06, bgrad 1.3e-06 | 3.0e-04."""
    worst = {}
    for T in GRID_T + ((9,) if B == 1 else ()):
        for Fq in GRID_F:
            _relu_case(cuda, B, T, Fq, 4, worst)
    for name, (err, e32, tol) in worst.items():
        print(f"  B {B} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")


@pytest.mark.parametrize("C", [6, 256, 258, 260])
def test_relu_depthwise_stage_channel_blocks(cuda, C):
    """6 and 258: the scalar kernels (258: their second channel block); 256 and 260: the v4 kernels (260: the channel loop's second pass).
    Worst measured kernel | torch fp32 | bound over the four widths (MI355X): fwd 6.2e-07 | 4.8e-07 | 3.9e-06 (C 256), dgrad 2.1e-07 | 2.1e-07 |
    2.9e-06 (C 256), wgrad 2.5e-06, bgrad 2.0e-06 | bound 3.0e-04 (C 258)."""
    worst = {}
    _relu_case(cuda, 2, 5, 7, C, worst)
    for name, (err, e32, tol) in worst.items():
        print(f"  C {C} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")


@pytest.mark.parametrize("n", [4, 1028, 1031, 1 << 20])
def test_relu_elementwise_is_exact(cuda, n):
    """max(x, 0) and its mask are exact in fp32: equal bits with torch, a tail that is no multiple of 4 included; in place allowed."""
    from dynamic_asr_eval_amd import ops
    g = K.gen(33000 + n)
    x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x[::7] = 0.0
    xd, dyd = x.to(cuda), dy.to(cuda)
    assert _bits_equal(ops.relu(xd), torch.relu(x))
    assert _bits_equal(ops.relu_bwd(xd, dyd), torch.where(x > 0, dy, torch.zeros_like(dy)))
    y = xd.clone()
    assert ops.relu(y, out=y) is y and _bits_equal(y, torch.relu(x))
    gd = dyd.clone()
    assert ops.relu_bwd(xd, gd, out=gd) is gd and _bits_equal(gd, torch.where(x > 0, dy, torch.zeros_like(dy)))
