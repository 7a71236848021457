"""The per-row (`_lens`) entries of a ragged batch against float64 restatements (tests/ragged_refs.py) at the smallest shapes where they can go
wrong: csrc/convmod_bn.hip (forward, activation / BatchNorm backward, fused GLU + depthwise data gradient), csrc/relshift.hip (the
relative-position softmax), csrc/softmax.hip (the plain row softmax of the teacher-forced cross-attention), csrc/conv.hip (the ReLU depthwise
3x3 stride-2 stage forward / dgrad / wgrad, the first conv forward / wgrad, the row mask), csrc/seq2seq_step.hip over csrc/dec_attn.h
(dyn_seq2seq_steps_len: per-row encoder keys in the batched greedy step).  Bars: ragged_refs.tol (4 x torch's own fp32 CPU error against float64 + 2e-5 * max(1, max |want|)) for activations,
probabilities and data gradients, kernel_refs.wgrad_tol for column sums and conv taps (the bars of tests/test_parakeet_kernels_gpu.py).
What lies past a row's length is compared with `== 0`.  Every ragged call is also bit-equal, row by row, to the scalar-`valid` entry
called on that row alone with its length: one kernel body serves both.  The entries from before keep their bits: against their
references at their tolerances, equal between two calls, and equal to the `_lens` entry given full lengths."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import parakeet_refs as R  # noqa: E402
import ragged_refs as RR  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
CONVMOD_T = 37
CONVMOD_LENS = ((37, 16, 1), (17, 37, 15), (-2, 37, 36))       # -2: clamped to 0 by the kernel, a row with no valid frame


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def _check(name, got, t32, w64, worst):
    tol, e32 = RR.tol(t32, w64)
    err = K.max_err(got, w64)
    worst[name] = max(worst.get(name, (0.0, 0.0, 0.0)), (err, e32, tol))
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _past_is_zero(t, lens, T):
    for b, n in enumerate(RR.clamp(lens, T)):
        assert t[b, n:].abs().max().item() == 0.0 if n < T else True, (b, n)


def _convmod_inputs(B, T, C, KW, seed):
    g = K.gen(52000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return dict(u=r(B, T, 2 * C), w=r(C, KW) * 0.3, cbias=r(C) * 0.2, mean=r(C) * 0.1, var=0.5 + torch.rand(C, generator=g), weight=1 + 0.1 * r(C),
                bias=r(C) * 0.1, c=r(B, T, C), ds=r(B, T, C), dc=r(B, T, C))


@pytest.mark.parametrize("KW", [9, 32])
@pytest.mark.parametrize("C", [256, 512])
def test_convmod_entries_per_row(cuda, C, KW):
    """[3, 37, C]: lengths on, one past and one short of the 16-frame tile (16, 17, 15), across the 32-frame tile (36, 37), a one-frame row, a
    full row and a count below zero (clamped: the row is all padding).  Forward s / gl / c, the activation / BatchNorm backward with its three
    column sums taken over the valid rows only (9 taps: the entry's only width), the fused data gradient.
    Worst measured kernel | torch fp32 | bound (MI355X), C 256 / 512:
      KW 9:  s 5.8e-07 | 6.1e-07 | 5.3e-05   gl 3.2e-07 | 3.2e-07 | 6.8e-05   c 4.2e-07 | 4.2e-07 | 6.6e-05   du 5.5e-07 | 4.7e-07 | 7.3e-05
             dc 7.9e-07 | 6.9e-07 | 9.1e-05   dweight 5.3e-06, dbias 2.4e-06, dcbias 4.6e-06 | bound 5.0e-04
      KW 32: s 1.4e-06 | 1.2e-06 | 9.2e-05   gl 2.7e-07 | 2.7e-07 | 6.1e-05   c 8.9e-07 | 7.7e-07 | 8.6e-05   du 1.0e-06 | 1.5e-06 | 1.2e-04"""
    from dynamic_asr_eval_amd import ops
    B, T = 3, CONVMOD_T
    i = _convmod_inputs(B, T, C, KW, C + KW)
    i64 = {k: v.double() for k, v in i.items()}
    d = {k: v.to(cuda) for k, v in i.items()}
    bn = lambda t: (t["mean"], t["var"], t["weight"], t["bias"])                                  # noqa: E731
    worst = {}
    for lens in CONVMOD_LENS:
        ld = _i32(lens, cuda)
        want = RR.convmod_bn_ref(i64["u"], i64["w"], i64["cbias"], *bn(i64), EPS, lens)
        t32 = RR.convmod_bn_ref(i["u"], i["w"], i["cbias"], *bn(i), EPS, lens)
        got = ops.convmod_bn(d["u"], d["w"], d["cbias"], *bn(d), "silu", EPS, lens=ld, save=True)
        again = ops.convmod_bn(d["u"], d["w"], d["cbias"], *bn(d), "silu", EPS, valid=ops.RowLens(ld), save=True)
        for name, o, o2, t, w in zip(("s", "gl", "c"), got, again, t32, want):
            _check(name, o, t, w, worst)
            _past_is_zero(o, lens, T)
            assert torch.equal(o, o2), name
        for b, n in enumerate(lens):                                                              # the scalar entry on the row alone: equal bits
            solo = ops.convmod_bn(d["u"][b:b + 1].clone(), d["w"], d["cbias"], *bn(d), "silu", EPS, valid=_i32([n], cuda), save=True)
            assert all(torch.equal(o[b:b + 1], s) for o, s in zip(got, solo)), (lens, b)
        # ---------------- data gradient
        want = RR.glu_dwconv1d_dgrad_ref(i64["u"], i64["w"], i64["dc"], lens)
        du = ops.glu_dwconv1d_dgrad(d["u"], d["w"], d["dc"], lens=ld)
        _check("du", du, RR.glu_dwconv1d_dgrad_ref(i["u"], i["w"], i["dc"], lens), want, worst)
        _past_is_zero(du, lens, T)
        for b, n in enumerate(lens):
            solo = ops.glu_dwconv1d_dgrad(d["u"][b:b + 1].clone(), d["w"], d["dc"][b:b + 1].clone(), valid=_i32([n], cuda))
            assert torch.equal(du[b:b + 1], solo), (lens, b)
        if KW != 9:
            continue
        # ---------------- activation / BatchNorm backward: dc and the three column sums, rows past the length left out
        want = RR.convmod_bn_bwd_act_ref(i64["c"], *bn(i64), i64["ds"], EPS, lens)
        t32 = RR.convmod_bn_bwd_act_ref(i["c"], *bn(i), i["ds"], EPS, lens)
        sums = [torch.full((C,), 0.25, device=cuda) for _ in range(3)]
        dc = ops.convmod_bn_bwd_act(d["c"], *bn(d), d["ds"], *sums, "silu", EPS, lens=ld, wgrad_beta=2.0)
        _check("dc", dc, t32[0], want[0], worst)
        _past_is_zero(dc, lens, T)
        bar = K.wgrad_tol(5e-4, B * T, 531)
        for name, s, w in zip(("dweight", "dbias", "dcbias"), sums, want[1:]):
            err = K.max_err(s, 0.5 + w)                                                           # wgrad_beta * old + the sum
            worst[name] = max(worst.get(name, (0.0,)), (err,))
            assert err <= bar, (name, err, bar)
        sums2 = [torch.full((C,), 0.25, device=cuda) for _ in range(3)]
        dc2 = ops.convmod_bn_bwd_act(d["c"], *bn(d), d["ds"], *sums2, "silu", EPS, lens=ld, wgrad_beta=2.0)
        assert torch.equal(dc, dc2) and all(torch.equal(a, b_) for a, b_ in zip(sums, sums2))
    print(f"C {C} KW {KW}: " + "  ".join(f"{k} " + " | ".join(f"{x:.1e}" for x in v) for k, v in worst.items()))


@pytest.mark.parametrize("T", [17, 300])
def test_relshift_softmax_per_row(cuda, T):
    """[3, 2, T, T] at one (T = 17) and two (T = 300) items per thread: a full row, a single key, 9 keys, T - 1 keys and a count across the
    256-column boundary (257; clamped to T at 17).  Probabilities past the count are exact zeros, a row's first lens[b] columns are bit for
    bit those of the scalar entry called on that batch entry alone, in place too.
    Measured (MI355X): within 2.1e-07 of float64 (torch fp32: 3.4e-07, bound 2.1e-05) at both sizes."""
    from dynamic_asr_eval_amd import ops
    B, nh, ld = 3, 2, 2 * T + 3
    g = K.gen(53000 + T)
    S, BD = torch.randn(B, nh, T, T, generator=g) * 2, torch.randn(B, nh, T, ld, generator=g) * 2
    Sd, BDd = S.to(cuda), BD.to(cuda)
    for lens in ((T, 1, 9), (T, T - 1, 257), (0, -5, 2)):
        ld_ = _i32(lens, cuda)
        want = RR.softmax_relshift_ref(S.double(), BD.double(), lens)
        got = ops.softmax_relshift(Sd, BDd, lens=ld_, ld_bd=ld)
        tol, e32 = RR.tol(RR.softmax_relshift_ref(S, BD, lens), want)
        err = K.max_err(got, want)
        print(f"T {T} lens {lens}: err {err:.1e} | torch fp32 {e32:.1e} | bound {tol:.1e}")
        assert err <= tol, (err, tol)
        assert torch.isfinite(got).all()
        assert (got.sum(-1) - 1).abs().max().item() < 1e-5
        for b, n in enumerate(RR.clamp(lens, T, 1)):
            assert got[b, :, :, n:].abs().max().item() == 0.0 if n < T else True
            solo = ops.softmax_relshift(Sd[b:b + 1].clone(), BDd[b:b + 1].clone(), valid=_i32([lens[b]], cuda), ld_bd=ld)
            assert torch.equal(got[b:b + 1], solo), (lens, b)
        inplace = Sd.clone()
        assert ops.softmax_relshift(inplace, BDd, out=inplace, valid=ops.RowLens(ld_), ld_bd=ld) is inplace and torch.equal(inplace, got)


def _stage_lens(T):
    """Input frame counts with an odd, an even and a one-frame row (the odd row's last output frame reads one frame past its length), then the
    same rows shorter so that whole tiles of rows are padding, and counts outside [0, T] (clamped)."""
    odd, even = (T, T - 1) if T % 2 else (T - 1, T)
    return ((odd, even, 1), (5, 2, 1), (T + 9, -1, 3))


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("T", [9, 34])
def test_depthwise_stage_per_row(cuda, T, C):
    """z [3, T, 16, C] -> u [3, To, 8, C] with ReLU in the loads: input rows past lens_in[b] hold junk and read as zeros, output rows past
    lens_out[b] are exact zeros; the data gradient has exact zeros past lens_in[b] and reads no du past lens_out[b] (junk there); the weight
    gradient with du zeroed past the length.  lens_out is the stage's own arithmetic, then also one row less (a mask that cuts a live row)."""
    from dynamic_asr_eval_amd import ops
    B, Fq = 3, 16
    To = RR.out_len(T)
    g = K.gen(54000 + 10 * T + C)
    z, du = torch.randn(B, T, Fq, C, generator=g), torch.randn(B, To, RR.out_len(Fq), C, generator=g)
    w, bias = torch.randn(C, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2
    zd, wd, bd = z.to(cuda), w.to(cuda), bias.to(cuda)
    for lin in _stage_lens(T):
        for lout in ([RR.out_len(n) for n in RR.clamp(lin, T)], [max(RR.out_len(n) - 1, 0) for n in RR.clamp(lin, T)]):
            li, lo = _i32(lin, cuda), _i32(lout, cuda)
            keep_in = RR.prefix_mask(RR.clamp(lin, T), T)[:, :, None, None]
            keep_out = RR.prefix_mask(RR.clamp(lout, To), To)[:, :, None, None]
            z_junk = torch.where(keep_in, z, torch.full_like(z, 1e4)).to(cuda)                    # what lies past the length must not matter
            du_junk = torch.where(keep_out, du, torch.full_like(du, -1e4)).to(cuda)
            du_zero = (du * keep_out).to(cuda)
            want = RR.relu_dwconv2d_s2_ref(z.double(), w.double(), bias.double(), lin, lout, du.double())
            t32 = RR.relu_dwconv2d_s2_ref(z, w, bias, lin, lout, du)
            u = ops.dwconv2d_s2_act(z_junk, wd, bd, "relu", lens_in=li, lens_out=lo)
            dz = ops.dwconv2d_s2_dgrad_act(z_junk, wd, du_junk, "relu", lens_in=li, lens_out=lo)
            for name, got, t, w64, lens, n in (("u", u, t32[0], want[0], lout, To), ("dz", dz, t32[1], want[1], lin, T)):
                tol, e32 = RR.tol(t, w64)
                err = K.max_err(got, w64)
                assert err <= tol, (name, lin, lout, err, tol, e32)
                _past_is_zero(got, lens, n)
            assert torch.equal(u, ops.dwconv2d_s2_act(zd, wd, bd, "relu", lens_in=li, lens_out=lo))            # junk or not: equal bits
            dw, db = torch.full((C, 3, 3), 0.5, device=cuda), torch.full((C,), 0.5, device=cuda)
            ops.dwconv2d_s2_wgrad_act(z_junk, du_zero, dw, db, "relu", beta=1.0, lens_in=li)
            bar = K.wgrad_tol(3e-4, B * To * 8, 400)
            assert K.max_err(dw, 0.5 + want[2]) <= bar and K.max_err(db, 0.5 + want[3]) <= bar, (lin, lout)


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("T", [9, 34])
def test_first_conv_per_row(cuda, T, C):
    """x [3, T, 16] with junk in the frames past a row's length -> z [3, To, 8, C]: every row of z is that of the zero-padded input (the rows
    that read no valid frame hold the bias), and the weight gradient reads the same zeros."""
    from dynamic_asr_eval_amd import ops
    B, Fq = 3, 16
    To = RR.out_len(T)
    g = K.gen(55000 + 10 * T + C)
    x, dz = torch.randn(B, T, Fq, generator=g), torch.randn(B, To, RR.out_len(Fq), C, generator=g)
    w, bias = torch.randn(C, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2
    wd, bd = w.to(cuda), bias.to(cuda)
    for lens in _stage_lens(T):
        ld = _i32(lens, cuda)
        xj = RR.junk_padded(x, RR.clamp(lens, T)).to(cuda)
        want = RR.conv2d_first_ref(x.double(), w.double(), bias.double(), lens, dz.double())
        t32 = RR.conv2d_first_ref(x, w, bias, lens, dz)
        zz = ops.conv2d_first(xj, wd, bd, lens=ld)
        tol, e32 = RR.tol(t32[0], want[0])
        assert K.max_err(zz, want[0]) <= tol, (lens, K.max_err(zz, want[0]), tol)
        assert torch.equal(zz, ops.conv2d_first(RR.zero_padded(x, RR.clamp(lens, T)).to(cuda), wd, bd))         # the old entry on zeros: equal bits
        dw, db = torch.full((C, 3, 3), 0.5, device=cuda), torch.full((C,), 0.5, device=cuda)
        ops.conv2d_first_wgrad(xj, dz.to(cuda), dw, db, beta=1.0, lens=ld)
        bar = K.wgrad_tol(3e-4, B * To * 8, 400)
        assert K.max_err(dw, 0.5 + want[1]) <= bar and K.max_err(db, 0.5 + want[2]) <= bar, lens


def test_row_mask(cuda):
    from dynamic_asr_eval_amd import ops
    x = torch.randn(3, 5, 7, 12, generator=K.gen(56000))
    for lens in ((5, 2, 1), (0, 9, -3)):
        got = ops.mask_rows_lens(x.to(cuda), _i32(lens, cuda))
        assert torch.equal(got.cpu(), x * RR.prefix_mask(RR.clamp(lens, 5), 5)[:, :, None, None])


def test_entries_from_before_keep_their_bits(cuda):
    """One shape each: the scalar entries (null `valid`) against the references and bars tests/test_parakeet_kernels_gpu.py and
    tests/test_attention_kernels_gpu.py give them, equal bits between two calls, and equal bits to the `_lens` entry given full lengths."""
    from dynamic_asr_eval_amd import ops
    B, T, C = 3, 37, 256
    full = _i32([T] * B, cuda)
    i = _convmod_inputs(B, T, C, 9, 1)
    i64 = {k: v.double() for k, v in i.items()}
    d = {k: v.to(cuda) for k, v in i.items()}
    bn = lambda t: (t["mean"], t["var"], t["weight"], t["bias"])                                  # noqa: E731
    runs = [ops.convmod_bn(d["u"], d["w"], d["cbias"], *bn(d), "silu", EPS, save=True) for _ in range(2)]
    lens_run = ops.convmod_bn(d["u"], d["w"], d["cbias"], *bn(d), "silu", EPS, lens=full, save=True)
    want, t32 = R.convmod_bn_ref(i64["u"], i64["w"], i64["cbias"], *bn(i64), EPS), R.convmod_bn_ref(i["u"], i["w"], i["cbias"], *bn(i), EPS)
    for a, b_, c_, t, w in zip(*runs, lens_run, t32, want):
        assert torch.equal(a, b_) and torch.equal(a, c_)
        assert K.max_err(a, w) <= K.measured_tol(t, w, 2e-6)[0]
    du = [ops.glu_dwconv1d_dgrad(d["u"], d["w"], d["dc"]) for _ in range(2)] + [ops.glu_dwconv1d_dgrad(d["u"], d["w"], d["dc"], lens=full)]
    assert torch.equal(du[0], du[1]) and torch.equal(du[0], du[2])
    w64 = R.glu_dwconv1d_dgrad_ref(i64["u"], i64["w"], i64["dc"])
    assert K.max_err(du[0], w64) <= K.measured_tol(R.glu_dwconv1d_dgrad_ref(i["u"], i["w"], i["dc"]), w64, 2e-6)[0]
    outs = []
    for lens in (None, None, full):
        sums = [torch.zeros(C, device=cuda) for _ in range(3)]
        outs.append([ops.convmod_bn_bwd_act(d["c"], *bn(d), d["ds"], *sums, "silu", EPS, lens=lens)] + sums)
    assert all(torch.equal(a, b_) and torch.equal(a, c_) for a, b_, c_ in zip(*outs))
    want = R.convmod_bn_bwd_act_ref(i64["c"], *bn(i64), i64["ds"], EPS)
    assert K.max_err(outs[0][0], want[0]) <= K.measured_tol(R.convmod_bn_bwd_act_ref(i["c"], *bn(i), i["ds"], EPS)[0], want[0], 2e-6)[0]
    assert all(K.max_err(s, w) <= K.wgrad_tol(5e-4, B * T, 531) for s, w in zip(outs[0][1:], want[1:]))
    # the relative-position softmax
    Ts, nh = 40, 2
    g = K.gen(57000)
    S, BD = torch.randn(B, nh, Ts, Ts, generator=g).to(cuda), torch.randn(B, nh, Ts, 2 * Ts - 1, generator=g).to(cuda)
    p = [ops.softmax_relshift(S, BD) for _ in range(2)] + [ops.softmax_relshift(S, BD, lens=_i32([Ts] * B, cuda))]
    assert torch.equal(p[0], p[1]) and torch.equal(p[0], p[2])
    want = torch.softmax(K.relshift_scores_ref(S.double().cpu(), BD.double().cpu()), -1)
    assert K.max_err(p[0], want) <= K.measured_tol(torch.softmax(K.relshift_scores_ref(S.cpu(), BD.cpu()), -1), want, 2e-6)[0]
    # the depthwise stage and the first conv
    Tz, Fq = 9, 16
    z, du_ = torch.randn(B, Tz, Fq, C, generator=g), torch.randn(B, 5, 8, C, generator=g)
    w, bias = torch.randn(C, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2
    zd, dud, wd, bd = z.to(cuda), du_.to(cuda), w.to(cuda), bias.to(cuda)
    fz, fo = _i32([Tz] * B, cuda), _i32([5] * B, cuda)
    u = [ops.dwconv2d_s2_act(zd, wd, bd, "relu") for _ in range(2)] + [ops.dwconv2d_s2_act(zd, wd, bd, "relu", lens_in=fz, lens_out=fo)]
    dz = [ops.dwconv2d_s2_dgrad_act(zd, wd, dud, "relu") for _ in range(2)] + [ops.dwconv2d_s2_dgrad_act(zd, wd, dud, "relu", lens_in=fz, lens_out=fo)]
    assert torch.equal(u[0], u[1]) and torch.equal(u[0], u[2]) and torch.equal(dz[0], dz[1]) and torch.equal(dz[0], dz[2])
    want, t32 = R.relu_dwconv2d_s2(z.double(), w.double(), bias.double(), du_.double()), R.relu_dwconv2d_s2(z, w, bias, du_)
    assert K.max_err(u[0], want[0]) <= K.measured_tol(t32[0], want[0], 2e-6)[0] and K.max_err(dz[0], want[1]) <= K.measured_tol(t32[1], want[1], 2e-6)[0]
    grads = []
    for lens in (None, None, fz):
        dw, db = torch.zeros(C, 3, 3, device=cuda), torch.zeros(C, device=cuda)
        ops.dwconv2d_s2_wgrad_act(zd, dud, dw, db, "relu", beta=0.0, lens_in=lens)
        grads.append((dw, db))
    assert all(torch.equal(a, b_) and torch.equal(a, c_) for a, b_, c_ in zip(*grads))
    assert K.max_err(grads[0][0], want[2]) <= K.wgrad_tol(3e-4, B * 5 * 8, 400) and K.max_err(grads[0][1], want[3]) <= K.wgrad_tol(3e-4, B * 5 * 8, 400)
    x = torch.randn(B, Tz, Fq, generator=g).to(cuda)
    z1 = [ops.conv2d_first(x, wd, bd) for _ in range(2)] + [ops.conv2d_first(x, wd, bd, lens=fz)]
    assert torch.equal(z1[0], z1[1]) and torch.equal(z1[0], z1[2])
    w64 = RR.conv2d_first_ref(x.double().cpu(), w.double(), bias.double(), [Tz] * B)
    assert K.max_err(z1[0], w64) <= K.measured_tol(RR.conv2d_first_ref(x.cpu(), w, bias, [Tz] * B), w64, 2e-6)[0]


# ----------------------------------------------------------------------------------------------------------- the seq2seq step, per-row keys
def _steps_len(SK, st, lens_dev, t, **over):
    import ctypes
    L = SK._lib()
    L.check(L.load().dyn_seq2seq_steps_len(ctypes.byref(st.desc(**over)), lens_dev.data_ptr(), t, 1, 0, torch.cuda.current_stream().cuda_stream),
            "dyn_seq2seq_steps_len")


@pytest.mark.parametrize("n_enc", [40, 1030])
@pytest.mark.parametrize("rows", [1, 4, 8])
def test_seq2seq_steps_per_row_keys(cuda, rows, n_enc):
    """dyn_seq2seq_steps_len on tests/test_seq2seq_step_kernels_gpu.py's smallest width tuple (d 256, 8 heads, d_ff 256, 2 layers, vocab 40),
    three greedy steps: the row-block instances of 1, 4 and 8 rows, 40 and 1030 encoder keys (the score loop's second pass and more),
    per-row counts 1 and 3 (fewer keys than the four splits: empty triples), n_enc, and counts in between / outside (clamped).  Every
    step's logits against cohere_asr_refs.decoder_ref on the row's TRUNCATED keys | values (the recipe of that file), and row r bit-equal
    to the same row stepped alone by dyn_seq2seq_steps with n_enc = lens[r] keys at the same stride."""
    import cohere_asr_refs as CR
    import test_seq2seq_step_kernels_gpu as SK
    S = 3
    lens = ([n_enc, 1, 3, n_enc // 2 + 1, n_enc + 7, 0, 2, n_enc - 1] if rows > 1 else [3])[:rows]
    keys = RR.clamp(lens, n_enc, 1)
    m = SK.Model(cuda, 256, 8, 256, layers=2, vocab=40, n_enc=n_enc, rows=rows, seed=rows + n_enc)
    ld = _i32(lens, cuda)
    starts = SK._starts(rows, 40, rows)
    st = SK.State(m, S)
    st.tokens[:, 0] = torch.tensor(starts, dtype=torch.int32).to(cuda)
    got = []
    for t in range(S):
        _steps_len(SK, st, ld, t)
        got.append(st.logits.clone())
    got = torch.stack(got, 1)
    toks = st.tokens[:, :S].cpu()
    for r in range(rows):
        kv = [t[r:r + 1, :keys[r]] for t in m.kv_cpu]
        want64 = CR.decoder_ref(m.cpu, toks[r:r + 1], kv, m.heads, torch.float64)[0]
        want32 = CR.decoder_ref(m.cpu, toks[r:r + 1], kv, m.heads, torch.float32)[0]
        SK._close(f"per-row keys R={rows} n_enc={n_enc} row {r} keys {keys[r]}", "logits", got[r:r + 1], want32, want64)
        assert all(int(st.tokens[r, t + 1]) == SK._first_max(got[r, t]) for t in range(S))
        one = SK.Model(cuda, 256, 8, 256, layers=2, vocab=40, n_enc=n_enc, rows=1, seed=rows + n_enc)
        one.kv_cpu = [t[r:r + 1].clone() for t in m.kv_cpu]
        one.kv = [t.to(cuda) for t in one.kv_cpu]
        s1 = SK.State(one, S)
        s1.tokens[:, 0] = torch.tensor(starts[r:r + 1], dtype=torch.int32).to(cuda)
        for t in range(S):
            s1.run(t, 1, n_enc=keys[r])                                                           # the entry from before, cross_stride of n_enc keys
            assert SK._same_bits(s1.logits[0], got[r, t]), (r, t)
        assert torch.equal(s1.tokens[0, :S + 1], st.tokens[r, :S + 1])
    assert not bool(st.finished.any()) and st.outside_untouched()
    full = SK.State(m, S)                                                                        # full counts: the bits of the entry from before
    old = SK.State(m, S)
    for s_ in (full, old):
        s_.tokens[:, 0] = torch.tensor(starts, dtype=torch.int32).to(cuda)
    for t in range(S):
        _steps_len(SK, full, _i32([n_enc] * rows, cuda), t)
        old.run(t, 1)
        assert SK._same_bits(full.logits, old.logits)


def test_softmax_per_row_and_wrapper_refusals(cuda):
    """dyn_softmax_fwd_lens on [3, 2, 5, T] scores (the teacher-forced cross-attention's shape) at T = 17 and 300 against float64, exact zeros
    past a row's count, bit-equal to the scalar entry on the batch entry alone; and what the wrappers refuse of a CUDA `lens`: a wrong
    count, a wrong dtype, a strided view."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd.ops import DynError
    for T in (17, 300):
        x = torch.randn(3, 2, 5, T, generator=K.gen(58000 + T)) * 2
        xd = x.to(cuda)
        for lens in ((T, 1, 9), (T, T - 1, 257), (0, -5, 2)):
            keep = RR.prefix_mask(RR.clamp(lens, T, 1), T)[:, None, None, :]
            ref = lambda t: torch.softmax(t.masked_fill(~keep, float("-inf")), -1) * keep           # noqa: E731
            got = ops.softmax(xd, lens=_i32(lens, cuda))
            tol, e32 = RR.tol(ref(x), ref(x.double()))
            assert K.max_err(got, ref(x.double())) <= tol
            assert (got.cpu()[~keep.expand_as(x)] == 0).all()
            for b in range(3):
                assert torch.equal(got[b:b + 1], ops.softmax(xd[b:b + 1].clone(), valid=_i32([lens[b]], cuda)))
        assert torch.equal(ops.softmax(xd, lens=_i32([T] * 3, cuda)), ops.softmax(xd))
    for bad, word in ((_i32([5, 5], cuda), "2 counts for a batch of 3"), (torch.tensor([5, 5, 5], device=cuda), "int32 CUDA tensor"),
                      (_i32([5, 0, 5, 0, 5, 0], cuda)[::2], "contiguous")):
        with pytest.raises(DynError) as e:
            ops.softmax(xd, lens=bad)
        assert word in str(e.value), str(e.value)
    with pytest.raises(DynError) as e:
        ops.softmax(xd, valid=_i32([5], cuda), lens=_i32([5, 5, 5], cuda))
    assert "not both" in str(e.value)
