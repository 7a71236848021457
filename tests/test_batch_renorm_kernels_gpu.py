"""csrc/convmod_brn.hip (dyn_convmod_brn_fwd / dyn_convmod_brn_bwd: the conv-module core with BatchRenorm1d in training mode, reference
nvidia_ctc/lib.py:74,89-102) against float64 references (tests/batch_renorm_refs.py).  Running statistics are built from the reference's own
float64 batch statistics with the factor sets of batch_renorm_refs.calibrated_running, so every case has unclamped, r-clamped (both sides)
and d-clamped (both sides) channels in all combinations.  Bars: kernel_refs.measured_tol (4 x the same formula in torch fp32 on the CPU
against float64, + 2e-6) for s, dc, mu, 1 / sig, r, d and the updated running statistics; kernel_refs.wgrad_tol(5e-4, rows, 531) for dweight
/ dbias (wgrad_tol_ill_conditioned on the offset case); dcbias - wgrad_beta * old exactly zero; rows >= valid exact zeros; two runs equal
bits."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import batch_renorm_refs as BR  # noqa: E402
import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, RMAX, DMAX, NAN, TINY = 1e-5, 3.0, 5.0, float("nan"), 1e-30
NAMES = ("s", "mu", "isig", "r", "d", "running_mean", "running_std")


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _run_case(cuda, shape, KW, valid, seed, momentum=0.001, rmax=RMAX, dmax=DMAX, eps=EPS, ratios=None, beta=1.0):
    """One forward + backward of the core on the device against float64; returns {name: (kernel error, torch fp32 error, bound)}."""
    from dynamic_asr_eval_amd import ops
    B, T, C = shape
    u, w, cbias, weight, bias, ds = BR.core_inputs(shape, KW, seed, ratios)
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    probe = BR.convmod_brn_ref(u, w, cbias, zero, one, weight, bias, eps, rmax, dmax, valid=valid)
    rmean, rstd = BR.calibrated_running(probe["mu"], 1.0 / probe["isig"])
    want = BR.convmod_brn_ref(u, w, cbias, rmean, rstd, weight, bias, eps, rmax, dmax, momentum, valid)
    f = lambda t: t.float()                                                                      # noqa: E731
    t32 = BR.convmod_brn_ref(f(u), f(w), f(cbias), f(rmean), f(rstd), f(weight), f(bias), eps, rmax, dmax, momentum, valid)
    bw64 = BR.convmod_brn_bwd_ref(u, w, cbias, rmean, rstd, weight, bias, ds, eps, rmax, dmax, valid)
    bw32 = BR.convmod_brn_bwd_ref(f(u), f(w), f(cbias), f(rmean), f(rstd), f(weight), f(bias), f(ds), eps, rmax, dmax, valid)
    if rmax > 1.0 and ratios is None:                    # the construction: every clamp state is present
        assert {round(x, 5) for x in want["r"].tolist()} == {round(1 / rmax, 5), 1.0, rmax}
        assert {round(x, 5) for x in want["d"].tolist()} == {-dmax, 0.0, 0.5, dmax}
    dev = lambda t: t.float().to(cuda)                                                           # noqa: E731
    vd = None if valid is None else torch.tensor([valid], dtype=torch.int32, device=cuda)
    v = T if valid is None else valid
    g = K.gen(seed + 1)
    old = [torch.randn(C, generator=g) for _ in range(3)]
    runs = []
    for _ in range(2):
        rm, rs = dev(rmean), dev(rstd)
        s, gl, c, stats = ops.convmod_brn(dev(u), dev(w), dev(cbias), rm, rs, dev(weight), dev(bias), rmax, dmax, momentum, "silu", eps, valid=vd)
        acc = [o.to(cuda) if beta else torch.full_like(o, NAN).to(cuda) for o in old]
        dsd = dev(ds)
        dc = ops.convmod_brn_bwd(c, stats, dsd, *acc, "silu", valid=vd, wgrad_beta=beta)
        over = dsd.clone()
        assert ops.convmod_brn_bwd(c, stats, over, None, None, None, valid=vd, out=over) is over and _bits_equal(over, dc)   # dc over ds; frozen sums
        runs.append([s, gl, c, stats, rm, rs, dc] + acc)
    for a, b in zip(*runs):
        assert _bits_equal(a, b), "two runs differ"
    s, gl, c, stats, rm, rs, dc, dw, db, dcb = runs[0]
    assert stats.shape == (7, C)
    if v < T:
        for t in (s, gl, c, dc):
            assert t[:, v:].abs().max().item() == 0.0
    if momentum == 0.0:
        assert _bits_equal(rm, rmean.float()) and _bits_equal(rs, rstd.float())
    got = dict(s=s, mu=stats[0], isig=stats[1], r=stats[2], d=stats[3], running_mean=rm, running_std=rs)
    out = {}
    for name in NAMES:
        tol, e32 = K.measured_tol(t32[name], want[name], 2e-6)
        out[name] = (K.max_err(got[name], want[name]), e32, tol)
    for name in ("gl", "c"):
        tol, e32 = K.measured_tol(t32[name], want[name], 2e-6)
        out[name] = (K.max_err(dict(gl=gl, c=c)[name], want[name]), e32, tol)
    tol, e32 = K.measured_tol(bw32[0], bw64[0], 2e-6)
    out["dc"] = (K.max_err(dc, bw64[0]), e32, tol)
    rows = B * v
    sums_tol = K.wgrad_tol_ill_conditioned(5e-4, rows) if ratios is not None else K.wgrad_tol(5e-4, rows, 531)
    out["dweight"] = (K.max_err(dw, bw64[1] + beta * old[0].double()), 0.0, sums_tol)
    out["dbias"] = (K.max_err(db, bw64[2] + beta * old[1].double()), 0.0, sums_tol)
    keep = beta * old[2] if beta else torch.zeros(C)
    out["dcbias"] = ((dcb.cpu() - keep).abs().max().item(), 0.0, 0.0)
    assert bw64[3].abs().max().item() < 1e-11                      # the float64 autograd gradient of the convolution bias: rounding only
    for name, (err, e32, tol) in out.items():
        print(f"  {shape} KW {KW} valid {valid} {name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    for name, (err, e32, tol) in out.items():
        assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"
    return out


@pytest.mark.parametrize("shape,KW,valid", [((3, 37, 256), 9, None), ((2, 37, 512), 9, 29), ((2, 37, 512), 9, 16), ((2, 70, 256), 32, 45),
                                            ((1, 5, 256), 9, None), ((5, 40, 1024), 9, None)],
                         ids=["tail-tile", "valid-29", "valid-16-two-empty-tiles", "32-taps-masked", "shorter-than-halo", "loop-batch-1024"])
def test_core_against_float64(cuda, shape, KW, valid):
    """[3, 37, 256]: a tail tile of 5 frames; [2, 37, 512] valid 29: a partly masked tile, valid 16: two tiles of count 0 (skipped by the
    combine); [2, 70, 256] 32 taps, valid 45: masked tiles at the 32-frame tile; [1, 5, 256]: shorter than the halo, 5 rows in all;
    [5, 40, 1024]: the loop's batch, four channel blocks.
    Worst measured kernel | torch fp32 | bound over the six cases (MI355X):
      s 3.4e-06 | 3.5e-06 | 1.6e-05   mu 6.5e-08 | 4.7e-08 | 2.2e-06   1 / sig 3.1e-06 | 3.3e-06 | 1.5e-05 (the 5-row case; else 5.9e-07)
      r 2.6e-07 | 2.2e-07 | 2.9e-06   d 3.7e-07 | 3.7e-07 | 3.5e-06   running_mean 9.5e-07 | 9.5e-07 | 5.8e-06   running_std 1.3e-07 | 1.3e-07 | 2.5e-06
      gl 3.1e-07 | 3.1e-07 | 3.2e-06   c 6.8e-07 | 5.0e-07 | 4.0e-06   dc 2.4e-05 | 2.4e-05 | 9.7e-05
      dweight 1.4e-04, dbias 2.4e-05 | bound 5.0e-04 (the loop's batch; the other cases at most 4.5e-05 / 1.1e-05); dcbias - old exactly 0."""
    _run_case(cuda, shape, KW, valid, seed=41000 + shape[1] + shape[2] + (valid or 0))


def test_offset_channels(cuda):
    """[3, 37, 256] with cbias moving a third of the channels each to mean / std = 30, 100 and 1000: an uncentred accumulation
    (E[x^2] - E[x]^2 in fp32) loses the deviation entirely at 1000 and fails 1 / sig; dweight takes wgrad_tol_ill_conditioned, for the
    reason its docstring gives (mu reaches the backward as an fp32 value).
    Measured kernel | torch fp32 | bound (MI355X): s 9.9e-04 | 1.1e-03 | 4.4e-03, mu 9.7e-05 | 8.9e-05 | 3.6e-04, 1 / sig 6.7e-05 | 6.4e-05 | 2.6e-04,
    r 2.9e-05 | 1.8e-05 | 7.3e-05, d 5.5e-04 | 4.8e-04 | 1.9e-03, c 1.9e-04 | 1.9e-04 | 7.5e-04 (one ulp of a value 1000 deviations from zero),
    dc 5.0e-03 | 5.9e-03 | 2.4e-02; dweight 5.1e-03, dbias 1.7e-03 | bound 5.3e-03.  The results are bit-reproducible, so dweight's 3 per cent
    of room is the same on every run."""
    _run_case(cuda, (3, 37, 256), 9, None, seed=42000, ratios=K.COLNORM_RATIOS)


def test_plain_batch_norm_limit(cuda):
    """rmax = 1, dmax = 0 (num_batches_tracked = 0): r = 1, d = 0, plain training-mode batch norm.  Checked against the float64 reference as every
    case, and, where the two eps placements (std + eps against sqrt(var + eps)) coincide, the core at eps = 0 against
    torch.nn.functional.batch_norm(training=True, eps=1e-30: it refuses 0) on the reference's convolution output.
    Measured kernel | torch fp32 | bound (MI355X): s 9.3e-07 | 8.8e-07 | 5.5e-06, r and d exact, dc 1.7e-06 | 1.9e-06 | 9.7e-06, dweight 7.3e-06,
    dbias 4.6e-06 | 5.0e-04; against F.batch_norm 8.9e-07 | 9.6e-07 | 5.8e-06."""
    from dynamic_asr_eval_amd import ops
    assert ops.batch_renorm_clamps(0) == (1.0, 0.0)
    shape, KW = (3, 37, 256), 9
    out = _run_case(cuda, shape, KW, None, seed=43000, rmax=1.0, dmax=0.0)
    assert out["r"][0] == 0.0 and out["d"][0] == 0.0
    u, w, cbias, weight, bias, _ = BR.core_inputs(shape, KW, 43000)
    C = shape[2]
    ref = BR.convmod_brn_ref(u, w, cbias, torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), weight, bias, 0.0, 1.0, 0.0)
    bn = F.silu(F.batch_norm(ref["c"].transpose(1, 2), None, None, weight, bias, training=True, eps=TINY).transpose(1, 2))
    assert K.max_err(ref["s"], bn) < 1e-12
    dev = lambda t: t.float().to(cuda)                                                           # noqa: E731
    s, _, _, _ = ops.convmod_brn(dev(u), dev(w), dev(cbias), torch.zeros(C, device=cuda), torch.ones(C, device=cuda), dev(weight), dev(bias), 1.0, 0.0,
                                 0.0, "silu", 0.0)
    t32 = F.silu(F.batch_norm(ref["c"].float().transpose(1, 2), None, None, weight.float(), bias.float(), training=True, eps=TINY).transpose(1, 2))
    tol, e32 = K.measured_tol(t32, bn, 2e-6)
    err = K.max_err(s, bn)
    print(f"  against F.batch_norm(training=True): kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol


@pytest.mark.parametrize("momentum", [0.0, 0.1])
def test_momentum(cuda, momentum):
    """momentum = 0: the running statistics keep their bits (asserted in _run_case); 0.1: they move by a tenth of the way, within measured_tol.
    wgrad_beta = 0 here: NaN-filled gradient buffers are overwritten, dcbias becomes exact zeros.
    Measured kernel | torch fp32 | bound at momentum 0.1 (MI355X): running_mean 1.0e-06 | 1.0e-06 | 6.2e-06, running_std 1.2e-07 | 1.3e-07 | 2.5e-06."""
    _run_case(cuda, (2, 37, 512), 9, 29, seed=44000, momentum=momentum, beta=0.0)


def test_refusals(cuda):
    """Every refusal of the header, before any launch: another C or KW or act DYN_E_UNSUPPORTED (-4); null pointers, rmax < 1, dmax < 0,
    momentum outside [0, 1], B * T < 2 DYN_E_ARG (-1); a short workspace DYN_E_WORKSPACE (-3); and the wrappers' own operand checks."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import load
    from dynamic_asr_eval_amd.ops import DynError
    L = load()
    B, T, C, KW = 2, 8, 256, 9
    z = lambda *s: torch.zeros(*s, device=cuda)                                                  # noqa: E731
    u = torch.randn(B, T, 2 * C, generator=K.gen(45000)).to(cuda)
    w, cb, rm, rs, wt, bs = torch.ones(C, 32, device=cuda), z(C), z(C), torch.ones(C, device=cuda), torch.ones(C, device=cuda), z(C)
    s, gl, c, stats = z(B, T, C), z(B, T, C), z(B, T, C), z(7, C)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()                                                                 # noqa: E731

    def fwd(B=B, T=T, C=C, KW=KW, act=0, eps=EPS, rmax=RMAX, dmax=DMAX, mom=0.001, null=None, wsb=ws.numel()):
        a = [u, w, cb, rm, rs, wt, bs, s, gl, c, stats]
        p = [None if k == null else ptr(t) for k, t in enumerate(a)]
        return L.dyn_convmod_brn_fwd(*p, None, B, T, C, KW, act, eps, rmax, dmax, mom, ptr(ws), wsb, st)

    def bwd(B=B, T=T, C=C, act=0, null=None, wsb=ws.numel()):
        a = [c, stats, s, gl]
        p = [None if k == null else ptr(t) for k, t in enumerate(a)]
        return L.dyn_convmod_brn_bwd(*p, None, None, None, 1.0, None, B, T, C, act, ptr(ws), wsb, st)

    assert fwd() == 0 and bwd() == 0
    assert fwd(C=128) == -4 and fwd(C=1280) == -4 and fwd(KW=7) == -4 and fwd(KW=31) == -4 and fwd(act=1) == -4
    assert bwd(C=128) == -4 and bwd(act=1) == -4
    for null in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10):                   # cbias (2) may be null
        assert fwd(null=null) == -1, null
    assert fwd(null=2) == 0
    for null in range(4):
        assert bwd(null=null) == -1, null
    assert fwd(rmax=0.99) == -1 and fwd(dmax=-0.1) == -1 and fwd(mom=-0.1) == -1 and fwd(mom=1.5) == -1
    assert fwd(B=1, T=1) == -1 and bwd(B=1, T=1) == -1 and fwd(B=0) == -1 and fwd(B=1, T=2) == 0
    need = L.dyn_convmod_brn_fwd_workspace_bytes(B, T, C, KW)
    assert need == 3 * B * 1 * C * 4 and L.dyn_convmod_brn_fwd_workspace_bytes(B, 33, C, 32) == 3 * B * 2 * C * 4
    assert fwd(wsb=need - 1) == -3 and fwd(wsb=need) == 0
    need = L.dyn_convmod_brn_bwd_workspace_bytes(B, T, C)
    assert need == (2 * B * T + 2) * C * 4 and L.dyn_convmod_brn_bwd_workspace_bytes(5, 2048, C) == (2 * 512 + 2) * C * 4
    assert bwd(wsb=need - 1) == -3 and bwd(wsb=need) == 0
    assert L.dyn_convmod_brn_stats_rows() == 7
    torch.cuda.synchronize()
    w9 = z(C, 9)
    with pytest.raises(DynError):
        ops.convmod_brn(u, w9, None, rm, rs, wt, bs, RMAX, DMAX, 0.001, act="gelu")
    with pytest.raises(DynError):
        ops.convmod_brn(u, z(C, 7), None, rm, rs, wt, bs, RMAX, DMAX, 0.001)
    with pytest.raises(DynError):
        ops.convmod_brn(u, w9, None, rm[:128], rs, wt, bs, RMAX, DMAX, 0.001)
    with pytest.raises(DynError):
        ops.convmod_brn(u, w9, z(128), rm, rs, wt, bs, RMAX, DMAX, 0.001)
    with pytest.raises(DynError):
        ops.convmod_brn_bwd(c, stats, s[:, :2], None, None, None)
    with pytest.raises(DynError):
        ops.convmod_brn_bwd(c, stats[:6], s, None, None, None)
    with pytest.raises(DynError):
        ops.convmod_brn_bwd(c, stats, s, z(128), None, None)
