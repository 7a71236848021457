"""The chunk entries of csrc/transducer.hip — dyn_tdt_arcs_chunk, dyn_tdt_lattice_run, dyn_tdt_grad_chunk, dyn_joint_bwd_chunk — fed slices of
one logits tensor: every output bit-equal to ops.tdt_loss / ops.joint_bwd on the whole tensor (a row's arithmetic depends on its own logits
and on the lattice state alone: no tolerance), and held to the float64 references of tests/transducer_refs.py by the bars of
tests/test_transducer_kernels_gpu.py (kernel_refs.measured_tol: 4 x the error of torch's own fp32 CPU result + the project's floor).  dp of
the joint backward sums the frames in another order than the whole kernel: held to float64 only, and to equal bits between two runs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import transducer_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 2e-6            # tests/test_transducer_kernels_gpu.py's floors
LOSS_FLOOR = 1e-6
SIGMA = 0.05

# name -> ((T, U), per-row lengths or None, durations, V1)
CASES = {"5x3": ((5, 3), None, R.DURATIONS, 9), "9x5-ragged": ((9, 5), ([9, 7, 4], [5, 0, 3]), R.DURATIONS, 9),
         "70x70": ((70, 70), None, (1, 2), 9), "70x70-d0-4": ((70, 70), None, R.DURATIONS, 9), "40x300": ((40, 300), None, (0, 1), 9),
         "5x3-wide": ((5, 3), None, R.DURATIONS, 1025)}
# (5, 3) with Tc 1 and 2: durations up to 4 span several chunks, the last chunk of Tc = 2 and the one chunk of Tc = 8 overhang the tensor;
# (9, 5) with Tc = 4: one row ends on a chunk boundary (T_b = 4), one inside a chunk (7), whole chunks lie past both; U_b = 0;
# (70, 70) with Tc = 33: an uneven last chunk of 4 frames.  With durations (1, 2) that lattice is INFEASIBLE (every label arc and the
# terminal blank advance the frame: 70 labels need 71 frames): +inf and an all-zero gradient on both paths, its alpha still bit-equal;
# the same shape with durations 0 .. 4 is the feasible one; 5x3-wide: N = 1025 + 5, the row stride loop
GRID = [("5x3", 1), ("5x3", 2), ("5x3", 5), ("5x3", 8), ("9x5-ragged", 1), ("9x5-ragged", 4), ("70x70", 33), ("70x70-d0-4", 33), ("40x300", 16),
        ("5x3-wide", 2)]
F64_GRID = [("5x3", 2), ("9x5-ragged", 4), ("70x70", 33), ("70x70-d0-4", 33), ("40x300", 16), ("5x3-wide", 2)]
_WHOLE = {}


def _check(name, got, t32, want, floor=FLOOR, rel=False):
    """test_transducer_kernels_gpu._check: where torch's logsumexp backward has no result (nan) its error is not counted."""
    want = torch.as_tensor(want, dtype=torch.float64)
    t32 = torch.as_tensor(t32).to(torch.float64)
    tol, e32 = K.measured_tol(torch.where(torch.isnan(t32), want, t32), want, floor, rel)
    err = K.max_err(torch.as_tensor(got), want, rel)
    print(f"{name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _whole(cuda, name):
    """The case's inputs and what ops.tdt_loss makes of the whole tensor (reduction "none", grad_scale 1), computed once and left alone."""
    if name not in _WHOLE:
        from dynamic_asr_eval_amd import ops
        (T, U), lens, durs, V1 = CASES[name]
        B = 1 if lens is None else len(lens[0])
        T_b, U_b = ([T] * B, [U] * B) if lens is None else lens
        x, tg = R.tdt_inputs(B, T, U, V1, len(durs), 1)
        xd, tgd = x.to(cuda), tg.to(cuda)
        il, tl = torch.tensor(T_b, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
        loss, nll, grad = ops.tdt_loss(xd, tgd, il, tl, V1 - 1, durs, SIGMA, "none", 1.0)
        alpha, beta, lp, lse = ops.tdt_lattice(B, T, U + 1, len(durs), cuda)
        _WHOLE[name] = dict(x=x, tg=tg, xd=xd, tgd=tgd, il=il, tl=tl, T_b=T_b, U_b=U_b, B=B, loss=loss, nll=nll, grad=grad, alpha=alpha, beta=beta,
                            lp=lp.clone(), lse=lse.clone())
    return _WHOLE[name]


def _chunked(cuda, w, T, U1, durs, V1, Tc, reduction="none", grad_scale=1.0, sigma=SIGMA, over_logits=False, pad=True):
    """The three passes on slices of w["xd"].  `pad`: every chunk has Tc frames, those past T hold NaN (never read by the arcs pass, exact
    zeros of the gradient pass); else the last chunk is the shorter one.  -> dict like _whole's, the gradient concatenated over chunks."""
    from dynamic_asr_eval_amd import ops
    B, N, D = w["B"], V1 + len(durs), len(durs)
    state = ops.tdt_state(B, T, U1, durs, cuda)
    chunks = []
    for t0 in range(0, T, Tc):
        n = min(Tc, T - t0)
        c = torch.full((B, Tc if pad else n, U1, N), float("nan"), device=cuda)
        c[:, :n] = w["xd"][:, t0:t0 + n]
        chunks.append((t0, n, c))
        ops.tdt_arcs_chunk(c, t0, T, w["tgd"], w["tl"], V1 - 1, durs, state, sigma)
    loss, nll = ops.tdt_lattice_run(B, T, U1, w["tgd"].shape[1], w["il"], w["tl"], durs, state, reduction, want_beta=True)
    alpha, beta, lp, lse = ops.tdt_lattice(B, T, U1, D, cuda, state=state)
    grads = []
    for t0, n, c in chunks:
        g = ops.tdt_grad_chunk(c, t0, T, w["tgd"], w["il"], w["tl"], V1 - 1, durs, state, reduction, grad_scale, out=c if over_logits else None)
        assert (g.data_ptr() == c.data_ptr()) == over_logits
        assert (g[:, n:] == 0).all()                                  # the overhang: exact zeros
        grads.append(g[:, :n])
    return dict(loss=loss, nll=nll, grad=torch.cat(grads, 1), alpha=alpha, beta=beta, lp=lp, lse=lse)


def _assert_equal_bits(got, want, T_b, U_b):
    for k in ("loss", "nll", "grad", "lp", "lse"):
        assert torch.equal(got[k], want[k]), k
    for b in range(len(T_b)):                                         # alpha / beta exist inside the row's lattice only
        for k in ("alpha", "beta"):
            assert torch.equal(got[k][b, :T_b[b], :U_b[b] + 1], want[k][b, :T_b[b], :U_b[b] + 1]), (k, b)


@pytest.mark.parametrize("name,Tc", GRID, ids=[f"{n}-Tc{c}" for n, c in GRID])
def test_chunked_passes_equal_the_whole_lattice_bit_for_bit(cuda, name, Tc):
    """lp, lse, alpha, beta, nll, loss and the concatenated gradient of the chunk entries `torch.equal` those of ops.tdt_loss on the whole
    tensor, over the grid above; rows past the lengths are exact zeros; the gradient written over the chunk's logits and a second run
    give the same bits."""
    (T, U), lens, durs, V1 = CASES[name]
    w = _whole(cuda, name)
    pad = T < 10
    got = _chunked(cuda, w, T, U + 1, durs, V1, Tc, pad=pad)
    _assert_equal_bits(got, w, w["T_b"], w["U_b"])
    for b in range(w["B"]):
        assert (got["grad"][b, w["T_b"][b]:] == 0).all() and (got["grad"][b, :, w["U_b"][b] + 1:] == 0).all()
    assert torch.isfinite(got["grad"]).all()
    if name == "70x70":
        assert torch.isposinf(got["nll"]).all() and torch.isposinf(got["loss"]).all() and (got["grad"] == 0).all()
    else:
        assert torch.isfinite(got["nll"]).all() and got["grad"].abs().max().item() > 0
    again = _chunked(cuda, w, T, U + 1, durs, V1, Tc, over_logits=True, pad=pad)
    _assert_equal_bits(again, got, w["T_b"], w["U_b"])


@pytest.mark.parametrize("reduction", ["sum", "mean_batch", "mean", "mean_volume", "none"])
def test_chunked_reductions_and_grad_scale_equal_the_whole_path(cuda, reduction):
    """Every reduction once, grad_scale 0.5, the lengths of test_tdt_loss_reductions, Tc = 4 (chunks of 4, 4 and 1 frames)."""
    from dynamic_asr_eval_amd import ops
    T_b, U_b, durs, V1 = [9, 6, 9], [5, 5, 2], R.DURATIONS, 9
    x, tg = R.tdt_inputs(3, 9, 5, V1, 5, 4)
    w = dict(B=3, xd=x.to(cuda), tgd=tg.to(cuda), il=torch.tensor(T_b, dtype=torch.int32, device=cuda),
             tl=torch.tensor(U_b, dtype=torch.int32, device=cuda))
    loss, nll, grad = ops.tdt_loss(w["xd"], w["tgd"], w["il"], w["tl"], V1 - 1, durs, 0.0, reduction, 0.5)
    got = _chunked(cuda, w, 9, 6, durs, V1, 4, reduction, 0.5, sigma=0.0, pad=False)
    assert torch.equal(got["loss"], loss) and torch.equal(got["nll"], nll) and torch.equal(got["grad"], grad)
    assert grad.abs().max().item() > 0


def test_chunked_infeasible_lattice_is_inf_with_zero_gradient(cuda):
    """The lattice of test_tdt_loss_infeasible_lattice_is_inf_with_zero_gradient (durations [1, 2], T = 2, U = 4 next to a feasible row)
    chunked at Tc = 1: +inf, an all-zero finite gradient for that row, the whole path's bits for both."""
    from dynamic_asr_eval_amd import ops
    x, tg = R.tdt_inputs(2, 2, 4, 9, 2, 0)
    w = dict(B=2, xd=x.to(cuda), tgd=tg.to(cuda), il=torch.tensor([2, 2], dtype=torch.int32, device=cuda),
             tl=torch.tensor([4, 1], dtype=torch.int32, device=cuda))
    loss, nll, grad = ops.tdt_loss(w["xd"], w["tgd"], w["il"], w["tl"], 8, (1, 2), 0.0, "sum")
    got = _chunked(cuda, w, 2, 5, (1, 2), 9, 1, "sum", sigma=0.0)
    assert torch.isposinf(got["nll"][0]) and torch.isposinf(got["loss"]).all() and torch.isfinite(got["grad"]).all() and (got["grad"][0] == 0).all()
    assert got["grad"][1].abs().max().item() > 0
    assert torch.equal(got["nll"], nll) and torch.equal(got["loss"], loss) and torch.equal(got["grad"], grad)


@pytest.mark.parametrize("name,Tc", F64_GRID, ids=[f"{n}-Tc{c}" for n, c in F64_GRID])
def test_chunked_passes_against_float64(cuda, name, Tc):
    """The chunked outputs against R.tdt_ref in float64 by the rules of test_tdt_loss_lattice_and_gradient_against_float64: nll and loss
    relatively with LOSS_FLOOR, the gradient absolutely, each within 4 x torch's own fp32 error + the floor; alpha / beta where the
    float64 lattice is finite, within 2^-24 * (number of diagonals) * (1 + |value|); the arc log-probs and the two log-sum-exps
    against float64 log_softmax / logsumexp.
    Measured (MI355X), worst over the grid, kernel | torch fp32 | bound: loss (rel) 6.1e-08 | 1.9e-07 | 1.8e-06, grad 2.4e-05 | 7.6e-05 |
    3.1e-04 (at (40, 300); N = 1030: 2.2e-06 | 4.7e-07 | 3.9e-06), blank 8.8e-07 | 8.8e-07 | 5.5e-06, label 6.6e-07 | 7.7e-07 | 5.1e-06."""
    (T, U), lens, durs, V1 = CASES[name]
    w = _whole(cuda, name)
    T_b, U_b, B = w["T_b"], w["U_b"], w["B"]
    want = R.tdt_ref(w["x"], w["tg"], T_b, U_b, V1 - 1, durs, SIGMA, "none")
    nll32, g32 = R.tdt_torch_fp32(w["x"], w["tg"], T_b, U_b, V1 - 1, durs, SIGMA, "none")
    got = {k: v.cpu() for k, v in _chunked(cuda, w, T, U + 1, durs, V1, Tc, pad=T < 10).items()}
    if name == "70x70":                                               # infeasible in float64 as well: +inf, the gradient all zeros
        assert np.isposinf(want["nll"]).all() and torch.isposinf(got["nll"]).all() and torch.isposinf(got["loss"]).all()
        assert not want["grad"].any()
    else:
        assert np.isfinite(want["nll"]).all()
        _check("nll (rel)", got["nll"], nll32, want["nll"], LOSS_FLOOR, rel=True)
        _check("loss (rel)", got["loss"], nll32.sum().reshape(1), np.array([want["nll"].sum()]), LOSS_FLOOR, rel=True)
    _check("grad", got["grad"], g32, want["grad"])
    for b in range(B):
        row = want["rows"][b]
        for k in ("alpha", "beta"):
            have, ref = got[k][b, :T_b[b], :U_b[b] + 1].numpy(), row[k]
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(have), fin), (k, b)
            assert np.abs((have[fin] - ref[fin]) / (1 + np.abs(ref[fin]))).max() <= 2.0 ** -24 * (T_b[b] + U_b[b]), (k, b)
    x64 = w["x"].double()
    for dt in (torch.float64, torch.float32):
        xx = w["x"].to(dt)
        ltok = torch.log_softmax(xx[..., :V1], -1) - SIGMA
        lab = torch.full((B, T, U + 1), -float("inf"), dtype=dt)
        for b in range(B):
            lab[b, :, :U_b[b]] = ltok[b, :, :U_b[b]].gather(-1, w["tg"][b, :U_b[b]].long()[None, :, None].expand(T, -1, 1))[..., 0]
        out = dict(blank=ltok[..., V1 - 1], label=lab, dur=torch.log_softmax(xx[..., V1:], -1),
                   lse_tok=torch.logsumexp(xx[..., :V1], -1), lse_dur=torch.logsumexp(xx[..., V1:], -1))
        if dt == torch.float64:
            ref = out
        else:
            t32 = out
    assert x64.shape[-1] == V1 + len(durs)
    _check("blank", got["lp"][..., 0], t32["blank"], ref["blank"])
    _check("dur", got["lp"][..., 2:], t32["dur"], ref["dur"])
    _check("lse_tok", got["lse"][..., 0], t32["lse_tok"], ref["lse_tok"])
    _check("lse_dur", got["lse"][..., 1], t32["lse_dur"], ref["lse_dur"])
    fin = torch.isfinite(ref["label"])                                # the label arc exists where u < U_b, and nowhere else
    assert torch.equal(torch.isfinite(got["lp"][..., 1]), fin)
    _check("label", got["lp"][..., 1][fin], t32["label"][fin], ref["label"][fin])


@pytest.mark.parametrize("shared", [False, True], ids=["per-row", "shared"])
@pytest.mark.parametrize("Hd", [64, 640])
@pytest.mark.parametrize("Tc", [1, 3])
def test_joint_backward_over_chunks(cuda, Hd, Tc, shared):
    """T = 7 in chunks of 1 and of 3 (3, 3, 1), Hd 64 and 640, p per batch row and one row set shared by the batch: de of every chunk is
    bit-equal to ops.joint_bwd's rows (it sums over u only); dp, accumulated over the chunks in ascending order, is held to float64 by
    measured_tol with the floor of tests/test_transducer_kernels_gpu.py and comes out with equal bits twice, batch-major and
    time-major; de or dp alone give the same bits."""
    from dynamic_asr_eval_amd import ops
    B, T, U1 = 3, 7, 4
    g = K.gen(63000 + Hd + Tc)
    e, p, dz = torch.randn(B, T, Hd, generator=g), torch.randn(1 if shared else B, U1, Hd, generator=g), torch.randn(B, T, U1, Hd, generator=g)
    _, de64, dp64 = R.joint_ref(e.double(), p.double(), dz.double())
    _, de32, dp32 = R.joint_ref(e, p, dz)
    dzd = dz.to(cuda)
    z = ops.joint(e.to(cuda), p.to(cuda))
    de_whole, _ = ops.joint_bwd(dzd, z, p)
    Bp = p.shape[0]

    def run(time_major=False, want_de=True, want_dp=True):
        de = torch.full((B, T, Hd), float("nan"), device=cuda) if want_de else None
        dp = torch.full((U1, Bp, Hd) if time_major else (Bp, U1, Hd), float("nan"), device=cuda) if want_dp else None      # the first chunk overwrites
        for t0 in range(0, T, Tc):
            n = min(Tc, T - t0)
            ops.joint_bwd_chunk(dzd[:, t0:t0 + n].contiguous(), z[:, t0:t0 + n].contiguous(), de, dp, t0, t0 > 0, time_major=time_major)
        return de, dp

    de, dp = run()
    assert torch.equal(de, de_whole)
    _check("de", de.cpu(), de32, de64)
    _check("dp", dp.cpu(), dp32, dp64)
    de2, dp2 = run()
    assert torch.equal(de2, de) and torch.equal(dp2, dp)
    _, dptm = run(time_major=True, want_de=False)
    assert torch.equal(dptm.transpose(0, 1), dp)
    only_e, none = run(want_dp=False)
    assert none is None and torch.equal(only_e, de)
