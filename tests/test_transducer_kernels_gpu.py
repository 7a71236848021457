"""The kernels of csrc/transducer.hip — LSTM cell forward / backward, joint input forward / backward, TDT arc log-probs, lattice, loss and
gradient — against float64 references (tests/transducer_refs.py).  Bars: kernel_refs.measured_tol, 4 x the error of torch's own fp32 CPU
result on the same inputs + 2e-6 (the floor of the project's activations and data gradients) or, for a loss, the same rule on the relative
error + 1e-6 (the project's floor for losses); for the TDT loss and its gradient the torch fp32 result is transformers' tdt_loss with autograd; kernel_refs.wgrad_tol (5e-4 at 531 summed rows) for the weight sums."""
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

FLOOR = 2e-6
LOSS_FLOOR = 1e-6       # losses are compared RELATIVELY with this floor, as tests/test_kernel_parity_f64_gpu.py::test_nll_loss_and_its_weighted_form
#                         does: an NLL of 194 has an fp32 spacing of 1.5e-5, no absolute floor of 2e-6 can be met by an fp32 output there


def _check(name, got, t32, want, floor=FLOOR, rel=False):
    """torch's logsumexp backward is nan at lattice cells no path reaches (a duration list without 0, u > t): where torch has no result
    its error is not counted (the kernel's is, everywhere)."""
    want = torch.as_tensor(want, dtype=torch.float64)
    t32 = torch.as_tensor(t32).to(torch.float64)
    tol, e32 = K.measured_tol(torch.where(torch.isnan(t32), want, t32), want, floor, rel)
    err = K.max_err(torch.as_tensor(got), want, rel)
    print(f"{name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"
    return err, e32, tol


# (T, U), per-row lengths or None, durations, V1
LATTICE = [((1, 0), None, R.DURATIONS, 9), ((1, 1), None, R.DURATIONS, 9), ((2, 0), None, (1, 2), 9), ((5, 3), None, R.DURATIONS, 9),
           ((5, 3), None, (0, 1), 9), ((9, 5), ([9, 7, 4], [5, 0, 3]), R.DURATIONS, 9), ((9, 5), ([9, 6, 9], [5, 5, 2]), (1, 2), 9),
           ((70, 70), None, R.DURATIONS, 9), ((90, 70), None, (1, 2), 9), ((300, 40), None, R.DURATIONS, 9), ((40, 300), None, (0, 1), 9),
           ((260, 260), None, R.DURATIONS, 9)]


@pytest.mark.parametrize("shape,lens,durs,V1", LATTICE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and v and isinstance(v[0], int) else "")
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_tdt_loss_lattice_and_gradient_against_float64(cuda, shape, lens, durs, V1, sigma):
    """Per-row NLL, alpha, beta, the compact arc log-probs and the gradient of the summed loss at (T, U) = (1, 0), (1, 1), (2, 0), (5, 3),
    (9, 5) with ragged rows (U_b = 0 among them), (70, 70) (a diagonal longer than a wave), (300, 40) and (40, 300) (340 diagonals, the
    longest lattices), (260, 260) (a diagonal longer than the workgroup's 256 threads: the stride loop), durations [0..4], [1, 2],
    [0, 1], sigma 0 and 0.05.  Rows past the lengths are exact zeros, a second run gives equal bits, the gradient may be written over the logits,
    grad_scale scales it.  alpha / beta are compared where the float64 lattice is finite, within 2^-24 * (number of diagonals) * (1 + |value|):
    one fp32 rounding per diagonal, taken to add up linearly (the worst case).
    Measured (MI355X), worst over the grid, kernel | torch fp32 | bound: nll (rel) 1.1e-07 | 1.8e-07 | 1.7e-06, loss (rel) 9.0e-08 | 4.7e-07 |
    2.9e-06, grad 5.2e-05 | 2.2e-04 | 8.9e-04 (at (40, 300); (70, 70): 9.7e-06 | 1.3e-05 | 5.2e-05; (5, 3): 6.9e-07 | 3.8e-07 | 3.5e-06)."""
    from dynamic_asr_eval_amd import ops
    (T, U), D = shape, len(durs)
    B = 1 if lens is None else len(lens[0])
    T_b, U_b = ([T] * B, [U] * B) if lens is None else lens
    x, tg = R.tdt_inputs(B, T, U, V1, D, 1)
    want = R.tdt_ref(x, tg, T_b, U_b, V1 - 1, durs, sigma, "none")
    nll32, g32 = R.tdt_torch_fp32(x, tg, T_b, U_b, V1 - 1, durs, sigma, "none")
    assert np.isfinite(want["nll"]).all()
    xd, tgd = x.to(cuda), tg.to(cuda)
    il, tl = torch.tensor(T_b, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
    loss, nll, grad = ops.tdt_loss(xd, tgd, il, tl, V1 - 1, durs, sigma, "none", 1.0)
    alpha, beta, lp, lse = (t.cpu() for t in ops.tdt_lattice(B, T, U + 1, D, cuda))
    _check("nll (rel)", nll.cpu(), nll32, want["nll"], LOSS_FLOOR, rel=True)
    _check("loss (rel)", loss.cpu(), nll32.sum().reshape(1), np.array([want["nll"].sum()]), LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), g32, want["grad"])
    for b in range(B):
        row = want["rows"][b]
        for name, got, ref in (("alpha", alpha, row["alpha"]), ("beta", beta, row["beta"])):
            got = got[b, :T_b[b], :U_b[b] + 1].numpy()
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin), (name, b)
            assert np.abs((got[fin] - ref[fin]) / (1 + np.abs(ref[fin]))).max() <= 2.0 ** -24 * (T_b[b] + U_b[b]), (name, b)
        assert (grad[b, T_b[b]:] == 0).all() and (grad[b, :, U_b[b] + 1:] == 0).all()
    loss2, nll2, grad2 = ops.tdt_loss(xd, tgd, il, tl, V1 - 1, durs, sigma, "none", 1.0)
    assert torch.equal(grad2, grad) and torch.equal(nll2, nll)
    xin = xd.clone()
    _, _, over = ops.tdt_loss(xin, tgd, il, tl, V1 - 1, durs, sigma, "sum", 0.25, out=xin)
    assert over.data_ptr() == xin.data_ptr() and torch.equal(over, grad * 0.25)
    _, nll3, none = ops.tdt_loss(xd, tgd, il, tl, V1 - 1, durs, sigma, "sum", want_grad=False)
    assert none is None and torch.equal(nll3, nll)


@pytest.mark.parametrize("reduction", ["sum", "mean_batch", "mean", "mean_volume"])
def test_tdt_loss_reductions(cuda, reduction):
    from dynamic_asr_eval_amd import ops
    T_b, U_b, durs, V1 = [9, 6, 9], [5, 5, 2], R.DURATIONS, 9
    x, tg = R.tdt_inputs(3, 9, 5, V1, 5, 4)
    want = R.tdt_ref(x, tg, T_b, U_b, V1 - 1, durs, 0.0, reduction, grad_scale=0.5)
    l32, g32 = R.tdt_torch_fp32(x, tg, T_b, U_b, V1 - 1, durs, 0.0, reduction)
    il, tl = torch.tensor(T_b, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
    loss, _, grad = ops.tdt_loss(x.to(cuda), tg.to(cuda), il, tl, V1 - 1, durs, 0.0, reduction, 0.5)
    _check("loss (rel)", loss.cpu(), l32.reshape(1), np.array([want["loss"]]), LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), g32 * 0.5, want["grad"])


def test_tdt_loss_infeasible_lattice_is_inf_with_zero_gradient(cuda):
    """durations [1, 2], T = 2, U = 4: no path emits four labels in two frames.  The loss is +inf and the gradient all zeros, finite; a
    feasible row next to it keeps its own loss and gradient."""
    from dynamic_asr_eval_amd import ops
    x, tg = R.tdt_inputs(2, 2, 4, 9, 2, 0)
    T_b, U_b = [2, 2], [4, 1]
    want = R.tdt_ref(x, tg, T_b, U_b, 8, (1, 2), 0.0, "none")
    assert np.isposinf(want["nll"][0]) and np.isfinite(want["nll"][1])
    il, tl = torch.tensor(T_b, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
    loss, nll, grad = ops.tdt_loss(x.to(cuda), tg.to(cuda), il, tl, 8, (1, 2), 0.0, "sum")
    assert torch.isposinf(nll[0]) and torch.isposinf(loss).all() and torch.isfinite(grad).all() and (grad[0] == 0).all()
    assert abs(float(nll[1]) - want["nll"][1]) < 1e-5 and np.abs(grad[1].cpu().numpy() - want["grad"][1]).max() < 1e-5
    assert grad[1].abs().max().item() > 0


@pytest.mark.parametrize("N", [6, 38, 64 + 5, 1025 + 5])
def test_tdt_arc_log_probs_against_float64(cuda, N):
    """Row widths V + 1 + D = 6, 38 (below a wave), 69 (just above) and 1030 (the stride loop), D = 5 (6: D = 2): blank, label and
    duration log-probs and the two log-sum-exps of every row, labels only where u < U_b (-inf elsewhere), sigma off the token part only.
    Measured (MI355X), worst over the four widths, kernel | torch fp32 | bound: blank 2.2e-06 | 2.1e-06 | 1.0e-05, label 1.0e-06 | 1.0e-06 |
    6.1e-06, dur 7.7e-07 | 8.1e-07 | 5.2e-06, lse_tok 5.4e-07 | 5.2e-07 | 4.1e-06, lse_dur 4.6e-07 | 4.6e-07 | 3.8e-06."""
    from dynamic_asr_eval_amd import ops
    D = 2 if N == 6 else 5
    durs, V1, B, T, U, sigma = tuple(range(D)) if D == 5 else (1, 2), N - D, 2, 3, 4, 0.05
    x, tg = R.tdt_inputs(B, T, U, V1, D, 9, scale=3.0)
    U_b = [4, 2]
    il, tl = torch.full((B,), T, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
    ops.tdt_loss(x.to(cuda), tg.to(cuda), il, tl, V1 - 1, durs, sigma, "sum", want_grad=False)
    _, _, lp, lse = (t.cpu() for t in ops.tdt_lattice(B, T, U + 1, D, cuda))
    x64 = x.double()
    for dt, store in ((torch.float64, "want"), (torch.float32, "t32")):
        xx = x.to(dt)
        ltok, ldur = torch.log_softmax(xx[..., :V1], -1) - sigma, torch.log_softmax(xx[..., V1:], -1)
        lab = torch.full((B, T, U + 1), -float("inf"), dtype=dt)
        for b in range(B):
            lab[b, :, :U_b[b]] = ltok[b, :, :U_b[b]].gather(-1, tg[b, :U_b[b]].long()[None, :, None].expand(T, -1, 1))[..., 0]
        out = dict(blank=ltok[..., V1 - 1], label=lab, dur=ldur, lse_tok=torch.logsumexp(xx[..., :V1], -1), lse_dur=torch.logsumexp(xx[..., V1:], -1))
        if store == "want":
            want = out
        else:
            t32 = out
    assert x64.shape[-1] == N
    fin = torch.isfinite(want["label"])
    assert torch.equal(torch.isfinite(lp[..., 1]), fin)
    _check("blank", lp[..., 0], t32["blank"], want["blank"])
    _check("label", lp[..., 1][fin], t32["label"][fin], want["label"][fin])
    _check("dur", lp[..., 2:], t32["dur"], want["dur"])
    _check("lse_tok", lse[..., 0], t32["lse_tok"], want["lse_tok"])
    _check("lse_dur", lse[..., 1], t32["lse_dur"], want["lse_dur"])


@pytest.mark.parametrize("shared", [False, True], ids=["per-row", "shared"])
@pytest.mark.parametrize("Hd,U1", [(64, 1), (64, 4), (640, 1), (640, 3)])
def test_joint_forward_and_backward_against_float64(cuda, Hd, U1, shared):
    """z = relu(e + p) and its two sums at Hd 64 and 640, U + 1 = 1 and more, p per batch row and one row set shared by the batch (dp then
    sums over b as well), batch-major and time-major dp.  The forward is one rounding: bit-equal to torch's fp32.
    Measured (MI355X), worst, kernel | torch fp32 | bound: de 4.8e-07 | 4.8e-07 | 3.9e-06, dp 1.4e-06 | 1.4e-06 | 7.7e-06."""
    from dynamic_asr_eval_amd import ops
    B, T = 3, 5
    g = K.gen(61000 + Hd + U1)
    e, p, dz = torch.randn(B, T, Hd, generator=g), torch.randn(1 if shared else B, U1, Hd, generator=g), torch.randn(B, T, U1, Hd, generator=g)
    z64, de64, dp64 = R.joint_ref(e.double(), p.double(), dz.double())
    z32, de32, dp32 = R.joint_ref(e, p, dz)
    z = ops.joint(e.to(cuda), p.to(cuda))
    assert torch.equal(z.cpu(), z32)
    ptm = p.transpose(0, 1).contiguous().to(cuda)                                # [U1, Bp, Hd]: the layout the model keeps
    assert torch.equal(ops.joint(e.to(cuda), ptm.transpose(0, 1)), z)
    de, dp = ops.joint_bwd(dz.to(cuda), z, p)
    _check("de", de.cpu(), de32, de64)
    _check("dp", dp.cpu(), dp32, dp64)
    de2, dptm = ops.joint_bwd(dz.to(cuda), z, p, time_major=True)
    assert torch.equal(de2, de) and torch.equal(dptm.transpose(0, 1), dp)
    only_e, none = ops.joint_bwd(dz.to(cuda), z, p, want_dp=False)
    assert none is None and torch.equal(only_e, de)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("U1", [1, 7])
def test_lstm_cells_against_torch_lstm_in_float64(cuda, layers, U1):
    """The teacher-forced LSTM assembled as the model does it (one GEMM for the input half of all steps, one per step for the recurrent
    half, ops.lstm_cell; backward ops.lstm_cell_bwd, ops.linear_dgrad, one weight-gradient product per matrix) against torch.nn.LSTM in
    float64, 1 and 2 layers, 1 and 7 steps: outputs and the data gradient within measured_tol, weight and bias gradients within wgrad_tol.
    Measured (MI355X), worst, kernel | torch fp32 | bound: y 5.3e-07 | 4.3e-07 | 3.7e-06, dx 1.1e-06 | 1.2e-06 | 7.0e-06; dw_ih 2.8e-06,
    dw_hh 7.9e-07, db 1.9e-06 | bound 5.0e-04."""
    from dynamic_asr_eval_amd import ops
    Bd, Hd = 3, 64
    g = K.gen(62000 + layers + U1)
    x = torch.randn(Bd, U1, Hd, generator=g)
    ws = [tuple(torch.randn(*s, generator=g) * 0.3 for s in ((4 * Hd, Hd), (4 * Hd, Hd), (4 * Hd,), (4 * Hd,))) for _ in range(layers)]
    dy = torch.randn(Bd, U1, Hd, generator=g)
    y64, g64, dx64 = R.lstm_ref(x, ws, dy)
    y32, g32, dx32 = R.lstm_ref(x, ws, dy, dtype=torch.float32)
    wd = [tuple(w.to(cuda) for w in l) for l in ws]
    inp = x.transpose(0, 1).contiguous().to(cuda)                                # time-major [U1, Bd, Hd]
    kept = []
    zeros = torch.zeros(Bd, Hd, device=cuda)
    for w_ih, w_hh, b_ih, b_hh in wd:
        xg = ops.linear(inp.view(U1 * Bd, Hd), w_ih, b_ih).view(U1, Bd, 4 * Hd)
        h_all, c_all, g_all = torch.empty(U1, Bd, Hd, device=cuda), torch.empty(U1, Bd, Hd, device=cuda), torch.empty(U1, Bd, 4 * Hd, device=cuda)
        for u in range(U1):
            ops.lstm_cell(xg[u], ops.linear(h_all[u - 1] if u else zeros, w_hh, b_hh), c_all[u - 1] if u else None, out=(c_all[u], h_all[u], g_all[u]))
        kept.append((inp, h_all, c_all, g_all))
        inp = h_all
    _check("y", inp.transpose(0, 1).cpu(), y32, y64)
    c1, h1, _ = ops.lstm_cell(xg[0], ops.linear(zeros, w_hh, b_hh))              # the allocating form, nothing saved
    assert torch.equal(h1, kept[-1][1][0]) and torch.equal(c1, kept[-1][2][0])
    d = dy.transpose(0, 1).contiguous().to(cuda)
    for k in reversed(range(layers)):
        xin, h_all, c_all, g_all = kept[k]
        w_ih, w_hh = wd[k][0], wd[k][1]
        dg_all = torch.empty_like(g_all)
        dc = None
        for u in reversed(range(U1)):
            _, dc = ops.lstm_cell_bwd(d[u], dc, g_all[u], c_all[u - 1] if u else None, c_all[u], dgates=dg_all[u])
            if u:
                ops.linear_dgrad(dg_all[u], w_hh, out=d[u - 1], beta=1.0)
        dg = dg_all.view(U1 * Bd, 4 * Hd)
        dw_ih, dw_hh, db = torch.zeros_like(w_ih), torch.zeros_like(w_hh), torch.zeros(4 * Hd, device=cuda)
        ops.linear_wgrad(dg, xin.view(U1 * Bd, Hd), dw_ih, beta=0.0)
        if U1 > 1:
            ops.linear_wgrad(dg_all[1:].reshape(-1, 4 * Hd), h_all[:-1].reshape(-1, Hd), dw_hh, beta=0.0)
        ops.colsum(dg, db, beta=0.0)
        tol = K.wgrad_tol(5e-4, U1 * Bd, 531)
        for name, got, want in (("dw_ih", dw_ih, g64[k][0]), ("dw_hh", dw_hh, g64[k][1]), ("db_ih", db, g64[k][2]), ("db_hh", db, g64[k][3])):
            err = K.max_err(got.cpu(), want)
            print(f"layer {k} {name}: {err:.2e} | bound {tol:.2e}")
            assert err <= tol, (k, name, err)
        d = ops.linear_dgrad(dg, w_ih).view(U1, Bd, Hd)
    _check("dx", d.transpose(0, 1).cpu(), dx32, dx64)
