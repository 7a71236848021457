"""The RNN-T kernels of csrc/transducer.hip — arc log-probs, lattice, loss, gradient, their chunk forms and the greedy steps — against the
float64 references of tests/rnnt_refs.py.  Bars: kernel_refs.measured_tol, 4 x the error of the torch fp32 CPU result on the same inputs +
2e-6 (gradients, log-probs) or, for a loss, the same rule on the relative error + 1e-6.  transformers' rnnt_loss cannot run without
torchaudio: the torch fp32 result is the torch recursion of rnnt_refs (log_softmax + the (t, u) double loop with logsumexp, autograd) in
float32."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import rnnt_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
LOSS_FLOOR = 1e-6
_REFS = {}


def _check(name, got, t32, want, floor=FLOOR, rel=False):
    want = torch.as_tensor(want, dtype=torch.float64)
    t32 = torch.as_tensor(t32).to(torch.float64)
    tol, e32 = K.measured_tol(torch.where(torch.isnan(t32), want, t32), want, floor, rel)
    err = K.max_err(torch.as_tensor(got), want, rel)
    print(f"{name}: kernel {err:.2e} | torch fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"
    return err, e32, tol


def _lens(B, T, U):
    """Ragged per-row lengths: the first row full, the others shorter (never T_b = 0 here)."""
    return [max(1, T - 3 * b) for b in range(B)], [max(0, U - 2 * b) for b in range(B)]


def _case(B, T, U, V1, scale=1.0, restated32=False):
    """Inputs and the float64 / torch fp32 per-row results of one shape: computed once on the CPU, shared by the tests, left alone.
    `restated32`: the fp32 result is the restatement run in float32 (rnnt_refs.rnnt_row's dtype argument) instead of the torch recursion,
    whose Python double loop with autograd takes 40 s at 90000 cells."""
    key = (B, T, U, V1, scale)
    if key not in _REFS:
        x, tg, blank = R.rnnt_inputs(B, T, U, V1, 1, scale)
        T_b, U_b = _lens(B, T, U)
        want = R.rnnt_ref(x, tg, T_b, U_b, blank, "none")
        if restated32:
            w32 = R.rnnt_ref(x, tg, T_b, U_b, blank, "none", dtype=np.float32)
            nll32, g32 = torch.as_tensor(w32["nll"]), torch.as_tensor(w32["grad"])
        else:
            nll32, g32 = R.rnnt_torch(x, tg, T_b, U_b, blank, "none")
        _REFS[key] = dict(x=x, tg=tg, blank=blank, T_b=T_b, U_b=U_b, want=want, nll32=nll32, g32=g32)
    return _REFS[key]


def _dev(c, cuda):
    il = torch.tensor(c["T_b"], dtype=torch.int32, device=cuda)
    tl = torch.tensor(c["U_b"], dtype=torch.int32, device=cuda)
    return c["x"].to(cuda), c["tg"].to(cuda), il, tl


SHAPES = [(1, 1, 0), (2, 1, 3), (2, 7, 0), (3, 33, 5), (2, 70, 40)]


@pytest.mark.parametrize("V1", [5, 64, 65, 130])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rnnt_loss_lattice_and_gradient_against_float64(cuda, shape, V1):
    """Per-row NLL, the summed loss, alpha, beta, the arc log-probs and the gradient at (B, T, U) = (1, 1, 0), (2, 1, 3), (2, 7, 0),
    (3, 33, 5), (2, 70, 40) with ragged T_b / U_b, V1 = 5 (a row narrower than a wave), 64 (one wave), 65 (one over), 130 (more than two
    strides); the blank is class V1 - 2, not the last.  Rows past the lengths are exact zeros, a second run gives equal bits, the gradient
    may be written over the logits and grad_scale scales it.  alpha / beta are compared where the float64 lattice is finite, within
    2^-24 * (T_b + U_b) * (1 + |value|): one fp32 rounding per diagonal, taken to add up linearly.
    Measured (MI355X), worst over the grid, kernel | torch fp32 | bound: nll (rel) 8.6e-08 | 2.5e-08 | 1.1e-06, loss (rel) 7.0e-08 |
    5.4e-09 | 1.0e-06, grad 3.2e-05 | 1.2e-04 | 4.8e-04 (at (2, 70, 40), V1 = 130; (3, 33, 5), V1 = 65: 2.5e-06 | 9.3e-06 | 3.9e-05), blank
    log-prob 1.0e-06 | 7.4e-07 | 5.0e-06, lse 8.0e-07 | 5.1e-07 | 4.1e-06."""
    from dynamic_asr_eval_amd import ops
    B, T, U = shape
    c = _case(B, T, U, V1)
    want, blank, T_b, U_b = c["want"], c["blank"], c["T_b"], c["U_b"]
    assert blank == V1 - 2 and np.isfinite(want["nll"]).all()
    xd, tgd, il, tl = _dev(c, cuda)
    loss, nll, grad = ops.rnnt_loss(xd, tgd, il, tl, blank, "none", 1.0)
    alpha, beta, lp, lse = (t.cpu() for t in ops.rnnt_lattice(B, T, U + 1, cuda))
    _check("nll (rel)", nll.cpu(), c["nll32"], want["nll"], LOSS_FLOOR, rel=True)
    _check("loss (rel)", loss.cpu(), c["nll32"].sum().reshape(1), np.array([want["nll"].sum()]), LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), c["g32"], want["grad"])
    x64 = c["x"].double()
    ltok = torch.log_softmax(x64, -1)
    for b in range(B):
        row = want["rows"][b]
        for name, got, ref in (("alpha", alpha, row["alpha"]), ("beta", beta, row["beta"])):
            got = got[b, :T_b[b], :U_b[b] + 1].numpy()
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin), (name, b)
            assert np.abs((got[fin] - ref[fin]) / (1 + np.abs(ref[fin]))).max() <= 2.0 ** -24 * (T_b[b] + U_b[b]), (name, b)
        assert (grad[b, T_b[b]:] == 0).all() and (grad[b, :, U_b[b] + 1:] == 0).all()
        assert torch.isneginf(lp[b, :, U_b[b]:, 1]).all() and torch.isfinite(lp[b, :, :U_b[b], 1]).all()
    _check("blank log-prob", lp[..., 0], torch.log_softmax(c["x"], -1)[..., blank], ltok[..., blank])
    _check("lse", lse, torch.logsumexp(c["x"], -1), torch.logsumexp(x64, -1))
    loss2, nll2, grad2 = ops.rnnt_loss(xd, tgd, il, tl, blank, "none", 1.0)
    assert torch.equal(grad2, grad) and torch.equal(nll2, nll)
    xin = xd.clone()
    _, _, over = ops.rnnt_loss(xin, tgd, il, tl, blank, "sum", 0.25, out=xin)
    assert over.data_ptr() == xin.data_ptr() and torch.equal(over, grad * 0.25)
    _, nll3, none = ops.rnnt_loss(xd, tgd, il, tl, blank, "sum", want_grad=False)
    assert none is None and torch.equal(nll3, nll)


@pytest.mark.parametrize("reduction", R.REDUCTIONS)
def test_rnnt_loss_reductions(cuda, reduction):
    """The five reductions of rnnt_loss ("none": the loss is the sum, the rows are nll) on ragged rows with grad_scale = 0.5; the default
    is "mean_volume"."""
    import inspect
    from dynamic_asr_eval_amd import ops
    assert inspect.signature(ops.rnnt_loss).parameters["reduction"].default == "mean_volume"
    c = _case(3, 33, 5, 65)
    x, tg, blank, T_b, U_b = c["x"], c["tg"], c["blank"], c["T_b"], c["U_b"]
    assert min(U_b) > 0
    want = R.rnnt_ref(x, tg, T_b, U_b, blank, reduction, grad_scale=0.5)
    l32, g32 = R.rnnt_torch(x, tg, T_b, U_b, blank, reduction)
    xd, tgd, il, tl = _dev(c, cuda)
    loss, nll, grad = ops.rnnt_loss(xd, tgd, il, tl, blank, reduction, 0.5)
    _check("loss (rel)", loss.cpu(), l32.sum().reshape(1), np.array([np.sum(want["loss"])]), LOSS_FLOOR, rel=True)
    _check("nll (rel)", nll.cpu(), c["nll32"], c["want"]["nll"], LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), g32 * 0.5, want["grad"])


def test_rnnt_lattice_with_a_diagonal_longer_than_the_workgroup(cuda):
    """T = 300, U = 299, V1 = 5: 599 diagonals, the longest 300 cells over the lattice workgroup's 256 threads (the stride loop).
    The fp32 result of the bars is here the restatement run in float32 (rnnt_row's dtype argument): the torch recursion's Python double
    loop with autograd takes 40 s at 90000 cells, and each test is to take a few seconds.
    Measured (MI355X), kernel | float32 restatement | bound: nll (rel) 4.5e-08 | 4.5e-08 | 1.2e-06, grad 7.2e-07 | 1.1e-04 | 4.5e-04."""
    from dynamic_asr_eval_amd import ops
    T, U, V1 = 300, 299, 5
    c = _case(1, T, U, V1, restated32=True)
    want, blank = c["want"], c["blank"]
    xd, tgd, il, tl = _dev(c, cuda)
    loss, nll, grad = ops.rnnt_loss(xd, tgd, il, tl, blank, "sum", 1.0)
    alpha, beta, _, _ = (t.cpu() for t in ops.rnnt_lattice(1, T, U + 1, cuda))
    _check("nll (rel)", nll.cpu(), c["nll32"], want["nll"], LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), c["g32"], want["grad"])
    row = want["rows"][0]
    for name, got, ref in (("alpha", alpha, row["alpha"]), ("beta", beta, row["beta"])):
        assert np.abs((got[0].numpy() - ref) / (1 + np.abs(ref))).max() <= 2.0 ** -24 * (T + U), name


def test_rnnt_lattice_hundreds_of_nats_down(cuda):
    """T = 300, U = 40 with the logits scaled by 4: alpha and beta reach hundreds of nats below zero; stored against integer bases, every
    cell stays within 2^-24 * (T_b + U_b) relative of float64, as the TDT test asks of its lattice.
    Measured (MI355X): alpha 3.0e-07, beta 2.2e-07 relative | bound 2.0e-05 (alpha and beta reach -1843 and -1847); kernel | torch fp32 |
    bound: nll (rel) 2.7e-08 | 1.6e-07 | 1.6e-06, grad 3.2e-05 | 1.2e-04 | 4.8e-04."""
    from dynamic_asr_eval_amd import ops
    T, U, V1 = 300, 40, 9
    c = _case(1, T, U, V1, 4.0)
    want, blank = c["want"], c["blank"]
    row = want["rows"][0]
    assert row["alpha"].min() < -300 and row["beta"].min() < -300
    xd, tgd, il, tl = _dev(c, cuda)
    loss, nll, grad = ops.rnnt_loss(xd, tgd, il, tl, blank, "sum", 1.0)
    alpha, beta, _, _ = (t.cpu() for t in ops.rnnt_lattice(1, T, U + 1, cuda))
    for name, got, ref in (("alpha", alpha, row["alpha"]), ("beta", beta, row["beta"])):
        err = np.abs((got[0].numpy() - ref) / np.abs(np.where(ref == 0, 1.0, ref))).max()
        print(f"{name}: relative error {err:.2e} | bound {2.0 ** -24 * (T + U):.2e}")
        assert err <= 2.0 ** -24 * (T + U), name
    _check("nll (rel)", nll.cpu(), c["nll32"], want["nll"], LOSS_FLOOR, rel=True)
    _check("grad", grad.cpu(), c["g32"], want["grad"])


def test_rnnt_unreachable_rows_are_inf_with_zero_gradient(cuda):
    """Row 0: the logit of its second target is -inf at every frame of u = 1, so that label has no probability and no complete path
    exists.  Row 1: T_b = 0.  Both give nll = +inf and a zero, finite gradient; the finite row 2 next to them stays within 1e-5."""
    from dynamic_asr_eval_amd import ops
    x, tg, blank = R.rnnt_inputs(3, 6, 3, 9, 2)
    x[0, :, 1, int(tg[0, 1])] = -float("inf")
    T_b, U_b = [6, 0, 5], [3, 2, 3]
    want = R.rnnt_ref(x, tg, T_b, U_b, blank, "none")
    assert np.isposinf(want["nll"][:2]).all() and np.isfinite(want["nll"][2])
    il, tl = torch.tensor(T_b, dtype=torch.int32, device=cuda), torch.tensor(U_b, dtype=torch.int32, device=cuda)
    loss, nll, grad = ops.rnnt_loss(x.to(cuda), tg.to(cuda), il, tl, blank, "sum")
    assert torch.isposinf(nll[:2]).all() and torch.isposinf(loss).all() and torch.isfinite(grad).all() and (grad[:2] == 0).all()
    assert abs(float(nll[2]) - want["nll"][2]) < 1e-5 and np.abs(grad[2].cpu().numpy() - want["grad"][2]).max() < 1e-5
    assert grad[2].abs().max().item() > 0


@pytest.mark.parametrize("dTc", ["1", "3", "T-1", "T", "T+5"])
def test_rnnt_chunk_forms_are_bit_equal_to_the_whole_form(cuda, dTc):
    """The arcs of every chunk of Tc frames into a caller-owned state, the lattice run on it, the gradient chunk by chunk: the state (lp, lse,
    alpha, beta), loss, nll and gradient are torch.equal to ops.rnnt_loss on the whole tensor, for Tc = 1, 3, T - 1, T and T + 5 (a chunk
    that overhangs the lattice: those rows are not read, and come out as zeros of the gradient)."""
    from dynamic_asr_eval_amd import ops
    B, T, U, V1 = 3, 33, 5, 65
    Tc = {"1": 1, "3": 3, "T-1": T - 1, "T": T, "T+5": T + 5}[dTc]
    c = _case(B, T, U, V1)
    blank = c["blank"]
    xd, tgd, il, tl = _dev(c, cuda)
    loss, nll, grad = ops.rnnt_loss(xd, tgd, il, tl, blank, "mean_volume", 0.5)
    whole = [t.clone() for t in ops.rnnt_lattice(B, T, U + 1, cuda)]
    state = ops.rnnt_state(B, T, U + 1, cuda)
    state.fill_(0xff)

    def chunk(t0):
        n = min(Tc, T - t0)
        buf = torch.full((B, Tc, U + 1, V1), float("nan"), device=cuda)         # the overhang is never read
        buf[:, :n] = xd[:, t0:t0 + n]
        return buf, n

    for t0 in range(0, T, Tc):
        ops.rnnt_arcs_chunk(chunk(t0)[0], t0, T, tgd, tl, blank, state)
    loss_c, nll_c = ops.rnnt_lattice_run(B, T, U + 1, tgd.shape[1], il, tl, state, "mean_volume")
    assert torch.equal(loss_c, loss) and torch.equal(nll_c, nll)
    got = ops.rnnt_lattice(B, T, U + 1, cuda, state=state)
    for b in range(B):
        tb, ub = c["T_b"][b], c["U_b"][b]
        for name, g, w in zip(("alpha", "beta"), got[:2], whole[:2]):
            assert torch.equal(g[b, :tb, :ub + 1], w[b, :tb, :ub + 1]), (name, b)
    assert torch.equal(got[2], whole[2]) and torch.equal(got[3], whole[3])
    for t0 in range(0, T, Tc):
        buf, n = chunk(t0)
        g = ops.rnnt_grad_chunk(buf, t0, T, tgd, il, tl, blank, state, "mean_volume", 0.5, out=buf)
        assert g.data_ptr() == buf.data_ptr() and torch.equal(g[:, :n], grad[:, t0:t0 + n]) and (g[:, n:] == 0).all(), t0


def test_rnnt_budget_refusal_is_by_name(cuda):
    from dynamic_asr_eval_amd import ops
    c = _case(3, 33, 5, 65)
    xd, tgd, il, tl = _dev(c, cuda)
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_loss(xd, tgd, il, tl, c["blank"], budget=1000)
    assert "dyn_rnnt_loss" in str(e.value) and "budget of 1000" in str(e.value) and "chunking the lattice state is not built" in str(e.value)
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_state(3, 33, 6, cuda, budget=1000)
    assert "rnnt_state" in str(e.value) and "budget of 1000" in str(e.value)
    state = ops.rnnt_state(3, 33, 6, cuda)
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_arcs_chunk(xd[:, :4].contiguous(), 0, 33, tgd, tl, c["blank"], state, budget=1000)
    assert "dyn_rnnt_arcs_chunk" in str(e.value) and "budget" in str(e.value)
    with pytest.raises(ops.DynError) as e:
        ops.rnnt_lattice_run(3, 33, 6, tgd.shape[1], il, tl, state, budget=1000)
    assert "dyn_rnnt_lattice_run" in str(e.value) and "budget" in str(e.value)


def _greedy_case(seed=6, B=3, T=11, Hd=64, L=2, V1=33):
    """Found by a seeded search on the CPU: with these gains the plain-torch loop alone shows blanks, frames that emit two or more symbols
    and are then left by a blank, and frames left by the forced advance, with top-2 margins of at least 2e-2."""
    g = K.gen(63000 + seed)
    emb = torch.nn.Embedding(V1, Hd)
    lstm = torch.nn.LSTM(Hd, Hd, L, batch_first=True)
    proj, head = torch.nn.Linear(Hd, Hd), torch.nn.Linear(Hd, V1)
    with torch.no_grad():
        for m, gain in ((emb, 3.0), (lstm, 4.0), (proj, 6.0), (head, 3.0)):     # scaled gains: the argmaxes have margins
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * gain / (p.shape[-1] ** 0.5 if p.dim() > 1 else 4.0))
        head.bias[V1 - 1] += 6.0                                                  # the blank wins often enough for frames to advance
    enc = torch.randn(B, T, Hd, generator=g) * 2.0
    return enc, emb, lstm, proj, head


@pytest.mark.parametrize("max_symbols", [2, 10])
def test_rnnt_greedy_steps_against_a_plain_torch_step_loop(cuda, max_symbols):
    """dyn_rnnt_greedy_steps against rnnt_refs.greedy_steps_torch on the CPU: random small weights with scaled gains, B = 3 rows with valid
    lengths 11, 7 and 1, max_symbols_per_step 2 (forcing is reached) and 10.  Tokens, frames, counts and steps are equal, and equal
    whether the steps are queued one per host call or 32.  The smallest top-2 margin of the CPU loop is asserted to be at least 1e-2."""
    from dynamic_asr_eval_amd import ops
    enc, emb, lstm, proj, head = _greedy_case()
    B, T, Hd = enc.shape
    V1, blank, valid = head.out_features, head.out_features - 1, [11, 7, 1]
    cap = max_symbols * T
    margins, want = [], []
    with torch.no_grad():
        for b in range(B):
            want.append(R.greedy_steps_torch(enc[b, :valid[b]], emb, lstm, proj, head, blank, blank, max_symbols, cap,
                                             lambda lg: margins.append(float(lg.topk(2).values.diff().abs()))))
    assert min(margins) >= 1e-2, min(margins)
    steps = [s for w in want for s in w[2]]
    assert any(k == blank for k, _, _ in steps) and any(k != blank for k, _, _ in steps)
    assert any(k != blank and adv == 1 for k, adv, _ in steps)                  # a forced advance is among them
    if max_symbols == 10:                                                       # and a frame of several symbols left by a blank
        import itertools
        frames = [[k for k, _, _ in grp] for w in want for _, grp in itertools.groupby(w[2], key=lambda s: s[2])]
        assert any(ks[-1] == blank and len(ks) >= 3 for ks in frames)
    dev = lambda t: t.detach().to(cuda).contiguous()                             # noqa: E731
    ws = [dev(getattr(lstm, f"{n}_l{k}")) for k in range(lstm.num_layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    ptrs = torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64, device=cuda)
    args = (dev(enc), torch.tensor(valid, dtype=torch.int32, device=cuda), dev(emb.weight), ptrs, dev(proj.weight), dev(proj.bias),
            dev(head.weight), dev(head.bias))
    outs = []
    for queue in (1, 32):
        st = ops.RnntGreedyState(B, Hd, lstm.num_layers, V1, cap, blank, cuda)
        done = 0
        while done < cap and not bool(st.istate[3].all()):
            n = min(queue, cap - done)
            ops.rnnt_greedy_steps(*args, st, blank, max_symbols, cap, n)
            done += n
        outs.append((st.tokens.cpu(), st.frames.cpu(), st.istate.cpu()))
        for b in range(B):
            toks, frs, stp = want[b]
            n = int(st.istate[4, b])
            assert n == len(toks) and st.tokens[b, :n].tolist() == toks and st.frames[b, :n].tolist() == frs, (queue, b)
            assert int(st.istate[5, b]) == len(stp) and int(st.istate[3, b]) == 1, (queue, b)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
