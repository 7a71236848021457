"""dyn_prompt_bias_gather, dyn_prompt_relu_fwd and dyn_prompt_relu_bwd (csrc/prompt_fuse.hip: the language prompt of Nemotron3_5AsrForRNNT as
a per-batch-row bias, its fused ReLU each way and the segment sum behind dW1p) against float64 torch on the CPU (tests/nemotron35_refs.py)
under kernel_refs.measured_tol: 4 x torch's own fp32 error + the floor 2e-6 for the bias, the activations and dz,
kernel_refs.wgrad_tol(5e-4, B * T, 531) for the column sums.  Beyond parity, asserted outright: a column of a prompt no row used is exactly
zero at beta = 0 and keeps its bits at beta = 1, a duplicated id's column is the fp32 sum of its rows' s[b] in ascending b, z + pb = 0
gives a = 0 and dz = 0, in place equals out of place, two runs give equal bits.  Every check prints `name: kernel error | torch fp32
error | bound` before it asserts."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import nemotron35_refs as PR  # noqa: E402

pytestmark = pytest.mark.gpu

NP = 8
ROW_TILE = 8                  # dyn_prompt_relu_bwd_row_tile(T) for T <= 8 * 64: checked below, so that T = 9 is one above the tile
BATCHES = {3: PR.PROMPTS_A, 1: [3]}


def _check(name, got, want, tol, e32=None):
    err = K.max_err(got, want)
    print(f"  {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")
    assert err <= tol, f"{name}: err {err} > {tol} (torch fp32: {e32})"


def _measured(name, got, torch32, want, floor):
    tol, e32 = K.measured_tol(torch32, want, floor)
    _check(name, got, want, tol, e32)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inputs(B, T, I, seed=0):
    g = K.gen(35000 + seed + 7 * B + 13 * T + I)
    z = torch.randn(B, T, I, generator=g)
    b1, w1p = torch.randn(I, generator=g), torch.randn(I, NP, generator=g) * 2.0
    da = torch.randn(B, T, I, generator=g)
    old_b, old_w = torch.randn(I, generator=g), torch.randn(I, NP, generator=g)
    old_w[::3] *= -0.0                                       # signed zeros among the old content: beta = 1 must keep their bits
    return z, b1, w1p, da, old_b, old_w


def _dev_ids(ids, cuda):
    return torch.tensor(ids, dtype=torch.int32, device=cuda)


@pytest.mark.parametrize("I", [96, 2048])
@pytest.mark.parametrize("T", [1, 5, 37, ROW_TILE + 1])
@pytest.mark.parametrize("B", [3, 1])
def test_gather_forward_and_backward_against_float64(cuda, B, T, I):
    from dynamic_asr_eval_amd import _lib, ops
    assert _lib.load().dyn_prompt_relu_bwd_row_tile(ROW_TILE) == ROW_TILE and _lib.load().dyn_prompt_relu_bwd_row_tile(ROW_TILE + 1) < ROW_TILE + 1
    ids = BATCHES[B]
    z, b1, w1p, da, old_b, old_w = _inputs(B, T, I)
    idd = _dev_ids(ids, cuda)
    # ---- gather
    pb = ops.prompt_bias_gather(b1.to(cuda), w1p.to(cuda), idd)
    assert pb.shape == (B, I) and _bits_equal(pb, PR.gather(b1, w1p, ids)), "one fp32 add per element: the CPU's bits"
    _measured("pb", pb, PR.gather(b1, w1p, ids), PR.gather(b1.double(), w1p.double(), ids), 2e-6)
    # ---- forward; a few pre-activations are exactly zero: z = -pb there
    zero_at = (slice(None), slice(0, T, 2), slice(0, I, 5))
    z[zero_at] = -pb.cpu()[:, None, ::5].expand(B, len(range(0, T, 2)), -1)
    zd = z.to(cuda)
    a = ops.prompt_relu(zd, pb)
    assert _bits_equal(zd, z), "out of place: z must not be modified"
    assert a.shape == (B, T, I) and _bits_equal(a, ops.prompt_relu(zd, pb)), "two runs, equal bits"
    inplace = zd.clone()
    assert ops.prompt_relu(inplace, pb, out=inplace) is inplace and _bits_equal(inplace, a), "in place equals out of place"
    _measured("a", a, PR.fused_fwd(z, pb.cpu()), PR.fused_fwd(z.double(), pb.cpu().double()), 2e-6)
    assert a[zero_at].abs().max().item() == 0.0 and bool((a >= 0).all())
    # ---- backward
    ah, dad = a.cpu(), da.to(cuda)
    r64, r32 = PR.fused_bwd(ah.double(), da.double(), ids, NP), PR.fused_bwd(ah, da, ids, NP)
    rows_s = []
    for b in range(B):                                         # s[b]: the kernel on row b alone at beta = 0 writes it as db1
        sb = torch.full((I,), float("nan"), device=cuda)
        ops.prompt_relu_bwd(a[b:b + 1].contiguous(), dad[b:b + 1].contiguous(), idd[b:b + 1].clone(), sb, None, beta=0.0)
        rows_s.append(sb.cpu())
    stol = K.wgrad_tol(5e-4, B * T, 531)
    _measured("s", torch.stack(rows_s), r32[1], r64[1], stol)
    unused = [p for p in range(NP) if p not in ids]
    for beta in (0.0, 1.0):
        db, dw = old_b.to(cuda), old_w.to(cuda)
        dz = ops.prompt_relu_bwd(a, dad, idd, db, dw, beta=beta)
        assert _bits_equal(dad, da), "out of place: da must not be modified"
        db2, dw2, g2 = old_b.to(cuda), old_w.to(cuda), dad.clone()
        assert ops.prompt_relu_bwd(a, g2, idd, db2, dw2, beta=beta, out=g2) is g2
        assert _bits_equal(g2, dz) and _bits_equal(db2, db) and _bits_equal(dw2, dw), "in place over da, a second run: equal bits"
        _measured(f"dz (beta {beta:g})", dz, r32[0], r64[0], 2e-6)
        assert dz[a <= 0].abs().max().item() == 0.0 and dz[zero_at].abs().max().item() == 0.0
        _measured(f"db1 (beta {beta:g})", db, r32[2] + beta * old_b, r64[2] + beta * old_b.double(), stol)
        _measured(f"dW1p (beta {beta:g})", dw, r32[3] + beta * old_w, r64[3] + beta * old_w.double(), stol)
        if beta == 0.0:
            assert dw[:, unused].abs().max().item() == 0.0, "unused prompts: exact zeros at beta = 0"
            acc = torch.zeros(I)
            for b in range(B):                                 # b ascending, as the kernel adds them
                acc = acc + rows_s[b]
            assert _bits_equal(db, acc), "db1 = the fp32 sum of s[b], b ascending"
            for p in set(ids):
                col = torch.zeros(I)
                for b in [b for b in range(B) if ids[b] == p]:
                    col = col + rows_s[b]
                assert _bits_equal(dw[:, p], col), f"column {p}: the fp32 sum of its rows' s[b], b ascending"
        else:
            assert _bits_equal(dw[:, unused], old_w[:, unused]), "unused prompts: the old bits at beta = 1"
    # ---- frozen gradients: null pointers, dz alone
    only = ops.prompt_relu_bwd(a, dad, idd, None, None)
    assert _bits_equal(only, dz)
    half_b = old_b.to(cuda)
    ops.prompt_relu_bwd(a, dad, idd, half_b, None, beta=1.0)
    assert _bits_equal(half_b, db)


def test_ids_outside_the_table_are_clamped_by_the_gather_and_skipped_by_the_segment_sum(cuda):
    """The callers validate the ids on the host; the kernels still stay inside the table for any id.  The gather clamps (-1 reads column 0,
    Np reads column Np - 1); the backward compares ids with column numbers and never indexes with them: such a row adds to db1 alone."""
    from dynamic_asr_eval_amd import ops
    B, T, I = 3, 5, 96
    z, b1, w1p, da, old_b, old_w = _inputs(B, T, I, seed=1)
    bad = _dev_ids([-1, NP, 3], cuda)
    pb = ops.prompt_bias_gather(b1.to(cuda), w1p.to(cuda), bad)
    assert _bits_equal(pb, PR.gather(b1, w1p, [0, NP - 1, 3]))
    a = ops.prompt_relu(z.to(cuda), pb)
    db, dw = torch.zeros(I, device=cuda), torch.zeros(I, NP, device=cuda)
    ops.prompt_relu_bwd(a, da.to(cuda), bad, db, dw, beta=0.0)
    _, s, db_ref, _ = PR.fused_bwd(a.cpu().double(), da.double(), [3, 3, 3], NP)
    tol = K.wgrad_tol(5e-4, B * T, 531)
    _check("db1", db, db_ref, tol)
    _check("column 3", dw[:, 3], s[2], tol)
    assert dw[:, [p for p in range(NP) if p != 3]].abs().max().item() == 0.0


def test_wrappers_refuse_before_any_launch(cuda):
    from dynamic_asr_eval_amd import ops
    z, b1, w1p, da, old_b, old_w = (t.to(cuda) for t in _inputs(3, 5, 96))
    ids = _dev_ids(PR.PROMPTS_A, cuda)
    pb = ops.prompt_bias_gather(b1, w1p, ids)
    a = ops.prompt_relu(z, pb)
    for call in (lambda: ops.prompt_bias_gather(b1, w1p, ids.long()), lambda: ops.prompt_bias_gather(b1, w1p[:95], ids),
                 lambda: ops.prompt_bias_gather(b1.cpu(), w1p, ids), lambda: ops.prompt_relu(z, pb[:2]), lambda: ops.prompt_relu(z[:, :, :92], pb),
                 lambda: ops.prompt_relu_bwd(a, da[:2], ids, old_b, old_w), lambda: ops.prompt_relu_bwd(a, da, ids[:2], old_b, old_w),
                 lambda: ops.prompt_relu_bwd(a, da, ids, old_b[:95], old_w), lambda: ops.prompt_relu_bwd(a, da, ids, old_b, old_w[:95]),
                 lambda: ops.prompt_relu_bwd(a, da, ids, old_b, old_w, out=a)):
        with pytest.raises(ops.DynError):
            call()
