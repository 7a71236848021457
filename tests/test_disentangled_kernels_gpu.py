"""dyn_softmax_disentangled_fwd / dyn_disentangled_bwd (csrc/disentangled.hip: SEW-D's bucket gather fused into the masked row softmax, and
the gathers' backward as segment sums) and dyn_squeeze_fwd / _bwd (csrc/squeeze.hip with the LayerNorm compiled out) against float64 torch on
the CPU.  The float64 side restates transformers' disentangled_attention_bias: build_relative_position, the two clamped indices, the two
`torch.gather`s, the transpose, and autograd for the backward (index_add under the hood).  Conventions of test_squeeze_kernels_gpu.py:
kernel_refs.measured_tol (4 x torch's own fp32 error + floor) with the masked softmax's floor 2e-6 for the probabilities
(tests/test_row_kernels_gpu.py), 5e-6 forward / 2e-5 gradients for the segment sums and the squeeze outputs, kernel_refs.wgrad_tol(5e-4, rows,
531) for the bias column sum.  Every check prints `name: kernel error | torch fp32 error | bound` before it asserts."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402
import test_squeeze_kernels_gpu as Q  # noqa: E402  (its five shapes, valid lengths, inputs and check helpers)

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 9, 8, 32), (1, 3, 46, 8, 32), (1, 2, 70, 4, 8), (2, 1, 33, 16, 16), (1, 1, 300, 256, 512)]      # (B, nh, T, buckets, max_position)
IDS = ["T9-no-clamp", "T46-clamp-both-ends", "T70-far-buckets", "T33-odd", "T300-stride-loop-256-512"]
PAD = 4                       # ldp - 2 span: columns (rows) of the position products that hold NaN and are never to be read
NAN = float("nan")


def _case(B, nh, T, b, m, seed=0):
    """Scores, both position products [B, nh, T, R] (c2p by query, p2c by KEY, as transformers forms them), dS, and transformers' two index
    matrices.  Buckets no (i, j) reaches are NaN in the kernel's copies, like the padding."""
    from transformers.models.sew_d.modeling_sew_d import build_relative_position
    from dynamic_asr_eval_amd.sew_d_model import att_span, bucket_table
    g = K.gen(7000 + seed + B * T + nh + b)
    span = att_span(b, m)
    R = 2 * span
    S, dS = (torch.randn(B, nh, T, T, generator=g) for _ in range(2))
    c2p, p2c = (torch.randn(B, nh, T, R, generator=g) for _ in range(2))
    rel = build_relative_position(T, T, bucket_size=b, max_position=m)[0]
    c2p_pos = torch.clamp(rel + span, 0, R - 1)
    p2c_pos = torch.clamp(-rel + span, 0, R - 1)
    tab = bucket_table(T, b, m)
    empty = tab.lo > tab.hi
    ldp = R + PAD
    c_k = torch.full((B, nh, T, ldp), NAN)
    c_k[..., :R] = c2p
    c_k[..., :R][..., empty] = NAN
    p_k = torch.full((B, nh, ldp, T), NAN)
    p_k[:, :, :R] = p2c.transpose(-1, -2)
    p_k[:, :, :R][:, :, empty] = NAN
    return dict(S=S, dS=dS, c2p=c2p, p2c=p2c, c2p_pos=c2p_pos, p2c_pos=p2c_pos, tab=tab, R=R, ldp=ldp, c_k=c_k.contiguous(), p_k=p_k.contiguous())


def _ref(case, valid, use_c2p, use_p2c, dtype):
    """(probabilities, dC2P [B, nh, T, R], dP2C [B, nh, T(key), R]): the gathers as transformers writes them, the key mask, autograd of
    sum(dS * score) with the rows and columns >= valid of dS cut."""
    S, dS = case["S"].to(dtype), case["dS"].to(dtype)
    c2p, p2c = (case[k].to(dtype).clone().requires_grad_() for k in ("c2p", "p2c"))
    B, nh, T, _ = S.shape
    Lv = K.clamped_valid(valid, T)
    score = S
    if use_c2p:
        score = score + torch.gather(c2p, -1, case["c2p_pos"].expand(B, nh, T, T))
    if use_p2c:
        score = score + torch.gather(p2c, -1, case["p2c_pos"].expand(B, nh, T, T)).transpose(-1, -2)
    y = torch.zeros_like(S)
    y[..., :Lv] = torch.softmax(score[..., :Lv].detach(), -1)
    keep = torch.zeros(T, dtype=dtype)
    keep[:Lv] = 1.0
    (score * dS * keep[:, None] * keep[None, :]).sum().backward()
    zero = torch.zeros_like(c2p)
    return y, (c2p.grad if use_c2p else zero), (p2c.grad if use_p2c else zero)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_softmax_and_segment_sums_against_float64(cuda, shape):
    """Every shape with valid in {None, T, T - 2, 1}, both terms and each alone.  ldp = 2 span + 4 with NaN in the padding and in every bucket
    no (i, j) reaches; dS holds NaN in the rows and columns >= valid.  Outputs at rows >= valid are exact zeros, so is the padding; the inputs
    are left unmodified; two identical calls give identical bits."""
    from dynamic_asr_eval_amd import ops
    B, nh, T, b, m = shape
    case = _case(B, nh, T, b, m)
    R, ldp, tab = case["R"], case["ldp"], case["tab"]
    Sd, ck, pk = (case[k].to(cuda) for k in ("S", "c_k", "p_k"))
    table, lo, hi = (t.to(cuda) for t in tab)
    S_before, ck_before, pk_before = Sd.clone(), ck.clone(), pk.clone()
    for valid in Q._valids(T):
        Lv = T if valid is None else valid
        vt = Q._vt(valid, cuda)
        dSn = case["dS"].clone()
        dSn[..., Lv:, :] = NAN
        dSn[..., :, Lv:] = NAN
        dSd = dSn.to(cuda)
        for use_c2p, use_p2c in ((True, True), (True, False), (False, True)):
            tag = f"valid {valid}, c2p {int(use_c2p)}, p2c {int(use_p2c)}"
            r64, r32 = (_ref(case, valid, use_c2p, use_p2c, dt) for dt in (torch.float64, torch.float32))
            args = (Sd, ck if use_c2p else None, pk if use_p2c else None, table, R, ldp)
            y = ops.softmax_disentangled(*args, valid=vt)
            assert y.shape == Sd.shape and torch.isfinite(y).all()
            assert Q._bits_equal(y, ops.softmax_disentangled(*args, valid=vt)), "two identical calls must give identical bits"
            if Lv < T:
                assert y[..., Lv:].abs().max().item() == 0.0
            Q._measured(f"probabilities ({tag})", y, r32[0], r64[0], 2e-6)
            dc, dpt = ops.disentangled_bwd(dSd, table, lo, hi, ldp, want_c2p=use_c2p, want_p2c=use_p2c, valid=vt)
            dc2, dpt2 = ops.disentangled_bwd(dSd, table, lo, hi, ldp, want_c2p=use_c2p, want_p2c=use_p2c, valid=vt)
            assert (dc is None) == (not use_c2p) and (dpt is None) == (not use_p2c)
            if use_c2p:
                assert dc.shape == (B, nh, T, ldp) and torch.isfinite(dc).all() and Q._bits_equal(dc, dc2)
                assert dc[..., R:].abs().max().item() == 0.0 and dc[..., :R][..., tab.lo > tab.hi].abs().sum().item() == 0.0
                if Lv < T:
                    assert dc[:, :, Lv:].abs().max().item() == 0.0
                Q._measured(f"dC2P ({tag})", dc[..., :R], r32[1], r64[1], 2e-5)
            if use_p2c:
                assert dpt.shape == (B, nh, ldp, T) and torch.isfinite(dpt).all() and Q._bits_equal(dpt, dpt2)
                assert dpt[:, :, R:].abs().max().item() == 0.0 and dpt[:, :, :R][:, :, tab.lo > tab.hi].abs().sum().item() == 0.0
                if Lv < T:
                    assert dpt[..., Lv:].abs().max().item() == 0.0
                Q._measured(f"dP2C ({tag})", dpt[:, :, :R].transpose(-1, -2), r32[2], r64[2], 2e-5)
            assert Q._bits_equal(Sd, S_before) and Q._bits_equal(ck, ck_before) and Q._bits_equal(pk, pk_before)
            assert Q._bits_equal(dSd, dSn), "dS must not be modified"
    inplace = Sd.clone()                                         # the model's call: the probabilities over the scores
    ops.softmax_disentangled(inplace, ck, pk, table, R, ldp, out=inplace)
    assert Q._bits_equal(inplace, ops.softmax_disentangled(Sd, ck, pk, table, R, ldp))


def test_wrappers_refuse_a_wrong_table_or_a_short_ldp_before_any_launch(cuda):
    from dynamic_asr_eval_amd import _lib, ops
    from dynamic_asr_eval_amd.sew_d_model import bucket_table
    T, R = 12, 16
    S = torch.randn(1, 2, T, T, device=cuda)
    table, lo, hi = (t.to(cuda) for t in bucket_table(T, 8, 32))
    wrong = bucket_table(T + 1, 8, 32).table.to(cuda)
    c2p, p2ct = torch.randn(1, 2, T, R, device=cuda), torch.randn(1, 2, R, T, device=cuda)
    out = torch.full_like(S, 7.0)
    for fn, word in ((lambda: ops.softmax_disentangled(S, c2p, p2ct, wrong, R, R, out=out), "2T - 1"),
                     (lambda: ops.softmax_disentangled(S, c2p, p2ct, table, R, R - 4, out=out), "shorter than the n_buckets"),
                     (lambda: ops.softmax_disentangled(S, None, None, table, R, R, out=out), "both position terms"),
                     (lambda: ops.softmax_disentangled(S, c2p[..., :8].contiguous(), p2ct, table, R, R, out=out), "c2p holds"),
                     (lambda: ops.softmax_disentangled(S, c2p, p2ct, table.float(), R, R, out=out), "dtype"),
                     (lambda: ops.disentangled_bwd(S, wrong, lo, hi, R), "2T - 1"),
                     (lambda: ops.disentangled_bwd(S, table, lo, hi, R - 4), "shorter than the n_buckets"),
                     (lambda: ops.disentangled_bwd(S, table, lo, hi[:8].contiguous(), R), "differ in length"),
                     (lambda: ops.disentangled_bwd(S, table, lo, hi, R, want_c2p=False, want_p2c=False), "at least one")):
        with pytest.raises(ops.DynError) as e:
            fn()
        assert word in str(e.value), str(e.value)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.dyn_softmax_disentangled_fwd(S.data_ptr(), out.data_ptr(), c2p.data_ptr(), p2ct.data_ptr(), table.data_ptr(), 2, T, R - 1, R, None, st)
    assert rc == -1 and b"dyn_softmax_disentangled_fwd" in lib.dyn_last_error() and b"ldp=15" in lib.dyn_last_error()
    rc = lib.dyn_disentangled_bwd(S.data_ptr(), out.data_ptr(), 0, table.data_ptr(), lo.data_ptr(), hi.data_ptr(), 2, T, R - 1, R, None, st)
    assert rc == -1 and b"dyn_disentangled_bwd" in lib.dyn_last_error() and b"ldp=15" in lib.dyn_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def _squeeze_ref(h, y, bias, dz, s, valid, dtype):
    """(z, dh, dy, dbias) of AvgPool1d(s, s)(h)[:T2] + gelu(y + bias) from torch's own ops and autograd in `dtype`; rows >= valid are zeroed."""
    hr, yr, br = (t.detach().to(dtype).clone().requires_grad_() for t in (h, y, bias))
    T2 = h.shape[1] // s
    z = F.avg_pool1d(hr.transpose(1, 2), s, s).transpose(1, 2)[:, :T2] + F.gelu(yr + br)
    keep = torch.zeros(T2, dtype=dtype)
    keep[:T2 if valid is None else valid] = 1.0
    z = z * keep[None, :, None]
    z.backward(dz.to(dtype))
    return z.detach(), hr.grad, yr.grad, br.grad


@pytest.mark.parametrize("shape", Q.SHAPES, ids=Q.IDS)
def test_squeeze_without_layernorm_against_float64(cuda, shape):
    """test_squeeze_kernels_gpu.py's five shapes, valid lengths and inputs (Tg = T2 + 3, NaN in the rows never to be read) through the
    no-LayerNorm entries; dz holds NaN in the rows >= valid.  Exact zeros past valid, wgrad_beta 0 / 1 and a null dbias, inputs unmodified,
    identical bits on a second call."""
    from dynamic_asr_eval_amd import ops
    B, T, H, G, s = shape
    T2 = T // s
    h, y, yg, bias, _, _, dz, old = Q._inputs(B, T, H, G, s, 0)
    hd, ygd, bd = (t.to(cuda) for t in (h, yg, bias))
    h_before, yg_before = hd.clone(), ygd.clone()
    wtol = K.wgrad_tol(5e-4, B * T2, 531)
    for valid in Q._valids(T2):
        tag = f"valid {valid}"
        Tv = T2 if valid is None else valid
        vt = Q._vt(valid, cuda)
        r64, r32 = (_squeeze_ref(h, y, bias, dz, s, valid, dt) for dt in (torch.float64, torch.float32))
        z = ops.squeeze(hd, ygd, bd, s, valid=vt)
        assert z.shape == (B, T2, H) and torch.isfinite(z).all() and Q._bits_equal(z, ops.squeeze(hd, ygd, bd, s, valid=vt))
        if Tv < T2:
            assert z[:, Tv:].abs().max().item() == 0.0
        Q._measured(f"z ({tag})", z, r32[0], r64[0], 5e-6)
        dzn = dz.clone()
        dzn[:, Tv:] = NAN
        dzd = dzn.to(cuda)
        for wbeta in (0.0, 1.0):
            db = old[2].to(cuda)
            dh, dyg = ops.squeeze_bwd(ygd, bd, dzd, T, s, db, wgrad_beta=wbeta, valid=vt)
            assert dh.shape == (B, T, H) and dyg.shape == (B, G, T2, H // G) and torch.isfinite(dh).all() and torch.isfinite(dyg).all()
            if s * Tv < T:
                assert dh[:, s * Tv:].abs().max().item() == 0.0
            if Tv < T2:
                assert dyg[:, :, Tv:].abs().max().item() == 0.0
            Q._measured(f"dh ({tag}, wgrad_beta {wbeta:g})", dh, r32[1], r64[1], 2e-5)
            Q._measured(f"dyg ({tag}, wgrad_beta {wbeta:g})", dyg, Q._grouped(r32[2], G), Q._grouped(r64[2], G), 2e-5)
            Q._check(f"dbias ({tag}, wgrad_beta {wbeta:g})", db, r64[3] + wbeta * old[2].double(), wtol)
        again = ops.squeeze_bwd(ygd, bd, dzd, T, s, old[2].to(cuda), wgrad_beta=1.0, valid=vt)
        frozen = ops.squeeze_bwd(ygd, bd, dzd, T, s, None, valid=vt)
        assert Q._bits_equal(again[0], dh) and Q._bits_equal(again[1], dyg), "two identical calls must give identical bits"
        assert Q._bits_equal(frozen[0], dh) and Q._bits_equal(frozen[1], dyg), "a null dbias: the same dh and dyg"
        assert Q._bits_equal(ygd, yg_before) and Q._bits_equal(hd, h_before) and Q._bits_equal(dzd, dzn)
