"""What the training-mode BatchRenorm feature shows without a GPU: the C-ABI surface, the loop's keyword, the clamp schedule, and the
test-side references of tests/batch_renorm_refs.py against each other (the oracle module, autograd, the closed form the kernels implement)."""
import argparse
import copy
import inspect
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import batch_renorm_refs as BR  # noqa: E402
import parakeet_refs as PR  # noqa: E402

ENTRIES = ("dyn_convmod_brn_fwd", "dyn_convmod_brn_bwd", "dyn_convmod_brn_fwd_workspace_bytes", "dyn_convmod_brn_bwd_workspace_bytes",
           "dyn_convmod_brn_stats_rows")


def test_header_declares_the_entries_and_the_parser_reads_them():
    import ctypes
    from dynamic_asr_eval_amd import _lib
    protos = _lib.prototypes()
    for name in ENTRIES:
        assert name in protos, name
    restype, args = protos["dyn_convmod_brn_fwd"]
    assert restype is ctypes.c_int and len(args) == 24
    assert args[:12] == [ctypes.c_void_p] * 12 and args[12:16] == [ctypes.c_int64] * 4 and args[16] is ctypes.c_int32
    assert args[17:21] == [ctypes.c_float] * 4 and args[21:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    restype, args = protos["dyn_convmod_brn_bwd"]
    assert restype is ctypes.c_int and len(args) == 16
    assert args[:7] == [ctypes.c_void_p] * 7 and args[7] is ctypes.c_float and args[8] is ctypes.c_void_p
    assert args[9:12] == [ctypes.c_int64] * 3 and args[12] is ctypes.c_int32 and args[13:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert protos["dyn_convmod_brn_fwd_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64] * 4)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dyneval.h")).read()
    assert "nvidia_ctc/lib.py:74,89-102" in hdr and "parity unpinned against upstream `lcasr`" in hdr


def test_loop_has_the_keyword_and_the_model_the_context():
    from dynamic_asr_eval_amd import lasr_model, nvidia_ctc_lib as N, parakeet_model
    p = inspect.signature(N.dynamic_eval_ctc_loss).parameters["batch_renorm"]
    assert p.default is None
    assert N.BATCH_RENORM == BR.REFERENCE == dict(momentum=0.001, eps=1e-5, num_batches_tracked=1000000)
    sig = inspect.signature(parakeet_model.ParakeetForCTC.batch_renorm_training).parameters
    assert (sig["momentum"].default, sig["eps"].default, sig["num_batches_tracked"].default) == (0.001, 1e-5, 1_000_000)
    assert lasr_model.LasrForCTC.batch_renorm_training is parakeet_model.ParakeetForCTC.batch_renorm_training


def test_clamp_schedule():
    from dynamic_asr_eval_amd import ops
    for f in (ops.batch_renorm_clamps, BR.clamps):
        assert f(0) == (1.0, 0.0)
        assert f(1e6) == (3.0, 5.0) and f(1000000) == (3.0, 5.0)
        rmax, dmax = f(10000)
        assert abs(rmax - (20000 / 35000 + 25 / 35)) < 1e-12 and abs(dmax - 1.25) < 1e-12
    assert ops.batch_renorm_clamps(12345) == BR.clamps(12345)


def test_oracle_module_without_active_clamps_is_the_eval_affine():
    """With neither clamp active r = sig / running_std and d = (mu - running_mean) / running_std, so the training-mode forward equals the
    eval-mode affine (x - running_mean) / running_std * w + b, to float64 rounding."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 8, 21, generator=g, dtype=torch.float64) * 2.0 + 0.7
    m = BR.BatchRenorm1d(8, eps=1e-5, momentum=0.001).double()
    with torch.no_grad():
        m.weight.copy_(1.0 + 0.1 * torch.randn(8, generator=g, dtype=torch.float64))
        m.bias.copy_(0.1 * torch.randn(8, generator=g, dtype=torch.float64))
        m.running_mean.copy_(0.5 + 0.1 * torch.randn(8, generator=g, dtype=torch.float64))
        m.running_std.copy_(2.0 + 0.1 * torch.rand(8, generator=g, dtype=torch.float64))
    m.num_batches_tracked.fill_(1000000)
    rm, rs = m.running_mean.clone(), m.running_std.clone()
    want = (x - rm[:, None]) / rs[:, None] * m.weight[:, None] + m.bias[:, None]
    got = m.train()(x)
    assert (got - want).abs().max().item() < 1e-12
    assert m.num_batches_tracked.item() == 1000001 and not torch.equal(m.running_mean, rm)
    mu = x.mean((0, 2))
    assert torch.allclose(m.running_mean, rm + 0.001 * (mu - rm), rtol=0, atol=1e-15)
    assert (m.eval()(x) - ((x - m.running_mean[:, None]) / m.running_std[:, None] * m.weight[:, None] + m.bias[:, None])).abs().max().item() < 1e-12
    y2 = m(x.transpose(1, 2).reshape(-1, 8))                                      # [N, C] too
    assert y2.shape == (63, 8)


@pytest.mark.parametrize("KW,valid", [(9, None), (9, 16), (32, 45)])
def test_closed_form_backward_is_autograd(KW, valid):
    """The formulas csrc/convmod_brn.hip implements (dbias = sum g, dweight = r sum(g x0) + d sum g, dx = w r / sig (g - mean g - xt mean(g x0)))
    against float64 autograd through the batch statistics, with every clamp state present; the convolution bias' gradient is below 1e-12."""
    u, w, cbias, weight, bias, ds = BR.core_inputs((2, 70, 12), KW, 5)
    fwd = BR.convmod_brn_ref(u, w, cbias, torch.zeros(12, dtype=torch.float64), torch.ones(12, dtype=torch.float64), weight, bias, 1e-5, 3.0, 5.0,
                             valid=valid)
    rmean, rstd = BR.calibrated_running(fwd["mu"], 1.0 / fwd["isig"])
    dc, dw, db, dcb = BR.convmod_brn_bwd_ref(u, w, cbias, rmean, rstd, weight, bias, ds, 1e-5, 3.0, 5.0, valid)
    dc2, dw2, db2 = BR.convmod_brn_bwd_closed(fwd["c"], rmean, rstd, weight, bias, ds, 1e-5, 3.0, 5.0, valid)
    assert (dc - dc2).abs().max().item() < 1e-12 and (dw - dw2).abs().max().item() < 1e-12 and (db - db2).abs().max().item() < 1e-12
    assert dcb.abs().max().item() < 1e-12
    assert dc.abs().max().item() > 1e-2
    r, d = BR.renorm_factors(fwd["mu"], 1.0 / fwd["isig"], rmean, rstd, 3.0, 5.0)
    assert sorted(set(r.round(decimals=6).tolist())) == [round(1 / 3, 6), 1.0, 3.0] and sorted(set(d.round(decimals=6).tolist())) == [-5.0, 0.0, 0.5, 5.0]
    if valid is not None:
        assert dc[:, valid:].abs().max().item() == 0.0


def test_core_reference_is_the_oracle_module():
    """convmod_brn_ref's norm is BatchRenorm1d's training forward on the convolution output, running statistics included."""
    u, w, cbias, weight, bias, _ = BR.core_inputs((3, 20, 6), 9, 1)
    rm = 0.3 * torch.ones(6, dtype=torch.float64)
    rs = torch.tensor([0.1, 0.5, 1.0, 2.0, 5.0, 0.7], dtype=torch.float64)
    out = BR.convmod_brn_ref(u, w, cbias, rm, rs, weight, bias, 1e-5, 3.0, 5.0, momentum=0.1)
    m = BR.BatchRenorm1d(6, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        m.weight.copy_(weight); m.bias.copy_(bias); m.running_mean.copy_(rm); m.running_std.copy_(rs)
    m.num_batches_tracked.fill_(1000000)
    want = torch.nn.functional.silu(m.train()(out["c"].transpose(1, 2)).transpose(1, 2))
    assert (out["s"] - want).abs().max().item() < 1e-12
    assert (out["running_mean"] - m.running_mean).abs().max().item() < 1e-14 and (out["running_std"] - m.running_std).abs().max().item() < 1e-14


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
def test_loop_oracle_seed_and_calibration(shuffle):
    """The loop tests' premises, checked where no kernel is involved: the calibrated share of active clamps lies in [0.25, 0.9] (5 / 6 by
    construction; 0.828 measured), the oracle's fp32 and float64 runs give the same pseudo-labels at every step at LOOP_SEED, without the
    optimiser step they agree to a quarter of the loop's 1e-3 bar (8.3e-6 measured), and the mode is live: the float64 result differs from
    the eval-mode oracle's by more than the bar (0.53 / 0.55 measured).  WITH the step the fp32 oracle is 1.7e-2 / 7.1e-3 from its float64
    run (printed, not asserted): Adam normalises the rounding noise that is all the conv bias' gradient consists of in this mode
    (batch_renorm_refs.LOOP_SEED's comment), which is why the GPU test takes the float64 run as its reference."""
    import numpy as np
    L = PR.LOOP
    cfg, ref, share = BR.loop_pair()
    assert 0.25 <= share <= 0.9, share
    spec, tok = PR.loop_inputs()

    def run(dt, adapt, lab=None):
        random.seed(17)
        return BR.dynamic_eval_ref(argparse.Namespace(epochs=1, shuffle=shuffle), copy.deepcopy(ref).to(dt), spec.to(dt), L["seq_len"], L["overlap"], tok,
                                   L["num_negatives"], L["lr_args"], generator=torch.Generator().manual_seed(L["mask_seed"]), adapt=adapt,
                                   labels_out=lab)

    labels = [[], []]
    outs = [run(dt, True, lab) for dt, lab in zip((torch.float32, torch.float64), labels)]
    assert labels[0] == labels[1] and len(labels[0]) == 4 and all(labels[0])
    print("share", share, "fp32 vs float64 with the optimiser step", np.abs(outs[0] - outs[1]).max())
    assert np.abs(run(torch.float32, False) - run(torch.float64, False)).max() < 2.5e-4
    random.seed(17)
    ev = PR.dynamic_eval_ref(argparse.Namespace(epochs=1, shuffle=shuffle), copy.deepcopy(ref), spec, L["seq_len"], L["overlap"], tok, L["num_negatives"],
                             L["lr_args"], generator=torch.Generator().manual_seed(L["mask_seed"]))
    assert ev.shape == outs[1].shape and np.abs(ev - outs[1]).max() > 1e-3
