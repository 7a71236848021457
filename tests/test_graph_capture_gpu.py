"""The one hipGraph capture helper both models use (dynamic_asr_eval_amd/_graphs.py::capture), on its own: a two-kernel launch sequence
replayed with new inputs, the GEMM profile parked around the capture, the collector's state restored."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_capture_replays_bit_identically_and_restores_profile_and_collector(cuda):
    from dynamic_asr_eval_amd import _graphs, ops
    N = 1024
    g = torch.Generator().manual_seed(0)
    inputs = [(torch.randn(N, generator=g).to(cuda), torch.randn(N, generator=g).to(cuda)) for _ in range(4)]

    def sequence(x, y):
        ops.axpby(x, y, 2.0, 1.0)           # y = 2 x + y, in place
        return ops.silu(y)

    want = [sequence(x.clone(), y.clone()).clone() for x, y in inputs]      # eager (and every kernel has run once before the capture)
    sx, sy = inputs[0][0].clone(), inputs[0][1].clone()
    inside = {}

    def launch():
        inside["profile"], inside["gc"] = ops.GEMM_PROFILE, gc.isenabled()
        return sequence(sx, sy)

    was_gc = gc.isenabled()
    ops.gemm_profile_start()
    try:
        prof = ops.GEMM_PROFILE
        calls = prof["calls"]
        graph, out = _graphs.capture(torch.cuda.graph_pool_handle(), launch)
        assert ops.GEMM_PROFILE is prof and prof["calls"] == calls
    finally:
        ops.gemm_profile_stop()
    assert inside == {"profile": None, "gc": False}                          # no event records, no collection inside the capture
    assert gc.isenabled() == was_gc
    for (x, y), w in zip(inputs[1:], want[1:]):
        sx.copy_(x)
        sy.copy_(y)
        graph.replay()
        assert torch.equal(out, w)
