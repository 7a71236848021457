"""What the models share that is not arithmetic: ALL parameters of a model in ONE flat fp32 buffer (256-B aligned slots) and all gradients
in a second, so the adaptation step is a single fused launch and snapshot / restore of the weights is one device-to-device copy; the
nn.Module-like surface the loops and optimisers use; the model-owned scratch; the deferred weight-gradient queue of a backward."""
import contextlib
import math
import os

import torch

from . import ops
from .optim import ParamList


def flat_layout(spec):
    """[(name, shape)] -> ({name: (offset, numel, shape)}, n_flat): slots in spec order, each rounded up to 64 floats (256 B)."""
    off, slots = 0, {}
    for name, shape in spec:
        n = math.prod(shape)
        slots[name] = (off, n, shape)
        off += (n + 63) // 64 * 64
    return slots, off


class FlatModel:
    _input = None      # name of forward()'s input in the reference's call surface (`model(audio_signal=...)`)

    def __init__(self, spec, device, replicas=1):
        """`replicas` = R: the buffers are [R, n_flat] (a lockstep group, model.py); P / G are replica 0's views, PR / GR the [R, *shape] views."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.DynError(f"{type(self).__name__} runs only on the HIP path (device must be cuda)")
        self.spec, self.R = list(spec), int(replicas)
        self._slots, self.n_flat = flat_layout(self.spec)
        R, off = self.R, self.n_flat
        self.flat_params = torch.zeros(R * off, device=self.device, dtype=torch.float32)
        self.flat_grads = torch.zeros(R * off, device=self.device, dtype=torch.float32)
        self.P, self.G, self.PR, self.GR = {}, {}, {}, {}
        fp, fg = self.flat_params.view(R, off), self.flat_grads.view(R, off)
        for name, (o, n, shape) in self._slots.items():
            self.P[name] = self.flat_params[o:o + n].view(shape)
            self.G[name] = self.flat_grads[o:o + n].view(shape)
            self.PR[name] = fp[:, o:o + n].view(R, *shape)
            self.GR[name] = fg[:, o:o + n].view(R, *shape)
        self.frozen = set()         # parameter-name prefixes excluded from adaptation
        self.training = False
        self._ws = None             # this model's scratch buffer (ops.use_workspace): never shared with another chain
        self._defer_arena = None
        # the backward's launch-bound weight-gradient / bias-sum reductions as one launch at its end (DYN_DEFER_REDUCE=0: one launch each)
        self.defer_reduces = os.environ.get("DYN_DEFER_REDUCE", "1") != "0"
        # A/B switch: the linear layers' weight gradients (+ bias column sums) of a backward deferred to ONE grouped launch (DYN_GROUPED_WGRAD=0: one each)
        self.grouped_wgrad = os.environ.get("DYN_GROUPED_WGRAD", "1") != "0"
        self._wq = None

    # ------------------------------------------------------------------ nn.Module-like surface
    def named_parameters(self):
        return [(n, self.P[n]) for n, _ in self.spec]

    def _flat_range(self):
        """(lo, hi) of the flat buffers an optimiser steps: all of them (a lockstep group narrows this to its active replicas)."""
        return 0, self.R * self.n_flat

    def parameters(self):
        pl = ParamList(self.P[n] for n, _ in self.spec)
        lo, hi = self._flat_range()
        pl.flat_params, pl.flat_grads = self.flat_params[lo:hi], self.flat_grads[lo:hi]
        pl.offsets = [self._slots[n][0] for n, _ in self.spec]
        pl.trainable = [self.trainable(n) for n, _ in self.spec]
        return pl

    def grads(self):
        return [self.G[n] for n, _ in self.spec]

    def zero_grad(self):
        self.flat_grads.zero_()

    def trainable(self, name):
        return not name.startswith(tuple(self.frozen))      # one C-level scan: adapter_only() freezes hundreds of names

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        self.training = mode
        return self

    def to(self, device):
        if torch.device(device) != self.device and torch.device(device).type != "cuda":
            raise ops.DynError(f"{type(self).__name__} cannot leave the GPU: there is no CPU path")
        return self

    def __call__(self, x=None, **kw):
        return self.forward(kw.get(self._input, x))

    # ------------------------------------------------------------------ scratch, deferred work of a backward
    def _scratch(self):
        if self._ws is None:        # the model's own scratch: a stream-keyed buffer is wrong inside a capture
            self._ws = torch.empty(ops.WORKSPACE_BYTES * self.R, dtype=torch.uint8, device=self.device)
            ops.counters(self._ws)          # zeroed arrival counters of this replica's GEMMs, allocated outside any graph capture
            if self.defer_reduces:          # partial sums of the backward's deferred column reductions (ops.reduce_defer)
                self._defer_arena = torch.empty(ops.DEFER_ARENA_BYTES * self.R, dtype=torch.uint8, device=self.device)
        return self._ws

    def _reduce_defer(self):
        return ops.reduce_defer(self._defer_arena if self.defer_reduces else None)

    @contextlib.contextmanager
    def _wgrad_queue(self, on=True):
        """Opens the deferred weight-gradient queue `_wq` (None with `on` false: every product launches at once) for the layers of one backward,
        flushes it as ONE grouped launch, and always closes it.  Operands of a queued descriptor must stay unmodified until the flush."""
        self._wq = [] if on else None
        try:
            yield
            if self._wq:
                ops.gemm_grouped(self._wq)
        finally:
            self._wq = None
