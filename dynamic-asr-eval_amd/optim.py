"""Optimisers of the adaptation step, backed by the fused HIP kernels (dyn_madgrad_step / dyn_adam_step / dyn_adafactor_step).

Same constructor / step() / zero_grad() / state_dict() surface the reference loop uses
(`optimizer = optim(model.parameters(), **lr_args)`, `optimizer.zero_grad()`, `optimizer.step()`,
`optimizer.load_state_dict(optimizer_state)` — reference lcasr/lib.py:494-496,578-581; Adam at
nvidia_ctc/lib.py:43,155-160).  When `params` is the ParamList of our SCConformerXL the whole model is ONE flat
buffer and a step is ONE kernel launch; any other list of CUDA tensors (a foreign torch model) is stepped tensor by
tensor with the same kernel."""
import torch

from . import ops


class ParamList(list):
    """List of parameter views that also carries the flat parameter / gradient buffers they alias."""
    flat_params = None
    flat_grads = None
    offsets = None      # where each view begins in the flat buffers (Adafactor's segment table needs the shapes and these)
    trainable = None    # per view: False for a parameter the model's freeze helpers exclude (its gradient is kept at zero)


class _FlatOptimizer:
    def __init__(self, params, defaults):
        self.defaults = dict(defaults)
        self.k = 0
        if isinstance(params, ParamList) and params.flat_params is not None:
            self._pairs = [(params.flat_params, params.flat_grads)]
            self._foreign = None
        else:
            self._foreign = [p for p in params]
            for p in self._foreign:
                if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32):
                    raise ops.DynError("optimizer: every parameter must be a float32 CUDA tensor (no CPU path)")
            self._pairs = None
        self.state = None

    def _iter_pairs(self):
        if self._pairs is not None:
            return self._pairs
        pairs = []
        for p in self._foreign:
            if getattr(p, "requires_grad", False) is False and p.grad is None:
                continue
            if p.grad is None:
                continue
            if not p.data.is_contiguous():
                raise ops.DynError("optimizer: non-contiguous parameter")
            pairs.append((p.data.view(-1), p.grad.contiguous().view(-1)))
        return pairs

    def zero_grad(self, set_to_none=False):
        if self._pairs is not None:
            for _, g in self._pairs:
                g.zero_()
        else:
            for p in self._foreign:
                p.grad = None

    def _alloc_state(self, pairs, n_bufs):
        if self.state is None:
            self.state = [[torch.empty_like(p) for _ in range(n_bufs)] for p, _ in pairs]

    def state_dict(self):
        return {"k": self.k, "defaults": dict(self.defaults),
                "state": None if self.state is None else [[b.clone() for b in bufs] for bufs in self.state]}

    def load_state_dict(self, sd):
        self.k = sd["k"]
        self.defaults.update(sd.get("defaults", {}))
        self.state = None if sd["state"] is None else [[b.clone() for b in bufs] for bufs in sd["state"]]


class MADGRAD(_FlatOptimizer):
    def __init__(self, params, lr=1e-2, momentum=0.9, weight_decay=0.0, eps=1e-6):
        if momentum < 0 or momentum >= 1:
            raise ValueError(f"Momentum {momentum} must be in the range [0,1)")
        if lr <= 0:
            raise ValueError(f"Learning rate {lr} must be positive")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, eps=eps))

    def step(self, limit=None):
        """`limit` (flat-buffer models only): step just the first `limit` elements — the replicas of a lockstep group that are still
        adapting; a finished recording's weights must not keep drifting towards its dual-averaged iterate."""
        d = self.defaults
        pairs = self._iter_pairs()
        self._alloc_state(pairs, 3)
        for (p, g), (s, nu, x0) in zip(pairs, self.state):
            if limit is not None:
                p, g, s, nu, x0 = p[:limit], g[:limit], s[:limit], nu[:limit], x0[:limit]
            ops.madgrad_step(p, g, s, nu, x0, d["lr"], d["momentum"], d["weight_decay"], d["eps"], self.k)
        self.k += 1

    def step_ranges(self, ranges):
        d = self.defaults
        _step_ranges(self, ranges, 3, lambda p, g, b, k: ops.madgrad_step(p, g, b[0], b[1], b[2], d["lr"], d["momentum"], d["weight_decay"], d["eps"], k))


def _step_ranges(opt, ranges, n_bufs, launch):
    """Shared by MADGRAD / Adam: one launch per (lo, hi, k) run of the flat buffers — the replicas of a lockstep group whose recordings have
    taken the same number of steps form one run (recordings of different lengths over several epochs, or under shuffle, get out of step: each
    keeps its OWN step count, as each would have alone)."""
    pairs = opt._iter_pairs()
    if opt._pairs is None or len(pairs) != 1:
        raise ops.DynError("step_ranges: only for a model's flat parameter buffer")
    opt._alloc_state(pairs, n_bufs)
    (p, g), bufs = pairs[0], opt.state[0]
    for lo, hi, k in ranges:
        launch(p[lo:hi], g[lo:hi], [b[lo:hi] for b in bufs], int(k))
    opt.k = max([opt.k] + [int(k) + 1 for _, _, k in ranges])


class Adam(_FlatOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    def step(self, limit=None):
        d = self.defaults
        pairs = self._iter_pairs()
        self._alloc_state(pairs, 2)
        for (p, g), (m, v) in zip(pairs, self.state):
            if limit is not None:
                p, g, m, v = p[:limit], g[:limit], m[:limit], v[:limit]
            ops.adam_step(p, g, m, v, d["lr"], d["betas"][0], d["betas"][1], d["eps"], d["weight_decay"], self.k)
        self.k += 1

    def step_ranges(self, ranges):
        d = self.defaults
        _step_ranges(self, ranges, 2, lambda p, g, b, k: ops.adam_step(p, g, b[0], b[1], d["lr"], d["betas"][0], d["betas"][1], d["eps"], d["weight_decay"], k))


_ADAFACTOR_PLANS = {}


def _adafactor_plan(device, shapes, offsets):
    """Segment table on the device, its totals and the scratch of a step; shared by every optimiser over the same tensors (the
    consistency loop holds one optimiser per window)."""
    key = (torch.device(device).index, torch.cuda.current_stream(device).cuda_stream, tuple(map(tuple, shapes)), tuple(offsets))
    plan = _ADAFACTOR_PLANS.get(key)
    if plan is None:
        table, totals = ops.adafactor_segments(shapes, offsets)
        if not table:
            raise ops.DynError("Adafactor: no parameter to step")
        seg = torch.tensor(table, dtype=torch.int64).to(device)
        scratch = torch.empty(ops.adafactor_scratch_bytes(totals, len(table)), dtype=torch.uint8, device=device)
        plan = _ADAFACTOR_PLANS[key] = (seg, totals, scratch)
    return plan


class Adafactor(_FlatOptimizer):
    """torch.optim.Adafactor (single-tensor rule, maximize=False) on the GPU: row / column second moments over the last two dimensions
    of every tensor of dimension >= 2, a full second moment for the rest, update clipping by max(1, RMS(update) / d), relative step
    max(eps2, RMS(p)) * min(lr, 1 / sqrt(step)).  Over a model's ParamList the whole model is six launches (segment table built from
    the views' shapes; parameters the model holds frozen are left out, as torch leaves out those without a gradient); any other list
    of CUDA tensors is stepped tensor by tensor."""

    def __init__(self, params, lr=1e-2, beta2_decay=-0.8, eps=(None, 1e-3), d=1.0, weight_decay=0.0):
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 >= beta2_decay:
            raise ValueError(f"beta2_decay should be <= 0 but is: {beta2_decay}")
        if eps[0] is not None and not 0.0 <= eps[0]:
            raise ValueError(f"epsilon1 should be >= 0 but is: {eps[0]}")
        if not 0.0 <= eps[1]:
            raise ValueError(f"epsilon2 should be >= 0 but is: {eps[1]}")
        if not 1.0 <= d:
            raise ValueError(f"Clipping threshold d should be >= 1 but is: {d}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight_decay should be >= 0 but is: {weight_decay}")
        flat = isinstance(params, ParamList) and params.flat_params is not None
        if flat and params.offsets is None:
            raise ops.DynError("Adafactor: the ParamList carries no offsets (it needs every tensor's shape and place in the flat buffer)")
        if flat and params.flat_params.numel() > max(o + p.numel() for o, p in zip(params.offsets, params)) + 63:
            raise ops.DynError("Adafactor: a lockstep group's buffers (several replicas) are not supported")
        if flat:
            keep = params.trainable if params.trainable is not None else [True] * len(params)
            self._shapes = [tuple(p.shape) for p, t in zip(params, keep) if t]
            self._offsets = [int(o) for o, t in zip(params.offsets, keep) if t]
        super().__init__(params, dict(lr=lr, beta2_decay=beta2_decay, eps=tuple(eps), d=d, weight_decay=weight_decay))

    def _launch(self, p, g, state, shapes, offsets):
        d = self.defaults
        seg, totals, scratch = _adafactor_plan(p.device, shapes, offsets)
        ops.adafactor_step(p, g, state, seg, totals, scratch, d["lr"], d["beta2_decay"], d["eps"][0], d["eps"][1], d["d"], d["weight_decay"],
                           self.k + 1)

    def step(self):
        pairs = self._iter_pairs()
        if self._pairs is not None:
            (p, g), = pairs
            if self.state is None:
                _, totals, _ = _adafactor_plan(p.device, self._shapes, self._offsets)
                self.state = [[torch.zeros(totals["n_state"], device=p.device, dtype=torch.float32)]]
            self._launch(p, g, self.state[0][0], self._shapes, self._offsets)
        else:
            # torch keeps a step count per tensor and starts it at the tensor's first gradient; here every tensor with a gradient must
            # have had one at every step so far (the loops never change what is trainable under a live optimiser)
            live = [q for q in self._foreign if q.grad is not None]
            if self.state is None:
                self._live = [id(q) for q in live]
                self.state = [[torch.zeros(ops.adafactor_segments([tuple(q.shape)], [0])[1]["n_state"], device=q.device, dtype=torch.float32)]
                              for q in live]
            elif self._live != [id(q) for q in live]:
                raise ops.DynError("Adafactor: the set of parameters with a gradient changed between steps")
            for (p, g), (st,), q in zip(pairs, self.state, live):
                self._launch(p, g, st, [tuple(q.shape)], [0])
        self.k += 1
