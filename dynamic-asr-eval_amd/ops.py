"""Thin tensor-level wrappers over the C-ABI (include/dyneval.h).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic op on the product path is a
hand-written HIP kernel reached through ctypes.  Wrappers validate device/dtype/contiguity/alignment on the host so
a kernel never sees a shape it does not expect.  There is no CPU fallback: a CPU tensor raises DynError."""
import ctypes

import torch

from . import _lib
from ._lib import DynError, GemmDesc, check

_WS = {}
WORKSPACE_BYTES = 1 << 30
F32 = torch.float32
I32 = torch.int32


def _L():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype=F32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DynError(f"{name}: expected a CUDA tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise DynError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def _cc(t, name, dtype=F32):
    _chk(t, name, dtype)
    if not t.is_contiguous():
        raise DynError(f"{name}: expected a contiguous tensor")
    if t.data_ptr() % 16:
        raise DynError(f"{name}: expected a 16-byte aligned tensor")
    return t


def _c(t, name, dtype=F32):
    """Contiguous but not necessarily 16-byte aligned (kernels with scalar accesses only)."""
    _chk(t, name, dtype)
    if not t.is_contiguous():
        raise DynError(f"{name}: expected a contiguous tensor")
    return t


def _opt(t, name, dtype=F32):
    return 0 if t is None else _cc(t, name, dtype).data_ptr()


class GroupParam:
    """A parameter (or its gradient) of a LOCKSTEP GROUP: R recordings advance through the same window step in one batch, each with its own
    adapted weights (model.SCConformerXL(group=R)).  `t` is the [R, *shape] view into the group's flat buffer, replicas `stride` elements
    apart.  Batches are ordered sample = chunk * R + replica, so sample s belongs to replica s % R."""
    __slots__ = ("t", "R", "stride")

    def __init__(self, t, R, stride):
        self.t, self.R, self.stride = t, int(R), int(stride)

    @property
    def shape(self):
        return self.t.shape[1:]

    def __getitem__(self, r):
        return self.t[r]

    def data_ptr(self):
        return self.t.data_ptr()


def _is_group(p):
    return isinstance(p, GroupParam)


_WS_OWNER = None   # scratch buffer of the model whose forward/backward is being launched or captured (use_workspace)


class use_workspace:
    """Route every op's scratch to `ws` while a model launches (or captures) its kernels.  A stream-keyed lookup is wrong
    inside a hipGraph capture: torch captures on its own side stream, so two models' graphs would be handed the same
    scratch buffer and race when their replays overlap on different streams."""

    def __init__(self, ws):
        self.ws = ws

    def __enter__(self):
        global _WS_OWNER
        self.prev, _WS_OWNER = _WS_OWNER, self.ws

    def __exit__(self, *exc):
        global _WS_OWNER
        _WS_OWNER = self.prev


def workspace(device=None):
    """Caller-owned scratch (split-K slabs, partial reductions, CTC lattice): the launching model's own buffer inside
    use_workspace(), otherwise one buffer per (device, stream) — concurrent recording chains must not share scratch."""
    if _WS_OWNER is not None:
        return _WS_OWNER
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        _WS[key] = ws
        counters(ws)
    return ws


import os as _os

_COUNTERS = {}
N_COUNTERS = 16384
TICKET_DEFAULT = _os.environ.get("DYN_GEMM_TICKET", "0") == "1"


def counters(ws):
    """Arrival counters of the GEMM's in-kernel K-slice combine, one zeroed int32 buffer per scratch buffer (so per model replica /
    stream: concurrent chains never share them)."""
    key = ws.data_ptr()
    c = _COUNTERS.get(key)
    if c is None:
        c = torch.zeros(N_COUNTERS, dtype=torch.int32, device=ws.device)
        _COUNTERS[key] = c
    return c


# ----------------------------------------------------------------------------------------------- GEMM
def gemm(a, b, c, *, trans_a=False, trans_b=False, M, N, K, lda, ldb, ldc, alpha=1.0, beta=0.0, bias=None,
         nb1=1, nb2=1, sa=(0, 0), sb=(0, 0), sc=(0, 0), a_off=0, b_off=0, c_off=0, split_k=0, force=None, c_in=None,
         epilogue=0, aux=None, ticket=None, sbias=(0, 0)):
    """Raw strided batched GEMM (see dyn_gemm_desc). Offsets are in elements from each tensor's data_ptr.
    `force=(tile_m, tile_n, tail_slices)` pins the kernel configuration (autotuner / tests).
    `epilogue`: 0 none, EPI_SILU (C = silu(v), aux = v if given), EPI_SILU_GRAD (C = v * silu'(aux)); aux addressed like C."""
    _chk(a, "gemm.A"); _chk(b, "gemm.B"); _chk(c, "gemm.C")
    d = GemmDesc()
    if force is not None:
        d.tile_m, d.tile_n, d.tail_slices = force
    d.trans_a, d.trans_b = int(trans_a), int(trans_b)
    d.M, d.N, d.K = M, N, K
    d.alpha, d.beta = alpha, beta
    d.A, d.lda, d.sa1, d.sa2 = a.data_ptr() + 4 * a_off, lda, sa[0], sa[1]
    d.B, d.ldb, d.sb1, d.sb2 = b.data_ptr() + 4 * b_off, ldb, sb[0], sb[1]
    d.C, d.ldc, d.sc1, d.sc2 = c.data_ptr() + 4 * c_off, ldc, sc[0], sc[1]
    d.bias = bias.data_ptr() if bias is not None else None
    d.bias_s1, d.bias_s2 = sbias
    d.C_in = (c_in.data_ptr() + 4 * c_off) if c_in is not None else None   # residual source (same addressing as C)
    d.nb1, d.nb2 = nb1, nb2
    d.split_k = split_k
    d.epilogue = int(epilogue)
    d.aux = (aux.data_ptr() + 4 * c_off) if aux is not None else None
    ws = workspace(c.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if ticket is None:
        ticket = TICKET_DEFAULT
    if ticket:       # in-kernel combine of K slices instead of the separate reduce pass (opt-in: DYN_GEMM_TICKET=1; see gemm_f32.hip)
        cnt = counters(ws)
        d.counters, d.n_counters = cnt.data_ptr(), cnt.numel()
    prof = GEMM_PROFILE
    if prof is not None:
        prof["calls"] += 1
        prof["flops"] += 2.0 * M * N * K * nb1 * nb2
        prof["bytes"] += 4.0 * nb1 * nb2 * (M * K + K * N + M * N * (2 if beta != 0.0 else 1))  # algorithmic operand bytes
        if prof["calls"] % prof["every"] == 0:  # HIP events on the launch stream around this one launch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(_L().dyn_gemm_f32(ctypes.byref(d), _stream()), "dyn_gemm_f32")
            e1.record()
            prof["samples_excl" if prof.get("exclusive_now") else "samples"].append((2.0 * M * N * K * nb1 * nb2, e0, e1))
            return c
    check(_L().dyn_gemm_f32(ctypes.byref(d), _stream()), "dyn_gemm_f32")
    return c


EPI_SILU, EPI_SILU_GRAD = 1, 2


def wgrad_desc(dy, x, dw, alpha=1.0, beta=1.0, colsum=None, colsum_beta=1.0):
    """Descriptor of dw[N, K] = alpha * dy[M, N]^T @ x[M, K] + beta * dw for gemm_grouped; `colsum` [N] also receives
    colsum_beta * colsum + column sums of dy (the bias gradient).  The tensors must stay alive and unmodified until the launch."""
    _cc(dy, "wgrad.dy"); _cc(x, "wgrad.x"); _cc(dw, "wgrad.dw")
    N, K = dw.shape
    M = dy.numel() // N
    d = GemmDesc()
    d.trans_a, d.trans_b = 1, 0
    d.M, d.N, d.K = N, K, M
    d.alpha, d.beta = alpha, beta
    d.A, d.lda = dy.data_ptr(), N
    d.B, d.ldb = x.data_ptr(), K
    d.C, d.ldc = dw.data_ptr(), K
    d.nb1 = d.nb2 = 1
    if colsum is not None:
        _cc(colsum, "wgrad.colsum")
        d.a_colsum, d.a_colsum_beta = colsum.data_ptr(), colsum_beta
    d._keep = (dy, x, dw, colsum)
    return d


MAX_GROUPS = 96     # kMaxGroups of csrc/gemm_f32.hip: descriptors per dyn_gemm_f32_grouped launch


def wgrad_groupable(dy, x, dw):
    """True when dw = dy^T @ x may ride in the grouped launch: dyn_gemm_f32_grouped has only the 16-byte vector staging, so it
    needs leading dimensions that are multiples of 4 (the single-GEMM path degrades to scalar staging instead of failing)."""
    N, K = dw.shape
    return N % 4 == 0 and K % 4 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0


def gemm_grouped(descs):
    """One launch over the 128x128 tiles of all `descs` (dyn_gemm_f32_grouped): the deferred weight gradients of a backward pass.
    More than MAX_GROUPS descriptors (8 per conformer block + 1: from 12 blocks on) go out in slices of MAX_GROUPS; the slices are
    stream-ordered, so they can share the descriptor-table workspace."""
    if len(descs) > MAX_GROUPS:
        for i in range(0, len(descs), MAX_GROUPS):
            gemm_grouped(descs[i:i + MAX_GROUPS])
        return
    n = len(descs)
    if n == 0:
        return
    arr = (GemmDesc * n)(*descs)
    ws = workspace()
    prof = GEMM_PROFILE
    fl = sum(2.0 * d.M * d.N * d.K for d in descs)
    if prof is not None:
        prof["calls"] += 1
        prof["flops"] += fl
        prof["bytes"] += sum(4.0 * (d.M * d.K + d.K * d.N + 2 * d.M * d.N) for d in descs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_L().dyn_gemm_f32_grouped(arr, n, ws.data_ptr(), ws.numel(), _stream()), "dyn_gemm_f32_grouped")
        e1.record()
        prof["samples_excl" if prof.get("exclusive_now") else "samples"].append((fl, e0, e1))
        return
    check(_L().dyn_gemm_f32_grouped(arr, n, ws.data_ptr(), ws.numel(), _stream()), "dyn_gemm_f32_grouped")


GEMM_PROFILE = None


def GEMM_PROFILE_EAGER():
    """True while bench.py's per-launch HIP-event sampling wants THIS model call to run eagerly (graph replays cannot be
    timed launch by launch): every `window_every`-th forward/backward pair of the timed region."""
    prof = GEMM_PROFILE
    if prof is None or not prof.get("window_every"):
        return False
    return prof["eager_now"]


def gemm_profile_start(every=8, window_every=0):
    """Sample every `every`-th GEMM launch with a HIP-event pair (bench.py's live roofline measurement).  With hipGraph
    replay enabled, `window_every` = n makes every n-th window step run eagerly (gemm_profile_tick) so its launches can
    be sampled; launch counters then cover the eager windows only."""
    global GEMM_PROFILE
    GEMM_PROFILE = {"calls": 0, "flops": 0.0, "bytes": 0.0, "every": int(every), "samples": [], "samples_excl": [],
                    "window_every": int(window_every), "windows": 0, "eager_now": False, "exclusive_now": False}


def gemm_profile_tick():
    """Called once per window step by the dynamic-eval loop: decides whether this step runs eagerly (sampled).
    -> 0 not sampled, 1 sampled as it runs (other chains may share the GPU), 2 sampled EXCLUSIVELY (the caller drains the
    device before and after, so each timed launch has the GPU to itself: the kernel's own duration).  Sampled steps
    alternate between the two kinds; with a single chain both are the same thing."""
    prof = GEMM_PROFILE
    if prof is None or not prof.get("window_every"):
        return 0
    kind = 0
    if prof["windows"] % prof["window_every"] == 0:
        kind = 2 if (prof["windows"] // prof["window_every"]) % 2 == 0 else 1
    prof["windows"] += 1
    return kind


def gemm_profile_mode(kind):
    """Set by the dynamic-eval loop right before each model call of a step (chains interleave on one host thread)."""
    prof = GEMM_PROFILE
    if prof is not None:
        prof["eager_now"] = kind > 0
        prof["exclusive_now"] = kind == 2


def gemm_profile_active():
    """True only while bench.py's sampling is on: the dynamic-eval loop enters its sampling blocks under this test and nowhere else."""
    return GEMM_PROFILE is not None


def gemm_profile_begin_step(device):
    """Start of a window step (or final-pass batch): -> 0 not sampled / 1 sampled shared / 2 sampled exclusively (device drained first)."""
    kind = gemm_profile_tick()
    if kind == 2:
        torch.cuda.synchronize(device)           # exclusive sample: the other chains' queued work drains first
    gemm_profile_mode(kind)
    return kind


def gemm_profile_before_yield(kind, ready_event):
    if kind == 2:
        ready_event.synchronize()                # keep the device to this chain until its forward has finished


def gemm_profile_resume_step(device, kind):
    """After the yield of a sampled step: other chains may have queued work meanwhile; the mode is per model call."""
    if kind == 2:
        torch.cuda.synchronize(device)
    gemm_profile_mode(kind)


def gemm_profile_end_step(device, kind):
    if kind == 2:
        torch.cuda.current_stream(device).synchronize()
    gemm_profile_mode(0)


def gemm_profile_stop():
    """-> dict(calls, flops, sampled, sampled_flops, sampled_ms): call after a stream synchronize."""
    global GEMM_PROFILE
    prof, GEMM_PROFILE = GEMM_PROFILE, None
    if prof is None:
        return None
    out = {"calls": prof["calls"], "flops": prof["flops"], "bytes": prof["bytes"], "attn_flops": prof.get("attn_flops", 0.0),
           "sampled_steps": (prof["windows"] + prof["window_every"] - 1) // prof["window_every"] if prof.get("window_every") else prof.get("windows", 0)}
    for key, name in (("samples", "shared"), ("samples_excl", "exclusive")):
        out[name] = {"sampled": len(prof[key]), "flops": sum(s[0] for s in prof[key]),
                     "ms": sum(s[1].elapsed_time(s[2]) for s in prof[key])}
    return out


def linear(x, w, bias=None, out=None, alpha=1.0, beta=0.0, residual=None, epilogue=0, aux=None):
    """out[M, N] = alpha * x[M, K] @ w[N, K]^T + beta * (residual if given else out) + bias   (torch.nn.Linear layout);
    with epilogue=EPI_SILU: out = silu(that) and aux (if given) = that."""
    if _is_group(w):
        return _linear_group(x, w, bias, out, alpha, beta, residual, epilogue, aux)
    _cc(x, "linear.x"); _cc(w, "linear.w")
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    assert w.shape[1] == K, (w.shape, K)
    if out is None:
        assert beta == 0.0 or residual is not None
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=F32)
    return gemm(x, w, out, trans_b=True, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, alpha=alpha, beta=beta, c_in=residual,
                epilogue=epilogue, aux=aux)


def _group_dims(x, R, what):
    """x [S, ..., K] with S = chunks * R samples (sample = chunk * R + replica) -> (chunks, rows per sample)."""
    S = x.shape[0]
    if S % R:
        raise DynError(f"{what}: batch {S} is not a multiple of the group size {R}")
    return S // R, x.numel() // (S * x.shape[-1])


def _linear_group(x, w, bias, out, alpha, beta, residual, epilogue, aux):
    """linear() over a lockstep group: ONE batched product, batch = (chunk, replica); replica r multiplies its own rows with its own weight
    (B operand and bias step through the group's flat parameter buffer with the replica stride)."""
    _cc(x, "linear.x")
    R = w.R
    N, K = w.shape
    assert x.shape[-1] == K, (x.shape, K)
    nch, M = _group_dims(x, R, "linear")
    if out is None:
        assert beta == 0.0 or residual is not None
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=F32)
    return gemm(x, w.t, out, trans_b=True, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=None if bias is None else bias.t, alpha=alpha, beta=beta,
                c_in=residual, epilogue=epilogue, aux=aux, nb1=nch, nb2=R, sa=(R * M * K, M * K), sb=(0, w.stride), sc=(R * M * N, M * N),
                sbias=(0, 0 if bias is None else bias.stride))


def linear_dgrad(dy, w, out=None, alpha=1.0, beta=0.0, epilogue=0, aux=None):
    """dx[M, K] = alpha * dy[M, N] @ w[N, K] + beta * dx; with epilogue=EPI_SILU_GRAD: dx *= silu'(aux) (aux = the pre-activation)."""
    if _is_group(w):
        _cc(dy, "linear_dgrad.dy")
        R = w.R
        N, K = w.shape
        nch, M = _group_dims(dy, R, "linear_dgrad")
        if out is None:
            assert beta == 0.0
            out = torch.empty(*dy.shape[:-1], K, device=dy.device, dtype=F32)
        return gemm(dy, w.t, out, M=M, N=K, K=N, lda=N, ldb=K, ldc=K, alpha=alpha, beta=beta, epilogue=epilogue, aux=aux, nb1=nch, nb2=R,
                    sa=(R * M * N, M * N), sb=(0, w.stride), sc=(R * M * K, M * K))
    _cc(dy, "linear_dgrad.dy"); _cc(w, "linear_dgrad.w")
    N, K = w.shape
    M = dy.numel() // N
    if out is None:
        assert beta == 0.0
        out = torch.empty(*dy.shape[:-1], K, device=dy.device, dtype=F32)
    return gemm(dy, w, out, M=M, N=K, K=N, lda=N, ldb=K, ldc=K, alpha=alpha, beta=beta, epilogue=epilogue, aux=aux)


def linear_wgrad(dy, x, dw, alpha=1.0, beta=1.0):
    """dw[N, K] = alpha * dy[M, N]^T @ x[M, K] + beta * dw   (deterministic split-K)."""
    _cc(dy, "linear_wgrad.dy"); _cc(x, "linear_wgrad.x"); _cc(dw, "linear_wgrad.dw")
    N, K = dw.shape
    M = dy.numel() // N
    return gemm(dy, x, dw, trans_a=True, M=N, N=K, K=M, lda=N, ldb=K, ldc=K, alpha=alpha, beta=beta)


# ----------------------------------------------------------------------------------------------- elementwise
def silu(x, out=None):
    _cc(x, "silu.x")
    out = torch.empty_like(x) if out is None else _cc(out, "silu.out")
    check(_L().dyn_silu_fwd(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_silu_fwd")
    return out


def silu_bwd(x, dy, out=None):
    _cc(x, "silu_bwd.x"); _cc(dy, "silu_bwd.dy")
    out = torch.empty_like(x) if out is None else _cc(out, "silu_bwd.out")
    check(_L().dyn_silu_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_silu_bwd")
    return out


def glu(u, out=None):
    _cc(u, "glu.u")
    C = u.shape[-1] // 2
    rows = u.numel() // (2 * C)
    out = torch.empty(*u.shape[:-1], C, device=u.device, dtype=F32) if out is None else _cc(out, "glu.out")
    check(_L().dyn_glu_fwd(u.data_ptr(), out.data_ptr(), rows, C, _stream()), "dyn_glu_fwd")
    return out


def glu_bwd(u, dy, out=None):
    _cc(u, "glu_bwd.u"); _cc(dy, "glu_bwd.dy")
    C = u.shape[-1] // 2
    rows = u.numel() // (2 * C)
    out = torch.empty_like(u) if out is None else _cc(out, "glu_bwd.out")
    check(_L().dyn_glu_bwd(u.data_ptr(), dy.data_ptr(), out.data_ptr(), rows, C, _stream()), "dyn_glu_bwd")
    return out


def axpby(x, y, a=1.0, b=1.0):
    """y = a * x + b * y (in place on y)."""
    _cc(x, "axpby.x"); _cc(y, "axpby.y")
    assert x.numel() == y.numel()
    check(_L().dyn_axpby(x.data_ptr(), y.data_ptr(), a, b, x.numel(), _stream()), "dyn_axpby")
    return y


def reduce_partials(partial, out, beta=1.0):
    """out[n] = beta * out[n] + sum_p partial[p, n] (deterministic: p in increasing order per column)."""
    _cc(partial, "reduce_partials.partial"); _cc(out, "reduce_partials.out")
    n = out.numel()
    P = partial.numel() // n
    assert P * n == partial.numel()
    check(_L().dyn_reduce_partials(partial.data_ptr(), out.data_ptr(), P, n, beta, _stream()), "dyn_reduce_partials")
    return out


DEFER_ARENA_BYTES = 160 << 20


class reduce_defer:
    """`with ops.reduce_defer(arena):` — the weight-gradient / bias-sum reductions of the backward kernels launched inside are recorded
    and run as one launch per 96 at exit (dyn_reduce_defer_begin / _flush; bit-identical).  Nothing inside may read those gradients; the
    block must not span a `yield` (the context is per host thread).  `arena=None`: no deferral."""

    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        if self.arena is not None:
            check(_L().dyn_reduce_defer_begin(self.arena.data_ptr(), self.arena.numel()), "dyn_reduce_defer_begin")
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.arena is None:
            return False
        if exc_type is not None:
            _L().dyn_reduce_defer_abort()
            return False
        check(_L().dyn_reduce_defer_flush(_stream()), "dyn_reduce_defer_flush")
        return False


def colsum(x, out, beta=1.0):
    """out[C] = beta * out + sum over rows of x[rows, C]."""
    _cc(x, "colsum.x"); _cc(out, "colsum.out")
    C = out.numel()
    rows = x.numel() // C
    ws = workspace(x.device)
    check(_L().dyn_colsum(x.data_ptr(), out.data_ptr(), rows, C, beta, ws.data_ptr(), ws.numel(), _stream()), "dyn_colsum")
    return out


def transpose_ft(x, out=None):
    """[F, T] window view (T contiguous, arbitrary row stride) -> contiguous [T, F]."""
    _chk(x, "transpose_ft.x")
    F, T = x.shape
    assert x.stride(1) == 1
    out = torch.empty(T, F, device=x.device, dtype=F32) if out is None else _cc(out, "transpose_ft.out")
    check(_L().dyn_transpose_ft(x.data_ptr(), out.data_ptr(), F, T, x.stride(0), _stream()), "dyn_transpose_ft")
    return out


def specaug_freqmask(x, f0, width, value=0.0):
    """In-place frequency masks on a contiguous [F, T] window; f0/width are int32 CUDA tensors; `value` may be a float or
    a 1-element CUDA tensor (device-side fill value: no host round trip)."""
    _cc(x, "specaug.x"); _cc(f0, "specaug.f0", I32); _cc(width, "specaug.width", I32)
    F, T = x.shape
    vdev = value.data_ptr() if isinstance(value, torch.Tensor) else 0
    check(_L().dyn_specaug_freqmask(x.data_ptr(), F, T, f0.data_ptr(), width.data_ptr(), f0.numel(), 0.0 if vdev else value, vdev, _stream()),
          "dyn_specaug_freqmask")
    return x


def specaug_timemask(x, t0, width, value=0.0):
    """In-place time masks on a contiguous [F, T] window."""
    _cc(x, "specaug.x"); _cc(t0, "specaug.t0", I32); _cc(width, "specaug.width", I32)
    F, T = x.shape
    vdev = value.data_ptr() if isinstance(value, torch.Tensor) else 0
    check(_L().dyn_specaug_timemask(x.data_ptr(), F, T, t0.data_ptr(), width.data_ptr(), t0.numel(), 0.0 if vdev else value, vdev, _stream()),
          "dyn_specaug_timemask")
    return x


ATTN_NSPLIT_DEFAULT = int(_os.environ.get("DYN_ATTN_NSPLIT", "0"))


def attention_fwd(qkv, B, T, H, D, scale, out=None, want_lse=False, nsplit=0):
    """Fused attention on the packed [B, T, 3 * H * D] QKV activation (q | k | v, head h at +h * D) -> [B, T, H * D];
    with `want_lse` (grad mode) returns (out, lse [B, H, T]) for attention_bwd.  `nsplit`: key splits per query block (0 = chosen
    by the library from the launch size, 1 = none): launches that do not fill the chip get nsplit x the workgroups, the partial
    outputs go through the caller's workspace and are merged in split order."""
    _cc(qkv, "attention.qkv")
    HD = H * D
    out = torch.empty(B, T, HD, device=qkv.device, dtype=F32) if out is None else out
    if GEMM_PROFILE is not None:
        GEMM_PROFILE["attn_flops"] = GEMM_PROFILE.get("attn_flops", 0.0) + 4.0 * B * H * T * T * D   # matrix-core work outside dyn_gemm_f32
    base = qkv.data_ptr()
    lse = torch.empty(B, H, T, device=qkv.device, dtype=F32) if want_lse else None
    if nsplit == 0 and ATTN_NSPLIT_DEFAULT:
        nsplit = ATTN_NSPLIT_DEFAULT     # A/B switch only (DYN_ATTN_NSPLIT=1: never split)
    ws = workspace(qkv.device)
    need = _L().dyn_attention_fwd_split_workspace_bytes(B, T, H, nsplit)
    if need > ws.numel():
        nsplit = 1                      # scratch too small for the slabs (very long windows): the unsplit launch needs none
    check(_L().dyn_attention_fwd_split(base, base + 4 * HD, base + 8 * HD, out.data_ptr(), 0 if lse is None else lse.data_ptr(), B, T, H, D,
                                       3 * HD, T * 3 * HD, HD, T * HD, scale, nsplit, ws.data_ptr(), ws.numel(), _stream()), "dyn_attention_fwd_split")
    return (out, lse) if want_lse else out


def attention_bwd(qkv, out, dout, lse, B, T, H, D, scale, dqkv=None):
    """Backward of attention_fwd: (packed qkv, out, dout [B, T, H * D], lse [B, H, T]) -> packed dqkv [B, T, 3 * H * D]."""
    _cc(qkv, "attention_bwd.qkv"); _cc(out, "attention_bwd.out"); _cc(dout, "attention_bwd.dout"); _cc(lse, "attention_bwd.lse")
    HD = H * D
    dqkv = torch.empty_like(qkv) if dqkv is None else _cc(dqkv, "attention_bwd.dqkv")
    delta = torch.empty(B, H, T, device=qkv.device, dtype=F32)
    if GEMM_PROFILE is not None:
        GEMM_PROFILE["attn_flops"] = GEMM_PROFILE.get("attn_flops", 0.0) + 14.0 * B * H * T * T * D   # 3 + 4 products (P is re-formed twice)
    base, g = qkv.data_ptr(), dqkv.data_ptr()
    check(_L().dyn_attention_bwd(base, base + 4 * HD, base + 8 * HD, out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                 g, g + 4 * HD, g + 8 * HD, B, T, H, D, 3 * HD, T * 3 * HD, HD, T * HD, 3 * HD, T * 3 * HD, scale, _stream()),
          "dyn_attention_bwd")
    return dqkv


# ----------------------------------------------------------------------------------------------- norms
def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _cc(x, "layernorm.x")
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty_like(x) if out is None else _cc(out, "layernorm.out")
    mean = torch.empty(rows, device=x.device, dtype=F32)
    rstd = torch.empty(rows, device=x.device, dtype=F32)
    if _is_group(gamma):       # lockstep group: sample s of x [S, T, C] is normalised with replica s % R's weights, one launch
        _, rps = _group_dims(x, gamma.R, "layernorm")
        check(_L().dyn_layernorm_fwd_g(x.data_ptr(), gamma.data_ptr(), 0 if beta is None else beta.data_ptr(), out.data_ptr(), mean.data_ptr(),
                                       rstd.data_ptr(), rows, C, eps, rps, gamma.R, gamma.stride, _stream()), "dyn_layernorm_fwd_g")
        return out, mean, rstd
    _cc(gamma, "layernorm.gamma")
    check(_L().dyn_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), _opt(beta, "layernorm.beta"), out.data_ptr(),
                                 mean.data_ptr(), rstd.data_ptr(), rows, C, eps, _stream()), "dyn_layernorm_fwd")
    return out, mean, rstd


def layernorm_bwd(x, gamma, mean, rstd, dy, dx, dgamma, dbeta, dx_beta=0.0, wgrad_beta=1.0, dx_in=None):
    """dx = norm_bwd(dy) + dx_beta * (dx_in if given else dx)."""
    _cc(x, "layernorm_bwd.x"); _cc(dy, "layernorm_bwd.dy"); _cc(dx, "layernorm_bwd.dx")
    C = x.shape[-1]
    rows = x.numel() // C
    ws = workspace(x.device)
    if _is_group(gamma):
        _, rps = _group_dims(x, gamma.R, "layernorm_bwd")
        src = dx if dx_in is None else _cc(dx_in, "layernorm_bwd.dx_in")
        check(_L().dyn_layernorm_bwd_g(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), src.data_ptr(),
                                       dx.data_ptr(), dx_beta, 0 if dgamma is None else dgamma.data_ptr(), 0 if dbeta is None else dbeta.data_ptr(),
                                       wgrad_beta, rows, C, rps, gamma.R, gamma.stride, ws.data_ptr(), ws.numel(), _stream()), "dyn_layernorm_bwd_g")
        return dx
    if dx_in is not None:
        _cc(dx_in, "layernorm_bwd.dx_in")
        check(_L().dyn_layernorm_bwd_res(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), dx_in.data_ptr(),
                                         dx.data_ptr(), dx_beta, _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), wgrad_beta, rows, C,
                                         ws.data_ptr(), ws.numel(), _stream()), "dyn_layernorm_bwd_res")
        return dx
    check(_L().dyn_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(),
                                 dx.data_ptr(), dx_beta, _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), wgrad_beta, rows, C,
                                 ws.data_ptr(), ws.numel(), _stream()), "dyn_layernorm_bwd")
    return dx


def chanaffine(x, mean, var, weight, bias, eps=1e-5, out=None):
    """BatchRenorm1d in eval mode: (x - mean_c) * rsqrt(var_c + eps) * weight_c + bias_c over the last dim."""
    _c(x, "chanaffine.x")
    C = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    check(_L().dyn_chanaffine_fwd(x.data_ptr(), mean.data_ptr(), var.data_ptr(), weight.data_ptr(), _opt(bias, "bias") if bias is not None else 0,
                                  out.data_ptr(), x.numel() // C, C, eps, _stream()), "dyn_chanaffine_fwd")
    return out


def chanaffine_bwd(x, mean, var, weight, dy, dx, dweight, dbias, eps=1e-5, dx_beta=0.0, wgrad_beta=1.0):
    _c(x, "chanaffine_bwd.x"); _c(dy, "chanaffine_bwd.dy"); _c(dx, "chanaffine_bwd.dx")
    C = x.shape[-1]
    ws = workspace(x.device)
    check(_L().dyn_chanaffine_bwd(x.data_ptr(), mean.data_ptr(), var.data_ptr(), weight.data_ptr(), dy.data_ptr(), dx.data_ptr(), dx_beta,
                                  0 if dweight is None else dweight.data_ptr(), 0 if dbias is None else dbias.data_ptr(), wgrad_beta,
                                  x.numel() // C, C, eps, ws.data_ptr(), ws.numel(), _stream()), "dyn_chanaffine_bwd")
    return dx


def rmsnorm(x, gamma, eps=1e-5, out=None):
    _cc(x, "rmsnorm.x"); _cc(gamma, "rmsnorm.gamma")
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty_like(x) if out is None else _cc(out, "rmsnorm.out")
    rstd = torch.empty(rows, device=x.device, dtype=F32)
    check(_L().dyn_rmsnorm_fwd(x.data_ptr(), gamma.data_ptr(), out.data_ptr(), rstd.data_ptr(), rows, C, eps, _stream()),
          "dyn_rmsnorm_fwd")
    return out, rstd


def rmsnorm_bwd(x, gamma, rstd, dy, dx, dgamma, dx_beta=0.0, wgrad_beta=1.0):
    _cc(x, "rmsnorm_bwd.x"); _cc(dy, "rmsnorm_bwd.dy"); _cc(dx, "rmsnorm_bwd.dx")
    C = x.shape[-1]
    rows = x.numel() // C
    ws = workspace(x.device)
    if _is_group(gamma):
        _, rps = _group_dims(x, gamma.R, "rmsnorm_bwd")
        check(_L().dyn_rmsnorm_bwd_g(x.data_ptr(), gamma.data_ptr(), rstd.data_ptr(), dy.data_ptr(), dx.data_ptr(), dx_beta,
                                     0 if dgamma is None else dgamma.data_ptr(), wgrad_beta, rows, C, rps, gamma.R, gamma.stride,
                                     ws.data_ptr(), ws.numel(), _stream()), "dyn_rmsnorm_bwd_g")
        return dx
    check(_L().dyn_rmsnorm_bwd(x.data_ptr(), gamma.data_ptr(), rstd.data_ptr(), dy.data_ptr(), dx.data_ptr(), dx_beta,
                               _opt(dgamma, "dgamma"), wgrad_beta, rows, C, ws.data_ptr(), ws.numel(), _stream()),
          "dyn_rmsnorm_bwd")
    return dx


# ----------------------------------------------------------------------------------------------- softmax
def _rows_L(x):
    L = x.shape[-1]
    return x.numel() // L, L


def softmax(x, out=None, valid=None, lens=None):
    """Row softmax; `valid` (device int32 scalar): columns >= valid are masked keys (probability 0); `lens` (int32 CUDA [B], x [B, ..., L]):
    lens[b] keys in every row of batch entry b."""
    _cc(x, "softmax.x")
    rows, L = _rows_L(x)
    out = torch.empty_like(x) if out is None else _cc(out, "softmax.out")
    valid, lens = _split_valid(valid, lens)
    if lens is not None:
        if x.dim() < 3:
            raise DynError("softmax: lens needs x as [B, ..., L]")
        B = x.shape[0]
        check(_L().dyn_softmax_fwd_lens(x.data_ptr(), out.data_ptr(), B, rows // max(B, 1), L, L, L, _lens_ptr(lens, B, "softmax", valid), _stream()),
              "dyn_softmax_fwd_lens")
        return out
    if valid is not None:
        check(_L().dyn_softmax_fwd_len(x.data_ptr(), out.data_ptr(), rows, L, L, L, _valid_ptr(valid, "softmax"), _stream()), "dyn_softmax_fwd_len")
        return out
    check(_L().dyn_softmax_fwd(x.data_ptr(), out.data_ptr(), rows, L, L, L, _stream()), "dyn_softmax_fwd")
    return out


def softmax_bwd(y, dy, out=None, scale=1.0):
    _cc(y, "softmax_bwd.y"); _cc(dy, "softmax_bwd.dy")
    rows, L = _rows_L(y)
    out = torch.empty_like(y) if out is None else _cc(out, "softmax_bwd.out")
    check(_L().dyn_softmax_bwd(y.data_ptr(), dy.data_ptr(), out.data_ptr(), rows, L, L, scale, _stream()), "dyn_softmax_bwd")
    return out


# ----------------------------------------------------------------------------------------------- WavLM gated relative-position bias
def relative_position_buckets(Tmax, num_buckets, max_distance):
    """int32 CPU table [2 Tmax - 1]: entry d + Tmax - 1 is the bucket of the signed distance d = key - query, d in (-Tmax, Tmax).  The
    expressions are those of transformers' WavLMAttention._relative_positions_bucket, evaluated by torch on the host: the logarithmic half
    goes through a float32 log and a truncation, so any other evaluation can land in the neighbouring bucket at an edge."""
    import math
    d = torch.arange(-(Tmax - 1), Tmax, dtype=torch.long)
    half = num_buckets // 2
    out = (d > 0).to(torch.long) * half
    d = torch.abs(d)
    max_exact = half // 2
    large = torch.log(d.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (half - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, half - 1))
    return (out + torch.where(d < max_exact, d, large)).to(I32)


def _relbias_dims(who, S, nh, D, E, table):
    if S.dim() != 4 or S.shape[1] != nh or S.shape[2] != S.shape[3]:
        raise DynError(f"{who}: scores must be [B, {nh}, T, T], got {tuple(S.shape)}")
    _cc(E, who + ".E"); _c(table, who + ".table", I32)
    if E.dim() != 2 or E.shape[1] != nh:
        raise DynError(f"{who}: E must be [num_buckets, {nh}], got {tuple(E.shape)}")
    if table.dim() != 1 or table.numel() % 2 != 1:
        raise DynError(f"{who}: the bucket table must hold 2 * Tmax - 1 entries")
    return S.shape[0], S.shape[2], nh * D, (table.numel() + 1) // 2, E.shape[0]


def relpos_gate(h, W, bias, const, nh):
    """WavLM's gate on the relative-position bias: h [B, T, H], W [8, H / nh], bias [8], const [nh] -> (gate, a, c), each [B, nh, T]
    (a, c: the two sigmoids, kept for relpos_gate_bwd)."""
    _cc(h, "relpos_gate.h"); _cc(W, "relpos_gate.W"); _c(bias, "relpos_gate.bias"); _c(const, "relpos_gate.const")
    B, T, H = h.shape
    if H % nh or W.shape != (8, H // nh) or bias.numel() != 8 or const.numel() != nh:
        raise DynError(f"relpos_gate: W {tuple(W.shape)} / bias {tuple(bias.shape)} / const {tuple(const.shape)} do not fit H={H}, heads={nh}")
    gate, a, c = (torch.empty(B, nh, T, device=h.device, dtype=F32) for _ in range(3))
    check(_L().dyn_relpos_gate_fwd(h.data_ptr(), W.data_ptr(), bias.data_ptr(), const.data_ptr(), gate.data_ptr(), a.data_ptr(), c.data_ptr(),
                                   B, T, H, nh, _stream()), "dyn_relpos_gate_fwd")
    return gate, a, c


def relpos_gate_bwd(dgate, a, c, h, W, const, dh, dW, dbias, dconst, dh_beta=1.0, beta=1.0):
    """Backward of relpos_gate: dh [B, T, H] = dh_beta * dh + its gradient (the attention's input gradient), dW / dbias / dconst = beta * old + sums."""
    for t, n in ((dgate, "dgate"), (a, "a"), (c, "c"), (h, "h"), (W, "W"), (dh, "dh"), (dW, "dW")):
        _cc(t, "relpos_gate_bwd." + n)
    _c(const, "relpos_gate_bwd.const"); _c(dbias, "relpos_gate_bwd.dbias"); _c(dconst, "relpos_gate_bwd.dconst")
    B, T, H = h.shape
    nh = const.numel()
    if tuple(dgate.shape) != (B, nh, T) or a.shape != dgate.shape or c.shape != dgate.shape or dh.shape != h.shape or dW.shape != W.shape \
            or dbias.numel() != 8 or dconst.numel() != nh:
        raise DynError("relpos_gate_bwd: operand shapes do not match")
    ws = workspace(h.device)
    check(_L().dyn_relpos_gate_bwd(dgate.data_ptr(), a.data_ptr(), c.data_ptr(), h.data_ptr(), W.data_ptr(), const.data_ptr(), dh.data_ptr(),
                                   dh_beta, dW.data_ptr(), dbias.data_ptr(), dconst.data_ptr(), beta, B, T, H, nh, ws.data_ptr(), ws.numel(),
                                   _stream()), "dyn_relpos_gate_bwd")
    return dh


def softmax_relbias(S, gate, E, table, D, out=None, valid=None):
    """softmax over the keys of S [B, nh, T, T] + gate[b, head, t] * E[table[s - t + Tmax - 1], head]; `valid` as in softmax()."""
    _cc(S, "softmax_relbias.S"); _cc(gate, "softmax_relbias.gate")
    B, T, H, Tmax, nbk = _relbias_dims("softmax_relbias", S, gate.shape[1] if gate.dim() == 3 else -1, D, E, table)
    if tuple(gate.shape) != (B, S.shape[1], T):
        raise DynError("softmax_relbias: gate does not match the scores")
    out = torch.empty_like(S) if out is None else _cc(out, "softmax_relbias.out")
    check(_L().dyn_softmax_relbias_fwd_len(S.data_ptr(), out.data_ptr(), gate.data_ptr(), E.data_ptr(), table.data_ptr(), B, T, H, S.shape[1],
                                           Tmax, nbk, _valid_ptr(valid, "softmax_relbias"), _stream()), "dyn_softmax_relbias_fwd_len")
    return out


def relbias_bwd(dS, gate, E, table, D, dE, beta=1.0):
    """From dS [B, nh, T, T] (gradient w.r.t. the pre-softmax sum): returns dgate [B, nh, T]; dE = beta * dE + the bias table's gradient."""
    _cc(dS, "relbias_bwd.dS"); _cc(gate, "relbias_bwd.gate"); _cc(dE, "relbias_bwd.dE")
    B, T, H, Tmax, nbk = _relbias_dims("relbias_bwd", dS, gate.shape[1] if gate.dim() == 3 else -1, D, E, table)
    if tuple(gate.shape) != (B, dS.shape[1], T) or dE.shape != E.shape:
        raise DynError("relbias_bwd: gate / dE do not match the scores / E")
    dgate = torch.empty_like(gate)
    ws = workspace(dS.device)
    check(_L().dyn_relbias_bwd(dS.data_ptr(), gate.data_ptr(), E.data_ptr(), table.data_ptr(), dgate.data_ptr(), dE.data_ptr(), beta, B, T, H,
                               dS.shape[1], Tmax, nbk, ws.data_ptr(), ws.numel(), _stream()), "dyn_relbias_bwd")
    return dgate


# ----------------------------------------------------------------------------------------------- Wav2Vec2-Conformer relative positions
def relative_position_table(T, H):
    """float32 CPU table [2 T - 1, H]: row k is the sinusoid of relative position T - 1 - k (positive ones first, reversed), what
    transformers' Wav2Vec2ConformerRelPositionalEmbedding returns for T frames.  Its own torch expressions, evaluated on the host: every
    entry depends on its position alone, so the slice transformers cuts out of a longer table (max_source_positions) holds the same floats."""
    import math
    pe_positive = torch.zeros(T, H)
    pe_negative = torch.zeros(T, H)
    position = torch.arange(0, T, dtype=torch.int64).float().unsqueeze(1)
    div_term = torch.exp(torch.arange(0, H, 2, dtype=torch.int64).float() * -(math.log(10000.0) / H))
    pe_positive[:, 0::2] = torch.sin(position * div_term)
    pe_positive[:, 1::2] = torch.cos(position * div_term)
    pe_negative[:, 0::2] = torch.sin(-1 * position * div_term)
    pe_negative[:, 1::2] = torch.cos(-1 * position * div_term)
    return torch.cat([torch.flip(pe_positive, [0]), pe_negative[1:]], dim=0).contiguous()


def rotary_tables(T, D, base):
    """(cos, sin) float32 CPU tables [T, D / 2] of transformers' Wav2Vec2ConformerRotaryPositionalEmbedding (the first half of its
    cat((freqs, freqs)) tables: ops.rotary's half-split convention), its own torch expressions on the host."""
    inv_freq = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    freqs = torch.einsum("i,j->ij", torch.arange(T).type_as(inv_freq), inv_freq)
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def _relshift_dims(who, S, ld_bd):
    if S.dim() != 4 or S.shape[2] != S.shape[3]:
        raise DynError(f"{who}: scores must be [B, heads, T, T], got {tuple(S.shape)}")
    T = S.shape[-1]
    ld = 2 * T - 1 if ld_bd is None else int(ld_bd)
    return S.shape[0] * S.shape[1], T, ld


def softmax_relshift(S, BD, out=None, valid=None, ld_bd=None, lens=None):
    """softmax over the keys of S [B, nh, T, T] + BD[b, h, i, T - 1 - i + j] (BD [B, nh, T, ld_bd >= 2T - 1], both scaled already: the
    Transformer-XL shift read in place); `valid` as in softmax(), or `lens` (int32 CUDA [B]): lens[b] keys in batch entry b.  `out` may be S."""
    valid, lens = _split_valid(valid, lens)
    _cc(S, "softmax_relshift.S"); _c(BD, "softmax_relshift.BD")
    M, T, ld = _relshift_dims("softmax_relshift", S, ld_bd)
    if BD.numel() != M * T * ld:
        raise DynError(f"softmax_relshift: BD holds {BD.numel()} floats, {M} x {T} x {ld} expected")
    out = torch.empty_like(S) if out is None else _cc(out, "softmax_relshift.out")
    if lens is not None:
        if S.dim() != 4:
            raise DynError("softmax_relshift: lens needs S as [B, nh, T, T]")
        check(_L().dyn_softmax_relshift_fwd_lens(S.data_ptr(), out.data_ptr(), BD.data_ptr(), S.shape[0], S.shape[1], T, ld,
                                                 _lens_ptr(lens, S.shape[0], "softmax_relshift", valid), _stream()), "dyn_softmax_relshift_fwd_lens")
        return out
    check(_L().dyn_softmax_relshift_fwd_len(S.data_ptr(), out.data_ptr(), BD.data_ptr(), M, T, ld, _valid_ptr(valid, "softmax_relshift"),
                                            _stream()), "dyn_softmax_relshift_fwd_len")
    return out


def relshift_bwd(dS, out=None, ld_bd=None):
    """dBD [B, nh, T, ld_bd] from dS [B, nh, T, T]: dS in every row's window, zeros written everywhere else (`out` may be stale scratch)."""
    _cc(dS, "relshift_bwd.dS")
    M, T, ld = _relshift_dims("relshift_bwd", dS, ld_bd)
    if out is None:
        out = torch.empty(*dS.shape[:3], ld, device=dS.device, dtype=F32)
    elif _c(out, "relshift_bwd.out").numel() != M * T * ld:
        raise DynError(f"relshift_bwd: out holds {out.numel()} floats, {M} x {T} x {ld} expected")
    check(_L().dyn_relshift_bwd(dS.data_ptr(), out.data_ptr(), M, T, ld, _stream()), "dyn_relshift_bwd")
    return out


def head_bias_add(q, u, v, H=None, ldq=None, q_off=0):
    """q [rows, H] inside a packed projection output (row stride `ldq` floats, first column `q_off`) + the per-head biases u, v [nh, D]
    -> (q + u, q + v), each [..., H] contiguous; q is read once."""
    _chk(q, "head_bias_add.q"); _cc(u, "head_bias_add.u"); _cc(v, "head_bias_add.v")
    H = u.numel() if H is None else H
    ldq = q.shape[-1] if ldq is None else ldq
    if not q.is_contiguous() or u.numel() != H or v.numel() != H or q.numel() % ldq or q_off + H > ldq:
        raise DynError("head_bias_add: operand shapes do not match")
    rows = q.numel() // ldq
    qu = torch.empty(*q.shape[:-1], H, device=q.device, dtype=F32)
    qv = torch.empty_like(qu)
    check(_L().dyn_head_bias_add(q.data_ptr() + 4 * q_off, ldq, u.data_ptr(), v.data_ptr(), qu.data_ptr(), qv.data_ptr(), rows, H, _stream()),
          "dyn_head_bias_add")
    return qu, qv


def head_bias_bwd(dqu, dqv, dq, du, dv, beta=1.0, ldq=None, q_off=0):
    """Backward of head_bias_add: dq (strided like q) = dqu + dqv; du = beta * du + column sums of dqu, dv likewise (fixed order)."""
    _cc(dqu, "head_bias_bwd.dqu"); _cc(dqv, "head_bias_bwd.dqv"); _c(dq, "head_bias_bwd.dq"); _cc(du, "head_bias_bwd.du"); _cc(dv, "head_bias_bwd.dv")
    H = du.numel()
    ldq = dq.shape[-1] if ldq is None else ldq
    rows = dqu.numel() // H
    if dqv.shape != dqu.shape or dv.numel() != H or dqu.numel() != rows * H or dq.numel() != rows * ldq or q_off + H > ldq:
        raise DynError("head_bias_bwd: operand shapes do not match")
    ws = workspace(dqu.device)
    check(_L().dyn_head_bias_bwd(dqu.data_ptr(), dqv.data_ptr(), dq.data_ptr() + 4 * q_off, ldq, du.data_ptr(), dv.data_ptr(), beta, rows, H,
                                 ws.data_ptr(), ws.numel(), _stream()), "dyn_head_bias_bwd")
    return dq


def log_softmax(x, out=None):
    _cc(x, "log_softmax.x")
    rows, L = _rows_L(x)
    out = torch.empty_like(x) if out is None else _cc(out, "log_softmax.out")
    check(_L().dyn_log_softmax_fwd(x.data_ptr(), out.data_ptr(), rows, L, L, L, _stream()), "dyn_log_softmax_fwd")
    return out


def log_softmax_bwd(y, dy, out=None):
    _cc(y, "log_softmax_bwd.y"); _cc(dy, "log_softmax_bwd.dy")
    rows, L = _rows_L(y)
    out = torch.empty_like(y) if out is None else _cc(out, "log_softmax_bwd.out")
    check(_L().dyn_log_softmax_bwd(y.data_ptr(), dy.data_ptr(), out.data_ptr(), rows, L, L, _stream()), "dyn_log_softmax_bwd")
    return out


def entropy_grad(log_probs, scale):
    """Gradient of `scale * sum_rows H(row)` w.r.t. log-probs [..., C]; returns (grad, per-row entropies)."""
    _cc(log_probs, "entropy_grad.log_probs")
    rows, L = _rows_L(log_probs)
    g = torch.empty_like(log_probs)
    ent = torch.empty(rows, device=log_probs.device, dtype=F32)
    check(_L().dyn_entropy_grad(log_probs.data_ptr(), g.data_ptr(), ent.data_ptr(), rows, L, L, scale, _stream()), "dyn_entropy_grad")
    return g, ent


def conv2d_first_dgrad(dz, w, T, F):
    """dz [B, To, Fo, C] -> dx [B, T, F] for the 1-channel 3x3/s2 first conv."""
    _cc(dz, "conv2d_first_dgrad.dz"); _cc(w, "conv2d_first_dgrad.w")
    B, C = dz.shape[0], dz.shape[-1]
    dx = torch.empty(B, T, F, device=dz.device, dtype=F32)
    check(_L().dyn_conv2d_first_dgrad(dz.data_ptr(), w.data_ptr(), dx.data_ptr(), B, T, F, C, _stream()), "dyn_conv2d_first_dgrad")
    return dx


# ----------------------------------------------------------------------------------------------- convolutions
def _odd_width(who, w):
    """The plain depthwise kernels pad (KW - 1) / 2 frames on both sides, and their data gradient is the flipped forward: both are right at
    an odd width only.  (The 32-tap conv module goes through convmod_bn / glu_dwconv1d_dgrad, which carry the two halos apart.)"""
    if w.shape[-1] % 2 == 0:
        raise DynError(f"{who}: an even kernel width ({w.shape[-1]}) is not built: SAME padding is asymmetric there")


def dwconv1d(x, w, bias, out=None):
    """x [B, T, C] channels-last, w [C, KW]."""
    _cc(x, "dwconv1d.x"); _cc(w, "dwconv1d.w")
    _odd_width("dwconv1d", w)
    B, T, C = x.shape
    out = torch.empty_like(x) if out is None else _cc(out, "dwconv1d.out")
    check(_L().dyn_dwconv1d_fwd(x.data_ptr(), w.data_ptr(), _opt(bias, "bias"), out.data_ptr(), B, T, C, w.shape[1], _stream()),
          "dyn_dwconv1d_fwd")
    return out


def dwconv1d_dgrad(dy, w, out=None, beta=0.0):
    _cc(dy, "dwconv1d_dgrad.dy")
    _odd_width("dwconv1d_dgrad", w)
    B, T, C = dy.shape
    out = torch.empty_like(dy) if out is None else _cc(out, "dwconv1d_dgrad.out")
    if _is_group(w):
        _group_dims(dy, w.R, "dwconv1d_dgrad")
        check(_L().dyn_dwconv1d_dgrad_g(dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, T, C, w.shape[1], beta, w.R, w.stride, _stream()),
              "dyn_dwconv1d_dgrad_g")
        return out
    _cc(w, "dwconv1d_dgrad.w")
    check(_L().dyn_dwconv1d_dgrad(dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, T, C, w.shape[1], beta, _stream()),
          "dyn_dwconv1d_dgrad")
    return out


def dwconv1d_wgrad(x, dy, dw, dbias, beta=1.0):
    _cc(x, "dwconv1d_wgrad.x"); _cc(dy, "dwconv1d_wgrad.dy")
    B, T, C = x.shape
    ws = workspace(x.device)
    if _is_group(dw):
        _group_dims(x, dw.R, "dwconv1d_wgrad")
        check(_L().dyn_dwconv1d_wgrad_g(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0 if dbias is None else dbias.data_ptr(), beta, B, T, C,
                                        dw.shape[1], dw.R, dw.stride, ws.data_ptr(), ws.numel(), _stream()), "dyn_dwconv1d_wgrad_g")
        return
    _cc(dw, "dwconv1d_wgrad.dw")
    check(_L().dyn_dwconv1d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _opt(dbias, "dbias"), beta, B, T, C,
                                  dw.shape[1], ws.data_ptr(), ws.numel(), _stream()), "dyn_dwconv1d_wgrad")


def convmod_fwd(u, w, bias, gamma, beta, layernorm, eps, save):
    """Fused GLU -> dwconv(k=9) -> norm -> SiLU.  u [B, T, 2C] -> s [B, T, C]; with `save` also (g, c, nn, mean, rstd).
    Lockstep group (w a GroupParam): one launch per sample into shared output tensors (sample s: replica s % R's weights)."""
    _cc(u, "convmod.u")
    B, T, C2 = u.shape
    C = C2 // 2
    dev = u.device
    s = torch.empty(B, T, C, device=dev, dtype=F32)
    g = c = nn = mean = rstd = None
    if save:
        g, c, nn = (torch.empty(B, T, C, device=dev, dtype=F32) for _ in range(3))
        rstd = torch.empty(B * T, device=dev, dtype=F32)
        mean = torch.empty(B * T, device=dev, dtype=F32) if layernorm else None
    if _is_group(w):        # lockstep group: one launch, sample k takes replica k % R's filters and norm weights
        _group_dims(u, w.R, "convmod")
        check(_L().dyn_convmod_fwd_g(u.data_ptr(), w.data_ptr(), 0 if bias is None else bias.data_ptr(), gamma.data_ptr(),
                                     0 if beta is None else beta.data_ptr(), s.data_ptr(), _opt(g, "g"), _opt(c, "c"), _opt(nn, "nn"),
                                     _opt(mean, "mean"), _opt(rstd, "rstd"), B, T, C, w.shape[1], int(layernorm), eps, w.R, w.stride, _stream()),
              "dyn_convmod_fwd_g")
        return s, g, c, nn, mean, rstd
    _cc(w, "convmod.w")
    check(_L().dyn_convmod_fwd(u.data_ptr(), w.data_ptr(), _opt(bias, "bias"), gamma.data_ptr(), _opt(beta, "beta"), s.data_ptr(),
                               _opt(g, "g"), _opt(c, "c"), _opt(nn, "nn"), _opt(mean, "mean"), _opt(rstd, "rstd"), B, T, C, w.shape[1],
                               int(layernorm), eps, _stream()), "dyn_convmod_fwd")
    return s, g, c, nn, mean, rstd


def out_len(n):
    """Output length of a 3-wide, stride-2, pad-1 convolution."""
    return (n - 1) // 2 + 1


def conv2d_first(x, w, bias, out=None, lens=None):
    """x [B, T, F] -> z [B, To, Fo, C]; w [C, 3, 3].  `lens` (int32 CUDA [B]): frames t >= lens[b] of x read as zeros."""
    _cc(x, "conv2d_first.x"); _cc(w, "conv2d_first.w"); _cc(bias, "conv2d_first.bias")
    B, T, F = x.shape
    C = w.shape[0]
    if out is None:
        out = torch.empty(B, out_len(T), out_len(F), C, device=x.device, dtype=F32)
    if lens is not None:
        check(_L().dyn_conv2d_first_fwd_lens(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C,
                                             _lens_ptr(lens, B, "conv2d_first"), _stream()), "dyn_conv2d_first_fwd_lens")
        return out
    check(_L().dyn_conv2d_first_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, _stream()),
          "dyn_conv2d_first_fwd")
    return out


def conv2d_first_wgrad(x, dz, dw, dbias, beta=1.0, lens=None):
    """dw [C, 3, 3], dbias [C] = beta * old + the gradients of conv2d_first.  `lens` (int32 CUDA [B]): frames t >= lens[b] of x read as zeros."""
    _cc(x, "conv2d_first_wgrad.x"); _cc(dz, "conv2d_first_wgrad.dz")
    B, T, F = x.shape
    C = dw.shape[0]
    ws = workspace(x.device)
    if lens is not None:
        check(_L().dyn_conv2d_first_wgrad_lens(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C,
                                               _lens_ptr(lens, B, "conv2d_first_wgrad"), ws.data_ptr(), ws.numel(), _stream()),
              "dyn_conv2d_first_wgrad_lens")
        return
    check(_L().dyn_conv2d_first_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C,
                                      ws.data_ptr(), ws.numel(), _stream()), "dyn_conv2d_first_wgrad")


def dwconv2d_s2(z, w, bias, out=None):
    """u = bias + dw3x3_s2(silu(z)); z [B, T, F, C] -> [B, To, Fo, C]; w [C, 3, 3]."""
    _cc(z, "dwconv2d_s2.z"); _cc(w, "dwconv2d_s2.w"); _cc(bias, "dwconv2d_s2.bias")
    B, T, F, C = z.shape
    if out is None:
        out = torch.empty(B, out_len(T), out_len(F), C, device=z.device, dtype=F32)
    check(_L().dyn_dwconv2d_s2_fwd(z.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, _stream()),
          "dyn_dwconv2d_s2_fwd")
    return out


def dwconv2d_s2_dgrad(z, w, du, out=None):
    _cc(z, "dwconv2d_s2_dgrad.z"); _cc(du, "dwconv2d_s2_dgrad.du")
    B, T, F, C = z.shape
    out = torch.empty_like(z) if out is None else _cc(out, "dwconv2d_s2_dgrad.out")
    check(_L().dyn_dwconv2d_s2_dgrad(z.data_ptr(), w.data_ptr(), du.data_ptr(), out.data_ptr(), B, T, F, C, _stream()),
          "dyn_dwconv2d_s2_dgrad")
    return out


def dwconv2d_s2_wgrad(z, du, dw, dbias, beta=1.0):
    _cc(z, "dwconv2d_s2_wgrad.z"); _cc(du, "dwconv2d_s2_wgrad.du")
    B, T, F, C = z.shape
    ws = workspace(z.device)
    check(_L().dyn_dwconv2d_s2_wgrad(z.data_ptr(), du.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C,
                                     ws.data_ptr(), ws.numel(), _stream()), "dyn_dwconv2d_s2_wgrad")


def sub12_fwd(x, w1, b1, w2, b2, out=None):
    """Fused first two subsampling stages: x [B, T, F] -> u2 [B, T2, F2, C] = b2 + dw3x3_s2(silu(b1 + conv3x3_s2(x))); the
    [B, T1, F1, C] intermediate never reaches HBM (dyn_sub12_fwd)."""
    _cc(x, "sub12.x"); _cc(w1, "sub12.w1"); _cc(b1, "sub12.b1"); _cc(w2, "sub12.w2"); _cc(b2, "sub12.b2")
    B, T, F = x.shape
    C = w1.shape[0]
    if out is None:
        out = torch.empty(B, out_len(out_len(T)), out_len(out_len(F)), C, device=x.device, dtype=F32)
    check(_L().dyn_sub12_fwd(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), B, T, F, C, _stream()),
          "dyn_sub12_fwd")
    return out


def sub12_bwd(x, du2, w1, b1, w2, dw1, db1, dw2, db2, beta=1.0):
    """Weight / bias gradients of both fused stages from du2 [B, T2, F2, C] (z1 recomputed from x, dz1 never stored)."""
    _cc(x, "sub12_bwd.x"); _cc(du2, "sub12_bwd.du2")
    B, T, F = x.shape
    C = w1.shape[0]
    ws = workspace(x.device)
    check(_L().dyn_sub12_bwd(x.data_ptr(), du2.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), dw1.data_ptr(), db1.data_ptr(),
                             dw2.data_ptr(), db2.data_ptr(), beta, B, T, F, C, ws.data_ptr(), ws.numel(), _stream()), "dyn_sub12_bwd")


def rotary(x, cos, sin, B, T, n_heads, D, row_stride, inverse=False):
    """In place on the first n_heads*D floats of every row_stride-float row of x."""
    _cc(x, "rotary.x"); _cc(cos, "rotary.cos"); _cc(sin, "rotary.sin")
    assert cos.shape[0] >= T and cos.shape[1] == D // 2
    check(_L().dyn_rotary(x.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, T, n_heads, D, row_stride, int(inverse), _stream()),
          "dyn_rotary")
    return x


# ----------------------------------------------------------------------------------------------- CTC
def ctc_greedy(log_probs, blank):
    """log_probs [B, T, C] (or [T, C]) on device -> (ids int32 [B, T] device, lengths int32 [B] device).
    Only out_len[b] leading ids of each row are valid."""
    _c(log_probs, "ctc_greedy.log_probs")
    lp = log_probs if log_probs.dim() == 3 else log_probs.unsqueeze(0)
    B, T, C = lp.shape
    arg = torch.empty(B, T, device=lp.device, dtype=I32)
    ids = torch.empty(B, T, device=lp.device, dtype=I32)
    n = torch.empty(B, device=lp.device, dtype=I32)
    check(_L().dyn_ctc_greedy(lp.data_ptr(), B, T, C, C, blank, arg.data_ptr(), ids.data_ptr(), n.data_ptr(), _stream()),
          "dyn_ctc_greedy")
    return ids, n


def argmax_rows(x):
    """x [rows, C] -> (ids int32 [rows], max values [rows]); first maximum wins."""
    _c(x, "argmax_rows.x")
    rows, C = x.shape
    ids = torch.empty(rows, device=x.device, dtype=I32)
    vals = torch.empty(rows, device=x.device, dtype=F32)
    check(_L().dyn_argmax_rows(x.data_ptr(), rows, C, C, ids.data_ptr(), vals.data_ptr(), _stream()), "dyn_argmax_rows")
    return ids, vals


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank, reduction="sum", grad_scale=1.0, want_grad=True):
    """log_probs [B, T, C] contiguous; targets int32 [B, S_max]; lengths int32 [B] (all on device).
    Returns (loss [1] device tensor, nll [B], grad [B, T, C] or None) with torch.nn.CTCLoss semantics."""
    _c(log_probs, "ctc_loss.log_probs"); _c(targets, "ctc_loss.targets", I32)
    _cc(input_lengths, "ctc_loss.input_lengths", I32); _cc(target_lengths, "ctc_loss.target_lengths", I32)
    B, T, C = log_probs.shape
    S_max = targets.shape[1] if targets.numel() else 0
    loss = torch.empty(1, device=log_probs.device, dtype=F32)
    nll = torch.empty(B, device=log_probs.device, dtype=F32)
    grad = torch.empty_like(log_probs) if want_grad else None
    ws = workspace(log_probs.device)
    need = _L().dyn_ctc_loss_workspace_bytes(T, B, S_max)
    if need > ws.numel():
        raise DynError(f"ctc_loss: workspace {ws.numel()} < {need} bytes")
    tptr = targets.data_ptr() if targets.numel() else nll.data_ptr()
    check(_L().dyn_ctc_loss(log_probs.data_ptr(), T, B, C, C, T * C, tptr, S_max, input_lengths.data_ptr(),
                            target_lengths.data_ptr(), blank, {"sum": 0, "mean": 1}[reduction], grad_scale, loss.data_ptr(),
                            nll.data_ptr(), 0 if grad is None else grad.data_ptr(), C, T * C, ws.data_ptr(), ws.numel(),
                            _stream()), "dyn_ctc_loss")
    return loss, nll, grad


def ctc_lattice(T, B, S_max, device):
    """Views of the lattice the last ops.ctc_loss call of this (device, stream) left in the workspace:
    (alpha [B, T, L], beta [B, T, L], nll [B]) with L = 2 * max(S_max, 1) + 1; beta is only written when a gradient was asked for."""
    import ctypes
    off = (ctypes.c_int64 * 4)()
    L = ctypes.c_int64()
    check(_L().dyn_ctc_loss_workspace_layout(T, B, S_max, ctypes.cast(off, ctypes.c_void_p), ctypes.cast(ctypes.byref(L), ctypes.c_void_p)),
          "dyn_ctc_loss_workspace_layout")
    ws = workspace(device)
    n = B * T * L.value * 4
    alpha = ws[off[1]:off[1] + n].view(F32).view(B, T, L.value)
    beta = ws[off[2]:off[2] + n].view(F32).view(B, T, L.value)
    nll = ws[off[3]:off[3] + 4 * B].view(F32)
    return alpha, beta, nll


def libm_f32(x):
    """(expf(x), logf(x), the lattice's branch-free expf for x <= 0) from the device build of csrc/libm_f32.h."""
    _cc(x, "libm_f32.x")
    e, l, n = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    check(_L().dyn_libm_f32(x.data_ptr(), x.numel(), e.data_ptr(), l.data_ptr(), n.data_ptr(), _stream()), "dyn_libm_f32")
    return e, l, n


# ----------------------------------------------------------------------------------------------- optimiser / stitch
def madgrad_step(p, g, s, nu, x0, lr, momentum, weight_decay, eps, step):
    for t, n in ((p, "p"), (g, "g"), (s, "s"), (nu, "nu"), (x0, "x0")):
        _cc(t, "madgrad." + n)
    check(_L().dyn_madgrad_step(p.data_ptr(), g.data_ptr(), s.data_ptr(), nu.data_ptr(), x0.data_ptr(), p.numel(), lr, momentum,
                                weight_decay, eps, step, _stream()), "dyn_madgrad_step")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _cc(t, "adam." + n)
    check(_L().dyn_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                             weight_decay, step, _stream()), "dyn_adam_step")


def clip_grad_norm(g, max_norm):
    """In-place global-norm clip of a flat gradient buffer; returns a 2-float device tensor (norm, coefficient)."""
    _cc(g, "clip_grad_norm.g")
    out = torch.empty(2, device=g.device, dtype=F32)
    ws = workspace(g.device)
    check(_L().dyn_clip_grad_norm(g.data_ptr(), g.numel(), max_norm, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "dyn_clip_grad_norm")
    return out


# ---- the consistency loop (csrc/consistency.hip)
MIX_DECAY_PER_DISTANCE = 0.95       # reference lcasr/lib.py:818


def grad_mix_tables(n_windows, decay_per_distance=MIX_DECAY_PER_DISTANCE):
    """(decay[k] = decay_per_distance ** k, total_sum[i]) as Python doubles, formed exactly as the reference forms them
    (lcasr/lib.py:828-834: `total_sum = 1`, then `+= decay ** abs(i - q)` over q != i in ascending q)."""
    decay = [decay_per_distance ** k for k in range(n_windows)]
    denom = []
    for i in range(n_windows):
        total = 1
        for q in range(n_windows):
            if q != i:
                total += decay[abs(i - q)]
        denom.append(float(total))
    return decay, denom


def merge_ranges(ranges):
    """Sorted [lo, hi) ranges with touching ones joined."""
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in ranges if b > a):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(r) for r in out]


def grad_mix_max_windows():
    return int(_L().dyn_grad_mix_decay_max_windows())


def grad_mix_decay(bank, ranges=None, decay_per_distance=MIX_DECAY_PER_DISTANCE):
    """In-place distance-decayed mix of the gradient bank `bank` [W, P] (rows = windows in key order), reference lcasr/lib.py:817-841,
    bit for bit.  `ranges`: [lo, hi) element ranges that carry a gradient (default: the whole row); the rest is not touched."""
    _chk(bank, "grad_mix.bank")
    if bank.dim() != 2 or bank.stride(1) != 1:
        raise DynError("grad_mix.bank: expected [W, P] with contiguous rows")
    W, P = bank.shape
    if W > grad_mix_max_windows():
        raise DynError(f"grad_mix_decay: {W} windows, the kernel stages at most {grad_mix_max_windows()} per element in LDS")
    ranges = merge_ranges([(0, P)] if ranges is None else ranges)
    if any(lo < 0 or hi > P for lo, hi in ranges):
        raise DynError(f"grad_mix_decay: range outside a row of {P} elements")
    if not ranges:
        return bank
    decay, denom = grad_mix_tables(W, decay_per_distance)
    tables = torch.tensor([decay, denom], dtype=torch.float64).to(bank.device)
    host = (ctypes.c_int64 * (2 * len(ranges)))(*[v for r in ranges for v in r])
    check(_L().dyn_grad_mix_decay(bank.data_ptr(), bank.stride(0), W, ctypes.cast(host, ctypes.c_void_p), len(ranges),
                                  tables[0].data_ptr(), tables[1].data_ptr(), _stream()), "dyn_grad_mix_decay")
    return bank


ADAFACTOR_SEG_COLS = 9


def adafactor_segments(shapes, offsets):
    """Segment table of dyn_adafactor_step for tensors of `shapes` at `offsets` of a flat buffer (include/dyneval.h): ->
    (rows [n, 9] as a list, totals dict(n_rows, n_batches, n_cols, n_state)).  A tensor of dimension >= 2 is factored over its last two
    dimensions with the leading ones as batch, as torch.optim.Adafactor does; 0-d and 1-D tensors keep a full second moment."""
    import math
    rows_tab, row0, batch0, col0, state0, extent = [], 0, 0, 0, 0, 0
    for shape, off in zip(shapes, offsets):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        if n == 0:
            continue
        if len(shape) >= 2:
            batch, rows, cols, factored = math.prod(shape[:-2]), shape[-2], shape[-1], 1
        else:
            batch, rows, cols, factored = 1, 1, n, 0
        rows_tab.append([int(off), batch, rows, cols, state0, factored, row0, batch0, col0])
        row0 += batch * rows
        batch0 += batch
        col0 += batch * cols if factored else 0
        state0 += batch * (rows + cols) if factored else n
        extent = max(extent, int(off) + n)
    return rows_tab, dict(n_rows=row0, n_batches=batch0, n_cols=col0, n_state=state0, extent=extent)


def adafactor_scratch_bytes(totals, n_segments):
    return int(_L().dyn_adafactor_scratch_bytes(totals["n_rows"], totals["n_batches"], n_segments))


def adafactor_step(p, g, state, seg_dev, totals, scratch, lr, beta2_decay, eps1, eps2, d, weight_decay, step):
    """One torch.optim.Adafactor step (`step` counts from 1) of the flat buffers p / g with `state` (zeros when fresh) and the device
    segment table `seg_dev` [n, 9] int64 of adafactor_segments()."""
    _cc(p, "adafactor.p"); _cc(g, "adafactor.g"); _cc(state, "adafactor.state")
    _cc(seg_dev, "adafactor.segments", torch.int64)
    if state.numel() < totals["n_state"] or p.numel() < totals["extent"] or g.numel() < totals["extent"]:
        raise DynError("adafactor: the segment table reaches beyond the parameter, gradient or state buffer")
    if eps1 is None:
        eps1 = torch.finfo(torch.float32).eps
    check(_L().dyn_adafactor_step(p.data_ptr(), g.data_ptr(), state.data_ptr(), seg_dev.data_ptr(), seg_dev.shape[0], totals["n_rows"],
                                  totals["n_batches"], totals["n_cols"], lr, beta2_decay, eps1, eps2, d, weight_decay, step,
                                  scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream()), "dyn_adafactor_step")


def stitch_accumulate(log_probs, acc, count, pos):
    _c(log_probs, "stitch.log_probs"); _cc(acc, "stitch.acc"); _cc(count, "stitch.count")
    rows, C = log_probs.shape
    check(_L().dyn_stitch_accumulate(log_probs.data_ptr(), C, acc.data_ptr(), count.data_ptr(), pos, rows, C, acc.shape[0],
                                     _stream()), "dyn_stitch_accumulate")


def stitch_finalize(acc, count, rows):
    _cc(acc, "stitch.acc"); _cc(count, "stitch.count")
    C = acc.shape[1]
    out = torch.empty(rows, C, device=acc.device, dtype=F32)
    check(_L().dyn_stitch_finalize(acc.data_ptr(), count.data_ptr(), out.data_ptr(), rows, C, _stream()), "dyn_stitch_finalize")
    return out


def stitch_finalize_rows(acc, count, row_index):
    """log(acc / count) over the listed rows (int64 CUDA tensor): coverage with gaps."""
    _cc(acc, "stitch.acc"); _cc(count, "stitch.count"); _c(row_index, "stitch.row_index", torch.int64)
    C = acc.shape[1]
    out = torch.empty(row_index.numel(), C, device=acc.device, dtype=F32)
    check(_L().dyn_stitch_finalize_rows(acc.data_ptr(), count.data_ptr(), row_index.data_ptr(), out.data_ptr(), row_index.numel(), C,
                                        _stream()), "dyn_stitch_finalize_rows")
    return out


# ----------------------------------------------------------------------------------------------- wav2vec2 pieces
def gelu(x, out=None):
    _c(x, "gelu.x")
    out = torch.empty_like(x) if out is None else out
    check(_L().dyn_gelu_fwd(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_gelu_fwd")
    return out


def gelu_bwd(x, dy, out=None):
    _c(x, "gelu_bwd.x"); _c(dy, "gelu_bwd.dy")
    out = torch.empty_like(x) if out is None else out
    check(_L().dyn_gelu_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_gelu_bwd")
    return out


def bias_layernorm_gelu(z, conv_bias, gamma, beta, eps=1e-5):
    """act = gelu(LayerNorm_C(z + conv_bias)) in one pass (layer-norm feature extractor).  z [..., C] is left unmodified; conv_bias may be
    None.  Returns (act, mean [rows], rstd [rows])."""
    _cc(z, "bias_layernorm_gelu.z"); _cc(gamma, "bias_layernorm_gelu.gamma"); _cc(beta, "bias_layernorm_gelu.beta")
    C = z.shape[-1]
    rows = z.numel() // C
    act = torch.empty_like(z)
    mean = torch.empty(rows, device=z.device, dtype=F32)
    rstd = torch.empty(rows, device=z.device, dtype=F32)
    check(_L().dyn_bias_layernorm_gelu_fwd(z.data_ptr(), _opt(conv_bias, "bias_layernorm_gelu.conv_bias"), gamma.data_ptr(), beta.data_ptr(),
                                           act.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, eps, _stream()),
          "dyn_bias_layernorm_gelu_fwd")
    return act, mean, rstd


def bias_layernorm_gelu_bwd(z, conv_bias, gamma, beta, mean, rstd, dact, dgamma, dbeta, dconv_bias, wgrad_beta=1.0, out=None):
    """Backward of bias_layernorm_gelu from z, mean, rstd (the normalised tensor is recomputed): returns dz (`out`, which may be dact);
    dgamma / dbeta / dconv_bias = wgrad_beta * old + column sums, each may be None (frozen)."""
    _cc(z, "bias_layernorm_gelu_bwd.z"); _cc(dact, "bias_layernorm_gelu_bwd.dact")
    _cc(gamma, "bias_layernorm_gelu_bwd.gamma"); _cc(beta, "bias_layernorm_gelu_bwd.beta")
    _cc(mean, "bias_layernorm_gelu_bwd.mean"); _cc(rstd, "bias_layernorm_gelu_bwd.rstd")
    C = z.shape[-1]
    rows = z.numel() // C
    if dact.numel() != z.numel() or mean.numel() != rows or rstd.numel() != rows:
        raise DynError("bias_layernorm_gelu_bwd: dact / mean / rstd do not match z")
    dz = torch.empty_like(z) if out is None else _cc(out, "bias_layernorm_gelu_bwd.out")
    if dz.numel() != z.numel():
        raise DynError("bias_layernorm_gelu_bwd: out does not match z")
    ws = workspace(z.device)
    check(_L().dyn_bias_layernorm_gelu_bwd(z.data_ptr(), _opt(conv_bias, "bias_layernorm_gelu_bwd.conv_bias"), gamma.data_ptr(), beta.data_ptr(),
                                           mean.data_ptr(), rstd.data_ptr(), dact.data_ptr(), dz.data_ptr(), _opt(dgamma, "dgamma"),
                                           _opt(dbeta, "dbeta"), _opt(dconv_bias, "dconv_bias"), wgrad_beta, rows, C, ws.data_ptr(),
                                           ws.numel(), _stream()), "dyn_bias_layernorm_gelu_bwd")
    return dz


def _valid_ptr(valid, what):
    """`valid`: None, or a one-element int32 CUDA tensor holding a row / column count that the kernel reads when it RUNS (so a captured launch
    follows later updates of the tensor)."""
    if valid is None:
        return None
    if not (isinstance(valid, torch.Tensor) and valid.is_cuda and valid.dtype == torch.int32 and valid.numel() == 1):
        raise DynError(f"{what}: the valid-length operand must be a one-element int32 CUDA tensor")
    return valid.data_ptr()


class RowLens:
    """The `valid` argument of a ragged batch: frame counts per batch entry (`lens`, int32 CUDA [B]) where a length bucket has one device
    scalar.  The layer code hands `valid` through unchanged; the wrappers that take `valid` route a RowLens to their `_lens` entry."""

    def __init__(self, lens):
        self.lens = lens

    def cut(self, nb):
        return RowLens(self.lens[:nb])


def _split_valid(valid, lens):
    return (None, valid.lens) if isinstance(valid, RowLens) and lens is None else (valid, lens)


def _lens_ptr(lens, B, what, valid=None):
    """`lens`: the frame counts of a ragged batch, one per batch entry: an int32 CUDA tensor [B] the kernel reads (and clamps) when it runs.
    It takes the place of the scalar `valid`; both together are refused."""
    if valid is not None:
        raise DynError(f"{what}: pass `valid` (one count for the batch) or `lens` (one per batch entry), not both")
    if not (isinstance(lens, torch.Tensor) and lens.is_cuda and lens.dtype == torch.int32 and lens.dim() == 1 and lens.is_contiguous()):
        raise DynError(f"{what}: lens must be a contiguous int32 CUDA tensor [B]")
    if lens.numel() != B:
        raise DynError(f"{what}: lens holds {lens.numel()} counts for a batch of {B}")
    return lens.data_ptr()


def mask_rows_lens(x, lens):
    """x [B, T, ...] in place: rows t >= lens[b] (int32 CUDA [B]) of batch entry b := 0."""
    _cc(x, "mask_rows_lens.x")
    if x.dim() < 3:
        raise DynError("mask_rows_lens: x must be [B, T, ...]")
    B, T = x.shape[:2]
    check(_L().dyn_mask_rows_lens(x.data_ptr(), B, T, x.numel() // max(B * T, 1), _lens_ptr(lens, B, "mask_rows_lens"), _stream()),
          "dyn_mask_rows_lens")
    return x


def colnorm(x, gamma, beta, eps=1e-5, valid=None):
    """x [B, T, C]: normalise over T per (b, c) (GroupNorm with groups == channels). Returns (y, mean, rstd).  `valid` (device int32 scalar):
    the statistics cover the first `valid` rows only (zero-padded bucket)."""
    _c(x, "colnorm.x")
    B, T, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B, C, device=x.device, dtype=F32); rstd = torch.empty(B, C, device=x.device, dtype=F32)
    ws = workspace(x.device)
    check(_L().dyn_colnorm_fwd_len(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, T, C,
                                   eps, _valid_ptr(valid, "colnorm"), ws.data_ptr(), ws.numel(), _stream()), "dyn_colnorm_fwd")
    return y, mean, rstd


def colnorm_bwd(x, gamma, mean, rstd, dy, dgamma, dbeta, wgrad_beta=1.0, valid=None):
    B, T, C = x.shape
    dx = torch.empty_like(x)
    ws = workspace(x.device)
    check(_L().dyn_colnorm_bwd_len(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                   _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), wgrad_beta, B, T, C, _valid_ptr(valid, "colnorm_bwd"),
                                   ws.data_ptr(), ws.numel(), _stream()), "dyn_colnorm_bwd")
    return dx


def mask_rows(x, valid):
    """x [B, T, C] in place: rows t >= valid (device int32 scalar) of every batch entry := 0."""
    _cc(x, "mask_rows.x")
    B, T, C = x.shape
    check(_L().dyn_mask_rows(x.data_ptr(), B, T, C, _valid_ptr(valid, "mask_rows"), _stream()), "dyn_mask_rows")
    return x


def conv1d_out_len(T, kw, stride):
    return (T - kw) // stride + 1


def conv1d(x, w, kw, stride):
    """Valid strided Conv1d as an implicit GEMM: x [B, T, Cin] channels-last, w [Cout, kw*Cin] -> [B, Tout, Cout]."""
    _c(x, "conv1d.x"); _c(w, "conv1d.w")
    B, T, Cin = x.shape
    Cout = w.shape[0]
    Tout = conv1d_out_len(T, kw, stride)
    y = torch.empty(B, Tout, Cout, device=x.device, dtype=F32)
    gemm(x, w, y, trans_b=True, M=Tout, N=Cout, K=kw * Cin, lda=stride * Cin, ldb=kw * Cin, ldc=Cout, nb1=B,
         sa=(T * Cin, 0), sc=(Tout * Cout, 0))
    return y


def conv1d_wgrad(x, dy, dw, kw, stride, beta=1.0):
    """dw [Cout, kw*Cin] = beta*dw + sum_b dy[b]^T @ rows(x[b])  (rows overlap: ldb = stride*Cin < kw*Cin)."""
    B, T, Cin = x.shape
    Tout, Cout = dy.shape[1], dy.shape[2]
    for b in range(B):
        gemm(dy, x, dw, trans_a=True, M=Cout, N=kw * Cin, K=Tout, lda=Cout, ldb=stride * Cin, ldc=kw * Cin,
             a_off=b * Tout * Cout, b_off=b * T * Cin, beta=beta if b == 0 else 1.0)
    return dw


def conv1d_dgrad(dy, w, T, Cin, kw, stride):
    """dx [B, T, Cin] from dy [B, Tout, Cout]: dense row gradients (GEMM) then col2im over the overlapping rows."""
    B, Tout, Cout = dy.shape
    dA = torch.empty(B, Tout, kw * Cin, device=dy.device, dtype=F32)
    gemm(dy, w, dA, M=B * Tout, N=kw * Cin, K=Cout, lda=Cout, ldb=kw * Cin, ldc=kw * Cin)
    return col2im_1d(dA, torch.empty(B, T, Cin, device=dy.device, dtype=F32), B, T, Tout, Cin, kw, stride)


def col2im_1d(dA, dx, B, T, Tout, C, kw, stride):
    """dx [B, T, C] = the dense row gradients dA [B, Tout, kw * C] added over the rows' overlaps (row t covers frames t * stride .. + kw)."""
    check(_L().dyn_col2im_1d(dA.data_ptr(), dx.data_ptr(), B, T, Tout, C, kw, stride, _stream()), "dyn_col2im_1d")
    return dx


def weight_norm(v, g):
    """v [rows, kw, cg], g [kw] -> w = g[tap] * v / ||v[:, tap, :]||."""
    rows, kw, cg = v.shape
    w = torch.empty_like(v)
    ws = workspace(v.device)
    check(_L().dyn_weight_norm_fwd(v.data_ptr(), g.data_ptr(), w.data_ptr(), rows, kw, cg, ws.data_ptr(), ws.numel(), _stream()),
          "dyn_weight_norm_fwd")
    return w


def weight_norm_bwd(v, g, dw, dv, dg, beta=1.0):
    rows, kw, cg = v.shape
    ws = workspace(v.device)
    check(_L().dyn_weight_norm_bwd(v.data_ptr(), g.data_ptr(), dw.data_ptr(), dv.data_ptr(), dg.data_ptr(), beta, rows, kw, cg,
                                   ws.data_ptr(), ws.numel(), _stream()), "dyn_weight_norm_bwd")


def group_pack(x, G, pad):
    B, T, C = x.shape
    xg = torch.empty(B, G, T + 2 * pad, C // G, device=x.device, dtype=F32)
    check(_L().dyn_group_pack(x.data_ptr(), xg.data_ptr(), B, T, C, G, pad, _stream()), "dyn_group_pack")
    return xg


def group_unpack(yg, bias, T, C):
    B, G, Tg, cg = yg.shape
    y = torch.empty(B, T, C, device=yg.device, dtype=F32)
    check(_L().dyn_group_unpack(yg.data_ptr(), y.data_ptr(), _opt(bias, "bias"), B, T, Tg, C, G, _stream()), "dyn_group_unpack")
    return y


def group_pack_grad(dy, G, Tg):
    B, T, C = dy.shape
    dyg = torch.empty(B, G, Tg, C // G, device=dy.device, dtype=F32)
    check(_L().dyn_group_pack_grad(dy.data_ptr(), dyg.data_ptr(), B, T, Tg, C, G, _stream()), "dyn_group_pack_grad")
    return dyg


def group_unpack_grad(dxg, dx, pad, beta=0.0):
    B, T, C = dx.shape
    G = dxg.shape[1]
    check(_L().dyn_group_unpack_grad(dxg.data_ptr(), dx.data_ptr(), B, T, C, G, pad, beta, _stream()), "dyn_group_unpack_grad")
    return dx


def _posconv_dims(who, yg, bias, T):
    if yg.dim() != 4:
        raise DynError(f"{who}: yg must be [B, G, Tg, cg]")
    B, G, Tg, cg = yg.shape
    H = G * cg
    if H % 256 or H > 1024:
        raise DynError(f"{who}: H = G * cg = {H} must be a multiple of 256 up to 1024")
    if cg % 4:
        raise DynError(f"{who}: cg = {cg} channels per group must be a multiple of 4")
    if not 0 <= T <= Tg:
        raise DynError(f"{who}: T = {T} rows of the {Tg} yg holds per group")
    if bias is None or bias.numel() != H:
        raise DynError(f"{who}: the conv bias must have H = {H} elements")
    return B, G, Tg, cg, H


def posconv_ln_gelu(yg, bias, T, pad=0, eps=1e-5, valid=None, want_act=True, want_packed=False):
    """One Data2Vec-Audio positional conv layer after its grouped GEMM: gelu(LayerNorm_H(rows of yg + bias)), no affine parameters.  yg
    [B, G, Tg >= T, cg] is left unmodified.  Returns (act [B, T, H] or None, xg_next [B, G, T + 2 pad, cg] or None, mean [B T], rstd [B T]):
    xg_next is the next layer's packed and zero-padded input; rows t >= `valid` (device int32 scalar) are zeros in both."""
    _cc(yg, "posconv_ln_gelu.yg"); _cc(bias, "posconv_ln_gelu.bias")
    B, G, Tg, cg, H = _posconv_dims("posconv_ln_gelu", yg, bias, T)
    if not (want_act or want_packed):
        raise DynError("posconv_ln_gelu: at least one of the two outputs must be wanted")
    act = torch.empty(B, T, H, device=yg.device, dtype=F32) if want_act else None
    xg = torch.empty(B, G, T + 2 * pad, cg, device=yg.device, dtype=F32) if want_packed else None
    mean = torch.empty(B * T, device=yg.device, dtype=F32)
    rstd = torch.empty(B * T, device=yg.device, dtype=F32)
    check(_L().dyn_posconv_ln_gelu_fwd(yg.data_ptr(), bias.data_ptr(), _opt(act, "act"), _opt(xg, "xg_next"), mean.data_ptr(), rstd.data_ptr(),
                                       B, T, Tg, H, G, pad, eps, _valid_ptr(valid, "posconv_ln_gelu"), _stream()), "dyn_posconv_ln_gelu_fwd")
    return act, xg, mean, rstd


def posconv_ln_gelu_bwd(yg, bias, mean, rstd, dact, dbias, wgrad_beta=1.0, valid=None):
    """Backward of posconv_ln_gelu from yg, mean, rstd (the normalised row is recomputed) and dact [B, T, H]: returns dyg [B, G, T, cg], the
    layout the weight- and data-gradient GEMMs read (rows >= `valid` exact zeros); dbias = wgrad_beta * old + column sums, or None (frozen)."""
    _cc(yg, "posconv_ln_gelu_bwd.yg"); _cc(bias, "posconv_ln_gelu_bwd.bias"); _cc(dact, "posconv_ln_gelu_bwd.dact")
    _cc(mean, "posconv_ln_gelu_bwd.mean"); _cc(rstd, "posconv_ln_gelu_bwd.rstd")
    if dact.dim() != 3:
        raise DynError("posconv_ln_gelu_bwd: dact must be [B, T, H]")
    T = dact.shape[1]
    B, G, Tg, cg, H = _posconv_dims("posconv_ln_gelu_bwd", yg, bias, T)
    if tuple(dact.shape) != (B, T, H) or mean.numel() != B * T or rstd.numel() != B * T:
        raise DynError("posconv_ln_gelu_bwd: dact / mean / rstd do not match yg")
    if dbias is not None and dbias.numel() != H:
        raise DynError("posconv_ln_gelu_bwd: dbias must have H elements")
    dyg = torch.empty(B, G, T, cg, device=yg.device, dtype=F32)
    ws = workspace(yg.device)
    check(_L().dyn_posconv_ln_gelu_bwd(yg.data_ptr(), bias.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dact.data_ptr(), dyg.data_ptr(),
                                       _opt(dbias, "dbias"), wgrad_beta, B, T, Tg, H, G, _valid_ptr(valid, "posconv_ln_gelu_bwd"),
                                       ws.data_ptr(), ws.numel(), _stream()), "dyn_posconv_ln_gelu_bwd")
    return dyg


def _squeeze_dims(who, h, yg, s):
    if not isinstance(s, int) or not 1 <= s <= 4:
        raise DynError(f"{who}: squeeze factor s = {s} must be 1, 2, 3 or 4")
    if h.dim() != 3 or yg.dim() != 4:
        raise DynError(f"{who}: h must be [B, T, H] and yg [B, G, Tg, cg]")
    B, T, H = h.shape
    G, Tg, cg = yg.shape[1:]
    if H % 256 or H > 1024:
        raise DynError(f"{who}: H = {H} must be a multiple of 256 up to 1024")
    if cg % 4:
        raise DynError(f"{who}: cg = {cg} channels per group must be a multiple of 4")
    if yg.shape[0] != B or G * cg != H or Tg < T // s:
        raise DynError(f"{who}: yg {tuple(yg.shape)} does not hold T // s = {T // s} rows of the {H} channels of h {tuple(h.shape)}")
    return B, T, H, G, Tg, cg


def squeeze_ln(h, yg, bias, gamma, beta, s, eps=1e-5, valid=None):
    """The front of SEW's squeezed encoder after the strided positional conv's grouped GEMM: z [B, T // s, H] = LayerNorm_H(the mean of s
    frames of h [B, T, H] + gelu(rows of yg [B, G, Tg >= T // s, cg] + bias)) * gamma + beta.  h and yg are left unmodified.  Returns (z,
    mean [B T2], rstd [B T2]); rows >= `valid` (device int32 scalar, squeezed frames) of z are zeros."""
    _cc(h, "squeeze_ln.h"); _cc(yg, "squeeze_ln.yg")
    B, T, H, G, Tg, cg = _squeeze_dims("squeeze_ln", h, yg, s)
    for t, n in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        if _cc(t, "squeeze_ln." + n).numel() != H:
            raise DynError(f"squeeze_ln: {n} must have H = {H} elements")
    T2 = T // s
    z = torch.empty(B, T2, H, device=h.device, dtype=F32)
    mean = torch.empty(B * T2, device=h.device, dtype=F32)
    rstd = torch.empty(B * T2, device=h.device, dtype=F32)
    check(_L().dyn_squeeze_ln_fwd(h.data_ptr(), yg.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), B, T, Tg, H, G, s, eps, _valid_ptr(valid, "squeeze_ln"), _stream()), "dyn_squeeze_ln_fwd")
    return z, mean, rstd


def squeeze_ln_bwd(h, yg, bias, gamma, mean, rstd, dz, s, dgamma, dbeta, dbias, wgrad_beta=1.0, valid=None):
    """Backward of squeeze_ln from h, yg, bias, mean, rstd (the pre-LayerNorm row is recomputed) and dz [B, T // s, H]: returns (dh [B, T, H],
    dyg [B, G, T // s, cg]): dh holds the pool's path only (rows >= s * `valid` and rows >= s (T // s) exact zeros), dyg is the layout the
    weight- and data-gradient GEMMs read (rows >= `valid` exact zeros).  dgamma / dbeta / dbias = wgrad_beta * old + column sums, or None
    (frozen)."""
    _cc(h, "squeeze_ln_bwd.h"); _cc(yg, "squeeze_ln_bwd.yg"); _cc(bias, "squeeze_ln_bwd.bias"); _cc(gamma, "squeeze_ln_bwd.gamma")
    _cc(mean, "squeeze_ln_bwd.mean"); _cc(rstd, "squeeze_ln_bwd.rstd"); _cc(dz, "squeeze_ln_bwd.dz")
    B, T, H, G, Tg, cg = _squeeze_dims("squeeze_ln_bwd", h, yg, s)
    T2 = T // s
    if tuple(dz.shape) != (B, T2, H) or mean.numel() != B * T2 or rstd.numel() != B * T2 or bias.numel() != H or gamma.numel() != H:
        raise DynError("squeeze_ln_bwd: dz / mean / rstd / bias / gamma do not match h and s")
    for t, n in ((dgamma, "dgamma"), (dbeta, "dbeta"), (dbias, "dbias")):
        if t is not None and t.numel() != H:
            raise DynError(f"squeeze_ln_bwd: {n} must have H elements")
    dh = torch.empty(B, T, H, device=h.device, dtype=F32)
    dyg = torch.empty(B, G, T2, cg, device=h.device, dtype=F32)
    ws = workspace(h.device)
    check(_L().dyn_squeeze_ln_bwd(h.data_ptr(), yg.data_ptr(), bias.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dz.data_ptr(),
                                  dh.data_ptr(), dyg.data_ptr(), _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), _opt(dbias, "dbias"), wgrad_beta,
                                  B, T, Tg, H, G, s, _valid_ptr(valid, "squeeze_ln_bwd"), ws.data_ptr(), ws.numel(), _stream()),
          "dyn_squeeze_ln_bwd")
    return dh, dyg


def _unsqueeze_dims(who, u, T, s):
    if not isinstance(s, int) or not 1 <= s <= 4:
        raise DynError(f"{who}: squeeze factor s = {s} must be 1, 2, 3 or 4")
    if u.dim() != 3 or u.shape[2] % s or (u.shape[2] // s) % 4:
        raise DynError(f"{who}: u must be [B, T2, s H] with H a multiple of 4")
    B, T2, sH = u.shape
    if T2 != T // s:
        raise DynError(f"{who}: u holds {T2} squeezed frames, T // s = {T} // {s} = {T // s} are expected")
    return B, T2, sH // s


def unsqueeze_act(u, T, s, valid=None):
    """The back of SEW's squeezed encoder after the upsampling projection u [B, T // s, s H] (bias added): [B, T, H] with gelu(u) in rows
    < s (T // s), each squeezed frame's s H channels as s frames, and exact zeros after; rows >= s * `valid` are zeros too."""
    _cc(u, "unsqueeze_act.u")
    B, T2, H = _unsqueeze_dims("unsqueeze_act", u, T, s)
    out = torch.empty(B, T, H, device=u.device, dtype=F32)
    check(_L().dyn_unsqueeze_act_fwd(u.data_ptr(), out.data_ptr(), B, T, H, s, _valid_ptr(valid, "unsqueeze_act"), _stream()),
          "dyn_unsqueeze_act_fwd")
    return out


def unsqueeze_act_bwd(u, d, s, valid=None):
    """Backward of unsqueeze_act: du [B, T // s, s H] = d * gelu'(u) with d [B, T, H]; rows >= `valid` exact zeros, d is read below s * `valid`
    only."""
    _cc(u, "unsqueeze_act_bwd.u"); _cc(d, "unsqueeze_act_bwd.d")
    if d.dim() != 3:
        raise DynError("unsqueeze_act_bwd: d must be [B, T, H]")
    T = d.shape[1]
    B, T2, H = _unsqueeze_dims("unsqueeze_act_bwd", u, T, s)
    if tuple(d.shape) != (B, T, H):
        raise DynError("unsqueeze_act_bwd: d does not match u")
    du = torch.empty_like(u)
    check(_L().dyn_unsqueeze_act_bwd(u.data_ptr(), d.data_ptr(), du.data_ptr(), B, T, H, s, _valid_ptr(valid, "unsqueeze_act_bwd"), _stream()),
          "dyn_unsqueeze_act_bwd")
    return du


def squeeze(h, yg, bias, s, valid=None):
    """squeeze_ln without the LayerNorm (SEW-D): z [B, T // s, H] = the mean of s frames of h [B, T, H] + gelu(rows of yg [B, G, Tg >= T // s,
    cg] + bias).  h and yg are left unmodified; rows >= `valid` (device int32 scalar, squeezed frames) of z are zeros."""
    _cc(h, "squeeze.h"); _cc(yg, "squeeze.yg")
    B, T, H, G, Tg, cg = _squeeze_dims("squeeze", h, yg, s)
    if _cc(bias, "squeeze.bias").numel() != H:
        raise DynError(f"squeeze: bias must have H = {H} elements")
    z = torch.empty(B, T // s, H, device=h.device, dtype=F32)
    check(_L().dyn_squeeze_fwd(h.data_ptr(), yg.data_ptr(), bias.data_ptr(), z.data_ptr(), B, T, Tg, H, G, s, _valid_ptr(valid, "squeeze"),
                               _stream()), "dyn_squeeze_fwd")
    return z


def squeeze_bwd(yg, bias, dz, T, s, dbias, wgrad_beta=1.0, valid=None):
    """Backward of squeeze from yg, bias and dz [B, T // s, H] (`T`: the frames of h): returns (dh [B, T, H], dyg [B, G, T // s, cg]) as
    squeeze_ln_bwd does; dbias = wgrad_beta * old + column sums of dyg, or None (frozen)."""
    _cc(yg, "squeeze_bwd.yg"); _cc(bias, "squeeze_bwd.bias"); _cc(dz, "squeeze_bwd.dz")
    if dz.dim() != 3 or not isinstance(T, int) or T < 0:
        raise DynError("squeeze_bwd: dz must be [B, T // s, H] and T the frame count of h")
    B, T2, H = dz.shape
    B, T, H, G, Tg, cg = _squeeze_dims("squeeze_bwd", torch.empty(B, T, H, device="meta"), yg, s)      # shapes only: h itself is not needed
    if T2 != T // s or bias.numel() != H:
        raise DynError("squeeze_bwd: dz / bias do not match T, s and yg")
    if dbias is not None and dbias.numel() != H:
        raise DynError("squeeze_bwd: dbias must have H elements")
    dh = torch.empty(B, T, H, device=dz.device, dtype=F32)
    dyg = torch.empty(B, G, T2, cg, device=dz.device, dtype=F32)
    ws = workspace(dz.device)
    check(_L().dyn_squeeze_bwd(yg.data_ptr(), bias.data_ptr(), dz.data_ptr(), dh.data_ptr(), dyg.data_ptr(), _opt(dbias, "dbias"), wgrad_beta,
                               B, T, Tg, H, G, s, _valid_ptr(valid, "squeeze_bwd"), ws.data_ptr(), ws.numel(), _stream()), "dyn_squeeze_bwd")
    return dh, dyg


def _disentangled_dims(who, S, table, n_buckets, ldp):
    """S [..., T, T] contiguous -> (M, T); the table must hold the 2T - 1 relative positions of THIS row length and ldp the n_buckets rows."""
    if S.dim() < 2 or S.shape[-1] != S.shape[-2]:
        raise DynError(f"{who}: the scores must be [..., T, T]")
    T = S.shape[-1]
    _c(table, who + ".table", I32)
    if table.numel() != 2 * T - 1:
        raise DynError(f"{who}: the bucket table holds {table.numel()} entries, 2T - 1 = {2 * T - 1} expected")
    if not isinstance(n_buckets, int) or n_buckets < 1 or ldp < n_buckets:
        raise DynError(f"{who}: ldp = {ldp} is shorter than the n_buckets = 2 * span = {n_buckets} relative positions")
    return S.numel() // (T * T), T


def softmax_disentangled(S, c2p, p2ct, table, n_buckets, ldp, out=None, valid=None):
    """SEW-D's disentangled attention probabilities: softmax_j(S[.., i, j] + c2p[.., i, t(i - j)] + p2ct[.., t(i - j), j]) over the keys, keys
    >= `valid` (device int32 scalar) masked.  S [B, nh, T, T] scaled content scores, c2p [B, nh, T, ldp] and p2ct [B, nh, ldp, T] the scaled
    position products (either may be None), `table` int32 [2T - 1] on the device with t(d) at d + T - 1 (sew_d_model.bucket_table).  `out`
    may be S."""
    _cc(S, "softmax_disentangled.S")
    M, T = _disentangled_dims("softmax_disentangled", S, table, n_buckets, ldp)
    if c2p is None and p2ct is None:
        raise DynError("softmax_disentangled: both position terms are None")
    for t, n in ((c2p, "c2p"), (p2ct, "p2ct")):
        if t is not None and _c(t, "softmax_disentangled." + n).numel() != M * T * ldp:
            raise DynError(f"softmax_disentangled: {n} holds {t.numel()} floats, {M} x {T} x {ldp} expected")
    out = torch.empty_like(S) if out is None else _cc(out, "softmax_disentangled.out")
    check(_L().dyn_softmax_disentangled_fwd(S.data_ptr(), out.data_ptr(), 0 if c2p is None else c2p.data_ptr(),
                                            0 if p2ct is None else p2ct.data_ptr(), table.data_ptr(), M, T, ldp, n_buckets,
                                            _valid_ptr(valid, "softmax_disentangled"), _stream()), "dyn_softmax_disentangled_fwd")
    return out


def disentangled_bwd(dS, table, seg_lo, seg_hi, ldp, want_c2p=True, want_p2c=True, valid=None):
    """The two gathers' backward from dS [B, nh, T, T] (softmax_bwd's output): returns (dC2P [B, nh, T, ldp] or None, dP2CT [B, nh, ldp, T] or
    None), each element one segment sum in a fixed order (bit-reproducible), both written completely.  Rows / columns >= `valid` of dS are
    not read.  seg_lo / seg_hi: int32 [n_buckets] on the device (sew_d_model.bucket_table)."""
    _cc(dS, "disentangled_bwd.dS")
    _c(seg_lo, "disentangled_bwd.seg_lo", I32); _c(seg_hi, "disentangled_bwd.seg_hi", I32)
    n_buckets = seg_lo.numel()
    if seg_hi.numel() != n_buckets:
        raise DynError("disentangled_bwd: seg_lo and seg_hi differ in length")
    M, T = _disentangled_dims("disentangled_bwd", dS, table, n_buckets, ldp)
    if not (want_c2p or want_p2c):
        raise DynError("disentangled_bwd: at least one of the two outputs must be wanted")
    lead = tuple(dS.shape[:-2])
    dc = torch.empty(lead + (T, ldp), device=dS.device, dtype=F32) if want_c2p else None
    dp = torch.empty(lead + (ldp, T), device=dS.device, dtype=F32) if want_p2c else None
    check(_L().dyn_disentangled_bwd(dS.data_ptr(), 0 if dc is None else dc.data_ptr(), 0 if dp is None else dp.data_ptr(), table.data_ptr(),
                                    seg_lo.data_ptr(), seg_hi.data_ptr(), M, T, ldp, n_buckets, _valid_ptr(valid, "disentangled_bwd"),
                                    _stream()), "dyn_disentangled_bwd")
    return dc, dp


# ----------------------------------------------------------------------------------------------- MMS adapter
def _adapter_dims(who, x, w1, w2):
    _cc(x, who + ".x"); _cc(w1, who + ".w1"); _cc(w2, who + ".w2")
    H = x.shape[-1]
    if w1.dim() != 2 or w1.shape[1] != H or tuple(w2.shape) != (H, w1.shape[0]):
        raise DynError(f"{who}: w1 {tuple(w1.shape)} / w2 {tuple(w2.shape)} must be [A, H] / [H, A] with H = {H}")
    A = w1.shape[0]
    if H % 256 or H > 2048:
        raise DynError(f"{who}: H = {H} must be a multiple of 256 up to 2048")
    if A % 4 or not 4 <= A <= 64:
        raise DynError(f"{who}: A = {A} must be a multiple of 4 from 4 to 64")
    return x.numel() // H, H, A


def attn_adapter(x, gamma, beta, w1, b1, w2, b2, eps=1e-5, out=None, save=False):
    """transformers' Wav2Vec2AttnAdapterLayer with its residual, one launch: y = x + w2 relu(w1 LayerNorm(x) + b1) + b2 over the last axis of
    x [..., H]; w1 [A, H], w2 [H, A].  `out` may be x (in place).  Returns (y, mean, rstd, a): with `save` the row statistics [rows] and the
    post-ReLU bottleneck [..., A] the backward needs, else three Nones."""
    M, H, A = _adapter_dims("attn_adapter", x, w1, w2)
    for t, n, k in ((gamma, "gamma", H), (beta, "beta", H), (b1, "b1", A), (b2, "b2", H)):
        if _cc(t, "attn_adapter." + n).numel() != k:
            raise DynError(f"attn_adapter: {n} must have {k} elements")
    y = torch.empty_like(x) if out is None else _cc(out, "attn_adapter.out")
    if y.shape != x.shape:
        raise DynError("attn_adapter: out must have the shape of x")
    mean = rstd = a = None
    if save:
        mean = torch.empty(M, device=x.device, dtype=F32)
        rstd = torch.empty(M, device=x.device, dtype=F32)
        a = torch.empty(x.shape[:-1] + (A,), device=x.device, dtype=F32)
    check(_L().dyn_attn_adapter_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                    y.data_ptr(), _opt(mean, "mean"), _opt(rstd, "rstd"), _opt(a, "a"), M, H, A, eps, _stream()),
          "dyn_attn_adapter_fwd")
    return y, mean, rstd, a


def attn_adapter_bwd(x, gamma, beta, w1, w2, mean, rstd, a, dy, dgamma, dbeta, dw1, db1, dw2, db2, dx=None):
    """Backward of attn_adapter from its input x, the saved (mean, rstd, a) and dy: returns dx = dy + the adapter path, out of place (dy may be
    a queued weight-gradient operand; x and dy are left unmodified).  The six gradients += their sums over the rows, each in a fixed order
    (no atomics; bit-reproducible); None: frozen, not computed."""
    M, H, A = _adapter_dims("attn_adapter_bwd", x, w1, w2)
    _cc(dy, "attn_adapter_bwd.dy"); _cc(a, "attn_adapter_bwd.a"); _cc(gamma, "attn_adapter_bwd.gamma"); _cc(beta, "attn_adapter_bwd.beta")
    _c(mean, "attn_adapter_bwd.mean"); _c(rstd, "attn_adapter_bwd.rstd")
    if dy.shape != x.shape or a.numel() != M * A or mean.numel() != M or rstd.numel() != M or gamma.numel() != H or beta.numel() != H:
        raise DynError("attn_adapter_bwd: dy / a / mean / rstd / gamma / beta do not match x and the weights")
    for t, n, k in ((dgamma, "dgamma", H), (dbeta, "dbeta", H), (dw1, "dw1", A * H), (db1, "db1", A), (dw2, "dw2", A * H), (db2, "db2", H)):
        if t is not None and _cc(t, "attn_adapter_bwd." + n).numel() != k:
            raise DynError(f"attn_adapter_bwd: {n} must have {k} elements")
    dx = torch.empty_like(dy) if dx is None else _cc(dx, "attn_adapter_bwd.dx")
    if dx.shape != dy.shape or dx.data_ptr() in (dy.data_ptr(), x.data_ptr()):
        raise DynError("attn_adapter_bwd: dx must have the shape of dy and alias neither dy nor x")
    ws = workspace(x.device)
    check(_L().dyn_attn_adapter_bwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w1.data_ptr(), w2.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    a.data_ptr(), dy.data_ptr(), dx.data_ptr(), _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), _opt(dw1, "dw1"),
                                    _opt(db1, "db1"), _opt(dw2, "dw2"), _opt(db2, "db2"), M, H, A, ws.data_ptr(), ws.numel(), _stream()),
          "dyn_attn_adapter_bwd")
    return dx


# ----------------------------------------------------------------------------------------------- Wav2Vec2-BERT
CAUSAL_ACTS = {"swish": 0, "silu": 0, "gelu": 1}


def _convmod_causal(name, u, w, cbias, gamma, beta, act, eps, save, launch):
    """The checks and buffers of convmod_causal / convmod_causal_k9; `launch(s, g, c, n, mean, rstd, B, T, C)` calls the entry."""
    _cc(u, name + ".u"); _cc(w, name + ".w"); _cc(gamma, name + ".gamma"); _cc(beta, name + ".beta")
    if act is not None and act not in CAUSAL_ACTS:
        raise DynError(f"{name}: act={act!r} is not built ({sorted(CAUSAL_ACTS)})")
    if u.dim() != 3 or u.shape[2] % 2 or w.dim() != 2 or w.shape[0] != u.shape[2] // 2 or gamma.numel() != w.shape[0] or beta.numel() != w.shape[0]:
        raise DynError(f"{name}: u must be [B, T, 2C], w [C, KW], gamma and beta [C]")
    B, T, C2 = u.shape
    C = C2 // 2
    if cbias is not None and _cc(cbias, name + ".cbias").numel() != C:
        raise DynError(f"{name}: cbias must be [C]")
    s = torch.empty(B, T, C, device=u.device, dtype=F32)
    g = c = n = mean = rstd = None
    if save:
        g, c, n = (torch.empty(B, T, C, device=u.device, dtype=F32) for _ in range(3))
        mean, rstd = (torch.empty(B * T, device=u.device, dtype=F32) for _ in range(2))
    outs = (s.data_ptr(), _opt(g, "g"), _opt(c, "c"), _opt(n, "n"), _opt(mean, "mean"), _opt(rstd, "rstd"))
    check(launch(outs, B, T, C), f"dyn_{name}_fwd")
    return s, g, c, n, mean, rstd


def _dwconv1d_causal_dgrad(name, dy, w, out, beta):
    _cc(dy, name + ".dy"); _cc(w, name + ".w")
    B, T, C = dy.shape
    if w.shape[0] != C:
        raise DynError(f"{name}: w must be [C, KW]")
    out = torch.empty_like(dy) if out is None else _cc(out, name + ".out")
    if out.shape != dy.shape or out.data_ptr() == dy.data_ptr():
        raise DynError(f"{name}: out must have the shape of dy and not alias it")
    check(getattr(_L(), "dyn_" + name)(dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, T, C, w.shape[1], beta, _stream()), "dyn_" + name)
    return out


def _dwconv1d_causal_wgrad(name, x, dy, dw, beta):
    _cc(x, name + ".x"); _cc(dy, name + ".dy"); _cc(dw, name + ".dw")
    B, T, C = x.shape
    if dy.shape != x.shape or dw.dim() != 2 or dw.shape[0] != C:
        raise DynError(f"{name}: dy must have the shape of x, dw must be [C, KW]")
    ws = workspace(x.device)
    check(getattr(_L(), "dyn_" + name)(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), beta, B, T, C, dw.shape[1], ws.data_ptr(), ws.numel(), _stream()),
          "dyn_" + name)
    return dw


def convmod_causal(u, w, gamma, beta, act="swish", eps=1e-5, save=False, time_tile=0):
    """Wav2Vec2-BERT's conv-module core in one launch: u [B, T, 2C] -> s [B, T, C] = act(LayerNorm_C(causal depthwise conv(GLU(u)))), w [C, 31],
    zeros left of frame 0.  Returns (s, g, c, n, mean, rstd): with `save` the GLU output, the convolution output, the LayerNorm output and the
    row statistics the backward needs, else five Nones.  `time_tile`: 0 (the library's choice), 8 or 16 frames per workgroup."""
    return _convmod_causal("convmod_causal", u, w, None, gamma, beta, act, eps, save, lambda outs, B, T, C: _L().dyn_convmod_causal_fwd(
        u.data_ptr(), w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *outs, B, T, C, w.shape[1], CAUSAL_ACTS[act], eps, int(time_tile), _stream()))


def dwconv1d_causal_dgrad(dy, w, out=None, beta=0.0):
    """dx [B, T, C] = beta * dx + the input gradient of the left-padded depthwise convolution (w [C, KW]) from dy [B, T, C]."""
    return _dwconv1d_causal_dgrad("dwconv1d_causal_dgrad", dy, w, out, beta)


def dwconv1d_causal_wgrad(x, dy, dw, beta=1.0):
    """dw [C, KW] = beta * dw + the weight gradient of the left-padded depthwise convolution of x [B, T, C] from dy [B, T, C]."""
    return _dwconv1d_causal_wgrad("dwconv1d_causal_wgrad", x, dy, dw, beta)


def narrow_layernorm(x, gamma, beta, eps=1e-5, out=None):
    """LayerNorm over the last axis of x [..., C] for a narrow row (C % 4 == 0, C <= 256; ops.layernorm needs C % 256 == 0): (y, mean, rstd)."""
    _cc(x, "narrow_layernorm.x"); _cc(gamma, "narrow_layernorm.gamma")
    C = x.shape[-1]
    if gamma.numel() != C or (beta is not None and beta.numel() != C):
        raise DynError("narrow_layernorm: gamma / beta must have C elements")
    rows = x.numel() // C
    out = torch.empty_like(x) if out is None else _cc(out, "narrow_layernorm.out")
    mean = torch.empty(rows, device=x.device, dtype=F32)
    rstd = torch.empty(rows, device=x.device, dtype=F32)
    check(_L().dyn_narrow_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), _opt(beta, "beta"), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        rows, C, eps, _stream()), "dyn_narrow_layernorm_fwd")
    return out, mean, rstd


def narrow_layernorm_bwd(x, gamma, mean, rstd, dy, dgamma, dbeta, dx=None, wgrad_beta=1.0):
    """Backward of narrow_layernorm: dgamma / dbeta = wgrad_beta * old + their sums over the rows (None: not computed), dx written when given
    (None: the input is data).  Returns dx."""
    _cc(x, "narrow_layernorm_bwd.x"); _cc(gamma, "narrow_layernorm_bwd.gamma"); _cc(dy, "narrow_layernorm_bwd.dy")
    _c(mean, "narrow_layernorm_bwd.mean"); _c(rstd, "narrow_layernorm_bwd.rstd")
    C = x.shape[-1]
    rows = x.numel() // C
    if dy.shape != x.shape or mean.numel() != rows or rstd.numel() != rows or gamma.numel() != C:
        raise DynError("narrow_layernorm_bwd: dy / mean / rstd / gamma do not match x")
    for t, n in ((dgamma, "dgamma"), (dbeta, "dbeta")):
        if t is not None and _cc(t, "narrow_layernorm_bwd." + n).numel() != C:
            raise DynError(f"narrow_layernorm_bwd: {n} must have C elements")
    if dx is not None and _cc(dx, "narrow_layernorm_bwd.dx").shape != x.shape:
        raise DynError("narrow_layernorm_bwd: dx must have the shape of x")
    ws = workspace(x.device)
    check(_L().dyn_narrow_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), _opt(dx, "dx"),
                                        _opt(dgamma, "dgamma"), _opt(dbeta, "dbeta"), wgrad_beta, rows, C, ws.data_ptr(), ws.numel(), _stream()),
          "dyn_narrow_layernorm_bwd")
    return dx


FBANK_MEL_FLOOR = 1.192092955078125e-07     # SeamlessM4TFeatureExtractor: float32 epsilon, as Kaldi


def fbank_finish(mel, valid=None, mel_floor=FBANK_MEL_FLOOR, eps=1e-7):
    """mel [B, F, M] filter-bank energies -> [B, F // 2, 2M], per sample: log(max(mel, floor)), per-bin (mean, unbiased variance) normalisation
    over the first `valid` frames (device int32 scalar; None: all), two frames stacked per row; rows past valid // 2 are zeros."""
    _c(mel, "fbank_finish.mel")
    if mel.dim() != 3 or mel.shape[1] < 2:
        raise DynError("fbank_finish: mel must be [B, F, M] with at least two frames (the unbiased variance of one frame is undefined)")
    B, F, M = mel.shape
    out = torch.empty(B, F // 2, 2 * M, device=mel.device, dtype=F32)
    check(_L().dyn_fbank_finish(mel.data_ptr(), out.data_ptr(), B, F, M, mel_floor, eps, _valid_ptr(valid, "fbank_finish"), _stream()),
          "dyn_fbank_finish")
    return out


def melfeat_prep(x, lens, out, pad, preemphasis, noise=None, dither=0.0, prev=None):
    """x [B, Lmax] waveforms, lens int32 CUDA [B] sample counts -> out [B, W] (W >= pad + Lmax, every element written): `pad` zeros, then
    the row after dither (noise [B, Lmax], None: none), pre-emphasis over the whole signal (sample 0 kept, or filtered against prev[b], the
    last sample of the chunk before) and the length mask (zeros at and past lens[b], whatever x holds there)."""
    _c(x, "melfeat_prep.x"); _c(out, "melfeat_prep.out")
    if x.dim() != 2 or out.dim() != 2 or out.shape[0] != x.shape[0]:
        raise DynError("melfeat_prep: x must be [B, Lmax] and out [B, W]")
    B, Lmax = x.shape
    if noise is not None and _c(noise, "melfeat_prep.noise").shape != x.shape:
        raise DynError("melfeat_prep: noise must have the shape of x")
    if prev is not None and tuple(_c(prev, "melfeat_prep.prev").shape) != (B,):
        raise DynError("melfeat_prep: prev must be [B]")
    check(_L().dyn_melfeat_prep(x.data_ptr(), out.data_ptr(), _lens_ptr(lens, B, "melfeat_prep"), None if noise is None else noise.data_ptr(),
                                None if prev is None else prev.data_ptr(), B, Lmax, pad, out.shape[1], preemphasis, dither, _stream()),
          "dyn_melfeat_prep")
    return out


def melfeat_finish(mel, lens, guard, clamp, normalize, eps=1e-5, layout="tf", out=None):
    """mel [B, T, F] energies, lens int32 CUDA [B] valid frames -> [B, T, F] (layout "tf") or [B, F, T] ("ft"): log(mel + guard), or
    log(max(mel, guard)) when `clamp`; `normalize`: (v - mean) / (std + eps) per row and bin over the row's valid frames (unbiased std, centred
    second pass, fixed order); frames >= lens[b] exact zeros."""
    _c(mel, "melfeat_finish.mel")
    if mel.dim() != 3 or layout not in ("tf", "ft"):
        raise DynError("melfeat_finish: mel must be [B, T, F] and layout \"tf\" or \"ft\"")
    B, T, F = mel.shape
    shape = (B, T, F) if layout == "tf" else (B, F, T)
    if out is None:
        out = torch.empty(shape, device=mel.device, dtype=F32)
    elif tuple(_c(out, "melfeat_finish.out").shape) != shape:
        raise DynError(f"melfeat_finish: out must be {shape}")
    ws = workspace(mel.device)
    check(_L().dyn_melfeat_finish(mel.data_ptr(), out.data_ptr(), _lens_ptr(lens, B, "melfeat_finish"), B, T, F, guard, int(bool(clamp)),
                                  int(bool(normalize)), eps, 0 if layout == "tf" else 1, ws.data_ptr(), ws.numel(), _stream()),
          "dyn_melfeat_finish")
    return out


def relkey_embed_grad(dc2p, q, dE, scale, beta=1.0):
    """The gradient of Wav2Vec2-BERT's shared distance embedding E [P, D] (`self_attn.distance_embedding.weight`, one table for all heads):
        dE[p, :] = beta * dE[p, :] + scale * sum_{b, h, i} dC2P[b, h, i, P - 1 - p] * q[b, h, i, :]
    dc2p [B, nh, T, ldp] is ops.disentangled_bwd's first output over the REVERSED table (column r belongs to E[P - 1 - r]), q an _attn.View
    of the queries.  Four launches whatever B * nh is: one strided batched GEMM leaves every (b, h)'s [P, D] product as a partial row, the
    fixed-order reducer sums them (bit-reproducible: two calls give equal bits), the rows are reversed by a copy and accumulated into dE."""
    _cc(dc2p, "relkey_embed_grad.dc2p"); _cc(dE, "relkey_embed_grad.dE")
    if dc2p.dim() != 4 or dE.dim() != 2:
        raise DynError("relkey_embed_grad: dc2p must be [B, nh, T, ldp], dE [P, D]")
    B, nh, T, ldp = dc2p.shape
    P, D = dE.shape
    if P > ldp or D != q.sh:
        raise DynError(f"relkey_embed_grad: dE [{P}, {D}] does not fit dc2p's {ldp} columns / the head dimension {q.sh}")
    part = torch.empty(B * nh, P, D, device=dE.device, dtype=F32)
    gemm(dc2p, q.t, part, trans_a=True, M=P, N=D, K=T, lda=ldp, ldb=q.ld, ldc=D, nb1=B, nb2=nh, sa=(nh * T * ldp, T * ldp), sb=(q.sb, q.sh),
         sc=(nh * P * D, P * D), b_off=q.off, alpha=scale)
    rev = torch.empty(P, D, device=dE.device, dtype=F32)
    reduce_partials(part, rev, beta=0.0)
    return axpby(rev.flip(0), dE, 1.0, beta)


# ----------------------------------------------------------------------------------------------- Parakeet (FastConformer)
CONVMOD_BN_ACTS = {"silu": 0, "swish": 0}
SUBSAMPLING_ACTS = {"silu": 0, "relu": 1}


CONVMOD_BN_WIDTHS = (9, 32)        # instances of dyn_convmod_bn_fwd / dyn_glu_dwconv1d_dgrad


def convmod_bn_time_tile(kw=None):
    """Frames per workgroup of the conv-module kernels below (tests place their edges around it): of the 9-tap instances, or of `kw` taps."""
    if kw is None:
        return int(_L().dyn_convmod_bn_time_tile())
    tt = int(_L().dyn_convmod_bn_time_tile_kw(int(kw)))
    if tt <= 0:
        raise DynError(f"convmod_bn_time_tile: kernel width {kw} is not built {CONVMOD_BN_WIDTHS}")
    return tt


def _bn_operands(what, C, mean, var, weight, bias):
    for n, t in (("mean", mean), ("var", var), ("weight", weight), ("bias", bias)):
        _cc(t, f"{what}.{n}")
        if t.numel() != C:
            raise DynError(f"{what}: {n} must have C = {C} elements")


def convmod_bn(u, w, cbias, mean, var, weight, bias, act="silu", eps=1e-5, valid=None, save=False, lens=None):
    """Parakeet's conv-module core in one launch: u [B, T, 2C] -> s [B, T, C] = act(BatchNorm_eval(cbias + depthwise conv(GLU(u)))), w [C, 9]
    or [C, 32] (LASR; 15 frames of padding left, 16 right, as torch's padding="same"), zero SAME padding; cbias None: no convolution bias.  `valid` (device int32 scalar): GLU rows past it read as zeros, output rows past it are
    zeros; `lens` (int32 CUDA [B]) in its place: the same with lens[b] for batch entry b.  Returns (s, gl, c): with `save` the masked GLU
    output and the convolution output the backward needs, else two Nones."""
    valid, lens = _split_valid(valid, lens)
    _cc(u, "convmod_bn.u"); _cc(w, "convmod_bn.w")
    if act not in CONVMOD_BN_ACTS:
        raise DynError(f"convmod_bn: act={act!r} is not built ({sorted(CONVMOD_BN_ACTS)})")
    if u.dim() != 3 or u.shape[2] % 2 or w.dim() != 2 or w.shape[0] != u.shape[2] // 2:
        raise DynError("convmod_bn: u must be [B, T, 2C], w [C, KW]")
    B, T, C2 = u.shape
    C = C2 // 2
    _bn_operands("convmod_bn", C, mean, var, weight, bias)
    if cbias is not None and cbias.numel() != C:
        raise DynError(f"convmod_bn: cbias must have C = {C} elements")
    s = torch.empty(B, T, C, device=u.device, dtype=F32)
    gl = c = None
    if save:
        gl, c = (torch.empty(B, T, C, device=u.device, dtype=F32) for _ in range(2))
    fn, vp = (_L().dyn_convmod_bn_fwd, _valid_ptr(valid, "convmod_bn")) if lens is None else \
        (_L().dyn_convmod_bn_fwd_lens, _lens_ptr(lens, B, "convmod_bn", valid))
    check(fn(u.data_ptr(), w.data_ptr(), _opt(cbias, "cbias"), mean.data_ptr(), var.data_ptr(), weight.data_ptr(), bias.data_ptr(),
             s.data_ptr(), _opt(gl, "gl"), _opt(c, "c"), vp, B, T, C, w.shape[1], CONVMOD_BN_ACTS[act], eps, _stream()),
          "dyn_convmod_bn_fwd" if lens is None else "dyn_convmod_bn_fwd_lens")
    return s, gl, c


def convmod_bn_bwd_act(c, mean, var, weight, bias, ds, dweight, dbias, dcbias, act="silu", eps=1e-5, valid=None, out=None, wgrad_beta=1.0,
                       lens=None):
    """Backward of convmod_bn's activation and BatchNorm: returns dc [B, T, C] = ds * act'(bn) * weight * rstd (`out` may be ds), and
    accumulates dweight / dbias / dcbias = wgrad_beta * old + their column sums (None: frozen, not computed).  Rows past `valid` (or past
    lens[b], `lens` int32 CUDA [B]): dc = 0, left out of the sums."""
    valid, lens = _split_valid(valid, lens)
    _cc(c, "convmod_bn_bwd_act.c"); _cc(ds, "convmod_bn_bwd_act.ds")
    if act not in CONVMOD_BN_ACTS:
        raise DynError(f"convmod_bn_bwd_act: act={act!r} is not built ({sorted(CONVMOD_BN_ACTS)})")
    if c.dim() != 3 or ds.shape != c.shape:
        raise DynError("convmod_bn_bwd_act: c and ds must be [B, T, C]")
    B, T, C = c.shape
    _bn_operands("convmod_bn_bwd_act", C, mean, var, weight, bias)
    for n, t in (("dweight", dweight), ("dbias", dbias), ("dcbias", dcbias)):
        if t is not None and _cc(t, f"convmod_bn_bwd_act.{n}").numel() != C:
            raise DynError(f"convmod_bn_bwd_act: {n} must have C = {C} elements")
    out = torch.empty_like(ds) if out is None else _cc(out, "convmod_bn_bwd_act.out")
    if out.shape != ds.shape:
        raise DynError("convmod_bn_bwd_act: out must have the shape of ds")
    ws = workspace(c.device)
    fn, vp = (_L().dyn_convmod_bn_bwd_act, _valid_ptr(valid, "convmod_bn_bwd_act")) if lens is None else \
        (_L().dyn_convmod_bn_bwd_act_lens, _lens_ptr(lens, B, "convmod_bn_bwd_act", valid))
    check(fn(c.data_ptr(), mean.data_ptr(), var.data_ptr(), weight.data_ptr(), bias.data_ptr(), ds.data_ptr(), out.data_ptr(),
             _opt(dweight, "dweight"), _opt(dbias, "dbias"), _opt(dcbias, "dcbias"), wgrad_beta, vp, B, T, C, CONVMOD_BN_ACTS[act], eps,
             ws.data_ptr(), ws.numel(), _stream()), "dyn_convmod_bn_bwd_act" if lens is None else "dyn_convmod_bn_bwd_act_lens")
    return out


def glu_dwconv1d_dgrad(u, w, dc, valid=None, out=None, lens=None):
    """du [B, T, 2C] = GLU'(u) * (the input gradient of the SAME-padded depthwise convolution w [C, 9] or [C, 32] from dc [B, T, C]) in one pass; rows past
    `valid` (or past lens[b], `lens` int32 CUDA [B]) are zeros."""
    valid, lens = _split_valid(valid, lens)
    _cc(u, "glu_dwconv1d_dgrad.u"); _cc(w, "glu_dwconv1d_dgrad.w"); _cc(dc, "glu_dwconv1d_dgrad.dc")
    if u.dim() != 3 or dc.dim() != 3 or u.shape[:2] != dc.shape[:2] or u.shape[2] != 2 * dc.shape[2] or w.dim() != 2 or w.shape[0] != dc.shape[2]:
        raise DynError("glu_dwconv1d_dgrad: u must be [B, T, 2C], dc [B, T, C], w [C, KW]")
    B, T, C = dc.shape
    out = torch.empty_like(u) if out is None else _cc(out, "glu_dwconv1d_dgrad.out")
    if out.shape != u.shape or out.data_ptr() in (u.data_ptr(), dc.data_ptr()):
        raise DynError("glu_dwconv1d_dgrad: out must have the shape of u and alias neither u nor dc")
    fn, vp = (_L().dyn_glu_dwconv1d_dgrad, _valid_ptr(valid, "glu_dwconv1d_dgrad")) if lens is None else \
        (_L().dyn_glu_dwconv1d_dgrad_lens, _lens_ptr(lens, B, "glu_dwconv1d_dgrad", valid))
    check(fn(u.data_ptr(), w.data_ptr(), dc.data_ptr(), out.data_ptr(), vp, B, T, C, w.shape[1], _stream()),
          "dyn_glu_dwconv1d_dgrad" if lens is None else "dyn_glu_dwconv1d_dgrad_lens")
    return out


def batch_renorm_clamps(num_batches_tracked):
    """(rmax, dmax) of BatchRenorm1d's schedule at `num_batches_tracked` (the value BEFORE the forward's increment): host arithmetic,
    rmax = clamp(2 / 35000 * n + 25 / 35, 1, 3), dmax = clamp(5 / 20000 * n - 25 / 20, 0, 5).  (1, 0) at 0: plain training-mode batch norm;
    (3, 5) from 40000 / 25000 on, so at the reference's 1000000 (nvidia_ctc/lib.py:97)."""
    n = float(num_batches_tracked)
    return min(max(2.0 / 35000.0 * n + 25.0 / 35.0, 1.0), 3.0), min(max(5.0 / 20000.0 * n - 25.0 / 20.0, 0.0), 5.0)


def convmod_brn_stats_rows():
    return int(_L().dyn_convmod_brn_stats_rows())


def convmod_brn(u, w, cbias, running_mean, running_std, weight, bias, rmax, dmax, momentum, act="silu", eps=1e-5, valid=None):
    """The conv-module core with BatchRenorm1d in TRAINING mode (reference nvidia_ctc/lib.py:74,89-102; the `batchrenorm` package form, parity
    unpinned against upstream `lcasr`): u [B, T, 2C] -> s = act(weight * ((x - mu) / sig * r + d) + bias), x = cbias + depthwise conv(GLU(u)),
    mu / sig = std + eps the statistics of the batch's B * valid rows, r / d the clamped (rmax, dmax) corrections towards running_mean /
    running_std, which then move IN PLACE by `momentum` (0: untouched).  Returns (s, gl, c, stats): gl, c as convmod_bn's, stats [7, C] =
    mu, 1 / sig, r, d, scale, shift, 1 / std for convmod_brn_bwd.  A channel of zero batch variance is outside the contract."""
    _cc(u, "convmod_brn.u"); _cc(w, "convmod_brn.w")
    if act not in CONVMOD_BN_ACTS:
        raise DynError(f"convmod_brn: act={act!r} is not built ({sorted(CONVMOD_BN_ACTS)})")
    if u.dim() != 3 or u.shape[2] % 2 or w.dim() != 2 or w.shape[0] != u.shape[2] // 2:
        raise DynError("convmod_brn: u must be [B, T, 2C], w [C, KW]")
    B, T, C2 = u.shape
    C = C2 // 2
    _bn_operands("convmod_brn", C, running_mean, running_std, weight, bias)
    if cbias is not None and cbias.numel() != C:
        raise DynError(f"convmod_brn: cbias must have C = {C} elements")
    s, gl, c = (torch.empty(B, T, C, device=u.device, dtype=F32) for _ in range(3))
    stats = torch.empty(convmod_brn_stats_rows(), C, device=u.device, dtype=F32)
    ws = workspace(u.device)
    check(_L().dyn_convmod_brn_fwd(u.data_ptr(), w.data_ptr(), _opt(cbias, "cbias"), running_mean.data_ptr(), running_std.data_ptr(),
                                   weight.data_ptr(), bias.data_ptr(), s.data_ptr(), gl.data_ptr(), c.data_ptr(), stats.data_ptr(),
                                   _valid_ptr(valid, "convmod_brn"), B, T, C, w.shape[1], CONVMOD_BN_ACTS[act], eps, rmax, dmax, momentum,
                                   ws.data_ptr(), ws.numel(), _stream()), "dyn_convmod_brn_fwd")
    return s, gl, c, stats


def convmod_brn_bwd(c, stats, ds, dweight, dbias, dcbias, act="silu", valid=None, out=None, wgrad_beta=1.0):
    """Backward of convmod_brn's activation and training-mode BatchRenorm1d through the batch mean and deviation (r, d constants): returns dc
    [B, T, C] (`out` may be ds) and writes dweight / dbias = wgrad_beta * old + their sums (None: frozen).  dcbias = wgrad_beta * old: the
    convolution bias cancels in x - mu.  The gradient reaches every row of the batch.  Rows past `valid`: dc = 0, left out of the sums."""
    _cc(c, "convmod_brn_bwd.c"); _cc(ds, "convmod_brn_bwd.ds"); _cc(stats, "convmod_brn_bwd.stats")
    if act not in CONVMOD_BN_ACTS:
        raise DynError(f"convmod_brn_bwd: act={act!r} is not built ({sorted(CONVMOD_BN_ACTS)})")
    if c.dim() != 3 or ds.shape != c.shape:
        raise DynError("convmod_brn_bwd: c and ds must be [B, T, C]")
    B, T, C = c.shape
    if stats.dim() != 2 or tuple(stats.shape) != (convmod_brn_stats_rows(), C):
        raise DynError(f"convmod_brn_bwd: stats must be convmod_brn's [{convmod_brn_stats_rows()}, C = {C}]")
    for n, t in (("dweight", dweight), ("dbias", dbias), ("dcbias", dcbias)):
        if t is not None and _cc(t, f"convmod_brn_bwd.{n}").numel() != C:
            raise DynError(f"convmod_brn_bwd: {n} must have C = {C} elements")
    out = torch.empty_like(ds) if out is None else _cc(out, "convmod_brn_bwd.out")
    if out.shape != ds.shape:
        raise DynError("convmod_brn_bwd: out must have the shape of ds")
    ws = workspace(c.device)
    check(_L().dyn_convmod_brn_bwd(c.data_ptr(), stats.data_ptr(), ds.data_ptr(), out.data_ptr(), _opt(dweight, "dweight"), _opt(dbias, "dbias"),
                                   _opt(dcbias, "dcbias"), wgrad_beta, _valid_ptr(valid, "convmod_brn_bwd"), B, T, C, CONVMOD_BN_ACTS[act],
                                   ws.data_ptr(), ws.numel(), _stream()), "dyn_convmod_brn_bwd")
    return out


def _sub_act(act, what):
    if act not in SUBSAMPLING_ACTS:
        raise DynError(f"{what}: act={act!r} is not built ({sorted(SUBSAMPLING_ACTS)})")
    return SUBSAMPLING_ACTS[act]


def _stage_lens(what, B, lens_in, lens_out):
    if (lens_in is None) != (lens_out is None):
        raise DynError(f"{what}: lens_in and lens_out go together")
    return None if lens_in is None else (_lens_ptr(lens_in, B, what + ".lens_in"), _lens_ptr(lens_out, B, what + ".lens_out"))


def dwconv2d_s2_act(z, w, bias, act, out=None, lens_in=None, lens_out=None):
    """u = bias + dw3x3_s2(act(z)), act "silu" (ops.dwconv2d_s2) or "relu"; z [B, T, F, C] -> [B, To, Fo, C]; w [C, 3, 3].  `lens_in` /
    `lens_out` (int32 CUDA [B], together): rows t >= lens_in[b] of z read as zeros, rows to >= lens_out[b] of u are written as zeros."""
    a = _sub_act(act, "dwconv2d_s2_act")
    _cc(z, "dwconv2d_s2_act.z"); _cc(w, "dwconv2d_s2_act.w"); _cc(bias, "dwconv2d_s2_act.bias")
    B, T, F, C = z.shape
    if out is None:
        out = torch.empty(B, out_len(T), out_len(F), C, device=z.device, dtype=F32)
    ll = _stage_lens("dwconv2d_s2_act", B, lens_in, lens_out)
    if ll is not None:
        check(_L().dyn_dwconv2d_s2_fwd_act_lens(z.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, a, ll[0], ll[1], _stream()),
              "dyn_dwconv2d_s2_fwd_act_lens")
        return out
    check(_L().dyn_dwconv2d_s2_fwd_act(z.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, a, _stream()),
          "dyn_dwconv2d_s2_fwd_act")
    return out


def dwconv2d_s2_dgrad_act(z, w, du, act, out=None, lens_in=None, lens_out=None):
    """dz of dwconv2d_s2_act from du.  `lens_in` / `lens_out`: rows t >= lens_in[b] of dz are zeros, rows to >= lens_out[b] of du are not read."""
    a = _sub_act(act, "dwconv2d_s2_dgrad_act")
    _cc(z, "dwconv2d_s2_dgrad_act.z"); _cc(du, "dwconv2d_s2_dgrad_act.du"); _cc(w, "dwconv2d_s2_dgrad_act.w")
    B, T, F, C = z.shape
    out = torch.empty_like(z) if out is None else _cc(out, "dwconv2d_s2_dgrad_act.out")
    ll = _stage_lens("dwconv2d_s2_dgrad_act", B, lens_in, lens_out)
    if ll is not None:
        check(_L().dyn_dwconv2d_s2_dgrad_act_lens(z.data_ptr(), w.data_ptr(), du.data_ptr(), out.data_ptr(), B, T, F, C, a, ll[0], ll[1],
                                                  _stream()), "dyn_dwconv2d_s2_dgrad_act_lens")
        return out
    check(_L().dyn_dwconv2d_s2_dgrad_act(z.data_ptr(), w.data_ptr(), du.data_ptr(), out.data_ptr(), B, T, F, C, a, _stream()),
          "dyn_dwconv2d_s2_dgrad_act")
    return out


def dwconv2d_s2_wgrad_act(z, du, dw, dbias, act, beta=1.0, lens_in=None):
    """dw, dbias = beta * old + the gradients of dwconv2d_s2_act.  `lens_in` (int32 CUDA [B]): rows t >= lens_in[b] of z read as zeros (du is
    zero past the output length already)."""
    a = _sub_act(act, "dwconv2d_s2_wgrad_act")
    _cc(z, "dwconv2d_s2_wgrad_act.z"); _cc(du, "dwconv2d_s2_wgrad_act.du"); _cc(dw, "dwconv2d_s2_wgrad_act.dw"); _cc(dbias, "dwconv2d_s2_wgrad_act.dbias")
    B, T, F, C = z.shape
    ws = workspace(z.device)
    if lens_in is not None:
        check(_L().dyn_dwconv2d_s2_wgrad_act_lens(z.data_ptr(), du.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C, a,
                                                  _lens_ptr(lens_in, B, "dwconv2d_s2_wgrad_act"), ws.data_ptr(), ws.numel(), _stream()),
              "dyn_dwconv2d_s2_wgrad_act_lens")
        return
    check(_L().dyn_dwconv2d_s2_wgrad_act(z.data_ptr(), du.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C, a, ws.data_ptr(),
                                         ws.numel(), _stream()), "dyn_dwconv2d_s2_wgrad_act")


def relu(x, out=None):
    _cc(x, "relu.x")
    out = torch.empty_like(x) if out is None else _cc(out, "relu.out")
    check(_L().dyn_relu_fwd(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_relu_fwd")
    return out


def relu_bwd(x, dy, out=None):
    """dx = dy where x > 0, else 0 (x: the activation's INPUT, or its output: the masks agree); out may be dy."""
    _cc(x, "relu_bwd.x"); _cc(dy, "relu_bwd.dy")
    out = torch.empty_like(dy) if out is None else _cc(out, "relu_bwd.out")
    check(_L().dyn_relu_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _stream()), "dyn_relu_bwd")
    return out


# ----------------------------------------------------------------------------------------------- transducer head (csrc/transducer.hip)
JOINT_ACTS = {"relu": 0}
TDT_REDUCTIONS = {"sum": 0, "mean_batch": 1, "mean": 2, "mean_volume": 3, "none": 4}
TDT_MAX_DURATIONS = 8
TDT_WORKSPACE_BUDGET = 512 << 20      # bytes of lattice state (44 B per cell at D = 5) a TDT loss may ask for; the state is never chunked
# Bytes of z + logits + dz a transducer head may hold at once before it streams the joint over frame chunks (parakeet_tdt_model.
# plan_joint_chunk).  A memory policy, not a tuned figure: nothing was timed to pick it; it is large enough that every shape the tests
# and the 16-frame windows of the loop use stays on the whole-joint path.
TDT_JOINT_BUDGET = 8 << 30


def _joint_act(act, what):
    if act not in JOINT_ACTS:
        raise DynError(f"{what}: hidden_act={act!r} is not built ({sorted(JOINT_ACTS)})")
    return JOINT_ACTS[act]


def check_durations(durations, what="durations"):
    """The duration list of a TDT head as a tuple of ints: 1 .. 8 values, non-negative, strictly ascending, at least one positive."""
    d = tuple(int(v) for v in durations)
    if not 1 <= len(d) <= TDT_MAX_DURATIONS:
        raise DynError(f"{what}: {len(d)} durations are not built (1 .. {TDT_MAX_DURATIONS})")
    if any(v < 0 for v in d):
        raise DynError(f"{what}: negative durations {d} are not built")
    if any(b <= a for a, b in zip(d, d[1:])):
        raise DynError(f"{what}: unsorted durations {d} are not built (strictly ascending)")
    if d[-1] == 0:
        raise DynError(f"{what}: durations {d} hold no positive value: no arc advances the frame")
    return d


def _durations_arg(durations):
    """-> (the duration arguments of a C entry: (int32 array, D); none for `durations` None, a head without durations; D)."""
    if durations is None:
        return (), 0
    d = check_durations(durations)
    return (ctypes.cast((ctypes.c_int32 * len(d))(*d), ctypes.c_void_p), len(d)), len(d)


def lstm_cell(xg, hg, c_prev=None, save=False, out=None):
    """gates = xg + hg [Bd, 4 Hd] (i | f | g | o) -> (c, h, gate activations or None); `out` = (c, h, gates or None) to write into."""
    _cc(xg, "lstm_cell.xg"); _cc(hg, "lstm_cell.hg")
    Bd, H4 = xg.shape
    if H4 % 4 or hg.shape != xg.shape or (c_prev is not None and tuple(c_prev.shape) != (Bd, H4 // 4)):
        raise DynError(f"lstm_cell: xg {tuple(xg.shape)}, hg {tuple(hg.shape)}, c_prev {None if c_prev is None else tuple(c_prev.shape)}")
    Hd = H4 // 4
    if out is None:
        c = torch.empty(Bd, Hd, device=xg.device, dtype=F32)
        h = torch.empty(Bd, Hd, device=xg.device, dtype=F32)
        gates = torch.empty(Bd, H4, device=xg.device, dtype=F32) if save else None
    else:
        c, h, gates = out
        _cc(c, "lstm_cell.c"); _cc(h, "lstm_cell.h")
        if tuple(c.shape) != (Bd, Hd) or tuple(h.shape) != (Bd, Hd) or (gates is not None and tuple(gates.shape) != (Bd, H4)):
            raise DynError("lstm_cell: out shapes do not fit")
    check(_L().dyn_lstm_cell_fwd(xg.data_ptr(), hg.data_ptr(), _opt(c_prev, "lstm_cell.c_prev"), c.data_ptr(), h.data_ptr(),
                                 _opt(gates, "lstm_cell.gates"), Bd, Hd, _stream()), "dyn_lstm_cell_fwd")
    return c, h, gates


def lstm_cell_bwd(dh, dc_next, gates, c_prev, c, dgates=None):
    """-> (dgates [Bd, 4 Hd] pre-activation gradients, dc_prev [Bd, Hd]); dc_next / c_prev None = zeros."""
    _cc(dh, "lstm_cell_bwd.dh"); _cc(gates, "lstm_cell_bwd.gates"); _cc(c, "lstm_cell_bwd.c")
    Bd, Hd = c.shape
    if tuple(gates.shape) != (Bd, 4 * Hd) or dh.shape != c.shape:
        raise DynError(f"lstm_cell_bwd: dh {tuple(dh.shape)}, gates {tuple(gates.shape)}, c {tuple(c.shape)}")
    dgates = torch.empty_like(gates) if dgates is None else _cc(dgates, "lstm_cell_bwd.dgates")
    if tuple(dgates.shape) != (Bd, 4 * Hd):
        raise DynError(f"lstm_cell_bwd: dgates {tuple(dgates.shape)}")
    dc_prev = torch.empty_like(c)
    check(_L().dyn_lstm_cell_bwd(dh.data_ptr(), _opt(dc_next, "lstm_cell_bwd.dc_next"), gates.data_ptr(), _opt(c_prev, "lstm_cell_bwd.c_prev"),
                                 c.data_ptr(), dgates.data_ptr(), dc_prev.data_ptr(), Bd, Hd, _stream()), "dyn_lstm_cell_bwd")
    return dgates, dc_prev


def _joint_p(p, B, Hd, what):
    """p [Bp, U1, Hd] (Bp = B, or 1: shared) as any view whose last axis is contiguous -> (shared, stride_b, stride_u)."""
    _chk(p, what + ".p")
    if p.dim() != 3 or p.shape[2] != Hd or p.shape[0] not in (1, B) or p.stride(2) != 1 or p.data_ptr() % 16:
        raise DynError(f"{what}: p {tuple(p.shape)} must be [{B} or 1, U + 1, {Hd}] with a contiguous, 16-byte aligned last axis")
    shared = p.shape[0] == 1 and B > 1
    return shared, 0 if p.shape[0] == 1 else p.stride(0), p.stride(1)


def joint(e, p, act="relu", out=None):
    """z [B, T, U1, Hd] = act(e[b, t] + p[b, u]); e [B, T, Hd], p [B or 1, U1, Hd] (one row set shared by the batch); `out`: z to write."""
    a = _joint_act(act, "joint")
    _cc(e, "joint.e")
    B, T, Hd = e.shape
    _, sb, su = _joint_p(p, B, Hd, "joint")
    U1 = p.shape[1]
    z = torch.empty(B, T, U1, Hd, device=e.device, dtype=F32) if out is None else _cc(out, "joint.out")
    if tuple(z.shape) != (B, T, U1, Hd):
        raise DynError(f"joint: out {tuple(z.shape)} must be {(B, T, U1, Hd)}")
    check(_L().dyn_joint_fwd(e.data_ptr(), p.data_ptr(), z.data_ptr(), B, T, U1, Hd, sb, su, a, _stream()), "dyn_joint_fwd")
    return z


def joint_bwd(dz, z, dp_like, act="relu", want_de=True, want_dp=True, time_major=False):
    """(de [B, T, Hd] or None, dp in the shape of `dp_like` ([B or 1, U1, Hd]: 1 sums over the batch too) or None); `time_major`: dp is
    written as [U1, B or 1, Hd] (the layout the LSTM backward walks)."""
    a = _joint_act(act, "joint_bwd")
    _cc(dz, "joint_bwd.dz"); _cc(z, "joint_bwd.z")
    B, T, U1, Hd = z.shape
    if dz.shape != z.shape or tuple(dp_like.shape[1:]) != (U1, Hd) or dp_like.shape[0] not in (1, B):
        raise DynError(f"joint_bwd: dz {tuple(dz.shape)}, z {tuple(z.shape)}, p {tuple(dp_like.shape)}")
    shared = dp_like.shape[0] == 1 and B > 1
    de = torch.empty(B, T, Hd, device=z.device, dtype=F32) if want_de else None
    Bp = dp_like.shape[0]
    dp = torch.empty((U1, Bp, Hd) if time_major else (Bp, U1, Hd), device=z.device, dtype=F32) if want_dp else None
    sb, su = (Hd, Bp * Hd) if time_major else (U1 * Hd, Hd)
    check(_L().dyn_joint_bwd(dz.data_ptr(), z.data_ptr(), 0 if de is None else de.data_ptr(), 0 if dp is None else dp.data_ptr(), B, T, U1, Hd,
                             int(shared), sb, su, a, _stream()), "dyn_joint_bwd")
    return de, dp


# One private function per pass for both transducer heads, behind the public tdt_* / rnnt_* names.  `durations` None: a plain RNN-T head,
# whose C entries take neither the duration list nor sigma.  `who` is the public name: it opens every message and names the C entry
# (dyn_<who>).
def _transducer_args(who, logits, targets, target_lengths, blank, durations, T=1, state=None):
    """Checks what every pass checks -> _durations_arg(durations)."""
    _c(logits, who + ".logits"); _c(targets, who + ".targets", I32); _cc(target_lengths, who + ".target_lengths", I32)
    if state is not None:
        _cc(state, who + ".state", torch.uint8)
    dur, D = _durations_arg(durations)
    if logits.dim() != 4 or logits.shape[3] <= D:
        raise DynError(f"{who}: logits {tuple(logits.shape)} must be [B, T, U + 1, V + 1 + {D}] ({D} duration columns)")
    B = logits.shape[0]
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < 1 or target_lengths.numel() != B or int(T) < 1:
        raise DynError(f"{who}: targets {tuple(targets.shape)} must be [B, S >= 1], the lengths [B], T positive")
    if not 0 <= int(blank) < logits.shape[3] - D:
        raise DynError(f"{who}: blank={blank} lies outside the {logits.shape[3] - D} classes")
    return dur, D


def _transducer_reduction(who, reduction):
    if reduction not in TDT_REDUCTIONS:
        raise DynError(f"{who}: reduction={reduction!r} is not one of {sorted(TDT_REDUCTIONS)}")
    return TDT_REDUCTIONS[reduction]


def _transducer_budget(durations, budget):
    if budget is not None:
        return int(budget)
    return RNNT_WORKSPACE_BUDGET if durations is None else TDT_WORKSPACE_BUDGET


def _transducer_loss(who, logits, targets, logit_lengths, target_lengths, blank, durations, sigma, reduction, grad_scale, want_grad, out, budget):
    dur, D = _transducer_args(who, logits, targets, target_lengths, blank, durations)
    _cc(logit_lengths, who + ".logit_lengths", I32)
    red = _transducer_reduction(who, reduction)
    B, T, U1, N = logits.shape
    if logit_lengths.numel() != B:
        raise DynError(f"{who}: the lengths must be [{B}]")
    loss = torch.empty(1, device=logits.device, dtype=F32)
    nll = torch.empty(B, device=logits.device, dtype=F32)
    grad = None
    if want_grad:
        grad = torch.empty_like(logits) if out is None else _c(out, who + ".out")
        if grad.shape != logits.shape:
            raise DynError(f"{who}: out {tuple(grad.shape)} != logits {tuple(logits.shape)}")
    ws = workspace(logits.device)
    check(getattr(_L(), "dyn_" + who)(logits.data_ptr(), B, T, U1, N - D, *dur, targets.data_ptr(), targets.shape[1], logit_lengths.data_ptr(),
                                      target_lengths.data_ptr(), int(blank), *((sigma,) if dur else ()), red, grad_scale, loss.data_ptr(),
                                      nll.data_ptr(), 0 if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _transducer_budget(durations, budget), _stream()), "dyn_" + who)
    return loss, nll, grad


def _transducer_state(who, B, T, U1, durations, device, budget):
    if durations is None:
        need = _L().dyn_rnnt_loss_workspace_bytes(B, T, U1)
    else:
        need = _L().dyn_tdt_loss_workspace_bytes(B, T, U1, len(check_durations(durations)))
    budget = _transducer_budget(durations, budget)
    if need < 0:
        raise DynError(f"{who}: bad lattice [{B}, {T}, {U1}]")
    if 0 < budget < need:
        raise DynError(f"{who}: the lattice of [{B}, {T}, {U1}] needs {need} bytes of state, over the workspace budget of {budget} "
                       "(chunking the lattice state is not built: only the joint streams over frame chunks)")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _transducer_arcs_chunk(who, logits, t0, T, targets, target_lengths, blank, durations, state, sigma, budget):
    dur, D = _transducer_args(who, logits, targets, target_lengths, blank, durations, T, state)
    B, Tc, U1, N = logits.shape
    check(getattr(_L(), "dyn_" + who)(logits.data_ptr(), B, int(T), U1, N - D, *dur, targets.data_ptr(), targets.shape[1],
                                      target_lengths.data_ptr(), int(blank), *((sigma,) if dur else ()), int(t0), Tc, state.data_ptr(),
                                      state.numel(), _transducer_budget(durations, budget), _stream()), "dyn_" + who)


def _transducer_lattice_run(who, B, T, U1, S, logit_lengths, target_lengths, durations, state, reduction, want_beta, budget):
    _cc(logit_lengths, who + ".logit_lengths", I32); _cc(target_lengths, who + ".target_lengths", I32)
    _cc(state, who + ".state", torch.uint8)
    red = _transducer_reduction(who, reduction)
    if logit_lengths.numel() != B or target_lengths.numel() != B:
        raise DynError(f"{who}: the lengths must be [{B}]")
    dur, _ = _durations_arg(durations)
    loss = torch.empty(1, device=state.device, dtype=F32)
    nll = torch.empty(B, device=state.device, dtype=F32)
    check(getattr(_L(), "dyn_" + who)(B, T, U1, *dur, int(S), logit_lengths.data_ptr(), target_lengths.data_ptr(), red, loss.data_ptr(),
                                      nll.data_ptr(), int(bool(want_beta)), state.data_ptr(), state.numel(),
                                      _transducer_budget(durations, budget), _stream()), "dyn_" + who)
    return loss, nll


def _transducer_grad_chunk(who, logits, t0, T, targets, logit_lengths, target_lengths, blank, durations, state, reduction, grad_scale, out):
    dur, D = _transducer_args(who, logits, targets, target_lengths, blank, durations, T, state)
    _cc(logit_lengths, who + ".logit_lengths", I32)
    red = _transducer_reduction(who, reduction)
    B, Tc, U1, N = logits.shape
    grad = torch.empty_like(logits) if out is None else _c(out, who + ".out")
    if grad.shape != logits.shape or logit_lengths.numel() != B:
        raise DynError(f"{who}: out {tuple(grad.shape)} != logits {tuple(logits.shape)}, or the lengths are not [{B}]")
    check(getattr(_L(), "dyn_" + who)(logits.data_ptr(), B, int(T), U1, N - D, *dur, targets.data_ptr(), targets.shape[1], logit_lengths.data_ptr(),
                                      target_lengths.data_ptr(), int(blank), red, grad_scale, int(t0), Tc, grad.data_ptr(), state.data_ptr(),
                                      state.numel(), _stream()), "dyn_" + who)
    return grad


def _transducer_lattice(B, T, U1, D, device, state):
    """(alpha, beta, lp [B, T, U1, 2 + D], lse [B, T, U1, 2]; D = 0, no duration head: lse [B, T, U1]) of the workspace or of `state`.  The
    kernels store every anti-diagonal relative to an integer base; the bases are added back here in float64 (host arithmetic, for tests)."""
    off = (ctypes.c_int64 * 8)()
    if D:
        check(_L().dyn_tdt_loss_workspace_layout(B, T, U1, D, ctypes.cast(off, ctypes.c_void_p)), "dyn_tdt_loss_workspace_layout")
    else:
        check(_L().dyn_rnnt_loss_workspace_layout(B, T, U1, ctypes.cast(off, ctypes.c_void_p)), "dyn_rnnt_loss_workspace_layout")
    ws = workspace(device) if state is None else state
    cells = B * T * U1

    def view(i, n, shape):
        return ws[off[i]:off[i] + 4 * n].view(F32).view(shape)

    diag = (torch.arange(T, device=ws.device)[:, None] + torch.arange(U1, device=ws.device)[None, :]).expand(B, T, U1).reshape(B, -1)
    alpha = view(2, cells, (B, T, U1)).double() + view(4, B * (T + U1), (B, T + U1)).double().gather(1, diag).view(B, T, U1)
    beta = view(3, cells, (B, T, U1)).double() + view(5, B * (T + U1), (B, T + U1)).double().gather(1, diag).view(B, T, U1)
    lse = view(1, cells * 2, (B, T, U1, 2)) if D else view(1, cells, (B, T, U1))
    return alpha, beta, view(0, cells * (2 + D), (B, T, U1, 2 + D)), lse


def _transducer_greedy_steps(who, enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank, durations, max_symbols, max_steps,
                             n_steps, chunk=()):
    """`durations` None: an RNN-T decode (RnntGreedyState, max_symbols per frame; `chunk` = (frame_base, rebase) of the chunk entry)."""
    _cc(enc, who + ".enc"); _cc(valid, who + ".valid", I32); _cc(embed, who + ".embed"); _cc(lstm_ptrs, who + ".lstm_ptrs", torch.int64)
    for t, n in ((proj_w, "proj_w"), (proj_b, "proj_b"), (head_w, "head_w"), (head_b, "head_b")):
        _cc(t, f"{who}.{n}")
    dur, D = _durations_arg(durations)
    rows, head = (6, ()) if dur else (7, (int(max_symbols),))
    B, T, Hd = enc.shape
    layers = state.h.shape[0]
    N = head_w.shape[0]
    V1 = N - D
    if (tuple(state.h.shape) != (layers, B, Hd) or lstm_ptrs.numel() != 4 * layers or embed.shape != (V1, Hd) or head_w.shape[1] != Hd
            or tuple(proj_w.shape) != (Hd, Hd) or tuple(state.logits.shape) != (B, N) or tuple(state.istate.shape) != (rows, B)
            or valid.numel() != B or head_b.numel() != N or not 0 <= blank < V1 or (head and head[0] < 1)):
        raise DynError(f"{who}: shapes of the state ({'Rnnt' if rows == 7 else 'Tdt'}GreedyState), the weights and enc do not fit together")
    check(getattr(_L(), "dyn_" + who)(enc.data_ptr(), valid.data_ptr(), embed.data_ptr(), lstm_ptrs.data_ptr(), proj_w.data_ptr(), proj_b.data_ptr(),
                                      head_w.data_ptr(), head_b.data_ptr(), state.istate.data_ptr(), state.h.data_ptr(), state.c.data_ptr(),
                                      state.h_new.data_ptr(), state.dec.data_ptr(), state.logits.data_ptr(), state.tokens.data_ptr(),
                                      state.frames.data_ptr(), B, T, Hd, layers, V1, *dur, int(blank), *head, state.n_max, int(max_steps),
                                      int(n_steps), *chunk, _stream()), "dyn_" + who)


def tdt_loss(logits, targets, logit_lengths, target_lengths, blank, durations, sigma=0.0, reduction="mean", grad_scale=1.0, want_grad=True,
             out=None, budget=None):
    """logits [B, T, U1, V1 + D] contiguous; targets int32 [B, S >= 1]; lengths int32 [B] (all on the device); `durations` a host list.
    Returns (loss [1], nll [B], grad [B, T, U1, V1 + D] of grad_scale * loss or None) with transformers' tdt_loss semantics
    (reduction "none": loss is the sum, the rows are nll).  `out` may be logits (the gradient written over them)."""
    return _transducer_loss("tdt_loss", logits, targets, logit_lengths, target_lengths, blank, check_durations(durations), sigma, reduction, grad_scale, want_grad,
                            out, budget)


def joint_bwd_chunk(dz, z, de, dp, t0, accumulate, act="relu", time_major=False):
    """joint_bwd of the frames [t0, t0 + Tc): dz, z [B, Tc, U1, Hd].  de [B, T, Hd] (or None) receives its rows [:, t0:t0 + Tc], the same
    bits as joint_bwd's; dp [B or 1, U1, Hd] (`time_major`: [U1, B or 1, Hd]; or None) the chunk's sum over its frames, written
    (`accumulate` false) or added to what it holds: chunks in ascending order give one fixed summation order."""
    a = _joint_act(act, "joint_bwd_chunk")
    _cc(dz, "joint_bwd_chunk.dz"); _cc(z, "joint_bwd_chunk.z")
    if z.dim() != 4 or dz.shape != z.shape or (de is None and dp is None):
        raise DynError(f"joint_bwd_chunk: dz {tuple(dz.shape)}, z {tuple(z.shape)} must be [B, Tc, U + 1, Hd], with de or dp to write")
    B, Tc, U1, Hd = z.shape
    t0 = int(t0)
    de_ptr = sde = 0
    if de is not None:
        _cc(de, "joint_bwd_chunk.de")
        if de.dim() != 3 or de.shape[0] != B or de.shape[2] != Hd or not 0 <= t0 <= de.shape[1] - Tc:
            raise DynError(f"joint_bwd_chunk: de {tuple(de.shape)} must be [{B}, T, {Hd}] with the frames [{t0}, {t0 + Tc}) inside T")
        de_ptr, sde = de.data_ptr() + 4 * t0 * Hd, de.shape[1] * Hd
    dp_ptr, shared, sb, su = 0, False, 0, Hd
    if dp is not None:
        _cc(dp, "joint_bwd_chunk.dp")
        Bp = dp.shape[1] if time_major and dp.dim() == 3 else dp.shape[0]
        if tuple(dp.shape) != ((U1, Bp, Hd) if time_major else (Bp, U1, Hd)) or Bp not in (1, B):
            raise DynError(f"joint_bwd_chunk: dp {tuple(dp.shape)} does not fit z {tuple(z.shape)}")
        shared = Bp == 1 and B > 1
        sb, su = (Hd, Bp * Hd) if time_major else (U1 * Hd, Hd)
        dp_ptr = dp.data_ptr()
    check(_L().dyn_joint_bwd_chunk(dz.data_ptr(), z.data_ptr(), de_ptr, dp_ptr, B, Tc, U1, Hd, int(shared), sde, sb, su, int(bool(accumulate)),
                                   a, _stream()), "dyn_joint_bwd_chunk")
    return de, dp


def tdt_state(B, T, U1, durations, device, budget=None):
    """A caller-owned lattice state for tdt_arcs_chunk / tdt_lattice_run / tdt_grad_chunk (uint8, dyn_tdt_loss_workspace_layout's
    layout; tdt_lattice(state=) reads it back).  Over `budget` (default TDT_WORKSPACE_BUDGET) it is refused by name before anything
    is allocated: the joint streams over frame chunks, the lattice state does not."""
    return _transducer_state("tdt_state", B, T, U1, check_durations(durations), device, budget)


def tdt_arcs_chunk(logits, t0, T, targets, target_lengths, blank, durations, state, sigma=0.0, budget=None):
    """The arcs pass of tdt_loss on the frames [t0, t0 + Tc) of a lattice of T frames: logits [B, Tc, U1, V1 + D] (a chunk may overhang T,
    those rows are not read) -> lp and lse of those cells in `state` (tdt_state).  Every frame has to be covered before tdt_lattice_run."""
    _transducer_arcs_chunk("tdt_arcs_chunk", logits, t0, T, targets, target_lengths, blank, check_durations(durations), state, sigma,
                           budget)


def tdt_lattice_run(B, T, U1, S, logit_lengths, target_lengths, durations, state, reduction="mean", want_beta=True, budget=None):
    """The lattice and the reduction of tdt_loss on a state the arcs pass filled -> (loss [1], nll [B]); beta (the gradient pass needs
    it) only with want_beta.  S = the width of the targets tensor the arcs pass saw (it caps the target lengths)."""
    return _transducer_lattice_run("tdt_lattice_run", B, T, U1, S, logit_lengths, target_lengths, check_durations(durations), state, reduction,
                                   want_beta, budget)


def tdt_grad_chunk(logits, t0, T, targets, logit_lengths, target_lengths, blank, durations, state, reduction="mean", grad_scale=1.0, out=None):
    """The gradient pass of tdt_loss on the frames [t0, t0 + Tc): the gradient of grad_scale * loss w.r.t. the chunk's logits
    [B, Tc, U1, V1 + D], from a state tdt_lattice_run(want_beta=True) completed.  `out` may be the logits; rows past T are zeros."""
    return _transducer_grad_chunk("tdt_grad_chunk", logits, t0, T, targets, logit_lengths, target_lengths, blank, check_durations(durations), state,
                                  reduction, grad_scale, out)


def tdt_lattice(B, T, U1, D, device, state=None):
    """What the last ops.tdt_loss call of this (device, stream) left in the workspace (or what the chunk entries left in `state`), as
    absolute values: (alpha [B, T, U1],
    beta [B, T, U1] (written only when a gradient was asked for), lp [B, T, U1, 2 + D], lse [B, T, U1, 2]).  The kernels store every
    anti-diagonal relative to an integer base; the bases are added back here in float64 (host arithmetic, for tests)."""
    if int(D) < 1:
        raise DynError(f"tdt_lattice: D={D} durations (a head without durations: rnnt_lattice)")
    return _transducer_lattice(B, T, U1, int(D), device, state)


class TdtGreedyState:
    """Device state of a greedy TDT decode (dyn_tdt_greedy_steps): istate [6, B] = frame pointer, last token, emit flag, done flag, output
    count, steps taken; the LSTM's h / c per layer, the cached projector output, the step's logits and the outputs."""

    def __init__(self, B, Hd, layers, N, n_max, start_token, device):
        z = lambda *s, dt=F32: torch.zeros(*s, device=device, dtype=dt)           # noqa: E731
        self.istate = z(6, B, dt=I32)
        self.istate[1] = int(start_token)
        self.istate[2] = 1                       # the first step primes the prediction network on the start token
        self.h, self.c, self.h_new = z(layers, B, Hd), z(layers, B, Hd), z(layers, B, Hd)
        self.dec, self.logits = z(B, Hd), z(B, N)
        self.tokens, self.frames = z(B, n_max, dt=I32), z(B, n_max, dt=I32)
        self.n_max = int(n_max)


def tdt_greedy_steps(enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, durations, blank, max_steps, n_steps):
    """n_steps greedy steps of every live row, queued from one call.  enc [B, T, Hd]; valid int32 [B]; lstm_ptrs int64 DEVICE tensor
    [4 * layers] of data pointers (w_ih, w_hh, b_ih, b_hh per layer); head_w [V1 + D, Hd]."""
    _transducer_greedy_steps("tdt_greedy_steps", enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank,
                             check_durations(durations), None, max_steps, n_steps)


# ----------------------------------------------------------------------------------------------- RNN-T (ParakeetForRNNT; csrc/transducer.hip)
RNNT_WORKSPACE_BUDGET = TDT_WORKSPACE_BUDGET      # bytes of lattice state (20 B per cell) an RNN-T loss may ask for; the state is never chunked


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, reduction="mean_volume", grad_scale=1.0, want_grad=True, out=None,
              budget=None):
    """logits [B, T, U1, V1] contiguous; targets int32 [B, S >= 1]; lengths int32 [B] (all on the device).
    Returns (loss [1], nll [B], grad [B, T, U1, V1] of grad_scale * loss or None) with transformers' rnnt_loss semantics: its five
    reductions under ops.TDT_REDUCTIONS' codes, default "mean_volume" (reduction "none": loss is the sum, the rows are nll).  `out` may
    be logits (the gradient written over them)."""
    return _transducer_loss("rnnt_loss", logits, targets, logit_lengths, target_lengths, blank, None, 0.0, reduction, grad_scale, want_grad, out,
                            budget)


def rnnt_state(B, T, U1, device, budget=None):
    """A caller-owned lattice state for rnnt_arcs_chunk / rnnt_lattice_run / rnnt_grad_chunk (uint8, dyn_rnnt_loss_workspace_layout's
    layout; rnnt_lattice(state=) reads it back).  Over `budget` (default RNNT_WORKSPACE_BUDGET) it is refused by name before anything
    is allocated: the joint streams over frame chunks, the lattice state does not."""
    return _transducer_state("rnnt_state", B, T, U1, None, device, budget)


def rnnt_arcs_chunk(logits, t0, T, targets, target_lengths, blank, state, budget=None):
    """The arcs pass of rnnt_loss on the frames [t0, t0 + Tc) of a lattice of T frames: logits [B, Tc, U1, V1] (a chunk may overhang T,
    those rows are not read) -> lp and lse of those cells in `state` (rnnt_state).  Every frame has to be covered before rnnt_lattice_run."""
    _transducer_arcs_chunk("rnnt_arcs_chunk", logits, t0, T, targets, target_lengths, blank, None, state, 0.0, budget)


def rnnt_lattice_run(B, T, U1, S, logit_lengths, target_lengths, state, reduction="mean_volume", want_beta=True, budget=None):
    """The lattice and the reduction of rnnt_loss on a state the arcs pass filled -> (loss [1], nll [B]); beta (the gradient pass needs
    it) only with want_beta.  S = the width of the targets tensor the arcs pass saw (it caps the target lengths)."""
    return _transducer_lattice_run("rnnt_lattice_run", B, T, U1, S, logit_lengths, target_lengths, None, state, reduction, want_beta, budget)


def rnnt_grad_chunk(logits, t0, T, targets, logit_lengths, target_lengths, blank, state, reduction="mean_volume", grad_scale=1.0, out=None):
    """The gradient pass of rnnt_loss on the frames [t0, t0 + Tc): the gradient of grad_scale * loss w.r.t. the chunk's logits
    [B, Tc, U1, V1], from a state rnnt_lattice_run(want_beta=True) completed.  `out` may be the logits; rows past T are zeros."""
    return _transducer_grad_chunk("rnnt_grad_chunk", logits, t0, T, targets, logit_lengths, target_lengths, blank, None, state, reduction,
                                  grad_scale, out)


def rnnt_lattice(B, T, U1, device, state=None):
    """What the last ops.rnnt_loss call of this (device, stream) left in the workspace (or what the chunk entries left in `state`), as
    absolute values: (alpha [B, T, U1], beta [B, T, U1] (written only when a gradient was asked for), lp [B, T, U1, 2], lse [B, T, U1]).
    The integer bases of the anti-diagonals are added back here in float64 (host arithmetic, for tests)."""
    return _transducer_lattice(B, T, U1, 0, device, state)


class RnntGreedyState(TdtGreedyState):
    """Device state of a greedy RNN-T decode (dyn_rnnt_greedy_steps): TdtGreedyState with one more int32 row of istate ([7, B]), the
    symbols emitted at the current frame; the logits row is [B, V1]."""

    def __init__(self, B, Hd, layers, V1, n_max, start_token, device):
        super().__init__(B, Hd, layers, V1, n_max, start_token, device)
        first = self.istate
        self.istate = torch.zeros(7, B, device=device, dtype=I32)
        self.istate[:6] = first


def rnnt_greedy_steps(enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank, max_symbols, max_steps, n_steps):
    """n_steps greedy RNN-T steps of every live row, queued from one call.  enc [B, T, Hd]; valid int32 [B]; lstm_ptrs int64 DEVICE tensor
    [4 * layers] of data pointers (w_ih, w_hh, b_ih, b_hh per layer); head_w [V1, Hd]; `max_symbols`: max_symbols_per_step."""
    _transducer_greedy_steps("rnnt_greedy_steps", enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank, None, max_symbols,
                             max_steps, n_steps)


# ----------------------------------------------------------------------------------------------- NemotronAsrStreamingForRNNT
def chunked_band(T, left_context, lookahead):
    """Pure host function: the geometry of transformers' chunked_limited_mask_function(left_context, lookahead) over T frames.
    cs = lookahead + 1 frames per chunk, lc = left_context // cs left chunks (-1: unlimited, left_context < 0); query i sees the keys
    [max(0, i // cs - lc) * cs, min(T, (i // cs + 1) * cs)).  j - i then lies in [-dlo, dhi]: W = dlo + dhi + 1 relative positions,
    the rows r0 .. r0 + W of the [2T - 1, H] position table (row T - 1 is distance 0), lc * cs + 2 cs - 1 of them once T - 1 reaches
    both ends.  Returns SimpleNamespace(cs, lc, dlo, dhi, W, r0)."""
    from types import SimpleNamespace
    for name, v in (("T", T), ("left_context", left_context), ("lookahead", lookahead)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise DynError(f"chunked_band: {name}={v!r} must be an integer")
    if T < 1 or lookahead < 0:
        raise DynError(f"chunked_band: T={T} must be positive and lookahead={lookahead} must not be negative")
    cs = lookahead + 1
    lc = left_context // cs if left_context >= 0 else -1
    dlo = T - 1 if lc < 0 else min(lc * cs + cs - 1, T - 1)
    dhi = min(cs - 1, T - 1)
    return SimpleNamespace(cs=cs, lc=lc, dlo=dlo, dhi=dhi, W=dlo + dhi + 1, r0=T - 1 - dlo)


def _band_dims(who, S, BD, band):
    if S.dim() != 4 or S.shape[2] != S.shape[3]:
        raise DynError(f"{who}: scores must be [B, heads, T, T], got {tuple(S.shape)}")
    M, T = S.shape[0] * S.shape[1], S.shape[-1]
    if BD is not None and (BD.dim() != 4 or tuple(BD.shape[:3]) != tuple(S.shape[:3]) or BD.shape[3] < band.W):
        raise DynError(f"{who}: the band buffer must be [B, heads, T, ld >= {band.W}], got {tuple(BD.shape)}")
    return M, T


def softmax_relshift_band(S, BD, band, out=None):
    """softmax over the keys the chunked mask leaves row i of S [B, nh, T, T] + BD[b, h, i, j - i + band.dlo] (BD [B, nh, T, ld >= band.W]:
    the band product, both scaled already), exact zeros in every other column.  `band`: chunked_band(T, ...).  `out` may be S."""
    _cc(S, "softmax_relshift_band.S"); _c(BD, "softmax_relshift_band.BD")
    M, T = _band_dims("softmax_relshift_band", S, BD, band)
    out = torch.empty_like(S) if out is None else _cc(out, "softmax_relshift_band.out")
    check(_L().dyn_softmax_relshift_band_fwd(S.data_ptr(), out.data_ptr(), BD.data_ptr(), M, T, BD.shape[3], band.cs, band.lc, _stream()),
          "dyn_softmax_relshift_band_fwd")
    return out


def relshift_band_bwd(dS, band, out=None, ld_bd=None):
    """dBD [B, nh, T, ld_bd (band.W)] from dS [B, nh, T, T]: dS of every row's key range in the band's columns, zeros written everywhere
    else (`out` may be stale scratch)."""
    _cc(dS, "relshift_band_bwd.dS")
    ld = band.W if ld_bd is None else int(ld_bd)
    if out is None:
        out = torch.empty(*dS.shape[:3], ld, device=dS.device, dtype=F32)
    M, T = _band_dims("relshift_band_bwd", dS, _c(out, "relshift_band_bwd.out"), band)
    check(_L().dyn_relshift_band_bwd(dS.data_ptr(), out.data_ptr(), M, T, out.shape[3], band.cs, band.lc, _stream()), "dyn_relshift_band_bwd")
    return out


def causal_out_len(n):
    """Output length of a 3-wide, stride-2 convolution padded (2, 1): NemotronAsrStreamingEncoderCausalConv2D."""
    return n // 2 + 1


def conv2d_first_causal(x, w, bias):
    """x [B, T, F] -> z [B, T // 2 + 1, F // 2 + 1, C], the causal stem (padding (2, 1) on both axes); w [C, 3, 3]."""
    _c(x, "conv2d_first_causal.x"); _cc(w, "conv2d_first_causal.w"); _cc(bias, "conv2d_first_causal.bias")
    B, T, F = x.shape
    C = w.shape[0]
    out = torch.empty(B, causal_out_len(T), causal_out_len(F), C, device=x.device, dtype=F32)
    check(_L().dyn_conv2d_first_causal_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, _stream()),
          "dyn_conv2d_first_causal_fwd")
    return out


def conv2d_first_causal_wgrad(x, dz, dw, dbias, beta=1.0):
    _c(x, "conv2d_first_causal_wgrad.x"); _cc(dz, "conv2d_first_causal_wgrad.dz"); _cc(dw, "conv2d_first_causal_wgrad.dw")
    _cc(dbias, "conv2d_first_causal_wgrad.dbias")
    B, T, F = x.shape
    C = dw.shape[0]
    if tuple(dz.shape) != (B, causal_out_len(T), causal_out_len(F), C):
        raise DynError("conv2d_first_causal_wgrad: dz must be [B, T // 2 + 1, F // 2 + 1, C]")
    ws = workspace(x.device)
    check(_L().dyn_conv2d_first_causal_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C, ws.data_ptr(),
                                             ws.numel(), _stream()), "dyn_conv2d_first_causal_wgrad")


def dwconv2d_s2_causal_act(z, w, bias, act):
    """u = bias + causal dw3x3_s2(act(z)), act "relu"; z [B, T, F, C] -> [B, T // 2 + 1, F // 2 + 1, C]; w [C, 3, 3]."""
    a = _sub_act(act, "dwconv2d_s2_causal_act")
    _cc(z, "dwconv2d_s2_causal_act.z"); _cc(w, "dwconv2d_s2_causal_act.w"); _cc(bias, "dwconv2d_s2_causal_act.bias")
    B, T, F, C = z.shape
    out = torch.empty(B, causal_out_len(T), causal_out_len(F), C, device=z.device, dtype=F32)
    check(_L().dyn_dwconv2d_s2_causal_fwd_act(z.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, C, a, _stream()),
          "dyn_dwconv2d_s2_causal_fwd_act")
    return out


def dwconv2d_s2_causal_dgrad_act(z, w, du, act):
    a = _sub_act(act, "dwconv2d_s2_causal_dgrad_act")
    _cc(z, "dwconv2d_s2_causal_dgrad_act.z"); _cc(du, "dwconv2d_s2_causal_dgrad_act.du"); _cc(w, "dwconv2d_s2_causal_dgrad_act.w")
    B, T, F, C = z.shape
    if tuple(du.shape) != (B, causal_out_len(T), causal_out_len(F), C):
        raise DynError("dwconv2d_s2_causal_dgrad_act: du must be [B, T // 2 + 1, F // 2 + 1, C]")
    out = torch.empty_like(z)
    check(_L().dyn_dwconv2d_s2_causal_dgrad_act(z.data_ptr(), w.data_ptr(), du.data_ptr(), out.data_ptr(), B, T, F, C, a, _stream()),
          "dyn_dwconv2d_s2_causal_dgrad_act")
    return out


def dwconv2d_s2_causal_wgrad_act(z, du, dw, dbias, act, beta=1.0):
    a = _sub_act(act, "dwconv2d_s2_causal_wgrad_act")
    _cc(z, "dwconv2d_s2_causal_wgrad_act.z"); _cc(du, "dwconv2d_s2_causal_wgrad_act.du"); _cc(dw, "dwconv2d_s2_causal_wgrad_act.dw")
    _cc(dbias, "dwconv2d_s2_causal_wgrad_act.dbias")
    B, T, F, C = z.shape
    if tuple(du.shape) != (B, causal_out_len(T), causal_out_len(F), C):
        raise DynError("dwconv2d_s2_causal_wgrad_act: du must be [B, T // 2 + 1, F // 2 + 1, C]")
    ws = workspace(z.device)
    check(_L().dyn_dwconv2d_s2_causal_wgrad_act(z.data_ptr(), du.data_ptr(), dw.data_ptr(), dbias.data_ptr(), beta, B, T, F, C, a, ws.data_ptr(),
                                                ws.numel(), _stream()), "dyn_dwconv2d_s2_causal_wgrad_act")


def convmod_causal_k9(u, w, cbias, gamma, beta, eps=1e-5, save=False):
    """NemotronAsrStreaming's conv-module core in one launch: u [B, T, 2C] -> s [B, T, C] = silu(LayerNorm_C(cbias + causal depthwise
    conv(GLU(u)))), w [C, 9], cbias [C] or None, zeros left of frame 0.  Returns (s, g, c, n, mean, rstd) as convmod_causal."""
    return _convmod_causal("convmod_causal_k9", u, w, cbias, gamma, beta, None, eps, save, lambda outs, B, T, C: _L().dyn_convmod_causal_k9_fwd(
        u.data_ptr(), w.data_ptr(), _opt(cbias, "cbias"), gamma.data_ptr(), beta.data_ptr(), *outs, B, T, C, w.shape[1], eps, _stream()))


def dwconv1d_causal_k9_dgrad(dy, w, out=None, beta=0.0):
    """dwconv1d_causal_dgrad at 9 taps."""
    return _dwconv1d_causal_dgrad("dwconv1d_causal_k9_dgrad", dy, w, out, beta)


def dwconv1d_causal_k9_wgrad(x, dy, dw, beta=1.0):
    """dwconv1d_causal_wgrad at 9 taps."""
    return _dwconv1d_causal_wgrad("dwconv1d_causal_k9_wgrad", x, dy, dw, beta)


# ----------------------------------------------------------------------------------------------- NemotronAsrStreamingForRNNT, streaming
def stream_geometry(sliding_window, lookahead):
    """Pure host function: the geometry of a cache-aware stream.  cs = lookahead + 1 encoder frames per chunk, lc = (sliding_window - 1) //
    cs visible cached chunks, the ring's lc + 1 slots, NK = (lc + 1) cs keys at most, W = NK + cs - 1 distances (lc cs + cs - 1 down to
    -(cs - 1)), and the feature frames of the first and of every later chunk (transformers' _required_stream_chunk_frames)."""
    from types import SimpleNamespace
    for name, v in (("sliding_window", sliding_window), ("lookahead", lookahead)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise DynError(f"stream_geometry: {name}={v!r} must be an integer")
    if sliding_window < 1 or lookahead < 0:
        raise DynError(f"stream_geometry: sliding_window={sliding_window} must be positive (a negative one leaves the left context, and so "
                       f"the cache, without a bound) and lookahead={lookahead} must not be negative")
    cs = lookahead + 1
    lc = (sliding_window - 1) // cs
    NK = (lc + 1) * cs
    return SimpleNamespace(cs=cs, lc=lc, slots=lc + 1, NK=NK, W=NK + cs - 1, dlo=NK - 1, first_frames=1 + 8 * lookahead, frames=8 * cs)


def stream_stage_len(n, first):
    """Output rows of a streamed 3-wide stride-2 stage on n input rows: one carried row to the left (two zero rows on the first chunk),
    nothing to the right (NemotronAsrStreamingEncoderCausalConv2D.output_length(streaming=True))."""
    return (n + (2 if first else 1) - 3) // 2 + 1


def stream_position_rows(geo, H):
    """[W, H] float32 on the host: the sinusoid rows of the distances geo.dlo .. -(geo.cs - 1), NemotronAsrStreamingEncoderRelPositionalEncoding's
    arithmetic (the rows ops.chunked_band names of a long enough offline table)."""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, H, 2, dtype=torch.float) / H))
    position_ids = torch.arange(geo.dlo, -geo.cs, -1)
    freqs = (inv_freq[None, :, None].float() @ position_ids[None, None, :].float()).transpose(1, 2)
    pe = torch.stack([freqs.sin(), freqs.cos()], dim=-1)
    return pe.reshape(*pe.shape[:-2], -1)[0].contiguous()


def _counter(counter, who):
    _c(counter, who + ".counter", I32)
    if counter.numel() < 1:
        raise DynError(f"{who}: the counter must hold one int32")
    return counter


def stream_advance(counter):
    """counter[0] += 1 on the device: the last launch of a streaming step."""
    check(_L().dyn_stream_advance(_counter(counter, "stream_advance").data_ptr(), _stream()), "dyn_stream_advance")


def stream_attn(qkv, bias_u, bias_v, pos, k_cache, v_cache, counter, nh, lc, scale=None, out=None):
    """The attention core of one layer and chunk: qkv [B, cs, 3H] -> context [B, cs, H]; pos [W, H]; k_cache / v_cache [B, lc + 1, cs, H]
    rings, the chunk's k / v stored into slot counter % (lc + 1)."""
    _cc(qkv, "stream_attn.qkv"); _cc(bias_u, "stream_attn.bias_u"); _cc(bias_v, "stream_attn.bias_v"); _cc(pos, "stream_attn.pos")
    _cc(k_cache, "stream_attn.k_cache"); _cc(v_cache, "stream_attn.v_cache"); _counter(counter, "stream_attn")
    if qkv.dim() != 3 or qkv.shape[2] % 3:
        raise DynError(f"stream_attn: qkv {tuple(qkv.shape)} must be [B, cs, 3H]")
    B, cs, H3 = qkv.shape
    H = H3 // 3
    if H % nh:
        raise DynError(f"stream_attn: H={H} is not a multiple of {nh} heads")
    W = (lc + 1) * cs + cs - 1
    if (tuple(pos.shape) != (W, H) or tuple(k_cache.shape) != (B, lc + 1, cs, H) or tuple(v_cache.shape) != (B, lc + 1, cs, H)
            or bias_u.numel() != H or bias_v.numel() != H):
        raise DynError(f"stream_attn: pos must be [{W}, {H}], the caches [{B}, {lc + 1}, {cs}, {H}], the head biases [{H}]")
    out = torch.empty(B, cs, H, device=qkv.device, dtype=F32) if out is None else _cc(out, "stream_attn.out")
    if tuple(out.shape) != (B, cs, H):
        raise DynError(f"stream_attn: out must be [{B}, {cs}, {H}]")
    D = H // nh
    check(_L().dyn_stream_attn(qkv.data_ptr(), bias_u.data_ptr(), bias_v.data_ptr(), pos.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                               counter.data_ptr(), out.data_ptr(), B, cs, lc, nh, D, D ** -0.5 if scale is None else scale, _stream()),
          "dyn_stream_attn")
    return out


def stream_convmod_k9(u, w, cbias, gamma, beta, state, counter, eps=1e-5):
    """convmod_causal_k9 on a chunk u [B, T, 2C] with the carried GLU frames state [2, B, 8, C] (half counter & 1 read, the other written)."""
    _cc(u, "stream_convmod_k9.u"); _cc(w, "stream_convmod_k9.w"); _cc(gamma, "stream_convmod_k9.gamma"); _cc(beta, "stream_convmod_k9.beta")
    _cc(state, "stream_convmod_k9.state"); _counter(counter, "stream_convmod_k9")
    B, T, C2 = u.shape
    C = C2 // 2
    if tuple(w.shape) != (C, 9) or tuple(state.shape) != (2, B, 8, C) or gamma.numel() != C or beta.numel() != C:
        raise DynError(f"stream_convmod_k9: w must be [{C}, 9], the state [2, {B}, 8, {C}], gamma and beta [{C}]")
    s = torch.empty(B, T, C, device=u.device, dtype=F32)
    check(_L().dyn_stream_convmod_k9(u.data_ptr(), w.data_ptr(), _opt(cbias, "cbias"), gamma.data_ptr(), beta.data_ptr(), state.data_ptr(),
                                     counter.data_ptr(), s.data_ptr(), B, T, C, w.shape[1], eps, _stream()), "dyn_stream_convmod_k9")
    return s


def stream_conv2d_first(x, w, bias, carry, counter, first):
    """The causal stem on a chunk x [B, T, F] -> z [B, stream_stage_len(T, first), F // 2 + 1, C]; carry [2, B, F]."""
    _c(x, "stream_conv2d_first.x"); _cc(w, "stream_conv2d_first.w"); _cc(bias, "stream_conv2d_first.bias"); _c(carry, "stream_conv2d_first.carry")
    _counter(counter, "stream_conv2d_first")
    B, T, F = x.shape
    C = w.shape[0]
    if tuple(carry.shape) != (2, B, F):
        raise DynError(f"stream_conv2d_first: the carry must be [2, {B}, {F}]")
    out = torch.empty(B, stream_stage_len(T, first), causal_out_len(F), C, device=x.device, dtype=F32)
    check(_L().dyn_stream_conv2d_first(x.data_ptr(), w.data_ptr(), bias.data_ptr(), carry.data_ptr(), counter.data_ptr(), out.data_ptr(), B, T, F,
                                       C, int(bool(first)), _stream()), "dyn_stream_conv2d_first")
    return out


def stream_dwconv2d_s2_act(z, w, bias, carry, counter, act, first):
    """The ReLU-fused causal depthwise stage on a chunk z [B, T, F, C] -> [B, stream_stage_len(T, first), F // 2 + 1, C]; carry [2, B, F, C]
    (rows before the ReLU)."""
    a = _sub_act(act, "stream_dwconv2d_s2_act")
    _cc(z, "stream_dwconv2d_s2_act.z"); _cc(w, "stream_dwconv2d_s2_act.w"); _cc(bias, "stream_dwconv2d_s2_act.bias")
    _cc(carry, "stream_dwconv2d_s2_act.carry"); _counter(counter, "stream_dwconv2d_s2_act")
    B, T, F, C = z.shape
    if tuple(carry.shape) != (2, B, F, C):
        raise DynError(f"stream_dwconv2d_s2_act: the carry must be [2, {B}, {F}, {C}]")
    out = torch.empty(B, stream_stage_len(T, first), causal_out_len(F), C, device=z.device, dtype=F32)
    check(_L().dyn_stream_dwconv2d_s2_act(z.data_ptr(), w.data_ptr(), bias.data_ptr(), carry.data_ptr(), counter.data_ptr(), out.data_ptr(), B, T,
                                          F, C, a, int(bool(first)), _stream()), "dyn_stream_dwconv2d_s2_act")
    return out


def rnnt_greedy_steps_chunk(enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank, max_symbols, max_steps, n_steps,
                            frame_base, rebase):
    """rnnt_greedy_steps on the frames enc [B, cs, Hd] of one streamed chunk; `rebase`: first move the state on to this chunk (frame pointer 0,
    done flags, per-frame counter, output and step counts cleared; h / c, the projector cache, the last token and the emit flag kept).
    Frames are recorded as frame_base + the frame inside the chunk."""
    _transducer_greedy_steps("rnnt_greedy_steps_chunk", enc, valid, embed, lstm_ptrs, proj_w, proj_b, head_w, head_b, state, blank, None,
                             max_symbols, max_steps, n_steps, chunk=(int(frame_base), int(bool(rebase))))


# ----------------------------------------------------------------------------------------------- Nemotron3_5AsrForRNNT, language-prompt fusion
def host_prompt_ids(prompt_ids, B, num_prompts, default, what="prompt_ids"):
    """Pure host function: None (`default` for every row), one int (broadcast), or an integer tensor / list [B] -> a list of B ints, every
    one inside [0, num_prompts).  A wrong length, a non-integer or an id outside the table is a DynError before any launch."""
    p = default if prompt_ids is None else prompt_ids
    if isinstance(p, bool):
        raise DynError(f"{what}={p!r} must be an integer, or an integer tensor or list [{B}]")
    if isinstance(p, int):
        ids = [p] * B
    else:
        t = torch.as_tensor(p).detach().cpu()
        if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64) or t.numel() != B:
            raise DynError(f"{what} must be one integer or an integer tensor or list [{B}], one language per row; got {tuple(t.shape)} {t.dtype}")
        ids = [int(v) for v in t.tolist()]
    if any(not 0 <= v < num_prompts for v in ids):
        raise DynError(f"{what}={ids}: every id must lie in [0, {num_prompts}) (num_prompts)")
    return ids


def _prompt_ids(ids, B, who):
    _c(ids, who + ".prompt_ids", I32)
    if ids.dim() != 1 or ids.numel() != B:
        raise DynError(f"{who}: prompt_ids must be int32 [{B}]")
    return ids


def prompt_bias_gather(b1, w1p, prompt_ids, out=None):
    """pb [B, I] = b1 [I] + the column p_b of w1p [I, Np] for every batch row: the language prompt as a per-row bias of linear_1.
    prompt_ids int32 [B] on the device, read when the kernel runs (validated by the caller: host_prompt_ids; the kernel clamps)."""
    _cc(b1, "prompt_bias_gather.b1"); _cc(w1p, "prompt_bias_gather.w1p")
    I = b1.numel()
    if w1p.dim() != 2 or w1p.shape[0] != I or I % 4:
        raise DynError(f"prompt_bias_gather: w1p {tuple(w1p.shape)} must be [I, num_prompts] with I = {I} a multiple of 4")
    B = prompt_ids.numel()
    _prompt_ids(prompt_ids, B, "prompt_bias_gather")
    out = torch.empty(B, I, device=b1.device, dtype=F32) if out is None else _cc(out, "prompt_bias_gather.out")
    if tuple(out.shape) != (B, I):
        raise DynError(f"prompt_bias_gather: out must be [{B}, {I}]")
    check(_L().dyn_prompt_bias_gather(b1.data_ptr(), w1p.data_ptr(), prompt_ids.data_ptr(), out.data_ptr(), B, I, w1p.shape[1], _stream()),
          "dyn_prompt_bias_gather")
    return out


def prompt_relu(z, pb, out=None):
    """a [B, T, I] = max(z + pb[:, None, :], 0) in one pass; out may be z."""
    _cc(z, "prompt_relu.z"); _cc(pb, "prompt_relu.pb")
    if z.dim() != 3 or tuple(pb.shape) != (z.shape[0], z.shape[2]):
        raise DynError(f"prompt_relu: z {tuple(z.shape)} must be [B, T, I] and pb {tuple(pb.shape)} [B, I]")
    out = torch.empty_like(z) if out is None else _cc(out, "prompt_relu.out")
    if out.shape != z.shape:
        raise DynError("prompt_relu: out must have z's shape")
    B, T, I = z.shape
    check(_L().dyn_prompt_relu_fwd(z.data_ptr(), pb.data_ptr(), out.data_ptr(), B, T, I, _stream()), "dyn_prompt_relu_fwd")
    return out


def prompt_relu_bwd(a, da, prompt_ids, db1, dw1p, beta=1.0, out=None):
    """Backward of prompt_relu and of the gather in one pass over (a, da) [B, T, I]: returns dz = da where a > 0, else 0 (out may be da);
    db1 [I] = beta * db1 + the column sums of dz; dw1p [I, Np] column p = beta * old + the sums of the batch rows whose prompt is p, b
    ascending (a column no row used: exactly beta * old).  db1 / dw1p None: frozen, that sum is skipped."""
    _cc(a, "prompt_relu_bwd.a"); _cc(da, "prompt_relu_bwd.da")
    if a.dim() != 3 or da.shape != a.shape:
        raise DynError(f"prompt_relu_bwd: a {tuple(a.shape)} and da {tuple(da.shape)} must both be [B, T, I]")
    B, T, I = a.shape
    out = torch.empty_like(da) if out is None else _cc(out, "prompt_relu_bwd.out")
    if out.shape != a.shape:
        raise DynError("prompt_relu_bwd: out must have a's shape")
    Np, ids_ptr, ws_ptr, ws_bytes = 1, 0, 0, 0
    if db1 is not None or dw1p is not None:
        ids_ptr = _prompt_ids(prompt_ids, B, "prompt_relu_bwd").data_ptr()
        if db1 is not None and _cc(db1, "prompt_relu_bwd.db1").numel() != I:
            raise DynError(f"prompt_relu_bwd: db1 must be [{I}]")
        if dw1p is not None:
            if _cc(dw1p, "prompt_relu_bwd.dw1p").dim() != 2 or dw1p.shape[0] != I:
                raise DynError(f"prompt_relu_bwd: dw1p {tuple(dw1p.shape)} must be [{I}, num_prompts]")
            Np = dw1p.shape[1]
        ws = workspace(a.device)
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    check(_L().dyn_prompt_relu_bwd(a.data_ptr(), da.data_ptr(), out.data_ptr(), ids_ptr, _opt(db1, "db1"), _opt(dw1p, "dw1p"), beta, B, T, I, Np,
                                   ws_ptr, ws_bytes, _stream()), "dyn_prompt_relu_bwd")
    return out
