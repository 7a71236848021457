"""The fused streaming attention (csrc/attention.hip: dyn_attention_fwd, _fwd_lse, _fwd_split with attention_merge_kernel, and the two
kernels of dyn_attention_bwd) against float64 at the tile, stride, split and score-range edges.

What was not covered before: the three attention tests of tests/test_ops_gpu.py share one input recipe (randn * 1.2 .. 1.5, scores about
N(0, 2)), at which the running-maximum rescale barely matters; their smallest T is 33; every call passes the packed layout; `delta` is never
compared; the merge kernel's stride loop never runs; no host guard is ever called.

Everything here goes through the C-ABI (`_lib.load()` / `check`), so strides and `delta` are reachable.  Tensors are [B, H, T, D] views
(kernel_refs.heads_view) of flat device buffers in the layout the entry points address.  Outputs are prefilled with NaN where the kernel
owns them and with a sentinel everywhere else; every check of a result also checks, bit for bit, that nothing outside the owned elements
changed.  lse and delta are exactly B * H * T floats between three guard elements on either side (they need no alignment).

References: tests/kernel_refs.py ("fused streaming attention"), float64 on the CPU, held to torch's softmax / logsumexp / autograd in
tests/test_kernel_refs_cpu.py.  The backward is handed the kernel's own `out` and `lse`, as in the model; its reference takes delta from
that same `out`.

Bounds: kernel_refs.measured_tol — 4 x the error of torch's own fp32 CPU evaluation of the same expression (for the gradients: fp32 autograd)
plus the floors tests/test_ops_gpu.py uses for these kernels: 2e-5 absolute for out and lse, 2e-5 * max|grad| for dQ, dK, dV; for delta
2e-5 * max(1, max|delta|).  scale = 0 is held to the floors alone.  One floor is widened, with its derivation in
kernel_refs.attention_cancellation_bound: at T = 1 the exact dQ and dK are identically 0, 2e-5 * max|grad| is 0, and what the kernel returns
is the rounding difference of its two fp32 sums dP and delta (on one MI355X run 9.3e-7 and 5.8e-7, against bounds of 5.7e-6 and 6.0e-6).
Exact routing, repeated runs and nsplit = 1 against the unsplit entry are bit-exact (torch.equal).  Every check prints `case name: kernel error | torch fp32 error | bound` before it asserts (pytest -s; the table of
one MI355X run is profiles/attention_kernels_parity.txt).  Nothing here measures speed."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

D = K.ATTN_D
SCALE = 1.0 / math.sqrt(D)
NAN = float("nan")
SENTINEL = -7.25
GUARD = 3                                # floats on either side of lse / delta
TILE_EDGES = [1, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


# ----------------------------------------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32)


def _line(case, name, err, e32, tol):
    print(f"  {case} {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")


def _measured(case, name, got, torch32, want, floor):
    """4 x torch's fp32 error + floor; the floor alone when there is no fp32 evaluation to measure (`torch32` None)."""
    tol, e32 = (floor, None) if torch32 is None else K.measured_tol(torch32, want, floor)
    err = K.max_err(got, want)
    _line(case, name, err, e32, tol)
    assert err <= tol, f"{case} {name}: err {err} > {tol} (torch fp32: {e32})"          # a NaN error fails here too


def _exact(case, name, ok):
    print(f"  {case} {name}: bit-equal {bool(ok)}")
    assert ok, f"{case} {name}: not bit-equal"


class Buf:
    """A flat fp32 device buffer holding one [B, H, T, D] tensor per entry of `offsets` (floats), rows `row` and batches `batch` floats
    apart; `tail` more floats follow the last owned one.  Filled with `outside`, the owned elements with `inside`."""

    def __init__(self, cuda, B, T, H, row, batch, offsets=(0,), outside=SENTINEL, inside=NAN, tail=0):
        size = max(offsets) + max(B - 1, 0) * batch + max(T - 1, 0) * row + H * D + tail
        self.dims, self.offsets = (B, T, H, row, batch), offsets
        self.flat = torch.full((size,), outside, device=cuda)
        self.views = [K.heads_view(self.flat, o, *self.dims) for o in offsets]
        for v in self.views:
            v.fill_(inside)
        self.ptrs = [self.flat.data_ptr() + 4 * o for o in offsets]
        self.before = None

    @property
    def ptr(self):
        return self.ptrs[0]

    def put(self, *tensors):
        for view, t in zip(self.views, tensors):
            view.copy_(t)
        return self

    def arm(self):
        """Remember the bits the buffer holds now, for contained()."""
        self.before = self.flat.clone()
        return self

    def contained(self, case, name):
        """Every float outside the owned [b, :T, h * 128 : (h + 1) * 128] still has the bits it had at arm()."""
        owned = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        for o in self.offsets:
            K.heads_view(owned, o, *self.dims).fill_(True)
        _exact(case, f"{name}: nothing written outside the owned elements", torch.equal(_bits(self.flat)[~owned], _bits(self.before)[~owned]))

    def cpu(self, i=0):
        return self.views[i].cpu()


class Stat:
    """lse or delta: exactly n floats (NaN) between GUARD sentinels on either side."""

    def __init__(self, cuda, B, H, T):
        self.shape, n = (B, H, T), B * H * T
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, device=cuda)
        self.inner = self.flat[GUARD:GUARD + n]
        self.inner.fill_(NAN)
        self.ptr = self.flat.data_ptr() + 4 * GUARD

    def contained(self, case, name):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]])
        _exact(case, f"{name}: guards on both sides", torch.equal(g, torch.full_like(g, SENTINEL)))

    def cpu(self):
        return self.inner.cpu().view(self.shape)


class Case:
    """One attention problem (q, k, v, dout: CPU fp32 [B, H, T, D]) on the device, packed (q | k | v in one [B, T, 3 HD] activation, out
    [B, T, HD], the gradients packed like the inputs) or `strided`: q, k, v in one [B, T, W = 3 HD + 8] buffer whose batches are 12 floats
    further apart, out / dout rows HD + 4 apart with a batch gap of 8, dq / dk / dv three separate buffers with rows HD + 12 apart and a batch
    gap of 4; the input padding holds NaN (none may reach a result), every buffer 128 rows of tail."""

    def __init__(self, cuda, name, q, k, v, dout, scale, strided=False, floors_only=False):
        self.cuda, self.name, self.scale, self.strided, self.floors_only = cuda, name, float(scale), strided, floors_only
        self.q, self.k, self.v, self.dout = q, k, v, dout
        B, H, T, _ = q.shape
        HD = H * D
        self.B, self.H, self.T, self.HD = B, H, T, HD
        if strided:
            self.row, self.orow, self.grow = 3 * HD + 8, HD + 4, HD + 12
            self.batch, self.obatch, self.gbatch = T * self.row + 12, T * self.orow + 8, T * self.grow + 4
        else:
            self.row, self.orow, self.grow = 3 * HD, HD, 3 * HD
            self.batch, self.obatch, self.gbatch = T * self.row, T * self.orow, T * self.grow
        self.inp = Buf(cuda, B, T, H, self.row, self.batch, (0, HD, 2 * HD), outside=NAN, tail=self._tail(self.row)).put(q, k, v)
        self._fwd = self._g32 = None

    def _tail(self, row):
        return 128 * row if self.strided else 0

    # ------------------------------------------------------------------ references, computed once per case
    def ref(self):
        if self._fwd is None:
            t32 = (None, None) if self.floors_only else K.attention_torch_fp32(self.q, self.k, self.v, self.scale)
            self._fwd = K.attention_ref(self.q, self.k, self.v, self.scale) + tuple(t32)
        return self._fwd                                            # out64, lse64, out32, lse32

    def grads32(self):
        if self._g32 is None and not self.floors_only:
            self._g32 = K.attention_torch_fp32(self.q, self.k, self.v, self.scale, self.dout)[2:]
        return self._g32 or (None, None, None)

    # ------------------------------------------------------------------ launches
    def _common(self):
        return (self.B, self.T, self.H, D, self.row, self.batch, self.orow, self.obatch, self.scale)

    def new_out(self):
        return Buf(self.cuda, self.B, self.T, self.H, self.orow, self.obatch, tail=self._tail(self.orow)).arm()

    def forward(self, entry, nsplit=1):
        """entry: "fwd" (no lse), "lse" (dyn_attention_fwd_lse) or "split" (dyn_attention_fwd_split with exactly the workspace it asks
        for, prefilled with NaN bytes).  Returns (out Buf, lse Stat or None)."""
        from dynamic_asr_eval_amd._lib import check, load
        lib = load()
        out, lse = self.new_out(), None if entry == "fwd" else Stat(self.cuda, self.B, self.H, self.T)
        qp, kp, vp = self.inp.ptrs
        if entry == "fwd":
            rc = lib.dyn_attention_fwd(qp, kp, vp, out.ptr, *self._common(), _stream())
        elif entry == "lse":
            rc = lib.dyn_attention_fwd_lse(qp, kp, vp, out.ptr, lse.ptr, *self._common(), _stream())
        else:
            need = lib.dyn_attention_fwd_split_workspace_bytes(self.B, self.T, self.H, nsplit)
            ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device=self.cuda)
            rc = lib.dyn_attention_fwd_split(qp, kp, vp, out.ptr, lse.ptr, *self._common(), nsplit, ws.data_ptr(), need, _stream())
        check(rc, f"{self.name} {entry}")
        return out, lse

    def check_forward(self, tag, out, lse):
        case = f"{self.name} {tag}"
        out64, lse64, out32, lse32 = self.ref()
        _measured(case, "out", out.cpu(), out32, out64, 2e-5)
        out.contained(case, "out")
        if lse is not None:
            _measured(case, "lse", lse.cpu(), lse32, lse64, 2e-5)
            lse.contained(case, "lse")

    def backward(self, out, lse):
        """dyn_attention_bwd on the kernel's own out / lse.  Returns (gradient Bufs [one packed, or three], delta Stat)."""
        from dynamic_asr_eval_amd._lib import check, load
        B, T, H, HD = self.B, self.T, self.H, self.HD
        dout = Buf(self.cuda, B, T, H, self.orow, self.obatch, outside=NAN, tail=self._tail(self.orow)).put(self.dout)
        if self.strided:
            grads = [Buf(self.cuda, B, T, H, self.grow, self.gbatch, tail=self._tail(self.grow)).arm() for _ in range(3)]
            gp = [g.ptr for g in grads]
        else:
            grads = [Buf(self.cuda, B, T, H, self.grow, self.gbatch, (0, HD, 2 * HD)).arm()]
            gp = grads[0].ptrs
        delta = Stat(self.cuda, B, H, T)
        qp, kp, vp = self.inp.ptrs
        check(load().dyn_attention_bwd(qp, kp, vp, out.ptr, dout.ptr, lse.ptr, delta.ptr, *gp, *self._common()[:-1], self.grow, self.gbatch,
                                       self.scale, _stream()), f"{self.name} bwd")
        return grads, delta

    def check_backward(self, tag, out, grads, delta):
        case = f"{self.name} {tag}"
        got = [g.cpu() for g in grads] if self.strided else [grads[0].cpu(i) for i in range(3)]
        o = out.cpu()
        want = K.attention_bwd_ref(self.q, self.k, self.v, o, self.dout, self.scale)
        floors = [2e-5 * g64.abs().max().item() for g64 in want[:3]]
        if self.T == 1:                  # dQ = dK = 0 identically: no gradient to be relative to (kernel_refs.attention_cancellation_bound)
            floors[:2] = K.attention_cancellation_bound(self.q, self.k, self.v, o, self.dout, self.scale)
        for name, g, g32, g64, floor in zip(("dq", "dk", "dv"), got, self.grads32(), want[:3], floors):
            _measured(case, name, g, g32, g64, floor)
        _measured(case, "delta", delta.cpu(), None if self.floors_only else (self.dout * o).sum(-1), want[3],
                  2e-5 * max(1.0, want[3].abs().max().item()))
        for name, g in zip(("dq", "dk", "dv") if self.strided else ("dqkv",), grads):
            g.contained(case, name)
        delta.contained(case, "delta")

    def all_entries(self, split=None):
        """Forward without lse, forward with lse, backward with delta — and the forced key split — against float64."""
        out, _ = self.forward("fwd")
        self.check_forward("fwd", out, None)
        out, lse = self.forward("lse")
        self.check_forward("fwd_lse", out, lse)
        grads, delta = self.backward(out, lse)
        self.check_backward("bwd", out, grads, delta)
        if split is not None:
            self.check_forward(f"split{split}", *self.forward("split", split))
        return out, lse, grads, delta


def _same_bits(a, b):
    return torch.equal(_bits(a.flat), _bits(b.flat))


def _inputs(B, H, T, seed, kind="plain", step=0.5):
    return K.attention_inputs(B, H, T, seed, kind, step, SCALE)


# ----------------------------------------------------------------------------------------------------------- 1. tile edges
@pytest.mark.parametrize("T", TILE_EDGES)
def test_tile_edges(cuda, T):
    """T at and next to 1, the 4-key register group, the 32-key tile and the 128-row block (for T <= 4 the whole upper lane half is masked
    and lives on the exchange of the maximum): forward, forward with lse, backward with delta against float64; the backward twice, bit-equal."""
    c = Case(cuda, f"edges T={T}", *_inputs(2, 2, T, 1), SCALE)
    out, lse, grads, delta = c.all_entries()
    again, delta2 = c.backward(out, lse)
    _exact(c.name, "dqkv of a second backward", _same_bits(grads[0], again[0]))
    _exact(c.name, "delta of a second backward", _same_bits(delta, delta2))


# ----------------------------------------------------------------------------------------------------------- 2. score range
@pytest.mark.parametrize("T", [100, 257])
@pytest.mark.parametrize("kind", ["peaky", "rising", "falling", "zero-scale"])
def test_score_range(cuda, kind, T):
    """(a) q rows * 8: peaky rows; (b) / (c) every score carries +- 0.5 per key index (16 per key tile): the running maximum rises on every
    tile and alpha = exp(m_run - m_new) rescales all of O each time, or it never rises after the first; (d) scale = 0: out is the column mean
    of V, lse = log T, dQ = dK = 0, held to the floors alone.  All three entry points, and two key splits at T = 257."""
    zero = kind == "zero-scale"
    c = Case(cuda, f"range {kind} T={T}", *_inputs(2, 2, T, 2, "plain" if zero else kind), 0.0 if zero else SCALE, floors_only=zero)
    c.all_entries(split=2 if T == 257 else None)


# ----------------------------------------------------------------------------------------------------------- 3. exact routing
@pytest.mark.parametrize("T", [96, 300])
def test_exact_routing(cuda, T):
    """q_i = 400 k_pi(i) on unit-length keys, scale 1: every weight but the winner's is exactly 0, so out must be v[pi] bit for bit and lse
    the winning score (to 2e-5 |s|) — through the plain forward and every split count in 1 .. 8 the host guard accepts for this T; the
    counts it does not accept are rejected with nothing written.  A wrong register -> key or key -> V-row mapping in any tile or split shows
    as a wrong row, not as an error a 2e-5 comparison on smooth data could blur."""
    from dynamic_asr_eval_amd._lib import DynError
    q, k, v, pi, win = K.attention_routing_inputs(2, 2, T)
    c = Case(cuda, f"routing T={T}", q, k, v, torch.zeros_like(v), 1.0)
    want = torch.gather(v, 2, pi[..., None].expand_as(v))
    lse_tol = 2e-5 * win.abs().max().item()

    def exact(tag, out, lse):
        o = out.cpu()
        for b in range(c.B):
            for h in range(c.H):
                _exact(f"{c.name} {tag}", f"out[{b}, {h}] is v[pi]", torch.equal(o[b, h], want[b, h]))
        out.contained(f"{c.name} {tag}", "out")
        if lse is not None:
            err = K.max_err(lse.cpu(), win)
            _line(f"{c.name} {tag}", "lse against the winning score", err, None, lse_tol)
            assert err <= lse_tol
            lse.contained(f"{c.name} {tag}", "lse")

    exact("fwd", *c.forward("fwd"))
    exact("fwd_lse", *c.forward("lse"))
    accepted = [n for n in range(1, 9) if K.attention_split_fits(T, n)]
    assert accepted == ([1, 2, 3] if T == 96 else [1, 2, 3, 4, 5])
    for n in range(1, 9):
        if n in accepted:
            exact(f"split{n}", *c.forward("split", n))
        else:
            with pytest.raises(DynError, match="key splits do not fit"):
                c.forward("split", n)


# ----------------------------------------------------------------------------------------------------------- 4. strides and containment
def test_strides_and_containment(cuda):
    """T = 130, B = 2, H = 3 in the strided layout of Case: forward, forward with lse, two key splits and the backward match float64, and
    every float outside [b, :T, h * 128 : (h + 1) * 128] of out, dq, dk, dv and outside the B * H * T of lse and delta keeps its bits.  The
    packed layout on the same inputs gives the same bits."""
    data = _inputs(2, 3, 130, 4)
    c = Case(cuda, "strided T=130", *data, SCALE, strided=True)
    out, lse, grads, delta = c.all_entries(split=2)
    p = Case(cuda, "packed T=130", *data, SCALE)
    pout, plse = p.forward("lse")
    pgrads, pdelta = p.backward(pout, plse)
    _exact(c.name, "out against the packed call", torch.equal(out.cpu(), pout.cpu()))
    _exact(c.name, "lse against the packed call", torch.equal(lse.cpu(), plse.cpu()))
    _exact(c.name, "delta against the packed call", torch.equal(delta.cpu(), pdelta.cpu()))
    for i, name in enumerate(("dq", "dk", "dv")):
        _exact(c.name, f"{name} against the packed call", torch.equal(grads[i].cpu(), pgrads[0].cpu(i)))


def test_batch_sub_view(cuda):
    """The model's clean-copy call: ops.attention_fwd(qkv[1:], B - 1, ..., out=O[1:]) on a batch of 2 — batch 1 matches float64, batch 0
    of the output is untouched."""
    from dynamic_asr_eval_amd import ops
    B, H, T, case = 2, 2, 130, "sub-view T=130"
    q, k, v, _ = _inputs(B, H, T, 5)
    qkv = torch.stack([q, k, v], 2).permute(0, 3, 2, 1, 4).reshape(B, T, 3 * H * D).contiguous().to(cuda)
    O = torch.full((B, T, H * D), NAN, device=cuda)
    ops.attention_fwd(qkv[1:], B - 1, T, H, D, SCALE, out=O[1:])
    out64, _ = K.attention_ref(q[1:], k[1:], v[1:], SCALE)
    out32, _ = K.attention_torch_fp32(q[1:], k[1:], v[1:], SCALE)
    _measured(case, "out[1:]", O[1:].view(B - 1, T, H, D).transpose(1, 2).cpu(), out32, out64, 2e-5)
    _exact(case, "out[0] untouched", bool(torch.isnan(O[0]).all()))


# ----------------------------------------------------------------------------------------------------------- 5. merge kernel
def test_merge_strides_over_rows_beyond_the_grid(cuda):
    """B = 33, H = 32, T = 64, two splits: 67584 rows x 32 float4 columns = 2162688 threads' worth against attention_merge_kernel's grid of
    8192 x 256 = 2097152, so the last 65536 items are the second pass of its stride loop (an unvisited one stays NaN).  out and lse against
    float64, and a second run bit-equal."""
    B, H, T = 33, 32, 64
    assert B * T * H * (D // 4) > 8192 * 256
    c = Case(cuda, f"merge grid B={B} H={H} T={T}", *_inputs(B, H, T, 6), SCALE)
    out, lse = c.forward("split", 2)
    c.check_forward("split2", out, lse)
    out2, lse2 = c.forward("split", 2)
    _exact(c.name, "out of a second run", _same_bits(out, out2))
    _exact(c.name, "lse of a second run", _same_bits(lse, lse2))


@pytest.mark.parametrize("nsplit", [7, 8])
def test_merge_uneven_and_even_splits(cuda, nsplit):
    """T = 1024 = 32 key tiles: 7 splits take 5, 5, 5, 5, 5, 5, 2 tiles (the last one short), 8 take 4 each."""
    assert K.attention_split_fits(1024, nsplit)
    c = Case(cuda, f"merge T=1024 nsplit={nsplit}", *_inputs(1, 2, 1024, 7), SCALE)
    c.check_forward(f"split{nsplit}", *c.forward("split", nsplit))


def test_merge_with_an_underflowing_split(cuda):
    """T = 256, two splits, scores rising by 1 per key: the first split's lse is more than 110 below the second's (asserted by the generator),
    its weight exp(lse_0 - m) is 0 in fp32.  Finite and within bound."""
    c = Case(cuda, "merge underflow T=256", *K.attention_underflow_inputs(2, 2), SCALE)
    out, lse = c.forward("split", 2)
    assert bool(torch.isfinite(out.cpu()).all()) and bool(torch.isfinite(lse.cpu()).all())
    c.check_forward("split2", out, lse)


@pytest.mark.parametrize("T", [100, 257])
def test_one_split_is_the_unsplit_kernel(cuda, T):
    """nsplit = 1 through dyn_attention_fwd_split is bit-equal to dyn_attention_fwd_lse (and needs no workspace)."""
    c = Case(cuda, f"one split T={T}", *_inputs(2, 2, T, 8), SCALE)
    out, lse = c.forward("lse")
    out1, lse1 = c.forward("split", 1)
    _exact(c.name, "out", _same_bits(out, out1))
    _exact(c.name, "lse", _same_bits(lse, lse1))


# ----------------------------------------------------------------------------------------------------------- 6. host guards
def test_host_guards(cuda):
    """Every call the host must reject raises the library's error and leaves the NaN-prefilled out / lse / delta / gradients all NaN;
    B = 0 and T = 0 return success and write nothing either."""
    from dynamic_asr_eval_amd._lib import DynError, check, load
    lib = load()
    B, H, T, TMAX = 1, 1, 100, 256                                # every buffer holds TMAX rows: the calls at T = 256 are valid but for the guard
    HD = H * D
    c = Case(cuda, "guards", *_inputs(B, H, TMAX, 9), SCALE)
    qp, kp, vp = c.inp.ptrs
    out = torch.full((B, TMAX, HD), NAN, device=cuda)
    lse = torch.full((B, H, TMAX), NAN, device=cuda)
    delta = torch.full((B, H, TMAX), NAN, device=cuda)
    dqkv = torch.full((B, TMAX, 3 * HD), NAN, device=cuda)
    o_in = torch.zeros(B, TMAX, HD, device=cuda)                 # out / dout / lse as inputs of the backward
    l_in = torch.zeros(B, H, TMAX, device=cuda)
    need2 = lib.dyn_attention_fwd_split_workspace_bytes(B, TMAX, H, 2)
    assert need2 == 2 * (B * TMAX * HD + B * H * TMAX) * 4
    ws = torch.full((9 * (need2 // 2) + 16,), 0xFF, dtype=torch.uint8, device=cuda)      # enough for nine splits, were they allowed
    g = dqkv.data_ptr()

    def split(q=qp, T=T, B=B, head_dim=D, row=3 * HD, nsplit=1, wsp=ws.data_ptr(), wsb=ws.numel(), lsep=lse.data_ptr()):
        return lib.dyn_attention_fwd_split(q, kp, vp, out.data_ptr(), lsep, B, T, H, head_dim, row, T * row, HD, T * HD, SCALE, nsplit, wsp, wsb,
                                           _stream())

    def fwd(q=qp, T=T, B=B, head_dim=D, row=3 * HD):
        return lib.dyn_attention_fwd(q, kp, vp, out.data_ptr(), B, T, H, head_dim, row, T * row, HD, T * HD, SCALE, _stream())

    def fwd_lse(lsep=lse.data_ptr(), T=T, B=B):
        return lib.dyn_attention_fwd_lse(qp, kp, vp, out.data_ptr(), lsep, B, T, H, D, 3 * HD, T * 3 * HD, HD, T * HD, SCALE, _stream())

    def bwd(q=qp, T=T, B=B, head_dim=D, row=3 * HD, deltap=delta.data_ptr()):
        return lib.dyn_attention_bwd(q, kp, vp, o_in.data_ptr(), o_in.data_ptr(), l_in.data_ptr(), deltap, g, g + 4 * HD, g + 8 * HD, B, T, H,
                                     head_dim, row, T * row, HD, T * HD, 3 * HD, T * 3 * HD, SCALE, _stream())

    def untouched(what):
        ok = all(bool(torch.isnan(t).all()) for t in (out, lse, delta, dqkv))
        print(f"  guards {what}: out, lse, delta and the gradients still all NaN {ok}")
        assert ok, what

    rejected = [("head_dim = 64 (fwd)", "head_dim 64", lambda: fwd(head_dim=64)),
                ("head_dim = 64 (split)", "head_dim 64", lambda: split(head_dim=64, nsplit=2, T=TMAX)),
                ("head_dim = 64 (bwd)", "head_dim 64", lambda: bwd(head_dim=64)),
                ("q offset by 4 bytes (fwd)", "16-byte aligned", lambda: fwd(q=qp + 4)),
                ("q offset by 4 bytes (bwd)", "16-byte aligned", lambda: bwd(q=qp + 4)),
                ("row_stride = 3 HD + 2 (fwd)", "multiples of 4 floats", lambda: fwd(row=3 * HD + 2)),
                ("row_stride = 3 HD + 2 (bwd)", "multiples of 4 floats", lambda: bwd(row=3 * HD + 2)),
                ("nsplit = 9", "key splits do not fit", lambda: split(nsplit=9, T=TMAX)),
                ("nsplit = 8 at T = 100 (4 key tiles)", "key splits do not fit", lambda: split(nsplit=8)),
                ("nsplit = 2, workspace one byte short", "workspace bytes", lambda: split(nsplit=2, T=TMAX, wsb=need2 - 1)),
                ("nsplit = 2, workspace 4 bytes off alignment", "workspace bytes", lambda: split(nsplit=2, T=TMAX, wsp=ws.data_ptr() + 4, wsb=need2)),
                ("nsplit = 2, no workspace", "workspace bytes", lambda: split(nsplit=2, T=TMAX, wsp=0, wsb=0)),
                ("fwd_lse with lse = NULL", "lse is NULL", lambda: fwd_lse(lsep=0)),
                ("bwd with delta = NULL", "bad arguments", lambda: bwd(deltap=0))]
    for what, text, call in rejected:
        with pytest.raises(DynError, match=text):
            check(call(), what)
        untouched(what)
    for what, kw in (("B = 0", dict(B=0)), ("T = 0", dict(T=0))):
        for name, call in (("fwd", fwd), ("fwd_lse", fwd_lse), ("split", split), ("bwd", bwd)):
            rc = call(**kw)
            print(f"  guards {what} {name}: returns {rc}")
            assert rc == 0
        untouched(what)
