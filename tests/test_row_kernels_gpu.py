"""The row softmax family (csrc/softmax_row.h and the kernels built on it: softmax.hip, relshift.hip, relbias.hip) against float64 at every
compiled instance, past every grid cap and at every edge of the device-side key length.

What was not covered before: tests/test_ops_gpu.py::test_softmax_family stops at rows of 4096 (ITEMS <= 16 of the instances 1, 2, 4, ..., 64
forward / ..., 32 backward), the relative-position kernels were compared at T <= 300 (ITEMS <= 2), no test had more rows than a grid
(`row += gridDim.x` never ran), `valid` was only given in-range values, and nothing called the plain kernels with a padded row stride.

References: tests/kernel_refs.py ("the row softmax family"), each held to torch's own op and autograd in tests/test_kernel_refs_cpu.py.  They
are evaluated ON THE DEVICE, in float64 for the reference and in float32 for torch's own fp32 result of the same expression; every row of
every case is compared (the square cases are too large for the CPU; T = 16384 square is left out: 10 GB of float64 for an instance T = 8193
already runs, and the plain kernels reach the limit itself).  Inputs come from a seeded device generator and are O(1): randn, * 4 for plain
scores as test_softmax_family does, gate in (0, 3) as tests/test_wavlm_gpu.py.

Bounds: kernel_refs.measured_tol — 4 x torch's fp32 error against float64 plus the project's floor for that kind of result: 2e-6
probabilities, 1e-5 log-probabilities, 2e-5 input gradients that sum a row (softmax_bwd, dgate), 2e-6 * scale for the entropy gradient and
2e-6 for the entropy (tests/test_kernel_parity_f64_gpu.py::test_entropy_grad); log_softmax_bwd keeps test_softmax_family's
2e-6 * max(L, 16); dE is a long sum of O(1) terms: kernel_refs.wgrad_tol(5e-4, products in the fullest bucket, 531).  Masked columns,
copies, in-place against out-of-place and repeated runs are bit-exact (torch.equal).  Outputs are prefilled with NaN, so an element a
kernel does not write shows.  Every check prints `case name: kernel error | torch fp32 error | bound` before it asserts (pytest -s; the
table of one MI355X run is profiles/row_kernels_parity.txt).  Nothing here measures speed."""
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

NAN = float("nan")
GRID_CAP = 65535 * 4                    # row_grid of csrc/softmax.hip and the relshift forward; relshift_bwd_kernel's is 65536
FWD_L = [1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384]      # both edges of ITEMS = 1 .. 64
BWD_L = [L for L in FWD_L if L <= 8192]                                                      # both edges of ITEMS = 1 .. 32
BUCKETS = (320, 800)                    # WavLM's default num_buckets, max_bucket_distance
D = 64                                  # head dimension the relbias entries are told (H = nh * D; they only check it)


# ----------------------------------------------------------------------------------------------------------- helpers
def _gen(cuda, seed):
    g = torch.Generator(device=cuda)
    g.manual_seed(seed)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device)


def _valid(cuda, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=cuda)


def _nan_like(t):
    return torch.full_like(t, NAN)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _line(case, name, err, e32, tol):
    print(f"  {case} {name}: kernel {err:.2e} | torch fp32 {'-' if e32 is None else format(e32, '.2e')} | bound {tol:.2e}")


def _measured(case, name, got, torch32, want, floor):
    tol, e32 = K.measured_tol(torch32, want, floor)
    err = K.max_err(got, want)
    _line(case, name, err, e32, tol)
    assert err <= tol, f"{case} {name}: err {err} > {tol} (torch fp32: {e32})"          # a NaN error fails here too


def _bounded(case, name, got, torch32, want, tol):
    err, e32 = K.max_err(got, want), K.max_err(torch32, want)
    _line(case, name, err, e32, tol)
    assert err <= tol, f"{case} {name}: err {err} > {tol} (torch fp32: {e32})"


def _exact(case, name, got, want):
    ok = got.shape == want.shape and torch.equal(got, want)
    print(f"  {case} {name}: bit-equal {ok}")
    assert ok, f"{case} {name}: not bit-equal"


def _finite_part(got, want):
    """(got, want) with the -inf entries of `want` set to 0 in both, after asserting that `got` is -inf exactly there."""
    inf = want == -math.inf
    assert torch.equal(got == -math.inf, inf), "-inf where, and only where, the reference has it"
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    return torch.where(inf, zero, got), torch.where(inf, zero.to(want.dtype), want)


def _masked_exactly(case, y, Lv, value=0.0):
    tail = y[..., Lv:]
    _exact(case, f"columns past {Lv} are {value:g}", tail, torch.full_like(tail, value))


def _entropy_grad(logp, scale):
    """dyn_entropy_grad on NaN-prefilled outputs (ops.entropy_grad hands the kernel uninitialised ones)."""
    from dynamic_asr_eval_amd._lib import check, load
    rows, L = logp.shape
    g, ent = _nan_like(logp), torch.full((rows,), NAN, device=logp.device)
    check(load().dyn_entropy_grad(logp.data_ptr(), g.data_ptr(), ent.data_ptr(), rows, L, L, scale, _stream()), "dyn_entropy_grad")
    return g, ent


def _check_softmax(case, x, dy, scale):
    from dynamic_asr_eval_amd import ops
    y = ops.softmax(x, out=_nan_like(x))
    _measured(case, "softmax", y, K.row_softmax_ref(x), K.row_softmax_ref(x.double()), 2e-6)
    return y


def _check_log_softmax(case, x, dy, scale):
    from dynamic_asr_eval_amd import ops
    ly = ops.log_softmax(x, out=_nan_like(x))
    _measured(case, "log_softmax", ly, K.row_log_softmax_ref(x), K.row_log_softmax_ref(x.double()), 1e-5)
    return ly


# The backward kernels are judged on their own: their y / log y is the float64 forward rounded to fp32, the same tensor for kernel and reference.
def _check_softmax_bwd(case, x, dy, scale):
    from dynamic_asr_eval_amd import ops
    y = K.row_softmax_ref(x.double()).float()
    got = ops.softmax_bwd(y, dy, out=_nan_like(y), scale=0.5)
    _measured(case, "softmax_bwd", got, K.softmax_bwd_ref(y, dy, 0.5), K.softmax_bwd_ref(y.double(), dy.double(), 0.5), 2e-5)


def _check_log_softmax_bwd(case, x, dy, scale):
    from dynamic_asr_eval_amd import ops
    logy = K.row_log_softmax_ref(x.double()).float()
    got = ops.log_softmax_bwd(logy, dy, out=_nan_like(logy))
    _bounded(case, "log_softmax_bwd", got, K.log_softmax_bwd_ref(logy, dy), K.log_softmax_bwd_ref(logy.double(), dy.double()),
             2e-6 * max(x.shape[-1], 16))


def _check_entropy_grad(case, x, dy, scale):
    logy = K.row_log_softmax_ref(x.double()).float()
    grad, ent = _entropy_grad(logy, scale)
    g64, H64 = K.entropy_grad_expr(logy.double(), scale)
    g32, H32 = K.entropy_grad_expr(logy, scale)
    _measured(case, "entropy", ent, H32, H64, 2e-6)
    _measured(case, "entropy_grad", grad, g32, g64, 2e-6 * scale)


PLAIN = {"softmax": _check_softmax, "log_softmax": _check_log_softmax, "softmax_bwd": _check_softmax_bwd,
         "log_softmax_bwd": _check_log_softmax_bwd, "entropy_grad": _check_entropy_grad}


def _plain_inputs(cuda, rows, L, seed):
    g = _gen(cuda, seed)
    return _randn(g, rows, L) * 4, _randn(g, rows, L)


# ----------------------------------------------------------------------------------------------------------- 1. every plain instance
@pytest.mark.parametrize("L", FWD_L)
def test_plain_forward_at_both_edges_of_every_instance(cuda, L):
    """softmax / log_softmax at L = 256 k and 256 k + 1 for every ITEMS = k in 1 .. 64 (L = 1 and the row limit 16384 included), three
    rows; at 8193 and 16384 also in place (the attention softmax runs in place), bit-equal to out of place."""
    from dynamic_asr_eval_amd import ops
    case = f"plain L={L}"
    x, dy = _plain_inputs(cuda, 3, L, 100 + L)
    y, ly = _check_softmax(case, x, dy, None), _check_log_softmax(case, x, dy, None)
    if L in (8193, 16384):
        a, b = x.clone(), x.clone()
        ops.softmax(a, out=a); ops.log_softmax(b, out=b)
        _exact(case, "softmax in place", a, y)
        _exact(case, "log_softmax in place", b, ly)


@pytest.mark.parametrize("L", BWD_L)
def test_plain_backward_at_both_edges_of_every_instance(cuda, L):
    """softmax_bwd (scale 0.5), log_softmax_bwd and entropy_grad (scale 1 / rows, the mean entropy) for every ITEMS in 1 .. 32."""
    case = f"plain L={L}"
    x, dy = _plain_inputs(cuda, 3, L, 200 + L)
    for name in ("softmax_bwd", "log_softmax_bwd", "entropy_grad"):
        PLAIN[name](case, x, dy, 1.0 / 3.0)


# ----------------------------------------------------------------------------------------------------------- 2. padded row strides
@pytest.mark.parametrize("L", [300, 4097])
def test_plain_kernels_with_padded_row_strides(cuda, L):
    """dyn_softmax_fwd / dyn_softmax_fwd_len / dyn_log_softmax_fwd with ldx = L + 3 != ldy = L + 5 and the two backwards with ld = L + 3, through the C-ABI: the
    input padding holds NaN (none may reach a result), the output padding a sentinel (it must stay), five rows."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    lib, case, rows, sentinel = load(), f"strided L={L}", 5, 5.0
    g = _gen(cuda, 300 + L)
    x, dy = _randn(g, rows, L) * 4, _randn(g, rows, L)

    def padded(t, ld, fill):
        p = torch.full((rows, ld), fill, device=cuda)
        if t is not None:
            p[:, :L] = t
        return p

    def untouched(name, p):
        _exact(case, f"{name} output padding", p[:, L:], torch.full_like(p[:, L:], sentinel))

    ldx, ldy, ld = L + 3, L + 5, L + 3
    xp = padded(x, ldx, NAN)
    for name, entry, ref, floor, dense in (("softmax", lib.dyn_softmax_fwd, K.row_softmax_ref, 2e-6, ops.softmax),
                                           ("log_softmax", lib.dyn_log_softmax_fwd, K.row_log_softmax_ref, 1e-5, ops.log_softmax)):
        yp = padded(None, ldy, sentinel)
        check(entry(xp.data_ptr(), yp.data_ptr(), rows, L, ldx, ldy, _stream()), name)
        _measured(case, name, yp[:, :L], ref(x), ref(x.double()), floor)
        _exact(case, f"{name} against the dense call", yp[:, :L], dense(x))
        untouched(name, yp)
    yp, vd = padded(None, ldy, sentinel), _valid(cuda, L - 7)                           # the masked form takes the same strides
    check(lib.dyn_softmax_fwd_len(xp.data_ptr(), yp.data_ptr(), rows, L, ldx, ldy, vd.data_ptr(), _stream()), "dyn_softmax_fwd_len")
    _measured(case, "softmax valid L-7", yp[:, :L], K.row_softmax_ref(x, L - 7), K.row_softmax_ref(x.double(), L - 7), 2e-6)
    _masked_exactly(case, yp[:, :L], L - 7)
    untouched("softmax valid L-7", yp)
    y, logy = K.row_softmax_ref(x.double()).float(), K.row_log_softmax_ref(x.double()).float()
    yp, lyp, dyp = padded(y, ld, NAN), padded(logy, ld, NAN), padded(dy, ld, NAN)
    dxp = padded(None, ld, sentinel)
    check(lib.dyn_softmax_bwd(yp.data_ptr(), dyp.data_ptr(), dxp.data_ptr(), rows, L, ld, 0.5, _stream()), "dyn_softmax_bwd")
    _measured(case, "softmax_bwd", dxp[:, :L], K.softmax_bwd_ref(y, dy, 0.5), K.softmax_bwd_ref(y.double(), dy.double(), 0.5), 2e-5)
    _exact(case, "softmax_bwd against the dense call", dxp[:, :L], ops.softmax_bwd(y, dy, scale=0.5))
    untouched("softmax_bwd", dxp)
    dxp = padded(None, ld, sentinel)
    check(lib.dyn_log_softmax_bwd(lyp.data_ptr(), dyp.data_ptr(), dxp.data_ptr(), rows, L, ld, _stream()), "dyn_log_softmax_bwd")
    _bounded(case, "log_softmax_bwd", dxp[:, :L], K.log_softmax_bwd_ref(logy, dy), K.log_softmax_bwd_ref(logy.double(), dy.double()),
             2e-6 * max(L, 16))
    untouched("log_softmax_bwd", dxp)


# ----------------------------------------------------------------------------------------------------------- 3. relshift instances
def _relshift_inputs(cuda, B, nh, T, pad, seed):
    g = _gen(cuda, seed)
    R = 2 * T - 1
    S = _randn(g, B, nh, T, T)
    BD = torch.full((B, nh, T, R + pad), NAN, device=cuda)
    BD[..., :R] = _randn(g, B, nh, T, R)
    return S, BD, R + pad


def _relshift_forward_case(cuda, case, S, BD, ld, valid, inplace):
    from dynamic_asr_eval_amd import ops
    T = S.shape[-1]
    vd = _valid(cuda, valid)
    y = ops.softmax_relshift(S, BD, out=_nan_like(S), valid=vd, ld_bd=ld)
    y64 = K.row_softmax_ref(K.relshift_scores_ref(S.double(), BD.double()), valid)
    y32 = K.row_softmax_ref(K.relshift_scores_ref(S, BD), valid)
    _measured(case, "probabilities", y, y32, y64, 2e-6)
    del y64, y32
    if valid is not None:
        _masked_exactly(case, y, K.clamped_valid(valid, T))
    if inplace:
        a = S.clone()
        ops.softmax_relshift(a, BD, out=a, valid=vd, ld_bd=ld)
        _exact(case, "in place", a, y)
    return y


@pytest.mark.parametrize("T,nh,pad,valid,inplace", [(513, 2, 0, None, False), (1025, 2, 4, 700, False), (2049, 2, 0, None, False),
                                                    (4097, 1, 0, None, False), (8193, 1, 0, 5000, True)],
                         ids=["T513", "T1025-ld2T+3-valid700", "T2049", "T4097", "T8193-valid5000-inplace"])
def test_softmax_relshift_instances(cuda, T, nh, pad, valid, inplace):
    """ITEMS = 4, 8, 16, 32 and 64 of softmax_relshift_fwd_kernel, one column past the previous instance each; `ld_bd = 2T + 3` pads BD's
    rows with NaN that is never read."""
    S, BD, ld = _relshift_inputs(cuda, 1, nh, T, pad, 400 + T)
    _relshift_forward_case(cuda, f"relshift T={T}", S, BD, ld, valid, inplace)


def test_relshift_bwd_is_a_copy_at_T1025(cuda):
    """dBD of a padded row (ld_bd = 2T + 3): dS inside the window, zeros everywhere else, every column written (the output starts as NaN)."""
    from dynamic_asr_eval_amd import ops
    T, ld = 1025, 2 * 1025 + 3
    dS = _randn(_gen(cuda, 450), 1, 2, T, T)
    out = torch.full((1, 2, T, ld), NAN, device=cuda)
    assert ops.relshift_bwd(dS, out=out, ld_bd=ld) is out
    _exact("relshift_bwd T=1025", "dBD", out, K.relshift_bwd_ref(dS, ld))


# ----------------------------------------------------------------------------------------------------------- 4. relbias instances
def _relbias_inputs(cuda, nh, T, Tmax, seed):
    from dynamic_asr_eval_amd import ops
    g = _gen(cuda, seed)
    S = _randn(g, 1, nh, T, T)
    gate = torch.rand(1, nh, T, generator=g, device=cuda) * 3
    E = _randn(g, BUCKETS[0], nh)
    table = ops.relative_position_buckets(Tmax, *BUCKETS).to(cuda)
    return S, gate, E, table


def _relbias_forward_case(cuda, case, S, gate, E, table, Tmax, valid, inplace):
    from dynamic_asr_eval_amd import ops
    T = S.shape[-1]
    vd = _valid(cuda, valid)
    y = ops.softmax_relbias(S, gate, E, table, D, out=_nan_like(S), valid=vd)
    y64 = K.row_softmax_ref(K.relbias_scores_ref(S.double(), gate.double(), E.double(), table, Tmax), valid)
    y32 = K.row_softmax_ref(K.relbias_scores_ref(S, gate, E, table, Tmax), valid)
    _measured(case, "probabilities", y, y32, y64, 2e-6)
    del y64, y32
    if valid is not None:
        _masked_exactly(case, y, K.clamped_valid(valid, T))
    if inplace:
        a = S.clone()
        ops.softmax_relbias(a, gate, E, table, D, out=a, valid=vd)
        _exact(case, "in place", a, y)
    return y


@pytest.mark.parametrize("T,nh,extra,valid,inplace", [(513, 2, 0, None, False), (1025, 2, 7, 700, False), (2049, 2, 0, None, False),
                                                      (4097, 1, 0, None, False), (8193, 1, 0, None, True)],
                         ids=["T513", "T1025-Tmax+7-valid700", "T2049", "T4097", "T8193-inplace"])
def test_softmax_relbias_instances(cuda, T, nh, extra, valid, inplace):
    """ITEMS = 4 .. 64 of softmax_relbias_fwd_kernel with WavLM's default (320, 800) table: the last row block holds one row, distances run
    through the exact, the logarithmic and the clamped part; `Tmax = T + 7` reads a table built for more frames than the scores have."""
    S, gate, E, table = _relbias_inputs(cuda, nh, T, T + extra, 500 + T)
    _relbias_forward_case(cuda, f"relbias T={T}", S, gate, E, table, T + extra, valid, inplace)


@pytest.mark.parametrize("T,nh,extra", [(513, 2, 0), (1025, 2, 7), (2049, 2, 0), (4097, 1, 0)], ids=["T513", "T1025-Tmax+7", "T2049", "T4097"])
def test_relbias_bwd_instances(cuda, T, nh, extra):
    """ITEMS = 4 .. 32 of relbias_bwd_rows_kernel and the two kernels that fold its diagonals into buckets: dgate and dE with beta 0 and 1
    on a prefilled dE, each run twice (the backward has no float atomics: bit-equal)."""
    from dynamic_asr_eval_amd import ops
    Tmax = T + extra
    dS, gate, E, table = _relbias_inputs(cuda, nh, T, Tmax, 600 + T)
    dgate64, dE64 = K.relbias_bwd_ref(dS.double(), gate.double(), E.double(), table, Tmax)
    dgate32, dE32 = K.relbias_bwd_ref(dS, gate, E, table, Tmax)
    dE_tol = K.wgrad_tol(5e-4, K.relbias_fullest_bucket(table, T, Tmax, 1), 531)
    old = torch.full_like(E, 0.75)
    for beta in (0.0, 1.0):
        case = f"relbias_bwd T={T} beta={beta:g}"
        dE = old.clone()
        dgate = ops.relbias_bwd(dS, gate, E, table, D, dE, beta=beta)
        _measured(case, "dgate", dgate, dgate32, dgate64, 2e-5)
        _bounded(case, "dE", dE, dE32 + beta * old, dE64 + beta * old.double(), dE_tol)
        again = old.clone()
        _exact(case, "dgate of a second run", ops.relbias_bwd(dS, gate, E, table, D, again, beta=beta), dgate)
        _exact(case, "dE of a second run", again, dE)


# ----------------------------------------------------------------------------------------------------------- 5. more rows than a grid
@pytest.mark.parametrize("kernel", list(PLAIN))
def test_plain_kernels_stride_over_rows_beyond_the_grid(cuda, kernel):
    """65535 * 4 + 41 rows of L = 3: the last 41 rows are the second pass of `row += gridDim.x` in softmax_fwd_kernel, softmax_bwd_kernel
    (both forms of each) and entropy_grad_kernel.  All rows are compared; an unvisited row stays NaN."""
    rows = GRID_CAP + 41
    x, dy = _plain_inputs(cuda, rows, 3, 700)
    PLAIN[kernel](f"stride rows={rows} L=3", x, dy, 0.25)


def test_softmax_relshift_strides_over_rows_beyond_the_grid(cuda):
    """M = 7086 score matrices of T = 37: 262 182 rows, 42 past the grid of 65535 * 4, which is no multiple of 37 — the second pass starts at
    another query position i = row % T, i.e. another window of BD, than the workgroup's first row had."""
    T, M = 37, 7086
    assert M * T > GRID_CAP and GRID_CAP % T != 0
    S, BD, ld = _relshift_inputs(cuda, 1, M, T, 0, 710)
    _relshift_forward_case(cuda, f"stride relshift T={T} M={M}", S, BD, ld, None, False)


def test_relshift_bwd_strides_over_rows_beyond_the_grid(cuda):
    """M = 1772, T = 37: 65 564 rows against relshift_bwd_kernel's grid of 65536 (no multiple of 37 either)."""
    from dynamic_asr_eval_amd import ops
    T, M = 37, 1772
    assert M * T > 65536 and 65536 % T != 0
    dS = _randn(_gen(cuda, 720), 1, M, T, T)
    out = torch.full((1, M, T, 2 * T - 1), NAN, device=cuda)
    ops.relshift_bwd(dS, out=out)
    _exact(f"stride relshift_bwd T={T} M={M}", "dBD", out, K.relshift_bwd_ref(dS, 2 * T - 1))


# ----------------------------------------------------------------------------------------------------------- 6. the key length's edges
@pytest.mark.parametrize("kernel", ["softmax", "softmax_relshift", "softmax_relbias"])
def test_valid_is_clamped_into_1_to_L(cuda, kernel):
    """valid_len() clamps the device scalar into [1, L]: -3 and 0 act as 1, 305 as 300.  The scalar is rewritten in place between launches
    and nothing else changes, as under graph replay.  The result is the reference at the clamped length, exactly 0 past it, finite."""
    from dynamic_asr_eval_amd import ops
    T = 300
    vd = _valid(cuda, T)
    if kernel == "softmax":
        x = _randn(_gen(cuda, 800), 9, T) * 4
        run = lambda: ops.softmax(x, out=_nan_like(x), valid=vd)                                   # noqa: E731
        scores = lambda dt: x.to(dt)                                                               # noqa: E731
    elif kernel == "softmax_relshift":
        S, BD, ld = _relshift_inputs(cuda, 1, 2, T, 0, 810)
        run = lambda: ops.softmax_relshift(S, BD, out=_nan_like(S), valid=vd, ld_bd=ld)            # noqa: E731
        scores = lambda dt: K.relshift_scores_ref(S.to(dt), BD.to(dt))                             # noqa: E731
    else:
        S, gate, E, table = _relbias_inputs(cuda, 2, T, T, 820)
        run = lambda: ops.softmax_relbias(S, gate, E, table, D, out=_nan_like(S), valid=vd)        # noqa: E731
        scores = lambda dt: K.relbias_scores_ref(S.to(dt), gate.to(dt), E.to(dt), table, T)        # noqa: E731
    s64, s32 = scores(torch.float64), scores(torch.float32)
    for v in (-3, 0, 1, 299, 300, 305):
        vd.fill_(v)
        Lv = min(max(v, 1), T)
        case = f"{kernel} L=300 valid={v}"
        y = run()
        _measured(case, "probabilities", y, K.row_softmax_ref(s32, Lv), K.row_softmax_ref(s64, Lv), 2e-6)
        _masked_exactly(case, y, Lv)
        assert bool(torch.isfinite(y).all()), case


# ----------------------------------------------------------------------------------------------------------- 7. the prefix claim
@pytest.mark.parametrize("L,valid", [(8193, 4097), (2049, 300)])
def test_masked_row_is_bitwise_the_cut_row_across_instances(cuda, L, valid):
    """softmax_row's promise that bucketed graph replay relies on: the first Lv columns of a masked row are bit for bit those of a row of
    length Lv — here with the masked row in ITEMS = 64 (8) and the cut row in ITEMS = 32 (2)."""
    from dynamic_asr_eval_amd import ops
    case = f"prefix L={L} valid={valid}"
    x = _randn(_gen(cuda, 900 + L), 3, L) * 4
    y = ops.softmax(x, out=_nan_like(x), valid=_valid(cuda, valid))
    cut = x[:, :valid].contiguous()
    _exact(case, "masked row against the cut row", y[:, :valid], ops.softmax(cut, out=_nan_like(cut)))
    _masked_exactly(case, y, valid)
    _measured(case, "probabilities", y, K.row_softmax_ref(x, valid), K.row_softmax_ref(x.double(), valid), 2e-6)


def test_softmax_relshift_masked_far_below_its_instance(cuda):
    """T = 1025 (ITEMS = 8) with 300 valid keys (two items' worth).  The cut problem has another T and another window, so bit equality
    does not apply: the masked result is held to its own float64 bound."""
    T = 1025
    S, BD, ld = _relshift_inputs(cuda, 1, 2, T, 0, 950)
    _relshift_forward_case(cuda, f"prefix relshift T={T}", S, BD, ld, 300, False)


# ----------------------------------------------------------------------------------------------------------- 8. -inf inputs
def test_minus_inf_inputs(cuda):
    """Rows of 513 in which a third of the entries are -inf (a causal or padding mask applied upstream); row 0 keeps a single finite entry.
    Probability exactly 0 and log-probability -inf there, no NaN anywhere, and the two backwards of such rows are finite."""
    from dynamic_asr_eval_amd import ops
    rows, L, case = 7, 513, "minus-inf L=513"
    g = _gen(cuda, 1000)
    x, dy = _randn(g, rows, L) * 4, _randn(g, rows, L)
    hole = torch.rand(rows, L, generator=g, device=cuda) < 1.0 / 3.0
    hole[0] = True
    hole[torch.arange(rows), (torch.arange(rows) * 71 + 5) % L] = False                             # at least one finite entry per row
    x[hole] = -math.inf
    assert 0.25 < hole[1:].float().mean().item() < 0.42 and int((~hole[0]).sum()) == 1
    y = ops.softmax(x, out=_nan_like(x))
    _measured(case, "softmax", y, K.row_softmax_ref(x), K.row_softmax_ref(x.double()), 2e-6)
    _exact(case, "probability of a -inf entry is 0", y[hole], torch.zeros_like(y[hole]))
    ly = ops.log_softmax(x, out=_nan_like(x))
    got, want = _finite_part(ly, K.row_log_softmax_ref(x.double()))
    l32 = K.row_log_softmax_ref(x)
    _measured(case, "log_softmax", got, _finite_part(l32, l32)[0], want, 1e-5)
    _exact(case, "log-probability of a -inf entry is -inf", ly[hole], torch.full_like(ly[hole], -math.inf))
    assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(ly).any()) and bool(torch.isfinite(ly[~hole]).all())
    dx = ops.softmax_bwd(y, dy, out=_nan_like(y), scale=0.5)
    _measured(case, "softmax_bwd", dx, K.softmax_bwd_ref(y, dy, 0.5), K.softmax_bwd_ref(y.double(), dy.double(), 0.5), 2e-5)
    dl = ops.log_softmax_bwd(ly, dy, out=_nan_like(ly))
    _bounded(case, "log_softmax_bwd", dl, K.log_softmax_bwd_ref(ly, dy), K.log_softmax_bwd_ref(ly.double(), dy.double()), 2e-6 * max(L, 16))
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dl).all())
