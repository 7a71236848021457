"""Float64 restatements of the operations behind the C-ABI kernels that only whole-model tests used to reach, each written from the
operation's definition (no call into the torch op it mirrors).  tests/test_kernel_refs_cpu.py checks every one of them against torch's own
op and autograd in float64 to 1e-12, so a wrong reference cannot hide a wrong kernel; tests/test_kernel_parity_f64_gpu.py compares the HIP
kernels with them (the row softmax family: tests/test_row_kernels_gpu.py, on the device; the conformer's own convolutions, dtype- and
device-agnostic: tests/test_conv_kernels_gpu.py; the log-mel front end and the window augmentations: tests/test_frontend_kernels_gpu.py;
the fused streaming attention: tests/test_attention_kernels_gpu.py; the one-token decoder steps, dtype-agnostic:
tests/test_decoder_step_kernels_gpu.py, held to oracle/enc_dec_ref.py's decoder instead of a torch op).
Also here: the inputs both files share, the tolerance rule, and CPU replays of the summation orders the column norm and the log-mel
normalisation used before their statistics were made stable (E[x^2] - mean^2 from fp32 running sums)."""
import math

import numpy as np
import torch

F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def d(t):
    return t.detach().cpu().to(F64)


def max_err(got, want, rel=False):
    """max |got - want| (divided by |want| elementwise when `rel`) in float64, computed where `want` lives (the CPU for the references
    built there; the device for the row-kernel references, whose square cases are too large to bring back)."""
    want = want.detach().to(F64)
    got = got.detach().to(device=want.device, dtype=F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.numel() == 0:
        return 0.0
    e = (got - want).abs()
    if rel:
        e = e / want.abs()
    return e.max().item()


def measured_tol(torch_fp32, ref64, floor, rel=False):
    """The rule for results the project had no tolerance for: torch's own fp32 CPU result of the same op on the same inputs is measured
    against float64, and the kernel is allowed 4 x that (another, equally valid fp32 summation order) plus the absolute floor the
    project already uses for that kind of result.  Returns (tolerance, torch's fp32 error)."""
    e32 = max_err(torch_fp32, ref64, rel)
    return 4.0 * e32 + floor, e32


def wgrad_tol(base, rows, base_rows):
    """Weight-gradient tolerance: `base` is what tests/test_ops_gpu.py asserts at `base_rows` summed rows (5e-4 for the norm gradients at
    531 rows, 3e-4 for the depthwise-conv taps at 400); the rounding error of an fp32 sum of `rows` O(1) terms grows like sqrt(rows),
    so longer sums scale by sqrt(rows / base_rows) (test_fused_first_two_subsampling_stages scales the same way), shorter ones keep `base`."""
    return base * max(1.0, math.sqrt(rows / base_rows))


def wgrad_tol_ill_conditioned(base, rows):
    """base * max(1, sqrt(rows)), the scaling of test_fused_first_two_subsampling_stages taken literally, for the one weight gradient whose
    terms are not O(1) quantities known to fp32 precision: the column norm's dgamma on offset inputs.  Its backward receives the mean as an
    fp32 INPUT, up to ulp(mean) / 2 from the float64 mean; xhat = (x - mean) * rstd carries that as a shift common to a whole column, and
    dgamma = sum dy * xhat collects it times |sum_t dy| ~ sqrt(T) (3e-5 * sqrt(300) = 5e-4 at mean / std = 1000, T = 300) — the property
    of a format, whatever the kernel does, and one wgrad_tol's sqrt(rows / base_rows) of rounding noise does not cover."""
    return base * max(1.0, math.sqrt(rows))


# ----------------------------------------------------------------------------------------------------------- column norm (GroupNorm, groups == C)
COLNORM_SHAPES = [(2, 1, 3), (3, 63, 5), (2, 64, 257), (2, 65, 64), (1, 300, 512), (1, 16500, 8), (1, 480000, 1)]
COLNORM_RATIOS = (30.0, 100.0, 1000.0)


def colnorm_eps(shape):
    return 1e-7 if shape[2] == 1 else 1e-5      # C == 1 is the waveform normaliser (eps 1e-7)


def colnorm_ratios(shape):
    """mean / std of every (b, c) column of the offset input: the three ratios cycle over the columns (rotated per batch entry), so every
    shape with three columns or more carries 30, 100 and 1000 at once; the one-column waveform shape carries 100."""
    B, T, C = shape
    if C == 1:
        return torch.full((B, 1), 100.0)
    idx = (torch.arange(C)[None, :] + torch.arange(B)[:, None]) % 3
    return torch.tensor(COLNORM_RATIOS)[idx]


def colnorm_inputs(shape, offset, seed=0):
    """x [B, T, C] fp32 (std `s` per column, plus ratio * s per column when `offset`), gamma, beta, dy — all fp32, seeded."""
    B, T, C = shape
    g = gen(1000 + seed + T + C)
    s = 0.01 if C == 1 else 1.0                 # waveform amplitude for the one-column shape
    x = torch.randn(B, T, C, generator=g) * s
    if offset:
        sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
        x = x + (colnorm_ratios(shape) * s * sign[None, :])[:, None, :]
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g)
    dy = torch.randn(B, T, C, generator=g)
    return x.float().contiguous(), gamma.float(), beta.float(), dy.float()


def colnorm_ref(x, gamma, beta, eps):
    """x [B, T, C]: per (b, c) mean and BIASED variance over T, two passes in float64.  Returns y, mean [B, C], rstd [B, C]."""
    x, gamma, beta = d(x), d(gamma), d(beta)
    mean = x.sum(1) / x.shape[1]
    var = ((x - mean[:, None]) ** 2).sum(1) / x.shape[1]
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    return y, mean, rstd


def colnorm_bwd_ref(x, gamma, dy, eps):
    """dx = rstd * gamma * (dy - mean_t(dy) - xhat * mean_t(dy * xhat)), dgamma = sum_{b,t} dy * xhat, dbeta = sum_{b,t} dy."""
    x, gamma, dy = d(x), d(gamma), d(dy)
    T = x.shape[1]
    mean = x.sum(1, keepdim=True) / T
    var = ((x - mean) ** 2).sum(1, keepdim=True) / T
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    s1 = dy.sum(1, keepdim=True) / T
    s2 = (dy * xh).sum(1, keepdim=True) / T
    dx = rstd * gamma * (dy - s1 - xh * s2)
    return dx, (dy * xh).sum((0, 1)), dy.sum((0, 1))


def colnorm_chunks(T):
    """chunks_for of csrc/wav2vec2.hip: at most 256 chunks of at least 64 rows.  Returns (chunks, rows per chunk)."""
    ch = min(max(-(-T // 64), 1), 256)
    per = -(-T // ch)
    return -(-T // per), per


def colnorm_unshifted_replay(x, eps):
    """The summation order the column norm had BEFORE its statistics were made stable, replayed on the CPU: per chunk fp32 running sums of
    x and x^2 in row order, the chunk sums added in double in chunk order, var = E[x^2] - mean^2 (biased, clamped at 0), mean and rstd
    rounded to fp32.  (The device contracts q += v * v into an fma, numpy does not: a difference of half an ulp per step, far below the
    cancellation this function exists to show.)  Returns xhat = (x - mean) * rstd in fp32 arithmetic, mean and rstd [B, C] fp32."""
    xn = x.detach().cpu().numpy().astype(np.float32)
    B, T, C = xn.shape
    chunks, per = colnorm_chunks(T)
    pad = np.zeros((B, chunks * per, C), np.float32)
    pad[:, :T] = xn
    pad = pad.reshape(B, chunks, per, C)
    s = np.zeros((B, chunks, C), np.float32)
    q = np.zeros((B, chunks, C), np.float32)
    for t in range(per):                         # zero rows past T add nothing, as the rows the kernel does not visit
        v = pad[:, :, t]
        s = (s + v).astype(np.float32)
        q = (q + (v * v).astype(np.float32)).astype(np.float32)
    sd, qd = np.zeros((B, C)), np.zeros((B, C))
    for ch in range(chunks):
        sd += s[:, ch].astype(np.float64)
        qd += q[:, ch].astype(np.float64)
    m = sd / T
    var = np.maximum(qd / T - m * m, 0.0)
    mean = m.astype(np.float32)
    rstd = (1.0 / np.sqrt(var + eps)).astype(np.float32)
    xhat = ((xn - mean[:, None]) * rstd[:, None]).astype(np.float32)
    return torch.from_numpy(xhat), torch.from_numpy(mean), torch.from_numpy(rstd)


def colnorm_torch_fp32(x, gamma, beta, eps):
    """torch's fp32 CPU GroupNorm (groups == channels) of the channels-last x: y [B, T, C], mean [B, C], rstd [B, C]."""
    B, T, C = x.shape
    y, mean, rstd = torch.native_group_norm(x.transpose(1, 2).contiguous(), gamma, beta, B, C, T, C, eps)
    return y.transpose(1, 2).contiguous(), mean.view(B, C), rstd.view(B, C)


# ----------------------------------------------------------------------------------------------------------- elementwise
GELU_EDGES = [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 10.0, -10.0]


def gelu_inputs(n, seed=0):
    g = gen(2000 + seed + n % 977)
    x = torch.randn(n, generator=g) * 3
    k = min(n, len(GELU_EDGES))
    x[:k] = torch.tensor(GELU_EDGES[:k])
    return x.float(), torch.randn(n, generator=g).float()


def gelu_ref(x):
    x = d(x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_bwd_ref(x, dy):
    x, dy = d(x), d(dy)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + x * pdf)


# ----------------------------------------------------------------------------------------------------------- weight norm (per tap)
def weight_norm_ref(v, g):
    """v [rows, kw, cg], g [kw]: w = g[j] * v / ||v[:, j, :]||_F."""
    v, g = d(v), d(g)
    n = torch.sqrt((v * v).sum((0, 2)))
    return g[None, :, None] * v / n[None, :, None]


def weight_norm_bwd_ref(v, g, dw):
    """dv = g / ||v_j|| * (dw - v <dw, v>_j / ||v_j||^2), dg[j] = <dw, v>_j / ||v_j||."""
    v, g, dw = d(v), d(g), d(dw)
    nn = (v * v).sum((0, 2))
    dot = (dw * v).sum((0, 2))
    dv = (g / torch.sqrt(nn))[None, :, None] * (dw - v * (dot / nn)[None, :, None])
    return dv, dot / torch.sqrt(nn)


# ----------------------------------------------------------------------------------------------------------- strided conv1d, channels-last
def conv1d_rows(x, kw, stride):
    """x [B, T, Cin] -> the overlapping rows [B, Tout, kw * Cin] (tap-major, then input channel) the implicit GEMM reads."""
    B, T, Cin = x.shape
    Tout = (T - kw) // stride + 1
    idx = torch.arange(Tout)[:, None] * stride + torch.arange(kw)[None, :]
    return x[:, idx].reshape(B, Tout, kw * Cin)


def conv1d_ref(x, w, kw, stride):
    """Valid strided conv: y[b, t, co] = sum_{j, ci} x[b, t * stride + j, ci] * w[co, j * Cin + ci]."""
    return conv1d_rows(d(x), kw, stride) @ d(w).T


def conv1d_wgrad_ref(x, dy, kw, stride):
    rows, dy = conv1d_rows(d(x), kw, stride), d(dy)
    return torch.einsum("bto,btk->ok", dy, rows)


def conv1d_dgrad_ref(dy, w, T, Cin, kw, stride):
    """dx[b, r, ci] = sum over (t, j) with t * stride + j == r of (dy[b, t] @ w)[j * Cin + ci]; rows no window covers stay 0."""
    dy, w = d(dy), d(w)
    B, Tout, _ = dy.shape
    dA = (dy @ w).view(B, Tout, kw, Cin)
    dx = torch.zeros(B, T, Cin, dtype=F64)
    for j in range(kw):
        dx[:, j:j + (Tout - 1) * stride + 1:stride] += dA[:, :, j]
    return dx


def torch_conv_weight(w, kw):
    """[Cout, kw * Cin] (tap-major) -> torch's [Cout, Cin, kw]."""
    return w.view(w.shape[0], kw, -1).permute(0, 2, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------- grouped positional conv layout
def group_pack_ref(x, G, pad):
    """[B, T, C] -> [B, G, T + 2 pad, C / G], zero padded in time."""
    B, T, C = x.shape
    xg = torch.zeros(B, G, T + 2 * pad, C // G, dtype=x.dtype)
    xg[:, :, pad:pad + T] = x.view(B, T, G, C // G).permute(0, 2, 1, 3)
    return xg


def group_unpack_ref(yg, bias, T, C):
    """[B, G, Tg, cg] -> [B, T, C] from the first T rows of every group (+ bias)."""
    B = yg.shape[0]
    y = yg[:, :, :T].permute(0, 2, 1, 3).reshape(B, T, C)
    return y if bias is None else y + bias


def group_pack_grad_ref(dy, G, Tg):
    B, T, C = dy.shape
    dyg = torch.zeros(B, G, Tg, C // G, dtype=dy.dtype)
    dyg[:, :, :T] = dy.view(B, T, G, C // G).permute(0, 2, 1, 3)
    return dyg


def group_unpack_grad_ref(dxg, dx, pad, beta):
    B, T, C = dx.shape
    v = dxg[:, :, pad:pad + T].permute(0, 2, 1, 3).reshape(B, T, C)
    return v + beta * dx if beta != 0.0 else v


def grouped_conv_ref(x, wg, bias, G, kw):
    """pack -> valid conv per group -> unpack of the first T frames: the `same`-padded grouped conv with an EVEN kernel whose last output
    frame is dropped.  x [B, T, C], wg [G, C/G (out), kw * C/G] tap-major."""
    x, wg = d(x), d(wg)
    B, T, C = x.shape
    xg = group_pack_ref(x, G, kw // 2)
    yg = torch.stack([conv1d_ref(xg[:, g], wg[g], kw, 1) for g in range(G)], 1)      # [B, G, T + 1, cg]
    return group_unpack_ref(yg, None if bias is None else d(bias), T, C)


def torch_grouped_weight(wg, kw):
    """[G, cg_out, kw * cg_in] -> torch's grouped layout [C, cg_in, kw]."""
    G, co, _ = wg.shape
    return wg.view(G * co, kw, -1).permute(0, 2, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------- row norms, channel affine
def layernorm_ref(x, gamma, beta, eps):
    x, gamma, beta = d(x), d(gamma), d(beta)
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).sum(-1, keepdim=True) / C + eps)
    return (x - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd_ref(x, gamma, dy, eps):
    x, gamma, dy = d(x), d(gamma), d(dy)
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).sum(-1, keepdim=True) / C + eps)
    xh = (x - mean) * rstd
    gy = dy * gamma
    dx = rstd * (gy - gy.sum(-1, keepdim=True) / C - xh * (gy * xh).sum(-1, keepdim=True) / C)
    return dx, (dy * xh).sum(0), dy.sum(0)


def rmsnorm_ref(x, gamma, eps):
    x, gamma = d(x), d(gamma)
    rstd = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + eps)
    return x * rstd * gamma, rstd.squeeze(-1)


def rmsnorm_bwd_ref(x, gamma, dy, eps):
    x, gamma, dy = d(x), d(gamma), d(dy)
    C = x.shape[-1]
    rstd = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / C + eps)
    gy = dy * gamma
    dx = rstd * gy - x * rstd ** 3 * (gy * x).sum(-1, keepdim=True) / C
    return dx, (dy * x * rstd).sum(0)


def chanaffine_ref(x, mean, var, weight, bias, eps):
    x, mean, var, weight = d(x), d(mean), d(var), d(weight)
    y = (x - mean) / torch.sqrt(var + eps) * weight
    return y if bias is None else y + d(bias)


def chanaffine_bwd_ref(x, mean, var, weight, dy, eps):
    """dx = dy * weight / sqrt(var + eps), dweight = sum_r dy * xhat, dbias = sum_r dy."""
    x, mean, var, weight, dy = d(x), d(mean), d(var), d(weight), d(dy)
    rs = 1.0 / torch.sqrt(var + eps)
    return dy * rs * weight, (dy * (x - mean) * rs).sum(0), dy.sum(0)


# ----------------------------------------------------------------------------------------------------------- softmax, entropy
def masked_softmax_ref(x, valid):
    """Row softmax over the first `valid` columns; the columns past them are exactly 0."""
    x = d(x)
    e = torch.exp(x[:, :valid] - x[:, :valid].max(-1, keepdim=True).values)
    y = torch.zeros_like(x)
    y[:, :valid] = e / e.sum(-1, keepdim=True)
    return y


def entropy_grad_expr(y, scale):
    """entropy_grad_ref's expression where `y` lives and in its dtype (see "the row softmax family" below)."""
    p = torch.exp(y)
    H = -(p * y).sum(-1)
    return -p * (y + H[:, None]) * scale, H


def entropy_grad_ref(logp, scale):
    """H_r = -sum_c p log p with p = exp(logp), logp normalised rows; the gradient of scale * sum_r H_r w.r.t. the LOGITS behind them
    (the simplex projection included): -p (logp + H_r) * scale.  Returns (grad, H)."""
    return entropy_grad_expr(d(logp), scale)


# ----------------------------------------------------------------------------------------------------------- the row softmax family
# csrc/softmax_row.h and the kernels built on it (softmax.hip, relshift.hip, relbias.hip), from the definitions.  Unlike the functions above
# these stay on the device and in the dtype of their operands: tests/test_row_kernels_gpu.py evaluates each one twice on the GPU, in float64
# (the reference; the square cases are too large for the CPU) and in float32 (torch's own fp32 result of the same expression: measured_tol).
def clamped_valid(valid, L):
    """The key length the kernels use for a device-side `valid` (valid_len of csrc/softmax_row.h): clamped into [1, L]; None is L."""
    return L if valid is None else min(max(int(valid), 1), L)


def row_softmax_ref(x, valid=None):
    """softmax over the first clamped_valid(valid, L) columns of the last axis; the columns past them are exactly 0."""
    Lv = clamped_valid(valid, x.shape[-1])
    xv = x[..., :Lv]
    e = torch.exp(xv - xv.max(-1, keepdim=True).values)
    y = torch.zeros_like(x)
    y[..., :Lv] = e / e.sum(-1, keepdim=True)
    return y


def row_log_softmax_ref(x, valid=None):
    """log-softmax over the first clamped_valid(valid, L) columns; the columns past them are -inf."""
    Lv = clamped_valid(valid, x.shape[-1])
    xv = x[..., :Lv]
    m = xv.max(-1, keepdim=True).values
    y = torch.full_like(x, -math.inf)
    y[..., :Lv] = xv - (m + torch.log(torch.exp(xv - m).sum(-1, keepdim=True)))
    return y


def softmax_bwd_ref(y, dy, scale=1.0):
    """dx = y * (dy - sum(dy * y)) * scale from the probabilities y."""
    return y * (dy - (dy * y).sum(-1, keepdim=True)) * scale


def log_softmax_bwd_ref(y, dy):
    """dx = dy - exp(y) * sum(dy) from the log-probabilities y."""
    return dy - torch.exp(y) * dy.sum(-1, keepdim=True)


def shift_pad_view_slice(bd):
    """transformers' pad / view / slice (_apply_relative_embeddings, step 5) restated: [B, nh, T, 2T - 1] -> [B, nh, T, T]."""
    B, nh, T, R = bd.shape
    padded = torch.cat([torch.zeros(B, nh, T, 1, dtype=bd.dtype, device=bd.device), bd], dim=-1).view(B, nh, R + 1, T)
    return padded[:, :, 1:].view_as(bd)[..., :R // 2 + 1]


def relshift_index(T, device=None):
    """[T, T] int64: the column T - 1 - i + j of BD's row i that key j of query i reads."""
    return T - 1 - torch.arange(T, device=device)[:, None] + torch.arange(T, device=device)[None, :]


def relshift_scores_ref(S, BD):
    """S [B, nh, T, T] + BD[b, h, i, T - 1 - i + j] by gather; BD [B, nh, T, ld >= 2T - 1], columns past 2T - 1 are never read."""
    T = S.shape[-1]
    return S + BD.gather(-1, relshift_index(T, S.device).expand(S.shape))


def relshift_bwd_ref(dS, ld):
    """dBD [B, nh, T, ld]: dS[b, h, i, j] at column T - 1 - i + j of row i, zeros everywhere else (a copy: exact in any dtype)."""
    T = dS.shape[-1]
    out = torch.zeros(*dS.shape[:-1], ld, dtype=dS.dtype, device=dS.device)
    return out.scatter_(-1, relshift_index(T, dS.device).expand(dS.shape), dS)


def bias_ref(gate, E, table, T, Tmax):
    """gate[b, head, t] * E[bucket(s - t), head] as [B, nh, T, T] (the restatement the WavLM tests differentiate)."""
    dev = gate.device
    idx = torch.arange(T, device=dev)[None, :] - torch.arange(T, device=dev)[:, None] + Tmax - 1                # [t, s]
    return gate.unsqueeze(-1) * E[table.to(dev).long()[idx]].permute(2, 0, 1).unsqueeze(0)


def relbias_buckets(table, T, Tmax):
    """[T, T] int64: bucket[i, j] = table[j - i + Tmax - 1], table [2 Tmax - 1]."""
    ar = torch.arange(T, device=table.device)
    return table.long()[ar[None, :] - ar[:, None] + Tmax - 1]


def relbias_scores_ref(S, gate, E, table, Tmax):
    """S[b, h, i, j] + gate[b, h, i] * E[table[j - i + Tmax - 1], h]; S [B, nh, T, T], gate [B, nh, T], E [num_buckets, nh]."""
    T = S.shape[-1]
    return S + gate[..., None] * E.t()[:, relbias_buckets(table, T, Tmax)][None]


def relbias_bwd_ref(dS, gate, E, table, Tmax):
    """Gradients of sum(dS * gate * E[bucket]) : dgate[b, h, i] = sum_j dS[b, h, i, j] * E[bucket[i, j], h] (the row dot product);
    dE[k, h] = sum over b and the (i, j) of bucket k of gate * dS (an index_add_ over buckets).  Returns (dgate, dE)."""
    B, nh, T, _ = dS.shape
    bucket = relbias_buckets(table, T, Tmax)
    dgate = (dS * E.t()[:, bucket][None]).sum(-1)
    per_pair = (gate[..., None] * dS).sum(0).permute(1, 2, 0).reshape(T * T, nh)
    dE = torch.zeros_like(E).index_add_(0, bucket.reshape(-1), per_pair)
    return dgate, dE


def relbias_fullest_bucket(table, T, Tmax, B):
    """The largest number of products one bucket of dE sums: distance d occurs B (T - |d|) times (as tests/test_wavlm_gpu.py counts it)."""
    dist = torch.arange(-(T - 1), T)
    counts = torch.zeros(int(table.max()) + 1, dtype=torch.long)
    return int(counts.index_add_(0, table.cpu().long()[dist + Tmax - 1], B * (T - dist.abs())).max())


# ----------------------------------------------------------------------------------------------------------- encoder-decoder pieces
def embedding_ref(ids, table, pos, pos_period):
    """out[s] = table[ids[s]] (+ pos[s % pos_period])."""
    out = d(table)[ids.long()]
    if pos is not None:
        out = out + d(pos)[torch.arange(ids.numel()) % pos_period]
    return out


def embedding_bwd_ref(ids, dy, old, beta):
    """dtable[v] = beta * old[v] + sum_{s: ids[s] == v} dy[s]."""
    out = beta * d(old) if beta != 0.0 else torch.zeros_like(d(old))
    for s in range(ids.numel()):
        out[int(ids[s])] += d(dy)[s]
    return out


def causal_mask_ref(scores):
    """[nb, S, S]: entries with column > row become -inf, the rest keep their bits."""
    S = scores.shape[-1]
    out = scores.clone()
    out[:, torch.arange(S)[None, :] > torch.arange(S)[:, None]] = -math.inf
    return out


def nll_ref(logp, targets, ignore_index, scale, weights=None):
    """row_loss[r] = -w_r logp[r, t_r], loss = sum, grad = w_r * scale * (exp(logp[r]) - onehot(t_r)) w.r.t. the logits; a row whose target
    is `ignore_index` or outside [0, C) contributes 0 loss and a zero gradient row."""
    y = d(logp)
    rows, C = y.shape
    w = torch.ones(rows, dtype=F64) if weights is None else d(weights)
    row_loss = torch.zeros(rows, dtype=F64)
    grad = torch.zeros_like(y)
    for r in range(rows):
        t = int(targets[r])
        if t == ignore_index or t < 0 or t >= C:
            continue
        row_loss[r] = -w[r] * y[r, t]
        grad[r] = w[r] * scale * torch.exp(y[r])
        grad[r, t] -= w[r] * scale
    return row_loss.sum(), row_loss, grad


def stitch_finalize_rows_ref(acc, count, row_index):
    return torch.log(d(acc)[row_index.cpu()] / d(count)[row_index.cpu()][:, None])


# ----------------------------------------------------------------------------------------------------------- conformer convolutions
# csrc/conv.hip and csrc/convmod.hip from the definitions, by index gathers.  Dtype- and device-agnostic: the result has the dtype of the
# operands (tests/test_conv_kernels_gpu.py passes float64 copies; tests/test_kernel_refs_cpu.py holds every function to torch's conv1d /
# conv2d / layer_norm / silu and autograd in float64).  Activations are channels-last, filters [C, KW] and [C, 3, 3].
def sigmoid_expr(x):
    return 1.0 / (1.0 + torch.exp(-x))


def silu_expr(x):
    return x * sigmoid_expr(x)


def silu_grad_expr(x):
    s = sigmoid_expr(x)
    return s * (1.0 + x * (1.0 - s))


def dwconv1d_windows(x, KW):
    """x [B, T, C] -> [B, T, KW, C]: window[b, t, j, c] = x[b, t + j - P, c] with P = (KW - 1) / 2, zeros outside [0, T) ('same')."""
    B, T, C = x.shape
    P = (KW - 1) // 2
    xp = torch.zeros(B, T + 2 * P, C, dtype=x.dtype, device=x.device)
    xp[:, P:P + T] = x
    idx = torch.arange(T, device=x.device)[:, None] + torch.arange(KW, device=x.device)[None, :]
    return xp[:, idx]


def dwconv1d_ref(x, w, bias=None):
    """y[b, t, c] = bias[c] + sum_j w[c, j] * x[b, t + j - P, c]."""
    y = (dwconv1d_windows(x, w.shape[1]) * w.t()[None, None]).sum(2)
    return y if bias is None else y + bias


def dwconv1d_dgrad_ref(dy, w):
    """dx[b, t, c] = sum_j w[c, j] * dy[b, t - j + P, c]: the same windows read with the taps reversed."""
    KW = w.shape[1]
    rev = w[:, torch.arange(KW - 1, -1, -1, device=w.device)]
    return (dwconv1d_windows(dy, KW) * rev.t()[None, None]).sum(2)


def dwconv1d_wgrad_ref(x, dy, KW):
    """dw[c, j] = sum_{b, t} dy[b, t, c] * x[b, t + j - P, c]  [C, KW];  dbias[c] = sum_{b, t} dy[b, t, c]."""
    dw = (dwconv1d_windows(x, KW) * dy[:, :, None, :]).sum((0, 1)).t()
    return dw, dy.sum((0, 1))


def group_samples(B, R, r):
    """The samples of replica r in a lockstep batch ordered sample = chunk * R + replica."""
    return torch.arange(r, B, R)


def dwconv1d_dgrad_group_ref(dy, w):
    """w [R, C, KW]: sample b is convolved with the filters of replica b % R."""
    R = w.shape[0]
    return torch.stack([dwconv1d_dgrad_ref(dy[b:b + 1], w[b % R])[0] for b in range(dy.shape[0])])


def dwconv1d_wgrad_group_ref(x, dy, old_w, old_b, beta):
    """old_w [R, C, KW], old_b [R, C]: replica r's gradient is beta * old + the sum over the samples b = r (mod R)."""
    R, _, KW = old_w.shape
    dws, dbs = [], []
    for r in range(R):
        sel = group_samples(x.shape[0], R, r).to(x.device)
        dw, db = dwconv1d_wgrad_ref(x[sel], dy[sel], KW)
        dws.append(dw + beta * old_w[r] if beta != 0.0 else dw)
        dbs.append(db + beta * old_b[r] if beta != 0.0 else db)
    return torch.stack(dws), torch.stack(dbs)


def s2_out_len(n):
    """Output length of a 3-wide, stride-2, pad-1 convolution."""
    return (n - 1) // 2 + 1


def s2_patches(a):
    """a [B, T, F, ...] -> [B, To, 3, Fo, 3, ...]: patch[b, to, dt, fo, df] = a[b, 2 to + dt - 1, 2 fo + df - 1], zeros outside the input."""
    B, T, Fq = a.shape[:3]
    To, Fo = s2_out_len(T), s2_out_len(Fq)
    ap = torch.zeros(B, 2 * To + 1, 2 * Fo + 1, *a.shape[3:], dtype=a.dtype, device=a.device)
    ap[:, 1:T + 1, 1:Fq + 1] = a
    ti = 2 * torch.arange(To, device=a.device)[:, None] + torch.arange(3, device=a.device)[None, :]
    fi = 2 * torch.arange(Fo, device=a.device)[:, None] + torch.arange(3, device=a.device)[None, :]
    return ap[:, ti][:, :, :, fi]


def s2_scatter(contrib, T, Fq):
    """The adjoint of s2_patches: contrib [B, To, 3, Fo, 3, ...] -> [B, T, F, ...], every patch element added back where it was read."""
    B, To, _, Fo = contrib.shape[:4]
    out = torch.zeros(B, 2 * To + 1, 2 * Fo + 1, *contrib.shape[5:], dtype=contrib.dtype, device=contrib.device)
    for dt in range(3):
        for df in range(3):
            out[:, dt:dt + 2 * To:2, df:df + 2 * Fo:2] += contrib[:, :, dt, :, df]
    return out[:, 1:T + 1, 1:Fq + 1]


def conv2d_first_ref(x, w, bias):
    """x [B, T, F] (one input channel), w [C, 3, 3] -> z[b, to, fo, c] = bias[c] + sum_{dt, df} w[c, dt, df] * x[b, 2 to + dt - 1, 2 fo + df - 1]."""
    return torch.einsum("btifj,cij->btfc", s2_patches(x), w) + bias


def conv2d_first_dgrad_ref(dz, w, T, Fq):
    """dx[b, t, f] = sum_c sum over the (to, dt), (fo, df) that read (t, f) of w[c, dt, df] * dz[b, to, fo, c]."""
    return s2_scatter(torch.einsum("btfc,cij->btifj", dz, w), T, Fq)


def conv2d_first_wgrad_ref(x, dz):
    """dw [C, 3, 3], dbias [C]."""
    return torch.einsum("btfc,btifj->cij", dz, s2_patches(x)), dz.sum((0, 1, 2))


def dwconv2d_s2_ref(z, w, bias):
    """z [B, T, F, C] -> u[b, to, fo, c] = bias[c] + sum_{dt, df} w[c, dt, df] * silu(z[b, 2 to + dt - 1, 2 fo + df - 1, c])."""
    return torch.einsum("btifjc,cij->btfc", s2_patches(silu_expr(z)), w) + bias


def dwconv2d_s2_dgrad_ref(z, w, du):
    """dz = silu'(z) * (the depthwise transposed conv of du)."""
    B, T, Fq, C = z.shape
    return s2_scatter(torch.einsum("btfc,cij->btifjc", du, w), T, Fq) * silu_grad_expr(z)


def dwconv2d_s2_wgrad_ref(z, du):
    return torch.einsum("btfc,btifjc->cij", du, s2_patches(silu_expr(z))), du.sum((0, 1, 2))


def sub12_ref(x, w1, b1, w2, b2):
    """The first two subsampling stages: dw3x3_s2(silu(conv3x3_s2(x)))."""
    return dwconv2d_s2_ref(conv2d_first_ref(x, w1, b1), w2, b2)


def sub12_bwd_ref(x, du2, w1, b1, w2):
    """(dw1, db1, dw2, db2) of sub12_ref given du2."""
    z1 = conv2d_first_ref(x, w1, b1)
    dw2, db2 = dwconv2d_s2_wgrad_ref(z1, du2)
    dw1, db1 = conv2d_first_wgrad_ref(x, dwconv2d_s2_dgrad_ref(z1, w2, du2))
    return dw1, db1, dw2, db2


def convmod_ref(u, w, bias, gamma, beta, layernorm, eps):
    """The fused conv-module core: u [B, T, 2C] -> GLU -> depthwise conv (w [C, 9], 'same', optional bias) -> LayerNorm (optional beta) or
    RMSNorm over the channels -> SiLU.  Returns (s, g, c, nn, mean, rstd): the output, the GLU output, the conv output, the norm output, and
    the per-frame statistics flattened to [B * T] (mean is None for RMSNorm)."""
    C = u.shape[-1] // 2
    g = u[..., :C] * sigmoid_expr(u[..., C:])
    c = dwconv1d_ref(g, w, bias)
    if layernorm:
        mean = c.sum(-1, keepdim=True) / C
        rstd = 1.0 / torch.sqrt(((c - mean) ** 2).sum(-1, keepdim=True) / C + eps)
        nn = (c - mean) * rstd * gamma
        if beta is not None:
            nn = nn + beta
        mean = mean.reshape(-1)
    else:
        mean = None
        rstd = 1.0 / torch.sqrt((c * c).sum(-1, keepdim=True) / C + eps)
        nn = c * rstd * gamma
    return silu_expr(nn), g, c, nn, mean, rstd.reshape(-1)


def convmod_group_ref(u, w, bias, gamma, beta, layernorm, eps):
    """Parameters [R, ...]: sample b takes replica b % R's.  Same tuple as convmod_ref."""
    R = w.shape[0]
    per = [convmod_ref(u[b:b + 1], w[b % R], None if bias is None else bias[b % R], gamma[b % R], None if beta is None else beta[b % R],
                       layernorm, eps) for b in range(u.shape[0])]
    return tuple(None if per[0][i] is None else torch.cat([p[i] for p in per]) for i in range(6))


# ----------------------------------------------------------------------------------------------------------- log-mel front end, window augmentations
# csrc/logmel.hip and csrc/augment.hip from the definitions (tests/test_frontend_kernels_gpu.py), and a CPU replay of the summation order
# dyn_logmel_finish had before its per-bin statistics were centred.
LOGMEL_EPS = 1e-6
LOGMEL_NORM_T = (2, 101, 801, 6001, 60001)
LOGMEL_CLASSES = ((-13.8, 1e-3), (-13.8, 1e-2), (-10.0, 0.05), (-9.0, 0.3), (-5.0, 2.0), (4.0, 1.0))      # (mu, sd) of log(mel + eps)
LOGMEL_ZERO_COLUMN = 79                          # this column of logmel_class_inputs is all zeros (an empty band)


def reflect_pad_ref(x, pad):
    """out[i] = x[|i - pad|] folded back at n - 1: torch.stft's center=True, pad_mode='reflect' (needs pad < n)."""
    n = x.numel()
    j = (torch.arange(n + 2 * pad) - pad).abs()
    return x[torch.where(j >= n, 2 * (n - 1) - j, j)]


def stft_power_ref(reim, KP):
    """reim [T, 2 KP] (re | im) -> re^2 + im^2 [T, KP]."""
    r = d(reim)
    return r[:, :KP] ** 2 + r[:, KP:2 * KP] ** 2


def centred_stats(x):
    """Mean and centred sum of squares over the last axis, two passes.  The mean is taken about the first element (x0 + mean(x - x0)),
    so a constant row has mean x0 and a centred sum of squares of 0, exactly."""
    x0 = x[..., :1]
    mean = x0 + (x - x0).sum(-1, keepdim=True) / x.shape[-1]
    return mean, ((x - mean) ** 2).sum(-1, keepdim=True)


def logmel_finish_ref(mel32, eps, normalize):
    """mel [T, F] fp32 -> log(double(mel) + double(float32(eps))) as [F, T]; `normalize`: per bin (x - mean) / unbiased std over T.  A bin
    whose centred variance is exactly 0, and T == 1, give zeros (dyn_logmel_finish's deliberate behaviour; the formula gives nan)."""
    x = torch.log(d(mel32) + float(np.float32(eps))).t().contiguous()
    if not normalize:
        return x
    T = x.shape[1]
    mean, m2 = centred_stats(x)
    var = m2 / max(T - 1, 1)
    return torch.where(var > 0, (x - mean) / torch.sqrt(torch.where(var > 0, var, torch.ones_like(var))), torch.zeros_like(x))


def rownorm_ref(x):
    """x [R, T]: (x - mean) / unbiased std per row, two passes."""
    x = d(x)
    mean, m2 = centred_stats(x)
    return (x - mean) / torch.sqrt(m2 / (x.shape[-1] - 1))


def moments_ref(x):
    """(sum, mean, unbiased std) of every element, as Python floats; the std of one element is 0."""
    x = d(x).reshape(-1)
    n = x.numel()
    mean, m2 = centred_stats(x)
    return x.sum().item(), mean.item(), math.sqrt(m2.item() / (n - 1)) if n > 1 else 0.0


def cutout_winner(shape, rects):
    """[F, T] int64: the index of the LAST rectangle (y0, y1, x0, x1) covering each cell, -1 where none does."""
    F_, T = shape
    f, t = torch.arange(F_)[:, None], torch.arange(T)[None, :]
    win = torch.full((F_, T), -1, dtype=torch.long)
    for k, (y0, y1, x0, x1) in enumerate(rects):
        win = torch.where((f >= y0) & (f < y1) & (t >= x0) & (t < x1), torch.full_like(win, k), win)
    return win


def cutout_ref(x, rects, mode, value=0.0):
    """x [F, T]; mode 0: zero, 1: every rectangle's own mean (all means taken from x before any fill), 2: `value`; later rectangles
    overwrite earlier ones.  Returns (out float64, winner [F, T], means [n_rects] float64 — 0 for an empty rectangle)."""
    x = d(x)
    win = cutout_winner(tuple(x.shape), rects)
    means = torch.zeros(len(rects), dtype=F64)
    for k, (y0, y1, x0, x1) in enumerate(rects):
        if y1 > y0 and x1 > x0:
            means[k] = x[y0:y1, x0:x1].sum() / ((y1 - y0) * (x1 - x0))
    fill = means if mode == 1 else torch.full((len(rects),), float(value) if mode == 2 else 0.0, dtype=F64)
    out = x.clone()
    if len(rects):
        out = torch.where(win >= 0, fill[win.clamp(min=0)], x)
    return out, win, means


def gather_frames_ref(x, index, along_time):
    """y[f, t] = x[f, index[t]] (along_time) or x[index[f], t]."""
    return x[:, index.long()] if along_time else x[index.long()]


def logmel_class_inputs(T, F_=80, seed=0):
    """mel [T, F] fp32 whose column f has log(mel + eps) ~ mu + sd * randn with (mu, sd) = LOGMEL_CLASSES[f % 6]: mel = exp(mu + sd z) - eps,
    clamped at 0.  Column LOGMEL_ZERO_COLUMN is all zeros.  The two (-13.8, .) classes sit at log(1e-6): a bin whose band is empty."""
    z = torch.randn(T, F_, generator=gen(7000 + seed + T), dtype=F64)
    mu = torch.tensor([LOGMEL_CLASSES[f % len(LOGMEL_CLASSES)][0] for f in range(F_)], dtype=F64)
    sd = torch.tensor([LOGMEL_CLASSES[f % len(LOGMEL_CLASSES)][1] for f in range(F_)], dtype=F64)
    mel = (torch.exp(mu + sd * z) - LOGMEL_EPS).clamp(min=0.0)
    mel[:, LOGMEL_ZERO_COLUMN] = 0.0
    return mel.float().contiguous()


def logmel_torch_fp32(mel32, eps, normalize):
    """torch's fp32 CPU chain of the same op: log, then mean and std (torch's own two-pass) per bin.  [F, T] fp32."""
    x = torch.log(mel32 + torch.tensor(eps, dtype=torch.float32)).t().contiguous()
    return (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True) if normalize else x


def logmel_log_unit_err(out, ref64, std64):
    """max |out - ref| * std_f: the error of a normalised [F, T] output in log-mel units (tests/test_frontend_gpu.py's metric)."""
    return ((d(out) - ref64).abs() * std64).max().item()


def unit_stats_err(out, cols):
    """(max |mean|, max |std - 1|) over the rows `cols` of a normalised [F, T] output, mean and unbiased std taken in float64."""
    o = d(out)[cols]
    return o.mean(-1).abs().max().item(), (o.std(-1) - 1).abs().max().item()


def normalise_fp32(x32):
    """torch's fp32 CPU (x - mean) / std over the last axis (torch's own two-pass mean and unbiased std); a constant row, where torch gives
    nan, is set to 0 (the kernels' zeros there are pinned separately)."""
    x32 = x32.detach().cpu().float()
    t32 = (x32 - x32.mean(-1, keepdim=True)) / x32.std(-1, keepdim=True)
    return torch.where(torch.isfinite(t32), t32, torch.zeros_like(t32))


def logmel_norm_bounds(mel32, eps=LOGMEL_EPS):
    """The bounds dyn_logmel_finish's normalised output of mel [T, F] is held to: torch's fp32 chain (fp32 log, mean, std) measured against
    logmel_finish_ref.  Returns a dict: `ref` [F, T] float64, `std` [F, 1] float64 (per-bin unbiased std of the float64 log-mel), `live`
    (the bins of non-zero variance) and the (bound, torch's error) pairs `out` (|out - ref| * std: log-mel units, floor 2e-6), `mean` and
    `unit_std` (per-bin mean 0 and std 1 of the output, floors 1e-5)."""
    lm = logmel_finish_ref(mel32, eps, False)
    std = torch.sqrt(centred_stats(lm)[1] / max(lm.shape[1] - 1, 1))
    ref = logmel_finish_ref(mel32, eps, True)
    live = [f for f in range(lm.shape[0]) if std[f, 0] > 0]
    t32 = normalise_fp32(logmel_torch_fp32(mel32, eps, False))
    e_m, e_s = unit_stats_err(t32, live)
    return dict(ref=ref, std=std, live=live, out=measured_tol(t32 * std, ref * std, 2e-6), mean=(4.0 * e_m + 1e-5, e_m),
                unit_std=(4.0 * e_s + 1e-5, e_s))


def logmel_uncentred_replay(logvals32):
    """The per-bin statistics dyn_logmel_finish formed BEFORE they were centred, replayed on the CPU from the fp32 log values [T, F]:
    per 256-row block 256 // F row lanes (3 for F = 80; lane l takes rows l, l + lanes, ...) of fp32 running (sum, sum of squares), the lanes
    added in order; the block partials added by 16 lanes of stride 16 in fp32, the lanes added in order; then mean = s / T and
    var = (q - s * mean) / (T - 1) in double.  (The device contracts q += v * v into an fma, numpy does not: half an ulp per step, far below
    the cancellation this shows.)  Returns (mean [F], var [F]) float64; the kernel replaced var <= 0 by 1."""
    x = logvals32.detach().cpu().numpy().astype(np.float32)
    T, F_ = x.shape
    lanes = 256 // F_
    nb = -(-T // 256)
    per = -(-256 // lanes)                        # rows a lane visits in a full block
    pad = np.zeros((nb, per * lanes, F_), np.float32)       # zero rows add nothing to either sum, as the rows past T the kernel skips
    pad.reshape(nb, per * lanes * F_)[:, :256 * F_] = np.pad(x, ((0, nb * 256 - T), (0, 0))).reshape(nb, 256 * F_)
    pad = pad.reshape(nb, per, lanes, F_)
    s = np.zeros((nb, lanes, F_), np.float32)
    q = np.zeros((nb, lanes, F_), np.float32)
    for i in range(per):
        v = pad[:, i]
        s = (s + v).astype(np.float32)
        q = (q + (v * v).astype(np.float32)).astype(np.float32)
    bs, bq = np.zeros((nb, F_), np.float32), np.zeros((nb, F_), np.float32)
    for k in range(lanes):
        bs = (bs + s[:, k]).astype(np.float32)
        bq = (bq + q[:, k]).astype(np.float32)
    ls, lq = np.zeros((16, F_), np.float32), np.zeros((16, F_), np.float32)
    for b in range(nb):
        ls[b % 16] = (ls[b % 16] + bs[b]).astype(np.float32)
        lq[b % 16] = (lq[b % 16] + bq[b]).astype(np.float32)
    ts, tq = np.zeros(F_, np.float32), np.zeros(F_, np.float32)
    for k in range(16):
        ts = (ts + ls[k]).astype(np.float32)
        tq = (tq + lq[k]).astype(np.float32)
    sd_, qd = ts.astype(np.float64), tq.astype(np.float64)
    mean = sd_ / T
    var = (qd - sd_ * mean) / (T - 1) if T > 1 else np.ones(F_)
    return torch.from_numpy(mean), torch.from_numpy(var)


# ----------------------------------------------------------------------------------------------------------- fused streaming attention
# csrc/attention.hip from the definitions (tests/test_attention_kernels_gpu.py): q, k, v [B, H, T, D], one softmax row per query.  The
# references return float64 on the CPU; attention_torch_fp32 is torch's own fp32 evaluation of the same expression (measured_tol).  Also
# here: the view of a strided [B, T, .] buffer as [B, H, T, D], and the generators of the cases whose construction carries an assertion.
ATTN_D = 128


def heads_view(flat, offset, B, T, H, row_stride, batch_stride, D=ATTN_D):
    """The [B, H, T, D] view of a flat buffer in the layout the C-ABI addresses: element (b, h, t, d) at
    offset + b * batch_stride + t * row_stride + h * D + d (floats).  Writes through the view land in the buffer."""
    return torch.as_strided(flat, (B, H, T, D), (batch_stride, D, row_stride, 1), offset)


def attention_ref(q, k, v, scale):
    """out = softmax(scale * q k^T) v and lse = log sum_j exp(scale * q k_j), the row maximum taken out first.  Returns (out, lse [B, H, T])."""
    q, k, v = d(q), d(k), d(v)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return (e / l) @ v, (m + torch.log(l)).squeeze(-1)


def attention_bwd_ref(q, k, v, out, dout, scale):
    """P = exp(s - lse), delta = sum_d dO o O (from the `out` it is handed, as the kernel does), dS = P o (dO V^T - delta),
    dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.  Returns (dq, dk, dv, delta [B, H, T])."""
    q, k, v, out, dout = d(q), d(k), d(v), d(out), d(dout)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
    p = torch.exp(s - lse)
    delta = (dout * out).sum(-1, keepdim=True)
    ds = p * (dout @ v.transpose(-1, -2) - delta)
    return scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ dout, delta.squeeze(-1)


def attention_cancellation_bound(q, k, v, out, dout, scale):
    """What dQ and dK may be off by where the exact gradient vanishes.  The backward forms dS = P o (dP - delta) from two separately
    rounded fp32 sums of D products, dP_ij = sum_d dO_id V_jd and delta_i = sum_d dO_id O_id (that is its interface: delta is an output,
    taken from `out`).  Where a row attends to one key alone (T = 1 always: P = 1, O = V, dP = delta and dQ = dK = 0 identically) torch's
    softmax backward returns exactly 0 and 2e-5 * max|grad| is no bound at all, while the two sums, accumulated in different orders, differ
    by their rounding.  An fp32 sum of D signed terms accumulated in any order: every addition rounds by at most u = 2^-24 of a partial sum,
    partial sums of random sign grow like sqrt(n) * rms term, so the errors add up (in quadrature) to about u * D * rms / sqrt(2), which is
    0.5 to 0.9 u * sum_d |term| — the rigorous worst case is D u sum |term| (Higham, Accuracy and Stability, (3.5)), 128 times more and
    never seen.  Allowing 2 u sum |term| per sum (the largest of many elements, not the rms):
        E_ij = 2 u (sum_d |dO_id V_jd| + sum_d |dO_id O_id|),  |err dQ_i| <= scale sum_j P_ij E_ij |K_j|,  |err dK_j| <= scale sum_i P_ij E_ij |Q_i|.
    Returns (bound on dQ, bound on dK) as floats: the largest element of each.  Used for T = 1 only; every other shape keeps the
    floor relative to its gradient."""
    q, k, v, out, dout = d(q), d(k), d(v), d(out), d(dout)
    s = (q @ k.transpose(-1, -2)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    pe = p * (2.0 * 2.0 ** -24 * (dout.abs() @ v.abs().transpose(-1, -2) + (dout.abs() * out.abs()).sum(-1, keepdim=True)))
    return (scale * (pe @ k.abs())).max().item(), (scale * (pe.transpose(-1, -2) @ q.abs())).max().item()


def attention_torch_fp32(q, k, v, scale, dout=None):
    """torch's fp32 CPU evaluation: softmax / logsumexp of (q k^T) * scale, and with `dout` fp32 autograd of it.
    Returns (out, lse) or (out, lse, dq, dk, dv)."""
    q, k, v = (t.detach().cpu().float().clone().requires_grad_(dout is not None) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    out = torch.softmax(s, -1) @ v
    lse = torch.logsumexp(s, -1).detach()
    if dout is None:
        return out, lse
    out.backward(dout.detach().cpu().float())
    return out.detach(), lse, q.grad, k.grad, v.grad


def attention_inputs(B, H, T, seed, kind="plain", step=0.5, scale=1.0 / math.sqrt(ATTN_D)):
    """q, k, v, dout [B, H, T, D] fp32, O(1) and seeded.  `kind`: "plain"; "peaky": q rows * 8 (one key takes most of a row, as after
    rotary and training); "rising" / "falling": dimension 0 of q is the constant 1 / scale and dimension 0 of k a ramp of `step` per key,
    so every score carries + step * j (rising: the running maximum rises on every key tile) or - step * j (falling: it never rises after
    the first tile) on top of the O(1) rest."""
    g = gen(9000 + seed + 7 * T)
    q, k, v, dout = (torch.randn(B, H, T, ATTN_D, generator=g) for _ in range(4))
    if kind == "peaky":
        q = q * 8
    elif kind in ("rising", "falling"):
        q[..., 0] = 1.0 / scale
        k[..., 0] = torch.arange(T, dtype=torch.float32) * (step if kind == "rising" else -step)
    else:
        assert kind == "plain", kind
    return q.contiguous(), k.contiguous(), v.contiguous(), dout.contiguous()


ATTN_ROUTING_SEED = 11
ATTN_ROUTING_GAIN = 400.0
ATTN_ROUTING_GAP = 120.0


def attention_routing_inputs(B, H, T, seed=ATTN_ROUTING_SEED):
    """Exact routing: k rows of unit length, q_i = 400 k_pi(i) for a seeded permutation pi per (b, h), scale = 1.  Query i's score with key
    pi(i) is 400 |k|^2 and every other one 400 cos, so far below that its exp is exactly 0 in fp32 (exp(-104) is below the smallest
    denormal): the output row i is the row pi(i) of v, bit for bit, and lse the winning score.  Asserts, in float64, that the gap between
    the best and the second-best score of every row exceeds ATTN_ROUTING_GAP and that the best is pi's.
    Returns (q, k, v, pi [B, H, T] int64, winning score [B, H, T] float64)."""
    g = gen(9500 + seed + T)
    k = torch.randn(B, H, T, ATTN_D, generator=g, dtype=F64)
    k = (k / torch.sqrt((k * k).sum(-1, keepdim=True))).float()
    v = torch.randn(B, H, T, ATTN_D, generator=g)
    pi = torch.stack([torch.randperm(T, generator=g) for _ in range(B * H)]).view(B, H, T)
    q = (ATTN_ROUTING_GAIN * torch.gather(k, 2, pi[..., None].expand(B, H, T, ATTN_D))).contiguous()
    s = d(q) @ d(k).transpose(-1, -2)
    top = s.topk(min(2, T), -1)
    assert torch.equal(top.indices[..., 0], pi), "the best key of every query is pi's"
    if T > 1:
        gap = (top.values[..., 0] - top.values[..., 1]).min().item()
        assert gap > ATTN_ROUTING_GAP, f"score gap {gap} at T = {T}, seed {seed}"
    return q, k.contiguous(), v.contiguous(), pi, top.values[..., 0]


ATTN_UNDERFLOW_STEP = 1.0
ATTN_UNDERFLOW_GAP = 110.0


def attention_underflow_inputs(B, H, T=256, seed=3, nsplit=2):
    """The rising ramp of attention_inputs, steep enough (1 per key) that the log-sum-exp of the first of `nsplit` key splits is more than
    ATTN_UNDERFLOW_GAP below the second's for every query: the first split's merge weight exp(lse_0 - lse_1) underflows to 0.  Asserts that
    gap in float64 (splits are whole 32-key tiles, ceil(tiles / nsplit) each, as in the kernel).  Returns (q, k, v, dout)."""
    scale = 1.0 / math.sqrt(ATTN_D)
    q, k, v, dout = attention_inputs(B, H, T, seed, "rising", ATTN_UNDERFLOW_STEP, scale)
    per = -(-(-(-T // 32)) // nsplit) * 32
    s = (d(q) @ d(k).transpose(-1, -2)) * scale
    lse = [torch.log(torch.exp(part - s.max(-1, keepdim=True).values).sum(-1)) for part in (s[..., :per], s[..., per:2 * per])]
    gap = (lse[1] - lse[0]).min().item()
    assert gap > ATTN_UNDERFLOW_GAP, f"lse gap {gap}"
    return q, k, v, dout


def attention_split_fits(T, nsplit):
    """The host guard of dyn_attention_fwd_split: 1 <= nsplit <= 8 and the last split still has a key tile."""
    tiles = -(-T // 32)
    return 1 <= nsplit <= 8 and (nsplit == 1 or (nsplit - 1) * -(-tiles // nsplit) < tiles)


# ----------------------------------------------------------------------------------------------------------- one-token decoder
# csrc/decoder_step.hip (dyn_decoder_steps, dyn_decoder_steps_batch) from the definition of a pre-LN decoder layer
# (tests/test_decoder_step_kernels_gpu.py).  Dtype-agnostic: the result has the dtype of `params`, so the same function on fp32 copies is the
# "torch fp32" column of measured_tol.  The projected encoder keys | values are an INPUT: the key count is the caller's choice and no
# encoder is needed.  tests/test_kernel_refs_cpu.py holds it to oracle.enc_dec_ref.Decoder in float64.
# The 16 parameters of a layer in the pointer order of dyn_decoder_desc.layer_ptrs (slot 16 is the cache, slot 17 the projected kv).
DECODER_LAYER_PARAMS = ("self.norm.weight", "self.norm.bias", "self.qkv.weight", "self.qkv.bias", "self.out.weight", "self.out.bias",
                        "cross.norm.weight", "cross.norm.bias", "cross.q.weight", "cross.q.bias", "cross.out.weight", "cross.out.bias",
                        "ff.norm.weight", "ff.norm.bias", "ff.w1.weight", "ff.w2.weight")
DECODER_EPS = 1e-5


def decoder_positions(n, d_model):
    """The sinusoidal position rows [n, d_model]: sin in the even columns, cos in the odd ones, float64 rounded to fp32 once."""
    pos = torch.arange(n, dtype=F64)[:, None]
    inv = torch.exp(torch.arange(0, d_model, 2, dtype=F64) * (-math.log(10000.0) / d_model))
    tab = torch.zeros(n, d_model, dtype=F64)
    tab[:, 0::2] = torch.sin(pos * inv)
    tab[:, 1::2] = torch.cos(pos * inv)
    return tab.float()


def decoder_params(d_model, d_ff, vocab, layers, max_positions, seed=0):
    """fp32 CPU weights of one decoder, drawn as oracle.enc_dec_ref.EncDecRef draws them: matrices uniform / sqrt(fan_in) (embedding and
    head times 3), norm weights 1 +- 0.05, biases +- 0.05.  Keys are the decoder's state-dict names, plus "pos" (the position table)."""
    g = gen(31000 + seed)

    def mat(o, i, gain=1.0):
        return (torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i) * gain

    def vec(n, centre=0.0):
        return centre + 0.1 * (torch.rand(n, generator=g) - 0.5)

    shapes = {"self.qkv.weight": (3 * d_model, d_model), "self.out.weight": (d_model, d_model), "cross.q.weight": (d_model, d_model),
              "cross.out.weight": (d_model, d_model), "ff.w1.weight": (d_ff, d_model), "ff.w2.weight": (d_model, d_ff)}
    p = {"embed.weight": mat(vocab, d_model, 3.0), "pos": decoder_positions(max_positions, d_model)}
    for l in range(layers):
        for nm in DECODER_LAYER_PARAMS:
            if nm in shapes:
                p[f"layers.{l}.{nm}"] = mat(*shapes[nm])
            elif nm.endswith("norm.weight"):
                p[f"layers.{l}.{nm}"] = vec(d_model, 1.0)
            elif nm.endswith("norm.bias"):
                p[f"layers.{l}.{nm}"] = vec(d_model)
            else:
                p[f"layers.{l}.{nm}"] = vec(shapes[nm.replace("bias", "weight")][0])
    p["norm_out.weight"], p["norm_out.bias"] = vec(d_model, 1.0), vec(d_model)
    p["head.weight"], p["head.bias"] = mat(vocab, d_model, 3.0), vec(vocab)
    return p


def decoder_kv(layers, n_enc, d_model, seed=0, gain=1.0):
    """Projected encoder keys | values [n_enc, 2 * d_model] per layer, fp32: N(0, 1) * gain."""
    g = gen(32000 + seed + 13 * n_enc)
    return [torch.randn(n_enc, 2 * d_model, generator=g) * gain for _ in range(layers)]


def _decoder_norm(x, w, b, eps):
    n = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / n
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / n
    return (x - mean) / torch.sqrt(var + eps) * w + b


def _decoder_attend(q, k, v, heads, causal):
    """softmax(q k^T / sqrt(hd)) v per head, rows of q against rows of k / v; `causal`: query i sees keys 0 .. i.  [S, d] -> [S, d]."""
    S, dd = q.shape
    hd = dd // heads
    q, k, v = (t.reshape(t.shape[0], heads, hd).permute(1, 0, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    if causal:
        i = torch.arange(S)
        s = s.masked_fill(i[None, :] > i[:, None], float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    return (p @ v).permute(1, 0, 2).reshape(S, dd)


def decoder_split_maxima(q, k, heads, nsplit=4):
    """Score maxima [heads, nsplit] of ONE query row q [d] against keys k [n, d], the keys cut into `nsplit` chunks of ceil(n / nsplit) as
    dec_attn_kernel cuts them (an empty chunk: -inf).  float64."""
    q, k = d(q), d(k)
    n, dd = k.shape
    hd = dd // heads
    s = torch.einsum("hc,nhc->hn", q.view(heads, hd), k.view(n, heads, hd)) / math.sqrt(hd)
    chunk = -(-n // nsplit)
    out = torch.full((heads, nsplit), float("-inf"), dtype=F64)
    for u in range(nsplit):
        if u * chunk < n:
            out[:, u] = s[:, u * chunk:(u + 1) * chunk].max(-1).values
    return out


def decoder_steps_ref(params, tokens, kv_per_layer, heads, eps, cross_q=None):
    """Positions 0 .. S - 1 of the decoder on the token ids `tokens` [S], all at once (the causal mask is the prefix each one-token step
    sees): x = embed[token] + pos; per layer x += out(selfattn(LN x)), x += out(crossattn(q(LN x), kv)), x += w2 SiLU(w1 LN x);
    logits = head(LN x).  `kv_per_layer`: the already-projected encoder keys | values [n_enc, 2 * d_model] of every layer.
    `cross_q`: a list that receives every layer's cross-attention queries [S, d_model] (for assertions on a case's scores).
    Returns (logits [S, V], [per layer: the packed q | k | v rows [S, 3 * d_model], what the kernel leaves in its cache])."""
    P = params
    tok = torch.as_tensor(tokens, dtype=torch.long)
    S = tok.numel()
    x = P["embed.weight"][tok] + P["pos"][:S]
    dd = x.shape[1]
    rows = []
    for l, kv in enumerate(kv_per_layer):
        L = lambda nm: P[f"layers.{l}.{nm}"]                                   # noqa: E731
        qkv = _decoder_norm(x, L("self.norm.weight"), L("self.norm.bias"), eps) @ L("self.qkv.weight").T + L("self.qkv.bias")
        rows.append(qkv)
        o = _decoder_attend(qkv[:, :dd], qkv[:, dd:2 * dd], qkv[:, 2 * dd:], heads, True)
        x = x + o @ L("self.out.weight").T + L("self.out.bias")
        q2 = _decoder_norm(x, L("cross.norm.weight"), L("cross.norm.bias"), eps) @ L("cross.q.weight").T + L("cross.q.bias")
        if cross_q is not None:
            cross_q.append(q2)
        o = _decoder_attend(q2, kv[:, :dd], kv[:, dd:], heads, False)
        x = x + o @ L("cross.out.weight").T + L("cross.out.bias")
        a = _decoder_norm(x, L("ff.norm.weight"), L("ff.norm.bias"), eps) @ L("ff.w1.weight").T
        x = x + silu_expr(a) @ L("ff.w2.weight").T
    return _decoder_norm(x, P["norm_out.weight"], P["norm_out.bias"], eps) @ P["head.weight"].T + P["head.bias"], rows


def decoder_tol(torch_fp32, ref64):
    """measured_tol with the floor the project asserts for these logits and cache rows (2e-5 absolute at O(1) values,
    test_one_token_decoder_kernels_match_the_tile_kernel_path), taken relative to the largest wanted value once that exceeds 1."""
    return measured_tol(torch_fp32, ref64, 2e-5 * max(1.0, ref64.abs().max().item()))
