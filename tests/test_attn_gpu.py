"""_attn.py (the five products of materialised-score attention, written once) against a float64 torch restatement, at the operand placements
the models use and two they do not reach: heads in a packed [B, T, 3H] projection, in three separate [B, T, H] tensors, and (one sample, the
enc-dec decoder's form) as column ranges of wider rows with different leading dimensions for q and k | v; self-attention (Tq = Tk = 37) and
cross-attention (Tq = 5, Tk = 37).  Every output goes into a NaN-filled buffer: what the function owns must be written, nothing else touched.
The bar is tests/test_gemm_gpu.py's for these products against float64 (1e-4 absolute at unit-variance operands; K <= 37 here)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NH, D = 3, 8
H = NH * D
BAR = 1e-4


class Operand:
    """One of q, k, v, O, dO, dq, dk, dv: a buffer, the columns of its rows that hold the heads, and the _attn.View of them."""

    def __init__(self, buf, col0, view):
        self.buf, self.col0, self.view = buf, col0, view

    def heads(self):
        """[B, nh, T, D] float64 on the host (B = 1 for a 2-D buffer)."""
        rows = self.buf if self.buf.dim() == 3 else self.buf[None]
        return rows[..., self.col0:self.col0 + H].reshape(rows.shape[0], rows.shape[1], NH, D).permute(0, 2, 1, 3).double().cpu()

    def untouched(self):
        """Every element outside the heads' columns is still NaN."""
        out = self.buf.clone()
        out[..., self.col0:self.col0 + H] = float("nan")
        return bool(torch.isnan(out).all())


def _place(A, layout, cuda, g, B, Tq, Tk, out):
    """q | k | v (or, `out`, NaN-filled dq | dk | dv) placed by `layout` -> three Operands."""
    new = (lambda *s: torch.full(s, float("nan"), device=cuda)) if out else (lambda *s: torch.randn(*s, generator=g).to(cuda))
    if layout == "packed":
        buf = new(B, Tq, 3 * H)
        return [Operand(buf, j * H, A.packed(buf, j, D)) for j in range(3)]
    if layout == "separate":
        bufs = [new(B, T, H) for T in (Tq, Tk, Tk)]
        return [Operand(b, 0, A.plain(b, D)) for b in bufs]
    ldq, ldk = H + 8, 2 * H + 16                               # padded: q at columns 4 .. 4 + H of [Tq, ldq]; k, v at 0 and H + 8 of [Tk, ldk]
    qb, kvb = new(Tq, ldq), new(Tk, ldk)
    return [Operand(qb, 4, A.plain(qb[:, 4:], D, ldq)), Operand(kvb, 0, A.plain(kvb, D, ldk)), Operand(kvb, H + 8, A.plain(kvb[:, H + 8:], D, ldk))]


def _plain(A, cuda, g, B, T, out):
    buf = torch.full((B, T, H), float("nan"), device=cuda) if out else torch.randn(B, T, H, generator=g).to(cuda)
    buf = buf if B > 1 else buf[0]
    return Operand(buf, 0, A.plain(buf, D))


def _scores(cuda, g, B, Tq, Tk, out, three_d):
    s = torch.full((B, NH, Tq, Tk), float("nan"), device=cuda) if out else torch.randn(B, NH, Tq, Tk, generator=g).to(cuda)
    return s[0] if three_d else s


def _err(got, ref):
    got = got.double().cpu()
    return (got.reshape(ref.shape) - ref).abs().max().item()


@pytest.mark.parametrize("layout,B,Tq,Tk", [("packed", 2, 37, 37), ("separate", 2, 37, 37), ("separate", 2, 5, 37), ("padded", 1, 37, 37),
                                            ("padded", 1, 5, 37)],
                         ids=["packed", "separate", "separate-cross", "padded-one-sample", "padded-one-sample-cross"])
def test_the_five_products_match_float64_and_write_only_their_views(cuda, layout, B, Tq, Tk):
    from dynamic_asr_eval_amd import _attn as A
    g = torch.Generator().manual_seed(Tq * 100 + B)
    scale = D ** -0.5
    three_d = layout == "padded"                               # one sample: scores [nh, Tq, Tk], batch stride 0
    q, k, v = _place(A, layout, cuda, g, B, Tq, Tk, out=False)
    qh, kh, vh = q.heads(), k.heads(), v.heads()

    S = _scores(cuda, g, B, Tq, Tk, True, three_d)
    A.scores(q.view, k.view, S, scale)
    e = _err(S, scale * qh @ kh.transpose(-1, -2))
    print("scores", e)
    assert e < BAR

    P = _scores(cuda, g, B, Tq, Tk, False, three_d)            # unit-variance stand-ins for the probabilities and for dS
    Ph = P.double().cpu().reshape(B, NH, Tq, Tk)
    O = _plain(A, cuda, g, B, Tq, out=True)
    A.context(P, v.view, O.view)
    e = _err(O.heads(), Ph @ vh)
    print("context", e)
    assert e < BAR

    dO = _plain(A, cuda, g, B, Tq, out=False)
    dq, dk, dv = _place(A, layout, cuda, g, B, Tq, Tk, out=True)
    dP = _scores(cuda, g, B, Tq, Tk, True, three_d)
    A.grad_v_dP(P, dO.view, v.view, dv.view, dP)
    e1, e2 = _err(dv.heads(), Ph.transpose(-1, -2) @ dO.heads()), _err(dP, dO.heads() @ vh.transpose(-1, -2))
    print("grad_v_dP", e1, e2)
    assert e1 < BAR and e2 < BAR
    assert dv.untouched(), "grad_v_dP wrote outside dv's columns"
    if layout == "packed":                                     # dq | dk share dv's buffer: still NaN
        assert bool(torch.isnan(dq.heads()).all()) and bool(torch.isnan(dk.heads()).all())

    dS, dSh = P, Ph
    dq2, dk2, dv2 = _place(A, layout, cuda, g, B, Tq, Tk, out=True)
    A.grad_qk(dS, q.view, k.view, dq2.view, dk2.view, scale)
    e1, e2 = _err(dq2.heads(), scale * dSh @ kh), _err(dk2.heads(), scale * dSh.transpose(-1, -2) @ qh)
    print("grad_qk", e1, e2)
    assert e1 < BAR and e2 < BAR
    assert bool(torch.isnan(dv2.heads()).all()), "grad_qk wrote dv's columns"
    if layout == "padded":                                     # the padding of both row widths, and (dk | dv share a buffer) nothing but dk
        assert dq2.untouched()
        probe = dk2.buf.clone()
        probe[:, :H] = float("nan")
        assert bool(torch.isnan(probe).all())
    elif layout == "packed":
        assert bool(torch.isnan(dq2.buf[..., 2 * H:]).all())


def test_grad_qk_routes_dq_and_reads_q_independently(cuda):
    """What the conformer's relative branch does: k from the packed projection, q = q + u a tensor of its own, dQ into a tensor of its own,
    dK into the packed gradient's k slot; the q and v slots of that gradient stay untouched."""
    from dynamic_asr_eval_amd import _attn as A
    g = torch.Generator().manual_seed(3)
    B, T = 2, 37
    scale = D ** -0.5
    qkv = torch.randn(B, T, 3 * H, generator=g).to(cuda)
    qu = _plain(A, cuda, g, B, T, out=False)
    dqu = _plain(A, cuda, g, B, T, out=True)
    dqkv = torch.full((B, T, 3 * H), float("nan"), device=cuda)
    k, dk = Operand(qkv, H, A.packed(qkv, 1, D)), Operand(dqkv, H, A.packed(dqkv, 1, D))
    dS = torch.randn(B, NH, T, T, generator=g).to(cuda)
    A.grad_qk(dS, qu.view, k.view, dqu.view, dk.view, scale)
    dSh = dS.double().cpu()
    assert _err(dqu.heads(), scale * dSh @ k.heads()) < BAR
    assert _err(dk.heads(), scale * dSh.transpose(-1, -2) @ qu.heads()) < BAR
    assert dk.untouched()
