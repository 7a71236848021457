"""Materialised-score attention as strided batched GEMMs, in one place for every model that keeps its scores in memory (SCConformerXL's
unfused path in model.py, Wav2Vec2ForCTC / WavLMForCTC in wav2vec2_model.py, both position schemes of Wav2Vec2ConformerForCTC, the enc-dec
decoder in enc_dec.py).  The chain is five products:

    S  = scale q k^T          scores
    O  = P v                  context
    dV = P^T dO, dP = dO v^T  grad_v_dP
    dQ = scale dS k, dK = scale dS^T q   grad_qk

Each function is exactly the one or two ops.gemm calls of its line.  What differs between the models happens between the calls, at the
call site: the softmax and its backward (plain, key-length masked, WavLM's gated bias, the conformer's shifted BD term), the decoder's
causal mask and dropout.  No state and no model knowledge here: an operand is a `View`, a score tensor is contiguous [B, nh, Tq, Tk] (or
[nh, Tq, Tk] for one sample) and gives the batch count, the head count and both lengths."""
from collections import namedtuple

from . import ops

# Where the heads of q, k, v or of an output live: head h of sample b is the [T, D] matrix at element `off + b * sb + h * sh` of tensor `t`
# (counted from its data_ptr), its rows `ld` elements apart.  Heads lie side by side in a row, so sh is also the head dimension D.
View = namedtuple("View", "t off ld sb sh")


def packed(qkv, j, D):
    """Slot j (0 q, 1 k, 2 v) of a packed projection [B, T, 3H], head h at column j H + h D."""
    T, H3 = qkv.shape[-2:]
    return View(qkv, j * (H3 // 3), H3, T * H3, D)


def plain(x, D, ld=None):
    """x [B, T, H] or [T, H] (one sample), head h at column h D; `ld`: the row stride when x is a column range of wider rows."""
    ld = x.shape[-1] if ld is None else ld
    return View(x, 0, ld, x.shape[-2] * ld if x.dim() == 3 else 0, D)


def _dims(S):
    nh, Tq, Tk = S.shape[-3:]
    if S.dim() == 3:
        return Tq, Tk, dict(nb1=1, nb2=nh), (0, Tq * Tk)
    return Tq, Tk, dict(nb1=S.shape[0], nb2=nh), (nh * Tq * Tk, Tq * Tk)


def scores(q, k, S, scale):
    """S = scale q k^T."""
    Tq, Tk, nb, sS = _dims(S)
    ops.gemm(q.t, k.t, S, trans_b=True, M=Tq, N=Tk, K=q.sh, lda=q.ld, ldb=k.ld, ldc=Tk, **nb, sa=(q.sb, q.sh), sb=(k.sb, k.sh), sc=sS,
             a_off=q.off, b_off=k.off, alpha=scale)


def context(P, v, O):
    """O = P v."""
    Tq, Tk, nb, sS = _dims(P)
    ops.gemm(P, v.t, O.t, M=Tq, N=v.sh, K=Tk, lda=Tk, ldb=v.ld, ldc=O.ld, **nb, sa=sS, sb=(v.sb, v.sh), sc=(O.sb, O.sh), b_off=v.off,
             c_off=O.off)


def grad_v_dP(P, dO, v, dv, dP):
    """dV = P^T dO and dP = dO v^T; P is what the forward multiplied with v (the dropped probabilities under dropout)."""
    Tq, Tk, nb, sS = _dims(P)
    ops.gemm(P, dO.t, dv.t, trans_a=True, M=Tk, N=v.sh, K=Tq, lda=Tk, ldb=dO.ld, ldc=dv.ld, **nb, sa=sS, sb=(dO.sb, dO.sh),
             sc=(dv.sb, dv.sh), b_off=dO.off, c_off=dv.off)
    ops.gemm(dO.t, v.t, dP, trans_b=True, M=Tq, N=Tk, K=v.sh, lda=dO.ld, ldb=v.ld, ldc=Tk, **nb, sa=(dO.sb, dO.sh), sb=(v.sb, v.sh), sc=sS,
             a_off=dO.off, b_off=v.off)


def grad_qk(dS, q, k, dq, dk, scale):
    """dQ = scale dS k and dK = scale dS^T q.  q, dq and dk are independent views: dQ may go where q did not come from."""
    Tq, Tk, nb, sS = _dims(dS)
    ops.gemm(dS, k.t, dq.t, M=Tq, N=k.sh, K=Tk, lda=Tk, ldb=k.ld, ldc=dq.ld, **nb, sa=sS, sb=(k.sb, k.sh), sc=(dq.sb, dq.sh), b_off=k.off,
             c_off=dq.off, alpha=scale)
    ops.gemm(dS, q.t, dk.t, trans_a=True, M=Tk, N=q.sh, K=Tq, lda=Tk, ldb=q.ld, ldc=dk.ld, **nb, sa=sS, sb=(q.sb, q.sh), sc=(dk.sb, dk.sh),
             b_off=q.off, c_off=dk.off, alpha=scale)
