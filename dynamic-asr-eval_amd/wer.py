"""Corpus-level word error rate with the return signature the reference harness unpacks:
`wer, words, ins_rate, del_rate, sub_rate = word_error_rate_detail(hypotheses=..., references=...)`
(reference lcasr/run_dynamic_eval_full.py:112-115; upstream `lcasr.eval.wer`, un-vendored).
Host-side integer dynamic programme (numpy rows); ties prefer substitution/match, then deletion, then insertion.
`edit_counts` exposes the four integer counters that the multi-GPU harness all-reduces over RCCL.
Every scoring function takes `device=None` (the host path, the default); with a GPU device the same integers come from the HIP
lattice kernel dyn_edit_counts (csrc/editdist.hip), all pairs of a call in one launch sequence."""
import re

import numpy as np


def basic_normalize(text):
    """Minimal stand-in for whisper.normalizers.EnglishTextNormalizer (un-vendored, reference
    run_dynamic_eval_full.py:8,20,106): lower-case, drop punctuation, squeeze whitespace."""
    text = text.lower()
    text = re.sub(r"[^a-z0-9' ]+", " ", text)
    return re.sub(r"\s+", " ", text).strip()


def _align(hyp, ref):
    """(ins, del, sub) of the minimum-edit alignment of two token-id arrays."""
    n, m = len(ref), len(hyp)
    if n == 0:
        return m, 0, 0
    if m == 0:
        return 0, n, 0
    # cost and op-count rows over hypothesis positions; one row per reference word
    cost = np.arange(m + 1, dtype=np.int64)
    ins = np.arange(m + 1, dtype=np.int64)
    dele = np.zeros(m + 1, dtype=np.int64)
    sub = np.zeros(m + 1, dtype=np.int64)
    hyp = np.asarray(hyp)
    idx = np.arange(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        neq = (hyp != ref[i - 1]).astype(np.int64)
        diag = cost[:-1] + neq            # substitution / match from (i-1, j-1)
        up = cost[1:] + 1                 # deletion from (i-1, j)
        best = np.minimum(diag, up)
        from_diag = diag <= up
        b_ins = np.where(from_diag, ins[:-1], ins[1:])
        b_del = np.where(from_diag, dele[:-1], dele[1:] + 1)
        b_sub = np.where(from_diag, sub[:-1] + neq, sub[1:])
        # insertions chain along the row: n_cost[j] = min_{k<=j} (start[k] + j - k) with start[0] = i (column 0) and
        # start[k] = best[k-1]; a running minimum of start[k] - k plus the LAST k that attains it (fewest insertions
        # on ties) vectorises the scan.
        start = np.concatenate(([i], best))
        v = start - idx
        run = np.minimum.accumulate(v)
        k_star = np.maximum.accumulate(np.where(v == run, idx, 0))
        n_cost = run + idx
        extra = idx - k_star
        s_ins = np.concatenate(([0], b_ins)); s_del = np.concatenate(([i], b_del)); s_sub = np.concatenate(([0], b_sub))
        n_ins = s_ins[k_star] + extra
        n_del = s_del[k_star]
        n_sub = s_sub[k_star]
        cost, ins, dele, sub = n_cost, n_ins, n_del, n_sub
    return int(ins[m]), int(dele[m]), int(sub[m])


def _pair_ids(h, r, use_cer):
    """Per-pair vocabulary ids; with `use_cer` the units are the characters of each string, spaces included (`list(h)`, as the
    NeMo-derived `lcasr.eval.wer` the reference imports)."""
    hw, rw = (list(h), list(r)) if use_cer else (h.split(), r.split())
    vocab = {}
    hi = [vocab.setdefault(w, len(vocab)) for w in hw]
    ri = [vocab.setdefault(w, len(vocab)) for w in rw]
    return hi, ri


def edit_counts_ids(hyp_ids, ref_ids, device, tile=0):
    """[P, 4] int32 numpy array of (ins, del, sub, n_ref) for P pairs of token-id sequences, scored on `device` by ONE
    dyn_edit_counts call (csrc/editdist.hip): ids and offsets go up in one pinned transfer, the counts come down in one.  The
    integers are those of `_align` on the same ids.  `tile` is the kernel's block size for long pairs (0 = its default)."""
    import torch

    from . import _lib
    P = len(hyp_ids)
    assert len(ref_ids) == P
    if P == 0:
        return np.zeros((0, 4), dtype=np.int32)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DynError(f"edit_counts: device {device} - the device path is the HIP kernel; pass device=None for the host path")
    off = np.zeros(2 * (P + 1), dtype=np.int64)   # hyp_off [P + 1] then ref_off [P + 1], the layout of the kernel's device copy
    np.cumsum([len(h) for h in hyp_ids], out=off[1:P + 1])
    np.cumsum([len(r) for r in ref_ids], out=off[P + 2:])
    n_hyp, n_ref = int(off[P]), int(off[-1])
    # one pinned int32 buffer: the offsets (as int64 pairs of words), the hypothesis ids, the reference ids
    words = 4 * (P + 1)
    host = torch.empty(words + n_hyp + n_ref + 1, dtype=torch.int32, pin_memory=True)
    view = host.numpy()
    view[:words] = off.view(np.int32)
    if n_hyp:
        view[words:words + n_hyp] = np.fromiter((t for h in hyp_ids for t in h), dtype=np.int32, count=n_hyp)
    if n_ref:
        view[words + n_hyp:words + n_hyp + n_ref] = np.fromiter((t for r in ref_ids for t in r), dtype=np.int32, count=n_ref)
    lib = _lib.load()
    hyp_off, ref_off = off[:P + 1], off[P + 1:]
    ws_bytes = lib.dyn_edit_counts_workspace_bytes(hyp_off.ctypes.data, ref_off.ctypes.data, P, tile)
    if ws_bytes < 0:
        _lib.check(int(ws_bytes), "dyn_edit_counts_workspace_bytes")
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream()
        dev = host.to(device, non_blocking=True)
        counts = torch.empty(P, 4, dtype=torch.int32, device=device)
        ws = torch.empty(max(int(ws_bytes), 4), dtype=torch.uint8, device=device)
        base = dev.data_ptr()
        _lib.check(lib.dyn_edit_counts(base + 4 * words, base + 4 * (words + n_hyp), hyp_off.ctypes.data, ref_off.ctypes.data, base,
                                       counts.data_ptr(), ws.data_ptr(), int(ws_bytes), P, tile, stream.cuda_stream), "dyn_edit_counts")
        out = torch.empty(P, 4, dtype=torch.int32, pin_memory=True)
        out.copy_(counts, non_blocking=True)
        stream.synchronize()
    return out.numpy().copy()


def edit_counts_pairs(hypotheses, references, use_cer=False, device=None):
    """Per-pair (insertions, deletions, substitutions, reference_units).  `device=None` is the host dynamic programme; with a
    GPU device all pairs are scored by one kernel call and the integers are the same."""
    ids = [_pair_ids(h, r, use_cer) for h, r in zip(hypotheses, references)]
    if device is None:
        return [_align(hi, ri) + (len(ri),) for hi, ri in ids]
    return [tuple(int(x) for x in row) for row in edit_counts_ids([hi for hi, _ in ids], [ri for _, ri in ids], device)]


def edit_counts(hypotheses, references, use_cer=False, device=None):
    """(insertions, deletions, substitutions, reference_words) summed over the corpus; with `use_cer` the units are the
    characters of each string, spaces included (`list(h)`, as the NeMo-derived `lcasr.eval.wer` the reference imports)."""
    tot = [0, 0, 0, 0]
    for i, d, s, n in edit_counts_pairs(hypotheses, references, use_cer=use_cer, device=device):
        tot[0] += i; tot[1] += d; tot[2] += s; tot[3] += n
    return tuple(tot)


def rates_from_counts(ins, dele, sub, words):
    if words == 0:
        return (float("inf") if (ins + dele + sub) else 0.0), 0, 0.0, 0.0, 0.0
    return (ins + dele + sub) / words, words, ins / words, dele / words, sub / words


def word_error_rate_detail(hypotheses, references, use_cer=False, device=None):
    return rates_from_counts(*edit_counts(hypotheses, references, use_cer=use_cer, device=device))
