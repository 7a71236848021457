"""Plumbing shared by the dynamic-eval loops (lib, awmc, wav2vec2_lib, run_seq_eval, run_half_concat_eval, enc_dec): the window
rule, the augmented batch, the on-device stitch, the pseudo-label round trip, bench.py's roofline-sampling hooks and the chain
scheduler.  The loops themselves read as the reference's steps (lcasr/lib.py:450-640); the mechanics live here."""
import time

import torch

from . import ops


# ------------------------------------------------------------------------------------------------ windows
def window_rule(args, spec_n, seq_len, overlap, downsampling_factor):
    """(seq_len, overlap) of one recording, reference lib.py:490-505: -1 takes the checkpoint config's value, a recording shorter
    than seq_len is one window without overlap."""
    seq_len = seq_len if seq_len != -1 else args.config['audio_chunking']['size']
    if seq_len > spec_n:
        seq_len, overlap = spec_n, 0
    else:
        overlap = overlap if overlap != -1 else args.config['audio_chunking']['overlap']
    assert args.config['training'].get("max_seq_len", 0) == 0, 'caching is not used anymore'
    assert overlap / downsampling_factor == overlap // downsampling_factor, 'Overlap must be a multiple of the downsampling factor'
    return seq_len, overlap


def window_fill_value(window, zero_masking):
    """Fill value of the SpecAugment masks: 0, or the window mean as a 1-element DEVICE tensor (dyn_moments) so that it
    never makes a host round trip."""
    if zero_masking:
        return 0.0
    from ._lib import check, load
    out = torch.empty(3, device=window.device, dtype=torch.float32)
    ws = ops.workspace(window.device)
    check(load().dyn_moments(window.data_ptr(), window.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                             torch.cuda.current_stream().cuda_stream), "dyn_moments")
    return out[1:2]


def augmented_batch(views, draw_masks, augmentation, extra=None):
    """[2 n, F, T] batch of the n equal-length windows `views` ([F, T] each): rows 0..n-1 the augmented copies, rows n..2n-1 the
    clean ones (reference lib.py:540-544 for n = 1: copy 0 augmented, copy -1 clean).  Row by row: both copies, the SpecAugment
    masks `draw_masks(k)` (host RNG, drawn in row order) on the augmented copy, then `extra(row)` on it."""
    n = len(views)
    Fq, u_len = views[0].shape
    batch = torch.empty(2 * n, Fq, u_len, device=views[0].device, dtype=torch.float32)
    for k, view in enumerate(views):
        batch[k].copy_(view)
        batch[n + k].copy_(view)
        masks = draw_masks(k)
        if masks[0][0] or masks[1][0]:
            augmentation.apply(batch[k], masks, window_fill_value(batch[k], augmentation.zero_masking))
        if extra is not None:
            extra(batch[k])
    return batch


# ------------------------------------------------------------------------------------------------ stitch
class Stitcher:
    """On-device overlap-add of window log-probs (reference lib.py:583-589,604-629 and run_seq_eval.py:120-142): exp, accumulate
    from the window's position, count; `finalize` = log(sum / count) over the covered rows."""

    def __init__(self, rows, num_classes, device):
        self.acc = torch.zeros(rows, num_classes, device=device, dtype=torch.float32)
        self.cnt = torch.zeros(rows, device=device, dtype=torch.float32)
        self.pos = self.end = 0

    @classmethod
    def for_recording(cls, spec_n, seq_len, num_classes, device):
        return cls(spec_n // 4 + seq_len, num_classes, device)      # the reference's two host buffers, lib.py:510

    def add(self, key, log_probs_2d, u_len, overlap):
        """Window `key` ([ds_len, C] log-probs of u_len input frames) starts overlap_ds rows before the previous one ended."""
        ds_len = log_probs_2d.shape[0]
        overlap_ds = int(overlap / (u_len / ds_len))
        self.pos -= overlap_ds if key != 0 else 0
        ops.stitch_accumulate(log_probs_2d, self.acc, self.cnt, self.pos)
        self.pos += ds_len
        self.end = max(self.end, self.pos)

    def reset(self):
        self.acc.zero_()
        self.cnt.zero_()
        self.pos = self.end = 0

    def finalize(self):
        return ops.stitch_finalize(self.acc, self.cnt, self.end)


# ------------------------------------------------------------------------------------------------ pseudo-labels
class PseudoLabels:
    """The pseudo-label round trip of one generator call.  Only ids cross PCIe, through pinned memory, so the host blocks only in
    `wait`: `fetch` the greedy ids of rows lo..hi-1 down, `record` the event the caller yields on, `wait`, read them with `ids`,
    then send the re-encoded targets up with `targets`.  `host_wait` (a one-element list) adds up the seconds spent in `wait`."""

    def __init__(self, rows, device, host_wait=None):
        self.rows, self.device, self.host_wait = rows, device, host_wait
        self.ready = None
        # Download: the ids of a step in one flat pinned buffer, one contiguous [hi - lo, width] block per fetch (a strided
        # destination would turn the copy into a blocking one), and the [rows] lengths.  `_start[q]`: where row q's ids begin.
        self._ids = self._n = None
        self._start, self._down = {}, 0
        self._up, self._used = None, 0  # upload slot: one flat pinned buffer holding all target rows of a step

    def fetch(self, ids_dev, n_dev, lo=0, hi=1):
        width = ids_dev.shape[1]
        if self._down == 0 and (self._ids is None or self._ids.numel() < self.rows * width):
            # before the first copy of a step, at its longest window (a group's shape classes run longest first)
            self._ids = torch.empty(self.rows * width, dtype=torch.int32, pin_memory=True)
            self._n = torch.empty(self.rows, dtype=torch.int32, pin_memory=True)
        block = self._ids[self._down:self._down + (hi - lo) * width]
        assert block.numel() == (hi - lo) * width, "pseudo-label ids: a step's windows outgrew its first one"
        block.view(hi - lo, width).copy_(ids_dev, non_blocking=True)
        self._n[lo:hi].copy_(n_dev, non_blocking=True)
        for q in range(lo, hi):
            self._start[q] = self._down + (q - lo) * width
        self._down += (hi - lo) * width

    def record(self):
        self.ready = torch.cuda.Event()
        self.ready.record()
        return self.ready

    def wait(self, resume=None):
        """Block until the ids are on the host; `resume` (the profile hook) runs first, inside the timed wait."""
        t0 = time.perf_counter()
        if resume is not None:
            resume()
        self.ready.synchronize()
        if self.host_wait is not None:
            self.host_wait[0] += time.perf_counter() - t0
        self._down = 0
        self._used = 0      # the slot is reused only now: `ready` follows every upload queued on this stream before the fetch

    def ids(self, row=0):
        return self._ids[self._start[row]:self._start[row] + int(self._n[row])].tolist()

    def targets(self, id_lists):
        """-> (targets [n, S_max] int32, lengths [n] int32) on the device, zero-padded; an empty label is the row [0] of length 0."""
        n = len(id_lists)
        S_max = max(1, max(len(t) for t in id_lists))
        need = n * S_max + n
        if self._up is None or self._used + need > self._up.numel():
            # a fresh slot; the caching host allocator keeps the old one's memory until its queued copies have run
            self._up, self._used = torch.empty(max(4 * need, 1024), dtype=torch.int32, pin_memory=True), 0
        block = self._up[self._used:self._used + need]
        self._used += need
        host, lens = block[:n * S_max].view(n, S_max), block[n * S_max:]
        host.zero_()
        for k, t in enumerate(id_lists):
            if t:
                host[k, :len(t)] = torch.as_tensor(t, dtype=torch.int32)
            lens[k] = len(t)
        targets = torch.empty(n, S_max, dtype=torch.int32, device=self.device)
        targets.copy_(host, non_blocking=True)
        if n == 1:      # one length: a fill, no copy
            return targets, torch.full((1,), len(id_lists[0]), dtype=torch.int32, device=self.device)
        tlen = torch.empty(n, dtype=torch.int32, device=self.device)
        tlen.copy_(lens, non_blocking=True)
        return targets, tlen


# ------------------------------------------------------------------------------------------------ roofline sampling
class ProfileStep:
    """bench.py's live roofline sampling (ops.gemm_profile_*) around one window step or final-pass batch: begin at construction,
    `before_yield(ready)`, `resume()` after the yield, `end()`.  No-ops while sampling is off."""

    def __init__(self, device):
        self.device = device
        self.kind = ops.gemm_profile_begin_step(device) if ops.gemm_profile_active() else 0

    def before_yield(self, ready):
        if self.kind:
            ops.gemm_profile_before_yield(self.kind, ready)

    def resume(self):
        if ops.gemm_profile_active():        # also for unsampled steps: the mode is per model call, chains interleave on this thread
            ops.gemm_profile_resume_step(self.device, self.kind)

    def end(self):
        if self.kind:
            ops.gemm_profile_end_step(self.device, self.kind)


# ------------------------------------------------------------------------------------------------ chains
_CHAIN_STREAMS = {}


def _new_chain_stream(device, k):
    """Stream of recording chain k.  DYN_CHAIN_CU_MASK=<n>[:stride] (experiment switch, off by default) gives chain k a stream whose
    kernels may not use a group of n of the 256 CUs — CUs k*n .. k*n+n-1, or with `:stride` every (256/n)-th CU starting at k — so the
    short kernels of the OTHER chains can start there while a matrix kernel of chain k holds the rest of the chip
    (dyn_stream_create_cu_mask = hipExtStreamCreateWithCUMask).  Measured: DESIGN.md §5."""
    import ctypes
    import os
    spec = os.environ.get("DYN_CHAIN_CU_MASK", "")
    if not spec or spec == "0":
        return torch.cuda.Stream(device=device)
    from ._lib import check, load
    n = int(spec.split(":")[0])
    strided = spec.endswith(":stride")
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    if not 0 < n < n_cu:
        raise ops.DynError(f"DYN_CHAIN_CU_MASK={spec!r}: hole size must be in 1..{n_cu - 1}")
    hole = {(k + j * (n_cu // n)) % n_cu for j in range(n)} if strided else {(k * n + j) % n_cu for j in range(n)}
    words = (ctypes.c_uint32 * ((n_cu + 31) // 32))()
    for cu in range(n_cu):
        if cu not in hole:
            words[cu // 32] |= 1 << (cu % 32)
    out = ctypes.c_void_p()
    with torch.cuda.device(device):
        check(load().dyn_stream_create_cu_mask(words, len(words), ctypes.byref(out)), "dyn_stream_create_cu_mask")
    return torch.cuda.ExternalStream(out.value, device=device)


def chain_streams(device, n):
    """The first n chain streams of `device`.  They are kept: the caching allocator's per-stream pools stay warm across calls (no
    hipMalloc in the loop)."""
    streams = _CHAIN_STREAMS.setdefault(torch.device(device).index, [])
    while len(streams) < n:
        streams.append(_new_chain_stream(device, len(streams)))
    return streams[:n]


def run_chains(models, jobs, make_gen, stagger_us=0):
    """Several jobs in flight on ONE GPU from one host thread: chain k runs `make_gen(models[k], payload)` on its own stream, one job at
    a time, and the chains are advanced round-robin at their yield points.  `jobs` = [(index, payload)]: a generator's return value is
    the result at `index`, or one result per index when `index` is a list.  With `stagger_us`, chain k starts k * stagger_us later (a
    device-side delay on its stream).  Returns the results in index order."""
    device = models[0].device
    streams = chain_streams(device, len(models))
    main = torch.cuda.current_stream(device)
    for st in streams:
        st.wait_stream(main)
    if stagger_us > 0:
        from ._lib import check, load
        for k, st in enumerate(streams):
            if k:
                check(load().dyn_sleep_us(min(k * stagger_us, 2000000), st.cuda_stream), "dyn_sleep_us")
    pending, results = list(jobs), {}
    free, active = list(range(len(models)))[::-1], []
    while pending or active:
        while pending and free:
            ci = free.pop()
            idx, payload = pending.pop(0)
            active.append((make_gen(models[ci], payload), ci, idx))
        for item in list(active):
            gen, ci, idx = item
            with torch.cuda.stream(streams[ci]):
                try:
                    next(gen)
                except StopIteration as stop:
                    results.update(zip(idx, stop.value) if isinstance(idx, list) else [(idx, stop.value)])
                    active.remove(item)
                    free.append(ci)
    for st in streams:
        main.wait_stream(st)
    return [results[k] for k in sorted(results)]


def drain(gen):
    """Run a generator to its end; -> its return value."""
    try:
        while True:
            next(gen)
    except StopIteration as stop:
        return stop.value
