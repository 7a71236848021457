"""GreedyCTCDecoder with the reference's call signature — `GreedyCTCDecoder(tokenizer=..., blank_id=...)` then
`decoder(log_probs[T, C]) -> str` (reference lcasr/lib.py:498,559,565; run_dynamic_eval_full.py:53,100) — but the
argmax / collapse / blank-drop runs on the GPU (dyn_ctc_greedy) and only the surviving token ids cross PCIe."""
import torch

from . import ops


class GreedyCTCDecoder:
    def __init__(self, tokenizer, blank_id, device=None):
        self.tokenizer = tokenizer
        self.blank_id = int(blank_id)
        self.device = device

    def ids(self, log_probs):
        """[T, C] (or [B, T, C]) log-probabilities -> list (or list of lists) of token ids."""
        lp = torch.as_tensor(log_probs)
        if not lp.is_cuda:
            dev = self.device or (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
            if dev is None:
                raise ops.DynError("GreedyCTCDecoder: no GPU available and there is no CPU decode path")
            lp = lp.to(dev, torch.float32)
        lp = lp.contiguous()
        single = lp.dim() == 2
        ids, n = ops.ctc_greedy(lp, self.blank_id)
        n = n.cpu().tolist()
        ids = ids.cpu()
        out = [ids[b, :n[b]].tolist() for b in range(len(n))]
        return out[0] if single else out

    def __call__(self, log_probs):
        ids = self.ids(log_probs)
        if ids and isinstance(ids[0], list):
            return [self.tokenizer.decode(i) for i in ids]
        return self.tokenizer.decode(ids)


class Beam:
    """One surviving beam in the reference's shapes (lcasr/ctc_beam_search.py:15-43): `am_sequence` = [None] + tokens
    (+ [blank] while the path ends in a blank), `lm_sequence` = [bos] + tokens, `score` a float."""
    __slots__ = ('score', 'am_sequence', 'lm_sequence')

    def __init__(self, score, am_sequence, lm_sequence):
        self.score, self.am_sequence, self.lm_sequence = score, am_sequence, lm_sequence

    def __repr__(self):
        return f"{self.am_sequence}"


class BeamSearch:
    """CTC + transformer-LM beam search (reference BeamSearch, lcasr/ctc_beam_search.py:89-319, max_cache_length = 128) run on
    the GPU by dyn_beam_search: the host enqueues the whole search on `stream` and reads back only the final beams."""

    def __init__(self, tokenizer, beam_width, log_probs, language_model, alpha=0.4, beta=0.4, blank_id=None, blank_penalty=0.0,
                 repitition_penalty=0.0, top_am_threshold=-6, prune_less_than_val=None, bos_id=0, stream=None):
        from ._lib import load
        lib = load()
        self.tokenizer, self.language_model = tokenizer, language_model
        self.beam_width = int(beam_width)
        self.vocab_size = tokenizer.vocab_size()
        self.blank_id = self.vocab_size if blank_id is None else int(blank_id)
        if self.blank_id != self.vocab_size:
            raise ValueError(f'BeamSearch: blank_id must be the vocabulary size {self.vocab_size} (got {self.blank_id})')
        if self.beam_width < 1 or self.beam_width > 20:
            raise ValueError(f'BeamSearch: beam_width must be in [1, 20] (got {beam_width})')
        self.alpha, self.beta, self.blank_penalty, self.repitition_penalty = alpha, beta, blank_penalty, repitition_penalty
        self.top_am_threshold, self.prune_less_than_val, self.bos_id = top_am_threshold, prune_less_than_val, int(bos_id)
        lp = torch.as_tensor(log_probs)
        if lp.dim() != 2 or lp.shape[1] != self.vocab_size + 1:
            raise ValueError(f'BeamSearch: log_probs must be [T, {self.vocab_size + 1}], got {tuple(lp.shape)}')
        self.log_probs = lp.to(language_model.device, torch.float32).contiguous()
        self.stream = stream
        self.beams, self.position, self._lib = [], 0, lib

    def run_search(self, use_tqdm=False):
        import ctypes
        from ._lib import check
        T = int(self.log_probs.shape[0])
        if T == 0:
            raise ValueError('BeamSearch: no frames')
        lm, lib, W = self.language_model, self._lib, self.beam_width
        L, D, H, F, V, maxpos, eps = lm.dims()
        nbytes = lib.dyn_beam_workspace_bytes(W, T, L, D, F, V)
        stream = self.stream if self.stream is not None else torch.cuda.current_stream(lm.device)
        stream.wait_stream(torch.cuda.current_stream(lm.device))     # log_probs were produced / uploaded on the caller's stream
        with torch.cuda.stream(stream):         # workspace, search and read-back all ordered on `stream`
            ws = torch.empty(nbytes, dtype=torch.uint8, device=lm.device)
            check(lib.dyn_beam_search(self.log_probs.data_ptr(), T, self.log_probs.stride(0), int(self.log_probs.shape[1]),
                                      ctypes.cast(lm.ptrs, ctypes.c_void_p), L, D, H, F, V, maxpos, eps, self.bos_id, W,
                                      float(self.alpha), float(self.beta), float(self.blank_penalty), float(self.repitition_penalty),
                                      float(self.top_am_threshold), float(self.prune_less_than_val or 0.0),
                                      int(self.prune_less_than_val is not None), ws.data_ptr(), nbytes, stream.cuda_stream),
                  "dyn_beam_search")
            self.log_probs.record_stream(stream)
            off = beam_layout(lib, W, T, L, D, F, V)
            hdr = ws[off['hdr']:off['hdr'] + 64].view(torch.int32).cpu()        # synchronises this stream only
            if int(hdr[2]) != 0:
                raise RuntimeError(f'beam search failed on the device (code {int(hdr[2])}: 1/3 = no candidate in a frame, '
                                   '2 = merge table overflow, 4/5 = trie / pool capacity)')
            par = T & 1
            nb, nodes = int(hdr[par]), int(hdr[3])

            def i32(name, n, start=0):
                return ws[off[name] + 4 * start:off[name] + 4 * (start + n)].view(torch.int32)
            node = i32('b_node', nb, par * W).cpu().tolist()
            tb = i32('b_tb', nb, par * W).cpu().tolist()
            score = i32('b_score', nb, par * W).view(torch.float32).cpu().tolist()
            parent = i32('n_parent', nodes).cpu().numpy()
            token = i32('n_token', nodes).cpu().numpy()
        beams = []
        for k in range(nb):
            toks, n = [], node[k]
            while n > 0:
                toks.append(int(token[n]))
                n = int(parent[n])
            toks.reverse()
            am = [None] + toks + ([self.blank_id] if tb[k] else [])
            beams.append(Beam(score[k], am, [self.bos_id] + toks))
        self.beams, self.position = beams, T

    def return_text(self, idx):
        if idx >= len(self.beams):
            print('Beam index out of range')
            return
        return self.tokenizer.decode(self.beams[idx].lm_sequence[1:])


_LAYOUT_NAMES = ('hdr', 'b_node', 'b_tb', 'b_score', 'b_hlen', 'b_hist', 'n_parent', 'n_token', 'pool_lp', 'r_tok', 'r_pos', 'r_hlen',
                 'r_slot', 'r_hist', 'pool_kv', 'max_nodes', 'pool_slots', 'total')


def beam_layout(lib, W, T, L, D, F, V):
    import ctypes
    from ._lib import check
    arr = (ctypes.c_int64 * len(_LAYOUT_NAMES))()
    check(lib.dyn_beam_layout(W, T, L, D, F, V, ctypes.cast(arr, ctypes.c_void_p)), "dyn_beam_layout")
    return dict(zip(_LAYOUT_NAMES, list(arr)))
