"""CPU float32 torch restatement of the beam search's LM (dynamic-asr-eval_amd/lm.py) with the call contract of the reference's
`transformer_lm` as lcasr/ctc_beam_search.py LanguageModel uses it: model(x=[B, S], length=[B], cache=None | {'cache':
[L, 2, B, H, N, hd], 'cache_lengths': [B]}) -> (logits [B, S, V], None, new_state).  Row b's new token attends to the first
cache_lengths[b] cached positions (padding beyond is ignored) plus itself; its position index is cache_lengths[b]."""
import math

import numpy as np
import torch


class CpuLM:
    def __init__(self, cfg, vocab, state):
        from dynamic_asr_eval_amd.lm import positions
        self.cfg, self.vocab = cfg, vocab
        self.P = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in state.items()}
        self.pos = torch.from_numpy(positions(cfg['max_positions'], cfg['d_model']))
        self.L, self.D, self.H = cfg['n_layers'], cfg['d_model'], cfg['n_heads']
        self.hd = self.D // self.H

    def eval(self):
        return self

    def to(self, *_):
        return self

    def _ln(self, x, w, b):
        return torch.nn.functional.layer_norm(x, (self.D,), self.P[w], self.P[b], self.cfg['norm_eps'])

    @torch.no_grad()
    def __call__(self, x, length, cache=None):
        B, S = x.shape
        assert S == 1 or cache is None
        L, H, hd, D = self.L, self.H, self.hd, self.D
        lens = [0] * B if cache is None else [int(v) for v in cache['cache_lengths']]
        nmax = max(lens) + S
        new = torch.zeros(L, 2, B, H, nmax, hd)
        out = torch.zeros(B, S, self.vocab)
        for b in range(B):
            n0 = lens[b]
            pos = torch.arange(n0, n0 + S).clamp(max=self.pos.shape[0] - 1)
            h = self.P['embed.weight'][x[b].long()] + self.pos[pos]
            for l in range(L):
                p = f'layers.{l}.'
                a = self._ln(h, p + 'self.norm.weight', p + 'self.norm.bias')
                qkv = a @ self.P[p + 'self.qkv.weight'].T + self.P[p + 'self.qkv.bias']
                q, k, v = qkv[:, :D].view(S, H, hd), qkv[:, D:2 * D].view(S, H, hd), qkv[:, 2 * D:].view(S, H, hd)
                if cache is not None:
                    k = torch.cat([cache['cache'][l, 0, b, :, :n0].permute(1, 0, 2), k], 0)
                    v = torch.cat([cache['cache'][l, 1, b, :, :n0].permute(1, 0, 2), v], 0)
                new[l, 0, b, :, :n0 + S] = k.permute(1, 0, 2)
                new[l, 1, b, :, :n0 + S] = v.permute(1, 0, 2)
                sc = torch.einsum('shd,nhd->hsn', q, k) / math.sqrt(hd)
                mask = torch.arange(n0 + S)[None, :] > (n0 + torch.arange(S))[:, None]
                sc = sc.masked_fill(mask[None], float('-inf'))
                o = torch.einsum('hsn,nhd->shd', sc.softmax(-1), v).reshape(S, D)
                h = h + o @ self.P[p + 'self.out.weight'].T + self.P[p + 'self.out.bias']
                a = self._ln(h, p + 'ff.norm.weight', p + 'ff.norm.bias')
                h = h + torch.nn.functional.silu(a @ self.P[p + 'ff.w1.weight'].T) @ self.P[p + 'ff.w2.weight'].T
            h = self._ln(h, 'norm_out.weight', 'norm_out.bias')
            out[b] = h @ self.P['head.weight'].T + self.P['head.bias']
        return out, None, {'cache': new, 'cache_lengths': torch.tensor([n + S for n in lens], dtype=torch.long)}
