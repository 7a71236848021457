"""Generates tests/golden/beam_pins.npz + beam_pins.json: outputs of the REFERENCE'S OWN beam search (lcasr/ctc_beam_search.py:
Beam, LanguageModel, BeamSearch), pulled out with `ast` and executed UNCHANGED, configured as reference lcasr/lib.py:37-72
load_beamsearch configures it (blank_id = vocab size, max_cache_length = 128).

Leaves bound by this script (what the pins do NOT cover): `transformer_lm` is the CPU float32 restatement of this package's LM
(tests/lm_cpu.py, toy size, weights from the seed and config stored in the json — numpy RandomState is bit-stable), `exists`
is `x is not None`, tqdm and einops are the installed packages.  The tokenizer is tests/golden/tokenizer_128.model (no BOS:
bos_id 0, as the package resolves it).
What the pins DO cover: candidate selection, the CTC prefix rules, merge arithmetic and order, the stable top-k, prune_less_than,
grab_state / trim_cache to 128 and the batching of the LM calls, as the reference wrote them.
Cases with an LM term (alpha != 0) are kept only when their beams are unchanged under +-1e-5 noise on the LM log-probs.
Run once where the reference tree is available:  python tests/golden/make_beam_pins.py --reference DIR"""
import argparse
import ast
import heapq
import json
import math
import os
import sys
import time
from typing import Dict, List, Optional, Tuple, Union  # noqa: F401  (annotations of the extracted code)

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

LM_CFG = dict(n_layers=2, d_model=256, n_heads=2, ff_mult=2, max_positions=129, norm_eps=1e-5)
LM_SEED = 7
V = 128


def extract(ref):
    src = open(os.path.join(ref, 'lcasr', 'ctc_beam_search.py')).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ('Beam', 'LanguageModel', 'BeamSearch')]
    assert len(keep) == 3
    from einops import rearrange, repeat
    from tqdm import tqdm
    ns = dict(torch=torch, np=np, math=math, heapq=heapq, time=time, tqdm=tqdm, rearrange=rearrange, repeat=repeat,
              exists=lambda x: x is not None, transformer_lm=object, List=List, Dict=Dict, Tuple=Tuple, Optional=Optional,
              Union=Union)
    exec(compile(ast.Module(body=keep, type_ignores=[]), 'ctc_beam_search.py', 'exec'), ns)
    return ns


def peaked(T, seed, branch=0.25, blank_p=0.45, temp=1.0):
    """Synthetic CTC log-probs [T, V+1] (float32): a random path of tokens / blanks with a peak each frame, a runner-up peak on
    `branch` of the frames so beams compete."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, V + 1, generator=g) * 0.5
    r = torch.rand(T, generator=g)
    tok = torch.randint(1, V, (T,), generator=g)
    alt = torch.randint(1, V + 1, (T,), generator=g)
    for t in range(T):
        top = V if r[t] < blank_p else int(tok[t])
        x[t, top] += 7.0 / temp
        if torch.rand(1, generator=g).item() < branch:
            x[t, int(alt[t])] += 6.0 / temp
    x[:, 0] -= 4.0                      # token 0 rarely competes
    return x.log_softmax(-1)


class Noisy:
    def __init__(self, lm, amp, seed):
        self.lm, self.amp, self.g = lm, amp, torch.Generator().manual_seed(seed)
        self.bos_id = lm.bos_id

    def get_initial_state(self):
        lp, st = self.lm.get_initial_state()
        return lp + self.amp * (2 * torch.rand(lp.shape, generator=self.g) - 1), st

    def __call__(self, *a, **k):
        lp, st = self.lm(*a, **k)
        return lp + self.amp * (2 * torch.rand(lp.shape, generator=self.g) - 1), st


def run(ns, tok, lm, lp, width, alpha, beta, prune):
    bs = ns['BeamSearch'](tokenizer=tok, beam_width=width, log_probs=lp, language_model=lm, blank_id=tok.vocab_size(), alpha=alpha,
                          beta=beta, debug=False, prune_less_than_val=prune, top_am_threshold=-6, max_cache_length=128)
    bs.run_search(use_tqdm=False)
    return bs


def summary(bs):
    return [{'lm_sequence': [int(x) for x in b.lm_sequence], 'am_sequence': [(-1 if x is None else int(x)) for x in b.am_sequence],
             'score': float(b.score)} for b in bs.beams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    ns = extract(args.reference)
    import sentencepiece as spm
    from lm_cpu import CpuLM
    from dynamic_asr_eval_amd.lm import synthetic_state
    tok = spm.SentencePieceProcessor(model_file=os.path.join(HERE, 'tokenizer_128.model'))
    assert tok.vocab_size() == V
    bos = tok.bos_id() if tok.bos_id() >= 0 else 0
    model = CpuLM(LM_CFG, V, synthetic_state(LM_CFG, V, LM_SEED))
    lm = ns['LanguageModel'](model=model, bos_id=bos, device='cpu')

    # LM logits: the initial state and one padded batch step whose rows have trimmed (128) and short caches
    init_lp, _ = lm.get_initial_state()
    seq = [int(x) for x in torch.randint(1, V, (140,), generator=torch.Generator().manual_seed(3))]
    grab = ns['BeamSearch'](tokenizer=tok, beam_width=1, log_probs=None, language_model=lm, max_cache_length=128)
    states, _ = [], None
    _, st = lm.get_initial_state()
    prefix_states = {0: st}
    for n, tkn in enumerate(seq):
        lps, st = lm(torch.tensor([[tkn]]), torch.LongTensor([1]), st)
        st = grab.grab_state(st, 0)
        prefix_states[n + 1] = st
    rows = [(140, 17), (5, 33), (128, 90), (0, 2)]       # (tokens already processed after bos, next token)
    caches = [rearrange_cache(prefix_states[n]['cache']) for n, _ in rows]
    L, KV, _, H, N, D = prefix_states[0]['cache'].shape
    padded = torch.nn.utils.rnn.pad_sequence(caches, batch_first=True, padding_value=0)
    from einops import rearrange
    padded = rearrange(padded, 'nb n (l kv b h) d -> l kv (b nb) h n d', l=L, kv=KV, h=H, d=D)
    batch_state = {'cache': padded, 'cache_lengths': torch.cat([prefix_states[n]['cache_lengths'] for n, _ in rows])}
    batch_lp, _ = lm(torch.tensor([[t] for _, t in rows]), torch.LongTensor([1] * len(rows)), batch_state)

    cases, arrays = [], {'lm_init': init_lp.numpy().astype(np.float32), 'lm_batch': batch_lp[:, -1].numpy().astype(np.float32),
                         'lm_seq': np.array(seq, np.int32), 'lm_rows': np.array(rows, np.int32)}
    specs = [
        dict(name='w1_a0', T=64, seed=1, width=1, alpha=0.0, beta=1.625, prune=None),
        dict(name='w3_a0', T=160, seed=2, width=3, alpha=0.0, beta=1.625, prune=None),
        dict(name='w3_a0_prune', T=160, seed=3, width=3, alpha=0.0, beta=1.625, prune=3.221),
        dict(name='w20_a0', T=120, seed=4, width=20, alpha=0.0, beta=1.625, prune=None),
        dict(name='w20_a0_prune', T=200, seed=5, width=20, alpha=0.0, beta=1.625, prune=3.221),
        dict(name='w20_a0_trim', T=600, seed=6, width=20, alpha=0.0, beta=1.625, prune=3.221, blank_p=0.1),
        dict(name='w3_lm', T=120, seed=7, width=3, alpha=0.4016, beta=1.625, prune=None),
        dict(name='w20_lm_prune', T=160, seed=8, width=20, alpha=0.4016, beta=1.625, prune=3.221),
        dict(name='w20_lm_trim', T=400, seed=9, width=20, alpha=0.4016, beta=1.625, prune=3.221, blank_p=0.1),
        dict(name='w1_lm', T=100, seed=10, width=1, alpha=0.4016, beta=1.625, prune=3.221),
        dict(name='w20_a0_numpy', T=100, seed=11, width=20, alpha=0.0, beta=1.625, prune=3.221, numpy=True),
    ]
    for s in specs:
        lp = peaked(s['T'], s['seed'], blank_p=s.get('blank_p', 0.45))
        feed = lp.numpy() if s.get('numpy') else lp
        bs = run(ns, tok, lm, feed, s['width'], s['alpha'], s['beta'], s['prune'])
        out = summary(bs)
        sc = [b['score'] for b in out]
        margin = min([a - b for a, b in zip(sc, sc[1:])] or [float('inf')])
        if s['alpha'] != 0.0:
            stable = True
            for amp_seed in (1, 2):
                alt = summary(run(ns, tok, Noisy(lm, 1e-5, amp_seed), feed, s['width'], s['alpha'], s['beta'], s['prune']))
                if [b['lm_sequence'] for b in alt] != [b['lm_sequence'] for b in out] or \
                        [b['am_sequence'] for b in alt] != [b['am_sequence'] for b in out]:
                    stable = False
            if not stable:
                print(f"{s['name']}: dropped (beams change under 1e-5 LM noise)")
                continue
        emitted = max(len(b['lm_sequence']) - 1 for b in out)
        arrays['lp_' + s['name']] = lp.numpy().astype(np.float32)
        cases.append(dict(s, beams=out, text=bs.return_text(0), min_margin=margin, max_emitted=emitted,
                          score_types=type(bs.beams[0].score).__name__))
        print(f"{s['name']}: {len(out)} beams, top {out[0]['score']:.6f}, emitted <= {emitted}, margin {margin:.3g}")
    np.savez_compressed(os.path.join(HERE, 'beam_pins.npz'), **arrays)
    with open(os.path.join(HERE, 'beam_pins.json'), 'w') as f:
        json.dump({'lm_config': LM_CFG, 'lm_seed': LM_SEED, 'vocab': V, 'bos_id': bos, 'top_am_threshold': -6,
                   'max_cache_length': 128, 'torch': torch.__version__, 'numpy': np.__version__, 'cases': cases}, f, indent=0)


def rearrange_cache(cache):
    from einops import rearrange
    return rearrange(cache, 'l kv b h n d -> n (l kv b h) d')


if __name__ == '__main__':
    main()
