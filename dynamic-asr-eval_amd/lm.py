"""Transformer LM of the CTC + LM beam search (reference lcasr/ctc_beam_search.py LanguageModel; the model itself,
`lming.models.transformer.transformer_lm`, is not vendored, so its architecture here is this package's choice).

Decoder-only pre-LN transformer with self-attention only: the layer shapes of enc_dec.decoder_spec without the cross block.
  x = embed[token] + sinusoidal_position[p]
  per layer: x += out(attn(qkv(LN(x))));  x += w2(silu(w1(LN(x))))
  log_softmax(head(LN_out(x)))   (temperature 1)
State contract (LanguageModel / BeamSearch.grab_state / trim_cache with max_cache_length = 128): a beam's state is the K/V of at
most 128 tokens; a new token attends to that history plus itself and its position index is the history length before the step,
which stays at 128 once the cache is trimmed (the reference's LM is not vendored: this indexing is this package's definition).
The arithmetic runs in csrc/beam_search.hip; this module keeps the config, the parameter spec, seeded synthetic weights and the
checkpoint loader.  No torch arithmetic: weights are built with numpy and uploaded."""
import math

import numpy as np
import torch

DEFAULT_LM_CONFIG = dict(n_layers=6, d_model=768, n_heads=6, ff_mult=4, max_positions=129, norm_eps=1e-5)
MAX_CACHE_LENGTH = 128          # load_beamsearch (reference lib.py:69)


def lm_spec(cfg, vocab):
    """[(name, shape)] in the order of the C-ABI pointer table (include/dyneval.h, dyn_beam_search)."""
    d, ff = cfg['d_model'], cfg['d_model'] * cfg['ff_mult']
    spec = [('embed.weight', (vocab, d)), ('norm_out.weight', (d,)), ('norm_out.bias', (d,)), ('head.weight', (vocab, d)),
            ('head.bias', (vocab,))]
    for l in range(cfg['n_layers']):
        p = f'layers.{l}.'
        spec += [(p + 'self.norm.weight', (d,)), (p + 'self.norm.bias', (d,)), (p + 'self.qkv.weight', (3 * d, d)),
                 (p + 'self.qkv.bias', (3 * d,)), (p + 'self.out.weight', (d, d)), (p + 'self.out.bias', (d,)),
                 (p + 'ff.norm.weight', (d,)), (p + 'ff.norm.bias', (d,)), (p + 'ff.w1.weight', (ff, d)), (p + 'ff.w2.weight', (d, ff))]
    return spec


def positions(n, d):
    """Sinusoidal table [n, d] (float64 -> float32 once), the same formula as enc_dec.sinusoidal_positions."""
    pos = np.arange(n, dtype=np.float64)[:, None]
    inv = np.exp(np.arange(0, d, 2, dtype=np.float64) * (-math.log(10000.0) / d))
    tab = np.zeros((n, d), dtype=np.float64)
    tab[:, 0::2] = np.sin(pos * inv)
    tab[:, 1::2] = np.cos(pos * inv)
    return tab.astype(np.float32)


def synthetic_state(cfg, vocab, seed=0):
    """Seeded synthetic weights {name: float32 ndarray}: normal(0, 1/sqrt(fan_in)) matrices, unit LayerNorm gains, small biases."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in lm_spec(cfg, vocab):
        if name.endswith('norm.weight') or name.endswith('norm_out.weight'):
            a = 1.0 + 0.05 * rng.standard_normal(shape)
        elif len(shape) == 1:
            a = 0.02 * rng.standard_normal(shape)
        elif name == 'embed.weight':
            a = rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / math.sqrt(shape[1])
        out[name] = a.astype(np.float32)
    return out


def strip_ddp(state):
    """convert_from_ddp: drop the `module.` prefix of DistributedDataParallel checkpoints."""
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state.items()}


def load_checkpoint(path, allow_missing=False):
    """{'model': state_dict, 'config': {...}} -> (config, {name: float32 ndarray}).  Missing / unexpected keys are reported the way
    run_dynamic_eval_full.load_model_and_tokenizer does: missing ones are an error unless allow_missing (then zero)."""
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    cfg = dict(DEFAULT_LM_CONFIG)
    cfg.update({k: v for k, v in dict(ckpt.get('config', {})).items() if k in DEFAULT_LM_CONFIG})
    return cfg, _match(cfg, strip_ddp(ckpt['model']), path, allow_missing)


def _match(cfg, state, what, allow_missing, vocab=None):
    if vocab is None:
        if 'embed.weight' not in state:
            raise KeyError(f'LM checkpoint {what}: no embed.weight, the vocabulary size is unknown')
        vocab = int(state['embed.weight'].shape[0])
    spec = dict(lm_spec(cfg, vocab))
    missing = [k for k in spec if k not in state]
    unexpected = [k for k in state if k not in spec]
    if missing or unexpected:
        msg = (f'LM checkpoint {what}: {len(missing)} parameters are missing (e.g. {missing[:3]}), '
               f'{len(unexpected)} checkpoint keys are unknown (e.g. {unexpected[:3]})')
        if missing and not allow_missing:
            raise KeyError(msg + '; pass `-kwargs allow_missing=True` to run with the missing tensors left at zero')
        print('WARNING: ' + msg)
    out = {}
    for k, shape in spec.items():
        a = np.zeros(shape, np.float32) if k not in state else np.asarray(
            state[k].detach().cpu().numpy() if hasattr(state[k], 'detach') else state[k], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f'LM checkpoint {what}: {k} has shape {tuple(a.shape)}, expected {tuple(shape)}')
        out[k] = a
    return out


class TransformerLM:
    """The LM's weights on one device plus the host pointer table the HIP entry points take."""

    def __init__(self, cfg, vocab, state, device):
        import ctypes
        self.cfg, self.vocab, self.device = dict(cfg), int(vocab), torch.device(device)
        d = cfg['d_model']
        if d % cfg['n_heads']:
            raise ValueError(f'LM d_model {d} is not a multiple of n_heads {cfg["n_heads"]}')
        self.d_model, self.heads, self.d_ff, self.layers = d, cfg['n_heads'], d * cfg['ff_mult'], cfg['n_layers']
        self.max_positions, self.eps = int(cfg['max_positions']), float(cfg['norm_eps'])
        self.params = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in state.items()}
        self.pos_table = torch.from_numpy(positions(self.max_positions, d)).to(self.device)
        P = self.params
        order = [P['embed.weight'], self.pos_table, P['norm_out.weight'], P['norm_out.bias'], P['head.weight'], P['head.bias']]
        for l in range(self.layers):
            p = f'layers.{l}.'
            order += [P[p + n] for n in ('self.norm.weight', 'self.norm.bias', 'self.qkv.weight', 'self.qkv.bias', 'self.out.weight',
                                         'self.out.bias', 'ff.norm.weight', 'ff.norm.bias', 'ff.w1.weight', 'ff.w2.weight')]
        self.ptrs = (ctypes.c_void_p * len(order))(*[t.data_ptr() for t in order])

    def weight_bytes(self):
        return sum(t.numel() * 4 for t in self.params.values())

    def dims(self):
        return (self.layers, self.d_model, self.heads, self.d_ff, self.vocab, self.max_positions, self.eps)

    @classmethod
    def synthetic(cls, vocab, device, cfg=None, seed=0):
        cfg = dict(cfg or DEFAULT_LM_CONFIG)
        return cls(cfg, vocab, synthetic_state(cfg, vocab, seed), device)

    @classmethod
    def from_checkpoint(cls, path, vocab, device, allow_missing=False):
        cfg, state = load_checkpoint(path, allow_missing)
        if state['embed.weight'].shape[0] != vocab:
            raise ValueError(f'LM checkpoint {path}: vocabulary {state["embed.weight"].shape[0]} != tokenizer vocabulary {vocab}')
        return cls(cfg, vocab, state, device)
