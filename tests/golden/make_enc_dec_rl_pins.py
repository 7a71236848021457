"""Generates tests/golden/enc_dec_rl_pins.json: outputs of the REFERENCE'S OWN `update_grpo`, `update_maxrl` and `generate_enc_dec`
(lcasr/lib.py:1400-1472,1172-1226), pulled out of the reference file with `ast` and executed UNCHANGED, at generation time only.
Outputs only are stored.

  (a) weights: `_policy_forward` is a stub that returns a seeded leaf tensor log_probs [R, Lmax] and the mask of the given lengths;
      recorded are the loss and d(loss)/d(log_probs) of both update functions: GRPO with / without std normalisation, MaxRL at
      several thresholds incl. both skip cases (None), unequal lengths incl. a zero-length hypothesis (one eos target).
  (b) retire: the reference's generate loop against a stub model (zero logits) and a scripted `torch.multinomial` (a row is
      recognised by its first token, unique per row): eos at step 0, a row that runs into max_generate, rows finishing at different
      steps.  The reference returns rows in finishing order; they are stored in ROW order.

Run once in the build container: `python tests/golden/make_enc_dec_rl_pins.py`."""
import contextlib
import io
import json
import os
import sys
import types
from typing import List

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_reference_pins import ref_functions  # noqa: E402

WEIGHT_CASES = [
    # (rewards, hypothesis lengths, mode, kwargs)
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "grpo", dict(normalize_std=True)),
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "grpo", dict(normalize_std=False)),
    ([-6.0, 1.0, -2.0, 1.0], [6, 0, 2, 0], "grpo", dict(normalize_std=True)),
    ([0.3, 0.3, 0.8, 0.1], [4, 4, 4, 4], "grpo", dict(normalize_std=True)),
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "maxrl", dict(success_threshold=0.9)),
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "maxrl", dict(success_threshold=0.5)),
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "maxrl", dict(success_threshold=0.3)),
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "maxrl", dict(success_threshold=0.99)),     # pass rate 0: skip
    ([0.15, 0.95, 0.4, 0.62], [7, 0, 3, 5], "maxrl", dict(success_threshold=0.1)),      # pass rate 1: skip
    ([0.2, 0.9], [0, 11], "maxrl", dict(success_threshold=0.9)),
]
RETIRE_CASES = [
    # (max_generate, draws[t][r]); the first draw of a row that survives step 0 is unique to the row
    (4, [[0, 11, 12, 13], [0, 21, 0, 23], [0, 31, 0, 0], [0, 41, 0, 0], [0, 51, 0, 0], [0, 61, 0, 0]]),
    (3, [[11, 12, 13], [0, 22, 23], [0, 32, 33], [0, 42, 43], [0, 52, 53]]),
    (6, [[11, 0, 13, 14], [21, 0, 0, 24], [0, 0, 0, 34], [0, 0, 0, 0]]),
    (2, [[0, 0], [5, 5]]),
]


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def weight_pins():
    out = []
    for i, (rewards, lengths, mode, kw) in enumerate(WEIGHT_CASES):
        R, Lmax = len(lengths), max(lengths) + 1
        g = torch.Generator().manual_seed(100 + i)
        log_probs = (-torch.rand(R, Lmax, generator=g) * 4).requires_grad_(True)
        mask = torch.arange(Lmax)[None, :] < (torch.tensor(lengths) + 1)[:, None]
        ns = ref_functions("lcasr/lib.py", ["update_grpo", "update_maxrl"],
                           {"torch": torch, "List": List, "_policy_forward": lambda model, audio, tok, hyps: (log_probs, mask)})
        loss = quiet(ns["update_" + mode], None, None, None, [""] * R, rewards, **kw)
        rec = dict(rewards=rewards, lengths=lengths, mode=mode, kwargs=kw, log_probs=log_probs.detach().tolist())
        if loss is None:
            rec.update(loss=None, grad=None)
        else:
            loss.backward()
            rec.update(loss=float(loss), grad=log_probs.grad.tolist())
        out.append(rec)
    return out


def retire_pins():
    out = []
    for max_generate, draws in RETIRE_CASES:
        n_rows = len(draws[0])
        state = dict(t=0, tokens=None)
        first = {draws[0][r]: r for r in range(n_rows)}

        def decoder(tokens, a_hidden, a_lengths):
            state["tokens"] = tokens
            return {"logits": torch.zeros(tokens.shape[0], tokens.shape[1], 8)}

        def multinomial(probs, num_samples=1):
            tok, t = state["tokens"], state["t"]
            rows = list(range(n_rows)) if t == 0 else [first[int(tok[i, 1])] for i in range(tok.shape[0])]
            assert len(rows) == probs.shape[0]
            step = draws[t] if t < len(draws) else [0] * n_rows
            state["t"] += 1
            return torch.LongTensor([[step[r]] for r in rows])

        model = types.SimpleNamespace(forward=lambda audio_signal: {"a_hidden": torch.zeros(1, 2, 3), "length": torch.LongTensor([2])},
                                      language_model_decoder=decoder)
        shim = types.SimpleNamespace(LongTensor=torch.LongTensor, cat=torch.cat, nn=torch.nn, multinomial=multinomial)
        ns = ref_functions("lcasr/lib.py", ["generate_enc_dec"], {"torch": shim})
        seqs, _, lens = ns["generate_enc_dec"](model, None, max_generate=max_generate, sample=n_rows, greedy=False)
        rows = [None] * n_rows
        empty = [r for r in range(n_rows) if draws[0][r] == 0]
        for q, n in zip(seqs.tolist(), lens.tolist()):
            q = q[:n]
            r = first[q[0]] if q else empty.pop(0)
            assert rows[r] is None
            rows[r] = q
        out.append(dict(max_generate=max_generate, draws=draws, rows=rows))
    return out


if __name__ == "__main__":
    pins = dict(weights=weight_pins(), retire=retire_pins())
    path = os.path.join(HERE, "enc_dec_rl_pins.json")
    json.dump(pins, open(path, "w"), indent=0)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; retire rows: {[p['rows'] for p in pins['retire']]}")
