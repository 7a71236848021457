"""Generates tests/golden/consistency_pins.npz + consistency_pins.json: outputs of the REFERENCE'S OWN consistency loop
(lcasr/lib.py:646-903), pulled out of the reference file with `ast` and executed UNCHANGED, at generation time only.

  (a) mixa_*: the statements lib.py:817-841 (the distance-decayed gradient mix) over a small synthetic `param_collections`
      (W = 7 and W = 40 windows, four tensors of different shapes, the last one without a gradient in every window).
      Stored as banks [W, P] before and after; the columns of the tensor without a gradient hold a sentinel that must survive.
  (b) loop_*: the whole function `dynamic_eval_consistency_ctc_loss` over the oracle's tiny conformer and the 128-piece tokenizer, with
      the stand-in namespace of make_loop_pins.py (SpecAugment -> content-derived stored masks, GreedyCTCDecoder -> the oracle's greedy
      ids, tqdm -> identity; `optim.Adafactor` is torch's own): epochs=2 offline, epochs=2 online, epochs=1 offline.  Recorded: the
      pseudo-label ids of every step, after each epoch a digest (every 61st element, sum, absolute sum) of the mixed gradients and of
      every window's parameters, the returned log-probs and a digest of `return_params`.

GPU semantics of the load at lib.py:765-766.  On a CPU model `p_cur.data.to(p.device, dtype)` returns the SAME storage, so the model
would alias the window's set and the later optimiser step would change the model too; on a GPU the load is a host-to-device copy.
(b) therefore runs under a TorchFunctionMode that turns a `Tensor.to` which would return its own storage into a clone, so the pins
carry what the reference computes with the model on a GPU.  Run once in the build container: `python tests/golden/make_consistency_pins.py`."""
import json
import os
import platform
import random
import sys
import time
import types
from typing import Callable, Dict, List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_reference_pins import ref_functions, ref_statements  # noqa: E402
from loop_pin_cases import (OracleGreedyCTCDecoder, StoredMaskSpecAugment, quiet, tokenizer_128, toy_args, toy_model,
                            VOCAB, TOY)  # noqa: E402

MIX_SHAPES = [(5, 7), (11,), (2, 3, 4), (6,)]          # the last tensor has no gradient in any window
MIX_WINDOWS = (7, 40)
DIGEST_STRIDE = 61
LOOP_CASES = {
    # tag: (spec frames, seq_len, overlap, args)
    "e2_offline": (1100, 512, 256, dict(epochs=2)),
    "e2_online": (1100, 512, 256, dict(epochs=2, online=True)),
    "e1_offline": (1100, 512, 256, dict(epochs=1)),
}


class ToCopies(TorchFunctionMode):
    """A same-device, same-dtype `Tensor.to` returns a clone (what a host-to-device load does), not the tensor's own storage."""

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is torch.Tensor.to and isinstance(out, torch.Tensor) and out.numel() and out.data_ptr() == args[0].data_ptr():
            out = out.clone()
        return out


def mix_collections_case(W, seed):
    g = torch.Generator().manual_seed(seed)
    keys = [k * 256 for k in range(W)]
    cols = {}
    for k in keys:
        ps = []
        for z, shape in enumerate(MIX_SHAPES):
            p = torch.zeros(shape, requires_grad=True)
            if z != len(MIX_SHAPES) - 1:
                p.grad = torch.randn(shape, generator=g) * (10.0 ** float(torch.randint(-6, 2, (1,), generator=g)))
            ps.append(p)
        cols[k] = ps
    return keys, cols


def bank_of(keys, cols, sentinel):
    rows = []
    for k in keys:
        rows.append(torch.cat([(q.grad if q.grad is not None else torch.full(q.shape, sentinel)).reshape(-1) for q in cols[k]]))
    return torch.stack(rows).numpy().copy()


def digest(tensors):
    flat = torch.cat([t.detach().reshape(-1) for t in tensors])
    return flat[::DIGEST_STRIDE].numpy().copy(), [float(flat.double().sum()), float(flat.double().abs().sum())]


def main():
    arrays = {}
    meta = {"source": "reference lcasr/lib.py:646-903 executed unchanged via ast extraction (tests/golden/make_consistency_pins.py); the load at "
                      ":765-766 made a copy (GPU semantics) by a TorchFunctionMode; leaf classes bound as in make_loop_pins.py",
            "machine": {"cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "threads": torch.get_num_threads()},
            "toy": TOY, "vocab": VOCAB, "digest_stride": DIGEST_STRIDE, "mix_shapes": [list(s) for s in MIX_SHAPES]}
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            meta["machine"]["cpu"] = line.split(":", 1)[1].strip()
            break

    # ---- (a) the mix statements
    code = ref_statements("lcasr/lib.py", 817, 841)
    meta["mix"] = {}
    for W in MIX_WINDOWS:
        keys, cols = mix_collections_case(W, seed=500 + W)
        arrays[f"mixa_W{W}_in"] = bank_of(keys, cols, sentinel=123.5)
        env = {"torch": torch, "param_collections": cols, "training_keys": list(reversed(keys)), "precision": torch.float32}
        exec(code, env)
        arrays[f"mixa_W{W}_out"] = bank_of(keys, cols, sentinel=123.5)
        assert not np.array_equal(arrays[f"mixa_W{W}_in"], arrays[f"mixa_W{W}_out"])
        meta["mix"][str(W)] = {"seed": 500 + W, "keys": keys, "sentinel": 123.5}

    # ---- (b) the whole function
    tok = tokenizer_128()
    record = {}

    class RecordingDecoder(OracleGreedyCTCDecoder):
        def __call__(self, log_probs, decode=True):
            text = super().__call__(log_probs, decode)
            record["calls"].append(list(self.tokenizer.encode(text)))
            return text

    class RecordingAdafactor(torch.optim.Adafactor):
        """Every window's optimiser steps once per epoch, in key order: before the step its set holds the mixed gradients."""

        def step(self, closure=None):
            ps = [p for g in self.param_groups for p in g["params"]]
            record["grads"].append([p.grad.detach().clone() for p in ps if p.grad is not None])
            out = super().step(closure)
            record["params"].append([p.detach().clone() for p in ps])
            return out

    base = {"torch": torch, "nn": nn, "optim": optim, "F": F, "random": random, "time": time, "Callable": Callable, "Dict": Dict,
            "List": List, "tqdm": lambda it, **k: it, "madgrad": types.SimpleNamespace(MADGRAD=None),
            "SpecAugment": StoredMaskSpecAugment, "GreedyCTCDecoder": RecordingDecoder}
    names = ["prepare_chunks", "get_specaugment_config_from_args", "get_frame_shuffle_config_from_args", "get_lr_args_from_args",
             "get_cutout_params_from_args", "frame_shuffle", "add_random_noise", "cutout", "dynamic_eval_consistency_ctc_loss"]
    ns = ref_functions("lcasr/lib.py", names, base)
    meta["loop"] = {}
    for tag, (T, seq_len, overlap, kw) in LOOP_CASES.items():
        model = toy_model(seed=21)
        spec = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(100 + T))
        before = [p.clone() for p in model.parameters()]
        record.update(calls=[], grads=[], params=[])
        random.seed(7); torch.manual_seed(9)
        with ToCopies():
            out, params = quiet(ns["dynamic_eval_consistency_ctc_loss"], toy_args(**kw), model, spec, seq_len, overlap, tok, use_tqdm=False,
                                optim=RecordingAdafactor, return_params=True)
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())), "the reference restores the weights (lib.py:899-900)"
        n_win = len(record["params"]) // kw["epochs"]
        labels = record["calls"][0::2]                  # the decoder runs on the clean copy, then on the noisy one (lib.py:773,779)
        assert len(labels) == n_win * kw["epochs"]
        arrays[f"loop_{tag}_out"] = out
        arrays[f"loop_{tag}_ret"], ret_sum = digest(params)
        sums = {"grads": [], "params": []}
        for e in range(kw["epochs"]):
            for what in ("grads", "params"):
                per_window = record[what][e * n_win:(e + 1) * n_win]
                d = [digest(ts) for ts in per_window]
                arrays[f"loop_{tag}_{what}_e{e}"] = np.stack([a for a, _ in d])
                sums[what].append([s for _, s in d])
        meta["loop"][tag] = {"frames": T, "seq_len": seq_len, "overlap": overlap, "args": kw, "spec_seed": 100 + T, "model_seed": 21,
                             "windows": n_win, "labels": labels, "rows": int(out.shape[0]), "ret_sum": ret_sum, "sums": sums}
    e1 = arrays["loop_e1_offline_out"]
    assert np.isfinite(e1).any()

    np.savez_compressed(os.path.join(HERE, "consistency_pins.npz"), **arrays)
    json.dump(meta, open(os.path.join(HERE, "consistency_pins.json"), "w"), indent=1)
    print("consistency pins written:", len(arrays), "arrays,", sum(a.nbytes for a in arrays.values()) // 1024, "KiB raw")


if __name__ == "__main__":
    main()
