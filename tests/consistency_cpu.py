"""CPU restatement, in plain PyTorch, of the reference's consistency loop `dynamic_eval_consistency_ctc_loss` (reference
lcasr/lib.py:646-903) over the oracle's tiny conformer: test infrastructure only, never imported by the product path.

  one parameter set and one optimiser per window          lib.py:732-737
  per window: load its set, forward on [augmented, clean], greedy pseudo-label of the clean copy, CTC loss of the augmented copy
              / (N * B), backward, the gradient STORED in the window's set, no step                                   :751-813
  after the windows of an epoch: the distance-decayed mix over the sorted keys, in place and sequential in i            :817-841
  every window's optimiser steps its own set                                                                            :845-848
  offline final pass with whatever set was loaded last (the load at :861 is discarded)                                  :852-875
  stitch, restore                                                                                                       :878-903
The load at :765-766 is a COPY here, as it is for a model on a GPU (on a CPU model the reference's `.to()` aliases the window's set);
tests/golden/consistency_pins.* were generated with the same semantics (see make_consistency_pins.py)."""
import random

import numpy as np
import torch

from oracle import dynamic_eval_ref as R

DECAY_PER_DISTANCE = 0.95


def mix_bank(bank, decay_per_distance=DECAY_PER_DISTANCE):
    """The statements of lib.py:817-841 on a gradient bank [W, ...] (row = window in key order), in place; -> bank."""
    W = bank.shape[0]
    for i in range(W):
        cur_grad = bank[i].clone().to(dtype=torch.float64)
        total_sum = 1
        for q in range(W):
            if q == i:
                continue
            decay = decay_per_distance ** abs(i - q)
            total_sum += decay
            cur_grad += (decay * bank[q].clone()).to(dtype=torch.float64)
        bank[i] = (cur_grad / total_sum).to(dtype=bank.dtype)
    return bank


def mix_collections(grads):
    """`grads`: {window key: [gradient or None per parameter]}; mixed in place over the sorted keys."""
    keys = sorted(grads)
    for z in range(len(grads[keys[0]])):
        if grads[keys[0]][z] is None:
            continue
        bank = torch.stack([grads[k][z] for k in keys])
        mix_bank(bank)
        for w, k in enumerate(keys):
            grads[k][z] = bank[w].clone()
    return grads


def consistency_ref(model, spec, seq_len, overlap, tokenizer, optimizer_cls=torch.optim.Adafactor, lr_args=None, epochs=1, shuffle=False,
                    online=False, downsampling_factor=8, fixed_masks=None, zero_masking=False, return_params=False, trace=None):
    """-> log-probs [T_ds, V+1] (and the parameters the reference returns).  `trace`: dict receiving 'labels' [(epoch, key, ids)] and per
    epoch 'grads' / 'params' = {key: [tensor or None per parameter]} (the mixed gradients; every window's set after the steps).
    A float64 model / spectrogram runs everything in float64."""
    lr_args = dict(lr_args or {})
    lr_args.setdefault('lr', 9e-5)
    dtype = spec.dtype
    spec_n = spec.shape[-1]
    params = list(model.parameters())
    original_model_params = [p.clone().detach() for p in params]
    blank = model.decoder.num_classes - 1
    ctc_loss_fn = torch.nn.CTCLoss(blank=blank, reduction='sum')
    if seq_len > spec_n:
        seq_len, overlap = spec_n, 0
    assert overlap / downsampling_factor == overlap // downsampling_factor
    all_logits = torch.zeros((1, spec_n // 4 + seq_len, tokenizer.vocab_size() + 1), dtype=dtype)
    logit_count = torch.zeros_like(all_logits)
    loop_epochs = epochs
    shuffle = False if online else shuffle
    model_outputs = {}
    model.eval()
    training_data, training_keys = R.prepare_chunks(spec, seq_len, overlap)
    param_collections = {key: [p.detach().clone().requires_grad_(p.requires_grad) for p in params] for key in training_keys}
    optim_collections = {key: optimizer_cls(param_collections[key], **lr_args) for key in training_keys}
    for epoch in range(loop_epochs):
        training_keys = list(training_data.keys())
        training_keys = random.sample(training_keys, len(training_keys)) if shuffle else training_keys
        for i in training_keys:
            audio_chunk = training_data[i].clone().repeat(2, 1, 1)
            u_len = audio_chunk.shape[-1]
            if fixed_masks is not None:
                R.apply_masks(audio_chunk[0], fixed_masks[i], zero_masking)
            for p, p_cur in zip(params, param_collections[i]):
                p.data = p_cur.data.clone()                                   # the load is a copy (GPU semantics)
            out = model(audio_signal=audio_chunk)
            pseudo_ids = R.greedy_ctc_ids(out['final_posteriors'][-1].detach(), blank)
            target_ids = tokenizer.encode(tokenizer.decode(pseudo_ids))
            if trace is not None:
                trace.setdefault('labels', []).append((epoch, i, list(target_ids)))
            pseudo_targets = torch.LongTensor(target_ids).unsqueeze(0)
            augmented_outs = out['final_posteriors'][:1]
            N, B = augmented_outs.shape[1], augmented_outs.shape[0]
            loss = ctc_loss_fn(augmented_outs.transpose(0, 1), pseudo_targets, torch.LongTensor([N] * B),
                               torch.LongTensor([pseudo_targets.shape[1]] * B)) / (N * B)
            loss.backward()
            for p, p_at_i in zip(params, param_collections[i]):
                if p.grad is None:
                    p_at_i.grad = None
                    continue
                p_at_i.grad = p.grad.clone()
                p.grad.zero_()
            if online:
                logits = torch.exp(out['final_posteriors'][-1].detach())
                ds_len = logits.shape[-2]
                model_outputs[i] = {'logits': logits, 'ds_len': ds_len, 'overlap_ds': int(overlap / (u_len / ds_len))}
        with torch.no_grad():
            grads = {k: [q.grad for q in param_collections[k]] for k in param_collections}
            mix_collections(grads)
            for k in param_collections:
                for q, g in zip(param_collections[k], grads[k]):
                    if g is not None:
                        q.grad.data = g
        if trace is not None:
            trace.setdefault('grads', []).append({k: [None if q.grad is None else q.grad.clone() for q in param_collections[k]]
                                                  for k in param_collections})
        for opt in optim_collections.values():
            opt.step()
            opt.zero_grad()
        if trace is not None:
            trace.setdefault('params', []).append({k: [q.detach().clone() for q in param_collections[k]] for k in param_collections})
    if not online:
        model.eval()
        training_data, training_keys = R.prepare_chunks(spec, seq_len, overlap)
        for i in training_keys:
            audio_chunk = training_data[i].clone()
            u_len = audio_chunk.shape[-1]
            with torch.no_grad():
                out = model(audio_signal=audio_chunk)
            logits = torch.exp(out['final_posteriors'][0].detach())
            ds_len = logits.shape[-2]
            model_outputs[i] = {'logits': logits, 'ds_len': ds_len, 'overlap_ds': int(overlap / (u_len / ds_len))}
    logits = R.stitch_ref(model_outputs, all_logits, logit_count)
    updated = [p.clone().detach() for p in params]
    for p, p_orig in zip(params, original_model_params):
        p.data = p_orig.data
        p.grad = None
    out = logits.squeeze(0).numpy().astype(np.float64 if dtype == torch.float64 else np.float32)
    return (out, updated) if return_params else out
