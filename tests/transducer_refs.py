"""References for the transducer tests: a float64 restatement of transformers' `tdt_loss` with its lattice (alpha, beta) and the gradient in
closed form from the arc posteriors (transformers' function casts to fp32 internally, so it cannot serve as the float64 reference; it is the
torch fp32 result the bars are measured from), plain-torch LSTM and joint references, the transformers ParakeetForTDT pair on
parakeet_refs.TOY, and the test-side oracle of parakeet_tdt_lib.dynamic_eval_tdt_loss on transformers' model, `generate`, `tdt_loss` and
torch.optim.Adam."""
import random

import numpy as np
import torch

import parakeet_refs as PR

NEG = -np.inf


# ----------------------------------------------------------------------------------------------------------- TDT loss, float64
def _lse(stack):
    """log sum exp over axis 0, -inf where every entry is -inf (never nan)."""
    m = stack.max(0)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.exp(stack - ms).sum(0)), NEG)


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def tdt_row(tok, dur, target, T, U, blank, durations, sigma, dtype=np.float64):
    """One batch row.  tok [T', U' + 1, V + 1], dur [T', U' + 1, D] logits (only [:T, :U + 1] is read), target [>= U] ints.
    Arcs as transformers.loss.loss_tdt.tdt_loss: from (t, u) a blank arc of every duration d > 0 to (t + d, u) and a label arc of every
    duration d to (t + d, u + 1); the terminal sums the blank arcs with t + d == T at u == U.
    Returns dict(nll, alpha [T, U + 1], beta [T, U + 1], dtok [T', U' + 1, V + 1], ddur [T', U' + 1, D]) of the row's NLL; an unreachable
    terminal gives nll = +inf and zero gradients."""
    tok, dur = np.asarray(tok, dtype), np.asarray(dur, dtype)
    D = len(durations)
    ltok = log_softmax(tok[:T, :U + 1]) - dtype(sigma)
    ldur = log_softmax(dur[:T, :U + 1])
    lb = ltok[..., blank]
    ll_ = np.full((T, U + 1), NEG, dtype)
    if U > 0:
        ll_[:, :U] = np.take_along_axis(ltok[:, :U], np.asarray(target[:U], np.int64)[None, :, None], -1)[..., 0]
    alpha = np.full((T, U + 1), NEG, dtype)
    alpha[0, 0] = 0.0
    for n in range(1, T + U):
        us = np.arange(max(0, n - T + 1), min(n, U) + 1)
        ts = n - us
        cands = []
        for i, d in enumerate(durations):
            tp = ts - d
            ok = tp >= 0
            tc = np.clip(tp, 0, None)
            if d > 0:
                cands.append(np.where(ok, alpha[tc, us] + lb[tc, us] + ldur[tc, us, i], NEG))
            okl = ok & (us > 0)
            uc = np.clip(us - 1, 0, None)
            cands.append(np.where(okl, alpha[tc, uc] + ll_[tc, uc] + ldur[tc, uc, i], NEG))
        alpha[ts, us] = _lse(np.stack(cands))
    beta = np.full((T, U + 1), NEG, dtype)
    for n in range(T + U - 1, -1, -1):
        us = np.arange(max(0, n - T + 1), min(n, U) + 1)
        ts = n - us
        cands = []
        for i, d in enumerate(durations):
            tn = ts + d
            inside = tn < T
            tc = np.clip(tn, None, T - 1)
            if d > 0:
                term = (tn == T) & (us == U)
                cands.append(np.where(term, lb[ts, us] + ldur[ts, us, i], np.where(inside, lb[ts, us] + ldur[ts, us, i] + beta[tc, us], NEG)))
            okl = inside & (us < U)
            uc = np.clip(us + 1, None, U)
            cands.append(np.where(okl, ll_[ts, us] + ldur[ts, us, i] + beta[tc, uc], NEG))
        beta[ts, us] = _lse(np.stack(cands))
    ll = beta[0, 0]
    dtok, ddur = np.zeros(tok.shape, dtype), np.zeros(dur.shape, dtype)
    if not np.isfinite(ll):
        return dict(nll=np.inf, alpha=alpha, beta=beta, dtok=dtok, ddur=ddur)
    tt, uu = np.meshgrid(np.arange(T), np.arange(U + 1), indexing="ij")
    gb, gl = np.zeros((D, T, U + 1), dtype), np.zeros((D, T, U + 1), dtype)
    with np.errstate(invalid="ignore"):
        for i, d in enumerate(durations):
            tn = tt + d
            inside = tn < T
            tc = np.clip(tn, None, T - 1)
            if d > 0:
                nxt = np.where((tn == T) & (uu == U), 0.0, np.where(inside, beta[tc, uu], NEG))
                e = alpha + lb + ldur[..., i] + nxt - ll
                gb[i] = np.where(np.isfinite(e), np.exp(e), 0.0)
            nxt = np.where(inside & (uu < U), beta[tc, np.clip(uu + 1, None, U)], NEG)
            e = alpha + ll_ + ldur[..., i] + nxt - ll
            gl[i] = np.where(np.isfinite(e), np.exp(e), 0.0)
    Gb, Gl = gb.sum(0), gl.sum(0)
    g = np.exp(ltok + dtype(sigma)) * (Gb + Gl)[..., None]
    g[..., blank] -= Gb
    if U > 0:
        idx = np.asarray(target[:U], np.int64)[None, :, None]
        np.put_along_axis(g[:, :U], idx, np.take_along_axis(g[:, :U], idx, -1) - Gl[:, :U, None], -1)
    dtok[:T, :U + 1] = g
    ddur[:T, :U + 1] = np.exp(ldur) * (Gb + Gl)[..., None] - np.moveaxis(gb + gl, 0, -1)
    return dict(nll=-ll, alpha=alpha, beta=beta, dtok=dtok, ddur=ddur)


def reduction_weights(reduction, U):
    """d loss / d nll_b of tdt_loss's five reductions ("none": the gradient of the sum of the rows)."""
    U = np.asarray(U, np.float64)
    B = len(U)
    with np.errstate(divide="ignore"):
        return {"sum": np.ones(B), "none": np.ones(B), "mean_batch": np.full(B, 1.0 / B), "mean": 1.0 / (U * B),
                "mean_volume": np.full(B, 1.0 / U.sum())}[reduction]


def tdt_ref(logits, targets, T_b, U_b, blank, durations, sigma=0.0, reduction="sum", grad_scale=1.0, dtype=np.float64):
    """logits [B, T', U' + 1, V + 1 + D] (torch or numpy).  Returns dict(nll [B], loss, grad [B, T', U' + 1, V + 1 + D] of
    grad_scale * loss, rows as lists of tdt_row's results) as numpy arrays of `dtype`."""
    x = np.asarray(logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else logits, dtype)
    tg = np.asarray(targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else targets, np.int64).reshape(x.shape[0], -1)
    V1 = x.shape[-1] - len(durations)
    rows = [tdt_row(x[b, ..., :V1], x[b, ..., V1:], tg[b], int(T_b[b]), int(U_b[b]), blank, list(durations), sigma, dtype) for b in range(x.shape[0])]
    nll = np.array([r["nll"] for r in rows], np.float64)
    w = reduction_weights(reduction, [int(u) for u in U_b])
    with np.errstate(invalid="ignore"):
        loss = nll if reduction == "none" else (nll * w).sum()
    grad = np.stack([np.concatenate([r["dtok"], r["ddur"]], -1) * (w[b] * grad_scale) for b, r in enumerate(rows)])
    return dict(nll=nll, loss=loss, grad=grad, rows=rows)


def tdt_torch_fp32(logits, targets, T_b, U_b, blank, durations, sigma=0.0, reduction="sum"):
    """transformers' tdt_loss with autograd on the CPU: (loss or per-row losses, gradient of its sum w.r.t. the logits) in fp32."""
    from transformers.loss.loss_tdt import tdt_loss
    x = logits.detach().cpu().float().clone().requires_grad_()
    V1 = x.shape[-1] - len(durations)
    tg = torch.as_tensor(np.asarray(targets), dtype=torch.int64).reshape(x.shape[0], -1)
    if tg.shape[1] < x.shape[2] - 1:
        tg = torch.cat([tg, torch.zeros(x.shape[0], x.shape[2] - 1 - tg.shape[1], dtype=torch.int64)], 1)
    loss = tdt_loss(x[..., :V1], x[..., V1:], tg[:, :x.shape[2] - 1], torch.as_tensor(list(T_b)), torch.as_tensor(list(U_b)), blank, list(durations),
                    sigma, reduction)
    if torch.isfinite(loss).all():
        loss.sum().backward()
        grad = x.grad
    else:
        grad = torch.zeros_like(x)
    return loss.detach(), grad


def tdt_inputs(B, T, U, V1, D, seed, scale=1.0):
    """Seeded logits [B, T, U + 1, V1 + D] and targets [B, max(U, 1)] in [0, V1 - 1) (blank = V1 - 1)."""
    g = torch.Generator().manual_seed(52000 + seed + 13 * T + 7 * U + V1)
    x = torch.randn(B, T, U + 1, V1 + D, generator=g) * scale
    tg = torch.randint(0, V1 - 1, (B, max(U, 1)), generator=g, dtype=torch.int32)
    return x.contiguous(), tg


# ----------------------------------------------------------------------------------------------------------- LSTM, joint
def lstm_ref(x, weights, dy=None, dtype=torch.float64):
    """torch.nn.LSTM(batch_first) from a zero state with the given [(w_ih, w_hh, b_ih, b_hh)] per layer; x [B, S, Hd].
    Returns (y, [grads per layer] or None, dx or None) in `dtype`."""
    Hd, L = x.shape[-1], len(weights)
    m = torch.nn.LSTM(Hd, Hd, L, batch_first=True).to(dtype)
    with torch.no_grad():
        for k, ws in enumerate(weights):
            for n, w in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ws):
                getattr(m, f"{n}_l{k}").copy_(w.to(dtype))
    xr = x.detach().to(dtype).clone().requires_grad_(dy is not None)
    y, _ = m(xr)
    if dy is None:
        return y.detach(), None, None
    y.backward(dy.to(dtype))
    grads = [tuple(getattr(m, f"{n}_l{k}").grad for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for k in range(L)]
    return y.detach(), grads, xr.grad


def joint_ref(e, p, dz=None):
    """z = relu(e[:, :, None] + p[:, None]) in the operands' dtype; p [B or 1, U1, Hd].  With dz: (z, de, dp)."""
    er, pr = e.detach().clone().requires_grad_(dz is not None), p.detach().clone().requires_grad_(dz is not None)
    z = torch.relu(er[:, :, None, :] + pr[:, None, :, :])
    if dz is None:
        return z.detach()
    z.backward(dz)
    return z.detach(), er.grad, pr.grad


# ----------------------------------------------------------------------------------------------------------- the transformers pair
TDT_VOCAB, TDT_BLANK, TDT_PAD = 33, 32, 2
DURATIONS = (0, 1, 2, 3, 4)


def hf_tdt_config(arch=PR.TOY, vocab=TDT_VOCAB, hidden=64, layers=2, durations=DURATIONS, **over):
    from transformers import ParakeetTDTConfig
    return ParakeetTDTConfig(vocab_size=vocab, decoder_hidden_size=hidden, num_decoder_layers=layers, durations=list(durations),
                             blank_token_id=vocab - 1, pad_token_id=TDT_PAD, encoder_config=dict(arch), **over)


def hf_tdt_model(seed=0, blank_bias=0.0, head_gain=1.0, token_shift=0.0, sub_gain=1.0, emb_gain=1.0, dec_gain=1.0, dur_gain=1.0, **kw):
    """transformers' ParakeetForTDT in eval mode, one-dimensional parameters and the batch norms' running statistics randomised as
    parakeet_refs.hf_model does.  `blank_bias` is added to the blank's joint-head bias and `head_gain` multiplies the joint head's
    weight (the decode tests: margins between the best and the second-best class), `token_shift` is added to every token class's bias:
    it changes no token argmax and no log-probability, and keeps the largest duration logit below the largest token logit, where
    transformers' generate, which takes its `sequences` from the argmax over the WHOLE joint row, would otherwise emit a duration's
    column as a token.  `sub_gain` multiplies the subsampling's weights, `emb_gain` the prediction network's embedding, `dec_gain` its
    projector's weight and `dur_gain` the duration rows of the joint head on top of head_gain: with
    transformers' initialisation (std 0.02) the biases drown the input, every encoder frame and every decoder state is nearly the same
    vector and a greedy decode repeats one step; with the gains the frames and states differ."""
    from transformers import ParakeetForTDT
    torch.manual_seed(seed)
    cfg = hf_tdt_config(**kw)
    ref = ParakeetForTDT(cfg).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
        for n, p in ref.named_parameters():
            if n.startswith("encoder.subsampling.") and n.endswith("weight"):
                p.mul_(sub_gain)
        ref.decoder.embedding.weight.mul_(emb_gain)
        ref.decoder.decoder_projector.weight.mul_(dec_gain)
        ref.joint.head.weight[cfg.vocab_size:].mul_(dur_gain)
        ref.joint.head.weight.mul_(head_gain)
        ref.joint.head.bias[cfg.blank_token_id] += blank_bias
        ref.joint.head.bias[:cfg.vocab_size] += token_shift
    ref.generation_config.decoder_start_token_id = cfg.blank_token_id        # unset in the config: generate() starts from the blank, as NeMo does
    return cfg, ref


def start_token(ref):
    s = ref.generation_config.decoder_start_token_id
    return ref.config.blank_token_id if s is None else int(s)


def hf_greedy(ref, feats):
    """transformers' generate on [B, T, F] features -> per row (non-blank tokens, their encoder frames), the steps taken before the row's
    frame pointer reached the end, and the smallest top-2 margins (token, duration) over those steps' argmaxes, recomputed step by step."""
    cfg = ref.config
    with torch.no_grad():
        out = ref.generate(input_features=feats)
    seq, dur = out.sequences[:, 1:], out.durations[:, 1:]
    Tp = int(ref.encoder._get_subsampling_output_length(torch.tensor([feats.shape[1]])).item())
    rows = []
    for b in range(feats.shape[0]):
        toks, frames, steps, t = [], [], [], 0
        for s in range(seq.shape[1]):
            if t >= Tp:
                break
            k, d = int(seq[b, s]), int(dur[b, s])
            steps.append((k, d, t))
            if k != cfg.blank_token_id:
                toks.append(k)
                frames.append(t)
            t += d
        rows.append(dict(tokens=toks, frames=frames, steps=steps))
    return rows, Tp


def hf_margins(ref, feats, rows):
    """The smallest top-2 margins (token logits, duration logits) over the steps hf_greedy reports, from a step-by-step replay of the
    prediction network and the joint in fp32 on the CPU; asserts that the replay takes the same steps."""
    cfg = ref.config
    V1 = cfg.vocab_size
    start = start_token(ref)
    mt, md = np.inf, np.inf
    with torch.no_grad():
        enc = ref.get_audio_features(input_features=feats).pooler_output
        for b, row in enumerate(rows):
            emb = ref.decoder.embedding(torch.tensor([[start]]))
            o, st = ref.decoder.lstm(emb)
            dec = ref.decoder.decoder_projector(o)[0, 0]
            for k, d, t in row["steps"]:
                lg = ref.joint.head(torch.relu(enc[b, t] + dec))
                tk, du = lg[:V1], lg[V1:]
                assert int(tk.argmax()) == k, (b, t, int(tk.argmax()), k)
                dd = int(du.argmax())
                assert (1 if (k == cfg.blank_token_id and dd == 0) else dd) == d, (b, t, dd, d)
                mt = min(mt, float(tk.topk(2).values.diff().abs()))
                md = min(md, float(du.topk(2).values.diff().abs()))
                if k != cfg.blank_token_id:
                    o, st = ref.decoder.lstm(ref.decoder.embedding(torch.tensor([[k]])), st)
                    dec = ref.decoder.decoder_projector(o)[0, 0]
    return mt, md


# ----------------------------------------------------------------------------------------------------------- the loop's oracle
def merged_ref(windows, starts, seq_lens, factor):
    """Independent restatement of the merge rule: windows = per-window [(token, absolute encoder frame)], starts / seq_lens in input frames,
    in any order.  A token at frame f is kept by the window whose ownership interval contains f * factor; the cut between consecutive
    windows is the midpoint of their overlap."""
    order = sorted(range(len(starts)), key=lambda i: starts[i])
    out = []
    for rank, i in enumerate(order):
        lo = -np.inf if rank == 0 else (starts[i] + starts[order[rank - 1]] + seq_lens[order[rank - 1]]) / 2.0
        hi = np.inf if rank == len(order) - 1 else (starts[order[rank + 1]] + starts[i] + seq_lens[i]) / 2.0
        out += [(k, f) for k, f in windows[i] if lo <= f * factor < hi]
    return [k for k, _ in out], [f for _, f in out]


def dynamic_eval_tdt_ref(args, model, spec, seq_len, overlap, tokenizer, num_negatives, lr_args, spec_augment_config=PR.SPEC_AUGMENT,
                         generator=None, batch_renorm=False, logits_out=None):
    """parakeet_tdt_lib.dynamic_eval_tdt_loss restated on transformers' ParakeetForTDT (CPU): per window SpecAugment on the first
    num_negatives copies, one grad-mode encoder pass of all copies, `generate`-style greedy decode of the clean copy from the same encoder
    states, the text hop, tdt_loss (reduction "sum") of the augmented copies on the decoded ids scaled by 1 / (T' * num_negatives), Adam on
    everything but encoder.subsampling and decoder.  `batch_renorm`: the conv modules' norm is batch_renorm_refs.swap_in's training-mode
    BatchRenorm1d (the model is changed for good: pass a copy).  Returns (ids, frames); `logits_out` collects the joint logits of a fixed probe after
    the last step."""
    from dynamic_asr_eval_amd.augment import SpecAugment
    from oracle.dynamic_eval_ref import apply_masks
    from transformers.loss.loss_tdt import tdt_loss
    cfg = model.config
    V1, blank = cfg.vocab_size, cfg.blank_token_id
    start = start_token(model)
    spec_n = spec.shape[-1]
    factor = 8
    original = [p.clone().detach() for p in model.parameters()]
    augmentation = SpecAugment(**spec_augment_config)
    model.eval()
    if batch_renorm:                         # reference nvidia_ctc/lib.py:74,89-102 on this model: `model` is then the caller's own copy
        import batch_renorm_refs as BR
        BR.swap_in(model)
    frozen = []
    for part in (model.encoder.subsampling, model.decoder):
        for p in part.parameters():
            frozen.append((p, p.requires_grad))
            p.requires_grad = False
    optimizer = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], **lr_args)
    if seq_len > spec_n:
        seq_len, overlap = spec_n, 0
    assert overlap % factor == 0
    last_ulen, kill_next = None, False
    training_data = {}
    for i in range(0, spec_n, seq_len - overlap):
        chunk = spec[:, :, i:i + seq_len]
        u_len = chunk.shape[-1]
        if kill_next:
            break
        elif last_ulen is not None and u_len < last_ulen:
            kill_next = True
        last_ulen = u_len
        training_data[i] = chunk
    windows = {}
    for epoch in range(args.__dict__.get('epochs', 1)):
        windows = {}
        keys = list(training_data.keys())
        keys = random.sample(keys, len(keys)) if args.__dict__.get('shuffle', False) else keys
        for i in keys:
            chunk = training_data[i].clone().repeat(num_negatives + 1, 1, 1)
            for j in range(num_negatives):
                apply_masks(chunk[j], augmentation.draw(chunk.shape[1], chunk.shape[2], generator), augmentation.zero_masking)
            enc = model.get_audio_features(input_features=chunk.transpose(1, 2)).pooler_output          # [n + 1, T', Hd]
            Tp = enc.shape[1]
            with torch.no_grad():                                                                        # greedy decode of the clean copy
                toks, frs, t, steps = [], [], 0, 0
                o, st = model.decoder.lstm(model.decoder.embedding(torch.tensor([[start]])))
                dec = model.decoder.decoder_projector(o)[0, 0]
                while t < Tp and steps < cfg.max_symbols_per_step * Tp:
                    lg = model.joint.head(torch.relu(enc[-1, t] + dec))
                    k, d = int(lg[:V1].argmax()), int(lg[V1:].argmax())
                    if logits_out is not None:
                        logits_out["margin"] = min(logits_out.get("margin", np.inf), float(lg[:V1].topk(2).values.diff().abs()),
                                                   float(lg[V1:].topk(2).values.diff().abs()))
                        logits_out.setdefault("steps", []).append((k, cfg.durations[d]))
                    d = cfg.durations[d]
                    if k == blank and d == 0:
                        d = 1
                    if k != blank:
                        toks.append(k)
                        frs.append(t)
                        o, st = model.decoder.lstm(model.decoder.embedding(torch.tensor([[k]])), st)
                        dec = model.decoder.decoder_projector(o)[0, 0]
                    t += d
                    steps += 1
            windows[i] = [(k, f + i // factor) for k, f in zip(toks, frs)]
            ids = tokenizer.text_to_ids(tokenizer.ids_to_text(toks))
            dec_in = torch.tensor([[start] + ids])
            p = model.decoder(dec_in)                                                                    # [1, U + 1, Hd]
            logits = model.joint(encoder_hidden_states=enc[:num_negatives, :, None, :], decoder_hidden_states=p[:, None, :, :])
            n = num_negatives
            loss = tdt_loss(logits[..., :V1], logits[..., V1:], torch.tensor([ids] * n, dtype=torch.int64).reshape(n, len(ids)),
                            torch.tensor([Tp] * n), torch.tensor([len(ids)] * n), blank, list(cfg.durations), 0.0, "sum") / (Tp * n)
            optimizer.zero_grad()
            if torch.isfinite(loss):
                loss.backward()
                optimizer.step()
    if logits_out is not None:
        with torch.no_grad():
            feats, dec_in = logits_out["probe"]
            e = model.get_audio_features(input_features=feats).pooler_output
            logits_out["logits"] = model.joint(encoder_hidden_states=e[:, :, None, :], decoder_hidden_states=model.decoder(dec_in)[:, None, :, :])
    keys = sorted(windows)
    ids, frames = merged_ref([windows[i] for i in keys], keys, [training_data[i].shape[-1] for i in keys], factor)
    with torch.no_grad():
        for p, p_orig in zip(model.parameters(), original):
            p.copy_(p_orig)
    for p, rg in frozen:
        p.requires_grad = rg
    model.zero_grad()
    return ids, frames


# ----------------------------------------------------------------------------------------------------------- the decode and loop cases
# Found by a seeded search on the CPU so that transformers' decode ALONE satisfies assert_decode_conditions (tests/test_parakeet_tdt_cpu.py).
DECODE = dict(seed=11, blank_bias=4.0, head_gain=50.0, token_shift=600.0, sub_gain=12.0, emb_gain=30.0, dec_gain=30.0)
DECODE_FEATS = dict(seed=1, T=300)
LOOP = dict(seq_len=128, num_negatives=2, lr_args={'lr': 1e-5}, T=300, spec_seed=8, mask_seed=5)


def decode_model():
    return hf_tdt_model(**DECODE)


def decode_feats(B):
    return torch.randn(3, DECODE_FEATS["T"], PR.TOY["num_mel_bins"], generator=torch.Generator().manual_seed(DECODE_FEATS["seed"]))[:B].contiguous()


def decode_case(B, ref=None):
    """(rows of hf_greedy, T', (smallest token margin, smallest duration margin)) of the decode tests' model on their first B feature rows."""
    ref = decode_model()[1] if ref is None else ref
    x = decode_feats(B)
    rows, Tp = hf_greedy(ref, x)
    return rows, Tp, hf_margins(ref, x, rows)


def assert_decode_conditions(rows, mt, md, blank=TDT_BLANK):
    steps = [s for r in rows for s in r["steps"]]
    nonblank = [s for s in steps if s[0] != blank]
    assert min(mt, md) >= 1e-2, (mt, md)                                         # the existing rule of the LASR loop test
    assert 4 * len(nonblank) >= len(steps) and len(nonblank) < len(steps), (len(nonblank), len(steps))
    assert len({d for _, d, _ in steps}) >= 3, sorted({d for _, d, _ in steps})
    assert any(d == 0 for _, d, _ in nonblank)


def loop_inputs():
    spec = torch.randn(1, PR.TOY["num_mel_bins"], LOOP["T"], generator=torch.Generator().manual_seed(LOOP["spec_seed"]))
    return spec, PR.Tokenizer(TDT_VOCAB - 1)
