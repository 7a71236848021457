"""Timings of the training-mode BatchRenorm conv module on the MI355X: a record, no bar.
  convmod  the conv-module core between the two pointwise convolutions, forward + backward, at [B, T, C] = [5, 256, 1024] and
           [5, 2048, 1024]: TRAIN = dyn_convmod_brn_fwd + dyn_convmod_brn_bwd + dyn_dwconv1d_wgrad + dyn_glu_dwconv1d_dgrad (8 launches) next to
           EVAL = dyn_convmod_bn_fwd + dyn_convmod_bn_bwd_act + dyn_dwconv1d_wgrad + dyn_glu_dwconv1d_dgrad, the fused eval-mode core of
           scripts/time_parakeet.py.  One process, the forms alternating, HIP events, median (min - max) of 25 after 5, eager launches.
  loop     nvidia_ctc_lib.dynamic_eval (seq_len 2048, 4 augmented copies + 1 clean, Adam) over the synthetic 10-minute spectrogram of
           scripts/time_parakeet.py at the 0.6b shape, batch_renorm False and True alternating: three passes each after a warm-up pass per
           mode over both window shapes, audio-s/s from a host clock around a pass that ends in a device synchronise.
Without a step name every step runs in a child process of its own under its own time limit, and the first failure ends the run.
Usage: python scripts/time_batch_renorm.py [convmod | loop] [--seconds S] [--out profiles/batch_renorm_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

EPS, KW = 1e-5, 9
STEP_LIMIT_S = {"convmod": 120, "loop": 300}


def time_convmod(dev, B, T, C, reps=25):
    from dynamic_asr_eval_amd import ops
    from time_data2vec_audio import _Counted, _median_us
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                                          # noqa: E731
    u, w, cb, mean, var, gamma, beta = r(B, T, 2 * C), r(C, KW) * 0.3, r(C) * 0.2, r(C) * 0.1, (0.5 + torch.rand(C, generator=g)).to(dev), 1 + 0.1 * r(C), r(C) * 0.1
    rmean, rstd = mean.clone(), var.sqrt()
    ds = r(B, T, C) / T
    grads = dict(w=torch.zeros(C, KW, device=dev), cb=torch.zeros(C, device=dev), gamma=torch.zeros(C, device=dev), beta=torch.zeros(C, device=dev))
    rmax, dmax = ops.batch_renorm_clamps(1000000)

    def evalmode():
        s, gl, c = ops.convmod_bn(u, w, cb, mean, var, gamma, beta, "silu", EPS, save=True)
        dc = ops.convmod_bn_bwd_act(c, mean, var, gamma, beta, ds, grads["gamma"], grads["beta"], grads["cb"], "silu", EPS, wgrad_beta=0.0)
        ops.dwconv1d_wgrad(gl, dc, grads["w"], None, beta=0.0)
        return s, ops.glu_dwconv1d_dgrad(u, w, dc)

    def train():
        s, gl, c, stats = ops.convmod_brn(u, w, cb, rmean, rstd, gamma, beta, rmax, dmax, 0.001, "silu", EPS)
        dc = ops.convmod_brn_bwd(c, stats, ds, grads["gamma"], grads["beta"], grads["cb"], "silu", wgrad_beta=0.0)
        ops.dwconv1d_wgrad(gl, dc, grads["w"], None, beta=0.0)
        return s, ops.glu_dwconv1d_dgrad(u, w, dc)

    with _Counted() as ne:
        evalmode()
    with _Counted() as nt:
        train()
    (tt, tt_lo, tt_hi), (te, te_lo, te_hi), (td, td_lo, td_hi) = _median_us([train, evalmode, evalmode], reps=reps, warm=5)
    return {"shape": [B, T, C], "train_us": round(tt, 1), "train_us_min_max": [round(tt_lo, 1), round(tt_hi, 1)], "train_abi_calls": nt.n,
            "train_launches": 8, "eval_us": round(te, 1), "eval_us_min_max": [round(te_lo, 1), round(te_hi, 1)],
            "eval_again_us": round(td, 1), "eval_again_us_min_max": [round(td_lo, 1), round(td_hi, 1)], "eval_abi_calls": ne.n, "eval_launches": 4,
            "eval_spread_us": round(abs(te - td), 1), "time_ratio_train_over_slower_eval": round(tt / max(te, td), 3)}


def time_loop(dev, seconds, passes=3):
    import argparse as ap
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.parakeet_model import ParakeetForCTC
    from dynamic_asr_eval_amd.run_wav2vec2 import init_synthetic
    model = ParakeetForCTC(None, device=dev)                                                     # the defaults are the 0.6b shape
    init_synthetic(model, seed=0)
    for n, b in model.buffers_.items():
        if n.endswith("running_var"):
            b.fill_(1.0)
    frames = int(seconds * 100)                                                                  # 10 ms hop
    spec = torch.randn(1, model.n_mels, frames, generator=torch.Generator().manual_seed(7))
    tok = N.SyntheticTokenizer(model.cfg["vocab_size"] - 1)
    args = ap.Namespace(epochs=1, shuffle=False, spec_augment_generator=torch.Generator().manual_seed(1))

    def run(sp, mode):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = N.dynamic_eval(args, model, sp, 2048, 0, tok, use_tqdm=False, return_device=True, batch_renorm=mode)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    tail = frames % 2048
    for mode in (False, True):
        run(spec[:, :, :2048 + tail] if tail else spec[:, :, :4096], mode)                       # warm-up: every window shape of the timed passes
    times = {False: [], True: []}
    for _ in range(passes):
        for mode in (False, True):
            t, out = run(spec, mode)
            assert torch.isfinite(out).all()
            times[mode].append(t)
    med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
    return {"shape": {"layers": 24, "hidden": 1024, "heads": 8, "ffn": 4096, "vocab": model.cfg["vocab_size"]},
            "audio_seconds": seconds, "windows": -(-frames // 2048), "copies": 5, "backward_rows": {"eval": 4, "train": 5},
            "eval_pass_s": [round(t, 3) for t in times[False]], "eval_audio_s_per_s": round(seconds / med[False], 1),
            "train_pass_s": [round(t, 3) for t in times[True]], "train_audio_s_per_s": round(seconds / med[True], 1),
            "time_ratio_train_over_eval": round(med[True] / med[False], 3)}


def run_step(step, seconds):
    if not torch.cuda.is_available():
        raise SystemExit("time_batch_renorm.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    if step == "convmod":
        return {"convmod_core_fwd_bwd": [time_convmod(dev, 5, 256, 1024), time_convmod(dev, 5, 2048, 1024)]}
    return {"dynamic_eval": time_loop(dev, seconds)}


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="?", default="", choices=["", "convmod", "loop"])
    p.add_argument("--seconds", type=float, default=600.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_renorm_timing.json"))
    a = p.parse_args()
    if a.what:
        print(json.dumps(run_step(a.what, a.seconds)))
        raise SystemExit(0)
    res = {}
    for step in ("convmod", "loop"):                            # a fresh process per step, each under its own limit; a failure ends the run
        done = subprocess.run([sys.executable, os.path.abspath(__file__), step, "--seconds", str(a.seconds)], capture_output=True, text=True,
                              timeout=STEP_LIMIT_S[step])
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            raise SystemExit(f"step {step} ended with status {done.returncode}: nothing further is started")
        res.update(json.loads(done.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
