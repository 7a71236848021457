"""Timings of LASR (MedASR) on the MI355X, one JSON line:
  convmod  the conv-module core between the two pointwise convolutions, forward + backward (dyn_convmod_bn_fwd + dyn_convmod_bn_bwd_act +
           dyn_dwconv1d_wgrad + dyn_glu_dwconv1d_dgrad), at 32 taps and [B, T, C] = [5, 509, 512] (the loop's window: 2048 feature frames, 4
           augmented copies + 1 clean, MedASR's width) and [5, 2048, 512], next to the YARDSTICK, the 9-tap core (Parakeet's, unchanged code)
           at the same [B, T, C]: the same HBM traffic, 3.6 x fewer multiply-adds.  One process, alternating, HIP events, median (min - max) of
           25 after a warm-up of 5, eager launches.  The 9-tap core is timed TWICE in the same alternation: the difference of its medians is
           the run-to-run spread the ratio is held against.  Each kernel is also timed alone, with the bytes it has to move over its time.
           A library built with the tiling experiment's switch (dyn_convmod_bn_debug_form: 0 = register window, 1 = LDS column) has both
           forms timed in the same alternation and checked against each other; the committed library holds one form and no switch.
  loop     nvidia_ctc_lib.dynamic_eval (seq_len 2048, 4 augmented copies + 1 clean, Adam) over a synthetic 10-minute feature matrix
           [1, 128, 60000] with seeded weights at MedASR's shape (17 layers, 512 wide, 8 heads, FFN 2048, 128 mel bins, vocabulary 512): three
           passes after a warm-up pass over both window shapes, audio-s/s from a host clock around a pass that ends in a device synchronise.
Usage: python scripts/time_lasr.py [convmod] [loop] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_data2vec_audio import _median_us  # noqa: E402

EPS = 1e-5


def _stat(t):
    return {"us": round(t[0], 1), "min_max": [round(t[1], 1), round(t[2], 1)]}


def time_convmod(dev, B, T, C, reps=25):
    from dynamic_asr_eval_amd import ops
    lib = ops._L()
    switch = getattr(lib, "dyn_convmod_bn_debug_form", None)
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                                          # noqa: E731
    u, mean, var, gamma, beta = r(B, T, 2 * C), r(C) * 0.1, (0.5 + torch.rand(C, generator=g)).to(dev), 1 + 0.1 * r(C), r(C) * 0.1
    ds = r(B, T, C) / T
    w = {9: r(C, 9) * 0.3, 32: r(C, 32) * 0.15}
    grads = {k: dict(w=torch.zeros(C, k, device=dev), gamma=torch.zeros(C, device=dev), beta=torch.zeros(C, device=dev)) for k in w}

    def core(kw, form=None):
        def run():
            if form is not None:
                switch(form)
            s, gl, c = ops.convmod_bn(u, w[kw], None, mean, var, gamma, beta, "silu", EPS, save=True)
            dc = ops.convmod_bn_bwd_act(c, mean, var, gamma, beta, ds, grads[kw]["gamma"], grads[kw]["beta"], None, "silu", EPS, wgrad_beta=0.0)
            ops.dwconv1d_wgrad(gl, dc, grads[kw]["w"], None, beta=0.0)
            return s, ops.glu_dwconv1d_dgrad(u, w[kw], dc)
        return run

    forms = {"register_window": 0, "lds_column": 1} if switch is not None else {"kept": None}
    out = {"shape": [B, T, C], "tile_frames_32": ops.convmod_bn_time_tile(32)}
    if switch is not None:
        a, b = core(32, 0)(), core(32, 1)()
        out["forms_bit_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        assert (a[0] - b[0]).abs().max().item() < 1e-5 and (a[1] - b[1]).abs().max().item() < 1e-5
    fns = [core(9), core(9)] + [core(32, f) for f in forms.values()]
    t = _median_us(fns, reps=reps, warm=5)
    nine = max(t[0][0], t[1][0])
    out["taps9_us"], out["taps9_again_us"] = _stat(t[0]), _stat(t[1])
    out["taps9_spread_us"] = round(abs(t[0][0] - t[1][0]), 1)
    for (name, _), tt in zip(forms.items(), t[2:]):
        out[f"taps32_{name}"] = dict(_stat(tt), ratio_to_slower_taps9=round(tt[0] / nine, 3))
    # each kernel alone: bytes it has to move (every operand once) over its time
    for name, f in forms.items():
        if f is not None:
            switch(f)
        s, gl, c = ops.convmod_bn(u, w[32], None, mean, var, gamma, beta, "silu", EPS, save=True)
        dc = ops.convmod_bn_bwd_act(c, mean, var, gamma, beta, ds, None, None, None, "silu", EPS)
        gw = grads[32]
        ks = {"fwd": (lambda: ops.convmod_bn(u, w[32], None, mean, var, gamma, beta, "silu", EPS, save=True), 5 * B * T * C * 4),
              "bwd_act": (lambda: ops.convmod_bn_bwd_act(c, mean, var, gamma, beta, ds, gw["gamma"], gw["beta"], None, "silu", EPS, wgrad_beta=0.0),
                          3 * B * T * C * 4),
              "wgrad": (lambda: ops.dwconv1d_wgrad(gl, dc, gw["w"], None, beta=0.0), 2 * B * T * C * 4),
              "dgrad": (lambda: ops.glu_dwconv1d_dgrad(u, w[32], dc), 5 * B * T * C * 4)}
        tk = _median_us([k[0] for k in ks.values()], reps=reps, warm=5)
        out[f"kernels_{name}"] = {n: dict(_stat(tt), bytes=by, GB_per_s=round(by / tt[0] / 1e3, 1)) for (n, (_, by)), tt in zip(ks.items(), tk)}
    if switch is not None:
        switch(0)
    return out


def time_loop(dev, seconds, passes=3):
    import argparse as ap
    from dynamic_asr_eval_amd import nvidia_ctc_lib as N
    from dynamic_asr_eval_amd.lasr_model import LasrForCTC
    from dynamic_asr_eval_amd.run_wav2vec2 import init_synthetic
    model = LasrForCTC(None, device=dev)                                                         # the defaults are MedASR's shape
    init_synthetic(model, seed=0)
    for n, b in model.buffers_.items():
        if n.endswith("running_var"):
            b.fill_(1.0)
    frames = int(seconds * 100)                                                                  # 10 ms hop
    spec = torch.randn(1, model.n_mels, frames, generator=torch.Generator().manual_seed(7))
    tok = N.SyntheticTokenizer(model.cfg["vocab_size"] - 1)
    args = ap.Namespace(epochs=1, shuffle=False, spec_augment_generator=torch.Generator().manual_seed(1))

    def run(sp):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = N.dynamic_eval(args, model, sp, 2048, 0, tok, use_tqdm=False, return_device=True)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    tail = frames % 2048
    run(spec[:, :, :2048 + tail] if tail else spec[:, :, :4096])                                 # warm-up: every window shape of the timed passes
    times = []
    for _ in range(passes):
        t, out = run(spec)
        assert torch.isfinite(out).all()
        times.append(t)
    c = model.cfg
    n_params = sum(p.numel() for _, p in model.named_parameters())
    return {"shape": {"layers": c["num_hidden_layers"], "hidden": c["hidden_size"], "heads": c["num_attention_heads"], "ffn": c["intermediate_size"],
                      "mel_bins": c["num_mel_bins"], "vocab": c["vocab_size"], "parameters_M": round(n_params / 1e6, 1)},
            "audio_seconds": seconds, "windows": -(-frames // 2048), "copies": 5, "encoder_frames_per_window": 509,
            "pass_s": [round(t, 3) for t in times], "audio_s_per_s": round(seconds / sorted(times)[len(times) // 2], 1)}


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["convmod", "loop"])
    p.add_argument("--seconds", type=float, default=600.0)
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lasr.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {}
    if "convmod" in a.what:
        res["convmod_core_fwd_bwd"] = [time_convmod(dev, 5, 509, 512), time_convmod(dev, 5, 2048, 512)]
    if "loop" in a.what:
        res["dynamic_eval"] = time_loop(dev, a.seconds)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
