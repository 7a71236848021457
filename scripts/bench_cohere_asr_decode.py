"""ms per token of the greedy decode of CohereAsrForConditionalGeneration at the released DECODER size (8 layers x 1024, d_ff 4096, vocab
16384) over a 2-layer encoder and 375 encoder frames, random weights, 64 tokens of forced length, R = 1, 4 and 8 rows:
  steps     dyn_seq2seq_steps alone (4 calls of 16 steps, the chunks generate() queues), device-synchronised host clock
  generate  this package's generate() end to end (encoder, decoder.proj, cross K | V, steps, the host reads)
  baseline  transformers' CohereAsrForConditionalGeneration with the same state dict on the same GPU in fp32,
            generate(do_sample=False, min_new_tokens = max_new_tokens = 64), end to end
Median over `--repeats` runs after `--warmup` runs, the three alternating within a repeat.  Bytes per token are the parameters one step
reads, counted from their shapes; bytes / steps time stands next to the 6.0 - 6.3 TB/s swept-read figure of the MI355X.  Run once on the
GPU under its own `timeout`; not part of bench.py.  Prints one JSON line and, with --out, writes it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DECODER = dict(vocab_size=16384, hidden_size=1024, num_hidden_layers=8, num_attention_heads=8, intermediate_size=4096, max_position_embeddings=1024)
ENCODER = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, subsampling_conv_channels=256, num_mel_bins=80)
N_ENC, TOKENS, CHUNK = 375, 64, 16


def step_bytes(model):
    """Bytes of parameters one step of one position reads: every decoder layer without the cross k | v projections (they run once per
    call), the final norm and the head; of the two embedding tables only a row per sequence."""
    from dynamic_asr_eval_amd.cohere_asr_model import DEC, HEAD
    skip = ("encoder_attn.k_proj", "encoder_attn.v_proj")
    n = sum(model.P[name].numel() for name, _ in model.spec
            if (name.startswith(DEC + "layers.") and not any(s in name for s in skip)) or name.startswith((DEC + "norm.", HEAD)))
    return 4 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--out", default="")
    ap.add_argument("--steps-only", action="store_true", help="time dyn_seq2seq_steps alone (a kernel trace of the step)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cohere_asr_decode: needs the GPU (no CPU timing is a timing)")
    from transformers import CohereAsrConfig
    from transformers import CohereAsrForConditionalGeneration as HF
    from dynamic_asr_eval_amd._lib import check, load
    from dynamic_asr_eval_amd.cohere_asr_model import DEC, HEAD, CohereAsrForConditionalGeneration
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = CohereAsrConfig(encoder_config=dict(ENCODER), decoder_start_token_id=4, **DECODER)
    ref = HF(cfg).eval()
    with torch.no_grad():
        for w in (ref.model.decoder.embed_tokens.weight, ref.model.decoder.pos_emb.weight, ref.proj_out.weight):
            w.mul_(8.0)
    model = CohereAsrForConditionalGeneration(cfg, device=dev)
    model.load_state_dict(ref.state_dict())
    ref = ref.to(dev)
    model.P[HEAD + "bias"][model.eos] = -1e30                     # our side: an eos that cannot win (the baseline gets min_new_tokens)
    d, L = model.d, model.L
    T = N_ENC * 8
    assert model.frames(T) == N_ENC
    sync = torch.cuda.synchronize
    st = torch.cuda.current_stream().cuda_stream
    result = dict(decoder=DECODER, encoder=ENCODER, encoder_frames=N_ENC, tokens=TOKENS, chunk=CHUNK, repeats=args.repeats, warmup=args.warmup,
                  bytes_per_token=step_bytes(model), device=torch.cuda.get_device_name(0), rows={})
    for R in args.rows:
        x = torch.randn(R, T, ENCODER["num_mel_bins"], device=dev, generator=torch.Generator(device=dev).manual_seed(R))
        prompt = torch.full((R, 1), model.start_token, dtype=torch.int64)
        with torch.no_grad():
            enc = model.encode(x)
            mem = torch.nn.functional.linear(enc, model.P[DEC + "proj.weight"], model.P[DEC + "proj.bias"])
            kv = [torch.nn.functional.linear(mem, model._ckv[l][0][0], model._ckv[l][1][0]).contiguous() for l in range(L)]
        cap = TOKENS
        cache = [torch.empty(R, cap, 3 * d, device=dev) for _ in range(L)]
        tokens = torch.zeros(R, cap + 1, dtype=torch.int32, device=dev)
        finished = torch.zeros(R, dtype=torch.int32, device=dev)
        logits = torch.empty(R, model.V, device=dev)
        scratch = torch.empty(R, int(load().dyn_seq2seq_row_scratch_floats(d, model.I, model.nh)), device=dev)
        desc, keep = model._step_desc(kv, cache, tokens, finished, logits, scratch, R, N_ENC, cap)

        def steps():
            tokens.zero_()
            tokens[:, 0] = model.start_token
            finished.zero_()
            sync()
            t0 = time.perf_counter()
            for t in range(0, cap, CHUNK):
                check(load().dyn_seq2seq_steps(ctypes.byref(desc), t, CHUNK, 1, st), "dyn_seq2seq_steps")
            sync()
            return (time.perf_counter() - t0) * 1e3 / TOKENS

        def generate():
            sync()
            t0 = time.perf_counter()
            out = model.generate(x, decoder_input_ids=prompt, max_new_tokens=TOKENS)
            sync()
            assert out.shape == (R, TOKENS + 1), out.shape
            return (time.perf_counter() - t0) * 1e3 / TOKENS, out

        def baseline():
            sync()
            t0 = time.perf_counter()
            with torch.no_grad():
                out = ref.generate(input_features=x, decoder_input_ids=prompt.to(dev), do_sample=False, max_new_tokens=TOKENS, min_new_tokens=TOKENS)
            sync()
            assert out.shape == (R, TOKENS + 1), out.shape
            return (time.perf_counter() - t0) * 1e3 / TOKENS, out

        times = {"steps": [], "generate": [], "baseline": []}
        agree = None
        for i in range(args.warmup + args.repeats):
            if args.steps_only:
                a = steps()
                if i >= args.warmup:
                    times["steps"].append(a)
                continue
            a, (b, ours), (c, theirs) = steps(), generate(), baseline()
            if i >= args.warmup:
                times["steps"].append(a); times["generate"].append(b); times["baseline"].append(c)
            agree = float((ours == theirs.cpu()).float().mean())        # random weights: near ties may differ; reported, not asserted
        if args.steps_only:
            result["rows"][str(R)] = dict(ms_per_token=dict(steps=round(statistics.median(times["steps"]), 4)))
            continue
        med = {k: statistics.median(v) for k, v in times.items()}
        result["rows"][str(R)] = dict(ms_per_token={k: round(v, 4) for k, v in med.items()},
                                      spread_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                                      steps_TB_per_s=round(result["bytes_per_token"] / (med["steps"] * 1e-3) / 1e12, 3),
                                      speedup_generate_vs_baseline=round(med["baseline"] / med["generate"], 2), token_agreement=round(agree, 4))
        del keep
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
