"""ms per token of CohereAsrForConditionalGeneration.generate() on a RAGGED batch at the released decoder size (bench_cohere_asr_decode.py's
models: 8 layers x 1024, d_ff 4096, vocab 16384 over a 2-layer encoder): 8 rows whose encoder lengths spread over 94 .. 375 frames, 64
tokens of forced length (an eos that cannot win), end to end (encoder, decoder.proj, cross K | V, the steps, the host reads):
  ragged  generate(x, input_lengths=...): every row's cross-attention reads its own frames (dyn_seq2seq_steps_len)
  padded  generate(x) on the same batch padded to 375 frames: the call from before per-row counts existed (what its rows compute past
          their length is wrong; it is the time that is compared)
  solo    the eight rows decoded one at a time, each at its own length: what a caller had to do for a right answer
Median of `--repeats` after `--warmup`, the modes alternating within a repeat.  `--root DIR` imports the package from another checkout
(`--modes padded` runs on one without the keyword).  Prints one JSON line and, with --out, writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TOKENS, ROWS, ENC_MIN, ENC_MAX = 64, 8, 94, 375


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", nargs="+", default=["ragged", "padded", "solo"])
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path[:0] = [args.root, HERE]
    import bench_cohere_asr_decode as BD
    from transformers import CohereAsrConfig
    from transformers import CohereAsrForConditionalGeneration as HF
    from dynamic_asr_eval_amd.cohere_asr_model import HEAD, CohereAsrForConditionalGeneration
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = CohereAsrConfig(encoder_config=dict(BD.ENCODER), decoder_start_token_id=4, **BD.DECODER)
    ref = HF(cfg).eval()
    model = CohereAsrForConditionalGeneration(cfg, device=dev)
    model.load_state_dict(ref.state_dict())
    del ref
    model.P[HEAD + "bias"][model.eos] = -1e30
    enc_lens = [ENC_MAX - (i * (ENC_MAX - ENC_MIN)) // (ROWS - 1) for i in range(ROWS)]
    lens = [8 * n for n in enc_lens]
    assert [model.frames(n) for n in lens] == enc_lens
    x = torch.randn(ROWS, lens[0], BD.ENCODER["num_mel_bins"], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rows = [x[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    prompt = torch.full((ROWS, 1), model.start_token, dtype=torch.int64)
    kw = dict(max_new_tokens=TOKENS)

    def run(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "ragged":
            out = model.generate(x, decoder_input_ids=prompt, input_lengths=lens, **kw)
        elif mode == "padded":
            out = model.generate(x, decoder_input_ids=prompt, **kw)
        else:
            out = torch.cat([model.generate(r, decoder_input_ids=prompt[:1], **kw) for r in rows])
        torch.cuda.synchronize()
        assert out.shape == (ROWS, TOKENS + 1), out.shape
        return (time.perf_counter() - t0) * 1e3 / TOKENS, out

    times, outs = {m: [] for m in args.modes}, {}
    for i in range(args.warmup + args.repeats):
        for m in args.modes:
            t, outs[m] = run(m)
            if i >= args.warmup:
                times[m].append(t)
    res = dict(decoder=BD.DECODER, encoder=BD.ENCODER, rows=ROWS, encoder_lengths=enc_lens, tokens=TOKENS, repeats=args.repeats, warmup=args.warmup,
               root=os.path.basename(os.path.abspath(args.root)), device=torch.cuda.get_device_name(0),
               ms_per_token={m: round(statistics.median(v), 4) for m, v in times.items()},
               spread_ms={m: [round(min(v), 4), round(max(v), 4)] for m, v in times.items()})
    if "ragged" in outs and "solo" in outs:
        res["ragged_ids_equal_solo"] = bool(torch.equal(outs["ragged"], outs["solo"]))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
