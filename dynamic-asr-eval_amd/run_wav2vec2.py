"""wav2vec2 harness (BASELINE config 3) mirroring the reference's two wav2vec2 drivers, same flags (`lib.apply_args`,
reference wav2vec2/lib.py:477-493), same stdout lines (`Loaded model from`, `Total number of parameters`, `WER:`) and the same
`-log` line:
  --mode su       reference wav2vec2/tedlium/run.py:106-175: split the talk into STM utterances (`fetch_utterances`, :56-83) ->
                  `lib.dynamic_eval_su` (:155) -> per-utterance greedy decode, lower, strip, join (:156-160) -> normalise -> WER (:169)
  --mode chunked  reference wav2vec2/earnings22/run.py:59-117: `lib.dynamic_eval` over waveform windows (`-seq 131072 -overlap 0`,
                  :100) -> greedy decode of the stitched log-probs (:103) -> normalise -> WER (:114)
Like both reference drivers it processes the FIRST recording only (they `break` after it: tedlium/run.py:166, earnings22/run.py:111).

`AutoModelForCTC.from_pretrained("facebook/wav2vec2-base-960h")` and the corpora cannot be fetched offline, so the harness builds
the base architecture (HF `Wav2Vec2Config()` defaults: 7 conv layers of 512 channels, positional conv k=128 g=16, 12 x 768, vocab 32)
or the one a `config.json` names (`--config`, or `-c DIR` = a local HF model directory; the layer-norm / stable-LN layout of
large-960h-lv60-self included, and by `model_type` WavLM, Wav2Vec2-Conformer, Data2Vec-Audio, HuBERT, SEW, SEW-D and Wav2Vec2-BERT: load_pretrained_model) with
seeded weights, or loads a local HF state_dict (`-c file.pt` / `DIR/pytorch_model.bin`, torch.load(weights_only=True)), and evaluates a synthetic
TEDLIUM-shape talk (`--seconds`, utterances of 2-15 s).  An MMS directory (`adapter_attn_dim` in its config.json) runs with its
per-layer adapters; `--target-lang LANG` loads `DIR/adapter.LANG.safetensors` (or `.bin`) over the base weights and `DIR/vocab.json` as the tokenizer,
`--adapter-only` adapts the adapters and lm_head alone (Wav2Vec2ForCTC.adapter_only).  Reported WERs use this package's reduced text
normaliser (wer.basic_normalize), not whisper's EnglishTextNormalizer (un-vendored)."""
import argparse
import os
import time

import torch

from . import ops
from . import wav2vec2_lib as lib
from .datasets import fetch_utterances_from_lines, synthetic_text, synthetic_waveform
from .decoding import GreedyCTCDecoder
from . import data2vec_audio_model, hubert_model, sew_d_model, sew_model, wav2vec2_bert_model, wav2vec2_conformer_model, wavlm_model
from .wav2vec2_model import Wav2Vec2ForCTC, config_from_json, make_config, param_spec
from .wer import basic_normalize as normalize, word_error_rate_detail


def synthetic_talk(total_seconds=900.0, seed=7, sample_rate=16000):
    """A TEDLIUM-shape talk: STM lines (utterances of 2-15 s, every 9th segment `ignore_time_segment_in_scoring`) and ONE waveform
    [1, L] for the whole talk, resident once; the utterances are cut out of it by the reference's own rule below."""
    g = torch.Generator().manual_seed(seed)
    lines, t, k = [], 0.0, 0
    while t < total_seconds:
        d = float(2.0 + 13.0 * torch.rand(1, generator=g).item())
        d = min(d, total_seconds - t) if total_seconds - t > 2.0 else d
        if k % 9 == 8:
            text = "ignore_time_segment_in_scoring"
        else:
            text = " ".join(w.replace("w", "word") for w in synthetic_text(max(1, int(2.5 * d)), seed + k).split())
        lines.append(f"talk{seed} 1 spk{seed} {t:.2f} {t + d:.2f} <o,f0,unknown> {text}")
        t, k = t + d, k + 1
    return lines, synthetic_waveform(t, seed=seed, sample_rate=sample_rate).unsqueeze(0)


def fetch_utterances_synthetic(total_seconds=900.0, seed=7, sample_rate=16000, stm_path=None):
    """Utterance list exactly as reference wav2vec2/tedlium/run.py:56-83 builds it (datasets.fetch_utterances, pinned to the
    reference's output): from `stm_path` when given (the audio itself cannot be decoded offline: a synthetic waveform of the STM's
    span stands in), else from a synthetic talk."""
    if stm_path:
        with open(stm_path, 'r') as f:
            lines = f.read().split('\n')
        ends = [float(l.split(' ')[4]) for l in lines if len(l.split(' ')) >= 6]
        wave = synthetic_waveform(max(ends) + 1.0, seed=seed, sample_rate=sample_rate).unsqueeze(0)
    else:
        lines, wave = synthetic_talk(total_seconds, seed, sample_rate)
    utts, _ = fetch_utterances_from_lines(lines, wave, sample_rate)
    return utts


def init_synthetic(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    ones = ("layer_norm.weight", "original0") + tuple(getattr(model, "_norm_weight_suffixes", ()))      # a model's own norm names (SEW-D: `LayerNorm`)
    for name, p in model.named_parameters():
        if p.dim() == 1:
            v = (1.0 if name.endswith(ones) else 0.0) + 0.02 * torch.randn(p.shape, generator=g)
        else:
            fan_in = p[0].numel()
            v = torch.randn(p.shape, generator=g) / fan_in ** 0.5
        p.copy_(v.to(p.device))


def replicate(model, n):
    """n - 1 more replicas of `model` (same configuration and weights) for lib.dynamic_eval_su_many."""
    out = [model]
    for _ in range(max(0, n - 1)):
        m = type(model)(model.cfg, device=model.device)
        m.flat_params.copy_(model.flat_params)
        if hasattr(model, 'buffers_'):                           # the conformer's batch-norm statistics live outside the flat vector
            m.copy_buffers_from(model)
        m.frozen = set(model.frozen)
        m.bucket_frames, m.graph_after, m.graph_budget_bytes = model.bucket_frames, model.graph_after, model.graph_budget_bytes
        out.append(m.eval())
    return out


class VocabTokenizer:
    """A character tokenizer from an HF `vocab.json`, with CharTokenizer's surface (`vocab_size`, `blank_id` = the id of `<pad>`, `decode(ids)`,
    `tokenizer(text).input_ids`): `|` is the word delimiter, `<unk>` stands for every unknown character.  The file is flat `{token: id}` or
    MMS's nested `{lang: {token: id}}`, of which `lang` picks one."""
    SPECIAL = ("<pad>", "<s>", "</s>")

    def __init__(self, vocab):
        self.vocab = {str(k): int(v) for k, v in vocab.items()}
        if "<pad>" not in self.vocab:
            raise KeyError("vocab.json: no <pad> token (the CTC blank)")
        self.ids = {i: t for t, i in self.vocab.items()}
        self.blank_id = self.vocab["<pad>"]
        self.unk_id = self.vocab.get("<unk>", self.blank_id)
        self.vocab_size = max(self.ids) + 1

    @classmethod
    def from_json(cls, path, lang=None):
        import json
        with open(path) as f:
            src = json.load(f)
        if src and all(isinstance(v, dict) for v in src.values()):        # MMS: one vocabulary per language
            if lang is None and len(src) == 1:
                lang = next(iter(src))
            if lang not in src:
                raise KeyError(f"{path}: no vocabulary for language {lang!r} (it holds {sorted(src)[:8]})")
            src = src[lang]
        return cls(src)

    def decode(self, ids):
        out = []
        for i in ids:
            t = self.ids.get(int(i), "<unk>")
            if t not in self.SPECIAL:
                out.append(" " if t == "|" else t)
        return "".join(out)

    def __call__(self, text):
        from types import SimpleNamespace
        word = self.vocab.get("|", self.unk_id)
        return SimpleNamespace(input_ids=[word if ch == " " else self.vocab.get(ch, self.unk_id) for ch in text])


def adapter_names(cfg):
    """The names transformers' `_get_adapters()` lists for this configuration: every adapter layer's parameters and lm_head's."""
    return [n for n, _, _ in param_spec(make_config(cfg)) if ".adapter_layer." in n or n.startswith("lm_head.")]


def load_target_lang(directory, lang, cfg):
    """transformers' `load_adapter(lang)` from local files only: `DIR/adapter.LANG.safetensors`, else `DIR/adapter.LANG.bin`
    (torch.load(weights_only=True)).  Its keys must be exactly adapter_names(cfg), else KeyError naming the missing and the unexpected ones.
    Returns (state dict, vocab size of its lm_head.weight)."""
    st, pt = (os.path.join(directory, f"adapter.{lang}.{ext}") for ext in ("safetensors", "bin"))
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd, path = load_file(st), st
    elif os.path.exists(pt):
        sd, path = torch.load(pt, map_location="cpu", weights_only=True), pt
    else:
        raise FileNotFoundError(f"no adapter file for language {lang!r}: neither {st} nor {pt} exists (local files only)")
    names = adapter_names(cfg)
    if not names or not any(".adapter_layer." in n for n in names):
        raise KeyError(f"--target-lang {lang}: this configuration has no adapters (adapter_attn_dim with do_stable_layer_norm)")
    missing, unexpected = [n for n in names if n not in sd], [k for k in sd if k not in names]
    if missing or unexpected:
        raise KeyError(f"{path}: the adapter file does not fit the model: missing keys {missing}, unexpected keys {unexpected}")
    return sd, int(sd["lm_head.weight"].shape[0])


def model_type(cfg_path):
    """`model_type` of an HF config.json ('' when it names none)."""
    import json
    with open(cfg_path) as f:
        src = json.load(f)
    return src.get('model_type', '') if isinstance(src, dict) else ''


def load_pretrained_model(args, device):
    """reference wav2vec2/lib.py:20-23 (`AutoModelForCTC.from_pretrained(checkpoint)`) — offline: `-c DIR` is a local HF model directory
    (`config.json` read as plain JSON for the architecture and the layout flags + `pytorch_model.bin`), `-c FILE` a bare state_dict at the
    base-960h architecture or at `--config PATH.json`; without a checkpoint: seeded weights at that architecture.  A config.json whose
    `model_type` is "wavlm" builds WavLMForCTC (wavlm_model.py), "wav2vec2-conformer" Wav2Vec2ConformerForCTC (wav2vec2_conformer_model.py),
    "data2vec-audio" Data2VecAudioForCTC (data2vec_audio_model.py), "hubert" HubertForCTC (hubert_model.py), "sew" SEWForCTC
    (sew_model.py), "sew-d" SEWDForCTC (sew_d_model.py), "wav2vec2-bert" Wav2Vec2BertForCTC (wav2vec2_bert_model.py: it reads the waveform
    through the filter-bank front end on the device), under `-c DIR` and under `--config` alike; anything else Wav2Vec2ForCTC."""
    cfg_path, ckpt = getattr(args, 'config', '') or '', args.checkpoint
    if ckpt and os.path.isdir(ckpt):
        cfg_path, ckpt = cfg_path or os.path.join(ckpt, 'config.json'), os.path.join(ckpt, 'pytorch_model.bin')
    kind = model_type(cfg_path) if cfg_path else ''         # what AutoModelForCTC dispatches on
    if kind == 'parakeet_ctc':
        raise ops.DynError(f'{cfg_path}: model_type "parakeet_ctc" takes log-mel features [B, T, num_mel_bins], not waveforms: build '
                           'parakeet_model.ParakeetForCTC and drive it with nvidia_ctc_lib.dynamic_eval (the reference\'s nvidia_ctc/lib.py)')
    if kind == 'lasr_ctc':
        raise ops.DynError(f'{cfg_path}: model_type "lasr_ctc" takes log-mel features [B, T, num_mel_bins], not waveforms: build '
                           'lasr_model.LasrForCTC and drive it with nvidia_ctc_lib.dynamic_eval (the reference\'s nvidia_ctc/lib.py)')
    if kind == 'parakeet_tdt':
        raise ops.DynError(f'{cfg_path}: model_type "parakeet_tdt" is a transducer over log-mel features [B, T, num_mel_bins], not a CTC model '
                           'over waveforms: build parakeet_tdt_model.ParakeetForTDT and drive it with parakeet_tdt_lib.dynamic_eval')
    if kind == 'parakeet_rnnt':
        raise ops.DynError(f'{cfg_path}: model_type "parakeet_rnnt" is a transducer over log-mel features [B, T, num_mel_bins], not a CTC model '
                           'over waveforms: build parakeet_rnnt_model.ParakeetForRNNT and drive it with '
                           'parakeet_tdt_lib.dynamic_eval_transducer_loss')
    if kind == 'nemotron_asr_streaming':
        raise ops.DynError(f'{cfg_path}: model_type "nemotron_asr_streaming" is a transducer over log-mel features [B, T, num_mel_bins], not a '
                           'CTC model over waveforms: build nemotron_asr_streaming_model.NemotronAsrStreamingForRNNT and drive it with '
                           'parakeet_tdt_lib.dynamic_eval_transducer_loss')
    if kind == 'nemotron3_5_asr':
        raise ops.DynError(f'{cfg_path}: model_type "nemotron3_5_asr" is a transducer over log-mel features [B, T, num_mel_bins], not a '
                           'CTC model over waveforms: build nemotron3_5_asr_model.Nemotron3_5AsrForRNNT (prompt_ids= or default_prompt_id '
                           'choose the language) and drive it with parakeet_tdt_lib.dynamic_eval_transducer_loss')
    if kind == 'cohere_asr':
        raise ops.DynError(f'{cfg_path}: model_type "cohere_asr" is an attention encoder-decoder over log-mel features [B, T, num_mel_bins], not a '
                           'CTC model over waveforms: build cohere_asr_model.CohereAsrForConditionalGeneration and drive it with '
                           'cohere_asr_lib.dynamic_eval_seq2seq_loss')
    lang, adapter_sd, tokenizer = getattr(args, 'target_lang', '') or '', None, None
    if lang:
        if kind not in ('', 'wav2vec2') or not (args.checkpoint and os.path.isdir(args.checkpoint)):
            raise KeyError('--target-lang needs -c DIR, a local wav2vec2 (MMS) model directory with adapter.LANG.safetensors / .bin')
        cfg = config_from_json(cfg_path)
        adapter_sd, vocab = load_target_lang(args.checkpoint, lang, cfg)
        cfg = dict(cfg, vocab_size=vocab)                    # the model is built at the adapter file's vocabulary
    if ckpt and os.path.isdir(args.checkpoint) and os.path.exists(os.path.join(args.checkpoint, 'vocab.json')):
        tokenizer = VocabTokenizer.from_json(os.path.join(args.checkpoint, 'vocab.json'), lang or None)
    if kind == 'wavlm':
        model = wavlm_model.WavLMForCTC(wavlm_model.config_from_json(cfg_path), device=device)
    elif kind == 'wav2vec2-conformer':
        model = wav2vec2_conformer_model.Wav2Vec2ConformerForCTC(wav2vec2_conformer_model.config_from_json(cfg_path), device=device)
    elif kind == 'data2vec-audio':
        model = data2vec_audio_model.Data2VecAudioForCTC(data2vec_audio_model.config_from_json(cfg_path), device=device)
    elif kind == 'hubert':
        model = hubert_model.HubertForCTC(hubert_model.config_from_json(cfg_path), device=device)
    elif kind == 'sew':
        model = sew_model.SEWForCTC(sew_model.config_from_json(cfg_path), device=device)
    elif kind == 'sew-d':
        model = sew_d_model.SEWDForCTC(sew_d_model.config_from_json(cfg_path), device=device)
    elif kind == 'wav2vec2-bert':
        model = wav2vec2_bert_model.Wav2Vec2BertForCTC(wav2vec2_bert_model.config_from_json(cfg_path), device=device)
    elif lang:
        model = Wav2Vec2ForCTC(cfg, device=device)
    else:
        model = Wav2Vec2ForCTC(config_from_json(cfg_path) if cfg_path else None, device=device)
    if ckpt:
        sd = torch.load(ckpt, map_location='cpu', weights_only=True)
        if adapter_sd is not None:                           # HF's ignore_mismatched_sizes on this path: the base lm_head of another vocabulary goes
            sd = {k: v for k, v in sd.items() if k not in adapter_sd or tuple(v.shape) == tuple(adapter_sd[k].shape)}
            sd.update(adapter_sd)
        res = model.load_state_dict(sd, strict=False)
        missing = getattr(res, 'missing_keys', [])
        if missing:
            raise KeyError(f'checkpoint {ckpt}: {len(missing)} parameters of the model are missing (e.g. {missing[:3]})')
        # extractor parameters the configuration has no slot for: the other extractor layout, which would otherwise run with them dropped
        extra = [k for k in getattr(res, 'unexpected_keys', []) if k.startswith(model._prefix + 'feature_extractor.conv_layers.')]
        if extra:
            raise KeyError(f'checkpoint {ckpt}: {len(extra)} feature-extractor parameters do not belong to the configured layout '
                           f'(e.g. {extra[:3]}): pass its config.json (-c DIR or --config)')
        # adapter parameters the configuration has no slot for: an MMS checkpoint, which would otherwise run as another model
        extra = [k for k in getattr(res, 'unexpected_keys', []) if '.adapter_layer.' in k]
        if extra:
            raise KeyError(f'checkpoint {ckpt}: {len(extra)} adapter parameters do not belong to the configured model (e.g. {extra[:3]}): '
                           f'pass its config.json with adapter_attn_dim (-c DIR or --config)')
    else:
        init_synthetic(model, args.seed)
    if getattr(args, 'adapter_only', False):
        model.adapter_only()
    return model, tokenizer if tokenizer is not None else lib.CharTokenizer()


def main(args):
    assert args.split in ['test', 'dev'], f'Split must be either test or dev (got {args.split})'
    device = torch.device('cuda', 0)
    model, tokenizer = load_pretrained_model(args, device)
    print(f'Loaded model from {args.checkpoint}')
    print(f'Total number of parameters: {sum(p.numel() for p in model.parameters()) / 1e6:.2f}M')
    model.eval()
    if isinstance(tokenizer, lib.CharTokenizer):
        tokenizer.blank_id = 0
    decoder = GreedyCTCDecoder(tokenizer=tokenizer, blank_id=tokenizer.blank_id, device=device)
    # the reference's driver walks the talks of the split, one dynamic_eval call each (tedlium/run.py:139-160); offline: `--talks` synthetic talks
    # (or the one `--stm` names).  Talks are independent (weights restored per call), so `--chains` of them can be in flight (lib.dynamic_eval_su_many)
    n_talks = 1 if args.stm else max(1, int(getattr(args, 'talks', 1)))
    talks = [fetch_utterances_synthetic(args.seconds, args.seed + (0 if args.split == 'test' else 1000) + 17 * t, stm_path=args.stm or None)
             for t in range(n_talks)]
    utterances = [u for talk in talks for u in talk]
    all_texts, all_golds = [], []
    torch.cuda.synchronize()
    t0 = time.time()
    chains = max(1, min(int(getattr(args, 'chains', 1)), n_talks))
    if args.mode == 'su' and chains > 1:
        outs = lib.dynamic_eval_su_many(args, replicate(model, chains), talks, args.seq_len, args.overlap, tokenizer, None, optim=lib.MADGRAD,
                                        lr_args={'lr': args.lr})
    for t, talk in enumerate(talks):
        gold_text = normalize(" ".join(u['text'] for u in talk)).lower()
        if args.mode == 'su':
            utterances_out = outs[t] if chains > 1 else lib.dynamic_eval_su(args, model, talk, args.seq_len, args.overlap, tokenizer, None, use_tqdm=False,
                                                                            optim=lib.MADGRAD, lr_args={'lr': args.lr})
            for i, utt in enumerate(utterances_out):
                utterances_out[i]['text'] = decoder(utt['probs']).lower()
            text = ' '.join([el['text'].strip() for el in utterances_out])
        else:
            audio_spec = torch.cat([u['waveform'] for u in talk], -1)                       # [1, L] waveform of the whole talk
            logits = lib.dynamic_eval(args, model, audio_spec, args.seq_len, args.overlap, tokenizer, None, use_tqdm=False,
                                      optim=lib.MADGRAD, lr_args={'lr': args.lr}, return_device=True)
            text = decoder(logits).lower()
        out = normalize(text).lower()
        if args.verbose:
            print(gold_text[:200], '\n', out[:200], '\n\n')
        all_texts.append(out)
        all_golds.append(gold_text)
    torch.cuda.synchronize()
    dt = time.time() - t0
    wer, words, ins_rate, del_rate, sub_rate = word_error_rate_detail(hypotheses=all_texts, references=all_golds)
    print(f'WER: {wer}')
    if args.log != '':
        with open(args.log, 'a') as f:
            f.write(f'{args.checkpoint}\t overlap: {args.overlap}\t seq_len: {args.seq_len}\t WER: {wer}\n')
    audio_s = sum(u['waveform'].shape[-1] for u in utterances) / 16000.0
    print(f'wav2vec2 {args.mode}: {len(utterances)} utterances, {audio_s:.0f} s of audio in {dt:.2f} s -> {audio_s / dt:.1f} audio-s/s')
    return wer


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['su', 'chunked'], default='su', help='su: tedlium/run.py (per utterance); chunked: earnings22/run.py')
    ap.add_argument('--seconds', type=float, default=900.0)
    ap.add_argument('--lr', type=float, default=1e-6)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--stm', type=str, default='', help='TEDLIUM .stm file: its segments define the utterances (reference tedlium/run.py:56-83)')
    ap.add_argument('--talks', type=int, default=1, help='synthetic talks of --seconds each (the reference walks the talks of the split)')
    ap.add_argument('--config', type=str, default='', help='HF config.json: architecture and layout (feat_extract_norm, conv_bias, do_stable_layer_norm) '
                                                           'for -c FILE or seeded weights; -c DIR reads DIR/config.json')
    ap.add_argument('--target-lang', type=str, default='', help='MMS: load DIR/adapter.LANG.safetensors (or .bin) over the base weights of -c DIR; '
                                                                'local files only')
    ap.add_argument('--adapter-only', action='store_true', help='adapt only the adapters and lm_head (the MMS recipe); the rest is frozen and its '
                                                                'weight gradients are skipped')
    ap.add_argument('--chains', type=int, default=1, help='talks in flight on the GPU (mode su): one model replica + HIP stream each')
    return ap


if __name__ == '__main__':
    main(lib.apply_args(build_parser()))
