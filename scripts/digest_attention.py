"""SHA-256 digests of everything the materialised-score attention path computes (_attn.py, csrc/softmax_row.h), for fixed seeds: one JSON
object {name: digest}.  Run on two builds of the package (each from its own tree: the package is imported from this file's parent
directory) the outputs must be equal key for key: the digests are over the raw float32 bits, so any changed launch argument or
floating-point expression shows.
  models   logits and flat_grads of small wav2vec2 (post-LN, stable-LN), WavLM, Wav2Vec2-Conformer (relative, rotary), SCConformerXL with and
           without `grad_samples` smaller than the batch, and one enc-dec teacher-forced step with the three dropout knobs on
  kernels  ops.softmax (plain and with `valid`), ops.log_softmax, ops.softmax_relbias, ops.softmax_relshift at row lengths 37, 257, 1500
           (below one item per thread, just above one, several) and valid in {1, T - 5, T}
Usage: python scripts/digest_attention.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256,) * 7,
           num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32)
POST_GROUP = dict(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False)
STABLE_LAYER = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
SMALL = dict(n_layers=2, d_model=256, n_heads=2, head_dim=128, subsampling_conv_channels=64)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def ctc_family(res, name, cls, cfg, dev):
    """logits + flat_grads of a model of the wav2vec2 family: 2 x 30000 samples (93 frames: two row blocks of the relbias kernel)."""
    from dynamic_asr_eval_amd import run_wav2vec2 as RW
    m = cls(cfg, device=dev)
    RW.init_synthetic(m, 3)
    m.eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 30000, generator=g).to(dev)
    with torch.enable_grad():
        out = m(x).logits
    gl = (torch.randn(out.shape, generator=g) / out.numel()).to(dev)
    m.zero_grad()
    m.backward(gl)
    res[name + ".logits"], res[name + ".flat_grads"] = sha(out), sha(m.flat_grads)


def conformer(res, name, grad_samples, dev):
    from dynamic_asr_eval_amd.model import SCConformerXL
    from dynamic_asr_eval_amd.synthetic_weights import init_synthetic
    m = init_synthetic(SCConformerXL(SMALL, vocab_size=128, device=dev), 5, blank_bias=1.5)
    m.grad_samples = grad_samples
    x = torch.randn(2, 80, 4800, generator=torch.Generator().manual_seed(21)).to(dev)      # T' = 600 >= 512: grad_samples applies
    with torch.enable_grad():
        out = m(audio_signal=x)['final_posteriors']
    gp = torch.randn(1, *out.shape[1:], generator=torch.Generator().manual_seed(22)).to(dev) / out[0].numel()
    m.zero_grad()
    m.backward(gp, n_active=1)
    res[name + ".logits"], res[name + ".flat_grads"] = sha(out), sha(m.flat_grads)


def enc_dec(res, dev):
    from dynamic_asr_eval_amd.enc_dec import EncDecSCConformerXL, calc_loss_enc_dec
    from dynamic_asr_eval_amd.synthetic_weights import init_synthetic
    from dynamic_asr_eval_amd.tokenizer import SyntheticTokenizer
    m = init_synthetic(EncDecSCConformerXL(dict(SMALL, dec_d_model=256, dec_layers=2, dec_heads=4, ctc_loss_weight=0.3), vocab_size=64, device=dev),
                       7, blank_bias=1.0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 80, 400, generator=g).to(dev)
    text = torch.randint(1, 64, (1, 11), generator=g)
    knobs = m.language_model_decoder
    knobs.dropout_emb, knobs.ff_out_dropout = 0.1, 0.2
    for layer in knobs.layers:
        layer[0].fn.dropout_p = 0.15
    m.random_seed, m._draws = 42, 0
    knobs.train()
    m.zero_grad()
    out = calc_loss_enc_dec(m, x, text, torch.LongTensor([400]), torch.LongTensor([11]), SyntheticTokenizer(64))
    knobs.eval()
    res["enc_dec.lm_posteriors"], res["enc_dec.ctc_posteriors"] = sha(out["lm_posteriors"]), sha(out["ctc_posteriors"])
    res["enc_dec.flat_grads"] = sha(m.flat_grads)


def kernels(res, dev):
    from dynamic_asr_eval_amd import ops
    B, nh, D, nbk = 2, 3, 8, 8
    for T in (37, 257, 1500):
        g = torch.Generator().manual_seed(T)
        S = torch.randn(B, nh, T, T, generator=g).to(dev)
        BD = torch.randn(B, nh, T, 2 * T - 1, generator=g).to(dev)
        gate = (1.0 + torch.rand(B, nh, T, generator=g)).to(dev)
        E = torch.randn(nbk, nh, generator=g).to(dev)
        table = ops.relative_position_buckets(T, nbk, 12).to(dev)
        res[f"softmax.T{T}"] = sha(ops.softmax(S))
        res[f"log_softmax.T{T}"] = sha(ops.log_softmax(S))
        for v in (1, T - 5, T):
            valid = torch.tensor([v], dtype=torch.int32, device=dev)
            res[f"softmax.T{T}.valid{v}"] = sha(ops.softmax(S, valid=valid))
            res[f"softmax_relbias.T{T}.valid{v}"] = sha(ops.softmax_relbias(S, gate, E, table, D, valid=valid))
            res[f"softmax_relshift.T{T}.valid{v}"] = sha(ops.softmax_relshift(S, BD, valid=valid))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from dynamic_asr_eval_amd.wav2vec2_conformer_model import Wav2Vec2ConformerForCTC
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
    from dynamic_asr_eval_amd.wavlm_model import WavLMForCTC
    res = {}
    ctc_family(res, "wav2vec2_post_ln", Wav2Vec2ForCTC, dict(TOY, **POST_GROUP), dev)
    ctc_family(res, "wav2vec2_stable_ln", Wav2Vec2ForCTC, dict(TOY, **STABLE_LAYER), dev)
    ctc_family(res, "wavlm", WavLMForCTC, dict(TOY, **POST_GROUP, num_buckets=8, max_bucket_distance=12), dev)
    for pos in ("relative", "rotary"):
        ctc_family(res, "wav2vec2_conformer_" + pos, Wav2Vec2ConformerForCTC,
                   dict(TOY, **POST_GROUP, position_embeddings_type=pos, hidden_act="swish"), dev)
    conformer(res, "sc_conformer_grad_samples_1_of_2", 1, dev)
    conformer(res, "sc_conformer", None, dev)
    enc_dec(res, dev)
    kernels(res, dev)
    line = json.dumps(res, indent=1, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
