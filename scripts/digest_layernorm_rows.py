"""SHA-256 digests of everything the wave-per-row LayerNorm kernels compute (csrc/layernorm_row.h and the six files built on it), for fixed
seeds: one JSON object {name: digest}.  Run on two builds of the library (DYN_LIB_PATH picks the shared library) the outputs must be equal
key for key: the digests are over the raw float32 bits, so any changed launch argument, summation order or floating-point expression shows.
  kernels  through the ops wrappers, forward and backward outputs with every weight gradient, rows in {7, 1031} (one idle wave; more rows than
           any backward's workgroup cap): layernorm / rmsnorm at C in {256, 512, 768, 1024, 1280, 2048} with dx_beta 0 and 1 and one
           lockstep-grouped call; bias_layernorm_gelu at C in {64, 128, 256, 512, 768, 1024} with and without the conv bias; posconv_ln_gelu
           (both outputs), squeeze_ln and squeeze at H in {256, 512, 768, 1024}, T = 33, with and without `valid`; attn_adapter at
           H = 256 .. 2048, A = 16, M = 37
  models   logits and flat_grads of toy Wav2Vec2ForCTC (layer-norm extractor, stable-LN encoder, adapter_attn_dim 16), Data2Vec-Audio, SEW,
           SEW-D and a small SCConformerXL; one enc-dec teacher-forced step; one enc-dec greedy decode (token ids and the last step's logits)
Usage: python scripts/digest_layernorm_rows.py [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from digest_attention import SMALL, STABLE_LAYER, TOY, conformer, ctc_family, enc_dec, sha  # noqa: E402

BASE = {k: v for k, v in TOY.items() if not k.startswith("num_conv_pos")}
SEW = dict(TOY, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), squeeze_factor=2)
ROWS = (7, 1031)


def norms(res, dev):
    from dynamic_asr_eval_amd import ops
    for C in (256, 512, 768, 1024, 1280, 2048):
        for rows in ROWS:
            g = torch.Generator().manual_seed(C + rows)
            x, dy, old = (torch.randn(rows, C, generator=g).to(dev) for _ in range(3))
            gamma, beta = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
            y, mean, rstd = ops.layernorm(x + 3.0, gamma, beta)
            yr, rr = ops.rmsnorm(x, gamma)
            res[f"layernorm.C{C}.rows{rows}"] = sha(torch.cat([y.flatten(), mean, rstd]))
            res[f"rmsnorm.C{C}.rows{rows}"] = sha(torch.cat([yr.flatten(), rr]))
            for dx_beta in (0.0, 1.0):
                dg, db, dgr = (torch.zeros(C, device=dev) for _ in range(3))
                dx = ops.layernorm_bwd(x + 3.0, gamma, mean, rstd, dy, old.clone(), dg, db, dx_beta=dx_beta)
                dxr = ops.rmsnorm_bwd(x, gamma, rr, dy, old.clone(), dgr, dx_beta=dx_beta)
                res[f"layernorm_bwd.C{C}.rows{rows}.dx_beta{dx_beta:g}"] = sha(torch.cat([dx.flatten(), dg, db]))
                res[f"rmsnorm_bwd.C{C}.rows{rows}.dx_beta{dx_beta:g}"] = sha(torch.cat([dxr.flatten(), dgr]))
    # a lockstep group: 4 samples of 37 rows over 2 replicas whose parameters lie `n` floats apart in one flat buffer
    C, R, n = 512, 2, 2 * 512 + 24
    g = torch.Generator().manual_seed(5)
    flat, gflat = torch.randn(R, n, generator=g).to(dev), torch.zeros(R, n, device=dev)
    view = lambda buf, lo: ops.GroupParam(buf[:, lo:lo + C], R, n)     # noqa: E731
    x, dy = torch.randn(4, 37, C, generator=g).to(dev), torch.randn(4, 37, C, generator=g).to(dev)
    y, mean, rstd = ops.layernorm(x, view(flat, 8), view(flat, 8 + C + 8))
    dx = ops.layernorm_bwd(x, view(flat, 8), mean, rstd, dy, torch.empty_like(x), view(gflat, 8), view(gflat, 8 + C + 8))
    res["layernorm.grouped"] = sha(torch.cat([y.flatten(), mean, rstd, dx.flatten(), gflat.flatten()]))


def bias_ln_gelu(res, dev):
    from dynamic_asr_eval_amd import ops
    for C in (64, 128, 256, 512, 768, 1024):
        for rows in ROWS:
            g = torch.Generator().manual_seed(C + rows)
            z, dact = torch.randn(rows, C, generator=g).to(dev), torch.randn(rows, C, generator=g).to(dev)
            gamma, beta, cb = ((o + 0.1 * torch.randn(C, generator=g)).to(dev) for o in (1.0, 0.0, 0.5))
            for name, bias in (("bias", cb), ("nobias", None)):
                act, mean, rstd = ops.bias_layernorm_gelu(z, bias, gamma, beta)
                dg, db, dc = (torch.zeros(C, device=dev) for _ in range(3))
                dz = ops.bias_layernorm_gelu_bwd(z, bias, gamma, beta, mean, rstd, dact, dg, db, dc if bias is not None else None)
                res[f"bias_layernorm_gelu.C{C}.rows{rows}.{name}"] = sha(torch.cat([act.flatten(), mean, rstd, dz.flatten(), dg, db, dc]))


def grouped_rows(res, dev):
    """posconv_ln_gelu, squeeze_ln and squeeze: rows gathered from the group-major layout of the grouped GEMMs."""
    from dynamic_asr_eval_amd import ops
    B, T, G, s, pad = 2, 33, 4, 2, 2
    T2 = T // s
    for H in (256, 512, 768, 1024):
        g = torch.Generator().manual_seed(H)
        cg = H // G
        yg, dact = torch.randn(B, G, T + 3, cg, generator=g).to(dev), torch.randn(B, T, H, generator=g).to(dev)
        h, dz = torch.randn(B, T, H, generator=g).to(dev), torch.randn(B, T2, H, generator=g).to(dev)
        gamma, beta, bias = ((o + 0.1 * torch.randn(H, generator=g)).to(dev) for o in (1.0, 0.0, 0.5))
        for vname, v, v2 in (("all", None, None), ("valid", 31, T2 - 1)):
            valid = None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)
            valid2 = None if v2 is None else torch.tensor([v2], dtype=torch.int32, device=dev)
            act, xg, mean, rstd = ops.posconv_ln_gelu(yg, bias, T, pad=pad, valid=valid, want_act=True, want_packed=True)
            db = torch.zeros(H, device=dev)
            dyg = ops.posconv_ln_gelu_bwd(yg, bias, mean, rstd, dact, db, valid=valid)
            res[f"posconv_ln_gelu.H{H}.{vname}"] = sha(torch.cat([act.flatten(), xg.flatten(), mean, rstd, dyg.flatten(), db]))
            z, mean, rstd = ops.squeeze_ln(h, yg, bias, gamma, beta, s, valid=valid2)
            dg, dbt, db = (torch.zeros(H, device=dev) for _ in range(3))
            dh, dyg = ops.squeeze_ln_bwd(h, yg, bias, gamma, mean, rstd, dz, s, dg, dbt, db, valid=valid2)
            res[f"squeeze_ln.H{H}.{vname}"] = sha(torch.cat([z.flatten(), mean, rstd, dh.flatten(), dyg.flatten(), dg, dbt, db]))
            z = ops.squeeze(h, yg, bias, s, valid=valid2)
            db = torch.zeros(H, device=dev)
            dh, dyg = ops.squeeze_bwd(yg, bias, dz, T, s, db, valid=valid2)
            res[f"squeeze.H{H}.{vname}"] = sha(torch.cat([z.flatten(), dh.flatten(), dyg.flatten(), db]))


def adapter(res, dev):
    from dynamic_asr_eval_amd import ops
    M, A = 37, 16
    for H in range(256, 2049, 256):
        g = torch.Generator().manual_seed(H)
        x, dy = torch.randn(M, H, generator=g).to(dev), torch.randn(M, H, generator=g).to(dev)
        gamma, beta, b2 = ((o + 0.1 * torch.randn(H, generator=g)).to(dev) for o in (1.0, 0.0, 0.0))
        w1, w2 = (torch.randn(A, H, generator=g) / H ** 0.5).to(dev), (torch.randn(H, A, generator=g) / A ** 0.5).to(dev)
        b1 = (0.1 * torch.randn(A, generator=g)).to(dev)
        y, mean, rstd, a = ops.attn_adapter(x, gamma, beta, w1, b1, w2, b2, save=True)
        grads = [torch.zeros_like(t) for t in (gamma, beta, w1, b1, w2, b2)]
        dx = ops.attn_adapter_bwd(x, gamma, beta, w1, w2, mean, rstd, a, dy, *grads)
        res[f"attn_adapter.H{H}"] = sha(torch.cat([t.flatten() for t in (y, mean, rstd, a, dx, *grads)]))


def greedy_decode(res, dev):
    """Twelve fused decoder steps (csrc/decoder_step.hip) of a small enc-dec model: the chosen ids and the logits of the last step."""
    from dynamic_asr_eval_amd import ops
    from dynamic_asr_eval_amd._lib import check, load
    from dynamic_asr_eval_amd.enc_dec import DEC, EncDecSCConformerXL
    from dynamic_asr_eval_amd.synthetic_weights import init_synthetic
    m = init_synthetic(EncDecSCConformerXL(dict(SMALL, dec_d_model=256, dec_layers=2, dec_heads=4, ctc_loss_weight=0.3), vocab_size=64, device=dev),
                       7, blank_bias=1.0)
    x = torch.randn(1, 80, 400, generator=torch.Generator().manual_seed(0)).to(dev)
    res["enc_dec.greedy.ids"] = json.dumps(m.generate(x, max_tokens=12)["text_sequence"])
    n, P, L, dd = 12, m.P, m.dec["dec_layers"], m.dec["dec_d_model"]
    with torch.no_grad(), ops.use_workspace(m._scratch()):
        h = m.forward(x)["hidden"][0]
        kv = [ops.linear(h, P[f"{DEC}layers.{l}.cross.kv.weight"], P[f"{DEC}layers.{l}.cross.kv.bias"]) for l in range(L)]
        cache = [torch.empty(n + 1, 3 * dd, device=dev, dtype=torch.float32) for _ in range(L)]
        tok = torch.zeros(n + 2, dtype=torch.int32, device=dev)
        desc, keep = m._decoder_desc(kv, cache, tok, h.shape[0])
        check(load().dyn_decoder_steps(ctypes.byref(desc), 0, n, 0, 1.0, 0, 0, torch.cuda.current_stream().cuda_stream), "dyn_decoder_steps")
        res["enc_dec.greedy.tokens"], res["enc_dec.greedy.last_logits"] = sha(tok), sha(keep[1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from dynamic_asr_eval_amd.data2vec_audio_model import Data2VecAudioForCTC
    from dynamic_asr_eval_amd.sew_d_model import SEWDForCTC
    from dynamic_asr_eval_amd.sew_model import SEWForCTC
    from dynamic_asr_eval_amd.wav2vec2_model import Wav2Vec2ForCTC
    res = {}
    norms(res, dev)
    bias_ln_gelu(res, dev)
    grouped_rows(res, dev)
    adapter(res, dev)
    ctc_family(res, "wav2vec2_stable_ln_adapter", Wav2Vec2ForCTC, dict(TOY, **STABLE_LAYER, adapter_attn_dim=16), dev)
    ctc_family(res, "data2vec_audio", Data2VecAudioForCTC, dict(BASE, num_conv_pos_embedding_groups=4), dev)
    ctc_family(res, "sew", SEWForCTC, dict(SEW, feat_extract_norm="layer", conv_bias=True), dev)
    ctc_family(res, "sew_d", SEWDForCTC, dict(SEW, feat_extract_norm="layer", conv_bias=True, position_buckets=8, max_position_embeddings=32), dev)
    conformer(res, "sc_conformer", None, dev)
    enc_dec(res, dev)
    greedy_decode(res, dev)
    line = json.dumps(res, indent=1, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
