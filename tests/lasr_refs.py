"""References for the LASR (MedASR) tests: torch restatements (any dtype, CPU) of the 32-tap conv-module kernels of csrc/convmod_bn.hip whose
depthwise step is torch's own `conv1d(..., padding="same", groups=C)` and autograd of it (so torch's padding rule, 15 frames left and 16 right
at 32 taps, is the oracle for the asymmetry, not an index formula written here), the transformers pair the model tests compare against, and
the test-side oracle of the reference's third loop (reference nvidia_ctc/lib.py:35-193) on transformers' LasrForCTC."""
import random

import torch
import torch.nn.functional as F

KW = 32
TOY = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, subsampling_conv_channels=256, num_mel_bins=128,
           dropout=0.0, dropout_positions=0.0, layerdrop=0.0, activation_dropout=0.0, attention_dropout=0.0)
WIDE = dict(TOY, hidden_size=512, num_hidden_layers=1, num_attention_heads=8)
VOCAB, PAD = 40, 39
SPEC_AUGMENT = {'n_time_masks': 3, 'n_freq_masks': 3, 'freq_mask_param': 40, 'time_mask_param': -1, 'min_p': 0.05, 'zero_masking': False}


# ----------------------------------------------------------------------------------------------------------- conv-module kernels
def _rows(T, valid):
    return T if valid is None else max(0, min(int(valid), T))


def _same_dw(x, w, bias=None):
    """x [B, T, C] channels-last through torch's SAME-padded depthwise Conv1d, w [C, KW]."""
    return F.conv1d(x.transpose(1, 2), w.unsqueeze(1), bias, padding="same", groups=w.shape[0]).transpose(1, 2)


def convmod_bn_ref(u, w, cbias, mean, var, weight, bias, eps, valid=None):
    """(s, gl, c) of dyn_convmod_bn_fwd in u's dtype: u [B, T, 2C], w [C, KW]; rows >= valid of the GLU output read as zeros, rows >= valid of
    all three outputs are zeros."""
    T = u.shape[1]
    v = _rows(T, valid)
    gl = F.glu(u, dim=-1)
    gl[:, v:] = 0
    c = _same_dw(gl, w, cbias).contiguous()
    s = F.silu((c - mean) * torch.rsqrt(var + eps) * weight + bias)
    c[:, v:] = 0
    s[:, v:] = 0
    return s, gl, c


def convmod_bn_bwd_act_ref(c, mean, var, weight, bias, ds, eps, valid=None):
    """(dc, dweight, dbias, dcbias) of dyn_convmod_bn_bwd_act by autograd in c's dtype; rows >= valid give dc = 0 and no term of the sums."""
    T = c.shape[1]
    v = _rows(T, valid)
    cr, wr, br = c[:, :v].clone().requires_grad_(), weight.clone().requires_grad_(), bias.clone().requires_grad_()
    s = F.silu((cr - mean) * torch.rsqrt(var + eps) * wr + br)
    s.backward(ds[:, :v])
    dc = torch.zeros_like(c)
    dc[:, :v] = cr.grad
    zero = torch.zeros_like(weight)
    return dc, (wr.grad if v else zero), (br.grad if v else zero), dc.sum((0, 1))


def glu_dwconv1d_dgrad_ref(u, w, dc, valid=None):
    """du of dyn_glu_dwconv1d_dgrad by autograd in u's dtype: GLU -> SAME depthwise conv, output gradient dc (all T rows of it are read), rows
    >= valid of du zeros."""
    T = u.shape[1]
    v = _rows(T, valid)
    ur = u.clone().requires_grad_()
    _same_dw(F.glu(ur, dim=-1), w).backward(dc)
    du = ur.grad.clone()
    du[:, v:] = 0
    return du


def dwconv1d_wgrad_ref(gl, dc, KW=KW):
    """dw [C, KW] of dyn_dwconv1d_wgrad(gl, dc): autograd of the SAME depthwise conv with respect to its taps, in gl's dtype."""
    w = torch.zeros(gl.shape[2], KW, dtype=gl.dtype, requires_grad=True)
    _same_dw(gl, w).backward(dc)
    return w.grad


# ----------------------------------------------------------------------------------------------------------- the transformers pair
def hf_config(arch=TOY, **over):
    from transformers import LasrCTCConfig
    return LasrCTCConfig(vocab_size=VOCAB, pad_token_id=PAD, encoder_config=dict(arch, **over))


def hf_model(arch=TOY, seed=0, blank_bias=0.0, **over):
    """transformers' LasrForCTC in eval mode with the 1-D parameters (biases, norm weights) and the batch norms' running statistics
    randomised, as parakeet_refs.hf_model does (transformers initialises them to trivial values).  `blank_bias` is added to the blank's
    ctc_head bias (the loop tests: a random model otherwise emits a token at almost every frame)."""
    from transformers import LasrForCTC
    torch.manual_seed(seed)
    cfg = hf_config(arch, **over)
    ref = LasrForCTC(cfg).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
        ref.ctc_head.bias[PAD] += blank_bias
    return cfg, ref


# ----------------------------------------------------------------------------------------------------------- the loop's oracle
class Tokenizer:
    """NeMo's tokenizer surface as the reference loop uses it (`vocab_size`, `ids_to_text`, `text_to_ids`): token i <-> the word "w<i>"."""

    def __init__(self, vocab_size):
        self.vocab_size = int(vocab_size)

    def ids_to_text(self, ids):
        return " ".join(f"w{int(i)}" for i in ids)

    def text_to_ids(self, text):
        return [int(w[1:]) for w in text.split()]


def dynamic_eval_ref(args, model, spec, seq_len, overlap, tokenizer, num_negatives, lr_args, spec_augment_config=SPEC_AUGMENT, generator=None,
                     adapt=True, labels_out=None):
    """reference nvidia_ctc/lib.py:35-193 restated on transformers' LasrForCTC (CPU), as tests/parakeet_refs.py restates it on ParakeetForCTC:
    torch.nn.CTCLoss, torch.optim.Adam, SpecAugment masks drawn on the host by the product's rule and applied by
    oracle.dynamic_eval_ref.apply_masks.  What this family changes: the frozen parts are `encoder.subsampler` and `ctc_head`, the
    downsampling factor the overlap is checked against is 4, and a window's ratio u_len / ds_len is not an integer (128 / 29), so
    overlap_ds = int(overlap / ratio) truncates.  Returns the stitched log-probs as a numpy array."""
    from dynamic_asr_eval_amd.augment import SpecAugment
    from oracle.dynamic_eval_ref import apply_masks, greedy_ctc_ids
    spec_n = spec.shape[-1]                                                                      # :58
    downsampling_factor = 4
    original = [p.clone().detach() for p in model.parameters()]                                  # :63-64
    blank = tokenizer.vocab_size
    ctc_loss_fn = torch.nn.CTCLoss(blank=blank, reduction='sum')                                 # :66
    augmentation = SpecAugment(**spec_augment_config)                                            # :72
    model.eval()
    frozen = []
    for part in (model.encoder.subsampler, model.ctc_head):                                      # :81-86
        for p in part.parameters():
            frozen.append((p, p.requires_grad))
            p.requires_grad = False
    optimizer = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], **lr_args)  # :105
    if seq_len > spec_n:
        seq_len, overlap = spec_n, 0
    assert overlap / downsampling_factor == overlap // downsampling_factor                       # :110
    C = tokenizer.vocab_size + 1
    all_logits, logit_count = torch.zeros((1, spec_n // 4 + seq_len, C)), torch.zeros((1, spec_n // 4 + seq_len, C))     # :113
    last_ulen, kill_next, logit_position = None, False, 0
    training_data = {}
    for i in range(0, spec_n, seq_len - overlap):                                                # :116-125
        audio_chunk = spec[:, :, i:i + seq_len]
        u_len = audio_chunk.shape[-1]
        if kill_next:
            break
        elif last_ulen is not None and u_len < last_ulen:
            kill_next = True
        last_ulen = u_len
        training_data[i] = audio_chunk
    model_outputs = {}
    for epoch in range(args.__dict__.get('epochs', 1)):                                          # :127
        model_outputs = {}
        training_keys = list(training_data.keys())
        training_keys = random.sample(training_keys, len(training_keys)) if args.__dict__.get('shuffle', False) else training_keys
        for i in training_keys:
            audio_chunk = training_data[i].clone().repeat(num_negatives + 1, 1, 1)               # :135-136
            for j in range(num_negatives):                                                       # :137
                apply_masks(audio_chunk[j], augmentation.draw(audio_chunk.shape[1], audio_chunk.shape[2], generator), augmentation.zero_masking)
            u_len = audio_chunk.shape[-1]
            log_p = torch.log_softmax(model(input_features=audio_chunk.transpose(1, 2)).logits, dim=-1)      # :141-142
            ids = greedy_ctc_ids(log_p[-1].detach(), blank)                                      # :144
            if labels_out is not None:
                labels_out.append(list(ids))
            ids = tokenizer.text_to_ids(tokenizer.ids_to_text(ids))                              # :146
            pseudo_targets = torch.LongTensor(ids).unsqueeze(0).repeat(num_negatives, 1)
            augmented_outs = log_p[:num_negatives]                                               # :147
            N, B = augmented_outs.shape[1], augmented_outs.shape[0]
            loss = ctc_loss_fn(augmented_outs.transpose(0, 1), pseudo_targets, torch.LongTensor([N] * B),
                               torch.LongTensor([pseudo_targets.shape[1]] * B)) / (N * B)        # :152
            optimizer.zero_grad()
            loss.backward()
            if adapt:
                optimizer.step()                                                                 # :160
            logits = torch.exp(log_p[-1].detach())                                               # :165-166
            ds_len = logits.shape[-2]
            overlap_ds = int(overlap / (u_len / ds_len))                                         # :168-169
            model_outputs[i] = {'logits': logits, 'ds_len': ds_len, 'overlap_ds': overlap_ds}
    for i in sorted(list(model_outputs.keys())):                                                 # :174-179
        logits, ds_len, overlap_ds = model_outputs[i]['logits'], model_outputs[i]['ds_len'], model_outputs[i]['overlap_ds']
        logit_position -= overlap_ds if i != 0 else 0
        logit_count[:, logit_position:logit_position + ds_len, :] += 1
        all_logits[:, logit_position:logit_position + ds_len, :] += logits
        logit_position += ds_len
    B, N, C = all_logits.shape                                                                   # :181-187
    all_logits = all_logits[logit_count.sum(dim=-1) != 0].reshape(B, -1, C)
    logit_count = logit_count[logit_count.sum(dim=-1) != 0].reshape(B, -1, C)
    logits = torch.log(all_logits / logit_count)
    with torch.no_grad():
        for p, p_orig in zip(model.parameters(), original):                                      # :189-191
            p.copy_(p_orig)
    for p, rg in frozen:
        p.requires_grad = rg
    model.zero_grad()
    return logits.squeeze(0).numpy()


# seed / blank_bias: chosen on the CPU so that the oracle's smallest top-2 log-prob margin over all stitched frames is >= 1e-2 (in order and
# shuffled) and at least a quarter of the frames are non-blank; tests/test_lasr_cpu.py and tests/test_lasr_gpu.py assert both
LOOP = dict(seq_len=128, overlap=64, num_negatives=2, lr_args={'lr': 1e-5}, T=300, seed=7, spec_seed=21, mask_seed=5, blank_bias=0.0)
LOOP_ROWS = 29 + 15 + 15 + 10          # windows of 128, 128, 128, 108 frames -> 29, 29, 29, 24 encoder frames, overlap_ds = int(64 / (128 / 29)) = int(64 / (108 / 24)) = 14


def loop_inputs():
    """The loop tests' feature matrix [1, 128, 300] (seeded) and tokenizer."""
    spec = torch.randn(1, TOY["num_mel_bins"], LOOP["T"], generator=torch.Generator().manual_seed(LOOP["spec_seed"]))
    return spec, Tokenizer(VOCAB - 1)
