"""References for the ragged-batch tests: torch restatements (any dtype, CPU) of the per-row kernel semantics, built on tests/parakeet_refs.py's
references with a `lens` list (one frame count per batch entry, clamped as the kernels clamp), the tolerance recipe of the kernel tests
(cohere_asr_refs.step_tol), and the transformers runs the model tests compare against: the masked batch, and every row alone at its length."""
import copy

import torch
import torch.nn.functional as F

import kernel_refs as K
import lasr_refs as LR
import parakeet_refs as R

T_FEAT, N_MELS = 131, 80
LENS = ((131, 67, 100), (131, 8, 9), (130, 17, 1))          # the model tests' batches [3, 131, 80]


def tol(want32, want64):
    """4 x the error of the same function in fp32 on the CPU against float64 + 2e-5 * max(1, max |want|) -> (tolerance, the fp32 error)."""
    e32 = (want32.double() - want64).abs().max().item()
    return 4.0 * e32 + 2e-5 * max(1.0, want64.abs().max().item()), e32


def clamp(lens, T, lo=0):
    return [max(lo, min(int(n), T)) for n in lens]


def out_len(n):
    return (n - 1) // 2 + 1


# ----------------------------------------------------------------------------------------------------------- conv module, per row
def convmod_bn_ref(u, w, cbias, mean, var, weight, bias, eps, lens):
    """(s, gl, c) of dyn_convmod_bn_fwd_lens: the scalar reference row by row with valid = lens[b] (lasr_refs': parakeet_refs' with torch's
    "same" padding, so right at 32 taps too: 15 frames left, 16 right)."""
    rows = [LR.convmod_bn_ref(u[b:b + 1], w, cbias, mean, var, weight, bias, eps, n) for b, n in enumerate(clamp(lens, u.shape[1]))]
    return tuple(torch.cat([r[i] for r in rows]) for i in range(3))


def convmod_bn_bwd_act_ref(c, mean, var, weight, bias, ds, eps, lens):
    """(dc, dweight, dbias, dcbias) of dyn_convmod_bn_bwd_act_lens: rows past lens[b] give dc = 0 and no term of the three sums."""
    rows = [LR.convmod_bn_bwd_act_ref(c[b:b + 1], mean, var, weight, bias, ds[b:b + 1], eps, n) for b, n in enumerate(clamp(lens, c.shape[1]))]
    return (torch.cat([r[0] for r in rows]),) + tuple(sum(r[i] for r in rows) for i in (1, 2, 3))


def glu_dwconv1d_dgrad_ref(u, w, dc, lens):
    return torch.cat([LR.glu_dwconv1d_dgrad_ref(u[b:b + 1], w, dc[b:b + 1], n) for b, n in enumerate(clamp(lens, u.shape[1]))])


# ----------------------------------------------------------------------------------------------------------- relative-position softmax
def softmax_relshift_ref(S, BD, lens):
    """softmax over the first lens[b] (clamped into [1, T]) keys of S + shift(BD), probability 0 past them; S [B, nh, T, T]."""
    x = K.relshift_scores_ref(S, BD)
    T = S.shape[-1]
    keep = torch.arange(T)[None, :] < torch.tensor(clamp(lens, T, 1))[:, None]                   # [B, T]
    p = torch.softmax(x.masked_fill(~keep[:, None, None, :], float("-inf")), -1)
    return p * keep[:, None, None, :]


# ----------------------------------------------------------------------------------------------------------- subsampling stages
def _row_mask(lens, T, like):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(like.dtype)               # [B, T]


def conv2d_first_ref(x, w, bias, lens, dz=None):
    """z [B, To, Fo, C] of dyn_conv2d_first_fwd_lens (frames t >= lens[b] of x read as zeros); with dz also (dw [C, 3, 3], dbias [C])."""
    B, T, _ = x.shape
    wr, br = w.clone().requires_grad_(), bias.clone().requires_grad_()
    xm = x * _row_mask(clamp(lens, T), T, x)[:, :, None]
    z = F.conv2d(xm[:, None], wr[:, None], br, stride=2, padding=1).permute(0, 2, 3, 1)
    if dz is None:
        return z.detach().contiguous()
    z.backward(dz)
    return z.detach().contiguous(), wr.grad, br.grad


def relu_dwconv2d_s2_ref(z, w, bias, lens_in, lens_out, du=None):
    """u of dyn_dwconv2d_s2_fwd_act_lens (ReLU): rows t >= lens_in[b] of z read as zeros, rows to >= lens_out[b] of u zeros; with du also
    (dz, dw, dbias) by autograd through both masks (du's rows past lens_out so carry no gradient: "wgrad via zeroed du")."""
    B, T, _, C = z.shape
    To = out_len(T)
    zr, wr, br = z.clone().requires_grad_(), w.clone().requires_grad_(), bias.clone().requires_grad_()
    zm = F.relu(zr) * _row_mask(clamp(lens_in, T), T, z)[:, :, None, None]
    u = F.conv2d(zm.permute(0, 3, 1, 2), wr[:, None], br, stride=2, padding=1, groups=C).permute(0, 2, 3, 1)
    u = u * _row_mask(clamp(lens_out, To), To, z)[:, :, None, None]
    if du is None:
        return u.detach().contiguous()
    u.backward(du)
    return u.detach().contiguous(), zr.grad, wr.grad, br.grad


# ----------------------------------------------------------------------------------------------------------- the transformers runs
def features(seed=1, B=3, T=T_FEAT):
    return torch.randn(B, T, N_MELS, generator=torch.Generator().manual_seed(seed))


def prefix_mask(lens, T):
    return torch.arange(T)[None, :] < torch.tensor(list(lens))[:, None]


def zero_padded(x, lens):
    return x * prefix_mask(lens, x.shape[1])[:, :, None].to(x.dtype)


def junk_padded(x, lens, value=37.5):
    """x with every frame past a row's length overwritten by large, varying junk."""
    keep = prefix_mask(lens, x.shape[1])[:, :, None]
    junk = value * (1.0 + torch.arange(x.numel(), dtype=x.dtype).reshape(x.shape) % 7)
    return torch.where(keep, x, junk)


def double(ref):
    return copy.deepcopy(ref).double()


def hf_masked(ref, x, lens):
    """transformers on the zero-padded ragged batch with its attention_mask (the default sdpa path): logits [B, T', V]."""
    return ref(input_features=zero_padded(x, lens).to(next(ref.parameters()).dtype), attention_mask=prefix_mask(lens, x.shape[1])).logits


def hf_unmasked(ref, x, lens):
    return ref(input_features=zero_padded(x, lens).to(next(ref.parameters()).dtype)).logits


def hf_solo(ref, x, lens):
    """Every row alone at its own length: a list of logits [1, T'_b, V]."""
    dt = next(ref.parameters()).dtype
    return [ref(input_features=x[b:b + 1, :n].to(dt)).logits for b, n in enumerate(lens)]


def valid_err(got, solo):
    """max |got[b, :T'_b] - solo[b]| over the rows."""
    return max((got[b, :s.shape[1]].double().cpu() - s[0].double()).abs().max().item() for b, s in enumerate(solo))


def enc_lens(lens):
    """Valid encoder frames per row: three stride-2 stages."""
    return [out_len(out_len(out_len(int(n)))) for n in lens]


def valid_cat(t, lens3):
    """The valid frames of every row of t [B, T', ...], concatenated: what a tolerance or an error is taken over."""
    return torch.cat([t[b, :n] for b, n in enumerate(lens3)])


def model_tol(ref, ref64, x, lens):
    """The recipe on the masked batch's valid logits: (tolerance, fp32 error, the float64 logits [B, T', V])."""
    with torch.no_grad():
        w32, w64 = hf_masked(ref, x, lens), hf_masked(ref64, x, lens)
    l3 = enc_lens(lens)
    return tol(valid_cat(w32, l3), valid_cat(w64, l3)) + (w64,)


# ----------------------------------------------------------------------------------------------------------- CohereAsr
def cohere_kv(ref, x, lens, masked=True, labels=None):
    """transformers' CohereAsr encoder on the zero-padded batch (with its attention_mask when `masked`) -> what the decoder's cross-attention
    reads: `decoder.proj` of the encoder states, then every layer's k_proj | v_proj, side by side [B, T', layers * 2d], in the model's dtype.
    The decoder's logits hardly depend on the audio with random weights, so THIS is where a forgotten encoder mask shows."""
    import cohere_asr_refs as CR
    dt = next(ref.parameters()).dtype
    ids = torch.full((x.shape[0], 1), ref.config.decoder_start_token_id)
    kw = dict(attention_mask=prefix_mask(lens, x.shape[1])) if masked else {}
    enc = ref(input_features=zero_padded(x, lens).to(dt), decoder_input_ids=ids, **kw).encoder_last_hidden_state
    return torch.cat(CR.cross_kv_of(CR.decoder_of(ref.state_dict()), enc, ref.config.num_hidden_layers, dt), -1)


def cohere_kv_solo(ref, x, lens):
    return [cohere_kv(ref, x[b:b + 1, :n], [n], masked=False) for b, n in enumerate(lens)]
