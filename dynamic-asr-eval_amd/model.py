"""SCConformerXL on MI355X: the acoustic model the reference drives through
`model(audio_signal=...)['final_posteriors']` (reference lcasr/lib.py:550,559,603), with an explicit
forward / backward built ONLY from the HIP kernels of libdyneval_hip.so (no torch arithmetic, no autograd).

Duck-type surface kept from the reference: callable with kw `audio_signal` ([B, 80, T] log-mel),
returns {'final_posteriors': [B, T/8, V+1] log-probs, blank = last class}; `.device`, `.decoder.num_classes`,
`.parameters()`, `.eval()/.train()`, `.subsampling`, `.layers`, `.decoder`, `.print_total_params()`,
`.load_state_dict(strict=False)`.  Activations are saved for the backward exactly when torch grad mode is on,
so `with torch.no_grad(): model(...)` (reference lib.py:603) behaves as in the reference.

HBM layout (MI355X-first): all parameters live in ONE flat fp32 buffer (256-B aligned slots), all gradients in a
second, so the adaptation step is a single fused launch over ~90 M elements and snapshot/restore of the weights is
one device-to-device copy (the reference round-trips them through host memory, lib.py:482-483,636-637).
Activations are channels-last ([B, T, C]) so pointwise convs and linears are plain row-major GEMMs and every
elementwise kernel is coalesced along C.  Architecture: see oracle/conformer_ref.py (same definition, shared names).
Attention is the fused kernel (csrc/attention.hip) where it applies, else materialised scores: the products of _attn.py around ops.softmax.
"""
import math
from types import SimpleNamespace

import torch

from . import _attn, _graphs, ops
from ._flat import FlatModel

DEFAULT_CONFIG = dict(
    feat_in=80, n_layers=6, d_model=768, n_heads=6, head_dim=128, ff_mult=4, subsampling_factor=8,
    subsampling_conv_channels=256, conv_kernel_size=9, conv_norm="rms_norm", rotary_base_freq=1500000.0,
    self_conditioning=True, norm_eps=1e-5,
)


# Keys of the reference yaml (earnings_finetune/lcasr160rb1.yaml:1-29) that select an architecture VARIANT upstream.  This
# implementation builds exactly one variant; a checkpoint config asking for another must not be run silently as this one.
SUPPORTED_VARIANT = dict(
    bias_in_ff=False, qk_rms_norm=False, sandwich_norm=False, default_norm="layer_norm", use_rotary=True, encoder_mode="conformer",
    decoder_norm=True, gated_sc=False, self_condition_subsampling=False, subsampling_norm_out=False, shift_kvs=False,
    subsampling="dw_striding", subsampling_act="silu",
)
# yaml keys that do not change the arithmetic of the eval path (dropout is off in eval mode; flash attention is an implementation choice)
IGNORED_KEYS = {"dropout_ff", "dropout_conv", "dropout_attn", "flash_attn", "checkpoint_every_n_layers"}


def make_config(**over):
    cfg = dict(DEFAULT_CONFIG)
    for k, v in over.items():
        if k in DEFAULT_CONFIG:
            cfg[k] = v
        elif k in SUPPORTED_VARIANT:
            if v != SUPPORTED_VARIANT[k]:
                raise ValueError(f"model config {k}={v!r}: this implementation supports only {k}={SUPPORTED_VARIANT[k]!r}")
        elif k not in IGNORED_KEYS:
            raise ValueError(f"unknown model config key {k!r} (known: {sorted(DEFAULT_CONFIG) + sorted(SUPPORTED_VARIANT)})")
    return cfg


def param_spec(cfg, num_classes):
    """[(name, shape)] in the oracle's named_parameters() order."""
    d, C, K = cfg["d_model"], cfg["subsampling_conv_channels"], cfg["conv_kernel_size"]
    HD, ff = cfg["n_heads"] * cfg["head_dim"], cfg["d_model"] * cfg["ff_mult"]
    fo = cfg["feat_in"]
    for _ in range(3):
        fo = ops.out_len(fo)
    spec = [("subsampling.conv1.weight", (C, 3, 3)), ("subsampling.conv1.bias", (C,))]
    for i in (2, 3):
        spec += [(f"subsampling.dw{i}.weight", (C, 3, 3)), (f"subsampling.dw{i}.bias", (C,)),
                 (f"subsampling.pw{i}.weight", (C, C)), (f"subsampling.pw{i}.bias", (C,))]
    spec += [("subsampling.out.weight", (d, fo * C)), ("subsampling.out.bias", (d,))]
    for l in range(cfg["n_layers"]):
        p = f"layers.{l}."
        for ffn in ("ff1",):
            spec += [(p + ffn + ".norm.weight", (d,)), (p + ffn + ".norm.bias", (d,)),
                     (p + ffn + ".w1.weight", (ff, d)), (p + ffn + ".w2.weight", (d, ff))]
        spec += [(p + "attn.norm.weight", (d,)), (p + "attn.norm.bias", (d,)), (p + "attn.qkv.weight", (3 * HD, d)),
                 (p + "attn.qkv.bias", (3 * HD,)), (p + "attn.out.weight", (d, HD)), (p + "attn.out.bias", (d,))]
        spec += [(p + "conv.norm.weight", (d,)), (p + "conv.norm.bias", (d,)), (p + "conv.pw1.weight", (2 * d, d)),
                 (p + "conv.pw1.bias", (2 * d,)), (p + "conv.dw.weight", (d, K)), (p + "conv.dw.bias", (d,)),
                 (p + "conv.cnorm.weight", (d,))]
        if cfg["conv_norm"] != "rms_norm":
            spec += [(p + "conv.cnorm.bias", (d,))]
        spec += [(p + "conv.pw2.weight", (d, d)), (p + "conv.pw2.bias", (d,))]
        spec += [(p + "ff2.norm.weight", (d,)), (p + "ff2.norm.bias", (d,)), (p + "ff2.w1.weight", (ff, d)),
                 (p + "ff2.w2.weight", (d, ff))]
        spec += [(p + "norm_out.weight", (d,)), (p + "norm_out.bias", (d,))]
    spec += [("decoder.norm.weight", (d,)), ("decoder.norm.bias", (d,)), ("decoder.ff.weight", (num_classes, d)),
             ("decoder.ff.bias", (num_classes,))]
    if cfg["self_conditioning"]:
        spec += [("decoder.reproj.weight", (d, num_classes)), ("decoder.reproj.bias", (d,))]
    return spec


def _parse_fused_attn_grad(value):
    """DYN_FUSED_ATTN_GRAD / `model.fused_attention_grad`: 0 = never, 1 = always, n > 1 = from T' >= n frames.  Validated where
    it is set, so a typo fails at construction instead of in the middle of a forward."""
    try:
        mode = int(str(value).strip())
    except ValueError:
        raise ValueError(f"DYN_FUSED_ATTN_GRAD / fused_attention_grad must be 0, 1 or a frame threshold, got {value!r}") from None
    if mode < 0:
        raise ValueError(f"DYN_FUSED_ATTN_GRAD / fused_attention_grad must be >= 0, got {value!r}")
    return mode


class _Group:
    """A named slice of the parameter list (`model.subsampling`, `model.layers[i]`, `model.decoder`): what the
    reference's freeze helpers iterate (reference lcasr/lib.py:163-204)."""

    def __init__(self, model, prefix, **attrs):
        self._model, self._prefix = model, prefix
        self.__dict__.update(attrs)

    def parameters(self):
        return [p for n, p in self._model.named_parameters() if n.startswith(self._prefix)]


class SCConformerXL(FlatModel):
    _input = "audio_signal"

    def __init__(self, config=None, vocab_size=128, device="cuda:0", extra_spec=None, group=1):
        """`extra_spec`: [(name, shape)] of further parameters placed in the SAME flat buffers (the enc-dec model appends its
        decoder there, so snapshot / restore / optimiser step stay single operations).
        `group` = R > 1: a LOCKSTEP GROUP of R model replicas in one object: parameters, gradients and optimiser state are
        [R, n_flat] buffers, a batch holds `chunks * R` samples ordered sample = chunk * R + replica, and every launch covers all R
        recordings — each linear layer one product batched over the replicas' weights, every parameter-free row-wise kernel one launch over
        all samples, LayerNorm / RMSNorm one launch with a per-sample parameter offset; the few kernels without a group form (fused conv
        module, depthwise convolutions, fused subsampling) run once per sample.  Per replica the arithmetic is that of a single model
        (tests/test_model_gpu.py::test_lockstep_group_matches_separate_models)."""
        self.config = make_config(**(config or {}))
        if int(group) < 1:
            raise ValueError("group must be >= 1")
        self._lo, self._n = 0, int(group)   # replicas [lo, lo + n) take part in the current batches (see `active` / set_range)
        cfg = self.config
        if cfg["conv_norm"] not in ("rms_norm", "layer_norm", "batch_renorm"):
            raise ValueError(f"unknown conv_norm {cfg['conv_norm']}")
        if cfg["d_model"] % 256:
            raise ValueError("d_model must be a multiple of 256 (wave-per-row norm kernels)")
        self.num_classes = vocab_size + 1
        super().__init__(param_spec(cfg, self.num_classes) + list(extra_spec or []), device, replicas=group)
        self.buffers = {}
        if cfg["conv_norm"] == "batch_renorm":
            for l in range(cfg["n_layers"]):
                self.buffers[f"layers.{l}.conv.cnorm.running_mean"] = torch.zeros(cfg["d_model"], device=self.device)
                self.buffers[f"layers.{l}.conv.cnorm.running_var"] = torch.ones(cfg["d_model"], device=self.device)
        self.subsampling = _Group(self, "subsampling.")
        self.layers = [_Group(self, f"layers.{l}.") for l in range(cfg["n_layers"])]
        self.decoder = _Group(self, "decoder.", num_classes=self.num_classes)
        self._rot = {}
        self.fused_attention = True   # no-grad passes use dyn_attention_fwd when the launch fills the chip (see _attn_fwd)
        self._ctx = None
        self._skip_wgrad = False
        self.use_graphs = False     # hipGraph replay of the forward / backward launch sequences (see forward())
        self._graphs = {"fwd": {}, "bwd": {}, "pool": {}}
        self._seen = _graphs.Seen()
        self._ctx_static = False
        self._ctx_key = None
        self.fused_convmod = True   # GLU + dwconv + norm + SiLU in one kernel (csrc/convmod.hip)
        import os
        # first two subsampling stages fused (csrc/conv.hip sub12_*): z1 = conv2d_first(x), the largest activation of the model, is
        # recomputed from x in forward and backward instead of making four trips through HBM (DYN_FUSED_SUB=0: the separate kernels)
        self.fused_subsampling = os.environ.get("DYN_FUSED_SUB", "1") != "0" and cfg["subsampling_conv_channels"] % 4 == 0
        # A/B switch (measurements only): SiLU / SiLU' in the epilogue of the producing GEMM: OFF
        # by default (A/B on one box, 3 chains: 739 vs 738 audio-s/s, while the GEMM's own rate drops 110 -> 101 TFLOP/s: the
        # activation runs with the MFMA pipe idle, whereas the separate HBM-bound kernels hide under the other chains' GEMMs)
        self.fused_silu = os.environ.get("DYN_FUSED_SILU", "0") != "0"
        # the shared CTC head / re-projection weight gradients (one product per block) through the grouped launch (DYN_STACK_SHARED_WGRAD=0: one launch per use)
        self.stack_shared_wgrads = os.environ.get("DYN_STACK_SHARED_WGRAD", "1") != "0"
        self._shared = {}           # (weight name, replica) -> slabs of a weight used once per block (see _shared_slab)
        # Number of LEADING samples of a grad-mode batch whose activations the backward will need (None = all).  The dynamic-eval loss
        # uses only the augmented copies (reference lcasr/lib.py:570-575; backward(n_active=...) below), so the clean copy's attention
        # can take the fused no-grad kernel: its probabilities are never read again.  Set by lib.dynamic_eval around its loop.
        self.grad_samples = None
        # grad-mode attention without the [B, H, T', T'] score matrix (forward keeps one log-sum-exp per row, the backward re-forms P
        # tile by tile: 7 products instead of 4): "0" never, "1" always, otherwise from T' >= this many frames
        self.fused_attention_grad = _parse_fused_attn_grad(os.environ.get("DYN_FUSED_ATTN_GRAD", "4096"))

    # ------------------------------------------------------------------ lockstep group helpers
    @property
    def active(self):
        """Number of replicas taking part in the current batches (a batch holds chunks * active samples)."""
        return self._n

    @active.setter
    def active(self, n):
        self.set_range(0, n)

    def set_range(self, lo, hi):
        """Batches from now on belong to replicas lo .. hi-1 (sample s -> replica lo + s % (hi - lo)): a group whose recordings have
        different lengths runs its full windows on a shrinking prefix and every short last window on the replica that owns it."""
        if not (0 <= lo < hi <= self.R):
            raise ops.DynError(f"replica range [{lo}, {hi}) outside the group of {self.R}")
        self._lo, self._n = int(lo), int(hi - lo)

    def _w(self, name):
        """The parameter as the kernels take it: the tensor itself, or (R > 1) the group view with its replica stride."""
        return self.P[name] if self.R == 1 else ops.GroupParam(self.PR[name][self._lo:self._lo + self._n], self._n, self.n_flat)

    def _gw(self, name):
        return self.G[name] if self.R == 1 else ops.GroupParam(self.GR[name][self._lo:self._lo + self._n], self._n, self.n_flat)

    def replica_params(self, r):
        """Views of replica r's parameters, in named_parameters() order."""
        return [self.PR[n][r] for n, _ in self.spec]

    def replica_flat(self, r):
        return self.flat_params.view(self.R, self.n_flat)[r]

    # ------------------------------------------------------------------ nn.Module-like surface
    def _flat_range(self):
        return self._lo * self.n_flat, (self._lo + self._n) * self.n_flat      # a lockstep group steps its active replicas' buffers in one launch

    def state_dict(self):
        sd = {n: p.detach().clone() for n, p in self.named_parameters()}
        sd.update({n: b.detach().clone() for n, b in self.buffers.items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        missing = [n for n, _ in self.spec if n not in sd] + [n for n in self.buffers if n not in sd]
        unexpected = [n for n in sd if n not in self.P and n not in self.buffers]
        if strict and (missing or unexpected):
            raise KeyError(f"missing {missing[:5]}… unexpected {unexpected[:5]}…")
        for n, _ in self.spec:
            if n in sd:
                src = sd[n].to(self.device, torch.float32).reshape(self.P[n].shape)
                for r in range(self.R):          # every replica of a lockstep group starts from the same weights
                    self.PR[n][r].copy_(src)
        for n in self.buffers:
            if n in sd:
                self.buffers[n].copy_(sd[n].to(self.device, torch.float32))
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def print_total_params(self):
        print(f"Total params: {sum(math.prod(s) for _, s in self.spec) / 1e6:.2f}M")

    # ------------------------------------------------------------------ helpers
    def _rotary(self, T):
        if T not in self._rot:
            D = self.config["head_dim"]
            inv = 1.0 / (float(self.config["rotary_base_freq"]) ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
            ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
            self._rot[T] = (ang.cos().float().to(self.device).contiguous(), ang.sin().float().to(self.device).contiguous())
        return self._rot[T]

    def _lin_bwd(self, dy, x, wname, bname=None, need_dx=True, alpha=1.0, silu_of=None):
        """Accumulates dW (and db) for y = x @ W^T + b and returns alpha * dy @ W (or None); with `silu_of` = u the returned
        gradient is multiplied by silu'(u) (the activation that produced x) in the GEMM's epilogue.
        While a deferred-wgrad queue is open (`_backward`), the weight gradient of a block-local weight is only QUEUED: dy and x
        must then stay unmodified until the queue is flushed (the residual-stream gradient gets a new buffer per module)."""
        wg = self.trainable(wname) and not self._skip_wgrad
        bg = bname is not None and self.trainable(bname) and not self._skip_wgrad   # bitfit trains a bias under a frozen weight
        if self.R > 1:
            return self._lin_bwd_group(dy, x, wname, bname, wg, bg, need_dx, alpha, silu_of)
        if wg and self._wq is not None and (wname.startswith("layers.") or wname == "subsampling.out.weight") \
                and ops.wgrad_groupable(dy, x, self.G[wname]):
            self._wq.append(ops.wgrad_desc(dy, x, self.G[wname], alpha=alpha, beta=1.0, colsum=self.G[bname] if bg else None, colsum_beta=1.0))
            bg = False
        elif wg and self._wq is not None and self.stack_shared_wgrads and wname in ("decoder.ff.weight", "decoder.reproj.weight") \
                and alpha == 1.0 and ops.wgrad_groupable(dy, x, self.G[wname]):
            self._wq.append(self._shared_slab(dy, x, wname, 0, self.G[wname], self.G[bname] if bg else None))
            bg = False
        elif wg:
            ops.linear_wgrad(dy, x, self.G[wname], alpha=alpha, beta=1.0)
        if bg:
            ops.colsum(dy, self.G[bname], beta=1.0)
        if not need_dx:
            return None
        if silu_of is not None and self.fused_silu:
            return ops.linear_dgrad(dy, self.P[wname], alpha=alpha, epilogue=ops.EPI_SILU_GRAD, aux=silu_of)
        dx = ops.linear_dgrad(dy, self.P[wname], alpha=alpha)
        return ops.silu_bwd(silu_of, dx, out=dx) if silu_of is not None else dx

    def _shared_slab(self, dy, x, wname, r, gw, gb):
        """Descriptor of dy^T x (+ column sums of dy with a bias gradient `gb`) for a weight used once per block (CTC head / re-projection of the
        self-conditioning): every use of (weight, replica r) writes its OWN slab in the grouped launch (outputs of one launch must not alias), and
        `_flush_shared` sums the slabs into the gradient views `gw` / `gb` after it, in use order — instead of one small launch with a
        read-modify-write of the whole gradient per use."""
        sh = self._shared.get((wname, r))
        if sh is None:
            cap = self.config["n_layers"] + 1
            sh = self._shared[(wname, r)] = {"w": torch.empty(cap, *gw.shape, device=self.device, dtype=torch.float32), "gw": gw, "gb": gb, "k": 0,
                                             "b": torch.empty(cap, gb.numel(), device=self.device, dtype=torch.float32) if gb is not None else None}
        k = sh["k"]
        sh["k"] = k + 1
        return ops.wgrad_desc(dy, x, sh["w"][k], alpha=1.0, beta=0.0, colsum=sh["b"][k] if sh["b"] is not None else None, colsum_beta=0.0)

    def _flush_shared(self):
        for sh in self._shared.values():
            ops.reduce_partials(sh["w"][:sh["k"]], sh["gw"], beta=1.0)
            if sh["b"] is not None:
                ops.reduce_partials(sh["b"][:sh["k"]], sh["gb"], beta=1.0)
        self._shared = {}

    def _lin_bwd_group(self, dy, x, wname, bname, wg, bg, need_dx, alpha, silu_of):
        """_lin_bwd over a lockstep group (the backward batch holds ONE chunk: sample r = replica r): every replica's weight gradient is its
        own descriptor of the grouped launch (its rows of dy and x are contiguous), the input gradient one product batched over the weights."""
        R = self.active
        if dy.shape[0] != R:
            raise ops.DynError(f"lockstep group: the backward runs on one sample per replica (got a batch of {dy.shape[0]} for {R} replicas)")
        lo = self._lo
        GR = {wname: self.GR[wname][lo:lo + R]}
        if bname is not None:
            GR[bname] = self.GR[bname][lo:lo + R]
        shared = wname in ("decoder.ff.weight", "decoder.reproj.weight") and self.stack_shared_wgrads and alpha == 1.0
        block_local = wname.startswith("layers.") or wname == "subsampling.out.weight"      # the deep-K subsampling products stay immediate (split-K)
        if wg and self._wq is not None and (block_local or shared) and ops.wgrad_groupable(dy[0], x[0], GR[wname][0]):
            for r in range(R):
                if shared:
                    self._wq.append(self._shared_slab(dy[r], x[r], wname, r, GR[wname][r], GR[bname][r] if bg else None))
                else:
                    self._wq.append(ops.wgrad_desc(dy[r], x[r], GR[wname][r], alpha=alpha, beta=1.0, colsum=GR[bname][r] if bg else None, colsum_beta=1.0))
            bg = False
        elif wg:
            for r in range(R):
                ops.linear_wgrad(dy[r], x[r], GR[wname][r], alpha=alpha, beta=1.0)
        if bg:
            for r in range(R):
                ops.colsum(dy[r], GR[bname][r], beta=1.0)
        if not need_dx:
            return None
        dx = ops.linear_dgrad(dy, self._w(wname), alpha=alpha)
        return ops.silu_bwd(silu_of, dx, out=dx) if silu_of is not None else dx

    def _check_not_queued(self, t, what):
        """An in-place update of `t` while a queued weight-gradient descriptor still reads it would corrupt that gradient (the
        descriptors hold raw pointers until the flush at the end of the backward): refuse instead of computing garbage."""
        if self._wq:
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * 4
            for d in self._wq:
                for src in d._keep[:2]:
                    if src is not None and src.data_ptr() < hi and lo < src.data_ptr() + src.numel() * 4:
                        raise ops.DynError(f"backward: in-place update of {what} while a deferred weight gradient still reads it")

    def _res_norm_bwd(self, h, wn, bn_, mean, rstd, dn, dh):
        """dh_out = dh + LayerNorm_bwd(dn): in place, or into a NEW buffer while weight gradients that read dh are still queued."""
        if self._wq is None:
            ops.layernorm_bwd(h, self._w(wn), mean, rstd, dn, dh, self._gw(wn), self._gw(bn_), dx_beta=1.0)
            return dh
        out = torch.empty_like(dh)
        ops.layernorm_bwd(h, self._w(wn), mean, rstd, dn, out, self._gw(wn), self._gw(bn_), dx_beta=1.0, dx_in=dh)
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, audio_signal):
        with ops.use_workspace(self._scratch()):
            return self._forward(audio_signal)

    def _graph_pool(self):
        """One private memory pool per replica range.  Graphs that share a pool may hand each other's freed capture-time memory around, which is
        only safe when they replay in capture order.  A lockstep group whose recordings have different lengths runs SEVERAL shape classes per window
        step as forward(class 1), forward(class 2), backward(class 1), backward(class 2): with one pool, a backward graph of class 1 captured in an
        earlier call can own, as a temporary, the very memory a forward graph of class 2 captured later keeps its saved activations in (seen: two
        epochs after one-epoch runs, 0.4 off on the shortest recording).  Classes of one step have disjoint replica ranges, so a pool per range keeps
        their graphs apart; within a range forward and backward alternate strictly."""
        pools = self._graphs["pool"]
        key = (self._lo, self._n)
        if key not in pools:
            pools[key] = torch.cuda.graph_pool_handle()
        return pools[key]

    def _forward(self, audio_signal):
        """Eager launch sequence, or — with `use_graphs` — a hipGraph replay of it.  A (shape, grad-mode) pair is captured
        the second time it is seen (one-off shapes such as the short last window stay eager); the captured graph owns its
        activations (static addresses), so the matching backward graph can be captured once and replayed too.  One window
        step is ~1300 launches: replaying them removes ~25 ms of Python/ctypes launch work per window from the host and
        the host-bound gaps between the short HBM-bound kernels."""
        x = audio_signal
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            raise ops.DynError("audio_signal must be a float32 CUDA tensor [B, feat_in, T]")
        if not self.use_graphs or ops.GEMM_PROFILE_EAGER():
            self._ctx_static = False
            return self._forward_eager(x)
        G = self._graphs
        key = (tuple(x.shape), torch.is_grad_enabled(), self.fused_convmod, self.fused_attention, self.fused_silu, str(self.fused_attention_grad),
               self.fused_subsampling, self.grad_samples, self._lo, self._n)
        ent = G["fwd"].get(key)
        if ent is None:
            if not self._seen(key, 2):
                self._ctx_static = False
                return self._forward_eager(x)
            pool = self._graph_pool()
            static_in = x.clone()
            graph, out = _graphs.capture(pool, lambda: self._forward_eager(static_in))
            ent = {"graph": graph, "in": static_in, "out": out, "ctx": self._ctx}
            G["fwd"][key] = ent
        ent["in"].copy_(x)
        ent["graph"].replay()
        self._ctx = ent["ctx"]
        self._ctx_static = True
        self._ctx_key = key
        return ent["out"]

    def _forward_eager(self, x):
        cfg, P, W, R = self.config, self.P, self._w, (self.active if self.R > 1 else 1)
        if self.R > 1 and (x.shape[0] % R or not self.fused_subsampling or not self.fused_convmod or self.fused_silu or cfg["conv_norm"] == "batch_renorm"):
            raise ops.DynError(f"lockstep group of {R}: the batch ({x.shape[0]}) must hold whole chunks of R samples, with the fused subsampling / "
                               "conv-module kernels, separate SiLU kernels and an rms_norm / layer_norm conv module")
        save = torch.is_grad_enabled()
        ctx = {} if save else None
        B, Fq, T = x.shape
        assert Fq == cfg["feat_in"], (Fq, cfg["feat_in"])
        C = cfg["subsampling_conv_channels"]
        xt = torch.empty(B, T, Fq, device=x.device, dtype=torch.float32)
        for b in range(B):
            ops.transpose_ft(x[b], out=xt[b])
        # --- dw_striding x8 subsampling
        grp = self.R > 1
        if self.fused_subsampling and grp:        # no group form: one launch per sample, replica k % R's filters
            z1 = None
            u2 = torch.empty(B, ops.out_len(ops.out_len(T)), ops.out_len(ops.out_len(Fq)), C, device=x.device, dtype=torch.float32)
            PR = self.PR
            for k in range(B):
                r = self._lo + k % R
                ops.sub12_fwd(xt[k:k + 1], PR["subsampling.conv1.weight"][r], PR["subsampling.conv1.bias"][r], PR["subsampling.dw2.weight"][r],
                              PR["subsampling.dw2.bias"][r], out=u2[k:k + 1])
        elif self.fused_subsampling:
            z1 = None
            u2 = ops.sub12_fwd(xt, P["subsampling.conv1.weight"], P["subsampling.conv1.bias"], P["subsampling.dw2.weight"], P["subsampling.dw2.bias"])
        else:
            z1 = ops.conv2d_first(xt, P["subsampling.conv1.weight"], P["subsampling.conv1.bias"])
            u2 = ops.dwconv2d_s2(z1, P["subsampling.dw2.weight"], P["subsampling.dw2.bias"])
        z2 = ops.linear(u2, W("subsampling.pw2.weight"), W("subsampling.pw2.bias"))
        if grp:
            u3 = torch.empty(B, ops.out_len(z2.shape[1]), ops.out_len(z2.shape[2]), C, device=x.device, dtype=torch.float32)
            for k in range(B):
                ops.dwconv2d_s2(z2[k:k + 1], self.PR["subsampling.dw3.weight"][self._lo + k % R], self.PR["subsampling.dw3.bias"][self._lo + k % R], out=u3[k:k + 1])
        else:
            u3 = ops.dwconv2d_s2(z2, P["subsampling.dw3.weight"], P["subsampling.dw3.bias"])
        if self.fused_silu:
            z3 = torch.empty(*u3.shape[:-1], C, device=x.device, dtype=torch.float32) if save else None
            a3 = ops.linear(u3, P["subsampling.pw3.weight"], P["subsampling.pw3.bias"], epilogue=ops.EPI_SILU, aux=z3)
        else:
            z3 = ops.linear(u3, W("subsampling.pw3.weight"), W("subsampling.pw3.bias"))
            a3 = ops.silu(z3)
        T3, F3 = a3.shape[1], a3.shape[2]
        if grp and save and R > 1 and (T3 * self.num_classes) % 4:
            raise ops.DynError(f"lockstep group: T' x (V + 1) = {T3} x {self.num_classes} must be a multiple of 4 (the backward takes per-replica "
                               "slices of the head's tensors with 16-byte vector accesses)")
        h = ops.linear(a3.view(B, T3, F3 * C), W("subsampling.out.weight"), W("subsampling.out.bias"))
        if save:
            ctx["sub"] = (xt, z1, u2, z2, u3, z3, a3)
            ctx["layers"] = []
            ctx["sc"] = []
        nl = cfg["n_layers"]
        for l in range(nl):
            lc = {} if save else None
            p = f"layers.{l}."
            h = self._ff_fwd(h, p + "ff1", lc, "ff1")
            h = self._attn_fwd(h, p + "attn", lc)
            h = self._conv_fwd(h, p + "conv", lc)
            h = self._ff_fwd(h, p + "ff2", lc, "ff2")
            hn, mean, rstd = ops.layernorm(h, W(p + "norm_out.weight"), W(p + "norm_out.bias"), cfg["norm_eps"])
            if save:
                lc["norm_out"] = (h, mean, rstd)
                ctx["layers"].append(lc)
            h = hn
            if cfg["self_conditioning"] and l != nl - 1:
                n, mean, rstd = ops.layernorm(h, W("decoder.norm.weight"), W("decoder.norm.bias"), cfg["norm_eps"])
                z = ops.linear(n, W("decoder.ff.weight"), W("decoder.ff.bias"))
                ops.softmax(z, out=z)
                if save:
                    h2 = ops.linear(z, W("decoder.reproj.weight"), W("decoder.reproj.bias"), beta=1.0, residual=h)
                else:
                    h2 = ops.linear(z, W("decoder.reproj.weight"), W("decoder.reproj.bias"), out=h, beta=1.0)
                if save:
                    ctx["sc"].append((h, mean, rstd, n, z))
                h = h2
        self._hidden = h      # encoder states before the CTC head (the enc-dec model's cross-attention reads them)
        n, mean, rstd = ops.layernorm(h, W("decoder.norm.weight"), W("decoder.norm.bias"), cfg["norm_eps"])
        z = ops.linear(n, W("decoder.ff.weight"), W("decoder.ff.bias"))
        logp = ops.log_softmax(z, out=z)
        if save:
            ctx["head"] = (h, mean, rstd, n, logp)
            ctx["dims"] = (B, T, T3, F3)
        self._ctx = ctx
        return {"final_posteriors": logp}

    def _ff_fwd(self, h, p, lc, key):
        P, W, eps = self.P, self._w, self.config["norm_eps"]
        n, mean, rstd = ops.layernorm(h, W(p + ".norm.weight"), W(p + ".norm.bias"), eps)
        if self.fused_silu:
            u = torch.empty(*n.shape[:-1], P[p + ".w1.weight"].shape[0], device=n.device, dtype=torch.float32) if lc is not None else None
            a = ops.linear(n, P[p + ".w1.weight"], epilogue=ops.EPI_SILU, aux=u)
        else:
            u = ops.linear(n, W(p + ".w1.weight"))
            a = ops.silu(u)
        if lc is not None:   # keep h for the backward: the GEMM reads the residual from h and writes a new buffer
            out = ops.linear(a, W(p + ".w2.weight"), alpha=0.5, beta=1.0, residual=h)
        else:
            out = ops.linear(a, W(p + ".w2.weight"), out=h, alpha=0.5, beta=1.0)
        if lc is not None:
            lc[key] = (h, mean, rstd, n, u, a)
        return out

    def _attn_fwd(self, h, p, lc):
        cfg, W = self.config, self._w
        H, D = cfg["n_heads"], cfg["head_dim"]
        HD = H * D
        B, T, _ = h.shape
        n, mean, rstd = ops.layernorm(h, W(p + ".norm.weight"), W(p + ".norm.bias"), cfg["norm_eps"])
        qkv = ops.linear(n, W(p + ".qkv.weight"), W(p + ".qkv.bias"))
        cos, sin = self._rotary(T)
        ops.rotary(qkv, cos, sin, B, T, 2 * H, D, 3 * HD)
        if lc is not None and D == 128 and self._fused_grad_attention(T):
            O, lse = ops.attention_fwd(qkv, B, T, H, D, 1.0 / math.sqrt(D), want_lse=True)
            out = ops.linear(O, W(p + ".out.weight"), W(p + ".out.bias"), beta=1.0, residual=h)
            lc["attn"] = (h, mean, rstd, n, qkv, lse, O)
            return out
        if lc is None and self.fused_attention and D == 128 and (B * H * ((T + 127) // 128) >= 320 or T >= 512):
            # no-grad pass: fused kernel, scores stay on chip.  Launches with too few (batch, head, query-block) workgroups to fill the
            # chip split the keys over several workgroups (dyn_attention_fwd_split: B = 1 at T' = 2048 130 us against 299 us unsplit)
            O = ops.attention_fwd(qkv, B, T, H, D, 1.0 / math.sqrt(D))
            return ops.linear(O, W(p + ".out.weight"), W(p + ".out.bias"), out=h, beta=1.0)
        # samples the backward will read the probabilities of: all, or (dynamic eval) only the leading augmented copies
        Bs = B
        if lc is not None and self.grad_samples is not None and self.fused_attention and D == 128 and T >= 512:
            Bs = max(0, min(B, int(self.grad_samples)))
        O = torch.empty(B, T, HD, device=h.device, dtype=torch.float32)
        S = torch.empty(Bs, H, T, T, device=h.device, dtype=torch.float32)
        if Bs > 0:
            _attn.scores(_attn.packed(qkv, 0, D), _attn.packed(qkv, 1, D), S, 1.0 / math.sqrt(D))     # the leading Bs samples: S's batch
            ops.softmax(S, out=S)
            _attn.context(S, _attn.packed(qkv, 2, D), _attn.plain(O, D))
        if Bs < B:      # the clean copies: scores stay on chip (key-split fused kernel), nothing kept for a backward
            ops.attention_fwd(qkv[Bs:], B - Bs, T, H, D, 1.0 / math.sqrt(D), out=O[Bs:])
        if lc is not None:
            out = ops.linear(O, W(p + ".out.weight"), W(p + ".out.bias"), beta=1.0, residual=h)
        else:
            out = ops.linear(O, W(p + ".out.weight"), W(p + ".out.bias"), out=h, beta=1.0)
        if lc is not None:
            lc["attn"] = (h, mean, rstd, n, qkv, S, O)
        return out

    def _fused_grad_attention(self, T):
        mode = _parse_fused_attn_grad(self.fused_attention_grad)     # tests and harnesses may assign the attribute directly
        return mode == 1 or (mode != 0 and T >= mode)

    def _cnorm_fwd(self, c, p):
        cfg, P = self.config, self.P
        kind = cfg["conv_norm"]
        if kind == "rms_norm":
            y, rstd = ops.rmsnorm(c, P[p + ".cnorm.weight"], cfg["norm_eps"])
            return y, (None, rstd)
        if kind == "layer_norm":
            y, mean, rstd = ops.layernorm(c, P[p + ".cnorm.weight"], P[p + ".cnorm.bias"], cfg["norm_eps"])
            return y, (mean, rstd)
        # batch_renorm, eval mode (the loop calls model.eval(), reference lib.py:525): running statistics are constants
        y = ops.chanaffine(c, self.buffers[p + ".cnorm.running_mean"], self.buffers[p + ".cnorm.running_var"],
                           P[p + ".cnorm.weight"], P[p + ".cnorm.bias"], cfg["norm_eps"])
        return y, (None, None)

    def _conv_fwd(self, h, p, lc):
        cfg, P, W = self.config, self.P, self._w
        n, mean, rstd = ops.layernorm(h, W(p + ".norm.weight"), W(p + ".norm.bias"), cfg["norm_eps"])
        u = ops.linear(n, W(p + ".pw1.weight"), W(p + ".pw1.bias"))
        if cfg["conv_kernel_size"] == 9 and cfg["d_model"] <= 1024 and self.fused_convmod and cfg["conv_norm"] != "batch_renorm":
            ln = cfg["conv_norm"] == "layer_norm"
            s, g, c, nn_, cmean, crstd = ops.convmod_fwd(u, W(p + ".dw.weight"), W(p + ".dw.bias"), W(p + ".cnorm.weight"),
                                                         W(p + ".cnorm.bias") if ln else None, ln, cfg["norm_eps"], lc is not None)
            stats = (cmean, crstd)
        elif self.R > 1:
            raise ops.DynError("lockstep group: the conv module needs the fused kernel (kernel size 9, d_model <= 1024)")
        else:
            g = ops.glu(u)
            c = ops.dwconv1d(g, P[p + ".dw.weight"], P[p + ".dw.bias"])
            nn_, stats = self._cnorm_fwd(c, p)
            s = ops.silu(nn_)
        if lc is not None:
            out = ops.linear(s, W(p + ".pw2.weight"), W(p + ".pw2.bias"), beta=1.0, residual=h)
        else:
            out = ops.linear(s, W(p + ".pw2.weight"), W(p + ".pw2.bias"), out=h, beta=1.0)
        if lc is not None:
            lc["conv"] = (h, mean, rstd, n, u, g, c, stats, nn_, s)
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, grad_posteriors, n_active=None, input_grad=False, param_grads=True, grad_hidden=None):
        """Gradient of a scalar loss w.r.t. every parameter, given dL/d(final_posteriors) [B, T', V+1].
        Accumulates into `flat_grads` (call zero_grad() first, as `optimizer.zero_grad()` at reference lib.py:578).
        `n_active` = nb: only the first nb samples of the batch carry a non-zero gradient (the dynamic-eval loss uses
        the augmented copies only, reference lib.py:570-575), so the backward runs on those samples; the skipped
        samples would contribute exact zeros to every gradient.
        `input_grad=True` also returns dL/d(audio_signal) [B, F, T]; `param_grads=False` skips every weight-gradient
        product (the entropy-gradient input perturbation, reference lib.py:96, needs only the input gradient).
        `grad_hidden` [nb, T', d]: an additional gradient w.r.t. the encoder states `_hidden` (enc-dec cross-attention)."""
        self._skip_wgrad = not param_grads
        self._grad_hidden = grad_hidden
        try:
            with ops.use_workspace(self._scratch()):
                if self._ctx_static and self.use_graphs and not input_grad and param_grads and self._ctx is not None and grad_hidden is None:
                    return self._backward_graphed(grad_posteriors, n_active)
                return self._backward(grad_posteriors, n_active, input_grad)
        finally:
            self._skip_wgrad = False
            self._shared = {}
            self._grad_hidden = None

    def _backward_graphed(self, grad_posteriors, n_active):
        G = self._graphs
        key = (self._ctx_key, tuple(grad_posteriors.shape), n_active, frozenset(self.frozen), self.grouped_wgrad, self.fused_silu, self.defer_reduces, self.stack_shared_wgrads)
        ent = G["bwd"].get(key)
        if ent is None:
            static_g = grad_posteriors.contiguous().clone()
            graph, _ = _graphs.capture(self._graph_pool(), lambda: self._backward(static_g, n_active, False))
            ent = {"graph": graph, "g": static_g}
            G["bwd"][key] = ent
        ent["g"].copy_(grad_posteriors)
        ent["graph"].replay()
        return None

    def saved_forward(self):
        """Opaque handle of what the last forward saved for its backward.  A loop that runs several forwards before their backwards takes the
        handle after each forward and hands it to `use_saved_forward` before the matching backward()."""
        return self._ctx, self._ctx_static, self._ctx_key

    def use_saved_forward(self, handle):
        self._ctx, self._ctx_static, self._ctx_key = handle

    def _backward(self, grad_posteriors, n_active, input_grad):
        with self._reduce_defer():
            with self._wgrad_queue(self.grouped_wgrad and not self._skip_wgrad):    # every block weight gradient (+ bias sums) of this backward: one launch
                dx = self._backward_body(grad_posteriors, n_active, input_grad)
            self._flush_shared()
        for name, _ in self.spec:                   # after the deferred reductions have been queued: they write gradients too
            if not self.trainable(name):
                self.GR[name].zero_()
        return dx

    def _backward_body(self, grad_posteriors, n_active, input_grad):
        if self._ctx is None:
            raise ops.DynError("backward() without a grad-mode forward")
        static = self._ctx_static
        ctx = dict(self._ctx)                       # shallow copy: a graph-owned context must survive the backward
        ctx["layers"], ctx["sc"] = list(ctx["layers"]), list(ctx["sc"])
        cfg, P, G = self.config, self.P, self.G
        B, T, T3, F3 = ctx["dims"]
        nb = B if n_active is None else int(n_active)
        if grad_posteriors.shape[0] != nb:
            raise ops.DynError(f"backward: gradient batch {grad_posteriors.shape[0]} != active samples {nb}")
        if nb != B:
            rows = nb * T3

            def cut(t):
                if isinstance(t, tuple):
                    return tuple(cut(x) for x in t)
                if t is None:
                    return None
                return t[:rows] if t.dim() == 1 else t[:nb]

            ctx["head"] = cut(ctx["head"])
            ctx["sc"] = [cut(s) for s in ctx["sc"]]
            ctx["layers"] = [{k: cut(v) for k, v in lc.items()} for lc in ctx["layers"]]
            ctx["sub"] = cut(ctx["sub"])
            ctx["dims"] = (nb, T, T3, F3)
        h, mean, rstd, n, logp = ctx["head"]
        dz = ops.log_softmax_bwd(logp, grad_posteriors.contiguous())
        dn = self._lin_bwd(dz, n, "decoder.ff.weight", "decoder.ff.bias")
        dh = torch.empty_like(h)
        ops.layernorm_bwd(h, self._w("decoder.norm.weight"), mean, rstd, dn, dh, self._gw("decoder.norm.weight"), self._gw("decoder.norm.bias"),
                          dx_beta=0.0)
        if getattr(self, "_grad_hidden", None) is not None:
            self._check_not_queued(dh, "the encoder-state gradient")
            ops.axpby(self._grad_hidden.contiguous(), dh, a=1.0, b=1.0)
        nl = cfg["n_layers"]
        for l in reversed(range(nl)):
            if cfg["self_conditioning"] and l != nl - 1:
                h0, mean, rstd, n, pz = ctx["sc"][l]
                dp = self._lin_bwd(dh, pz, "decoder.reproj.weight", "decoder.reproj.bias")
                dzz = ops.softmax_bwd(pz, dp, out=dp)
                dn = self._lin_bwd(dzz, n, "decoder.ff.weight", "decoder.ff.bias")
                dh = self._res_norm_bwd(h0, "decoder.norm.weight", "decoder.norm.bias", mean, rstd, dn, dh)   # dh is a queued operand (re-projection)
            lc = ctx["layers"][l]
            p = f"layers.{l}."
            h0, mean, rstd = lc["norm_out"]
            dh2 = torch.empty_like(dh)
            ops.layernorm_bwd(h0, self._w(p + "norm_out.weight"), mean, rstd, dh, dh2, self._gw(p + "norm_out.weight"),
                              self._gw(p + "norm_out.bias"), dx_beta=0.0)
            dh = dh2
            dh = self._ff_bwd(dh, p + "ff2", lc["ff2"])
            dh = self._conv_bwd(dh, p + "conv", lc["conv"])
            dh = self._attn_bwd(dh, p + "attn", lc["attn"])
            dh = self._ff_bwd(dh, p + "ff1", lc["ff1"])
            ctx["layers"][l] = None  # release this block's activations (queued weight gradients keep what they read)
        dx = self._sub_bwd(dh, ctx, input_grad)
        if not static:
            self._ctx = None
        return dx

    def _ff_bwd(self, dh, p, saved):
        h, mean, rstd, n, u, a = saved
        P, G = self.P, self.G
        du = self._lin_bwd(dh, a, p + ".w2.weight", None, alpha=0.5, silu_of=u)
        dn = self._lin_bwd(du, n, p + ".w1.weight", None)
        return self._res_norm_bwd(h, p + ".norm.weight", p + ".norm.bias", mean, rstd, dn, dh)

    def _attn_bwd(self, dh, p, saved):
        cfg, P, G = self.config, self.P, self.G
        h, mean, rstd, n, qkv, S, O = saved
        H, D = cfg["n_heads"], cfg["head_dim"]
        HD = H * D
        B, T, _ = h.shape
        scale = 1.0 / math.sqrt(D)
        dO = self._lin_bwd(dh, O, p + ".out.weight", p + ".out.bias")
        if S.dim() == 4 and S.shape[0] < B:
            raise ops.DynError(f"backward over {B} samples, but the forward kept the attention probabilities of {S.shape[0]} (model.grad_samples)")
        if S.dim() == 3:        # fused forward kept lse [B, H, T] instead of the probabilities
            dqkv = ops.attention_bwd(qkv, O, dO, S, B, T, H, D, scale)
            cos, sin = self._rotary(T)
            ops.rotary(dqkv, cos, sin, B, T, 2 * H, D, 3 * HD, inverse=True)
            dn = self._lin_bwd(dqkv, n, p + ".qkv.weight", p + ".qkv.bias")
            return self._res_norm_bwd(h, p + ".norm.weight", p + ".norm.bias", mean, rstd, dn, dh)
        dqkv = torch.empty_like(qkv)
        (q, k, v), (dq, dk, dv) = ([_attn.packed(t, j, D) for j in range(3)] for t in (qkv, dqkv))
        dP = torch.empty_like(S)
        _attn.grad_v_dP(S, _attn.plain(dO, D), v, dv, dP)
        ops.softmax_bwd(S, dP, out=dP, scale=1.0)               # dP is now dS
        _attn.grad_qk(dP, q, k, dq, dk, scale)
        cos, sin = self._rotary(T)
        ops.rotary(dqkv, cos, sin, B, T, 2 * H, D, 3 * HD, inverse=True)
        dn = self._lin_bwd(dqkv, n, p + ".qkv.weight", p + ".qkv.bias")
        return self._res_norm_bwd(h, p + ".norm.weight", p + ".norm.bias", mean, rstd, dn, dh)

    def _conv_bwd(self, dh, p, saved):
        cfg, P, G = self.config, self.P, self.G
        h, mean, rstd, n, u, g, c, stats, nn_, s = saved
        dnn = self._lin_bwd(dh, s, p + ".pw2.weight", p + ".pw2.bias", silu_of=nn_)
        dc = torch.empty_like(c)
        if cfg["conv_norm"] == "rms_norm":
            ops.rmsnorm_bwd(c, self._w(p + ".cnorm.weight"), stats[1], dnn, dc, self._gw(p + ".cnorm.weight"), dx_beta=0.0)
        elif cfg["conv_norm"] == "batch_renorm":
            ops.chanaffine_bwd(c, self.buffers[p + ".cnorm.running_mean"], self.buffers[p + ".cnorm.running_var"],
                               P[p + ".cnorm.weight"], dnn, dc, G[p + ".cnorm.weight"], G[p + ".cnorm.bias"], cfg["norm_eps"])
        else:
            ops.layernorm_bwd(c, self._w(p + ".cnorm.weight"), stats[0], stats[1], dnn, dc, self._gw(p + ".cnorm.weight"),
                              self._gw(p + ".cnorm.bias"), dx_beta=0.0)
        if self.R > 1:          # group forms of the depthwise kernels: sample r = replica lo + r
            if self.trainable(p + ".dw.weight") and not self._skip_wgrad:
                ops.dwconv1d_wgrad(g, dc, self._gw(p + ".dw.weight"), self._gw(p + ".dw.bias"), beta=1.0)
            dg = ops.dwconv1d_dgrad(dc, self._w(p + ".dw.weight"))
            du = ops.glu_bwd(u, dg)
            dn = self._lin_bwd(du, n, p + ".pw1.weight", p + ".pw1.bias")
            return self._res_norm_bwd(h, p + ".norm.weight", p + ".norm.bias", mean, rstd, dn, dh)
        if self.trainable(p + ".dw.weight") and not self._skip_wgrad:
            ops.dwconv1d_wgrad(g, dc, G[p + ".dw.weight"], G[p + ".dw.bias"], beta=1.0)
        dg = ops.dwconv1d_dgrad(dc, P[p + ".dw.weight"])
        du = ops.glu_bwd(u, dg)
        dn = self._lin_bwd(du, n, p + ".pw1.weight", p + ".pw1.bias")
        return self._res_norm_bwd(h, p + ".norm.weight", p + ".norm.bias", mean, rstd, dn, dh)

    def _sub_bwd(self, dh, ctx, input_grad=False):
        if not self.trainable("subsampling.") and not input_grad:
            return None
        P, G = self.P, self.G
        wg = self.trainable("subsampling.") and not self._skip_wgrad
        xt, z1, u2, z2, u3, z3, a3 = ctx["sub"]
        B, T, T3, F3 = ctx["dims"]
        C = self.config["subsampling_conv_channels"]
        dz3 = self._lin_bwd(dh, a3.view(B, T3, F3 * C), "subsampling.out.weight", "subsampling.out.bias",
                            silu_of=z3.view(B, T3, F3 * C)).view_as(z3)
        du3 = self._lin_bwd(dz3, u3, "subsampling.pw3.weight", "subsampling.pw3.bias")
        if self.R > 1:
            if z1 is not None or input_grad:
                raise ops.DynError("lockstep group: the subsampling backward needs the fused first two stages and no input gradient")
            PR, GR = self.PR, self.GR
            dz2 = torch.empty_like(z2)
            for r in range(B):
                q = self._lo + r % self.active
                if wg:
                    ops.dwconv2d_s2_wgrad(z2[r:r + 1], du3[r:r + 1], GR["subsampling.dw3.weight"][q], GR["subsampling.dw3.bias"][q], beta=1.0)
                ops.dwconv2d_s2_dgrad(z2[r:r + 1], PR["subsampling.dw3.weight"][q], du3[r:r + 1], out=dz2[r:r + 1])
            du2 = self._lin_bwd(dz2, u2, "subsampling.pw2.weight", "subsampling.pw2.bias")
            if wg:
                for r in range(B):
                    q = self._lo + r % self.active
                    ops.sub12_bwd(xt[r:r + 1], du2[r:r + 1], PR["subsampling.conv1.weight"][q], PR["subsampling.conv1.bias"][q],
                                  PR["subsampling.dw2.weight"][q], GR["subsampling.conv1.weight"][q], GR["subsampling.conv1.bias"][q],
                                  GR["subsampling.dw2.weight"][q], GR["subsampling.dw2.bias"][q], beta=1.0)
            return None
        if wg:
            ops.dwconv2d_s2_wgrad(z2, du3, G["subsampling.dw3.weight"], G["subsampling.dw3.bias"], beta=1.0)
        dz2 = ops.dwconv2d_s2_dgrad(z2, P["subsampling.dw3.weight"], du3)
        du2 = self._lin_bwd(dz2, u2, "subsampling.pw2.weight", "subsampling.pw2.bias")
        if z1 is None and not input_grad:           # fused stages: z1 and dz1 are recomputed inside one kernel, never stored
            if wg:
                ops.sub12_bwd(xt, du2, P["subsampling.conv1.weight"], P["subsampling.conv1.bias"], P["subsampling.dw2.weight"],
                              G["subsampling.conv1.weight"], G["subsampling.conv1.bias"], G["subsampling.dw2.weight"], G["subsampling.dw2.bias"],
                              beta=1.0)
            return None
        if z1 is None:                              # the input gradient (entropy augmentation, lib.py:86-99) needs dz1 itself
            z1 = ops.conv2d_first(xt, P["subsampling.conv1.weight"], P["subsampling.conv1.bias"])
        if wg:
            ops.dwconv2d_s2_wgrad(z1, du2, G["subsampling.dw2.weight"], G["subsampling.dw2.bias"], beta=1.0)
        dz1 = ops.dwconv2d_s2_dgrad(z1, P["subsampling.dw2.weight"], du2)
        if wg:
            ops.conv2d_first_wgrad(xt, dz1, G["subsampling.conv1.weight"], G["subsampling.conv1.bias"], beta=1.0)
        if not input_grad:
            return None
        dxt = ops.conv2d_first_dgrad(dz1, P["subsampling.conv1.weight"], T, xt.shape[-1])      # [B, T, F]
        dx = torch.empty(B, xt.shape[-1], T, device=dxt.device, dtype=torch.float32)
        for b in range(B):
            ops.transpose_ft(dxt[b], out=dx[b])                                                 # -> [B, F, T]
        return dx
