"""The one-token decoder kernels (csrc/decoder_step.hip: dec_gemv_kernel, dec_gemv_rows_kernel, dec_attn_kernel, dec_pick_kernel behind
dyn_decoder_steps and dyn_decoder_steps_batch) against float64 at their row-length, key-count and batch edges.

What was not covered before: test_one_token_decoder_kernels_match_the_tile_kernel_path compares the fused path with another fp32 HIP path at
d_model 256 / 512 (2 of the 8 row-length instances), head dims 32 .. 128, about 20 keys per split and 24 positions; tests/test_enc_dec_rl_gpu.py
runs the batch entry with at most 4 rows (one row group) on the smallest decoder.  Here: every row length for K = d_model and K = d_ff, every
head dim from 4 to 256, 1 / 2 / 4 weight rows per wave and their odd tails, empty key splits, more than 64 and more than 256 keys per split,
the eight-rows-in-flight value loop and its tail, split maxima far apart, the pick kernel's stride loop / ties / -inf, 1 .. 8 batch rows with
retired rows and retired row groups, and every host refusal.

Everything goes through the C-ABI (`_lib.load()` / `check`); the descriptor is built here from a dict of device tensors in the pointer order
of EncDecSCConformerXL._decoder_desc (kernel_refs.DECODER_LAYER_PARAMS, slot 16 the cache, slot 17 the projected kv), so no encoder exists and
the key count is the test's choice.  Weights are drawn as the oracle draws them (kernel_refs.decoder_params).  Caches, logits and scratch start
as NaN; every buffer lies between sentinel guards, every batch row is followed by sentinel padding (a cache row, three token slots, four
scratch floats), and every check of a result also checks, bit for bit, that nothing outside the owned elements — the weights included — changed.

Reference: kernel_refs.decoder_steps_ref, float64 on the CPU, held to oracle.enc_dec_ref.Decoder in tests/test_kernel_refs_cpu.py.
Bounds: kernel_refs.decoder_tol — 4 x the error of the same function evaluated in fp32 on the CPU, plus 2e-5 * max(1, max|want|) (the 2e-5
test_one_token_decoder_kernels_match_the_tile_kernel_path asserts for these logits and cache rows).  Token ids are held exactly where they are
scripted (zero head weight: the logits ARE the head bias) and bit-exact claims use torch.equal on the bits.  Every check prints
`case name: kernel error | fp32 error | bound` before it asserts (pytest -s; the table of one MI355X run is profiles/decoder_step_parity.txt).
Nothing here measures speed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
INF = float("inf")
SENTINEL = -7.25
TOK_SENTINEL = -77
GUARD = 64                               # elements on either side of every buffer (256 bytes: the owned part stays 16-byte aligned)
V = 67
OK, E_ARG, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -3, -4
TEMPERATURE = 1.5
INV_T = float(np.float32(1.0) / np.float32(TEMPERATURE))


# ----------------------------------------------------------------------------------------------------------- helpers
def _lib():
    from dynamic_asr_eval_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _close(case, name, got, want32, want64):
    tol, e32 = K.decoder_tol(want32, want64)
    err = K.max_err(got, want64)
    print(f"  {case} {name}: kernel {err:.2e} | fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, f"{case} {name}: err {err} > {tol} (fp32: {e32})"                 # a NaN error fails here too


def _exact(case, name, ok):
    print(f"  {case} {name}: bit-equal {bool(ok)}")
    assert ok, f"{case} {name}: not bit-equal"


def _first_max(x):
    x = x.detach().cpu()
    return int((x == x.max()).nonzero()[0])


class Model:
    """One decoder's weights and projected encoder keys | values: fp32 on the CPU (what the references read) and on the device."""

    def __init__(self, cuda, d_model, heads, d_ff, layers=1, vocab=V, n_enc=37, max_positions=8, seed=0, kv_gain=1.0, edit=None):
        self.cuda, self.d_model, self.heads, self.d_ff, self.layers, self.vocab = cuda, d_model, heads, d_ff, layers, vocab
        self.n_enc, self.max_positions = n_enc, max_positions
        self.cpu = K.decoder_params(d_model, d_ff, vocab, layers, max_positions, seed)
        if edit is not None:
            edit(self.cpu)
        self.kv_cpu = K.decoder_kv(layers, n_enc, d_model, seed, kv_gain)
        self.dev = {k: v.to(cuda) for k, v in self.cpu.items()}
        self.kv = [t.to(cuda) for t in self.kv_cpu]
        self.per_row = int(_lib().load().dyn_decoder_row_scratch_floats(d_model, d_ff, heads))
        assert self.per_row == 6 * d_model + d_ff + 16 * heads

    def set_head_bias(self, b):
        self.cpu["head.bias"] = b.clone()
        self.dev["head.bias"].copy_(b)

    def ref(self, tokens, dtype, cross_q=None):
        return K.decoder_steps_ref({k: v.to(dtype) for k, v in self.cpu.items()}, tokens, [t.to(dtype) for t in self.kv_cpu], self.heads,
                                   K.DECODER_EPS, cross_q=cross_q)

    def untouched(self):
        return all(torch.equal(self.dev[k].cpu(), v) for k, v in self.cpu.items()) and \
            all(torch.equal(a.cpu(), b) for a, b in zip(self.kv, self.kv_cpu))


def _zero_head(p):
    p["head.weight"].zero_()


def _never_id_0(p):
    """Head bias -30 at id 0, the default eos of a batch state: no greedy row retires by chance."""
    p["head.bias"][0] = -30.0


class State:
    """What one decode owns: token slots 0 .. positions, cache rows 0 .. positions - 1 of every layer, the logits and the scratch, for one
    row (`rows` None: dyn_decoder_steps) or `rows` rows (dyn_decoder_steps_batch).  Each lives in a flat buffer between GUARD sentinels;
    a row's tokens are followed by 3 sentinel slots, its cache by one sentinel row, its scratch (batch) by 4 sentinel floats."""

    def __init__(self, model, positions, rows=None, eos=0):
        m, dev = model, model.cuda
        self.model, self.positions, self.rows, self.eos = m, positions, rows, eos
        R = self.R = rows or 1
        dd = m.d_model
        self.tok_stride = positions + 1 + 3
        self.cache_stride = (positions + 1) * 3 * dd
        self.scr_stride = m.per_row + (4 if rows else 0)

        def buf(n, sentinel, dtype):
            return torch.full((2 * GUARD + n,), sentinel, dtype=dtype, device=dev)

        self.tok_flat = buf(R * self.tok_stride, TOK_SENTINEL, torch.int32)
        self.tokens = self.tok_flat[GUARD:GUARD + R * self.tok_stride].view(R, self.tok_stride)
        self.cache_flat = [buf(R * self.cache_stride, SENTINEL, torch.float32) for _ in range(m.layers)]
        self.cache = [f[GUARD:GUARD + R * self.cache_stride].view(R, positions + 1, 3 * dd) for f in self.cache_flat]
        self.logits_flat = buf(R * m.vocab, SENTINEL, torch.float32)
        self.logits = self.logits_flat[GUARD:GUARD + R * m.vocab].view(R, m.vocab)
        self.scr_flat = buf(R * self.scr_stride, SENTINEL, torch.float32)
        self.scratch = self.scr_flat[GUARD:GUARD + R * self.scr_stride].view(R, self.scr_stride)
        self.finished = torch.zeros(R, dtype=torch.int32, device=dev)
        self.flats = [self.tok_flat, *self.cache_flat, self.logits_flat, self.scr_flat]
        owned = [self.tokens[:, :positions + 1], *[c[:, :positions] for c in self.cache], self.logits, self.scratch[:, :m.per_row]]
        self.outside = []
        for flat, view in zip(self.flats, owned):                # the owned views write through to the flat buffers
            view.fill_(1)
            self.outside.append(_bits(flat) != _bits(torch.ones((), dtype=flat.dtype, device=dev)))
            view.fill_(0 if flat.dtype == torch.int32 else NAN)
        self.prefill = self.snapshot()
        self._keep = None

    def snapshot(self):
        return [f.clone() for f in self.flats]

    def unchanged_since(self, snap):
        return all(_same_bits(f, s) for f, s in zip(self.flats, snap))

    def outside_untouched(self):
        return all(torch.equal(_bits(f)[o], _bits(s)[o]) for f, s, o in zip(self.flats, self.prefill, self.outside)) and self.model.untouched()

    def desc(self, null_layer_ptr=None, **over):
        m, L = self.model, _lib()
        ptrs = (ctypes.c_void_p * (m.layers * L.DEC_PTRS_PER_LAYER))()
        for l in range(m.layers):
            for i, nm in enumerate(K.DECODER_LAYER_PARAMS):
                ptrs[l * L.DEC_PTRS_PER_LAYER + i] = m.dev[f"layers.{l}.{nm}"].data_ptr()
            ptrs[l * L.DEC_PTRS_PER_LAYER + 16] = self.cache[l].data_ptr()
            ptrs[l * L.DEC_PTRS_PER_LAYER + 17] = m.kv[l].data_ptr()
        if null_layer_ptr is not None:
            ptrs[null_layer_ptr] = None
        self._keep = ptrs
        f = dict(d_model=m.d_model, heads=m.heads, d_ff=m.d_ff, vocab=m.vocab, layers=m.layers, n_enc=m.n_enc, max_positions=m.max_positions,
                 eps=K.DECODER_EPS, embed=m.dev["embed.weight"].data_ptr(), pos_table=m.dev["pos"].data_ptr(),
                 norm_out_w=m.dev["norm_out.weight"].data_ptr(), norm_out_b=m.dev["norm_out.bias"].data_ptr(),
                 head_w=m.dev["head.weight"].data_ptr(), head_b=m.dev["head.bias"].data_ptr(),
                 layer_ptrs=ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), tokens=self.tokens.data_ptr(), logits=self.logits.data_ptr(),
                 scratch=self.scratch.data_ptr(), scratch_floats=self.R * self.scr_stride)
        b = dict(rows=self.R, eos_id=self.eos, token_stride=self.tok_stride, cache_stride=self.cache_stride, finished=self.finished.data_ptr())
        for k, v in over.items():
            (b if k in b else f)[k] = v
        base = L.DecoderDesc(**f)
        return base if self.rows is None else L.DecoderBatchDesc(base=base, **b)

    def steps(self, t0, n, sample=0, inv_t=1.0, seed=0, step0=0, **over):
        """The entry's return code."""
        lib = _lib().load()
        fn = lib.dyn_decoder_steps if self.rows is None else lib.dyn_decoder_steps_batch
        return fn(ctypes.byref(self.desc(**over)), t0, n, sample, inv_t, seed, step0, _stream())

    def run(self, *a, **k):
        _lib().check(self.steps(*a, **k), "dyn_decoder_steps" if self.rows is None else "dyn_decoder_steps_batch")


def _scripted(st, script):
    """One step per call on row 0 of a single-row state, tokens[t + 1] overwritten with the script after each: the logits of every step
    [S, V] (the entry keeps only the last position's).  The id the kernel wrote is the first maximum of its own logits."""
    S = len(script)
    st.tokens[0, 0] = script[0]
    out = []
    for t in range(S):
        st.run(t, 1)
        out.append(st.logits[0].clone())
        assert int(st.tokens[0, t + 1]) == _first_max(out[-1]), f"step {t}: the id written is not the first maximum of the logits"
        if t + 1 < S:
            st.tokens[0, t + 1] = script[t + 1]
    return torch.stack(out)


def _parity(case, m, script):
    """Scripted steps of a fresh single-row state against float64: the logits of every step and the cache rows of every layer."""
    S = len(script)
    st = State(m, S)
    got = _scripted(st, script)
    want64, rows64 = m.ref(script, F64)
    want32, rows32 = m.ref(script, torch.float32)
    _close(case, "logits", got, want32, want64)
    for l in range(m.layers):
        _close(case, f"cache rows, layer {l}", st.cache[l][0, :S], rows32[l], rows64[l])
    _exact(case, "nothing written outside the owned elements", st.outside_untouched())
    return st


# ----------------------------------------------------------------------------------------------------------- a. row lengths
# NV = 1 .. 8 for K = d_model and for K = d_ff, head dims 4 .. 256, 1 / 2 / 4 weight rows per wave (N = V = 67 and 256: 1; 512 .. 3840: 2;
# 3 * d_model >= 4096: 4) with the odd tail of a pair at V = 67.  The 2-layer case reaches the LayerNorm qkv launch that does not embed.
ROW_LENGTHS = [(256, 64, 256, 1), (256, 1, 512, 1), (512, 64, 1536, 1), (768, 48, 768, 1), (1024, 32, 2048, 1), (1280, 20, 1280, 1),
               (1536, 12, 1536, 1), (1792, 7, 1792, 1), (2048, 8, 2048, 1), (768, 48, 768, 2)]


@pytest.mark.parametrize("d_model,heads,d_ff,layers", ROW_LENGTHS)
def test_row_lengths(cuda, d_model, heads, d_ff, layers):
    print()
    m = Model(cuda, d_model, heads, d_ff, layers=layers, n_enc=37, max_positions=6, seed=d_model // 256)
    script = torch.randint(0, V, (6,), generator=K.gen(d_model + heads)).tolist()
    _parity(f"rows d={d_model} H={heads} hd={d_model // heads} ff={d_ff} L={layers}", m, script)


# ----------------------------------------------------------------------------------------------------------- b. cross-attention key counts
def _cross_counts(hd):
    """1 .. 5: empty splits (n_keys < 4, and 5 = chunks of 2, 2, 1, 0); 255 .. 260: 64 keys per split, the second pass of the score loop;
    1024 .. 1029: 256 per split, the second turn of the max / exp stride loops; 4 * n for n around 7 ng and 8 ng (ng = 256 / hd value rows
    per pass): the first full turn of the eight-rows-in-flight value loop and its tail."""
    ng = 256 // hd
    return sorted(set([1, 2, 3, 4, 5, 255, 256, 257, 260, 1024, 1025, 1029] + [4 * n for n in (7 * ng, 7 * ng + 1, 8 * ng, 8 * ng + 1)]))


@pytest.mark.parametrize("heads,n_enc", [(H, n) for H in (64, 4, 1) for n in _cross_counts(256 // H)])
def test_cross_attention_key_counts(cuda, heads, n_enc):
    print()
    m = Model(cuda, 256, heads, 256, n_enc=n_enc, max_positions=2, seed=heads)
    _parity(f"cross hd={256 // heads} n_enc={n_enc}", m, [5, 40])


PEAKY_SPREAD = 10.0


@pytest.mark.parametrize("heads,gain", [(64, 8.0), (4, 32.0), (1, 64.0)])
def test_cross_attention_split_maxima_far_apart(cuda, heads, gain):
    """kv scaled by 8 at head dim 4 (by 32 and 64 at head dims 64 and 256, whose scores average over more terms): the four splits' score
    maxima differ by more than 10 for some (step, head) — asserted on the float64 scores — so whole splits enter the merge with weights
    exp(max_u - max) of e^-10 and below."""
    print()
    case = f"peaky hd={256 // heads} n_enc=260 kv x {gain:g}"
    m = Model(cuda, 256, heads, 256, n_enc=260, max_positions=2, seed=heads, kv_gain=gain)
    cross_q = []
    m.ref([5, 40], F64, cross_q=cross_q)
    spread = 0.0
    for t in range(2):
        mx = K.decoder_split_maxima(cross_q[0][t], m.kv_cpu[0][:, :256], heads)
        spread = max(spread, (mx.max(-1).values - mx.min(-1).values).max().item())
    print(f"  {case}: largest spread of a head's split maxima {spread:.1f}")
    assert spread > PEAKY_SPREAD, f"fixture: split maxima only {spread} apart"
    _parity(case, m, [5, 40])


# ----------------------------------------------------------------------------------------------------------- c. self-attention key counts
LONG_STEPS = 1030


def test_self_attention_key_counts_over_one_long_sampled_run(cuda):
    """ONE call of 1030 sampled steps (no sync between them): t + 1 keys walk through every split boundary, more than 64 keys per split from
    t = 256 and more than 256 from t = 1024.  The reference runs teacher-forced on the ids the kernel drew; the 1030 cache rows the call
    wrote (positions 0 .. 1029) of both layers and the final logits are compared — the ids are not (a sampled near-tie may flip one).
    The same run in calls of 1, 7 and 64 steps leaves the same bits."""
    print()
    N, seed, step0, case = LONG_STEPS, 5, 100, "self 1030 steps"
    m = Model(cuda, 256, 4, 512, layers=2, n_enc=37, max_positions=N, seed=3)
    st = State(m, N)
    st.run(0, N, 1, INV_T, seed, step0)
    toks = st.tokens[0, :N + 1].tolist()
    assert min(toks) >= 0 and max(toks) < V and len(set(toks)) > V // 2, "the sampled prefix is varied"
    want64, rows64 = m.ref(toks[:N], F64)
    want32, rows32 = m.ref(toks[:N], torch.float32)
    for l in range(2):
        _close(case, f"cache rows, layer {l}", st.cache[l][0, :N], rows32[l], rows64[l])
    _close(case, "final logits", st.logits[0], want32[N - 1], want64[N - 1])
    _exact(case, "nothing written outside the owned elements", st.outside_untouched())
    for chunk in (1, 7, 64):
        st2 = State(m, N)
        for t in range(0, N, chunk):
            st2.run(t, min(chunk, N - t), 1, INV_T, seed, step0)
        _exact(case, f"tokens, caches and logits of calls of {chunk}", all(_same_bits(a, b) for a, b in zip(st2.flats[:-1], st.flats[:-1])))


# ----------------------------------------------------------------------------------------------------------- d. pick kernel, exact
PICK_VOCABS = [2, 63, 64, 65, 1023, 1024, 1025, 4097]


def pick_scripts(Vv):
    """(name, head bias [Vv], the id a first-maximum argmax returns): thread c of the 1024 takes columns c, c + 1024, ..; wave = c / 64."""
    g = K.gen(700 + Vv)
    out = []
    b = torch.randn(Vv, generator=g)
    b[Vv - 1] = b.max() + 1
    out.append(("unique maximum in the last column", b, Vv - 1))
    pairs = [(1, Vv - 1) if Vv > 2 else (0, 1)]                  # V > 65: two waves; V <= 64: two lanes of one wave
    if Vv > 1024:
        pairs += [(1023, 1024), (0, 1024), (1000, Vv - 1)]       # either side of the stride: last and first thread; one thread's two turns
    for lo, hi in pairs:
        b = torch.randn(Vv, generator=g)
        b[lo] = b[hi] = b.max() + 1
        out.append((f"equal maxima at {lo} and {hi}", b, lo))
    b = torch.randn(Vv, generator=g)
    b[::2] = -INF
    out.append(("-inf entries", b, _first_max(b)))
    b = torch.randn(Vv, generator=g)
    b[:Vv - 1] = -INF
    out.append(("-inf everywhere but the last column", b, Vv - 1))
    out.append(("all -inf", torch.full((Vv,), -INF), 0))
    return out


def sampled_bias(Vv, eos=None, eos_shift=0.0):
    """Head bias for the sampled picks: N(0, 2), every seventh entry -inf; `eos`: that entry finite and shifted, or -inf (never drawn)."""
    b = torch.randn(Vv, generator=K.gen(810 + Vv)) * 2
    b[3::7] = -INF
    if eos is not None:
        b[eos] = eos_shift
    return b


def oracle_draw(b, seed, step, margins):
    """oracle.enc_dec_ref.gumbel_argmax on the logits `b`; `margins` collects the top-2 margin of the keys."""
    from oracle.enc_dec_ref import gumbel_argmax
    from enc_dec_rl_cpu import gumbel_keys
    if b.numel() > 1:
        top = np.sort(gumbel_keys(b, INV_T, seed, step))[-2:]
        margins.append(float(top[1] - top[0]))
    return gumbel_argmax(b, TEMPERATURE, seed, step)


@pytest.mark.parametrize("Vv", PICK_VOCABS)
def test_pick_kernel_greedy_ids_are_exact(cuda, Vv):
    """Zero head weight: the logits are the head bias bit for bit (asserted), so the id is decided by the pick kernel alone."""
    print()
    m = Model(cuda, 256, 4, 256, vocab=Vv, n_enc=5, max_positions=2, edit=_zero_head)
    for name, b, want in pick_scripts(Vv):
        case = f"pick V={Vv} {name}"
        m.set_head_bias(b)
        for rows in (None, 3):
            st = State(m, 1, rows=rows, eos=(want + 1) % Vv)
            st.tokens[:, 0] = torch.arange(st.R, dtype=torch.int32, device=cuda) % Vv
            st.run(0, 1)
            entry = "single" if rows is None else "batch"
            _exact(case, f"{entry}: logits are the head bias", all(_same_bits(st.logits[r].cpu(), b) for r in range(st.R)))
            got = st.tokens[:, 1].tolist()
            print(f"  {case} {entry}: ids {got} | want {want}")
            assert got == [want] * st.R and st.finished.tolist() == [0] * st.R
            assert st.outside_untouched()


@pytest.mark.parametrize("Vv", PICK_VOCABS)
def test_pick_kernel_sampled_ids_are_the_oracles(cuda, Vv):
    """Sampled ids equal oracle.enc_dec_ref.gumbel_argmax at (seed, step0 + t), at seed + row in the batch entry; the oracle's top-2 key
    margin exceeds 1e-3 at every draw (asserted here, on the CPU side)."""
    print()
    seed, step0, n = 9, 1000, 3
    eos = 0
    b = sampled_bias(Vv, eos=eos, eos_shift=-INF)                # eos is never drawn: no row retires
    m = Model(cuda, 256, 4, 256, vocab=Vv, n_enc=5, max_positions=n, edit=_zero_head)
    m.set_head_bias(b)
    for rows in (None, 3):
        margins = []
        st = State(m, n, rows=rows, eos=eos)
        want = [[oracle_draw(b, seed + r, step0 + t, margins) for t in range(n)] for r in range(st.R)]
        assert min(margins) > 1e-3, f"fixture: a sampled step is a near-tie on the oracle ({min(margins):.2e})"
        st.run(0, n, 1, INV_T, seed, step0)
        got = st.tokens[:, 1:n + 1].tolist()
        print(f"  pick V={Vv} sampled {'single' if rows is None else 'batch'}: ids {got} | want {want} | smallest margin {min(margins):.2e}")
        assert got == want and st.finished.tolist() == [0] * st.R
        assert all(_same_bits(st.logits[r].cpu(), b) for r in range(st.R)) and st.outside_untouched()


# ----------------------------------------------------------------------------------------------------------- e. batch entry, bitwise
BATCH_CONFIGS = [(256, 4, 256), (2048, 8, 2048)]
BATCH_STEPS = 3
_MODEL = {}


def _batch_model(cuda, cfg):
    """One model per configuration, kept while consecutive cases use it (the 2048-wide one is 135 MB).  Its eos (the last id) is never the
    greedy pick: head bias -30."""
    if _MODEL.get("cfg") != cfg:
        _MODEL.clear()
        _MODEL.update(cfg=cfg, model=Model(cuda, *cfg, n_enc=37, max_positions=BATCH_STEPS, seed=11,
                                            edit=lambda p: p["head.bias"].__setitem__(V - 1, -30.0)), single={})
    return _MODEL["model"], _MODEL["single"]


def _single_rows(m, cache, scripts):
    """dyn_decoder_steps on each row alone: per row (logits of every step [S, V], the cache rows of every layer)."""
    for r, script in enumerate(scripts):
        if tuple(script) not in cache:
            st = State(m, BATCH_STEPS)
            cache[tuple(script)] = (_scripted(st, script), [c[0, :BATCH_STEPS].clone() for c in st.cache])
    return [cache[tuple(s)] for s in scripts]


def retirement_patterns(R):
    """{name: {step: rows whose flag is set before that step}}."""
    pats = {"all live": {}}
    if R >= 2:
        pats["a row retired mid-run in each group"] = {1: [1] + ([R - 1] if R > 4 else [])}
    if R > 4:
        pats["second group retired"] = {0: list(range(4, R))}
        pats["first group retired"] = {0: [0, 1, 2, 3]}
    return pats


@pytest.mark.parametrize("cfg,R", [pytest.param(c, R, id=f"d{c[0]}-R{R}") for c in BATCH_CONFIGS for R in (1, 2, 4, 5, 7, 8)])
def test_batch_rows_are_the_single_row_entry_bit_for_bit(cuda, cfg, R):
    """Every live row's logits (each step) and cache rows equal dyn_decoder_steps on that row alone; a retired row's cache rows, logits and
    scratch block keep their bits (NaN where never written) and its next token slot holds eos."""
    print()
    m, cache = _batch_model(cuda, cfg)
    eos = V - 1
    scripts = torch.randint(0, V - 1, (R, BATCH_STEPS), generator=K.gen(900 + R)).tolist()
    single = _single_rows(m, cache, scripts)
    for name, retire in retirement_patterns(R).items():
        case = f"batch d={cfg[0]} R={R} {name}"
        st = State(m, BATCH_STEPS, rows=R, eos=eos)
        st.tokens[:, 0] = torch.tensor([s[0] for s in scripts], dtype=torch.int32)
        retired_at = {}
        ok_live = ok_retired = True
        for t in range(BATCH_STEPS):
            for r in retire.get(t, []):
                st.finished[r] = 1
                retired_at[r] = t
            before = [c.clone() for c in st.cache], st.logits.clone(), st.scratch.clone()
            st.run(t, 1)
            toks = st.tokens[:, t + 1].tolist()
            for r in range(R):
                if r in retired_at:
                    ok_retired = ok_retired and all(_same_bits(c[r], b[r]) for c, b in zip(st.cache, before[0])) and \
                        _same_bits(st.logits[r], before[1][r]) and _same_bits(st.scratch[r], before[2][r]) and toks[r] == eos
                else:
                    ok_live = ok_live and torch.equal(st.logits[r], single[r][0][t]) and toks[r] == _first_max(single[r][0][t])
                    if t + 1 < BATCH_STEPS:
                        st.tokens[r, t + 1] = scripts[r][t + 1]
        assert st.finished.tolist() == [1 if r in retired_at else 0 for r in range(R)]
        for r in range(R):
            n = retired_at.get(r, BATCH_STEPS)
            ok_live = ok_live and all(torch.equal(c[r, :n], s[:n]) for c, s in zip(st.cache, single[r][1]))
            ok_retired = ok_retired and all(bool(torch.isnan(c[r, n:BATCH_STEPS]).all()) for c in st.cache)
            if n == 0:
                ok_retired = ok_retired and bool(torch.isnan(st.logits[r]).all()) and bool(torch.isnan(st.scratch[r, :m.per_row]).all())
        _exact(case, "live rows: logits of every step and cache rows equal the single-row entry", ok_live)
        _exact(case, "retired rows: cache, logits and scratch keep their bits, eos in the next slot", ok_retired)
        _exact(case, "nothing written outside the owned elements", st.outside_untouched())


def eos_fixture(R=8, n=4, seed=21, step0=50, eos=7):
    """Head bias (zero head weight: the logits) and, per row, the oracle's draws of (seed + row, step0 + t) up to its eos: the token
    matrix [R, n] the batch entry must leave (eos after a row's eos) and the flags."""
    b = sampled_bias(V, eos=eos, eos_shift=5.0)
    margins, want, flags = [], [], []
    for r in range(R):
        row, done = [], False
        for t in range(n):
            row.append(eos if done else oracle_draw(b, seed + r, step0 + t, margins))
            done = done or row[-1] == eos
        want.append(row)
        flags.append(int(done))
    assert min(margins) > 1e-3, f"fixture: a sampled step is a near-tie on the oracle ({min(margins):.2e})"
    firsts = [row.index(eos) if eos in row else n for row in want]
    assert 0 in firsts and n in firsts and any(0 < f < n for f in firsts), f"fixture: rows end at mixed steps ({firsts})"
    return b, want, flags, firsts


def test_batch_rows_that_pick_eos_retire(cuda):
    """ONE call of 4 steps, 8 rows: a live row that picks eos sets its flag, writes no cache row after that step and eos fills its later
    slots.  Scripted through the head bias (zero head weight); sampled rows end at mixed steps, the greedy rows all at step 0."""
    print()
    R, n, seed, step0, eos = 8, 4, 21, 50, 7
    b, want, flags, firsts = eos_fixture(R, n, seed, step0, eos)
    m = Model(cuda, 256, 4, 256, n_enc=5, max_positions=n, edit=_zero_head)
    m.set_head_bias(b)
    st = State(m, n, rows=R, eos=eos)
    st.run(0, n, 1, INV_T, seed, step0)
    got = st.tokens[:, 1:n + 1].tolist()
    print(f"  eos sampled: ids {got} | want {want} | first eos at {firsts}")
    assert got == want and st.finished.tolist() == flags
    for r in range(R):
        rows_written = min(firsts[r] + 1, n)                     # the step that drew eos still wrote its cache row
        for c in st.cache:
            assert bool(torch.isfinite(c[r, :rows_written]).all()) and bool(torch.isnan(c[r, rows_written:n]).all()), (r, firsts[r])
    assert st.outside_untouched()
    g = b.clone()
    g[eos] = 9.0
    m.set_head_bias(g)
    st = State(m, n, rows=R, eos=eos)
    st.run(0, n)
    print(f"  eos greedy: ids {st.tokens[:, 1:n + 1].tolist()}")
    assert st.tokens[:, 1:n + 1].tolist() == [[eos] * n] * R and st.finished.tolist() == [1] * R
    for c in st.cache:
        assert bool(torch.isfinite(c[:, :1]).all()) and bool(torch.isnan(c[:, 1:n]).all())
    assert st.outside_untouched()


# ----------------------------------------------------------------------------------------------------------- f. guards
def _refused(st, code, what, *a, **over):
    """The entry returns `code` and every buffer keeps its prefill bits: nothing was launched."""
    rc = st.steps(*a, **over)
    torch.cuda.synchronize()
    print(f"  guard {'single' if st.rows is None else 'batch'} {what}: code {rc} | want {code} | buffers untouched {st.unchanged_since(st.prefill)}")
    assert rc == code, f"{what}: code {rc}, wanted {code}"
    assert st.unchanged_since(st.prefill) and st.model.untouched(), f"{what}: a refused call wrote something"
    if code != OK:
        with pytest.raises(_lib().DynError):
            _lib().check(rc, what)


@pytest.mark.parametrize("rows", [None, 3])
def test_guards_shared_by_both_entries(cuda, rows):
    """Host-side argument checks only: every refused call changes descriptor fields, never the buffers behind them."""
    print()
    m = Model(cuda, 256, 4, 256, n_enc=5, max_positions=9, edit=_never_id_0)
    st = State(m, 9, rows=rows)
    R = st.R
    for what, code, args, over in [
            ("d_model 128", E_UNSUPPORTED, (0, 1), dict(d_model=128)),
            ("d_model 2304", E_UNSUPPORTED, (0, 1), dict(d_model=2304, heads=9)),
            ("d_ff 384", E_UNSUPPORTED, (0, 1), dict(d_ff=384)),
            ("head dim 192", E_UNSUPPORTED, (0, 1), dict(d_model=768, heads=4)),
            ("head dim 512", E_UNSUPPORTED, (0, 1), dict(d_model=512, heads=1)),
            ("d_model % heads", E_ARG, (0, 1), dict(heads=3)),
            ("t0 + n_steps > max_positions", E_ARG, (8, 2), {}),
            ("t0 past max_positions", E_ARG, (9, 1), {}),
            ("n_enc 0", E_ARG, (0, 1), dict(n_enc=0)),
            ("scratch one float short", E_WORKSPACE, (0, 1), dict(scratch_floats=R * m.per_row - 1)),
            ("sampling at inverse temperature 0", E_ARG, (0, 1, 1, 0.0), {}),
            ("null layer pointer", E_ARG, (0, 1), dict(null_layer_ptr=10)),
            ("null cache pointer", E_ARG, (0, 1), dict(null_layer_ptr=16)),
            ("null logits", E_ARG, (0, 1), dict(logits=None)),
            ("n_steps 0", OK, (3, 0), {})]:
        _refused(st, code, what, *args, **over)
    lib = _lib().load()
    fn = lib.dyn_decoder_steps if rows is None else lib.dyn_decoder_steps_batch
    rc = fn(None, 0, 1, 0, 1.0, 0, 0, _stream())
    print(f"  guard null descriptor: code {rc}")
    assert rc == E_ARG and st.unchanged_since(st.prefill)
    # the last legal position: t0 + n_steps == max_positions == 9 is accepted and correct
    script = torch.randint(0, V, (9,), generator=K.gen(77)).tolist()
    if rows is None:
        _parity("guard last legal position (9 of 9)", m, script)
    else:
        want64, rows64 = m.ref(script, F64)
        want32, rows32 = m.ref(script, torch.float32)
        st.tokens[:, :9] = torch.tensor(script, dtype=torch.int32, device=cuda)
        for t in range(9):                                       # teacher-forced: the slot a step writes is rewritten before the next
            st.run(t, 1)
            if t + 1 < 9:
                st.tokens[:, t + 1] = script[t + 1]
        for r in range(R):
            _close("guard last legal position (9 of 9)", f"batch row {r} logits", st.logits[r], want32[8], want64[8])
            _close("guard last legal position (9 of 9)", f"batch row {r} cache rows", st.cache[0][r, :9], rows32[0], rows64[0])
        assert st.outside_untouched()


def test_guards_of_the_batch_entry(cuda):
    print()
    m = Model(cuda, 256, 4, 256, n_enc=5, max_positions=9, edit=_never_id_0)
    st = State(m, 9, rows=2)
    need = 3 * 3 * 256                                           # cache floats of t0 + n_steps = 3 positions
    for what, over in [
            ("rows 0", dict(rows=0)), ("rows 9", dict(rows=9)), ("eos = vocab", dict(eos_id=V)), ("eos -1", dict(eos_id=-1)),
            ("token_stride = last slot", dict(token_stride=3)), ("cache_stride too small", dict(cache_stride=need - 4)),
            ("cache_stride not a multiple of 4", dict(cache_stride=need + 2)),
            ("per-row scratch not a multiple of 4", dict(scratch_floats=2 * (m.per_row + 1))),
            ("null finished flags", dict(finished=None))]:
        _refused(st, E_ARG, what, 0, 3, **over)
    st.run(0, 3)                                                 # the same call with nothing overridden is accepted
    assert bool(torch.isfinite(st.logits).all()) and st.outside_untouched()
