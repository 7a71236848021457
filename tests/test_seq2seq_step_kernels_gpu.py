"""The one-token seq2seq step (csrc/seq2seq_step.hip: s2s_gemv_kernel in its four prologues and three row-block instances, dec_attn_kernel,
s2s_pick_kernel behind dyn_seq2seq_steps) through the C ABI against float64, at its width, row and key edges.

Reference: cohere_asr_refs.decoder_ref on the CPU (held to transformers in tests/test_cohere_asr_cpu.py) over the tokens the kernel itself
picked, in float64 and, for the bound, in fp32.  Bound (cohere_asr_refs.step_tol, the recipe of tests/test_decoder_step_kernels_gpu.py):
4 x the error of the same function in fp32 on the CPU + 2e-5 * max(1, max |want|).  Every check prints `case: kernel | fp32 | bound`
before it asserts (pytest -s; one MI355X run's table is profiles/seq2seq_step_parity.txt); bit-exact claims compare the bits.

Caches, logits and scratch start as NaN; tokens, caches, logits, scratch and flags each lie between sentinel guards, every batch row's
cache is followed by a sentinel row and its tokens by three sentinel slots, and every check of a result also checks, bit for bit, that no
unowned element and no weight changed.  The id every live step writes is the first maximum of its own logits.  Nothing here measures speed."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cohere_asr_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
SENTINEL, TOK_SENTINEL, GUARD = -7.25, -77, 64
OK, E_ARG, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -3, -4
PAD, EOS = 2, 3


def _lib():
    from dynamic_asr_eval_amd import _lib as L
    return L


def _bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _close(case, name, got, want32, want64):
    tol, e32 = R.step_tol(want32, want64)
    err = (got.detach().cpu().double() - want64).abs().max().item()
    print(f"  {case} {name}: kernel {err:.2e} | fp32 {e32:.2e} | bound {tol:.2e}")
    assert err <= tol, f"{case} {name}: err {err} > {tol} (fp32: {e32})"                 # a NaN error fails here too


def _exact(case, name, ok):
    print(f"  {case} {name}: bit-equal {bool(ok)}")
    assert ok, f"{case} {name}: not bit-equal"


def _first_max(x):
    x = x.detach().cpu()
    return int((x == x.max()).nonzero()[0])


class Model:
    """One decoder's weights (cohere_asr_refs.decoder_params; the packed q | k | v built here) and per-row cross keys | values: fp32 on
    the CPU (what the references read) and on the device."""

    def __init__(self, cuda, d, heads, ff, layers=1, vocab=40, n_enc=9, rows=1, max_positions=12, seed=0, edit=None):
        self.cuda, self.d, self.heads, self.ff, self.layers, self.vocab, self.n_enc, self.rows = cuda, d, heads, ff, layers, vocab, n_enc, rows
        self.max_positions = max_positions
        self.cpu = R.decoder_params(d, ff, vocab, layers, max_positions, seed)
        self.cpu["proj_out.bias"][EOS] = -30.0                       # no greedy row retires by chance
        if edit is not None:
            edit(self.cpu)
        self.kv_cpu = R.cross_kv(layers, rows, n_enc, d, seed)
        self.dev = {k: v.to(cuda) for k, v in self.cpu.items()}
        for l in range(layers):
            p = f"layers.{l}.self_attn."
            self.dev[p + "qkv.weight"] = torch.cat([self.dev[p + f"{c}_proj.weight"] for c in "qkv"]).contiguous()
            self.dev[p + "qkv.bias"] = torch.cat([self.dev[p + f"{c}_proj.bias"] for c in "qkv"]).contiguous()
        self.kept = {k: v.clone() for k, v in self.dev.items()}
        self.kv = [t.to(cuda) for t in self.kv_cpu]
        self.per_row = int(_lib().load().dyn_seq2seq_row_scratch_floats(d, ff, heads))
        assert self.per_row == 2 * d + ff + 4 * heads * (d // heads + 4)

    def set_head_bias(self, b):
        self.cpu["proj_out.bias"] = b.clone()
        self.dev["proj_out.bias"].copy_(b)
        self.kept["proj_out.bias"].copy_(b)

    def ref(self, tokens, dtype, rows=None):
        kv = self.kv_cpu if rows is None else [t[rows] for t in self.kv_cpu]
        return R.decoder_ref(self.cpu, tokens, kv, self.heads, dtype)

    def untouched(self):
        return all(torch.equal(self.dev[k], v) for k, v in self.kept.items()) and all(torch.equal(a.cpu(), b) for a, b in zip(self.kv, self.kv_cpu))


LAYER_ORDER = ("input_layernorm.weight", "input_layernorm.bias", "self_attn.qkv.weight", "self_attn.qkv.bias", "self_attn.o_proj.weight",
               "self_attn.o_proj.bias", "post_attention_layernorm.weight", "post_attention_layernorm.bias", "encoder_attn.q_proj.weight",
               "encoder_attn.q_proj.bias", "encoder_attn.o_proj.weight", "encoder_attn.o_proj.bias", "final_layernorm.weight",
               "final_layernorm.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


class State:
    """What one decode of model.rows rows owns: token slots 0 .. positions, cache rows 0 .. positions - 1 of every layer, the logits, the
    scratch and the flags, each in a flat buffer between GUARD sentinels."""

    def __init__(self, model, positions):
        m, dev = model, model.cuda
        self.model, self.positions = m, positions
        Rn = self.R = m.rows
        self.tok_stride = positions + 1 + 3
        self.cache_stride = (positions + 1) * 3 * m.d

        def buf(n, sentinel, dtype):
            return torch.full((2 * GUARD + n,), sentinel, dtype=dtype, device=dev)

        self.tok_flat = buf(Rn * self.tok_stride, TOK_SENTINEL, torch.int32)
        self.tokens = self.tok_flat[GUARD:GUARD + Rn * self.tok_stride].view(Rn, self.tok_stride)
        self.cache_flat = [buf(Rn * self.cache_stride, SENTINEL, torch.float32) for _ in range(m.layers)]
        self.cache = [f[GUARD:GUARD + Rn * self.cache_stride].view(Rn, positions + 1, 3 * m.d) for f in self.cache_flat]
        self.logits_flat = buf(Rn * m.vocab, SENTINEL, torch.float32)
        self.logits = self.logits_flat[GUARD:GUARD + Rn * m.vocab].view(Rn, m.vocab)
        self.scr_flat = buf(Rn * m.per_row, SENTINEL, torch.float32)
        self.scratch = self.scr_flat[GUARD:GUARD + Rn * m.per_row].view(Rn, m.per_row)
        self.fin_flat = buf(Rn, TOK_SENTINEL, torch.int32)
        self.finished = self.fin_flat[GUARD:GUARD + Rn]
        self.flats = [self.tok_flat, *self.cache_flat, self.logits_flat, self.scr_flat, self.fin_flat]
        owned = [self.tokens[:, :positions + 1], *[c[:, :positions] for c in self.cache], self.logits, self.scratch, self.finished]
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

    def desc(self, row0=0, rows=None, null_layer_ptr=None, odd_layer_ptr=None, **over):
        """The descriptor of rows row0 .. row0 + rows - 1 (default: all)."""
        m, L = self.model, _lib()
        n = L.S2S_PTRS_PER_LAYER
        ptrs = (ctypes.c_void_p * (m.layers * n))()
        for l in range(m.layers):
            for i, nm in enumerate(LAYER_ORDER):
                ptrs[l * n + i] = m.dev[f"layers.{l}.{nm}"].data_ptr()
            ptrs[l * n + 18] = self.cache[l][row0].data_ptr()
            ptrs[l * n + 19] = m.kv[l][row0].data_ptr()
        if null_layer_ptr is not None:
            ptrs[null_layer_ptr] = None
        if odd_layer_ptr is not None:
            ptrs[odd_layer_ptr] = ptrs[odd_layer_ptr] + 4
        self._keep = ptrs
        rows = self.R - row0 if rows is None else rows
        f = dict(d_model=m.d, heads=m.heads, d_ff=m.ff, vocab=m.vocab, layers=m.layers, n_enc=m.n_enc, max_positions=m.max_positions, rows=rows,
                 pad_id=PAD, eos_id=EOS, eps=R.EPS, embed=m.dev["embed_tokens.weight"].data_ptr(), pos_emb=m.dev["pos_emb.weight"].data_ptr(),
                 emb_ln_w=m.dev["embedding_layernorm.weight"].data_ptr(), emb_ln_b=m.dev["embedding_layernorm.bias"].data_ptr(),
                 norm_w=m.dev["norm.weight"].data_ptr(), norm_b=m.dev["norm.bias"].data_ptr(), head_w=m.dev["proj_out.weight"].data_ptr(),
                 head_b=m.dev["proj_out.bias"].data_ptr(), layer_ptrs=ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)),
                 tokens=self.tokens[row0].data_ptr(), finished=self.finished[row0:].data_ptr(), logits=self.logits[row0].data_ptr(),
                 scratch=self.scratch[row0].data_ptr(), scratch_floats=rows * m.per_row, token_stride=self.tok_stride,
                 cache_stride=self.cache_stride, cross_stride=m.n_enc * 2 * m.d)
        f.update(over)
        return L.Seq2SeqDesc(**f)

    def steps(self, t0, n, n_forced=0, **over):
        """The entry's return code."""
        return _lib().load().dyn_seq2seq_steps(ctypes.byref(self.desc(**over)), t0, n, n_forced, torch.cuda.current_stream().cuda_stream)

    def run(self, *a, **k):
        _lib().check(self.steps(*a, **k), "dyn_seq2seq_steps")


def _decode(st, first, S):
    """S greedy steps, one per call, from the start tokens `first` [R]: the logits of every step [R, S, V].  The id every step wrote is
    the first maximum of its own logits."""
    st.tokens[:, 0] = torch.as_tensor(first, dtype=torch.int32).to(st.tokens.device)
    out = []
    for t in range(S):
        st.run(t, 1)
        out.append(st.logits.clone())
        for r in range(st.R):
            assert int(st.tokens[r, t + 1]) == _first_max(out[-1][r]), f"step {t}, row {r}: the id written is not the first maximum of the logits"
    return torch.stack(out, 1)


def _starts(Rn, vocab, seed):
    return torch.randint(5, vocab, (Rn,), generator=R.gen(seed)).tolist()


def _parity(case, m, S, seed=0):
    """A fresh greedy decode of S steps against float64, teacher-forced on the tokens the kernel picked: the logits of every step and the
    cache rows of every layer, for every row."""
    st = State(m, S)
    got = _decode(st, _starts(m.rows, m.vocab, seed), S)
    toks = st.tokens[:, :S].cpu()
    want64, rows64, _ = m.ref(toks, F64)
    want32, rows32, _ = m.ref(toks, torch.float32)
    _close(case, "logits", got, want32, want64)
    for l in range(m.layers):
        _close(case, f"cache rows, layer {l}", st.cache[l][:, :S], rows32[l], rows64[l])
    assert not bool(st.finished.any())
    _exact(case, "nothing written outside the owned elements", st.outside_untouched())
    return st


# ----------------------------------------------------------------------------------------------------------- a. width edges
# (d_model, d_ff) at both ends of both ranges: 1 and 16 strips of 256 (1 .. 4 per wave), head dims 32 / 128 / 256, vocab 40 and 1030 (no
# multiple of the four output rows in flight); two layers on the small one reach the LayerNorm q | k | v launch that does not embed.
WIDTHS = [(256, 8, 256, 2, 40), (256, 1, 4096, 1, 1030), (1024, 8, 512, 1, 40), (1024, 8, 4096, 1, 1030), (1024, 4, 4096, 1, 40), (768, 6, 1280, 1, 40)]


@pytest.mark.parametrize("d,heads,ff,layers,vocab", WIDTHS)
def test_width_edges(cuda, d, heads, ff, layers, vocab):
    print()
    m = Model(cuda, d, heads, ff, layers=layers, vocab=vocab, n_enc=9, rows=3, seed=d // 256 + ff // 256)
    _parity(f"widths d={d} H={heads} hd={d // heads} ff={ff} L={layers} V={vocab}", m, 3)


# ----------------------------------------------------------------------------------------------------------- b. row edges
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 8])
def test_row_edges(cuda, rows):
    """Both sides of the row-block instances (1, 4 and 8 rows held per workgroup)."""
    print()
    m = Model(cuda, 256, 2, 512, layers=2, vocab=40, n_enc=9, rows=rows, seed=rows)
    _parity(f"rows R={rows}", m, 3, seed=rows)


# ----------------------------------------------------------------------------------------------------------- c. key edges
@pytest.mark.parametrize("n_enc", [1, 9, 4 * 64 + 1])
def test_key_edges(cuda, n_enc):
    """t + 1 = 1 .. 9 self-attention keys (1, 4, 5, and 8 -> 9 where every key split grows to a third key); n_enc = 1 (three empty
    splits), 9, and one above 4 x 64 (the second pass of the score loop)."""
    print()
    m = Model(cuda, 256, 8, 256, layers=1, vocab=40, n_enc=n_enc, rows=2, seed=n_enc)
    _parity(f"keys n_enc={n_enc} t+1=1..9", m, 9, seed=n_enc)


# ----------------------------------------------------------------------------------------------------------- d. the layer-0 prologue
def test_residual_stream_after_the_layer0_prologue(cuda):
    """With o_proj, the cross o_proj and fc2 zeroed (weights and biases) no block adds to the residual stream: after a step the scratch's
    first d floats of a row ARE embedding_layernorm(embed[token] + pos_emb[t]), written once by the layer-0 prologue."""
    print()

    def edit(p):
        for n in ("self_attn.o_proj", "encoder_attn.o_proj", "mlp.fc2"):
            p[f"layers.0.{n}.weight"].zero_()
            p[f"layers.0.{n}.bias"].zero_()
    for d, ff in ((256, 256), (1024, 4096)):
        m = Model(cuda, d, 8, ff, layers=1, vocab=40, n_enc=9, rows=5, seed=d, edit=edit)
        st = State(m, 3)
        st.tokens[:, 0] = torch.tensor(_starts(5, 40, d), dtype=torch.int32).to(cuda)
        for t in range(3):
            st.run(t, 1)
            toks = st.tokens[:, :t + 1].cpu()
            _close(f"prologue d={d} t={t}", "residual stream", st.scratch[:, :d], m.ref(toks, torch.float32)[2][:, t], m.ref(toks, F64)[2][:, t])
        _exact(f"prologue d={d}", "nothing written outside the owned elements", st.outside_untouched())


# ----------------------------------------------------------------------------------------------------------- e. row independence
@pytest.mark.parametrize("rows", [5, 8])
def test_a_row_does_not_depend_on_its_neighbours(cuda, rows):
    """Row r of an R-row call is bit-equal to the same row decoded alone (the one-row instance): logits of every step, tokens, cache rows."""
    print()
    S = 4
    m = Model(cuda, 1024, 8, 512, layers=2, vocab=1030, n_enc=9, rows=rows, seed=rows)
    starts = _starts(rows, 1030, rows)
    st = State(m, S)
    got = _decode(st, starts, S)
    for r in sorted({0, 3, 4, rows - 1}):
        one = Model(cuda, 1024, 8, 512, layers=2, vocab=1030, n_enc=9, rows=1, seed=rows)
        one.kv_cpu = [t[r:r + 1].clone() for t in m.kv_cpu]
        one.kv = [t.to(cuda) for t in one.kv_cpu]
        s1 = State(one, S)
        alone = _decode(s1, starts[r:r + 1], S)
        ok = _same_bits(alone[0], got[r]) and torch.equal(s1.tokens[0, :S + 1], st.tokens[r, :S + 1]) and \
            all(_same_bits(s1.cache[l][0, :S], st.cache[l][r, :S]) for l in range(2))
        _exact(f"independence R={rows}", f"row {r} alone", ok)
    _exact(f"independence R={rows}", "nothing written outside the owned elements", st.outside_untouched())


# ----------------------------------------------------------------------------------------------------------- f. call splitting
def test_one_call_of_n_steps_equals_calls_of_1_and_3(cuda):
    print()
    m = Model(cuda, 256, 2, 512, layers=2, vocab=40, n_enc=9, rows=5, seed=11)
    a, b = State(m, 4), State(m, 4)
    for st in (a, b):
        st.tokens[:, 0] = torch.tensor(_starts(5, 40, 11), dtype=torch.int32).to(cuda)
    a.run(0, 4)
    b.run(0, 1)
    b.run(1, 3)
    _exact("splitting", "tokens, caches, logits, scratch, flags", all(_same_bits(x, y) for x, y in zip(a.flats, b.flats)))
    toks = a.tokens[:, :4].cpu()
    _close("splitting", "logits of the last step", a.logits, m.ref(toks, torch.float32)[0][:, 3], m.ref(toks, F64)[0][:, 3])
    _exact("splitting", "nothing written outside the owned elements", a.outside_untouched() and b.outside_untouched())


# ----------------------------------------------------------------------------------------------------------- g. retiring
def test_a_row_that_picks_eos_retires(cuda):
    """Zero head weight: the logits ARE the head bias, so the bias scripts the pick.  Steps 0 - 1: every row picks 7.  Step 2: rows 0 - 1
    (their own descriptor) pick eos, rows 2 - 4 pick 9.  Steps 3 - 5: rows 0 - 1 write no cache row and receive pad in every slot, rows
    2 - 4 carry on; against a control decode in which nobody retires, rows 2 - 4 keep every bit."""
    print()

    def edit(p):
        p["proj_out.weight"].zero_()
    Rn, S = 5, 6
    m = Model(cuda, 256, 2, 512, layers=2, vocab=40, n_enc=9, rows=Rn, seed=4, edit=edit)

    def bias(best):
        b = torch.zeros(40)
        b[best] = 5.0
        return b

    def run(retire):
        st = State(m, S)
        st.tokens[:, 0] = torch.tensor(_starts(Rn, 40, 4), dtype=torch.int32).to(cuda)
        m.set_head_bias(bias(7))
        st.run(0, 2)
        m.set_head_bias(bias(EOS if retire else 9))
        st.run(2, 1, row0=0, rows=2)
        m.set_head_bias(bias(9))
        st.run(2, 1, row0=2)
        st.run(3, 3)
        return st
    st, ctl = run(True), run(False)
    assert st.finished.tolist() == [1, 1, 0, 0, 0] and ctl.finished.tolist() == [0] * Rn
    assert st.tokens[:2, 1:S + 1].tolist() == [[7, 7, EOS, PAD, PAD, PAD]] * 2
    assert st.tokens[2:, 1:S + 1].tolist() == [[7, 7, 9, 9, 9, 9]] * 3
    for l in range(2):
        assert not bool(st.cache[l][:2, :3].isnan().any()) and bool(st.cache[l][:2, 3:S].isnan().all()), "a retired row wrote a cache row"
    same = torch.equal(st.tokens[2:], ctl.tokens[2:]) and _same_bits(st.logits[2:], ctl.logits[2:]) and _same_bits(st.scratch[2:], ctl.scratch[2:]) \
        and all(_same_bits(st.cache[l][2:], ctl.cache[l][2:]) for l in range(2))
    _exact("retiring", "the live rows next to retired ones", same)
    _exact("retiring", "nothing written outside the owned elements", st.outside_untouched())
    snap = st.snapshot()                                         # every row finished on entry: nothing but pad in the next slot
    st.finished.fill_(1)
    snap[-1] = st.fin_flat.clone()
    want_tokens = st.tokens.clone()
    want_tokens[:, 6] = PAD
    st.run(5, 1)
    assert torch.equal(st.tokens, want_tokens) and all(_same_bits(f, s) for f, s in list(zip(st.flats, snap))[1:])


# ----------------------------------------------------------------------------------------------------------- h. forced prompt
def test_forced_prompt_slots_keep_their_bits(cuda):
    """n_forced = 3: slots 1 .. 2 hold the prompt and keep it, the head runs first at t = 2 and slot 3 is its pick; caches and the logits
    equal, bit for bit, a free decode that happened to see the same tokens."""
    print()
    m = Model(cuda, 256, 2, 512, layers=2, vocab=40, n_enc=9, rows=3, seed=6)
    st = State(m, 4)
    prompt = torch.tensor([[4, 17, 30], [4, 21, 8], [4, 33, 12]], dtype=torch.int32)
    st.tokens[:, :3] = prompt.to(cuda)
    st.run(0, 2, n_forced=3)
    _exact("forced", "the logits were not written before the prompt's last position", bool(st.logits.isnan().all()))
    st.run(2, 2, n_forced=3)
    assert torch.equal(st.tokens[:, :3].cpu(), prompt)
    free = State(m, 4)
    free.tokens[:, 0] = prompt[:, 0].to(cuda)
    for t in range(4):
        free.run(t, 1)
        if t < 2:
            free.tokens[:, t + 1] = prompt[:, t + 1].to(cuda)
    _exact("forced", "tokens, caches, logits against the free decode", torch.equal(st.tokens, free.tokens) and _same_bits(st.logits, free.logits) and
           all(_same_bits(a, b) for a, b in zip(st.cache, free.cache)))
    toks = st.tokens[:, :4].cpu()
    want64, want32 = m.ref(toks, F64)[0], m.ref(toks, torch.float32)[0]
    _close("forced", "logits of the last step", st.logits, want32[:, 3], want64[:, 3])
    for r in range(3):
        assert int(st.tokens[r, 3]) == int(want64[r, 2].argmax())
    _exact("forced", "nothing written outside the owned elements", st.outside_untouched())


# ----------------------------------------------------------------------------------------------------------- i. host guards
GUARDS = [
    ("d_model 320", dict(d_model=320), E_UNSUPPORTED), ("d_model 4352", dict(d_model=4352, heads=17), E_UNSUPPORTED),
    ("d_ff 1000", dict(d_ff=1000), E_UNSUPPORTED), ("d_ff 4352", dict(d_ff=4352), E_UNSUPPORTED),
    ("head dim 192", dict(d_model=768, heads=4), E_UNSUPPORTED), ("head dim 512", dict(d_model=512, heads=1), E_UNSUPPORTED),
    ("heads do not divide", dict(heads=3), E_ARG), ("rows 0", dict(rows=0), E_ARG), ("rows 9", dict(rows=9), E_ARG),
    ("vocab 0", dict(vocab=0), E_ARG), ("layers 0", dict(layers=0), E_ARG), ("n_enc 0", dict(n_enc=0), E_ARG),
    ("eos outside", dict(eos_id=40), E_ARG), ("pad outside", dict(pad_id=-1), E_ARG),
    ("null embed", dict(embed=None), E_ARG), ("null tokens", dict(tokens=None), E_ARG), ("null finished", dict(finished=None), E_ARG),
    ("null logits", dict(logits=None), E_ARG), ("null scratch", dict(scratch=None), E_ARG), ("null head bias", dict(head_b=None), E_ARG),
    ("null layer pointer", dict(null_layer_ptr=21), E_ARG), ("misaligned layer pointer", dict(odd_layer_ptr=4), E_ARG),
    ("scratch one float short", dict(scratch_floats=-1), E_WORKSPACE), ("token_stride", dict(token_stride=4), E_ARG),
    ("cache_stride short", dict(cache_stride=4 * 3 * 256 - 4), E_ARG), ("cache_stride odd", dict(cache_stride=5 * 3 * 256 + 2), E_ARG),
    ("cross_stride short", dict(cross_stride=9 * 512 - 4), E_ARG), ("cross_stride odd", dict(cross_stride=9 * 512 + 2), E_ARG),
    ("max_positions", dict(max_positions=3), E_ARG),
]


def test_host_guards_return_their_code_and_launch_nothing(cuda):
    print()
    m = Model(cuda, 256, 2, 512, layers=2, vocab=40, n_enc=9, rows=3, seed=1)
    st = State(m, 4)
    st.tokens[:, 0] = 5
    snap = st.snapshot()
    lib = _lib().load()
    for name, over, code in GUARDS:
        if over.get("scratch_floats") == -1:
            over = dict(scratch_floats=3 * m.per_row - 1)
        rc = st.steps(0, 4, **over)
        torch.cuda.synchronize()
        print(f"  guard {name}: code {rc}")
        assert rc == code, (name, rc, lib.dyn_last_error())
        assert st.unchanged_since(snap) and m.untouched(), name
    for name, args in (("negative t0", (-1, 1, 0)), ("negative n_steps", (0, -1, 0)), ("negative n_forced", (0, 1, -1)),
                       ("past max_positions", (10, 3, 0))):
        rc = lib.dyn_seq2seq_steps(ctypes.byref(st.desc()), *args, torch.cuda.current_stream().cuda_stream)
        print(f"  guard {name}: code {rc}")
        assert rc == E_ARG and st.unchanged_since(snap), name
    assert lib.dyn_seq2seq_steps(None, 0, 1, 0, torch.cuda.current_stream().cuda_stream) == E_ARG
    assert lib.dyn_seq2seq_row_scratch_floats(256, 512, 3) == -1 and lib.dyn_seq2seq_row_scratch_floats(0, 512, 2) == -1
    assert st.steps(0, 0) == OK and st.unchanged_since(snap)          # no steps: nothing to do
    st.run(0, 4)                                                      # and the state is a working one
    assert not bool(st.logits.isnan().any())
