"""Cache-aware chunk-by-chunk streaming of NemotronAsrStreamingForRNNT (nemotron_asr_streaming_model.py): what transformers does with
`encoder(..., use_cache=True, past_key_values=..., padding_cache=...)` and its streaming `generate`, as a SESSION that owns every piece
of state on the device, allocated once: `model.stream(batch_size, num_lookahead_tokens=None, graph=False)`.

The chunked limited-context mask of the offline encode is what makes this equal to it: with cs = lookahead + 1 and
lc = (sliding_window - 1) // cs, the cs frames of a chunk see the min(chunks so far, lc) * cs cached frames and themselves, all of them
the same keys, so a step has no per-row mask.  Geometry (ops.stream_geometry): the first chunk carries 1 + 8 * lookahead feature frames,
every later one 8 * (lookahead + 1); both give cs encoder frames; any other length is an error (the caller pads a short last chunk).

State of a session (B streams, L layers, hidden H, C subsampling channels, F mel bins, F1 / F2 the widths after one / two stages):
  k / v caches     [L, B, lc + 1, cs, H] each: a RING of chunk slots, never moved (csrc/stream.hip says why lc + 1)
  conv states      [L, 2, B, 8, H]: the last 8 GLU frames per layer, double buffered on the chunk counter's parity
  carries          [2, B, F], [2, B, F1, C], [2, B, F2, C]: the last input row of each subsampling stage (before the ReLU), double buffered
  position rows    [L, W, H]: relative_k_proj of the W = lc cs + 2 cs - 1 sinusoid rows, projected once per session and layer
  counter          int32 [1] on the device: chunks consumed; every streaming kernel reads slot, warm-up count and state half from it
  greedy state     ops.RnntGreedyState for max_symbols_per_step * cs outputs per chunk
A step is: three subsampling stages (streamed kernels) with their two pointwise GEMMs, ReLU, the linear; per layer 19 launches (the
offline layer's 24: the six launches between the q | k | v product and the output product are ONE, ops.stream_attn); the projector; the
counter's advance.  With graph=True the steady-state step (everything from the subsampling to the advance: one linear chain on one stream)
is captured once through _graphs.capture and replayed per chunk; the first chunk has other shapes and the second warms the kernels, both
run eagerly.  The decode stays eager: ops.rnnt_greedy_steps_chunk, one host read per `greedy_chunk` steps.

Refused by name before any launch: `sliding_window` < 0 (unlimited left context: the cache would have no bound), lc cs + cs >
`max_position_embeddings`, a TDT head, `attention_mask`, a chunk whose batch differs from the session's (rows cannot join or leave),
a chunk of the wrong length, and model.backward() after a push (everything here runs under no_grad)."""
from types import SimpleNamespace

import torch

from . import _graphs, ops
from . import parakeet_tdt_model as TM

SUB = "encoder.subsampling."


class StreamSession:
    def __init__(self, model, batch_size, num_lookahead_tokens=None, graph=False):
        from .nemotron_asr_streaming_model import check_lookahead
        c = model.cfg
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ops.DynError(f"stream(batch_size={batch_size!r}): a positive integer number of streams")
        if len(c["durations"]):
            raise ops.DynError("stream(): a TDT head (durations) is not built for streaming, only the RNN-T greedy decode")
        if c["sliding_window"] < 0:
            raise ops.DynError(f"stream(): sliding_window={c['sliding_window']} leaves the left context unlimited, so the K/V cache would have "
                               "no bound: streaming needs a positive sliding_window")
        R = c["default_num_lookahead_tokens"] if num_lookahead_tokens is None else check_lookahead(num_lookahead_tokens)
        geo = ops.stream_geometry(c["sliding_window"], R)
        if geo.NK > c["max_position_embeddings"]:
            raise ops.DynError(f"stream(): {geo.lc * geo.cs} cached + {geo.cs} new frames exceed max_position_embeddings="
                               f"{c['max_position_embeddings']}")
        H, nh = c["hidden_size"], c["num_attention_heads"]
        lds = ops._L().dyn_stream_attn_lds_bytes(geo.cs, geo.lc, H // nh)
        if lds < 0 or lds > 160 * 1024:
            raise ops.DynError(f"stream(): sliding_window={c['sliding_window']} with lookahead {R} at head width {H // nh} needs {lds} B of LDS "
                               "per workgroup in the attention step, more than the 160 KiB of a CU")
        self.model, self.B, self.lookahead, self.geo, self.graph = model, batch_size, R, geo, bool(graph)
        self.first_chunk_frames, self.chunk_frames = geo.first_frames, geo.frames
        dev, L, C, F = model.device, c["num_hidden_layers"], c["subsampling_conv_channels"], c["num_mel_bins"]
        F1, F2 = ops.causal_out_len(F), ops.causal_out_len(ops.causal_out_len(F))
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)        # noqa: E731
        B = batch_size
        self.k_cache, self.v_cache = z(L, B, geo.slots, geo.cs, H), z(L, B, geo.slots, geo.cs, H)
        self.conv_state = z(L, 2, B, 8, H)
        self.carries = (z(2, B, F), z(2, B, F1, C), z(2, B, F2, C))
        self.counter = torch.zeros(1, device=dev, dtype=torch.int32)
        self.valid = torch.full((B,), geo.cs, device=dev, dtype=torch.int32)
        self.cap = c["max_symbols_per_step"] * geo.cs
        self.greedy = model._greedy_state(B, self.cap)
        self._chunks = 0
        self._graph = self._pool = self._static_in = self._static_out = None
        self._audio, self._pending, self._flushed = None, None, False     # push_audio()'s state, built at its first call
        with torch.no_grad(), ops.use_workspace(model._scratch()):
            tab = ops.stream_position_rows(geo, H).to(dev)
            self.pos = torch.stack([ops.linear(tab, model.P[f"encoder.layers.{l}.self_attn.linear_pos.weight"]) for l in range(L)])

    # ------------------------------------------------------------------ bookkeeping
    @property
    def frames_seen(self):
        """Encoder frames consumed so far."""
        return self._chunks * self.geo.cs

    def state_bytes(self):
        ts = (self.k_cache, self.v_cache, self.conv_state, *self.carries, self.pos, self.counter)
        return sum(t.numel() * t.element_size() for t in ts)

    def reset(self):
        """Back to the start of a stream: caches, states, carries, the counter and the greedy state cleared in place (a captured step stays
        valid: it holds their addresses)."""
        for t in (self.k_cache, self.v_cache, self.conv_state, *self.carries, self.counter):
            t.zero_()
        g = self.greedy
        for t in (g.istate, g.h, g.c, g.h_new, g.dec, g.logits, g.tokens, g.frames):
            t.zero_()
        g.istate[1] = int(self.model.start_token)
        g.istate[2] = 1
        self._chunks = 0
        if self._audio is not None:                            # the audio tail, the previous samples and the frames waiting for a chunk
            self._audio.reset()
            self._pending = self._pending[:, :0]
        self._flushed = False

    def close(self):
        """Drops the captured step (never while a replay may be in flight)."""
        if self._graph is not None:
            torch.cuda.synchronize(self.model.device)
            self._graph = self._static_in = self._static_out = self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_chunk(self, feats, attention_mask):
        if attention_mask is not None:
            raise ops.DynError("attention_mask is not built for a streaming session: every frame of a chunk is taken as valid (ragged batches "
                               "are out of scope)")
        F = self.model.cfg["num_mel_bins"]
        if not (isinstance(feats, torch.Tensor) and feats.dtype == torch.float32 and feats.dim() == 3 and feats.shape[2] == F):
            raise ops.DynError(f"a chunk must be a float32 CUDA tensor [{self.B}, frames, {F}]")
        if feats.shape[0] != self.B:
            raise ops.DynError(f"a chunk of {feats.shape[0]} rows in a session of batch_size={self.B}: rows cannot join or leave a running session")
        first = self._chunks == 0
        need = self.first_chunk_frames if first else self.chunk_frames
        if feats.shape[1] != need:
            raise ops.DynError(f"the {'first' if first else 'next'} chunk has {feats.shape[1]} feature frames, but num_lookahead_tokens="
                               f"{self.lookahead} needs exactly {need} (first chunk {self.first_chunk_frames} = 1 + 8 * lookahead, every later "
                               f"chunk {self.chunk_frames} = 8 * (lookahead + 1)): pad a short last chunk to {need} frames")
        if not feats.is_cuda:
            raise ops.DynError("a chunk must be a CUDA tensor (the HIP path has no CPU fallback)")
        return first

    # ------------------------------------------------------------------ one step
    def _step(self, x, first):
        """x [B, n, F] -> the projected encoder states [B, cs, Hd]; advances the device counter."""
        m, geo, cnt = self.model, self.geo, self.counter
        P, c = m.P, m.cfg
        c0, c1, c2 = self.carries
        z1 = ops.stream_conv2d_first(x, P[SUB + "conv_in.weight"], P[SUB + "conv_in.bias"], c0, cnt, first)
        u2 = ops.stream_dwconv2d_s2_act(z1, P[SUB + "layers.0.depthwise_conv.weight"], P[SUB + "layers.0.depthwise_conv.bias"], c1, cnt, "relu", first)
        z2 = ops.linear(u2, P[SUB + "layers.0.pointwise_conv.weight"], P[SUB + "layers.0.pointwise_conv.bias"])
        u3 = ops.stream_dwconv2d_s2_act(z2, P[SUB + "layers.1.depthwise_conv.weight"], P[SUB + "layers.1.depthwise_conv.bias"], c2, cnt, "relu", first)
        z3 = ops.linear(u3, P[SUB + "layers.1.pointwise_conv.weight"], P[SUB + "layers.1.pointwise_conv.bias"])
        a3 = ops.relu(z3)
        B, T3, F3, C = a3.shape
        if T3 != geo.cs:
            raise ops.DynError(f"the subsampling gave {T3} frames for a chunk of {geo.cs}")
        x = ops.linear(a3.view(B, T3, F3 * C), P[SUB + "linear.weight"], P[SUB + "linear.bias"])
        if m.input_scale != 1.0:
            raw, x = x, x.clone()                              # as the offline _subsample scales it: the same rounding
            ops.axpby(raw, x, 0.0, m.input_scale)
        H, nh = c["hidden_size"], c["num_attention_heads"]
        for l in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{l}."
            x, _ = m._ffn_fwd(x, p, "ffn1", False)
            n, _, _ = ops.layernorm(x, P[p + "self_attn_layer_norm.weight"], P[p + "self_attn_layer_norm.bias"], m._layer_eps)
            Wqkv, bqkv = m.Pqkv[l]
            qkv = ops.linear(n, Wqkv, bqkv)
            o = ops.stream_attn(qkv, P[p + "self_attn.pos_bias_u"], P[p + "self_attn.pos_bias_v"], self.pos[l], self.k_cache[l], self.v_cache[l],
                                cnt, nh, geo.lc)
            ops.linear(o, P[p + "self_attn.linear_out.weight"], P[p + "self_attn.linear_out.bias"], out=x, beta=1.0)
            (ln, pw1, dw, dln, pw2) = m._causal_conv_spec(l)[0]
            n, _, _ = ops.layernorm(x, P[ln + ".weight"], P[ln + ".bias"], m._layer_eps)
            u = ops.linear(n, P[pw1 + ".weight"], P.get(pw1 + ".bias"))
            a = ops.stream_convmod_k9(u, P[dw + ".weight"], P.get(dw + ".bias"), P[dln + ".weight"], P[dln + ".bias"], self.conv_state[l], cnt,
                                      m._layer_eps)
            ops.linear(a, P[pw2 + ".weight"], P.get(pw2 + ".bias"), out=x, beta=1.0)
            x, _ = m._ffn_fwd(x, p, "ffn2", False)
            x, _, _ = ops.layernorm(x, P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"], m._layer_eps)
        enc = self._project(x)
        ops.stream_advance(cnt)
        return enc

    def _project(self, x):
        """The chunk's last hidden states -> the projected states: the model's _project_enc (a session with state of its own between the
        encoder and the projector overrides this)."""
        return self.model._project_enc(x, False)[0]

    def _encode(self, feats, attention_mask=None, input_lengths=None):
        """The step of one chunk -> enc [B, cs, Hd]; under graph=True the captured step's own output buffer (valid until the next chunk)."""
        if input_lengths is not None:
            raise ops.DynError("input_lengths is not built for a streaming session: every frame of a chunk is taken as valid")
        first = self._check_chunk(feats, attention_mask)
        m = self.model
        m._ctx = m._tdt = m._ctx_lookahead = None
        m._after_stream = True
        with torch.no_grad(), ops.use_workspace(m._scratch()):
            if self.graph and self._chunks >= 2:
                if self._graph is None:
                    if self._pool is None:
                        self._pool = torch.cuda.graph_pool_handle()
                    self._static_in = torch.zeros(self.B, self.chunk_frames, feats.shape[2], device=m.device, dtype=torch.float32)
                    self._graph, self._static_out = _graphs.capture(self._pool, lambda: self._step(self._static_in, False))
                self._static_in.copy_(feats)
                self._graph.replay()
                enc = self._static_out
            else:
                enc = self._step(feats.contiguous(), first)
        self._chunks += 1
        return enc

    # ------------------------------------------------------------------ the public calls
    def encode_chunk(self, feats, attention_mask=None, input_lengths=None):
        """feats [B, first_chunk_frames | chunk_frames, num_mel_bins] -> the projected encoder states [B, cs, Hd] of the chunk."""
        enc = self._encode(feats, attention_mask, input_lengths)
        return enc.clone() if enc is self._static_out else enc

    def push(self, feats, attention_mask=None, input_lengths=None):
        """encode_chunk + the greedy RNN-T decode of the chunk's cs frames, the decoder's state carried over from the chunk before ->
        SimpleNamespace(enc [B, cs, Hd], tokens int32 [B, max_symbols_per_step * cs], frames (absolute encoder frames), count int32 [B],
        steps int32 [B]), all of this chunk."""
        base = self.frames_seen
        enc = self._encode(feats, attention_mask, input_lengths)
        m, st, P = self.model, self.greedy, self.model.P
        DEC, JOINT = TM.DEC, TM.JOINT
        with torch.no_grad():
            done, rebase = 0, True
            while done < self.cap:
                n = min(m.greedy_chunk, self.cap - done)
                ops.rnnt_greedy_steps_chunk(enc, self.valid, P[DEC + "embedding.weight"], m._lstm_ptrs, P[DEC + "decoder_projector.weight"],
                                            P[DEC + "decoder_projector.bias"], P[JOINT + "head.weight"], P[JOINT + "head.bias"], st, m.blank,
                                            m.cfg["max_symbols_per_step"], self.cap, n, base, rebase)
                done, rebase = done + n, False
                if bool(st.istate[3].all()):             # the one host read of the chunk
                    break
        return SimpleNamespace(enc=enc.clone() if enc is self._static_out else enc, tokens=st.tokens.clone(), frames=st.frames.clone(),
                               count=st.istate[4].clone(), steps=st.istate[5].clone())

    # ------------------------------------------------------------------ audio in (frontend.MelStream, csrc/melfeat.hip)
    def _audio_state(self):
        if self._audio is None:
            from .frontend import MelStream
            self._audio = MelStream(self.model.feature_extractor(), self.B)
            self._pending = torch.zeros(self.B, 0, self.model.cfg["num_mel_bins"], device=self.model.device, dtype=torch.float32)
        return self._audio

    def _push_ready(self, new, pad_last=False):
        """Appends the extracted frames `new` ([B, n, F] or None) and pushes every complete chunk; `pad_last`: a started last chunk is
        filled up with zero frames.  The result of a chunk carries the feature frames it was fed as `features`."""
        if new is not None:
            self._pending = torch.cat([self._pending, new], dim=1)
        outs = []
        while True:
            need = self.first_chunk_frames if self._chunks == 0 else self.chunk_frames
            have = self._pending.shape[1]
            if have < need and not (pad_last and have > 0):
                return outs
            chunk = self._pending[:, :need]
            if have < need:
                chunk = torch.nn.functional.pad(chunk, (0, 0, 0, need - have))
            chunk, self._pending = chunk.contiguous(), self._pending[:, need:]
            out = self.push(chunk)
            out.features = chunk
            outs.append(out)

    def push_audio(self, samples):
        """samples [B, n] float32 on the device, any n >= 0 (16 kHz mono; all streams advance together) -> the list of push() results of
        the chunks these samples completed, possibly empty.  Feature frame t is extracted as soon as the samples below 160 t + 200 have
        arrived; the extraction runs eagerly in front of the (possibly captured) encoder step."""
        if self._flushed:
            raise ops.DynError("push_audio after flush(): the stream has ended; reset() starts the next one")
        return self._push_ready(self._audio_state().push(samples))

    def flush(self):
        """Ends the audio stream: the frames below total_samples // 160 that were still waiting for samples are extracted with zeros behind
        the last sample; frame total_samples // 160, which the offline extractor emits and masks, follows as zeros, so the stream's
        features are the offline pass's 1 + total_samples // 160 frames; the last chunk is filled up with zero frames -> the remaining
        push() results.  The session then stands at the end of its stream: reset() starts the next one."""
        a = self._audio_state()
        if a.total == 0 or self._flushed:
            return []
        new, last = a.finish(), self._pending.new_zeros(self.B, 1, self._pending.shape[2])
        self._flushed = True
        return self._push_ready(last if new is None else torch.cat([new, last], dim=1), pad_last=True)


def split_chunks(session, input_features):
    """[B, T, F] -> the list of a stream's chunks; T must be first_chunk_frames + k * chunk_frames."""
    T, a, b = input_features.shape[1], session.first_chunk_frames, session.chunk_frames
    if T < a or (T - a) % b:
        short = a - T if T < a else b - (T - a) % b
        raise ops.DynError(f"{T} feature frames are not a whole stream at num_lookahead_tokens={session.lookahead}: the first chunk has {a} "
                           f"frames and every later one {b}; pad the features by {short} frames")
    return [input_features[:, :a]] + [input_features[:, s:s + b] for s in range(a, T, b)]


def generate_streaming(model, input_features, num_lookahead_tokens=None, graph=False, **session_kw):
    """The greedy decode of a whole stream, chunk by chunk: `input_features` [B, T, F] (T = first_chunk_frames + k * chunk_frames) or an
    iterable of chunks, or 16 kHz mono waveforms [B, L] (push_audio + flush) -> generate()'s fields, concatenated over the chunks (frames are absolute encoder frames).  `session_kw`: what
    the model's stream() takes beyond these (nemotron3_5_asr_model.py: prompt_ids)."""
    chunks = input_features
    outs = None
    if isinstance(input_features, torch.Tensor) and input_features.dim() == 2:        # waveforms [B, L]: the session extracts the features
        if input_features.shape[1] < 160:
            raise ops.DynError(f"generate_streaming: {input_features.shape[1]} samples give no valid feature frame (160 samples, one hop, are "
                               "the shortest stream)")
        session = model.stream(input_features.shape[0], num_lookahead_tokens, graph, **session_kw)
        outs = session.push_audio(input_features.contiguous()) + session.flush()
    elif isinstance(input_features, torch.Tensor):
        if input_features.dim() != 3:
            raise ops.DynError("generate_streaming: input_features must be [B, T, num_mel_bins], waveforms [B, L] or an iterable of chunks")
        session = model.stream(input_features.shape[0], num_lookahead_tokens, graph, **session_kw)
        chunks = split_chunks(session, input_features)
    else:
        chunks = list(chunks)
        if not chunks or not isinstance(chunks[0], torch.Tensor) or chunks[0].dim() != 3:
            raise ops.DynError("generate_streaming: input_features must be [B, T, num_mel_bins] or an iterable of chunks [B, frames, num_mel_bins]")
        session = model.stream(chunks[0].shape[0], num_lookahead_tokens, graph, **session_kw)
    if outs is None:
        outs = [session.push(ch) for ch in chunks]
    session.close()
    B, n_max, dev = session.B, session.cap, model.device
    tokens = torch.zeros(B, n_max * len(outs), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(tokens)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    steps = torch.zeros(B, dtype=torch.int32, device=dev)
    col = torch.arange(n_max, device=dev)[None, :]
    row = torch.arange(B, device=dev)[:, None].expand(B, n_max)
    for o in outs:
        keep = col < o.count[:, None]
        at = (count[:, None] + col).long()
        tokens[row[keep], at[keep]] = o.tokens[keep]
        frames[row[keep], at[keep]] = o.frames[keep]
        count += o.count
        steps += o.steps
    return SimpleNamespace(tokens=tokens, frames=frames, count=count, steps=steps)
