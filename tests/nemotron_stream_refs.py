"""References for the streaming tests of NemotronAsrStreamingForRNNT, plain torch in the dtype of their inputs (float64: the reference;
float32: the yardstick of kernel_refs.measured_tol): one subsampling stage with its carried row, the conv-module core with its carried
GLU frames, one attention step written from the mask formula on ABSOLUTE positions against the full key history, and the chunk-by-chunk
drive of transformers' encoder with its own caches."""
import torch
import torch.nn.functional as Fn


def geometry(sliding_window, lookahead):
    """(cs, lc, first chunk's feature frames, every later chunk's) of a stream."""
    cs = lookahead + 1
    return cs, (sliding_window - 1) // cs, 1 + 8 * lookahead, 8 * cs


def stage_len(n, first):
    """Output rows of a streamed stage on n input rows: left context 1 (first chunk: 2), no right padding, kernel 3, stride 2."""
    return (n + (2 if first else 1) - 3) // 2 + 1


def chunks_of(x, sliding_window, lookahead):
    """x [B, T, F] with T = first + k * per -> the list of chunks."""
    _, _, first, per = geometry(sliding_window, lookahead)
    T = x.shape[1]
    assert T >= first and (T - first) % per == 0, (T, first, per)
    return [x[:, :first]] + [x[:, s:s + per] for s in range(first, T, per)]


# ----------------------------------------------------------------------------------------------------------- subsampling stages
def stream_stage(chunk, carry, w, bias, first, stem):
    """One streamed stage.  chunk [B, n, F] (stem) or [B, n, F, C] (depthwise: the rows BEFORE the ReLU); carry: the last row of the chunk
    before, [B, F] / [B, F, C] (ignored on the first chunk, where two zero rows stand in).  Frequency is padded (2, 1), time only by the
    left context.  Returns (output channels-last [B, stage_len(n, first), F // 2 + 1, C], the new carry)."""
    left = torch.zeros_like(chunk[:, :2]) if first else carry[:, None]
    rows = torch.cat([left, chunk], 1)
    if stem:
        y = Fn.conv2d(Fn.pad(rows[:, None], (2, 1)), w[:, None], bias, stride=2)
    else:
        y = Fn.conv2d(Fn.pad(torch.relu(rows).permute(0, 3, 1, 2), (2, 1)), w[:, None], bias, stride=2, groups=w.shape[0])
    return y.permute(0, 2, 3, 1), chunk[:, -1].clone()


# ----------------------------------------------------------------------------------------------------------- conv-module core
def stream_convmod(u, state, w, cbias, gamma, beta, eps=1e-5):
    """u [B, T, 2C], state [B, KW - 1, C] (the GLU frames left of the chunk) -> (silu(LayerNorm(cbias + conv(state | GLU(u)))) [B, T, C],
    the new state: the last KW - 1 frames of state | GLU(u), whatever T is)."""
    C, KW = w.shape
    full = torch.cat([state, Fn.glu(u, dim=-1)], 1)
    c = Fn.conv1d(full.transpose(1, 2), w[:, None], cbias, groups=C).transpose(1, 2)
    return Fn.silu(Fn.layer_norm(c, (C,), gamma, beta, eps)), full[:, -(KW - 1):].clone()


# ----------------------------------------------------------------------------------------------------------- attention step
def attn_step(qkv, k_hist, v_hist, bias_u, bias_v, pos, cs, lc, nh):
    """The chunk's context [B, cs, H] from the mask formula on absolute positions.  qkv [B, cs, 3H] of the chunk; k_hist / v_hist
    [B, t0, H]: EVERY earlier frame's key / value (t0 = chunks so far * cs); pos [W, H]: the projected position rows of the distances
    lc cs + cs - 1 .. -(cs - 1).  Query t0 + i sees key j iff 0 <= (t0 + i) // cs - j // cs <= lc."""
    B, _, H3 = qkv.shape
    H = H3 // 3
    D = H // nh
    q, k, v = qkv.split(H, dim=-1)
    K, V = torch.cat([k_hist, k], 1), torch.cat([v_hist, v], 1)
    t0, Tk = k_hist.shape[1], k_hist.shape[1] + cs
    qi, kj = t0 + torch.arange(cs)[:, None], torch.arange(Tk)[None, :]
    diff = qi // cs - kj // cs
    mask = (diff >= 0) & (diff <= lc)
    dlo = lc * cs + cs - 1
    idx = (dlo - (qi - kj)).clamp(0, pos.shape[0] - 1)                       # the row of distance i - j; masked pairs read any row
    heads = lambda t: t.reshape(B, -1, nh, D).transpose(1, 2)                # noqa: E731
    qu, qv = heads(q + bias_u), heads(q + bias_v)
    ac = qu @ heads(K).transpose(-1, -2)                                     # [B, nh, cs, Tk]
    P = pos.reshape(-1, nh, D).permute(1, 0, 2)                              # [nh, W, D]
    bd_all = qv @ P.transpose(-1, -2)[None]                                  # [B, nh, cs, W]
    bd = torch.gather(bd_all, 3, idx[None, None].expand(B, nh, cs, Tk))
    s = ((ac + bd) * D ** -0.5).masked_fill(~mask, float("-inf"))
    o = torch.softmax(s, -1) @ heads(V)
    return o.transpose(1, 2).reshape(B, cs, H), K, V


# ----------------------------------------------------------------------------------------------------------- transformers, chunk by chunk
def hf_stream_encode(ref, x, lookahead, dtype=torch.float64):
    """transformers' encoder of `ref` (NemotronAsrStreamingForRNNT) driven chunk by chunk with its own caches on x [B, T, F], in `dtype`
    -> the projected encoder states [B, T', Hd] (the model's `pooler_output`), one chunk's states after the other."""
    import copy
    m = copy.deepcopy(ref).to(dtype).eval()
    sw = m.config.encoder_config.sliding_window
    pkv = pc = None
    outs = []
    with torch.no_grad():
        for ch in chunks_of(x.to(dtype), sw, lookahead):
            out = m.encoder(input_features=ch, use_cache=True, past_key_values=pkv, padding_cache=pc, num_lookahead_tokens=lookahead)
            pkv, pc = out.past_key_values, out.padding_cache
            outs.append(m.encoder_projector(out.last_hidden_state))
    return torch.cat(outs, 1)
