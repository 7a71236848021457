"""The flat parameter layout both models build on (dynamic_asr_eval_amd/_flat.py) and the capture policy's counter (_graphs.py), without a GPU."""
import gc
import math


def _running_sum(spec):
    """The layout rule restated: slot i begins at the sum of ceil(n_j / 64) * 64 over the slots before it."""
    off, want = 0, {}
    for name, shape in spec:
        n = math.prod(shape)
        want[name] = (off, n, shape)
        off += -(-n // 64) * 64
    return want, off


def test_layout_rounds_every_slot_up_to_64_floats():
    from dynamic_asr_eval_amd._flat import flat_layout
    spec = [("one", (1,)), ("below", (63,)), ("exact", (64,)), ("above", (65,)), ("cube", (3, 5, 7))]
    slots, n_flat = flat_layout(spec)
    assert [slots[n][0] for n, _ in spec] == [0, 64, 128, 192, 320]
    assert [slots[n][1:] for n, _ in spec] == [(math.prod(s), s) for _, s in spec]
    assert n_flat == 320 + 128                                   # 105 floats take two 64-float units
    assert list(slots) == [n for n, _ in spec]                   # spec order is slot order


def test_layout_of_both_models_follows_the_rule():
    from dynamic_asr_eval_amd import model, wav2vec2_model
    from dynamic_asr_eval_amd._flat import flat_layout
    w2v = [(n, s) for n, s, _ in wav2vec2_model.param_spec(wav2vec2_model.make_config())]
    for spec in (model.param_spec(model.make_config(), 129), w2v):
        slots, n_flat = flat_layout(spec)
        want, total = _running_sum(spec)
        assert len(slots) == len(spec) and n_flat == total
        for name, _ in spec:
            assert slots[name] == want[name], name


def test_wav2vec2_qkv_slots_are_contiguous():
    """What Wav2Vec2ForCTC's packed [3H, H] projection views assert: q | k | v weights (then their biases) side by side for H = 768."""
    from dynamic_asr_eval_amd import wav2vec2_model
    from dynamic_asr_eval_amd._flat import flat_layout
    cfg = wav2vec2_model.make_config()
    H = cfg["hidden_size"]
    assert H == 768
    slots, _ = flat_layout([(n, s) for n, s, _ in wav2vec2_model.param_spec(cfg)])
    for l in range(cfg["num_hidden_layers"]):
        p = f"wav2vec2.encoder.layers.{l}.attention."
        ow, ob = slots[p + "q_proj.weight"][0], slots[p + "q_proj.bias"][0]
        assert [slots[p + f"{n}_proj.weight"][0] for n in "qkv"] == [ow, ow + H * H, ow + 2 * H * H]
        assert [slots[p + f"{n}_proj.bias"][0] for n in "qkv"] == [ob, ob + H, ob + 2 * H]


def test_seen_counter_is_true_from_the_nth_sighting_per_key():
    from dynamic_asr_eval_amd._graphs import Seen
    for n in (1, 2, 3):
        seen = Seen()
        a = [seen("a", n) for _ in range(n + 2)]
        assert a == [False] * (n - 1) + [True] * 3
        b = [seen(("b", 1), n) for _ in range(n)]                # another key starts from zero, whatever "a" has reached
        assert b == [False] * (n - 1) + [True]
        assert seen("a", n)


def test_no_gc_restores_the_collector_state_it_found():
    from dynamic_asr_eval_amd._graphs import _no_gc
    was = gc.isenabled()
    try:
        for state in (True, False):
            gc.enable() if state else gc.disable()
            with _no_gc():
                assert not gc.isenabled()
            assert gc.isenabled() == state
    finally:
        gc.enable() if was else gc.disable()
