"""Edit-distance counts, host side (-m "not gpu"): the three-way cell recurrence that csrc/editdist.hip implements, restated in plain
Python and held equal to `wer._align` (distance AND the (ins, del, sub) of its alignment), and the `device=None` form of every scoring
function, which is the host path and returns what it returned before the device path existed."""
import itertools

import numpy as np
import pytest


def cell_rule(hyp, ref):
    """(ins, del, sub) by the plain cell recurrence: row 0 is (j, j, 0), column 0 is (i, 0, i) as (cost, ins, del); a cell takes the
    diagonal if diag <= up, else up, and keeps that unless left + 1 is strictly smaller.  sub = cost - ins - del."""
    n, m = len(ref), len(hyp)
    row = [(j, j, 0) for j in range(m + 1)]
    for i in range(1, n + 1):
        new = [(i, 0, i)]
        for j in range(1, m + 1):
            dc, di, dd = row[j - 1]
            uc, ui, ud = row[j]
            dc += int(hyp[j - 1] != ref[i - 1])
            cell = (dc, di, dd) if dc <= uc + 1 else (uc + 1, ui, ud + 1)
            lc, li, ld = new[j - 1]
            if lc + 1 < cell[0]:
                cell = (lc + 1, li + 1, ld)
            new.append(cell)
        row = new
    c, i, d = row[m]
    return i, d, c - i - d


def test_cell_rule_equals_align_exhaustively_over_three_symbols():
    from dynamic_asr_eval_amd.wer import _align
    seqs = [s for n in range(1, 6) for s in itertools.product(range(3), repeat=n)]
    assert len(seqs) == 363
    for h in seqs:
        for r in seqs:
            assert cell_rule(h, r) == _align(list(h), list(r)), (h, r)


@pytest.mark.parametrize("alphabet", [2, 3, 10])
def test_cell_rule_equals_align_on_random_pairs(alphabet):
    from dynamic_asr_eval_amd.wer import _align
    rng = np.random.default_rng(100 + alphabet)
    for _ in range(120):
        h = rng.integers(0, alphabet, rng.integers(1, 61)).tolist()
        r = rng.integers(0, alphabet, rng.integers(1, 61)).tolist()
        assert cell_rule(h, r) == _align(h, r), (h, r)


def test_cell_rule_empty_sides_are_aligns():
    from dynamic_asr_eval_amd.wer import _align
    assert cell_rule([1, 2, 3], []) == _align([1, 2, 3], []) == (3, 0, 0)
    assert cell_rule([], [1, 2]) == _align([], [1, 2]) == (0, 2, 0)


HYPS = ["a b c d", "x y", "", "the cat sat", "q"]
REFS = ["a c d e", "x y z", "u v", "the cat sat on the mat", ""]


def test_wer_functions_accept_device_none_and_return_the_host_values():
    from dynamic_asr_eval_amd.wer import _align, edit_counts, edit_counts_pairs, word_error_rate_detail
    assert edit_counts(HYPS[:2], REFS[:2], device=None) == edit_counts(HYPS[:2], REFS[:2]) == (1, 2, 0, 7)
    pairs = edit_counts_pairs(HYPS, REFS, device=None)
    assert pairs == edit_counts_pairs(HYPS, REFS) == [(1, 1, 0, 4), (0, 1, 0, 3), (0, 2, 0, 2), (0, 3, 0, 6), (1, 0, 0, 0)]
    assert edit_counts(HYPS, REFS) == tuple(sum(p[k] for p in pairs) for k in range(4))
    chars = edit_counts_pairs(["ab cd", "a  b"], ["ab xd", "a b"], use_cer=True, device=None)
    assert chars == [(0, 0, 1, 5), (1, 0, 0, 3)]                 # spaces are units
    assert chars[0][:3] == _align([0, 1, 2, 3, 4], [0, 1, 2, 5, 4])
    assert edit_counts(["ab cd", "a  b"], ["ab xd", "a b"], use_cer=True, device=None) == (1, 0, 1, 8)
    assert word_error_rate_detail(["the cat sat"], ["the cat sat on the mat"], device=None) == (0.5, 6, 0.0, 0.5, 0.0)
    assert word_error_rate_detail(["ab"], ["abcd"], use_cer=True, device=None) == (0.5, 4, 0.0, 0.5, 0.0)


def test_calc_rewards_and_score_texts_accept_device_none(capsys):
    from dynamic_asr_eval_amd.enc_dec import calc_rewards
    from dynamic_asr_eval_amd.harness_common import score_texts
    assert calc_rewards("ab cd ef", ["ab xy ef", "", "ab cd ef"], device=None) == [((1 - 1 / 3) + (1 - 2 / 8)) / 2, 0.0, 1.0]
    assert calc_rewards(" ", ["x y z", "q", ""], device=None) == [-3.0, -1.0, 1.0]
    assert calc_rewards("a", ["a b c d"], device=None) == calc_rewards("a", ["a b c d"]) == [((1 - 3.0) + (1 - 6.0)) / 2]
    assert capsys.readouterr().out.count("avg reward") == 4
    want = {"wer": 3 / 7, "words": 7, "ins_rate": 1 / 7, "del_rate": 2 / 7, "sub_rate": 0.0}
    assert score_texts(HYPS[:2], REFS[:2], device=None) == score_texts(HYPS[:2], REFS[:2]) == want


def test_device_path_refuses_a_cpu_device():
    """A device that is not a GPU is an error, never a quiet host computation."""
    from dynamic_asr_eval_amd._lib import DynError
    from dynamic_asr_eval_amd.wer import edit_counts
    with pytest.raises(DynError):
        edit_counts(["a b"], ["a c"], device="cpu")


def test_abi_argument_checks_run_before_any_launch():
    """Offsets and the tile are checked on the host, so a bad call is a DYN_E_* code without a GPU."""
    from dynamic_asr_eval_amd import _lib
    lib = _lib.load()
    good = np.array([0, 3, 5], dtype=np.int64)
    assert lib.dyn_edit_counts_resident_limit() == (160 * 1024 - 1024) // 44
    assert lib.dyn_edit_counts_workspace_bytes(good.ctypes.data, good.ctypes.data, 2, 0) == 0
    big = np.array([0, 5000], dtype=np.int64)
    # 5000 x 5000 at the default tile of 1024: 5 x 5 blocks, 4 boundary rows and 4 boundary columns of 5001 cells x 3 int32
    assert lib.dyn_edit_counts_workspace_bytes(big.ctypes.data, big.ctypes.data, 1, 0) == 2 * 4 * 5001 * 3 * 4
    assert lib.dyn_edit_counts_workspace_bytes(good.ctypes.data, good.ctypes.data, 2, 8) == 0
    for bad in (np.array([0, -1, 5], dtype=np.int64), np.array([-2, 3, 5], dtype=np.int64), np.array([0, 4, 3], dtype=np.int64)):
        assert lib.dyn_edit_counts_workspace_bytes(bad.ctypes.data, good.ctypes.data, 2, 0) == -1
        assert lib.dyn_edit_counts_workspace_bytes(good.ctypes.data, bad.ctypes.data, 2, 0) == -1
        assert lib.dyn_edit_counts(None, None, bad.ctypes.data, good.ctypes.data, None, None, None, 0, 2, 0, None) == -1
        assert b"dyn_edit_counts" in lib.dyn_last_error()
    assert lib.dyn_edit_counts_workspace_bytes(good.ctypes.data, good.ctypes.data, 2, 7) == -1        # tile outside [8, 2048]
    assert lib.dyn_edit_counts_workspace_bytes(good.ctypes.data, good.ctypes.data, 2, 4096) == -1
    assert lib.dyn_edit_counts_workspace_bytes(None, good.ctypes.data, 2, 0) == -1
    assert lib.dyn_edit_counts(None, None, good.ctypes.data, good.ctypes.data, None, None, None, 0, 2, 0, None) == -1   # null pointers
    assert lib.dyn_edit_counts(None, None, big.ctypes.data, big.ctypes.data, None, None, None, 0, 1, 0, None) == -1
