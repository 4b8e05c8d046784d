"""CPU: the host half of the scores -- gpt.sequence_scores and gpt.rank_takes against the float64 reference of tests/scores_cases.py,
the reference of the per-code log-probability against values known in closed form, and the parked row's layout with and without the
log-probability segment."""
import math

import numpy as np
import pytest
import torch

import scores_cases as sk
from indextts_amd import gpt


def test_reference_logprob_closed_forms():
    for V in sk.VOCABS:
        rows = sk.crafted_rows(V)
        lp = sk.ref_logprobs(rows["equal"])
        assert np.allclose(lp, -math.log(V), rtol=0, atol=1e-13)
        for name, b in rows.items():
            lp = sk.ref_logprobs(b)
            assert np.isfinite(lp).all(), name
            assert abs(np.exp(lp).sum() - 1.0) < 1e-12, name
        lp = sk.ref_logprobs(rows["stop_-1e4"])
        assert lp[V - 1] < -9990.0 and np.isfinite(lp[V - 1])
        assert sk.ref_logprobs(rows["peaked"]).max() > -1e-3      # the peak holds nearly all the mass
    # two logits: log-sigmoid
    assert abs(sk.ref_logprob(np.float32([1.0, 3.0]), 1) + math.log1p(math.exp(-2.0))) < 1e-15


def test_sequence_scores_definition():
    rng = np.random.default_rng(5)
    lp = -rng.random((4, 9)).astype(np.float32) * 7
    lengths = [9, 1, 4, 6]
    for pen in (1.0, 0.0, 2.0):
        got = gpt.sequence_scores(lp, lengths, pen)
        assert got.dtype == np.float64
        for i, n in enumerate(lengths):
            assert got[i] == sk.ref_sequence_score(lp[i], n, pen)
    # length_penalty 0: the plain sum; 1: the mean; values behind the length never count
    assert gpt.sequence_scores(lp, lengths, 0.0)[2] == sum(float(x) for x in lp[2, :4])
    lp2 = lp.copy()
    lp2[2, 4:] = -1e9
    assert gpt.sequence_scores(lp2, lengths)[2] == gpt.sequence_scores(lp, lengths)[2]
    # tensors and ragged lists
    assert np.array_equal(gpt.sequence_scores(torch.from_numpy(lp), lengths), gpt.sequence_scores(lp, lengths))
    assert np.array_equal(gpt.sequence_scores([lp[i, :n] for i, n in enumerate(lengths)], lengths), gpt.sequence_scores(lp, lengths))
    # float64 accumulation in index order: fp32 accumulation would lose the small terms
    big = np.float32([-1e8] + [-1.0] * 8)
    assert gpt.sequence_scores([big], [9], 0.0)[0] == -1e8 - 8.0
    with pytest.raises(ValueError):
        gpt.sequence_scores(lp, [9, 1, 4])
    with pytest.raises(ValueError):
        gpt.sequence_scores(lp, [9, 0, 4, 6])
    with pytest.raises(ValueError):
        gpt.sequence_scores(lp, [10, 1, 4, 6])


def test_rank_takes_definition():
    # a truncated take ranks below every stopped one, whatever its score
    assert gpt.rank_takes([-0.1, -5.0, -2.0], [False, True, True]) == [2, 1, 0]
    # ties: the lower take index first
    assert gpt.rank_takes([-1.0, -1.0, -1.0], [True, True, True]) == [0, 1, 2]
    assert gpt.rank_takes([-1.0, -0.5, -1.0, -0.5], [True, False, True, False]) == [0, 2, 1, 3]
    # nobody stopped: by score alone
    assert gpt.rank_takes([-3.0, -1.0, -2.0], [False, False, False]) == [1, 2, 0]
    rng = np.random.default_rng(9)
    for _ in range(200):
        n = int(rng.integers(1, 7))
        scores = (-rng.integers(0, 4, n)).astype(np.float64)      # few values: many ties
        stopped = rng.integers(0, 2, n).astype(bool)
        assert gpt.rank_takes(scores, stopped) == sk.ref_rank(list(scores), list(stopped))
    with pytest.raises(ValueError):
        gpt.rank_takes([0.0, 1.0], [True])


def test_parked_row_layout_with_and_without_the_segment():
    for kv in (0, 1, 2):
        for (layers, heads, V, pos, step) in ((1, 2, 130, 9, 1), (2, 4, 8194, 37, 5), (24, 20, 8194, 600, 333), (1, 1, 19, 4, 4)):
            plain = sk.park_bytes(kv, layers, heads, V, pos, step, scores=False)
            scored = sk.park_bytes(kv, layers, heads, V, pos, step, scores=True)
            # without the flag: the parent's formula, byte for byte, and no room between codes and caches
            assert plain["bytes"] == sk.parent_park_bytes(kv, layers, heads, V, pos, step)
            assert plain["kv"] == plain["logprobs"] == plain["codes"] + sk.pad16(8 * step)
            # with it: one 16-byte-aligned segment of 4 * step bytes behind the codes, everything behind it moved by its padded size
            assert scored["seen"] == plain["seen"] and scored["codes"] == plain["codes"] and scored["logprobs"] == plain["logprobs"]
            assert scored["kv"] - plain["kv"] == scored["bytes"] - plain["bytes"] == sk.pad16(4 * step)
            assert all(v % 16 == 0 for v in scored.values())
