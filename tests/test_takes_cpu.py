"""CPU: the host side of several takes per request.

  * the n-best read's order, tie and padding rule (`idxtts_beam_finalize_host`, the routine behind generate_beam_nbest and
    session_read_nbest) against a small restatement of BeamSearchScorer.finalize (transformers_beam_search.py:320-414) on hand-made
    hypothesis lists -- the tiny model yields no two hypotheses of one group with equal scores, so ties are made by hand here;
  * the new prototypes: include/idxtts.h and the ctypes binding agree on their argument counts."""
import ctypes
import os
import re

import numpy as np
import pytest

from indextts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP, LD = 99, 8
NEW = ("idxtts_gpt_session_admit_takes", "idxtts_gpt_session_fork", "idxtts_gpt_generate_beam_nbest", "idxtts_gpt_session_read_nbest",
       "idxtts_beam_finalize_host")


def _finalize(nb, lp, hyps, done, open_beams, steps, cap, n_best):
    """BeamHypotheses.add for the open beams of an utterance that is not done (keep num_beams, drop the worst: the first of the lowest
    scores), then sorted(beams, key=score) popped from the end n_best times; each row = the hypothesis, the stop token where it fits
    under the cap, stop-padded.  hyps / open_beams: [(score or sum of log-probabilities, tokens)]."""
    beams = [(float(s), list(t)) for s, t in hyps]
    if not done:
        worst = min([s for s, _ in beams], default=1e9)
        for total, toks in open_beams:
            score = float(np.float32(total)) / (steps ** lp)
            if len(beams) < nb or score > worst:
                beams.append((score, list(toks[:steps])))
                if len(beams) > nb:
                    ranked = sorted([(s, i) for i, (s, _) in enumerate(beams)])
                    del beams[ranked[0][1]]
                    worst = ranked[1][0]
                else:
                    worst = min(worst, score)
    ranked = sorted(beams, key=lambda x: x[0])      # stable: of equal scores the one added later is popped first
    rows = []
    for _ in range(n_best):
        score, toks = ranked.pop()
        rows.append((toks + [STOP] * (LD - len(toks)), min(len(toks) + 1, cap), np.float32(score)))
    return rows


def _native(nb, lp, hyps, done, open_beams, steps, cap, n_best, slots=None):
    lib = _lib.load()
    H = 9
    slots = list(range(len(hyps))) if slots is None else slots
    score = np.zeros(H, np.float64)
    length, slot = np.zeros(H, np.int32), np.zeros(H, np.int32)
    hyp_seq = np.full((H, LD), -7, np.int32)
    for q, (s, toks) in enumerate(hyps):
        score[q], length[q], slot[q] = s, len(toks), slots[q]
        hyp_seq[slots[q], : len(toks)] = toks
    bscore = np.array([b[0] for b in open_beams], np.float32)
    seq = np.full((nb, LD), -7, np.int32)
    for j, (_, toks) in enumerate(open_beams):
        seq[j, : len(toks)] = toks
    codes = np.zeros((n_best, LD), np.int64)
    lens, scores = np.zeros(n_best, np.int32), np.zeros(n_best, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.idxtts_beam_finalize_host(nb, lp, len(hyps), p(score), p(length), p(slot), p(hyp_seq), LD, int(done), p(bscore), p(seq), steps,
                                       cap, STOP, n_best, p(codes), p(lens), p(scores))
    return rc, codes, lens, scores


def _check(nb, lp, hyps, done, open_beams, steps, cap, slots=None):
    for n_best in range(1, nb + 1):
        want = _finalize(nb, lp, hyps, done, open_beams, steps, cap, n_best)
        rc, codes, lens, scores = _native(nb, lp, hyps, done, open_beams, steps, cap, n_best, slots)
        assert rc == 0
        for q, (row, ln, sc) in enumerate(want):
            assert codes[q].tolist() == row and lens[q] == ln and scores[q] == sc, (n_best, q, codes[q], row, lens[q], ln, scores[q], sc)
    return want


def _open(nb, steps, scores):
    return [(s, [10 * (j + 1) + t for t in range(steps)]) for j, s in zip(range(nb), scores)]


def test_ties_go_to_the_hypothesis_added_later():
    # three finished hypotheses, the two best with the same score: the later one comes first; the scorer is done
    hyps = [(-1.5, [1, 2, 3]), (-1.5, [4, 5]), (-2.0, [6])]
    want = _check(3, 0.0, hyps, True, _open(3, 6, [-9, -9, -9]), 6, 8)
    assert [w[0][:3] for w in want] == [[4, 5, STOP], [1, 2, 3], [6, STOP, STOP]]
    # all equal, stored in shuffled rows of hyp_seq: list order decides, not the storage row
    hyps = [(-3.0, [1]), (-3.0, [2]), (-3.0, [3]), (-3.0, [4])]
    want = _check(4, 1.0, hyps, True, _open(4, 5, [-9] * 4), 5, 8, slots=[3, 0, 8, 1])
    assert [w[0][0] for w in want] == [4, 3, 2, 1]


def test_open_beams_top_the_list_up():
    # not done, one finished hypothesis: the open beams join at steps_done tokens, an open beam that ties with the finished one is
    # added later and so comes first; with length_penalty 1 the open beams' sums are divided by the steps
    hyps = [(-2.0, [7, 7])]
    want = _check(3, 0.0, hyps, False, _open(3, 4, [-2.0, -5.0, -1.0]), 4, 8)
    assert [w[0][0] for w in want] == [30, 10, 7] and [w[1] for w in want] == [5, 5, 3]
    _check(3, 1.0, hyps, False, _open(3, 4, [-8.0, -5.0, -1.0]), 4, 8)
    # a full list: an open beam replaces the worst only when it is strictly better, and the first of two equal worst ones leaves
    hyps = [(-4.0, [1]), (-4.0, [2]), (-1.0, [3])]
    want = _check(3, 0.0, hyps, False, _open(3, 3, [-4.0, -3.0, -6.0]), 3, 8)
    assert [w[0][0] for w in want] == [3, 20, 2]
    # no finished hypothesis at all (the cap came first): the open beams in beam order, equal ones later first
    want = _check(2, 0.0, [], False, _open(2, 8, [-3.0, -3.0]), 8, 8)
    assert [w[0][0] for w in want] == [20, 10]


def test_padding_and_lengths_under_the_cap():
    # the stop token follows where it fits under the cap and counts in the length; a hypothesis as long as the cap gets none
    hyps = [(-1.0, [1, 2, 3, 4, 5, 6]), (-2.0, [1, 2, 3, 4, 5]), (-3.0, [])]
    want = _check(3, 0.0, hyps, True, _open(3, 6, [-9] * 3), 6, 6)
    assert [w[1] for w in want] == [6, 6, 1] and want[0][0] == [1, 2, 3, 4, 5, 6, STOP, STOP] and want[2][0] == [STOP] * LD


def test_bad_calls_are_refused():
    hyps = [(-1.0, [1])]
    beams = _open(2, 3, [-2.0, -3.0])
    assert _native(2, 0.0, hyps, False, beams, 3, 8, 3)[0] != 0       # n_best > num_beams
    assert _native(2, 0.0, hyps, False, beams, 3, 8, 0)[0] != 0
    assert _native(2, 0.0, hyps, False, beams, 3, 2, 1)[0] != 0       # cap below the steps done
    assert _native(2, 0.0, hyps, True, beams, 3, 8, 2)[0] != 0        # fewer hypotheses than n_best (cannot occur after finalize)
    assert _native(2, 0.0, hyps, False, beams, 3, 8, 1, slots=[-1])[0] != 0       # a storage row out of range


def _header_params():
    text = open(os.path.join(ROOT, "include", "idxtts.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(idxtts_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(params.split(","))
    return out


@pytest.mark.parametrize("name", NEW)
def test_header_and_binding_agree(name):
    declared = _header_params()
    assert name in declared and name in _lib.SYMBOLS
    fn = getattr(_lib.load(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name], (name, len(fn.argtypes or ()), declared[name])


# ---------------------------------------------------------------------------------------------------------------------------------
# ContinuousPipeline.submit(takes=) over stand-in sessions (tests/cancel_standins.py's counting session and fake TTS)

import torch  # noqa: E402

from cancel_standins import WAIT, EvictSession, FakeTTS, Gate, cond, text, wave  # noqa: E402
from indextts_amd.serving import ContinuousPipeline, utterance_noise_seeds, utterance_samplers  # noqa: E402


class TakesSession(EvictSession):
    """The counting session with DecodeSession.admit's `sampling`, `takes`: one prompt row per request, takes[b] slots for it; logs
    ("admit", slot lists, tags, takes, the seed of every take)."""

    def admit(self, rows, caps, sampling=None, takes=None):
        if takes is None:
            takes, caps, sampling = [1] * len(rows), [[c] for c in caps], [[e] for e in sampling]
        free = self.free_slots
        assert len(rows) == len(takes) == len(caps) == len(sampling) and sum(takes) <= len(free), "more takes than free slots"
        out, o = [], 0
        for r, t, cs, es in zip(rows, takes, caps, sampling):
            assert len(cs) == len(es) == t
            ids = free[o:o + t]
            o += t
            for s, c in zip(ids, cs):
                self.state[s] = {"n": min(int(r[0, 0]), int(c)), "have": 1, "tag": int(r[1, 0])}
            out.append(ids)
        self.log.append(("admit", out, [int(r[1, 0]) for r in rows], list(takes), [[e["seed"] for e in es] for es in sampling]))
        return out if max(takes) > 1 else [g[0] for g in out]


class SeedTTS(FakeTTS):
    def __init__(self):
        super().__init__()
        self.seeds = []

    def acoustic_stage(self, st, noise=None, noise_seeds=None):
        self.seeds.append(list(noise_seeds) if noise_seeds is not None else None)
        return super().acoustic_stage(st, noise=noise, noise_seeds=noise_seeds)


SAMPLING = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 11}


def _pipe(tts, slots, log, gate=None, **kw):
    return ContinuousPipeline(tts, slots=slots, poll_steps=1, allow_sampling=True,
                              session_factory=lambda mp, mn: TakesSession(slots, mp, mn, log, gate), **kw)


def test_pipeline_takes_order_shape_and_shared_prefill():
    tts, log = SeedTTS(), []
    with _pipe(tts, 8, log) as pipe:
        fut = pipe.submit(text((3, 1), (5, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, noise_seed=7, takes=3)
        one = pipe.submit(text((2, 3)), cond(), max_mel_tokens=100, sampling=SAMPLING, noise_seed=7)
        res, flat = fut.result(timeout=WAIT), one.result(timeout=WAIT)
    assert len(res) == 2 and all(len(r) == 3 for r in res)                       # result[i][j]
    assert all(torch.equal(res[i][j][:n], wave(n, tag)) for i, (n, tag) in enumerate(((3, 1), (5, 2))) for j in range(3))      # (padded to the longest row)
    assert len(flat) == 1 and torch.equal(flat[0], wave(2, 3))                   # takes = 1 keeps the flat list
    want = [e["seed"] for e in utterance_samplers(SAMPLING, 6)]
    admits = [e for e in log if e[0] == "admit"]
    assert admits[0][2][:2] == [1, 2] and admits[0][3][:2] == [3, 3]            # one prompt row per utterance, three slots each
    assert admits[0][4][:2] == [want[0:3], want[3:6]]                           # entry i * n + j
    assert utterance_noise_seeds(7, 6) in tts.seeds and utterance_noise_seeds(7, 1) in tts.seeds
    assert [len(set(s)) for s in (want,)] == [6]


def test_pipeline_takes_admitted_in_parts():
    log = []
    with _pipe(SeedTTS(), 4, log) as pipe:
        res = pipe.submit(text((3, 1), (4, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=3).result(timeout=WAIT)
    assert [[int(w[0]) // 1000 for w in r] for r in res] == [[1, 1, 1], [2, 2, 2]]
    admits = [e for e in log if e[0] == "admit"]
    want = [e["seed"] for e in utterance_samplers(SAMPLING, 6)]
    assert admits[0][2] == [1, 2] and admits[0][3] == [3, 1] and admits[0][4] == [want[0:3], want[3:4]]      # four slots: 3 + 1 ...
    assert admits[1][2] == [2] and admits[1][3] == [2] and admits[1][4] == [want[4:6]]                       # ... then the other two, one prefill


def test_pipeline_cancel_a_request_with_takes():
    log, gate = [], Gate(armed=True)
    with _pipe(SeedTTS(), 8, log, gate) as pipe:
        fut = pipe.submit(text((50, 1), (50, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=3)
        other = pipe.submit(text((2, 3)), cond(), max_mel_tokens=100, sampling=SAMPLING)
        gate.wait()                              # all seven rows are admitted, the lane stands at its first step
        assert pipe.cancel(fut)
        gate.open()
        assert torch.equal(other.result(timeout=WAIT)[0], wave(2, 3))
    assert fut.cancelled()
    evicted = [e[1] for e in log if e[0] == "evict"]
    assert evicted == [[0, 1, 2, 3, 4, 5]]       # every take's slot, in one call


def test_pipeline_refuses_greedy_takes():
    log = []
    with _pipe(SeedTTS(), 4, log) as pipe:
        with pytest.raises(ValueError, match="takes > 1"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, takes=2)
        with pytest.raises(ValueError, match="takes > 1"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, sampling={"do_sample": False}, takes=2)
        with pytest.raises(ValueError, match="takes"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=0)
    assert not log


class NBestSession:
    """A beam stand-in: groups that finish after one step; take(g, n_best=) returns n (codes, score), hypothesis q = [tag, q]."""

    def __init__(self, groups, log):
        self.state, self.log = [None] * groups, log

    @property
    def free_groups(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps, beam):
        ids = self.free_groups[: len(rows)]
        for g, r, b in zip(ids, rows, beam):
            self.state[g] = int(r[1, 0])
            self.log.append(("admit", g, int(r[1, 0]), b["seed"]))
        return ids

    def step(self, n=1):
        return [i for i, s in enumerate(self.state) if s is not None]

    def take(self, g, n_best=None):
        tag, self.state[g] = self.state[g], None
        self.log.append(("take", tag, n_best))
        if n_best is None:
            return torch.tensor([1000 * tag, 1000 * tag])
        return [(torch.tensor([1000 * tag, 1000 * tag + q]), -float(q)) for q in range(n_best)]

    def close(self):
        pass


def test_beam_pipeline_takes_are_the_n_best_and_too_many_fail_only_that_future():
    tts, log = SeedTTS(), []
    beam = {"do_sample": True, "num_beams": 3, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 5}
    with ContinuousPipeline(tts, slots=6, num_beams=3, poll_steps=1, session_factory=lambda mp, mn: NBestSession(2, log)) as pipe:
        bad = pipe.submit(text((2, 9)), cond(), max_mel_tokens=100, sampling=beam, takes=4)
        good = pipe.submit(text((2, 1), (2, 2)), cond(), max_mel_tokens=100, sampling=beam, noise_seed=3, takes=2)
        plain = pipe.submit(text((2, 4)), cond(), max_mel_tokens=100, sampling=beam)
        with pytest.raises(ValueError, match="num_beams"):
            bad.result(timeout=WAIT)
        res, flat = good.result(timeout=WAIT), plain.result(timeout=WAIT)
    assert [[w.tolist() for w in r] for r in res] == [[[1000, 1000], [1000, 1001]], [[2000, 2000], [2000, 2001]]]
    assert [w.tolist() for w in flat] == [[4000, 4000]]
    assert ("take", 1, 2) in log and ("take", 2, 2) in log and ("take", 4, None) in log and not any(e[2] == 9 for e in log if e[0] == "admit")
    assert utterance_noise_seeds(3, 4) in tts.seeds      # one noise seed per take: B * n
