"""CPU: ContinuousPipeline(scores=True).submit(takes=n, keep=k) over stand-in sessions (tests/cancel_standins.py's counting session
and fake TTS, through `session_factory`): the takes are ranked when all of them are decoded, exactly k rows per utterance reach the
acoustic stage, fut.ranking is in rank_request's order, noise seeds follow the kept takes, a cancelled request never ranks, and
keep=None leaves results and trace as they were.

The stand-in's takes follow a plan: PLAN[tag][j] = (codes produced, stopped, log-probability of every code) for take j of the
utterance with that tag; take j's codes start at 1000 * tag + 100 * j, so every result row names its utterance and take."""
import pytest
import torch

from cancel_standins import CFG, WAIT, EvictSession, FakeTTS, Gate, cond, text
from indextts_amd.serving import ContinuousPipeline, rank_request, utterance_noise_seeds

STOP = CFG.stop_mel_token
SAMPLING = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 11}
#       take 0: best mean but ran into its cap   1: stopped, -1.0   2: stopped, -0.5 (the winner)   3: stopped, -1.0 (ties with 1)
PLAN = {1: [(6, False, -0.1), (4, True, -1.0), (5, True, -0.5), (3, True, -1.0)],
        2: [(3, True, -2.0), (3, True, -2.0), (2, False, -0.2), (4, True, -0.25)],
        3: [(50, True, -1.0), (50, True, -1.0), (50, True, -1.0), (50, True, -1.0)]}
WANT = {1: [2, 1, 3, 0], 2: [3, 0, 1, 2]}      # stopped first, higher score, lower index


class ScoredSession(EvictSession):
    """The counting session with DecodeSession.admit's `sampling` and `takes` and take(slot, scores=True) -> (codes, logprobs).  A
    session built with scores=False refuses take(scores=True), as the real one does."""

    def __init__(self, slots, max_prompt, max_new, log, gate=None, scores=True):
        super().__init__(slots, max_prompt, max_new, log, gate)
        self.scores, self.nth = scores, {}

    def admit(self, rows, caps, sampling=None, takes=None):
        if takes is None:
            takes, caps, sampling = [1] * len(rows), [[c] for c in caps], [[e] for e in sampling]
        free = self.free_slots
        assert sum(takes) <= len(free), "more takes than free slots"
        out, o = [], 0
        for r, t, cs in zip(rows, takes, caps):
            ids, tag = free[o:o + t], int(r[1, 0])
            o += t
            for s in ids:
                j = self.nth.get(tag, 0)      # the takes of an utterance are admitted in take order, in one poll or in parts
                self.nth[tag] = j + 1
                n = PLAN[tag][j][0] if tag in PLAN else int(r[0, 0])
                self.state[s] = {"n": n, "have": 1, "tag": tag, "take": j}
            out.append(ids)
        self.log.append(("admit", out))
        return out if max(takes) > 1 else [g[0] for g in out]

    def take(self, slot, scores=False):
        s = self.state[slot]
        assert s is not None and s["have"] >= s["n"], "took a slot that has not finished"
        assert self.scores or not scores, "take(scores=True) on a session without scores"
        self.state[slot] = None
        tag, j, n = s["tag"], s["take"], s["n"]
        codes = 1000 * tag + 100 * j + torch.arange(n, dtype=torch.long)
        if tag not in PLAN:
            return (codes, torch.full((n,), -1.0)) if scores else codes
        if PLAN[tag][j][1]:
            codes[-1] = STOP
        self.log.append(("take", tag, j, scores))
        return (codes, torch.full((n,), PLAN[tag][j][2])) if scores else codes


class SeedTTS(FakeTTS):
    def __init__(self):
        super().__init__()
        self.seeds, self.rows = [], []

    def acoustic_stage(self, st, noise=None, noise_seeds=None):
        self.seeds.append(list(noise_seeds) if noise_seeds is not None else None)
        self.rows.append([(int(r[0]) // 1000, int(r[0]) % 1000 // 100) for r in st["codes"]])      # (utterance tag, take) of every row
        return super().acoustic_stage(st, noise=noise, noise_seeds=noise_seeds)


def _pipe(tts, slots, log, gate=None, scores=True, **kw):
    return ContinuousPipeline(tts, slots=slots, poll_steps=1, allow_sampling=True, scores=scores,
                              session_factory=lambda mp, mn: ScoredSession(slots, mp, mn, log, gate, scores), **kw)


def _who(w):
    return int(w[0]) // 1000, int(w[0]) % 1000 // 100


@pytest.mark.parametrize("keep", [1, 2, 4])
def test_keep_runs_the_acoustic_stage_on_k_rows_per_utterance_in_ranking_order(keep):
    tts, log = SeedTTS(), []
    with _pipe(tts, 8, log) as pipe:
        pipe.trace = []
        fut = pipe.submit(text((9, 1), (9, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, noise_seed=7, takes=4, keep=keep)
        res = fut.result(timeout=WAIT)
        trace = list(pipe.trace)
    assert [[t for t, *_ in rk] for rk in fut.ranking] == [WANT[1], WANT[2]]
    # (take, score, stopped, n_codes): the mean log-probability, float64
    assert fut.ranking[0][0] == (2, -0.5, True, 5) and fut.ranking[0][3] == (0, pytest.approx(-0.1, abs=1e-7), False, 6)
    assert fut.ranking[1][0] == (3, -0.25, True, 4) and fut.ranking[1][1][:1] == (0,) and fut.ranking[1][2][:1] == (1,)
    # result[i][j], j < keep, best first; exactly keep rows per utterance reached the acoustic stage, and no others
    assert len(res) == 2 and all(len(r) == keep for r in res)
    assert [[_who(w) for w in r] for r in res] == [[(1, t) for t in WANT[1][:keep]], [(2, t) for t in WANT[2][:keep]]]
    assert tts.rows == [[(1, t) for t in WANT[1][:keep]] + [(2, t) for t in WANT[2][:keep]]]
    assert [e[3] for e in trace if e[0] == "acoustic"] == [2 * keep]
    # the noise seeds follow the kept takes: take j of utterance i keeps entry i * n + j
    seeds = utterance_noise_seeds(7, 8)
    assert tts.seeds == [[seeds[t] for t in WANT[1][:keep]] + [seeds[4 + t] for t in WANT[2][:keep]]]
    # every take was decoded to its end and read with its scores
    assert sorted(e[1:3] for e in log if e[0] == "take") == [(u, t) for u in (1, 2) for t in range(4)]


def test_rank_request_is_the_order_the_pipeline_uses():
    codes, lps = [], []
    for tag in (1, 2):
        for j, (n, stopped, lp) in enumerate(PLAN[tag]):
            c = 1000 * tag + 100 * j + torch.arange(n)
            if stopped:
                c[-1] = STOP
            codes.append(c)
            lps.append(torch.full((n,), lp))
    rk = rank_request(codes, lps, 4, STOP)
    assert [[t for t, *_ in r] for r in rk] == [WANT[1], WANT[2]]
    # length_penalty 0: the plain sums -- utterance 1's take 3 (-3.0) now beats take 1 (-4.0), take 2 (-2.5) still wins
    assert [t for t, *_ in rank_request(codes, lps, 4, STOP, length_penalty=0.0)[0]] == [2, 3, 1, 0]
    with pytest.raises(ValueError):
        rank_request(codes, lps[:-1], 4, STOP)
    with pytest.raises(ValueError):
        rank_request(codes[:7], lps[:7], 4, STOP)


def test_explicit_noise_rows_follow_the_kept_takes():
    tts, log = SeedTTS(), []
    seen = {}
    orig = tts.acoustic_stage
    tts.acoustic_stage = lambda st, noise=None, noise_seeds=None: (seen.update(noise=noise), orig(st, noise, noise_seeds))[1]
    noise = torch.arange(8.0)[:, None, None].expand(8, 2, 3).contiguous()      # row r is all r
    with _pipe(tts, 8, log) as pipe:
        res = pipe.submit(text((9, 1), (9, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, noise=noise, takes=4, keep=2).result(timeout=WAIT)
    assert [[_who(w) for w in r] for r in res] == [[(1, 2), (1, 1)], [(2, 3), (2, 0)]]
    assert seen["noise"][:, 0, 0].tolist() == [2.0, 1.0, 7.0, 4.0]


def test_a_cancelled_request_never_ranks():
    tts, log, gate = SeedTTS(), [], Gate(armed=True)
    with _pipe(tts, 8, log, gate) as pipe:
        fut = pipe.submit(text((50, 3)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=4, keep=1)
        other = pipe.submit(text((9, 1)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=4, keep=1)
        gate.wait()                              # all eight rows are admitted, the lane stands at its first step
        assert pipe.cancel(fut)
        gate.open()
        res = other.result(timeout=WAIT)
    assert fut.cancelled() and not hasattr(fut, "ranking")
    assert [_who(w) for w in res[0]] == [(1, 2)] and [t for t, *_ in other.ranking[0]] == WANT[1]
    assert [e[1] for e in log if e[0] == "evict"] == [[0, 1, 2, 3]]
    assert all(tag != 3 for rows in tts.rows for tag, _ in rows)


def test_keep_none_is_the_pipeline_of_before():
    """Every take is synthesised, in take order, on a pipeline with scores and on one without (whose sessions are never asked for
    scores: the stand-in asserts it)."""
    for scores in (False, True):
        tts, log = SeedTTS(), []
        with _pipe(tts, 8, log, scores=scores) as pipe:
            pipe.trace = []
            fut = pipe.submit(text((9, 1), (9, 2)), cond(), max_mel_tokens=100, sampling=SAMPLING, noise_seed=7, takes=4)
            res = fut.result(timeout=WAIT)
            trace = list(pipe.trace)
        assert not hasattr(fut, "ranking")
        assert [[_who(w) for w in r] for r in res] == [[(u, t) for t in range(4)] for u in (1, 2)]
        assert tts.seeds == [utterance_noise_seeds(7, 8)] and [e[3] for e in trace if e[0] == "acoustic"] == [8]
        assert all(e[3] == scores for e in log if e[0] == "take")


def test_keep_is_refused_where_it_cannot_rank():
    tts, log = SeedTTS(), []
    with _pipe(tts, 8, log, scores=False) as pipe:
        with pytest.raises(ValueError, match="scores=True"):
            pipe.submit(text((9, 1)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=4, keep=1)
    with _pipe(tts, 8, log) as pipe:
        for bad in (0, 5):
            with pytest.raises(ValueError, match="1 .. takes"):
                pipe.submit(text((9, 1)), cond(), max_mel_tokens=100, sampling=SAMPLING, takes=4, keep=bad)
        with pytest.raises(ValueError, match="sampled takes"):
            pipe.submit(text((9, 1)), cond(), max_mel_tokens=100, keep=1)
    with pytest.raises(ValueError, match="num_beams == 1"):
        ContinuousPipeline(tts, slots=6, num_beams=3, scores=True, session_factory=lambda mp, mn: None)
    beam = {"do_sample": True, "num_beams": 3, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 5}

    class Idle:
        free_groups = [0, 1]

        def close(self):
            pass
    with ContinuousPipeline(tts, slots=6, num_beams=3, session_factory=lambda mp, mn: Idle()) as pipe:
        with pytest.raises(ValueError, match="n best"):
            pipe.submit(text((9, 1)), cond(), max_mel_tokens=100, sampling=beam, takes=2, keep=1)
    assert not log
