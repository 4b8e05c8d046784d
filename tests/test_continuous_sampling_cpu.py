"""CPU: ContinuousPipeline(allow_sampling=True) -- per-request sampling parameters and per-utterance seeds reach the decode session's
admit() in utterance order, bad parameters fail only their own request, greedy requests reach it as "greedy" (fake session, no GPU)."""
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.serving import ContinuousPipeline, utterance_samplers

CFG = GPTConfig.tiny()
STOP = CFG.stop_mel_token


class SamplingSession:
    """admit(rows, caps, sampling) / step / take / free_slots / close; every row finishes after one step with two codes.  Records the
    sampler each admitted row came with, keyed by (first prompt value, text token) so a test can find its utterances."""

    def __init__(self, slots, log):
        self.state = [None] * slots
        self.log = log
        self.closed = False

    @property
    def free_slots(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps, sampling):
        assert len(sampling) == len(rows)
        free = self.free_slots
        ids = free[: len(rows)]
        for s, r, smp in zip(ids, rows, sampling):
            self.state[s] = smp
            self.log.append((float(r[0, 0]), float(r[-1, 0]), dict(smp)))
        return ids

    def step(self, n=1):
        return [i for i, s in enumerate(self.state) if s is not None]

    def take(self, slot):
        self.state[slot] = None
        return torch.tensor([3, STOP])

    def close(self):
        self.closed = True


class FakeGPT:
    def conds_latent(self, lat, emo):
        return lat

    def prompt_rows(self, conds, text):
        return [torch.cat([conds[0], t.float()[:, None].expand(-1, conds.shape[-1])]) for t in text]


class FakeTTS:
    def __init__(self):
        self.cfg = SimpleNamespace(gpt=CFG)
        self.device = "cpu"
        self.gpt = FakeGPT()

    def gpt_stage(self, text, cond, max_mel_tokens, repetition_penalty, codes):
        return {"codes": codes}

    def acoustic_stage(self, st, noise=None):
        return [row.clone() for row in st["codes"]]


def _cond(v):
    return SimpleNamespace(spk_cond_latent=torch.full((1, 2, 4), float(v)), emo_vec=torch.zeros(1, 4), to=lambda dev, _v=v: _cond(_v))


def _pipe(log, slots=3):
    return ContinuousPipeline(FakeTTS(), slots=slots, poll_steps=1, allow_sampling=True,
                              session_factory=lambda mp, mn: SamplingSession(slots, log))


def _by_utterance(log, cond_v, text):
    """The samplers the session saw for the utterances of a request, in utterance order (text rows end in distinct tokens)."""
    out = []
    for t in text:
        hits = [smp for c, last, smp in log if c == float(cond_v) and last == float(t[-1])]
        assert len(hits) == 1
        out.append(hits[0])
    return out


def test_parameters_and_seeds_reach_admit_in_utterance_order():
    log = []
    hf = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "num_beams": 1, "generator": None}
    text = torch.tensor([[5, 11], [5, 12], [5, 13], [5, 14]])
    torch.manual_seed(1234)
    want_global = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
    torch.manual_seed(1234)
    with _pipe(log) as pipe:
        f_seed = pipe.submit(text, _cond(1), max_mel_tokens=8, sampling=dict(hf, seed=77))
        f_gen = pipe.submit(text[:3], _cond(2), max_mel_tokens=8,
                            sampling=dict(hf, sampler="accel", generator=torch.Generator().manual_seed(5)))
        f_glob = pipe.submit(text[:2], _cond(3), max_mel_tokens=8, sampling=hf)
        for f, n in ((f_seed, 4), (f_gen, 3), (f_glob, 2)):
            assert len(f.result(timeout=60)) == n
    g = torch.Generator().manual_seed(77)
    want_seed = [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(4)]
    g = torch.Generator().manual_seed(5)
    want_gen = [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(3)]
    got = _by_utterance(log, 1, text)
    assert [s["seed"] for s in got] == want_seed
    assert all(s["sampler"] == "hf" and s["temperature"] == 0.8 and s["top_k"] == 30 and s["top_p"] == 0.8 for s in got)
    got = _by_utterance(log, 2, text[:3])
    assert [s["seed"] for s in got] == want_gen and all(s["sampler"] == "accel" for s in got)
    assert [s["seed"] for s in _by_utterance(log, 3, text[:2])] == want_global
    assert utterance_samplers(dict(hf, seed=77), 4) == [{"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": s}
                                                        for s in want_seed]


def test_bad_parameters_fail_only_their_own_future():
    log = []
    with _pipe(log, slots=2) as pipe:
        with pytest.raises(ValueError, match="num_beams"):
            pipe.submit(torch.tensor([[5, 6]]), _cond(0), sampling={"do_sample": True, "num_beams": 3})
        good = pipe.submit(torch.tensor([[5, 6]]), _cond(1), max_mel_tokens=5, sampling={"do_sample": True, "seed": 1})
        bads = [pipe.submit(torch.tensor([[5, 7]]), _cond(1), max_mel_tokens=5, sampling=s) for s in (
            {"do_sample": True, "temperature": 0.0},
            {"do_sample": True, "top_k": 0, "top_p": 0.5},
            {"do_sample": True, "sampler": "beam"},
            {"do_sample": True, "typical_p": 0.3})]
        # takes of a request whose one conditioning holds a row per utterance: it cannot be repeated per take
        per_row = SimpleNamespace(spk_cond_latent=torch.zeros(2, 2, 4), emo_vec=torch.zeros(2, 4))
        bads.append(pipe.submit(torch.tensor([[5, 7], [5, 7]]), per_row, max_mel_tokens=5, sampling={"do_sample": True, "seed": 1}, takes=2))
        good2 = pipe.submit(torch.tensor([[5, 8], [5, 9]]), _cond(2), max_mel_tokens=5)
        for b in bads:
            with pytest.raises(ValueError):
                b.result(timeout=60)
        assert len(good.result(timeout=60)) == 1 and len(good2.result(timeout=60)) == 2
    assert len(log) == 3          # only the good requests' utterances reached the session
    # what says nothing about one request raises at submit: a closed pipeline, and one whose lanes have all failed
    with pytest.raises(RuntimeError, match="pipeline closed"):
        pipe.submit(torch.tensor([[5, 6]]), _cond(1), max_mel_tokens=5)

    def no_session(mp, mn):
        raise OSError("no device")
    with ContinuousPipeline(FakeTTS(), slots=2, poll_steps=1, allow_sampling=True, session_factory=no_session) as dead:
        for t in dead._lanes:
            t.join(60)
        with pytest.raises(RuntimeError, match="every decode lane has failed"):
            dead.submit(torch.tensor([[5, 6]]), _cond(1), max_mel_tokens=5)


def test_greedy_requests_reach_the_session_as_greedy():
    log = []
    with _pipe(log) as pipe:
        a = pipe.submit(torch.tensor([[5, 21]]), _cond(4), max_mel_tokens=5)
        b = pipe.submit(torch.tensor([[5, 22]]), _cond(4), max_mel_tokens=5, sampling={"do_sample": False, "num_beams": 1})
        a.result(timeout=60), b.result(timeout=60)
    assert [smp for _, _, smp in log] == [{"sampler": "greedy"}, {"sampler": "greedy"}]


def test_off_by_default_and_session_gets_two_arguments():
    """Without allow_sampling nothing changes: sampling= is refused and admit() is called with (rows, caps) only."""
    calls = []

    class TwoArgSession(SamplingSession):
        def admit(self, rows, caps):
            calls.append(len(rows))
            return super().admit(rows, caps, [{"sampler": "greedy"}] * len(rows))

    with ContinuousPipeline(FakeTTS(), slots=2, poll_steps=1, session_factory=lambda mp, mn: TwoArgSession(2, [])) as pipe:
        with pytest.raises(ValueError):
            pipe.submit(torch.tensor([[5]]), _cond(0), sampling={"do_sample": True})
        assert len(pipe.submit(torch.tensor([[5, 6]]), _cond(0), max_mel_tokens=4).result(timeout=60)) == 1
    assert calls == [1]
