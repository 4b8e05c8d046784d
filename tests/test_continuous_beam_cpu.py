"""CPU: ContinuousPipeline(num_beams=N) -- per-request beam parameters and per-utterance seeds reach the beam session's admit() in
utterance order, num_beams must match the pipeline's, a bad request fails only its own Future, and a pipeline built without num_beams
still refuses beam requests (fake session, no GPU)."""
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.serving import ContinuousPipeline, utterance_beams

CFG = GPTConfig.tiny()
STOP = CFG.stop_mel_token
INFER = {"do_sample": True, "num_beams": 3, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0, "generator": None}


class BeamSession:
    """admit(rows, caps, beam) / step / take / free_groups / close over `groups` groups; every group finishes after one step with two
    codes.  Records the beam entry each admitted row came with, keyed by (first prompt value, text token)."""

    def __init__(self, groups, log):
        self.state = [None] * groups
        self.log = log

    @property
    def free_groups(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps, beam):
        assert len(beam) == len(rows)
        ids = self.free_groups[: len(rows)]
        for g, r, b in zip(ids, rows, beam):
            self.state[g] = b
            self.log.append((float(r[0, 0]), float(r[-1, 0]), dict(b)))
        return ids

    def step(self, n=1):
        return [i for i, s in enumerate(self.state) if s is not None]

    def take(self, g):
        self.state[g] = None
        return torch.tensor([3, STOP])

    def close(self):
        pass


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


def _pipe(log, slots=6, nb=3):
    return ContinuousPipeline(FakeTTS(), slots=slots, poll_steps=1, num_beams=nb, session_factory=lambda mp, mn: BeamSession(slots // nb, log))


def _by_utterance(log, cond_v, text):
    out = []
    for t in text:
        hits = [b for c, last, b in log if c == float(cond_v) and last == float(t[-1])]
        assert len(hits) == 1
        out.append(hits[0])
    return out


def test_seeds_drawn_at_submit_in_utterance_order():
    log = []
    text = torch.tensor([[5, 11], [5, 12], [5, 13], [5, 14]])
    torch.manual_seed(4321)
    want_global = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
    torch.manual_seed(4321)
    with _pipe(log) as pipe:
        f_glob = pipe.submit(text[:2], _cond(3), max_mel_tokens=8, sampling=INFER)
        f_seed = pipe.submit(text, _cond(1), max_mel_tokens=8, sampling=dict(INFER, seed=77, generator=torch.Generator().manual_seed(9)))
        f_gen = pipe.submit(text[:3], _cond(2), max_mel_tokens=8, sampling=dict(INFER, generator=torch.Generator().manual_seed(5)))
        f_search = pipe.submit(text[:2], _cond(4), max_mel_tokens=8, sampling={"do_sample": False, "num_beams": 3})
        for f, n in ((f_seed, 4), (f_gen, 3), (f_glob, 2), (f_search, 2)):
            assert len(f.result(timeout=60)) == n
    g = torch.Generator().manual_seed(77)
    want_seed = [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(4)]
    g = torch.Generator().manual_seed(5)
    want_gen = [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(3)]
    got = _by_utterance(log, 1, text)
    assert [b["seed"] for b in got] == want_seed      # `seed` wins over `generator`
    assert all(b == {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0, "early_stopping": False,
                     "seed": s} for b, s in zip(got, want_seed))
    assert [b["seed"] for b in _by_utterance(log, 2, text[:3])] == want_gen
    assert [b["seed"] for b in _by_utterance(log, 3, text[:2])] == want_global
    search = _by_utterance(log, 4, text[:2])
    assert all(not b["do_sample"] and b["length_penalty"] == 1.0 and b["top_k"] == 50 for b in search)      # generate_beam's defaults
    assert utterance_beams(dict(INFER, seed=77), 4, 3) == got


def test_num_beams_mismatch_refused():
    for s in ({"do_sample": True, "num_beams": 2}, {"do_sample": True}, None, {"do_sample": True, "num_beams": 1}):
        with pytest.raises(ValueError, match="num_beams"):
            utterance_beams(s, 1, 3)
    log = []
    with _pipe(log) as pipe:
        bad = pipe.submit(torch.tensor([[5, 6]]), _cond(0), max_mel_tokens=5, sampling=dict(INFER, num_beams=4))
        with pytest.raises(ValueError, match="num_beams"):
            bad.result(timeout=60)
    assert log == []
    with pytest.raises(ValueError, match="multiple"):
        ContinuousPipeline(FakeTTS(), slots=7, num_beams=3, session_factory=lambda mp, mn: BeamSession(2, []))


def test_bad_request_fails_only_its_own_future():
    log = []
    with _pipe(log, slots=4, nb=2) as pipe:
        good = pipe.submit(torch.tensor([[5, 6]]), _cond(1), max_mel_tokens=5, sampling=dict(INFER, num_beams=2, seed=1))
        bads = [pipe.submit(torch.tensor([[5, 7]]), _cond(1), max_mel_tokens=5, sampling=dict(INFER, num_beams=2, **s)) for s in (
            {"temperature": 0.0},
            {"top_k": 0, "top_p": 0.5},
            {"top_k": 2000},
            {"sampler": "hf"})]
        after = pipe.submit(torch.tensor([[5, 8]]), _cond(2), max_mel_tokens=5, sampling={"do_sample": False, "num_beams": 2})
        for b in bads:
            with pytest.raises(ValueError):
                b.result(timeout=60)
        assert len(good.result(timeout=60)) == 1 and len(after.result(timeout=60)) == 1
    assert len(log) == 2


def test_default_pipeline_still_refuses_beams():
    with ContinuousPipeline(FakeTTS(), slots=2, poll_steps=1, session_factory=lambda mp, mn: BeamSession(2, [])) as pipe:
        with pytest.raises(ValueError, match="BatchPipeline"):
            pipe.submit(torch.tensor([[5, 6]]), _cond(0), sampling=INFER)
    with ContinuousPipeline(FakeTTS(), slots=2, poll_steps=1, allow_sampling=True,
                            session_factory=lambda mp, mn: BeamSession(2, [])) as pipe:
        with pytest.raises(ValueError, match="num_beams"):
            pipe.submit(torch.tensor([[5, 6]]), _cond(0), sampling=INFER)
