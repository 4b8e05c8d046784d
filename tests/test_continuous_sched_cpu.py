"""CPU: ContinuousPipeline's slot bookkeeping -- admission into free slots, freeing, per-request completion and error isolation --
driven by a fake decode session (no GPU, no kernels)."""
import threading
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.serving import ContinuousPipeline

CFG = GPTConfig.tiny()
STOP = CFG.stop_mel_token


def _length(row) -> int:
    """The fake model's number of codes for a prompt row (stop token included)."""
    return 2 + int(row[:, 0].sum().item()) % 13


class FakeSession:
    """admit / step / take / free_slots / close, with the decode replaced by a counter per slot."""

    def __init__(self, slots, max_prompt, max_new, log):
        self.slots, self.max_prompt, self.max_new = slots, max_prompt, max_new
        self.state = [None] * slots          # [target length, produced, ended]
        self.log = log
        self.closed = False

    @property
    def free_slots(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps):
        free = self.free_slots
        assert 1 <= len(rows) <= len(free), "admitted more rows than free slots"
        for r, c in zip(rows, caps):
            assert r.shape[0] <= self.max_prompt and 1 <= c <= self.max_new
        ids = free[: len(rows)]
        for s, r, c in zip(ids, rows, caps):
            n = _length(r)
            self.state[s] = [n, 1, n == 1 or c == 1, n <= c, min(n, c)]
        self.log["admits"].append(len(rows))
        self.log["max_busy"] = max(self.log["max_busy"], sum(s is not None for s in self.state))
        return ids

    def step(self, n=1):
        for s in self.state:
            if s is not None and not s[2]:
                s[1] = min(s[1] + n, s[4])
                s[2] = s[1] >= s[4]
        return [i for i, s in enumerate(self.state) if s is not None and s[2]]

    def take(self, slot):
        s = self.state[slot]
        assert s is not None and s[2], "took a slot that has not finished"
        self.state[slot] = None
        codes = torch.arange(s[1], dtype=torch.long)
        if s[3]:
            codes[-1] = STOP
        return codes

    def close(self):
        self.closed = True


class FakeGPT:
    def conds_latent(self, lat, emo):
        return lat

    def prompt_rows(self, conds, text):
        if int(text.max()) > CFG.number_text_tokens:
            raise IndexError("text token id out of range")
        return [torch.cat([conds[0], t[t != CFG.stop_text_token].float()[:, None].expand(-1, conds.shape[-1])]) for t in text]


class FakeTTS:
    def __init__(self):
        self.cfg = SimpleNamespace(gpt=CFG)
        self.device = "cpu"
        self.gpt = FakeGPT()
        self.stage_rows = []

    def gpt_stage(self, text, cond, max_mel_tokens, repetition_penalty, codes):
        self.stage_rows.append(int(codes.shape[0]))
        assert codes.shape[0] == text.shape[0]
        return {"codes": codes}

    def acoustic_stage(self, st, noise=None):
        return [row.clone() for row in st["codes"]]


def _cond(v):
    return SimpleNamespace(spk_cond_latent=torch.full((1, 3, 4), float(v)), emo_vec=torch.zeros(1, 4),
                           to=lambda dev, _v=v: _cond(_v))


def _expected(text, cond_v, cap):
    out = []
    for t in text:
        row = torch.cat([torch.full((3, 4), float(cond_v)), t[t != CFG.stop_text_token].float()[:, None].expand(-1, 4)])
        n = _length(row)
        codes = torch.arange(min(n, cap), dtype=torch.long)
        if n <= cap:
            codes[-1] = STOP
        out.append(codes)
    return out


def _requests():
    g = torch.Generator().manual_seed(0)
    reqs = []
    for k in range(9):
        B, L = 1 + k % 3, 3 + (5 * k) % 11
        text = torch.randint(2, 50, (B, L), generator=g)
        if B > 1:
            text[1, L - 2:] = CFG.stop_text_token
        reqs.append((text, k % 2, 4 + (7 * k) % 9))
    return reqs


def _pad(rows):
    n = max(r.shape[0] for r in rows)
    out = torch.full((len(rows), n), STOP, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, : r.shape[0]] = r
    return list(out)


@pytest.mark.parametrize("slots,lanes,poll", [(1, 1, 1), (3, 1, 2), (4, 2, 5), (16, 1, 16)])
def test_every_request_completes_with_its_own_rows(slots, lanes, poll):
    log = {"admits": [], "max_busy": 0}
    lock = threading.Lock()
    sessions = []

    def factory(mp, mn):
        with lock:
            s = FakeSession(slots, mp, mn, log)
            sessions.append(s)
            return s

    tts = FakeTTS()
    reqs = _requests()
    with ContinuousPipeline(tts, slots=slots, decode_lanes=lanes, poll_steps=poll, session_factory=factory) as pipe:
        futs = [pipe.submit(text, _cond(c), max_mel_tokens=cap) for text, c, cap in reqs]
        results = [f.result(timeout=60) for f in futs]
    for (text, c, cap), got in zip(reqs, results):
        want = _pad(_expected(text, c, cap))
        assert len(got) == text.shape[0]
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert log["max_busy"] <= slots
    assert all(s.closed for s in sessions) and len(sessions) == lanes
    assert sorted(tts.stage_rows) == sorted(int(t.shape[0]) for t, _, _ in reqs)      # one acoustic call per request, all its rows
    if slots >= 4:
        assert max(log["admits"]) > 1          # utterances of different requests and widths shared a session


def test_bad_request_fails_only_its_own_future():
    tts = FakeTTS()
    with ContinuousPipeline(tts, slots=2, poll_steps=3, session_factory=lambda mp, mn: FakeSession(2, mp, mn, {"admits": [], "max_busy": 0})) as pipe:
        good1 = pipe.submit(torch.tensor([[5, 6, 7]]), _cond(1), max_mel_tokens=20)
        bad = pipe.submit(torch.tensor([[5, CFG.number_text_tokens + 7]]), _cond(1), max_mel_tokens=20)
        good2 = pipe.submit(torch.tensor([[8, 9], [4, 4]]), _cond(0), max_mel_tokens=5)
        with pytest.raises(IndexError):
            bad.result(timeout=60)
        assert len(good1.result(timeout=60)) == 1
        assert len(good2.result(timeout=60)) == 2


def test_refuses_sampling_and_out_of_range_caps():
    tts = FakeTTS()
    with ContinuousPipeline(tts, slots=2, max_new=50, session_factory=lambda mp, mn: FakeSession(2, mp, mn, {"admits": [], "max_busy": 0})) as pipe:
        with pytest.raises(ValueError):
            pipe.submit(torch.tensor([[5]]), _cond(0), sampling={"do_sample": True})
        with pytest.raises(ValueError):
            pipe.submit(torch.tensor([[5]]), _cond(0), max_mel_tokens=51)
        with pytest.raises(ValueError):
            pipe.submit(torch.tensor([[5]]), _cond(0), max_mel_tokens=10, repetition_penalty=2.0)
