"""CPU: ContinuousPipeline(acoustic_coalesce=N) -- which finished requests one acoustic job merges (up to N requests and
acoustic_max_rows rows, explicit noise only), how every request gets its own rows back, and that a failure stays inside its merged
batch -- with a fake decode session and a fake tts (no GPU, no kernels).  Also merge_acoustic_states' prompt bookkeeping."""
import threading
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.serving import ContinuousPipeline, merge_acoustic_states

CFG = GPTConfig.tiny()
STOP = CFG.stop_mel_token
BAD = 99.0          # a prompt value the fake acoustic stage refuses


class GatedSession:
    """Every row decodes exactly its cap (codes 1, 2, ..., cap); no stop token."""

    def __init__(self, slots):
        self.state = [None] * slots

    @property
    def free_slots(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps):
        ids = self.free_slots[: len(rows)]
        for s, c in zip(ids, caps):
            self.state[s] = [c, 0]
        return ids

    def step(self, n=1):
        for s in self.state:
            if s is not None:
                s[1] = min(s[1] + n, s[0])
        return [i for i, s in enumerate(self.state) if s is not None and s[1] >= s[0]]

    def take(self, slot):
        c = self.state[slot][0]
        self.state[slot] = None
        return torch.arange(1, c + 1, dtype=torch.long)

    def close(self):
        pass


class FakeGPT:
    def conds_latent(self, lat, emo):
        return lat

    def prompt_rows(self, conds, text):
        return [conds[0][:1].expand(2 + int(t.shape[0]), -1) for t in text]


class FakeTTS:
    """gpt_stage returns the state the real one returns (per-row code lengths, a latent that carries the prompt's value);
    acoustic_stage returns, per row, [its codes, its prompt's value, its noise row's first value]."""

    def __init__(self):
        self.cfg = SimpleNamespace(gpt=CFG)
        self.device = "cpu"
        self.gpt = FakeGPT()
        self.latent_rows = []       # rows of every gpt_stage call
        self.acoustic_calls = []    # (rows, per-row prompt values) of every acoustic_stage call

    def gpt_stage(self, text, cond, max_mel_tokens, repetition_penalty, codes):
        self.latent_rows.append(int(codes.shape[0]))
        lens = [int((row != STOP).sum()) for row in codes]
        return {"cond": cond, "B": int(codes.shape[0]), "codes": codes, "code_lens": lens, "code_lens_t": torch.tensor(lens),
                "latent": torch.zeros(codes.shape[0], codes.shape[1], 2), "times": {}}

    def acoustic_stage(self, st, noise=None):
        conds = st["cond"] if isinstance(st["cond"], list) else [st["cond"]] * st["B"]
        vals = [c.value for c in conds]
        self.acoustic_calls.append((st["B"], vals))
        if BAD in vals:
            raise RuntimeError("bad prompt in this batch")
        out = []
        for b in range(st["B"]):
            z = float(noise[b, 0, 0]) if noise is not None else -1.0
            out.append(torch.cat([st["codes"][b, : st["code_lens"][b]].float(), torch.tensor([conds[b].value, z])]))
        return out


def _cond(v):
    c = SimpleNamespace(value=float(v), spk_cond_latent=torch.full((1, 3, 4), float(v)), emo_vec=torch.zeros(1, 4))
    c.to = lambda dev: c
    return c


def _run(reqs, coalesce, max_rows=16, cap=5):
    """reqs: (rows, prompt, noise?) per request; all are decoded in one session and finish in the same poll."""
    tts = FakeTTS()
    gate = threading.Event()

    def factory(mp, mn):
        gate.wait(30)           # the lane starts once every request is waiting: one admission, one finishing poll
        return GatedSession(64)

    conds = {}
    with ContinuousPipeline(tts, slots=64, poll_steps=cap, session_factory=factory, acoustic_coalesce=coalesce,
                            acoustic_max_rows=max_rows) as pipe:
        pipe.trace = []
        futs, want = [], []
        for k, (rows, p, has_noise) in enumerate(reqs):
            c = conds.setdefault(p, _cond(p))
            noise = torch.full((rows, 80, 7 + k), 0.0) + torch.arange(rows, dtype=torch.float32)[:, None, None] + 10 * k if has_noise else None
            text = torch.full((rows, 4), 5, dtype=torch.long)
            futs.append(pipe.submit(text, c, max_mel_tokens=cap, noise=noise))
            want.append([torch.cat([torch.arange(1, cap + 1).float(), torch.tensor([float(p), float(r + 10 * k) if has_noise else -1.0])])
                         for r in range(rows)])
        gate.set()
        got = []
        for f in futs:
            try:
                got.append(f.result(timeout=60))
            except RuntimeError as e:
                got.append(e)
        trace = list(pipe.trace)
    return tts, got, want, [t[4] for t in sorted(trace, key=lambda t: t[1])], trace


def _check(got, want, skip=()):
    for k, (g, w) in enumerate(zip(got, want)):
        if k in skip:
            continue
        assert not isinstance(g, Exception), (k, g)
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert torch.equal(a, b), k


def test_groups_up_to_n_requests_and_the_row_cap():
    reqs = [(2, 1, True), (2, 2, True), (2, 3, True), (1, 1, True), (3, 2, True), (1, 3, True)]
    tts, got, want, groups, trace = _run(reqs, coalesce=3, max_rows=5)
    _check(got, want)
    # the oldest request, then the next ones that fit: 2 + 2 (+ 2 would be 6 rows) + 1; then 2 + 3; then the last
    assert groups == [(0, 1, 3), (2, 4), (5,)]
    assert [t[3] for t in sorted(trace, key=lambda t: t[1])] == [5, 5, 1]
    assert tts.latent_rows == [reqs[k][0] for g in groups for k in g], "the latent pass runs per request"
    assert tts.acoustic_calls[0][1] == [1.0, 1.0, 2.0, 2.0, 1.0], "rows keep their own prompts"


def test_requests_without_noise_run_alone():
    reqs = [(1, 1, True), (1, 2, False), (2, 3, True), (1, 2, True), (1, 1, False)]
    tts, got, want, groups, _ = _run(reqs, coalesce=4)
    _check(got, want)
    assert groups == [(0, 2, 3), (1,), (4,)]


def test_a_request_over_the_row_cap_runs_alone():
    reqs = [(6, 1, True), (1, 2, True), (2, 1, True)]
    tts, got, want, groups, _ = _run(reqs, coalesce=4, max_rows=4)
    _check(got, want)
    assert groups == [(0,), (1, 2)]


def test_failure_stays_inside_its_merged_batch():
    reqs = [(1, 1, True), (2, BAD, True), (1, 2, True), (1, 3, True), (2, 1, True)]
    tts, got, want, groups, _ = _run(reqs, coalesce=2)
    assert groups == [(2, 3), (4,)]                   # (the trace records the jobs that succeeded)
    assert tts.acoustic_calls[0] == (3, [1.0, BAD, BAD])
    for k in (0, 1):
        assert isinstance(got[k], RuntimeError) and "bad prompt" in str(got[k])
    _check(got, want, skip=(0, 1))


def test_coalesce_1_is_one_job_per_request():
    reqs = [(1, 1, True), (2, 2, True), (1, 3, False), (3, 1, True)]
    tts, got, want, groups, _ = _run(reqs, coalesce=1)
    _check(got, want)
    assert groups == [(0,), (1,), (2,), (3,)]
    assert [n for n, _ in tts.acoustic_calls] == [1, 2, 1, 3]


def test_merge_keeps_one_prompt_or_lists_every_rows():
    a, b = _cond(1), _cond(2)
    da, da2, db = _cond(1), _cond(1), _cond(2)       # the device copies two gpt_stage calls made of a, and one of b

    def st(c, B, n):
        return {"cond": c, "B": B, "codes": torch.ones(B, n, dtype=torch.long), "code_lens": [n] * B, "code_lens_t": torch.full((B,), n),
                "latent": torch.zeros(B, n, 2), "times": {}}
    z = lambda B, T: torch.ones(B, 80, T)
    m, noise = merge_acoustic_states([(a, st(da, 2, 3), z(2, 5)), (a, st(da2, 1, 4), z(1, 6))])
    assert m["cond"] is da and m["B"] == 3 and m["codes"].shape == (3, 4) and noise.shape == (3, 80, 6)
    assert (noise[:2, :, 5] == 0).all() and (noise[:2, :, :5] == 1).all()
    m, _ = merge_acoustic_states([(a, st(da, 2, 3), z(2, 5)), (b, st(db, 1, 4), z(1, 6)), (a, st(da2, 1, 2), z(1, 4))])
    assert isinstance(m["cond"], list) and [c.value for c in m["cond"]] == [1, 1, 2, 1]
    assert m["cond"][3] is da, "rows of one submitted prompt share one device copy"
    m, _ = merge_acoustic_states([([a, b], st([da, db], 2, 3), z(2, 5)), (b, st(db, 1, 4), z(1, 6))])
    assert [c.value for c in m["cond"]] == [1, 2, 2] and m["cond"][2] is db


def test_bad_arguments():
    with pytest.raises(ValueError):
        ContinuousPipeline(FakeTTS(), slots=4, session_factory=lambda mp, mn: GatedSession(4), acoustic_coalesce=0)
    with pytest.raises(ValueError):
        ContinuousPipeline(FakeTTS(), slots=4, session_factory=lambda mp, mn: GatedSession(4), acoustic_max_rows=0)
