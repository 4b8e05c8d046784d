"""CPU: per-utterance CFM noise seeds through the serving pipelines -- utterance_noise_seeds' input forms, seeds fixed at submit,
which decoded requests one acoustic job merges once requests carry seeds (seeded with seeded, explicit noise with explicit noise,
neither kind alone) and what the merged call hands acoustic_stage -- with a fake decode session and a fake tts (no GPU, no kernels)
in the style of test_acoustic_coalesce_cpu.py, whose acoustic_stage also accepts noise_seeds."""
import threading
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.serving import ContinuousPipeline, merge_acoustic_states, utterance_noise_seeds

CFG = GPTConfig.tiny()
STOP = CFG.stop_mel_token


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
    """acoustic_stage returns, per row, [its prompt's value, its noise row's first value or -1, its seed or -1] and records
    (rows, noise given?, seeds) of every call."""

    def __init__(self):
        self.cfg = SimpleNamespace(gpt=CFG)
        self.device = "cpu"
        self.gpt = FakeGPT()
        self.acoustic_calls = []

    def gpt_stage(self, text, cond, max_mel_tokens, repetition_penalty, codes):
        lens = [int((row != STOP).sum()) for row in codes]
        return {"cond": cond, "B": int(codes.shape[0]), "codes": codes, "code_lens": lens, "code_lens_t": torch.tensor(lens),
                "latent": torch.zeros(codes.shape[0], codes.shape[1], 2), "times": {}}

    def acoustic_stage(self, st, noise=None, noise_seeds=None):
        if noise is not None and noise_seeds is not None:
            raise ValueError("both")
        conds = st["cond"] if isinstance(st["cond"], list) else [st["cond"]] * st["B"]
        self.acoustic_calls.append((st["B"], noise is not None, None if noise_seeds is None else list(noise_seeds)))
        if noise_seeds is not None:
            assert len(noise_seeds) == st["B"]
        return [torch.tensor([conds[b].value, float(noise[b, 0, 0]) if noise is not None else -1.0,
                              float(noise_seeds[b]) if noise_seeds is not None else -1.0]) for b in range(st["B"])]


def _cond(v):
    c = SimpleNamespace(value=float(v), spk_cond_latent=torch.full((1, 3, 4), float(v)), emo_vec=torch.zeros(1, 4))
    c.to = lambda dev: c
    return c


def _run(reqs, coalesce, max_rows=16, cap=5):
    """reqs: (rows, prompt, kind) per request, kind "seed" (noise_seed = [1000 k + r per row]), "noise" (explicit), "both" or None;
    all are decoded in one session and finish in the same poll."""
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
        for k, (rows, p, kind) in enumerate(reqs):
            c = conds.setdefault(p, _cond(p))
            noise = torch.zeros(rows, 80, 7 + k) + torch.arange(rows, dtype=torch.float32)[:, None, None] + 10 * k
            seeds = [1000 * k + r for r in range(rows)]
            text = torch.full((rows, 4), 5, dtype=torch.long)
            futs.append(pipe.submit(text, c, max_mel_tokens=cap, noise=noise if kind in ("noise", "both") else None,
                                    noise_seed=seeds if kind in ("seed", "both") else None))
            want.append([torch.tensor([float(p), float(r + 10 * k) if kind == "noise" else -1.0, float(seeds[r]) if kind == "seed" else -1.0])
                         for r in range(rows)])
        gate.set()
        got = []
        for f in futs:
            try:
                got.append(f.result(timeout=60))
            except ValueError as e:
                got.append(e)
        trace = list(pipe.trace)
    return tts, got, want, [t[4] for t in sorted(trace, key=lambda t: t[1])]


def _check(got, want, skip=()):
    for k, (g, w) in enumerate(zip(got, want)):
        if k in skip:
            continue
        assert not isinstance(g, Exception), (k, g)
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert torch.equal(a, b), k


def test_utterance_noise_seeds_forms():
    assert utterance_noise_seeds(None, 3) is None
    g = torch.Generator().manual_seed(1234)
    want = [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(4)]
    torch.manual_seed(1)
    state = torch.get_rng_state()
    assert utterance_noise_seeds(1234, 4) == want
    assert utterance_noise_seeds(1234, 2) == want[:2], "drawn in utterance order"
    assert torch.equal(state, torch.get_rng_state()), "the global generator is not touched"
    assert utterance_noise_seeds(1235, 4) != want
    given = [0, 2 ** 64 - 1, 2 ** 63 + 12345]
    assert utterance_noise_seeds(given, 3) == given
    assert utterance_noise_seeds(tuple(given), 3) == given
    assert utterance_noise_seeds(torch.tensor([4, 5]), 2) == [4, 5]


@pytest.mark.parametrize("bad,n", [([1, 2], 3), ([1, -1], 2), ([1, 2 ** 64], 2), ([1.5, 2], 2), ("12", 2), (1.5, 1), (-1, 1), (2 ** 64, 1),
                                   ([[1], [2]], 2)])
def test_utterance_noise_seeds_errors(bad, n):
    with pytest.raises(ValueError):
        utterance_noise_seeds(bad, n)


def test_three_seeded_requests_form_one_call_with_the_seeds_in_row_order():
    reqs = [(2, 1, "seed"), (1, 2, "seed"), (3, 1, "seed")]
    tts, got, want, groups = _run(reqs, coalesce=3)
    _check(got, want)
    assert groups == [(0, 1, 2)]
    assert tts.acoustic_calls == [(6, False, [0, 1, 1000, 2000, 2001, 2002])]


def test_an_int_seed_is_fixed_at_submit():
    """noise_seed=int: the per-row seeds are those of utterance_noise_seeds at submit, whatever the global generator does later."""
    tts = FakeTTS()
    gate = threading.Event()

    def factory(mp, mn):
        gate.wait(30)
        return GatedSession(8)
    with ContinuousPipeline(tts, slots=8, poll_steps=5, session_factory=factory) as pipe:
        torch.manual_seed(3)
        f = pipe.submit(torch.full((3, 4), 5, dtype=torch.long), _cond(1), max_mel_tokens=5, noise_seed=42)
        torch.manual_seed(4)
        torch.rand(5)
        gate.set()
        got = f.result(timeout=60)
    assert tts.acoustic_calls == [(3, False, utterance_noise_seeds(42, 3))]
    assert len(got) == 3


def test_kinds_are_not_mixed_and_unseeded_requests_run_alone():
    reqs = [(1, 1, "seed"), (1, 2, None), (2, 3, "noise"), (1, 2, "seed"), (1, 1, "noise"), (1, 3, None), (1, 1, "seed")]
    tts, got, want, groups = _run(reqs, coalesce=4)
    _check(got, want)
    assert groups == [(0, 3, 6), (1,), (2, 4), (5,)]
    assert [(n, z, s is not None) for n, z, s in tts.acoustic_calls] == [(3, False, True), (1, False, False), (3, True, False),
                                                                         (1, False, False)]


def test_row_cap_holds_for_seeded_requests():
    reqs = [(2, 1, "seed"), (2, 2, "seed"), (2, 3, "seed"), (1, 1, "seed"), (6, 2, "seed")]
    tts, got, want, groups = _run(reqs, coalesce=3, max_rows=5)
    _check(got, want)
    assert groups == [(0, 1, 3), (2,), (4,)]
    assert [n for n, _, _ in tts.acoustic_calls] == [5, 2, 6]


def test_noise_and_seed_together_fail_only_that_request():
    reqs = [(1, 1, "seed"), (2, 2, "both"), (1, 3, "seed")]
    tts, got, want, groups = _run(reqs, coalesce=1)
    assert isinstance(got[1], ValueError) and "not both" in str(got[1])
    _check(got, want, skip=(1,))
    assert groups == [(0,), (1,)], "a request refused at submit is never queued (the trace numbers the queued ones)"
    # and a bad seed value
    with ContinuousPipeline(FakeTTS(), slots=4, session_factory=lambda mp, mn: GatedSession(4)) as pipe:
        f = pipe.submit(torch.full((2, 4), 5, dtype=torch.long), _cond(1), max_mel_tokens=5, noise_seed=[1, 2, 3])
        with pytest.raises(ValueError):
            f.result(timeout=60)
        ok = pipe.submit(torch.full((2, 4), 5, dtype=torch.long), _cond(1), max_mel_tokens=5, noise_seed=[1, 2])
        assert len(ok.result(timeout=60)) == 2


def test_merge_acoustic_states_with_seed_lists():
    a, b = _cond(1), _cond(2)

    def st(c, B, n):
        return {"cond": c, "B": B, "codes": torch.ones(B, n, dtype=torch.long), "code_lens": [n] * B, "code_lens_t": torch.full((B,), n),
                "latent": torch.zeros(B, n, 2), "times": {}}
    m, seeds = merge_acoustic_states([(a, st(a, 2, 3), [7, 8]), (b, st(b, 1, 4), [2 ** 64 - 1])])
    assert m["B"] == 3 and seeds == [7, 8, 2 ** 64 - 1] and [c.value for c in m["cond"]] == [1, 1, 2]
    m, noise = merge_acoustic_states([(a, st(a, 2, 3), torch.ones(2, 80, 5)), (a, st(a, 1, 4), torch.ones(1, 80, 6))])
    assert noise.shape == (3, 80, 6), "tensor items keep today's contract"
