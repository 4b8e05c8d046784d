"""CPU: per-request diffusion steps and CFG rates on their way to the acoustic batch -- the schedule tables S2Mel hands
idxtts_s2mel_cfm_sched, the argument rules, what merge_acoustic_states carries, and what both pipelines hand acoustic_stage for each
request's rows (takes and keep included).  Stand-in sessions and a fake tts (tests/cancel_standins.py), no GPU, no kernels."""
import contextlib
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cancel_standins as cs
from cancel_standins import FakeTTS, PlainSession, cond, text, wave
from indextts_amd import serving
from indextts_amd.s2mel import cfm_schedule_tables, per_row_values, timestep_tables
from indextts_amd.serving import BatchPipeline, ContinuousPipeline, _keep_best, acoustic_settings, merge_acoustic_states

WAIT = cs.WAIT
DEFAULTS = (25, 0.7)


# ---- the schedule tables ----
def test_schedule_tables_are_timestep_tables_per_distinct_count():
    sched, t_emb, dt, row_sched = cfm_schedule_tables([3, 1, 2, 3, 1])
    assert sched.dtype == np.int32 and row_sched.dtype == np.int32
    assert sched.tolist() == [3, 1, 2]                      # distinct counts, in order of first appearance
    assert row_sched.tolist() == [0, 1, 2, 0, 1]
    assert t_emb.shape == (6, 256) and dt.shape == (6,) and t_emb.dtype == torch.float32 and dt.dtype == torch.float32
    at = 0
    for n in sched.tolist():
        e, d = timestep_tables(n)
        assert torch.equal(t_emb[at:at + n], e) and torch.equal(dt[at:at + n], d), n
        at += n
    for b, n in enumerate([3, 1, 2, 3, 1]):                 # every row's schedule has the row's step count
        assert sched[row_sched[b]] == n
    one = cfm_schedule_tables([4, 4])
    assert one[0].tolist() == [4] and one[3].tolist() == [0, 0] and torch.equal(one[1], timestep_tables(4)[0])


# ---- argument rules ----
def test_per_row_values_forms():
    assert per_row_values(3, 2, "diffusion_steps") == ([3, 3], False)
    assert per_row_values([3, 1], 2, "diffusion_steps") == ([3, 1], True)
    assert per_row_values(torch.tensor([2, 5]), 2, "diffusion_steps") == ([2, 5], True)
    assert per_row_values(0.5, 3, "cfg_rate") == ([0.5, 0.5, 0.5], False)
    assert per_row_values((0.0, 1.5), 2, "cfg_rate") == ([0.0, 1.5], True)
    assert per_row_values(np.float32(0.25), 1, "cfg_rate") == ([0.25], False)


@pytest.mark.parametrize("value,rows,name", [
    ([3, 1], 3, "diffusion_steps"), ([3], 2, "diffusion_steps"), (0, 2, "diffusion_steps"), ([2, 0], 2, "diffusion_steps"),
    (-1, 1, "diffusion_steps"), (2.5, 1, "diffusion_steps"), (True, 1, "diffusion_steps"),
    ([0.7], 2, "cfg_rate"), (-0.1, 2, "cfg_rate"), ([0.7, -1e-9], 2, "cfg_rate"), (float("nan"), 1, "cfg_rate"),
    ([0.0, float("inf")], 2, "cfg_rate"), ([0.0, float("-inf")], 2, "cfg_rate")])
def test_per_row_values_errors(value, rows, name):
    with pytest.raises(ValueError):
        per_row_values(value, rows, name)


def test_acoustic_settings():
    assert acoustic_settings(None, None, 3) == (None, None)
    assert acoustic_settings(8, None, 2) == ([8, 8], None)
    assert acoustic_settings([8, 20], 0.0, 2) == ([8, 20], [0.0, 0.0])
    with pytest.raises(ValueError):
        acoustic_settings([8, 20, 3], None, 2)
    with pytest.raises(ValueError):
        acoustic_settings(None, [0.7, -0.7], 2)


# ---- merge_acoustic_states ----
def _state(B, n, c, **extra):
    st = {"cond": c, "B": B, "codes": torch.zeros(B, n, dtype=torch.long), "code_lens": [n] * B, "code_lens_t": torch.tensor([n] * B),
          "latent": torch.zeros(B, n, 2), "times": {}}
    st.update(extra)
    return st


def test_merge_carries_per_row_values_and_keeps_todays_keys_without_them():
    c = cond()
    keys = set(merge_acoustic_states([(c, _state(2, 3, c), [1, 2]), (c, _state(1, 5, c), [3])], DEFAULTS)[0])
    assert keys == {"cond", "B", "codes", "code_lens", "code_lens_t", "latent", "times"}
    assert set(merge_acoustic_states([(c, _state(2, 3, c), [1, 2]), (c, _state(1, 5, c), [3])])[0]) == keys      # (no defaults given)
    st, seeds = merge_acoustic_states([(c, _state(2, 3, c, diffusion_steps=[3, 1], cfg_rate=[0.7, 0.0]), [1, 2]),
                                       (c, _state(1, 5, c), [3]),
                                       (c, _state(2, 4, c, diffusion_steps=[8, 8]), [4, 5])], DEFAULTS)
    assert st["B"] == 5 and seeds == [1, 2, 3, 4, 5]
    assert st["diffusion_steps"] == [3, 1, 25, 8, 8]
    assert st["cfg_rate"] == [0.7, 0.0, 0.7, 0.7, 0.7]
    assert set(st) == keys | {"diffusion_steps", "cfg_rate"}
    only = merge_acoustic_states([(c, _state(1, 3, c, cfg_rate=[1.5]), [1]), (c, _state(1, 3, c), [2])], DEFAULTS)[0]
    assert only["cfg_rate"] == [1.5, 0.7] and "diffusion_steps" not in only
    with pytest.raises(ValueError):
        merge_acoustic_states([(c, _state(1, 3, c, cfg_rate=[1.5]), [1]), (c, _state(1, 3, c), [2])])


def test_keep_best_keeps_the_kept_rows_values():
    r = SimpleNamespace(takes=3, text=torch.arange(6)[:, None], cond=cond(), noise=None, noise_seeds=[10, 11, 12, 13, 14, 15],
                        diffusion_steps=[1, 2, 3, 4, 5, 6], cfg_rate=[0.0, 0.1, 0.2, 0.3, 0.4, 0.5])
    ranking = [[(2, 0.0, True, 4), (0, -1.0, True, 4), (1, -2.0, True, 4)], [(1, 0.0, True, 4), (2, -1.0, True, 4), (0, -2.0, True, 4)]]
    assert _keep_best(r, ranking, 2) == [2, 0, 4, 5]
    assert r.diffusion_steps == [3, 1, 5, 6] and r.cfg_rate == [0.2, 0.0, 0.4, 0.5] and r.noise_seeds == [12, 10, 14, 15] and r.takes == 2
    r = SimpleNamespace(takes=2, text=torch.arange(2)[:, None], cond=cond(), noise=None, noise_seeds=None, diffusion_steps=None, cfg_rate=[0.0, 0.9])
    assert _keep_best(r, [[(1, 0.0, True, 4), (0, -1.0, True, 4)]], 1) == [1]
    assert r.diffusion_steps is None and r.cfg_rate == [0.9]


# ---- the pipelines ----
class SettingsTTS(FakeTTS):
    """records, per acoustic call, each row's (tag, steps, rate) as acoustic_stage finds them in the state (None: key absent)"""
    _diffusion_steps, _cfg_rate = DEFAULTS

    def __init__(self):
        super().__init__()
        self.calls = []

    def acoustic_stage(self, st, noise=None, noise_seeds=None):
        tags = [int(row[0]) // 1000 for row in st["codes"]]
        for key in ("diffusion_steps", "cfg_rate"):
            assert key not in st or len(st[key]) == st["B"]
        with self.lock:
            self.calls.append([(t, st["diffusion_steps"][b] if "diffusion_steps" in st else None, st["cfg_rate"][b] if "cfg_rate" in st else None)
                               for b, t in enumerate(tags)])
        return super().acoustic_stage(st, noise=noise, noise_seeds=noise_seeds)


def test_continuous_pipeline_hands_each_request_its_values():
    tts = SettingsTTS()
    gate = threading.Event()

    def factory(mp, mn):
        gate.wait(WAIT)          # the lane starts once every request waits: one admission, one finishing poll, one acoustic job
        return PlainSession(16, mp, mn, [], None)

    with ContinuousPipeline(tts, slots=16, poll_steps=4, session_factory=factory, acoustic_coalesce=4) as pipe:
        pipe.trace = []
        futs = [pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, noise_seed=1, diffusion_steps=3, cfg_rate=0.7),
                pipe.submit(text((3, 2), (3, 3)), cond(), max_mel_tokens=100, noise_seed=2, diffusion_steps=[1, 2], cfg_rate=0.0),
                pipe.submit(text((3, 4)), cond(), max_mel_tokens=100, noise_seed=3, cfg_rate=[1.5]),
                pipe.submit(text((3, 5)), cond(), max_mel_tokens=100, noise_seed=4)]
        bad = [pipe.submit(text((3, 6)), cond(), max_mel_tokens=100, noise_seed=5, **kw)
               for kw in (dict(diffusion_steps=[1, 2]), dict(diffusion_steps=0), dict(cfg_rate=-0.5), dict(cfg_rate=float("nan")))]
        gate.set()
        for k, f in enumerate(futs):
            assert torch.equal(f.result(timeout=WAIT)[0], wave(3, [1, 2, 4, 5][k]))
        for f in bad:
            with pytest.raises(ValueError):
                f.result(timeout=WAIT)
        jobs = [t for t in pipe.trace if t[0] == "acoustic"]
    assert len(jobs) == 1 and jobs[0][3] == 5, jobs          # one acoustic batch of all five rows
    assert tts.calls == [[(1, 3, 0.7), (2, 1, 0.0), (3, 2, 0.0), (4, 25, 1.5), (5, 25, 0.7)]]


def test_continuous_pipeline_without_values_hands_todays_state():
    tts = SettingsTTS()
    with ContinuousPipeline(tts, slots=4, poll_steps=4, session_factory=lambda mp, mn: PlainSession(4, mp, mn, [], None)) as pipe:
        assert torch.equal(pipe.submit(text((3, 7)), cond(), max_mel_tokens=100, noise_seed=1).result(timeout=WAIT)[0], wave(3, 7))
    assert tts.calls == [[(7, None, None)]]


# BatchPipeline's scheduling needs streams and events only as tokens (tests/test_cancel_sched_cpu.py): a torch whose `cuda` is a stand-in
class _Stream:
    cuda_stream = 1

    def __init__(self, device=None, priority=0):
        pass

    priority_range = staticmethod(lambda: (0, -1))
    wait_event = wait_stream = lambda self, x: None
    synchronize = lambda self: None


class _Torch:
    class cuda:
        Stream = _Stream
        Event = type("Event", (), {"record": lambda self, s=None: None})
        current_stream = staticmethod(lambda device=None: _Stream())
        set_device = staticmethod(lambda device: None)
        stream = staticmethod(lambda s: contextlib.nullcontext())
        device = staticmethod(lambda d: contextlib.nullcontext())

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.fixture
def hostonly(monkeypatch):
    from indextts_amd import _lib
    monkeypatch.setattr(serving, "torch", _Torch())
    monkeypatch.setattr(_lib, "release_stream", lambda s: None)


def test_batch_pipeline_hands_each_request_its_values_takes_included(hostonly):
    """x holds the only acoustic worker while a, b, c, d are decoded and queue behind it: they run as one acoustic batch.  b has two
    takes per utterance: its per-row values follow utterance_noise_seeds' row rule, row i * takes + j."""
    tts = SettingsTTS()
    tts.acoustic_gate.armed = True
    same = cond()
    pipe = BatchPipeline(tts, decode_lanes=1, acoustic_workers=1, acoustic_coalesce=4)
    x = pipe.submit(text((2, 9)), same, max_mel_tokens=100, noise_seed=1)
    tts.acoustic_gate.wait()
    tts.decode_gate.armed = True
    a = pipe.submit(text((3, 1)), same, max_mel_tokens=100, noise_seed=1, diffusion_steps=3, cfg_rate=0.7)
    b = pipe.submit(text((3, 2)), same, max_mel_tokens=100, noise_seed=1, sampling={"do_sample": True}, takes=2, diffusion_steps=[1, 2], cfg_rate=0.0)
    c = pipe.submit(text((3, 3)), same, max_mel_tokens=100, noise_seed=1, diffusion_steps=[2])
    d = pipe.submit(text((3, 4)), same, max_mel_tokens=100, noise_seed=1)
    e = pipe.submit(text((3, 5)), same, max_mel_tokens=100, noise_seed=1, cfg_rate=0.0)
    bad = [pipe.submit(text((3, 6)), same, max_mel_tokens=100, noise_seed=1, **kw)
           for kw in (dict(diffusion_steps=[1, 2]), dict(diffusion_steps=0), dict(cfg_rate=-0.5), dict(cfg_rate=[0.1, float("inf")]))]
    for f in bad:
        with pytest.raises(ValueError):
            f.result(timeout=WAIT)
    for _ in range(5):                                  # the lane decodes a .. d (each queued before the next starts) and stands at e
        tts.decode_gate.wait()
        if tts.decode_gate.seen[-1] == 5:
            break
        tts.decode_gate.release()
    assert tts.decode_gate.seen == [1, 2, 3, 4, 5] and [r.done for r in pipe._aq] == [a, b, c, d]
    tts.acoustic_gate.open()
    assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1)) and torch.equal(d.result(timeout=WAIT)[0], wave(3, 4))
    assert [len(t) for t in b.result(timeout=WAIT)] == [2] and torch.equal(c.result(timeout=WAIT)[0], wave(3, 3))
    tts.decode_gate.open()
    assert torch.equal(e.result(timeout=WAIT)[0], wave(3, 5)) and torch.equal(x.result(timeout=WAIT)[0], wave(2, 9))
    pipe.close()
    assert tts.calls == [[(9, None, None)], [(1, 3, 0.7), (2, 1, 0.0), (2, 2, 0.0), (3, 2, 0.7), (4, 25, 0.7)], [(5, None, 0.0)]]
