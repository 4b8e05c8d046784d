"""CPU: request cancellation in ContinuousPipeline and BatchPipeline -- where a cancelled (or failed, or expired) request is dropped,
which slots are evicted and when, the point of no return at the acoustic job, and that the neighbours of a cancelled request in a
merged acoustic batch keep their own results.  Driven by the stand-ins of tests/cancel_standins.py (no GPU, no kernels); every order
is fixed by gates inside the stand-ins' `step`, static decode and `acoustic_stage`."""
import concurrent.futures
import contextlib
import threading
from types import SimpleNamespace

import pytest
import torch

import cancel_standins as cs
from cancel_standins import EvictSession, FakeTTS, Gate, PlainSession, cond, text, wave
from indextts_amd import serving
from indextts_amd.serving import BatchPipeline, ContinuousPipeline

WAIT = cs.WAIT


def _pipe(tts, slots, log, gate, poll=1, session=EvictSession, **kw):
    return ContinuousPipeline(tts, slots=slots, poll_steps=poll, session_factory=lambda mp, mn: session(slots, mp, mn, log, gate), **kw)


def _submit_all(pipe, reqs, **kw):
    """Several requests queued as one: the lanes see all of them or none (submit takes the same, re-entrant, lock)."""
    with pipe._cv:
        return [pipe.submit(t, cond(), max_mel_tokens=100, **kw) for t in reqs]


def _sync(pipe, tag=99):
    """A request submitted now is decoded after everything the lane has been asked to do so far."""
    got = pipe.submit(text((1, tag)), cond(), max_mel_tokens=100).result(timeout=WAIT)
    assert torch.equal(got[0], wave(1, tag))


def _kinds(log):
    return [e[0] for e in log]


def test_cancel_while_waiting_is_never_admitted():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate) as pipe:
        a, b, c = _submit_all(pipe, [text((3, 1)), text((3, 2)), text((2, 3))])
        gate.wait()                                     # a is in the only slot, b and c wait
        assert pipe.cancel(b) is True
        gate.open()
        assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1))
        assert torch.equal(c.result(timeout=WAIT)[0], wave(2, 3))
        assert b.cancelled()
        assert b in concurrent.futures.wait([b], timeout=WAIT).done      # its waiters were told when it was dropped
    assert [e[2] for e in log if e[0] == "admit"] == [[1], [3]]
    assert "evict" not in _kinds(log)
    assert sorted(tts.acoustic_batches) == [[1], [3]]


def test_cancel_while_decoding_evicts_its_slots_and_admits_into_them_in_the_same_poll():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 2, log, gate) as pipe:
        a, b, c = _submit_all(pipe, [text((50, 1)), text((4, 2)), text((3, 3))])
        gate.wait()                                     # a in slot 0, b in slot 1, c waits
        assert log == [("admit", [0, 1], [1, 2])]
        assert pipe.cancel(a) is True
        gate.release()                                  # the step that was due runs; the next poll evicts, admits, and stands at the gate
        gate.wait()
        assert log[1:] == [("step", 1, [0, 1]), ("evict", [0]), ("admit", [0], [3])]
        gate.open()
        assert torch.equal(b.result(timeout=WAIT)[0], wave(4, 2))
        assert torch.equal(c.result(timeout=WAIT)[0], wave(3, 3))
        assert a.cancelled()
    assert _kinds(log).count("evict") == 1
    assert sum(1 for e in log if e[0] == "step") < 10      # nobody decoded a's 50 codes
    assert sorted(tts.acoustic_batches) == [[2], [3]]


def test_partly_admitted_job_two_rows_evicted_one_dropped():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 2, log, gate) as pipe:
        (a,) = _submit_all(pipe, [text((40, 1), (40, 2), (40, 3))])
        gate.wait()
        assert log == [("admit", [0, 1], [1, 2])]
        assert pipe.cancel(a) is True
        gate.open()
        _sync(pipe)
        assert a.cancelled()
    assert [e for e in log if e[0] == "evict"] == [("evict", [0, 1])]
    assert [e[2] for e in log if e[0] == "admit"] == [[1, 2], [99]]      # utterance 3 was never admitted
    assert tts.acoustic_batches == [[99]]


def test_cancel_after_decode_before_the_acoustic_job():
    """The only acoustic worker is held inside x's job while a finishes decoding and queues; a is cancelled there and never reaches
    the acoustic stage."""
    tts, log, gate = FakeTTS(), [], Gate()
    tts.acoustic_gate.armed = True
    with _pipe(tts, 2, log, gate) as pipe:
        x = pipe.submit(text((2, 7)), cond(), max_mel_tokens=100)
        tts.acoustic_gate.wait()                        # x's acoustic job has started
        a = pipe.submit(text((2, 1)), cond(), max_mel_tokens=100)
        gate.armed = True
        _submit_all(pipe, [text((30, 5))])              # the lane stands at the gate with this one: a was collected before
        gate.wait()
        gate.release()
        gate.wait()
        assert a in [j.done for j in pipe._aq]
        assert pipe.cancel(a) is True
        assert pipe.cancel(x) is False                  # past the point of no return
        gate.open()
        tts.acoustic_gate.open()
        assert torch.equal(x.result(timeout=WAIT)[0], wave(2, 7))
        _sync(pipe)
        assert a.cancelled()
    assert [1] not in tts.acoustic_batches and [7] in tts.acoustic_batches
    assert "evict" not in _kinds(log)                   # a had left its slot already


def test_cancel_returns_false_once_the_acoustic_job_has_started():
    tts, log = FakeTTS(), []
    tts.acoustic_gate.armed = True
    with _pipe(tts, 1, log, Gate()) as pipe:
        a = pipe.submit(text((3, 1)), cond(), max_mel_tokens=100)
        tts.acoustic_gate.wait()
        assert a.running()
        assert pipe.cancel(a) is False and a.cancel() is False
        tts.acoustic_gate.open()
        assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1))


def _queue_three_behind_a_blocker(pipe, tts, gate, **kw):
    """x holds the only acoustic worker; a, b, c decode and queue for the acoustic stage behind it.  Returns (x, a, b, c, long) with the lane
    standing at the gate and all three queued; `long` is a fourth request that is still decoding."""
    x = pipe.submit(text((2, 7)), cond(), max_mel_tokens=100, **kw)
    tts.acoustic_gate.wait()
    gate.armed = True
    same = cond()
    with pipe._cv:
        a, b, c = (pipe.submit(text((3, t)), same, max_mel_tokens=100, **kw) for t in (1, 2, 3))
        long = pipe.submit(text((30, 5)), same, max_mel_tokens=100, **kw)
    gate.wait()                                         # all four admitted
    gate.release()                                      # poll of 4 steps: a, b, c end and are collected together
    gate.wait()
    assert [j.done for j in pipe._aq] == [a, b, c]
    return x, a, b, c, long


def test_cancelling_the_middle_of_a_merged_acoustic_batch_leaves_its_neighbours_alone():
    """acoustic_coalesce = 3 and three queued requests: without the drop, set_result on the cancelled one raises InvalidStateError and
    the request behind it in the batch gets that exception instead of its waveform."""
    tts, log, gate = FakeTTS(), [], Gate()
    tts.acoustic_gate.armed = True
    with _pipe(tts, 4, log, gate, poll=4, acoustic_coalesce=3) as pipe:
        x, a, b, c, _ = _queue_three_behind_a_blocker(pipe, tts, gate, noise_seed=5)
        assert b.cancel() is True                       # the Future alone is the interface
        tts.acoustic_gate.open()                        # the lane still stands at its gate: nothing else joins the queue
        assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1))
        assert torch.equal(c.result(timeout=WAIT)[0], wave(3, 3))
        gate.open()
        assert torch.equal(x.result(timeout=WAIT)[0], wave(2, 7))
        assert b.cancelled()
    assert [1, 3] in tts.acoustic_batches               # merged, without the cancelled one
    assert not any(2 in tags for tags in tts.acoustic_batches)


def test_a_failure_in_a_merged_batch_still_fails_only_that_batch():
    """The exceptions of the others stay what they would have been: an acoustic failure reaches a and c, not the cancelled b."""
    tts, log, gate = FakeTTS(), [], Gate()
    tts.acoustic_gate.armed = True
    real = tts.acoustic_stage

    def failing(st, noise=None, noise_seeds=None):
        if int(st["codes"][0, 0]) // 1000 == 1:
            raise RuntimeError("vocoder fell over")
        return real(st, noise=noise, noise_seeds=noise_seeds)

    with _pipe(tts, 4, log, gate, poll=4, acoustic_coalesce=3) as pipe:
        x, a, b, c, _ = _queue_three_behind_a_blocker(pipe, tts, gate, noise_seed=5)
        tts.acoustic_stage = failing
        assert pipe.cancel(b) is True
        tts.acoustic_gate.open()
        for f in (a, c):
            with pytest.raises(RuntimeError, match="vocoder"):
                f.result(timeout=WAIT)
        gate.open()
        assert b.cancelled()
        with pytest.raises(concurrent.futures.CancelledError):
            b.result(timeout=WAIT)


def test_a_failed_jobs_rows_are_evicted_not_stepped_to_their_cap():
    """A three-utterance job in two slots: its short row ends, its bad third utterance fails the job at its admission, and the long
    second row (80 codes) is evicted at the next poll instead of being decoded to the end."""
    tts, log, gate = FakeTTS(), [], Gate()
    with _pipe(tts, 2, log, gate) as pipe:
        bad = pipe.submit(text((2, 1), (80, 2), (3, 950)), cond(), max_mel_tokens=100)
        with pytest.raises(IndexError):
            bad.result(timeout=WAIT)
        _sync(pipe)
        _sync(pipe, tag=98)
    assert ("evict", [1]) in log
    assert sum(1 for e in log if e[0] == "step" and 1 in e[2]) <= 3, log


def test_deadlines():
    """On the pipeline's clock: a request past its deadline is cancelled while it waits and while it decodes; one whose acoustic job
    has started completes."""
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    now = [100.0]
    with _pipe(tts, 1, log, gate) as pipe:
        pipe._clock = lambda: now[0]
        d, w = _submit_all(pipe, [text((60, 1))], deadline_s=5.0) + _submit_all(pipe, [text((3, 2))], deadline_s=5.0)
        keep = pipe.submit(text((2, 3)), cond(), max_mel_tokens=100, deadline_s=None)
        gate.wait()                                     # d decodes, w and keep wait
        now[0] += 4.0
        gate.release()
        gate.wait()
        assert not d.done() and not w.done()            # not yet
        now[0] += 2.0
        gate.open()
        assert torch.equal(keep.result(timeout=WAIT)[0], wave(2, 3))
        assert d.cancelled() and w.cancelled()
        assert ("evict", [0]) in log and [e[2] for e in log if e[0] == "admit"] == [[1], [3]]
        tts.acoustic_gate.armed = True
        late = pipe.submit(text((2, 4)), cond(), max_mel_tokens=100, deadline_s=5.0)
        tts.acoustic_gate.wait()                        # its acoustic job has started
        now[0] += 60.0
        assert pipe.cancel(late) is False
        tts.acoustic_gate.open()
        assert torch.equal(late.result(timeout=WAIT)[0], wave(2, 4))


def test_sessions_without_evict_work_while_nothing_is_cancelled():
    tts, log, gate = FakeTTS(), [], Gate()
    assert not hasattr(PlainSession, "evict")
    reqs = [text((2 + k % 5, 10 + k), (1 + k % 3, 30 + k)) if k % 2 else text((3 + k % 4, 10 + k)) for k in range(8)]
    with _pipe(tts, 3, log, gate, poll=2, session=PlainSession) as pipe:
        futs = [pipe.submit(t, cond(), max_mel_tokens=100) for t in reqs]
        results = [f.result(timeout=WAIT) for f in futs]
    for t, got in zip(reqs, results):
        assert len(got) == t.shape[0]
        for row, g in zip(t, got):
            n = int(row[0])
            assert torch.equal(g[:n], wave(n, int(row[1])))


def test_close_returns_with_cancelled_requests_in_every_stage():
    tts, log, gate = FakeTTS(), [], Gate()
    tts.acoustic_gate.armed = True
    pipe = _pipe(tts, 4, log, gate, poll=4, acoustic_coalesce=3)
    x, a, b, c, long = _queue_three_behind_a_blocker(pipe, tts, gate, noise_seed=5)      # a, b, c queued for the acoustic stage, `long` decoding
    waiting = _submit_all(pipe, [text((5, 20 + k)) for k in range(5)])                  # the lane stands at the gate: all five wait
    gone = [b, long] + waiting[:3]
    for f in gone:
        f.cancel()
    tts.acoustic_gate.open()
    gate.open()
    t = threading.Thread(target=pipe.close)
    t.start()
    t.join(WAIT)
    assert not t.is_alive(), "close() did not return"
    assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1)) and torch.equal(c.result(timeout=WAIT)[0], wave(3, 3))
    for k in (3, 4):
        assert torch.equal(waiting[k].result(timeout=WAIT)[0], wave(5, 20 + k))
    assert all(f.cancelled() for f in gone)
    assert ("evict", [3]) in log                        # `long` had the fourth slot


# ---- BatchPipeline: its scheduling needs streams and events only as tokens; a torch whose `cuda` is a stand-in lets it run here
class _Stream:
    cuda_stream = 1

    def __init__(self, device=None, priority=0):
        pass

    @staticmethod
    def priority_range():
        return 0, -1

    def wait_event(self, e):
        pass

    def wait_stream(self, s):
        pass

    def synchronize(self):
        pass


class _Event:
    def record(self, s=None):
        pass


class _Torch:
    class cuda:
        Stream, Event = _Stream, _Event
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


def test_batch_pipeline_merged_neighbours_and_accounting(hostonly):
    """x holds the only acoustic worker; a, b, c are decoded and queue behind it; the lane stands at d's decode.  b (the middle of the
    batch of three) and d are cancelled: a and c are merged and get their own waveforms, d's static decode runs to its end and its
    rows are dropped behind it, e -- cancelled while it waits -- is never decoded, and _running comes back to 0."""
    tts = FakeTTS()
    tts.acoustic_gate.armed = True
    same = cond()
    pipe = BatchPipeline(tts, decode_lanes=1, acoustic_workers=1, acoustic_coalesce=3)
    x = pipe.submit(text((2, 7)), same, max_mel_tokens=100, noise_seed=1)
    tts.acoustic_gate.wait()
    tts.decode_gate.armed = True
    a, b, c = (pipe.submit(text((3, t)), same, max_mel_tokens=100, noise_seed=1) for t in (1, 2, 3))
    d = pipe.submit(text((3, 4)), same, max_mel_tokens=100, noise_seed=1)
    for _ in range(4):                                  # the lane decodes a, b, c (each queued before the next starts) and stands at d
        tts.decode_gate.wait()
        if tts.decode_gate.seen[-1] == 4:
            break
        tts.decode_gate.release()
    assert tts.decode_gate.seen == [1, 2, 3, 4] and [r.done for r in pipe._aq] == [a, b, c]
    e = pipe.submit(text((3, 5)), same, max_mel_tokens=100, noise_seed=1)
    assert b.cancel() is True and pipe.cancel(d) is True and pipe.cancel(e) is True
    assert pipe.cancel(x) is False
    assert [r.done for r in pipe._queue] == []          # pipe.cancel dropped e at once
    tts.decode_gate.open()
    tts.acoustic_gate.open()
    assert torch.equal(a.result(timeout=WAIT)[0], wave(3, 1))
    assert torch.equal(c.result(timeout=WAIT)[0], wave(3, 3))
    assert torch.equal(x.result(timeout=WAIT)[0], wave(2, 7))
    # what submit refuses: a bad takes / keep raises there; a bad noise or noise_seed, or a conditioning that cannot be repeated per
    # take, fails that request's Future only -- and none of them is ever queued
    sampled = {"do_sample": True}
    for kw in (dict(takes=0), dict(takes=2), dict(takes=2, sampling={"do_sample": False}), dict(keep=1), dict(sampling=sampled, takes=2, keep=3),
               dict(sampling=sampled, takes=2, keep=0), dict(sampling={"do_sample": True, "num_beams": 2}, takes=2, keep=1)):
        with pytest.raises(ValueError):
            pipe.submit(text((3, 6)), same, max_mel_tokens=100, **kw)
    per_row = SimpleNamespace(spk_cond_latent=torch.zeros(2, 3, 4), emo_vec=torch.zeros(2, 4))
    for c, kw in ((same, dict(noise=torch.zeros(1, 2, 3), noise_seed=1)), (same, dict(noise_seed=[1, 2])), (same, dict(noise_seed=-1)),
                  (same, dict(noise_seed="x")), (per_row, dict(sampling=sampled, takes=2, noise_seed=1))):
        bad = pipe.submit(text((3, 6)), c, max_mel_tokens=100, **kw)
        with pytest.raises(ValueError):
            bad.result(timeout=WAIT)
    assert [r.done for r in pipe._queue] == []
    pipe.close()
    assert b.cancelled() and d.cancelled() and e.cancelled()
    assert concurrent.futures.wait([b, d, e], timeout=WAIT).not_done == set()
    assert tts.acoustic_batches == [[7], [1, 3]]
    assert tts.decode_gate.seen == [1, 2, 3, 4]         # e never reached the decode
    assert pipe._running == 0
