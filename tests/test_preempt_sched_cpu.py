"""CPU: priorities and preemption in ContinuousPipeline -- the order of the waiting queue, which rows a lane parks for an urgent
request and how many, that the urgent request is admitted in the same poll, that parked rows come back through `resume` (on whichever
lane has room) ahead of later arrivals of their priority, and what happens to a parked request that is cancelled, expires or cannot
be resumed.  Driven by the stand-ins of tests/preempt_standins.py (no GPU, no kernels); every order is fixed by the gate inside the
stand-ins' `step`, never by sleeping."""
import gc
import threading

import pytest
import torch

import cancel_standins as cs
from cancel_standins import FakeTTS, Gate, cond, text, wave
from indextts_amd.serving import ContinuousPipeline
from preempt_standins import ParkSession

WAIT = cs.WAIT


def _pipe(tts, slots, log, gate, poll=1, **kw):
    ses = {k: kw.pop(k) for k in ("fail_resume", "parked") if k in kw}
    return ContinuousPipeline(tts, slots=slots, poll_steps=poll, session_factory=lambda mp, mn: ParkSession(slots, mp, mn, log, gate, **ses),
                              **kw)


def _submit(pipe, rows, **kw):
    return pipe.submit(text(*rows), cond(), max_mel_tokens=100, **kw)


def _sync(pipe, tag=99):
    got = _submit(pipe, [(1, tag)]).result(timeout=WAIT)
    assert torch.equal(got[0], wave(1, tag))


def _of(log, *kinds):
    return [e for e in log if e[0] in kinds]


@pytest.mark.parametrize("preempt", [False, True])
def test_equal_priorities_are_fifo(preempt):
    """With every priority equal (0, or any other one value) the admissions are those of a pipeline built without the new arguments."""
    reqs = [[(5, 1), (3, 2)], [(4, 3)], [(2, 4), (6, 5), (3, 6)], [(3, 7)]]

    def run(submit_kw, **kw):
        tts, log = FakeTTS(), []
        with _pipe(tts, 2, log, Gate(), **kw) as pipe:
            with pipe._cv:
                futs = [_submit(pipe, r, **submit_kw) for r in reqs]
            for f, r in zip(futs, reqs):
                got = f.result(timeout=WAIT)
                assert all(torch.equal(g[: u[0]], wave(*u)) for g, u in zip(got, r))      # (rows of a request are padded to its longest)
        assert not _of(log, "park", "resume")
        return _of(log, "admit")
    fifo = run({})
    assert [t for e in fifo for t in e[2]] == [1, 2, 3, 4, 5, 6, 7]
    assert run({}, preempt=preempt) == fifo
    assert run({"priority": 7}, preempt=preempt) == fifo


def test_urgent_request_parks_the_lowest_priority_last_admitted_row():
    """Three rows decode (priorities 1, 0, 0), an urgent request and a later arrival of priority 0 come in: exactly one row is parked,
    the one of priority 0 that was admitted last; the urgent request is admitted in that poll; the parked row comes back through
    resume, before the later arrival of its own priority."""
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 3, log, gate, preempt=True) as pipe:
        with pipe._cv:
            a, b, c = _submit(pipe, [(12, 1)]), _submit(pipe, [(12, 2)], priority=1), _submit(pipe, [(12, 3)])
        gate.wait()
        assert log == [("admit", [0, 1, 2], [2, 1, 3])]              # b first: the queue is ordered by priority
        with pipe._cv:
            u, d = _submit(pipe, [(2, 9)], priority=5), _submit(pipe, [(2, 4)])
        gate.release()
        gate.wait()
        assert log[1:] == [("step", 1, [0, 1, 2]), ("park", 0, 2, 3), ("admit", [2], [9])]
        gate.release()                                               # u ends in this step; the next poll has one free slot
        gate.wait()
        assert log[4:] == [("step", 1, [0, 1, 2]), ("resume", 0, 2, 3, "device")]
        assert torch.equal(u.result(timeout=WAIT)[0], wave(2, 9))
        gate.open()
        for f, (n, tag) in ((a, (12, 1)), (b, (12, 2)), (c, (12, 3)), (d, (2, 4))):
            assert torch.equal(f.result(timeout=WAIT)[0], wave(n, tag))
    assert len(_of(log, "park")) == 1 and len(_of(log, "resume")) == 1
    assert [e[2] for e in _of(log, "admit")] == [[2, 1, 3], [9], [4]]  # c came back by resume, never by a second admit


def test_no_more_rows_are_parked_than_urgent_utterances_wait():
    """Two urgent utterances and three rows of lower priority: two are parked -- priority 0 before priority 1, the later admission
    first -- and both come back in submission order."""
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 3, log, gate, preempt=True) as pipe:
        with pipe._cv:
            a, b, c = _submit(pipe, [(9, 1)]), _submit(pipe, [(9, 2)], priority=1), _submit(pipe, [(9, 3)])
        gate.wait()
        u = _submit(pipe, [(2, 8), (2, 9)], priority=5)
        gate.release()
        gate.wait()
        assert log[1:] == [("step", 1, [0, 1, 2]), ("park", 0, 2, 3), ("park", 0, 1, 1), ("admit", [1, 2], [8, 9])]
        gate.release()
        gate.wait()
        assert log[5:] == [("step", 1, [0, 1, 2]), ("resume", 0, 1, 1, "device"), ("resume", 0, 2, 3, "device")]
        gate.open()
        got = u.result(timeout=WAIT)
        assert torch.equal(got[0], wave(2, 8)) and torch.equal(got[1], wave(2, 9))
        for f, tag in ((a, 1), (b, 2), (c, 3)):
            assert torch.equal(f.result(timeout=WAIT)[0], wave(9, tag))
    assert len(_of(log, "park")) == 2


def test_equal_priority_never_preempts_and_priority_orders_the_queue():
    """preempt=False: priorities reorder the waiting utterances and nothing is parked.  preempt=True with an arrival of the SAME
    priority as the rows decoding: nothing is parked either."""
    for preempt in (False, True):
        tts, log, gate = FakeTTS(), [], Gate(armed=True)
        with _pipe(tts, 1, log, gate, preempt=preempt) as pipe:
            a = _submit(pipe, [(3, 1)], priority=2)
            gate.wait()
            with pipe._cv:
                b, c, d = _submit(pipe, [(2, 2)]), _submit(pipe, [(2, 3)], priority=2), _submit(pipe, [(2, 4)], priority=1)
            gate.open()
            for f, (n, tag) in ((a, (3, 1)), (b, (2, 2)), (c, (2, 3)), (d, (2, 4))):
                assert torch.equal(f.result(timeout=WAIT)[0], wave(n, tag))
        assert [e[2] for e in _of(log, "admit")] == [[1], [3], [4], [2]]
        assert not _of(log, "park", "resume")


def test_a_row_parked_on_one_lane_resumes_on_the_other():
    """Two lanes of one slot each, both busy; the lane that is let go parks its row for the urgent request; the other lane's request is
    cancelled, and the parked row -- moved to host memory: park_to="host" -- resumes there."""
    tts, log, gates, sessions, lock = FakeTTS(), [], [Gate(armed=True), Gate(armed=True)], [], threading.Lock()

    def factory(mp, mn):
        with lock:
            s = ParkSession(1, mp, mn, log, gates[len(sessions)], lane=len(sessions))
            sessions.append(s)
        return s
    with ContinuousPipeline(tts, slots=1, decode_lanes=2, poll_steps=1, session_factory=factory, preempt=True, park_to="host") as pipe:
        with pipe._cv:
            a, b = _submit(pipe, [(30, 1)]), _submit(pipe, [(30, 2)])
        gates[0].wait()
        gates[1].wait()                                              # one row in each lane's only slot
        la = next(k for k in (0, 1) if sessions[k].state[0]["tag"] == 1)
        lb = 1 - la
        u = _submit(pipe, [(2, 9)], priority=3)
        gates[la].release()
        gates[la].wait()
        assert _of(log, "park") == [("park", la, 0, 1)] and sessions[la].state[0]["tag"] == 9
        assert pipe.cancel(b) is True
        gates[lb].release()
        gates[lb].wait()
        assert _of(log, "resume") == [("resume", lb, 0, 1, "cpu")] and ("evict", [0]) in log
        for g in gates:
            g.open()
        assert torch.equal(a.result(timeout=WAIT)[0], wave(30, 1))
        assert torch.equal(u.result(timeout=WAIT)[0], wave(2, 9))
        assert b.cancelled()
    assert len(_of(log, "park")) == 1 and len(_of(log, "resume")) == 1


@pytest.mark.parametrize("how", ["cancel", "deadline"])
def test_a_parked_request_that_is_gone_is_dropped_not_resumed(how):
    tts, log, gate, parked, now = FakeTTS(), [], Gate(armed=True), [], [0.0]
    with _pipe(tts, 1, log, gate, preempt=True, parked=parked) as pipe:
        pipe._clock = lambda: now[0]
        a = _submit(pipe, [(30, 1)], deadline_s=10.0 if how == "deadline" else None)
        gate.wait()
        u = _submit(pipe, [(3, 9)], priority=1)
        gate.release()
        gate.wait()
        assert _of(log, "park") == [("park", 0, 0, 1)] and len(parked) == 1 and parked[0]() is not None
        if how == "cancel":
            assert pipe.cancel(a) is True
        else:
            now[0] = 11.0
        gate.open()
        assert torch.equal(u.result(timeout=WAIT)[0], wave(3, 9))
        _sync(pipe)
        _sync(pipe, 98)
        assert a.cancelled()
        gc.collect()
        assert parked[0]() is None, "the dropped request's parked row is still held"
    assert not _of(log, "resume") and [e[2] for e in _of(log, "admit")] == [[1], [9], [99], [98]]
    assert sorted(tts.acoustic_batches) == [[9], [98], [99]]


def test_a_failing_resume_fails_only_its_request():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate, preempt=True, fail_resume={1}) as pipe:
        a = _submit(pipe, [(30, 1)])
        gate.wait()
        with pipe._cv:
            u, d = _submit(pipe, [(2, 9)], priority=1), _submit(pipe, [(2, 4)])
        gate.open()
        assert torch.equal(u.result(timeout=WAIT)[0], wave(2, 9))
        assert isinstance(a.exception(timeout=WAIT), RuntimeError) and "refused" in str(a.exception())
        assert torch.equal(d.result(timeout=WAIT)[0], wave(2, 4))
        _sync(pipe)
    assert len(_of(log, "park")) == 1 and not _of(log, "resume")


def test_close_drains_parked_rows():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate, preempt=True) as pipe:
        a = _submit(pipe, [(6, 1)])
        gate.wait()
        u = _submit(pipe, [(2, 9)], priority=1)
        gate.release()
        gate.wait()
        assert _of(log, "park") == [("park", 0, 0, 1)]
        gate.open()
    assert a.done() and torch.equal(a.result()[0], wave(6, 1)) and torch.equal(u.result()[0], wave(2, 9))
    assert len(_of(log, "resume")) == 1


def test_constructor_refusals():
    tts = FakeTTS()
    with pytest.raises(ValueError, match="num_beams"):
        ContinuousPipeline(tts, slots=4, num_beams=2, preempt=True, session_factory=lambda mp, mn: None)
    for bad in ("disk", "cpu", None):
        with pytest.raises(ValueError, match="park_to"):
            ContinuousPipeline(tts, slots=4, park_to=bad, session_factory=lambda mp, mn: None)
