"""CPU: preemption in a beam ContinuousPipeline (`num_beams > 1, preempt_groups=True`) -- which groups a lane parks for an urgent
request and how many, that the pipeline speaks to its session through `park_group` / `resume_group` (the row calls raise, as
BeamDecodeSession's do), that parked groups come back ahead of later arrivals of their priority on whichever lane has room, what
happens to a parked request that is cancelled, expires or cannot be parked or resumed, and the two constructor rules.  Driven by the
stand-ins of tests/preempt_group_standins.py (no GPU, no kernels); every order is fixed by the gate inside the stand-ins' `step`.
Also: the ctypes mirror of idxtts_park_group_header against the layout include/idxtts.h documents."""
import ctypes
import gc
import os
import re
import threading

import pytest
import torch

import cancel_standins as cs
from cancel_standins import FakeTTS, Gate, cond, text, wave
from indextts_amd import _lib
from indextts_amd.serving import ContinuousPipeline
from preempt_group_standins import GroupParkSession

WAIT = cs.WAIT
NB = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pipe(tts, groups, log, gate, poll=1, **kw):
    ses = {k: kw.pop(k) for k in ("fail_resume", "fail_park", "parked") if k in kw}
    kw.setdefault("preempt_groups", True)
    return ContinuousPipeline(tts, slots=groups * NB, num_beams=NB, poll_steps=poll,
                              session_factory=lambda mp, mn: GroupParkSession(groups, mp, mn, log, gate, **ses), **kw)


def _submit(pipe, rows, **kw):
    return pipe.submit(text(*rows), cond(), max_mel_tokens=100, sampling={"num_beams": NB, "do_sample": False}, **kw)


def _sync(pipe, tag=99):
    assert torch.equal(_submit(pipe, [(1, tag)]).result(timeout=WAIT)[0], wave(1, tag))


def _of(log, *kinds):
    return [e for e in log if e[0] in kinds]


def test_urgent_request_parks_the_lowest_priority_last_admitted_group():
    """Three groups decode (priorities 1, 0, 0); an urgent request and a later arrival of priority 0 come in: exactly one group is
    parked -- through park_group -- the one of priority 0 admitted last; the urgent request is admitted in that poll; the parked group
    comes back through resume_group, before the later arrival of its own priority, and never by a second admission."""
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 3, log, gate) as pipe:
        with pipe._cv:
            a, b, c = _submit(pipe, [(12, 1)]), _submit(pipe, [(12, 2)], priority=1), _submit(pipe, [(12, 3)])
        gate.wait()
        assert log == [("admit", [0, 1, 2], [2, 1, 3])]
        with pipe._cv:
            u, d = _submit(pipe, [(2, 9)], priority=5), _submit(pipe, [(2, 4)])
        gate.release()
        gate.wait()
        assert log[1:] == [("step", 1, [0, 1, 2]), ("park", 0, 2, 3), ("admit", [2], [9])]
        gate.release()
        gate.wait()
        assert log[4:] == [("step", 1, [0, 1, 2]), ("resume", 0, 2, 3, "device")]
        assert torch.equal(u.result(timeout=WAIT)[0], wave(2, 9))
        gate.open()
        for f, (n, tag) in ((a, (12, 1)), (b, (12, 2)), (c, (12, 3)), (d, (2, 4))):
            assert torch.equal(f.result(timeout=WAIT)[0], wave(n, tag))
    assert len(_of(log, "park")) == 1 and len(_of(log, "resume")) == 1
    assert [e[2] for e in _of(log, "admit")] == [[2, 1, 3], [9], [4]]


def test_no_more_groups_are_parked_than_urgent_utterances_wait():
    tts, log, gate, trace = FakeTTS(), [], Gate(armed=True), []
    with _pipe(tts, 3, log, gate) as pipe:
        pipe.trace = trace
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
    moves = [(e[0], e[2], e[3]) for e in trace if e[0] in ("park", "resume")]
    assert moves == [("park", 2, 0), ("park", 0, 0), ("resume", 0, 0), ("resume", 2, 0)]


def test_equal_priority_never_preempts_and_default_pipeline_parks_nothing():
    """preempt_groups=True with an arrival of the SAME priority as the groups decoding parks nothing; a beam pipeline built without
    preempt_groups orders its queue by priority and parks nothing either."""
    for on in (False, True):
        tts, log, gate = FakeTTS(), [], Gate(armed=True)
        with _pipe(tts, 1, log, gate, preempt_groups=on) as pipe:
            a = _submit(pipe, [(3, 1)], priority=2)
            gate.wait()
            with pipe._cv:
                b, c, d = _submit(pipe, [(2, 2)]), _submit(pipe, [(2, 3)], priority=2), _submit(pipe, [(2, 4)], priority=1 if on else 9)
            gate.open()
            for f, (n, tag) in ((a, (3, 1)), (b, (2, 2)), (c, (2, 3)), (d, (2, 4))):
                assert torch.equal(f.result(timeout=WAIT)[0], wave(n, tag))
        assert [e[2] for e in _of(log, "admit")] == ([[1], [3], [4], [2]] if on else [[1], [4], [3], [2]])
        assert not _of(log, "park", "resume")


def test_a_group_parked_on_one_lane_resumes_on_the_other_from_host_memory():
    tts, log, gates, sessions, lock = FakeTTS(), [], [Gate(armed=True), Gate(armed=True)], [], threading.Lock()

    def factory(mp, mn):
        with lock:
            s = GroupParkSession(1, mp, mn, log, gates[len(sessions)], lane=len(sessions))
            sessions.append(s)
        return s
    with ContinuousPipeline(tts, slots=NB, num_beams=NB, decode_lanes=2, poll_steps=1, session_factory=factory, preempt_groups=True,
                            park_to="host") as pipe:
        with pipe._cv:
            a, b = _submit(pipe, [(30, 1)]), _submit(pipe, [(30, 2)])
        gates[0].wait()
        gates[1].wait()
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


@pytest.mark.parametrize("how", ["cancel", "deadline"])
def test_a_parked_request_that_is_gone_is_dropped_not_resumed(how):
    tts, log, gate, parked, now = FakeTTS(), [], Gate(armed=True), [], [0.0]
    with _pipe(tts, 1, log, gate, parked=parked) as pipe:
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
        assert parked[0]() is None, "the dropped request's parked group is still held"
    assert not _of(log, "resume") and [e[2] for e in _of(log, "admit")] == [[1], [9], [99], [98]]


def test_a_failing_resume_or_park_fails_only_its_request():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate, fail_resume={1}) as pipe:
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
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate, fail_park={1}) as pipe:
        a = _submit(pipe, [(30, 1)])
        gate.wait()
        u = _submit(pipe, [(2, 9)], priority=1)
        gate.open()
        assert torch.equal(u.result(timeout=WAIT)[0], wave(2, 9))      # the group was freed by eviction: the urgent request still got it
        assert isinstance(a.exception(timeout=WAIT), RuntimeError) and "park of 1 refused" in str(a.exception())
    assert not _of(log, "park", "resume") and ("evict", [0]) in log


def test_close_drains_parked_groups():
    tts, log, gate = FakeTTS(), [], Gate(armed=True)
    with _pipe(tts, 1, log, gate) as pipe:
        a = _submit(pipe, [(6, 1)])
        gate.wait()
        u = _submit(pipe, [(2, 9)], priority=1)
        gate.release()
        gate.wait()
        assert _of(log, "park") == [("park", 0, 0, 1)]
        gate.open()
    assert a.done() and torch.equal(a.result()[0], wave(6, 1)) and torch.equal(u.result()[0], wave(2, 9))
    assert len(_of(log, "resume")) == 1


def test_constructor_rules():
    tts = FakeTTS()
    with pytest.raises(ValueError, match="num_beams"):
        ContinuousPipeline(tts, slots=4, preempt_groups=True, session_factory=lambda mp, mn: None)
    with pytest.raises(ValueError, match="num_beams"):
        ContinuousPipeline(tts, slots=4, num_beams=2, preempt=True, preempt_groups=True, session_factory=lambda mp, mn: None)
    with pytest.raises(ValueError, match="park_to"):
        ContinuousPipeline(tts, slots=4, num_beams=2, preempt_groups=True, park_to="disk", session_factory=lambda mp, mn: None)


def test_group_header_mirror_matches_the_documented_layout():
    """128 bytes, every field where the struct in include/idxtts.h puts it (natural alignment, in declaration order), a magic of its
    own, and the row header untouched."""
    H = _lib.ParkGroupHeaderC
    assert ctypes.sizeof(H) == 128 and ctypes.sizeof(_lib.ParkHeaderC) == 128
    want = [("magic", 0, 4), ("version", 4, 4), ("layers", 8, 4), ("heads", 12, 4), ("model_dim", 16, 4), ("number_mel_codes", 20, 4),
            ("slots", 24, 4), ("num_beams", 28, 4), ("kv_format", 32, 4), ("gemm_mode", 36, 4), ("pos", 40, 4), ("mel_pos", 44, 4),
            ("step", 48, 4), ("max_step", 52, 4), ("do_sample", 56, 4), ("temperature", 60, 4), ("top_k", 64, 4), ("top_p", 68, 4),
            ("length_penalty", 72, 8), ("early_stopping", 80, 4), ("batch_invariant", 84, 4), ("seed", 88, 8), ("exp_noise", 96, 8),
            ("hyp_n", 104, 4), ("done", 108, 4), ("bytes", 112, 8), ("reserved", 120, 8)]
    assert [(n, getattr(H, n).offset, getattr(H, n).size) for n, _ in H._fields_] == want
    assert dict(H._fields_)["length_penalty"] is ctypes.c_double
    # the header text declares the same names in the same order
    src = open(os.path.join(ROOT, "include", "idxtts.h")).read()
    body = re.search(r"typedef struct idxtts_park_group_header \{(.*?)\} idxtts_park_group_header;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^\s*(unsigned long long|unsigned|int|float|double)\s+", "", decl.strip())
        names += [re.sub(r"\[\d+\]", "", n.strip()) for n in decl.split(",") if n.strip()]
    assert names == [n for n, _, _ in want]
    magic = int(re.search(r"#define IDXTTS_PARK_GROUP_MAGIC (0x[0-9a-f]+)u", src).group(1), 16)
    row_magic = int(re.search(r"#define IDXTTS_PARK_MAGIC (0x[0-9a-f]+)u", src).group(1), 16)
    assert magic == _lib.PARK_GROUP_MAGIC and row_magic == _lib.PARK_MAGIC and magic != row_magic
    assert re.search(r"#define IDXTTS_PARK_VERSION 1\b", src)
