"""Stand-ins for the group preemption scheduler tests (tests/test_preempt_groups_sched_cpu.py): the counting session of
tests/preempt_standins.py with a beam session's interface -- `free_groups`, `admit(rows, caps, beam=...)`, `park_group` and
`resume_group`.  The row calls `park` / `resume` raise NotImplementedError as BeamDecodeSession's do, so a pipeline that used them
on a beam session would fail its requests.  A place of the counting session stands for a group."""
import weakref

from preempt_standins import Parked, ParkSession


class ParkedGroupStandIn(Parked):
    pass


class GroupParkSession(ParkSession):
    def __init__(self, groups, max_prompt, max_new, log, gate=None, lane=0, fail_resume=(), parked=None, fail_park=()):
        super().__init__(groups, max_prompt, max_new, log, gate, lane, fail_resume, parked)
        self.fail_park = set(fail_park)
        self.beams = []                     # the `beam` entries of every admission, in order

    @property
    def free_groups(self):
        return super().free_slots

    @property
    def free_slots(self):
        raise AssertionError("a beam pipeline asks for free_groups")

    def admit(self, rows, caps, beam=None):
        assert beam is not None and len(beam) == len(rows), "a beam pipeline admits with one beam entry per request"
        self.beams.extend(beam)
        free = self.free_groups
        assert 1 <= len(rows) <= len(free), "admitted more requests than free groups"
        ids = free[: len(rows)]
        for s, r, c in zip(ids, rows, caps):
            self.state[s] = {"n": min(int(r[0, 0]), int(c)), "have": 1, "tag": int(r[1, 0])}
        self.log.append(("admit", ids, [self.state[s]["tag"] for s in ids]))
        return ids

    def park(self, slot):
        raise NotImplementedError("one row of a beam group cannot leave it")

    def resume(self, parked, slot=None):
        raise NotImplementedError("a beam session resumes whole groups")

    def park_group(self, group):
        s = self.state[group]
        assert s is not None and s["have"] < s["n"], "parked a group that is free or has finished"
        if s["tag"] in self.fail_park:
            raise RuntimeError(f"park of {s['tag']} refused")
        self.state[group] = None
        self.log.append(("park", self.lane, group, s["tag"]))
        p = ParkedGroupStandIn(s, self.lane)
        self.parked.append(weakref.ref(p))
        return p

    def resume_group(self, parked, group=None):
        assert isinstance(parked, ParkedGroupStandIn) and not parked.resumed, "resumed something that is no parked group, or twice"
        if parked.state["tag"] in self.fail_resume:
            raise RuntimeError(f"resume of {parked.state['tag']} refused")
        free = self.free_groups
        assert free, "resumed into a full session"
        group = free[0] if group is None else group
        assert self.state[group] is None
        parked.resumed = True
        self.state[group] = parked.state
        self.log.append(("resume", self.lane, group, parked.state["tag"], parked.where))
        return group
