"""Stand-ins for the preemption scheduler tests (tests/test_preempt_sched_cpu.py): the counting session of tests/cancel_standins.py
with `park` and `resume`.  A parked row is an object that carries the slot's counters, so a resumed row goes on where it stopped and
its result still names its owner; `to("cpu")` only notes where the row was sent.  Every parked row is also remembered by a weak
reference, so a test can see that a dropped one is really let go."""
import weakref

from cancel_standins import EvictSession


class Parked:
    def __init__(self, state, lane):
        self.state, self.lane, self.where, self.resumed = state, lane, "device", False

    def to(self, device):
        self.where = str(device)
        return self


class ParkSession(EvictSession):
    """EvictSession + park / resume.  `lane`: a name that goes into every park / resume log entry (which session did it);
    fail_resume: tags whose resume raises; parked: weak references to every row this session parked."""

    def __init__(self, slots, max_prompt, max_new, log, gate=None, lane=0, fail_resume=(), parked=None):
        super().__init__(slots, max_prompt, max_new, log, gate)
        self.lane, self.fail_resume = lane, set(fail_resume)
        self.parked = parked if parked is not None else []

    def park(self, slot):
        s = self.state[slot]
        assert s is not None and s["have"] < s["n"], "parked a slot that is free or has finished"
        self.state[slot] = None
        self.log.append(("park", self.lane, slot, s["tag"]))
        p = Parked(s, self.lane)
        self.parked.append(weakref.ref(p))
        return p

    def resume(self, parked, slot=None):
        assert isinstance(parked, Parked) and not parked.resumed, "resumed something that is no parked row, or twice"
        if parked.state["tag"] in self.fail_resume:
            raise RuntimeError(f"resume of {parked.state['tag']} refused")
        free = self.free_slots
        assert free, "resumed into a full session"
        slot = free[0] if slot is None else slot
        assert self.state[slot] is None
        parked.resumed = True
        self.state[slot] = parked.state
        self.log.append(("resume", self.lane, slot, parked.state["tag"], parked.where))
        return slot
