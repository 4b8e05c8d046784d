"""Stand-ins for the cancellation scheduler tests (tests/test_cancel_sched_cpu.py): a decode session with a counter per slot, an
`evict` and a log of every call, and a TTS whose stages return full states, so merged acoustic batches work.  Gates inside `step`, the
static decode and `acoustic_stage` let a test stop a worker at a known place: orders are fixed by events, never by sleeping.

The fake model: a request row is text [n, tag, ...] -- it decodes to n codes (its cap permitting), 1000 * tag + 0, 1, 2, ...; its
"waveform" is its row of codes, so every request's result names its owner."""
import threading
from types import SimpleNamespace

import torch

from indextts_amd.config import GPTConfig

CFG = GPTConfig.tiny()
WAIT = 30.0      # no wait in these tests is expected to take this long: a failure, not a hang


class Gate:
    """While armed, a worker that calls pause() reports its arrival and blocks until the test releases it."""

    def __init__(self, armed=False):
        self.armed = armed
        self._arrived = threading.Semaphore(0)
        self._go = threading.Semaphore(0)
        self.seen = []

    def pause(self, what=None):
        if self.armed:
            self.seen.append(what)
            self._arrived.release()
            assert self._go.acquire(timeout=WAIT), "the test never released the gate"

    def wait(self):
        """Blocks until a worker stands at the gate."""
        assert self._arrived.acquire(timeout=WAIT), "no worker reached the gate"

    def release(self):
        self._go.release()

    def open(self):
        """Disarms the gate and lets a worker standing at it go."""
        self.armed = False
        self._go.release()


class PlainSession:
    """admit / step / take / free_slots / close: the session interface from before eviction."""

    def __init__(self, slots, max_prompt, max_new, log, gate=None):
        self.slots, self.max_prompt, self.max_new = slots, max_prompt, max_new
        self.state = [None] * slots          # per slot: {"n": target, "have": produced, "tag": owner}
        self.log, self.gate = log, gate or Gate()
        self.closed = False

    @property
    def free_slots(self):
        return [i for i, s in enumerate(self.state) if s is None]

    def admit(self, rows, caps):
        free = self.free_slots
        assert 1 <= len(rows) <= len(free), "admitted more rows than free slots"
        ids = free[: len(rows)]
        for s, r, c in zip(ids, rows, caps):
            self.state[s] = {"n": min(int(r[0, 0]), int(c)), "have": 1, "tag": int(r[1, 0])}
        self.log.append(("admit", ids, [self.state[s]["tag"] for s in ids]))
        return ids

    def _ended(self):
        return [i for i, s in enumerate(self.state) if s is not None and s["have"] >= s["n"]]

    def step(self, n=1):
        self.gate.pause("step")
        live = [i for i, s in enumerate(self.state) if s is not None and s["have"] < s["n"]]
        self.log.append(("step", n, live))
        for i in live:
            self.state[i]["have"] = min(self.state[i]["have"] + n, self.state[i]["n"])
        return self._ended()

    def take(self, slot):
        s = self.state[slot]
        assert s is not None and s["have"] >= s["n"], "took a slot that has not finished"
        self.state[slot] = None
        return 1000 * s["tag"] + torch.arange(s["have"], dtype=torch.long)

    def close(self):
        self.closed = True


class EvictSession(PlainSession):
    def evict(self, ids):
        ids = list(ids)
        assert ids and all(self.state[i] is not None for i in ids), "evicted a slot that holds no request"
        self.log.append(("evict", sorted(ids)))
        for i in ids:
            self.state[i] = None


class Wave(torch.Tensor):
    """A result row: a tensor whose record_stream (the hand-over to the caller's stream) needs no device."""

    def record_stream(self, stream):
        pass


def wave(n, tag, cap=10 ** 6):
    """What a request row [n, tag] comes back as."""
    return 1000 * tag + torch.arange(min(n, cap), dtype=torch.long)


class FakeGPT:
    MAX_WORKSPACES = 1
    weight_format = "f32"

    def conds_latent(self, lat, emo):
        return lat

    def prompt_rows(self, conds, text):
        if int(text.max()) > 900:
            raise IndexError("text token id out of range")
        return [t.float()[:, None].expand(-1, 4) for t in text]


class FakeTTS:
    """gpt_stage (static decode, or codes= for the latent pass) and acoustic_stage with the real states' keys."""

    def __init__(self, device="cpu"):
        self.cfg = SimpleNamespace(gpt=CFG)
        self.device = device
        self.gpt = FakeGPT()
        self.decode_gate, self.acoustic_gate = Gate(), Gate()
        self.acoustic_batches = []          # the owners (tags) of every acoustic batch, in call order
        self.lock = threading.Lock()

    def gpt_stage(self, text, cond, max_mel_tokens, repetition_penalty, sampling=None, codes=None):
        text = torch.as_tensor(text)
        if codes is None:                   # BatchPipeline: the static decode of the whole batch
            self.decode_gate.pause(int(text[0, 1]))
            rows = [wave(int(t[0]), int(t[1]), max_mel_tokens) for t in text]
            n = max(r.shape[0] for r in rows)
            codes = torch.zeros(len(rows), n, dtype=torch.long)
            for i, r in enumerate(rows):
                codes[i, : r.shape[0]] = r
            lens = [int(r.shape[0]) for r in rows]
        else:
            lens = [int(codes.shape[1])] * int(codes.shape[0])
        assert codes.shape[0] == text.shape[0]
        B = int(codes.shape[0])
        return {"cond": cond, "B": B, "codes": codes, "code_lens": lens, "code_lens_t": torch.tensor(lens), "times": {},
                "latent": torch.zeros(B, codes.shape[1], 2)}

    def acoustic_stage(self, st, noise=None, noise_seeds=None):
        tags = [int(row[0]) // 1000 for row in st["codes"]]
        self.acoustic_gate.pause(tags)
        with self.lock:
            self.acoustic_batches.append(tags)
        return [row[:n].clone().as_subclass(Wave) for row, n in zip(st["codes"], st["code_lens"])]      # each row at its own length


def cond():
    c = SimpleNamespace(spk_cond_latent=torch.zeros(1, 3, 4), emo_vec=torch.zeros(1, 4))
    c.to = lambda dev: c
    return c


def text(*rows):
    """One request: a (n, tag) pair per utterance."""
    return torch.tensor([[n, tag] for n, tag in rows], dtype=torch.long)
