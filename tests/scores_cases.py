"""Scores (include/idxtts.h "Scores"): the float64 reference of the per-code log-probability, of the sequence score and of the
ranking of takes, the bound the kernels are held to, the crafted logit rows, and the byte layout of a parked row with and without the
log-probability segment.  No GPU here: tests/test_scores_cases_cpu.py checks this file against the package's host functions,
the tests/test_scores_*_gpu.py files check the kernels against it."""
import math

import numpy as np

import sampler_cases as sc

VOCABS = (8194, 130)      # the real size (2 * 4096 + 2 = 8 * 1024 + 2: the last trip of either loop holds two ids); below one id per thread
BATCHES = (1, 3, 16)
STEPS = 12


def bound(ref):
    """|lp - ref| <= 1e-5 + 2^-22 |ref|: twice what the arithmetic allows -- V positive terms summed at depth <= 26 in fp32 (each
    thread's <= 9 terms, 6 butterfly levels, 15 wave additions), expf and logf at 1-2 ulp, the subtraction's rounding: about
    5e-6 + 2^-23 |ref|."""
    return 1e-5 + 2.0 ** -22 * np.abs(ref)


def ref_logprobs(logits) -> np.ndarray:
    """float64 log-softmax over the last axis of fp32 logits (taken exactly)."""
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(axis=-1, keepdims=True)
    return (l - m) - np.log(np.exp(l - m).sum(axis=-1, keepdims=True))


def ref_logprob(logits_row, tok: int) -> float:
    return float(ref_logprobs(logits_row)[int(tok)])


def ref_sequence_score(lp, n: int, length_penalty: float = 1.0) -> float:
    """(sum_{t < n} lp[t]) / n ** length_penalty, float64, index order."""
    tot = 0.0
    for t in range(int(n)):
        tot += float(np.float32(lp[t]))
    return tot / float(n) ** float(length_penalty)


def ref_rank(scores, stopped) -> list:
    """Stopped first, then the higher score, then the lower take index -- written as a selection, not as a sort key."""
    left = list(range(len(scores)))
    out = []
    while left:
        best = left[0]
        for j in left[1:]:
            if (stopped[j] and not stopped[best]) or (stopped[j] == stopped[best] and scores[j] > scores[best]):
                best = j
        out.append(best)
        left.remove(best)
    return out


def crafted_rows(V: int) -> dict:
    """name -> bias [V] on the 1/8 grid (exact inputs for the reference): all logits equal (lp = -log V), one stop bias of -1e4 (what the
    benchmark's model carries: no NaN, no inf), a peaked row."""
    equal = np.full(V, 0.5, np.float32)
    stop = sc._row(V, 77 + V, stop=-1e4)
    peaked = sc._row(V, 78 + V)
    peaked[min(V - 3, 4096 + 5)] = 20.0
    return {"equal": equal, "stop_-1e4": stop, "peaked": peaked}


# ---- the parked row ---------------------------------------------------------------------------------------------------------
def pad16(n: int) -> int:
    return (n + 15) & ~15


def park_bytes(kv_format: int, layers: int, heads: int, V: int, pos: int, step: int, scores: bool = False) -> dict:
    """Offsets and size of a parked row from the header's fields (include/idxtts.h "Preempt and resume"); scores: reserved[1]."""
    C = 16 if kv_format == 0 else 8
    g = 8 if kv_format == 2 else 16
    e = (4, 2, 1)[kv_format]
    per_head = C * pad16(pos * g) + pos * 64 * e + (2 * pad16(4 * pos) if kv_format == 2 else 0)
    off_seen = 128
    off_codes = off_seen + pad16(V)
    off_lp = off_codes + pad16(8 * step)
    off_kv = off_lp + (pad16(4 * step) if scores else 0)
    return {"seen": off_seen, "codes": off_codes, "logprobs": off_lp, "kv": off_kv, "bytes": off_kv + layers * heads * per_head}


def parent_park_bytes(kv_format: int, layers: int, heads: int, V: int, pos: int, step: int) -> int:
    """The size formula as the header printed it before rows could carry scores."""
    C = 16 if kv_format == 0 else 8
    g = 8 if kv_format == 2 else 16
    e = (4, 2, 1)[kv_format]
    return 128 + pad16(V) + pad16(8 * step) + layers * heads * (C * pad16(pos * g) + pos * 64 * e + (2 * pad16(4 * pos) if kv_format == 2 else 0))


LOG_V = {V: -math.log(V) for V in VOCABS}
