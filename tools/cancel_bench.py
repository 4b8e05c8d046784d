"""What cancelling requests gives back: a ContinuousPipeline of 16 slots on the full-size model with synthetic weights (bf16 GPT
weights and KV), a fixed set of one-utterance requests at one cap with the stop token biased away, and `fut.cancel()` on every second
request once the first poll after its admission has run.  Wall time runs from the first submit until the surviving requests are done.

Only `submit` and `fut.cancel()` are used, and the counting is done by a wrapper around the pipeline's decode session, so the same file
runs on a commit whose pipeline does not look at cancelled Futures: there the cancelled rows decode to their cap and go through the
acoustic stage, and `rows_evicted` is 0.  `acoustic_coalesce` is 1, so that commit's merged-batch failure does not enter.

    python tools/cancel_bench.py [--requests 32] [--cap 384] [--poll-steps 16] [--reps 3]

Prints one JSON line: per repetition the wall time, the session steps run, the slot-steps (live rows summed over the steps), the rows
evicted and the host time of the evict calls; `evict_call_us`: the median host time of one evict call -- a launch plus bookkeeping, no
synchronisation."""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "index-tts_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Counted:
    """The lane's decode session with its calls counted; after every poll it tells the bench which requests have had their first
    poll (requests are one utterance each and admitted in submission order, so the k-th admitted row is the k-th request that was
    not cancelled before its admission -- and the bench only cancels after admission)."""

    def __init__(self, sess, stats, first_poll_done):
        self._sess, self._stats, self._tell = sess, stats, first_poll_done
        self._fresh = 0

    def __getattr__(self, name):
        return getattr(self._sess, name)

    def admit(self, rows, caps, **kw):
        ids = self._sess.admit(rows, caps, **kw)
        self._fresh += len(ids)
        return ids

    def step(self, n=1):
        live = len(self._sess.live_slots)
        out = self._sess.step(n)
        self._stats["steps"] += n if live else 0
        self._stats["slot_steps"] += n * live      # an upper bound: rows that end inside the poll are counted to its end
        fresh, self._fresh = self._fresh, 0
        if fresh:
            self._tell(fresh)
        return out

    def evict(self, ids):
        t0 = time.perf_counter()
        self._sess.evict(ids)
        self._stats["evict_s"].append(time.perf_counter() - t0)
        self._stats["rows_evicted"] += len(ids)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--cap", type=int, default=384)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--poll-steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from indextts_amd import synth, weights
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import ContinuousPipeline
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    dev = torch.device("cuda:0")
    cfg = PipelineConfig()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=dev, gpt_weight_format="bf16", gpt_kv_format="bf16")
    cond = PromptConditioning.synthetic(cfg, prompt_frames=689, tag="bench/prompt").to(dev)
    N, L = args.requests, 128
    text = torch.from_numpy(synth.integers("cbench/text", (N, L), 2, cfg.gpt.number_text_tokens))
    noise = torch.from_numpy(synth.uniform("cancelbench/noise", (1, cfg.s2mel.in_channels, 689 + int(args.cap * cfg.code_to_frame)), 1.7)).to(dev)

    def run(cancel: bool):
        stats = {"steps": 0, "slot_steps": 0, "rows_evicted": 0, "evict_s": []}
        futs, lock = [], threading.Lock()
        polled = [0]                                # requests whose first poll has run

        def first_poll_done(n):
            with lock:
                lo, polled[0] = polled[0], polled[0] + n
                mine = futs[lo:lo + n]
            if cancel:
                for k, f in enumerate(mine, start=lo):
                    if k % 2:
                        f.cancel()

        def factory(mp, mn):
            return Counted(tts.gpt.decode_session(args.slots, mp, mn, repetition_penalty=10.0), stats, first_poll_done)

        with ContinuousPipeline(tts, slots=args.slots, decode_lanes=1, poll_steps=args.poll_steps, max_new=args.cap, acoustic_coalesce=1,
                                session_factory=factory) as pipe:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with lock:                              # the lane's first poll finds the whole list
                for i in range(N):
                    futs.append(pipe.submit(text[i:i + 1], cond, max_mel_tokens=args.cap, noise=noise))
            for k, f in enumerate(futs):
                if not (cancel and k % 2):
                    f.result()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        ev = stats.pop("evict_s")
        return dict(stats, wall_s=wall, cancelled=sum(f.cancelled() for f in futs), evict_calls=len(ev)), ev

    run(False)                                      # warm-up: prefill width, step graph, acoustic length
    out = {"requests": N, "slots": args.slots, "cap": args.cap, "poll_steps": args.poll_steps, "reps": args.reps, "all": [], "cancel_half": []}
    evict_s = []
    for _ in range(args.reps):
        r, _ = run(False)
        out["all"].append(r)
        r, ev = run(True)
        out["cancel_half"].append(r)
        evict_s += ev
    for k in ("all", "cancel_half"):
        out[f"{k}_wall_s_median"] = float(np.median([r["wall_s"] for r in out[k]]))
    out["evict_call_us"] = float(np.median(evict_s) * 1e6) if evict_s else None
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
