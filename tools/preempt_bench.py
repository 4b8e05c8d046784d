"""What preemption costs and what it buys, on the full-size model with synthetic weights (bf16 GPT weights, stop token biased away).

(a) Park and resume times.  A 16-slot decode session, 128-token texts (configs[2]'s prompt: 164 rows); one row is decoded to one code
    short of 512 codes (configs[2]'s row length) and one to one short of 1500 (configs[4]'s), with the bf16 and with the fp8 KV cache.
    Each row is then parked and resumed `--cycles` times through the C entry points; every call is timed with the host clock around the
    call and a synchronise of the session's stream, so a time holds the call's small device-to-host read of the slot state, the launch
    and the kernel.  A plain device-to-device copy of the parked row's byte count is timed the same way in the same loop.  The kernels'
    own times come from a profiler run of this file (`--only park`), see profiles/README.md.
(b) Time to an urgent request's codes.  A ContinuousPipeline whose 16 slots are taken by 16 one-utterance requests of `--low-cap` codes
    and priority 0; once their first poll has run, one request of `--urgent-cap` codes and priority 5 is submitted.  The time runs from
    that submit until the lane takes the urgent row's codes from its session, with preempt=False and preempt=True alternating on the
    same build; the wall time until every request has its audio is reported too.

(c) --beam: the same two measurements for beam groups (the reference's default request: beam-sample, 3 beams).  Park and resume of one
    group of a 5 groups x 3 beams session at configs[2]'s prompt and one code short of 512, bf16 and fp8 KV, against the plain copy of
    the same byte count, with the group's bytes beside 3 x a parked row's at the same position; and the time to an urgent beam
    request's codes and audio on a beam pipeline whose 5 groups are taken, with preempt_groups off and on.

    python tools/preempt_bench.py [--beam] [--only park|urgent] [--cycles 20] [--reps 3] [--low-cap 512] [--urgent-cap 64] [--poll-steps 16]

Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
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

SLOTS, TEXT = 16, 128


def park_times(uv, kv: str, lengths, cycles: int) -> list:
    from indextts_amd import _lib, synth
    lib, cfg = _lib.load(), uv.cfg
    uv.set_kv_format(kv)
    conds = torch.from_numpy(synth.uniform("pbench/conds", (1, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    row = uv.prompt_rows(conds, torch.from_numpy(synth.integers("pbench/text", (1, TEXT), 2, cfg.number_text_tokens)))[0]
    lengths = sorted(lengths)
    sess = uv.decode_session(SLOTS, max_prompt=int(row.shape[0]), max_new=lengths[-1])
    ws, sp, out, done = _lib.ptr(sess._ws), sess._sp(), [], 0
    assert sess.admit([row] * len(lengths), lengths) == list(range(len(lengths)))

    def timed(fn):
        sess.stream.synchronize()
        t0 = time.perf_counter()
        fn()
        sess.stream.synchronize()
        return time.perf_counter() - t0
    for slot, n in enumerate(lengths):
        for s in sess.step(n - 2 - done):                            # n - 1 codes: one step short of the cap, still decoding
            sess.take(s)                                             # (a shorter row measured before has ended meanwhile)
        done = n - 2
        assert slot in sess.live_slots
        need = int(lib.idxtts_gpt_session_park_bytes(uv._h, slot, ws, sp))
        assert need > 0
        with torch.cuda.stream(sess.stream):
            blob, other = torch.empty(need, dtype=torch.uint8, device=uv.device), torch.empty(need, dtype=torch.uint8, device=uv.device)
        t = {"park": [], "resume": [], "copy": []}
        for c in range(cycles + 3):                                  # the first three: warm-up
            wr = ctypes.c_size_t(0)
            a = timed(lambda: _lib.check(lib.idxtts_gpt_session_park(uv._h, slot, _lib.ptr(blob), need, ctypes.byref(wr), ws, sp)))
            with torch.cuda.stream(sess.stream):
                k = timed(lambda: other.copy_(blob))
            b = timed(lambda: _lib.check(lib.idxtts_gpt_session_resume(uv._h, slot, _lib.ptr(blob), need, ws, sp)))
            if c >= 3:
                t["park"].append(a); t["copy"].append(k); t["resume"].append(b)
        held = []                                                    # the Python path once more, as the pipeline calls it
        py_park = timed(lambda: held.append(sess.park(slot)))
        py_resume = timed(lambda: sess.resume(held.pop(), slot))
        pos = n - 1 + int(row.shape[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        out.append({"kv": kv, "codes": n - 1, "pos": pos, "bytes": need, "park_us": med["park"] * 1e6, "resume_us": med["resume"] * 1e6,
                    "copy_us": med["copy"] * 1e6, "park_min_us": min(t["park"]) * 1e6, "resume_min_us": min(t["resume"]) * 1e6,
                    "copy_min_us": min(t["copy"]) * 1e6, "python_park_us": py_park * 1e6, "python_resume_us": py_resume * 1e6,
                    "park_gbps_moved": 2 * need / med["park"] / 1e9, "copy_gbps_moved": 2 * need / med["copy"] / 1e9})
    sess.close()
    return out


BEAMS, GROUPS = 3, 5
BEAM = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}      # IndexTTS2.infer's defaults


def _pad16(n: int) -> int:
    return (n + 15) & ~15


def row_bytes(cfg, kv: str, pos: int, step: int) -> int:
    """A parked row's size (include/idxtts.h "Preempt and resume")."""
    C, g, e = {"bf16": (8, 16, 2), "fp8": (8, 8, 1)}[kv]
    per_head = C * _pad16(pos * g) + pos * 64 * e + (2 * _pad16(4 * pos) if kv == "fp8" else 0)
    return 128 + _pad16(cfg.number_mel_codes) + _pad16(8 * step) + cfg.layers * cfg.heads * per_head


def group_park_times(uv, kv: str, codes: int, cycles: int) -> dict:
    """park_times for one group of a GROUPS x BEAMS beam session, through idxtts_gpt_session_park_group / _resume_group."""
    from indextts_amd import _lib, synth
    lib, cfg = _lib.load(), uv.cfg
    uv.set_kv_format(kv)
    conds = torch.from_numpy(synth.uniform("pbench/conds", (1, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    row = uv.prompt_rows(conds, torch.from_numpy(synth.integers("pbench/text", (1, TEXT), 2, cfg.number_text_tokens)))[0]
    sess = uv.beam_session(GROUPS * BEAMS, BEAMS, max_prompt=int(row.shape[0]), max_new=codes)
    ws, sp = _lib.ptr(sess._ws), sess._sp()
    assert sess.admit([row], [codes], beam=dict(BEAM, seed=7)) == [0]
    assert sess.step(codes - 2) == [] and sess.live_groups == [0]   # codes - 1 tokens per beam: one step short of the cap

    def timed(fn):
        sess.stream.synchronize()
        t0 = time.perf_counter()
        fn()
        sess.stream.synchronize()
        return time.perf_counter() - t0
    need = int(lib.idxtts_gpt_session_park_group_bytes(uv._h, 0, ws, sp))
    assert need > 0
    with torch.cuda.stream(sess.stream):
        blob, other = torch.empty(need, dtype=torch.uint8, device=uv.device), torch.empty(need, dtype=torch.uint8, device=uv.device)
    t = {"park": [], "resume": [], "copy": []}
    for c in range(cycles + 3):                                      # the first three: warm-up
        wr = ctypes.c_size_t(0)
        a = timed(lambda: _lib.check(lib.idxtts_gpt_session_park_group(uv._h, 0, _lib.ptr(blob), need, ctypes.byref(wr), ws, sp)))
        with torch.cuda.stream(sess.stream):
            k = timed(lambda: other.copy_(blob))
        b = timed(lambda: _lib.check(lib.idxtts_gpt_session_resume_group(uv._h, 0, _lib.ptr(blob), need, ws, sp)))
        if c >= 3:
            t["park"].append(a); t["copy"].append(k); t["resume"].append(b)
    held = []
    py_park = timed(lambda: held.append(sess.park_group(0)))
    py_resume = timed(lambda: sess.resume_group(held.pop(), 0))
    sess.close()
    pos, step = codes - 1 + int(row.shape[0]), codes - 1
    med = {k: float(np.median(v)) for k, v in t.items()}
    rows = BEAMS * row_bytes(cfg, kv, pos, step)
    return {"kv": kv, "beams": BEAMS, "codes": step, "pos": pos, "bytes": need, "bytes_of_rows": rows, "bytes_ratio": need / rows,
            "park_us": med["park"] * 1e6, "resume_us": med["resume"] * 1e6, "copy_us": med["copy"] * 1e6,
            "park_min_us": min(t["park"]) * 1e6, "resume_min_us": min(t["resume"]) * 1e6, "copy_min_us": min(t["copy"]) * 1e6,
            "python_park_us": py_park * 1e6, "python_resume_us": py_resume * 1e6,
            "park_gbps_moved": 2 * need / med["park"] / 1e9, "copy_gbps_moved": 2 * need / med["copy"] / 1e9}


class Timed:
    """The lane's decode session: tells the bench when the first poll has run, and notes when each row's codes are taken."""

    def __init__(self, sess, first_poll, takes, parks):
        self._sess, self._first_poll, self._takes, self._parks = sess, first_poll, takes, parks

    def __getattr__(self, name):
        return getattr(self._sess, name)

    def step(self, n=1):
        out = self._sess.step(n)
        self._first_poll.set()
        return out

    def take(self, i):
        codes = self._sess.take(i)
        self._takes.append((time.perf_counter(), int(codes.shape[0])))
        return codes

    def park(self, slot):
        t0 = time.perf_counter()
        row = self._sess.park(slot)
        self._parks.append(time.perf_counter() - t0)
        return row

    def park_group(self, group):
        t0 = time.perf_counter()
        parked = self._sess.park_group(group)
        self._parks.append(time.perf_counter() - t0)
        return parked


def urgent_times(tts, cond, args) -> dict:
    from indextts_amd import synth
    from indextts_amd.serving import ContinuousPipeline
    cfg = tts.cfg
    beam = bool(getattr(args, "beam", False))
    places = GROUPS if beam else SLOTS                  # requests a full session holds
    text = torch.from_numpy(synth.integers("pbench/ptext", (SLOTS + 1, TEXT), 2, cfg.gpt.number_text_tokens))
    samp = (lambda i: dict(BEAM, num_beams=BEAMS, seed=100 + i)) if beam else (lambda i: None)

    def run(preempt: bool):
        first_poll, takes, parks = threading.Event(), [], []

        def factory(mp, mn):
            if beam:
                return Timed(tts.gpt.beam_session(GROUPS * BEAMS, BEAMS, mp, mn, repetition_penalty=10.0), first_poll, takes, parks)
            return Timed(tts.gpt.decode_session(SLOTS, mp, mn, repetition_penalty=10.0), first_poll, takes, parks)
        kind = dict(slots=GROUPS * BEAMS, num_beams=BEAMS, preempt_groups=preempt) if beam else dict(slots=SLOTS, preempt=preempt)
        with ContinuousPipeline(tts, decode_lanes=1, poll_steps=args.poll_steps, max_new=args.low_cap, session_factory=factory,
                                **kind) as pipe:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with pipe._cv:                          # the lane's first poll finds all of them
                low = [pipe.submit(text[i:i + 1], cond, max_mel_tokens=args.low_cap, noise_seed=1000 + i, sampling=samp(i))
                       for i in range(places)]
            assert first_poll.wait(600)
            t1 = time.perf_counter()
            urgent = pipe.submit(text[SLOTS:], cond, max_mel_tokens=args.urgent_cap, noise_seed=999, priority=5, sampling=samp(99))
            urgent.result()
            t_audio = time.perf_counter() - t1
            for f in low:
                f.result()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        (t_codes,) = [t - t1 for t, n in takes if n == args.urgent_cap]
        return {"urgent_codes_s": t_codes, "urgent_audio_s": t_audio, "wall_s": wall, "parks": len(parks),
                "park_call_ms": [round(p * 1e3, 3) for p in parks]}
    run(True)                                       # warm-up: prefill widths, step graph, acoustic lengths, the park kernels
    out = {"preempt_off": [], "preempt_on": []}
    for _ in range(args.reps):
        out["preempt_off"].append(run(False))
        out["preempt_on"].append(run(True))
    for k in ("preempt_off", "preempt_on"):
        for m in ("urgent_codes_s", "urgent_audio_s", "wall_s"):
            out[f"{k}_{m}_median"] = float(np.median([r[m] for r in out[k]]))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["park", "urgent"], default=None)
    ap.add_argument("--beam", action="store_true", help="measure beam groups (3 beams, 5 groups) instead of rows")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--low-cap", type=int, default=512)
    ap.add_argument("--urgent-cap", type=int, default=64)
    ap.add_argument("--poll-steps", type=int, default=16)
    args = ap.parse_args()
    assert args.urgent_cap < args.low_cap
    from indextts_amd import weights
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    dev = torch.device("cuda:0")
    cfg = PipelineConfig()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=dev, gpt_weight_format="bf16", gpt_kv_format="bf16")
    out = {"slots": GROUPS * BEAMS if args.beam else SLOTS, "beam": args.beam, "text_tokens": TEXT, "cycles": args.cycles, "reps": args.reps, "low_cap": args.low_cap,
           "urgent_cap": args.urgent_cap, "poll_steps": args.poll_steps}
    if args.only != "park":
        cond = PromptConditioning.synthetic(cfg, prompt_frames=689, tag="bench/prompt").to(dev)
        out["urgent"] = urgent_times(tts, cond, args)
    if args.only != "urgent" and args.beam:
        out["park"] = [group_park_times(tts.gpt, kv, 512, args.cycles) for kv in ("bf16", "fp8")]
        tts.gpt.set_kv_format("bf16")
    elif args.only != "urgent":
        out["park"] = park_times(tts.gpt, "bf16", [512, 1500], args.cycles) + park_times(tts.gpt, "fp8", [512, 1500], args.cycles)
        tts.gpt.set_kv_format("bf16")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
