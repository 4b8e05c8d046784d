#!/usr/bin/env python3
"""Time the CFM solver's per-row-schedule entry (idxtts_s2mel_cfm_sched) against the one-schedule entry (idxtts_s2mel_cfm_rows) at
configs[2]'s acoustic shapes: 16 rows, prompt 689 + 880 generated frames, full-size s2mel on synthetic weights, alone on the device.

  (a) 20 steps, rate 0.7 for all rows: one-schedule entry vs per-row entry (the same work; the per-row entry evaluates the two CFG
      halves as two launches chains of 16 sequences instead of one of 32, and gathers each row's step constants per iteration)
  (b) 8 rows x 20 steps + 8 rows x 8 steps in one call, vs the two calls made separately (one-schedule entry), vs 16 x 20
  (c) all rows at rate 0 (one estimator evaluation per step) vs rate 0.7

Every variant runs once per round, the rounds alternate in one process (after one warm-up round); reported: median [min .. max] ms over
the rounds.  usage: cfm_sched_bench.py [rounds=7]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "index-tts_amd"))
import torch  # noqa: E402
from indextts_amd import _lib, weights  # noqa: E402
from indextts_amd.config import PipelineConfig  # noqa: E402
from indextts_amd.s2mel import S2Mel  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
cfg = PipelineConfig()
dev = torch.device("cuda:0")
_lib.load()
m = S2Mel(weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel"), cfg.s2mel, device=dev)
B, Tp, Tg = 16, 689, 880
g = torch.Generator().manual_seed(0)
pc = torch.randn(1, Tp, 512, generator=g).to(dev)
rm = torch.randn(1, 80, Tp, generator=g).to(dev)
gen = torch.randn(B, Tg, 512, generator=g).to(dev)
style = torch.randn(1, 192, generator=g).to(dev).expand(B, -1).contiguous()
z = torch.randn(B, 80, Tp + Tg, generator=g).to(dev)


def solve(rows, steps, rate):
    n = len(rows)
    return m.cfm_rows(gen[rows], [Tg] * n, [pc] * n, [rm] * n, style[rows], steps, inference_cfg_rate=rate, z=z[rows])


ALL, LO, HI = list(range(B)), list(range(8)), list(range(8, B))
variants = {
    "a/c  one-schedule entry, 16 x 20 steps, rate 0.7": lambda: solve(ALL, 20, 0.7),
    "a    per-row entry,      16 x 20 steps, rate 0.7": lambda: solve(ALL, [20] * B, [0.7] * B),
    "b    per-row entry,      8 x 20 + 8 x 8 steps, rate 0.7, one call": lambda: solve(ALL, [20] * 8 + [8] * 8, [0.7] * B),
    "b    one-schedule entry, 8 x 20 then 8 x 8 steps, rate 0.7, two calls": lambda: (solve(LO, 20, 0.7), solve(HI, 8, 0.7)),
    "c    per-row entry,      16 x 20 steps, rate 0": lambda: solve(ALL, 20, 0.0),
}
times = {k: [] for k in variants}
for r in range(rounds + 1):
    for name, fn in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:          # round 0 warms up (workspaces, scratch, clocks)
            times[name].append((time.perf_counter() - t0) * 1e3)
print(f"gemm mode {_lib.get_gemm_mode()} (1 = split-bf16), acoustic_bf16 {int(_lib.get_acoustic_bf16())}, {rounds} alternating rounds")
for name, t in times.items():
    print(f"{name}: {statistics.median(t):8.1f} ms  [{min(t):.1f} .. {max(t):.1f}]", flush=True)
