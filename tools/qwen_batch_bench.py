"""Times batched against sequential emotion classification at full size (Qwen3-0.6B shape, synthetic weights, bf16 storage): for
B in {1, 2, 4, 8, 16} texts, B calls of QwenLM.generate in series against one QwenLM.generate_batch.  Every row has a 150-token
prompt and 64 FORCED steps (teacher forcing on ids that are no end id), so no row stops early and both sides run the same steps.
Both sides replay their kept step graph; each is warmed (capture included) before it is timed; the figure is the median of the
repetitions, and their min..max spread is printed beside it.  Prints one JSON line per B:

    sequential ms, batched ms, ratio, the time of one replayed batched step of one tile, launches per step.

The step time is a difference: (the N-step call - a 3-step call of the same batch) / (N - 3) / tiles.  Both calls hold every
tile's upload, prefill, the eager first step and the hand-back; the longer one holds N - 3 more replays of the kept step per tile.
A call of one row runs the single-prompt path and captures no batched step: its launches per step print as null.

The whole sweep runs in one child process under a time limit (a fault or hang ends the run there).  Not part of bench.py.
    python tools/qwen_batch_bench.py [--batches 1,2,4,8,16] [--prompt 150] [--new 64] [--reps 7]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(batches, P, N, reps):
    import torch
    from indextts_amd import synth
    from indextts_amd.qwen_emo import QwenConfig, QwenLM, synth_qwen_weights
    cfg = QwenConfig()
    lm = QwenLM(synth_qwen_weights(cfg, tag="bench/qwen"), cfg, device="cuda:0", weight_format="bf16")
    tile = lm.max_batch()
    for B in batches:
        prompts = [synth.integers(f"bench/qwen/batch/prompt{b}", (P,), 0, cfg.vocab_size) for b in range(B)]
        forced = [synth.integers(f"bench/qwen/batch/forced{b}", (N,), 0, cfg.vocab_size) for b in range(B)]

        def seq(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = [lm.generate(prompts[b], n, forced_ids=forced[b][:n], use_graph=True)[0] for b in range(B)]
            return (time.perf_counter() - t0) * 1e3, out

        def bat(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = lm.generate_batch(prompts, n, forced_ids=[f[:n] for f in forced], use_graph=True)[0]
            return (time.perf_counter() - t0) * 1e3, out

        res = {}
        for name, fn in (("sequential", seq), ("batched", bat)):
            fn(N), fn(N)      # capture, then one replayed call
            t = sorted(fn(N)[0] for _ in range(reps))
            res[name] = (t[len(t) // 2], t[0], t[-1])
        assert seq(N)[1] == bat(N)[1] and all(len(r) == N for r in bat(N)[1])      # same ids, nobody stopped early
        launches = lm.batch_step_graph_launches()
        bat(3)
        short = sorted(bat(3)[0] for _ in range(reps))[reps // 2]      # the same call with 3 steps: N - 3 fewer replays per tile, all else equal
        (s, s0, s1), (b, b0, b1) = res["sequential"], res["batched"]
        tiles = -(-B // tile)
        print(json.dumps({"tool": "qwen_batch_bench", "B": B, "prompt_tokens": P, "new_tokens": N, "sequential_ms": round(s, 2),
                          "sequential_spread_ms": [round(s0, 2), round(s1, 2)], "batched_ms": round(b, 2),
                          "batched_spread_ms": [round(b0, 2), round(b1, 2)], "ratio": round(s / b, 2),
                          "batched_us_per_step": round((b - short) / (N - 3) / tiles * 1e3, 1), "tiles": tiles,
                          "launches_per_step": launches if launches > 0 else None, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--prompt", type=int, default=150)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        child([int(b) for b in a.batches.split(",")], a.prompt, a.new, a.reps)
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--batches", a.batches,
                        "--prompt", str(a.prompt), "--new", str(a.new), "--reps", str(a.reps)])
    if r.returncode != 0:
        print(f"qwen_batch_bench: ended with status {r.returncode}", file=sys.stderr)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
