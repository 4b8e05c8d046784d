"""Times one emotion-from-text classification at full size (Qwen3-0.6B, synthetic weights): a 40-token prompt, 64 new tokens,
graph replay, fp32 and bf16 weight storage.  Prints one JSON line per format:

    ms per call, µs per token (decode steps only and whole call), launches per token (counted from the captured graph), and the
    floor of DESIGN.md §5 -- (weight + KV bytes per token) / 6.3 TB/s + 1.5 µs per launch -- with the ratio to it.

Each format runs in a child process of its own under a time limit (a fault or hang in one ends the run there).
    python tools/qwen_emo_bench.py [--formats bf16,f32] [--prompt 40] [--new 64] [--reps 5]
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

HBM_BPS, LAUNCH_US = 6.3e12, 1.5


def floor_us(cfg, fmt, keys, launches):
    """Weight + KV bytes of one decode step at `keys` cached positions, over the achievable bandwidth, plus the launch boundaries."""
    wb = 2 if fmt == "bf16" else 4
    H, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    qd, kd = cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim
    weights = L * ((qd + 2 * kd) * H + H * qd + 3 * I * H) + cfg.vocab_size * H
    kv = L * 2 * kd * keys * 4
    return (weights * wb + kv) / HBM_BPS * 1e6 + LAUNCH_US * launches, weights * wb, kv


def child(fmt, P, N, reps):
    import numpy as np
    import torch
    from indextts_amd import synth
    from indextts_amd.qwen_emo import QwenConfig, QwenLM, synth_qwen_weights
    cfg = QwenConfig()
    lm = QwenLM(synth_qwen_weights(cfg, tag="bench/qwen"), cfg, device="cuda:0", weight_format=fmt)
    prompt = synth.integers("bench/qwen/prompt", (P,), 0, cfg.vocab_size)

    def timed(new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, _ = lm.generate(prompt, new, use_graph=True)      # returns after the stream has finished
        return (time.perf_counter() - t0) * 1e3, ids

    timed(N), timed(2)      # capture + warm both shapes
    full = sorted(timed(N)[0] for _ in range(reps))
    short = sorted(timed(2)[0] for _ in range(reps))      # prefill + 2 steps: what is not the replayed decode
    timed(N)      # leaves the N-token graph as the kept one
    launches = lm.step_graph_launches()
    ms, ms2 = full[len(full) // 2], short[len(short) // 2]
    step_us = (ms - ms2) / (N - 2) * 1e3
    fl, wbytes, kvbytes = floor_us(cfg, fmt, P + N // 2, launches)
    print(json.dumps({"tool": "qwen_emo_bench", "weight_format": fmt, "prompt_tokens": P, "new_tokens": N, "ms_per_call": round(ms, 3),
                      "ms_prefill_plus_2_steps": round(ms2, 3), "us_per_token_decode": round(step_us, 2),
                      "us_per_token_call": round(ms / N * 1e3, 2), "launches_per_token": launches,
                      "launch_bound": 5 * cfg.num_hidden_layers + 3, "weight_bytes_per_token": wbytes, "kv_bytes_per_token": kvbytes,
                      "floor_us_per_token": round(fl, 2), "ratio_to_floor": round(step_us / fl, 3), "reps": reps}), flush=True)
    assert 0 < launches <= 5 * cfg.num_hidden_layers + 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bf16,f32")
    ap.add_argument("--prompt", type=int, default=40)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.prompt, a.new, a.reps)
        return 0
    for fmt in a.formats.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", fmt,
                            "--prompt", str(a.prompt), "--new", str(a.new), "--reps", str(a.reps)])
        if r.returncode != 0:      # nothing more on the GPU after a failure
            print(f"qwen_emo_bench: format {fmt} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
