"""What continuing from given codes costs, on the full-size GPT with synthetic weights (bf16 weights, bf16 KV cache, stop token biased
away) at configs[2]'s decode shape: a 16-slot decode session, 128-token texts (164 prompt rows), 512-code requests.

(a) k decode steps.  Sixteen rows are admitted and stepped to 64, 256 and 448 codes; the cumulative host time of those step() calls
    (graph replay, one synchronise per call) is what decoding a row's first k codes costs while the session is full -- the price of
    rebuilding a row from nothing.
(b) Admissions into that session, four slots freed, twelve rows still live at 448 codes.  For k = 64 / 256 / 448, each `--reps` times
    and followed by an eviction: a plain admission of one row (prefill over P + 1 positions + first token), an admission of the same row
    behind k codes (prefill over P + 1 + k positions, DecodeSession.admit(prefix=)), fork(at=k) from a live row that holds 448 codes, an
    admission behind k codes with takes=4 (one prefill, fanned out), and four separate admissions behind k codes.
Every time is the host clock around the Python call and a synchronise of the session's stream; medians are reported.

    python tools/prefix_bench.py [--reps 5]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "index-tts_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SLOTS, TEXT, CAP, KS = 16, 128, 512, (64, 256, 448)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from indextts_amd import synth, weights
    from indextts_amd.config import GPTConfig
    from indextts_amd.gpt import UnifiedVoice
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    cfg = GPTConfig()
    w = weights.synth_gpt_weights(cfg, tag="bench/gpt")
    w["mel_head.bias"][cfg.stop_mel_token] = -1e4
    uv = UnifiedVoice(w, cfg, device=torch.device("cuda:0"), weight_format="bf16", kv_format="bf16")
    conds = torch.from_numpy(synth.uniform("xbench/conds", (1, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    row = uv.prompt_rows(conds, torch.from_numpy(synth.integers("xbench/text", (1, TEXT), 2, cfg.number_text_tokens)))[0]
    codes = torch.from_numpy(synth.integers("xbench/codes", (KS[-1],), 0, cfg.start_mel_token))
    sess = uv.decode_session(SLOTS, max_prompt=int(row.shape[0]), max_new=CAP, prefix=True)

    def timed(fn):
        sess.stream.synchronize()
        t0 = time.perf_counter()
        r = fn()
        sess.stream.synchronize()
        return time.perf_counter() - t0, r

    out = {"slots": SLOTS, "text_tokens": TEXT, "prompt_rows": int(row.shape[0]), "cap": CAP, "reps": args.reps, "weights": "bf16", "kv": "bf16"}
    t_admit16, ids = timed(lambda: sess.admit([row] * SLOTS, CAP))
    assert ids == list(range(SLOTS))
    out["admit_16_rows_ms"] = t_admit16 * 1e3
    have, total, steps = 1, 0.0, {}
    for k in KS:      # (a): the first admission's call holds the one-off captures; the step graph is captured in the first step() call
        t, fin = timed(lambda: sess.step(k - have))
        assert fin == []
        total, have = total + t, k
        steps[k] = total * 1e3
    out["decode_steps_ms"] = {str(k): v for k, v in steps.items()}
    out["decode_steps_note"] = "cumulative step() time to k codes, 16 live rows; the first call includes the graph capture"
    t, _ = timed(lambda: sess.step(0))
    sess.evict([12, 13, 14, 15])
    med = lambda v: float(np.median(v)) * 1e3      # noqa: E731

    def run(fn, n_slots):
        ts = []
        for _ in range(args.reps + 1):      # the first: warm-up
            t, got = timed(fn)
            flat = [s for g in got for s in (g if isinstance(g, list) else [g])]
            assert len(flat) == n_slots
            sess.evict(flat)
            ts.append(t)
        return med(ts[1:])
    out["plain_admit_ms"] = run(lambda: sess.admit([row], CAP), 1)
    rows = []
    for k in KS:
        pre = codes[:k]
        rows.append({"k": k,
                     "prefix_admit_ms": run(lambda: sess.admit([row], CAP, prefix=[pre]), 1),
                     "fork_ms": run(lambda: sess.fork(0, at=k), 1),
                     "prefix_admit_takes4_ms": run(lambda: sess.admit([row], CAP, takes=4, prefix=[pre]), 4),
                     "four_prefix_admits_ms": run(lambda: [sess.admit([row], CAP, prefix=[pre])[0] for _ in range(4)], 4),
                     "decode_steps_ms": steps[k]})
    out["by_k"] = rows
    sess.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
