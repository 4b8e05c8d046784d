"""What scoring given codes costs, on the full-size GPT with synthetic weights (bf16 weights, bf16 KV cache, stop token biased away)
at configs[2]'s decode shape: 128-token texts (164 prompt rows), sequences of 512 codes.

(a) 1 and 16 sequences of 512 codes: UnifiedVoice.score_codes (one prefill, the head in chunks of 64 positions) against
    generate(forced_codes=, return_logprobs=True) over the same codes (512 decode steps, no step graph) -- the step path of the same
    build.
(b) The head's share of score_codes: the number of 64-position chunks and, from idxtts_profile_*, the time per chunk of the head
    GEMV(s), the row norm and score_rows_kernel (one profiled call; the profiler serialises launches).
(c) An admission of 16 rows behind 256 codes into a 16-slot session, prefix_logprobs given by the caller against "model".
Every time is the host clock around the Python call and a synchronise of the stream, after a warm-up call; the median of `--reps`
repeats and their spread (min .. max) are reported.

    python tools/score_bench.py [--reps 5]

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

TEXT, N, BATCHES, SLOTS, K_ADMIT = 128, 512, (1, 16), 16, 256


def profile(fn):
    """{kernel family: (total ms, launches)} of one call of fn under the library's profiler (it reads an event pair per launch)."""
    from indextts_amd import _lib
    _lib.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    out = {k: (v["ms"], int(v["launches"])) for k, v in _lib.profile_read().items()}
    _lib.profile_enable(False)
    return out


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
    P, d = row.shape
    codes = torch.from_numpy(synth.integers("xbench/score_codes", (max(BATCHES), N), 0, cfg.start_mel_token))

    def timed(fn, sync):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t0, r

    def stats(fn):
        ts, r = [], None
        for _ in range(args.reps + 1):      # the first: warm-up
            t, r = timed(fn, torch.cuda.synchronize)
            ts.append(t * 1e3)
        ts = ts[1:]
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}, r

    out = {"text_tokens": TEXT, "prompt_rows": int(P), "codes": N, "reps": args.reps, "weights": "bf16", "kv": "bf16", "by_batch": []}
    for B in BATCHES:
        emb = row[None].expand(B, P, d).contiguous()
        c = codes[:B].contiguous()
        fake = torch.ones(B, P + 1, dtype=torch.long)
        fake[:, -1] = cfg.start_mel_token
        s_score, lp = stats(lambda: uv.score_codes(c, emb))
        # the forced call scores the row's own argmax, not the forced token: its logits give the step path's value for the given codes
        s_steps, _ = stats(lambda: uv.generate(fake, max_new_tokens=N, tts_embeddings=emb, repetition_penalty=10.0, forced_codes=c,
                                               return_logprobs=True, use_graph=False))
        prof = profile(lambda: uv.score_codes(c, emb))
        chunks = -(-B * N // 64)
        head = {k: v for k, v in prof.items() if k.startswith(("gemv", "score_rows", "rows_norm"))}
        total = sum(ms for ms, _ in prof.values())
        out["by_batch"].append({"B": B, "score_codes": s_score, "forced_steps": s_steps,
                                "speedup_median": s_steps["median_ms"] / s_score["median_ms"], "chunks": chunks,
                                "profiled_kernel_ms": total,
                                "head_us_per_chunk": {k: 1e3 * ms / chunks for k, (ms, _) in head.items()},
                                "head_share_of_kernel_time": sum(ms for ms, _ in head.values()) / total if total else None,
                                "launches": {k: n for k, (_, n) in head.items()}})
        del lp
    # (c) an admission of 16 rows behind 256 codes, the prefix values given and computed
    sess = uv.decode_session(SLOTS, max_prompt=int(P), max_new=N, sampled=False, scores=True, prefix=True, prefix_scores=True)
    pre = [codes[i, :K_ADMIT] for i in range(SLOTS)]
    given = [np.zeros(K_ADMIT, np.float32)] * SLOTS
    sync = sess.stream.synchronize

    def admit(lps):
        ts = []
        for _ in range(args.reps + 1):      # the first: warm-up; the eviction that follows is not timed
            t, ids = timed(lambda: sess.admit([row] * SLOTS, N, prefix=pre, prefix_logprobs=lps), sync)
            sess.evict(ids)
            ts.append(t * 1e3)
        ts = ts[1:]
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}
    out["admit_16_rows_behind_256_codes"] = {"given": admit(given), "model": admit(["model"] * SLOTS)}
    sess.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
