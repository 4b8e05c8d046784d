#!/usr/bin/env python3
"""What the batch-invariant mode (`UnifiedVoice.set_batch_invariant`, idxtts_gpt_set_batch_invariant) costs, decode only, on the
full-size synthetic GPT, mode off against mode on in the same process:
    configs[2]'s decode: 16 rows, bf16 weights, 512 codes
    a merged decode:     48 rows, bf16 weights, 512 codes  (mode off: the plane GEMV; mode on: the fp32-MFMA GEMV)
    configs[4]'s decode:  1 row,  fp8 weights, 1500 codes  (mode off: 12 key pieces and the 4-row GEMV form; mode on: ceil(n / 512)
                                                            pieces and the 16-row form)
each with a bf16 and an fp8 KV cache.  Per shape, cache and mode: the tokens per second of the graph-replayed chain (host clock around
generations that end in a device synchronise, the two modes interleaved, the first round discarded as warm-up, median and spread of
the rest) and, from a pass of its own under the library's per-launch profiler, the decode attention's and the decode GEMVs' time per
step -- which launch carries a loss.

    python tools/batch_invariant_bench.py [--reps 3] [--shapes 0,1,2] [--json out.json]
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from indextts_amd import _lib, synth, weights  # noqa: E402
from indextts_amd.config import GPTConfig  # noqa: E402
from indextts_amd.gpt import UnifiedVoice  # noqa: E402

SHAPES = [("configs[2]", 16, "bf16", 512), ("48 rows", 48, "bf16", 512), ("configs[4]", 1, "fp8", 1500)]
ATTN = ("decode_attn_kernel", "decode_attn16_kernel", "decode_attn8_kernel")
GEMV = ("gemv_fx_kernel", "gemv_pl_kernel")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed generations per mode behind the warm-up round")
    ap.add_argument("--shapes", default="0,1,2", help="indices into the shape table")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    _lib.load()
    torch.set_num_threads(16)
    cfg = GPTConfig()
    w = weights.synth_gpt_weights(cfg, tag="bench/gpt")
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = -1e4          # fixed-length utterances
    # the build's DECODE_ATTN_PIECE_KEYS, read off the plan query: 4096 keys are 4096 / piece length pieces
    result = {"reps": args.reps, "piece_keys": 4096 // _lib.batch_invariant_plan(1280, 1280, 1, 0, n_keys=4096, smax=4096)["attn_pieces"],
              "shapes": {}}
    models = {}
    for idx in (int(i) for i in args.shapes.split(",")):
        name, rows, wfmt, codes = SHAPES[idx]
        if wfmt not in models:
            models.clear()
            torch.cuda.empty_cache()
            models[wfmt] = UnifiedVoice(w, cfg, device=dev, weight_format=wfmt, kv_format="bf16")
        uv = models[wfmt]
        lat = torch.from_numpy(synth.uniform("binvbench/lat", (rows, cfg.cond_latents, cfg.model_dim), 0.5))
        emo = torch.from_numpy(synth.uniform("binvbench/emo", (rows, cfg.model_dim), 0.3))
        text = torch.from_numpy(synth.integers("binvbench/text", (rows, 128), 2, cfg.number_text_tokens))

        def generate():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=codes, repetition_penalty=10.0)
            torch.cuda.synchronize()
            assert out.shape[1] == codes
            return time.perf_counter() - t0

        shape = {"rows": rows, "weights": wfmt, "codes": codes, "cache": {}}
        for kv in ("bf16", "fp8"):
            uv.set_kv_format(kv)
            times = {0: [], 1: []}
            for rnd in range(args.reps + 1):               # interleaved; round 0 warms up (and captures each mode's decode graph)
                for on in (0, 1):
                    uv.set_batch_invariant(bool(on))
                    t = generate()
                    if rnd:
                        times[on].append(t)
            entry = {}
            for on in (0, 1):
                uv.set_batch_invariant(bool(on))
                _lib.profile_enable(True)
                generate()
                prof = _lib.profile_read()
                _lib.profile_enable(False)
                ts = times[on]
                entry["on" if on else "off"] = {
                    "tokens_per_s": rows * codes / statistics.median(ts), "tokens_per_s_min": rows * codes / max(ts),
                    "tokens_per_s_max": rows * codes / min(ts),
                    "attn_ms_per_step": sum(prof[k]["ms"] for k in ATTN if k in prof) / codes,
                    "gemv_ms_per_step": sum(prof[k]["ms"] for k in GEMV if k in prof) / codes,
                }
            uv.set_batch_invariant(False)
            shape["cache"][kv] = entry
        result["shapes"][name] = shape

    print(f"batch-invariant mode off / on, decode only, full-size synthetic GPT; {args.reps} timed generations per mode; "
          f"attention pieces of at most {result['piece_keys']} keys")
    print(f"{'shape':12s}{'KV':>6s}{'off tok/s':>12s}{'on tok/s':>12s}{'on / off':>10s}{'attn ms/step off':>18s}{'on':>9s}{'gemv ms/step off':>18s}{'on':>9s}")
    for name, shape in result["shapes"].items():
        for kv, e in shape["cache"].items():
            a, b = e["off"], e["on"]
            print(f"{name:12s}{kv:>6s}{a['tokens_per_s']:12.1f}{b['tokens_per_s']:12.1f}{b['tokens_per_s'] / a['tokens_per_s']:10.3f}"
                  f"{a['attn_ms_per_step']:18.4f}{b['attn_ms_per_step']:9.4f}{a['gemv_ms_per_step']:18.4f}{b['gemv_ms_per_step']:9.4f}")
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
