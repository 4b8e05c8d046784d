#!/usr/bin/env python3
"""What the fp8 KV cache (`kv_format="fp8"`, idxtts_gpt_set_kv_format(ctx, 2)) buys and costs against the bf16 cache, decode only, on the
full-size synthetic GPT at two shapes:
    configs[2]'s decode: 16 rows, bf16 weights, about 510 codes
    configs[4]'s decode:  1 row,  fp8 weights, 1500 codes (key-split decode attention)
For each shape and cache: the decode attention's time per step (the library's per-launch profiler, a pass of its own), the tokens per
second of the graph-replayed chain (host clock around generations that end in a device synchronise, the two caches interleaved, the
first round discarded as warm-up, median and spread of the rest), and oracle/parity.py's teacher-forced figures on 6 x 96 steps
against the CPU oracle that rounds keys and values the same way (for fp8: tests/kv_fp8_cases.py::fp8_stack patched in).

    python tools/kv_fp8_bench.py [--reps 3] [--no-parity] [--json out.json]
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from indextts_amd import _lib, synth, weights  # noqa: E402
from indextts_amd.config import GPTConfig  # noqa: E402
from indextts_amd.gpt import UnifiedVoice  # noqa: E402

SHAPES = [("configs[2]", 16, "bf16", 510), ("configs[4]", 1, "fp8", 1500)]
ATTN = {"bf16": "decode_attn16_kernel", "fp8": "decode_attn8_kernel"}


def parity_figures(uv, tw, cfg, kv):
    import kv_fp8_cases as kc
    import oracle.gpt as og
    from oracle import parity
    B, L = 6, 32
    lat = torch.from_numpy(synth.uniform("kv8bench/par/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("kv8bench/par/emo", (B, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("kv8bench/par/text", (B, L), 2, cfg.number_text_tokens))
    stack = og.gpt2_stack
    try:
        if kv == "fp8":
            og.gpt2_stack = kc.fp8_stack
        r = parity.decode_parity(uv, tw, cfg, lat, emo, text, 96)
    finally:
        og.gpt2_stack = stack
    return {k: r[k] for k in ("max_abs_logit_diff", "mean_abs_logit_diff", "logit_std", "codes_match_rate_teacher_forced",
                              "worst_oracle_margin_at_a_mismatch", "first_mismatch_step_teacher_forced", "first_difference_step_free_running")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed generations per cache behind the warm-up round")
    ap.add_argument("--no-parity", action="store_true")
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
    result = {"reps": args.reps, "shapes": {}}
    for name, rows, wfmt, codes in SHAPES:
        uv = UnifiedVoice(w, cfg, device=dev, weight_format=wfmt, keep_effective=True, kv_format="bf16")
        tw = {k: torch.from_numpy(v) for k, v in uv.effective_state_dict.items()}
        lat = torch.from_numpy(synth.uniform("kv8bench/lat", (rows, cfg.cond_latents, cfg.model_dim), 0.5))
        emo = torch.from_numpy(synth.uniform("kv8bench/emo", (rows, cfg.model_dim), 0.3))
        text = torch.from_numpy(synth.integers("kv8bench/text", (rows, 128), 2, cfg.number_text_tokens))

        def generate():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=codes, repetition_penalty=10.0)
            torch.cuda.synchronize()
            assert out.shape[1] == codes
            return time.perf_counter() - t0

        times = {"bf16": [], "fp8": []}
        for rnd in range(args.reps + 1):                   # interleaved; round 0 warms up (and captures each cache's decode graph)
            for kv in ("bf16", "fp8"):
                uv.set_kv_format(kv)
                t = generate()
                if rnd:
                    times[kv].append(t)
        shape = {"rows": rows, "weights": wfmt, "codes": codes, "cache": {}}
        for kv in ("bf16", "fp8"):
            uv.set_kv_format(kv)
            _lib.profile_enable(True)
            generate()
            prof = _lib.profile_read()
            _lib.profile_enable(False)
            attn = prof[ATTN[kv]]
            ts = times[kv]
            shape["cache"][kv] = {
                "attn_ms_per_step": attn["ms"] / codes, "attn_launches": attn["launches"],
                "attn_alg_gb_per_s": attn["bytes"] / (attn["ms"] * 1e-3) / 1e9 if attn["ms"] else 0.0,
                "tokens_per_s": rows * codes / statistics.median(ts), "tokens_per_s_min": rows * codes / max(ts),
                "tokens_per_s_max": rows * codes / min(ts),
                "workspace_mb": int(_lib.load().idxtts_gpt_workspace_bytes(uv._h, rows, cfg.cond_latents + 2 + 128 + 2 + 1, codes)) / 2 ** 20,
            }
            if not args.no_parity:
                shape["cache"][kv]["parity_6x96"] = parity_figures(uv, tw, cfg, kv)
        result["shapes"][name] = shape
        del uv
        torch.cuda.empty_cache()

    print(f"fp8 against bf16 KV cache, decode only, full-size synthetic GPT; {args.reps} timed generations per cache")
    for name, shape in result["shapes"].items():
        print(f"{name}: {shape['rows']} rows, {shape['weights']} weights, {shape['codes']} codes")
        a, b = shape["cache"]["bf16"], shape["cache"]["fp8"]
        print(f"  {'':30s}{'bf16':>14s}{'fp8':>14s}{'bf16 / fp8':>12s}")
        print(f"  {'decode attention, ms / step':30s}{a['attn_ms_per_step']:14.4f}{b['attn_ms_per_step']:14.4f}{a['attn_ms_per_step'] / b['attn_ms_per_step']:12.2f}")
        print(f"  {'its algorithmic GB/s':30s}{a['attn_alg_gb_per_s']:14.0f}{b['attn_alg_gb_per_s']:14.0f}")
        print(f"  {'chain, tokens / s (median)':30s}{a['tokens_per_s']:14.1f}{b['tokens_per_s']:14.1f}{a['tokens_per_s'] / b['tokens_per_s']:12.3f}")
        print(f"  {'  min .. max':30s}{a['tokens_per_s_min']:7.1f}..{a['tokens_per_s_max']:<7.1f}{b['tokens_per_s_min']:7.1f}..{b['tokens_per_s_max']:<7.1f}")
        print(f"  {'workspace, MiB':30s}{a['workspace_mb']:14.1f}{b['workspace_mb']:14.1f}")
        for kv in ("bf16", "fp8"):
            p = shape["cache"][kv].get("parity_6x96")
            if p:
                print(f"  parity {kv:5s}: max |dlogit| {p['max_abs_logit_diff']:.3e}, mean {p['mean_abs_logit_diff']:.3e} (logit std {p['logit_std']:.2f}), "
                      f"teacher-forced match {p['codes_match_rate_teacher_forced']:.4f}, worst oracle margin at a mismatch "
                      f"{p['worst_oracle_margin_at_a_mismatch']:.3e}, free-running first differences {p['first_difference_step_free_running']}")
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
