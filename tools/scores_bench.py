"""What recording every code's log-probability costs, and what ranking saves, on the full-size models with synthetic weights (bf16 GPT
weights and KV, stop token biased away) at configs[2]'s shapes: 128-token texts (a 162-row prompt with its conditioning), 512 codes.

(a) Decode step.  A sampled decode session of 1, 16 and 48 slots, every slot decoding (HF sampler 0.8 / 30 / 0.8), scores off
    (`decode_session(sampled=True)`: the `off` leg, which also runs on a commit without scores) and on (`scores=True`): the time of
    `--steps` replayed steps, host clock around `step()` and a synchronise of the session's stream, per step; the median of
    `--repeats` such windows after a warm-up window that captures the graph.
(b) Best of four.  `ContinuousPipeline(slots=16, allow_sampling=True, scores=True)`: four utterances x four takes (the 16 decode rows
    of configs[2]) as `submit(takes=4, keep=1)` against `submit(takes=4)`, alternating: wall time from submit to result, and the rows
    the acoustic stage ran (from `trace`).

    python tools/scores_bench.py [--legs off,on,keep] [--steps 128] [--repeats 3]

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

TEXT, CODES, PROMPT_FRAMES = 128, 512, 689
HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}


def step_times(uv, rows: int, scores: bool, steps: int, repeats: int) -> dict:
    from indextts_amd import synth
    cfg = uv.cfg
    conds = torch.from_numpy(synth.uniform("sbench/conds", (1, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    row = uv.prompt_rows(conds, torch.from_numpy(synth.integers("sbench/text", (1, TEXT), 2, cfg.number_text_tokens)))[0]
    cap = 4 + steps * (repeats + 1)
    sess = uv.decode_session(rows, max_prompt=int(row.shape[0]), max_new=cap, sampled=True, **({"scores": True} if scores else {}))
    left = list(range(rows))
    while left:      # (an admission prefills at most 16 prompts of this length at once comfortably)
        now, left = left[:16], left[16:]
        sess.admit([row] * len(now), [cap] * len(now), sampling=[dict(HF, seed=100 + s) for s in now], slots=now)
    sess.step(2)      # the eager step, then the capture
    windows = []
    for w in range(repeats + 1):
        sess.stream.synchronize()
        t0 = time.perf_counter()
        done = sess.step(steps)
        sess.stream.synchronize()
        dt = time.perf_counter() - t0
        assert not done, "a row ended inside the timed window"
        if w:
            windows.append(dt / steps * 1e6)
    sess.close()
    return {"rows": rows, "scores": scores, "step_us": float(np.median(windows)), "step_us_min": float(min(windows)),
            "step_us_max": float(max(windows))}


def keep_times(repeats: int) -> dict:
    from indextts_amd import synth, weights
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import ContinuousPipeline
    cfg = PipelineConfig()
    dev = torch.device("cuda:0")
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan"), device=dev, gpt_weight_format="bf16")
    cond = PromptConditioning.synthetic(cfg, prompt_frames=PROMPT_FRAMES, tag="bench/prompt").to(dev)
    text = torch.from_numpy(synth.integers("sbench/ptext", (4, TEXT), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8}
    out = {"utterances": 4, "takes": 4, "codes": CODES, "all": [], "keep1": [], "acoustic_rows_all": [], "acoustic_rows_keep1": []}
    with ContinuousPipeline(tts, slots=16, allow_sampling=True, scores=True, max_new=CODES) as pipe:
        for r in range(repeats + 1):
            for name, keep in (("all", None), ("keep1", 1)):
                pipe.trace = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = pipe.submit(text, cond, max_mel_tokens=CODES, sampling=dict(samp, seed=r), noise_seed=r, takes=4, keep=keep).result()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert len(res) == 4 and all(len(x) == (keep or 4) for x in res)
                if r:      # (the first round warms both up)
                    out[name].append(dt)
                    out["acoustic_rows_" + name].append(sum(e[3] for e in pipe.trace if e[0] == "acoustic"))
    for name in ("all", "keep1"):
        out[name + "_s"] = float(np.median(out[name]))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on,keep")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="1,16,48")
    args = ap.parse_args()
    legs = args.legs.split(",")
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    out = {"text_tokens": TEXT, "steps": args.steps, "repeats": args.repeats, "step": []}
    if "off" in legs or "on" in legs:
        from indextts_amd import weights
        from indextts_amd.config import GPTConfig
        from indextts_amd.gpt import UnifiedVoice
        cfg = GPTConfig()
        wg = weights.synth_gpt_weights(cfg, tag="bench/gpt")
        wg["mel_head.bias"][cfg.stop_mel_token] = -1e4
        uv = UnifiedVoice(wg, cfg, device=torch.device("cuda:0"), weight_format="bf16", kv_format="bf16")
        for rows in (int(x) for x in args.rows.split(",")):
            for leg in ("off", "on", "off", "on"):      # alternating: each leg twice
                if leg in legs:
                    out["step"].append(step_times(uv, rows, leg == "on", args.steps, args.repeats))
        del uv
    if "keep" in legs:
        out["keep"] = keep_times(args.repeats)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
