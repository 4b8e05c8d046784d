"""ContinuousPipeline against BatchPipeline at equal decode width, full-size model with synthetic weights (bf16 GPT weights and KV).

Two workloads over the same utterances (configs[2]-shaped: 128 text tokens, 689-frame prompt, EOS suppressed so that lengths are
exactly the caps):
  (a) fixed: every utterance 512 codes -- BatchPipeline takes requests of 16 utterances, ContinuousPipeline the same requests;
  (b) ragged: utterance caps drawn with a fixed seed from 256..768 codes.  ContinuousPipeline takes one request per utterance with
      its own cap; BatchPipeline takes the same utterances as requests of 16 whose cap is the longest of the 16 (a static batch decodes
      until its longest row is done).  Throughput counts the audio of the utterances' own caps for both (for BatchPipeline the
      acoustic stage also renders the padding codes: an upper bound of its cost where rows would stop on their own).
The two pipelines alternate, every shape is warmed up first, and each is repeated so the spread is known.  Prints one JSON line.
--sampling compares ContinuousPipeline with greedy requests against ContinuousPipeline(allow_sampling=True) with HF-sampled requests
(temperature 0.8, top_k 30, top_p 0.8: IndexTTS2.infer's defaults; one seed per request) on the same workloads instead.
--beams N compares BatchPipeline and ContinuousPipeline(num_beams=N, slots = 16 N: 16 utterances in flight in both) on beam-sample
requests with IndexTTS2.infer's defaults (num_beams N, temperature 0.8, top_k 30, top_p 0.8, length_penalty 0; seeded).
--acoustic-coalesce N: ContinuousPipeline(acoustic_coalesce=N) -- a free acoustic worker renders up to N finished requests (any
prompts) as one s2mel + vocoder batch.  --speakers K: K synthetic prompts of different lengths (400, 689, 1000, then 400 + 150 k
frames) assigned to the utterances round-robin; a static batch then holds rows of several speakers (one PromptConditioning per
row), and each request's noise covers its own prompt.  The JSON line also reports, per pipeline, the padding fraction of the
acoustic batches ContinuousPipeline ran: the share of the s2mel frames B * T_max that lie beyond each row's own Tp_b + Tg_b.
--noise-seed: requests carry submit(noise_seed=...) instead of an explicit noise tensor (the only other form that is merged).

    python tools/continuous_bench.py [--utterances 64] [--reps 3] [--sampling | --beams 3] [--acoustic-coalesce 4] [--speakers 3]
                                     [--workloads ragged] [--noise-seed]
"""
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poll-steps", type=int, default=16)
    ap.add_argument("--sampling", action="store_true", help="greedy against HF-sampled requests, both on ContinuousPipeline")
    ap.add_argument("--beams", type=int, default=1, help="N > 1: beam-sample requests, BatchPipeline against ContinuousPipeline(num_beams=N)")
    ap.add_argument("--acoustic-coalesce", type=int, default=1, help="ContinuousPipeline(acoustic_coalesce=N)")
    ap.add_argument("--speakers", type=int, default=1, help="K prompts of different lengths, round-robin over the utterances")
    ap.add_argument("--workloads", default="fixed,ragged", help="comma-separated subset of fixed,ragged")
    ap.add_argument("--noise-seed", action="store_true", help="submit(noise_seed=request number) instead of explicit noise tensors")
    args = ap.parse_args()
    if args.beams > 1 and args.sampling:
        ap.error("--sampling and --beams are separate comparisons")
    from indextts_amd import synth, weights
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import BatchPipeline, ContinuousPipeline
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    dev = torch.device("cuda:0")
    cfg = PipelineConfig()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=dev, gpt_weight_format="bf16", gpt_kv_format="bf16")
    L, W, N = 128, args.slots, args.utterances
    K = max(1, args.speakers)
    plens = [689] if K == 1 else [(400, 689, 1000)[k] if k < 3 else 400 + 150 * k for k in range(K)]
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=plens[0], tag="bench/prompt").to(dev)] if K == 1 else \
        [PromptConditioning.synthetic(cfg, prompt_frames=p, tag=f"cbench/prompt{k}").to(dev) for k, p in enumerate(plens)]
    spk = [i % K for i in range(N)]          # utterance i speaks with prompt spk[i]
    text = torch.from_numpy(synth.integers("cbench/text", (N, L), 2, cfg.gpt.number_text_tokens))
    rng = np.random.default_rng(7)
    caps = {"fixed": [512] * N, "ragged": [int(c) for c in rng.integers(256, 769, N)]}
    caps = {wl: caps[wl] for wl in args.workloads.split(",")}
    frame_s = cfg.bigvgan.total_upsample / cfg.bigvgan.sampling_rate

    def noise(k, rows, Tp, M):
        if args.noise_seed:
            return None
        return torch.from_numpy(synth.uniform(f"cbench/noise/{k}", (rows, cfg.s2mel.in_channels, Tp + int(M * cfg.code_to_frame)), 1.7)).to(dev)

    def cond_of(idx):        # one prompt for the request, or one per row when its utterances have different speakers
        if len({spk[i] for i in idx}) == 1:
            return conds[spk[idx[0]]]
        return [conds[spk[i]] for i in idx]

    jobs = {}
    for wl, cp in caps.items():
        static = []          # BatchPipeline: requests of W utterances, cap = the longest
        for g in range(0, N, W):
            idx = list(range(g, min(g + W, N)))
            M = max(cp[g:g + W])
            static.append((text[g:g + W], M, noise(f"{wl}/s{g}", len(idx), max(plens[spk[i]] for i in idx), M), cond_of(idx)))
        if wl == "fixed" and K == 1:
            cont = static
        else:                # ContinuousPipeline: one request per utterance, its own cap and prompt
            cont = [(text[i:i + 1], cp[i], noise(f"{wl}/c{i}", 1, plens[spk[i]], cp[i]), conds[spk[i]]) for i in range(N)]
        jobs[wl] = {"batch": static, "continuous": cont,
                    "audio_s": sum(int(c * cfg.code_to_frame) for c in cp) * frame_s}

    traces = {}

    def continuous(**kw):
        p = ContinuousPipeline(tts, slots=W, decode_lanes=1, poll_steps=args.poll_steps, max_new=800,
                               acoustic_coalesce=args.acoustic_coalesce, **kw)
        p.trace = traces.setdefault("continuous", [])
        return p

    pipes = {"batch": lambda: BatchPipeline(tts, decode_lanes=1), "continuous": continuous}
    sampling = {}
    if args.sampling:
        pipes = {"continuous": pipes["continuous"],
                 "continuous_sampled": lambda: ContinuousPipeline(tts, slots=W, decode_lanes=1, poll_steps=args.poll_steps, max_new=800,
                                                                  allow_sampling=True)}
        for wl in jobs:
            jobs[wl]["continuous_sampled"] = jobs[wl]["continuous"]
        sampling["continuous_sampled"] = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8}
    if args.beams > 1:
        nb = args.beams
        pipes["continuous"] = lambda: ContinuousPipeline(tts, slots=W * nb, decode_lanes=1, poll_steps=args.poll_steps, max_new=800,
                                                         num_beams=nb)
        beam = {"do_sample": True, "num_beams": nb, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}
        sampling["batch"] = sampling["continuous"] = beam
    seeded = {"continuous", "continuous_sampled"}      # BatchPipeline's gpt_stage draws its seed from torch's global RNG (seeded below)

    def run(kind, wl):
        with pipes[kind]() as pipe:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp = sampling.get(kind)
            futs = [pipe.submit(t, c, max_mel_tokens=M, noise=z, noise_seed=i if args.noise_seed else None, sampling=(dict(sp, seed=i) if kind in seeded else dict(sp)) if sp else None)
                    for i, (t, M, z, c) in enumerate(jobs[wl][kind])]
            for f in futs:
                f.result()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

    out = {"utterances": N, "slots": W, "text_tokens": L, "prompt_frames": plens, "reps": args.reps, "poll_steps": args.poll_steps,
           "sampling": bool(args.sampling), "num_beams": args.beams, "acoustic_coalesce": args.acoustic_coalesce, "speakers": K,
           "noise_seed": bool(args.noise_seed)}
    torch.manual_seed(0)
    base, other = ("continuous", "continuous_sampled") if args.sampling else ("batch", "continuous")
    for wl in caps:
        for kind in pipes:          # warm-up: every shape (prefill widths, graphs, acoustic lengths) once
            run(kind, wl)
        rates = {k: [] for k in pipes}
        traces.get("continuous", []).clear()
        for _ in range(args.reps):
            for kind in pipes:      # alternated
                rates[kind].append(jobs[wl]["audio_s"] / run(kind, wl))
        acoustic = traces.get("continuous", [])
        if acoustic and args.beams == 1 and not args.sampling and all(int(c[0].shape[0]) == 1 for c in jobs[wl]["continuous"]):
            # what the timed ContinuousPipeline runs' acoustic jobs were made of: requests per job, and the padding of the mixed-length
            # batches (frames beyond each row's own Tp_b + Tg_b, of B * T_max)
            cont = jobs[wl]["continuous"]
            used = padded = 0
            for *_, reqs in acoustic:
                fr = [plens[spk[k]] + int(cont[k][1] * cfg.code_to_frame) for k in reqs]
                used += sum(fr)
                padded += len(fr) * max(fr)
            out.setdefault("acoustic_jobs", {})[wl] = {
                "jobs": len(acoustic), "requests_per_job_mean": float(np.mean([len(t[4]) for t in acoustic])),
                "rows_per_job_max": max(t[3] for t in acoustic), "padding_fraction": 1.0 - used / padded,
                "seconds_mean": float(np.mean([t[2] - t[1] for t in acoustic]))}
        out[wl] = {k: {"audio_s_per_s_median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in rates.items()}
        out[wl][f"{other}_over_{base}"] = out[wl][other]["audio_s_per_s_median"] / out[wl][base]["audio_s_per_s_median"]
        out[wl]["audio_s"] = jobs[wl]["audio_s"]
        print(f"[continuous_bench] {wl}: {json.dumps(out[wl])}", file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
