"""Prompt block for N new voices: N x encode() + from_features() (one voice per call, the only form before encode_batch) against
encode_batch(N) + from_features_batch, with the host and the device front-end.

    python tools/prompt_batch_bench.py [--voices 1,2,4,8] [--seconds 15] [--rate 48000] [--reps 5] [--warmup 2]

Each voice is a speaker prompt and an emotion prompt of --seconds at --rate (synthetic signal: chirp + tone + seeded noise), full-size
encoders with synthetic weights.  Every timed window ends in a device synchronise; the variants of one N are timed alternately inside
each repetition, after --warmup untimed rounds of all of them, and the median over --reps is printed.  The host time of file samples ->
PromptAudio (channel mean, two or three `sinc_resample` calls per voice) is measured on its own and reported beside the rows that need it:
    serial          N x (encode(PromptAudio, PromptAudio) + from_features)                       -- PromptAudio ready
    batch/host      encode_batch(N PromptAudio) + from_features_batch, frontend="host"           -- PromptAudio ready
    batch/gpu       the same with frontend="gpu": both filter banks on the device                -- PromptAudio ready
    raw: serial / batch/host     the rows above + the host resampling of the N voices (measured separately, added)
    raw: batch/gpu  encode_batch(N RawAudio) with frontend="gpu": resampling on the device too   -- measured as one window
Prints one markdown table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "index-tts_amd")]

import numpy as np
import torch


def signal(tag, sr, seconds):
    from indextts_amd import synth
    n = int(sr * seconds)
    t = np.arange(n) / sr
    return (0.4 * np.sin(2 * np.pi * (180 + 40 * np.sin(2 * np.pi * 1.3 * t)) * t) + 0.1 * np.sin(2 * np.pi * 1900 * t)
            + 0.05 * synth.uniform(tag, (n,), 1.0)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", default="1,2,4,8")
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prompt_batch_bench.py measures on the GPU; there is none here")
    from indextts_amd import weights
    from indextts_amd.config import CamPPlusConfig, PipelineConfig, RepCodecConfig, W2VBertConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.prompt import PromptEncoders, RawAudio
    dev = torch.device("cuda", 0)
    cfg = PipelineConfig()
    t0 = time.time()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    wg.update(weights.synth_gpt_cond_weights(cfg.gpt, tag="bench/gpt"))
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel")
    wcfg, ccfg, pcfg = W2VBertConfig(), RepCodecConfig(), CamPPlusConfig()
    wc = weights.synth_repcodec_weights(ccfg, tag="bench/codec")
    for k in ("codebook.weight", "out_project.weight", "out_project.bias"):
        ws[f"semantic_codec.quantizer.quantizers.0.{k}"] = wc[f"quantizer.quantizers.0.{k}"]
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan"), device=dev)
    gpu = PromptEncoders(weights.synth_w2vbert_weights(wcfg, tag="bench/w2v"), wc, weights.synth_campplus_weights(pcfg, tag="bench/campplus"),
                         tts.s2mel, device=dev, w2vbert_cfg=wcfg, codec_cfg=ccfg, campplus_cfg=pcfg, frontend="gpu")
    host = gpu.with_frontend("host")
    print(f"[prompt_batch_bench] synthetic weights + contexts in {time.time() - t0:.1f}s", file=sys.stderr)
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    counts = [int(v) for v in args.voices.split(",")]
    nmax = max(counts)
    raw_spk = [RawAudio(signal(f"pbb/spk/{i}", args.rate, args.seconds), args.rate) for i in range(nmax)]
    raw_emo = [RawAudio(signal(f"pbb/emo/{i}", args.rate, args.seconds), args.rate) for i in range(nmax)]

    def to_prompt_audio(i):
        return host._host_audio(raw_spk[i], False), host._host_audio(raw_emo[i], True)

    to_prompt_audio(0)      # resampler tables, BLAS threads
    per_voice = []
    ready = []
    for i in range(nmax):
        t = time.perf_counter()
        ready.append(to_prompt_audio(i))
        per_voice.append((time.perf_counter() - t) * 1e3)
    host_ms = statistics.median(per_voice)      # one voice: speaker (2 resamples) + emotion (1 resample)

    def sync_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    rows = []
    for n in counts:
        spk, emo = [r[0] for r in ready[:n]], [r[1] for r in ready[:n]]

        def serial():
            return [PromptConditioning.from_features(tts.gpt, host.encode(spk[i], emo[i]), emo_alpha=0.7) for i in range(n)]

        variants = {
            "serial": serial,
            "batch/host": lambda: PromptConditioning.from_features_batch(tts.gpt, host.encode_batch(spk, emo), emo_alpha=0.7),
            "batch/gpu": lambda: PromptConditioning.from_features_batch(tts.gpt, gpu.encode_batch(spk, emo), emo_alpha=0.7),
            "raw: batch/gpu": lambda: PromptConditioning.from_features_batch(tts.gpt, gpu.encode_batch(raw_spk[:n], raw_emo[:n]), emo_alpha=0.7),
        }
        for _ in range(args.warmup):
            for fn in variants.values():
                sync_ms(fn)
        ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                ms[k].append(sync_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        med["raw: serial"] = med["serial"] + n * host_ms
        med["raw: batch/host"] = med["batch/host"] + n * host_ms
        rows.append({"voices": n, "ms": med, "spread_ms": spread})
    order = ("serial", "batch/host", "batch/gpu", "raw: serial", "raw: batch/host", "raw: batch/gpu")
    print(f"host time of file samples -> PromptAudio, one voice ({args.seconds:g} s + {args.seconds:g} s at {args.rate} Hz): {host_ms:.1f} ms "
          f"(min {min(per_voice):.1f}, max {max(per_voice):.1f} over {nmax} voices)")
    print("| voices | " + " | ".join(order) + " |")
    print("|---|" + "---|" * len(order))
    for r in rows:
        print(f"| {r['voices']} | " + " | ".join(f"{r['ms'][k]:.1f}" for k in order) + " |")
    print("ms per N voices, median of %d; widest min-max spread of a measured cell: %.1f ms" %
          (args.reps, max(max(r["spread_ms"].values()) for r in rows)))
    print(json.dumps({"tool": "prompt_batch_bench", "seconds": args.seconds, "rate": args.rate, "reps": args.reps, "host_ms_per_voice": host_ms,
                      "rows": rows}))


if __name__ == "__main__":
    main()
