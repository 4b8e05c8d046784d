#!/usr/bin/env python3
"""What idxtts_set_acoustic_bf16 buys and costs at configs[2]'s acoustic shapes: the CFM solver on 16 rows of T = 689 + 880 frames
(20 steps, cfg 0.7) and BigVGAN on the 16 x 880 generated frames, switch off against switch on.

One process.  Weights and inputs are synthetic and seeded.  Times: host clock around calls that end in a device synchronise, the two
arithmetics interleaved (off, on, off, on, ...), the first round discarded as warm-up, median and spread of the rest.  Per-kernel
times: the library's per-launch profiler (an event pair around every launch) in a pass of its own behind the timed rounds, per
kernel family.  Errors: mel and waveform of each arithmetic against the GEMM_F32 run of the same inputs (mel L1 = mean |diff|, max
|diff|; waveform SNR in dB, the waveform being the vocoder's output on that arithmetic's own mel).

    python tools/acoustic_bf16_bench.py [--reps 4] [--rows 16] [--steps 20] [--json out.json]
Prints a table and one JSON line."""
import argparse
import json
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
from indextts_amd.vocoder import BigVGAN  # noqa: E402

FAMILIES = {"gemm": ("gemm_bf16x3_v2_kernel", "split_planes_kernel"), "attention": ("flash_attn_planes_kernel", "flash_attn_bf16x3_kernel"),
            "conv": ("conv1d_bf16x3_kernel",)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4, help="timed rounds per arithmetic behind the warm-up round")
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--prompt-frames", type=int, default=689)
    ap.add_argument("--frames", type=int, default=880)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", file=sys.stderr)
        return 1
    cfg = PipelineConfig()
    dev = torch.device("cuda:0")
    _lib.load()
    sm = S2Mel(weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel"), cfg.s2mel, device=dev)
    voc = BigVGAN(weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/voc"), cfg.bigvgan)
    B, Tp, Tg = args.rows, args.prompt_frames, args.frames
    T = Tp + Tg
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(B, T, cfg.s2mel.content_dim, generator=g).to(dev)
    prompt = torch.randn(B, cfg.s2mel.in_channels, Tp, generator=g).to(dev)
    style = torch.randn(B, cfg.s2mel.style_dim, generator=g).to(dev)
    z = torch.randn(B, cfg.s2mel.in_channels, T, generator=g).to(dev)

    def s2mel():
        return sm.cfm_inference(mu, [T] * B, prompt, style, None, args.steps, inference_cfg_rate=0.7, z=z)[:, :, Tp:].float().contiguous()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def arithmetic(name):
        _lib.set_gemm_mode(_lib.GEMM_F32 if name == "f32" else _lib.GEMM_BF16X3)
        _lib.set_acoustic_bf16(name == "bf16")

    # ---- outputs of the three arithmetics on the same inputs (also the first warm-up of every shape) ----
    mel, wav = {}, {}
    for name in ("f32", "bf16x3", "bf16"):
        arithmetic(name)
        mel[name] = s2mel()
        wav[name] = voc(mel[name], clamp=False)
    torch.cuda.synchronize()
    errors = {}
    for name in ("bf16x3", "bf16"):
        dm = (mel[name] - mel["f32"]).abs()
        dw = (wav[name] - wav["f32"]).double()
        snr = 10.0 * torch.log10(wav["f32"].double().pow(2).sum() / dw.pow(2).sum().clamp_min(1e-300)).item()
        errors[name] = {"mel_l1": dm.mean().item(), "mel_max": dm.max().item(), "mel_abs_mean": mel["f32"].abs().mean().item(), "wav_snr_db": snr}

    # ---- end-to-end times, interleaved; round 0 is warm-up ----
    times = {"bf16x3": {"s2mel": [], "vocoder": []}, "bf16": {"s2mel": [], "vocoder": []}}
    for rnd in range(args.reps + 1):
        for name in ("bf16x3", "bf16"):
            arithmetic(name)
            m, ts = timed(s2mel)
            _, tv = timed(lambda: voc(m, clamp=False))
            if rnd:
                times[name]["s2mel"].append(ts)
                times[name]["vocoder"].append(tv)

    # ---- per-kernel times: the per-launch profiler, one pass per arithmetic ----
    kernels = {}
    for name in ("bf16x3", "bf16"):
        arithmetic(name)
        _lib.profile_enable(True)
        m = s2mel()
        voc(m, clamp=False)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        kernels[name] = {fam: sum(v["ms"] for k, v in prof.items() if k.startswith(names)) for fam, names in FAMILIES.items()}
        kernels[name]["all"] = sum(v["ms"] for v in prof.values())
    arithmetic("bf16x3")

    def med(xs):
        return statistics.median(xs) * 1e3

    print(f"acoustic stage at {B} rows, T = {Tp} + {Tg}, {args.steps} steps, cfg 0.7; vocoder on {B} x {Tg} frames; {args.reps} timed rounds")
    print(f"{'':22s}{'split-bf16 (off)':>20s}{'bf16 (on)':>16s}{'off / on':>10s}")
    for what in ("s2mel", "vocoder"):
        a, b = med(times["bf16x3"][what]), med(times["bf16"][what])
        sa = (max(times["bf16x3"][what]) - min(times["bf16x3"][what])) * 1e3
        sb = (max(times["bf16"][what]) - min(times["bf16"][what])) * 1e3
        print(f"{what + ' call, ms':22s}{a:14.1f} +-{sa:4.1f}{b:10.1f} +-{sb:4.1f}{a / b:10.2f}")
    for fam in ("gemm", "attention", "conv", "all"):
        a, b = kernels["bf16x3"][fam], kernels["bf16"][fam]
        print(f"{fam + ' kernels, ms':22s}{a:20.1f}{b:16.1f}{a / b if b else float('nan'):10.2f}")
    for name in ("bf16x3", "bf16"):
        e = errors[name]
        print(f"{name:8s} vs fp32: mel L1 {e['mel_l1']:.3e} (mean |mel| {e['mel_abs_mean']:.3f}), mel max {e['mel_max']:.3e}, waveform SNR {e['wav_snr_db']:.1f} dB")
    result = {"rows": B, "prompt_frames": Tp, "frames": Tg, "steps": args.steps, "reps": args.reps,
              "ms": {n: {w: med(v) for w, v in t.items()} for n, t in times.items()}, "kernel_ms": kernels, "errors": errors}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
