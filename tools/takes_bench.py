"""What several takes of one request cost, on the full-size GPT with synthetic weights (bf16 GPT weights, stop token biased away), at
configs[2]'s shapes: a 16-slot sampled decode session, 128-token texts (a 162-row prompt with its conditioning), bf16 and fp8 KV.

(a) Admission.  `admit(takes=4)` -- one prefill row, its keys and values written to four slots, four first tokens -- against four
    single admissions of the same prompt (four prefills), each timed with the host clock around the call(s) and a synchronise of the
    session's stream; the slots are evicted between calls.
(b) Fork.  A row decoded to 64 and to 512 generated positions is forked to 1, 3 and 7 destinations (`idxtts_gpt_session_fork`, the
    destinations evicted after each call), against a plain device-to-device copy of the bytes the fork writes (n times the row's cached
    bytes) and against the way without it: park the row once, resume it into n slots from the parked bytes, and resume the source.

Every figure is the median of `--cycles` calls (default 20) after three warm-up calls.

    python tools/takes_bench.py [--cycles 20]

Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "index-tts_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SLOTS, TEXT, TAKES = 16, 128, 4
HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}


def _timed(sess, fn) -> float:
    sess.stream.synchronize()
    t0 = time.perf_counter()
    fn()
    sess.stream.synchronize()
    return time.perf_counter() - t0


def _row(uv):
    from indextts_amd import synth
    cfg = uv.cfg
    conds = torch.from_numpy(synth.uniform("tbench/conds", (1, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    return uv.prompt_rows(conds, torch.from_numpy(synth.integers("tbench/text", (1, TEXT), 2, cfg.number_text_tokens)))[0]


def cached_bytes(cfg, kv: str, pos: int) -> int:
    """Bytes of keys, values and scales a row holds for `pos` positions."""
    e = {"bf16": 2, "fp8": 1}[kv]
    return cfg.layers * cfg.heads * (2 * pos * 64 * e + (8 * pos if kv == "fp8" else 0))


def admit_times(uv, kv: str, cycles: int) -> dict:
    uv.set_kv_format(kv)
    row = _row(uv)
    sess = uv.decode_session(SLOTS, max_prompt=int(row.shape[0]), max_new=64, sampled=True)
    samp = [dict(HF, seed=100 + j) for j in range(TAKES)]
    t = {"takes": [], "singles": []}
    for c in range(cycles + 3):
        got = []
        a = _timed(sess, lambda: got.extend(sess.admit([row], [[64] * TAKES], sampling=[samp], takes=TAKES)[0]))
        sess.evict(got)
        got = []
        b = _timed(sess, lambda: [got.extend(sess.admit([row], [64], sampling=[s])) for s in samp])
        sess.evict(got)
        if c >= 3:
            t["takes"].append(a); t["singles"].append(b)
    sess.close()
    return {"kv": kv, "prompt_rows": int(row.shape[0]), "takes": TAKES, "admit_takes_us": float(np.median(t["takes"])) * 1e6,
            "four_admissions_us": float(np.median(t["singles"])) * 1e6}


def fork_times(uv, kv: str, lengths, fans, cycles: int) -> list:
    from indextts_amd import _lib
    lib, cfg = _lib.load(), uv.cfg
    uv.set_kv_format(kv)
    row = _row(uv)
    P, cap = int(row.shape[0]), max(lengths) + 2
    sess = uv.decode_session(SLOTS, max_prompt=P, max_new=cap, sampled=True)
    ws, sp, out, done = _lib.ptr(sess._ws), sess._sp(), [], 1
    (src,) = sess.admit([row], [cap], sampling=[dict(HF, seed=1)])
    for n in sorted(lengths):
        assert sess.step(n - done) == []                             # n codes, still decoding
        done = n
        pos = P + n
        need = int(lib.idxtts_gpt_session_park_bytes(uv._h, src, ws, sp))
        with torch.cuda.stream(sess.stream):
            blob = torch.empty(need, dtype=torch.uint8, device=uv.device)
        for fan in fans:
            dst = [s for s in range(SLOTS) if s != src][:fan]
            ids = np.ascontiguousarray(dst, dtype=np.int32)
            moved = fan * cached_bytes(cfg, kv, pos)
            with torch.cuda.stream(sess.stream):
                a_buf, b_buf = (torch.empty(moved, dtype=torch.uint8, device=uv.device) for _ in range(2))

            def fork():
                _lib.check(lib.idxtts_gpt_session_fork(uv._h, src, -1, fan, ids.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(0),
                                                       ctypes.c_void_p(0), ws, sp))

            def park_resumes():
                wr = ctypes.c_size_t(0)
                _lib.check(lib.idxtts_gpt_session_park(uv._h, src, _lib.ptr(blob), need, ctypes.byref(wr), ws, sp))
                for s in dst + [src]:
                    _lib.check(lib.idxtts_gpt_session_resume(uv._h, s, _lib.ptr(blob), need, ws, sp))
            t = {"fork": [], "copy": [], "park": []}
            for c in range(cycles + 3):
                a = _timed(sess, fork)
                lib.idxtts_gpt_session_evict(uv._h, fan, ids.ctypes.data_as(ctypes.c_void_p), ws, sp)
                with torch.cuda.stream(sess.stream):
                    k = _timed(sess, lambda: b_buf.copy_(a_buf))
                b = _timed(sess, park_resumes)
                lib.idxtts_gpt_session_evict(uv._h, fan, ids.ctypes.data_as(ctypes.c_void_p), ws, sp)
                if c >= 3:
                    t["fork"].append(a); t["copy"].append(k); t["park"].append(b)
            med = {k: float(np.median(v)) for k, v in t.items()}
            out.append({"kv": kv, "codes": n, "pos": pos, "destinations": fan, "bytes_written": moved, "fork_us": med["fork"] * 1e6,
                        "copy_us": med["copy"] * 1e6, "park_and_resumes_us": med["park"] * 1e6,
                        "fork_gbps_written": moved / med["fork"] / 1e9, "copy_gbps_written": moved / med["copy"] / 1e9})
    sess.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=20)
    args = ap.parse_args()
    from indextts_amd import weights
    from indextts_amd.config import GPTConfig
    from indextts_amd.gpt import UnifiedVoice
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    cfg = GPTConfig()
    wg = weights.synth_gpt_weights(cfg, tag="bench/gpt")
    wg["mel_head.bias"][cfg.stop_mel_token] = -1e4
    uv = UnifiedVoice(wg, cfg, device=torch.device("cuda:0"), weight_format="bf16", kv_format="bf16")
    out = {"slots": SLOTS, "text_tokens": TEXT, "cycles": args.cycles,
           "admit": [admit_times(uv, kv, args.cycles) for kv in ("bf16", "fp8")],
           "fork": [r for kv in ("bf16", "fp8") for r in fork_times(uv, kv, (64, 512), (1, 3, 7), args.cycles)]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
