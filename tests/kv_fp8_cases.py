"""Helpers of the fp8 KV-cache tests (include/idxtts.h, IDXTTS_KV_FP8): a numpy restatement of the quantiser that shares nothing with the
library -- scales from `frexp`, e4m3 codes from an explicit grid -- the vectors both test files quantise, and `fp8_stack`, the oracle's
transformer stack with that quantiser where the bf16 cache mode casts."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def fp8_grid():
    """Every finite non-negative OCP e4m3fn value by code 0..126 (bias 7, 3 mantissa bits, max 448)."""
    vals = []
    for c in range(127):
        e, m = (c >> 3) & 15, c & 7
        vals.append(m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return np.array(vals, dtype=np.float64)


GRID = fp8_grid()


def scale_exponents(amax):
    """e with s = 2^e = 2^ceil(log2(amax / 448)), clamped to [-100, 100]; 0 for amax == 0.  amax = m 2^k with m in [0.5, 1), and
    448 = 0.875 * 2^9: amax / 448 = (m / 0.875) 2^(k - 9) with m / 0.875 in [0.571, 1.143), so the ceiling is k - 9, plus 1 when m > 0.875."""
    amax = np.asarray(amax, dtype=np.float32).astype(np.float64)
    m, k = np.frexp(amax)
    e = k.astype(np.int64) - 9 + (m > 0.875)
    return np.where(amax == 0.0, 0, np.clip(e, -100, 100))


def encode_e4m3(y):
    """float64 values with |y| <= 448 -> codes: the nearest grid value, a tie to the even code; the sign bit of y on top."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert (a <= 448.0).all()
    hi = np.minimum(np.searchsorted(GRID, a, side="left"), 126)
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - GRID[lo], GRID[hi] - a
    code = np.where(dhi < dlo, hi, np.where(dhi > dlo, lo, np.where(lo % 2 == 0, lo, hi)))
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def decode_e4m3(code):
    code = np.asarray(code, dtype=np.uint8)
    return np.where(code & 0x80, -1.0, 1.0) * GRID[np.minimum(code & 0x7F, 126)]


def quantize(x):
    """x [..., 64] float32 -> (codes uint8 [..., 64], scales float32 [...], cached values float32 [..., 64])."""
    x = np.asarray(x, dtype=np.float32)
    e = scale_exponents(np.abs(x).max(axis=-1))
    s = np.ldexp(1.0, e)
    y = x.astype(np.float64) / s[..., None]              # exact: a power of two, and float64 holds every float32 scaled by 2^+-100
    y = np.where(np.abs(y) < 2.0 ** -126, np.copysign(0.0, y), y)      # below the fp32 normal range: far below half of 2^-9 anyway
    codes = encode_e4m3(y)
    return codes, s.astype(np.float32), (decode_e4m3(codes) * s[..., None]).astype(np.float32)


def Q(t: torch.Tensor) -> torch.Tensor:
    """Keys or values [..., 64] as the fp8 cache holds them, in t's dtype (the quantiser reads them as fp32)."""
    return torch.from_numpy(quantize(t.detach().to(torch.float32).numpy())[2]).to(t.dtype)


def case_vectors():
    """[n, 64] float32: what the CPU test checks the restatement on and the GPU test the device quantiser."""
    rng = np.random.default_rng(20240607)
    out = []
    mags = 2.0 ** rng.uniform(-20, 10, size=(3000, 1))                    # random vectors of magnitude 2^-20 .. 2^10
    out.append((rng.standard_normal((3000, 64)) * mags).astype(np.float32))
    out.append(np.zeros((1, 64), np.float32))                             # all zero, and -0.0 among zeros and beside values
    z = np.zeros((2, 64), np.float32); z[0, 5] = -0.0; z[1, :] = 1.0; z[1, 7] = -0.0
    out.append(z)
    edge = []                                                             # amax exactly 448 * 2^e and the next float above: the scale steps there
    for e in range(-24, 12):
        for top in (np.float32(448.0 * 2.0 ** e), np.nextafter(np.float32(448.0 * 2.0 ** e), np.float32(np.inf)),
                    np.nextafter(np.float32(448.0 * 2.0 ** e), np.float32(0.0))):
            v = (rng.standard_normal(64) * 0.3 * float(top)).astype(np.float32)
            v = np.clip(v, -top, top); v[rng.integers(64)] = top * (1 if e % 2 else -1)
            edge.append(v)
    out.append(np.array(edge, np.float32))
    mids = np.concatenate([GRID, 0.5 * (GRID[:-1] + GRID[1:])])             # every code value and every midpoint (ties to even) ...
    mids = np.concatenate([mids, -mids]).astype(np.float32)
    for sc in (1.0, 2.0 ** -9, 2.0 ** 5):                                   # ... at three scales; amax = 448 * scale pins s = scale
        for i in range(0, len(mids), 63):
            v = np.zeros(64, np.float32); chunk = mids[i:i + 63]; v[:len(chunk)] = chunk; v[63] = 448.0
            out.append((v * np.float32(sc))[None])
    sub = np.zeros((4, 64), np.float32)                                     # the subnormal range of the scaled grid: below 2^-6 * s
    sub[:, 0] = 448.0 * 2.0 ** -3
    sub[:, 1:] = (rng.uniform(-1, 1, (4, 63)) * 2.0 ** -6 * 2.0 ** -3).astype(np.float32)
    sub[0, 1:9] = np.array([1, 2, 3, -1, -2, 0.5, -0.5, 0.25]) * 2.0 ** -9 * 2.0 ** -3       # grid points, half a step (tie to 0), a quarter
    out.append(sub)
    return np.concatenate(out, axis=0)


def fp8_stack(w, cfg, emb, key_valid=None, past=None, kv_round=False):
    """oracle.gpt.gpt2_stack with every key / value quantised by Q when it is produced (prefill and decode alike) where the bf16 cache
    mode rounds -- whatever `kv_round` says: oracle.parity passes False for a format it does not know."""
    from oracle.gpt import _t, gelu_new
    B, S, d = emb.shape
    H, hd = cfg.heads, cfg.head_dim
    past_len = 0 if past is None else past[0][0].shape[2]
    total = past_len + S
    qpos = torch.arange(past_len, total)[:, None]
    kpos = torch.arange(total)[None, :]
    allowed = (kpos <= qpos)[None, None]
    if key_valid is not None:
        allowed = allowed & key_valid.bool()[:, None, None, :]
    x = emb
    present = []
    for i in range(cfg.layers):
        p = f"gpt.h.{i}"
        h = F.layer_norm(x, (d,), _t(w, f"{p}.ln_1.weight"), _t(w, f"{p}.ln_1.bias"), 1e-5)
        qkv = h @ _t(w, f"{p}.attn.c_attn.weight") + _t(w, f"{p}.attn.c_attn.bias")
        q, k, v = qkv.split(d, dim=2)
        q = q.view(B, S, H, hd).transpose(1, 2)
        k = Q(k.view(B, S, H, hd).transpose(1, 2))
        v = Q(v.view(B, S, H, hd).transpose(1, 2))
        if past is not None:
            k = torch.cat([past[i][0], k], dim=2)
            v = torch.cat([past[i][1], v], dim=2)
        present.append((k, v))
        scores = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        scores = torch.where(allowed, scores, torch.full_like(scores, torch.finfo(scores.dtype).min))
        att = torch.softmax(scores, dim=-1)
        a = (att @ v).transpose(1, 2).reshape(B, S, d)
        a = a @ _t(w, f"{p}.attn.c_proj.weight") + _t(w, f"{p}.attn.c_proj.bias")
        x = x + a
        h = F.layer_norm(x, (d,), _t(w, f"{p}.ln_2.weight"), _t(w, f"{p}.ln_2.bias"), 1e-5)
        m = gelu_new(h @ _t(w, f"{p}.mlp.c_fc.weight") + _t(w, f"{p}.mlp.c_fc.bias"))
        m = m @ _t(w, f"{p}.mlp.c_proj.weight") + _t(w, f"{p}.mlp.c_proj.bias")
        x = x + m
    x = F.layer_norm(x, (d,), _t(w, "gpt.ln_f.weight"), _t(w, "gpt.ln_f.bias"), 1e-5)
    return x, present


# ---- the tiny models of the greedy test (test_gpt_gpu.py::test_bf16_kv_cache_long_decode_vs_oracle's), shared with the CPU test ----
GREEDY_SHAPES = [(2, 2, 300), (9, 16, 240)]      # (B, heads, NEW): keys split over workgroups / unsplit with pos past 512
# Weights on which the reference alone is stable: the patched oracle decodes the same codes in fp32 and in float64 (8 torch threads;
# tests/test_kv_fp8_cpu.py asserts it).  The bf16 test's own weights do for 2 heads; with 16 heads they flip one row of nine at a
# near-tie of 1e-3, as do two of the first three other tags tried.
WEIGHT_TAG = {2: "t/gpt/kv16/2", 16: "t/gpt/kv8/16/2"}


def greedy_case(B, heads):
    from indextts_amd import synth, weights
    from indextts_amd.config import GPTConfig
    cfg = GPTConfig(model_dim=64 * heads, heads=heads, layers=2, number_mel_codes=130, number_text_tokens=90, start_mel_token=128,
                    stop_mel_token=129, max_mel_tokens=700, max_text_tokens=300, cond_latents=8)
    w = weights.synth_gpt_weights(cfg, tag=WEIGHT_TAG[heads])
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = -1e4          # never stop
    L = 290
    lat = torch.from_numpy(synth.uniform("t/gpt/kv16/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/gpt/kv16/emo", (B, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/gpt/kv16/text", (B, L), 2, cfg.number_text_tokens))
    text[1, 23:] = cfg.stop_text_token                      # left padding, kstart
    return cfg, w, lat, emo, text
