"""Shared by the front-end tests (test_fbank_gpu.py, test_resample_gpu.py, test_prompt_batch_gpu.py): the test signal, the host references
computed once, and the float32 / float64 restatements that give each tolerance its floor.

The device front-end (csrc/fbank.hip) computes in float32; its host references do not (`features.kaldi_fbank` is float64 up to the log;
`audioio.sinc_resample` sums in float32 in BLAS's order).  Neither tolerance is invented: each is 4 x the deviation of a plain numpy
restatement in the OTHER precision from the host reference on the very input that is compared -- what changing the precision alone costs --
and the factor 4 covers what differs beyond that (the MFMA's k order, the device logf).
"""
import functools
import math

import numpy as np

from indextts_amd import audioio, features, synth


def audio(tag, sr, n):
    """tests/test_prompt_gpu.py::_audio for n samples: chirp + tone + seeded noise, so every mel bin carries energy."""
    n = int(n)
    t = np.arange(n) / sr
    return (0.4 * np.sin(2 * np.pi * (180 + 40 * np.sin(2 * np.pi * 1.3 * t)) * t) + 0.1 * np.sin(2 * np.pi * 1900 * t)
            + 0.05 * synth.uniform(tag, (n,), 1.0)).astype(np.float32)


# ---- filter bank ----------------------------------------------------------------------------------------------------------------
FBANK_SINGLE = (400, 559, 560, 720, 2480, 4000)          # frames 1, 1, 2, 3 (odd), 14, 23
FBANK_RAGGED = (720, 4000, 560, 2480)
FBANK_SWITCH = (16240, 16240, 9840)                      # 100 + 100 + 60 = 260 frames: across lin()'s 256-row switch
FBANK_LONG = 41600                                       # 2.6 s
SCALES = (1.0, float(2 ** 15))


@functools.lru_cache(maxsize=None)
def fbank_audio(n):
    return audio(f"t/fbank/{n}", 16000, n)


def frames_of(n):
    return 0 if n < 400 else 1 + (n - 400) // 160


def fbank_f32(x, scale):
    """features.kaldi_fbank restated in float32 numpy, the DFT as a product with the windowed cos / sin matrix."""
    x = np.asarray(x, np.float32) * np.float32(scale)
    T = frames_of(x.size)
    fr = np.lib.stride_tricks.as_strided(x, (T, 400), (160 * x.strides[0], x.strides[0])).astype(np.float32)
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=np.float32)
    pre = np.empty_like(fr)
    pre[:, 1:] = fr[:, 1:] - np.float32(0.97) * fr[:, :-1]
    pre[:, 0] = fr[:, 0] * np.float32(0.03)
    win = features.povey_window(400)
    ang = 2.0 * np.pi * ((np.arange(257)[:, None] * np.arange(400)[None, :]) % 512) / 512
    re = pre @ (win * np.cos(ang)).astype(np.float32).T
    im = pre @ (-win * np.sin(ang)).astype(np.float32).T
    power = re * re + im * im
    mel = power @ features.kaldi_mel_filters().astype(np.float32)
    return np.log(np.maximum(mel, np.float32(1.192092955078125e-07))).astype(np.float32)


def normalise_f32(f):
    f = np.asarray(f, np.float32)
    mean = f.mean(0, keepdims=True, dtype=np.float32)
    var = ((f - mean) ** 2).sum(0, keepdims=True, dtype=np.float32) / np.float32(f.shape[0] - 1)
    return ((f - mean) / np.sqrt(var + np.float32(1e-7))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fbank_host(n, scale):
    """features.kaldi_fbank of the test signal of n samples (float64 inside) -- computed once"""
    return features.kaldi_fbank(fbank_audio(n), scale=scale)


@functools.lru_cache(maxsize=None)
def w2v_host(n):
    return features.seamless_m4t_features(fbank_audio(n))


def fbank_lengths():
    return sorted(set(FBANK_SINGLE + FBANK_RAGGED + FBANK_SWITCH + (FBANK_LONG,)))


@functools.lru_cache(maxsize=None)
def fbank_floors(n):
    """max |float32 restatement - host| of (the log-mel energies, the same minus their mean over time, the normalised w2v-BERT features)
    for the test signal of n samples: every input is judged against its OWN floor (a 3-frame row, whose three near-equal frames divide
    by a small deviation, does not widen the bound of a long row)."""
    return fbank_floors_of((fbank_audio(n),))


def campplus_host(x):
    f = features.kaldi_fbank(x)
    return f - f.mean(axis=0, keepdims=True)


def fbank_floors_of(waves):
    raw = cp = norm = 0.0
    for x in waves:
        n = x.size
        for s in SCALES:
            raw = max(raw, float(np.abs(fbank_f32(x, s) - features.kaldi_fbank(x, scale=s)).max()))
        f = fbank_f32(x, 1.0)
        cp = max(cp, float(np.abs((f - f.mean(0, keepdims=True, dtype=np.float32)) - campplus_host(x)).max()))
        T = frames_of(n)
        if T >= 2:
            got = normalise_f32(fbank_f32(x, SCALES[1]))
            want = features.seamless_m4t_features(x)["input_features"][0].reshape(-1, 80)[:T]
            norm = max(norm, float(np.abs(got - want).max()))
    return raw, cp, norm


# ---- resampler --------------------------------------------------------------------------------------------------------------------
RATE_PAIRS = ((48000, 16000), (44100, 22050), (44100, 16000), (48000, 22050), (22050, 16000), (16000, 22050))


def resample_lengths(orig_freq, new_freq):
    orig = orig_freq // math.gcd(orig_freq, new_freq)
    return (1, orig - 1, orig, orig + 1, 2 * orig + 3, int(0.2 * orig_freq))


@functools.lru_cache(maxsize=None)
def resample_audio(orig_freq, n):
    return audio(f"t/resample/{orig_freq}/{n}", orig_freq, n)


@functools.lru_cache(maxsize=None)
def resample_host(orig_freq, new_freq, n):
    return audioio.sinc_resample(resample_audio(orig_freq, n), orig_freq, new_freq)


def resample_f64(x, orig_freq, new_freq):
    """audioio.sinc_resample with the same float32 taps, products and sums in float64"""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    kern, width = audioio.sinc_resample_kernel(orig, new)
    w = np.pad(np.asarray(x, np.float64), (width, width + orig))
    nfr = (w.size - kern.shape[1]) // orig + 1
    fr = np.lib.stride_tricks.as_strided(w, (nfr, kern.shape[1]), (w.strides[0] * orig, w.strides[0]))
    return (fr @ kern.astype(np.float64).T).reshape(-1)[: int(math.ceil(new * len(x) / orig))]


@functools.lru_cache(maxsize=None)
def resample_floor():
    """max |audioio.sinc_resample - its float64 evaluation| over every input of the resampler tests"""
    worst = 0.0
    for o, nw in RATE_PAIRS:
        for n in resample_lengths(o, nw):
            worst = max(worst, float(np.abs(resample_host(o, nw, n) - resample_f64(resample_audio(o, n), o, nw)).max()))
    return worst
