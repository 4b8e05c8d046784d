"""Device mirrors of the prompt block's front-end, backed by libidxtts_hip (csrc/fbank.hip): what `features.py` and `audioio.py`
compute in numpy on the host, for a ragged batch of prompts that is already on the GPU.

  * `KaldiFbank()(audio [B,N], n_samples, scale, mode)` restates `features.kaldi_fbank` (16 kHz, 400-sample povey frames, hop 160,
    snip_edges, 512-point power spectrum, 80 Kaldi mel bins from 20 Hz, log(max(., 2^-23))) and its two users' finishing steps:
        `seamless_m4t_features(audio, n_samples)`  = `features.seamless_m4t_features`  (infer_v2.py:633, 680; samples * 2^15, every bin
                                                      normalised over the row's frames, frames stacked in pairs)
        `campplus_features(audio, n_samples)`      = `kaldi_fbank(x) - mean over time`   (infer_v2.py:641-646)
    The window and the filter table are `features.povey_window` / `features.kaldi_mel_filters`, loaded as tensors of the context.
  * `SincResampler()(x [B,N], lengths, orig_freq, new_freq)` restates `audioio.sinc_resample` (torchaudio's `sinc_interp_hann`
    polyphase correlation) with the float32 table of `audioio.sinc_resample_kernel`; equal rates return the input.
Rows are ragged through host lengths; every row equals its own B = 1 call bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_void_p
from typing import Optional

import numpy as np
import torch

from . import _lib, features

_MODES = {"raw": _lib.FBANK_RAW, "campplus": _lib.FBANK_CAMPPLUS, "w2vbert": _lib.FBANK_W2VBERT}


def _device_rows(x, what: str) -> torch.Tensor:
    """`x` as a contiguous float32 [B, N] GPU tensor; anything that is not on the GPU already is an error (no silent upload)."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError(f"{what}: expected a ROCm GPU tensor; the HIP path has no CPU fallback")
    if x.dim() != 2:
        raise ValueError(f"{what} must be [B, samples]")
    return x.to(torch.float32).contiguous()


def _row_lengths(lengths, B: int, N: int, what: str) -> np.ndarray:
    ln = np.full(B, N, np.int32) if lengths is None else np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int32)
    if ln.shape != (B,) or (ln < 0).any() or (ln > N).any():
        raise ValueError(f"{what}: one length per row, each in [0, {N}]")
    return ln


class KaldiFbank:
    def __init__(self, device="cuda:0", num_mel_bins: int = 80, frame_length: int = 400, hop_length: int = 160, fft_length: int = 512,
                 sampling_rate: int = 16000, preemphasis: float = 0.97, low_freq: float = 20.0):
        lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the HIP filter bank needs a ROCm GPU device; there is no CPU fallback")
        self.num_mel_bins, self.frame_length, self.hop_length = num_mel_bins, frame_length, hop_length
        c = _lib.FbankConfigC(frame_length, hop_length, fft_length, num_mel_bins, preemphasis)
        h = c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.idxtts_fbank_create(ctypes.byref(c), ctypes.byref(h)))
            self._h = h
            _lib.load_state_dict(h, {"window": features.povey_window(frame_length),
                                     "mel_filters": features.kaldi_mel_filters(num_mel_bins, fft_length, sampling_rate, low_freq).T})
        self._ws = _lib.StreamWorkspaces()

    def frames(self, n_samples: int) -> int:
        return 0 if n_samples < self.frame_length else 1 + (n_samples - self.frame_length) // self.hop_length

    def __call__(self, audio: torch.Tensor, n_samples=None, scale: float = 1.0, mode: str = "raw"):
        """audio: GPU [B, N], row b holds n_samples[b] samples (default N).  -> (features, frames per row): "raw" / "campplus"
        [B, max frames, bins], "w2vbert" [B, ceil(max frames / 2), 2 * bins]; zero at padded positions."""
        lib = _lib.load()
        if mode not in _MODES:
            raise ValueError(f"mode must be one of {sorted(_MODES)}")
        y = _device_rows(audio, "audio")
        B, N = y.shape
        ln = _row_lengths(n_samples, B, N, "n_samples")
        frames = [self.frames(int(n)) for n in ln]
        if B == 0 or min(frames) < 1:
            raise ValueError("audio shorter than one frame")
        if mode == "w2vbert" and min(frames) < 2:
            raise ValueError("the audio is shorter than two 25 ms frames")
        stack = 2 if mode == "w2vbert" else 1
        T_out = (max(frames) + stack - 1) // stack
        out = torch.empty(B, T_out, stack * self.num_mel_bins, device=y.device, dtype=torch.float32)
        with torch.cuda.device(y.device):
            ws = self._ws.get(int(lib.idxtts_fbank_workspace_bytes(self._h, c_void_p(ln.ctypes.data), B)), y.device)
            _lib.check(lib.idxtts_fbank_forward(self._h, _lib.ptr(y), N, c_void_p(ln.ctypes.data), B, float(scale), _MODES[mode], _lib.ptr(out),
                                                T_out, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
        return out, frames

    def seamless_m4t_features(self, audio: torch.Tensor, n_samples=None):
        """-> (input_features [B, T', 160] on the GPU, valid stacked frames per row): `features.seamless_m4t_features`, with the
        attention mask as lengths (an odd frame count leaves a last row of (frame | zeros) that is not counted)."""
        x, frames = self(audio, n_samples, scale=float(2 ** 15), mode="w2vbert")
        return x, [t // 2 for t in frames]

    def campplus_features(self, audio: torch.Tensor, n_samples=None):
        """-> ([B, max frames, 80] on the GPU: fbank minus its mean over the row's own frames, frames per row)."""
        return self(audio, n_samples, scale=1.0, mode="campplus")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().idxtts_ctx_destroy(self._h)
        except Exception:
            pass


class SincResampler:
    def __init__(self, device="cuda:0", lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the HIP resampler needs a ROCm GPU device; there is no CPU fallback")
        self.lowpass_filter_width, self.rolloff = lowpass_filter_width, rolloff
        self._tables = {}

    def _table(self, orig: int, new: int, device):
        """(transposed float32 table [2 * width + orig, new] on `device`, width) of the reduced rate pair, built once."""
        key = (orig, new, device.index)
        if key not in self._tables:
            from .audioio import sinc_resample_kernel
            kern, width = sinc_resample_kernel(orig, new, self.lowpass_filter_width, self.rolloff)
            self._tables[key] = (torch.from_numpy(np.ascontiguousarray(kern.T)).to(device), int(width))
        return self._tables[key]

    def __call__(self, x: torch.Tensor, lengths, orig_freq: int, new_freq: int, max_out: Optional[int] = None):
        """x: GPU [B, N], row b holds lengths[b] samples (default N).  -> (out [B, max output length], output length per row):
        row b's first ceil(new * lengths[b] / orig) samples are `audioio.sinc_resample(x[b, :lengths[b]], orig_freq, new_freq)`, the rest is 0.
        `max_out`: keep only the first max_out output samples of every row (the 15 s cut), reading no more input than they need."""
        lib = _lib.load()
        y = _device_rows(x, "x")
        B, N = y.shape
        ln = _row_lengths(lengths, B, N, "lengths")
        orig_freq, new_freq = int(orig_freq), int(new_freq)
        if orig_freq <= 0 or new_freq <= 0:
            raise ValueError("sample rates must be positive")
        if orig_freq == new_freq:
            out_len = [int(n) if max_out is None else min(int(n), int(max_out)) for n in ln]
            return (y if max_out is None else y[:, :max_out]), out_len
        g = math.gcd(orig_freq, new_freq)
        orig, new = orig_freq // g, new_freq // g
        kt, width = self._table(orig, new, y.device)
        out_len = [int(math.ceil(new * int(n) / orig)) for n in ln]
        if max_out is not None:
            # output o = f * new + p reads padded[f * orig .. f * orig + taps), i.e. samples below (f + 1) * orig + width
            keep = ((int(max_out) - 1) // new + 1) * orig + width
            ln = np.minimum(ln, keep).astype(np.int32) if max_out > 0 else np.zeros_like(ln)
            out_len = [min(t, int(max_out)) for t in out_len]
        ldo = max([int(math.ceil(new * int(n) / orig)) for n in ln] + [0]) if B else 0
        out = torch.empty(B, ldo, device=y.device, dtype=torch.float32)
        if B and ldo:
            with torch.cuda.device(y.device):
                _lib.check(lib.idxtts_resample_forward(_lib.ptr(kt), orig, new, width, _lib.ptr(y), N, c_void_p(ln.ctypes.data), B, _lib.ptr(out),
                                                       ldo, _lib.current_stream()))
        if max_out is not None:
            out = out[:, :max_out]
        return out, out_len
