"""The audio-side half of the reference's prompt block (infer_v2.py:618-660, 677-694) on the HIP path.

    enc = PromptEncoders(w2vbert_sd, codec_sd, campplus_sd, tts.s2mel)      # state dicts in the reference modules' own key layouts
    feats = enc.encode(PromptAudio(audio_16k, audio_22k))                   # -> PromptFeatures (spk_cond_emb, style, prompt_condition, ref_mel)
    tts.infer(feats, token_segments, None, return_audio=True)               # or tts.prompt_encoders = enc; tts.infer(PromptAudio(...), ...)

`encode()` takes one voice whose audio is already cut to 15 s and resampled to 16 kHz and 22.05 kHz (`PromptAudio`; `audioio.py` makes one
from a file on the host: librosa.load / torchaudio.transforms.Resample in the reference, infer_v2.py:628-631 -- neither library is in
this image, so the resampler is torchaudio's published algorithm restated and parity-unpinned).

    feats = enc.encode_batch([PromptAudio(...), RawAudio(samples, 48000), "speaker.wav"], [None, "emotion.wav", None])      # N voices
    conds = PromptConditioning.from_features_batch(tts.gpt, feats)          # -> cond= of synthesize_batch / BatchPipeline / ContinuousPipeline

`encode_batch()` takes several voices at once, each a `PromptAudio`, a `RawAudio` (samples at the file's own rate) or a wav path; raw audio
follows `audioio.load_and_cut_audio` (channel mean, file rate -> 22 050, cut to 15 s, -> 16 000; the emotion side straight to 16 000).
All speaker and emotion waveforms go through the front-end and the 17 w2v-bert layers as ONE ragged batch; codec, mel, CAMPPlus and the
length regulator run row by row on their B = 1 entries.  `PromptEncoders(..., frontend="gpu")` runs the resamples and both filter banks of
`encode_batch` in HIP kernels (frontend.py, csrc/fbank.hip) instead of numpy; the default, and all of `encode()`, is the host front-end.
Per step:
    extract_features (SeamlessM4TFeatureExtractor)   -> features.seamless_m4t_features        host numpy, as in the reference
                                                        (frontend="gpu": frontend.KaldiFbank  csrc/fbank.hip)
    get_emb (w2v-bert-2.0, hidden_states[17], stats) -> semantic.SemanticModel                 csrc/semantic.hip
    semantic_codec.quantize                          -> codec.SemanticCodec                    csrc/codec.hip
    mel_fn                                           -> audio.MelSpectrogram                   csrc/audio.hip
    kaldi.fbank - mean, campplus_model               -> features.kaldi_fbank, campplus.CAMPPlus  csrc/campplus.hip
    length_regulator(S_ref, ylens=[ref_mel frames])  -> S2Mel.length_regulator                 csrc/s2mel.hip
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import features
from .audio import MelSpectrogram
from .campplus import CAMPPlus
from .codec import SemanticCodec
from .frontend import KaldiFbank, SincResampler
from .config import CamPPlusConfig, RepCodecConfig, W2VBertConfig
from .semantic import SemanticModel


@dataclass
class PromptAudio:
    """One prompt, already cut (<= 15 s, infer_v2.py:628) and resampled: mono float waveforms in [-1, 1]."""
    audio_16k: np.ndarray
    audio_22k: Optional[np.ndarray] = None       # not needed for an emotion prompt (infer_v2.py:678-686 uses the 16 kHz audio only)


@dataclass
class RawAudio:
    """One prompt as its file holds it: float samples in [-1, 1], [channels, n] or [n], at the file's own rate (`audioio.read_wav`)."""
    samples: np.ndarray
    sample_rate: int


MAX_PROMPT_SECONDS = 15          # infer_v2.py:628
FRONTENDS = ("host", "gpu")


def check_frontend(name) -> str:
    if name not in FRONTENDS:
        raise ValueError(f"frontend must be one of {FRONTENDS}, not {name!r}")
    return name


def as_prompt_input(p):
    """A prompt as `encode_batch` takes it -> PromptAudio or RawAudio (a path is read with `audioio.read_wav`)."""
    if isinstance(p, (PromptAudio, RawAudio)):
        return p
    if isinstance(p, str):
        from .audioio import read_wav
        return RawAudio(*read_wav(p))
    if isinstance(p, (tuple, list)) and len(p) == 2 and np.ndim(p[1]) == 0:
        return RawAudio(np.asarray(p[0], np.float32), int(p[1]))
    raise TypeError(f"a prompt is a PromptAudio, a RawAudio, (samples, sample_rate) or a wav path, not {type(p).__name__}")


def _mono(raw: RawAudio) -> np.ndarray:
    x = np.asarray(raw.samples, np.float32)
    if x.ndim == 1:
        return x
    if x.ndim != 2:
        raise ValueError("RawAudio.samples must be [n] or [channels, n]")
    return x.mean(axis=0, dtype=np.float32) if x.shape[0] > 1 else x[0]      # librosa.load's to_mono


class PromptEncoders:
    def __init__(self, w2vbert_sd, codec_sd, campplus_sd, s2mel, device="cuda:0", w2vbert_cfg: W2VBertConfig = W2VBertConfig(),
                 codec_cfg: RepCodecConfig = RepCodecConfig(), campplus_cfg: CamPPlusConfig = CamPPlusConfig(), semantic_mean=None,
                 semantic_std=None, mel_kwargs: Optional[dict] = None, frontend: str = "host"):
        self.frontend = check_frontend(frontend)
        self.device = torch.device(device)
        self.semantic = SemanticModel(w2vbert_sd, w2vbert_cfg, device=self.device, mean=semantic_mean, std=semantic_std)
        self.codec = SemanticCodec(codec_sd, codec_cfg, device=self.device)
        self.campplus = CAMPPlus(campplus_sd, campplus_cfg, device=self.device)
        self.mel = MelSpectrogram(device=self.device, **(mel_kwargs or {}))
        self.s2mel = s2mel
        self.fbank = self.resampler = None      # the device front-end's mirrors, built with frontend="gpu"
        if self.frontend == "gpu":
            self.fbank = KaldiFbank(device=self.device)
            self.resampler = SincResampler(device=self.device)

    def with_frontend(self, frontend: str) -> "PromptEncoders":
        """These encoders (the same contexts and weights, nothing copied) behind the other front-end of `encode_batch`."""
        import copy
        check_frontend(frontend)
        other = copy.copy(self)
        other.frontend = frontend
        if frontend == "gpu" and other.fbank is None:
            other.fbank = KaldiFbank(device=self.device)
            other.resampler = SincResampler(device=self.device)
        return other

    def get_emb(self, audio_16k) -> torch.Tensor:
        """extract_features + get_emb (infer_v2.py:633-638, 680-686) -> [1, T, 1024] (valid frames only)."""
        f = features.seamless_m4t_features(np.asarray(audio_16k, np.float32))
        emb = self.semantic(torch.from_numpy(f["input_features"]), torch.from_numpy(f["attention_mask"]))
        return emb[:, : int(f["attention_mask"].sum())]

    def get_emb_batch(self, audios_16k) -> list:
        """get_emb of several prompts as ONE ragged batch (right-padded, attention-masked): the speaker and the emotion prompt of a
        request go through the 17 w2v-bert layers together -- twice the GEMM rows per launch (a 15 s prompt is 750 frames: 6 row tiles
        of 128 under-fill 256 CUs), half the launches.  Each row equals its own B = 1 call (rows and valid frames are independent in
        every kernel; tests/test_prompt_gpu.py)."""
        fs = [features.seamless_m4t_features(np.asarray(a, np.float32)) for a in audios_16k]
        lens = [int(f["attention_mask"].sum()) for f in fs]
        T = max(f["input_features"].shape[1] for f in fs)
        x = np.zeros((len(fs), T, fs[0]["input_features"].shape[2]), np.float32)
        m = np.zeros((len(fs), T), np.int64)
        for i, f in enumerate(fs):
            t = f["input_features"].shape[1]
            x[i, :t] = f["input_features"][0]
            m[i, :lens[i]] = 1
        emb = self.semantic(torch.from_numpy(x), torch.from_numpy(m))
        return [emb[i:i + 1, :lens[i]].contiguous() for i in range(len(fs))]

    def encode(self, prompt: PromptAudio, emo_prompt: Optional[PromptAudio] = None):
        from .infer_v2 import PromptFeatures
        if prompt.audio_22k is None:
            raise ValueError("the speaker prompt needs its 22.05 kHz waveform (ref_mel)")
        a16 = np.asarray(prompt.audio_16k, np.float32).reshape(-1)
        emo = None
        if emo_prompt is None:
            spk_cond_emb = self.get_emb(a16)
        else:
            spk_cond_emb, emo = self.get_emb_batch([a16, np.asarray(emo_prompt.audio_16k, np.float32).reshape(-1)])
        _, S_ref = self.codec.quantize(spk_cond_emb)                                          # infer_v2.py:637
        ref_mel = self.mel(torch.from_numpy(np.asarray(prompt.audio_22k, np.float32).reshape(1, -1)).to(self.device))     # 640
        feat = features.kaldi_fbank(a16)                                                      # 642-645 (dither 0, 80 bins)
        feat = feat - feat.mean(axis=0, keepdims=True)                                        # 646
        style = self.campplus(torch.from_numpy(feat[None]))                                   # 647
        prompt_condition = self.s2mel.length_regulator(S_ref, ylens=torch.LongTensor([ref_mel.size(2)]), n_quantizers=3, f0=None)[0]   # 649-652
        return PromptFeatures(spk_cond_emb, style, prompt_condition, ref_mel, emo)

    # ---- several voices at once -------------------------------------------------------------------------------------------------
    def _host_audio(self, p, emotion: bool) -> PromptAudio:
        """`audioio.load_prompt_audio` on samples that are already read: channel mean, -> 22 050, cut, -> 16 000 (emotion: -> 16 000, cut)."""
        if isinstance(p, PromptAudio):
            return p
        from .audioio import sinc_resample
        mono = _mono(p)
        if emotion:
            return PromptAudio(sinc_resample(mono, p.sample_rate, 16000)[: MAX_PROMPT_SECONDS * 16000])
        a22 = sinc_resample(mono, p.sample_rate, 22050)[: MAX_PROMPT_SECONDS * 22050]
        return PromptAudio(sinc_resample(a22, 22050, 16000), a22)

    def _device_audio(self, items, emotion: bool):
        """items: PromptAudio / RawAudio -> per item (audio_16k, audio_22k or None), 1-D GPU tensors.  Raw audio of one file rate is
        resampled as one ragged batch per step."""
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))).to(self.device)
        out = [None] * len(items)
        by_rate = {}
        for i, p in enumerate(items):
            if isinstance(p, PromptAudio):
                out[i] = (up(p.audio_16k), None if emotion or p.audio_22k is None else up(p.audio_22k))
            else:
                by_rate.setdefault(int(p.sample_rate), []).append(i)
        for sr, idx in by_rate.items():
            monos = [_mono(items[i]) for i in idx]
            lens = [m.size for m in monos]
            x = np.zeros((len(idx), max(lens)), np.float32)
            for r, m in enumerate(monos):
                x[r, : m.size] = m
            x = torch.from_numpy(x).to(self.device)
            if emotion:
                a16, n16 = self.resampler(x, lens, sr, 16000, max_out=MAX_PROMPT_SECONDS * 16000)
                a22 = n22 = None
            else:
                a22, n22 = self.resampler(x, lens, sr, 22050, max_out=MAX_PROMPT_SECONDS * 22050)
                a16, n16 = self.resampler(a22, n22, 22050, 16000)
            for r, i in enumerate(idx):
                out[i] = (a16[r, : n16[r]], None if emotion else a22[r, : n22[r]])
        return out

    def encode_batch(self, prompts: Sequence, emo_prompts: Optional[Sequence] = None) -> list:
        """`encode()` of several voices: prompts[i] (and emo_prompts[i], or None) -> a list of PromptFeatures.  Each prompt is a
        PromptAudio, a RawAudio / (samples, sample_rate), or a wav path."""
        return self._encode_batch(prompts, emo_prompts)[0]

    def _encode_batch(self, prompts, emo_prompts):
        """-> (the list of PromptFeatures, what the front-end handed to the encoders: input_features, feature_lens, campplus_feats,
        campplus_frames, audio_16k, audio_22k -- the tests compare each stage on handed-over inputs)."""
        from .infer_v2 import PromptFeatures
        spk = [as_prompt_input(p) for p in prompts]
        n = len(spk)
        if n == 0:
            raise ValueError("encode_batch needs at least one prompt")
        emo_prompts = [None] * n if emo_prompts is None else list(emo_prompts)
        if len(emo_prompts) != n:
            raise ValueError(f"{len(emo_prompts)} emotion prompts for {n} speaker prompts: pass None, or one entry (or None) per prompt")
        emo_of = [i for i, e in enumerate(emo_prompts) if e is not None]      # rows n.. of the batch
        emo = [as_prompt_input(emo_prompts[i]) for i in emo_of]
        for p in spk:
            if isinstance(p, PromptAudio) and p.audio_22k is None:
                raise ValueError("the speaker prompt needs its 22.05 kHz waveform (ref_mel)")
        if self.frontend == "gpu":
            wav = self._device_audio(spk, False) + self._device_audio(emo, True)
            n16 = [int(a.numel()) for a, _ in wav]
            a16 = torch.zeros(len(wav), max(n16), device=self.device, dtype=torch.float32)
            for r, (a, _) in enumerate(wav):
                a16[r, : n16[r]] = a
            x, lens = self.fbank.seamless_m4t_features(a16, n16)
            cp, cp_frames = self.fbank.campplus_features(a16[:n], n16[:n])
            a22 = [w[1].reshape(1, -1) for w in wav[:n]]
            cp_rows = [cp[i:i + 1, : cp_frames[i]] for i in range(n)]
            mid_audio = [w[0] for w in wav]
        else:
            wav = [self._host_audio(p, False) for p in spk] + [self._host_audio(p, True) for p in emo]
            w16 = [np.asarray(w.audio_16k, np.float32).reshape(-1) for w in wav]
            fs = [features.seamless_m4t_features(a) for a in w16]
            lens = [int(f["attention_mask"].sum()) for f in fs]
            T = max(f["input_features"].shape[1] for f in fs)
            xh = np.zeros((len(fs), T, fs[0]["input_features"].shape[2]), np.float32)
            for i, f in enumerate(fs):
                xh[i, : f["input_features"].shape[1]] = f["input_features"][0]
            x = torch.from_numpy(xh).to(self.device)
            cp_rows = []
            for a in w16[:n]:
                feat = features.kaldi_fbank(a)                                                # infer_v2.py:642-645
                cp_rows.append(torch.from_numpy((feat - feat.mean(axis=0, keepdims=True))[None]).to(self.device))      # 646
            cp_frames = [int(c.shape[1]) for c in cp_rows]
            a22 = [torch.from_numpy(np.asarray(w.audio_22k, np.float32).reshape(1, -1)).to(self.device) for w in wav[:n]]
            mid_audio = w16
        mask = (torch.arange(x.shape[1])[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)
        emb = self.semantic(x, mask)                                                          # all rows, one ragged batch
        rows = [emb[i:i + 1, : lens[i]].contiguous() for i in range(len(lens))]
        out = []
        for i in range(n):                                                                    # B = 1 entries, no synchronisation between rows
            _, S_ref = self.codec.quantize(rows[i])                                           # infer_v2.py:637
            ref_mel = self.mel(a22[i])                                                        # 640
            style = self.campplus(cp_rows[i])                                                 # 647
            prompt_condition = self.s2mel.length_regulator(S_ref, ylens=torch.LongTensor([ref_mel.size(2)]), n_quantizers=3, f0=None)[0]
            out.append(PromptFeatures(rows[i], style, prompt_condition, ref_mel, rows[n + emo_of.index(i)] if i in emo_of else None))
        return out, {"input_features": x, "feature_lens": lens, "campplus_feats": cp_rows, "campplus_frames": cp_frames,
                     "audio_16k": mid_audio, "audio_22k": a22}
