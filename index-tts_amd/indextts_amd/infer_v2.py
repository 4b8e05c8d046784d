"""Host-side mirror of `indextts.infer_v2.IndexTTS2` for the hot path (reference infer_v2.py:69-937).

Scope: the three hot stages -- GPT decode + latent pass, s2mel, BigVGAN --, the GPT's own prompt conditioning
(conformer + perceiver + emotion vector, model_v2.py:627-671, 897-910; hoisted out of the segment loop), the audio-side prompt
encoders (w2v-bert, RepCodec, CAMPPlus, mel; infer_v2.py:618-696 -> indextts_amd/prompt.py), the text front-end (tokenizer.py,
segmenter.py) and the segment loop that sequences them (infer_v2.py:732-881), with the reference's return contract (905-937) and
generation defaults (714-722: beam-sample, num_beams=3).  `IndexTTS2(cfg_path, model_dir)` assembles all of it from a
checkpoint directory as the reference's constructor does; `infer()` takes a WAV path + a string, or any of the intermediate
forms (`PromptAudio`, `PromptFeatures`, `PromptConditioning`; token-id segments).
"""
from __future__ import annotations

import functools
import os
import time
import warnings
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, synth
from .config import PipelineConfig
from .gpt import UnifiedVoice
from .s2mel import S2Mel
from .vocoder import BigVGAN


@dataclass
class InferenceResult:                       # infer_v2.py:58-66
    sampling_rate: int
    audio: object
    duration_sec: float
    saved_path: Optional[str]
    rtf: Optional[float]


@dataclass
class PromptFeatures:
    """What the reference's audio-side prompt encoders leave behind per prompt (infer_v2.py:637-658, 691-694): the inputs of the
    GPT's conditioning encoders plus the s2mel conditioning."""
    spk_cond_emb: torch.Tensor        # [1, T50, 1024]  w2v-bert layer-17 features of the speaker prompt     infer_v2.py:637
    style: torch.Tensor               # [1, 192]        CAMPPlus                                              infer_v2.py:647
    prompt_condition: torch.Tensor    # [1, Tp, 512]    length_regulator(S_ref)                               infer_v2.py:649
    ref_mel: torch.Tensor             # [1, 80, Tp]     mel_fn(prompt audio)                                  infer_v2.py:640
    emo_cond_emb: Optional[torch.Tensor] = None       # [1, T50', 1024] features of the emotion prompt (default: the speaker's, 583-584)

    @staticmethod
    def synthetic(cfg: PipelineConfig, prompt_frames: int = 689, feat_frames: int = 400, tag: str = "prompt", emo_frames: int = 0) -> "PromptFeatures":
        """Seeded stand-in for an 8 s prompt (spk_cond_emb [1,400,1024], Tp = 689)."""
        t = lambda n, shape, s, o=0.0: torch.from_numpy(synth.uniform(f"{tag}/{n}", shape, s, o))
        return PromptFeatures(t("spk_cond_emb", (1, feat_frames, cfg.gpt.cond_module.input_size), 1.0), t("style", (1, cfg.s2mel.style_dim), 1.0),
                              t("prompt_condition", (1, prompt_frames, cfg.s2mel.content_dim), 1.0),
                              t("ref_mel", (1, cfg.s2mel.in_channels, prompt_frames), 2.6, -4.0),
                              t("emo_cond_emb", (1, emo_frames, cfg.gpt.cond_module.input_size), 1.0) if emo_frames else None)


@dataclass
class PromptConditioning:
    """What the reference caches per prompt (infer_v2.py:654-658, 693-694) after its encoders have run."""
    spk_cond_latent: torch.Tensor     # [1, 32, d]   get_conditioning(spk_cond_emb)           model_v2.py:819
    emo_vec: torch.Tensor             # [1, d]       merge_emovec(...)                        model_v2.py:904-910
    style: torch.Tensor               # [1, 192]     CAMPPlus                                 infer_v2.py:647
    prompt_condition: torch.Tensor    # [1, Tp, 512] length_regulator(S_ref)                  infer_v2.py:649
    ref_mel: torch.Tensor             # [1, 80, Tp]  mel_fn(prompt audio)                     infer_v2.py:640

    FIELDS = ("spk_cond_latent", "emo_vec", "style", "prompt_condition", "ref_mel")

    @staticmethod
    def synthetic(cfg: PipelineConfig, prompt_frames: int = 689, tag: str = "prompt") -> "PromptConditioning":
        """Seeded stand-in for an 8 s prompt (Tp = 689)."""
        d = cfg.gpt.model_dim
        t = lambda n, shape, s, o=0.0: torch.from_numpy(synth.uniform(f"{tag}/{n}", shape, s, o))
        return PromptConditioning(
            t("latent", (1, cfg.gpt.cond_latents, d), 0.5), t("emo", (1, d), 0.3), t("style", (1, cfg.s2mel.style_dim), 1.0),
            t("prompt_condition", (1, prompt_frames, cfg.s2mel.content_dim), 1.0),
            t("ref_mel", (1, cfg.s2mel.in_channels, prompt_frames), 2.6, -4.0))

    @staticmethod
    def from_features(gpt: UnifiedVoice, feats: "PromptFeatures", emo_alpha: float = 1.0, emo_mix=None) -> "PromptConditioning":
        """The per-prompt half of the reference's segment loop, once per prompt instead of once per segment:
        `merge_emovec(spk_cond_emb, emo_cond_emb, ..., alpha=emo_alpha)` (infer_v2.py:748-754) and the `get_conditioning` call
        inside `inference_speech` (model_v2.py:819), on the HIP conditioning encoders.  The "lengths" are the reference's:
        `shape[-1]` of the [1,T,1024] tensors (infer_v2.py:751-752), i.e. no padding."""
        dev = gpt.device
        spk = feats.spk_cond_emb.to(dev, torch.float32)
        emo = spk if feats.emo_cond_emb is None else feats.emo_cond_emb.to(dev, torch.float32)
        ln_s, ln_e = torch.tensor([spk.shape[-1]]), torch.tensor([emo.shape[-1]])
        emovec = gpt.merge_emovec(spk, emo, ln_s, ln_e, alpha=emo_alpha)
        if emo_mix is not None:
            emovec = PromptConditioning.mix_emovec(emovec, emo_mix)
        latent = gpt.get_conditioning(spk.transpose(1, 2), ln_s)
        return PromptConditioning(latent, emovec, feats.style, feats.prompt_condition, feats.ref_mel)

    @staticmethod
    def from_features_batch(gpt: UnifiedVoice, feats_list, emo_alpha: float = 1.0) -> list:
        """`from_features` of several prompts (PromptEncoders.encode_batch) with `get_conditioning` and `merge_emovec` run ONCE over the
        ragged batch: the features are right-padded and the conditioning encoders take each row's own frame count as its extent
        (idxtts_cond_forward_rows: every row computes what its own unpadded call computes; the reference's masks alone do not give
        that) beside the "length" `from_features` passes, the reference's `shape[-1]`.
        -> one PromptConditioning per prompt, as `cond=` of synthesize_batch / BatchPipeline / ContinuousPipeline takes them."""
        feats_list = list(feats_list)
        if not feats_list:
            raise ValueError("from_features_batch needs at least one PromptFeatures")
        for f in feats_list:
            if f.spk_cond_emb.dim() != 3 or int(f.spk_cond_emb.shape[0]) != 1:
                raise ValueError("every PromptFeatures holds one prompt: spk_cond_emb [1, T, features]")
        dev = gpt.device

        def pad(rows):
            ln = [int(r.shape[1]) for r in rows]
            x = torch.zeros(len(rows), max(ln), rows[0].shape[2], device=dev, dtype=torch.float32)
            for i, r in enumerate(rows):
                x[i, : ln[i]] = r[0].to(dev, torch.float32)
            return x, torch.tensor([int(rows[0].shape[2])] * len(rows)), torch.tensor(ln)

        spk, ln_s, ex_s = pad([f.spk_cond_emb for f in feats_list])
        emo, ln_e, ex_e = pad([f.spk_cond_emb if f.emo_cond_emb is None else f.emo_cond_emb for f in feats_list])
        emovec = gpt.merge_emovec(spk, emo, ln_s, ln_e, alpha=emo_alpha, extents=ex_s, emo_extents=ex_e)
        latent = gpt.get_conditioning(spk.transpose(1, 2), ln_s, extents=ex_s)
        return [PromptConditioning(latent[i:i + 1], emovec[i:i + 1], f.style, f.prompt_condition, f.ref_mel) for i, f in enumerate(feats_list)]

    @staticmethod
    def mix_emovec(emovec: torch.Tensor, emo_mix) -> torch.Tensor:
        """The prompt's emotion vector with an `emo_vector` mix laid over it; emo_mix = (emovec_mat [1,d], weight_vector): infer_v2.py:756-757."""
        emovec_mat, weight_vector = emo_mix
        dev = emovec.device
        return emovec_mat.to(dev, torch.float32) + (1 - torch.sum(weight_vector.to(dev, torch.float32))) * emovec

    def to(self, device) -> "PromptConditioning":
        return PromptConditioning(*[getattr(self, f).to(device, torch.float32).contiguous() for f in self.FIELDS])

    # one flat buffer for the RCCL broadcast ("one packed buffer")
    def pack(self) -> torch.Tensor:
        return torch.cat([getattr(self, f).reshape(-1) for f in self.FIELDS])

    def shapes(self):
        return [tuple(getattr(self, f).shape) for f in self.FIELDS]

    @staticmethod
    def unpack(flat: torch.Tensor, shapes) -> "PromptConditioning":
        out, off = [], 0
        for shp in shapes:
            n = int(np.prod(shp))
            out.append(flat[off:off + n].reshape(shp))
            off += n
        return PromptConditioning(*out)


def rows_conditioning(cond, B: int, device):
    """`cond` as the stages take it: ONE PromptConditioning for all B rows, or a list / tuple of B of them, one per row (rows of one
    speaker pass the same object).  Returns the single conditioning on `device` when every row shares one prompt (the single-prompt
    path, unchanged), else a list of B device conditionings in which rows that passed the same object share one converted copy."""
    if not isinstance(cond, (list, tuple)):
        return cond.to(device)
    if len(cond) != B:
        raise ValueError(f"{len(cond)} prompt conditionings for {B} rows: pass one, or one per row")
    if any(c is not cond[0] for c in cond):
        if any(int(c.spk_cond_latent.shape[0]) != 1 or int(c.emo_vec.shape[0]) != 1 for c in cond):
            raise ValueError("a per-row PromptConditioning holds one prompt (batch dimension 1)")
    else:
        return cond[0].to(device)
    conv = {}
    for c in cond:
        if id(c) not in conv:
            conv[id(c)] = c.to(device)
    return [conv[id(c)] for c in cond]


class IndexTTS2:
    """Drop-in for the hot path of `indextts.infer_v2.IndexTTS2`.

    Construct from a checkpoint directory with the reference's constructor signature (infer_v2.py:69-72): everything that
    constructor loads (infer_v2.py:138-289) is assembled -- gpt / s2mel / BigVGAN, the semantic model + its statistics, the
    semantic codec, CAMPPlus, the emotion banks, the tokenizer -- so `infer("voice.wav", "text", "out.wav")` works as it does there
    (files are looked up where the reference looks, hub cache included; nothing is downloaded).  Or from state dicts
    (reference key layout) with `from_state_dicts` (+ `attach_prompt_models`).
    """

    def __init__(self, cfg_path="checkpoints/config.yaml", model_dir="checkpoints", use_fp16=False, device=None,
                 use_cuda_kernel=None, use_deepspeed=False, use_accel=False, use_torch_compile=False, gpt_weight_format=None,
                 segment_batch: int = 16, gpt_kv_format=None, acoustic_bf16=None, batch_invariant: bool = False):
        # acoustic_bf16: see from_state_dicts (process-wide).  batch_invariant: see from_state_dicts (this object's GPT only).
        # use_fp16 (reference: gpt.half() + fp16 autocast, infer_v2.py:109, 145-146) maps to bf16 STORAGE of the GPT weights:
        # the arithmetic of the HIP path stays fp32.  gpt_weight_format ("f32" | "bf16" | "fp8") overrides it.
        if gpt_weight_format is None:
            gpt_weight_format = "bf16" if use_fp16 else "f32"
        need = [os.path.join(model_dir, f) for f in ("gpt.pth", "s2mel.pth")]
        missing = [p for p in need if not os.path.exists(p)]
        if missing:
            raise FileNotFoundError(f"IndexTTS-2 checkpoints not found ({missing}); use IndexTTS2.from_state_dicts(...)")
        from .checkpoint import config_from_yaml, load_reference_checkpoints
        cfg, raw = config_from_yaml(cfg_path, model_dir) if os.path.exists(cfg_path) else (PipelineConfig(), None)
        gpt_sd, s2mel_sd, voc_sd = load_reference_checkpoints(model_dir, raw)
        self._init(cfg, gpt_sd, s2mel_sd, voc_sd, device, gpt_weight_format, segment_batch=segment_batch, gpt_kv_format=gpt_kv_format,
                   acoustic_bf16=acoustic_bf16, batch_invariant=batch_invariant)
        # the rest of the reference's constructor (infer_v2.py:187-289): semantic model + statistics, semantic codec, CAMPPlus,
        # emotion banks, tokenizer
        from .checkpoint import load_prompt_checkpoints, reference_text_normalizer
        self.model_dir = model_dir
        self.attach_prompt_models(load_prompt_checkpoints(model_dir, raw), normalizer=reference_text_normalizer())
        if raw and raw.get("qwen_emo_path"):      # loaded on first use, as the reference does (infer_v2.py:118-128, 322-328)
            self._qwen_emo_path = os.path.join(model_dir, str(raw["qwen_emo_path"]))

    def attach_prompt_models(self, ck: dict, normalizer=None) -> None:
        """ck: checkpoint.load_prompt_checkpoints()'s dict (state dicts in the reference modules' own key layouts, statistics,
        emotion banks, bpe path) -> self.prompt_encoders, the emotion banks, self.tokenizer."""
        from .prompt import PromptEncoders
        from .tokenizer import TextTokenizer
        self.prompt_encoders = PromptEncoders(ck["w2vbert"], ck["codec"], ck["campplus"], self.s2mel, device=self.device,
                                              w2vbert_cfg=ck["w2vbert_cfg"], codec_cfg=ck["codec_cfg"], campplus_cfg=ck["campplus_cfg"],
                                              semantic_mean=ck["semantic_mean"], semantic_std=ck["semantic_std"], mel_kwargs=ck.get("mel_kwargs"))
        self.set_emotion_matrices(ck["emo_matrix"], ck["spk_matrix"], ck["emo_num"])
        self.normalizer = normalizer
        self.tokenizer = TextTokenizer(ck["bpe_path"], normalizer)
        self.bpe_path = ck["bpe_path"]

    @classmethod
    def from_state_dicts(cls, cfg: PipelineConfig, gpt_sd, s2mel_sd, bigvgan_sd, device=None, gpt_weight_format="f32",
                         keep_effective_gpt=False, segment_batch: int = 16, gpt_kv_format=None, acoustic_bf16=None,
                         batch_invariant: bool = False) -> "IndexTTS2":
        """gpt_weight_format: "f32" | "bf16" | "fp8" storage of the GPT linear weights, gpt_kv_format: "f32" | "bf16" | "fp8" storage of its KV
        cache (default: fp32 with fp32 weights, bf16 with compact weights; fp8 only when asked for) (UnifiedVoice); keep_effective_gpt keeps
        `self.gpt.effective_state_dict` (the rounded model, reference keys) for parity checks; segment_batch: segments of one
        infer() call synthesised together (1 = the reference's loop as written); acoustic_bf16: None leaves the library's switch as
        it is, True / False sets it (_lib.set_acoustic_bf16): s2mel and the vocoder on one bf16 MFMA per product instead of the split
        form's three -- about 1.45 x faster, mel L1 7.7e-3 instead of 1.3e-5 from the exact mode (profiles/README.md "Acoustic bf16"), the GPT and the codes it
        chooses untouched.  The switch is PROCESS-WIDE: it holds for every IndexTTS2 of the process, not for this object.
        batch_invariant: this object's GPT in the batch-invariant mode (UnifiedVoice.set_batch_invariant): an utterance's codes do not
        depend on the batch, session size, lane or pipeline it is decoded in (the acoustic stage is outside that contract)."""
        self = cls.__new__(cls)
        self._init(cfg, gpt_sd, s2mel_sd, bigvgan_sd, device, gpt_weight_format, keep_effective_gpt, segment_batch, gpt_kv_format, acoustic_bf16,
                   batch_invariant)
        return self

    def _init(self, cfg, gpt_sd, s2mel_sd, bigvgan_sd, device, gpt_weight_format="f32", keep_effective_gpt=False, segment_batch=16,
              gpt_kv_format=None, acoustic_bf16=None, batch_invariant=False):
        if acoustic_bf16 is not None:
            _lib.set_acoustic_bf16(bool(acoustic_bf16))
        if device is None:
            device = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("IndexTTS2 (HIP path) needs an MI355X device; there is no CPU fallback")
        self.cfg = cfg
        self.gpt = UnifiedVoice(gpt_sd, cfg.gpt, device=self.device, weight_format=gpt_weight_format, keep_effective=keep_effective_gpt,
                                kv_format=gpt_kv_format, batch_invariant=batch_invariant)
        self.s2mel = S2Mel(s2mel_sd, cfg.s2mel, device=self.device)
        self.bigvgan = BigVGAN(bigvgan_sd, cfg.bigvgan)
        self.stop_mel_token = cfg.gpt.stop_mel_token
        self.model_version = 2.0
        self.gr_progress = None
        self._diffusion_steps = int(os.environ.get("TARS_DIFFUSION_STEPS", cfg.diffusion_steps))   # infer_v2.py:125
        self._cfg_rate = float(os.environ.get("TARS_CFG_RATE", cfg.cfg_rate))                      # infer_v2.py:126
        self.last_stage_times = {}
        self.segment_batch = int(segment_batch)      # segments of one infer() call synthesised together

    @property
    def qwen_emo(self):
        """The emotion-from-text classifier (qwen_emo.QwenEmotion, or anything with `inference(text) -> dict` of the eight scores in
        order): set it, or -- built from a checkpoint directory whose config names `qwen_emo_path` -- it loads on first use."""
        if getattr(self, "_qwen_emo", None) is None:
            path = getattr(self, "_qwen_emo_path", None)
            if path is None:
                raise NotImplementedError("emo_text routing (the Qwen emotion classifier, infer_v2.py:590-598) needs a classifier: set "
                                          "tts.qwen_emo = QwenEmotion(...), or pass its result as emo_vector")
            from .checkpoint import qwen_emotion_from_pretrained
            self._qwen_emo = qwen_emotion_from_pretrained(path, device=self.device)
        return self._qwen_emo

    @qwen_emo.setter
    def qwen_emo(self, value):
        self._qwen_emo = value

    def normalize_emo_vec(self, emo_vector, apply_bias=True):
        """infer_v2.py:524-538: de-emphasise the emotions that tend to sound odd, then cap the sum at 0.8."""
        from .qwen_emo import normalize_emo_vec
        return normalize_emo_vec(emo_vector, apply_bias)

    # ------------------------------------------------------------------------------------------
    def synthesize_batch(self, text_tokens: torch.Tensor, cond: PromptConditioning, max_mel_tokens: int = 1500,
                         repetition_penalty: float = 10.0, noise: Optional[torch.Tensor] = None, sync_timers: bool = False,
                         return_intermediates: bool = False, sampling: Optional[dict] = None, per_row_noise: bool = False,
                         noise_seeds=None, diffusion_steps=None, cfg_rate=None):
        """One batch of single-segment utterances: the body of the reference's segment loop (infer_v2.py:732-881) for B rows at once.
        text_tokens [B, L] (right-padded with stop_text_token).  cond: one PromptConditioning shared by every row, or a list of B
        of them, one per row (several speakers in one batch; see rows_conditioning).
        Returns a list of B waveforms, float32 [1, n_b] in int16 range (infer_v2.py:866).
        sampling: None = greedy; else the num_beams=1 sampling kwargs of UnifiedVoice.inference_speech
        (do_sample, temperature, top_k, top_p, sampler, exp_noise / generator).
        per_row_noise: draw the CFM noise row by row, `randn([1, 80, Tp + Tg_b])` in row order -- the draws the reference's
        sequential segment loop makes (flow_matching.py:62 once per segment) -- instead of one [B, 80, T] draw.
        noise_seeds: one int per row instead of `noise` (see acoustic_stage).
        diffusion_steps / cfg_rate: the CFM solver's Euler steps and guidance rate, one value or one per row (see acoustic_stage).
        = acoustic_stage(gpt_stage(...)): the two halves are separate entry points so that a serving loop can overlap the
        (latency-bound) decode of one batch with the (MFMA-bound) s2mel + vocoder of the previous one on another stream."""
        st = self.gpt_stage(text_tokens, cond, max_mel_tokens=max_mel_tokens, repetition_penalty=repetition_penalty,
                            sampling=sampling, sync_timers=sync_timers)
        return self.acoustic_stage(st, noise=noise, per_row_noise=per_row_noise, sync_timers=sync_timers,
                                   return_intermediates=return_intermediates, noise_seeds=noise_seeds, diffusion_steps=diffusion_steps,
                                   cfg_rate=cfg_rate)

    def _tick(self, sync: bool) -> float:
        if sync:
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    @staticmethod
    def _row_latents(c, B: int):
        """The GPT's per-row conditioning latents and emotion vectors of rows_conditioning's result."""
        if isinstance(c, list):      # one prompt per row: the GPT takes per-row conditioning latents and emotion vectors as they are
            return torch.cat([x.spk_cond_latent for x in c]), torch.cat([x.emo_vec for x in c])
        lat = c.spk_cond_latent.expand(B, -1, -1) if c.spk_cond_latent.shape[0] == 1 else c.spk_cond_latent
        emo = c.emo_vec.expand(B, -1) if c.emo_vec.shape[0] == 1 else c.emo_vec
        return lat, emo

    def ranked_takes(self, text_tokens: torch.Tensor, cond, takes: int, max_mel_tokens: int = 1500, repetition_penalty: float = 10.0,
                     sampling: Optional[dict] = None, length_penalty: float = 1.0):
        """`takes` sampled takes of every row, decoded with one prefill per row (generate(num_return_sequences=takes,
        return_logprobs=True)), and their ranking.  Returns (codes [B * takes, n] on the device, row i * takes + j take j of row i,
        stop-padded; ranking): ranking[i] lists all the takes of row i best first as (take_index, score, stopped, n_codes) --
        serving.rank_request: a take whose last code is the stop token ranks above every take that ran into max_mel_tokens, then the
        higher score (gpt.sequence_scores of the codes' log-probabilities), then the lower index.  sampling: gpt_stage's dict, with
        do_sample true and num_beams 1 (ValueError otherwise)."""
        from .serving import rank_request
        gen = dict(sampling or {})
        if not gen.get("do_sample") or int(gen.pop("num_beams", None) or 1) != 1:
            raise ValueError("ranked takes need do_sample=True and num_beams=1: greedy takes are all the same, and a beam search returns "
                             "its scorer's n best")
        gen.pop("length_penalty", None)
        B = text_tokens.shape[0]
        lat, emo = self._row_latents(rows_conditioning(cond, B, self.device), B)
        codes, _, lp = self.gpt.inference_speech(lat, text_tokens, emo_vec=emo, max_generate_length=max_mel_tokens,
                                                 repetition_penalty=repetition_penalty, num_return_sequences=int(takes),
                                                 return_logprobs=True, num_beams=1, **gen)
        hc, hl = codes.cpu(), lp.cpu()
        rows, lps = [], []
        for r in range(hc.shape[0]):
            hits = (hc[r] == self.stop_mel_token).nonzero()
            n = int(hits[0]) + 1 if len(hits) else int(hc.shape[1])
            rows.append(hc[r, :n])
            lps.append(hl[r, :n])
        return codes, rank_request(rows, lps, int(takes), self.stop_mel_token, length_penalty)

    def score_takes(self, text_tokens: torch.Tensor, cond, codes, length_penalty: float = 1.0):
        """Ranks GIVEN takes of one text and one conditioning: codes is a list of 1-D code sequences (each up to and including its stop
        token, or cut at its cap), from any source -- an unscored session, another process, an exact-mode or fp8-KV context.  The prompt
        is built as gpt_stage builds it; all takes are scored in one call of UnifiedVoice.score_codes (one prefill, layout "resume":
        the values a scored run would have recorded).  Returns (logprobs: one fp32 CPU row per take, ranking): ranking lists the takes
        best first as (take_index, score, stopped, n_codes), serving.rank_request's format for one utterance."""
        from .serving import rank_request
        text_tokens = torch.as_tensor(text_tokens)
        if text_tokens.dim() != 2 or text_tokens.shape[0] != 1:
            raise ValueError("score_takes: text_tokens must be [1, L], one text for all the takes")
        rows = [torch.as_tensor(c).detach().to("cpu", torch.long).reshape(-1) for c in codes]
        if not rows or any(r.numel() == 0 for r in rows):
            raise ValueError("score_takes: at least one take, each with at least one code")
        n = len(rows)
        lat, emo = self._row_latents(rows_conditioning(cond, 1, self.device), 1)
        _, emb, mask = self.gpt.prepare_gpt_inputs(self.gpt.conds_latent(lat, emo), text_tokens)
        lp = self.gpt.score_codes(rows, emb.expand(n, -1, -1), attention_mask=mask.expand(n, -1)).cpu()
        lps = [lp[i, : rows[i].numel()] for i in range(n)]
        return lps, rank_request(rows, lps, n, self.stop_mel_token, length_penalty)[0]

    def synthesize_best_of(self, text_tokens: torch.Tensor, cond, best_of: int, max_mel_tokens: int = 1500,
                           repetition_penalty: float = 10.0, sampling: Optional[dict] = None, noise: Optional[torch.Tensor] = None,
                           per_row_noise: bool = False, noise_seeds=None, diffusion_steps=None, cfg_rate=None):
        """synthesize_batch on the best of `best_of` sampled takes of every row: ranked_takes, then only each row's winner goes through
        the latent pass, s2mel and the vocoder.  Returns the B waveforms; self.last_ranking keeps ranked_takes' ranking."""
        codes, ranking = self.ranked_takes(text_tokens, cond, best_of, max_mel_tokens=max_mel_tokens, repetition_penalty=repetition_penalty,
                                           sampling=sampling)
        self.last_ranking = ranking
        win = [i * int(best_of) + rk[0][0] for i, rk in enumerate(ranking)]
        st = self.gpt_stage(text_tokens, cond, max_mel_tokens=max_mel_tokens, repetition_penalty=repetition_penalty, codes=codes[win])
        return self.acoustic_stage(st, noise=noise, per_row_noise=per_row_noise, noise_seeds=noise_seeds, diffusion_steps=diffusion_steps,
                                   cfg_rate=cfg_rate)

    def gpt_stage(self, text_tokens: torch.Tensor, cond: PromptConditioning, max_mel_tokens: int = 1500,
                  repetition_penalty: float = 10.0, sampling: Optional[dict] = None, sync_timers: bool = False,
                  codes: Optional[torch.Tensor] = None) -> dict:
        """Decode + stop-token trim + latent pass (infer_v2.py:732-828) on the current stream; returns the state
        acoustic_stage consumes (device tensors + host lengths).  `codes` [B, n] (optional): take these codes instead of decoding --
        the rest of the flow on a given code sequence (parity checks feed the reference's codes through the stages behind the decode)."""
        dev = self.device
        B = text_tokens.shape[0]
        c = rows_conditioning(cond, B, dev)
        times = {}
        t0 = self._tick(sync_timers)
        lat, emo = self._row_latents(c, B)
        gen = dict(sampling) if sampling else {"do_sample": False}
        gen.setdefault("num_beams", 1)
        if codes is None:
            codes, _ = self.gpt.inference_speech(lat, text_tokens, emo_vec=emo, max_generate_length=max_mel_tokens,
                                                 repetition_penalty=repetition_penalty, **gen)
        else:
            codes = torch.as_tensor(codes).to(dev, torch.long)
        t1 = self._tick(sync_timers)
        times["gpt_gen_time"] = t1 - t0
        # trim at the first stop token (infer_v2.py:795-807)
        hc = codes.cpu().numpy()
        code_lens = []
        for row in hc:
            hits = np.nonzero(row == self.stop_mel_token)[0]
            code_lens.append(int(hits[0]) if len(hits) else len(row))
        if not all(cl > 0 for cl in code_lens):
            raise RuntimeError("a row produced the stop token first: nothing to synthesise")
        if any(cl == len(row) for cl, row in zip(code_lens, hc)) and hc.shape[1] >= max_mel_tokens:
            warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({max_mel_tokens}).", RuntimeWarning)
        max_len = max(code_lens)
        codes = codes[:, :max_len].contiguous()
        code_lens_t = torch.tensor(code_lens, dtype=torch.long)
        # per-row text length (rows are right-padded with stop_text_token); the latent pass left-pads + masks shorter rows
        tt = torch.as_tensor(text_tokens).cpu()
        text_lens = ((tt != self.cfg.gpt.stop_text_token) & (tt != self.cfg.gpt.start_text_token)).sum(1)
        latent = self.gpt.forward(lat, text_tokens, text_lens, codes, code_lens_t, emo_vec=emo)
        t2 = self._tick(sync_timers)
        times["gpt_forward_time"] = t2 - t1
        return {"cond": c, "B": B, "codes": codes, "code_lens": code_lens, "code_lens_t": code_lens_t, "latent": latent, "times": times}

    def acoustic_stage(self, st: dict, noise: Optional[torch.Tensor] = None, per_row_noise: bool = False, sync_timers: bool = False,
                       return_intermediates: bool = False, noise_seeds=None, diffusion_steps=None, cfg_rate=None):
        """s2mel (length regulator + CFM) and the vocoder (infer_v2.py:835-866) on the current stream.  st["cond"]: one
        PromptConditioning, or a list of one per row (rows_conditioning): then the CFM runs as ONE mixed-prompt batch
        (S2Mel.cfm_rows) and row b's noise -- given, or drawn -- covers its own Tp_b + Tg_b frames from column 0.
        noise_seeds: one int per row instead of `noise` (both: ValueError).  Row b's noise is then S2Mel.noise's function of
        (noise_seeds[b], channel, frame) alone -- the same in any batch, on any stream -- and torch's generators are not touched;
        per_row_noise is ignored.
        diffusion_steps / cfg_rate: the solver's Euler steps (ints >= 1) and inference_cfg_rate (finite, >= 0; 0 = the reference's
        single-evaluation branch).  None: st["diffusion_steps"] / st["cfg_rate"] where a serving pipeline put per-row values, else this
        instance's values (TARS_DIFFUSION_STEPS / TARS_CFG_RATE, the configuration) on the path of a call without them.  One value
        applies to every row; a sequence gives one per row (a wrong length: ValueError) and runs the batch through the per-row solver
        (S2Mel.cfm_rows / cfm_inference: idxtts_s2mel_cfm_sched), as does any rate equal to 0."""
        if noise is not None and noise_seeds is not None:
            raise ValueError("pass `noise` or `noise_seeds`, not both")
        if noise_seeds is not None:
            noise_seeds = [int(s) for s in noise_seeds]
            if len(noise_seeds) != st["B"]:
                raise ValueError(f"{len(noise_seeds)} noise seeds for {st['B']} rows")
            per_row_noise = False
        seeded = noise_seeds is not None
        steps = diffusion_steps if diffusion_steps is not None else st.get("diffusion_steps", self._diffusion_steps)
        rate = cfg_rate if cfg_rate is not None else st.get("cfg_rate", self._cfg_rate)
        if diffusion_steps is not None or cfg_rate is not None:      # (a wrong length, a value out of range: ValueError)
            from .s2mel import per_row_values
            per_row_values(steps, st["B"], "diffusion_steps")
            per_row_values(rate, st["B"], "cfg_rate")
        dev = self.device
        c, B, codes, code_lens, code_lens_t, latent, times = (st["cond"], st["B"], st["codes"], st["code_lens"], st["code_lens_t"],
                                                              st["latent"], dict(st["times"]))
        t2 = self._tick(sync_timers)
        condv, target_lens = self.s2mel.prepare_condition(latent, codes, code_lens_t)
        Tg = condv.shape[1]
        C = self.cfg.s2mel.in_channels
        if isinstance(c, list):
            x_lens = [int(x.prompt_condition.shape[1]) + int(t) for x, t in zip(c, target_lens.cpu().tolist())]
            T = max(x_lens)
            if noise is None and per_row_noise and B > 1:
                noise = torch.zeros([B, C, T], device=dev)
                for b in range(B):
                    noise[b, :, :x_lens[b]] = torch.randn([1, C, x_lens[b]], device=dev)[0]
            elif noise is None and not seeded:
                noise = torch.randn([B, C, T], device=dev)
            vc_target = self.s2mel.cfm_rows(condv, target_lens, [x.prompt_condition for x in c], [x.ref_mel for x in c],
                                            torch.cat([x.style for x in c]), steps, inference_cfg_rate=rate,
                                            z=noise, noise_seeds=noise_seeds)              # infer_v2.py:850-856, row by row
        else:
            Tp = c.prompt_condition.shape[1]
            cat_condition = torch.cat([c.prompt_condition.expand(B, -1, -1), condv], dim=1)     # infer_v2.py:850
            x_lens = target_lens.cpu() + Tp
            if noise is None and per_row_noise and B > 1:
                noise = torch.zeros([B, C, Tp + Tg], device=dev)
                for b in range(B):
                    nb = int(x_lens[b])
                    noise[b, :, :nb] = torch.randn([1, C, nb], device=dev)[0]
            elif noise is None and not seeded:
                noise = torch.randn([B, C, Tp + Tg], device=dev)
            mel = self.s2mel.cfm_inference(cat_condition, x_lens, c.ref_mel.expand(B, -1, -1), c.style.expand(B, -1), None,
                                           steps, inference_cfg_rate=rate, z=noise, noise_seeds=noise_seeds)
            vc_target = mel[:, :, Tp:]                                                      # infer_v2.py:856
        t3 = self._tick(sync_timers)
        times["s2mel_time"] = t3 - t2
        # vocoder: one ragged batch; every layer pads at each row's OWN end (zeros for the convolutions, replicate for the
        # anti-alias filters), exactly what the reference's B=1 call per utterance sees (infer_v2.py:860)
        wavs: List[Optional[torch.Tensor]] = [None] * B
        tl = target_lens.cpu().tolist()
        Tmax = max(tl)
        w = self.bigvgan(vc_target[:, :, :Tmax].float().contiguous(), lengths=tl if len(set(tl)) > 1 else None)
        w = torch.clamp(32767 * w, -32767.0, 32767.0)                                       # infer_v2.py:866
        up = self.cfg.bigvgan.total_upsample
        for b in range(B):
            wavs[b] = w[b, :, : tl[b] * up].contiguous()
        t4 = self._tick(sync_timers)
        times["bigvgan_time"] = t4 - t3
        self.last_stage_times = times
        if return_intermediates:
            return wavs, {"codes": codes, "code_lens": code_lens, "latent": latent, "cond": condv, "mel": vc_target,
                          "target_lens": tl}
        return wavs

    # ------------------------------------------------------------------------------------------
    def interval_silence(self, sampling_rate=22050, interval_silence=200):                 # infer_v2.py:484-497
        n = int(sampling_rate * interval_silence / 1000.0)
        return torch.zeros(1, n, device=self.device)

    def infer(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
              use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
              max_text_tokens_per_segment=120, stream_return=False, more_segment_before=0, return_audio=False,
              return_numpy=False, takes=1, best_of=1, diffusion_steps=None, cfg_rate=None, **generation_kwargs):
        """Reference signature and return contract (infer_v2.py:541-567): the generator itself when `stream_return`, else its
        first (only) item -- the output path, an InferenceResult, or (sampling_rate, int16 [n, 1]) -- or None for empty input.
        takes=n > 1: n takes of the whole text, one after the other, each drawing on from where the last one left the generators --
        a list of n results; with an output path the files are `stem.takeK.ext`, K = 0 .. n - 1.  Refused with `stream_return`.
        best_of=n > 1: every segment is decoded as n sampled takes that share one prefill, the takes are ranked by the model's own
        log-probabilities (ranked_takes: a take that ran into max_mel_tokens ranks last) and only the best one is synthesised; the
        return contract is that of a plain call, streaming included.  Needs do_sample=True, num_beams=1 (ValueError otherwise) and is
        refused together with takes > 1.
        diffusion_steps / cfg_rate: the CFM solver's Euler steps and guidance rate for this call (every segment); None: the instance's.
        `spk_audio_prompt` (and `emo_audio_prompt`): a WAV file path as in the reference, or a PromptAudio / PromptFeatures /
        PromptConditioning; `text`: a string (needs self.tokenizer), a list of token-id segments (List[List[int]]) or one segment
        (List[int] / 1-D tensor)."""
        takes = int(takes)
        if takes < 1 or (takes > 1 and stream_return):
            raise ValueError("takes must be >= 1, and takes > 1 does not stream (stream_return)")
        best_of = self._check_best_of(best_of, generation_kwargs)
        if best_of > 1 and takes > 1:
            raise ValueError("best_of returns the one best take, takes every take: pass one of them")
        if takes > 1:
            stem, ext = os.path.splitext(output_path) if output_path else (None, "")
            return [self.infer(spk_audio_prompt, text, f"{stem}.take{k}{ext}" if stem else output_path, emo_audio_prompt, emo_alpha,
                               emo_vector, use_emo_text, emo_text, use_random, interval_silence, verbose, max_text_tokens_per_segment,
                               False, more_segment_before, return_audio=return_audio, return_numpy=return_numpy,
                               diffusion_steps=diffusion_steps, cfg_rate=cfg_rate, **generation_kwargs)
                    for k in range(takes)]
        gen = self.infer_generator(spk_audio_prompt, text, output_path, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text,
                                   emo_text, use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return,
                                   more_segment_before, return_audio=return_audio, return_numpy=return_numpy, best_of=best_of,
                                   diffusion_steps=diffusion_steps, cfg_rate=cfg_rate, **generation_kwargs)
        if stream_return:
            return gen
        try:
            return list(gen)[0]
        except IndexError:
            return None

    @staticmethod
    def _check_best_of(best_of, generation_kwargs) -> int:
        best_of = int(best_of)
        if best_of < 1:
            raise ValueError("best_of must be >= 1")
        if best_of > 1 and not (generation_kwargs.get("do_sample", True) and int(generation_kwargs.get("num_beams", 3)) == 1):
            raise ValueError("best_of needs do_sample=True and num_beams=1: greedy takes are all the same, and a beam search already "
                             "returns its best hypothesis")
        return best_of

    def set_emotion_matrices(self, emo_matrix: torch.Tensor, spk_matrix: torch.Tensor, emo_num):
        """feat2.pt / feat1.pt and cfg.emo_num (infer_v2.py:281-289): the per-emotion banks the emo_vector mode mixes from."""
        emo_num = list(emo_num)
        self.emo_num = emo_num
        self.emo_matrix = torch.split(torch.as_tensor(emo_matrix).to(self.device, torch.float32), emo_num)
        self.spk_matrix = torch.split(torch.as_tensor(spk_matrix).to(self.device, torch.float32), emo_num)

    def emotion_vector_mix(self, style: torch.Tensor, emo_vector, use_random: bool = False):
        """infer_v2.py:668-679: per emotion pick the bank entry whose speaker vector is closest (cosine) to this prompt's style -- or a
        random one --, weight by emo_vector.  Returns (emovec_mat [1,d], weight_vector)."""
        if not hasattr(self, "emo_matrix"):
            raise RuntimeError("emo_vector needs the emotion banks: call set_emotion_matrices(emo_matrix, spk_matrix, emo_num) first")
        if len(emo_vector) != len(self.emo_num):
            raise ValueError(f"emo_vector needs {len(self.emo_num)} weights")
        import random
        weight_vector = torch.tensor(emo_vector, device=self.device, dtype=torch.float32)
        style = style.to(self.device, torch.float32)
        if use_random:
            index = [random.randint(0, x - 1) for x in self.emo_num]
        else:
            index = [int(torch.argmax(torch.nn.functional.cosine_similarity(style, tmp, dim=1))) for tmp in self.spk_matrix]     # find_most_similar_cosine
        emo_matrix = torch.cat([tmp[i].unsqueeze(0) for i, tmp in zip(index, self.emo_matrix)], 0)
        return torch.sum(weight_vector.unsqueeze(1) * emo_matrix, 0).unsqueeze(0), weight_vector

    def conditionings_from_emo_texts(self, feats: "PromptFeatures", emo_texts, emo_alpha=1.0, use_random=False) -> List["PromptConditioning"]:
        """One PromptConditioning per emotion text for the same speaker prompt, for the per-row `cond` of BatchPipeline.submit /
        ContinuousPipeline.submit: ONE batched classification (`qwen_emo.inference_batch`), the speaker-side encoders once, then per
        text the scaling, `emotion_vector_mix` and merge of `infer_generator`.  Element i is what
        `infer(feats, ..., use_emo_text=True, emo_text=emo_texts[i], emo_alpha=emo_alpha)` conditions on."""
        if not isinstance(feats, PromptFeatures):
            raise NotImplementedError("conditionings_from_emo_texts takes the speaker prompt as PromptFeatures")
        emo_texts = list(emo_texts)
        classifier = self.qwen_emo      # NotImplementedError when none is attached
        scores = classifier.inference_batch(emo_texts) if emo_texts else []
        scale = max(0.0, min(1.0, emo_alpha))                                                        # infer_v2.py:600-608
        base = PromptConditioning.from_features(self.gpt, feats, emo_alpha=1.0)                      # 610-615: the speaker prompt serves
        out = []
        for d in scores:
            emo_vector = list(d.values())      # the dict's order is the vector's
            if scale != 1.0:
                emo_vector = [int(x * scale * 10000) / 10000 for x in emo_vector]
            emovec = PromptConditioning.mix_emovec(base.emo_vec, self.emotion_vector_mix(feats.style, emo_vector, use_random=use_random))
            out.append(PromptConditioning(base.spk_cond_latent, emovec, base.style, base.prompt_condition, base.ref_mel))
        return out

    def infer_generator(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
                        use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
                        max_text_tokens_per_segment=120, stream_return=False, quick_streaming_tokens=0, return_audio=False,
                        return_numpy=False, best_of=1, diffusion_steps=None, cfg_rate=None, **generation_kwargs):
        """infer_v2.py:569-937.  Streaming (`stream_return`): after every segment yields its waveform (`[1, n]` float32 on the
        CPU, already scaled and clamped to +-32767) and then the inter-segment silence, and nothing else (874-879, 885-886)."""
        if stream_return and return_audio:
            raise ValueError("stream_return and return_audio are mutually exclusive")                # infer_v2.py:575-576
        best_of = self._check_best_of(best_of, generation_kwargs)
        if any(v is not None and not isinstance(v, (int, float)) for v in (diffusion_steps, cfg_rate)):
            raise ValueError("infer takes one diffusion_steps / cfg_rate value per call")
        text_str = text if isinstance(text, str) else None      # use_emo_text without emo_text classifies the text itself
        if isinstance(text, str):
            # text front-end (infer_v2.py:697-704): tokenize, split into segments, ids.  The tokenizer (indextts_amd/tokenizer.py) needs
            # the checkpoint's bpe.model and, for real text, the reference's normaliser (WeTextProcessing): both absent offline.
            tok = getattr(self, "tokenizer", None)
            if tok is None:
                raise RuntimeError("a str text needs the tokenizer: tts.tokenizer = TextTokenizer('checkpoints/bpe.model', normalizer); "
                                   "or pass token-id segments")
            tokens = tok.tokenize(text)
            text = [tok.convert_tokens_to_ids(seg) for seg in tok.split_segments(tokens, max_text_tokens_per_segment,
                                                                                 quick_streaming_tokens=quick_streaming_tokens)]
        if use_emo_text:                                                                             # infer_v2.py:591-598
            classifier = self.qwen_emo      # NotImplementedError when none is attached
            if emo_text is None:
                emo_text = text_str
            if emo_text is None:
                raise ValueError("use_emo_text with token-id text needs emo_text: there is no string to classify")
            emo_vector = list(classifier.inference(emo_text).values())      # the dict's order is the vector's
        if emo_vector is not None:
            emo_audio_prompt = None                                                                  # infer_v2.py:586-589
            scale = max(0.0, min(1.0, emo_alpha))                                                    # 600-608
            if scale != 1.0:
                emo_vector = [int(x * scale * 10000) / 10000 for x in emo_vector]
            emo_alpha = 1.0                                                                          # 610-615: the speaker prompt serves
        from .prompt import PromptAudio
        import os as _os
        if isinstance(spk_audio_prompt, (str, _os.PathLike)):
            # file path, as the reference takes it (infer_v2.py:628-630, 685): read, cut to 15 s, resample on the host
            # (indextts_amd/audioio.py); loaded once per path like cache_spk_audio_prompt / cache_emo_audio_prompt (618, 681)
            from .audioio import load_prompt_audio
            # ONE entry per kind, like the reference's cache_spk_audio_prompt / cache_emo_audio_prompt (infer_v2.py:304-310, 618, 681):
            # another path replaces it, and so does the same path once the file has changed (size / modification time)
            files = getattr(self, "_prompt_files", None)
            if files is None:
                files = self._prompt_files = {}

            def cached(kind, path, **kw):
                path = _os.fspath(path)
                st = _os.stat(path)
                key = (path, st.st_mtime_ns, st.st_size)
                hit = files.get(kind)
                if hit is None or hit[0] != key:
                    hit = files[kind] = (key, load_prompt_audio(path, **kw))
                return hit[1]
            spk_audio_prompt = cached("spk", spk_audio_prompt)
            if isinstance(emo_audio_prompt, (str, _os.PathLike)):
                emo_audio_prompt = cached("emo", emo_audio_prompt, emotion=True)
        if isinstance(spk_audio_prompt, PromptAudio):
            # audio path: w2v-bert / semantic codec / CAMPPlus / mel / length regulator on the GPU (indextts_amd/prompt.py), cached per
            # prompt object like the reference's cache_spk_cond / cache_emo_cond (infer_v2.py:618, 681)
            enc = getattr(self, "prompt_encoders", None)
            if enc is None:
                raise RuntimeError("attach the audio-side encoders first: tts.prompt_encoders = PromptEncoders(w2vbert_sd, codec_sd, campplus_sd, tts.s2mel)")
            if emo_audio_prompt is not None and not isinstance(emo_audio_prompt, PromptAudio):
                raise NotImplementedError("with an audio speaker prompt the emotion prompt must be a PromptAudio too")
            akey = (id(spk_audio_prompt), id(emo_audio_prompt))
            if getattr(self, "_audio_cache_key", None) != akey:
                self._audio_cache = enc.encode(spk_audio_prompt, emo_audio_prompt)
                self._audio_cache_key = akey
                self._audio_cache_refs = (spk_audio_prompt, emo_audio_prompt)
            spk_audio_prompt, emo_audio_prompt = self._audio_cache, None
        if isinstance(spk_audio_prompt, PromptFeatures):
            # prompt-feature path: conformer + perceiver + emotion vector on the GPU, cached per (prompt, emotion prompt, alpha) like
            # the reference caches its prompt features (infer_v2.py:618, 681)
            feats = spk_audio_prompt
            if emo_audio_prompt is not None:
                if not isinstance(emo_audio_prompt, (PromptFeatures, torch.Tensor)):
                    raise NotImplementedError("emo_audio_prompt must be a PromptFeatures or the emotion prompt's [1,T,1024] features")
                emo_emb = emo_audio_prompt.spk_cond_emb if isinstance(emo_audio_prompt, PromptFeatures) else emo_audio_prompt
                feats = PromptFeatures(feats.spk_cond_emb, feats.style, feats.prompt_condition, feats.ref_mel, emo_emb)
            key = (id(spk_audio_prompt), id(emo_audio_prompt), float(emo_alpha), None if emo_vector is None else (tuple(emo_vector), bool(use_random)))
            if getattr(self, "_cond_cache_key", None) != key or (emo_vector is not None and use_random):
                mix = None if emo_vector is None else self.emotion_vector_mix(feats.style, emo_vector, use_random=use_random)
                self._cond_cache = PromptConditioning.from_features(self.gpt, feats, emo_alpha=emo_alpha, emo_mix=mix)
                self._cond_cache_key = key
                self._cond_cache_refs = (spk_audio_prompt, emo_audio_prompt)     # keep the ids alive
            spk_audio_prompt = self._cond_cache
        elif emo_audio_prompt is not None or emo_vector is not None:
            raise NotImplementedError("with a ready PromptConditioning the emotion prompt / vector is already folded into emo_vec")
        if not isinstance(spk_audio_prompt, PromptConditioning):
            raise NotImplementedError("pass a wav file path or a PromptAudio (both need tts.prompt_encoders), PromptFeatures or a PromptConditioning: "
                                      "reading and resampling audio files is left to the caller (librosa / torchaudio are not in this image)")
        segs = text if (len(text) and isinstance(text[0], (list, tuple, np.ndarray, torch.Tensor))) else [text]
        segs = [torch.as_tensor(s, dtype=torch.long).reshape(1, -1) for s in segs]
        if not segs or any(s.numel() == 0 for s in segs):
            return                                                                                   # nothing yielded -> infer() returns None
        # generation kwargs and their defaults: infer_v2.py:714-722.  The reference pops `do_sample` and then hard-codes
        # do_sample=True in the call (line 767): its default mode is beam-sample with 3 beams.  Here the popped value is honoured
        # (do_sample=False, num_beams=1 is the greedy parity mode of BASELINE configs[2]); the defaults are the reference's.
        do_sample = generation_kwargs.pop("do_sample", True)
        top_p = generation_kwargs.pop("top_p", 0.8)
        top_k = generation_kwargs.pop("top_k", 30)
        temperature = generation_kwargs.pop("temperature", 0.8)
        length_penalty = generation_kwargs.pop("length_penalty", 0.0)
        num_beams = generation_kwargs.pop("num_beams", 3)
        repetition_penalty = generation_kwargs.pop("repetition_penalty", 10.0)
        max_mel_tokens = generation_kwargs.pop("max_mel_tokens", 1500)
        # noise_seed: the CFM noise of segment i comes from seed i of utterance_noise_seeds(noise_seed, n_segments) instead of
        # torch's generator -- the same audio streaming or not, at any segment_batch, whatever else draws from torch
        from .serving import utterance_noise_seeds
        nseeds = utterance_noise_seeds(generation_kwargs.pop("noise_seed", None), len(segs))
        sampling = {"do_sample": bool(do_sample), "num_beams": int(num_beams), "generator": generation_kwargs.pop("generator", None)}
        if do_sample:
            sampling.update(top_p=top_p, top_k=top_k, temperature=temperature)
        if num_beams > 1:
            sampling["length_penalty"] = length_penalty
        elif do_sample:
            sampling["sampler"] = generation_kwargs.pop("sampler", "hf")
        if generation_kwargs:
            raise TypeError(f"unsupported generation kwargs: {sorted(generation_kwargs)}")
        start = time.perf_counter()
        wavs = []
        sil = self.interval_silence(interval_silence=interval_silence)
        # best_of: the same call on each row's best take (synthesize_best_of)
        synthesize = self.synthesize_batch if best_of == 1 else functools.partial(self.synthesize_best_of, best_of=best_of)
        if diffusion_steps is not None or cfg_rate is not None:
            synthesize = functools.partial(synthesize, diffusion_steps=diffusion_steps, cfg_rate=cfg_rate)
        if stream_return:
            for i, s in enumerate(segs):                                                             # segment loop, infer_v2.py:732
                w = synthesize(s, spk_audio_prompt, max_mel_tokens=max_mel_tokens, repetition_penalty=repetition_penalty,
                               sampling=sampling, noise_seeds=None if nseeds is None else nseeds[i:i + 1])[0]
                yield w.cpu()                                                                        # infer_v2.py:874-879
                yield sil.cpu()
            return                                                                                   # infer_v2.py:885-886
        # Not streaming: the segments of one text are independent utterances of the same prompt, so they go through the
        # batched path `segment_batch` at a time (one decode loop, one CFM solve, one ragged vocoder pass) instead of one by
        # one; greedy codes are identical to the one-by-one flow, and the CFM noise is drawn segment by segment in order, so
        # under a seed the waveforms agree with it to fp32 rounding.  segment_batch = 1 is the reference's loop as written.
        nb = max(1, int(self.segment_batch))
        stop_text = self.cfg.gpt.stop_text_token
        for i in range(0, len(segs), nb):
            grp = segs[i:i + nb]
            L = max(s.shape[1] for s in grp)
            toks = torch.full((len(grp), L), stop_text, dtype=torch.long)
            for r, s in enumerate(grp):
                toks[r, : s.shape[1]] = s[0]
            wavs.extend(synthesize(toks, spk_audio_prompt, max_mel_tokens=max_mel_tokens, repetition_penalty=repetition_penalty,
                                   sampling=sampling, per_row_noise=True, noise_seeds=None if nseeds is None else nseeds[i:i + nb]))
        out = []
        for i, w in enumerate(wavs):                                                                 # insert_interval_silence 499-522
            out.append(w)
            if i + 1 < len(wavs):
                out.append(sil)
        wav = torch.cat(out, dim=1).cpu()
        total = time.perf_counter() - start
        mono = wav.squeeze(0).contiguous()
        sr = 22050
        wav_length = mono.shape[-1] / sr
        rtf = (total / wav_length) if wav_length else None
        saved = None
        if output_path and not return_audio:
            from .wavio import write_wav_int16
            if os.path.dirname(output_path):
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            write_wav_int16(output_path, mono.to(torch.int16).numpy(), sr)
            yield output_path                                                                        # infer_v2.py:917
            return
        if return_audio:
            audio = mono.clone()
            yield InferenceResult(sr, audio.numpy().copy() if return_numpy else audio, float(wav_length), saved, rtf)
            return
        yield (sr, mono.unsqueeze(0).to(torch.int16).numpy().T)                                      # infer_v2.py:935-937
