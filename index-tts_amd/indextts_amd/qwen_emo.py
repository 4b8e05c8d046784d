"""Emotion from text: the reference's `QwenEmotion` (indextts/infer_v2.py:948-1063) on the HIP Qwen3 decoder.

`QwenLM` is the language model (include/idxtts.h "emotion-from-text classifier"): a Qwen3 causal LM, prefill + greedy decode on the
GPU for one prompt (`generate`) or for several that share every weight pass (`generate_batch`, each row bit-equal to its own `generate`).  `QwenEmotion` wraps it the way the reference wraps transformers: a two-message chat prompt, greedy generation up
to the end token, the answer parsed as JSON into eight scores in a fixed order.  The tokenizer is whatever the caller hands in (the
reference's is transformers' AutoTokenizer; checkpoint.qwen_emotion_from_pretrained binds it) -- this module imports no transformers.
"""
from __future__ import annotations

import ctypes
import json
import re
import warnings
from ctypes import c_int, c_void_p
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, synth

WEIGHT_FORMATS = {"f32": 0, "fp32": 0, "bf16": 1}
THINK_END_ID = 151668      # "</think>" of the Qwen3 vocabulary (infer_v2.py:1029-1033)


@dataclass(frozen=True)
class QwenConfig:
    """The fields of HF `Qwen3Config` the arithmetic needs; defaults = the published Qwen3-0.6B."""
    vocab_size: int = 151936
    hidden_size: int = 1024
    intermediate_size: int = 3072
    num_hidden_layers: int = 28
    num_attention_heads: int = 16
    num_key_value_heads: int = 8
    head_dim: int = 128
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    tie_word_embeddings: bool = True
    max_context: int = 4096

    @staticmethod
    def from_hf(j: dict, max_context: int = 4096) -> "QwenConfig":
        """From a parsed config.json (keys absent there keep the 0.6B defaults)."""
        d = QwenConfig()
        keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
                "head_dim", "rms_norm_eps", "rope_theta", "tie_word_embeddings")
        return QwenConfig(**{k: type(getattr(d, k))(j.get(k, getattr(d, k))) for k in keys}, max_context=int(max_context))

    @staticmethod
    def tiny() -> "QwenConfig":
        return QwenConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                          num_key_value_heads=1, max_context=512)


def to_bf16_grid(a: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bf16 (ties to even), still float32: what a bf16 checkpoint widened to fp32 holds."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    with np.errstate(over="ignore"):
        r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32).reshape(a.shape)


def synth_qwen_weights(cfg: QwenConfig, tag: str = "qwen") -> dict:
    """Random-initialised Qwen3 state dict under the HF keys, every tensor on the bf16 grid (as the published checkpoint is)."""
    H, I, hd = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    qd, kd = cfg.num_attention_heads * hd, cfg.num_key_value_heads * hd
    w = {"model.embed_tokens.weight": synth.uniform(f"{tag}/embed", (cfg.vocab_size, H), 0.08),
         "model.norm.weight": synth.uniform(f"{tag}/norm", (H,), 0.3, 1.0)}
    for i in range(cfg.num_hidden_layers):
        p, t = f"model.layers.{i}.", f"{tag}/l{i}/"
        for name, shape, fan in (("self_attn.q_proj", (qd, H), H), ("self_attn.k_proj", (kd, H), H), ("self_attn.v_proj", (kd, H), H),
                                 ("self_attn.o_proj", (H, qd), qd), ("mlp.gate_proj", (I, H), H), ("mlp.up_proj", (I, H), H),
                                 ("mlp.down_proj", (H, I), I)):
            w[p + name + ".weight"] = synth.fan_in_uniform(t + name, shape, fan, gain=1.4)
        for name, n in (("self_attn.q_norm", hd), ("self_attn.k_norm", hd), ("input_layernorm", H), ("post_attention_layernorm", H)):
            w[p + name + ".weight"] = synth.uniform(t + name, (n,), 0.3, 1.0)
    if not cfg.tie_word_embeddings:
        w["lm_head.weight"] = synth.fan_in_uniform(f"{tag}/lm_head", (cfg.vocab_size, H), H)
    return {k: to_bf16_grid(v) for k, v in w.items()}


def rotary_inv_freq(cfg: QwenConfig) -> torch.Tensor:
    """transformers' default rope initialisation, step for step in fp32 (modeling_rope_utils._compute_default_rope_parameters)."""
    return 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.int64).float() / cfg.head_dim))


def _hp(a):
    """Host pointer of a numpy array (null for None or an empty one)."""
    return c_void_p(a.ctypes.data) if a is not None and a.size else c_void_p(0)


class QwenLM:
    """Qwen3 causal LM on the HIP library: `generate(prompt_ids, ...)` = prefill + greedy decode; `generate_batch` for several prompts."""

    def __init__(self, state_dict, cfg: QwenConfig = QwenConfig(), device="cuda:0", weight_format: str = "bf16"):
        if weight_format not in WEIGHT_FORMATS:
            raise ValueError(f"weight_format must be one of {sorted(WEIGHT_FORMATS)}")
        self.cfg, self.device, self.weight_format = cfg, torch.device(device), weight_format
        lib = self._lib = _lib.load()
        c = _lib.QwenConfigC(cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                             cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.rope_theta, int(cfg.tie_word_embeddings),
                             cfg.max_context)
        h = c_void_p()
        _lib.check(lib.idxtts_qwen_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h
        sd = dict(state_dict)
        if cfg.tie_word_embeddings:
            sd.pop("lm_head.weight", None)      # the checkpoint may repeat the table under this key
        sd.setdefault("model.rotary_emb.inv_freq", rotary_inv_freq(cfg))
        with torch.cuda.device(self.device):
            _lib.load_state_dict(h, sd, before_finalize=lambda ctx: _lib.check(
                lib.idxtts_qwen_set_weight_format(ctx, WEIGHT_FORMATS[weight_format])))
        self._ws = _lib.StreamWorkspaces(2)

    def _call_args(self, eos_ids, logits: bool, logit_cols):
        """What `generate` and `generate_batch` hand over alike: (eos, cols, n_cols), then the C arguments that follow out_logits."""
        eos = np.ascontiguousarray(list(eos_ids), dtype=np.int32).reshape(-1)
        cols = None if logit_cols is None else np.ascontiguousarray(logit_cols, dtype=np.int32).reshape(-1)
        n_cols = 0 if not logits else (self.cfg.vocab_size if cols is None else int(cols.size))
        return eos, cols, n_cols, (_hp(cols) if logits else c_void_p(0), 0 if cols is None else int(cols.size))

    def generate(self, prompt_ids, max_new_tokens: int, eos_ids=(), forced_ids=None, logits: bool = False, logit_cols=None,
                 use_graph: bool = True):
        """Greedy continuation of `prompt_ids`: returns (ids, logits).  ids: each step's argmax up to and including the first one in
        `eos_ids` (or `max_new_tokens` of them); logits: None, or a [len(ids), n] float32 tensor of every step's logits at
        `logit_cols` (all columns when None).  forced_ids: teacher forcing -- they continue the sequence, ids stay the model's own."""
        prompt = np.ascontiguousarray(prompt_ids, dtype=np.int32).reshape(-1)
        eos, cols, n_cols, col_args = self._call_args(eos_ids, logits, logit_cols)
        P, M = int(prompt.size), int(max_new_tokens)
        forced = None
        if forced_ids is not None:
            forced = np.ascontiguousarray(forced_ids, dtype=np.int32).reshape(-1)
            if forced.size != M:
                raise ValueError("forced_ids needs max_new_tokens entries")
        out_ids = np.zeros(M, dtype=np.int32)
        n_out = c_int(0)
        with torch.cuda.device(self.device):
            need = self._lib.idxtts_qwen_workspace_bytes(self._h, P, M, int(eos.size), n_cols)
            if need == 0:
                raise ValueError("empty prompt or max_new_tokens < 1")
            ws = self._ws.get(need, self.device)
            lg = torch.zeros(M, n_cols, dtype=torch.float32, device=self.device) if logits else None
            _lib.check(self._lib.idxtts_qwen_generate(self._h, _hp(prompt), P, M, _hp(eos), int(eos.size), _hp(forced), _hp(out_ids),
                                                      ctypes.byref(n_out), _lib.ptr(lg), *col_args, _lib.ptr(ws), ws.numel(), int(use_graph),
                                                      _lib.current_stream()))
        n = n_out.value
        return out_ids[:n].tolist(), (lg[:n] if logits else None)

    def max_batch(self) -> int:
        """Rows the library passes through the weights together; `generate_batch` takes any number and serves them in such tiles."""
        return int(self._lib.idxtts_qwen_max_batch(self._h))

    def generate_batch(self, prompts, max_new_tokens, eos_ids=(), forced_ids=None, logits: bool = False, logit_cols=None,
                       use_graph: bool = True):
        """`generate` for several prompts at once: row b equals generate(prompts[b], max_new_tokens[b], ...) bit for bit.
        max_new_tokens: an int or one per row; forced_ids: one array per row (max_new_tokens[b] entries).  Returns (list of id lists,
        list of [n_b, n_cols] float32 tensors or None)."""
        rows = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in prompts]
        B = len(rows)
        if B < 1:
            raise ValueError("generate_batch needs at least one prompt")
        caps = [int(max_new_tokens)] * B if np.isscalar(max_new_tokens) else [int(m) for m in max_new_tokens]
        if len(caps) != B:
            raise ValueError("max_new_tokens: an int, or one per prompt")
        eos, cols, n_cols, col_args = self._call_args(eos_ids, logits, logit_cols)
        forced = None
        if forced_ids is not None:
            fr = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1) for f in forced_ids]
            if len(fr) != B or any(f.size != m for f, m in zip(fr, caps)):
                raise ValueError("forced_ids needs one array per prompt with that row's max_new_tokens entries")
            forced = np.ascontiguousarray(np.concatenate(fr)) if fr else None
        n_prompt = np.ascontiguousarray([r.size for r in rows], dtype=np.int32)
        max_new = np.ascontiguousarray(caps, dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(rows)) if all(r.size for r in rows) else np.zeros(0, dtype=np.int32)
        total = int(sum(max(0, m) for m in caps))
        out_ids = np.zeros(max(1, total), dtype=np.int32)
        n_out = np.zeros(B, dtype=np.int32)
        with torch.cuda.device(self.device):
            need = self._lib.idxtts_qwen_batch_workspace_bytes(self._h, B, _hp(n_prompt), _hp(max_new), int(eos.size), n_cols)
            if need == 0:
                raise ValueError("empty prompt or max_new_tokens < 1")
            ws = self._ws.get(need, self.device)
            lg = torch.zeros(total, n_cols, dtype=torch.float32, device=self.device) if logits else None
            _lib.check(self._lib.idxtts_qwen_generate_batch(self._h, B, _hp(flat), _hp(n_prompt), _hp(max_new), _hp(eos), int(eos.size), _hp(forced),
                                                            _hp(out_ids), _hp(n_out), _lib.ptr(lg), *col_args, _lib.ptr(ws), ws.numel(),
                                                            int(use_graph), _lib.current_stream()))
        ids, lgs, off = [], [], 0
        for b in range(B):
            n = int(n_out[b])
            ids.append(out_ids[off:off + n].tolist())
            if logits:
                lgs.append(lg[off:off + n])
            off += caps[b]
        return ids, (lgs if logits else None)

    def batch_step_graph_launches(self) -> int:
        """Kernel launches of the kept batched decode-step graph (-1: none held)."""
        return int(self._lib.idxtts_qwen_batch_step_graph_launches(self._h))

    def step_graph_launches(self) -> int:
        """Kernel launches of the kept decode-step graph (-1: none held)."""
        return int(self._lib.idxtts_qwen_step_graph_launches(self._h))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().idxtts_ctx_destroy(self._h)
        except Exception:
            pass


# score name in the model's answer -> name in the result, in the order of the emotion vector (infer_v2.py:966-981, 530)
EMOTION_KEYS = (("高兴", "happy"), ("愤怒", "angry"), ("悲伤", "sad"), ("恐惧", "afraid"), ("反感", "disgusted"), ("低落", "melancholic"),
                ("惊讶", "surprised"), ("自然", "calm"))
# words in the input that turn a detected "sad" into "melancholic": the model does not tell the two apart (infer_v2.py:982-991)
MELANCHOLIC_WORDS = ("低落", "melancholy", "melancholic", "depression", "depressed", "gloomy")
EMO_BIAS = (0.9375, 0.875, 1.0, 1.0, 0.9375, 0.9375, 0.6875, 0.5625)      # IndexTTS2.normalize_emo_vec, infer_v2.py:524-538


def normalize_emo_vec(emo_vector, apply_bias: bool = True):
    """infer_v2.py:524-538: optional per-emotion de-emphasis, then the sum is brought down to 0.8 when it is above."""
    vec = list(emo_vector)
    if apply_bias:
        vec = [v * b for v, b in zip(vec, EMO_BIAS)]
    total = sum(vec)
    if total > 0.8:
        k = 0.8 / total
        vec = [v * k for v in vec]
    return vec


class QwenEmotion:
    """`inference(text) -> {"happy": .., "angry": .., "sad": .., "afraid": .., "disgusted": .., "melancholic": .., "surprised": ..,
    "calm": ..}` as the reference's class of the same name.  state_dict / cfg: the fine-tuned Qwen3 under the HF keys; tokenizer:
    duck-typed (apply_chat_template, __call__, decode, eos_token_id).  eos_ids: ids that end the answer (generation_config.json's;
    default: the tokenizer's eos_token_id).  max_new_tokens caps the answer (the reference asks for 32768 and relies on the end
    token; an answer is ~60 tokens) -- reaching the cap warns."""

    def __init__(self, state_dict, cfg: QwenConfig, tokenizer, weight_format: str = "bf16", device="cuda:0", max_new_tokens: int = 512,
                 eos_ids=None, model=None):
        self.tokenizer = tokenizer
        self.model = model if model is not None else QwenLM(state_dict, cfg, device=device, weight_format=weight_format)
        self.max_new_tokens = int(max_new_tokens)
        self.eos_ids = eos_ids
        self.prompt = "文本情感分类"
        self.cn_key_to_en = dict(EMOTION_KEYS)
        self.desired_vector_order = [cn for cn, _ in EMOTION_KEYS]
        self.melancholic_words = set(MELANCHOLIC_WORDS)
        self.max_score = 1.2
        self.min_score = 0.0

    @classmethod
    def from_pretrained(cls, model_dir: str, **kw) -> "QwenEmotion":
        """From a checkpoint directory (checkpoint.qwen_emotion_from_pretrained)."""
        from .checkpoint import qwen_emotion_from_pretrained
        return qwen_emotion_from_pretrained(model_dir, **kw)

    def clamp_score(self, value):
        return max(self.min_score, min(self.max_score, value))

    def convert(self, content):
        out = {en: self.clamp_score(content.get(cn, 0.0)) for cn, en in EMOTION_KEYS}
        if all(v <= 0.0 for v in out.values()):
            out["calm"] = 1.0      # nothing detected: the neutral voice
        return out

    def _end_ids(self):
        ids = self.eos_ids if self.eos_ids is not None else self.tokenizer.eos_token_id
        if ids is None:
            return []
        return [int(i) for i in ids] if isinstance(ids, (list, tuple)) else [int(ids)]

    def _warn_if_cut(self, ids):
        if len(ids) >= self.max_new_tokens and (not ids or ids[-1] not in self._end_ids()):
            warnings.warn(f"QwenEmotion: no end token within max_new_tokens={self.max_new_tokens}; the answer is cut there")

    def generate(self, input_ids):
        """The answer's token ids (the end token included when it came): what the reference slices off model.generate's output."""
        ids, _ = self.model.generate(input_ids, self.max_new_tokens, eos_ids=self._end_ids())
        self._warn_if_cut(ids)
        return ids

    def generate_batch(self, input_ids_rows):
        """`generate` for several prompts in one batched call of the language model; the cap warning fires per row."""
        rows, _ = self.model.generate_batch(input_ids_rows, self.max_new_tokens, eos_ids=self._end_ids())
        for ids in rows:
            self._warn_if_cut(ids)
        return rows

    def _prompt_ids(self, text_input):
        messages = [{"role": "system", "content": f"{self.prompt}"}, {"role": "user", "content": f"{text_input}"}]
        text = self.tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True, enable_thinking=False)
        enc = self.tokenizer([text])
        input_ids = enc["input_ids"] if isinstance(enc, dict) else enc.input_ids
        input_ids = input_ids[0]
        if hasattr(input_ids, "tolist"):
            input_ids = input_ids.tolist()
        return list(input_ids)

    def _scores(self, text_input, output_ids):
        """The answer's ids -> the eight scores: parsing, the melancholic swap, clamping (one copy for `inference` and `inference_batch`)."""
        output_ids = list(output_ids)
        # what follows the last "</think>"
        start = 0
        for i in range(len(output_ids) - 1, -1, -1):
            if output_ids[i] == THINK_END_ID:
                start = i + 1
                break
        content = self.tokenizer.decode(output_ids[start:], skip_special_tokens=True)
        try:
            content = json.loads(content)
        except json.decoder.JSONDecodeError:      # not JSON: pick `name: number` pairs out of the string
            content = {m.group(1): float(m.group(2)) for m in re.finditer(r'([^\s":.,]+?)"?\s*:\s*([\d.]+)', content)}
        lowered = text_input.lower()
        if any(word in lowered for word in self.melancholic_words):
            content["悲伤"], content["低落"] = content.get("低落", 0.0), content.get("悲伤", 0.0)
        return self.convert(content)

    def inference(self, text_input):
        return self._scores(text_input, self.generate(self._prompt_ids(text_input)))

    def inference_batch(self, texts):
        """`inference` for several texts with one batched generation: element i equals inference(texts[i])."""
        texts = list(texts)
        if not texts:
            return []
        answers = self.generate_batch([self._prompt_ids(t) for t in texts])
        return [self._scores(t, ids) for t, ids in zip(texts, answers)]
