"""Host-side mirror of the reference's GPT interface (indextts/gpt/model_v2.py), backed by libidxtts_hip.

`UnifiedVoice` keeps the reference's method names and argument meaning for the hot path:
  * prepare_gpt_inputs(conditional_latents, text_inputs)           model_v2.py:725-794
  * inference_speech(..., text_inputs, emo_vec=..., **generate kw)  model_v2.py:796-895 (greedy path)
  * forward(...) -> latent                                          model_v2.py:673-723
  * accel_engine-style generate(input_ids, max_new_tokens, ..., attention_mask, tts_embeddings, ...)
                                                                    accel/accel_engine.py:378-645 (plugin slot)
  * get_conditioning / get_emovec / merge_emovec                      model_v2.py:627-671, 897-910 (cond.py, csrc/cond.hip)
The conformer / perceiver conditioning encoders are built when the state dict carries their weights; `inference_speech`
then accepts the prompt features [B,T,1024] like the reference does, or -- hoisted out of the segment loop, where the
reference recomputes them per segment (infer_v2.py:748-765) -- the ready `speech_conditioning_latent` [B,32,d] + `emo_vec`.
All arithmetic runs in the HIP kernels; numpy/torch only build int32 index arrays and own the buffers.
"""
from __future__ import annotations

import ctypes
import warnings
from ctypes import c_void_p
from typing import Optional

import numpy as np
import torch

from . import _lib
from .config import GPTConfig


def _i32(dev, arr) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(dev)


WEIGHT_FORMATS = {"f32": 0, "bf16": 1, "fp8": 2}
KV_FORMATS = {"f32": 0, "bf16": 1, "fp8": 2}


class UnifiedVoice:
    MAX_WORKSPACES = 4

    def __init__(self, state_dict, cfg: GPTConfig = GPTConfig(), device="cuda:0", weight_format: str = "f32", keep_effective: bool = False,
                 kv_format: str = None, batch_invariant: bool = False):
        """weight_format: storage of the GPT's linear weights -- "f32" (default), "bf16", or "fp8" (e4m3 + power-of-two scale
        per output channel): the reference's `use_fp16` switch (infer_v2.py:145-146) / BASELINE configs[4].  The weights are
        rounded ONCE at load (`idxtts_gpt_quantize_weights`); the arithmetic stays fp32, and every pass runs that one rounded
        model.  keep_effective: keep `self.effective_state_dict` (numpy, reference keys) = exactly that model, for parity checks.
        kv_format: storage of the KV cache of the cached generation, "f32", "bf16" or "fp8" (`idxtts_gpt_set_kv_format`: keys /
        values rounded once, when produced -- to bf16, or to e4m3 codes with one power-of-two scale per 64-dim vector; fp32
        arithmetic).  Default: "f32" with fp32 weights, "bf16" with compact weights -- the reference's `use_fp16` halves weights
        and cache together; "fp8" is opt-in only, fp8 weights do not select it.
        batch_invariant: the opt-in batch-invariant mode (`set_batch_invariant`)."""
        lib = _lib.load()
        if weight_format not in WEIGHT_FORMATS:
            raise ValueError(f"weight_format must be one of {sorted(WEIGHT_FORMATS)}")
        self.weight_format = weight_format
        if kv_format is None:
            kv_format = "f32" if weight_format == "f32" else "bf16"
        if kv_format not in KV_FORMATS:
            raise ValueError(f"kv_format must be one of {sorted(KV_FORMATS)}")
        self.kv_format = kv_format
        self.effective_state_dict = None
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the HIP GPT path needs a ROCm GPU device; there is no CPU fallback")
        c = _lib.GPTConfigC(cfg.model_dim, cfg.heads, cfg.layers, cfg.number_mel_codes, cfg.number_text_tokens,
                            cfg.start_mel_token, cfg.stop_mel_token, cfg.mel_pos_len, cfg.text_pos_len)
        h = c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.idxtts_gpt_create(ctypes.byref(c), ctypes.byref(h)))
            self._h = h
            sd = {k: v for k, v in state_dict.items() if self._on_path(k)}

            def hook(ctx):
                if WEIGHT_FORMATS[weight_format]:
                    _lib.check(lib.idxtts_gpt_quantize_weights(ctx, WEIGHT_FORMATS[weight_format]))
                if keep_effective:
                    self.effective_state_dict = {k: _lib.get_tensor(ctx, k, tuple(v.shape)) for k, v in sd.items()}
            _lib.load_state_dict(h, sd, before_finalize=hook)
            _lib.check(lib.idxtts_gpt_set_kv_format(h, KV_FORMATS[kv_format]))
            _lib.check(lib.idxtts_gpt_set_batch_invariant(h, int(bool(batch_invariant))))
        self.batch_invariant = bool(batch_invariant)
        from .cond import ConditioningEncoders
        self.cond = ConditioningEncoders(state_dict, cfg, device=self.device) if ConditioningEncoders.has_weights(state_dict) else None
        se = state_dict["speed_emb.weight"]
        self.speed_emb = (se if isinstance(se, torch.Tensor) else torch.from_numpy(np.asarray(se))).float().to(self.device)
        import threading
        self._ws = None
        self._ws_lock = threading.Lock()
        self._conds_cache = {}
        self._conds_lock = threading.Lock()
        self.stop_mel_token = cfg.stop_mel_token
        self.start_mel_token = cfg.start_mel_token
        self.accel_engine = self       # the reference selects `self.accel_engine.generate` (model_v2.py:871)

    def set_kv_format(self, kv_format: str) -> None:
        """Switch the KV-cache storage between generations ("f32" | "bf16" | "fp8")."""
        if kv_format not in KV_FORMATS:
            raise ValueError(f"kv_format must be one of {sorted(KV_FORMATS)}")
        _lib.check(_lib.load().idxtts_gpt_set_kv_format(self._h, KV_FORMATS[kv_format]))
        self.kv_format = kv_format

    def set_batch_invariant(self, on: bool = True) -> None:
        """Switch the batch-invariant mode between generations (`idxtts_gpt_set_batch_invariant`, per context, default off).  With it
        on, a request's codes (and recorded logits) equal bit for bit those of the B = 1 call on its own unpadded prompt, whichever
        batch, session size, slot, lane or park / resume history it runs with, and seeded draws carry no term in the batch size.  A
        decode session keeps the mode it was opened in."""
        _lib.check(_lib.load().idxtts_gpt_set_batch_invariant(self._h, int(bool(on))))
        self.batch_invariant = bool(on)

    @staticmethod
    def _on_path(key: str) -> bool:
        return key.startswith(("gpt.h.", "gpt.ln_f.", "final_norm.", "mel_head.", "mel_embedding.", "text_embedding.",
                               "mel_pos_embedding.", "text_pos_embedding.", "speed_emb."))

    # ------------------------------------------------------------------------------------------
    def _workspace(self, B: int, S: int, max_new: int) -> torch.Tensor:
        need = int(_lib.load().idxtts_gpt_workspace_bytes(self._h, B, S, max_new))
        if need == 0:
            raise RuntimeError("idxtts_gpt_workspace_bytes returned 0")
        return self._workspace_bytes(need)

    def _workspace_bytes(self, need: int) -> torch.Tensor:
        # one workspace per HIP stream (calls on one stream are ordered, so they can share it; generate() may run concurrently
        # on several streams from several host threads); least-recently-used streams beyond MAX_WORKSPACES are dropped, so
        # short-lived threads / streams cannot pile up KV arenas
        import collections
        if self._ws is None:
            self._ws = collections.OrderedDict()
        key = int(torch.cuda.current_stream(self.device).cuda_stream)
        with self._ws_lock:
            ws = self._ws.pop(key, None)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
            while len(self._ws) > self.MAX_WORKSPACES:
                self._ws.popitem(last=False)
        return ws

    def _embed(self, rows: int, text_ids=None, text_pos=None, mel_ids=None, mel_pos=None, extra=None, extra_idx=None):
        # nn.Embedding raises IndexError on an out-of-range id (the reference's behaviour); the gather kernel would read past
        # its table instead, so the same check happens here, on the host index arrays, before anything is launched
        cfg = self.cfg
        for name, arr, hi in (("text token id", text_ids, cfg.number_text_tokens + 1), ("text position", text_pos, cfg.text_pos_len),
                              ("mel code", mel_ids, cfg.number_mel_codes), ("mel position", mel_pos, cfg.mel_pos_len),
                              ("conditioning row", extra_idx, 0 if extra is None else extra.shape[0])):
            if arr is not None and len(arr) and int(np.max(arr)) >= hi:
                raise IndexError(f"{name} {int(np.max(arr))} is out of range (table has {hi} rows)")
        out = torch.empty(rows, self.cfg.model_dim, device=self.device, dtype=torch.float32)
        idx = [None if a is None else _i32(self.device, a) for a in (text_ids, text_pos, mel_ids, mel_pos, extra_idx)]
        ex = None if extra is None else extra.to(self.device, torch.float32).contiguous()
        _lib.check(_lib.load().idxtts_gpt_embed(self._h, _lib.ptr(out), rows, _lib.ptr(idx[0]), _lib.ptr(idx[1]), _lib.ptr(idx[2]),
                                                _lib.ptr(idx[3]), _lib.ptr(ex), _lib.ptr(idx[4]), _lib.current_stream()))
        return out

    # ---- prompt conditioning (model_v2.py:627-671, 897-910): reference names and argument layouts ------------------
    def _need_cond(self):
        if self.cond is None:
            raise RuntimeError("this UnifiedVoice was built without conditioning_encoder / perceiver_encoder weights")
        return self.cond

    def get_conditioning(self, speech_conditioning_input: torch.Tensor, cond_mel_lengths=None, extents=None) -> torch.Tensor:
        """[B,1024,T] (transposed features, as model_v2.py:819 passes them) -> [B,32,d].  `extents` [B] (here and below): the frames each
        right-padded row holds, for a batch of several prompts in which every row computes what its own call computes (cond.py)."""
        return self._need_cond().get_conditioning(speech_conditioning_input, cond_mel_lengths, extents)

    def get_emovec(self, emo_speech_conditioning_latent: torch.Tensor, emo_cond_lengths=None, extents=None) -> torch.Tensor:
        return self._need_cond().get_emovec(emo_speech_conditioning_latent, emo_cond_lengths, extents)

    def merge_emovec(self, speech_conditioning_latent, emo_speech_conditioning_latent, cond_lengths=None, emo_cond_lengths=None, alpha=1.0,
                     extents=None, emo_extents=None):
        return self._need_cond().merge_emovec(speech_conditioning_latent, emo_speech_conditioning_latent, cond_lengths, emo_cond_lengths, alpha,
                                              extents, emo_extents)

    def conds_latent(self, speech_conditioning_latent: torch.Tensor, emo_vec: torch.Tensor) -> torch.Tensor:
        """cat(latent + emo_vec, speed_emb(1), speed_emb(0)) -> [B, 34, d]   (model_v2.py:830-834)."""
        lat = speech_conditioning_latent.to(self.device, torch.float32)
        ev = emo_vec.to(self.device, torch.float32)
        B = lat.shape[0]
        # One prompt is decoded many times (segments, batches, serving lanes): the sum is kept per (latent, emotion vector) storage so that
        # no torch elementwise kernel runs on a decode lane's stream per call (torch's own fp32 kernels beside bf16 MFMAs are
        # outside the NOPK build switch); a consumer on another stream waits for the event of the stream that produced the entry.
        # (keyed on storage address + torch's version counter: a write that bypasses the counter -- `.data.copy_`, a kernel or collective
        #  writing through the raw pointer -- is not seen; prompt conditioning tensors are built once and not written again)
        key = (lat.data_ptr(), lat._version, tuple(lat.shape), tuple(lat.stride()), ev.data_ptr(), ev._version, tuple(ev.shape), tuple(ev.stride()))
        cur = torch.cuda.current_stream(self.device)
        with self._conds_lock:      # decode lanes call this from several host threads
            hit = self._conds_cache.get(key)
        if hit is not None:
            cur.wait_event(hit[1])
            hit[0].record_stream(cur)      # allocated on the producer's stream, read on this one: not reused while a lane still reads it
            return hit[0]
        se = self.speed_emb
        conds = torch.cat([lat + ev[:, None, :], se[1].expand(B, 1, -1), se[0].expand(B, 1, -1)], dim=1).contiguous()
        done = torch.cuda.Event()
        done.record(cur)
        with self._conds_lock:
            if len(self._conds_cache) >= 16:
                self._conds_cache.pop(next(iter(self._conds_cache)), None)
            self._conds_cache[key] = (conds, done, lat.untyped_storage(), ev.untyped_storage())      # the storages are kept alive: a data_ptr is not reused
        return conds

    def prepare_gpt_inputs(self, conditional_latents: torch.Tensor, text_inputs: torch.Tensor):
        """model_v2.py:725-794 -> (fake_inputs [B,P+1], inputs_embeds [B,P,d] on the GPU, attention_mask [B,P+1])."""
        cfg = self.cfg
        text = text_inputs.detach().cpu().numpy().astype(np.int64)
        B, L = text.shape
        nc = conditional_latents.shape[1]
        single = conditional_latents.shape[0] == 1
        if not single and conditional_latents.shape[0] != B:
            raise AssertionError(f"batch size mismatch: {conditional_latents.shape[0]} vs {B}")
        P = nc + L + 2
        tid = -np.ones((B, P), np.int32)
        tpos = -np.ones((B, P), np.int32)
        eidx = -np.ones((B, P), np.int32)
        mask = np.ones((B, P + 1), np.int64)
        for i in range(B):
            ti = text[i]
            ti = ti[(ti != cfg.stop_text_token) & (ti != cfg.start_text_token)]
            ti = np.concatenate([[cfg.start_text_token], ti, [cfg.stop_text_token]])
            pad = L + 2 - len(ti)
            mask[i, :pad] = 0
            eidx[i, pad:pad + nc] = np.arange(nc) + (0 if single else i * nc)
            tid[i, pad + nc:] = ti
            tpos[i, pad + nc:] = np.arange(len(ti))
        extra = conditional_latents.reshape(-1, cfg.model_dim)
        emb = self._embed(B * P, text_ids=tid.reshape(-1), text_pos=tpos.reshape(-1), extra=extra, extra_idx=eidx.reshape(-1))
        fake = torch.ones(B, P + 1, dtype=torch.long)
        fake[:, -1] = cfg.start_mel_token
        return fake, emb.view(B, P, cfg.model_dim), torch.from_numpy(mask)

    def prompt_rows(self, conditional_latents: torch.Tensor, text_inputs: torch.Tensor):
        """prepare_gpt_inputs per row, without the left padding: a list of [P_b, d] prompt embeddings (what a decode session
        admits; generate() on a row with attention_mask=None sees the same prompt)."""
        _, emb, mask = self.prepare_gpt_inputs(conditional_latents, text_inputs)
        pads = (mask[:, :-1] == 0).sum(1).tolist()
        return [emb[i, int(p):] for i, p in enumerate(pads)]

    def decode_session(self, slots: int, max_prompt: int, max_new: int, repetition_penalty: float = 10.0, do_sample: bool = False,
                       num_beams: int = 1, use_graph: bool = True, sampled: bool = False, scores: bool = False,
                       prefix: bool = False, prefix_scores: bool = False) -> "DecodeSession":
        """Continuous batching: `slots` decode rows, one KV region each, that requests enter and leave between steps
        (DecodeSession; `idxtts_gpt_session_*`).  A request's codes equal row 0 of generate() on `slots` copies of its prompt.
        sampled=True: every request samples with its own parameters and draws (DecodeSession.admit(..., sampling=...)).
        scores=True: every code's log-probability is recorded (take(slot, scores=True); include/idxtts.h "Scores").
        prefix=True: rows may be admitted behind given codes (DecodeSession.admit(..., prefix=...)); the session's prefill area then
        holds at least one row of max_prompt + 1 + max_new positions.
        prefix_scores=True (with prefix=True and scores=True): admit(..., prefix_logprobs=[..., "model", ...]) lets the admission's own
        prefill score a request's prefix (include/idxtts.h "Scoring given codes")."""
        if do_sample:
            raise ValueError("decode sessions sample per request, not session-wide: do_sample=True is not supported; the session is "
                             "greedy unless created with sampled=True and given per-request parameters (admit(..., sampling=...))")
        if num_beams != 1:
            if prefix:
                raise ValueError("beams do not continue from given codes: prefix=True is for greedy and sampled sessions")
            raise ValueError("decode sessions are greedy or sampled per request: beam search runs in beam_session() (or generate_beam())")
        return DecodeSession(self, slots, max_prompt, max_new, repetition_penalty, use_graph, sampled=sampled, scores=scores, prefix=prefix,
                             prefix_scores=prefix_scores)

    def beam_session(self, slots: int, num_beams: int, max_prompt: int, max_new: int, repetition_penalty: float = 10.0,
                     use_graph: bool = True, scores: bool = False) -> "BeamDecodeSession":
        """Continuous batching of beam search / beam-sample: `slots` decode rows as slots / num_beams groups of num_beams, one request
        per group (BeamDecodeSession; `idxtts_gpt_session_*_beam`).  A request's codes equal row 0 of generate_beam() on
        slots / num_beams copies of its prompt.  scores=True raises: a beam session's hypotheses carry the scorer's scores
        (take(group, n_best=))."""
        if scores:
            raise ValueError("a beam session records no per-code scores: take(group, n_best=) returns the scorer's sequences_scores")
        return BeamDecodeSession(self, slots, num_beams, max_prompt, max_new, repetition_penalty, use_graph)

    # ------------------------------------------------------------------------------------------
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 100, temperature: float = 1.0, top_k: int = 50,
                 top_p: float = 1.0, stop_tokens=None, attention_mask: Optional[torch.Tensor] = None,
                 tts_embeddings: Optional[torch.Tensor] = None, tts_mel_embedding=None, tts_text_pos_embedding=None,
                 repetition_penalty: float = 10.0, return_logits: bool = False, use_graph: bool = True,
                 do_sample: bool = False, sampler: str = "hf", exp_noise: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None, forced_codes: Optional[torch.Tensor] = None,
                 seed: Optional[int] = None, num_return_sequences: int = 1, return_logprobs: bool = False,
                 prefix_layout: str = "hf") -> torch.Tensor:
        """The accel-engine plugin contract (accel_engine.py:378-645): returns LongTensor [B, P+1+generated]
        (prompt ids followed by the generated codes, padded with the stop token).

        input_ids may be [B, P+1+k]: k mel codes behind the start token, the reference's torch.cat([input_ids, input_tokens], 1)
        (model_v2.py:853; attention_mask may cover the extra columns).  Generation continues behind them and the result is
        [B, P+1+k+generated] = [input_ids | new codes], as HF returns it; max_new_tokens, exp_noise, logits and logprobs count the new
        codes.  The repetition penalty sees the given codes.  prefix_layout="hf" puts given code j at mel position j + 1, what the
        reference's first forward embeds (model_v2.py:163-165); "resume" puts it at j + 2, where an uninterrupted run fed it, so that
        the call goes on as that run would have (include/idxtts.h "Continuing from given codes").  A prefix that holds the stop token,
        or that leaves no room in the mel position table, raises; so does forced_codes together with a prefix.

        num_return_sequences=n > 1: n takes of every prompt, rows expanded as HF's _expand_inputs_for_generation does
        (repeat_interleave: row b * n + j is take j of prompt b); returns [B * n, P+1+generated].  exp_noise is then
        [max_new_tokens, B * n, V] and a seeded call draws the stream of row b * n + j of a B * n-row call, so the result equals generate
        on the caller-expanded batch wherever the two prefills choose the same kernels -- the prefill runs once per prompt, on B rows,
        and each row's keys and values are written to its n takes' cache rows (the `takes` of `idxtts_gpt_generate_prefix`, the one entry every non-forced form calls).  That holds always with
        an fp32 (or fp8) KV cache or in the batch-invariant mode; with a bf16 cache in split-bf16 GEMM mode when B * (P + 1) and
        B * n * (P + 1) lie on the same side of 256 prefill rows.

        do_sample=False: greedy (temperature / top_k / top_p ignored).  do_sample=True: multinomial sampling,
        sampler="hf" = HF `_sample` with its warpers (repetition penalty -> temperature -> top-k -> top-p -> multinomial,
        transformers_generation_utils.py:1036-1044, 3222-3250), sampler="accel" = the accel engine's own Sampler
        (softmax(logits / T) / Exp(1) noise, argmax; accel_engine.py:648-659).  torch.multinomial(probs, 1) is
        argmax(probs / q) with q ~ Exp(1): `exp_noise` [max_new_tokens, B, V] supplies the draws, or `generator` draws them on the
        CPU with one exponential_() per step, the order HF consumes them; with neither the kernels generate them from `seed` (see
        _noise; None = a seed drawn from torch's global RNG).
        forced_codes [B, max_new_tokens] (greedy only; a parity instrument, `idxtts_gpt_generate_forced`): the sequence is continued with
        these tokens while the returned codes are each step's own argmax -- with return_logits, the logits of a GIVEN token sequence.
        return_logprobs=True: also returns logprobs [rows, generated] fp32, the model's log-probability of every generated code under
        the raw logits (what return_logits records, log-softmaxed: HF's output_logits + compute_transition_scores(normalize_logits=True),
        not the processed output_scores; include/idxtts.h "Scores"); 0 on the pad steps of a row that has stopped.  The return value is
        (sequences, logprobs), with return_logits (sequences, logits, logprobs).  Every mode: greedy, forced, both samplers, takes.
        The codes are bit for bit those of the call without it."""
        if tts_embeddings is None:
            raise ValueError("tts_embeddings ([pad][cond][text] prompt embeddings) is required")
        if stop_tokens is not None and list(stop_tokens) != [self.cfg.stop_mel_token]:
            raise ValueError("stop_tokens must be [stop_mel_token]")
        emb = tts_embeddings.to(self.device, torch.float32).contiguous()
        nrs = int(num_return_sequences)
        if nrs < 1:
            raise ValueError("num_return_sequences must be >= 1")
        if nrs > 1:
            if forced_codes is not None:
                raise ValueError("forced_codes is a single-sequence instrument (num_return_sequences must be 1)")
        B, P, d = emb.shape
        if input_ids.dim() != 2 or input_ids.shape[0] != B or input_ids.shape[1] < P + 1:
            raise ValueError("input_ids must be [B, P+1] (fake prefix + start_mel_token), or [B, P+1+k] with k given mel codes behind it")
        k = int(input_ids.shape[1]) - (P + 1)
        if prefix_layout not in ("hf", "resume"):
            raise ValueError("prefix_layout must be 'hf' or 'resume'")
        prefix = None
        if k > 0:
            if forced_codes is not None:
                raise ValueError("forced_codes together with given codes in input_ids is not supported")
            if attention_mask is not None and attention_mask.shape[1] not in (P + 1, P + 1 + k):
                raise ValueError("attention_mask must cover [B, P+1] or [B, P+1+k]")
            if int((input_ids[:, P + 1:] == self.cfg.stop_mel_token).sum()) > 0:
                raise ValueError("the given codes contain the stop token: nothing follows a stop token")
            if int(input_ids[:, P + 1:].min()) < 0 or int(input_ids[:, P + 1:].max()) >= self.cfg.number_mel_codes:
                raise ValueError("the given codes must be mel codes (0 .. number_mel_codes - 1)")
            if k + int(max_new_tokens) + 1 >= self.cfg.mel_pos_len:
                raise ValueError("given codes + max_new_tokens exceed the mel position table")
            prefix = input_ids[:, P + 1:].to(self.device, torch.long).contiguous()      # one row per prompt: its takes share it
        pad_left = np.zeros(B, np.int32)      # one entry per prompt: the prefill runs on the B prompts, the takes share it
        if attention_mask is not None:
            am = attention_mask.detach().cpu().numpy()
            pad_left = (am[:, :P] == 0).sum(1).astype(np.int32)
        prompts, B = B, B * nrs               # from here on B counts decode rows (row b * n + j: take j of prompt b)
        if nrs > 1:
            input_ids = input_ids.repeat_interleave(nrs, dim=0)
        codes = torch.full((B, max_new_tokens), self.cfg.stop_mel_token, dtype=torch.long, device=self.device)
        V = self.cfg.number_mel_codes
        logits = torch.zeros(max_new_tokens, B, V, device=self.device) if return_logits else None
        logprobs = torch.zeros(B, max_new_tokens, device=self.device) if return_logprobs else None
        ws = self._workspace(B, P + 1 + k, max_new_tokens)
        n = ctypes.c_int(0)
        if do_sample and forced_codes is not None:
            raise ValueError("forced_codes is a greedy-mode instrument")
        sc = None
        if do_sample:
            if sampler not in ("hf", "accel"):
                raise ValueError("sampler must be 'hf' or 'accel'")
            noise, seed = self._noise(exp_noise, generator, (max_new_tokens, B, V), seed)
            sc = _sampling_c(sampler, temperature, top_k, top_p, noise, seed)
        # one argument list: (the call's own arguments go between `head` and `tail`)
        lib = _lib.load()
        head = (self._h, _lib.ptr(emb), pad_left.ctypes.data_as(c_void_p))
        tail = (_lib.ptr(logits), _lib.ptr(ws), ws.numel())
        if forced_codes is not None:      # the parity instrument keeps its own entries: they run without the step graph
            fc = forced_codes.to(self.device, torch.long).contiguous()
            if tuple(fc.shape) != (B, max_new_tokens):
                raise ValueError(f"forced_codes must be {(B, max_new_tokens)}")
            mid = (B, P, max_new_tokens, float(repetition_penalty), _lib.ptr(fc), _lib.ptr(codes), ctypes.byref(n))
            if return_logprobs:
                _lib.check(lib.idxtts_gpt_generate_forced_scored(*head, *mid, _lib.ptr(logprobs), *tail, _lib.current_stream()))
            else:
                _lib.check(lib.idxtts_gpt_generate_forced(*head, *mid, *tail, _lib.current_stream()))
        else:      # greedy (sampling NULL) and both samplers; takes, logprobs (NULL unless asked) and a prefix (NULL, k = 0 without one)
            _lib.check(lib.idxtts_gpt_generate_prefix(
                *head, prompts, nrs, P, max_new_tokens, float(repetition_penalty),
                ctypes.cast(ctypes.pointer(sc), c_void_p) if sc is not None else c_void_p(0), _lib.ptr(prefix), k,
                1 if prefix_layout == "hf" else 2, _lib.ptr(codes), ctypes.byref(n), _lib.ptr(logprobs), *tail, int(use_graph),
                _lib.current_stream()))
        out = torch.cat([input_ids.to(self.device), codes[:, : n.value]], dim=1)
        res = (out,)
        if return_logits:
            res += (logits[: n.value].permute(1, 0, 2).contiguous(),)
        if return_logprobs:
            res += (logprobs[:, : n.value].contiguous(),)
        return res if len(res) > 1 else out

    def score_codes(self, codes, tts_embeddings: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, code_lens=None,
                    layout: str = "resume", return_logits: bool = False):
        """The model's log-probability of every code of GIVEN sequences, from one prefill (`idxtts_gpt_score`; include/idxtts.h "Scoring
        given codes"): logprobs [B, n] fp32, what generate(return_logprobs=True) records for codes it emits itself, 0 from each row's
        length on.  codes [B, n] (a tensor, or a list of 1-D sequences, right-padded here); code_lens [B]: the codes each row holds
        (default: the list's lengths, else n).  A row's last code may be the stop token, no other.  tts_embeddings [B, P, d] and
        attention_mask as generate() takes them.  layout "resume": code j at mel position j + 2, where the run that emitted the codes fed
        them; "hf": at j + 1, the reference's first forward with input_tokens.  return_logits=True: (logprobs, logits [B, n, V]), the
        raw logits of every scored position.  No repetition penalty, temperature or warper enters.  sequence_scores / rank_takes take
        the result as they take a scored run's."""
        if layout not in ("hf", "resume"):
            raise ValueError("layout must be 'hf' or 'resume'")
        emb = tts_embeddings.to(self.device, torch.float32).contiguous()
        if emb.dim() != 3 or emb.shape[2] != self.cfg.model_dim:
            raise ValueError("tts_embeddings must be [B, P, d]")
        B, P, _ = emb.shape
        if not isinstance(codes, torch.Tensor):
            rows = [torch.as_tensor(np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r), dtype=torch.long).reshape(-1) for r in codes]
            if code_lens is None:
                code_lens = [int(r.numel()) for r in rows]
            codes = torch.zeros(len(rows), max([int(r.numel()) for r in rows] + [1]), dtype=torch.long)
            for i, r in enumerate(rows):
                codes[i, : r.numel()] = r
        if codes.dim() != 2 or codes.shape[0] != B or codes.shape[1] < 1:
            raise ValueError("codes must be [B, n] with n >= 1, one row per prompt")
        n = int(codes.shape[1])
        lens = None
        if code_lens is not None:
            lens = np.ascontiguousarray(np.asarray(code_lens, dtype=np.int64).reshape(-1).astype(np.int32))
            if lens.shape[0] != B:
                raise ValueError("code_lens must hold one length per row")
        pad_left = np.zeros(B, np.int32)
        if attention_mask is not None:
            pad_left = (attention_mask.detach().cpu().numpy()[:, :P] == 0).sum(1).astype(np.int32)
        dc = codes.to(self.device, torch.long).contiguous()
        V = self.cfg.number_mel_codes
        logprobs = torch.empty(B, n, device=self.device, dtype=torch.float32)
        logits = torch.empty(B, n, V, device=self.device, dtype=torch.float32) if return_logits else None
        lib = _lib.load()
        need = int(lib.idxtts_gpt_score_workspace_bytes(self._h, B, P, n))
        if need == 0:
            raise ValueError("score_codes: 1 <= B <= 64 rows of n >= 1 codes behind P >= 1 prompt positions")
        ws = self._workspace_bytes(need)
        _lib.check(lib.idxtts_gpt_score(self._h, _lib.ptr(emb), pad_left.ctypes.data_as(c_void_p), B, P, _lib.ptr(dc),
                                        lens.ctypes.data_as(c_void_p) if lens is not None else c_void_p(0), n, 1 if layout == "hf" else 2,
                                        _lib.ptr(logprobs), _lib.ptr(logits), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
        return (logprobs, logits) if return_logits else logprobs

    def _noise(self, exp_noise, generator, shape, seed: Optional[int] = None):
        """The Exp(1) draws of a sampled generation: (device tensor | None, seed).  An explicit `exp_noise`, or a torch `generator`
        (one exponential_() per step, the order HF consumes them: reproduces the reference's stream under that seed); with neither,
        the kernels draw from a counter-based generator keyed by a 63-bit seed taken from torch's global RNG (so torch.manual_seed
        still makes a run repeatable), or `seed` itself when given -- no [steps, B, V] tensor is materialised."""
        if exp_noise is None and generator is not None:
            exp_noise = torch.stack([torch.empty(shape[1:]).exponential_(1, generator=generator) for _ in range(shape[0])])
        return _draws(exp_noise, seed, shape, self.device)

    def generate_beam(self, input_ids: torch.Tensor, max_new_tokens: int, attention_mask: Optional[torch.Tensor], tts_embeddings: torch.Tensor,
                      num_beams: int = 3, do_sample: bool = True, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                      repetition_penalty: float = 1.0, length_penalty: float = 1.0, early_stopping: bool = False,
                      exp_noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, use_graph: bool = True,
                      seed: Optional[int] = None, num_return_sequences: int = 1, return_scores: bool = False):
        """HF `generate(num_beams > 1)` of the reference (model_v2.py:885-889 -> transformers_generation_utils.py:3325-3516):
        beam search, or beam-sample when do_sample.  Returns LongTensor [B, P+1+n]: the best hypothesis per utterance.
        num_return_sequences=n (1 <= n <= num_beams): the scorer's n best hypotheses of every utterance, best first (row b * n + j;
        BeamSearchScorer.finalize's order: of equal scores the one added later first) -- for n > 1, or with return_scores, the result is
        (sequences [B * n, P+1+L], sequences_scores fp32 [B * n]); row b * n of it is bit for bit row b of the n = 1 call.
        Sampling draws 2 * num_beams candidates per utterance without replacement: torch.multinomial == top-k of probs / q with
        q ~ Exp(1) from one exponential_() per step on a [B, num_beams * V] tensor -- `exp_noise` [max_new_tokens, B, num_beams*V]
        supplies them, or `generator` draws them on the CPU in that order; with neither the kernels generate them from `seed` (see _noise)."""
        emb = tts_embeddings.to(self.device, torch.float32).contiguous()
        B, P, d = emb.shape
        if input_ids.dim() == 2 and input_ids.shape[0] == B and input_ids.shape[1] > P + 1:
            raise NotImplementedError("beam search does not continue from given codes (input_ids wider than [B, P+1]): HF's length "
                                      "penalty counts the prefix and the scorer's rows would have to hold it; use generate()")
        if input_ids.shape != (B, P + 1):
            raise ValueError("input_ids must be [B, P+1] (fake prefix + start_mel_token)")
        if not (2 <= int(num_beams) <= 8) or B * int(num_beams) > 64:
            raise ValueError("2 <= num_beams <= 8 and B * num_beams <= 64")
        if early_stopping not in (False, True):
            raise NotImplementedError('early_stopping="never" is not implemented')
        pad_left = np.zeros(B, np.int32)
        if attention_mask is not None:
            pad_left = (attention_mask.detach().cpu().numpy()[:, :P] == 0).sum(1).astype(np.int32)
        V, nb = self.cfg.number_mel_codes, int(num_beams)
        noise, seed = self._noise(exp_noise, generator, (max_new_tokens, B, nb * V), seed) if do_sample else (None, 0)
        lib = _lib.load()
        need = int(lib.idxtts_gpt_beam_workspace_bytes(self._h, B, nb, P + 1, max_new_tokens))
        if need == 0:
            raise RuntimeError("idxtts_gpt_beam_workspace_bytes returned 0")
        ws = self._workspace_bytes(need)
        nrs = int(num_return_sequences)
        if not 1 <= nrs <= nb:
            raise ValueError("1 <= num_return_sequences <= num_beams")
        codes = torch.full((B * nrs, max_new_tokens), self.cfg.stop_mel_token, dtype=torch.long, device=self.device)
        bc = _lib.BeamC(num_beams=nb, do_sample=int(bool(do_sample)), temperature=float(temperature), top_k=int(top_k or 0),
                        top_p=float(top_p if top_p is not None else 1.0), length_penalty=float(length_penalty),
                        early_stopping=int(bool(early_stopping)), exp_noise=noise.data_ptr() if noise is not None else None, seed=seed)
        n = ctypes.c_int(0)
        if nrs == 1 and not return_scores:
            _lib.check(lib.idxtts_gpt_generate_beam(self._h, _lib.ptr(emb), pad_left.ctypes.data_as(c_void_p), B, P, max_new_tokens,
                                                    float(repetition_penalty), ctypes.byref(bc), _lib.ptr(codes), ctypes.byref(n), _lib.ptr(ws),
                                                    ws.numel(), int(use_graph), _lib.current_stream()))
            return torch.cat([input_ids.to(self.device), codes[:, : n.value]], dim=1)
        lens, scores = np.zeros(B * nrs, np.int32), np.zeros(B * nrs, np.float32)
        _lib.check(lib.idxtts_gpt_generate_beam_nbest(
            self._h, _lib.ptr(emb), pad_left.ctypes.data_as(c_void_p), B, P, max_new_tokens, float(repetition_penalty), ctypes.byref(bc), nrs,
            _lib.ptr(codes), lens.ctypes.data_as(c_void_p), scores.ctypes.data_as(c_void_p), ctypes.byref(n), _lib.ptr(ws), ws.numel(),
            int(use_graph), _lib.current_stream()))
        seqs = torch.cat([input_ids.to(self.device).repeat_interleave(nrs, dim=0), codes[:, : n.value]], dim=1)
        return seqs, torch.from_numpy(scores).to(self.device)

    def inference_speech(self, speech_condition, text_inputs, emo_speech_condition=None, cond_lengths=None, emo_cond_lengths=None,
                         emo_vec=None, use_speed=False, input_tokens=None, num_return_sequences=1, max_generate_length=None,
                         typical_sampling=False, typical_mass=.9, return_logits=False, return_logprobs=False, **hf_generate_kwargs):
        """`inference_speech` (model_v2.py:796-895): returns (codes [B, n], speech_conditioning_latent).
        speech_condition: the prompt features [B, T, 1024] as the reference takes them (conditioning encoders run here, model_v2.py:
        819-828) or -- hoisted out of the caller's segment loop -- the ready conditioning latent [B, 32, d] together with `emo_vec`.
        Decoding modes = HF generate's: greedy (do_sample=False, num_beams=1), multinomial sampling with the warpers
        (do_sample=True, num_beams=1; extra kwargs `exp_noise` / `generator` / `sampler`, see generate()), beam search and
        beam-sample (num_beams > 1: generate_beam()).  input_tokens ((s,) or (1, s) mel codes, one utterance, num_return_sequences=1):
        generation continues behind them in the reference's position layout (generate(prefix_layout="hf")); the returned codes are the
        new ones, as the reference truncates at trunc_index.  num_return_sequences=n: codes [B * n, L], row b * n + j take j of utterance b --
        n sampled takes (generate()), or the n best beam hypotheses (n <= num_beams), as HF's generate returns them.
        return_logprobs (num_beams = 1): the log-probability of every code, [rows, n] fp32 (generate(return_logprobs=True)), as one more
        value at the end of the returned tuple."""
        if typical_sampling or use_speed:
            raise NotImplementedError("typical_sampling / use_speed are not used by IndexTTS2.infer and not implemented")
        nrs = int(num_return_sequences)
        if nrs < 1:
            raise ValueError("num_return_sequences must be >= 1")
        if input_tokens is not None:
            if nrs > 1:
                raise NotImplementedError("input_tokens with num_return_sequences > 1 is not implemented: the reference repeats the rows "
                                          "itself (model_v2.py:847-852) and HF's generate then expands them a second time")
            input_tokens = torch.as_tensor(input_tokens)
            if input_tokens.ndim == 1:
                input_tokens = input_tokens.unsqueeze(0)
            # the reference's asserts (model_v2.py:843-846) at num_return_sequences = 1: both batches must divide 1
            assert nrs % input_tokens.shape[0] == 0, "The num_return_sequences must be divisible by the batch number of input_tokens"
            assert nrs % text_inputs.shape[0] == 0, "The num_return_sequences must be divisible by the batch number of text_inputs"
        sc = speech_condition if speech_condition.ndim == 3 else speech_condition.unsqueeze(0)
        if sc.shape[-1] == self.cfg.cond_module.input_size and sc.shape[-1] != self.cfg.model_dim:      # raw features
            if emo_speech_condition is None:
                emo_speech_condition = sc
            speech_conditioning_latent = self.get_conditioning(sc.transpose(1, 2), cond_lengths)
            if emo_vec is None:
                emo_vec = self.get_emovec(emo_speech_condition, emo_cond_lengths)                      # model_v2.py:823-826
        else:
            speech_conditioning_latent = sc
            if emo_vec is None:
                raise ValueError("pass emo_vec together with a ready conditioning latent")
        do_sample = bool(hf_generate_kwargs.pop("do_sample", False))
        num_beams = int(hf_generate_kwargs.pop("num_beams", 1))
        penalty = float(hf_generate_kwargs.pop("repetition_penalty", 1.0))
        samp = {"do_sample": do_sample, "top_p": hf_generate_kwargs.pop("top_p", 1.0), "top_k": hf_generate_kwargs.pop("top_k", 50),
                "temperature": hf_generate_kwargs.pop("temperature", 1.0), "exp_noise": hf_generate_kwargs.pop("exp_noise", None),
                "generator": hf_generate_kwargs.pop("generator", None)}
        forced_codes = hf_generate_kwargs.pop("forced_codes", None)
        sampler = hf_generate_kwargs.pop("sampler", "hf")
        length_penalty = float(hf_generate_kwargs.pop("length_penalty", 1.0))
        early_stopping = hf_generate_kwargs.pop("early_stopping", False)
        use_graph = bool(hf_generate_kwargs.pop("use_graph", True))
        if hf_generate_kwargs:
            raise TypeError(f"unsupported generate kwargs: {sorted(hf_generate_kwargs)}")
        B = text_inputs.shape[0]
        lat = speech_conditioning_latent.expand(B, -1, -1) if speech_conditioning_latent.shape[0] == 1 else speech_conditioning_latent
        ev = emo_vec.expand(B, -1) if emo_vec.shape[0] == 1 else emo_vec
        conds = self.conds_latent(lat, ev)
        input_ids, inputs_embeds, attention_mask = self.prepare_gpt_inputs(conds, text_inputs)
        if input_tokens is not None:      # model_v2.py:853-855: the codes behind input_ids, the mask extended with ones
            if num_beams > 1:
                raise NotImplementedError("input_tokens with num_beams > 1 is not implemented (beams do not continue from given codes)")
            tok = input_tokens.to(input_ids.device, torch.long)
            input_ids = torch.cat([input_ids, tok], dim=1)
            attention_mask = torch.nn.functional.pad(attention_mask, (0, tok.shape[1]), value=1)
        trunc_index = input_ids.shape[1]
        max_new = (self.cfg.max_mel_tokens - 1) if max_generate_length is None else int(max_generate_length)
        if num_beams > 1:
            if return_logits or return_logprobs:
                raise NotImplementedError("return_logits / return_logprobs are num_beams=1 features (generate_beam(return_scores=True) "
                                          "returns the scorer's sequence scores)")
            out = self.generate_beam(input_ids, max_new, attention_mask, inputs_embeds, num_beams=num_beams, repetition_penalty=penalty,
                                     length_penalty=length_penalty, early_stopping=early_stopping, use_graph=use_graph,
                                     num_return_sequences=nrs, **samp)
            out = out[0] if nrs > 1 else out
            return out[:, trunc_index:], speech_conditioning_latent
        if nrs > 1 and return_logits:
            raise NotImplementedError("return_logits is a num_return_sequences=1 feature")
        out = self.generate(input_ids, max_new_tokens=max_new, stop_tokens=[self.cfg.stop_mel_token],
                            attention_mask=attention_mask, tts_embeddings=inputs_embeds, repetition_penalty=penalty,
                            return_logits=return_logits, sampler=sampler, use_graph=use_graph, forced_codes=forced_codes,
                            num_return_sequences=nrs, return_logprobs=return_logprobs, **samp)
        if return_logits or return_logprobs:
            return (out[0][:, trunc_index:], speech_conditioning_latent) + tuple(out[1:])
        return out[:, trunc_index:], speech_conditioning_latent

    # ------------------------------------------------------------------------------------------
    def forward(self, speech_conditioning_latent, text_inputs, text_lengths, mel_codes, mel_codes_lengths,
                emo_speech_conditioning_latent=None, cond_mel_lengths=None, emo_cond_mel_lengths=None, emo_vec=None,
                use_speed=None, do_spk_cond=False) -> torch.Tensor:
        """Latent pass (model_v2.py:673-723) -> [B, M, d]."""
        if do_spk_cond or emo_vec is None:
            raise NotImplementedError("conditioning encoders are outside this hot path: pass the latent and emo_vec")
        cfg = self.cfg
        text = text_inputs.detach().cpu().numpy().astype(np.int64).copy()
        codes = mel_codes.detach().cpu().numpy().astype(np.int64).copy()
        B, L = text.shape
        M = codes.shape[1]
        tl = np.asarray(text_lengths.detach().cpu() if isinstance(text_lengths, torch.Tensor) else text_lengths).reshape(-1)
        ml = np.asarray(mel_codes_lengths.detach().cpu() if isinstance(mel_codes_lengths, torch.Tensor) else mel_codes_lengths).reshape(-1)
        tlv = [int(tl[min(b, len(tl) - 1)]) for b in range(B)]
        mlv = [int(ml[min(b, len(ml) - 1)]) for b in range(B)]
        for b in range(B):      # set_mel_padding (model_v2.py:569-581)
            codes[b, mlv[b]:] = cfg.stop_mel_token
        min_ = np.concatenate([np.full((B, 1), cfg.start_mel_token), codes, np.full((B, 1), cfg.stop_mel_token)], 1)
        conds = self.conds_latent(speech_conditioning_latent, emo_vec)
        nc = conds.shape[1]
        S = nc + L + 2 + M + 2
        tid = -np.ones((B, S), np.int32); tpos = -np.ones((B, S), np.int32)
        mid = -np.ones((B, S), np.int32); mpos = -np.ones((B, S), np.int32)
        eidx = -np.ones((B, S), np.int32)
        pad_left = np.zeros(B, np.int32)
        for b in range(B):
            # row layout [pad][conds][start, text_b, stop][start, codes, stop, stop]; a row whose text is shorter than L is
            # LEFT-padded (and the pad masked), which reproduces the reference's unpadded B=1 call for that row
            pad = L - tlv[b]
            pad_left[b] = pad
            trow = np.concatenate([[cfg.start_text_token], text[b, :tlv[b]], [cfg.stop_text_token]])
            eidx[b, pad:pad + nc] = np.arange(nc) + b * nc
            tid[b, pad + nc:nc + L + 2] = trow
            tpos[b, pad + nc:nc + L + 2] = np.arange(tlv[b] + 2)
            mid[b, nc + L + 2:] = min_[b]
            mpos[b, nc + L + 2:] = np.arange(M + 2)
        emb = self._embed(B * S, tid.reshape(-1), tpos.reshape(-1), mid.reshape(-1), mpos.reshape(-1),
                          conds.reshape(-1, cfg.model_dim), eidx.reshape(-1))
        latent = torch.empty(B, M, cfg.model_dim, device=self.device, dtype=torch.float32)
        ws = self._workspace(B, S, 0)
        pl = pad_left.ctypes.data_as(c_void_p) if pad_left.any() else c_void_p(0)
        _lib.check(_lib.load().idxtts_gpt_latent(self._h, _lib.ptr(emb), pl, B, S, nc + L + 2, M, _lib.ptr(latent), _lib.ptr(ws),
                                                 ws.numel(), _lib.current_stream()))
        return latent

    __call__ = forward

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().idxtts_ctx_destroy(self._h)
        except Exception:
            pass


def sequence_scores(logprobs, lengths, length_penalty: float = 1.0) -> np.ndarray:
    """Sequence score of every row: (sum_{t < n} lp[t]) / n ** length_penalty with n = lengths[row], the codes the row produced (the
    stop token included) -- HF's sum_logprobs / len ** length_penalty.  logprobs: [rows, steps] (tensor or array; or a list of 1-D rows),
    the fp32 values generate(return_logprobs=True) / take(scores=True) return; summed on the host in float64, in index order.
    Returns float64 [rows]."""
    rows = [np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float32) for r in logprobs]
    lengths = [int(n) for n in lengths]
    if len(rows) != len(lengths):
        raise ValueError("one length per row")
    out = np.zeros(len(rows), np.float64)
    for i, (r, n) in enumerate(zip(rows, lengths)):
        if r.ndim != 1 or not 1 <= n <= r.shape[0]:
            raise ValueError(f"row {i}: length {n} outside 1 .. {r.shape[0] if r.ndim == 1 else '?'}")
        tot = 0.0
        for t in range(n):      # index order, float64
            tot += float(r[t])
        out[i] = tot / float(n) ** float(length_penalty)
    return out


def rank_takes(scores, stopped) -> list:
    """The takes of one utterance, best first: a take that stopped (its last code is the stop token) before every take that ran into its
    cap, then the higher score, then the lower take index.  Returns the take indices in that order."""
    scores = [float(x) for x in scores]
    stopped = [bool(x) for x in stopped]
    if len(scores) != len(stopped):
        raise ValueError("one stopped flag per score")
    return sorted(range(len(scores)), key=lambda j: (not stopped[j], -scores[j], j))


def _seed64(seed) -> int:
    s = int(seed)
    if not 0 <= s < 2 ** 64:
        raise ValueError("seed must be in 0 .. 2**64 - 1")
    return s


def _draws(exp_noise, seed, shape, device, dims: str = ""):
    """The one rule for a row's Exp(1) draws -> (device tensor | None, seed): an explicit `exp_noise` of `shape` (the seed is then 0), else
    `seed`, else a 62-bit seed taken from torch's global RNG (one randint per unseeded row, in the order the rows are stated, so that
    torch.manual_seed makes a run repeatable).  dims: how the message of a wrong shape names the dimensions."""
    if exp_noise is not None:
        noise = torch.as_tensor(exp_noise)
        if tuple(noise.shape) != tuple(shape):
            raise ValueError(f"exp_noise must be {dims}{tuple(shape)}")
        return noise.to(device, torch.float32).contiguous(), 0
    return None, int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else _seed64(seed)


def _sampling_c(sampler: str, temperature=1.0, top_k=0, top_p=1.0, noise=None, seed: int = 0) -> "_lib.SamplingC":
    """idxtts_sampling of one row: "greedy", or "hf" / "accel" with their parameters (top_k / top_p are the HF sampler's) and draws."""
    if sampler == "greedy":
        return _lib.SamplingC(mode=0, temperature=1.0, top_k=0, top_p=1.0, exp_noise=None, seed=0)
    hf = sampler == "hf"
    return _lib.SamplingC(mode=1 if hf else 2, temperature=float(temperature), top_k=int(top_k or 0) if hf else 0,
                          top_p=float(top_p if top_p is not None else 1.0) if hf else 1.0,
                          exp_noise=noise.data_ptr() if noise is not None else None, seed=seed)


def check_sampling(temperature: float, top_k: int, top_p: float, warpers: bool = True, beam: bool = False) -> None:
    """The ranges of a sampled row's parameters, ValueError outside them: a positive temperature and, where the HF warpers run
    (`warpers`: not for sampler="accel"), top_k >= 0 -- a beam scorer's rows (`beam`) hold at most 1024 candidates, so there top_k <=
    1024 always -- top_p > 0, and top_p < 1 only with 0 < top_k <= 1024 (the nucleus is cut from the top-k candidates)."""
    if not temperature > 0.0:
        raise ValueError(f"{'beam-sample' if beam else 'sampling'} needs a positive temperature")
    if not warpers:
        return
    if top_k < 0 or (beam and top_k > 1024) or not top_p > 0.0:
        raise ValueError("top_k must be in 0 .. 1024 and top_p > 0" if beam else "top_k must be >= 0 and top_p > 0")
    if top_p < 1.0 and not 0 < top_k <= 1024:
        raise ValueError("top_p < 1 needs 0 < top_k <= 1024")


# How check_prefix words a refusal, by the name its caller knows the codes under (DecodeSession.admit's argument, the pipeline's
# submit argument): whose entry it is, the verb, and what a prefix that leaves no room under the cap is told
_PREFIX_WORDS = {"prefix": ("request", "contains", "prefix of {k} codes but a cap of {cap}: the cap counts prefix + new codes (k < cap)"),
                 "prefix_codes": ("utterance", "contain", "prefix_codes must be shorter than max_mel_tokens, which caps prefix + continuation")}


def check_prefix(codes, logprobs, cfg, cap: int, label: str = "prefix"):
    """Given codes a row is to continue from, and their log-probabilities if any -> (codes, logprobs) as CPU tensors (long; fp32 or
    None).  ValueError unless the codes are a 1-D sequence of mel codes without the stop token, shorter than `cap` (which counts given +
    new codes), and the log-probabilities are one value per code.  label: what the messages call the codes (_PREFIX_WORDS)."""
    per, verb, too_long = _PREFIX_WORDS[label]
    c = torch.as_tensor(codes).detach().to("cpu", torch.long)
    if c.dim() != 1:
        raise ValueError(f"{label}: a 1-D sequence of mel codes (or None) per {per}")
    k = int(c.numel())
    if k and (int(c.min()) < 0 or int(c.max()) >= cfg.number_mel_codes):
        raise ValueError(f"{label}: mel codes are 0 .. {cfg.number_mel_codes - 1}")
    if k and bool((c == cfg.stop_mel_token).any()):
        raise ValueError(f"{label} {verb} the stop token: nothing follows a stop token")
    if k >= cap:
        raise ValueError(too_long.format(k=k, cap=cap))
    if logprobs is not None:
        logprobs = torch.as_tensor(logprobs).detach().to("cpu", torch.float32)
        if tuple(logprobs.shape) != (k,):
            raise ValueError("prefix_logprobs: one value per prefix code")
    return c, logprobs


class ParkedRow:
    """A decode row that stepped aside (DecodeSession.park): the parked row's bytes (include/idxtts.h "Preempt and resume") on the
    device or, after to("cpu"), in pinned host memory; `n_codes` codes produced so far, the request's `cap`, and the request's
    exp_noise tensor if it has one (kept alive here while the row is parked).  DecodeSession.resume takes it once."""

    def __init__(self, blob: torch.Tensor, n_codes: int, cap: int, noise, stream):
        self._blob, self.n_codes, self.cap, self._noise, self._stream = blob, int(n_codes), int(cap), noise, stream

    @property
    def device(self) -> torch.device:
        self._check()
        return self._blob.device

    @property
    def nbytes(self) -> int:
        self._check()
        return int(self._blob.numel())

    @property
    def resumed(self) -> bool:
        return self._blob is None

    def _check(self) -> None:
        if self._blob is None:
            raise RuntimeError("this ParkedRow has been resumed: a parked row is resumed once")

    def to(self, device) -> "ParkedRow":
        """Moves the bytes IN PLACE (through pinned host memory) and returns self: to("cpu") gives the device memory back, to(a GPU)
        stages it again.  The copy runs on the stream the row was written on and is complete on return."""
        self._check()
        device = torch.device(device)
        if device.type == self._blob.device.type and (device.index is None or device == self._blob.device):
            return self
        if device.type == "cpu":
            host = torch.empty(self._blob.numel(), dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(self._stream):
                host.copy_(self._blob, non_blocking=True)
            self._stream.synchronize()
            self._blob = host
        elif device.type == "cuda":
            host = self._blob if self._blob.is_pinned() else self._blob.pin_memory()
            stream = torch.cuda.current_stream(device)
            with torch.cuda.stream(stream):
                dev = torch.empty(host.numel(), dtype=torch.uint8, device=device)
                dev.copy_(host, non_blocking=True)
            stream.synchronize()      # the pinned buffer is let go below
            self._blob, self._stream = dev, stream
        else:
            raise ValueError(f"a ParkedRow lives on the GPU or in host memory, not on {device}")
        return self


class ParkedGroup(ParkedRow):
    """A beam group that stepped aside (BeamDecodeSession.park_group): a ParkedRow whose bytes are a parked group (include/idxtts.h
    "Preempt and resume, beam sessions").  `n_codes` is the tokens each beam holds, `hyp_n` the finished hypotheses the scorer carried,
    `header` a copy of the blob's idxtts_park_group_header.  BeamDecodeSession.resume_group takes it once; DecodeSession.resume
    refuses it, as resume_group refuses a ParkedRow."""

    def __init__(self, blob: torch.Tensor, header, noise, stream):
        super().__init__(blob, header.step, header.max_step, noise, stream)
        self.header, self.num_beams, self.hyp_n = header, int(header.num_beams), int(header.hyp_n)


class _Session:
    """What DecodeSession and BeamDecodeSession share: the stream, the workspace and its native session, prompt staging, the step loop
    and the release.  Subclasses set the slot bookkeeping (_busy, _done, _noise) and _unit (slots per request)."""
    _unit = 1

    def __init__(self, gpt: UnifiedVoice, slots: int, max_prompt: int, max_new: int, use_graph: bool, need: int, init):
        self.gpt = gpt
        self.slots, self.max_prompt, self.max_new = int(slots), int(max_prompt), int(max_new)
        self.use_graph = bool(use_graph)
        self._lib = _lib.load()
        self.stream = torch.cuda.current_stream(gpt.device)
        if self.stream.cuda_stream == 0:        # the legacy default stream cannot be captured: a stream of the session's own
            self.stream = torch.cuda.Stream(device=gpt.device)
            self.stream.wait_stream(torch.cuda.current_stream(gpt.device))
        with torch.cuda.stream(self.stream):
            self._ws = torch.empty(need, dtype=torch.uint8, device=gpt.device)
            _lib.check(init(_lib.ptr(self._ws), need, self._sp()))
        n = self.slots // self._unit
        self._busy = [False] * n
        self._noise = {}          # request index (slot or group) -> the exp_noise tensor it reads (kept alive until take())
        self._done = set()

    def _sp(self) -> c_void_p:
        return c_void_p(self.stream.cuda_stream)

    @property
    def _what(self) -> str:
        return "slot" if self._unit == 1 else "group"

    def _free(self):
        return [i for i, b in enumerate(self._busy) if not b]

    def _live(self):
        return [i for i, b in enumerate(self._busy) if b and i not in self._done]

    def _stage(self, inputs_embeds_rows, max_new_each, free):
        """Checks and stages the admitted prompts: (rows, plen, caps, emb [n, P_max, d]) -- emb on the session stream."""
        rows = [r.to(self.gpt.device, torch.float32) for r in inputs_embeds_rows]
        n = len(rows)
        caps = [int(max_new_each)] * n if isinstance(max_new_each, int) else [int(c) for c in max_new_each]
        if len(caps) != n:
            raise ValueError("one cap per row")
        if n > len(free):
            raise RuntimeError(f"{n} rows but {len(free)} free {self._what}s")
        d = self.gpt.cfg.model_dim
        plen = [int(r.shape[0]) for r in rows]
        for r, p, c in zip(rows, plen, caps):
            if r.dim() != 2 or r.shape[1] != d or not 1 <= p <= self.max_prompt:
                raise ValueError(f"a prompt row must be [P, {d}] with 1 <= P <= {self.max_prompt}")
            if not 1 <= c <= self.max_new:
                raise ValueError(f"caps must be in 1 .. {self.max_new}")
        return rows, plen, caps

    def _embed_rows(self, rows, plen):
        pm = max(plen)
        emb = torch.zeros(len(rows), pm, self.gpt.cfg.model_dim, device=self.gpt.device, dtype=torch.float32)
        for i, r in enumerate(rows):
            emb[i, : plen[i]] = r
        return emb, pm

    def step(self, n: int = 1) -> list:
        """n decode steps of every live request; returns every request (slot, or group) that has finished and is not taken yet."""
        fin = np.zeros(self.slots, np.int32)
        nf = ctypes.c_int(0)
        steps = int(n) if self._live() else 0
        _lib.check(self._lib.idxtts_gpt_session_step(self.gpt._h, steps, int(self.use_graph), fin.ctypes.data_as(c_void_p),
                                                     ctypes.byref(nf), _lib.ptr(self._ws), self._sp()))
        done = [int(x) // self._unit for x in fin[: nf.value]]
        self._done.update(done)
        return done

    def take(self, i: int, scores: bool = False):
        """The codes of the finished request `i` (a slot, or a group) as a LongTensor on the device; `i` is free again.
        scores=True (a session created with scores=True): (codes, logprobs fp32 of the same length)."""
        n = ctypes.c_int(0)
        self.stream.wait_stream(torch.cuda.current_stream(self.gpt.device))
        with torch.cuda.stream(self.stream):
            out = torch.empty(self.max_new, dtype=torch.long, device=self.gpt.device)
            if scores:
                lp = torch.empty(self.max_new, dtype=torch.float32, device=self.gpt.device)
                _lib.check(self._lib.idxtts_gpt_session_read_scored(self.gpt._h, int(i) * self._unit, _lib.ptr(out), _lib.ptr(lp),
                                                                    ctypes.byref(n), _lib.ptr(self._ws), self._sp()))
            else:
                _lib.check(self._lib.idxtts_gpt_session_read(self.gpt._h, int(i) * self._unit, _lib.ptr(out), ctypes.byref(n),
                                                             _lib.ptr(self._ws), self._sp()))
        self._vacate(i, record=False)
        return (out[: n.value], lp[: n.value]) if scores else out[: n.value]

    def _held(self, i) -> int:
        """The id of a request this session holds (admitted and not taken), as an int; ValueError otherwise."""
        if not isinstance(i, (int, np.integer)) or not 0 <= int(i) < len(self._busy) or not self._busy[int(i)]:
            raise ValueError(f"{i!r} holds no request ({self._what} ids 0 .. {len(self._busy) - 1})")
        return int(i)

    def _ids(self, ids) -> list:
        """One id or a list of them -> a list of requests this session holds; ValueError otherwise."""
        return [self._held(i) for i in ([ids] if isinstance(ids, (int, np.integer)) else list(ids))]

    def _occupy(self, ids, noises) -> None:
        """The places `ids` hold requests now; a request's exp_noise tensor is kept alive while it reads it."""
        for i, nz in zip(ids, noises):
            self._busy[i] = True
            if nz is not None:
                self._noise[i] = nz

    def _vacate(self, i: int, record: bool):
        """The place `i` is free again; returns its request's draws.  record: they are let go (or move on) with a launch that ends the
        request's reads on the session's stream -- evict, park -- and not after a read that has synchronised, as take has."""
        self._busy[i] = False
        self._done.discard(i)
        nz = self._noise.pop(i, None)
        if record and nz is not None:
            nz.record_stream(self.stream)
        return nz

    def _end(self, fn, ids: list) -> None:
        h = np.ascontiguousarray([i * self._unit for i in ids], dtype=np.int32)
        _lib.check(fn(self.gpt._h, len(ids), h.ctypes.data_as(c_void_p), _lib.ptr(self._ws), self._sp()))

    def evict(self, ids) -> None:
        """Ends the requests `ids` (one id or a list: slots, or groups) and frees them now: live ones and ones that have finished and
        were not taken.  Their places are admissible at once, step() never reports them and take() on them raises.  One launch on the
        session's stream, no synchronisation; every other request's codes are untouched.  A bad id raises ValueError, nothing changes."""
        ids = self._ids(ids)
        if not ids:
            return
        self._end(self._lib.idxtts_gpt_session_evict, ids)
        for i in ids:       # as take(); a request's draws are let go only now, with the launch that ends its reads on the stream
            self._vacate(i, record=True)

    def stop(self, ids) -> None:
        """Ends the live requests among `ids` and keeps them: the next step() (step(0) too) reports them and take() returns the k
        codes produced so far -- bit for bit what the same request with cap k returns (a beam group: generate_beam with
        max_new_tokens = k).  A request that has already finished is left alone.  A bad id raises ValueError, nothing changes."""
        ids = self._ids(ids)
        if ids:
            self._end(self._lib.idxtts_gpt_session_stop, ids)

    def _take_out(self, i: int, bytes_fn, park_fn, header_t):
        """Park the request in place `i` (a slot, or a group): size, allocate, gather, read the header, free the place.  Returns
        (blob, header, the request's draws -- they move with it: alive while it is parked)."""
        with torch.cuda.stream(self.stream):
            need = int(bytes_fn(self.gpt._h, i, _lib.ptr(self._ws), self._sp()))
            if need == 0:
                _lib.check(1)
            blob = torch.empty(need, dtype=torch.uint8, device=self.gpt.device)
            written = ctypes.c_size_t(0)
            _lib.check(park_fn(self.gpt._h, i, _lib.ptr(blob), need, ctypes.byref(written), _lib.ptr(self._ws), self._sp()))
            hdr = header_t.from_buffer_copy(blob[: ctypes.sizeof(header_t)].cpu().numpy().tobytes())
        assert written.value == need == hdr.bytes
        return blob, hdr, self._vacate(i, record=True)

    def _put_back(self, parked: ParkedRow, i, resume_fn) -> int:
        """Resume `parked` into place `i` (default: the first free one): stage, wait, scatter, occupy, consume.  Returns the place."""
        parked._check()
        if i is None:
            free = self._free()
            if not free:
                raise RuntimeError(f"no free {self._what}")
            i = free[0]
        if not isinstance(i, (int, np.integer)) or not 0 <= int(i) < len(self._busy):
            raise ValueError(f"{self._what} {i!r} out of range (0 .. {len(self._busy) - 1})")
        i = int(i)
        if self._busy[i]:
            raise ValueError(f"{self._what} {i} is not free")
        if parked._blob.device != self.gpt.device:
            with torch.cuda.stream(self.stream):
                parked.to(self.gpt.device)
        blob = parked._blob
        self.stream.wait_stream(parked._stream)      # it may have been written on another session's stream
        with torch.cuda.stream(self.stream):
            _lib.check(resume_fn(self.gpt._h, i, _lib.ptr(blob), blob.numel(), _lib.ptr(self._ws), self._sp()))
        blob.record_stream(self.stream)
        if parked._noise is not None:
            parked._noise.record_stream(self.stream)
        self._occupy([i], [parked._noise])
        parked._blob = parked._noise = None
        return i

    def close(self) -> None:
        if getattr(self, "_ws", None) is not None:
            self.stream.synchronize()
            self._lib.idxtts_gpt_session_release(self.gpt._h, _lib.ptr(self._ws))
            self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodeSession(_Session):
    """A fixed set of greedy decode rows ("slots") with one KV region each, on one HIP stream (the current stream at creation, or a
    stream of its own when that is the legacy default stream, which cannot be captured):
      * admit(rows, caps) runs the prefill and first token of new requests in free slots and returns their slot ids;
      * step(n) runs n decode steps of every live slot and returns the slots whose request has finished;
      * take(slot) returns that request's codes (up to and including the stop token, or `cap` codes) and frees the slot.
    Every slot has its own positions, cap and finished state, so requests of any prompt length, prompt and cap share a session.
    Determinism: a request's codes equal, bit for bit, row 0 of UnifiedVoice.generate on `slots` copies of its prompt
    (attention_mask=None) with max_new_tokens = its cap -- whatever else is in flight, when it was admitted and which slot it has.
    With a bf16 KV cache in split-bf16 GEMM mode that reference batch needs slots * (P + 1) >= 256 prefill rows (or the exact
    GEMM mode).  Results can depend on `slots`: the decode attention's key split and the decode GEMV are chosen from it.
    With the batch-invariant mode on (UnifiedVoice.set_batch_invariant, before the session is created; it keeps the mode) the rule is
    simply: a request's codes equal, bit for bit, those of generate on its own prompt alone (B = 1), for every `slots` -- greedy and
    sampled (a seeded request draws the B = 1 stream) -- and a parked row resumes into a session of any slot count.

    sampled=True: admit(rows, caps, sampling=...) gives each request its own sampler -- a dict per row with `sampler` ("greedy" |
    "hf" | "accel"), `temperature`, `top_k`, `top_p` (HF only), and `seed` or `exp_noise` [cap, V].  A sampled request's codes equal,
    bit for bit, row 0 of generate(do_sample=True, sampler=..., temperature=..., top_k=..., top_p=..., seed=seed) on `slots` copies of
    its prompt (with exp_noise: generate's exp_noise whose row 0 is the request's noise); greedy rows equal those of a greedy session.
    The repetition penalty is the session's (the HF sampler applies it, the accel sampler does not).

    scores=True: the samplers also record every code's log-probability under the raw logits; take(slot, scores=True) returns them
    with the codes.  They follow a row through admit(takes=), fork (a take gets the source's first `at` values), park (the ParkedRow
    carries them, to("cpu") included) and resume (into a session that was also created with scores=True; the reverse is refused too),
    and obey every determinism rule above, bit for bit.  The codes are those of a session without scores.

    prefix_scores=True (needs prefix=True and scores=True): a request admitted behind given codes with prefix_logprobs "model" gets
    the log-probabilities of those codes from its own admission prefill (`idxtts_gpt_session_admit_prefix_scored`)."""

    def __init__(self, gpt: UnifiedVoice, slots: int, max_prompt: int, max_new: int, repetition_penalty: float = 10.0,
                 use_graph: bool = True, sampled: bool = False, scores: bool = False, prefix: bool = False, prefix_scores: bool = False):
        self.sampled, self.scores, self.prefix, self.prefix_scores = bool(sampled), bool(scores), bool(prefix), bool(prefix_scores)
        if self.prefix_scores and not (self.prefix and self.scores):
            raise ValueError("prefix_scores=True needs prefix=True and scores=True (IDXTTS_SESSION_PREFIX_SCORES goes with both)")
        lib = _lib.load()
        flags = ((_lib.SESSION_SAMPLED if self.sampled else 0) | (_lib.SESSION_SCORES if self.scores else 0) |
                 (_lib.SESSION_PREFIX if self.prefix else 0) | (_lib.SESSION_PREFIX_SCORES if self.prefix_scores else 0))
        need = int(lib.idxtts_gpt_session_workspace_bytes_ex(gpt._h, int(slots), int(max_prompt), int(max_new), flags))
        if need == 0:
            raise ValueError(f"decode session shape (slots={slots}, max_prompt={max_prompt}, max_new={max_new}) not supported")
        super().__init__(gpt, slots, max_prompt, max_new, use_graph, need,
                         lambda ws, nbytes, sp: lib.idxtts_gpt_session_init_ex(gpt._h, int(slots), int(max_prompt), int(max_new),
                                                                              float(repetition_penalty), flags, ws, nbytes, sp))

    @property
    def free_slots(self):
        return self._free()

    @property
    def live_slots(self):
        return self._live()

    def _samplers(self, sampling, caps):
        """sampling (one dict per row, or one dict for every row) -> (SamplingC array, noise tensors); raises ValueError on a bad row."""
        caps = [None] * len(sampling) if caps is None else caps
        entries = [sampling] * len(caps) if isinstance(sampling, dict) else list(sampling)
        if len(entries) != len(caps):
            raise ValueError("sampling: one entry per row, or one entry for every row")
        V = self.gpt.cfg.number_mel_codes
        arr = (_lib.SamplingC * len(caps))()
        noises = []
        for i, (e, cap) in enumerate(zip(entries, caps)):
            unknown = set(e) - {"sampler", "temperature", "top_k", "top_p", "seed", "exp_noise"}
            if unknown:
                raise ValueError(f"sampling: unknown keys {sorted(unknown)}")
            kind = e.get("sampler", "hf")
            noise = None
            if kind == "greedy":
                arr[i] = _sampling_c("greedy")
            elif kind in ("hf", "accel"):
                t = float(e.get("temperature", 1.0))
                k = int(e.get("top_k") or 0) if kind == "hf" else 0
                p = float(e.get("top_p") if e.get("top_p") is not None else 1.0) if kind == "hf" else 1.0
                check_sampling(t, k, p)
                noise, seed = _draws(e.get("exp_noise"), e.get("seed"), (cap, V), self.gpt.device, "[cap, V] = ")
                arr[i] = _sampling_c(kind, t, k, p, noise, seed)
            else:
                raise ValueError("sampler must be 'greedy', 'hf' or 'accel'")
            noises.append(noise)
        return arr, noises

    def admit(self, inputs_embeds_rows, max_new_each, sampling=None, takes=None, slots=None, prefix=None, prefix_logprobs=None):
        """inputs_embeds_rows: [P_b, d] prompt embeddings (UnifiedVoice.prompt_rows); max_new_each: a cap per row (or one int).
        sampling (sampled sessions): None = every row greedy, else one dict per row or one for every row (see the class).
        takes (an int for every row, or one per row): that many takes of each request -- its prefill runs once, its keys and values go
        to all of its takes' slots, and every take is an ordinary row from then on.  The result is then a list of slot lists, one per
        request; max_new_each and sampling may be given per request (each take of it gets them; a seeded entry would make the takes
        equal, so give seeds per take) or per take, as a list of lists.  Take j's codes equal those of the same prompt admitted alone
        with its sampler.  slots: the free slots to use, in order (default: the first free ones).
        prefix (a session created with prefix=True): one 1-D sequence of mel codes, or None, per request -- the row starts behind
        them, as the row that produced them would have gone on (position layout "resume": code j at mel position j + 2).  The cap counts
        prefix + new codes (k < cap), the row's codes, take() and the draws (exp_noise [cap, V], rows below k never read; a seed's
        counter) are indexed by the absolute step, and a request's takes share its prefix and one prefill.  prefix_logprobs: one fp32
        sequence of the same length, None (= zeros) or the string "model", per request: what take(scores=True) returns for the prefix
        codes.  "model" (a session created with prefix_scores=True): the admission's own prefill scores them, the values
        UnifiedVoice.score_codes gives for prompt and prefix in layout "resume"; the codes drawn do not depend on it.  Rows with
        and without a prefix may share a call; an admission too large for the prefill area is split into groups that fit.  The row's
        codes equal row 0 of generate(input_ids=[fake | prefix], prefix_layout="resume") on `slots` copies of the prompt, with
        exp_noise rows offset by k.  A prefix that holds the stop token, or with k >= cap, raises and nothing changes."""
        n = len(inputs_embeds_rows)
        if n == 0:
            return []
        nested, prefixed = takes is not None, prefix is not None or prefix_logprobs is not None
        if prefixed and not self.prefix:
            raise ValueError("prefix= needs a session created with prefix=True (IDXTTS_SESSION_PREFIX sizes the prefill area for it)")
        if prefixed and prefix is None:
            raise ValueError("prefix_logprobs without prefix")
        pf = [None] * n if prefix is None else list(prefix)
        lp = [None] * n if prefix_logprobs is None else list(prefix_logprobs)
        model = [isinstance(v, str) for v in lp]
        if any(m and v != "model" for m, v in zip(model, lp)):
            raise ValueError('prefix_logprobs: a sequence, None or the string "model" per request')
        if any(model) and not self.prefix_scores:
            raise ValueError('prefix_logprobs="model" needs a session created with prefix_scores=True (IDXTTS_SESSION_PREFIX_SCORES adds the '
                             "scoring head's buffers)")
        lp = [None if m else v for m, v in zip(model, lp)]
        if len(pf) != n or len(lp) != n:
            raise ValueError("prefix / prefix_logprobs: one entry (a 1-D sequence or None) per request")
        tk = [1] * n if takes is None else [int(takes)] * n if isinstance(takes, (int, np.integer)) else [int(t) for t in takes]
        if len(tk) != n or any(t < 1 for t in tk):
            raise ValueError("takes: one count >= 1 per row (or one int for every row)")
        if sampling is not None and not self.sampled:
            raise ValueError("sampling= needs a session created with sampled=True")
        if prefix_logprobs is not None and not self.scores:
            raise ValueError("prefix_logprobs= needs a session created with scores=True")
        T = sum(tk)
        free = self.free_slots
        if T > len(free) and slots is None:
            raise RuntimeError(f"{T} {'takes' if nested and not prefixed else 'rows'} but {len(free)} free slots")
        ids = self._pick(slots, T, free)
        caps_t = [int(c) for c in self._per_take(max_new_each if not isinstance(max_new_each, np.integer) else int(max_new_each), tk,
                                                 "max_new_each")]
        rows, plen, _ = self._stage(inputs_embeds_rows, [1] * n, free)
        if any(not 1 <= c <= self.max_new for c in caps_t):
            raise ValueError(f"caps must be in 1 .. {self.max_new}")
        first = [0]      # request b's takes: ids / caps_t / samplers [first[b] : first[b + 1]]
        for t in tk:
            first.append(first[-1] + t)
        codes, lps = [], []
        for b in range(n):      # (no prefix: an empty one; the smallest cap of the request's takes decides)
            c, l = check_prefix(torch.zeros(0, dtype=torch.long) if pf[b] is None else pf[b], lp[b], self.gpt.cfg,
                                min(caps_t[first[b]:first[b + 1]]))
            codes.append(c)
            lps.append(torch.zeros(c.numel()) if l is None else l)
        klen = [int(c.numel()) for c in codes]
        # the library gets what each caller form has always given it: takes NULL for plain rows, samplers NULL for greedy ones, prefix
        # lengths of zero (which it drops) and no codes where there is no prefix; one group unless prefixes outgrow the prefill area
        self.stream.wait_stream(torch.cuda.current_stream(self.gpt.device))      # the rows may come from another stream
        with torch.cuda.stream(self.stream):
            samplers, noises = (self._samplers(self._per_take(sampling, tk, "sampling"), caps_t) if sampling is not None
                                else (None, [None] * T))
            for g in self._prefix_groups(plen, klen, self._prefill_area()):
                t0, t1 = first[g[0]], first[g[-1] + 1]
                emb, pm = self._embed_rows([rows[b] for b in g], [plen[b] for b in g])
                kg = sum(klen[b] for b in g)
                pk = torch.cat([codes[b] for b in g]).to(self.gpt.device) if kg else None
                pl = torch.cat([lps[b] for b in g]).to(self.gpt.device) if kg and self.scores else None
                h_p, h_t, h_ids, h_caps, h_k = (np.ascontiguousarray(a, dtype=np.int32) for a in (
                    [plen[b] for b in g], [tk[b] for b in g], ids[t0:t1], caps_t[t0:t1], [klen[b] for b in g]))
                args = (self.gpt._h, len(g), _lib.ptr(emb), pm, h_p.ctypes.data_as(c_void_p),
                        h_t.ctypes.data_as(c_void_p) if nested or prefixed else c_void_p(0), h_ids.ctypes.data_as(c_void_p),
                        h_caps.ctypes.data_as(c_void_p),
                        c_void_p(ctypes.addressof(samplers) + t0 * ctypes.sizeof(_lib.SamplingC)) if samplers is not None else c_void_p(0),
                        h_k.ctypes.data_as(c_void_p), _lib.ptr(pk), _lib.ptr(pl))
                if any(model[b] for b in g):      # (no request asks the model: the entry of before)
                    h_m = np.ascontiguousarray([model[b] for b in g], dtype=np.uint8)
                    _lib.check(self._lib.idxtts_gpt_session_admit_prefix_scored(*args, h_m.ctypes.data_as(c_void_p), _lib.ptr(self._ws), self._sp()))
                else:
                    _lib.check(self._lib.idxtts_gpt_session_admit_prefix(*args, _lib.ptr(self._ws), self._sp()))
                self._occupy(ids[t0:t1], noises[t0:t1])
        return [ids[first[b]:first[b + 1]] for b in range(n)] if nested else ids

    def _pick(self, slots, n: int, free: list) -> list:
        """The n slots an admission takes: the first free ones, or the caller's choice (free, distinct)."""
        if slots is None:
            if n > len(free):
                raise RuntimeError(f"{n} rows but {len(free)} free slots")
            return free[:n]
        ids = [int(i) for i in slots]
        if len(ids) != n or len(set(ids)) != n or any(i not in free for i in ids):
            raise ValueError(f"slots= must name {n} distinct free slots")
        return ids

    @staticmethod
    def _per_take(value, tk: list, what: str) -> list:
        """One value for all, one per request, or a list per request with one per take -> a flat list, one per take."""
        if isinstance(value, (int, dict)) or value is None:
            return [value] * sum(tk)
        value = list(value)
        if len(value) != len(tk):
            raise ValueError(f"{what}: one entry per request (or a list per request with one entry per take)")
        flat = []
        for v, t in zip(value, tk):
            if isinstance(v, (list, tuple)):
                if len(v) != t:
                    raise ValueError(f"{what}: a request's list must have one entry per take")
                flat.extend(v)
            else:
                flat.extend([v] * t)
        return flat

    def _prefill_area(self) -> int:
        """Positions of the admission's prefill area (gpt.h session_prefill_rows)."""
        area = self.slots * (self.max_prompt + 1) + 256
        return max(area, self.max_prompt + 1 + self.max_new + 256) if self.prefix else area

    @staticmethod
    def _prefix_groups(plen: list, klen: list, area: int) -> list:
        """Consecutive requests grouped so that each group's right-padded prefill -- rows x the longest P + 1 + k of the group -- fits
        an area of `area` positions; rows are counted as the bf16 cache's padded prefill counts them (at least ceil(256 / S)), which
        is never fewer than the native call takes.  One request always fits (the area holds max_prompt + 1 + max_new + 256)."""
        groups, cur, smax = [], [], 0
        for b in range(len(plen)):
            sb = max(smax, plen[b] + 1 + klen[b])
            if cur and max(len(cur) + 1, -(-256 // sb)) * sb > area:
                groups.append(cur)
                cur, sb = [], plen[b] + 1 + klen[b]
            cur.append(b)
            smax = sb
        if cur:
            groups.append(cur)
        return groups

    def fork(self, slot: int, samplers=None, at=None, caps=None, n=None, slots=None) -> list:
        """Further takes of the request in `slot`, branching where it stood after `at` codes (default: where it stands now): one per
        entry of `samplers` (dicts as in admit(sampling=...); exp_noise [cap, V], rows below `at` are never read), or `n` greedy takes
        when samplers is None.  The source may be decoding, or finished and not taken; it is only read.  One launch on the session's
        stream copies what the source holds for its first `at` codes -- keys and values read once, written to every take -- into free
        slots (`slots`, or the first free ones), which are returned; each take decodes on from the next step() with its own sampler
        and cap (caps: one per take or one int; default the source's, or the row count of a take's exp_noise).  A take forked at k with explicit draws that equal the source's
        below k returns, bit for bit, the codes of a fresh admission with those draws; a seeded take draws from its own seed from step
        k on.  at = 0 redraws the first token too (not on a row that came in through resume()).  A refusal raises, nothing changes."""
        slot = self._held(slot)
        if samplers is not None and not self.sampled:
            raise ValueError("samplers= needs a session created with sampled=True")
        if samplers is None:
            k = 1 if n is None else int(n)
        else:
            samplers = [samplers] if isinstance(samplers, dict) else list(samplers)
            k = len(samplers)
            if n is not None and int(n) != k:
                raise ValueError("n differs from the number of samplers")
        if k < 1:
            raise ValueError("fork to at least one take")
        ids = self._pick(slots, k, self.free_slots)
        caps_t = None if caps is None else [int(caps)] * k if isinstance(caps, (int, np.integer)) else [int(c) for c in caps]
        if caps_t is None and samplers is not None and any(e.get("exp_noise") is not None for e in samplers):
            # explicit draws are [cap, V]: a take that brings them says its cap with their row count (the source's cap: NULL below)
            if any(e.get("exp_noise") is None for e in samplers):
                raise ValueError("caps=: needed when only some takes carry exp_noise")
            caps_t = [int(torch.as_tensor(e["exp_noise"]).shape[0]) for e in samplers]
        if caps_t is not None and (len(caps_t) != k or any(not 1 <= c <= self.max_new for c in caps_t)):
            raise ValueError(f"caps: one per take, in 1 .. {self.max_new}")
        self.stream.wait_stream(torch.cuda.current_stream(self.gpt.device))      # the draws may come from another stream
        with torch.cuda.stream(self.stream):
            arr, noises = self._samplers(samplers, caps_t) if samplers is not None else (None, [None] * k)
            h_ids = np.ascontiguousarray(ids, dtype=np.int32)
            h_caps = np.ascontiguousarray(caps_t, dtype=np.int32) if caps_t is not None else None
            _lib.check(self._lib.idxtts_gpt_session_fork(
                self.gpt._h, slot, -1 if at is None else int(at), k, h_ids.ctypes.data_as(c_void_p),
                ctypes.cast(arr, c_void_p) if arr is not None else c_void_p(0),
                h_caps.ctypes.data_as(c_void_p) if h_caps is not None else c_void_p(0), _lib.ptr(self._ws), self._sp()))
        self._occupy(ids, noises)
        return ids

    def take(self, slot: int, scores: bool = False):
        """The codes of the finished request in `slot` (LongTensor on the device); the slot is free again.  scores=True, on a session
        created with scores=True: (codes, logprobs) -- one fp32 log-probability per code (include/idxtts.h "Scores")."""
        if scores and not self.scores:
            raise ValueError("take(scores=True) needs a session created with scores=True")
        return super().take(slot, scores=scores)

    def park(self, slot: int) -> ParkedRow:
        """Takes the decoding request in `slot` out of the session with everything it has computed -- its step state, sampler, codes
        and the keys and values of its pos cached positions -- and frees the slot: admissible at once, never reported by step().  One
        gather launch on the session's stream; bytes moved are proportional to the row's length.  resume() puts the row back, into any
        free slot of this session or of another one of the same shape, and it goes on to produce, bit for bit, the codes of its
        uninterrupted run.  A slot that is free, has finished (take() it) or is out of range raises, nothing changes."""
        blob, hdr, nz = self._take_out(self._held(slot), self._lib.idxtts_gpt_session_park_bytes, self._lib.idxtts_gpt_session_park,
                                       _lib.ParkHeaderC)
        return ParkedRow(blob, hdr.step, hdr.max_step, nz, self.stream)

    def resume(self, parked: ParkedRow, slot=None) -> int:
        """Puts a parked row into `slot` (default: the first free slot) and returns the slot; the row decodes on from the next step().
        `parked` may live on the device or in host memory (it is staged here) and may come from another session of the same model,
        slots, KV format and GEMM mode whose max_new and cache length hold the rest of the request.  In the batch-invariant mode the
        slot counts need not match (both sessions must be in the mode; a row parked with the mode off is refused there, and the
        reverse).  A refusal raises and changes nothing; a ParkedRow is resumed once."""
        if not isinstance(parked, ParkedRow) or isinstance(parked, ParkedGroup):
            raise TypeError("resume() takes a ParkedRow (a ParkedGroup goes to BeamDecodeSession.resume_group)")
        return self._put_back(parked, slot, self._lib.idxtts_gpt_session_resume)


class BeamDecodeSession(_Session):
    """Beam search / beam-sample with continuous batching: the session's `slots` decode rows form slots / num_beams groups of num_beams
    consecutive slots, one request per group, each with its own parameters:
      * admit(rows, caps, beam=...) runs the prefill (once per request) and first beam step of new requests in free groups and returns
        their group ids;
      * step(n) runs n decode steps of every live group and returns the groups whose request has finished -- its scorer is done
        (BeamHypotheses.is_done with the request's early_stopping / length_penalty) or it reached its cap;
      * take(group) returns that request's codes (the best hypothesis, then the stop token if it fits under the cap) and frees it;
      * park_group(group) takes a decoding request out with everything it has computed and frees its group, resume_group(parked)
        puts it into a free group of this or another session of the same shape: it goes on to bit-identical codes.
    `beam`: one dict, or one per request, with keys do_sample, temperature, top_k, top_p, length_penalty, early_stopping (defaults:
    generate_beam's) and `seed` or `exp_noise` [cap, num_beams * V] (neither: a seed drawn from torch's global RNG).
    Determinism: a request's codes equal, bit for bit, row 0 of UnifiedVoice.generate_beam with the same parameters and repetition penalty
    on slots / num_beams copies of its prompt (attention_mask=None, max_new_tokens = its cap; with exp_noise: generate_beam's exp_noise
    whose [:, 0, :] is the request's noise), cut after its first stop token -- whatever else is in flight, when it was admitted and which
    group it has (DecodeSession's conditions: a bf16 KV cache in split-bf16 GEMM mode needs slots * (P + 1) >= 256).
    With the batch-invariant mode on (UnifiedVoice.set_batch_invariant) a request's codes equal those of generate(num_beams=...) on
    its own prompt alone, for every `slots` and group; a seeded request draws the B = 1 stream."""

    _BEAM_KEYS = {"do_sample", "temperature", "top_k", "top_p", "length_penalty", "early_stopping", "seed", "exp_noise"}

    def __init__(self, gpt: UnifiedVoice, slots: int, num_beams: int, max_prompt: int, max_new: int, repetition_penalty: float = 10.0,
                 use_graph: bool = True):
        nb = int(num_beams)
        if not 2 <= nb <= 8:
            raise ValueError("2 <= num_beams <= 8")
        if int(slots) % nb:
            raise ValueError(f"slots ({slots}) must be a multiple of num_beams ({nb})")
        lib = _lib.load()
        need = int(lib.idxtts_gpt_session_workspace_bytes_beam(gpt._h, int(slots), nb, int(max_prompt), int(max_new)))
        if need == 0:
            raise ValueError(f"beam session shape (slots={slots}, num_beams={nb}, max_prompt={max_prompt}, max_new={max_new}) not supported")
        self.num_beams = nb
        self._unit = nb
        super().__init__(gpt, slots, max_prompt, max_new, use_graph, need,
                         lambda ws, nbytes, sp: lib.idxtts_gpt_session_init_beam(gpt._h, int(slots), nb, int(max_prompt), int(max_new),
                                                                                float(repetition_penalty), ws, nbytes, sp))
        self.groups = self.slots // nb

    @property
    def free_groups(self):
        return self._free()

    @property
    def live_groups(self):
        return self._live()

    def _beams(self, beam, caps):
        """beam (one dict, or one per request) -> (BeamC array, noise tensors); parameter values are checked by the library."""
        entries = [beam or {}] * len(caps) if beam is None or isinstance(beam, dict) else list(beam)
        if len(entries) != len(caps):
            raise ValueError("beam: one entry per request, or one entry for every request")
        V, nb = self.gpt.cfg.number_mel_codes, self.num_beams
        arr = (_lib.BeamC * len(caps))()
        noises = []
        for i, (e, cap) in enumerate(zip(entries, caps)):
            unknown = set(e) - self._BEAM_KEYS
            if unknown:
                raise ValueError(f"beam: unknown keys {sorted(unknown)}")
            if e.get("early_stopping", False) not in (False, True):
                raise NotImplementedError('early_stopping="never" is not implemented')
            noise, seed = _draws(e.get("exp_noise"), e.get("seed"), (cap, nb * V), self.gpt.device, "[cap, num_beams * V] = ")
            tp = e.get("top_p")
            arr[i] = _lib.BeamC(num_beams=nb, do_sample=int(bool(e.get("do_sample", True))), temperature=float(e.get("temperature", 1.0)),
                                top_k=int(e.get("top_k", 50) or 0), top_p=float(tp if tp is not None else 1.0),
                                length_penalty=float(e.get("length_penalty", 1.0)), early_stopping=int(bool(e.get("early_stopping", False))),
                                exp_noise=noise.data_ptr() if noise is not None else None, seed=seed)
            noises.append(noise)
        return arr, noises

    def admit(self, inputs_embeds_rows, max_new_each, beam=None, prefix=None, prefix_logprobs=None) -> list:
        """inputs_embeds_rows: [P_b, d] prompt embeddings (UnifiedVoice.prompt_rows); max_new_each: a cap per request (or one int);
        beam: the requests' parameters (see the class).  Returns their group ids.  A refused call takes no group.
        prefix / prefix_logprobs: refused -- beams do not continue from given codes (DecodeSession.admit does)."""
        if prefix is not None or prefix_logprobs is not None:
            raise NotImplementedError("a beam session takes no prefix: HF's length penalty counts the prefix and the scorer's rows would "
                                      "have to hold it; continue from given codes in a DecodeSession (decode_session(prefix=True))")
        if len(inputs_embeds_rows) == 0:
            return []
        free = self.free_groups
        rows, plen, caps = self._stage(inputs_embeds_rows, max_new_each, free)
        n = len(rows)
        ids = free[:n]
        self.stream.wait_stream(torch.cuda.current_stream(self.gpt.device))      # the rows may come from another stream
        with torch.cuda.stream(self.stream):
            beams, noises = self._beams(beam, caps)
            emb, pm = self._embed_rows(rows, plen)
            h_p, h_ids, h_caps = (np.ascontiguousarray(a, dtype=np.int32) for a in (plen, ids, caps))
            _lib.check(self._lib.idxtts_gpt_session_admit_beam(
                self.gpt._h, n, _lib.ptr(emb), pm, h_p.ctypes.data_as(c_void_p), h_ids.ctypes.data_as(c_void_p),
                h_caps.ctypes.data_as(c_void_p), ctypes.cast(beams, c_void_p), _lib.ptr(self._ws), self._sp()))
        self._occupy(ids, noises)
        return ids

    def take(self, group: int, n_best=None):
        """The codes of the finished request in `group` (LongTensor on the device); the group is free again.
        n_best (1 .. num_beams): the scorer's n_best best hypotheses instead, best first -- a list of (codes, score), each codes as the
        plain take() cuts it (the hypothesis, then the stop token where it fits under the cap), in generate_beam(num_return_sequences=)'s
        order; entry 0's codes are bit for bit what take(group) returns."""
        if n_best is None:
            return super().take(group)
        n_best = int(n_best)
        if not 1 <= n_best <= self.num_beams:
            raise ValueError("1 <= n_best <= num_beams")
        lens, scores = np.zeros(n_best, np.int32), np.zeros(n_best, np.float32)
        self.stream.wait_stream(torch.cuda.current_stream(self.gpt.device))
        with torch.cuda.stream(self.stream):
            out = torch.empty(n_best, self.max_new, dtype=torch.long, device=self.gpt.device)
            _lib.check(self._lib.idxtts_gpt_session_read_nbest(self.gpt._h, int(group) * self._unit, n_best, _lib.ptr(out),
                                                               lens.ctypes.data_as(c_void_p), scores.ctypes.data_as(c_void_p),
                                                               _lib.ptr(self._ws), self._sp()))
        self._vacate(group, record=False)
        return [(out[q, : int(lens[q])], float(scores[q])) for q in range(n_best)]

    def park(self, group: int):
        raise NotImplementedError("one row of a beam group cannot leave it: park the whole group with park_group()")

    def resume(self, parked, group=None):
        raise NotImplementedError("a beam session resumes whole groups: resume_group() takes what park_group() returned")

    def park_group(self, group: int) -> ParkedGroup:
        """Takes the decoding request in `group` out of the session with everything it has computed -- the step state, the request's
        beam parameters, every beam's tokens, seen ids and score, the scorer's finished hypotheses, and the cached keys and values: the
        prompt positions once, the generated positions per beam -- and frees the group: admissible at once, never reported by step().
        One gather launch on the session's stream.  resume_group() puts it back, into any free group of this session or of another
        beam session of the same shape, and it goes on to produce, bit for bit, the codes of its uninterrupted run.  A group that is
        free, has finished (take() it) or is out of range raises, nothing changes."""
        blob, hdr, nz = self._take_out(self._held(group), self._lib.idxtts_gpt_session_park_group_bytes,
                                       self._lib.idxtts_gpt_session_park_group, _lib.ParkGroupHeaderC)
        return ParkedGroup(blob, hdr, nz, self.stream)

    def resume_group(self, parked: ParkedGroup, group=None) -> int:
        """Puts a parked group into `group` (default: the first free group) and returns the group id; it decodes on from the next
        step().  `parked` may live on the device or in host memory (it is staged here) and may come from another beam session of the
        same model, slots, num_beams, KV format and GEMM mode whose max_new and cache length hold the rest of the request.  In the
        batch-invariant mode the slot counts need not match (both sessions must be in the mode).  A refusal raises and changes nothing;
        a ParkedGroup is resumed once."""
        if not isinstance(parked, ParkedGroup):
            raise TypeError("resume_group() takes a ParkedGroup (a ParkedRow goes to DecodeSession.resume)")
        return self._put_back(parked, group, self._lib.idxtts_gpt_session_resume_group)
