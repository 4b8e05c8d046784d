"""CPU: the host side of batched emotion classification (QwenEmotion.inference_batch against the recorded reference cases of
tests/golden/qwen_emo_cases.json, the language model stubbed), the refusals of idxtts_qwen_batch_workspace_bytes, and a guard that
the batches tests/test_qwen_batch_gpu.py builds from the fixtures stay buildable: a fixture change fails here, not quietly there."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest

import qwen_shapes as qs
from qwen_ckpt_dir import StubTokenizer


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "qwen_emo_cases.json"), encoding="utf-8") as f:
        return json.load(f)


class CannedBatchLM:
    """Stands in for qwen_emo.QwenLM: every prompt gets the answer recorded for it."""

    def __init__(self):
        self.by_prompt, self.batch_calls = {}, 0

    def generate(self, prompt_ids, max_new_tokens, eos_ids=(), **kw):
        return list(self.by_prompt[tuple(prompt_ids)]), None

    def generate_batch(self, prompts, max_new_tokens, eos_ids=(), **kw):
        self.batch_calls += 1
        return [list(self.by_prompt[tuple(p)]) for p in prompts], None


def _classifier(**kw):
    from indextts_amd.qwen_emo import QwenConfig, QwenEmotion
    tok, lm = StubTokenizer(), CannedBatchLM()
    return QwenEmotion(None, QwenConfig.tiny(), tok, model=lm, **kw), lm


def test_inference_batch_equals_the_recorded_reference_and_inference(golden):
    emo, lm = _classifier()
    cases = golden["cases"]
    assert len(cases) >= 8
    for c in cases:
        lm.by_prompt[tuple(emo._prompt_ids(c["text"]))] = c["output_ids"]
    assert len(lm.by_prompt) == len({c["text"] for c in cases})      # distinct texts give distinct prompts
    got = emo.inference_batch([c["text"] for c in cases])
    assert lm.batch_calls == 1                                       # one batched generation for all texts
    for c, d in zip(cases, got):
        assert [[k, v] for k, v in d.items()] == c["expected"], c["name"]      # keys, their order and the values, exactly
        assert d == emo.inference(c["text"]), c["name"]
    assert emo.inference_batch([]) == [] and lm.batch_calls == 1


def test_the_cap_warning_fires_per_row():
    emo, lm = _classifier(max_new_tokens=4)
    texts = ["a", "b", "c"]
    end = emo._end_ids()[0]
    answers = [[1100, 1101, 1102, 1103], [1100, 1101, end], [1100, 1101, 1102, end]]      # cut at the cap; ended early; ended at the cap
    for t, a in zip(texts, answers):
        lm.by_prompt[tuple(emo._prompt_ids(t))] = a
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        emo.inference_batch(texts)
    assert len([w for w in rec if "max_new_tokens" in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        emo.inference_batch([texts[0], texts[1], texts[0]])
    assert len([w for w in rec if "max_new_tokens" in str(w.message)]) == 2


def test_batch_workspace_refusals_and_growth():
    from indextts_amd import _lib
    lib = _lib.load()
    cfg = qs.CONFIGS["tiny"]
    c = _lib.QwenConfigC(cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                         cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.rope_theta, int(cfg.tie_word_embeddings), cfg.max_context)
    h = ctypes.c_void_p()
    _lib.check(lib.idxtts_qwen_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        need = lambda B, P, M: lib.idxtts_qwen_batch_workspace_bytes(h, B, ptr(P) if P is not None else None, ptr(M) if M is not None else None, 1, 64)
        P, M = arr([40] * 16), arr([25] * 16)
        tile = lib.idxtts_qwen_max_batch(h)
        assert 1 <= tile <= 16
        assert need(0, P, M) == 0 and need(-1, P, M) == 0
        assert need(2, None, M) == 0 and need(2, P, None) == 0
        assert need(2, arr([40, 0]), M) == 0 and need(2, P, arr([25, -3])) == 0
        sizes = [need(B, P, M) for B in range(1, tile + 1)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))      # it grows with B, up to the tile
        assert need(tile + 3, P, M) == sizes[-1]                                  # further rows reuse the workspace tile by tile
        assert lib.idxtts_qwen_workspace_bytes(h, 40, 25, 1, 64) > 0
        assert lib.idxtts_qwen_batch_step_graph_launches(h) == -1
    finally:
        lib.idxtts_ctx_destroy(h)


def test_a_batch_of_one_needs_the_single_call_workspace():
    """Both size functions go through the one carve: a one-row tile takes no row table."""
    from indextts_amd import _lib
    lib = _lib.load()
    cfg = qs.CONFIGS["tiny"]
    c = _lib.QwenConfigC(cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                         cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.rope_theta, int(cfg.tie_word_embeddings), cfg.max_context)
    h = ctypes.c_void_p()
    _lib.check(lib.idxtts_qwen_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        for P, M in ((1, 3), (40, 25), (63, 8), (65, 8), (980, 40)):
            for n_eos, n_cols in ((0, 0), (1, 64), (2, 512)):
                Pa, Ma = np.ascontiguousarray([P], dtype=np.int32), np.ascontiguousarray([M], dtype=np.int32)
                one = lib.idxtts_qwen_workspace_bytes(h, P, M, n_eos, n_cols)
                batch = lib.idxtts_qwen_batch_workspace_bytes(h, 1, ctypes.c_void_p(Pa.ctypes.data), ctypes.c_void_p(Ma.ctypes.data), n_eos, n_cols)
                assert batch == one > 0, (P, M, n_eos, n_cols)
    finally:
        lib.idxtts_ctx_destroy(h)


@pytest.fixture(scope="module")
def lm_golden(golden_dir):
    return {f: dict(np.load(os.path.join(golden_dir, f))) for f in ("qwen_lm.npz", "qwen_lm_shapes.npz")}


def test_the_gpu_batches_are_buildable_from_the_fixtures(lm_golden):
    import test_qwen_batch_gpu as gpu
    shapes, lm = lm_golden["qwen_lm_shapes.npz"], lm_golden["qwen_lm.npz"]
    for batch in (gpu.RAGGED, gpu.PARTIAL, gpu.RAGGED + gpu.PARTIAL, ["tiny_p980_n40", "tiny_p40_n25", "tiny_p1_n200"]):
        assert {qs.BY_NAME[n].cfg for n in batch} == {"tiny"}
        assert len({qs.weights_tag(qs.BY_NAME[n], shapes) for n in batch}) == 1      # one loaded model serves the batch
        assert len({int(shapes[n + "_wseed"]) for n in batch}) == 1
    assert [qs.geometry(qs.BY_NAME[n].P, qs.BY_NAME[n].max_new)[1] for n in gpu.RAGGED] == [1, 4, 2, 2, 2, 2, 5, 16]
    assert sorted(qs.BY_NAME[n].max_new for n in gpu.RAGGED) == [3, 8, 8, 8, 25, 25, 40, 200]
    assert qs.BY_NAME["tiny_p1_n3"].P == 1 and qs.BY_NAME["tiny_p1_n200"].P + 1 < qs.BY_NAME["tiny_p1_n200"].nsplit
    assert max(qs.BY_NAME[n].smax for n in gpu.RAGGED) <= qs.CONFIGS["tiny"].max_context
    # full width: full_long runs on the weights of full, one key piece beside four
    assert qs.weights_tag(qs.BY_NAME["full_long"], shapes) == qs.weights_tag(qs.BY_NAME["full"], lm)
    assert (qs.BY_NAME["full"].nsplit, qs.BY_NAME["full_long"].nsplit) == (1, 4)
    # the other head groupings: 60 stored steps, capped again at 17; K = 3072 is g3's
    for n in ("g1", "g3", "g4"):
        assert qs.BY_NAME[n].max_new == 60 and len(shapes[n + "_ids"]) == 60
    assert qs.CONFIGS["g3"].intermediate_size == 3072
    # the stop test: an end id on the first row that the host's look every 8 steps does not fall on
    assert qs.stop_step(shapes["tiny_p980_n40_ids"]) is not None
