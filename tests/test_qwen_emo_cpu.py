"""CPU: the host side of the emotion-from-text classifier (indextts_amd/qwen_emo.py, checkpoint.py) against the reference's own
QwenEmotion / normalize_emo_vec as recorded in tests/golden/qwen_emo_cases.json (tests/golden/make_qwen_golden.py); the language
model's generate is stubbed with the recorded ids.  Also: the language-model fixtures (qwen_lm.npz, qwen_lm_shapes.npz) keep the
properties the GPU tests lean on, and idxtts_qwen_create refuses the shapes the kernels are not built for."""
import json
import os

import numpy as np
import pytest
import torch

import qwen_shapes as qs
from qwen_ckpt_dir import StubTokenizer, write_qwen_dir, write_safetensors


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "qwen_emo_cases.json"), encoding="utf-8") as f:
        return json.load(f)


class CannedLM:
    """Stands in for qwen_emo.QwenLM: returns the recorded answer."""

    def __init__(self):
        self.canned, self.seen = [], []

    def generate(self, prompt_ids, max_new_tokens, eos_ids=(), **kw):
        self.seen.append((list(prompt_ids), int(max_new_tokens), list(eos_ids)))
        return list(self.canned), None


def _classifier():
    from indextts_amd.qwen_emo import QwenConfig, QwenEmotion
    tok, lm = StubTokenizer(), CannedLM()
    return QwenEmotion(None, QwenConfig.tiny(), tok, model=lm), tok, lm


def test_every_recorded_case_parses_as_the_reference(golden):
    emo, tok, lm = _classifier()
    assert len(golden["cases"]) >= 8
    for case in golden["cases"]:
        lm.canned = case["output_ids"]
        got = emo.inference(case["text"])
        assert [[k, v] for k, v in got.items()] == case["expected"], case["name"]      # keys, their order and the values, exactly


def test_chat_messages_and_tokenizer_calls_follow_the_reference(golden):
    emo, tok, lm = _classifier()
    case = golden["cases"][0]
    lm.canned = case["output_ids"]
    emo.inference(case["text"])
    ref = case["calls"]
    assert [c[0] for c in tok.calls] == [c[0] for c in ref] == ["apply_chat_template", "__call__", "decode"]
    assert tok.calls[0][1] == ref[0][1] and tok.calls[0][2] == ref[0][2]      # the two messages; tokenize / generation prompt / thinking
    assert tok.calls[0][1] == [{"role": "system", "content": golden["misc"]["prompt"]}, {"role": "user", "content": case["text"]}]
    assert tok.calls[1][1] == ref[1][1]                                          # tokenizer([text]) on the templated string
    assert tok.calls[2][2] == ref[2][2] == {"skip_special_tokens": True}
    # the model sees the tokenizer's ids of the templated prompt and stops at the tokenizer's end token
    prompt_ids, cap, eos = lm.seen[0]
    assert prompt_ids == tok(ref[1][1])["input_ids"][0] and eos == [tok.eos_token_id] and cap == 512


def test_clamp_key_order_and_constants(golden):
    emo, _, _ = _classifier()
    m = golden["misc"]
    assert [[v, emo.clamp_score(v)] for v, _ in m["clamp_score"]] == m["clamp_score"]
    assert emo.max_score == m["max_score"] == 1.2 and emo.min_score == m["min_score"] and emo.prompt == m["prompt"]
    assert list(emo.convert({}).keys()) == m["key_order"]


def test_hitting_the_cap_warns():
    from indextts_amd.qwen_emo import QwenConfig, QwenEmotion
    tok, lm = StubTokenizer(), CannedLM()
    emo = QwenEmotion(None, QwenConfig.tiny(), tok, model=lm, max_new_tokens=4)
    lm.canned = [1100, 1101, 1102, 1103]
    with pytest.warns(UserWarning, match="max_new_tokens"):
        emo.inference("x")


def test_normalize_emo_vec_equals_the_reference_method(golden):
    from indextts_amd.infer_v2 import IndexTTS2
    tts = IndexTTS2.__new__(IndexTTS2)
    assert len(golden["normalize_emo_vec"]) >= 3
    for c in golden["normalize_emo_vec"]:
        assert tts.normalize_emo_vec(list(c["emo_vector"]), c["apply_bias"]) == c["expected"]
    assert tts.normalize_emo_vec([0.1] * 8) == tts.normalize_emo_vec([0.1] * 8, apply_bias=True)


def test_use_emo_text_without_a_classifier_is_refused():
    from indextts_amd.infer_v2 import IndexTTS2
    tts = IndexTTS2.__new__(IndexTTS2)
    with pytest.raises(NotImplementedError, match="emo_text"):
        tts.infer(None, [[1, 2, 3]], None, use_emo_text=True, emo_text="happy")


def test_use_emo_text_with_token_ids_needs_emo_text(golden):
    from indextts_amd.infer_v2 import IndexTTS2
    tts = IndexTTS2.__new__(IndexTTS2)
    tts.qwen_emo, _, _ = _classifier()
    with pytest.raises(ValueError, match="emo_text"):
        tts.infer(None, [[1, 2, 3]], None, use_emo_text=True)


def test_safetensors_reader_round_trips(tmp_path):
    from indextts_amd.checkpoint import read_safetensors
    from indextts_amd.qwen_emo import to_bf16_grid
    rng = np.random.default_rng(3)
    t = {"a.weight": to_bf16_grid(rng.standard_normal((5, 7)).astype(np.float32)), "b": to_bf16_grid(rng.standard_normal(3).astype(np.float32)),
         "scalar": to_bf16_grid(np.float32(2.5).reshape(()))}
    for dtype in ("BF16", "F32"):
        p = str(tmp_path / f"{dtype}.safetensors")
        write_safetensors(p, t, dtype)
        got = read_safetensors(p)
        assert set(got) == set(t)
        for k in t:
            assert got[k].dtype == torch.float32 and tuple(got[k].shape) == t[k].shape and np.array_equal(got[k].numpy(), t[k]), (dtype, k)
    from safetensors.torch import load_file      # the container the third-party reader sees is the same one
    theirs = load_file(str(tmp_path / "BF16.safetensors"))
    assert all(np.array_equal(theirs[k].float().numpy(), t[k]) for k in t)


def test_checkpoint_directory_fields(tmp_path):
    """config.json / generation_config.json / model.safetensors as from_pretrained reads them (the model itself needs the GPU:
    tests/test_qwen_emo_gpu.py)."""
    from indextts_amd.checkpoint import read_safetensors
    from indextts_amd.qwen_emo import QwenConfig
    cfg, w = write_qwen_dir(str(tmp_path / "qwen"))
    with open(tmp_path / "qwen" / "config.json") as f:
        assert QwenConfig.from_hf(json.load(f), max_context=cfg.max_context) == cfg
    sd = read_safetensors(str(tmp_path / "qwen" / "model.safetensors"))
    assert set(sd) == set(w) and all(np.array_equal(sd[k].numpy(), w[k]) for k in w)
    assert QwenConfig() == QwenConfig.from_hf({})      # the published Qwen3-0.6B values are the defaults
    d = QwenConfig()
    assert (d.vocab_size, d.hidden_size, d.intermediate_size, d.num_hidden_layers, d.num_attention_heads, d.num_key_value_heads, d.head_dim,
            d.rms_norm_eps, d.rope_theta, d.tie_word_embeddings) == (151936, 1024, 3072, 28, 16, 8, 128, 1e-6, 1e6, True)


def test_head_dim_other_than_128_is_refused_with_a_message():
    import dataclasses
    from indextts_amd.qwen_emo import QwenConfig, QwenLM
    with pytest.raises(RuntimeError, match="head_dim 64 is not supported"):
        QwenLM({}, dataclasses.replace(QwenConfig.tiny(), head_dim=64), device="cpu")


# ---- the language-model fixtures: what the GPU tests assume of them, re-asserted from the stored arrays alone ----
@pytest.fixture(scope="module")
def lm_golden(golden_dir):
    return {f: dict(np.load(os.path.join(golden_dir, f))) for f in ("qwen_lm.npz", "qwen_lm_shapes.npz")}


@pytest.mark.parametrize("name", [c.name for c in qs.LM_CASES + qs.SHAPE_CASES])
def test_lm_fixture_case_is_self_consistent(name, lm_golden):
    case = qs.BY_NAME[name]
    g = lm_golden[case.file]
    prompt, ids, cols, logits = g[name + "_prompt"], g[name + "_ids"], g[name + "_cols"], g[name + "_logits"]
    eps, tol = float(g[name + "_eps"]), float(g[name + "_logit_tol"])
    V = case.config().vocab_size
    # the inputs: the prompt is its synth regeneration, the weights' tag is the one the case list names
    assert prompt.dtype == np.int32 and np.array_equal(prompt, case.prompt(int(g[name + "_seed"]))) and len(prompt) == case.P
    if case.name == "full_long":
        assert int(g[name + "_wseed"]) == int(lm_golden["qwen_lm.npz"]["full_seed"])      # the GPU test reuses that loaded model
        assert qs.weights_tag(case, g) == qs.weights_tag(qs.BY_NAME["full"], lm_golden["qwen_lm.npz"])
    # the stored columns: sorted, distinct, in the vocabulary, as many as the list says (at least), every step's two best among them
    assert logits.shape == (case.max_new, len(cols)) and len(ids) == case.max_new and logits.dtype == np.float32
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < V and len(cols) >= (case.n_cols or V)
    assert np.isfinite(logits).all()
    order = np.argsort(-logits, axis=1, kind="stable")
    best, second = np.take_along_axis(logits, order[:, :1], 1)[:, 0], np.take_along_axis(logits, order[:, 1:2], 1)[:, 0]
    # a column outside the subset that beat a stored one would make ids != argmax here: the generator put both best in
    assert np.array_equal(cols[order[:, 0]], ids)
    assert tol == 4.0 * eps and eps > 0
    margin = float((best - second).min())
    assert margin >= 4.0 * tol, f"{name}: top-2 margin {margin:.3e} < 4 x logit_tol {tol:.3e}"
    # the path the case is there for
    qs.check_claims(case)
    smax = (case.P + case.max_new + 3) & ~3
    nsplit = min(16, max(1, -(-smax // 64)))
    assert (smax, nsplit, -(-smax // nsplit)) == (case.smax, case.nsplit, case.slice_cap)
    if case.file == "qwen_lm_shapes.npz":
        assert (int(g[name + "_nsplit"]), int(g[name + "_slice_cap"])) == (nsplit, -(-smax // nsplit))


def test_lm_fixtures_hold_exactly_the_listed_cases(lm_golden, golden_dir):
    keys = ("ids", "logits", "cols", "prompt", "eps", "logit_tol", "seed")
    assert set(lm_golden["qwen_lm.npz"]) == {f"{c.name}_{k}" for c in qs.LM_CASES for k in keys}
    assert set(lm_golden["qwen_lm_shapes.npz"]) == {f"{c.name}_{k}" for c in qs.SHAPE_CASES for k in keys + ("wseed", "nsplit", "slice_cap")}
    assert os.path.getsize(os.path.join(golden_dir, "qwen_lm_shapes.npz")) <= os.path.getsize(os.path.join(golden_dir, "qwen_lm.npz"))
    # what the behavioural GPU tests take from the fixture
    g = lm_golden["qwen_lm_shapes.npz"]
    k = qs.stop_step(g["tiny_p980_n40_ids"])
    assert k is not None and k >= 9 and (k + 1) % 8 != 0
    assert not np.array_equal(g["tiny_p40_n25_prompt"], g["tiny_p40_n25_b_prompt"]) and not np.array_equal(g["tiny_p40_n25_ids"], g["tiny_p40_n25_b_ids"])
    assert {qs.BY_NAME[n].nsplit for n in ("tiny_p980_n40", "tiny_p40_n25", "tiny_p1_n200")} == {16, 2, 4}


# ---- idxtts_qwen_create: shapes the kernels are not built for are refused by name, without a device ----
def _create(cfg):
    import ctypes
    from indextts_amd import _lib
    lib = _lib.load()
    c = _lib.QwenConfigC(cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                         cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.rope_theta, int(cfg.tie_word_embeddings), cfg.max_context)
    h = ctypes.c_void_p()
    _lib.check(lib.idxtts_qwen_create(ctypes.byref(c), ctypes.byref(h)))
    assert h.value
    lib.idxtts_ctx_destroy(h)


REFUSED = [
    ("five_query_heads_per_kv_head", dict(num_attention_heads=5, num_key_value_heads=1), "1..4 query heads per kv head"),
    ("heads_not_a_multiple_of_kv_heads", dict(num_attention_heads=3, num_key_value_heads=2), "1..4 query heads per kv head"),
    ("odd_vocabulary", dict(vocab_size=511), "vocab_size must be even"),
    ("hidden_size_3080", dict(hidden_size=3080), "hidden_size: a multiple of 8, at most 3072"),
    ("hidden_size_132", dict(hidden_size=132), "hidden_size: a multiple of 8, at most 3072"),
    ("intermediate_size_3080", dict(intermediate_size=3080), "intermediate_size: a multiple of 8, at most 3072"),
    ("query_width_above_3072", dict(num_attention_heads=32, num_key_value_heads=8), "num_attention_heads * head_dim: at most 3072"),
    ("scores_past_the_lds_budget", dict(max_context=5124), "query heads per kv head * max_context <= 10240"),      # tiny: G = 2
    ("max_context_4", dict(max_context=4), "query heads per kv head * max_context <= 10240"),
]


@pytest.mark.parametrize("change,message", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_qwen_create_refuses(change, message):
    import dataclasses
    import re
    from indextts_amd.qwen_emo import QwenConfig
    with pytest.raises(RuntimeError, match=re.escape(message)):
        _create(dataclasses.replace(QwenConfig.tiny(), **change))


@pytest.mark.parametrize("name", ["tiny", "g1", "g4", "g3"])
def test_qwen_create_accepts_the_fixture_configurations(name):
    _create(qs.CONFIGS[name])
    if name == "tiny":      # right at the bounds the refusals sit behind
        import dataclasses
        _create(dataclasses.replace(qs.CONFIGS[name], max_context=8))
        _create(dataclasses.replace(qs.CONFIGS[name], hidden_size=3072, intermediate_size=3072, num_attention_heads=24, num_key_value_heads=6, max_context=2560))
