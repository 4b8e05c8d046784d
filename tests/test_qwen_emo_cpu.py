"""CPU: the host side of the emotion-from-text classifier (indextts_amd/qwen_emo.py, checkpoint.py) against the reference's own
QwenEmotion / normalize_emo_vec as recorded in tests/golden/qwen_emo_cases.json (tests/golden/make_qwen_golden.py); the language
model's generate is stubbed with the recorded ids."""
import json
import os

import numpy as np
import pytest
import torch

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
