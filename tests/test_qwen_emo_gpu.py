"""GPU: the Qwen3 decoder of the emotion-from-text classifier (csrc/qwen.hip through indextts_amd/qwen_emo.QwenLM) against
tests/golden/qwen_lm.npz -- third-party transformers.Qwen3ForCausalLM on the same synthetic weights, tests/golden/make_qwen_golden.py --
and `IndexTTS2.infer(use_emo_text=True)` end to end at reduced width.

The logit tolerance is the fixture's: 4 x the reference's own fp32-vs-fp64 error, measured by the generator.  The generator also
made sure the reference's two best logits are >= 4 tolerances apart at every recorded step, so the argmax comparison skips none.
Measured on an MI355X: worst error 2.6e-6 = 0.25 x logit_tol (tiny), 2.6e-5 = 0.19 x logit_tol (full), both storage formats."""
import os

import numpy as np
import pytest
import torch

from indextts_amd import synth, weights
from indextts_amd.config import PipelineConfig
from indextts_amd.qwen_emo import QwenConfig, QwenEmotion, QwenLM, synth_qwen_weights
import qwen_shapes as qs
from qwen_ckpt_dir import EOS_ID, StubTokenizer, write_qwen_dir

pytestmark = pytest.mark.gpu

CONFIGS = {"tiny": QwenConfig.tiny(), "full": QwenConfig()}
_weights, _models = {}, {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "qwen_lm.npz")))


def _w(name, golden):
    if name not in _weights:
        _weights[name] = synth_qwen_weights(CONFIGS[name], tag=f"golden/qwen/{name}/s{int(golden[name + '_seed'])}")
    return _weights[name]


def _lm(name, fmt, golden, device):
    if (name, fmt) not in _models:
        _models[(name, fmt)] = QwenLM(_w(name, golden), CONFIGS[name], device=device, weight_format=fmt)
    return _models[(name, fmt)]


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "full"])
def test_logits_and_ids_match_the_reference(name, fmt, golden, device):
    lm = _lm(name, fmt, golden, device)
    prompt, ids, cols = golden[name + "_prompt"], golden[name + "_ids"], golden[name + "_cols"]
    ref, tol = golden[name + "_logits"], float(golden[name + "_logit_tol"])
    steps = len(ids)
    # teacher-forced on the reference's ids: every step's logits and every step's own argmax
    own, lg = lm.generate(prompt, steps, forced_ids=ids, logits=True, logit_cols=None if name == "tiny" else cols)
    lg = lg.cpu().numpy()
    assert lg.shape == ref.shape
    err = np.abs(lg - ref).max(axis=1)
    print(f"{name}/{fmt}: max |logit - reference| per step {np.array2string(err, precision=2)}; worst {err.max():.3e} = "
          f"{err.max() / tol:.3f} x logit_tol {tol:.3e} (eps {float(golden[name + '_eps']):.3e})")
    assert np.isfinite(lg).all() and err.max() <= tol, f"worst logit error {err.max():.3e} > logit_tol {tol:.3e}"
    assert own == ids.tolist()
    # free-running greedy decode
    free, _ = lm.generate(prompt, steps)
    assert free == ids.tolist()


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_bf16_storage_equals_fp32_storage_bit_for_bit(name, golden, device):
    prompt, ids, cols = golden[name + "_prompt"], golden[name + "_ids"], golden[name + "_cols"]
    out = []
    for fmt in ("f32", "bf16"):
        out.append(_lm(name, fmt, golden, device).generate(prompt, len(ids), forced_ids=ids, logits=True, logit_cols=cols))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name,fmt", [("tiny", "f32"), ("tiny", "bf16"), ("full", "bf16")])
def test_graph_replay_equals_eager_bit_for_bit(name, fmt, golden, device):
    lm = _lm(name, fmt, golden, device)
    prompt, ids, cols = golden[name + "_prompt"], golden[name + "_ids"], golden[name + "_cols"]
    eager = lm.generate(prompt, len(ids), logits=True, logit_cols=cols, use_graph=False)
    graph = lm.generate(prompt, len(ids), logits=True, logit_cols=cols, use_graph=True)
    assert eager[0] == graph[0] == ids.tolist() and torch.equal(eager[1], graph[1])
    # the decode replays a graph of at most 5 launches per layer + 3 per token
    n = lm.step_graph_launches()
    assert 0 < n <= 5 * CONFIGS[name].num_hidden_layers + 3, n
    lm.generate(prompt, len(ids), use_graph=True)
    assert 0 < lm.step_graph_launches() <= 5 * CONFIGS[name].num_hidden_layers + 2


@pytest.fixture(scope="module")
def shapes(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "qwen_lm_shapes.npz")))


# "full_long" (tests/qwen_shapes.py): the "full" weights at prompt 150 + 100 steps -- four key pieces, as every real call has
@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_full_width_key_split_matches_the_reference(fmt, golden, shapes, device):
    assert int(shapes["full_long_wseed"]) == int(golden["full_seed"]) and qs.BY_NAME["full_long"].nsplit == 4
    qs.check_against_reference(_lm("full", fmt, golden, device), "full_long", fmt, shapes)


def test_full_width_key_split_formats_and_graph_agree_bit_for_bit(golden, shapes, device):
    assert int(shapes["full_long_wseed"]) == int(golden["full_seed"])
    qs.check_formats_agree(_lm("full", "f32", golden, device), _lm("full", "bf16", golden, device), "full_long", shapes)
    qs.check_graph_equals_eager(_lm("full", "bf16", golden, device), "full_long", shapes)


def test_stops_at_an_end_id_and_at_the_cap(golden, device):
    lm = _lm("tiny", "bf16", golden, device)
    prompt, ids = golden["tiny_prompt"], golden["tiny_ids"].tolist()
    k = 9
    stop = ids[k]
    first = ids.index(stop)
    for use_graph in (False, True):
        got, lg = lm.generate(prompt, len(ids), eos_ids=[stop, 511 if stop != 511 else 510], logits=True, use_graph=use_graph)
        assert got == ids[:first + 1] and lg.shape[0] == first + 1
        capped, _ = lm.generate(prompt, 7, use_graph=use_graph)
        assert capped == ids[:7]
    one, _ = lm.generate(prompt, 1)
    assert one == ids[:1]
    with pytest.raises(RuntimeError, match="context"):
        lm.generate(prompt, CONFIGS["tiny"].max_context)


def test_bf16_finalize_names_the_tensor_off_the_grid(golden, device):
    w = dict(_w("tiny", golden))
    key = "model.layers.1.mlp.up_proj.weight"
    w[key] = w[key].copy()
    w[key][3, 5] = np.float32(0.1)      # 0.1 has no finite binary expansion: not a bf16 value
    with pytest.raises(RuntimeError, match=key.replace(".", r"\.")):
        QwenLM(w, CONFIGS["tiny"], device=device, weight_format="bf16")
    lm = QwenLM(w, CONFIGS["tiny"], device=device, weight_format="f32")      # fp32 storage takes it
    assert len(lm.generate(golden["tiny_prompt"], 3)[0]) == 3


def test_other_head_dims_are_refused(device):
    import dataclasses
    with pytest.raises(RuntimeError, match="head_dim 64"):
        QwenLM({}, dataclasses.replace(CONFIGS["tiny"], head_dim=64), device=device)


def test_from_pretrained_reads_the_checkpoint_directory(tmp_path, device):
    import dataclasses
    from indextts_amd.checkpoint import qwen_emotion_from_pretrained
    cfg, w = write_qwen_dir(str(tmp_path / "qwen"), eos_ids=(EOS_ID % 512, 7))
    tok = StubTokenizer(vocab=cfg.vocab_size)
    emo = qwen_emotion_from_pretrained(str(tmp_path / "qwen"), device=device, tokenizer=tok, max_new_tokens=12)
    assert emo.eos_ids == [EOS_ID % 512, 7] and emo.model.cfg == dataclasses.replace(cfg, max_context=4096)
    direct = QwenLM(w, cfg, device=device, weight_format="f32")
    prompt = tok([tok.apply_chat_template([{"role": "system", "content": emo.prompt}, {"role": "user", "content": "hello"}])])["input_ids"][0]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert emo.generate(prompt) == direct.generate(prompt, 12, eos_ids=emo.eos_ids)[0]
        d = emo.inference("hello")
    assert list(d) == ["happy", "angry", "sad", "afraid", "disgusted", "melancholic", "surprised", "calm"]


class ScoringTokenizer(StubTokenizer):
    """decode: a JSON answer whose scores come from the generated ids, so the emotion vector depends on what the GPU decoded."""

    def decode(self, ids, **kw):
        ids = list(ids)
        return '{"高兴": %.1f, "悲伤": %.1f, "惊讶": 0.3}' % ((ids[0] % 9 + 1) / 10, (ids[1] % 9 + 1) / 10)


def test_infer_use_emo_text_end_to_end(golden, device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptFeatures
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/pipe/gpt")
    wg.update(weights.synth_gpt_cond_weights(cfg.gpt, tag="t/pipe/gpt"))
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/pipe/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/pipe/voc"), device=device)
    feats = PromptFeatures.synthetic(cfg, prompt_frames=11, feat_frames=31, tag="t/pipe/feats")
    emo_num = [3, 2, 4, 1, 2, 1, 2, 3]
    emo_matrix = torch.from_numpy(synth.uniform("t/qwen/emo_matrix", (sum(emo_num), cfg.gpt.model_dim), 0.5))
    spk_matrix = torch.from_numpy(synth.uniform("t/qwen/spk_matrix", (sum(emo_num), cfg.s2mel.style_dim), 1.0))
    tts.set_emotion_matrices(emo_matrix, spk_matrix, emo_num)
    seg = synth.integers("t/qwen/eseg", (1, 6), 2, cfg.gpt.number_text_tokens).tolist()
    G = dict(do_sample=False, num_beams=1, max_mel_tokens=12)
    import warnings
    warnings.simplefilter("ignore")
    with pytest.raises(NotImplementedError):
        tts.infer(feats, seg, None, use_emo_text=True, emo_text="so happy", **G)
    qcfg = CONFIGS["tiny"]
    tts.qwen_emo = QwenEmotion(_w("tiny", golden), qcfg, ScoringTokenizer(vocab=qcfg.vocab_size), device=device, max_new_tokens=8)
    scores = tts.qwen_emo.inference("so happy")
    assert len(scores) == 8 and 0 < scores["happy"] <= 0.9 and 0 < scores["sad"] <= 0.9 and scores["surprised"] == 0.3
    torch.manual_seed(4)
    _, a = tts.infer(feats, seg, None, use_emo_text=True, emo_text="so happy", **G)
    torch.manual_seed(4)
    _, b = tts.infer(feats, seg, None, emo_vector=list(scores.values()), **G)
    assert np.array_equal(a, b)
    torch.manual_seed(4)
    _, c = tts.infer(feats, seg, None, **G)
    assert not np.array_equal(a, c)
    torch.manual_seed(4)
    _, a2 = tts.infer(feats, seg, None, use_emo_text=True, emo_text="so happy", emo_alpha=0.5, **G)
    torch.manual_seed(4)
    _, b2 = tts.infer(feats, seg, None, emo_vector=list(scores.values()), emo_alpha=0.5, **G)
    assert np.array_equal(a2, b2) and not np.array_equal(a, a2)
