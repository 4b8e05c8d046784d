"""GPU: batched generation of the Qwen3 decoder (csrc/qwen.hip, csrc/qwen_kernels.hip through QwenLM.generate_batch, QwenEmotion.inference_batch and
IndexTTS2.conditionings_from_emo_texts).  Rows of a batch are independent, so every expectation is the single-prompt one: the
fixtures tests/golden/qwen_lm.npz and qwen_lm_shapes.npz (third-party transformers on the same synthetic weights; case list:
tests/qwen_shapes.py) give each row's ids and logits within that case's own logit_tol, and `generate` on the same model gives them
bit for bit.  tests/test_qwen_batch_cpu.py re-asserts what these batches assume of the fixtures (shared weights, the key pieces).

Every tolerance case prints its worst |logit - reference| and that figure / logit_tol (run with -s).  Measured on an MI355X, the
same figures in both storage formats: the ragged batch of 8 (test 1) 1.1e-6 .. 3.0e-6, worst 0.459 x logit_tol (tiny_p1_n3; the
other rows 0.17 .. 0.27 x); g1 6.9e-6 = 0.242 x, g3 4.4e-6 = 0.240 x, g4 1.0e-5 = 0.255 x (test 4); full 2.6e-5 = 0.187 x and
full_long 3.2e-5 = 0.210 x (test 5).  Every row equalled its single call bit for bit.
"""
import os

import numpy as np
import pytest
import torch

import qwen_shapes as qs
from indextts_amd import synth, weights
from indextts_amd.config import PipelineConfig
from indextts_amd.qwen_emo import QwenConfig, QwenEmotion, QwenLM, synth_qwen_weights
from qwen_ckpt_dir import StubTokenizer

pytestmark = pytest.mark.gpu

RAGGED = ["tiny_p1_n3", "tiny_p1_n200", "tiny_p40_n25", "tiny_p40_n25_b", "tiny_p63_n8", "tiny_p65_n8", "tiny_p257_n8", "tiny_p980_n40"]
PARTIAL = ["tiny_p64_n8", "tiny_p255_n8", "tiny_p256_n8"]
_models, _single = {}, {}


@pytest.fixture(scope="module")
def shapes(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "qwen_lm_shapes.npz")))


@pytest.fixture(scope="module")
def lm_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "qwen_lm.npz")))


def _lm(name, fmt, fixture, device):
    """One model per (weights, storage format)."""
    case = qs.BY_NAME[name]
    key = (qs.weights_tag(case, fixture), fmt)
    if key not in _models:
        _models[key] = QwenLM(qs.case_weights(case, fixture), case.config(), device=device, weight_format=fmt)
    return _models[key]


def _single_call(lm, key, prompt, n, **kw):
    """generate(prompt, n, ...) on `lm`, computed once per distinct call and left unchanged."""
    cols = kw.get("logit_cols")
    k = (id(lm), key, n, tuple(sorted((a, v) for a, v in kw.items() if a != "logit_cols")),
         None if cols is None else tuple(int(c) for c in cols))
    if k not in _single:
        _single[k] = lm.generate(prompt, n, **kw)
    return _single[k]


def _rows(names, fixture):
    return [qs.stored(n, fixture) for n in names]


def _check_rows_against_reference(names, fmt, ids_b, lg_b, cols_of, fixture):
    for b, name in enumerate(names):
        _, ids, cols = qs.stored(name, fixture)
        ref, tol = fixture[name + "_logits"], float(fixture[name + "_logit_tol"])
        lg = lg_b[b].cpu().numpy()[:, cols_of(cols)]
        assert lg.shape == ref.shape, (name, lg.shape, ref.shape)
        err = np.abs(lg - ref).max(axis=1)
        print(f"batch row {b} {name}/{fmt}: worst |logit - reference| {err.max():.3e} (step {int(err.argmax())}) = {err.max() / tol:.3f} x logit_tol {tol:.3e}")
        assert np.isfinite(lg).all() and err.max() <= tol, f"{name}: worst logit error {err.max():.3e} > logit_tol {tol:.3e}"
        assert ids_b[b] == ids.tolist(), name


# ---- 1. a ragged batch of 8: key pieces 1, 4, 2, 2, 2, 2, 5, 16; rows finish after 3, 8, 25, 40 steps while one runs 200 ----
@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_ragged_batch_matches_the_reference(fmt, shapes, device):
    assert [qs.BY_NAME[n].nsplit for n in RAGGED] == [1, 4, 2, 2, 2, 2, 5, 16]
    lm = _lm(RAGGED[0], fmt, shapes, device)
    rows = _rows(RAGGED, shapes)
    prompts, caps, forced = [r[0] for r in rows], [len(r[1]) for r in rows], [r[1] for r in rows]
    ids_b, lg_b = lm.generate_batch(prompts, caps, forced_ids=forced, logits=True)      # all 512 columns
    assert all(l.shape == (c, 512) for l, c in zip(lg_b, caps))
    _check_rows_against_reference(RAGGED, fmt, ids_b, lg_b, lambda cols: cols, shapes)
    free, none = lm.generate_batch(prompts, caps)
    assert none is None and free == [f.tolist() for f in forced]


# ---- 2. bit for bit with the single call, both formats, eager and graph ----
@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_ragged_batch_equals_the_single_calls_bit_for_bit(fmt, shapes, device):
    lm = _lm(RAGGED[0], fmt, shapes, device)
    rows = _rows(RAGGED, shapes)
    prompts, caps = [r[0] for r in rows], [len(r[1]) for r in rows]
    graph = lm.generate_batch(prompts, caps, logits=True, use_graph=True)
    assert 0 < lm.batch_step_graph_launches() <= 5 * 2 + 3
    eager = lm.generate_batch(prompts, caps, logits=True, use_graph=False)
    for b, name in enumerate(RAGGED):
        for use_graph in (False, True):
            one = _single_call(lm, name, prompts[b], caps[b], logits=True, use_graph=use_graph)
            for got in (graph, eager):
                assert got[0][b] == one[0], (name, use_graph)
                assert torch.equal(got[1][b], one[1]), (name, use_graph)


# ---- 3. a partial tile, a single row, more rows than one tile ----
def test_partial_tile_single_row_and_over_full_call(shapes, device):
    lm = _lm(PARTIAL[0], "bf16", shapes, device)
    tile = lm.max_batch()
    assert tile >= 1
    over = (PARTIAL + RAGGED[2:6]) * 4
    over = over[:tile + 3]
    for names in (PARTIAL, PARTIAL[:1], over):
        rows = _rows(names, shapes)
        prompts, caps = [r[0] for r in rows], [len(r[1]) for r in rows]
        ids_b, lg_b = lm.generate_batch(prompts, caps, logits=True)
        assert len(ids_b) == len(names)
        for b, name in enumerate(names):
            one = _single_call(lm, name, prompts[b], caps[b], logits=True, use_graph=True)
            assert ids_b[b] == one[0] == rows[b][1].tolist(), (name, b)
            assert torch.equal(lg_b[b], one[1]), (name, b)
        for b, name in enumerate(names):      # equal prompts in different slots give equal rows
            first = names.index(name)
            assert ids_b[b] == ids_b[first] and torch.equal(lg_b[b], lg_b[first])


# ---- 4. other head groupings and GEMV templates (g3: K = 3072, the largest activation staging) ----
@pytest.mark.parametrize("name", ["g1", "g3", "g4"])
def test_other_head_groupings(name, shapes, device):
    prompt, ids, cols = qs.stored(name, shapes)
    assert len(ids) == 60
    for fmt in ("bf16", "f32"):
        lm = _lm(name, fmt, shapes, device)
        ids_b, lg_b = lm.generate_batch([prompt, prompt], [60, 17], logits=True, logit_cols=cols)
        _check_rows_against_reference([name], fmt, ids_b[:1], lg_b[:1], lambda c: slice(None), shapes)
        assert ids_b[1] == ids.tolist()[:17]
        for b, n in enumerate((60, 17)):
            one = _single_call(lm, name, prompt, n, logits=True, logit_cols=cols)
            assert ids_b[b] == one[0] and torch.equal(lg_b[b], one[1]), (fmt, n)


def test_full_tile_at_the_widest_k(shapes, device):
    """g3 with every row of the tile in flight: K = 3072 x 8 rows is the one staging above 64 KiB of LDS (the function attribute)."""
    prompt, ids, cols = qs.stored("g3", shapes)
    lm = _lm("g3", "bf16", shapes, device)
    caps = ([60, 17, 9, 33, 60, 1, 2, 25] * 2)[:lm.max_batch()]
    ids_b, lg_b = lm.generate_batch([prompt] * len(caps), caps, logits=True, logit_cols=cols)
    for b, n in enumerate(caps):
        one = _single_call(lm, "g3", prompt, n, logits=True, logit_cols=cols)
        assert ids_b[b] == one[0] == ids.tolist()[:n] and torch.equal(lg_b[b], one[1]), (b, n)


# ---- 5. full width: full (P 40, 24 steps, one piece) with full_long (P 150, 100 steps, four pieces) ----
def test_full_width_batch(shapes, lm_golden, device):
    assert int(shapes["full_long_wseed"]) == int(lm_golden["full_seed"]) and qs.BY_NAME["full_long"].nsplit == 4
    lm = _lm("full", "bf16", lm_golden, device)
    assert lm is _lm("full_long", "bf16", shapes, device)
    (pa, ia, ca), (pb, ib, cb) = qs.stored("full", lm_golden), qs.stored("full_long", shapes)
    union = np.union1d(ca, cb).astype(np.int32)
    ids_b, lg_b = lm.generate_batch([pa, pb], [len(ia), len(ib)], logits=True, logit_cols=union)
    for b, (name, fx, cols, prompt, ids) in enumerate((("full", lm_golden, ca, pa, ia), ("full_long", shapes, cb, pb, ib))):
        at = np.searchsorted(union, cols)
        assert np.array_equal(union[at], cols)
        _check_rows_against_reference([name], "bf16", ids_b[b:b + 1], [lg_b[b]], lambda c: at, fx)
        one = _single_call(lm, name, prompt, len(ids), logits=True, logit_cols=union)
        assert ids_b[b] == one[0] and torch.equal(lg_b[b], one[1]), name


# ---- 6. stops: an end id on one row, the others to their caps or their own first occurrence; the context check ----
def test_stops_per_row_and_context_check(shapes, device):
    names = ["tiny_p980_n40", "tiny_p40_n25", "tiny_p1_n200"]
    lm = _lm(names[0], "bf16", shapes, device)
    rows = _rows(names, shapes)
    prompts, caps = [r[0] for r in rows], [len(r[1]) for r in rows]
    ids0 = rows[0][1].tolist()
    k = qs.stop_step(ids0)
    assert k is not None
    eos = ids0[k]
    expect = []
    for _, ids, _ in rows:
        ids = ids.tolist()
        expect.append(ids[:ids.index(eos) + 1] if eos in ids else ids)
    assert expect[0] == ids0[:k + 1]
    out = {}
    for use_graph in (False, True):
        ids_b, lg_b = lm.generate_batch(prompts, caps, eos_ids=[eos], logits=True, use_graph=use_graph)
        assert ids_b == expect
        assert [l.shape[0] for l in lg_b] == [len(e) for e in expect]
        out[use_graph] = lg_b
    assert all(torch.equal(a, b) for a, b in zip(out[False], out[True]))
    before = lm.generate_batch(prompts[:2], caps[:2])[0]
    with pytest.raises(RuntimeError, match="context"):
        lm.generate_batch(prompts[:2], [caps[0], qs.CONFIGS["tiny"].max_context])
    assert lm.generate_batch(prompts[:2], caps[:2])[0] == before


# ---- 7. the batched step costs no more launches than the single one ----
def test_launch_count(shapes, device):
    lm = _lm("tiny_p40_n25", "bf16", shapes, device)
    (pa, ia, _), (pb, ib, _) = qs.stored("tiny_p40_n25", shapes), qs.stored("tiny_p40_n25_b", shapes)
    lm.generate_batch([pa, pb], [len(ia), len(ib)], logits=True)
    layers = qs.CONFIGS["tiny"].num_hidden_layers
    assert 0 < lm.batch_step_graph_launches() <= 5 * layers + 3
    lm.generate_batch([pa, pb], [len(ia), len(ib)])
    assert 0 < lm.batch_step_graph_launches() <= 5 * layers + 2


# ---- 8. the kept step graphs: one more key than the tiles' cache holds, and the two caches side by side ----
MAX_BATCH_GRAPHS = 8      # QwenModel::MAX_BATCH_GRAPHS (csrc/qwen.h)


def test_step_graph_eviction_and_recapture(shapes, device):
    lm = _lm("tiny_p40_n25", "bf16", shapes, device)
    (pa, ia, _), (pb, ib, _) = qs.stored("tiny_p40_n25", shapes), qs.stored("tiny_p40_n25_b", shapes)
    layers = qs.CONFIGS["tiny"].num_hidden_layers

    def call(i):
        caps = [3 + i, 4]
        ids, lg = lm.generate_batch([pa, pb], caps, logits=True)
        assert ids == [ia.tolist()[:caps[0]], ib.tolist()[:caps[1]]], i
        assert 0 < lm.batch_step_graph_launches() <= 5 * layers + 3, i
        return ids, lg

    first = call(0)
    for i in range(1, MAX_BATCH_GRAPHS + 1):      # nine distinct keys: the first one leaves
        call(i)
    again = call(0)                               # captured anew
    assert again[0] == first[0]
    assert all(torch.equal(a, b) for a, b in zip(again[1], first[1]))


def test_the_two_step_graph_caches_do_not_disturb_each_other(shapes, device):
    lm = _lm("tiny_p40_n25", "bf16", shapes, device)
    (pa, ia, _), (pb, ib, _) = qs.stored("tiny_p40_n25", shapes), qs.stored("tiny_p40_n25_b", shapes)
    assert len(ia) == len(ib) == 25
    single = lambda: lm.generate(pa, 25, logits=True)
    batch = lambda: lm.generate_batch([pa, pb], [25, 25], logits=True)
    one = single()
    kept = lm.step_graph_launches()
    assert kept > 0
    batch()
    two = single()
    assert two[0] == one[0] == ia.tolist() and torch.equal(two[1], one[1])
    assert lm.step_graph_launches() == kept
    b1 = batch()
    kept_b = lm.batch_step_graph_launches()
    assert kept_b > 0
    single()
    b2 = batch()
    assert b2[0] == b1[0] == [ia.tolist(), ib.tolist()] and all(torch.equal(x, y) for x, y in zip(b2[1], b1[1]))
    assert lm.batch_step_graph_launches() == kept_b and lm.step_graph_launches() == kept


# ---- 9. the classifier and the conditioning helper ----
class ScoringTokenizer(StubTokenizer):
    """decode: a JSON answer whose scores come from the generated ids, so the emotion vector depends on what the GPU decoded."""

    def decode(self, ids, **kw):
        ids = list(ids)
        return '{"高兴": %.1f, "悲伤": %.1f, "惊讶": 0.3}' % ((ids[0] % 9 + 1) / 10, (ids[1] % 9 + 1) / 10)


def test_classifier_batch_and_conditionings(lm_golden, device):
    import warnings
    from indextts_amd.infer_v2 import IndexTTS2, PromptFeatures
    warnings.simplefilter("ignore")
    qcfg = QwenConfig.tiny()
    qw = synth_qwen_weights(qcfg, tag=f"golden/qwen/tiny/s{int(lm_golden['tiny_seed'])}")
    emo = QwenEmotion(qw, qcfg, ScoringTokenizer(vocab=qcfg.vocab_size), device=device, max_new_tokens=8)
    texts = ["so happy", "I feel low and gloomy today", "what a surprise, truly"]
    single = [emo.inference(t) for t in texts]
    assert emo.inference_batch(texts) == single
    assert emo.inference_batch([]) == []

    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/pipe/gpt")
    wg.update(weights.synth_gpt_cond_weights(cfg.gpt, tag="t/pipe/gpt"))
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/pipe/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/pipe/voc"), device=device)
    feats = PromptFeatures.synthetic(cfg, prompt_frames=11, feat_frames=31, tag="t/pipe/feats")
    emo_num = [3, 2, 4, 1, 2, 1, 2, 3]
    tts.set_emotion_matrices(torch.from_numpy(synth.uniform("t/qwen/emo_matrix", (sum(emo_num), cfg.gpt.model_dim), 0.5)),
                             torch.from_numpy(synth.uniform("t/qwen/spk_matrix", (sum(emo_num), cfg.s2mel.style_dim), 1.0)), emo_num)
    seg = synth.integers("t/qwen/eseg", (1, 6), 2, cfg.gpt.number_text_tokens).tolist()
    G = dict(do_sample=False, num_beams=1, max_mel_tokens=12)
    tts.qwen_emo = emo
    conds = tts.conditionings_from_emo_texts(feats, texts, emo_alpha=0.5)
    assert len(conds) == len(texts)
    waves = []
    for i, t in enumerate(texts):
        torch.manual_seed(4)
        _, a = tts.infer(conds[i], seg, None, **G)
        torch.manual_seed(4)
        _, b = tts.infer(feats, seg, None, use_emo_text=True, emo_text=t, emo_alpha=0.5, **G)
        assert np.array_equal(a, b), t
        waves.append(a)
    assert single[0] != single[1] and not np.array_equal(waves[0], waves[1])
