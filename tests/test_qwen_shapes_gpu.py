"""GPU: the Qwen3 decoder (csrc/qwen.hip through indextts_amd/qwen_emo.QwenLM) at the shapes tests/test_qwen_emo_gpu.py leaves out,
against tests/golden/qwen_lm_shapes.npz -- third-party transformers.Qwen3ForCausalLM on the same synthetic weights
(tests/golden/make_qwen_golden.py shapes; the case list with what each case reaches is tests/qwen_shapes.py):
  the decode attention's key split (partials, last-arriver merge, pieces without a key), a piece longer than one 256-thread pass,
  prompt lengths 1, around 64 and 256, and 4200, 1 / 3 / 4 query heads per kv head, GEMV widths whose last 512-chunk is part-filled or
  empty, a head whose last workgroup is part-filled, an untied head; and, on key-split sizes, stopping at an end id under graph replay,
  a kept graph replayed for another prompt, and calls of different splits back to back on one workspace.

The logit tolerance is each case's own: 4 x the reference's fp32-vs-fp64 error, measured by the generator, which also made sure the
reference's two best logits are >= 4 tolerances apart at every step (tests/test_qwen_emo_cpu.py re-asserts it): no step is left out.
Every case prints its worst |logit - reference| and that figure / logit_tol (run with -s).  Not yet measured on an MI355X: no GPU
could be had while these tests were written; the figures belong here once a run has printed them.
"""
import os

import numpy as np
import pytest
import torch

import qwen_shapes as qs
from indextts_amd.qwen_emo import QwenLM

pytestmark = pytest.mark.gpu

_models = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "qwen_lm_shapes.npz")))


def _lm(name, fmt, golden, device):
    """One model per (configuration, storage format): the cases of a configuration share their weights."""
    case = qs.BY_NAME[name]
    key = (case.cfg, fmt)
    if key not in _models:
        _models[key] = (qs.weights_tag(case, golden), QwenLM(qs.case_weights(case, golden), case.config(), device=device, weight_format=fmt))
    tag, lm = _models[key]
    assert tag == qs.weights_tag(case, golden)
    return lm


_case = qs.stored


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
@pytest.mark.parametrize("name", qs.REDUCED)
def test_logits_and_ids_match_the_reference(name, fmt, golden, device):
    qs.check_against_reference(_lm(name, fmt, golden, device), name, fmt, golden)


@pytest.mark.parametrize("name", qs.REDUCED)
def test_bf16_storage_equals_fp32_storage_bit_for_bit(name, golden, device):
    qs.check_formats_agree(_lm(name, "f32", golden, device), _lm(name, "bf16", golden, device), name, golden)


@pytest.mark.parametrize("name,fmt", [("tiny_p1_n200", "bf16"), ("tiny_p980_n40", "bf16"), ("tiny_p980_n40", "f32"), ("tiny_p4200_n60", "bf16"),
                                      ("g1", "bf16"), ("g3", "bf16"), ("g4", "bf16"), ("g4", "f32")])
def test_graph_replay_equals_eager_bit_for_bit(name, fmt, golden, device):
    qs.check_graph_equals_eager(_lm(name, fmt, golden, device), name, golden)


STOP_CASE = "tiny_p980_n40"      # 16 key pieces


def test_stops_at_an_end_id_inside_a_key_split_graph_replayed_run(golden, device):
    """The host looks for the end every 8 steps; the end id here comes between two looks, so replays follow it and must change nothing."""
    lm = _lm(STOP_CASE, "bf16", golden, device)
    prompt, ids, _ = _case(STOP_CASE, golden)
    ids = ids.tolist()
    k = qs.stop_step(ids)
    assert k is not None and k >= 9 and (k + 1) % 8 != 0 and ids.index(ids[k]) == k and qs.BY_NAME[STOP_CASE].nsplit > 1
    other = next(v for v in range(512) if v not in ids)      # a second end id that never comes
    out = {}
    for use_graph in (False, True):
        got, lg = lm.generate(prompt, len(ids), eos_ids=[other, ids[k]], logits=True, use_graph=use_graph)
        assert got == ids[:k + 1] and lg.shape[0] == k + 1
        out[use_graph] = lg
    assert lm.step_graph_launches() > 0
    assert torch.equal(out[False], out[True])


def test_a_kept_graph_is_replayed_for_another_prompt(golden, device):
    lm = _lm("tiny_p40_n25", "bf16", golden, device)
    pa, ia, _ = _case("tiny_p40_n25", golden)
    pb, ib, _ = _case("tiny_p40_n25_b", golden)
    assert len(pa) == len(pb) and len(ia) == len(ib) and not np.array_equal(pa, pb) and ia.tolist() != ib.tolist()
    a_eager, _ = lm.generate(pa, len(ia), use_graph=False)
    a_graph, _ = lm.generate(pa, len(ia), use_graph=True)
    n_a = lm.step_graph_launches()
    b_graph, _ = lm.generate(pb, len(ib), use_graph=True)      # same workspace, lengths and outputs: the kept graph, no eager step
    n_b = lm.step_graph_launches()
    b_eager, _ = lm.generate(pb, len(ib), use_graph=False)
    assert n_a == n_b and 0 < n_a <= 5 * 2 + 2
    assert a_eager == a_graph == ia.tolist()
    assert b_graph == b_eager == ib.tolist()


def test_calls_with_different_splits_back_to_back_on_one_workspace(golden, device):
    """16 pieces, then 2, then 16 again on the same (grow-only) workspace: counters and partials of one call do not reach the next."""
    lm = _lm("tiny_p980_n40", "bf16", golden, device)
    p_long, i_long, c_long = _case("tiny_p980_n40", golden)
    p_short, i_short, c_short = _case("tiny_p40_n25", golden)
    first = lm.generate(p_long, len(i_long), logits=True, logit_cols=c_long)
    mid = lm.generate(p_short, len(i_short), logits=True, logit_cols=c_short)
    third = lm.generate(p_long, len(i_long), logits=True, logit_cols=c_long)
    assert first[0] == third[0] == i_long.tolist() and torch.equal(first[1], third[1])
    assert mid[0] == i_short.tolist()
    for (_, lg), name in ((first, "tiny_p980_n40"), (mid, "tiny_p40_n25")):
        assert np.abs(lg.cpu().numpy() - golden[name + "_logits"]).max() <= float(golden[name + "_logit_tol"])
