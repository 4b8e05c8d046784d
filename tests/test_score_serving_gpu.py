"""GPU: scoring given codes in serving, on the tiny synthetic pipeline.
  * ContinuousPipeline(prefix=True, scores=True, prefix_scores=True).submit(prefix_codes=[c[:k]], prefix_logprobs="model", takes=3,
    keep=1): the ranking is serving.rank_request of the three takes' codes and of UnifiedVoice.score_codes of those codes (through
    IndexTTS2.score_takes) -- every code counts, the given ones included -- and the codes are those of the run with caller-given values;
  * IndexTTS2.score_takes on the takes of a scored run: a stopped take above every capped one, the order of gpt.sequence_scores, the
    scores the run recorded."""
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu
GAP = 1e-3          # score gaps the ranking must not depend on tolerances for
SCORE_TOL = 1e-4    # the same quantity through the prefill instead of the steps (tests/test_prefix_session_gpu.py), averaged over a take


def _tts(device, tag, stop_bias):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag=f"{tag}/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = stop_bias
    wg["mel_head.bias"][cfg.gpt.start_mel_token] = -1e4      # a sampled start token is no semantic code
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag=f"{tag}/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag=f"{tag}/voc"), device=device)
    return cfg, tts, PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"{tag}/prompt").to(device)


def _trim(row, stop, cap):
    hits = (row == stop).nonzero()
    return row[: int(hits[0]) + 1] if len(hits) else row[:cap]


def _gaps(ranking):
    """Smallest score gap between neighbours of the same group (stopped / capped)."""
    g = [abs(a[1] - b[1]) for a, b in zip(ranking, ranking[1:]) if a[2] == b[2]]
    return min(g) if g else float("inf")


def test_pipeline_ranks_retakes_with_the_prefix_scored(device):
    from indextts_amd.serving import ContinuousPipeline
    cfg, tts, cond = _tts(device, "t/score/pipe", stop_bias=1.0)
    stop = cfg.gpt.stop_mel_token
    L, cap, k, n, T = 7, 14, 5, 3, 9
    text = torch.from_numpy(synth.integers("t/score/pipe/text", (1, L), 2, cfg.gpt.number_text_tokens))
    pre = torch.from_numpy(synth.integers("t/score/pipe/prefix", (k,), 0, cfg.gpt.start_mel_token))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9}
    seen, stage = [], tts.gpt_stage

    def recording(t, c, **kw):
        if kw.get("codes") is not None:
            seen.append(kw["codes"].clone().cpu())
        return stage(t, c, **kw)
    tts.gpt_stage = recording
    checked = 0
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True, scores=True, prefix=True,
                                    prefix_scores=True) as pipe:
                for S in (21, 22, 23, 24):
                    kw = dict(max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n, prefix_codes=[pre])
                    pipe.submit(text, cond, prefix_logprobs=[np.zeros(k, np.float32)], **kw).result()      # caller-given values, all takes
                    codes_all = seen.pop()
                    fut = pipe.submit(text, cond, prefix_logprobs="model", keep=1, **kw)
                    fut.result()
                    codes_best = seen.pop()
                    assert not seen and codes_all.shape[0] == n and bool((codes_all[:, :k] == pre).all())
                    rows = [_trim(codes_all[t], stop, cap) for t in range(n)]
                    lps, want = tts.score_takes(text, cond, rows)
                    (got,) = fut.ranking
                    print(f"seed {S}: pipeline ranking {[(t, round(sc, 5), st, nc) for t, sc, st, nc in got]}, smallest gap {_gaps(want):.3e}")
                    if _gaps(want) <= GAP:
                        continue      # (a seed whose takes score too close together says nothing about the order)
                    checked += 1
                    assert [(t, st, nc) for t, _, st, nc in got] == [(t, st, nc) for t, _, st, nc in want]
                    assert all(abs(a[1] - b[1]) <= SCORE_TOL for a, b in zip(got, want))
                    # the score counts the given codes: with the caller's zeros for them it would be another number
                    t0, sc0, _, n0 = got[0]
                    tail_only = float(lps[t0][k:].double().sum()) / n0
                    assert abs(sc0 - tail_only) > GAP
                    # the kept take is the winner, its codes those of the run with caller-given values
                    assert torch.equal(codes_best[0, :n0], rows[t0]) and bool((codes_best[0, n0:] == stop).all())
    finally:
        tts.gpt_stage = stage
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert checked, "every seed's takes scored within 1e-3 of each other: the test shows nothing"


def test_score_takes_ranks_stopped_above_capped(device):
    from indextts_amd.gpt import rank_takes, sequence_scores
    cfg, tts, cond = _tts(device, "t/scores/cap", stop_bias=2.0)      # (the model of test_scores_pipeline_gpu.py's cap test)
    stop = cfg.gpt.stop_mel_token
    text = torch.from_numpy(synth.integers("t/scores/cap/text", (1, 7), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 1.0, "top_k": 30, "top_p": 0.9}
    mixed = 0
    for cap in (8, 11, 14):
        codes, ran = tts.ranked_takes(text, cond, 8, max_mel_tokens=cap, sampling=dict(samp, generator=torch.Generator().manual_seed(cap)))
        rows = [_trim(r, stop, cap) for r in codes.cpu()]
        lps, ranking = tts.score_takes(text, cond, rows)
        assert sorted(t for t, *_ in ranking) == list(range(8)) and [len(l) for l in lps] == [len(r) for r in rows]
        flags = [st for _, _, st, _ in ranking]
        assert flags == sorted(flags, reverse=True), "a capped take ranks above a stopped one"
        scores = sequence_scores(lps, [len(r) for r in rows])
        stopped = [int(r[-1]) == stop for r in rows]
        assert [t for t, *_ in ranking] == rank_takes(scores, stopped)
        assert all(nc == cap for _, _, st, nc in ranking if not st)
        by_run = {t: sc for t, sc, _, _ in ran[0]}
        worst = max(abs(sc - by_run[t]) for t, sc, _, _ in ranking)
        print(f"cap {cap}: {sum(flags)} stopped of 8, max |score(score_takes) - score(scored run)| = {worst:.3e}")
        assert worst <= SCORE_TOL
        mixed += 0 < sum(flags) < 8
    assert mixed, "no cap had both stopped and capped takes: the test shows nothing"
    with pytest.raises(ValueError, match="one text"):
        tts.score_takes(text.repeat(2, 1), cond, rows)
    with pytest.raises(ValueError, match="at least one"):
        tts.score_takes(text, cond, [])
