"""GPU: ranking and best-of-n through the pipelines and the top level, on the tiny pipeline.
  * ContinuousPipeline(scores=True).submit(takes=3, keep=1, noise_seed=...) returns, bit for bit, the waveform that submit(takes=3)
    returns at index fut.ranking[i][0][0], and the one a single request with exactly that take's seed and noise seed returns (in the
    exact GEMM mode: the kept takes' latent pass has a third of the full request's rows, and the split-bf16 GEMMs start at 256 rows);
  * with a model whose stop bias lets a take run into its cap, that take ranks last;
  * BatchPipeline.submit(takes=3, keep=1) ranks through generate(num_return_sequences=3, return_logprobs=True);
  * IndexTTS2.infer(best_of=3) equals the plain stages on the winning take's codes."""
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu


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


def _recording(tts, seen):
    stage = tts.gpt_stage

    def recording(t, c, **kw):
        if kw.get("codes") is not None:
            seen.append(kw["codes"].clone())
        return stage(t, c, **kw)
    tts.gpt_stage = recording
    return stage


def test_continuous_pipeline_keep_returns_the_ranked_take(device):
    from indextts_amd.gpt import rank_takes, sequence_scores
    from indextts_amd.serving import ContinuousPipeline, utterance_noise_seeds
    cfg, tts, cond = _tts(device, "t/takes/pipe", stop_bias=2.0)      # (the model, prompt and text of test_takes_gpu.py's pipeline test)
    stop = cfg.gpt.stop_mel_token
    B, n, L, cap, S, T = 2, 3, 7, 14, 21, 9
    text = torch.from_numpy(synth.integers("t/takes/pipe/text", (B, L), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9}
    seen = []
    stage = _recording(tts, seen)
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True) as pipe:
                full = pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n).result()
            codes_full = seen.pop()
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True, scores=True) as pipe:
                pipe.trace = []
                fut = pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n, keep=1)
                best = fut.result()
                rows_run = [e[3] for e in pipe.trace if e[0] == "acoustic"]
                # all three takes again, from the scored sessions: the scores change no code
                again = pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n).result()
            codes_again, codes_best = seen.pop(), seen.pop()
            assert not seen and rows_run == [B]      # one row per utterance reached the acoustic stage
            assert torch.equal(codes_again, codes_full)
            ranking = fut.ranking
            assert len(best) == B and all(len(r) == 1 for r in best) and len(ranking) == B
            singles = []
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True) as pipe:
                for i in range(B):
                    r = i * n + ranking[i][0][0]
                    g = torch.Generator().manual_seed(S)
                    for _ in range(r):          # utterance_samplers draws the seeds in row order
                        torch.randint(0, 2 ** 62, (1,), generator=g)
                    (w,) = pipe.submit(text[i:i + 1], cond, max_mel_tokens=cap, sampling=dict(samp, generator=g),
                                       noise_seed=[utterance_noise_seeds(T, B * n)[r]]).result()
                    singles.append(w)
                    seen.pop()
    finally:
        tts.gpt_stage = stage
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    for i in range(B):
        rk = ranking[i]
        assert sorted(t for t, *_ in rk) == list(range(n))
        take = rk[0][0]
        # the ranking restated from the full request's codes: n_codes and stopped per take, the order by rank_takes
        rows = [codes_full[i * n + t] for t in range(n)]
        lens = [int((row == stop).nonzero()[0]) + 1 if (row == stop).any() else cap for row in rows]
        by_take = {t: (sc, st, nc) for t, sc, st, nc in rk}
        assert [by_take[t][2] for t in range(n)] == lens and [by_take[t][1] for t in range(n)] == [bool((row == stop).any()) for row in rows]
        assert [t for t, *_ in rk] == rank_takes([by_take[t][0] for t in range(n)], [by_take[t][1] for t in range(n)])
        assert all(np.isfinite(sc) and sc < 0 for sc, _, _ in by_take.values())
        # the kept codes are that take's, and the waveform is the one a request of that take alone gives
        k = lens[take]
        assert torch.equal(codes_best[i, :k], codes_full[i * n + take, :k]) and (codes_best[i, k:] == stop).all()
        assert torch.equal(best[i][0].cpu(), singles[i].cpu()), i
        assert torch.equal(best[i][0].cpu(), full[i][take].cpu()), i      # submit(takes=3) at that index
    assert len({tuple(c.tolist()) for c in codes_full[:n]}) > 1, "the takes of one utterance are all equal: the test shows nothing"
    assert sequence_scores([[-1.0, -3.0]], [2])[0] == -2.0


def test_a_take_that_runs_into_its_cap_ranks_last(device):
    """Eight takes per request, caps from 2 to 14 codes: under the short caps most takes are cut off, under the long ones most stop, and
    in between both kinds meet in one request.  Every truncated take stands below every stopped one, whatever its score."""
    from indextts_amd.serving import ContinuousPipeline
    cfg, tts, cond = _tts(device, "t/scores/cap", stop_bias=2.0)
    text = torch.from_numpy(synth.integers("t/scores/cap/text", (1, 7), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 1.0, "top_k": 30, "top_p": 0.9}
    caps = (2, 3, 4, 6, 8, 11, 14)
    mixed = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=8, poll_steps=4, max_new=14, allow_sampling=True, scores=True) as pipe:
            futs = [pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=cap), noise_seed=1, takes=8, keep=2) for cap in caps]
            for cap, f in zip(caps, futs):
                try:
                    res = f.result()
                    assert len(res) == 1 and len(res[0]) == 2
                except RuntimeError as e:      # a kept take that is the stop token alone has nothing to synthesise: the request says so
                    assert "stop token first" in str(e) and any(nc == 1 for _, _, _, nc in f.ranking[0][:2])
                flags = [st for _, _, st, _ in f.ranking[0]]
                assert flags == sorted(flags, reverse=True), "a truncated take ranks above a stopped one"
                assert all(nc == cap for _, _, st, nc in f.ranking[0] if not st) and all(1 <= nc <= cap for _, _, _, nc in f.ranking[0])
                for grp in (True, False):      # inside each group: by score, then by index
                    g = [(sc, t) for t, sc, st, _ in f.ranking[0] if st == grp]
                    assert g == sorted(g, key=lambda x: (-x[0], x[1]))
                mixed += 0 < sum(flags) < 8
    assert mixed, "no request had both stopped and truncated takes: the test shows nothing"


def test_batch_pipeline_keep_and_infer_best_of(device):
    from indextts_amd.serving import BatchPipeline, utterance_noise_seeds
    cfg, tts, cond = _tts(device, "t/scores/batch", stop_bias=1.0)
    B, n, cap = 2, 3, 14
    text = torch.from_numpy(synth.integers("t/scores/batch/text", (B, 7), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9}
    seeds = utterance_noise_seeds(5, B * n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(11)
        codes, ranking = tts.ranked_takes(text, cond, n, max_mel_tokens=cap, sampling=samp)
        with BatchPipeline(tts, decode_lanes=1) as pipe:
            with pytest.raises(ValueError, match="1 .. takes"):
                pipe.submit(text, cond, max_mel_tokens=cap, sampling=samp, takes=n, keep=4)
            with pytest.raises(ValueError, match="sampled takes"):
                pipe.submit(text, cond, max_mel_tokens=cap, keep=1)
            torch.manual_seed(11)      # (the request's draws are seeded from torch's global generator when it decodes)
            fut = pipe.submit(text, cond, max_mel_tokens=cap, sampling=samp, noise_seed=5, takes=n, keep=2)
            res = fut.result()
        assert fut.ranking == ranking and len(res) == B and all(len(r) == 2 for r in res)
        rows = [i * n + ranking[i][q][0] for i in range(B) for q in range(2)]
        want = tts.acoustic_stage(tts.gpt_stage(text.repeat_interleave(n, 0)[rows], cond, max_mel_tokens=cap, codes=codes[rows]),
                                  noise_seeds=[seeds[r] for r in rows])
        for q, w in enumerate(w for r in res for w in r):
            assert torch.equal(w.cpu(), want[q].cpu()), q
        # infer(best_of=3): one segment; the plain stages on the winning take's codes, with the same noise seed
        seg = text[0].tolist()
        kw = dict(max_mel_tokens=cap, do_sample=True, top_p=0.9, top_k=30, temperature=0.9, num_beams=1, noise_seed=3)
        torch.manual_seed(12)
        sr, audio = tts.infer(cond, seg, None, best_of=n, **kw)
        torch.manual_seed(12)
        c1, rk1 = tts.ranked_takes(text[:1], cond, n, max_mel_tokens=cap, sampling=dict(samp, sampler="hf"))
        assert tts.last_ranking == rk1
        (w1,) = tts.acoustic_stage(tts.gpt_stage(text[:1], cond, max_mel_tokens=cap, codes=c1[[rk1[0][0][0]]]),
                                   noise_seeds=utterance_noise_seeds(3, 1))
        assert np.array_equal(audio[:, 0], w1.cpu()[0].to(torch.int16).numpy())
        # streaming keeps its contract; the refusals
        chunks = list(tts.infer(cond, seg, None, best_of=n, stream_return=True, **kw))
        assert len(chunks) == 2 and chunks[0].shape[0] == 1
        with pytest.raises(ValueError, match="best_of"):
            tts.infer(cond, seg, None, best_of=n, max_mel_tokens=cap)                       # the default mode is beam-sample
        with pytest.raises(ValueError, match="best_of"):
            tts.infer(cond, seg, None, best_of=n, do_sample=False, num_beams=1)
        with pytest.raises(ValueError, match="best_of"):
            tts.infer(cond, seg, None, best_of=n, takes=2, **kw)
