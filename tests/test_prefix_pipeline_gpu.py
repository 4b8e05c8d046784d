"""GPU: ContinuousPipeline(prefix=True).submit(prefix_codes=) on the tiny synthetic pipeline.  A session's seeded draws are keyed by
the absolute step, so an utterance continued from the first k codes of its own earlier run, with the same seed, must return that run:
  * alone and among other requests the codes handed to gpt_stage(codes=) are the uninterrupted run's -- prefix + continuation -- and
    the waveform is gpt_stage(codes=) + acoustic_stage of them on the same noise seed;
  * takes=3 share the prefix (and differ behind it); a cancelled prefixed request frees its slots."""
import warnings

import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu
TAG = "t/prefix/pipe"


def _tts(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag=f"{TAG}/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -30.0      # every row runs to its cap: no prefix holds the stop token
    wg["mel_head.bias"][cfg.gpt.start_mel_token] = -1e4      # a sampled start token is no semantic code
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag=f"{TAG}/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag=f"{TAG}/voc"), device=device)
    return cfg, tts, PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"{TAG}/prompt").to(device)


def test_prefixed_requests_through_the_pipeline(device):
    from indextts_amd.serving import ContinuousPipeline, utterance_noise_seeds
    cfg, tts, cond = _tts(device)
    B, L, cap, S, T, k = 2, 7, 12, 21, 9, 5
    text = torch.from_numpy(synth.integers(f"{TAG}/text", (B, L), 2, cfg.gpt.number_text_tokens))
    other = torch.from_numpy(synth.integers(f"{TAG}/other", (3, L + 2), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9}
    seen, stage = [], tts.gpt_stage

    def recording(t, c, **kw):
        if kw.get("codes") is not None:
            seen.append((int(torch.as_tensor(t).shape[0]), kw["codes"].clone().cpu()))
        return stage(t, c, **kw)
    tts.gpt_stage = recording
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ContinuousPipeline(tts, slots=8, poll_steps=3, max_new=16, allow_sampling=True, prefix=True) as pipe:
                kw = dict(max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T)
                full = pipe.submit(text, cond, **kw).result()
                (_, codes_full), = seen
                assert codes_full.shape == (B, cap)
                del seen[:]
                pfx = [codes_full[0, :k], None]
                alone = pipe.submit(text, cond, prefix_codes=pfx, **kw).result()
                (_, codes_alone), = seen
                del seen[:]
                futs = [pipe.submit(other, cond, max_mel_tokens=cap - 3), pipe.submit(text, cond, prefix_codes=[codes_full[0, :k], codes_full[1, :cap - 1]], **kw),
                        pipe.submit(other[:1], cond, max_mel_tokens=cap, sampling=dict(samp, seed=2))]
                among = futs[1].result()
                for f in futs:
                    f.result()
                (codes_among,) = [c for n, c in seen if n == B]
                del seen[:]
                # three takes of utterance 0 behind its prefix
                takes = pipe.submit(text[:1], cond, prefix_codes=[codes_full[0, :k]], takes=3, **kw).result()
                (_, codes_takes), = seen
                del seen[:]
                # a cancelled prefixed request gives its slots back: a request that needs all eight follows it
                gone = pipe.submit(text.repeat(4, 1), cond, max_mel_tokens=16, prefix_codes=[codes_full[0, :k]] * 8)
                pipe.cancel(gone)
                after = pipe.submit(text.repeat(4, 1), cond, max_mel_tokens=4).result()
            want = tts.acoustic_stage(stage(text, cond, max_mel_tokens=cap, codes=codes_full.to(device)), noise_seeds=utterance_noise_seeds(T, B))
    finally:
        tts.gpt_stage = stage
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert torch.equal(codes_alone, codes_full) and torch.equal(codes_among, codes_full)      # prefix + continuation = the uninterrupted run
    for res in (full, alone, among):
        assert len(res) == B and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(res, want))
    assert codes_takes.shape == (3, cap) and bool((codes_takes[:, :k] == codes_full[0, :k]).all())
    assert len({tuple(r) for r in codes_takes[:, k:].tolist()}) > 1 and len(takes) == 1 and len(takes[0]) == 3
    assert gone.cancelled() or gone.done()
    assert len(after) == 8
