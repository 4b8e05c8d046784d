"""GPU: ContinuousPipeline (indextts_amd/serving.py) -- utterances of ragged requests with two different prompts share decode sessions;
every waveform equals acoustic_stage(gpt_stage(text, cond, codes=reference codes), noise), where the reference codes of an utterance are
row 0 of UnifiedVoice.generate on `slots` copies of its prompt (the decode session's contract, tests/test_decode_session_gpu.py)."""
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu

SLOTS = 4


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/cserve/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 2.0          # some rows stop early, some run to their cap
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/cserve/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/cserve/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"t/cserve/prompt{k}").to(device) for k in range(2)]
    reqs = []
    for k in range(7):
        B, L = 1 + k % 3, 4 + (5 * k) % 17
        text = torch.from_numpy(synth.integers(f"t/cserve/text{k}", (B, L), 2, cfg.gpt.number_text_tokens))
        if B > 1:
            text[1, L - 2:] = cfg.gpt.stop_text_token     # a shorter row inside the request
        cap = 8 + (11 * k) % 25
        reqs.append({"text": text, "cond": conds[k % 2], "cap": cap})
    # reference codes per utterance, then the noise of each request sized to its acoustic stage
    gpt = tts.gpt
    stop = cfg.gpt.stop_mel_token
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, r in enumerate(reqs):
            c = r["cond"]
            rows = gpt.prompt_rows(gpt.conds_latent(c.spk_cond_latent, c.emo_vec), r["text"])
            codes = []
            for row in rows:
                P, d = row.shape
                ids = torch.ones(SLOTS, P + 1, dtype=torch.long)
                ids[:, -1] = cfg.gpt.start_mel_token
                out = gpt.generate(ids, max_new_tokens=r["cap"], tts_embeddings=row[None].expand(SLOTS, P, d).contiguous())[0, P + 1:]
                codes.append(out.cpu())
            n = max(len(x) for x in codes)
            r["codes"] = torch.stack([torch.nn.functional.pad(x, (0, n - len(x)), value=stop) for x in codes])
            st = tts.gpt_stage(r["text"], c, max_mel_tokens=r["cap"], codes=r["codes"])
            condv, _ = tts.s2mel.prepare_condition(st["latent"], st["codes"], st["code_lens_t"])
            T = c.prompt_condition.shape[1] + condv.shape[1]
            r["noise"] = torch.from_numpy(synth.uniform(f"t/cserve/noise{k}", (r["text"].shape[0], cfg.s2mel.in_channels, T), 1.0)).to(device)
            r["want"] = tts.acoustic_stage(st, noise=r["noise"])
    torch.cuda.synchronize()
    return tts, reqs


def _run(tts, reqs, order, lanes):
    from indextts_amd.serving import ContinuousPipeline
    got = [None] * len(reqs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=SLOTS, decode_lanes=lanes, poll_steps=3, max_new=40) as pipe:
            futs = {k: pipe.submit(reqs[k]["text"], reqs[k]["cond"], max_mel_tokens=reqs[k]["cap"], noise=reqs[k]["noise"]) for k in order}
            for k, f in futs.items():
                got[k] = f.result(timeout=600)
    return got


@pytest.mark.parametrize("lanes,reverse", [(1, False), (1, True), (2, False)])
def test_continuous_pipeline_equals_stages_on_reference_codes(setup, lanes, reverse):
    """Ragged requests, two prompts, per-request caps; the result does not depend on submission order or the number of lanes."""
    tts, reqs = setup
    order = list(range(len(reqs)))[::-1 if reverse else 1]
    got = _run(tts, reqs, order, lanes)
    for k, r in enumerate(reqs):
        assert len(got[k]) == len(r["want"])
        for a, b in zip(got[k], r["want"]):
            assert torch.equal(a, b), k


def test_bad_token_fails_only_its_own_request(setup):
    from indextts_amd.serving import ContinuousPipeline
    tts, reqs = setup
    bad = reqs[1]["text"].clone()
    bad[0, 1] = tts.cfg.gpt.number_text_tokens + 5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=SLOTS, poll_steps=4, max_new=40) as pipe:
            f0 = pipe.submit(reqs[0]["text"], reqs[0]["cond"], max_mel_tokens=reqs[0]["cap"], noise=reqs[0]["noise"])
            fb = pipe.submit(bad, reqs[1]["cond"], max_mel_tokens=reqs[1]["cap"], noise=reqs[1]["noise"])
            f2 = pipe.submit(reqs[2]["text"], reqs[2]["cond"], max_mel_tokens=reqs[2]["cap"], noise=reqs[2]["noise"])
            with pytest.raises(IndexError):
                fb.result(timeout=600)
            for f, k in ((f0, 0), (f2, 2)):
                for a, b in zip(f.result(timeout=600), reqs[k]["want"]):
                    assert torch.equal(a, b), k
    assert np.isfinite(reqs[0]["want"][0].cpu().numpy()).all()
