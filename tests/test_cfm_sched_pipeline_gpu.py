"""GPU: per-request diffusion steps and CFG rates through IndexTTS2 and the serving pipelines, on the tiny synthetic weights of
tests/test_noise_seed_gpu.py.  Requests with different settings share ONE acoustic batch (the per-row solver, idxtts_s2mel_cfm_sched) and
every waveform equals the stages run on that request alone with its values; a request without values keeps the path of before.

Exact GEMM mode, seeded noise: there kernel selection does not depend on the row count and a row of a merged batch equals its own run bit
for bit."""
import threading
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig
from indextts_amd.serving import utterance_noise_seeds

pytestmark = pytest.mark.gpu

SLOTS = 4
SETTINGS = [(3, 0.7), (1, 0.0), (2, 1.5), None]      # (diffusion_steps, cfg_rate) per request; None: neither given


class _exact_gemm:
    def __enter__(self):
        self.old = _lib.get_gemm_mode()
        _lib.set_gemm_mode(_lib.GEMM_F32)

    def __exit__(self, *exc):
        _lib.set_gemm_mode(self.old)


def _kw(k):
    return {} if SETTINGS[k] is None else {"diffusion_steps": SETTINGS[k][0], "cfg_rate": SETTINGS[k][1]}


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/csched/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 2.0          # some rows stop early, some run to their cap
    wg["mel_head.bias"][cfg.gpt.start_mel_token] = -1e4        # a sampled start token is no semantic code
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/csched/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/csched/voc"), device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=p, tag=f"t/csched/prompt{p}").to(device) for p in (40, 23)]
    return cfg, tts, conds


@pytest.fixture(scope="module")
def served(setup):
    """Four one-row requests over the two prompts with SETTINGS; per request its reference codes (row 0 of generate on SLOTS copies of
    the utterance, the decode session's contract) and the stages run alone on them with the request's seed and values."""
    cfg, tts, conds = setup
    reqs = []
    for k in range(4):
        L = 5 + 3 * k
        text = torch.from_numpy(synth.integers(f"t/csched/text{k}", (1, L), 2, cfg.gpt.number_text_tokens))
        reqs.append({"text": text, "cond": conds[k % 2], "cap": 12, "seed": 300 + k})
    gpt, stop = tts.gpt, cfg.gpt.stop_mel_token
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, r in enumerate(reqs):
            c = r["cond"]
            (row,) = gpt.prompt_rows(gpt.conds_latent(c.spk_cond_latent, c.emo_vec), r["text"])
            P, d = row.shape
            ids = torch.ones(SLOTS, P + 1, dtype=torch.long)
            ids[:, -1] = cfg.gpt.start_mel_token
            r["codes"] = gpt.generate(ids, max_new_tokens=r["cap"], tts_embeddings=row[None].expand(SLOTS, P, d).contiguous())[0, P + 1:].cpu()[None]
            st = tts.gpt_stage(r["text"], c, max_mel_tokens=r["cap"], codes=r["codes"])
            r["want"] = tts.acoustic_stage(st, noise_seeds=utterance_noise_seeds(r["seed"], 1), **_kw(k))
            r["plain"] = tts.acoustic_stage(st, noise_seeds=utterance_noise_seeds(r["seed"], 1))
    torch.cuda.synchronize()
    assert stop >= 0
    return tts, reqs


def test_settings_change_the_audio(served):
    tts, reqs = served
    for k in range(4):      # (request 0's values are the tiny configuration's own: 3 steps, rate 0.7)
        same = SETTINGS[k] is None or SETTINGS[k] == (tts._diffusion_steps, tts._cfg_rate)
        assert reqs[k]["want"][0].shape == reqs[k]["plain"][0].shape and torch.equal(reqs[k]["want"][0], reqs[k]["plain"][0]) == same, k
    assert [SETTINGS[k] is None or SETTINGS[k] == (tts._diffusion_steps, tts._cfg_rate) for k in range(4)] == [True, False, False, True]


def test_acoustic_stage_argument_rules(setup):
    cfg, tts, conds = setup
    text = torch.from_numpy(synth.integers("t/csched/rules", (2, 6), 2, cfg.gpt.number_text_tokens))
    codes = torch.from_numpy(synth.integers("t/csched/rules/codes", (2, 7), 0, cfg.s2mel.codebook_size))
    with _exact_gemm():
        st = tts.gpt_stage(text, conds[0], codes=codes)
        for kw in (dict(diffusion_steps=[2]), dict(diffusion_steps=[2, 2, 2]), dict(cfg_rate=[0.7]), dict(diffusion_steps=0),
                   dict(cfg_rate=-0.1), dict(cfg_rate=[0.1, float("nan")])):
            with pytest.raises(ValueError):
                tts.acoustic_stage(st, noise_seeds=[1, 2], **kw)
        # a scalar applies to every row; the same values per row give the same audio (two entries of the library, exact mode)
        a = tts.acoustic_stage(st, noise_seeds=[1, 2], diffusion_steps=2, cfg_rate=0.7)
        b = tts.acoustic_stage(st, noise_seeds=[1, 2], diffusion_steps=[2, 2], cfg_rate=[0.7, 0.7])
        c = tts.synthesize_batch(text, conds[0], noise_seeds=[1, 2], diffusion_steps=[2, 1], cfg_rate=0.0, max_mel_tokens=7)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(c) == 2


def test_continuous_pipeline_merges_requests_with_different_settings(served):
    from indextts_amd.serving import ContinuousPipeline
    tts, reqs = served
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # every row fits the session and ends inside the first poll (poll_steps = the cap): one admission, one finishing poll
        with ContinuousPipeline(tts, slots=SLOTS, decode_lanes=1, poll_steps=12, max_new=12, acoustic_coalesce=4, acoustic_max_rows=8) as pipe:
            pipe.trace = []
            with pipe._cv:          # queued as one: the lane sees all four or none
                futs = [pipe.submit(r["text"], r["cond"], max_mel_tokens=r["cap"], noise_seed=r["seed"], **_kw(k)) for k, r in enumerate(reqs)]
            got = [f.result(timeout=600) for f in futs]
            jobs = [t for t in pipe.trace if t[0] == "acoustic"]
            alone = pipe.submit(reqs[3]["text"], reqs[3]["cond"], max_mel_tokens=12, noise_seed=reqs[3]["seed"]).result(timeout=600)
    assert len(jobs) == 1 and jobs[0][3] == 4 and len(jobs[0][4]) == 4, jobs          # ONE acoustic batch of the four requests
    for k, r in enumerate(reqs):
        assert len(got[k]) == 1 and torch.equal(got[k][0], r["want"][0]), k
    assert torch.equal(alone[0], reqs[3]["plain"][0])


def test_batch_pipeline_merges_requests_with_different_settings(served):
    """BatchPipeline decodes a request as its own batch: its reference is synthesize_batch alone with the request's seed and values."""
    from indextts_amd.serving import BatchPipeline
    tts, reqs = served
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [tts.synthesize_batch(r["text"], r["cond"], max_mel_tokens=r["cap"], noise_seeds=utterance_noise_seeds(r["seed"], 1), **_kw(k))
                for k, r in enumerate(reqs)]
        plain = tts.synthesize_batch(reqs[3]["text"], reqs[3]["cond"], max_mel_tokens=12, noise_seeds=utterance_noise_seeds(reqs[3]["seed"], 1))
        torch.cuda.synchronize()
        with BatchPipeline(tts, decode_lanes=1, acoustic_workers=1, acoustic_coalesce=4, acoustic_mix_prompts=True) as pipe:
            pipe.trace = []
            hold = threading.Event()
            pipe._acoustic.submit(hold.wait, 600)          # the one acoustic worker stands here while the four requests are decoded
            futs = [pipe.submit(r["text"], r["cond"], max_mel_tokens=r["cap"], noise_seed=r["seed"], **_kw(k)) for k, r in enumerate(reqs)]
            pipe._lanes.submit(lambda: None).result(timeout=600)      # the one lane is through its four decodes
            assert len(pipe._aq) == 4
            hold.set()
            got = [f.result(timeout=600) for f in futs]
            jobs = [t for t in pipe.trace if t[0] == "acoustic"]
            alone = pipe.submit(reqs[3]["text"], reqs[3]["cond"], max_mel_tokens=12, noise_seed=reqs[3]["seed"]).result(timeout=600)
    assert len(jobs) == 1 and jobs[0][3] == 4, jobs
    for k in range(4):
        assert len(got[k]) == 1 and torch.equal(got[k][0], want[k][0]), k
    assert torch.equal(alone[0], plain[0]) and torch.equal(plain[0], want[3][0])


def test_keep_keeps_the_kept_takes_value(setup):
    from indextts_amd.serving import ContinuousPipeline
    cfg, tts, conds = setup
    text = torch.from_numpy(synth.integers("t/csched/keep/text", (1, 7), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9, "seed": 21}
    given, T = [1, 3], 9
    seen = []
    gpt_stage, acoustic_stage = tts.gpt_stage, tts.acoustic_stage

    def rec_gpt(t, c, **kw):
        seen.append(("codes", kw["codes"].clone()))
        return gpt_stage(t, c, **kw)

    def rec_acoustic(st, **kw):
        seen.append(("steps", st.get("diffusion_steps"), st.get("cfg_rate")))
        return acoustic_stage(st, **kw)
    tts.gpt_stage, tts.acoustic_stage = rec_gpt, rec_acoustic
    try:
        with _exact_gemm(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ContinuousPipeline(tts, slots=SLOTS, poll_steps=3, max_new=24, allow_sampling=True, scores=True) as pipe:
                fut = pipe.submit(text, conds[0], max_mel_tokens=14, sampling=samp, noise_seed=T, takes=2, keep=1, diffusion_steps=given)
                (best,) = fut.result(timeout=600)
            take = fut.ranking[0][0][0]
            tts.gpt_stage, tts.acoustic_stage = gpt_stage, acoustic_stage
            (_, codes), (_, steps, rates) = seen
            assert steps == [given[take]] and rates is None
            st = tts.gpt_stage(text, conds[0], max_mel_tokens=14, codes=codes)
            want = tts.acoustic_stage(st, noise_seeds=[utterance_noise_seeds(T, 2)[take]], diffusion_steps=given[take])
            other = tts.acoustic_stage(st, noise_seeds=[utterance_noise_seeds(T, 2)[take]], diffusion_steps=given[1 - take])
    finally:
        tts.gpt_stage, tts.acoustic_stage = gpt_stage, acoustic_stage
    assert len(best) == 1 and torch.equal(best[0], want[0]) and not torch.equal(best[0], other[0])


def test_infer_takes_steps_and_rate_per_call(setup):
    cfg, tts, conds = setup
    segs = synth.integers("t/csched/seg", (2, 6), 2, cfg.gpt.number_text_tokens).tolist()
    G = dict(do_sample=False, num_beams=1, max_mel_tokens=12)
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = tts.infer(conds[0], segs, None, noise_seed=5, diffusion_steps=2, cfg_rate=0.0, **G)[1]
        default = tts.infer(conds[0], segs, None, noise_seed=5, **G)[1]
        # the staged calls with those values: segment i has seed i of utterance_noise_seeds(5, 2), with the silence between the two
        seeds = utterance_noise_seeds(5, 2)
        toks = torch.tensor(segs, dtype=torch.long)
        wavs = tts.acoustic_stage(tts.gpt_stage(toks, conds[0], max_mel_tokens=12, sampling={"do_sample": False, "num_beams": 1}),
                                  noise_seeds=seeds, diffusion_steps=2, cfg_rate=0.0)
        want = torch.cat([wavs[0], tts.interval_silence(), wavs[1]], dim=1).cpu().to(torch.int16).numpy().T
        with pytest.raises(TypeError):
            tts.infer(conds[0], segs, None, noise_seed=5, diffusion_step=2, **G)
        with pytest.raises(ValueError):
            tts.infer(conds[0], segs, None, noise_seed=5, diffusion_steps=[2, 2], **G)
    assert np.array_equal(got, want)
    assert got.shape == default.shape and not np.array_equal(got, default)
