"""GPU: per-utterance CFM noise seeds through the layers, on tiny synthetic weights built as in test_continuous_serving_gpu.py --
acoustic_stage(noise_seeds=) against acoustic_stage(noise=S2Mel.noise(...)) on both CFM paths, the argument rules, and
ContinuousPipeline / BatchPipeline / infer with seeds and no noise tensor against the stages run alone.

The pipelines merge acoustic batches here (acoustic_coalesce > 1), so their comparisons run in the exact GEMM mode: there kernel
selection does not depend on the row count and a row of a merged batch equals its own run bit for bit (INTEGRATION.md §4a,
tests/test_mixed_prompt_acoustic_gpu.py)."""
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig
from indextts_amd.serving import utterance_noise_seeds

pytestmark = pytest.mark.gpu

SLOTS = 4


class _exact_gemm:
    def __enter__(self):
        self.old = _lib.get_gemm_mode()
        _lib.set_gemm_mode(_lib.GEMM_F32)

    def __exit__(self, *exc):
        _lib.set_gemm_mode(self.old)


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/nseed/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 2.0          # some rows stop early, some run to their cap
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/nseed/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/nseed/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=p, tag=f"t/nseed/prompt{p}").to(device) for p in (40, 23)]
    return cfg, tts, conds


@pytest.fixture(scope="module")
def served(setup):
    """Seven ragged requests over the two prompts; per request its reference codes (row 0 of generate on SLOTS copies of each
    utterance, the decode session's contract) and the stages run alone on them with the request's own seeds.  Exact GEMM mode."""
    cfg, tts, conds = setup
    reqs = []
    for k in range(7):
        B, L = 1 + k % 3, 4 + (5 * k) % 17
        text = torch.from_numpy(synth.integers(f"t/nseed/text{k}", (B, L), 2, cfg.gpt.number_text_tokens))
        if B > 1:
            text[1, L - 2:] = cfg.gpt.stop_text_token     # a shorter row inside the request
        reqs.append({"text": text, "cond": conds[k % 2], "cap": 8 + (11 * k) % 25, "seed": 100 + k})
    gpt = tts.gpt
    stop = cfg.gpt.stop_mel_token
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in reqs:
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
            r["want"] = tts.acoustic_stage(st, noise_seeds=utterance_noise_seeds(r["seed"], r["text"].shape[0]))
    torch.cuda.synchronize()
    return tts, reqs


def _state(cfg, tts, cond, lens, tag):
    """gpt_stage's state for given (ragged) code lengths."""
    B = len(lens)
    text = torch.from_numpy(synth.integers(f"{tag}/text", (B, 9), 2, cfg.gpt.number_text_tokens))
    codes = torch.full((B, max(lens)), cfg.gpt.stop_mel_token, dtype=torch.long)
    for b, n in enumerate(lens):
        codes[b, :n] = torch.from_numpy(synth.integers(f"{tag}/codes{b}", (n,), 0, cfg.s2mel.codebook_size))
    return tts.gpt_stage(text, cond, codes=codes)


@pytest.mark.parametrize("mixed", [False, True], ids=["cfm_inference", "cfm_rows"])
def test_seeded_stage_equals_the_stage_on_its_noise_tensor(device, setup, mixed):
    cfg, tts, conds = setup
    lens = [9, 17, 12]
    seeds = [5, 2 ** 64 - 1, 2 ** 63 + 12345]
    rows = [conds[0], conds[1], conds[0]] if mixed else [conds[0]] * 3
    st = _state(cfg, tts, rows if mixed else conds[0], lens, "t/nseed/stage%d" % mixed)
    assert isinstance(st["cond"], list) == mixed
    gpu_rng, cpu_rng = torch.cuda.get_rng_state(device), torch.get_rng_state()
    got, mid = tts.acoustic_stage(st, noise_seeds=seeds, per_row_noise=True, return_intermediates=True)
    torch.cuda.synchronize()
    assert torch.equal(gpu_rng, torch.cuda.get_rng_state(device)) and torch.equal(cpu_rng, torch.get_rng_state())
    x_lens = [int(c.prompt_condition.shape[1]) + t for c, t in zip(rows, mid["target_lens"])]
    assert len(set(x_lens)) == 3
    noise = tts.s2mel.noise(seeds, x_lens)
    assert noise.shape == (3, cfg.s2mel.in_channels, max(x_lens))
    want = tts.acoustic_stage(st, noise=noise)
    for b in range(3):
        assert torch.equal(got[b], want[b]), b
        assert np.isfinite(got[b].cpu().numpy()).all() and float(got[b].abs().max()) > 0
    other = tts.acoustic_stage(st, noise_seeds=[6] + seeds[1:])
    assert not torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])
    with pytest.raises(ValueError):
        tts.acoustic_stage(st, noise=noise, noise_seeds=seeds)
    with pytest.raises(ValueError):
        tts.acoustic_stage(st, noise_seeds=seeds[:2])


def test_s2mel_argument_rules(device, setup):
    cfg, tts, conds = setup
    sm, c = tts.s2mel, conds[0]
    Tp = c.prompt_condition.shape[1]
    z = sm.noise([1, 2], [Tp + 3, Tp + 5])
    assert z.shape == (2, cfg.s2mel.in_channels, Tp + 5) and bool((z[0, :, Tp + 3:] == 0).all())
    assert sm.noise([1], [4], T=9).shape == (1, cfg.s2mel.in_channels, 9)
    mu = torch.zeros(2, Tp + 5, cfg.s2mel.content_dim, device=device)
    with pytest.raises(ValueError):
        sm.cfm_inference(mu, [Tp + 3, Tp + 5], c.ref_mel.expand(2, -1, -1), c.style.expand(2, -1), None, 2, z=z, noise_seeds=[1, 2])
    with pytest.raises(ValueError):
        sm.cfm_rows(mu[:, :5], [3, 5], [c.prompt_condition] * 2, [c.ref_mel] * 2, c.style.expand(2, -1), 2, z=z, noise_seeds=[1, 2])
    with pytest.raises(ValueError):
        sm.noise([1, 2 ** 64], [3, 4])
    with pytest.raises(ValueError):
        sm.noise([1], [3, 4])
    # temperature scales the seeded draw as it scales torch's
    a = sm.cfm_inference(mu, [Tp + 3, Tp + 5], c.ref_mel.expand(2, -1, -1), c.style.expand(2, -1), None, 2, noise_seeds=[1, 2], temperature=0.5)
    b = sm.cfm_inference(mu, [Tp + 3, Tp + 5], c.ref_mel.expand(2, -1, -1), c.style.expand(2, -1), None, 2, z=z * 0.5)
    assert torch.equal(a, b)


def _same(got, reqs):
    for k, r in enumerate(reqs):
        assert len(got[k]) == len(r["want"])
        for a, b in zip(got[k], r["want"]):
            assert torch.equal(a, b), k


@pytest.mark.parametrize("lanes,reverse", [(1, False), (1, True), (2, False)])
def test_continuous_pipeline_with_seeds_equals_stages_on_reference_codes(served, lanes, reverse):
    """Seeds and no noise tensor: requests are merged as they finish (up to 3 requests, 8 rows, both prompts in one batch) and every
    waveform is still that of the stages run alone, whatever the submission order or the number of lanes."""
    from indextts_amd.serving import ContinuousPipeline
    tts, reqs = served
    order = list(range(len(reqs)))[::-1 if reverse else 1]
    got = [None] * len(reqs)
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=SLOTS, decode_lanes=lanes, poll_steps=3, max_new=40, acoustic_coalesce=3,
                                acoustic_max_rows=8) as pipe:
            pipe.trace = []
            futs = {k: pipe.submit(reqs[k]["text"], reqs[k]["cond"], max_mel_tokens=reqs[k]["cap"], noise_seed=reqs[k]["seed"]) for k in order}
            for k, f in futs.items():
                got[k] = f.result(timeout=600)
            trace = list(pipe.trace)
    assert all(len(t[4]) <= 3 and t[3] <= 8 for t in trace)
    _same(got, reqs)


def test_batch_pipeline_with_seeds_equals_sequential(served):
    """BatchPipeline decodes a request as its own batch, so its reference is synthesize_batch alone with the request's seeds."""
    from indextts_amd.serving import BatchPipeline
    tts, reqs = served
    with _exact_gemm(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [tts.synthesize_batch(r["text"], r["cond"], max_mel_tokens=r["cap"],
                                     noise_seeds=utterance_noise_seeds(r["seed"], r["text"].shape[0])) for r in reqs]
        torch.cuda.synchronize()
        with BatchPipeline(tts, decode_lanes=2, acoustic_coalesce=2, acoustic_mix_prompts=True) as pipe:
            futs = [pipe.submit(r["text"], r["cond"], max_mel_tokens=r["cap"], noise_seed=r["seed"]) for r in reqs]
            got = [f.result(timeout=600) for f in futs]
            bad = pipe.submit(reqs[0]["text"], reqs[0]["cond"], max_mel_tokens=8, noise=torch.zeros(1), noise_seed=1)
            with pytest.raises(ValueError):
                bad.result(timeout=60)
    for k in range(len(reqs)):
        assert len(got[k]) == len(want[k])
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k


def test_infer_noise_seed(device, setup):
    cfg, tts, conds = setup
    segs = synth.integers("t/nseed/seg", (3, 6), 2, cfg.gpt.number_text_tokens).tolist()
    G = dict(do_sample=False, num_beams=1, max_mel_tokens=16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(1)
        a = tts.infer(conds[0], segs, None, noise_seed=5, **G)[1]
        torch.manual_seed(2)
        b = tts.infer(conds[0], segs, None, noise_seed=5, **G)[1]
        c = tts.infer(conds[0], segs, None, noise_seed=6, **G)[1]
        assert np.array_equal(a, b)
        assert a.shape == c.shape and not np.array_equal(a, c)
        # segment i has seed i of utterance_noise_seeds(5, 3): streaming, or one segment at a time, is the same audio
        with _exact_gemm():
            whole = tts.infer(conds[0], segs, None, noise_seed=5, **G)[1]
            parts = [w for w in tts.infer(conds[0], segs, None, noise_seed=5, stream_return=True, **G)]
            old, tts.segment_batch = tts.segment_batch, 2
            try:
                pairs = tts.infer(conds[0], segs, None, noise_seed=5, **G)[1]
            finally:
                tts.segment_batch = old
        streamed = torch.cat(parts[:-1], dim=1).to(torch.int16).numpy().T      # (the last yield is the trailing silence)
        assert np.array_equal(whole, streamed) and np.array_equal(whole, pairs)
        with pytest.raises(ValueError):
            tts.infer(conds[0], segs, None, noise_seed=[1, 2], **G)
