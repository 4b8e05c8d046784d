"""GPU: ContinuousPipeline(num_beams=3) serves beam-sample and beam-search requests side by side.  Each utterance's codes equal row 0 of
UnifiedVoice.generate_beam on slots / num_beams copies of its prompt with its parameters and its seed (serving.utterance_beams), and
every waveform equals acoustic_stage(gpt_stage(text, cond, codes=those reference codes), noise)."""
import warnings

import pytest
import torch

from indextts_amd import synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu

NB, SLOTS = 3, 6
SAMPLINGS = [{"do_sample": True, "num_beams": NB, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0, "seed": 11},
             {"do_sample": False, "num_beams": NB, "length_penalty": 0.0},
             {"do_sample": True, "num_beams": NB, "temperature": 1.2, "top_k": 8, "top_p": 0.6, "generator": None, "seed": 13}]


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import utterance_beams
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/cbeam/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 2.0
    wg["mel_head.bias"][cfg.gpt.start_mel_token] = -1e4      # a sampled start token is no semantic code (the trained head never draws it)
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/cbeam/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/cbeam/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"t/cbeam/prompt{k}").to(device) for k in range(2)]
    gpt = tts.gpt
    stop = cfg.gpt.stop_mel_token
    reqs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(5):
            B, L = 1 + k % 2, 4 + (5 * k) % 17
            text = torch.from_numpy(synth.integers(f"t/cbeam/text{k}", (B, L), 2, cfg.gpt.number_text_tokens))
            if B > 1:
                text[1, L - 2:] = cfg.gpt.stop_text_token
            r = {"text": text, "cond": conds[k % 2], "cap": 8 + (11 * k) % 25, "sampling": SAMPLINGS[k % len(SAMPLINGS)]}
            c = r["cond"]
            rows = gpt.prompt_rows(gpt.conds_latent(c.spk_cond_latent, c.emo_vec), text)
            codes = []
            for row, b in zip(rows, utterance_beams(r["sampling"], B, NB)):
                P, d = row.shape
                G = SLOTS // NB
                ids = torch.ones(G, P + 1, dtype=torch.long)
                ids[:, -1] = cfg.gpt.start_mel_token
                out = gpt.generate_beam(ids, r["cap"], None, row[None].expand(G, P, d).contiguous(), num_beams=NB, do_sample=b["do_sample"],
                                        temperature=b["temperature"], top_k=b["top_k"], top_p=b["top_p"], repetition_penalty=10.0,
                                        length_penalty=b["length_penalty"], early_stopping=b["early_stopping"], seed=b["seed"])
                codes.append(out[0, P + 1:].cpu())
            n = max(len(x) for x in codes)
            r["codes"] = torch.stack([torch.nn.functional.pad(x, (0, n - len(x)), value=stop) for x in codes])
            st = tts.gpt_stage(text, c, max_mel_tokens=r["cap"], codes=r["codes"])
            condv, _ = tts.s2mel.prepare_condition(st["latent"], st["codes"], st["code_lens_t"])
            T = c.prompt_condition.shape[1] + condv.shape[1]
            r["noise"] = torch.from_numpy(synth.uniform(f"t/cbeam/noise{k}", (B, cfg.s2mel.in_channels, T), 1.0)).to(device)
            r["want"] = tts.acoustic_stage(st, noise=r["noise"])
            reqs.append(r)
    torch.cuda.synchronize()
    return tts, reqs


@pytest.mark.parametrize("lanes,reverse", [(1, False), (2, True)])
def test_beam_pipeline_equals_stages_on_reference_codes(setup, lanes, reverse):
    from indextts_amd.serving import ContinuousPipeline
    tts, reqs = setup
    order = list(range(len(reqs)))[::-1 if reverse else 1]
    got = [None] * len(reqs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=SLOTS, decode_lanes=lanes, poll_steps=3, max_new=40, num_beams=NB) as pipe:
            futs = {k: pipe.submit(reqs[k]["text"], reqs[k]["cond"], max_mel_tokens=reqs[k]["cap"], noise=reqs[k]["noise"],
                                   sampling=reqs[k]["sampling"]) for k in order}
            for k, f in futs.items():
                got[k] = f.result(timeout=600)
    for k, r in enumerate(reqs):
        assert len(got[k]) == len(r["want"])
        for a, b in zip(got[k], r["want"]):
            assert torch.equal(a, b), (k, r["sampling"])
