"""CPU: what `stop` on a beam group rests on.  A group stopped after k steps is read out as BeamSearchScorer.finalize at k steps, which
is claimed to equal generate_beam with max_new_tokens = k.  That holds if nothing the beam loop keeps after k steps -- beam ancestry,
tokens, running scores, the finished hypotheses -- depends on the cap.  Checked here on oracle.gpt.generate_beam: its first k steps with
a larger cap are its k steps with cap k, bit for bit (ancestry, tokens and scores are compared; the hypotheses' lists are filled from
those steps' candidates alone), and the codes of the capped run are finalize on that state.  The cap enters generate_beam in two
places only: the loop's exit and the length of the returned row."""
import pytest
import torch

from indextts_amd import synth, weights
from indextts_amd.config import GPTConfig
from oracle import gpt as og


@pytest.mark.parametrize("do_sample,stop_bias", [(True, -1e4), (False, -1e4), (True, 3.0), (False, 3.0)])
def test_beam_state_after_k_steps_does_not_depend_on_the_cap(do_sample, stop_bias):
    cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=70, number_text_tokens=40, start_mel_token=68, stop_mel_token=69,
                    max_mel_tokens=60, max_text_tokens=30, cond_latents=4)
    w = weights.synth_gpt_weights(cfg, tag="t/cancel/oracle")
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] += stop_bias      # 3.0: hypotheses finish along the way (the scorer's lists fill up)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    nb, CAP, V = 3, 14, cfg.number_mel_codes
    lat = torch.from_numpy(synth.uniform("t/cancel/oracle/lat", (1, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/cancel/oracle/emo", (1, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/cancel/oracle/text", (1, 7), 2, cfg.number_text_tokens))
    noise = torch.empty(CAP, 1, nb * V).exponential_(1.0, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        conds = og.conds_latent(tw, cfg, lat, emo)
        run = lambda cap: og.generate_beam(tw, cfg, conds, text, cap, noise[:cap], num_beams=nb, do_sample=do_sample, return_trace=True)
        _, full = run(CAP)
        for k in (1, 2, 5, 9):
            if k > len(full):       # the scorer was done before k steps: there is no live group to stop
                continue
            codes_k, trace_k = run(k)
            assert len(trace_k) == k
            for t in range(k):
                for a, b in zip(full[t][:3], trace_k[t][:3]):      # beam_idx, tokens, running scores
                    assert torch.equal(a, b), (k, t)
            assert codes_k.shape[1] <= k
