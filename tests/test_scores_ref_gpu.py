"""GPU: the per-code log-probabilities against the REFERENCE's own logits (tests/golden/gpt_ref.npz, `step_logits` / `step_codes` of
GPT2InferenceModel.forward: what tests/test_gpt_ref_gpu.py pins the logits and the greedy codes to).

The bound is 2 x 5e-4, twice the logits bound that file asserts: an error of eps in every logit moves l[tok] by at most eps and
log-sum-exp by at most eps, so lp = l[tok] - logsumexp(l) by at most 2 eps (the kernel's own arithmetic, ~5e-6, is far below)."""
import os

import numpy as np
import pytest
import torch

import scores_cases as sk
from indextts_amd import weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu


def test_greedy_logprobs_vs_reference_logits(golden_dir, device):
    from indextts_amd.gpt import UnifiedVoice
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    uv = UnifiedVoice(weights.synth_gpt_weights(cfg, tag="golden/gptref"), cfg, device=device)
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(device), torch.from_numpy(g["text"]))
    want_codes, ref_logits = g["step_codes"], g["step_logits"]      # [B, NEW], [NEW, B, V] or [B, NEW, V]
    B, NEW = want_codes.shape
    if ref_logits.shape[0] != B:
        ref_logits = ref_logits.transpose(1, 0, 2)
    ref = sk.ref_logprobs(ref_logits)      # float64 log-softmax, [B, NEW, V]
    worst = 0.0
    for graph in (False, True):
        out, lp = uv.generate(fake, max_new_tokens=NEW, stop_tokens=[cfg.stop_mel_token], attention_mask=mask, tts_embeddings=emb,
                              repetition_penalty=10.0, use_graph=graph, return_logprobs=True)
        codes = out[:, fake.shape[1]:].cpu().numpy()
        np.testing.assert_array_equal(codes, want_codes)      # the codes test_gpt_ref_gpu.py pins
        lp = lp.cpu().numpy().astype(np.float64)
        assert lp.shape == (B, NEW)
        for b in range(B):
            ended = False
            for t in range(NEW):
                if ended:
                    assert lp[b, t] == 0.0
                    continue
                err = abs(lp[b, t] - ref[b, t, codes[b, t]])
                worst = max(worst, err)
                assert err <= 2 * 5e-4, (graph, b, t, lp[b, t], ref[b, t, codes[b, t]])
                ended = codes[b, t] == cfg.stop_mel_token
    print(f"largest |lp - log_softmax(reference logits)[code]| = {worst:.3e}")
