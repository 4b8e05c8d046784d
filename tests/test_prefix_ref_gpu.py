"""GPU: the reference's continuation from given codes (inference_speech(..., input_tokens=), model_v2.py:838-856) against fixtures its
own GPT2InferenceModel produced (tests/golden/make_prefix_golden.py -> prefix_ref.npz), in the configuration of
tests/test_gpt_ref_gpu.py: the codes behind input_ids at mel positions 1 .. k (prefix_layout="hf"), the first new code fed at k + 2.
Prefixes of 1, 4 and 10 codes (P + 1 = 23: with k = 10 row 0's prefill is 33 keys, one past a 32-key tile; rows 1 and 2 are
left-padded by 3 and 7), 6 new steps each; one sampled case with the Exp(1) draws the reference consumed."""
import os

import numpy as np
import pytest
import torch

from indextts_amd import weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(golden_dir, device):
    from indextts_amd.gpt import UnifiedVoice
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    p = np.load(os.path.join(golden_dir, "prefix_ref.npz"))
    cfg = GPTConfig.tiny()
    uv = UnifiedVoice(weights.synth_gpt_weights(cfg, tag="golden/gptref"), cfg, device=device)
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(device), torch.from_numpy(g["text"]))
    return g, p, cfg, uv, fake, emb, mask


@pytest.mark.parametrize("k", [1, 4, 10])
def test_greedy_continuation_vs_reference(ref, k):
    g, p, cfg, uv, fake, emb, mask = ref
    NEW = int(p["new"])
    ids = torch.cat([fake, torch.from_numpy(g["step_codes"][:, :k])], 1)
    am = torch.nn.functional.pad(mask, (0, k), value=1)      # the reference extends the mask with ones (model_v2.py:854)
    for graph in (False, True):
        out = uv.generate(ids, max_new_tokens=NEW, stop_tokens=[cfg.stop_mel_token], attention_mask=am, tts_embeddings=emb,
                          repetition_penalty=10.0, use_graph=graph)
        np.testing.assert_array_equal(out[:, :ids.shape[1]].cpu().numpy(), ids.numpy())
        np.testing.assert_array_equal(out[:, ids.shape[1]:].cpu().numpy(), p[f"prefix_k{k}_codes"])
    out, logits = uv.generate(ids, max_new_tokens=NEW, stop_tokens=[cfg.stop_mel_token], attention_mask=am, tts_embeddings=emb,
                              repetition_penalty=10.0, return_logits=True)
    np.testing.assert_allclose(logits.cpu().numpy(), p[f"prefix_k{k}_logits"], rtol=0, atol=5e-4)


def test_sampled_continuation_vs_reference(ref):
    """HF's warpers and torch.multinomial behind 4 given codes, token for token with the recorded draws."""
    g, p, cfg, uv, fake, emb, mask = ref
    temperature, top_k, top_p = (float(x) for x in p["sample_params"])
    noise = torch.from_numpy(p["sample_k4_noise"])
    ids = torch.cat([fake, torch.from_numpy(g["step_codes"][:, :4])], 1)
    for graph in (False, True):
        out = uv.generate(ids, max_new_tokens=noise.shape[0], stop_tokens=[cfg.stop_mel_token], attention_mask=mask, tts_embeddings=emb,
                          repetition_penalty=10.0, do_sample=True, sampler="hf", temperature=temperature, top_k=int(top_k), top_p=top_p,
                          exp_noise=noise, use_graph=graph)
        np.testing.assert_array_equal(out[:, ids.shape[1]:].cpu().numpy(), p["sample_k4_codes"])


def test_inference_speech_input_tokens_vs_reference(ref):
    """UnifiedVoice.inference_speech(input_tokens=) on one utterance: the reference's call, the new codes returned."""
    g, p, cfg, uv, fake, emb, mask = ref
    codes, _ = uv.inference_speech(torch.from_numpy(g["cond_latent"]), torch.from_numpy(g["text"])[:1], emo_vec=torch.from_numpy(g["emovec_merged"]),
                                   input_tokens=torch.from_numpy(g["step_codes"][0, :4]), max_generate_length=int(p["new"]), do_sample=False,
                                   num_beams=1, repetition_penalty=10.0)
    np.testing.assert_array_equal(codes.cpu().numpy(), p["prefix_k4_codes"][:1])
