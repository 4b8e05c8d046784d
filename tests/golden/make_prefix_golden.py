"""Continuation-from-given-codes fixtures for tests/test_prefix_ref_gpu.py -> prefix_ref.npz.

The reference's inference_speech(..., input_tokens=) appends the given mel codes to input_ids and extends the attention mask with ones
(model_v2.py:838-856); its GPT2InferenceModel then embeds [start, codes...] at mel positions 0, 1, ..., k in the first forward
(model_v2.py:163-165) and feeds the first generated code at position k + 2 (model_v2.py:175).  Here that model is driven the way
make_golden.py::make_gpt_ref section a3 drives it -- its own prepare_inputs_for_generation, the HF repetition penalty 10, the choice by
hand so that every step's logits are recorded -- with ids = cat([prep_fake, prefix]) and prefix = gpt_ref.npz's step_codes[:, :k]:
  prefix_k{k}_logits [3, 6, 258], prefix_k{k}_codes [3, 6]   for k = 1, 4, 10 (greedy)
  sample_k4_codes [3, 6], sample_k4_noise [6, 3, 258], sample_params   one sampled case: HF's warpers (temperature .8, top-k 30, top-p
      .8) and torch.multinomial, seeded; the Exp(1) draws it consumed are re-drawn with the same seed and stored.
Conditioning and texts are gpt_ref.npz's (`conds`, `text`), so the file holds results only.  P + 1 = 23: with k = 10 row 0's prefill
is 33 keys, one past a 32-key tile; rows 1 and 2 are left-padded by 3 and 7.

Run on the CPU:  python tests/golden/make_prefix_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository and the package on sys.path)

KS, NEW, SEED = (1, 4, 10), 6, 977
TEMP, TOPK, TOPP = 0.8, 30, 0.8


def drive(im, cfg, fake, mask, prefix, new, choose):
    """prefill on [fake | prefix], then cached single-token steps: (logits [B, new, V], codes [B, new])."""
    B = fake.shape[0]
    ids = torch.cat([fake, prefix], 1)
    mask = torch.cat([mask, torch.ones(B, prefix.shape[1], dtype=mask.dtype)], 1)
    past, logits_all = None, []
    unfinished = torch.ones(B, dtype=torch.long)
    with torch.no_grad():
        for _ in range(new):
            mi = im.prepare_inputs_for_generation(ids, past_key_values=past, attention_mask=mask, use_cache=True)
            o = im(**mi, return_dict=True)
            past = o.past_key_values
            logits = o.logits[:, -1].float()
            logits_all.append(logits.clone())
            nxt = choose(ids, logits.clone())
            nxt = nxt * unfinished + cfg.stop_mel_token * (1 - unfinished)
            ids = torch.cat([ids, nxt[:, None]], 1)
            mask = torch.cat([mask, torch.ones(B, 1, dtype=mask.dtype)], 1)
            unfinished = unfinished & (nxt != cfg.stop_mel_token).long()
    return torch.stack(logits_all, 1), ids[:, fake.shape[1] + prefix.shape[1]:]


def main():
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    from indextts_amd import weights
    from indextts_amd.config import GPTConfig
    mv = mg._import_reference_model_v2()
    cfg = GPTConfig.tiny()
    g = np.load(os.path.join(HERE, "gpt_ref.npz"))
    conds, text = torch.from_numpy(g["conds"]), torch.from_numpy(g["text"])
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    w.update(weights.synth_gpt_cond_weights(cfg, tag="golden/gptref"))
    uv = mg.build_reference_unified_voice(mv, cfg, w)
    with torch.no_grad():
        fake, inputs_embeds, mask = uv.prepare_gpt_inputs(conds, text)
    assert np.array_equal(fake.numpy(), g["prep_fake"]) and np.array_equal(mask.numpy(), g["prep_mask"])
    im = uv.inference_model
    im.store_mel_emb(inputs_embeds)
    proc = RepetitionPenaltyLogitsProcessor(penalty=10.0)
    step_codes = torch.from_numpy(g["step_codes"])
    out = {"ks": np.array(KS), "new": np.array(NEW)}
    for k in KS:
        prefix = step_codes[:, :k]
        assert not bool((prefix == cfg.stop_mel_token).any()), "a prefix holds the stop token"
        logits, codes = drive(im, cfg, fake, mask, prefix, NEW, lambda ids, lg: torch.argmax(proc(ids, lg), -1))
        out[f"prefix_k{k}_logits"], out[f"prefix_k{k}_codes"] = logits.numpy(), codes.numpy()
        print(f"k = {k}: greedy continuation", codes.tolist(), "| the uninterrupted run's", step_codes[:, k:k + NEW].tolist())
    # one sampled case: HF's _sample order -- processor, warpers, softmax, torch.multinomial (one exponential_() on [B, V] per step)
    warpers = [TemperatureLogitsWarper(TEMP), TopKLogitsWarper(top_k=TOPK, min_tokens_to_keep=1), TopPLogitsWarper(top_p=TOPP, min_tokens_to_keep=1)]
    probs_seen = []

    def sample(ids, lg):
        scores = proc(ids, lg)
        for wp in warpers:
            scores = wp(ids, scores)
        probs = torch.softmax(scores, -1)
        probs_seen.append(probs)
        return torch.multinomial(probs, num_samples=1).squeeze(1)
    k = 4
    prefix = step_codes[:, :k]
    torch.manual_seed(SEED)
    _, codes = drive(im, cfg, fake, mask, prefix, NEW, sample)
    torch.manual_seed(SEED)
    noise = torch.stack([torch.empty(text.shape[0], cfg.number_mel_codes).exponential_(1) for _ in range(NEW)])
    # the stored draws are the ones multinomial consumed: argmax(probs / q) gives its tokens (rows that had finished emit the stop token)
    redo = torch.stack([torch.argmax(p / noise[t], -1) for t, p in enumerate(probs_seen)], 1)
    live = torch.cumsum((codes == cfg.stop_mel_token).long(), 1) - (codes == cfg.stop_mel_token).long() == 0
    assert bool((redo[live] == codes[live]).all()), "re-drawn Exp(1) noise does not reproduce torch.multinomial's tokens"
    out["sample_k4_codes"], out["sample_k4_noise"] = codes.numpy(), noise.numpy()
    out["sample_params"] = np.array([TEMP, TOPK, TOPP], dtype=np.float64)
    print("k = 4 sampled continuation", codes.tolist())
    np.savez_compressed(os.path.join(HERE, "prefix_ref.npz"), **out)
    print("wrote prefix_ref.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
