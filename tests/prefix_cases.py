"""What the prefix tests share (continuing from given codes): the tiny synthetic model, its prompts, fake input_ids with codes behind
them and the session drain."""
import numpy as np
import torch

from indextts_amd import synth, weights

PENALTY = 10.0
GREEDY = {"sampler": "greedy"}
HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
ACCEL = {"sampler": "accel", "temperature": 0.8}


def model(device, cfg, tag, kv_format=None, stop_bias=-30.0):
    """stop_bias -30: no row stops by itself, so every row runs to its cap and no prefix holds the stop token."""
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
    return UnifiedVoice(w, cfg, device=device, kv_format=kv_format)


def prompt_rows(uv, cfg, tag, widths):
    n = len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    return [uv.prompt_rows(conds[i:i + 1], torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens)))[0]
            for i in range(n)]


def fake_ids(cfg, B, P, prefix=None):
    """[B, P + 1] fake prefix of 1s + the start token, and behind it the given codes [B, k] (or one row of them for every row)."""
    f = torch.ones(B, P + 1, dtype=torch.long)
    f[:, -1] = cfg.start_mel_token
    if prefix is not None:
        p = torch.as_tensor(prefix).cpu().long()
        f = torch.cat([f, p.expand(B, -1) if p.dim() == 1 else p], 1)
    return f


def sampler_kw(samp):
    """A session sampler dict -> generate()'s keywords (exp_noise and seed are the caller's)."""
    if samp["sampler"] == "greedy":
        return {}
    return dict(do_sample=True, sampler=samp["sampler"], temperature=samp["temperature"], top_k=samp.get("top_k", 0), top_p=samp.get("top_p", 1.0))


def noise(cfg, cap, seed):
    return torch.empty(cap, cfg.number_mel_codes).exponential_(1, generator=torch.Generator().manual_seed(seed))


def one_shot_row0(uv, cfg, row, prefix, cap, samp, slots, draws=None, **kw):
    """Row 0 of generate(input_ids=[fake | prefix], prefix_layout="resume") on `slots` copies of the prompt, max_new = cap - k; the
    session's draws [cap, V] are offset by k: the one-shot call counts new steps from 0.  Returns prefix + new codes."""
    P, d = row.shape
    k = 0 if prefix is None else int(len(prefix))
    if samp["sampler"] != "greedy":
        kw = dict(kw, exp_noise=draws[k:, None, :].expand(cap - k, slots, -1).contiguous(), **sampler_kw(samp))
    out = uv.generate(fake_ids(cfg, slots, P, prefix if k else None), max_new_tokens=cap - k, tts_embeddings=row[None].expand(slots, P, d).contiguous(),
                      repetition_penalty=PENALTY, prefix_layout="resume", **kw)
    return out


def drain(sess, want, got=None, steps=3, scores=False):
    got = {} if got is None else got
    t = 0
    while not set(want) <= set(got):
        for s in sess.step(steps):
            r = sess.take(s, scores=scores)
            got[s] = tuple(x.cpu().numpy() for x in r) if scores else r.cpu().numpy()
        t += 1
        assert t < 1000
    return got


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
