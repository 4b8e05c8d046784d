"""GPU: continuing a one-shot generation from given codes (`idxtts_gpt_generate_prefix`, UnifiedVoice.generate with input_ids
[B, P+1+k]) on the tiny synthetic model.
  * an empty prefix is idxtts_gpt_generate_scored, bit for bit: codes, logits, log-probabilities;
  * layout "resume" goes on as the uninterrupted run did -- greedy and both samplers, on left-padded rows, from k = 1 to the k that
    leaves one position in the mel position table -- and its first new logits equal the teacher-forced logits of the same codes;
  * takes with a prefix equal the caller-expanded batch;
  * every refusal."""
import ctypes
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import prefix_cases as pc
from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def padded(golden_dir, device):
    """gpt_ref.npz's ragged batch (rows 1 and 2 left-padded by 3 and 7) on a model that never stops by itself."""
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    uv = pc.model(device, cfg, "golden/gptref")
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(device), torch.from_numpy(g["text"]))
    assert (mask[:, :-1] == 0).sum(1).tolist() == [0, 3, 7]
    return cfg, uv, fake, emb, mask


def _prefix_call(uv, emb, pad_left, B, takes, P, max_new, sc, prefix, k, pos0, logprobs=True):
    """idxtts_gpt_generate_prefix / idxtts_gpt_generate_scored (prefix is None) through the C ABI: (codes, n, logits, logprobs)."""
    R, V = B * takes, uv.cfg.number_mel_codes
    codes = torch.full((R, max_new), uv.cfg.stop_mel_token, dtype=torch.long, device=uv.device)
    logits = torch.zeros(max_new, R, V, device=uv.device)
    lp = torch.zeros(R, max_new, device=uv.device) if logprobs else None
    ws = uv._workspace(R, P + 1 + k, max_new)
    n = ctypes.c_int(0)
    head = (uv._h, _lib.ptr(emb), pad_left.ctypes.data_as(c_void_p), B, takes, P, max_new, pc.PENALTY,
            ctypes.cast(ctypes.pointer(sc), c_void_p) if sc is not None else c_void_p(0))
    tail = (_lib.ptr(logits), _lib.ptr(ws), ws.numel(), 0, _lib.current_stream())
    if prefix is None:
        _lib.check(_lib.load().idxtts_gpt_generate_scored(*head, _lib.ptr(codes), ctypes.byref(n), _lib.ptr(lp), *tail))
    else:
        _lib.check(_lib.load().idxtts_gpt_generate_prefix(*head, _lib.ptr(prefix), k, pos0, _lib.ptr(codes), ctypes.byref(n), _lib.ptr(lp), *tail))
    torch.cuda.synchronize()
    return codes.cpu().numpy(), n.value, logits.cpu().numpy(), None if lp is None else lp.cpu().numpy()


@pytest.mark.parametrize("samp", [None, pc.HF], ids=["greedy", "hf"])
def test_empty_prefix_is_the_scored_call_bit_for_bit(padded, samp):
    cfg, uv, fake, emb, mask = padded
    B, P, _ = emb.shape
    pad_left = (mask[:, :P] == 0).sum(1).numpy().astype(np.int32)
    takes, NEW = 2, 7
    sc = None
    if samp is not None:
        E = torch.stack([pc.noise(cfg, B * takes, 40 + t) for t in range(NEW)]).to(uv.device)      # [NEW, B * takes, V]
        sc = _lib.SamplingC(mode=1, temperature=samp["temperature"], top_k=samp["top_k"], top_p=samp["top_p"], exp_noise=E.data_ptr(), seed=0)
    want = _prefix_call(uv, emb, pad_left, B, takes, P, NEW, sc, None, 0, 1)
    dummy = torch.zeros(1, dtype=torch.long, device=uv.device)
    for pos0 in (1, 2):
        got = _prefix_call(uv, emb, pad_left, B, takes, P, NEW, sc, dummy, 0, pos0)
        assert got[1] == want[1]
        for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert pc.same_bits(a, b)


@pytest.mark.parametrize("samp", [pc.GREEDY, pc.HF, pc.ACCEL], ids=["greedy", "hf", "accel"])
def test_resume_layout_goes_on_as_the_uninterrupted_run(padded, samp):
    """Left-padded rows: the run cut after k codes and continued from them returns the uninterrupted run's codes (draws offset by k)."""
    cfg, uv, fake, emb, mask = padded
    B, NEW = fake.shape[0], 12
    kw = pc.sampler_kw(samp)
    E = torch.stack([pc.noise(cfg, B, 70 + t) for t in range(NEW)])
    draws = (lambda k: dict(kw, exp_noise=E[k:])) if kw else (lambda k: {})
    full = uv.generate(fake, max_new_tokens=NEW, attention_mask=mask, tts_embeddings=emb, repetition_penalty=pc.PENALTY, **draws(0))
    u = full[:, fake.shape[1]:]
    assert u.shape[1] == NEW and not bool((u == cfg.stop_mel_token).any())
    for k in (1, 5, NEW - 1):
        ids = torch.cat([fake, u[:, :k].cpu()], 1)
        am = torch.nn.functional.pad(mask, (0, k), value=1)
        for m in (mask, am):      # the mask may cover the extra columns
            out = uv.generate(ids, max_new_tokens=NEW - k, attention_mask=m, tts_embeddings=emb, repetition_penalty=pc.PENALTY,
                              prefix_layout="resume", **draws(k))
            assert torch.equal(out.cpu(), full.cpu()), k      # [input_ids | new codes], as HF returns it
    # the reference's layout puts the given codes elsewhere: another continuation (k = 5: four codes at other positions)
    out = uv.generate(torch.cat([fake, u[:, :5].cpu()], 1), max_new_tokens=NEW - 5, attention_mask=mask, tts_embeddings=emb,
                      repetition_penalty=pc.PENALTY, **draws(5))
    assert torch.equal(out[:, :fake.shape[1] + 5].cpu(), full[:, :fake.shape[1] + 5].cpu()) and not torch.equal(out.cpu(), full.cpu())


def test_prefix_up_to_the_last_position_of_the_table(device):
    """k + max_new + 1 < mel_pos_len: the longest prefix leaves max_new positions, one more is refused."""
    cfg = GPTConfig.tiny()
    uv = pc.model(device, cfg, "t/prefix/table")
    (row,) = pc.prompt_rows(uv, cfg, "t/prefix/table", [6])
    P, d = row.shape
    max_new = 2
    k = cfg.mel_pos_len - 2 - max_new
    emb = row[None].expand(2, P, d).contiguous()
    full = uv.generate(pc.fake_ids(cfg, 2, P), max_new_tokens=k + max_new, tts_embeddings=emb, repetition_penalty=pc.PENALTY)
    u = full[:, P + 1:]
    out = uv.generate(pc.fake_ids(cfg, 2, P, u[:, :k]), max_new_tokens=max_new, tts_embeddings=emb, repetition_penalty=pc.PENALTY, prefix_layout="resume")
    assert torch.equal(out.cpu(), full.cpu())
    out = uv.generate(pc.fake_ids(cfg, 2, P, u[:, :k]), max_new_tokens=max_new, tts_embeddings=emb, repetition_penalty=pc.PENALTY, prefix_layout="hf")
    assert out.shape == full.shape
    with pytest.raises(ValueError, match="mel position table"):
        uv.generate(pc.fake_ids(cfg, 2, P, u[:, :k]), max_new_tokens=max_new + 1, tts_embeddings=emb, repetition_penalty=pc.PENALTY)
    pre = u[:, :k].contiguous()
    pad_left = np.zeros(2, np.int32)
    with pytest.raises(RuntimeError, match="exceed the mel position table"):      # the native check, with the workspace it would need
        _prefix_call(uv, emb, pad_left, 2, 1, P, max_new + 1, None, pre, k, 2)


def test_takes_with_a_prefix_equal_the_expanded_batch(padded):
    """generate(num_return_sequences=3) behind a prefix: one prefill row per prompt, fanned out -- the caller-expanded batch's codes and
    log-probabilities (fp32 cache: always)."""
    cfg, uv, fake, emb, mask = padded
    B, n, NEW, k = fake.shape[0], 3, 8, 4
    pre = torch.from_numpy(synth.integers("t/prefix/takes", (B, k), 0, cfg.start_mel_token))
    ids = torch.cat([fake, pre], 1)
    E = torch.stack([pc.noise(cfg, B * n, 90 + t) for t in range(NEW)])
    kw = dict(max_new_tokens=NEW, repetition_penalty=pc.PENALTY, exp_noise=E, return_logprobs=True, **pc.sampler_kw(pc.HF))
    for layout in ("hf", "resume"):
        a, alp = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, num_return_sequences=n, prefix_layout=layout, **kw)
        b, blp = uv.generate(ids.repeat_interleave(n, 0), attention_mask=mask.repeat_interleave(n, 0),
                             tts_embeddings=emb.repeat_interleave(n, 0).contiguous(), prefix_layout=layout, **kw)
        assert a.shape == (B * n, ids.shape[1] + NEW) and torch.equal(a.cpu(), b.cpu())
        assert pc.same_bits(alp.cpu().numpy(), blp.cpu().numpy())
        assert len({tuple(r) for r in a[:n, ids.shape[1]:].tolist()}) > 1      # the takes of a prompt differ


def _forced_and_resumed(uv, g, ks):
    """(teacher-forced logits [3, NEW, V] of c = step_codes, {k: first new logits behind c[:, :k] in layout "resume"})."""
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(uv.device), torch.from_numpy(g["text"]))
    c = torch.from_numpy(g["step_codes"])
    kw = dict(attention_mask=mask, tts_embeddings=emb, repetition_penalty=10.0, return_logits=True)
    _, forced = uv.generate(fake, max_new_tokens=c.shape[1], forced_codes=c, **kw)
    first = {}
    for k in ks:
        _, lg = uv.generate(torch.cat([fake, c[:, :k]], 1), max_new_tokens=1, prefix_layout="resume", **kw)
        first[k] = lg[:, 0].cpu().numpy()
    return forced.cpu().numpy(), first


def test_resume_layout_against_teacher_forced_logits(golden_dir, device):
    """Contract 7.  The first new step behind c[:, :k] and column k of generate(forced_codes=c) are the same function of the same
    codes, once through the prefill and once through k decode steps.  Both are within 5e-4 of the reference in this configuration
    (tests/test_gpt_ref_gpu.py, tests/test_prefix_ref_gpu.py), hence the bound 1e-3.  Measured: see profiles/README.md "Prefix".
    bf16 / fp8 cache, k = 4: the bound is twice the largest difference, measured here, between that format's teacher-forced logits
    and the fp32 cache's -- the prefill-written and the step-written cache round the same quantities once each."""
    from indextts_amd.gpt import UnifiedVoice
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    forced32, first = _forced_and_resumed(UnifiedVoice(w, cfg, device=device), g, (1, 4, 9))
    for k, lg in first.items():
        err = float(np.abs(lg - forced32[:, k]).max())
        print(f"fp32 cache k = {k}: max |dlogit| resume vs teacher-forced = {err:.3e} (bound 1e-3)")
        assert err <= 1e-3, (k, err)
    for fmt in ("bf16", "fp8"):
        forced, first = _forced_and_resumed(UnifiedVoice(w, cfg, device=device, kv_format=fmt), g, (4,))
        fmt_err = float(np.abs(forced - forced32).max())
        err = float(np.abs(first[4] - forced[:, 4]).max())
        print(f"{fmt} cache k = 4: max |dlogit| resume vs teacher-forced = {err:.3e}; {fmt} vs fp32 teacher-forced = {fmt_err:.3e} (bound {2 * fmt_err:.3e})")
        assert err <= 2 * fmt_err, (fmt, err, fmt_err)


def test_refusals(padded):
    cfg, uv, fake, emb, mask = padded
    B, P, _ = emb.shape
    kw = dict(max_new_tokens=4, attention_mask=mask, tts_embeddings=emb, repetition_penalty=pc.PENALTY)
    ok = torch.from_numpy(synth.integers("t/prefix/refuse", (B, 3), 0, cfg.start_mel_token))
    bad = ok.clone()
    bad[1, 2] = cfg.stop_mel_token
    with pytest.raises(ValueError, match="stop token"):
        uv.generate(torch.cat([fake, bad], 1), **kw)
    bad[1, 2] = cfg.number_mel_codes
    with pytest.raises(ValueError, match="mel codes"):
        uv.generate(torch.cat([fake, bad], 1), **kw)
    with pytest.raises(ValueError, match="prefix_layout"):
        uv.generate(torch.cat([fake, ok], 1), prefix_layout="other", **kw)
    with pytest.raises(ValueError, match="forced_codes"):
        uv.generate(torch.cat([fake, ok], 1), forced_codes=torch.zeros(B, 4, dtype=torch.long), **kw)
    with pytest.raises(ValueError, match="input_ids"):
        uv.generate(fake[:, :-1], **kw)
    with pytest.raises(ValueError, match="attention_mask"):
        uv.generate(torch.cat([fake, ok], 1), **dict(kw, attention_mask=torch.nn.functional.pad(mask, (0, 1), value=1)))
    with pytest.raises(NotImplementedError, match="beam"):
        uv.generate_beam(torch.cat([fake, ok], 1), 4, mask, emb)
    # the native checks, behind the wrapper's: the stop token, a code outside the table, the layout, k < 0
    pad_left = (mask[:, :P] == 0).sum(1).numpy().astype(np.int32)
    stop = ok.clone()
    stop[2, 0] = cfg.stop_mel_token
    for prefix, k, pos0, msg in ((stop, 3, 1, "prefix contains the stop token"), (stop + 1000, 3, 1, "outside the mel code table"),
                                 (ok, 3, 3, "prefix_pos0"), (ok, -1, 1, "k >= 0")):
        with pytest.raises(RuntimeError, match=msg):
            _prefix_call(uv, emb, pad_left, B, 1, P, 4, None, prefix.to(uv.device).contiguous(), k, pos0)
    # nothing was left behind: the plain call still gives what it gave
    a = uv.generate(fake, **kw)
    assert torch.equal(a.cpu(), uv.generate(fake, **kw).cpu())


def test_inference_speech_input_tokens(golden_dir, device):
    """The reference's call: one utterance, (s,) or (1, s) codes, the new codes returned; the reference's layout."""
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    uv = pc.model(device, cfg, "golden/gptref")
    lat, emo, text = torch.from_numpy(g["cond_latent"]), torch.from_numpy(g["emovec_merged"]), torch.from_numpy(g["text"])[:1]
    kw = dict(emo_vec=emo, max_generate_length=5, do_sample=False, num_beams=1, repetition_penalty=10.0)
    tok = torch.from_numpy(synth.integers("t/prefix/speech", (4,), 0, cfg.start_mel_token))
    a, _ = uv.inference_speech(lat, text, input_tokens=tok, **kw)
    b, _ = uv.inference_speech(lat, text, input_tokens=tok[None], **kw)
    fake, emb, mask = uv.prepare_gpt_inputs(uv.conds_latent(lat.to(device), emo.to(device)), text)
    want = uv.generate(torch.cat([fake, tok[None]], 1), max_new_tokens=5, attention_mask=mask, tts_embeddings=emb, repetition_penalty=10.0,
                       prefix_layout="hf")[:, fake.shape[1] + 4:]
    assert a.shape == (1, 5) and torch.equal(a.cpu(), b.cpu()) and torch.equal(a.cpu(), want.cpu())
    with pytest.raises(NotImplementedError, match="expands them a second time"):
        uv.inference_speech(lat, text, input_tokens=tok, num_return_sequences=2, **dict(kw, do_sample=True))
    with pytest.raises(AssertionError, match="input_tokens"):
        uv.inference_speech(lat, text, input_tokens=tok[None].repeat(2, 1), **kw)
    with pytest.raises(AssertionError, match="text_inputs"):
        uv.inference_speech(lat, torch.from_numpy(g["text"])[:2], input_tokens=tok, **kw)
    with pytest.raises(NotImplementedError):
        uv.inference_speech(lat, text, input_tokens=tok, typical_sampling=True, **kw)
    with pytest.raises(NotImplementedError):
        uv.inference_speech(lat, text, input_tokens=tok, **dict(kw, num_beams=3))
