"""GPU: the GPT decode session (continuous batching, `UnifiedVoice.decode_session` / `idxtts_gpt_session_*`).

Contract pinned here: a request decoded in a session of width `slots` yields, bit for bit, row 0 of `UnifiedVoice.generate` on `slots`
copies of its prompt (no left padding, max_new_tokens = the request's cap) -- whatever else is in flight, when it was admitted and which
slot it had.  With a bf16 KV cache in split-bf16 GEMM mode the reference batch is chosen with slots * (P + 1) >= 256 prefill rows."""
import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu


def _model(device, cfg, tag, weight_format="f32", kv_format=None, stop_bias=None):
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    if stop_bias is not None:
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
    return UnifiedVoice(w, cfg, device=device, weight_format=weight_format, kv_format=kv_format), w


def _requests(uv, cfg, tag, n, widths, caps):
    """n prompts ([P, d] rows) of the given text widths; each with its own conditioning."""
    nc = cfg.cond_latents + 2
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, nc, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "conds": conds[i:i + 1].cpu(), "text": text})
    return reqs


def _trim(codes, stop):
    c = codes.cpu().numpy()
    hits = np.nonzero(c == stop)[0]
    return c[: hits[0] + 1] if len(hits) else c


def _reference(uv, row, slots, cap):
    """Row 0 of generate() on `slots` copies of the prompt, up to and including the stop token."""
    P, d = row.shape
    emb = row[None].expand(slots, P, d).contiguous()
    ids = torch.ones(slots, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    out = uv.generate(ids, max_new_tokens=cap, tts_embeddings=emb, repetition_penalty=10.0)
    return _trim(out[0, P + 1:], uv.cfg.stop_mel_token)


def _run(sess, reqs, seed, max_admit=None):
    """Admit waiting requests as slots free up (in random-sized groups), step a random number of steps at a time, collect finished
    rows.  Returns {request index: (codes, admission step)}."""
    rng = np.random.default_rng(seed)
    waiting = list(range(len(reqs)))
    in_slot, out, t = {}, {}, 0
    while waiting or in_slot:
        free = sess.free_slots
        if waiting and free:
            k = min(len(waiting), len(free), int(rng.integers(1, (max_admit or len(free)) + 1)))
            group, waiting = waiting[:k], waiting[k:]
            slots = sess.admit([reqs[i]["row"] for i in group], [reqs[i]["cap"] for i in group])
            for s, i in zip(slots, group):
                in_slot[s] = (i, t)
        steps = int(rng.integers(1, 6))
        for s in sess.step(steps):
            i, t0 = in_slot.pop(s)
            out[i] = (sess.take(s).cpu().numpy(), t0)
        t += steps
        assert t < 10000
    return out


def _check(uv, reqs, out, slots, stop):
    for i, r in enumerate(reqs):
        codes = out[i][0]
        ref = _reference(uv, r["row"], slots, r["cap"])
        assert np.array_equal(codes, ref), (i, codes[:12], ref[:12])
        assert len(codes) <= r["cap"]
        assert (codes[:-1] != stop).all()


@pytest.mark.parametrize("kv,mode,use_graph", [("f32", _lib.GEMM_BF16X3, True), ("f32", _lib.GEMM_BF16X3, False),
                                               ("bf16", _lib.GEMM_F32, True), ("bf16", _lib.GEMM_BF16X3, True),
                                               ("bf16", _lib.GEMM_BF16X3, False)])
def test_staggered_admission_equals_generate_on_copies(device, kv, mode, use_graph):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/sess/stag", kv_format=kv, stop_bias=2.0)
    slots, n = 4, 10
    # bf16 cache + split-bf16 GEMMs: texts long enough that the reference's prefill (4 x (P + 1) rows) is >= 256 rows too
    long_texts = kv == "bf16" and mode == _lib.GEMM_BF16X3
    widths = [int(x) for x in synth.integers(f"t/sess/stag/w/{long_texts}", (n,), 56 if long_texts else 3, 61 if long_texts else 40)]
    caps = [int(x) for x in synth.integers("t/sess/stag/caps", (n,), 3, 40)]
    try:
        _lib.set_gemm_mode(mode)
        reqs = _requests(uv, cfg, "t/sess/stag", n, widths, caps)
        sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=40, use_graph=use_graph)
        out = _run(sess, reqs, seed=1)
        sess.close()
        assert sorted(out) == list(range(n))
        assert len({t for _, t in out.values()}) > 1, "every request admitted at once: the test shows nothing"
        _check(uv, reqs, out, slots, cfg.stop_mel_token)
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_plane_gemv_session(device):
    """Width >= 17 with bf16 weights: the decode step and the first-token head run on the plane GEMV."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/sess/pl", weight_format="bf16", stop_bias=2.0)
    assert _lib.load().idxtts_get_decode_plane_rows() <= 20
    slots, n = 20, 26
    widths = [int(x) for x in synth.integers("t/sess/pl/w", (n,), 8, 30)]
    caps = [int(x) for x in synth.integers("t/sess/pl/caps", (n,), 4, 30)]
    reqs = _requests(uv, cfg, "t/sess/pl", n, widths, caps)
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=30)
    out = _run(sess, reqs, seed=2, max_admit=7)
    sess.close()
    _check(uv, reqs, out, slots, cfg.stop_mel_token)


def test_slot_reuse_leaks_nothing(device):
    """A long request, then a short one in the same slot: no stale seen row, finished flag or keys reach the second."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/sess/reuse", stop_bias=-1e4)      # no stop token: every row runs to its cap
    reqs = _requests(uv, cfg, "t/sess/reuse", 3, [30, 5, 12], [60, 7, 9])
    sess = uv.decode_session(2, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=60)
    a, b = sess.admit([reqs[0]["row"], reqs[2]["row"]], [reqs[0]["cap"], reqs[2]["cap"]])
    got = {}
    while len(got) < 2:
        for s in sess.step(4):
            got[s] = sess.take(s).cpu().numpy()
    assert len(got[a]) == 60           # ran to its cap: the slot's cache holds 60 decoded keys beyond a 30-token text
    (c,) = sess.admit([reqs[1]["row"]], [reqs[1]["cap"]])
    assert c == a
    while not sess.step(3):
        pass
    short = sess.take(c).cpu().numpy()
    sess.close()
    assert np.array_equal(short, _reference(uv, reqs[1]["row"], 2, reqs[1]["cap"]))
    assert np.array_equal(got[a], _reference(uv, reqs[0]["row"], 2, reqs[0]["cap"]))
    assert np.array_equal(got[b], _reference(uv, reqs[2]["row"], 2, reqs[2]["cap"]))


def test_retirement_by_stop_token_matches_oracle(device):
    """mel_head.bias[stop] so that rows stop at different steps: the codes, and the step at which each row retires, equal the CPU
    oracle's greedy loop for that row alone."""
    from oracle import gpt as og
    cfg = GPTConfig.tiny()
    uv, w = _model(device, cfg, "t/gpt/eos", stop_bias=3.5)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    n = 6
    reqs = _requests(uv, cfg, "t/sess/stop", n, [9, 4, 7, 2, 9, 5], [48] * n)
    sess = uv.decode_session(4, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=48)
    out = _run(sess, reqs, seed=3)
    sess.close()
    lens = set()
    for i, r in enumerate(reqs):
        ref = og.generate_greedy(tw, cfg, r["conds"], r["text"], 48, 10.0)[0].numpy()
        assert np.array_equal(out[i][0], _trim(torch.from_numpy(ref), cfg.stop_mel_token)), i
        lens.add(len(out[i][0]))
    assert len(lens) > 1, "every row stopped at the same step: the test shows nothing"


def test_full_width_bf16_session(device):
    """GPTConfig() with synthetic weights, 16 slots, bf16 weights and KV, ~40 requests with caps over 24..96 codes."""
    cfg = GPTConfig()
    uv, _ = _model(device, cfg, "t/sess/full", weight_format="bf16", kv_format="bf16")
    n, slots = 40, 16
    widths = [int(x) for x in synth.integers("t/sess/full/w", (n,), 20, 120)]
    caps = [int(x) for x in synth.integers("t/sess/full/caps", (n,), 24, 97)]
    reqs = _requests(uv, cfg, "t/sess/full", n, widths, caps)
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=96)
    out = _run(sess, reqs, seed=4, max_admit=6)
    sess.close()
    assert sorted(out) == list(range(n))
    for i in (0, 13, 27, 39):
        ref = _reference(uv, reqs[i]["row"], slots, reqs[i]["cap"])
        assert np.array_equal(out[i][0], ref), i


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_unsplit_attention_session(device, kv):
    """33 slots x 4 heads = 132 attention workgroups, past the 128 up to which the decode attention splits a row's keys over several
    workgroups: every key range here is ONE piece, in both cache formats (the sessions above, 4 or 20 slots x 2 heads, split theirs).
    Prompts of about 40 rows run to caps of up to 24 codes, so a key range crosses a 16-key boundary; most slots stay dead."""
    import dataclasses
    cfg = dataclasses.replace(GPTConfig.tiny(), model_dim=256, heads=4)
    uv, _ = _model(device, cfg, "t/sess/unsplit", kv_format=kv, stop_bias=-1e4)      # no stop token: every row runs to its cap
    slots = 33
    reqs = _requests(uv, cfg, "t/sess/unsplit", 3, [33, 30, 35], [24, 17, 24])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24)
    out = _run(sess, reqs, seed=5, max_admit=2)
    sess.close()
    assert sorted(out) == [0, 1, 2]
    _check(uv, reqs, out, slots, cfg.stop_mel_token)


def test_session_refuses_sampling_and_beams(device):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/sess/refuse")
    with pytest.raises(ValueError, match="greedy"):
        uv.decode_session(2, 10, 10, do_sample=True)
    with pytest.raises(ValueError, match="greedy"):
        uv.decode_session(2, 10, 10, num_beams=3)
