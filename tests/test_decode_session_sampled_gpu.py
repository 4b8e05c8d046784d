"""GPU: sampled GPT decode sessions (`UnifiedVoice.decode_session(sampled=True)`, `idxtts_gpt_session_admit_sampled`).

Contract pinned here: a sampled request decoded in a session of width `slots` yields, bit for bit, row 0 of
`UnifiedVoice.generate(do_sample=True, sampler=..., temperature=..., top_k=..., top_p=..., seed=s)` on `slots` copies of its prompt
(no left padding, max_new_tokens = its cap); with an explicit noise tensor N [cap, V], the same call with exp_noise whose row 0 is N.
Greedy rows of a sampled session equal the same rows of a greedy session.  This holds whatever else is in flight, when the request
was admitted and which slot it has.  With a bf16 KV cache in split-bf16 GEMM mode the reference batch has slots * (P + 1) >= 256
prefill rows."""
import ctypes

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}          # IndexTTS2.infer's defaults
HF2 = {"sampler": "hf", "temperature": 1.3, "top_k": 5, "top_p": 0.5}
HF_FULL = {"sampler": "hf", "temperature": 0.7, "top_k": 0, "top_p": 1.0}      # no top-k / top-p: the whole-row path
ACCEL = {"sampler": "accel", "temperature": 0.8}


def _model(device, cfg, tag, weight_format="f32", kv_format=None, stop_bias=None):
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    if stop_bias is not None:
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
    return UnifiedVoice(w, cfg, device=device, weight_format=weight_format, kv_format=kv_format), w


def _requests(uv, cfg, tag, n, widths, caps, samplers):
    """n prompts ([P, d] rows) of the given text widths, each with its own conditioning and sampler (seeded per request)."""
    nc = cfg.cond_latents + 2
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, nc, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        samp = dict(samplers[i % len(samplers)])
        if samp["sampler"] != "greedy":
            samp["seed"] = 1000 + 7919 * i
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "conds": conds[i:i + 1].cpu(), "text": text,
                     "samp": samp})
    return reqs


def _trim(codes, stop):
    c = codes.cpu().numpy() if torch.is_tensor(codes) else np.asarray(codes)
    hits = np.nonzero(c == stop)[0]
    return c[: hits[0] + 1] if len(hits) else c


def _reference(uv, row, slots, cap, samp, noise=None):
    """Row 0 of generate() on `slots` copies of the prompt with the request's sampler, up to and including the stop token."""
    P, d = row.shape
    emb = row[None].expand(slots, P, d).contiguous()
    ids = torch.ones(slots, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    kw = {}
    if samp["sampler"] != "greedy":
        kw = dict(do_sample=True, sampler=samp["sampler"], temperature=samp.get("temperature", 1.0), top_k=samp.get("top_k", 0),
                  top_p=samp.get("top_p", 1.0))
        if noise is not None:
            kw["exp_noise"] = noise[:, None, :].expand(cap, slots, noise.shape[1]).contiguous()
        else:
            kw["seed"] = samp["seed"]
    out = uv.generate(ids, max_new_tokens=cap, tts_embeddings=emb, repetition_penalty=10.0, **kw)
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
            slots = sess.admit([reqs[i]["row"] for i in group], [reqs[i]["cap"] for i in group],
                               sampling=[reqs[i]["samp"] for i in group])
            for s, i in zip(slots, group):
                in_slot[s] = (i, t)
        steps = int(rng.integers(1, 6))
        for s in sess.step(steps):
            i, t0 = in_slot.pop(s)
            out[i] = (sess.take(s).cpu().numpy(), t0)
        t += steps
        assert t < 10000
    return out


def _check(uv, reqs, out, slots, stop, which=None):
    for i in (range(len(reqs)) if which is None else which):
        r = reqs[i]
        codes = out[i][0]
        ref = _reference(uv, r["row"], slots, r["cap"], r["samp"])
        assert np.array_equal(codes, ref), (i, r["samp"]["sampler"], codes[:12], ref[:12])
        assert len(codes) <= r["cap"]
        assert (codes[:-1] != stop).all()


@pytest.mark.parametrize("kv,mode,use_graph", [("f32", _lib.GEMM_BF16X3, True), ("f32", _lib.GEMM_BF16X3, False),
                                               ("bf16", _lib.GEMM_F32, True), ("bf16", _lib.GEMM_BF16X3, True),
                                               ("bf16", _lib.GEMM_BF16X3, False)])
def test_staggered_sampled_admission_equals_generate_on_copies(device, kv, mode, use_graph):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/stag", kv_format=kv, stop_bias=2.0)
    slots, n = 4, 10
    long_texts = kv == "bf16" and mode == _lib.GEMM_BF16X3      # the reference's prefill (4 x (P + 1) rows) >= 256 rows too
    widths = [int(x) for x in synth.integers(f"t/ssess/stag/w/{long_texts}", (n,), 56 if long_texts else 3, 61 if long_texts else 40)]
    caps = [int(x) for x in synth.integers("t/ssess/stag/caps", (n,), 3, 40)]
    try:
        _lib.set_gemm_mode(mode)
        reqs = _requests(uv, cfg, "t/ssess/stag", n, widths, caps, [HF, ACCEL, HF2, HF_FULL])
        sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=40, use_graph=use_graph, sampled=True)
        out = _run(sess, reqs, seed=1)
        sess.close()
        assert sorted(out) == list(range(n))
        assert len({t for _, t in out.values()}) > 1, "every request admitted at once: the test shows nothing"
        _check(uv, reqs, out, slots, cfg.stop_mel_token)
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_plane_gemv_sampled_session(device):
    """Width >= 17 with bf16 weights: the decode step and the first-token head run on the plane GEMV."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/pl", weight_format="bf16", stop_bias=2.0)
    assert _lib.load().idxtts_get_decode_plane_rows() <= 20
    slots, n = 20, 26
    widths = [int(x) for x in synth.integers("t/ssess/pl/w", (n,), 8, 30)]
    caps = [int(x) for x in synth.integers("t/ssess/pl/caps", (n,), 4, 30)]
    reqs = _requests(uv, cfg, "t/ssess/pl", n, widths, caps, [HF, ACCEL, HF2])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=30, sampled=True)
    out = _run(sess, reqs, seed=2, max_admit=7)
    sess.close()
    _check(uv, reqs, out, slots, cfg.stop_mel_token)


@pytest.mark.parametrize("sampler", ["hf", "accel"])
@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_explicit_noise_matches_oracle(device, sampler, kv):
    """Each request supplies its draws [cap, V]: the codes equal the CPU oracle's sampling loop on that utterance alone with those draws
    (bf16 cache: the oracle rounds keys and values, in the exact GEMM mode so the prefill kernels are the oracle's arithmetic)."""
    from oracle import gpt as og
    cfg = GPTConfig.tiny()
    uv, w = _model(device, cfg, "t/gpt/eos", kv_format=kv, stop_bias=3.5)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    n, cap, V = 5, 32, cfg.number_mel_codes
    samp = dict(HF if sampler == "hf" else ACCEL)
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32 if kv == "bf16" else _lib.GEMM_BF16X3)
        reqs = _requests(uv, cfg, f"t/ssess/noise/{sampler}", n, [9, 4, 7, 2, 9], [cap] * n, [samp])
        gen = torch.Generator().manual_seed(5)
        noises = [torch.empty(cap, V).exponential_(1, generator=gen) for _ in range(n)]
        for r, nz in zip(reqs, noises):
            r["samp"] = dict(samp, exp_noise=nz.to(device))
        sess = uv.decode_session(4, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=cap, sampled=True)
        out = _run(sess, reqs, seed=3)
        sess.close()
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    lens = set()
    for i, r in enumerate(reqs):
        with torch.no_grad():
            ref = og.generate_sample(tw, cfg, r["conds"], r["text"], cap, noises[i][:, None, :], 10.0, samp["temperature"],
                                     samp.get("top_k", 0), samp.get("top_p", 1.0), accel_sampler=(sampler == "accel"),
                                     kv_round=(kv == "bf16"))
        assert np.array_equal(out[i][0], _trim(ref[0], cfg.stop_mel_token)), i
        lens.add(len(out[i][0]))
    assert len(lens) > 1, "every row stopped at the same step: the test shows nothing"


def test_placement_independence(device):
    """One request (prompt, sampler, seed) returns the same codes admitted alone, beside five others, into a slot reused after other
    requests retired, and into another slot id."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/place", stop_bias=1.0)
    slots = 6
    reqs = _requests(uv, cfg, "t/ssess/place", 7, [12, 5, 30, 8, 17, 3, 22], [36, 10, 30, 7, 12, 9, 25], [HF, ACCEL, HF2])
    x = reqs[0]
    mp = max(r["row"].shape[0] for r in reqs)

    def drain(sess, want_slot):
        got = {}
        while want_slot not in got:
            for s in sess.step(3):
                got[s] = sess.take(s).cpu().numpy()
        return got[want_slot]

    def fresh():
        return uv.decode_session(slots, max_prompt=mp, max_new=40, sampled=True)

    results = {}
    sess = fresh()                                                   # alone, slot 0
    (s,) = sess.admit([x["row"]], [x["cap"]], sampling=[x["samp"]])
    results["alone"] = (s, drain(sess, s))
    sess.close()
    sess = fresh()                                                   # with five others, last slot
    others = reqs[1:6]
    ids = sess.admit([r["row"] for r in others] + [x["row"]], [r["cap"] for r in others] + [x["cap"]],
                     sampling=[r["samp"] for r in others] + [x["samp"]])
    results["crowded"] = (ids[-1], drain(sess, ids[-1]))
    sess.close()
    sess = fresh()                                                   # reused slot: others ran (to their caps or stop) and left
    ids = sess.admit([r["row"] for r in reqs[1:7]], [r["cap"] for r in reqs[1:7]], sampling=[r["samp"] for r in reqs[1:7]])
    left = set(ids)
    while left:
        for s in sess.step(4):
            sess.take(s)
            left.discard(s)
    (s,) = sess.admit([x["row"]], [x["cap"]], sampling=[x["samp"]])
    results["reused"] = (s, drain(sess, s))
    sess.close()
    sess = fresh()                                                   # another slot id: two fillers first
    sess.admit([reqs[3]["row"], reqs[5]["row"]], [reqs[3]["cap"], reqs[5]["cap"]], sampling=[reqs[3]["samp"], reqs[5]["samp"]])
    (s,) = sess.admit([x["row"]], [x["cap"]], sampling=[x["samp"]])
    results["moved"] = (s, drain(sess, s))
    sess.close()
    assert results["moved"][0] != results["alone"][0] and results["crowded"][0] != results["alone"][0]
    ref = _reference(uv, x["row"], slots, x["cap"], x["samp"])
    for k, (_, codes) in results.items():
        assert np.array_equal(codes, ref), k


def test_mixed_modes_greedy_rows_equal_greedy_session(device):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/mixed", stop_bias=2.0)
    slots, n = 4, 9
    widths = [int(x) for x in synth.integers("t/ssess/mixed/w", (n,), 3, 30)]
    caps = [int(x) for x in synth.integers("t/ssess/mixed/caps", (n,), 5, 36)]
    reqs = _requests(uv, cfg, "t/ssess/mixed", n, widths, caps, [{"sampler": "greedy"}, HF, ACCEL])
    mp = max(r["row"].shape[0] for r in reqs)
    sess = uv.decode_session(slots, max_prompt=mp, max_new=36, sampled=True)
    out = _run(sess, reqs, seed=5)
    sess.close()
    greedy = [i for i, r in enumerate(reqs) if r["samp"]["sampler"] == "greedy"]
    gsess = uv.decode_session(slots, max_prompt=mp, max_new=36)
    gout = {}
    for i in greedy:
        (s,) = gsess.admit([reqs[i]["row"]], [reqs[i]["cap"]])
        while s not in gout:
            for f in gsess.step(5):
                gout[f] = gsess.take(f).cpu().numpy()
        assert np.array_equal(out[i][0], gout.pop(s)), i
    gsess.close()
    _check(uv, reqs, out, slots, cfg.stop_mel_token)
    sampled = [i for i in range(n) if i not in greedy]
    assert any(not np.array_equal(out[i][0], _reference(uv, reqs[i]["row"], slots, reqs[i]["cap"], {"sampler": "greedy"}))
               for i in sampled), "sampled rows all equal greedy decoding: the test shows nothing"


def test_sampled_retirement_by_stop_token(device):
    """A stop bias so that sampled rows stop at different steps, well before their caps: the codes end at the stop token and equal the
    reference."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/stop", stop_bias=3.5)
    n = 8
    reqs = _requests(uv, cfg, "t/ssess/stop", n, [9, 4, 7, 2, 9, 5, 11, 6], [48] * n, [HF, ACCEL])
    sess = uv.decode_session(4, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=48, sampled=True)
    out = _run(sess, reqs, seed=6)
    sess.close()
    stopped = [len(out[i][0]) for i in range(n) if out[i][0][-1] == cfg.stop_mel_token and len(out[i][0]) < 48]
    assert len(stopped) >= n // 2 and len(set(stopped)) > 1, f"too few rows retired on the stop token: {stopped}"
    _check(uv, reqs, out, 4, cfg.stop_mel_token)


def test_refusals_take_no_slot(device):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/ssess/refuse", stop_bias=2.0)
    reqs = _requests(uv, cfg, "t/ssess/refuse", 2, [6, 9], [12, 12], [HF])
    mp = max(r["row"].shape[0] for r in reqs)
    sess = uv.decode_session(3, max_prompt=mp, max_new=12, sampled=True)
    rows, caps = [r["row"] for r in reqs], [r["cap"] for r in reqs]
    with pytest.raises(ValueError, match="top_k"):
        sess.admit(rows, caps, sampling=[HF, dict(HF, top_k=0)])                 # top_p < 1 without top-k
    with pytest.raises(ValueError, match="temperature"):
        sess.admit(rows, caps, sampling=[dict(HF, temperature=0.0), HF])
    with pytest.raises(ValueError, match="temperature"):
        sess.admit(rows, caps, sampling=dict(ACCEL, temperature=-1.0))
    assert sess.free_slots == [0, 1, 2]
    # the library checks every row itself: a bad row refuses the whole call, no slot taken
    lib = _lib.load()
    emb = torch.stack([torch.nn.functional.pad(r, (0, 0, 0, mp - r.shape[0])) for r in rows]).to(device).contiguous()
    plen = np.array([r.shape[0] for r in rows], np.int32)
    ids = np.array([0, 1], np.int32)
    hcaps = np.array(caps, np.int32)

    def raw_admit(s, per_row):
        arr = (_lib.SamplingC * 2)(*per_row)
        torch.cuda.synchronize()
        rc = lib.idxtts_gpt_session_admit_sampled(uv._h, 2, _lib.ptr(emb), mp, plen.ctypes.data_as(ctypes.c_void_p),
                                                  ids.ctypes.data_as(ctypes.c_void_p), hcaps.ctypes.data_as(ctypes.c_void_p),
                                                  ctypes.cast(arr, ctypes.c_void_p), _lib.ptr(s._ws), s._sp())
        s.stream.synchronize()
        return rc

    good = _lib.SamplingC(mode=1, temperature=0.8, top_k=30, top_p=0.8, exp_noise=None, seed=1)
    for bad in (_lib.SamplingC(mode=1, temperature=0.8, top_k=0, top_p=0.8, exp_noise=None, seed=1),
                _lib.SamplingC(mode=2, temperature=0.0, top_k=0, top_p=1.0, exp_noise=None, seed=1),
                _lib.SamplingC(mode=3, temperature=1.0, top_k=0, top_p=1.0, exp_noise=None, seed=1)):
        assert raw_admit(sess, [good, bad]) != 0
    # nothing was taken: both requests are admitted now and decode to their references
    got = {}
    ids2 = sess.admit(rows, caps, sampling=[r["samp"] for r in reqs])
    assert ids2 == [0, 1]
    while len(got) < 2:
        for s in sess.step(4):
            got[s] = sess.take(s).cpu().numpy()
    sess.close()
    for s, r in zip(ids2, reqs):
        assert np.array_equal(got[s], _reference(uv, r["row"], 3, r["cap"], r["samp"]))
    # sampling= on a greedy session: refused in Python and by the library
    gsess = uv.decode_session(3, max_prompt=mp, max_new=12)
    with pytest.raises(ValueError, match="sampled=True"):
        gsess.admit(rows, caps, sampling=[HF, HF])
    assert raw_admit(gsess, [good, good]) != 0
    assert gsess.free_slots == [0, 1, 2]
    gsess.close()


def test_full_width_bf16_sampled_session(device):
    """GPTConfig() with synthetic weights, 16 slots, bf16 weights and KV, the reference defaults (HF 0.8 / 30 / 0.8), ~30 requests
    with caps over 24..80 codes."""
    cfg = GPTConfig()
    uv, _ = _model(device, cfg, "t/ssess/full", weight_format="bf16", kv_format="bf16")
    n, slots = 30, 16
    widths = [int(x) for x in synth.integers("t/ssess/full/w", (n,), 20, 120)]
    caps = [int(x) for x in synth.integers("t/ssess/full/caps", (n,), 24, 81)]
    reqs = _requests(uv, cfg, "t/ssess/full", n, widths, caps, [HF])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=80, sampled=True)
    out = _run(sess, reqs, seed=7, max_admit=6)
    sess.close()
    assert sorted(out) == list(range(n))
    _check(uv, reqs, out, slots, cfg.stop_mel_token, which=(0, 11, 29))
