"""GPU: beam decode sessions (`UnifiedVoice.beam_session`, `idxtts_gpt_session_*_beam`).

Contract pinned here: a beam request decoded in a session of `slots` rows (slots / num_beams groups) yields, bit for bit, row 0 of
`UnifiedVoice.generate_beam` with the same num_beams, do_sample, temperature, top_k, top_p, length_penalty, early_stopping and repetition
penalty on slots / num_beams copies of its prompt (no attention mask, max_new_tokens = its cap; the same seed, or an exp_noise whose
[:, 0, :] is the request's noise), cut after its first stop token.  This holds whatever else is in flight, when the request was admitted
and which group it has.  With a bf16 KV cache in split-bf16 GEMM mode the reference batch has slots * (P + 1) >= 256 prefill rows."""
import ctypes

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

INFER = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}     # IndexTTS2.infer's defaults
SAMPLE2 = {"do_sample": True, "temperature": 1.3, "top_k": 5, "top_p": 0.5, "length_penalty": 1.0, "early_stopping": True}
SEARCH = {"do_sample": False, "length_penalty": 1.0}
SEARCH_ES = {"do_sample": False, "length_penalty": 0.0, "early_stopping": True}


def _model(device, cfg, tag, weight_format="f32", kv_format=None, stop_bias=None):
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    if stop_bias is not None:
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
    return UnifiedVoice(w, cfg, device=device, weight_format=weight_format, kv_format=kv_format), w


def _requests(uv, cfg, tag, n, widths, caps, beams, nb, noise=False):
    """n prompts ([P, d] rows), each with its own conditioning and beam parameters (a seed per request, or its own noise)."""
    nc = cfg.cond_latents + 2
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, nc, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        beam = dict(beams[i % len(beams)])
        if noise and beam.get("do_sample"):
            g = torch.Generator().manual_seed(500 + i)
            beam["exp_noise"] = torch.empty(int(caps[i]), nb * cfg.number_mel_codes).exponential_(1.0, generator=g)
        else:
            beam["seed"] = 1000 + 7919 * i
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "beam": beam})
    return reqs


def _trim(codes, stop):
    c = codes.cpu().numpy() if torch.is_tensor(codes) else np.asarray(codes)
    hits = np.nonzero(c == stop)[0]
    return c[: hits[0] + 1] if len(hits) else c


def _reference(uv, row, groups, nb, cap, beam):
    """Row 0 of generate_beam() on `groups` copies of the prompt with the request's parameters, up to and including the stop token."""
    P, d = row.shape
    emb = row[None].expand(groups, P, d).contiguous()
    ids = torch.ones(groups, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    kw = dict(num_beams=nb, do_sample=beam.get("do_sample", True), temperature=beam.get("temperature", 1.0), top_k=beam.get("top_k", 50),
              top_p=beam.get("top_p", 1.0), length_penalty=beam.get("length_penalty", 1.0), early_stopping=beam.get("early_stopping", False))
    if beam.get("exp_noise") is not None:
        nz = beam["exp_noise"]
        kw["exp_noise"] = nz[:, None, :].expand(cap, groups, nz.shape[1]).contiguous()
    else:
        kw["seed"] = beam["seed"]
    out = uv.generate_beam(ids, cap, None, emb, repetition_penalty=10.0, **kw)
    return _trim(out[0, P + 1:], uv.cfg.stop_mel_token)


def _run(sess, reqs, seed, max_admit=None):
    """Admit waiting requests as groups free up (in random-sized batches), step a random number of steps at a time, collect finished
    groups.  Returns {request index: (codes, admission step)}."""
    rng = np.random.default_rng(seed)
    waiting = list(range(len(reqs)))
    in_group, out, t = {}, {}, 0
    while waiting or in_group:
        free = sess.free_groups
        if waiting and free:
            k = min(len(waiting), len(free), int(rng.integers(1, (max_admit or len(free)) + 1)))
            batch, waiting = waiting[:k], waiting[k:]
            groups = sess.admit([reqs[i]["row"] for i in batch], [reqs[i]["cap"] for i in batch], beam=[reqs[i]["beam"] for i in batch])
            for g, i in zip(groups, batch):
                in_group[g] = (i, t)
        steps = int(rng.integers(1, 6))
        for g in sess.step(steps):
            i, t0 = in_group.pop(g)
            out[i] = (sess.take(g).cpu().numpy(), t0)
        t += steps
        assert t < 10000
    return out


def _check(uv, reqs, out, groups, nb, stop, which=None):
    for i in (range(len(reqs)) if which is None else which):
        r = reqs[i]
        codes = out[i][0]
        ref = _reference(uv, r["row"], groups, nb, r["cap"], r["beam"])
        assert np.array_equal(codes, ref), (i, codes[:12], ref[:12])
        assert 1 <= len(codes) <= r["cap"]
        assert (codes[:-1] != stop).all()


@pytest.mark.parametrize("kv,mode,use_graph,nb,beams,noise", [
    ("f32", _lib.GEMM_BF16X3, True, 3, [INFER, SEARCH], False),
    ("f32", _lib.GEMM_BF16X3, False, 2, [SAMPLE2, SEARCH_ES], True),
    ("f32", _lib.GEMM_F32, True, 4, [INFER, SAMPLE2], True),
    ("bf16", _lib.GEMM_F32, True, 4, [SEARCH, INFER], False),
    ("bf16", _lib.GEMM_BF16X3, True, 3, [INFER, SEARCH_ES, SAMPLE2], False),
    ("bf16", _lib.GEMM_BF16X3, False, 2, [SEARCH, INFER], True),
])
def test_staggered_beam_admission_equals_generate_beam(device, kv, mode, use_graph, nb, beams, noise):
    """Requests admitted at different steps, with caps from 3 up, retire at different steps; each equals its generate_beam reference."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/bsess/stag", kv_format=kv, stop_bias=2.0)
    groups, n = 3, 8
    slots = groups * nb
    long_texts = kv == "bf16" and mode == _lib.GEMM_BF16X3      # the reference's prefill (slots x (P + 1) rows) >= 256 rows too
    lo, hi = (40, 58) if long_texts else (3, 30)                # 40 text tokens: P + 1 > 256 / 6 rows
    widths = [int(x) for x in synth.integers(f"t/bsess/stag/w/{nb}/{long_texts}", (n,), lo, hi)]
    caps = [int(x) for x in synth.integers(f"t/bsess/stag/caps/{nb}", (n,), 3, 32)]
    caps[1] = 2                                                  # one group with a short cap
    try:
        _lib.set_gemm_mode(mode)
        reqs = _requests(uv, cfg, f"t/bsess/stag/{nb}", n, widths, caps, beams, nb, noise=noise)
        sess = uv.beam_session(slots, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=32, use_graph=use_graph)
        out = _run(sess, reqs, seed=nb)
        sess.close()
        assert sorted(out) == list(range(n))
        assert len({t for _, t in out.values()}) > 1, "every request admitted at once: the test shows nothing"
        assert len(out[1][0]) <= 2
        _check(uv, reqs, out, groups, nb, cfg.stop_mel_token)
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_placement_independence(device):
    """The same request in different groups and beside different neighbours gives identical codes."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/bsess/place", stop_bias=1.5)
    nb, groups = 3, 3
    reqs = _requests(uv, cfg, "t/bsess/place", 4, [7, 12, 3, 9], [24, 24, 10, 18], [INFER, SEARCH], nb)
    mp = max(r["row"].shape[0] for r in reqs)
    results = []
    for order, pre in (([0, 1, 2], 0), ([3, 2, 0], 0), ([1, 0], 1)):
        sess = uv.beam_session(groups * nb, nb, max_prompt=mp, max_new=24)
        if pre:                                     # a neighbour admitted earlier, stepped a few times
            sess.admit([reqs[3]["row"]], [reqs[3]["cap"]], beam=[reqs[3]["beam"]])
            sess.step(3)
        ids = sess.admit([reqs[i]["row"] for i in order], [reqs[i]["cap"] for i in order], beam=[reqs[i]["beam"] for i in order])
        g0 = ids[order.index(0)]
        got = None
        while got is None:
            for g in sess.step(4):
                c = sess.take(g).cpu().numpy()
                if g == g0:
                    got = c
        sess.close()
        results.append((g0, got))
    assert len({g for g, _ in results}) > 1, "request 0 always had the same group"
    for _, c in results[1:]:
        assert np.array_equal(c, results[0][1])
    assert np.array_equal(results[0][1], _reference(uv, reqs[0]["row"], groups, nb, reqs[0]["cap"], reqs[0]["beam"]))


def test_retirement_by_scorer_done_matches_oracle(device):
    """A stop bias that makes the stop token likely after a few steps: groups retire when their scorer is done, before their caps, with the
    codes of oracle.gpt.generate_beam on the utterance alone (bf16 cache, exact GEMM mode: the oracle's arithmetic); the freed groups
    are reused by later admissions with correct results."""
    from indextts_amd.gpt import UnifiedVoice
    from oracle import gpt as og
    cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=70, number_text_tokens=40, start_mel_token=68, stop_mel_token=69,
                    max_mel_tokens=60, max_text_tokens=30, cond_latents=4)
    w = weights.synth_gpt_weights(cfg, tag="t/bsess/done")
    w["mel_head.bias"][cfg.stop_mel_token] += 3.0
    uv = UnifiedVoice(w, cfg, device=device, kv_format="bf16")
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    nb, groups, n, NEW, L = 3, 2, 5, 24, 7
    V = cfg.number_mel_codes
    lat = torch.from_numpy(synth.uniform("t/bsess/done/lat", (n, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/bsess/done/emo", (n, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/bsess/done/text", (n, L), 2, cfg.number_text_tokens))
    g = torch.Generator().manual_seed(11)
    noise = torch.empty(NEW, n, nb * V).exponential_(1.0, generator=g)
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        conds = uv.conds_latent(lat.to(device), emo.to(device))
        rows = uv.prompt_rows(conds, text)
        sess = uv.beam_session(groups * nb, nb, max_prompt=max(r.shape[0] for r in rows), max_new=NEW)
        do_sample = [True, False, True, True, False]
        reqs = [{"row": rows[i], "cap": NEW, "beam": dict(INFER, do_sample=do_sample[i], exp_noise=noise[:, i])} for i in range(n)]
        out = _run(sess, reqs, seed=5, max_admit=2)
        sess.close()
        assert len({t for _, t in out.values()}) > 1, "no group was reused"
        with torch.no_grad():
            for i in range(n):
                want = og.generate_beam(tw, cfg, og.conds_latent(tw, cfg, lat[i:i + 1], emo[i:i + 1]), text[i:i + 1], NEW, noise[:, i:i + 1],
                                        num_beams=nb, do_sample=do_sample[i], kv_round=True)
                assert np.array_equal(out[i][0], _trim(want[0], cfg.stop_mel_token)), (i, out[i][0], want[0])
        early = [i for i in range(n) if len(out[i][0]) < NEW]
        assert len(early) >= 3, f"too few groups retired before their cap: {[len(out[i][0]) for i in range(n)]}"
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_plane_gemv_beam_session(device):
    """48 rows (16 groups x 3 beams) with bf16 weights: the decode step and the first-step head run on the plane GEMV."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/bsess/pl", weight_format="bf16", stop_bias=2.0)
    assert _lib.load().idxtts_get_decode_plane_rows() <= 48
    nb, groups, n = 3, 16, 22
    widths = [int(x) for x in synth.integers("t/bsess/pl/w", (n,), 4, 24)]
    caps = [int(x) for x in synth.integers("t/bsess/pl/caps", (n,), 4, 24)]
    reqs = _requests(uv, cfg, "t/bsess/pl", n, widths, caps, [INFER, SEARCH, SAMPLE2], nb)
    sess = uv.beam_session(groups * nb, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24)
    out = _run(sess, reqs, seed=2, max_admit=7)
    sess.close()
    assert sorted(out) == list(range(n))
    _check(uv, reqs, out, groups, nb, cfg.stop_mel_token, which=(0, 1, 2, 9, 17, 21))


def test_refusals_take_no_group(device):
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/bsess/refuse", stop_bias=2.0)
    nb = 3
    reqs = _requests(uv, cfg, "t/bsess/refuse", 2, [6, 9], [12, 12], [INFER], nb)
    mp = max(r["row"].shape[0] for r in reqs)
    with pytest.raises(ValueError, match="num_beams"):
        uv.beam_session(6, 1, max_prompt=mp, max_new=12)
    with pytest.raises(ValueError, match="multiple"):
        uv.beam_session(7, nb, max_prompt=mp, max_new=12)
    with pytest.raises(ValueError, match="greedy"):
        uv.decode_session(6, max_prompt=mp, max_new=12, num_beams=3)
    lib = _lib.load()
    assert lib.idxtts_gpt_session_workspace_bytes_beam(uv._h, 7, nb, mp, 12) == 0
    sess = uv.beam_session(9, nb, max_prompt=mp, max_new=12)
    rows, caps = [r["row"] for r in reqs], [r["cap"] for r in reqs]
    bad = [dict(INFER, temperature=0.0), dict(INFER, top_k=0), dict(INFER, top_k=2000, top_p=1.0)]
    for b in bad:
        with pytest.raises(RuntimeError):
            sess.admit(rows, caps, beam=[reqs[0]["beam"], dict(b, seed=3)])
    with pytest.raises(ValueError, match="caps"):
        sess.admit(rows, [12, 13], beam=[r["beam"] for r in reqs])
    assert sess.free_groups == [0, 1, 2]
    # the library checks every request itself: num_beams, the cap and the parameters; a bad one refuses the whole call
    emb = torch.stack([torch.nn.functional.pad(r, (0, 0, 0, mp - r.shape[0])) for r in rows]).to(device).contiguous()
    plen = np.array([r.shape[0] for r in rows], np.int32)
    ids = np.array([0, 1], np.int32)
    vp = ctypes.c_void_p

    def raw_admit(s, per, hcaps=(12, 12)):
        arr = (_lib.BeamC * 2)(*per)
        hc = np.array(hcaps, np.int32)
        torch.cuda.synchronize()
        rc = lib.idxtts_gpt_session_admit_beam(uv._h, 2, _lib.ptr(emb), mp, plen.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                               hc.ctypes.data_as(vp), ctypes.cast(arr, vp), _lib.ptr(s._ws), s._sp())
        s.stream.synchronize()
        return rc

    def bc(**kw):
        base = dict(num_beams=nb, do_sample=1, temperature=0.8, top_k=30, top_p=0.8, length_penalty=0.0, early_stopping=0, exp_noise=None,
                    seed=1)
        base.update(kw)
        return _lib.BeamC(**base)

    good = bc()
    for b in (bc(num_beams=2), bc(temperature=0.0), bc(top_k=0), bc(early_stopping=2)):
        assert raw_admit(sess, [good, b]) != 0
    assert raw_admit(sess, [good, good], hcaps=(12, 0)) != 0
    assert raw_admit(sess, [good, good], hcaps=(13, 12)) != 0
    # _admit / _admit_sampled on a beam session are refused
    samp = (_lib.SamplingC * 2)(*[_lib.SamplingC(mode=0, temperature=1.0, top_k=0, top_p=1.0, exp_noise=None, seed=0)] * 2)
    hc = np.array([12, 12], np.int32)
    torch.cuda.synchronize()
    assert lib.idxtts_gpt_session_admit(uv._h, 2, _lib.ptr(emb), mp, plen.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                        hc.ctypes.data_as(vp), _lib.ptr(sess._ws), sess._sp()) != 0
    assert lib.idxtts_gpt_session_admit_sampled(uv._h, 2, _lib.ptr(emb), mp, plen.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                                hc.ctypes.data_as(vp), ctypes.cast(samp, vp), _lib.ptr(sess._ws), sess._sp()) != 0
    assert sess.free_groups == [0, 1, 2]
    # nothing was taken: both requests are admitted now, a non-first slot of a group cannot be read, and they decode to their references
    got = {}
    assert sess.admit(rows, caps, beam=[r["beam"] for r in reqs]) == [0, 1]
    while len(got) < 2:
        for g in sess.step(4):
            out = torch.empty(12, dtype=torch.long, device=device)
            nc = ctypes.c_int(0)
            assert lib.idxtts_gpt_session_read(uv._h, g * nb + 1, _lib.ptr(out), ctypes.byref(nc), _lib.ptr(sess._ws), sess._sp()) != 0
            got[g] = sess.take(g).cpu().numpy()
    assert sess.free_groups == [0, 1, 2]
    sess.close()
    for g, r in zip((0, 1), reqs):
        assert np.array_equal(got[g], _reference(uv, r["row"], 3, nb, r["cap"], r["beam"]))
    # _admit_beam on a greedy session is refused
    gsess = uv.decode_session(6, max_prompt=mp, max_new=12)
    assert raw_admit(gsess, [good, good]) != 0
    assert gsess.free_slots == list(range(6))
    gsess.close()


def test_full_width_bf16_beam_session(device):
    """GPTConfig() with synthetic weights, 48 rows (16 groups x 3 beams), bf16 weights and KV, the reference defaults (beam-sample
    0.8 / 30 / 0.8, length_penalty 0), ~24 requests with caps over 16..48 codes."""
    cfg = GPTConfig()
    uv, _ = _model(device, cfg, "t/bsess/full", weight_format="bf16", kv_format="bf16")
    nb, groups, n = 3, 16, 24
    widths = [int(x) for x in synth.integers("t/bsess/full/w", (n,), 20, 120)]
    caps = [int(x) for x in synth.integers("t/bsess/full/caps", (n,), 16, 49)]
    reqs = _requests(uv, cfg, "t/bsess/full", n, widths, caps, [INFER], nb)
    sess = uv.beam_session(groups * nb, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=48)
    out = _run(sess, reqs, seed=7, max_admit=6)
    sess.close()
    assert sorted(out) == list(range(n))
    _check(uv, reqs, out, groups, nb, cfg.stop_mel_token, which=(0, 11, 23))
