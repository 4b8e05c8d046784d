"""GPU: ending requests of a decode session from outside -- `evict` and `stop` of `DecodeSession` / `BeamDecodeSession`
(`idxtts_gpt_session_evict`, `idxtts_gpt_session_stop`).

Contracts pinned here, all bit for bit:
  * neighbours are untouched: with evict and stop calls between steps every other request still equals row 0 of `generate` /
    `generate_beam` on `slots` (slots / num_beams) copies of its prompt with its own cap, sampler and seed;
  * a freed place is clean: a request admitted into an evicted slot or group meets the same contract;
  * stop is a cap set late: a request stopped after k codes returns what the same request with max_new_tokens = k returns (greedy and
    sampled: the first k codes of its uninterrupted run);
  * no phantom results: step never reports an evicted id, take on it raises; a stopped id is reported once.
The stop token is biased away (mel_head.bias[stop] = -1e4), so no row or group ends by itself before its cap: every end seen here
before a cap is one the test asked for."""
import ctypes

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
ACCEL = {"sampler": "accel", "temperature": 0.8}
GREEDY = {"sampler": "greedy"}
INFER = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}
SEARCH = {"do_sample": False, "length_penalty": 1.0}

_MODELS, _REFS = {}, {}


def _model(device, kv):
    """One model per KV format for the whole module (the references below are computed once on it)."""
    from indextts_amd.gpt import UnifiedVoice
    if kv not in _MODELS:
        cfg = GPTConfig.tiny()
        w = weights.synth_gpt_weights(cfg, tag="t/evict/model")
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = -1e4
        _MODELS[kv] = UnifiedVoice(w, cfg, device=device, kv_format=kv)
    return _MODELS[kv]


def _requests(uv, tag, widths, caps, extra=None):
    """Prompts ([P, d] rows) of the given text widths, each with its own conditioning; extra[i]: the request's sampler or beam dict."""
    cfg, n = uv.cfg, len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "par": dict(extra[i]) if extra else None,
                     "key": (tag, i)})
    return reqs


def _copies(uv, row, n):
    P, d = row.shape
    ids = torch.ones(n, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    return ids, row[None].expand(n, P, d).contiguous(), P


def _reference(uv, r, copies, cap=None, nb=0):
    """Row 0 of generate() -- nb > 0: generate_beam() -- on `copies` copies of the request's prompt with its own parameters and cap (or
    `cap`).  Computed once per (model, request, cap) and shared by the tests."""
    cap = int(cap or r["cap"])
    key = (uv.kv_format, r["key"], copies, cap, nb)
    if key not in _REFS:
        ids, emb, P = _copies(uv, r["row"], copies)
        p = r["par"] or {}
        if nb:
            kw = dict(num_beams=nb, do_sample=p["do_sample"], temperature=p.get("temperature", 1.0), top_k=p.get("top_k", 50),
                      top_p=p.get("top_p", 1.0), length_penalty=p["length_penalty"], early_stopping=False)
            if p.get("exp_noise") is not None:
                nz = p["exp_noise"][:cap]
                kw["exp_noise"] = nz[:, None, :].expand(cap, copies, nz.shape[1]).contiguous()
            else:
                kw["seed"] = p["seed"]
            out = uv.generate_beam(ids, cap, None, emb, repetition_penalty=10.0, **kw)
        else:
            kw = {}
            if p.get("sampler", "greedy") != "greedy":
                kw = dict(do_sample=True, sampler=p["sampler"], temperature=p["temperature"], top_k=p.get("top_k", 0), top_p=p.get("top_p", 1.0))
                if p.get("exp_noise") is not None:
                    nz = p["exp_noise"][:cap]
                    kw["exp_noise"] = nz[:, None, :].expand(cap, copies, nz.shape[1]).contiguous()
                else:
                    kw["seed"] = p["seed"]
            out = uv.generate(ids, max_new_tokens=cap, tts_embeddings=emb, repetition_penalty=10.0, **kw)
        c = out[0, P + 1:].cpu().numpy()
        hits = np.nonzero(c == uv.cfg.stop_mel_token)[0]
        _REFS[key] = c[: hits[0] + 1] if len(hits) else c
    return _REFS[key]


def _finish(sess, where, rng, out):
    """Steps a random number of steps at a time until every request of `where` ({slot or group: request index}) is collected.  step may
    only ever report a place that holds one of them: an evicted id that was not admitted again, or a stopped one that was taken,
    showing up here fails the test."""
    t = 0
    while where:
        for u in sess.step(int(rng.integers(1, 6))):
            assert u in where, f"step reported {u}, which holds no request of the test"
            out[where.pop(u)] = sess.take(u).cpu().numpy()
        t += 1
        assert t < 1000
    return out


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_evict_mid_flight_and_reuse(device, kv, use_graph):
    """4 rows admitted, 5 steps, the two middle ones evicted, two new prompts admitted into their slots: the survivors and the newcomers
    equal their references, and no step reports an evicted slot before it holds a new request."""
    uv = _model(device, kv)
    slots = 4
    # bf16 cache + split-bf16 GEMMs: texts long enough that the reference's prefill (4 x (P + 1) rows) is >= 256 rows too
    widths = [56, 58, 57, 60, 59, 56] if kv == "bf16" else [9, 31, 4, 17, 23, 12]
    reqs = _requests(uv, f"t/evict/greedy/{kv == 'bf16'}", widths, [24, 40, 33, 29, 26, 37])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=40, use_graph=use_graph)
    rng = np.random.default_rng(11)
    assert sess.admit([r["row"] for r in reqs[:4]], [r["cap"] for r in reqs[:4]]) == [0, 1, 2, 3]
    assert sess.step(5) == []
    assert {1, 2} <= set(sess.live_slots)
    sess.evict([1, 2])
    assert {1, 2} <= set(sess.free_slots) and not {1, 2} & set(sess.live_slots)
    assert sess.step(0) == [] and sess.step(1) == []
    assert sess.admit([r["row"] for r in reqs[4:]], [r["cap"] for r in reqs[4:]]) == [1, 2]
    out = _finish(sess, {0: 0, 3: 3, 1: 4, 2: 5}, rng, {})
    sess.close()
    for i in (0, 3, 4, 5):
        ref = _reference(uv, reqs[i], slots)
        assert len(ref) == reqs[i]["cap"], "the row stopped by itself: the stop bias is not low enough"
        assert np.array_equal(out[i], ref), (i, out[i][:12], ref[:12])


def test_evict_states_and_refusals(device):
    """Evict right after admit; evict a slot that ended and was not taken; bad ids (a free slot, out of range, one bad id in a list)
    raise and change nothing, in Python and at the C ABI; take on an evicted slot raises.  The other rows finish against their
    references, and a request admitted into a slot evicted at step 0 does too."""
    uv = _model(device, "f32")
    slots = 4
    reqs = _requests(uv, "t/evict/states", [7, 15, 11, 5, 20], [21, 26, 3, 30, 18])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=30)
    lib, vp = _lib.load(), ctypes.c_void_p
    assert sess.admit([r["row"] for r in reqs[:4]], [r["cap"] for r in reqs[:4]]) == [0, 1, 2, 3]
    sess.evict(3)                                                   # before any step
    assert sess.free_slots == [3]
    with pytest.raises(RuntimeError):
        sess.take(3)
    for bad in (3, 4, -1, [0, 3], [1, 9], "0"):                     # free, out of range, a list with one bad id
        for op in (sess.evict, sess.stop):
            with pytest.raises(ValueError):
                op(bad)
    for ids in ([3], [4], [-1], [0, 3], [1, 64]):                   # the library's own checks
        h = np.array(ids, np.int32)
        for fn in (lib.idxtts_gpt_session_evict, lib.idxtts_gpt_session_stop):
            assert fn(uv._h, len(ids), h.ctypes.data_as(vp), _lib.ptr(sess._ws), sess._sp()) != 0
    assert sess.free_slots == [3] and sess.live_slots == [0, 1, 2]
    fin = sess.step(4)                                              # request 2 (cap 3) has ended
    assert fin == [2] and sess.step(0) == [2]
    sess.evict([2])                                                 # ended, not taken
    assert sess.free_slots == [2, 3] and sess.step(0) == []
    with pytest.raises(RuntimeError):
        sess.take(2)
    assert sess.admit([reqs[4]["row"]], [reqs[4]["cap"]]) == [2]
    out = _finish(sess, {0: 0, 1: 1, 2: 4}, np.random.default_rng(5), {})
    assert sess.free_slots == [0, 1, 2, 3]
    sess.close()
    for i in (0, 1, 4):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), i


def test_stop_is_a_cap_set_late(device):
    """7 steps after admission a live slot is stopped: step(0) reports it, take returns its k = 8 codes -- the reference with cap k and
    the prefix of its uninterrupted run -- and it is never reported again.  Stopping a slot that has already ended changes nothing."""
    uv = _model(device, "f32")
    slots = 4
    reqs = _requests(uv, "t/evict/stop", [12, 6, 19, 9], [30, 34, 27, 3])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=34)
    assert sess.admit([r["row"] for r in reqs], [r["cap"] for r in reqs]) == [0, 1, 2, 3]
    assert sess.step(7) == [3]                                      # cap 3: ended by itself
    sess.stop([3, 1])                                               # 3 has ended: left alone; 1 is live
    assert 1 in sess.live_slots
    assert sorted(sess.step(0)) == [1, 3]
    got1, got3 = sess.take(1).cpu().numpy(), sess.take(3).cpu().numpy()
    k = len(got1)
    assert k == 8                                                   # the first token at admission + 7 steps
    assert np.array_equal(got1, _reference(uv, reqs[1], slots, cap=k))
    assert np.array_equal(got1, _reference(uv, reqs[1], slots)[:k])
    assert np.array_equal(got3, _reference(uv, reqs[3], slots))
    out = _finish(sess, {0: 0, 2: 2}, np.random.default_rng(3), {})
    sess.close()
    for i in (0, 2):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), i


def test_sampled_session_evict_reuse_and_stop(device):
    """One HF row by seed, one HF row with its own draws, one accel row, one greedy row.  The row that reads an exp_noise tensor is evicted
    and a seeded one admitted into its slot; the seeded HF row is stopped and equals generate(seed=..., max_new_tokens=k)."""
    uv = _model(device, "f32")
    slots, V = 4, uv.cfg.number_mel_codes
    g = torch.Generator().manual_seed(77)
    par = [dict(HF, seed=1234), dict(HF, exp_noise=torch.empty(28, V).exponential_(1.0, generator=g)), dict(ACCEL, seed=99), dict(GREEDY),
           dict(HF, seed=4321)]
    reqs = _requests(uv, "t/evict/sampled", [10, 22, 5, 14, 8], [32, 28, 25, 30, 19], extra=par)
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=32, sampled=True)
    assert sess.admit([r["row"] for r in reqs[:4]], [r["cap"] for r in reqs[:4]], sampling=[r["par"] for r in reqs[:4]]) == [0, 1, 2, 3]
    assert sess.step(5) == []
    assert 1 in sess._noise
    sess.evict(1)
    assert 1 not in sess._noise and sess.free_slots == [1]
    assert sess.admit([reqs[4]["row"]], [reqs[4]["cap"]], sampling=[reqs[4]["par"]]) == [1]
    assert sess.step(2) == []
    sess.stop(0)
    assert sess.step(0) == [0]
    got0 = sess.take(0).cpu().numpy()
    k = len(got0)
    assert k == 8
    assert np.array_equal(got0, _reference(uv, reqs[0], slots, cap=k))
    assert np.array_equal(got0, _reference(uv, reqs[0], slots)[:k])
    out = _finish(sess, {1: 4, 2: 2, 3: 3}, np.random.default_rng(8), {})
    sess.close()
    for i in (2, 3, 4):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), (i, reqs[i]["par"]["sampler"])


@pytest.mark.parametrize("nb,slots,beam,noise", [(3, 6, INFER, False), (2, 8, SEARCH, False), (2, 8, INFER, True)])
def test_beam_session_evict_reuse_and_stop(device, nb, slots, beam, noise):
    """A live group is evicted mid-flight and a new request admitted into it; another group is stopped after k steps and equals
    generate_beam(max_new_tokens=k) (with its own draws: their first k rows); the place of the stopped group is used again.  Neighbours
    and newcomers equal generate_beam on slots / num_beams copies."""
    uv = _model(device, "f32")
    groups, V = slots // nb, uv.cfg.number_mel_codes
    n = groups + 2
    widths = [8, 19, 5, 13, 24, 10][:n]
    caps = [22, 26, 24, 20, 18, 23][:n]
    par = []
    for i in range(n):
        p = dict(beam)
        if noise:
            p["exp_noise"] = torch.empty(caps[i], nb * V).exponential_(1.0, generator=torch.Generator().manual_seed(300 + i))
        else:
            p["seed"] = 1000 + 7919 * i
        par.append(p)
    reqs = _requests(uv, f"t/evict/beam/{nb}/{beam['do_sample']}/{noise}", widths, caps, extra=par)
    sess = uv.beam_session(slots, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=26)
    first = list(range(groups))
    assert sess.admit([reqs[i]["row"] for i in first], [reqs[i]["cap"] for i in first], beam=[reqs[i]["par"] for i in first]) == first
    assert sess.step(4) == []
    ev, st = 0, groups - 1                                          # evicted group, stopped group
    assert {ev, st} <= set(sess.live_groups)
    with pytest.raises(ValueError):
        sess.evict([ev, groups])
    sess.evict(ev)
    assert sess.free_groups == [ev] and sess.step(0) == []
    with pytest.raises(RuntimeError):
        sess.take(ev)
    assert sess.admit([reqs[groups]["row"]], [reqs[groups]["cap"]], beam=[reqs[groups]["par"]]) == [ev]
    assert sess.step(3) == []
    sess.stop(st)
    assert sess.step(0) == [st]
    k = 1 + 4 + 3                                                   # the first beam step at admission + the steps since
    got = sess.take(st).cpu().numpy()
    assert np.array_equal(got, _reference(uv, reqs[st], groups, cap=k, nb=nb)), (got, _reference(uv, reqs[st], groups, cap=k, nb=nb))
    assert sess.admit([reqs[groups + 1]["row"]], [reqs[groups + 1]["cap"]], beam=[reqs[groups + 1]["par"]]) == [st]
    where = {g: g for g in range(groups) if g not in (ev, st)}
    where.update({ev: groups, st: groups + 1})
    out = _finish(sess, where, np.random.default_rng(nb), {})
    sess.close()
    for i in where.values():
        assert np.array_equal(out[i], _reference(uv, reqs[i], groups, nb=nb)), (i, out[i][:12])
