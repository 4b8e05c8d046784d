"""GPU: preempt and resume of decode rows -- `DecodeSession.park` / `resume` (`idxtts_gpt_session_park_bytes`, `_park`, `_resume`).

The contract, bit for bit and without a tolerance: a row whose state is gathered into a parked row and scattered back -- into any slot,
at any later time, from device or host memory, in the session it left or in another one of the same shape -- goes on to produce the
codes of its uninterrupted run, which are row 0 of `UnifiedVoice.generate` on `slots` copies of its prompt; nobody else's codes move;
`step` never reports a parked slot.  A parked row is a function of the request's state alone (no uninitialised padding), and every
refusal leaves everything as it was.  The stop token is biased away (mel_head.bias[stop] = -1e4): rows end at their caps only."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig
from indextts_amd.gpt import ParkedRow

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
ACCEL = {"sampler": "accel", "temperature": 0.8}
GREEDY = {"sampler": "greedy"}
KV_CODE = {"f32": 0, "bf16": 1, "fp8": 2}

_MODELS, _REFS = {}, {}


def _model(device, kv, weight_format="f32", inst=0):
    """One model per (KV format, weight format) for the whole module; inst > 0: another model built from the same weights."""
    from indextts_amd.gpt import UnifiedVoice
    key = (kv, weight_format, inst)
    if key not in _MODELS:
        cfg = GPTConfig.tiny()
        w = weights.synth_gpt_weights(cfg, tag="t/park/model")
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = -1e4
        _MODELS[key] = UnifiedVoice(w, cfg, device=device, weight_format=weight_format, kv_format=kv)
        _MODELS[key]._park_key = key[:2]      # models of one key pair compute the same references
    return _MODELS[key]


def _requests(uv, tag, widths, caps, extra=None):
    cfg, n = uv.cfg, len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "par": dict(extra[i]) if extra else None,
                     "key": (tag, i)})
    return reqs


def _reference(uv, r, copies):
    """Row 0 of generate() on `copies` copies of the request's prompt with its own sampler and cap: code that exists without this
    feature.  Computed once per (model kind, request) and shared."""
    key = (uv._park_key, r["key"], copies)
    if key not in _REFS:
        row, cap = r["row"], r["cap"]
        P, d = row.shape
        ids = torch.ones(copies, P + 1, dtype=torch.long)
        ids[:, -1] = uv.cfg.start_mel_token
        emb = row[None].expand(copies, P, d).contiguous()
        p, kw = r["par"] or {}, {}
        if p.get("sampler", "greedy") != "greedy":
            kw = dict(do_sample=True, sampler=p["sampler"], temperature=p["temperature"], top_k=p.get("top_k", 0), top_p=p.get("top_p", 1.0))
            if p.get("exp_noise") is not None:
                nz = p["exp_noise"][:cap]
                kw["exp_noise"] = nz[:, None, :].expand(cap, copies, nz.shape[1]).contiguous()
            else:
                kw["seed"] = p["seed"]
        out = uv.generate(ids, max_new_tokens=cap, tts_embeddings=emb, repetition_penalty=10.0, **kw)
        c = out[0, P + 1:].cpu().numpy()
        assert len(c) == cap and uv.cfg.stop_mel_token not in c, "the row stopped by itself: the stop bias is not low enough"
        _REFS[key] = c
    return _REFS[key]


def _collect(sess, where, out, n):
    """One step(n); every finished place must hold a request of the test (a parked slot showing up here fails)."""
    for u in sess.step(n):
        assert u in where, f"step reported {u}, which holds no request of the test"
        out[where.pop(u)] = sess.take(u).cpu().numpy()


def _finish(sess, where, rng, out):
    t = 0
    while where:
        _collect(sess, where, out, int(rng.integers(1, 6)))
        t += 1
        assert t < 1000
    return out


def _hdr(parked):
    n = ctypes.sizeof(_lib.ParkHeaderC)
    return _lib.ParkHeaderC.from_buffer_copy(parked._blob[:n].cpu().numpy().tobytes())


def _pad16(n):
    return (n + 15) & ~15


def _park_bytes(cfg, kv, pos, step):
    """The size formula of include/idxtts.h, restated."""
    C, g, e = {"f32": (16, 16, 4), "bf16": (8, 16, 2), "fp8": (8, 8, 1)}[kv]
    per_head = C * _pad16(pos * g) + pos * 64 * e + (2 * _pad16(4 * pos) if kv == "fp8" else 0)
    return 128 + _pad16(cfg.number_mel_codes) + _pad16(8 * step) + cfg.layers * cfg.heads * per_head


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_park_resume_round_trip(device, kv, use_graph):
    """4 rows, 5 steps, slots 1 and 2 parked, two newcomers admitted there, 7 steps, slot 0 parked, the first two parked rows resumed
    into slots they did not leave, the third one later into a fourth slot: all six requests equal their references."""
    uv = _model(device, kv)
    slots = 4
    widths = [56, 58, 57, 60, 59, 56] if kv == "bf16" else [9, 31, 4, 17, 23, 12]
    reqs = _requests(uv, f"t/park/rt/{kv == 'bf16'}", widths, [30, 26, 33, 16, 8, 29])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=40, use_graph=use_graph)
    rng, out = np.random.default_rng(11), {}
    assert sess.admit([r["row"] for r in reqs[:4]], [r["cap"] for r in reqs[:4]]) == [0, 1, 2, 3]
    assert sess.step(5) == []
    pa, pb = sess.park(1), sess.park(2)
    assert isinstance(pa, ParkedRow) and (pa.n_codes, pa.cap, pb.n_codes, pb.cap) == (6, 26, 6, 33)
    assert sess.free_slots == [1, 2] and sess.live_slots == [0, 3] and sess.step(0) == []
    assert sess.admit([r["row"] for r in reqs[4:]], [r["cap"] for r in reqs[4:]]) == [1, 2]
    where = {0: 0, 1: 4, 2: 5, 3: 3}
    _collect(sess, where, out, 7)
    assert sorted(where) == [0, 2, 3], "the newcomer with cap 8 ends after 7 steps"
    pc = sess.park(0)
    del where[0]
    assert pc.n_codes == 13 and sess.free_slots == [0, 1]
    assert sess.resume(pa, 0) == 0 and sess.resume(pb) == 1            # they left slots 1 and 2
    where.update({0: 1, 1: 2})
    assert pa.resumed and pb.resumed and sess.free_slots == []
    while 3 in where:                                                # request 3 (cap 16) ends next
        _collect(sess, where, out, 1)
    assert sess.resume(pc) == 3
    where[3] = 0
    _finish(sess, where, rng, out)
    sess.close()
    for i in range(6):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), (i, out[i][:12], _reference(uv, reqs[i], slots)[:12])


@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_park_edge_positions(device, kv):
    """A row parked right after admit (one code), a row parked one step before its cap, an odd and an even pos, and a resume into a slot
    whose previous tenant cached more keys than the parked row has: stale keys beyond pos do not matter."""
    uv = _model(device, kv)
    slots = 4
    reqs = _requests(uv, f"t/park/edge/{kv == 'bf16'}", [60, 56, 58, 57] if kv == "bf16" else [30, 4, 10, 7], [12, 20, 9, 30])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=30)
    out = {}
    assert sess.admit([r["row"] for r in reqs], [r["cap"] for r in reqs]) == [0, 1, 2, 3]
    p1 = sess.park(1)                                                # before any step
    h1 = _hdr(p1)
    assert (p1.n_codes, h1.step, h1.pos) == (1, 1, reqs[1]["row"].shape[0] + 1)
    where = {0: 0, 2: 2, 3: 3}
    _collect(sess, where, out, 7)
    assert sorted(where) == [0, 2, 3]
    p2 = sess.park(2)
    del where[2]
    h2 = _hdr(p2)
    assert h2.step == h2.max_step - 1 == 8, "one step is left before the cap"
    assert {h1.pos % 2, h2.pos % 2} == {0, 1}, "an odd and an even row length"
    _collect(sess, where, out, 4)                                    # request 0 (cap 12) ends: its slot has cached P0 + 11 keys
    assert sorted(where) == [3] and reqs[0]["row"].shape[0] + 11 > h1.pos
    assert sess.resume(p1, 0) == 0 and sess.resume(p2, 1) == 1
    where.update({0: 1, 1: 2})
    _collect(sess, where, out, 1)
    assert 1 not in where, "the row parked one step before its cap ends with the next step"
    _finish(sess, where, np.random.default_rng(4), out)
    sess.close()
    for i in range(4):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), (i, out[i][:12])


def test_park_slot_stride(device):
    """Slot 0 -> the last slot and the last -> 0 (the largest slot strides of the cache)."""
    uv = _model(device, "fp8")
    slots = 4
    reqs = _requests(uv, "t/park/stride", [13, 6, 21, 9], [19, 22, 17, 24])
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24)
    assert sess.admit([r["row"] for r in reqs], [r["cap"] for r in reqs]) == [0, 1, 2, 3]
    assert sess.step(3) == []
    first, last = sess.park(0), sess.park(3)
    assert sess.step(2) == []
    assert sess.resume(first, 3) == 3 and sess.resume(last, 0) == 0
    out = _finish(sess, {0: 3, 1: 1, 2: 2, 3: 0}, np.random.default_rng(2), {})
    sess.close()
    for i in range(4):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), i


def test_park_plane_gemv_step(device):
    """bf16 weights, 20 slots: the step runs on the plane GEMV, whose input is a row plus statistics that resume rebuilds.  6 of 20 rows
    are parked at different steps and resumed into other slots."""
    uv = _model(device, "bf16", weight_format="bf16")
    assert _lib.load().idxtts_get_decode_plane_rows() <= 20
    slots = 20
    widths = [int(x) for x in synth.integers("t/park/pl/w", (slots,), 8, 30)]
    caps = [int(x) for x in synth.integers("t/park/pl/caps", (slots,), 14, 30)]
    reqs = _requests(uv, "t/park/pl", widths, caps)
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=30)
    assert sess.admit([r["row"] for r in reqs], caps) == list(range(slots))
    where, out, parked = {s: s for s in range(slots)}, {}, {}
    for n, batch in ((2, (1, 5)), (3, (8, 19)), (1, (0, 12))):
        _collect(sess, where, out, n)
        for s in batch:
            parked[s] = sess.park(s)
            del where[s]
    assert len(where) == 14 and sess.free_slots == [0, 1, 5, 8, 12, 19]
    _collect(sess, where, out, 2)
    for src, dst in ((1, 5), (5, 8), (8, 12)):
        assert sess.resume(parked[src], dst) == dst
        where[dst] = src
    _collect(sess, where, out, 1)
    for src, dst in ((19, 0), (0, 1), (12, 19)):
        assert sess.resume(parked[src], dst) == dst
        where[dst] = src
    _finish(sess, where, np.random.default_rng(6), out)
    sess.close()
    for i in range(slots):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), (i, out[i][:12])


def test_park_sampled_rows(device):
    """HF by seed, HF with its own draws, accel by seed and a greedy row in a sampled session, each parked mid-flight and resumed into
    another slot.  The exp_noise tensor travels with the parked row: the caller's reference is dropped while it is parked."""
    uv = _model(device, "f32")
    slots, V = 4, uv.cfg.number_mel_codes
    g = torch.Generator().manual_seed(78)
    par = [dict(HF, seed=1234), dict(HF, exp_noise=torch.empty(28, V).exponential_(1.0, generator=g)), dict(ACCEL, seed=99), dict(GREEDY)]
    reqs = _requests(uv, "t/park/sampled", [10, 22, 5, 14], [32, 28, 25, 30], extra=par)
    refs = [_reference(uv, r, slots) for r in reqs]
    sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=32, sampled=True)
    admit_par = [dict(r["par"]) for r in reqs]
    admit_par[1]["exp_noise"] = reqs[1]["par"]["exp_noise"].clone().to(device)      # the copy the session reads
    assert sess.admit([r["row"] for r in reqs], [r["cap"] for r in reqs], sampling=admit_par) == [0, 1, 2, 3]
    del admit_par
    assert sess.step(5) == []
    p0, p1 = sess.park(0), sess.park(1)
    assert 1 not in sess._noise and p1._noise is not None and p0._noise is None
    gc.collect()
    torch.cuda.empty_cache()
    junk = torch.full((28 * V * 4,), 7.0, device=device)              # what a freed noise tensor would be overwritten by
    assert sess.step(3) == []
    p2, p3 = sess.park(2), sess.park(3)
    assert sess.free_slots == [0, 1, 2, 3] and sess.step(2) == []
    assert [sess.resume(p, s) for p, s in ((p0, 1), (p1, 2), (p2, 3), (p3, 0))] == [1, 2, 3, 0]
    assert 2 in sess._noise and p1._noise is None
    out = _finish(sess, {1: 0, 2: 1, 3: 2, 0: 3}, np.random.default_rng(9), {})
    sess.close()
    del junk
    for i in range(4):
        assert np.array_equal(out[i], refs[i]), (i, reqs[i]["par"]["sampler"], out[i][:12], refs[i][:12])


@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_parked_row_bytes(device, kv):
    """A parked row is a function of the request's state alone: park -> resume (another slot) -> park with no step in between gives the
    same bytes, and so does the same request at the same step on a second model built from the same weights.  Its size is the documented
    formula, and for a short row less than the slot's whole cache region."""
    lib = _lib.load()
    blobs = []
    for inst in (0, 1):
        uv = _model(device, kv, inst=inst)
        cfg = uv.cfg
        reqs = _requests(uv, "t/park/bytes", [9, 5], [40, 36])         # text widths 9 and 5: rows of odd and even length below
        sess = uv.decode_session(4, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=40)
        # dirty the slots first, so that padding left unwritten or stale keys copied along would show
        assert sess.admit([reqs[1]["row"]] * 4, [30] * 4) == [0, 1, 2, 3]
        sess.step(29 if inst else 17)
        sess.evict([0, 1, 2, 3])
        assert sess.admit([r["row"] for r in reqs], [r["cap"] for r in reqs]) == [0, 1]
        assert sess.step(4 + inst) == []
        if inst:                                                     # the second model's row 1 takes a detour through another slot
            sess.resume(sess.park(1), 3)
            sess.evict(3)
        else:
            sess.step(1)
        pos, step = reqs[0]["row"].shape[0] + 1 + 5, 6
        need = int(lib.idxtts_gpt_session_park_bytes(uv._h, 0, _lib.ptr(sess._ws), sess._sp()))
        assert need == _park_bytes(cfg, kv, pos, step)
        smax = (sess.max_prompt + 1 + sess.max_new + 3) & ~3
        e = {"f32": 4, "bf16": 2, "fp8": 1}[kv]
        region = 2 * cfg.layers * cfg.heads * smax * (64 * e + (4 if kv == "fp8" else 0))
        assert need < region, (need, region)
        p = sess.park(0)
        h = _hdr(p)
        assert (h.magic, h.version, h.bytes, h.pos, h.step, h.max_step, h.mel_pos) == (0x4b525049, 1, need, pos, step, 40, step + 1)
        assert (h.layers, h.heads, h.model_dim, h.number_mel_codes, h.slots, h.kv_format) == (
            cfg.layers, cfg.heads, cfg.model_dim, cfg.number_mel_codes, 4, KV_CODE[kv])
        assert p.nbytes == need
        first = p._blob.clone()
        assert sess.resume(p, 2) == 2
        again = sess.park(2)
        assert torch.equal(again._blob, first), "park -> resume -> park moved bytes"
        blobs.append(first.cpu())
        sess.close()
    assert torch.equal(blobs[0], blobs[1]), "two models from the same weights park different bytes for the same request and step"


def test_park_to_host_and_cross_session(device):
    """ParkedRow.to("cpu") holds no device memory and resumes to equal codes; a row parked in session A resumes in a second session B of
    the same shape; A's other rows equal their references."""
    uv = _model(device, "f32")
    slots = 4
    reqs = _requests(uv, "t/park/host", [11, 24, 6, 17], [27, 23, 29, 21])
    mp = max(r["row"].shape[0] for r in reqs)
    a, b = uv.decode_session(slots, max_prompt=mp, max_new=30), uv.decode_session(slots, max_prompt=mp, max_new=30)
    assert a.admit([r["row"] for r in reqs], [r["cap"] for r in reqs]) == [0, 1, 2, 3]
    assert a.step(4) == []
    ph = a.park(2)
    assert ph.to("cpu") is ph and ph.device.type == "cpu" and ph._blob.is_pinned()
    px = a.park(1)
    assert a.step(3) == []
    assert b.resume(px) == 0 and b.live_slots == [0]
    assert a.resume(ph) == 1                                         # staged from host memory by resume itself
    out = _finish(a, {0: 0, 1: 2, 3: 3}, np.random.default_rng(5), {})
    _finish(b, {0: 1}, np.random.default_rng(6), out)
    a.close()
    b.close()
    for i in range(4):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), i


def test_park_refusals_change_nothing(device):
    """Every refused park and resume raises (Python) or returns non-zero (C ABI) and changes nothing: afterwards the session's rows
    still equal their references, and the parked row that was refused elsewhere still resumes."""
    uv, uv16 = _model(device, "f32"), _model(device, "bf16")
    lib, vp, slots = _lib.load(), ctypes.c_void_p, 4
    reqs = _requests(uv, "t/park/refuse", [7, 15, 11, 9], [21, 26, 3, 45])
    mp = max(r["row"].shape[0] for r in reqs)
    sess = uv.decode_session(slots, max_prompt=mp, max_new=34)
    ws, sp = _lib.ptr(sess._ws), sess._sp()
    assert sess.admit([r["row"] for r in reqs[:3]], [r["cap"] for r in reqs[:3]]) == [0, 1, 2]
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    wr = ctypes.c_size_t(0)
    for bad in (3, 4, -1, "0"):                                      # a free slot, out of range
        with pytest.raises(ValueError):
            sess.park(bad)
    for bad in (3, 4, -1, 64):                                       # the library's own checks
        assert lib.idxtts_gpt_session_park_bytes(uv._h, bad, ws, sp) == 0
        assert lib.idxtts_gpt_session_park(uv._h, bad, _lib.ptr(scratch), scratch.numel(), ctypes.byref(wr), ws, sp) != 0
    assert sess.step(4) == [2]                                       # request 2 (cap 3) has ended and is not read
    with pytest.raises(RuntimeError, match="ended"):
        sess.park(2)
    assert sess.step(0) == [2]
    need = int(lib.idxtts_gpt_session_park_bytes(uv._h, 0, ws, sp))
    assert need > 0
    assert lib.idxtts_gpt_session_park(uv._h, 0, _lib.ptr(scratch), need - 16, ctypes.byref(wr), ws, sp) != 0      # dst too small
    assert sess.live_slots == [0, 1] and not scratch.any()
    p = sess.park(1)
    blob = p._blob
    with pytest.raises(ValueError):
        sess.resume(p, 0)                                            # busy
    with pytest.raises(ValueError):
        sess.resume(p, 4)
    assert lib.idxtts_gpt_session_resume(uv._h, 0, _lib.ptr(blob), blob.numel(), ws, sp) != 0                      # busy
    assert lib.idxtts_gpt_session_resume(uv._h, 3, _lib.ptr(blob), blob.numel() - 16, ws, sp) != 0                 # truncated
    assert lib.idxtts_gpt_session_resume(uv._h, 3, _lib.ptr(blob), 64, ws, sp) != 0
    bad_magic = blob.clone()
    bad_magic[0] ^= 0x01
    assert lib.idxtts_gpt_session_resume(uv._h, 3, _lib.ptr(bad_magic), bad_magic.numel(), ws, sp) != 0

    def foreign(model, slots_, max_new, req, sampled=False, sampling=None):
        s = model.decode_session(slots_, max_prompt=mp, max_new=max_new, sampled=sampled)
        s.admit([req["row"]], [req["cap"]], **({"sampling": [sampling]} if sampled else {}))
        s.step(2)
        row = s.park(0)
        s.close()
        return row
    strangers = {
        "another KV format": foreign(uv16, slots, 34, reqs[0]),
        "a session with other slots": foreign(uv, 2, 34, reqs[0]),
        "a cap above max_new": foreign(uv, slots, 50, reqs[3]),
        "a sampled row": foreign(uv, slots, 34, reqs[0], sampled=True, sampling=dict(HF, seed=5)),
    }
    for what, row in strangers.items():
        with pytest.raises(RuntimeError):
            sess.resume(row, 3)
        assert not row.resumed and sess.free_slots == [1, 3], what
    assert sess.step(0) == [2]
    beam = uv.beam_session(4, 2, max_prompt=mp, max_new=20)
    assert beam.admit([reqs[0]["row"]], [12], beam={"do_sample": False, "length_penalty": 1.0}) == [0]
    with pytest.raises(NotImplementedError):
        beam.park(0)
    assert lib.idxtts_gpt_session_park_bytes(uv._h, 0, _lib.ptr(beam._ws), beam._sp()) == 0
    assert lib.idxtts_gpt_session_resume(uv._h, 2, _lib.ptr(blob), blob.numel(), _lib.ptr(beam._ws), beam._sp()) != 0
    beam.close()
    assert sess.resume(p, 3) == 3
    with pytest.raises(RuntimeError, match="resumed once"):
        sess.resume(p, 1)
    assert sess.free_slots == [1]
    out = {2: sess.take(2).cpu().numpy()}
    _finish(sess, {0: 0, 3: 1}, np.random.default_rng(3), out)
    sess.close()
    for i in range(3):
        assert np.array_equal(out[i], _reference(uv, reqs[i], slots)), i
