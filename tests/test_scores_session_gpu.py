"""GPU: scores through every decode-session operation (`IDXTTS_SESSION_SCORES`, `idxtts_gpt_session_read_scored`), bit for bit on
the tiny synthetic model.  Wherever include/idxtts.h says "codes equal, bit for bit", the log-probabilities do too:
  * a row of a scored session equals row 0 of generate(return_logprobs=True) on `slots` copies of its prompt -- with bystanders
    evicted and stopped around it, and after park -> to("cpu") -> resume into another slot of another session;
  * a stopped row returns the first k values of its uninterrupted run;
  * takes admitted together equal single admissions; a forked take carries the source's first `at` values and equals a fresh
    admission with the same draws;
  * in the batch-invariant mode a row equals the B = 1 call from sessions of 4 and 16 slots;
  * refusals change nothing; a row parked from a session without the flag is byte for byte what it was, a scored row is that row
    with one segment more."""
import ctypes

import numpy as np
import pytest
import torch

import scores_cases as sk
from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
HF2 = {"sampler": "hf", "temperature": 1.3, "top_k": 5, "top_p": 0.5}
ACCEL = {"sampler": "accel", "temperature": 0.8}
GREEDY = {"sampler": "greedy"}
PENALTY = 10.0
KV = {"f32": 0, "bf16": 1, "fp8": 2}


def _model(device, cfg, tag, kv_format=None, stop_bias=-30.0):
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = stop_bias      # -30: rows run to their caps, the step counts below are exact
    return UnifiedVoice(w, cfg, device=device, kv_format=kv_format)


def _rows(uv, cfg, tag, widths):
    n = len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    return [uv.prompt_rows(conds[i:i + 1], torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens)))[0]
            for i in range(n)]


def _seeded(samp, seed):
    return samp if samp["sampler"] == "greedy" else dict(samp, seed=seed)


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _same(a, b):
    """codes and log-probabilities, bit for bit."""
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype == np.float32 and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _drain(sess, want, got=None, steps=3):
    got = {} if got is None else got
    t = 0
    while not set(want) <= set(got):
        for s in sess.step(steps):
            got[s] = _np(sess.take(s, scores=True))
        t += 1
        assert t < 1000
    return got


def _generate_row0(uv, row, cap, samp, slots, use_graph):
    """Row 0 of generate(return_logprobs=True) on `slots` copies of the prompt: (codes, lp)."""
    P, d = row.shape
    fake = torch.ones(slots, P + 1, dtype=torch.long)
    fake[:, -1] = uv.cfg.start_mel_token
    kw = {}
    if samp["sampler"] != "greedy":
        kw = dict(do_sample=True, sampler=samp["sampler"], temperature=samp["temperature"], top_k=samp.get("top_k", 0),
                  top_p=samp.get("top_p", 1.0), seed=samp["seed"])
    seq, lp = uv.generate(fake, max_new_tokens=cap, tts_embeddings=row[None].expand(slots, P, d).contiguous(), repetition_penalty=PENALTY,
                          use_graph=use_graph, return_logprobs=True, **kw)
    return seq[0, P + 1:].cpu().numpy(), lp[0].cpu().numpy()


def _alone(uv, row, cap, samp, slots, mp, mx, use_graph):
    sess = uv.decode_session(slots, max_prompt=mp, max_new=mx, repetition_penalty=PENALTY, use_graph=use_graph, sampled=True, scores=True)
    (s,) = sess.admit([row], [cap], sampling=[samp])
    out = _drain(sess, [s])[s]
    sess.close()
    return out


@pytest.mark.parametrize("slots", [4, 16])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_session_rows_equal_generate_row0(device, kv, use_graph, slots):
    """Two bystanders (one evicted, one stopped) around a greedy row and two sampled rows; one sampled row is parked, moved to host
    memory and resumed into another slot of another session.  bf16 cache: the exact GEMM mode, so that the reference batch's prefill and
    the admission's run the same kernels at every row count."""
    cfg = GPTConfig.tiny()
    uv = _model(device, cfg, "t/scores/sess", kv_format=kv)
    rows = _rows(uv, cfg, "t/scores/sess", [5, 12])
    mp, mx = max(r.shape[0] for r in rows), 20
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32 if kv == "bf16" else _lib.GEMM_BF16X3)
        mk = lambda: uv.decode_session(slots, max_prompt=mp, max_new=mx, repetition_penalty=PENALTY, use_graph=use_graph,      # noqa: E731
                                       sampled=True, scores=True)
        A, B = mk(), mk()
        b_stop = (1, 20, _seeded(HF2, 5))
        (s_ev, s_st) = A.admit([rows[1], rows[b_stop[0]]], [20, b_stop[1]], sampling=[GREEDY, b_stop[2]], slots=[1, 2])
        A.step(2)
        want = {0: (0, 14, GREEDY), 3: (1, 17, _seeded(HF, 11))}
        assert A.admit([rows[0], rows[1]], [14, 17], sampling=[want[0][2], want[3][2]], slots=[0, 3]) == [0, 3]
        A.step(1)
        A.evict(s_ev)
        A.step(1)
        A.stop(s_st)
        assert A.step(0) == [s_st]
        stopped = _np(A.take(s_st, scores=True))
        k = len(stopped[0])
        assert k == 1 + 2 + 2 and len(stopped[1]) == k      # its first code, then four steps
        # a third sampled row into the evicted slot, beside the running ones
        want[s_ev] = (0, 9, _seeded(ACCEL, 12))
        assert A.admit([rows[0]], [9], sampling=[want[s_ev][2]], slots=[s_ev]) == [s_ev]
        A.step(3)
        parked = A.park(3)
        assert parked.n_codes == 1 + 2 + 3 and 3 in A.free_slots
        parked.to("cpu")
        assert parked.device.type == "cpu"
        assert B.resume(parked, slot=2) == 2
        got = _drain(A, [0, s_ev])
        got[3] = _drain(B, [2])[2]
        A.close()
        B.close()
        for s, (i, cap, samp) in want.items():
            ref = _generate_row0(uv, rows[i], cap, samp, slots, use_graph)
            assert len(got[s][0]) == cap and _same(got[s], ref), (s, got[s][1][:6], ref[1][:6])
            assert np.isfinite(got[s][1]).all() and (got[s][1] < 0).all()
        ref = _generate_row0(uv, rows[b_stop[0]], b_stop[1], b_stop[2], slots, use_graph)
        assert _same(stopped, (ref[0][:k], ref[1][:k])), "a stopped row returns the first k values of its uninterrupted run"
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


@pytest.mark.parametrize("kv,use_graph,slots", [("f32", True, 4), ("f32", False, 16), ("bf16", True, 16), ("fp8", True, 4), ("fp8", False, 16)])
def test_takes_and_forks_carry_their_scores(device, kv, use_graph, slots):
    """admit(takes=3) against single admissions; then a source with explicit draws forked at 0, 1 and mid-row."""
    cfg = GPTConfig.tiny()
    uv = _model(device, cfg, "t/scores/takes", kv_format=kv)
    V = cfg.number_mel_codes
    rows = _rows(uv, cfg, "t/scores/takes", [5, 12])
    mp, mx = max(r.shape[0] for r in rows), 16
    sess = uv.decode_session(slots, max_prompt=mp, max_new=mx, repetition_penalty=PENALTY, use_graph=use_graph, sampled=True, scores=True)
    samps = [_seeded(HF, 21), GREEDY, _seeded(ACCEL, 22)]
    caps = [14, 14, 10]
    (ids,) = sess.admit([rows[0]], [caps], sampling=[samps], takes=3, slots=[3, 0, 2])
    got = _drain(sess, ids)
    for s, cap, samp in zip(ids, caps, samps):
        assert _same(got[s], _alone(uv, rows[0], cap, samp, slots, mp, mx, use_graph)), (s, samp)
    # fork: explicit draws, spliced so that a take's draws equal the source's below `at`
    noise = lambda seed, cap: torch.empty(cap, V).exponential_(1, generator=torch.Generator().manual_seed(seed)).to(device)      # noqa: E731
    E = noise(31, 16)
    (src,) = sess.admit([rows[1]], [16], sampling=[dict(HF, exp_noise=E)], slots=[1])
    sess.step(6)      # 7 codes
    takes = {}
    for j, at in enumerate((0, 1, 4)):
        Et = noise(40 + j, 16)
        Et[:at] = E[:at]
        (d,) = sess.fork(src, samplers=[dict(HF, exp_noise=Et)], at=at, slots=[(0, 2, 3)[j]])
        takes[d] = (at, Et)
    got = _drain(sess, [src] + list(takes))
    sess.close()
    assert _same(got[src], _alone(uv, rows[1], 16, dict(HF, exp_noise=E), slots, mp, mx, use_graph)), "the source is only read"
    for d, (at, Et) in takes.items():
        assert np.array_equal(got[d][1][:at].view(np.uint32), got[src][1][:at].view(np.uint32)) and np.array_equal(got[d][0][:at], got[src][0][:at])
        assert _same(got[d], _alone(uv, rows[1], 16, dict(HF, exp_noise=Et), slots, mp, mx, use_graph)), f"take forked at {at}"
    assert len({tuple(got[d][0]) for d in takes}) > 1, "every take drew the same codes: the test shows nothing"


@pytest.mark.parametrize("slots", [4, 16])
def test_batch_invariant_scores_equal_the_single_call(device, slots):
    cfg = GPTConfig.tiny()
    uv = _model(device, cfg, "t/scores/inv")
    uv.set_batch_invariant(True)
    rows = _rows(uv, cfg, "t/scores/inv", [5, 12])
    mp = max(r.shape[0] for r in rows)
    want = [(0, 12, GREEDY), (1, 15, _seeded(HF, 3)), (0, 15, _seeded(ACCEL, 4))]
    sess = uv.decode_session(slots, max_prompt=mp, max_new=15, repetition_penalty=PENALTY, sampled=True, scores=True)
    (a,) = sess.admit([rows[0]], [12], sampling=[GREEDY], slots=[slots - 1])
    sess.step(2)
    ids = [a] + sess.admit([rows[1], rows[0]], [15, 15], sampling=[want[1][2], want[2][2]], slots=[0, 2])
    got = _drain(sess, ids)
    sess.close()
    for s, (i, cap, samp) in zip(ids, want):
        assert _same(got[s], _generate_row0(uv, rows[i], cap, samp, 1, True)), (slots, s, samp)


def test_refusals_change_nothing_and_parked_rows_keep_their_layout(device):
    cfg = GPTConfig.tiny()
    uv = _model(device, cfg, "t/scores/refuse", kv_format="fp8")
    V = cfg.number_mel_codes
    (row,) = _rows(uv, cfg, "t/scores/refuse", [7])
    mp, mx = row.shape[0], 12
    with pytest.raises(ValueError, match="scorer"):
        uv.beam_session(4, 2, max_prompt=mp, max_new=mx, scores=True)
    mk = lambda scores: uv.decode_session(4, max_prompt=mp, max_new=mx, repetition_penalty=PENALTY, sampled=True, scores=scores)      # noqa: E731
    plain, scored = mk(False), mk(True)
    samp = _seeded(HF, 9)
    (p,) = plain.admit([row], [mx], sampling=[samp], slots=[1])
    (s,) = scored.admit([row], [mx], sampling=[samp], slots=[2])
    plain.step(4)
    scored.step(4)
    rp, rs = plain.park(p), scored.park(s)
    hp = _lib.ParkHeaderC.from_buffer_copy(rp._blob[:128].cpu().numpy().tobytes())
    hs = _lib.ParkHeaderC.from_buffer_copy(rs._blob[:128].cpu().numpy().tobytes())
    assert list(hp.reserved) == [0] * 8 and list(hs.reserved) == [0, 1] + [0] * 6
    args = (KV["fp8"], cfg.layers, cfg.heads, V, hp.pos, hp.step)
    assert (hs.pos, hs.step) == (hp.pos, hp.step) == (mp + 5, 5)
    lay_p, lay_s = sk.park_bytes(*args), sk.park_bytes(*args, scores=True)
    assert rp.nbytes == hp.bytes == sk.parent_park_bytes(*args) == lay_p["bytes"], "a row without scores is what it always was"
    assert rs.nbytes == hs.bytes == lay_s["bytes"] == lay_p["bytes"] + 32
    bp, bs = rp._blob.cpu().numpy(), rs._blob.cpu().numpy()
    # the scored row = the plain row with the segment put in behind the codes (headers: the size and the flag differ)
    assert np.array_equal(bp[128:lay_p["kv"]], bs[128:lay_s["logprobs"]]) and np.array_equal(bp[lay_p["kv"]:], bs[lay_s["kv"]:])
    seg = bs[lay_s["logprobs"]:lay_s["kv"]].view(np.float32)
    assert (seg[:5] < 0).all() and (seg[5:] == 0).all()
    # resume across the flag is refused either way, before anything changes
    with pytest.raises(RuntimeError, match="IDXTTS_SESSION_SCORES"):
        scored.resume(rp, slot=0)
    with pytest.raises(RuntimeError, match="IDXTTS_SESSION_SCORES"):
        plain.resume(rs, slot=0)
    assert plain.free_slots == [0, 1, 2, 3] and scored.free_slots == [0, 1, 2, 3] and not rp.resumed and not rs.resumed
    assert plain.resume(rp, slot=3) == 3 and scored.resume(rs, slot=0) == 0
    while not plain.step(4):
        pass
    got = _drain(scored, [0])[0]
    assert np.array_equal(got[1][:5].view(np.uint32), seg[:5].view(np.uint32)), "the segment holds the row's first values"
    # _read_scored on a session without the flag: refused, the slot keeps its request
    with pytest.raises(ValueError, match="scores=True"):
        plain.take(3, scores=True)
    out = torch.empty(mx, dtype=torch.long, device=device)
    lp = torch.empty(mx, dtype=torch.float32, device=device)
    n = ctypes.c_int(0)
    rc = _lib.load().idxtts_gpt_session_read_scored(uv._h, 3, _lib.ptr(out), _lib.ptr(lp), ctypes.byref(n), _lib.ptr(plain._ws), plain._sp())
    assert rc != 0 and b"IDXTTS_SESSION_SCORES" in _lib.load().idxtts_last_error()
    codes = plain.take(3).cpu().numpy()
    assert np.array_equal(codes, got[0]), "the codes do not depend on the flag"
    plain.close()
    scored.close()
    # flags 0 and 1 keep their sizes; the flag adds the table
    lib = _lib.load()
    size = lambda f: int(lib.idxtts_gpt_session_workspace_bytes_ex(uv._h, 16, mp, 100, f))      # noqa: E731
    table = 16 * 100 * 4      # [slots][max_new_tokens] fp32; sizes are rounded up to 256 bytes
    assert size(0) == int(lib.idxtts_gpt_session_workspace_bytes(uv._h, 16, mp, 100)) and size(1) > size(0)
    assert table - 256 < size(2) - size(0) <= table + 256 and table - 256 < size(3) - size(1) <= table + 256 and size(4) == 0
