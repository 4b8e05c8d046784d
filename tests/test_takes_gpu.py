"""GPU: several takes per request -- admission with takes (`idxtts_gpt_session_admit_takes`), fork of a row that is already in a
session (`idxtts_gpt_session_fork`), `generate(num_return_sequences=)`, and the n best beam hypotheses
(`idxtts_gpt_generate_beam_nbest`, `idxtts_gpt_session_read_nbest`).

Contracts pinned here, all bit for bit on the tiny synthetic model:
  * every take of an admission equals the same prompt admitted alone, with that take's sampler, into a fresh session of the same
    configuration (slots, KV format, GEMM mode, graph replay);
  * a take forked at k codes with explicit draws that equal the source's below k equals a fresh admission with those draws; the
    source and every bystander equal their uninterrupted runs; a refused fork changes nothing;
  * generate(num_return_sequences=n) equals generate on the caller-expanded batch and the CPU oracle on the expanded inputs;
  * the n best beam hypotheses equal what the reference's BeamSearchScorer(num_beam_hyps_to_keep=n) returned
    (tests/golden/takes_ref.npz): tokens, lengths and order exactly, scores within a bound worked out below."""
import ctypes
import os

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
HF2 = {"sampler": "hf", "temperature": 1.3, "top_k": 5, "top_p": 0.5}
ACCEL = {"sampler": "accel", "temperature": 0.8}
GREEDY = {"sampler": "greedy"}


def _model(device, cfg, tag, kv_format=None, stop_bias=None):
    from indextts_amd.gpt import UnifiedVoice
    w = weights.synth_gpt_weights(cfg, tag=tag)
    if stop_bias is not None:
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
    return UnifiedVoice(w, cfg, device=device, kv_format=kv_format), w


def _rows(uv, cfg, tag, widths):
    """One prompt ([P, d] rows) per text width, each with its own conditioning."""
    n = len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    return [uv.prompt_rows(conds[i:i + 1], torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens)))[0]
            for i in range(n)]


def _drain(sess, want, got=None, steps=3):
    """Steps until every slot of `want` has finished; takes whatever finishes on the way.  {slot: codes}."""
    got = {} if got is None else got
    t = 0
    while not set(want) <= set(got):
        for s in sess.step(steps):
            got[s] = sess.take(s).cpu().numpy()
        t += 1
        assert t < 1000
    return got


def _alone(uv, row, cap, samp, slots, max_prompt, max_new, use_graph=True, sampled=True):
    """The rule every take is held to: the same prompt and sampler admitted alone into a fresh session of the same configuration."""
    sess = uv.decode_session(slots, max_prompt=max_prompt, max_new=max_new, use_graph=use_graph, sampled=sampled)
    if sampled:
        (s,) = sess.admit([row], [cap], sampling=[samp])
    else:
        (s,) = sess.admit([row], [cap])
    codes = _drain(sess, [s])[s]
    sess.close()
    return codes


def _seeded(samp, seed):
    return samp if samp["sampler"] == "greedy" else dict(samp, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# admission with takes

@pytest.mark.parametrize("slots", [4, 16])
@pytest.mark.parametrize("kv,mode,use_graph", [("f32", _lib.GEMM_BF16X3, True), ("f32", _lib.GEMM_BF16X3, False),
                                               ("bf16", _lib.GEMM_F32, True), ("bf16", _lib.GEMM_BF16X3, True),
                                               ("bf16", _lib.GEMM_BF16X3, False), ("fp8", _lib.GEMM_BF16X3, True)])
def test_admit_takes_equals_single_admissions(device, kv, mode, use_graph, slots):
    """takes in {1, 2, 3} and one count that fills the session, prompt widths 5 and 12, caps up to 24, mixed samplers per take (hf,
    accel, a greedy take beside sampled ones), slots that are neither adjacent nor in order, other requests admitted and retired
    around the admission."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/takes/admit", kv_format=kv, stop_bias=1.0)
    rows = _rows(uv, cfg, "t/takes/admit", [5, 12, 5, 12])
    mp, mx = max(r.shape[0] for r in rows), 24
    try:
        _lib.set_gemm_mode(mode)
        sess = uv.decode_session(slots, max_prompt=mp, max_new=mx, use_graph=use_graph, sampled=True)
        expect = {}      # slot -> (row index, cap, sampler), filled at each admission, checked and emptied when the slot is taken

        def admit(idx, takes, caps, samps, where):
            ids = sess.admit([rows[i] for i in idx], caps, sampling=samps, takes=takes, slots=where)
            flat = [s for group in ids for s in group]
            assert flat == list(where) and [len(g) for g in ids] == list(takes)
            for b, group in enumerate(ids):
                for j, s in enumerate(group):
                    expect[s] = (idx[b], caps[b][j], samps[b][j])
            return ids

        # a bystander first, in the middle of the session, two steps ahead of the admission
        (f,) = sess.admit([rows[3]], [9], sampling=[_seeded(HF2, 5)], slots=[1])
        expect[f] = (3, 9, _seeded(HF2, 5))
        sess.step(2)
        if slots == 4:      # one request whose three takes fill the session: slots out of order around the bystander
            admit([0], [3], [[24, 11, 17]], [[_seeded(HF, 11), GREEDY, _seeded(ACCEL, 12)]], [3, 0, 2])
        else:
            admit([0, 1, 2], [2, 3, 1], [[24, 13], [7, 24, 16], [10]],
                  [[_seeded(HF, 11), _seeded(HF, 12)], [_seeded(ACCEL, 13), GREEDY, _seeded(HF2, 14)], [_seeded(HF, 15)]],
                  [15, 3, 7, 0, 9, 4])
        got = _drain(sess, list(expect))
        assert sess.free_slots == list(range(slots))
        # a second round into the retired slots: takes = 1 beside takes = 2 (slots 4), or one request on every slot (slots 16)
        first = dict(expect)
        expect.clear()
        if slots == 4:
            admit([1, 0], [1, 2], [[12], [9, 20]], [[_seeded(HF, 21)], [_seeded(HF2, 22), _seeded(ACCEL, 23)]], [2, 3, 1])
        else:
            order = [int(x) for x in np.random.default_rng(3).permutation(slots)]
            admit([1], [slots], [[6 + (j % 5) for j in range(slots)]],
                  [[_seeded((HF, ACCEL, HF2, GREEDY)[j % 4], 100 + j) for j in range(slots)]], order)
        got2 = _drain(sess, list(expect))
        sess.close()
        for res, exp in ((got, first), (got2, expect)):
            for s, (i, cap, samp) in exp.items():
                ref = _alone(uv, rows[i], cap, samp, slots, mp, mx, use_graph)
                assert np.array_equal(res[s], ref), (s, i, cap, samp, res[s][:12], ref[:12])
        sampled = [res[s] for res, exp in ((got, first),) for s, (i, cap, samp) in exp.items() if i == 0 and samp["sampler"] != "greedy"]
        assert len({tuple(c[:6]) for c in sampled}) > 1, "every sampled take of one prompt drew the same codes: the test shows nothing"
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_admit_takes_on_a_greedy_session_and_refusals(device):
    """A greedy session admits takes (all equal: the plain greedy row); bad calls are refused before anything changes."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/takes/greedy", stop_bias=1.0)
    rows = _rows(uv, cfg, "t/takes/greedy", [5, 12])
    mp = max(r.shape[0] for r in rows)
    sess = uv.decode_session(4, max_prompt=mp, max_new=16)
    with pytest.raises(ValueError, match="sampled=True"):
        sess.admit([rows[0]], [8], sampling=[HF], takes=2)
    with pytest.raises(RuntimeError, match="free slots"):
        sess.admit(rows, [8, 8], takes=[2, 3])
    with pytest.raises(ValueError, match="takes"):
        sess.admit(rows, [8, 8], takes=[2, 0])
    with pytest.raises(ValueError, match="distinct free slots"):
        sess.admit([rows[0]], [8], takes=2, slots=[1, 1])
    lib = _lib.load()
    emb = torch.zeros(1, mp, cfg.model_dim, device=device)
    emb[0, : rows[0].shape[0]] = rows[0]

    def raw(takes, ids, caps):
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in ([rows[0].shape[0]], takes, ids, caps)]
        torch.cuda.synchronize()
        rc = lib.idxtts_gpt_session_admit_takes(uv._h, 1, _lib.ptr(emb), mp, *(x.ctypes.data_as(ctypes.c_void_p) for x in a),
                                                ctypes.c_void_p(0), _lib.ptr(sess._ws), sess._sp())
        sess.stream.synchronize()
        return rc

    assert raw([2], [0, 0], [8, 8]) != 0 and raw([2], [0, 4], [8, 8]) != 0 and raw([0], [0], [8]) != 0      # repeated, out of range, none
    assert raw([5], [0, 1, 2, 3, 0], [8] * 5) != 0 and raw([2], [0, 1], [8, 17]) != 0                      # too many, cap beyond the session's
    assert sess.free_slots == [0, 1, 2, 3]
    ((a, b, c),) = sess.admit([rows[0]], [[16, 16, 5]], takes=3, slots=[2, 0, 3])
    got = _drain(sess, [a, b, c])
    sess.close()
    ref = _alone(uv, rows[0], 16, None, 4, mp, 16, sampled=False)
    assert np.array_equal(got[a], ref) and np.array_equal(got[b], ref) and np.array_equal(got[c], ref[:5])


# ---------------------------------------------------------------------------------------------------------------------------------
# fork

def _noise(seed, cap, V, device):
    return torch.empty(cap, V).exponential_(1, generator=torch.Generator().manual_seed(seed)).to(device)


def _splice(src, k, seed, cap=None):
    """Draws that equal the source's below step k and are new from k on (cap rows: a take may run longer than its source)."""
    cap = src.shape[0] if cap is None else cap
    out = _noise(seed, cap, src.shape[1], src.device)
    out[: min(k, src.shape[0], cap)] = src[: min(k, src.shape[0], cap)]
    return out


@pytest.mark.parametrize("kv,use_graph", [("f32", True), ("f32", False), ("bf16", True), ("fp8", True)])
def test_fork_equals_fresh_admission_with_spliced_draws(device, kv, use_graph):
    """Source just admitted (1 code), after 2 and after 7 codes (k = 7); at in {0, 1, k - 1, k}; n in {1, 3, every free slot}; two
    prompt lengths 7 apart, so that the copied position counts P + max(at, 1) (and P + 1 + at) take every residue mod 4 -- the fp8
    scale runs end on every dword of a 16-byte vector.  A take that is parked and resumed still matches; the source and the bystander
    equal their uninterrupted runs."""
    cfg = GPTConfig.tiny()
    uv, _ = _model(device, cfg, "t/takes/fork", kv_format=kv, stop_bias=-30.0)      # rows run to their caps: the steps below are exact
    V = cfg.number_mel_codes
    rows = _rows(uv, cfg, "t/takes/fork", [5, 12])
    P = [r.shape[0] for r in rows]
    assert {(p + 1 + at) % 4 for p in P for at in (0, 1, 6, 7)} == {0, 1, 2, 3}
    assert {(p + max(at, 1)) % 4 for p in P for at in (0, 1, 6, 7)} == {0, 1, 2, 3}
    slots, mp, cap = 16, max(P), 20
    sess = uv.decode_session(slots, max_prompt=mp, max_new=cap, use_graph=use_graph, sampled=True)
    E = [_noise(40 + i, cap, V, device) for i in range(2)]
    base = [dict(HF, exp_noise=E[0]), dict(ACCEL, exp_noise=E[1])]
    src = sess.admit(rows, [cap, cap], sampling=base, slots=[5, 2])
    expect = {src[0]: (0, cap, base[0]), src[1]: (1, cap, base[1])}      # slot -> (row, cap, sampler) of the fresh admission it must equal
    seed = [1000]

    def fork(i, at, k, n=1, caps=None, where=None, samp=None):
        """n takes of source i, forked at `at` (None: where it stands, k codes); records what each must equal.  A take that keeps
        codes of its source has the source's sampler (the fresh admission draws the prefix with it); one forked at 0 may have any."""
        cut = k if at is None else at
        samp = (HF, ACCEL)[i] if samp is None else samp
        assert cut == 0 or samp is (HF, ACCEL)[i]
        samplers = []
        for j in range(n):
            seed[0] += 1
            c = cap if caps is None else caps[j]
            samplers.append(dict(samp, exp_noise=_splice(E[i], cut, seed[0], c)))
        ids = sess.fork(src[i], samplers, at=at, caps=caps, slots=where)
        assert len(ids) == n and (where is None or ids == list(where))
        for j, s in enumerate(ids):
            expect[s] = (i, cap if caps is None else caps[j], samplers[j])
        return ids

    fork(0, 0, 1, where=[9], samp=ACCEL)            # just admitted: the first token redrawn ...
    fork(0, None, 1, n=3, where=[15, 0, 7])         # ... and kept, three takes in scattered slots
    fork(1, 1, 1, caps=[11])                        # the other prompt length, its own cap
    sess.step(1)                                    # 2 codes
    (t1,) = fork(0, 1, 2)
    fork(1, 2, 2)
    sess.step(5)                                    # 7 codes
    fork(0, 6, 7)
    (t7,) = fork(0, 7, 7)
    fork(1, 0, 7, samp=HF2)
    fork(1, 6, 7, caps=[20])
    parked = sess.park(t7)                          # a take steps aside and comes back into another slot
    sess.step(2)
    free = sess.free_slots
    back = sess.resume(parked, slot=free[-1])
    expect[back] = expect.pop(t7)
    free = sess.free_slots                          # 9 codes; every slot that is left
    assert len(free) >= 2
    fork(1, None, 9, n=len(free), where=free[::-1])
    assert sess.free_slots == []
    got = _drain(sess, list(expect))
    sess.close()
    assert len(expect) == slots
    for s, (i, c, samp) in expect.items():
        ref = _alone(uv, rows[i], c, samp, slots, mp, cap, use_graph)
        assert np.array_equal(got[s], ref), (s, i, c, got[s], ref)
    assert not np.array_equal(got[t1][:cap], got[src[0]][:cap]), "a take equals its source after the fork: the test shows nothing"
    assert np.array_equal(got[t1][:1], got[src[0]][:1])


def test_fork_of_an_ended_source_and_seeded_takes(device):
    """A source that has ended and is not read yet: at its cap (a take with a larger cap of its own runs on where the source had to
    stop) and on the stop token (nothing follows a stop token: at <= the codes in front of it).  Seeded takes draw their own stream
    from step k on: equal to a fresh admission with that seed wherever the first k codes agree -- here by forking a greedy prefix."""
    cfg = GPTConfig.tiny()
    V = cfg.number_mel_codes
    uv, _ = _model(device, cfg, "t/takes/ended", stop_bias=-30.0)
    (row,) = _rows(uv, cfg, "t/takes/ended", [6])
    mp, mx = row.shape[0], 16
    sess = uv.decode_session(4, max_prompt=mp, max_new=mx, sampled=True)
    E = _noise(7, 8, V, device)
    (s,) = sess.admit([row], [8], sampling=[dict(HF, exp_noise=E)])
    assert sess.step(10) == [s]                                      # ended at its cap of 8, not read
    with pytest.raises(RuntimeError, match="cap"):
        sess.fork(s, [dict(HF, exp_noise=_splice(E, 8, 1))])         # at = 8 with the source's cap of 8: nothing left to produce
    a = dict(HF, exp_noise=_splice(E, 8, 2, 16))
    b = dict(HF, exp_noise=_splice(E, 7, 3))
    (ta,) = sess.fork(s, [a], caps=[16])                             # at = k = 8
    (tb,) = sess.fork(s, [b], at=7)                                  # at = k - 1, the source's cap
    got = _drain(sess, [ta, tb, s])
    sess.close()
    assert np.array_equal(got[s], _alone(uv, row, 8, dict(HF, exp_noise=E), 4, mp, mx))
    assert np.array_equal(got[ta], _alone(uv, row, 16, a, 4, mp, mx)) and len(got[ta]) == 16 and np.array_equal(got[ta][:8], got[s])
    assert np.array_equal(got[tb], _alone(uv, row, 8, b, 4, mp, mx)) and np.array_equal(got[tb][:7], got[s][:7])

    # ended on the stop token
    uv2, _ = _model(device, cfg, "t/takes/ended", stop_bias=3.0)
    for seed in range(9, 25):      # draws under which the source stops by itself after a few codes
        E = _noise(seed, mx, V, device)
        full = _alone(uv2, row, mx, dict(HF, exp_noise=E), 4, mp, mx)
        k = len(full)
        if 3 <= k < mx and full[-1] == cfg.stop_mel_token:
            break
    else:
        pytest.fail("no draws under which the source stops by itself after a few codes")
    sess = uv2.decode_session(4, max_prompt=mp, max_new=mx, sampled=True)
    (s,) = sess.admit([row], [mx], sampling=[dict(HF, exp_noise=E)])
    while s not in sess._done:
        sess.step(2)
    with pytest.raises(RuntimeError, match="at out of range"):
        sess.fork(s, [dict(HF, exp_noise=_splice(E, k, 4))], at=k)
    c = dict(HF, exp_noise=_splice(E, k - 1, 5))
    (tc,) = sess.fork(s, [c])                                        # default: the codes in front of the stop token
    got = _drain(sess, [tc, s])
    assert np.array_equal(got[s], full)
    assert np.array_equal(got[tc], _alone(uv2, row, mx, c, 4, mp, mx)) and np.array_equal(got[tc][: k - 1], full[: k - 1])
    sess.close()

    # seeds: a greedy source, seeded takes from k on == a session that decodes greedily to k, whose row is then given the seed; the
    # stream is keyed by (seed, step), so the same take forked at k from two sources with equal prefixes draws equal codes
    sess = uv.decode_session(4, max_prompt=mp, max_new=mx, sampled=True)
    s1, s2 = sess.admit([row, row], [mx, mx], sampling=[GREEDY, GREEDY])
    sess.step(4)
    (u1,) = sess.fork(s1, [dict(HF, seed=77)])
    sess.step(3)
    (u2,) = sess.fork(s2, [dict(HF, seed=77)], at=5)
    got = _drain(sess, [s1, s2, u1, u2])
    sess.close()
    assert np.array_equal(got[s1], got[s2]) and np.array_equal(got[u1], got[u2])
    assert np.array_equal(got[u1][:5], got[s1][:5]) and not np.array_equal(got[u1], got[s1])


def test_fork_refusals_change_nothing(device):
    cfg = GPTConfig.tiny()
    V = cfg.number_mel_codes
    uv, _ = _model(device, cfg, "t/takes/refuse", stop_bias=-30.0)
    rows = _rows(uv, cfg, "t/takes/refuse", [5, 12])
    mp, mx = max(r.shape[0] for r in rows), 12
    sess = uv.decode_session(4, max_prompt=mp, max_new=mx, sampled=True)
    E = [_noise(60 + i, mx, V, device) for i in range(2)]
    samp = [dict(HF, exp_noise=E[0]), dict(HF2, exp_noise=E[1])]
    a, b = sess.admit(rows, [mx, mx], sampling=samp, slots=[0, 2])
    sess.step(3)                                                     # 4 codes each
    lib = _lib.load()

    def raw(s, src, at, dst, caps=None, samplers=None):
        ids = np.ascontiguousarray(dst, dtype=np.int32)
        hc = np.ascontiguousarray(caps, dtype=np.int32) if caps is not None else None
        arr = (_lib.SamplingC * len(dst))(*samplers) if samplers else None
        torch.cuda.synchronize()
        rc = lib.idxtts_gpt_session_fork(uv._h, src, at, len(dst), ids.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.cast(arr, ctypes.c_void_p) if arr is not None else ctypes.c_void_p(0),
                                         hc.ctypes.data_as(ctypes.c_void_p) if hc is not None else ctypes.c_void_p(0), _lib.ptr(s._ws), s._sp())
        s.stream.synchronize()
        return rc

    assert raw(sess, 1, 1, [3]) != 0                                 # a free source
    assert raw(sess, 4, 1, [3]) != 0 and raw(sess, -1, 1, [3]) != 0  # a source out of range
    assert raw(sess, a, 5, [3]) != 0 and raw(sess, a, -2, [3]) != 0  # at beyond the source's 4 codes, at below 0
    assert raw(sess, a, 2, [b]) != 0                                 # a busy destination
    assert raw(sess, a, 2, [1, 1]) != 0                              # a repeated one
    assert raw(sess, a, 2, [4]) != 0 and raw(sess, a, 2, [-1]) != 0  # out of range
    assert raw(sess, a, 2, [a]) != 0                                 # the source itself
    assert raw(sess, a, 2, [1], caps=[mx + 1]) != 0                  # a cap beyond the session's
    assert raw(sess, a, 2, [1], caps=[2]) != 0                       # a cap that leaves the take nothing to produce
    bad = _lib.SamplingC(mode=1, temperature=0.0, top_k=30, top_p=0.8, exp_noise=None, seed=1)
    assert raw(sess, a, 2, [1], samplers=[bad]) != 0                 # a bad sampler
    with pytest.raises(ValueError, match="holds no request"):
        sess.fork(1, [HF])
    with pytest.raises(ValueError, match="distinct free slots"):
        sess.fork(a, [HF], slots=[b])
    assert sess.free_slots == [1, 3]
    gs = uv.decode_session(4, max_prompt=mp, max_new=mx)              # a sampled take on a greedy session
    (g,) = gs.admit([rows[0]], [mx])
    with pytest.raises(ValueError, match="sampled=True"):
        gs.fork(g, [HF])
    good = _lib.SamplingC(mode=1, temperature=0.8, top_k=30, top_p=0.8, exp_noise=None, seed=1)
    assert raw(gs, g, 1, [1], samplers=[good]) != 0
    assert gs.free_slots == [1, 2, 3]
    (g2,) = gs.fork(g, n=1)                                          # greedy takes are allowed there: equal to their source
    gg = _drain(gs, [g, g2])
    gs.close()
    assert np.array_equal(gg[g], gg[g2])
    bs = uv.beam_session(4, 2, max_prompt=mp, max_new=mx)             # a beam session
    (grp,) = bs.admit([rows[0]], [mx], beam=dict(do_sample=False))
    assert raw(bs, 0, 1, [2]) != 0
    bs.evict([grp])
    bs.close()
    # everything in flight still equals its uninterrupted run, and the slots the refused calls named are usable
    (t,) = sess.fork(a, [dict(HF, exp_noise=_splice(E[0], 4, 9))], slots=[3])
    got = _drain(sess, [a, b, t])
    sess.close()
    for s, i, sp in ((a, 0, samp[0]), (b, 1, samp[1]), (t, 0, dict(HF, exp_noise=_splice(E[0], 4, 9)))):
        assert np.array_equal(got[s], _alone(uv, rows[i], mx, sp, 4, mp, mx)), s


# ---------------------------------------------------------------------------------------------------------------------------------
# static path

@pytest.mark.parametrize("kv,invariant", [("f32", False), ("f32", True), ("fp8", False), ("bf16", False), ("bf16", True)])
def test_generate_num_return_sequences(device, kv, invariant):
    """generate(num_return_sequences=3) prefills the B prompts once and fans their keys and values out to B * 3 decode rows; the plain
    call on the caller-expanded batch prefills B * 3 rows.  The two are equal bit for bit with an fp32 (and fp8) cache, with the
    batch-invariant mode on, and with a bf16 cache in split-bf16 mode here, where both prefills (B * (P + 1) and 3 B * (P + 1) rows)
    stay under 256 rows and so run the same GEMM; with the fp32 cache the tokens also equal the CPU oracle's sampling loop on the
    expanded inputs with the same draws.  Row 1 is left-padded."""
    from oracle import gpt as og
    cfg = GPTConfig.tiny()
    uv, w = _model(device, cfg, "t/takes/static", kv_format=kv, stop_bias=2.0)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    B, n, L, NEW, V = 2, 3, 9, 12, cfg.number_mel_codes
    conds = torch.from_numpy(synth.uniform("t/takes/static/conds", (B, cfg.cond_latents + 2, cfg.model_dim), 0.5))
    text = torch.from_numpy(synth.integers("t/takes/static/text", (B, L), 2, cfg.number_text_tokens))
    text[1, 6:] = cfg.stop_text_token      # a ragged batch: row 1 is left-padded
    noise = torch.empty(NEW, B * n, V).exponential_(1, generator=torch.Generator().manual_seed(8))
    try:
        uv.set_batch_invariant(invariant)
        ids, emb, mask = uv.prepare_gpt_inputs(conds.to(device), text)
        assert B * n * ids.shape[1] < 256 and (mask[1] == 0).any()
        kw = dict(max_new_tokens=NEW, do_sample=True, temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=10.0)
        exp_kw = dict(attention_mask=mask.repeat_interleave(n, 0), tts_embeddings=emb.repeat_interleave(n, 0))
        for use_graph in (True, False):
            out = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, exp_noise=noise, num_return_sequences=n, use_graph=use_graph, **kw)
            exp = uv.generate(ids.repeat_interleave(n, 0), exp_noise=noise, use_graph=use_graph, **exp_kw, **kw)
            assert out.shape[0] == B * n and torch.equal(out, exp)
        seeded = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, seed=5, num_return_sequences=n, **kw)
        assert torch.equal(seeded, uv.generate(ids.repeat_interleave(n, 0), seed=5, **exp_kw, **kw))
        greedy = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, max_new_tokens=NEW, num_return_sequences=n)
        assert torch.equal(greedy, uv.generate(ids.repeat_interleave(n, 0), max_new_tokens=NEW, **exp_kw))
        lg = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, exp_noise=noise, num_return_sequences=n, return_logits=True, **kw)
        lge = uv.generate(ids.repeat_interleave(n, 0), exp_noise=noise, return_logits=True, **exp_kw, **kw)
        assert torch.equal(lg[0], lge[0]) and torch.equal(lg[1], lge[1])
        one = uv.generate(ids, attention_mask=mask, tts_embeddings=emb, exp_noise=noise[:, :B].contiguous(), num_return_sequences=1, **kw)
        assert torch.equal(one, uv.generate(ids, attention_mask=mask, tts_embeddings=emb, exp_noise=noise[:, :B].contiguous(), **kw))
    finally:
        uv.set_batch_invariant(False)
    got = out[:, ids.shape[1]:].cpu().numpy()
    assert any(not np.array_equal(got[0], got[j]) for j in range(1, n)), "the takes of one prompt are all equal: the test shows nothing"
    if kv != "f32":
        return
    with torch.no_grad():
        ref = og.generate_sample(tw, cfg, conds.repeat_interleave(n, 0), text.repeat_interleave(n, 0), NEW, noise, 10.0, 0.8, 30, 0.8)
    ref = ref.numpy()
    m = min(got.shape[1], ref.shape[1])      # (either side may have cut the columns in which every row is stop-padded)
    assert np.array_equal(got[:, :m], ref[:, :m]) and (got[:, m:] == cfg.stop_mel_token).all() and (ref[:, m:] == cfg.stop_mel_token).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# n-best

@pytest.fixture(scope="module")
def nbest_ref(golden_dir):
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    t = np.load(os.path.join(golden_dir, "takes_ref.npz"))
    cfg = GPTConfig.tiny()
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    w.update(weights.synth_gpt_cond_weights(cfg, tag="golden/gptref"))
    return g, t, cfg, w


def _score_bound(cfg, row, stopped):
    """A hypothesis' score here (length_penalty 0) is the sum of its tokens' processed log-probabilities, the stop token's included
    when it ended on one.
    The logits agree with the reference's to 5e-4 (tests/test_gpt_ref_gpu.py holds the decode step to that against this golden's
    source), a log-softmax moves by at most twice its inputs' error: 1e-3 per token -- ten times that for a token that had been seen
    before, whose negative log-probability the repetition penalty of 10 multiplies (and temperature >= 1 only shrinks it)."""
    seen, bound = {1, cfg.start_mel_token}, 0.0
    for t in list(row) + ([cfg.stop_mel_token] if stopped else []):
        bound += 1e-3 * (10.0 if int(t) in seen else 1.0)
        seen.add(int(t))
    return bound


@pytest.mark.parametrize("nb", [2, 3, 8])
@pytest.mark.parametrize("mode", ["det", "sample"])
def test_generate_beam_nbest_vs_reference(nbest_ref, device, nb, mode):
    from indextts_amd.gpt import UnifiedVoice
    g, t, cfg, w = nbest_ref
    wb = dict(w)
    wb["mel_head.bias"] = w["mel_head.bias"].copy()
    wb["mel_head.bias"][cfg.stop_mel_token] += float(t[f"nb{nb}_stop_bias"])
    uv = UnifiedVoice(wb, cfg, device=device)
    noise = torch.from_numpy(t[f"nb{nb}_noise"])
    temperature, top_k, top_p = (float(x) for x in t[f"nb{nb}_warpers"])
    conds = uv.conds_latent(torch.from_numpy(g["cond_latent"]).to(device).expand(3, -1, -1), torch.from_numpy(g["emovec_merged"]).to(device).expand(3, -1))
    ids, emb, mask = uv.prepare_gpt_inputs(conds, torch.from_numpy(g["text"]))
    kw = dict(num_beams=nb, do_sample=(mode == "sample"), temperature=temperature, top_k=int(top_k), top_p=top_p, repetition_penalty=10.0,
              length_penalty=0.0, exp_noise=noise)
    plain = uv.generate_beam(ids, noise.shape[0], mask, emb, **kw)
    for n in sorted({1, 2, nb}):
        want, want_scores = t[f"nb{nb}_{mode}_n{n}_codes"], t[f"nb{nb}_{mode}_n{n}_scores"]
        seqs, scores = uv.generate_beam(ids, noise.shape[0], mask, emb, num_return_sequences=n, return_scores=True, **kw)
        codes = seqs[:, ids.shape[1]:].cpu().numpy()
        print(f"num_beams {nb} {mode} n {n}: score error {np.abs(scores.cpu().numpy() - want_scores).max():.3g}")
        np.testing.assert_array_equal(codes, want)                      # tokens, lengths (stop padding) and order
        for r in range(codes.shape[0]):
            stopped = bool((want[r] == cfg.stop_mel_token).any())
            hyp = want[r][: int(np.argmax(want[r] == cfg.stop_mel_token))] if stopped else want[r]
            assert abs(float(scores[r]) - float(want_scores[r])) <= _score_bound(cfg, hyp, stopped), (r, float(scores[r]), float(want_scores[r]))
        best = seqs[::n]                                                 # row b * n is bit for bit the n = 1 call's row b
        assert torch.equal(best[:, : plain.shape[1]], plain) and (best[:, plain.shape[1]:] == cfg.stop_mel_token).all()
    with pytest.raises(ValueError, match="num_return_sequences"):
        uv.generate_beam(ids, 4, mask, emb, num_return_sequences=nb + 1, **dict(kw, exp_noise=None))


@pytest.mark.parametrize("nb", [2, 3])
def test_beam_session_take_nbest(nbest_ref, device, nb):
    """BeamDecodeSession.take(n_best=) with other groups in flight: the hypotheses, order and scores of generate_beam's n-best on
    copies of the prompt (the beam session's rule), entry 0 bit for bit what the plain take() returns."""
    from indextts_amd.gpt import UnifiedVoice
    g, t, cfg, w = nbest_ref
    wb = dict(w)
    wb["mel_head.bias"] = w["mel_head.bias"].copy()
    wb["mel_head.bias"][cfg.stop_mel_token] += float(t[f"nb{nb}_stop_bias"])
    uv = UnifiedVoice(wb, cfg, device=device)
    V, G, cap = cfg.number_mel_codes, 3, 16
    conds = uv.conds_latent(torch.from_numpy(g["cond_latent"]).to(device).expand(3, -1, -1), torch.from_numpy(g["emovec_merged"]).to(device).expand(3, -1))
    rows = uv.prompt_rows(conds, torch.from_numpy(g["text"]))
    noise = torch.from_numpy(t[f"nb{nb}_noise"])[:, 0].contiguous().to(device)      # [cap, nb * V]: utterance 0's draws
    beam = dict(do_sample=True, temperature=1.6, top_k=30, top_p=0.97, length_penalty=0.0, exp_noise=noise)
    results = []
    for n_best in (None, nb):
        sess = uv.beam_session(G * nb, nb, max_prompt=max(r.shape[0] for r in rows), max_new=cap, repetition_penalty=10.0)
        (other,) = sess.admit([rows[1]], [cap], beam=dict(do_sample=False, length_penalty=0.0))
        sess.step(2)
        (grp,) = sess.admit([rows[0]], [cap], beam=beam)
        while grp not in sess._done:
            sess.step(3)
        results.append(sess.take(grp) if n_best is None else sess.take(grp, n_best=n_best))
        sess.evict([other]) if other not in sess._done else sess.take(other)
        sess.close()
    plain, lst = results
    assert len(lst) == nb and torch.equal(lst[0][0], plain)
    # the session rule: row 0 of generate_beam on G copies of the prompt, here with its n best
    P = rows[0].shape[0]
    emb = rows[0][None].expand(G, P, -1).contiguous()
    ids = torch.ones(G, P + 1, dtype=torch.long)
    ids[:, -1] = cfg.start_mel_token
    seqs, scores = uv.generate_beam(ids, cap, None, emb, num_beams=nb, do_sample=True, temperature=1.6, top_k=30, top_p=0.97,
                                    repetition_penalty=10.0, length_penalty=0.0, num_return_sequences=nb,
                                    exp_noise=noise[:, None, :].expand(cap, G, nb * V).contiguous())
    stop = cfg.stop_mel_token
    for q, (codes, score) in enumerate(lst):
        ref = seqs[q, P + 1:].cpu().numpy()
        hits = np.nonzero(ref == stop)[0]
        ref = ref[: hits[0] + 1] if len(hits) else ref
        assert np.array_equal(codes.cpu().numpy(), ref) and score == float(scores[q]), q
    assert all(lst[q][1] >= lst[q + 1][1] for q in range(nb - 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# pipelines

def test_continuous_pipeline_takes(device):
    """ContinuousPipeline(allow_sampling=True).submit(takes=3, sampling={"seed": s}, noise_seed=t): the same codes and audio per take
    alone and under load (other requests in the session first; four slots, so the six takes are admitted in parts either way), and
    each take's codes equal to those of a single request that carries that take's seed (entry i * 3 + j of utterance_samplers; the
    single request's audio comes from a latent pass and an acoustic batch of one row, which may choose other kernels than six rows)."""
    import warnings
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import ContinuousPipeline, utterance_noise_seeds
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/takes/pipe/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 2.0
    wg["mel_head.bias"][cfg.gpt.start_mel_token] = -1e4      # a sampled start token is no semantic code
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/takes/pipe/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/takes/pipe/voc"), device=device)
    cond = PromptConditioning.synthetic(cfg, prompt_frames=40, tag="t/takes/pipe/prompt").to(device)
    B, n, L, cap, S, T = 2, 3, 7, 14, 21, 9
    text = torch.from_numpy(synth.integers("t/takes/pipe/text", (B, L), 2, cfg.gpt.number_text_tokens))
    other = torch.from_numpy(synth.integers("t/takes/pipe/other", (1, 11), 2, cfg.gpt.number_text_tokens))
    samp = {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9}
    seen = []                                   # the codes every request went into its latent pass with
    stage = tts.gpt_stage

    def recording(t, c, **kw):
        seen.append(kw["codes"].clone())
        return stage(t, c, **kw)
    tts.gpt_stage = recording

    def nested(res):
        assert len(res) == B and all(len(r) == n for r in res)
        return [w.cpu() for r in res for w in r]
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True) as pipe:
                alone = nested(pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n).result())
            codes_alone = seen.pop()
            assert codes_alone.shape[0] == B * n and not seen
            with ContinuousPipeline(tts, slots=4, poll_steps=2, max_new=24, allow_sampling=True) as pipe:
                pre = [pipe.submit(other, cond, max_mel_tokens=20, sampling=dict(samp, seed=100 + k), noise_seed=k) for k in range(3)]
                fut = pipe.submit(text, cond, max_mel_tokens=cap, sampling=dict(samp, seed=S), noise_seed=T, takes=n)
                loaded = nested(fut.result())
                [f.result() for f in pre]
            (codes_loaded,) = [c for c in seen if c.shape[0] == B * n]
            seen.clear()
            singles, codes_single = [], []
            with ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=24, allow_sampling=True) as pipe:
                for r in range(B * n):
                    g = torch.Generator().manual_seed(S)
                    for _ in range(r):          # utterance_samplers draws the seeds in row order: row r's is the (r + 1)-th draw
                        torch.randint(0, 2 ** 62, (1,), generator=g)
                    (w,) = pipe.submit(text[r // n: r // n + 1], cond, max_mel_tokens=cap, sampling=dict(samp, generator=g),
                                       noise_seed=[utterance_noise_seeds(T, B * n)[r]]).result()
                    singles.append(w.cpu())
                    codes_single.append(seen.pop())
    finally:
        tts.gpt_stage = stage
    stop = cfg.gpt.stop_mel_token
    assert torch.equal(codes_alone, codes_loaded)
    for r in range(B * n):
        assert torch.equal(alone[r], loaded[r]), r
        c = codes_single[r][0]
        assert torch.equal(codes_alone[r, : c.shape[0]], c) and (codes_alone[r, c.shape[0]:] == stop).all(), r
    assert len({tuple(c.tolist()) for c in codes_alone[:n]}) > 1, "the takes of one utterance are all equal: the test shows nothing"


def test_infer_takes(device, tmp_path):
    """IndexTTS2.infer(takes=n): a list of n results (return_audio), or the files stem.takeK.ext; equal to n calls in a row under the
    same generator state; refused with stream_return."""
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, InferenceResult, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/takes/infer/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 4.0
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/takes/infer/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/takes/infer/voc"), device=device)
    cond = PromptConditioning.synthetic(cfg, prompt_frames=11, tag="t/takes/infer/prompt")
    seg = synth.integers("t/takes/infer/seg", (6,), 2, cfg.gpt.number_text_tokens).tolist()
    kw = dict(max_mel_tokens=16, do_sample=True, top_p=0.9, top_k=30, temperature=1.0, num_beams=1)
    torch.manual_seed(3)
    res = tts.infer(cond, seg, None, return_audio=True, return_numpy=True, takes=3, generator=torch.Generator().manual_seed(5), **kw)
    assert len(res) == 3 and all(isinstance(r, InferenceResult) for r in res)
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(5)
    for r in res:
        one = tts.infer(cond, seg, None, return_audio=True, return_numpy=True, generator=g, **kw)
        assert np.array_equal(np.asarray(one.audio), np.asarray(r.audio))
    paths = tts.infer(cond, seg, str(tmp_path / "o.wav"), takes=2, **kw)
    assert [os.path.basename(p) for p in paths] == ["o.take0.wav", "o.take1.wav"] and all(os.path.exists(p) for p in paths)
    with pytest.raises(ValueError, match="takes"):
        tts.infer(cond, seg, None, stream_return=True, takes=2, **kw)


def test_batch_pipeline_takes_shape_and_refusal(device):
    """BatchPipeline.submit(takes=n) over the stand-in TTS of tests/cancel_standins.py: rows i * n + j, result[i][j], B * n noise seeds,
    greedy takes refused."""
    from cancel_standins import WAIT, FakeTTS, cond, text
    from indextts_amd.serving import BatchPipeline, utterance_noise_seeds
    seeds = []

    class SeedTTS(FakeTTS):
        def acoustic_stage(self, st, noise=None, noise_seeds=None):
            seeds.append(list(noise_seeds) if noise_seeds is not None else None)
            return super().acoustic_stage(st, noise=noise, noise_seeds=noise_seeds)
    tts = SeedTTS(device=device)
    sampling = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8}
    with BatchPipeline(tts, decode_lanes=1) as pipe:
        with pytest.raises(ValueError, match="takes"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, takes=2)
        res = pipe.submit(text((3, 1), (4, 2)), cond(), max_mel_tokens=100, sampling=sampling, noise_seed=7, takes=2).result(timeout=WAIT)
    assert [[int(w[0]) // 1000 for w in r] for r in res] == [[1, 1], [2, 2]]
    assert utterance_noise_seeds(7, 4) in seeds
