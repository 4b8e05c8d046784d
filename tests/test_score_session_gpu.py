"""GPU: prefix log-probabilities from the admission's own prefill (`IDXTTS_SESSION_PREFIX_SCORES`,
`idxtts_gpt_session_admit_prefix_scored`, DecodeSession.admit(prefix_logprobs=[..., "model", ...])), in the set-up of
tests/test_prefix_session_gpu.py (tiny synthetic model, greedy and HF samplers, f32 and fp8 caches):
  * a row admitted with "model" draws the codes of the row admitted with the caller's values and records the same lp[k:], bit for bit;
    its lp[:k] are the uninterrupted scored row's own values within 1e-4 (that file's tolerance for the same quantity through the
    prefill instead of the steps), and UnifiedVoice.score_codes' values for prompt and prefix;
  * "model", an array and None share one admission; three takes share the computed values; rows admitted before are unchanged;
  * fork, park and resume carry lp[:k], bit for bit;
  * a session without the flag refuses "model" and names the flag; every flag combination that existed keeps its workspace size."""
import numpy as np
import pytest
import torch

import prefix_cases as pc
from indextts_amd import _lib
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu
TAG = "t/prefix/sess"
CAP = 16
LP_TOL = 1e-4


def _setup(device, kv=None, invariant=False):
    cfg = GPTConfig.tiny()
    uv = pc.model(device, cfg, TAG, kv_format=kv)
    if invariant:
        uv.set_batch_invariant(True)
    rows = pc.prompt_rows(uv, cfg, TAG, [5, 12])
    return cfg, uv, rows, max(r.shape[0] for r in rows)


def _session(uv, slots, mp, mx=CAP, **kw):
    kw = dict(dict(sampled=True, scores=True, prefix=True, prefix_scores=True), **kw)
    return uv.decode_session(slots, max_prompt=mp, max_new=mx, repetition_penalty=pc.PENALTY, **kw)


def _full(uv, slots, mp, row, samp, cap=CAP):
    sess = _session(uv, slots, mp, max(cap, CAP))
    (s,) = sess.admit([row], [cap], sampling=[samp])
    out = pc.drain(sess, [s], scores=True)[s]
    sess.close()
    return out


@pytest.mark.parametrize("kv", ["f32", "fp8"])
def test_model_values_beside_the_callers(device, kv):
    cfg, uv, rows, mp = _setup(device, kv)
    row = rows[1]
    E = pc.noise(cfg, CAP, 11)
    hf = dict(pc.HF, exp_noise=E)
    worst = 0.0
    for samp in (pc.GREEDY, hf):
        full = _full(uv, 4, mp, row, samp)
        assert len(full[0]) == CAP
        for k in (1, 6, CAP - 1):
            given = np.arange(k, dtype=np.float32) - 3.0
            got = {}
            for how in ("given", "model"):
                sess = _session(uv, 4, mp)
                (s,) = sess.admit([row], [CAP], sampling=[samp], prefix=[full[0][:k]], prefix_logprobs=[given if how == "given" else "model"],
                                  slots=[2])
                got[how] = pc.drain(sess, [s], scores=True)[s]
                sess.close()
            assert np.array_equal(got["model"][0], got["given"][0]) and np.array_equal(got["model"][0], full[0])
            assert pc.same_bits(got["model"][1][k:], got["given"][1][k:])
            assert pc.same_bits(got["given"][1][:k], given)
            err = float(np.abs(got["model"][1][:k] - full[1][:k]).max())
            worst = max(worst, err)
            assert err <= LP_TOL, (kv, samp["sampler"], k, err)
            direct = uv.score_codes([full[0][:k]], row[None].contiguous())[0].cpu().numpy()
            assert float(np.abs(got["model"][1][:k] - direct).max()) <= LP_TOL
    print(f"{kv}: max |lp[:k] from the admission prefill - the uninterrupted row's| = {worst:.3e} (bound {LP_TOL:.0e})")


def test_mixed_admission_takes_and_bystanders(device):
    cfg, uv, rows, mp = _setup(device)
    A, B = rows[1], rows[0]
    E1, E2, E3 = (pc.noise(cfg, CAP, s) for s in (21, 22, 23))
    hf1, hf2, ac3 = dict(pc.HF, exp_noise=E1), dict(pc.HF, exp_noise=E2), dict(pc.ACCEL, exp_noise=E3)
    fa, fb = _full(uv, 16, mp, A, pc.GREEDY), _full(uv, 16, mp, B, hf1)
    given = np.linspace(-2.0, -1.0, 9).astype(np.float32)
    reqs = [(A, fa[0][:5], "model", [pc.GREEDY]), (B, fb[0][:9], given, [hf1]), (A, fa[0][:3], None, [pc.GREEDY]),
            (A, fa[0][:7], "model", [pc.GREEDY, hf2, ac3])]
    by_seed = dict(pc.HF, seed=3)

    def run(lps):
        sess = _session(uv, 16, mp)
        by = sess.admit([rows[1]], [CAP], sampling=[by_seed])      # a bystander that is already decoding
        sess.step(2)
        ids = sess.admit([r[0] for r in reqs], CAP, sampling=[r[3] for r in reqs], takes=[len(r[3]) for r in reqs], prefix=[r[1] for r in reqs],
                         prefix_logprobs=lps, slots=[15, 2, 9, 4, 11, 1])
        got = pc.drain(sess, [s for g in ids for s in g] + by, scores=True)
        sess.close()
        return ids, by, got

    ids, by, got = run([r[2] for r in reqs])
    _, by0, plain = run([None if isinstance(r[2], str) else r[2] for r in reqs])      # the admission of before: no request asks the model
    assert ids == [[15], [2], [9], [4, 11, 1]]
    for g in ids:
        for s in g:
            assert np.array_equal(got[s][0], plain[s][0]), s      # the codes do not depend on where lp[:k] comes from
    assert pc.same_bits(got[by[0]][1], plain[by0[0]][1]) and np.array_equal(got[by[0]][0], plain[by0[0]][0])      # the bystander: unchanged
    assert float(np.abs(got[15][1][:5] - fa[1][:5]).max()) <= LP_TOL and pc.same_bits(got[15][1][5:], plain[15][1][5:])
    assert pc.same_bits(got[2][1][:9], given) and pc.same_bits(got[2][1], plain[2][1])
    assert not got[9][1][:3].any() and pc.same_bits(got[9][1], plain[9][1])
    for s in (4, 11, 1):      # three takes share the computed prefix values
        assert pc.same_bits(got[s][1][:7], got[4][1][:7]) and pc.same_bits(got[s][1][7:], plain[s][1][7:])
    assert float(np.abs(got[4][1][:7] - fa[1][:7]).max()) <= LP_TOL and got[4][1][:7].all()
    assert len({tuple(got[s][0]) for s in (4, 11, 1)}) > 1


def test_fork_park_resume_carry_the_values(device):
    cfg, uv, rows, mp = _setup(device)
    row = rows[1]
    full = _full(uv, 4, mp, row, pc.GREEDY)
    k = 6
    sess = _session(uv, 4, mp)
    (s,) = sess.admit([row], [CAP], sampling=[pc.GREEDY], prefix=[full[0][:k]], prefix_logprobs=["model"], slots=[0])
    plain = pc.drain(sess, [s], scores=True)[s]      # the prefixed row left alone
    (s,) = sess.admit([row], [CAP], sampling=[pc.GREEDY], prefix=[full[0][:k]], prefix_logprobs=["model"], slots=[0])
    sess.step(3)
    (f,) = sess.fork(s, samplers=[pc.GREEDY], at=k + 1, slots=[3])
    parked = sess.park(s)
    r = sess.resume(parked, slot=1)
    got = pc.drain(sess, [f, r], scores=True)
    sess.close()
    assert np.array_equal(got[r][0], full[0]) and np.array_equal(got[f][0], full[0])
    assert got[r][1][:k].all() and float(np.abs(got[r][1][:k] - full[1][:k]).max()) <= LP_TOL
    assert pc.same_bits(got[f][1][:k], got[r][1][:k])
    assert pc.same_bits(got[r][1], plain[1]) and pc.same_bits(got[f][1], plain[1])


def test_batch_invariant_values_equal_score_codes(device):
    """In the batch-invariant mode the admission's values are score_codes' on the same prompt and prefix, bit for bit, whatever else
    is admitted with the row."""
    cfg, uv, rows, mp = _setup(device, invariant=True)
    row = rows[0]
    full = _full(uv, 4, mp, row, pc.GREEDY)
    k = 9
    direct = uv.score_codes([full[0][:k]], row[None].contiguous())[0].cpu().numpy()
    sess = _session(uv, 4, mp)
    ids = sess.admit([rows[1], row], [CAP, CAP], sampling=[pc.GREEDY, pc.GREEDY], prefix=[full[0][:2], full[0][:k]],
                     prefix_logprobs=["model", "model"])
    got = pc.drain(sess, ids, scores=True)
    sess.close()
    assert pc.same_bits(got[ids[1]][1][:k], direct)


def test_refusals_and_workspace_sizes(device):
    cfg, uv, rows, mp = _setup(device)
    row = rows[0]
    pre = np.array([3, 4, 5])
    sess = _session(uv, 2, mp, prefix_scores=False)
    with pytest.raises(ValueError, match="prefix_scores=True"):
        sess.admit([row], [CAP], prefix=[pre], prefix_logprobs=["model"])
    with pytest.raises(ValueError, match='"model"'):
        sess.admit([row], [CAP], prefix=[pre], prefix_logprobs=["other"])
    # the native entry on a session without the flag: refused, the flag named, nothing changed
    lib = _lib.load()
    emb = row[None].contiguous()
    i32 = lambda *v: np.asarray(v, np.int32)
    plen, ids, caps, klen, fm = i32(row.shape[0]), i32(0), i32(CAP), i32(3), np.ones(1, np.uint8)
    codes = torch.from_numpy(pre).to(uv.device)
    args = lambda ws: (uv._h, 1, _lib.ptr(emb), row.shape[0], plen.ctypes.data, None, ids.ctypes.data, caps.ctypes.data, None, klen.ctypes.data,
                       _lib.ptr(codes), None, fm.ctypes.data, _lib.ptr(ws), sess._sp())
    with torch.cuda.stream(sess.stream):
        with pytest.raises(RuntimeError, match="IDXTTS_SESSION_PREFIX_SCORES"):
            _lib.check(lib.idxtts_gpt_session_admit_prefix_scored(*args(sess._ws)))
    assert sess.free_slots == [0, 1]
    (s,) = sess.admit([row], [CAP], prefix=[pre])      # the next valid call works
    assert len(pc.drain(sess, [s])[s]) == CAP
    sess.close()
    # a session with the flag refuses what _admit_prefix refuses, before anything changes
    sess = _session(uv, 2, mp)
    with pytest.raises(ValueError, match="stop token"):
        sess.admit([row], [CAP], prefix=[np.array([3, cfg.stop_mel_token])], prefix_logprobs=["model"])
    with torch.cuda.stream(sess.stream):
        with pytest.raises(RuntimeError, match="null prefix_lens or from_model"):
            a = list(args(sess._ws))
            a[12] = None
            _lib.check(lib.idxtts_gpt_session_admit_prefix_scored(*a))
    assert sess.free_slots == [0, 1]
    sess.close()
    with pytest.raises(ValueError, match="prefix=True and scores=True"):
        uv.decode_session(2, max_prompt=mp, max_new=CAP, prefix=True, prefix_scores=True)
    # sizes: the flag is valid only with PREFIX | SCORES, adds bytes behind everything else, and changes no combination that existed
    size = lambda flags: int(lib.idxtts_gpt_session_workspace_bytes_ex(uv._h, 4, mp, CAP, flags))
    P, S, SM, PS = _lib.SESSION_PREFIX, _lib.SESSION_SCORES, _lib.SESSION_SAMPLED, _lib.SESSION_PREFIX_SCORES
    for flags in (PS, PS | P, PS | S, PS | SM, 4, 32):
        assert size(flags) == 0, flags
    assert size(PS | P | S) > size(P | S) and size(PS | P | S | SM) > size(P | S | SM)
    assert size(0) < size(S) < size(S | P) and size(SM) > size(0)
