"""GPU: decode-session rows admitted behind given codes (`IDXTTS_SESSION_PREFIX`, `idxtts_gpt_session_admit_prefix`,
DecodeSession.admit(prefix=)), bit for bit on the tiny synthetic model:
  * an admission whose prefixes are all empty is the admission of before;
  * a prefixed row equals row 0 of generate(input_ids=[fake | prefix], prefix_layout="resume") on `slots` copies of its prompt (draws
    offset by k) -- sessions of 2 and 16 slots, every KV format -- and, in the batch-invariant mode, the B = 1 call from 1, 2 and 16 slots;
  * rows with different k (0 among them, and cap - 1) share an admission, in any slots, and equal the rows admitted alone; takes of a
    prefixed request equal separate prefixed admissions;
  * park + resume and fork (below, at and above k) give the uninterrupted prefixed row; scores follow;
  * an admission larger than the prefill area is split; refusals change nothing."""
import numpy as np
import pytest
import torch

import prefix_cases as pc
from indextts_amd import _lib
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu
TAG = "t/prefix/sess"
CAP = 16


def _setup(device, kv=None, invariant=False):
    cfg = GPTConfig.tiny()
    uv = pc.model(device, cfg, TAG, kv_format=kv)
    if invariant:
        uv.set_batch_invariant(True)
    rows = pc.prompt_rows(uv, cfg, TAG, [5, 12])
    return cfg, uv, rows, max(r.shape[0] for r in rows)


def _session(uv, slots, mp, mx=CAP, **kw):
    kw = dict(dict(sampled=True, scores=True, prefix=True), **kw)
    return uv.decode_session(slots, max_prompt=mp, max_new=mx, repetition_penalty=pc.PENALTY, **kw)


def _full(uv, slots, mp, row, samp, cap=CAP):
    """The uninterrupted row: (codes, lp)."""
    sess = _session(uv, slots, mp, max(cap, CAP))
    (s,) = sess.admit([row], [cap], sampling=[samp])
    out = pc.drain(sess, [s], scores=True)[s]
    sess.close()
    return out


@pytest.mark.parametrize("slots", [2, 16])
@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
def test_prefixed_row_equals_one_shot_row0(device, kv, slots):
    """Contract 2 (and 4: the two rows share the admission, in the last slots).  bf16 cache: the exact GEMM mode, so that the
    reference batch's prefill and the admission's run the same kernels at every row count."""
    cfg, uv, rows, mp = _setup(device, kv)
    row = rows[1]
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32 if kv == "bf16" else _lib.GEMM_BF16X3)
        E = pc.noise(cfg, CAP, 11)
        hf = dict(pc.HF, exp_noise=E)
        fg, fs = _full(uv, slots, mp, row, pc.GREEDY), _full(uv, slots, mp, row, hf)
        assert len(fg[0]) == CAP and len(fs[0]) == CAP
        for k in (1, 6, CAP - 1):
            sess = _session(uv, slots, mp)
            given = np.arange(k, dtype=np.float32) - 3.0
            ids = sess.admit([row, row], [CAP, CAP], sampling=[pc.GREEDY, hf], prefix=[fg[0][:k], fs[0][:k]],
                             prefix_logprobs=[given, None], slots=[slots - 1, slots - 2])
            assert ids == [slots - 1, slots - 2]
            got = pc.drain(sess, ids, scores=True)
            sess.close()
            for s, samp, pre in ((ids[0], pc.GREEDY, fg[0][:k]), (ids[1], hf, fs[0][:k])):
                seq, lp = pc.one_shot_row0(uv, cfg, row, pre, CAP, samp, slots, draws=E, return_logprobs=True)
                want = seq[0, row.shape[0] + 1:].cpu().numpy()
                assert np.array_equal(got[s][0], want), (k, samp["sampler"])
                assert pc.same_bits(got[s][1][k:], lp[0].cpu().numpy())      # the recorded values behind the prefix ...
            assert pc.same_bits(got[ids[0]][1][:k], given) and not got[ids[1]][1][:k].any()      # ... the caller's, or 0, for it
            assert np.array_equal(got[ids[0]][0], fg[0]) and np.array_equal(got[ids[1]][0], fs[0])      # the row went on as it would have
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


@pytest.mark.parametrize("slots", [1, 2, 16])
def test_batch_invariant_prefixed_row_equals_the_b1_call(device, slots):
    cfg, uv, rows, mp = _setup(device, invariant=True)
    row = rows[0]
    E = pc.noise(cfg, CAP, 12)
    hf = dict(pc.HF, exp_noise=E)
    for samp in (pc.GREEDY, hf):
        full = _full(uv, slots, mp, row, samp)
        for k in (1, 7):
            sess = _session(uv, slots, mp)
            (s,) = sess.admit([row], [CAP], sampling=[samp], prefix=[full[0][:k]], slots=[slots - 1])
            got = pc.drain(sess, [s], scores=True)[s]
            sess.close()
            seq, lp = pc.one_shot_row0(uv, cfg, row, full[0][:k], CAP, samp, 1, draws=E, return_logprobs=True)
            assert np.array_equal(got[0], seq[0, row.shape[0] + 1:].cpu().numpy()) and pc.same_bits(got[1][k:], lp[0].cpu().numpy())


def test_empty_prefixes_are_the_admission_of_before(device):
    """Contract 1: prefix=[None, ...] on a session with the flag, against a session without it -- codes and log-probabilities."""
    cfg, uv, rows, mp = _setup(device)
    hf = dict(pc.HF, seed=5)
    out = []
    for prefix in (False, True):
        sess = _session(uv, 4, mp, prefix=prefix)
        kw = dict(prefix=[None, torch.zeros(0, dtype=torch.long)]) if prefix else {}
        ids = sess.admit([rows[0], rows[1]], [CAP, 9], sampling=[hf, pc.GREEDY], takes=[2, 1], **kw)
        flat = [s for g in ids for s in g]
        got = pc.drain(sess, flat, scores=True)
        out.append([got[s] for s in flat])
        sess.close()
    for a, b in zip(*out):
        assert np.array_equal(a[0], b[0]) and pc.same_bits(a[1], b[1])


def test_mixed_admission_takes_neighbours_and_slots(device):
    """Contracts 3 and 4 in a session of 16: rows with k = 5, 0, 9, CAP - 1 and a request with two takes behind k = 2, admitted
    together into scattered slots, against the same rows admitted alone (the takes: two separate prefixed admissions)."""
    cfg, uv, rows, mp = _setup(device)
    A, B = rows[1], rows[0]
    E1, E2, E3 = (pc.noise(cfg, CAP, s) for s in (21, 22, 23))
    hf1, hf2, ac3 = dict(pc.HF, exp_noise=E1), dict(pc.HF, exp_noise=E2), dict(pc.ACCEL, exp_noise=E3)
    fa, fb = _full(uv, 16, mp, A, pc.GREEDY)[0], _full(uv, 16, mp, B, hf1)[0]
    reqs = [(A, fa[:5], [pc.GREEDY]), (B, None, [hf1]), (B, fb[:9], [hf1]), (A, fa[:CAP - 1], [pc.GREEDY]), (A, fa[:2], [hf2, ac3])]
    alone = []
    for row, pre, samps in reqs:
        for samp in samps:
            sess = _session(uv, 16, mp)
            (s,) = sess.admit([row], [CAP], sampling=[samp], prefix=[pre], slots=[7])
            alone.append(pc.drain(sess, [s], scores=True)[s])
            sess.close()
    sess = _session(uv, 16, mp)
    by = sess.admit([rows[1]], [CAP], sampling=[dict(pc.HF, seed=3)])      # a bystander that is already decoding
    sess.step(2)
    ids = sess.admit([r[0] for r in reqs], CAP, sampling=[r[2] for r in reqs], takes=[len(r[2]) for r in reqs], prefix=[r[1] for r in reqs],
                     slots=[15, 2, 9, 4, 11, 1])
    assert ids == [[15], [2], [9], [4], [11, 1]]
    flat = [s for g in ids for s in g]
    got = pc.drain(sess, flat + by, scores=True)
    sess.close()
    for s, want in zip(flat, alone):
        assert np.array_equal(got[s][0], want[0]) and pc.same_bits(got[s][1], want[1])
    assert np.array_equal(got[15][0], fa) and np.array_equal(got[9][0], fb) and np.array_equal(got[4][0], fa)
    assert np.array_equal(got[2][0], fb)      # k = 0 beside prefixed rows: the plain row
    assert not np.array_equal(got[11][0], got[1][0]) and np.array_equal(got[11][0][:2], fa[:2]) and np.array_equal(got[1][0][:2], fa[:2])


@pytest.mark.parametrize("kv", ["f32", "fp8"])
def test_park_resume_and_fork_on_a_prefixed_row(device, kv):
    """Contract 5.  The prefix and its log-probabilities are the uninterrupted row's own, so every row below must return that row:
    codes bit for bit; log-probabilities bit for bit where every later code is computed as the source computed it (park + resume,
    fork above k).  A fork at j <= k computes code k with a decode step where the source computed it in the admission's prefill (and,
    below k, decodes positions j .. k - 1 again instead of reading the prefill's): the source's first j values, then values within
    1e-4 -- the two paths' logits differ by summation order, 1e-6 here."""
    cfg, uv, rows, mp = _setup(device, None if kv == "f32" else kv)
    row, k = rows[1], 6
    E = pc.noise(cfg, CAP, 31)
    for samp in (pc.GREEDY, dict(pc.HF, exp_noise=E)):
        full = _full(uv, 8, mp, row, samp)
        sess, other = _session(uv, 8, mp), _session(uv, 8, mp)
        (s,) = sess.admit([row], [CAP], sampling=[samp], prefix=[full[0][:k]], prefix_logprobs=[full[1][:k]], slots=[1])
        ref = pc.drain(sess, [s], scores=True)[s]      # the uninterrupted prefixed row
        assert np.array_equal(ref[0], full[0]) and pc.same_bits(ref[1][:k], full[1][:k])
        (s,) = sess.admit([row], [CAP], sampling=[samp], prefix=[full[0][:k]], prefix_logprobs=[full[1][:k]], slots=[5])
        sess.step(2)      # k + 3 codes
        f = sess.fork(s, samplers=[samp], at=3, caps=[CAP]) + sess.fork(s, samplers=[samp], at=k, caps=[CAP]) + \
            sess.fork(s, samplers=[samp], at=k + 2, caps=[CAP])
        with pytest.raises(RuntimeError, match="at = 0"):      # x_last is position P + k's: as on a resumed row
            sess.fork(s, samplers=[samp], at=0, caps=[CAP])
        parked = sess.park(s).to("cpu")
        assert s in sess.free_slots
        r = other.resume(parked.to(device), slot=2)
        got = pc.drain(sess, f, scores=True)
        back = pc.drain(other, [r], scores=True)[r]
        sess.close()
        other.close()
        assert np.array_equal(back[0], ref[0]) and pc.same_bits(back[1], ref[1])      # parked, moved to the host and resumed elsewhere
        ref_lp = ref[1]       # the prefixed row's own values: the caller's for [0, k), recorded behind them
        for slot, at in zip(f, (3, k, k + 2)):
            assert np.array_equal(got[slot][0], full[0]), (samp["sampler"], at)
            if at > k:
                assert pc.same_bits(got[slot][1], ref_lp), at
            else:
                assert pc.same_bits(got[slot][1][:at], ref_lp[:at])
                np.testing.assert_allclose(got[slot][1][at:], ref_lp[at:], rtol=0, atol=1e-4)


def test_stop_and_evict_treat_the_row_like_any_other(device):
    cfg, uv, rows, mp = _setup(device)
    full = _full(uv, 4, mp, rows[0], pc.GREEDY)[0]
    sess = _session(uv, 4, mp)
    a, b = sess.admit([rows[0], rows[0]], CAP, prefix=[full[:4], full[:8]])
    sess.stop([a])
    sess.evict([b])
    assert sess.step(0) == [a] and b in sess.free_slots
    assert np.array_equal(sess.take(a).cpu().numpy(), full[:5])      # the prefix and the admission's one new code
    sess.close()


def test_an_admission_above_the_prefill_area_is_split(device):
    """16 requests of P + 1 + 40 positions each against an area of 16 * (max_prompt + 1) + 256: DecodeSession.admit splits them
    into groups that fit; the native call refuses the whole admission with the limit in its message and changes nothing."""
    cfg, uv, rows, mp = _setup(device)
    row, mx, k = rows[1], 48, 40
    full = _full(uv, 16, mp, row, pc.GREEDY, cap=mx)[0]
    assert len(full) == mx
    sess = _session(uv, 16, mp, mx)
    area = sess._prefill_area()
    assert 16 * (row.shape[0] + 1 + k) > area >= mp + 1 + mx + 256
    sess._prefill_area = lambda: 1 << 30      # no splitting: the native limit
    with pytest.raises(RuntimeError, match=f"prefill area of {area} positions"):
        sess.admit([row] * 16, mx, prefix=[full[:k]] * 16)
    assert sess.free_slots == list(range(16))
    del sess._prefill_area
    ids = sess.admit([row] * 16, mx, prefix=[full[:k - i] for i in range(16)])
    assert ids == list(range(16))
    got = pc.drain(sess, ids)
    sess.close()
    for s in ids:
        assert np.array_equal(got[s], full), s


def test_refusals_change_nothing(device):
    cfg, uv, rows, mp = _setup(device)
    row = rows[0]
    full = _full(uv, 4, mp, row, pc.GREEDY)[0]
    plain = uv.decode_session(4, max_prompt=mp, max_new=CAP, repetition_penalty=pc.PENALTY)
    with pytest.raises(ValueError, match="prefix=True"):
        plain.admit([row], CAP, prefix=[full[:3]])
    plain.prefix = True      # past the wrapper's check: the native one names the flag
    with pytest.raises(RuntimeError, match="IDXTTS_SESSION_PREFIX"):
        plain.admit([row], CAP, prefix=[full[:3]])
    plain.prefix = False
    assert plain.free_slots == [0, 1, 2, 3]
    (s,) = plain.admit([row], CAP)
    assert np.array_equal(pc.drain(plain, [s])[s], full)
    plain.close()
    sess = _session(uv, 4, mp, scores=False)
    stop = full[:3].copy()
    stop[1] = cfg.stop_mel_token
    for kw, err, msg in ((dict(prefix=[stop]), ValueError, "stop token"), (dict(prefix=[full[:CAP]]), ValueError, "k < cap"),
                         (dict(prefix=[np.array([cfg.number_mel_codes])]), ValueError, "mel codes"),
                         (dict(prefix=[full[:3], None]), ValueError, "one entry"), (dict(prefix=[full[None, :3]]), ValueError, "1-D"),
                         (dict(prefix=[full[:3]], prefix_logprobs=[np.zeros(3)]), ValueError, "scores=True"),
                         (dict(prefix_logprobs=[np.zeros(3)]), ValueError, "without prefix")):
        with pytest.raises(err, match=msg):
            sess.admit([row], CAP, **kw)
    with pytest.raises(ValueError, match="k < cap"):      # the cap counts prefix + new codes, for every take
        sess.admit([row], [[CAP, 3]], takes=2, prefix=[full[:3]])
    assert sess.free_slots == [0, 1, 2, 3]
    sess.close()
    with pytest.raises(ValueError):
        uv.decode_session(4, max_prompt=mp, max_new=CAP, num_beams=2, prefix=True)
    beam = uv.beam_session(4, 2, max_prompt=mp, max_new=CAP)
    with pytest.raises(NotImplementedError, match="beam session takes no prefix"):
        beam.admit([row], CAP, prefix=[full[:3]])
    assert beam.free_groups == [0, 1]
    beam.close()
