"""GPU: the per-code log-probability the sampler kernels record (`row_logprob` under `sample_greedy_kernel`, `sample_slots_kernel`,
`sample_warp_kernel` and `sample_slots_warp_kernel`, csrc/decode.hip) against the float64 reference of tests/scores_cases.py, at the
vocabularies where its loops can go wrong: V = 8194 (the last trip of every loop holds two ids) and V = 130 (below one id per thread).

Crafted rows (a zero head weight: the logits are the bias, on the 1/8 grid, so the reference's inputs are exact) and natural rows
(the reference works on the fp32 logits the same call returned); one-shot greedy, teacher-forced, HF and accel sampling, greedy and
sampled decode sessions; 1, 3 and 16 rows; eager and through the replayed graph.  In every case the codes with the scores on equal
the codes with them off, bit for bit.  The bound: scores_cases.bound.  Each test prints the largest error it saw (-s shows it)."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
import scores_cases as sk

pytestmark = pytest.mark.gpu

HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
HF_FULL = {"sampler": "hf", "temperature": 1.0, "top_k": 0, "top_p": 1.0}
ACCEL = {"sampler": "accel", "temperature": 0.8}
GREEDY = {"sampler": "greedy"}
PENALTY = 10.0
_MODELS = {}


def _model(device, key, weights_of, V):
    from indextts_amd.gpt import UnifiedVoice
    if key not in _MODELS:
        _MODELS[key] = UnifiedVoice(weights_of(), sc.config(V), device=device)
    return _MODELS[key]


def _kw(samp, seed):
    if samp["sampler"] == "greedy":
        return {}
    return dict(do_sample=True, sampler=samp["sampler"], temperature=samp["temperature"], top_k=samp.get("top_k", 0),
                top_p=samp.get("top_p", 1.0), seed=seed)


def _inputs(uv, V, B):
    conds, texts = sc.prompts(V, (5,), tag="t/scores/prompt")
    row = uv.prompt_rows(conds[:1].to(uv.device), texts[0])[0]
    P, d = row.shape
    fake = torch.ones(B, P + 1, dtype=torch.long)
    fake[:, -1] = uv.cfg.start_mel_token
    return fake, row[None].expand(B, P, d).contiguous(), row


def _gen(uv, fake, emb, samp, seed, logprobs, logits, graph, forced=None, n=sk.STEPS):
    out = uv.generate(fake, max_new_tokens=n, tts_embeddings=emb, repetition_penalty=PENALTY, return_logits=logits, use_graph=graph,
                      return_logprobs=logprobs, forced_codes=forced, **_kw(samp, seed))
    out = out if isinstance(out, tuple) else (out,)
    res = [out[0][:, fake.shape[1]:].cpu().numpy()]
    res += [o.cpu().numpy() for o in out[1:]]
    return res


class Worst:
    def __init__(self):
        self.err, self.frac, self.n = 0.0, 0.0, 0

    def check(self, lp, ref, what):
        lp, ref = np.asarray(lp, np.float64), np.asarray(ref, np.float64)
        assert np.isfinite(lp).all(), f"{what}: a log-probability is not finite"
        err = np.abs(lp - ref)
        b = sk.bound(ref)
        self.n += err.size
        if err.size:
            self.err = max(self.err, float(err.max()))
            self.frac = max(self.frac, float((err / b).max()))
        assert (err <= b).all(), f"{what}: |lp - ref| = {err.max():.3e} at ref {ref.flat[int(err.argmax())]:.6f}, bound {b.flat[int(err.argmax())]:.3e}"


def _check_rows(codes, lp, logits_of, stop, worst, what):
    """Every row of one call: lp at each step against the reference on that step's logits; exactly 0 on the pad steps behind a stop."""
    for b in range(codes.shape[0]):
        ended = False
        for t in range(codes.shape[1]):
            if ended:
                assert lp[b, t] == 0.0 and codes[b, t] == stop, f"{what} row {b} step {t}: a pad step records {lp[b, t]}"
                continue
            worst.check(lp[b, t], sk.ref_logprob(logits_of(b, t), codes[b, t]), f"{what} row {b} step {t}")
            ended = codes[b, t] == stop


def _session(uv, row, samplings, caps, use_graph, slots=4):
    """One request per sampler, staggered; {index: (codes, lp)}."""
    sess = uv.decode_session(slots, max_prompt=row.shape[0], max_new=max(caps), repetition_penalty=PENALTY, use_graph=use_graph,
                             sampled=True, scores=True)
    ids = sess.admit([row], caps[:1], sampling=samplings[:1])
    sess.step(2)
    ids += sess.admit([row] * (len(caps) - 1), caps[1:], sampling=samplings[1:])
    done, guard = set(), 0
    while len(done) < len(ids):
        done.update(sess.step(4))
        guard += 1
        assert guard < 100
    out = {}
    for i, s in enumerate(ids):
        c, lp = sess.take(s, scores=True)
        out[i] = (c.cpu().numpy(), lp.cpu().numpy())
    sess.close()
    return out


@pytest.mark.parametrize("name", ["equal", "stop_-1e4", "peaked"])
@pytest.mark.parametrize("V", sk.VOCABS)
def test_crafted_rows_every_kernel(device, V, name):
    bias = sk.crafted_rows(V)[name]
    uv = _model(device, ("crafted", V, name), lambda: sc.crafted_weights(bias), V)
    stop = uv.cfg.stop_mel_token
    ref_all = sk.ref_logprobs(bias)
    worst = Worst()
    for B in sk.BATCHES:
        fake, emb, row = _inputs(uv, V, B)
        for samp, seed in ((GREEDY, None), (HF, 31), (HF_FULL, 32), (ACCEL, 33)):
            if samp is HF and name == "equal":
                # thousands of scores tie at the top-k threshold: more survivors than the top-p stage can sort, and which of them it
                # drops follows their arrival order (SW_CAP, csrc/decode.hip) -- the codes of two calls need not agree.  The row is
                # sampled in HF mode without the nucleus (HF_FULL) instead
                continue
            what = f"V={V} {name} B={B} {samp['sampler']}"
            codes, logits, lp = _gen(uv, fake, emb, samp, seed, True, True, False)
            assert np.array_equal(np.ascontiguousarray(logits).view(np.uint32), np.broadcast_to(bias.view(np.uint32), logits.shape)), \
                "harness precondition: with a zero head weight the logits are the bias, bit for bit"
            assert lp.shape == codes.shape and lp.dtype == np.float32
            _check_rows(codes, lp, lambda b, t: bias, stop, worst, what)
            (off,) = _gen(uv, fake, emb, samp, seed, False, False, False)
            assert np.array_equal(off, codes), f"{what}: the codes change when the scores are recorded"
            g_codes, g_lp = _gen(uv, fake, emb, samp, seed, True, False, True)
            assert np.array_equal(g_codes, codes) and np.array_equal(g_lp.view(np.uint32), lp.view(np.uint32)), f"{what}: the replayed graph differs"
            (g_off,) = _gen(uv, fake, emb, samp, seed, False, False, True)
            assert np.array_equal(g_off, codes)
        if name == "equal":
            assert abs(float(lp[0, 0]) - sk.LOG_V[V]) <= sk.bound(sk.LOG_V[V])
        # teacher-forced: the scores describe the row's own argmax (the code written), not the token fed back; row 0 is forced to stop
        # after two steps and pads from there on
        forced = torch.from_numpy(np.random.default_rng(V + B).integers(0, V - 2, (B, sk.STEPS)))
        forced[0, 1] = stop
        codes, logits, lp = _gen(uv, fake, emb, GREEDY, None, True, True, False, forced=forced)
        for b in range(B):
            for t in range(codes.shape[1]):
                if b == 0 and t >= 2:
                    assert lp[b, t] == 0.0 and codes[b, t] == stop
                else:
                    worst.check(lp[b, t], ref_all[codes[b, t]], f"V={V} {name} B={B} forced row {b} step {t}")
        (off,) = _gen(uv, fake, emb, GREEDY, None, False, False, False, forced=forced)
        assert np.array_equal(off, codes)
    # sessions: greedy and sampled rows of a scored session, eager and replayed, against the reference and against each other
    fake, emb, row = _inputs(uv, V, 1)
    samplings = [dict(GREEDY), dict(HF_FULL if name == "equal" else HF, seed=41), dict(ACCEL, seed=42), dict(HF_FULL, seed=43)]
    caps = [sk.STEPS, 9, sk.STEPS, 7]
    runs = [_session(uv, row, samplings, caps, g) for g in (False, True)]
    for i in range(len(caps)):
        codes, lp = runs[0][i]
        assert len(codes) == len(lp) and (len(codes) == caps[i] or codes[-1] == stop)
        worst.check(lp, ref_all[codes], f"V={V} {name} session request {i}")
        assert np.array_equal(runs[1][i][0], codes) and np.array_equal(runs[1][i][1].view(np.uint32), lp.view(np.uint32))
    # the same requests in a session without scores: the same codes
    sess = uv.decode_session(4, max_prompt=row.shape[0], max_new=max(caps), repetition_penalty=PENALTY, sampled=True)
    ids = sess.admit([row] * len(caps), caps, sampling=samplings)
    left = set(ids)
    plain = {}
    while left:
        for s in sess.step(4):
            plain[s] = sess.take(s).cpu().numpy()
            left.discard(s)
    sess.close()
    # (admitted together here, staggered above: the draws are keyed by the request's own step, so the codes are the same)
    for i, s in enumerate(ids):
        assert np.array_equal(plain[s], runs[0][i][0]), f"V={V} {name} session request {i}: the codes change when the scores are recorded"
    print(f"V={V} {name}: {worst.n} values, largest |lp - ref| = {worst.err:.3e}, largest fraction of the bound = {worst.frac:.3f}")
    assert worst.n > 0


@pytest.mark.parametrize("V", sk.VOCABS)
def test_natural_rows_against_the_returned_logits(device, V):
    """lp against float64 log-softmax of the fp32 logits the same call returned; the stop bias lets rows stop inside the call, so pad
    steps occur (rows of one call draw different streams and stop at different steps)."""
    def w():
        w = sc.natural_weights(V)
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][V - 1] += 3.0
        return w
    uv = _model(device, ("natural", V), w, V)
    stop = uv.cfg.stop_mel_token
    worst = Worst()
    pads = 0
    for B in sk.BATCHES:
        fake, emb, row = _inputs(uv, V, B)
        for samp, seed in ((GREEDY, None), (HF, 51), (HF_FULL, 52), (ACCEL, 53)):
            what = f"V={V} natural B={B} {samp['sampler']}"
            codes, logits, lp = _gen(uv, fake, emb, samp, seed, True, True, False, n=24)
            _check_rows(codes, lp, lambda b, t: logits[b, t], stop, worst, what)
            pads += int((lp == 0.0).sum())
            (off,) = _gen(uv, fake, emb, samp, seed, False, False, False, n=24)
            assert np.array_equal(off, codes), f"{what}: the codes change when the scores are recorded"
            g_codes, g_lp = _gen(uv, fake, emb, samp, seed, True, False, True, n=24)
            assert np.array_equal(g_codes, codes) and np.array_equal(g_lp.view(np.uint32), lp.view(np.uint32)), f"{what}: the replayed graph differs"
    print(f"V={V} natural: {worst.n} values, {pads} pad steps, largest |lp - ref| = {worst.err:.3e}, "
          f"largest fraction of the bound = {worst.frac:.3f}")


def test_takes_share_the_prefill_and_score_each_row(device):
    """generate(num_return_sequences=3, return_logprobs=True): the codes of the call without scores, every take's lp against its own
    logits row."""
    V = 8194
    uv = _model(device, ("natural", V), lambda: sc.natural_weights(V), V)
    fake, emb, row = _inputs(uv, V, 2)
    worst = Worst()
    kw = dict(max_new_tokens=10, tts_embeddings=emb, repetition_penalty=PENALTY, num_return_sequences=3, **_kw(HF, 61))
    seq, lp = uv.generate(fake, return_logprobs=True, **kw)
    off = uv.generate(fake, **kw)
    assert torch.equal(seq, off) and lp.shape == (6, seq.shape[1] - fake.shape[1])
    # the caller-expanded batch records the same values (fp32 cache: the two prefills choose the same kernels)
    kw2 = dict(kw, num_return_sequences=1, tts_embeddings=emb.repeat_interleave(3, dim=0))
    seq2, logits2, lp2 = uv.generate(fake.repeat_interleave(3, dim=0), return_logits=True, return_logprobs=True, **kw2)
    assert torch.equal(seq2, seq) and torch.equal(lp2, lp)
    codes = seq[:, fake.shape[1]:].cpu().numpy()
    _check_rows(codes, lp.cpu().numpy(), lambda b, t: logits2[b, t].cpu().numpy(), uv.cfg.stop_mel_token, worst, "takes")
    assert len({tuple(c) for c in codes[:3]}) > 1, "every take drew the same codes: the test shows nothing"
