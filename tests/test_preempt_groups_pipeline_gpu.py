"""GPU: group preemption in a beam ContinuousPipeline on the reduced full pipeline (beam decode sessions -> latent pass -> s2mel ->
vocoder), with real sessions behind a thin gate wrapper.  Two groups of three beams hold the two long utterances of a low-priority
request; a high-priority request arrives while both decode.  One group is parked, the urgent request decodes in its place and
completes, the parked group resumes -- and every waveform is bit-equal to that of the same request submitted alone to the same
pipeline without preempt_groups (seeded beams and noise seeds; exact GEMM mode, so that equal codes give equal audio bit for bit).
The stop token is biased away: groups end at their caps."""
import threading
import warnings

import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu

NB, GROUPS = 3, 2
WAIT = 600
_ALONE = {}


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/gpreempt/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/gpreempt/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/gpreempt/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"t/gpreempt/prompt{k}").to(device) for k in range(2)]
    yield tts, conds
    _ALONE.clear()


class _Gated:
    """A beam session that tells the test when its first step has run and waits there for the go-ahead, and that holds a resume until
    the test has seen the urgent request complete; records park_group, take and resume_group in call order."""

    def __init__(self, sess, stepped, go, urgent_done, log):
        self._sess, self._stepped, self._go, self._urgent_done, self._log = sess, stepped, go, urgent_done, log

    def __getattr__(self, name):
        return getattr(self._sess, name)

    def step(self, n=1):
        out = self._sess.step(n)
        if not self._stepped.is_set():
            self._stepped.set()
            assert self._go.wait(WAIT)
        return out

    def park_group(self, group):
        p = self._sess.park_group(group)
        self._log.append(("park", group, p.n_codes, p.device.type))
        return p

    def resume_group(self, parked, group=None):
        assert self._urgent_done.wait(WAIT)
        self._log.append(("resume", parked.device.type))
        return self._sess.resume_group(parked, group)

    def take(self, i):
        self._log.append(("take", i))
        return self._sess.take(i)


def _pipeline(tts, events, log, **kw):
    from indextts_amd.serving import ContinuousPipeline

    def factory(mp, mn):
        return _Gated(tts.gpt.beam_session(GROUPS * NB, NB, mp, mn, repetition_penalty=10.0), *events, log)
    return ContinuousPipeline(tts, slots=GROUPS * NB, num_beams=NB, poll_steps=2, max_new=16, session_factory=factory, **kw)


def _submit(pipe, r, **kw):
    return pipe.submit(r["text"], r["cond"], max_mel_tokens=r["cap"], sampling=r["sampling"], noise_seed=r["noise_seed"], **kw)


def _alone(tts, k, r):
    """The request by itself on the same pipeline without preempt_groups: computed once per request."""
    if k not in _ALONE:
        events = (threading.Event(), threading.Event(), threading.Event())
        for e in events:
            e.set()
        with _pipeline(tts, events, []) as pipe:
            _ALONE[k] = [w.cpu() for w in _submit(pipe, r).result(timeout=WAIT)]
    return _ALONE[k]


@pytest.mark.parametrize("park_to", ["device", "host"])
def test_urgent_beam_request_preempts_a_group_and_everybody_gets_their_own_audio(setup, park_to):
    tts, conds = setup
    cfg = tts.cfg

    def sampling(k):
        return {"num_beams": NB, "do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0, "seed": 300 + k}
    reqs = [{"text": torch.from_numpy(synth.integers(f"t/gpreempt/text/{k}", (B, L), 2, cfg.gpt.number_text_tokens)), "cond": conds[k],
             "cap": cap, "sampling": sampling(k), "noise_seed": 9000 + k} for k, (B, L, cap) in enumerate([(2, 12, 16), (1, 7, 6)])]
    stepped, go, urgent_done, log = threading.Event(), threading.Event(), threading.Event(), []
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with _pipeline(tts, (stepped, go, urgent_done), log, preempt_groups=True, park_to=park_to) as pipe:
                pipe.trace = []
                low = _submit(pipe, reqs[0])
                assert stepped.wait(WAIT)                            # both of its utterances are decoding, one group each
                urgent = _submit(pipe, reqs[1], priority=5)
                go.set()
                got_urgent = [w.cpu() for w in urgent.result(timeout=WAIT)]
                assert not low.done()                                # one of its groups is parked until the line below
                urgent_done.set()
                got_low = [w.cpu() for w in low.result(timeout=WAIT)]
                trace = list(pipe.trace)
            want_low, want_urgent = _alone(tts, 0, reqs[0]), _alone(tts, 1, reqs[1])
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    # the session saw: the group admitted last parked (group 1, 3 tokens per beam: admission + one poll of 2 steps), the urgent
    # request taken from that group, the resume -- from where park_to says -- and then the two groups of the low request
    where = "cpu" if park_to == "host" else "cuda"
    assert log[:3] == [("park", 1, 3, "cuda"), ("take", 1), ("resume", where)], log
    assert sorted(e[0] for e in log) == ["park", "resume", "take", "take", "take"]
    parks, resumes = [e for e in trace if e[0] == "park"], [e for e in trace if e[0] == "resume"]
    jobs = {e[4]: e for e in trace if e[0] == "acoustic"}
    assert len(parks) >= 1 and parks == [("park", parks[0][1], 0, 1)] and resumes == [("resume", resumes[0][1], 0, 1)]
    assert set(jobs) == {(0,), (1,)}
    assert parks[0][1] < jobs[(1,)][2] < resumes[0][1] < jobs[(0,)][1]                  # the urgent request finished first
    assert [e[0] for e in trace] == ["park", "acoustic", "resume", "acoustic"]
    for got, want in ((got_low, want_low), (got_urgent, want_urgent)):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.numel() > 0 and torch.isfinite(a).all() and torch.equal(a, b)
