"""GPU: cancelling requests of the serving pipelines on the reduced full pipeline (GPT decode sessions -> latent pass -> s2mel ->
vocoder).  A request cancelled while its rows are live is evicted from its slots (groups); the requests beside it come out exactly as
in a run where it was never submitted: the same codes (the session contract) and, in the exact GEMM mode, the same waveforms bit for
bit.  BatchPipeline: cancelling one of two requests that would share an acoustic batch leaves the other's waveform that of its solo
run.  The stop token is biased away, so every row runs to its cap and the cancel always lands on live rows."""
import threading
import warnings

import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu

SLOTS = 4
WAIT = 600


@pytest.fixture(scope="module")
def setup(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/cancel/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/cancel/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/cancel/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=40, tag=f"t/cancel/prompt{k}").to(device) for k in range(2)]
    return tts, conds


def _text(cfg, tag, B, L):
    return torch.from_numpy(synth.integers(f"t/cancel/{tag}", (B, L), 2, cfg.gpt.number_text_tokens))


class _Watched:
    """A decode session that tells the test when its first step has run and waits there for the go-ahead; records evict and take."""

    def __init__(self, sess, stepped, go, log):
        self._sess, self._stepped, self._go, self._log = sess, stepped, go, log

    def __getattr__(self, name):
        return getattr(self._sess, name)

    def step(self, n=1):
        out = self._sess.step(n)
        if not self._stepped.is_set():
            self._stepped.set()
            assert self._go.wait(WAIT)
        return out

    def evict(self, ids):
        self._log["evict"].append(sorted(ids))
        return self._sess.evict(ids)

    def take(self, i):
        codes = self._sess.take(i)
        self._log["take"].append((i, codes.cpu()))
        return codes


def _run(tts, reqs, submit, cancel, num_beams):
    """Submits reqs[k] for k in `submit` to a fresh ContinuousPipeline; once the first poll's steps have run, cancels those in `cancel`,
    then lets the lane go on.  Returns ({k: waveforms}, log)."""
    from indextts_amd.serving import ContinuousPipeline
    stepped, go, log = threading.Event(), threading.Event(), {"evict": [], "take": []}

    def factory(mp, mn):
        if num_beams > 1:
            return _Watched(tts.gpt.beam_session(SLOTS, num_beams, mp, mn, repetition_penalty=10.0), stepped, go, log)
        return _Watched(tts.gpt.decode_session(SLOTS, mp, mn, repetition_penalty=10.0, sampled=True), stepped, go, log)

    kw = {"num_beams": num_beams} if num_beams > 1 else {"allow_sampling": True}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ContinuousPipeline(tts, slots=SLOTS, poll_steps=2, max_new=16, session_factory=factory, **kw) as pipe:
            with pipe._cv:          # queued as one: the first poll admits what fits, in submission order
                futs = {k: pipe.submit(reqs[k]["text"], reqs[k]["cond"], max_mel_tokens=reqs[k]["cap"], sampling=reqs[k]["sampling"],
                                       noise_seed=reqs[k]["noise_seed"]) for k in submit}
            assert stepped.wait(WAIT)
            for k in cancel:
                assert pipe.cancel(futs[k]) is True
            go.set()
            got = {k: futs[k].result(timeout=WAIT) for k in submit if k not in cancel}
            for k in cancel:
                assert futs[k].cancelled()
    return got, log


@pytest.mark.parametrize("num_beams", [1, 2])
def test_cancelled_request_is_evicted_and_its_neighbours_are_untouched(setup, num_beams):
    tts, conds = setup
    cfg = tts.cfg
    if num_beams == 1:      # rows: request 0 -> slot 0, request 1 -> slots 1 and 2, request 2 -> slot 3
        shapes, places = [(1, 9), (2, 14), (1, 6)], {0: [0], 1: [1, 2], 2: [3]}
        sampling = [{"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 100 + k} for k in range(3)]
    else:                   # groups: request 0 -> group 0, request 1 -> group 1; request 2 waits and gets the evicted group
        shapes, places = [(1, 9), (1, 14), (1, 6)], {0: [0], 1: [1], 2: [1]}
        sampling = [{"do_sample": True, "num_beams": 2, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0, "seed": 100 + k}
                    for k in range(3)]
    reqs = [{"text": _text(cfg, f"text/{num_beams}/{k}", B, L), "cond": conds[k % 2], "cap": 10 + 2 * k, "sampling": sampling[k],
             "noise_seed": 7000 + k} for k, (B, L) in enumerate(shapes)]
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        got, log = _run(tts, reqs, [0, 1, 2], [1], num_beams)
        want, wlog = _run(tts, reqs, [0, 2], [], num_beams)
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert log["evict"] == [places[1]] and wlog["evict"] == []
    # codes: what the sessions handed out, in each run's own places (the second run: request 2 right behind request 0)
    mine = {k: [c for i, c in log["take"] if i in places[k]] for k in (0, 2)}
    solo = {0: [c for i, c in wlog["take"] if i == 0], 2: [c for i, c in wlog["take"] if i == 1]}
    assert len(log["take"]) == 2 and len(wlog["take"]) == 2
    for k in (0, 2):
        assert len(mine[k]) == 1 and len(mine[k][0]) == reqs[k]["cap"]
        assert torch.equal(mine[k][0], solo[k][0]), k
        assert len(got[k]) == len(want[k]) == reqs[k]["text"].shape[0]
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k
            assert torch.isfinite(a).all() and a.numel() > 0


class _HeldTTS:
    """The pipeline's tts with two places a test can hold a worker at: the first acoustic_stage call and the n-th gpt_stage call."""

    def __init__(self, tts, nth_decode):
        self._tts, self._nth, self._decodes = tts, nth_decode, 0
        self.in_acoustic, self.at_decode, self.go = threading.Event(), threading.Event(), threading.Event()

    def __getattr__(self, name):
        return getattr(self._tts, name)

    def gpt_stage(self, *a, **kw):
        self._decodes += 1
        if self._decodes == self._nth:
            self.at_decode.set()
            assert self.go.wait(WAIT)
        return self._tts.gpt_stage(*a, **kw)

    def acoustic_stage(self, *a, **kw):
        if not self.in_acoustic.is_set():
            self.in_acoustic.set()
            assert self.go.wait(WAIT)
        return self._tts.acoustic_stage(*a, **kw)


def test_batch_pipeline_cancel_in_a_merged_acoustic_batch(setup):
    """x holds the only acoustic worker, a and b are decoded and queued behind it (the lane stands at a fourth request's decode), and
    a -- the first of the pair that acoustic_coalesce = 2 would merge -- is cancelled: b's waveform is that of its solo run."""
    from indextts_amd.serving import BatchPipeline
    tts, conds = setup
    cfg = tts.cfg
    req = {n: {"text": _text(cfg, f"batch/{n}", 1, L), "seed": 9000 + i} for i, (n, L) in enumerate([("x", 5), ("a", 8), ("b", 11), ("d", 4)])}

    def submit(pipe, n):
        return pipe.submit(req[n]["text"], conds[0], max_mel_tokens=10, noise_seed=req[n]["seed"])

    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with BatchPipeline(tts, decode_lanes=1, acoustic_workers=1) as pipe:
                solo = submit(pipe, "b").result(timeout=WAIT)
            held = _HeldTTS(tts, nth_decode=4)
            with BatchPipeline(held, decode_lanes=1, acoustic_workers=1, acoustic_coalesce=2) as pipe:
                x = submit(pipe, "x")
                assert held.in_acoustic.wait(WAIT)
                a, b, d = (submit(pipe, n) for n in ("a", "b", "d"))
                assert held.at_decode.wait(WAIT)            # one lane: a and b are decoded and queued by now
                assert [r.done for r in pipe._aq] == [a, b]
                assert a.cancel() is True and pipe.cancel(x) is False
                held.go.set()
                got = b.result(timeout=WAIT)
                assert len(x.result(timeout=WAIT)) == 1 and len(d.result(timeout=WAIT)) == 1
            assert a.cancelled() and pipe._running == 0
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert len(got) == len(solo) == 1
    assert torch.equal(got[0], solo[0]) and torch.isfinite(got[0]).all() and got[0].numel() > 0
