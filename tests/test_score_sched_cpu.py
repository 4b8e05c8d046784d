"""CPU: the host side of scoring given codes.
  * ContinuousPipeline(prefix=True, scores=True, prefix_scores=True) over a stand-in session: prefix_logprobs="model" reaches admit per
    utterance (beside arrays and None), and its refusals hold;
  * DecodeSession.admit's and UnifiedVoice.score_codes' argument checks that need no device;
  * the new prototypes: include/idxtts.h and the ctypes binding agree."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cancel_standins import WAIT, FakeTTS, cond, text
from indextts_amd import _lib
from indextts_amd.config import GPTConfig
from indextts_amd.gpt import DecodeSession, UnifiedVoice
from indextts_amd.serving import ContinuousPipeline
from test_prefix_cpu import SAMPLING, PrefixSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = GPTConfig.tiny()


def _pipe(tts, slots, log, factory_log=None, **kw):
    def factory(mp, mn):
        return PrefixSession(slots, mp, mn, log, None)
    return ContinuousPipeline(tts, slots=slots, poll_steps=1, session_factory=factory, **kw)


def _lps(entry):
    return [l if l is None or isinstance(l, str) else torch.as_tensor(l).tolist() for l in entry]


def test_model_reaches_admit_per_utterance():
    tts, log = FakeTTS(), []
    with _pipe(tts, 8, log, prefix=True, allow_sampling=True, scores=True, prefix_scores=True) as pipe:
        fut = pipe.submit(text((50, 1), (50, 2), (50, 3)), cond(), max_mel_tokens=6, sampling=SAMPLING, takes=2,
                          prefix_codes=[[7, 8], [9, 9, 9], [4]], prefix_logprobs=["model", [-1.0, -2.0, -3.0], None])
        res = fut.result(timeout=WAIT)
        assert [[w.tolist()[:2] for w in r] for r in res][0] == [[7, 8]] * 2
        every = pipe.submit(text((50, 4), (50, 5)), cond(), max_mel_tokens=6, sampling=SAMPLING, prefix_codes=[[7, 8], None],
                            prefix_logprobs="model")
        every.result(timeout=WAIT)
    admits = [e for e in log if e[0] == "admit"]
    assert admits[0][3] == [2, 2, 2] and admits[0][4] == [[7, 8], [9, 9, 9], [4]]
    assert _lps(admits[0][5]) == ["model", [-1.0, -2.0, -3.0], None]
    assert admits[1][4] == [[7, 8], None] and _lps(admits[1][5]) == ["model", None]      # one string: every utterance that has a prefix


def test_submit_and_constructor_refusals():
    log = []
    with _pipe(FakeTTS(), 4, log, prefix=True, scores=True) as pipe:
        with pytest.raises(ValueError, match="prefix_scores=True"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[[1, 2]], prefix_logprobs=["model"])
        with pytest.raises(ValueError, match="prefix_scores=True"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[[1, 2]], prefix_logprobs="model")
    with _pipe(FakeTTS(), 4, log, prefix=True, scores=True, prefix_scores=True) as pipe:
        for kw, msg in ((dict(prefix_codes=[[1, 2]], prefix_logprobs=["other"]), '"model"'),
                        (dict(prefix_codes=[None], prefix_logprobs=["model"]), "without prefix_codes"),
                        (dict(prefix_logprobs="model"), "without prefix_codes"),
                        (dict(prefix_codes=[[1, CFG.stop_mel_token]], prefix_logprobs="model"), "stop token")):
            with pytest.raises(ValueError, match=msg):
                pipe.submit(text((3, 1)), cond(), **dict(dict(max_mel_tokens=100), **kw))
        # the next valid request still runs
        assert [w.tolist() for w in pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[[5]],
                                                prefix_logprobs="model").result(timeout=WAIT)] == [[5, 1001, 1002]]
    for kw in (dict(prefix=True), dict(scores=True), dict()):
        with pytest.raises(ValueError, match="prefix=True and scores=True"):
            ContinuousPipeline(FakeTTS(), slots=4, prefix_scores=True, session_factory=lambda mp, mn: None, **kw)
    assert not [e for e in log if e[0] == "admit" and e[5] is not None and "other" in _lps(e[5])]


def _bare_session(prefix_scores, slots=4, max_prompt=8, max_new=12):
    s = object.__new__(DecodeSession)
    s.gpt = SimpleNamespace(cfg=CFG, device=torch.device("cpu"))
    s.slots, s.max_prompt, s.max_new = slots, max_prompt, max_new
    s.prefix, s.scores, s.sampled, s.prefix_scores = True, True, True, prefix_scores
    s._busy, s._done, s._noise, s._ws = [False] * slots, set(), {}, None
    return s


def test_admit_argument_checks():
    row = torch.zeros(5, CFG.model_dim)
    with pytest.raises(ValueError, match="prefix_scores=True"):
        _bare_session(False).admit([row], 12, prefix=[[3, 4]], prefix_logprobs=["model"])
    s = _bare_session(True)
    for kw, msg in ((dict(prefix=[[3, 4]], prefix_logprobs=["logits"]), '"model"'),
                    (dict(prefix_logprobs=["model"]), "without prefix"),
                    (dict(prefix=[[3, CFG.stop_mel_token]], prefix_logprobs=["model"]), "stop token"),
                    (dict(prefix=[list(range(12))], prefix_logprobs=["model"]), "k < cap")):
        with pytest.raises(ValueError, match=msg):
            s.admit([row], 12, **kw)
    assert s._busy == [False] * 4
    with pytest.raises(ValueError, match="prefix=True and scores=True"):
        DecodeSession(SimpleNamespace(), 4, 8, 12, prefix=True, prefix_scores=True)


def test_score_codes_argument_checks():
    uv = object.__new__(UnifiedVoice)       # no context: every check below comes before the first native call
    uv.cfg, uv.device = CFG, torch.device("cpu")
    emb = torch.zeros(2, 5, CFG.model_dim)
    codes = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="layout"):
        uv.score_codes(codes, emb, layout="plain")
    with pytest.raises(ValueError, match=r"\[B, P, d\]"):
        uv.score_codes(codes, emb[0])
    with pytest.raises(ValueError, match="one row per prompt"):
        uv.score_codes(codes[:1], emb)
    with pytest.raises(ValueError, match="one row per prompt"):
        uv.score_codes([[1, 2], [3], [4]], emb)
    with pytest.raises(ValueError, match="code_lens"):
        uv.score_codes(codes, emb, code_lens=[4, 4, 4])


def _header_params():
    src = open(os.path.join(ROOT, "include", "idxtts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"\b(idxtts_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


@pytest.mark.parametrize("name", ["idxtts_gpt_score", "idxtts_gpt_score_workspace_bytes", "idxtts_gpt_session_admit_prefix_scored"])
def test_header_and_binding_agree(name):
    declared = _header_params()
    assert name in declared and name in _lib.SYMBOLS
    fn = getattr(_lib.load(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name]
    src = open(os.path.join(ROOT, "include", "idxtts.h")).read()
    assert _lib.SESSION_PREFIX_SCORES == int(re.search(r"#define IDXTTS_SESSION_PREFIX_SCORES (\d+)", src).group(1)) == 16
