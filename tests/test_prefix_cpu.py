"""CPU: the host side of continuing from given codes.
  * argument checks of UnifiedVoice.generate, DecodeSession.admit and ContinuousPipeline.submit that need no device;
  * how DecodeSession.admit groups a prefixed admission that exceeds the prefill area;
  * ContinuousPipeline(prefix=True) over a stand-in session: the prefixes reach admit (one per utterance, shared by its takes), the
    codes that reach the acoustic stage are prefix + continuation; a beam pipeline and a pipeline without prefix=True refuse;
  * the new prototypes: include/idxtts.h and the ctypes binding agree; tests/golden/prefix_ref.npz holds what the GPU test reads."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cancel_standins import WAIT, EvictSession, FakeTTS, Gate, cond, text
from indextts_amd import _lib
from indextts_amd.config import GPTConfig
from indextts_amd.gpt import BeamDecodeSession, DecodeSession, UnifiedVoice
from indextts_amd.serving import BatchPipeline, ContinuousPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = GPTConfig.tiny()


def _fake(B, P, k=0, fill=7):
    f = torch.ones(B, P + 1, dtype=torch.long)
    f[:, -1] = CFG.start_mel_token
    return torch.cat([f, torch.full((B, k), fill, dtype=torch.long)], 1)


def test_generate_argument_checks():
    uv = object.__new__(UnifiedVoice)       # no context: every check below comes before the first native call
    uv.cfg, uv.device = CFG, torch.device("cpu")
    emb = torch.zeros(2, 5, CFG.model_dim)
    with pytest.raises(ValueError, match=r"\[B, P\+1\+k\]"):
        uv.generate(_fake(2, 4), tts_embeddings=emb)
    with pytest.raises(ValueError, match=r"\[B, P\+1\+k\]"):
        uv.generate(_fake(3, 5, 2), tts_embeddings=emb)
    with pytest.raises(ValueError, match="prefix_layout"):
        uv.generate(_fake(2, 5, 2), tts_embeddings=emb, prefix_layout="plain")
    with pytest.raises(ValueError, match="stop token"):
        uv.generate(_fake(2, 5, 2, CFG.stop_mel_token), tts_embeddings=emb)
    with pytest.raises(ValueError, match="mel codes"):
        uv.generate(_fake(2, 5, 2, CFG.number_mel_codes), tts_embeddings=emb)
    with pytest.raises(ValueError, match="forced_codes"):
        uv.generate(_fake(2, 5, 2), tts_embeddings=emb, max_new_tokens=3, forced_codes=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="attention_mask"):
        uv.generate(_fake(2, 5, 2), tts_embeddings=emb, attention_mask=torch.ones(2, 7, dtype=torch.long))
    k = CFG.mel_pos_len - 2 - 4
    with pytest.raises(ValueError, match="mel position table"):
        uv.generate(_fake(2, 5, k + 1), tts_embeddings=emb, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="beam search does not continue"):
        uv.generate_beam(_fake(2, 5, 2), 4, None, emb)


def _bare_session(prefix=True, scores=True, sampled=True, slots=4, max_prompt=8, max_new=12):
    s = object.__new__(DecodeSession)
    s.gpt = SimpleNamespace(cfg=CFG, device=torch.device("cpu"))
    s.slots, s.max_prompt, s.max_new = slots, max_prompt, max_new
    s.prefix, s.scores, s.sampled = prefix, scores, sampled
    s._busy, s._done, s._noise, s._ws = [False] * slots, set(), {}, None
    return s


def test_admit_argument_checks():
    row = torch.zeros(5, CFG.model_dim)
    ok = [3, 4, 5]
    with pytest.raises(ValueError, match="prefix=True"):
        _bare_session(prefix=False).admit([row], 12, prefix=[ok])
    s = _bare_session()
    for kw, msg in ((dict(prefix=[[3, CFG.stop_mel_token]]), "stop token"), (dict(prefix=[[-1]]), "mel codes"),
                    (dict(prefix=[[CFG.number_mel_codes]]), "mel codes"), (dict(prefix=[ok, ok]), "one entry"),
                    (dict(prefix=[[ok]]), "1-D"), (dict(prefix=[list(range(12))]), "k < cap"),
                    (dict(prefix=[ok], prefix_logprobs=[[0.0]]), "one value per prefix code"), (dict(prefix_logprobs=[[0.0]]), "without prefix"),
                    (dict(prefix=[ok], takes=0), "takes"), (dict(prefix=[ok], slots=[9]), "slots=")):
        with pytest.raises(ValueError, match=msg):
            s.admit([row], 12, **kw)
    with pytest.raises(ValueError, match="k < cap"):
        s.admit([row], [[12, 3]], takes=2, prefix=[ok])
    with pytest.raises(ValueError, match="scores=True"):
        _bare_session(scores=False).admit([row], 12, prefix=[ok], prefix_logprobs=[[0.0] * 3])
    with pytest.raises(ValueError, match="sampled=True"):
        _bare_session(sampled=False).admit([row], 12, prefix=[ok], sampling={"sampler": "hf"})
    assert s._busy == [False] * 4
    b = object.__new__(BeamDecodeSession)
    b._ws = None
    with pytest.raises(NotImplementedError, match="beam session takes no prefix"):
        b.admit([row], 12, prefix=[ok])


def test_prefixed_admissions_are_grouped_to_fit_the_prefill_area():
    s = _bare_session(slots=16, max_prompt=22, max_new=48)
    assert s._prefill_area() == 16 * 23 + 256
    s.prefix = False
    assert s._prefill_area() == 16 * 23 + 256
    t = _bare_session(slots=1, max_prompt=22, max_new=400)
    assert t._prefill_area() == 22 + 1 + 400 + 256      # one row of max_prompt + 1 + max_new positions, padded rows included
    g = DecodeSession._prefix_groups
    area = 16 * 23 + 256
    assert g([22] * 16, [0] * 16, area) == [list(range(16))]                       # plain rows: one prefill, as ever
    groups = g([22] * 16, [40] * 16, area)                                         # 16 x 63 positions: 9 rows fit
    assert groups == [list(range(9)), list(range(9, 16))]
    for grp in g([22, 5, 22, 9] * 4, [40, 0, 47, 3] * 4, area):                    # ragged: every group fits, order kept
        S = max(p + 1 + k for p, k in zip(([22, 5, 22, 9] * 4)[grp[0]:grp[-1] + 1], ([40, 0, 47, 3] * 4)[grp[0]:grp[-1] + 1]))
        assert max(len(grp), -(-256 // S)) * S <= area and grp == list(range(grp[0], grp[-1] + 1))
    assert g([22], [47], t._prefill_area()) == [[0]] and g([], [], area) == []
    assert g([22] * 3, [399] * 3, t._prefill_area()) == [[0], [1], [2]]            # one request always fits


class PrefixSession(EvictSession):
    """The counting session with DecodeSession.admit's sampling / takes / prefix: a row behind k given codes holds them and one new
    code; take returns prefix + continuation.  Logs ("admit", slot lists, tags, takes, prefix lists, prefix_logprobs)."""

    def admit(self, rows, caps, sampling=None, takes=None, prefix=None, prefix_logprobs=None):
        nested = takes is not None
        takes = [1] * len(rows) if takes is None else list(takes)
        caps = [[c] for c in caps] if not isinstance(caps[0], (list, tuple)) else caps
        prefix = [None] * len(rows) if prefix is None else prefix
        free, out, o = self.free_slots, [], 0
        assert sum(takes) <= len(free)
        for r, t, cs, p in zip(rows, takes, caps, prefix):
            ids = free[o:o + t]
            o += t
            k = 0 if p is None else len(p)
            for s, c in zip(ids, cs):
                assert k < c
                self.state[s] = {"n": min(max(int(r[0, 0]), k + 1), int(c)), "have": k + 1, "tag": int(r[1, 0]),
                                 "prefix": torch.zeros(0, dtype=torch.long) if p is None else torch.as_tensor(p).long()}
            out.append(ids)
        self.log.append(("admit", out, [int(r[1, 0]) for r in rows], takes, [None if p is None else [int(x) for x in p] for p in prefix],
                         prefix_logprobs))
        return out if nested else [g[0] for g in out]

    def take(self, slot, scores=False):
        s = self.state[slot]
        k = len(s["prefix"])
        codes = torch.cat([s["prefix"], super().take(slot)[k:]])
        return (codes, torch.zeros(len(codes))) if scores else codes


SAMPLING = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 11}


def _pipe(tts, slots, log, gate=None, **kw):
    return ContinuousPipeline(tts, slots=slots, poll_steps=1, session_factory=lambda mp, mn: PrefixSession(slots, mp, mn, log, gate), **kw)


def test_pipeline_prefixes_reach_admit_and_results_are_prefix_plus_continuation():
    tts, log = FakeTTS(), []
    with _pipe(tts, 8, log, prefix=True) as pipe:
        fut = pipe.submit(text((6, 1), (5, 2), (4, 3)), cond(), max_mel_tokens=100, prefix_codes=[[7, 8, 9], None, torch.tensor([5])])
        plain = pipe.submit(text((3, 4)), cond(), max_mel_tokens=100)
        res, other = fut.result(timeout=WAIT), plain.result(timeout=WAIT)
    want = [[7, 8, 9, 1003, 1004, 1005], [2000, 2001, 2002, 2003, 2004], [5, 3001, 3002, 3003]]
    assert [w[:len(x)].tolist() for w, x in zip(res, want)] == want      # (the fake acoustic stage pads a request's rows to its longest)
    assert [w.tolist() for w in other] == [[4000, 4001, 4002]]
    admits = [e for e in log if e[0] == "admit"]
    assert admits[0][2][:3] == [1, 2, 3] and admits[0][4][:3] == [[7, 8, 9], None, [5]] and admits[0][5] is None


def test_pipeline_takes_share_the_prefix_and_max_mel_tokens_caps_the_whole_row():
    tts, log = FakeTTS(), []
    with _pipe(tts, 8, log, prefix=True, allow_sampling=True, scores=True) as pipe:
        fut = pipe.submit(text((50, 1), (50, 2)), cond(), max_mel_tokens=6, sampling=SAMPLING, takes=3, prefix_codes=[[7, 8], [9, 9, 9, 9]],
                          prefix_logprobs=[[-1.0, -2.0], None])
        res = fut.result(timeout=WAIT)
    assert [[w.tolist() for w in r] for r in res] == [[[7, 8, 1002, 1003, 1004, 1005]] * 3, [[9, 9, 9, 9, 2004, 2005]] * 3]
    admits = [e for e in log if e[0] == "admit"]
    assert admits[0][2] == [1, 2] and admits[0][3] == [3, 3] and admits[0][4] == [[7, 8], [9, 9, 9, 9]]      # one prompt row, one prefix each
    assert [None if l is None else l.tolist() for l in admits[0][5]] == [[-1.0, -2.0], None]


def test_pipeline_cancelled_prefixed_request_frees_its_slots():
    log, gate = [], Gate(armed=True)
    with _pipe(FakeTTS(), 4, log, gate, prefix=True) as pipe:
        fut = pipe.submit(text((50, 1), (50, 2)), cond(), max_mel_tokens=100, prefix_codes=[[7, 8], None])
        other = pipe.submit(text((2, 3)), cond(), max_mel_tokens=100)
        gate.wait()
        assert pipe.cancel(fut)
        gate.open()
        assert [w.tolist() for w in other.result(timeout=WAIT)] == [[3000, 3001]]
    assert fut.cancelled() and [e[1] for e in log if e[0] == "evict"] == [[0, 1]]


def test_submit_refusals():
    log = []
    with _pipe(FakeTTS(), 4, log) as pipe:
        with pytest.raises(ValueError, match="prefix=True"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[[1, 2]])
    with _pipe(FakeTTS(), 4, log, prefix=True) as pipe:
        for kw, msg in ((dict(prefix_codes=[[1, CFG.stop_mel_token]]), "stop token"), (dict(prefix_codes=[[1], [2]]), "one entry"),
                        (dict(prefix_codes=[[CFG.number_mel_codes]]), "mel codes"), (dict(prefix_codes=[[[1, 2]]]), "1-D"),
                        (dict(prefix_codes=[list(range(10))], max_mel_tokens=10), "shorter than max_mel_tokens"),
                        (dict(prefix_codes=[[1, 2]], prefix_logprobs=[[0.0, 0.0]]), "scores=True"), (dict(prefix_logprobs=[[0.0]]), "without prefix_codes")):
            with pytest.raises(ValueError, match=msg):
                pipe.submit(text((3, 1)), cond(), **dict(dict(max_mel_tokens=100), **kw))
        assert [w.tolist() for w in pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[None]).result(timeout=WAIT)] == [[1000, 1001, 1002]]
    with pytest.raises(ValueError, match="num_beams == 1"):
        ContinuousPipeline(FakeTTS(), slots=4, num_beams=2, prefix=True, session_factory=lambda mp, mn: None)
    beam = {"do_sample": True, "num_beams": 2, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 5}
    with ContinuousPipeline(FakeTTS(), slots=4, num_beams=2, poll_steps=1, session_factory=lambda mp, mn: SimpleNamespace(
            free_groups=[], step=lambda n=1: [], close=lambda: None)) as pipe:
        with pytest.raises(ValueError, match="beam pipeline"):
            pipe.submit(text((3, 1)), cond(), max_mel_tokens=100, sampling=beam, prefix_codes=[[1, 2]])
    with pytest.raises(NotImplementedError, match="ContinuousPipeline"):      # (refused before the pipeline is looked at: no lanes needed)
        BatchPipeline.submit(object.__new__(BatchPipeline), text((3, 1)), cond(), max_mel_tokens=100, prefix_codes=[[1, 2]])
    assert not [e for e in log if e[0] == "admit" and e[4] is not None and any(p is not None for p in e[4])]


def _header_params():
    src = open(os.path.join(ROOT, "include", "idxtts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"\b(idxtts_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


@pytest.mark.parametrize("name", ["idxtts_gpt_generate_prefix", "idxtts_gpt_session_admit_prefix"])
def test_header_and_binding_agree(name):
    declared = _header_params()
    assert name in declared and name in _lib.SYMBOLS
    fn = getattr(_lib.load(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name]
    assert _lib.SESSION_PREFIX == int(re.search(r"#define IDXTTS_SESSION_PREFIX (\d+)", open(os.path.join(ROOT, "include", "idxtts.h")).read()).group(1))


def test_fixture_shapes_and_no_stop_token_in_a_prefix(golden_dir):
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    p = np.load(os.path.join(golden_dir, "prefix_ref.npz"))
    B, V, NEW = g["text"].shape[0], CFG.number_mel_codes, int(p["new"])
    assert p["ks"].tolist() == [1, 4, 10] and NEW == 6 and g["prep_fake"].shape[1] == 23
    for k in p["ks"]:
        assert p[f"prefix_k{k}_logits"].shape == (B, NEW, V) and p[f"prefix_k{k}_logits"].dtype == np.float32
        assert p[f"prefix_k{k}_codes"].shape == (B, NEW)
        assert not (g["step_codes"][:, :k] == CFG.stop_mel_token).any()
    assert p["sample_k4_codes"].shape == (B, NEW) and p["sample_k4_noise"].shape == (NEW, B, V) and (p["sample_k4_noise"] > 0).all()
    assert p["sample_params"].tolist() == [0.8, 30.0, 0.8]
    assert (g["prep_mask"][:, :-1] == 0).sum(1).tolist() == [0, 3, 7]
