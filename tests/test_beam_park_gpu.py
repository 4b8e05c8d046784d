"""GPU: park and resume of beam groups (`BeamDecodeSession.park_group` / `resume_group`, `idxtts_gpt_session_park_group` /
`_resume_group`).

Contract pinned here: a beam group taken out of its session between steps and put back later -- into the same group, another group,
another session of the same shape, through host memory, any number of times -- goes on to the codes of its uninterrupted run, bit for
bit: row 0 of `UnifiedVoice.generate_beam` on slots / num_beams copies of its prompt (in the batch-invariant mode: the B = 1 call on its
own prompt, whatever the slot counts).  Every bystander keeps its own codes.  A parked group is a function of the request's state
alone, byte for byte, of the size include/idxtts.h documents; every refusal changes nothing.

Prompt widths are chosen so that Ps = P + 1, where the per-beam cache runs start, takes every residue mod 4: odd values leave fp8 key
runs 8-byte aligned only, non-multiples of 4 leave the scale runs 4-byte aligned only."""
import ctypes

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig
from indextts_amd.gpt import ParkedGroup, ParkedRow

pytestmark = pytest.mark.gpu

INFER = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}     # IndexTTS2.infer's defaults
SAMPLE2 = {"do_sample": True, "temperature": 1.3, "top_k": 5, "top_p": 0.5, "length_penalty": 1.0, "early_stopping": True}
SEARCH = {"do_sample": False, "length_penalty": 1.0}
SEARCH_ES = {"do_sample": False, "length_penalty": 0.0, "early_stopping": True}
KV_CODE = {"f32": 0, "bf16": 1, "fp8": 2}
NEVER, OFTEN = -1e4, 5.5      # stop-token bias: rows end at their caps / hypotheses finish while the group goes on

_MODELS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()
    _REFS.clear()


def _model(device, kv, stop_bias):
    """One model per (KV format, stop bias) for the whole module."""
    from indextts_amd.gpt import UnifiedVoice
    key = (kv, stop_bias)
    if key not in _MODELS:
        cfg = GPTConfig.tiny()
        w = weights.synth_gpt_weights(cfg, tag="t/bpark/model")
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = stop_bias
        _MODELS[key] = UnifiedVoice(w, cfg, device=device, kv_format=kv)
        _MODELS[key]._bpark_key = key
    return _MODELS[key]


def _requests(uv, tag, widths, caps, beams, nb, noise=False):
    """Prompts ([P, d] rows; P = text width + 10), each with its own conditioning and beam parameters (a seed, or its own noise)."""
    cfg, n = uv.cfg, len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, cfg.cond_latents + 2, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        beam = dict(beams[i % len(beams)])
        if noise and beam.get("do_sample"):
            g = torch.Generator().manual_seed(500 + i)
            beam["exp_noise"] = torch.empty(int(caps[i]), nb * cfg.number_mel_codes).exponential_(1.0, generator=g)
        else:
            beam["seed"] = 1000 + 7919 * i
        reqs.append({"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i]), "beam": beam, "key": (tag, i, nb, noise)})
    return reqs


def _trim(codes, stop):
    c = codes.cpu().numpy() if torch.is_tensor(codes) else np.asarray(codes)
    hits = np.nonzero(c == stop)[0]
    return c[: hits[0] + 1] if len(hits) else c


def _reference(uv, r, copies, nb):
    """Row 0 of generate_beam() on `copies` copies of the prompt with the request's parameters, up to and including the stop token:
    code that exists without this feature.  Computed once per (model, GEMM mode, mode flag, request, copies) and shared."""
    key = (uv._bpark_key, _lib.get_gemm_mode(), bool(getattr(uv, "batch_invariant", False)), r["key"], copies)
    if key not in _REFS:
        row, cap, beam = r["row"], r["cap"], r["beam"]
        P, d = row.shape
        emb = row[None].expand(copies, P, d).contiguous()
        ids = torch.ones(copies, P + 1, dtype=torch.long)
        ids[:, -1] = uv.cfg.start_mel_token
        kw = dict(num_beams=nb, do_sample=beam.get("do_sample", True), temperature=beam.get("temperature", 1.0), top_k=beam.get("top_k", 50),
                  top_p=beam.get("top_p", 1.0), length_penalty=beam.get("length_penalty", 1.0), early_stopping=beam.get("early_stopping", False))
        if beam.get("exp_noise") is not None:
            nz = beam["exp_noise"]
            kw["exp_noise"] = nz[:, None, :].expand(cap, copies, nz.shape[1]).contiguous()
        else:
            kw["seed"] = beam["seed"]
        out = uv.generate_beam(ids, cap, None, emb, repetition_penalty=10.0, **kw)
        _REFS[key] = _trim(out[0, P + 1:], uv.cfg.stop_mel_token)
    return _REFS[key]


class _Run:
    """A session with the test's book of which request sits in which group; finished groups are collected as they are reported."""

    def __init__(self, sess, reqs):
        self.sess, self.reqs, self.where, self.out = sess, reqs, {}, {}

    def admit(self, idx):
        got = self.sess.admit([self.reqs[i]["row"] for i in idx], [self.reqs[i]["cap"] for i in idx], beam=[self.reqs[i]["beam"] for i in idx])
        self.where.update(zip(got, idx))
        return got

    def step(self, n):
        for g in self.sess.step(n):
            assert g in self.where, f"step reported group {g}, which holds no request of the test"
            self.out[self.where.pop(g)] = self.sess.take(g).cpu().numpy()

    def park(self, g):
        i = self.where.pop(g)
        p = self.sess.park_group(g)
        assert isinstance(p, ParkedGroup) and isinstance(p, ParkedRow) and p.cap == self.reqs[i]["cap"] and g in self.sess.free_groups
        return i, p

    def resume(self, ip, g=None):
        got = self.sess.resume_group(ip[1], g)
        assert ip[1].resumed and got not in self.sess.free_groups and (g is None or got == g)
        self.where[got] = ip[0]
        return got

    def finish(self):
        t = 0
        while self.where:
            self.step(3)
            t += 1
            assert t < 1000


def _pad16(n):
    return (n + 15) & ~15


def _group_bytes(cfg, kv, nb, pos, step):
    """The size formula of include/idxtts.h, restated."""
    C, g, e = {"f32": (16, 16, 4), "bf16": (8, 16, 2), "fp8": (8, 8, 1)}[kv]

    def kvb(n):
        return C * _pad16(n * g) + n * 64 * e + (2 * _pad16(4 * n) if kv == "fp8" else 0)
    Ps, T = pos - step + 1, step - 1
    small = 128 + nb * _pad16(cfg.number_mel_codes) + 2 * nb * _pad16(4 * step) + 16 + _pad16(8 * nb) + 2 * _pad16(4 * nb)
    return small + cfg.layers * cfg.heads * (kvb(Ps) + nb * kvb(T))


@pytest.mark.parametrize("kv,mode,use_graph,nb,beams,noise,w0", [
    ("f32", _lib.GEMM_BF16X3, True, 3, [INFER, SEARCH], False, 5),
    ("f32", _lib.GEMM_F32, False, 2, [SAMPLE2, SEARCH_ES], True, 6),
    ("bf16", _lib.GEMM_BF16X3, True, 4, [INFER, SAMPLE2], True, 44),
    ("bf16", _lib.GEMM_F32, False, 3, [SEARCH, INFER], False, 7),
    ("fp8", _lib.GEMM_BF16X3, True, 3, [INFER, SEARCH_ES, SAMPLE2], False, 5),
    ("fp8", _lib.GEMM_F32, False, 4, [SAMPLE2, INFER], True, 6),
    ("fp8", _lib.GEMM_BF16X3, True, 2, [SEARCH, INFER], False, 8),
])
def test_group_round_trip(device, kv, mode, use_graph, nb, beams, noise, w0):
    """Three groups, five requests that end at their caps.  Request 1 is parked right after its admission (step 1: no per-beam
    positions), request 2 after one more step (step 2), request 0 mid-run (step 7); two newcomers take vacated groups and step; 1 comes
    back into the group 0 left, 2 into a group whose later tenant has finished, 0 through host memory; 1 is parked again one step
    before its cap and put back into the same group.  The parked requests have Ps = w0 + 11, w0 + 12, w0 + 13."""
    uv = _model(device, kv, NEVER)
    cfg, G = uv.cfg, 3
    widths, caps = [w0, w0 + 1, w0 + 2, w0 + 3, w0 + 8], [20, 17, 22, 9, 14]
    try:
        _lib.set_gemm_mode(mode)
        reqs = _requests(uv, f"t/bpark/rt/{w0}", widths, caps, beams, nb, noise=noise)
        sess = uv.beam_session(G * nb, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24, use_graph=use_graph)
        run = _Run(sess, reqs)
        assert run.admit([0, 1, 2]) == [0, 1, 2]
        pa = run.park(1)
        assert pa[1].n_codes == 1 and pa[1].hyp_n == 0 and pa[1].header.pos == widths[1] + 11
        assert pa[1].nbytes == _group_bytes(cfg, kv, nb, widths[1] + 11, 1)
        run.step(1)
        pb = run.park(2)
        assert pb[1].n_codes == 2 and pb[1].nbytes == _group_bytes(cfg, kv, nb, widths[2] + 12, 2)
        assert sess.free_groups == [1, 2] and sess.live_groups == [0]
        assert run.admit([3, 4]) == [1, 2]                           # newcomers in the vacated groups
        run.step(5)
        pc = run.park(0)
        assert pc[1].n_codes == 7 and pc[1].nbytes == _group_bytes(cfg, kv, nb, widths[0] + 17, 7)
        assert run.resume(pa) == 0                                   # request 1 left group 1
        run.step(3)
        assert sorted(run.out) == [3], "request 3 (cap 9) ends here"
        assert run.resume(pb) == 1                                   # request 2 left group 2; group 1 has held requests 1 and 3 since
        run.step(5)
        assert sorted(run.out) == [3, 4] and sess.free_groups == [2]
        pc[1].to("cpu")
        assert pc[1].device.type == "cpu"
        assert run.resume(pc) == 2                                   # through host memory
        run.step(7)
        pd = run.park(0)                                             # request 1 a second time, one step before its cap
        assert pd[0] == 1 and pd[1].n_codes == caps[1] - 1
        assert run.resume(pd, 0) == 0                                # into the group it just left
        run.finish()
        sess.close()
        for i, r in enumerate(reqs):
            ref = _reference(uv, r, G, nb)
            assert np.array_equal(run.out[i], ref), (i, run.out[i][:12], ref[:12])
            assert len(ref) == r["cap"], "a request stopped by itself: the stop bias is not low enough"
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


@pytest.mark.parametrize("kv", ["f32", "fp8"])
def test_scorer_state_travels_and_blobs_are_deterministic(device, kv):
    """A stop bias under which beams finish while their group goes on (early_stopping off).  Each request runs in two sessions in
    lockstep; after EVERY step both copies are parked, the two parked groups must be byte-equal and of the documented size, and each
    goes on in the OTHER session.  Session B's group first held a tenant that ran to its end, and every group holds earlier tenants'
    hypotheses and tokens as the test goes on: none of that may reach a blob.  Some parked groups carry finished hypotheses, some none."""
    uv = _model(device, kv, OFTEN)
    cfg, nb, G = uv.cfg, 3, 2
    beams = [dict(SEARCH), dict(INFER), dict(SEARCH, length_penalty=2.0), dict(SEARCH, length_penalty=0.5)]
    widths = [5, 6, 7, 8]
    reqs = _requests(uv, f"t/bpark/hyp/{kv}", widths, [24] * 4, beams, nb)
    mp = max(r["row"].shape[0] for r in reqs)
    A, B = (uv.beam_session(G * nb, nb, max_prompt=mp, max_new=24) for _ in range(2))
    first = _Run(B, reqs)
    assert first.admit([3]) == [0]
    first.finish()
    hyp_ns = []
    for i in range(3):
        r = reqs[i]
        sa, sb = A, B
        ga, gb = (s.admit([r["row"]], [r["cap"]], beam=[r["beam"]])[0] for s in (sa, sb))
        assert gb == 0
        steps = 1
        while True:
            fa, fb = sa.step(1), sb.step(1)
            assert (ga in fa) == (gb in fb), "the two copies of a request ended at different steps"
            if ga in fa:
                ca, cb = sa.take(ga).cpu().numpy(), sb.take(gb).cpu().numpy()
                break
            steps += 1
            pa, pb = sa.park_group(ga), sb.park_group(gb)
            assert torch.equal(pa._blob, pb._blob), f"request {i}: the groups parked at step {steps} differ"
            h = pa.header
            assert (h.step, h.pos, h.num_beams, h.slots, h.done) == (steps, widths[i] + 10 + steps, nb, G * nb, 0)
            assert h.bytes == pa.nbytes == _group_bytes(cfg, kv, nb, h.pos, h.step)
            assert h.magic == _lib.PARK_GROUP_MAGIC and h.length_penalty == float(r["beam"]["length_penalty"]) and list(h.reserved) == [0, 0]
            hyp_ns.append(h.hyp_n)
            ga, gb = sb.resume_group(pa), sa.resume_group(pb)       # each copy goes on in the other session
            sa, sb = sb, sa
        ref = _reference(uv, r, G, nb)
        assert np.array_equal(ca, ref) and np.array_equal(cb, ref), (i, ca[:12], cb[:12], ref[:12])
    A.close()
    B.close()
    assert np.array_equal(first.out[3], _reference(uv, reqs[3], G, nb))
    print(f"hyp_n of the parked groups ({kv}): {hyp_ns}")
    assert min(hyp_ns) == 0 and max(hyp_ns) >= 1, f"no parked group carried finished hypotheses, or every one did: {hyp_ns}"


def test_resume_restores_the_host_table(device):
    """A resumed group's parameters live in the session's host image too, which every admission uploads whole: a request is parked,
    resumed into another group, and only then another request is admitted beside it.  Both stay exact."""
    uv = _model(device, "f32", OFTEN)
    nb, G = 2, 3
    reqs = _requests(uv, "t/bpark/mirror", [9, 6], [20, 20], [dict(INFER, length_penalty=1.5), dict(SEARCH)], nb)
    sess = uv.beam_session(G * nb, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=20)
    run = _Run(sess, reqs)
    assert run.admit([0]) == [0]
    run.step(2)
    p = run.park(0)
    assert run.resume(p, 2) == 2
    assert run.admit([1]) == [0]
    run.finish()
    sess.close()
    for i, r in enumerate(reqs):
        assert np.array_equal(run.out[i], _reference(uv, r, G, nb)), i


def test_batch_invariant_groups_move_between_session_sizes(device):
    """In the batch-invariant mode a group parked in a 6-slot session resumes in a 3-slot and in a 12-slot one, to the codes of the
    B = 1 call on its own prompt; a group and a session that differ in the mode refuse each other."""
    uv = _model(device, "f32", NEVER)
    nb = 3
    uv.set_batch_invariant(True)
    try:
        reqs = _requests(uv, "t/bpark/inv", [7, 12, 5], [16, 16, 16], [INFER, SEARCH, INFER], nb)
        mp = max(r["row"].shape[0] for r in reqs)
        mk = lambda slots: uv.beam_session(slots, nb, max_prompt=mp, max_new=16)      # noqa: E731
        s6, s3, s12 = mk(6), mk(3), mk(12)
        for dst, i, k, via_cpu in ((s3, 0, 2, False), (s12, 1, 6, True)):
            src = _Run(s6, reqs)
            got = src.admit([2, i])
            s6.step(k)
            ip = src.park(got[1])
            assert ip[1].n_codes == k + 1 and ip[1].header.batch_invariant == 1 and ip[1].header.slots == 6
            if via_cpu:
                ip[1].to("cpu")
            run = _Run(dst, reqs)
            if dst is s12:
                run.admit([2])
            run.resume(ip)
            run.finish()
            assert np.array_equal(run.out[i], _reference(uv, reqs[i], 1, nb)), f"parked in 6 slots at step {k + 1}, resumed in {dst.slots}"
            src.finish()
            assert np.array_equal(src.out[2], _reference(uv, reqs[2], 1, nb))
        on = _Run(s6, reqs)
        p_on = on.park(on.admit([0])[0])
        uv.set_batch_invariant(False)
        try:
            s_off = uv.beam_session(6, nb, max_prompt=mp, max_new=16)
            off = _Run(s_off, reqs)
            p_off = off.park(off.admit([0])[0])
            assert p_off[1].header.batch_invariant == 0
            with pytest.raises(RuntimeError, match="batch-invariant"):
                s_off.resume_group(p_on[1])
            with pytest.raises(RuntimeError, match="batch-invariant mode changed"):
                s6.resume_group(p_off[1])
            assert s_off.free_groups == [0, 1] and not p_on[1].resumed and not p_off[1].resumed
            s_off.close()
        finally:
            uv.set_batch_invariant(True)
        with pytest.raises(RuntimeError, match="batch-invariant"):
            s6.resume_group(p_off[1])
        assert s6.free_groups == [0, 1] and not p_off[1].resumed
        on.resume(p_on)
        on.finish()
        assert np.array_equal(on.out[0], _reference(uv, reqs[0], 1, nb))
        for s in (s6, s3, s12):
            s.close()
    finally:
        uv.set_batch_invariant(False)


def _tampered(parked, **fields):
    """A copy of the parked group's bytes with header fields changed."""
    h = _lib.ParkGroupHeaderC.from_buffer_copy(parked._blob[:128].cpu().numpy().tobytes())
    for k, v in fields.items():
        setattr(h, k, v)
    blob = parked._blob.clone()
    blob[:128] = torch.frombuffer(bytearray(bytes(h)), dtype=torch.uint8).to(blob.device)
    return blob


# idxtts_gpt_session_workspace_bytes_beam(slots, num_beams, max_prompt, max_new) of GPTConfig.tiny() as the commit before this feature
# returns it (measured on that commit's library): the feature adds nothing to a session's workspace
WORKSPACE_BYTES = {(9, 3, 19, 14): 3497728, (6, 3, 19, 14): 2796288, (6, 2, 19, 14): 2796800, (12, 4, 62, 24): 8762624,
                   (6, 3, 18, 24): 2914560, (12, 3, 22, 16): 4532224, (3, 3, 22, 16): 2178048}


def test_refusals_change_nothing(device):
    uv = _model(device, "f32", NEVER)
    lib, nb, G = _lib.load(), 3, 3
    reqs = _requests(uv, "t/bpark/refuse", [6, 9, 4], [14, 14, 2], [INFER, SEARCH, SEARCH], nb)
    mp = max(r["row"].shape[0] for r in reqs)
    for shape, want in WORKSPACE_BYTES.items():
        assert lib.idxtts_gpt_session_workspace_bytes_beam(uv._h, *shape) == want, shape
    sess = uv.beam_session(G * nb, nb, max_prompt=mp, max_new=14)
    run = _Run(sess, reqs)
    assert run.admit([0, 1]) == [0, 1]
    run.step(3)
    vp = ctypes.c_void_p

    def raw_bytes(s, g):
        torch.cuda.synchronize()
        return lib.idxtts_gpt_session_park_group_bytes(uv._h, g, _lib.ptr(s._ws), s._sp())

    def raw_park(s, g, dst, n):
        torch.cuda.synchronize()
        rc = lib.idxtts_gpt_session_park_group(uv._h, g, _lib.ptr(dst), n, None, _lib.ptr(s._ws), s._sp())
        s.stream.synchronize()
        return rc

    def raw_resume(s, g, blob, n=None, fn=None):
        torch.cuda.synchronize()
        rc = (fn or lib.idxtts_gpt_session_resume_group)(uv._h, g, _lib.ptr(blob), blob.numel() if n is None else n, _lib.ptr(s._ws), s._sp())
        s.stream.synchronize()
        return rc

    # ---- park: a free group, a group out of range, too small a buffer, a group that has ended, another kind of session
    need = raw_bytes(sess, 0)
    assert need == _group_bytes(uv.cfg, "f32", nb, 6 + 10 + 4, 4)
    for g in (2, 3, -1):
        assert raw_bytes(sess, g) == 0
        with pytest.raises(ValueError, match="holds no request"):
            sess.park_group(g)
    buf = torch.zeros(need, dtype=torch.uint8, device=device)
    assert raw_park(sess, 0, buf, need - 16) != 0 and raw_park(sess, 2, buf, need) != 0
    assert int(buf.max()) == 0 and sess.free_groups == [2] and sess.live_groups == [0, 1]
    assert run.admit([2]) == [2]                                     # cap 2: ends with the next step
    assert sess.step(1) == [2]
    assert raw_bytes(sess, 2) == 0
    with pytest.raises(RuntimeError, match="ended"):
        sess.park_group(2)
    run.out[2] = sess.take(2).cpu().numpy()
    del run.where[2]
    greedy = uv.decode_session(G * nb, max_prompt=mp, max_new=14)
    assert greedy.admit([reqs[0]["row"]], [14]) == [0]
    greedy.step(2)
    assert raw_bytes(greedy, 0) == 0 and raw_park(greedy, 0, buf, need) != 0
    with pytest.raises(NotImplementedError):
        sess.park(0)
    with pytest.raises(NotImplementedError):
        sess.resume(None)
    # ---- resume: one parked group and one parked row, offered where they do not fit
    ip = run.park(0)
    p = ip[1]
    row = greedy.park(0)
    assert p.n_codes == 5 and sess.free_groups == [0, 2]
    with pytest.raises(TypeError):
        sess.resume_group(row)
    with pytest.raises(TypeError):
        greedy.resume(p)
    with pytest.raises(TypeError):
        sess.resume_group(p._blob)
    assert raw_resume(sess, 0, row._blob) != 0                                            # a row's magic
    assert raw_resume(greedy, 0, p._blob, fn=lib.idxtts_gpt_session_resume) != 0          # a group's magic
    assert raw_resume(greedy, 0, p._blob) != 0                                            # _resume_group on a greedy session
    for bad in (dict(magic=_lib.PARK_MAGIC), dict(version=2), dict(layers=uv.cfg.layers + 1), dict(number_mel_codes=300),
                dict(kv_format=KV_CODE["bf16"]), dict(gemm_mode=_lib.GEMM_F32), dict(num_beams=2), dict(slots=6), dict(batch_invariant=1),
                dict(max_step=15), dict(hyp_n=nb + 1), dict(bytes=p.nbytes + 16)):
        assert raw_resume(sess, 0, _tampered(p, **bad)) != 0, bad
    assert raw_resume(sess, 0, p._blob, n=p.nbytes - 16) != 0 and raw_resume(sess, 0, p._blob, n=64) != 0      # shorter than the header says
    assert raw_resume(sess, 1, p._blob) != 0 and raw_resume(sess, 3, p._blob) != 0        # busy, out of range
    with pytest.raises(ValueError, match="not free"):
        sess.resume_group(p, 1)
    with pytest.raises(ValueError, match="out of range"):
        sess.resume_group(p, 3)
    others = {"num_beams": uv.beam_session(6, 2, max_prompt=mp, max_new=14), "slots": uv.beam_session(6, nb, max_prompt=mp, max_new=14),
              "cap": uv.beam_session(G * nb, nb, max_prompt=mp, max_new=13), "cache": uv.beam_session(G * nb, nb, max_prompt=mp - 6, max_new=14)}
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        others["GEMM mode"] = uv.beam_session(G * nb, nb, max_prompt=mp, max_new=14)
        with pytest.raises(RuntimeError, match="GEMM mode"):
            others["GEMM mode"].resume_group(p)
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    for what, s in others.items():
        with pytest.raises(RuntimeError, match=what):
            s.resume_group(p)
        assert s.free_groups == list(range(s.groups)) and not p.resumed, what
        s.close()
    # ---- nothing changed: the free groups are free, the bystander decodes on, and the parked group and row resume to their codes
    assert sess.free_groups == [0, 2] and sess.live_groups == [1] and not p.resumed and not row.resumed
    assert run.resume(ip, 2) == 2
    run.finish()
    sess.close()
    for i, r in enumerate(reqs):
        assert np.array_equal(run.out[i], _reference(uv, r, G, nb)), i
    assert greedy.resume(row) == 0
    greedy.close()
