"""GPU: the batch-invariant mode of the GPT decode (`idxtts_gpt_set_batch_invariant`, `UnifiedVoice.set_batch_invariant`).

The contract (include/idxtts.h), bit for bit and without a tolerance: with the mode on, a request's codes and logits equal those of the
B = 1 call on its own unpadded prompt -- as any row of a one-shot call of any B with any left padding, in any slot or group of a
session of any size, after a park and a resume into a session of another size, through every pipeline -- and seeded draws carry no term
in the batch size.

Model: full width (d = 1280, 20 heads, V = 8194: N and K hit the real GEMV plan rules), 2 layers, synthetic weights, the stop token
biased away so rows end at their caps.  Requests are prompt-embedding rows: R (40 positions), its neighbours of other lengths, and
LONG (500 positions), whose decode crosses 512 keys -- where the mode's attention goes from one piece to two -- and puts > 16 rows of
left padding on R.  Every B = 1 reference is computed once per (weights, KV format) and shared."""
import os

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

NEW = 24
P_R, P_LONG = 40, 500
PENALTY = 10.0
_MODELS, _REFS = {}, {}


def _cfg():
    return GPTConfig(model_dim=1280, heads=20, layers=2, number_mel_codes=8194, number_text_tokens=60, start_mel_token=8192,
                     stop_mel_token=8193, max_mel_tokens=80, max_text_tokens=20, cond_latents=4)


def _model(device, wfmt="f32", kv="f32", on=True):
    """One model per weight format for the whole module, its KV format switched between generations; in the mode unless `on` is false
    (the guard test, which has to run on a library without the mode too)."""
    from indextts_amd.gpt import UnifiedVoice
    if wfmt not in _MODELS:
        cfg = _cfg()
        w = weights.synth_gpt_weights(cfg, tag="t/binv/model")
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = -1e4
        _MODELS[wfmt] = UnifiedVoice(w, cfg, device=device, weight_format=wfmt, kv_format="f32")
    uv = _MODELS[wfmt]
    if on or hasattr(uv, "set_batch_invariant"):
        uv.set_batch_invariant(on)
    if uv.kv_format != kv:
        uv.set_kv_format(kv)
    return uv


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()
    _REFS.clear()


def _prompt(name, P, device):
    return torch.from_numpy(synth.uniform(f"t/binv/prompt/{name}", (P, 1280), 0.5)).to(device)


def _forced(name):
    return torch.from_numpy(synth.integers(f"t/binv/forced/{name}", (NEW,), 0, 8192)).long()


def _batch(rows):
    """Left-padded one-shot inputs of the prompt rows: (fake ids, embeddings [B, Pmax, d], attention mask)."""
    B, pm = len(rows), max(r.shape[0] for r in rows)
    emb = torch.zeros(B, pm, 1280, device=rows[0].device)
    mask = torch.ones(B, pm + 1, dtype=torch.long)
    for i, r in enumerate(rows):
        emb[i, pm - r.shape[0]:] = r
        mask[i, : pm - r.shape[0]] = 0
    ids = torch.ones(B, pm + 1, dtype=torch.long)
    ids[:, -1] = 8192
    return ids, emb, mask


def _forced_run(uv, rows, names):
    """Teacher-forced one-shot call: (each row's own argmax codes [B, NEW], logits [B, NEW, V])."""
    ids, emb, mask = _batch(rows)
    fc = torch.stack([_forced(n) for n in names])
    out, logits = uv.generate(ids, max_new_tokens=NEW, attention_mask=mask, tts_embeddings=emb, repetition_penalty=PENALTY,
                              return_logits=True, forced_codes=fc)
    codes = out[:, ids.shape[1]:]
    assert codes.shape[1] == NEW
    return codes, logits


def _ref(uv, name, P):
    """The B = 1 teacher-forced call of request `name` on its own unpadded prompt, once per (weights, KV format)."""
    key = (uv.weight_format, uv.kv_format, _lib.get_gemm_mode(), name)
    if key not in _REFS:
        _REFS[key] = _forced_run(uv, [_prompt(name, P, uv.device)], [name])
    return _REFS[key]


def _fillers(n, device, longest):
    """n neighbours of R with lengths 8 .. longest, all different from R's where it matters."""
    return [(f"f{i}", _prompt(f"f{i}", 8 + (7 * i) % (longest - 7), device)) for i in range(n)]


def _compose(B, where, pad, device):
    """A B-row batch with R at row `where` under `pad` rows of left padding: 0 (R is the longest), 1 (one neighbour a row longer) or
    'long' (LONG beside it: P_LONG - P_R rows).  Returns (names, rows)."""
    rows = _fillers(B, device, P_R - 1)
    rows[where] = ("R", _prompt("R", P_R, device))
    other = (where + 1) % B
    if pad == 1 and B > 1:
        rows[other] = ("g41", _prompt("g41", P_R + 1, device))
    elif pad == "long" and B > 1:
        rows[other] = ("LONG", _prompt("LONG", P_LONG, device))
    return [n for n, _ in rows], [r for _, r in rows]


def _check_rows(uv, B, label):
    """R at row 0 without padding, at a middle row under 1 row of padding and at the last row under P_LONG - P_R rows, in B-row
    one-shot calls; LONG (no padding, two attention pieces from 512 keys on) is checked in the call that holds it."""
    dev = uv.device
    want_c, want_l = _ref(uv, "R", P_R)
    for where, pad in ((0, 0), (B // 2, 1), (B - 1, "long")):
        names, rows = _compose(B, where, pad, dev)
        codes, logits = _forced_run(uv, rows, names)
        r = names.index("R")
        assert torch.equal(logits[r], want_l[0]), f"{label} B={B}: logits of R at row {r} (pad {pad}) differ from its B = 1 call"
        assert torch.equal(codes[r], want_c[0]), f"{label} B={B}: codes of R at row {r} (pad {pad}) differ from its B = 1 call"
        if "LONG" in names:
            lc, ll = _ref(uv, "LONG", P_LONG)
            q = names.index("LONG")
            assert torch.equal(logits[q], ll[0]) and torch.equal(codes[q], lc[0]), f"{label} B={B}: LONG at row {q} differs from its B = 1 call"


# ---- 1. the shapes can tell ----
@pytest.mark.parametrize("B", [4, 16])
def test_mode_off_rows_depend_on_batch(device, B):
    """Guard: with the mode off, LONG's teacher-forced logits at B = 1 and as a row of B = 4 / 16 are not all bit-equal (key split of
    12 / 3 / 1 pieces, the 4-row GEMV form against the 16-row one) -- so the equalities below are not vacuous."""
    uv = _model(device, on=False)
    _, one = _forced_run(uv, [_prompt("LONG", P_LONG, device)], ["LONG"])
    names, rows = _compose(B, 0, "long", device)
    _, many = _forced_run(uv, rows, names)
    assert not torch.equal(many[names.index("LONG")], one[0]), f"mode off: B = 1 and B = {B} agree bit for bit; lengthen the context"


# ---- 2. static calls ----
@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("B", [2, 4, 5, 16, 17, 48, 64])
def test_static_rows_equal_single_f32_weights(device, B, kv):
    _check_rows(_model(device, "f32", kv), B, f"f32 weights, {kv} KV")


@pytest.mark.parametrize("kv", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("B", [4, 5, 17, 64])
def test_static_rows_equal_single_bf16_weights(device, B, kv):
    _check_rows(_model(device, "bf16", kv), B, f"bf16 weights, {kv} KV")


@pytest.mark.parametrize("B", [4, 16, 49])
def test_static_rows_equal_single_fp8_weights(device, B):
    _check_rows(_model(device, "fp8", "bf16"), B, "fp8 weights, bf16 KV")


@pytest.mark.parametrize("B", [2, 5, 16])
def test_static_rows_bf16_kv_split_mode_both_sides_of_256(device, B):
    """bf16 KV in split-bf16 GEMM mode (the default mode; asserted): the B = 1 prefill of R has 41 rows, B = 2 with LONG 1002, B = 5
    without it 5 x 42 = 210, B = 16 656 -- total prefill rows on both sides of the 256-row kernel switch, one GEMM family."""
    assert _lib.get_gemm_mode() == _lib.GEMM_BF16X3
    _check_rows(_model(device, "f32", "bf16"), B, "split-bf16 mode, bf16 KV")


def test_graph_replay_codes_equal_single(device):
    """Free-running greedy generation through the captured step (graphs keyed by the mode): R's codes at B = 1, 4, 16 and 48."""
    uv = _model(device, "bf16", "bf16")
    got = {}
    for B in (1, 4, 16, 48):
        names, rows = _compose(B, B - 1, "long" if B > 1 else 0, device)
        ids, emb, mask = _batch(rows)
        out = uv.generate(ids, max_new_tokens=NEW, attention_mask=mask, tts_embeddings=emb, repetition_penalty=PENALTY)
        got[B] = out[names.index("R"), ids.shape[1]:]
        assert got[B].shape[0] == NEW
    for B in (4, 16, 48):
        assert torch.equal(got[B], got[1]), f"graph-replayed codes of R at B = {B} differ from B = 1"


# ---- 3. sampled ----
@pytest.mark.parametrize("sampler", ["hf", "accel"])
def test_sampled_seed_row0_and_noise_every_row(device, sampler):
    uv = _model(device, "f32", "f32")
    kw = dict(do_sample=True, sampler=sampler, temperature=0.8, top_k=30, top_p=0.8, max_new_tokens=NEW, repetition_penalty=PENALTY)
    R = _prompt("R", P_R, device)

    def run(rows, **extra):
        ids, emb, mask = _batch(rows)
        return uv.generate(ids, attention_mask=mask, tts_embeddings=emb, **kw, **extra)[:, ids.shape[1]:]

    one = run([R], seed=1234)
    assert one.shape[1] == NEW
    for B in (3, 17):
        rows = [R] + [r for _, r in _fillers(B - 1, device, 60)]
        assert torch.equal(run(rows, seed=1234)[0], one[0]), f"{sampler}: seeded row 0 at B = {B} differs from the B = 1 call"
    B = 5
    rows = [r for _, r in _fillers(B - 1, device, 60)] + [R]
    noise = torch.from_numpy(np.random.default_rng(5).exponential(size=(NEW, B, 8194)).astype(np.float32))
    many = run(rows, exp_noise=noise)
    for b in range(B):
        assert torch.equal(run([rows[b]], exp_noise=noise[:, b:b + 1].contiguous())[0], many[b]), f"{sampler}: row {b} under its own noise"


# ---- 4. beams ----
BEAM = dict(num_beams=3, temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=PENALTY, length_penalty=0.0)


def _beam_single(uv, do_sample):
    key = ("beam", uv.weight_format, uv.kv_format, do_sample)
    if key not in _REFS:
        ids, emb, mask = _batch([_prompt("R", P_R, uv.device)])
        _REFS[key] = uv.generate_beam(ids, NEW, mask, emb, do_sample=do_sample, seed=77, **BEAM)[0, ids.shape[1]:]
    return _REFS[key]


@pytest.mark.parametrize("do_sample", [False, True])
def test_beam_static_utterance0_equal_single(device, do_sample):
    uv = _model(device, "f32", "f32")
    want = _beam_single(uv, do_sample)
    for B in (2, 5, 16):
        rows = [_prompt("R", P_R, device)] + [r for _, r in _fillers(B - 1, device, 60)]
        ids, emb, mask = _batch(rows)
        got = uv.generate_beam(ids, NEW, mask, emb, do_sample=do_sample, seed=77, **BEAM)[0, ids.shape[1]:]
        n = min(len(got), len(want))      # the call's width is its longest utterance: R's own codes are its first len(want)
        assert n == len(want) and torch.equal(got[:n], want), f"beam (do_sample={do_sample}): utterance 0 at B = {B} differs from B = 1"


@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("slots", [6, 12, 48])
def test_beam_session_equal_single(device, slots, do_sample):
    uv = _model(device, "f32", "f32")
    want = _beam_single(uv, do_sample).cpu()
    stop = uv.cfg.stop_mel_token
    want = want[: int((want == stop).nonzero()[0]) + 1] if (want == stop).any() else want
    sess = uv.beam_session(slots, 3, max_prompt=80, max_new=NEW, repetition_penalty=PENALTY)
    beam = dict(do_sample=do_sample, temperature=0.8, top_k=30, top_p=0.8, length_penalty=0.0, seed=77)
    fill = [r for _, r in _fillers(slots // 3 - 1, device, 60)]
    sess.admit(fill, NEW, beam=dict(beam, seed=5))
    g = sess.admit([_prompt("R", P_R, device)], NEW, beam=beam)[0]
    done = set()
    for _ in range(NEW + 2):
        done |= set(sess.step(4))
        if g in done:
            break
    assert g in done
    assert torch.equal(sess.take(g).cpu(), want), f"beam session of {slots} slots (do_sample={do_sample}) differs from the B = 1 call"
    sess.close()


# ---- 5. sessions ----
def _single_codes(uv, name, P, par):
    key = ("gen", uv.weight_format, uv.kv_format, name, tuple(sorted(par.items())))
    if key not in _REFS:
        ids, emb, mask = _batch([_prompt(name, P, uv.device)])
        kw = {}
        if par.get("sampler", "greedy") != "greedy":
            kw = dict(do_sample=True, sampler=par["sampler"], temperature=par["temperature"], top_k=par.get("top_k", 0),
                      top_p=par.get("top_p", 1.0), seed=par["seed"])
        out = uv.generate(ids, max_new_tokens=NEW, attention_mask=mask, tts_embeddings=emb, repetition_penalty=PENALTY, **kw)
        _REFS[key] = out[0, ids.shape[1]:].cpu()
        assert len(_REFS[key]) == NEW
    return _REFS[key]


def _run_to_end(sess, slot):
    for _ in range(2 * NEW):
        if slot in sess.step(3):
            return sess.take(slot).cpu()
    raise AssertionError("the request did not finish")


GREEDY = {"sampler": "greedy"}
HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8, "seed": 99}


@pytest.mark.parametrize("par", [GREEDY, HF], ids=["greedy", "sampled"])
@pytest.mark.parametrize("slots", [1, 3, 16, 48])
def test_session_requests_equal_single(device, slots, par):
    """R admitted alone, admitted late beside running neighbours, and admitted into an evicted slot: always the B = 1 call's codes."""
    uv = _model(device, "f32", "bf16")
    want = _single_codes(uv, "R", P_R, par)
    sampled = par is not GREEDY
    sess = uv.decode_session(slots, max_prompt=80, max_new=NEW, repetition_penalty=PENALTY, sampled=sampled)
    samp = (lambda n: [dict(par)] * n) if sampled else (lambda n: None)
    R = _prompt("R", P_R, device)
    s = sess.admit([R], NEW, sampling=samp(1))[0]                       # alone
    assert torch.equal(_run_to_end(sess, s), want), f"{slots} slots: admitted alone"
    if slots > 1:
        fill = [r for _, r in _fillers(slots - 1, device, 60)]
        ids = sess.admit(fill, NEW, sampling=[dict(HF, seed=i) for i in range(slots - 1)] if sampled else None)
        sess.step(5)
        s = sess.admit([R], NEW, sampling=samp(1))[0]                   # late, beside running neighbours
        assert torch.equal(_run_to_end(sess, s), want), f"{slots} slots: admitted late"
        for i in sess.step(2 * NEW):
            sess.take(i)
        ids = sess.admit(fill + [fill[0]], NEW, sampling=[dict(HF, seed=i) for i in range(slots)] if sampled else None)
        sess.step(7)
        sess.evict(ids[slots // 2])
        s = sess.admit([R], NEW, sampling=samp(1))[0]                   # into the evicted slot
        assert s == ids[slots // 2]
        assert torch.equal(_run_to_end(sess, s), want), f"{slots} slots: admitted into an evicted slot"
    sess.close()


# ---- 6. park / resume across sizes ----
@pytest.mark.parametrize("par", [GREEDY, HF], ids=["greedy", "sampled"])
def test_park_resume_across_session_sizes(device, par):
    uv = _model(device, "f32", "bf16")
    want = _single_codes(uv, "R", P_R, par)
    sampled = par is not GREEDY
    R = _prompt("R", P_R, device)
    mk = lambda n: uv.decode_session(n, max_prompt=80, max_new=NEW, repetition_penalty=PENALTY, sampled=sampled)
    s16, s4, s48 = mk(16), mk(4), mk(48)
    fill = [r for _, r in _fillers(15, device, 60)]
    for dst, via_cpu, k in ((s4, False, 5), (s48, False, 9), (s48, True, 13)):
        s16.admit(fill[:7], NEW, sampling=[dict(HF, seed=i) for i in range(7)] if sampled else None)
        slot = s16.admit([R], NEW, sampling=[dict(par)] if sampled else None)[0]
        s16.step(k)
        parked = s16.park(slot)
        assert parked.n_codes == k + 1
        if via_cpu:
            parked = parked.to("cpu").to(uv.device)
        dst.admit(fill[7:9], NEW, sampling=[dict(HF, seed=50 + i) for i in range(2)] if sampled else None)
        got = _run_to_end(dst, dst.resume(parked))
        assert torch.equal(got, want), f"parked at step {k} in 16 slots, resumed in {dst.slots} (via cpu: {via_cpu})"
        for sess in (s16, dst):
            sess.evict([i for i in range(sess.slots) if i not in sess.free_slots])
    for sess in (s16, s4, s48):
        sess.close()


def test_park_resume_refused_across_modes(device):
    """A mode-on row offered to a mode-off session, and the reverse, is refused with nothing changed."""
    uv = _model(device, "f32", "bf16")
    R = _prompt("R", P_R, device)
    mk = lambda: uv.decode_session(4, max_prompt=80, max_new=NEW, repetition_penalty=PENALTY)
    on = mk()
    slot = on.admit([R], NEW)[0]
    on.step(3)
    row_on = on.park(slot)
    hdr = _lib.ParkHeaderC.from_buffer_copy(row_on._blob[:128].cpu().numpy().tobytes())
    assert hdr.version == 1 and list(hdr.reserved) == [1, 0, 0, 0, 0, 0, 0, 0]
    uv.set_batch_invariant(False)
    try:
        off = mk()
        slot = off.admit([R], NEW)[0]
        off.step(3)
        row_off = off.park(slot)
        hdr = _lib.ParkHeaderC.from_buffer_copy(row_off._blob[:128].cpu().numpy().tobytes())
        assert list(hdr.reserved) == [0] * 8, "a row parked with the mode off carries zeros"
        with pytest.raises(RuntimeError, match="batch-invariant"):
            off.resume(row_on)
        assert off.free_slots == [0, 1, 2, 3] and not row_on.resumed
        with pytest.raises(RuntimeError, match="batch-invariant mode changed"):
            on.resume(row_off)          # the context's mode differs from the session's: every call on it is refused
    finally:
        uv.set_batch_invariant(True)
    with pytest.raises(RuntimeError, match="batch-invariant"):
        on.resume(row_off)
    assert on.free_slots == [0, 1, 2, 3] and not row_off.resumed
    want = _single_codes(uv, "R", P_R, GREEDY)
    assert torch.equal(_run_to_end(on, on.resume(row_on)), want)
    on.close()
    uv.set_batch_invariant(False)
    try:
        off.resume(row_off)
        off.close()
    finally:
        uv.set_batch_invariant(True)


# ---- 8. switches ignored ----
def test_process_switches_do_not_move_the_mode(device):
    uv = _model(device, "bf16", "bf16")
    dev = uv.device
    names, rows = _compose(16, 15, "long", dev)
    want = _forced_run(uv, rows, names)
    try:
        _lib.set_decode_geometry(True)
        _lib.set_decode_plane_rows(5)
        got = _forced_run(uv, rows, names)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), "narrow geometry / plane_rows = 5 moved the mode's logits"
        r = names.index("R")
        assert torch.equal(got[1][r], _ref(uv, "R", P_R)[1][0])
    finally:
        _lib.set_decode_geometry(False)
        _lib.set_decode_plane_rows(0)
    assert _lib.get_decode_plane_rows() == 17 and _lib.get_decode_geometry() is False


# ---- 9. still the right model ----
def test_mode_greedy_codes_equal_golden(golden_dir, device):
    """fp32 KV, exact GEMM: the reference's own greedy codes (tests/golden/gpt_ref.npz), as tests/test_gpt_ref_gpu.py checks them."""
    from indextts_amd.gpt import UnifiedVoice
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    uv = UnifiedVoice(weights.synth_gpt_weights(cfg, tag="golden/gptref"), cfg, device=device, batch_invariant=True)
    mode = _lib.get_gemm_mode()
    _lib.set_gemm_mode(_lib.GEMM_F32)
    try:
        conds = torch.from_numpy(g["conds"]).to(device)
        fake, emb, mask = uv.prepare_gpt_inputs(conds, torch.from_numpy(g["text"]))
        n = g["step_codes"].shape[1]
        for graph in (False, True):
            out = uv.generate(fake, max_new_tokens=n, stop_tokens=[cfg.stop_mel_token], attention_mask=mask, tts_embeddings=emb,
                              repetition_penalty=10.0, use_graph=graph)
            np.testing.assert_array_equal(out[:, fake.shape[1]:].cpu().numpy(), g["step_codes"])
    finally:
        _lib.set_gemm_mode(mode)


@pytest.mark.parametrize("model,fmt", [("d1280", "f32"), ("d128", "bf16"), ("d64", "fp8")])
def test_mode_logits_within_float64_bound(device, model, fmt):
    """Teacher-forced logits against the float64 oracle within the bound tests/gemv_cases.py derives -- 4 x what fp32 accumulation in
    another summation order costs the float32 oracle: the mode changes summation order and nothing else."""
    import gemv_cases as gc
    from indextts_amd.gpt import UnifiedVoice
    rows = gc.max_rows(model, fmt)
    uv = UnifiedVoice(gc.original_weights(model), gc.config(model), device=device, weight_format=fmt, kv_format="f32", batch_invariant=True)
    ref = gc.reference(model, fmt)
    want = ref.codes[:rows]
    n = want.shape[1]
    lat, emo, text = gc.inputs(model, rows)
    forced = torch.full((rows, gc.NEW), uv.cfg.stop_mel_token, dtype=torch.long)
    forced[:, :n] = want
    codes, _, logits = uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=gc.NEW, repetition_penalty=gc.PENALTY,
                                           return_logits=True, forced_codes=forced)
    kerr = float((logits.cpu()[:, :n].double() - ref.logits[:rows]).abs().max())
    tol = ref.tolerance(rows)
    print(f"\n{model} {fmt} {rows} rows, mode on: kernel error {kerr:.3e}, float32 oracle error {ref.oracle_error(rows):.3e}, bound {tol:.3e}")
    assert np.isfinite(kerr) and kerr <= tol
    free, _ = uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=gc.NEW, repetition_penalty=gc.PENALTY)
    assert np.array_equal(free.cpu().numpy(), want.numpy())


# ---- 7. pipelines ----
def test_pipelines_give_the_same_codes(device):
    """The same requests through ContinuousPipeline(slots=4), ContinuousPipeline(slots=16, decode_lanes=2), BatchPipeline(coalesce=3),
    synthesize_batch, and a decode merged by hand (what a coalesced BatchPipeline group runs): the same codes per utterance.  The
    requests are greedy with seeded CFM noise -- BatchPipeline and synthesize_batch take no sampler seed -- and the codes are read where
    every path hands them to the stages behind the decode (gpt_stage's state), keyed by the utterance's text."""
    import threading
    import warnings
    from indextts_amd.config import PipelineConfig
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    from indextts_amd.serving import BatchPipeline, ContinuousPipeline
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/binv/pipe/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = 6.5      # rows stop by themselves, at different steps
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/binv/pipe/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/binv/pipe/voc"), device=device,
                                     gpt_weight_format="bf16", batch_invariant=True)
    assert tts.gpt.batch_invariant and _lib.load().idxtts_gpt_get_batch_invariant(tts.gpt._h) == 1
    cond = PromptConditioning.synthetic(cfg, prompt_frames=40, tag="t/binv/pipe/prompt").to(device)
    CAP, L = 24, 9
    reqs = []
    for k in range(7):
        B = 1 + k % 3
        text = torch.from_numpy(synth.integers(f"t/binv/pipe/text{k}", (B, L), 2, cfg.gpt.number_text_tokens))
        if B > 1:
            text[1, L - 1 - k % 4:] = cfg.gpt.stop_text_token      # a shorter utterance: left padding inside the request
        reqs.append(text)
    seen, lock, stage = {}, threading.Lock(), tts.gpt_stage

    def recording(text_tokens, *a, **kw):
        st = stage(text_tokens, *a, **kw)
        with lock:
            for row, c, n in zip(torch.as_tensor(text_tokens).cpu().tolist(), st["codes"].cpu(), st["code_lens"]):
                seen.setdefault(tuple(row), []).append(tuple(c[:n].tolist()))
        return st

    tts.gpt_stage = recording
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            paths = 0
            for make in (lambda: ContinuousPipeline(tts, slots=4, poll_steps=3, max_new=CAP),
                         lambda: ContinuousPipeline(tts, slots=16, decode_lanes=2, poll_steps=5, max_new=CAP),
                         lambda: BatchPipeline(tts, decode_lanes=1, coalesce=3)):
                with make() as pipe:
                    futs = [pipe.submit(t, cond, max_mel_tokens=CAP, noise_seed=100 + k) for k, t in enumerate(reqs)]
                    for f in futs:
                        f.result(timeout=600)
                paths += 1
            for k, t in enumerate(reqs):
                tts.synthesize_batch(t, cond, max_mel_tokens=CAP, noise_seeds=[100 + k] * t.shape[0])
            paths += 1
            tts.gpt_stage(torch.cat(reqs), cond, max_mel_tokens=CAP)      # one decode of all 13 utterances
            paths += 1
    finally:
        del tts.gpt_stage
    torch.cuda.synchronize()
    rows = [tuple(r) for t in reqs for r in t.tolist()]
    assert len(set(rows)) == len(rows) == 13
    for r in rows:
        assert len(seen[r]) == paths, f"an utterance went through {len(seen[r])} of {paths} paths"
        assert len(set(seen[r])) == 1, f"the paths gave {len(set(seen[r]))} different code sequences for one utterance"
    print("\ncode lengths per utterance:", [len(seen[r][0]) for r in rows])
    assert len({len(seen[r][0]) for r in rows}) > 1, "every utterance has the same length: the stop token never decided anything"
