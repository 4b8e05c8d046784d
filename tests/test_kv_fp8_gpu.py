"""GPU: the opt-in scaled-fp8 KV cache of the GPT decode (include/idxtts.h, IDXTTS_KV_FP8; `kv_format="fp8"`).

The reference is the CPU oracle with the format's quantiser (tests/kv_fp8_cases.py, a numpy restatement independent of the library)
patched in where the bf16 cache mode casts: `monkeypatch.setattr(oracle.gpt, "gpt2_stack", fp8_stack)`."""
import numpy as np
import pytest
import torch

import kv_fp8_cases as kc
from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

# What the fp8 cache may add to a logit against the patched fp32 oracle on the two greedy shapes below: a key / value a few ulp apart
# between two fp32 summation orders may round to the other e4m3 neighbour (2^-4 relative, against bf16's 2^-9), and a vector's largest
# element to the other side of a scale step.  Measured on MI355X, teacher-forced: max |dlogit| 6.5e-3 (mean 1.3e-4) at (B, heads,
# NEW) = (2, 2, 300) and 1.835e-2 (mean 4.8e-4) at (9, 16, 240), no argmax differing (profiles/README.md "fp8 KV cache"); the constant
# is about 2.5 x the larger.  For scale: the patched fp32 and float64 oracles themselves differ by up to 3.9e-4 and 1.85e-2
# on these shapes (tests/test_kv_fp8_cpu.py prints it), the quantisation itself moves a logit by 0.15-0.32 against the fp32 cache, and at 5e-2 the
# bound would no longer tell this format from a wrong one.  (With the prefill on the split-bf16 GEMMs the same run gave 5.5e-2 and
# 4.3e-2: why the prefill of an fp8 cache stays on the exact GEMMs, csrc/gpt.hip::layer_full.)
BOUND = 4.5e-2


@pytest.fixture
def fp8_oracle(monkeypatch):
    import oracle.gpt
    monkeypatch.setattr(oracle.gpt, "gpt2_stack", kc.fp8_stack)
    return oracle.gpt


def _uv(device, cfg, w, kv="fp8", **kw):
    from indextts_amd.gpt import UnifiedVoice
    return UnifiedVoice(w, cfg, device=device, kv_format=kv, **kw)


def test_device_quantiser_equals_the_restatement_bit_for_bit(device):
    """idxtts_kv_fp8_quantize -- the device routine the store kernels and the decode attention call -- on the CPU test's vectors."""
    lib = _lib.load()
    x = kc.case_vectors()
    n = x.shape[0]
    xd = torch.from_numpy(x).to(device)
    codes = torch.zeros(n, 64, dtype=torch.uint8, device=device)
    scales = torch.zeros(n, dtype=torch.float32, device=device)
    _lib.check(lib.idxtts_kv_fp8_quantize(xd.data_ptr(), n, codes.data_ptr(), scales.data_ptr(), None))
    torch.cuda.synchronize()
    want_codes, want_scales, _ = kc.quantize(x)
    assert np.array_equal(scales.cpu().numpy(), want_scales)
    bad = np.nonzero(codes.cpu().numpy() != want_codes)
    assert len(bad[0]) == 0, (len(bad[0]), x[bad][:8], codes.cpu().numpy()[bad][:8], want_codes[bad][:8])


@pytest.mark.parametrize("B,heads,NEW", kc.GREEDY_SHAPES)
def test_fp8_kv_cache_long_decode_vs_patched_oracle(device, fp8_oracle, B, heads, NEW):
    """Teacher-forced on the patched oracle's codes (oracle/parity.py): every logit within BOUND, every differing argmax a near-tie of
    the oracle (margin <= 2 BOUND), and the free-running decode leaves the oracle exactly at its first teacher-forced mismatch.
    (2, 2, 300): the keys split over workgroups, about 600 of them; (9, 16, 240): unsplit, `pos` passes 512 -- the second pass of the
    512-thread score loop -- with a left-padded row (kstart)."""
    from oracle import parity
    cfg, w, lat, emo, text = kc.greedy_case(B, heads)
    uv = _uv(device, cfg, w)
    assert uv.kv_format == "fp8" and uv.weight_format == "f32" and _lib.load().idxtts_gpt_get_kv_format(uv._h) == 2
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    torch.set_num_threads(8)
    r = parity.decode_parity(uv, tw, cfg, lat, emo, text, NEW)
    print(f"[kv fp8 parity B={B} heads={heads}] max|dlogit| {r['max_abs_logit_diff']:.3e} (mean {r['mean_abs_logit_diff']:.3e}, logit std "
          f"{r['logit_std']:.2f}), teacher-forced match rate {r['codes_match_rate_teacher_forced']:.4f}, mismatches {r['mismatching_steps']}, "
          f"first teacher-forced {r['first_mismatch_step_teacher_forced']}, first free-running {r['first_difference_step_free_running']}")
    assert r["steps"] == NEW and r["utterances"] == B and r["kv_cache"] == "fp8"
    assert r["max_abs_logit_diff"] <= BOUND, r["max_abs_logit_diff"]
    for t in r["mismatching_steps"]:
        assert 0.0 <= t["oracle_margin_to_hip_token"] <= 2 * BOUND, t
    assert r["first_difference_step_free_running"] == r["first_mismatch_step_teacher_forced"]


def test_format_switching_on_one_context(device):
    """f32 -> fp8 -> bf16 -> fp8 on one context and one workspace: the two fp8 runs are bit-equal (cached decode graphs are keyed by
    the format), the f32 and bf16 runs equal what the context gave before fp8 was ever selected."""
    cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=130, number_text_tokens=90, start_mel_token=128, stop_mel_token=129,
                    max_mel_tokens=200, max_text_tokens=60, cond_latents=8)
    w = weights.synth_gpt_weights(cfg, tag="t/gpt/kv8/switch")
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = -1e4
    B, L, NEW = 3, 21, 70
    lat = torch.from_numpy(synth.uniform("t/gpt/kv8/switch/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/gpt/kv8/switch/emo", (B, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/gpt/kv8/switch/text", (B, L), 2, cfg.number_text_tokens))
    text[2, 9:] = cfg.stop_text_token
    uv = _uv(device, cfg, w, kv="f32")

    def run(fmt):
        uv.set_kv_format(fmt)
        assert uv.kv_format == fmt
        return uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=NEW, repetition_penalty=10.0)[0].cpu()

    before = {"f32": run("f32"), "bf16": run("bf16")}
    seq = [(f, run(f)) for f in ("f32", "fp8", "bf16", "fp8")]
    assert torch.equal(seq[0][1], before["f32"]) and torch.equal(seq[2][1], before["bf16"])
    assert torch.equal(seq[1][1], seq[3][1]) and seq[1][1].shape[1] == NEW
    assert not torch.equal(seq[1][1], before["f32"]), "70 codes on flat logits: an fp8 cache that decodes like the fp32 one is not in use"


# The beam test's weights and the decision margin it asserts of them.  Margins above BOUND do not exist on this shape: among 120 weight
# tags, the patched oracle's smallest decision gap over a generation of 12 steps or more is at best 4.3e-3 (48 to 144 twelve-way
# decisions on nearly flat logits; only generations that stop after 3 or 4 steps, and move no cache rows, reach 3e-2).  Tag 0 runs all
# 24 steps in both modes with gaps of 4.2e-3 (beam-sample) and 8.0e-3 (beam search); that is what is asserted, against a cache of at
# most 40 keys, where the greedy test's 600-key shape of the same width measured a largest logit difference of 6.5e-3.
BEAM_TAG = "t/gpt/kv8/beam/0"
BEAM_MARGIN = 4e-3


def _decision_margin(trace):
    """The oracle's closest decision: the smallest per-step gap of generate_beam's trace over every step and utterance.  A gap of
    exactly 0 or NaN is structural, not a near-tie -- a finished utterance's padding, or a sampled step with fewer survivors than
    candidates, whose zero keys and -inf scores both sides order by index -- and is left out."""
    gaps = torch.stack([t[3] for t in trace]).flatten()
    gaps = gaps[torch.isfinite(gaps) & (gaps != 0)]
    assert len(gaps) >= len(trace)
    return float(gaps.min())


def test_fp8_kv_cache_beam_search_and_beam_sample_vs_patched_oracle(device, fp8_oracle):
    """test_bf16_kv_cache_beam_sample_vs_oracle's shape on the fp8 cache: codes AND scales of the generated positions follow their rows
    through the beam re-indexing -- tokens equal the patched oracle.gpt.generate_beam.  The weight tag is one for which the oracle's
    own decisions (return_trace: the smallest gap of a step's selection keys and candidate scores) stay above BEAM_MARGIN; asserted
    here, so that a change of the inputs cannot make the comparison flaky silently."""
    og = fp8_oracle
    cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=70, number_text_tokens=40, start_mel_token=68, stop_mel_token=69,
                    max_mel_tokens=60, max_text_tokens=30, cond_latents=4)
    w = weights.synth_gpt_weights(cfg, tag=BEAM_TAG)
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] += 3.0
    uv = _uv(device, cfg, w)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    B, L, NEW, NB = 2, 7, 24, 3
    lat = torch.from_numpy(synth.uniform("t/gpt/kv16/beam/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/gpt/kv16/beam/emo", (B, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/gpt/kv16/beam/text", (B, L), 2, cfg.number_text_tokens))
    g = torch.Generator().manual_seed(11)
    noise = torch.empty(NEW, B, NB * cfg.number_mel_codes).exponential_(1.0, generator=g)
    for do_sample in (True, False):
        codes, _ = uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=NEW, num_beams=NB, do_sample=do_sample, top_p=0.8, top_k=30,
                                       temperature=0.8, repetition_penalty=10.0, length_penalty=0.0, exp_noise=noise)
        with torch.no_grad():
            want, trace = og.generate_beam(tw, cfg, og.conds_latent(tw, cfg, lat, emo), text, NEW, noise, num_beams=NB, do_sample=do_sample,
                                           return_trace=True)
        margin = _decision_margin(trace)
        print(f"[kv fp8 beam do_sample={do_sample}] oracle's smallest decision gap {margin:.3e} over {len(trace)} steps")
        assert margin > BEAM_MARGIN and len(trace) == NEW, (do_sample, margin, len(trace))
        got = codes.cpu().numpy()
        assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy()), do_sample


# ---- sessions keep their contracts bit for bit under fp8: slots = 4, staggered admissions, caps <= 24 ----
HF = {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8}
GREEDY = {"sampler": "greedy"}
BEAM_SAMPLE = {"do_sample": True, "temperature": 0.8, "top_k": 30, "top_p": 0.8, "length_penalty": 0.0}
BEAM_SEARCH = {"do_sample": False, "length_penalty": 1.0}


def _session_model(device, tag):
    cfg = GPTConfig.tiny()
    w = weights.synth_gpt_weights(cfg, tag=tag)
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] = 2.0
    return cfg, _uv(device, cfg, w)


def _requests(uv, cfg, tag, widths, caps, extra=None):
    nc = cfg.cond_latents + 2
    n = len(widths)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (n, nc, cfg.model_dim), 0.5)).to(uv.device)
    reqs = []
    for i in range(n):
        text = torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, widths[i]), 2, cfg.number_text_tokens))
        r = {"row": uv.prompt_rows(conds[i:i + 1], text)[0], "cap": int(caps[i])}
        if extra is not None:
            r["par"] = dict(extra[i % len(extra)])
            if r["par"].get("sampler") != "greedy":
                r["par"]["seed"] = 1000 + 7919 * i
        reqs.append(r)
    return reqs


def _trim(codes, stop):
    c = codes.cpu().numpy()
    hits = np.nonzero(c == stop)[0]
    return c[: hits[0] + 1] if len(hits) else c


def _drive(sess, reqs, key, free, live, seed):
    """Admit one or two waiting requests whenever units are free, step one to four steps at a time.  Returns ({request: codes}, how
    many admissions landed beside a unit that was already decoding)."""
    rng = np.random.default_rng(seed)
    waiting, where, out, beside = list(range(len(reqs))), {}, {}, 0
    while waiting or where:
        units = getattr(sess, free)
        if waiting and units:
            k = min(len(waiting), len(units), int(rng.integers(1, 3)))
            group, waiting = waiting[:k], waiting[k:]
            beside += 1 if getattr(sess, live) else 0
            kw = {key: [reqs[i]["par"] for i in group]} if key else {}
            for u, i in zip(sess.admit([reqs[i]["row"] for i in group], [reqs[i]["cap"] for i in group], **kw), group):
                where[u] = i
        for u in sess.step(int(rng.integers(1, 5))):
            out[where.pop(u)] = sess.take(u).cpu().numpy()
    return out, beside


def _copies(uv, row, n):
    P, d = row.shape
    ids = torch.ones(n, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    return ids, row[None].expand(n, P, d).contiguous(), P


@pytest.mark.parametrize("sampled,mode", [(False, _lib.GEMM_BF16X3), (True, _lib.GEMM_BF16X3), (False, _lib.GEMM_F32)])
def test_fp8_decode_session_equals_generate_on_copies(device, sampled, mode):
    """Prompts of a few dozen rows in either arithmetic mode: the prefill of an fp8 cache runs on the exact GEMMs whatever its row
    count, so (unlike a bf16 session in split-bf16 mode) an admission needs no padding to match a 4-copy reference."""
    cfg, uv = _session_model(device, "t/kv8/sess")
    slots = 4
    widths, caps = [3, 17, 9, 30, 5, 12, 22], [24, 9, 17, 24, 5, 20, 13]
    try:
        _lib.set_gemm_mode(mode)
        reqs = _requests(uv, cfg, "t/kv8/sess", widths, caps, extra=[HF, GREEDY, HF] if sampled else None)
        sess = uv.decode_session(slots, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24, sampled=sampled)
        out, beside = _drive(sess, reqs, "sampling" if sampled else None, "free_slots", "live_slots", seed=3)
        sess.close()
        assert sorted(out) == list(range(len(reqs))) and beside >= 2
        for i, r in enumerate(reqs):
            ids, emb, P = _copies(uv, r["row"], slots)
            kw = {}
            if sampled and r["par"]["sampler"] != "greedy":
                p = r["par"]
                kw = dict(do_sample=True, sampler=p["sampler"], temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], seed=p["seed"])
            ref = _trim(uv.generate(ids, max_new_tokens=r["cap"], tts_embeddings=emb, repetition_penalty=10.0, **kw)[0, P + 1:], cfg.stop_mel_token)
            assert np.array_equal(out[i], ref), (i, out[i][:12], ref[:12])
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_fp8_beam_session_equals_generate_beam_on_copies(device):
    """num_beams = 2 in 4 slots: an admission fans the prompt's codes and scales out to both slots of its group."""
    cfg, uv = _session_model(device, "t/kv8/bsess")
    slots, nb = 4, 2
    widths, caps = [4, 19, 11, 27, 6], [24, 10, 16, 21, 8]
    reqs = _requests(uv, cfg, "t/kv8/bsess", widths, caps, extra=[BEAM_SAMPLE, BEAM_SEARCH])
    sess = uv.beam_session(slots, nb, max_prompt=max(r["row"].shape[0] for r in reqs), max_new=24)
    out, beside = _drive(sess, reqs, "beam", "free_groups", "live_groups", seed=2)
    sess.close()
    assert sorted(out) == list(range(len(reqs))) and beside >= 2
    for i, r in enumerate(reqs):
        ids, emb, P = _copies(uv, r["row"], slots // nb)
        p = r["par"]
        ref = uv.generate_beam(ids, r["cap"], None, emb, repetition_penalty=10.0, num_beams=nb, do_sample=p["do_sample"],
                               temperature=p.get("temperature", 1.0), top_k=p.get("top_k", 50), top_p=p.get("top_p", 1.0),
                               length_penalty=p["length_penalty"], early_stopping=False, seed=p["seed"])
        ref = _trim(ref[0, P + 1:], cfg.stop_mel_token)
        assert np.array_equal(out[i], ref), (i, out[i][:12], ref[:12])


def test_fp8_workspace_is_about_half_the_bf16_one(device):
    """Codes plus fp32 scales, 68 bytes per cached vector against 128: the KV region of every workspace entry is at most 0.57 x the
    bf16 one at (16 rows, Smax = 2048).  The fp32 region is twice the bf16 one, so their difference measures the bf16 region."""
    cfg = GPTConfig(model_dim=256, heads=4, layers=3, number_mel_codes=130, number_text_tokens=90, start_mel_token=128, stop_mel_token=129,
                    max_mel_tokens=1600, max_text_tokens=600, cond_latents=8)
    uv = _uv(device, cfg, weights.synth_gpt_weights(cfg, tag="t/gpt/kv8/mem"), kv="f32")
    lib, h = _lib.load(), uv._h
    B, S, NEW = 16, 548, 1500
    entries = {
        "generate": lambda: lib.idxtts_gpt_workspace_bytes(h, B, S, NEW),
        "beam": lambda: lib.idxtts_gpt_beam_workspace_bytes(h, 4, 4, S, NEW),
        "session": lambda: lib.idxtts_gpt_session_workspace_bytes(h, B, S - 1, NEW),
        "sampled session": lambda: lib.idxtts_gpt_session_workspace_bytes_ex(h, B, S - 1, NEW, 1),
        "beam session": lambda: lib.idxtts_gpt_session_workspace_bytes_beam(h, B, 4, S - 1, NEW),
    }
    vectors = 2 * cfg.layers * B * cfg.heads * 2048
    for name, fn in entries.items():
        size = {}
        for fmt in ("f32", "bf16", "fp8"):
            uv.set_kv_format(fmt)
            size[fmt] = int(fn())
            assert size[fmt] > 0, (name, fmt)
        kv16 = size["f32"] - size["bf16"]
        kv8 = size["fp8"] - (size["bf16"] - kv16)
        assert abs(kv16 - 128 * vectors) <= 4096, (name, kv16, 128 * vectors)
        assert 64 * vectors <= kv8 <= 0.57 * kv16, (name, kv8, kv16)
        assert abs(kv8 - 68 * vectors) <= 4096, (name, kv8)


def test_device_gate_and_unknown_format(device):
    cfg = GPTConfig.tiny()
    uv = _uv(device, cfg, weights.synth_gpt_weights(cfg, tag="t/kv8/gate"), kv="bf16")
    lib = _lib.load()
    uv.set_kv_format("fp8")                                   # this device's conversions are OCP e4m3fn, both ways
    assert uv.kv_format == "fp8" and lib.idxtts_gpt_get_kv_format(uv._h) == 2
    with pytest.raises(ValueError, match="kv_format"):
        uv.set_kv_format("fp4")
    assert uv.kv_format == "fp8" and lib.idxtts_gpt_get_kv_format(uv._h) == 2      # untouched
    assert lib.idxtts_gpt_set_kv_format(uv._h, 3) != 0 and lib.idxtts_gpt_get_kv_format(uv._h) == 2
    with pytest.raises(ValueError, match="kv_format"):
        _uv(device, cfg, weights.synth_gpt_weights(cfg, tag="t/kv8/gate"), kv="e5m2")
    from indextts_amd.gpt import UnifiedVoice
    assert UnifiedVoice(weights.synth_gpt_weights(cfg, tag="t/kv8/gate"), cfg, device=device, weight_format="fp8").kv_format == "bf16"
