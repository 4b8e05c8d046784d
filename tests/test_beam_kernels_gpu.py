"""GPU: the beam kernels (`beam_scores_kernel`, `beam_select_kernel`, the two reorder kernels, `beam_session_reset_kernel`:
csrc/beam.hip) and `beam_finalize` / `check_beam` (csrc/gpt_beam.hip) against the float64 reference and the restated draws of
tests/beam_cases.py -- at real vocabulary sizes, on both paths of beam_select_kernel (nb * V up to 32768 in registers, the
re-reading loop above), with 2 to 8 beams, on crafted rows with ties, oversized tie groups, few survivors and scorer edge cases, with
seeded and explicit draws, and as a distribution.

Every case admits one crafted request into every group of a beam session with caps 1, 2, ... G (eager and replayed) and compares
group c with the reference stopped after c steps; then `generate_beam` at cap G, eager and replayed.  What "equal" means, the rows and
the cap on undecidable caps: tests/beam_cases.py; tests/test_beam_cases_cpu.py checks that the reference alone keeps every case list
here within the cap and agrees with oracle.gpt.generate_beam.  Natural rows go through the oracle itself and cover what crafted rows
cannot: the KV re-indexing.  Each test prints its counts (-s shows them)."""
import numpy as np
import pytest
import torch

import beam_cases as bc
import sampler_cases as sc

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(device, bias, weight_format="f32"):
    """Crafted models by row: cases that differ in the request's parameters only share one (the last few are kept)."""
    from indextts_amd.gpt import UnifiedVoice
    key = (bias.tobytes(), weight_format)
    if key not in _MODELS:
        while len(_MODELS) >= 4:
            _MODELS.pop(next(iter(_MODELS)))
        _MODELS[key] = UnifiedVoice(sc.crafted_weights(bias), sc.config(bias.size), device=device, weight_format=weight_format)
    return _MODELS[key]


def _prompt_row(uv, device):
    conds, texts = sc.prompts(uv.cfg.number_mel_codes, (6,))
    return uv.prompt_rows(conds[:1].to(device), texts[0])[0]


def _beam_kw(c):
    p = c["prm"]
    return dict(do_sample=p["do_sample"], temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"],
                length_penalty=p["length_penalty"], early_stopping=p["early_stopping"])


def _trim(codes, stop):
    c = codes.cpu().numpy() if torch.is_tensor(codes) else np.asarray(codes)
    hits = np.nonzero(c == stop)[0]
    return [int(x) for x in (c[: hits[0] + 1] if len(hits) else c)]


def _session_outs(uv, row, c, use_graph):
    """The case's request in every group of a G-group session, caps 1 .. G: the codes per cap."""
    G, nb = c["G"], c["prm"]["num_beams"]
    sess = uv.beam_session(G * nb, nb, max_prompt=row.shape[0], max_new=G, repetition_penalty=c["prm"]["penalty"], use_graph=use_graph)
    beams = []
    for cap in range(1, G + 1):
        b = _beam_kw(c)
        if c["draws"] is not None:
            kind, x = c["draws"]
            if kind == "seed":
                b["seed"] = x
            else:
                b["exp_noise"] = torch.from_numpy(np.ascontiguousarray(x[:cap]))
        beams.append(b)
    groups = sess.admit([row] * G, list(range(1, G + 1)), beam=beams)
    assert groups == list(range(G))
    done, guard = set(), 0
    while len(done) < G:
        done.update(sess.step(2))
        guard += 1
        assert guard < 50
    outs = [[int(x) for x in sess.take(g).cpu().numpy()] for g in groups]
    sess.close()
    return outs


def _generate_beam(uv, row, c, use_graph, B=None):
    """Row 0 of generate_beam on B copies of the prompt at cap G (a seeded case: G copies, the session's draws), up to and including
    its first stop token."""
    G, nb, V = c["G"], c["prm"]["num_beams"], uv.cfg.number_mel_codes
    B = B or (G if c["draws"] is not None and c["draws"][0] == "seed" else 2)
    P, d = row.shape
    ids = torch.ones(B, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    kw = _beam_kw(c)
    if c["draws"] is not None:
        kind, x = c["draws"]
        if kind == "seed":
            kw["seed"] = x
        else:
            kw["exp_noise"] = torch.from_numpy(x)[:, None, :].expand(G, B, nb * V).contiguous()
    out = uv.generate_beam(ids, G, None, row[None].expand(B, P, d).contiguous(), num_beams=nb, repetition_penalty=c["prm"]["penalty"],
                           use_graph=use_graph, **kw)
    return _trim(out[0, P + 1:], uv.cfg.stop_mel_token)


def _check_case(device, c, what, tally, ref=None):
    uv = _model(device, c["bias"], c["weight_format"])
    row = _prompt_row(uv, device)
    ref = ref or bc.reference(c)
    G = c["G"]
    for use_graph in (False, True):
        outs = _session_outs(uv, row, c, use_graph)
        for cap in range(1, G + 1):
            tally.checked += 1
            if ref.first_bad is not None and cap >= ref.first_bad:
                tally.excused += 1
                continue
            assert outs[cap - 1] == ref.outs[cap - 1], \
                f"{what} session(graph={use_graph}) cap {cap}: codes {outs[cap - 1]}, reference {ref.outs[cap - 1]}"
        got = _generate_beam(uv, row, c, use_graph)
        tally.checked += 1
        if ref.first_bad is not None:
            tally.excused += 1
        else:
            assert got == ref.outs[G - 1], f"{what} generate_beam(graph={use_graph}): codes {got}, reference {ref.outs[G - 1]}"
    return ref


def _run_list(device, lst, name):
    c = bc.ALL_LISTS[lst]()[name]
    tally = bc.Tally()
    ref = _check_case(device, c, f"{lst}[{name}]", tally)
    print(f"{lst}[{name}]: {tally}; reference {ref.outs[-1]}")
    assert tally.checked == 2 * (c["G"] + 1)
    if c["exact"]:
        assert tally.excused == 0
    return tally


# ---- the harness's own precondition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", ["f32", "bf16"])
def test_returned_logits_are_the_bias(device, weight_format):
    """A zero mel_head.weight makes every row's logits mel_head.bias bit for bit, with f32 and with bf16 weight streams (the bias
    stays fp32): an exact row and a flat sampling row, through generate(..., return_logits=True) on the models the cases use."""
    for bias in (bc.scorer_cases()["near3_lp1_es0"]["bias"], bc.select_switch_cases()["nb8_V8194_noise"]["bias"]):
        uv = _model(device, bias, weight_format)
        conds, texts = sc.prompts(bias.size, (6, 6))
        fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
        out, logits = uv.generate(fake, max_new_tokens=3, tts_embeddings=emb, repetition_penalty=1.0, return_logits=True)
        logits = logits.cpu().numpy()
        assert logits.shape[0] == 2 and logits.shape[2] == bias.size
        want = np.broadcast_to(bias.view(np.uint32), logits.shape)
        assert np.array_equal(np.ascontiguousarray(logits).view(np.uint32), want)


# ---- the case lists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.vocabulary_cases()))
def test_vocabulary_edges(device, name):
    """num_beams = 3 at V = 1023 .. 16384 (one to sixteen slices of a 1024-thread block, partial last slices), beam-sample with a
    seed and with explicit draws."""
    _run_list(device, "vocabulary", name)


@pytest.mark.parametrize("name", sorted(bc.select_switch_cases()))
def test_select_path_switch(device, name):
    """nb * V = 32768 exactly (4 x 8192, 8 x 4096: every key in registers) and above (4 x 8193, 8 x 4097, 4 x 8194, 8 x 8194: the
    re-reading loop), beam-sample with explicit draws that are the same per (beam, token) on either side of the switch, seeded
    beam-sample over the whole vocabulary, and beam search on an exact row."""
    _run_list(device, "select_switch", name)


@pytest.mark.parametrize("name", sorted(bc.filter_cases()))
def test_filters(device, name):
    """top_k 1 (raised to 2), 2, 30, 1024 and above V; ties that straddle the k-th value; signed zeros; 3029 survivors of top_k = 30
    under top_p < 1 (more than the 2048 the top-p stage sorts: the tie group is walked by count); top-p between two cumulative sums,
    down to the last two, just below 1, and off with top_k = 0; fewer survivors than 2 * num_beams with 3, 4 and 8 beams (fillers by
    the lowest flat index, with a score of -inf).
    Before the tie group was walked by count, ties3000_all_removed and ties3000_cut_inside failed: the staging area took the first
    2048 survivors to arrive, the threshold came from those, and ids of the tie group that the nucleus excludes became beams (cap 2
    of the first: [8143, 8191] for [8148, 8143]; cap 1 of the second: [1919] for [5958])."""
    _run_list(device, "filter", name)


@pytest.mark.parametrize("name", sorted(bc.scorer_cases()))
def test_scorer(device, name):
    """BeamSearchScorer.process, BeamHypotheses.add / is_done and finalize on exact rows (nothing excused) and under beam-sample:
    a stop token inside and below the best num_beams, num_beams + 1 hypotheses (the worst dropped, the earliest of equals), is_done
    one grid step either side of equality under length_penalty 0, 1, 2, -1, early_stopping, equal best scores at finalize (the last
    wins), groups that finish before their caps beside ones that reach them; 2, 3, 4 and 8 beams."""
    _run_list(device, "scorer", name)


def test_plane_gemv_head_feeds_the_same_kernels(device):
    """bf16 weight streams, 8 beams x 6 groups = 48 rows: the head runs on the plane GEMV; the loop path of beam_select_kernel."""
    from indextts_amd import _lib
    assert _lib.load().idxtts_get_decode_plane_rows() <= 48
    c = dict(bc.select_switch_cases()["nb8_V8194_noise"], weight_format="bf16")
    tally = bc.Tally()
    _check_case(device, c, "bf16 weights", tally)
    print(f"plane_gemv_head: {tally}")
    assert tally.excused == 0


# ---- draw extremes --------------------------------------------------------------------------------------------------------
def test_draw_extremes(device):
    """The seeds under which one element of step 0 draws the all-ones 24 bits (bounded at u = 1 - 2^-24: a draw of 6e-8, not 0) or the
    all-zero bits (17.3): the likeliest id becomes the first beam under the first, and both stay the reference's codes."""
    x = bc.extreme_seeds()
    tally = bc.Tally()
    for what, seed in (("plain", x["base"]), ("all-ones", x["ones"][0]), ("all-zero", x["zeros"][0])):
        ref = _check_case(device, bc.extreme_case(seed), f"draw extremes, {what}", tally)
        if what == "all-ones":
            assert ref.outs[0][0] == x["ones"][1]
    print(f"draw_extremes: {tally}")
    assert tally.excused == 0


# ---- the distribution -----------------------------------------------------------------------------------------------------
def test_distribution_of_first_step_candidates(device):
    """100 seeded calls x 32 utterances, 2 beams, cap 1: each returned code is the likeliest of the four ids drawn without replacement
    from the eight survivors of top_k = 8.  Pearson's chi-square against that law (by enumeration) at the 1 - 1e-6 quantile, as in
    tests/test_sampler_gpu.py; every code the reference's on the restated draws.  The reference alone (test_beam_cases_cpu.py) gives
    1.1 on 3 degrees of freedom against 30.7."""
    bias = bc.dist_bias()
    uv = _model(device, bias)
    row = _prompt_row(uv, device)
    P, d = row.shape
    B, nb = bc.DIST_B, bc.DIST_NB
    ids = torch.ones(B, P + 1, dtype=torch.long)
    ids[:, -1] = uv.cfg.start_mel_token
    emb = row[None].expand(B, P, d).contiguous()
    p = bc.dist_prm()
    kw = dict(num_beams=nb, do_sample=True, temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"],
              repetition_penalty=p["penalty"], length_penalty=p["length_penalty"])
    toks, tally = [], bc.Tally()
    for call in range(bc.DIST_CALLS):
        out = uv.generate_beam(ids, 1, None, emb, seed=bc.DIST_SEED + call, use_graph=False, **kw)[:, P + 1:].cpu().numpy()
        assert out.shape == (B, 1)
        for b in range(B):
            want, ok = bc.dist_reference(call, b)
            tally.checked += 1
            if ok:
                assert out[b, 0] == want, (call, b, out[b, 0], want)
            else:
                tally.excused += 1
        toks.extend(out[:, 0].tolist())
    stat, dof = sc.chi_square(np.array(toks), bc.dist_probs())
    bound = sc.chi2_quantile(dof)
    print(f"distribution: chi-square {stat:.1f} on {dof} degrees of freedom, bound {bound:.1f}; {tally}")
    assert stat <= bound and tally.within_cap()
    replay = uv.generate_beam(ids, 1, None, emb, seed=bc.DIST_SEED, use_graph=True, **kw)[:, P + 1:].cpu().numpy()
    assert replay[:, 0].tolist() == toks[:B]


# ---- natural rows: the KV re-indexing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", bc.KV_FORMATS)
@pytest.mark.parametrize("nb", bc.KV_BEAMS)
def test_kv_reindexing_on_natural_rows(device, nb, kv):
    """2 layers, model_dim 128, natural logits, 2, 4 and 8 beams in an f32 and a bf16 KV cache: the beams' generated keys and
    values move every step (beam_reorder_kv_kernel; register arrays of num_beams granules), and a wrong move changes the next
    logits.  Against oracle.gpt.generate_beam (exact GEMM mode, the oracle's arithmetic; kv_round for the bf16 cache), beam search
    and beam-sample; an utterance may leave the oracle only where the oracle's own closest decision up to there was within 2e-3
    (the rule of tests/test_fullsize_gpu.py), and at most one of the three does."""
    from indextts_amd import _lib, synth, weights
    from indextts_amd.config import GPTConfig
    from indextts_amd.gpt import UnifiedVoice
    from oracle import gpt as og
    cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=258, number_text_tokens=40, start_mel_token=256, stop_mel_token=257,
                    max_mel_tokens=40, max_text_tokens=30, cond_latents=4)
    w = weights.synth_gpt_weights(cfg, tag="t/beamk/kv")
    w["mel_head.bias"] = w["mel_head.bias"].copy()
    w["mel_head.bias"][cfg.stop_mel_token] += 1.0
    uv = UnifiedVoice(w, cfg, device=device, kv_format=kv if kv == "bf16" else None)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    B, L, NEW, V = 3, 7, bc.KV_NEW, cfg.number_mel_codes
    lat = torch.from_numpy(synth.uniform("t/beamk/kv/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
    emo = torch.from_numpy(synth.uniform("t/beamk/kv/emo", (B, cfg.model_dim), 0.3))
    text = torch.from_numpy(synth.integers("t/beamk/kv/text", (B, L), 2, cfg.number_text_tokens))
    noise = torch.empty(NEW, B, nb * V).exponential_(1.0, generator=torch.Generator().manual_seed(100 + nb))
    try:
        _lib.set_gemm_mode(_lib.GEMM_F32)
        fake, emb, mask = uv.prepare_gpt_inputs(uv.conds_latent(lat.to(device), emo.to(device)), text)
        for do_sample in (False, True):
            with torch.no_grad():
                want, trace = og.generate_beam(tw, cfg, og.conds_latent(tw, cfg, lat, emo), text, NEW, noise, num_beams=nb,
                                               do_sample=do_sample, return_trace=True, kv_round=kv == "bf16")
            want = want.numpy()
            moved = sum(int((tr[0].view(B, nb) != torch.arange(B * nb).view(B, nb)).any()) for tr in trace)
            assert moved >= 3, "the beams never changed places: the test shows nothing"
            for use_graph in (False, True):
                out = uv.generate_beam(fake, NEW, mask, emb, num_beams=nb, do_sample=do_sample, temperature=0.8, top_k=30, top_p=0.8,
                                       repetition_penalty=10.0, length_penalty=0.0, exp_noise=noise, use_graph=use_graph)
                got = out[:, fake.shape[1]:].cpu().numpy()
                assert got.shape == want.shape, (got.shape, want.shape)
                rows = np.nonzero((got != want).any(axis=1))[0]
                assert len(rows) <= 1, f"{len(rows)} of {B} utterances differ (do_sample={do_sample}, graph={use_graph})"
                for b in rows:
                    t = int(np.nonzero(got[b] != want[b])[0][0])
                    gaps = [float(tr[3][b]) for tr in trace[: t + 1]]
                    assert min(gaps) <= bc.KV_GAP, f"utterance {b} differs from step {t} on; the oracle's closest decision: {min(gaps):.3e}"
    finally:
        _lib.set_gemm_mode(_lib.GEMM_BF16X3)
