"""GPU: the multinomial sampler (`warp_row_token` under `sample_warp_kernel` and `sample_slots_warp_kernel`, csrc/decode.hip), the
greedy argmax (`greedy_row_argmax`) and the counter-based draws (`exp1_draw`, csrc/decode.h) against the float64 reference and the
restated draws of tests/sampler_cases.py -- at real vocabulary sizes (up to 16 slices of 1024 ids per workgroup, a partial last
slice), on crafted rows with ties and boundary cases, with seeded draws, and as a distribution.

Every case runs generate() (eager, with the logits the reference then works on, and through the replayed graph) and a sampled decode
session of 4 slots with staggered admission (eager and replayed).  A session request equals row 0 of generate() on 4 copies of its
prompt, so its reference works on that row's logits for as long as the two have produced the same codes.  What "equal" means, the
crafted-row harness and the cap on undecidable steps: tests/sampler_cases.py; tests/test_sampler_cases_cpu.py checks that the
reference alone keeps every case here within the cap.  Each test prints its counts (-s shows them)."""
import numpy as np
import pytest
import torch

import sampler_cases as sc

pytestmark = pytest.mark.gpu

_MODELS = {}


def _natural_model(device, V):
    """One natural model per vocabulary for the whole module."""
    from indextts_amd.gpt import UnifiedVoice
    if V not in _MODELS:
        _MODELS[V] = UnifiedVoice(sc.natural_weights(V), sc.config(V), device=device)
    return _MODELS[V]


def _crafted_model(device, bias, max_mel_tokens=40):
    from indextts_amd.gpt import UnifiedVoice
    return UnifiedVoice(sc.crafted_weights(bias, max_mel_tokens), sc.config(bias.size, max_mel_tokens), device=device)


def _kw(samp):
    if samp["sampler"] == "greedy":
        return {}
    return dict(do_sample=True, sampler=samp["sampler"], temperature=samp["temperature"], top_k=samp.get("top_k", 0),
                top_p=samp.get("top_p", 1.0))


def _generate(uv, fake, emb, n, samp, penalty, noise=None, seed=None, logits=True, graph=False, forced=None):
    """codes [B, steps] (and logits [B, steps, V]) of generate() as numpy."""
    out = uv.generate(fake, max_new_tokens=n, tts_embeddings=emb, repetition_penalty=penalty, return_logits=logits, use_graph=graph,
                      exp_noise=None if noise is None else torch.from_numpy(noise), seed=seed, forced_codes=forced, **_kw(samp))
    P1 = fake.shape[1]
    if logits:
        return out[0][:, P1:].cpu().numpy(), out[1].cpu().numpy()
    return out[:, P1:].cpu().numpy()


def _copies(uv, row, B):
    """generate()'s inputs for B copies of one prompt row [P, d]."""
    P, d = row.shape
    fake = torch.ones(B, P + 1, dtype=torch.long)
    fake[:, -1] = uv.cfg.start_mel_token
    return fake, row[None].expand(B, P, d).contiguous()


def _assert_logits_are_bias(logits, bias):
    """The crafted-row harness's own precondition: a zero head weight makes every row's logits the bias, bit for bit."""
    want = np.broadcast_to(bias.view(np.uint32), logits.shape)
    assert np.array_equal(np.ascontiguousarray(logits).view(np.uint32), want), \
        "harness precondition failed: with a zero mel_head.weight the returned logits are not mel_head.bias bit for bit"


def _check_generate(codes, logits, draws, samp, penalty, cfg, tally, what):
    V = cfg.number_mel_codes
    for b in range(codes.shape[0]):
        sc.check_row(codes[b], lambda t: logits[b, t], lambda t: draws(t, b), samp, penalty, V, cfg.start_mel_token, cfg.stop_mel_token,
                     tally, f"{what} row {b}")


def _session(uv, rows, caps, samplings, penalty, use_graph, slots=sc.NAT_SLOTS, stagger=3, sampled=True):
    """Request 0 enters slot 0 at once, the others `stagger` steps later (slots 1, 2, ...: nothing is taken before the end).
    Returns the codes per request and the slots they had."""
    sess = uv.decode_session(slots, max_prompt=max(r.shape[0] for r in rows), max_new=max(caps), repetition_penalty=penalty,
                             use_graph=use_graph, sampled=sampled)
    done = set()
    ids = sess.admit(rows[:1], caps[:1], sampling=samplings[:1] if sampled else None)
    done.update(sess.step(stagger))
    if len(rows) > 1:
        ids += sess.admit(rows[1:], caps[1:], sampling=samplings[1:] if sampled else None)
    guard = 0
    while len(done) < len(rows):
        done.update(sess.step(4))
        guard += 1
        assert guard < 100
    out = [sess.take(s).cpu().numpy() for s in ids]
    sess.close()
    assert ids == list(range(len(rows)))
    return out, ids


def _session_sampling(samp, noise=None, seed=None):
    s = {k: v for k, v in samp.items() if k in ("sampler", "temperature", "top_k", "top_p")}
    if noise is not None:
        s["exp_noise"] = torch.from_numpy(np.ascontiguousarray(noise))
    elif seed is not None:
        s["seed"] = seed
    return s


def _check_session_vs_row0(codes, gen_codes0, gen_logits0, draws, samp, penalty, cfg, tally, what):
    """A session request against the reference on row 0 of generate() on `slots` copies of its prompt: those logits are this
    request's for as long as both have produced the same codes."""
    def logits_of(t):
        if t >= gen_logits0.shape[0] or not np.array_equal(codes[:t], gen_codes0[:t]):
            return None
        return gen_logits0[t]
    return sc.check_row(codes, logits_of, draws, samp, penalty, cfg.number_mel_codes, cfg.start_mel_token, cfg.stop_mel_token, tally, what)


def _natural_case(device, V, samp, penalty, n, widths, tag, tally, noise_of=None, seed=None, prompt_tag="t/sampler/prompt"):
    """Two requests.  Each: generate() on 4 copies of its prompt with its own draws per row (eager with logits, then replayed), every
    row against the reference; then both in a session (eager, replayed), each against row 0 of its generate()."""
    uv = _natural_model(device, V)
    cfg = uv.cfg
    B = sc.NAT_SLOTS
    conds, texts = sc.prompts(V, widths, tag=prompt_tag)
    rows = [uv.prompt_rows(conds[r:r + 1].to(device), texts[r])[0] for r in range(2)]
    gens, samplings, sdraws = [], [], []
    for r in range(2):
        fake, emb = _copies(uv, rows[r], B)
        if seed is None:
            q = noise_of(r)
            draws = lambda t, b, q=q: q[t, b]      # noqa: E731
            samplings.append(_session_sampling(samp, noise=q[:, 0]))
            sdraws.append(lambda t, q=q: q[t, 0])
        else:
            q = None
            draws = lambda t, b: sc.generate_draws(seed, t, b, B, V)      # noqa: E731
            samplings.append(_session_sampling(samp, seed=seed))
            sdraws.append(lambda t: sc.session_draws(seed, t, B, V))
        codes, logits = _generate(uv, fake, emb, n, samp, penalty, noise=q, seed=seed)
        _check_generate(codes, logits, draws, samp, penalty, cfg, tally, f"{tag} generate request {r}")
        replay = _generate(uv, fake, emb, n, samp, penalty, noise=q, seed=seed, logits=False, graph=True)
        assert np.array_equal(replay[:, :codes.shape[1]], codes), f"{tag} request {r}: the replayed graph gives other codes"
        gens.append((codes[0], logits[0]))
    for use_graph in (False, True):
        out, ids = _session(uv, rows, [n, n], samplings, penalty, use_graph)
        for r in range(2):
            walked = _check_session_vs_row0(out[r], gens[r][0], gens[r][1], sdraws[r], samp, penalty, cfg, tally,
                                            f"{tag} session(graph={use_graph}) request {r} in slot {ids[r]}")
            assert walked >= 1


# ---- vocabulary edges: natural logits, explicit draws ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.NATURAL_SAMPLERS))
@pytest.mark.parametrize("V", sc.VOCABS)
def test_vocabulary_edges(device, V, name):
    samp = sc.NATURAL_SAMPLERS[name]
    tally = sc.Tally()
    _natural_case(device, V, samp, sc.NAT_PENALTY, sc.NAT_STEPS, sc.NAT_WIDTHS, f"V={V} {name}", tally,
                  noise_of=lambda r: sc.noise(sc.nat_noise_seed(V, name, r), (sc.NAT_STEPS, sc.NAT_SLOTS, V)))
    print(f"vocabulary_edges[{V}, {name}]: {tally}")
    assert tally.checked >= 2 * sc.NAT_SLOTS * sc.NAT_STEPS // 2 and tally.within_cap(), tally


def test_vocabulary_above_the_limit_is_refused(device):
    """V = 16385 = 1024 * 16 + 1: the sampler refuses it by name; a greedy call on that model and a sampled call at 16384 still work."""
    from indextts_amd.gpt import UnifiedVoice
    V = 16385
    uv = UnifiedVoice(sc.natural_weights(V), sc.config(V), device=device)
    conds, texts = sc.prompts(V, (5,))
    fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), texts[0])
    samp = sc.NATURAL_SAMPLERS["hf_0.8_30_0.8"]
    with pytest.raises(RuntimeError, match="vocabulary size"):
        _generate(uv, fake, emb, 4, samp, 10.0, seed=1, logits=False)
    codes, logits = _generate(uv, fake, emb, 4, {"sampler": "greedy"}, 10.0)
    seen = np.zeros(V, bool)
    seen[1] = seen[V - 2] = True
    assert codes.shape == (1, 4)
    for t in range(4):      # the greedy walk on its own logits (a natural row: the two best penalised logits are not within rounding)
        assert codes[0, t] == sc.ref_greedy(logits[0, t], seen, 10.0), t
        seen[codes[0, t]] = True
    ok = _natural_model(device, 16384)
    conds, texts = sc.prompts(16384, (5,))
    fake, emb, _ = ok.prepare_gpt_inputs(conds.to(device), texts[0])
    tally = sc.Tally()
    codes, logits = _generate(ok, fake, emb, 4, samp, 10.0, seed=1)
    _check_generate(codes, logits, lambda t, b: sc.generate_draws(1, t, b, 1, 16384), samp, 10.0, ok.cfg, tally, "after the refusal")
    assert tally.checked >= 1 and tally.excused == 0


# ---- crafted rows: top-k, top-p, the penalty --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.crafted_cases()))
def test_crafted_rows(device, name):
    c = sc.crafted_cases()[name]
    bias, samp, penalty = c["bias"], c["samp"], c["penalty"]
    V, B, n = bias.size, sc.CRAFTED_ROWS, sc.CRAFTED_STEPS
    uv = _crafted_model(device, bias)
    cfg = uv.cfg
    q = sc.probe_noise(sc.noise(sc.CRAFTED_NOISE_SEED, (n, B, V)), c["probe"])
    conds, texts = sc.prompts(V, (6,) * B)
    fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
    tally = sc.Tally()
    codes, logits = _generate(uv, fake, emb, n, samp, penalty, noise=q)
    _assert_logits_are_bias(logits, bias)
    _check_generate(codes, logits, lambda t, b: q[t, b], samp, penalty, cfg, tally, f"{name} generate")
    replay = _generate(uv, fake, emb, n, samp, penalty, noise=q, logits=False, graph=True)
    assert np.array_equal(replay[:, :codes.shape[1]], codes), "the replayed graph gives other codes"
    if name == "topk1":      # whatever the noise: the greedy walk
        for b in range(B):
            assert codes[b].tolist() == sc.simulate_greedy(bias, penalty, n)
    rows = [uv.prompt_rows(conds[r:r + 1].to(device), texts[r])[0] for r in range(2)]
    for use_graph in (False, True):
        out, ids = _session(uv, rows, [n, n], [_session_sampling(samp, noise=q[:, r]) for r in range(2)], penalty, use_graph)
        for r in range(2):
            sc.check_row(out[r], lambda t: bias, lambda t: q[t, r], samp, penalty, V, cfg.start_mel_token, cfg.stop_mel_token, tally,
                         f"{name} session(graph={use_graph}) slot {ids[r]}")
    print(f"crafted_rows[{name}]: {tally}")
    assert tally.checked >= 4 * n and tally.within_cap(), tally


# ---- greedy ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8194, 258])
def test_greedy_ties(device, V):
    """Equal maxima at a high id (slice 7 at V = 8194) and at a low id in another wave: the lower id wins, again after the penalty
    has demoted each winner -- generate(), forced codes, a greedy session and the greedy rows of a sampled session."""
    bias = sc.greedy_tie_bias(V)
    uv = _crafted_model(device, bias)
    n, penalty = 8, 2.0
    want = sc.simulate_greedy(bias, penalty, n)
    conds, texts = sc.prompts(V, (6, 6))
    fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
    greedy = {"sampler": "greedy"}
    codes, logits = _generate(uv, fake, emb, n, greedy, penalty)
    _assert_logits_are_bias(logits, bias)
    assert codes[0].tolist() == want and codes[1].tolist() == want
    assert _generate(uv, fake, emb, n, greedy, penalty, logits=False, graph=True).tolist() == [want, want]
    # forced codes: the recorded codes are each step's own argmax, the penalty set follows the forced tokens (row 0: the tie ids in
    # another order; row 1: ids outside the tiers, so the first maximum stays)
    tiers = [int(v) for v in np.nonzero(bias >= 7.0)[0]]
    forced = np.array([tiers[::-1][:n], [5, 6, 7, 8, 9, 10, 11, 12][:n]])
    fcodes, flogits = _generate(uv, fake, emb, n, greedy, penalty, forced=torch.from_numpy(forced))
    _assert_logits_are_bias(flogits, bias)
    for b in range(2):
        assert fcodes[b].tolist() == sc.simulate_greedy(bias, penalty, n, forced=forced[b]), b
    assert fcodes[1].tolist() == [want[0]] * n
    rows = [uv.prompt_rows(conds[r:r + 1].to(device), texts[r])[0] for r in range(2)]
    for use_graph in (False, True):
        out, _ = _session(uv, rows, [n, n], None, penalty, use_graph, sampled=False)
        assert [o.tolist() for o in out] == [want, want], f"greedy session(graph={use_graph})"
        out, _ = _session(uv, rows, [n, n], [greedy, greedy], penalty, use_graph)
        assert [o.tolist() for o in out] == [want, want], f"greedy rows of a sampled session(graph={use_graph})"
    print(f"greedy_ties[{V}]: {(2 + 2 + 2 + 8) * n} steps checked, 0 excused (every comparison is exact)")


# ---- seeded draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sc.SEEDS)
def test_seeded_draws(device, seed):
    """No exp_noise: the draws are exp1_draw(seed, (step * B + b) * V + v) in generate() and exp1_draw(seed, (t * slots) * V + v) for a
    session request at its own step t, in whichever slot and whenever admitted."""
    V = sc.SEEDED_V
    uv = _natural_model(device, V)
    B, n = sc.SEEDED_ROWS, sc.NAT_STEPS
    conds, texts = sc.prompts(V, (sc.SEEDED_WIDTH,) * B, tag="t/sampler/seeded")
    fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
    for name in sc.SEEDED_SAMPLERS:
        samp = sc.NATURAL_SAMPLERS[name]
        tally = sc.Tally()
        codes, logits = _generate(uv, fake, emb, n, samp, sc.NAT_PENALTY, seed=seed)
        _check_generate(codes, logits, lambda t, b: sc.generate_draws(seed, t, b, B, V), samp, sc.NAT_PENALTY, uv.cfg, tally,
                        f"seed {seed} {name} generate on {B} rows")
        replay = _generate(uv, fake, emb, n, samp, sc.NAT_PENALTY, seed=seed, logits=False, graph=True)
        assert np.array_equal(replay[:, :codes.shape[1]], codes)
        assert len({tuple(r) for r in codes}) == B, "rows share their draws"
        _natural_case(device, V, samp, sc.NAT_PENALTY, n, (sc.SEEDED_WIDTH,) * 2, f"seed {seed} {name}", tally, seed=seed,
                      prompt_tag="t/sampler/seeded")
        print(f"seeded_draws[{seed}, {name}]: {tally}")
        assert tally.checked >= (B + 4) * n // 2 and tally.within_cap(), tally


def test_seeded_draw_of_all_ones_is_small_not_zero(device):
    """The seed under which one element draws h = 2^24 - 1: u would round to 1 in fp32 and the draw to 0, p / q = inf: that id
    taken whatever its probability.  Bounded at 1 - 2^-24 the draw is 6e-8: an id of ordinary probability is still taken, one
    whose probability is e^-40 of the others' is not."""
    V, B, v = 258, 3, 17
    samp = {"sampler": "hf", "temperature": 1.0, "top_k": 0, "top_p": 1.0}
    conds, texts = sc.prompts(V, (6,) * B)
    tally = sc.Tally()
    for likely in (True, False):
        bias = sc._row(V, 15, -3.0, 0.0)
        if not likely:
            bias[v] = -40.0
        uv = _crafted_model(device, bias)
        fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
        for b, t in ((1, 0), (2, 3)):
            seed = sc.seed_for_bits(2 ** 24 - 1, (t * B + b) * V + v)
            codes, logits = _generate(uv, fake, emb, 6, samp, 1.0, seed=seed)
            _assert_logits_are_bias(logits, bias)
            assert (codes[b, t] == v) == likely, (likely, b, t, codes[b, t])
            _check_generate(codes, logits, lambda t, b: sc.generate_draws(seed, t, b, B, V), samp, 1.0, uv.cfg, tally, "extreme draw")
        rows = [uv.prompt_rows(conds[r:r + 1].to(device), texts[r])[0] for r in range(2)]
        seed = sc.seed_for_bits(2 ** 24 - 1, (2 * sc.NAT_SLOTS) * V + v)
        out, _ = _session(uv, rows, [6, 6], [_session_sampling(samp, seed=seed)] * 2, 1.0, True)
        for r in range(2):
            assert (out[r][2] == v) == likely, (likely, r, out[r])
            sc.check_row(out[r], lambda t: bias, lambda t: sc.session_draws(seed, t, sc.NAT_SLOTS, V), samp, 1.0, V, V - 2, V - 1, tally,
                         "extreme draw, session")
    print(f"seeded_draw_of_all_ones: {tally}")
    assert tally.checked >= 48 and tally.within_cap()


# ---- the distribution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.DIST_CASES))
def test_distribution(device, name):
    """64 rows x 100 steps of one crafted row, seeded, penalty 1: 6400 draws from one known distribution.  Pearson's chi-square over
    the tokens (cells with an expected count below 5 pooled) against the 1 - 1e-6 quantile of the chi-square law for that number of
    degrees of freedom; no two rows equal; and every token the reference's on the restated draws.
    The reference on the restated draws (tests/test_sampler_cases_cpu.py, the same seeds) gives: full 116.1 on 137 degrees of
    freedom against 230.5; T0.5_k8 3.1 on 7 against 40.5."""
    samp, seed = sc.DIST_CASES[name]
    bias = sc.dist_bias()
    V, B, n = sc.DIST_V, sc.DIST_B, sc.DIST_STEPS
    uv = _crafted_model(device, bias, max_mel_tokens=120)
    conds, texts = sc.prompts(V, (6,) * B)
    fake, emb, _ = uv.prepare_gpt_inputs(conds.to(device), torch.cat(texts))
    codes, logits = _generate(uv, fake, emb, n, samp, 1.0, seed=seed)
    assert codes.shape == (B, n)
    _assert_logits_are_bias(logits, bias)
    stat, dof = sc.chi_square(codes, sc.dist_probs(samp))
    bound = sc.chi2_quantile(dof)
    tally = sc.Tally()
    _check_generate(codes, logits, lambda t, b: sc.generate_draws(seed, t, b, B, V), samp, 1.0, uv.cfg, tally, name)
    print(f"distribution[{name}]: chi-square {stat:.1f} on {dof} degrees of freedom, bound {bound:.1f}; {tally}")
    assert stat <= bound
    assert len({tuple(r) for r in codes}) == B, "two rows drew the same sequence"
    assert tally.checked == B * n and tally.within_cap(), tally
    assert np.array_equal(_generate(uv, fake, emb, n, samp, 1.0, seed=seed, logits=False, graph=True), codes)


# ---- more survivors than the top-p stage can hold, without top-p ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.overflow_cases()))
def test_survivor_overflow(device, name):
    """top_k = 2100 on natural logits, and 3000 equal top scores under top_k = 30, both with top_p = 1: more than the 2048 entries
    the top-p stage can sort.  Without top-p nothing is sorted, so the tokens are the reference's, and the same in every run."""
    c = sc.overflow_cases()[name]
    samp, penalty = c["samp"], c["penalty"]
    V, B, n = sc.OVERFLOW_V, sc.CRAFTED_ROWS, sc.OVERFLOW_STEPS
    uv = _natural_model(device, V) if c["bias"] is None else _crafted_model(device, c["bias"])
    q = sc.overflow_noise(B)
    conds, texts = sc.prompts(V, sc.NAT_WIDTHS)
    row = uv.prompt_rows(conds[:1].to(device), texts[0])[0]
    fake, emb = _copies(uv, row, B)
    tally = sc.Tally()
    codes, logits = _generate(uv, fake, emb, n, samp, penalty, noise=q)
    if c["bias"] is not None:
        _assert_logits_are_bias(logits, c["bias"])
    again = _generate(uv, fake, emb, n, samp, penalty, noise=q, logits=False)
    replay = _generate(uv, fake, emb, n, samp, penalty, noise=q, logits=False, graph=True)
    _check_generate(codes, logits, lambda t, b: q[t, b], samp, penalty, uv.cfg, tally, f"{name} generate")
    assert np.array_equal(again[:, :codes.shape[1]], codes) and np.array_equal(replay[:, :codes.shape[1]], codes), "two runs differ"
    # sessions of 3 slots: a request equals row 0 of the 3 copies above
    outs = []
    for use_graph in (False, True):
        out, ids = _session(uv, [row, row], [n, n], [_session_sampling(samp, noise=q[:, 0])] * 2, penalty, use_graph, slots=B, stagger=1)
        for r in range(2):
            _check_session_vs_row0(out[r], codes[0], logits[0], lambda t: q[t, 0], samp, penalty, uv.cfg, tally,
                                   f"{name} session(graph={use_graph}) slot {ids[r]}")
        outs.append([o.tolist() for o in out])
    assert outs[0] == outs[1] and outs[0][0] == outs[0][1], "two session runs differ"
    print(f"survivor_overflow[{name}]: {tally}")
    assert tally.checked >= B * n and tally.within_cap(), tally
