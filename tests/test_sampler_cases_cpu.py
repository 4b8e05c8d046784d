"""CPU: what tests/test_sampler_gpu.py rests on (tests/sampler_cases.py) -- the float64 reference sampler against the oracle's
warpers, the restated Exp(1) draws, and, for every case of the GPU file, that the reference alone keeps the undecidable steps
within the cap (the seeds and rows were chosen for that; crafted rows also have to meet the margins their comments promise)."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
from oracle import gpt as og


def _oracle_token(logits, seen, q, samp, penalty):
    """oracle.gpt's fp32 path: repetition penalty -> warp_scores -> softmax -> argmax(probs / q), or the accel form."""
    lg = torch.from_numpy(np.asarray(logits, np.float32))[None]
    qt = torch.from_numpy(np.asarray(q, np.float32))[None]
    if samp["sampler"] == "accel":
        return int((torch.softmax(lg / samp["temperature"], -1) / qt.clamp_min(1e-10)).argmax(-1))
    ids = torch.from_numpy(np.nonzero(seen)[0])[None]
    s = og.repetition_penalty(ids, lg, penalty) if penalty != 1.0 else lg
    s = og.warp_scores(s, samp["temperature"], samp.get("top_k", 0), samp.get("top_p", 1.0))
    return int((torch.softmax(s, -1) / qt).argmax(-1))


def test_reference_agrees_with_oracle_on_crafted_rows():
    """Every crafted case, its own probed draws, 10 steps of the reference's own walk: the oracle's fp32 token on every decidable
    step (crafted scores are exact in fp32 too; top_p cases have no cut inside a tie group, so torch.sort's order does not matter)."""
    n = 0
    for name, c in sc.crafted_cases().items():
        V = c["bias"].size
        q = sc.probe_noise(sc.noise(11, (10, 1, V)), c["probe"])
        seen = np.zeros(V, bool)
        seen[1] = seen[V - 2] = True
        for t in range(10):
            st = sc.ref_step(c["bias"], seen, q[t, 0], c["samp"], c["penalty"])
            if st.decidable:
                assert st.token == _oracle_token(c["bias"], seen, q[t, 0], c["samp"], c["penalty"]), (name, t)
                n += 1
            seen[st.token] = True
    assert n >= 9 * len(sc.crafted_cases())


@pytest.mark.parametrize("V", [1025, 8194])
@pytest.mark.parametrize("name", sorted(sc.NATURAL_SAMPLERS))
def test_reference_agrees_with_oracle_on_random_logits(V, name):
    samp = sc.NATURAL_SAMPLERS[name]
    rng = np.random.default_rng(V)
    decided = 0
    for t in range(24):
        logits = (rng.standard_normal(V) * 2.0).astype(np.float32)
        seen = rng.random(V) < 0.01
        q = sc.noise(100 + t, (V,))
        st = sc.ref_step(logits, seen, q, samp, 10.0)
        if st.decidable:
            assert st.token == _oracle_token(logits, seen, q, samp, 10.0), t
            decided += 1
    assert decided >= 22


def test_reference_filters():
    """The reference on rows small enough to check by hand."""
    l = np.array([0.0, 1.0, 2.0, 2.0, 3.0, -1.0], np.float32)
    none = np.zeros(6, bool)
    q = np.ones(6, np.float32)
    hf = lambda k, p, T=1.0: {"sampler": "hf", "temperature": T, "top_k": k, "top_p": p}      # noqa: E731
    assert sc.ref_step(l, none, q, hf(2, 1.0), 1.0).keep.tolist() == [False, False, True, True, True, False]      # ties kept
    assert sc.ref_step(l, none, q, hf(6, 1.0), 1.0).keep.all() and sc.ref_step(l, none, q, hf(13, 1.0), 1.0).keep.all()
    assert sc.ref_step(l, none, q, hf(5, 1.0), 1.0).keep.tolist() == [True] * 5 + [False]
    # ascending (-1, 0, 1, 2, 2, 3): p = .0094 .0257 .0698 .1897 .1897 .5158, running sums .0094 .0351 .1049 ...
    st = sc.ref_step(l, none, q, hf(6, 0.9), 1.0)
    assert st.keep.tolist() == [False, True, True, True, True, False] and abs(st.margins["top_p"] - (0.1049 - 0.1) / 0.1) < 5e-3
    assert sc.ref_step(l, none, q, hf(6, 1e-6), 1.0).keep.tolist() == [False, False, False, False, True, False]      # the last stays
    # penalty 2: seen ids 4 (3 -> 1.5), 5 (-1 -> -2), 0 (0 stays 0); the argmax with equal draws moves to the first 2.0
    seen = np.array([1, 0, 0, 0, 1, 1], bool)
    st = sc.ref_step(l, seen, q, hf(0, 1.0), 2.0)
    assert st.token == 2 and not st.decidable and st.accept.tolist() == [False, False, True, True, False, False]
    assert sc.ref_greedy(l, seen, 2.0) == 2 and sc.ref_greedy(l, none, 2.0) == 4
    # a small draw wins: p / q
    q2 = q.copy()
    q2[0] = 1e-3
    assert sc.ref_step(l, none, q2, hf(0, 1.0), 1.0).token == 0 and sc.ref_step(l, none, q2, hf(3, 1.0), 1.0).token == 4
    acc = sc.ref_step(l, seen, q2, {"sampler": "accel", "temperature": 0.5}, 2.0)      # no penalty, no filter
    assert acc.token == 0 and acc.keep.all()


def test_draw_restatement_is_the_scalar_definition():
    import math
    for seed, idx in ((0, 0), (1, 8193), (2 ** 63 + 5, (99 * 4 + 3) * 16384 + 16383), (2 ** 64 - 1, 12345678901)):
        z = (seed + sc._GOLD * (idx + 1)) & sc.MASK
        z = ((z ^ (z >> 30)) * sc._M1) & sc.MASK
        z = ((z ^ (z >> 27)) * sc._M2) & sc.MASK
        z ^= z >> 31
        h = z >> 40
        assert int(sc.draw_bits(seed, [idx])[0]) == h
        u = float(np.float32(h) + np.float32(0.5)) / 2.0 ** 24
        assert abs(float(sc.exp1(seed, [idx])[0]) + math.log(min(u, 1.0 - 2.0 ** -24))) <= 1e-7 * max(1.0, -math.log(u))
    # the index rules: row b of step t of a B-row generation; a session slot is row 0 of a `slots`-row generation
    V = 1025
    assert np.array_equal(sc.generate_draws(7, 3, 2, 5, V), sc.exp1(7, np.arange((3 * 5 + 2) * V, (3 * 5 + 2) * V + V)))
    assert np.array_equal(sc.session_draws(7, 3, 4, V), sc.generate_draws(7, 3, 0, 4, V))
    assert not np.array_equal(sc.generate_draws(7, 3, 2, 5, V), sc.generate_draws(7, 2, 2, 5, V))


def test_draw_extremes_stay_in_the_open_interval():
    """h = 2^24 - 1 would round to u = 1 in fp32 (a draw of 0): the bound 1 - 2^-24 keeps every draw positive and finite; and the
    inverse of the finaliser that the GPU test uses to place such a draw."""
    for h, idx in ((2 ** 24 - 1, 0), (0, 17), (2 ** 24 - 1, 5 * 258 + 17), (2 ** 23, 3)):
        seed = sc.seed_for_bits(h, idx)
        assert int(sc.draw_bits(seed, [idx])[0]) == h
    q = sc.exp1(sc.seed_for_bits(2 ** 24 - 1, 9), [9])[0]
    assert 5.9e-8 < q < 6.0e-8
    q = sc.exp1(sc.seed_for_bits(0, 9), [9])[0]
    assert abs(q - 25 * np.log(2.0)) < 1e-5


def test_draws_are_exp1():
    """10^6 restated draws: mean 1 (standard error 1e-3), variance 1 (the fourth central moment of Exp(1) is 9: standard error
    sqrt(8e-6) = 2.83e-3), at 5 standard errors; the 24-bit grid moves either by less than 1e-6.  Also P(q > 1) = 1 / e (binomial
    standard error 4.8e-4) and independence between neighbouring ids, rows and steps (a correlation has standard error 1e-3)."""
    n = 10 ** 6
    for seed in sc.SEEDS:
        q = sc.exp1(seed, np.arange(n, dtype=np.uint64)).astype(np.float64)
        assert (q > 0).all() and np.isfinite(q).all()
        assert abs(q.mean() - 1.0) <= 5e-3
        assert abs(q.var() - 1.0) <= 5 * 2.83e-3
        assert abs((q > 1.0).mean() - np.exp(-1.0)) <= 5 * 4.8e-4
        for lag in (1, 258, 8194, 4 * 8194):
            assert abs(np.corrcoef(q[:-lag], q[lag:])[0, 1]) <= 5e-3, (seed, lag)
    a = sc.exp1(0, np.arange(n, dtype=np.uint64)).astype(np.float64)
    b = sc.exp1(1, np.arange(n, dtype=np.uint64)).astype(np.float64)
    assert abs(np.corrcoef(a, b)[0, 1]) <= 5e-3


@pytest.mark.parametrize("name", sorted(sc.crafted_cases()))
def test_crafted_case_is_decidable(name):
    """The reference's own walk of every crafted case (3 rows, 12 steps, the GPU test's draws): within the cap; the top-p cases
    keep their running sums at least 1e-3 (relative to 1 - top_p) away from the cut."""
    c = sc.crafted_cases()[name]
    V = c["bias"].size
    q = sc.probe_noise(sc.noise(sc.CRAFTED_NOISE_SEED, (sc.CRAFTED_STEPS, sc.CRAFTED_ROWS, V)), c["probe"])
    tally = sc.Tally()
    for b in range(sc.CRAFTED_ROWS):
        sc.simulate(c["bias"], lambda t: q[t, b], c["samp"], c["penalty"], sc.CRAFTED_STEPS, tally)
    assert tally.within_cap() and tally.checked >= 2 * sc.CRAFTED_STEPS, tally
    if c["samp"]["top_p"] < 1.0:
        seen = np.zeros(V, bool)
        st = sc.ref_step(c["bias"], seen, q[0, 0], c["samp"], 1.0)
        assert st.margins["top_p"] >= 1e-3, st.margins


def test_crafted_cases_do_what_their_names_say():
    cs = sc.crafted_cases()
    none = lambda V: np.zeros(V, bool)      # noqa: E731

    def kept(name):
        c = cs[name]
        return set(np.nonzero(sc.ref_step(c["bias"], none(c["bias"].size), np.ones(c["bias"].size, np.float32), c["samp"], 1.0).keep)[0])

    assert kept("topk12") == set(sc.SPREAD) and len({v >> 10 for v in sc.SPREAD}) >= 6
    assert kept("topk5_T2") == set(sc.SPREAD[7:])
    assert len(kept("topk8_ties5")) == 12
    assert len(kept("topk_Vm1")) == 2049 and 1500 not in kept("topk_Vm1")
    assert len(kept("topk_V")) == 2050 and len(kept("topk_Vp7")) == 2050
    assert len(kept("topk1")) == 1
    assert kept("topp_only_largest") == {5000}
    assert len(kept("topp_nothing")) == 8
    assert kept("topp_ties_above") == {sc.SPREAD[4], sc.SPREAD[7], sc.SPREAD[10], sc.SPREAD[9], sc.SPREAD[1]}
    assert kept("topp_ties_below") == {sc.SPREAD[9], sc.SPREAD[1]}
    assert kept("topp_threshold_ties_below") == {1024, 3, 4097, 2048}
    # the penalty cases: the kept set moves from step to step
    c = cs["penalty_moves_topk"]
    q = sc.probe_noise(sc.noise(sc.CRAFTED_NOISE_SEED, (sc.CRAFTED_STEPS, 1, 8194)), c["probe"])
    seen = none(8194)
    seen[1] = seen[8192] = True
    sets = []
    for t in range(6):
        st = sc.ref_step(c["bias"], seen, q[t, 0], c["samp"], c["penalty"])
        sets.append(frozenset(np.nonzero(st.keep)[0]))
        seen[st.token] = True
    assert len(set(sets)) >= 5
    # the overflow rows: more survivors than the 2048 the top-p stage can hold
    assert (sc.overflow_tie_bias() == sc.overflow_tie_bias().max()).sum() == 3000


@pytest.mark.parametrize("V", [8194, 258])
def test_greedy_tie_rows(V):
    b = sc.greedy_tie_bias(V)
    toks = sc.simulate_greedy(b, 2.0, 8)
    mx = np.nonzero(b == b.max())[0]
    assert toks[0] == mx.min() and toks[1] == mx.max() and len(set(toks)) == 8
    assert toks[0] < toks[1] and toks[2] < toks[3] and toks[4] < toks[5] and toks[6] < toks[7]
    if V == 8194:
        assert toks[1] >> 10 == 7 and toks[0] >> 6 != 0


@pytest.mark.parametrize("name", sorted(sc.DIST_CASES))
def test_distribution_case_on_the_cpu(name):
    """The chi-square test of the GPU file on the reference fed the restated draws: the seed's statistic lies below the bound, every
    draw is decidable within the cap, and no two rows are equal.  A wrong index rule is caught: rows that share draws are equal."""
    samp, seed = sc.DIST_CASES[name]
    toks, undecided = sc.dist_simulate(samp, seed)
    assert undecided <= sc.CAP * toks.size
    stat, dof = sc.chi_square(toks, sc.dist_probs(samp))
    bound = sc.chi2_quantile(dof)
    print(f"{name}: chi-square {stat:.1f} on {dof} degrees of freedom, bound {bound:.1f}, {undecided} undecidable of {toks.size}")
    assert stat <= bound
    assert len({tuple(r) for r in toks}) == sc.DIST_B
    # the bound has teeth: the same number of draws from the distribution at another temperature fails it
    other = dict(samp, temperature=samp["temperature"] * 1.25)
    rng = np.random.default_rng(1)
    wrong = rng.choice(sc.DIST_V, size=toks.size, p=sc.dist_probs(other))
    keep = sc.dist_probs(samp)[wrong] > 0
    assert sc.chi_square(wrong[keep], sc.dist_probs(samp))[0] > bound


def test_chi2_quantile():
    """Even degrees of freedom have a closed survival function, exp(-x / 2) * sum_{j < dof / 2} (x / 2)^j / j!: the quantile's must be
    the tail it was asked for."""
    import math
    assert abs(sc.chi2_quantile(2) - 2 * np.log(1e6)) < 1e-6
    for dof in (2, 8, 14, 60, 200):
        x = sc.chi2_quantile(dof) / 2
        tail = math.exp(-x) * sum(x ** j / math.factorial(j) for j in range(dof // 2))
        assert abs(tail - 1e-6) < 1e-11, dof
    assert sc.chi2_quantile(13) < sc.chi2_quantile(14) < sc.chi2_quantile(15)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_natural_cases_stay_within_the_cap(V):
    """The reference on the oracle's fp32 logits of the natural model (what the GPU computes up to rounding), every sampler of
    the vocabulary-edge cases with the GPU test's explicit draws: the undecidable steps stay within the cap."""
    cfg = sc.config(V)
    w = {k: torch.from_numpy(v) for k, v in sc.natural_weights(V).items()}
    conds, texts = sc.prompts(V, sc.NAT_WIDTHS)
    B, n = sc.NAT_SLOTS, sc.NAT_STEPS
    for name, samp in sc.NATURAL_SAMPLERS.items():
        tally = sc.Tally()
        for r, text in enumerate(texts):
            q = sc.noise(sc.nat_noise_seed(V, name, r), (n, B, V))
            _oracle_walk(w, cfg, conds[r:r + 1].expand(B, -1, -1), text.expand(B, -1), n, lambda t, b: q[t, b], samp, tally)
        assert tally.within_cap() and tally.checked >= B * n, (name, tally)


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_seeded_cases_stay_within_the_cap(seed):
    """The same for the seeded cases: generate() on 5 different rows, and on 4 copies of a prompt (what a session slot equals)."""
    V = sc.SEEDED_V
    cfg = sc.config(V)
    w = {k: torch.from_numpy(v) for k, v in sc.natural_weights(V).items()}
    conds, texts = sc.prompts(V, (sc.SEEDED_WIDTH,) * sc.SEEDED_ROWS, tag="t/sampler/seeded")
    n = sc.NAT_STEPS
    for name in sc.SEEDED_SAMPLERS:
        samp = sc.NATURAL_SAMPLERS[name]
        tally = sc.Tally()
        B = sc.SEEDED_ROWS
        _oracle_walk(w, cfg, conds, torch.cat(texts), n, lambda t, b: sc.generate_draws(seed, t, b, B, V), samp, tally)
        for r in range(2):
            _oracle_walk(w, cfg, conds[r:r + 1].expand(4, -1, -1), texts[r].expand(4, -1), n,
                         lambda t, b: sc.generate_draws(seed, t, b, 4, V), samp, tally)
        assert tally.within_cap() and tally.checked >= 9 * n, (name, tally)


def test_overflow_cases_stay_within_the_cap():
    """More survivors of the top-k filter than the top-p stage's 2048 staging entries, top_p = 1: the crafted tie row on the CPU (the
    natural top_k = 2100 rows are walked on the oracle's logits)."""
    for name, c in sc.overflow_cases().items():
        V = sc.OVERFLOW_V
        q = sc.overflow_noise(sc.CRAFTED_ROWS)
        tally = sc.Tally()
        if c["bias"] is not None:
            for b in range(sc.CRAFTED_ROWS):
                sc.simulate(c["bias"], lambda t: q[t, b], c["samp"], c["penalty"], sc.OVERFLOW_STEPS, tally)
        else:
            cfg = sc.config(V)
            w = {k: torch.from_numpy(v) for k, v in sc.natural_weights(V).items()}
            conds, texts = sc.prompts(V, sc.NAT_WIDTHS)
            _oracle_walk(w, cfg, conds[:1].expand(sc.CRAFTED_ROWS, -1, -1), texts[0].expand(sc.CRAFTED_ROWS, -1), sc.OVERFLOW_STEPS,
                         lambda t, b: q[t, b], c["samp"], tally, penalty=c["penalty"])
        assert tally.within_cap() and tally.checked >= 2 * sc.OVERFLOW_STEPS, (name, tally)


def _oracle_walk(w, cfg, conds, text, n, draws, samp, tally, penalty=sc.NAT_PENALTY):
    """generate_sample's loop (oracle/gpt.py) with the reference sampler in place of its own."""
    fake, emb, mask = og.prepare_gpt_inputs(w, cfg, conds, text)
    B, P, d = emb.shape
    V = cfg.number_mel_codes
    me, mp = og._t(w, "mel_embedding.weight"), og._t(w, "mel_pos_embedding.emb.weight")
    seen = np.zeros((B, V), bool)
    seen[:, 1] = seen[:, cfg.start_mel_token] = True
    live = np.ones(B, bool)
    past, last = None, None
    with torch.no_grad():
        for t in range(n):
            if past is None:
                x = torch.cat([emb, (me[cfg.start_mel_token] + mp[0])[None, None, :].expand(B, 1, d)], dim=1)
            else:
                x = (me[last] + mp[mask.shape[1] - P])[:, None, :]
            hidden, past = og.gpt2_stack(w, cfg, x, mask, past, False)
            logits = og.lm_head(w, cfg, hidden[:, -1]).float().numpy()
            nxt = np.full(B, cfg.stop_mel_token)
            for b in range(B):
                if live[b]:
                    st = sc.ref_step(logits[b], seen[b], draws(t, b), samp, penalty)
                    tally.checked += 1
                    tally.excused += 0 if st.decidable else 1
                    nxt[b] = st.token
                    seen[b, st.token] = True
                    live[b] = st.token != cfg.stop_mel_token
            last = torch.from_numpy(nxt)
            mask = torch.cat([mask, torch.ones(B, 1, dtype=torch.long)], dim=1)
