"""CPU: what tests/test_beam_kernels_gpu.py rests on (tests/beam_cases.py) -- the float64 beam reference against
oracle.gpt.generate_beam on the same crafted models (the oracle sees the same bias-only logits), the two draw-index formulas against
hand-computed indices, and, for every case list of the GPU file, that the reference alone keeps the caps at or after a first
undecidable comparison within CAP (exactly 0 on the exact rows).  The seeds and rows were chosen for that.  Each test prints its
counts (-s shows them)."""
import collections

import numpy as np
import pytest
import torch

import beam_cases as bc
import sampler_cases as sc
from oracle import gpt as og


def _events(r):
    return collections.Counter(e if isinstance(e, str) else f"{e[0]}_{e[1]}" for e in r.ref.events)


_REFS = {}


def _reference(lst, name):
    """One reference run per case for the whole module."""
    if (lst, name) not in _REFS:
        _REFS[lst, name] = bc.reference(bc.ALL_LISTS[lst]()[name])
    return _REFS[lst, name]


def _oracle_codes(c, cap):
    """oracle.gpt.generate_beam on the crafted model of case c with max_new_tokens = cap, fed the case's own draws."""
    bias, p = c["bias"], c["prm"]
    V, nb = bias.size, p["num_beams"]
    cfg = sc.config(V)
    tw = {k: torch.from_numpy(v) for k, v in sc.crafted_weights(bias).items()}
    conds, texts = sc.prompts(V, (6,))
    noise = None
    if p["do_sample"]:
        d = bc.draws_of(c)
        noise = torch.from_numpy(np.stack([d(t) for t in range(cap)]))[:, None, :]
    with torch.no_grad():
        out = og.generate_beam(tw, cfg, conds, texts[0], cap, noise, num_beams=nb, repetition_penalty_value=p["penalty"],
                               temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], length_penalty=p["length_penalty"],
                               do_sample=p["do_sample"], early_stopping=p["early_stopping"])
    return [int(x) for x in out[0]]


@pytest.mark.parametrize("lst", sorted(bc.ALL_LISTS))
def test_reference_agrees_with_oracle(lst):
    """Every case, every cap the reference decides: the oracle's codes.  The oracle runs in fp32 through torch, with the tie order
    pinned to the lower flat index; on exact rows it therefore has to agree everywhere."""
    torch.set_num_threads(8)
    n = 0
    for name, c in bc.ALL_LISTS[lst]().items():
        r = _reference(lst, name)
        for cap in range(1, c["G"] + 1):
            if r.first_bad is not None and cap >= r.first_bad:
                break
            if cap < c["G"] and cap > 2 and lst != "scorer" and c["bias"].size > 3000:
                continue                                   # large vocabularies: caps 1, 2 and the last one
            assert _oracle_codes(c, cap) == r.outs[cap - 1], (lst, name, cap)
            n += 1
    print(f"reference == oracle[{lst}]: {n} runs")
    assert n >= 2 * len(bc.ALL_LISTS[lst]())


def test_draw_indices_by_hand():
    """generate_beam: element ((t * B + b) * nb * V) + i; a seeded session request: (t * groups) * nb * V + i, row 0 of generate_beam
    on `groups` utterances; a session request with exp_noise reads row t of its own [cap][nb * V]."""
    assert bc.generate_beam_index(0, 0, 1, 3, 8194) == 0
    assert bc.generate_beam_index(2, 1, 4, 3, 8194, 5 + 8194) == (2 * 4 + 1) * 24582 + 8199 == 229437
    assert bc.generate_beam_index(5, 3, 8, 8, 8194, 7 * 8194 + 8193) == 43 * 65552 + 65551 == 2884287
    assert bc.session_index(3, 6, 4, 8193, 11) == 18 * 32772 + 11 == 589907
    assert bc.session_index(3, 6, 4, 8193, 11) == bc.generate_beam_index(3, 0, 6, 4, 8193, 11)
    V, nb = 1025, 3
    assert np.array_equal(bc.generate_beam_draws(7, 2, 1, 4, nb, V), bc.exp1(7, np.arange(9 * nb * V, 10 * nb * V)))
    assert np.array_equal(bc.session_draws(7, 2, 4, nb, V), bc.generate_beam_draws(7, 2, 0, 4, nb, V))
    assert not np.array_equal(bc.session_draws(7, 2, 4, nb, V), bc.session_draws(7, 2, 5, nb, V))
    q = bc.noise(3, 4, nb, V)
    c = bc.case(bc.fine_row(V, 1), nb, G=4, draws=("noise", q))
    assert np.array_equal(bc.draws_of(c)(2), q[2])
    # a flat index above 2^31 elements stays exact (the kernels add in size_t)
    assert bc.generate_beam_index(40, 7, 8, 8, 16384, 131071) == 327 * 131072 + 131071 > 2 ** 25
    assert int(bc.exp1(1, [bc.generate_beam_index(4000, 7, 8, 8, 16384, 131071)]).size) == 1


def test_reference_by_hand():
    """The reference on a row small enough to follow: V = 8, two beams, beam search, ids 6 / 7 the start / stop tokens."""
    V = 8
    b = np.array([-111.0, -110.5, 0.0, -110.0, -112.0, -110.0, -120.0, -110.25], np.float32)
    prm = dict(num_beams=2, do_sample=False, length_penalty=0.0, early_stopping=False, penalty=2.0)
    r = bc.run(b, lambda t: None, prm, 3, exact=True)
    # step 0 (beam 0 only; id 1 is seen: -221): 2 (0), 3 (-110), 5 (-110), 7 = stop (-110.25: rank 3 >= 2, and the beams are full
    # before it anyway).  Beams [2] 0, [3] -110.  Cap 1: the best open beam, then the stop token does not fit.
    assert r.outs[0] == [2]
    # step 1: [2] + 2 (seen, 0 stays 0) = 0; [2] + 3 = -110, [2] + 5 = -110, [3] + 2 = -110 (flat index 8 + 2 after 3 and 5).
    # Beams [2, 2] 0, [2, 3] -110.
    assert r.outs[1] == [2, 2]
    assert r.outs[2] == [2, 2, 2] and r.first_bad is None and r.done_at is None
    # the stop token at 0: the empty hypothesis at step 0, one per beam at step 1; is_done compares -110.5 with -110
    b[2], b[7] = -110.5, 0.0
    r = bc.run(b, lambda t: None, dict(prm, penalty=1.0), 4, exact=True)
    assert r.outs == [[7]] * 4 and r.done_at == 2
    # sampling, top_k = 1 (raised to 2): two survivors for four candidates: the fillers are flat ids 0 and 1 with a score of -inf
    b = np.array([-3.0, -2.5, 1.0, -4.0, 0.5, -6.0, -9.0, -8.0], np.float32)
    ref = bc.BeamRef(V, 6, 7, dict(prm, do_sample=True, top_k=1, penalty=1.0))
    q = (1.0 + np.arange(2 * V) / 64.0).astype(np.float32)
    ref.step(b, q)
    assert [s[-1] for s in ref.seqs] == [2, 4] and ref.undecided == []
    ref.step(b, q)      # [2, 2], then [2, 4] and [4, 2]: bit-equal sums, the lower flat index first
    assert ref.seqs == [[2, 2], [2, 4]] and ref.undecided == []


def test_few_survivors_fill_up_by_flat_index():
    """top_k = 2 with 3, 4 and 8 beams: step 0 has two survivors for 2 * num_beams candidates.  Pinned: the rest are zero-probability
    fillers taken by the lowest flat index (ids 0, 1, ... of beam 0, unless they survive), which become beams with a score of -inf;
    a later step takes no NaN from them (-inf - -inf never arises: the maximum is finite as long as one beam is).
    The vendored reference calls torch.multinomial(probs, 2 * num_beams) there (transformers_generation_utils.py:3515): ATen's
    no-replacement path is topk(probs / q) with no check of the number of positive entries, so it returns zero-probability ids as
    well, in whatever order its topk leaves equal keys -- [14, 16, 13, 12] after the two real ones for a 20-entry row with torch 2.10 on
    the CPU.  oracle.gpt.generate_beam and the kernels pin that order."""
    for nb in (3, 4, 8):
        c = bc.filter_cases()[f"two_survivors_nb{nb}"]
        V = c["bias"].size
        ref = bc.BeamRef(V, V - 2, V - 1, c["prm"])
        ref.step(c["bias"], c["draws"][1][0])
        real = [s[0] for s, x in zip(ref.seqs, ref.scores) if np.isfinite(x)]
        fill = [s[0] for s, x in zip(ref.seqs, ref.scores) if not np.isfinite(x)]
        assert len(real) == 2 and set(real) == {bc.SPREAD[0], bc.SPREAD[1]}
        lowest = [v for v in range(V) if v not in real][: nb - 2]
        assert fill == lowest and ref.undecided == []
        ref.step(c["bias"], c["draws"][1][1])
        assert not np.isnan(ref.scores).any() and np.isfinite(ref.scores[0]) and ref.undecided == []


@pytest.mark.parametrize("lst", sorted(bc.ALL_LISTS))
def test_reference_alone_stays_within_the_cap(lst):
    tally = bc.Tally()
    lines = []
    for name, c in bc.ALL_LISTS[lst]().items():
        r = _reference(lst, name)
        tally.checked += r.checked()
        tally.excused += r.excused()
        if c["exact"]:
            assert r.excused() == 0, (name, r.ref.undecided)
        lines.append(f"{name}: {r.checked()}/{r.excused()}")
    print(f"{lst}: {tally}\n  " + ", ".join(lines))
    assert tally.within_cap(), tally
    if lst == "scorer":
        assert tally.excused == 0


def test_case_lists_reach_what_they_are_for():
    """Every path and every scorer event the issue names occurs in some case."""
    sw = bc.select_switch_cases()
    sizes = {c["prm"]["num_beams"] * c["bias"].size for c in sw.values()}
    assert bc.SELECT_REGISTER_LIMIT in sizes and {32772, 32776, 32768 + 8, 65552} <= sizes
    for a, b in bc.SWITCH_PAIRS:      # the same row and draws on either side of the switch: the same codes
        assert _reference("select_switch", a).outs == _reference("select_switch", b).outs, (a, b)
    ev = collections.Counter()
    for lst in bc.ALL_LISTS:
        for name in bc.ALL_LISTS[lst]():
            ev.update(_events(_reference(lst, name)))
    print(dict(ev))
    for what in ("stop_in_num_beams", "stop_below_num_beams", "worst_dropped", "worst_dropped_among_equals", "add_refused",
                 "finalize_worst_dropped", "finalize_equal_best", "is_done_True", "is_done_False", "done"):
        assert ev[what] > 0, what
    sco = bc.scorer_cases()
    for lp in (0, 1, 2, -1):
        # is_done true and false one grid step apart: the second hypothesis of step 1 ties with the first, or is 1/8 below it
        t, f = _reference("scorer", f"zero0_lp{lp}_es0"), _reference("scorer", f"zero1_lp{lp}_es0")
        assert t.done_at == 2 and f.done_at != 2
        assert np.abs(sco[f"zero0_lp{lp}_es0"]["bias"] - sco[f"zero1_lp{lp}_es0"]["bias"]).max() == 0.125
        assert _reference("scorer", f"zero1_lp{lp}_es1").done_at == 2      # early_stopping does not wait
        # a group that finishes before its cap beside one that reaches it
        assert _reference("scorer", f"near0_lp{lp}_es0").done_at is None
    # the stop token moved across the best continuations changes what is returned
    assert len({tuple(map(tuple, _reference("scorer", f"near{j}_lp{lp}_es1").outs)) for j in range(bc.NEAR_SWEEP) for lp in (0, 1, -1)}) >= 3
    # the oversized tie group: 3029 survivors of top_k = 30
    for name in ("ties3000_all_removed", "ties3000_cut_inside"):
        b = bc.filter_cases()[name]["bias"]
        assert (b >= np.sort(b)[::-1][29]).sum() == 3029 > bc.STAGE


def test_draw_extremes_in_the_reference():
    """All-ones bits (the smallest draw, 6e-8) on the likeliest id: it becomes the first beam.  All-zero bits (the largest, 17.3)
    on the id that a plain seed makes the first beam: the draws of that seed are other ones, and the case stays decidable."""
    V, nb, G = bc.EXTREME_V, bc.EXTREME_NB, bc.EXTREME_G
    x = bc.extreme_seeds()
    seed, best = x["ones"]
    assert best not in bc._first_tokens(x["base"])
    q = bc.session_draws(seed, 0, G, nb, V)
    assert 5.9e-8 < q[best] < 6.0e-8 and bc._first_tokens(seed)[0] == best
    seed, first = x["zeros"]
    q = bc.session_draws(seed, 0, G, nb, V)
    assert abs(q[first] - 25 * np.log(2.0)) < 1e-5
    for seed in (x["base"], x["ones"][0], x["zeros"][0]):
        r = bc.reference(bc.extreme_case(seed))
        assert r.first_bad is None, (seed, r.ref.undecided)


def test_distribution_of_the_reference():
    """The chi-square test of the GPU file on the reference fed the restated draws: 3200 first-step codes against the law of the
    likeliest of four ids drawn without replacement."""
    p = bc.dist_probs()
    assert abs(p.sum() - 1.0) < 1e-12 and (p > 0).sum() == 5      # the three least likely ids are never the best of four
    toks, undecided = [], 0
    for call in range(bc.DIST_CALLS):
        for b in range(bc.DIST_B):
            tok, ok = bc.dist_reference(call, b)
            toks.append(tok)
            undecided += 0 if ok else 1
    stat, dof = sc.chi_square(np.array(toks), p)
    bound = sc.chi2_quantile(dof)
    print(f"distribution: chi-square {stat:.1f} on {dof} degrees of freedom, bound {bound:.1f}; {len(toks)} codes, {undecided} undecidable")
    assert stat <= bound and undecided <= bc.CAP * len(toks)
