"""What the beam kernel tests share (tests/test_beam_cases_cpu.py, tests/test_beam_kernels_gpu.py): a float64 reference of one
utterance's whole beam step -- `beam_scores_kernel`, `beam_select_kernel` with its BeamSearchScorer bookkeeping (csrc/beam.hip) and
`beam_finalize` (csrc/gpt_beam.hip) --, the two draw-index formulas of `beam_select_kernel`, and the case lists.

Logits reach the kernels as in tests/sampler_cases.py: a zero mel_head.weight makes every row's logits mel_head.bias at every step.
  Exact rows (beam search, the scorer): one entry at 0, every other on the 1/8 grid in [-128, -110].  expf gives 0 there, so lse == 0
    and the log-softmax is the row itself; with penalty 1 or 2 every score and running sum is exact in fp32 and in float64, every tie is
    exact and the index rules decide it.  Nothing is excused on these rows.
  Grid rows (sampling, the filters): a bulk on the 1/8 grid in [-20, -14) and a dozen raised entries whose offsets are the marks of a
    Golomb ruler, temperatures 1 / 0.5 / 2, penalties 1 / 2.  lse and the running sums round in fp32, so every comparison carries a
    margin (EPS of sampler_cases).  Sums of one token multiset in another order tie in exact arithmetic; [a, b] and [b, a] are
    bit-equal in fp32 as well (decided by the index rule), from the third step on such sums are near-ties: undecidable.  Rows that
    put the mass on a dozen ids meet them at the third step at the latest and run two steps.
  Fine rows (sampling at length): flat rows on the 1/1024 grid in [-6, -1), for top_k = 30 with thirty raised entries whose offsets
    are a Sidon set (no two pairs with one sum): beams that hold different tokens then rarely tie, and seeds are chosen so that none
    do within six steps.  A 1/8 grid has 40 values for 8194 ids and would tie at nearly every step.

What is compared: a beam session admits the same request into every group with caps 1, 2, ... G (a seeded group draws as row 0 whichever
group it has), so group c returns the finalized output of the first c steps; the reference is stopped at each c.  From the first cap whose
output rests on an undecidable comparison on, nothing is asserted about the case, and those caps count against CAP."""
import functools

import numpy as np

import sampler_cases as sc
from sampler_cases import CAP, EPS, exp1, seed_for_bits      # noqa: F401  (draw_bits: through exp1)

SELECT_REGISTER_LIMIT = 1024 * 32      # nb * V up to here: beam_select_kernel keeps every key in registers; above, the re-reading loop
STAGE = 2048                           # top-k survivors beam_scores_kernel can sort for the top-p cut
GREY = 1e-30                           # a probability below this may be 0 in fp32 (expf underflows near e^-87 .. e^-103)


# ---- the draws ------------------------------------------------------------------------------------------------------------
def generate_beam_index(t: int, b: int, B: int, nb: int, V: int, i=0):
    """generate_beam on B utterances: element ((t * B + b) * nb * V) + i for flat candidate i = beam * V + token of utterance b."""
    return (t * B + b) * nb * V + i


def session_index(t: int, groups: int, nb: int, V: int, i=0):
    """A seeded session request at its own step t, whichever group it has: row 0 of generate_beam on `groups` utterances."""
    return (t * groups) * nb * V + i


def generate_beam_draws(seed, t, b, B, nb, V):
    return exp1(seed, generate_beam_index(t, b, B, nb, V) + np.arange(nb * V, dtype=np.uint64))


def session_draws(seed, t, groups, nb, V):
    return exp1(seed, session_index(t, groups, nb, V) + np.arange(nb * V, dtype=np.uint64))


# ---- the reference --------------------------------------------------------------------------------------------------------
def _rel(a, b):
    if np.isinf(a) or np.isinf(b):
        return np.inf
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


class BeamRef:
    """One utterance.  prm: num_beams, do_sample, temperature, top_k, top_p, length_penalty, early_stopping, penalty.
    exact: the row is an exact row (asserted: lse == 0, every finite score on the 1/8 grid) -- equal values are then decided by the
    index rules and every unequal pair is decided; otherwise a comparison is decidable when its margin is at least EPS, equal finite
    values are undecidable, and only equal zero keys / equal -inf scores (the fillers) are decided by the index rule.
    events: what the scorer did, for the coverage checks of the CPU test."""

    def __init__(self, V, start, stop, prm, exact=False):
        self.V, self.stop, self.prm, self.exact = V, stop, prm, exact
        nb = self.nb = int(prm["num_beams"])
        self.scores = np.full(nb, -1e9)
        self.scores[0] = 0.0
        self.seqs = [[] for _ in range(nb)]
        self.seen = np.zeros((nb, V), bool)
        self.seen[:, 1] = self.seen[:, start] = True      # input_ids = [1 ... 1, start]
        self.hyps = []                                     # (score, tokens) in the order added
        self.worst = 1e9
        self.done = False
        self.n = 0
        self.undecided = []                                # (step | "finalize c", which margin, value)
        self.sig = [() for _ in range(nb)]                 # per beam: its addends' (logit, seen) in order, while every row is one row
        self.events = []

    def _margin(self, what, m):
        if m < EPS:
            self.undecided.append((self.n, what, m))

    @staticmethod
    def _canon(sig):
        """Two running sums are bit-equal in fp32 when they add the same fp32 values in the same order, the first two in either
        order (0 + a is exact, a + b == b + a): [a, b] and [b, a] tie exactly at step 2, [a, b, c] and [a, c, b] only nearly."""
        return None if sig is None else tuple(sorted(sig[:2])) + tuple(sig[2:])

    def _cmp(self, what, a, b, same=False):
        """How surely a and b differ; equal values are for the index rule only where both sides hold them bit for bit (exact rows,
        -inf, or `same`: the same sum by _canon)."""
        if a == b:
            if not (self.exact or a == -np.inf or same):
                self._margin(what + " (equal)", 0.0)
        elif not self.exact:
            self._margin(what, _rel(a, b))

    def _proc(self, l, seen, live):
        """log_softmax -> repetition penalty -> (sampling) temperature, top-k, top-p: one beam's row, float64."""
        p, V = self.prm, self.V
        l = np.asarray(l, np.float32).astype(np.float64)
        m = l.max()
        lse = np.log(np.exp(l - m).sum())
        s = (l - m) - lse
        if self.exact:
            assert lse == 0.0 and np.array_equal(s * 8, np.round(s * 8)) and np.abs(s).max() <= 128
        pen = float(np.float32(p.get("penalty", 1.0)))
        if pen != 1.0:
            s = np.where(seen, np.where(s < 0, s * pen, s / pen), s)
        if not p["do_sample"]:
            return s
        T = float(np.float32(p.get("temperature", 1.0)))
        if T != 1.0:
            s = s / T
        k = max(int(p.get("top_k") or 0), 2) if int(p.get("top_k") or 0) > 0 else 0      # min_tokens_to_keep = 2
        if 0 < k < V:
            desc = np.sort(s)[::-1]
            kth = desc[k - 1]
            below = desc[desc < kth]
            if below.size and live:
                self._margin("top_k", _rel(kth, below[0]))
            s = np.where(s >= kth, s, -np.inf)
        top_p = float(np.float32(p.get("top_p", 1.0)))
        if top_p < 1.0:
            order = np.lexsort((np.arange(V), s))
            sv = s[order]
            pr = np.exp(sv - sv[-1])
            cum = np.cumsum(pr / pr.sum())
            thr = float(np.float32(1.0 - top_p))
            remove = cum <= thr
            remove[-2:] = False                            # never the last two
            compared = cum[:-2][np.isfinite(sv[:-2])]
            if compared.size and live:
                self._margin("top_p", float(np.abs(compared - thr).min() / thr))
            s = s.copy()
            s[order[remove]] = -np.inf
        return s

    def step(self, logits, q=None):
        """logits: [V] (every beam's row) or [nb, V]; q: fp32 [nb * V] Exp(1) draws when sampling."""
        assert not self.done
        p, nb, V = self.prm, self.nb, self.V
        logits = np.asarray(logits)
        flat = np.empty((nb, V))
        for j in range(nb):
            flat[j] = self._proc(logits if logits.ndim == 1 else logits[j], self.seen[j], self.scores[j] > -1e8) + self.scores[j]
        f = flat.reshape(-1)
        N, n_keep = nb * V, 2 * nb
        if p["do_sample"]:
            pr = np.exp(f - f.max())
            pr /= pr.sum()
            key = pr / np.asarray(q, np.float32).astype(np.float64)
        else:
            key = f
        order = np.lexsort((np.arange(N), -key))[: n_keep + 1]      # descending, the lower flat index among equals
        kv = key[order]
        for a, b in zip(kv[:-1], kv[1:]):
            if p["do_sample"]:
                if a == b:
                    if a != 0.0:
                        self._margin("select (equal keys)", 0.0)
                else:
                    self._margin("select", (a - b) / a)
            else:
                self._cmp("select", a, b)
        if p["do_sample"] and ((pr[order] > 0) & (pr[order] < GREY)).any():
            self._margin("select (a probability fp32 may flush to 0)", 0.0)
        cand = order[:n_keep]
        o2 = np.argsort(-f[cand], kind="stable")                     # by score, stable
        cand = cand[o2]
        cs = f[cand]
        one_row = logits.ndim == 1
        pen = float(p.get("penalty", 1.0)) != 1.0      # without a penalty a seen token's addend is an unseen one's
        csig = [self.sig[int(i) // V] + ((float(logits[int(i) % V]), pen and bool(self.seen[int(i) // V, int(i) % V])),) if one_row else None
                for i in cand]
        for r in range(n_keep - 1):
            self._cmp("order", cs[r], cs[r + 1], one_row and self._canon(csig[r]) == self._canon(csig[r + 1]))
        # ---- BeamSearchScorer.process ----
        gen_len = self.n + 1
        lp = float(p.get("length_penalty", 1.0))
        denom = float(gen_len) ** lp
        nxt = []
        for rank in range(n_keep):
            tok, src, s = int(cand[rank] % V), int(cand[rank] // V), float(cs[rank])
            sig = csig[rank]
            if tok == self.stop:
                if rank >= nb:
                    self.events.append("stop_below_num_beams")
                    continue
                self.events.append("stop_in_num_beams")
                self._add(s / denom, list(self.seqs[src]), sig=self.sig[src] + ((np.inf, True),) if one_row else None)
            else:
                nxt.append((s, tok, src, sig))
            if len(nxt) == nb:
                break
        assert len(nxt) == nb
        if len(self.hyps) >= nb:
            if p.get("early_stopping", False):
                self.done = True
            else:
                best = float(cs[0]) / denom
                self._cmp("is_done", self.worst, best)
                self.done = self.worst >= best
                self.events.append(("is_done", self.done, self.worst - best))
        self.scores = np.array([x[0] for x in nxt])
        self.seqs = [self.seqs[src] + [tok] for _, tok, src, _ in nxt]
        self.seen = np.stack([self.seen[src] for _, _, src, _ in nxt])
        self.sig = [x[3] for x in nxt]
        for j, (_, tok, _, _) in enumerate(nxt):
            self.seen[j, tok] = True
        self.n += 1
        if self.done:
            self.events.append("done")

    def _add(self, score, toks, hyps=None, tag="", sig=None):
        """BeamHypotheses.add on self (process) or on a copy (finalize): returns the new worst."""
        own = hyps is None
        hyps = self.hyps if own else hyps
        worst = self.worst if own else min([h[0] for h in hyps], default=1e9)
        nb = self.nb
        if len(hyps) >= nb:
            self._cmp(tag + "add", score, worst)
        if len(hyps) < nb or score > worst:
            hyps.append((score, toks, self._canon(sig)))
            if len(hyps) > nb:
                ss = [h[0] for h in hyps]
                wi = int(np.argmin(ss))                   # the smallest score, the earliest among equals
                rest = sorted(ss)
                if rest[0] == rest[1]:
                    self.events.append(tag + "worst_dropped_among_equals")
                self._cmp(tag + "drop", rest[0], rest[1])
                self.events.append(tag + "worst_dropped")
                del hyps[wi]
            worst = min(h[0] for h in hyps)
        else:
            self.events.append(tag + "add_refused")
        if own:
            self.worst = worst
        return worst

    def finalize(self, steps_done):
        """BeamSearchScorer.finalize after `steps_done` steps (the cap, or the step the scorer finished at): the best hypothesis, the
        stop token appended when it fits.  Leaves the state as it was; its undecided comparisons are recorded under "finalize"."""
        keep_n, self.n = self.n, f"finalize {steps_done}"
        hyps = list(self.hyps)
        if not self.done:
            lp = float(self.prm.get("length_penalty", 1.0))
            for j in range(self.nb):
                self._add(float(self.scores[j]) / float(steps_done) ** lp, list(self.seqs[j]), hyps, "finalize_", self.sig[j])
        ss = [h[0] for h in hyps]
        bi = max(range(len(ss)), key=lambda i: (ss[i], i))      # the largest score, the LAST of equals
        if ss.count(ss[bi]) > 1:
            self.events.append("finalize_equal_best")
        for i, s in enumerate(ss):
            if i != bi:
                self._cmp("finalize best", ss[bi], s, hyps[i][2] is not None and hyps[i][2] == hyps[bi][2])
        self.n = keep_n
        toks = list(hyps[bi][1])
        return toks + [self.stop] if len(toks) < steps_done else toks


class Run:
    """outs[c - 1]: the codes a request with cap c returns; first_bad: the first cap whose output rests on an undecidable comparison
    (None: every cap is asserted); done_at: the step count at which the scorer finished (None: never within G)."""

    def checked(self):
        return len(self.outs)

    def excused(self):
        return 0 if self.first_bad is None else len(self.outs) - self.first_bad + 1


def run(bias_or_logits, draws_of, prm, G, V=None, exact=False):
    """The reference on caps 1 .. G.  bias_or_logits: [V], or a callable (t, ref) -> [nb, V]; draws_of(t) -> fp32 [nb * V] or None."""
    V = V or np.asarray(bias_or_logits).size
    ref = BeamRef(V, V - 2, V - 1, prm, exact)
    r = Run()
    r.outs, r.first_bad, r.done_at, r.ref = [], None, None, ref
    for c in range(1, G + 1):
        if not ref.done:
            lg = bias_or_logits(c - 1, ref) if callable(bias_or_logits) else bias_or_logits
            ref.step(lg, draws_of(c - 1) if prm["do_sample"] else None)
            if ref.done:
                r.done_at = c
        r.outs.append(ref.finalize(ref.n))
        if ref.undecided and r.first_bad is None:
            r.first_bad = c
    return r


class Tally(sc.Tally):
    def __repr__(self):
        return f"{self.checked} caps checked, {self.excused} excused"


# ---- rows -----------------------------------------------------------------------------------------------------------------
def exact_row(V, seed, zero_at, stop=None, runners=None):
    """One entry at 0, the rest on the 1/8 grid in [-128, -110] (every value many times over, ties everywhere).  runners: id ->
    value of the best continuations after the 0; the rest is then at or below -110.5."""
    rng = np.random.default_rng(seed)
    b = (-110.0 - (4 if runners else 0) / 8.0 - rng.integers(0, 17 * 8 + 1, V) / 8.0).astype(np.float32)
    for v, x in (runners or {}).items():
        b[v] = x
    if stop is not None:
        b[V - 1] = stop
    b[zero_at] = 0.0
    return b


RUNNERS = {7: -110.125, 600: -110.125, 1023: -110.25}      # two equal ones: beams whose hypotheses tie


def grid_row(V, seed, stop=-100.0, lo=-20.0, hi=-14.0):
    """The bulk of a sampling row: far enough down that nearly all the mass is on the entries a case then raises."""
    return sc._row(V, seed, lo, hi, stop)


def fine_row(V, seed, stop=-100.0, lo=-6.0, hi=-1.0):
    """A flat sampling row on the 1/1024 grid: still exact in fp32 under temperatures 0.5 and 2 and penalty 2, but two pairs of tokens
    rarely have the same sum, so beams that hold different tokens do not tie (on the 1/8 grid, 40 values for 8194 ids, they would at
    nearly every step).  The 30 largest values lie within 0.02 of each other: many beams of similar probability."""
    b = np.random.default_rng(seed).integers(int(lo * 1024), int(hi * 1024), V).astype(np.float32) / np.float32(1024.0)
    b[V - 1] = stop
    return b


# the Mian-Chowla sequence: no two pairs of its members have the same sum
SIDON = (1, 2, 4, 8, 13, 21, 31, 45, 66, 81, 97, 123, 148, 182, 204, 252, 290, 361, 401, 475, 565, 593, 662, 775, 822, 916, 970, 1016, 1159,
         1312)


def sidon_top(b, limit, seed, hi=-1.0, also=()):
    """Raises 30 ids below `limit` (`also` among them), spread over the row, to hi - SIDON[j] / 1024: the survivors of top_k = 30,
    no two pairs of which have the same sum.  The bulk must lie below hi - 1.3."""
    ids = list(also) + [int(v) for v in np.random.default_rng(seed).permutation(limit) if v not in also][: 30 - len(also)]
    order = np.random.default_rng(seed + 1).permutation(30)
    for j, v in zip(order, ids):
        b[v] = hi - SIDON[j] / 1024.0
    return b


# a Golomb ruler: every difference between two marks is different, so no two pairs of raised entries have the same sum and
# beams that hold different tokens rarely tie; in eighths
RULER = (0, 2, 6, 24, 29, 40, 43, 55, 68, 75, 76, 85)


def _top(b, ids, hi=3.0):
    """Raises ids to hi - RULER[j] / 8."""
    for j, v in enumerate(ids):
        b[v] = hi - RULER[j] / 8.0
    return b


def noise(seed, G, nb, V, probe=(), scale=1e-3, together=False):
    """Explicit draws [G, nb * V]; at step t the token probe[t % len] gets a draw 1000 times (1 / scale) smaller on every beam --
    together: every probe at every step.  The candidates are re-ordered by score before the best num_beams become beams, so one
    wrongly kept id of low score is drawn and then dropped again; four of them among 2 * num_beams = 6 candidates leave at most two
    real ones, and one of the four becomes a beam."""
    q = sc.noise(seed, (G, nb * V))
    for t in range(G if probe else 0):
        for j in range(nb):
            for v in (probe if together else [probe[t % len(probe)]]):
                q[t, j * V + v] *= np.float32(scale)
    return q


def case(bias, nb, G=6, exact=False, draws=None, weight_format="f32", **prm):
    """draws: None (beam search), ("seed", s) or ("noise", q [G, nb * V])."""
    p = dict(num_beams=nb, do_sample=draws is not None, temperature=1.0, top_k=0, top_p=1.0, length_penalty=0.0, early_stopping=False,
             penalty=1.0)
    p.update(prm)
    assert nb * G <= 64
    return {"bias": np.ascontiguousarray(bias, np.float32), "prm": p, "G": G, "exact": exact, "draws": draws, "weight_format": weight_format}


def draws_of(c, groups=None):
    """t -> the draws of the case's request at step t in a session of `groups` groups (= row 0 of generate_beam on that many)."""
    if c["draws"] is None:
        return lambda t: None
    V, nb = c["bias"].size, c["prm"]["num_beams"]
    kind, x = c["draws"]
    if kind == "seed":
        return lambda t: session_draws(x, t, groups or c["G"], nb, V)
    return lambda t: x[t]


def reference(c):
    return run(c["bias"], draws_of(c), c["prm"], c["G"], exact=c["exact"])


# The draws of a sampled case: the seed (of the kernels' own generator, or of the explicit noise) under which the reference alone
# decides every cap -- chosen on the CPU by the reference's margins (tests/test_beam_cases_cpu.py proves it); names not listed use
# the default written at the case.
SEEDS = {"V8194_seed": 8203, "topk1024": 305}


# ---- the case lists -------------------------------------------------------------------------------------------------------
SAMPLE = dict(temperature=0.5, top_k=30, top_p=0.8, penalty=2.0)      # IndexTTS2.infer's shape of request on grid values
VOCABS = (1023, 1024, 1025, 2049, 8194, 16384)
# ids over several slices of a 1024-thread block, both ends of the thread range and wave edges (sampler_cases.SPREAD below 8190)
SPREAD = [v for v in sc.SPREAD if v < 8190]


@functools.lru_cache(maxsize=None)
def vocabulary_cases():
    """num_beams = 3 at every vocabulary edge, seeded and with explicit draws; the stop token is among the raised entries so that
    hypotheses finish."""
    cases = {}
    for V in VOCABS:
        b = sidon_top(fine_row(V, 100 + V, hi=-2.5), V - 2, 200 + V, also=(V - 1, 0, V - 3, 1023 % (V - 3), 1024 % (V - 3)))
        cases[f"V{V}_seed"] = case(b, 3, draws=("seed", SEEDS.get(f"V{V}_seed", 7 + V)), **SAMPLE)
        cases[f"V{V}_noise"] = case(b, 3, draws=("noise", noise(SEEDS.get(f"V{V}_noise", V), 6, 3, V)), temperature=2.0, top_k=30, top_p=0.8,
                                    length_penalty=1.0)
    return cases


def _switch_bias(V):
    """The same values at every id below 8188 (4092 for the 8-beam pair) whatever V is; the ids above, where the start and stop
    tokens of the neighbouring vocabularies sit, are far below: the two sides of the switch see one distribution."""
    base = 8192 if V > 6000 else 4096
    b = np.full(V, -100.0, np.float32)
    b[: base - 4] = fine_row(base, 31, hi=-2.5)[: base - 4]
    return sidon_top(b, base - 4, 32, also=(base - 5, 0, 1023, 1024))


def _switch_noise(seed, nb, V, G=6):
    """Per-(beam, token) draws that do not depend on V: drawn for the base vocabulary, ids beyond it get a draw of 50."""
    base = 8192 if V > 6000 else 4096
    q0 = sc.noise(seed, (G, nb, base))
    q = np.full((G, nb, V), 50.0, np.float32)
    q[:, :, :base] = q0
    return q.reshape(G, nb * V)


@functools.lru_cache(maxsize=None)
def select_switch_cases():
    """nb * V = 32768 exactly (keys in registers) and just above (the re-reading loop), beam-sample and beam search."""
    cases = {}
    for nb, V in ((4, 8192), (4, 8193), (4, 8194), (8, 4096), (8, 4097), (8, 8194)):
        b = _switch_bias(V)
        base = 8192 if V > 6000 else 4096
        cases[f"nb{nb}_V{V}_noise"] = case(b, nb, draws=("noise", _switch_noise(SEEDS.get(f"switch_nb{nb}_{base}", 77 + nb), nb, V)),
                                           temperature=1.0, top_k=30, top_p=0.9)
        cases[f"nb{nb}_V{V}_seed"] = case(b, nb, draws=("seed", SEEDS.get(f"nb{nb}_V{V}_seed", 5 + nb)), temperature=2.0, top_k=0, top_p=1.0,
                                          length_penalty=1.0)
        cases[f"nb{nb}_V{V}_search"] = case(exact_row(V, 3, 5, stop=-110.5), nb, exact=True, penalty=2.0, length_penalty=1.0)
    return cases


SWITCH_PAIRS = [("nb4_V8192_noise", "nb4_V8193_noise"), ("nb4_V8192_noise", "nb4_V8194_noise"), ("nb8_V4096_noise", "nb8_V4097_noise")]


def ties3000_bias(V=8194, seed=21, top_gap=8.0):
    """29 higher scores on top, 3000 scores tied at the top-k threshold of top_k = 30 (the 30th value), everything else lower:
    3029 survivors, more than the 2048 the top-p stage can sort.  The 29 sit in the last slices."""
    b = grid_row(V, seed)
    rng = np.random.default_rng(seed + 1)
    ties = np.sort(rng.choice(V - 2, 3000, replace=False))
    b[ties] = -4.0
    free = [v for v in range(V - 3, 0, -1) if b[v] != -4.0][:29]
    for j, v in enumerate(free):
        b[v] = -4.0 + top_gap + SIDON[j] / 1024.0
    return b, ties


def _between(bias, top_k, T, j):
    """top_p for which 1 - top_p lies midway between the j-th and the (j + 1)-th ascending cumulative sum of the top-k survivors."""
    s = bias.astype(np.float64) / T
    s = np.sort(s[s >= np.sort(s)[::-1][top_k - 1]])
    cum = np.cumsum(np.exp(s - s[-1]) / np.exp(s - s[-1]).sum())
    return float(1.0 - 0.5 * (cum[j - 1] + cum[j]))


@functools.lru_cache(maxsize=None)
def filter_cases():
    """top-k, top-p and the few-survivor steps of beam-sample, num_beams = 3 unless named; explicit draws with probes on the ids a
    wrong filter would let through.  Rows that put the mass on a dozen ids run two steps: from the third on, beams that hold one
    multiset of tokens in another order are the rule there, and those are near-ties in fp32."""
    V = 8194
    cases = {}

    def add(name, b, nb, probe, G=2, scale=1e-3, together=False, **prm):
        cases[name] = case(b, nb, G=G, draws=("noise", noise(SEEDS.get(name, 50 + len(cases)), G, nb, b.size, probe, scale, together)),
                           **prm)

    b = _top(grid_row(V, 41), SPREAD, hi=2.0)
    out = [2, 1025, 5000, 8189]
    for k in (1, 2, 30):
        add(f"topk{k}", b, 3, SPREAD[:4] + out, top_k=k, penalty=2.0)
    add("topk1024", fine_row(V, 48, stop=-1.0), 3, [], G=6, top_k=1024, penalty=2.0)
    add("topk30_topp0.8_T0.5", b, 3, SPREAD[:4] + out, **SAMPLE)
    b1023 = _top(grid_row(1023, 42), [1020, 0, 63, 64, 1000, 512, 700, 1022], hi=1.0)
    add("topk_ge_V_1023", b1023, 3, [3, 900], top_k=1024, top_p=0.9, temperature=2.0)
    # the k-th value five times, two of them inside k = 8: all five stay
    b = _top(grid_row(V, 43), SPREAD[:6], hi=3.0)
    ties = [8188, 7168 + 64, 5, 3 * 1024 + 1023, 8187]
    b[ties] = -8.5
    add("topk8_ties_straddle", b, 3, ties + [6, 4096], top_k=8, penalty=2.0)
    # the two maxima are zeros of either sign: the log-softmax gives both the same score, top_k = 1 (raised to 2) keeps exactly them
    b = grid_row(V, 44)
    b[70], b[7173] = np.float32(-0.0), np.float32(0.0)
    add("topk1_signed_zeros", b, 2, [70, 7173, 9], G=4, top_k=1)
    # 3000 scores at the threshold, top_p < 1: (a) the 29 above hold nearly all the mass, so the whole tie group and some of the 29
    # go; (b) the tie group holds most of it and the cut lands inside it, midway between two of its cumulative sums
    b, ties = ties3000_bias(top_gap=8.0)
    add("ties3000_all_removed", b, 3, [int(ties[-1]), int(ties[-7]), int(ties[1500]), int(ties[-100])], G=3, scale=1e-6, together=True, top_k=30,
        top_p=0.8)
    b, ties = ties3000_bias(top_gap=1.0)
    add("ties3000_cut_inside", b, 3, [int(ties[699]), int(ties[700]), int(ties[350]), int(ties[2999])], G=3, scale=1e-6, together=True, top_k=30,
        top_p=_between(b, 30, 1.0, 700))
    # top-p: a threshold midway between two cumulative sums; so small a top_p that only the last two stay; just below 1; and
    # top_p = 1 with top_k = 0 (the whole vocabulary survives)
    b = _top(grid_row(V, 45), SPREAD, hi=2.0)
    add("topp_between", b, 3, SPREAD[8:], top_k=12, top_p=_between(b, 12, 1.0, 5))
    add("topp_last_two", b, 3, SPREAD[:4], top_k=12, top_p=1e-6)
    add("topp_below_1", b, 3, SPREAD[8:], top_k=12, top_p=float(np.float32(1.0 - 2.0 ** -24)))
    add("topp1_topk0", fine_row(V, 46, stop=-30.0), 3, [], G=6, temperature=2.0)
    # fewer survivors than 2 * num_beams at step 0
    for nb in (3, 4, 8):
        add(f"two_survivors_nb{nb}", b, nb, SPREAD[:3], top_k=2, penalty=2.0)
    return cases


NEAR_SWEEP = 6
RUNNERS = {7: -110.5, 600: -110.5, 1023: -110.625}      # two equal ones: beams whose hypotheses tie


def _zero_row(V, a, b3):
    """The stop token at 0; three best continuations at -110, -110 - a / 8 and -110 - b3 / 8, everything else at or below -112."""
    r = exact_row(V, 1, V - 1, runners={9: -110.0, 700: -110.0 - a / 8.0, 1023: -110.0 - b3 / 8.0})
    r[(r > -112.0) & (r < -110.0 - max(a, b3) / 8.0)] = -112.0
    return r


@functools.lru_cache(maxsize=None)
def scorer_cases():
    """Exact rows, beam search, every length_penalty.
    zero<a>: the entry at 0 is the stop token and the best continuations are -110, -110 - a / 8, -110.5.  Step 0 finishes the empty
      hypothesis, step 1 one per beam; is_done then compares the second of them with the first: true at a = 0, false one grid step on.
    near<j>: the entry at 0 is id 5 and the stop token is at -110 - j / 8, moved across the best continuations one grid step at a
      time; the beam of 5s never ends and stays the best, so without early_stopping these groups reach their caps and return it
      while their hypotheses are replaced; with early_stopping the best hypothesis held at that moment is returned.
    sampled: beam-sample on a flat row with a likely stop token, where the hypotheses decide what is returned."""
    V = 1025
    cases = {}
    for lp in (0.0, 1.0, 2.0, -1.0):
        for a in (0, 1, 2):
            for es in (False, True):
                cases[f"zero{a}_lp{lp:g}_es{int(es)}"] = case(_zero_row(V, a, 4), 3, exact=True, length_penalty=lp, early_stopping=es,
                                                              penalty=1.0 + (a % 2))
        for j in range(NEAR_SWEEP):
            for es in (False, True):
                cases[f"near{j}_lp{lp:g}_es{int(es)}"] = case(exact_row(V, 2, 5, stop=-110.0 - j / 8, runners=RUNNERS), 3, G=8, exact=True,
                                                              length_penalty=lp, early_stopping=es, penalty=1.0 + (j % 2))
        for es in (False, True):      # beam-sample: no beam lasts for ever, so the hypotheses decide what is returned
            name = f"sampled_lp{lp:g}_es{int(es)}"
            b = sidon_top(fine_row(V, 60, hi=-2.5), V - 2, 61, also=(0, 1023))
            b[V - 1] = -0.25
            cases[name] = case(b, 3, draws=("noise", noise(SEEDS.get(name, 900), 6, 3, V)), top_k=30, top_p=0.9, length_penalty=lp,
                               early_stopping=es)
    for nb in (2, 4, 8):
        cases[f"near3_lp1_nb{nb}"] = case(exact_row(V, 2, 5, stop=-110.375, runners=RUNNERS), nb, exact=True, length_penalty=1.0, penalty=2.0)
        cases[f"zero1_lp2_nb{nb}"] = case(_zero_row(V, 1, 4), nb, exact=True, length_penalty=2.0)
    return cases


# ---- draw extremes --------------------------------------------------------------------------------------------------------
EXTREME_V, EXTREME_NB, EXTREME_G = 1025, 3, 2


def extreme_bias():
    return sidon_top(fine_row(EXTREME_V, 47, hi=-2.5), EXTREME_V - 2, 48)


def extreme_case(seed):
    return case(extreme_bias(), EXTREME_NB, G=EXTREME_G, draws=("seed", seed), top_k=30)


def _first_tokens(seed):
    c = extreme_case(seed)
    ref = BeamRef(EXTREME_V, EXTREME_V - 2, EXTREME_V - 1, c["prm"])
    ref.step(c["bias"], draws_of(c)(0))
    return [s[0] for s in ref.seqs]


@functools.lru_cache(maxsize=None)
def extreme_seeds():
    """(seed, id, expected to become a beam) twice: the seed under which the likeliest id draws the all-ones bits (the smallest
    draw, 6e-8) at step 0 of a seeded session request, found among seeds under which it is otherwise not drawn; and the seed under
    which an id that a plain seed makes the first beam draws the all-zero bits (the largest draw, 17.3)."""
    b = extreme_bias()
    best = int(np.argmax(np.where(np.arange(EXTREME_V) < EXTREME_V - 2, b, -np.inf)))
    ones = seed_for_bits(2 ** 24 - 1, session_index(0, EXTREME_G, EXTREME_NB, EXTREME_V, best))
    base = next(s for s in range(12345, 12400) if best not in _first_tokens(s))
    first = _first_tokens(base)[0]
    zeros = seed_for_bits(0, session_index(0, EXTREME_G, EXTREME_NB, EXTREME_V, first), low=base)
    return {"base": base, "ones": (ones, best), "zeros": (zeros, first)}


# ---- the distribution -----------------------------------------------------------------------------------------------------
DIST_V, DIST_NB, DIST_B, DIST_CALLS, DIST_SEED = 258, 2, 32, 100, 20241019
DIST_IDS = [200, 3, 64, 255, 127, 129, 190, 17]


def dist_bias():
    return sc.dist_bias()


def dist_prm():
    return dict(num_beams=DIST_NB, do_sample=True, temperature=1.0, top_k=8, top_p=1.0, length_penalty=1.0, early_stopping=False,
                penalty=1.0)


def dist_probs():
    """With a cap of 1 the returned code is the likeliest of the 2 * num_beams = 4 ids drawn without replacement from the eight
    survivors of top_k = 8 (the best-scored open beam): its law by enumeration of the ordered draws (successive sampling)."""
    import itertools
    b = dist_bias().astype(np.float64)
    w = np.exp(b[DIST_IDS] - b[DIST_IDS].max())
    w /= w.sum()
    out = np.zeros(DIST_V)
    for seq in itertools.permutations(range(8), 4):
        pr, rest = 1.0, 1.0
        for i in seq:
            pr *= w[i] / rest
            rest -= w[i]
        out[DIST_IDS[min(seq)]] += pr                 # DIST_IDS is in descending order of probability
    return out


def dist_reference(call, b):
    """The reference's code for utterance b of call `call` (seed DIST_SEED + call, B = DIST_B utterances, cap 1)."""
    r = run(dist_bias(), lambda t: generate_beam_draws(DIST_SEED + call, t, b, DIST_B, DIST_NB, DIST_V), dist_prm(), 1)
    return r.outs[0][0], r.first_bad is None


# ---- natural rows: the KV re-indexing -------------------------------------------------------------------------------------
KV_BEAMS, KV_FORMATS, KV_NEW, KV_GAP = (2, 4, 8), ("f32", "bf16"), 12, 2e-3

ALL_LISTS = {"vocabulary": vocabulary_cases, "select_switch": select_switch_cases, "filter": filter_cases, "scorer": scorer_cases}
