"""What the sampler tests share (tests/test_sampler_cases_cpu.py, tests/test_sampler_gpu.py): a float64 reference of the multinomial
sampler of csrc/decode.hip (`warp_row_token`) and of the greedy argmax, a restatement of the counter-based Exp(1) draws of
`exp1_draw` (csrc/decode.h), the models that hand the sampler exact logits, and the case lists.

How a test hands the sampler its logits: `mel_head` is not LayerNorm-folded, so a model whose mel_head.weight is all zeros has
logits[b][v] = mel_head.bias[v] at every step and row ("crafted rows").  Crafted values lie on a grid of 1/8, temperatures are 1, 0.5
or 2 and penalties 1 or 2: every score is exact in fp32 and in float64, so every comparison the kernel makes up to the softmax is
decided exactly.  "Natural rows" use ordinary synthetic head weights; the reference then runs on the GPU's own returned logits.

What "equal" means (EPS): a step is decidable when every margin of the reference -- the relative gap below the top-k threshold, the
distance of the cumulative sums from 1 - top_p relative to it, the relative gap between the best and second-best p / q -- is at
least 1e-5, about a hundred fp32 roundings where the kernel makes a handful and one expf per value.  On a decidable step the
kernel's token must be the reference's; on any other it must survive the reference's filters with each comparison loosened by EPS,
and such steps may be at most 1 % of a test's steps (CAP)."""
import functools

import numpy as np

EPS = 1e-5
CAP = 0.01
MASK = (1 << 64) - 1
_GOLD, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
U_MAX = np.float32(1.0 - 2.0 ** -24)


# ---- the draws ------------------------------------------------------------------------------------------------------------
def draw_bits(seed: int, idx) -> np.ndarray:
    """Top 24 bits of splitmix64's finaliser on seed + GOLD * (idx + 1), in uint64 arithmetic (numpy wraps mod 2^64)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(_GOLD) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(40)


def exp1(seed: int, idx) -> np.ndarray:
    """float32 Exp(1) draws of elements `idx`: u = (h + 0.5) / 2^24 in fp32 (a sum that rounds to even from h = 2^23 on), at most
    1 - 2^-24, q = -log(u) rounded to fp32."""
    h = draw_bits(seed, idx).astype(np.float32)
    u = np.minimum((h + np.float32(0.5)) * np.float32(2.0 ** -24), U_MAX)
    return (-np.log(u.astype(np.float64))).astype(np.float32)


def generate_draws(seed: int, step: int, b: int, B: int, V: int) -> np.ndarray:
    """Row b of step `step` of generate() on B rows: element (step * B + b) * V + v."""
    return exp1(seed, (step * B + b) * V + np.arange(V, dtype=np.uint64))


def session_draws(seed: int, t: int, slots: int, V: int) -> np.ndarray:
    """Step t (counted from the request's admission) of a request in a session of `slots` slots, whichever slot it has: row 0 of
    generate() on `slots` rows."""
    return exp1(seed, (t * slots) * V + np.arange(V, dtype=np.uint64))


def seed_for_bits(h: int, idx: int, low: int = 0x5A5A5A5A5A) -> int:
    """The seed under which element `idx` draws the 24 bits h: the finaliser run backwards (each of its steps is a bijection)."""
    def unshift(z, s):
        x = z
        for _ in range(64 // s + 1):
            x = z ^ (x >> s)
        return x
    z = ((h & 0xFFFFFF) << 40) | (low & ((1 << 40) - 1))
    z = unshift(z, 31)
    z = (z * pow(_M2, -1, 1 << 64)) & MASK
    z = unshift(z, 27)
    z = (z * pow(_M1, -1, 1 << 64)) & MASK
    z = unshift(z, 30)
    return (z - _GOLD * (idx + 1)) & MASK


# ---- the reference sampler ------------------------------------------------------------------------------------------------
class Step:
    __slots__ = ("token", "accept", "margins", "keep")

    @property
    def decidable(self):
        return all(m >= EPS for m in self.margins.values())


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def ref_step(logits, seen, q, samp, penalty) -> Step:
    """One row, one step.  logits: fp32 [V]; seen: bool [V] (the ids of input_ids: the prompt's fake ids and the earlier codes); q:
    fp32 [V] Exp(1) draws; samp: {"sampler": "hf" | "accel", "temperature", "top_k", "top_p"}.  Everything in float64.
    HF: repetition penalty -> / temperature -> top-k (scores strictly below the k-th largest removed, ties kept; off at 0 and from V
    on) -> top-p (ascending by (score, index), softmax, removed where the running sum <= 1 - top_p, never the last) -> softmax ->
    argmax(p / q), the lowest index on equality.  accel: softmax(l / T) / max(q, 1e-10), no penalty, no filters."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    V = l.size
    qd = np.asarray(q, dtype=np.float32).astype(np.float64)
    T = float(np.float32(samp.get("temperature", 1.0)))
    st = Step()
    st.margins = {}
    keep = np.ones(V, bool)
    loose = np.ones(V, bool)
    if samp["sampler"] == "accel":
        s = l / T
        qd = np.maximum(qd, float(np.float32(1e-10)))
    else:
        pen = float(np.float32(penalty))
        if pen != 1.0:
            l = np.where(seen, np.where(l < 0, l * pen, l / pen), l)
        s = l / T
        k = int(samp.get("top_k") or 0)
        top_p = float(np.float32(samp.get("top_p", 1.0)))
        if 0 < k < V:
            desc = np.sort(s)[::-1]
            kth = desc[k - 1]
            keep = s >= kth
            below = desc[desc < kth]
            if below.size:
                st.margins["top_k"] = _rel(kth, below[0])
                loose = s >= kth - EPS * max(abs(kth), 1e-300)
        if top_p < 1.0:
            sk = np.where(keep, s, -np.inf)
            order = np.lexsort((np.arange(V), sk))
            sv = sk[order]
            p = np.exp(sv - sv[-1])
            cum = np.cumsum(p / p.sum())
            thr = 1.0 - top_p
            remove = cum <= thr
            remove[-1] = False
            compared = cum[:-1][np.isfinite(sv[:-1])]
            st.margins["top_p"] = float(np.abs(compared - thr).min() / thr) if compared.size else np.inf
            surely = cum <= thr * (1.0 - EPS)
            surely[-1] = False
            gone = np.zeros(V, bool)
            gone[order[remove]] = True
            surely_gone = np.zeros(V, bool)
            surely_gone[order[surely]] = True
            loose = loose & ~(keep & surely_gone)
            keep = keep & ~gone
    top = s[keep].max()
    with np.errstate(over="ignore", divide="ignore"):
        r = np.where(keep, np.exp(s - top), 0.0) / qd
        rl = np.where(loose, np.exp(np.minimum(s - top, 700.0)), 0.0) / qd
    tok = int(np.argmax(r))
    others = np.delete(r, tok)
    second = others.max() if others.size else 0.0
    st.margins["argmax"] = (r[tok] - second) / r[tok] if second > 0.0 else np.inf
    st.token = tok
    st.keep = keep
    st.accept = loose & (rl >= r[tok] * (1.0 - EPS))
    st.accept[tok] = True
    return st


def ref_greedy(logits, seen, penalty) -> int:
    """argmax of the penalised logits, the lowest index among equal values."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    pen = float(np.float32(penalty))
    if pen != 1.0:
        l = np.where(seen, np.where(l < 0, l * pen, l / pen), l)
    return int(np.argmax(l))


class Tally:
    """Steps compared with the reference and, of those, the ones excused as undecidable."""

    def __init__(self):
        self.checked = self.excused = 0

    def add(self, other):
        self.checked += other.checked
        self.excused += other.excused

    def within_cap(self):
        return self.excused <= CAP * self.checked

    def __repr__(self):
        return f"{self.checked} steps checked, {self.excused} excused"


def check_row(codes, logits_of, draws_of, samp, penalty, V, start, stop, tally, what=""):
    """One row's codes against the reference, step by step on the logits it was sampled from and its own earlier codes.
    logits_of(t) -> fp32 [V], or None once the logits no longer belong to this row's history (the walk ends there);
    draws_of(t) -> fp32 [V].  Returns the steps walked.  Codes after the stop token must all be the stop token."""
    seen = np.zeros(V, bool)
    seen[1] = seen[start] = True      # the prompt's fake ids: 1 everywhere, then start_mel_token
    codes = [int(c) for c in codes]
    for t, tok in enumerate(codes):
        lg = logits_of(t)
        if lg is None:
            return t
        st = ref_step(lg, seen, draws_of(t), samp, penalty)
        tally.checked += 1
        if st.decidable:
            assert tok == st.token, f"{what} step {t}: token {tok}, reference {st.token}, margins {st.margins}"
        else:
            tally.excused += 1
            assert 0 <= tok < V and st.accept[tok], f"{what} step {t} (undecidable, {st.margins}): token {tok} survives no loosened filter"
        seen[tok] = True
        if tok == stop:
            assert all(c == stop for c in codes[t + 1:]), f"{what}: codes after the stop token"
            return t + 1
    return len(codes)


# ---- models ---------------------------------------------------------------------------------------------------------------
def config(V: int, max_mel_tokens: int = 40):
    from indextts_amd.config import GPTConfig
    return GPTConfig(model_dim=128, heads=2, layers=1, number_text_tokens=300, number_mel_codes=V, start_mel_token=V - 2,
                     stop_mel_token=V - 1, max_mel_tokens=max_mel_tokens, max_text_tokens=30, cond_latents=4)


@functools.lru_cache(maxsize=None)
def _base_weights(V: int, max_mel_tokens: int):
    from indextts_amd import weights
    return weights.synth_gpt_weights(config(V, max_mel_tokens), tag=f"t/sampler/{V}")


def natural_weights(V: int, max_mel_tokens: int = 40):
    return dict(_base_weights(V, max_mel_tokens))


def crafted_weights(bias: np.ndarray, max_mel_tokens: int = 40):
    """The model whose logits are `bias` at every step and row: a zero head weight."""
    V = bias.size
    w = dict(_base_weights(V, max_mel_tokens))
    w["mel_head.weight"] = np.zeros_like(w["mel_head.weight"])
    w["mel_head.bias"] = np.ascontiguousarray(bias, dtype=np.float32)
    return w


def prompts(V: int, widths, tag="t/sampler/prompt"):
    """(conds [n, 6, 128], texts: a list of [1, width] id tensors)."""
    import torch
    from indextts_amd import synth
    cfg = config(V)
    conds = torch.from_numpy(synth.uniform(f"{tag}/conds", (len(widths), cfg.cond_latents + 2, cfg.model_dim), 0.5))
    texts = [torch.from_numpy(synth.integers(f"{tag}/text/{i}", (1, int(wd)), 2, cfg.number_text_tokens)) for i, wd in enumerate(widths)]
    return conds, texts


def noise(seed: int, shape) -> np.ndarray:
    """Explicit Exp(1) draws, fp32, from torch's CPU generator (what HF's multinomial consumes)."""
    import torch
    return torch.empty(*shape).exponential_(1, generator=torch.Generator().manual_seed(seed)).numpy()


# ---- crafted rows ---------------------------------------------------------------------------------------------------------
def _grid(rng, V, lo, hi):
    """Values on the 1/8 grid in [lo, hi)."""
    return rng.integers(int(lo * 8), int(hi * 8), V).astype(np.float32) / np.float32(8.0)


def _row(V, seed, lo=-6.0, hi=-1.0, stop=-100.0):
    b = _grid(np.random.default_rng(seed), V, lo, hi)
    b[V - 1] = stop
    return b


# ids of one row of 1024 threads' 16 slices: both ends of the thread range, wave edges, several slices, the last partial slice
SPREAD = [0, 63, 64, 1023, 1024, 2047 + 513, 3071, 4096 + 5, 6 * 1024 + 700, 7168, 8191, 8190]
CRAFTED_ROWS, CRAFTED_STEPS, CRAFTED_NOISE_SEED = 3, 12, 4242


def crafted_cases():
    """name -> dict(bias, samp, penalty, probe): the crafted rows of section "Cases".  probe: ids whose draws the test makes small
    in turn (step t: probe[t % len] gets q * 1e-3), so that a token wrongly kept is drawn, not merely possible."""
    V = 8194
    cases = {}

    def add(name, bias, sampler="hf", T=1.0, k=0, p=1.0, penalty=1.0, probe=()):
        assert np.array_equal(bias * 8, np.round(bias * 8)) and np.abs(bias).max() <= 128
        cases[name] = {"bias": bias.astype(np.float32), "samp": {"sampler": sampler, "temperature": T, "top_k": k, "top_p": p},
                       "penalty": penalty, "probe": list(probe)}

    # top-k: the 12 largest values over several slices and both ends of the thread range; everything else below 0
    b = _row(V, 1)
    for j, v in enumerate(SPREAD):
        b[v] = 1.0 + j / 8
    outside = [2, 1025, 5000, 8189]
    add("topk12", b, T=1.0, k=12, probe=SPREAD[:4] + outside)
    add("topk12_T0.5", b, T=0.5, k=12, probe=SPREAD[8:] + outside)
    add("topk5_T2", b, T=2.0, k=5, probe=SPREAD[5:9] + outside)      # the threshold is SPREAD[7]: SPREAD[5], [6] are just outside
    # the threshold value five times: k = 8 keeps 12
    b = _row(V, 2)
    for j, v in enumerate(SPREAD[:7]):
        b[v] = 3.0 - j / 8
    ties = [8191, 7168 + 64, 5, 3 * 1024 + 1023, 8189]
    for v in ties:
        b[v] = 1.5
    add("topk8_ties5", b, k=8, probe=ties + [6, 4096])
    # top_k = V - 1 removes the one minimum; V and V + 7 switch the filter off (small vocabulary: one block-wide pass per k)
    Vs = 2050
    b = _row(Vs, 3, -4.0, 0.0, stop=-3.0)
    b[1500] = -9.0
    add("topk_Vm1", b, k=Vs - 1, probe=[1500, 3, 2049])
    add("topk_V", b, k=Vs, probe=[1500, 3, 2049])
    add("topk_Vp7", b, T=0.5, k=Vs + 7, probe=[1500, 3, 2049])
    # top_k = 1: the argmax of the penalised scores whatever the noise; the penalty demotes each winner in turn
    b = _row(V, 4)
    for j, v in enumerate([8191, 70, 7173, 1024, 3, 6 * 1024 + 1, 2048, 8190, 1023, 4097]):
        b[v] = 8.0 - j / 8
    add("topk1", b, k=1, penalty=2.0, probe=[5, 6, 7])

    # top-p (top_k <= 1024 required).  Survivors 0.125 .. 0.875 and one 7: the ascending running sum of the seven ends at 0.011,
    # far below 1 - top_p = 0.5: only the largest stays
    b = _row(V, 5)
    for j, v in enumerate([0, 1023, 1024, 4096, 7168, 8191, 8190]):
        b[v] = 0.125 * (1 + j)
    b[5000] = 7.0
    add("topp_only_largest", b, k=8, p=0.5, probe=[0, 8190, 1023])
    # eight survivors 1.0 .. 1.875: the smallest has p = 0.077 > 1 - 0.95: nothing removed
    b = _row(V, 6)
    for j, v in enumerate(SPREAD[:8]):
        b[v] = 1.0 + j / 8
    add("topp_nothing", b, k=8, p=0.95, probe=SPREAD[:3])
    # survivors 0, 0.5, then 2 2 2 (a tie group), 3, 3.5: p = .0128 .0211 .0947 x3 .2575 .4245.  Running sums .0128 .0339 | .1286 ...:
    # 1 - top_p = 0.07 cuts just below the group (wholly kept) ...
    b = _row(V, 7)
    vals = {SPREAD[0]: 0.0, SPREAD[3]: 0.5, SPREAD[4]: 2.0, SPREAD[7]: 2.0, SPREAD[10]: 2.0, SPREAD[9]: 3.0, SPREAD[1]: 3.5}
    for v, x in vals.items():
        b[v] = x
    add("topp_ties_above", b, k=7, p=0.93, probe=[SPREAD[0], SPREAD[3], SPREAD[4], SPREAD[10]])
    # ... and 1 - top_p = 0.35 just above it (running sum .3180 after the group, .5755 after the next): wholly removed
    add("topp_ties_below", b, k=7, p=0.65, probe=[SPREAD[4], SPREAD[7], SPREAD[10], SPREAD[9]])
    # the tie group at the top-k threshold itself (k = 5 keeps 7: 0.5 x3 is the threshold), wholly below the cut: survivors
    # .5 .5 .5 2 2.5 3 3.5 -> p = .0212 x3 .0951 .1567 .2585 .4261, running sums .0212 .0424 .0636 | .1587: 1 - top_p = 0.1
    b = _row(V, 8)
    vals = {70: 0.5, 7173: 0.5, 8191: 0.5, 1024: 2.0, 3: 2.5, 4097: 3.0, 2048: 3.5}
    for v, x in vals.items():
        b[v] = x
    add("topp_threshold_ties_below", b, T=1.0, k=5, p=0.9, probe=[70, 7173, 8191, 1024])

    # penalty 2.0 on seen ids with a negative (start id: -1 -> -2), a zero (id 1: stays 0) and positive logits (every sampled id):
    # k = 3 over candidates 0.5, 0 (id 1), -0.5, -1 (start), -1.5, ... -- halving instead of doubling the negative one would tie it
    # with -0.5 at the threshold; each sampled id is then halved or doubled and the membership of the top 3 moves from step to step
    b = _row(V, 9, -30.0, -20.0)
    cand = {5000: 0.5, 1: 0.0, 64: -0.5, V - 2: -1.0, 7168: -1.5, 1023: -2.0, 8191: -2.5, 2048: -3.0, 3: -3.5}
    for v, x in cand.items():
        b[v] = x
    add("penalty_signs_topk3", b, k=3, penalty=2.0, probe=[V - 2, 1, 64, 7168, 1023])
    add("penalty_signs_full", b, T=2.0, penalty=2.0, probe=[V - 2, 1, 64])
    b = _row(V, 10)
    for j, v in enumerate([8191, 70, 7173, 1024, 3, 6 * 1024 + 1, 2048, 8190, 1023, 4097, 5, 3000]):
        b[v] = 4.0 - j / 8
    add("penalty_moves_topk", b, T=0.5, k=3, penalty=2.0, probe=[8191, 70, 7173, 1024])
    add("accel_ignores_penalty", b, sampler="accel", T=0.5, penalty=2.0, probe=[8191, 70])
    return cases


def probe_noise(q: np.ndarray, probe) -> np.ndarray:
    """q [steps, B, V]: at step t the id probe[(t + b) % len(probe)] of row b gets a draw 1000 times smaller."""
    q = q.copy()
    if probe:
        for t in range(q.shape[0]):
            for b in range(q.shape[1]):
                q[t, b, probe[(t + b) % len(probe)]] *= np.float32(1e-3)
    return q


def simulate(bias, draws_of, samp, penalty, steps, tally=None):
    """The reference alone on a crafted row: its tokens (the walk ends after the stop token) and whether each step was decidable."""
    V = bias.size
    seen = np.zeros(V, bool)
    seen[1] = seen[V - 2] = True
    toks, dec = [], []
    for t in range(steps):
        st = ref_step(bias, seen, draws_of(t), samp, penalty)
        toks.append(st.token)
        dec.append(st.decidable)
        if tally is not None:
            tally.checked += 1
            tally.excused += 0 if st.decidable else 1
        seen[st.token] = True
        if st.token == V - 1:
            break
    return toks, dec


def greedy_tie_bias(V: int) -> np.ndarray:
    """Tiers of equal maxima: tier j has the value 8 - j / 8 at a high id (slice 7 at V = 8194) and at a low id in another wave.
    Greedy decoding with penalty 2 takes the low id, then -- the winner demoted to half -- the high one, then the next tier."""
    b = _row(V, 11, -6.0, 0.0)
    hi = [7 * 1024 + 5, 6 * 1024 + 9, 8191, 5 * 1024 + 1023] if V > 8000 else [200, 255, 129, 190]
    lo = [70, 200, 1030, 3] if V > 8000 else [3, 64, 127, 2]
    for j, (h, l) in enumerate(zip(hi, lo)):
        b[h] = b[l] = 8.0 - j / 8
    return b


def simulate_greedy(bias, penalty, steps, forced=None):
    V = bias.size
    seen = np.zeros(V, bool)
    seen[1] = seen[V - 2] = True
    toks = []
    for t in range(steps):
        tok = ref_greedy(bias, seen, penalty)
        toks.append(tok)
        nxt = tok if forced is None else int(forced[t])
        seen[nxt] = True
        if nxt == V - 1:
            break
    return toks


# ---- the distribution test ------------------------------------------------------------------------------------------------
DIST_V, DIST_B, DIST_STEPS = 258, 64, 100
DIST_CASES = {"full": ({"sampler": "hf", "temperature": 1.0, "top_k": 0, "top_p": 1.0}, 20240501),
              "T0.5_k8": ({"sampler": "hf", "temperature": 0.5, "top_k": 8, "top_p": 1.0}, 20240502)}


def dist_bias() -> np.ndarray:
    """Eight distinct values on top (3.0, 2.625, ... 0.375, in several waves), the rest in [-5, 0)."""
    b = _row(DIST_V, 12, -5.0, 0.0)
    for j, v in enumerate([200, 3, 64, 255, 127, 129, 190, 17]):
        b[v] = 3.0 - 0.375 * j
    return b


def dist_probs(samp) -> np.ndarray:
    """The distribution every (row, step) draws from (penalty 1: no dependence on the history)."""
    st = ref_step(dist_bias(), np.zeros(DIST_V, bool), np.ones(DIST_V, np.float32), samp, 1.0)
    s = dist_bias().astype(np.float64) / samp["temperature"]
    p = np.where(st.keep, np.exp(s - s[st.keep].max()), 0.0)
    return p / p.sum()


def chi2_quantile(dof: int, tail: float = 1e-6) -> float:
    """x with P(chi-square(dof) > x) = tail: bisection on the regularised upper incomplete gamma function."""
    import torch
    lo, hi = 0.0, 10.0 * dof + 200.0
    a = torch.tensor(dof / 2.0, dtype=torch.float64)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64))) > tail:
            lo = mid
        else:
            hi = mid
    return hi


def chi_square(tokens, p):
    """Pearson's statistic of the token counts against p, cells with an expected count below 5 pooled into one; tokens of
    probability 0 must not occur.  Returns (statistic, degrees of freedom)."""
    tokens = np.asarray(tokens).reshape(-1)
    n = tokens.size
    counts = np.bincount(tokens, minlength=p.size).astype(np.float64)
    assert counts[p == 0].sum() == 0, "a token of probability 0 was drawn"
    exp = n * p
    big = exp >= 5.0
    o, e = list(counts[big]), list(exp[big])
    if (~big & (p > 0)).any():
        o.append(counts[~big].sum())
        e.append(exp[~big].sum())
    o, e = np.array(o), np.array(e)
    return float(((o - e) ** 2 / e).sum()), len(o) - 1


def dist_simulate(samp, seed):
    """The reference fed the restated draws: tokens [B, STEPS] of generate() on DIST_B rows, and the undecidable count."""
    bias = dist_bias()
    toks = np.zeros((DIST_B, DIST_STEPS), np.int64)
    none = np.zeros(DIST_V, bool)
    undecided = 0
    for t in range(DIST_STEPS):
        for b in range(DIST_B):
            st = ref_step(bias, none, generate_draws(seed, t, b, DIST_B, DIST_V), samp, 1.0)
            toks[b, t] = st.token
            undecided += 0 if st.decidable else 1
    return toks, undecided


# ---- natural rows ---------------------------------------------------------------------------------------------------------
VOCABS = (1023, 1024, 1025, 2050, 8194, 16384)
NATURAL_SAMPLERS = {"hf_0.8_30_0.8": {"sampler": "hf", "temperature": 0.8, "top_k": 30, "top_p": 0.8},
                    "hf_1_0_1": {"sampler": "hf", "temperature": 1.0, "top_k": 0, "top_p": 1.0},
                    "hf_1.3_1_1": {"sampler": "hf", "temperature": 1.3, "top_k": 1, "top_p": 1.0},
                    "accel_0.8": {"sampler": "accel", "temperature": 0.8}}
NAT_SLOTS, NAT_STEPS, NAT_PENALTY = 4, 10, 10.0
NAT_WIDTHS = (5, 9)
SEEDS = (0, 1, 2 ** 63 + 5)
SEEDED_V, SEEDED_ROWS, SEEDED_WIDTH = 8194, 5, 7
SEEDED_SAMPLERS = ("hf_0.8_30_0.8", "hf_1_0_1")


def nat_noise_seed(V: int, name: str, r: int) -> int:
    return V * 100 + sorted(NATURAL_SAMPLERS).index(name) * 10 + r + 2000000


# ---- more survivors of the top-k filter than the top-p stage can stage (2048), without top-p --------------------------------
OVERFLOW_V, OVERFLOW_STEPS = 8194, 4


def overflow_tie_bias() -> np.ndarray:
    """3000 equal top scores over every slice."""
    b = _row(OVERFLOW_V, 13)
    b[np.random.default_rng(14).choice(OVERFLOW_V - 2, 3000, replace=False)] = 2.0
    return b


def overflow_noise(B: int) -> np.ndarray:
    """Draws [steps, B, V] that favour the ids of the last full slice (1000 times smaller there): the survivors a capped staging
    area would be most likely to lose, since every thread hands its slices over in ascending order."""
    q = noise(CRAFTED_NOISE_SEED + 1, (OVERFLOW_STEPS, B, OVERFLOW_V))
    q[:, :, 7168:8192] *= np.float32(1e-3)
    return q


def overflow_cases():
    """bias None: natural logits."""
    return {"natural_topk2100": {"bias": None, "samp": {"sampler": "hf", "temperature": 0.8, "top_k": 2100, "top_p": 1.0},
                                 "penalty": NAT_PENALTY},
            "ties3000_topk30": {"bias": overflow_tie_bias(), "samp": {"sampler": "hf", "temperature": 1.0, "top_k": 30, "top_p": 1.0},
                                "penalty": 1.0}}
