"""The decode attention (csrc/decode.hip: decode_attn_body, three cache formats x two addressing modes x two merge modes) and the
kv_store_* kernels case by case: the layouts and index rules restated from the comments of csrc/decode.h, a float64 reference, the
float32 restatement that sets each case's bound, and the case table.  Host only (numpy): nothing here calls the library.
tests/test_decode_attn_cases_cpu.py checks the table with the reference alone; tests/test_decode_attn_gpu.py runs it through
idxtts_decode_attn_probe_run.

One attention step of one (row, head): the query q [64] of the new token against the row's keys kstart .. pos, where positions < pos are
cached and position pos is the new token's own k / v, rounded as the format rounds what it caches:  out = softmax(q . K / 8) V.

A *shape* is one set of buffers (format, addressing mode, rows, positions, left pads, dead slots, slot list, fan).  On a shape the
GPU file runs every *config* -- (nsplit, invariant) of CONFIGS, plus the fragment-image output -- on three input *kinds*; a *case*
is (shape, kind), and its bound comes from the float32 restatement over every launch of that case.

  natural   q, k uniform in +-1.7: the scores q . k / 8 have a standard deviation of about 1, so no key's weight vanishes
  zero_q    q = 0: the output is the mean of the values, which exposes a key counted twice or not at all through the denominator
  needle    per launch and (row, head), q is moved along one key -- each edge index of the row in turn -- until that key carries
            about half the weight

n >= 8192 keys (pieces longer than 512 keys in the batch-invariant mode) cannot occur in the product -- the position tables end at
2449 keys -- and is left out."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import kv_fp8_cases
from indextts_amd import synth

FMT = {"f32": 0, "bf16": 1, "fp8": 2}
# keys of the main row, the new token included: the edges of decode_attn_body (one key; a 16-key piece; the 128-key value prefetch; 128 +
# one P.V stride of 256 (fp32) or 512 (bf16, fp8) keys; the 512-key score pass and invariant piece; two and three pieces) and 2449, the
# longest the real position tables allow
N_VALUES = (1, 2, 16, 17, 127, 128, 129, 384, 385, 512, 513, 640, 641, 1024, 1025, 1537, 2449)
NSPLITS = (1, 2, 3, 5, 16)
# (nsplit, invariant): 0 = the library's own rule
CONFIGS = tuple((ns, inv) for inv in (0, 1) for ns in (0,) + NSPLITS)
KINDS = ("natural", "zero_q", "needle")
SENTINEL = 0xA5            # every byte of the caches and scales before the store
PIECE_KEYS, MAX_PIECES = 512, 16


# ---- index rules, restated ---------------------------------------------------------------------------------------------------------
def frag_index(row, k, kc16):
    """common.h: activations as MFMA A-fragment images [rows / 16][K / 16][64 lanes][4]."""
    return ((((row >> 4) * kc16 + (k >> 4)) * 64 + ((k & 15) >> 2) * 16 + (row & 15)) << 2) + (k & 3)


def frag_floats(rows, K):
    return ((rows + 15) // 16) * ((K + 15) // 16) * 256


def split_rule(B, H):
    """decode_attn_nsplit: workgroups per (row, head) of the key split."""
    wgs = B * H
    return max(1, min(16, 256 // wgs)) if wgs <= 128 else 1


def pieces(n):
    """decode_attn_pieces: pieces of a row with n keys in the batch-invariant mode."""
    return max(1, min(MAX_PIECES, (n + PIECE_KEYS - 1) // PIECE_KEYS))


def inv_wgs(B, H, Smax):
    """decode_attn_inv_wgs: workgroups per (row, head) in the batch-invariant mode."""
    return min(split_rule(B, H), pieces(max(Smax, 1)))


def resolve_nsplit(nsplit, invariant, B, H, Smax):
    return nsplit if nsplit else (inv_wgs(B, H, Smax) if invariant else split_rule(B, H))


def chunk_keys(n, NP):
    return ((n - 1 + NP) // NP + 15) & ~15 if NP > 1 else n


def piece_ranges(n, NP):
    """[(first, end)] of the NP contiguous pieces of a row's n keys, relative to its first key (first >= end: an empty piece)."""
    c = chunk_keys(n, NP)
    return [(z * c, max(z * c, min(n, (z + 1) * c))) for z in range(NP)]


def row_pieces(n, nsplit_used, invariant):
    """The pieces the kernel cuts a row of n keys into, and how many workgroups walk them."""
    NP = pieces(n) if invariant else nsplit_used
    return piece_ranges(n, NP), (min(nsplit_used, NP) if invariant else nsplit_used)


def edge_indices(n):
    """The key indices (relative to the row's first key) at which a key is most easily dropped or doubled: the first and last key of
    every piece of every config, the keys around the value prefetch (127 / 128) and the first score pass (511 / 512), the last cached
    key and the new token."""
    out = {n - 1}
    if n >= 2:
        out.add(n - 2)
    for NP in set(NSPLITS) | {pieces(n)}:
        for a, e in piece_ranges(n, NP):
            if a < e:
                out |= {a, e - 1}
    out |= {j for j in (127, 128, 511, 512) if j < n}
    return sorted(out)


# ---- roundings ---------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def cached(fmt, x):
    """x [..., 64] float32 -> what the cache of this format holds for it: (values float32, raw, scales | None); raw = the float32
    values, the bf16 bits or the e4m3 codes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if fmt == "f32":
        return x, x, None
    if fmt == "bf16":
        b = bf16_bits(x)
        return bf16_widen(b), b, None
    codes, scales, vals = kv_fp8_cases.quantize(x)
    return vals, codes, scales


RAW_DTYPE = {"f32": np.float32, "bf16": np.uint16, "fp8": np.uint8}


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    name: str
    fmt: str
    mode: str                      # "state": one DecodeState (a uniform pos, kstart per row); "slots": one SlotState per row
    H: int
    Smax: int
    pos: Tuple[int, ...]           # per step row: position of the new token = keys cached
    kstart: Tuple[int, ...]        # per step row: first valid key
    live: Tuple[int, ...]          # per step row (state mode: all 1)
    step_key: Tuple[Optional[str], ...]      # per step row: the data key of its step_qkv row (None: a dead slot)
    pre: Tuple[str, ...]           # per prefill row: the data key of its qkv rows
    S: int                         # prefill positions
    slot_ids: Optional[Tuple[int, ...]] = None     # slots mode: first cache row of each prefill row
    lens: Optional[Tuple[int, ...]] = None         # slots mode: valid positions of each prefill row
    fan: int = 1

    @property
    def B(self):
        return len(self.pos)

    @property
    def d(self):
        return 64 * self.H

    def n_keys(self, b):
        return self.pos[b] - self.kstart[b] + 1 if self.live[b] else 0

    def source(self, b):
        """(prefill row, copy) cache row b was stored from, or None."""
        if self.mode == "state":
            return (b, 0)
        for r, s0 in enumerate(self.slot_ids):
            if s0 <= b < s0 + self.fan:
                return (r, b - s0)
        return None


def _smax(n):
    return (n + 11) & ~3


def main_shape(n, fmt, mode, H=2):
    """The shape of n keys: row 0 sees n keys from key 0; beside it a left-padded / shorter row, and a row that sees (nearly) only its
    new token.  Slots mode: the prefill rows go to slots (2, 0, 3) and slot 1 is dead."""
    pos = n - 1
    keys = tuple(f"{n}/r{i}" for i in range(3))
    if mode == "state":
        k1 = min(pos, (pos // 3) | 1)
        return Shape(f"n{n}-{fmt}-state" + (f"-h{H}" if H != 2 else ""), fmt, mode, H, _smax(n), (pos,) * 3, (0, k1, pos), (1, 1, 1), keys, keys, pos)
    lens = (pos, min(pos, (pos // 2) | 1), min(pos, 1))
    return Shape(f"n{n}-{fmt}-slots", fmt, mode, H, _smax(n), (lens[1], 0, lens[0], lens[2]), (0,) * 4, (1, 0, 1, 1),
                 (keys[1], None, keys[0], keys[2]), keys, pos, (2, 0, 3), lens, 1)


def single_shape(n, fmt):
    """Row 0 of main_shape alone (B = 1): the batch-invariant mode's other batch size."""
    return Shape(f"n{n}-{fmt}-state-b1", fmt, "state", 2, _smax(n), (n - 1,), (0,), (1,), (f"{n}/r0",), (f"{n}/r0",), n - 1)


def fan_shape(n, fmt):
    """Two prefill rows, each to three consecutive slots (a beam group): slots 3..5 and 0..2, every slot with its own query."""
    pos = n - 1
    lens = (pos, pos // 2)
    keys = (f"{n}/r0", f"{n}/r1")
    sk = tuple(keys[1] + (f"/c{j}" if j else "") for j in range(3)) + tuple(keys[0] + (f"/c{j}" if j else "") for j in range(3))
    return Shape(f"n{n}-{fmt}-slots-fan3", fmt, "slots", 2, _smax(n), (lens[1],) * 3 + (lens[0],) * 3, (0,) * 6, (1,) * 6, sk, keys, pos,
                 (3, 0), lens, 3)


MAIN_SHAPES = [main_shape(n, fmt, mode) for n in N_VALUES for fmt in FMT for mode in ("state", "slots")]
SINGLE_SHAPES = [single_shape(n, fmt) for n in N_VALUES for fmt in FMT]
EXTRA_SHAPES = [main_shape(641, "bf16", "state", H=3)] + [fan_shape(385, fmt) for fmt in FMT]
SHAPES = MAIN_SHAPES + SINGLE_SHAPES + EXTRA_SHAPES
SHAPE = {s.name: s for s in SHAPES}
assert len(SHAPE) == len(SHAPES) and all(s.Smax <= 2560 and s.B <= 6 for s in SHAPES)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
_MAX_ROWS = max(N_VALUES)


@functools.lru_cache(maxsize=16)
def _pre_rows(key, H):
    """The prefill qkv rows of one data key: [rows][3d], q and k columns in +-1.7, v columns in +-1 (a prefix of one stream: the rows of a
    key do not depend on how many a shape takes)."""
    n = int(key.split("/")[0])
    d = 64 * H
    x = synth.uniform(f"t/dattn/{key}/pre/h{H}", (max(n - 1, 1), 3 * d), 1.0)
    x[:, :2 * d] *= np.float32(1.7)
    return x


def _step_row(key, H):
    d = 64 * H
    x = synth.uniform(f"t/dattn/{key}/step/h{H}", (3 * d,), 1.0)
    x[:2 * d] *= np.float32(1.7)
    return x


def prefill_qkv(shape):
    """[n][S][3d] float32: what the store reads (positions at and behind a row's len are right padding: arbitrary values)."""
    d = shape.d
    out = np.zeros((len(shape.pre), shape.S, 3 * d), np.float32)
    for r, key in enumerate(shape.pre):
        out[r] = _pre_rows(key, shape.H)[:shape.S]
    return out


def step_qkv0(shape):
    """[B][3d] float32: the natural step rows (a dead slot's row: arbitrary values the kernel must not read into the cache)."""
    return np.stack([_step_row(k if k is not None else f"dead/{shape.name}", shape.H) for k in shape.step_key])


def _heads(x, H):
    """[..., 3d] -> q, k, v [..., H, 64]"""
    d = 64 * H
    return tuple(x[..., i * d:(i + 1) * d].reshape(x.shape[:-1] + (H, 64)) for i in range(3))


@dataclass
class Stored:
    """What the store and one step leave behind, on the host."""
    kcache: np.ndarray
    vcache: np.ndarray
    kscale: Optional[np.ndarray]
    vscale: Optional[np.ndarray]
    qkv_after: np.ndarray          # the prefill qkv with its k / v columns as the store rewrites them
    K: list                        # per step row: dequantised keys [H][n_b][64] float32, the new token's last (None: dead)
    V: list


@functools.lru_cache(maxsize=4)
def stored(shape):
    """The expected raw buffers (SENTINEL bytes wherever nothing is stored) and each row's dequantised keys and values (shared: read only)."""
    fmt, H, B, Smax, d = shape.fmt, shape.H, shape.B, shape.Smax, shape.d
    raw = RAW_DTYPE[fmt]
    kg = 16 if fmt == "f32" else 8           # granules per key, EPG elements each
    epg = 64 // kg
    sent = np.full(8, SENTINEL, np.uint8)
    kc = np.full((B, H, kg, Smax, epg), sent[:raw().itemsize].view(raw)[0], raw)
    vc = np.full((B, H, Smax, 64), sent[:raw().itemsize].view(raw)[0], raw)
    ksc = vsc = None
    if fmt == "fp8":
        ksc = np.full((B, H, Smax), sent[:4].view(np.float32)[0], np.float32)
        vsc = ksc.copy()
    qkv = prefill_qkv(shape)
    _, pk, pv = _heads(qkv, H)                                   # [n][S][H][64]
    kval, kraw, kscl = cached(fmt, pk)
    vval, vraw, vscl = cached(fmt, pv)
    after = qkv.copy()
    if fmt != "f32":        # bf16 / fp8: every row of the prefill is rounded in place, right padding too
        after[..., d:2 * d] = kval.reshape(kval.shape[:2] + (d,))
        after[..., 2 * d:] = vval.reshape(vval.shape[:2] + (d,))
    sq = step_qkv0(shape)
    _, nk, nv = _heads(sq, H)                                    # [B][H][64]
    nkval, nkraw, nkscl = cached(fmt, nk)
    nvval, nvraw, nvscl = cached(fmt, nv)
    Ks, Vs = [], []
    for b in range(B):
        src = shape.source(b)
        if src is not None:
            r = src[0]
            ln = shape.S if shape.lens is None else shape.lens[r]
            for h in range(H):
                kc[b, h, :, :ln, :] = kraw[r, :ln, h].reshape(ln, kg, epg).transpose(1, 0, 2)
                vc[b, h, :ln, :] = vraw[r, :ln, h]
                if fmt == "fp8":
                    ksc[b, h, :ln] = kscl[r, :ln, h]
                    vsc[b, h, :ln] = vscl[r, :ln, h]
        if not shape.live[b]:
            Ks.append(None)
            Vs.append(None)
            continue
        p, k0 = shape.pos[b], shape.kstart[b]
        for h in range(H):
            kc[b, h, :, p, :] = nkraw[b, h].reshape(kg, epg)
            vc[b, h, p, :] = nvraw[b, h]
            if fmt == "fp8":
                ksc[b, h, p] = nkscl[b, h]
                vsc[b, h, p] = nvscl[b, h]
        r = src[0] if src is not None else None
        assert p == 0 or r is not None
        oldk = kval[r, k0:p].transpose(1, 0, 2) if p > k0 else np.zeros((H, 0, 64), np.float32)
        oldv = vval[r, k0:p].transpose(1, 0, 2) if p > k0 else np.zeros((H, 0, 64), np.float32)
        Ks.append(np.concatenate([oldk, nkval[b][:, None, :]], axis=1))
        Vs.append(np.concatenate([oldv, nvval[b][:, None, :]], axis=1))
    return Stored(kc, vc, ksc, vsc, after, Ks, Vs)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def ref64(Q, K, V, mult=None):
    """softmax(Q K^T / 8) V in float64: Q [m][64], K / V [n][64] -> [m][64]; mult [m][n]: how many times each query counts each key."""
    s = (Q.astype(np.float64) * 0.125) @ K.astype(np.float64).T
    e = np.exp(s - s.max(axis=1, keepdims=True))
    if mult is not None:
        e = e * mult
    l = e.sum(axis=1, keepdims=True)
    return np.where(l > 0, (e @ V.astype(np.float64)) / np.where(l > 0, l, 1.0), 0.0)


def ref32(Q, K, V):
    """The same formula in float32 throughout, every sum in natural order: head dims 0..63 for a score, keys first to last for the
    denominator and the output."""
    Q, K, V = (np.ascontiguousarray(a, dtype=np.float32) for a in (Q, K, V))
    qs = Q * np.float32(0.125)
    s = np.zeros((Q.shape[0], K.shape[0]), np.float32)
    for i in range(64):
        s += qs[:, i, None] * K[None, :, i]
    e = np.exp(s - s.max(axis=1, keepdims=True))
    assert e.dtype == np.float32
    l = np.zeros(Q.shape[0], np.float32)
    acc = np.zeros((Q.shape[0], 64), np.float32)
    for j in range(K.shape[0]):
        l += e[:, j]
        acc += e[:, j, None] * V[j]
    return acc / l[:, None]


def needle_query(q0, K, j):
    """q0 moved along key j until that key's score equals the log-sum-exp of the others' (about half the weight), in float32."""
    K64 = K.astype(np.float64)
    s = (q0.astype(np.float64) * 0.125) @ K64.T
    others = np.delete(s, j)
    lse = others.max() + np.log(np.exp(others - others.max()).sum()) if others.size else s[j]
    t = lse - s[j]
    return (q0.astype(np.float64) + t * 8.0 * K64[j] / (K64[j] @ K64[j])).astype(np.float32)


@dataclass
class Case:
    shape: Shape
    kind: str
    step_qkv: np.ndarray           # [L][B][3d] float32: one step_qkv per launch (k / v columns the same in every launch)
    target: np.ndarray             # [L][B][H] needle: the key index (relative to the row's first key) the query points at, else -1
    ref: np.ndarray                # [L][B][d] float64
    err32: float                   # max |float32 restatement - ref| over the case
    vmax: float                    # max |value| of the case
    score_mass: float              # max over (query, key) of sum_i |q_i k_i| / 8: what a score's rounding error scales with
    bound: float

    @property
    def id(self):
        return f"{self.shape.name}-{self.kind}"


def _bound(err32, vmax):
    """4 x the float32 restatement's own error (two fp32 evaluations in different orders); never below 2 fp32 ulps of the largest value:
    expf and the division, where the restatement happens to be exact (one key)."""
    return max(4.0 * err32, 2.0 * float(np.spacing(np.float32(vmax))))


@functools.lru_cache(maxsize=None)
def case(shape_name, kind):
    shape = SHAPE[shape_name]
    st = stored(shape)
    B, H, d = shape.B, shape.H, shape.d
    sq0 = step_qkv0(shape)
    q0 = _heads(sq0, H)[0]                                        # [B][H][64]
    if kind == "needle":
        edges = [edge_indices(shape.n_keys(b)) if shape.live[b] else [] for b in range(B)]
        L = max(-(-len(e) // H) for e in edges)
    else:
        L = 1
    step = np.repeat(sq0[None], L, axis=0).copy()
    target = np.full((L, B, H), -1, np.int64)
    ref = np.zeros((L, B, d), np.float64)
    err32 = vmax = mass = 0.0
    for b in range(B):
        if not shape.live[b]:
            continue
        for h in range(H):
            K, V = st.K[b][h], st.V[b][h]
            if kind == "natural":
                Q = q0[b, h][None]
            elif kind == "zero_q":
                Q = np.zeros((1, 64), np.float32)
            else:
                e = edges[b]
                target[:, b, h] = [e[(i * H + h) % len(e)] for i in range(L)]
                Q = np.stack([needle_query(q0[b, h], K, j) for j in target[:, b, h]])
            step[:, b, h * 64:(h + 1) * 64] = Q
            r = ref64(Q, K, V)
            ref[:, b, h * 64:(h + 1) * 64] = r
            r32 = ref32(Q, K, V)
            assert np.isfinite(r32).all()
            err32 = max(err32, float(np.abs(r32.astype(np.float64) - r).max()))
            vmax = max(vmax, float(np.abs(V).max()))
            mass = max(mass, float((np.abs(Q).astype(np.float64) @ np.abs(K).astype(np.float64).T).max()) * 0.125)
    return Case(shape, kind, step, target, ref, err32, vmax, mass, _bound(err32, vmax))


def perturbed(c, l, b, h, js):
    """The float64 reference of launch l, (row b, head h) with key j removed, and with it counted twice, for every j of js:
    ([len(js)][64], [len(js)][64])."""
    st = stored(c.shape)
    K, V = st.K[b][h].astype(np.float64), st.V[b][h].astype(np.float64)
    s = (c.step_qkv[l, b, h * 64:(h + 1) * 64].astype(np.float64) * 0.125) @ K.T
    e = np.exp(s - s.max())
    js = np.asarray(js)
    out = []
    for m in (0.0, 2.0):
        mult = np.ones((len(js), K.shape[0]))
        mult[np.arange(len(js)), js] = m
        w = e[None] * mult
        l_ = w.sum(axis=1, keepdims=True)
        out.append(np.where(l_ > 0, (w @ V) / np.where(l_ > 0, l_, 1.0), 0.0))
    return out


def unfrag(image, B, d):
    """The A-fragment image of [B][d] -> rows."""
    rows, cols = np.meshgrid(np.arange(B), np.arange(d), indexing="ij")
    return image[frag_index(rows, cols, d >> 4)]
