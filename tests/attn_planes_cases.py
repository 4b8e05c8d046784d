"""The DiT plane attention (csrc/attention.hip: flash_attn_planes_kernel, launched by flash_attn_planes_forward, reached through
idxtts_attention_planes_fwd) case by case: the plane layout and the launcher's index rules restated from csrc/common.h and
csrc/attention.hip, a float64 reference, the float32 restatement that sets each case's bound, and the case table.  Host only (numpy):
nothing here calls the library.  tests/test_attn_planes_cases_cpu.py checks the table with the reference alone;
tests/test_attn_planes_gpu.py runs it through the instrument.

One call: B batch rows of T rows each in one [Mrows][ncols] projection output held as split-bf16 planes; head h of batch row b
attends from the queries b T + q_row0 + [0, Sq) to the keys b T + [0, min(kend[b], T)):  out = softmax(q^ k^T scale) v^ on the values
the planes hold -- q^ = hi + lo in the three-product form, q^ = hi in the one-product form -- so the split's own representation error
is not in the comparison.

A *shape* is one set of launch parameters; on it the GPU file runs both arithmetic *forms* (3: three MFMAs per product, 1: one) on
three input *kinds*; a *case* is (shape, kind, form).

  natural   q, k, v uniform in +-1.7: the scores q . k / 8 have a standard deviation of about 1, so no key's weight vanishes
  zero_q    q = 0: the output is the mean of the visible values, which exposes a key counted twice or not at all through the
            denominator
  needle    query i of (batch row, head) is moved along one edge key of the row -- edge (i + head) mod (number of edges), so every
            query block of 128 walks every edge -- until that key carries about half the weight.  The key `kend` itself is an edge
            too, where the planes hold such a row: the query points at it and it must not count."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from indextts_amd import synth

KINDS = ("natural", "zero_q", "needle")
FORMS = (3, 1)                 # MFMAs per product: idxtts_attention_planes_fwd's one_product = 0, 1
SCALE = 0.125
TILE, QBLK = 32, 128
NEG_BIG = np.float32(-1e30)
NAN_BITS = 0x7FC1              # a bf16 NaN: what the tests put wherever nothing may be read or must be written


# ---- layout, restated (csrc/common.h) ----------------------------------------------------------------------------------------------
def plane_index(row, col, rows):
    """chunk-major [col / 16][row][16]"""
    return ((col >> 4) * rows + row) * 16 + (col & 15)


def plane_elems(rows, cols):
    """elements of one plane; the lo plane follows the hi plane"""
    return ((cols + 15) // 16) * rows * 16


def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def split(x):
    """x float32 -> (hi, lo) float32 values of the split: hi = bf16_rne(x), lo = bf16_rne(x - hi)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_widen(bf16_bits(x))
    return hi, bf16_widen(bf16_bits(x - hi))


def pack(x):
    """[rows][cols] float32 (cols a multiple of 16; NaN allowed: it becomes NAN_BITS in both planes) -> uint16 [2 * plane_elems]"""
    rows, cols = x.shape
    assert cols % 16 == 0
    nan = np.isnan(x)
    x0 = np.where(nan, np.float32(0), x).astype(np.float32)
    hi = bf16_bits(x0)
    lo = bf16_bits(x0 - bf16_widen(hi))
    hi[nan] = NAN_BITS
    lo[nan] = NAN_BITS
    n = plane_elems(rows, cols)
    out = np.empty(2 * n, np.uint16)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    at = plane_index(r, c, rows)
    out[at] = hi
    out[n + at] = lo
    return out


def unpack_bits(planes, rows, cols):
    """uint16 [>= 2 * plane_elems] -> (hi bits, lo bits) [rows][cols]"""
    n = plane_elems(rows, cols)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    at = plane_index(r, c, rows)
    return planes[at], planes[n + at]


def unpack(planes, rows, cols):
    """-> hi + lo as float32 [rows][cols] (exact: the sum of a split fits fp32)"""
    hi, lo = unpack_bits(planes, rows, cols)
    return bf16_widen(hi) + bf16_widen(lo)


# ---- launcher and kernel control flow, restated (csrc/attention.hip) -----------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def acc_key(r, h):
    """register r of lane half h of a 32 x 32 accumulator holds this key of the tile"""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def launch_map(B, H, Sq):
    """flash_attn_planes_forward's grid and the kernel's XCD walk: (nqblk, pairs8, [(pair, qblk) | None per workgroup id])"""
    nq = cdiv(Sq, QBLK)
    pairs8 = cdiv(B * H, 8) * 8
    wgs = []
    for L in range(pairs8 * nq):
        qx = L >> 3
        pair, qblk = (qx // nq) * 8 + (L & 7), qx % nq
        wgs.append((pair, qblk) if pair < B * H else None)
    return nq, pairs8, wgs


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    name: str
    B: int
    H: int
    T: int
    q_row0: int
    Sq: int
    kend: Optional[Tuple[int, ...]]   # what the call passes (None: NULL); may exceed T
    alt_cols: bool                    # False: ncols = 3 * 64 H, q, k, v in that order from column 0; True: the other layout below
    pad_rows: int                     # Mrows = B T + pad_rows
    out: str                          # "rows" (o_token_stride > 64 H), "planes", "both"

    @property
    def d(self):
        return 64 * self.H

    @property
    def Mrows(self):
        return self.B * self.T + self.pad_rows

    @property
    def ncols(self):
        return 3 * self.d + (32 if self.alt_cols else 0)

    @property
    def cols(self):
        """(q_col, k_col, v_col)"""
        d = self.d
        return (16 + d, 16 + 2 * d, 16) if self.alt_cols else (0, d, 2 * d)

    def keys(self, b):
        """visible keys of batch row b"""
        return self.T if self.kend is None else min(self.kend[b], self.T)

    def ntiles(self, b):
        return cdiv(self.keys(b), TILE)

    @property
    def o_ts(self):
        return self.d + 24

    @property
    def o_bs(self):
        return self.Sq * self.o_ts + 40


SHAPES = [
    Shape("t5", 1, 1, 5, 0, 5, None, False, 0, "rows"),                     # one partial tile, three idle waves, seven idle workgroups
    Shape("t32", 1, 2, 32, 0, 32, None, True, 37, "both"),                  # one whole tile, mask branch not taken
    Shape("t33", 2, 1, 33, 0, 33, (33, 1), False, 0, "planes"),             # two tiles, one key in the last; a row with a single key
    Shape("t65", 2, 2, 65, 0, 65, (65, 64), True, 37, "rows"),              # three tiles: ring full, no reuse; a row ending on a tile edge
    Shape("t97", 1, 3, 97, 0, 97, None, False, 0, "both"),                  # four tiles: slot 0 reused
    Shape("t97k96", 1, 3, 97, 0, 97, (96,), False, 37, "planes"),           # ... three whole tiles of a 97-row sequence
    Shape("t129", 3, 3, 129, 0, 129, (129, 200, 0), True, 0, "both"),       # two query blocks, the second of one query; nine pairs: two
                                                                            # rounds with nq = 2; an empty row; kend clamped to T
    Shape("b17", 17, 1, 40, 0, 40, None, False, 37, "rows"),                # three rounds of pairs
    Shape("t300", 2, 4, 300, 0, 300, (300, 293), False, 0, "both"),         # exactly eight pairs, three query blocks, ten tiles
    Shape("tail65", 2, 2, 200, 65, 135, (200, 137), False, 37, "planes"),   # tail queries, odd offset, two query blocks
    Shape("tail144", 2, 2, 200, 144, 56, (200, 137), True, 0, "rows"),      # tail queries behind the shorter row's last key
]
SHAPE = {s.name: s for s in SHAPES}
assert len(SHAPE) == len(SHAPES)


def edge_keys(shape, b):
    """The keys of batch row b at which a key is most easily dropped or doubled: the first and the last visible key, both sides of
    every 32-key tile boundary, the last key of tiles 2 and 3 (the ring filling and its first slot reuse) -- and key `kend` itself
    (not visible) where the planes hold that row."""
    n = shape.keys(b)
    if n == 0:
        return []
    out = {0, n - 1}
    for t in range(1, shape.ntiles(b)):
        out |= {TILE * t - 1, TILE * t}
    for t in (2, 3):
        if n > TILE * t:
            out.add(min(TILE * t + TILE - 1, n - 1))
    if b * shape.T + n < shape.Mrows:
        out.add(n)
    return sorted(out)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _blocks(x, shape, b, rows=None):
    """q, k, v [H][rows][64] of batch row b out of the matrix (rows: a slice of the batch row's T rows, default all)"""
    rows = rows if rows is not None else slice(0, shape.T)
    r0 = b * shape.T
    sub = x[r0 + (rows.start or 0):r0 + rows.stop]
    return tuple(sub[:, c:c + shape.d].reshape(sub.shape[0], shape.H, 64).transpose(1, 0, 2) for c in shape.cols)


def natural_matrix(shape):
    """[Mrows][ncols] float32, uniform in +-1.7 (padding rows too: finite, as the kernel's contract asks); the columns that belong to
    nobody (alt_cols: the first and the last 16) are NaN -- the kernel has no business there."""
    x = synth.uniform(f"t/attn_planes/{shape.name}", (shape.Mrows, shape.ncols), 1.7)
    if shape.alt_cols:
        x[:, :16] = np.nan
        x[:, -16:] = np.nan
    return x


def needle_query(q0, K, vis, j):
    """q0 [64] moved along key j of K [n][64] until its score equals the log-sum-exp of the other visible keys' (about half the weight
    if j is visible; what it would take to get there if it is not)"""
    K64 = K.astype(np.float64)
    s = (q0.astype(np.float64) * SCALE) @ K64.T
    idx = np.arange(K.shape[0])
    others = s[(idx < vis) & (idx != j)]
    if others.size == 0:
        return q0
    lse = others.max() + np.log(np.exp(others - others.max()).sum())
    t = lse - s[j]
    return (q0.astype(np.float64) + t / SCALE * K64[j] / (K64[j] @ K64[j])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(shape_name, kind):
    """(matrix [Mrows][ncols] float32, target [B][H][Sq]: the key each query points at, or -1).  Shared: read only."""
    shape = SHAPE[shape_name]
    x = natural_matrix(shape)
    target = np.full((shape.B, shape.H, shape.Sq), -1, np.int64)
    qc = shape.cols[0]
    for b in range(shape.B):
        r0 = b * shape.T + shape.q_row0
        if kind == "zero_q":
            x[r0:r0 + shape.Sq, qc:qc + shape.d] = 0.0
        elif kind == "needle":
            edges = edge_keys(shape, b)
            if not edges:
                continue
            n = shape.keys(b)
            nk = min(n + 1, shape.Mrows - b * shape.T)               # the visible keys and key `kend`
            kc = shape.cols[1]
            for h in range(shape.H):
                K = x[b * shape.T:b * shape.T + nk, kc + 64 * h:kc + 64 * h + 64]
                K = sum(split(K))
                for i in range(shape.Sq):
                    j = edges[(i + h) % len(edges)]
                    target[b, h, i] = j
                    c = qc + 64 * h
                    x[r0 + i, c:c + 64] = needle_query(x[r0 + i, c:c + 64], K, n, j)
    x.setflags(write=False)
    return x, target


def held_values(x, form):
    """what the kernel of this form reads out of the planes of x: hi + lo, or hi alone (NaN columns stay NaN)"""
    hi, lo = split(np.where(np.isnan(x), np.float32(0), x))
    v = hi + lo if form == 3 else hi
    return np.where(np.isnan(x), np.float32(np.nan), v).astype(np.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def ref64(Q, K, V, mult=None):
    """softmax(Q K^T scale) V in float64: Q [m][64], K / V [n][64] -> [m][64]; mult [m][n]: how many times each query counts each key.
    No key: zeros."""
    if K.shape[0] == 0:
        return np.zeros((Q.shape[0], 64))
    s = (Q.astype(np.float64) * SCALE) @ K.astype(np.float64).T
    e = np.exp(s - s.max(axis=1, keepdims=True))
    if mult is not None:
        e = e * mult
    l = e.sum(axis=1, keepdims=True)
    return np.where(l > 0, (e @ V.astype(np.float64)) / np.where(l > 0, l, 1.0), 0.0)


def _dot16(a, b):
    """one bf16 MFMA step: 16 exact products summed in float32: a [m][16], b [n][16] -> [m][n]"""
    return (a[:, None, :] * b[None, :, :]).sum(axis=2, dtype=np.float32)


def ref32(Q, K, V, n, form):
    """The kernel's arithmetic restated in float32, in its own tile order, for the queries Q [m][64] (float32 matrix values; split
    here) of one (batch row, head) against its n visible keys; K / V [>= n][64] hold the rows of every tile, or end at the matrix's last
    row (a tile beyond reads that row again, as the kernel's address clamp does).  32-key tiles; per 16-dim chunk kl.qh + kh.ql + kh.qh (form 1: kh.qh); -1e30 in the last
    tile only; log2-domain online softmax with sc = scale log2 e in the exponent, the running sum per lane half; P split into bf16
    hi / lo (form 1: hi only); per 16-key group vl.ph + vh.pl + vh.ph; o / l."""
    f32 = np.float32
    m = Q.shape[0]
    qh, ql = split(Q)
    kh, kl = split(K)
    vh, vl = split(V)
    sc = f32(f32(SCALE) * f32(1.4426950408889634))
    o = np.zeros((m, 64), f32)
    m_run = np.full(m, NEG_BIG, f32)
    l_run = np.zeros((m, 2), f32)                       # per lane half
    half = np.array([[acc_key(r, h) for r in range(16)] for h in range(2)])
    last = K.shape[0] - 1
    for tile in range(cdiv(n, TILE)):
        key0 = tile * TILE
        rows = np.minimum(np.arange(key0, key0 + TILE), last)
        s = np.zeros((m, TILE), f32)
        for c in range(4):
            d = slice(16 * c, 16 * c + 16)
            if form == 3:
                s = s + _dot16(qh[:, d], kl[rows, d])
                s = s + _dot16(ql[:, d], kh[rows, d])
            s = s + _dot16(qh[:, d], kh[rows, d])
        if key0 + TILE > n:
            s[:, np.arange(key0, key0 + TILE) >= n] = NEG_BIG
        m_new = np.maximum(m_run, s.max(axis=1) * sc)
        alpha = np.exp2(m_run - m_new).astype(f32)
        p = np.exp2((s.astype(np.float64) * np.float64(sc) - m_new[:, None].astype(np.float64)).astype(f32)).astype(f32)      # one fma
        for h in range(2):
            psum = np.zeros(m, f32)
            for r in range(16):
                psum = psum + p[:, half[h, r]]
            l_run[:, h] = l_run[:, h] * alpha + psum
        o = o * alpha[:, None]
        m_run = m_new
        ph, pl = split(p)
        for t2 in range(2):
            g = slice(16 * t2, 16 * t2 + 16)
            kr = rows[g]
            if form == 3:
                o = o + _dot16(ph[:, g], vl[kr].T)
                o = o + _dot16(pl[:, g], vh[kr].T)
            o = o + _dot16(ph[:, g], vh[kr].T)
    l_tot = l_run[:, 0] + l_run[:, 1]
    with np.errstate(divide="ignore"):
        inv = np.where(l_tot > 0, f32(1) / l_tot, f32(0)).astype(f32)
    out = o * inv[:, None]
    assert out.dtype == f32
    return out


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def bound_of(form, err32, vmax):
    """form 3: 4 x the float32 restatement's own error (two fp32 evaluations in different orders), never below 2 fp32 ulps of the largest
    value -- the rule of decode_attn_cases._bound.  form 1: the derived bound of tests/test_acoustic_bf16_attention_gpu.py: rounding P
    once costs at most 2^-9 of sum(p |v|) in the numerator and 2^-9 relative in the denominator's counterpart."""
    if form == 3:
        return max(4.0 * err32, 2.0 * ulp32(vmax))
    return 2.0 ** -8 * vmax + 1e-5


@dataclass
class Case:
    shape: Shape
    kind: str
    form: int
    x: np.ndarray                  # [Mrows][ncols] float32: what is packed into the planes
    target: np.ndarray             # [B][H][Sq]
    ref: np.ndarray                # [B][Sq][64 H] float64
    err32: float                   # max |float32 restatement - ref|
    vmax: float                    # max |v^| over the visible values
    score_mass: float              # max over (query, key) of scale sum_i |q_i k_i|
    bound: float

    @property
    def id(self):
        return f"{self.shape.name}-{self.kind}-x{self.form}"


def head_operands(shape, xv, b, h):
    """Q [Sq][64], K, V [the rows of this batch row's tiles and one tile more, as far as the matrix goes][64] of (b, h) from the held
    values xv"""
    qc, kc, vc = (c + 64 * h for c in shape.cols)
    r0 = b * shape.T
    hi = min(r0 + (shape.ntiles(b) + 1) * TILE, shape.Mrows)
    return (xv[r0 + shape.q_row0:r0 + shape.q_row0 + shape.Sq, qc:qc + 64], xv[r0:hi, kc:kc + 64], xv[r0:hi, vc:vc + 64])


@functools.lru_cache(maxsize=None)
def case(shape_name, kind, form):
    shape = SHAPE[shape_name]
    x, target = inputs(shape_name, kind)
    xv = held_values(x, form)
    ref = np.zeros((shape.B, shape.Sq, shape.d), np.float64)
    err32 = vmax = mass = 0.0
    for b in range(shape.B):
        n = shape.keys(b)
        for h in range(shape.H):
            Q, K, V = head_operands(shape, xv, b, h)
            r = ref64(Q, K[:n], V[:n])
            ref[b, :, 64 * h:64 * h + 64] = r
            if n == 0:
                continue
            # the restatement splits the matrix values itself: hi + lo of x (form 3) or hi (form 1) are what held_values gave
            Qm, Km, Vm = head_operands(shape, np.where(np.isnan(x), np.float32(0), x), b, h)
            r32 = ref32(Qm, Km, Vm, n, form)
            assert np.isfinite(r32).all()
            err32 = max(err32, float(np.abs(r32.astype(np.float64) - r).max()))
            vmax = max(vmax, float(np.abs(V[:n]).max()))
            mass = max(mass, float((np.abs(Q).astype(np.float64) @ np.abs(K[:n]).astype(np.float64).T).max()) * SCALE)
    ref.setflags(write=False)
    return Case(shape, kind, form, x, target, ref, err32, vmax, mass, bound_of(form, err32, vmax))


def perturbed(c, b, h, queries, js, mult):
    """The float64 reference of query queries[i] of (b, h) with key js[i] counted mult times (0: removed, 2: twice, 1: a key behind
    kend counted after all): [len(js)][64]"""
    shape = c.shape
    n = shape.keys(b)
    Q, K, V = head_operands(shape, held_values(c.x, c.form), b, h)
    nk = min(n + 1, K.shape[0])
    m = np.ones((len(js), nk))
    m[:, n:] = 0.0
    m[np.arange(len(js)), np.asarray(js)] = mult
    return ref64(Q[np.asarray(queries)], K[:nk], V[:nk], m)
