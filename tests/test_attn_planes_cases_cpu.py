"""CPU: the case table of tests/attn_planes_cases.py, checked with the reference alone (no library call).

  (a) coverage     through the restated launcher and control flow of flash_attn_planes_kernel (ntiles = ceil(kend / 32), nqblk =
                   ceil(Sq / 128), pairs8, the workgroup -> (pair, query block) map), some shape reaches every edge, by name; the map
                   covers every (pair, query block) exactly once;
  (b) sensitivity  for every needle case (both forms) and every zero_q case (three-product form), for every row, head and edge key: the
                   float64 reference with that key removed, and with it counted twice -- for key `kend` itself: counted at all -- is at
                   least 8 x the case's bound away from the reference.  A kernel that drops, doubles or unmasks one such key cannot pass
                   tests/test_attn_planes_gpu.py.  A condition on the inputs, not a measurement;
  (c) restatement  the float32 restatement that sets each three-product bound is finite and within an a-priori rounding premise of
                   the float64 reference, every such bound stays below test_attention_vs_torch's 1e-4 max(1, |ref|max), and the
                   one-product restatement stays inside its derived bound; the errors are printed per case (-s);
  (d) layout       pack then unpack is the identity on split values; one hand-checked index."""
import numpy as np
import pytest

import attn_planes_cases as ac


def test_table_reaches_every_edge_of_the_control_flow():
    seen = set()
    for s in ac.SHAPES:
        nq, pairs8, wgs = ac.launch_map(s.B, s.H, s.Sq)
        assert nq == ac.cdiv(s.Sq, 128) and pairs8 % 8 == 0 and 0 <= pairs8 - s.B * s.H < 8 and len(wgs) == pairs8 * nq
        live = [w for w in wgs if w is not None]
        assert sorted(live) == [(p, q) for p in range(s.B * s.H) for q in range(nq)], f"{s.name}: the map misses or repeats a (pair, query block)"
        for L, w in enumerate(wgs):         # all query blocks of a pair on one XCD (workgroup id mod 8)
            assert w is None or w[0] % 8 == L % 8
        assert s.q_row0 >= 0 and s.q_row0 + s.Sq <= s.T and s.B * s.T <= s.Mrows
        for b in range(s.B):
            nt, n = s.ntiles(b), s.keys(b)
            seen.add(f"ntiles {nt}" if nt < 5 else "ntiles 5 or more")
            if n:
                seen.add("last tile masked" if n % 32 else "last tile unmasked")
            if n == 1:
                seen.add("a row with a single key")
            if s.kend is not None and s.kend[b] > s.T:
                seen.add("kend clamped to T")
            if any(b * s.T + t * 32 + 31 > s.Mrows - 1 for t in range(nt)):
                seen.add("an address clamp at Mrows - 1")
            if n < s.T and s.q_row0 + s.Sq > n:
                seen.add("queries behind the row's last key")
        if any(q * 128 + wv * 32 >= s.Sq for q in range(nq) for wv in range(4)):
            seen.add("a wave with no query")
        if s.Sq - (nq - 1) * 128 == 1:
            seen.add("a query block with one query")
        if None in wgs:
            seen.add("idle workgroups")
        if pairs8 > 8 and nq > 1:
            seen.add("more than one round of pairs with nq > 1")
        if pairs8 >= 24:
            seen.add("three rounds of pairs")
        if s.B * s.H == 8 and nq == 3:
            seen.add("exactly eight pairs, three query blocks")
        if s.q_row0 > 0 and s.q_row0 % 2:
            seen.add("q_row0 > 0, odd")
        if s.q_row0 > 0 and s.q_row0 % 32 == 16:
            seen.add("q_row0 > 0, not a tile multiple")
        seen.add("padding rows" if s.pad_rows else "Mrows == B T")
        seen.add("kend NULL" if s.kend is None else "kend given")
        seen.add("columns q, k, v from 0" if not s.alt_cols else "columns v, q, k from 16")
        seen.add(f"output {s.out}")
        assert s.o_ts > s.d
    for form in ac.FORMS:
        seen.add(f"form x{form}")
    want = {"ntiles 0", "ntiles 1", "ntiles 2", "ntiles 3", "ntiles 4", "ntiles 5 or more", "last tile masked", "last tile unmasked",
            "a wave with no query", "a query block with one query", "idle workgroups", "more than one round of pairs with nq > 1",
            "three rounds of pairs", "exactly eight pairs, three query blocks", "q_row0 > 0, odd", "q_row0 > 0, not a tile multiple",
            "an address clamp at Mrows - 1", "padding rows", "Mrows == B T", "kend NULL", "kend given", "kend clamped to T",
            "a row with a single key", "queries behind the row's last key", "columns q, k, v from 0", "columns v, q, k from 16",
            "output rows", "output planes", "output both", "form x3", "form x1"}
    assert want <= seen, sorted(want - seen)


def test_table_is_the_issue_s():
    """the shapes as listed, none larger than 2 x 4 x 300 x 300"""
    t = {s.name: (s.B, s.H, s.T, s.q_row0, s.Sq, s.kend) for s in ac.SHAPES}
    assert t["t5"] == (1, 1, 5, 0, 5, None) and t["t32"][:3] == (1, 2, 32) and t["t33"] == (2, 1, 33, 0, 33, (33, 1))
    assert t["t65"] == (2, 2, 65, 0, 65, (65, 64)) and t["t97"][:3] == (1, 3, 97) and t["t97k96"][5] == (96,)
    assert t["t129"] == (3, 3, 129, 0, 129, (129, 200, 0)) and t["b17"][:3] == (17, 1, 40) and t["t300"] == (2, 4, 300, 0, 300, (300, 293))
    assert t["tail65"][2:] == (200, 65, 135, (200, 137)) and t["tail144"][2:] == (200, 144, 56, (200, 137))
    assert max(s.B * s.H * s.Sq * s.T for s in ac.SHAPES) == 2 * 4 * 300 * 300
    for s in ac.SHAPES:
        if s.alt_cols:
            assert s.ncols == 3 * s.d + 32 and s.cols == (16 + s.d, 16 + 2 * s.d, 16)
        else:
            assert s.ncols == 3 * s.d and s.cols == (0, s.d, 2 * s.d)


def test_edge_keys():
    assert ac.edge_keys(ac.SHAPE["t5"], 0) == [0, 4]                                           # no row 5 in the planes
    assert ac.edge_keys(ac.SHAPE["t33"], 0) == [0, 31, 32, 33] and ac.edge_keys(ac.SHAPE["t33"], 1) == [0, 1]
    assert ac.edge_keys(ac.SHAPE["t65"], 1) == [0, 31, 32, 63, 64]
    assert ac.edge_keys(ac.SHAPE["t97"], 0) == [0, 31, 32, 63, 64, 95, 96]
    assert ac.edge_keys(ac.SHAPE["t129"], 0) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 129] and ac.edge_keys(ac.SHAPE["t129"], 2) == []
    assert ac.edge_keys(ac.SHAPE["tail65"], 1) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 136, 137]
    e = ac.edge_keys(ac.SHAPE["t300"], 1)
    assert e[-3:] == [288, 292, 293] and 95 in e and 127 in e and len(e) == 21


def test_layout_round_trip():
    assert ac.plane_index(3, 37, 5) == (2 * 5 + 3) * 16 + 5 == 213 and ac.plane_elems(5, 40) == 3 * 5 * 16
    x = ac.natural_matrix(ac.SHAPE["t33"])
    p = ac.pack(x)
    rows, cols = x.shape
    assert p.shape == (2 * ac.plane_elems(rows, cols),) and p.dtype == np.uint16
    hi, lo = ac.split(x)
    assert np.array_equal(ac.unpack(p, rows, cols), hi + lo) and np.abs(hi + lo - x).max() <= 2.0 ** -16 * 1.7
    hb, lb = ac.unpack_bits(p, rows, cols)
    assert np.array_equal(ac.bf16_widen(hb), hi) and np.array_equal(ac.bf16_widen(lb), lo)
    assert p[ac.plane_index(7, 21, rows)] == ac.bf16_bits(x[7, 21]) and p[ac.plane_elems(rows, cols) + ac.plane_index(7, 21, rows)] == lb[7, 21]
    # on values a split can hold, pack then unpack is the identity (the bits may differ at a tie: hi + lo has two splits there)
    assert np.array_equal(ac.unpack(ac.pack(hi + lo), rows, cols), hi + lo)
    # round to nearest even at a tie: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert ac.bf16_bits(np.float32(1 + 2.0 ** -8)) == 0x3F80 and ac.bf16_bits(np.float32(1 + 3 * 2.0 ** -8)) == 0x3F82
    xa = ac.natural_matrix(ac.SHAPE["t32"])
    ha, la = ac.unpack_bits(ac.pack(xa), *xa.shape)
    assert (ha[:, :16] == ac.NAN_BITS).all() and (la[:, -16:] == ac.NAN_BITS).all() and np.isnan(ac.bf16_widen(np.uint16(ac.NAN_BITS)))
    assert np.isfinite(xa[:, 16:-16]).all()


@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES])
def test_sensitivity_and_restatement(shape):
    s = ac.SHAPE[shape]
    nmax = max(s.keys(b) for b in range(s.B))
    for kind in ac.KINDS:
        for form in ac.FORMS:
            c = ac.case(shape, kind, form)
            rmax = float(np.abs(c.ref).max())
            assert np.isfinite(c.ref).all() and np.isfinite(c.err32)
            if form == 3:
                # (c) the three-product arithmetic against float64 on hi + lo: the dropped lo . lo products (2^-18 of a score's |q_i k_i|
                # mass) and 3 x 64 + 2 fp32 roundings per score, entering the weights twice (by itself and through the maximum); P as
                # hi + lo and the dropped pl . vl (2^-18 each, numerator and denominator); nmax + 1 roundings per sum over the keys; 64 for
                # v_exp_f32, its argument's fma and the division
                premise = c.vmax * (2 * c.score_mass * (2.0 ** -18 + 2.0 ** -24 * (3 * 64 + 2)) + 4 * 2.0 ** -18 + 2.0 ** -24 * (2 * nmax + 64))
                assert c.err32 <= premise, f"{c.id}: float32 restatement {c.err32:.3e} from float64 (> {premise:.3e})"
                assert c.bound == max(4 * c.err32, 2 * ac.ulp32(c.vmax))
                assert c.bound < 1e-4 * max(1.0, rmax), f"{c.id}: bound {c.bound:.3e} above the project's ceiling for this arithmetic"
            else:
                assert c.bound == 2.0 ** -8 * c.vmax + 1e-5
                assert c.err32 <= c.bound, f"{c.id}: one-product restatement {c.err32:.3e} beyond its bound {c.bound:.3e}"
            print(f"{c.id:<22} float32 restatement error {c.err32:.3e}  bound {c.bound:.3e}  score mass {c.score_mass:6.2f}")
            xv = ac.held_values(c.x, form)
            if kind == "zero_q":
                for b in range(s.B):
                    for h in range(s.H):
                        _, _, V = ac.head_operands(s, xv, b, h)
                        n = s.keys(b)
                        mean = V[:n].astype(np.float64).mean(axis=0) if n else np.zeros(64)
                        assert np.abs(c.ref[b, :, 64 * h:64 * h + 64] - mean[None]).max() <= 1e-15
            if kind == "natural" or (kind == "zero_q" and form == 1):
                continue
            # (b)
            for b in range(s.B):
                edges = ac.edge_keys(s, b)
                n = s.keys(b)
                if n == 0:
                    assert not c.ref[b].any() and not edges
                    continue
                for h in range(s.H):
                    if kind == "needle":
                        queries, js = np.arange(s.Sq), c.target[b, h]
                        assert set(js.tolist()) <= set(edges)
                        if s.Sq >= len(edges):      # every edge key of the row is some query's needle
                            assert set(js.tolist()) == set(edges), (c.id, b, h)
                            for blk in range(s.Sq // 128):
                                assert set(js[blk * 128:blk * 128 + 128].tolist()) == set(edges)
                    else:
                        queries, js = np.zeros(len(edges), np.int64), np.asarray(edges)
                    want = c.ref[b, :, 64 * h:64 * h + 64][queries]
                    vis = js < n
                    for name, mult, sel in (("removed", 0.0, vis), ("counted twice", 2.0, vis & (n > 1)), ("counted although behind kend", 1.0, ~vis)):
                        if not sel.any():
                            continue
                        got = ac.perturbed(c, b, h, queries[sel], js[sel], mult)
                        gap = np.abs(got - want[sel]).max(axis=1)
                        worst = int(np.argmin(gap))
                        assert gap[worst] >= 8 * c.bound, (f"{c.id} row {b} head {h} query {queries[sel][worst]}: key {js[sel][worst]} {name} moves "
                                                           f"the reference by {gap[worst]:.3e} < 8 x {c.bound:.3e}")


def test_natural_inputs_alone_could_not_carry_the_condition():
    """why the needle kind exists: on natural inputs the last of 293 keys moves the reference by less than the one-product bound"""
    c = ac.case("t300", "natural", 1)
    n = c.shape.keys(1)
    got = ac.perturbed(c, 1, 0, np.arange(c.shape.Sq), np.full(c.shape.Sq, n - 1), 0.0)
    gap = np.abs(got - c.ref[1, :, :64]).max(axis=1)
    print(f"t300 natural: key {n - 1} removed moves the reference by {gap.min():.3e} .. {gap.max():.3e}; one-product bound {c.bound:.3e}")
    assert gap.min() < c.bound
