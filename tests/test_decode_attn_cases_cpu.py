"""CPU: the case table of tests/decode_attn_cases.py, checked with the reference alone (no library call).

  (a) coverage     through the restated piece and split rules, some case reaches every edge of decode_attn_body's control flow;
  (b) sensitivity  for every natural and needle case and every edge index, the float64 reference with that key removed, and with it
                   counted twice, is at least 8 x the case's bound away from the reference: a kernel that drops or doubles one such key
                   cannot pass tests/test_decode_attn_gpu.py.  A condition on the inputs, not a measurement;
  (c) restatement  the float32 restatement that sets each bound is finite and within an a-priori rounding bound of the float64
                   reference; its error is printed per case (-s)."""
import numpy as np
import pytest

import decode_attn_cases as dc

PV_STRIDE = {"f32": 256, "bf16": 512, "fp8": 512}       # keys per pass of the P.V loop behind the 128-key prefetch


def _rows():
    """(shape, row, keys, config, pieces, workgroups) of every live row of every shape under every config."""
    for s in dc.SHAPES:
        for ns, inv in dc.CONFIGS:
            used = dc.resolve_nsplit(ns, inv, s.B, s.H, s.Smax)
            for b in range(s.B):
                if s.live[b]:
                    n = s.n_keys(b)
                    pcs, wgs = dc.row_pieces(n, used, inv)
                    yield s, b, n, (ns, inv, used), pcs, wgs


def test_table_reaches_every_edge_of_the_control_flow():
    seen = set()
    for s, b, n, (ns, inv, used), pcs, wgs in _rows():
        lens = [e - a for a, e in pcs]
        assert sum(lens) == n and all(a2 == e1 or a2 >= n for (_, e1), (a2, _) in zip(pcs, pcs[1:]) if e1 < n), (s.name, b, ns, inv)
        assert 1 <= used <= 16 and len(pcs) <= 16
        if 0 in lens:
            seen.add("empty piece")
        for a, e in pcs:
            if a == n - 1 and e == n:
                seen.add("a piece holding only the new token")
                if n > 1:
                    seen.add("the new token as the first key of a later piece")
            if e - a > 512:
                seen.add("second score pass")
            if e - a > 128 + PV_STRIDE[s.fmt]:
                seen.add(f"P.V loop past one stride, {s.fmt}")
            if 128 < e - a <= 128 + PV_STRIDE[s.fmt]:
                seen.add(f"P.V loop of one stride, {s.fmt}")
            if 0 < e - a <= 128:
                seen.add(f"prefetch only, {s.fmt}")
        if inv:
            if len(pcs) > wgs:
                seen.add("invariant: a workgroup walks two pieces")
            if len(pcs) > 1 and used > len(pcs):
                seen.add("invariant: more workgroups than pieces")
            if len(pcs) > 1 and used == 1:
                seen.add("invariant: one workgroup walks every piece")
            seen.add(f"invariant merge of {len(pcs)}")
        elif used == 16 and min(lens) > 0:
            seen.add("merge of 16 pieces")
        seen.add(f"{s.fmt} {s.mode} inv{inv}")
    want = {"empty piece", "a piece holding only the new token", "the new token as the first key of a later piece", "second score pass",
            "invariant: a workgroup walks two pieces", "invariant: more workgroups than pieces", "invariant: one workgroup walks every piece",
            "merge of 16 pieces"}
    want |= {f"{k}, {f}" for f in dc.FMT for k in ("P.V loop past one stride", "P.V loop of one stride", "prefetch only")}
    want |= {f"invariant merge of {k}" for k in (1, 2, 3, 4, 5)}
    want |= {f"{f} {m} inv{i}" for f in dc.FMT for m in ("state", "slots") for i in (0, 1)}      # the twelve kernels
    assert want <= seen, sorted(want - seen)


def test_every_nsplit_is_the_rule_of_some_batch():
    """Every nsplit of the table is what decode_attn_nsplit gives for some batch of the real model (20 heads) or a tiny one (2, 3)."""
    rule = {dc.split_rule(B, H): (B, H) for H in (3, 2, 20) for B in range(64, 0, -1)}
    assert set(dc.NSPLITS) <= set(rule), sorted(set(dc.NSPLITS) - set(rule))
    assert [dc.split_rule(B, 20) for B in (1, 2, 3, 4, 5, 6, 7)] == [12, 6, 4, 3, 2, 2, 1]      # the real model's small batches
    assert dc.split_rule(8, 2) == 16 and dc.split_rule(64, 2) == 2 and dc.split_rule(65, 2) == 1
    print({ns: rule[ns] for ns in dc.NSPLITS})


def test_table_holds_the_variations():
    names = {s.name for s in dc.SHAPES}
    for n in dc.N_VALUES:
        for fmt in dc.FMT:
            assert {f"n{n}-{fmt}-state", f"n{n}-{fmt}-slots", f"n{n}-{fmt}-state-b1"} <= names
    assert {s.n_keys(0) for s in dc.MAIN_SHAPES if s.mode == "state"} == set(dc.N_VALUES)
    assert any(s.H == 3 for s in dc.SHAPES) and any(s.fan == 3 for s in dc.SHAPES)
    for s in dc.MAIN_SHAPES:
        if s.mode == "state":
            assert len(set(s.pos)) == 1 and s.kstart[0] == 0 and s.kstart[2] == s.pos[2]           # a row that sees only its new token
            assert s.pos[0] < 2 or 0 < s.kstart[1] < s.pos[1] or s.pos[1] <= 2                        # ragged left padding
        else:
            assert s.live.count(0) == 1 and list(s.slot_ids) != sorted(s.slot_ids) and set(s.kstart) == {0}
            assert s.pos[2] == s.lens[0] == dc.SHAPE[s.name.replace("slots", "state")].pos[0]       # the main row at an equal position
        assert all(0 <= k <= p < s.Smax for k, p, l in zip(s.kstart, s.pos, s.live) if l) and s.S <= s.Smax
    # nothing the product never passes: one c_attn part, no bias -- the probe has no such parameter -- and at most 2449 keys
    assert max(s.n_keys(b) for s in dc.SHAPES for b in range(s.B)) == 2449 < 8192


def test_restated_layout_round_trip():
    """stored() places position s of (row, head) where the comments of decode.h say: K granule c of position s at [c][s], V rows whole."""
    s = dc.SHAPE["n17-bf16-slots"]
    st = dc.stored(s)
    assert st.kcache.shape == (4, 2, 8, s.Smax, 8) and st.vcache.shape == (4, 2, s.Smax, 64) and st.kcache.dtype == np.uint16
    sent = np.uint16(dc.SENTINEL * 0x0101)
    assert (st.kcache[1] == sent).all() and (st.vcache[1] == sent).all()                             # the dead slot: untouched
    for b, ln in ((2, s.lens[0]), (0, s.lens[1]), (3, s.lens[2])):
        assert (st.kcache[b, :, :, ln + 1:, :] == sent).all() and (st.vcache[b, :, ln + 1:] == sent).all()
        k = dc.bf16_widen(st.kcache[b].transpose(0, 2, 1, 3).reshape(2, s.Smax, 64)[:, :ln + 1])
        assert np.array_equal(k, st.K[b]) and np.array_equal(dc.bf16_widen(st.vcache[b, :, :ln + 1]), st.V[b])
    f = dc.stored(dc.SHAPE["n17-f32-state"])
    assert f.kcache.shape == (3, 2, 16, 28, 4) and f.kcache.dtype == np.float32 and f.kscale is None
    q = dc.stored(dc.SHAPE["n17-fp8-state"])
    assert q.kcache.dtype == np.uint8 and q.kscale.shape == (3, 2, 28)
    img = np.arange(dc.frag_floats(5, 128), dtype=np.float32)
    rows = dc.unfrag(img, 5, 128)
    assert rows.shape == (5, 128) and len(np.unique(rows)) == 5 * 128 and rows[3, 37] == dc.frag_index(3, 37, 8)


@pytest.mark.parametrize("shape", [s.name for s in dc.SHAPES])
def test_sensitivity_and_restatement(shape):
    s = dc.SHAPE[shape]
    for kind in dc.KINDS:
        c = dc.case(shape, kind)
        n = max(s.n_keys(b) for b in range(s.B))
        # (c) a float32 evaluation in any order: a score within 64 roundings of its |q_i k_i| mass (entering the weight twice, by itself
        # and through the maximum), n + 1 roundings per sum over the keys, a few for expf, the products and the division
        premise = 2.0 ** -24 * c.vmax * (2 * 64 * c.score_mass + 2 * n + 16)
        assert np.isfinite(c.ref).all() and c.err32 <= premise, f"{c.id}: float32 restatement {c.err32:.3e} from float64 (> {premise:.3e})"
        assert c.bound >= 4 * c.err32 and c.bound < 2e-5
        print(f"{c.id:<34} launches {c.step_qkv.shape[0]:>3}  float32 error {c.err32:.3e}  bound {c.bound:.3e}")
        if kind == "zero_q":
            for b in range(s.B):
                if s.live[b]:
                    mean = np.stack([v.astype(np.float64).mean(axis=0) for v in dc.stored(s).V[b]]).reshape(-1)
                    assert np.abs(c.ref[0, b] - mean).max() <= 1e-15
            continue
        # (b)
        for b in range(s.B):
            if not s.live[b]:
                assert not c.ref[:, b].any()
                continue
            edges = dc.edge_indices(s.n_keys(b))
            for h in range(s.H):
                for l in range(c.step_qkv.shape[0]):
                    js = edges if kind == "natural" else [int(c.target[l, b, h])]
                    removed, doubled = dc.perturbed(c, l, b, h, js)
                    want = c.ref[l, b, h * 64:(h + 1) * 64]
                    for name, got in (("removed", removed), ("counted twice", doubled)):
                        if s.n_keys(b) == 1 and name == "counted twice":
                            continue                      # the only key twice is the same mean
                        gap = np.abs(got - want[None]).max(axis=1)
                        worst = int(np.argmin(gap))
                        assert gap[worst] >= 8 * c.bound, (f"{c.id} row {b} head {h} launch {l}: key {js[worst]} {name} moves the reference by "
                                                           f"{gap[worst]:.3e} < 8 x {c.bound:.3e}")
        if kind == "needle":      # every edge index of every row is some launch's needle
            for b in range(s.B):
                if s.live[b]:
                    assert set(c.target[:, b].reshape(-1).tolist()) == set(dc.edge_indices(s.n_keys(b)))
