"""CPU: the case table of tests/gemv_cases.py, checked through the library's own plan functions (idxtts_gemv_fx_plan_query /
idxtts_gemv_pl_plan_query: gemv_fx_make_plan, gemv_fx_ksb, gemv_pl_plan -- no GPU work), and its float64 reference.

The table has to reach every one of the 44 gemv_fx instantiations, every gemv_pl one that a GPT shape can select, and the edge classes
of the K split; the reference has to be decided (no step of any case closer to a tie than the tolerance the GPU file applies), so that
"greedy codes equal the reference's" is a statement about the kernels and not about a coin."""
import pytest

import gemv_cases as gc
from indextts_amd import _lib


def _case_launches(c):
    model, fmt, rows, plane_rows, narrow = c
    d, _, _, V = gc.model_dims(model)
    return gc.launches(d, V, fmt, rows, plane_rows, narrow)


def test_plan_query_names_the_documented_geometry():
    """The query against what csrc/gemv16.h and csrc/gemv_pl.h say of the production shapes: d = 1280 runs 16 waves x 5 chunks in one
    batch, mlp.c_proj split over 4 workgroups; 8 x 10 in the narrow form; c_fc two column tiles per wave; the plane GEMV 4 K parts at
    K = 1280 and CT 4 -> 8 for mel_head at 17 rows."""
    p = _lib.gemv_fx_plan(3840, 1280, 16, 1)
    assert (p["mt"], p["ntw"], p["single"], p["r4"], p["narrow"], p["kw"], p["cps"], p["ksb"]) == (1, 1, 1, 0, 0, 16, 5, 1)
    p = _lib.gemv_fx_plan(1280, 5120, 16, 2, with_slab=True)
    assert (p["kw"], p["cps"], p["ksb"], p["single"]) == (16, 5, 4, 1)
    assert _lib.gemv_fx_plan(1280, 5120, 16, 2, with_slab=False)["ksb"] == 1
    p = _lib.gemv_fx_plan(1280, 5120, 16, 2, with_slab=True, narrow=True)
    assert (p["narrow"], p["kw"], p["cps"], p["ksb"]) == (1, 8, 10, 4)
    assert _lib.gemv_fx_plan(1280, 5120, 16, 0, with_slab=True, narrow=True)["narrow"] == 0      # fp32 streams keep the 16-wave form
    assert _lib.gemv_fx_plan(5120, 1280, 16, 0)["ntw"] == 2 and _lib.gemv_fx_plan(5120, 1280, 33, 0)["ntw"] == 1
    assert _lib.gemv_fx_plan(1280, 1280, 4, 0)["r4"] == 1 and _lib.gemv_fx_plan(1280, 1280, 5, 0)["r4"] == 0
    assert _lib.gemv_pl_plan(3840, 1280, 16) == {"ct": 4, "kparts": 4, "has_kernel": True}
    assert _lib.gemv_pl_plan(8194, 1280, 16)["ct"] == 4 and _lib.gemv_pl_plan(8194, 1280, 17)["ct"] == 8
    assert _lib.gemv_pl_plan(1280, 5120, 64) == {"ct": 8, "kparts": 32, "has_kernel": True}
    with pytest.raises(RuntimeError):
        _lib.gemv_fx_plan(1280, 1280, 65, 0)
    with pytest.raises(RuntimeError):
        _lib.gemv_pl_plan(1280, 1280, 0)


def test_table_reaches_every_gemv_fx_instantiation():
    want = gc.all_fx_keys()
    assert len(want) == 44
    got = {}
    for c in gc.CASES:
        for layer, N, K, kind, plan in _case_launches(c):
            if kind == "fx":
                got.setdefault(gc.fx_key(plan, c[1]), (gc.case_id(c), layer))
    assert set(got) <= want, f"a plan outside the 44: {set(got) - want}"
    assert set(got) == want, f"not launched by any case: {sorted(want - set(got))}"
    print(f"\n{len(got)} of 44 gemv_fx instantiations (MT, NTW, one batch, format, R4, narrow) -> first case, layer")
    for k in sorted(got):
        print(f"  {k}: {got[k][0]} {got[k][1]}")


def _reachable_pl():
    """Every gemv_pl (MT, CT, format) that the decode step of a GPT with head_dim 64, d <= 1344, V <= 8194 and <= 64 rows selects: swept
    through the query (the plan depends on the rows through their 16-row tiles and on V through its 16-column tiles)."""
    reach, no_kernel = set(), set()
    for d in range(64, 1344 + 1, 64):
        for V in list(range(16, 8193, 16)) + [8194]:
            for rows in (16, 32, 48, 64):
                plans = [_lib.gemv_pl_plan(N, K, rows) for _, N, K, _ in gc.shapes(d, V)]
                if all(p["has_kernel"] for p in plans):      # GPTModel::use_pl: otherwise the step stays on gemv_fx
                    reach |= {(rows // 16, p["ct"]) for p in plans}
                else:
                    no_kernel |= {(d, rows, p["ct"], p["kparts"]) for p in plans if not p["has_kernel"]}
    return reach, no_kernel


def test_table_reaches_every_reachable_gemv_pl_instantiation():
    reach, no_kernel = _reachable_pl()
    got = {}
    for c in gc.CASES:
        for layer, N, K, kind, plan in _case_launches(c):
            if kind == "pl":
                assert plan["has_kernel"]
                got.setdefault(gc.pl_key(plan, c[1], c[2]), (gc.case_id(c), layer))
    want = {(mt, ct, fmt) for mt, ct in reach for fmt in ("bf16", "fp8")}
    assert set(got) <= want
    assert set(got) == want, f"not launched by any case: {sorted(want - set(got))}"
    # the 20 instantiations pl_launch_ct holds: every (MT, CT) whose LDS footprint fits, in two formats
    every = {(mt, ct) for ct, mts in ((1, (1,)), (2, (1, 2)), (4, (1, 2, 3)), (8, (1, 2, 3, 4))) for mt in mts}
    assert reach <= every and 2 * len(every) == 20
    print(f"\n{len(got)} gemv_pl instantiations (MT, CT, format) reachable and launched -> first case, layer")
    for k in sorted(got):
        print(f"  {k}: {got[k][0]} {got[k][1]}")
    print(f"reachable only with the CT override (each in bf16 and fp8): {sorted(every - reach)}")
    print(f"plans without a kernel, kept on gemv_fx (d, rows, ct, kparts): {sorted(no_kernel)[:4]} ... {len(no_kernel)} in all")
    # the 49..64-row decodes of a compact model wider than d = 1280: no plane kernel, and the table runs them on gemv_fx
    assert no_kernel and all(d > 1280 and rows == 64 and ct == 4 for d, rows, ct, _ in no_kernel)
    for c in (("d1344", "bf16", 64, 17, False), ("d1344", "fp8", 49, 17, False)):
        assert c in gc.CASES and {kind for _, _, _, kind, _ in _case_launches(c)} == {"fx"}
        assert not _lib.gemv_pl_plan(1344, 4 * 1344, c[2])["has_kernel"]


def test_table_has_every_edge_class():
    got = {}
    for c in gc.CASES:
        model, fmt, rows, plane_rows, narrow = c
        d, _, _, V = gc.model_dims(model)
        for e in gc.edge_classes(d, V, fmt, rows, plane_rows, narrow):
            got.setdefault(e, []).append(gc.case_id(c))
            if e == "pl:k-remainder":
                got.setdefault(f"{e}@{model}", []).append(gc.case_id(c))
    want = ["fx:empty-wave-slice", "fx:empty-k-piece-workgroup", "fx:kw<16", "fx:cps1", "fx:cps2", "fx:cps5", "fx:cps6", "fx:cps10",
            "pl:kparts1", "pl:kparts2", "pl:kparts4", "pl:kparts8", "pl:kparts16", "pl:kparts32",
            "pl:k-remainder@d192", "pl:k-remainder@d1344", "fx:N%16", "pl:N%16"]
    print()
    for e in want:
        assert e in got, f"no case has {e}"
        print(f"  {e}: {got[e][0]}" + (f" (+{len(got[e]) - 1})" if len(got[e]) > 1 else ""))
    # the narrow geometry at both ends of its row range, in both compact formats
    for fmt in ("bf16", "fp8"):
        for rows in (5, 16):
            plans = [p for _, _, _, kind, p in _case_launches(("d1280", fmt, rows, 17, True)) if kind == "fx"]
            assert ("d1280", fmt, rows, 17, True) in gc.CASES and len(plans) == 5 and all(p["narrow"] for p in plans)


def test_case_rows_and_switches_are_legal():
    for c in gc.CASES:
        model, fmt, rows, plane_rows, narrow = c
        assert model in gc.MODELS and fmt in gc.FMT and 1 <= rows <= 64 and plane_rows in (5, 17, 65)
        d, heads, layers, V = gc.model_dims(model)
        assert d == 64 * heads and layers in (1, 2) and gc.L_TEXT <= 6 and 4 <= gc.NEW <= 6
        assert not narrow or (d == 1280 and 5 <= rows <= 16)
    assert len(set(gc.CASES)) == len(gc.CASES)


@pytest.mark.parametrize("model,fmt", sorted({(c[0], c[1]) for c in gc.CASES}))
def test_reference_is_decided(model, fmt):
    """The float64 oracle's greedy codes equal the float32 oracle's on every row any case uses (where they part, the float32 oracle's
    margin there has to be a near-tie -- and the inputs are chosen so that there is none: no step of any row has a top-2 margin below
    the tolerance the GPU file allows a kernel)."""
    import numpy as np
    from oracle import gpt as og
    import torch
    r = gc.reference(model, fmt)
    R = r.rows
    tol, err = r.tolerance(R), r.oracle_error(R)
    margins = r.margins()
    print(f"\n{model} {fmt}: {R} rows x {r.codes.shape[1]} steps, float32 oracle error {err:.2e}, tolerance {tol:.2e}, "
          f"largest |logit| {float(r.logits.abs().max()):.2f}, smallest top-2 margin {float(margins.min()):.2e}")
    assert r.codes.shape == (R, gc.NEW) and r.logits.shape == (R, gc.NEW, gc.model_dims(model)[3]) and r.logits.dtype == torch.float64
    n = min(r.codes.shape[1], r.codes32.shape[1])
    for b in range(R):
        d = np.nonzero((r.codes[b, :n] != r.codes32[b, :n]).numpy())[0]
        if len(d):
            s = int(d[0])
            ids = torch.cat([r.fake[b], r.codes32[b, :s]])[None]
            sc = og.repetition_penalty(ids, r.logits32[b, s][None], gc.PENALTY)[0]
            m32 = float(sc[int(r.codes32[b, s])] - sc[int(r.codes[b, s])])
            print(f"  row {b} parts at step {s}: float32 margin {m32:.3e}")
            assert 0.0 <= m32 <= tol
    assert torch.equal(r.codes, r.codes32) and r.codes32.shape[1] == r.codes.shape[1]
    assert err > 0.0 and tol >= 4.0 * err
    assert float(margins.min()) > 2.0 * tol, "a step closer to a tie than the kernels' tolerance: choose another input tag"
