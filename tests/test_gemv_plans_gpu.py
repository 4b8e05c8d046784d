"""GPU: every instantiation of the decode GEMVs (csrc/gemv_fx.hip, csrc/gemv_pl.hip) on the cases of tests/gemv_cases.py -- small GPTs whose
width, vocabulary, weight format, row count and process-wide switches make the decode step launch each kernel, on each split of K
(tests/test_gemv_cases_cpu.py proves the coverage through the library's own plan functions).

  * against float64: teacher-forced logits of every case against the float64 oracle on the rounded model, fp32 KV cache (nothing but
    the GEMVs and the attention rounds); the bound is 4 x the float32 CPU oracle's own error on the same rows (both accumulate in fp32,
    in different orders), never below one fp32 ulp of the largest logit; greedy codes, graph-replayed and eager, equal the reference's;
  * exact, formats: a bf16 / fp8 model on gemv_fx equals, bit for bit in every logit, an f32-format model loaded with the compact
    model's read-back weights (csrc/wstream.h: the compact kernels ARE the fp32 kernel on the dequantised matrix);
  * exact, plane geometry: a row's logits do not depend on the batch (16, 17, 33, 64 rows) or the geometry (CT, K parts) it selects;
  * the narrow geometry and the 49..64-row compact decode of a model wider than d = 1280 are cases of the table.

The file prints a table of (case, float32 oracle error, kernel error, ratio) with the worst ratio last (-s shows it)."""
import time

import numpy as np
import pytest
import torch

import gemv_cases as gc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu

_MODELS = {}
_REFS = {}
_TABLE = []
_T0 = time.time()


def _model(device, model, fmt, eff_of=None):
    """The case's model (fp32 KV cache); eff_of: an f32-format model loaded with the read-back weights of the `eff_of`-format one.
    The last few are kept: the parametrised cases come sorted by model."""
    from indextts_amd.gpt import UnifiedVoice
    key = (model, fmt, eff_of)
    if key not in _MODELS:
        while len(_MODELS) >= 4:
            _MODELS.pop(next(iter(_MODELS)))
        w = gc.original_weights(model) if eff_of is None else _model(device, model, eff_of).effective_state_dict
        _MODELS[key] = UnifiedVoice(w, gc.config(model), device=device, weight_format=fmt, keep_effective=True, kv_format="f32")
    return _MODELS[key]


def _reference(uv, model, fmt):
    """The float64 reference on the model the library read back (effective_state_dict).  That model is the one tests/gemv_cases.py
    derives on the host -- bf16 through the same library call, fp8 restated: equal weights, folded biases to a float32 rounding -- and
    then the reference is the one the CPU file has checked; otherwise it is computed from the read-back model itself."""
    key = (model, fmt)
    if key not in _REFS:
        eff, host = uv.effective_state_dict, gc.effective_weights(model, fmt)
        assert set(eff) == set(host)
        same = True
        for k in host:
            if k.endswith(".weight") or fmt != "fp8":
                assert np.array_equal(eff[k], host[k]), f"{model} {fmt}: {k} of the read-back model is not the documented rounding"
            else:
                assert np.all(np.abs(eff[k].astype(np.float64) - host[k]) <= np.spacing(np.abs(host[k]))), k
                same = same and np.array_equal(eff[k], host[k])
        _REFS[key] = gc.reference(model, fmt) if same else gc.Reference(model, fmt, eff=eff)
    return _REFS[key]


@pytest.fixture
def switches():
    """idxtts_set_decode_plane_rows / idxtts_set_decode_geometry for one test, the defaults restored behind it."""
    def set_(plane_rows, narrow=False):
        _lib.set_decode_plane_rows(plane_rows)
        _lib.set_decode_geometry(narrow)
    yield set_
    _lib.set_decode_plane_rows(0)
    _lib.set_decode_geometry(False)
    assert _lib.get_decode_plane_rows() == 17 and _lib.get_decode_geometry() is False


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if _TABLE:
        print(f"\n{'case':<28}{'oracle32 err':>14}{'kernel err':>14}{'ratio':>8}{'bound':>12}")
        for cid, oerr, kerr, tol in _TABLE:
            print(f"{cid:<28}{oerr:>14.3e}{kerr:>14.3e}{kerr / oerr:>8.2f}{tol:>12.3e}")
        worst = max(_TABLE, key=lambda r: r[2] / r[1])
        print(f"worst kernel error / float32 oracle error: {worst[2] / worst[1]:.2f} ({worst[0]}); {len(_TABLE)} cases")
    print(f"tests/test_gemv_plans_gpu.py wall time: {time.time() - _T0:.1f} s")
    _MODELS.clear()


def _generate(uv, model, rows, **kw):
    lat, emo, text = gc.inputs(model, rows)
    return uv.inference_speech(lat, text, emo_vec=emo, max_generate_length=gc.NEW, repetition_penalty=gc.PENALTY, **kw)


def _check_case(device, switches, c):
    model, fmt, rows, plane_rows, narrow = c
    uv = _model(device, model, fmt)
    ref = _reference(uv, model, fmt)
    switches(plane_rows, narrow)
    want = ref.codes[:rows]
    n = want.shape[1]
    codes, _ = _generate(uv, model, rows)
    eager, _ = _generate(uv, model, rows, use_graph=False)
    forced = torch.full((rows, gc.NEW), uv.cfg.stop_mel_token, dtype=torch.long)
    forced[:, :n] = want
    _, _, logits = _generate(uv, model, rows, return_logits=True, forced_codes=forced)
    kerr = float((logits.cpu()[:, :n].double() - ref.logits[:rows]).abs().max())
    oerr, tol = ref.oracle_error(rows), ref.tolerance(rows)
    print(f"\n{gc.case_id(c)}: float32 oracle error {oerr:.3e}, kernel error {kerr:.3e} ({kerr / oerr:.2f} x), bound {tol:.3e}")
    _TABLE.append((gc.case_id(c), oerr, kerr, tol))
    assert np.isfinite(kerr) and kerr <= tol, f"{gc.case_id(c)}: logits {kerr:.3e} from the float64 reference (> {tol:.3e})"
    assert np.array_equal(codes.cpu().numpy(), want.numpy()), f"{gc.case_id(c)}: graph-replayed codes differ from the reference's"
    assert torch.equal(eager, codes), f"{gc.case_id(c)}: eager launches differ from the replayed graph"


@pytest.mark.parametrize("case", sorted(gc.CASES), ids=gc.case_id)
def test_case_vs_float64(device, switches, case):
    _check_case(device, switches, case)


@pytest.mark.parametrize("case", [c for i, c in enumerate(sorted(gc.CASES)) if c[1] != "f32" and c[0] not in {x[0] for x in sorted(gc.CASES)[:i] if x[1] != "f32"}],
                         ids=gc.case_id)
def test_bf16_kv_cache_per_model(device, switches, case):
    """One compact case per model with the bf16 KV cache: codes equal the float32 oracle's with keys / values rounded the same way, or
    a row parts from it at a near-tie of the oracle (tests/test_gpt_gpu.py::_assert_equal_or_near_tie and its bounds)."""
    from test_gpt_gpu import _assert_equal_or_near_tie
    model, fmt, rows, plane_rows, narrow = case
    uv = _model(device, model, fmt)
    _reference(uv, model, fmt)                              # (the read-back model is the one the host derives)
    ref = gc.reference_kv16(model, fmt)
    switches(plane_rows, narrow)
    uv.set_kv_format("bf16")
    try:
        codes, _ = _generate(uv, model, rows)
        eager, _ = _generate(uv, model, rows, use_graph=False)
    finally:
        uv.set_kv_format("f32")
    flips = _assert_equal_or_near_tie(codes.cpu().numpy(), ref.codes32[:rows].numpy(), ref.logits32[:rows], ref.fake[:rows], 1e-2, gc.PENALTY)
    assert flips <= max(1, rows // 16) and torch.equal(eager, codes)


# one case per gemv_fx (MT, NTW, one batch | two buffers, R4) class: d128 has (1,1)/(1,2) one batch with and without R4 and (2,1)/(2,2),
# d64 (3,1) one batch, d1344 the two-buffer forms of MT 1 (NTW 1, 2; R4 and not), 2, 3 and 4
_FORMAT_ROWS = {"d128": (1, 5, 17), "d64": (33,), "d1344": (1, 5, 17, 33, 64)}


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("model", sorted(_FORMAT_ROWS))
def test_compact_format_equals_fp32_kernel_on_the_dequantised_matrix(device, switches, model, fmt):
    """csrc/wstream.h: a compact format changes what is read, not the arithmetic -- so with every step on gemv_fx (plane_rows 65) the
    logits of a bf16 / fp8 model equal bit for bit those of an f32-format model loaded with the compact model's read-back weights."""
    d, _, _, V = gc.model_dims(model)
    classes = set()
    for rows in _FORMAT_ROWS[model]:
        for kind, key in ((k, gc.fx_key(p, fmt)) for _, _, _, k, p in gc.launches(d, V, fmt, rows, 65, False)):
            assert kind == "fx"
            classes.add((key[0], key[1], key[2], key[4]))
    switches(65, False)
    for rows in _FORMAT_ROWS[model]:
        got = _generate(_model(device, model, fmt), model, rows, return_logits=True)
        want = _generate(_model(device, model, "f32", eff_of=fmt), model, rows, return_logits=True)
        assert got[2].shape[1] == gc.NEW and torch.equal(got[0], want[0]), (model, fmt, rows)
        diff = (got[2] - want[2]).abs().max().item()
        assert torch.equal(got[2], want[2]), f"{model} {fmt} {rows} rows: logits differ by up to {diff:.3e} from the fp32 kernel on the same matrix"
    print(f"\n{model} {fmt}: bitwise equal to the f32-format model at rows {_FORMAT_ROWS[model]}: classes (MT, NTW, one batch, R4) {sorted(classes)}")


def test_format_classes_cover_gemv_fx():
    """The rows of the test above reach every (MT, NTW, one batch | two buffers, R4) class of gemv_fx (a plan query; no GPU work)."""
    classes = set()
    for model, rows_list in _FORMAT_ROWS.items():
        d, _, _, V = gc.model_dims(model)
        for rows in rows_list:
            classes |= {(k[0], k[1], k[2], k[4]) for k in (gc.fx_key(p, "bf16") for _, _, _, _, p in gc.launches(d, V, "bf16", rows, 65, False))}
    assert classes == {(k[0], k[1], k[2], k[4]) for k in gc.all_fx_keys() if not k[5]} and len(classes) == 14


@pytest.mark.parametrize("model,fmt,batches", [("d1280", "bf16", ((16, 5), (17, 17), (33, 17), (64, 17))),
                                               ("d1344", "fp8", ((17, 17), (33, 17), (48, 17)))])
def test_plane_rows_do_not_depend_on_the_batch_or_geometry(device, switches, model, fmt, batches):
    """20 and 21 heads: every batch of 7 rows or more keeps the decode attention unsplit, so nothing but the plane GEMV's geometry
    (1 to 4 row tiles, CT 4 and 8, 4 to 32 K parts; at d = 1344 a short last K part) changes between the batches -- and the logits
    of the rows they share are the same bit for bit (csrc/gemv_pl.hip: CT 4 and CT 8 add the K groups in the same order)."""
    d, _, _, V = gc.model_dims(model)
    uv = _model(device, model, fmt)
    geoms = set()
    base = None
    for rows, plane_rows in batches:
        assert rows * gc.model_dims(model)[1] > 128
        ls = gc.launches(d, V, fmt, rows, plane_rows, False)
        assert all(kind == "pl" for _, _, _, kind, _ in ls)
        geoms |= {((rows + 15) // 16, p["ct"], p["kparts"]) for _, _, _, _, p in ls}
        switches(plane_rows, False)
        codes, _, logits = _generate(uv, model, rows, return_logits=True)
        if base is None:
            base = (rows, codes, logits)
            continue
        k = base[0]
        assert torch.equal(codes[:k], base[1]), (model, rows)
        diff = (logits[:k] - base[2]).abs().max().item()
        assert torch.equal(logits[:k], base[2]), f"{model} {fmt}: rows 0..{k - 1} differ by up to {diff:.3e} between batches of {k} and {rows}"
    assert len({g[1] for g in geoms}) == 2 and len(geoms) >= 6
    print(f"\n{model} {fmt}: rows bitwise equal across batches {[b[0] for b in batches]}; geometries (MT, CT, K parts) {sorted(geoms)}")


@pytest.mark.parametrize("case", [("d1344", "bf16", 64, 17, False), ("d1344", "fp8", 49, 17, False)], ids=gc.case_id)
def test_wide_compact_model_decodes_49_to_64_rows(device, switches, case):
    """K = 5376 at 49..64 rows: the plane plan's CT = 4 has no kernel at four row tiles and CT = 8 would need 34 > 32 K parts, so such a
    decode stays on gemv_fx (GPTModel::use_pl): it generates, equals the reference, and runs the kernels it runs with the plane path off."""
    model, fmt, rows, plane_rows, _ = case
    d, _, _, V = gc.model_dims(model)
    assert case in gc.CASES and rows >= plane_rows
    assert not _lib.gemv_pl_plan(d, 4 * d, rows)["has_kernel"] and not gc.use_pl(d, V, fmt, rows, plane_rows)
    switches(plane_rows, False)
    uv = _model(device, model, fmt)
    codes, _ = _generate(uv, model, rows)
    assert np.array_equal(codes.cpu().numpy(), _reference(uv, model, fmt).codes[:rows].numpy())
    switches(65, False)                       # the same kernels as with the plane path off
    off, _ = _generate(uv, model, rows)
    assert torch.equal(off, codes)
