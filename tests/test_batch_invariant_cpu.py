"""No GPU: the launch policy of the batch-invariant mode (`idxtts_gpt_set_batch_invariant`), from the library's own plan query
(`idxtts_batch_invariant_plan_query`, host only), and the merge rule of the serving layer in the mode.

What decides a row's bits -- which GEMV family runs, how K is cut into slices, chunks and pieces; into how many pieces a row's keys
are cut and how long they are -- must not depend on the number of rows or on B.  What may follow them is how much is launched: row
tiles (mt), column tiles per wave (ntw), one or two register batches (single), workgroups per (row, head)."""
import itertools
import types

import pytest

from indextts_amd import _lib
from indextts_amd.config import GPTConfig

D, V, HEADS = 1280, 8194, 20
# the five GEMVs of a decode step: (layer, N, K, with_slab)
STEP = [("c_attn", 3 * D, D, False), ("c_proj", D, D, False), ("c_fc", 4 * D, D, False), ("mlp.c_proj", D, 4 * D, True),
        ("mel_head", V, D, False)]
ORDER = _lib.BATCH_INVARIANT_ORDER_FIELDS


@pytest.fixture
def switches():
    yield
    _lib.set_decode_geometry(False)
    _lib.set_decode_plane_rows(0)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["f32", "bf16", "fp8"])
@pytest.mark.parametrize("layer,N,K,slab", STEP, ids=[s[0] for s in STEP])
def test_gemv_order_is_constant_over_rows_and_batch(switches, layer, N, K, slab, fmt):
    seen = set()
    for narrow, plane in ((False, 0), (True, 5)):      # the process-wide switches must not reach the plan
        _lib.set_decode_geometry(narrow)
        _lib.set_decode_plane_rows(plane)
        for rows in range(1, 65):
            for B in (1, 7, 64):
                p = _lib.batch_invariant_plan(N, K, rows, fmt, slab, B=B, heads=HEADS, smax=2048, n_keys=700)
                seen.add(tuple(p[f] for f in ORDER))
                assert p["mt"] == (rows + 15) // 16
    assert len(seen) == 1, f"{layer}: the summation order depends on rows, B or a process switch: {sorted(seen)}"
    order = dict(zip(ORDER, seen.pop()))
    assert order["family"] == 0 and order["r4"] == 0 and order["narrow"] == 0      # the fp32-MFMA GEMV, its 16-row-tile forms only
    want = _lib.gemv_fx_plan(N, K, 16, fmt, slab, False)                          # ... cut as that GEMV cuts K at 16 rows today
    assert (order["kw"], order["cps"], order["ksb"]) == (want["kw"], want["cps"], want["ksb"])


def test_attention_pieces_follow_the_key_count_alone():
    for n in list(range(1, 40)) + [511, 512, 513, 1024, 1025, 1660, 2047, 2048, 8192, 8193, 20000]:
        seen = set()
        for B, smax, rows in itertools.product((1, 2, 6, 7, 16, 48, 64), (max(n, 64), max(n, 2048), 24000), (1, 64)):
            p = _lib.batch_invariant_plan(D, D, rows, 0, False, B=B, heads=HEADS, smax=smax, n_keys=n)
            seen.add((p["attn_pieces"], p["attn_piece_keys"]))
            assert 1 <= p["attn_workgroups"] <= p["attn_pieces"]
        assert len(seen) == 1, f"{n} keys: pieces depend on B, the cache length or the row count: {sorted(seen)}"
        pieces, keys = seen.pop()
        assert pieces == min(16, -(-n // 512)) and pieces * keys >= n and (pieces - 1) * keys < n
        assert keys == n if pieces == 1 else keys % 16 == 0
    # configs[4] (1 row, ~1660 keys) keeps a split, every piece with a workgroup of its own; a 16..64-row step pays one workgroup
    # per (row, head) whatever the piece count
    one = _lib.batch_invariant_plan(D, D, 1, 2, False, B=1, heads=HEADS, smax=1700, n_keys=1660)
    assert one["attn_pieces"] == 4 and one["attn_workgroups"] == 4
    for B in (16, 48, 64):
        assert _lib.batch_invariant_plan(D, D, B, 1, False, B=B, heads=HEADS, smax=1700, n_keys=1660)["attn_workgroups"] == 1


def test_plan_query_refuses_bad_arguments():
    for kw in (dict(rows=0), dict(rows=65), dict(fmt=3), dict(B=0), dict(B=65), dict(n_keys=0), dict(n_keys=100, smax=99)):
        a = dict(N=D, K=D, rows=1, fmt=0, B=1, heads=HEADS, smax=2048, n_keys=1)
        a.update(kw)
        with pytest.raises(RuntimeError):
            _lib.batch_invariant_plan(a["N"], a["K"], a["rows"], a["fmt"], False, B=a["B"], heads=a["heads"], smax=a["smax"], n_keys=a["n_keys"])


def _pipeline(weight_format, batch_invariant):
    """What BatchPipeline._keeps_kernels reads of its pipeline: a stand-in with the model's configuration, weight format and mode."""
    gpt = types.SimpleNamespace(weight_format=weight_format, batch_invariant=batch_invariant)
    return types.SimpleNamespace(tts=types.SimpleNamespace(cfg=types.SimpleNamespace(gpt=GPTConfig()), gpt=gpt))


def _request(rows, width):
    import torch
    return types.SimpleNamespace(text=torch.zeros(rows, width, dtype=torch.long))


def test_merge_keeps_kernels_in_the_mode_and_without_it():
    from indextts_amd.serving import BatchPipeline, merge_keeps_kernels
    groupings = [[16, 16, 16], [4, 4, 4, 8], [2, 3, 4], [1, 63], [16, 1], [32, 32], [7]]
    today = {}
    for rows, prefix, split, compact, plane in itertools.product(groupings, (19, 165), (False, True), (False, True), (5, 17, 65)):
        off = merge_keeps_kernels(rows, prefix, split, compact, plane)
        today[(tuple(rows), prefix, split, compact, plane)] = off
        assert merge_keeps_kernels(rows, prefix, split, compact, plane, batch_invariant=False) == off
        assert merge_keeps_kernels(rows, prefix, split, compact, plane, batch_invariant=True) is True
    # today's answers, as tests/test_dist_cpu.py pins them: refusals exist with the mode off
    assert today[((16, 16, 16), 165, True, True, 17)] is False and today[((2, 3, 4), 19, True, False, 17)] is False
    assert today[((16, 16, 16), 165, True, True, 5)] is True
    # the pipeline's own guard, with a stand-in pipeline: compact weights, 16-utterance requests, default switches
    assert _lib.get_decode_plane_rows() == 17 and _lib.get_gemm_mode() == _lib.GEMM_BF16X3
    for rows in groupings:
        group = [_request(r, 12) for r in rows]      # 12 text tokens: 32 + 2 + 12 + 2 + 1 = 49 prompt rows per utterance
        for wf in ("f32", "bf16", "fp8"):
            assert BatchPipeline._keeps_kernels(_pipeline(wf, True), group) is True
            assert BatchPipeline._keeps_kernels(_pipeline(wf, False), group) == merge_keeps_kernels(rows, 49, True, wf != "f32", 17)
    assert BatchPipeline._keeps_kernels(_pipeline("bf16", False), [_request(16, 12)] * 3) is False
