"""CPU: the fp8 KV-cache format (include/idxtts.h, IDXTTS_KV_FP8) as tests/kv_fp8_cases.py restates it -- against torch's float8_e4m3fn
cast and the library's host codec -- and the noise floor of the reference the GPU tests use: the oracle with the quantiser patched in,
evaluated in fp32 and in float64."""
import numpy as np
import pytest
import torch

import kv_fp8_cases as kc


def _torch_codes(y):
    return torch.from_numpy(np.asarray(y, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_quantiser_restatement_vs_torch_and_host_codec():
    from indextts_amd import _lib
    lib = _lib.load()
    x = kc.case_vectors()
    assert x.shape[0] > 3000 and x.shape[1] == 64
    codes, scales, vals = kc.quantize(x)
    amax = np.abs(x).max(axis=1).astype(np.float64)
    # the scale: a power of two, the smallest with amax / s <= 448 (so nothing saturates), 1 for an all-zero vector
    m, _ = np.frexp(scales.astype(np.float64))
    assert (m == 0.5).all()
    assert (scales[amax == 0] == 1.0).all() and (amax == 0).sum() == 2
    nz = amax > 0
    assert (amax[nz] / scales[nz] <= 448.0).all() and (amax[nz] / scales[nz] > 224.0).all()
    y = (x.astype(np.float64) / scales[:, None].astype(np.float64)).astype(np.float32)      # exact (power of two; the cases stay normal)
    assert np.array_equal(y.astype(np.float64) * scales[:, None], x.astype(np.float64))
    # codes: torch's cast of x / s, and the library's host encoder, agree with the explicit grid
    assert np.array_equal(codes, _torch_codes(y))
    flat_y, flat_c = y.reshape(-1), codes.reshape(-1)
    pick = np.unique(np.concatenate([np.arange(0, flat_y.size, 37), np.nonzero(np.abs(flat_y) < 2.0 ** -5)[0][:4000]]))
    for i in pick:
        assert lib.idxtts_fp8_e4m3_encode(float(flat_y[i])) == flat_c[i], (flat_y[i], flat_c[i])
    for c in range(256):
        if c & 0x7F != 0x7F:
            assert lib.idxtts_fp8_e4m3_decode(c) == kc.decode_e4m3(np.uint8(c)), c
    # the cached value decode(code) * s is an exact fp32 product; -0.0 keeps its sign bit
    assert np.array_equal(vals.astype(np.float64), kc.decode_e4m3(codes) * scales[:, None].astype(np.float64))
    assert np.array_equal(np.signbit(vals), np.signbit(x))


def test_scale_steps_exactly_at_448_times_a_power_of_two():
    for e in range(-24, 12):
        at = np.float32(448.0 * 2.0 ** e)
        above, below = np.nextafter(at, np.float32(np.inf)), np.nextafter(at, np.float32(0))
        assert list(kc.scale_exponents([below, at, above])) == [e, e, e + 1]
    assert kc.scale_exponents([0.0])[0] == 0 and kc.scale_exponents([1e-38])[0] == -100 and kc.scale_exponents([3e38])[0] == 100


def test_midpoints_tie_to_the_even_code():
    mids = 0.5 * (kc.GRID[:-1] + kc.GRID[1:])
    got = kc.encode_e4m3(mids)
    want = np.array([c if c % 2 == 0 else c + 1 for c in range(126)], dtype=np.uint8)
    assert np.array_equal(got, want) and np.array_equal(kc.encode_e4m3(-mids), want | 0x80)
    assert np.array_equal(got, _torch_codes(mids))


@pytest.fixture
def fp8_oracle(monkeypatch):
    import oracle.gpt
    monkeypatch.setattr(oracle.gpt, "gpt2_stack", kc.fp8_stack)
    return oracle.gpt


@pytest.mark.parametrize("B,heads,NEW", kc.GREEDY_SHAPES)
def test_patched_oracle_fp32_and_float64_agree_on_every_code(fp8_oracle, B, heads, NEW):
    """The reference of tests/test_kv_fp8_gpu.py alone stays inside that file's "equal or near-tie" cap: on its inputs the patched fp32
    oracle and the patched float64 oracle decode the same codes.  Prints their max |dlogit|, the noise floor of that comparison."""
    og = fp8_oracle
    cfg, w, lat, emo, text = kc.greedy_case(B, heads)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    torch.set_num_threads(8)
    with torch.no_grad():
        conds = og.conds_latent(tw, cfg, lat, emo)
        c32, l32 = og.generate_greedy(tw, cfg, conds, text, NEW, 10.0, return_logits=True)
        c64, l64 = og.generate_greedy(tw, cfg, conds, text, NEW, 10.0, return_logits=True, dtype=torch.float64)
    live = l64.abs() < 1e3
    noise = ((l32.double() - l64.double()).abs() * live).max().item()
    print(f"[kv fp8 oracle noise B={B} heads={heads}] fp32 vs float64 patched oracle: max |dlogit| {noise:.3e} over {NEW} steps")
    assert c32.shape[1] == NEW and torch.equal(c32, c64)
