"""GPU: idxtts_cfm_noise (csrc/cfm_noise.hip) -- the seeded CFM noise -- against a float64 numpy restatement of the draw in
include/idxtts.h: values, the zero tail, bit-for-bit invariance to batch / padding / row position / stream, the moments of the
stream, and the argument errors.

The 2e-5 bound on |device - restatement|: the integer part and the 23-bit uniforms are exact in fp32; what is left is fp32 log (3 ulp),
sqrt (3 ulp) and cos (4 ulp) by OpenCL's bounds plus a rounded 2*pi*u2 argument, at |n| <= 5.77: about 1.1e-5 in the worst case,
doubled."""
import ctypes

import numpy as np
import pytest
import torch

from indextts_amd import _lib

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1
SEEDS = (0, 2 ** 64 - 1, 2 ** 63 + 12345)


def restate(seed: int, C: int, T: int) -> np.ndarray:
    """[C, T] float64: the draw of include/idxtts.h, integer part in uint64 (numpy wraps mod 2^64)."""
    c = np.arange(C, dtype=np.uint64)[:, None]
    t = np.arange(T, dtype=np.uint64)[None, :]
    idx = (c << np.uint64(32)) | t
    with np.errstate(over="ignore"):
        z = np.uint64(seed ^ 0xD1B54A32D192ED03) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u1 = ((z >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (((z >> np.uint64(18)) & np.uint64(0x7FFFFF)).astype(np.float64) + 0.5) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def test_restatement_is_the_scalar_definition():
    """The vectorised restatement against the definition written out with Python ints for a few elements."""
    import math
    for seed, c, t in ((0, 0, 0), (2 ** 64 - 1, 79, 1028), (2 ** 63 + 12345, 3, 7)):
        z = ((seed ^ 0xD1B54A32D192ED03) + 0x9E3779B97F4A7C15 * (((c << 32) | t) + 1)) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        u1 = ((z >> 41) + 0.5) * 2.0 ** -23
        u2 = (((z >> 18) & 0x7FFFFF) + 0.5) * 2.0 ** -23
        n = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
        assert abs(restate(seed, c + 1, t + 1)[c, t] - n) < 1e-12


def call(seeds, x_lens, C, T, device, out=None):
    """idxtts_cfm_noise on the current stream -> (return code, z [B, C, T])."""
    B = len(seeds)
    sa = np.array([int(s) for s in seeds], dtype=np.uint64)
    xl = np.array(x_lens, dtype=np.int32)
    z = out if out is not None else torch.empty(max(B, 1), C, T, device=device)
    rc = _lib.load().idxtts_cfm_noise(sa.ctypes.data_as(ctypes.c_void_p), xl.ctypes.data_as(ctypes.c_void_p), B, C, T, _lib.ptr(z),
                                      _lib.current_stream())
    return rc, z


@pytest.mark.parametrize("C,x_lens,T", [(80, [1, 1023, 1029], 1029), (5, [0, 7, 260], 264)])
def test_values_and_zero_tail(device, C, x_lens, T):
    out = torch.full((3, C, T), float("nan"), device=device)
    rc, z = call(SEEDS, x_lens, C, T, device, out=out)
    assert rc == 0, _lib.load().idxtts_last_error()
    z = z.cpu().numpy()
    worst = 0.0
    for b, (seed, n) in enumerate(zip(SEEDS, x_lens)):
        assert not np.isnan(z[b, :, :n]).any(), b
        assert (z[b, :, n:] == 0.0).all() and not np.signbit(z[b, :, n:]).any(), b
        if n:
            worst = max(worst, np.abs(z[b, :, :n].astype(np.float64) - restate(seed, C, n)).max())
    print(f"max |device - restatement| = {worst:.3e}")
    assert worst <= 2e-5


def test_more_rows_than_one_launch_carries(device):
    """33 rows: the seeds and lengths of a launch travel by value, 32 rows at a time."""
    B, C, T = 33, 3, 9
    seeds = [1000 + 7 * b for b in range(B)]
    x_lens = [b % (T + 1) for b in range(B)]
    rc, z = call(seeds, x_lens, C, T, device, out=torch.full((B, C, T), float("nan"), device=device))
    assert rc == 0, _lib.load().idxtts_last_error()
    z = z.cpu().numpy()
    for b in range(B):
        want = np.zeros((C, T))
        want[:, :x_lens[b]] = restate(seeds[b], C, x_lens[b])
        assert np.abs(z[b] - want).max() <= 2e-5, b


def test_a_row_does_not_depend_on_batch_padding_position_or_stream(device):
    C, n = 80, 1023
    seed = SEEDS[2]
    rc, alone = call([seed], [n], C, n, device)
    assert rc == 0
    alone = alone[0].clone()
    others = [(11, 1200), (12, 5)]
    for pos in range(3):
        seeds = [s for s, _ in others]
        lens = [m for _, m in others]
        seeds.insert(pos, seed)
        lens.insert(pos, n)
        rc, z = call(seeds, lens, C, 1201, device)      # odd width: channels start at every offset from a 16-byte boundary
        assert rc == 0
        assert torch.equal(z[pos, :, :n], alone), pos
        assert not torch.equal(z[(pos + 1) % 3, :, :5], alone[:, :5])
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        rc, z = call([3, seed], [40, n], C, 1026, device)
        assert rc == 0
        side.synchronize()
    assert torch.equal(z[1, :, :n], alone)
    # rows of 3 x 11 floats: each starts at another offset from a 16-byte boundary, and 4-float groups run across channels
    rc, small = call([seed], [10], 3, 10, device)
    assert rc == 0
    rc, z = call([1, 2, seed, 4, seed], [11, 0, 10, 3, 10], 3, 11, device)
    assert rc == 0
    assert torch.equal(z[2, :, :10], small[0]) and torch.equal(z[4, :, :10], small[0]) and torch.equal(small[0], alone[:3, :10])
    rc, z = call([seed, 5, seed], [n, n, n], C, n, device)
    assert rc == 0
    assert torch.equal(z[0], z[2]) and torch.equal(z[0], alone)
    assert not torch.equal(z[0], z[1])


def test_moments(device):
    """4-sigma conditions on N = 80 x 4096 draws per seed; the restatement alone meets them for these seeds (worst variance
    deviation 0.0039, kurtosis 0.035, lag 0.0026)."""
    seeds = (0, 1, 77, 2 ** 63 + 12345, 2 ** 64 - 1)
    C, n = 80, 4096
    rc, z = call(seeds, [n] * len(seeds), C, n, device)
    assert rc == 0
    z = z.cpu().numpy().astype(np.float64)
    N = C * n
    for b, seed in enumerate(seeds):
        x = z[b]
        mean, var, m4 = x.mean(), x.var(), (x ** 4).mean()
        lag_t, lag_c = (x[:, 1:] * x[:, :-1]).mean(), (x[1:] * x[:-1]).mean()
        print(f"seed {seed}: mean {mean:+.4f} var {var:.4f} m4 {m4:.4f} lag_t {lag_t:+.4f} lag_c {lag_c:+.4f} max |n| {np.abs(x).max():.3f}")
        assert abs(mean) < 4 / np.sqrt(N)
        assert abs(var - 1) < 4 * np.sqrt(2 / N)
        assert abs(m4 - 3) < 4 * np.sqrt(96 / N)
        assert abs(lag_t) < 0.0070 and abs(lag_c) < 0.0070
        assert np.abs(x).max() <= 5.77


def test_errors_and_torch_generators_untouched(device):
    lib = _lib.load()
    rc, _ = call([1, 2], [4, 9], 3, 8, device)
    assert rc != 0 and b"x_lens[1]" in lib.idxtts_last_error()
    rc, _ = call([1], [-1], 3, 8, device)
    assert rc != 0 and lib.idxtts_last_error()
    rc, _ = call([], [], 3, 8, device)
    assert rc != 0 and lib.idxtts_last_error()
    for C, T in ((0, 8), (3, 0)):
        z = torch.empty(1, 4, 8, device=device)
        rc, _ = call([1], [0], C, T, device, out=z)
        assert rc != 0 and lib.idxtts_last_error()
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(device)
    rc, _ = call([1, 2], [4, 8], 3, 8, device)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(cpu, torch.get_rng_state()) and torch.equal(gpu, torch.cuda.get_rng_state(device))
