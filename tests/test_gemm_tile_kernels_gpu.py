"""The register-staged split-bf16 tile kernel (gemm_bf16x3.hip), the three instantiations the dispatch picks for shapes the LDS-DMA
kernel does not take (N < 96 or K % 16 != 0; any shape below 256 rows): 128 x 128 tiles, and from 4096 rows 256 x 128 and, for
N >= 256 without a paired activation, 256 x 256.  Operator level (idxtts_linear_fwd, bf16x3 = 1) against the float64 product with the
bounds of test_gemm_split_bf16_vs_torch, and bit-wise row invariance across the three."""
import ctypes
import math
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

from indextts_amd import _lib, synth

pytestmark = pytest.mark.gpu


class _Linear:
    def __init__(self, w, b):
        self.lib = _lib.load()
        self.N, self.K = w.shape
        self.h = c_void_p()
        _lib.check(self.lib.idxtts_linear_create(_lib.ptr(w.contiguous()), _lib.ptr(b), self.N, self.K, 0, ctypes.byref(self.h)))

    def __call__(self, xd, act=0, res=None):
        M = xd.shape[0]
        No = self.N // 2 if act == 3 else self.N
        y = torch.full((M, No), float("nan"), device=xd.device)
        _lib.check(self.lib.idxtts_linear_fwd(self.h, _lib.ptr(xd), self.K, _lib.ptr(y), No, _lib.ptr(res), No, M, act, 1, _lib.current_stream()))
        return y.cpu()

    def close(self):
        self.lib.idxtts_linear_destroy(self.h)


def _check(y, ref, what):
    err = (y.double() - ref).abs()
    print(what, "max", err.max().item(), "mean", err.mean().item(), "|ref|max", ref.abs().max().item())
    assert err.max().item() <= 1e-4 * max(1.0, ref.abs().max().item()), (what, err.max().item())
    assert err.mean().item() <= 1e-5, (what, err.mean().item())


def _gelu_new(v):
    return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))


@pytest.mark.parametrize("shape,forms", [
    ((300, 257, 40), ("plain", "res", "gelu+res")),      # 128-row tiles: last k-step 8 of 32 columns, last column block one column, last row tile 44 rows
    ((4097, 257, 40), ("plain", "gelu+res")),            # 256 x 256: one row in the last row tile; the second column block holds one column and no second weight tile
    ((4352, 512, 184), ("plain",)),                      # 256 x 256, whole tiles, the production merge K (5 k-steps and 24 columns)
])
def test_tile_kernels_vs_float64(device, shape, forms):
    M, N, K = shape
    x = torch.from_numpy(synth.uniform(f"t/tile16/x/{shape}", (M, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/tile16/w/{shape}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/tile16/b/{shape}", (N,), 0.2))
    r = torch.from_numpy(synth.uniform(f"t/tile16/r/{shape}", (M, N), 1.0))
    pre = x.double() @ w.double().t() + b.double()
    refs = {"plain": (0, False, pre), "res": (0, True, pre + r.double()), "gelu+res": (1, True, _gelu_new(pre) + r.double())}
    lin = _Linear(w, b)
    xd, rd = x.to(device), r.to(device)
    try:
        for what in forms:
            act, with_res, ref = refs[what]
            _check(lin(xd, act, rd if with_res else None), ref, (shape, what))
    finally:
        lin.close()


@pytest.mark.parametrize("M,Hd", [(300, 64), (4097, 160)])      # packed N = 128 on 128 x 128 tiles; N = 320, two and a half 128-column blocks, on 256 x 128
def test_paired_epilogue_on_tile_kernels_vs_float64(device, M, Hd):
    K = 40
    x = torch.from_numpy(synth.uniform(f"t/tile16/sw/x/{M}", (M, K), 1.0))
    w1 = torch.from_numpy(synth.fan_in_uniform(f"t/tile16/sw/w1/{Hd}", (Hd, K), K, 2.0))
    w3 = torch.from_numpy(synth.fan_in_uniform(f"t/tile16/sw/w3/{Hd}", (Hd, K), K, 2.0))
    r = torch.from_numpy(synth.uniform(f"t/tile16/sw/r/{M}/{Hd}", (M, Hd), 1.0))
    packed = torch.stack([w1.view(Hd // 32, 32, K), w3.view(Hd // 32, 32, K)], dim=1).reshape(2 * Hd, K)
    ref = F.silu(x.double() @ w1.double().t()) * (x.double() @ w3.double().t())
    lin = _Linear(packed, None)
    xd, rd = x.to(device), r.to(device)
    try:
        _check(lin(xd, 3), ref, ("swiglu", M, Hd))
        _check(lin(xd, 3, rd), ref + r.double(), ("swiglu+res", M, Hd))
    finally:
        lin.close()


@pytest.mark.parametrize("N,K", [(257, 40), (80, 512)])      # M = 4097 runs on 256 x 256 tiles / on 256 x 128 tiles; M = 300 on 128 x 128
def test_rows_equal_across_the_three_tile_shapes(device, N, K):
    """All three add the same 32-k steps in the same MFMA order: rows of an M = 4097 call equal, bit for bit, the same rows inside an
    M = 300 call, where they sit among other rows at another place of another tile."""
    M = 4097
    x = torch.from_numpy(synth.uniform(f"t/tile16/inv/x/{N}/{K}", (M, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/tile16/inv/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/tile16/inv/b/{N}", (N,), 0.2))
    lin = _Linear(w, b)
    xd = x.to(device)
    try:
        big = lin(xd)
        _check(big, x.double() @ w.double().t() + b.double(), (N, K))
        for lo, hi in ((0, 77), (130, 258), (4090, 4097)):
            n, at = hi - lo, (300 - (hi - lo)) // 2 | 1        # odd offset: another register and lane of the accumulator tile
            small_x = xd[700:1000].clone()
            small_x[at:at + n] = xd[lo:hi]
            small = lin(small_x)
            assert torch.equal(small[at:at + n], big[lo:hi]), (lo, hi)
    finally:
        lin.close()
