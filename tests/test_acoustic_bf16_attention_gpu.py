"""idxtts_attention_bf16_fwd (AttnArgs::split_bf16 = 2, what the DiT attention runs under idxtts_set_acoustic_bf16): q, k, v rounded
once to nearest-even bf16, one MFMA per product, P rounded once to bf16.

Reference: float64 attention on the ROUNDED q, k, v.  Rounding P costs at most 2^-9 sum(p |v|) in the numerator (and at most 2^-9
relative in a denominator summed from rounded P), the fp32 sums and exponentials ~1e-6:
    |o - ref_r| <= 2^-8 max|v^| + 1e-5
(CPU emulation, unit-variance inputs, S = 150: 1.7e-3 against the bound's 1.6e-2.)  That the kernel really rounds shows against
float64 attention on the UNROUNDED inputs: the output misses the split kernel's 1e-4 tolerance, which the split entry passes."""
from ctypes import c_void_p

import pytest
import torch

from indextts_amd import _lib, synth

pytestmark = pytest.mark.gpu

B, H = 2, 3


def _attention64(q, k, v, allowed):
    scores = (q @ k.transpose(-1, -2)) / 8.0
    att = torch.nan_to_num(torch.softmax(scores.masked_fill(~allowed, float("-inf")), -1), nan=0.0)
    return att @ v


@pytest.mark.parametrize("S,causal", [(37, False), (64, False), (150, False), (150, True)])
def test_bf16_attention_vs_float64_of_rounded_inputs(device, S, causal):
    """S = 37: one partial key tile; 64: two whole tiles, one row of which ends inside the second; 150: two query blocks, five key
    tiles, ragged ends (kend = S, S - 7: a masked last tile and a tile boundary that moves)."""
    d = H * 64
    qkv = torch.from_numpy(synth.uniform(f"t/abf16/attn/qkv/{S}", (B, S, 3 * d), 1.7))      # unit variance
    kend = torch.tensor([S - 7 * b for b in range(B)], dtype=torch.int32)
    pos = torch.arange(S)
    allowed = (pos[None, :] < kend[:, None])[:, None, None, :].expand(B, 1, S, S)
    if causal:
        allowed = allowed & (pos[None, :] <= pos[:, None])[None, None]
    q, k, v = (t.view(B, S, H, 64).transpose(1, 2) for t in qkv.split(d, dim=2))
    ref = _attention64(q.double(), k.double(), v.double(), allowed).transpose(1, 2).reshape(B, S, d)
    ref_r = _attention64(q.bfloat16().double(), k.bfloat16().double(), v.bfloat16().double(), allowed).transpose(1, 2).reshape(B, S, d)
    vmax = v.bfloat16().double().abs().max().item()
    lib = _lib.load()
    qd = qkv.to(device).contiguous()
    base = qd.data_ptr()
    ke = kend.to(device)
    out = {}
    for name, fn in (("bf16", lib.idxtts_attention_bf16_fwd), ("bf16x3", lib.idxtts_attention_bf16x3_fwd)):
        o = torch.full((B, S, d), float("nan"), device=device)
        _lib.check(fn(c_void_p(base), c_void_p(base + 4 * d), c_void_p(base + 8 * d), _lib.ptr(o), S * 3 * d, 3 * d, S * 3 * d, 3 * d,
                      S * d, d, B, H, S, S, int(causal), None, _lib.ptr(ke), 0.125, _lib.current_stream()))
        out[name] = o.cpu().double()
    err_r = (out["bf16"] - ref_r).abs().max().item()
    bound = 2.0 ** -8 * vmax + 1e-5
    gap = (out["bf16"] - ref).abs().max().item()
    tol = 1e-4 * max(1.0, ref.abs().max().item())
    print(f"ERR bf16 attention S {S} causal {causal}: {err_r:.3e} of {bound:.3e}; from the unrounded reference {gap:.3e} (split tolerance {tol:.1e})")
    assert err_r <= bound, err_r
    assert gap > tol, gap
    assert (out["bf16x3"] - ref).abs().max().item() <= tol
