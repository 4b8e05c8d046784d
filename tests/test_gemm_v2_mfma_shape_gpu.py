"""The LDS-DMA split-bf16 GEMM's main loop on v_mfma_f32_16x16x32_bf16: a step multiplies a PAIR of 16-k stages, an odd stage
count ends in a 16-k tail step, and the epilogue reads the 16 x 16 C/D layout.  Operator level (idxtts_linear_fwd, every case
M >= 256 and N >= 96 so that this kernel takes it) against the float64 product, bit-wise row invariance, and the tap / rotary /
plane hand-over forms through the CFM estimator against the CPU oracle."""
import ctypes
import dataclasses
import math
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

from indextts_amd import _lib, synth, weights
from indextts_amd.config import S2MelConfig

pytestmark = pytest.mark.gpu

MS = (256, 257, 383)                 # whole tiles, one row into the clamped last row tile, an odd remainder


class _Linear:
    def __init__(self, w, b):
        self.lib = _lib.load()
        self.N, self.K = w.shape
        self.h = c_void_p()
        _lib.check(self.lib.idxtts_linear_create(_lib.ptr(w.contiguous()), _lib.ptr(b), self.N, self.K, 0, ctypes.byref(self.h)))

    def __call__(self, xd, act=0, res=None, loop=1):      # loop: idxtts_linear_fwd's bf16x3, 1 = the 16x16x32 loop, 2 = the 32x32x16 loop
        M = xd.shape[0]
        No = self.N // 2 if act == 3 else self.N
        y = torch.full((M, No), float("nan"), device=xd.device)
        _lib.check(self.lib.idxtts_linear_fwd(self.h, _lib.ptr(xd), self.K, _lib.ptr(y), No, _lib.ptr(res), No, M, act, loop, _lib.current_stream()))
        return y.cpu()

    def close(self):
        self.lib.idxtts_linear_destroy(self.h)


def _check(y, ref, what):
    err = (y.double() - ref).abs()
    assert err.max().item() <= 1e-4 * max(1.0, ref.abs().max().item()), (what, err.max().item())
    assert err.mean().item() <= 1e-5, (what, err.mean().item())


@pytest.mark.parametrize("N", [96, 112, 129, 8194])
@pytest.mark.parametrize("K", [16, 32, 48, 80, 864])
def test_stage_pairs_tail_and_partial_tiles_vs_float64(device, K, N):
    """K = 16: the tail step alone; 32: one pair; 48, 80: pairs + tail; 864: 54 stages.  N: partial column tiles (N = 129, 8194: no
    16-byte rows, so the scalar store path).  Plain, residual, gelu and silu epilogues at each M, one float64 product for all."""
    Mx = max(MS)
    x = torch.from_numpy(synth.uniform(f"t/mf16/x/{K}", (Mx, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/b/{N}", (N,), 0.2))
    r = torch.from_numpy(synth.uniform(f"t/mf16/r/{N}", (Mx, N), 1.0))
    pre = x.double() @ w.double().t() + b.double()
    gelu = 0.5 * pre * (1 + torch.tanh(math.sqrt(2 / math.pi) * (pre + 0.044715 * pre ** 3)))
    refs = {"plain": (0, False, pre), "res": (0, True, pre + r.double()), "gelu": (1, False, gelu), "gelu+res": (1, True, gelu + r.double()),
            "silu": (2, False, F.silu(pre))}
    lin = _Linear(w, b)
    xd, rd = x.to(device), r.to(device)
    try:
        for M in MS:
            for what, (act, with_res, ref) in refs.items():
                y = lin(xd[:M].contiguous(), act, rd[:M].contiguous() if with_res else None)
                _check(y, ref[:M], (what, M))
    finally:
        lin.close()


@pytest.mark.parametrize("Hd", [96, 4128])          # packed N = 192 (a whole and a half column tile), 8256 (64.5 column tiles)
@pytest.mark.parametrize("K", [16, 32, 48, 80, 864])
def test_packed_swiglu_vs_float64(device, K, Hd):
    """act 3: columns packed as [32 gate | 32 linear] groups, so N is a multiple of 64 (the N of the other test cannot be packed)."""
    Mx = max(MS)
    x = torch.from_numpy(synth.uniform(f"t/mf16/x/{K}", (Mx, K), 1.0))
    w1 = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w1/{Hd}/{K}", (Hd, K), K, 2.0))
    w3 = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w3/{Hd}/{K}", (Hd, K), K, 2.0))
    r = torch.from_numpy(synth.uniform(f"t/mf16/rs/{Hd}", (Mx, Hd), 1.0))
    packed = torch.stack([w1.view(Hd // 32, 32, K), w3.view(Hd // 32, 32, K)], dim=1).reshape(2 * Hd, K)
    ref = F.silu(x.double() @ w1.double().t()) * (x.double() @ w3.double().t())
    lin = _Linear(packed, None)
    xd, rd = x.to(device), r.to(device)
    try:
        for M in MS:
            _check(lin(xd[:M].contiguous(), 3), ref[:M], ("swiglu", M))
            _check(lin(xd[:M].contiguous(), 3, rd[:M].contiguous()), ref[:M] + r[:M].double(), ("swiglu+res", M))
    finally:
        lin.close()


@pytest.mark.parametrize("N,K", [(512, 864), (256, 80)])        # 54 stages; two pairs and the tail
def test_rows_do_not_depend_on_row_count_or_tile_place(device, N, K):
    """The k order of a row's sum is fixed: rows of an M = 2000 call equal, bit for bit, the same rows inside an M = 256 call, where
    they sit among other rows at another place of the tile."""
    M = 2000
    x = torch.from_numpy(synth.uniform(f"t/mf16/inv/x/{N}/{K}", (M, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/inv/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/inv/b/{N}", (N,), 0.2))
    lin = _Linear(w, b)
    xd = x.to(device)
    try:
        big = lin(xd)
        for lo, hi in ((0, 77), (130, 258), (1990, 2000)):
            n, at = hi - lo, (256 - (hi - lo)) // 2 | 1        # odd offset: another register and lane of the accumulator tile
            small_x = xd[700:956].clone()
            small_x[at:at + n] = xd[lo:hi]
            small = lin(small_x)
            assert torch.equal(small[at:at + n], big[lo:hi]), (lo, hi)
    finally:
        lin.close()


@pytest.mark.parametrize("N,K", [(129, 48), (512, 864)])
def test_32x32x16_loop_vs_float64_and_row_invariance(device, N, K):
    """The loop that the GPT, conditioning and semantic weights keep (their results select discrete codes, so their sums stay what
    they were): same bounds against float64, rows independent of the row count, and really another loop than the 16x16x32 one."""
    M = 2000
    x = torch.from_numpy(synth.uniform(f"t/mf16/inv/x/{N}/{K}", (M, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/inv/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/inv/b/{N}", (N,), 0.2))
    r = torch.from_numpy(synth.uniform(f"t/mf16/inv/r/{N}", (M, N), 1.0))
    ref = x.double() @ w.double().t() + b.double() + r.double()
    lin = _Linear(w, b)
    xd, rd = x.to(device), r.to(device)
    try:
        big = lin(xd, 0, rd, loop=2)
        _check(big, ref, "32x32x16")
        for lo, hi in ((0, 77), (130, 258), (1990, 2000)):
            small_x, small_r = xd[700:956].clone(), rd[700:956].clone()
            small_x[3:3 + hi - lo], small_r[3:3 + hi - lo] = xd[lo:hi], rd[lo:hi]
            assert torch.equal(lin(small_x, 0, small_r, loop=2)[3:3 + hi - lo], big[lo:hi]), (lo, hi)
        if K > 48:      # 54 stages: the two k orders round differently somewhere
            assert not torch.equal(lin(xd, 0, rd, loop=1), big)
    finally:
        lin.close()


def test_tap_form_takes_whole_32k_pairs_per_tap_only(device):
    """A pair step never straddles a tap and the tap form never ends in a tail, because no caller can build that case: the s2mel model
    refuses channel counts that are no multiple of 32 when it loads (s2mel.hip), and gemm_prepare, which every GEMM kernel shares,
    refuses a convolution whose channels per tap are none (gemm.hip).  Here: the length regulator's 3-tap convolutions at 112."""
    from indextts_amd.s2mel import S2Mel
    cfg = dataclasses.replace(S2MelConfig.tiny(), lr_channels=112)
    S = torch.from_numpy(synth.uniform("t/s2mel/mf16/lr112/S", (2, 90, cfg.lr_in_channels), 1.0))
    with pytest.raises(RuntimeError, match="multiples? of 32"):
        sm = S2Mel(weights.synth_s2mel_weights(cfg, tag="t/s2mel/mf16/lr112"), cfg, device=device, max_frames=512)
        sm.length_regulator(S, torch.LongTensor([150, 131]))


def test_estimator_taps_rotary_and_plane_handover_vs_oracle(device):
    """Five-tap gate GEMMs (reflected edges, 12 chunks per tap: the convolution form takes only whole 32-k pairs per tap, see the
    test above), the rotary
    qkv epilogue, SwiGLU and plane outputs feeding the next GEMM's LDS-DMA, at hidden 192 (3 heads; K = 192 is 12 stages, the merge
    and skip GEMMs have other counts): ragged batch, 2B*T = 596 rows, against the fp32 CPU oracle.  (The oracle ties wn_hidden to
    hidden_dim through the final layer's modulation, and hidden_dim is 64 per head, so an odd chunk count per tap cannot be built.)"""
    from indextts_amd.s2mel import S2Mel
    from oracle import s2mel as osm
    cfg = dataclasses.replace(S2MelConfig.tiny(), hidden_dim=192, num_heads=3, depth=3, wn_hidden=192, wn_layers=2, block_size=512)
    w = weights.synth_s2mel_weights(cfg, tag="t/s2mel/mf16")
    sm = S2Mel(w, cfg, device=device, max_frames=512)
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    lens, plens = [149, 131], [40, 21]
    B, T, Tpm = 2, max(lens), max(plens)
    z = torch.from_numpy(synth.uniform("t/s2mel/mf16/z", (B, cfg.in_channels, T), 1.7))
    mu = torch.from_numpy(synth.uniform("t/s2mel/mf16/mu", (B, T, cfg.content_dim), 1.0))
    prompt = torch.from_numpy(synth.uniform("t/s2mel/mf16/prompt", (B, cfg.in_channels, Tpm), 1.0))
    st = torch.from_numpy(synth.uniform("t/s2mel/mf16/style", (B, cfg.style_dim), 1.0))
    for b in range(B):
        mu[b, lens[b]:] = 0
    out = sm.cfm_inference(mu, torch.LongTensor(lens), prompt, st, None, 2, inference_cfg_rate=0.7, z=z,
                           prompt_lens=torch.LongTensor(plens)).cpu()
    for b in range(B):
        Lb, Pb = lens[b], plens[b]
        ref = osm.cfm_inference(tw, cfg, mu[b:b + 1, :Lb], torch.LongTensor([Lb]), prompt[b:b + 1, :, :Pb], st[b:b + 1],
                                z[b:b + 1, :, :Lb], 2, 0.7)
        err = (out[b, :, :Lb] - ref[0]).abs()
        assert err.mean().item() <= 1e-4 and err.max().item() <= 3e-3, (b, err.mean().item(), err.max().item())
