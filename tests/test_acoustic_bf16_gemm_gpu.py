"""The LDS-DMA GEMM's single-product form (idxtts_linear_fwd(bf16x3 = 3), what idxtts_set_acoustic_bf16 selects for s2mel): x and w
rounded to nearest-even bf16, ONE bf16 MFMA per product on the 16x16x32 loop, fp32 accumulation in the split loop's k order.

Reference: ref_r = float64 product of the ROUNDED operands + bias.  Products of two bf16 values are exact in fp32; K fp32 additions
in any order, truncation allowed, lose at most K * 2^-23 of the absolute sum; one more unit covers the bias add and the store:
    |y - ref_r| <= K * 2^-23 * (|x^| |w^|^T) + 2^-22 * |ref_r|          (activated epilogues: x 1.2 + 1e-6 for the gate's slope and the
                                                                         fast exp / rcp)
An fp32 emulation on the CPU stays below 0.06 of this bound on these inputs.  That the kernel really multiplies once shows against
ref = the float64 product of the UNROUNDED operands: on these inputs the two references are 9.4e-4 .. 1.0e-3 apart in the mean (max
about 5e-3), so the output must be >= 3e-4 from ref in the mean and must fail the split kernel's own check, which the bf16x3 = 1
output of the same call passes."""
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
KS = (16, 32, 48, 80, 864)           # the tail step alone; one pair; pairs + tail (twice); 54 stages


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _lib.set_acoustic_bf16(False)
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)


class _Linear:
    def __init__(self, w, b):
        self.lib = _lib.load()
        self.N, self.K = w.shape
        self.h = c_void_p()
        _lib.check(self.lib.idxtts_linear_create(_lib.ptr(w.contiguous()), _lib.ptr(b), self.N, self.K, 0, ctypes.byref(self.h)))

    def __call__(self, xd, act=0, res=None, form=3):      # form: idxtts_linear_fwd's bf16x3 (3 = one MFMA per product)
        M = xd.shape[0]
        No = self.N // 2 if act == 3 else self.N
        y = torch.full((M, No), float("nan"), device=xd.device)
        _lib.check(self.lib.idxtts_linear_fwd(self.h, _lib.ptr(xd), self.K, _lib.ptr(y), No, _lib.ptr(res), No, M, act, form, _lib.current_stream()))
        return y.cpu()

    def close(self):
        self.lib.idxtts_linear_destroy(self.h)


def _r(t):
    return t.bfloat16().double()


def _check_rounded(y, ref_r, absprod, K, what, activated=False, res=None):
    """ref_r: the reference without the residual.  A residual is added last, in fp32: one more rounding of the sum, 2^-23 |sum|."""
    bound = K * 2.0 ** -23 * absprod + 2.0 ** -22 * ref_r.abs()
    if activated:
        bound = 1.2 * bound + 1e-6
    if res is not None:
        ref_r = ref_r + res.double()
        bound = bound + 2.0 ** -23 * ref_r.abs()
    err = (y.double() - ref_r).abs()
    worst = (err / bound).max().item()
    print(f"ERR bf16 gemm {what}: max err/bound {worst:.3f}, mean err {err.mean().item():.3e}")
    assert worst <= 1.0, (what, worst)
    assert err.mean().item() <= 1e-5, (what, err.mean().item())


def _passes_split_check(y, ref):
    err = (y.double() - ref).abs()
    return err.max().item() <= 1e-4 * max(1.0, ref.abs().max().item()) and err.mean().item() <= 1e-5


@pytest.mark.parametrize("N", [96, 129, 512])
@pytest.mark.parametrize("K", KS)
def test_single_product_vs_float64_of_rounded_operands(device, K, N):
    """Plain, residual, gelu and silu epilogues at each M against ref_r; on the plain epilogue the output is bf16-far from the
    product of the unrounded operands while the split form of the same call is not."""
    Mx = max(MS)
    x = torch.from_numpy(synth.uniform(f"t/mf16/x/{K}", (Mx, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/b/{N}", (N,), 0.2))
    r = torch.from_numpy(synth.uniform(f"t/mf16/r/{N}", (Mx, N), 1.0))
    pre = _r(x) @ _r(w).t() + b.double()
    absprod = _r(x).abs() @ _r(w).abs().t()
    ref = x.double() @ w.double().t() + b.double()
    gelu = 0.5 * pre * (1 + torch.tanh(math.sqrt(2 / math.pi) * (pre + 0.044715 * pre ** 3)))
    refs = {"plain": (0, False, pre), "res": (0, True, pre), "gelu": (1, False, gelu), "gelu+res": (1, True, gelu), "silu": (2, False, F.silu(pre))}
    lin = _Linear(w, b)
    xd, rd = x.to(device), r.to(device)
    try:
        for M in MS:
            for what, (act, with_res, ref_r) in refs.items():
                y = lin(xd[:M].contiguous(), act, rd[:M].contiguous() if with_res else None)
                _check_rounded(y, ref_r[:M], absprod[:M], K, (what, M, N, K), activated=act != 0, res=r[:M] if with_res else None)
            y3 = lin(xd[:M].contiguous())
            gap = (y3.double() - ref[:M]).abs()
            print(f"GAP bf16 gemm {(M, N, K)}: mean {gap.mean().item():.3e} max {gap.max().item():.3e}")
            assert gap.mean().item() >= 3e-4, (M, gap.mean().item())
            assert gap.max().item() > 1e-4 * max(1.0, ref[:M].abs().max().item()), (M, gap.max().item())
            assert not _passes_split_check(y3, ref[:M])
            assert _passes_split_check(lin(xd[:M].contiguous(), form=1), ref[:M])
    finally:
        lin.close()


@pytest.mark.parametrize("K", KS)
def test_packed_swiglu_vs_float64_of_rounded_operands(device, K):
    """act 3 (Hd 96: packed N = 192, a whole and a half column tile): columns packed as [32 gate | 32 linear] groups."""
    Hd, Mx = 96, max(MS)
    x = torch.from_numpy(synth.uniform(f"t/mf16/x/{K}", (Mx, K), 1.0))
    w1 = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w1/{Hd}/{K}", (Hd, K), K, 2.0))
    w3 = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w3/{Hd}/{K}", (Hd, K), K, 2.0))
    r = torch.from_numpy(synth.uniform(f"t/mf16/rs/{Hd}", (Mx, Hd), 1.0))
    packed = torch.stack([w1.view(Hd // 32, 32, K), w3.view(Hd // 32, 32, K)], dim=1).reshape(2 * Hd, K)
    g, l = _r(x) @ _r(w1).t(), _r(x) @ _r(w3).t()
    ag, al = _r(x).abs() @ _r(w1).abs().t(), _r(x).abs() @ _r(w3).abs().t()
    ref_r = F.silu(g) * l
    # silu(g) l: first-order propagation of the two sums' bounds, |d silu| <= 1.1 |dg|, |silu(g)| <= |g|
    eg, el = K * 2.0 ** -23 * ag + 2.0 ** -22 * g.abs(), K * 2.0 ** -23 * al + 2.0 ** -22 * l.abs()
    bound = 1.2 * (1.1 * eg * l.abs() + g.abs() * el + 2.0 ** -22 * ref_r.abs()) + 1e-6
    lin = _Linear(packed, None)
    xd, rd = x.to(device), r.to(device)
    try:
        for M in MS:
            for res in (None, rd[:M].contiguous()):
                y = lin(xd[:M].contiguous(), 3, res)
                want = ref_r[:M] + (r[:M].double() if res is not None else 0.0)
                err = (y.double() - want).abs()
                worst = (err / (bound[:M] + 2.0 ** -23 * want.abs())).max().item()
                print(f"ERR bf16 gemm swiglu {(M, K, res is not None)}: max err/bound {worst:.3f}, mean err {err.mean().item():.3e}")
                assert worst <= 1.0 and err.mean().item() <= 1e-5, (M, worst, err.mean().item())
    finally:
        lin.close()


@pytest.mark.parametrize("N,K", [(512, 864), (256, 80)])        # 54 stages; two pairs and the tail
def test_rows_do_not_depend_on_row_count_or_tile_place(device, N, K):
    """Rows of an M = 2000 call equal, bit for bit, the same rows placed at an odd offset inside an M = 256 call."""
    M = 2000
    x = torch.from_numpy(synth.uniform(f"t/mf16/inv/x/{N}/{K}", (M, K), 1.0))
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/inv/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/inv/b/{N}", (N,), 0.2))
    lin = _Linear(w, b)
    xd = x.to(device)
    try:
        big = lin(xd)
        assert not torch.equal(big, lin(xd, form=1))
        for lo, hi in ((0, 77), (130, 258), (1990, 2000)):
            n, at = hi - lo, (256 - (hi - lo)) // 2 | 1        # odd offset: another register and lane of the accumulator tile
            small_x = xd[700:956].clone()
            small_x[at:at + n] = xd[lo:hi]
            small = lin(small_x)
            assert torch.equal(small[at:at + n], big[lo:hi]), (lo, hi)
    finally:
        lin.close()


def test_switch_round_trips_and_leaves_the_other_forms_alone(device):
    """idxtts_linear_fwd's forms 0, 1 and 2 never read the switch; form 3 does not need it."""
    N, K, M = 129, 80, 383
    x = torch.from_numpy(synth.uniform(f"t/mf16/x/{K}", (M, K), 1.0)).to(device)
    w = torch.from_numpy(synth.fan_in_uniform(f"t/mf16/w/{N}/{K}", (N, K), K))
    b = torch.from_numpy(synth.uniform(f"t/mf16/b/{N}", (N,), 0.2))
    lin = _Linear(w, b)
    try:
        assert _lib.get_acoustic_bf16() is False              # the default
        off = {f: lin(x, form=f) for f in (0, 1, 2, 3)}
        _lib.set_acoustic_bf16(True)
        assert _lib.get_acoustic_bf16() is True
        for f in (0, 1, 2, 3):
            assert torch.equal(lin(x, form=f), off[f]), f
        _lib.set_acoustic_bf16(False)
        assert _lib.get_acoustic_bf16() is False
        with pytest.raises(RuntimeError):                      # below 256 rows there is no single-product kernel
            lin(x[:255].contiguous(), form=3)
    finally:
        lin.close()


def test_exact_mode_ignores_the_switch(device):
    """GEMM_F32 and the switch on: an s2mel estimator call is bit-identical to switch off (596 rows: every GEMM and the attention
    would take the single-product kernels in the split mode)."""
    from indextts_amd.s2mel import S2Mel
    cfg = dataclasses.replace(S2MelConfig.tiny(), hidden_dim=192, num_heads=3, depth=3, wn_hidden=192, wn_layers=2, block_size=512)
    sm = S2Mel(weights.synth_s2mel_weights(cfg, tag="t/s2mel/mf16"), cfg, device=device, max_frames=512)
    lens, plens = [149, 131], [40, 21]
    B, T, Tpm = 2, max(lens), max(plens)
    z = torch.from_numpy(synth.uniform("t/s2mel/mf16/z", (B, cfg.in_channels, T), 1.7))
    mu = torch.from_numpy(synth.uniform("t/s2mel/mf16/mu", (B, T, cfg.content_dim), 1.0))
    prompt = torch.from_numpy(synth.uniform("t/s2mel/mf16/prompt", (B, cfg.in_channels, Tpm), 1.0))
    st = torch.from_numpy(synth.uniform("t/s2mel/mf16/style", (B, cfg.style_dim), 1.0))
    for b in range(B):
        mu[b, lens[b]:] = 0

    def run():
        return sm.cfm_inference(mu, torch.LongTensor(lens), prompt, st, None, 2, inference_cfg_rate=0.7, z=z,
                                prompt_lens=torch.LongTensor(plens)).cpu()
    _lib.set_gemm_mode(_lib.GEMM_F32)
    off = run()
    _lib.set_acoustic_bf16(True)
    on = run()
    assert torch.equal(on, off)
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert not torch.equal(run(), off)
