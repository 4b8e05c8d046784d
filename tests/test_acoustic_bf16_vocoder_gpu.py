"""The vocoder convolutions under idxtts_set_acoustic_bf16: conv1d_bf16x3.hip's single-product form (the hi plane of the x tile and
the hi halves of the weight images alone, one MFMA per product) at every case of tests/vocoder_dispatch_cases.py.

Every layer built through idxtts_conv1d_create or a BigVGAN context carries the bf16 pack, so every case is compared against
conv_reference on bf16-ROUNDED w and x with the bound of tests/test_acoustic_bf16_gemm_gpu.py, K read as products per output
(Cin x taps; a transposed convolution runs as 3 GEMM taps):
    |y - ref_r| <= Cin taps 2^-23 (|w^| * |x^|) + 2^-22 |ref_r|
What carries no pack in effect is the exact mode: there the output is bit-identical to switch off."""
import pytest
import torch

import vocoder_dispatch_cases as dc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _lib.set_acoustic_bf16(False)
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def _r(t):
    return t.bfloat16().float()


def _check_conv(device, case, transposed):
    from indextts_amd.vocoder import Conv1d
    w, b, x, res, out = dc.conv_inputs(case, transposed)
    _, Cin, _, K, _, _ = case
    ref = dc.conv_reference(case, w, b, x, transposed)
    ref_r = dc.conv_reference(case, _r(w), b, _r(x), transposed)
    absprod = dc.conv_reference(case, _r(w).abs(), torch.zeros_like(b), _r(x).abs(), transposed)
    bound = Cin * (3 if transposed else K) * 2.0 ** -23 * absprod + 2.0 ** -22 * ref_r.abs()
    conv = Conv1d(w, b, transposed_stride=case[4]) if transposed else Conv1d(w, b)
    kw = {} if transposed else {"dilation": case[4]}
    xd = x.to(device)
    off = conv(xd, **kw).cpu()
    _lib.set_acoustic_bf16(True)
    on = conv(xd, **kw).cpu()
    assert on.shape == ref_r.shape
    err = (on.double() - ref_r).abs()
    worst = (err / bound.clamp_min(1e-30)).max().item()
    gap_on, gap_off = (on.double() - ref).abs().max().item(), (off.double() - ref).abs().max().item()
    print(f"ERR bf16 conv {case} T={transposed}: max err/bound {worst:.3f}; from the unrounded reference: on {gap_on:.3e}, off {gap_off:.3e}")
    assert worst <= 1.0, worst
    assert gap_on > 4 * gap_off                               # the path ran: bf16-far from the product of the unrounded operands
    # fused epilogue: residual, scale, accumulate into a pre-filled out -- three more fp32 roundings of values <= |want| + |out|
    got = conv(xd, residual=res.to(device), scale=1.0 / 3, out=out.to(device).clone(), accumulate=True, **kw).cpu()
    want = out.double() + (ref_r + res.double()) / 3
    slack = 2.0 ** -22 * (want.abs() + out.double().abs() + (ref_r + res.double()).abs())
    assert ((got.double() - want).abs() <= bound / 3 + slack).all()
    # the exact mode never reads the switch
    _lib.set_gemm_mode(_lib.GEMM_F32)
    exact_on = conv(xd, **kw).cpu()
    _lib.set_acoustic_bf16(False)
    assert torch.equal(conv(xd, **kw).cpu(), exact_on)
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    assert torch.equal(conv(xd, **kw).cpu(), off)             # and switch off is what it was before the toggle


@pytest.mark.parametrize("case", [c for c, _ in dc.CONV_CASES], ids=["-".join(map(str, c)) for c, _ in dc.CONV_CASES])
def test_conv1d_bf16_vs_float64_of_rounded_operands(device, case):
    _check_conv(device, case, False)


@pytest.mark.parametrize("case", [c for c, _ in dc.CONVT_CASES], ids=["-".join(map(str, c)) for c, _ in dc.CONVT_CASES])
def test_conv_transpose1d_bf16_vs_float64_of_rounded_operands(device, case):
    _check_conv(device, case, True)


@pytest.mark.parametrize("case", dc.RAGGED_CASES + [dc.RAGGED_FULL], ids=lambda c: f"ragged{c[0]}")
def test_bigvgan_ragged_rows_equal_solo_calls_bitwise(device, case):
    """Switch on: row b of a ragged batch equals the vocoder on that row's own frames alone, bit for bit (an output's sum does not
    depend on the tile its column falls in, nor on what lies behind the row's end)."""
    from indextts_amd.vocoder import BigVGAN
    num, width, Tm, lens = case
    cfg, w = dc.ragged_weights(width)
    voc = BigVGAN(w, cfg)
    mel = dc.ragged_mel(num, cfg, len(lens), Tm)
    up = cfg.total_upsample
    off = voc(mel.to(device), clamp=False, lengths=lens).cpu()
    _lib.set_acoustic_bf16(True)
    voc(dc.ragged_mel(num, cfg, len(lens), Tm, "dirty").to(device), clamp=False)      # non-zero scratch beyond every short row's end
    got = voc(mel.to(device), clamp=False, lengths=lens).cpu()
    assert torch.isfinite(got).all() and not torch.equal(got, off)
    for b, n in enumerate(lens):
        if n == 0:
            assert (got[b] == 0).all()
            continue
        solo = voc(mel[b:b + 1, :, :n].contiguous().to(device), clamp=False).cpu()
        assert solo.shape[-1] == n * up
        diff = (got[b:b + 1, :, : n * up] - solo).abs().max().item()
        print(f"ragged{num} row {b} ({n} frames): max |ragged - solo| {diff:.3e}")
        assert torch.equal(got[b:b + 1, :, : n * up], solo), (b, diff)
