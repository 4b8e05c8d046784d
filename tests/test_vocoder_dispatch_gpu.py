"""GPU: the vocoder's kernels at every point where their host code switches tiles, store forms or kernel instances, against
float64 references, in both arithmetic modes (cases and the restated dispatch: tests/vocoder_dispatch_cases.py; what the case
tables cover, and that the constants they were derived from still hold: tests/test_vocoder_dispatch_cpu.py).

  * aa_act at the real tile (1016) and workgroup (4064) edges and within the +-4 / +-8 halos of them, fp32 and 16-bit IO;
  * conv1d / conv_transpose1d at both sides of every M threshold, in both epilogue forms, with 1 tap and several, at the halo
    limit, under the walk = 0 tile order with a plain conv, on unaligned views, at T = 1;
  * BigVGAN(..., lengths=) row by row against the oracle run on each row alone, with dirty scratch buffers, twice.
Bounds are those of tests/test_vocoder_gpu.py (ACT_ATOL, CONV_RTOL, TOL, the mid-width vocoder bound); none is wider here.
Every test prints its largest error beside its bound (pytest -s).  Measured on an MI355X, largest error / its bound:
  aa_act                 1.6e-6 / 1e-5      (T = 1015)
  conv, GEMM_F32         9.0e-6 / 5.2e-5    (768 x 768, k 11: 8448 products per output)      transposed 1.3e-6 / 5.1e-5
  conv, GEMM_BF16X3      1.6e-5 / 4.1e-4    (K1, Cin 5)                                      transposed 1.3e-5 / 3.6e-4
  ragged, GEMM_F32       1.1e-6 / 2e-5      ragged, GEMM_BF16X3   1.6e-5 / 1.6e-4      full width against the solo call: 0
Forcing either tile walk (IDXTTS_CONV_WALK = 0 / 1) changes no result: a walk only orders the tiles."""
import pytest
import torch

import vocoder_dispatch_cases as dc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu

ACT_ATOL = 1e-5       # tests/test_vocoder_gpu.py
CONV_RTOL = 2e-5
TOL = {"m": 1.0}
_ORACLE = {}          # ragged case number -> float64 oracle rows (computed once, shared by both modes, never modified)


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def arith(request):
    _lib.set_gemm_mode(_lib.GEMM_F32 if request.param == "f32" else _lib.GEMM_BF16X3)
    TOL["m"] = 1.0 if request.param == "f32" else 8.0
    yield request.param
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    TOL["m"] = 1.0


def _filt(device):
    from indextts_amd.vocoder import kaiser_sinc_filter12
    return kaiser_sinc_filter12().to(device)


def _report(group, arith, what, err, bound):
    print(f"ERR {group} {arith} {what}: {err:.3e} of {bound:.3e} = {err / bound:.3f}")


# ------------------------------------------------------------------------------------------
# fused anti-aliased activation
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.AA_CASES, ids=[f"{b}x{c}x{t}" for b, c, t in dc.AA_CASES])
def test_aa_act_vs_float64_oracle(device, arith, shape):
    from indextts_amd.vocoder import anti_alias_activation_forward
    from oracle import vocoder as ov
    x, la, lb = dc.aa_inputs(shape)
    f = _filt(device)
    y = anti_alias_activation_forward(x.to(device), f, f, la.to(device), lb.to(device)).cpu()
    ref = ov.activation1d(x.double(), la.double(), lb.double())
    assert y.shape == ref.shape and ref.dtype == torch.float64
    err = (y.double() - ref).abs().max().item()
    _report("aa_act", arith, shape, err, ACT_ATOL)
    assert err <= ACT_ATOL


@pytest.mark.parametrize("T", dc.AA16_T)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_aa_act_16bit_io_across_tile_seams(device, dtype, T):
    """The two assertions of test_vocoder_gpu.py::test_aa_act_half_precision_io where the 4-wide 16-bit store crosses a tile or
    workgroup seam (T % 4 == 0), and where it falls back to scalar stores (T = 1017)."""
    from indextts_amd.vocoder import anti_alias_activation_forward
    from oracle import vocoder as ov
    shape = (dc.AA16_B, dc.AA16_C, T)
    x, la, lb = dc.aa_inputs(shape, 3.0)
    x = x.to(dtype)
    f = _filt(device)
    y = anti_alias_activation_forward(x.to(device), f, f, la.to(device), lb.to(device))
    assert y.dtype == dtype and y.shape == x.shape
    y32 = anti_alias_activation_forward(x.float().to(device), f, f, la.to(device), lb.to(device))
    assert torch.equal(y.cpu(), y32.cpu().to(dtype))                              # one rounding, at the store
    ref = ov.activation1d(x.float(), la, lb)                                       # CPU oracle on the rounded input
    ulp = 2.0 ** (-10 if dtype == torch.float16 else -7)
    assert ((y.cpu().float() - ref).abs() <= ulp * ref.abs().clamp_min(1.0)).all()


# ------------------------------------------------------------------------------------------
# implicit-GEMM conv1d
# ------------------------------------------------------------------------------------------
def _check_conv(device, arith, case, transposed):
    from indextts_amd.vocoder import Conv1d
    w, b, x, res, out = dc.conv_inputs(case, transposed)
    ref = dc.conv_reference(case, w, b, x, transposed)
    conv = Conv1d(w, b, transposed_stride=case[4]) if transposed else Conv1d(w, b)
    kw = {} if transposed else {"dilation": case[4]}
    group = "convT" if transposed else "conv"
    y = conv(x.to(device), **kw).cpu()
    assert y.shape == ref.shape
    scale = ref.abs().max().item()
    err, bound = (y.double() - ref).abs().max().item(), TOL["m"] * CONV_RTOL * scale + 1e-6
    _report(group, arith, f"{case} plain", err, bound)
    assert err <= bound
    # fused epilogue: residual, scale, accumulate into a pre-filled out
    got = conv(x.to(device), residual=res.to(device), scale=1.0 / 3, out=out.to(device).clone(), accumulate=True, **kw).cpu()
    want = out.double() + (ref + res.double()) / 3
    err, bound = (got.double() - want).abs().max().item(), TOL["m"] * CONV_RTOL * max(scale, 1.0) + 1e-6
    _report(group, arith, f"{case} fused", err, bound)
    assert err <= bound


@pytest.mark.parametrize("case", [c for c, _ in dc.CONV_CASES], ids=["-".join(map(str, c)) for c, _ in dc.CONV_CASES])
def test_conv1d_vs_float64(device, arith, case):
    _check_conv(device, arith, case, False)


@pytest.mark.parametrize("case", [c for c, _ in dc.CONVT_CASES], ids=["-".join(map(str, c)) for c, _ in dc.CONVT_CASES])
def test_conv_transpose1d_vs_float64(device, arith, case):
    _check_conv(device, arith, case, True)


def test_conv1d_halo_over_the_limit_raises(device):
    from indextts_amd.vocoder import Conv1d
    B, Cin, Cout, K, dil, T = dc.CONV_HALO_OVER
    w, b, x, _, _ = dc.conv_inputs(dc.CONV_HALO_OVER)
    with pytest.raises(RuntimeError, match="CONV_MAX_HALO"):
        Conv1d(w, b)(x.to(device), dilation=dil)


@pytest.mark.parametrize("case,out_unaligned,res_unaligned", dc.CONV_UNALIGNED, ids=["out+res", "out", "res"])
def test_conv1d_unaligned_views(device, arith, case, out_unaligned, res_unaligned):
    """`out` / `residual` one float into a larger buffer: not 16-byte aligned, so a shape the wide epilogue would take runs the
    narrow one.  The result is right and the floats around the views keep their sentinel."""
    from indextts_amd.vocoder import Conv1d
    w, b, x, res, out = dc.conv_inputs(case)
    ref = dc.conv_reference(case, w, b, x)
    n = ref.numel()

    def view(t, unaligned):
        buf = torch.full((n + 8,), dc.SENTINEL, device=device)
        off = 1 if unaligned else 4
        v = buf[off:off + n].view(ref.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == unaligned
        return buf, off, v

    conv = Conv1d(w, b)
    scale = ref.abs().max().item()
    for fused in (False, True):
        obuf, ooff, o = view(out, out_unaligned)
        rbuf, roff, r = view(res, res_unaligned)
        if fused:
            got = conv(x.to(device), dilation=case[4], residual=r, scale=1.0 / 3, out=o, accumulate=True)
            want = out.double() + (ref + res.double()) / 3
        else:
            got = conv(x.to(device), dilation=case[4], residual=r, out=o)
            want = ref + res.double()
        assert got.data_ptr() == o.data_ptr()
        err, bound = (got.cpu().double() - want).abs().max().item(), TOL["m"] * CONV_RTOL * max(scale, 1.0) + 1e-6
        _report("conv", arith, f"{case} unaligned fused={fused}", err, bound)
        assert err <= bound
        for buf, off in ((obuf, ooff), (rbuf, roff)):
            assert (buf[:off] == dc.SENTINEL).all() and (buf[off + n:] == dc.SENTINEL).all()
        assert torch.equal(r.cpu(), res)


# ------------------------------------------------------------------------------------------
# whole vocoder, ragged batches
# ------------------------------------------------------------------------------------------
def _ragged_twice_on_dirty_scratch(voc, cfg, num, mel, lens, device, clamp=False):
    """One full-length random batch first, so the scratch buffers hold non-zero data beyond every short row's end; then the
    ragged call, twice, bit-equal."""
    B, _, Tm = mel.shape
    voc(dc.ragged_mel(num, cfg, B, Tm, "dirty").to(device), clamp=False)
    got = voc(mel.to(device), clamp=clamp, lengths=lens)
    again = voc(mel.to(device), clamp=clamp, lengths=lens)
    assert torch.equal(got, again)
    return got.cpu()


@pytest.mark.parametrize("case", dc.RAGGED_CASES, ids=[f"ragged{c[0]}" for c in dc.RAGGED_CASES])
def test_bigvgan_ragged_vs_oracle_rows(device, arith, case):
    """Row b of the ragged call against the float64 oracle on that row's own frames alone."""
    from indextts_amd.vocoder import BigVGAN
    num, width, Tm, lens = case
    cfg, w = dc.ragged_weights(width)
    mel = dc.ragged_mel(num, cfg, len(lens), Tm)
    if num not in _ORACLE:
        _ORACLE[num] = dc.ragged_oracle_rows(w, cfg, mel, lens)
    got = _ragged_twice_on_dirty_scratch(BigVGAN(w, cfg), cfg, num, mel, lens, device)
    up = cfg.total_upsample
    assert got.shape == (len(lens), 1, Tm * up)
    for b, n in enumerate(lens):
        ref = _ORACLE[num][b]
        if n == 0:
            assert (got[b] == 0).all()
            continue
        amax = ref.abs().max().item()
        err, bound = (got[b, :, : n * up].double() - ref).abs().max().item(), TOL["m"] * dc.RAGGED_ORACLE_ATOL * max(1.0, amax)
        _report("ragged", arith, f"case {num} row {b} ({n} frames, max|ref| {amax:.3f})", err, bound)
        assert err <= bound, (b, err)


def test_bigvgan_ragged_full_width_vs_solo_rows(device, arith):
    """The full 1536-channel configuration (the walk = 0 layers, the widest tiles) under lengths.  The CPU oracle takes minutes at
    this width, so the reference is the same library's solo call on each row's own frames, at the bound of
    test_vocoder_gpu.py::test_bigvgan_ragged_batch_equals_per_row_calls; the oracle comparisons are the narrower cases above."""
    from indextts_amd.vocoder import BigVGAN
    num, width, Tm, lens = dc.RAGGED_FULL
    cfg, w = dc.ragged_weights(width)
    voc = BigVGAN(w, cfg)
    mel = dc.ragged_mel(num, cfg, len(lens), Tm)
    got = _ragged_twice_on_dirty_scratch(voc, cfg, num, mel, lens, device)
    up = cfg.total_upsample
    for b, n in enumerate(lens):
        solo = voc(mel[b:b + 1, :, :n].contiguous().to(device), clamp=False).cpu()
        assert solo.shape[-1] == n * up and solo.abs().max().item() > 0.05
        err, bound = (got[b:b + 1, :, : n * up] - solo).abs().max().item(), 1e-6 * TOL["m"]
        _report("ragged_solo", arith, f"case {num} row {b}", err, bound)
        assert err <= bound, (b, err)


def test_bigvgan_ragged_clamped(device, arith):
    from indextts_amd.vocoder import BigVGAN
    num, width, Tm, lens = dc.RAGGED_CASES[0]
    cfg, w = dc.ragged_weights(width)
    w = dict(w)
    w["conv_post.weight"] = w["conv_post.weight"] * 4      # (conv_post is linear and has no bias: the waveform leaves [-1, 1])
    voc = BigVGAN(w, cfg)
    mel = dc.ragged_mel(num, cfg, len(lens), Tm)
    raw = voc(mel.to(device), clamp=False, lengths=lens).cpu()
    wav = voc(mel.to(device), clamp=True, lengths=lens).cpu()
    assert raw.abs().max().item() > 1.5 and (raw[-1] == 0).all()
    assert torch.isfinite(wav).all() and wav.abs().max().item() <= 1.0
    assert torch.equal(wav, raw.clamp(-1.0, 1.0))
