"""GPU: the device Kaldi filter bank (indextts_amd/frontend.py::KaldiFbank, csrc/fbank.hip) against the host front-end it restates
(`features.kaldi_fbank`, `features.seamless_m4t_features`: tests/test_features_cpu.py pins those to transformers' extractor).

Tolerance.  The host computes in float64 up to the log, the device in float32, so the bound is not invented: frontend_cases.py restates
the algorithm in float32 numpy, and its deviation from the host ON THE SAME INPUT is that input's floor -- what float32 alone costs there.
The device gets 4 x that floor (the MFMA's k order and the device logf differ from numpy's).  Measured, max |delta| against the host
(floor: the restatement on the host; device: MI355X):

    samples (frames)     log-mel, both scales      minus mean (CAMPPlus)     normalised (w2v-BERT)
                         floor      device         floor      device         floor      device
    400 (1)              1.10e-05   1.24e-05       0          0              -- raises --
    560 (2)              8.58e-06   5.72e-06       5.72e-06   3.82e-06       5.51e-05   9.66e-05
    720 (3)              1.14e-05   1.53e-05       6.68e-06   1.19e-05       1.73e-04   8.51e-05
    2480 (14)            3.24e-05   3.62e-05       3.24e-05   2.96e-05       3.62e-05   7.63e-05
    4000 (23)            2.96e-05   4.10e-05       2.72e-05   3.82e-05       3.93e-05   7.78e-05
    9840 (60)            7.63e-05   9.63e-05       7.63e-05   9.54e-05       3.42e-05   7.26e-05
    16240 (100)          1.52e-04   6.10e-05       1.48e-04   5.91e-05       6.06e-05   9.11e-05
    41600 (258)          9.25e-05   2.06e-04       9.30e-05   2.03e-04       5.89e-05   8.07e-05
(the 3-frame row's normalised floor is large because three near-equal frames divide by a small deviation)

Both GEMMs of the filter bank are the exact-fp32 kernel in every mode, so rows of a batch equal their own B = 1 calls bit for bit, also
across the 256-row switch at which `lin` would move to split-bf16."""
import contextlib

import numpy as np
import pytest
import torch

import frontend_cases as fc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = ("raw", "campplus", "w2vbert")


@pytest.fixture(scope="module")
def fb(device):
    from indextts_amd.frontend import KaldiFbank
    return KaldiFbank(device=device)


@contextlib.contextmanager
def _mode(mode):
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode(mode)
    try:
        yield
    finally:
        _lib.set_gemm_mode(old)


def _rows(device, lens):
    """[B, longest + 37] on the GPU: row b = the test signal of lens[b] samples, then a constant the kernels must never read"""
    x = np.full((len(lens), max(lens) + 37), 0.77, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = fc.fbank_audio(n)
    return torch.from_numpy(x).to(device)


def _worst(got, want):
    return float(np.abs(got - want).max()) if want.size else 0.0


@pytest.mark.parametrize("n", fc.FBANK_SINGLE)
def test_single_row_vs_host(device, fb, n):
    """shapes, valid lengths and padded positions exactly the host's; values within 4 x the float32 floor"""
    f_raw, f_cp, f_norm = fc.fbank_floors(n)
    T = fc.frames_of(n)
    x = _rows(device, [n])
    for scale in fc.SCALES:
        got, frames = fb(x, [n], scale=scale, mode="raw")
        want = fc.fbank_host(n, scale)
        assert frames == [T] and tuple(got.shape) == (1,) + want.shape == (1, T, 80)
        d = _worst(got[0].cpu().numpy(), want)
        print(f"n={n} scale={scale:g} raw: device {d:.3e} floor {f_raw:.3e}")
        assert d <= 4 * f_raw
    got, frames = fb.campplus_features(x, [n])
    want = fc.campplus_host(fc.fbank_audio(n))
    assert frames == [T] and tuple(got.shape) == (1,) + want.shape
    d = _worst(got[0].cpu().numpy(), want)
    print(f"n={n} campplus: device {d:.3e} floor {f_cp:.3e}")
    assert d <= 4 * f_cp
    if T < 2:
        with pytest.raises(ValueError, match="shorter than two"):
            fb.seamless_m4t_features(x, [n])
        return
    got, lens = fb.seamless_m4t_features(x, [n])
    want = fc.w2v_host(n)
    got = got.cpu().numpy()
    assert got.shape == want["input_features"].shape == (1, (T + 1) // 2, 160)
    assert lens == [int(want["attention_mask"].sum())] == [T // 2]
    if T % 2:      # (last frame | zeros), exactly as the host pads it, and not counted as valid
        assert not got[0, -1, 80:].any() and not want["input_features"][0, -1, 80:].any() and got[0, -1, :80].any()
    d = _worst(got, want["input_features"])
    print(f"n={n} w2vbert: device {d:.3e} floor {f_norm:.3e}")
    assert d <= 4 * f_norm


def test_shorter_than_one_frame_raises(device, fb):
    x = _rows(device, [399])
    for form in FORMS:
        with pytest.raises(ValueError):
            fb(x, [399], mode=form)
    with pytest.raises(ValueError):      # one short row among long ones
        fb(_rows(device, [4000, 399]), [4000, 399])


def _batch_equals_solo(device, fb, lens):
    x = _rows(device, list(lens))
    for form in FORMS:
        for scale in fc.SCALES:
            got, frames = fb(x, list(lens), scale=scale, mode=form)
            stack = 2 if form == "w2vbert" else 1
            assert frames == [fc.frames_of(n) for n in lens] and got.shape[1] == (max(frames) + stack - 1) // stack
            flat = got.reshape(len(lens), -1, 80)
            for b, n in enumerate(lens):
                solo, _ = fb(x[b:b + 1, :n].contiguous(), None, scale=scale, mode=form)
                solo = solo.reshape(1, -1, 80)
                t = solo.shape[1]
                assert torch.equal(flat[b, :t], solo[0]), (form, scale, b, (flat[b, :t] - solo[0]).abs().max().item())
                assert not flat[b, t:].any(), (form, scale, b)


def test_ragged_batch_rows_equal_their_own_call(device, fb):
    _batch_equals_solo(device, fb, fc.FBANK_RAGGED)


def test_rows_equal_their_own_call_across_the_256_row_switch(device, fb):
    """260 frames in the batch, at most 100 in a call of one row: `lin` would run the batch on split-bf16 and the single rows on the exact
    kernel.  Bit-equal in the default mode and in GEMM_F32, and the two modes bit-equal to each other: the exact path is used."""
    x = _rows(device, list(fc.FBANK_SWITCH))
    per_mode = []
    for mode in (_lib.GEMM_BF16X3, _lib.GEMM_F32):
        with _mode(mode):
            _batch_equals_solo(device, fb, fc.FBANK_SWITCH)
            per_mode.append(fb.seamless_m4t_features(x, list(fc.FBANK_SWITCH))[0])
    assert torch.equal(per_mode[0], per_mode[1])


def test_long_rows_vs_host(device, fb):
    """2.6 s, and the rows of the 256-row case, in one ragged batch: every form of every row within 4 x that row's float32 floor"""
    lens = [fc.FBANK_LONG] + list(fc.FBANK_SWITCH[1:])
    x = _rows(device, lens)
    raw = [fb(x, lens, scale=scale, mode="raw") for scale in fc.SCALES]
    cp, cp_frames = fb.campplus_features(x, lens)
    w2v, valid = fb.seamless_m4t_features(x, lens)
    for b, n in enumerate(lens):
        f_raw, f_cp, f_norm = fc.fbank_floors(n)
        d_raw = max(_worst(got[b, :frames[b]].cpu().numpy(), fc.fbank_host(n, scale)) for scale, (got, frames) in zip(fc.SCALES, raw))
        d_cp = _worst(cp[b, :cp_frames[b]].cpu().numpy(), fc.campplus_host(fc.fbank_audio(n)))
        want = fc.w2v_host(n)
        assert valid[b] == int(want["attention_mask"].sum())
        d_norm = _worst(w2v[b, :want["input_features"].shape[1]].cpu().numpy(), want["input_features"][0])
        print(f"n={n}: raw device {d_raw:.3e} floor {f_raw:.3e}; campplus {d_cp:.3e} / {f_cp:.3e}; w2vbert {d_norm:.3e} / {f_norm:.3e}")
        assert d_raw <= 4 * f_raw and d_cp <= 4 * f_cp and d_norm <= 4 * f_norm, n


def test_argument_checks(device, fb):
    x = _rows(device, [4000])
    with pytest.raises(RuntimeError):
        fb(x.cpu(), [4000])
    with pytest.raises(ValueError):
        fb(x, [4000], mode="mfcc")
    with pytest.raises(ValueError):
        fb(x, [x.shape[1] + 1])
