"""GPU: the device polyphase sinc resampler (indextts_amd/frontend.py::SincResampler, csrc/fbank.hip) against `audioio.sinc_resample`.

Tolerance.  The reference sums its float32 products in float32 (BLAS order); the device sums them in float64 and rounds once.  The floor
is the reference's own deviation from a float64 evaluation of the same taps on these inputs (frontend_cases.resample_f64), and the device
gets 4 x that.  Measured at amplitude <= 0.55 (floor: this file's inputs on the host; device: MI355X):

    float64 floor of the reference   1.68e-07
    device max |delta|               1.79e-07

Output lengths are exact: ceil(new * length / orig)."""
import math

import numpy as np
import pytest
import torch

import frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rs(device):
    from indextts_amd.frontend import SincResampler
    return SincResampler(device=device)


def _dev(device, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(1, -1)).to(device)


@pytest.mark.parametrize("orig_freq,new_freq", fc.RATE_PAIRS)
def test_rate_pair_vs_host(device, rs, orig_freq, new_freq):
    """tables from 1 x 41 (48000 -> 16000) to 320 x 459 (22050 -> 16000) and up-sampling; lengths 1, orig - 1, orig, orig + 1, 2 orig + 3, 0.2 s"""
    floor = fc.resample_floor()
    g = math.gcd(orig_freq, new_freq)
    worst = 0.0
    for n in fc.resample_lengths(orig_freq, new_freq):
        want = fc.resample_host(orig_freq, new_freq, n)
        got, lens = rs(_dev(device, fc.resample_audio(orig_freq, n)), None, orig_freq, new_freq)
        assert lens == [want.size] == [int(math.ceil((new_freq // g) * n / (orig_freq // g)))] and tuple(got.shape) == (1, want.size)
        worst = max(worst, float(np.abs(got[0].cpu().numpy() - want).max()))
    print(f"{orig_freq} -> {new_freq}: device {worst:.3e} floor {floor:.3e}")
    assert worst <= 4 * floor


def test_equal_rates_are_the_identity(device, rs):
    x = _dev(device, fc.resample_audio(16000, 3200))
    got, lens = rs(x, None, 16000, 16000)
    assert lens == [3200] and torch.equal(got, x)


def test_ragged_batch_rows_equal_their_own_call(device, rs):
    orig_freq, new_freq = 48000, 22050
    lens = list(fc.resample_lengths(orig_freq, new_freq)[3:])      # orig + 1, 2 orig + 3, 0.2 s
    x = np.full((3, max(lens) + 29), 0.77, np.float32)             # behind a row: a constant the kernel must never read
    for b, n in enumerate(lens):
        x[b, :n] = fc.resample_audio(orig_freq, n)
    x = torch.from_numpy(x).to(device)
    got, out_lens = rs(x, lens, orig_freq, new_freq)
    assert got.shape[1] == max(out_lens)
    for b, n in enumerate(lens):
        solo, sl = rs(x[b:b + 1, :n].contiguous(), None, orig_freq, new_freq)
        assert out_lens[b] == sl[0] == fc.resample_host(orig_freq, new_freq, n).size
        assert torch.equal(got[b, :sl[0]], solo[0]) and not got[b, sl[0]:].any()


def test_cut_keeps_the_first_samples(device, rs):
    """max_out (the 15 s cut of a long file) reads less input and leaves the kept samples bit for bit"""
    n = int(0.2 * 48000)
    x = _dev(device, fc.resample_audio(48000, n))
    full, fl = rs(x, None, 48000, 22050)
    cut, cl = rs(x, None, 48000, 22050, max_out=1000)
    assert fl[0] > 1000 and cl == [1000] and torch.equal(cut, full[:, :1000])
    same, sl = rs(x, None, 48000, 22050, max_out=fl[0] + 5)
    assert sl == fl and torch.equal(same, full)


def test_argument_checks(device, rs):
    x = _dev(device, fc.resample_audio(48000, 480))
    with pytest.raises(RuntimeError):
        rs(x.cpu(), None, 48000, 16000)
    with pytest.raises(ValueError):
        rs(x, [481], 48000, 16000)
    with pytest.raises(ValueError):
        rs(x[0], None, 48000, 16000)
