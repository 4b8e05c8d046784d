"""CPU: the one rule for a row's Exp(1) draws (gpt._draws) and its users -- UnifiedVoice._noise, DecodeSession._samplers and
BeamDecodeSession._beams.  The expected seeds come from torch itself: after torch.manual_seed(s) the unseeded entries, in entry order,
hold what successive torch.randint(0, 2 ** 62, (1,)) calls give after the same manual_seed, and nothing else touches the global RNG."""
import re
from types import SimpleNamespace

import pytest
import torch

from indextts_amd.config import GPTConfig
from indextts_amd.gpt import BeamDecodeSession, DecodeSession, UnifiedVoice, _draws

CFG = GPTConfig.tiny()
V = CFG.number_mel_codes
CPU = torch.device("cpu")


def _torch_seeds(s, n):
    torch.manual_seed(s)
    return [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(n)]


def test_draws_rule():
    want = _torch_seeds(1234, 3)
    torch.manual_seed(1234)
    assert [_draws(None, None, (4, 7), CPU) for _ in range(3)] == [(None, w) for w in want]
    torch.manual_seed(1234)
    assert _draws(None, 99, (4, 7), CPU) == (None, 99) and _draws(None, 2 ** 64 - 1, (4, 7), CPU) == (None, 2 ** 64 - 1)
    given = torch.rand(4, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(0))      # (not from the global RNG)
    noise, seed = _draws(given, 99, (4, 7), CPU)
    assert seed == 0 and noise.dtype == torch.float32 and noise.is_contiguous() and torch.equal(noise, given.float())
    noise, seed = _draws(given.tolist(), None, (4, 7), CPU)
    assert seed == 0 and torch.equal(noise, given.float())
    assert _draws(None, None, (4, 7), CPU) == (None, want[0])      # neither a seed nor explicit draws took anything from the global RNG
    with pytest.raises(ValueError, match=re.escape("exp_noise must be (4, 7)")):
        _draws(torch.zeros(3, 7), None, (4, 7), CPU)
    with pytest.raises(ValueError, match=re.escape("exp_noise must be [cap, V] = (4, 7)")):
        _draws(torch.zeros(4, 6), 5, (4, 7), CPU, "[cap, V] = ")
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed must be in"):
            _draws(None, bad, (4, 7), CPU)


def test_generate_draws():
    uv = object.__new__(UnifiedVoice)
    uv.cfg, uv.device = CFG, CPU
    want = _torch_seeds(7, 2)
    torch.manual_seed(7)
    assert uv._noise(None, None, (3, 2, V)) == (None, want[0])
    assert uv._noise(None, None, (3, 2, V), seed=5) == (None, 5)
    noise, seed = uv._noise(None, torch.Generator().manual_seed(11), (3, 2, V), seed=5)      # HF's order: one exponential_() per step
    g = torch.Generator().manual_seed(11)
    assert seed == 0 and torch.equal(noise, torch.stack([torch.empty(2, V).exponential_(1, generator=g) for _ in range(3)]))
    assert uv._noise(None, None, (3, 2, V)) == (None, want[1])
    with pytest.raises(ValueError, match=re.escape(f"exp_noise must be {(3, 2, V)}")):
        uv._noise(torch.zeros(3, 1, V), None, (3, 2, V))


def test_session_samplers_draw_in_entry_order():
    s = object.__new__(DecodeSession)
    s.gpt = SimpleNamespace(cfg=CFG, device=CPU)
    given = torch.rand(6, V)
    entries = [{"sampler": "hf"}, {"sampler": "accel", "seed": 42}, {"sampler": "hf", "exp_noise": given, "seed": 3}, {"sampler": "greedy"},
               {"sampler": "accel", "temperature": 0.5}, {}]
    want = _torch_seeds(99, 3)
    torch.manual_seed(99)
    arr, noises = s._samplers(entries, [6] * 6)
    assert [a.seed for a in arr] == [want[0], 42, 0, 0, want[1], want[2]]
    assert [a.mode for a in arr] == [1, 2, 1, 0, 2, 1]
    assert [nz is None for nz in noises] == [True, True, False, True, True, True] and torch.equal(noises[2], given)
    assert arr[2].exp_noise == noises[2].data_ptr() and arr[0].exp_noise is None
    with pytest.raises(ValueError, match=re.escape(f"exp_noise must be [cap, V] = {(6, V)}")):
        s._samplers({"exp_noise": torch.zeros(5, V)}, [6])


def test_beam_requests_draw_in_entry_order():
    b = object.__new__(BeamDecodeSession)
    b.gpt, b.num_beams = SimpleNamespace(cfg=CFG, device=CPU), 2
    given = torch.rand(4, 2 * V)
    want = _torch_seeds(5, 2)
    torch.manual_seed(5)
    arr, noises = b._beams([{}, {"seed": 8}, {"exp_noise": given}, {"do_sample": False}], [4] * 4)
    assert [a.seed for a in arr] == [want[0], 8, 0, want[1]]
    assert [nz is None for nz in noises] == [True, True, False, True] and torch.equal(noises[2], given)
    with pytest.raises(ValueError, match=re.escape(f"exp_noise must be [cap, num_beams * V] = {(4, 2 * V)}")):
        b._beams({"exp_noise": torch.zeros(4, V)}, [4])
