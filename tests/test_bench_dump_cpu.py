"""CPU: bench.py --dump-outputs writes float32 / float64 .npy files within its 64 MB budget, small outputs whole and large ones as
the same seeded sample on every run (so that two builds compare element for element)."""
import os

import numpy as np
import torch

import bench


def test_small_outputs_are_written_whole(tmp_path):
    arrays = {"wavs": torch.randn(4, 1000), "wav_lengths": torch.tensor([1000.0, 900.0, 800.0, 700.0], dtype=torch.float64),
              "latent": torch.randn(3, 5).bfloat16()}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["latent.npy", "wav_lengths.npy", "wavs.npy"]
    for name, want in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == (np.float64 if want.dtype == torch.float64 else np.float32)
        np.testing.assert_array_equal(got, want.to(torch.float64 if want.dtype == torch.float64 else torch.float32).numpy())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    limit = 1 << 20
    arrays = {"wavs": torch.randn(16, 40000), "wav_lengths": torch.full((16,), 40000.0, dtype=torch.float64)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= limit
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "wav_lengths.npy"), arrays["wav_lengths"].numpy())      # fits: whole
    a, b = np.load(tmp_path / "a" / "wavs.npy"), np.load(tmp_path / "b" / "wavs.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and 0.5 * limit / 4 < a.size < limit / 4
    np.testing.assert_array_equal(a, b)
    assert np.isin(a, arrays["wavs"].numpy().reshape(-1)).all()
