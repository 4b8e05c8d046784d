"""CPU: argument checking of the batched prompt entry points and of the device front-end's mirrors (indextts_amd/frontend.py,
prompt.py::encode_batch, infer_v2.py::PromptConditioning.from_features_batch) -- everything that must fail before a kernel is launched."""
import wave

import numpy as np
import pytest
import torch

from indextts_amd import _lib


def test_binding_lists_the_front_end_entries():
    for name in ("idxtts_fbank_create", "idxtts_fbank_frames", "idxtts_fbank_workspace_bytes", "idxtts_fbank_forward", "idxtts_resample_forward",
                 "idxtts_cond_forward_rows"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)


def test_mirrors_refuse_what_is_not_on_the_gpu():
    from indextts_amd.frontend import KaldiFbank, SincResampler
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KaldiFbank(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SincResampler(device="cpu")
    rs = SincResampler(device="cuda:0")      # holds no device state until it is called
    with pytest.raises(RuntimeError, match="expected a ROCm GPU tensor"):
        rs(torch.zeros(1, 480), None, 48000, 16000)
    with pytest.raises(RuntimeError, match="expected a ROCm GPU tensor"):
        rs(np.zeros((1, 480), np.float32), None, 48000, 16000)
    with pytest.raises(RuntimeError, match="expected a ROCm GPU tensor"):
        rs(torch.zeros(1, 480), None, 16000, 16000)      # also where nothing would be computed


def test_frontend_name_is_checked_before_anything_is_built():
    from indextts_amd.prompt import PromptEncoders, check_frontend
    assert check_frontend("host") == "host" and check_frontend("gpu") == "gpu"
    for bad in ("cuda", "GPU", None):
        with pytest.raises(ValueError, match="frontend must be one of"):
            PromptEncoders(None, None, None, None, frontend=bad)
    enc = PromptEncoders.__new__(PromptEncoders)      # with_frontend checks the name before it copies or builds anything
    with pytest.raises(ValueError, match="frontend must be one of"):
        enc.with_frontend("cuda")


def test_prompt_inputs(tmp_path):
    from indextts_amd.prompt import PromptAudio, RawAudio, as_prompt_input
    pa = PromptAudio(np.zeros(16000, np.float32))
    assert as_prompt_input(pa) is pa
    raw = as_prompt_input((np.zeros(100), 44100))
    assert isinstance(raw, RawAudio) and raw.sample_rate == 44100 and raw.samples.dtype == np.float32
    with wave.open(str(tmp_path / "p.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(np.arange(200, dtype="<i2").tobytes())
    raw = as_prompt_input(str(tmp_path / "p.wav"))
    assert isinstance(raw, RawAudio) and raw.sample_rate == 48000 and raw.samples.shape == (2, 100)
    for bad in (3.5, None, (np.zeros(4), np.zeros(4))):
        with pytest.raises(TypeError):
            as_prompt_input(bad)


def test_from_features_batch_checks_its_list():
    from indextts_amd.infer_v2 import PromptConditioning, PromptFeatures
    with pytest.raises(ValueError):
        PromptConditioning.from_features_batch(None, [])
    two = PromptFeatures(torch.zeros(2, 5, 8), torch.zeros(1, 4), torch.zeros(1, 3, 4), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="one prompt"):
        PromptConditioning.from_features_batch(None, [two])
