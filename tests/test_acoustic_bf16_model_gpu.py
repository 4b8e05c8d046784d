"""idxtts_set_acoustic_bf16 through the models: the CFM estimator (five-tap gates, the rotary epilogue, the plane hand-over into the
planes attention) against the CPU oracle, and the tiny pipeline end to end -- the GPT's codes and latents do not move by one bit,
mel and waveform move by bf16 rounding.

The error bounds here are 3 x what one run on an MI355X gave (results are deterministic: the margin is for later changes of
summation order, not for noise); the measured values stand in the docstrings and in profiles/README.md "Acoustic bf16"."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig, S2MelConfig

pytestmark = pytest.mark.gpu

# measured: switch-on estimator output against the fp32 CPU oracle, worst row of the two (mean, max)
CFM_MEAN_MEASURED, CFM_MAX_MEASURED = 6.201e-3, 4.825e-2
# measured: switch-on waveform against the switch-off waveform, fraction of full scale (max), and mel (mean abs)
WAV_MAX_MEASURED, MEL_MEAN_MEASURED = 2.386e-3, 7.239e-3


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _lib.set_acoustic_bf16(False)
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)


def test_estimator_with_bf16_products_vs_oracle(device):
    """The CFM case of tests/test_gemm_v2_mfma_shape_gpu.py (hidden 192, 3 heads, depth 3, lens [149, 131]: 2B*T = 596 rows, every
    GEMM on the LDS-DMA kernel) with the switch on.  Measured against the oracle: mean 6.201e-3, max 4.825e-2 (switch off:
    mean 1.229e-5); asserted at 3 x each."""
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

    def run():
        return sm.cfm_inference(mu, torch.LongTensor(lens), prompt, st, None, 2, inference_cfg_rate=0.7, z=z,
                                prompt_lens=torch.LongTensor(plens)).cpu()
    off = run()
    _lib.set_acoustic_bf16(True)
    on = run()
    _lib.set_acoustic_bf16(False)
    assert torch.equal(run(), off)                      # switch off is unchanged by having toggled
    mean_on = max_on = mean_off = 0.0
    for b in range(B):
        Lb, Pb = lens[b], plens[b]
        ref = osm.cfm_inference(tw, cfg, mu[b:b + 1, :Lb], torch.LongTensor([Lb]), prompt[b:b + 1, :, :Pb], st[b:b + 1],
                                z[b:b + 1, :, :Lb], 2, 0.7)
        e_on, e_off = (on[b, :, :Lb] - ref[0]).abs(), (off[b, :, :Lb] - ref[0]).abs()
        mean_on, max_on, mean_off = max(mean_on, e_on.mean().item()), max(max_on, e_on.max().item()), max(mean_off, e_off.mean().item())
        assert e_on.mean().item() > e_off.mean().item(), b          # the single-product path ran
    print(f"MEASURED cfm bf16 vs oracle: mean {mean_on:.3e} max {max_on:.3e} (switch off: mean {mean_off:.3e})")
    assert np.isfinite(max_on)
    assert mean_on <= 3 * CFM_MEAN_MEASURED and max_on <= 3 * CFM_MAX_MEASURED, (mean_on, max_on)


def test_tiny_pipeline_codes_and_latents_untouched(device):
    """IndexTTS2.from_state_dicts(..., acoustic_bf16=True) on the tiny configuration, 4 rows x 48 codes (B*T >= 256 rows in the CFM):
    greedy codes and the latent pass are bit-identical to switch off, the waveform is finite and within 3 x the measured distance from
    the switch-off waveform.  Measured: max |wav| difference 2.386e-3 of full scale, mel mean difference 7.239e-3."""
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/abf16/gpt")
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/abf16/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/abf16/voc")
    cond = PromptConditioning.synthetic(cfg, prompt_frames=9, tag="t/abf16/prompt")
    B, L, MAXM = 4, 8, 48
    text = torch.from_numpy(synth.integers("t/abf16/text", (B, L), 2, cfg.gpt.number_text_tokens))
    runs = {}
    for on in (False, True):
        tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device, acoustic_bf16=on)
        assert _lib.get_acoustic_bf16() is on
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs[on] = tts.synthesize_batch(text, cond, max_mel_tokens=MAXM, noise_seeds=list(range(11, 11 + B)), return_intermediates=True)
    (wav_off, mid_off), (wav_on, mid_on) = runs[False], runs[True]
    Tp = cond.ref_mel.shape[-1]
    assert B * (Tp + min(mid_off["target_lens"])) >= 256, "the CFM must run from 256 rows up"
    assert mid_on["code_lens"] == mid_off["code_lens"] and torch.equal(mid_on["codes"], mid_off["codes"])
    assert torch.equal(mid_on["latent"], mid_off["latent"])
    mel_d = (mid_on["mel"] - mid_off["mel"]).abs().mean().item()
    wav_d = 0.0
    for b in range(B):
        assert torch.isfinite(wav_on[b]).all()
        wav_d = max(wav_d, (wav_on[b] - wav_off[b]).abs().max().item() / 32767.0)
    print(f"MEASURED tiny pipeline bf16 vs switch off: max |wav| diff {wav_d:.3e} of full scale, mel mean diff {mel_d:.3e}")
    assert wav_d > 0.0 and mel_d > 0.0                  # the acoustic stage did change
    assert wav_d <= 3 * WAV_MAX_MEASURED and mel_d <= 3 * MEL_MEAN_MEASURED, (wav_d, mel_d)
