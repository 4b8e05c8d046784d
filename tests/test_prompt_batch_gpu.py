"""GPU: several voices through the prompt block at once (PromptEncoders.encode_batch, PromptConditioning.from_features_batch) with the
host and the device front-end, on the tiny encoders of tests/test_prompt_gpu.py: three voices of 2.6 s, 1.7 s and 0.9 s, the first and
the last with an emotion prompt.

Bounds.  A row of the ragged w2v-bert batch against its own call: the 2e-4 test_prompt_gpu.py allows.  Codec, mel, CAMPPlus and the
length regulator run on their B = 1 entries, so they are bit-equal to those entries on the same input; every stage gets THIS path's
input handed over, so a near-tie of the nearest-code search cannot cascade.  The device front-end's features against the host's, on the
samples the device produced: 4 x the float32 floor of these waveforms (frontend_cases.fbank_floors_of; on this test's five waveforms the
floors are 2.8e-04 log-mel minus mean and 1.2e-04 normalised, the device's deviations 2.3e-04 and 1.9e-04); the device resampler
against the host's: 4 x the float64 floor of the same inputs (2.3e-07; device 2.4e-07).  Conditioning rows against `from_features`: the
1e-4 tests/test_cond_gpu.py allows its ragged rows."""
import warnings

import numpy as np
import pytest
import torch

import frontend_cases as fc
from indextts_amd import audioio, features, synth, weights
from test_prompt_gpu import _cfgs

pytestmark = pytest.mark.gpu

SECONDS = (2.6, 1.7, 0.9)
EMO_SECONDS = (1.7, None, 1.1)


@pytest.fixture(scope="module")
def rig(device):
    from indextts_amd.infer_v2 import IndexTTS2
    from indextts_amd.prompt import PromptEncoders
    cfg, wcfg, ccfg, pcfg = _cfgs()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/pbatch/gpt")
    wg.update(weights.synth_gpt_cond_weights(cfg.gpt, tag="t/pbatch/gpt"))
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4           # fixed-length utterances
    tts = IndexTTS2.from_state_dicts(cfg, wg, weights.synth_s2mel_weights(cfg.s2mel, tag="t/pbatch/s2mel"),
                                     weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/pbatch/voc"), device=device)
    gpu = PromptEncoders(weights.synth_w2vbert_weights(wcfg, tag="t/pbatch/w2v"), weights.synth_repcodec_weights(ccfg, tag="t/pbatch/codec"),
                         weights.synth_campplus_weights(pcfg, tag="t/pbatch/campplus"), tts.s2mel, device=device, w2vbert_cfg=wcfg,
                         codec_cfg=ccfg, campplus_cfg=pcfg, mel_kwargs=dict(num_mels=cfg.s2mel.in_channels), frontend="gpu")
    host = gpu.with_frontend("host")    # the same encoders behind the host front-end
    return cfg, tts, host, gpu


def _voices():
    from indextts_amd.prompt import PromptAudio
    spk = [PromptAudio(fc.audio(f"t/pbatch/a16/{i}", 16000, 16000 * s), fc.audio(f"t/pbatch/a22/{i}", 22050, 22050 * s)) for i, s in enumerate(SECONDS)]
    emo = [None if s is None else PromptAudio(fc.audio(f"t/pbatch/e16/{i}", 16000, 16000 * s)) for i, s in enumerate(EMO_SECONDS)]
    return spk, emo


def _check_downstream(enc, feats, i, a22, cp_feat):
    """codec + regulator, mel and CAMPPlus of row i: bit-equal to the B = 1 entries on the handed-over inputs"""
    _, S_ref = enc.codec.quantize(feats[i].spk_cond_emb)
    assert torch.equal(feats[i].ref_mel, enc.mel(a22))
    pc = enc.s2mel.length_regulator(S_ref, ylens=torch.LongTensor([feats[i].ref_mel.size(2)]), n_quantizers=3, f0=None)[0]
    assert torch.equal(feats[i].prompt_condition, pc)
    assert torch.equal(feats[i].style, enc.campplus(cp_feat))


def test_host_frontend_rows_vs_encode(device, rig):
    cfg, tts, enc, _ = rig
    spk, emo = _voices()
    feats = enc.encode_batch(spk, emo)
    assert len(feats) == 3 and feats[1].emo_cond_emb is None
    for i in range(3):
        solo = enc.get_emb(spk[i].audio_16k)
        assert feats[i].spk_cond_emb.shape == solo.shape and (feats[i].spk_cond_emb - solo).abs().max().item() <= 2e-4
        if emo[i] is not None:
            solo = enc.get_emb(emo[i].audio_16k)
            assert feats[i].emo_cond_emb.shape == solo.shape and (feats[i].emo_cond_emb - solo).abs().max().item() <= 2e-4
        one = enc.encode(spk[i], emo[i])
        assert torch.equal(feats[i].ref_mel, one.ref_mel) and torch.equal(feats[i].style, one.style)
        fb = fc.campplus_host(np.asarray(spk[i].audio_16k))
        _check_downstream(enc, feats, i, torch.from_numpy(spk[i].audio_22k[None]).to(device), torch.from_numpy(fb[None]))


def _raw_voices():
    """the same three voices as files would give them: 48 kHz samples, a ready PromptAudio, (samples, 22 050 Hz); emotion: 48 kHz, none, ready"""
    from indextts_amd.prompt import PromptAudio, RawAudio
    spk, emo = _voices()
    stereo = np.stack([fc.audio("t/pbatch/raw48/l", 48000, 48000 * SECONDS[0]), fc.audio("t/pbatch/raw48/r", 48000, 48000 * SECONDS[0])])
    spk = [RawAudio(stereo, 48000), spk[1], (fc.audio("t/pbatch/raw22", 22050, 22050 * SECONDS[2]), 22050)]
    emo = [RawAudio(fc.audio("t/pbatch/rawe48", 48000, 48000 * EMO_SECONDS[0]), 48000), None, emo[2]]
    return spk, emo


def test_gpu_frontend_chain(device, rig):
    cfg, tts, host, enc = rig
    spk, emo = _raw_voices()
    feats, mid = enc._encode_batch(spk, emo)
    assert len(feats) == 3 and feats[1].emo_cond_emb is None and len(mid["audio_16k"]) == 5
    # -- the device resampler: each step against the host's on the input the device had
    mono = spk[0].samples.mean(axis=0, dtype=np.float32)
    a22 = mid["audio_22k"][0][0].cpu().numpy()
    a16 = mid["audio_16k"][0].cpu().numpy()
    e16 = mid["audio_16k"][3].cpu().numpy()
    steps = ((mono, 48000, 22050, a22), (a22, 22050, 16000, a16), (spk[2][0], 22050, 16000, mid["audio_16k"][2].cpu().numpy()),
             (emo[0].samples, 48000, 16000, e16))
    floor = worst = 0.0
    for x, o, nw, got in steps:
        want = audioio.sinc_resample(x, o, nw)
        assert got.shape == want.shape
        floor = max(floor, float(np.abs(want - fc.resample_f64(x, o, nw)).max()))
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"resampler: device {worst:.3e} floor {floor:.3e}")
    assert worst <= 4 * floor
    assert np.array_equal(mid["audio_16k"][1].cpu().numpy(), spk[1].audio_16k) and np.array_equal(mid["audio_22k"][2][0].cpu().numpy(), spk[2][0])
    # -- the device filter bank: features of the samples the device produced against the host's features of the same samples
    waves = [a.cpu().numpy() for a in mid["audio_16k"]]
    _, f_cp, f_norm = fc.fbank_floors_of(tuple(waves))
    d_cp = d_norm = 0.0
    for r, w in enumerate(waves):
        f = features.seamless_m4t_features(w)
        t = f["input_features"].shape[1]
        assert mid["feature_lens"][r] == int(f["attention_mask"].sum())
        got = mid["input_features"][r].cpu().numpy()
        d_norm = max(d_norm, float(np.abs(got[:t] - f["input_features"][0]).max()))
        assert not got[t:].any()
        if r < 3:
            want = fc.campplus_host(w)
            assert mid["campplus_frames"][r] == want.shape[0] and tuple(mid["campplus_feats"][r].shape) == (1,) + want.shape
            d_cp = max(d_cp, float(np.abs(mid["campplus_feats"][r][0].cpu().numpy() - want).max()))
    print(f"filter bank: campplus device {d_cp:.3e} floor {f_cp:.3e}; w2vbert device {d_norm:.3e} floor {f_norm:.3e}")
    assert d_cp <= 4 * f_cp and d_norm <= 4 * f_norm
    # -- everything downstream on handed-over inputs
    x = mid["input_features"]
    for r in range(5):
        n = mid["feature_lens"][r]
        t = (features.seamless_m4t_features(waves[r])["input_features"]).shape[1]
        solo = enc.semantic(x[r:r + 1, :t].contiguous(), torch.ones(1, t, dtype=torch.int64) * (torch.arange(t) < n))[:, :n]
        got = feats[r].spk_cond_emb if r < 3 else feats[(0, 2)[r - 3]].emo_cond_emb
        assert got.shape == solo.shape and (got - solo).abs().max().item() <= 2e-4
    for i in range(3):
        _check_downstream(enc, feats, i, mid["audio_22k"][i], mid["campplus_feats"][i])


def test_from_features_batch_vs_from_features(device, rig):
    """Each element against `from_features` of the same PromptFeatures, within the 1e-4 tests/test_cond_gpu.py allows its ragged rows, and
    the list as `cond=` of synthesize_batch: one waveform per row.  The conditioning encoders run once over the right-padded batch with
    each row's frame count as its extent (idxtts_cond_forward_rows).  Here the batch (192 subsampled rows) and the single calls are on the
    same GEMM kernel and agree to the last bit; across the 256-row switch: the next test.  With the reference's masks alone the padded rows miss this bound
    by 30 x: the CPU oracle on this rig's weights, rows of 130 / 85 / 44 frames padded to 130, gives latent |padded row - own call| =
    1.1e-06 / 2.8e-03 / 6.6e-03 -- a padded frame's pointwise-conv bias reaches the last valid frames through the depthwise taps --
    and 1.1e-06 / 1.1e-06 / 1.2e-06 once the gated rows behind a row's extent are zeroed, which is what the kernels do."""
    from indextts_amd.infer_v2 import PromptConditioning
    cfg, tts, enc, _ = rig
    spk, emo = _voices()
    feats = enc.encode_batch(spk, emo)
    conds = PromptConditioning.from_features_batch(tts.gpt, feats, emo_alpha=0.7)
    assert len(conds) == 3
    worst = []
    for c, f in zip(conds, feats):
        one = PromptConditioning.from_features(tts.gpt, f, emo_alpha=0.7)
        assert c.spk_cond_latent.shape == one.spk_cond_latent.shape and c.emo_vec.shape == one.emo_vec.shape
        assert c.style is f.style and c.prompt_condition is f.prompt_condition and c.ref_mel is f.ref_mel
        worst.append(((c.spk_cond_latent - one.spk_cond_latent).abs().max().item() / max(1.0, one.spk_cond_latent.abs().max().item()),
                      (c.emo_vec - one.emo_vec).abs().max().item() / max(1.0, one.emo_vec.abs().max().item())))
    print("from_features_batch vs from_features, (latent, emotion vector) relative to max(1, |ref|):", worst)
    assert all(a <= 1e-4 and b <= 1e-4 for a, b in worst), worst
    text = torch.from_numpy(synth.integers("t/pbatch/text", (3, 7), 2, cfg.gpt.number_text_tokens))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs = tts.synthesize_batch(text, conds, max_mel_tokens=12)
    assert len(wavs) == 3 and all(w.numel() > 0 and bool(torch.isfinite(w.float()).all()) for w in wavs)


def test_from_features_batch_across_the_256_row_switch(device, rig):
    """Three voices of 251 / 240 / 200 feature frames: 3 x 125 = 375 subsampled rows in the batch, on which the conditioning encoders'
    projections run on the split-bf16 GEMM, against at most 125 in a voice's own call, which stays on the exact kernel.  The rows are then
    not bit-equal to `from_features` (they are when both sides run the same kernel, as in the test above) and move with the size of the
    batch they share; what holds is the 1e-4 of tests/test_cond_gpu.py, in the default mode and in GEMM_F32.
    Feature width 96 < frames, so the reference's "length" (shape[-1]) masks each row beyond 96 frames, in both forms alike."""
    from indextts_amd import _lib
    from indextts_amd.infer_v2 import PromptConditioning, PromptFeatures
    cfg, tts, enc, _ = rig
    D = cfg.gpt.cond_module.input_size
    t = lambda tag, shape: torch.from_numpy(synth.uniform(f"t/pbatch/switch/{tag}", shape, 1.0))
    feats = [PromptFeatures(t(f"spk{i}", (1, n, D)), t(f"style{i}", (1, cfg.s2mel.style_dim)), t(f"pc{i}", (1, 9, cfg.s2mel.content_dim)),
                            t(f"mel{i}", (1, cfg.s2mel.in_channels, 9)), t(f"emo{i}", (1, m, D)) if m else None)
             for i, (n, m) in enumerate(((251, 230), (240, None), (200, 251)))]
    T2 = (251 - 3) // 2 + 1
    assert 3 * T2 >= 256 > T2
    old = _lib.get_gemm_mode()
    try:
        for mode in (_lib.GEMM_BF16X3, _lib.GEMM_F32):
            _lib.set_gemm_mode(mode)
            conds = PromptConditioning.from_features_batch(tts.gpt, feats, emo_alpha=0.7)
            worst = []
            for c, f in zip(conds, feats):
                one = PromptConditioning.from_features(tts.gpt, f, emo_alpha=0.7)
                worst.append(((c.spk_cond_latent - one.spk_cond_latent).abs().max().item() / max(1.0, one.spk_cond_latent.abs().max().item()),
                              (c.emo_vec - one.emo_vec).abs().max().item() / max(1.0, one.emo_vec.abs().max().item())))
            print(f"GEMM mode {mode}: from_features_batch ({3 * T2} rows) vs from_features (<= {T2} rows), relative to max(1, |ref|):", worst)
            assert all(a <= 1e-4 and b <= 1e-4 for a, b in worst), (mode, worst)
    finally:
        _lib.set_gemm_mode(old)


def test_cond_rows_vs_oracle_own_call(device, rig):
    """idxtts_cond_forward_rows through the mirrors: rows of 61 / 20 / 7 / 3 frames in one padded batch, each against the CPU oracle's
    call of that row alone (the 1e-4 of tests/test_cond_gpu.py); the existing masked form on the same batch is left as it was, and
    differs from the own call where the reference's does."""
    from oracle import cond as oc
    cfg, tts, enc, _ = rig
    w = {k: torch.from_numpy(v) for k, v in weights.synth_gpt_cond_weights(cfg.gpt, tag="t/pbatch/gpt").items()}
    D, lens = cfg.gpt.cond_module.input_size, (61, 20, 7, 3)
    rows = [torch.from_numpy(synth.uniform(f"t/pbatch/cond/{n}", (1, n, D), 1.0)) for n in lens]
    x = torch.zeros(len(lens), max(lens), D)
    for i, r in enumerate(rows):
        x[i, : r.shape[1]] = r[0]
    ln, ex = torch.tensor([D] * len(lens)), torch.tensor(lens)
    lat = tts.gpt.get_conditioning(x.transpose(1, 2), ln, extents=ex).cpu()
    ev = tts.gpt.get_emovec(x, ln, extents=ex).cpu()
    masked = tts.gpt.get_conditioning(x.transpose(1, 2), ex).cpu()
    with torch.no_grad():
        for i, r in enumerate(rows):
            ref_lat, ref_ev = oc.get_conditioning(w, cfg.gpt, r, torch.tensor([D])), oc.get_emovec(w, cfg.gpt, r, torch.tensor([D]))
            assert (lat[i:i + 1] - ref_lat).abs().max().item() <= 1e-4 * max(1.0, ref_lat.abs().max().item()), i
            assert (ev[i:i + 1] - ref_ev).abs().max().item() <= 1e-4 * max(1.0, ref_ev.abs().max().item()), i
        ref_masked = oc.get_conditioning(w, cfg.gpt, x, ex)
    assert (masked - ref_masked).abs().max().item() <= 1e-4 * max(1.0, ref_masked.abs().max().item())
    with pytest.raises(RuntimeError):
        tts.gpt.get_emovec(x, ln, extents=torch.tensor([61, 20, 7, 2]))      # a row needs 3 frames
    with pytest.raises(ValueError):
        tts.gpt.get_emovec(x, ln, extents=torch.tensor([61, 20]))


def test_argument_checks(device, rig):
    cfg, tts, enc, _ = rig
    spk, emo = _voices()
    with pytest.raises(ValueError):
        enc.encode_batch(spk, emo[:2])
    with pytest.raises(ValueError):
        enc.encode_batch([])
    with pytest.raises(ValueError):
        enc.encode_batch([emo[0]])               # a speaker prompt needs its 22.05 kHz side
    with pytest.raises(TypeError):
        enc.encode_batch([3.5])
