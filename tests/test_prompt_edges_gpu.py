"""GPU: the five prompt-side HIP models at the lengths where their kernels branch, against their CPU oracles, in both arithmetic modes.

Every model runs on every request at whatever length the user's audio has; the other prompt tests pin one or two lengths each.
Here each model is swept over its tails, reflections, partial segments and limits:
  melspec      one frame (N = pad + 1), N just above the pad, N mod hop in {0, 1, hop - 1}, B * T on both sides of 256 rows
  w2v-bert     ragged rows of length 1, shorter than the depthwise kernel (31), shorter than the distance table (64), B * T at 255 /
               256 / 280 rows, B up to 5
  RepCodec     T = 1 ... 8 (shorter than the k7 input conv and the k7 depthwise convs), B up to 5
  CAMPPlus     T = 8 (the limit), odd and even T, T2 = 100 / 200 (whole segments of SEG_LEN) and 101 (a one-frame last segment),
               T2 = 255 / 256 (the 256-row switch), B = 3 with different rows
  conditioning lengths 3 / 4 / 5 (len2 = 1, 1, 2), a row longer than T ("no padding"), T2 = pe_len, B * T2 around 256
Each ragged or batched case also checks that a batch row equals its own B = 1 call (unpadded, except for the conditioning
encoders, whose reference lets padding reach valid frames: there the solo call keeps the row's padding): bit-exact when both calls run the same GEMM
kernels (GEMM_F32 mode, or every launch on the same side of the 256-row switch of `lin()`, model_util.h), within the oracle
tolerance when the switch separates them.  The tolerances are those of the existing tests of each model."""
import dataclasses

import numpy as np
import pytest
import torch

from indextts_amd import synth, weights
from indextts_amd.config import CamPPlusConfig, CondModuleConfig, GPTConfig, RepCodecConfig, W2VBertConfig

pytestmark = pytest.mark.gpu
SWITCH = 256                  # lin(): the split-bf16 GEMM takes launches of >= 256 rows in GEMM_BF16X3 mode
MODE = {"bf16x3": True}


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def arith(request):
    from indextts_amd import _lib
    _lib.set_gemm_mode(_lib.GEMM_F32 if request.param == "f32" else _lib.GEMM_BF16X3)
    MODE["bf16x3"] = request.param == "bf16x3"
    torch.set_num_threads(16)
    yield request.param
    _lib.set_gemm_mode(_lib.GEMM_BF16X3)
    MODE["bf16x3"] = True


def _same_kernels(batch_rows, solo_rows):
    """True when every lin() launch of the batched call runs the same GEMM kernel as the matching launch of the solo call."""
    if not MODE["bf16x3"]:
        return True
    return all((a >= SWITCH) == (b >= SWITCH) for a, b in zip(batch_rows, solo_rows))


def _row_vs_solo(row, solo, same, tol, what):
    """a batch row against its own B = 1 call"""
    if same:
        assert torch.equal(row, solo), f"{what}: batch row differs from its solo call although both run the same GEMM kernels"
    else:
        err = (row - solo).abs().max().item()
        assert err <= tol, f"{what}: batch row vs solo call {err} > {tol} (the 256-row GEMM switch separates the two calls)"


def _tw(w):
    return {k: torch.from_numpy(v) for k, v in w.items()}


# ---------------------------------------------------------------------------------------------------------------- melspec
@pytest.fixture(scope="module")
def mel(device):
    from indextts_amd.audio import MelSpectrogram, slaney_mel_basis
    return MelSpectrogram(device=device), torch.from_numpy(slaney_mel_basis(22050, 1024, 80))


def _audio(tag, B, n):
    t = np.arange(n) / 22050.0
    f = 200.0 + 150.0 * np.arange(B)[:, None]
    y = 0.5 * np.sin(2 * np.pi * f * t[None]) + 0.1 * synth.uniform(f"t/edges/mel/{tag}", (B, n), 1.0)
    return torch.from_numpy(y.astype(np.float32))


def _check_mel(mf, basis, y, device, what):
    from oracle import audio as oa
    B, n = y.shape
    got = mf(y.to(device)).cpu()
    with torch.no_grad():
        want = oa.mel_spectrogram(y, basis)
    T = n // 256
    assert got.shape == want.shape == (B, 80, T), what
    err = (got - want).abs()
    assert err.max().item() <= 1e-3 and err.mean().item() <= 1e-5, (what, err.max().item(), err.mean().item())
    return got


# pad = (n_fft - hop) / 2 = 384: the reflection at the end reaches back to sample N - 1 - pad
MEL_CASES = [(1, 385), (2, 386), (1, 400), (3, 511), (2, 512), (2, 513), (1, 2560), (2, 2561), (3, 2815),
             (2, 128 * 256 + 5), (3, 90 * 256), (2, 300 * 256 + 255), (1, 255 * 256), (1, 256 * 256 + 1)]


@pytest.mark.parametrize("B,n", MEL_CASES)
def test_melspec_edges(device, mel, B, n):
    mf, basis = mel
    y = _audio(f"{B}/{n}", B, n)
    got = _check_mel(mf, basis, y, device, (B, n))
    if B > 1:
        T = n // 256
        for b in range(B):
            solo = mf(y[b:b + 1].to(device)).cpu()
            _row_vs_solo(got[b], solo[0], _same_kernels([B * T], [T]), 1e-3, f"melspec B={B} N={n} row {b}")


def test_melspec_limits(device, mel):
    mf, basis = mel
    with pytest.raises(RuntimeError, match="reflect padding needs more samples"):
        mf(torch.zeros(1, 384, device=device))                 # N = pad: one frame would fit, the reflection would not
    with pytest.raises(ValueError, match="shorter than one frame"):
        mf(torch.zeros(2, 200, device=device))
    _check_mel(mf, basis, _audio("after", 2, 385), device, "after the refused calls")


# ---------------------------------------------------------------------------------------------------------------- w2v-bert
@pytest.fixture(scope="module")
def w2v(device):
    from indextts_amd.semantic import SemanticModel
    cfg = dataclasses.replace(W2VBertConfig(), num_layers=2)      # real widths: 1024 / 4096 / 16 heads / k31 / 64 left, 8 right
    w = weights.synth_w2vbert_weights(cfg, tag="t/edges/w2v")
    return cfg, _tw(w), SemanticModel(w, cfg, device=device)


def _check_w2v(cfg, tw, sm, feats, lens, what):
    from oracle import semantic as osem
    B, T, _ = feats.shape
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).long()
    with torch.no_grad():
        want = osem.get_emb(tw, cfg, feats, mask)
    got = sm(feats, mask).cpu()
    scale = max(1.0, want.abs().max().item())
    for b, n in enumerate(lens):
        err = (got[b, :n] - want[b, :n]).abs()
        assert err.max().item() <= 3e-4 * scale and err.mean().item() <= 3e-5 * scale, (what, b, n, err.max().item(), err.mean().item())
    return got, scale


W2V_CASES = [
    (1, [1]),
    (5, [5, 1, 3, 5, 2]),                 # every row shorter than the depthwise kernel
    (51, [51, 1, 17, 40, 2]),             # B * T = 255 rows
    (64, [64, 30, 31, 63]),               # B * T = 256 rows; rows at and around k = 31, just under left_max = 64
    (70, [70, 1, 30, 63]),                # B * T = 280 rows, solo calls below 256
    (300, [300, 260]),                    # both sides above 256 rows
]


@pytest.mark.parametrize("T,lens", W2V_CASES)
def test_w2vbert_ragged(device, w2v, T, lens):
    cfg, tw, sm = w2v
    B = len(lens)
    feats = torch.from_numpy(synth.uniform(f"t/edges/w2v/{B}/{T}", (B, T, cfg.input_dim), 1.5))    # padding left as noise: masked
    got, scale = _check_w2v(cfg, tw, sm, feats, lens, (T, lens))
    if B > 1:
        for b, n in enumerate(lens):
            solo = sm(feats[b:b + 1, :n]).cpu()
            _row_vs_solo(got[b, :n], solo[0], _same_kernels([B * T], [n]), 3e-4 * scale, f"w2v-bert T={T} lens={lens} row {b}")


def test_w2vbert_limits(device, w2v):
    cfg, tw, sm = w2v
    feats = torch.from_numpy(synth.uniform("t/edges/w2v/limit", (2, 9, cfg.input_dim), 1.5))
    mask = torch.ones(2, 9, dtype=torch.long)
    mask[1] = 0
    with pytest.raises(RuntimeError, match="at least one valid frame"):
        sm(feats, mask)
    _check_w2v(cfg, tw, sm, feats, [9, 1], "after the refused call")


# ---------------------------------------------------------------------------------------------------------------- RepCodec
def _margin(z_e, codebook):
    """as tests/test_codec_gpu.py: the cosine-similarity gap between the best and second-best code of every frame"""
    e = torch.nn.functional.normalize(z_e.reshape(-1, z_e.shape[-1]))
    c = torch.nn.functional.normalize(codebook)
    top = (e @ c.t()).topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]).reshape(z_e.shape[:-1])


@pytest.fixture(scope="module")
def codec(device):
    from indextts_amd.codec import SemanticCodec
    cfg = RepCodecConfig()                                        # real widths: 1024 -> 384 x 12 ConvNeXt blocks -> 8-dim codes, 8192
    w = weights.synth_repcodec_weights(cfg, tag="t/edges/codec")
    return cfg, _tw(w), SemanticCodec(w, cfg, device=device), {"frames": 0, "same": 0}


@pytest.mark.parametrize("B,T", [(3, 1), (3, 2), (2, 3), (4, 4), (3, 5), (2, 6), (3, 7), (2, 8), (5, 1), (5, 9)])
def test_repcodec_short(device, codec, B, T):
    from oracle import codec as ocd
    cfg, tw, sc, tally = codec
    x = torch.from_numpy(synth.uniform(f"t/edges/codec/{B}/{T}", (B, T, cfg.hidden_size), 1.0))
    with torch.no_grad():
        want_idx, want_q = ocd.quantize(tw, x)
        z_e = torch.nn.functional.conv1d(ocd.encoder(tw, x).transpose(1, 2), tw["quantizer.quantizers.0.in_project.weight"],
                                         tw["quantizer.quantizers.0.in_project.bias"]).transpose(1, 2)
    idx, q = sc.quantize(x)
    idx, q = idx.cpu(), q.cpu()
    same = idx == want_idx
    gap = _margin(z_e, tw["quantizer.quantizers.0.codebook.weight"])
    assert bool((same | (gap < 1e-4)).all()), ("a frame with a clear nearest code resolved differently", B, T)
    if bool(same.any()):
        err = (q - want_q).abs().amax(-1)
        assert err[same].max().item() <= 5e-4, (B, T, err[same].max().item())
    tally["frames"] += same.numel()
    tally["same"] += int(same.sum())
    assert tally["same"] >= 0.99 * tally["frames"] - 1, tally      # near-ties aside, the codes agree
    for b in range(B):                                            # every launch is the exact-fp32 kernel: rows are bit-exact
        i1, q1 = sc.quantize(x[b:b + 1])
        assert torch.equal(i1.cpu()[0], idx[b]) and torch.equal(q1.cpu()[0], q[b]), f"RepCodec B={B} T={T} row {b} differs from its solo call"


# ---------------------------------------------------------------------------------------------------------------- CAMPPlus
@pytest.fixture(scope="module")
def cam(device):
    from indextts_amd.campplus import CAMPPlus
    cfg = CamPPlusConfig()
    w = weights.synth_campplus_weights(cfg, tag="t/edges/campplus")
    return cfg, _tw(w), CAMPPlus(w, cfg, device=device)


def _cam_feat(tag, B, T):
    f = torch.from_numpy(synth.uniform(f"t/edges/campplus/{tag}", (B, T, 80), 2.0))
    return f - f.mean(dim=1, keepdim=True)


def _check_cam(cfg, tw, cp, feat, what):
    from oracle import campplus as ocp
    with torch.no_grad():
        want = ocp.forward(tw, cfg, feat)
    got = cp(feat).cpu()
    scale = max(1.0, want.abs().max().item())
    assert got.shape == want.shape == (feat.shape[0], 192)
    err = (got - want).abs().amax(-1)
    assert err.max().item() <= 5e-4 * scale, (what, err.tolist(), scale)
    return got


# T -> T2 = (T - 1) / 2 + 1 after the stride-2 TDNN layer; CAMLayer segments of 100 frames
CAM_CASES = [(1, 8), (1, 9), (2, 10), (1, 64), (1, 199), (2, 200), (1, 201), (3, 202), (1, 398), (2, 399), (1, 509), (1, 510), (1, 511)]


@pytest.mark.parametrize("B,T", CAM_CASES)
def test_campplus_edges(device, cam, B, T):
    cfg, tw, cp = cam
    feat = _cam_feat(f"{B}/{T}", B, T)
    got = _check_cam(cfg, tw, cp, feat, (B, T))
    for b in range(B if B > 1 else 0):                            # rows run one by one at the same T2: bit-exact in both modes
        assert torch.equal(cp(feat[b:b + 1]).cpu()[0], got[b]), f"CAMPPlus B={B} T={T} row {b} differs from its solo call"


def test_campplus_limits(device, cam):
    cfg, tw, cp = cam
    with pytest.raises(ValueError, match="at least 8 frames"):
        cp(torch.zeros(1, 7, 80))
    _check_cam(cfg, tw, cp, _cam_feat("after", 2, 8), "after the refused call")


# ---------------------------------------------------------------------------------------------------------------- conditioning
PE_LEN = 40               # a shortened positional-encoding table: T2 = pe_len is reachable at a small T


def _cond_model(cfg, tag, device, pe_len=None):
    from indextts_amd.cond import ConditioningEncoders
    w = weights.synth_gpt_cond_weights(cfg, tag=tag)
    if pe_len is not None:
        for p, m in (("conditioning_encoder", cfg.cond_module), ("emo_conditioning_encoder", cfg.emo_cond_module)):
            w[f"{p}.embed.pos_enc.pe"] = weights.conformer_pe(5000, m.output_size)[:, :pe_len].copy()
    return cfg, _tw(w), ConditioningEncoders(w, cfg, device=device)


@pytest.fixture(scope="module")
def cond_tiny(device):
    return _cond_model(GPTConfig.tiny(), "t/edges/cond/tiny", device, pe_len=PE_LEN)


@pytest.fixture(scope="module")
def cond_mid(device):
    cfg = dataclasses.replace(GPTConfig.tiny(), model_dim=256, cond_latents=8,
                              cond_module=CondModuleConfig(output_size=128, linear_units=256, attention_heads=2, num_blocks=2),
                              emo_cond_module=CondModuleConfig(output_size=128, linear_units=192, attention_heads=1, num_blocks=1))
    return _cond_model(cfg, "t/edges/cond/mid", device)


@pytest.fixture(scope="module")
def cond_full(device):
    return _cond_model(GPTConfig(), "t/edges/cond/full", device)


def _cond_rows(cfg, B, T2, n):
    """the row counts of the lin() launches of one encoder: conformer rows, the positional projection, the perceiver's key/value
    rows, its latent rows, the emotion vector"""
    return [B * T2, T2, B * (n + T2), B * n, B]


def _check_cond(model, x, lens, what, solo=True):
    from oracle import cond as oc
    cfg, tw, enc = model
    B, T, _ = x.shape
    lt = torch.tensor(lens)
    with torch.no_grad():
        ref_lat = oc.get_conditioning(tw, cfg, x, lt)
        ref_emo = oc.get_emovec(tw, cfg, x, lt)
    lat = enc.get_conditioning(x.transpose(1, 2), lt).cpu()
    ev = enc.get_emovec(x, lt).cpu()
    s_lat, s_emo = max(1.0, ref_lat.abs().max().item()), max(1.0, ref_emo.abs().max().item())
    assert (lat - ref_lat).abs().max().item() <= 1e-4 * s_lat, (what, (lat - ref_lat).abs().max().item(), s_lat)
    assert (ev - ref_emo).abs().max().item() <= 1e-4 * s_emo, (what, (ev - ref_emo).abs().max().item(), s_emo)
    if not solo or B == 1:
        return
    # the solo call keeps the row's padding: the reference masks the conv module's input BEFORE pointwise_conv1, whose bias then
    # reaches the k15 depthwise conv from the padded frames (GLU(bias), not zero), so a padded row does not equal its unpadded run
    T2 = (T - 3) // 2 + 1
    rows_l, rows_e = _cond_rows(cfg, B, T2, cfg.cond_latents), _cond_rows(cfg, B, T2, 1)
    same_l = _same_kernels(rows_l, _cond_rows(cfg, 1, T2, cfg.cond_latents))
    same_e = _same_kernels(rows_e, _cond_rows(cfg, 1, T2, 1))
    for b, l in enumerate(lens):
        s_l = enc.get_conditioning(x[b:b + 1].transpose(1, 2), lt[b:b + 1]).cpu()
        s_e = enc.get_emovec(x[b:b + 1], lt[b:b + 1]).cpu()
        _row_vs_solo(lat[b], s_l[0], same_l, 1e-4 * s_lat, f"conditioning lens={lens} T={T} row {b}")
        _row_vs_solo(ev[b], s_e[0], same_e, 1e-4 * s_emo, f"emovec lens={lens} T={T} row {b}")


def _cond_x(tag, B, T):
    return torch.from_numpy(synth.uniform(f"t/edges/cond/{tag}", (B, T, 1024), 1.0))     # padding left as noise: masked


# (T, lens): len2 = (len - 3) / 2 + 1 frames after Conv2dSubsampling2
COND_TINY_CASES = [(3, [3]), (4, [4]), (5, [5]), (5, [5, 3, 4]), (9, [9, 5, 3, 4]), (12, [1024, 7]), (11, [50, 11, 3]),
                   (2 * PE_LEN + 1, [2 * PE_LEN + 1, 40, 3]), (2 * PE_LEN + 2, [2 * PE_LEN + 2])]


@pytest.mark.parametrize("T,lens", COND_TINY_CASES)
def test_cond_tiny_edges(device, cond_tiny, T, lens):
    _check_cond(cond_tiny, _cond_x(f"tiny/{T}/{len(lens)}", len(lens), T), lens, ("tiny", T, lens))


# B * T2 = 254 / 256 / 258 rows; the solo calls stay below 256
@pytest.mark.parametrize("T,lens", [(255, [255, 200]), (257, [257, 5]), (259, [259, 130])])
def test_cond_mid_switch(device, cond_mid, T, lens):
    _check_cond(cond_mid, _cond_x(f"mid/{T}", len(lens), T), lens, ("mid", T, lens))


def test_cond_full_width(device, cond_full):
    """the real widths (512 / 2048 / 8 heads / 6 blocks, the emotion encoder 512 / 1024 / 4 heads / 4 blocks, 32 latents)"""
    _check_cond(cond_full, _cond_x("full", 3, 9), [9, 5, 3], ("full", 9))


def test_cond_full_width_many_rows(device, cond_full):
    """B * T2 = 520 rows against the solo calls' 260: the split-K embed GEMM's partition must not follow the batch's row count"""
    # bug found here: embed_ksplit() (cond.hip) sized the K split from B * T2, so a batch row was not bit-exact with its solo call
    _check_cond(cond_full, _cond_x("full/many", 2, 521), [521, 300], ("full", 521))


def test_cond_limits(device, cond_tiny):
    cfg, tw, enc = cond_tiny
    x = _cond_x("limits", 2, 6)
    with pytest.raises(RuntimeError, match="at least 3 frames"):
        enc.get_conditioning(x[:, :2].transpose(1, 2), torch.tensor([2, 2]))
    with pytest.raises(RuntimeError, match="at least 3 valid frames"):
        enc.get_emovec(x, torch.tensor([6, 2]))
    with pytest.raises(RuntimeError, match="longer than the positional-encoding table"):
        enc.get_conditioning(_cond_x("limits/pe", 1, 2 * PE_LEN + 3).transpose(1, 2), torch.tensor([2 * PE_LEN + 3]))
    _check_cond(cond_tiny, x, [6, 3], "after the refused calls")
