"""GPU: the acoustic stage on batches whose rows come from DIFFERENT prompts (speakers): S2Mel.cfm_rows (idxtts_s2mel_cfm_rows)
against the CPU oracle and against today's single-prompt entry on each row alone; IndexTTS2.acoustic_stage / synthesize_batch with
one PromptConditioning per row against per-request runs; ContinuousPipeline(acoustic_coalesce=4) and
BatchPipeline(acoustic_mix_prompts=True) against their unmerged results.

Contract: in the exact GEMM mode (GEMM_F32) kernel selection does not depend on the row count, and every row of
a mixed batch equals its own run bit for bit.  In the default split-bf16 mode a merge can move a GEMM across the 256-row threshold
(toy sizes do); there rows are held to the bounds of test_fullsize_gpu.py::test_config2_batch16_rows_equal_their_solo_runs (mel
L1 <= 1e-3, waveform max |d| <= 32767 * 2e-3)."""
import dataclasses
import threading
import warnings

import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import PipelineConfig, S2MelConfig

pytestmark = pytest.mark.gpu


def _halo(cfg):
    h, dil = 0, 1
    for _ in range(cfg.wn_layers):
        h += (cfg.wn_kernel - 1) // 2 * dil
        dil *= cfg.wn_dilation_rate
    return h


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = _lib.get_gemm_mode()
        _lib.set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        _lib.set_gemm_mode(self.old)


@pytest.fixture(scope="module")
def cfm_setup(device):
    from indextts_amd.s2mel import S2Mel
    cfg = dataclasses.replace(S2MelConfig.tiny(), hidden_dim=512, num_heads=8, depth=3, wn_hidden=512, wn_layers=2, block_size=2048)
    w = weights.synth_s2mel_weights(cfg, tag="t/mixed/s2mel")
    return cfg, w, S2Mel(w, cfg, device=device, max_frames=2048)


# prompts on both sides of the tail threshold (64 + WaveNet halo): the first case's batch evaluates its tail on every frame
# (shortest prompt 40), the second from 120 - halo on -- each row alone from its own prompt - halo
@pytest.mark.parametrize("plens,glens,oracle", [([300, 40, 150], [400, 250, 330], True), ([300, 120, 200], [400, 250, 330], False)])
def test_cfm_rows_vs_oracle_and_single_prompt_entry(device, cfm_setup, plens, glens, oracle):
    from oracle import s2mel as osm
    cfg, w, sm = cfm_setup
    assert max(plens) >= 64 + _halo(cfg)
    B, C = len(plens), cfg.in_channels
    T, Tg = max(p + g for p, g in zip(plens, glens)), max(glens)
    pcs = [torch.from_numpy(synth.uniform(f"t/mixed/pc{p}", (1, p, cfg.content_dim), 1.0)).to(device) for p in plens]
    rms = [torch.from_numpy(synth.uniform(f"t/mixed/rm{p}", (1, C, p), 1.0)).to(device) for p in plens]
    gen = torch.from_numpy(synth.uniform("t/mixed/gen", (B, Tg, cfg.content_dim), 1.0))
    for b in range(B):
        gen[b, glens[b]:] = 0
    gen = gen.to(device)
    style = torch.from_numpy(synth.uniform("t/mixed/style", (B, cfg.style_dim), 1.0)).to(device)
    z = torch.from_numpy(synth.uniform("t/mixed/z", (B, C, T), 1.7)).to(device)
    for mode in (_lib.GEMM_F32, _lib.GEMM_BF16X3):
        with _mode(mode):
            out = sm.cfm_rows(gen, glens, pcs, rms, style, 2, inference_cfg_rate=0.7, z=z)
            assert out.shape == (B, C, Tg)
            for b in range(B):
                Tp, Tb = plens[b], plens[b] + glens[b]
                assert (out[b, :, glens[b]:] == 0).all()
                mu = torch.cat([pcs[b], gen[b:b + 1, :glens[b]]], dim=1)
                solo = sm.cfm_inference(mu, [Tb], rms[b], style[b:b + 1], None, 2, inference_cfg_rate=0.7, z=z[b:b + 1, :, :Tb].contiguous())
                solo = solo[0, :, Tp:Tb]
                if mode == _lib.GEMM_F32:
                    assert torch.equal(out[b, :, :glens[b]], solo), (b, (out[b, :, :glens[b]] - solo).abs().max().item())
                else:
                    err = (out[b, :, :glens[b]] - solo).abs()
                    assert err.mean().item() <= 1e-4 and err.max().item() <= 3e-3, (b, err.mean().item(), err.max().item())
    if oracle:
        tw = {k: torch.from_numpy(v) for k, v in w.items()}
        torch.set_num_threads(16)
        for b in range(B):
            Tp, Tb = plens[b], plens[b] + glens[b]
            mu = torch.cat([pcs[b], gen[b:b + 1, :glens[b]]], dim=1).cpu()
            ref = osm.cfm_inference(tw, cfg, mu, torch.LongTensor([Tb]), rms[b].cpu(), style[b:b + 1].cpu(), z[b:b + 1, :, :Tb].cpu(), 2, 0.7)
            err = (out[b, :, :glens[b]].cpu() - ref[0, :, Tp:Tb]).abs()
            assert err.max().item() <= 3e-3 and err.mean().item() <= 1e-4, (b, err.max().item(), err.mean().item())


def test_cfm_rows_refuses_bad_shapes(device, cfm_setup):
    cfg, w, sm = cfm_setup
    pc = torch.zeros(1, 10, cfg.content_dim, device=device)
    rm = torch.zeros(1, cfg.in_channels, 10, device=device)
    gen = torch.zeros(2, 5, cfg.content_dim, device=device)
    st = torch.zeros(2, cfg.style_dim, device=device)
    with pytest.raises(ValueError):
        sm.cfm_rows(gen, [5, 5], [pc], [rm, rm], st, 2, z=torch.zeros(2, cfg.in_channels, 15, device=device))
    with pytest.raises(ValueError):      # noise shorter than the longest row
        sm.cfm_rows(gen, [5, 5], [pc, pc], [rm, rm], st, 2, z=torch.zeros(2, cfg.in_channels, 14, device=device))
    with pytest.raises(RuntimeError):    # a target length beyond gen_cond
        sm.cfm_rows(gen, [6, 5], [pc, pc], [rm, rm], st, 2, z=torch.zeros(2, cfg.in_channels, 16, device=device))


@pytest.fixture(scope="module")
def tiny(device):
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig.tiny()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="t/mixed/gpt")
    wg["mel_head.bias"] = wg["mel_head.bias"].copy()
    wg["mel_head.bias"][cfg.gpt.stop_mel_token] = -1e4        # every row runs to its cap
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="t/mixed/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="t/mixed/voc")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    # prompts of 90 (>= 64 + halo: a tail cut of its own), 12 and 40 frames
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=p, tag=f"t/mixed/prompt{p}").to(device) for p in (90, 12, 40)]
    return cfg, tts, conds


def _tg(cfg, n):
    """target frames of n codes, as prepare_condition computes them (infer_v2.py:844)"""
    return int((torch.tensor([n]) * cfg.code_to_frame).long()[0])


def _noise(cfg, tag, rows, frames, device):
    return torch.from_numpy(synth.uniform(tag, (rows, cfg.s2mel.in_channels, frames), 1.0)).to(device)


def test_acoustic_stage_three_speakers_equals_per_request_runs_tiny(device, tiny):
    cfg, tts, conds = tiny
    # 5 requests (1-2 rows) of 3 speakers, ragged code lengths
    reqs = []
    for k in range(5):
        B = 1 + k % 2
        text = torch.from_numpy(synth.integers(f"t/mixed/text{k}", (B, 10), 2, cfg.gpt.number_text_tokens))
        n = [9 + (7 * k + 3 * b) % 14 for b in range(B)]
        codes = torch.full((B, max(n)), cfg.gpt.stop_mel_token, dtype=torch.long)
        for b in range(B):
            codes[b, :n[b]] = torch.from_numpy(synth.integers(f"t/mixed/codes{k}/{b}", (n[b],), 0, cfg.s2mel.codebook_size))
        c = conds[k % 3]
        frames = c.prompt_condition.shape[1] + _tg(cfg, max(n))
        reqs.append({"text": text, "codes": codes, "cond": c, "noise": _noise(cfg, f"t/mixed/noise{k}", B, frames, device)})
    from indextts_amd.serving import merge_acoustic_states
    for mode in (_lib.GEMM_F32, _lib.GEMM_BF16X3):
        with _mode(mode), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sts = [tts.gpt_stage(r["text"], r["cond"], codes=r["codes"]) for r in reqs]
            solo = [tts.acoustic_stage(st, noise=r["noise"], return_intermediates=True) for st, r in zip(sts, reqs)]
            st, noise = merge_acoustic_states([(r["cond"], s, r["noise"]) for r, s in zip(reqs, sts)])
            assert isinstance(st["cond"], list) and len(st["cond"]) == st["B"] == 7
            wavs, mid = tts.acoustic_stage(st, noise=noise, return_intermediates=True)
        a = 0
        for (w1, m1), r in zip(solo, reqs):
            for b in range(r["text"].shape[0]):
                tl = m1["target_lens"][b]
                assert mid["target_lens"][a] == tl
                if mode == _lib.GEMM_F32:
                    assert torch.equal(mid["mel"][a, :, :tl], m1["mel"][b, :, :tl]), (a, b)
                    assert torch.equal(wavs[a], w1[b]), (a, b)
                else:
                    assert (mid["mel"][a, :, :tl] - m1["mel"][b, :, :tl]).abs().mean().item() <= 1e-3
                    assert (wavs[a] - w1[b]).abs().max().item() <= 32767 * 2e-3
                a += 1


def test_synthesize_batch_with_a_prompt_per_row_equals_solo_calls_tiny(device, tiny):
    cfg, tts, conds = tiny
    B, M = 5, 14
    text = torch.from_numpy(synth.integers("t/mixed/sbtext", (B, 10), 2, cfg.gpt.number_text_tokens))
    rows = [conds[0], conds[1], conds[2], conds[1], conds[0]]
    T = max(c.prompt_condition.shape[1] for c in rows) + _tg(cfg, M)
    noise = _noise(cfg, "t/mixed/sbnoise", B, T, device)
    with _mode(_lib.GEMM_F32), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wavs, mid = tts.synthesize_batch(text, rows, max_mel_tokens=M, noise=noise, return_intermediates=True)
        for b in range(B):
            Tb = rows[b].prompt_condition.shape[1] + _tg(cfg, M)
            w1, m1 = tts.synthesize_batch(text[b:b + 1], rows[b], max_mel_tokens=M, noise=noise[b:b + 1, :, :Tb].contiguous(),
                                          return_intermediates=True)
            assert torch.equal(m1["codes"][0], mid["codes"][b]), b
            assert torch.equal(w1[0], wavs[b]), (b, (w1[0] - wavs[b]).abs().max().item())
        # one list entry per row, all the same object: the single-prompt path, same result as passing the object
        w_same = tts.synthesize_batch(text[:2], [conds[2], conds[2]], max_mel_tokens=M, noise=noise[:2, :, :40 + _tg(cfg, M)].contiguous())
        w_one = tts.synthesize_batch(text[:2], conds[2], max_mel_tokens=M, noise=noise[:2, :, :40 + _tg(cfg, M)].contiguous())
    for a, b in zip(w_same, w_one):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        tts.gpt_stage(text, rows[:3], max_mel_tokens=M)


def test_continuous_pipeline_acoustic_coalesce_equals_unmerged(device, tiny):
    from indextts_amd.serving import ContinuousPipeline
    cfg, tts, conds = tiny
    cap = 12
    reqs = []
    for k in range(6):
        B = 1 + k % 2
        text = torch.from_numpy(synth.integers(f"t/mixed/ctext{k}", (B, 8 + k), 2, cfg.gpt.number_text_tokens))
        c = conds[k % 3]
        frames = c.prompt_condition.shape[1] + _tg(cfg, cap)
        reqs.append((text, c, _noise(cfg, f"t/mixed/cnoise{k}", B, frames, device)))

    def run(coalesce):
        gate = threading.Event()

        def factory(mp, mn):      # the lane starts once every request is waiting: one admission, one poll finishes them all
            gate.wait(60)
            return tts.gpt.decode_session(16, mp, mn, repetition_penalty=10.0)
        with ContinuousPipeline(tts, slots=16, poll_steps=cap, max_new=40, session_factory=factory, acoustic_coalesce=coalesce) as pipe:
            pipe.trace = []
            futs = [pipe.submit(t, c, max_mel_tokens=cap, noise=z) for t, c, z in reqs]
            gate.set()
            got = [f.result(timeout=600) for f in futs]
            return got, list(pipe.trace)
    with _mode(_lib.GEMM_F32), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, tr1 = run(1)
        got, tr4 = run(4)
    assert all(len(t[4]) == 1 for t in tr1)
    assert sorted(k for t in tr4 for k in t[4]) == list(range(len(reqs)))
    merged = [t[4] for t in tr4 if len({id(reqs[k][1]) for k in t[4]}) >= 2]
    assert merged, tr4
    assert max(len(t[4]) for t in tr4) == 4 and all(t[3] <= 16 for t in tr4)
    for k in range(len(reqs)):
        assert len(got[k]) == len(want[k])
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k


def test_batch_pipeline_mixed_prompts_equals_sequential(device, tiny):
    from indextts_amd.serving import BatchPipeline
    cfg, tts, conds = tiny
    M = 10
    reqs = []
    for k in range(6):
        B = 1 + k % 2
        text = torch.from_numpy(synth.integers(f"t/mixed/btext{k}", (B, 9), 2, cfg.gpt.number_text_tokens))
        c = conds[k % 3]
        reqs.append((text, c, _noise(cfg, f"t/mixed/bnoise{k}", B, c.prompt_condition.shape[1] + _tg(cfg, M), device)))
    with _mode(_lib.GEMM_F32), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [tts.synthesize_batch(t, c, max_mel_tokens=M, noise=z) for t, c, z in reqs]
        torch.cuda.synchronize()
        with BatchPipeline(tts, decode_lanes=2, acoustic_coalesce=3, acoustic_mix_prompts=True) as pipe:
            pipe.trace = []
            futs = [pipe.submit(t, c, max_mel_tokens=M, noise=z) for t, c, z in reqs]
            got = [f.result(timeout=600) for f in futs]
    for k in range(len(reqs)):
        assert len(got[k]) == len(want[k])
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k


def test_fullsize_three_speakers_equal_their_solo_runs(device):
    """Full-size weights, prompts of 400 / 689 / 1000 frames, 300 / 220 / 260 codes, default (split-bf16) mode: every row of the
    mixed batch within the solo bounds of its own request (mel L1 <= 1e-3, waveform max |d| <= 32767 * 2e-3).  The requests of
    >= 256 codes cross no row-count threshold by the merge and come out bit for bit (their CFM tail's conv2 moves to the 256-row-tile
    kernel at >= 4096 rows, which changes no result); the 220-code request does cross one: alone, prepare_condition's gpt_layer and
    content_in_proj GEMMs run its 220 code rows on the exact fp32 kernel (< 256 rows), merged on split-bf16."""
    from indextts_amd.infer_v2 import IndexTTS2, PromptConditioning
    cfg = PipelineConfig()
    wg = weights.synth_gpt_weights(cfg.gpt, tag="bench/gpt")
    ws = weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel")
    wv = weights.synth_bigvgan_weights(cfg.bigvgan, tag="bench/bigvgan")
    tts = IndexTTS2.from_state_dicts(cfg, wg, ws, wv, device=device)
    plens, ncodes = [400, 689, 1000], [300, 220, 260]
    conds = [PromptConditioning.synthetic(cfg, prompt_frames=p, tag=f"t/mixed/full/prompt{p}").to(device) for p in plens]
    texts = [torch.from_numpy(synth.integers(f"t/mixed/full/text{k}", (1, 48 + 16 * k), 2, cfg.gpt.number_text_tokens)) for k in range(3)]
    codes = [torch.from_numpy(synth.integers(f"t/mixed/full/codes{k}", (1, n), 0, cfg.s2mel.codebook_size)) for k, n in enumerate(ncodes)]
    noises = [_noise(cfg, f"t/mixed/full/noise{k}", 1, p + _tg(cfg, n), device) for k, (p, n) in enumerate(zip(plens, ncodes))]
    from indextts_amd.serving import merge_acoustic_states
    assert _lib.get_gemm_mode() == _lib.GEMM_BF16X3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sts = [tts.gpt_stage(t, c, codes=x) for t, c, x in zip(texts, conds, codes)]
        solo = [tts.acoustic_stage(st, noise=z, return_intermediates=True) for st, z in zip(sts, noises)]
        st, noise = merge_acoustic_states([(c, s, z) for c, s, z in zip(conds, sts, noises)])
        wavs, mid = tts.acoustic_stage(st, noise=noise, return_intermediates=True)
    res = []
    for b, (w1, m1) in enumerate(solo):
        tl = m1["target_lens"][0]
        assert wavs[b].shape == w1[0].shape and torch.isfinite(wavs[b]).all()
        res.append((b, (mid["mel"][b, :, :tl] - m1["mel"][0, :, :tl]).abs().mean().item(), (wavs[b] - w1[0]).abs().max().item(),
                    torch.equal(mid["mel"][b, :, :tl], m1["mel"][0, :, :tl]), torch.equal(wavs[b], w1[0])))
    print("full-size mixed vs solo (row, mel L1, wav max|d|, mel equal, wav equal):", res)
    assert all(l1 <= 1e-3 and dw <= 32767 * 2e-3 for _, l1, dw, _, _ in res), res
    assert all(me and we for b, _, _, me, we in res if ncodes[b] >= 256), res
