"""GPU: per-row Euler schedules and guidance rates in one CFM batch (idxtts_s2mel_cfm_sched through S2Mel.cfm_rows / cfm_inference).

Every row has its own step count and inference_cfg_rate; rows leave the batch when their schedule ends, and the null half runs on the
rows with a rate > 0 only.  Oracle comparisons run `oracle.s2mel.cfm_inference` row by row with that row's steps and rate, at <= 3 steps,
under the 2e-4 max-abs bound of tests/test_s2mel_gpu.py (test_cfm_vs_reference_golden at 3 steps, test_cfm_ragged_batch_vs_oracle at 2);
the rate-0 branch does fewer operations than the branch that bound was set for.  In the exact GEMM mode kernel selection does not depend
on the row count, so rows equal their solo runs bit for bit."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import S2MelConfig

pytestmark = pytest.mark.gpu

ORACLE_BOUND = 2e-4


class _mode:
    def __init__(self, mode, acoustic_bf16=False):
        self.mode, self.ab = mode, acoustic_bf16

    def __enter__(self):
        self.old, self.old_ab = _lib.get_gemm_mode(), _lib.get_acoustic_bf16()
        _lib.set_gemm_mode(self.mode)
        _lib.set_acoustic_bf16(self.ab)

    def __exit__(self, *exc):
        _lib.set_gemm_mode(self.old)
        _lib.set_acoustic_bf16(self.old_ab)


def _halo(cfg):
    h, dil = 0, 1
    for _ in range(cfg.wn_layers):
        h += (cfg.wn_kernel - 1) // 2 * dil
        dil *= cfg.wn_dilation_rate
    return h


@pytest.fixture(scope="module")
def tiny(device):
    """the synthetic model of tests/test_s2mel_gpu.py::_tiny"""
    from indextts_amd.s2mel import S2Mel
    cfg = S2MelConfig.tiny()
    w = weights.synth_s2mel_weights(cfg, tag="golden/s2mel")
    return cfg, {k: torch.from_numpy(v) for k, v in w.items()}, S2Mel(w, cfg, device=device)


class _Batch:
    """Rows with their own prompts: row b's tensors depend on the row's tag alone, so a permuted batch holds the same rows."""

    def __init__(self, cfg, device, plens, glens, tag="t/cfm_sched"):
        self.cfg, self.plens, self.glens = cfg, list(plens), list(glens)
        B, C = len(plens), cfg.in_channels
        self.lens = [p + g for p, g in zip(plens, glens)]
        self.pcs = [torch.from_numpy(synth.uniform(f"{tag}/pc{b}", (1, plens[b], cfg.content_dim), 1.0)).to(device) for b in range(B)]
        self.rms = [torch.from_numpy(synth.uniform(f"{tag}/rm{b}", (1, C, plens[b]), 1.0)).to(device) for b in range(B)]
        self.gens = [torch.from_numpy(synth.uniform(f"{tag}/gen{b}", (glens[b], cfg.content_dim), 1.0)).to(device) for b in range(B)]
        self.style = torch.from_numpy(synth.uniform(f"{tag}/style", (B, cfg.style_dim), 1.0)).to(device)
        self.zs = [torch.from_numpy(synth.uniform(f"{tag}/z{b}", (C, self.lens[b]), 1.7)).to(device) for b in range(B)]

    def args(self, rows):
        """(gen_cond, target_lens, prompt_conditions, ref_mels, style, z) of the batch made of `rows`, in that order"""
        cfg = self.cfg
        Tg, T = max(self.glens[b] for b in rows), max(self.lens[b] for b in rows)
        gen = torch.zeros(len(rows), Tg, cfg.content_dim, device=self.style.device)
        z = torch.zeros(len(rows), cfg.in_channels, T, device=self.style.device)
        for i, b in enumerate(rows):
            gen[i, :self.glens[b]] = self.gens[b]
            z[i, :, :self.lens[b]] = self.zs[b]
        return (gen, [self.glens[b] for b in rows], [self.pcs[b] for b in rows], [self.rms[b] for b in rows],
                self.style[list(rows)].contiguous(), z)

    def run(self, sm, rows, steps, rates):
        gen, tl, pcs, rms, style, z = self.args(rows)
        return sm.cfm_rows(gen, tl, pcs, rms, style, steps, inference_cfg_rate=rates, z=z)

    def oracle(self, tw, b, steps, rate):
        from oracle import s2mel as osm
        L, P = self.lens[b], self.plens[b]
        mu = torch.cat([self.pcs[b][0], self.gens[b]], dim=0)[None].cpu()
        ref = osm.cfm_inference(tw, self.cfg, mu, torch.LongTensor([L]), self.rms[b].cpu(), self.style[b:b + 1].cpu(), self.zs[b][None].cpu(),
                                steps, rate)
        return ref[0, :, P:L]


MIX_P, MIX_L = [10, 7, 12, 9], [41, 29, 36, 33]
MIX_STEPS, MIX_RATES = [3, 1, 2, 3], [0.7, 0.7, 0.0, 1.5]


@pytest.fixture(scope="module")
def mixed(tiny, device):
    cfg, tw, sm = tiny
    bt = _Batch(cfg, device, MIX_P, [l - p for l, p in zip(MIX_L, MIX_P)])
    with _mode(_lib.GEMM_F32):
        out = bt.run(sm, [0, 1, 2, 3], MIX_STEPS, MIX_RATES)
    return bt, out


def test_mixed_batch_vs_oracle_and_solo_runs(tiny, mixed):
    cfg, tw, sm = tiny
    bt, out = mixed
    assert out.shape == (4, cfg.in_channels, max(bt.glens))
    with _mode(_lib.GEMM_F32):
        for b in range(4):
            g = bt.glens[b]
            err = (out[b, :, :g].cpu() - bt.oracle(tw, b, MIX_STEPS[b], MIX_RATES[b])).abs().max().item()
            print(f"row {b}: steps {MIX_STEPS[b]} rate {MIX_RATES[b]} max |d| vs oracle {err:.3e}")
            assert err <= ORACLE_BOUND, (b, err)
            assert (out[b, :, g:] == 0).all()
            # a row with guidance: the solver of one schedule (idxtts_s2mel_cfm_rows) on that row alone, its steps and rate as scalars;
            # the rate-0 row: this entry on that row alone
            solo = bt.run(sm, [b], MIX_STEPS[b], MIX_RATES[b])
            assert torch.equal(out[b, :, :g], solo[0, :, :g]), (b, (out[b, :, :g] - solo[0, :, :g]).abs().max().item())


def test_mixed_batch_through_cfm_inference_has_zero_prompt_frames(tiny, mixed, device):
    """The padded single-tensor interface with per-row values: the same rows, prompt frames (and the padding) exactly 0."""
    cfg, tw, sm = tiny
    bt, out = mixed
    B, T, Tp = 4, max(bt.lens), max(bt.plens)
    mu = torch.zeros(B, T, cfg.content_dim, device=device)
    prompt = torch.zeros(B, cfg.in_channels, Tp, device=device)
    z = torch.zeros(B, cfg.in_channels, T, device=device)
    for b in range(B):
        mu[b, :bt.lens[b]] = torch.cat([bt.pcs[b][0], bt.gens[b]], dim=0)
        prompt[b, :, :bt.plens[b]] = bt.rms[b][0]
        z[b, :, :bt.lens[b]] = bt.zs[b]
    with _mode(_lib.GEMM_F32):
        mel = sm.cfm_inference(mu, torch.LongTensor(bt.lens), prompt, bt.style, None, MIX_STEPS, inference_cfg_rate=MIX_RATES, z=z,
                               prompt_lens=torch.LongTensor(bt.plens))
    for b in range(B):
        P, L = bt.plens[b], bt.lens[b]
        assert (mel[b, :, :P] == 0).all() and (mel[b, :, L:] == 0).all()
        assert torch.equal(mel[b, :, P:L], out[b, :, :L - P]), b


@pytest.mark.parametrize("perm", [[2, 1, 3, 0], [1, 3, 0, 2], [3, 2, 1, 0]])
def test_permuting_rows_permutes_outputs(tiny, mixed, perm):
    """[2, 1, 3, 0]: the rate-0 row first and a row with the most steps last."""
    cfg, tw, sm = tiny
    bt, out = mixed
    with _mode(_lib.GEMM_F32):
        got = bt.run(sm, perm, [MIX_STEPS[b] for b in perm], [MIX_RATES[b] for b in perm])
    for i, b in enumerate(perm):
        g = bt.glens[b]
        assert torch.equal(got[i, :, :g], out[b, :, :g]), (i, b)
        assert (got[i, :, g:] == 0).all()


def test_uniform_call_equals_one_schedule_entry_exact_mode(tiny, mixed):
    cfg, tw, sm = tiny
    bt, _ = mixed
    with _mode(_lib.GEMM_F32):
        old = bt.run(sm, [0, 1, 2, 3], 2, 0.7)
        new = bt.run(sm, [0, 1, 2, 3], [2, 2, 2, 2], [0.7] * 4)
    assert torch.equal(old, new), (old - new).abs().max().item()


def test_all_rows_without_guidance_vs_oracle(tiny, device):
    cfg, tw, sm = tiny
    bt = _Batch(cfg, device, [10, 7], [31, 22], tag="t/cfm_sched/c0")
    steps = [2, 3]
    with _mode(_lib.GEMM_F32):
        out = bt.run(sm, [0, 1], steps, [0.0, 0.0])
        scalar = bt.run(sm, [0, 1], 2, 0.0)          # a scalar rate of 0 takes the same entry
        row0 = bt.run(sm, [0], 2, 0.0)
    for b in range(2):
        g = bt.glens[b]
        err = (out[b, :, :g].cpu() - bt.oracle(tw, b, steps[b], 0.0)).abs().max().item()
        print(f"row {b}: steps {steps[b]} rate 0 max |d| vs oracle {err:.3e}")
        assert err <= ORACLE_BOUND, (b, err)
    assert torch.equal(scalar[0, :, :bt.glens[0]], out[0, :, :bt.glens[0]])
    assert torch.equal(row0[0, :, :bt.glens[0]], out[0, :, :bt.glens[0]])


def test_cfm_inference_accepts_rate_zero(tiny, device):
    """S2Mel.cfm_inference(inference_cfg_rate=0.0), refused before: the reference's else-branch (flow_matching.py:105-106)."""
    from oracle import s2mel as osm
    cfg, tw, sm = tiny
    Tp, T = 11, 34
    z = torch.from_numpy(synth.uniform("golden/s2mel/cfm/z", (1, cfg.in_channels, T), 1.7))
    mu = torch.from_numpy(synth.uniform("golden/s2mel/cfm/mu", (1, T, cfg.content_dim), 1.0))
    prompt = torch.from_numpy(synth.uniform("golden/s2mel/cfm/prompt", (1, cfg.in_channels, Tp), 1.0))
    st = torch.from_numpy(synth.uniform("golden/s2mel/cfm/style", (1, cfg.style_dim), 1.0))
    with _mode(_lib.GEMM_F32):
        out = sm.cfm_inference(mu, torch.LongTensor([T]), prompt, st, None, 3, inference_cfg_rate=0.0, z=z).cpu()
    ref = osm.cfm_inference(tw, cfg, mu, torch.LongTensor([T]), prompt, st, z, 3, 0.0)
    err = (out - ref).abs().max().item()
    print(f"cfm_inference rate 0, 3 steps: max |d| vs oracle {err:.3e}")
    assert err <= ORACLE_BOUND, err
    assert (out[..., :Tp] == 0).all()


def test_tail_compaction_rows_equal_their_solo_runs(tiny, device):
    """Prompts of at least 64 + halo frames: the post-transformer part runs from the SHORTEST prompt minus the halo on (tail_t0 > 0), each
    row alone from its own."""
    cfg, tw, sm = tiny
    base = 64 + _halo(cfg)
    bt = _Batch(cfg, device, [base + 9, base + 2], [20, 26], tag="t/cfm_sched/tail")
    steps = [2, 1]
    with _mode(_lib.GEMM_F32):
        out = bt.run(sm, [0, 1], steps, [0.7, 0.0])
        for b in range(2):
            g = bt.glens[b]
            solo = bt.run(sm, [b], steps[b], [0.7, 0.0][b])
            assert torch.equal(out[b, :, :g], solo[0, :, :g]), (b, (out[b, :, :g] - solo[0, :, :g]).abs().max().item())
        uni = bt.run(sm, [0, 1], [2, 2], [0.7, 0.7])
        assert torch.equal(uni, bt.run(sm, [0, 1], 2, 0.7))


# ---- the default split-bf16 mode ----
def test_split_bf16_row_count_crosses_256_when_a_row_leaves(tiny, device):
    """Each CFG half is an evaluation of its own on its live rows: 3 rows of 96 frames are 288 rows per half (the LDS-DMA split-bf16
    kernels), and 192 (the exact kernels) once the one-step row has left.  Bound: test_cfm_split_bf16_mode_vs_oracle's."""
    cfg, tw, sm = tiny
    bt = _Batch(cfg, device, [10, 12, 9], [86, 84, 87], tag="t/cfm_sched/b16")
    assert all(l == 96 for l in bt.lens)
    steps, rates = [2, 1, 2], [0.7, 0.7, 1.5]
    with _mode(_lib.GEMM_BF16X3):
        out = bt.run(sm, [0, 1, 2], steps, rates)
    for b in range(3):
        err = (out[b, :, :bt.glens[b]].cpu() - bt.oracle(tw, b, steps[b], rates[b])).abs()
        print(f"row {b}: mean {err.mean().item():.3e} max {err.max().item():.3e}")
        assert err.mean().item() <= 1e-4 and err.max().item() <= 3e-3, (b, err.mean().item(), err.max().item())


@pytest.mark.parametrize("acoustic_bf16", [False, True])
def test_uniform_call_equals_one_schedule_entry_split_bf16(tiny, device, acoustic_bf16):
    """288 rows per half here, 576 stacked in the one-schedule entry: both run every GEMM on the kernels the row count >= 256 selects, so
    the per-sequence-bias instantiation must add what the shared-bias one adds, in the order it adds it."""
    cfg, tw, sm = tiny
    bt = _Batch(cfg, device, [10, 12, 9], [86, 84, 87], tag="t/cfm_sched/b16")
    with _mode(_lib.GEMM_BF16X3, acoustic_bf16):
        old = bt.run(sm, [0, 1, 2], 2, 0.7)
        new = bt.run(sm, [0, 1, 2], [2, 2, 2], [0.7, 0.7, 0.7])
    assert torch.isfinite(new).all()
    assert torch.equal(old, new), (old - new).abs().max().item()


# ---- refusals of the C entry ----
def test_c_entry_refuses_bad_arguments(tiny, device):
    cfg, tw, sm = tiny
    lib = _lib.load()
    bt = _Batch(cfg, device, [10, 7], [31, 22], tag="t/cfm_sched/c0")
    gen, tl, pcs, rms, style, z = bt.args([0, 1])
    B, Tg, T = 2, gen.shape[1], z.shape[-1]
    from indextts_amd.s2mel import cfm_schedule_tables
    sched, t_emb, dt, row_sched = cfm_schedule_tables([2, 1])
    t_emb = t_emb.to(device)
    dt = np.ascontiguousarray(dt.numpy(), dtype=np.float32)
    pcs = [p.contiguous() for p in pcs]
    rms = [r.contiguous() for r in rms]
    need = int(lib.idxtts_s2mel_cfm_sched_workspace_bytes(sm._h, B, T, max(bt.plens), len(sched), sched.ctypes.data_as(c_void_p)))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    out = torch.full((B, cfg.in_channels, Tg), 7.0, device=device)
    good = dict(gen=_lib.ptr(gen), tl=np.array(tl, np.int32), pc=[p.data_ptr() for p in pcs], rm=[r.data_ptr() for r in rms],
                pl=np.array(bt.plens, np.int32), style=_lib.ptr(style), z=_lib.ptr(z), n_sched=len(sched), sched=sched, t_emb=_lib.ptr(t_emb),
                dt=dt, row_sched=row_sched, rates=np.array([0.7, 0.0], np.float32), out=_lib.ptr(out), T=T, ws=_lib.ptr(ws), ws_bytes=need)

    def call(**over):
        a = dict(good, **over)
        arr = lambda v: v.ctypes.data_as(c_void_p) if v is not None else c_void_p(0)
        pc_tab = (c_void_p * B)(*a["pc"])
        rm_tab = (c_void_p * B)(*a["rm"])
        rc = lib.idxtts_s2mel_cfm_sched(sm._h, a["gen"], arr(a["tl"]), Tg, pc_tab, rm_tab, arr(a["pl"]), a["style"], a["z"], a["n_sched"],
                                        arr(a["sched"]), a["t_emb"], arr(a["dt"]), arr(a["row_sched"]), arr(a["rates"]), a["out"], B, a["T"],
                                        a["ws"], a["ws_bytes"], _lib.current_stream())
        torch.cuda.synchronize()
        return rc, (lib.idxtts_last_error() or b"").decode("utf-8", "replace")

    i32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float32))
    bad = {
        "null gen_cond": dict(gen=c_void_p(0)), "null style": dict(style=c_void_p(0)), "null z": dict(z=c_void_p(0)),
        "null t_emb": dict(t_emb=c_void_p(0)), "null out-of-table": dict(pc=[0, pcs[1].data_ptr()]), "null sched_steps": dict(sched=None),
        "null dt": dict(dt=None), "null row_sched": dict(row_sched=None), "null cfg_rates": dict(rates=None),
        "n_sched 0": dict(n_sched=0), "a schedule of 0 steps": dict(sched=i32(2, 0)),
        "row_sched beyond n_sched": dict(row_sched=i32(0, 2)), "row_sched negative": dict(row_sched=i32(-1, 1)),
        "negative rate": dict(rates=f32(0.7, -0.1)), "NaN rate": dict(rates=f32(float("nan"), 0.0)), "infinite rate": dict(rates=f32(0.7, float("inf"))),
        "target length beyond gen_cond (as cfm_rows)": dict(tl=i32(Tg + 1, tl[1])), "prompt length 0 (as cfm_rows)": dict(pl=i32(0, bt.plens[1])),
        "T not the longest row (as cfm_rows)": dict(T=T + 1), "workspace too small": dict(ws_bytes=need - 256), "null workspace": dict(ws=c_void_p(0)),
    }
    for name, over in bad.items():
        rc, msg = call(**over)
        assert rc != 0 and msg, name
        assert (out == 7.0).all(), name
    assert "cfg_rates" in call(rates=f32(0.7, -0.1))[1] and "row_sched" in call(row_sched=i32(0, 2))[1]
    assert "step" in call(sched=i32(2, 0))[1] and "n_sched" in call(n_sched=0)[1] and "workspace" in call(ws_bytes=need - 256)[1]
    rc, msg = call()
    assert rc == 0, msg
    want = bt.run(sm, [0, 1], [2, 1], [0.7, 0.0])
    assert torch.equal(out, want)
