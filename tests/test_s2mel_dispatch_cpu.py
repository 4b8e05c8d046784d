"""CPU: what tests/test_s2mel_dispatch_gpu.py rests on (cases and helpers: tests/s2mel_dispatch_cases.py).

  * the case table lands where it says (M, t0, Mt against the solver's own rules restated in s2mel_dispatch_cases.py);
  * the bounds separate: the solver's tail compaction, restated from the oracle's own pieces, reproduces the unmodified oracle at
    t0 = pmin - halo and misses it by more than 3 x the exact-fp32 max bound (3e-4) one frame later -- the slip an off-by-one in
    halo, lens2t or v_t0 would make.  Measured with these inputs, max |d| of the slip over the bound: solver cases 5-12
    12.9, 8.1, 3.7, 10.6, 7.6, 6.7, 3.9, 5.4; cfm_rows cases 8.0, 5.3 (3.7 means 1.10e-3: inside the split-bf16 bound of 3e-3,
    which is why every case also runs in exact-fp32 mode).  If other input data ever made a slip invisible, the case changes, not
    the bound;
  * the float64 oracle runs, agrees with the fp32 oracle, and the fp32 oracle still gives the golden file's values."""
import os

import numpy as np
import pytest
import torch

import s2mel_dispatch_cases as dc
from indextts_amd import synth, weights
from oracle import s2mel as osm

F32_MAX_BOUND = dc.SOLVER_BOUNDS["f32"][0]


@pytest.fixture(scope="module")
def model():
    cfg = dc.config()
    _, tw, tw64 = dc.synth_weights(cfg)
    return cfg, tw, tw64


def test_case_table_geometry(model):
    cfg = model[0]
    assert dc.halo(cfg) == 6
    for num, lens, plens in dc.SOLVER_CASES:
        assert dc.geometry(cfg, lens, plens) == dc.SOLVER_GEOMETRY[num], num
    for num, plens, glens in dc.ROWS_CASES:
        assert dc.geometry(cfg, [p + g for p, g in zip(plens, glens)], plens) == dc.ROWS_GEOMETRY[num], num
    planes = lambda rows: rows >= 256
    for num, (M, t0, Mt) in dc.SOLVER_GEOMETRY.items():
        assert (num in dc.MIXED_NEIGHBOUR) == (t0 > 0 and planes(M) and not planes(Mt)), num
    for mixed, nb in dc.MIXED_NEIGHBOUR.items():
        M, t0, Mt = dc.SOLVER_GEOMETRY[nb]
        assert t0 > 0 and planes(M) and planes(Mt), nb
    # two streams: each half is a dit_eval of its own on half the rows
    same_side = {n: planes(M) == planes(M // 2) and planes(Mt) == planes(Mt // 2) for n, (M, t0, Mt) in dc.SOLVER_GEOMETRY.items()}
    assert [same_side[n] for n in dc.TWO_STREAM_CASES] == [False, False, True, True]


def _tail_rows():
    out = [(f"solver{num}", lens, plens, lambda cfg, num=num, lens=lens, plens=plens: dc.solver_inputs(cfg, num, lens, plens))
           for num, lens, plens in dc.SOLVER_CASES if dc.SOLVER_GEOMETRY[num][1] > 0]
    for num, plens, glens in dc.ROWS_CASES:
        lens = [p + g for p, g in zip(plens, glens)]

        def build(cfg, num=num, plens=plens, glens=glens, lens=lens):      # the batch cfm_rows packs for cfm_solve
            gen, pcs, rms, style, z = dc.rows_inputs(cfg, num, plens, glens)
            B, T = len(lens), max(lens)
            mu = torch.zeros(B, T, cfg.content_dim)
            prompt = torch.zeros(B, cfg.in_channels, max(plens))
            for b in range(B):
                mu[b, :lens[b]] = torch.cat([pcs[b][0], gen[b, :glens[b]]], 0)
                prompt[b, :, :plens[b]] = rms[b][0]
            return z, mu, prompt, style
        out.append((f"rows{num}", lens, plens, build))
    return out


@pytest.mark.parametrize("name,lens,plens,build", _tail_rows(), ids=[r[0] for r in _tail_rows()])
def test_tail_cut_is_exact_and_one_frame_later_is_caught(model, name, lens, plens, build):
    cfg, tw, _ = model
    inputs = build(cfg)
    z, mu, prompt, style = inputs
    t0 = dc.tail_t0(cfg, plens)
    assert t0 == min(plens) - dc.halo(cfg) >= 64
    want = dc.solver_oracle_rows(tw, cfg, lens, plens, inputs)
    exact = slip = 0.0
    for b, (Lb, Pb) in enumerate(zip(lens, plens)):
        row = (mu[b:b + 1, :Lb], Lb, prompt[b:b + 1, :, :Pb], style[b:b + 1], z[b:b + 1, :, :Lb])
        exact = max(exact, (dc.cfm_tail_cut(tw, cfg, *row, t0)[0] - want[b]).abs().max().item())
        slip = max(slip, (dc.cfm_tail_cut(tw, cfg, *row, t0 + 1)[0] - want[b]).abs().max().item())
    print(f"{name}: t0 = {t0}: max|d| {exact:.2e}; t0 + 1: {slip:.2e} = {slip / F32_MAX_BOUND:.1f} x the fp32 bound")
    assert exact <= 1e-5, exact
    assert slip > 3 * F32_MAX_BOUND, slip


def test_float64_oracle_runs_and_agrees_with_fp32(model):
    cfg, tw, tw64 = model
    num, lens, plens = dc.SOLVER_CASES[10]          # ragged, three rows
    inputs = dc.solver_inputs(cfg, num, lens, plens)
    r32 = dc.solver_oracle_rows(tw, cfg, lens, plens, inputs)
    r64 = dc.solver_oracle_rows(tw64, cfg, lens, plens, inputs, torch.float64)
    for b, (a, d) in enumerate(zip(r32, r64)):
        assert a.dtype == torch.float32 and d.dtype == torch.float64 and d.shape == (cfg.in_channels, lens[b])
        assert torch.isfinite(d).all() and (d[:, :plens[b]] == 0).all()
        assert (a.double() - d).abs().max().item() <= 1e-4, b
    e32 = dc.estimator_oracle_rows(tw, cfg, dc.estimator_inputs(cfg, 127))
    e64 = dc.estimator_oracle_rows(tw64, cfg, dc.estimator_inputs(cfg, 127), torch.float64)
    for a, d in zip(e32, e64):
        assert d.dtype == torch.float64 and (a.double() - d).abs().max().item() <= 1e-4
    # the tables it creates follow the dtype asked for, and fp32 is what it was
    assert osm.rope_cache(16, 64, dtype=torch.float64).dtype == torch.float64
    assert osm.rope_cache(16, 64).dtype == torch.float32
    assert (osm.rope_cache(16, 64) - osm.rope_cache(16, 64, dtype=torch.float64)).abs().max().item() <= 1e-6
    t = torch.tensor([0.0, 0.25, 0.5])
    assert osm.timestep_embedding(t.double(), dtype=torch.float64).dtype == torch.float64 and osm.timestep_embedding(t).dtype == torch.float32


def test_fp32_oracle_still_matches_the_reference_golden(golden_dir):
    """tests/test_oracle_s2mel.py::test_cfm_euler_with_cfg's comparison, at its tolerance: the fp32 path is what it was."""
    g = np.load(os.path.join(golden_dir, "s2mel.npz"))
    cfg = dc.config()
    w = {k: torch.from_numpy(v) for k, v in weights.synth_s2mel_weights(cfg, tag="golden/s2mel").items()}
    Tp, T = 11, 34
    z = torch.from_numpy(synth.uniform("golden/s2mel/cfm/z", (1, cfg.in_channels, T), 1.7))
    mu = torch.from_numpy(synth.uniform("golden/s2mel/cfm/mu", (1, T, cfg.content_dim), 1.0))
    prompt = torch.from_numpy(synth.uniform("golden/s2mel/cfm/prompt", (1, cfg.in_channels, Tp), 1.0))
    st = torch.from_numpy(synth.uniform("golden/s2mel/cfm/style", (1, cfg.style_dim), 1.0))
    out = osm.cfm_inference(w, cfg, mu, torch.LongTensor([T]), prompt, st, z, 3, 0.7)
    assert out.dtype == torch.float32
    np.testing.assert_allclose(out.numpy(), g["cfm"], rtol=0, atol=1e-4)
    w64 = {k: (v.double() if v.is_floating_point() else v) for k, v in w.items()}
    out64 = osm.cfm_inference(w64, cfg, mu.double(), torch.LongTensor([T]), prompt.double(), st.double(), z.double(), 3, 0.7)
    assert out64.dtype == torch.float64
    np.testing.assert_allclose(out64.numpy(), g["cfm"], rtol=0, atol=1e-4)
