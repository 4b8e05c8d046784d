"""GPU: the CFM solver at every point where s2mel.hip::dit_eval switches kernel families, against the float64 oracle, in both
arithmetic modes, with the launch signature of each case asserted (cases and helpers: tests/s2mel_dispatch_cases.py; what the
bounds can and cannot see: tests/test_s2mel_dispatch_cpu.py).

Config S2MelConfig.tiny() (D = 128, 2 heads, depth 5, 3 WaveNet layers: halo 6), 3 Euler steps, cfg rate 0.7.  Every case runs in
GEMM_F32 (pins the geometry: tail cut, row lengths, Euler offset are host logic shared by both modes) and in GEMM_BF16X3 (pins
the plane hand-offs).  Bounds are those of test_s2mel_gpu.py::test_cfm_split_bf16_mode_vs_oracle (solver: fp32 max 3e-4 / mean
2e-5, split-bf16 max 3e-3 / mean 1e-4) and ::test_estimator_vs_reference_golden (1e-4 / 4e-4 x max(1, |ref|max)).

Paths, as the launch profile shows them in GEMM_BF16X3 mode (launches per call; tn = gemm_tn_kernel, the exact fp32 GEMM; v2 =
gemm_bf16x3_v2_kernel, the LDS-DMA GEMM; x3 = gemm_bf16x3_kernel, split-bf16 for shapes v2 does not take: the merge GEMM's K = 184,
conv2's 16 columns).  Attention is ONE family per call, 15 launches (5 blocks x 3 steps): the qkv planes decide it from M, also
in the last block of a compacted tail.  rows_norm_kernel is the only norm family at D = 128 (36 launches everywhere), so the
mixed cases show in the GEMM counts: the 17 GEMMs per evaluation that run on Mt rows (wo, w13, w2 of the last block; skip_linear
x 2, conv1; 8 in the WaveNet; res_projection, final linear, conv2) move to tn, 51 over 3 steps.  In GEMM_F32 mode every solver
and cfm_rows case is 125 tn, 15 flash_attn_f32_kernel, 15 rotary_qk_kernel, 36 rows_norm_kernel (one estimator evaluation: 47 /
5 / 5 / 12), no other GEMM or attention family.  rotary_qk_kernel runs wherever the qkv projection is not on the LDS-DMA GEMM
(15 launches in cases 1 and 10, 5 at estimator 127), nowhere else in GEMM_BF16X3 mode.  The table below is
s2mel_dispatch_cases.LAUNCHES as text; _check_signature asserts the counts of both modes exactly.  In the library's terms
(s2mel.hip): M and Mt are the rows of dit_eval's two RowSets, all frames and the tail; "planes" is RowSet::planes.

  case            M    t0   Mt  attention        tn   v2  x3  gather_tail_rows  path
  solver 1      254     0  254  bf16x3 (rows)   125    -   -   -                rows, no tail
  solver 2      256     0  256  planes            8  111   6   -                planes, two full 128-row tiles
  solver 3      258     0  258  planes            8  111   6   -                planes, 2-row last tile
  solver 4      400     0  400  planes            8  111   6   -                pmin - halo = 63: no tail
  solver 5      400    64  272  planes            8  111   6   6                planes tail
  solver 6      400    65  270  planes            8  111   6   6                planes tail, odd offset
  solver 7      400   144  112  planes           59   63   3   6                planes, then rows
  solver 8      544   144  256  planes            7  112   6   6                planes tail at its floor
  solver 9      542   144  254  planes           58   64   3   6                planes, then rows
  solver 10     240    94   52  bf16x3 (rows)   125    -   -   6                rows, rows tail
  solver 11    1200    70  780  planes            7  112   6   6                ragged, planes tail
  solver 12     600   104  184  planes           58   64   3   6                ragged, planes, then rows
  cfm_rows 1    800    70  520  planes            7  112   6   6                planes tail
  cfm_rows 2    760   134  224  planes           58   64   3   6                planes, then rows
  estimator 127 254     0  254  bf16x3 (rows)    47    -   -   -                one evaluation of B = 2 sequences
  estimator 128 256     0  256  planes            7   38   2   -
(tn 8 against 7: cond_projection runs on B*T rows, 200 in the B = 1 cases.)

Two streams (set_s2mel_overlap(1): each CFG half a dit_eval of its own on half the rows), max |d| against the stacked result:
cases 11 (1200 / 600, 780 / 390 rows) and 12 (600 / 300, 184 / 92): 0 in both modes; cases 5 and 7 (400 / 200 rows): 0 in
GEMM_F32, 6.7e-5 and 3.2e-5 in GEMM_BF16X3 (the halves run the fp32-row kernels), held to the oracle bounds.

How much of each bound is the reference's own rounding: max / mean |fp32 oracle - float64 oracle| on the compared frames (CPU),
beside what the library measured against the float64 oracle on an MI355X (max |d|, worst row):

  case           oracle fp32 - f64      GEMM_F32   GEMM_BF16X3
  solver 1       1.56e-05 / 2.32e-06    1.32e-05   1.51e-05
  solver 2       1.41e-05 / 2.67e-06    1.21e-05   9.16e-05
  solver 3       1.07e-05 / 1.57e-06    9.41e-06   5.95e-05
  solver 4       1.12e-05 / 1.55e-06    1.06e-05   7.05e-05
  solver 5       1.32e-05 / 1.85e-06    1.34e-05   7.31e-05
  solver 6       1.27e-05 / 2.11e-06    1.25e-05   6.42e-05
  solver 7       1.04e-05 / 6.56e-07    9.51e-06   3.61e-05
  solver 8       1.52e-05 / 1.66e-06    1.36e-05   6.78e-05
  solver 9       1.73e-05 / 1.34e-06    1.60e-05   5.11e-05
  solver 10      1.52e-05 / 5.95e-07    1.55e-05   1.44e-05
  solver 11      1.22e-05 / 1.02e-06    1.20e-05   7.53e-05
  solver 12      1.01e-05 / 4.73e-07    1.13e-05   4.44e-05
  cfm_rows 1     1.23e-05 / 2.71e-06    1.08e-05   6.34e-05
  cfm_rows 2     1.13e-05 / 2.77e-06    1.01e-05   4.65e-05
  estimator 127  8.66e-06 / 1.81e-06    8.52e-06   1.02e-05
  estimator 128  1.03e-05 / 1.66e-06    1.03e-05   6.31e-05
The reference's noise is at most 6 % of the fp32 max bound (14 % of the mean bound), nowhere near a quarter of it.

What the bounds catch (tests/test_s2mel_dispatch_cpu.py): a tail cut one frame late misses the oracle by 1.1e-3 .. 3.9e-3 in these
cases -- 3.7 .. 12.9 x the fp32 max bound, mostly INSIDE the split-bf16 one.  With the solver's tail_t0 moved one frame on purpose,
every tail case here failed its GEMM_F32 leg and only cases 5, 8 and 9 their GEMM_BF16X3 leg.
"""
import types

import pytest
import torch

import s2mel_dispatch_cases as dc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu

MODES = {"f32": _lib.GEMM_F32, "bf16x3": _lib.GEMM_BF16X3}
ATTENTION = ("flash_attn_planes_kernel", "flash_attn_bf16x3_kernel", "flash_attn_f32_kernel")


@pytest.fixture(scope="module")
def model(device):
    from indextts_amd.s2mel import S2Mel
    cfg = dc.config()
    w, _, tw64 = dc.synth_weights(cfg)
    # refs: float64 oracle results, computed once per case and shared by the two modes; runs: (output, launches) per profiled call
    return types.SimpleNamespace(cfg=cfg, sm=S2Mel(w, cfg, device=device, max_frames=512), tw64=tw64, refs={}, runs={})


def _call(mode, fn, overlap=False):
    """fn() in GEMM mode `mode`; stacked: under the launch profile -> (output on the host, {family: launches}); overlap: the CFG
    halves on two streams, unprofiled (profiling disables the overlap) -> (output, None).  Every setting is put back."""
    old_mode, old_overlap = _lib.get_gemm_mode(), _lib.get_s2mel_overlap()
    try:
        _lib.set_gemm_mode(MODES[mode])
        _lib.set_s2mel_overlap(overlap)
        if overlap:
            assert _lib.get_s2mel_overlap()
            return fn().cpu(), None
        try:
            _lib.profile_enable(True)
            out = fn().cpu()
            return out, {k: v["launches"] for k, v in _lib.profile_read().items()}
        finally:
            _lib.profile_enable(False)
    finally:
        _lib.set_s2mel_overlap(old_overlap)
        _lib.set_gemm_mode(old_mode)


def _solver_case(num):
    return next(c for c in dc.SOLVER_CASES if c[0] == num)


def _run_solver(m, num, mode, overlap=False):
    key = ("solver", num, mode, overlap)
    if key not in m.runs:
        _, lens, plens = _solver_case(num)
        z, mu, prompt, style = dc.solver_inputs(m.cfg, num, lens, plens)
        m.runs[key] = _call(mode, lambda: m.sm.cfm_inference(mu, torch.LongTensor(lens), prompt, style, None, dc.STEPS,
                                                             inference_cfg_rate=dc.CFG_RATE, z=z, prompt_lens=torch.LongTensor(plens)),
                            overlap)
    return m.runs[key]


def _run_rows(m, num, mode):
    key = ("rows", num, mode)
    if key not in m.runs:
        _, plens, glens = next(c for c in dc.ROWS_CASES if c[0] == num)
        gen, pcs, rms, style, z = dc.rows_inputs(m.cfg, num, plens, glens)
        m.runs[key] = _call(mode, lambda: m.sm.cfm_rows(gen, glens, pcs, rms, style, dc.STEPS, inference_cfg_rate=dc.CFG_RATE, z=z))
    return m.runs[key]


def _solver_ref(m, num):
    if ("solver", num) not in m.refs:
        _, lens, plens = _solver_case(num)
        m.refs["solver", num] = dc.solver_oracle_rows(m.tw64, m.cfg, lens, plens, dc.solver_inputs(m.cfg, num, lens, plens), torch.float64)
    return m.refs["solver", num]


def _check_solver_rows(what, out, ref, valid, mode):
    """out[b][:, :valid[b]] against the float64 oracle of row b alone, at test_cfm_split_bf16_mode_vs_oracle's bounds"""
    max_bound, mean_bound = dc.SOLVER_BOUNDS[mode]
    errs = [(out[b, :, :n].double() - ref[b]).abs() for b, n in enumerate(valid)]
    figures = [(e.max().item(), e.mean().item()) for e in errs]
    print(f"{what} {mode}: (max, mean) |d| per row vs float64 oracle:", [(f"{a:.2e}", f"{b:.2e}") for a, b in figures])
    for b, (emax, emean) in enumerate(figures):
        assert emax <= max_bound and emean <= mean_bound, (what, mode, b, emax, emean)


def _check_signature(what, prof, mode, geo, evals, depth, case):
    """The launch families of one call against the path (M, t0, Mt) names, and their launch counts against dc.LAUNCHES[mode][case]
    exactly: a later change of a threshold, or a launch that moves from one row set to the other, turns the case red."""
    M, t0, Mt = geo
    print(f"{what} {mode}: M = {M}, t0 = {t0}, Mt = {Mt}:", dict(sorted(prof.items())))
    assert tuple(prof.get(k, 0) for k in dc.LAUNCH_FAMILIES) == dc.LAUNCHES[mode][case], (what, mode, prof)
    planes = mode == "bf16x3" and M >= 256
    assert ("gather_tail_rows_kernel" in prof) == (t0 > 0), (what, mode, prof)
    assert ("flash_attn_planes_kernel" in prof) == planes and ("gemm_bf16x3_v2_kernel" in prof) == planes, (what, mode, prof)
    # every block's attention in ONE family: the qkv planes decide it from M, also in the last block of a compacted tail
    family = "flash_attn_planes_kernel" if planes else "flash_attn_bf16x3_kernel" if mode == "bf16x3" else "flash_attn_f32_kernel"
    assert [prof.get(k, 0) for k in ATTENTION] == [depth * evals if k == family else 0 for k in ATTENTION], (what, mode, prof)
    if mode == "f32":
        assert not [k for k in prof if "bf16x3" in k or "planes" in k], (what, prof)
    if mode == "bf16x3" and M < 256:       # no GEMM reaches 256 rows: nothing of the split-bf16 families may run
        assert not [k for k in prof if "gemm_bf16x3" in k or "planes" in k], (what, prof)


def _tail_gemms(cfg):
    """GEMMs of one dit_eval on the compacted rows: last block's wo, w13, w2; skip_linear's two halves, conv1; per WaveNet layer
    in / res / skip (the last layer has no res); res_projection, final linear, conv2"""
    return 3 + 3 + (3 * cfg.wn_layers - 1) + 3


def _check_mixed(what, prof, neighbour_prof, evals, tail_gemms):
    """M >= 256 > Mt: the transformer's GEMMs on the LDS-DMA kernel AND the tail's GEMMs on the exact fp32 one -- more launches of
    the latter, and fewer of the former, than a call of the same steps whose tail stays on planes (there the exact fp32 kernel
    runs the per-call constants only)"""
    assert prof.get("gemm_bf16x3_v2_kernel", 0) > 0, (what, prof)
    assert prof.get("gemm_tn_kernel", 0) > neighbour_prof.get("gemm_tn_kernel", 0), (what, prof, neighbour_prof)
    assert prof["gemm_bf16x3_v2_kernel"] < neighbour_prof["gemm_bf16x3_v2_kernel"], (what, prof, neighbour_prof)
    # exactly the GEMMs on Mt rows moved, no more (the module docstring lists the 17); the neighbour has the same per-call GEMMs
    assert prof["gemm_tn_kernel"] - neighbour_prof["gemm_tn_kernel"] == evals * tail_gemms, (what, prof, neighbour_prof)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("num", [c[0] for c in dc.SOLVER_CASES])
def test_solver_switch_points_vs_float64_oracle(model, num, mode):
    m = model
    _, lens, plens = _solver_case(num)
    geo = dc.geometry(m.cfg, lens, plens)
    assert geo == dc.SOLVER_GEOMETRY[num]
    out, prof = _run_solver(m, num, mode)
    assert out.shape == (len(lens), m.cfg.in_channels, max(lens)) and torch.isfinite(out).all()
    _check_signature(f"solver {num}", prof, mode, geo, dc.STEPS, m.cfg.depth, ("solver", num))
    if mode == "bf16x3" and num in dc.MIXED_NEIGHBOUR:
        nb = dc.MIXED_NEIGHBOUR[num]
        _check_mixed(f"solver {num}", prof, _run_solver(m, nb, mode)[1], dc.STEPS, _tail_gemms(m.cfg))
    _check_solver_rows(f"solver {num}", out, _solver_ref(m, num), lens, mode)
    for b, p in enumerate(plens):
        assert (out[b, :, :p] == 0).all(), (num, mode, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("num", dc.TWO_STREAM_CASES)
def test_solver_halves_on_two_streams(model, num, mode):
    """set_s2mel_overlap(1): each CFG half is a dit_eval of its own on B sequences.  Stacked and half row counts on the same side of
    256, for all frames (2BT, BT) and for the tail (2B*Tt, B*Tt): the same kernels on the same rows, bit-equal (cases 11, 12).
    Otherwise (cases 5, 7: 400 rows stacked, 200 per half) the halves leave the split-bf16 kernels: held to the oracle bounds;
    the exact-fp32 mode picks its kernels regardless of the row count and stays bit-equal."""
    m = model
    _, lens, plens = _solver_case(num)
    M, t0, Mt = dc.SOLVER_GEOMETRY[num]
    same_side = (M >= 256) == (M // 2 >= 256) and (Mt >= 256) == (Mt // 2 >= 256)
    assert same_side == (num in (11, 12))
    stacked, _ = _run_solver(m, num, mode)
    halves, _ = _run_solver(m, num, mode, overlap=True)
    assert not _lib.get_s2mel_overlap()
    valid = torch.zeros_like(stacked, dtype=torch.bool)
    for b, n in enumerate(lens):
        valid[b, :, :n] = True
    d = ((halves - stacked).abs() * valid).max().item()
    print(f"solver {num} {mode}: two streams vs stacked max |d| = {d:.2e}")
    if same_side or mode == "f32":
        assert torch.equal(halves[valid], stacked[valid]), (num, mode, d)
    _check_solver_rows(f"solver {num} two streams", halves, _solver_ref(m, num), lens, mode)
    for b, p in enumerate(plens):
        assert (halves[b, :, :p] == 0).all(), (num, mode, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("num", [c[0] for c in dc.ROWS_CASES])
def test_cfm_rows_switch_points_vs_float64_oracle(model, num, mode):
    m = model
    _, plens, glens = next(c for c in dc.ROWS_CASES if c[0] == num)
    geo = dc.geometry(m.cfg, [p + g for p, g in zip(plens, glens)], plens)
    assert geo == dc.ROWS_GEOMETRY[num]
    out, prof = _run_rows(m, num, mode)
    assert out.shape == (len(plens), m.cfg.in_channels, max(glens)) and torch.isfinite(out).all()
    _check_signature(f"cfm_rows {num}", prof, mode, geo, dc.STEPS, m.cfg.depth, ("rows", num))
    assert prof.get("cfm_rows_pack_kernel") == 1 and prof.get("cfm_rows_emit_kernel") == 1
    if mode == "bf16x3" and num == 2:
        _check_mixed("cfm_rows 2", prof, _run_rows(m, 1, mode)[1], dc.STEPS, _tail_gemms(m.cfg))
    if ("rows", num) not in m.refs:
        m.refs["rows", num] = dc.rows_oracle(m.tw64, m.cfg, plens, glens, dc.rows_inputs(m.cfg, num, plens, glens), torch.float64)
    _check_solver_rows(f"cfm_rows {num}", out, m.refs["rows", num], glens, mode)
    for b, g in enumerate(glens):
        assert (out[b, :, g:] == 0).all(), (num, mode, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("T", dc.ESTIMATOR_T)
def test_estimator_switch_point_vs_float64_oracle(model, T, mode):
    """One DiT.forward on two rows, lens [T, T - 31]: S2MelModel::estimator evaluates the conditional half alone (N2 = B = 2, no
    tail), so T = 127 / 128 put its 2T rows on either side of 256."""
    m = model
    inputs = dc.estimator_inputs(m.cfg, T)
    x, px, lens, style, mu = inputs
    out, prof = _call(mode, lambda: m.sm.estimator(x, px, lens, torch.full((2,), dc.ESTIMATOR_TIME), style, mu,
                                                   prompt_lens=[dc.ESTIMATOR_PROMPT] * 2))
    assert out.shape == x.shape
    _check_signature(f"estimator T = {T}", prof, mode, (2 * T, 0, 2 * T), 1, m.cfg.depth, ("estimator", T))
    if ("est", T) not in m.refs:
        m.refs["est", T] = dc.estimator_oracle_rows(m.tw64, m.cfg, inputs, torch.float64)
    ref = m.refs["est", T]
    scale = max(1.0, max(r.abs().max().item() for r in ref))
    errs = [(out[b, :, :n].double() - ref[b]).abs().max().item() for b, n in enumerate(lens)]
    print(f"estimator T = {T} {mode}: max |d| per row vs float64 oracle:", [f"{e:.2e}" for e in errs], f"scale {scale:.2f}")
    for b, e in enumerate(errs):
        assert e <= dc.ESTIMATOR_TOL[mode] * scale, (T, mode, b, e)


def test_instrument_runs_the_solver_s_planes_attention(model, device):
    """idxtts_attention_planes_fwd, which tests/test_attn_planes_gpu.py measures, launches the family the solver's planes path counts
    (solver 2: 15 launches of flash_attn_planes_kernel, asserted by _check_signature above) and no other: one launch per call, in
    either form."""
    import numpy as np

    import attn_planes_cases as ac
    _, solver_prof = _run_solver(model, 2, "bf16x3")
    assert solver_prof["flash_attn_planes_kernel"] == dc.STEPS * model.cfg.depth
    s = ac.SHAPE["t33"]
    c = ac.case("t33", "natural", 3)
    planes = torch.from_numpy(ac.pack(c.x).view(np.int16)).to(device)
    kend = torch.tensor(list(s.kend), dtype=torch.int32, device=device)
    o = torch.full((s.B, s.Sq, s.d), float("nan"), device=device)

    def instrument():
        for one_product in (0, 1):
            _lib.check(_lib.load().idxtts_attention_planes_fwd(planes.data_ptr(), s.Mrows, s.ncols, *s.cols, s.T, 0, s.Sq, s.B, s.H, _lib.ptr(kend),
                                                               ac.SCALE, _lib.ptr(o), s.Sq * s.d, s.d, None, one_product, _lib.current_stream()))
            if not one_product:
                first = o.clone()
        return first

    out, prof = _call("bf16x3", instrument)
    assert prof == {"flash_attn_planes_kernel": 2}, prof
    assert np.abs(out.double().numpy() - c.ref).max() <= c.bound
