"""CPU: what tests/test_vocoder_dispatch_gpu.py rests on (cases and helpers: tests/vocoder_dispatch_cases.py).

  * the constants the case tables were derived from are still the ones in the sources (tile sizes, thresholds, limits);
  * a coverage ledger: conditions on the tables, computed with the restated dispatch -- every tile configuration meets both
    epilogue forms with 1 and with several taps, every configuration runs a transposed conv, both tile walks run with several
    time tiles, every aa_act position class occurs in the operator table and (where a row end can reach it) among the per-stage
    row ends of the ragged cases;
  * the oracle alone, row by row, on the ragged cases: float32 against float64 stays below a quarter of the GPU bound
    (measured: <= 8.4e-7 against 2e-5), and every row longer than one frame carries signal."""
import os
import re

import pytest
import torch

import vocoder_dispatch_cases as dc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "index-tts_amd", "csrc")
REDERIVE = "the tables of tests/vocoder_dispatch_cases.py were derived from the old value and must be re-derived"


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} not found"
    return int(m.group(1))


def _forward_body(text, name):
    m = re.search(r"\nint " + name + r"\(.*?\n\}\n", text, re.S)
    assert m, f"{name} not found"
    return m.group(0)


def test_constants_match_the_sources():
    aa = _src("aa_act.hip")
    for name in ("AA_TILE", "AA_TPW", "AA_XH", "AA_VH"):
        assert _const(aa, name) == getattr(dc, name), f"{name}: {REDERIVE}"
    assert _const(_src("conv1d.h"), "CONV_MAX_HALO") == dc.CONV_MAX_HALO, f"CONV_MAX_HALO: {REDERIVE}"
    # the one tile table (conv1d.h: conv_tile_dispatch) ...
    header = _src("conv1d.h")
    m = re.search(r"\nstatic inline int conv_tile_dispatch\(int M, F&& f\) \{\n(.*?)\n\}\n", header, re.S)
    assert m, "conv_tile_dispatch not found"
    table = m.group(1)
    rows = re.findall(r"if \(M > (\d+)\) return f\(ConvTile<(\d), (\d), (\d), (\d)>\{\}\);", table)
    last = re.findall(r"\n\s+return f\(ConvTile<(\d), (\d), (\d), (\d)>\{\}\);", table)
    assert len(rows) + len(last) == len(re.findall(r"ConvTile<\d", header)) == 4, "one table of four configurations"
    assert tuple(int(r[0]) for r in rows) == dc.CONV_M_THRESHOLDS, f"M thresholds: {REDERIVE}"
    tiles = [(int(tm), int(tn), int(wgm), int(wgn)) for _, tm, tn, wgm, wgn in rows] + [tuple(int(v) for v in last[-1])]
    assert tuple((32 * tm * wgm, 32 * tn * wgn) for tm, tn, wgm, wgn in tiles) == dc.CONV_CONFIGS, f"tile configurations: {REDERIVE}"
    assert "BM = 32 * TM_ * WGM_, BN = 32 * TN_ * WGN_" in header, f"tile size of a configuration: {REDERIVE}"
    # ... which both forward functions go through, the bf16 one with a separate K == 1 instance; no second table in either file
    f32, b16 = _src("conv1d.hip"), _src("conv1d_bf16x3.hip")
    assert "return conv_tile_dispatch(w.M, " in _forward_body(f32, "conv1d_forward")
    body16 = _forward_body(b16, "conv1d_bf16x3_forward")
    assert "return conv_tile_dispatch(w.M, " in body16
    assert re.search(r"w\.K == 1 \? launch_conv16<decltype\(tile\), true>\(.*?\) : launch_conv16<decltype\(tile\), false>\(", body16), \
        f"K1 dispatch: {REDERIVE}"
    for text in (f32, b16):
        assert not re.search(r"launch_conv(?:16)?<\d, \d, \d, \d", text) and "ConvTile<" not in text, "a second tile table"
    m = re.search(r"weight_bytes <= ([0-9.e]+)", _src("conv1d_bf16x3.hip"))
    assert m and float(m.group(1)) == dc.CONV_WALK_BYTES, f"walk limit: {REDERIVE}"
    assert "4.0 * w.M * (double)w.Cin * w.K" in _src("conv1d_bf16x3.hip"), f"walk's weight bytes: {REDERIVE}"


def test_helpers_at_the_switch_points():
    assert [dc.conv_config(m) for m in (1, 32, 33, 64, 65, 96, 97, 128, 129)] == \
        [(32, 512)] * 2 + [(64, 256)] * 2 + [(96, 256)] * 2 + [(128, 128)] * 3
    assert dc.epilogue_form(4) == "wide" and dc.epilogue_form(3) == dc.epilogue_form(5) == "narrow"
    assert dc.epilogue_form(8, transposed=True) == dc.epilogue_form(8, aligned=False) == "narrow"
    assert dc.walk(768, 768, 11) == 0 and dc.walk(768, 768, 3) == 1 and dc.walk(96, 9999, 11) == 0 and dc.walk(129, 18, 3) == 1
    assert dc.aa_position(1016) == {"edge"} and dc.aa_position(4064) == {"edge", "wg_edge"} and dc.aa_position(1) == set()
    assert dc.aa_position(1020) == {"edge+4"} and dc.aa_position(4065) == {"edge+1", "wg_edge+1"} and dc.aa_position(1008) == {"edge-8"}


def test_coverage_ledger_conv():
    plain = [dc.conv_geometry(case) for case, _ in dc.CONV_CASES]
    hit = {(cfg, form, one) for cfg, form, one, _, _, _ in plain}
    for cfg in dc.CONV_CONFIGS:
        for form in ("wide", "narrow"):
            for one in (True, False):
                assert (cfg, form, one) in hit, (cfg, form, one)
    for (case, _), (cfg, form, _, _, tiles, _) in zip(dc.CONV_CASES, plain):      # the switch-point claim: a second tile of 1 / 4 columns
        if case[1:5] == (18, case[2], 3, 2):
            assert tiles == 2 and case[5] - cfg[1] in (1, 4) and (form == "wide") == (case[5] - cfg[1] == 4), case
    halos = {((case[3] - 1) * case[4], dc.conv_geometry(case)[0][0]) for case, _ in dc.CONV_CASES}
    assert {(64, 32), (64, 96), (50, 96), (50, 64), (50, 32)} <= halos
    assert (dc.CONV_HALO_OVER[3] - 1) * dc.CONV_HALO_OVER[4] == dc.CONV_MAX_HALO + 1
    transposed = {dc.conv_geometry(case, transposed=True)[0] for case, _ in dc.CONVT_CASES}
    assert transposed == set(dc.CONV_CONFIGS)
    assert dc.conv_geometry(dc.CONVT_CASES[3][0], transposed=True)[5] == 2 and dc.CONVT_CASES[3][0][2] * dc.CONVT_CASES[3][0][4] == 132
    # both walks with several row blocks AND several time tiles (walk 0 with one row block is the same map as walk 1)
    every = plain + [dc.conv_geometry(case, transposed=True) for case, _ in dc.CONVT_CASES]
    for wk in (0, 1):
        assert any(w == wk and tiles > 1 and blocks > 1 for _, _, _, w, tiles, blocks in every), wk
    assert any(w == 0 and tiles > 1 and blocks > 1 for _, _, _, w, tiles, blocks in plain)      # ... walk 0 in a PLAIN conv
    for case, out_un, res_un in dc.CONV_UNALIGNED:      # wide-eligible, and narrow only because of the view
        assert (out_un or res_un) and dc.epilogue_form(case[5]) == "wide" and dc.epilogue_form(case[5], aligned=False) == "narrow"
    assert {dc.conv_config(c[0][2])[0] for c in dc.CONV_UNALIGNED} == {32, 64, 128}


def test_coverage_ledger_aa_act():
    table = set().union(*(dc.aa_position(T) for _, _, T in dc.AA_CASES))
    assert set(dc.AA_CLASSES) | {"edge-8", "edge+8"} <= table, table
    assert any(B > 1 and C % 2 and T % 4 and T > dc.AA_TILE for B, C, T in dc.AA_CASES)      # strides that are no tile multiples
    seam16 = set().union(*(dc.aa_position(T) for T in dc.AA16_T if T % 4 == 0))
    assert {"edge", "edge+4", "wg_edge"} <= seam16 and any(T % 4 for T in dc.AA16_T)
    # ragged rows end at multiples of 4 samples (the first up-sampling is x 4): +-1 classes cannot occur there
    ends = set()
    for _, width, Tm, lens in dc.RAGGED_CASES:
        cfg = dc.ragged_config(width)
        assert cfg.upsample_rates[0] % 4 == 0 and max(lens) == Tm
        for n in lens:
            for T_row in dc.stage_row_ends(cfg, n):
                ends |= dc.aa_position(T_row)
    assert set(dc.AA_CLASSES_ROW_ENDS) <= ends, ends
    assert not (set(dc.AA_CLASSES) - set(dc.AA_CLASSES_ROW_ENDS)) & ends
    cfg = dc.ragged_config(64)
    assert dc.stage_row_ends(cfg, 127)[1:3] == [2 * dc.AA_TILE, dc.AA_WG]
    assert [dc.stage_row_ends(cfg, n)[0] for n in (253, 254, 255)] == [dc.AA_TILE - 4, dc.AA_TILE, dc.AA_TILE + 4]


def test_coverage_ledger_ragged_conv():
    num, width, Tm, lens = dc.RAGGED_CASES[0]
    cfg = dc.ragged_config(width)
    assert {dc.conv_config(cfg.channels(i)) for i in range(cfg.num_upsamples + 1)} == set(dc.CONV_CONFIGS)
    assert dc.conv_config(cfg.channels(1))[0] == 96
    # conv_pre runs the wide form and a row ends inside one of its 4-vectors; one row is empty
    assert dc.epilogue_form(Tm) == "wide" and any(n % 4 for n in lens if n) and 0 in lens
    num, width, Tm, lens = dc.RAGGED_FULL
    cfg = dc.ragged_config(width)
    assert width == 1536 and dc.walk(cfg.channels(1) * 4, cfg.channels(0), 3) == 0 and dc.walk(cfg.channels(1), cfg.channels(1), 11) == 0
    assert dc.walk(cfg.channels(1), cfg.channels(1), 3) == 1


@pytest.mark.parametrize("case", dc.RAGGED_CASES, ids=[f"ragged{c[0]}" for c in dc.RAGGED_CASES])
def test_oracle_rows_float32_vs_float64(case):
    num, width, Tm, lens = case
    cfg, w = dc.ragged_weights(width)
    mel = dc.ragged_mel(num, cfg, len(lens), Tm)
    r64 = dc.ragged_oracle_rows(w, cfg, mel, lens, torch.float64)
    r32 = dc.ragged_oracle_rows(w, cfg, mel, lens, torch.float32)
    for b, n in enumerate(lens):
        if n == 0:
            assert r64[b] is None
            continue
        assert r64[b].dtype == torch.float64 and r32[b].dtype == torch.float32 and r64[b].shape == (1, n * cfg.total_upsample)
        amax = r64[b].abs().max().item()
        d = (r32[b].double() - r64[b]).abs().max().item()
        print(f"ragged{num} row {b} ({n} frames): max|ref| {amax:.3f}, fp32 - f64 {d:.2e}")
        assert d <= 0.25 * dc.RAGGED_ORACLE_ATOL * max(1.0, amax), (b, d)
        if n > 1:
            assert amax > 0.05, (b, amax)
