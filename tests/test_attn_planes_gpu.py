"""GPU: the DiT plane attention (csrc/attention.hip: flash_attn_planes_kernel in its two forms) on the cases of
tests/attn_planes_cases.py, through the instrument idxtts_attention_planes_fwd -- the library's own launcher on planes whose every bit
the test knows (tests/test_attn_planes_cases_cpu.py proves the table's coverage and sensitivity on the host).  Every output buffer
is prefilled with NaN (planes: a NaN bit pattern) and every call checks that nothing but the addressed outputs changed.

  * against float64: every case (shape x input kind x form): |out - float64 on the planes' own values| <= the case's bound --
    three-product form max(4 x the float32 restatement's own error, 2 fp32 ulps of the largest value), one-product form
    2^-8 max|v^| + 1e-5.  A failure names (batch row, head, query, needle key and its tile);
  * exact legs, each of which follows from the code: masked keys and padding rows do not reach the output (+-1e4 there against zeros);
    a batch row alone gives the bits it gives in the batch; a query range gives the bits of the whole row's call; a head's bits do
    not depend on the column layout or on the other heads; the one-product form never reads a lo plane (NaN there); o_planes is the
    split of o bit for bit, with or without o; empty rows are exactly zero;
  * argument rejections and no-ops of the launcher.
(The link to the product -- the solver's planes attention is what the instrument runs -- is in tests/test_s2mel_dispatch_gpu.py.)

The file prints a table of (case, float32 restatement error, kernel error, bound, ratio) and the worst ratio per form (-s).
Measured on an MI355X (max |out - float64| over the case; x3 = three-product form, x1 = one-product form; float32 = the restatement's
own error, which the kernel's follows to a few per cent nearly everywhere: the two evaluate the same arithmetic):

  shape-kind       x3 float32  x3 kernel   x3 bound  ratio  x1 float32  x1 kernel   x1 bound  ratio
  t5-natural        4.566e-06  4.566e-06  1.826e-05  0.250   1.494e-03  1.494e-03  6.632e-03  0.225
  t5-zero_q         4.768e-08  4.768e-08  2.384e-07  0.200   7.153e-08  7.153e-08  6.632e-03  0.000
  t5-needle         3.700e-06  8.747e-06  1.480e-05  0.591   1.829e-03  1.829e-03  6.632e-03  0.276
  t32-natural       4.964e-06  4.606e-06  1.986e-05  0.232   1.240e-03  1.240e-03  6.663e-03  0.186
  t32-zero_q        2.200e-08  2.235e-08  2.384e-07  0.094   0.000e+00  0.000e+00  6.663e-03  0.000
  t32-needle        6.173e-06  6.173e-06  2.469e-05  0.250   1.368e-03  1.368e-03  6.663e-03  0.205
  t33-natural       4.996e-06  5.011e-06  1.998e-05  0.251   1.173e-03  1.173e-03  6.663e-03  0.176
  t33-zero_q        3.025e-08  3.025e-08  2.384e-07  0.127   2.258e-08  2.258e-08  6.663e-03  0.000
  t33-needle        4.492e-06  4.433e-06  1.797e-05  0.247   1.142e-03  1.142e-03  6.663e-03  0.171
  t65-natural       3.738e-06  3.798e-06  1.495e-05  0.254   1.054e-03  1.054e-03  6.663e-03  0.158
  t65-zero_q        4.402e-08  4.402e-08  2.384e-07  0.185   9.313e-09  9.170e-09  6.663e-03  0.000
  t65-needle        5.292e-06  5.319e-06  2.117e-05  0.251   1.387e-03  1.387e-03  6.663e-03  0.208
  t97-natural       2.621e-06  2.633e-06  1.048e-05  0.251   8.024e-04  8.024e-04  6.663e-03  0.120
  t97-zero_q        3.833e-08  2.642e-08  2.384e-07  0.111   1.721e-08  1.721e-08  6.663e-03  0.000
  t97-needle        6.119e-06  6.059e-06  2.448e-05  0.248   8.684e-04  8.684e-04  6.663e-03  0.130
  t97k96-natural    3.341e-06  3.304e-06  1.337e-05  0.247   8.456e-04  8.456e-04  6.663e-03  0.127
  t97k96-zero_q     2.235e-08  2.670e-08  2.384e-07  0.112   9.934e-09  9.934e-09  6.663e-03  0.000
  t97k96-needle     6.623e-06  6.742e-06  2.649e-05  0.254   8.552e-04  8.552e-04  6.663e-03  0.128
  t129-natural      2.433e-06  2.356e-06  9.734e-06  0.242   8.813e-04  8.813e-04  6.663e-03  0.132
  t129-zero_q       4.453e-08  4.453e-08  2.384e-07  0.187   8.837e-09  8.837e-09  6.663e-03  0.000
  t129-needle       7.138e-06  6.781e-06  2.855e-05  0.237   1.239e-03  1.239e-03  6.663e-03  0.186
  b17-natural       6.044e-06  5.918e-06  2.418e-05  0.245   1.298e-03  1.298e-03  6.663e-03  0.195
  b17-zero_q        4.172e-08  4.172e-08  2.384e-07  0.175   1.788e-08  1.788e-08  6.663e-03  0.000
  b17-needle        6.613e-06  6.822e-06  2.645e-05  0.258   1.290e-03  1.290e-03  6.663e-03  0.194
  t300-natural      2.023e-06  2.098e-06  8.093e-06  0.259   6.178e-04  6.179e-04  6.663e-03  0.093
  t300-zero_q       2.156e-08  3.102e-08  2.384e-07  0.130   1.113e-08  1.113e-08  6.663e-03  0.000
  t300-needle       5.619e-06  5.793e-06  2.248e-05  0.258   8.520e-04  8.521e-04  6.663e-03  0.128
  tail65-natural    2.611e-06  2.604e-06  1.044e-05  0.249   6.856e-04  6.856e-04  6.663e-03  0.103
  tail65-zero_q     2.828e-08  3.025e-08  2.384e-07  0.127   1.013e-08  1.013e-08  6.663e-03  0.000
  tail65-needle     5.445e-06  5.557e-06  2.178e-05  0.255   7.169e-04  7.169e-04  6.663e-03  0.108
  tail144-natural   2.251e-06  2.251e-06  9.005e-06  0.250   6.209e-04  6.209e-04  6.663e-03  0.093
  tail144-zero_q    2.570e-08  4.902e-08  2.384e-07  0.206   1.132e-08  1.132e-08  6.663e-03  0.000
  tail144-needle    4.585e-06  4.525e-06  1.834e-05  0.247   6.214e-04  6.214e-04  6.663e-03  0.093
  plane attention, form x3: worst kernel error / bound 0.591 (t5-needle-x3: kernel 8.747e-06, float32 restatement 3.700e-06)
  plane attention, form x1: worst kernel error / bound 0.276 (t5-needle-x1: kernel 1.829e-03, float32 restatement 1.829e-03)
Every exact leg held bit for bit in both forms; the whole file takes about 3 s.
"""
import dataclasses
import time

import numpy as np
import pytest
import torch

import attn_planes_cases as ac
from indextts_amd import _lib, synth

pytestmark = pytest.mark.gpu

_TABLE = []
_T0 = time.time()
SLACK = 64                     # elements behind each output buffer that must keep their prefill


def _u16(a, device):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(device)


def launch(device, planes, *, Mrows, ncols, cols, T, q_row0, Sq, B, H, kend, form, out, o_ts=None, o_bs=None, scale=ac.SCALE,
           planes_offset_bytes=0, raw=False):
    """One instrument call on planes (uint16 [2 * plane_elems(Mrows, ncols)], host) -> (rows [B][Sq][64 H] float32 | None,
    (hi bits, lo bits) [B * Sq][64 H] | None).  Checks the NaN prefill outside the addressed outputs.  raw: -> (rc, rows buffer,
    planes buffer) unchecked, for the rejection tests."""
    d = 64 * H
    o_ts = o_ts if o_ts is not None else d + 24
    o_bs = o_bs if o_bs is not None else Sq * o_ts + 40
    dp = planes if isinstance(planes, torch.Tensor) else _u16(planes, device)
    dk = torch.tensor(list(kend), dtype=torch.int32, device=device) if kend is not None else None
    o = torch.full((max(B, 1) * o_bs + SLACK,), float("nan"), device=device) if out in ("rows", "both") else None
    n_op = ac.plane_elems(B * Sq, d)
    op = torch.full((2 * n_op + SLACK,), ac.NAN_BITS, dtype=torch.int16, device=device) if out in ("planes", "both") else None
    q_col, k_col, v_col = cols
    rc = _lib.load().idxtts_attention_planes_fwd(dp.data_ptr() + planes_offset_bytes, Mrows, ncols, q_col, k_col, v_col, T, q_row0, Sq, B, H,
                                                 _lib.ptr(dk), scale, _lib.ptr(o), o_bs, o_ts, _lib.ptr(op), int(form == 1),
                                                 _lib.current_stream())
    torch.cuda.synchronize()
    ho = o.cpu().numpy() if o is not None else None
    hp = op.cpu().numpy().view(np.uint16) if op is not None else None
    if raw:
        return rc, ho, hp
    _lib.check(rc)
    rows = bits = None
    if ho is not None:
        b, q, c = np.meshgrid(np.arange(B), np.arange(Sq), np.arange(d), indexing="ij")
        at = b * o_bs + q * o_ts + c
        rows = ho[at]
        untouched = np.ones(ho.shape, bool)
        untouched[at] = False
        assert np.isnan(ho[untouched]).all(), "fp32 output written outside its rows (stride gaps, behind Sq)"
        assert np.isfinite(rows).all(), "non-finite output (or an addressed element not written)"
    if hp is not None:
        assert (hp[2 * n_op:] == ac.NAN_BITS).all(), "output planes written behind their end"
        bits = ac.unpack_bits(hp, B * Sq, d)
        assert np.isfinite(ac.bf16_widen(bits[0])).all() and np.isfinite(ac.bf16_widen(bits[1])).all(), "an output plane element not written"
    return rows, bits


def call(device, s, x_or_planes, form, out=None, **over):
    """The call of shape s (any field overridden) on a matrix (packed here) or on packed planes."""
    planes = ac.pack(x_or_planes) if getattr(x_or_planes, "ndim", 1) == 2 else x_or_planes
    kw = dict(Mrows=s.Mrows, ncols=s.ncols, cols=s.cols, T=s.T, q_row0=s.q_row0, Sq=s.Sq, B=s.B, H=s.H, kend=s.kend, form=form,
              out=out or s.out, o_ts=s.o_ts, o_bs=s.o_bs)
    kw.update(over)
    return launch(device, planes, **kw)


def rows_of(device, s, x_or_planes, form, **over):
    """fp32 rows of the call, whatever outputs the shape names"""
    return call(device, s, x_or_planes, form, out="rows", **over)[0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    diff = _bits(a) != _bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} elements differ, first at {np.argwhere(diff)[:4].tolist()}, max |d| {np.abs(a - b).max():.3e}"


def _split_bits(rows):
    """(hi, lo) bits of fp32 rows [B][Sq][d] as the kernel's epilogue splits them, [B * Sq][d]"""
    r = rows.reshape(-1, rows.shape[-1])
    hi = ac.bf16_bits(r)
    return hi, ac.bf16_bits(r - ac.bf16_widen(hi))


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if _TABLE:
        ratio = lambda r: r[2] / r[3]
        print(f"\n{'case':<24}{'float32 err':>14}{'kernel err':>14}{'bound':>12}{'err/bound':>11}")
        for cid, oerr, kerr, bound in _TABLE:
            print(f"{cid:<24}{oerr:>14.3e}{kerr:>14.3e}{bound:>12.3e}{kerr / bound:>11.3f}")
        for form in ac.FORMS:
            rows = [r for r in _TABLE if r[0].endswith(f"-x{form}")]
            if rows:
                w = max(rows, key=ratio)
                print(f"plane attention, form x{form}: worst kernel error / bound {ratio(w):.3f} ({w[0]}: kernel {w[2]:.3e}, float32 restatement "
                      f"{w[1]:.3e}, bound {w[3]:.3e}); {len(rows)} cases")
    print(f"tests/test_attn_planes_gpu.py wall time: {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES])
def test_case_vs_float64(device, shape):
    s = ac.SHAPE[shape]
    failures = []
    for kind in ac.KINDS:
        planes = ac.pack(ac.inputs(shape, kind)[0])
        for form in ac.FORMS:
            c = ac.case(shape, kind, form)
            rows, bits = call(device, s, planes, form)
            if rows is None:        # planes only: the same bits as beside the fp32 rows, which carry the comparison
                rows, both = call(device, s, planes, form, out="both")
                assert np.array_equal(bits[0], both[0]) and np.array_equal(bits[1], both[1]), f"{c.id}: planes alone differ from planes beside rows"
            if bits is not None:
                want = _split_bits(rows)
                assert np.array_equal(bits[0], want[0]) and np.array_equal(bits[1], want[1]), f"{c.id}: o_planes is not the split of o"
            for b in range(s.B):
                if s.keys(b) == 0:
                    assert not _bits(rows[b]).any(), f"{c.id}: the empty row {b} is not exactly zero"
            err = np.abs(rows.astype(np.float64) - c.ref)
            kerr = float(err.max())
            print(f"\n{c.id}: float32 restatement {c.err32:.3e}, kernel {kerr:.3e}, bound {c.bound:.3e} ({kerr / c.bound:.3f} of it)")
            _TABLE.append((c.id, c.err32, kerr, c.bound))
            bad = np.argwhere(err.reshape(s.B, s.Sq, s.H, 64).max(axis=3) > c.bound)
            for b, q, h in bad[:6]:
                j = int(c.target[b, h, q])
                failures.append(f"{c.id} batch row {b} head {h} query {q} (row {s.q_row0 + q}, block {q // 128}, wave {q % 128 // 32}; "
                                f"{f'needle at key {j}, tile {j // 32}' if j >= 0 else 'no needle'}; {s.keys(b)} keys in {s.ntiles(b)} tiles): {err[b, q, 64 * h:64 * h + 64].max():.3e} from float64 > {c.bound:.3e}")
            if len(bad) > 6:
                failures.append(f"{c.id}: {len(bad)} (batch row, query, head) beyond the bound")
    assert not failures, "\n".join(failures[:40])


def _masked_variants(s, x):
    """x with the k / v columns of every row no query may see -- behind a batch row's kend, and the padding rows -- at zero and at
    +-1e4 (signs alternating along both axes)"""
    out = []
    for big in (False, True):
        y = np.array(x)
        for b in range(s.B + 1):
            lo, hi = (b * s.T + s.keys(b), (b + 1) * s.T) if b < s.B else (s.B * s.T, s.Mrows)
            for c0 in s.cols[1:]:
                blk = y[lo:hi, c0:c0 + s.d]
                r, c = np.meshgrid(np.arange(blk.shape[0]), np.arange(s.d), indexing="ij")
                blk[...] = np.where((r + c) % 2, 1e4, -1e4).astype(np.float32) if big else 0.0
        out.append(y)
    return out


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES if s.pad_rows or any(s.keys(b) < s.T for b in range(s.B))])
def test_masked_keys_and_padding_rows_do_not_reach_the_output(device, shape, form):
    s = ac.SHAPE[shape]
    zeros, big = _masked_variants(s, ac.inputs(shape, "natural")[0])
    assert not np.array_equal(zeros, big)
    _same(rows_of(device, s, big, form), rows_of(device, s, zeros, form), f"{shape} x{form}: +-1e4 behind kend against zeros there")


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES if s.B > 1])
def test_batch_row_alone_is_bit_identical(device, shape, form):
    s = ac.SHAPE[shape]
    x = ac.inputs(shape, "needle")[0]
    batch = rows_of(device, s, x, form)
    for b in (range(s.B) if s.B <= 3 else (0, 7, 8, 16)):
        alone = rows_of(device, s, x[b * s.T:(b + 1) * s.T], form, B=1, Mrows=s.T, kend=None if s.kend is None else (s.kend[b],))
        _same(alone[0], batch[b], f"{shape} x{form}: batch row {b} alone (Mrows = T) against the batch")


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES if s.q_row0 > 0])
def test_query_range_is_bit_identical_to_the_whole_row(device, shape, form):
    s = ac.SHAPE[shape]
    planes = ac.pack(ac.inputs(shape, "needle")[0])
    part = rows_of(device, s, planes, form)
    whole = rows_of(device, s, planes, form, q_row0=0, Sq=s.T, o_bs=s.T * s.o_ts + 40)
    _same(part, whole[:, s.q_row0:s.q_row0 + s.Sq], f"{shape} x{form}: queries [{s.q_row0}, {s.q_row0 + s.Sq}) against the whole row's call")


def _relayout(s, x):
    """(shape, matrix) with the same q / k / v values in the other column layout"""
    t = dataclasses.replace(s, alt_cols=not s.alt_cols)
    y = np.full((t.Mrows, t.ncols), np.nan, np.float32)
    for cs, ct in zip(s.cols, t.cols):
        y[:, ct:ct + t.d] = x[:, cs:cs + s.d]
    return t, y


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("shape", ["t65", "t97", "t129"])
def test_head_does_not_depend_on_columns_or_other_heads(device, shape, form):
    s = ac.SHAPE[shape]
    x = ac.inputs(shape, "needle")[0]
    base = rows_of(device, s, x, form)
    t, y = _relayout(s, x)
    assert t.cols != s.cols and t.ncols != s.ncols
    _same(rows_of(device, t, y, form), base, f"{shape} x{form}: columns {t.cols} of {t.ncols} against {s.cols} of {s.ncols}")
    other = synth.uniform(f"t/attn_planes/{shape}/other-heads", x.shape, 3.0)
    for h in range(s.H):
        z = np.array(x)
        for c0 in s.cols:
            keep = slice(c0 + 64 * h, c0 + 64 * h + 64)
            blk = np.array(other[:, c0:c0 + s.d])
            blk[:, 64 * h:64 * h + 64] = x[:, keep]
            z[:, c0:c0 + s.d] = blk
        got = rows_of(device, s, z, form)
        _same(got[..., 64 * h:64 * h + 64], base[..., 64 * h:64 * h + 64], f"{shape} x{form}: head {h} with the other heads' q, k, v replaced")
        assert not np.array_equal(got, base)


@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES])
def test_one_product_form_never_reads_a_lo_plane(device, shape):
    s = ac.SHAPE[shape]
    planes = ac.pack(ac.inputs(shape, "natural")[0])
    poisoned = planes.copy()
    poisoned[ac.plane_elems(s.Mrows, s.ncols):] = ac.NAN_BITS
    _same(rows_of(device, s, poisoned, 1), rows_of(device, s, planes, 1), f"{shape} x1: NaN in the lo planes")


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("shape", [s.name for s in ac.SHAPES])
def test_output_planes_are_the_split_of_the_rows(device, shape, form):
    s = ac.SHAPE[shape]
    planes = ac.pack(ac.inputs(shape, "natural")[0])
    rows, both = call(device, s, planes, form, out="both")
    _, alone = call(device, s, planes, form, out="planes")
    hi, lo = _split_bits(rows)
    for name, got in (("beside o", both), ("with o NULL", alone)):
        for plane, g, w in (("hi", got[0], hi), ("lo", got[1], lo)):
            diff = g != w
            assert not diff.any(), (f"{shape} x{form}: o_planes {name}, {plane} plane: {int(diff.sum())} elements are not the split of o, first at "
                                    f"(row b Sq + q, column) {np.argwhere(diff)[:4].tolist()}")
    _same(rows_of(device, s, planes, form, o_ts=s.d, o_bs=s.Sq * s.d), rows, f"{shape} x{form}: dense rows against strided rows")


def test_empty_rows_are_exactly_zero(device):
    s = ac.SHAPE["t129"]
    assert s.keys(2) == 0
    x = ac.inputs("t129", "natural")[0]
    for form in ac.FORMS:
        rows, bits = call(device, s, x, form, out="both")
        assert not _bits(rows[2]).any() and rows[:2].any()
        assert not bits[0][2 * s.Sq:].any() and not bits[1][2 * s.Sq:].any()
        every = rows_of(device, s, x, form, kend=(0, 0, 0))          # no tile at all in the whole launch
        assert not _bits(every).any()


def test_scale_is_applied_in_the_exponent(device):
    """the softmax scale is a parameter: at 0.25 on q / 2 the three-product form stays within the natural case's bound"""
    s = ac.SHAPE["t97"]
    c = ac.case("t97", "natural", 3)
    x = np.array(c.x)
    x[:, s.cols[0]:s.cols[0] + s.d] *= np.float32(0.5)              # exact: the split of q / 2 is half the split of q
    rows = rows_of(device, s, x, 3, scale=0.25)
    assert np.abs(rows.astype(np.float64) - c.ref).max() <= c.bound


def test_argument_rejections_and_no_ops(device):
    s = ac.SHAPE["t33"]
    planes = _u16(np.concatenate([ac.pack(ac.inputs("t33", "natural")[0]), np.zeros(16, np.uint16)]), device)
    lib = _lib.load()
    good = dict(Mrows=s.Mrows, ncols=s.ncols, cols=s.cols, T=s.T, q_row0=0, Sq=s.Sq, B=s.B, H=s.H, kend=s.kend, form=3, out="both")
    rc, o, op = launch(device, planes, raw=True, **good)
    assert rc == 0 and np.isfinite(o).any() and (op != ac.NAN_BITS).any()
    q, k, v = s.cols
    rejected = {
        "a column that is not a multiple of 16": (dict(cols=(q + 8, k, v)), "multiples of 16"),
        "ncols not a multiple of 16": (dict(ncols=s.ncols + 8), "multiples of 16"),
        "columns out of range": (dict(cols=(q, k, v + 16)), "out of range"),
        "q_row0 + Sq > T": (dict(q_row0=1), "rows"),
        "B T > Mrows": (dict(Mrows=s.B * s.T - 1), "rows"),
        "a misaligned planes pointer": (dict(planes_offset_bytes=2), "aligned"),
        "both outputs NULL": (dict(out="none"), "null pointer"),
    }
    for what, (change, text) in rejected.items():
        rc, o, op = launch(device, planes, raw=True, **{**good, **change})
        msg = (lib.idxtts_last_error() or b"").decode()
        assert rc != 0 and text in msg, f"{what}: rc {rc}, message {msg!r}"
        assert (o is None or np.isnan(o).all()) and (op is None or (op == ac.NAN_BITS).all()), f"{what}: rejected, yet an output was written"
    for what, change in (("B = 0", dict(B=0)), ("H = 0", dict(H=0, cols=(0, 0, 0))), ("Sq = 0", dict(Sq=0))):
        rc, o, op = launch(device, planes, raw=True, **{**good, **change})
        assert rc == 0, f"{what}: {(lib.idxtts_last_error() or b'').decode()}"
        assert np.isnan(o).all() and (op == ac.NAN_BITS).all(), f"{what}: a no-op wrote an output"
