"""GPU: the decode attention (csrc/decode.hip: decode_attn_body in its twelve forms) and the kv_store_* kernels on the cases of
tests/decode_attn_cases.py, through the instrument idxtts_decode_attn_probe_run -- the library's own store and attention launchers on
buffers whose every bit the test knows (tests/test_decode_attn_cases_cpu.py proves the table's coverage and sensitivity on the host).

  * against float64: every case (shape x input kind), under every config (nsplit 0 = the rule, 1, 2, 3, 5, 16; batch-invariant off and
    on): |out - float64| <= max(4 x the float32 restatement's own error, 2 fp32 ulps of the largest value) of that case.  Dead slots give
    zeros, the arrival counters are zero afterwards;
  * cache contents: after the store and a step the raw buffers equal the restated layout bit for bit -- codes, scales, bf16 bits at
    [0, len) and at pos, the sentinel everywhere else, fanned slots alike -- and the prefill's k / v columns hold the cached values;
  * exact legs: batch-invariant outputs do not depend on nsplit (1..16), the batch or the addressing mode; without the mode nsplit 0 is
    the restated rule and the two addressing modes agree; the fragment image is the row output permuted;
  * one wiring leg through generate(): teacher-forced logits of a 450-step decode past 1025 keys against the float64 oracle, mode off
    and on.

The file prints a table of (case, float32 error, kernel error, ratio) with the worst ratio last, and the worst per format (-s)."""
import time

import numpy as np
import pytest
import torch

import decode_attn_cases as dc
from indextts_amd import _lib

pytestmark = pytest.mark.gpu

_TABLE = []
_T0 = time.time()
OUT_SENTINEL = 777.0


class Probe:
    """One shape's buffers on the device: the first run stores the prefill, every run is one attention step."""

    def __init__(self, shape, device):
        self.shape, self.device = shape, device
        s = shape
        elem = np.dtype(dc.RAW_DTYPE[s.fmt]).itemsize
        fill = lambda nbytes: torch.full((nbytes,), dc.SENTINEL, dtype=torch.uint8, device=device)
        self.kc, self.vc = fill(s.B * s.H * s.Smax * 64 * elem), fill(s.B * s.H * s.Smax * 64 * elem)
        self.ksc = self.vsc = None
        if s.fmt == "fp8":
            self.ksc, self.vsc = fill(s.B * s.H * s.Smax * 4), fill(s.B * s.H * s.Smax * 4)
        self.qkv = torch.from_numpy(dc.prefill_qkv(s)).to(device)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)
        self.kstart = i32(list(s.kstart))
        self.slot_ids = i32(list(s.slot_ids)) if s.slot_ids is not None else None
        self.lens = i32(list(s.lens)) if s.lens is not None else None
        self.slots = i32([[p, 0, 0, 0, l] for p, l in zip(s.pos, s.live)]) if s.mode == "slots" else None
        self.ws_bytes = _lib.decode_attn_probe_workspace_bytes(s.H, s.B)
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=device)
        self.step = torch.zeros(s.B, 3 * s.d, device=device)
        self.out = torch.zeros(max(s.B * s.d, dc.frag_floats(s.B, s.d)), device=device)
        self.stored = False

    def run(self, step_qkv, nsplit, invariant, frag=False):
        """One step -> (output rows [B][d], or the whole fragment image; nsplit_used)."""
        s = self.shape
        self.step.copy_(torch.from_numpy(np.ascontiguousarray(step_qkv)))
        self.out.fill_(OUT_SENTINEL)
        torch.cuda.synchronize()
        store = not self.stored and s.S > 0
        ptr = lambda t: t.data_ptr() if t is not None else 0
        used = _lib.decode_attn_probe(
            kv_format=dc.FMT[s.fmt], heads=s.H, rows=s.B, smax=s.Smax, n=len(s.pre), S=s.S if store else 0, qkv=ptr(self.qkv),
            slot_ids=ptr(self.slot_ids), len=ptr(self.lens), fan=s.fan, kcache=ptr(self.kc), vcache=ptr(self.vc), kscale=ptr(self.ksc),
            vscale=ptr(self.vsc), step_qkv=ptr(self.step), pos=s.pos[0] if s.mode == "state" else 0, kstart=ptr(self.kstart),
            slot_state=ptr(self.slots), invariant=invariant, nsplit=nsplit, out_frag=int(frag), out=ptr(self.out), workspace=ptr(self.ws),
            workspace_bytes=self.ws_bytes)
        self.stored = True
        assert used == dc.resolve_nsplit(nsplit, invariant, s.B, s.H, s.Smax), "nsplit_used is not the restated rule"
        counters = self.ws[:s.B * s.H * 4].cpu().numpy().view(np.uint32)
        assert not counters.any(), f"{s.name}: arrival counters {counters} after the step (nsplit {nsplit}, invariant {invariant})"
        out = self.out.cpu().numpy()
        if frag:
            return out[:dc.frag_floats(s.B, s.d)], used
        assert (out[s.B * s.d:] == OUT_SENTINEL).all()
        return out[:s.B * s.d].reshape(s.B, s.d), used

    def raw(self):
        s = self.shape
        dt = dc.RAW_DTYPE[s.fmt]
        kg = 16 if s.fmt == "f32" else 8
        kc = self.kc.cpu().numpy().view(dt).reshape(s.B, s.H, kg, s.Smax, 64 // kg)
        vc = self.vc.cpu().numpy().view(dt).reshape(s.B, s.H, s.Smax, 64)
        sc = [t.cpu().numpy().view(np.float32).reshape(s.B, s.H, s.Smax) if t is not None else None for t in (self.ksc, self.vsc)]
        return kc, vc, sc[0], sc[1]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if _TABLE:
        ratio = lambda r: r[2] / r[3]
        print(f"\n{'case':<36}{'float32 err':>14}{'kernel err':>14}{'bound':>12}{'err/bound':>11}{'err/f32':>9}")
        for cid, oerr, kerr, bound in sorted(_TABLE, key=ratio):
            print(f"{cid:<36}{oerr:>14.3e}{kerr:>14.3e}{bound:>12.3e}{kerr / bound:>11.3f}{kerr / oerr if oerr else float('nan'):>9.2f}")
        for fmt in dc.FMT:
            rows = [r for r in _TABLE if f"-{fmt}-" in r[0]]
            if rows:
                w = max(rows, key=ratio)
                print(f"decode attention, {fmt}: worst kernel error / bound {ratio(w):.3f} ({w[0]}: kernel {w[2]:.3e}, float32 restatement "
                      f"{w[1]:.3e}); {len(rows)} cases")
    print(f"tests/test_decode_attn_gpu.py wall time: {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("shape", [s.name for s in dc.SHAPES])
def test_case_vs_float64(device, shape):
    s = dc.SHAPE[shape]
    p = Probe(s, device)
    failures = []
    for kind in dc.KINDS:
        c = dc.case(shape, kind)
        kerr = 0.0
        for ns, inv in dc.CONFIGS:
            for l in range(c.step_qkv.shape[0]):
                out, _ = p.run(c.step_qkv[l], ns, inv)
                assert np.isfinite(out).all(), f"{c.id} nsplit {ns} invariant {inv} launch {l}: non-finite output"
                for b in range(s.B):
                    if not s.live[b]:
                        assert not out[b].any(), f"{c.id}: a dead slot's output is not zero"
                err = np.abs(out.astype(np.float64) - c.ref[l]).max(axis=1)
                kerr = max(kerr, float(err.max()))
                if err.max() > c.bound:
                    b = int(np.argmax(err))
                    failures.append(f"{c.id} nsplit {ns} invariant {inv} launch {l} row {b} (needle at {c.target[l, b].tolist()}): "
                                    f"{err.max():.3e} from float64 > {c.bound:.3e}")
        print(f"\n{c.id}: float32 restatement {c.err32:.3e}, kernel {kerr:.3e}, bound {c.bound:.3e} ({kerr / c.bound:.3f} of it)")
        _TABLE.append((c.id, c.err32, kerr, c.bound))
    assert not failures, "\n".join(failures[:20]) + f"\n({len(failures)} launches beyond their bound)"


@pytest.mark.parametrize("shape", [s.name for s in dc.MAIN_SHAPES + dc.EXTRA_SHAPES])
def test_cache_contents(device, shape):
    s = dc.SHAPE[shape]
    want = dc.stored(s)
    p = Probe(s, device)
    before = dc.prefill_qkv(s)
    step = dc.step_qkv0(s)
    for n_run, (ns, inv) in enumerate(((0, 0), (5, 1), (16, 0))):      # a later step at the same position rewrites the same bits
        p.run(step, ns, inv)
        kc, vc, ksc, vsc = p.raw()
        for name, got, exp in (("kcache", kc, want.kcache), ("vcache", vc, want.vcache), ("kscale", ksc, want.kscale), ("vscale", vsc, want.vscale)):
            if exp is None:
                continue
            diff = _bits(got) != _bits(exp)
            assert not diff.any(), f"{shape} run {n_run}: {name} differs from the restated layout at {np.argwhere(diff)[:4].tolist()} ({int(diff.sum())} elements)"
    if s.fan > 1:
        for r, s0 in enumerate(s.slot_ids):
            ln = s.lens[r]
            for j in range(1, s.fan):
                assert np.array_equal(_bits(kc[s0 + j, :, :, :ln]), _bits(kc[s0, :, :, :ln])) and np.array_equal(_bits(vc[s0 + j, :, :ln]), _bits(vc[s0, :, :ln]))
    after = p.qkv.cpu().numpy()
    assert np.array_equal(_bits(after), _bits(want.qkv_after)), f"{shape}: the prefill's k / v columns are not the cached values"
    assert np.array_equal(_bits(after[..., :s.d]), _bits(before[..., :s.d]))


def _trio(n, fmt, device):
    """The main row of n keys in a 3-row DecodeState batch, in slot 2 of a 4-slot session and alone: [(probe, row)]"""
    return [(Probe(dc.SHAPE[f"n{n}-{fmt}-state"], device), 0), (Probe(dc.SHAPE[f"n{n}-{fmt}-slots"], device), 2),
            (Probe(dc.SHAPE[f"n{n}-{fmt}-state-b1"], device), 0)]


@pytest.mark.parametrize("fmt", list(dc.FMT))
@pytest.mark.parametrize("n", dc.N_VALUES)
def test_invariant_rows_are_bit_identical(device, n, fmt):
    """Batch-invariant mode: a row's output is one bit pattern for every nsplit 1..16, in a batch of 3, of 4 slots and of 1."""
    base = None
    for p, row in _trio(n, fmt, device):
        c = dc.case(p.shape.name, "natural")
        first = None
        for ns in range(1, 17):
            out, _ = p.run(c.step_qkv[0], ns, 1)
            if first is None:
                first = out
            assert np.array_equal(_bits(out), _bits(first)), f"{p.shape.name}: nsplit {ns} differs from nsplit 1 in rows {np.argwhere((_bits(out) != _bits(first)).any(axis=1)).ravel().tolist()}"
        if base is None:
            base = first[row]
        assert np.array_equal(_bits(first[row]), _bits(base)), f"{p.shape.name}: the main row differs from the 3-row batch's by {np.abs(first[row] - base).max():.3e}"


@pytest.mark.parametrize("fmt", list(dc.FMT))
@pytest.mark.parametrize("n", dc.N_VALUES)
def test_key_split_exact_legs(device, n, fmt):
    """Without the mode: nsplit 0 is the restated rule bit for bit, and at one explicit nsplit the addressing modes and batches agree."""
    trio = _trio(n, fmt, device)
    outs = {}
    for p, row in trio:
        c = dc.case(p.shape.name, "natural")
        s = p.shape
        ruled, used = p.run(c.step_qkv[0], 0, 0)
        assert used == dc.split_rule(s.B, s.H)
        explicit, _ = p.run(c.step_qkv[0], used, 0)
        assert np.array_equal(_bits(ruled), _bits(explicit)), f"{s.name}: nsplit 0 differs from nsplit {used}"
        for ns in dc.NSPLITS:
            outs[(s.name, ns)] = p.run(c.step_qkv[0], ns, 0)[0][row]
    for ns in dc.NSPLITS:
        a, b, c1 = (outs[(p.shape.name, ns)] for p, _ in trio)
        assert np.array_equal(_bits(a), _bits(b)), f"n {n} {fmt} nsplit {ns}: session and DecodeState forms differ by {np.abs(a - b).max():.3e}"
        assert np.array_equal(_bits(a), _bits(c1)), f"n {n} {fmt} nsplit {ns}: the row alone differs by {np.abs(a - c1).max():.3e}"


@pytest.mark.parametrize("shape", [s.name for s in dc.MAIN_SHAPES + dc.EXTRA_SHAPES])
def test_fragment_image_is_the_row_output_permuted(device, shape):
    s = dc.SHAPE[shape]
    p = Probe(s, device)
    step = dc.case(shape, "natural").step_qkv[0]
    for ns, inv in ((0, 0), (1, 0), (3, 0), (0, 1), (2, 1)):
        rows, _ = p.run(step, ns, inv)
        image, _ = p.run(step, ns, inv, frag=True)
        assert np.array_equal(_bits(dc.unfrag(image, s.B, s.d)), _bits(rows)), f"{shape} nsplit {ns} invariant {inv}"
        written = np.zeros(image.shape, bool)
        r, k = np.meshgrid(np.arange(s.B), np.arange(s.d), indexing="ij")
        written[dc.frag_index(r, k, s.d >> 4)] = True
        assert (image[~written] == OUT_SENTINEL).all(), f"{shape}: the image is written outside its {s.B} rows"


# ---- one wiring leg through generate(): the product's own attn_part, attn_cnt and Smax past 1025 keys ------------------------------
_WIRING = {}


def _wiring_reference():
    """tests/test_gpt_gpu.py::test_maximum_text_length_and_long_decode_vs_oracle's model and inputs; the float64 oracle's codes and
    logits and the float32 oracle's beside them (gemv_cases.Reference's rule), computed once for both modes."""
    if not _WIRING:
        from indextts_amd import synth, weights
        from indextts_amd.config import GPTConfig
        from oracle import gpt as og
        cfg = GPTConfig(model_dim=128, heads=2, layers=2, number_mel_codes=130, number_text_tokens=90, start_mel_token=128, stop_mel_token=129,
                        max_mel_tokens=1815, max_text_tokens=600, cond_latents=8)
        w = weights.synth_gpt_weights(cfg, tag="t/gpt/maxlen")
        w["mel_head.bias"] = w["mel_head.bias"].copy()
        w["mel_head.bias"][cfg.stop_mel_token] = -1e4          # never stop
        tw = {k: torch.from_numpy(v) for k, v in w.items()}
        B, L, NEW = 2, 600, 450
        lat = torch.from_numpy(synth.uniform("t/gpt/maxlen/lat", (B, cfg.cond_latents, cfg.model_dim), 0.5))
        emo = torch.from_numpy(synth.uniform("t/gpt/maxlen/emo", (B, cfg.model_dim), 0.3))
        text = torch.from_numpy(synth.integers("t/gpt/maxlen/text", (B, L), 2, cfg.number_text_tokens))
        text[1, 37:] = cfg.stop_text_token                      # a short row next to the maximal one (left-padded prompt)
        conds = og.conds_latent(tw, cfg, lat, emo)
        with torch.no_grad():
            codes, logits = og.generate_greedy(tw, cfg, conds, text, NEW, 10.0, return_logits=True, dtype=torch.float64)
            codes32, logits32 = og.generate_greedy(tw, cfg, conds, text, NEW, 10.0, return_logits=True)
        P = og.prepare_gpt_inputs(tw, cfg, conds, text)[0].shape[1] - 1
        _WIRING.update(cfg=cfg, w=w, lat=lat, emo=emo, text=text, NEW=NEW, codes=codes, logits=logits, codes32=codes32, logits32=logits32, keys=P + NEW)
    return _WIRING


@pytest.mark.parametrize("invariant", [False, True], ids=["off", "invariant"])
def test_generate_logits_vs_float64_past_1025_keys(device, invariant):
    from indextts_amd.gpt import UnifiedVoice
    r = _wiring_reference()
    cfg, NEW = r["cfg"], r["NEW"]
    assert r["keys"] > 1025 and r["codes"].shape == (2, NEW)
    # the float32 oracle's logits are those of the same token sequence as long as its codes are the float64 oracle's
    same = (r["codes32"] == r["codes"]).all(dim=0).long().cumprod(0)
    steps = int(same.sum()) + (1 if int(same.sum()) < NEW else 0)          # (a step's logits depend on the codes before it)
    assert steps >= NEW // 2, f"the float32 oracle leaves the float64 oracle's codes at step {steps}"
    uv = UnifiedVoice(r["w"], cfg, device=device, kv_format="f32", batch_invariant=invariant)
    _, _, logits = uv.inference_speech(r["lat"], r["text"], emo_vec=r["emo"], max_generate_length=NEW, repetition_penalty=10.0,
                                       return_logits=True, forced_codes=r["codes"])
    got = logits.cpu().double()
    # the stop token's logit carries the -1e4 bias (an ulp of 1e-3): the rule is applied to it and to the other columns separately
    cols = torch.ones(cfg.number_mel_codes, dtype=torch.bool)
    cols[cfg.stop_mel_token] = False
    for name, m in (("codes", cols), ("stop token", ~cols)):
        ref, ref32 = r["logits"][:, :, m], r["logits32"][:, :steps][:, :, m].double()
        oerr = float((ref32 - ref[:, :steps]).abs().max())
        tol = max(4.0 * oerr, float(np.spacing(np.float32(ref.abs().max()))))
        kerr = float((got[:, :, m] - ref).abs().max())
        print(f"\ngenerate, invariant {invariant}, {name}: {r['keys']} keys, float32 oracle error {oerr:.3e} over {steps} steps, kernel error "
              f"{kerr:.3e} over {NEW} ({kerr / oerr:.2f} x), bound {tol:.3e}")
        assert np.isfinite(kerr) and kerr <= tol, f"{name}: logits {kerr:.3e} from the float64 oracle (> {tol:.3e})"
