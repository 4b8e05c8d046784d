"""GPU: `UnifiedVoice.score_codes` / `idxtts_gpt_score` (include/idxtts.h "Scoring given codes") -- the log-probabilities of GIVEN codes
from one prefill, the head in packed chunks of at most 64 positions, each chunk reduced by `score_rows_kernel`.

* the model path against the reference's fixtures (tests/score_cases.py: both layouts, rows 1 and 2 left-padded by 3 and 7);
* the kernel's arithmetic against the float64 log-softmax of the logits the same call returned, at V = 8194 and V = 130, natural and
  crafted rows, with lengths that make every chunk edge occur (1, 63, 64, 65, 129 codes; ragged 1 / 65 / 130; 16 rows of 5: a full
  chunk and a remainder of 16; a remainder of 17), fp32 weights (every chunk on the fp32-MFMA GEMV) and bf16 weights (the plane GEMV
  from 17 rows on);
* against the step path: generate(forced_codes=, return_logits=True), every KV and weight format;
* the batch-invariant mode: a row's values do not depend on the other rows, their order, the left padding or the chunk;
* the refusals, each before any launch.
Each test prints the largest error it saw (-s shows it)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import prefix_cases as pc
import sampler_cases as sc
import score_cases as sk
import scores_cases as scc
from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

pytestmark = pytest.mark.gpu

MAXMEL = 140      # sampler_cases.config: room in the mel position table for 130 codes
_MODELS = {}


def _model(device, key, weights_of, V, **kw):
    from indextts_amd.gpt import UnifiedVoice
    if key not in _MODELS:
        _MODELS[key] = UnifiedVoice(weights_of(), sc.config(V, MAXMEL), device=device, **kw)
    return _MODELS[key]


def _prompt(uv, V, B, width=5):
    conds, texts = sc.prompts(V, (width,), tag="t/score/prompt")
    row = uv.prompt_rows(conds[:1].to(uv.device), texts[0])[0]
    P, d = row.shape
    return row[None].expand(B, P, d).contiguous()


def _codes(V, lens, seed, stop_last=()):
    """Random non-stop codes [B, max lens]; rows in stop_last end on the stop token; columns from n_b on hold the stop token (never
    read: a call that read them would refuse them)."""
    rng = np.random.default_rng(seed)
    c = np.full((len(lens), max(lens)), V - 1, np.int64)
    for b, n in enumerate(lens):
        c[b, :n] = rng.integers(0, V - 2, n)
        if b in stop_last:
            c[b, n - 1] = V - 1
    return c


def _check(lp, logits, codes, lens, worst, what):
    lp, logits = lp.cpu().numpy(), logits.cpu().numpy()
    assert lp.dtype == np.float32 and lp.shape == codes.shape and np.isfinite(lp).all(), what
    ref = sk.ref_logprobs(logits, codes, lens)
    for b, n in enumerate(lens):
        assert (lp[b, n:] == 0.0).all(), f"{what} row {b}: a value beyond the row's {n} codes"
        assert not logits[b, n:].any(), f"{what} row {b}: logits beyond the row's {n} codes"
        err = np.abs(lp[b, :n].astype(np.float64) - ref[b, :n])
        bound = scc.bound(ref[b, :n])
        worst[0] = max(worst[0], float(err.max()))
        worst[1] = max(worst[1], float((err / bound).max()))
        assert (err <= bound).all(), f"{what} row {b}: |lp - ref| = {err.max():.3e}"
    return ref


# ---- the model path against the reference ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir, device):
    from indextts_amd.gpt import UnifiedVoice
    g, p, cases = sk.golden(golden_dir)
    cfg = GPTConfig.tiny()
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    uv = UnifiedVoice(w, cfg, device=device)
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(device), torch.from_numpy(g["text"]))
    assert (mask[:, :-1] == 0).sum(1).tolist() == [0, 3, 7]
    return g, cfg, w, uv, fake, emb, mask, cases


@pytest.mark.parametrize("layout", ["resume", "hf"])
def test_model_path_against_the_reference_fixtures(golden, layout):
    g, cfg, w, uv, fake, emb, mask, cases = golden
    codes, cols = cases[layout]
    lp, logits = uv.score_codes(torch.from_numpy(codes), emb, attention_mask=mask, layout=layout, return_logits=True)
    lp, logits = lp.cpu().numpy(), logits.cpu().numpy()
    assert lp.shape == codes.shape and logits.shape == codes.shape + (cfg.number_mel_codes,)
    worst_l = worst_p = 0.0
    for j, want in cols.items():
        worst_l = max(worst_l, float(np.abs(logits[:, j] - want).max()))
        for b in range(3):
            ref = scc.ref_logprob(want[b], codes[b, j])
            err = abs(float(lp[b, j]) - ref)
            worst_p = max(worst_p, err)
            assert err <= 2 * sk.LOGIT_BOUND + scc.bound(ref), (layout, b, j, err)
    print(f"{layout}: max |dlogit| vs the reference's fixtures = {worst_l:.3e} (bound {sk.LOGIT_BOUND:.0e}), max |dlp| = {worst_p:.3e}")
    assert worst_l <= sk.LOGIT_BOUND
    # the other layout's codes at the same positions are another function: the call tells the layouts apart as the fixtures do
    other = uv.score_codes(torch.from_numpy(codes), emb, attention_mask=mask, layout="hf" if layout == "resume" else "resume",
                           return_logits=True)[1].cpu().numpy()
    assert min(float(np.abs(other[:, j] - cols[j]).max()) for j in cols if j > 0) > 4.0


def test_model_path_against_the_float64_reference(golden):
    """Ragged lengths on the golden model: every scored position against score_cases.ref_logits (5e-4, the fixtures' bound)."""
    g, cfg, w, uv, fake, emb, mask, cases = golden
    codes = cases["hf"][0]
    lens = [11, 4, 1]
    for layout in ("resume", "hf"):
        lp, logits = uv.score_codes(torch.from_numpy(codes), emb, attention_mask=mask, code_lens=lens, layout=layout, return_logits=True)
        ref = sk.ref_logits(w, cfg, g["prep_embeds"], g["prep_mask"], [list(codes[b, :lens[b]]) for b in range(3)], layout=layout)
        err = max(float(np.abs(logits[b, :lens[b]].cpu().numpy() - ref[b, :lens[b]]).max()) for b in range(3))
        print(f"{layout} ragged {lens}: max |dlogit| vs float64 = {err:.3e}")
        assert err <= sk.LOGIT_BOUND
        want = sk.ref_logprobs(ref, codes, lens)
        assert (np.abs(lp.cpu().numpy() - want) <= 2 * sk.LOGIT_BOUND + scc.bound(want)).all()
        assert (lp[1, 4:] == 0).all() and (lp[2, 1:] == 0).all()


# ---- the kernel's arithmetic -------------------------------------------------------------------------------------------------
def _length_cases(V):
    cases = [([n], ()) for n in sk.ONE_ROW_LENGTHS]
    cases += [(list(sk.RAGGED_LENGTHS), (1,)), ([5] * 16, (0, 7)), ([27] * 3, ()), ([64, 64], (1,))]
    return cases


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
@pytest.mark.parametrize("V", scc.VOCABS)
def test_natural_rows_against_the_returned_logits(device, V, fmt):
    uv = _model(device, ("natural", V, fmt), lambda: sc.natural_weights(V, MAXMEL), V, weight_format=fmt)
    worst = [0.0, 0.0]
    n_vals = 0
    for i, (lens, stops) in enumerate(_length_cases(V)):
        codes = _codes(V, lens, 100 * V + i, stop_last=stops)
        emb = _prompt(uv, V, len(lens))
        lp, logits = uv.score_codes(torch.from_numpy(codes), emb, code_lens=lens, return_logits=True)
        _check(lp, logits, codes, lens, worst, f"V={V} {fmt} lens={lens}")
        n_vals += sum(lens)
        # a last-code stop token is scored, and so is a capped row's last code
        for b in stops:
            assert codes[b, lens[b] - 1] == V - 1 and lp[b, lens[b] - 1] < 0
        # without the logits: the same values, bit for bit
        assert pc.same_bits(uv.score_codes(torch.from_numpy(codes), emb, code_lens=lens).cpu().numpy(), lp.cpu().numpy())
    print(f"V={V} {fmt}: {n_vals} values, largest |lp - ref| = {worst[0]:.3e}, largest fraction of the bound = {worst[1]:.3f}")


@pytest.mark.parametrize("name", ["equal", "stop_-1e4", "peaked"])
@pytest.mark.parametrize("V", scc.VOCABS)
def test_crafted_rows(device, V, name):
    """A zero head weight: the logits are the bias on the 1/8 grid, the reference's inputs are exact."""
    bias = scc.crafted_rows(V)[name]
    uv = _model(device, ("crafted", V, name), lambda: sc.crafted_weights(bias, MAXMEL), V)
    ref_all = scc.ref_logprobs(bias)
    worst = [0.0, 0.0]
    for i, (lens, stops) in enumerate((([65], (0,)), (list(sk.RAGGED_LENGTHS), (2,)), ([5] * 16, ()))):
        codes = _codes(V, lens, 7 * V + i, stop_last=stops)
        codes[0, 0] = min(V - 3, 4096 + 5)      # the peaked row's peak
        lp, logits = uv.score_codes(torch.from_numpy(codes), _prompt(uv, V, len(lens)), code_lens=lens, return_logits=True)
        lg = logits.cpu().numpy()
        for b, n in enumerate(lens):
            assert np.array_equal(np.ascontiguousarray(lg[b, :n]).view(np.uint32), np.broadcast_to(bias.view(np.uint32), (n, V))), \
                "harness precondition: with a zero head weight the logits are the bias, bit for bit"
        _check(lp, logits, codes, lens, worst, f"V={V} {name} lens={lens}")
        for b, n in enumerate(lens):
            assert (np.abs(lp[b, :n].cpu().numpy() - ref_all[codes[b, :n]]) <= scc.bound(ref_all[codes[b, :n]])).all()
    if name == "equal":
        assert abs(float(lp[0, 0]) - scc.LOG_V[V]) <= scc.bound(scc.LOG_V[V])
    print(f"V={V} {name}: largest |lp - ref| = {worst[0]:.3e}, largest fraction of the bound = {worst[1]:.3f}")


def test_equals_what_a_scored_run_records(device):
    """The codes a scored greedy run emitted, scored again from one prefill: the same quantity through the prefill instead of the steps
    (fp32 cache: logits within 1e-3, hence lp within 2e-3 + the kernel's bound)."""
    V = 8194
    uv = _model(device, ("natural", V, "f32"), lambda: sc.natural_weights(V, MAXMEL), V)
    emb = _prompt(uv, V, 2)
    fake = pc.fake_ids(uv.cfg, 2, emb.shape[1])
    seq, lp_run = uv.generate(fake, max_new_tokens=20, tts_embeddings=emb, repetition_penalty=pc.PENALTY, return_logprobs=True)
    codes = seq[:, fake.shape[1]:]
    lens = [int((r == V - 1).nonzero()[0]) + 1 if (r == V - 1).any() else r.numel() for r in codes.cpu()]
    lp = uv.score_codes(codes, emb, code_lens=lens)
    for b, n in enumerate(lens):
        err = float((lp[b, :n] - lp_run[b, :n]).abs().max())
        print(f"row {b}: {n} codes, max |lp(score) - lp(run)| = {err:.3e}")
        assert err <= 2e-3 + 2e-5


# ---- against the step path ---------------------------------------------------------------------------------------------------
def _step_path(uv, g, ks):
    """(score-call logits [3, 10, V], teacher-forced logits [3, 10, V], {k: first new logits behind c[:, :k], layout "resume"})."""
    fake, emb, mask = uv.prepare_gpt_inputs(torch.from_numpy(g["conds"]).to(uv.device), torch.from_numpy(g["text"]))
    c = torch.from_numpy(g["step_codes"])
    kw = dict(attention_mask=mask, tts_embeddings=emb, repetition_penalty=10.0, return_logits=True)
    _, forced = uv.generate(fake, max_new_tokens=c.shape[1], forced_codes=c, **kw)
    first = {k: uv.generate(torch.cat([fake, c[:, :k]], 1), max_new_tokens=1, prefix_layout="resume", **kw)[1][:, 0].cpu().numpy() for k in ks}
    _, scored = uv.score_codes(c, emb, attention_mask=mask, return_logits=True)
    return scored.cpu().numpy(), forced.cpu().numpy(), first


def test_against_teacher_forced_steps_fp32(golden):
    g, cfg, w, uv, fake, emb, mask, cases = golden
    scored, forced, _ = _step_path(uv, g, ())
    for k in range(scored.shape[1]):
        err = float(np.abs(scored[:, k] - forced[:, k]).max())
        print(f"fp32 cache and weights, column {k}: max |dlogit| score call vs teacher-forced = {err:.3e} (bound 1e-3)")
        assert err <= 1e-3, (k, err)


@pytest.mark.parametrize("what,fmt", [("kv", "bf16"), ("kv", "fp8"), ("weights", "bf16"), ("weights", "fp8")])
def test_against_teacher_forced_steps_formats(golden_dir, device, what, fmt):
    """The bound: twice the largest difference, measured here, between that format's own prefix prefill (generate behind c[:, :k],
    one new token, layout "resume") and its teacher-forced column k, at k = 1, 4, 9 -- the same pair of paths."""
    from indextts_amd.gpt import UnifiedVoice
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    cfg = GPTConfig.tiny()
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    uv = UnifiedVoice(w, cfg, device=device, **({"kv_format": fmt} if what == "kv" else {"weight_format": fmt}))
    ks = (1, 4, 9)
    scored, forced, first = _step_path(uv, g, ks)
    base = max(float(np.abs(first[k] - forced[:, k]).max()) for k in ks)
    errs = {k: float(np.abs(scored[:, k] - forced[:, k]).max()) for k in range(scored.shape[1])}
    print(f"{what} {fmt}: prefix prefill vs teacher-forced at k = 1, 4, 9: {base:.3e} (bound {2 * base:.3e}); score call vs teacher-forced "
          f"per column: {' '.join(f'{e:.2e}' for e in errs.values())}")
    for k in ks:
        assert errs[k] <= 2 * base, (what, fmt, k, errs[k], base)


# ---- batch-invariant mode ----------------------------------------------------------------------------------------------------
def test_batch_invariant_rows_do_not_depend_on_the_call(device):
    from indextts_amd.gpt import UnifiedVoice
    cfg = sc.config(8194, MAXMEL)
    uv = UnifiedVoice(sc.natural_weights(8194, MAXMEL), cfg, device=device)
    uv.set_batch_invariant(True)
    conds, texts = sc.prompts(8194, (5, 9, 12), tag="t/score/inv")
    text = torch.full((3, 12), cfg.stop_text_token, dtype=torch.long)
    for i, t in enumerate(texts):
        text[i, :t.shape[1]] = t[0]
    _, emb, mask = uv.prepare_gpt_inputs(conds.to(device), text)
    pads = (mask[:, :-1] == 0).sum(1).tolist()
    assert sorted(pads) == [0, 3, 7]
    alone = [emb[i, pads[i]:][None].contiguous() for i in range(3)]
    lens = [70, 1, 33]
    codes = _codes(8194, lens, 5)
    n = max(lens)
    single = [uv.score_codes(torch.from_numpy(codes[i:i + 1]), alone[i], code_lens=[lens[i]], return_logits=True) for i in range(3)]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        o = list(order)
        lp, lg = uv.score_codes(torch.from_numpy(codes[o]), emb[o].contiguous(), attention_mask=mask[o], code_lens=[lens[i] for i in o],
                                return_logits=True)
        for r, i in enumerate(o):
            assert pc.same_bits(lp[r].cpu().numpy(), single[i][0][0].cpu().numpy()), (order, i)
            assert pc.same_bits(lg[r].cpu().numpy(), single[i][1][0].cpu().numpy()), (order, i)
    # across different n: row 2 alone at its own n = 33 (another S, other chunks)
    lp33, lg33 = uv.score_codes(torch.from_numpy(codes[2:3, :33]), alone[2], return_logits=True)
    d_lg = float((lg33[0] - single[2][1][0, :33]).abs().max())
    d_lp = float((lp33[0] - single[2][0][0, :33]).abs().max())
    print(f"batch-invariant, the same row at n = 33 and n = {n}: bits agree = {pc.same_bits(lp33[0].cpu().numpy(), single[2][0][0, :33].cpu().numpy())}, "
          f"max |dlogit| = {d_lg:.3e}, max |dlp| = {d_lp:.3e}")
    assert d_lg <= 1e-3 and d_lp <= 2e-3 + 2e-5


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _raw(uv, emb, codes, lens, n, pos0, ws_bytes=None, pad_left=None, null=None):
    lib = _lib.load()
    B, P, _ = emb.shape
    dc = codes.to(uv.device).contiguous()
    lp = torch.zeros(B, max(n, 1), device=uv.device)
    need = int(lib.idxtts_gpt_score_workspace_bytes(uv._h, B, P, max(n, 1))) or 1 << 20
    ws = torch.empty(need, dtype=torch.uint8, device=uv.device)
    la = None if lens is None else np.asarray(lens, np.int32)
    pl = None if pad_left is None else np.asarray(pad_left, np.int32)
    args = dict(emb=_lib.ptr(emb), codes=_lib.ptr(dc), lp=_lib.ptr(lp), ws=_lib.ptr(ws))
    if null:
        args[null] = ctypes.c_void_p(0)
    _lib.check(lib.idxtts_gpt_score(uv._h, args["emb"], pl.ctypes.data_as(ctypes.c_void_p) if pl is not None else ctypes.c_void_p(0), B, P,
                                    args["codes"], la.ctypes.data_as(ctypes.c_void_p) if la is not None else ctypes.c_void_p(0), n, pos0,
                                    args["lp"], ctypes.c_void_p(0), args["ws"], need if ws_bytes is None else ws_bytes, _lib.current_stream()))
    return lp


def test_refusals(device):
    V = 130
    uv = _model(device, ("natural", V, "f32"), lambda: sc.natural_weights(V, MAXMEL), V)
    cfg = uv.cfg
    emb = _prompt(uv, V, 2)
    ok = torch.from_numpy(_codes(V, [6, 6], 3))
    want = uv.score_codes(ok, emb).cpu().numpy()
    stop_mid, outside = ok.clone(), ok.clone()
    stop_mid[1, 2] = cfg.stop_mel_token
    outside[0, 5] = V
    table = cfg.mel_pos_len      # pos0 + n - 1 must stay below it
    long = torch.zeros(2, table, dtype=torch.long)
    for kw, msg in ((dict(codes=stop_mid, lens=None, n=6, pos0=2), "a stop token before a row's last code"),
                    (dict(codes=outside, lens=None, n=6, pos0=2), "outside the mel code table"),
                    (dict(codes=-ok - 1, lens=None, n=6, pos0=2), "outside the mel code table"),
                    (dict(codes=ok, lens=[6, 0], n=6, pos0=2), "1 <= n_b <= n"),
                    (dict(codes=ok, lens=[7, 6], n=6, pos0=2), "1 <= n_b <= n"),
                    (dict(codes=ok, lens=None, n=6, pos0=0), "prefix_pos0"),
                    (dict(codes=ok, lens=None, n=6, pos0=3), "prefix_pos0"),
                    (dict(codes=long, lens=None, n=table - 1, pos0=2), "exceed the mel position table"),
                    (dict(codes=long, lens=None, n=table, pos0=1), "exceed the mel position table"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, ws_bytes=4096), "workspace too small"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, pad_left=[0, emb.shape[1]]), "pad_left"),
                    (dict(codes=ok, lens=None, n=0, pos0=2), "shape"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, null="emb"), "null pointer"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, null="codes"), "null pointer"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, null="lp"), "null pointer"),
                    (dict(codes=ok, lens=None, n=6, pos0=2, null="ws"), "workspace too small")):
        with pytest.raises(RuntimeError, match=msg):
            _raw(uv, emb, **kw)
        # refused before anything ran: the next valid call gives what it gave
        assert pc.same_bits(_raw(uv, emb, ok, None, 6, 2).cpu().numpy(), want), msg
    # the longest sequence the table admits runs in either layout
    assert torch.isfinite(_raw(uv, emb, long, None, table - 2, 2)).all() and torch.isfinite(_raw(uv, emb, long, None, table - 1, 1)).all()
    assert int(_lib.load().idxtts_gpt_score_workspace_bytes(uv._h, 65, 8, 4)) == 0
    # the wrapper's own refusals
    with pytest.raises(ValueError, match="layout"):
        uv.score_codes(ok, emb, layout="other")
    with pytest.raises(ValueError, match="one row per prompt"):
        uv.score_codes(ok[:1], emb)
    with pytest.raises(ValueError, match="code_lens"):
        uv.score_codes(ok, emb, code_lens=[6])
    with pytest.raises(RuntimeError, match="stop token"):
        uv.score_codes(stop_mid, emb)
    # a stop token as a row's LAST code is accepted, at any length
    last = ok.clone()
    last[0, 3] = cfg.stop_mel_token
    lp = uv.score_codes(last, emb, code_lens=[4, 6])
    assert (lp[0, :4] < 0).all() and (lp[0, 4:] == 0).all()
