"""The decode GEMVs (csrc/gemv_fx.hip: 44 instantiations of the fp32-MFMA GEMV; csrc/gemv_pl.hip: 20 of the plane GEMV) case by case:
which small GPT, weight format, row count and process-wide switches make the decode step launch which kernel, on what split of K --
and the float64 reference of each case.  tests/test_gemv_cases_cpu.py checks the table (through the library's own plan query) and the
reference; tests/test_gemv_plans_gpu.py runs the cases.

A case is (model, format, rows, plane_rows, narrow): `model` names a row of MODELS (model_dim, heads, layers, number_mel_codes),
`plane_rows` is the value handed to idxtts_set_decode_plane_rows (65 = every step on gemv_fx), `narrow` the one handed to
idxtts_set_decode_geometry.  The decode step issues five GEMV shapes (GPTModel::decode_step / decode_step_pl / head_logits, csrc/gpt.hip):

    c_attn      N = 3d  K = d    LayerNorm folded
    c_proj      N = d   K = d    residual, output as fragment images (gemv_fx) / with row statistics (gemv_pl)
    c_fc        N = 4d  K = d    LayerNorm folded, gelu_new
    mlp.c_proj  N = d   K = 4d   residual; the only launch that hands gemv_fx the K-split slab
    mel_head    N = V   K = d

and runs all five on the plane GEMV when (GPTModel::use_pl) the format is compact, rows >= plane_rows, d % 32 == 0 and the plane plan
of every one of the five shapes names a kernel that exists; otherwise all five on gemv_fx."""
import ctypes
import functools
from ctypes import c_void_p

import numpy as np
import torch

from indextts_amd import _lib, synth, weights
from indextts_amd.config import GPTConfig

FMT = {"f32": 0, "bf16": 1, "fp8": 2}
PENALTY = 10.0
L_TEXT, NEW, COND = 6, 5, 4          # text tokens (rows b % 3 shorter: left padding), generated tokens, conditioning latents

# name -> (model_dim, heads, layers, number_mel_codes)
MODELS = {
    "d64": (64, 1, 2, 90),              # kw = 4: four K slices per workgroup
    "d128": (128, 2, 2, 4200),          # mel_head in 4097..8192 columns: two column tiles per wave on a few megabytes; N % 16 != 0
    "d192": (192, 3, 2, 210),           # K = 192: a remainder of the plane GEMV's 32-k chunks per K part; N % 16 != 0
    "d256": (256, 4, 2, 210),
    "d320": (320, 5, 1, 8194),          # waves 10..15 without a chunk; mlp.c_proj: a K-piece workgroup without a chunk; last tile of 2 columns
    "d320e": (320, 5, 1, 8192),         # 512 column tiles: two per wave
    "d1280": (1280, 20, 1, 8194),       # the production width: cps = 5, the edge of the one-batch form
    "d1344": (1344, 21, 1, 8194),       # one head wider: cps = 6, the two-buffer form at every row count
}

# (model, format, rows, plane_rows, narrow)  # what only this case brings.  gemv_fx instantiations as <MT, NTW, one batch | two buffers, R4>
# of that format, gemv_pl ones as <MT, CT>.  The grid this was pruned from: every model x format x rows {1, 4, 5, 16, 17, 32, 33, 48, 49, 64}
# x plane_rows {65, 17, 5} (+ narrow at d = 1280, 5..16 rows); tests/test_gemv_cases_cpu.py holds the coverage this table has to keep.
CASES = [
    ("d64", "f32", 33, 17, False),      # fx <3,1,one batch>; kw = 4 (kw < 16), cps 1
    ("d64", "f32", 49, 17, False),      # fx <4,1,two buffers> f32
    ("d64", "bf16", 33, 65, False),     # fx <3,1,one batch> bf16
    ("d64", "fp8", 33, 65, False),      # fx <3,1,one batch> fp8
    ("d64", "fp8", 5, 5, False),        # pl <1,4> fp8; pl kparts 1
    ("d64", "fp8", 49, 17, False),      # pl <4,8> fp8; pl kparts 2 (mlp.c_proj: 8 chunks of 32 over parts of 5)
    ("d128", "f32", 5, 17, False),      # fx <1,1,one batch> and <1,2,one batch> (mel_head: 263 column tiles); N % 16 != 0 on fx
    ("d128", "f32", 17, 17, False),     # fx <2,1,one batch> and <2,2,one batch>
    ("d128", "bf16", 1, 65, False),     # fx <1,1,one batch,R4> and <1,2,one batch,R4> bf16
    ("d128", "bf16", 5, 65, False),     # fx <1,1,one batch> and <1,2,one batch> bf16
    ("d128", "bf16", 17, 65, False),    # fx <2,1,one batch> and <2,2,one batch> bf16
    ("d128", "fp8", 1, 65, False),      # the same three on fp8
    ("d128", "fp8", 5, 65, False),
    ("d128", "fp8", 17, 65, False),
    ("d192", "bf16", 5, 5, False),      # pl K remainder (6 chunks of 32 in parts of 10); pl <1,4> bf16; N % 16 != 0 on pl
    ("d256", "bf16", 48, 17, False),    # pl <3,4> at a third narrow width (mlp.c_proj: 32 chunks in 7 parts of 5, the last one short)
    ("d320", "f32", 1, 17, False),      # empty wave slices (waves 10..15); mlp.c_proj: an empty K-piece workgroup; cps 2; last tile of 2 columns
    ("d320", "bf16", 5, 5, False),      # pl with a last tile of 2 columns (V = 8194); pl kparts 4 (mlp.c_proj: 40 chunks of 32)
    ("d320e", "fp8", 4, 65, False),     # two column tiles per wave (512 tiles) over empty wave slices, R4
    ("d1280", "f32", 1, 17, False),     # fx <1,2,one batch,R4> f32; cps 5: the edge of the one-batch form
    ("d1280", "bf16", 5, 17, True),     # the narrow form, bf16: 8 waves x 10 chunks
    ("d1280", "bf16", 16, 17, True),
    ("d1280", "fp8", 5, 17, True),      # the narrow form, fp8
    ("d1280", "fp8", 16, 17, True),
    ("d1280", "bf16", 17, 17, False),   # pl <2,4> and <2,8> (mel_head: CT 4 -> 8 at 17 rows) bf16; pl kparts 4, 8 and 16
    ("d1280", "bf16", 33, 17, False),   # pl <3,4> and <3,8> (c_fc: CT 4 -> 8 at 33 rows) bf16
    ("d1280", "bf16", 64, 17, False),   # pl <4,8> bf16; pl kparts 32, the limit (mlp.c_proj)
    ("d1280", "fp8", 33, 17, False),    # pl <3,4> and <3,8> fp8
    ("d1344", "f32", 1, 17, False),     # fx <1,1,two buffers,R4> and <1,2,two buffers,R4> f32; cps 6
    ("d1344", "f32", 5, 17, False),     # fx <1,1,two buffers> and <1,2,two buffers> f32
    ("d1344", "f32", 17, 17, False),    # fx <2,1,two buffers> f32
    ("d1344", "f32", 33, 17, False),    # fx <3,1,two buffers> f32
    ("d1344", "bf16", 1, 65, False),    # the same four on bf16
    ("d1344", "bf16", 5, 65, False),
    ("d1344", "bf16", 17, 65, False),
    ("d1344", "bf16", 33, 65, False),
    ("d1344", "bf16", 64, 17, False),   # fx <4,1,two buffers> bf16 -- the 64-row compact decode whose plane plan names no kernel (mlp.c_proj)
    ("d1344", "fp8", 1, 65, False),     # the same four on fp8
    ("d1344", "fp8", 5, 65, False),
    ("d1344", "fp8", 17, 65, False),
    ("d1344", "fp8", 33, 65, False),
    ("d1344", "fp8", 49, 17, False),    # fx <4,1,two buffers> fp8 -- 49 rows, the first count without a plane kernel
    ("d1344", "fp8", 17, 17, False),    # pl <2,4> and <2,8> fp8; pl K remainder (42 chunks of 32 in parts of 10 and 5)
]


def model_dims(model):
    return MODELS[model]


def config(model):
    d, heads, layers, V = MODELS[model]
    return GPTConfig(model_dim=d, heads=heads, layers=layers, number_mel_codes=V, number_text_tokens=60, start_mel_token=V - 2,
                     stop_mel_token=V - 1, max_mel_tokens=40, max_text_tokens=20, cond_latents=COND)


def shapes(d, V):
    """(layer, N, K, with_slab) of the five GEMVs of a decode step."""
    return [("c_attn", 3 * d, d, False), ("c_proj", d, d, False), ("c_fc", 4 * d, d, False), ("mlp.c_proj", d, 4 * d, True),
            ("mel_head", V, d, False)]


def use_pl(d, V, fmt, rows, plane_rows):
    return fmt != "f32" and rows >= plane_rows and d % 32 == 0 and all(_lib.gemv_pl_plan(N, K, rows)["has_kernel"] for _, N, K, _ in shapes(d, V))


def launches(d, V, fmt, rows, plane_rows, narrow):
    """What the decode step of this case launches, from the library's plan query: [(layer, N, K, kind, plan)], kind "fx" | "pl"."""
    pl = use_pl(d, V, fmt, rows, plane_rows)
    out = []
    for layer, N, K, slab in shapes(d, V):
        plan = _lib.gemv_pl_plan(N, K, rows) if pl else _lib.gemv_fx_plan(N, K, rows, FMT[fmt], slab, narrow)
        out.append((layer, N, K, "pl" if pl else "fx", plan))
    return out


def fx_key(plan, fmt):
    """The template arguments of gemv_fx_kernel the plan selects (fx_launch_wt): (MT, NTW, SINGLE, format, R4, narrow)."""
    return (plan["mt"], plan["ntw"], bool(plan["single"]), fmt, bool(plan["r4"]), bool(plan["narrow"]))


def pl_key(plan, fmt, rows):
    """The template arguments of gemv_pl_kernel: (MT, CT, format)."""
    return ((rows + 15) // 16, plan["ct"], fmt)


def all_fx_keys():
    """The 44 instantiations fx_launch_wt can reach: per format 8 at MT 1 (R4 x NTW x SINGLE), MT 2: (2, one batch), (1, one batch),
    (1, two buffers); MT 3: both forms; MT 4: two buffers; and the narrow form on the two compact formats."""
    keys = set()
    for fmt in FMT:
        for r4 in (False, True):
            for ntw in (1, 2):
                for single in (False, True):
                    keys.add((1, ntw, single, fmt, r4, False))
        keys |= {(2, 2, True, fmt, False, False), (2, 1, True, fmt, False, False), (2, 1, False, fmt, False, False),
                 (3, 1, True, fmt, False, False), (3, 1, False, fmt, False, False), (4, 1, False, fmt, False, False)}
        if fmt != "f32":
            keys.add((1, 1, True, fmt, False, True))
    return keys


def edge_classes(d, V, fmt, rows, plane_rows, narrow):
    """The edge classes of the K split and of the column tiles that this case's launches fall in."""
    out = set()
    for layer, N, K, kind, p in launches(d, V, fmt, rows, plane_rows, narrow):
        if N % 16:
            out.add(f"{kind}:N%16")
        if kind == "fx":
            kc16 = (K + 15) // 16
            out.add(f"fx:cps{p['cps']}")
            if p["kw"] < 16:
                out.add("fx:kw<16")
            slices = p["kw"] * p["ksb"]
            if (slices - 1) * p["cps"] >= kc16:
                out.add("fx:empty-wave-slice")
            if p["ksb"] > 1 and (p["ksb"] - 1) * p["kw"] * p["cps"] >= kc16:
                out.add("fx:empty-k-piece-workgroup")
        else:
            out.add(f"pl:kparts{p['kparts']}")
            if ((K + 31) // 32) % ((8 // p["ct"]) * 5):
                out.add("pl:k-remainder")
    return out


def case_id(c):
    model, fmt, rows, plane_rows, narrow = c
    return f"{model}-{fmt}-{rows}r-pl{plane_rows}" + ("-narrow" if narrow else "")


# ---- the model every kernel runs, and its inputs --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def original_weights(model):
    return weights.synth_gpt_weights(config(model), tag=f"t/gemv/{model}")


def _fp8_round(x):
    """float32 -> the nearest OCP e4m3fn value (ties to the even code, saturating at 448), restated from csrc/wstream.hip::fp8_e4m3_encode."""
    a = np.abs(x).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7ffff + ((u >> 20) & 1)) & 0xfff00000).astype(np.uint32)
    normal = np.minimum(u.view(np.float32), np.float32(448.0))
    sub = (np.rint(a * np.float32(512.0)) / np.float32(512.0)).astype(np.float32)
    v = np.where(a < np.float32(0.015625), sub, normal)
    v = np.where(a < np.float32(448.0), v, np.float32(448.0)).astype(np.float32)
    return np.copysign(v, x).astype(np.float32)


def _fp8_quantize(w, axis):
    """quantize_matrix (csrc/wstream.hip) for fp8: a power-of-two scale per output channel, 2^ceil(log2(max|w| / 448)) (the maximum taken
    over `axis`, the K axis), and the nearest e4m3 value of w / scale."""
    mx = np.abs(w).max(axis=axis, keepdims=True).astype(np.float32)
    f, e = np.frexp(mx / np.float32(448.0))
    e = np.where(f == 0.5, e - 1, e)
    s = np.where(mx > 0, np.ldexp(np.float32(1.0), np.clip(e, -100, 100)), np.float32(1.0)).astype(np.float32)
    return (s * _fp8_round((w / s).astype(np.float32))).astype(np.float32)


def _restated_fp8_weights(model):
    """GPTModel::quantize_weights for fp8, restated (the library's transform first checks the device's fp8 decoder, so it runs only
    beside a GPU): c_attn / c_fc become (1, 0, Q(diag(ln.weight) W), ln.bias . W + b), c_proj / mlp.c_proj / mel_head Q(W).  The GPU file
    holds the model the library reads back against this one: weights equal, folded biases to a rounding of the float64 dot product."""
    cfg = config(model)
    w = {k: np.array(v, dtype=np.float32) for k, v in original_weights(model).items()}
    for i in range(cfg.layers):
        p = f"gpt.h.{i}"
        for ln, proj in ((".ln_1", ".attn.c_attn"), (".ln_2", ".mlp.c_fc")):
            g, b, W = w[p + ln + ".weight"], w[p + ln + ".bias"], w[p + proj + ".weight"]
            w[p + proj + ".bias"] = (b.astype(np.float64) @ W.astype(np.float64) + w[p + proj + ".bias"]).astype(np.float32)
            w[p + proj + ".weight"] = _fp8_quantize((g[:, None] * W).astype(np.float32), 0)
            w[p + ln + ".weight"], w[p + ln + ".bias"] = np.ones_like(g), np.zeros_like(b)
        for proj in (".attn.c_proj", ".mlp.c_proj"):
            w[p + proj + ".weight"] = _fp8_quantize(w[p + proj + ".weight"], 0)
    w["mel_head.weight"] = _fp8_quantize(w["mel_head.weight"], 1)
    return w


def effective_weights(model, fmt):
    """The rounded model under the reference's keys: what UnifiedVoice(..., keep_effective=True).effective_state_dict holds.  bf16 through
    the library (idxtts_gpt_quantize_weights is a host transform of the staged tensors, read back with idxtts_ctx_get_tensor), fp8
    restated above."""
    w = original_weights(model)
    if fmt == "f32":
        return w
    if fmt == "fp8":
        return _restated_fp8_weights(model)
    cfg = config(model)
    lib = _lib.load()
    c = _lib.GPTConfigC(cfg.model_dim, cfg.heads, cfg.layers, cfg.number_mel_codes, cfg.number_text_tokens, cfg.start_mel_token,
                        cfg.stop_mel_token, cfg.mel_pos_len, cfg.text_pos_len)
    h = c_void_p()
    _lib.check(lib.idxtts_gpt_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        for name, arr in w.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (ctypes.c_int64 * max(1, a.ndim))(*a.shape)
            _lib.check(lib.idxtts_ctx_load_tensor(h, name.encode(), c_void_p(a.ctypes.data), shape, a.ndim))
        _lib.check(lib.idxtts_gpt_quantize_weights(h, FMT[fmt]))
        return {k: _lib.get_tensor(h, k, tuple(v.shape)) for k, v in w.items()}
    finally:
        lib.idxtts_ctx_destroy(h)


def inputs(model, rows):
    """Rows 0 .. rows - 1 of the model's one input set (a row's prompt does not depend on how many rows are taken): conditioning
    latent, emotion vector, text with every third row one or two tokens shorter (left padding)."""
    cfg = config(model)
    d = cfg.model_dim
    lat = torch.from_numpy(synth.uniform(f"t/gemv/{model}/lat", (64, cfg.cond_latents, d), 0.5))
    emo = torch.from_numpy(synth.uniform(f"t/gemv/{model}/emo", (64, d), 0.3))
    text = torch.from_numpy(synth.integers(f"t/gemv/{model}/text", (64, L_TEXT), 2, cfg.number_text_tokens))
    for b in range(64):
        if b % 3:
            text[b, L_TEXT - (b % 3):] = cfg.stop_text_token
    return lat[:rows], emo[:rows], text[:rows]


def max_rows(model, fmt):
    return max([c[2] for c in CASES if c[0] == model and c[1] == fmt] + [1])


class Reference:
    """codes [R, n] and logits [R, n, V] of the float64 oracle on the rounded model, the float32 oracle's beside them."""

    def __init__(self, model, fmt, kv_round=False, eff=None):
        from oracle import gpt as og
        cfg = config(model)
        self.rows = max_rows(model, fmt)
        self.eff = effective_weights(model, fmt) if eff is None else eff
        tw = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.eff.items()}
        lat, emo, text = inputs(model, self.rows)
        conds = og.conds_latent(tw, cfg, lat, emo)
        self.fake = og.prepare_gpt_inputs(tw, cfg, conds, text)[0]
        with torch.no_grad():
            self.codes32, self.logits32 = og.generate_greedy(tw, cfg, conds, text, NEW, PENALTY, return_logits=True, kv_round=kv_round)
            if not kv_round:
                self.codes, self.logits = og.generate_greedy(tw, cfg, conds, text, NEW, PENALTY, return_logits=True, dtype=torch.float64)

    def margins(self):
        """[R, n] the float64 reference's own margin between its token and the runner-up, on the penalised scores the argmax sees."""
        from oracle import gpt as og
        R, n, _ = self.logits.shape
        out = torch.zeros(R, n, dtype=torch.float64)
        for s in range(n):
            ids = torch.cat([self.fake, self.codes[:, :s]], dim=1)
            top = torch.topk(og.repetition_penalty(ids, self.logits[:, s], PENALTY), 2, dim=-1)[0]
            out[:, s] = top[:, 0] - top[:, 1]
        return out

    def oracle_error(self, rows):
        """max |float32 oracle - float64 reference| over the logits of rows 0 .. rows - 1: what fp32 accumulation in ANOTHER summation order costs."""
        n = min(self.logits.shape[1], self.logits32.shape[1])
        return float((self.logits32[:rows, :n].double() - self.logits[:rows, :n]).abs().max())

    def tolerance(self, rows):
        """What a kernel may differ by from the float64 reference on rows 0 .. rows - 1: 4 x the float32 oracle's own error (both accumulate
        in fp32, in different orders), and never less than one fp32 ulp of the largest logit."""
        big = float(self.logits[:rows].abs().max())
        return max(4.0 * self.oracle_error(rows), float(np.spacing(np.float32(big))))


@functools.lru_cache(maxsize=None)
def reference(model, fmt):
    return Reference(model, fmt)


@functools.lru_cache(maxsize=None)
def reference_kv16(model, fmt):
    """The float32 oracle with keys / values rounded to bf16 (the library's bf16 KV cache)."""
    return Reference(model, fmt, kv_round=True)
