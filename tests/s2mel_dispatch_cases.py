"""Cases of tests/test_s2mel_dispatch_gpu.py and tests/test_s2mel_dispatch_cpu.py: shapes at which the CFM solver
(index-tts_amd/csrc/s2mel.hip::dit_eval) switches kernel families, their synthetic inputs and the oracle calls both files share.

dit_eval runs on two row sets (s2mel.hip: RowSet, built by row_set; N2 = 2B sequences stacked, B per half with
idxtts_s2mel_set_overlap(1)) and picks its kernels from three numbers:
  M  = N2 * T            all frames.  Split-bf16 mode and M >= 256: RowSet::planes, producers hand bf16 hi/lo planes on, attention
                         is flash_attn_planes_kernel
  t0 = pmin - halo       when >= 64 (else 0, and the tail is the set of all frames): the last block (dit_block) behind K/V, long
                         skip, WaveNet and final layer run on the tail rows [N2][T - t0]
  Mt = N2 * (T - t0)     the tail.  The 256-row test again on the compacted rows; M >= 256 > Mt hands planes over to fp32 rows in
                         the last block
S2MelConfig.tiny(): 3 WaveNet layers of kernel 5, dilation rate 1 -> halo = 6, tail compaction from a 70-frame prompt on."""
import numpy as np
import torch

from indextts_amd import synth, weights
from indextts_amd.config import S2MelConfig
from oracle import s2mel as osm

STEPS, CFG_RATE = 3, 0.7
TAG = "t/s2mel/dispatch"
# bounds of tests/test_s2mel_gpu.py::test_cfm_split_bf16_mode_vs_oracle (same config, steps and input scales): (max, mean)
SOLVER_BOUNDS = {"f32": (3e-4, 2e-5), "bf16x3": (3e-3, 1e-4)}
# tests/test_s2mel_gpu.py::test_estimator_vs_reference_golden: tol * max(1, |ref|max)
ESTIMATOR_TOL = {"f32": 1e-4, "bf16x3": 4e-4}

# (number, lens, prompt lens): stacked rows M = 2 * B * max(lens)
SOLVER_CASES = [
    (1, [127], [20]),                         # M = 254: rows, no tail
    (2, [128], [20]),                         # M = 256: planes, exactly two 128-row tiles
    (3, [129], [20]),                         # M = 258: planes, a 2-row last tile
    (4, [200], [69]),                         # pmin - halo = 63: no tail
    (5, [200], [70]),                         # t0 = 64, Mt = 272: planes tail
    (6, [200], [71]),                         # t0 = 65 (odd offset), Mt = 270
    (7, [200], [150]),                        # t0 = 144, Mt = 112: planes, then rows
    (8, [272], [150]),                        # Mt = 256: planes tail at its floor
    (9, [271], [150]),                        # Mt = 254: mixed, one step below
    (10, [120], [100]),                       # M = 240: tail (t0 = 94) with no planes anywhere
    (11, [200, 137, 171], [150, 90, 76]),     # ragged, t0 = 70, Mt = 780, row 1 has 67 tail frames
    (12, [150, 131], [120, 110]),             # ragged, M = 600, t0 = 104, Mt = 184: mixed
]
# what the table above claims, checked by test_s2mel_dispatch_cpu.py::test_case_table_geometry: number -> (M, t0, Mt)
SOLVER_GEOMETRY = {1: (254, 0, 254), 2: (256, 0, 256), 3: (258, 0, 258), 4: (400, 0, 400), 5: (400, 64, 272), 6: (400, 65, 270),
                   7: (400, 144, 112), 8: (544, 144, 256), 9: (542, 144, 254), 10: (240, 94, 52), 11: (1200, 70, 780),
                   12: (600, 104, 184)}
MIXED_NEIGHBOUR = {7: 5, 9: 8, 12: 11}        # mixed case -> a case of the same steps whose tail stays on planes
TWO_STREAM_CASES = [5, 7, 11, 12]

# mixed-prompt entry (S2Mel.cfm_rows): (number, prompt lens, target lens)
ROWS_CASES = [
    (1, [150, 76], [50, 95]),                 # T = 200, t0 = 70, Mt = 520
    (2, [150, 140], [40, 30]),                # T = 190, t0 = 134, Mt = 224: mixed
]
ROWS_GEOMETRY = {1: (800, 70, 520), 2: (760, 134, 224)}

# estimator: B = 2, lens [T, T - 31]; S2MelModel::estimator evaluates the conditional half alone (N2 = B), so M = 2 * T
ESTIMATOR_T = [127, 128]
ESTIMATOR_PROMPT = 20
ESTIMATOR_TIME = 0.35


# Launches per call of the families a path shows in (the launch profile of every case, as the library's event profile counts
# them; tests/test_s2mel_dispatch_gpu.py asserts them exactly).  Columns: LAUNCH_FAMILIES.  tn = the exact fp32 GEMM, v2 = the
# LDS-DMA split-bf16 GEMM, x3 = the split-bf16 tile GEMM (shapes v2 does not take: the merge GEMM's K = 184, conv2's 16 columns).
LAUNCH_FAMILIES = ("gemm_tn_kernel", "gemm_bf16x3_v2_kernel", "gemm_bf16x3_kernel", "flash_attn_planes_kernel", "flash_attn_bf16x3_kernel",
                   "flash_attn_f32_kernel", "gather_tail_rows_kernel", "rows_norm_kernel", "rotary_qk_kernel")
_F32_SOLVE, _F32_SOLVE_TAIL, _F32_EST = (125, 0, 0, 0, 0, 15, 0, 36, 15), (125, 0, 0, 0, 0, 15, 6, 36, 15), (47, 0, 0, 0, 0, 5, 0, 12, 5)
LAUNCHES = {
    "f32": {**{("solver", n): _F32_SOLVE for n in (1, 2, 3, 4)}, **{("solver", n): _F32_SOLVE_TAIL for n in range(5, 13)},
            ("rows", 1): _F32_SOLVE_TAIL, ("rows", 2): _F32_SOLVE_TAIL, ("estimator", 127): _F32_EST, ("estimator", 128): _F32_EST},
    "bf16x3": {                       #  tn   v2  x3  planes  bf16x3  f32  gather  norm  rotary
        ("solver", 1):                 (125,   0,  0,      0,     15,   0,      0,   36,     15),      # rows, no tail
        ("solver", 2):                 (  8, 111,  6,     15,      0,   0,      0,   36,      0),      # planes, two full 128-row tiles
        ("solver", 3):                 (  8, 111,  6,     15,      0,   0,      0,   36,      0),      # planes, 2-row last tile
        ("solver", 4):                 (  8, 111,  6,     15,      0,   0,      0,   36,      0),      # pmin - halo = 63: no tail
        ("solver", 5):                 (  8, 111,  6,     15,      0,   0,      6,   36,      0),      # planes tail
        ("solver", 6):                 (  8, 111,  6,     15,      0,   0,      6,   36,      0),      # planes tail, odd offset
        ("solver", 7):                 ( 59,  63,  3,     15,      0,   0,      6,   36,      0),      # planes, then rows
        ("solver", 8):                 (  7, 112,  6,     15,      0,   0,      6,   36,      0),      # planes tail at its floor
        ("solver", 9):                 ( 58,  64,  3,     15,      0,   0,      6,   36,      0),      # planes, then rows
        ("solver", 10):                (125,   0,  0,      0,     15,   0,      6,   36,     15),      # rows, rows tail
        ("solver", 11):                (  7, 112,  6,     15,      0,   0,      6,   36,      0),      # ragged, planes tail
        ("solver", 12):                ( 58,  64,  3,     15,      0,   0,      6,   36,      0),      # ragged, planes, then rows
        ("rows", 1):                   (  7, 112,  6,     15,      0,   0,      6,   36,      0),      # planes tail
        ("rows", 2):                   ( 58,  64,  3,     15,      0,   0,      6,   36,      0),      # planes, then rows
        ("estimator", 127):            ( 47,   0,  0,      0,      5,   0,      0,   12,      5),      # one evaluation of B = 2 sequences
        ("estimator", 128):            (  7,  38,  2,      5,      0,   0,      0,   12,      0),
    },
}


def config():
    return S2MelConfig.tiny()


def halo(cfg) -> int:
    h, dil = 0, 1
    for _ in range(cfg.wn_layers):
        h += (cfg.wn_kernel - 1) // 2 * dil
        dil *= cfg.wn_dilation_rate
    return h


def tail_t0(cfg, plens) -> int:
    """The solver's rule (s2mel.hip: upload_lens, called by S2MelModel::cfm_solve)."""
    cut = min(plens) - halo(cfg)
    return cut if cut >= 64 else 0


def geometry(cfg, lens, plens, stacked: int = 2):
    """(M, t0, Mt) of one dit_eval over `stacked` * B sequences."""
    T, t0 = max(lens), tail_t0(cfg, plens)
    return stacked * len(lens) * T, t0, stacked * len(lens) * (T - t0)


def synth_weights(cfg):
    """(numpy state dict for S2Mel, the same as fp32 torch tensors, the same as float64 torch tensors)"""
    w = weights.synth_s2mel_weights(cfg, tag=f"{TAG}/w")
    tw = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}
    return w, tw, {k: (v.double() if v.is_floating_point() else v) for k, v in tw.items()}


def _u(name, shape, scale=1.0):
    return torch.from_numpy(synth.uniform(f"{TAG}/{name}", shape, scale))


def solver_inputs(cfg, num, lens, plens):
    """z [B,C,T] (scale 1.7), mu [B,T,content] zero beyond each row's length, prompt [B,C,max(plens)], style [B,style]"""
    B, T = len(lens), max(lens)
    z = _u(f"s{num}/z", (B, cfg.in_channels, T), 1.7)
    mu = _u(f"s{num}/mu", (B, T, cfg.content_dim))
    prompt = _u(f"s{num}/prompt", (B, cfg.in_channels, max(plens)))
    style = _u(f"s{num}/style", (B, cfg.style_dim))
    for b in range(B):
        mu[b, lens[b]:] = 0
    return z, mu, prompt, style


def solver_oracle_rows(tw, cfg, lens, plens, inputs, dtype=torch.float32):
    """The oracle on each row ALONE, as the reference runs it (infer_v2 only ever has B = 1): a list of [C, lens[b]]."""
    z, mu, prompt, style = (t.to(dtype) for t in inputs)
    out = []
    for b, (Lb, Pb) in enumerate(zip(lens, plens)):
        out.append(osm.cfm_inference(tw, cfg, mu[b:b + 1, :Lb], torch.LongTensor([Lb]), prompt[b:b + 1, :, :Pb], style[b:b + 1],
                                     z[b:b + 1, :, :Lb], STEPS, CFG_RATE)[0])
    return out


def rows_inputs(cfg, num, plens, glens):
    """cfm_rows arguments: gen [B,Tg,content] zero beyond target_lens, prompt_conditions / ref_mels per row, style, z [B,C,T]"""
    B, Tg, T = len(plens), max(glens), max(p + g for p, g in zip(plens, glens))
    pcs = [_u(f"r{num}/pc{b}", (1, p, cfg.content_dim)) for b, p in enumerate(plens)]
    rms = [_u(f"r{num}/rm{b}", (1, cfg.in_channels, p)) for b, p in enumerate(plens)]
    gen = _u(f"r{num}/gen", (B, Tg, cfg.content_dim))
    for b in range(B):
        gen[b, glens[b]:] = 0
    return gen, pcs, rms, _u(f"r{num}/style", (B, cfg.style_dim)), _u(f"r{num}/z", (B, cfg.in_channels, T), 1.7)


def rows_oracle(tw, cfg, plens, glens, inputs, dtype=torch.float32):
    """Row b alone: cfm_inference(cat[prompt_condition, gen]) on Tp_b + Tg_b frames -> its generated frames [C, Tg_b]."""
    gen, pcs, rms, style, z = inputs
    out = []
    for b, (Tp, Tg) in enumerate(zip(plens, glens)):
        mu = torch.cat([pcs[b], gen[b:b + 1, :Tg]], dim=1).to(dtype)
        ref = osm.cfm_inference(tw, cfg, mu, torch.LongTensor([Tp + Tg]), rms[b].to(dtype), style[b:b + 1].to(dtype),
                                z[b:b + 1, :, :Tp + Tg].to(dtype), STEPS, CFG_RATE)
        out.append(ref[0, :, Tp:])
    return out


def estimator_inputs(cfg, T):
    """x, prompt_x (zero from ESTIMATOR_PROMPT on), lens [T, T - 31], style, cond for one DiT.forward on two rows"""
    x = _u(f"e{T}/x", (2, cfg.in_channels, T))
    px = _u(f"e{T}/prompt", (2, cfg.in_channels, T))
    px[..., ESTIMATOR_PROMPT:] = 0
    return x, px, [T, T - 31], _u(f"e{T}/style", (2, cfg.style_dim)), _u(f"e{T}/mu", (2, T, cfg.content_dim))


def estimator_oracle_rows(tw, cfg, inputs, dtype=torch.float32):
    """dit_forward on each row ALONE on its own frames (test_estimator_vs_reference_golden's comparison): a list of [C, lens[b]]."""
    x, px, lens, style, mu = inputs
    out = []
    for b, Lb in enumerate(lens):
        out.append(osm.dit_forward(tw, cfg, x[b:b + 1, :, :Lb].to(dtype), px[b:b + 1, :, :Lb].to(dtype), torch.LongTensor([Lb]),
                                   torch.tensor([ESTIMATOR_TIME], dtype=dtype), style[b:b + 1].to(dtype), mu[b:b + 1, :Lb].to(dtype))[0])
    return out


# ---- the solver's tail compaction restated from the oracle's own pieces (CPU only) ---------------------------------------------
def dit_forward_tail(w, cfg, x, prompt_x, x_lens, t, style, cond, t0: int):
    """dit_forward with everything after the transformer evaluated on the frames from t0 on alone, lengths x_lens - t0 (so the
    WaveNet's reflect padding sits at the cut): what dit_eval computes with tail_t0 = t0.  -> [N, C, T - t0]"""
    import torch.nn.functional as F
    e = "cfm.estimator"
    N, _, T = x.shape
    t1 = osm.t_embed(w, f"{e}.t_embedder", t)
    cond = osm._lin(w, f"{e}.cond_projection", cond)
    xt, pt = x.transpose(1, 2), prompt_x.transpose(1, 2)
    x_in = osm._lin(w, f"{e}.cond_x_merge_linear", torch.cat([xt, pt, cond, style[:, None, :].repeat(1, T, 1)], dim=-1))
    x_res = osm.dit_transformer(w, cfg, x_in, t1.unsqueeze(1), osm.sequence_mask(x_lens, T))
    x_res, xt = x_res[:, t0:], xt[:, t0:]
    mask_t = osm.sequence_mask(x_lens - t0, T - t0)
    x_res = osm._lin(w, f"{e}.skip_linear", torch.cat([x_res, xt], dim=-1))
    h = osm._lin(w, f"{e}.conv1", x_res).transpose(1, 2)
    t2 = osm.t_embed(w, f"{e}.t_embedder2", t)
    h = osm.wavenet(w, cfg, h, mask_t.unsqueeze(1), t2.unsqueeze(2)).transpose(1, 2) + osm._lin(w, f"{e}.res_projection", x_res)
    mod = osm._lin(w, f"{e}.final_layer.adaLN_modulation.1", F.silu(t1))
    shift, scale = mod.chunk(2, dim=1)
    h = F.layer_norm(h, (h.shape[-1],), None, None, 1e-6) * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)
    h = osm._lin(w, f"{e}.final_layer.linear", h).transpose(1, 2)
    return F.conv1d(h, osm._t(w, f"{e}.conv2.weight"), osm._t(w, f"{e}.conv2.bias"))


def cfm_tail_cut(w, cfg, mu, x_len: int, prompt, style, z, t0: int):
    """osm.cfm_inference for one row (B = 1, CFG stacked) with the estimate taken from dit_forward_tail(t0): the Euler update
    touches only the frames from t0 on, as cfm_euler does with v_t0 = t0."""
    x = z.clone()
    t_span = torch.linspace(0, 1, STEPS + 1, dtype=z.dtype)
    Tp = prompt.shape[-1]
    prompt_x = torch.zeros_like(x)
    prompt_x[..., :Tp] = prompt
    x[..., :Tp] = 0
    lens = torch.LongTensor([x_len, x_len])
    t = t_span[0]
    for step in range(1, STEPS + 1):
        dt = t_span[step] - t_span[step - 1]
        d = dit_forward_tail(w, cfg, torch.cat([x, x], 0), torch.cat([prompt_x, torch.zeros_like(prompt_x)], 0), lens,
                             torch.stack([t, t]), torch.cat([style, torch.zeros_like(style)], 0),
                             torch.cat([mu, torch.zeros_like(mu)], 0), t0)
        dphi, cfg_dphi = d.chunk(2, dim=0)
        x[..., t0:] = x[..., t0:] + dt * ((1.0 + CFG_RATE) * dphi - CFG_RATE * cfg_dphi)
        t = t + dt
        x[:, :, :Tp] = 0
    return x
