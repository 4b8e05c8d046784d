"""Cases of tests/test_vocoder_dispatch_gpu.py and tests/test_vocoder_dispatch_cpu.py: shapes at which the vocoder's kernels
(index-tts_amd/csrc/aa_act.hip, conv1d.hip, conv1d_bf16x3.hip, conv_epilogue.h, bigvgan.hip) switch tiles, store forms or
kernel instances, the host dispatch restated in Python, synthetic inputs and the oracle calls both files share.

What the host code decides, and from what:
  aa_act          tiles of AA_TILE = 1016 outputs, AA_TPW = 4 tiles per workgroup (4064); x halo 8, polyphase halo 4 each side
  conv_config     GEMM rows M (= Cout, or Cout * u for a transposed conv): > 96 -> 128 x 128, > 64 -> 96 x 256, > 32 -> 64 x 256,
                  else 32 x 512 (rows x time columns per workgroup); the same table in exact-fp32 and in split-bf16 mode
  epilogue_form   wide (quad transpose, 16-byte loads / stores): plain conv, T % 4 == 0, T >= 4, y / residual 16-byte aligned
  k1              split-bf16 mode compiles a separate instance of each configuration for 1-tap convolutions
  walk            split-bf16 mode: row blocks fastest (1) unless there is one row block or the weights are > 20 MB (0)
test_vocoder_dispatch_cpu.py reads every constant below back from the sources: if one moves, the tables must be re-derived."""
import numpy as np
import torch
import torch.nn.functional as F

from indextts_amd import synth, weights
from indextts_amd.config import BigVGANConfig
from oracle import vocoder as ov

TAG = "t/vocoder/dispatch"

# ---- the host dispatch, restated ------------------------------------------------------------------------------------------------
AA_TILE, AA_TPW, AA_XH, AA_VH = 1016, 4, 8, 4
AA_WG = AA_TILE * AA_TPW
CONV_MAX_HALO = 64
CONV_M_THRESHOLDS = (96, 64, 32)                                   # M > threshold, first match
CONV_CONFIGS = ((128, 128), (96, 256), (64, 256), (32, 512))      # (BM, BN)
CONV_WALK_BYTES = 20e6


def conv_config(M: int):
    """(BM, BN) of conv_tile_dispatch (conv1d.h: the one table of conv1d_forward and conv1d_bf16x3_forward) for M GEMM rows."""
    for thr, cfg in zip(CONV_M_THRESHOLDS, CONV_CONFIGS):
        if M > thr:
            return cfg
    return CONV_CONFIGS[-1]


def epilogue_form(T: int, transposed: bool = False, aligned: bool = True) -> str:
    """conv_epilogue's store form for rows of T GEMM columns."""
    return "wide" if (not transposed and T % 4 == 0 and T >= 4 and aligned) else "narrow"


def row_blocks(M: int) -> int:
    return -(-M // conv_config(M)[0])


def walk(M: int, Cin: int, K: int) -> int:
    """The bf16 kernels' tile walk, chosen in launch_conv16 of conv1d_bf16x3.hip (M, K as the GEMM sees them: a transposed conv has M = Cout * u rows and 3 taps)."""
    return 1 if row_blocks(M) > 1 and 4.0 * M * Cin * K <= CONV_WALK_BYTES else 0


def k1(K: int) -> bool:
    return K == 1


def time_tiles(M: int, T: int) -> int:
    return -(-T // conv_config(M)[1])


def aa_position(T_row: int):
    """Where a row of T_row samples ends relative to aa_act's tile (1016) and workgroup (4064) edges: a set of classes.
    edge: the last tile is full; edge+-1 / edge+-4 / edge+-8: one sample, one polyphase halo, one x halo off a tile edge."""
    out = set()
    if T_row <= 0:
        return out
    r = T_row % AA_TILE
    for d in (1, 4, 8):
        if r == d and T_row > AA_TILE:
            out.add(f"edge+{d}")
        if r == AA_TILE - d:
            out.add(f"edge-{d}")
    if r == 0:
        out.add("edge")
    if T_row % AA_WG == 0:
        out.add("wg_edge")
    if T_row % AA_WG == 1 and T_row > AA_WG:
        out.add("wg_edge+1")
    return out


AA_CLASSES = ("edge-1", "edge", "edge+1", "edge-4", "edge+4", "wg_edge", "wg_edge+1")
# a ragged row ends at lens[b] * 4, * 16, ... samples: always a multiple of 4, so only these classes can occur among row ends
AA_CLASSES_ROW_ENDS = ("edge", "edge-4", "edge+4", "wg_edge")

# ---- aa_act operator cases: (B, C, T) ----------------------------------------------------------------------------------------------
AA_CASES = [
    (1, 2, 1008),      # one x halo short of a full tile
    (1, 2, 1012),      # one polyphase halo short: the last vector of the tile is the row's last
    (1, 2, 1015),      # edge - 1: scalar stores, the tile's last output missing
    (1, 2, 1016),      # exactly one tile
    (1, 2, 1017),      # edge + 1: a second tile of one sample, all of its halo replicate padding
    (1, 2, 1020),      # edge + 4: a second tile of one vector
    (1, 2, 1024),      # edge + 8: the old tile size
    (1, 2, 2031),      # second tile one short
    (2, 2, 2032),      # two full tiles
    (1, 2, 2033),      # third tile of one sample
    (1, 2, 4060),      # workgroup one vector short
    (1, 2, 4063),      # workgroup edge - 1
    (2, 2, 4064),      # exactly one workgroup: no prefetch past the fourth tile
    (1, 2, 4065),      # a second workgroup for one sample
    (1, 2, 4068),      # a second workgroup for one vector
    (1, 1, 8128),      # two full workgroups
    (1, 1, 8129),      # a third workgroup for one sample
    (2, 3, 2033),      # odd T, C = 3, B = 2: row strides are no tile (or vector) multiples
]
# 16-bit tensors: the 4-wide store across a tile seam (T % 4 == 0) and the scalar store (1017)
AA16_T = [1016, 1020, 2032, 4064, 4068, 1017]
AA16_B, AA16_C = 2, 3


def aa_inputs(shape, amp: float = 4.0):
    """x [B,C,T] (uniform +-amp), log alpha [C], log beta [C]"""
    B, C, T = shape
    return (torch.from_numpy(synth.uniform(f"{TAG}/act/x/{shape}", shape, amp)),
            torch.from_numpy(synth.uniform(f"{TAG}/act/a/{shape}", (C,), 1.0)),
            torch.from_numpy(synth.uniform(f"{TAG}/act/b/{shape}", (C,), 1.0)))


# ---- conv operator cases: (B, Cin, Cout, K, dil, T) ------------------------------------------------------------------------------
def _bn(cout: int) -> int:
    return conv_config(cout)[1]


CONV_CASES = []      # (case, what it pins)


def _conv(case, note):
    CONV_CASES.append((case, note))


for _co in (32, 33, 64, 65, 96, 97, 128, 129):      # both sides of every M threshold, and of the 128-row block
    _conv((1, 18, _co, 3, 2, _bn(_co) + 1), "switch point: narrow form, the second time tile holds one column")
    _conv((1, 18, _co, 3, 2, _bn(_co) + 4), "switch point: wide form, the second time tile holds one vector")
for _co in (24, 48, 80, 160):                       # one Cout per configuration
    _conv((1, 7, _co, 3, 1, 1), "T = 1: every tap but one reads padding")
    _conv((2, 7, _co, 3, 1, 3), "T = 3: narrow, shorter than a vector")
    _conv((2, 7, _co, 3, 1, 4), "T = 4: the smallest wide row (tmax = 0)")
for _co in (24, 48, 96, 160):                       # 1-tap instances: 1, 2 and 3 K-steps against a prefetch distance of 2
    for _ci in (5, 32, 40):                         # (32: two full chunks, the only Cin here that is a multiple of 16)
        _conv((2, _ci, _co, 1, 1, _bn(_co) + 8), "K1 instance, wide, crosses a time tile")
        _conv((2, _ci, _co, 1, 1, _bn(_co) + 3), "K1 instance, narrow, crosses a time tile")
for _co in (24, 96):
    _conv((1, 18, _co, 5, 16, _bn(_co) + 5), "halo 64 = CONV_MAX_HALO, narrow")
    _conv((1, 18, _co, 9, 8, _bn(_co) + 4), "halo 64 = CONV_MAX_HALO, wide")
for _co in (80, 48, 24):
    _conv((1, 18, _co, 11, 5, _bn(_co) + 4), "halo 50 (the vocoder's widest) below 128 rows")
_conv((2, 768, 768, 11, 5, 130), "walk = 0 in a plain conv: 26 MB of weights, 6 row blocks x 2 time tiles per batch row")
CONV_HALO_OVER = (1, 18, 24, 6, 13, 40)             # (K - 1) * dil = 65: must raise
# wide-eligible shapes run on views one float into a larger buffer: (case, out unaligned, residual unaligned)
CONV_UNALIGNED = [((2, 18, 48, 3, 2, 260), True, True), ((2, 18, 160, 3, 2, 132), True, False), ((1, 18, 24, 3, 2, 516), False, True)]
SENTINEL = 12345.0

# transposed: (B, Cin, Cout, K, u, T); GEMM rows M = Cout * u, 3 taps
CONVT_CASES = [
    ((1, 96, 48, 8, 4, 130), "M = 192: two row blocks, the second half full; two time tiles"),
    ((1, 96, 48, 4, 2, 515), "M = 96: production's 96 -> 48 upsampler at the 96-row configuration, time tile 256"),
    ((1, 24, 12, 4, 2, 1030), "M = 24: 32-row configuration, time tile 512"),
    ((2, 40, 33, 8, 4, 130), "M = 132: the second row block holds 4 rows"),
    ((2, 18, 12, 8, 4, 259), "M = 48: 64-row configuration, a second time tile of 3 columns"),
    ((1, 96, 48, 8, 4, 1), "T = 1 at 128 rows"),
    ((1, 40, 24, 4, 2, 1), "T = 1 at the 64-row configuration"),
]


def conv_inputs(case, transposed: bool = False):
    """w, bias, x, residual, out (fp32 CPU tensors) of one case; `out` is what the accumulate form starts from."""
    B, Cin, Cout, K, d, T = case
    kind = "convt" if transposed else "conv"
    if transposed:
        w = synth.fan_in_uniform(f"{TAG}/{kind}/w/{case}", (Cin, Cout, K), Cin * K // d)
        To = T * d
    else:
        w = synth.fan_in_uniform(f"{TAG}/{kind}/w/{case}", (Cout, Cin, K), Cin * K)
        To = T
    b = synth.uniform(f"{TAG}/{kind}/b/{case}", (Cout,), 0.1)
    x = synth.uniform(f"{TAG}/{kind}/x/{case}", (B, Cin, T), 1.0)
    r = synth.uniform(f"{TAG}/{kind}/r/{case}", (B, Cout, To), 1.0)
    o = synth.uniform(f"{TAG}/{kind}/o/{case}", (B, Cout, To), 1.0)
    return tuple(torch.from_numpy(v) for v in (w, b, x, r, o))


def conv_reference(case, w, b, x, transposed: bool = False):
    """float64 F.conv1d / F.conv_transpose1d"""
    _, _, _, K, d, _ = case
    if transposed:
        return F.conv_transpose1d(x.double(), w.double(), b.double(), stride=d, padding=(K - d) // 2)
    return F.conv1d(x.double(), w.double(), b.double(), dilation=d, padding=(K - 1) * d // 2)


def conv_geometry(case, transposed: bool = False, aligned: bool = True):
    """(config, epilogue form, K1, walk, time tiles, row blocks) of one case"""
    _, Cin, Cout, K, d, T = case
    M, Kg = (Cout * d, 3) if transposed else (Cout, K)
    return conv_config(M), epilogue_form(T, transposed, aligned), k1(Kg), walk(M, Cin, Kg), time_tiles(M, T), row_blocks(M)


# ---- ragged whole-vocoder cases: (number, width, Tm, lens) ---------------------------------------------------------------------------
RAGGED_CASES = [
    # stage channels 192 / 96 / 48 / 24 / 12 / 6 / 3: every tile configuration under lens, the 96-row one included; Tm % 4 == 0 with
    # lengths 9, 1, 7 puts the row end inside a wide-form vector of conv_pre; one row is empty
    (1, 192, 12, [12, 9, 1, 7, 0]),
    # row ends 1020 / 1016 / 1012 at stage 1, 127 frames -> 2032 (tile edge) at stage 2 and 4064 (workgroup edge) at stage 3
    (2, 64, 255, [255, 254, 253, 127, 1]),
]
RAGGED_FULL = (3, 1536, 6, [6, 3, 5])      # the walk = 0 layers and the widest tiles under lens (reference: the solo call per row)
RAGGED_ORACLE_ATOL = 2e-5                   # x TOL x max(1, |ref|max): tests/test_vocoder_gpu.py::test_bigvgan_vs_oracle_mid_width


def ragged_config(width: int):
    return BigVGANConfig() if width == BigVGANConfig().upsample_initial_channel else BigVGANConfig.tiny(width)


def ragged_weights(width: int):
    cfg = ragged_config(width)
    return cfg, weights.synth_bigvgan_weights(cfg, tag=f"{TAG}/bigvgan/{width}")


def ragged_mel(num: int, cfg, B: int, Tm: int, what: str = "mel"):
    return torch.from_numpy(weights.synth_mel(f"{TAG}/ragged{num}/{what}", B, cfg.num_mels, Tm))


def stage_row_ends(cfg, n: int):
    """samples of an n-frame row after each up-sampling stage: where aa_act's ragged kernel meets the row's own end"""
    out, mul = [], 1
    for u in cfg.upsample_rates:
        mul *= u
        out.append(n * mul)
    return out


def ragged_oracle_rows(w, cfg, mel, lens, dtype=torch.float64):
    """The oracle on each row ALONE on its own frames, unclamped: a list of [1, lens[b] * 256] (None for an empty row)."""
    tw = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in w.items()}
    return [ov.bigvgan_forward(tw, cfg, mel[b:b + 1, :, :n].to(dtype), clamp=False)[0] if n > 0 else None
            for b, n in enumerate(lens)]
