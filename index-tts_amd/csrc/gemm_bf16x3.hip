// Token-major GEMM on the bf16 matrix core with fp32-class accuracy ("split-bf16", 3 products).
//
// Same contract as gemm.hip (Y = epi(X W^T + b), conv taps, paired gates, row masks) for the compute-bound
// shapes of the hot path: the s2mel DiT / WaveNet linears and convolutions (diffusion_transformer.py:213-252,
// gpt_fast/model.py:270-319, wavenet.py:149-161) and the GPT latent pass (model_v2.py:673-723).
//
// Why: gfx950 has no TF32/xf32; its f32-input MFMA runs at the VALU rate (157 TFLOP/s) while
// v_mfma_f32_32x32x16_bf16 runs 16x faster.  Every fp32 operand is written as hi + lo with hi = bf16(x),
// lo = bf16(x - hi) (16 significant bits), and x*w ~= hi*hi' + hi*lo' + lo*hi' is accumulated in the fp32
// accumulator: three bf16 MFMAs per product = 5.3x the f32 MFMA rate at a relative product error of ~2^-16
// (vs 2^-24 for fp32), far inside the path's stated tolerance (mel L1 <= 1e-3) -- measured in the parity tests.
// The KV-cached greedy decode stays on exact-fp32 kernels (token indices must be bit-exact).
//
// Structure: one kernel template, (64 WM) x (64 TN) tile / 128 WM threads (WM x 2 waves, 2 x TN tiles of 32x32 per wave), K stepped
// 32 at a time: 128 x 128, and 256 x 128 / 256 x 256 from 4096 rows up.  It runs the shapes the LDS-DMA kernel (gemm_bf16x3_v2.hip)
// does not take.  Its weights (LinearWeights::tiles16) are split and laid out at context creation exactly as the LDS image
// ([hl][128 rows][32 k + 8 pad] bf16, 20 KiB per (128-column block, k-step)): their tile load is a linear 16-B/lane copy.  Activations
// are fp32 in HBM; the tile loader converts them to hi/lo on the way into LDS (v_cvt_pk_bf16_f32).  80-byte LDS rows make every
// ds_read_b128 fragment read conflict-free (rows r and r+4 of an unpadded 64-byte row would share banks).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gemm_common.h"
#include "prof.h"

namespace idxtts {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int BROW = 40;                       // bf16 elements per LDS row (32 + 8 pad) = 80 bytes
constexpr int TILE_HALF = 128 * BROW;          // elements of one [128][40] image (hi or lo)
constexpr int WTILE_BYTES = 2 * TILE_HALF * 2; // 20480 bytes per packed (n-block, k-step) weight tile

size_t linear_tiles_bytes(int N, int K) { return (size_t)cdiv(N, 128) * cdiv(K, 32) * WTILE_BYTES; }

// w: [N][K] fp32 -> [N/128][K/32][hl][128][40] bf16
void pack_linear_tiles(void* dst, const float* w, int N, int K) {
  uint16_t* o = static_cast<uint16_t*>(dst);
  const int NB = cdiv(N, 128), KS = cdiv(K, 32);
  std::memset(o, 0, linear_tiles_bytes(N, K));
  for (int nb = 0; nb < NB; ++nb)
    for (int ks = 0; ks < KS; ++ks) {
      uint16_t* tile = o + ((size_t)nb * KS + ks) * (2 * TILE_HALF);
      for (int r = 0; r < 128; ++r) {
        const int n = nb * 128 + r;
        if (n >= N) break;
        for (int kk = 0; kk < 32; ++kk) {
          const int k = ks * 32 + kk;
          if (k >= K) break;
          const float x = w[(size_t)n * K + k];
          const uint16_t hi = f2bf(x);
          tile[r * BROW + kk] = hi;
          tile[TILE_HALF + r * BROW + kk] = f2bf(x - bf2f(hi));
        }
      }
    }
}

// Workgroup tile (64 WM) x (64 TN), 128 WM threads = WM (M) x 2 (N) waves, wave tile 64 x (32 TN).  <2, 2>: 128 x 128.  From 4096 rows
// up <4, 2> and <4, 4>: the 128 x 128 tile needs 48 B/clk/CU of operand traffic at the bf16 MFMA rate (measured: a CU sustains ~13, L2
// hit rate 66 %); doubling the rows a weight tile is applied to halves the weight traffic per flop and doubles the MFMA work per
// barrier (one workgroup per CU, two waves per SIMD).  All three add a row's 32-k steps in the same MFMA order: the same sum, bit for bit.
// SEQB: the per-sequence-bias epilogue (GemmArgs::ld_bias), kernels of their own beside the ones every other launch runs.
template <int WM /* waves along M: 2 or 4 */, int TN /* 32-column MFMA tiles per wave: 2 or 4 */, bool SEQB>
__device__ __forceinline__ void gemm_bf16x3_tile(const GemmKP& p) {
  constexpr int NT = 128 * WM, BM = 64 * WM, BN = 64 * TN;      // threads, rows and columns per workgroup
  constexpr int NB128 = BN / 128;             // packed 128-column weight tiles per k-step
  constexpr int A_HALF = BM * BROW;           // elements of one [BM][40] activation image
  constexpr int B_HALF = TILE_HALF;           // [128][40] per packed weight tile (hi or lo)
  constexpr int A_STAGE = 2 * A_HALF, B_STAGE = NB128 * 2 * B_HALF;
  constexpr int NXL = BM * 8 / NT;            // 16-byte activation loads per thread per k-step (4)
  constexpr int NWL = (NB128 * 1280 + NT - 1) / NT;      // 16-byte weight loads per thread per k-step
  constexpr bool W_WHOLE = NB128 == 1 && NWL * NT == 1280;      // <2, 2>: ... exactly the block's one weight tile, which always exists
  static_assert((WM == 2 || WM == 4) && (TN == 2 || TN == 4), "tile");
  extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
  __bf16* As = sm16;                          // [2][hl][BM][40]
  __bf16* Bs = sm16 + 2 * A_STAGE;            // [2][NB128][hl][128][40]

  int bn, bm;
  if (!gemm_tile_walk(p, blockIdx.x, bm, bn)) return;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = lane >> 5, j = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int ksteps = (p.K + 31) >> 5;

  f32x4 xr[NXL];
  f32x4 wr[NWL];
  ConvRow xrow[NXL];
#pragma unroll
  for (int l = 0; l < NXL; ++l) xrow[l] = conv_row(p, bm * BM + ((tid + NT * l) >> 3));
  const int n128 = cdiv(p.N, 128);
  auto load_tiles = [&](int kstep) {
    const KStep ks = gemm_kstep(p, kstep);
#pragma unroll
    for (int l = 0; l < NXL; ++l) {
      const int idx = tid + NT * l;
      xr[l] = gemm_load_x(p, xrow[l], bm * BM + (idx >> 3), ks, idx & 7);
    }
#pragma unroll
    for (int l = 0; l < NWL; ++l) {
      const int idx = tid + NT * l;                  // 16-byte unit inside this k-step's weight tiles
      const int sub = W_WHOLE ? 0 : idx / 1280, off = idx - sub * 1280;
      const int nb = bn * NB128 + sub;      // (the second 128-column tile of a 256-column block may not exist)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (W_WHOLE || (idx < NB128 * 1280 && nb < n128))
        v = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.wp) + ((size_t)nb * ksteps + kstep) * WTILE_BYTES)[off];
      wr[l] = v;
    }
  };
  auto store_tiles = [&](int buf) {
    __bf16* a_hi = As + buf * A_STAGE;
    __bf16* a_lo = a_hi + A_HALF;
#pragma unroll
    for (int l = 0; l < NXL; ++l) {
      const int idx = tid + NT * l;
      const int row = idx >> 3, q8 = idx & 7;
      const bf16x4 hi = __builtin_convertvector(xr[l], bf16x4);
      const f32x4 back = __builtin_convertvector(hi, f32x4);
      const bf16x4 lo = __builtin_convertvector(xr[l] - back, bf16x4);
      *reinterpret_cast<bf16x4*>(a_hi + row * BROW + q8 * 4) = hi;
      *reinterpret_cast<bf16x4*>(a_lo + row * BROW + q8 * 4) = lo;
    }
    f32x4* wdst = reinterpret_cast<f32x4*>(Bs + buf * B_STAGE);
#pragma unroll
    for (int l = 0; l < NWL; ++l) {
      const int idx = tid + NT * l;
      if (W_WHOLE || idx < NB128 * 1280) wdst[idx] = wr[l];
    }
  };

  f32x16 acc[2][TN];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  for (int ks = 0; ks < ksteps; ++ks) {
    const bool has_next = ks + 1 < ksteps;
    if (has_next) load_tiles(ks + 1);
    const __bf16* a_hi = As + (ks & 1) * A_STAGE;
    const __bf16* b_st = Bs + (ks & 1) * B_STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[2], al[2], bh[TN], bl[TN];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ar = (wm * 64 + t * 32 + j) * BROW + s * 16 + h * 8;
        ah[t] = *reinterpret_cast<const bf16x8*>(a_hi + ar);
        al[t] = *reinterpret_cast<const bf16x8*>(a_hi + A_HALF + ar);
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const int col = wn * 32 * TN + t * 32 + j;                 // column inside the workgroup tile
        const __bf16* bt = b_st + (col >> 7) * 2 * B_HALF + (col & 127) * BROW + s * 16 + h * 8;
        bh[t] = *reinterpret_cast<const bf16x8*>(bt);
        bl[t] = *reinterpret_cast<const bf16x8*>(bt + B_HALF);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    if (has_next) store_tiles((ks + 1) & 1);
    __syncthreads();
  }
  gemm_epilogue_t<2, TN, SEQB>(p, acc, bm * BM + wm * 64, bn * BN + wn * 32 * TN, h, j);
}

template <int WM, int TN> __global__ __launch_bounds__(128 * WM) void gemm_bf16x3_tile_kernel(const GemmKP p) { gemm_bf16x3_tile<WM, TN, false>(p); }
template <int WM, int TN> __global__ __launch_bounds__(128 * WM) void gemm_bf16x3_tile_seqbias_kernel(const GemmKP p) { gemm_bf16x3_tile<WM, TN, true>(p); }

template <int WM, int TN>
static int launch_tile(GemmKP p, const LinearWeights& w, const GemmArgs& a, hipStream_t stream, double flops, double bytes) {
  constexpr int BM = 64 * WM, BN = 64 * TN, NB128 = BN / 128;
  p.mtiles = cdiv(a.M, BM);
  p.mt8 = cdiv(p.mtiles, 8);
  p.nblocks = cdiv(w.N, BN);
  const int64_t grid = (int64_t)8 * p.nblocks * p.mt8;
  IDX_CHECK(grid < (1ll << 31), "grid size");
  constexpr size_t lds = (size_t)(2 * 2 * BM * BROW + 2 * NB128 * 2 * TILE_HALF) * sizeof(__bf16);
  static DynLdsLimit lds_limit;
  if (p.ld_bias) {      // paired activations only (gemm_prepare): <2, 2> and <4, 2>
    if constexpr (TN == 2) {
      static DynLdsLimit lds_limit_sb;
      IDX_HIP(lds_limit_sb.set((int)lds, gemm_bf16x3_tile_seqbias_kernel<WM, TN>));
      static const int cat_sb = prof_register(WM == 2 ? "gemm_bf16x3_seqbias_kernel" : "gemm_bf16x3_big_seqbias_kernel<2>");
      ProfScope prof(cat_sb, stream, flops, bytes);
      hipLaunchKernelGGL((gemm_bf16x3_tile_seqbias_kernel<WM, TN>), dim3((unsigned)grid), dim3(128 * WM), lds, stream, p);
      IDX_LAUNCH_CHECK();
      return 0;
    }
    IDX_FAIL("a per-sequence bias on an unpaired tile");
  }
  IDX_HIP(lds_limit.set((int)lds, gemm_bf16x3_tile_kernel<WM, TN>));
  // (the profile categories keep the names the three kernels had as two: committed profiles and tools read them)
  static const int cat = prof_register(WM == 2 ? "gemm_bf16x3_kernel" : TN == 2 ? "gemm_bf16x3_big_kernel<2>" : "gemm_bf16x3_big_kernel<4>");
  ProfScope prof(cat, stream, flops, bytes);
  hipLaunchKernelGGL((gemm_bf16x3_tile_kernel<WM, TN>), dim3((unsigned)grid), dim3(128 * WM), lds, stream, p);
  IDX_LAUNCH_CHECK();
  return 0;
}

int gemm_bf16x3_forward(const LinearWeights& w, const GemmArgs& a, hipStream_t stream) {
  IDX_CHECK((a.x || a.x_planes) && (a.y || a.y_planes), "null pointer");
  if (a.M == 0) return 0;
  const bool v2 = gemm_bf16x3_uses_v2(w, a);
  if (a.x_planes || a.y_planes || !a.x || !a.y || a.rope) IDX_CHECK(v2, "operand planes are only understood by the LDS-DMA kernel (shape not eligible)");
  IDX_CHECK(v2 ? w.planes16 : w.tiles16, "the split-bf16 weight pack this launch reads was not made (model_util.h: make_linear)");
  IDX_CHECK(a.ksplit <= 1, "split-K is a feature of the exact-fp32 kernel");
  GemmKP p;
  double flops, bytes;
  if (gemm_prepare(w, a, &p, &flops, &bytes)) return 1;
  if (v2) return gemm_bf16x3_v2_forward(p, w, a, stream, flops, bytes);
  p.wp = static_cast<const float*>(w.tiles16);
  if (a.M < 4096) return launch_tile<2, 2>(p, w, a, stream, flops, bytes);
  const bool paired = a.act == ACT_SWIGLU || a.act == ACT_GATE;
  if (w.N >= 256 && !paired) return launch_tile<4, 4>(p, w, a, stream, flops, bytes);
  return launch_tile<4, 2>(p, w, a, stream, flops, bytes);
}

}  // namespace idxtts
