// Decode-step skinny GEMM: Y[rows <= 64][N] = epi(LN?(X)[rows][K] . W[K][N]), one HBM pass over the weights, no split-K
// slabs, no LayerNorm launch, no prologue.  Replaces, per generated token, the Conv1D projections of every GPT-2 block
// (transformers_gpt2.py:304-355, 578-592), the LayerNorms in front of c_attn / c_fc (615-674) and the residual adds
// behind c_proj / mlp.c_proj: 5 launches per layer (c_attn, attention, c_proj, c_fc, mlp.c_proj).
//
// What bounds it (tools/stream_probe.hip, tools/gemv_probe.hip on MI355X): a cold 26 MB weight stream alone takes 5.9 us
// (4.5 TB/s) when >= ~256 waves x 5 KiB are in flight; everything else in the kernel is a chain of dependent
// L2 / LDS round trips (~1-2 us each), so the kernel is built to have as few of those as possible:
//   * activations live in HBM as MFMA A-fragment images ([rows/16][K/16][64 lanes][4], frag_index() in common.h): the
//     activation fragment of a 16-k chunk is ONE contiguous 1 KiB load (8 full cache lines), exactly like the weight
//     fragment (packed [N/16][K/16][64][4] for v_mfma_f32_16x16x4_f32), and both are issued together;
//   * a wave owns a K-slice for NTW adjacent column tiles, so one activation fragment feeds NTW weight fragments
//     (L2->L1 activation traffic = weight traffic / NTW);
//   * LayerNorm is folded algebraically: with W' = diag(g) W, u = colsum(W'), c = b.W + bias (precomputed at load),
//         LN(x) . W + bias = rstd * (x . W' - mean * u) + c
//     so the matrix product runs on the RAW residual stream while the row statistics are accumulated from the very
//     fragments the MFMAs consume (shifted sums per wave, Chan's pairwise update across the K-slices in a fixed order:
//     as accurate as the two-pass form, bitwise reproducible);
//   * the K-slices of the 16 waves of a workgroup are reduced through LDS in a fixed order; bias / colsum / residual
//     operands of the epilogue are fetched at kernel entry.
#include <algorithm>
#include <atomic>

#include "device_util.h"
#include "gemv16.h"
#include "prof.h"

namespace idxtts {

// Ablation masks of tools/gemv_probe.hip (built with -DGEMV_PROBE); the product build compiles every probe branch out.
#ifdef GEMV_PROBE
#define FX_DBG(mask) (p.dbg & (mask))
#else
#define FX_DBG(mask) false
#endif

struct GemvFXP {
  const float* xf;          // A-fragment images [MT][kc16][64][4]
  const void* wp;           // packed weights [ntiles][kc16][64][4] elements of the WT format
  const float* wscale;      // fp8: [N] power-of-two column scales (null otherwise)
  const float* bias;        // [N] or null (LN-folded layers: c = b.W + bias)
  const float* colsum;      // [N] LN-folded layers: u = colsum(diag(g) W); null = plain GEMV
  float ln_eps;
  const float* res;         // residual, same layout as y, may alias y
  float* y; int y_frag; int ldy;   // y_frag: fragment images with kc16 = N/16 (N % 16 == 0), else row-major [rows][ldy]
  int rows, N, K, kc16, ntiles, kw, cps, act;
  int ksb;                  // > 1: K also split across gridDim.y workgroups
  float* slab;              // K-split: partial sums [ksb][rows][N]; the last workgroup of a column tile finishes the job
  unsigned* cnt;            // K-split: [gridDim.x] arrival counters (0 on entry and on exit); null with ksb == 1
  int dbg;
};

__device__ __forceinline__ float gelu_new_fx(float v) {
  const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
  return 0.5f * v * (1.0f + tanhf(u));
}

// UN = chunks per register batch (two batches live: the next one is in flight while the current one is multiplied)
// SINGLE: the whole K-slice of a wave fits one register batch (every GPT-2 decode shape: K / 16 waves = 5 chunks, the long
// K of mlp.c_proj is split across workgroups): no second register set, which keeps the 16-row kernels at <= 64 VGPRs so
// TWO 1024-thread workgroups fit a CU (8 waves per SIMD) and a 320-tile layer runs in one round.
template <int MT, int NTW, bool SINGLE>
struct FXCfg { static constexpr int UN = SINGLE ? 5 : ((MT + NTW == 2) ? 5 : (NTW == 2 ? 3 : (MT == 2 ? 2 : 1))); };

// What one lane reads of a 16-k weight chunk (4 weights) in each storage format, and how it widens to fp32 (exact)
template <int WT> struct WRaw;
template <> struct WRaw<WFMT_F32> {
  typedef f32x4 raw;
  static __device__ __forceinline__ raw zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f32x4 widen(raw r) { return r; }
};
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
template <> struct WRaw<WFMT_BF16> {
  typedef u32x2_t raw;
  static __device__ __forceinline__ raw zero() { return raw{0u, 0u}; }
  static __device__ __forceinline__ f32x4 widen(raw r) {
    return f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
  }
};
template <> struct WRaw<WFMT_FP8> {
  typedef uint32_t raw;
  static __device__ __forceinline__ raw zero() { return 0u; }
  static __device__ __forceinline__ f32x4 widen(raw r) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r, true);
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  }
};

// R4 (rows <= 4, MT == 1): the 16-block v_mfma_f32_4x4x1_16B_f32 instead of 16x16x4 -- a quarter of the MFMA cycles for the
// same exact fp32 products.  Block b = lane >> 2 multiplies x[row r][k = 4 (b >> 2) + s] (lane 4 b + r) by
// w[k][n = 4 (b & 3) + c] (lane 4 b + c): the weight stream is read as it is, the activation fragment is read from the lane
// that holds row (lane & 3), and the accumulator ends up as the 16x16 C layout with the four k-groups (lane >> 4) still to add.
// UNS: chunks of the one-batch form.  5 = a K-slice per wave of 16 waves (1024 threads, <= 64 VGPRs: 256 registers per SIMD); 10 = the
// NARROW geometry: 8 waves (512 threads) of 10 chunks each at <= 88 VGPRs -- 176 registers per SIMD, what ONE retiring workgroup of the
// acoustic stage's GEMM / convolution / attention kernels (168 x 1 wave per SIMD) frees on a CU, so a decode launch beside them does
// not have to wait until two of a CU's three workgroups have gone.
template <int MT, int NTW, bool SINGLE, int WT, bool R4, int UNS = 5>
__global__ __launch_bounds__(UNS == 10 ? 512 : 1024) void gemv_fx_kernel(const GemvFXP p) {
  static_assert(!R4 || MT == 1, "the 4-row form has one row tile");
  typedef typename WRaw<WT>::raw wraw_t;
  if (FX_DBG(8)) return;      // tools/gemv_probe.hip: launch + dispatch cost of this geometry alone
  constexpr int UN = SINGLE ? UNS : FXCfg<MT, NTW, SINGLE>::UN;
  constexpr int NB = SINGLE ? 1 : 2;
  constexpr int NACC = MT * NTW;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* redbuf = sm;                               // [kw][NACC][256]
  float* wstat = sm + p.kw * NACC * 256;            // [kw][MT*16][2]  per K-slice: mean, M2 (count is known)

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nt0 = blockIdx.x * NTW;
  const int c0 = (blockIdx.y * p.kw + wave) * p.cps;
  const int nch = max(0, min(p.cps, p.kc16 - c0));
  const bool ln = p.colsum != nullptr;

  // ---- epilogue operands of this thread's output element, fetched up front ----
  // element e = tid (< NACC*256): r = e & 3, ln16 = (e >> 2) & 63, t = e >> 8 -> (mt, ntw) = (t / NTW, t % NTW)
  const int e_r = tid & 3, e_ln = (tid >> 2) & 63, e_t = tid >> 8;
  const int e_mt = e_t / NTW, e_ntw = e_t - e_mt * NTW;
  const int e_row = e_mt * 16 + (e_ln >> 4) * 4 + e_r, e_col = (nt0 + e_ntw) * 16 + (e_ln & 15);
  const bool e_ok = e_t < NACC && e_row < p.rows && e_col < p.N;
  size_t e_addr = 0;
  float e_bias = 0.f, e_u = 0.f, e_res = 0.f, e_s = 1.f;
  if (e_ok) {
    if (WT == WFMT_FP8) e_s = p.wscale[e_col];
    e_addr = p.y_frag ? frag_index(e_row, e_col, p.N >> 4) : (size_t)e_row * p.ldy + e_col;
    // (never taken: the launcher sets cnt whenever ksb > 1.  The select stays because register allocation and instruction order of
    // every instantiation change without it, which this kernel's measured figures do not cover.)
    if (p.ksb > 1 && !p.cnt) e_addr = ((size_t)blockIdx.y * p.rows + e_row) * p.N + e_col;
    if (p.bias) e_bias = p.bias[e_col];
    if (ln) e_u = p.colsum[e_col];
    if (p.res) e_res = p.res[e_addr];
  }

  // ---- K loop ----
  f32x4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Every load of a batch is issued unconditionally, at a clamped chunk index; chunks past this wave's slice are zeroed on the
  // ACTIVATION side when they are consumed.  (A per-element "load or zero" made the compiler branch around each load, and one of
  // the merges became a register copy behind an s_waitcnt vmcnt(0) in the middle of the batch: the last three loads of five were
  // issued only after the first two had come back.)
  const int c0c = min(c0, p.kc16 - 1), last = max(nch - 1, 0);
  const wraw_t* wbase[NTW];      // one raw element = this lane's 4 weights of a chunk; 64 per chunk
#pragma unroll
  for (int j = 0; j < NTW; ++j) wbase[j] = static_cast<const wraw_t*>(p.wp) + ((size_t)min(nt0 + j, p.ntiles - 1) * p.kc16 + c0c) * 64 + lane;
  const float* xbase = p.xf + (size_t)c0c * 256 + (R4 ? ((lane & 48) | (lane & 3)) : lane) * 4;
  const size_t ximg = (size_t)p.kc16 * 256;

  wraw_t wq[NB][UN][NTW];
  f32x4 xq[NB][UN][MT];
  auto load_batch = [&](int buf, int cb) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const size_t idx = (size_t)min(cb + u, last);
#pragma unroll
      for (int j = 0; j < NTW; ++j) wq[buf][u][j] = __builtin_nontemporal_load(wbase[j] + idx * 64);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[buf][u][mt] = *reinterpret_cast<const f32x4*>(xbase + mt * ximg + idx * 256);
    }
  };
  // shifted row sums for the folded LayerNorm: this lane holds row (lane & 15) of every fragment
  float shift[MT], s1[MT], s2[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) shift[mt] = s1[mt] = s2[mt] = 0.f;

  load_batch(0, 0);
  if (ln) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) shift[mt] = __shfl(xq[0][0][mt][0], lane & 15);   // a sample of the row as the shift
  }
  auto consume = [&](int buf, int cb) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (!(cb + u < nch) || FX_DBG(1)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xq[buf][u][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (ln && cb + u < nch) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float dlt = xq[buf][u][mt][s] - shift[mt];
            s1[mt] += dlt;
            s2[mt] += dlt * dlt;
          }
      }
      f32x4 wf[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) wf[j] = WRaw<WT>::widen(wq[buf][u][j]);
      if (FX_DBG(2)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < NTW; ++j) acc[mt][j] += xq[buf][u][mt] * wf[j];
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < NTW; ++j)
              acc[mt][j] = R4 ? __builtin_amdgcn_mfma_f32_4x4x1f32(xq[buf][u][mt][s], wf[j][s], acc[mt][j], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_16x16x4f32(xq[buf][u][mt][s], wf[j][s], acc[mt][j], 0, 0, 0);
      }
    }
  };
  if constexpr (SINGLE) {
    consume(0, 0);
  } else {
    for (int cb = 0; cb < nch; cb += 2 * UN) {
      if (cb + UN < nch) load_batch(NB - 1, cb + UN);
      consume(0, cb);
      if (cb + UN < nch) {
        if (cb + 2 * UN < nch) load_batch(0, cb + 2 * UN);
        consume(NB - 1, cb + UN);
      }
    }
  }

  if (FX_DBG(4)) {
    if (acc[0][0][0] == 123.456f) p.y[tid] = acc[0][0][1];
    return;
  }
  if constexpr (R4) {      // add the four k-groups; lanes 0-15 then hold rows 0-3 exactly where the 16x16 layout has them
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[0][j][r];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        acc[0][j][r] = lane < 16 ? v : 0.f;
      }
  }

  // ---- per-slice partial results to LDS (waves beyond kw exist only as epilogue threads) ----
  const bool kwave = wave < p.kw;
  if (kwave)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) *reinterpret_cast<f32x4*>(&redbuf[((wave * NACC + mt * NTW + j) * 64 + lane) * 4]) = acc[mt][j];
  if (ln && kwave && !FX_DBG(16)) {
    // the four lane groups (lane >> 4) hold disjoint k of the same row: fold them, then slice mean / M2 about the mean
    const float cnt = 16.0f * nch;    // K-slice elements per row (padded chunks excluded: K % 16 == 0 for folded layers)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float a = s1[mt], b = s2[mt];
      a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);
      a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
      if (lane < 16) {
        const float mean_w = nch > 0 ? shift[mt] + a / cnt : 0.f;
        const float m2_w = nch > 0 ? b - a * a / cnt : 0.f;
        wstat[(wave * MT * 16 + mt * 16 + lane) * 2 + 0] = mean_w;
        wstat[(wave * MT * 16 + mt * 16 + lane) * 2 + 1] = m2_w;
      }
    }
  }
  __syncthreads();
  // Row statistics of the folded LayerNorm, combined per WAVE for the 4 rows its 64 epilogue threads own (no serial pass, no
  // second barrier): lane j holds K-slice (j >> 2) of its own row (row = ... + (j & 3), see e_row), an xor butterfly over the
  // slice bits adds them -- the same tree in every lane, so all lanes of a row agree bit for bit -- with the exact identity
  //   mean = sum_w n_w mean_w / n,   M2 = sum_w M2_w + sum_w n_w (mean_w - mean)^2
  float ln_mean = 0.f, ln_rstd = 0.f;
  if (ln && e_t < NACC && !FX_DBG(32)) {      // wave-uniform (e_t = tid >> 8); rows beyond p.rows are zero padding: harmless
    const int sl = lane >> 2;
    const bool on = sl < p.kw;
    const float nw = on ? 16.0f * max(0, min(p.cps, p.kc16 - sl * p.cps)) : 0.f;      // (folded LayerNorm implies ksb == 1)
    const int srow = e_mt * 16 + (e_ln >> 4) * 4 + e_r;
    const float2 st = on ? *reinterpret_cast<const float2*>(&wstat[(sl * MT * 16 + srow) * 2]) : make_float2(0.f, 0.f);
    float n = nw, a = nw * st.x;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) { n += __shfl_xor(n, m); a += __shfl_xor(a, m); }
    ln_mean = a / n;
    const float dlt = st.x - ln_mean;
    float m2 = st.y + nw * dlt * dlt;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) m2 += __shfl_xor(m2, m);
    ln_rstd = rsqrtf(m2 / n + p.ln_eps);
  }

  // ---- fixed-order reduction over the K-slices and the epilogue: one output element per thread ----
  if (p.ksb > 1 && p.cnt) {
    // K split across workgroups, finished by whichever of them arrives last (wait-free: nobody spins).  Partial sums travel
    // through agent-scope atomics (coherent across the XCDs' L2s); the sum runs in slab order, so the result does not depend
    // on who is last.
    if (e_ok) {
      float v = 0.f;
      for (int w = 0; w < p.kw; ++w) v += redbuf[(w * NACC + e_t) * 256 + (tid & 255)];
      if (WT == WFMT_FP8) v *= e_s;
      __hip_atomic_store(&p.slab[((size_t)blockIdx.y * p.rows + e_row) * p.N + e_col], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!wg_arrive_last(&p.cnt[blockIdx.x], (unsigned)p.ksb) || !e_ok) return;
    float t[8];      // all partial sums in ONE round trip (a loop of atomic loads is issued one after the other)
#pragma unroll
    for (int s = 0; s < 8; ++s)
      t[s] = s < p.ksb ? __hip_atomic_load(&p.slab[((size_t)s * p.rows + e_row) * p.N + e_col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    float v = p.res ? e_res : 0.f;
    v += e_bias;
#pragma unroll
    for (int s = 0; s < 8; ++s) v += t[s];
    p.y[e_addr] = v;
    return;
  }
  if (e_t < NACC) {
    float v = 0.f;
    for (int w = 0; w < p.kw; ++w) v += redbuf[(w * NACC + e_t) * 256 + (tid & 255)];
    if (e_ok) {
      if (WT == WFMT_FP8) v *= e_s;        // power-of-two column scale: exact
      if (ln) v = ln_rstd * (v - ln_mean * e_u);
      v += e_bias;
      if (p.act == 1) v = gelu_new_fx(v);
      if (p.res) v += e_res;
      p.y[e_addr] = v;
    }
  }
}


// ---- host side ----
// Narrow layers (N = d: 80 column tiles) with a long K (mlp.c_proj: 26 MB) cannot reach HBM speed from 80 workgroups:
// a CU sustains ~11 B/clk from HBM (tools/l2_probe.hip), so all 256 have to stream.  Their K is split across `ksb`
// workgroups per column tile; the partial sums go to a [ksb][rows][N] slab and the last workgroup of a column tile to arrive
// adds them in a fixed order (bitwise reproducible) together with bias and residual.
int gemv_fx_ksb(int N, int K) {
  const int ntiles = cdiv(N, 16), kc16 = cdiv(K, 16);
  return (ntiles <= 128 && kc16 >= 64) ? 4 : 1;
}

// Process-wide geometry of the 5..16-row decode GEMVs on compact weight streams (include/idxtts.h::idxtts_set_decode_geometry).
static std::atomic<int> g_decode_narrow{0};
void set_decode_geometry(int narrow) { g_decode_narrow.store(narrow ? 1 : 0); }
int get_decode_geometry() { return g_decode_narrow.load(); }

FxPlan gemv_fx_make_plan(int N, int K, int rows, int fmt, int ksb, bool narrow_geom, bool invariant) {
  if (invariant) narrow_geom = false;
  const int kc16 = cdiv(K, 16), ntiles = cdiv(N, 16);
  FxPlan pl;
  pl.MT = cdiv(rows, 16);
  pl.r4 = rows <= 4 && !invariant;
  // The narrow geometry: 5..16 rows on a compact stream whose K gives each of 8 waves exactly 10 chunks (d = 1280, and 4 d split
  // over 4 workgroups); fp32 streams and every other shape keep the 16-wave form.
  pl.narrow = narrow_geom && pl.MT == 1 && rows > 4 && fmt != WFMT_F32 && kc16 % 80 == 0 && cdiv(kc16, 8 * ksb) == 10;
  if (pl.narrow) {
    pl.kw = 8; pl.ntw = 1;
  } else {
    pl.kw = 16;
    while (pl.kw > 1 && kc16 < pl.kw) pl.kw >>= 1;
    // Two column tiles per wave (one activation fragment feeds both) exactly when that turns a two-round launch into one
    // round of <= 256 workgroups (c_fc: 320 tiles); measured per shape in profiles/r01_gemv_probe.txt
    pl.ntw = (pl.MT <= 2 && ntiles > 256 && cdiv(ntiles, 2) <= 256) ? 2 : 1;
  }
  pl.cps = cdiv(kc16, pl.kw * ksb);
  // 17..48 rows (coalesced decodes, 16 utterances x 3 beams): the one-batch form as well -- all five chunks of a wave's K-slice in
  // flight at once (10 + 20 MT VGPRs of operands: one workgroup per CU); the two-buffer form with 1-2 chunks per batch measured
  // 14.6 / 16.5 us per launch at 32 / 48 rows against 7.8 at 16 (profiles/README.md "Round 3").  49..64 rows have the two-buffer form only.
  pl.single = pl.narrow || (pl.cps <= 5 && pl.MT <= 3);
  if (pl.MT == 2 && !pl.single) pl.ntw = 1;      // two column tiles per wave at 17..32 rows exist in the one-batch form only
  const int nacc = pl.MT * pl.ntw;
  pl.threads = std::max(64 * pl.kw, 256 * nacc);      // one epilogue thread per output element of the workgroup
  pl.lds = (size_t)(pl.kw * nacc * 256 + pl.kw * pl.MT * 32 + pl.MT * 32) * sizeof(float);
  pl.grid_x = cdiv(ntiles, pl.ntw); pl.grid_y = ksb;
  return pl;
}

template <int MT, int NTW, bool SINGLE, int WT, bool R4, int UNS = 5>
static int fx_launch(const GemvFXP& p, const FxPlan& pl, hipStream_t stream) {
  static DynLdsLimit lds_limit;
  IDX_HIP(lds_limit.set(128 * 1024, gemv_fx_kernel<MT, NTW, SINGLE, WT, R4, UNS>));
  hipLaunchKernelGGL((gemv_fx_kernel<MT, NTW, SINGLE, WT, R4, UNS>), dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), pl.lds, stream, p);
  return 0;
}

template <int WT, bool R4>
static int fx_launch_mt1(const GemvFXP& p, const FxPlan& pl, hipStream_t stream) {
  if (pl.ntw == 2) return pl.single ? fx_launch<1, 2, true, WT, R4>(p, pl, stream) : fx_launch<1, 2, false, WT, R4>(p, pl, stream);
  return pl.single ? fx_launch<1, 1, true, WT, R4>(p, pl, stream) : fx_launch<1, 1, false, WT, R4>(p, pl, stream);
}

template <int WT>
static int fx_launch_wt(const GemvFXP& p, const FxPlan& pl, hipStream_t stream) {
  if (pl.narrow) {
    if constexpr (WT == WFMT_F32) IDX_FAIL("gemv_fx: the narrow form reads compact streams");
    else return fx_launch<1, 1, true, WT, false, 10>(p, pl, stream);
  }
  switch (pl.MT) {
    case 1: return pl.r4 ? fx_launch_mt1<WT, true>(p, pl, stream) : fx_launch_mt1<WT, false>(p, pl, stream);
    case 2:
      if (pl.ntw == 2) return fx_launch<2, 2, true, WT, false>(p, pl, stream);
      return pl.single ? fx_launch<2, 1, true, WT, false>(p, pl, stream) : fx_launch<2, 1, false, WT, false>(p, pl, stream);
    case 3: return pl.single ? fx_launch<3, 1, true, WT, false>(p, pl, stream) : fx_launch<3, 1, false, WT, false>(p, pl, stream);
    case 4: return fx_launch<4, 1, false, WT, false>(p, pl, stream);
  }
  IDX_FAIL("gemv_fx: no kernel for this plan");
}

int gemv_fx_forward(const WeightStream& w, const GemvFXArgs& a, hipStream_t stream) {
  const bool narrow_geom = g_decode_narrow.load() != 0;      // the process-wide switch, read ONCE per launch (a setter racing with a launch cannot tear the plan)
  IDX_CHECK(w.wp && a.xf && a.y, "null pointer");
  IDX_CHECK(w.kdepth == 16, "weight stream of 16 k per chunk");
  IDX_CHECK(a.rows > 0 && a.rows <= 64, "1..64 rows");
  IDX_CHECK((reinterpret_cast<uintptr_t>(a.xf) & 15) == 0, "x alignment");
  if (a.colsum) IDX_CHECK(w.K % 16 == 0, "folded LayerNorm needs K % 16 == 0");
  if (a.y_frag) IDX_CHECK(w.N % 16 == 0, "fragment-image output needs N % 16 == 0");
  IDX_CHECK(w.fmt == WFMT_F32 || w.fmt == WFMT_BF16 || (w.fmt == WFMT_FP8 && w.wscale), "weight format");
  const int ksb = (a.slab && a.ksb_counters) ? gemv_fx_ksb(w.N, w.K) : 1;
  if (ksb > 1) IDX_CHECK(!a.colsum && a.act == 0 && ksb <= 8, "K split across workgroups: no folded LayerNorm, no activation, <= 8 pieces");
  const FxPlan pl = gemv_fx_make_plan(w.N, w.K, a.rows, w.fmt, ksb, narrow_geom, a.invariant != 0);
  IDX_CHECK(pl.threads <= 1024, "workgroup size");
  GemvFXP p;
  p.xf = a.xf; p.wp = w.wp; p.wscale = w.wscale; p.bias = a.bias; p.colsum = a.colsum; p.ln_eps = a.ln_eps;
  p.res = a.res; p.y = a.y; p.y_frag = a.y_frag; p.ldy = a.ldy;
  p.rows = a.rows; p.N = w.N; p.K = w.K; p.kc16 = cdiv(w.K, 16); p.ntiles = cdiv(w.N, 16);
  p.kw = pl.kw; p.cps = pl.cps; p.act = a.act;
  p.ksb = ksb; p.slab = a.slab; p.cnt = ksb > 1 ? a.ksb_counters : nullptr;
  p.dbg = a.dbg;
  const double flops = 2.0 * a.rows * (double)w.N * w.K;
  const double bytes = (double)wfmt_bytes(w.fmt) * w.N * w.K + 4.0 * ((double)a.rows * w.N * (a.res ? 2.0 : 1.0) + (double)a.rows * w.K);
  static const int cat = prof_register("gemv_fx_kernel");
  ProfScope prof(cat, stream, flops, bytes);
  const int rc = w.fmt == WFMT_FP8 ? fx_launch_wt<WFMT_FP8>(p, pl, stream)
               : w.fmt == WFMT_BF16 ? fx_launch_wt<WFMT_BF16>(p, pl, stream) : fx_launch_wt<WFMT_F32>(p, pl, stream);
  if (rc) return rc;
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
