// Split-bf16 token-major GEMM, LDS-DMA pipeline (128 x 128 tile): same contract and arithmetic as gemm_bf16x3.hip
// (Y = epi(X W^T + b), x*w ~= hi*hi' + hi*lo' + lo*hi' on v_mfma_f32_16x16x32_bf16 or 32x32x16, fp32 accumulation), different
// data movement.
//
// Why (profiles/r01 PMC, gemm_bf16x3_big_kernel<4> at M=50208 N=1024 K=2560): MFMA busy 30 %, waves parked 39 % of their
// lifetime on the s_waitcnt in front of the fp32 -> hi/lo conversion of the NEXT activation tile -- the register-staged
// loop can only prefetch one 72 KB K-step per CU and issues it as one burst (tools/l2_probe.hip: a CU moves 34 B/clk
// from L2 with 64 KB in flight, 18 B/clk with 32 KB, ~11 B/clk from HBM), and two register sets do not fit beside the
// 128 accumulator registers.  Here nothing on the operand path touches a VGPR or the VALU:
//   * both operands live in HBM already split, as planes [hl][K/16][rows][16] bf16 (a 16-k chunk of all rows is one
//     contiguous run): the weights are laid out like that at load, the activations by one streaming pre-pass
//     (split_planes_kernel; 8 B/element moved once per GEMM instead of a conversion in every column-block);
//   * tiles go HBM/L2 -> LDS by global_load_lds_dwordx4 (1 KiB per wave-instruction) into a 3-deep ring of 16-k stages
//     (16 KiB each), retired with counted s_waitcnt vmcnt and raw s_barriers (RAW: wait, then barrier, then read; WAR: a
//     stage is overwritten only after a barrier behind its last read);
//   * LDS rows are 32 B (2 x 16-B units); unit' = unit ^ (row >> 3 & 1), applied on the DMA's SOURCE address and on the
//     ds_read_b128 address, makes every fragment read conflict-free without padding (the DMA destination is lane-linear).
//
// Opt-in bf16 arithmetic (gemm.h: set_acoustic_bf16; GemmArgs::bf16_products = 1): the 16x16x32 loop also exists with ONE MFMA per
// product, hi * hi' alone (template parameter NP of gemm_v2_tile).  gemm_forward selects it when the switch is on, the launch runs this
// kernel and the weights carry mf16.  The 32x32x16 loop here, the register-staged tile kernel (gemm_bf16x3.hip: fewer than 256 rows, or
// shapes without planes) and the exact kernel (gemm.hip) keep their arithmetic under the switch.  Both output planes (y_planes) and both
// planes of split_planes_kernel are written in either form: launches below 256 rows read the lo plane.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gemm_common.h"
#include "prof.h"

namespace idxtts {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---- weight planes: [hl][K/16][Npad][16] bf16, Npad = N rounded up to 256 (zero rows), K rounded up to 16 ----
size_t linear_planes_bytes(int N, int K) { return (size_t)2 * cdiv(K, 16) * (cdiv(N, 256) * 256) * 16 * sizeof(uint16_t); }

void pack_linear_planes(void* dst, const float* w, int N, int K) {
  uint16_t* o = static_cast<uint16_t*>(dst);
  const int KC = cdiv(K, 16), NP = cdiv(N, 256) * 256;
  std::memset(o, 0, linear_planes_bytes(N, K));
  uint16_t* lo = o + (size_t)KC * NP * 16;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      const float x = w[(size_t)n * K + k];
      const uint16_t hi = f2bf(x);
      const size_t idx = ((size_t)(k >> 4) * NP + n) * 16 + (k & 15);
      o[idx] = hi;
      lo[idx] = f2bf(x - bf2f(hi));
    }
}

// ---- activation pre-pass: x fp32 [M][ldx] -> planes [hl][K/16][M][16] bf16 ----
// Workgroup = 64 rows x 64 k.  Reads: 16 lanes per row (256 B = two full lines); writes: the four lanes of a 16-k chunk
// produce 32 B and the four rows of one wave-instruction are adjacent in the plane, so every store instruction fills
// four full 128-byte lines per plane.
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, int ldx, int M, int K, __bf16* __restrict__ hi,
                                                           __bf16* __restrict__ lo) {
  const int k = blockIdx.y * 64 + (threadIdx.x & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = blockIdx.x * 64 + (threadIdx.x >> 4) + 16 * i;
    if (m >= M || k >= ((K + 15) & ~15)) continue;
    const f32x4 v = k < K ? *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x4 h, l;
    split_bf16_x4(v, h, l);
    const size_t o = ((size_t)(k >> 4) * M + m) * 16 + (k & 15);
    *reinterpret_cast<bf16x4*>(hi + o) = h;
    *reinterpret_cast<bf16x4*>(lo + o) = l;
  }
}

#ifdef V2_TIMING
// Diagnostic build (tools/gemm_stamps.py; never the shipped library): s_memtime stamps of one wave per workgroup, written to a
// buffer of their own: [workgroup][8] = start, first stage landed, end of the main loop, end of the epilogue (stores drained),
// s_memrealtime x2, stores issued (wave 1 of the workgroup).
static unsigned long long* g_v2_stamps = nullptr;
extern "C" int idxtts_dbg_v2_stamps(void* buf) { g_v2_stamps = static_cast<unsigned long long*>(buf); return 0; }
#define V2_STAMP(k) do { if (q.stamps && tid == 64) q.stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define V2_RSTAMP(k) do { if (q.stamps && tid == 64) q.stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define V2_STAMP(k)
#define V2_RSTAMP(k)
#endif

struct GemmV2P {
  GemmKP g;                      // shapes, epilogue operands, conv parameters (x unused)
  const __bf16* a_hi; const __bf16* a_lo;   // [K/16][a_rows][16]
  const __bf16* b_hi; const __bf16* b_lo;   // [K/16][npad][16]
  int a_rows, npad, nstages;
  int a_bytes, b_bytes;          // bytes of the hi + lo planes of each operand (buffer descriptors)
  int a_plane, b_plane;          // byte offset of the lo plane
  int cs, nbg;                   // tile walk: column groups over the XCDs (1, 2, 4 or 8) and column blocks per group
#ifdef V2_TIMING
  unsigned long long* stamps;
#endif
};

// Geometry: workgroup = 2 x 2 waves, each 64 x 64: 128 x 128 per workgroup, 256 threads, 16 KiB stages, 3-deep ring (48 KiB),
// <= 168 registers: THREE workgroups per CU, whose phases (main loop / store-bound epilogue) interleave on a CU; launches of a
// few hundred rows still spread over the chip.  (Round 2's 256 x 256 tiles at one workgroup per CU were slower on every shape,
// see the dispatch, and are gone.)  Two main loops (MF) over the same ring, DMA pieces and epilogue:
//   32  v_mfma_f32_32x32x16_bf16, one 16-k stage per step, two fragment register sets, one barrier per stage;
//   16  v_mfma_f32_16x16x32_bf16, a pair of stages per step (below).
//
// Round 3: what a stage's instruction stream holds besides its MFMAs (24 per stage) decides the kernel (profiles/README.md "Round 3"):
//   * every LDS-DMA is ONE buffer_load_dwordx4 ... lds: the lane's byte offset inside the operand planes is a VGPR computed
//     once per tile (once per tap for the convolution form), the stage offset an SGPR that advances by a constant, the
//     ring slot goes to M0 -- no vector arithmetic per piece (the per-piece 64-bit address arithmetic of the first form was
//     ~20 VALU + ~35 SALU instructions, 100-185 issue cycles each time, four times per stage);
//   * rows outside a convolution's sequence read zeros through the descriptor's range check (offset bit 31 set), rows
//     beyond M re-read row M - 1 (never stored);
//   * the counted waits are the compiler's own s_waitcnt (builtin), not inline asm: with the asm form the compiler could not
//     know that a fragment set had landed and put s_waitcnt lgkmcnt(0) in front of the first MFMA of every stage -- i.e.
//     BEHIND the 12 fragment reads of the NEXT stage it had just issued, which undid the double-buffered fragment registers.
struct V2Rsrc { __amdgpu_buffer_rsrc_t a, b; };

#define V2_WAITCNT(vm) __builtin_amdgcn_s_waitcnt(((vm) & 15) | (((vm) >> 4) << 14) | 0x70)   /* vmcnt(vm) lgkmcnt(0) */

// NP: bf16 MFMAs per product.  3 = split-bf16 (above).  1 (MF == 16 only; the opt-in acoustic bf16 arithmetic, gemm.h:
// set_acoustic_bf16) = hi * hi' alone, fp32 accumulation: a stage requests and reads its two hi pieces only (the lo halves of the ring
// slots stay unwritten), a step issues 16 MFMAs for 8 fragment reads, the k order of a row's sum is that of the split loop.
template <bool TAPS, int EPI, int MF, int NP = 3>      // MF: the MFMA shape of the main loop, 32 = 32x32x16, 16 = 16x16x32
__device__ __forceinline__ void gemm_v2_tile(const GemmV2P& q, const int bm, const int bn, const int tid) {
  constexpr int NSTAGE = 3;                // ring depth (16-k stages)
  constexpr int WMW = 2, WNW = 2, TN = 2;      // waves along M / N, 32-column MFMA tiles per wave
  constexpr int BM = 64 * WMW, BN = 32 * TN * WNW;                 // 128 x 128
  static_assert(BM / 32 == WMW * WNW && BN / 32 == WMW * WNW, "one 32-row block of A and of B per wave and plane");
  static_assert(MF == 32 || MF == 16, "MFMA shape");
  static_assert(NP == 3 || (NP == 1 && MF == 16), "one MFMA per product exists in the 16x16x32 loop only");
  constexpr int PLANE = BM * 32;               // bytes of one operand plane of a stage (BM = BN rows x 32 B)
  constexpr int STAGE_BYTES = 4 * PLANE;       // [A hi][A lo][B hi][B lo]
  constexpr int PPW = NP == 1 ? 2 : 4;         // DMA instructions per wave and stage (the counted waits follow it)
  const GemmKP& p = q.g;
  extern __shared__ __attribute__((aligned(1024))) char smv2[];

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int h = lane >> 5, j = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;

  // ---- DMA role of this lane: row (lane >> 1) of the wave's 32-row block, LDS unit lane & 1, source unit swizzled ----
  const int lrow = lane >> 1;
  const int dunit = (lane & 1) ^ ((lrow >> 3) & 1);        // block bases are multiples of 32: row bit 3 = lrow bit 3
  const int a_m = bm * BM + 32 * wave + lrow;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(q.a_hi), 0, q.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(q.b_hi), 0, q.b_bytes, 0x00020000);
  const int voffB = (bn * BN + 32 * wave + lrow) * 32 + dunit * 16;
  int voffA = min(a_m, q.a_rows - 1) * 32 + dunit * 16;
  const ConvRow arow = conv_row(p, a_m);
  // the lane's A offset for tap `tap` (convolution form): row t = arow.t + tap * dil - pad_left of its own sequence, reflected
  // or zero outside [0, arow.n)
  auto tap_voff = [&](int tap) -> int {
    const int t = conv_src_row(arow.t + tap * p.dil - p.pad_left, arow.n, p.pad_mode);
    return a_m < p.M && t >= 0 ? (arow.base + t) * 32 + dunit * 16 : (int)0x80000000;
  };
  V2_STAMP(0); V2_RSTAMP(4);
  const int ns = q.nstages;
  const int sA = q.a_rows * 32, sB = q.npad * 32;          // bytes between two 16-k chunks of a plane
  const int cpt = TAPS ? (p.kc >> 4) : ns;                 // chunks per tap
  // scalar issue state: the next stage to request, its plane offsets, its chunk inside the tap
  int ist = 0, soA = 0, soB = 0, ich = 0, itap = 0, wslot = 0, rslot = 0;      // (ring slots of the next stage to request / to read)
  if (TAPS) voffA = tap_voff(0);
  char* const lds_w = smv2 + wave * 1024;
  auto issue_piece = [&](int pi) {           // piece pi of stage ist: A hi, A lo, B hi, B lo
    auto dst = (__attribute__((address_space(3))) void*)(lds_w + wslot * STAGE_BYTES + pi * PLANE);
    if (pi == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, dst, 16, voffA, soA, 0, 0);
    else if (pi == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, dst, 16, voffA, soA + q.a_plane, 0, 0);
    else if (pi == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, dst, 16, voffB, soB, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, dst, 16, voffB, soB + q.b_plane, 0, 0);
  };
  auto issue_a = [&]() { issue_piece(0); if (NP == 3) issue_piece(1); };      // the A pieces of stage ist / its B pieces
  auto issue_b = [&]() { issue_piece(2); if (NP == 3) issue_piece(3); };
  auto advance = [&]() {
    ++ist;
    wslot = wslot + 1 == NSTAGE ? 0 : wslot + 1;
    soB += sB;
    soA += sA;
    if (TAPS) {
      if (++ich == cpt) { ich = 0; soA = 0; ++itap; voffA = tap_voff(itap); }
    }
  };

  if constexpr (MF == 16) {
    // ---- v_mfma_f32_16x16x32_bf16: a step multiplies a PAIR of stages (32 k).  Lane (g = lane >> 4, r = lane & 15) holds row r of a
    // 16-row tile and k = 8 g .. 8 g + 7 of the pair: 16-B unit g & 1 of stage (pair's first) + (g >> 1), same swizzle.  A step reads
    // each of its 4 + 4 A and 4 + 4 B fragments once (16 ds_read_b128 per 32 k, as the 32x32 loop) and issues 48 MFMAs:
    //   wait (the pair has landed) | barrier | 16 fragment reads | 12 MFMAs (column tile 0, each row tile as its fragments arrive) |
    //   lgkmcnt(0), barrier: every wave has the pair in registers, its two ring slots are free | 36 MFMAs with the DMA of the two
    //   stages that take those slots between them.
    // The ring holds three stages, so the fragments of pair p + 1 cannot be read beside the MFMAs of pair p (their second stage
    // needs a slot of pair p); what hides the reads and the barriers is the other two workgroups of the CU.  One stage stays in
    // flight across the step's first barrier, two across the next step's wait.  Against the 32x32x16 loop (stamps, profiles/README.md
    // "MFMA shape"): + 14-20 % cycles per stage, + 12-19 % clock held -- 0.6-7 % less wall per launch.
    // An odd stage count ends in a step whose upper 32 lanes hold zero fragments (k order of a row's sum: pairs in order, then the
    // tail; independent of M and of the tile).
    const int g = lane >> 4, r16 = lane & 15;
    const int sw = ((g & 1) ^ ((r16 >> 3) & 1)) * 16;
    const int a_off = (wm * 64 + r16) * 32 + sw;                       // + t * 512 per 16-row tile
    const int b_off = 2 * PLANE + (wn * 64 + r16) * 32 + sw;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.0f;
    for (int s = 0; s < NSTAGE; ++s)
      if (s < ns) {
        issue_a(); issue_b();
        advance();
      }

    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    // one step: stages (done, done + 1), or the last stage alone (tail); nreq = stages to request in it (0 .. 2)
    auto pair_step = [&](const bool tail, const bool vm_one_behind, const int nreq) {
      if (vm_one_behind) V2_WAITCNT(PPW); else V2_WAITCNT(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const int second = rslot + 1 == NSTAGE ? 0 : rslot + 1;
      const char* st = smv2 + ((g >> 1) && !tail ? second : rslot) * STAGE_BYTES;
      rslot = second + 1 == NSTAGE ? 0 : second + 1;       // (a tail is the last step)
      bf16x8 ah[4], al[4], bh[4], bl[4];
      auto rd_a = [&](int t) {
        ah[t] = *reinterpret_cast<const bf16x8*>(st + a_off + t * 512);
        if (NP == 3) al[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + a_off + t * 512);
      };
      auto rd_b = [&](int t) {
        bh[t] = *reinterpret_cast<const bf16x8*>(st + b_off + t * 512);
        if (NP == 3) bl[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + b_off + t * 512);
      };
      // row tile 0 and column tile 0 first: the first MFMAs wait for three reads, not for all of A
      rd_a(0); rd_b(0);
      __builtin_amdgcn_sched_barrier(0);
      rd_a(1);
      __builtin_amdgcn_sched_barrier(0);
      rd_a(2);
      __builtin_amdgcn_sched_barrier(0);
      rd_a(3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 1; t < 4; ++t) rd_b(t);
      if (tail) {
        const unsigned keep = (g >> 1) ? 0u : 0xffffffffu;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          ah[t] = (bf16x8)((u32x4)ah[t] & keep); if (NP == 3) al[t] = (bf16x8)((u32x4)al[t] & keep);
          bh[t] = (bf16x8)((u32x4)bh[t] & keep); if (NP == 3) bl[t] = (bf16x8)((u32x4)bl[t] & keep);
        }
      }
      // one product of tile (mt, nt): lo * hi' + hi * lo' + hi * hi', or hi * hi' alone
      auto prod = [&](int mt, int nt) {
        if (NP == 3) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
        }
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
      };
#define V2_MFMA3(nt) _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) prod(mt, nt);
#define V2_MFMA1(mt, nt) prod(mt, nt); __builtin_amdgcn_sched_barrier(0);

      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA1(0, 0) V2_MFMA1(1, 0) V2_MFMA1(2, 0) V2_MFMA1(3, 0)      // (in the order their A fragments arrive)
      V2_WAITCNT(63);                           // lgkmcnt(0): every fragment of the pair is in registers
      __builtin_amdgcn_s_barrier();             // ... in every wave: the pair's ring slots are free
      __builtin_amdgcn_sched_barrier(0);
      if (nreq >= 1) issue_a();
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(1)
      __builtin_amdgcn_sched_barrier(0);
      if (nreq >= 1) { issue_b(); advance(); }
      if (nreq >= 2) issue_a();
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(2)
      __builtin_amdgcn_sched_barrier(0);
      if (nreq >= 2) { issue_b(); advance(); }
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(3)
      __builtin_amdgcn_sched_barrier(0);
#undef V2_MFMA1
#undef V2_MFMA3
    };
    V2_STAMP(1);
    int done = 0;                               // stages multiplied
    // steady state, straight-line: the stage behind the pair is in flight at the wait, two stages to request in the step
    for (; ist + 2 <= ns && ist > done + 2; done += 2) pair_step(false, true, 2);
    for (; done + 2 <= ns; done += 2) pair_step(false, ist > done + 2, min(ns - ist, 2));
    if (done < ns) pair_step(true, false, 0);
    V2_STAMP(2);
    // 16 x 16 C/D layout: register e of tile (mt, nt) is row mt * 16 + 4 g + e, column nt * 16 + r16
    auto write_pass = [&](int ps, float* lds, int RS) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[(4 * g + e) * RS + nt * 16 + r16] = acc[ps][nt][e];
    };
    gemm_epilogue_wave<EPI, TN, 3>(p, write_pass, reinterpret_cast<float*>(smv2), bm * BM + wm * 64, bn * BN + wn * TN * 32, wave, lane);
  } else {
    // fragment read offsets (bytes inside a plane image): row * 32 + (h ^ (row >> 3 & 1)) * 16, row = tile row of lane j
    const int sw = (h ^ ((j >> 3) & 1)) * 16;
    const int a_off = (wm * 64 + j) * 32 + sw;          // + t * 1024 for the second 32-row tile
    const int b_offr = (wn * TN * 32 + j) * 32 + sw;    // + t * 1024 per 32-column tile

    f32x16 acc[2][TN];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    for (int s = 0; s < NSTAGE; ++s)
      if (s < ns) {
#pragma unroll
        for (int pi = 0; pi < PPW; ++pi) issue_piece(pi);
        advance();
      }

    struct Frag { bf16x8 ah[2], al[2], bh[TN], bl[TN]; };
    // stage s has landed for the whole workgroup: this wave's pieces by the counted wait (younger stages may stay in
    // flight), everyone's by the barrier; the lgkmcnt(0) retires this wave's fragment reads of stage s - 1, so after the
    // barrier that ring slot may be overwritten.  Stages in flight behind s: min(2, ns - 1 - s) (3 behind stage 0).
    auto wait_stage = [&](int s) {
      const int rem = ns - 1 - s;           // stages behind s; at most NSTAGE - 2 of them have been requested
      if (rem >= 1) V2_WAITCNT(PPW);
      else V2_WAITCNT(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    auto load_frags = [&](Frag& f) {           // the next stage in order
      const char* st = smv2 + rslot * STAGE_BYTES;
      rslot = rslot + 1 == NSTAGE ? 0 : rslot + 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f.ah[t] = *reinterpret_cast<const bf16x8*>(st + a_off + t * 1024);
        f.al[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + a_off + t * 1024);
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        f.bh[t] = *reinterpret_cast<const bf16x8*>(st + 2 * PLANE + b_offr + t * 1024);
        f.bl[t] = *reinterpret_cast<const bf16x8*>(st + 3 * PLANE + b_offr + t * 1024);
      }
    };
    // 24 MFMAs of stage i; the DMA of stage i + NSTAGE (ring slot of stage i, free since the last barrier) is issued
    // piecewise between the four MFMA groups
    auto compute = [&](const Frag& f, const bool more) {
#define V2_MFMA3(mt, nt)                                                                                         \
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);             \
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bl[nt], acc[mt][nt], 0, 0, 0);             \
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);
      // four MFMA groups (half a row of tiles each) with one DMA piece behind each
      V2_MFMA3(0, 0)
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_piece(0);
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(0, 1)
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_piece(1);
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(1, 0)
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_piece(2);
      __builtin_amdgcn_sched_barrier(0);
      V2_MFMA3(1, 1)
      __builtin_amdgcn_sched_barrier(0);
      if (more) { issue_piece(3); advance(); }
      __builtin_amdgcn_sched_barrier(0);
#undef V2_MFMA3
    };

    // two fragment register sets: the reads of stage i + 1 are in flight while stage i is multiplied
    Frag f0, f1;
    {   // stage 0: up to three younger stages in flight
      const int rem = ns - 1;
      if (rem >= 2) V2_WAITCNT(2 * PPW);
      else if (rem >= 1) V2_WAITCNT(PPW);
      else V2_WAITCNT(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    V2_STAMP(1);
    load_frags(f0);
    int i = 0;
    // steady state, straight-line: two younger stages in flight behind every wait, a stage to request beside every compute
    // (a branch-free body also keeps the compiler's counter model exact: at a join of paths with different numbers of LDS reads
    // pending it falls back to s_waitcnt lgkmcnt(0) in front of the first MFMA, i.e. behind the next stage's fragment reads)
    for (; i + NSTAGE + 1 < ns; i += 2) {
      V2_WAITCNT((NSTAGE - 2) * PPW);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      load_frags(f1);
      compute(f0, true);
      V2_WAITCNT((NSTAGE - 2) * PPW);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      load_frags(f0);
      compute(f1, true);
    }
    for (; i < ns; i += 2) {     // the last stages: the ring drains
      if (i + 1 < ns) { wait_stage(i + 1); load_frags(f1); }
      else V2_WAITCNT(0);
      compute(f0, ist < ns);
      if (i + 1 < ns) {
        if (i + 2 < ns) { wait_stage(i + 2); load_frags(f0); }
        else V2_WAITCNT(0);
        compute(f1, ist < ns);
      }
    }
    // (the last wait_stage left no DMA in flight; the epilogue synchronises the workgroup itself before it reuses the ring)
    V2_STAMP(2);
    // 32 x 32 C/D layout: register r = (2 hh + qq) * 4 + e of tile (mt, nt) is row mt * 32 + 16 hh + 8 qq + 4 h + e, column nt * 32 + j
    auto write_pass = [&](int ps, float* lds, int RS) {
      const int mt = ps >> 1, hh = ps & 1;
#pragma unroll
      for (int nt = 0; nt < TN; ++nt)
#pragma unroll
        for (int qq = 0; qq < 2; ++qq)
#pragma unroll
          for (int e = 0; e < 4; ++e) lds[(8 * qq + 4 * h + e) * RS + nt * 32 + j] = acc[mt][nt][(2 * hh + qq) * 4 + e];
    };
    gemm_epilogue_wave<EPI, TN, 3>(p, write_pass, reinterpret_cast<float*>(smv2), bm * BM + wm * 64, bn * BN + wn * TN * 32, wave, lane);
  }
  V2_STAMP(6);
#ifdef V2_TIMING
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  V2_STAMP(3); V2_RSTAMP(5);
}

// one output tile per workgroup, walked in column groups (gemm_common.h: gemm_tile_walk)
template <bool TAPS, int EPI, int MF, int NP = 3>
__global__ __launch_bounds__(256, 3) void gemm_bf16x3_v2_kernel(const GemmV2P q) {
  int bn, bm;
  if (!gemm_tile_walk(q.g, blockIdx.x, bm, bn, q.cs, q.nbg)) return;
  gemm_v2_tile<TAPS, EPI, MF, NP>(q, bm, bn, threadIdx.x);
}

// per-stream scratch for the activation planes: room for a quarter more rows than the launch that grows it
StreamScratch g_plane_scratch(8);

int gemm_bf16x3_v2_forward(GemmKP p, const LinearWeights& w, const GemmArgs& a, hipStream_t stream, double flops, double bytes) {
  IDX_CHECK(w.K % 16 == 0 && (a.taps <= 1 || (w.K / a.taps) % 16 == 0), "v2 needs K % 16 == 0");
  const int xk = a.taps > 1 ? w.K / a.taps : w.K;       // channels of the activation rows
  const size_t plane = (size_t)(xk / 16) * a.M * 16 * sizeof(__bf16);
  void* scratch = nullptr;
  if (!a.x_planes && g_plane_scratch.acquire(stream, 2 * plane, &scratch)) return 1;
  const __bf16* hi = static_cast<const __bf16*>(a.x_planes ? a.x_planes : scratch);
  const __bf16* lo = hi + plane / sizeof(__bf16);
  if (!a.x_planes) {
    static const int cat_split = prof_register("split_planes_kernel");
    ProfScope prof(cat_split, stream, 0.0, 8.0 * a.M * (double)xk);
    hipLaunchKernelGGL(split_planes_kernel, dim3(cdiv(a.M, 64), cdiv(xk, 64)), dim3(256), 0, stream, a.x, a.ldx, a.M, xk, const_cast<__bf16*>(hi), const_cast<__bf16*>(lo));
    IDX_LAUNCH_CHECK();
  }
  GemmV2P q;
  q.g = p;
  if (a.y_planes) {
    const int n_out = (a.act == ACT_SWIGLU || a.act == ACT_GATE) ? w.N / 2 : w.N;
    IDX_CHECK(n_out % 16 == 0 && (a.ldy & 3) == 0, "output planes need N_out % 16 == 0");
    q.g.y_hi = static_cast<__bf16*>(a.y_planes);
    q.g.y_lo = q.g.y_hi + plane_elems(a.M, n_out);
  }
  if (a.rope) {
    IDX_CHECK(a.rope_T > 0 && a.rope_cols % 64 == 0 && a.act == ACT_NONE && (a.ldy & 3) == 0, "fused rotary arguments");
    q.g.rope = a.rope; q.g.rope_T = a.rope_T; q.g.rope_cols = a.rope_cols;
  }
  // geometry (tools/gemm_ab.py, one process, interleaved; profiles/README.md "Round 3"): 128 x 128 tiles, three workgroups per CU,
  // beat the 256 x 256 form on every shape measured -- M = 50 208: N = 512, K = 512 99 vs 117 us, N = 1536 224 vs 252, N = 3072 (SwiGLU)
  // 410 vs 456; M = 10 848, N = 5120, K = 1280 364 vs 435; 8192^2 x 1024 334 vs 347; under-filled grids (M = 750 .. 2066) 1.8-2.5x --
  // three co-resident workgroups overlap one tile's store-bound epilogue with the others' main loops, and four times as many tiles
  // quantise better over 256 CUs.
  const int BMh = 128, BNh = 128;
  q.g.mtiles = cdiv(a.M, BMh);
  q.g.mt8 = cdiv(q.g.mtiles, 8);
  q.g.nblocks = cdiv(w.N, BNh);
  q.a_hi = hi; q.a_lo = lo; q.a_rows = a.M;
  q.npad = cdiv(w.N, 256) * 256;
  q.b_hi = static_cast<const __bf16*>(w.planes16);
  q.b_lo = q.b_hi + (size_t)(w.K / 16) * q.npad * 16;
  q.nstages = w.K / 16;
#ifdef V2_TIMING
  q.stamps = g_v2_stamps;
#endif
  const size_t b_plane = (size_t)(w.K / 16) * q.npad * 32;
  IDX_CHECK(2 * plane < (1ull << 31) && 2 * b_plane < (1ull << 31), "operand planes beyond the 2 GiB a buffer offset addresses");
  q.a_plane = (int)plane; q.a_bytes = (int)(2 * plane);
  q.b_plane = (int)b_plane; q.b_bytes = (int)(2 * b_plane);
  // Column groups: the smallest power of two that brings an XCD's B slice (hi + lo planes) under ~3.2 MB, i.e. next to the streaming A
  // in its 4 MiB L2.  Time does not depend on the threshold between 1.5 and 7 MB (s2mel 0.497-0.503 s sequential, 183-185 audio-s/s
  // pipelined); the bytes past the L2 do (profiles/r04_gemm_cs_pmc.txt: mean FETCH_SIZE per launch 289 MiB at 1.5 MB -- A re-read once per
  // group --, 234 at 3.2, 309 at 7 -- the SwiGLU B no longer fits): 3.2 MB.  A B of up to 8 slices walks the same way (its column groups
  // keep their slices resident; walking column blocks slowest re-read A once per 128 columns).
  q.cs = 1;
  static const double cs_bytes = [] { const char* e = getenv("IDXTTS_GEMM_CS_BYTES"); return e ? atof(e) : 3.2e6; }();      // (measurement hook)
  if (!q.g.n_fast && (double)w.N * w.K * 4.0 <= 8.0 * cs_bytes && a.M > w.N) q.g.n_fast = 1;
  if (q.g.n_fast) {
    while (q.cs < 8 && (double)w.N * w.K * 4.0 / q.cs > cs_bytes && q.g.nblocks >= 2 * q.cs) q.cs *= 2;
  }
  q.nbg = cdiv(q.g.nblocks, q.cs);
  const int64_t grid = q.g.n_fast ? (int64_t)8 * q.nbg * cdiv(q.g.mtiles, 8 / q.cs) : (int64_t)8 * q.g.nblocks * q.g.mt8;
  IDX_CHECK(grid < (1ll << 31), "grid size");
  static const int cat = prof_register("gemm_bf16x3_v2_kernel");
  ProfScope prof(cat, stream, flops, bytes);
  const int lds = 3 * (4 * 128 * 32);
  const bool paired = a.act == ACT_SWIGLU || a.act == ACT_GATE;
  IDX_CHECK(!(a.rope && (a.res || paired)), "the rotary epilogue takes no residual and no paired activation");
  IDX_CHECK(!a.row_len || a.seq_len >= 16, "row masks need seq_len >= 16");
  const int epi = a.rope ? EPI_ROPE : paired ? EPI_PAIRED : a.act != ACT_NONE ? EPI_ACT : EPI_PLAIN;
  IDX_CHECK(!a.ld_bias || (paired && a.taps > 1), "the LDS-DMA kernel takes a per-sequence bias in its paired convolution form");
  typedef void (*KernelFn)(const GemmV2P);
#define V2_ROW(T, F, P) gemm_bf16x3_v2_kernel<T, EPI_PLAIN, F, P>, gemm_bf16x3_v2_kernel<T, EPI_ROPE, F, P>, gemm_bf16x3_v2_kernel<T, EPI_PAIRED, F, P>, gemm_bf16x3_v2_kernel<T, EPI_ACT, F, P>
  // the main loop's MFMA shape comes with the weights (model_util.h: WP16_ALWAYS_MF16): 16x16x32 is 1.5-7 % faster on six of eight
  // shapes and equal on two (tools/gemm_ab.py, profiles/README.md "MFMA shape"), but its sums differ in the last bits from the
  // 32x32x16 loop's, which the models that feed a choice of discrete codes keep
  // (row 2: one MFMA per product, GemmArgs::bf16_products == 1 -- the 16x16x32 loop only)
  static const KernelFn kernels[3][2][4] = {{{V2_ROW(false, 32, 3)}, {V2_ROW(true, 32, 3)}}, {{V2_ROW(false, 16, 3)}, {V2_ROW(true, 16, 3)}},
                                            {{V2_ROW(false, 16, 1)}, {V2_ROW(true, 16, 1)}}};
  static DynLdsLimit lds_limit;
  IDX_HIP(lds_limit.set(lds, V2_ROW(false, 32, 3), V2_ROW(true, 32, 3), V2_ROW(false, 16, 3), V2_ROW(true, 16, 3), V2_ROW(false, 16, 1), V2_ROW(true, 16, 1)));
  IDX_CHECK(a.bf16_products == 3 || (a.bf16_products == 1 && w.mf16), "one MFMA per product needs weights of the 16x16x32 loop");
  int mf16 = w.mf16 ? 1 : 0;
#ifdef V2_EXP_SHAPE
  if (const char* e = getenv("IDXTTS_EXP_V2_SHAPE")) mf16 = atoi(e) == 16;      // tools/gemm_ab.py's scratch build only
#endif
  // the per-sequence bias (GemmArgs::ld_bias): the paired convolution form of each loop, instantiations of their own
  static const KernelFn seqbias_kernels[3] = {gemm_bf16x3_v2_kernel<true, EPI_PAIRED_SEQB, 32, 3>, gemm_bf16x3_v2_kernel<true, EPI_PAIRED_SEQB, 16, 3>,
                                              gemm_bf16x3_v2_kernel<true, EPI_PAIRED_SEQB, 16, 1>};
  static DynLdsLimit lds_limit_sb;
  if (a.ld_bias) IDX_HIP(lds_limit_sb.set(lds, seqbias_kernels[0], seqbias_kernels[1], seqbias_kernels[2]));
  const int loop = a.bf16_products == 1 ? 2 : mf16;
  const KernelFn kernel = a.ld_bias ? seqbias_kernels[loop] : kernels[loop][a.taps > 1 ? 1 : 0][epi];
#undef V2_ROW
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), lds, stream, q);
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
