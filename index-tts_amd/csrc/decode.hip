// Per-token kernels of the GPT autoregressive decode (the reference's `accel_engine.generate` plugin
// slot, model_v2.py:871-883 / accel/accel_engine.py:378-645, and the HF `_sample` loop it falls back to,
// transformers_generation_utils.py:3196-3269):
//   decode_attn_kernel   one query token per (utterance, head) against the KV cache (HBM-bound KV read);
//                        also folds the c_attn split-K partial sum + bias and the KV-cache write
//                        (the reference's Triton `store_kvcache_kernel`, accel/attention.py:57-86)
//   sample_greedy_kernel lm_head partial sum + bias -> RepetitionPenalty (gen_utils 900-901) -> argmax
//                        (3252) -> finished/pad bookkeeping (3255-3264), all on device: no host sync per token
//   kv_store_prefill / advance_state  glue
// All per-step scalars (cache position, mel position, output column) live in a DecodeState in HBM so a
// step is replayable (hipGraph) without re-binding kernel arguments.
//
// KV cache layout (chosen for the decode read pattern, the only hot reader):
//   K: [B][H][16][Smax][4]   dot products walk the keys with lanes = keys -> 16-byte, fully coalesced
//   V: [B][H][Smax][64]      P.V walks the keys with lanes = head dim    -> 256-byte coalesced rows
// or, with DecodeAttnArgs::kv_fmt 1 (decode_attn16_kernel), the same in bf16: K [B][H][8][Smax][8], V [B][H][Smax][64];
// or, with kv_fmt 2 (decode_attn8_kernel), that geometry in scaled fp8 codes plus one fp32 scale per key and per value (kv_fp8.h).
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "beam.h"
#include "decode.h"
#include "device_util.h"
#include "kv_fp8.h"
#include "prof.h"
#include "wstream.h"

namespace idxtts {

// Output of one (utterance, head) workgroup: o = this thread's unnormalised output element (threads 0..63), mx / l = the piece's
// score maximum and exp-sum.  NS == 1: normalise and write the A-fragment image for the c_proj GEMV.  Key split: leave (o, max, sum)
// of this piece; the last piece to arrive merges all of them in piece order.
__device__ __forceinline__ void decode_attn_finish(const DecodeAttnArgs& p, const int b, const int h, const int z, const int NS, const int tid,
                                                   const float o, const float mx, const float l) {
  const int d = p.d;
  auto put = [&](float val) {      // input of the c_proj GEMV: an A-fragment image (gemv_fx.hip) or a plain fp32 row (gemv_pl.hip)
    if (p.out_row) p.out_row[(size_t)b * d + h * 64 + tid] = val;
    else p.out[frag_index(b, h * 64 + tid, d >> 4)] = val;
  };
  if (NS == 1) {
    if (tid < 64) put(l > 0.f ? o / l : 0.f);
    return;
  }
  // ---- key split: leave (o, max, sum) of this piece; the last piece to arrive merges all of them in piece order ----
  float* mine = p.part + ((size_t)(b * p.H + h) * NS + z) * 66;
  if (tid < 64) __hip_atomic_store(&mine[tid], o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 64) __hip_atomic_store(&mine[64], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 65) __hip_atomic_store(&mine[65], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!wg_arrive_last(&p.cnt[b * p.H + h], (unsigned)NS) || tid >= 64) return;
  const float* all = p.part + (size_t)(b * p.H + h) * NS * 66;
  float mi[16], li[16], oi[16];       // every piece's (max, sum, this lane's output) in ONE round trip
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const bool on = i < NS;
    mi[i] = on ? __hip_atomic_load(&all[i * 66 + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1e30f;
    li[i] = on ? __hip_atomic_load(&all[i * 66 + 65], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    oi[i] = on ? __hip_atomic_load(&all[i * 66 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
  }
  float M = -1e30f;
#pragma unroll
  for (int i = 0; i < 16; ++i) M = fmaxf(M, mi[i]);
  float O = 0.f, L = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float wgt = li[i] > 0.f ? expf(mi[i] - M) : 0.f;
    O += wgt * oi[i];
    L += wgt * li[i];
  }
  put(L > 0.f ? O / L : 0.f);
}

// Output of a row whose session slot is not live: zeros, written once per (row, head)
__device__ __forceinline__ void decode_attn_dead(const DecodeAttnArgs& p, const int b, const int h, const int z, const int tid) {
  if (z != 0 || tid >= 64) return;
  if (p.out_row) p.out_row[(size_t)b * p.d + h * 64 + tid] = 0.f;
  else p.out[frag_index(b, h * 64 + tid, p.d >> 4)] = 0.f;
}

// Batch-invariant mode (DecodeAttnArgs::invariant): piece z of the row's NP = decode_attn_pieces(n) pieces leaves (o, max, sum) at a
// fixed stride of 16 pieces per (row, head), whichever workgroup computed it
__device__ __forceinline__ void decode_attn_piece_store(const DecodeAttnArgs& p, const int b, const int h, const int z, const int tid,
                                                        const float o, const float mx, const float l) {
  float* mine = p.part + ((size_t)(b * p.H + h) * DECODE_ATTN_MAX_PIECES + z) * 66;
  if (tid < 64) __hip_atomic_store(&mine[tid], o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 64) __hip_atomic_store(&mine[64], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 65) __hip_atomic_store(&mine[65], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... and the last of the row's `wgs` workgroups to arrive merges the NP pieces in piece order: the same sums whether one workgroup
// walked all the pieces or each piece had its own
__device__ __forceinline__ void decode_attn_piece_merge(const DecodeAttnArgs& p, const int b, const int h, const int NP, const int wgs,
                                                        const int tid) {
  if (!wg_arrive_last(&p.cnt[b * p.H + h], (unsigned)wgs) || tid >= 64) return;
  const float* all = p.part + (size_t)(b * p.H + h) * DECODE_ATTN_MAX_PIECES * 66;
  float mi[DECODE_ATTN_MAX_PIECES], li[DECODE_ATTN_MAX_PIECES], oi[DECODE_ATTN_MAX_PIECES];
#pragma unroll
  for (int i = 0; i < DECODE_ATTN_MAX_PIECES; ++i) {
    const bool on = i < NP;
    mi[i] = on ? __hip_atomic_load(&all[i * 66 + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1e30f;
    li[i] = on ? __hip_atomic_load(&all[i * 66 + 65], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    oi[i] = on ? __hip_atomic_load(&all[i * 66 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
  }
  float M = -1e30f;
#pragma unroll
  for (int i = 0; i < DECODE_ATTN_MAX_PIECES; ++i) M = fmaxf(M, mi[i]);
  float O = 0.f, L = 0.f;
#pragma unroll
  for (int i = 0; i < DECODE_ATTN_MAX_PIECES; ++i) {
    const float wgt = li[i] > 0.f ? expf(mi[i] - M) : 0.f;
    O += wgt * oi[i];
    L += wgt * li[i];
  }
  const float val = L > 0.f ? O / L : 0.f;
  if (p.out_row) p.out_row[(size_t)b * p.d + h * 64 + tid] = val;
  else p.out[frag_index(b, h * 64 + tid, p.d >> 4)] = val;
}

// ---- the cache formats: how a key / value granule (16 bytes; fp8: 8) is laid out, widened, multiplied and stored.  All keep a key
//      as 64 / EPG granules [granule][Smax] and a value row as 64 / EPG granules, one per lane; every product and sum is fp32. ----
// fp32 cache: K [B][H][16][Smax][4], V [B][H][Smax][64] (256-byte rows)
struct KvF32 {
  static constexpr bool SCALED = false;   // no per-vector scales
  typedef float E;                        // cache element
  typedef f32x4 G;                        // granule
  typedef f32x4 Acc;                      // a lane's P.V accumulator: the head dims of its granule
  typedef f32x4 VNew;                     // the new token's value, this lane's granule
  static constexpr int EPG = 4;           // elements per granule
  static constexpr int NACC = 4;          // independent accumulators
  static constexpr int OUT_UNROLL = 32;   // the group reduction, fully unrolled
  __device__ static __forceinline__ G zero() { return G{0.f, 0.f, 0.f, 0.f}; }
  // the new token's k / v element: the cache gets it (piece 0), this step uses what a later step will read back
  __device__ static __forceinline__ float put(E* dst, const bool write, const float x) {
    if (write) *dst = x;
    return x;
  }
  __device__ static __forceinline__ float dot_new(const float (&qv)[64], const float* knew) {
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dot += qv[4 * i] * knew[4 * i] + qv[4 * i + 1] * knew[4 * i + 1] + qv[4 * i + 2] * knew[4 * i + 2] + qv[4 * i + 3] * knew[4 * i + 3];
    return dot;
  }
  __device__ static __forceinline__ float dot_key(const float (&qv)[64], const G (&kk)[16]) {
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dot += qv[4 * i] * kk[i][0] + qv[4 * i + 1] * kk[i][1] + qv[4 * i + 2] * kk[i][2] + qv[4 * i + 3] * kk[i][3];
    return dot;
  }
  __device__ static __forceinline__ VNew vnew_of(const float* vnew, const int l) { return *reinterpret_cast<const f32x4*>(&vnew[4 * l]); }
  __device__ static __forceinline__ void fma(Acc& acc, const float pw, const G v) { acc += pw * v; }
  __device__ static __forceinline__ void fma_new(Acc& acc, const float pw, const VNew vn) { acc += pw * vn; }
  __device__ static __forceinline__ void store(float* dst, const Acc (&a)[4]) { *reinterpret_cast<f32x4*>(dst) = (a[0] + a[1]) + (a[2] + a[3]); }
};
// bf16 cache (DecodeAttnArgs::kv16), half the bytes: K [B][H][8][Smax][8], V [B][H][Smax][64] (128-byte rows).  A key / value is
// rounded to bf16 (nearest even) when it is produced -- the new token's own k / v too, so a position reads the same whether it is
// the newest or an old one -- and widened exactly (<< 16) when used.
struct KvBf16 {
  static constexpr bool SCALED = false;
  typedef unsigned short E;
  typedef u32x4 G;
  struct Acc { float e[8]; };
  typedef const float* VNew;
  static constexpr int EPG = 8;
  static constexpr int NACC = 2;
  static constexpr int OUT_UNROLL = 16;
  __device__ static __forceinline__ G zero() { return G{0u, 0u, 0u, 0u}; }
  __device__ static __forceinline__ float put(E* dst, const bool write, const float x) {
    const unsigned bits = bf16_rne_bits(x);
    if (write) *dst = (unsigned short)bits;
    return __uint_as_float(bits << 16);
  }
  __device__ static __forceinline__ float dot_new(const float (&qv)[64], const float* knew) {
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 64; ++i) dot += qv[i] * knew[i];
    return dot;
  }
  __device__ static __forceinline__ float dot_key(const float (&qv)[64], const G (&kk)[8]) {
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        dot += qv[8 * i + 2 * j] * __uint_as_float(kk[i][j] << 16) + qv[8 * i + 2 * j + 1] * __uint_as_float(kk[i][j] & 0xffff0000u);
    return dot;
  }
  __device__ static __forceinline__ VNew vnew_of(const float* vnew, const int l) { return vnew + 8 * l; }
  __device__ static __forceinline__ void fma(Acc& acc, const float pw, const G v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc.e[2 * j] += pw * __uint_as_float(v[j] << 16);
      acc.e[2 * j + 1] += pw * __uint_as_float(v[j] & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ void fma_new(Acc& acc, const float pw, const VNew vn) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.e[e] += pw * vn[e];
  }
  __device__ static __forceinline__ void store(float* dst, const Acc (&a)[2]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = a[0].e[e] + a[1].e[e];
  }
};

// scaled fp8 cache (DecodeAttnArgs::kv_fmt 2; the format: kv_fp8.h), half the bf16 bytes in its geometry: K [B][H][8][Smax][8],
// V [B][H][Smax][64] (64-byte rows), 8-byte granules, LPR = 8 lanes per value row and NG = 64 key groups as KvBf16 -- 16-byte granules
// (LPR = 4, NG = 128: 32 KB of outp, a 128-term group reduction) were not tried.  The body multiplies a key's score by its scale and
// folds a value's scale into its probability; both are powers of two, so a position reads the same whether it is the newest (knew /
// vnew hold decode(code) * scale) or an old one.
struct KvFp8 {
  static constexpr bool SCALED = true;
  typedef unsigned char E;
  typedef u32x2 G;
  struct Acc { float e[8]; };
  typedef const float* VNew;
  static constexpr int EPG = 8;
  static constexpr int NACC = 2;
  static constexpr int OUT_UNROLL = 16;
  __device__ static __forceinline__ G zero() { return G{0u, 0u}; }
  __device__ static __forceinline__ float dot_new(const float (&qv)[64], const float* knew) { return KvBf16::dot_new(qv, knew); }
  __device__ static __forceinline__ float dot_key(const float (&qv)[64], const G (&kk)[8]) {
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[i][j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[i][j], true);
        dot += qv[8 * i + 4 * j] * lo[0] + qv[8 * i + 4 * j + 1] * lo[1];
        dot += qv[8 * i + 4 * j + 2] * hi[0] + qv[8 * i + 4 * j + 3] * hi[1];
      }
    return dot;
  }
  __device__ static __forceinline__ VNew vnew_of(const float* vnew, const int l) { return vnew + 8 * l; }
  __device__ static __forceinline__ void fma(Acc& acc, const float pw, const G v) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], true);
      acc.e[4 * j] += pw * lo[0];
      acc.e[4 * j + 1] += pw * lo[1];
      acc.e[4 * j + 2] += pw * hi[0];
      acc.e[4 * j + 3] += pw * hi[1];
    }
  }
  __device__ static __forceinline__ void fma_new(Acc& acc, const float pw, const VNew vn) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.e[e] += pw * vn[e];
  }
  __device__ static __forceinline__ void store(float* dst, const Acc (&a)[2]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = a[0].e[e] + a[1].e[e];
  }
};

// One query token per (utterance, head) workgroup against its cached keys, or against one of gridDim.z pieces of them.
// NT threads per workgroup: NT keys per pass of the score phase, NG = NT / (lanes of a value row) key groups in the P.V phase.  512
// threads at <= 128 VGPRs (two workgroups per CU) halve the number of dependent load -> use passes of the 256-thread form.
// SLOTS: decode session (DecodeAttnArgs::slot) -- the row's own position, dead rows return at once.  KV: the cache format.
// BI: the batch-invariant mode (DecodeAttnArgs::invariant).  The row's n keys are cut into NP = decode_attn_pieces(n) pieces, a rule of
// n alone, and the gridDim.z workgroups of the (row, head) share them out: workgroup z walks pieces z, z + gridDim.z, ... one after
// the other, each through the same score / softmax / P.V passes a piece of the key split takes.  gridDim.z decides how many workgroups
// work on the row, never what is summed with what.
template <int NT, bool SLOTS, class KV, bool BI = false>
__device__ __forceinline__ void decode_attn_body(const DecodeAttnArgs& p) {
  typedef typename KV::G G;
  typedef typename KV::E E;
  constexpr int NW = NT / 64, EPG = KV::EPG, KG = 64 / EPG, LPR = 64 / EPG, NG = NT / LPR, NACC = KV::NACC;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* qs = sm;            // [64] scaled query
  float* knew = sm + 64;     // [64] the new token's key and value, as the cache holds them
  float* vnew = sm + 128;    // [64]
  float* red = sm + 192;     // [2 * NW]
  float* outp = sm + 256;    // [NG][64] per-key-group partial outputs
  float* pr = sm + 256 + NG * 64;   // [Smax] scores / probabilities

  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int pos;                                    // index of the token being processed = keys already cached
  if constexpr (SLOTS) {
    if (!p.slot[b].live) { decode_attn_dead(p, b, h, blockIdx.z, tid); return; }
    pos = p.slot[b].pos;
  } else {
    pos = p.st->pos;
  }
  const int d = p.d, Smax = p.Smax;
  G* const kc = static_cast<G*>(p.kcache) + (size_t)(b * p.H + h) * KG * Smax;       // granule (c, s) at c * Smax + s
  G* const vc = static_cast<G*>(p.vcache) + (size_t)(b * p.H + h) * Smax * LPR;      // granule (s, c) at s * LPR + c
  float* const ksc = KV::SCALED ? p.kscale + (size_t)(b * p.H + h) * Smax : nullptr;   // scaled formats: one scale per key / value
  float* const vsc = KV::SCALED ? p.vscale + (size_t)(b * p.H + h) * Smax : nullptr;

  // Everything that does not depend on the new token's q is put in flight first: this thread's first key (KG x 16 B,
  // coalesced across threads) and its first value rows of the P.V phase; the kernel is a chain of dependent
  // HBM / L2 round trips, so the cache streams have to overlap the qkv fetch and the softmax barriers.
  // key range of this workgroup: all of [kstart, pos] (pos = the new token), or one of gridDim.z contiguous pieces of it
  const int ks0 = p.kstart ? p.kstart[b] : 0;
  const int NS = gridDim.z, z0 = blockIdx.z;
  const int NP = BI ? decode_attn_pieces(pos - ks0 + 1) : NS;      // pieces of this row's keys
  if (BI && z0 >= NP) return;                                       // (workgroup-uniform) more workgroups than pieces
  const int chunk = NP > 1 ? (((pos - ks0 + NP) / NP + 15) & ~15) : pos - ks0 + 1;
  const int grp = tid / LPR, lpr = tid % LPR;
  for (int z = z0;; z += NS) {      // one pass unless BI (the body below keeps the one-pass kernels' indentation)
  const int ks = ks0 + z * chunk;
  const int ke = min(pos, ks + chunk - 1);          // inclusive; ks > ke: an empty piece
  const int s_first = ks + tid;
  G kk0[KG];
#pragma unroll
  for (int i = 0; i < KG; ++i) kk0[i] = (s_first < pos && s_first <= ke) ? kc[(size_t)i * Smax + s_first] : KV::zero();
  float ks_first = 1.f, vs_first = 1.f;      // scaled formats: the first key's scales travel with it (the new token's own: 1)
  if constexpr (KV::SCALED) {
    if (s_first < pos && s_first <= ke) { ks_first = ksc[s_first]; vs_first = vsc[s_first]; }
  }
  constexpr int VP = 128 / NG;      // value rows prefetched per lane before the scores (NG * VP = 128 keys)
  G vpre[VP];
#pragma unroll
  for (int j = 0; j < VP; ++j) {
    const int sj = ks + grp + NG * j;
    vpre[j] = (sj < pos && sj <= ke) ? vc[(size_t)sj * LPR + lpr] : KV::zero();
  }

  // ---- q, k, v of the new token (waves 0,1,2 take q,k,v): the c_attn split-K partial sum + bias, k / v to the cache ----
  if ((!BI || z == z0) && tid < 192) {
    const int which = tid >> 6, dd = tid & 63;
    const int col = which * d + h * 64 + dd;
    const float* row = p.qkv_part + (size_t)b * 3 * d + col;
    const size_t sst = (size_t)p.part_rows * 3 * d;
    float acc = p.qkv_bias ? p.qkv_bias[col] : 0.0f;
    for (int s = 0; s < p.parts; ++s) acc += row[(size_t)s * sst];
    if (which == 0) qs[dd] = acc * p.scale;
    else if constexpr (KV::SCALED) {      // waves 1 and 2 whole, one vector each: its scale needs the maximum over the 64 lanes
      unsigned code;
      float sc;
      const float val = kv_fp8_quantize_lane(acc, code, sc);
      (which == 1 ? knew : vnew)[dd] = val;
      if (z == 0) {
        if (which == 1) reinterpret_cast<E*>(kc + (size_t)(dd / EPG) * Smax + pos)[dd % EPG] = (E)code;
        else reinterpret_cast<E*>(vc + (size_t)pos * LPR)[dd] = (E)code;
        if (dd == 0) (which == 1 ? ksc : vsc)[pos] = sc;
      }
    } else if (which == 1) knew[dd] = KV::put(reinterpret_cast<E*>(kc + (size_t)(dd / EPG) * Smax + pos) + dd % EPG, z == 0, acc);
    else vnew[dd] = KV::put(reinterpret_cast<E*>(vc + (size_t)pos * LPR) + dd, z == 0, acc);
  }
  __syncthreads();

  // the query is wave-uniform: 64 SGPRs (v_readlane of one LDS read per lane) instead of 64 VGPRs
  // (BI: read again in every pass -- 64 scalar moves -- rather than carried round the loop)
  const float qlane = qs[lane];
  float qv[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) qv[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qlane), i));

  // ---- scores: one key per thread and pass; the first pass consumes the prefetched key ----
  float mx = -1e30f;
  if (s_first <= ke) {
    float dot = s_first == pos ? KV::dot_new(qv, knew) : KV::dot_key(qv, kk0);
    if constexpr (KV::SCALED) dot *= ks_first;
    pr[s_first] = dot;
    mx = dot;
  }
  for (int s = s_first + NT; s <= ke; s += NT) {
    float dot;
    if (s == pos) dot = KV::dot_new(qv, knew);
    else {
      G kk[KG];
#pragma unroll
      for (int i = 0; i < KG; ++i) kk[i] = kc[(size_t)i * Smax + s];
      dot = KV::dot_key(qv, kk);
      if constexpr (KV::SCALED) dot *= ksc[s];
    }
    pr[s] = dot;
    mx = fmaxf(mx, dot);
  }
  // (the two softmax reductions: disjoint halves of `red`, one barrier each)
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red[w]);
  float sum = 0.f;
  for (int s = s_first; s <= ke; s += NT) {
    const float e = expf(pr[s] - mx);
    if constexpr (KV::SCALED) {      // the P.V weight of a cached value carries its scale; the sum does not
      pr[s] = e * (s == s_first ? vs_first : s == pos ? 1.f : vsc[s]);
    } else {
      pr[s] = e;
    }
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[NW + wave] = sum;
  __syncthreads();
  float l = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) l += red[NW + w];

  // ---- P.V : NG key groups x LPR lanes; a lane owns the head dims of one granule (one 16-byte load per key, whole rows
  //      coalesced), 8 keys in flight per lane; group g takes keys ks+g, ks+g+NG, ... ----
  const typename KV::VNew vn = KV::vnew_of(vnew, lpr);
  typename KV::Acc acc[NACC] = {};
#pragma unroll
  for (int j = 0; j < VP; ++j) {
    const int sj = ks + grp + NG * j;
    if (sj <= ke) {
      if (sj == pos) KV::fma_new(acc[j % NACC], pr[sj], vn);
      else KV::fma(acc[j % NACC], pr[sj], vpre[j]);
    }
  }
  for (int sb = ks + grp + VP * NG; sb <= ke; sb += 8 * NG) {
    G v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int sj = sb + NG * j;
      v[j] = (sj < pos && sj <= ke) ? vc[(size_t)sj * LPR + lpr] : KV::zero();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int sj = sb + NG * j;
      if (sj <= ke) {
        if (sj == pos) KV::fma_new(acc[j % NACC], pr[sj], vn);
        else KV::fma(acc[j % NACC], pr[sj], v[j]);
      }
    }
  }
  KV::store(&outp[grp * 64 + EPG * lpr], acc);
  __syncthreads();
  float o = 0.f;
  if (tid < 64) {
#pragma unroll KV::OUT_UNROLL
    for (int g = 0; g < NG; ++g) o += outp[g * 64 + tid];
  }
  if constexpr (!BI) {
    decode_attn_finish(p, b, h, z, NS, tid, o, mx, l);
    break;
  } else {
    if (NP == 1) {      // n <= DECODE_ATTN_PIECE_KEYS: the row's only piece, normalised in place
      decode_attn_finish(p, b, h, 0, 1, tid, o, mx, l);
      break;
    }
    decode_attn_piece_store(p, b, h, z, tid, o, mx, l);
    if (z + NS >= NP) {
      decode_attn_piece_merge(p, b, h, NP, min(NS, NP), tid);
      break;
    }
    // (pr / red / outp are reused by the next piece: the barrier behind its prefetch orders that)
  }
  }
}

template <int NT, bool SLOTS>
__global__ __launch_bounds__(NT, (NT == 512 ? 4 : 1)) void decode_attn_kernel(const DecodeAttnArgs p) {
  decode_attn_body<NT, SLOTS, KvF32>(p);
}
template <int NT, bool SLOTS>
__global__ __launch_bounds__(NT, (NT == 512 ? 4 : 1)) void decode_attn16_kernel(const DecodeAttnArgs p) {
  decode_attn_body<NT, SLOTS, KvBf16>(p);
}
template <int NT, bool SLOTS>
__global__ __launch_bounds__(NT, (NT == 512 ? 4 : 1)) void decode_attn8_kernel(const DecodeAttnArgs p) {
  decode_attn_body<NT, SLOTS, KvFp8>(p);
}
// the batch-invariant mode's form of the three (KVF: DecodeAttnArgs::kv_fmt)
template <int NT, bool SLOTS, int KVF>
__global__ __launch_bounds__(NT, (NT == 512 ? 4 : 1)) void decode_attn_inv_kernel(const DecodeAttnArgs p) {
  if constexpr (KVF == 2) decode_attn_body<NT, SLOTS, KvFp8, true>(p);
  else if constexpr (KVF == 1) decode_attn_body<NT, SLOTS, KvBf16, true>(p);
  else decode_attn_body<NT, SLOTS, KvF32, true>(p);
}

int decode_attn_nsplit(int B, int H) {
  const int wgs = B * H;
  // (bf16 cache, 320 workgroups: two / three key pieces per (utterance, head) measured 185 / 215 ms per step against 156 unsplit)
  return wgs <= 128 ? std::max(1, std::min(16, 256 / wgs)) : 1;
}

// Workgroups per (row, head) in the batch-invariant mode: as many as the key split would use at this batch size, and no more than the
// longest row the cache can hold has pieces.  Only the parallelism follows B; the pieces follow the row (decode_attn_pieces).
int decode_attn_inv_wgs(int B, int H, int Smax) { return std::min(decode_attn_nsplit(B, H), decode_attn_pieces(std::max(Smax, 1))); }

int decode_attn_forward(const DecodeAttnArgs& a, hipStream_t stream) {
  IDX_CHECK(a.qkv_part && a.kcache && a.vcache && (a.out || a.out_row) && (a.st || a.slot), "null pointer");
  IDX_CHECK(a.d == a.H * 64, "head_dim must be 64");
  IDX_CHECK(a.kv_fmt >= 0 && a.kv_fmt <= 2 && (a.kv_fmt != 2 || (a.kscale && a.vscale)), "KV format 0 / 1 / 2 (2: with the scale arrays)");
  constexpr int nt = 512;      // 512 threads measured 4 % faster than 256 (profiles/README.md)
  const size_t lds = (size_t)(256 + (nt / (a.kv_fmt ? 8 : 16)) * 64 + a.Smax) * sizeof(float);
  IDX_CHECK(lds <= 128 * 1024, "Smax too large for the LDS score buffer");
  static DynLdsLimit lds_limit;
  IDX_HIP(lds_limit.set(128 * 1024, decode_attn_kernel<512, false>, decode_attn16_kernel<512, false>, decode_attn8_kernel<512, false>,
                        decode_attn_kernel<512, true>, decode_attn16_kernel<512, true>, decode_attn8_kernel<512, true>));
  IDX_CHECK(a.nsplit >= 1 && a.nsplit <= 16 && (a.nsplit == 1 || (a.part && a.cnt)), "key split: 1..16 pieces, partial buffer and counters");
  // algorithmic bytes: K and V of every cached position, all heads: B * S * 2 * d * (4 | 2 | 1), fp8: + two fp32 scales per 64 (S as
  // the host knows it: pos_hint)
  static const int cat = prof_register("decode_attn_kernel"), cat16 = prof_register("decode_attn16_kernel");
  int cat_of = a.kv_fmt ? cat16 : cat;
  if (a.kv_fmt == 2) {      // (registered at its first use: a profile of the other formats lists what it always listed)
    static const int cat8 = prof_register("decode_attn8_kernel");
    cat_of = cat8;
  }
  const double bytes_per = a.kv_fmt == 2 ? 2.0 + 8.0 / 64.0 : a.kv_fmt ? 4.0 : 8.0;
  ProfScope prof(cat_of, stream, 0.0, bytes_per * a.B * (double)a.pos_hint * a.d);
  const dim3 grid(a.H, a.B, a.nsplit);
  if (a.invariant) {
    IDX_CHECK(a.part && a.cnt, "batch-invariant attention: partial buffer and counters");
    static DynLdsLimit inv_limit;
    IDX_HIP(inv_limit.set(128 * 1024, decode_attn_inv_kernel<512, false, 0>, decode_attn_inv_kernel<512, false, 1>,
                          decode_attn_inv_kernel<512, false, 2>, decode_attn_inv_kernel<512, true, 0>,
                          decode_attn_inv_kernel<512, true, 1>, decode_attn_inv_kernel<512, true, 2>));
    if (a.slot) {
      if (a.kv_fmt == 2) hipLaunchKernelGGL((decode_attn_inv_kernel<512, true, 2>), grid, dim3(512), lds, stream, a);
      else if (a.kv_fmt) hipLaunchKernelGGL((decode_attn_inv_kernel<512, true, 1>), grid, dim3(512), lds, stream, a);
      else hipLaunchKernelGGL((decode_attn_inv_kernel<512, true, 0>), grid, dim3(512), lds, stream, a);
    } else {
      if (a.kv_fmt == 2) hipLaunchKernelGGL((decode_attn_inv_kernel<512, false, 2>), grid, dim3(512), lds, stream, a);
      else if (a.kv_fmt) hipLaunchKernelGGL((decode_attn_inv_kernel<512, false, 1>), grid, dim3(512), lds, stream, a);
      else hipLaunchKernelGGL((decode_attn_inv_kernel<512, false, 0>), grid, dim3(512), lds, stream, a);
    }
    IDX_LAUNCH_CHECK();
    return 0;
  }
  if (a.slot) {
    if (a.kv_fmt == 2) hipLaunchKernelGGL((decode_attn8_kernel<512, true>), grid, dim3(512), lds, stream, a);
    else if (a.kv_fmt) hipLaunchKernelGGL((decode_attn16_kernel<512, true>), grid, dim3(512), lds, stream, a);
    else hipLaunchKernelGGL((decode_attn_kernel<512, true>), grid, dim3(512), lds, stream, a);
  } else {
    if (a.kv_fmt == 2) hipLaunchKernelGGL((decode_attn8_kernel<512, false>), grid, dim3(512), lds, stream, a);
    else if (a.kv_fmt) hipLaunchKernelGGL((decode_attn16_kernel<512, false>), grid, dim3(512), lds, stream, a);
    else hipLaunchKernelGGL((decode_attn_kernel<512, false>), grid, dim3(512), lds, stream, a);
  }
  IDX_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Row b of the greedy samplers: logits (split-K partial sum + bias, optionally recorded) -> repetition penalty -> argmax, the first
// maximum on ties.  The result is valid in thread 0 only (rv / ri: [16] of shared scratch).
__device__ __forceinline__ void greedy_row_argmax(const SampleArgs& p, const int b, const int tid, float* rv, int* ri, float& best_out,
                                                  int& bidx_out) {
  const int wave = tid >> 6, lane = tid & 63;
  const int V = p.V;
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  const unsigned char* seen = p.seen + (size_t)b * V;
  const size_t sst = (size_t)p.part_rows * V;
  const float* prow = p.part + (size_t)b * V;
  for (int v0 = tid; v0 < V; v0 += 4096) {       // 4 vocabulary entries per trip, all their slab loads in flight together
    float l4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = v0 + 1024 * u;
      l4[u] = (v < V && p.bias) ? p.bias[v] : 0.0f;
    }
    for (int s = 0; s < p.parts; ++s) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int v = v0 + 1024 * u;
        if (v < V) l4[u] += prow[(size_t)s * sst + v];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = v0 + 1024 * u;
      if (v >= V) continue;
      float l = l4[u];
      if (p.logits_out) p.logits_out[(size_t)b * V + v] = l;
      if (seen[v]) l = l < 0.f ? l * p.penalty : l / p.penalty;
      if (l > best) { best = l; bidx = v; }      // ascending v per thread: strict > keeps the first maximum
    }
  }
  wave_argmax(best, bidx);
  if (lane == 0) { rv[wave] = best; ri[wave] = bidx; }
  __syncthreads();
  if (tid == 0) argmax_take_waves<16>(best, bidx, rv, ri);
  best_out = best;
  bidx_out = bidx;
}

// Scores (SampleArgs::logprob_out, idxtts.h "Scores"): the log-probability of token `tok` (workgroup-uniform) under row b's raw logits,
// lp = (l[tok] - m) - logf(S) with m = max_v l[v] and S = sum_v expf(l[v] - m); valid in every thread of the 1024.  A pass of its own
// behind the sampler, in the kernels' LP = true instantiations only: with scores off the kernels of before run, instruction for instruction.  It RE-SUMS the slab
// (no row values are kept in registers: greedy_row_argmax holds four per trip and has no bound on V): l[v] is rebuilt as the samplers
// build it -- the bias (or 0), then the split-K parts in ascending order -- so it is bit for bit the value logits_out records, and the
// row's 4 V bytes per part come from L2 the second and third time.  m first; then S in an order that depends on V and the workgroup
// size alone: every thread its own ids tid, tid + 1024, ... ascending, the wave butterfly, the waves in ascending order (block_sum).
// Neither B, the slot, nor the sampler mode enters; parts only through l[v] itself.  red: [16] of shared scratch.
// Registers and occupancy (hipcc --offload-arch=gfx950 -save-temps; 1024-thread workgroups, so at most 2 per CU either way):
//   LP = false as before (22, 22, 66, 67 VGPRs); LP = true: sample_greedy_kernel and sample_slots_kernel 32 VGPRs, occupancy 8 as
//   before; sample_warp_kernel 68, sample_slots_warp_kernel 67, occupancy 7 as before; no scratch in any of them.
__device__ __forceinline__ float row_logit(const SampleArgs& p, const int b, const int v) {
  float l = p.bias ? p.bias[v] : 0.0f;
  const float* prow = p.part + (size_t)b * p.V + v;
  const size_t sst = (size_t)p.part_rows * p.V;
  for (int s = 0; s < p.parts; ++s) l += prow[(size_t)s * sst];
  return l;
}
__device__ __forceinline__ float row_logprob(const SampleArgs& p, const int b, const int tok, const int tid, float* red) {
  const int V = p.V;
  float m = -INFINITY;
  for (int v = tid; v < V; v += 1024) m = fmaxf(m, row_logit(p, b, v));
  m = block_max<16>(m, red);
  float part = 0.f;
  for (int v = tid; v < V; v += 1024) part += expf(row_logit(p, b, v) - m);
  const float S = block_sum<16>(part, red);
  return (row_logit(p, b, tok) - m) - logf(S);
}

// Row b's next input x = mel_emb[tok] + mel_pos[mel_pos], by all 1024 threads of a sampler's workgroup: A-fragment images for the
// fp32-MFMA GEMV step (the folded LayerNorm's statistics are computed by the consumer), or a row + its statistics for the plane GEMV
// (NT threads; session_resume_slot rebuilds a resumed row's input with it)
template <int NT>
__device__ __forceinline__ void write_next_input(const SampleArgs::Embed& em, const int B, const int b, const int tok, const int mel_pos,
                                                 const int tid) {
  if (em.x_frag) {
    const int d = em.d;
    for (int e = tid; e < d; e += NT) em.x_frag[frag_index(b, e, d >> 4)] = em.mel_emb[(size_t)tok * d + e] + em.mel_pos[(size_t)mel_pos * d + e];
  } else {
    embed_row_pl<NT>(em.x_row, em.x_stats, b, B, em.d, em.mel_emb, em.mel_pos, tok, mel_pos, tid);
  }
}

// LP (every sampler kernel): scores are recorded (p.logprob_out set).  The LP = false instantiations are the kernels of before.
template <bool LP>
__global__ __launch_bounds__(1024) void sample_greedy_kernel(const SampleArgs p) {
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ int s_tok, s_code;
  const bool fused = p.embed.x_row || p.embed.x_frag;
  const int mp_next = fused ? p.st->mel_pos + 1 : 0;      // read before anybody can advance the state
  const int b = blockIdx.x, tid = threadIdx.x;
  float best;
  int bidx;
  greedy_row_argmax(p, b, tid, rv, ri, best, bidx);
  int step = 0;      // (thread 0's)
  if (tid == 0) {
    const bool pad = p.finished[b] != 0;
    int tok = pad ? p.stop_token : bidx;      // finished rows emit pad (= eos = stop token)
    step = p.st->step;
    p.codes[(size_t)b * p.codes_ld + step] = tok;
    if (LP) s_code = pad ? -1 : tok;      // what the scores describe: the code just written, not a forced token
    if (p.forced) tok = (int)p.forced[(size_t)b * p.forced_ld + step];      // teacher forcing: the given token continues the sequence
    p.seen[(size_t)b * p.V + tok] = 1;
    if (tok == p.stop_token) p.finished[b] = 1;
    p.cur_tok[b] = tok;
    s_tok = tok;
  }
  if (LP) {      // (before this workgroup's arrival below, so `step` is still this launch's)
    __syncthreads();
    const int code = s_code;
    const float lp = code < 0 ? 0.0f : row_logprob(p, b, code, tid, rv);
    if (tid == 0) p.logprob_out[(size_t)b * p.logprob_ld + step] = lp;
  }
  if (!fused) return;
  __syncthreads();
  write_next_input<1024>(p.embed, p.B, b, s_tok, mp_next, tid);
  __syncthreads();      // every read of the step scalars by this workgroup is behind us
  // (not wg_arrive_last: this workgroup hands over no stores, so there is no wait in front and nothing to return behind)
  if (tid == 0) {
    DecodeState* st = p.embed.st_rw;
    const unsigned old = __hip_atomic_fetch_add(&st->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == gridDim.x - 1u) {      // everybody has read pos / mel_pos / step: advance them for the next launch
      __hip_atomic_store(&st->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->pos += 1; st->mel_pos += 1; st->step += 1;
    }
  }
}

int sample_greedy_forward(const SampleArgs& a, hipStream_t stream) {
  IDX_CHECK(a.part && a.seen && a.finished && a.codes && a.cur_tok && a.st, "null pointer");
  static const int cat = prof_register("sample_greedy_kernel");
  ProfScope prof(cat, stream, 0.0, 4.0 * a.B * (double)a.V * (a.parts + 1));
  if (a.logprob_out) hipLaunchKernelGGL(sample_greedy_kernel<true>, dim3(a.B), dim3(1024), 0, stream, a);
  else hipLaunchKernelGGL(sample_greedy_kernel<false>, dim3(a.B), dim3(1024), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// Scoring given codes (idxtts.h): workgroup r reduces row r of a logits slab [rows][V] to the log-probability of the row's given code
// tok[r] and writes it to out[dst[r]] -- the samplers' geometry and their row_logprob, so a teacher-forced value is summed in the order
// a sampler would have recorded it.  tok[r] < 0 marks a row that is not scored: 0 is written and the row's logits are not read.
// Registers and occupancy (hipcc --offload-arch=gfx950 -save-temps): 30 VGPRs, 29 SGPRs, no scratch, 64 bytes of LDS; occupancy 8, so
// the 1024-thread workgroup size alone bounds it at 2 workgroups per CU (the LP = true greedy sampler: 32 VGPRs, the same occupancy).
__global__ __launch_bounds__(1024) void score_rows_kernel(const ScoreRowsArgs a) {
  __shared__ float red[16];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int tok = a.tok[r];      // (workgroup-uniform)
  float lp = 0.0f;
  if (tok >= 0) {
    SampleArgs p;
    p.part = a.logits; p.parts = 1; p.part_rows = a.rows; p.V = a.V;
    lp = row_logprob(p, r, min(tok, a.V - 1), tid, red);      // (inside the row whatever the caller holds: the host has checked)
  }
  if (tid == 0) a.out[a.dst[r]] = lp;
}

int score_rows_forward(const ScoreRowsArgs& a, hipStream_t stream) {
  IDX_CHECK(a.logits && a.tok && a.dst && a.out, "null pointer");
  IDX_CHECK(a.rows >= 1 && a.rows <= 64 && a.V >= 1, "score rows: 1 <= rows <= 64");
  static const int cat = prof_register("score_rows_kernel");
  ProfScope prof(cat, stream, 0.0, 4.0 * a.rows * (double)a.V);
  hipLaunchKernelGGL(score_rows_kernel, dim3(a.rows), dim3(1024), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Decode session (continuous batching): the greedy tail with per-slot state (SlotState, decode.h)

// The tail of a session sampler, once thread 0 holds the slot's token: record it, then end the slot (stop token or cap) or write its
// next input row and advance its own scalars.  s_tok / s_mp / s_end: shared scratch; red: [16] floats of it (scores only).
template <bool LP>
__device__ __forceinline__ void slot_tail(const SampleArgs& p, SlotState* const ss, const int b, const int tid, const int token, int& s_tok,
                                          int& s_mp, int& s_end, float* red) {
  int step = 0;      // (thread 0's)
  if (tid == 0) {
    const int tok = token;
    step = ss->step;
    p.codes[(size_t)b * p.codes_ld + step] = tok;
    p.seen[(size_t)b * p.V + tok] = 1;
    p.cur_tok[b] = tok;
    s_tok = tok;
    s_mp = ss->mel_pos + 1;
    s_end = tok == p.stop_token || step + 1 >= ss->max_step;
  }
  __syncthreads();
  if (LP) {
    const float lp = row_logprob(p, b, s_tok, tid, red);
    if (tid == 0) p.logprob_out[(size_t)b * p.logprob_ld + step] = lp;
  }
  if (s_end) {      // the stop token (recorded) or the slot's cap: the slot retires; step = codes produced
    if (tid == 0) { ss->step += 1; ss->live = 0; }
    return;
  }
  write_next_input<1024>(p.embed, p.B, b, s_tok, s_mp, tid);
  if (tid == 0) { ss->pos += 1; ss->mel_pos += 1; ss->step += 1; }      // this slot's scalars: nobody else reads them in this launch
}

template <bool LP>
__global__ __launch_bounds__(1024) void sample_slots_kernel(const SampleArgs p, SlotState* slots, const int* slot_ids) {
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ int s_tok, s_mp, s_end;
  const int b = slot_ids ? slot_ids[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
  SlotState* const ss = slots + b;
  if (!ss->live) return;      // free or ended slot: nothing is read or written (workgroup-uniform)
  float best;
  int bidx;
  greedy_row_argmax(p, b, tid, rv, ri, best, bidx);
  slot_tail<LP>(p, ss, b, tid, bidx, s_tok, s_mp, s_end, rv);
}

int sample_slots_forward(const SampleArgs& a, SlotState* slots, const int* slot_ids, int n, hipStream_t stream) {
  IDX_CHECK(a.part && a.seen && a.codes && a.cur_tok && slots && (a.embed.x_row || a.embed.x_frag) && a.embed.mel_emb && a.embed.mel_pos,
            "null pointer");
  IDX_CHECK(!a.forced && !a.logits_out, "decode sessions are greedy only");
  if (n <= 0) return 0;
  static const int cat = prof_register("sample_slots_kernel");
  ProfScope prof(cat, stream, 0.0, 4.0 * n * (double)a.V * (a.parts + 1));
  if (a.logprob_out) hipLaunchKernelGGL(sample_slots_kernel<true>, dim3(n), dim3(1024), 0, stream, a, slots, slot_ids);
  else hipLaunchKernelGGL(sample_slots_kernel<false>, dim3(n), dim3(1024), 0, stream, a, slots, slot_ids);
  IDX_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// multinomial sampling with the HF warpers / the accel-engine sampler (SampleWarpArgs, decode.h)
constexpr int SW_NPT = 16;          // vocabulary entries per thread: V <= 16384
// Survivors of the top-k filter that the top-p stage (top_p < 1 only) can sort.  Its callers require 0 < top_k <= 1024 there, so the
// survivors are top_k plus the other entries equal to the k-th largest score: more than SW_CAP only when over SW_CAP - top_k + 1
// scores tie exactly at the threshold, and then the ones that arrive after the first SW_CAP are dropped (HF's own sort leaves the
// order inside such a group unspecified too).  Without top-p nothing is staged and nothing is capped.
constexpr int SW_CAP = 2048;

// Row b of the warped sampler (parts = 1; the penalty in HF mode only): the token, valid in every thread.  The draw for id v is
// exp1_draw(noise, seed, nbase + v).  rv / ri: [16], sval / sidx / sorted_v / sorted_i: [SW_CAP] of shared scratch.
__device__ __forceinline__ int warp_row_token(const SampleArgs& p, const int b, const int mode, const float temperature, const int top_k,
                                              const float top_p, const float* noise, const unsigned long long seed, const size_t nbase,
                                              const int tid, float* rv, int* ri, float* sval, int* sidx, float* sorted_v, int* sorted_i,
                                              int& s_count, int& s_keep_from, float& s_sum) {
  const int V = p.V;
  const unsigned char* seen = p.seen + (size_t)b * V;
  const float* prow = p.part + (size_t)b * V;
  auto draw = [&](int v) { return exp1_draw(noise, seed, nbase + v); };

  // ---- scores: logits -> (repetition penalty) -> / temperature ----
  float sc[SW_NPT];
#pragma unroll
  for (int u = 0; u < SW_NPT; ++u) {
    const int v = tid + 1024 * u;
    float l = -INFINITY;
    if (v < V) {
      l = prow[v] + (p.bias ? p.bias[v] : 0.0f);
      if (p.logits_out) p.logits_out[(size_t)b * V + v] = l;
      if (mode == SAMPLE_HF && p.penalty != 1.0f && seen[v]) l = l < 0.f ? l * p.penalty : l / p.penalty;
      if (temperature != 1.0f) l = l / temperature;
    }
    sc[u] = l;
  }

  // ---- top-k (HF): the k-th largest value (with multiplicity) by k rounds of block-wide max extraction; everything strictly below
  //      it becomes -inf, ties at the threshold stay ----
  if (mode == SAMPLE_HF && top_k > 0 && top_k < V) {
    unsigned taken = 0;
    float kth = -INFINITY;
    for (int r = 0; r < top_k; ++r) {
      float mx = -INFINITY; int mi = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < SW_NPT; ++u) {
        const int v = tid + 1024 * u;
        if (v < V && !((taken >> u) & 1u) && (sc[u] > mx || (sc[u] == mx && v < mi))) { mx = sc[u]; mi = v; }
      }
      block_argmax<16>(mx, mi, rv, ri, tid);
      kth = mx;
      if ((mi & 1023) == tid && mi < V) taken |= 1u << (mi >> 10);
    }
#pragma unroll
    for (int u = 0; u < SW_NPT; ++u) if (sc[u] < kth) sc[u] = -INFINITY;
  }

  int token;
  if (mode == SAMPLE_ACCEL || top_p >= 1.0f) {
    // no top-p, so nothing needs sorting: softmax over the row as it stands in the registers (a filtered entry is -inf and weighs 0,
    // whatever top_k is and however many entries tie at its threshold), divided by the (accel sampler: clamped) noise, argmax
    const float qmin = mode == SAMPLE_ACCEL ? 1e-10f : 0.0f;
    float mx = -INFINITY; int mi = 0;
#pragma unroll
    for (int u = 0; u < SW_NPT; ++u) if (sc[u] > mx) { mx = sc[u]; mi = tid + 1024 * u; }
    block_argmax<16>(mx, mi, rv, ri, tid);
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < SW_NPT; ++u) if (tid + 1024 * u < V) part += expf(sc[u] - mx);
    const float tot = block_sum<16>(part, rv);
    float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < SW_NPT; ++u) {
      const int v = tid + 1024 * u;
      if (v < V) {
        const float r = (expf(sc[u] - mx) / tot) / fmaxf(draw(v), qmin);
        if (r > best) { best = r; bi = v; }
      }
    }
    block_argmax<16>(best, bi, rv, ri, tid);
    token = bi;
  } else {
    // ---- top-p: survivors of the top-k filter -> LDS (finite scores only: -inf has probability 0 and sorts first).  Survivor
    //      number SW_CAP and later (in arrival order) is dropped; the host rule for top_p < 1, 0 < top_k <= 1024 (check_sampling),
    //      leaves that to a tie group of more than SW_CAP - top_k + 1 entries at the top-k threshold ----
    if (tid == 0) s_count = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SW_NPT; ++u) {
      const int v = tid + 1024 * u;
      if (v < V && sc[u] > -INFINITY) {
        const int slot = atomicAdd(&s_count, 1);
        if (slot < SW_CAP) { sval[slot] = sc[u]; sidx[slot] = v; }
      }
    }
    __syncthreads();
    const int n = min(s_count, SW_CAP);
    // rank sort, ascending by (value, index)
    for (int e = tid; e < n; e += 1024) {
      const float ve = sval[e]; const int ie = sidx[e];
      int rank = 0;
      for (int o = 0; o < n; ++o) rank += (sval[o] < ve || (sval[o] == ve && sidx[o] < ie)) ? 1 : 0;
      sorted_v[rank] = ve; sorted_i[rank] = ie;
    }
    __syncthreads();
    // ---- top-p on the ascending list: softmax, running sum, remove while cum <= 1 - top_p (never the last one) ----
    if (tid == 0) {
      int keep_from = 0;
      const float mx = sorted_v[n - 1];
      if (top_p < 1.0f) {
        float tot = 0.f;
        for (int e = 0; e < n; ++e) tot += expf(sorted_v[e] - mx);
        const float thr = (float)(1.0 - (double)top_p);
        float cum = 0.f;
        for (int e = 0; e < n - 1; ++e) {
          cum += expf(sorted_v[e] - mx) / tot;
          if (cum <= thr) keep_from = e + 1; else break;
        }
      }
      float tot2 = 0.f;      // softmax denominator of the warped scores
      for (int e = keep_from; e < n; ++e) tot2 += expf(sorted_v[e] - mx);
      s_keep_from = keep_from;
      s_sum = tot2;
    }
    __syncthreads();
    // ---- multinomial == argmax(probs / q) over the kept tokens ----
    const float mx = sorted_v[n - 1];
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int e = s_keep_from + tid; e < n; e += 1024) {
      const int v = sorted_i[e];
      const float r = (expf(sorted_v[e] - mx) / s_sum) / draw(v);
      if (r > best || (r == best && v < bi)) { best = r; bi = v; }
    }
    block_argmax<16>(best, bi, rv, ri, tid);
    token = bi;
  }
  return token;
}

template <bool LP>
__global__ __launch_bounds__(1024) void sample_warp_kernel(const SampleWarpArgs q) {
  const SampleArgs& p = q.base;
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ float sval[SW_CAP];
  __shared__ int sidx[SW_CAP];
  __shared__ float sorted_v[SW_CAP];
  __shared__ int sorted_i[SW_CAP];
  __shared__ int s_count, s_keep_from;
  __shared__ float s_sum;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V;
  const bool own = p.invariant && !q.exp_noise;      // the row's own stream (SampleArgs::invariant)
  const size_t nbase = own ? (size_t)p.st->step * V : ((size_t)p.st->step * p.B + b) * V;
  const unsigned long long seed = own ? q.seed + DRAW_ROW_STRIDE * (unsigned long long)b : q.seed;
  const int token = warp_row_token(p, b, q.mode, q.temperature, q.top_k, q.top_p, q.exp_noise, seed, nbase, tid, rv, ri, sval, sidx,
                                   sorted_v, sorted_i, s_count, s_keep_from, s_sum);
  if (LP) {      // (every thread reads finished[b] before the barriers inside, thread 0 sets it after them)
    const float lp = p.finished[b] ? 0.0f : row_logprob(p, b, token, tid, rv);
    if (tid == 0) p.logprob_out[(size_t)b * p.logprob_ld + p.st->step] = lp;
  }
  if (tid == 0) {
    const int tok = p.finished[b] ? p.stop_token : token;
    p.codes[(size_t)b * p.codes_ld + p.st->step] = tok;
    p.seen[(size_t)b * V + tok] = 1;
    if (tok == p.stop_token) p.finished[b] = 1;
    p.cur_tok[b] = tok;
  }
}

int sample_warp_forward(const SampleWarpArgs& a, hipStream_t stream) {
  const SampleArgs& b = a.base;
  IDX_CHECK(b.part && b.parts == 1 && b.seen && b.finished && b.codes && b.cur_tok && b.st, "null pointer");
  IDX_CHECK(b.V > 0 && b.V <= 1024 * SW_NPT, "vocabulary size");
  IDX_CHECK(a.temperature > 0.0f && a.top_k >= 0 && a.top_p > 0.0f, "sampling parameters");
  IDX_CHECK(a.mode == SAMPLE_HF || a.mode == SAMPLE_ACCEL, "sampling mode");
  static const int cat = prof_register("sample_warp_kernel");
  ProfScope prof(cat, stream, 0.0, 8.0 * b.B * (double)b.V);
  if (b.logprob_out) hipLaunchKernelGGL(sample_warp_kernel<true>, dim3(b.B), dim3(1024), 0, stream, a);
  else hipLaunchKernelGGL(sample_warp_kernel<false>, dim3(b.B), dim3(1024), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// Decode session with per-request sampling: sample_slots_kernel with the sampler of each slot's own SlotSampling row -- greedy_row_argmax
// (mode 0) or the warped sampler of sample_warp_kernel, whose draws for the slot's step t are the request's noise row t, or the
// counter-based stream at row 0 of a `p.B`-row generation (independent of the slot id)
template <bool LP>
__global__ __launch_bounds__(1024) void sample_slots_warp_kernel(const SampleArgs p, SlotState* slots, const SlotSampling* samp,
                                                                 const int* slot_ids) {
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ float sval[SW_CAP];
  __shared__ int sidx[SW_CAP];
  __shared__ float sorted_v[SW_CAP];
  __shared__ int sorted_i[SW_CAP];
  __shared__ int s_count, s_keep_from;
  __shared__ float s_sum;
  __shared__ int s_tok, s_mp, s_end;
  const int b = slot_ids ? slot_ids[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
  SlotState* const ss = slots + b;
  if (!ss->live) return;      // free or ended slot (workgroup-uniform)
  const SlotSampling sp = samp[b];
  int token;
  if (sp.mode == 0) {
    float best;
    greedy_row_argmax(p, b, tid, rv, ri, best, token);
  } else {
    const size_t t = (size_t)ss->step;      // read before any thread can reach slot_tail's update (the warper synchronises first)
    const size_t nbase = (sp.exp_noise || p.invariant) ? t * p.V : t * p.B * p.V;
    token = warp_row_token(p, b, sp.mode, sp.temperature, sp.top_k, sp.top_p, sp.exp_noise, sp.seed, nbase, tid, rv, ri, sval, sidx,
                           sorted_v, sorted_i, s_count, s_keep_from, s_sum);
  }
  slot_tail<LP>(p, ss, b, tid, token, s_tok, s_mp, s_end, rv);
}

int sample_slots_warp_forward(const SampleArgs& a, SlotState* slots, const SlotSampling* samp, const int* slot_ids, int n,
                              hipStream_t stream) {
  IDX_CHECK(a.part && a.parts == 1 && a.seen && a.codes && a.cur_tok && slots && samp && (a.embed.x_row || a.embed.x_frag) &&
            a.embed.mel_emb && a.embed.mel_pos, "null pointer");
  IDX_CHECK(!a.forced && !a.logits_out, "decode sessions record no logits and take no forced tokens");
  IDX_CHECK(a.V > 0 && a.V <= 1024 * SW_NPT, "vocabulary size");
  if (n <= 0) return 0;
  static const int cat = prof_register("sample_slots_warp_kernel");
  ProfScope prof(cat, stream, 0.0, 8.0 * n * (double)a.V);
  if (a.logprob_out) hipLaunchKernelGGL(sample_slots_warp_kernel<true>, dim3(n), dim3(1024), 0, stream, a, slots, samp, slot_ids);
  else hipLaunchKernelGGL(sample_slots_warp_kernel<false>, dim3(n), dim3(1024), 0, stream, a, slots, samp, slot_ids);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ void advance_state_kernel(DecodeState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { st->pos += 1; st->mel_pos += 1; st->step += 1; }
}

int advance_state(DecodeState* st, hipStream_t stream) {
  hipLaunchKernelGGL(advance_state_kernel, dim3(1), dim3(64), 0, stream, st);
  IDX_LAUNCH_CHECK();
  return 0;
}

// qkv [B][S][3d] (token-major, after bias) -> K/V caches, positions [0, S)
template <bool KV16>
__global__ __launch_bounds__(256) void kv_store_prefill_kernel(float* qkv, void* kcache, void* vcache, int B, int H, int S, int Smax, int d) {
  const int s = blockIdx.x, b = blockIdx.y;
  float* row = qkv + ((size_t)b * S + s) * 3 * d;
  for (int col = threadIdx.x; col < d; col += 256) {
    const int h = col >> 6, dd = col & 63;
    if (KV16) {      // bf16 cache; the fp32 row keeps the rounded values for the prefill attention
      const unsigned kb = bf16_rne_bits(row[d + col]), vb = bf16_rne_bits(row[2 * d + col]);
      static_cast<unsigned short*>(kcache)[(((size_t)(b * H + h) * 8 + (dd >> 3)) * Smax + s) * 8 + (dd & 7)] = (unsigned short)kb;
      static_cast<unsigned short*>(vcache)[((size_t)(b * H + h) * Smax + s) * 64 + dd] = (unsigned short)vb;
      row[d + col] = __uint_as_float(kb << 16);
      row[2 * d + col] = __uint_as_float(vb << 16);
    } else {
      static_cast<float*>(kcache)[(((size_t)(b * H + h) * 16 + (dd >> 2)) * Smax + s) * 4 + (dd & 3)] = row[d + col];
      static_cast<float*>(vcache)[((size_t)(b * H + h) * Smax + s) * 64 + dd] = row[2 * d + col];
    }
  }
}

// scaled fp8 cache (kv_fp8.h): one wave owns one head -- a vector's scale needs the maximum over its 64 lanes -- and takes the heads
// wave, wave + 4, ...; k / v columns of qkv become the cached values in place.  slot_ids / len null: the prefill (row b -> cache row b,
// every position); else the admission rule of kv_store_slots_kernel (positions [0, len[b]) -> slot slot_ids[b], FAN: and the next
// fan - 1 slots, codes and scales alike)
template <bool FAN>
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(float* qkv, unsigned char* kcache, unsigned char* vcache, float* kscale,
                                                           float* vscale, int H, int S, int Smax, int d, const int* slot_ids,
                                                           const int* len, int fan, const int* first) {
  const int s = blockIdx.x, b = blockIdx.y, wave = threadIdx.x >> 6, dd = threadIdx.x & 63;
  const int slot0 = slot_ids ? slot_ids[FAN && first ? first[b] : b] : b;
  const int* const list = FAN && first ? slot_ids + first[b] : nullptr;      // takes: the row's own slot list
  if (list) fan = first[b + 1] - first[b];
  const bool keep = !len || s < len[b];
  float* row = qkv + ((size_t)b * S + s) * 3 * d;
  for (int h = wave; h < H; h += 4) {      // (wave-uniform: every lane of a wave reaches the quantiser's reduction)
    const int col = h * 64 + dd;
    unsigned kcode, vcode;
    float ks, vs;
    const float kq = kv_fp8_quantize_lane(row[d + col], kcode, ks), vq = kv_fp8_quantize_lane(row[2 * d + col], vcode, vs);
    if (keep) {
      auto put = [&](int slot) {
        const size_t vec = (size_t)slot * H + h;
        kcache[((vec * 8 + (dd >> 3)) * Smax + s) * 8 + (dd & 7)] = (unsigned char)kcode;
        vcache[(vec * Smax + s) * 64 + dd] = (unsigned char)vcode;
        if (dd == 0) { kscale[vec * Smax + s] = ks; vscale[vec * Smax + s] = vs; }
      };
      if (FAN) for (int j = 0; j < fan; ++j) put(list ? list[j] : slot0 + j);
      else put(slot0);
    }
    row[d + col] = kq;
    row[2 * d + col] = vq;
  }
}

static int kv_store_fp8(float* qkv, const KvDst& kv, int n, int H, int S, int Smax, int d, const int* slot_ids, const int* len, int fan,
                        hipStream_t stream, const int* first = nullptr) {
  IDX_CHECK(kv.kscale && kv.vscale, "the fp8 cache needs its scale arrays");
  unsigned char* const kc = static_cast<unsigned char*>(kv.kcache);
  unsigned char* const vc = static_cast<unsigned char*>(kv.vcache);
  if (fan > 1 || first) hipLaunchKernelGGL(kv_store_fp8_kernel<true>, dim3(S, n), dim3(256), 0, stream, qkv, kc, vc, kv.kscale, kv.vscale, H, S, Smax, d, slot_ids, len, fan, first);
  else hipLaunchKernelGGL(kv_store_fp8_kernel<false>, dim3(S, n), dim3(256), 0, stream, qkv, kc, vc, kv.kscale, kv.vscale, H, S, Smax, d, slot_ids, len, 1, nullptr);
  IDX_LAUNCH_CHECK();
  return 0;
}

int kv_store_prefill(float* qkv, const KvDst& kv, int B, int H, int S, int Smax, int d, hipStream_t stream) {
  IDX_CHECK(S <= Smax, "prefill longer than the cache");
  static const int cat = prof_register("kv_store_prefill_kernel");
  ProfScope prof(cat, stream, 0.0, (kv.fmt == 2 ? 26.0 : kv.fmt ? 28.0 : 16.0) * B * (double)S * d);
  if (kv.fmt == 2) return kv_store_fp8(qkv, kv, B, H, S, Smax, d, nullptr, nullptr, 1, stream);
  if (kv.fmt) hipLaunchKernelGGL(kv_store_prefill_kernel<true>, dim3(S, B), dim3(256), 0, stream, qkv, kv.kcache, kv.vcache, B, H, S, Smax, d);
  else hipLaunchKernelGGL(kv_store_prefill_kernel<false>, dim3(S, B), dim3(256), 0, stream, qkv, kv.kcache, kv.vcache, B, H, S, Smax, d);
  IDX_LAUNCH_CHECK();
  return 0;
}

// decode-session admission: prefill row b (right-padded, S positions) -> the cache rows of slot slot_ids[b], positions [0, len[b]);
// FAN: to several slots -- first null (beam sessions): the `fan` consecutive slots slot_ids[b] .. slot_ids[b] + fan - 1 (a group's beams
// start identical); else (takes) the row's own list slot_ids[first[b]] .. slot_ids[first[b + 1] - 1], in any order
template <bool KV16, bool FAN>
__global__ __launch_bounds__(256) void kv_store_slots_kernel(float* qkv, void* kcache, void* vcache, int H, int S, int Smax, int d,
                                                             const int* slot_ids, const int* len, int fan, const int* first) {
  const int s = blockIdx.x, b = blockIdx.y;
  const int* const list = FAN && first ? slot_ids + first[b] : nullptr;
  const int slot0 = list ? list[0] : slot_ids[b];
  if (list) fan = first[b + 1] - first[b];
  const bool keep = s < len[b];
  float* row = qkv + ((size_t)b * S + s) * 3 * d;
  for (int col = threadIdx.x; col < d; col += 256) {
    const int h = col >> 6, dd = col & 63;
    if (KV16) {      // every row is rounded (as kv_store_prefill does): the prefill attention sees the cached values
      const unsigned kb = bf16_rne_bits(row[d + col]), vb = bf16_rne_bits(row[2 * d + col]);
      if (keep) {
        auto put = [&](int slot) {
          static_cast<unsigned short*>(kcache)[(((size_t)(slot * H + h) * 8 + (dd >> 3)) * Smax + s) * 8 + (dd & 7)] = (unsigned short)kb;
          static_cast<unsigned short*>(vcache)[((size_t)(slot * H + h) * Smax + s) * 64 + dd] = (unsigned short)vb;
        };
        if (FAN) for (int j = 0; j < fan; ++j) put(list ? list[j] : slot0 + j);
        else put(slot0);
      }
      row[d + col] = __uint_as_float(kb << 16);
      row[2 * d + col] = __uint_as_float(vb << 16);
    } else if (keep) {
      auto put = [&](int slot) {
        static_cast<float*>(kcache)[(((size_t)(slot * H + h) * 16 + (dd >> 2)) * Smax + s) * 4 + (dd & 3)] = row[d + col];
        static_cast<float*>(vcache)[((size_t)(slot * H + h) * Smax + s) * 64 + dd] = row[2 * d + col];
      };
      if (FAN) for (int j = 0; j < fan; ++j) put(list ? list[j] : slot0 + j);
      else put(slot0);
    }
  }
}

int kv_store_slots(float* qkv, const KvDst& kv, int n, int H, int S, int Smax, int d, const int* slot_ids, const int* len,
                   hipStream_t stream, int fan, const int* first) {
  IDX_CHECK(S <= Smax, "prefill longer than the cache");
  IDX_CHECK(slot_ids && len && fan >= 1 && (!first || fan == 1), "null pointer");
  if (n <= 0) return 0;
  static const int cat = prof_register("kv_store_slots_kernel");
  ProfScope prof(cat, stream, 0.0, (kv.fmt == 2 ? 26.0 : kv.fmt ? 28.0 : 16.0) * n * (double)S * d);
  if (kv.fmt == 2) return kv_store_fp8(qkv, kv, n, H, S, Smax, d, slot_ids, len, fan, stream, first);
  void* const kcache = kv.kcache;
  void* const vcache = kv.vcache;
  const int kv16 = kv.fmt;
  if (fan > 1 || first) {
    if (kv16) hipLaunchKernelGGL((kv_store_slots_kernel<true, true>), dim3(S, n), dim3(256), 0, stream, qkv, kcache, vcache, H, S, Smax, d, slot_ids, len, fan, first);
    else hipLaunchKernelGGL((kv_store_slots_kernel<false, true>), dim3(S, n), dim3(256), 0, stream, qkv, kcache, vcache, H, S, Smax, d, slot_ids, len, fan, first);
  } else if (kv16) {
    hipLaunchKernelGGL((kv_store_slots_kernel<true, false>), dim3(S, n), dim3(256), 0, stream, qkv, kcache, vcache, H, S, Smax, d, slot_ids, len, 1, nullptr);
  } else {
    hipLaunchKernelGGL((kv_store_slots_kernel<false, false>), dim3(S, n), dim3(256), 0, stream, qkv, kcache, vcache, H, S, Smax, d, slot_ids, len, 1, nullptr);
  }
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---- the fp8 cache's instruments: its quantiser on plain vectors, and the check of the device's f32 -> fp8 conversion ----
__global__ __launch_bounds__(256) void kv_fp8_quantize_kernel(const float* x, int n, unsigned char* codes, float* scales) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), dd = threadIdx.x & 63;
  if (v >= n) return;      // (wave-uniform)
  unsigned code;
  float sc;
  kv_fp8_quantize_lane(x[(size_t)v * 64 + dd], code, sc);
  codes[(size_t)v * 64 + dd] = (unsigned char)code;
  if (dd == 0) scales[v] = sc;
}

int kv_fp8_quantize(const float* x, int n, unsigned char* codes, float* scales, hipStream_t stream) {
  IDX_CHECK(x && codes && scales && n >= 0, "null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(kv_fp8_quantize_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, x, n, codes, scales);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ void fp8_encode_table_kernel(const float* in, unsigned char* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (unsigned char)kv_fp8_encode(in[i]);
}

int fp8_check_device_encode(hipStream_t stream) {
  static bool ok = false;
  if (ok) return 0;
  std::vector<float> tab;      // every code value and every midpoint between neighbouring codes, both signs
  for (int c = 0; c <= 126; ++c) {
    const float v = fp8_e4m3_decode((unsigned char)c);
    tab.push_back(v);
    tab.push_back(-v);
    if (c < 126) {
      const float mid = 0.5f * (v + fp8_e4m3_decode((unsigned char)(c + 1)));      // exact: neighbours share all but 4 mantissa bits
      tab.push_back(mid);
      tab.push_back(-mid);
    }
  }
  const int n = (int)tab.size();
  float* din = nullptr;
  unsigned char* dout = nullptr;
  IDX_HIP(hipMalloc(&din, n * sizeof(float)));
  hipError_t e = hipMalloc(&dout, n);
  std::vector<unsigned char> got(n);
  if (e == hipSuccess) e = hipMemcpyAsync(din, tab.data(), n * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fp8_encode_table_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, din, dout, n);
    e = hipMemcpyAsync(got.data(), dout, n, hipMemcpyDeviceToHost, stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(din);
  (void)hipFree(dout);
  IDX_HIP(e);
  for (int i = 0; i < n; ++i)
    if (got[i] != fp8_e4m3_encode(tab[i])) IDX_FAIL("this device's f32 -> fp8 conversion is not OCP e4m3fn, nearest even (input " + std::to_string(tab[i]) + ")");
  ok = true;
  return 0;
}

// decode-session admission: the right-padded prefill input (the same values generate() builds for an unpadded row)
__global__ __launch_bounds__(256) void session_prefill_input_kernel(float* x, const float* emb, int ld_rows, const int* P, int S, int d,
                                                                    const float* mel_emb, const float* mel_pos, int start_token) {
  const int s = blockIdx.x, b = blockIdx.y, Pb = P[b];
  float* out = x + ((size_t)b * S + s) * d;
  for (int e = threadIdx.x; e < d; e += 256) {
    float v = 0.f;
    if (s < Pb) v = emb[((size_t)b * ld_rows + s) * d + e];
    else if (s == Pb) { v += mel_emb[(size_t)start_token * d + e]; v += mel_pos[e]; }      // gather_sum_rows' order (generate)
    out[e] = v;
  }
}

int session_prefill_input(float* x, const float* emb, int ld_rows, const int* P, int n, int S, int d, const float* mel_emb,
                          const float* mel_pos, int start_token, hipStream_t stream) {
  IDX_CHECK(x && emb && P && mel_emb && mel_pos, "null pointer");
  if (n <= 0) return 0;
  static const int cat = prof_register("session_prefill_input_kernel");
  ProfScope prof(cat, stream, 0.0, 8.0 * n * (double)S * d);
  hipLaunchKernelGGL(session_prefill_input_kernel, dim3(S, n), dim3(256), 0, stream, x, emb, ld_rows, P, S, d, mel_emb, mel_pos, start_token);
  IDX_LAUNCH_CHECK();
  return 0;
}

// decode-session admission: reset the admitted slots, stage the prefill's last valid row of each for the first-token head
__global__ __launch_bounds__(256) void session_reset_slots_kernel(SlotState* slots, unsigned char* seen, int V, int start_token, float* x_last,
                                                                  const float* x, int S, int d, const int* slot_ids, const int* P, const int* cap,
                                                                  const int* row) {
  const int t = blockIdx.x, slot = slot_ids[t], b = row ? row[t] : t, Pb = P[b];      // (takes: slot t holds a take of prefill row row[t])
  unsigned char* sr = seen + (size_t)slot * V;
  for (int v = threadIdx.x; v < V; v += 256) sr[v] = (v == 1 || v == start_token) ? 1 : 0;      // input_ids = [1 ... 1, start]
  const float* src = x + ((size_t)b * S + Pb) * d;
  for (int e = threadIdx.x; e < d; e += 256) x_last[(size_t)slot * d + e] = src[e];
  if (threadIdx.x == 0) slots[slot] = SlotState{Pb, 1, 0, cap[t], 1};
}

int session_reset_slots(SlotState* slots, unsigned char* seen, int V, int start_token, float* x_last, const float* x, int S, int d,
                        const int* slot_ids, const int* P, const int* cap, int n, hipStream_t stream, const int* row) {
  IDX_CHECK(slots && seen && x_last && x && slot_ids && P && cap, "null pointer");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(session_reset_slots_kernel, dim3(n), dim3(256), 0, stream, slots, seen, V, start_token, x_last, x, S, d, slot_ids, P, cap, row);
  IDX_LAUNCH_CHECK();
  return 0;
}

// Continuing from given codes: the prefill input rows behind the start token.  Workgroup (j, b) writes position P_b + 1 + j of prefill
// row b, x = mel_emb[prefix_b[j]] + mel_pos[pos0 + j] -- the sum write_next_input forms for a decode step's input.  Every other row of
// the input is written by the kernels of before (the generation's copies and gather, session_prefill_input_kernel), which run first.
__global__ __launch_bounds__(256) void prefix_input_rows_kernel(const PrefixRows p) {
  const int j = blockIdx.x, b = blockIdx.y;
  const int Pb = p.P ? p.P[b] : p.P_all, kb = p.klen ? p.klen[b] : p.k_all;
  if (j >= kb) return;      // (workgroup-uniform)
  const size_t base = p.off ? (size_t)p.off[b] : (size_t)(b / p.row_div) * p.k_all;
  const int tok = min(max((int)p.prefix[base + j], 0), p.V - 1);      // (inside the table whatever the caller holds: the host has checked)
  float* out = p.x + ((size_t)b * p.S + Pb + 1 + j) * p.d;
  const float* te = p.mel_emb + (size_t)tok * p.d;
  const float* pe = p.mel_pos + (size_t)(p.pos0 + j) * p.d;
  for (int e = threadIdx.x; e < p.d; e += 256) out[e] = te[e] + pe[e];
}

int prefix_input_rows(const PrefixRows& a, int rows, int kmax, hipStream_t stream) {
  IDX_CHECK(a.x && a.prefix && a.mel_emb && a.mel_pos, "null pointer");
  IDX_CHECK(a.S >= 1 && a.d >= 1 && a.V >= 1 && a.row_div >= 1 && (a.pos0 == 1 || a.pos0 == 2), "prefix rows: shape");
  IDX_CHECK(a.P || (a.P_all >= 1 && a.P_all + 1 + a.k_all <= a.S), "prefix rows: the prefix does not fit the prefill row");
  IDX_CHECK(a.klen || kmax == a.k_all, "prefix rows: one length for every row, or a length per row");
  if (rows <= 0 || kmax <= 0) return 0;
  IDX_CHECK(rows <= 65535, "prefix rows: too many rows");
  static const int cat = prof_register("prefix_input_rows_kernel");
  ProfScope prof(cat, stream, 0.0, 12.0 * rows * (double)kmax * a.d);
  hipLaunchKernelGGL(prefix_input_rows_kernel, dim3(kmax, rows), dim3(256), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// session_reset_slots for an admission with prefixes: entry t's slot starts behind its prefill row's k = klen[b] given codes -- seen =
// {1, start} and the codes, codes[slot][0, k) = the codes, logprobs[slot][0, k) = the caller's values or 0 (scored sessions), x_last from
// position P + k, state {P + k, k + 1, k, cap, 1}: what session_fork_kernel leaves a take cut at k, in front of its next token
__global__ __launch_bounds__(256) void session_reset_slots_prefix_kernel(const PrefixReset p) {
  const int t = blockIdx.x, slot = p.slot_ids[t], b = p.row ? p.row[t] : t, Pb = p.P[b], kb = p.klen[b];
  const size_t base = (size_t)p.off[b];
  unsigned char* sr = p.seen + (size_t)slot * p.V;
  for (int v = threadIdx.x; v < p.V; v += 256) sr[v] = (v == 1 || v == p.start_token) ? 1 : 0;      // input_ids = [1 ... 1, start | prefix]
  __syncthreads();
  for (int i = threadIdx.x; i < kb; i += 256) {
    const long long c = p.prefix[base + i];
    p.codes[(size_t)slot * p.codes_ld + i] = c;
    sr[min(max((int)c, 0), p.V - 1)] = 1;
    if (p.logprobs) p.logprobs[(size_t)slot * p.codes_ld + i] = p.prefix_lp ? p.prefix_lp[base + i] : 0.0f;
  }
  const float* src = p.x + ((size_t)b * p.S + Pb + kb) * p.d;
  for (int e = threadIdx.x; e < p.d; e += 256) p.x_last[(size_t)slot * p.d + e] = src[e];
  if (threadIdx.x == 0) p.slots[slot] = SlotState{Pb + kb, kb + 1, kb, p.cap[t], 1};
}

int session_reset_slots_prefix(const PrefixReset& a, int n, hipStream_t stream) {
  IDX_CHECK(a.slots && a.seen && a.x_last && a.x && a.slot_ids && a.P && a.cap && a.klen && a.off && a.prefix && a.codes, "null pointer");
  IDX_CHECK(a.V >= 2 && a.S >= 1 && a.d >= 1 && a.codes_ld >= 1, "prefix reset: shape");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(session_reset_slots_prefix_kernel, dim3(n), dim3(256), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ends the slots of `mask` (bit i = slot i) from outside the step: live = 0, step left as it is (the codes produced so far), as the
// sampler leaves a slot that ended by itself.  cap_at_step (stop): a slot that was live also gets max_step = step, the cap it would
// have ended at by itself; one that had ended keeps its state.
__global__ __launch_bounds__(64) void session_end_slots_kernel(SlotState* slots, int n_slots, unsigned long long mask, int cap_at_step) {
  const int i = threadIdx.x;
  if (i >= n_slots || !((mask >> i) & 1ull)) return;
  if (cap_at_step && slots[i].live) slots[i].max_step = slots[i].step;
  slots[i].live = 0;
}

int session_end_slots(SlotState* slots, int n_slots, unsigned long long mask, bool cap_at_step, hipStream_t stream) {
  IDX_CHECK(slots, "null pointer");
  IDX_CHECK(n_slots >= 1 && n_slots <= 64, "1 <= slots <= 64");
  if (!mask) return 0;
  hipLaunchKernelGGL(session_end_slots_kernel, dim3(1), dim3(64), 0, stream, slots, n_slots, mask, cap_at_step ? 1 : 0);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---- preempt and resume (decode.h ParkArgs, idxtts.h "Preempt and resume") ----
// n bytes (a multiple of 4) from src to dst, both 16-byte aligned, by the PARK_NT threads of a workgroup: 16-byte vectors, consecutive
// lanes on consecutive vectors, four in flight per thread; the last n % 16 bytes go dword by dword.  PAD: dst is a segment of the
// parked row, whose last vector is written whole with zeros behind the data; else exactly n bytes are written (a cache run: what lies
// behind position pos belongs to later steps).
constexpr int PARK_NT = 256;
template <bool PAD>
__device__ __forceinline__ void park_copy_run(char* dst, const char* src, const size_t n, const int tid) {
  const size_t nv = n >> 4;
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  size_t i = tid;
  for (; i + 3 * PARK_NT < nv; i += 4 * PARK_NT) {
    const uint4 a = s4[i], b = s4[i + PARK_NT], c = s4[i + 2 * PARK_NT], e = s4[i + 3 * PARK_NT];
    d4[i] = a; d4[i + PARK_NT] = b; d4[i + 2 * PARK_NT] = c; d4[i + 3 * PARK_NT] = e;
  }
  for (; i < nv; i += PARK_NT) d4[i] = s4[i];
  const int tail = (int)(n & 15) >> 2;      // dwords behind the last whole vector
  if (tail && tid == 0) {
    const unsigned* sw = reinterpret_cast<const unsigned*>(src) + nv * 4;
    unsigned* dw = reinterpret_cast<unsigned*>(dst) + nv * 4;
    if (PAD) {
      d4[nv] = make_uint4(sw[0], tail > 1 ? sw[1] : 0u, tail > 2 ? sw[2] : 0u, 0u);
    } else {
      dw[0] = sw[0];
      if (tail > 1) dw[1] = sw[1];
      if (tail > 2) dw[2] = sw[2];
    }
  }
}

// Grid (runs + 1, heads, layers), runs = 2 * chunks (+ 2: fp8 scales).  Workgroup (r, h, l): r < chunks: key chunk r of (l, h), one
// straight run of pos granules; r < 2 * chunks: piece r - chunks of the value run (pos * 64 elements, cut into `chunks` pieces at
// vector boundaries so that every workgroup moves about as much as a key run); then the two scale runs.  Workgroup (runs, 0, 0) moves
// the small state -- header, seen row, codes, step scalars, sampler -- and on resume writes the slot's next input.
template <bool RESUME>
__global__ __launch_bounds__(PARK_NT) void session_park_kernel(const ParkArgs p) {
  const int tid = threadIdx.x, r = blockIdx.x, h = blockIdx.y, l = blockIdx.z, H = gridDim.y;
  const idxtts_park_header& hd = p.hdr;
  const ParkLayout lay = park_layout(hd.kv_format, hd.layers, hd.heads, hd.number_mel_codes, hd.pos, hd.step, hd.reserved[1]);
  const int C = lay.chunks, runs = 2 * C + (hd.kv_format == 2 ? 2 : 0);
  auto move = [&](char* cache, char* seg, size_t n) {      // one run between the cache and its segment of the parked row
    if (RESUME) park_copy_run<false>(cache, seg, n, tid);
    else park_copy_run<true>(seg, cache, n, tid);
  };
  if (r < runs) {
    char* const seg = p.blob + lay.off_kv + ((size_t)l * H + h) * lay.per_head;
    const size_t sh = (size_t)p.slot * H + h;
    if (r < C) {
      move(p.kcache + l * p.layer_bytes + (sh * C + r) * p.Smax * lay.gran, seg + r * lay.krun, (size_t)hd.pos * lay.gran);
    } else if (r < 2 * C) {
      const size_t nv = lay.vrun >> 4, v0 = nv * (r - C) / C, v1 = nv * (r - C + 1) / C;
      move(p.vcache + l * p.layer_bytes + sh * p.Smax * 64 * lay.elem + (v0 << 4), seg + C * lay.krun + (v0 << 4), (v1 - v0) << 4);
    } else {
      float* const sc = (r == 2 * C ? p.kscale : p.vscale) + l * p.layer_scales + sh * p.Smax;
      move(reinterpret_cast<char*>(sc), seg + C * lay.krun + lay.vrun + (r - 2 * C) * lay.srun, (size_t)hd.pos * 4);
    }
    return;
  }
  if (h || l) return;
  const int V = hd.number_mel_codes, step = hd.step;
  unsigned char* const seen = p.seen + (size_t)p.slot * V;      // (a row of seen is only byte aligned)
  long long* const codes = p.codes + (size_t)p.slot * p.codes_ld;
  unsigned* const bseen = reinterpret_cast<unsigned*>(p.blob + lay.off_seen);
  long long* const bcodes = reinterpret_cast<long long*>(p.blob + lay.off_codes);
  const int nd = (int)(park_pad16((size_t)V) >> 2), nc = (int)(park_pad16((size_t)step * 8) >> 3);
  SlotState* const ss = p.slots + p.slot;
  if (!RESUME) {
    for (int i = tid; i < nd; i += PARK_NT) {
      unsigned w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * i + j < V) w |= (unsigned)seen[4 * i + j] << (8 * j);
      bseen[i] = w;
    }
    for (int i = tid; i < nc; i += PARK_NT) bcodes[i] = i < step ? codes[i] : 0ll;
    if (hd.reserved[1]) {      // scored row: the log-probabilities of its codes, zeros to the end of the last vector
      const float* const lp = p.logprobs + (size_t)p.slot * p.codes_ld;
      float* const blp = reinterpret_cast<float*>(p.blob + lay.off_lp);
      const int nl = (int)(park_pad16((size_t)step * 4) >> 2);
      for (int i = tid; i < nl; i += PARK_NT) blp[i] = i < step ? lp[i] : 0.0f;
    }
    if (tid == 0) {
      *reinterpret_cast<idxtts_park_header*>(p.blob) = hd;
      ss->live = 0;      // the slot is free, as session_end_slots leaves an evicted one
    }
  } else {
    for (int i = tid; i < nd; i += PARK_NT) {
      const unsigned w = bseen[i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * i + j < V) seen[4 * i + j] = (unsigned char)(w >> (8 * j));
    }
    for (int i = tid; i < step; i += PARK_NT) codes[i] = bcodes[i];
    if (hd.reserved[1]) {
      float* const lp = p.logprobs + (size_t)p.slot * p.codes_ld;
      const float* const blp = reinterpret_cast<const float*>(p.blob + lay.off_lp);
      for (int i = tid; i < step; i += PARK_NT) lp[i] = blp[i];
    }
    // the row's last code, kept inside the embedding table whatever the bytes say (the header is checked on the host, the body is not)
    const int tok = min(max((int)bcodes[step - 1], 0), V - 1);
    write_next_input<PARK_NT>(p.embed, p.B, p.slot, tok, hd.mel_pos, tid);
    if (tid == 0) {
      p.cur_tok[p.slot] = tok;
      if (p.samp) p.samp[p.slot] = SlotSampling{hd.mode, hd.temperature, hd.top_k, hd.top_p, hd.seed, reinterpret_cast<const float*>(hd.exp_noise)};
      *ss = SlotState{hd.pos, hd.mel_pos, hd.step, hd.max_step, 1};
    }
  }
}

static int park_launch(const ParkArgs& a, bool resume, hipStream_t stream) {
  const idxtts_park_header& hd = a.hdr;
  IDX_CHECK(a.blob && a.kcache && a.vcache && a.slots && a.seen && a.codes && a.cur_tok, "null pointer");
  IDX_CHECK(hd.kv_format >= 0 && hd.kv_format <= 2 && (hd.kv_format != 2 || (a.kscale && a.vscale)), "KV format");
  IDX_CHECK(hd.layers >= 1 && hd.layers <= 65535 && hd.heads >= 1 && hd.heads <= 65535, "shape");
  IDX_CHECK(a.slot >= 0 && a.slot < a.B && hd.step >= 1 && hd.step <= a.codes_ld && hd.pos >= 1 && hd.pos <= a.Smax, "slot state out of range");
  IDX_CHECK(a.Smax % 4 == 0 && a.layer_bytes % 16 == 0 && a.layer_scales % 4 == 0, "cache runs must start 16-byte aligned");
  IDX_CHECK(((uintptr_t)a.blob | (uintptr_t)a.kcache | (uintptr_t)a.vcache | (uintptr_t)a.kscale | (uintptr_t)a.vscale) % 16 == 0,
            "the parked row and the caches must be 16-byte aligned");
  IDX_CHECK(!resume || ((a.embed.x_row && a.embed.x_stats) || a.embed.x_frag), "resume needs the step's input buffers");
  IDX_CHECK((hd.reserved[1] == 0 && !a.logprobs) || (hd.reserved[1] == 1 && a.logprobs), "a scored row needs a scored session, and the reverse");
  const ParkLayout lay = park_layout(hd.kv_format, hd.layers, hd.heads, hd.number_mel_codes, hd.pos, hd.step, hd.reserved[1]);
  const int runs = 2 * lay.chunks + (hd.kv_format == 2 ? 2 : 0);
  static const int cat_p = prof_register("session_park_kernel"), cat_r = prof_register("session_resume_kernel");
  ProfScope prof(resume ? cat_r : cat_p, stream, 0.0, 2.0 * (double)lay.bytes);
  const dim3 grid(runs + 1, hd.heads, hd.layers);
  if (resume) hipLaunchKernelGGL(session_park_kernel<true>, grid, dim3(PARK_NT), 0, stream, a);
  else hipLaunchKernelGGL(session_park_kernel<false>, grid, dim3(PARK_NT), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

int session_park_slot(const ParkArgs& a, hipStream_t stream) { return park_launch(a, false, stream); }
int session_resume_slot(const ParkArgs& a, hipStream_t stream) { return park_launch(a, true, stream); }

// ---- fork (decode.h ForkArgs, idxtts.h "Several takes of one request") ----
// n bytes (a multiple of 4) of the source slot's run to the same run of every destination slot: run0 is the run in slot 0, a slot's run
// lies slot * stride bytes behind it, and every run starts 16-byte aligned.  park_copy_run's access pattern -- 16-byte vectors,
// consecutive lanes on consecutive vectors, four loads in flight per thread -- with each vector loaded once and stored p.n times; the
// n % 16 bytes behind the last whole vector (fp8 scale runs and odd fp8 key runs end off a vector) go as dwords, one lane each.
__device__ __forceinline__ void fork_copy_run(char* const run0, const size_t stride, const ForkArgs& p, const size_t n, const int tid) {
  const uint4* const s4 = reinterpret_cast<const uint4*>(run0 + p.src * stride);
  const size_t nv = n >> 4;
  size_t i = tid;
  for (; i + 3 * PARK_NT < nv; i += 4 * PARK_NT) {
    const uint4 a = s4[i], b = s4[i + PARK_NT], c = s4[i + 2 * PARK_NT], e = s4[i + 3 * PARK_NT];
    for (int j = 0; j < p.n; ++j) {
      uint4* const d4 = reinterpret_cast<uint4*>(run0 + p.dst[j] * stride);
      d4[i] = a; d4[i + PARK_NT] = b; d4[i + 2 * PARK_NT] = c; d4[i + 3 * PARK_NT] = e;
    }
  }
  for (; i < nv; i += PARK_NT) {
    const uint4 a = s4[i];
    for (int j = 0; j < p.n; ++j) reinterpret_cast<uint4*>(run0 + p.dst[j] * stride)[i] = a;
  }
  const int tail = (int)(n & 15) >> 2;      // dwords behind the last whole vector: exactly n bytes are written
  if (tid < tail) {
    const unsigned w = reinterpret_cast<const unsigned*>(s4)[nv * 4 + tid];
    for (int j = 0; j < p.n; ++j) reinterpret_cast<unsigned*>(run0 + p.dst[j] * stride)[nv * 4 + tid] = w;
  }
}

// The grid of session_park_kernel: (runs + 1, heads, layers), workgroup (r, h, l) on run r of (l, h) -- a key chunk, a piece of the value
// run, a scale run -- and workgroup (runs, 0, 0) on the small state of every destination.
__global__ __launch_bounds__(PARK_NT) void session_fork_kernel(const ForkArgs p) {
  const int tid = threadIdx.x, r = blockIdx.x, h = blockIdx.y, l = blockIdx.z, H = gridDim.y;
  const int pos = p.P + (p.at > 1 ? p.at : 1);      // cached positions of a row that holds `at` codes (the prefill alone: P + 1)
  const ParkLayout lay = park_layout(p.kv_fmt, p.layers, H, p.V, pos, p.at);
  const int C = lay.chunks, runs = 2 * C + (p.kv_fmt == 2 ? 2 : 0);
  if (r < runs) {
    if (r < C) {
      const size_t run = (size_t)p.Smax * lay.gran;
      fork_copy_run(p.kcache + l * p.layer_bytes + ((size_t)h * C + r) * run, (size_t)H * C * run, p, (size_t)pos * lay.gran, tid);
    } else if (r < 2 * C) {
      const size_t run = (size_t)p.Smax * 64 * lay.elem, nv = lay.vrun >> 4, v0 = nv * (r - C) / C, v1 = nv * (r - C + 1) / C;
      fork_copy_run(p.vcache + l * p.layer_bytes + h * run + (v0 << 4), H * run, p, (v1 - v0) << 4, tid);
    } else {
      float* const sc = (r == 2 * C ? p.kscale : p.vscale) + l * p.layer_scales + (size_t)h * p.Smax;
      fork_copy_run(reinterpret_cast<char*>(sc), (size_t)H * p.Smax * 4, p, (size_t)pos * 4, tid);
    }
    return;
  }
  if (h || l) return;
  const int V = p.V, at = p.at;
  const long long* const scodes = p.codes + (size_t)p.src * p.codes_ld;
  for (int j = 0; j < p.n; ++j) {      // input_ids = [1 ... 1, start] and nothing else yet
    unsigned char* const sr = p.seen + (size_t)p.dst[j] * V;
    for (int v = tid; v < V; v += PARK_NT) sr[v] = (v == 1 || v == p.start_token) ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < at; i += PARK_NT) {
    const long long c = scodes[i];
    const int tok = min(max((int)c, 0), V - 1);      // (inside the row whatever the source holds)
    for (int j = 0; j < p.n; ++j) {
      p.codes[(size_t)p.dst[j] * p.codes_ld + i] = c;
      p.seen[(size_t)p.dst[j] * V + tok] = 1;
    }
    if (p.logprobs) {      // scored session: lp[0, at) of the source
      const float lp = p.logprobs[(size_t)p.src * p.codes_ld + i];
      for (int j = 0; j < p.n; ++j) p.logprobs[(size_t)p.dst[j] * p.codes_ld + i] = lp;
    }
  }
  for (int j = 0; j < p.n; ++j)      // the prefill's last row travels with every take: a take can be forked at 0 like its source
    for (int e = tid; e < p.embed.d; e += PARK_NT) p.x_last[(size_t)p.dst[j] * p.embed.d + e] = p.x_last[(size_t)p.src * p.embed.d + e];
  if (at == 0) {      // the admission's state before the first token: the head reads x_last
    if (tid < p.n) p.slots[p.dst[tid]] = SlotState{p.P, 1, 0, p.cap[tid], 1};
    return;
  }
  const int tok = min(max((int)scodes[at - 1], 0), V - 1);
  for (int j = 0; j < p.n; ++j) write_next_input<PARK_NT>(p.embed, p.B, p.dst[j], tok, at + 1, tid);
  if (tid < p.n) {
    p.cur_tok[p.dst[tid]] = tok;
    p.slots[p.dst[tid]] = SlotState{p.P + at, at + 1, at, p.cap[tid], 1};
  }
}

int session_fork_slots(const ForkArgs& a, hipStream_t stream) {
  IDX_CHECK(a.kcache && a.vcache && a.slots && a.seen && a.codes && a.cur_tok && a.x_last, "null pointer");
  IDX_CHECK(a.kv_fmt >= 0 && a.kv_fmt <= 2 && (a.kv_fmt != 2 || (a.kscale && a.vscale)), "KV format");
  IDX_CHECK(a.layers >= 1 && a.layers <= 65535 && a.heads >= 1 && a.heads <= 65535 && a.V >= 2, "shape");
  IDX_CHECK(a.B >= 1 && a.B <= FORK_MAX && a.n >= 1 && a.n < a.B && a.n <= PARK_NT && a.src >= 0 && a.src < a.B, "slots out of range");
  for (int j = 0; j < a.n; ++j) IDX_CHECK(a.dst[j] < a.B && a.dst[j] != a.src, "destination slot out of range");
  IDX_CHECK(a.P >= 1 && a.at >= 0 && a.at <= a.codes_ld && a.P + std::max(a.at, 1) <= a.Smax, "slot state out of range");
  IDX_CHECK(a.Smax % 4 == 0 && a.layer_bytes % 16 == 0 && a.layer_scales % 4 == 0, "cache runs must start 16-byte aligned");
  IDX_CHECK(((uintptr_t)a.kcache | (uintptr_t)a.vcache | (uintptr_t)a.kscale | (uintptr_t)a.vscale) % 16 == 0, "the caches must be 16-byte aligned");
  IDX_CHECK((a.embed.x_row && a.embed.x_stats) || a.embed.x_frag, "fork needs the step's input buffers");
  const ParkLayout lay = park_layout(a.kv_fmt, a.layers, a.heads, a.V, a.P + std::max(a.at, 1), a.at);
  const int runs = 2 * lay.chunks + (a.kv_fmt == 2 ? 2 : 0);
  static const int cat = prof_register("session_fork_kernel");
  ProfScope prof(cat, stream, 0.0, (1.0 + a.n) * (double)lay.bytes);
  hipLaunchKernelGGL(session_fork_kernel, dim3(runs + 1, a.heads, a.layers), dim3(PARK_NT), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---- preempt and resume of a beam group (beam.h ParkGroupArgs, idxtts.h "Preempt and resume, beam sessions") ----
// n bytes (a multiple of sizeof(U)) in units of U, for a run whose cache side starts in the middle of a cache row and is only
// sizeof(U)-aligned: consecutive lanes on consecutive units.  PAD as in park_copy_run: dst is a 16-byte aligned segment of the parked
// group and is written up to pad16(n) with zeros behind the data; else exactly n bytes are written.
template <class U, bool PAD>
__device__ __forceinline__ void park_copy_units(char* dst, const char* src, const size_t n, const int tid) {
  const size_t nu = n / sizeof(U), nt = PAD ? park_pad16(n) / sizeof(U) : nu;
  const U* s = reinterpret_cast<const U*>(src);
  U* d = reinterpret_cast<U*>(dst);
  for (size_t i = tid; i < nt; i += PARK_NT) d[i] = i < nu ? s[i] : U{};
}

// Grid (runs + 1, heads, layers), runs as in session_park_kernel: workgroup (r, h, l) moves run r -- a key chunk, a piece of the value
// run or a scale run, split as the row kernel splits them -- of every part of (l, h) in turn: part 0 is the shared run, positions
// [0, Ps), read from the group's first slot and on resume written to all nb rows, and part 1 + j the positions [Ps, pos) of beam j.
// So every workgroup of one kind moves the same Ps + nb * T positions' worth, and there are no more workgroups than a row's launch
// has (one per part would be nb + 1 times as many of a few KB each, and the launch would be bound by the workgroup dispatch rate,
// not by bytes: measured, profiles/README.md "Preemption").  The per-beam runs start at position Ps inside a cache row: values and
// 16-byte key granules stay 16-byte aligned, fp8 key granules are 8-byte aligned when Ps is odd and scales 4-byte aligned unless
// Ps % 4 == 0, so the copy is chosen from the cache address.  Workgroup (runs, 0, 0) moves the small state and on resume writes the
// rows' next inputs.
template <bool RESUME>
__global__ __launch_bounds__(PARK_NT) void session_park_group_kernel(const ParkGroupArgs p) {
  const int tid = threadIdx.x, r = blockIdx.x, h = blockIdx.y, H = gridDim.y;
  const idxtts_park_group_header& hd = p.hdr;
  const int nb = hd.num_beams, l = blockIdx.z, slot0 = p.group * nb;
  const ParkGroupLayout lay = park_group_layout(hd.kv_format, hd.layers, hd.heads, hd.number_mel_codes, nb, hd.pos, hd.step);
  const int C = lay.sh.chunks, runs = 2 * C + (hd.kv_format == 2 ? 2 : 0);
  auto move = [&](char* cache, char* seg, size_t n) {      // one run between the cache and its segment of the parked group
    const unsigned mis = (unsigned)((uintptr_t)cache & 15);
    if (mis == 0) {
      if (RESUME) park_copy_run<false>(cache, seg, n, tid);
      else park_copy_run<true>(seg, cache, n, tid);
    } else if ((mis & 7) == 0 && (n & 7) == 0) {
      if (RESUME) park_copy_units<uint2, false>(cache, seg, n, tid);
      else park_copy_units<uint2, true>(seg, cache, n, tid);
    } else {
      if (RESUME) park_copy_units<unsigned, false>(cache, seg, n, tid);
      else park_copy_units<unsigned, true>(seg, cache, n, tid);
    }
  };
  if (r < runs) {
    for (int part = 0; part <= nb; ++part) {
      const ParkLayout& pl = part ? lay.pb : lay.sh;
      const int first = part ? lay.Ps : 0, npos = part ? lay.T : lay.Ps;
      if (npos <= 0) continue;
      char* const seg = p.blob + lay.off_kv + ((size_t)l * H + h) * lay.per_head + (part ? lay.sh.per_head + (size_t)(part - 1) * lay.pb.per_head : 0);
      const int j0 = part ? part - 1 : 0, j1 = part ? part : (RESUME ? nb : 1);      // the cache rows this segment belongs to
      for (int j = j0; j < j1; ++j) {
        const size_t sh = (size_t)(slot0 + j) * H + h;
        if (r < C) {
          move(p.kcache + l * p.layer_bytes + ((sh * C + r) * p.Smax + first) * pl.gran, seg + r * pl.krun, (size_t)npos * pl.gran);
        } else if (r < 2 * C) {
          const size_t nv = pl.vrun >> 4, v0 = nv * (r - C) / C, v1 = nv * (r - C + 1) / C;
          move(p.vcache + l * p.layer_bytes + (sh * p.Smax + first) * 64 * pl.elem + (v0 << 4), seg + C * pl.krun + (v0 << 4), (v1 - v0) << 4);
        } else {
          float* const sc = (r == 2 * C ? p.kscale : p.vscale) + l * p.layer_scales + sh * p.Smax + first;
          move(reinterpret_cast<char*>(sc), seg + C * pl.krun + pl.vrun + (r - 2 * C) * pl.srun, (size_t)npos * 4);
        }
      }
    }
    return;
  }
  if (h || l) return;
  const BeamState& b = p.bs;
  const int V = hd.number_mel_codes, step = hd.step, g = p.group, ld = b.seq_ld, hn = hd.hyp_n;
  const size_t o = (size_t)g * (BEAM_MAX + 1);
  const int nd = (int)(lay.seen_row >> 2), nt = (int)(lay.tok_row >> 2);
  const int nsc = (int)(park_pad16((size_t)nb * 4) >> 2), nhs = (int)(park_pad16((size_t)nb * 8) >> 3);
  float* const bscore = reinterpret_cast<float*>(p.blob + lay.off_scores);
  double* const bworst = reinterpret_cast<double*>(p.blob + lay.off_worst);
  double* const bhscore = reinterpret_cast<double*>(p.blob + lay.off_hscore);
  int* const bhlen = reinterpret_cast<int*>(p.blob + lay.off_hlen);
  for (int j = 0; j < nb; ++j) {
    unsigned char* const seen = b.seen + (size_t)(slot0 + j) * V;      // (a row of seen is only byte aligned)
    int* const seq = b.seq + (size_t)(slot0 + j) * ld;
    unsigned* const bseen = reinterpret_cast<unsigned*>(p.blob + lay.off_seen + j * lay.seen_row);
    int* const bseq = reinterpret_cast<int*>(p.blob + lay.off_seq + j * lay.tok_row);
    if (!RESUME) {
      for (int i = tid; i < nd; i += PARK_NT) {
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * i + k < V) w |= (unsigned)seen[4 * i + k] << (8 * k);
        bseen[i] = w;
      }
      for (int i = tid; i < nt; i += PARK_NT) bseq[i] = i < step ? seq[i] : 0;
    } else {
      for (int i = tid; i < nd; i += PARK_NT) {
        const unsigned w = bseen[i];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * i + k < V) seen[4 * i + k] = (unsigned char)(w >> (8 * k));
      }
      for (int i = tid; i < step; i += PARK_NT) seq[i] = bseq[i];
      // the beam's last token, kept inside the embedding table whatever the bytes say (the header is checked on the host, the body is not)
      const int tok = min(max(bseq[step - 1], 0), V - 1);
      write_next_input<PARK_NT>(p.embed, p.B, slot0 + j, tok, hd.mel_pos, tid);
      if (tid == 0) {
        b.cur_tok[slot0 + j] = tok;
        b.slots[slot0 + j] = SlotState{hd.pos, hd.mel_pos, hd.step, hd.max_step, 1};
      }
    }
  }
  // the scorer's list in its own order: hypothesis q of the parked group is row q, whatever physical row of hyp_seq held it
  for (int q = 0; q < nb; ++q) {
    int* const bh = reinterpret_cast<int*>(p.blob + lay.off_hseq + q * lay.tok_row);
    if (!RESUME) {
      const int len = q < hn ? min(max(b.hyp_len[o + q], 0), step) : 0;
      const int* const src = b.hyp_seq + (o + (q < hn ? min(max(b.hyp_slot[o + q], 0), BEAM_MAX) : 0)) * ld;
      for (int i = tid; i < nt; i += PARK_NT) bh[i] = i < len ? src[i] : 0;
    } else if (q < hn) {
      int* const dst = b.hyp_seq + (o + q) * ld;
      for (int i = tid; i < step; i += PARK_NT) dst[i] = bh[i];
    }
  }
  if (!RESUME) {
    for (int i = tid; i < nsc; i += PARK_NT) bscore[i] = i < nb ? b.beam_scores[slot0 + i] : 0.f;
    for (int i = tid; i < nhs; i += PARK_NT) bhscore[i] = i < hn ? b.hyp_score[o + i] : 0.0;
    for (int i = tid; i < nsc; i += PARK_NT) bhlen[i] = i < hn ? min(max(b.hyp_len[o + i], 0), step) : 0;
    if (tid == 0) {
      bworst[0] = b.hyp_worst[g]; bworst[1] = 0.0;
      *reinterpret_cast<idxtts_park_group_header*>(p.blob) = hd;
    }
    if (tid < nb) b.slots[slot0 + tid].live = 0;      // the group is free, as session_end_slots leaves an evicted one
  } else {
    if (tid < nb) {
      b.beam_scores[slot0 + tid] = bscore[tid];
      b.hyp_score[o + tid] = bhscore[tid];
      b.hyp_len[o + tid] = min(max(bhlen[tid], 0), step);
      b.hyp_slot[o + tid] = tid;
    }
    if (tid == 0) {
      b.hyp_n[g] = hn; b.hyp_worst[g] = bworst[0]; b.done[g] = hd.done;
      p.group_tab[g] = SlotBeam{hd.do_sample, hd.temperature, hd.top_k, hd.top_p, hd.length_penalty, hd.early_stopping, hd.seed,
                                reinterpret_cast<const float*>(hd.exp_noise)};
    }
  }
}

static int park_group_launch(const ParkGroupArgs& a, bool resume, hipStream_t stream) {
  const idxtts_park_group_header& hd = a.hdr;
  const BeamState& b = a.bs;
  IDX_CHECK(a.blob && a.kcache && a.vcache && a.group_tab && b.slots && b.seen && b.seq && b.cur_tok && b.beam_scores && b.hyp_score &&
            b.hyp_len && b.hyp_slot && b.hyp_seq && b.hyp_n && b.hyp_worst && b.done, "null pointer");
  IDX_CHECK(hd.kv_format >= 0 && hd.kv_format <= 2 && (hd.kv_format != 2 || (a.kscale && a.vscale)), "KV format");
  IDX_CHECK(hd.num_beams >= 2 && hd.num_beams <= BEAM_MAX && hd.num_beams == b.nb, "num_beams");
  IDX_CHECK(hd.layers >= 1 && hd.layers <= 65535 && hd.heads >= 1 && hd.heads <= 65535, "shape");
  IDX_CHECK(a.group >= 0 && (a.group + 1) * hd.num_beams <= a.B && hd.step >= 1 && hd.step <= b.seq_ld && hd.pos >= hd.step &&
            hd.pos <= a.Smax && hd.hyp_n >= 0 && hd.hyp_n <= hd.num_beams, "group state out of range");
  IDX_CHECK(a.Smax % 4 == 0 && a.layer_bytes % 16 == 0 && a.layer_scales % 4 == 0, "cache rows must start 16-byte aligned");
  IDX_CHECK(((uintptr_t)a.blob | (uintptr_t)a.kcache | (uintptr_t)a.vcache | (uintptr_t)a.kscale | (uintptr_t)a.vscale) % 16 == 0,
            "the parked group and the caches must be 16-byte aligned");
  IDX_CHECK(!resume || ((a.embed.x_row && a.embed.x_stats) || a.embed.x_frag), "resume needs the step's input buffers");
  const ParkGroupLayout lay = park_group_layout(hd.kv_format, hd.layers, hd.heads, hd.number_mel_codes, hd.num_beams, hd.pos, hd.step);
  const int runs = 2 * lay.sh.chunks + (hd.kv_format == 2 ? 2 : 0);
  static const int cat_p = prof_register("session_park_group_kernel"), cat_r = prof_register("session_resume_group_kernel");
  ProfScope prof(resume ? cat_r : cat_p, stream, 0.0, 2.0 * (double)lay.bytes);
  const dim3 grid(runs + 1, hd.heads, hd.layers);
  if (resume) hipLaunchKernelGGL(session_park_group_kernel<true>, grid, dim3(PARK_NT), 0, stream, a);
  else hipLaunchKernelGGL(session_park_group_kernel<false>, grid, dim3(PARK_NT), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

int session_park_group(const ParkGroupArgs& a, hipStream_t stream) { return park_group_launch(a, false, stream); }
int session_resume_group(const ParkGroupArgs& a, hipStream_t stream) { return park_group_launch(a, true, stream); }

// out[r][:] = sum over the tables t with idx[t][r] >= 0 of table[t][idx[t][r]][:]
__global__ __launch_bounds__(256) void gather_sum_rows_kernel(const GatherArgs p) {
  const int r = blockIdx.x;
  int id[GATHER_MAX_TABLES];
#pragma unroll
  for (int t = 0; t < GATHER_MAX_TABLES; ++t) {
    id[t] = (p.table[t] && p.idx[t]) ? p.idx[t][r] : -1;
    if (p.table_rows[t] > 0 && id[t] >= p.table_rows[t]) {      // nn.Embedding would raise IndexError: never read past the table
      if (p.oob && threadIdx.x == 0) *p.oob = 1 + t;
      id[t] = -1;
    }
  }
  for (int e = threadIdx.x; e < p.d; e += 256) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < GATHER_MAX_TABLES; ++t)
      if (id[t] >= 0) v += p.table[t][(size_t)id[t] * p.d + e];
    p.out[(size_t)r * p.ld_out + e] = v;
  }
}

int gather_sum_rows(const GatherArgs& a, int rows, hipStream_t stream) {
  if (rows == 0) return 0;
  IDX_CHECK(a.out && a.d > 0, "gather args");
  static const int cat = prof_register("gather_sum_rows_kernel");
  ProfScope prof(cat, stream, 0.0, 8.0 * rows * (double)a.d);
  hipLaunchKernelGGL(gather_sum_rows_kernel, dim3(rows), dim3(256), 0, stream, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// decode-step embedding: x[b] = mel_emb[cur_tok[b]] + mel_pos[st->mel_pos], written as A-fragment images (common.h)
__global__ __launch_bounds__(256) void embed_step_kernel(float* x, int d, const float* mel_emb, const float* mel_pos,
                                                         const int* cur_tok, const DecodeState* st) {
  const int b = blockIdx.x;
  const int tok = cur_tok[b], mp = st->mel_pos;
  for (int e = threadIdx.x; e < d; e += 256) x[frag_index(b, e, d >> 4)] = mel_emb[(size_t)tok * d + e] + mel_pos[(size_t)mp * d + e];
}

__global__ __launch_bounds__(256) void embed_step_pl_kernel(float* x_row, float* x_stats, int B, int d, const float* mel_emb,
                                                            const float* mel_pos, const int* cur_tok, const DecodeState* st) {
  embed_row_pl<256>(x_row, x_stats, blockIdx.x, B, d, mel_emb, mel_pos, cur_tok[blockIdx.x], st->mel_pos, threadIdx.x);
}

int embed_step_pl(float* x_row, float* x_stats, int B, int d, const float* mel_emb, const float* mel_pos, const int* cur_tok,
                  const DecodeState* st, hipStream_t stream) {
  IDX_CHECK(d % 16 == 0, "row statistics per 16 columns need d % 16 == 0");
  static const int cat = prof_register("embed_step_kernel");
  ProfScope prof(cat, stream, 0.0, 12.0 * B * (double)d);
  hipLaunchKernelGGL(embed_step_pl_kernel, dim3(B), dim3(256), 0, stream, x_row, x_stats, B, d, mel_emb, mel_pos, cur_tok, st);
  IDX_LAUNCH_CHECK();
  return 0;
}

int embed_step(float* x, int B, int d, const float* mel_emb, const float* mel_pos, const int* cur_tok, const DecodeState* st,
               hipStream_t stream) {
  static const int cat = prof_register("embed_step_kernel");
  ProfScope prof(cat, stream, 0.0, 12.0 * B * (double)d);
  hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(256), 0, stream, x, d, mel_emb, mel_pos, cur_tok, st);
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
