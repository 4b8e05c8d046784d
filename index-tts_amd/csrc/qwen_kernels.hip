// Qwen3 causal LM (qwen.h): every kernel of the decode step and the prefill helpers, with their launchers.  A step is five launches per layer --
//   qkv GEMV (input RMSNorm in its prologue) | q/k RMSNorm + rotary + KV append + grouped-query attention (keys split over
//   workgroups, merged by the last to arrive) | o_proj GEMV + residual | gate/up GEMV (post-attention RMSNorm in its prologue,
//   silu(g) * u in its epilogue) | down_proj GEMV + residual
// -- and a tail of final norm + head GEMV with a two-stage argmax, the optional logits hand-over, and the next token's embedding row.
// Each launch exists twice: for one row (geometry in the arguments, x in registers over the GEMV's unit loop) and for a tile of
// R <= QWEN_BATCH_ROWS rows (a GEMV wave loads each weight fragment once and forms one dot product per row from it, the attention
// grid gets a row axis, the tail and the logits hand-over run one workgroup (column) per row).  Both inline the same bodies, each a
// fixed sequence of operations: that is what makes a row of a tile equal its own single call bit for bit -- ids, stop step, every
// logit, either storage format, eager or replayed.  No row's arithmetic depends on another row: the same staging and RMSNorm of the
// activation vector, the same k -> lane map and FMA chain (chunk-major, then the 8 elements) and the same shuffle butterfly per dot
// product (so no MFMA here), the attention body with the row's OWN geometry (Smax_b, nsplit_b, slice) from a per-row device table,
// the same tail.  Rows that have finished ride along in the GEMVs (the weights are read anyway); they skip the attention, and
// nothing they compute is recorded.
//
// The RMSNorm gain is applied to the activation vector in the GEMV's prologue ((x * rsqrt(mean x^2 + eps)) * g, the reference's order of
// operations), not folded into the weights: W diag(g) would leave the bf16 grid, and bf16 storage here holds the checkpoint's weights
// exactly.  Each workgroup redoes the norm of the <= 3072-element vector it multiplies with (L2-resident, a few hundred FMAs a thread).
//
// The GEMVs are plain weight streams: a wave owns whole rows, a lane the same 8 consecutive k of every 512-k chunk (two 16-byte loads
// of fp32, one of bf16), all loads of a row pair issued before the first FMA, no branch among them (addresses past K are clamped and
// meet zeros of x), then a shuffle butterfly.  The k -> lane map and the order of the FMAs do not depend on the storage format or on how the step is
// launched: bf16 and fp32 storage of the same values, and eager launches and graph replay, agree bit for bit.
//
// Row tile, QWEN_BATCH_ROWS = 8.  The R activation vectors are staged in LDS (R x chunks x 2 KiB, dynamic, sized by the rows in
// flight), the weight rows of a unit stay in registers, and each row's 8 k per chunk come back from LDS by two conflict-free
// ds_read_b128 (qwen_x_slot).  What 8 rows cost in occupancy, by K:
//   K <= 1024 (qkv, gate / up, head of the 0.6 B model): 32 KiB a workgroup, 5 workgroups = 5 waves a SIMD on the 160 KiB of a CU;
//   K  = 2048 (o_proj): 64 KiB, 2 workgroups a CU;  K = 3072 (down_proj): 96 KiB, 1 workgroup a CU, one wave a SIMD.
// The two large-K matrices have 1024 rows, i.e. 256 workgroups of four one-row waves -- one workgroup a CU whatever LDS allows --
// so the LDS limit takes nothing from them at this shape; registers (two weight rows of 6 chunks in fp32: 96 VGPRs, plus one row's
// 48 x values) leave 2 waves a SIMD on the 6-chunk template and more below.  16 rows would need 192 KiB at K = 3072: over a CU's LDS.
// A tile of one row has nothing to share and runs the one-row kernels.
#include "qwen.h"

#include <cmath>
#include <type_traits>

#include "device_util.h"

namespace idxtts {

constexpr int HD = QWEN_HD, GMAX = QWEN_GMAX;

// ---- the bodies, one definition each.  They stay in namespace idxtts, not in the unnamed one with the kernels: the compiler lays a
// kernel's LDS variables out by their symbol names, and the kernels' instructions were compared with these names in place. ----

// The GEMV's activation vector into LDS (NCH * 512 slots, zeros past K), RMS-normed when a gain is given: (x * rsqrt(mean x^2 + eps)) * g.
// A workgroup of 256 threads; every thread calls.  red: 4 floats of LDS.
// SWZ: slot of k = its 512-chunk | (k / 4 & 1) * 256 | (k / 8 & 63) * 4 | (k & 3) -- a lane's two 16-byte halves of a chunk sit 16 bytes
// from the next lane's, so a wave's ds_read_b128 meets no bank twice (the plain order, 32 bytes a lane, meets each twice).
template <bool SWZ>
__device__ __forceinline__ int qwen_x_slot(const int k) {
  return SWZ ? ((k & ~511) | (((k >> 2) & 1) << 8) | (((k >> 3) & 63) << 2) | (k & 3)) : k;
}
template <int NCH, bool SWZ>
__device__ __forceinline__ void qwen_stage_x(float* xs, const float* x, const float* g, const float eps, const int K, float* red) {
  const int tid = threadIdx.x;
  float ss = 0.0f;
  for (int k = tid; k < NCH * 512; k += 256) {
    const float v = k < K ? x[k] : 0.0f;
    xs[qwen_x_slot<SWZ>(k)] = v;
    ss = fmaf(v, v, ss);
  }
  if (g) {
    const float tot = block_sum<4>(ss, red);
    const float rs = 1.0f / sqrtf(tot / (float)K + eps);
    for (int k = tid; k < K; k += 256) xs[qwen_x_slot<SWZ>(k)] = (xs[qwen_x_slot<SWZ>(k)] * rs) * g[k];
  }
}
// a lane's 8 consecutive k of every chunk, from the staged vector
template <int NCH, bool SWZ>
__device__ __forceinline__ void qwen_lane_x(const float* xs, const int lane, float (&xr)[NCH][8]) {
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    if (SWZ) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(xs + j * 512 + 4 * lane), hi = *reinterpret_cast<const f32x4*>(xs + j * 512 + 256 + 4 * lane);
#pragma unroll
      for (int e = 0; e < 4; ++e) { xr[j][e] = lo[e]; xr[j][4 + e] = hi[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) xr[j][e] = xs[j * 512 + 8 * lane + e];
    }
  }
}

template <int NCH, typename WT> struct RowRaw;
template <int NCH> struct RowRaw<NCH, float> {
  f32x4 v[NCH][2];
  __device__ __forceinline__ void load(const float* row, const int (&koff)[NCH]) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      v[j][0] = *reinterpret_cast<const f32x4*>(row + koff[j]);
      v[j][1] = *reinterpret_cast<const f32x4*>(row + koff[j] + 4);
    }
  }
  __device__ __forceinline__ float get(int j, int e) const { return v[j][e >> 2][e & 3]; }
};
template <int NCH> struct RowRaw<NCH, unsigned short> {
  u32x4 v[NCH];
  __device__ __forceinline__ void load(const unsigned short* row, const int (&koff)[NCH]) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) v[j] = *reinterpret_cast<const u32x4*>(row + koff[j]);
  }
  __device__ __forceinline__ float get(int j, int e) const {
    const unsigned w = v[j][e >> 1];
    return __builtin_bit_cast(float, (e & 1) ? (w & 0xffff0000u) : (w << 16));
  }
};
template <int NCH, typename WT>
__device__ __forceinline__ float row_dot(const RowRaw<NCH, WT>& r, const float (&xr)[NCH][8]) {
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < NCH; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(r.get(j, e), xr[j][e], acc);
  return wave_sum(acc);
}

// The GEMV workgroup (256 threads), single-prompt (RT = 1, R = 1) and batched (RT = QWEN_BATCH_ROWS, R <= RT rows run) alike: a wave
// owns whole units -- rows (EPI_RES), row pairs, (gate, up) pairs --, loads each weight fragment once and forms one dot product
// per row of x from it.  xs: LDS for [R][NCH * 512] floats.  p.x: [R][K]; p.y: [R][ldy]; p.st: [R]; p.part_val / part_idx: [R][part_stride].
// RT = 1 keeps the row's x in registers over the unit loop; RT > 1 takes each row's back from LDS (swizzled slots, qwen_x_slot) per unit.
template <int NCH, int EPI, typename WT, int RT>
__device__ __forceinline__ void qwen_gemv_body(const QwenGemvArgs& p, float* xs, const int R, const int ldy, const int part_stride) {
  constexpr bool SWZ = RT > 1;
  __shared__ float red[4];
  __shared__ float s_val[RT][4];
  __shared__ int s_idx[RT][4];
  __shared__ int s_last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = p.K;
  // ---- prologue: the activation vectors, RMS-normed when a gain is given ----
#pragma unroll 1
  for (int r = 0; r < R; ++r) qwen_stage_x<NCH, SWZ>(xs + r * NCH * 512, p.x + (size_t)r * K, p.g, p.eps, K, red);
  __syncthreads();
  float xr[NCH][8];
  if (RT == 1) qwen_lane_x<NCH, SWZ>(xs, lane, xr);
  int koff[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) koff[j] = min(j * 512 + 8 * lane, K - 8);      // past K: a valid address whose weights meet zeros of x
  const WT* wa = static_cast<const WT*>(p.wa);
  const WT* wb = static_cast<const WT*>(p.wb);
  float best[RT];
  int best_i[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) { best[r] = -INFINITY; best_i[r] = 0x7fffffff; }
  const int u0 = (blockIdx.x * 4 + wave) * p.upw;
  for (int i = 0; i < p.upw; ++i) {
    const int u = u0 + i;
    if (u >= p.units) break;      // the whole wave
    if (EPI == EPI_RES) {
      RowRaw<NCH, WT> a;
      a.load(wa + (size_t)u * K, koff);
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < R) {
          if (RT > 1) qwen_lane_x<NCH, SWZ>(xs + r * NCH * 512, lane, xr);
          const float s = row_dot(a, xr);
          if (lane == 0) p.y[(size_t)r * ldy + u] += s;
        }
    } else {
      RowRaw<NCH, WT> a, b;
      if (EPI == EPI_SWIGLU) {
        a.load(wa + (size_t)u * K, koff);
        b.load(wb + (size_t)u * K, koff);
      } else {
        a.load(wa + (size_t)(2 * u) * K, koff);
        b.load(wa + (size_t)(2 * u + 1) * K, koff);
      }
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < R) {
          if (RT > 1) qwen_lane_x<NCH, SWZ>(xs + r * NCH * 512, lane, xr);
          const float s0 = row_dot(a, xr), s1 = row_dot(b, xr);
          float* y = p.y + (size_t)r * ldy;
          if (EPI == EPI_SWIGLU) {
            if (lane == 0) y[u] = (s0 / (1.0f + expf(-s0))) * s1;
          } else {
            if (lane == 0) { y[2 * u] = s0; y[2 * u + 1] = s1; }
            if (EPI == EPI_HEAD) {      // rows ascend within a wave: a strict > keeps the lowest index among equals
              if (s0 > best[r]) { best[r] = s0; best_i[r] = 2 * u; }
              if (s1 > best[r]) { best[r] = s1; best_i[r] = 2 * u + 1; }
            }
          }
        }
    }
  }
  if (EPI != EPI_HEAD) return;
  // ---- per-row argmax, stage 1: this workgroup's best of each row; stage 2: the last workgroup to arrive reduces every workgroup's ----
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r) { s_val[r][wave] = best[r]; s_idx[r][wave] = best_i[r]; }
  }
  __syncthreads();
  if (wave == 0) {
    if (lane < R) {      // lane r leaves row r's
      float bv = s_val[lane][0]; int bi = s_idx[lane][0];
      argmax_take_waves<4>(bv, bi, s_val[lane], s_idx[lane]);
      __hip_atomic_store(&p.part_val[(size_t)lane * part_stride + blockIdx.x], bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&p.part_idx[(size_t)lane * part_stride + blockIdx.x], bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // wg_arrive_last (device_util.h) by wave 0 alone, the only one that stored: one barrier behind it, none in front
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      const unsigned old = __hip_atomic_fetch_add(p.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = old == gridDim.x - 1u;
      if (s_last) __hip_atomic_store(p.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  if (!s_last) return;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {      // block_argmax opens with a barrier: the rows may share its LDS
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int b = tid; b < (int)gridDim.x; b += 256) {
      const float v = __hip_atomic_load(&p.part_val[(size_t)r * part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int ix = __hip_atomic_load(&p.part_idx[(size_t)r * part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      argmax_take(bv, bi, v, ix);
    }
    block_argmax<4>(bv, bi, s_val[0], s_idx[0], tid);
    if (tid == 0) p.st[r].argmax = bi;
  }
}

// RMSNorm over the head + rotary of one 128-vector by one wave: the lane holds elements lane and lane + 64, a rotary pair
// (rotate_half: out[i] = x[i] cos - x[i + 64] sin, out[i + 64] = x[i + 64] cos + x[i] sin, products rounded before the sum as the
// reference's element-wise ops are)
__device__ __forceinline__ void head_norm_rope(const float* v, const float* g, float eps, const float* rope_pos, int lane, float* o0, float* o1) {
  const float a = v[lane], b = v[lane + 64];
  const float ss = wave_sum(fmaf(a, a, b * b));
  const float rs = 1.0f / sqrtf(ss / (float)QWEN_HD + eps);
  const float na = (a * rs) * g[lane], nb = (b * rs) * g[lane + 64];
  const float c = rope_pos[2 * lane], s = rope_pos[2 * lane + 1];
  *o0 = __fadd_rn(__fmul_rn(na, c), __fmul_rn(-nb, s));
  *o1 = __fadd_rn(__fmul_rn(nb, c), __fmul_rn(na, s));
}

// the body of a workgroup; pos: the query's position (the cache holds pos keys before it), r: its row of qkv / out
template <bool APPEND>
__device__ __forceinline__ void qwen_attn_body(const QwenAttnArgs& p, const int kvh, const int z, const int r, const int pos) {
  constexpr int HD = QWEN_HD, GMAX = QWEN_GMAX;
  extern __shared__ float sc[];      // [G][slice_cap]
  __shared__ __attribute__((aligned(16))) float qs[GMAX][HD];
  __shared__ __attribute__((aligned(16))) float kn[HD];
  __shared__ float vn[HD];
  __shared__ float acc2[GMAX][HD];
  __shared__ float red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int G = p.G;
  const float* row = p.qkv + (size_t)r * p.ld_qkv;
  const float* rope_pos = p.rope + (size_t)pos * HD;
  const int qdim = p.Hq * HD, kvdim = p.Hkv * HD;
  for (int item = wave; item < G + (APPEND ? 2 : 0); item += 4) {
    if (item < G) {
      float o0, o1;
      head_norm_rope(row + (kvh * G + item) * HD, p.qn_g, p.eps, rope_pos, lane, &o0, &o1);
      qs[item][lane] = o0; qs[item][lane + 64] = o1;
    } else if (item == G) {
      float o0, o1;
      head_norm_rope(row + qdim + kvh * HD, p.kn_g, p.eps, rope_pos, lane, &o0, &o1);
      kn[lane] = o0; kn[lane + 64] = o1;
      if (z == 0) {
        float* kd = p.kc + ((size_t)kvh * p.Smax + pos) * HD;
        kd[lane] = o0; kd[lane + 64] = o1;
      }
    } else {
      const float* vs = row + qdim + kvdim + kvh * HD;
      const float a = vs[lane], b = vs[lane + 64];
      vn[lane] = a; vn[lane + 64] = b;
      if (z == 0) {
        float* vd = p.vc + ((size_t)kvh * p.Smax + pos) * HD;
        vd[lane] = a; vd[lane + 64] = b;
      }
    }
  }
  __syncthreads();
  const int n_keys = pos + 1;
  const int slice = (n_keys + p.nsplit - 1) / p.nsplit;
  const int j0 = z * slice, j1 = min(n_keys, j0 + slice);
  const int cap = p.slice_cap;
  float mx[GMAX], l[GMAX], o[GMAX];
#pragma unroll
  for (int g = 0; g < GMAX; ++g) { mx[g] = -INFINITY; l[g] = 0.0f; o[g] = 0.0f; }
  if (j0 < j1) {
    // ---- pass 1: scores, threads = keys ----
    for (int j = j0 + tid; j < j1; j += 256) {
      float s[GMAX];
#pragma unroll
      for (int g = 0; g < GMAX; ++g) s[g] = 0.0f;
      if (APPEND && j == pos) {
        for (int e = 0; e < HD; e += 4) {
          const f32x4 kv = *reinterpret_cast<const f32x4*>(kn + e);
#pragma unroll
          for (int g = 0; g < GMAX; ++g)
            if (g < G) {
              const f32x4 qq = *reinterpret_cast<const f32x4*>(&qs[g][e]);
              s[g] = fmaf(qq[0], kv[0], s[g]); s[g] = fmaf(qq[1], kv[1], s[g]); s[g] = fmaf(qq[2], kv[2], s[g]); s[g] = fmaf(qq[3], kv[3], s[g]);
            }
        }
      } else {
        const f32x4* kr = reinterpret_cast<const f32x4*>(p.kc + ((size_t)kvh * p.Smax + j) * HD);
        for (int e = 0; e < HD / 4; ++e) {
          const f32x4 kv = kr[e];
#pragma unroll
          for (int g = 0; g < GMAX; ++g)
            if (g < G) {
              const f32x4 qq = *reinterpret_cast<const f32x4*>(&qs[g][4 * e]);
              s[g] = fmaf(qq[0], kv[0], s[g]); s[g] = fmaf(qq[1], kv[1], s[g]); s[g] = fmaf(qq[2], kv[2], s[g]); s[g] = fmaf(qq[3], kv[3], s[g]);
            }
        }
      }
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) {
          const float v = s[g] * p.scale;
          sc[g * cap + (j - j0)] = v;
          mx[g] = fmaxf(mx[g], v);
        }
    }
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
      if (g < G) mx[g] = block_max<4>(mx[g], red);
    for (int j = j0 + tid; j < j1; j += 256) {
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) {
          const float e = expf(sc[g * cap + (j - j0)] - mx[g]);
          sc[g * cap + (j - j0)] = e;
          l[g] += e;
        }
    }
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
      if (g < G) l[g] = block_sum<4>(l[g], red);      // (its barriers also publish the probabilities)
    // ---- pass 2: probabilities x values, threads = (feature, key parity) ----
    const int d = tid & 127, half = tid >> 7;
    for (int j = j0 + half; j < j1; j += 2) {
      const float v = (APPEND && j == pos) ? vn[d] : p.vc[((size_t)kvh * p.Smax + j) * HD + d];
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) o[g] = fmaf(sc[g * cap + (j - j0)], v, o[g]);
    }
    if (half == 1) {
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) acc2[g][d] = o[g];
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) o[g] += acc2[g][d];
    }
  }
  float* out = p.out + (size_t)r * p.ld_out;
  if (p.nsplit == 1) {
    if (tid < 128)
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) out[(kvh * G + g) * HD + tid] = o[g] / l[g];
    return;
  }
  // ---- key split: leave (o, max, sum) of this piece; the last piece of the kv head to arrive merges them in piece order ----
  const int NS = p.nsplit;
  if (tid < 128) {
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
      if (g < G) {
        float* mine = p.part + ((size_t)(kvh * G + g) * NS + z) * 130;
        __hip_atomic_store(&mine[tid], o[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) {
          __hip_atomic_store(&mine[128], mx[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&mine[129], l[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
  }
  if (!wg_arrive_last(&p.cnt[kvh], (unsigned)NS) || tid >= 128) return;
  for (int g = 0; g < G; ++g) {
    const float* all = p.part + (size_t)(kvh * G + g) * NS * 130;
    float M = -INFINITY;
    for (int i = 0; i < NS; ++i) M = fmaxf(M, __hip_atomic_load(&all[i * 130 + 128], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    float L = 0.0f, O = 0.0f;
    for (int i = 0; i < NS; ++i) {
      const float mi = __hip_atomic_load(&all[i * 130 + 128], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float li = __hip_atomic_load(&all[i * 130 + 129], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float oi = __hip_atomic_load(&all[i * 130 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float w = li > 0.0f ? expf(mi - M) : 0.0f;      // an empty piece (more pieces than keys) carries nothing
      L = fmaf(li, w, L);
      O = fmaf(oi, w, O);
    }
    out[(kvh * G + g) * HD + tid] = O / L;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The step's last launch (one workgroup per row): record the head's choice, pick what continues the sequence (the forced id, or the
// choice), stop on an end id or at the cap, write the next input's embedding row and advance the step scalars.
template <typename WT>
__device__ __forceinline__ void qwen_tail_row(const QwenTailArgs& p) {
  const QwenState s = *p.st;
  const bool live = !s.done && s.step < p.max_new;
  int next = s.argmax;
  if (live && p.forced) next = p.forced[s.step];
  next = min(max(next, 0), p.V - 1);
  bool stop = false;
  for (int i = 0; i < p.n_eos; ++i) stop |= next == p.eos[i];
  const WT* er = static_cast<const WT*>(p.emb) + (size_t)next * p.H;
  for (int k = threadIdx.x; k < p.H; k += 256) p.xd[k] = load_w(er + k);
  __syncthreads();      // every thread has read the step scalars
  if (threadIdx.x == 0 && live) {
    p.out_ids[s.step] = s.argmax;
    p.st->n_out = s.step + 1;
    p.st->step = s.step + 1;
    if (stop || s.step + 1 >= p.max_new) p.st->done = 1;
    else p.st->pos = s.pos + 1;
  }
}

// out_logits[step][c] = logits[cols[c]] (cols null: column c) of a live step
__device__ __forceinline__ void qwen_logits_row(const QwenState* st, const float* logits, const int* cols, int n_cols, int max_new, float* out, const int c) {
  const QwenState s = *st;
  if (s.done || s.step >= max_new) return;
  if (c < n_cols) out[(size_t)s.step * n_cols + c] = logits[cols ? cols[c] : c];
}

// ---------------------------------------------------------------------------------------------------------------------------
// The kernels: each body above at one row, and at the row tile
namespace {

template <int NCH, int EPI, typename WT>
__global__ __launch_bounds__(256) void qwen_gemv_kernel(const QwenGemvArgs p) {
  __shared__ float xs[NCH * 512];
  qwen_gemv_body<NCH, EPI, WT, 1>(p, xs, 1, 0, 0);
}

// the full row tile: R <= QWEN_BATCH_ROWS rows run
template <int NCH, int EPI, typename WT>
__global__ __launch_bounds__(256) void qwen_gemv_batch_kernel(const QwenGemvArgs p) {
  extern __shared__ __attribute__((aligned(16))) float xs[];      // [R][NCH * 512], slots by qwen_x_slot
  qwen_gemv_body<NCH, EPI, WT, QWEN_BATCH_ROWS>(p, xs, p.R, p.ldy, p.part_stride);
}

template <bool APPEND>
__global__ __launch_bounds__(256) void qwen_attn_kernel(const QwenAttnArgs p) {
  const int r = blockIdx.z;
  qwen_attn_body<APPEND>(p, blockIdx.x, blockIdx.y, r, p.st ? p.st->pos : p.pos0 + r);
}

// grid (kv head, key piece, row): the row's geometry -- what its own single call would use -- from the table
__global__ __launch_bounds__(256) void qwen_attn_batch_kernel(const QwenAttnArgs q) {
  const int z = blockIdx.y, b = blockIdx.z;
  const QwenBatchRow row = q.rows[b];
  const QwenState* st = q.st + b;
  if (z >= row.nsplit || st->done) return;      // the whole workgroup
  QwenAttnArgs a = q;
  const size_t off = (size_t)q.layer * a.Hkv * row.Smax * HD;
  a.kc = row.kc + off; a.vc = row.vc + off; a.Smax = row.Smax;
  a.nsplit = row.nsplit; a.slice_cap = (row.Smax + row.nsplit - 1) / row.nsplit;
  a.part += (size_t)b * q.part_stride; a.cnt += b * a.Hkv; a.st = st;
  qwen_attn_body<true>(a, blockIdx.x, z, b, st->pos);
}

template <typename WT>
__global__ __launch_bounds__(256) void qwen_tail_kernel(const QwenTailArgs p) { qwen_tail_row<WT>(p); }

template <typename WT>
__global__ __launch_bounds__(256) void qwen_tail_batch_kernel(const QwenTailArgs q) {
  const int b = blockIdx.x;
  const QwenBatchRow row = q.rows[b];
  QwenTailArgs t = q;
  t.st += b; t.xd += (size_t)b * t.H; t.out_ids = row.out_ids; t.forced = q.use_forced ? row.forced : nullptr; t.max_new = row.max_new;
  qwen_tail_row<WT>(t);
}

__global__ __launch_bounds__(256) void qwen_logits_kernel(const QwenState* st, const float* logits, const int* cols, int n_cols, int max_new, float* out) {
  qwen_logits_row(st, logits, cols, n_cols, max_new, out, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void qwen_logits_batch_kernel(const QwenState* st, const float* logits, int V, const int* cols, int n_cols,
                                                                const QwenBatchRow* rows) {
  const int b = blockIdx.y;
  const QwenBatchRow row = rows[b];
  qwen_logits_row(st + b, logits + (size_t)b * V, cols, n_cols, row.max_new, row.out_logits, blockIdx.x * 256 + threadIdx.x);
}

// ---- prefill helpers (once per call, not tuned) ----
template <typename WT>
__global__ __launch_bounds__(256) void qwen_embed_rows_kernel(float* x, const int* ids, const void* emb, int H, int V) {
  const int id = min(max(ids[blockIdx.x], 0), V - 1);
  const WT* er = static_cast<const WT*>(emb) + (size_t)id * H;
  for (int k = threadIdx.x; k < H; k += 256) x[(size_t)blockIdx.x * H + k] = load_w(er + k);
}

__global__ __launch_bounds__(256) void qwen_rmsnorm_rows_kernel(const float* x, float* y, const float* g, int H, float eps) {
  __shared__ float red[4];
  const float* xr = x + (size_t)blockIdx.x * H;
  float ss = 0.0f;
  for (int k = threadIdx.x; k < H; k += 256) ss = fmaf(xr[k], xr[k], ss);
  const float rs = 1.0f / sqrtf(block_sum<4>(ss, red) / (float)H + eps);
  for (int k = threadIdx.x; k < H; k += 256) y[(size_t)blockIdx.x * H + k] = (xr[k] * rs) * g[k];
}

// keys (RMSNorm + rotary) and values of every prompt position into the cache: grid (P, Hkv), one wave
__global__ __launch_bounds__(64) void qwen_kv_store_kernel(const float* qkv, int ld_qkv, const float* kn_g, float eps, const float* rope, float* kc,
                                                           float* vc, int Smax, int qdim, int kvdim) {
  const int pos = blockIdx.x, kvh = blockIdx.y, lane = threadIdx.x;
  const float* row = qkv + (size_t)pos * ld_qkv;
  float o0, o1;
  head_norm_rope(row + qdim + kvh * HD, kn_g, eps, rope + (size_t)pos * HD, lane, &o0, &o1);
  float* kd = kc + ((size_t)kvh * Smax + pos) * HD;
  kd[lane] = o0; kd[lane + 64] = o1;
  const float* vs = row + qdim + kvdim + kvh * HD;
  float* vd = vc + ((size_t)kvh * Smax + pos) * HD;
  vd[lane] = vs[lane]; vd[lane + 64] = vs[lane + 64];
}

__global__ __launch_bounds__(256) void qwen_silu_mul_kernel(const float* gu, float* h, int I) {      // gu row: [gate I | up I]
  const float* r = gu + (size_t)blockIdx.x * 2 * I;
  for (int k = threadIdx.x; k < I; k += 256) {
    const float g = r[k];
    h[(size_t)blockIdx.x * I + k] = (g / (1.0f + expf(-g))) * r[I + k];
  }
}

// ---- launchers ----
template <int NCH, int EPI, typename WT>
int gemv_launch_one(const QwenGemvArgs& a, int blocks, hipStream_t st) {
  if (a.R == 1) {
    hipLaunchKernelGGL((qwen_gemv_kernel<NCH, EPI, WT>), dim3(blocks), dim3(256), 0, st, a);
  } else {
    const size_t lds = (size_t)a.R * NCH * 512 * sizeof(float);      // above 64 KiB: allowed by qwen_kernels_prepare
    hipLaunchKernelGGL((qwen_gemv_batch_kernel<NCH, EPI, WT>), dim3(blocks), dim3(256), lds, st, a);
  }
  IDX_LAUNCH_CHECK();
  return 0;
}

template <int EPI, typename WT>
int gemv_launch_fmt(const QwenGemvArgs& a, int blocks, hipStream_t st) {
  const int nch = cdiv(a.K, 512);
  if (nch <= 1) return gemv_launch_one<1, EPI, WT>(a, blocks, st);
  if (nch <= 2) return gemv_launch_one<2, EPI, WT>(a, blocks, st);
  if (nch <= 4) return gemv_launch_one<4, EPI, WT>(a, blocks, st);
  return gemv_launch_one<6, EPI, WT>(a, blocks, st);
}

template <int EPI>
int gemv_launch(const QwenGemvArgs& a, int fmt, int blocks, hipStream_t st) {
  return fmt == QWEN_W_BF16 ? gemv_launch_fmt<EPI, unsigned short>(a, blocks, st) : gemv_launch_fmt<EPI, float>(a, blocks, st);
}

// dynamic LDS above 64 KiB needs the function attribute: only the 6-chunk templates at the full tile ask for it (96 KiB)
template <int EPI, typename WT>
hipError_t gemv_batch_allow_lds() {
  static_assert(QWEN_BATCH_ROWS * 4 * 512 * sizeof(float) <= 64 * 1024, "the 4-chunk templates would need the attribute too");
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&qwen_gemv_batch_kernel<6, EPI, WT>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, QWEN_BATCH_ROWS * 6 * 512 * (int)sizeof(float));
}
template <typename WT>
hipError_t gemv_batch_allow_lds_fmt() {
  hipError_t e = gemv_batch_allow_lds<EPI_STORE, WT>();
  if (e == hipSuccess) e = gemv_batch_allow_lds<EPI_RES, WT>();
  if (e == hipSuccess) e = gemv_batch_allow_lds<EPI_SWIGLU, WT>();
  if (e == hipSuccess) e = gemv_batch_allow_lds<EPI_HEAD, WT>();
  return e;
}

}  // namespace

int qwen_kernels_prepare() {
  IDX_HIP(gemv_batch_allow_lds_fmt<float>());
  IDX_HIP(gemv_batch_allow_lds_fmt<unsigned short>());
  return 0;
}

int qwen_gemv_blocks(const QwenGemvArgs& a) { return cdiv(a.units, 4 * a.upw); }

int qwen_gemv(int epi, const QwenGemvArgs& a, int fmt, int w_rows, hipStream_t st) {
  IDX_CHECK(a.K >= 8 && a.K % 8 == 0 && a.K <= 3072, "GEMV K must be a multiple of 8, at most 3072");
  IDX_CHECK(a.units > 0 && a.upw > 0 && a.R >= 1 && a.R <= QWEN_BATCH_ROWS, "GEMV shape");
  static const int cat1 = prof_register("qwen_gemv_kernel"), catR = prof_register("qwen_gemv_batch_kernel");
  ProfScope prof(a.R == 1 ? cat1 : catR, st, 2.0 * a.R * w_rows * a.K, (double)w_rows * a.K * (fmt == QWEN_W_BF16 ? 2 : 4));
  const int blocks = qwen_gemv_blocks(a);
  switch (epi) {
    case EPI_STORE: return gemv_launch<EPI_STORE>(a, fmt, blocks, st);
    case EPI_RES: return gemv_launch<EPI_RES>(a, fmt, blocks, st);
    case EPI_SWIGLU: return gemv_launch<EPI_SWIGLU>(a, fmt, blocks, st);
    case EPI_HEAD: return gemv_launch<EPI_HEAD>(a, fmt, blocks, st);
  }
  IDX_FAIL("GEMV epilogue");
}

int qwen_attn(const QwenAttnArgs& a, int rows, bool append, double query_keys, double keys, hipStream_t st) {
  IDX_CHECK(a.G >= 1 && a.G <= GMAX && a.Hq == a.Hkv * a.G, "query heads per kv head: 1..4");
  IDX_CHECK(a.nsplit >= 1 && a.slice_cap >= 1 && (a.nsplit == 1 || (a.part && a.cnt && (rows == 1 || a.rows))) && (!a.rows || append), "key split");
  const size_t lds = (size_t)a.G * a.slice_cap * sizeof(float);
  IDX_CHECK(lds <= 40 * 1024, "context too long for the attention kernel's score buffer");
  static const int cat1 = prof_register("qwen_attn_kernel"), catR = prof_register("qwen_attn_batch_kernel");
  ProfScope prof(a.rows ? catR : cat1, st, 4.0 * a.Hq * query_keys * HD, 8.0 * a.Hkv * keys * HD);
  const dim3 grid(a.Hkv, a.nsplit, rows);
  if (a.rows) hipLaunchKernelGGL(qwen_attn_batch_kernel, grid, dim3(256), lds, st, a);
  else if (append) hipLaunchKernelGGL(qwen_attn_kernel<true>, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(qwen_attn_kernel<false>, grid, dim3(256), lds, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

int qwen_logits(const QwenState* st, const float* logits, int V, const int* cols, int n_cols, int R, int max_new, float* out, const QwenBatchRow* rows,
                hipStream_t s) {
  static const int cat1 = prof_register("qwen_logits_kernel"), catR = prof_register("qwen_logits_batch_kernel");
  ProfScope prof(rows ? catR : cat1, s, 0.0, 8.0 * R * n_cols);
  if (rows) hipLaunchKernelGGL(qwen_logits_batch_kernel, dim3(cdiv(n_cols, 256), R), dim3(256), 0, s, st, logits, V, cols, n_cols, rows);
  else hipLaunchKernelGGL(qwen_logits_kernel, dim3(cdiv(n_cols, 256)), dim3(256), 0, s, st, logits, cols, n_cols, max_new, out);
  IDX_LAUNCH_CHECK();
  return 0;
}

int qwen_tail(const QwenTailArgs& t, int R, int fmt, hipStream_t st) {
  static const int cat1 = prof_register("qwen_tail_kernel"), catR = prof_register("qwen_tail_batch_kernel");
  ProfScope prof(t.rows ? catR : cat1, st, 0.0, 8.0 * R * t.H);
  if (t.rows) {
    if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_tail_batch_kernel<unsigned short>, dim3(R), dim3(256), 0, st, t);
    else hipLaunchKernelGGL(qwen_tail_batch_kernel<float>, dim3(R), dim3(256), 0, st, t);
  } else {
    if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_tail_kernel<unsigned short>, dim3(1), dim3(256), 0, st, t);
    else hipLaunchKernelGGL(qwen_tail_kernel<float>, dim3(1), dim3(256), 0, st, t);
  }
  IDX_LAUNCH_CHECK();
  return 0;
}

int qwen_embed_rows(float* x, const int* ids, const void* emb, int P, int H, int V, int fmt, hipStream_t st) {
  if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_embed_rows_kernel<unsigned short>, dim3(P), dim3(256), 0, st, x, ids, emb, H, V);
  else hipLaunchKernelGGL(qwen_embed_rows_kernel<float>, dim3(P), dim3(256), 0, st, x, ids, emb, H, V);
  IDX_LAUNCH_CHECK();
  return 0;
}

static int prefill_cat() {
  static const int cat = prof_register("qwen_prefill_rows");
  return cat;
}

int qwen_rmsnorm_rows(const float* x, float* y, const float* g, int P, int H, float eps, hipStream_t st) {
  ProfScope prof(prefill_cat(), st, 0.0, 8.0 * P * H);
  hipLaunchKernelGGL(qwen_rmsnorm_rows_kernel, dim3(P), dim3(256), 0, st, x, y, g, H, eps);
  IDX_LAUNCH_CHECK();
  return 0;
}

int qwen_kv_store(const QwenAttnArgs& a, int P, hipStream_t st) {
  ProfScope prof(prefill_cat(), st, 0.0, 16.0 * P * a.Hkv * HD);
  hipLaunchKernelGGL(qwen_kv_store_kernel, dim3(P, a.Hkv), dim3(64), 0, st, a.qkv, a.ld_qkv, a.kn_g, a.eps, a.rope, a.kc, a.vc, a.Smax, a.Hq * HD, a.Hkv * HD);
  IDX_LAUNCH_CHECK();
  return 0;
}

int qwen_silu_mul(const float* gu, float* h, int P, int I, hipStream_t st) {
  ProfScope prof(prefill_cat(), st, 0.0, 12.0 * P * I);
  hipLaunchKernelGGL(qwen_silu_mul_kernel, dim3(P), dim3(256), 0, st, gu, h, I);
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
