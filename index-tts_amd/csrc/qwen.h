// Qwen3 causal LM, greedy generation for one prompt (qwen.hip) or a batch of prompts that share each weight pass (qwen_batch.hip): the
// emotion-from-text classifier of the reference (QwenEmotion, infer_v2.py:948-1063).
// RMSNorm, per-head q/k RMSNorm, rotary positions, grouped-query attention at head_dim 128, SwiGLU MLP, (tied) vocabulary head.
// fp32 arithmetic; linear weights stored fp32 or bf16 (exact for a bf16 checkpoint).  Kernels and host code: qwen.hip, qwen_batch.hip;
// the device code both files inline (one definition each) is at the end of this header.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/idxtts.h"
#include "ctx.h"
#include "device_util.h"
#include "gemm.h"
#include "prof.h"

namespace idxtts {

enum QwenWeightFormat { QWEN_W_F32 = 0, QWEN_W_BF16 = 1 };

constexpr int QWEN_HD = 128;          // head_dim (the one instantiation)
constexpr int QWEN_GMAX = 4;          // q heads per kv head, at most
constexpr int QWEN_HEAD_UPW = 8;      // row pairs per wave of the head GEMV (64 rows per workgroup)
constexpr int QWEN_BATCH_ROWS = 8;    // prompts that share one weight pass of a batched step (qwen_batch.hip: what the choice costs)

// key pieces of a decode step over a cache of Smax rows
inline int qwen_nsplit_for(int Smax) { return std::min(16, std::max(1, cdiv(Smax, 64))); }

// step scalars of the generation in flight, device-resident: a captured decode step replays on them
struct QwenState {
  int pos;        // position of the token whose embedding is in xd (= keys in the cache before its step)
  int step;       // generated tokens so far
  int done;       // an end id has been fed (or the cap reached): later launches change nothing
  int argmax;     // the head's choice of the step in flight
  int n_out;      // valid entries of out_ids
  int pad[3];
};

struct QwenStream {      // a weight matrix [N][K] row-major in the decode format
  const void* w = nullptr;
  int N = 0, K = 0;
};

struct QwenLayer {
  const float *in_g = nullptr, *post_g = nullptr, *qn_g = nullptr, *kn_g = nullptr;
  LinearWeights qkv_l, o_l, gu_l, down_l;      // MFMA-packed fp32 (prefill)
  QwenStream qkv_s, o_s, gate_s, up_s, down_s; // decode streams
};

struct QwenBatchRow;      // the per-row device table of a batched step (qwen_batch.hip)

struct QwenModel : ModelBase {
  idxtts_qwen_config cfg;
  int fmt = QWEN_W_F32;
  std::vector<QwenLayer> layers;
  const float* norm_g = nullptr;
  QwenStream embed_s, head_s;      // head_s == embed_s when tied
  const float* rope = nullptr;     // [max_context][head_dim / 2][2] = (cos, sin)
  int qdim() const { return cfg.num_attention_heads * cfg.head_dim; }
  int kvdim() const { return cfg.num_key_value_heads * cfg.head_dim; }
  int qkvdim() const { return qdim() + 2 * kvdim(); }

  struct Buffers {
    float *x, *x2, *xn, *qkv, *att, *gu, *hmid;      // prefill activations, P rows
    float *kc, *vc; int Smax;                        // [L][Hkv][Smax][128] each
    float *xd, *qkvd, *attd, *hd, *logits;           // decode vectors
    float* head_val; int* head_idx; unsigned* head_cnt; int head_blocks;
    float* attn_part; unsigned* attn_cnt; int nsplit;
    QwenState* st;
    int *prompt, *eos, *forced, *cols, *out_ids;
    size_t bytes;
  };
  // one kept decode-step graph: nothing call-specific but these is baked into its launches
  struct GraphKey {
    void* ws = nullptr; size_t ws_bytes = 0; int P = 0, max_new = 0, n_eos = 0, n_cols = 0; bool forced = false, all_cols = false;
    float* out_logits = nullptr;
    bool operator==(const GraphKey& o) const {
      return ws == o.ws && ws_bytes == o.ws_bytes && P == o.P && max_new == o.max_new && n_eos == o.n_eos && n_cols == o.n_cols &&
             forced == o.forced && all_cols == o.all_cols && out_logits == o.out_logits;
    }
  };
  GraphKey graph_key;
  hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
  int graph_kernel_nodes = -1;
  hipStream_t own_stream = nullptr;

  // ---- batched generation (qwen_batch.hip): a tile of R <= QWEN_BATCH_ROWS prompts per weight pass ----
  struct BatchBuffers {
    Buffers pre;                                     // prefill activations for the longest prompt of the tile; kc / vc / Smax / prompt: per row
    int R;
    float *kc[QWEN_BATCH_ROWS], *vc[QWEN_BATCH_ROWS]; int Smax[QWEN_BATCH_ROWS], nsplit[QWEN_BATCH_ROWS];
    int *prompt[QWEN_BATCH_ROWS], *forced[QWEN_BATCH_ROWS], *out_ids[QWEN_BATCH_ROWS];
    float *xd, *qkvd, *attd, *hd, *logits;           // decode vectors, R rows each
    float* head_val; int* head_idx; unsigned* head_cnt; int head_blocks;      // [R][head_blocks], one counter
    float* attn_part; unsigned* attn_cnt; int part_stride, max_nsplit, max_cap;      // [R][part_stride], [R][Hkv]
    QwenState* st;                                   // [R]
    QwenBatchRow* rows;                       // [R], the per-row device table
    int *eos, *cols;
    size_t bytes;
  };
  struct BatchGraphKey {      // everything baked into a captured batched step: the workspace layout, grids and LDS sizes follow from the lengths;
                              // the rows' logits blocks are not in it (they come from the device table, written anew by every call)
    void* ws = nullptr; size_t ws_bytes = 0; std::vector<int> P, max_new; int n_eos = 0, n_cols = 0; bool forced = false, all_cols = false;
    bool operator==(const BatchGraphKey& o) const {
      return ws == o.ws && ws_bytes == o.ws_bytes && P == o.P && max_new == o.max_new && n_eos == o.n_eos && n_cols == o.n_cols &&
             forced == o.forced && all_cols == o.all_cols;
    }
  };
  struct BatchGraph { BatchGraphKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
  // kept steps, the latest used last: the tiles of a call differ in their lengths, so each has its own; the oldest leaves when full
  static constexpr int MAX_BATCH_GRAPHS = 8;
  std::vector<BatchGraph> bgraphs;
  int bgraph_kernel_nodes = -1;      // of the step captured last
  void drop_batch_graph();
  int batch_prepare();      // once, from finalize, on the model's device: function attributes of the batched kernels
  BatchBuffers carve_batch(void* ws, int R, const int* P, const int* max_new, int n_eos, int n_cols) const;
  // the largest tile's need: a call of B rows is served in consecutive tiles of QWEN_BATCH_ROWS on one workspace
  size_t batch_workspace_bytes(int B, const int* P, const int* max_new, int n_eos, int n_cols) const;
  int batch_head_tail(const BatchBuffers& w, int n_eos, bool forced, bool logits, int n_cols, bool all_cols, hipStream_t st);
  int batch_decode_step(const BatchBuffers& w, int n_eos, bool forced, bool logits, int n_cols, bool all_cols, hipStream_t st);
  int generate_tile(int R, const int* const* prompts, const int* P, const int* max_new, const int* eos_ids, int n_eos, const int* const* forced,
                    int* const* out_ids, int* n_out, float* const* out_logits, const int* logit_cols, int n_cols, bool all_cols, void* ws,
                    size_t ws_bytes, int use_graph, hipStream_t st);
  int generate_batch(int B, const int* prompt_ids, const int* n_prompt, const int* max_new, const int* eos_ids, int n_eos, const int* forced_ids,
                     int* out_ids, int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols, void* ws, size_t ws_bytes,
                     int use_graph, hipStream_t st);

  explicit QwenModel(const idxtts_qwen_config& c) : cfg(c) {}
  ~QwenModel() override;
  void drop_graph();
  bool accepts(const std::string& name) const override;
  int finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) override;
  Buffers carve(void* ws, int P, int max_new, int n_eos, int n_cols) const;
  size_t workspace_bytes(int P, int max_new, int n_eos, int n_cols) const { return carve(nullptr, P, max_new, n_eos, n_cols).bytes; }
  int prefill(const Buffers& w, int P, hipStream_t st);
  // the step's tail: final norm + head + argmax, the logits hand-over, then record / next embedding / advance
  int head_tail(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st);
  int decode_step(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st);
  int generate(const int* prompt_ids, int n_prompt, int max_new, const int* eos_ids, int n_eos, const int* forced_ids, int* out_ids,
               int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols, void* ws, size_t ws_bytes, int use_graph,
               hipStream_t st);
};


// ===========================================================================================================================
// Device code shared by qwen.hip and qwen_batch.hip.  Every function is a fixed sequence of operations: the single-prompt kernels
// and the batched ones inline the same definitions, which is what makes a row of a batch equal its own single call bit for bit.

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

enum { EPI_STORE = 0, EPI_RES = 1, EPI_SWIGLU = 2, EPI_HEAD = 3 };

struct QwenGemvArgs {
  const void* wa = nullptr;      // [N][K]; EPI_SWIGLU: gate_proj
  const void* wb = nullptr;      // EPI_SWIGLU: up_proj
  int K = 0, units = 0, upw = 1; // units: rows (EPI_RES), row pairs (EPI_STORE / EPI_HEAD), (gate, up) pairs (EPI_SWIGLU); per wave
  const float* x = nullptr;      // [K]
  const float* g = nullptr;      // RMSNorm gain [K], or null: x as it is
  float eps = 0.0f;
  float* y = nullptr;            // [N] (EPI_RES: y[n] += ...; EPI_SWIGLU: [units]; EPI_HEAD: the logits)
  float* part_val = nullptr; int* part_idx = nullptr; unsigned* cnt = nullptr; QwenState* st = nullptr;   // EPI_HEAD
};

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

// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per (kv head, key piece, query): the G q heads of the group against the piece's keys.  q (and, when APPEND, the new
// k) get their per-head RMSNorm and rotary here; APPEND also writes the new k / v to the cache (piece 0) and every piece takes them
// from LDS, so no workgroup waits for another's store.  Pass 1: threads = keys; pass 2: threads = (output feature, key parity).
struct QwenAttnArgs {
  const float* qkv = nullptr; int ld_qkv = 0;      // per query row [q: Hq*128 | k: Hkv*128 | v: Hkv*128]
  const float *qn_g = nullptr, *kn_g = nullptr; float eps = 0.0f;
  const float* rope = nullptr;                     // [pos][64][2]
  float *kc = nullptr, *vc = nullptr; int Smax = 0; // this layer's [Hkv][Smax][128]
  int Hq = 0, Hkv = 0, G = 0;
  float* out = nullptr; int ld_out = 0;            // per query row [Hq*128]
  const QwenState* st = nullptr; int pos0 = 0;     // query row r sits at position (st ? st->pos : pos0 + r)
  int nsplit = 1, slice_cap = 0;
  float* part = nullptr; unsigned* cnt = nullptr;  // [Hq][nsplit][130], [Hkv]
  float scale = 0.0f;
};

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
// ---------------------------------------------------------------------------------------------------------------------------
// The step's last launch (one workgroup): record the head's choice, pick what continues the sequence (the forced id, or the choice),
// stop on an end id or at the cap, write the next input's embedding row and advance the step scalars.
struct QwenTailArgs {
  QwenState* st; int* out_ids; const int* forced; const int* eos; int n_eos, max_new;
  const void* emb; int H, V; float* xd;
};
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

}  // namespace idxtts
