// Qwen3 causal LM, batched greedy generation (qwen.h): R <= QWEN_BATCH_ROWS prompts share every weight pass of a decode step.  The step
// keeps the launch plan of the single-prompt step in qwen.hip -- five launches a layer and the tail's three -- with every launch
// carrying all rows: a GEMV wave loads each weight fragment once and forms one dot product per row from it, the attention grid gets a
// row axis, the tail and the logits hand-over run one workgroup (column) per row.
//
// Contract: row b of a batched call equals generate(prompt_b, max_new_b, ...) bit for bit -- ids, stop step, every logit, either
// storage format, eager or replayed.  No row's arithmetic depends on another row, and every per-row operation is the one the
// single-prompt kernels inline from qwen.h: the same staging and RMSNorm of the activation vector, the same k -> lane map and FMA
// chain (chunk-major, then the 8 elements) and the same shuffle butterfly per dot product (so no MFMA here), the attention body
// with the row's OWN geometry (Smax_b, nsplit_b, slice) from a per-row device table, the same tail.  Rows that have finished ride
// along in the GEMVs (the weights are read anyway); they skip the attention, and nothing they compute is recorded.
//
// Row tile, QWEN_BATCH_ROWS = 8.  The R activation vectors are staged in LDS (R x chunks x 2 KiB, dynamic, sized by the rows in
// flight), the weight rows of a unit stay in registers, and each row's 8 k per chunk come back from LDS by two conflict-free
// ds_read_b128 (qwen_x_slot).  What 8 rows cost in occupancy, by K:
//   K <= 1024 (qkv, gate / up, head of the 0.6 B model): 32 KiB a workgroup, 5 workgroups = 5 waves a SIMD on the 160 KiB of a CU;
//   K  = 2048 (o_proj): 64 KiB, 2 workgroups a CU;  K = 3072 (down_proj): 96 KiB, 1 workgroup a CU, one wave a SIMD.
// The two large-K matrices have 1024 rows, i.e. 256 workgroups of four one-row waves -- one workgroup a CU whatever LDS allows --
// so the LDS limit takes nothing from them at this shape; registers (two weight rows of 6 chunks in fp32: 96 VGPRs, plus one row's
// 48 x values) leave 2 waves a SIMD on the 6-chunk template and more below.  16 rows would need 192 KiB at K = 3072: over a CU's LDS.
// A tile of one row (B = 1, or the last row of an over-full call) has nothing to share: generate_batch hands it to the single-prompt
// path, QwenModel::generate, on the same workspace and stream -- its kernels, its kept step graph, its cost.
//
// Step graphs: a captured step bakes in the tile's workspace layout, i.e. every row's prompt length and cap.  Tiles of real texts
// differ in these, so up to MAX_BATCH_GRAPHS steps are kept, one per key, and the one unused longest leaves; a tile whose lengths
// have not been seen pays one capture and instantiation.  The rows' logits blocks are not baked in (they are read from the device table).
//
// Prefill is not batched: the single-prompt prefill runs once per row into that row's cache region (a packed prefill would change
// the GEMM's M and is not claimed to keep the contract).
#include "qwen.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "model_util.h"

namespace idxtts {

// what differs between the rows of a tile, on the device; everything else is row b of an array
struct QwenBatchRow {
  float *kc, *vc;            // the row's cache, [L][Hkv][Smax][128] each
  int Smax, nsplit, max_new, pad;
  int* out_ids;
  const int* forced;
  float* out_logits;         // the row's block [max_new][n_cols], or null
};

namespace {

constexpr int HD = QWEN_HD;

struct QwenBatchGemvArgs {
  QwenGemvArgs a;            // x: [R][K]; st: [R]; part_val / part_idx: [R][part_stride]
  int R = 0, ldy = 0, part_stride = 0;
};

// qwen_gemv_body (qwen.h) with the full row tile: R <= QWEN_BATCH_ROWS rows run
template <int NCH, int EPI, typename WT>
__global__ __launch_bounds__(256) void qwen_gemv_batch_kernel(const QwenBatchGemvArgs q) {
  extern __shared__ __attribute__((aligned(16))) float xs[];      // [R][NCH * 512], slots by qwen_x_slot
  qwen_gemv_body<NCH, EPI, WT, QWEN_BATCH_ROWS>(q.a, xs, q.R, q.ldy, q.part_stride);
}

template <int NCH, int EPI, typename WT>
int gemv_batch_launch_one(const QwenBatchGemvArgs& a, int blocks, hipStream_t st) {
  const size_t lds = (size_t)a.R * NCH * 512 * sizeof(float);      // above 64 KiB: allowed by QwenModel::batch_prepare
  hipLaunchKernelGGL((qwen_gemv_batch_kernel<NCH, EPI, WT>), dim3(blocks), dim3(256), lds, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

template <int EPI, typename WT>
int gemv_batch_launch_fmt(const QwenBatchGemvArgs& a, int blocks, hipStream_t st) {
  const int nch = cdiv(a.a.K, 512);
  if (nch <= 1) return gemv_batch_launch_one<1, EPI, WT>(a, blocks, st);
  if (nch <= 2) return gemv_batch_launch_one<2, EPI, WT>(a, blocks, st);
  if (nch <= 4) return gemv_batch_launch_one<4, EPI, WT>(a, blocks, st);
  return gemv_batch_launch_one<6, EPI, WT>(a, blocks, st);
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

int gemv_blocks(const QwenGemvArgs& a) { return cdiv(a.units, 4 * a.upw); }

// rows: weight rows streamed (for the profile's byte count)
template <int EPI>
int qwen_gemv_batch(const QwenBatchGemvArgs& a, int fmt, int rows, hipStream_t st) {
  IDX_CHECK(a.a.K >= 8 && a.a.K % 8 == 0 && a.a.K <= 3072, "GEMV K must be a multiple of 8, at most 3072");
  IDX_CHECK(a.a.units > 0 && a.a.upw > 0 && a.R >= 1 && a.R <= QWEN_BATCH_ROWS, "GEMV shape");
  static const int cat = prof_register("qwen_gemv_batch_kernel");
  ProfScope prof(cat, st, 2.0 * a.R * rows * a.a.K, (double)rows * a.a.K * (fmt == QWEN_W_BF16 ? 2 : 4));
  const int blocks = gemv_blocks(a.a);
  return fmt == QWEN_W_BF16 ? gemv_batch_launch_fmt<EPI, unsigned short>(a, blocks, st) : gemv_batch_launch_fmt<EPI, float>(a, blocks, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode attention, grid (kv head, key piece, row): the row's geometry -- what its own single call would use -- from the table.
// Pieces the row does not have, and rows that are done, return at entry without arriving; counters are per (row, kv head).
struct QwenBatchAttnArgs {
  QwenAttnArgs a;            // qkv / out: [R][ld]; st: [R]; part: [R][part_stride]; cnt: [R][Hkv]; kc / vc / Smax / nsplit / slice_cap: per row
  const QwenBatchRow* rows = nullptr;
  int layer = 0, part_stride = 0;
};
__global__ __launch_bounds__(256) void qwen_attn_batch_kernel(const QwenBatchAttnArgs q) {
  const int z = blockIdx.y, b = blockIdx.z;
  const QwenBatchRow row = q.rows[b];
  const QwenState* st = q.a.st + b;
  if (z >= row.nsplit || st->done) return;      // the whole workgroup
  QwenAttnArgs a = q.a;
  const size_t off = (size_t)q.layer * a.Hkv * row.Smax * HD;
  a.kc = row.kc + off; a.vc = row.vc + off; a.Smax = row.Smax;
  a.nsplit = row.nsplit; a.slice_cap = (row.Smax + row.nsplit - 1) / row.nsplit;
  a.part += (size_t)b * q.part_stride; a.cnt += b * a.Hkv; a.st = st;
  qwen_attn_body<true>(a, blockIdx.x, z, b, st->pos);
}

// ---------------------------------------------------------------------------------------------------------------------------
struct QwenBatchTailArgs {
  QwenTailArgs t;            // st: [R]; xd: [R][H]; out_ids / forced / max_new: per row
  const QwenBatchRow* rows;
  int forced;
};
template <typename WT>
__global__ __launch_bounds__(256) void qwen_tail_batch_kernel(const QwenBatchTailArgs q) {
  const int b = blockIdx.x;
  const QwenBatchRow row = q.rows[b];
  QwenTailArgs t = q.t;
  t.st += b; t.xd += (size_t)b * t.H; t.out_ids = row.out_ids; t.forced = q.forced ? row.forced : nullptr; t.max_new = row.max_new;
  qwen_tail_row<WT>(t);
}

__global__ __launch_bounds__(256) void qwen_logits_batch_kernel(const QwenState* st, const float* logits, int V, const int* cols, int n_cols,
                                                                const QwenBatchRow* rows) {
  const int b = blockIdx.y;
  const QwenBatchRow row = rows[b];
  qwen_logits_row(st + b, logits + (size_t)b * V, cols, n_cols, row.max_new, row.out_logits, blockIdx.x * 256 + threadIdx.x);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
static void destroy_batch_graph(QwenModel::BatchGraph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr; g.graph = nullptr;
}

int QwenModel::batch_prepare() {
  IDX_HIP(gemv_batch_allow_lds_fmt<float>());
  IDX_HIP(gemv_batch_allow_lds_fmt<unsigned short>());
  return 0;
}

void QwenModel::drop_batch_graph() {
  for (BatchGraph& g : bgraphs) destroy_batch_graph(g);
  bgraphs.clear();
}

QwenModel::BatchBuffers QwenModel::carve_batch(void* ws, int R, const int* P, const int* max_new, int n_eos, int n_cols) const {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, L = cfg.num_hidden_layers, V = cfg.vocab_size;
  BatchBuffers b;
  memset(&b, 0, sizeof(b));
  Carver c(ws);
  b.R = R;
  int Pmax = 0;
  for (int r = 0; r < R; ++r) Pmax = std::max(Pmax, P[r]);
  Buffers& w = b.pre;
  w.x = c.take<float>((size_t)Pmax * H);
  w.x2 = c.take<float>((size_t)Pmax * H);
  w.xn = c.take<float>((size_t)Pmax * H);
  w.qkv = c.take<float>((size_t)Pmax * qkvdim());
  w.att = c.take<float>((size_t)Pmax * qdim());
  w.gu = c.take<float>((size_t)Pmax * 2 * I);
  w.hmid = c.take<float>((size_t)Pmax * I);
  for (int r = 0; r < R; ++r) {
    b.Smax[r] = (P[r] + max_new[r] + 3) & ~3;
    b.nsplit[r] = qwen_nsplit_for(b.Smax[r]);
    b.max_nsplit = std::max(b.max_nsplit, b.nsplit[r]);
    b.max_cap = std::max(b.max_cap, cdiv(b.Smax[r], b.nsplit[r]));
    const size_t kv = (size_t)L * cfg.num_key_value_heads * b.Smax[r] * HD;
    b.kc[r] = c.take<float>(kv);
    b.vc[r] = c.take<float>(kv);
    b.prompt[r] = c.take<int>(P[r]);
    b.forced[r] = c.take<int>(max_new[r]);
    b.out_ids[r] = c.take<int>(max_new[r]);
  }
  b.xd = c.take<float>((size_t)R * H);
  b.qkvd = c.take<float>((size_t)R * qkvdim());
  b.attd = c.take<float>((size_t)R * qdim());
  b.hd = c.take<float>((size_t)R * I);
  b.logits = c.take<float>((size_t)R * V);
  b.head_blocks = cdiv(V / 2, 4 * QWEN_HEAD_UPW);
  b.head_val = c.take<float>((size_t)R * b.head_blocks);
  b.head_idx = c.take<int>((size_t)R * b.head_blocks);
  b.head_cnt = c.take<unsigned>(1);
  b.part_stride = cfg.num_attention_heads * b.max_nsplit * 130;
  b.attn_part = c.take<float>((size_t)R * b.part_stride);
  b.attn_cnt = c.take<unsigned>((size_t)R * cfg.num_key_value_heads);
  b.st = c.take<QwenState>(R);
  b.rows = c.take<QwenBatchRow>(R);
  b.eos = c.take<int>(std::max(1, n_eos));
  b.cols = c.take<int>(std::max(1, n_cols));
  b.bytes = (c.off + 255) & ~(size_t)255;
  return b;
}

size_t QwenModel::batch_workspace_bytes(int B, const int* P, const int* max_new, int n_eos, int n_cols) const {
  size_t need = 0;
  for (int t0 = 0; t0 < B; t0 += QWEN_BATCH_ROWS)
    need = std::max(need, B - t0 == 1 ? workspace_bytes(P[t0], max_new[t0], n_eos, n_cols)      // a one-row tile runs the single-prompt path
                                      : carve_batch(nullptr, std::min(QWEN_BATCH_ROWS, B - t0), P + t0, max_new + t0, n_eos, n_cols).bytes);
  return need;
}

int QwenModel::batch_head_tail(const BatchBuffers& w, int n_eos, bool forced, bool logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, V = cfg.vocab_size, R = w.R;
  QwenBatchGemvArgs h;
  QwenGemvArgs& a = h.a;
  a.wa = head_s.w; a.K = H; a.units = V / 2; a.upw = QWEN_HEAD_UPW; a.x = w.xd; a.g = norm_g; a.eps = cfg.rms_norm_eps; a.y = w.logits;
  a.part_val = w.head_val; a.part_idx = w.head_idx; a.cnt = w.head_cnt; a.st = w.st;
  h.R = R; h.ldy = V; h.part_stride = w.head_blocks;
  IDX_CHECK(gemv_blocks(a) == w.head_blocks, "head partial buffers");
  if (qwen_gemv_batch<EPI_HEAD>(h, fmt, V, st)) return 1;
  if (logits) {
    static const int cat = prof_register("qwen_logits_batch_kernel");
    ProfScope prof(cat, st, 0.0, 8.0 * R * n_cols);
    hipLaunchKernelGGL(qwen_logits_batch_kernel, dim3(cdiv(n_cols, 256), R), dim3(256), 0, st, w.st, w.logits, V, all_cols ? nullptr : w.cols, n_cols,
                       w.rows);
    IDX_LAUNCH_CHECK();
  }
  QwenBatchTailArgs q;
  memset(&q, 0, sizeof(q));
  q.t.st = w.st; q.t.eos = w.eos; q.t.n_eos = n_eos; q.t.emb = embed_s.w; q.t.H = H; q.t.V = V; q.t.xd = w.xd;
  q.rows = w.rows; q.forced = forced ? 1 : 0;
  static const int cat = prof_register("qwen_tail_batch_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * R * H);
  if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_tail_batch_kernel<unsigned short>, dim3(R), dim3(256), 0, st, q);
  else hipLaunchKernelGGL(qwen_tail_batch_kernel<float>, dim3(R), dim3(256), 0, st, q);
  IDX_LAUNCH_CHECK();
  return 0;
}

int QwenModel::batch_decode_step(const BatchBuffers& w, int n_eos, bool forced, bool logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, QD = qdim(), QKV = qkvdim(), R = w.R;
  const int Hq = cfg.num_attention_heads, Hkv = cfg.num_key_value_heads, G = Hq / Hkv;
  const size_t lds = (size_t)G * w.max_cap * sizeof(float);
  IDX_CHECK(lds <= 40 * 1024, "context too long for the attention kernel's score buffer");
  int keys = 0;
  for (int r = 0; r < R; ++r) keys += w.Smax[r];
  for (int li = 0; li < cfg.num_hidden_layers; ++li) {
    const QwenLayer& Y = layers[li];
    QwenBatchGemvArgs q;      // qkv = [q_proj; k_proj; v_proj] RMSNorm(x)
    q.a.wa = Y.qkv_s.w; q.a.K = H; q.a.units = QKV / 2; q.a.x = w.xd; q.a.g = Y.in_g; q.a.eps = cfg.rms_norm_eps; q.a.y = w.qkvd;
    q.R = R; q.ldy = QKV;
    if (qwen_gemv_batch<EPI_STORE>(q, fmt, QKV, st)) return 1;
    {
      QwenBatchAttnArgs b;
      QwenAttnArgs& a = b.a;
      a.qkv = w.qkvd; a.ld_qkv = QKV; a.qn_g = Y.qn_g; a.kn_g = Y.kn_g; a.eps = cfg.rms_norm_eps; a.rope = rope;
      a.Hq = Hq; a.Hkv = Hkv; a.G = G; a.out = w.attd; a.ld_out = QD; a.st = w.st;
      a.part = w.attn_part; a.cnt = w.attn_cnt; a.scale = 1.0f / sqrtf((float)HD);
      b.rows = w.rows; b.layer = li; b.part_stride = w.part_stride;
      static const int cat = prof_register("qwen_attn_batch_kernel");
      ProfScope prof(cat, st, 4.0 * Hq * (double)keys * HD, 8.0 * Hkv * (double)keys * HD);
      hipLaunchKernelGGL(qwen_attn_batch_kernel, dim3(Hkv, w.max_nsplit, R), dim3(256), lds, st, b);
      IDX_LAUNCH_CHECK();
    }
    QwenBatchGemvArgs o;      // x += o_proj(att)
    o.a.wa = Y.o_s.w; o.a.K = QD; o.a.units = H; o.a.x = w.attd; o.a.y = w.xd; o.R = R; o.ldy = H;
    if (qwen_gemv_batch<EPI_RES>(o, fmt, H, st)) return 1;
    QwenBatchGemvArgs g;      // h = silu(gate_proj(n)) * up_proj(n), n = RMSNorm(x)
    g.a.wa = Y.gate_s.w; g.a.wb = Y.up_s.w; g.a.K = H; g.a.units = I; g.a.x = w.xd; g.a.g = Y.post_g; g.a.eps = cfg.rms_norm_eps; g.a.y = w.hd;
    g.R = R; g.ldy = I;
    if (qwen_gemv_batch<EPI_SWIGLU>(g, fmt, 2 * I, st)) return 1;
    QwenBatchGemvArgs d;      // x += down_proj(h)
    d.a.wa = Y.down_s.w; d.a.K = I; d.a.units = H; d.a.x = w.hd; d.a.y = w.xd; d.R = R; d.ldy = H;
    if (qwen_gemv_batch<EPI_RES>(d, fmt, H, st)) return 1;
  }
  return batch_head_tail(w, n_eos, forced, logits, n_cols, all_cols, st);
}

// one tile: the arrays hold R host pointers / lengths; out_logits[r]: the row's device block, or null for every row
int QwenModel::generate_tile(int R, const int* const* prompts, const int* P, const int* max_new, const int* eos_ids, int n_eos,
                             const int* const* forced_ids, int* const* out_ids, int* n_out, float* const* out_logits, const int* logit_cols,
                             int n_cols, bool all_cols, void* ws, size_t ws_bytes, int use_graph, hipStream_t st) {
  const int H = cfg.hidden_size;
  const bool forced = forced_ids != nullptr, logits = out_logits != nullptr;
  const BatchBuffers w = carve_batch(ws, R, P, max_new, n_eos, n_cols);
  IDX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small");
  QwenBatchRow rows[QWEN_BATCH_ROWS];
  QwenState s0[QWEN_BATCH_ROWS];
  memset(rows, 0, sizeof(rows));
  memset(s0, 0, sizeof(s0));
  int Nmax = 0;
  for (int r = 0; r < R; ++r) {
    rows[r].kc = w.kc[r]; rows[r].vc = w.vc[r]; rows[r].Smax = w.Smax[r]; rows[r].nsplit = w.nsplit[r]; rows[r].max_new = max_new[r];
    rows[r].out_ids = w.out_ids[r]; rows[r].forced = w.forced[r]; rows[r].out_logits = logits ? out_logits[r] : nullptr;
    s0[r].pos = P[r] - 1;      // the tail of the prefill's head step moves it to P, the first generated token's position
    Nmax = std::max(Nmax, max_new[r]);
    IDX_HIP(hipMemcpyAsync(w.prompt[r], prompts[r], P[r] * sizeof(int), hipMemcpyHostToDevice, st));
    if (forced) IDX_HIP(hipMemcpyAsync(w.forced[r], forced_ids[r], max_new[r] * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipMemsetAsync(w.out_ids[r], 0, max_new[r] * sizeof(int), st));
  }
  IDX_HIP(hipMemcpyAsync(w.rows, rows, R * sizeof(QwenBatchRow), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.st, s0, R * sizeof(QwenState), hipMemcpyHostToDevice, st));
  if (n_eos) IDX_HIP(hipMemcpyAsync(w.eos, eos_ids, n_eos * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_cols && !all_cols) IDX_HIP(hipMemcpyAsync(w.cols, logit_cols, n_cols * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.head_cnt, 0, sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.attn_cnt, 0, (size_t)R * cfg.num_key_value_heads * sizeof(unsigned), st));
  IDX_HIP(hipStreamSynchronize(st));      // the host arrays above are the caller's, or this frame's

  for (int r = 0; r < R; ++r) {      // the single-prompt prefill, row by row, into the row's cache
    Buffers pw = w.pre;
    pw.kc = w.kc[r]; pw.vc = w.vc[r]; pw.Smax = w.Smax[r]; pw.prompt = w.prompt[r];
    if (prefill(pw, P[r], st)) return 1;
    IDX_HIP(hipMemcpyAsync(w.xd + (size_t)r * H, pw.x + (size_t)(P[r] - 1) * H, H * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (batch_head_tail(w, n_eos, forced, logits, n_cols, all_cols, st)) return 1;

  const bool graph_ok = use_graph && !prof_enabled() && Nmax > 2;
  hipGraphExec_t exec = nullptr;
  int n_first = 1;
  if (graph_ok) {
    BatchGraphKey key;
    key.ws = ws; key.ws_bytes = ws_bytes; key.P.assign(P, P + R); key.max_new.assign(max_new, max_new + R); key.n_eos = n_eos; key.n_cols = n_cols;
    key.forced = forced; key.all_cols = all_cols;
    const auto hit = std::find_if(bgraphs.begin(), bgraphs.end(), [&](const BatchGraph& g) { return g.key == key; });
    if (hit != bgraphs.end()) {
      std::rotate(hit, hit + 1, bgraphs.end());      // the latest used last
      exec = bgraphs.back().exec;
    } else {
      if ((int)bgraphs.size() >= MAX_BATCH_GRAPHS) {
        destroy_batch_graph(bgraphs.front());
        bgraphs.erase(bgraphs.begin());
      }
      // step 1 runs eagerly (a first launch may load code objects, which a capture refuses), then one step is captured
      if (batch_decode_step(w, n_eos, forced, logits, n_cols, all_cols, st)) return 1;
      n_first = 2;
      BatchGraph g;
      g.key = key;
      IDX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const int rc = batch_decode_step(w, n_eos, forced, logits, n_cols, all_cols, st);
      const hipError_t e = hipStreamEndCapture(st, &g.graph);
      if (rc || e != hipSuccess) destroy_batch_graph(g);
      if (rc) return 1;
      IDX_HIP(e);
      size_t n_nodes = 0;
      hipError_t en = hipGraphGetNodes(g.graph, nullptr, &n_nodes);
      std::vector<hipGraphNode_t> nodes(n_nodes);
      if (en == hipSuccess && n_nodes) en = hipGraphGetNodes(g.graph, nodes.data(), &n_nodes);
      bool kernels_only = true;
      for (size_t i = 0; en == hipSuccess && i < n_nodes; ++i) {
        hipGraphNodeType ty;
        en = hipGraphNodeGetType(nodes[i], &ty);
        kernels_only = kernels_only && ty == hipGraphNodeTypeKernel;
      }
      if (en == hipSuccess) en = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
      if (en != hipSuccess || !kernels_only) destroy_batch_graph(g);
      IDX_HIP(en);
      IDX_CHECK(kernels_only, "the captured decode step holds a node that is not a kernel launch");
      bgraph_kernel_nodes = (int)n_nodes;
      bgraphs.push_back(g);
      exec = g.exec;
    }
  }
  QwenState hs[QWEN_BATCH_ROWS];
  for (int n = n_first; n < Nmax; ++n) {
    if (exec) IDX_HIP(hipGraphLaunch(exec, st));
    else if (batch_decode_step(w, n_eos, forced, logits, n_cols, all_cols, st)) return 1;
    if ((n + 1) % 8 == 0 && n + 1 < Nmax) {      // look every 8 steps: when every row is done, later launches change nothing
      IDX_HIP(hipMemcpyAsync(hs, w.st, R * sizeof(QwenState), hipMemcpyDeviceToHost, st));
      IDX_HIP(hipStreamSynchronize(st));
      bool all = true;
      for (int r = 0; r < R; ++r) all = all && hs[r].done;
      if (all) break;
    }
  }
  IDX_HIP(hipMemcpyAsync(hs, w.st, R * sizeof(QwenState), hipMemcpyDeviceToHost, st));
  for (int r = 0; r < R; ++r) IDX_HIP(hipMemcpyAsync(out_ids[r], w.out_ids[r], max_new[r] * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < R; ++r) {
    IDX_CHECK(hs[r].n_out >= 1 && hs[r].n_out <= max_new[r], "generation state");
    n_out[r] = hs[r].n_out;
  }
  return 0;
}

int QwenModel::generate_batch(int B, const int* prompt_ids, const int* n_prompt, const int* max_new, const int* eos_ids, int n_eos,
                              const int* forced_ids, int* out_ids, int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols, void* ws,
                              size_t ws_bytes, int use_graph, hipStream_t user) {
  IDX_CHECK(prompt_ids && n_prompt && max_new && out_ids && n_out, "null pointer");
  IDX_CHECK(B > 0 && n_eos >= 0 && (n_eos == 0 || eos_ids), "shape");
  const int V = cfg.vocab_size;
  const bool all_cols = out_logits && !logit_cols;
  const int n_cols = out_logits ? (all_cols ? V : n_logit_cols) : 0;
  IDX_CHECK(!out_logits || n_cols > 0, "n_logit_cols");
  // every row is checked before anything runs
  std::vector<size_t> p_off(B + 1, 0), m_off(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    IDX_CHECK(n_prompt[b] > 0 && max_new[b] > 0, "shape");
    p_off[b + 1] = p_off[b] + n_prompt[b];
    m_off[b + 1] = m_off[b] + max_new[b];
  }
  for (size_t i = 0; i < p_off[B]; ++i) IDX_CHECK(prompt_ids[i] >= 0 && prompt_ids[i] < V, "prompt id outside the vocabulary");
  for (size_t i = 0; forced_ids && i < m_off[B]; ++i) IDX_CHECK(forced_ids[i] >= 0 && forced_ids[i] < V, "forced id outside the vocabulary");
  for (int i = 0; i < n_cols && !all_cols; ++i) IDX_CHECK(logit_cols[i] >= 0 && logit_cols[i] < V, "logit column outside the vocabulary");
  for (int b = 0; b < B; ++b)
    IDX_CHECK(((n_prompt[b] + max_new[b] + 3) & ~3) <= cfg.max_context, "prompt + max_new_tokens exceeds the context the model was created for");
  IDX_CHECK(ws && ws_bytes >= batch_workspace_bytes(B, n_prompt, max_new, n_eos, n_cols), "workspace too small");
  hipStream_t st = user;
  if (!user) {      // the legacy default stream cannot be captured: run on a private stream, after what the caller has queued
    if (!own_stream) IDX_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    IDX_HIP(hipStreamSynchronize(user));
    st = own_stream;
  }
  for (int t0 = 0; t0 < B; t0 += QWEN_BATCH_ROWS) {      // consecutive tiles on the one workspace; each ends with the stream finished
    const int R = std::min(QWEN_BATCH_ROWS, B - t0);
    const int* prompts[QWEN_BATCH_ROWS]; const int* forced[QWEN_BATCH_ROWS]; int* outs[QWEN_BATCH_ROWS]; float* lg[QWEN_BATCH_ROWS];
    for (int r = 0; r < R; ++r) {
      prompts[r] = prompt_ids + p_off[t0 + r];
      forced[r] = forced_ids ? forced_ids + m_off[t0 + r] : nullptr;
      outs[r] = out_ids + m_off[t0 + r];
      lg[r] = out_logits ? out_logits + m_off[t0 + r] * (size_t)n_cols : nullptr;
    }
    if (R == 1) {      // nothing to share: the single-prompt path
      if (generate(prompts[0], n_prompt[t0], max_new[t0], eos_ids, n_eos, forced[0], outs[0], n_out + t0, lg[0], logit_cols, n_logit_cols, ws, ws_bytes,
                   use_graph, st))
        return 1;
      continue;
    }
    if (generate_tile(R, prompts, n_prompt + t0, max_new + t0, eos_ids, n_eos, forced_ids ? forced : nullptr, outs, n_out + t0,
                      out_logits ? lg : nullptr, logit_cols, n_cols, all_cols, ws, ws_bytes, use_graph, st))
      return 1;
  }
  return 0;
}

}  // namespace idxtts

using namespace idxtts;

extern "C" {

int idxtts_qwen_max_batch(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  return dynamic_cast<const QwenModel*>(ctx->model.get()) ? QWEN_BATCH_ROWS : -1;
}

size_t idxtts_qwen_batch_workspace_bytes(const idxtts_ctx* ctx, int B, const int* n_prompt, const int* max_new_tokens, int n_eos, int n_logit_cols) {
  if (!ctx || B < 1 || !n_prompt || !max_new_tokens || n_eos < 0 || n_logit_cols < 0) return 0;
  for (int b = 0; b < B; ++b)
    if (n_prompt[b] <= 0 || max_new_tokens[b] <= 0) return 0;
  auto* m = dynamic_cast<const QwenModel*>(ctx->model.get());
  return m ? m->batch_workspace_bytes(B, n_prompt, max_new_tokens, n_eos, n_logit_cols) : 0;
}

int idxtts_qwen_generate_batch(idxtts_ctx* ctx, int B, const int* prompt_ids, const int* n_prompt, const int* max_new_tokens, const int* eos_ids,
                               int n_eos, const int* forced_ids, int* out_ids, int* n_out, float* out_logits, const int* logit_cols,
                               int n_logit_cols, void* workspace, size_t bytes, int use_graph, void* stream) {
  try {
    IDX_CHECK(ctx && ctx->finalized, "context not finalized");
    auto* m = dynamic_cast<QwenModel*>(ctx->model.get());
    IDX_CHECK(m, "not a Qwen context");
    return m->generate_batch(B, prompt_ids, n_prompt, max_new_tokens, eos_ids, n_eos, forced_ids, out_ids, n_out, out_logits, logit_cols,
                             n_logit_cols, workspace, bytes, use_graph, static_cast<hipStream_t>(stream));
  } catch (const std::exception& e) { return fail(__FILE__, __LINE__, std::string("exception: ") + e.what()); }
}

int idxtts_qwen_batch_step_graph_launches(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  auto* m = dynamic_cast<const QwenModel*>(ctx->model.get());
  return m && !m->bgraphs.empty() ? m->bgraph_kernel_nodes : -1;
}

}  // extern "C"
