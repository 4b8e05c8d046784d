// Qwen3 causal LM, greedy generation for a tile of R <= QWEN_BATCH_ROWS prompts that share each weight pass (a single prompt is a tile of
// one row): the emotion-from-text classifier of the reference (QwenEmotion, infer_v2.py:948-1063).
// RMSNorm, per-head q/k RMSNorm, rotary positions, grouped-query attention at head_dim 128, SwiGLU MLP, (tied) vocabulary head.
// fp32 arithmetic; linear weights stored fp32 or bf16 (exact for a bf16 checkpoint).  This header: the model, the kernels' argument
// structs and their launchers.  qwen_kernels.hip: every kernel and its launcher.  qwen.hip: loading, the workspace, the step, generation, C API.
#pragma once
#include <algorithm>
#include <array>
#include <functional>
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
constexpr int QWEN_BATCH_ROWS = 8;    // prompts that share one weight pass of a step (qwen_kernels.hip: what the choice costs)

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

// what differs between the rows of a tile of several, on the device; everything else is row b of an array
struct QwenBatchRow {
  float *kc, *vc;            // the row's cache, [L][Hkv][Smax][128] each
  int Smax, nsplit, max_new, pad;
  int* out_ids;
  const int* forced;
  float* out_logits;         // the row's block [max_new][n_cols], or null
};

// ---- the kernels' arguments and launchers (qwen_kernels.hip).  One row: the single-row kernels, geometry from the arguments;
// several: the row-tile kernels, each row's geometry from the table `rows`.  Either way a row's arithmetic is the same code. ----
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
  int R = 1, ldy = 0, part_stride = 0;      // rows of x; then x: [R][K], y: [R][ldy], st: [R], part_val / part_idx: [R][part_stride]
};
int qwen_gemv_blocks(const QwenGemvArgs& a);
// w_rows: weight rows streamed (the profile's byte count)
int qwen_gemv(int epi, const QwenGemvArgs& a, int fmt, int w_rows, hipStream_t st);

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
  // several rows (decode only): qkv / out / st: [R]; part: [R][part_stride]; cnt: [R][Hkv]; kc / vc / Smax / nsplit / slice_cap of a row
  // from rows[r] at `layer`, the host's nsplit / slice_cap being the largest of any row (grid and LDS).  Pieces a row does not have,
  // and rows that are done, return at entry without arriving.
  const QwenBatchRow* rows = nullptr; int layer = 0, part_stride = 0;
};
// rows: queries (the grid's z); query_keys, keys: (query, key) pairs and cache rows read, for the profile
int qwen_attn(const QwenAttnArgs& a, int rows, bool append, double query_keys, double keys, hipStream_t st);

// The step's last launch (one workgroup): record the head's choice, pick what continues the sequence (the forced id, or the choice),
// stop on an end id or at the cap, write the next input's embedding row and advance the step scalars.
struct QwenTailArgs {
  QwenState* st; int* out_ids; const int* forced; const int* eos; int n_eos, max_new;
  const void* emb; int H, V; float* xd;
  const QwenBatchRow* rows; int use_forced;      // several rows: st: [R]; xd: [R][H]; out_ids / forced (when use_forced) / max_new from rows[r]
};
int qwen_tail(const QwenTailArgs& t, int R, int fmt, hipStream_t st);
// out_logits[step][c] = logits[cols[c]] (cols null: column c) of a live step.  rows null: one row, into out; else row r of logits [R][V] into rows[r].out_logits
int qwen_logits(const QwenState* st, const float* logits, int V, const int* cols, int n_cols, int R, int max_new, float* out, const QwenBatchRow* rows,
                hipStream_t s);
// prefill helpers (once per call): P rows each.  qwen_kv_store: keys (RMSNorm + rotary) and values of positions 0 .. P-1 into a's cache
int qwen_embed_rows(float* x, const int* ids, const void* emb, int P, int H, int V, int fmt, hipStream_t st);
int qwen_rmsnorm_rows(const float* x, float* y, const float* g, int P, int H, float eps, hipStream_t st);
int qwen_kv_store(const QwenAttnArgs& a, int P, hipStream_t st);
int qwen_silu_mul(const float* gu, float* h, int P, int I, hipStream_t st);
int qwen_kernels_prepare();      // once per device, before the first launch: function attributes of the row-tile GEMVs

struct QwenStream {      // a weight matrix [N][K] row-major in the decode format
  const void* w = nullptr;
  int N = 0, K = 0;
};

struct QwenLayer {
  const float *in_g = nullptr, *post_g = nullptr, *qn_g = nullptr, *kn_g = nullptr;
  LinearWeights qkv_l, o_l, gu_l, down_l;      // MFMA-packed fp32 (prefill)
  QwenStream qkv_s, o_s, gate_s, up_s, down_s; // decode streams
};

// Captured decode steps, at most `cap` of them, the latest used last; the one unused longest leaves when full.
class QwenStepGraphs {
 public:
  // everything baked into a captured step: the workspace layout, grids and LDS sizes follow from the lengths.  out_logits: set at one
  // row only, where it is a launch argument (the blocks of several rows come from the device table, written anew by every call).
  struct Key {
    void* ws = nullptr; size_t ws_bytes = 0; int R = 0; std::array<int, QWEN_BATCH_ROWS> P{}, max_new{}; int n_eos = 0, n_cols = 0;
    bool forced = false, all_cols = false; float* out_logits = nullptr;
    bool operator==(const Key& o) const {
      return ws == o.ws && ws_bytes == o.ws_bytes && R == o.R && P == o.P && max_new == o.max_new && n_eos == o.n_eos && n_cols == o.n_cols &&
             forced == o.forced && all_cols == o.all_cols && out_logits == o.out_logits;
    }
  };
  explicit QwenStepGraphs(int cap) : cap_(cap) {}
  ~QwenStepGraphs() { clear(); }
  QwenStepGraphs(const QwenStepGraphs&) = delete;
  QwenStepGraphs& operator=(const QwenStepGraphs&) = delete;
  // The kept step of `key`; or, *captured set, a new one: step() once eagerly, once under capture on st.  A failure keeps nothing of it.
  int get(const Key& key, hipStream_t st, const std::function<int()>& step, hipGraphExec_t* exec, bool* captured);
  int launches() const { return kept_.empty() ? -1 : kernel_nodes_; }      // of the step captured last; -1: none held
  void clear();

 private:
  struct Entry { Key key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
  static void destroy(Entry& e);
  int cap_;
  std::vector<Entry> kept_;
  int kernel_nodes_ = -1;
};

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

  // the workspace of R <= QWEN_BATCH_ROWS prompts that share each weight pass
  struct Tile {
    int R;
    float *x, *x2, *xn, *qkv, *att, *gu, *hmid;      // prefill activations, sized for the longest prompt
    float *kc[QWEN_BATCH_ROWS], *vc[QWEN_BATCH_ROWS]; int Smax[QWEN_BATCH_ROWS], nsplit[QWEN_BATCH_ROWS];      // [L][Hkv][Smax][128] each
    int *prompt[QWEN_BATCH_ROWS], *forced[QWEN_BATCH_ROWS], *out_ids[QWEN_BATCH_ROWS]; int max_new[QWEN_BATCH_ROWS];
    float *xd, *qkvd, *attd, *hd, *logits;           // decode vectors, R rows each
    float* head_val; int* head_idx; unsigned* head_cnt; int head_blocks;      // [R][head_blocks], one counter
    float* attn_part; unsigned* attn_cnt; int part_stride, max_nsplit, max_cap, keys;      // [R][part_stride], [R][Hkv]; keys: every row's Smax together
    QwenState* st;                                   // [R]
    QwenBatchRow* rows;                              // [R], the per-row device table; null at R == 1
    int *eos, *cols;
    size_t bytes;
  };
  // kept steps: one for one-row tiles; several for larger ones, whose lengths differ from tile to tile of a call
  static constexpr int MAX_BATCH_GRAPHS = 8;
  QwenStepGraphs graphs1{1}, graphs{MAX_BATCH_GRAPHS};
  hipStream_t own_stream = nullptr;

  explicit QwenModel(const idxtts_qwen_config& c) : cfg(c) {}
  ~QwenModel() override;
  bool accepts(const std::string& name) const override;
  int finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) override;
  Tile carve(void* ws, int R, const int* P, const int* max_new, int n_eos, int n_cols) const;
  // the largest tile's need: a call of B rows is served in consecutive tiles of QWEN_BATCH_ROWS on one workspace
  size_t workspace_bytes(int B, const int* P, const int* max_new, int n_eos, int n_cols) const;
  int prefill(const Tile& w, int r, int P, hipStream_t st);      // row r's prompt into its cache; its last position's hidden state into xd
  // the step's tail: final norm + head + argmax, the logits hand-over, then record / next embedding / advance.
  // out_logits: null, or the rows' device blocks (one row: a launch argument; several: already in the table)
  int head_tail(const Tile& w, int n_eos, bool forced, float* const* out_logits, int n_cols, bool all_cols, hipStream_t st);
  int decode_step(const Tile& w, int n_eos, bool forced, float* const* out_logits, int n_cols, bool all_cols, hipStream_t st);
  // one tile: the arrays hold R host pointers / lengths; forced_ids, out_logits: null for every row, or one per row
  int generate_tile(int R, const int* const* prompts, const int* P, const int* max_new, const int* eos_ids, int n_eos, const int* const* forced_ids,
                    int* const* out_ids, int* n_out, float* const* out_logits, const int* logit_cols, int n_cols, bool all_cols, void* ws,
                    size_t ws_bytes, int use_graph, hipStream_t st);
  // prompt_ids, forced_ids, out_ids, out_logits: the rows concatenated.  A single-prompt call is B = 1.
  int generate_batch(int B, const int* prompt_ids, const int* n_prompt, const int* max_new, const int* eos_ids, int n_eos, const int* forced_ids,
                     int* out_ids, int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols, void* ws, size_t ws_bytes,
                     int use_graph, hipStream_t st);
};

}  // namespace idxtts
