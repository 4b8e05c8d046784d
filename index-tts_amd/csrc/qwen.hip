// Qwen3 causal LM (qwen.h), host side: loading, the workspace of a tile, the decode step's launch sequence, generation, the C API.
// A call of B prompts is served in consecutive tiles of R <= QWEN_BATCH_ROWS rows that share every weight pass of a step; a single-prompt
// call is a tile of one row.  Per tile: prefill on the exact-fp32 GEMM, row by row into the row's cache (not batched: a packed prefill
// would change the GEMM's M and is not claimed to keep a row equal to its own single call), then greedy decode steps of five launches
// per layer and a tail of three (qwen_kernels.hip).  Every per-step value lives in QwenState on the device, so one captured step
// replays for the whole generation.
//
// Step graphs (QwenStepGraphs): a captured step bakes in the tile's workspace layout, i.e. every row's prompt length and cap.  Tiles of
// real texts differ in these, so up to MAX_BATCH_GRAPHS steps are kept for tiles of several rows, one per key, and the one unused
// longest leaves; a tile whose lengths have not been seen pays one capture and instantiation.  One-row tiles keep one step of their own.
#include "qwen.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "model_util.h"

namespace idxtts {

namespace {

constexpr int HD = QWEN_HD, GMAX = QWEN_GMAX;

const char* const LAYER_KEYS[] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                  "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                                  "mlp.down_proj.weight", "input_layernorm.weight", "post_attention_layernorm.weight"};
const char* const INV_FREQ_KEY = "model.rotary_emb.inv_freq";

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
QwenModel::~QwenModel() {
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

bool QwenModel::accepts(const std::string& name) const {
  if (name == "model.embed_tokens.weight" || name == "model.norm.weight" || name == INV_FREQ_KEY) return true;
  if (name == "lm_head.weight") return true;      // a tied checkpoint may carry it too: it must then equal the embedding (finalize)
  const std::string pre = "model.layers.";
  if (name.compare(0, pre.size(), pre) != 0) return false;
  const size_t dot = name.find('.', pre.size());
  if (dot == std::string::npos || dot == pre.size()) return false;
  int li = 0;
  for (size_t i = pre.size(); i < dot; ++i) {
    if (name[i] < '0' || name[i] > '9' || li > 100000) return false;
    li = li * 10 + (name[i] - '0');
  }
  if (li >= cfg.num_hidden_layers) return false;
  const std::string rest = name.substr(dot + 1);
  for (const char* k : LAYER_KEYS)
    if (rest == k) return true;
  return false;
}

// bf16 storage takes only values on the bf16 grid: the first tensor with another one is named (no silent rounding)
static int check_bf16_grid(const std::string& key, const std::vector<float>& w) {
  for (size_t i = 0; i < w.size(); ++i) {
    unsigned bits;
    memcpy(&bits, &w[i], 4);
    if (bits & 0xffffu)
      IDX_FAIL("tensor '" + key + "' is not exactly representable in bf16 (element " + std::to_string(i) + "): load it with the fp32 weight format");
  }
  return 0;
}

// a linear weight [N][K] in the decode format (bf16: the upper halves of values already checked to be on the grid)
static int make_stream(DeviceArena& arena, const float* w, int N, int K, int fmt, QwenStream* out) {
  out->N = N; out->K = K;
  const size_t n = (size_t)N * K;
  void* d = nullptr;
  if (fmt == QWEN_W_BF16) {
    std::vector<unsigned short> h(n);
    for (size_t i = 0; i < n; ++i) {
      unsigned bits;
      memcpy(&bits, &w[i], 4);
      h[i] = (unsigned short)(bits >> 16);
    }
    if (arena.upload_bytes(h.data(), n * 2, &d)) return 1;
  } else {
    if (arena.upload_bytes(w, n * 4, &d)) return 1;
  }
  out->w = d;
  return 0;
}

// the staged linear weight `key` [N][K], checked for the format
static int linear_tensor(std::map<std::string, HostTensor>& t, const std::string& key, int N, int K, int fmt, HostTensor** out) {
  if (need(t, key, {N, K}, out)) return 1;
  return fmt == QWEN_W_BF16 ? check_bf16_grid(key, (*out)->data) : 0;
}

static int make_prefill_linear(DeviceArena& arena, const float* w, int N, int K, LinearWeights* out) {      // exact-fp32 pack only
  std::vector<float> packed(linear_packed_floats(N, K));
  pack_linear(packed.data(), w, N, K);
  if (up(arena, packed, &out->wp)) return 1;
  out->N = N; out->K = K;
  return 0;
}

int QwenModel::finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, L = cfg.num_hidden_layers, V = cfg.vocab_size;
  const int QD = qdim(), KD = kvdim();
  layers.resize(L);
  HostTensor* h = nullptr;
  for (int li = 0; li < L; ++li) {
    QwenLayer& Y = layers[li];
    const std::string p = "model.layers." + std::to_string(li) + ".";
    if (vec_from(t, arena, p + "input_layernorm.weight", H, &Y.in_g) || vec_from(t, arena, p + "post_attention_layernorm.weight", H, &Y.post_g) ||
        vec_from(t, arena, p + "self_attn.q_norm.weight", HD, &Y.qn_g) || vec_from(t, arena, p + "self_attn.k_norm.weight", HD, &Y.kn_g))
      return 1;
    HostTensor *q = nullptr, *k = nullptr, *v = nullptr, *g = nullptr, *u = nullptr;
    if (linear_tensor(t, p + "self_attn.q_proj.weight", QD, H, fmt, &q) || linear_tensor(t, p + "self_attn.k_proj.weight", KD, H, fmt, &k) ||
        linear_tensor(t, p + "self_attn.v_proj.weight", KD, H, fmt, &v))
      return 1;
    std::vector<float> cat;      // [q_proj; k_proj; v_proj]: one stream, one GEMM
    cat.reserve((size_t)(QD + 2 * KD) * H);
    cat.insert(cat.end(), q->data.begin(), q->data.end());
    cat.insert(cat.end(), k->data.begin(), k->data.end());
    cat.insert(cat.end(), v->data.begin(), v->data.end());
    if (make_stream(arena, cat.data(), QD + 2 * KD, H, fmt, &Y.qkv_s) || make_prefill_linear(arena, cat.data(), QD + 2 * KD, H, &Y.qkv_l)) return 1;
    if (linear_tensor(t, p + "self_attn.o_proj.weight", H, QD, fmt, &h)) return 1;
    if (make_stream(arena, h->data.data(), H, QD, fmt, &Y.o_s) || make_prefill_linear(arena, h->data.data(), H, QD, &Y.o_l)) return 1;
    if (linear_tensor(t, p + "mlp.gate_proj.weight", I, H, fmt, &g) || linear_tensor(t, p + "mlp.up_proj.weight", I, H, fmt, &u)) return 1;
    if (make_stream(arena, g->data.data(), I, H, fmt, &Y.gate_s) || make_stream(arena, u->data.data(), I, H, fmt, &Y.up_s)) return 1;
    cat.clear();      // [gate_proj; up_proj] for the prefill GEMM
    cat.insert(cat.end(), g->data.begin(), g->data.end());
    cat.insert(cat.end(), u->data.begin(), u->data.end());
    if (make_prefill_linear(arena, cat.data(), 2 * I, H, &Y.gu_l)) return 1;
    if (linear_tensor(t, p + "mlp.down_proj.weight", H, I, fmt, &h)) return 1;
    if (make_stream(arena, h->data.data(), H, I, fmt, &Y.down_s) || make_prefill_linear(arena, h->data.data(), H, I, &Y.down_l)) return 1;
    for (const char* k2 : LAYER_KEYS) t.erase(p + k2);      // staged copies of a 0.6 B model are 2.4 GB: give each layer's back at once
  }
  if (vec_from(t, arena, "model.norm.weight", H, &norm_g)) return 1;
  HostTensor* e = nullptr;
  if (linear_tensor(t, "model.embed_tokens.weight", V, H, fmt, &e)) return 1;
  if (make_stream(arena, e->data.data(), V, H, fmt, &embed_s)) return 1;
  auto lm = t.find("lm_head.weight");
  if (cfg.tie_word_embeddings) {
    if (lm != t.end()) IDX_CHECK(lm->second.shape == e->shape && lm->second.data == e->data, "tie_word_embeddings is set but lm_head.weight differs from model.embed_tokens.weight");
    head_s = embed_s;
  } else {
    if (linear_tensor(t, "lm_head.weight", V, H, fmt, &h)) return 1;
    if (make_stream(arena, h->data.data(), V, H, fmt, &head_s)) return 1;
  }
  // rotary table.  inv_freq: the checkpoint's buffer when it is given; else theta^(-2i/d) through the same fp32 steps the reference
  // takes (1 / theta ** (2i / d) on fp32 tensors).  angle = fp32(pos) * inv_freq in fp32, as the reference's fp32 outer product.
  std::vector<float> inv(HD / 2);
  auto fi = t.find(INV_FREQ_KEY);
  if (fi != t.end()) {
    IDX_CHECK(fi->second.numel() == HD / 2, "model.rotary_emb.inv_freq must have head_dim / 2 entries");
    inv = fi->second.data;
  } else {
    for (int i = 0; i < HD / 2; ++i) inv[i] = 1.0f / powf(cfg.rope_theta, (float)(2 * i) / (float)HD);
  }
  std::vector<float> tab((size_t)cfg.max_context * HD);
  for (int pos = 0; pos < cfg.max_context; ++pos)
    for (int i = 0; i < HD / 2; ++i) {
      const float ang = (float)pos * inv[i];
      tab[((size_t)pos * (HD / 2) + i) * 2] = (float)std::cos((double)ang);
      tab[((size_t)pos * (HD / 2) + i) * 2 + 1] = (float)std::sin((double)ang);
    }
  if (up(arena, tab, &rope)) return 1;
  return qwen_kernels_prepare();
}

// Every take starts 256-aligned, so the total does not depend on the order of the takes.  The time of a step does, a little: a row's
// id arrays sit behind its cache in a tile of several rows, and behind the step state in a tile of one row, where the other order
// measured 0.2 - 0.3 % more per token (profiles/README.md, "One host path").
QwenModel::Tile QwenModel::carve(void* ws, int R, const int* P, const int* max_new, int n_eos, int n_cols) const {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, L = cfg.num_hidden_layers, V = cfg.vocab_size;
  Tile b;
  memset(&b, 0, sizeof(b));
  Carver c(ws);
  b.R = R;
  const int Pmax = *std::max_element(P, P + R);
  b.x = c.take<float>((size_t)Pmax * H);
  b.x2 = c.take<float>((size_t)Pmax * H);
  b.xn = c.take<float>((size_t)Pmax * H);
  b.qkv = c.take<float>((size_t)Pmax * qkvdim());
  b.att = c.take<float>((size_t)Pmax * qdim());
  b.gu = c.take<float>((size_t)Pmax * 2 * I);
  b.hmid = c.take<float>((size_t)Pmax * I);
  for (int r = 0; r < R; ++r) {
    b.max_new[r] = max_new[r];
    b.Smax[r] = (P[r] + max_new[r] + 3) & ~3;
    b.nsplit[r] = qwen_nsplit_for(b.Smax[r]);
    b.max_nsplit = std::max(b.max_nsplit, b.nsplit[r]);
    b.max_cap = std::max(b.max_cap, cdiv(b.Smax[r], b.nsplit[r]));
    b.keys += b.Smax[r];
    const size_t kv = (size_t)L * cfg.num_key_value_heads * b.Smax[r] * HD;
    b.kc[r] = c.take<float>(kv);
    b.vc[r] = c.take<float>(kv);
    if (R > 1) {
      b.prompt[r] = c.take<int>(P[r]);
      b.forced[r] = c.take<int>(max_new[r]);
      b.out_ids[r] = c.take<int>(max_new[r]);
    }
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
  if (R > 1) b.rows = c.take<QwenBatchRow>(R);      // one row: its geometry goes into the launch arguments
  if (R == 1) b.prompt[0] = c.take<int>(P[0]);
  b.eos = c.take<int>(std::max(1, n_eos));
  if (R == 1) b.forced[0] = c.take<int>(max_new[0]);
  b.cols = c.take<int>(std::max(1, n_cols));
  if (R == 1) b.out_ids[0] = c.take<int>(max_new[0]);
  b.bytes = (c.off + 255) & ~(size_t)255;
  return b;
}

size_t QwenModel::workspace_bytes(int B, const int* P, const int* max_new, int n_eos, int n_cols) const {
  size_t need = 0;
  for (int t0 = 0; t0 < B; t0 += QWEN_BATCH_ROWS)
    need = std::max(need, carve(nullptr, std::min(QWEN_BATCH_ROWS, B - t0), P + t0, max_new + t0, n_eos, n_cols).bytes);
  return need;
}

int QwenModel::prefill(const Tile& w, int r, int P, hipStream_t st) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, V = cfg.vocab_size, QD = qdim(), QKV = qkvdim();
  const int Hq = cfg.num_attention_heads, Hkv = cfg.num_key_value_heads;
  if (qwen_embed_rows(w.x, w.prompt[r], embed_s.w, P, H, V, fmt, st)) return 1;
  const size_t per_layer = (size_t)Hkv * w.Smax[r] * HD;
  for (int li = 0; li < cfg.num_hidden_layers; ++li) {
    const QwenLayer& Y = layers[li];
    if (qwen_rmsnorm_rows(w.x, w.xn, Y.in_g, P, H, cfg.rms_norm_eps, st)) return 1;
    if (lin_exact(Y.qkv_l, w.xn, H, w.qkv, QKV, P, st)) return 1;
    QwenAttnArgs a;
    a.qkv = w.qkv; a.ld_qkv = QKV; a.qn_g = Y.qn_g; a.kn_g = Y.kn_g; a.eps = cfg.rms_norm_eps; a.rope = rope;
    a.kc = w.kc[r] + li * per_layer; a.vc = w.vc[r] + li * per_layer; a.Smax = w.Smax[r]; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv;
    a.out = w.att; a.ld_out = QD; a.st = nullptr; a.pos0 = 0; a.nsplit = 1; a.slice_cap = P; a.scale = 1.0f / sqrtf((float)HD);
    if (qwen_kv_store(a, P, st)) return 1;
    if (qwen_attn(a, P, false, (double)P * P, P, st)) return 1;
    if (lin_exact(Y.o_l, w.att, QD, w.x2, H, P, st, ACT_NONE, w.x, H)) return 1;
    if (qwen_rmsnorm_rows(w.x2, w.xn, Y.post_g, P, H, cfg.rms_norm_eps, st)) return 1;
    if (lin_exact(Y.gu_l, w.xn, H, w.gu, 2 * I, P, st)) return 1;
    if (qwen_silu_mul(w.gu, w.hmid, P, I, st)) return 1;
    if (lin_exact(Y.down_l, w.hmid, I, w.x, H, P, st, ACT_NONE, w.x2, H)) return 1;
  }
  IDX_HIP(hipMemcpyAsync(w.xd + (size_t)r * H, w.x + (size_t)(P - 1) * H, H * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

int QwenModel::head_tail(const Tile& w, int n_eos, bool forced, float* const* out_logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, V = cfg.vocab_size, R = w.R;
  QwenGemvArgs a;
  a.wa = head_s.w; a.K = H; a.units = V / 2; a.upw = QWEN_HEAD_UPW; a.x = w.xd; a.g = norm_g; a.eps = cfg.rms_norm_eps; a.y = w.logits;
  a.part_val = w.head_val; a.part_idx = w.head_idx; a.cnt = w.head_cnt; a.st = w.st;
  a.R = R; a.ldy = V; a.part_stride = w.head_blocks;
  IDX_CHECK(qwen_gemv_blocks(a) == w.head_blocks, "head partial buffers");
  if (qwen_gemv(EPI_HEAD, a, fmt, V, st)) return 1;
  if (out_logits && qwen_logits(w.st, w.logits, V, all_cols ? nullptr : w.cols, n_cols, R, w.max_new[0], out_logits[0], w.rows, st)) return 1;
  QwenTailArgs t;
  memset(&t, 0, sizeof(t));
  t.st = w.st; t.eos = w.eos; t.n_eos = n_eos; t.emb = embed_s.w; t.H = H; t.V = V; t.xd = w.xd;
  t.rows = w.rows; t.use_forced = forced ? 1 : 0;
  if (!w.rows) { t.out_ids = w.out_ids[0]; t.forced = forced ? w.forced[0] : nullptr; t.max_new = w.max_new[0]; }
  return qwen_tail(t, R, fmt, st);
}

int QwenModel::decode_step(const Tile& w, int n_eos, bool forced, float* const* out_logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, QD = qdim(), QKV = qkvdim(), R = w.R;
  const int Hq = cfg.num_attention_heads, Hkv = cfg.num_key_value_heads;
  for (int li = 0; li < cfg.num_hidden_layers; ++li) {
    const QwenLayer& Y = layers[li];
    QwenGemvArgs q;      // qkv = [q_proj; k_proj; v_proj] RMSNorm(x)
    q.wa = Y.qkv_s.w; q.K = H; q.units = QKV / 2; q.x = w.xd; q.g = Y.in_g; q.eps = cfg.rms_norm_eps; q.y = w.qkvd; q.R = R; q.ldy = QKV;
    if (qwen_gemv(EPI_STORE, q, fmt, QKV, st)) return 1;
    QwenAttnArgs a;      // the grid and the score buffer cover the largest row; one row: that row's geometry, baked in
    a.qkv = w.qkvd; a.ld_qkv = QKV; a.qn_g = Y.qn_g; a.kn_g = Y.kn_g; a.eps = cfg.rms_norm_eps; a.rope = rope;
    a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.out = w.attd; a.ld_out = QD; a.st = w.st; a.nsplit = w.max_nsplit; a.slice_cap = w.max_cap;
    a.part = w.attn_part; a.cnt = w.attn_cnt; a.scale = 1.0f / sqrtf((float)HD);
    a.rows = w.rows; a.layer = li; a.part_stride = w.part_stride;
    if (!w.rows) {
      const size_t off = (size_t)li * Hkv * w.Smax[0] * HD;
      a.kc = w.kc[0] + off; a.vc = w.vc[0] + off; a.Smax = w.Smax[0];
    }
    if (qwen_attn(a, R, true, w.keys, w.keys, st)) return 1;
    QwenGemvArgs o;      // x += o_proj(att)
    o.wa = Y.o_s.w; o.K = QD; o.units = H; o.x = w.attd; o.y = w.xd; o.R = R; o.ldy = H;
    if (qwen_gemv(EPI_RES, o, fmt, H, st)) return 1;
    QwenGemvArgs g;      // h = silu(gate_proj(n)) * up_proj(n), n = RMSNorm(x)
    g.wa = Y.gate_s.w; g.wb = Y.up_s.w; g.K = H; g.units = I; g.x = w.xd; g.g = Y.post_g; g.eps = cfg.rms_norm_eps; g.y = w.hd; g.R = R; g.ldy = I;
    if (qwen_gemv(EPI_SWIGLU, g, fmt, 2 * I, st)) return 1;
    QwenGemvArgs d;      // x += down_proj(h)
    d.wa = Y.down_s.w; d.K = I; d.units = H; d.x = w.hd; d.y = w.xd; d.R = R; d.ldy = H;
    if (qwen_gemv(EPI_RES, d, fmt, H, st)) return 1;
  }
  return head_tail(w, n_eos, forced, out_logits, n_cols, all_cols, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
void QwenStepGraphs::destroy(Entry& e) {
  if (e.exec) (void)hipGraphExecDestroy(e.exec);
  if (e.graph) (void)hipGraphDestroy(e.graph);
  e.exec = nullptr; e.graph = nullptr;
}

void QwenStepGraphs::clear() {
  for (Entry& e : kept_) destroy(e);
  kept_.clear();
}

int QwenStepGraphs::get(const Key& key, hipStream_t st, const std::function<int()>& step, hipGraphExec_t* exec, bool* captured) {
  *captured = false;
  const auto hit = std::find_if(kept_.begin(), kept_.end(), [&](const Entry& e) { return e.key == key; });
  if (hit != kept_.end()) {
    std::rotate(hit, hit + 1, kept_.end());      // the latest used last
    *exec = kept_.back().exec;
    return 0;
  }
  if ((int)kept_.size() >= cap_) {
    destroy(kept_.front());
    kept_.erase(kept_.begin());
  }
  // one step runs eagerly (a first launch may load code objects, which a capture refuses), then one step is captured
  if (step()) return 1;
  *captured = true;
  Entry g;
  g.key = key;
  IDX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = step();
  const hipError_t e = hipStreamEndCapture(st, &g.graph);
  if (rc || e != hipSuccess) destroy(g);
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
  if (en != hipSuccess || !kernels_only) destroy(g);
  IDX_HIP(en);
  IDX_CHECK(kernels_only, "the captured decode step holds a node that is not a kernel launch");
  kernel_nodes_ = (int)n_nodes;
  kept_.push_back(g);
  *exec = g.exec;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
int QwenModel::generate_tile(int R, const int* const* prompts, const int* P, const int* max_new, const int* eos_ids, int n_eos,
                             const int* const* forced_ids, int* const* out_ids, int* n_out, float* const* out_logits, const int* logit_cols,
                             int n_cols, bool all_cols, void* ws, size_t ws_bytes, int use_graph, hipStream_t st) {
  const bool forced = forced_ids != nullptr;
  const Tile w = carve(ws, R, P, max_new, n_eos, n_cols);
  IDX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small");
  QwenBatchRow rows[QWEN_BATCH_ROWS];
  QwenState s0[QWEN_BATCH_ROWS];
  memset(rows, 0, sizeof(rows));
  memset(s0, 0, sizeof(s0));
  int Nmax = 0;
  for (int r = 0; r < R; ++r) {
    rows[r].kc = w.kc[r]; rows[r].vc = w.vc[r]; rows[r].Smax = w.Smax[r]; rows[r].nsplit = w.nsplit[r]; rows[r].max_new = max_new[r];
    rows[r].out_ids = w.out_ids[r]; rows[r].forced = w.forced[r]; rows[r].out_logits = out_logits ? out_logits[r] : nullptr;
    s0[r].pos = P[r] - 1;      // the tail of the prefill's head step moves it to P, the first generated token's position
    Nmax = std::max(Nmax, max_new[r]);
    IDX_HIP(hipMemcpyAsync(w.prompt[r], prompts[r], P[r] * sizeof(int), hipMemcpyHostToDevice, st));
    if (forced) IDX_HIP(hipMemcpyAsync(w.forced[r], forced_ids[r], max_new[r] * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipMemsetAsync(w.out_ids[r], 0, max_new[r] * sizeof(int), st));
  }
  if (w.rows) IDX_HIP(hipMemcpyAsync(w.rows, rows, R * sizeof(QwenBatchRow), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.st, s0, R * sizeof(QwenState), hipMemcpyHostToDevice, st));
  if (n_eos) IDX_HIP(hipMemcpyAsync(w.eos, eos_ids, n_eos * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_cols && !all_cols) IDX_HIP(hipMemcpyAsync(w.cols, logit_cols, n_cols * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.head_cnt, 0, sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.attn_cnt, 0, (size_t)R * cfg.num_key_value_heads * sizeof(unsigned), st));
  IDX_HIP(hipStreamSynchronize(st));      // the host arrays above are the caller's, or this frame's

  for (int r = 0; r < R; ++r)      // row by row, into the row's cache
    if (prefill(w, r, P[r], st)) return 1;
  const auto step = [&]() { return decode_step(w, n_eos, forced, out_logits, n_cols, all_cols, st); };
  if (head_tail(w, n_eos, forced, out_logits, n_cols, all_cols, st)) return 1;

  hipGraphExec_t exec = nullptr;
  int n_first = 1;
  if (use_graph && !prof_enabled() && Nmax > 2) {
    QwenStepGraphs::Key key;
    key.ws = ws; key.ws_bytes = ws_bytes; key.R = R; std::copy(P, P + R, key.P.begin()); std::copy(max_new, max_new + R, key.max_new.begin());
    key.n_eos = n_eos; key.n_cols = n_cols; key.forced = forced; key.all_cols = all_cols;
    key.out_logits = out_logits && R == 1 ? out_logits[0] : nullptr;
    bool captured = false;
    const int rc = (R == 1 ? graphs1 : graphs).get(key, st, std::cref(step), &exec, &captured);
    if (captured) n_first = 2;
    if (rc) return 1;
  }
  QwenState hs[QWEN_BATCH_ROWS];
  for (int n = n_first; n < Nmax; ++n) {
    if (exec) IDX_HIP(hipGraphLaunch(exec, st));
    else if (step()) return 1;
    if ((n + 1) % 8 == 0 && n + 1 < Nmax) {      // look every 8 steps: when every row is done, later launches change nothing
      IDX_HIP(hipMemcpyAsync(hs, w.st, R * sizeof(QwenState), hipMemcpyDeviceToHost, st));
      IDX_HIP(hipStreamSynchronize(st));
      if (std::all_of(hs, hs + R, [](const QwenState& s) { return s.done != 0; })) break;
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
  IDX_CHECK(ws && ws_bytes >= workspace_bytes(B, n_prompt, max_new, n_eos, n_cols), "workspace too small");
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
    if (generate_tile(R, prompts, n_prompt + t0, max_new + t0, eos_ids, n_eos, forced_ids ? forced : nullptr, outs, n_out + t0,
                      out_logits ? lg : nullptr, logit_cols, n_cols, all_cols, ws, ws_bytes, use_graph, st))
      return 1;
  }
  return 0;
}

}  // namespace idxtts

using namespace idxtts;

extern "C" {

int idxtts_qwen_create(const idxtts_qwen_config* cfg, idxtts_ctx** out) {
  try {
    IDX_CHECK(cfg && out, "null pointer");
    const idxtts_qwen_config& c = *cfg;
    if (c.head_dim != HD) IDX_FAIL("head_dim " + std::to_string(c.head_dim) + " is not supported: the Qwen3 kernels are built for head_dim 128 only");
    IDX_CHECK(c.vocab_size >= 2 && c.vocab_size % 2 == 0, "vocab_size must be even");
    IDX_CHECK(c.hidden_size >= 8 && c.hidden_size % 8 == 0 && c.hidden_size <= 3072, "hidden_size: a multiple of 8, at most 3072");
    IDX_CHECK(c.intermediate_size >= 8 && c.intermediate_size % 8 == 0 && c.intermediate_size <= 3072, "intermediate_size: a multiple of 8, at most 3072");
    IDX_CHECK(c.num_hidden_layers > 0 && c.num_attention_heads > 0 && c.num_key_value_heads > 0, "layers / heads");
    IDX_CHECK(c.num_attention_heads % c.num_key_value_heads == 0 && c.num_attention_heads / c.num_key_value_heads <= GMAX, "1..4 query heads per kv head");
    IDX_CHECK(c.num_attention_heads * HD <= 3072, "num_attention_heads * head_dim: at most 3072");
    IDX_CHECK(c.rms_norm_eps > 0.0f && c.rope_theta > 0.0f, "rms_norm_eps / rope_theta");
    IDX_CHECK(c.max_context >= 8 && (size_t)(c.num_attention_heads / c.num_key_value_heads) * c.max_context * sizeof(float) <= 40 * 1024, "max_context (the prefill attention keeps a query's scores in LDS: query heads per kv head * max_context <= 10240)");
    std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
    ctx->model.reset(new QwenModel(c));
    *out = ctx.release();
    return 0;
  } catch (const std::exception& e) { return fail(__FILE__, __LINE__, std::string("exception: ") + e.what()); }
}

int idxtts_qwen_set_weight_format(idxtts_ctx* ctx, int format) {
  IDX_CHECK(ctx, "null ctx");
  auto* m = dynamic_cast<QwenModel*>(ctx->model.get());
  IDX_CHECK(m, "not a Qwen context");
  IDX_CHECK(!ctx->finalized, "the weight format is chosen before finalize");
  IDX_CHECK(format == QWEN_W_F32 || format == QWEN_W_BF16, "weight format: 0 fp32, 1 bf16");
  m->fmt = format;
  return 0;
}

size_t idxtts_qwen_batch_workspace_bytes(const idxtts_ctx* ctx, int B, const int* n_prompt, const int* max_new_tokens, int n_eos, int n_logit_cols) {
  if (!ctx || B < 1 || !n_prompt || !max_new_tokens || n_eos < 0 || n_logit_cols < 0) return 0;
  for (int b = 0; b < B; ++b)
    if (n_prompt[b] <= 0 || max_new_tokens[b] <= 0) return 0;
  auto* m = dynamic_cast<const QwenModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, n_prompt, max_new_tokens, n_eos, n_logit_cols) : 0;
}

size_t idxtts_qwen_workspace_bytes(const idxtts_ctx* ctx, int n_prompt, int max_new_tokens, int n_eos, int n_logit_cols) {
  return idxtts_qwen_batch_workspace_bytes(ctx, 1, &n_prompt, &max_new_tokens, n_eos, n_logit_cols);
}

int idxtts_qwen_max_batch(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  return dynamic_cast<const QwenModel*>(ctx->model.get()) ? QWEN_BATCH_ROWS : -1;
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

// a single-prompt call is a batch of one row
int idxtts_qwen_generate(idxtts_ctx* ctx, const int* prompt_ids, int n_prompt, int max_new_tokens, const int* eos_ids, int n_eos,
                         const int* forced_ids, int* out_ids, int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols,
                         void* workspace, size_t bytes, int use_graph, void* stream) {
  return idxtts_qwen_generate_batch(ctx, 1, prompt_ids, &n_prompt, &max_new_tokens, eos_ids, n_eos, forced_ids, out_ids, n_out, out_logits,
                                    logit_cols, n_logit_cols, workspace, bytes, use_graph, stream);
}

static int kept_launches(const idxtts_ctx* ctx, QwenStepGraphs QwenModel::*which) {
  auto* m = ctx ? dynamic_cast<const QwenModel*>(ctx->model.get()) : nullptr;
  return m ? (m->*which).launches() : -1;
}
int idxtts_qwen_step_graph_launches(const idxtts_ctx* ctx) { return kept_launches(ctx, &QwenModel::graphs1); }
int idxtts_qwen_batch_step_graph_launches(const idxtts_ctx* ctx) { return kept_launches(ctx, &QwenModel::graphs); }

}  // extern "C"
