// Qwen3 causal LM at B = 1 (qwen.h): prefill on the exact-fp32 GEMM, then a greedy decode step of five launches per layer --
//   qkv GEMV (input RMSNorm in its prologue) | q/k RMSNorm + rotary + KV append + grouped-query attention (keys split over
//   workgroups, merged by the last to arrive) | o_proj GEMV + residual | gate/up GEMV (post-attention RMSNorm in its prologue,
//   silu(g) * u in its epilogue) | down_proj GEMV + residual
// -- and a tail of final norm + head GEMV with a two-stage argmax, the optional logits hand-over, and the next token's embedding row.
// Every per-step value lives in QwenState on the device, so one captured step replays for the whole generation.
//
// The RMSNorm gain is applied to the activation vector in the GEMV's prologue ((x * rsqrt(mean x^2 + eps)) * g, the reference's order of
// operations), not folded into the weights: W diag(g) would leave the bf16 grid, and bf16 storage here holds the checkpoint's weights
// exactly.  Each workgroup redoes the norm of the <= 3072-element vector it multiplies with (L2-resident, a few hundred FMAs a thread).
//
// The GEMVs are plain weight streams: a wave owns whole rows, a lane the same 8 consecutive k of every 512-k chunk (two 16-byte loads
// of fp32, one of bf16), all loads of a row pair issued before the first FMA, no branch among them (addresses past K are clamped and
// meet zeros of x), then a shuffle butterfly.  The k -> lane map and the order of the FMAs do not depend on the storage format or on how the step is
// launched: bf16 and fp32 storage of the same values, and eager launches and graph replay, agree bit for bit.
#include "qwen.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "device_util.h"
#include "model_util.h"

namespace idxtts {

namespace {

constexpr int HD = QWEN_HD, GMAX = QWEN_GMAX;      // the shared device code and its argument structs: qwen.h

// ---------------------------------------------------------------------------------------------------------------------------
template <int NCH, int EPI, typename WT>
__global__ __launch_bounds__(256) void qwen_gemv_kernel(const QwenGemvArgs p) {
  __shared__ float xs[NCH * 512];
  qwen_gemv_body<NCH, EPI, WT, 1>(p, xs, 1, 0, 0);
}

template <int EPI, typename WT>
int gemv_launch_fmt(const QwenGemvArgs& a, int blocks, hipStream_t st) {
  const int nch = cdiv(a.K, 512);
  if (nch <= 1) hipLaunchKernelGGL((qwen_gemv_kernel<1, EPI, WT>), dim3(blocks), dim3(256), 0, st, a);
  else if (nch <= 2) hipLaunchKernelGGL((qwen_gemv_kernel<2, EPI, WT>), dim3(blocks), dim3(256), 0, st, a);
  else if (nch <= 4) hipLaunchKernelGGL((qwen_gemv_kernel<4, EPI, WT>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((qwen_gemv_kernel<6, EPI, WT>), dim3(blocks), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

int gemv_blocks(const QwenGemvArgs& a) { return cdiv(a.units, 4 * a.upw); }

template <int EPI>
int qwen_gemv(const QwenGemvArgs& a, int fmt, int rows, hipStream_t st) {
  IDX_CHECK(a.K >= 8 && a.K % 8 == 0 && a.K <= 3072, "GEMV K must be a multiple of 8, at most 3072");
  IDX_CHECK(a.units > 0 && a.upw > 0, "GEMV shape");
  static const int cat = prof_register("qwen_gemv_kernel");
  ProfScope prof(cat, st, 2.0 * rows * a.K, (double)rows * a.K * (fmt == QWEN_W_BF16 ? 2 : 4));
  const int blocks = gemv_blocks(a);
  return fmt == QWEN_W_BF16 ? gemv_launch_fmt<EPI, unsigned short>(a, blocks, st) : gemv_launch_fmt<EPI, float>(a, blocks, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per (kv head, key piece, query): qwen_attn_body (qwen.h)
template <bool APPEND>
__global__ __launch_bounds__(256) void qwen_attn_kernel(const QwenAttnArgs p) {
  const int r = blockIdx.z;
  qwen_attn_body<APPEND>(p, blockIdx.x, blockIdx.y, r, p.st ? p.st->pos : p.pos0 + r);
}

int qwen_attn(const QwenAttnArgs& a, int rows, bool append, int keys_hint, hipStream_t st) {
  IDX_CHECK(a.G >= 1 && a.G <= GMAX && a.Hq == a.Hkv * a.G, "query heads per kv head: 1..4");
  IDX_CHECK(a.nsplit >= 1 && a.slice_cap >= 1 && (a.nsplit == 1 || (a.part && a.cnt && rows == 1)), "key split");
  const size_t lds = (size_t)a.G * a.slice_cap * sizeof(float);
  IDX_CHECK(lds <= 40 * 1024, "context too long for the attention kernel's score buffer");
  static const int cat = prof_register("qwen_attn_kernel");
  ProfScope prof(cat, st, 4.0 * rows * a.Hq * (double)keys_hint * HD, 8.0 * a.Hkv * (double)keys_hint * HD);
  const dim3 grid(a.Hkv, a.nsplit, rows);
  if (append) hipLaunchKernelGGL(qwen_attn_kernel<true>, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(qwen_attn_kernel<false>, grid, dim3(256), lds, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The step's last launch (one workgroup): qwen_tail_row (qwen.h)
template <typename WT>
__global__ __launch_bounds__(256) void qwen_tail_kernel(const QwenTailArgs p) { qwen_tail_row<WT>(p); }

// out_logits[step][c] = logits[cols[c]] (cols null: column c) of a live step
__global__ __launch_bounds__(256) void qwen_logits_kernel(const QwenState* st, const float* logits, const int* cols, int n_cols, int max_new, float* out) {
  qwen_logits_row(st, logits, cols, n_cols, max_new, out, blockIdx.x * 256 + threadIdx.x);
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

int nsplit_for(int Smax) { return qwen_nsplit_for(Smax); }

const char* const LAYER_KEYS[] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                  "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                                  "mlp.down_proj.weight", "input_layernorm.weight", "post_attention_layernorm.weight"};
const char* const INV_FREQ_KEY = "model.rotary_emb.inv_freq";

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
QwenModel::~QwenModel() {
  drop_graph();
  drop_batch_graph();
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

void QwenModel::drop_graph() {
  if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
  if (graph) (void)hipGraphDestroy(graph);
  graph_exec = nullptr; graph = nullptr;
  graph_key = GraphKey();
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
  return batch_prepare();
}

QwenModel::Buffers QwenModel::carve(void* ws, int P, int max_new, int n_eos, int n_cols) const {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, L = cfg.num_hidden_layers, V = cfg.vocab_size;
  Buffers b;
  Carver c(ws);
  b.Smax = (P + max_new + 3) & ~3;
  b.x = c.take<float>((size_t)P * H);
  b.x2 = c.take<float>((size_t)P * H);
  b.xn = c.take<float>((size_t)P * H);
  b.qkv = c.take<float>((size_t)P * qkvdim());
  b.att = c.take<float>((size_t)P * qdim());
  b.gu = c.take<float>((size_t)P * 2 * I);
  b.hmid = c.take<float>((size_t)P * I);
  const size_t kv = (size_t)L * cfg.num_key_value_heads * b.Smax * HD;
  b.kc = c.take<float>(kv);
  b.vc = c.take<float>(kv);
  b.xd = c.take<float>(H);
  b.qkvd = c.take<float>(qkvdim());
  b.attd = c.take<float>(qdim());
  b.hd = c.take<float>(I);
  b.logits = c.take<float>(V);
  b.head_blocks = cdiv(V / 2, 4 * QWEN_HEAD_UPW);
  b.head_val = c.take<float>(b.head_blocks);
  b.head_idx = c.take<int>(b.head_blocks);
  b.head_cnt = c.take<unsigned>(1);
  b.nsplit = nsplit_for(b.Smax);
  b.attn_part = c.take<float>((size_t)cfg.num_attention_heads * b.nsplit * 130);
  b.attn_cnt = c.take<unsigned>(cfg.num_key_value_heads);
  b.st = c.take<QwenState>(1);
  b.prompt = c.take<int>(P);
  b.eos = c.take<int>(std::max(1, n_eos));
  b.forced = c.take<int>(max_new);
  b.cols = c.take<int>(std::max(1, n_cols));
  b.out_ids = c.take<int>(max_new);
  b.bytes = (c.off + 255) & ~(size_t)255;
  return b;
}

int QwenModel::prefill(const Buffers& w, int P, hipStream_t st) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, V = cfg.vocab_size, QD = qdim(), KD = kvdim(), QKV = qkvdim();
  const int Hq = cfg.num_attention_heads, Hkv = cfg.num_key_value_heads;
  static const int cat = prof_register("qwen_prefill_rows");
  if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_embed_rows_kernel<unsigned short>, dim3(P), dim3(256), 0, st, w.x, w.prompt, embed_s.w, H, V);
  else hipLaunchKernelGGL(qwen_embed_rows_kernel<float>, dim3(P), dim3(256), 0, st, w.x, w.prompt, embed_s.w, H, V);
  IDX_LAUNCH_CHECK();
  const size_t per_layer = (size_t)Hkv * w.Smax * HD;
  for (int li = 0; li < cfg.num_hidden_layers; ++li) {
    const QwenLayer& Y = layers[li];
    float* kc = w.kc + li * per_layer;
    float* vc = w.vc + li * per_layer;
    {
      ProfScope prof(cat, st, 0.0, 8.0 * P * H);
      hipLaunchKernelGGL(qwen_rmsnorm_rows_kernel, dim3(P), dim3(256), 0, st, w.x, w.xn, Y.in_g, H, cfg.rms_norm_eps);
      IDX_LAUNCH_CHECK();
    }
    if (lin_exact(Y.qkv_l, w.xn, H, w.qkv, QKV, P, st)) return 1;
    {
      ProfScope prof(cat, st, 0.0, 16.0 * P * KD);
      hipLaunchKernelGGL(qwen_kv_store_kernel, dim3(P, Hkv), dim3(64), 0, st, w.qkv, QKV, Y.kn_g, cfg.rms_norm_eps, rope, kc, vc, w.Smax, QD, KD);
      IDX_LAUNCH_CHECK();
    }
    QwenAttnArgs a;
    a.qkv = w.qkv; a.ld_qkv = QKV; a.qn_g = Y.qn_g; a.kn_g = Y.kn_g; a.eps = cfg.rms_norm_eps; a.rope = rope;
    a.kc = kc; a.vc = vc; a.Smax = w.Smax; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.out = w.att; a.ld_out = QD;
    a.st = nullptr; a.pos0 = 0; a.nsplit = 1; a.slice_cap = P; a.scale = 1.0f / sqrtf((float)HD);
    if (qwen_attn(a, P, false, P, st)) return 1;
    if (lin_exact(Y.o_l, w.att, QD, w.x2, H, P, st, ACT_NONE, w.x, H)) return 1;
    {
      ProfScope prof(cat, st, 0.0, 8.0 * P * H);
      hipLaunchKernelGGL(qwen_rmsnorm_rows_kernel, dim3(P), dim3(256), 0, st, w.x2, w.xn, Y.post_g, H, cfg.rms_norm_eps);
      IDX_LAUNCH_CHECK();
    }
    if (lin_exact(Y.gu_l, w.xn, H, w.gu, 2 * I, P, st)) return 1;
    {
      ProfScope prof(cat, st, 0.0, 12.0 * P * I);
      hipLaunchKernelGGL(qwen_silu_mul_kernel, dim3(P), dim3(256), 0, st, w.gu, w.hmid, I);
      IDX_LAUNCH_CHECK();
    }
    if (lin_exact(Y.down_l, w.hmid, I, w.x, H, P, st, ACT_NONE, w.x2, H)) return 1;
  }
  return 0;
}

int QwenModel::head_tail(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, V = cfg.vocab_size;
  QwenGemvArgs a;
  a.wa = head_s.w; a.K = H; a.units = V / 2; a.upw = QWEN_HEAD_UPW; a.x = w.xd; a.g = norm_g; a.eps = cfg.rms_norm_eps; a.y = w.logits;
  a.part_val = w.head_val; a.part_idx = w.head_idx; a.cnt = w.head_cnt; a.st = w.st;
  IDX_CHECK(gemv_blocks(a) == w.head_blocks, "head partial buffers");
  if (qwen_gemv<EPI_HEAD>(a, fmt, V, st)) return 1;
  if (out_logits) {
    static const int cat = prof_register("qwen_logits_kernel");
    ProfScope prof(cat, st, 0.0, 8.0 * n_cols);
    hipLaunchKernelGGL(qwen_logits_kernel, dim3(cdiv(n_cols, 256)), dim3(256), 0, st, w.st, w.logits, all_cols ? nullptr : w.cols, n_cols, max_new, out_logits);
    IDX_LAUNCH_CHECK();
  }
  QwenTailArgs t;
  t.st = w.st; t.out_ids = w.out_ids; t.forced = forced ? w.forced : nullptr; t.eos = w.eos; t.n_eos = n_eos; t.max_new = max_new;
  t.emb = embed_s.w; t.H = H; t.V = V; t.xd = w.xd;
  static const int cat = prof_register("qwen_tail_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * H);
  if (fmt == QWEN_W_BF16) hipLaunchKernelGGL(qwen_tail_kernel<unsigned short>, dim3(1), dim3(256), 0, st, t);
  else hipLaunchKernelGGL(qwen_tail_kernel<float>, dim3(1), dim3(256), 0, st, t);
  IDX_LAUNCH_CHECK();
  return 0;
}

int QwenModel::decode_step(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st) {
  const int H = cfg.hidden_size, I = cfg.intermediate_size, QD = qdim(), QKV = qkvdim();
  const int Hq = cfg.num_attention_heads, Hkv = cfg.num_key_value_heads;
  const size_t per_layer = (size_t)Hkv * w.Smax * HD;
  for (int li = 0; li < cfg.num_hidden_layers; ++li) {
    const QwenLayer& Y = layers[li];
    QwenGemvArgs q;      // qkv = [q_proj; k_proj; v_proj] RMSNorm(x)
    q.wa = Y.qkv_s.w; q.K = H; q.units = QKV / 2; q.x = w.xd; q.g = Y.in_g; q.eps = cfg.rms_norm_eps; q.y = w.qkvd;
    if (qwen_gemv<EPI_STORE>(q, fmt, QKV, st)) return 1;
    QwenAttnArgs a;
    a.qkv = w.qkvd; a.ld_qkv = QKV; a.qn_g = Y.qn_g; a.kn_g = Y.kn_g; a.eps = cfg.rms_norm_eps; a.rope = rope;
    a.kc = w.kc + li * per_layer; a.vc = w.vc + li * per_layer; a.Smax = w.Smax; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv;
    a.out = w.attd; a.ld_out = QD; a.st = w.st; a.nsplit = w.nsplit; a.slice_cap = cdiv(w.Smax, w.nsplit);
    a.part = w.attn_part; a.cnt = w.attn_cnt; a.scale = 1.0f / sqrtf((float)HD);
    if (qwen_attn(a, 1, true, w.Smax, st)) return 1;
    QwenGemvArgs o;      // x += o_proj(att)
    o.wa = Y.o_s.w; o.K = QD; o.units = H; o.x = w.attd; o.y = w.xd;
    if (qwen_gemv<EPI_RES>(o, fmt, H, st)) return 1;
    QwenGemvArgs g;      // h = silu(gate_proj(n)) * up_proj(n), n = RMSNorm(x)
    g.wa = Y.gate_s.w; g.wb = Y.up_s.w; g.K = H; g.units = I; g.x = w.xd; g.g = Y.post_g; g.eps = cfg.rms_norm_eps; g.y = w.hd;
    if (qwen_gemv<EPI_SWIGLU>(g, fmt, 2 * I, st)) return 1;
    QwenGemvArgs d;      // x += down_proj(h)
    d.wa = Y.down_s.w; d.K = I; d.units = H; d.x = w.hd; d.y = w.xd;
    if (qwen_gemv<EPI_RES>(d, fmt, H, st)) return 1;
  }
  return head_tail(w, max_new, n_eos, forced, out_logits, n_cols, all_cols, st);
}

int QwenModel::generate(const int* prompt_ids, int P, int max_new, const int* eos_ids, int n_eos, const int* forced_ids, int* out_ids, int* n_out,
                        float* out_logits, const int* logit_cols, int n_logit_cols, void* ws, size_t ws_bytes, int use_graph, hipStream_t user) {
  IDX_CHECK(prompt_ids && out_ids && n_out, "null pointer");
  IDX_CHECK(P > 0 && max_new > 0 && n_eos >= 0 && (n_eos == 0 || eos_ids), "shape");
  const int V = cfg.vocab_size;
  const bool all_cols = out_logits && !logit_cols;
  const int n_cols = out_logits ? (all_cols ? V : n_logit_cols) : 0;
  IDX_CHECK(!out_logits || n_cols > 0, "n_logit_cols");
  for (int i = 0; i < P; ++i) IDX_CHECK(prompt_ids[i] >= 0 && prompt_ids[i] < V, "prompt id outside the vocabulary");
  for (int i = 0; forced_ids && i < max_new; ++i) IDX_CHECK(forced_ids[i] >= 0 && forced_ids[i] < V, "forced id outside the vocabulary");
  for (int i = 0; i < n_cols && !all_cols; ++i) IDX_CHECK(logit_cols[i] >= 0 && logit_cols[i] < V, "logit column outside the vocabulary");
  IDX_CHECK(((P + max_new + 3) & ~3) <= cfg.max_context, "prompt + max_new_tokens exceeds the context the model was created for");
  IDX_CHECK(ws && ws_bytes >= workspace_bytes(P, max_new, n_eos, n_cols), "workspace too small");
  hipStream_t st = user;
  if (!user) {      // the legacy default stream cannot be captured: run on a private stream, after what the caller has queued
    if (!own_stream) IDX_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    IDX_HIP(hipStreamSynchronize(user));
    st = own_stream;
  }
  const Buffers w = carve(ws, P, max_new, n_eos, n_cols);
  IDX_HIP(hipMemcpyAsync(w.prompt, prompt_ids, P * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_eos) IDX_HIP(hipMemcpyAsync(w.eos, eos_ids, n_eos * sizeof(int), hipMemcpyHostToDevice, st));
  if (forced_ids) IDX_HIP(hipMemcpyAsync(w.forced, forced_ids, max_new * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_cols && !all_cols) IDX_HIP(hipMemcpyAsync(w.cols, logit_cols, n_cols * sizeof(int), hipMemcpyHostToDevice, st));
  QwenState s0;
  memset(&s0, 0, sizeof(s0));
  s0.pos = P - 1;      // the tail of the prefill's head step moves it to P, the first generated token's position
  IDX_HIP(hipMemcpyAsync(w.st, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.head_cnt, 0, sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.attn_cnt, 0, cfg.num_key_value_heads * sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.out_ids, 0, max_new * sizeof(int), st));
  IDX_HIP(hipStreamSynchronize(st));      // the host arrays above are the caller's

  if (prefill(w, P, st)) return 1;
  IDX_HIP(hipMemcpyAsync(w.xd, w.x + (size_t)(P - 1) * cfg.hidden_size, cfg.hidden_size * sizeof(float), hipMemcpyDeviceToDevice, st));
  const bool forced = forced_ids != nullptr;
  if (head_tail(w, max_new, n_eos, forced, out_logits, n_cols, all_cols, st)) return 1;

  const bool graph_ok = use_graph && !prof_enabled() && max_new > 2;
  hipGraphExec_t exec = nullptr;
  int n_first = 1;
  if (graph_ok) {
    GraphKey key;
    key.ws = ws; key.ws_bytes = ws_bytes; key.P = P; key.max_new = max_new; key.n_eos = n_eos; key.n_cols = n_cols; key.forced = forced;
    key.all_cols = all_cols; key.out_logits = out_logits;
    if (graph_exec && graph_key == key) {
      exec = graph_exec;
    } else {
      drop_graph();
      // step 1 runs eagerly (a first launch may load code objects, which a capture refuses), then one step is captured
      if (decode_step(w, max_new, n_eos, forced, out_logits, n_cols, all_cols, st)) return 1;
      n_first = 2;
      IDX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const int rc = decode_step(w, max_new, n_eos, forced, out_logits, n_cols, all_cols, st);
      const hipError_t e = hipStreamEndCapture(st, &graph);
      if (rc) { drop_graph(); return 1; }
      IDX_HIP(e);
      IDX_HIP(hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
      size_t n_nodes = 0;
      IDX_HIP(hipGraphGetNodes(graph, nullptr, &n_nodes));
      std::vector<hipGraphNode_t> nodes(n_nodes);
      if (n_nodes) IDX_HIP(hipGraphGetNodes(graph, nodes.data(), &n_nodes));
      graph_kernel_nodes = 0;
      for (hipGraphNode_t n : nodes) {
        hipGraphNodeType ty;
        IDX_HIP(hipGraphNodeGetType(n, &ty));
        IDX_CHECK(ty == hipGraphNodeTypeKernel, "the captured decode step holds a node that is not a kernel launch");
        ++graph_kernel_nodes;
      }
      graph_key = key;
      exec = graph_exec;
    }
  }
  QwenState hs;
  for (int n = n_first; n < max_new; ++n) {
    if (exec) IDX_HIP(hipGraphLaunch(exec, st));
    else if (decode_step(w, max_new, n_eos, forced, out_logits, n_cols, all_cols, st)) return 1;
    if ((n + 1) % 8 == 0 && n + 1 < max_new) {      // an end id ends the generation: look every 8 steps (later launches change nothing)
      IDX_HIP(hipMemcpyAsync(&hs, w.st, sizeof(hs), hipMemcpyDeviceToHost, st));
      IDX_HIP(hipStreamSynchronize(st));
      if (hs.done) break;
    }
  }
  IDX_HIP(hipMemcpyAsync(&hs, w.st, sizeof(hs), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(out_ids, w.out_ids, max_new * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(hs.n_out >= 1 && hs.n_out <= max_new, "generation state");
  *n_out = hs.n_out;
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

size_t idxtts_qwen_workspace_bytes(const idxtts_ctx* ctx, int n_prompt, int max_new_tokens, int n_eos, int n_logit_cols) {
  if (!ctx || n_prompt <= 0 || max_new_tokens <= 0 || n_eos < 0 || n_logit_cols < 0) return 0;
  auto* m = dynamic_cast<const QwenModel*>(ctx->model.get());
  return m ? m->workspace_bytes(n_prompt, max_new_tokens, n_eos, n_logit_cols) : 0;
}

int idxtts_qwen_generate(idxtts_ctx* ctx, const int* prompt_ids, int n_prompt, int max_new_tokens, const int* eos_ids, int n_eos,
                         const int* forced_ids, int* out_ids, int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols,
                         void* workspace, size_t bytes, int use_graph, void* stream) {
  try {
    IDX_CHECK(ctx && ctx->finalized, "context not finalized");
    auto* m = dynamic_cast<QwenModel*>(ctx->model.get());
    IDX_CHECK(m, "not a Qwen context");
    return m->generate(prompt_ids, n_prompt, max_new_tokens, eos_ids, n_eos, forced_ids, out_ids, n_out, out_logits, logit_cols, n_logit_cols,
                       workspace, bytes, use_graph, static_cast<hipStream_t>(stream));
  } catch (const std::exception& e) { return fail(__FILE__, __LINE__, std::string("exception: ") + e.what()); }
}

int idxtts_qwen_step_graph_launches(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  auto* m = dynamic_cast<const QwenModel*>(ctx->model.get());
  return m && m->graph_exec ? m->graph_kernel_nodes : -1;
}

}  // extern "C"
