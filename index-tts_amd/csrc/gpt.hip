// IndexTTS-2 GPT stage on MI355X: prefill, KV-cached greedy decode and the latent pass.
//
// Reference: UnifiedVoice.inference_speech model_v2.py:796-895 (decode through GPT2InferenceModel.forward
// 131-225 + GenerationMixin._sample, or the accel_engine.generate plugin slot 871-883), and
// UnifiedVoice.forward 673-723 (latent pass).  The 24 GPT-2 blocks are third-party HF code
// (transformers_gpt2.py:615-674 is the in-tree spec).
//
// Two weight copies are kept on purpose (288 GB HBM): an MFMA-32x32 packed copy for the GEMM-shaped
// passes (prefill, latent: M = B*S rows) and a B-fragment stream-order copy for the M<=64 decode GEMVs.
//
// Decode step = 5 launches per layer, every activation an MFMA A-fragment image (gemv_fx.hip):
//   c_attn [LayerNorm 1 folded in] -> decode_attn (+ KV-cache write) -> c_proj (+ residual, in place)
//   -> c_fc [LayerNorm 2 folded in, gelu_new] -> mlp.c_proj (+ residual; K split over 4 workgroups per column tile, finished
//   by the last one to arrive),
// + final norms, head and ONE launch for sampler + next embedding + advance (greedy): 123 launches per token.  Every per-step scalar is device-resident, so the whole
// step is captured once into a hipGraph and replayed per token (launch-bound otherwise).
// The decode weight streams are fp32 by default; quantize_weights() rounds the model once to bf16 / fp8-e4m3 storage
// (BASELINE configs[4]) -- the arithmetic stays the fp32 MFMA.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gpt.h"
#include "model_util.h"

namespace idxtts {

GPTModel::GPTModel(const idxtts_gpt_config& c) : cfg(c) {}

bool GPTModel::accepts(const std::string& name) const {
  static const char* prefixes[] = {"gpt.h.", "gpt.ln_f.", "final_norm.", "mel_head.", "mel_embedding.", "text_embedding.",
                                   "mel_pos_embedding.", "text_pos_embedding.", "speed_emb."};
  for (const char* p : prefixes)
    if (name.rfind(p, 0) == 0) return true;
  return false;
}

// One decode weight stream: the matrix ([K][N] if kn, else [N][K]) packed at `kdepth` in the model's storage format (wstream.h) and
// uploaded; the matrix holds values the format represents exactly
static int upload_stream(DeviceArena& arena, const float* w, int N, int K, bool kn, int fmt, int kdepth, WeightStream* ws) {
  ws->N = N; ws->K = K; ws->fmt = fmt; ws->kdepth = kdepth;
  std::vector<unsigned char> buf(wstream_elems(N, K, kdepth) * wfmt_bytes(fmt));
  std::vector<float> scale(N, 1.0f);
  if (pack_wstream(buf.data(), w, N, K, kn, fmt, kdepth, scale.data())) IDX_FAIL("decode weights are not representable in the compact format (quantize_weights not applied?)");
  void* d = nullptr;
  if (arena.upload_bytes(buf.data(), buf.size(), &d)) return 1;
  ws->wp = d;
  if (fmt == WFMT_FP8) {
    float* ds = nullptr;
    if (arena.upload(scale.data(), scale.size(), &ds)) return 1;
    ws->wscale = ds;
  }
  return 0;
}

// HF Conv1D weight [K][N] -> every packed form: the GEMM's, the decode stream (gw) and, where gp is given, the plane GEMV's stream
// ln_g / ln_b (host, [K]) non-null: the decode copies get the LayerNorm in front of them folded in (gemv_fx.hip):
//   W' = diag(g) W (packed), u = colsum(W'), c = b . W + bias
static int make_proj(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& prefix, int K, int N, int fmt,
                     LinearWeights* lw, WeightStream* gw, WeightStream* gp, const HostTensor* ln_g = nullptr, const HostTensor* ln_b = nullptr,
                     const float** u_out = nullptr, const float** c_out = nullptr) {
  HostTensor *w = nullptr, *bias = nullptr;
  if (need(t, prefix + ".weight", {K, N}, &w) || need(t, prefix + ".bias", {N}, &bias)) return 1;
  // the split-bf16 copy is used by the latent pass only (the KV-cache-building prefill stays exact fp32)
  if (make_linear(arena, w->data.data(), bias->data.data(), N, K, {WP16_ALWAYS, W_KN}, lw)) return 1;
  const float* wm = w->data.data();
  std::vector<float> wf;
  if (ln_g) {
    wf.resize((size_t)K * N);
    std::vector<float> u(N), c(N);
    std::vector<double> ud(N, 0.0), cd(N, 0.0);
    for (int k = 0; k < K; ++k) {
      const float g = ln_g->data[k];
      const double b = ln_b->data[k];
      for (int n = 0; n < N; ++n) {
        const float wv = w->data[(size_t)k * N + n];
        const float wg = g * wv;
        wf[(size_t)k * N + n] = wg;
        ud[n] += (double)wg;
        cd[n] += b * (double)wv;
      }
    }
    for (int n = 0; n < N; ++n) { u[n] = (float)ud[n]; c[n] = (float)(cd[n] + (double)bias->data[n]); }
    float *du = nullptr, *dc = nullptr;
    if (arena.upload(u.data(), u.size(), &du) || arena.upload(c.data(), c.size(), &dc)) return 1;
    *u_out = du; *c_out = dc;
    wm = wf.data();
  }
  if (gp && upload_stream(arena, wm, N, K, true, fmt, 32, gp)) return 1;
  return upload_stream(arena, wm, N, K, true, fmt, 16, gw);
}

int GPTModel::quantize_weights(std::map<std::string, HostTensor>& t, int fmt) {
  IDX_CHECK(fmt == WFMT_F32 || fmt == WFMT_BF16 || fmt == WFMT_FP8, "weight format: 0 fp32, 1 bf16, 2 fp8-e4m3 + power-of-two column scale");
  IDX_CHECK(weight_fmt == WFMT_F32, "weights already quantised");
  if (fmt == WFMT_F32) return 0;
  if (fmt == WFMT_FP8 && fp8_check_device_decode(nullptr)) return 1;
  const int d = cfg.model_dim, f = 4 * d;
  auto fold = [&](const std::string& ln, const std::string& proj, int K, int N) -> int {
    HostTensor *g = nullptr, *b = nullptr, *w = nullptr, *bias = nullptr;
    if (need(t, ln + ".weight", {K}, &g) || need(t, ln + ".bias", {K}, &b) || need(t, proj + ".weight", {K, N}, &w) ||
        need(t, proj + ".bias", {N}, &bias)) return 1;
    std::vector<double> cd(N, 0.0);
    for (int k = 0; k < K; ++k) {
      const float gk = g->data[k];
      const double bk = b->data[k];
      float* row = &w->data[(size_t)k * N];
      for (int n = 0; n < N; ++n) { cd[n] += bk * (double)row[n]; row[n] = gk * row[n]; }
    }
    for (int n = 0; n < N; ++n) bias->data[n] = (float)(cd[n] + (double)bias->data[n]);
    quantize_matrix(w->data.data(), K, N, true, fmt);
    std::fill(g->data.begin(), g->data.end(), 1.0f);
    std::fill(b->data.begin(), b->data.end(), 0.0f);
    return 0;
  };
  auto plain = [&](const std::string& proj, int K, int N) -> int {
    HostTensor* w = nullptr;
    if (need(t, proj + ".weight", {K, N}, &w)) return 1;
    quantize_matrix(w->data.data(), K, N, true, fmt);
    return 0;
  };
  for (int i = 0; i < cfg.layers; ++i) {
    const std::string p = "gpt.h." + std::to_string(i);
    if (fold(p + ".ln_1", p + ".attn.c_attn", d, 3 * d) || plain(p + ".attn.c_proj", d, d)) return 1;
    if (fold(p + ".ln_2", p + ".mlp.c_fc", d, f) || plain(p + ".mlp.c_proj", f, d)) return 1;
  }
  HostTensor* hw = nullptr;
  if (need(t, "mel_head.weight", {cfg.number_mel_codes, d}, &hw)) return 1;
  quantize_matrix(hw->data.data(), d, cfg.number_mel_codes, false, fmt);
  weight_fmt = fmt;
  return 0;
}

int GPTModel::finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) {
  const int d = cfg.model_dim, f = 4 * d;
  IDX_CHECK(d == cfg.heads * 64, "head_dim must be 64");
  IDX_CHECK(cfg.layers > 0 && (d & 15) == 0, "config");
  {
    const int zeros[OOB_SLOTS] = {0};
    void* flag = nullptr;
    if (arena.upload_bytes(zeros, sizeof(zeros), &flag)) return 1;
    oob_flag = static_cast<int*>(flag);
  }
  layers.resize(cfg.layers);
  for (int i = 0; i < cfg.layers; ++i) {
    GPTLayer& L = layers[i];
    const std::string p = "gpt.h." + std::to_string(i);
    if (tensor_from(t, arena, p + ".ln_1.weight", {d}, &L.ln1_g) || tensor_from(t, arena, p + ".ln_1.bias", {d}, &L.ln1_b)) return 1;
    if (tensor_from(t, arena, p + ".ln_2.weight", {d}, &L.ln2_g) || tensor_from(t, arena, p + ".ln_2.bias", {d}, &L.ln2_b)) return 1;
    HostTensor *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    if (need(t, p + ".ln_1.weight", {d}, &g1) || need(t, p + ".ln_1.bias", {d}, &b1)) return 1;
    if (need(t, p + ".ln_2.weight", {d}, &g2) || need(t, p + ".ln_2.bias", {d}, &b2)) return 1;
    WeightStream* const no32 = nullptr;
    const bool p32 = weight_fmt != WFMT_F32 && d % 32 == 0;
    if (make_proj(t, arena, p + ".attn.c_attn", d, 3 * d, weight_fmt, &L.attn_l, &L.attn_g, p32 ? &L.attn_p : no32, g1, b1, &L.attn_u, &L.attn_c)) return 1;
    if (make_proj(t, arena, p + ".attn.c_proj", d, d, weight_fmt, &L.proj_l, &L.proj_g, p32 ? &L.proj_p : no32)) return 1;
    if (make_proj(t, arena, p + ".mlp.c_fc", d, f, weight_fmt, &L.fc_l, &L.fc_g, p32 ? &L.fc_p : no32, g2, b2, &L.fc_u, &L.fc_c)) return 1;
    if (make_proj(t, arena, p + ".mlp.c_proj", f, d, weight_fmt, &L.fc2_l, &L.fc2_g, p32 ? &L.fc2_p : no32)) return 1;
  }
  if (tensor_from(t, arena, "gpt.ln_f.weight", {d}, &lnf_g) || tensor_from(t, arena, "gpt.ln_f.bias", {d}, &lnf_b)) return 1;
  if (tensor_from(t, arena, "final_norm.weight", {d}, &fn_g) || tensor_from(t, arena, "final_norm.bias", {d}, &fn_b)) return 1;
  const int V = cfg.number_mel_codes;
  HostTensor* hw = nullptr;
  if (need(t, "mel_head.weight", {V, d}, &hw)) return 1;
  if (upload_stream(arena, hw->data.data(), V, d, false, weight_fmt, 16, &head_g)) return 1;
  if (weight_fmt != WFMT_F32 && d % 32 == 0 && upload_stream(arena, hw->data.data(), V, d, false, weight_fmt, 32, &head_p)) return 1;
  if (tensor_from(t, arena, "mel_head.bias", {V}, &head_b)) return 1;
  if (tensor_from(t, arena, "mel_embedding.weight", {V, d}, &mel_emb)) return 1;
  if (tensor_from(t, arena, "text_embedding.weight", {cfg.number_text_tokens + 1, d}, &text_emb)) return 1;
  if (tensor_from(t, arena, "mel_pos_embedding.emb.weight", {cfg.mel_pos_len, d}, &mel_pos)) return 1;
  if (tensor_from(t, arena, "text_pos_embedding.emb.weight", {cfg.text_pos_len, d}, &text_pos)) return 1;
  return 0;
}

// ---- workspace carving ----
GPTModel::Buffers GPTModel::carve(void* ws, int B, int S, int max_new, size_t prefill_rows) const {
  const int d = cfg.model_dim, V = cfg.number_mel_codes, L = cfg.layers;
  Buffers b;
  b.invariant = batch_invariant;
  Carver c(ws);
  const size_t rows = prefill_rows ? prefill_rows : (size_t)B * S;
  b.x = c.take<float>(rows * d);
  b.h = c.take<float>(rows * d);
  b.qkv = c.take<float>(rows * 3 * d);
  b.att = c.take<float>(rows * d);
  b.ff = c.take<float>(rows * 4 * d);
  b.Smax = max_new > 0 ? ((S + max_new + 3) & ~3) : 0;
  const size_t cache = (size_t)L * kv_layer_bytes(B, b.Smax);
  b.kcache = c.take<char>(cache);
  b.vcache = c.take<char>(cache);
  if (kv_fmt == 2) {      // (the other formats' carve is what it always was)
    b.kscale = c.take<float>((size_t)L * kv_layer_scales(B, b.Smax));
    b.vscale = c.take<float>((size_t)L * kv_layer_scales(B, b.Smax));
  }
  // decode activations as A-fragment images (frag_index, common.h); one contiguous region so it can be zeroed in one go
  b.xd = c.take<float>(frag_image_floats(B, d));
  b.frag_off = c.off - frag_image_floats(B, d) * sizeof(float);
  b.hd = c.take<float>(frag_image_floats(B, d));
  b.attd = c.take<float>(frag_image_floats(B, d));
  b.ffd = c.take<float>(frag_image_floats(B, 4 * d));
  b.pl_cnt = c.take<unsigned>((size_t)cdiv(std::max(V, 4 * d), 16));      // (arrival counters of the plane GEMV: part of the zeroed region)
  b.frag_bytes = c.off - b.frag_off;
  b.xrow = c.take<float>((size_t)B * d);
  b.hrow = c.take<float>((size_t)B * d);
  b.attrow = c.take<float>((size_t)B * d);
  b.ffrow = c.take<float>((size_t)B * 4 * d);
  b.stats = c.take<float>((size_t)cdiv(d, 16) * cdiv(B, 16) * 16 * 2);
  b.pl_slab = c.take<float>(std::max({gemv_pl_slab_floats(3 * d, d, B), gemv_pl_slab_floats(d, d, B), gemv_pl_slab_floats(4 * d, d, B),
                                      gemv_pl_slab_floats(d, 4 * d, B), gemv_pl_slab_floats(V, d, B), (size_t)64}));
  b.qkvd = c.take<float>((size_t)B * 3 * d);
  b.slab = c.take<float>((size_t)8 * B * d);
  b.logits = c.take<float>((size_t)B * V);
  b.seen = c.take<unsigned char>((size_t)B * V);
  b.finished = c.take<int>(B);
  b.cur_tok = c.take<int>(B);
  b.kstart = c.take<int>(B);
  b.ksb_cnt = c.take<unsigned>((size_t)cdiv(d, 16));
  b.attn_cnt = c.take<unsigned>((size_t)B * cfg.heads);
  b.attn_part = c.take<float>((size_t)B * cfg.heads * 16 * 66);
  b.state = c.take<DecodeState>(1);
  b.codes = c.take<long long>((size_t)B * (max_new > 0 ? max_new : 0));
  b.bytes = (c.off + 255) & ~(size_t)255;
  return b;
}

size_t GPTModel::workspace_bytes(int B, int S, int max_new) const { return carve(nullptr, B, S, max_new).bytes; }

// one transformer layer over M = B*S token rows (prefill / latent pass)
int GPTModel::layer_full(int li, const Buffers& w, int B, int S, const int* kstart, bool store_kv, hipStream_t st, const KvScatter* scatter) {
  // The prefill (store_kv) that fills an fp32 KV cache feeds an exact greedy decode: exact fp32 MFMA.  With a bf16 cache its keys and
  // values are rounded to 8 bits on the way in (relative 2^-9), which buries the split-bf16 GEMM's 2^-16 product error: that prefill
  // runs like the latent pass, mode-dependent (split-bf16 by default, 3-4 x the exact kernel's rate).  An fp8 cache keeps the exact
  // prefill: a key / value moved by the split GEMM's 2^-16 lands on the other e4m3 neighbour 250 x as often as one moved by an fp32
  // summation order, and each such flip is 2^-4 of the element -- measured against the oracle, max |dlogit| 5.5e-2 with the split
  // prefill and 1.8e-2 with the exact one (profiles/README.md "fp8 KV cache").
  // Batch-invariant mode: the exact kernel for every cache format -- one GEMM family whatever M is (its K groups follow K alone) -- and
  // the prefill attention's key tiles counted from each row's first real key, so a left-padded row is summed as the unpadded one.
  const bool exact = store_kv && (kv_fmt != 1 || batch_invariant);
  auto mm = [&](const LinearWeights& lw, const GemmArgs& ga) { return exact ? gemm_tn_forward(lw, ga, st) : gemm_forward(lw, ga, st); };
  const GPTLayer& L = layers[li];
  const int d = cfg.model_dim, M = B * S;
  RowsNormArgs n1;
  n1.x_in = w.x; n1.ld_in = d; n1.y = w.h; n1.ld_y = d; n1.M = M; n1.d = d; n1.mode = NORM_LN; n1.g1 = L.ln1_g; n1.b1 = L.ln1_b;
  if (rows_norm_forward(n1, st)) return 1;
  GemmArgs g;
  g.x = w.h; g.ldx = d; g.y = w.qkv; g.ldy = 3 * d; g.M = M;
  if (mm(L.attn_l, g)) return 1;
  if (store_kv && scatter) {      // decode-session admission: the rows go to their slots' cache regions
    if (kv_store_slots(w.qkv, kv_dst(li, w, scatter->slots), scatter->n, cfg.heads, S, w.Smax, d, scatter->slot_ids, scatter->len, st,
                       scatter->fan, scatter->first)) return 1;
  } else if (store_kv && w.kv_scratch) {      // score(): the cache formats' rounding of k / v in place, the one-layer region rewritten
    if (kv_fmt && kv_store_prefill(w.qkv, kv_dst(0, w, B), B, cfg.heads, S, w.Smax, d, st)) return 1;
  } else if (store_kv) {
    if (kv_store_prefill(w.qkv, kv_dst(li, w, B), B, cfg.heads, S, w.Smax, d, st)) return 1;
  }
  AttnArgs a;
  a.q = w.qkv; a.k = w.qkv + d; a.v = w.qkv + 2 * d; a.o = w.att;
  a.q_bs = a.k_bs = a.v_bs = (long)S * 3 * d; a.o_bs = (long)S * d;
  a.q_ts = a.k_ts = a.v_ts = 3 * d; a.o_ts = d;
  a.B = B; a.H = cfg.heads; a.Sq = S; a.Sk = S; a.causal = 1; a.kstart = kstart; a.scale = 0.125f;
  a.split_bf16 = !exact && get_gemm_mode() == GEMM_BF16X3;      // the prefill of an fp32 cache stays exact fp32
  a.tiles_from_kstart = store_kv && batch_invariant;
  if (flash_attn_forward(a, st)) return 1;
  GemmArgs p;
  p.x = w.att; p.ldx = d; p.y = w.x; p.ldy = d; p.res = w.x; p.ldr = d; p.M = M;
  if (mm(L.proj_l, p)) return 1;
  RowsNormArgs n2 = n1;
  n2.g1 = L.ln2_g; n2.b1 = L.ln2_b;
  if (rows_norm_forward(n2, st)) return 1;
  GemmArgs f1;
  f1.x = w.h; f1.ldx = d; f1.y = w.ff; f1.ldy = 4 * d; f1.M = M; f1.act = ACT_GELU_NEW;
  if (mm(L.fc_l, f1)) return 1;
  GemmArgs f2;
  f2.x = w.ff; f2.ldx = 4 * d; f2.y = w.x; f2.ldy = d; f2.res = w.x; f2.ldr = d; f2.M = M;
  if (mm(L.fc2_l, f2)) return 1;
  return 0;
}

// head on B rows: ln_f -> final_norm (one rows_norm launch, output as fragment images) -> mel_head -> w.logits
int GPTModel::head_logits(const Buffers& w, int B, const float* x, int ldx, bool x_frag, hipStream_t st) {
  const int V = cfg.number_mel_codes, d = cfg.model_dim;
  const bool pl = use_pl(B);
  RowsNormArgs n;
  n.x_in = x; n.ld_in = ldx; n.in_frag = x_frag ? 1 : 0; n.M = B; n.d = d;
  if (pl) { n.y = w.hrow; n.ld_y = d; } else { n.y = w.hd; n.ld_y = d; n.y_frag = 1; }
  n.mode = NORM_LN_LN; n.g1 = lnf_g; n.b1 = lnf_b; n.g2 = fn_g; n.b2 = fn_b;
  if (rows_norm_forward(n, st)) return 1;
  if (pl) {
    GemvPLArgs hv;
    hv.x = w.hrow; hv.ldx = d; hv.rows = B; hv.bias = head_b; hv.y = w.logits; hv.ldy = V; hv.slab = w.pl_slab; hv.counters = w.pl_cnt;
    if (gemv_pl_forward(head_p, hv, st)) return 1;
  } else {
    GemvFXArgs hv;
    hv.xf = w.hd; hv.rows = B; hv.bias = head_b; hv.y = w.logits; hv.ldy = V; hv.invariant = w.invariant;
    if (gemv_fx_forward(head_g, hv, st)) return 1;
  }
  return 0;
}

// where the fused tail writes the next step's input: the plane-GEMV step's fp32 row + statistics, or the fragment image
SampleArgs::Embed GPTModel::tail_embed(const Buffers& w, bool pl) const {
  SampleArgs::Embed e;
  if (pl) { e.x_row = w.xrow; e.x_stats = w.stats; } else e.x_frag = w.xd;
  e.mel_emb = mel_emb; e.mel_pos = mel_pos; e.d = cfg.model_dim;
  return e;
}

// head on B rows -> the step tail w describes: greedy sampler, sampler, beam stages, or a session's per-slot samplers
int GPTModel::head_and_sample(const Buffers& w, int B, const float* x, int ldx, bool x_frag, float penalty, int codes_ld,
                              float* logits_out, hipStream_t st) {
  const int V = cfg.number_mel_codes;
  const bool pl = use_pl(B);
  if (head_logits(w, B, x, ldx, x_frag, st)) return 1;
  if (w.beam_tail) {      // the beam stages (beam.h); a beam session's work on every live group, its last one with the fused tail
    BeamState bs = w.beam;
    bs.penalty = penalty;
    return beam_scores_forward(bs, st) || beam_select_forward(bs, st) || beam_reorder_forward(bs, st);
  }
  SampleArgs s;
  s.part = w.logits; s.parts = 1; s.part_rows = B; s.bias = nullptr; s.logits_out = logits_out;
  s.seen = w.seen; s.finished = w.finished; s.codes = w.codes; s.codes_ld = codes_ld; s.cur_tok = w.cur_tok;
  s.st = w.state; s.B = B; s.V = V; s.stop_token = cfg.stop_mel_token; s.penalty = penalty;
  s.forced = w.forced; s.forced_ld = w.forced_ld; s.invariant = w.invariant;
  s.logprob_out = w.logprobs; s.logprob_ld = codes_ld;
  if (w.slots) {      // decode session: the per-slot greedy tail (sample + next input row + the slot's own advance)
    s.embed = tail_embed(w, pl);
    if (w.slot_samp) return sample_slots_warp_forward(s, w.slots, w.slot_samp, nullptr, B, st);      // sampled session: each slot's own sampler
    return sample_slots_forward(s, w.slots, nullptr, B, st);
  }
  if (fused_tail(w)) {      // the sampler's workgroups also write the next step's input and advance the step scalars
    s.embed = tail_embed(w, pl);
    s.embed.st_rw = w.state;
  }
  if (w.samp.mode != 0) {
    const idxtts_sampling& r = w.samp;
    SampleWarpArgs sw;
    sw.base = s; sw.mode = r.mode; sw.temperature = r.temperature; sw.top_k = r.top_k; sw.top_p = r.top_p;
    sw.exp_noise = r.exp_noise; sw.seed = r.seed;
    return sample_warp_forward(sw, st);
  }
  return sample_greedy_forward(s, st);
}

// one autoregressive step for all B rows (replayable: no host-dependent arguments); 5 launches per layer, every
// activation a fragment image:  c_attn [LN1 folded] -> attention -> c_proj (+x, in place) -> c_fc [LN2 folded, gelu_new]
// -> mlp.c_proj (+x, in place)
// The decode step runs on the plane GEMV from idxtts_set_decode_plane_rows() rows on (default 17: two or more MFMA row tiles -- merged
// requests, 16 utterances x 3 beams).  Measured on the full-size model, 256 tokens, graph replay: 16 rows 0.328 s against 0.303 s on the
// fp32-MFMA GEMV (its single-round-trip launches win), 32 rows 0.432 / 0.432, 48 rows 0.567 / 0.612 (profiles/README.md "Round 4").
// A shape whose plane plan names no kernel (49..64 rows with K in 5121..10240, a compact model wider than d = 1280: gemv_pl_can_run)
// keeps the whole step on the fp32-MFMA GEMV, which serves every row count.
bool GPTModel::use_pl(int B) const {
  // batch-invariant mode: one GEMV family for 1..64 rows.  The plane GEMV's three bf16 planes are other arithmetic than the fp32 MFMA,
  // and it has no form below 5 rows, so the mode stays on the fp32-MFMA GEMV (48 rows: 0.612 s against 0.567 s per 256 tokens)
  if (batch_invariant) return false;
  if (weight_fmt == WFMT_F32 || B < get_decode_plane_rows() || cfg.model_dim % 32 != 0 || !head_p.wp) return false;
  const int d = cfg.model_dim;
  return gemv_pl_can_run(3 * d, d, B) && gemv_pl_can_run(d, d, B) && gemv_pl_can_run(4 * d, d, B) && gemv_pl_can_run(d, 4 * d, B) &&
         gemv_pl_can_run(cfg.number_mel_codes, d, B);
}
// sessions, and greedy one-shot generations: sample + next embedding + advance are ONE launch
bool GPTModel::fused_tail(const Buffers& w) const { return w.slots || (w.samp.mode == 0 && !w.beam_tail); }

// The decode step on the plane GEMV (gemv_pl.hip): the same five launches per layer, every activation a plain fp32 row-major matrix
// (split into bf16 planes inside the GEMV), the residual stream updated in place, the LayerNorm statistics handed from producer to consumer; greedy generations close the
// step with ONE launch (sample + next embedding + advance).
KvDst GPTModel::kv_dst(int li, const Buffers& w, int rows) const {
  const size_t per_layer = kv_layer_bytes(rows, w.Smax), scales = kv_layer_scales(rows, w.Smax);
  KvDst kv;
  kv.kcache = w.kcache + li * per_layer; kv.vcache = w.vcache + li * per_layer; kv.fmt = kv_fmt;
  if (kv_fmt == 2) { kv.kscale = w.kscale + li * scales; kv.vscale = w.vscale + li * scales; }
  return kv;
}

DecodeAttnArgs GPTModel::attn_args(int li, const Buffers& w, int B, int pos_hint) const {
  const KvDst kv = kv_dst(li, w, B);
  DecodeAttnArgs da;
  da.qkv_part = w.qkvd; da.parts = 1; da.part_rows = B; da.qkv_bias = nullptr;
  da.kcache = kv.kcache; da.vcache = kv.vcache; da.kv_fmt = kv.fmt; da.kscale = kv.kscale; da.vscale = kv.vscale; da.kstart = w.kstart;
  da.st = w.state; da.B = B; da.H = cfg.heads; da.Smax = w.Smax; da.d = cfg.model_dim; da.scale = 0.125f;
  da.nsplit = decode_attn_nsplit(B, cfg.heads); da.part = w.attn_part; da.cnt = w.attn_cnt; da.slot = w.slots;
  if (w.invariant) { da.invariant = 1; da.nsplit = decode_attn_inv_wgs(B, cfg.heads, w.Smax); }
  da.pos_hint = pos_hint;
  return da;
}

int GPTModel::decode_step_pl(const Buffers& w, int B, float penalty, int codes_ld, float* logits_base, int pos_hint, hipStream_t st) {
  const int d = cfg.model_dim, T = d / 16;
  const bool fused = fused_tail(w);
  if (!fused && embed_step_pl(w.xrow, w.stats, B, d, mel_emb, mel_pos, w.cur_tok, w.state, st)) return 1;
  for (int li = 0; li < cfg.layers; ++li) {
    const GPTLayer& L = layers[li];
    GemvPLArgs qa;      // qkv = c_attn(LN1(x)) + b, row-major for the attention kernel
    qa.x = w.xrow; qa.ldx = d; qa.rows = B; qa.colsum = L.attn_u; qa.bias = L.attn_c; qa.stats_in = w.stats; qa.stats_tiles = T;
    qa.y = w.qkvd; qa.ldy = 3 * d; qa.slab = w.pl_slab; qa.counters = w.pl_cnt;
    if (gemv_pl_forward(L.attn_p, qa, st)) return 1;
    DecodeAttnArgs da = attn_args(li, w, B, pos_hint);
    da.out_row = w.attrow;
    if (decode_attn_forward(da, st)) return 1;
    GemvPLArgs pa;      // x += c_proj(attn) + b (in place: a lane reads and writes only its own elements of x), + the row statistics of the new x
    pa.x = w.attrow; pa.ldx = d; pa.rows = B; pa.bias = L.proj_l.bias; pa.res = w.xrow; pa.y = w.xrow; pa.ldy = d; pa.stats_out = w.stats;
    pa.slab = w.pl_slab; pa.counters = w.pl_cnt;
    if (gemv_pl_forward(L.proj_p, pa, st)) return 1;
    GemvPLArgs fa;      // ff = gelu_new(c_fc(LN2(x)) + b)
    fa.x = w.xrow; fa.ldx = d; fa.rows = B; fa.colsum = L.fc_u; fa.bias = L.fc_c; fa.stats_in = w.stats; fa.stats_tiles = T; fa.act = 1; fa.y = w.ffrow; fa.ldy = 4 * d;
    fa.slab = w.pl_slab; fa.counters = w.pl_cnt;
    if (gemv_pl_forward(L.fc_p, fa, st)) return 1;
    GemvPLArgs fb;      // x += mlp.c_proj(ff) + b
    fb.x = w.ffrow; fb.ldx = 4 * d; fb.rows = B; fb.bias = L.fc2_l.bias; fb.res = w.xrow; fb.y = w.xrow; fb.ldy = d; fb.stats_out = w.stats;
    fb.slab = w.pl_slab; fb.counters = w.pl_cnt;
    if (gemv_pl_forward(L.fc2_p, fb, st)) return 1;
  }
  if (head_and_sample(w, B, w.xrow, d, false, penalty, codes_ld, logits_base, st)) return 1;
  return fused ? 0 : advance_state(w.state, st);
}

int GPTModel::decode_step(const Buffers& w, int B, float penalty, int codes_ld, float* logits_base, int pos_hint, hipStream_t st) {
  if (use_pl(B)) return decode_step_pl(w, B, penalty, codes_ld, logits_base, pos_hint, st);
  const int d = cfg.model_dim;
  const bool fused = fused_tail(w);      // the previous step's tail has written this step's x and advanced the step scalars
  if (!fused && embed_step(w.xd, B, d, mel_emb, mel_pos, w.cur_tok, w.state, st)) return 1;
  for (int li = 0; li < cfg.layers; ++li) {
    const GPTLayer& L = layers[li];
    GemvFXArgs qa;      // qkv = c_attn(LN1(x)) + b, row-major for the attention kernel
    qa.xf = w.xd; qa.rows = B; qa.colsum = L.attn_u; qa.bias = L.attn_c; qa.y = w.qkvd; qa.ldy = 3 * d; qa.invariant = w.invariant;
    if (gemv_fx_forward(L.attn_g, qa, st)) return 1;
    DecodeAttnArgs da = attn_args(li, w, B, pos_hint);
    da.out = w.attd;
    if (decode_attn_forward(da, st)) return 1;
    GemvFXArgs pa;      // x += c_proj(attn) + b  (in place: a thread reads and writes only its own element of x)
    pa.xf = w.attd; pa.rows = B; pa.bias = L.proj_l.bias; pa.res = w.xd; pa.y = w.xd; pa.y_frag = 1; pa.invariant = w.invariant;
    if (gemv_fx_forward(L.proj_g, pa, st)) return 1;
    GemvFXArgs fa;      // ff = gelu_new(c_fc(LN2(x)) + b)
    fa.xf = w.xd; fa.rows = B; fa.colsum = L.fc_u; fa.bias = L.fc_c; fa.act = 1; fa.y = w.ffd; fa.y_frag = 1; fa.invariant = w.invariant;
    if (gemv_fx_forward(L.fc_g, fa, st)) return 1;
    GemvFXArgs fb;      // x += mlp.c_proj(ff) + b; at full size K is also split across workgroups (gemv_fx_ksb: all 256 CUs stream), the
                        // partial sums combined in a fixed order by the last workgroup of each column tile to arrive (no combine launch)
    fb.xf = w.ffd; fb.rows = B; fb.bias = L.fc2_l.bias; fb.res = w.xd; fb.y = w.xd; fb.y_frag = 1;
    fb.slab = w.slab; fb.ksb_counters = w.ksb_cnt; fb.invariant = w.invariant;
    if (gemv_fx_forward(L.fc2_g, fb, st)) return 1;
  }
  if (head_and_sample(w, B, w.xd, d, true, penalty, codes_ld, logits_base, st)) return 1;
  return fused ? 0 : advance_state(w.state, st);
}

int GPTModel::step_key() const { return batch_invariant ? 1 << 16 : get_decode_geometry() | (get_decode_plane_rows() << 1); }

// one decode step captured into g (every per-step value is device-resident, so the graph replays the step); the caller drops g
int GPTModel::capture_step(const Buffers& w, int B, float penalty, int codes_ld, hipStream_t st, StepGraph* g) {
  IDX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = decode_step(w, B, penalty, codes_ld, nullptr, 0, st);
  const hipError_t e = hipStreamEndCapture(st, &g->graph);
  if (rc) return 1;
  IDX_HIP(e);
  IDX_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0));
  return 0;
}

// The legacy default stream cannot be captured into a graph: a one-shot generation on it runs on a private stream, ordered after
// everything already queued by the caller (the call ends with a host sync anyway: n_steps is a host value).
int GPTModel::call_stream(hipStream_t user, hipStream_t* st) {
  *st = user;
  if (user) return 0;
  if (!own_stream) IDX_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
  IDX_HIP(hipStreamSynchronize(user));
  *st = own_stream;
  return 0;
}

// The one-shot generations' driver (generate, generate_beam) on R = B * fan rows, row r on prompt r / fan with its left pad: resets
// the per-call state, prefills, runs the first head step, then steps 1 .. max_new - 1 -- eagerly (logits_out [max_new][R][V]), or
// with `graph` step 1 eagerly and the others replayed from `exec` (a kept graph of this shape) or else from a captured one, handed
// to *captured when that is not null.  Every poll_every steps it reads the poll_n device flags `poll` and stops when all are set.
int GPTModel::run_generation(const Buffers& w, const float* inputs_embeds, const int* pad_left_host, int B, int fan, int P, int max_new,
                             float penalty, float* logits_out, bool graph, hipGraphExec_t exec, StepGraph* captured, const int* poll,
                             int poll_n, int poll_every, int* steps_done, hipStream_t st, const GenerateCall& call) {
  const long long *const prefix = call.prefix.codes, *const prefix_host = call.prefix.host;
  const int k = call.prefix.k, pos0 = call.prefix.pos0;
  const int d = cfg.model_dim, V = cfg.number_mel_codes, S = P + 1 + k, R = B * fan;
  IDX_CHECK(k == 0 || (prefix && prefix_host), "null prefix");
  IDX_CHECK(call.takes == 1 || call.takes == fan, "takes: the rows of each prompt");
  const bool share_prefill = call.takes > 1;
  // ---- per-call state ----
  std::vector<int> kstart(R, 0);
  for (int r = 0; r < R; ++r) {
    kstart[r] = pad_left_host ? pad_left_host[r / fan] : 0;
    IDX_CHECK(kstart[r] >= 0 && kstart[r] < P, "pad_left out of range");
  }
  IDX_HIP(hipMemcpyAsync(w.kstart, kstart.data(), R * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.finished, 0, R * sizeof(int), st));
  IDX_HIP(hipMemsetAsync(w.ksb_cnt, 0, (size_t)cdiv(d, 16) * sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.attn_cnt, 0, (size_t)R * cfg.heads * sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.xd, 0, w.frag_bytes, st));      // padding rows of the fragment images (the region starts at xd)
  // input_ids of the reference = fake prefix of 1s + start_mel_token: both count for the repetition penalty
  std::vector<unsigned char> seen((size_t)R * V, 0);
  for (int r = 0; r < R; ++r) { seen[(size_t)r * V + 1] = 1; seen[(size_t)r * V + cfg.start_mel_token] = 1; }
  for (int r = 0; r < R; ++r)      // ... and so do the given codes behind them (HF's processor reads the whole input_ids)
    for (int j = 0; j < k; ++j) seen[(size_t)r * V + prefix_host[(size_t)(r / fan) * k + j]] = 1;
  IDX_HIP(hipMemcpyAsync(w.seen, seen.data(), seen.size(), hipMemcpyHostToDevice, st));
  const DecodeState s0{P + k, 1 + k, 0, 0};      // behind a prefix of k codes: the scalars an uninterrupted run holds after k steps
  IDX_HIP(hipMemcpyAsync(w.state, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
  const std::vector<int> tok(R, cfg.start_mel_token);
  IDX_HIP(hipMemcpyAsync(w.cur_tok, tok.data(), R * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));

  // ---- prefill: x = [inputs_embeds | mel_emb[start] + mel_pos[0]] ----
  // share_prefill (takes of one prompt: generate(takes > 1)): B prefill rows, one per prompt; each row's keys and values go to its fan
  // decode rows (the beam admission's fan-out), and so does its last position, the head's input
  const int Rp = share_prefill ? B : R, pfan = share_prefill ? 1 : fan;
  for (int j = 0; j < pfan; ++j)      // rows j, fan + j, 2 fan + j, ... from prompts 0, 1, 2, ...
    IDX_HIP(hipMemcpy2DAsync(w.x + (size_t)j * S * d, (size_t)pfan * S * d * sizeof(float), inputs_embeds, (size_t)P * d * sizeof(float),
                             (size_t)P * d * sizeof(float), B, hipMemcpyDeviceToDevice, st));
  GatherArgs ga;
  ga.out = w.x + (size_t)P * d; ga.ld_out = S * d; ga.d = d;
  ga.table[0] = mel_emb; ga.idx[0] = w.cur_tok;           // start_mel_token rows
  ga.table[1] = mel_pos; ga.idx[1] = w.finished;          // all zeros -> mel position 0
  if (gather_sum_rows(ga, Rp, st)) return 1;
  if (k > 0) {      // ... | mel_emb[prefix[j]] + mel_pos[pos0 + j], j < k]
    PrefixRows pr;
    pr.x = w.x; pr.S = S; pr.d = d; pr.P_all = P; pr.k_all = k; pr.prefix = prefix; pr.row_div = pfan; pr.pos0 = pos0;
    pr.mel_emb = mel_emb; pr.mel_pos = mel_pos; pr.V = V;
    if (prefix_input_rows(pr, Rp, k, st)) return 1;
  }
  if (share_prefill) {
    // the prefill rows' own left pads in w.kstart while they run (the decode rows' afterwards); the fan-out's first rows and lengths in
    // w.cur_tok, which nobody reads between the gather above and the sampler that rewrites it (2 B <= R entries)
    std::vector<int> pk(B), sc(2 * (size_t)B);
    for (int b = 0; b < B; ++b) { pk[b] = kstart[(size_t)b * fan]; sc[b] = b * fan; sc[B + b] = S; }
    IDX_HIP(hipMemcpyAsync(w.kstart, pk.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipMemcpyAsync(w.cur_tok, sc.data(), 2 * B * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipStreamSynchronize(st));      // the staging vectors go out of scope below
    KvScatter fo;
    fo.slot_ids = w.cur_tok; fo.len = w.cur_tok + B; fo.n = B; fo.slots = R; fo.fan = fan;
    for (int li = 0; li < cfg.layers; ++li)
      if (layer_full(li, w, B, S, w.kstart, true, st, &fo)) return 1;
    IDX_HIP(hipMemcpyAsync(w.kstart, kstart.data(), R * sizeof(int), hipMemcpyHostToDevice, st));
    float* const last = w.x + (size_t)B * S * d;      // [R][d] behind the B prefill rows (x holds R * S rows; fan <= (fan - 1) S)
    for (int j = 0; j < fan; ++j)
      IDX_HIP(hipMemcpy2DAsync(last + (size_t)j * d, (size_t)fan * d * sizeof(float), w.x + (size_t)(S - 1) * d, (size_t)S * d * sizeof(float),
                               d * sizeof(float), B, hipMemcpyDeviceToDevice, st));
    if (head_and_sample(w, R, last, d, false, penalty, max_new, logits_out, st)) return 1;
  } else {
    for (int li = 0; li < cfg.layers; ++li)
      if (layer_full(li, w, R, S, w.kstart, true, st)) return 1;
    // the first token: the head on the last position of every row
    if (head_and_sample(w, R, w.x + (size_t)(S - 1) * d, S * d, false, penalty, max_new, logits_out, st)) return 1;
  }
  if (!fused_tail(w) && advance_state(w.state, st)) return 1;

  // ---- decode ----
  struct Guard {      // a captured graph not handed over: released on every return path
    StepGraph g;
    ~Guard() { g.drop(); }
  } cap;
  int n_first = 1;
  if (graph && max_new > 2) {
    // step 1 runs eagerly (first-use function attributes are set outside the capture), steps >= 2 replay
    if (decode_step(w, R, penalty, max_new, nullptr, S + 1, st)) return 1;
    n_first = 2;
    if (!exec) {
      if (capture_step(w, R, penalty, max_new, st, &cap.g)) return 1;
      exec = cap.g.exec;
    }
  }
  std::vector<int> flags(poll_n);
  *steps_done = n_first;
  for (int n = n_first; n < max_new; ++n) {
    if (exec) {
      IDX_HIP(hipGraphLaunch(exec, st));
    } else {
      float* lo = logits_out ? logits_out + (size_t)n * R * V : nullptr;
      if (decode_step(w, R, penalty, max_new, lo, S + n, st)) return 1;      // S + n: keys this step reads
    }
    *steps_done = n + 1;
    if ((n + 1) % poll_every == 0 || n + 1 == max_new) {      // every row finished / every utterance done? (HF stops there)
      IDX_HIP(hipMemcpyAsync(flags.data(), poll, poll_n * sizeof(int), hipMemcpyDeviceToHost, st));
      IDX_HIP(hipStreamSynchronize(st));
      if (std::all_of(flags.begin(), flags.end(), [](int f) { return f != 0; })) break;
    }
  }
  if (captured) std::swap(*captured, cap.g);
  return 0;
}

// the rules sample_warp_forward applies, checked before anything runs (generate(), every row of a sampled session admission)
static int check_sampling(const idxtts_sampling& r) {
  IDX_CHECK(r.mode == 0 || r.mode == SAMPLE_HF || r.mode == SAMPLE_ACCEL, "sampling mode (0 greedy, 1 HF, 2 accel)");
  if (r.mode == 0) return 0;
  IDX_CHECK(r.temperature > 0.0f, "sampling needs a positive temperature");
  IDX_CHECK(r.top_k >= 0 && r.top_p > 0.0f, "sampling parameters");
  IDX_CHECK(r.top_p >= 1.0f || (r.top_k > 0 && r.top_k <= 1024), "top-p needs 0 < top_k <= 1024");
  return 0;
}

int GPTModel::generate(const float* inputs_embeds, const int* pad_left_host, int B, int P, int max_new, float penalty, long long* codes,
                       int* n_steps_out, float* logits_out, void* ws, size_t ws_bytes, int use_graph, hipStream_t user_stream,
                       const GenerateCall& call) {
  const idxtts_sampling* const sampling = call.sampling;
  const long long *const forced = call.forced, *const prefix = call.prefix.codes;
  float* const logprobs = call.logprobs;
  const int takes = call.takes, k = call.prefix.k;
  IDX_CHECK(inputs_embeds && codes && n_steps_out, "null pointer");
  IDX_CHECK(k >= 0 && (k == 0 || prefix), "prefix: k >= 0 codes per prompt (k > 0 needs the codes)");
  IDX_CHECK(k == 0 || call.prefix.pos0 == 1 || call.prefix.pos0 == 2, "prefix_pos0: 1 (the reference's layout) or 2 (the uninterrupted run's)");
  IDX_CHECK(k == 0 || !forced, "teacher forcing together with a prefix is not supported");
  GenScope gen_scope(this);
  IDX_CHECK(!forced || !(sampling && sampling->mode != 0), "teacher forcing is a greedy-mode instrument");
  IDX_CHECK(takes >= 1 && (takes == 1 || !forced), "takes >= 1 (teacher forcing: 1)");
  IDX_CHECK(B > 0 && B * takes <= 64 && P > 0 && max_new > 0, "shape (1 <= B * takes <= 64)");
  const int prompts = B;      // the prefill's rows; from here on B counts decode rows, row b * takes + j being take j of prompt b
  B *= takes;
  if (sampling && check_sampling(*sampling)) return 1;
  const int S = P + 1 + k;
  IDX_CHECK(max_new + 1 < cfg.mel_pos_len, "max_new_tokens exceeds the mel position table");
  IDX_CHECK((long long)k + max_new + 1 < cfg.mel_pos_len, "prefix + max_new_tokens exceed the mel position table");
  IDX_CHECK(ws && ws_bytes >= workspace_bytes(B, S, max_new), "workspace too small");
  hipStream_t st = nullptr;
  if (call_stream(user_stream, &st)) return 1;
  std::vector<long long> hp((size_t)prompts * k);      // the given codes: checked here, and counted as seen by the repetition penalty
  if (k > 0) {
    IDX_HIP(hipMemcpyAsync(hp.data(), prefix, hp.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    IDX_HIP(hipStreamSynchronize(st));
    for (long long c : hp) {
      IDX_CHECK(c >= 0 && c < cfg.number_mel_codes, "prefix: a code outside the mel code table");
      IDX_CHECK(c != cfg.stop_mel_token, "prefix contains the stop token: nothing follows a stop token");
    }
  }
  Buffers w = carve(ws, B, S, max_new);
  if (sampling && sampling->mode != 0) w.samp = *sampling;
  w.forced = forced; w.forced_ld = max_new;
  w.logprobs = logprobs;      // the samplers write the caller's buffer; a kept graph is keyed by it (GraphSlot::logprobs)
  // every launch writes w.codes (a stable address: the captured decode step can be kept); the caller's pad fill in, copied out at the end
  IDX_HIP(hipMemcpyAsync(w.codes, codes, (size_t)B * max_new * sizeof(long long), hipMemcpyDeviceToDevice, st));

  // Instantiated decode-step graphs of greedy generations are kept (graph_cache): nothing call-specific is baked into their launches
  const bool graph = use_graph && !logits_out && !forced && !prof_enabled();
  const bool cacheable = graph && w.samp.mode == 0;
  const int geom = step_key();
  struct SlotLease {       // a cached graph in use by this call
    GPTModel* m = nullptr; int idx = -1;
    ~SlotLease() { if (m && idx >= 0) { std::lock_guard<std::mutex> l(m->graph_mu); m->graph_cache[idx].in_use = false; } }
  } lease;
  hipGraphExec_t exec = nullptr;
  if (cacheable) {
    std::lock_guard<std::mutex> l(graph_mu);
    for (size_t i = 0; i < graph_cache.size(); ++i) {
      GraphSlot& g = graph_cache[i];
      if (!g.in_use && g.ws == ws && g.ws_bytes == ws_bytes && g.B == B && g.S == S && g.max_new == max_new && g.penalty == penalty && g.kv_fmt == kv_fmt && g.geom == geom &&
          g.logprobs == logprobs) {
        g.in_use = true; g.stamp = ++graph_stamp; exec = g.step.exec; lease.m = this; lease.idx = (int)i;
        break;
      }
    }
  }
  StepGraph fresh;
  int steps_done = 0;
  GenerateCall run = call;
  run.prefix.host = hp.data();
  if (run_generation(w, inputs_embeds, pad_left_host, prompts, takes, P, max_new, penalty, logits_out, graph, exec, cacheable ? &fresh : nullptr,
                     w.finished, B, 16, &steps_done, st, run)) return 1;
  if (fresh.exec) {      // keep it: a free cache slot, or the least recently used idle one
    std::lock_guard<std::mutex> l(graph_mu);
    int slot = -1;
    // an idle entry on the same workspace address describes launches that can no longer be replayed safely: replace it
    for (size_t i = 0; i < graph_cache.size() && slot < 0; ++i) if (!graph_cache[i].in_use && graph_cache[i].ws == ws) slot = (int)i;
    if (slot < 0 && graph_cache.size() < GRAPH_CACHE_MAX) { graph_cache.emplace_back(); slot = (int)graph_cache.size() - 1; }
    if (slot < 0) {
      for (size_t i = 0; i < graph_cache.size(); ++i)
        if (!graph_cache[i].in_use && (slot < 0 || graph_cache[i].stamp < graph_cache[slot].stamp)) slot = (int)i;
    }
    if (slot >= 0) {
      GraphSlot& g = graph_cache[slot];
      g.step.drop();
      g.ws = ws; g.ws_bytes = ws_bytes; g.B = B; g.S = S; g.max_new = max_new; g.penalty = penalty; g.kv_fmt = kv_fmt; g.geom = geom;
      g.logprobs = logprobs;
      g.step = fresh; g.stamp = ++graph_stamp;
    } else {
      fresh.drop();
    }
  }

  // exact HF length: generation stops at the first step after which every row has emitted the stop token
  std::vector<long long> hc((size_t)B * max_new);
  IDX_HIP(hipMemcpyAsync(codes, w.codes, hc.size() * sizeof(long long), hipMemcpyDeviceToDevice, st));
  IDX_HIP(hipMemcpyAsync(hc.data(), w.codes, hc.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  int n_steps = steps_done;
  int worst = 0;
  bool every_row_stops = true;
  for (int b = 0; b < B; ++b) {
    int first = -1;
    for (int s = 0; s < steps_done; ++s)
      if (hc[(size_t)b * max_new + s] == cfg.stop_mel_token) { first = s; break; }
    if (first < 0) every_row_stops = false;
    else worst = std::max(worst, first + 1);
  }
  if (every_row_stops && !forced) n_steps = worst;      // forced: every step that ran is reported (codes = the rows' own choices)
  *n_steps_out = n_steps;
  return 0;
}

// ---- scoring given codes (idxtts.h; gpt.h) ----
// The head's buffers for SCORE_CHUNK rows (Buffers fields head_logits uses) and the chunk's packed hidden rows, carved from c
GPTModel::ScoreHead GPTModel::carve_score_head(Carver& c, const Buffers& base, size_t positions) const {
  const int d = cfg.model_dim, V = cfg.number_mel_codes;
  ScoreHead h;
  h.w = base;
  h.w.hd = c.take<float>(frag_image_floats(SCORE_CHUNK, d));
  h.hd_bytes = frag_image_floats(SCORE_CHUNK, d) * sizeof(float);
  h.w.hrow = c.take<float>((size_t)SCORE_CHUNK * d);
  h.w.logits = c.take<float>((size_t)SCORE_CHUNK * V);
  size_t slab = 64;      // the head's plan follows the chunk's row count: the largest slab any count asks for
  for (int r = 1; r <= SCORE_CHUNK; ++r) slab = std::max(slab, gemv_pl_slab_floats(V, d, r));
  h.w.pl_slab = c.take<float>(slab);
  h.xs = c.take<float>((size_t)SCORE_CHUNK * d);
  h.tok = c.take<int>(positions);
  h.dst = c.take<int>(positions);
  return h;
}

// ln_f -> final_norm -> mel_head -> score_rows_kernel over the hidden rows of `runs` (each `rows` consecutive rows of d floats), packed
// one run behind the other and cut into chunks of SCORE_CHUNK: the head weights stream ceil(positions / SCORE_CHUNK) times.  Packed
// position i is scored for code tok[i] and its value goes to out[dst[i]]; with logits_out its logits row goes to logits_out[dst[i]].
// Each chunk takes the head's plan for its own row count, as a decode step of that many rows does.
int GPTModel::score_positions(const ScoreHead& h, const std::vector<ScoreRun>& runs, const std::vector<int>& tok, const std::vector<int>& dst,
                              float* out, float* logits_out, hipStream_t st) {
  const int d = cfg.model_dim, V = cfg.number_mel_codes, T = (int)tok.size();
  if (T == 0) return 0;
  IDX_HIP(hipMemcpyAsync(h.tok, tok.data(), T * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(h.dst, dst.data(), T * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(h.w.hd, 0, h.hd_bytes, st));      // padding rows of the head's fragment image
  IDX_HIP(hipStreamSynchronize(st));                       // (the caller's vectors may go out of scope)
  size_t run = 0; int used = 0;      // the next unpacked row: row `used` of runs[run]
  for (int c0 = 0; c0 < T; c0 += SCORE_CHUNK) {
    const int rows = std::min(SCORE_CHUNK, T - c0);
    for (int r = 0; r < rows;) {
      while (used == runs[run].rows) { ++run; used = 0; }
      const int m = std::min(rows - r, runs[run].rows - used);
      IDX_HIP(hipMemcpyAsync(h.xs + (size_t)r * d, runs[run].x + (size_t)used * d, (size_t)m * d * sizeof(float), hipMemcpyDeviceToDevice, st));
      r += m; used += m;
    }
    if (head_logits(h.w, rows, h.xs, d, false, st)) return 1;
    ScoreRowsArgs sr;
    sr.logits = h.w.logits; sr.rows = rows; sr.V = V; sr.tok = h.tok + c0; sr.dst = h.dst + c0; sr.out = out;
    if (score_rows_forward(sr, st)) return 1;
    for (int r = 0; logits_out && r < rows;) {      // the slab rows out: one copy per run of consecutive destinations
      int e = r + 1;
      while (e < rows && dst[c0 + e] == dst[c0 + e - 1] + 1) ++e;
      IDX_HIP(hipMemcpyAsync(logits_out + (size_t)dst[c0 + r] * V, h.w.logits + (size_t)r * V, (size_t)(e - r) * V * sizeof(float),
                             hipMemcpyDeviceToDevice, st));
      r = e;
    }
  }
  return 0;
}

// Workspace of score(): carve()'s buffers for B * S prefill rows without a cache (max_new = 0), then the head's, the codes the prefill
// feeds, and for a bf16 / fp8 KV format one layer of cache.
GPTModel::ScoreBuffers GPTModel::carve_score(void* ws, int B, int S) const {
  ScoreBuffers sb;
  sb.w = carve(ws, B, S, 0);
  Carver c(ws);
  c.off = sb.w.bytes;
  const size_t T = (size_t)B * (S > 1 ? S - 1 : 1);      // scored positions at most: n = S - P <= S - 1 a row
  sb.head = carve_score_head(c, sb.w, T);
  sb.fed = c.take<long long>(T);
  sb.w.kv_scratch = true;
  sb.w.Smax = (S + 3) & ~3;
  if (kv_fmt) {
    sb.w.kcache = c.take<char>(kv_layer_bytes(B, sb.w.Smax));
    sb.w.vcache = c.take<char>(kv_layer_bytes(B, sb.w.Smax));
  }
  if (kv_fmt == 2) {
    sb.w.kscale = c.take<float>(kv_layer_scales(B, sb.w.Smax));
    sb.w.vscale = c.take<float>(kv_layer_scales(B, sb.w.Smax));
  }
  sb.bytes = (c.off + 255) & ~(size_t)255;
  return sb;
}

// The prefill of generate() behind a prefix, on [prompt | start | c_0 .. c_{n-2}] (the same input kernels, layer_full as that prefill
// runs it for the context's KV format, nothing cached); then every scored position P + j, j < n_b, through score_positions.
int GPTModel::score(const float* inputs_embeds, const int* pad_left_host, int B, int P, const long long* codes, const int* lens_host, int n,
                    int pos0, float* logprobs, float* logits_out, void* ws, size_t ws_bytes, hipStream_t st) {
  const int d = cfg.model_dim, V = cfg.number_mel_codes;
  IDX_CHECK(inputs_embeds && codes && logprobs, "null pointer");
  IDX_CHECK(B >= 1 && B <= 64 && P > 0 && n >= 1, "shape (1 <= B <= 64, n >= 1)");
  IDX_CHECK(pos0 == 1 || pos0 == 2, "prefix_pos0: 1 (the reference's layout) or 2 (the uninterrupted run's)");
  IDX_CHECK((long long)pos0 + n - 1 < cfg.mel_pos_len, "the codes exceed the mel position table");
  const int S = P + n, k = n - 1;
  IDX_CHECK(ws && ws_bytes >= score_workspace_bytes(B, P, n), "workspace too small");
  std::vector<int> len(B, n), kstart(B, 0);
  for (int b = 0; b < B; ++b) {
    if (lens_host) len[b] = lens_host[b];
    IDX_CHECK(len[b] >= 1 && len[b] <= n, "lens: 1 <= n_b <= n");
    if (pad_left_host) kstart[b] = pad_left_host[b];
    IDX_CHECK(kstart[b] >= 0 && kstart[b] < P, "pad_left out of range");
  }
  GenScope gen_scope(this);
  std::vector<long long> hc((size_t)B * n);
  IDX_HIP(hipMemcpyAsync(hc.data(), codes, hc.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  ScoreBuffers sb = carve_score(ws, B, S);
  const Buffers& w = sb.w;
  std::vector<long long> fed((size_t)B * std::max(k, 1), 0);      // padding: code 0, a valid table row
  std::vector<int> tok, dst;
  std::vector<ScoreRun> runs;
  for (int b = 0; b < B; ++b) {
    for (int j = 0; j < len[b]; ++j) {
      const long long c = hc[(size_t)b * n + j];
      IDX_CHECK(c >= 0 && c < V, "codes: a code outside the mel code table");
      IDX_CHECK(c != cfg.stop_mel_token || j == len[b] - 1, "codes: a stop token before a row's last code (nothing follows a stop token)");
      if (j < len[b] - 1) fed[(size_t)b * k + j] = c;
      tok.push_back((int)c);
      dst.push_back(b * n + j);
    }
    runs.push_back(ScoreRun{w.x + ((size_t)b * S + P) * d, len[b]});      // row b's scored positions P .. P + n_b - 1
  }

  const std::vector<int> start(B, cfg.start_mel_token);
  IDX_HIP(hipMemcpyAsync(w.kstart, kstart.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.cur_tok, start.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.finished, 0, B * sizeof(int), st));
  if (k > 0) IDX_HIP(hipMemcpyAsync(sb.fed, fed.data(), (size_t)B * k * sizeof(long long), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(w.pl_cnt, 0, (size_t)cdiv(std::max(V, 4 * d), 16) * sizeof(unsigned), st));      // the plane GEMV's arrival counters
  IDX_HIP(hipMemsetAsync(logprobs, 0, (size_t)B * n * sizeof(float), st));      // lp[b][j] = 0 from n_b on
  if (logits_out) IDX_HIP(hipMemsetAsync(logits_out, 0, (size_t)B * n * V * sizeof(float), st));
  IDX_HIP(hipStreamSynchronize(st));      // the staging vectors are read by then

  // ---- prefill: x = [inputs_embeds | mel_emb[start] + mel_pos[0] | mel_emb[c_j] + mel_pos[pos0 + j], j < n - 1] ----
  IDX_HIP(hipMemcpy2DAsync(w.x, (size_t)S * d * sizeof(float), inputs_embeds, (size_t)P * d * sizeof(float), (size_t)P * d * sizeof(float), B,
                           hipMemcpyDeviceToDevice, st));
  GatherArgs ga;
  ga.out = w.x + (size_t)P * d; ga.ld_out = S * d; ga.d = d;
  ga.table[0] = mel_emb; ga.idx[0] = w.cur_tok;
  ga.table[1] = mel_pos; ga.idx[1] = w.finished;      // all zeros -> mel position 0
  if (gather_sum_rows(ga, B, st)) return 1;
  if (k > 0) {
    PrefixRows pr;
    pr.x = w.x; pr.S = S; pr.d = d; pr.P_all = P; pr.k_all = k; pr.prefix = sb.fed; pr.pos0 = pos0;
    pr.mel_emb = mel_emb; pr.mel_pos = mel_pos; pr.V = V;
    if (prefix_input_rows(pr, B, k, st)) return 1;
  }
  for (int li = 0; li < cfg.layers; ++li)
    if (layer_full(li, w, B, S, w.kstart, true, st)) return 1;
  return score_positions(sb.head, runs, tok, dst, logprobs, logits_out, st);
}

// ---- decode session (continuous batching; gpt.h) ----
// Workspace: the decode buffers of a `slots`-row generation with Smax = max_prompt + 1 + max_new (rounded to 4), whose prefill
// activations are sized for an admission of up to every slot at max_prompt (+ 256 rows: see session_admit), then the per-slot state,
// the staged last prefill rows and the admission's index arrays.
GPTModel::SessionBuffers GPTModel::carve_session(void* ws, const SessionShape& shape) const {
  const int slots = shape.slots, max_prompt = shape.max_prompt, max_new = shape.max_new, num_beams = shape.num_beams;
  SessionBuffers sb;
  const size_t pre = session_prefill_rows(slots, max_prompt, shape.prefix ? max_new : 0);
  sb.w = carve(ws, slots, max_prompt + 1, max_new, pre);
  Carver c(ws);
  c.off = sb.w.bytes;
  sb.w.slots = c.take<SlotState>(slots);
  sb.x_last = c.take<float>((size_t)slots * cfg.model_dim);
  sb.ids = c.take<int>(slots);
  sb.plen = c.take<int>(pre);
  sb.klen = c.take<int>(slots);
  sb.cap = c.take<int>(slots);
  sb.samp = nullptr;
  if (shape.sampled) sb.w.slot_samp = sb.samp = c.take<SlotSampling>(slots);
  sb.bb = BeamBuffers{};
  sb.beam = nullptr;
  if (num_beams > 0) {      // beam session: slots / num_beams groups
    const int G = slots / num_beams, V = cfg.number_mel_codes;
    c.off = (c.off + 255) & ~(size_t)255;
    sb.bb = carve_beam(ws ? static_cast<char*>(ws) + c.off : nullptr, G, num_beams, V, max_new);
    c.off += sb.bb.bytes;
    sb.beam = c.take<SlotBeam>(G);
    const Buffers& w = sb.w;
    sb.w.beam_tail = true;
    BeamState& b = sb.w.beam;
    b = beam_state(w, sb.bb, G, num_beams, max_new);
    b.slots = w.slots; b.group = sb.beam;
    if (use_pl(slots)) { b.x_row = w.xrow; b.x_stats = w.stats; } else b.x_frag = w.xd;
    b.mel_emb = mel_emb; b.mel_pos = mel_pos; b.d = cfg.model_dim;
  }
  if (shape.scores) sb.w.logprobs = c.take<float>((size_t)slots * max_new);      // (after everything else: flags 0 and 1 keep their layout)
  sb.pk = sb.poff = nullptr;
  if (shape.prefix) { sb.pk = c.take<int>(slots); sb.poff = c.take<int>(slots); }
  if (shape.prefix_scores) {      // (behind everything else: every other flag combination keeps its size and layout)
    sb.score = carve_score_head(c, sb.w, (size_t)slots * max_new);
    sb.lp_stage = c.take<float>((size_t)slots * max_new);
  }
  sb.bytes = (c.off + 255) & ~(size_t)255;
  return sb;
}

size_t GPTModel::session_workspace_bytes(const SessionShape& shape) const { return carve_session(nullptr, shape).bytes; }

GPTModel::Session* GPTModel::find_session(void* ws) {
  std::lock_guard<std::mutex> l(session_mu);
  auto it = sessions.find(ws);
  return it == sessions.end() ? nullptr : &it->second;
}

int GPTModel::session_init(void* ws, size_t ws_bytes, const SessionShape& shape, float penalty, hipStream_t st) {
  const int slots = shape.slots, max_prompt = shape.max_prompt, max_new = shape.max_new, num_beams = shape.num_beams;
  IDX_CHECK(ws, "null workspace");
  IDX_CHECK(num_beams == 0 || !shape.prefix, "a beam session takes no prefix: the scorer's length penalty and rows would have to count it");
  IDX_CHECK(num_beams == 0 || !shape.scores, "a beam session records no per-code scores: its hypotheses carry the scorer's");
  IDX_CHECK(!shape.prefix_scores || (shape.prefix && shape.scores), "IDXTTS_SESSION_PREFIX_SCORES needs IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_SCORES");
  IDX_CHECK(slots >= 1 && slots <= 64 && max_prompt >= 1 && max_new >= 1, "shape (1 <= slots <= 64)");
  IDX_CHECK(num_beams == 0 || (num_beams >= 2 && num_beams <= BEAM_MAX), "2 <= num_beams <= 8");
  IDX_CHECK(num_beams == 0 || slots % num_beams == 0, "slots must be a multiple of num_beams");
  IDX_CHECK(num_beams == 0 || !shape.sampled, "a beam session has no per-slot samplers");
  IDX_CHECK(max_new + 1 < cfg.mel_pos_len, "max_new_tokens exceeds the mel position table");
  IDX_CHECK(ws_bytes >= session_workspace_bytes(shape), "workspace too small");
  const SessionBuffers sb = carve_session(ws, shape);
  const Buffers& w = sb.w;
  const int d = cfg.model_dim;
  IDX_HIP(hipMemsetAsync(w.kstart, 0, slots * sizeof(int), st));
  IDX_HIP(hipMemsetAsync(w.ksb_cnt, 0, (size_t)cdiv(d, 16) * sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(w.attn_cnt, 0, (size_t)slots * cfg.heads * sizeof(unsigned), st));
  IDX_HIP(hipMemsetAsync(static_cast<char*>(ws) + w.frag_off, 0, w.frag_bytes, st));   // padding rows of the fragment images
  IDX_HIP(hipMemsetAsync(w.slots, 0, slots * sizeof(SlotState), st));                // every slot free
  IDX_HIP(hipMemsetAsync(sb.x_last, 0, (size_t)slots * d * sizeof(float), st));
  IDX_HIP(hipMemsetAsync(w.xrow, 0, (size_t)slots * d * sizeof(float), st));
  if (shape.sampled) IDX_HIP(hipMemsetAsync(sb.samp, 0, slots * sizeof(SlotSampling), st));      // every slot greedy
  if (num_beams) {      // every group free (SlotState zeroed above) and finished: no stale scorer state is ever read
    const int G = slots / num_beams;
    IDX_HIP(hipMemsetAsync(sb.beam, 0, G * sizeof(SlotBeam), st));
    std::vector<int> ones(G, 1);
    IDX_HIP(hipMemcpyAsync(sb.bb.done, ones.data(), G * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipMemsetAsync(sb.bb.hyp_n, 0, G * sizeof(int), st));
    IDX_HIP(hipStreamSynchronize(st));      // `ones` goes out of scope below
  }
  std::lock_guard<std::mutex> l(session_mu);
  Session& s = sessions[ws];
  s.step.drop();
  s = Session();
  s.shape = shape; s.penalty = penalty; s.kv_fmt = kv_fmt; s.gemm_mode = get_gemm_mode();
  s.invariant = batch_invariant;
  s.ws_bytes = ws_bytes;
  s.busy.assign(slots, 0);
  s.prompt.assign(slots, 0);
  s.first_in.assign(slots, 0);
  if (shape.sampled) s.samp.assign(slots, SlotSampling{0, 1.0f, 0, 1.0f, 0, nullptr});
  if (num_beams) s.beam.assign(slots / num_beams, SlotBeam{0, 1.0f, 0, 1.0f, 0.0, 0, 0, nullptr});
  return 0;
}

int GPTModel::session_release(void* ws) {
  std::lock_guard<std::mutex> l(session_mu);
  auto it = sessions.find(ws);
  IDX_CHECK(it != sessions.end(), "no decode session on this workspace");
  it->second.step.drop();
  sessions.erase(it);
  return 0;
}

int GPTModel::admit_prefill(Session& s, const SessionBuffers& sb, const Admission& a, int fan, const std::function<int()>& params,
                            int* S_out, const int** take_row, hipStream_t st) {
  const int n = a.n, ld_rows = a.ld_rows;
  const float* const inputs_embeds = a.inputs_embeds;
  const int *const prompt_lens = a.prompt_lens, *const ids = a.ids, *const caps = a.caps, *const takes = a.takes, *const prefix_lens = a.prefix_lens;
  IDX_CHECK(inputs_embeds && prompt_lens && ids && caps, "null pointer");
  IDX_CHECK(!prefix_lens || fan == 1, "a beam session takes no prefix");
  IDX_CHECK(!takes || (fan == 1 && take_row), "takes belong to sessions of single rows");
  const int units = s.shape.slots / fan;
  IDX_CHECK(n >= 1 && n <= units, "admit 1 .. slots / num_beams requests");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  int pmax = 0, T = 0;      // T: units taken (with takes: ids and caps have one entry per take, request after request)
  std::vector<char> taken(units, 0);
  for (int b = 0; b < n; ++b) {
    const int tb = takes ? takes[b] : 1;
    IDX_CHECK(tb >= 1 && T + tb <= units, "takes: at least 1 per request, at most the session's slots in all");
    for (int t = T; t < T + tb; ++t) {
      IDX_CHECK(ids[t] >= 0 && ids[t] < units, "slot or group id out of range");
      IDX_CHECK(!s.busy[ids[t] * fan] && !taken[ids[t]], "slot or group is not free");
      taken[ids[t]] = 1;
    }
    IDX_CHECK(prompt_lens[b] >= 1 && prompt_lens[b] <= s.shape.max_prompt && prompt_lens[b] <= ld_rows, "prompt length out of range");
    for (int t = T; t < T + tb; ++t) IDX_CHECK(caps[t] >= 1 && caps[t] <= s.shape.max_new, "token cap out of range (1 .. max_new)");
    const int kb = prefix_lens ? prefix_lens[b] : 0;      // (>= 0: session_admit has checked)
    // a row that holds its cap already has nothing to produce; k < cap <= max_new also keeps P + 1 + k inside the cache and k + 2
    // inside the position table (session_init: max_new + 1 < mel_pos_len)
    for (int t = T; t < T + tb; ++t) IDX_CHECK(kb < caps[t], "prefix: k >= cap, the row would have no code left to produce (cap counts prefix + new codes)");
    T += tb;
    pmax = std::max(pmax, prompt_lens[b] + kb);
  }
  // One right-padded prefill of the admitted rows: under the causal mask a row sees exactly the keys (and key tiles) it would see alone
  // with no left padding.  The GEMMs are chosen from the session's properties, never from n: with an fp32 cache layer_full runs the
  // exact kernel, and so it does with an fp8 cache; with a bf16 cache in split-bf16 mode gemm_forward takes the split-bf16 kernel from 256 rows on, so the prefill is padded
  // with zero rows (b >= n) to at least 256 rows -- every admission then runs the kernel a generate() batch of >= 256 prefill rows runs.
  // (A request with takes is one prefill row: it counts once.)
  const int S = pmax + 1;
  int rows = n;
  if (kv_fmt == 1 && s.gemm_mode == GEMM_BF16X3 && !s.invariant) rows = std::max(n, cdiv(256, S));      // (the mode's prefill is exact)
  const size_t pre = session_prefill_rows(s.shape.slots, s.shape.max_prompt, s.shape.prefix ? s.shape.max_new : 0);
  if (prefix_lens) IDX_CHECK((size_t)rows * S <= pre, "prefixed admission: " + std::to_string(rows) + " prefill rows x " + std::to_string(S) +
                             " positions exceed the session's prefill area of " + std::to_string(pre) + " positions: admit in smaller groups");
  IDX_CHECK((size_t)rows * S <= pre, "admission prefill exceeds the workspace");
  // takes: the index arrays of the fan-out live behind the prefill rows' lengths in sb.plen (rows <= pre / 2, n + 1 + T <= 2 slots + 1)
  IDX_CHECK(!takes || (size_t)rows + n + 1 + T <= pre, "admission index arrays exceed the workspace");
  if (params()) return 1;
  // first slots | (fan > 1: the group ids, sb.ids + n) | klen | cap | plen | (takes: first [n + 1], row [T])
  std::vector<int> stage((size_t)3 * s.shape.slots + rows + (takes ? n + 1 + T : 0), 0);
  for (int t = 0; t < T; ++t) {
    stage[t] = ids[t] * fan;
    if (fan > 1) stage[n + t] = ids[t];
    stage[2 * s.shape.slots + t] = caps[t];
  }
  for (int b = 0; b < n; ++b) stage[s.shape.slots + b] = prompt_lens[b] + 1 + (prefix_lens ? prefix_lens[b] : 0);
  for (int b = 0; b < rows; ++b) stage[3 * s.shape.slots + b] = b < n ? prompt_lens[b] : -1;
  if (takes) {
    int* const first = stage.data() + 3 * s.shape.slots + rows;
    for (int b = 0, t = 0; b < n; t += takes[b], ++b) {
      first[b] = t; first[b + 1] = t + takes[b];
      for (int j = 0; j < takes[b]; ++j) first[n + 1 + t + j] = b;
    }
  }
  IDX_HIP(hipMemcpyAsync(sb.ids, stage.data(), (fan > 1 ? 2 : 1) * T * sizeof(int), hipMemcpyHostToDevice, st));      // 2 n <= slots
  IDX_HIP(hipMemcpyAsync(sb.klen, stage.data() + s.shape.slots, n * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(sb.cap, stage.data() + 2 * s.shape.slots, T * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(sb.plen, stage.data() + 3 * s.shape.slots, (rows + (takes ? n + 1 + T : 0)) * sizeof(int), hipMemcpyHostToDevice, st));
  std::vector<int> pstage;      // prefixes: k of each request | its offset in the packed codes
  int kmax = 0;
  if (prefix_lens) {
    pstage.assign(2 * (size_t)s.shape.slots, 0);
    for (int b = 0, o = 0; b < n; o += prefix_lens[b], ++b) { pstage[b] = prefix_lens[b]; pstage[s.shape.slots + b] = o; kmax = std::max(kmax, prefix_lens[b]); }
    IDX_HIP(hipMemcpyAsync(sb.pk, pstage.data(), s.shape.slots * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipMemcpyAsync(sb.poff, pstage.data() + s.shape.slots, s.shape.slots * sizeof(int), hipMemcpyHostToDevice, st));
  }
  IDX_HIP(hipStreamSynchronize(st));      // the staging vectors go out of scope below

  if (session_prefill_input(sb.w.x, inputs_embeds, ld_rows, sb.plen, rows, S, cfg.model_dim, mel_emb, mel_pos, cfg.start_mel_token, st))
    return 1;
  if (kmax > 0) {      // the given codes behind the start token, at the mel positions the uninterrupted row fed them at (2, 3, ...)
    PrefixRows pr;
    pr.x = sb.w.x; pr.S = S; pr.d = cfg.model_dim; pr.P = sb.plen; pr.klen = sb.pk; pr.prefix = a.prefix; pr.off = sb.poff; pr.pos0 = 2;
    pr.mel_emb = mel_emb; pr.mel_pos = mel_pos; pr.V = cfg.number_mel_codes;
    if (prefix_input_rows(pr, n, kmax, st)) return 1;
  }
  KvScatter sc;
  sc.slot_ids = sb.ids; sc.len = sb.klen; sc.n = n; sc.slots = s.shape.slots; sc.fan = fan;
  if (takes) { sc.first = sb.plen + rows; *take_row = sb.plen + rows + n + 1; }
  for (int li = 0; li < cfg.layers; ++li)
    if (layer_full(li, sb.w, rows, S, nullptr, true, st, &sc)) return 1;
  *S_out = S;
  return 0;
}

// a slot's sampler as its table holds it (null, or mode 0: greedy)
static SlotSampling slot_sampling(const idxtts_sampling* r) {
  if (!r || r->mode == 0) return SlotSampling{0, 1.0f, 0, 1.0f, 0, nullptr};
  return SlotSampling{r->mode, r->temperature, r->top_k, r->top_p, r->seed, r->exp_noise};
}

// The first token of the n rows whose slots stand in sb.ids (admitted, or forked at 0): the head on all `slots` rows (the GEMV
// use_pl(slots) selects, as a generate() of `slots` rows), sampled for those slots only; the sampler writes their first decode input
int GPTModel::session_first_tokens(const Session& s, const SessionBuffers& sb, int n, hipStream_t st) {
  const Buffers& w = sb.w;
  if (head_logits(w, s.shape.slots, sb.x_last, cfg.model_dim, false, st)) return 1;
  SampleArgs sa;
  sa.part = w.logits; sa.parts = 1; sa.part_rows = s.shape.slots; sa.seen = w.seen; sa.codes = w.codes; sa.codes_ld = s.shape.max_new;
  sa.cur_tok = w.cur_tok; sa.B = s.shape.slots; sa.V = cfg.number_mel_codes; sa.stop_token = cfg.stop_mel_token; sa.penalty = s.penalty;
  sa.logprob_out = w.logprobs; sa.logprob_ld = s.shape.max_new;
  sa.embed = tail_embed(w, use_pl(s.shape.slots));
  return s.shape.sampled ? sample_slots_warp_forward(sa, w.slots, sb.samp, sb.ids, n, st) : sample_slots_forward(sa, w.slots, sb.ids, n, st);
}

int GPTModel::session_admit(void* ws, const Admission& adm, hipStream_t st) {
  Admission a = adm;      // (an admission whose prefixes are all empty drops them below)
  const int n = a.n;
  const int *const prompt_lens = a.prompt_lens, *const slot_ids = a.ids, *const takes = a.takes;
  const idxtts_sampling* const per_row = a.per_row;
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams == 0 || !a.prefix_lens, "a beam session takes no prefix (beams with a prefix are not supported)");
  IDX_CHECK(s.shape.num_beams == 0, "a beam session admits with _admit_beam (one idxtts_beam per request)");
  IDX_CHECK(!per_row || s.shape.sampled, "per-request sampling needs a session initialised with IDXTTS_SESSION_SAMPLED");
  IDX_CHECK(n >= 1 && n <= s.shape.slots, "admit 1 .. slots requests");
  // takes: slot_ids, caps and per_row have one entry per take, request after request (T of them); else one per request
  int T = n;
  if (takes) {
    T = 0;
    for (int b = 0; b < n; ++b) {
      IDX_CHECK(takes[b] >= 1 && T + takes[b] <= s.shape.slots, "takes: at least 1 per request, at most the session's slots in all");
      T += takes[b];
    }
  }
  GenScope gen_scope(this);
  const int d = cfg.model_dim, V = cfg.number_mel_codes;
  const SessionBuffers sb = carve_session(ws, s.shape);
  const Buffers& w = sb.w;
  // prefixes: the codes are read here -- nothing follows a stop token, and a code outside the table is no code.  No request with
  // codes: the admission of before, kernel for kernel.
  long long ktot = 0;
  if (a.prefix_lens)
    for (int b = 0; b < n; ++b) {
      IDX_CHECK(a.prefix_lens[b] >= 0 && a.prefix_lens[b] < s.shape.max_new, "prefix: k >= cap, the row would have no code left to produce (0 <= k < max_new_tokens)");
      ktot += a.prefix_lens[b];
    }
  IDX_CHECK(!a.from_model || s.shape.prefix_scores, "prefix log-probabilities from the model need a session initialised with "
            "IDXTTS_SESSION_PREFIX_SCORES (with IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_SCORES)");
  IDX_CHECK(!a.from_model || a.prefix_lens, "null prefix_lens");
  if (ktot == 0) { a.prefix_lens = nullptr; a.prefix = nullptr; a.prefix_logprobs = nullptr; a.from_model = nullptr; }
  if (a.from_model && !std::any_of(a.from_model, a.from_model + n, [](unsigned char f) { return f != 0; })) a.from_model = nullptr;
  std::vector<long long> hp((size_t)ktot);      // the packed prefix codes
  if (a.prefix_lens) {
    IDX_CHECK(s.shape.prefix, "a prefixed admission needs a session initialised with IDXTTS_SESSION_PREFIX (its prefill area holds prompt + prefix)");
    IDX_CHECK(a.prefix, "null prefix");
    IDX_HIP(hipMemcpyAsync(hp.data(), a.prefix, hp.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    IDX_HIP(hipStreamSynchronize(st));
    for (long long c : hp) {
      IDX_CHECK(c >= 0 && c < V, "prefix: a code outside the mel code table");
      IDX_CHECK(c != cfg.stop_mel_token, "prefix contains the stop token: nothing follows a stop token");
    }
  }
  auto params = [&]() -> int {      // the admitted slots' samplers (greedy when per_row is null); the other rows are rewritten unchanged
    if (!s.shape.sampled) return 0;
    if (per_row)
      for (int b = 0; b < T; ++b)
        if (check_sampling(per_row[b])) return 1;
    for (int b = 0; b < T; ++b) s.samp[slot_ids[b]] = slot_sampling(per_row ? per_row + b : nullptr);
    IDX_HIP(hipMemcpyAsync(sb.samp, s.samp.data(), s.shape.slots * sizeof(SlotSampling), hipMemcpyHostToDevice, st));
    return 0;
  };
  int S = 0;
  const int* take_row = nullptr;      // takes: the prefill row of each take (device)
  if (admit_prefill(s, sb, a, 1, params, &S, &take_row, st)) return 1;
  if (a.prefix_lens) {
    PrefixReset pr;
    pr.slots = w.slots; pr.seen = w.seen; pr.V = V; pr.start_token = cfg.start_mel_token; pr.x_last = sb.x_last; pr.x = w.x; pr.S = S; pr.d = d;
    pr.slot_ids = sb.ids; pr.P = sb.plen; pr.cap = sb.cap; pr.row = take_row; pr.klen = sb.pk; pr.off = sb.poff; pr.prefix = a.prefix;
    pr.prefix_lp = a.prefix_logprobs; pr.codes = w.codes; pr.codes_ld = s.shape.max_new; pr.logprobs = w.logprobs;
    if (a.from_model) {
      // _admit_prefix_scored: position P_b + j of request b's prefill row predicts its prefix code j -- the rows of every from_model
      // request through the scoring head into the staging buffer, packed as the codes are; the other requests' segments hold the
      // caller's values (or 0), and the reset below hands the buffer to every take's slot as the caller's array is handed
      std::vector<ScoreRun> runs;
      std::vector<int> tok, dst;
      for (int b = 0, o = 0; b < n; o += a.prefix_lens[b], ++b) {
        const int kb = a.prefix_lens[b];
        if (kb == 0) continue;
        if (a.from_model[b]) {
          runs.push_back(ScoreRun{w.x + ((size_t)b * S + prompt_lens[b]) * d, kb});
          for (int j = 0; j < kb; ++j) { tok.push_back((int)hp[(size_t)o + j]); dst.push_back(o + j); }
        } else if (a.prefix_logprobs) {
          IDX_HIP(hipMemcpyAsync(sb.lp_stage + o, a.prefix_logprobs + o, kb * sizeof(float), hipMemcpyDeviceToDevice, st));
        } else {
          IDX_HIP(hipMemsetAsync(sb.lp_stage + o, 0, kb * sizeof(float), st));
        }
      }
      if (score_positions(sb.score, runs, tok, dst, sb.lp_stage, nullptr, st)) return 1;
      pr.prefix_lp = sb.lp_stage;
    }
    if (session_reset_slots_prefix(pr, T, st)) return 1;
  } else if (session_reset_slots(w.slots, w.seen, V, cfg.start_mel_token, sb.x_last, w.x, S, d, sb.ids, sb.plen, sb.cap, T, st, take_row)) return 1;
  if (session_first_tokens(s, sb, T, st)) return 1;
  for (int b = 0, t = 0; b < n; ++b)
    for (int j = 0; j < (takes ? takes[b] : 1); ++j, ++t) {
      s.busy[slot_ids[t]] = 1; s.prompt[slot_ids[t]] = prompt_lens[b];
      s.first_in[slot_ids[t]] = !(a.prefix_lens && a.prefix_lens[b] > 0);      // behind a prefix x_last is position P + k's, not the prompt's last
    }
  return 0;
}

int GPTModel::session_step(void* ws, int n_steps, int use_graph, int* finished_slots, int* n_finished, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(n_steps >= 0, "n_steps");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  GenScope gen_scope(this);
  const SessionBuffers sb = carve_session(ws, s.shape);
  const Buffers& w = sb.w;
  const int geom = step_key();
  if (s.step.exec && s.geom != geom) s.step.drop();
  IDX_CHECK(st != nullptr || !use_graph, "graph replay needs a stream other than the legacy default stream");
  const bool graph_ok = use_graph && !prof_enabled();
  for (int k = 0; k < n_steps; ++k) {
    if (graph_ok && s.warm && !s.step.exec) {
      // every per-step value lives on the device (SlotState, seen, the input rows): admissions between replays keep the graph valid
      if (capture_step(w, s.shape.slots, s.penalty, s.shape.max_new, st, &s.step)) { s.step.drop(); return 1; }
      s.geom = geom;
    }
    if (graph_ok && s.step.exec) {
      IDX_HIP(hipGraphLaunch(s.step.exec, st));
    } else {
      if (decode_step(w, s.shape.slots, s.penalty, s.shape.max_new, nullptr, 0, st)) return 1;
      s.warm = true;
    }
  }
  std::vector<SlotState> hs(s.shape.slots);
  IDX_HIP(hipMemcpyAsync(hs.data(), w.slots, s.shape.slots * sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  int nf = 0;
  const int stride = s.shape.num_beams ? s.shape.num_beams : 1;      // beam sessions report the first slot of each finished group
  for (int i = 0; i < s.shape.slots; i += stride)
    if (s.busy[i] && !hs[i].live) { if (finished_slots) finished_slots[nf] = i; ++nf; }
  if (n_finished) *n_finished = nf;
  return 0;
}

int GPTModel::session_read(void* ws, int slot, long long* codes, int* n_codes, hipStream_t st, float* logprobs, bool scored) {
  IDX_SESSION(ws);
  IDX_CHECK(codes && n_codes && (logprobs || !scored), "null pointer");
  IDX_CHECK(!scored || s.shape.scores, "_read_scored needs a session initialised with IDXTTS_SESSION_SCORES");
  IDX_CHECK(slot >= 0 && slot < s.shape.slots && s.busy[slot], "slot holds no request");
  const SessionBuffers sb = carve_session(ws, s.shape);
  if (s.shape.num_beams) return session_read_beam(s, sb, slot, codes, n_codes, st);
  SlotState hs;
  IDX_HIP(hipMemcpyAsync(&hs, sb.w.slots + slot, sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(!hs.live, "slot is still decoding");
  IDX_CHECK(hs.step >= 1 && hs.step <= s.shape.max_new, "slot state corrupt");
  IDX_HIP(hipMemcpyAsync(codes, sb.w.codes + (size_t)slot * s.shape.max_new, (size_t)hs.step * sizeof(long long), hipMemcpyDeviceToDevice, st));
  if (scored)
    IDX_HIP(hipMemcpyAsync(logprobs, sb.w.logprobs + (size_t)slot * s.shape.max_new, (size_t)hs.step * sizeof(float), hipMemcpyDeviceToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  *n_codes = hs.step;
  s.busy[slot] = 0;
  return 0;
}

int GPTModel::session_read_nbest(void* ws, int slot, int n_best, long long* codes, int* lens, float* scores, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams > 0, "_read_nbest needs a beam session: every other session holds one sequence per slot (_read)");
  IDX_CHECK(codes && lens && scores, "null pointer");
  IDX_CHECK(slot >= 0 && slot < s.shape.slots && s.busy[slot], "slot holds no request");
  const SessionBuffers sb = carve_session(ws, s.shape);
  return session_read_beam(s, sb, slot, codes, lens, st, n_best, scores);
}

// evict and stop: every id is checked before anything changes; then one launch on the session's stream (ordered between step replays;
// the ids travel in the launch arguments) ends the requests' slots -- a beam group's num_beams slots, which is all the beam stages read
// to find a group dead (the state they leave a group in at its cap) -- and evict gives the units back
int GPTModel::session_end(void* ws, int n, const int* slot_ids, bool evict, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(n >= 0 && (slot_ids || n == 0), "null pointer");
  const int fan = s.shape.num_beams ? s.shape.num_beams : 1;
  unsigned long long mask = 0;
  for (int b = 0; b < n; ++b) {
    const int slot = slot_ids[b];
    IDX_CHECK(slot >= 0 && slot < s.shape.slots, "slot out of range");
    IDX_CHECK(slot % fan == 0, "a beam session's group is addressed by its first slot");
    IDX_CHECK(s.busy[slot], "slot holds no request");
    for (int j = 0; j < fan; ++j) mask |= 1ull << (slot + j);
  }
  const SessionBuffers sb = carve_session(ws, s.shape);
  if (session_end_slots(sb.w.slots, s.shape.slots, mask, !evict, st)) return 1;
  if (evict)
    for (int i = 0; i < s.shape.slots; ++i)
      if ((mask >> i) & 1ull) s.busy[i] = 0;
  return 0;
}

// ---- preempt and resume ----
ParkArgs GPTModel::park_args(const Session& s, const SessionBuffers& sb, int slot) const {
  const Buffers& w = sb.w;
  ParkArgs a;
  a.kcache = w.kcache; a.vcache = w.vcache; a.kscale = w.kscale; a.vscale = w.vscale;
  a.layer_bytes = kv_layer_bytes(s.shape.slots, w.Smax); a.layer_scales = kv_layer_scales(s.shape.slots, w.Smax);
  a.slot = slot; a.Smax = w.Smax; a.slots = w.slots; a.samp = sb.samp; a.seen = w.seen; a.codes = w.codes; a.codes_ld = s.shape.max_new;
  a.cur_tok = w.cur_tok; a.embed = tail_embed(w, use_pl(s.shape.slots)); a.B = s.shape.slots;
  a.logprobs = w.logprobs;
  return a;
}

int GPTModel::session_park_header(void* ws, int slot, idxtts_park_header* hdr, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams == 0, "one row of a beam group cannot be parked: park the group (idxtts_gpt_session_park_group)");
  IDX_CHECK(slot >= 0 && slot < s.shape.slots, "slot out of range");
  IDX_CHECK(s.busy[slot], "slot holds no request");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  const SessionBuffers sb = carve_session(ws, s.shape);
  SlotState hs;
  IDX_HIP(hipMemcpyAsync(&hs, sb.w.slots + slot, sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(hs.live, "slot has ended: read it, a request that is over cannot be parked");
  IDX_CHECK(hs.step >= 1 && hs.step < hs.max_step && hs.max_step <= s.shape.max_new && hs.pos >= 1 && hs.pos < sb.w.Smax, "slot state corrupt");
  idxtts_park_header h{};
  h.magic = IDXTTS_PARK_MAGIC; h.version = IDXTTS_PARK_VERSION;
  h.layers = cfg.layers; h.heads = cfg.heads; h.model_dim = cfg.model_dim; h.number_mel_codes = cfg.number_mel_codes;
  h.slots = s.shape.slots; h.kv_format = s.kv_fmt; h.gemm_mode = s.gemm_mode; h.sampled = s.shape.sampled ? IDXTTS_SESSION_SAMPLED : 0;
  h.pos = hs.pos; h.mel_pos = hs.mel_pos; h.step = hs.step; h.max_step = hs.max_step;
  h.mode = 0; h.temperature = 1.0f; h.top_k = 0; h.top_p = 1.0f;
  if (s.shape.sampled) {
    const SlotSampling& e = s.samp[slot];
    h.mode = e.mode; h.temperature = e.temperature; h.top_k = e.top_k; h.top_p = e.top_p; h.seed = e.seed;
    h.exp_noise = (unsigned long long)(uintptr_t)e.exp_noise;
  }
  h.reserved[0] = s.invariant;      // a row parked in the batch-invariant mode says so; every other row carries zeros
  h.reserved[1] = s.shape.scores ? 1 : 0; // a scored session's row carries its log-probabilities behind the codes
  h.bytes = park_layout(h.kv_format, h.layers, h.heads, h.number_mel_codes, h.pos, h.step, h.reserved[1]).bytes;
  *hdr = h;
  return 0;
}

size_t GPTModel::session_park_bytes(void* ws, int slot, hipStream_t st) {
  idxtts_park_header h;
  return session_park_header(ws, slot, &h, st) ? 0 : (size_t)h.bytes;
}

int GPTModel::session_park(void* ws, int slot, void* dst, size_t dst_bytes, size_t* written, hipStream_t st) {
  IDX_CHECK(dst, "null pointer");
  IDX_CHECK((uintptr_t)dst % 16 == 0, "the parked row must be 16-byte aligned");
  idxtts_park_header h;
  if (session_park_header(ws, slot, &h, st)) return 1;
  IDX_CHECK(dst_bytes >= h.bytes, "dst is smaller than the parked row (idxtts_gpt_session_park_bytes)");
  Session& s = *find_session(ws);
  ParkArgs a = park_args(s, carve_session(ws, s.shape), slot);
  a.hdr = h; a.blob = static_cast<char*>(dst);
  if (session_park_slot(a, st)) return 1;
  s.busy[slot] = 0;
  if (written) *written = (size_t)h.bytes;
  return 0;
}

int GPTModel::session_resume(void* ws, int slot, const void* src, size_t src_bytes, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams == 0, "a beam session resumes whole groups (idxtts_gpt_session_resume_group), not rows");
  IDX_CHECK(src, "null pointer");
  IDX_CHECK((uintptr_t)src % 16 == 0, "the parked row must be 16-byte aligned");
  IDX_CHECK(slot >= 0 && slot < s.shape.slots, "slot out of range");
  IDX_CHECK(!s.busy[slot], "slot is not free");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  IDX_CHECK(src_bytes >= sizeof(idxtts_park_header), "parked row shorter than its header");
  idxtts_park_header h;
  IDX_HIP(hipMemcpyAsync(&h, src, sizeof(h), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(h.magic == IDXTTS_PARK_MAGIC, "not a parked row (magic)");
  IDX_CHECK(h.version == IDXTTS_PARK_VERSION, "parked row of another format version");
  IDX_CHECK(h.layers == cfg.layers && h.heads == cfg.heads && h.model_dim == cfg.model_dim && h.number_mel_codes == cfg.number_mel_codes,
            "parked row of another model (dimensions)");
  IDX_CHECK(h.reserved[0] == 0 || h.reserved[0] == 1, "parked row's mode field is corrupt");
  IDX_CHECK(h.reserved[0] == s.invariant, "parked row and session differ in the batch-invariant mode");
  IDX_CHECK(h.reserved[1] == 0 || h.reserved[1] == 1, "parked row's scores field is corrupt");
  IDX_CHECK(h.reserved[1] == (s.shape.scores ? 1 : 0), "parked row and session differ in IDXTTS_SESSION_SCORES (a scored row carries a segment more)");
  // in the mode nothing on a row's path depends on the slot count: a row moves between sessions of any size
  IDX_CHECK(s.invariant || h.slots == s.shape.slots, "parked row of a session with a different number of slots (the key split and the GEMV differ)");
  IDX_CHECK(h.kv_format == s.kv_fmt, "parked row of another KV format");
  IDX_CHECK(h.gemm_mode == s.gemm_mode, "parked row of another GEMM mode");
  IDX_CHECK(h.mode == 0 || s.shape.sampled, "a sampled request needs a session initialised with IDXTTS_SESSION_SAMPLED");
  const SessionBuffers sb = carve_session(ws, s.shape);
  IDX_CHECK(h.max_step >= 1 && h.max_step <= s.shape.max_new, "token cap above the session's max_new_tokens");
  IDX_CHECK(h.step >= 1 && h.step < h.max_step && h.mel_pos == h.step + 1 && h.pos >= 1, "parked row's step scalars are corrupt");
  IDX_CHECK((long long)h.pos + (h.max_step - h.step) + 1 <= sb.w.Smax, "the request's remaining steps do not fit the session's cache");
  if (h.mode != 0) {
    idxtts_sampling r{h.mode, h.temperature, h.top_k, h.top_p, reinterpret_cast<const float*>((uintptr_t)h.exp_noise), h.seed};
    if (check_sampling(r)) return 1;
  }
  IDX_CHECK(h.bytes == park_layout(h.kv_format, h.layers, h.heads, h.number_mel_codes, h.pos, h.step, h.reserved[1]).bytes,
            "parked row's size field is corrupt");
  IDX_CHECK(src_bytes >= h.bytes, "parked row is truncated");
  ParkArgs a = park_args(s, sb, slot);
  a.hdr = h; a.blob = const_cast<char*>(static_cast<const char*>(src));
  if (session_resume_slot(a, st)) return 1;
  if (s.shape.sampled) s.samp[slot] = SlotSampling{h.mode, h.temperature, h.top_k, h.top_p, h.seed, reinterpret_cast<const float*>((uintptr_t)h.exp_noise)};
  s.busy[slot] = 1; s.prompt[slot] = h.pos - h.step; s.first_in[slot] = 0;
  return 0;
}

// ---- fork: further takes of a row that is already in the session (idxtts.h "Several takes of one request") ----
int GPTModel::session_fork(void* ws, int src, int at, int n, const int* dst_slots, const idxtts_sampling* samplers, const int* caps,
                           hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams == 0, "a beam session's rows cannot be forked: beams of a group are not independent requests");
  IDX_CHECK(dst_slots && n >= 1 && n < s.shape.slots, "fork to 1 .. slots - 1 destinations");
  IDX_CHECK(!samplers || s.shape.sampled, "a sampled take needs a session initialised with IDXTTS_SESSION_SAMPLED");
  IDX_CHECK(src >= 0 && src < s.shape.slots, "source slot out of range");
  IDX_CHECK(s.busy[src], "source slot holds no request");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  std::vector<char> taken(s.shape.slots, 0);
  for (int j = 0; j < n; ++j) {
    IDX_CHECK(dst_slots[j] >= 0 && dst_slots[j] < s.shape.slots, "destination slot out of range");
    IDX_CHECK(dst_slots[j] != src, "a destination is the source slot");
    IDX_CHECK(!s.busy[dst_slots[j]] && !taken[dst_slots[j]], "destination slot is not free");
    taken[dst_slots[j]] = 1;
  }
  if (samplers)
    for (int j = 0; j < n; ++j)
      if (check_sampling(samplers[j])) return 1;
  const SessionBuffers sb = carve_session(ws, s.shape);
  const Buffers& w = sb.w;
  const int V = cfg.number_mel_codes;
  SlotState hs;
  IDX_HIP(hipMemcpyAsync(&hs, w.slots + src, sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(hs.step >= 1 && hs.step <= hs.max_step && hs.max_step <= s.shape.max_new && hs.pos >= 1 && hs.pos <= w.Smax, "slot state corrupt");
  // a row that ended on the stop token has nothing behind it: a take may keep at most the codes in front of the stop token
  int most = hs.step;
  if (!hs.live) {
    long long last = 0;
    IDX_HIP(hipMemcpyAsync(&last, w.codes + (size_t)src * s.shape.max_new + hs.step - 1, sizeof(last), hipMemcpyDeviceToHost, st));
    IDX_HIP(hipStreamSynchronize(st));
    if (last == cfg.stop_mel_token) most = hs.step - 1;
  }
  if (at == -1) at = most;      // where the source stands now
  IDX_CHECK(at >= 0 && at <= most, "at out of range (0 .. the source's codes, the stop token not among them)");
  const int P = s.prompt[src];      // (an ended row's pos does not say: it stays behind when the row ends by itself, not when it is stopped)
  IDX_CHECK(P >= 1 && P <= s.shape.max_prompt && P + hs.step - 1 <= hs.pos && hs.pos <= P + hs.step, "slot state corrupt");
  IDX_CHECK(at > 0 || s.first_in[src], "at = 0 needs a source that still has its prefill output: a resumed row (and a take of one) does not");
  ForkArgs a;
  for (int j = 0; j < n; ++j) {
    const int cap = caps ? caps[j] : hs.max_step;
    IDX_CHECK(cap >= 1 && cap <= s.shape.max_new, "token cap out of range (1 .. max_new)");
    IDX_CHECK(cap > at, "a take's cap must leave it a code to produce (cap > at)");
    IDX_CHECK((long long)P + 1 + cap <= w.Smax, "the take does not fit the session's cache");
    a.dst[j] = (unsigned char)dst_slots[j]; a.cap[j] = cap;
  }
  GenScope gen_scope(this);
  a.kv_fmt = s.kv_fmt; a.layers = cfg.layers; a.heads = cfg.heads; a.V = V; a.start_token = cfg.start_mel_token;
  a.src = src; a.P = P; a.at = at; a.n = n;
  a.kcache = w.kcache; a.vcache = w.vcache; a.kscale = w.kscale; a.vscale = w.vscale;
  a.layer_bytes = kv_layer_bytes(s.shape.slots, w.Smax); a.layer_scales = kv_layer_scales(s.shape.slots, w.Smax);
  a.Smax = w.Smax; a.slots = w.slots; a.seen = w.seen; a.codes = w.codes; a.codes_ld = s.shape.max_new; a.cur_tok = w.cur_tok;
  a.x_last = sb.x_last; a.embed = tail_embed(w, use_pl(s.shape.slots)); a.B = s.shape.slots; a.logprobs = w.logprobs;
  if (session_fork_slots(a, st)) return 1;      // (its own checks come before its launch: from here on nothing refuses)
  if (s.shape.sampled) {      // the takes' samplers (greedy when samplers is null); the other rows are rewritten unchanged
    for (int j = 0; j < n; ++j) s.samp[dst_slots[j]] = slot_sampling(samplers ? samplers + j : nullptr);
    IDX_HIP(hipMemcpyAsync(sb.samp, s.samp.data(), s.shape.slots * sizeof(SlotSampling), hipMemcpyHostToDevice, st));
  }
  if (at == 0) {      // the takes' first token: the admission's head-and-sample pass on the destinations
    std::vector<int> ids(dst_slots, dst_slots + n);
    IDX_HIP(hipMemcpyAsync(sb.ids, ids.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipStreamSynchronize(st));      // the staging vector goes out of scope below
    if (session_first_tokens(s, sb, n, st)) return 1;
  }
  for (int j = 0; j < n; ++j) { s.busy[dst_slots[j]] = 1; s.prompt[dst_slots[j]] = P; s.first_in[dst_slots[j]] = s.first_in[src]; }
  return 0;
}

int GPTModel::latent(const float* emb, const int* pad_left_host, int B, int S, int mel_start, int M, float* latent_out, void* ws,
                     size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(emb && latent_out, "null pointer");
  IDX_CHECK(B > 0 && S > 0 && M > 0 && mel_start >= 0 && mel_start + M <= S, "shape");
  IDX_CHECK(ws && ws_bytes >= workspace_bytes(B, S, 0), "workspace too small");
  const int d = cfg.model_dim;
  Buffers w = carve(ws, B, S, 0);
  const int* kstart = nullptr;
  if (pad_left_host) {      // rows with shorter texts are left-padded; padded keys are masked exactly like the decode prompt
    for (int b = 0; b < B; ++b) IDX_CHECK(pad_left_host[b] >= 0 && pad_left_host[b] < mel_start, "pad_left out of range");
    IDX_HIP(hipMemcpyAsync(w.kstart, pad_left_host, B * sizeof(int), hipMemcpyHostToDevice, st));
    IDX_HIP(hipStreamSynchronize(st));
    kstart = w.kstart;
  }
  IDX_HIP(hipMemcpyAsync(w.x, emb, (size_t)B * S * d * sizeof(float), hipMemcpyDeviceToDevice, st));
  for (int li = 0; li < cfg.layers; ++li)
    if (layer_full(li, w, B, S, kstart, false, st)) return 1;
  RowsNormArgs n;     // final_norm(ln_f(h)) on the mel rows only (model_v2.py:611, 723)
  n.x_in = w.x + (size_t)mel_start * d; n.ld_in = d; n.in_rows_per_batch = M; n.in_batch_stride = (long)S * d;
  n.y = latent_out; n.ld_y = d; n.M = B * M; n.d = d; n.mode = NORM_LN_LN;
  n.g1 = lnf_g; n.b1 = lnf_b; n.g2 = fn_g; n.b2 = fn_b;
  return rows_norm_forward(n, st);
}

int GPTModel::embed(float* out, int rows, const int* text_ids, const int* text_pos_idx, const int* mel_ids, const int* mel_pos_idx,
                    const float* extra, const int* extra_idx, hipStream_t st) {
  GatherArgs ga;
  ga.out = out; ga.ld_out = cfg.model_dim; ga.d = cfg.model_dim;
  ga.table[0] = text_emb; ga.idx[0] = text_ids;
  ga.table[1] = text_pos; ga.idx[1] = text_pos_idx;
  ga.table[2] = mel_emb; ga.idx[2] = mel_ids;
  ga.table[3] = mel_pos; ga.idx[3] = mel_pos_idx;
  ga.table[4] = extra; ga.idx[4] = extra_idx;
  ga.table_rows[0] = cfg.number_text_tokens + 1; ga.table_rows[1] = cfg.text_pos_len;
  ga.table_rows[2] = cfg.number_mel_codes; ga.table_rows[3] = cfg.mel_pos_len;
  // one flag slot per call in flight: embed() runs concurrently on several streams (serving.BatchPipeline's lanes), and a shared
  // flag could be cleared by one call's memset before another call has read it
  int* const flag = oob_flag + (oob_next.fetch_add(1, std::memory_order_relaxed) % OOB_SLOTS);
  ga.oob = flag;
  IDX_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  if (gather_sum_rows(ga, rows, st)) return 1;
  int bad = 0;       // the reference's nn.Embedding raises IndexError on such an id (model_v2.py:759-760); fail as loudly
  IDX_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  static const char* names[] = {"", "text token id", "text position", "mel code", "mel position", "conditioning row"};
  if (bad) IDX_FAIL(std::string("embedding index out of range: ") + names[bad < 6 ? bad : 0]);
  return 0;
}

}  // namespace idxtts
