// extern "C" surface of libidxtts_hip (declared in include/idxtts.h).  Nothing here throws.
#include <cstring>
#include <new>

#include "../../include/idxtts.h"
#include "bigvgan.h"
#include "cond.h"
#include "semantic.h"
#include "codec.h"
#include "audio.h"
#include "campplus.h"
#include "conv1d.h"
#include "ctx.h"
#include "fbank.h"
#include "gpt.h"
#include "model_util.h"
#include "s2mel.h"

namespace idxtts {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(const char* file, int line, const std::string& msg) {
  const char* base = std::strrchr(file, '/');
  g_last_error = std::string(base ? base + 1 : file) + ":" + std::to_string(line) + ": " + msg;
  return 1;
}

}  // namespace idxtts

using namespace idxtts;

struct idxtts_conv1d {
  ConvWeights w;
  DeviceArena arena;
  int Cout = 0;
};

struct idxtts_linear {
  LinearWeights w;
  DeviceArena arena;
};

#define API_BEGIN try {
#define API_END                                                        \
  }                                                                    \
  catch (const std::exception& e) { return fail(__FILE__, __LINE__, std::string("exception: ") + e.what()); } \
  catch (...) { return fail(__FILE__, __LINE__, "unknown exception"); }

extern "C" {

int idxtts_version(void) { return 100; }

const char* idxtts_last_error(void) { return g_last_error.c_str(); }

int idxtts_aa_act_fwd(void* out, const void* in, const float* up_filter, const float* down_filter,
                      const float* log_alpha, const float* log_beta, int B, int C, int T, int dtype, void* stream) {
  API_BEGIN
  IDX_CHECK(dtype == IDXTTS_DTYPE_F32 || dtype == IDXTTS_DTYPE_F16 || dtype == IDXTTS_DTYPE_BF16, "dtype must be IDXTTS_DTYPE_F32 / F16 / BF16");
  IDX_CHECK(B >= 0 && C >= 0 && T >= 0, "negative shape");
  return aa_act_forward(out, in, up_filter, down_filter, log_alpha, log_beta, B, C, T, static_cast<hipStream_t>(stream), nullptr, 1, dtype);
  API_END
}

// copies `n` floats from a host-or-device pointer into a host vector
static int fetch(const float* src, size_t n, std::vector<float>* dst) {
  dst->resize(n);
  if (!n) return 0;
  const hipError_t e = hipMemcpy(dst->data(), src, n * sizeof(float), hipMemcpyDefault);      // host or device source
  if (e == hipErrorNoDevice) {       // no GPU in this process (host-side staging / tests): every pointer is a host pointer
    (void)hipGetLastError();
    memcpy(dst->data(), src, n * sizeof(float));
    return 0;
  }
  IDX_HIP(e);
  return 0;
}

int idxtts_conv1d_create(const float* weight, const float* bias, int Cout, int Cin, int K, int transposed_stride,
                         idxtts_conv1d** out) {
  API_BEGIN
  IDX_CHECK(weight && out, "null pointer");
  IDX_CHECK(Cout > 0 && Cin > 0 && K > 0 && transposed_stride >= 1, "bad shape");
  std::unique_ptr<idxtts_conv1d> c(new idxtts_conv1d());
  std::vector<float> hw, hb;
  if (fetch(weight, (size_t)Cout * Cin * K, &hw)) return 1;
  if (bias && fetch(bias, Cout, &hb)) return 1;
  c->Cout = Cout;
  if (make_conv_weights(c->arena, hw.data(), bias ? hb.data() : nullptr, Cout, Cin, K, transposed_stride, &c->w)) return 1;
  *out = c.release();
  return 0;
  API_END
}

int idxtts_conv1d_fwd(const idxtts_conv1d* conv, const float* x, float* y, const float* residual, int B, int T,
                      int dilation, int pad_left, int pad_mode, float scale, int accumulate, void* stream) {
  API_BEGIN
  IDX_CHECK(conv, "null handle");
  if (B == 0 || T == 0) return 0;
  ConvArgs a;
  a.x = x; a.y = y; a.res = residual; a.B = B; a.T = T; a.dil = dilation; a.pad_left = pad_left;
  a.pad_mode = pad_mode; a.scale = scale; a.accum = accumulate;
  return conv1d_forward(conv->w, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_conv1d_destroy(idxtts_conv1d* conv) {
  delete conv;
  return 0;
}

int idxtts_ctx_load_tensor(idxtts_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim) {
  API_BEGIN
  IDX_CHECK(ctx && name && shape, "null pointer");
  IDX_CHECK(!ctx->finalized, "context already finalized");
  IDX_CHECK(ndim >= 0 && ndim <= 8, "ndim");
  const std::string key(name);
  if (!ctx->model->accepts(key)) IDX_FAIL("unknown tensor name '" + key + "'");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const int64_t n = t.numel();
  IDX_CHECK(n >= 0, "negative numel");
  IDX_CHECK(n == 0 || data, "null data");
  if (fetch(data, (size_t)n, &t.data)) return 1;
  ctx->tensors[key] = std::move(t);
  return 0;
  API_END
}

int idxtts_ctx_finalize(idxtts_ctx* ctx) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(!ctx->finalized, "context already finalized");
  if (ctx->model->finalize(ctx->tensors, ctx->arena)) return 1;
  ctx->tensors.clear();
  ctx->finalized = true;
  return 0;
  API_END
}

int idxtts_ctx_get_tensor(idxtts_ctx* ctx, const char* name, float* host_out, size_t capacity) {
  API_BEGIN
  IDX_CHECK(ctx && name && host_out, "null pointer");
  IDX_CHECK(!ctx->finalized, "staged tensors are released by finalize");
  auto it = ctx->tensors.find(name);
  if (it == ctx->tensors.end()) IDX_FAIL(std::string("no staged tensor '") + name + "'");
  IDX_CHECK(capacity >= it->second.data.size(), "output buffer too small");
  std::copy(it->second.data.begin(), it->second.data.end(), host_out);
  return 0;
  API_END
}

int idxtts_ctx_destroy(idxtts_ctx* ctx) {
  delete ctx;
  return 0;
}

float idxtts_fp8_e4m3_decode(unsigned char code) { return fp8_e4m3_decode(code); }
unsigned char idxtts_fp8_e4m3_encode(float v) { return fp8_e4m3_encode(v); }

int idxtts_kv_fp8_quantize(const float* x, int n_vectors, unsigned char* codes, float* scales, void* stream) {
  API_BEGIN
  if (fp8_check_device_decode(nullptr) || fp8_check_device_encode(nullptr)) return 1;
  return kv_fp8_quantize(x, n_vectors, codes, scales, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_bigvgan_create(const idxtts_bigvgan_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new BigVGANModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

size_t idxtts_bigvgan_workspace_bytes(const idxtts_ctx* ctx, int B, int Tm) {
  if (!ctx || B <= 0 || Tm <= 0) return 0;
  auto* m = dynamic_cast<const BigVGANModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, Tm) : 0;
}

int idxtts_bigvgan_fwd(idxtts_ctx* ctx, const float* mel, float* wav, int B, int Tm, void* workspace,
                       size_t workspace_bytes, int clamp, int stage_idx, float* stage_out, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<BigVGANModel*>(ctx->model.get());
  IDX_CHECK(m, "not a BigVGAN context");
  IDX_CHECK(B >= 0 && Tm >= 0, "negative shape");
  return m->forward(mel, wav, B, Tm, workspace, workspace_bytes, clamp, stage_idx, stage_out, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_bigvgan_fwd_ragged(idxtts_ctx* ctx, const float* mel, const int* mel_lengths, float* wav, int B, int Tm, void* workspace,
                              size_t workspace_bytes, int clamp, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx && ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<BigVGANModel*>(ctx->model.get());
  IDX_CHECK(m, "not a BigVGAN context");
  IDX_CHECK(B >= 0 && Tm >= 0 && mel_lengths, "shape / lengths");
  return m->forward(mel, wav, B, Tm, workspace, workspace_bytes, clamp, 0, nullptr, static_cast<hipStream_t>(stream), mel_lengths);
  API_END
}


int idxtts_linear_create(const float* weight, const float* bias, int N, int K, int weight_is_kn, idxtts_linear** out) {
  API_BEGIN
  IDX_CHECK(weight && out && N > 0 && K > 0, "bad arguments");
  std::unique_ptr<idxtts_linear> l(new idxtts_linear());
  std::vector<float> hw, hb;
  if (fetch(weight, (size_t)N * K, &hw)) return 1;
  if (bias && fetch(bias, N, &hb)) return 1;
  // idxtts_linear_fwd(bf16x3 = 1) takes any shape and any M: the tile pack always, the planes where the LDS-DMA kernel takes the shape
  if (make_linear(l->arena, hw.data(), bias ? hb.data() : nullptr, N, K, {WP16_ALWAYS_MF16, weight_is_kn ? W_KN : W_NK, 0, true}, &l->w)) return 1;
  *out = l.release();
  return 0;
  API_END
}

int idxtts_linear_fwd(const idxtts_linear* lin, const float* x, int ldx, float* y, int ldy, const float* residual, int ldr, int M,
                      int act, int bf16x3, void* stream) {
  API_BEGIN
  IDX_CHECK(lin, "null handle");
  GemmArgs a;
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.res = residual; a.ldr = ldr; a.M = M; a.act = act;
  if (!bf16x3) return gemm_tn_forward(lin->w, a, static_cast<hipStream_t>(stream));
  LinearWeights w = lin->w;
  if (bf16x3 == 2) w.mf16 = false;      // the LDS-DMA kernel's 32x32x16 loop: what the GPT, conditioning and semantic weights run
  if (bf16x3 == 3) {                    // one bf16 MFMA per product: the LDS-DMA kernel's 16x16x32 loop only, whatever the switch says
    IDX_CHECK(w.planes16 && w.mf16 && M >= 256 && linear_takes_planes(w.N, w.K), "bf16x3 = 3 needs M >= 256 and a shape the LDS-DMA kernel takes (N >= 96, K % 16 == 0)");
    a.bf16_products = 1;
  } else {
    IDX_CHECK(bf16x3 == 1 || bf16x3 == 2, "bf16x3: 0 .. 3");
  }
  return gemm_bf16x3_forward(w, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_linear_destroy(idxtts_linear* lin) {
  delete lin;
  return 0;
}

// what the attention entry points share: pointers, strides, shape and mask of one call (each adds its own mode)
static AttnArgs attn_args(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                          long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                          int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale) {
  AttnArgs a;
  a.q = q; a.k = k; a.v = v; a.o = o;
  a.q_bs = q_batch_stride; a.k_bs = a.v_bs = kv_batch_stride; a.o_bs = o_batch_stride;
  a.q_ts = q_token_stride; a.k_ts = a.v_ts = kv_token_stride; a.o_ts = o_token_stride;
  a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.causal = causal; a.kstart = kstart; a.kend = kend; a.scale = scale;
  return a;
}

int idxtts_attention_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream) {
  API_BEGIN
  const AttnArgs a = attn_args(q, k, v, o, q_batch_stride, q_token_stride, kv_batch_stride, kv_token_stride, o_batch_stride,
                               o_token_stride, B, H, Sq, Sk, causal, kstart, kend, scale);
  return flash_attn_forward(a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_attention_relkey_fwd(const float* q, const float* k, const float* v, float* o, long batch_stride, int token_stride,
                                long o_batch_stride, int o_token_stride, int B, int H, int S, const int* kend, float scale,
                                const float* rel_key, int rel_left, int rel_right, int split_bf16, void* stream) {
  API_BEGIN
  IDX_CHECK(rel_key, "rel_key is null");
  AttnArgs a = attn_args(q, k, v, o, batch_stride, token_stride, batch_stride, token_stride, o_batch_stride, o_token_stride, B, H, S, S,
                         0, nullptr, kend, scale);
  a.rel_key = rel_key; a.rel_left = rel_left; a.rel_right = rel_right; a.split_bf16 = split_bf16 ? 1 : 0;
  return flash_attn_forward(a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_attention_bf16x3_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream) {
  API_BEGIN
  AttnArgs a = attn_args(q, k, v, o, q_batch_stride, q_token_stride, kv_batch_stride, kv_token_stride, o_batch_stride, o_token_stride,
                         B, H, Sq, Sk, causal, kstart, kend, scale);
  a.split_bf16 = 1;
  return flash_attn_forward(a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_attention_bf16_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream) {
  API_BEGIN
  AttnArgs a = attn_args(q, k, v, o, q_batch_stride, q_token_stride, kv_batch_stride, kv_token_stride, o_batch_stride, o_token_stride,
                         B, H, Sq, Sk, causal, kstart, kend, scale);
  a.split_bf16 = 2;
  return flash_attn_forward(a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_attention_planes_fwd(const void* planes, int Mrows, int ncols, int q_col, int k_col, int v_col, int T, int q_row0, int Sq, int B,
                                int H, const int* kend, float scale, float* o, long o_batch_stride, int o_token_stride, void* o_planes,
                                int one_product, void* stream) {
  API_BEGIN
  AttnPlanesArgs a;
  a.planes = planes; a.Mrows = Mrows; a.ncols = ncols; a.q_col = q_col; a.k_col = k_col; a.v_col = v_col;
  a.T = T; a.q_row0 = q_row0; a.Sq = Sq; a.B = B; a.H = H; a.kend = kend; a.scale = scale;
  a.o = o; a.o_bs = o_batch_stride; a.o_ts = o_token_stride; a.o_planes = o_planes;
  a.split_bf16 = one_product ? 2 : 1;
  return flash_attn_planes_forward(a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, int M, int d, float eps, void* stream) {
  API_BEGIN
  RowsNormArgs n;
  n.x_in = x; n.ld_in = d; n.y = y; n.ld_y = d; n.M = M; n.d = d; n.mode = NORM_LN; n.eps = eps; n.g1 = gamma; n.b1 = beta;
  return rows_norm_forward(n, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_create(const idxtts_gpt_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new GPTModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

int idxtts_gpt_quantize_weights(idxtts_ctx* ctx, int format) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(!ctx->finalized, "quantise before idxtts_ctx_finalize");
  auto* m = dynamic_cast<GPTModel*>(ctx->model.get());
  IDX_CHECK(m, "not a GPT context");
  return m->quantize_weights(ctx->tensors, format);
  API_END
}

int idxtts_gpt_set_kv_format(idxtts_ctx* ctx, int format) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(format == 0 || format == 1 || format == 2, "KV cache format: 0 (fp32), 1 (bf16) or 2 (scaled fp8)");
  auto* m = dynamic_cast<GPTModel*>(ctx->model.get());
  IDX_CHECK(m, "not a GPT context");
  // scaled fp8 needs a device whose conversions are OCP e4m3fn, both ways (as idxtts_gpt_quantize_weights(ctx, 2) does for decoding)
  if (format == 2 && (fp8_check_device_decode(nullptr) || fp8_check_device_encode(nullptr))) return 1;
  // a generation in flight has carved its workspace for the current format: switching under it would overrun the cache
  IDX_CHECK(m->kv_fmt == format || m->generating.load() == 0, "a generation is in flight on this context: switch the KV format between generations");
  m->kv_fmt = format;      // cached decode graphs carry the format in their key; workspace sizes follow idxtts_gpt_workspace_bytes
  return 0;
  API_END
}

int idxtts_gpt_get_kv_format(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->kv_fmt : -1;
}

int idxtts_gpt_set_batch_invariant(idxtts_ctx* ctx, int on) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(on == 0 || on == 1, "batch-invariant mode: 0 (off) or 1 (on)");
  auto* m = dynamic_cast<GPTModel*>(ctx->model.get());
  IDX_CHECK(m, "not a GPT context");
  // a generation in flight has chosen its kernels (and captured its step) for the current mode
  IDX_CHECK(m->batch_invariant == on || m->generating.load() == 0, "a generation is in flight on this context: switch the mode between generations");
  m->batch_invariant = on;      // cached decode graphs carry the mode in their key; a session keeps the mode it was initialised in
  return 0;
  API_END
}

int idxtts_gpt_get_batch_invariant(const idxtts_ctx* ctx) {
  if (!ctx) return -1;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->batch_invariant : -1;
}

int idxtts_gpt_graph_cache_entries(idxtts_ctx* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  auto* m = dynamic_cast<GPTModel*>(ctx->model.get());
  if (!m) return -1;
  std::lock_guard<std::mutex> l(m->graph_mu);
  return (int)m->graph_cache.size();
}

size_t idxtts_gpt_workspace_bytes(const idxtts_ctx* ctx, int B, int S, int max_new_tokens) {
  if (!ctx || B <= 0 || S <= 0 || max_new_tokens < 0 || !ctx->finalized) return 0;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, S, max_new_tokens) : 0;
}

#define GPT_MODEL(ctx)                                        \
  IDX_CHECK(ctx, "null ctx");                                 \
  IDX_CHECK(ctx->finalized, "context not finalized");         \
  auto* m = dynamic_cast<GPTModel*>(ctx->model.get());        \
  IDX_CHECK(m, "not a GPT context")

int idxtts_gpt_embed(idxtts_ctx* ctx, float* out, int rows, const int* text_ids, const int* text_pos_idx, const int* mel_ids,
                     const int* mel_pos_idx, const float* extra, const int* extra_idx, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->embed(out, rows, text_ids, text_pos_idx, mel_ids, mel_pos_idx, extra, extra_idx, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_generate(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                        float repetition_penalty, long long* codes, int* n_steps, float* logits_out, void* workspace,
                        size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, use_graph, static_cast<hipStream_t>(stream), GPTModel::GenerateCall{});
  API_END
}

int idxtts_gpt_generate_forced(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                               float repetition_penalty, const long long* forced_codes, long long* codes, int* n_steps, float* logits_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(forced_codes, "null forced_codes");
  GPTModel::GenerateCall call;
  call.forced = forced_codes;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, 0, static_cast<hipStream_t>(stream), call);
  API_END
}

int idxtts_gpt_generate_sampled(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps,
                                float* logits_out, void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(sampling, "null sampling configuration");
  GPTModel::GenerateCall call;
  call.sampling = sampling;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, use_graph, static_cast<hipStream_t>(stream), call);
  API_END
}

int idxtts_gpt_generate_takes(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                              float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps, float* logits_out,
                              void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  GPTModel::GenerateCall call;
  call.sampling = sampling; call.takes = takes;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, use_graph, static_cast<hipStream_t>(stream), call);
  API_END
}

int idxtts_gpt_generate_scored(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                               float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps, float* logprobs,
                               float* logits_out, void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(logprobs, "null logprobs");
  GPTModel::GenerateCall call;
  call.sampling = sampling; call.takes = takes; call.logprobs = logprobs;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, use_graph, static_cast<hipStream_t>(stream), call);
  API_END
}

int idxtts_gpt_generate_prefix(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                               float repetition_penalty, const idxtts_sampling* sampling, const long long* prefix, int k, int prefix_pos0,
                               long long* codes, int* n_steps, float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes,
                               int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  GPTModel::GenerateCall call;
  call.sampling = sampling; call.takes = takes; call.logprobs = logprobs;
  call.prefix.codes = prefix; call.prefix.k = k; call.prefix.pos0 = prefix_pos0;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, use_graph, static_cast<hipStream_t>(stream), call);
  API_END
}

int idxtts_gpt_generate_forced_scored(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                      float repetition_penalty, const long long* forced_codes, long long* codes, int* n_steps,
                                      float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(forced_codes && logprobs, "null forced_codes or logprobs");
  GPTModel::GenerateCall call;
  call.forced = forced_codes; call.logprobs = logprobs;
  return m->generate(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, codes, n_steps, logits_out, workspace,
                     workspace_bytes, 0, static_cast<hipStream_t>(stream), call);
  API_END
}

size_t idxtts_gpt_score_workspace_bytes(const idxtts_ctx* ctx, int B, int P, int n) {
  if (!ctx || B <= 0 || B > 64 || P <= 0 || n <= 0 || !ctx->finalized) return 0;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->score_workspace_bytes(B, P, n) : 0;
}

int idxtts_gpt_score(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, const long long* codes, const int* lens,
                     int n, int prefix_pos0, float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->score(inputs_embeds, pad_left, B, P, codes, lens, n, prefix_pos0, logprobs, logits_out, workspace, workspace_bytes,
                  static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_gpt_beam_workspace_bytes(const idxtts_ctx* ctx, int B, int num_beams, int S, int max_new_tokens) {
  if (!ctx || !ctx->finalized || B <= 0 || num_beams < 2 || S <= 0 || max_new_tokens <= 0) return 0;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->beam_workspace_bytes(B, num_beams, S, max_new_tokens) : 0;
}

int idxtts_gpt_generate_beam(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                             float repetition_penalty, const idxtts_beam* beam, long long* codes, int* n_steps, void* workspace,
                             size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->generate_beam(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, beam, codes, n_steps, workspace,
                          workspace_bytes, use_graph, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_generate_beam_nbest(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                   float repetition_penalty, const idxtts_beam* beam, int n_best, long long* codes, int* lens, float* scores,
                                   int* n_steps, void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(lens && scores, "null pointer");
  return m->generate_beam(inputs_embeds, pad_left, B, P, max_new_tokens, repetition_penalty, beam, codes, n_steps, workspace,
                          workspace_bytes, use_graph, static_cast<hipStream_t>(stream), n_best, lens, scores);
  API_END
}

int idxtts_beam_finalize_host(int num_beams, double length_penalty, int hyp_n, const double* hyp_score, const int* hyp_len,
                              const int* hyp_slot, const int* hyp_seq, int seq_ld, int done, const float* beam_scores, const int* seq,
                              int steps_done, int cap, int stop_token, int n_best, long long* codes, int* lens, float* scores) {
  API_BEGIN
  IDX_CHECK(hyp_score && hyp_len && hyp_slot && hyp_seq && beam_scores && seq && codes && lens && scores, "null pointer");
  IDX_CHECK(num_beams >= 2 && num_beams <= BEAM_MAX && hyp_n >= 0 && hyp_n <= num_beams && seq_ld >= 1, "shape");
  IDX_CHECK(steps_done >= 1 && steps_done <= seq_ld && cap >= steps_done && cap <= seq_ld, "steps_done <= cap <= seq_ld");
  IDX_CHECK(n_best >= 1 && n_best <= num_beams, "1 <= n_best <= num_beams");
  for (int q = 0; q < hyp_n; ++q)
    IDX_CHECK(hyp_slot[q] >= 0 && hyp_slot[q] <= BEAM_MAX && hyp_len[q] >= 0 && hyp_len[q] <= seq_ld, "hypothesis out of range");
  std::vector<BeamHyp> best(n_best);
  if (beam_finalize(num_beams, length_penalty, hyp_n, hyp_score, hyp_len, hyp_slot, hyp_seq, seq_ld, done != 0, beam_scores, seq, steps_done,
                    best.data(), n_best)) return 1;
  beam_fill_rows(best.data(), n_best, seq_ld, cap, stop_token, codes, lens, scores);
  return 0;
  API_END
}

// the shape a session entry point describes: its sizes, its IDXTTS_SESSION_* flags (0: none), its num_beams (0: no beam session)
static GPTModel::SessionShape session_shape(int slots, int max_prompt, int max_new_tokens, int flags, int num_beams) {
  GPTModel::SessionShape sh;
  sh.slots = slots; sh.max_prompt = max_prompt; sh.max_new = max_new_tokens; sh.num_beams = num_beams;
  sh.sampled = flags & IDXTTS_SESSION_SAMPLED; sh.scores = flags & IDXTTS_SESSION_SCORES; sh.prefix = flags & IDXTTS_SESSION_PREFIX;
  sh.prefix_scores = flags & IDXTTS_SESSION_PREFIX_SCORES;
  return sh;
}

size_t idxtts_gpt_session_workspace_bytes(const idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens) {
  return idxtts_gpt_session_workspace_bytes_ex(ctx, slots, max_prompt, max_new_tokens, 0);
}

int idxtts_gpt_session_init(idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, float repetition_penalty, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return idxtts_gpt_session_init_ex(ctx, slots, max_prompt, max_new_tokens, repetition_penalty, 0, workspace, workspace_bytes, stream);
}

size_t idxtts_gpt_session_workspace_bytes_ex(const idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, int flags) {
  if (!ctx || !ctx->finalized || slots <= 0 || slots > 64 || max_prompt <= 0 || max_new_tokens <= 0) return 0;
  if (flags & ~(IDXTTS_SESSION_SAMPLED | IDXTTS_SESSION_SCORES | IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_PREFIX_SCORES)) return 0;
  if ((flags & IDXTTS_SESSION_PREFIX_SCORES) && (~flags & (IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_SCORES))) return 0;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->session_workspace_bytes(session_shape(slots, max_prompt, max_new_tokens, flags, 0)) : 0;
}

int idxtts_gpt_session_init_ex(idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, float repetition_penalty, int flags,
                               void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(!(flags & ~(IDXTTS_SESSION_SAMPLED | IDXTTS_SESSION_SCORES | IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_PREFIX_SCORES)), "unknown session flags");
  return m->session_init(workspace, workspace_bytes, session_shape(slots, max_prompt, max_new_tokens, flags, 0), repetition_penalty,
                         static_cast<hipStream_t>(stream));
  API_END
}

// what every greedy / sampled admission entry point carries; each names the further fields it sets
static GPTModel::Admission admission(int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* slot_ids,
                                     const int* max_new_tokens) {
  GPTModel::Admission a;
  a.n = n; a.inputs_embeds = inputs_embeds; a.ld_rows = ld_rows; a.prompt_lens = prompt_lens; a.ids = slot_ids; a.caps = max_new_tokens;
  return a;
}

int idxtts_gpt_session_admit(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                             const int* slot_ids, const int* max_new_tokens, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_admit(workspace, admission(n, inputs_embeds, ld_rows, prompt_lens, slot_ids, max_new_tokens), static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_admit_sampled(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                     const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_row, void* workspace,
                                     void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(per_row, "null pointer");
  GPTModel::Admission a = admission(n, inputs_embeds, ld_rows, prompt_lens, slot_ids, max_new_tokens);
  a.per_row = per_row;
  return m->session_admit(workspace, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_admit_takes(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* takes,
                                   const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take, void* workspace,
                                   void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(takes, "null pointer");
  GPTModel::Admission a = admission(n, inputs_embeds, ld_rows, prompt_lens, slot_ids, max_new_tokens);
  a.per_row = per_take; a.takes = takes;
  return m->session_admit(workspace, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_admit_prefix(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* takes,
                                    const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take, const int* prefix_lens,
                                    const long long* prefix, const float* prefix_logprobs, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(prefix_lens, "null prefix_lens");
  GPTModel::Admission a = admission(n, inputs_embeds, ld_rows, prompt_lens, slot_ids, max_new_tokens);
  a.per_row = per_take; a.takes = takes; a.prefix_lens = prefix_lens; a.prefix = prefix; a.prefix_logprobs = prefix_logprobs;
  return m->session_admit(workspace, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_admit_prefix_scored(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                           const int* takes, const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take,
                                           const int* prefix_lens, const long long* prefix, const float* prefix_logprobs,
                                           const unsigned char* from_model, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(prefix_lens && from_model, "null prefix_lens or from_model");
  GPTModel::Admission a = admission(n, inputs_embeds, ld_rows, prompt_lens, slot_ids, max_new_tokens);
  a.per_row = per_take; a.takes = takes; a.prefix_lens = prefix_lens; a.prefix = prefix; a.prefix_logprobs = prefix_logprobs;
  a.from_model = from_model;
  return m->session_admit(workspace, a, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_fork(idxtts_ctx* ctx, int src_slot, int at, int n, const int* dst_slots, const idxtts_sampling* samplers,
                            const int* max_new_tokens, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_fork(workspace, src_slot, at, n, dst_slots, samplers, max_new_tokens, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_gpt_session_workspace_bytes_beam(const idxtts_ctx* ctx, int slots, int num_beams, int max_prompt, int max_new_tokens) {
  if (!ctx || !ctx->finalized || slots <= 0 || slots > 64 || max_prompt <= 0 || max_new_tokens <= 0) return 0;
  if (num_beams < 2 || num_beams > BEAM_MAX || slots % num_beams) return 0;
  auto* m = dynamic_cast<const GPTModel*>(ctx->model.get());
  return m ? m->session_workspace_bytes(session_shape(slots, max_prompt, max_new_tokens, 0, num_beams)) : 0;
}

int idxtts_gpt_session_init_beam(idxtts_ctx* ctx, int slots, int num_beams, int max_prompt, int max_new_tokens, float repetition_penalty,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  IDX_CHECK(num_beams >= 2 && num_beams <= BEAM_MAX, "2 <= num_beams <= 8");
  return m->session_init(workspace, workspace_bytes, session_shape(slots, max_prompt, max_new_tokens, 0, num_beams), repetition_penalty,
                         static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_admit_beam(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                  const int* group_ids, const int* max_new_tokens, const idxtts_beam* per_request, void* workspace,
                                  void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_admit_beam(workspace, n, inputs_embeds, ld_rows, prompt_lens, group_ids, max_new_tokens, per_request,
                               static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_step(idxtts_ctx* ctx, int n_steps, int use_graph, int* finished_slots, int* n_finished, void* workspace,
                            void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_step(workspace, n_steps, use_graph, finished_slots, n_finished, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_read(idxtts_ctx* ctx, int slot, long long* codes, int* n_codes, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_read(workspace, slot, codes, n_codes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_read_scored(idxtts_ctx* ctx, int slot, long long* codes, float* logprobs, int* n_codes, void* workspace,
                                   void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_read(workspace, slot, codes, n_codes, static_cast<hipStream_t>(stream), logprobs, true);
  API_END
}

int idxtts_gpt_session_read_nbest(idxtts_ctx* ctx, int slot, int n_best, long long* codes, int* lens, float* scores, void* workspace,
                                  void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_read_nbest(workspace, slot, n_best, codes, lens, scores, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_evict(idxtts_ctx* ctx, int n, const int* slots, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_end(workspace, n, slots, true, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_stop(idxtts_ctx* ctx, int n, const int* slots, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_end(workspace, n, slots, false, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_gpt_session_park_bytes(idxtts_ctx* ctx, int slot, void* workspace, void* stream) {
  auto* m = ctx && ctx->finalized ? dynamic_cast<GPTModel*>(ctx->model.get()) : nullptr;
  if (!m) { set_error("not a finalized GPT context"); return 0; }
  try {
    return m->session_park_bytes(workspace, slot, static_cast<hipStream_t>(stream));
  } catch (const std::exception& e) { set_error(std::string("exception: ") + e.what()); return 0; }
}

int idxtts_gpt_session_park(idxtts_ctx* ctx, int slot, void* dst, size_t dst_bytes, size_t* written, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_park(workspace, slot, dst, dst_bytes, written, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_resume(idxtts_ctx* ctx, int slot, const void* src, size_t src_bytes, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_resume(workspace, slot, src, src_bytes, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_gpt_session_park_group_bytes(idxtts_ctx* ctx, int group, void* workspace, void* stream) {
  auto* m = ctx && ctx->finalized ? dynamic_cast<GPTModel*>(ctx->model.get()) : nullptr;
  if (!m) { set_error("not a finalized GPT context"); return 0; }
  try {
    return m->session_park_group_bytes(workspace, group, static_cast<hipStream_t>(stream));
  } catch (const std::exception& e) { set_error(std::string("exception: ") + e.what()); return 0; }
}

int idxtts_gpt_session_park_group(idxtts_ctx* ctx, int group, void* dst, size_t dst_bytes, size_t* written, void* workspace,
                                  void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_park_group(workspace, group, dst, dst_bytes, written, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_resume_group(idxtts_ctx* ctx, int group, const void* src, size_t src_bytes, void* workspace, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_resume_group(workspace, group, src, src_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_gpt_session_release(idxtts_ctx* ctx, void* workspace) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->session_release(workspace);
  API_END
}

int idxtts_gpt_latent(idxtts_ctx* ctx, const float* emb, const int* pad_left, int B, int S, int mel_start, int M, float* latent,
                      void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  GPT_MODEL(ctx);
  return m->latent(emb, pad_left, B, S, mel_start, M, latent, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}


int idxtts_cond_create(const idxtts_cond_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new CondModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

size_t idxtts_cond_workspace_bytes(const idxtts_ctx* ctx, int B, int T) {
  if (!ctx || !ctx->finalized || B <= 0 || T < 3) return 0;
  auto* m = dynamic_cast<const CondModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, T) : 0;
}

int idxtts_cond_forward(idxtts_ctx* ctx, const float* feats, const int* lengths, int B, int T, float* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<CondModel*>(ctx->model.get());
  IDX_CHECK(m, "not a conditioning-encoder context");
  return m->forward(feats, lengths, B, T, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_cond_forward_rows(idxtts_ctx* ctx, const float* feats, const int* lengths, const int* extents, int B, int T, float* out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<CondModel*>(ctx->model.get());
  IDX_CHECK(m, "not a conditioning-encoder context");
  IDX_CHECK(extents, "null extents");
  return m->forward(feats, lengths, B, T, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), extents);
  API_END
}

int idxtts_w2vbert_create(const idxtts_w2vbert_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new W2VBertModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

size_t idxtts_w2vbert_workspace_bytes(const idxtts_ctx* ctx, int B, int T) {
  if (!ctx || !ctx->finalized || B <= 0 || T <= 0) return 0;
  auto* m = dynamic_cast<const W2VBertModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, T) : 0;
}

int idxtts_w2vbert_forward(idxtts_ctx* ctx, const float* feats, const int* lengths, int B, int T, float* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<W2VBertModel*>(ctx->model.get());
  IDX_CHECK(m, "not a w2v-bert context");
  return m->forward(feats, lengths, B, T, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_repcodec_create(const idxtts_repcodec_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new RepCodecModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

size_t idxtts_repcodec_workspace_bytes(const idxtts_ctx* ctx, int B, int T) {
  if (!ctx || !ctx->finalized || B <= 0 || T <= 0) return 0;
  auto* m = dynamic_cast<const RepCodecModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, T) : 0;
}

int idxtts_repcodec_quantize(idxtts_ctx* ctx, const float* x, int B, int T, long long* indices, float* quantized, void* workspace,
                             size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<RepCodecModel*>(ctx->model.get());
  IDX_CHECK(m, "not a semantic-codec context");
  return m->quantize(x, B, T, indices, quantized, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_melspec_create(const idxtts_melspec_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new MelSpecModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

int idxtts_melspec_frames(const idxtts_ctx* ctx, int n_samples) {
  if (!ctx || n_samples <= 0) return 0;
  auto* m = dynamic_cast<const MelSpecModel*>(ctx->model.get());
  return m ? m->frames(n_samples) : 0;
}

size_t idxtts_melspec_workspace_bytes(const idxtts_ctx* ctx, int B, int n_samples) {
  if (!ctx || !ctx->finalized || B <= 0 || n_samples <= 0) return 0;
  auto* m = dynamic_cast<const MelSpecModel*>(ctx->model.get());
  return m ? m->workspace_bytes(B, n_samples) : 0;
}

int idxtts_melspec_forward(idxtts_ctx* ctx, const float* audio, int B, int n_samples, float* mel, void* workspace, size_t workspace_bytes,
                           void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<MelSpecModel*>(ctx->model.get());
  IDX_CHECK(m, "not a mel-spectrogram context");
  return m->forward(audio, B, n_samples, mel, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_fbank_create(const idxtts_fbank_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new FbankModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

int idxtts_fbank_frames(const idxtts_ctx* ctx, int n_samples) {
  if (!ctx || n_samples <= 0) return 0;
  auto* m = dynamic_cast<const FbankModel*>(ctx->model.get());
  return m && m->cfg.frame_length > 0 && m->cfg.hop_length > 0 ? m->frames(n_samples) : 0;
}

size_t idxtts_fbank_workspace_bytes(const idxtts_ctx* ctx, const int* n_samples, int B) {
  if (!ctx || !ctx->finalized || !n_samples || B <= 0) return 0;
  auto* m = dynamic_cast<const FbankModel*>(ctx->model.get());
  return m ? m->workspace_bytes(n_samples, B) : 0;
}

int idxtts_fbank_forward(idxtts_ctx* ctx, const float* audio, int ld_audio, const int* n_samples, int B, float scale, int mode, float* out,
                         int T_out, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<FbankModel*>(ctx->model.get());
  IDX_CHECK(m, "not a filter-bank context");
  return m->forward(audio, ld_audio, n_samples, B, scale, mode, out, T_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_resample_forward(const float* kernel_t, int orig, int new_rate, int width, const float* x, int ldx, const int* lengths, int B,
                            float* out, int ldo, void* stream) {
  API_BEGIN
  return resample_forward(kernel_t, orig, new_rate, width, x, ldx, lengths, B, out, ldo, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_campplus_create(const idxtts_campplus_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new CamPPlusModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

size_t idxtts_campplus_workspace_bytes(const idxtts_ctx* ctx, int T) {
  if (!ctx || !ctx->finalized || T < 8) return 0;
  auto* m = dynamic_cast<const CamPPlusModel*>(ctx->model.get());
  return m ? m->workspace_bytes(T) : 0;
}

int idxtts_campplus_forward(idxtts_ctx* ctx, const float* feat, int B, int T, float* style, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  IDX_CHECK(ctx, "null ctx");
  IDX_CHECK(ctx->finalized, "context not finalized");
  auto* m = dynamic_cast<CamPPlusModel*>(ctx->model.get());
  IDX_CHECK(m, "not a CAMPPlus context");
  return m->forward(feat, B, T, style, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_emovec_merge(float* out, const float* base, const float* emo, float alpha, size_t n, void* stream) {
  API_BEGIN
  return lerp_rows(out, base, emo, alpha, n, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_s2mel_create(const idxtts_s2mel_config* cfg, idxtts_ctx** out) {
  API_BEGIN
  IDX_CHECK(cfg && out, "null pointer");
  std::unique_ptr<idxtts_ctx> ctx(new idxtts_ctx());
  ctx->model.reset(new S2MelModel(*cfg));
  *out = ctx.release();
  return 0;
  API_END
}

#define S2MEL_MODEL(ctx)                                      \
  IDX_CHECK(ctx, "null ctx");                                 \
  IDX_CHECK(ctx->finalized, "context not finalized");         \
  auto* m = dynamic_cast<S2MelModel*>(ctx->model.get());      \
  IDX_CHECK(m, "not an s2mel context")

size_t idxtts_s2mel_cond_workspace_bytes(const idxtts_ctx* ctx, int B, int M, int Tg) {
  if (!ctx || !ctx->finalized || B <= 0 || M <= 0 || Tg <= 0) return 0;
  auto* m = dynamic_cast<const S2MelModel*>(ctx->model.get());
  return m ? m->cond_workspace_bytes(B, M, Tg) : 0;
}

int idxtts_s2mel_prepare_cond(idxtts_ctx* ctx, const float* latent, const long long* codes, const int* code_lens,
                              const int* target_lens, int B, int M, int Tg, float* cond_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->prepare_cond(latent, codes, code_lens, target_lens, B, M, Tg, cond_out, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_s2mel_regulate(idxtts_ctx* ctx, const float* S, const int* in_lens, const int* target_lens, int B, int M, int Tg, float* cond_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->regulate(S, in_lens, target_lens, B, M, Tg, cond_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_s2mel_cfm_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int n_steps) {
  if (!ctx || !ctx->finalized || B <= 0 || T <= 0 || n_steps <= 0) return 0;
  auto* m = dynamic_cast<const S2MelModel*>(ctx->model.get());
  return m ? m->cfm_workspace_bytes(B, T, n_steps) : 0;
}

int idxtts_s2mel_cfm(idxtts_ctx* ctx, const float* mu, const int* x_lens, const float* prompt, const int* prompt_lens, int Tp_max,
                     const float* style, const float* z, const float* t_emb, const float* dt, int n_steps, float cfg_rate,
                     float* out, int B, int T, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->cfm(mu, x_lens, prompt, prompt_lens, Tp_max, style, z, t_emb, dt, n_steps, cfg_rate, out, B, T, workspace,
                workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_s2mel_cfm_rows_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int Tp_max, int n_steps) {
  if (!ctx || !ctx->finalized || B <= 0 || T <= 0 || Tp_max <= 0 || n_steps <= 0) return 0;
  auto* m = dynamic_cast<const S2MelModel*>(ctx->model.get());
  return m ? m->cfm_rows_workspace_bytes(B, T, Tp_max, n_steps) : 0;
}

int idxtts_s2mel_cfm_rows(idxtts_ctx* ctx, const float* gen_cond, const int* target_lens, int Tg_max, const float* const* prompt_conditions,
                          const float* const* ref_mels, const int* prompt_lens, const float* style, const float* z, const float* t_emb,
                          const float* dt, int n_steps, float cfg_rate, float* out, int B, int T, void* workspace, size_t workspace_bytes,
                          void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->cfm_rows(gen_cond, target_lens, Tg_max, prompt_conditions, ref_mels, prompt_lens, style, z, t_emb, dt, n_steps, cfg_rate, out,
                     B, T, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

size_t idxtts_s2mel_cfm_sched_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int Tp_max, int n_sched, const int* sched_steps) {
  if (!ctx || !ctx->finalized) return 0;
  auto* m = dynamic_cast<const S2MelModel*>(ctx->model.get());
  return m ? m->cfm_sched_workspace_bytes(B, T, Tp_max, n_sched, sched_steps) : 0;
}

int idxtts_s2mel_cfm_sched(idxtts_ctx* ctx, const float* gen_cond, const int* target_lens, int Tg_max, const float* const* prompt_conditions,
                           const float* const* ref_mels, const int* prompt_lens, const float* style, const float* z, int n_sched,
                           const int* sched_steps, const float* t_emb, const float* dt, const int* row_sched, const float* cfg_rates,
                           float* out, int B, int T, void* workspace, size_t workspace_bytes, void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->cfm_sched(gen_cond, target_lens, Tg_max, prompt_conditions, ref_mels, prompt_lens, style, z, n_sched, sched_steps, t_emb, dt,
                      row_sched, cfg_rates, out, B, T, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END
}

int idxtts_s2mel_estimator(idxtts_ctx* ctx, const float* x, const float* prompt, const int* prompt_lens, int Tp_max, const int* x_lens,
                           const float* t_emb, const float* style, const float* mu, float* out, int B, int T, void* workspace,
                           size_t workspace_bytes, void* stream) {
  API_BEGIN
  S2MEL_MODEL(ctx);
  return m->estimator(x, prompt, prompt_lens, Tp_max, x_lens, t_emb, style, mu, out, B, T, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
  API_END
}


int idxtts_set_gemm_mode(int mode) {
  set_gemm_mode(mode);
  return 0;
}

int idxtts_get_gemm_mode(void) { return get_gemm_mode(); }

int idxtts_set_acoustic_bf16(int on) {
  set_acoustic_bf16(on);
  return 0;
}

int idxtts_get_acoustic_bf16(void) { return get_acoustic_bf16(); }

int idxtts_set_decode_geometry(int narrow) {
  set_decode_geometry(narrow);
  return 0;
}

int idxtts_get_decode_geometry(void) { return get_decode_geometry(); }

int idxtts_release_stream(void* stream) {
  API_BEGIN
  hipStream_t st = static_cast<hipStream_t>(stream);
  return gemm_release_stream_scratch(st) || s2mel_release_stream(st);
  API_END
}

int idxtts_set_decode_plane_rows(int min_rows) {
  API_BEGIN
  IDX_CHECK(min_rows == 0 || (min_rows >= 5 && min_rows <= 65), "0 (default), 5..64 or 65 (off)");
  set_decode_plane_rows(min_rows);
  return 0;
  API_END
}

int idxtts_get_decode_plane_rows(void) { return get_decode_plane_rows(); }

int idxtts_gemv_fx_plan_query(int N, int K, int rows, int format, int with_slab, int narrow, idxtts_gemv_fx_plan* out) {
  API_BEGIN
  IDX_CHECK(out && N > 0 && K > 0 && rows > 0 && rows <= 64, "N, K > 0, 1..64 rows");
  IDX_CHECK(format == WFMT_F32 || format == WFMT_BF16 || format == WFMT_FP8, "weight format 0..2");
  const int ksb = with_slab ? gemv_fx_ksb(N, K) : 1;
  const FxPlan pl = gemv_fx_make_plan(N, K, rows, format, ksb, narrow != 0);
  out->mt = pl.MT; out->ntw = pl.ntw; out->single = pl.single; out->r4 = pl.r4; out->narrow = pl.narrow;
  out->kw = pl.kw; out->cps = pl.cps; out->ksb = ksb;
  return 0;
  API_END
}

int idxtts_batch_invariant_plan_query(int N, int K, int rows, int format, int with_slab, int B, int heads, int smax, int n_keys,
                                      idxtts_batch_invariant_plan* out) {
  API_BEGIN
  IDX_CHECK(out && N > 0 && K > 0 && rows > 0 && rows <= 64, "N, K > 0, 1..64 rows");
  IDX_CHECK(format == WFMT_F32 || format == WFMT_BF16 || format == WFMT_FP8, "weight format 0..2");
  IDX_CHECK(B > 0 && B <= 64 && heads > 0 && n_keys > 0 && smax >= n_keys, "1..64 attention rows, 1 <= n_keys <= smax");
  const int ksb = with_slab ? gemv_fx_ksb(N, K) : 1;
  // the switches as they stand: the plan must not read them
  const FxPlan pl = gemv_fx_make_plan(N, K, rows, format, ksb, get_decode_geometry() != 0, true);
  out->family = 0; out->r4 = pl.r4; out->narrow = pl.narrow; out->kw = pl.kw; out->cps = pl.cps; out->ksb = ksb;
  out->mt = pl.MT; out->ntw = pl.ntw; out->single = pl.single;
  const int np = decode_attn_pieces(n_keys);
  out->attn_pieces = np;
  out->attn_piece_keys = np > 1 ? ((n_keys + np - 1) / np + 15) & ~15 : n_keys;
  out->attn_workgroups = std::min(decode_attn_inv_wgs(B, heads, smax), np);
  return 0;
  API_END
}

// Instrument: kv_store_prefill / kv_store_slots and one decode_attn_forward step on caller-owned buffers (idxtts.h).  Workspace: the
// arrival counters [rows * heads], the partial results [rows * heads][16][66] -- both as GPTModel::carve sizes them -- and a DecodeState
static size_t probe_pad(size_t n) { return (n + 255) & ~(size_t)255; }
size_t idxtts_decode_attn_probe_workspace_bytes(int heads, int rows) {
  if (heads < 1 || rows < 1) return 0;
  const size_t rh = (size_t)rows * heads;
  return probe_pad(rh * sizeof(unsigned)) + probe_pad(rh * 16 * 66 * sizeof(float)) + probe_pad(sizeof(DecodeState));
}

int idxtts_decode_attn_probe_run(idxtts_decode_attn_probe* p, void* stream) {
  API_BEGIN
  IDX_CHECK(p, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int H = p->heads, B = p->rows, Smax = p->smax, d = 64 * H;
  IDX_CHECK(H >= 1 && B >= 1 && B <= 64 && Smax >= 1, "heads >= 1, 1..64 rows, smax >= 1");
  IDX_CHECK(p->kv_format >= 0 && p->kv_format <= 2, "KV format 0 / 1 / 2");
  IDX_CHECK(p->kcache && p->vcache && (p->kv_format != 2 || (p->kscale && p->vscale)), "null cache pointer");
  IDX_CHECK(p->workspace && ((uintptr_t)p->workspace & 255) == 0 && p->workspace_bytes >= idxtts_decode_attn_probe_workspace_bytes(H, B),
            "workspace: idxtts_decode_attn_probe_workspace_bytes, 256-byte aligned");
  if (p->kv_format == 2 && (fp8_check_device_decode(nullptr) || fp8_check_device_encode(nullptr))) return 1;
  KvDst kv;
  kv.kcache = p->kcache; kv.vcache = p->vcache; kv.fmt = p->kv_format;
  if (p->kv_format == 2) { kv.kscale = p->kscale; kv.vscale = p->vscale; }
  std::vector<int> host;      // every index the kernels will follow is checked here: the buffers are the caller's
  auto fetch_ints = [&](const int* src, size_t n) {
    host.resize(n);
    return hipMemcpy(host.data(), src, n * sizeof(int), hipMemcpyDeviceToHost);
  };
  if (p->S > 0) {
    IDX_CHECK(p->qkv && p->n >= 1 && p->S <= Smax, "store: qkv, n >= 1, S <= smax");
    if (!p->slot_ids) {
      IDX_CHECK(p->n == B, "kv_store_prefill fills every cache row: n == rows");
      if (kv_store_prefill(p->qkv, kv, B, H, p->S, Smax, d, st)) return 1;
    } else {
      IDX_CHECK(p->len && p->fan >= 1, "kv_store_slots: len, fan >= 1");
      IDX_HIP(fetch_ints(p->slot_ids, p->n));
      for (int b = 0; b < p->n; ++b) IDX_CHECK(host[b] >= 0 && host[b] + p->fan <= B, "slot_ids: a slot outside the cache rows");
      IDX_HIP(fetch_ints(p->len, p->n));
      for (int b = 0; b < p->n; ++b) IDX_CHECK(host[b] >= 0 && host[b] <= p->S, "len: 0..S");
      if (kv_store_slots(p->qkv, kv, p->n, H, p->S, Smax, d, p->slot_ids, p->len, st, p->fan)) return 1;
    }
  }
  IDX_CHECK(p->step_qkv && p->out && p->kstart, "step: step_qkv, out, kstart");
  IDX_HIP(fetch_ints(p->kstart, B));
  const std::vector<int> ks = host;
  if (p->slot_state) {
    static_assert(sizeof(SlotState) == 5 * sizeof(int), "slot_state rows are SlotStates");
    IDX_HIP(fetch_ints(p->slot_state, (size_t)B * 5));
    for (int b = 0; b < B; ++b)
      IDX_CHECK(!host[5 * b + 4] || (ks[b] >= 0 && ks[b] <= host[5 * b] && host[5 * b] < Smax), "a live slot needs 0 <= kstart <= pos < smax");
  } else {
    for (int b = 0; b < B; ++b) IDX_CHECK(ks[b] >= 0 && ks[b] <= p->pos && p->pos < Smax, "0 <= kstart <= pos < smax");
  }
  const size_t rh = (size_t)B * H;
  char* ws = static_cast<char*>(p->workspace);
  unsigned* cnt = reinterpret_cast<unsigned*>(ws);
  float* part = reinterpret_cast<float*>(ws + probe_pad(rh * sizeof(unsigned)));
  DecodeState* state = reinterpret_cast<DecodeState*>(ws + probe_pad(rh * sizeof(unsigned)) + probe_pad(rh * 16 * 66 * sizeof(float)));
  IDX_HIP(hipMemsetAsync(cnt, 0, rh * sizeof(unsigned), st));
  const DecodeState hs = {p->pos, 0, 0, 0u};
  IDX_HIP(hipMemcpyAsync(state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
  DecodeAttnArgs da;      // GPTModel::attn_args
  da.qkv_part = p->step_qkv; da.parts = 1; da.part_rows = B; da.qkv_bias = nullptr;
  da.kcache = kv.kcache; da.vcache = kv.vcache; da.kv_fmt = kv.fmt; da.kscale = kv.kscale; da.vscale = kv.vscale; da.kstart = p->kstart;
  da.st = state; da.B = B; da.H = H; da.Smax = Smax; da.d = d; da.scale = 0.125f;
  da.nsplit = decode_attn_nsplit(B, H); da.part = part; da.cnt = cnt; da.slot = reinterpret_cast<const SlotState*>(p->slot_state);
  if (p->invariant) { da.invariant = 1; da.nsplit = decode_attn_inv_wgs(B, H, Smax); }
  if (p->nsplit) {
    IDX_CHECK(p->nsplit >= 1 && p->nsplit <= 16, "nsplit: 0 (the rule) or 1..16");
    da.nsplit = p->nsplit;
  }
  (p->out_frag ? da.out : da.out_row) = p->out;
  p->nsplit_used = da.nsplit;
  if (decode_attn_forward(da, st)) return 1;
  IDX_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int idxtts_gemv_pl_plan_query(int N, int K, int rows, int* ct, int* kparts, int* has_kernel) {
  API_BEGIN
  IDX_CHECK(ct && kparts && has_kernel && N > 0 && K > 0 && rows > 0 && rows <= 64, "N, K > 0, 1..64 rows");
  gemv_pl_plan(N, K, rows, ct, kparts);
  *has_kernel = gemv_pl_can_run(N, K, rows) ? 1 : 0;
  return 0;
  API_END
}

int idxtts_s2mel_set_overlap(int on) {
  set_s2mel_overlap(on);
  return 0;
}

int idxtts_s2mel_get_overlap(void) { return get_s2mel_overlap(); }

}  // extern "C"
