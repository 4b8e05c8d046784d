// Weight staging and the small models' per-layer launches (model_util.h).
#include "model_util.h"

#include <cstring>

#include "norm.h"

namespace idxtts {

int need(std::map<std::string, HostTensor>& t, const std::string& key, std::vector<int64_t> shape, HostTensor** out) {
  auto it = t.find(key);
  if (it == t.end()) IDX_FAIL("missing tensor '" + key + "'");
  if (it->second.shape != shape) {
    std::string s = "tensor '" + key + "' has shape [";
    for (auto d : it->second.shape) s += std::to_string(d) + ",";
    s += "] expected [";
    for (auto d : shape) s += std::to_string(d) + ",";
    IDX_FAIL(s + "]");
  }
  *out = &it->second;
  return 0;
}

int up(DeviceArena& arena, const std::vector<float>& v, const float** out) {
  float* d = nullptr;
  if (arena.upload(v.data(), v.size(), &d)) return 1;
  *out = d;
  return 0;
}

int tensor_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& key, std::vector<int64_t> shape, const float** out) {
  HostTensor* h = nullptr;
  if (need(t, key, shape, &h)) return 1;
  return up(arena, h->data, out);
}

int vec_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& key, int n, const float** out) {
  return tensor_from(t, arena, key, {n}, out);
}

int ln_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& prefix, int n, const float** g, const float** b) {
  return vec_from(t, arena, prefix + ".weight", n, g) || vec_from(t, arena, prefix + ".bias", n, b);
}

int make_linear(DeviceArena& arena, const float* w, const float* bias, int N, int K, const LinearOpts& o, LinearWeights* out) {
  const int Kpad = o.Kpad ? o.Kpad : K;
  IDX_CHECK(Kpad >= K, "Kpad < K");
  std::vector<float> rows;      // [N][Kpad], where the source is not that already
  if (o.layout == W_KN || Kpad != K) {
    rows.assign((size_t)N * Kpad, 0.0f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) rows[(size_t)n * Kpad + k] = o.layout == W_KN ? w[(size_t)k * N + n] : w[(size_t)n * K + k];
    w = rows.data();
  }
  std::vector<float> packed(linear_packed_floats(N, Kpad));
  pack_linear(packed.data(), w, N, Kpad);
  if (up(arena, packed, &out->wp)) return 1;
  out->N = N; out->K = Kpad;
  out->mf16 = o.wp16 == WP16_ALWAYS_MF16;
  auto pack16 = [&](size_t bytes, void (*pack)(void*, const float*, int, int), const void** dst) {
    std::vector<float> p16((bytes + 3) / 4);
    pack(p16.data(), w, N, Kpad);
    const float* d16 = nullptr;
    if (up(arena, p16, &d16)) return 1;
    *dst = d16;
    return 0;
  };
  const bool planes = o.wp16 != WP16_NONE && linear_takes_planes(N, Kpad);
  const bool tiles = o.wp16 != WP16_NONE && (o.split_bf16_below_256_rows || (o.wp16 != WP16_DMA_SHAPES && !planes));
  if (planes && pack16(linear_planes_bytes(N, Kpad), pack_linear_planes, &out->planes16)) return 1;
  if (tiles && pack16(linear_tiles_bytes(N, Kpad), pack_linear_tiles, &out->tiles16)) return 1;
  if (bias && up(arena, std::vector<float>(bias, bias + N), &out->bias)) return 1;
  return 0;
}

int linear_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& prefix, int N, int K, bool bias, Wp16Policy wp16,
                LinearWeights* out, std::vector<int64_t> wshape) {
  HostTensor *w = nullptr, *b = nullptr;
  if (wshape.empty()) wshape = {N, K};
  if (need(t, prefix + ".weight", wshape, &w)) return 1;
  if (bias && need(t, prefix + ".bias", {N}, &b)) return 1;
  return make_linear(arena, w->data.data(), b ? b->data.data() : nullptr, N, K, {wp16, W_NK, (K + 3) & ~3}, out);
}

static GemmArgs lin_args(const float* x, int ldx, float* y, int ldy, int M, int act, const float* res, int ldr) {
  GemmArgs g;
  g.x = x; g.ldx = ldx; g.y = y; g.ldy = ldy; g.M = M; g.act = act; g.res = res; g.ldr = ldr;
  return g;
}

int lin(const LinearWeights& w, const float* x, int ldx, float* y, int ldy, int M, hipStream_t st, int act, const float* res, int ldr) {
  const GemmArgs g = lin_args(x, ldx, y, ldy, M, act, res, ldr);
  if (act == ACT_GELU_ERF || act == ACT_RELU) return gemm_tn_forward(w, g, st);      // (activations only the exact kernel's epilogue has)
  return gemm_forward(w, g, st);
}

int lin_exact(const LinearWeights& w, const float* x, int ldx, float* y, int ldy, int M, hipStream_t st, int act, const float* res, int ldr) {
  return gemm_tn_forward(w, lin_args(x, ldx, y, ldy, M, act, res, ldr), st);
}

int layer_norm(const float* x, float* y, const float* g, const float* b, int M, int d, hipStream_t st) {
  RowsNormArgs n;
  n.x_in = x; n.ld_in = d; n.y = y; n.ld_y = d; n.M = M; n.d = d; n.mode = NORM_LN; n.eps = 1e-5f; n.g1 = g; n.b1 = b;
  return rows_norm_forward(n, st);
}

}  // namespace idxtts
