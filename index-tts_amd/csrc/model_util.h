// Shared by every model's finalize(): staged host tensors -> device weights (the exact-fp32 MFMA GEMM pack, the split-bf16 packs),
// workspace carving, and the two launches every layer of the small once-per-prompt models repeats.  Definitions: model_util.hip.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "ctx.h"
#include "gemm.h"

namespace idxtts {

// the staged tensor `key`, which must have `shape`
int need(std::map<std::string, HostTensor>& t, const std::string& key, std::vector<int64_t> shape, HostTensor** out);
int up(DeviceArena& arena, const std::vector<float>& v, const float** out);
// need + up: a tensor that goes to the device as it is (vec_from: a vector of n)
int tensor_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& key, std::vector<int64_t> shape, const float** out);
int vec_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& key, int n, const float** out);
int ln_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& prefix, int n, const float** g, const float** b);

// Which linears get a split-bf16 pack beside the fp32 one.  gemm_forward runs a launch of >= 256 rows on the split-bf16 kernel of its
// shape (linear_takes_planes, gemm.h) when the weights carry that kernel's pack, and on the exact fp32 kernel when they do not.  A
// pack is made only where that dispatch can read it: planes for the shapes the LDS-DMA kernel takes, tiles for the others.
enum Wp16Policy {
  WP16_ALWAYS,      // every shape: the GPT projections (N < 96 or K % 16 != 0 get tiles and run on the tile kernel)
  WP16_DMA_SHAPES,  // only shapes the LDS-DMA kernel takes (N >= 96, K % 16 == 0), the rest stays exact fp32: the small models
  // every shape, and the LDS-DMA kernel's v_mfma_f32_16x16x32_bf16 loop (LinearWeights::mf16): s2mel and idxtts_linear_create.  That
  // loop adds a row's k in another order than the 32x32x16 loop, so results move in the last bits.  Where they only become a waveform
  // that is rounding; a GPT prefill into a bf16 cache, the conditioning and the semantic models feed a choice of discrete codes, where
  // a last bit can flip a near-tie and change the whole utterance: those keep the sums they have always had.
  WP16_ALWAYS_MF16,
  WP16_NONE,        // no split-bf16 pack: weights only lin_exact ever reads (the filter bank's DFT and mel matrices)
};
enum WeightLayout { W_NK /* torch nn.Linear [N][K] */, W_KN /* HF Conv1D [K][N] (y = x @ W + b) */ };
struct LinearOpts {
  Wp16Policy wp16;
  WeightLayout layout = W_NK;
  int Kpad = 0;      // K of the packed weights, >= K: zero columns are added (0: K as it is)
  // launches below 256 rows also run split-bf16 (idxtts_linear_fwd calls gemm_bf16x3_forward at any M): tiles for every shape
  bool split_bf16_below_256_rows = false;
};
// host weights (+ bias [N] or null) -> the fp32 pack and the split-bf16 packs of the policy, on the device
int make_linear(DeviceArena& arena, const float* w, const float* bias, int N, int K, const LinearOpts& o, LinearWeights* out);
// the nn.Linear `prefix`.weight [N][K] (or `wshape`, a 1-tap Conv1d's [N][K][1]) + `prefix`.bias; K is padded to a multiple of 4
int linear_from(std::map<std::string, HostTensor>& t, DeviceArena& arena, const std::string& prefix, int N, int K, bool bias, Wp16Policy wp16,
                LinearWeights* out, std::vector<int64_t> wshape = {});

struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <typename T> T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// exact fp32 MFMA in GEMM_F32 mode; split-bf16 (3 bf16 MFMAs per product, ~2^-16 per product) for M >= 256 in the default mode
int lin(const LinearWeights& w, const float* x, int ldx, float* y, int ldy, int M, hipStream_t st, int act = ACT_NONE,
        const float* res = nullptr, int ldr = 0);
// exact fp32 whatever the mode: where an integer result follows (the semantic codec's nearest-code search)
int lin_exact(const LinearWeights& w, const float* x, int ldx, float* y, int ldy, int M, hipStream_t st, int act = ACT_NONE,
              const float* res = nullptr, int ldr = 0);
int layer_norm(const float* x, float* y, const float* g, const float* b, int M, int d, hipStream_t st);

}  // namespace idxtts
