// Channels-first Conv1d / ConvTranspose1d as an implicit GEMM: M = output channels, N = time, K = (input channel, tap).  Called by BigVGAN
// (bigvgan.hip) and the idxtts_conv1d_* entries (capi.hip).  One weight builder, tile table and launch set-up (conv_launch.h) serve three
// arithmetics: exact fp32 (conv1d.hip, v_mfma_f32_32x32x2_f32), split-bf16 and single-product bf16 (conv1d_bf16x3.hip, v_mfma_f32_32x32x16_bf16).
#pragma once
#include "common.h"

namespace idxtts {

struct DeviceArena;

constexpr int CONV_KC = 16;        // input channels per K-chunk
constexpr int CONV_MT = 32;        // rows per packed weight sub-tile
constexpr int CONV_SUB = 512;      // floats per packed sub-tile: [g2][h2][i32][4]
constexpr int CONV_SUB16_BYTES = 2 * CONV_SUB * 2;   // bytes of a sub-tile's split-bf16 image: [hl] planes of CONV_SUB bf16
constexpr int CONV_MAX_HALO = 64;  // (K-1)*dil upper bound supported by the tile loader

enum ConvPadMode { PAD_ZERO = 0, PAD_REFLECT = 1 };

struct ConvWeights {           // packed, device-resident
  const float* wp = nullptr;   // [ceil(M/32)][nchunk][K][g2][h2][i32][4]
  const void* wp16 = nullptr;  // optional split-bf16 images [ceil(M/32)][nchunk][K][hl][g2][i32][8] (conv1d_bf16x3.hip)
  const float* bias = nullptr; // [Cout_real] or null
  int M = 0;                   // GEMM rows (= Cout, or Cout*u for a transposed conv)
  int Cin = 0;
  int K = 0;                   // taps
  int nchunk = 0;              // ceil(Cin/16)
  int ups = 1;                 // u>1: rows are (co*u + r), output written interleaved y[co][s*u + r]
};

static inline size_t conv_packed_floats(int M, int Cin, int K) {
  return (size_t)cdiv(M, CONV_MT) * cdiv(Cin, CONV_KC) * K * CONV_SUB;
}
static inline size_t conv_packed16_bytes(int M, int Cin, int K) {      // the split-bf16 images of the same sub-tiles
  return conv_packed_floats(M, Cin, K) / CONV_SUB * CONV_SUB16_BYTES;
}

// Host-side packing (ctx creation time, not on the hot path).
// w: [Cout][Cin][K] (torch Conv1d layout).
void pack_conv1d(float* dst, const float* w, int Cout, int Cin, int K);
// w: [Cin][Cout][Kt] (torch ConvTranspose1d layout), stride u, padding (Kt-u)/2, Kt == 2u.
// Produces the equivalent 3-tap conv with M = Cout*u rows (row co*u+r, taps over x[s-1],x[s],x[s+1]).
void pack_conv_transpose1d(float* dst, const float* w, int Cin, int Cout, int Kt, int u);
// fp32 pack -> split-bf16 images, conv_packed16_bytes of them (conv1d_bf16x3.hip)
void pack_conv_bf16x3(void* dst, const float* packed_f32, size_t n_subtiles);
// Host weights of a Conv1d (ups == 1: w [Cout][Cin][K]) or a ConvTranspose1d of stride ups (w [Cin][Cout][K], K == 2 * ups), and
// bias [Cout] or null -> the GEMM geometry, the fp32 pack and the split-bf16 images, on the device.
int make_conv_weights(DeviceArena& arena, const float* w, const float* bias, int Cout, int Cin, int K, int ups, ConvWeights* out);

struct ConvArgs {
  const float* x = nullptr;    // [B][Cin][T]
  float* y = nullptr;          // [B][Cout][T*ups]
  const float* res = nullptr;  // optional residual, same layout as y
  int B = 0, T = 0;            // T = input length = GEMM columns per batch row
  int dil = 1;
  int pad_left = 0;            // y[t] taps x[t + k*dil - pad_left]
  int pad_mode = PAD_ZERO;
  float scale = 1.0f;          // v = (acc + bias + res) * scale
  int accum = 0;               // y = accum ? y + v : v
  // ragged batches: output samples t >= lens[b] * len_mul_out are written as 0 (a shorter row's tail stays zero, so the next
  // layer's zero padding at that row's own end is what a B = 1 call would see)
  const int* lens = nullptr; int len_mul_out = 1;
};

// A tile configuration (a wave owns TM x TN MFMA tiles of 32 x 32, the workgroup's 4 waves lie WGM x WGN), and the tile table of
// every arithmetic: f(ConvTile<...>{}) for a convolution of M GEMM rows.
template <int TM_, int TN_, int WGM_, int WGN_>
struct ConvTile {
  static constexpr int TM = TM_, TN = TN_, WGM = WGM_, WGN = WGN_;
  static constexpr int BM = 32 * TM_ * WGM_, BN = 32 * TN_ * WGN_, NSUB = TM_ * WGM_;      // output tile, weight sub-tiles per step
};
template <typename F>
static inline int conv_tile_dispatch(int M, F&& f) {
  if (M > 96) return f(ConvTile<2, 2, 2, 2>{});   // 128 x 128
  if (M > 64) return f(ConvTile<3, 2, 1, 4>{});   //  96 x 256
  if (M > 32) return f(ConvTile<2, 2, 1, 4>{});   //  64 x 256
  return f(ConvTile<1, 4, 1, 4>{});               //  32 x 512
}

// exact fp32, or conv1d_bf16x3_forward when the GEMM mode is GEMM_BF16X3 and w.wp16 is set (products = 1 while the acoustic-bf16
// switch of gemm.h is on, else 3).  products: bf16 MFMAs per product, 3 = split-bf16, 1 = hi * hi' alone
int conv1d_forward(const ConvWeights& w, const ConvArgs& a, hipStream_t stream);
int conv1d_bf16x3_forward(const ConvWeights& w, const ConvArgs& a, hipStream_t stream, int products = 3);

}  // namespace idxtts
