// Decode weight streams (wstream.h): the storage formats' host codecs, the rounding of a model to a format, and the one packer that
// turns a matrix into the lane-ordered stream either decode GEMV reads (gemv_fx.hip at 16 k per chunk, gemv_pl.hip at 32).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wstream.h"

namespace idxtts {

float fp8_e4m3_decode(unsigned char code) {
  const int e = (code >> 3) & 15, m = code & 7;
  float v;
  if (e == 15 && m == 7) v = NAN;
  else if (e == 0) v = ldexpf((float)m, -9);                 // m/8 * 2^-6
  else v = ldexpf(8.0f + (float)m, e - 10);                  // (1 + m/8) * 2^(e-7)
  return (code & 0x80) ? -v : v;
}

unsigned char fp8_e4m3_encode(float v) {
  const unsigned char sign = std::signbit(v) ? 0x80 : 0;
  const float a = std::fabs(v);
  if (!(a < 448.0f)) return sign | 126;                      // saturate (NaN too: quantize_matrix never feeds one)
  if (a < 0.015625f) return sign | (unsigned char)nearbyintf(a * 512.0f);   // subnormal grid 2^-9 (8 -> the smallest normal)
  uint32_t u; memcpy(&u, &a, 4);
  u += 0x7ffffu + ((u >> 20) & 1u);                          // nearest-even on the 3 kept mantissa bits
  const int c = (int)(u >> 20) - ((127 - 7) << 3);
  return sign | (unsigned char)std::min(c, 126);
}

float bf16_round(float v) {
  uint32_t u; memcpy(&u, &v, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return v;
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  float r; memcpy(&r, &u, 4);
  return r;
}

float fp8_column_scale(float maxabs) {
  if (!(maxabs > 0.0f)) return 1.0f;
  int e; const float f = frexpf(maxabs / 448.0f, &e);        // maxabs/448 = f * 2^e, f in [0.5, 1)
  if (f == 0.5f) e -= 1;
  return ldexpf(1.0f, std::max(-100, std::min(100, e)));
}

void quantize_matrix(float* w, int K, int N, bool kn, int fmt) {
  if (fmt == WFMT_F32) return;
  auto at = [&](int k, int n) -> float& { return kn ? w[(size_t)k * N + n] : w[(size_t)n * K + k]; };
  if (fmt == WFMT_BF16) {
    for (size_t i = 0; i < (size_t)K * N; ++i) w[i] = bf16_round(w[i]);
    return;
  }
  std::vector<float> mx(N, 0.0f);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) mx[n] = std::max(mx[n], std::fabs(at(k, n)));
  for (int n = 0; n < N; ++n) mx[n] = fp8_column_scale(mx[n]);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) { float& v = at(k, n); v = mx[n] * fp8_e4m3_decode(fp8_e4m3_encode(v / mx[n])); }
}

int pack_wstream(void* dst, const float* w, int N, int K, bool kn, int fmt, int kdepth, float* scale_out) {
  if ((kdepth != 16 && kdepth != 32) || (fmt != WFMT_F32 && fmt != WFMT_BF16 && fmt != WFMT_FP8)) return 1;
  const int NT = cdiv(N, 16), KC = cdiv(K, kdepth), per = kdepth / 4;
  auto at = [&](int k, int n) -> float { return (k < K && n < N) ? (kn ? w[(size_t)k * N + n] : w[(size_t)n * K + k]) : 0.0f; };
  std::vector<float> sc(NT * 16, 1.0f);      // fp8: the column scales, from the matrix itself (the rule of quantize_matrix)
  if (fmt == WFMT_FP8) {
    std::vector<float> mx(N, 0.0f);
    for (int k = 0; k < K; ++k)
      for (int n = 0; n < N; ++n) mx[n] = std::max(mx[n], std::fabs(at(k, n)));
    for (int n = 0; n < N; ++n) {
      sc[n] = fp8_column_scale(mx[n]);
      if (scale_out) scale_out[n] = sc[n];
    }
  }
  size_t i = 0;      // the destination is written front to back: [nt][c][lane][j]
  for (int nt = 0; nt < NT; ++nt)
    for (int c = 0; c < KC; ++c)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < per; ++j, ++i) {
          const int n = nt * 16 + (lane & 15);
          const float v = at(c * kdepth + per * (lane >> 4) + j, n);
          if (fmt == WFMT_F32) {
            static_cast<float*>(dst)[i] = v;
          } else if (fmt == WFMT_BF16) {
            uint32_t u; memcpy(&u, &v, 4);
            if (u & 0xffffu) return 1;
            static_cast<uint16_t*>(dst)[i] = (uint16_t)(u >> 16);
          } else {
            const unsigned char q = fp8_e4m3_encode(v / sc[n]);
            if (sc[n] * fp8_e4m3_decode(q) != v) return 1;
            static_cast<unsigned char*>(dst)[i] = q;
          }
        }
  return 0;
}

__global__ void fp8_decode_table_kernel(float* out) {
  const int c = threadIdx.x;      // 256 codes
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(c, false);
  out[c] = lo[0];
}

int fp8_check_device_decode(hipStream_t stream) {
  static bool ok = false;
  if (ok) return 0;
  float* d = nullptr;
  IDX_HIP(hipMalloc(&d, 256 * sizeof(float)));
  hipLaunchKernelGGL(fp8_decode_table_kernel, dim3(1), dim3(256), 0, stream, d);
  float h[256];
  hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(d);
  IDX_HIP(e);
  for (int c = 0; c < 256; ++c) {
    const float want = fp8_e4m3_decode((unsigned char)c);
    if (std::isnan(want)) continue;
    if (!(h[c] == want)) IDX_FAIL("this device's fp8 conversion is not OCP e4m3fn (code " + std::to_string(c) + ")");
  }
  ok = true;
  return 0;
}

}  // namespace idxtts
