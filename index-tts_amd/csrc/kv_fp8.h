// The scaled-fp8 KV cache format (IDXTTS_KV_FP8, include/idxtts.h): the one quantiser every producer of a cached key or value calls.
//   unit      one vector: the 64 head dims of one (layer, row, head, position); keys and values separately, by the same rule
//   scale     s = 2^e, e = ceil(log2(amax / 448)) clamped to [-100, 100] (wstream.h::fp8_column_scale's rule), s = 1 for amax == 0.
//             Taken from amax's exponent and mantissa with integer operations, so it is exact: 448 = 1.75 * 2^8, hence
//             e = exponent(amax) - 8, plus 1 when the mantissa exceeds that of 1.75
//   code      OCP e4m3fn of x / s, nearest with ties to the even code (the device's conversion, checked against the host codec by
//             fp8_check_device_encode).  x * 2^-e is exact above the subnormal range and |x / s| <= 448: nothing saturates
//   value     decode(code) * s, an exact fp32 product; every later product and sum is fp32
// Storage: codes in the bf16 cache's geometry with one byte per element, K [rows][H][8][Smax][8], V [rows][H][Smax][64], and one fp32
// scale per vector, [rows][H][Smax] for K and for V (chosen over a one-byte exponent: the reader multiplies by it as loaded).
#pragma once
#include "common.h"
#include "device_util.h"

namespace idxtts {

__device__ __forceinline__ int kv_fp8_scale_exp(const float amax) {
  const unsigned u = __float_as_uint(amax) & 0x7fffffffu;
  if (u == 0u) return 0;
  const int e = (int)(u >> 23) - 127 - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return max(-100, min(100, e));      // (a subnormal amax lands far below the clamp)
}
__device__ __forceinline__ float kv_fp8_pow2(const int e) { return __uint_as_float((unsigned)(127 + e) << 23); }
__device__ __forceinline__ unsigned kv_fp8_encode(const float y) { return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(y, 0.0f, 0, false) & 0xffu; }
__device__ __forceinline__ float kv_fp8_decode(const unsigned code) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)code, false)[0]; }

// One vector per wave, lane = head dim (every lane of the wave calls): this lane's code, the vector's scale (the same in every lane),
// and the value the cache now stands for
__device__ __forceinline__ float kv_fp8_quantize_lane(const float x, unsigned& code, float& scale) {
  const int e = kv_fp8_scale_exp(wave_max(fabsf(x)));
  scale = kv_fp8_pow2(e);
  code = kv_fp8_encode(x * kv_fp8_pow2(-e));
  return kv_fp8_decode(code) * scale;
}

}  // namespace idxtts
