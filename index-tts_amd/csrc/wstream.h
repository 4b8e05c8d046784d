#pragma once
#include "common.h"

namespace idxtts {

// Storage format of a decode weight stream.  The arithmetic is the same fp32 MFMA in every format: a compact format only
// changes what is READ (the decode is bound by the weight stream), the values are widened to fp32 in registers.
//   WFMT_F32  4 B / weight
//   WFMT_BF16 2 B / weight (the fp32 value rounded to nearest-even bf16)
//   WFMT_FP8  1 B / weight: OCP e4m3fn code q and a per-output-channel POWER-OF-TWO scale s, weight = s * q (exact in fp32,
//             so s * sum(x q) == sum(x (s q)) bit for bit: the kernel equals the fp32 kernel run on the dequantised matrix)
enum WeightFormat { WFMT_F32 = 0, WFMT_BF16 = 1, WFMT_FP8 = 2 };
static inline int wfmt_bytes(int fmt) { return fmt == WFMT_FP8 ? 1 : (fmt == WFMT_BF16 ? 2 : 4); }

// A matrix W[K][N] as the B fragments one MFMA lane reads in one piece: [ceil(N/16)][ceil(K/kdepth)][64 lanes][kdepth/4] elements of
// `fmt`, lane l holding n = 16 t + (l & 15), k = kdepth c + (kdepth/4) (l >> 4) + j; padding is zero.
//   kdepth 16: v_mfma_f32_16x16x4_f32, four k per lane (gemv_fx.hip)
//   kdepth 32: v_mfma_f32_16x16x32_bf16, eight k per lane (gemv_pl.hip)
struct WeightStream {
  const void* wp = nullptr;
  const float* wscale = nullptr;    // WFMT_FP8: [N] power-of-two column scales
  int fmt = WFMT_F32;
  int N = 0, K = 0;
  int kdepth = 0;
};
static inline size_t wstream_elems(int N, int K, int kdepth) { return (size_t)cdiv(N, 16) * cdiv(K, kdepth) * 16 * kdepth; }

// ---- host side (wstream.hip) ----
float fp8_e4m3_decode(unsigned char code);                 // OCP e4m3fn (bias 7, max 448, 0x7f / 0xff = NaN)
unsigned char fp8_e4m3_encode(float v);                    // round to nearest, ties to even code, saturating, never NaN
float bf16_round(float v);                                 // fp32 -> nearest-even bf16 -> fp32
float fp8_column_scale(float maxabs);                      // 2^ceil(log2(maxabs / 448)) (1 for an all-zero column)
// Round a [K][N] (kn) or [N][K] matrix IN PLACE to the values the format can hold (fp8: per output channel n).
void quantize_matrix(float* w, int K, int N, bool kn, int fmt);
// Pack an already-quantised matrix (every value representable in `fmt`), given as [K][N] (kn: HF Conv1D) or [N][K] (nn.Linear), into
// the stream order above: dst holds wstream_elems(N, K, kdepth) elements of `fmt`.  fp8 also returns the per-column scales
// (scale_out[N], may be null).  Returns 1 if a value is not representable.
int pack_wstream(void* dst, const float* w, int N, int K, bool kn, int fmt, int kdepth, float* scale_out);
int fp8_check_device_decode(hipStream_t stream);           // the device's v_cvt_pk_f32_fp8 equals fp8_e4m3_decode on all codes

}  // namespace idxtts
