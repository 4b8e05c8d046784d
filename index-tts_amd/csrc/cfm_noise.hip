// idxtts_cfm_noise: the flow-matching noise z of flow_matching.py:52 from a counter-based generator keyed by one seed per utterance.
// Element (b, c, t) is a pure function of (seeds[b], c, t): it does not depend on the batch, the padded width T, the row's position,
// the stream or the thread that asks for it, so a request's noise -- and with it its audio -- is the same alone and merged.
//
// The draw (integer part mod 2^64; the tests restate it):
//   idx = (c << 32) | t                                   t counted from the row's column 0, prompt frames included
//   z   = (seed ^ 0xD1B54A32D192ED03) + 0x9E3779B97F4A7C15 * (idx + 1)      the xor keeps this stream apart from a sampler's
//   z   = splitmix64 finaliser of z                       exp1_draw's mix (decode.h)
//   u1  = ((z >> 41) + 0.5) * 2^-23,  u2 = (((z >> 18) & 0x7FFFFF) + 0.5) * 2^-23      23 bits each: exact in fp32, never 0 or 1
//   n   = sqrt(-2 ln u1) * cos(2 pi u2)                   Box-Muller, one hash per element (no pairing with a neighbour)
// The smallest u1 is 2^-24, so |n| <= sqrt(2 * 24 ln 2) = 5.77: the tail is cut at 5.77 sigma, 8e-9 of the mass per draw.
// cos(2 pi u2) is v_cos_f32, whose argument is in revolutions: u2 goes in exactly, no rounded 2 pi u2 (abs error ~1e-7 on [0, 1),
// profiles/README.md "v_sin_f32").  log stays logf (relative accuracy where u1 is near 1 and n is small); sqrt is v_sqrt_f32 (1 ulp).
#include "../../include/idxtts.h"
#include "common.h"

namespace idxtts {

constexpr int NOISE_ROWS = 32;        // utterances per launch: their seeds and lengths travel by value in the launch arguments
constexpr int NOISE_THREADS = 256;    // x 4 floats = 4 KiB of one row per workgroup

struct NoiseRows {
  unsigned long long seed[NOISE_ROWS];
  int x_len[NOISE_ROWS];
};

__device__ static inline float cfm_noise_draw(unsigned long long seed, int c, int t) {
  const unsigned long long idx = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)t;
  unsigned long long z = (seed ^ 0xD1B54A32D192ED03ull) + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const float u1 = ((float)(unsigned)(z >> 41) + 0.5f) * (1.0f / 8388608.0f);
  const float u2 = ((float)(unsigned)((z >> 18) & 0x7FFFFFull) + 0.5f) * (1.0f / 8388608.0f);
  return __builtin_amdgcn_sqrtf(-2.0f * logf(u1)) * __builtin_amdgcn_cosf(u2);
}

// grid (float4 groups of a row, rows of this launch).  A row is its C * T contiguous floats; a thread owns the 16-byte-aligned
// group of 4 floats number `g`, counted from the aligned address at or below the row's start: group 0 and the last group may be cut
// by the row's ends and are stored float by float, every whole group as one float4 (a group may run from one channel into the next).
// All four values of a thread come from the same call, whole or cut.
__global__ void __launch_bounds__(NOISE_THREADS) cfm_noise_kernel(NoiseRows rows, int C, int T, float* __restrict__ z) {
  const int b = blockIdx.y;
  const int CT = C * T;
  float* row = z + (size_t)b * CT;
  const int lead = (int)(((uintptr_t)row >> 2) & 3);           // floats between the aligned address below and the row's start
  const int e0 = (blockIdx.x * NOISE_THREADS + threadIdx.x) * 4 - lead;      // the group's first float in the row (< 0 only in group 0)
  if (e0 >= CT) return;
  const unsigned long long seed = rows.seed[b];
  const int x_len = rows.x_len[b];
  int c = e0 >= 0 ? e0 / T : 0;
  int t = e0 - c * T;                                          // < 0 in front of the row: counts up to frame 0 of channel 0
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = (t >= 0 && t < x_len && e0 + i < CT) ? cfm_noise_draw(seed, c, t) : 0.0f;
    if (++t == T) { t = 0; ++c; }
  }
  if (e0 >= 0 && e0 + 4 <= CT) {
    *reinterpret_cast<float4*>(row + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i >= 0 && e0 + i < CT) row[e0 + i] = v[i];
  }
}

}  // namespace idxtts

using namespace idxtts;

extern "C" int idxtts_cfm_noise(const unsigned long long* seeds, const int* x_lens, int B, int C, int T, float* z, void* stream) {
  IDX_CHECK(seeds && x_lens && z, "null pointer");
  IDX_CHECK(B >= 1 && C >= 1 && T >= 1, "B, C and T must be at least 1");
  IDX_CHECK((long long)C * T <= 0x7fffff00ll, "C * T must fit an int");
  IDX_CHECK(((uintptr_t)z & 3) == 0, "z must be aligned to 4 bytes");
  for (int b = 0; b < B; ++b)
    IDX_CHECK(x_lens[b] >= 0 && x_lens[b] <= T, "x_lens[" + std::to_string(b) + "] = " + std::to_string(x_lens[b]) + " outside 0.." + std::to_string(T));
  const int groups = (C * T + 3) / 4 + 1;                      // + 1: a row that starts off a 16-byte boundary spills into one more
  const dim3 block(NOISE_THREADS);
  for (int b0 = 0; b0 < B; b0 += NOISE_ROWS) {
    const int n = B - b0 < NOISE_ROWS ? B - b0 : NOISE_ROWS;
    NoiseRows rows = {};
    for (int i = 0; i < n; ++i) { rows.seed[i] = seeds[b0 + i]; rows.x_len[i] = x_lens[b0 + i]; }
    const dim3 grid((groups + NOISE_THREADS - 1) / NOISE_THREADS, n);
    hipLaunchKernelGGL(cfm_noise_kernel, grid, block, 0, static_cast<hipStream_t>(stream), rows, C, T, z + (size_t)b0 * C * (size_t)T);
    IDX_LAUNCH_CHECK();
  }
  return 0;
}
