// Device-only helpers shared by the kernels: one definition each of the wave64 / workgroup reductions, the argmax tie rule and the
// last-arrival hand-off between workgroups.  Every helper is a fixed sequence of operations: a result does not depend on which
// kernel inlines it.
#pragma once
#include "common.h"

namespace idxtts {

// ---- sum / max over a wave64: xor butterfly, offsets 32 .. 1; every lane gets the result ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// ---- sum / max over a workgroup of NW waves; every thread gets the result.  red: NW floats of LDS.  The barrier in front protects
//      `red` from its previous use; the waves' values are combined in ascending wave order, left to right, starting FROM red[0] (not
//      from 0.f + red[0]: the two differ only for red[0] == -0.f, which no caller that once started from 0.f -- the softmax
//      denominators of beam.hip and of the warped sampler, sums of expf -- can produce) ----
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = fmaxf(t, red[w]);
  return t;
}

// ---- argmax: the larger value wins, the lower index among equal values ----
__device__ __forceinline__ void argmax_take(float& v, int& i, const float ov, const int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argmax(float& v, int& i) {      // every lane gets the result
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    argmax_take(v, i, ov, oi);
  }
}
// the waves' candidates, already in rv / ri, in ascending wave order on top of (v, i)
template <int NW>
__device__ __forceinline__ void argmax_take_waves(float& v, int& i, const float* rv, const int* ri) {
  for (int w = 1; w < NW; ++w) argmax_take(v, i, rv[w], ri[w]);
}
// over a workgroup of NW waves; every thread gets the result.  rv / ri: NW entries of LDS, protected by the barrier in front
template <int NW>
__device__ __forceinline__ void block_argmax(float& v, int& i, float* rv, int* ri, const int tid) {
  wave_argmax(v, i);
  __syncthreads();
  if ((tid & 63) == 0) { rv[tid >> 6] = v; ri[tid >> 6] = i; }
  __syncthreads();
  v = rv[0]; i = ri[0];
  argmax_take_waves<NW>(v, i, rv, ri);
}

// ---- last-arrival hand-off: several workgroups leave partial results in device memory and bump `counter`; the one that finds
//      expected - 1 earlier arrivals is the last, resets the counter for the next launch and finishes the job (wait-free: nobody
//      spins).  Returns the workgroup-uniform flag.  Call it from every thread, after the workgroup's stores of its partial results
//      (device scope: agent-scope atomics or sc1 write-through stores), at most once per kernel.
// EVERY wave waits for the acknowledgement of its device-scope stores before the workgroup barrier, so the arrival is issued after
// all partial results of this workgroup are at the device coherence point.  (An acq_rel arrival would say the same in the memory
// model, but costs an L2 write-back + invalidate per launch: measured +10 us on the decode GEMV.) ----
__device__ __forceinline__ bool wg_arrive_last(unsigned* counter, const unsigned expected) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == expected - 1u;
    if (s_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return s_last;
}

}  // namespace idxtts
