// The split-bf16 GEMM's wave-level stage loop on both bf16 MFMA shapes, at EQUAL LDS bytes per flop, on random data, with no
// global traffic: which shape is faster by wall, and what clock does the chip hold under each?
//
// Both arms: 4 waves per workgroup, a 64 x 64 fp32 tile per wave, hi / lo operand planes in LDS in gemm_bf16x3_v2.hip's stage
// image ([A hi][A lo][B hi][B lo], 128 rows x 32 B each, 16-B unit ^= row bit 3; a 3-slot ring of 16-k stages), fragments by
// ds_read_b128, three products per MAC (lo*hi, hi*lo, hi*hi), 16 fragment reads per wave and 32 k:
//   arm 0  v_mfma_f32_32x32x16_bf16: per 16-k stage 2 + 2 A and 2 + 2 B fragments, 12 MFMAs (the shipped loop's body);
//   arm 1  v_mfma_f32_16x16x32_bf16: per PAIR of stages 4 + 4 A fragments (kept live, the next pair's loaded beside the MFMAs)
//          and 4 + 4 B fragments streamed column tile by column tile through two buffers, 48 MFMAs.  A lane's 8 k come from
//          stage s + (lane >> 5), unit (lane >> 4) & 1.
// One, two and three workgroups per CU (= waves per SIMD), set by the dynamic LDS size.  Per arm: wall time per MFMA flop (HIP
// events), wave cycles per flop (s_memtime around the loop) and the in-kernel clock (delta s_memtime / delta s_memrealtime x 100 MHz,
// median over workgroups) of a launch that follows >= 2 s of back-to-back launches of the same arm.  Arms alternate within a round.
// A short launch first checks both arms against a float64 host product of the same planes.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma_shape_probe.hip -o /tmp/mfma_shape_probe && /tmp/mfma_shape_probe > profiles/mfma_shape_probe.txt
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int PLANE = 128 * 32, STAGE = 4 * PLANE, NSLOT = 3;

__host__ __device__ inline uint16_t f2bf(float x) {
  uint32_t u; __builtin_memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf2f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float x; __builtin_memcpy(&x, &u, 4); return x; }
// element (slot, operand, row, k) of workgroup `wg`: uniform in [-0.5, 0.5)
__host__ __device__ inline float elem(uint32_t wg, uint32_t idx) {
  uint32_t h = idx * 2654435761u + wg * 0x9e3779b9u + 12345u;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

template <int SHAPE>
__global__ __launch_bounds__(256, 3) void probe(int steps, unsigned long long* __restrict__ stamps, float* __restrict__ cout) {
  extern __shared__ __attribute__((aligned(1024))) char sm[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  for (int idx = tid; idx < NSLOT * 2 * 128 * 16; idx += 256) {
    const int k = idx & 15, row = (idx >> 4) & 127, op = (idx >> 11) & 1, slot = idx >> 12;
    const float x = elem(blockIdx.x, idx);
    const uint16_t hi = f2bf(x), lo = f2bf(x - bf2f(hi));
    char* at = sm + slot * STAGE + op * 2 * PLANE + row * 32 + (((k >> 3) ^ ((row >> 3) & 1)) * 16) + (k & 7) * 2;
    *reinterpret_cast<uint16_t*>(at) = hi;
    *reinterpret_cast<uint16_t*>(at + PLANE) = lo;
  }
  __syncthreads();
  unsigned long long t0 = 0, r0 = 0;
  if (stamps) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }

  if constexpr (SHAPE == 0) {
    const int h = lane >> 5, j = lane & 31;
    const int sw = (h ^ ((j >> 3) & 1)) * 16;
    const int a_off = (wm * 64 + j) * 32 + sw, b_off = 2 * PLANE + (wn * 64 + j) * 32 + sw;
    f32x16 acc[2][2];
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    struct Frag { bf16x8 ah[2], al[2], bh[2], bl[2]; };
    int rslot = 0;
    auto load_frags = [&](Frag& f) {
      const char* st = sm + rslot * STAGE;
      rslot = rslot + 1 == NSLOT ? 0 : rslot + 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f.ah[t] = *reinterpret_cast<const bf16x8*>(st + a_off + t * 1024);
        f.al[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + a_off + t * 1024);
        f.bh[t] = *reinterpret_cast<const bf16x8*>(st + b_off + t * 1024);
        f.bl[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + b_off + t * 1024);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    auto compute = [&](const Frag& f) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bl[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    };
    Frag f0, f1;
    load_frags(f0);
    for (int s = 0; s < steps; ++s) {        // a step = 32 k = two stages
      load_frags(f1);
      compute(f0);
      load_frags(f0);
      compute(f1);
    }
    if (cout && blockIdx.x == 0)
      for (int mt = 0; mt < 2; ++mt) for (int nt = 0; nt < 2; ++nt) for (int r = 0; r < 16; ++r)
        cout[(wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 128 + wn * 64 + nt * 32 + j] = acc[mt][nt][r];
  } else {
    const int g = lane >> 4, r16 = lane & 15;
    const int sw = ((g & 1) ^ ((r16 >> 3) & 1)) * 16;
    const int a_off = (wm * 64 + r16) * 32 + sw, b_off = 2 * PLANE + (wn * 64 + r16) * 32 + sw;      // + t * 512 per 16-row tile
    f32x4 acc[4][4];
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
    struct FragA { bf16x8 h[4], l[4]; };
    bf16x8 bh[2], bl[2];
    int s0 = 0;                                       // ring slot of the pair's first stage
    auto pair_base = [&](int first) -> const char* {  // lanes 0-31 read the pair's first stage, lanes 32-63 its second
      const int second = first + 1 >= NSLOT ? first + 1 - NSLOT : first + 1;
      return sm + ((g >> 1) ? second : first) * STAGE;
    };
    auto load_a = [&](FragA& f, const char* st, int t) {
      f.h[t] = *reinterpret_cast<const bf16x8*>(st + a_off + t * 512);
      f.l[t] = *reinterpret_cast<const bf16x8*>(st + PLANE + a_off + t * 512);
    };
    auto load_b = [&](const char* st, int t) {
      bh[t & 1] = *reinterpret_cast<const bf16x8*>(st + b_off + t * 512);
      bl[t & 1] = *reinterpret_cast<const bf16x8*>(st + PLANE + b_off + t * 512);
    };
    auto step = [&](const FragA& a, FragA& an) {
      const char* cur = pair_base(s0);
      s0 = s0 + 2 >= NSLOT ? s0 + 2 - NSLOT : s0 + 2;
      const char* nxt = pair_base(s0);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt < 3) load_b(cur, nt + 1); else load_b(nxt, 0);
        load_a(an, nxt, nt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l[mt], bh[nt & 1], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h[mt], bl[nt & 1], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h[mt], bh[nt & 1], acc[mt][nt], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    FragA a0, a1;
    {
      const char* st = pair_base(0);
#pragma unroll
      for (int t = 0; t < 4; ++t) load_a(a0, st, t);
      load_b(st, 0);
    }
    for (int s = 0; s < steps; s += 2) {     // steps is even
      step(a0, a1);
      step(a1, a0);
    }
    if (cout && blockIdx.x == 0)
      for (int mt = 0; mt < 4; ++mt) for (int nt = 0; nt < 4; ++nt) for (int e = 0; e < 4; ++e)
        cout[(wm * 64 + mt * 16 + 4 * g + e) * 128 + wn * 64 + nt * 16 + r16] = acc[mt][nt][e];
  }

  if (stamps && lane == 0 && wave == 0) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    stamps[2 * blockIdx.x] = t1 - t0;
    stamps[2 * blockIdx.x + 1] = r1 - r0;
  }
}

typedef void (*ProbeFn)(int, unsigned long long*, float*);

int main() {
  const ProbeFn fn[2] = {probe<0>, probe<1>};
  const char* name[2] = {"32x32x16", "16x16x32"};
  for (int a = 0; a < 2; ++a) CK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn[a]), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const int max_wg = cus * 3 * 4;
  unsigned long long* stamps; float* cout;
  CK(hipMalloc(&stamps, sizeof(unsigned long long) * 2 * max_wg)); CK(hipMalloc(&cout, sizeof(float) * 128 * 128));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

  {   // both arms against the float64 three-product sum of workgroup 0's planes: 6 steps = 12 stages = every ring slot four times
    const int steps = 6;
    std::vector<float> hi(NSLOT * 2 * 128 * 16), lo(hi.size());
    for (size_t i = 0; i < hi.size(); ++i) { const float x = elem(0, (uint32_t)i); hi[i] = bf2f(f2bf(x)); lo[i] = bf2f(f2bf(x - hi[i])); }
    std::vector<double> ref(128 * 128, 0.0);
    for (int slot = 0; slot < NSLOT; ++slot)
      for (int m = 0; m < 128; ++m)
        for (int n = 0; n < 128; ++n) {
          double s = 0;
          for (int k = 0; k < 16; ++k) {
            const size_t ia = (((size_t)slot * 2 + 0) * 128 + m) * 16 + k, ib = (((size_t)slot * 2 + 1) * 128 + n) * 16 + k;
            s += (double)hi[ia] * hi[ib] + (double)hi[ia] * lo[ib] + (double)lo[ia] * hi[ib];
          }
          ref[m * 128 + n] += s * (2 * steps / NSLOT);
        }
    std::vector<float> got(128 * 128);
    for (int a = 0; a < 2; ++a) {
      CK(hipMemset(cout, 0xff, sizeof(float) * 128 * 128));
      hipLaunchKernelGGL(fn[a], dim3(4), dim3(256), NSLOT * STAGE, 0, steps, nullptr, cout);
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(got.data(), cout, sizeof(float) * got.size(), hipMemcpyDeviceToHost));
      double err = 0;
      for (size_t i = 0; i < got.size(); ++i) err = std::max(err, std::isfinite(got[i]) ? std::fabs(got[i] - ref[i]) : 1e30);
      printf("check %s: max |C - fp64| = %.3e over 128 x 128 (K = %d)\n", name[a], err, 32 * steps);
      if (!(err < 1e-4)) { printf("MISMATCH\n"); return 1; }
    }
  }

  const int steps = 2048;                       // 64 Ki k per wave and launch
  const double flop_wave = 3.0 * 2.0 * 64 * 64 * 32 * steps;       // MFMA flops (three products per MAC)
  const int lds_for[4] = {0, 96 * 1024, 64 * 1024, NSLOT * STAGE};  // one / two / three workgroups fit a CU's 160 KiB
  printf("device: %s, %d CUs; %d steps of 32 k per launch, 4 workgroup rounds per launch\n", prop.gcnArchName, cus, steps);
  printf("waves/SIMD  shape     round  wall fs/flop   TF/s (MFMA)  wave cyc/kflop  in-kernel clock GHz\n");
  for (int wps = 1; wps <= 3; ++wps) {
    const int grid = cus * wps * 4;
    double wall[2][3];
    for (int round = 0; round < 3; ++round)
      for (int a = 0; a < 2; ++a) {
        const auto w0 = std::chrono::steady_clock::now();
        do {
          for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(fn[a], dim3(grid), dim3(256), lds_for[wps], 0, steps, nullptr, nullptr);
          CK(hipDeviceSynchronize());
        } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0);
        const int reps = 8;
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(fn[a], dim3(grid), dim3(256), lds_for[wps], 0, steps, nullptr, nullptr);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        hipLaunchKernelGGL(fn[a], dim3(grid), dim3(256), lds_for[wps], 0, steps, stamps, nullptr);      // the stamped (diagnostic) launch
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> st(2 * grid);
        CK(hipMemcpy(st.data(), stamps, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost));
        std::vector<double> cyc(grid), clk(grid);
        for (int i = 0; i < grid; ++i) { cyc[i] = (double)st[2 * i]; clk[i] = (double)st[2 * i] / (double)st[2 * i + 1] * 0.1; }
        std::nth_element(cyc.begin(), cyc.begin() + grid / 2, cyc.end());
        std::nth_element(clk.begin(), clk.begin() + grid / 2, clk.end());
        const double flops = flop_wave * 4.0 * grid * reps;
        wall[a][round] = ms * 1e-3 / flops;
        printf("%10d  %s  %5d  %12.4f  %12.1f  %14.4f  %19.3f\n", wps, name[a], round, wall[a][round] * 1e15, flops / (ms * 1e-3) / 1e12,
               cyc[grid / 2] / flop_wave * 1e3, clk[grid / 2]);
        fflush(stdout);
      }
    for (int a = 0; a < 2; ++a) std::sort(wall[a], wall[a] + 3);
    printf("waves/SIMD %d: median wall 32x32x16 / 16x16x32 = %.4f   (spread of a shape's rounds: %.2f %% / %.2f %%)\n", wps, wall[0][1] / wall[1][1],
           (wall[0][2] / wall[0][0] - 1) * 100, (wall[1][2] / wall[1][0] - 1) * 100);
  }
  return 0;
}
