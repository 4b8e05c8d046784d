// Small HBM-bound element-wise kernels of the s2mel stage (everything GEMM-shaped is in gemm.hip).
#include "device_util.h"
#include "prof.h"
#include "s2mel_ops.h"

namespace idxtts {

__global__ __launch_bounds__(256) void rotary_qk_kernel(float* qkv, int M, int H, int seq_len, const float* rope) {
  // one thread per (row, head, pair) over q and k: 2*H*32 pairs per row
  const int pairs = 2 * H * 32;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)M * pairs) return;
  const int m = (int)(idx / pairs), r = (int)(idx - (size_t)m * pairs);
  const int i = r & 31;                       // pair index inside the head
  const int t = m % seq_len;
  float2* ptr = reinterpret_cast<float2*>(qkv + (size_t)m * 3 * H * 64) + r;   // q then k are contiguous: r < 2*H*32
  const float2 cs = reinterpret_cast<const float2*>(rope)[(size_t)t * 32 + i];
  const float2 v = *ptr;
  *ptr = float2{v.x * cs.x - v.y * cs.y, v.y * cs.x + v.x * cs.y};
}

int rotary_qk(float* qkv, int M, int H, int seq_len, const float* rope, hipStream_t st) {
  IDX_CHECK(qkv && rope && seq_len > 0, "rotary args");
  const size_t n = (size_t)M * 2 * H * 32;
  static const int cat = prof_register("rotary_qk_kernel");
  ProfScope prof(cat, st, 0.0, 16.0 * n);
  hipLaunchKernelGGL(rotary_qk_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, qkv, M, H, seq_len, rope);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void silu_kernel(float* y, const float* x, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { const float v = x[i]; y[i] = v / (1.0f + expf(-v)); }
}

int silu_rows(float* y, const float* x, size_t n, hipStream_t st) {
  if (!n) return 0;
  hipLaunchKernelGGL(silu_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, y, x, n);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_pack_kernel(const CfmPackArgs p) {
  // block = (t-tile of 64 frames, stacked row n); threads sweep the 864 columns
  const int n = blockIdx.y, b = n % p.B;
  const bool is_cond = n < p.B;
  const int t0 = blockIdx.x * 64;
  const int W = p.x_only ? p.C : 2 * p.C + p.D + p.S;      // x_only: the columns that change from one Euler step to the next
  const int Tp = p.prompt_len[b];
  for (int e = threadIdx.x; e < 64 * W; e += 256) {
    const int tt = e / W, c = e - tt * W;
    const int t = t0 + tt;
    if (t >= p.T) break;
    float v;
    if (c < p.C) v = p.x[((size_t)b * p.C + c) * p.T + t];
    else if (c < 2 * p.C) v = (is_cond && t < Tp) ? p.prompt[((size_t)b * p.C + (c - p.C)) * p.Tp_max + t] : 0.0f;
    else if (c < 2 * p.C + p.D) v = is_cond ? p.cond[((size_t)b * p.T + t) * p.D + (c - 2 * p.C)] : p.cond_null[c - 2 * p.C];
    else v = is_cond ? p.style[(size_t)b * p.S + (c - 2 * p.C - p.D)] : 0.0f;
    p.x_in[((size_t)n * p.T + t) * p.ld + c] = v;
  }
}

int cfm_pack(const CfmPackArgs& a, hipStream_t st) {
  const double bytes = 4.0 * 2 * a.B * (double)a.T * (a.x_only ? a.C : 2 * a.C + a.D + a.S) * 2;
  static const int cat = prof_register("cfm_pack_kernel");
  ProfScope prof(cat, st, 0.0, bytes);
  hipLaunchKernelGGL(cfm_pack_kernel, dim3(cdiv(a.T, 64), 2 * a.B), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_euler_kernel(const CfmEulerArgs p) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.B * p.C * p.T;
  if (idx >= total) return;
  const int t = (int)(idx % p.T);
  const int c = (int)((idx / p.T) % p.C);
  const int b = (int)(idx / ((size_t)p.T * p.C));
  if (t < p.prompt_len[b] || t < p.v_t0) { p.x[idx] = 0.0f; return; }
  const int vT = p.v_T > 0 ? p.v_T : p.T, tv = t - p.v_t0;
  const float vc = p.v[((size_t)b * vT + tv) * p.ldv + c];
  const float vn = p.v_null ? p.v_null[((size_t)b * vT + tv) * p.ldv + c] : p.v[((size_t)(p.B + b) * vT + tv) * p.ldv + c];
  const float dphi = (1.0f + p.cfg_rate) * vc - p.cfg_rate * vn;
  p.x[idx] = p.x[idx] + p.dt * dphi;
}

int cfm_euler(const CfmEulerArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.B * a.C * a.T;
  static const int cat = prof_register("cfm_euler_kernel");
  ProfScope prof(cat, st, 0.0, 16.0 * total);
  hipLaunchKernelGGL(cfm_euler_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void gather_tail_rows_kernel(float* dst, int ld_dst, const float* src, int ld_src, int cols, int T, int t0, int Tn) {
  const int j = blockIdx.x, n = blockIdx.y;
  const float* s = src + ((size_t)n * T + t0 + j) * ld_src;
  float* d = dst + ((size_t)n * Tn + j) * ld_dst;
  if (((cols | ld_dst | ld_src) & 3) == 0) {
    for (int e = threadIdx.x; e < cols / 4; e += 256) reinterpret_cast<f32x4*>(d)[e] = reinterpret_cast<const f32x4*>(s)[e];
  } else {
    for (int e = threadIdx.x; e < cols; e += 256) d[e] = s[e];
  }
}

int gather_tail_rows(float* dst, int ld_dst, const float* src, int ld_src, int cols, int N, int T, int t0, hipStream_t st) {
  IDX_CHECK(dst && src && t0 >= 0 && t0 < T && cols > 0, "gather_tail_rows args");
  const int Tn = T - t0;
  static const int cat = prof_register("gather_tail_rows_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * N * (double)Tn * cols);
  hipLaunchKernelGGL(gather_tail_rows_kernel, dim3(Tn, N), dim3(256), 0, st, dst, ld_dst, src, ld_src, cols, T, t0, Tn);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_init_state_kernel(float* x, const float* z, const int* prompt_len, int B, int C, int T) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C * T) return;
  const int t = (int)(idx % T), b = (int)(idx / ((size_t)T * C));
  x[idx] = t < prompt_len[b] ? 0.0f : z[idx];
}

int cfm_init_state(float* x, const float* z, const int* prompt_len, int B, int C, int T, hipStream_t st) {
  const size_t total = (size_t)B * C * T;
  hipLaunchKernelGGL(cfm_init_state_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, x, z, prompt_len, B, C, T);
  IDX_LAUNCH_CHECK();
  return 0;
}

// block = (t-tile of 64 frames, row b): the tile's mu rows (float4 columns), then the tile's prompt-mel columns t < Tp_max
__global__ __launch_bounds__(256) void cfm_rows_pack_kernel(const CfmRowsPackArgs p) {
  const int b = blockIdx.y, t0 = blockIdx.x * 64;
  const int Tp = p.prompt_len[b], Tg = p.gen_len[b];
  const int nt = min(64, p.T - t0);
  const int W = p.Dc / 4;                   // (Dc % 4 == 0: checked by the caller)
  const f32x4* pc = reinterpret_cast<const f32x4*>(p.pcond[b]);
  const f32x4* gen = reinterpret_cast<const f32x4*>(p.gen + (size_t)(p.gen_row ? p.gen_row[b] : b) * p.Tg_max * p.Dc);
  f32x4* mu = reinterpret_cast<f32x4*>(p.mu + ((size_t)b * p.T + t0) * p.Dc);
  for (int e = threadIdx.x; e < nt * W; e += 256) {
    const int tt = e / W, c = e - tt * W, t = t0 + tt;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t < Tp) v = pc[(size_t)t * W + c];
    else if (t < Tp + Tg) v = gen[(size_t)(t - Tp) * W + c];
    mu[(size_t)tt * W + c] = v;
  }
  if (t0 >= p.Tp_max) return;
  const int np = min(64, p.Tp_max - t0);
  const float* ref = p.ref_mel[b];
  for (int e = threadIdx.x; e < p.C * np; e += 256) {
    const int c = e / np, t = t0 + (e - c * np);
    p.prompt[((size_t)b * p.C + c) * p.Tp_max + t] = t < Tp ? ref[(size_t)c * Tp + t] : 0.0f;
  }
}

int cfm_rows_pack(const CfmRowsPackArgs& a, hipStream_t st) {
  IDX_CHECK(a.mu && a.prompt && a.pcond && a.ref_mel && a.gen && a.prompt_len && a.gen_len, "cfm_rows_pack args");
  IDX_CHECK(a.B > 0 && a.T > 0 && a.Dc > 0 && a.Dc % 4 == 0 && a.Tp_max > 0 && a.Tp_max <= a.T, "cfm_rows_pack shape");
  static const int cat = prof_register("cfm_rows_pack_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * a.B * ((double)a.T * a.Dc + (double)a.C * a.Tp_max));
  hipLaunchKernelGGL(cfm_rows_pack_kernel, dim3(cdiv(a.T, 64), a.B), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_rows_emit_kernel(float* out, const float* x, const int* prompt_len, const int* gen_len, int B,
                                                            int C, int T, int Tg_max) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C * Tg_max) return;
  const int j = (int)(idx % Tg_max);
  const size_t bc = idx / Tg_max;           // = b * C + c
  const int b = (int)(bc / C);
  out[idx] = j < gen_len[b] ? x[bc * T + prompt_len[b] + j] : 0.0f;
}

int cfm_rows_emit(float* out, const float* x, const int* prompt_len, const int* gen_len, int B, int C, int T, int Tg_max, hipStream_t st) {
  IDX_CHECK(out && x && prompt_len && gen_len && B > 0 && C > 0 && Tg_max > 0 && Tg_max <= T, "cfm_rows_emit args");
  const size_t total = (size_t)B * C * Tg_max;
  static const int cat = prof_register("cfm_rows_emit_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * total);
  hipLaunchKernelGGL(cfm_rows_emit_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, out, x, prompt_len, gen_len, B, C, T, Tg_max);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---- per-row schedules: the kernels that go through the solver's row maps (s2mel_ops.h) ----
__global__ __launch_bounds__(256) void cfm_init_state_rows_kernel(float* x, const float* z, const int* prompt_len, const int* order, int B, int C, int T) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C * T) return;
  const int t = (int)(idx % T), b = (int)(idx / ((size_t)T * C));
  x[idx] = t < prompt_len[b] ? 0.0f : z[idx + ((size_t)order[b] - b) * C * T];
}

int cfm_init_state_rows(float* x, const float* z, const int* prompt_len, const int* order, int B, int C, int T, hipStream_t st) {
  IDX_CHECK(x && z && prompt_len && order && B > 0, "cfm_init_state_rows args");
  const size_t total = (size_t)B * C * T;
  hipLaunchKernelGGL(cfm_init_state_rows_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, x, z, prompt_len, order, B, C, T);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_pack_half_kernel(const CfmPackArgs p, const int is_cond, const int* slot, const int* order) {
  // block = (t-tile of 64 frames, row n of the half); the columns are cfm_pack_kernel's
  const int n = blockIdx.y, b = slot ? slot[n] : n;
  const int t0 = blockIdx.x * 64;
  const int W = p.x_only ? p.C : 2 * p.C + p.D + p.S;
  const int Tp = p.prompt_len[b];
  const float* style = p.style + (size_t)order[b] * p.S;
  for (int e = threadIdx.x; e < 64 * W; e += 256) {
    const int tt = e / W, c = e - tt * W;
    const int t = t0 + tt;
    if (t >= p.T) break;
    float v;
    if (c < p.C) v = p.x[((size_t)b * p.C + c) * p.T + t];
    else if (c < 2 * p.C) v = (is_cond && t < Tp) ? p.prompt[((size_t)b * p.C + (c - p.C)) * p.Tp_max + t] : 0.0f;
    else if (c < 2 * p.C + p.D) v = is_cond ? p.cond[((size_t)b * p.T + t) * p.D + (c - 2 * p.C)] : p.cond_null[c - 2 * p.C];
    else v = is_cond ? style[c - 2 * p.C - p.D] : 0.0f;
    p.x_in[((size_t)n * p.T + t) * p.ld + c] = v;
  }
}

int cfm_pack_half(const CfmPackArgs& a, bool is_cond, int N, const int* slot, const int* order, hipStream_t st) {
  IDX_CHECK(a.x_in && a.x && a.prompt_len && order && N > 0 && a.T > 0, "cfm_pack_half args");
  static const int cat = prof_register("cfm_pack_half_kernel");
  ProfScope prof(cat, st, 0.0, 4.0 * N * (double)a.T * (a.x_only ? a.C : 2 * a.C + a.D + a.S) * 2);
  hipLaunchKernelGGL(cfm_pack_half_kernel, dim3(cdiv(a.T, 64), N), dim3(256), 0, st, a, is_cond ? 1 : 0, slot, order);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_gather_consts_kernel(const CfmGatherConstsArgs p) {
  const int n = blockIdx.x, k = blockIdx.y;
  const int cols = p.cols[k];
  const float* s = p.src[k] + (size_t)p.src_row[n] * cols;
  float* d = p.dst[k] + (size_t)n * cols;
  for (int e = threadIdx.x; e < cols; e += 256) d[e] = s[e];
}

int cfm_gather_consts(const CfmGatherConstsArgs& a, hipStream_t st) {
  IDX_CHECK(a.src_row && a.N > 0, "cfm_gather_consts args");
  for (int k = 0; k < 3; ++k) IDX_CHECK(a.dst[k] && a.src[k] && a.cols[k] > 0, "cfm_gather_consts tables");
  static const int cat = prof_register("cfm_gather_consts_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * a.N * ((double)a.cols[0] + a.cols[1] + a.cols[2]));
  hipLaunchKernelGGL(cfm_gather_consts_kernel, dim3(a.N, 3), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_euler_rows_kernel(const CfmEulerRowsArgs p) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.N * p.C * p.T;
  if (idx >= total) return;
  const int t = (int)(idx % p.T);
  const int c = (int)((idx / p.T) % p.C);
  const int b = (int)(idx / ((size_t)p.T * p.C));
  if (t < p.prompt_len[b] || t < p.v_t0) { p.x[idx] = 0.0f; return; }
  const int vT = p.v_T > 0 ? p.v_T : p.T, tv = t - p.v_t0;
  const float vc = p.v[((size_t)b * vT + tv) * p.ldv + c];
  const int bn = p.null_row[b];
  const float dt = p.dt[b];
  if (bn < 0) { p.x[idx] = p.x[idx] + dt * vc; return; }      // no null estimate of this row: dphi_dt = v_cond (flow_matching.py:106)
  const float vn = p.v_null[((size_t)bn * vT + tv) * p.ldv + c];
  const float cfg_rate = p.cfg_rate[b];
  const float dphi = (1.0f + cfg_rate) * vc - cfg_rate * vn;
  p.x[idx] = p.x[idx] + dt * dphi;
}

int cfm_euler_rows(const CfmEulerRowsArgs& a, hipStream_t st) {
  IDX_CHECK(a.x && a.v && a.prompt_len && a.dt && a.cfg_rate && a.null_row && a.N > 0, "cfm_euler_rows args");
  const size_t total = (size_t)a.N * a.C * a.T;
  static const int cat = prof_register("cfm_euler_rows_kernel");
  ProfScope prof(cat, st, 0.0, 16.0 * total);
  hipLaunchKernelGGL(cfm_euler_rows_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
  IDX_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void cfm_rows_emit_map_kernel(float* out, const float* x, const int* prompt_len, const int* gen_len,
                                                                const int* order, int B, int C, int T, int Tg_max) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C * Tg_max) return;
  const int j = (int)(idx % Tg_max);
  const size_t bc = idx / Tg_max;           // = slot * C + c
  const int b = (int)(bc / C), c = (int)(bc - (size_t)b * C);
  out[((size_t)order[b] * C + c) * Tg_max + j] = j < gen_len[b] ? x[bc * T + prompt_len[b] + j] : 0.0f;
}

int cfm_rows_emit_map(float* out, const float* x, const int* prompt_len, const int* gen_len, const int* order, int B, int C, int T, int Tg_max,
                      hipStream_t st) {
  IDX_CHECK(out && x && prompt_len && gen_len && order && B > 0 && C > 0 && Tg_max > 0 && Tg_max <= T, "cfm_rows_emit_map args");
  const size_t total = (size_t)B * C * Tg_max;
  static const int cat = prof_register("cfm_rows_emit_map_kernel");
  ProfScope prof(cat, st, 0.0, 8.0 * total);
  hipLaunchKernelGGL(cfm_rows_emit_map_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, out, x, prompt_len, gen_len, order, B, C, T, Tg_max);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---- GroupNorm(1) + Mish over token-major [B][T][C] with per-sequence valid length ----
__global__ __launch_bounds__(1024) void gn_stats_kernel(const float* x, const int* row_len, int T, int C, float* stats) {
  // one 1024-thread workgroup per sequence: mean, then centred variance (two passes, as torch)
  __shared__ float red[16];
  __shared__ float bc;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t n = (size_t)row_len[b] * C;
  const float* xb = x + (size_t)b * T * C;
  float s = 0.f;
  for (size_t i = tid; i < n; i += 1024) s += xb[i];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) { float a = 0.f; for (int i = 0; i < 16; ++i) a += red[i]; bc = n ? a / (float)n : 0.f; }
  __syncthreads();
  const float mean = bc;
  float ss = 0.f;
  for (size_t i = tid; i < n; i += 1024) { const float c = xb[i] - mean; ss += c * c; }
  ss = wave_sum(ss);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) { float a = 0.f; for (int i = 0; i < 16; ++i) a += red[i]; stats[2 * b] = mean; stats[2 * b + 1] = n ? a / (float)n : 0.f; }
}

__global__ __launch_bounds__(256) void gn_apply_mish_kernel(float* y, const float* x, const float* gamma, const float* beta,
                                                            const int* row_len, const float* stats, int T, int C, float eps) {
  const int m = blockIdx.x;                 // row = (b, t)
  const int b = m / T, t = m - b * T;
  const bool valid = t < row_len[b];
  const float mean = stats[2 * b], rstd = rsqrtf(stats[2 * b + 1] + eps);
  for (int c = threadIdx.x; c < C; c += 256) {
    float o = 0.0f;
    if (valid) {
      const float v = (x[(size_t)m * C + c] - mean) * rstd * gamma[c] + beta[c];
      const float sp = v > 20.0f ? v : log1pf(expf(v));      // torch softplus threshold
      o = v * tanhf(sp);
    }
    y[(size_t)m * C + c] = o;
  }
}

int groupnorm1_mish(float* y, const float* x, const float* gamma, const float* beta, const int* row_len, int B, int T, int C,
                    float eps, float* stats, hipStream_t st) {
  static const int cat = prof_register("gn_stats_kernel + gn_apply_mish_kernel");
  ProfScope prof(cat, st, 0.0, 12.0 * B * (double)T * C);
  hipLaunchKernelGGL(gn_stats_kernel, dim3(B), dim3(1024), 0, st, x, row_len, T, C, stats);
  hipLaunchKernelGGL(gn_apply_mish_kernel, dim3(B * T), dim3(256), 0, st, y, x, gamma, beta, row_len, stats, T, C, eps);
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
