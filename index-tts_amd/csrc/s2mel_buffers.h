// The workspace of the CFM solver (s2mel.hip): ONE table of its buffers.  carve_cfm lays them out from it, half_view takes from it
// which of them one CFG half owns.  Pointer arithmetic only, no HIP call (tools/s2mel_buffers_check.cpp runs it on the CPU).
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/idxtts.h"
#include "model_util.h"

namespace idxtts {

struct CfmBuffers {
  float *x_in, *ha, *hb, *hmid, *hn, *qkv, *att, *ff, *xres, *wn_x, *wn_acts, *wn_out, *vout, *condp, *xstate;
  void *hn_p, *att_p, *ff_p, *acts_p;     // split-bf16 planes of hn / att / ff / wn_acts (producers write them for the next GEMM)
  void *h_p, *wnx_p, *xres_p;             // planes of the residual stream entering a skip-receive layer, of wn_x, of xres
  std::vector<void*> skips_p;             // planes of the U-ViT skip tensors
  std::vector<float*> skips;
  float *t1, *t1s, *mods, *fmod, *t2, *wnb, *tmp_steps;
  int *lens2, *plen, *lens2t;      // lens2t: lens2 - tail_t0
  int tail_t0 = 0;                 // first frame the post-transformer part is evaluated on (0 = every frame)
  size_t bytes;
};

// What an entry of the table counts its rows in.  An element is 4 bytes in every kind: a float, an int, or hi + lo bf16.
enum CfmKind {
  CFM_ROWS,     // fp32 [(sequence, frame)][cols]
  CFM_PLANES,   // split-bf16 planes of such rows: [hi | lo][cols / 16][rows][16]
  CFM_STEPS,    // per-call constants [n_steps][cols]: the t-only vectors of every Euler step
  CFM_INTS,     // one int per sequence
};
// HALVED: the buffer holds the stacked [conditional | null] batch of 2B sequences, and half h owns the block of B sequences at
// h * B*T*cols elements -- planes too: a half's planes [cols / 16][B*T][16] are B*T*cols elements, laid out with rows = B*T.
// SHARED: B sequences (or n_steps rows) that both halves read where they stand.
constexpr bool CFM_HALVED = true, CFM_SHARED = false;

// elements of ONE half's block (of the whole buffer when it is shared)
inline size_t cfm_block_elems(int B, int T, int n_steps, CfmKind kind, size_t cols) {
  return cols * (kind == CFM_STEPS ? (size_t)n_steps : kind == CFM_INTS ? (size_t)B : (size_t)B * T);
}

// THE table: f(member, columns per row, kind, halved) for every buffer, in workspace order
template <typename F> void cfm_buffer_table(CfmBuffers& b, const idxtts_s2mel_config& c, int ffn, F&& f) {
  const int D = c.hidden_dim, C = c.in_channels, Wh = c.wn_hidden;
  const CfmKind R = CFM_ROWS, P = CFM_PLANES, S = CFM_STEPS;
  const bool H = CFM_HALVED;
  f(b.x_in, 2 * C + D + c.style_dim, R, H); f(b.ha, D, R, H); f(b.hb, D, R, H); f(b.hmid, D, R, H); f(b.hn, D, R, H);
  f(b.qkv, 3 * D, R, H); f(b.att, D, R, H); f(b.ff, ffn, R, H); f(b.xres, D, R, H);
  f(b.hn_p, std::max(D, Wh), P, H); f(b.att_p, D, P, H); f(b.ff_p, ffn, P, H); f(b.acts_p, Wh, P, H);
  f(b.h_p, D, P, H); f(b.wnx_p, Wh, P, H); f(b.xres_p, D, P, H);
  f(b.wn_x, Wh, R, H); f(b.wn_acts, Wh, R, H); f(b.wn_out, Wh, R, H); f(b.vout, C, R, H);
  f(b.condp, D, R, CFM_SHARED);       // cond_projection(mu); the null half reads the projection's bias instead
  f(b.xstate, C, R, CFM_SHARED);      // the ODE state [B][C][T]
  for (float*& s : b.skips) f(s, D, R, H);
  for (void*& s : b.skips_p) f(s, D, P, H);
  f(b.t1, D, S, CFM_SHARED); f(b.t1s, D, S, CFM_SHARED); f(b.tmp_steps, std::max(D, Wh), S, CFM_SHARED);
  f(b.mods, (2 * c.depth + 1) * 2 * D, S, CFM_SHARED); f(b.fmod, 2 * Wh, S, CFM_SHARED); f(b.t2, Wh, S, CFM_SHARED);
  f(b.wnb, c.wn_layers * 2 * Wh, S, CFM_SHARED);
  f(b.lens2, 1, CFM_INTS, H); f(b.plen, 1, CFM_INTS, CFM_SHARED); f(b.lens2t, 1, CFM_INTS, H);
}

template <typename T> inline void cfm_take(T*& p, Carver& k, size_t n) { p = k.take<T>(n); }
inline void cfm_take(void*& p, Carver& k, size_t n) { p = k.take<float>(n); }
template <typename T> inline void cfm_advance(T*& p, size_t n) { p += n; }
inline void cfm_advance(void*& p, size_t n) { p = static_cast<float*>(p) + n; }

// ws == nullptr: the byte total alone (every pointer null)
inline CfmBuffers carve_cfm(const idxtts_s2mel_config& c, int ffn, void* ws, int B, int T, int n_steps) {
  CfmBuffers b;
  b.skips.resize(c.depth / 2);
  b.skips_p.resize(c.depth / 2);
  Carver k(ws);
  cfm_buffer_table(b, c, ffn, [&](auto*& p, size_t cols, CfmKind kind, bool halved) {
    cfm_take(p, k, (halved ? 2 : 1) * cfm_block_elems(B, T, n_steps, kind, cols));
  });
  b.bytes = (k.off + 255) & ~(size_t)255;
  return b;
}

// The buffers of ONE half (h = 0 conditional, 1 null) of the stacked batch.  The two halves never read each other's rows between
// cfm_pack and the Euler update, which is what lets them run on two streams (s2mel.hip: dit_eval_halves).
inline CfmBuffers half_view(const idxtts_s2mel_config& c, int ffn, const CfmBuffers& w, int h, int B, int T) {
  CfmBuffers v = w;
  cfm_buffer_table(v, c, ffn, [&](auto*& p, size_t cols, CfmKind kind, bool halved) {
    if (halved) cfm_advance(p, h * cfm_block_elems(B, T, 0, kind, cols));
  });
  return v;
}

// The t-only constants of the steps from row `first` on: a call with several schedules keeps them one block after the other, and
// computes and reads each block as a call of that schedule alone would.
inline CfmBuffers steps_view(const idxtts_s2mel_config& c, int ffn, const CfmBuffers& w, int first) {
  CfmBuffers v = w;
  cfm_buffer_table(v, c, ffn, [&](auto*& p, size_t cols, CfmKind kind, bool) {
    if (kind == CFM_STEPS) cfm_advance(p, (size_t)first * cols);
  });
  return v;
}

// Per-row schedules (S2MelModel::cfm_sched), behind the solver's and the row pack's buffers.  The solver keeps its rows in an order of
// its own, slot i = the caller's row order[i], in which the live rows of each CFG half are a prefix at every iteration.
struct CfmSchedBuffers {
  float *mods[2], *fmod[2], *wnb[2];   // per half: the step constants of each live row's own schedule, [B][cols], gathered per iteration
  int *order;                          // [B] caller's row of slot i
  int *null_slot, *null_row;           // [B] slot of null-half row j; null-half row of slot i (-1: the row has no null estimate)
  int *src_row[2];                     // per half [max steps][B]: the row of the step-constant blocks that row n reads at iteration s
  float *dt, *cfg_rate;                // [max steps][B] dt of slot i at iteration s; [B] guidance rate of slot i
  size_t bytes;                        // end of the block, from the workspace's start
};

inline CfmSchedBuffers carve_cfm_sched(const idxtts_s2mel_config& c, void* ws, size_t base, int B, int max_steps) {
  CfmSchedBuffers b;
  Carver k(ws ? static_cast<char*>(ws) + base : nullptr);
  for (int h = 0; h < 2; ++h) {
    b.mods[h] = k.take<float>((size_t)B * (2 * c.depth + 1) * 2 * c.hidden_dim);
    b.fmod[h] = k.take<float>((size_t)B * 2 * c.wn_hidden);
    b.wnb[h] = k.take<float>((size_t)B * c.wn_layers * 2 * c.wn_hidden);
    b.src_row[h] = k.take<int>((size_t)max_steps * B);
  }
  b.order = k.take<int>(B);
  b.null_slot = k.take<int>(B);
  b.null_row = k.take<int>(B);
  b.dt = k.take<float>((size_t)max_steps * B);
  b.cfg_rate = k.take<float>(B);
  b.bytes = base + ((k.off + 255) & ~(size_t)255);
  return b;
}

}  // namespace idxtts
