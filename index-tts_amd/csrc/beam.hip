// Beam search / beam-sample step kernels (see beam.h).  Reference semantics: vendored GenerationMixin._beam_search
// (indextts/gpt/transformers_generation_utils.py:3325-3516), BeamSearchScorer.process and BeamHypotheses
// (indextts/gpt/transformers_beam_search.py:215-318, 930-1013), logits warpers with min_tokens_to_keep = 2 (1022-1043),
// cache re-indexing `_reorder_cache` (indextts/gpt/model_v2.py:227-240) -- the mode IndexTTS2.infer runs by default
// (infer_v2.py:714-722, 767: do_sample=True, num_beams=3).
//
// The reference re-indexes the WHOLE KV cache of all 24 layers with index_select every step (3 x the prompt + everything
// generated).  Here the beams of an utterance share their prompt rows by construction (identical inputs -> identical
// K/V), so only the generated positions move, in place, and not at all when the step kept every beam where it was.
#include <cmath>

#include "beam.h"
#include "device_util.h"
#include "prof.h"

namespace idxtts {

namespace {

constexpr int NPT = 16;          // vocabulary entries per thread of a 1024-thread block: V <= 16384
// Survivors of the top-k filter that the top-p stage can sort.  check_beam requires 0 < top_k <= 1024 with top_p < 1, so more survive
// only when more than CAP - top_k + 1 scores tie exactly at the top-k threshold; that group is one value in index order and needs no
// sorting: it is then walked by count, and only the (fewer than top_k) scores above the threshold are staged.
constexpr int CAP = 2048;
constexpr int SEL_EPT = 32;      // beam_select: candidates per thread kept in registers (nb * V <= 32768), else the re-reading loop

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// SESSION (beam decode session, beam.h): block -> row nb * g + j of group g (group_ids[blockIdx.x / nb] at an admission), the request's
// parameters from group[g]; a group that is not live returns at once
template <bool SESSION>
__global__ __launch_bounds__(1024) void beam_scores_kernel(const BeamState p) {
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ float sval[CAP];
  __shared__ int sidx[CAP];
  __shared__ float sorted_v[CAP];
  __shared__ int sorted_i[CAP];
  __shared__ int s_count, s_thr_i, s_digit, s_kk, s_tie_skip;
  __shared__ int hist[16][256];
  __shared__ float s_thr_v;
  const int tid = threadIdx.x, V = p.V;
  int r = blockIdx.x, do_sample = p.do_sample, top_k = p.top_k;
  float temperature = p.temperature, top_p = p.top_p;
  if constexpr (SESSION) {
    const int g = p.group_ids ? p.group_ids[blockIdx.x / p.nb] : blockIdx.x / p.nb;
    r = g * p.nb + blockIdx.x % p.nb;
    if (!p.slots[g * p.nb].live) return;
    const SlotBeam& gb = p.group[g];
    do_sample = gb.do_sample; top_k = gb.top_k; temperature = gb.temperature; top_p = gb.top_p;
  } else {
    if (p.done[r / p.nb]) return;
  }
  const float* lrow = p.logits + (size_t)r * V;
  const unsigned char* seen = p.seen + (size_t)r * V;
  float sc[NPT];
  float mx = -INFINITY; int mi = 0;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int v = tid + 1024 * u;
    sc[u] = v < V ? lrow[v] : -INFINITY;
    if (sc[u] > mx) { mx = sc[u]; mi = v; }
  }
  block_argmax<16>(mx, mi, rv, ri, tid);
  float part = 0.f;
#pragma unroll
  for (int u = 0; u < NPT; ++u) if (tid + 1024 * u < V) part += expf(sc[u] - mx);
  const float lse = logf(block_sum<16>(part, rv));
  // log_softmax (fp32, before the processors: transformers_generation_utils.py:3473-3477), repetition penalty, temperature
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int v = tid + 1024 * u;
    if (v < V) {
      float s = (sc[u] - mx) - lse;
      if (p.penalty != 1.0f && seen[v]) s = s < 0.f ? s * p.penalty : s / p.penalty;
      if (do_sample && temperature != 1.0f) s = s / temperature;
      sc[u] = s;
    }
  }
  if (do_sample && (top_k > 0 || top_p < 1.0f)) {
    const int k = top_k > 0 ? max(top_k, 2) : 0;         // TopKLogitsWarper: max(top_k, min_tokens_to_keep)
    float kth = -INFINITY;
    if (k > 0 && k < V) {
      // the k-th largest score by a radix select over order-preserving 32-bit keys (four 8-bit digits, high to low): per-wave
      // histograms in LDS, one wave walks the 256 bins from the top -- 16 barriers in all instead of 2 k block-wide argmax rounds
      unsigned key[NPT];
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const unsigned b = __float_as_uint(sc[u] + 0.0f);      // (+ 0: -0 and +0 are one value to `<`)
        key[u] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      }
      unsigned prefix = 0;
      int kk = k;
      const int wv = tid >> 6, ln = tid & 63;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
#pragma unroll
        for (int j = 0; j < 4; ++j) (&hist[0][0])[tid + 1024 * j] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NPT; ++u)
          if (tid + 1024 * u < V && (pass == 0 || (key[u] >> (shift + 8)) == prefix)) atomicAdd(&hist[wv][(key[u] >> shift) & 255u], 1);
        __syncthreads();
        if (tid < 256) {
          int t = 0;
#pragma unroll
          for (int w = 0; w < 16; ++w) t += hist[w][tid];
          hist[0][tid] = t;
        }
        __syncthreads();
        if (wv == 0) {      // lane l owns bins 4 l .. 4 l + 3; `above` = the count in every bin of a higher lane
          int c[4], mine = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) { c[j] = hist[0][4 * ln + j]; mine += c[j]; }
          int incl = mine;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(incl, off);
            if (ln + off < 64) incl += o;
          }
          int a = incl - mine;
          if (a < kk && kk <= incl) {
#pragma unroll
            for (int j = 3; j >= 0; --j) {
              if (a + c[j] >= kk) { s_digit = 4 * ln + j; s_kk = kk - a; break; }
              a += c[j];
            }
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned)s_digit;
        kk = s_kk;
      }
      const unsigned kb = (prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix;
      kth = __uint_as_float(kb);
#pragma unroll
      for (int u = 0; u < NPT; ++u) if (sc[u] < kth) sc[u] = -INFINITY;
    }
    if (top_p < 1.0f) {
      if (tid == 0) s_count = 0;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int v = tid + 1024 * u;
        if (v < V && sc[u] > -INFINITY) {
          const int slot = atomicAdd(&s_count, 1);
          if (slot < CAP) { sval[slot] = sc[u]; sidx[slot] = v; }
        }
      }
      __syncthreads();
      const int total = s_count;
      int n = total, m = 0;      // n staged entries; m entries of the tie group at the threshold, counted instead
      if (total > CAP) {         // (block-uniform) only the scores above the threshold are staged: fewer than k <= 1024
        __syncthreads();
        if (tid == 0) s_count = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
          const int v = tid + 1024 * u;
          if (v < V && sc[u] > kth) {
            const int slot = atomicAdd(&s_count, 1);
            if (slot < CAP) { sval[slot] = sc[u]; sidx[slot] = v; }
          }
        }
        __syncthreads();
        n = min(s_count, CAP); m = total - s_count;
      }
      for (int e = tid; e < n; e += 1024) {        // rank sort, ascending by (value, index)
        const float ve = sval[e]; const int ie = sidx[e];
        int rank = 0;
        for (int o = 0; o < n; ++o) rank += (sval[o] < ve || (sval[o] == ve && sidx[o] < ie)) ? 1 : 0;
        sorted_v[rank] = ve; sorted_i[rank] = ie;
      }
      __syncthreads();
      if (tid == 0) {      // TopPLogitsWarper, min_tokens_to_keep = 2: remove while cum <= 1 - top_p, never the last two
        // ascending order: the m tied entries by index, then the n staged ones
        const int N = n + m;
        int keep_from = 0;
        const float top = n > 0 ? sorted_v[n - 1] : kth;
        const float pt = m > 0 ? expf(kth - top) : 0.f;
        float tot = (float)m * pt;
        for (int e = 0; e < n; ++e) tot += expf(sorted_v[e] - top);
        const float thr = (float)(1.0 - (double)top_p);
        float cum = 0.f;
        if (m > 0) {       // j tied entries sum to j * pt / tot: the largest j with that at or below thr
          const float each = pt / tot;
          int j = min((int)fminf(thr / each, (float)m), min(m, N - 2));
          while (j < min(m, N - 2) && (float)(j + 1) * each <= thr) ++j;
          while (j > 0 && (float)j * each > thr) --j;
          keep_from = j; cum = (float)j * each;
        }
        if (keep_from == m) {
          for (int e = m; e < N - 2; ++e) {
            cum += expf(sorted_v[e - m] - top) / tot;
            if (cum <= thr) keep_from = e + 1; else break;
          }
        }
        if (keep_from < m) { s_thr_v = kth; s_thr_i = 0; s_tie_skip = keep_from; }
        else { s_thr_v = sorted_v[keep_from - m]; s_thr_i = sorted_i[keep_from - m]; s_tie_skip = -1; }
      }
      __syncthreads();
      if (s_tie_skip > 0) {      // (block-uniform) the index below which exactly s_tie_skip tied entries lie: bisection on the count
        const int want = s_tie_skip;
        int lo = 0, hi = V;        // the count below lo is < want, the count below hi is >= want
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          float c = 0.f;
#pragma unroll
          for (int u = 0; u < NPT; ++u) c += (sc[u] == kth && tid + 1024 * u < mid) ? 1.f : 0.f;
          if (block_sum<16>(c, rv) >= (float)want) hi = mid; else lo = mid;
        }
        __syncthreads();
        if (tid == 0) s_thr_i = hi;
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int v = tid + 1024 * u;
        if (sc[u] < s_thr_v || (sc[u] == s_thr_v && v < s_thr_i)) sc[u] = -INFINITY;
      }
    }
  }
  const float bs = p.beam_scores[r];
  float* out = p.proc + (size_t)r * V;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int v = tid + 1024 * u;
    if (v < V) out[v] = sc[u] + bs;
  }
}

int beam_scores_forward(const BeamState& s, hipStream_t st) {
  IDX_CHECK(s.logits && s.proc && s.seen && s.beam_scores && s.done, "null pointer");
  IDX_CHECK(s.V > 0 && s.V <= 1024 * NPT && s.nb >= 2 && s.nb <= BEAM_MAX, "beam shape");
  static const int cat = prof_register("beam_scores_kernel");
  const int groups = s.slots && s.group_ids ? s.n_ids : s.B;
  ProfScope prof(cat, st, 0.0, 8.0 * groups * s.nb * (double)s.V);
  if (s.slots) {
    IDX_CHECK(s.group, "null pointer");
    hipLaunchKernelGGL(beam_scores_kernel<true>, dim3(groups * s.nb), dim3(1024), 0, st, s);
  } else {
    hipLaunchKernelGGL(beam_scores_kernel<false>, dim3(s.B * s.nb), dim3(1024), 0, st, s);
  }
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// SESSION: block -> group g (group_ids[blockIdx.x] at an admission); n = the group's step, the request's parameters and draws
// (its own exp_noise row n, or the seed's stream at row 0 of a B-group generate_beam); a group that is not live returns at once
template <bool SESSION>
__global__ __launch_bounds__(1024) void beam_select_kernel(const BeamState p) {
  __shared__ float rv[16];
  __shared__ int ri[16];
  __shared__ int cand_i[2 * BEAM_MAX];
  __shared__ float cand_s[2 * BEAM_MAX];
  __shared__ int cp_slot[BEAM_MAX], cp_src[BEAM_MAX], n_cp;
  const int tid = threadIdx.x, nb = p.nb, V = p.V, N = nb * V;
  int b = blockIdx.x, n, do_sample = p.do_sample, early_stopping = p.early_stopping;
  const float* exp_noise = p.exp_noise;
  unsigned long long seed = p.seed;
  double length_penalty = p.length_penalty;
  size_t nbase;
  if constexpr (SESSION) {
    if (p.group_ids) b = p.group_ids[blockIdx.x];
    const SlotState& ss = p.slots[b * nb];
    if (!ss.live) return;
    n = ss.step;
    const SlotBeam& gb = p.group[b];
    do_sample = gb.do_sample; early_stopping = gb.early_stopping; exp_noise = gb.exp_noise; seed = gb.seed;
    length_penalty = gb.length_penalty;
    nbase = (exp_noise || p.invariant) ? (size_t)n * N : (size_t)n * p.B * N;
  } else {
    n = p.st->step;                           // tokens each live beam holds before this step
    if (p.done[b]) {                          // BeamSearchScorer.process pads a finished utterance
      if (tid < nb) { p.next_tok[b * nb + tid] = p.stop_token; p.beam_idx[b * nb + tid] = b * nb + tid; p.beam_scores[b * nb + tid] = 0.f; }
      return;
    }
    nbase = ((size_t)n * p.B + b) * N;
    if (p.invariant && !exp_noise) { nbase = (size_t)n * N; seed += DRAW_ROW_STRIDE * (unsigned long long)b; }
  }
  const float* base = p.proc + (size_t)b * N;
  const int n_keep = 2 * nb;
  // multinomial without replacement = the n_keep largest probs / q (ATen: q ~ Exp(1) once per element, then topk); plain
  // top-k of the scores when not sampling.  Equal keys go to the smaller flat index: the zero-probability fillers of a step with fewer
  // than n_keep survivors, and in beam search the bit-equal scores of beams that hold the same tokens in another order ([a, b] and
  // [b, a] at step 2) -- that rule and the stable sort below decide which of them becomes which beam.
  if (N <= 1024 * SEL_EPT) {
    // every element's key is computed ONCE and stays in registers (the exponential, the division and the draw are the cost of a
    // round); a round is then a masked scan of SEL_EPT registers and one block-wide argmax
    float ks[SEL_EPT];
    float mx = -INFINITY; int mi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e) {
      const int i = tid + 1024 * e;
      ks[e] = i < N ? base[i] : -INFINITY;
      if (i < N && (ks[e] > mx || (ks[e] == mx && i < mi))) { mx = ks[e]; mi = i; }
    }
    block_argmax<16>(mx, mi, rv, ri, tid);
    if (do_sample) {
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < SEL_EPT; ++e) if (tid + 1024 * e < N) part += expf(ks[e] - mx);
      const float tot = block_sum<16>(part, rv);
#pragma unroll
      for (int e = 0; e < SEL_EPT; ++e) {
        const int i = tid + 1024 * e;
        if (i < N) ks[e] = (expf(ks[e] - mx) / tot) / exp1_draw(exp_noise, seed, nbase + i);
      }
    }
    unsigned taken = 0;
    for (int c = 0; c < n_keep; ++c) {
      float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < SEL_EPT; ++e) {
        const int i = tid + 1024 * e;
        if (i < N && !((taken >> e) & 1u) && (ks[e] > best || (ks[e] == best && i < bi))) { best = ks[e]; bi = i; }
      }
      block_argmax<16>(best, bi, rv, ri, tid);
      if (bi < N && (bi & 1023) == tid) taken |= 1u << (bi >> 10);
      if (tid == 0) { cand_i[c] = bi; cand_s[c] = base[bi]; }
    }
    __syncthreads();
  } else {
    float mx = -INFINITY; int mi = 0x7fffffff;
    for (int i = tid; i < N; i += 1024) { const float x = base[i]; if (x > mx || (x == mx && i < mi)) { mx = x; mi = i; } }
    block_argmax<16>(mx, mi, rv, ri, tid);
    float tot = 1.0f;
    if (do_sample) {
      float part = 0.f;
      for (int i = tid; i < N; i += 1024) part += expf(base[i] - mx);
      tot = block_sum<16>(part, rv);
    }
    for (int c = 0; c < n_keep; ++c) {
      float best = -INFINITY; int bi = 0x7fffffff;
      for (int i = tid; i < N; i += 1024) {
        bool taken = false;
        for (int o = 0; o < c; ++o) taken = taken || cand_i[o] == i;
        if (taken) continue;
        const float x = base[i];
        const float key = do_sample ? (expf(x - mx) / tot) / exp1_draw(exp_noise, seed, nbase + i) : x;
        if (key > best || (key == best && i < bi)) { best = key; bi = i; }
      }
      block_argmax<16>(best, bi, rv, ri, tid);
      if (tid == 0) { cand_i[c] = bi; cand_s[c] = base[bi]; }
      __syncthreads();
    }
  }
  if (tid == 0) {
    // candidates by score, descending (transformers_generation_utils.py:3511-3513; stable)
    for (int a = 1; a < n_keep; ++a) {
      const int ci = cand_i[a]; const float cs = cand_s[a];
      int o = a - 1;
      while (o >= 0 && cand_s[o] < cs) { cand_i[o + 1] = cand_i[o]; cand_s[o + 1] = cand_s[o]; --o; }
      cand_i[o + 1] = ci; cand_s[o + 1] = cs;
    }
    double* hs = p.hyp_score + (size_t)b * (BEAM_MAX + 1);
    int* hl = p.hyp_len + (size_t)b * (BEAM_MAX + 1);
    int* hslot = p.hyp_slot + (size_t)b * (BEAM_MAX + 1);
    int hn = p.hyp_n[b];
    double worst = p.hyp_worst[b];
    const int gen_len = n + 1;                                  // cur_len - decoder_prompt_len
    const double denom = pow((double)gen_len, length_penalty);
    int slot = 0, ncp = 0;
    for (int rank = 0; rank < n_keep && slot < nb; ++rank) {
      const int tok = cand_i[rank] % V, src = b * nb + cand_i[rank] / V;
      const float sc = cand_s[rank];
      if (tok == p.stop_token) {
        if (rank >= nb) continue;                               // not among the top num_beams: dropped
        const double score = (double)sc / denom;                // BeamHypotheses.add
        if (hn < nb || score > worst) {
          bool used[BEAM_MAX + 1];
          for (int q = 0; q <= nb; ++q) used[q] = false;
          for (int q = 0; q < hn; ++q) used[hslot[q]] = true;
          int phys = 0;
          while (used[phys]) ++phys;
          hs[hn] = score; hl[hn] = n; hslot[hn] = phys; ++hn;
          cp_slot[ncp] = phys; cp_src[ncp] = src; ++ncp;
          if (hn > nb) {                                        // drop the worst (smallest score, then earliest)
            int wi = 0;
            for (int q = 1; q < hn; ++q) if (hs[q] < hs[wi]) wi = q;
            for (int q = wi; q + 1 < hn; ++q) { hs[q] = hs[q + 1]; hl[q] = hl[q + 1]; hslot[q] = hslot[q + 1]; }
            --hn;
            worst = hs[0];
            for (int q = 1; q < hn; ++q) worst = fmin(worst, hs[q]);
          } else {
            worst = fmin(score, worst);
          }
        }
      } else {
        p.beam_scores[b * nb + slot] = sc; p.next_tok[b * nb + slot] = tok; p.beam_idx[b * nb + slot] = src;
        ++slot;
      }
    }
    p.hyp_n[b] = hn; p.hyp_worst[b] = worst;
    n_cp = ncp;
    // BeamHypotheses.is_done with the best candidate of this step
    bool fin = false;
    if (hn >= nb) fin = early_stopping ? true : worst >= (double)cand_s[0] / denom;
    if (fin) p.done[b] = 1;
  }
  __syncthreads();
  for (int c = 0; c < n_cp; ++c) {
    const int* src = p.seq + (size_t)cp_src[c] * p.seq_ld;
    int* dst = p.hyp_seq + ((size_t)b * (BEAM_MAX + 1) + cp_slot[c]) * p.seq_ld;
    for (int t = tid; t < n; t += 1024) dst[t] = src[t];
  }
}

int beam_select_forward(const BeamState& s, hipStream_t st) {
  IDX_CHECK(s.proc && s.next_tok && s.beam_idx && s.seq && s.hyp_score && s.hyp_len && s.hyp_slot && s.hyp_seq && s.hyp_n && s.hyp_worst &&
            (s.st || s.slots), "null pointer");
  if (s.slots) hipLaunchKernelGGL(beam_select_kernel<true>, dim3(s.group_ids ? s.n_ids : s.B), dim3(1024), 0, st, s);
  else hipLaunchKernelGGL(beam_select_kernel<false>, dim3(s.B), dim3(1024), 0, st, s);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// SESSION: block -> group; a group that is not live returns at once, a group the scorer has just finished ends (live = 0 and step = the
// steps taken, on all its slots).  Otherwise the re-indexing and the new tokens as below, then the fused tail: the group ends at its
// cap, or each of its rows gets its next input row (slot_tail's write, sample_slots) and its slots advance.
template <bool SESSION>
__global__ __launch_bounds__(1024) void beam_reorder_rows_kernel(const BeamState p) {
  const int tid = threadIdx.x, nb = p.nb, V = p.V;
  int b = blockIdx.x, n, mp = 0, max_step = 0;
  if constexpr (SESSION) {
    if (p.group_ids) b = p.group_ids[blockIdx.x];
    const SlotState ss = p.slots[b * nb];      // read by every thread before the barrier below; written after it
    if (!ss.live) return;
    n = ss.step; mp = ss.mel_pos; max_step = ss.max_step;
    if (p.done[b]) {
      __syncthreads();
      if (tid < nb) { p.slots[b * nb + tid].live = 0; p.slots[b * nb + tid].step = n + 1; }
      return;
    }
  } else {
    n = p.st->step;
    if (p.done[b]) {
      if (tid < nb) { p.cur_tok[b * nb + tid] = p.stop_token; if (n < p.seq_ld) p.seq[(size_t)(b * nb + tid) * p.seq_ld + n] = p.stop_token; }
      return;
    }
  }
  int src[BEAM_MAX];
  bool identity = true;
  for (int j = 0; j < nb; ++j) { src[j] = p.beam_idx[b * nb + j]; identity = identity && src[j] == b * nb + j; }
  if (!identity) {      // a thread owns one column of all nb rows: reads every source before it writes (in place)
    for (int t = tid; t < n; t += 1024) {
      int v[BEAM_MAX];
      for (int j = 0; j < nb; ++j) v[j] = p.seq[(size_t)src[j] * p.seq_ld + t];
      for (int j = 0; j < nb; ++j) p.seq[(size_t)(b * nb + j) * p.seq_ld + t] = v[j];
    }
    for (int t = tid; t < V; t += 1024) {
      unsigned char v[BEAM_MAX];
      for (int j = 0; j < nb; ++j) v[j] = p.seen[(size_t)src[j] * V + t];
      for (int j = 0; j < nb; ++j) p.seen[(size_t)(b * nb + j) * V + t] = v[j];
    }
  }
  __syncthreads();
  if (tid < nb) {
    const int r = b * nb + tid, tok = p.next_tok[r];
    p.seq[(size_t)r * p.seq_ld + n] = tok;
    p.seen[(size_t)r * V + tok] = 1;
    p.cur_tok[r] = tok;
  }
  if constexpr (SESSION) {
    SlotState* const ss = p.slots + b * nb;
    if (n + 1 >= max_step) {      // the request's cap: the open beams are final (finalize reads them with step = cap)
      if (tid < nb) { ss[tid].live = 0; ss[tid].step = n + 1; }
      return;
    }
    const int R = p.B * nb;
    for (int j = 0; j < nb; ++j) {
      const int r = b * nb + j, tok = p.next_tok[r];
      if (p.x_frag) {
        const int d = p.d;
        for (int e = tid; e < d; e += 1024) p.x_frag[frag_index(r, e, d >> 4)] = p.mel_emb[(size_t)tok * d + e] + p.mel_pos[(size_t)(mp + 1) * d + e];
      } else {
        embed_row_pl<1024>(p.x_row, p.x_stats, r, R, p.d, p.mel_emb, p.mel_pos, tok, mp + 1, tid);
      }
    }
    if (tid < nb) { ss[tid].pos += 1; ss[tid].mel_pos += 1; ss[tid].step += 1; }      // the group's own scalars: read by nobody else
  }
}

// KV rows of the generated positions [prompt_len, pos]: granules of type GT (G per key: 16 x 16 bytes in a fp32 cache, 8 x 16 in a bf16
// one, 8 x 8 in an fp8 one), a thread moves one granule of all nb beams; an fp8 cache's scales of the same positions move with the
// same ancestry
// SESSION: blockIdx.y -> group; nothing moves for a group that is not live, has just finished or is at its cap.  The range starts at
// pos - step + 1 = P_g + 1 (admission: pos = P_g, step 0), so npos = step.
template <bool SESSION, class GT>
__global__ __launch_bounds__(256) void beam_reorder_kv_kernel(const BeamState p) {
  const int nb = p.nb;
  int b = blockIdx.y, pos, prompt_len;
  if constexpr (SESSION) {
    const SlotState ss = p.slots[b * nb];
    if (!ss.live || p.done[b] || ss.step + 1 >= ss.max_step) return;
    pos = ss.pos; prompt_len = ss.pos - ss.step + 1;
  } else {
    if (p.done[b]) return;
  }
  int src[BEAM_MAX];
  bool identity = true;
  for (int j = 0; j < nb; ++j) { src[j] = p.beam_idx[b * nb + j]; identity = identity && src[j] == b * nb + j; }
  if (identity) return;
  if constexpr (!SESSION) { pos = p.st->pos; prompt_len = p.prompt_len; }      // position written by this step's attention
  const int npos = pos - prompt_len + 1;
  if (npos <= 0) return;
  const int R = p.B * nb, H = p.H, Smax = p.Smax, G = p.kv_gran;
  GT* const kc = static_cast<GT*>(p.kcache);
  GT* const vc = static_cast<GT*>(p.vcache);
  const long items = (long)p.L * H * G * npos;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const int lh = (int)(it / (G * npos)), rem = (int)(it - (long)lh * G * npos);
    const int l = lh / H, h = lh - l * H;
    {   // K: [L][R][H][G][Smax] granules
      const int c = rem / npos, s = prompt_len + (rem - c * npos);
      GT v[BEAM_MAX];
      for (int j = 0; j < nb; ++j) v[j] = kc[((((size_t)l * R + src[j]) * H + h) * G + c) * Smax + s];
      for (int j = 0; j < nb; ++j) kc[((((size_t)l * R + b * nb + j) * H + h) * G + c) * Smax + s] = v[j];
    }
    {   // V: [L][R][H][Smax][G] granules
      const int s = prompt_len + rem / G, k = rem - (rem / G) * G;
      GT v[BEAM_MAX];
      for (int j = 0; j < nb; ++j) v[j] = vc[((((size_t)l * R + src[j]) * H + h) * Smax + s) * G + k];
      for (int j = 0; j < nb; ++j) vc[((((size_t)l * R + b * nb + j) * H + h) * Smax + s) * G + k] = v[j];
    }
  }
  if constexpr (sizeof(GT) == 8) {      // the fp8 cache (8-byte granules): its scales [L][R][H][Smax], K and V
    const long sitems = (long)p.L * H * npos;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < sitems; it += (long)gridDim.x * 256) {
      const int lh = (int)(it / npos), s = prompt_len + (int)(it - (long)lh * npos);
      const int l = lh / H, h = lh - l * H;
      float kv[BEAM_MAX], vv[BEAM_MAX];
      for (int j = 0; j < nb; ++j) {
        const size_t at = (((size_t)l * R + src[j]) * H + h) * Smax + s;
        kv[j] = p.kscale[at]; vv[j] = p.vscale[at];
      }
      for (int j = 0; j < nb; ++j) {
        const size_t at = (((size_t)l * R + b * nb + j) * H + h) * Smax + s;
        p.kscale[at] = kv[j]; p.vscale[at] = vv[j];
      }
    }
  }
}

// the launch for the cache's granule width
template <bool SESSION>
static void launch_beam_reorder_kv(const BeamState& s, hipStream_t st) {
  if (s.kscale) hipLaunchKernelGGL((beam_reorder_kv_kernel<SESSION, u32x2>), dim3(256, s.B), dim3(256), 0, st, s);
  else hipLaunchKernelGGL((beam_reorder_kv_kernel<SESSION, f32x4>), dim3(256, s.B), dim3(256), 0, st, s);
}

int beam_reorder_forward(const BeamState& s, hipStream_t st) {
  IDX_CHECK(s.seq && s.seen && s.cur_tok && s.kcache && s.vcache && s.beam_idx && s.next_tok, "null pointer");
  if (s.slots) {      // session: the KV rows move first (the rows launch advances the group's scalars); the rows launch writes the next inputs
    IDX_CHECK(s.mel_emb && s.mel_pos && (s.x_frag || (s.x_row && s.x_stats)) && s.d % 16 == 0, "null pointer");
    static const int cat_s = prof_register("beam_select_kernel + beam_reorder_kv_kernel + beam_reorder_rows_kernel (session)");
    ProfScope prof(cat_s, st, 0.0, 0.0);
    if (!s.group_ids) {      // (an admission is step 0: no generated position to move)
      launch_beam_reorder_kv<true>(s, st);
      IDX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(beam_reorder_rows_kernel<true>, dim3(s.group_ids ? s.n_ids : s.B), dim3(1024), 0, st, s);
    IDX_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(beam_reorder_rows_kernel<false>, dim3(s.B), dim3(1024), 0, st, s);
  IDX_LAUNCH_CHECK();
  static const int cat = prof_register("beam_select_kernel + beam_reorder_rows_kernel + beam_reorder_kv_kernel");
  ProfScope prof(cat, st, 0.0, 0.0);
  launch_beam_reorder_kv<false>(s, st);
  IDX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_session_reset_kernel(const BeamState p, int start_token, float* x_last, const float* x, int S,
                                                                 const int* P, const int* cap) {
  const int b = blockIdx.x, g = p.group_ids[b], Pb = P[b], nb = p.nb, V = p.V, d = p.d;
  const float* src = x + ((size_t)b * S + Pb) * d;
  for (int j = 0; j < nb; ++j) {
    const int r = g * nb + j;
    unsigned char* sr = p.seen + (size_t)r * V;
    for (int v = threadIdx.x; v < V; v += 256) sr[v] = (v == 1 || v == start_token) ? 1 : 0;      // input_ids = [1 ... 1, start]
    for (int e = threadIdx.x; e < d; e += 256) x_last[(size_t)r * d + e] = src[e];
    if (threadIdx.x == 0) {
      p.slots[r] = SlotState{Pb, 1, 0, cap[b], 1};
      p.beam_scores[r] = j == 0 ? 0.0f : -1e9f;      // only the first beam's tokens count in the first step (as generate_beam)
    }
  }
  if (threadIdx.x == 0) { p.hyp_n[g] = 0; p.hyp_worst[g] = 1e9; p.done[g] = 0; }
}

int beam_session_reset(const BeamState& s, int start_token, float* x_last, const float* x, int S, const int* P, const int* cap, int n,
                       hipStream_t st) {
  IDX_CHECK(s.slots && s.group_ids && s.seen && s.beam_scores && s.hyp_n && s.hyp_worst && s.done && x_last && x && P && cap, "null pointer");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(beam_session_reset_kernel, dim3(n), dim3(256), 0, st, s, start_token, x_last, x, S, P, cap);
  IDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace idxtts
