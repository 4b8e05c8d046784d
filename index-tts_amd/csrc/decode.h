#pragma once
#include "../../include/idxtts.h"
#include "common.h"

namespace idxtts {

struct DecodeState {   // device-resident per-generation scalars (replay-friendly)
  int pos;       // KV index of the token being processed (= keys already in the cache)
  int mel_pos;   // row of mel_pos_embedding for that token (reference quirk: 0, 2, 3, 4, ... model_v2.py:175-177)
  int step;      // column of `codes` the sampler writes
  unsigned arrive;   // workgroups of the fused sample + embed + advance launch that have finished (0 between launches)
};

// One row of a decode session (continuous batching, gpt.hip "decode session"): every slot carries its own step scalars, so rows
// can be admitted and retired between steps while the captured step graph stays valid.
struct SlotState {
  int pos;        // keys already cached for this slot (= KV index of the token being processed)
  int mel_pos;    // mel_pos_embedding row of that token (0, 2, 3, 4, ... as in DecodeState)
  int step;       // column of `codes` the sampler writes next; once the slot has ended: the number of codes it produced
  int max_step;   // token cap of the request in this slot
  int live;       // 1 while the slot decodes; cleared by the sampler on the stop token or at max_step (0 = free or ended)
};

struct DecodeAttnArgs {
  const float* qkv_part = nullptr; int parts = 0; int part_rows = 0;   // [parts][part_rows][3d] c_attn split-K slab
  const float* qkv_bias = nullptr;                                      // [3d]
  // this layer's cache.  kv_fmt = 0: fp32, K [B][H][16][Smax][4], V [B][H][Smax][64].  kv_fmt = 1: bf16 (rounded to nearest even when a
  // key / value is produced, the new token's own included), K [B][H][8][Smax][8], V [B][H][Smax][64]: 16-byte granules either way.
  // kv_fmt = 2: scaled fp8 (kv_fp8.h), the bf16 geometry with one-byte codes -- K [B][H][8][Smax][8], V [B][H][Smax][64], 8-byte
  // granules -- and one fp32 scale per cached vector, kscale / vscale [B][H][Smax]
  void* kcache = nullptr; void* vcache = nullptr; int kv_fmt = 0;
  float* kscale = nullptr; float* vscale = nullptr;
  float* out = nullptr;                                                 // [B][d] as A-fragment images (frag_index), or
  float* out_row = nullptr;                                             // as fp32 rows [B][d] (the plane GEMV's input, gemv_pl.h)
  const int* kstart = nullptr;                                          // [B] first valid key (left pad), or null
  const DecodeState* st = nullptr;
  int B = 0, H = 0, Smax = 0, d = 0;
  float scale = 0.125f;
  int pos_hint = 0;             // cached positions incl. this step as the HOST knows them (profiler accounting only; 0 under graph replay)
  // Key split for small batches (B * H workgroups cannot pull the KV stream through 256 CUs: a CU sustains ~25 GB/s):
  // nsplit > 1 workgroups per (utterance, head) each take a contiguous range of the keys and leave (max, sum, unnormalised
  // output); the last one to arrive merges them in split order (wait-free, decode_attn_nsplit() depends on B and H only).
  int nsplit = 1;
  float* part = nullptr;        // [B][H][nsplit][66]
  unsigned* cnt = nullptr;      // [B][H] arrival counters: 0 on entry, left at 0
  // Decode session: per-row positions slot[b].pos instead of st->pos; a row whose slot is not live returns at once (zero output,
  // no KV traffic).  The key split keeps its rule: pieces start at the row's first key, nsplit = decode_attn_nsplit(B, H).
  const SlotState* slot = nullptr;
  // Batch-invariant mode (idxtts_gpt_set_batch_invariant): the row's n = pos - kstart + 1 keys are cut into decode_attn_pieces(n)
  // pieces whatever B is, and nsplit only says how many workgroups share a (row, head)'s pieces out (decode_attn_inv_wgs); part is
  // [B][H][DECODE_ATTN_MAX_PIECES][66].  The merged result is a function of the row's own keys alone.
  int invariant = 0;
};
int decode_attn_nsplit(int B, int H);
// The invariant mode's rule: pieces of at most DECODE_ATTN_PIECE_KEYS keys (one key per thread of a 512-thread workgroup: each piece
// is exactly one pass of the score phase), at most DECODE_ATTN_MAX_PIECES of them (longer pieces from 8192 keys on), cut as the key
// split cuts: ceil(n / pieces) keys each, rounded up to 16
#ifndef IDXTTS_DECODE_ATTN_PIECE_KEYS
#define IDXTTS_DECODE_ATTN_PIECE_KEYS 512      // (a build-time constant so that another piece length can be measured: profiles/README.md)
#endif
constexpr int DECODE_ATTN_PIECE_KEYS = IDXTTS_DECODE_ATTN_PIECE_KEYS;
constexpr int DECODE_ATTN_MAX_PIECES = 16;
__host__ __device__ static inline int decode_attn_pieces(int n) {
  const int np = (n + DECODE_ATTN_PIECE_KEYS - 1) / DECODE_ATTN_PIECE_KEYS;
  return np < 1 ? 1 : np > DECODE_ATTN_MAX_PIECES ? DECODE_ATTN_MAX_PIECES : np;
}
int decode_attn_inv_wgs(int B, int H, int Smax);      // workgroups per (row, head): min(decode_attn_nsplit, pieces of a full cache)
int decode_attn_forward(const DecodeAttnArgs& a, hipStream_t stream);

struct SampleArgs {
  const float* part = nullptr; int parts = 0; int part_rows = 0;   // [parts][part_rows][V] lm_head split-K slab
  const float* bias = nullptr;                                     // [V]
  float* logits_out = nullptr;                                     // optional [B][V] raw logits of this step
  unsigned char* seen = nullptr;                                   // [B][V] ids present in input_ids
  int* finished = nullptr;                                         // [B]
  long long* codes = nullptr; int codes_ld = 0;                    // [B][codes_ld]
  // optional [B][logprob_ld]: the log-probability of the token written to codes[b][step] under the row's raw logits (the values
  // logits_out records: before penalty, temperature, top-k and top-p, in every mode); a pad step of a finished row records 0
  // (idxtts.h "Scores").  Null = off: the samplers then run as they always did
  float* logprob_out = nullptr; int logprob_ld = 0;
  int* cur_tok = nullptr;                                          // [B]
  const DecodeState* st = nullptr;
  int B = 0, V = 0, stop_token = 0;
  float penalty = 1.0f;
  // teacher forcing (idxtts_gpt_generate_forced): `codes` still records the row's own argmax, but the token fed back (cur_tok, the
  // repetition-penalty set, the finished flag) is forced[b][step]
  const long long* forced = nullptr; int forced_ld = 0;
  // Batch-invariant mode: the counter-based draws (no exp_noise) are keyed without the batch size -- row b of a one-shot generation
  // draws exp1_draw(seed + b * DRAW_ROW_STRIDE, step * V + v), so row 0 is the B = 1 stream, and a session slot draws that B = 1 stream
  int invariant = 0;
  // Fused tail of a greedy step (embed.x_row or embed.x_frag != null): the workgroup that picked row b's token also writes the NEXT
  // step's input x[b] = mel_emb[token] + mel_pos[st->mel_pos + 1] (model_v2.py:173-177) -- as the fp32 residual row
  // and the per-16-column row statistics of the first folded LayerNorm -- and the last workgroup to arrive advances the
  // step scalars (DecodeState::arrive counts them): sample + embed + advance in ONE launch.
  struct Embed {
    float* x_row = nullptr; float* x_stats = nullptr;      // plane-GEMV step: fp32 row + per-16-column statistics, or
    float* x_frag = nullptr;                               // fp32-MFMA GEMV step: the A-fragment image (frag_index)
    const float* mel_emb = nullptr; const float* mel_pos = nullptr; int d = 0;
    DecodeState* st_rw = nullptr;
  } embed;
};
int sample_greedy_forward(const SampleArgs& a, hipStream_t stream);
// Greedy sampler of a decode session (always the fused tail: a.embed.x_row or a.embed.x_frag set; a.st / a.embed.st_rw unused,
// a.finished unused): one workgroup per slot -- slot_ids[i] for i < n, or every slot 0..a.B-1 when slot_ids is null.  A slot that is
// not live returns at once.  Otherwise it samples row `slot` of the logits, writes codes[slot][step], updates seen, and either ends the
// slot (stop token or step + 1 == max_step: live = 0, step = codes produced) or writes the slot's next input row with mel_pos + 1 and
// advances its own pos / mel_pos / step.
int sample_slots_forward(const SampleArgs& a, SlotState* slots, const int* slot_ids, int n, hipStream_t stream);

// Scoring given codes (idxtts.h): one 1024-thread workgroup per row of a logits slab [rows <= 64][V] (the head's output on `rows` packed
// positions) writes out[dst[r]] = the "Scores" log-probability of code tok[r] under row r, or 0 without reading the row where tok[r] < 0.
// tok / dst: device [rows]; dst[r] indexes `out`, which the caller has sized and whose other elements stay as they are.
struct ScoreRowsArgs {
  const float* logits = nullptr; int rows = 0, V = 0;
  const int* tok = nullptr; const int* dst = nullptr;
  float* out = nullptr;
};
int score_rows_forward(const ScoreRowsArgs& a, hipStream_t stream);

// Multinomial sampling of the next token (HF _sample, transformers_generation_utils.py:3222-3250, with the warpers of
// 1036-1044): repetition penalty -> / temperature -> top-k (ties at the threshold kept) -> top-p (ascending sort, softmax,
// cumulative <= 1 - top_p removed, largest always kept) -> softmax -> torch.multinomial(probs, 1), which IS
// argmax(probs / q) with q ~ Exp(1): the draw is an explicit input, exp_noise[step][b][V].
// mode SAMPLE_ACCEL restates the accel engine's Sampler instead (accel_engine.py:648-659): softmax(logits / T) divided by
// clamp_min(q, 1e-10), argmax; no penalty, no top-k / top-p.
enum SampleMode { SAMPLE_HF = 1, SAMPLE_ACCEL = 2 };
// The Exp(1) draw of element `idx` of a generation: the caller's tensor when it supplied one (reproduces torch's stream), else a
// counter-based generator -- splitmix64 of (seed, idx + 1) -> its top 24 bits h -> u = (h + 0.5) / 2^24 in fp32, at most 1 - 2^-24 ->
// -log(u) -- so that default calls need no [steps][B][V] noise tensor (0.8 GB for 16 utterances x 1500 steps; 2.4 GB with 3 beams).
// From h = 2^23 on, h + 0.5 is no fp32 number and rounds to the even neighbour, which for h = 2^24 - 1 is 2^24: u = 1, a draw of
// 0 and that id taken whatever its probability, hence the upper bound (tests/sampler_cases.py restates all of this).
__host__ __device__ static inline float exp1_draw(const float* noise, unsigned long long seed, size_t idx) {
  if (noise) return noise[idx];
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  // the open interval: u = 1 would make the draw 0 and probs / q infinite (or 0 / 0 for a filtered token) -- torch's exponential_
  // never returns 0 either
  const float u = fminf(((float)(z >> 40) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
  return -logf(u);
}
constexpr unsigned long long DRAW_ROW_STRIDE = 0xD6E8FEB86659FD93ull;      // odd: rows of one seed are distinct seeds
struct SampleWarpArgs {
  SampleArgs base;                   // logits source, bookkeeping buffers, penalty (parts must be 1)
  int mode = SAMPLE_HF;
  float temperature = 1.0f;
  int top_k = 0;                     // 0 = off
  float top_p = 1.0f;                // >= 1 = off
  const float* exp_noise = nullptr;  // [steps][B][V], or null: draws come from exp1_draw(seed, ...)
  unsigned long long seed = 0;
};
int sample_warp_forward(const SampleWarpArgs& a, hipStream_t stream);
// Per-request sampler of a sampled decode session: one row per slot, in the session workspace (idxtts_sampling's values)
struct SlotSampling {
  int mode;                      // 0 greedy (sample_slots_forward's rule), SAMPLE_HF, SAMPLE_ACCEL
  float temperature;
  int top_k;
  float top_p;
  unsigned long long seed;       // draws when exp_noise is null: exp1_draw(seed, (t * B + 0) * V + v) at the slot's step t
  const float* exp_noise;        // the request's draws [max_step][V] (row t at step t), or null
};
// sample_slots_forward with each slot's own sampler samp[slot] (a.parts must be 1): mode 0 rows are bit-identical to
// sample_slots_forward, HF / accel rows to row 0 of sample_warp_forward on an a.B-row generation with the same draws
int sample_slots_warp_forward(const SampleArgs& a, SlotState* slots, const SlotSampling* samp, const int* slot_ids, int n,
                              hipStream_t stream);

// x[b] = mel_emb[tok] + mel_pos[mp] for the plane-GEMV decode step: fp32 row + (mean, M2) per 16 columns (every thread of the
// workgroup takes part; the session tails of sample_slots_forward and the beam session share it)
template <int NT>
__device__ __forceinline__ void embed_row_pl(float* x_row, float* x_stats, const int b, const int B, const int d, const float* mel_emb,
                                             const float* mel_pos, const int tok, const int mp, const int tid) {
  const int R = ((B + 15) >> 4) * 16;
  for (int e0 = 0; e0 < d; e0 += NT) {      // d % 16 == 0: a 16-column tile never straddles the loop's edge or a wave
    const int e = e0 + tid;
    const bool on = e < d;
    const float v = on ? mel_emb[(size_t)tok * d + e] + mel_pos[(size_t)mp * d + e] : 0.f;
    float s = v;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) s += __shfl_xor(s, m);
    const float mean = s * 0.0625f;
    float q = (v - mean) * (v - mean);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) q += __shfl_xor(q, m);
    if (on) {
      x_row[(size_t)b * d + e] = v;
      if ((e & 15) == 0) *reinterpret_cast<float2*>(&x_stats[((size_t)(e >> 4) * R + b) * 2]) = make_float2(mean, q);
    }
  }
}

int advance_state(DecodeState* st, hipStream_t stream);
// The cache one layer's producers write: kcache / vcache in format fmt (DecodeAttnArgs::kv_fmt); kscale / vscale: the fp8 format's
// scales [rows][H][Smax], else null
struct KvDst {
  void* kcache = nullptr; void* vcache = nullptr; int fmt = 0;
  float* kscale = nullptr; float* vscale = nullptr;
};
// qkv [B][S][3d] -> caches, positions [0, S).  bf16 / fp8: the k / v columns of qkv are rounded IN PLACE to what the cache holds, so
// the prefill attention that follows sees exactly the keys and values later steps read from the cache
int kv_store_prefill(float* qkv, const KvDst& kv, int B, int H, int S, int Smax, int d, hipStream_t stream);
// Decode-session admission: the same for a right-padded prefill of n rows whose cache rows are the slots slot_ids[b]: positions
// [0, len[b]) of row b go to slot slot_ids[b] (the caches laid out for `slots` rows); k / v columns rounded in place as above.
// fan > 1 (beam sessions): row b goes to the fan slots slot_ids[b] .. slot_ids[b] + fan - 1.  first (device [n + 1], fan = 1; admission
// with takes): row b goes to the slots slot_ids[first[b]] .. slot_ids[first[b + 1] - 1] instead, any slots in any order
int kv_store_slots(float* qkv, const KvDst& kv, int n, int H, int S, int Smax, int d, const int* slot_ids, const int* len,
                   hipStream_t stream, int fan = 1, const int* first = nullptr);
// Instrument (idxtts_kv_fp8_quantize): the fp8 cache's quantiser on n vectors x [n][64] -> codes [n][64], scales [n]
int kv_fp8_quantize(const float* x, int n, unsigned char* codes, float* scales, hipStream_t stream);
// the device's f32 -> fp8 conversion equals wstream.h::fp8_e4m3_encode on every code value and every midpoint between neighbours
int fp8_check_device_encode(hipStream_t stream);
// Decode-session admission, input rows of the prefill: x[b][s] = emb[b][s] for s < P[b] (emb [n][ld_rows][d]), mel_emb[start] +
// mel_pos[0] at s = P[b], 0 after it (right padding); every row S long
int session_prefill_input(float* x, const float* emb, int ld_rows, const int* P, int n, int S, int d, const float* mel_emb,
                          const float* mel_pos, int start_token, hipStream_t stream);
// Decode-session admission, per admitted row b: reset slot slot_ids[b] -- seen row = {1, start_token}, state {pos = P[b], mel_pos = 1,
// step = 0, max_step = cap[b], live = 1} -- and copy the prefill's last valid row x[b][P[b]] (x [n][S][d]) to x_last[slot].  row
// (admission with takes): entry t of slot_ids / cap is a take of prefill row row[t], whose P and x row it gets
int session_reset_slots(SlotState* slots, unsigned char* seen, int V, int start_token, float* x_last, const float* x, int S, int d,
                        const int* slot_ids, const int* P, const int* cap, int n, hipStream_t stream, const int* row = nullptr);
// Continuing from given codes (idxtts.h): the prefill input rows of a prefix.  Row b of x [rows][S][d] gets, at positions
// P_b + 1 + j for j < k_b, mel_emb[prefix_b[j]] + mel_pos[pos0 + j]; pos0 = 1 (the reference's layout) or 2 (the positions an
// uninterrupted run fed).  P / klen null: P_all / k_all for every row.  prefix_b starts at prefix + off[b], or (off null) at
// prefix + (b / row_div) * k_all: a dense [prompts][k_all] array, row_div prefill rows per prompt.  The caller has checked that
// P_b + 1 + k_b <= S, pos0 + k_b <= the position table's rows and every code is a row of mel_emb.  kmax: the longest k_b.
struct PrefixRows {
  float* x = nullptr; int S = 0, d = 0;
  const int* P = nullptr; int P_all = 0;
  const int* klen = nullptr; int k_all = 0;
  const long long* prefix = nullptr; const int* off = nullptr; int row_div = 1;
  int pos0 = 2;
  const float* mel_emb = nullptr; const float* mel_pos = nullptr; int V = 0;
};
int prefix_input_rows(const PrefixRows& a, int rows, int kmax, hipStream_t stream);
// session_reset_slots for an admission with prefixes (klen [rows], off [rows] into the packed prefix / prefix_lp): slot slot_ids[t]
// starts behind the k = klen[b] codes of its prefill row b -- seen = {1, start_token} and the codes, codes[slot][0, k) = the codes,
// logprobs[slot][0, k) = prefix_lp's values or 0 (logprobs null: the session records none), x_last[slot] = x[b][P[b] + k], state
// {P[b] + k, k + 1, k, cap[t], 1}.  k = 0 is exactly session_reset_slots.
struct PrefixReset {
  SlotState* slots = nullptr; unsigned char* seen = nullptr; int V = 0, start_token = 0;
  float* x_last = nullptr; const float* x = nullptr; int S = 0, d = 0;
  const int* slot_ids = nullptr; const int* P = nullptr; const int* cap = nullptr; const int* row = nullptr;
  const int* klen = nullptr; const int* off = nullptr; const long long* prefix = nullptr; const float* prefix_lp = nullptr;
  long long* codes = nullptr; int codes_ld = 0; float* logprobs = nullptr;
};
int session_reset_slots_prefix(const PrefixReset& a, int n, hipStream_t stream);
// Ends slots of a decode session between steps (eviction, stop): slot i of the n_slots <= 64 slots for every set bit i of `mask`, passed
// by value -- live = 0, step kept (the codes produced so far).  cap_at_step: a slot that was live also gets max_step = step (a cap set
// late: what reads the slot afterwards sees a request that ended at that cap); a slot that had ended is left as it was.
int session_end_slots(SlotState* slots, int n_slots, unsigned long long mask, bool cap_at_step, hipStream_t stream);
// Preempt and resume (idxtts.h "Preempt and resume"): the byte layout of a parked row, from the header's fields alone
struct ParkLayout {
  int chunks = 0, gran = 0, elem = 0;      // key chunks per head, bytes of one chunk per position, bytes per element
  size_t krun = 0, vrun = 0, srun = 0;     // padded bytes of one key run, the value run, one scale run (fp8 only, else 0)
  size_t off_seen = 0, off_codes = 0, off_lp = 0, off_kv = 0, per_head = 0, bytes = 0;      // off_lp: scored rows only, else = off_kv
};
__host__ __device__ static inline size_t park_pad16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ static inline ParkLayout park_layout(int kv_fmt, int layers, int heads, int V, int pos, int step,
                                                                int scores = 0) {      // scores: idxtts_park_header::reserved[1]
  ParkLayout l;
  l.chunks = kv_fmt == 0 ? 16 : 8; l.gran = kv_fmt == 2 ? 8 : 16; l.elem = kv_fmt == 2 ? 1 : kv_fmt ? 2 : 4;
  l.krun = park_pad16((size_t)pos * l.gran); l.vrun = (size_t)pos * 64 * l.elem; l.srun = kv_fmt == 2 ? park_pad16((size_t)pos * 4) : 0;
  l.off_seen = sizeof(idxtts_park_header);
  l.off_codes = l.off_seen + park_pad16((size_t)V);
  l.off_lp = l.off_codes + park_pad16((size_t)step * 8);
  l.off_kv = l.off_lp + (scores ? park_pad16((size_t)step * 4) : 0);
  l.per_head = l.chunks * l.krun + l.vrun + 2 * l.srun;
  l.bytes = l.off_kv + (size_t)layers * heads * l.per_head;
  return l;
}
static_assert(sizeof(idxtts_park_header) == 128, "parked-row header");
struct ParkArgs {
  idxtts_park_header hdr;        // by value: _park writes it in front of the row, _resume restores the slot from it (checked on the host)
  char* blob = nullptr;          // the parked row (16-byte aligned): written by park, read by resume
  char* kcache = nullptr; char* vcache = nullptr; float* kscale = nullptr; float* vscale = nullptr;   // layer 0 of the session's cache
  size_t layer_bytes = 0, layer_scales = 0;      // one layer of kcache / vcache in bytes, of kscale / vscale in floats
  int slot = 0, Smax = 0;
  SlotState* slots = nullptr; SlotSampling* samp = nullptr;      // samp: sampled sessions only (resume rewrites the slot's row)
  unsigned char* seen = nullptr; long long* codes = nullptr; int codes_ld = 0; int* cur_tok = nullptr;
  float* logprobs = nullptr;               // scored sessions (hdr.reserved[1] = 1): [B][codes_ld], the row's segment behind the codes
  SampleArgs::Embed embed; int B = 0;      // resume: where the slot's next input goes (the session tails' block), B = the session's slots
};
// One launch each, between steps on the session's stream.  park: slot -> blob, then live = 0.  resume: blob -> slot, live = 1 with the
// header's scalars, and the slot's next input mel_emb[last code] + mel_pos[mel_pos] written as the sampler tails write it.
int session_park_slot(const ParkArgs& a, hipStream_t stream);
int session_resume_slot(const ParkArgs& a, hipStream_t stream);
// Fork (idxtts.h "Several takes of one request"): the row in slot `src`, cut back to `at` codes, copied to the n free slots dst[] in one
// launch that reads every 16-byte vector of the source once and stores it n times -- positions [0, P + max(at, 1)) of the keys, values and
// fp8 scales of every layer (what a row holding `at` codes has cached), codes[0, at) (scored sessions: and their log-probabilities), a seen row rebuilt from the start token and those
// codes, SlotState {P + at, at + 1, at, cap[j], 1} and the next input mel_emb[codes[at - 1]] + mel_pos[at + 1] as the sampler tails write
// it.  at = 0: the state session_reset_slots leaves (SlotState {P, 1, 0, cap[j], 1}, x_last[src] copied), and the caller runs the
// admission's head-and-sample pass on the destinations.  The source is only read.
constexpr int FORK_MAX = 64;
struct ForkArgs {
  int kv_fmt = 0, layers = 0, heads = 0, V = 0, start_token = 0;
  int src = 0, P = 0, at = 0, n = 0;
  unsigned char dst[FORK_MAX] = {}; int cap[FORK_MAX] = {};      // by value: no staging copy, no synchronisation
  char* kcache = nullptr; char* vcache = nullptr; float* kscale = nullptr; float* vscale = nullptr;   // layer 0 of the session's cache
  size_t layer_bytes = 0, layer_scales = 0;
  int Smax = 0;
  SlotState* slots = nullptr; unsigned char* seen = nullptr; long long* codes = nullptr; int codes_ld = 0; int* cur_tok = nullptr;
  float* x_last = nullptr;
  float* logprobs = nullptr;      // scored sessions: [B][codes_ld], else null
  SampleArgs::Embed embed; int B = 0;
};
int session_fork_slots(const ForkArgs& a, hipStream_t stream);
constexpr int GATHER_MAX_TABLES = 5;
struct GatherArgs {
  float* out = nullptr; int ld_out = 0; int d = 0;
  const float* table[GATHER_MAX_TABLES] = {};   // [n_t][d]
  const int* idx[GATHER_MAX_TABLES] = {};       // [rows], -1 = skip
  int table_rows[GATHER_MAX_TABLES] = {};       // rows of each table (0 = not checked): an id >= table_rows is NOT read ...
  int* oob = nullptr;                           // ... and, when given, *oob is set to 1 + table index (device int, caller zeroes it)
};
int gather_sum_rows(const GatherArgs& a, int rows, hipStream_t stream);
int embed_step(float* x, int B, int d, const float* mel_emb, const float* mel_pos, const int* cur_tok, const DecodeState* st,
               hipStream_t stream);
// the same for the plane-GEMV path: x as fp32 rows [B][d] + the row statistics per 16 columns
int embed_step_pl(float* x_row, float* x_stats, int B, int d, const float* mel_emb, const float* mel_pos, const int* cur_tok,
                  const DecodeState* st, hipStream_t stream);

}  // namespace idxtts
