// Device side of beam search / beam-sample for the GPT decode loop (HF `_beam_search` + BeamSearchScorer, restated in
// oracle/gpt.py::generate_beam).  Everything of a step that depends on data -- candidate selection, hypothesis bookkeeping,
// beam re-indexing of the token history, the repetition-penalty masks and the KV cache -- stays on the device, so a step has
// no host round trip and can be replayed from a hipGraph like the greedy step.
#pragma once
#include "decode.h"

namespace idxtts {

constexpr int BEAM_MAX = 8;     // num_beams <= 8 (the reference default is 3)

// Per-request parameters of a beam decode session (one row per group, in the session workspace; idxtts_beam's values)
struct SlotBeam {
  int do_sample;
  float temperature;
  int top_k;
  float top_p;
  double length_penalty;
  int early_stopping;
  unsigned long long seed;       // draws when exp_noise is null: exp1_draw(seed, (t * groups + 0) * nb * V + i) at the group's step t
  const float* exp_noise;        // the request's draws [max_step][nb * V] (row t at step t), or null
};

struct BeamState {
  // per decode row r = b * nb + j
  const float* logits = nullptr;      // [R][V] raw lm_head output of this step
  float* proc = nullptr;              // [R][V] processed scores + running beam score (scratch)
  unsigned char* seen = nullptr;      // [R][V] ids present in the row's input_ids (repetition penalty)
  float* beam_scores = nullptr;       // [R]
  int* next_tok = nullptr;            // [R] chosen by select, consumed by reorder
  int* beam_idx = nullptr;            // [R] source row of each new beam (global row index)
  int* seq = nullptr; int seq_ld = 0; // [R][seq_ld] generated tokens of each live beam
  int* cur_tok = nullptr;             // [R] token fed to the next decode step
  // finished hypotheses per utterance: up to nb + 1 while one is being inserted (BeamHypotheses.add)
  double* hyp_score = nullptr;        // [B][BEAM_MAX + 1] in list (insertion) order
  int* hyp_len = nullptr;             // [B][BEAM_MAX + 1]
  int* hyp_slot = nullptr;            // [B][BEAM_MAX + 1] physical row of hyp_seq holding that hypothesis
  int* hyp_seq = nullptr;             // [B][BEAM_MAX + 1][seq_ld]
  int* hyp_n = nullptr;               // [B]
  double* hyp_worst = nullptr;        // [B]
  int* done = nullptr;                // [B]
  const DecodeState* st = nullptr;
  const float* exp_noise = nullptr;   // [steps][B][nb * V] Exp(1) draws (do_sample), or null: exp1_draw(seed, ...)
  unsigned long long seed = 0;
  int invariant = 0;                  // batch-invariant mode: seeded draws without a term in B (utterance b: seed + b * DRAW_ROW_STRIDE,
                                      // index n * nb * V + i; a session group draws utterance 0's stream)
  void* kcache = nullptr; void* vcache = nullptr;     // [L][R][H][G][Smax] / [L][R][H][Smax][G] granules of 16 bytes (fp8 cache: 8)
  int kv_gran = 16;                                   // G: granules per key (16 = fp32 cache, 8 = bf16 or fp8 cache; decode.h)
  float* kscale = nullptr; float* vscale = nullptr;   // fp8 cache: [L][R][H][Smax] scales, which follow their rows; else null
  int B = 0, nb = 0, V = 0, stop_token = 0, L = 0, H = 0, Smax = 0, prompt_len = 0;   // prompt_len: KV positions shared by all beams (P + 1)
  int do_sample = 0, top_k = 0, early_stopping = 0;
  float penalty = 1.0f, temperature = 1.0f, top_p = 1.0f;
  double length_penalty = 0.0;
  // Beam decode session (slots != null; gpt.hip "decode session"): B groups of nb consecutive slots, each group one request.  Every
  // per-group value comes from the workspace -- step / pos / mel_pos from the group's SlotState (its first slot; all nb are equal), the
  // request's parameters from group[g] (the scalar parameters above are unused), the KV range that moves from pos - step + 1 = P_g + 1
  // -- so a captured step stays valid across admissions.  Groups that are not live do nothing.  The last stage ends a group (done or
  // cap: live = 0 on its slots, step = steps taken) or writes its rows' next inputs x = mel_emb[tok] + mel_pos[mel_pos + 1] (x_row +
  // x_stats on the plane GEMV path, else x_frag) and advances its slots: no embed_step / advance_state.
  SlotState* slots = nullptr;
  const SlotBeam* group = nullptr;
  const int* group_ids = nullptr; int n_ids = 0;      // admission: these groups only (every group when null)
  float* x_row = nullptr; float* x_stats = nullptr; float* x_frag = nullptr;
  const float* mel_emb = nullptr; const float* mel_pos = nullptr; int d = 0;
};

// log_softmax -> repetition penalty -> (sampling: temperature, top-k, top-p with min_tokens_to_keep = 2) -> + beam score
int beam_scores_forward(const BeamState& s, hipStream_t st);
// 2 * nb candidates per utterance (multinomial without replacement == top-(2 nb) of probs / q, or plain top-k), sorted by score;
// BeamSearchScorer.process: finished hypotheses, next beams, done flags
int beam_select_forward(const BeamState& s, hipStream_t st);
// re-index token history, seen masks, KV cache rows (generated positions only) by beam_idx; append the chosen tokens
// (session mode: the KV launch first, then the rows launch with the fused tail; no KV launch for an admission, whose step is 0)
int beam_reorder_forward(const BeamState& s, hipStream_t st);
// Beam session admission, per admitted group b (group_ids[b]; s.slots / s.group / s.nb set): reset its nb slots -- seen = {1,
// start_token}, SlotState {P[b], 1, 0, cap[b], 1}, x_last[slot] = x[b][P[b]] (x [n][S][d]) -- and its scorer: beam scores 0, -1e9, ...,
// hyp_n 0, hyp_worst 1e9, done 0
int beam_session_reset(const BeamState& s, int start_token, float* x_last, const float* x, int S, const int* P, const int* cap, int n,
                       hipStream_t st);

// Preempt and resume of a beam group (idxtts.h "Preempt and resume, beam sessions"): the byte layout of a parked group, from the
// header's fields alone.  The KV part of a (layer, head) is a parked row's for the Ps = pos - step + 1 shared positions (ParkLayout of
// Ps: sh), then one for the T = step - 1 generated positions of every beam (ParkLayout of T: pb).
struct ParkGroupLayout {
  ParkLayout sh, pb;
  int Ps = 0, T = 0;
  size_t seen_row = 0, tok_row = 0;      // padded bytes of one seen row, of one token row (seq and hypotheses alike)
  size_t off_seen = 0, off_seq = 0, off_scores = 0, off_worst = 0, off_hscore = 0, off_hlen = 0, off_hseq = 0, off_kv = 0;
  size_t per_head = 0, bytes = 0;
};
__host__ __device__ static inline ParkGroupLayout park_group_layout(int kv_fmt, int layers, int heads, int V, int nb, int pos, int step) {
  ParkGroupLayout l;
  l.Ps = pos - step + 1; l.T = step - 1;
  l.sh = park_layout(kv_fmt, 1, 1, V, l.Ps, step);
  l.pb = park_layout(kv_fmt, 1, 1, V, l.T, step);
  l.seen_row = park_pad16((size_t)V); l.tok_row = park_pad16((size_t)step * 4);
  l.off_seen = sizeof(idxtts_park_group_header);
  l.off_seq = l.off_seen + nb * l.seen_row;
  l.off_scores = l.off_seq + nb * l.tok_row;
  l.off_worst = l.off_scores + park_pad16((size_t)nb * 4);
  l.off_hscore = l.off_worst + 16;
  l.off_hlen = l.off_hscore + park_pad16((size_t)nb * 8);
  l.off_hseq = l.off_hlen + park_pad16((size_t)nb * 4);
  l.off_kv = l.off_hseq + nb * l.tok_row;
  l.per_head = l.sh.per_head + nb * l.pb.per_head;
  l.bytes = l.off_kv + (size_t)layers * heads * l.per_head;
  return l;
}
static_assert(sizeof(idxtts_park_group_header) == 128, "parked-group header");
struct ParkGroupArgs {
  idxtts_park_group_header hdr;  // by value: park writes it in front of the group, resume restores the group from it (checked on the host)
  char* blob = nullptr;          // the parked group (16-byte aligned): written by park, read by resume
  char* kcache = nullptr; char* vcache = nullptr; float* kscale = nullptr; float* vscale = nullptr;   // layer 0 of the session's cache
  size_t layer_bytes = 0, layer_scales = 0;      // one layer of kcache / vcache in bytes, of kscale / vscale in floats
  int group = 0, Smax = 0, B = 0;                // B: the session's slots
  BeamState bs;                  // the session's beam buffers (slots, seen, seq, cur_tok, beam scores, hypotheses)
  SlotBeam* group_tab = nullptr; // the session's SlotBeam table (resume rewrites the group's entry)
  SampleArgs::Embed embed;       // resume: where the rows' next inputs go (the session tails' block)
};
// One launch each, between steps on the session's stream.  park: group -> blob, then live = 0 on its slots.  resume: blob -> group,
// live = 1 with the header's scalars, the device SlotBeam entry, and every row's next input as the tails write it.
int session_park_group(const ParkGroupArgs& a, hipStream_t stream);
int session_resume_group(const ParkGroupArgs& a, hipStream_t stream);

}  // namespace idxtts
