// Beam search / beam-sample generation on the GPT decode step (host side; kernels in beam.hip).
//
// Reference: UnifiedVoice.inference_speech with num_beams > 1 (indextts/gpt/model_v2.py:835-892) = HF generate ->
// _beam_search (indextts/gpt/transformers_generation_utils.py:2226-2255, 3325-3516) with BeamSearchScorer
// (indextts/gpt/transformers_beam_search.py:123-420): the decoding mode IndexTTS2.infer runs by default
// (infer_v2.py:714-722, 767).  Rows r = b * num_beams + j (_expand_inputs_for_generation = repeat_interleave).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gpt.h"
#include "model_util.h"

namespace idxtts {

BeamBuffers carve_beam(void* ws, int B, int nb, int V, int max_new) {
  const int R = B * nb;
  BeamBuffers b;
  Carver c(ws);
  b.proc = c.take<float>((size_t)R * V);
  b.beam_scores = c.take<float>(R);
  b.next_tok = c.take<int>(R);
  b.beam_idx = c.take<int>(R);
  b.seq = c.take<int>((size_t)R * max_new);
  b.hyp_score = c.take<double>((size_t)B * (BEAM_MAX + 1));
  b.hyp_worst = c.take<double>(B);
  b.hyp_len = c.take<int>((size_t)B * (BEAM_MAX + 1));
  b.hyp_slot = c.take<int>((size_t)B * (BEAM_MAX + 1));
  b.hyp_seq = c.take<int>((size_t)B * (BEAM_MAX + 1) * max_new);
  b.hyp_n = c.take<int>(B);
  b.done = c.take<int>(B);
  b.bytes = (c.off + 255) & ~(size_t)255;
  return b;
}

int beam_finalize(int nb, double lp, int hyp_n, const double* hyp_score, const int* hyp_len, const int* hyp_slot, const int* hyp_seq,
                  int seq_ld, bool done, const float* bscore, const int* seq, int steps_done, BeamHyp* best, int n_best) {
  std::vector<BeamHyp> list;
  for (int q = 0; q < hyp_n; ++q) list.push_back(BeamHyp{hyp_score[q], &hyp_seq[(size_t)hyp_slot[q] * seq_ld], hyp_len[q]});
  if (!done) {      // open beams become hypotheses (BeamHypotheses.add with its keep-the-best rule)
    double worst = 1e9;
    for (const BeamHyp& h : list) worst = std::min(worst, h.score);
    for (int j = 0; j < nb; ++j) {
      const double score = (double)bscore[j] / std::pow((double)steps_done, lp);
      if ((int)list.size() < nb || score > worst) {
        list.push_back(BeamHyp{score, &seq[(size_t)j * seq_ld], steps_done});
        if ((int)list.size() > nb) {
          size_t wi = 0;
          for (size_t q = 1; q < list.size(); ++q) if (list[q].score < list[wi].score) wi = q;
          list.erase(list.begin() + wi);
          worst = list[0].score;
          for (const BeamHyp& h : list) worst = std::min(worst, h.score);
        } else {
          worst = std::min(worst, score);
        }
      }
    }
  }
  IDX_CHECK(!list.empty(), "no hypothesis");
  // sorted(..., key=score), popped from the end n_best times: best first, among equal scores the one added LATER first
  IDX_CHECK(n_best >= 1 && (size_t)n_best <= list.size(), "fewer hypotheses than n_best");
  std::stable_sort(list.begin(), list.end(), [](const BeamHyp& a, const BeamHyp& b) { return a.score < b.score; });
  for (int q = 0; q < n_best; ++q) best[q] = list[list.size() - 1 - q];
  return 0;
}

void beam_fill_rows(const BeamHyp* hyps, int n, int ld, int cap, int stop_token, long long* out, int* lens, float* scores) {
  for (int q = 0; q < n; ++q) {
    for (int t = 0; t < ld; ++t) out[(size_t)q * ld + t] = t < hyps[q].len ? hyps[q].toks[t] : stop_token;
    if (lens) lens[q] = std::min(hyps[q].len + 1, cap);
    if (scores) scores[q] = (float)hyps[q].score;
  }
}

size_t GPTModel::beam_workspace_bytes(int B, int nb, int S, int max_new) const {
  return workspace_bytes(B * nb, S, max_new) + carve_beam(nullptr, B, nb, cfg.number_mel_codes, max_new).bytes;
}

// the beam stages' buffers of B utterances (session: groups) x nb rows; the caller adds the per-request or per-session fields
BeamState GPTModel::beam_state(const Buffers& w, const BeamBuffers& bb, int B, int nb, int seq_ld) const {
  BeamState b;
  b.logits = w.logits; b.proc = bb.proc; b.seen = w.seen; b.beam_scores = bb.beam_scores; b.next_tok = bb.next_tok;
  b.beam_idx = bb.beam_idx; b.seq = bb.seq; b.seq_ld = seq_ld; b.cur_tok = w.cur_tok;
  b.hyp_score = bb.hyp_score; b.hyp_len = bb.hyp_len; b.hyp_slot = bb.hyp_slot; b.hyp_seq = bb.hyp_seq; b.hyp_n = bb.hyp_n;
  b.hyp_worst = bb.hyp_worst; b.done = bb.done;
  b.kcache = w.kcache; b.vcache = w.vcache; b.kv_gran = kv_fmt ? 8 : 16; b.kscale = w.kscale; b.vscale = w.vscale;
  b.invariant = w.invariant;
  b.B = B; b.nb = nb; b.V = cfg.number_mel_codes; b.stop_token = cfg.stop_mel_token; b.L = cfg.layers; b.H = cfg.heads; b.Smax = w.Smax;
  return b;
}

// generate_beam()'s rules for one request's parameters (num_beams is checked by the caller)
static int check_beam(const idxtts_beam& r) {
  IDX_CHECK(!r.do_sample || (r.temperature > 0.0f && r.top_k >= 0 && r.top_k <= 1024 && r.top_p > 0.0f),
            "beam-sample needs a positive temperature, top_k <= 1024 and top_p > 0");
  // the nucleus is cut inside the top-k survivors: beam_scores_kernel sorts at most 2048 of them, and with 0 < top_k <= 1024 more
  // survive only as one group of equal scores at the top-k threshold, which it walks by count.  Without a top-k the whole vocabulary
  // would survive unsorted, so that combination is refused; top_p >= 1 needs no sorting and takes any top_k <= 1024, 0 included.
  IDX_CHECK(!r.do_sample || r.top_p >= 1.0f || (r.top_k > 0 && r.top_k <= 1024), "top-p needs 0 < top_k <= 1024");
  IDX_CHECK(r.early_stopping == 0 || r.early_stopping == 1, "early_stopping must be 0 (False) or 1 (True)");
  return 0;
}

int GPTModel::generate_beam(const float* inputs_embeds, const int* pad_left_host, int B, int P, int max_new, float penalty,
                            const idxtts_beam* beam, long long* codes, int* n_steps_out, void* ws, size_t ws_bytes, int use_graph,
                            hipStream_t user_stream, int n_best, int* lens, float* scores) {
  IDX_CHECK(inputs_embeds && codes && n_steps_out && beam, "null pointer");
  IDX_CHECK(n_best >= 1 && n_best <= beam->num_beams, "1 <= n_best <= num_beams");
  GenScope gen_scope(this);
  const int nb = beam->num_beams, R = B * nb;
  IDX_CHECK(nb >= 2 && nb <= BEAM_MAX, "2 <= num_beams <= 8");
  IDX_CHECK(B > 0 && R <= 64 && P > 0 && max_new > 0, "shape (B * num_beams <= 64)");
  if (check_beam(*beam)) return 1;
  const int V = cfg.number_mel_codes, S = P + 1;
  IDX_CHECK(max_new + 1 < cfg.mel_pos_len, "max_new_tokens exceeds the mel position table");
  IDX_CHECK(ws && ws_bytes >= beam_workspace_bytes(B, nb, S, max_new), "workspace too small");
  hipStream_t st = nullptr;
  if (call_stream(user_stream, &st)) return 1;
  Buffers w = carve(ws, R, S, max_new);
  const BeamBuffers bb = carve_beam(static_cast<char*>(ws) + w.bytes, B, nb, V, max_new);
  w.beam_tail = true;
  BeamState& bst = w.beam;
  bst = beam_state(w, bb, B, nb, max_new);
  bst.st = w.state; bst.exp_noise = beam->exp_noise; bst.seed = beam->seed; bst.prompt_len = S;
  bst.do_sample = beam->do_sample ? 1 : 0; bst.top_k = beam->top_k; bst.early_stopping = beam->early_stopping;
  bst.penalty = penalty; bst.temperature = beam->temperature; bst.top_p = beam->top_p; bst.length_penalty = (double)beam->length_penalty;

  // first beam 0, the others -1e9: only the first beam's tokens count in the first step (transformers_generation_utils.py:3420-3422)
  std::vector<float> bs0(R, -1e9f);
  for (int b = 0; b < B; ++b) bs0[b * nb] = 0.0f;
  IDX_HIP(hipMemcpyAsync(bb.beam_scores, bs0.data(), R * sizeof(float), hipMemcpyHostToDevice, st));
  std::vector<double> worst0(B, 1e9);
  IDX_HIP(hipMemcpyAsync(bb.hyp_worst, worst0.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemsetAsync(bb.hyp_n, 0, B * sizeof(int), st));
  IDX_HIP(hipMemsetAsync(bb.done, 0, B * sizeof(int), st));
  // the beams of an utterance start identical: its prompt on all nb rows; beam_scorer.is_done (every utterance finished) polled
  int steps_done = 0;
  if (run_generation(w, inputs_embeds, pad_left_host, B, nb, P, max_new, penalty, nullptr, use_graph && !prof_enabled(), nullptr, nullptr,
                     bb.done, B, 8, &steps_done, st, GenerateCall{})) return 1;      // (nb prefill rows per utterance, no prefix)

  // ---- BeamSearchScorer.finalize on the host (transformers_beam_search.py:320-414) ----
  std::vector<int> seq((size_t)R * max_new), hyp_len((size_t)B * (BEAM_MAX + 1)), hyp_slot(hyp_len.size()), hyp_n(B), done(B);
  std::vector<int> hyp_seq((size_t)B * (BEAM_MAX + 1) * max_new);
  std::vector<double> hyp_score(hyp_len.size());
  std::vector<float> bscore(R);
  IDX_HIP(hipMemcpyAsync(seq.data(), bb.seq, seq.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_len.data(), bb.hyp_len, hyp_len.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_slot.data(), bb.hyp_slot, hyp_slot.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_n.data(), bb.hyp_n, B * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_seq.data(), bb.hyp_seq, hyp_seq.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_score.data(), bb.hyp_score, hyp_score.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(bscore.data(), bb.beam_scores, R * sizeof(float), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(done.data(), bb.done, B * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  // codes [B][n_best][max_new]: each hypothesis, then eos if it fits (already the fill value), stop-padded
  std::vector<BeamHyp> best((size_t)B * n_best);
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * (BEAM_MAX + 1);
    if (beam_finalize(nb, (double)beam->length_penalty, hyp_n[b], &hyp_score[o], &hyp_len[o], &hyp_slot[o], &hyp_seq[o * max_new], max_new,
                      done[b] != 0, &bscore[(size_t)b * nb], &seq[(size_t)b * nb * max_new], steps_done, &best[(size_t)b * n_best], n_best))
      return 1;
    for (int q = 0; q < n_best; ++q) longest = std::max(longest, best[(size_t)b * n_best + q].len);
  }
  const int n_out = std::min(longest + 1, max_new);          // min(sent_lengths.max() + 1, max_length) - prompt
  std::vector<long long> out((size_t)B * n_best * max_new);
  beam_fill_rows(best.data(), B * n_best, max_new, max_new, cfg.stop_mel_token, out.data(), lens, scores);
  IDX_HIP(hipMemcpyAsync(codes, out.data(), out.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  *n_steps_out = n_out;
  return 0;
}

// ---- beam decode session (gpt.h; the greedy session's machinery in gpt.hip) ----
int GPTModel::session_admit_beam(void* ws, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* group_ids,
                                 const int* caps, const idxtts_beam* per_request, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams > 0, "_admit_beam needs a session initialised with num_beams (idxtts_gpt_session_init_beam)");
  IDX_CHECK(per_request, "null pointer");
  GenScope gen_scope(this);
  const int nb = s.shape.num_beams, G = s.shape.slots / nb, d = cfg.model_dim;
  const SessionBuffers sb = carve_session(ws, s.shape);
  const Buffers& w = sb.w;
  auto params = [&]() -> int {      // every request is checked before any group is taken (generate_beam's rules)
    for (int b = 0; b < n; ++b) {
      IDX_CHECK(per_request[b].num_beams == nb, "num_beams differs from the session's");
      if (check_beam(per_request[b])) return 1;
    }
    for (int b = 0; b < n; ++b) {
      const idxtts_beam& r = per_request[b];
      s.beam[group_ids[b]] = SlotBeam{r.do_sample ? 1 : 0, r.temperature, r.top_k, r.top_p, (double)r.length_penalty, r.early_stopping,
                                      r.seed, r.exp_noise};
    }
    IDX_HIP(hipMemcpyAsync(sb.beam, s.beam.data(), G * sizeof(SlotBeam), hipMemcpyHostToDevice, st));
    return 0;
  };
  // one prefill row per request, its keys and values going to every slot of its group
  int S = 0;
  Admission a;
  a.n = n; a.inputs_embeds = inputs_embeds; a.ld_rows = ld_rows; a.prompt_lens = prompt_lens; a.ids = group_ids; a.caps = caps;
  if (admit_prefill(s, sb, a, nb, params, &S, nullptr, st)) return 1;
  BeamState bs = w.beam;
  bs.penalty = s.penalty; bs.group_ids = sb.ids + n; bs.n_ids = n;
  if (beam_session_reset(bs, cfg.start_mel_token, sb.x_last, w.x, S, sb.plen, sb.cap, n, st)) return 1;
  // the first beam step of the admitted groups: the head on all `slots` rows (the GEMV generate_beam's R = slots rows selects), the beam
  // stages on those groups only; the last one writes their first decode inputs
  if (head_logits(w, s.shape.slots, sb.x_last, d, false, st)) return 1;
  if (beam_scores_forward(bs, st) || beam_select_forward(bs, st) || beam_reorder_forward(bs, st)) return 1;
  for (int b = 0; b < n; ++b)
    for (int j = 0; j < nb; ++j) s.busy[group_ids[b] * nb + j] = 1;
  return 0;
}

// BeamSearchScorer.finalize of the group whose first slot is `slot`, with the steps it took: its best hypothesis, then the stop token
// if it fits under the cap (row 0 of generate_beam's codes, cut after its first stop token)
int GPTModel::session_read_beam(Session& s, const SessionBuffers& sb, int slot, long long* codes, int* n_codes, hipStream_t st, int n_best,
                                float* scores) {
  const int nb = s.shape.num_beams, g = slot / nb, L = s.shape.max_new;
  IDX_CHECK(n_best >= 1 && n_best <= nb, "1 <= n_best <= num_beams");
  IDX_CHECK(slot % nb == 0, "a beam session is read at the first slot of a group");
  SlotState hs;
  IDX_HIP(hipMemcpyAsync(&hs, sb.w.slots + slot, sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(!hs.live, "slot is still decoding");
  IDX_CHECK(hs.step >= 1 && hs.step <= hs.max_step && hs.max_step <= L, "slot state corrupt");
  const BeamBuffers& bb = sb.bb;
  const size_t H = BEAM_MAX + 1, o = (size_t)g * H;
  std::vector<int> seq((size_t)nb * L), hyp_len(H), hyp_slot(H), hyp_seq(H * L);
  std::vector<double> hyp_score(H);
  std::vector<float> bscore(nb);
  int hyp_n = 0, done = 0;
  IDX_HIP(hipMemcpyAsync(seq.data(), bb.seq + (size_t)slot * L, seq.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_len.data(), bb.hyp_len + o, H * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_slot.data(), bb.hyp_slot + o, H * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_seq.data(), bb.hyp_seq + o * L, hyp_seq.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(hyp_score.data(), bb.hyp_score + o, H * sizeof(double), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(bscore.data(), bb.beam_scores + slot, nb * sizeof(float), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(&hyp_n, bb.hyp_n + g, sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(&done, bb.done + g, sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(hyp_n >= 0 && hyp_n <= nb, "group state corrupt");
  // n_best = 1: codes holds the hypothesis alone (n_codes[0] entries); else codes [n_best][L], every row stop-padded to L
  std::vector<BeamHyp> best(n_best);
  if (beam_finalize(nb, s.beam[g].length_penalty, hyp_n, hyp_score.data(), hyp_len.data(), hyp_slot.data(), hyp_seq.data(), L, done != 0,
                    bscore.data(), seq.data(), hs.step, best.data(), n_best)) return 1;
  for (const BeamHyp& h : best) IDX_CHECK(h.len >= 0 && h.len <= hs.max_step, "group state corrupt");
  std::vector<long long> out((size_t)n_best * L);
  beam_fill_rows(best.data(), n_best, L, hs.max_step, cfg.stop_mel_token, out.data(), n_codes, scores);
  IDX_HIP(hipMemcpyAsync(codes, out.data(), (n_best == 1 ? (size_t)n_codes[0] : out.size()) * sizeof(long long), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < nb; ++j) s.busy[slot + j] = 0;
  return 0;
}

// ---- preempt and resume of a group (idxtts.h "Preempt and resume, beam sessions"; kernel in decode.hip) ----
ParkGroupArgs GPTModel::park_group_args(const Session& s, const SessionBuffers& sb, int group) const {
  const Buffers& w = sb.w;
  ParkGroupArgs a;
  a.kcache = w.kcache; a.vcache = w.vcache; a.kscale = w.kscale; a.vscale = w.vscale;
  a.layer_bytes = kv_layer_bytes(s.shape.slots, w.Smax); a.layer_scales = kv_layer_scales(s.shape.slots, w.Smax);
  a.group = group; a.Smax = w.Smax; a.B = s.shape.slots; a.bs = w.beam; a.group_tab = sb.beam;
  a.embed = tail_embed(w, use_pl(s.shape.slots));
  return a;
}

int GPTModel::session_park_group_header(void* ws, int group, idxtts_park_group_header* hdr, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams > 0, "_park_group needs a beam session: a greedy or sampled session parks rows (idxtts_gpt_session_park)");
  const int nb = s.shape.num_beams, G = s.shape.slots / nb;
  IDX_CHECK(group >= 0 && group < G, "group out of range");
  IDX_CHECK(s.busy[group * nb], "group holds no request");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  const SessionBuffers sb = carve_session(ws, s.shape);
  SlotState hs;
  int hyp_n = 0, done = 0;
  IDX_HIP(hipMemcpyAsync(&hs, sb.w.slots + group * nb, sizeof(SlotState), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(&hyp_n, sb.bb.hyp_n + group, sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipMemcpyAsync(&done, sb.bb.done + group, sizeof(int), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(hs.live, "group has ended: read it, a request that is over cannot be parked");
  IDX_CHECK(hs.step >= 1 && hs.step < hs.max_step && hs.max_step <= s.shape.max_new && hs.pos >= hs.step && hs.pos < sb.w.Smax &&
            hs.mel_pos == hs.step + 1, "group state corrupt");
  IDX_CHECK(hyp_n >= 0 && hyp_n <= nb && (done == 0 || done == 1), "group state corrupt");
  const SlotBeam& e = s.beam[group];
  idxtts_park_group_header h{};
  h.magic = IDXTTS_PARK_GROUP_MAGIC; h.version = IDXTTS_PARK_GROUP_VERSION;
  h.layers = cfg.layers; h.heads = cfg.heads; h.model_dim = cfg.model_dim; h.number_mel_codes = cfg.number_mel_codes;
  h.slots = s.shape.slots; h.num_beams = nb; h.kv_format = s.kv_fmt; h.gemm_mode = s.gemm_mode;
  h.pos = hs.pos; h.mel_pos = hs.mel_pos; h.step = hs.step; h.max_step = hs.max_step;
  h.do_sample = e.do_sample; h.temperature = e.temperature; h.top_k = e.top_k; h.top_p = e.top_p;
  h.length_penalty = e.length_penalty; h.early_stopping = e.early_stopping; h.batch_invariant = s.invariant;
  h.seed = e.seed; h.exp_noise = (unsigned long long)(uintptr_t)e.exp_noise;
  h.hyp_n = hyp_n; h.done = done;
  h.bytes = park_group_layout(h.kv_format, h.layers, h.heads, h.number_mel_codes, nb, h.pos, h.step).bytes;
  *hdr = h;
  return 0;
}

size_t GPTModel::session_park_group_bytes(void* ws, int group, hipStream_t st) {
  idxtts_park_group_header h;
  return session_park_group_header(ws, group, &h, st) ? 0 : (size_t)h.bytes;
}

int GPTModel::session_park_group(void* ws, int group, void* dst, size_t dst_bytes, size_t* written, hipStream_t st) {
  IDX_CHECK(dst, "null pointer");
  IDX_CHECK((uintptr_t)dst % 16 == 0, "the parked group must be 16-byte aligned");
  idxtts_park_group_header h;
  if (session_park_group_header(ws, group, &h, st)) return 1;
  IDX_CHECK(dst_bytes >= h.bytes, "dst is smaller than the parked group (idxtts_gpt_session_park_group_bytes)");
  Session& s = *find_session(ws);
  const int nb = s.shape.num_beams;
  ParkGroupArgs a = park_group_args(s, carve_session(ws, s.shape), group);
  a.hdr = h; a.blob = static_cast<char*>(dst);
  if (idxtts::session_park_group(a, st)) return 1;
  // the host image too: the next admission uploads the whole SlotBeam table, and a free group carries no request's parameters
  s.beam[group] = SlotBeam{0, 1.0f, 0, 1.0f, 0.0, 0, 0, nullptr};
  for (int j = 0; j < nb; ++j) s.busy[group * nb + j] = 0;
  if (written) *written = (size_t)h.bytes;
  return 0;
}

int GPTModel::session_resume_group(void* ws, int group, const void* src, size_t src_bytes, hipStream_t st) {
  IDX_SESSION(ws);
  IDX_CHECK(s.shape.num_beams > 0, "_resume_group needs a beam session: a greedy or sampled session resumes rows (idxtts_gpt_session_resume)");
  const int nb = s.shape.num_beams, G = s.shape.slots / nb;
  IDX_CHECK(src, "null pointer");
  IDX_CHECK((uintptr_t)src % 16 == 0, "the parked group must be 16-byte aligned");
  IDX_CHECK(group >= 0 && group < G, "group out of range");
  IDX_CHECK(!s.busy[group * nb], "group is not free");
  IDX_CHECK(kv_fmt == s.kv_fmt && get_gemm_mode() == s.gemm_mode, "KV format or GEMM mode changed since the session was initialised");
  IDX_CHECK(batch_invariant == s.invariant, "batch-invariant mode changed since the session was initialised");
  IDX_CHECK(src_bytes >= sizeof(idxtts_park_group_header), "parked group shorter than its header");
  idxtts_park_group_header h;
  IDX_HIP(hipMemcpyAsync(&h, src, sizeof(h), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  IDX_CHECK(h.magic == IDXTTS_PARK_GROUP_MAGIC, "not a parked group (magic; a parked row goes to idxtts_gpt_session_resume)");
  IDX_CHECK(h.version == IDXTTS_PARK_GROUP_VERSION, "parked group of another format version");
  IDX_CHECK(h.layers == cfg.layers && h.heads == cfg.heads && h.model_dim == cfg.model_dim && h.number_mel_codes == cfg.number_mel_codes,
            "parked group of another model (dimensions)");
  IDX_CHECK(h.num_beams == nb, "parked group of another num_beams");
  IDX_CHECK(h.batch_invariant == 0 || h.batch_invariant == 1, "parked group's mode field is corrupt");
  IDX_CHECK(h.batch_invariant == s.invariant, "parked group and session differ in the batch-invariant mode");
  // seeded draws index with slots / num_beams, the key split and the GEMV follow the row count; in the mode none of them does
  IDX_CHECK(s.invariant || h.slots == s.shape.slots, "parked group of a session with a different number of slots");
  IDX_CHECK(h.kv_format == s.kv_fmt, "parked group of another KV format");
  IDX_CHECK(h.gemm_mode == s.gemm_mode, "parked group of another GEMM mode");
  const SessionBuffers sb = carve_session(ws, s.shape);
  IDX_CHECK(h.max_step >= 1 && h.max_step <= s.shape.max_new, "token cap above the session's max_new_tokens");
  IDX_CHECK(h.step >= 1 && h.step < h.max_step && h.mel_pos == h.step + 1 && h.pos >= h.step, "parked group's step scalars are corrupt");
  IDX_CHECK((long long)h.pos + (h.max_step - h.step) + 1 <= sb.w.Smax, "the request's remaining steps do not fit the session's cache");
  IDX_CHECK(h.hyp_n >= 0 && h.hyp_n <= nb && (h.done == 0 || h.done == 1), "parked group's scorer fields are corrupt");
  idxtts_beam r{nb, h.do_sample, h.temperature, h.top_k, h.top_p, (float)h.length_penalty, h.early_stopping,
                reinterpret_cast<const float*>((uintptr_t)h.exp_noise), h.seed};
  IDX_CHECK(h.do_sample == 0 || h.do_sample == 1, "parked group's beam parameters are corrupt");
  if (check_beam(r)) return 1;
  IDX_CHECK(h.bytes == park_group_layout(h.kv_format, h.layers, h.heads, h.number_mel_codes, nb, h.pos, h.step).bytes,
            "parked group's size field is corrupt");
  IDX_CHECK(src_bytes >= h.bytes, "parked group is truncated");
  ParkGroupArgs a = park_group_args(s, sb, group);
  a.hdr = h; a.blob = const_cast<char*>(static_cast<const char*>(src));
  if (idxtts::session_resume_group(a, st)) return 1;
  s.beam[group] = SlotBeam{h.do_sample, h.temperature, h.top_k, h.top_p, h.length_penalty, h.early_stopping, h.seed,
                           reinterpret_cast<const float*>((uintptr_t)h.exp_noise)};
  for (int j = 0; j < nb; ++j) s.busy[group * nb + j] = 1;
  return 0;
}

}  // namespace idxtts
