#pragma once
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/idxtts.h"
#include "attention.h"
#include "beam.h"
#include "ctx.h"
#include "decode.h"
#include "gemm.h"
#include "gemv16.h"
#include "gemv_pl.h"
#include "norm.h"
#include "prof.h"

namespace idxtts {

struct Carver;      // model_util.h

// beam search buffers after a decode workspace (gpt_beam.hip): B utterances (session: groups) x nb rows
struct BeamBuffers {
  float *proc, *beam_scores;
  int *next_tok, *beam_idx, *seq, *hyp_len, *hyp_slot, *hyp_seq, *hyp_n, *done;
  double *hyp_score, *hyp_worst;
  size_t bytes;
};
BeamBuffers carve_beam(void* ws, int B, int nb, int V, int max_new);

struct GPTLayer {
  const float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  LinearWeights attn_l, proj_l, fc_l, fc2_l;     // MFMA-32x32 packed (prefill / latent pass)
  WeightStream attn_g, proj_g, fc_g, fc2_g;      // stream-order packed (decode, kdepth 16); attn_g / fc_g carry diag(ln_g) folded in
  WeightStream attn_p, proj_p, fc_p, fc2_p;      // compact formats only: kdepth 32, the bf16-MFMA order of the plane GEMV (gemv_pl.h), 5..64 rows
  const float *attn_u = nullptr, *attn_c = nullptr;   // folded LayerNorm 1: colsum(diag(g) W), b . W + bias
  const float *fc_u = nullptr, *fc_c = nullptr;       // folded LayerNorm 2
};

// a captured decode step and its instance (plain data: whoever holds one drops it)
struct StepGraph {
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
  void drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr;
  }
};

struct GPTModel : ModelBase {
  idxtts_gpt_config cfg;
  std::vector<GPTLayer> layers;
  const float *lnf_g = nullptr, *lnf_b = nullptr, *fn_g = nullptr, *fn_b = nullptr;
  WeightStream head_g, head_p;
  const float* head_b = nullptr;
  const float *mel_emb = nullptr, *text_emb = nullptr, *mel_pos = nullptr, *text_pos = nullptr;
  int weight_fmt = WFMT_F32;      // storage format of the decode weight streams (quantize_weights)
  int kv_fmt = 0;                 // KV cache of the cached generation: 0 = fp32, 1 = bf16, 2 = scaled fp8 (keys / values rounded when produced; decode.h)
  // idxtts_gpt_set_batch_invariant: every launch that feeds the choice of a code is chosen from the request alone (idxtts.h
  // "Batch-invariant mode") -- fp32-MFMA GEMV in its 16-row-tile forms at every row count, decode attention in pieces that follow the
  // row's own key count, exact prefill GEMMs with key tiles counted from the row's first key, seeded draws without a term in B
  int batch_invariant = 0;
  std::atomic<int> generating{0}; // generate() / generate_beam() calls in flight: idxtts_gpt_set_kv_format refuses to switch under them
  struct GenScope { GPTModel* m; explicit GenScope(GPTModel* mm) : m(mm) { m->generating.fetch_add(1); } ~GenScope() { m->generating.fetch_sub(1); } };
  size_t kv_layer_bytes(int B, int Smax) const { return (size_t)B * cfg.heads * Smax * 64 * (kv_fmt == 2 ? 1 : kv_fmt ? 2 : 4); }
  size_t kv_layer_scales(int B, int Smax) const { return kv_fmt == 2 ? (size_t)B * cfg.heads * Smax : 0; }      // fp8: one per cached vector
  hipStream_t own_stream = nullptr;
  static constexpr int OOB_SLOTS = 64;
  int* oob_flag = nullptr;        // device ints (one per embed() call in flight): set by the embedding gather when an index exceeds its table
  std::atomic<unsigned> oob_next{0};
  ~GPTModel() override {
    for (GraphSlot& g : graph_cache) g.step.drop();
    for (auto& kv : sessions) kv.second.step.drop();
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }

  struct Buffers {
    float *x, *h, *qkv, *att, *ff;            // [B*S][..] prefill / latent activations
    char *kcache, *vcache; int Smax;          // [L][B][H] x (Smax x 64 elements) each; fp32, bf16 or fp8 elements (kv_fmt, decode.h)
    float *kscale = nullptr, *vscale = nullptr;   // fp8 cache only: [L][B][H][Smax] scales, carved right after the codes
    float *xd, *hd, *attd, *ffd;              // decode residual / final-normed / attention output / mlp hidden: A-fragment images
    // plane-GEMV decode step (gemv_pl.h; compact weight streams, more than 4 rows): every activation a plain fp32 row-major matrix,
    // per-16-column row statistics for the folded LayerNorms, K-part partial sums and arrival counters
    float *xrow, *hrow, *attrow, *ffrow, *stats, *pl_slab; unsigned* pl_cnt;
    float *qkvd, *logits, *slab;              // [B][3d], [B][V] row-major; [<=8][B][d] K-split partial sums of mlp.c_proj
    size_t frag_off, frag_bytes;              // the fragment-image region (zeroed once per generate: padding rows stay 0)
    unsigned char* seen; int *finished, *cur_tok, *kstart;
    float* attn_part; unsigned* attn_cnt;     // key-split decode attention: [B][H][<=16][66] partials, [B][H] counters
    unsigned* ksb_cnt;                        // [d/16] arrival counters of the fused K-split mlp.c_proj (zeroed per generate)
    DecodeState* state;
    long long* codes;                         // [B][max_new] generated codes of the call in flight (copied to the caller's tensor at the end)
    size_t bytes;
    // The step's tail (its last launches) is chosen from these fields alone:
    SlotState* slots = nullptr;               // decode session only (carve_session): per-row step scalars; the step uses them, not `state`
    SlotSampling* slot_samp = nullptr;        // sampled decode session only: each slot's sampler (the step samples with it)
    idxtts_sampling samp{0, 1.0f, 0, 1.0f, nullptr, 0};      // generate(): the call's sampler (mode 0 = greedy)
    const long long* forced = nullptr; int forced_ld = 0;   // generate_forced: [B][forced_ld] tokens fed back instead of the argmax
    int invariant = 0;                        // the context's batch_invariant when the buffers were carved
    float* logprobs = nullptr;                // scores (idxtts.h "Scores"): [B][codes_ld] beside `codes` -- a scored session's table in
                                              // its workspace, generate()'s caller's buffer -- or null: the samplers record none
    bool beam_tail = false;                   // the beam stages on `beam`: a beam session's (slots set) or generate_beam's
    bool kv_scratch = false;                  // score(): kcache / vcache hold ONE layer, rewritten by every layer -- only the rounding of the
                                              // keys and values in place (decode.h kv_store_prefill) is kept; an fp32 cache stores nothing
    BeamState beam;
  };
  // Instantiated decode-step graphs of greedy generations, keyed by everything the captured launches depend on (workspace
  // address and carve, batch, penalty): a server replaying the same shapes on the same stream re-captures nothing.
  struct GraphSlot {
    void* ws = nullptr; size_t ws_bytes = 0; int B = 0, S = 0, max_new = 0; float penalty = 0.0f; int kv_fmt = 0, geom = 0;
    float* logprobs = nullptr;      // the caller's scores buffer the captured samplers write (null: none); the one address outside ws
    StepGraph step; unsigned long stamp = 0; bool in_use = false;
  };
  std::vector<GraphSlot> graph_cache;
  std::mutex graph_mu;
  unsigned long graph_stamp = 0;
  static constexpr size_t GRAPH_CACHE_MAX = 8;

  explicit GPTModel(const idxtts_gpt_config& c);
  bool accepts(const std::string& name) const override;
  int finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) override;
  // Host transform of the staged tensors (before finalize) into the model a compact decode format can hold exactly:
  //   (ln_g, ln_b, W, b) of c_attn / c_fc -> (1, 0, Q(diag(ln_g) W), ln_b . W + b);  c_proj, mlp.c_proj, mel_head -> Q(W).
  // Every consumer (prefill, latent pass, decode) is then packed from these tensors, so they all run the SAME model.
  int quantize_weights(std::map<std::string, HostTensor>& t, int fmt);
  // prefill_rows: rows of the prefill / latent activations (0 = B * S)
  Buffers carve(void* ws, int B, int S, int max_new, size_t prefill_rows = 0) const;
  size_t workspace_bytes(int B, int S, int max_new) const;
  struct KvScatter {      // decode-session admission: prefill row b's positions [0, len[b]) go to the cache rows of slot slot_ids[b]
    const int* slot_ids = nullptr; const int* len = nullptr; int n = 0; int slots = 0;
    int fan = 1;          // beam sessions: row b goes to the fan slots slot_ids[b] .. slot_ids[b] + fan - 1 (its group)
    const int* first = nullptr;      // takes (fan = 1): row b goes to the slots slot_ids[first[b]] .. slot_ids[first[b + 1] - 1]
  };
  int layer_full(int li, const Buffers& w, int B, int S, const int* kstart, bool store_kv, hipStream_t st, const KvScatter* scatter = nullptr);
  int head_logits(const Buffers& w, int B, const float* x, int ldx, bool x_frag, hipStream_t st);      // ln_f -> final_norm -> mel_head
  // the step's tail writes w.codes [B][codes_ld]; pos_hint: keys the step reads as the host knows them (profiler accounting; 0 when
  // the step is captured)
  int head_and_sample(const Buffers& w, int B, const float* x, int ldx, bool x_frag, float penalty, int codes_ld, float* logits_out,
                      hipStream_t st);
  KvDst kv_dst(int li, const Buffers& w, int rows) const;      // layer li of a cache laid out for `rows` rows, as its producers write it
  DecodeAttnArgs attn_args(int li, const Buffers& w, int B, int pos_hint) const;      // layer li's decode attention; the caller sets out / out_row
  SampleArgs::Embed tail_embed(const Buffers& w, bool pl) const;                      // the fused tail's next-input block (st_rw left to the caller)
  int decode_step(const Buffers& w, int B, float penalty, int codes_ld, float* logits_base, int pos_hint, hipStream_t st);
  int decode_step_pl(const Buffers& w, int B, float penalty, int codes_ld, float* logits_base, int pos_hint, hipStream_t st);
  int capture_step(const Buffers& w, int B, float penalty, int codes_ld, hipStream_t st, StepGraph* g);   // one decode step -> *g
  bool use_pl(int B) const;                   // this many decode rows run on the plane GEMV (never in the batch-invariant mode)
  int step_key() const;                       // what a captured step's kernels were chosen by besides shape and KV format: the two
                                              // process-wide decode switches, or the batch-invariant mode, which ignores both
  bool fused_tail(const Buffers& w) const;    // w's step tail also writes the next input and advances: no embed_step / advance_state
  // generate() and generate_beam() are re-entrant across host threads, each call with its own workspace and stream; both run on
  // call_stream()'s stream through run_generation() (gpt.hip): R = B * fan rows, row r on prompt r / fan, the step tail w's own
  int call_stream(hipStream_t user, hipStream_t* st);
  struct GenerateCall {      // what one generate call may carry besides its shape and buffers; a caller names the fields it sets
    const idxtts_sampling* sampling = nullptr;      // null (or mode 0): greedy
    const long long* forced = nullptr;              // generate_forced: [B][max_new] tokens fed back instead of the argmax
    int takes = 1;                   // takes > 1: B * takes decode rows (codes, logits, exp_noise, ws sized for them), one prefill row per
                                     // prompt, each row's KV and last position fanned out to its takes' decode rows
    float* logprobs = nullptr;       // device [B * takes][max_new]: every code's log-probability (idxtts.h "Scores")
    struct Prefix {                  // k > 0: continue behind given codes (idxtts.h), one row per prompt; the prefill runs on
      const long long* codes = nullptr;      // P + 1 + k positions and the state starts behind the prefix.  codes: device [B][k],
      const long long* host = nullptr;       // host: their host copy (generate() makes it and checks the codes)
      int k = 0, pos0 = 1;           // prefix code j at mel position pos0 + j: 1 (the reference's layout) or 2 (the uninterrupted run's)
    } prefix;
  };
  // fan rows per prompt: call.takes of them behind one shared prefill row (generate), or fan prefill rows with call.takes = 1 (beams)
  int run_generation(const Buffers& w, const float* inputs_embeds, const int* pad_left_host, int B, int fan, int P, int max_new,
                     float penalty, float* logits_out, bool graph, hipGraphExec_t exec, StepGraph* captured, const int* poll, int poll_n,
                     int poll_every, int* steps_done, hipStream_t st, const GenerateCall& call);
  int generate(const float* inputs_embeds, const int* pad_left_host, int B, int P, int max_new, float penalty, long long* codes,
               int* n_steps_out, float* logits_out, void* ws, size_t ws_bytes, int use_graph, hipStream_t st, const GenerateCall& call);
  // Beam search / beam-sample (HF _beam_search; the reference's default decoding mode, infer_v2.py:714-722): B utterances x
  // num_beams rows through the same decode step, selection / hypotheses / re-indexing on the device (beam.hip).
  size_t beam_workspace_bytes(int B, int nb, int S, int max_new) const;
  BeamState beam_state(const Buffers& w, const BeamBuffers& bb, int B, int nb, int seq_ld) const;   // the fields both beam paths share
  int generate_beam(const float* inputs_embeds, const int* pad_left_host, int B, int P, int max_new, float penalty, const idxtts_beam* beam,
                    long long* codes, int* n_steps_out, void* ws, size_t ws_bytes, int use_graph, hipStream_t st, int n_best = 1,
                    int* lens = nullptr, float* scores = nullptr);      // codes [B][n_best][max_new]; lens / scores: HOST [B][n_best]
  // Scoring given codes (idxtts.h): one prefill over [prompt | start | codes], the head over the scored positions in chunks of at most
  // SCORE_CHUNK packed rows, score_rows_kernel behind each chunk
  static constexpr int SCORE_CHUNK = 64;
  struct ScoreHead {                  // what score_positions works in
    Buffers w;                        // head_logits' fields for SCORE_CHUNK rows (hd, hrow, logits, pl_slab); the rest the owner's
    size_t hd_bytes = 0;
    float* xs = nullptr;              // [SCORE_CHUNK][d] the chunk's hidden rows, packed
    int *tok = nullptr, *dst = nullptr;      // [positions] each packed position's code and where its value goes
  };
  struct ScoreRun { const float* x; int rows; };      // consecutive hidden rows (device, d floats each) to be scored
  struct ScoreBuffers {
    Buffers w;                        // prefill activations for B * S rows
    ScoreHead head;
    long long* fed;                   // [B][n - 1] the codes the prefill feeds (padding: code 0)
    size_t bytes;
  };
  ScoreHead carve_score_head(Carver& c, const Buffers& base, size_t positions) const;
  int score_positions(const ScoreHead& h, const std::vector<ScoreRun>& runs, const std::vector<int>& tok, const std::vector<int>& dst, float* out,
                      float* logits_out, hipStream_t st);
  ScoreBuffers carve_score(void* ws, int B, int S) const;
  size_t score_workspace_bytes(int B, int P, int n) const { return carve_score(nullptr, B, P + n).bytes; }
  int score(const float* inputs_embeds, const int* pad_left_host, int B, int P, const long long* codes, const int* lens_host, int n, int pos0,
            float* logprobs, float* logits_out, void* ws, size_t ws_bytes, hipStream_t st);
  int latent(const float* emb, const int* pad_left_host, int B, int S, int mel_start, int M, float* latent_out, void* ws, size_t ws_bytes,
             hipStream_t st);

  // ---- decode session (continuous batching): `slots` decode rows with one KV region each; requests are admitted into free slots
  // between steps, every slot advances on its own (SlotState), a slot ends on the stop token or its own cap and is read out.  Greedy,
  // or (sampled sessions) each request with its own sampler and draws.  A row's codes equal row 0 of generate() on `slots` copies of it
  // (pad_left 0): every kernel on its path is chosen from the session's properties (slots, KV format, GEMM mode) alone, never from how
  // many rows are admitted at once.
  struct SessionShape {      // what a session's workspace is carved by (carve_session): fixed at _init
    int slots = 0, max_prompt = 0, max_new = 0;
    bool sampled = false;             // IDXTTS_SESSION_SAMPLED: per-slot samplers (SlotSampling table in the workspace)
    int num_beams = 0;                // beam sessions: slots / num_beams groups of num_beams consecutive slots, one request each
    bool scores = false;              // IDXTTS_SESSION_SCORES: [slots][max_new] log-probabilities behind everything else (w.logprobs)
    bool prefix = false;              // IDXTTS_SESSION_PREFIX: a prefill area that holds one row of max_prompt + 1 + max_new positions
    bool prefix_scores = false;       // IDXTTS_SESSION_PREFIX_SCORES (with prefix and scores): the scoring head's buffers and the packed
                                      // log-probability staging buffer behind everything else (SessionBuffers::score, lp_stage)
  };
  struct Session {      // host-side record, keyed by the workspace address (the caller owns the workspace)
    SessionShape shape; float penalty = 1.0f; int kv_fmt = 0, gemm_mode = 0;
    int invariant = 0;                // the context's batch-invariant mode at _init: the session keeps it (changed since: every call refuses)
    std::vector<SlotSampling> samp;   // host image of the SlotSampling table (sampled sessions), copied whole at each admission
    std::vector<SlotBeam> beam;       // host image of the SlotBeam table (beam sessions), copied whole at each admission
    size_t ws_bytes = 0;
    std::vector<char> busy;           // admitted and not yet read
    std::vector<int> prompt;          // greedy / sampled sessions: prompt length P of the request in each busy slot (fork needs it)
    std::vector<char> first_in;       // ... and whether x_last[slot] still is that request's last prefill row (not after a resume)
    bool warm = false;                // one step has run eagerly (first-use function attributes are set outside a capture)
    int geom = -1;                    // decode geometry the graph was captured under
    StepGraph step;
  };
  std::map<void*, Session> sessions;
  std::mutex session_mu;
  struct SessionBuffers {
    Buffers w;                        // decode buffers for `slots` rows (w.slots set) + the admission prefill's activations
    float* x_last;                    // [slots][d] last valid prefill row of each admitted request (first-token head input)
    int *ids, *plen, *klen, *cap;     // admission staging: slot ids, prompt lengths (prefill rows: -1 = padding row), P + 1, caps
    int *pk, *poff;                   // IDXTTS_SESSION_PREFIX: [slots] prefix length of each admitted request and its offset in the packed codes
    ScoreHead score;                  // IDXTTS_SESSION_PREFIX_SCORES: the admission prefill's scoring head ...
    float* lp_stage = nullptr;        // ... and [slots * max_new] the admitted prefixes' log-probabilities, packed as the codes are
    SlotSampling* samp;               // [slots] per-slot samplers (sampled sessions only, else null)
    BeamBuffers bb;                   // beam sessions: proc, beam scores, next_tok, beam_idx, seq [slots][max_new], hypotheses per group
    SlotBeam* beam;                   // [groups] per-request beam parameters (beam sessions only, else null)
    size_t bytes;
  };
  // prefix_new (IDXTTS_SESSION_PREFIX: the session's max_new, else 0): at least one row of max_prompt + 1 + max_new positions as well
  size_t session_prefill_rows(int slots, int max_prompt, int prefix_new = 0) const {
    const size_t rows = (size_t)slots * (max_prompt + 1) + 256;
    return prefix_new > 0 ? std::max(rows, (size_t)max_prompt + 1 + prefix_new + 256) : rows;
  }
  // sampled: the SlotSampling table is carved after everything else, so a greedy session's layout and size are those of before;
  // num_beams > 0 (beam session): the beam buffers and the SlotBeam table likewise
  SessionBuffers carve_session(void* ws, const SessionShape& shape) const;
  size_t session_workspace_bytes(const SessionShape& shape) const;
  Session* find_session(void* ws);
#define IDX_SESSION(ws) /* `s`: the session on this workspace, or the calling method refuses */ \
  Session* const session_of_ws = find_session(ws);                                               \
  IDX_CHECK(session_of_ws, "no decode session on this workspace");                               \
  Session& s = *session_of_ws
  int session_init(void* ws, size_t ws_bytes, const SessionShape& shape, float penalty, hipStream_t st);
  struct Admission {      // n requests for free units of a session; a caller names the fields it sets
    int n = 0, ld_rows = 0;
    const float* inputs_embeds = nullptr;      // device [n][ld_rows][d], right-padded
    const int* prompt_lens = nullptr;          // HOST [n]
    const int *ids = nullptr, *caps = nullptr; // HOST: the free units -- slots, or (beam sessions) groups -- and a token cap for each
    const idxtts_sampling* per_row = nullptr;      // null = every row greedy; else one sampler per row (sampled sessions only)
    const int* takes = nullptr;       // null, or takes[b] >= 1 slots per request: ids, caps and per_row then have one entry per take,
                                      // request after request, and the request's one prefill row's keys and values go to all of them
    // sessions with IDXTTS_SESSION_PREFIX (idxtts.h "Continuing from given codes"); all of them null: the call of before
    const int* prefix_lens = nullptr;           // HOST [n]: request b's prefill row holds P_b + 1 + prefix_lens[b] positions, the last
    const long long* prefix = nullptr;          // prefix_lens[b] of them its codes of this packed device array (one behind the other)
    const float* prefix_logprobs = nullptr;     // device fp32, packed likewise, or null: what _read_scored returns for those codes
    const unsigned char* from_model = nullptr;  // HOST [n] (_admit_prefix_scored): 1 = request b's values come from this prefill instead
  };
  // The admission both session kinds share: a.n requests into the free units a.ids[] -- slots, or (fan > 1) groups of fan slots -- each
  // checked, `params` (the caller's checks and table upload) run, before any unit is taken; then one right-padded prefill, each row's
  // keys and values going to its unit's slots.  *S: positions per prefill row; *take_row (a.takes): device array, the prefill row of
  // each take; the prefixes' lengths and offsets are left in sb.pk / sb.poff.
  int admit_prefill(Session& s, const SessionBuffers& sb, const Admission& a, int fan, const std::function<int()>& params, int* S,
                    const int** take_row, hipStream_t st);
  int session_first_tokens(const Session& s, const SessionBuffers& sb, int n, hipStream_t st);      // of the n slots in sb.ids
  int session_admit(void* ws, const Admission& a, hipStream_t st);
  // n further takes of the request in slot src, cut back to `at` codes, in the free slots dst_slots (idxtts.h); samplers: null = greedy
  // takes; caps: null = the source's cap.  Every refusal happens before anything changes.
  int session_fork(void* ws, int src, int at, int n, const int* dst_slots, const idxtts_sampling* samplers, const int* caps, hipStream_t st);
  // beam sessions: n requests into the free groups group_ids, each with its own idxtts_beam (num_beams == the session's); every request
  // is checked before any group is taken.  One prefill row per request, its KV fanned out to the group's slots; then its first beam step.
  int session_admit_beam(void* ws, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* group_ids,
                         const int* max_new, const idxtts_beam* per_request, hipStream_t st);
  int session_read_beam(Session& s, const SessionBuffers& sb, int slot, long long* codes, int* n_codes, hipStream_t st, int n_best = 1,
                        float* scores = nullptr);
  int session_read_nbest(void* ws, int slot, int n_best, long long* codes, int* lens, float* scores, hipStream_t st);
  int session_step(void* ws, int n_steps, int use_graph, int* finished_slots, int* n_finished, hipStream_t st);
  // logprobs: null = _read; else _read_scored (device fp32, the slot's log-probabilities; a scored session only)
  int session_read(void* ws, int slot, long long* codes, int* n_codes, hipStream_t st, float* logprobs = nullptr, bool scored = false);
  // Ends the requests in slot_ids (HOST; beam sessions: the first slot of each group) from outside the step.  evict: they are free at
  // once -- admissible in the next admit, never reported by a later step; allowed on a live request and on one that ended and was not
  // read.  Otherwise stop: a live request ends as if its cap were the codes it has (the next step reports it, read returns them); one
  // that has ended is left alone.  One id that is out of range, holds no request or is no group's first slot refuses the whole call.
  int session_end(void* ws, int n, const int* slot_ids, bool evict, hipStream_t st);
  // Preempt and resume (idxtts.h): park gathers a live slot's state into the parked row dst and frees the slot; resume scatters a parked
  // row into a free slot and marks it busy.  Greedy and sampled sessions; every refusal happens before anything changes.
  ParkArgs park_args(const Session& s, const SessionBuffers& sb, int slot) const;      // everything but hdr and blob
  int session_park_header(void* ws, int slot, idxtts_park_header* hdr, hipStream_t st);   // the checks of park + the slot's header now
  size_t session_park_bytes(void* ws, int slot, hipStream_t st);
  int session_park(void* ws, int slot, void* dst, size_t dst_bytes, size_t* written, hipStream_t st);
  int session_resume(void* ws, int slot, const void* src, size_t src_bytes, hipStream_t st);
  // The same for a beam session's group (idxtts.h "Preempt and resume, beam sessions"; gpt_beam.hip): park also clears the group's
  // busy flags, resume restores them and the host image of the group's SlotBeam entry, which every admission uploads whole.
  ParkGroupArgs park_group_args(const Session& s, const SessionBuffers& sb, int group) const;      // everything but hdr and blob
  int session_park_group_header(void* ws, int group, idxtts_park_group_header* hdr, hipStream_t st);
  size_t session_park_group_bytes(void* ws, int group, hipStream_t st);
  int session_park_group(void* ws, int group, void* dst, size_t dst_bytes, size_t* written, hipStream_t st);
  int session_resume_group(void* ws, int group, const void* src, size_t src_bytes, hipStream_t st);
  int session_release(void* ws);
  int embed(float* out, int rows, const int* text_ids, const int* text_pos_idx, const int* mel_ids, const int* mel_pos_idx,
            const float* extra, const int* extra_idx, hipStream_t st);
};

// BeamSearchScorer.finalize for one utterance (transformers_beam_search.py:320-414) on host copies of its device state: the finished
// hypotheses (hyp_* rows of the utterance, hyp_seq [BEAM_MAX + 1][seq_ld]) and, unless `done`, its nb open beams (bscore [nb], seq
// [nb][seq_ld]) scored at steps_done tokens.  Returns the best hypothesis (tokens point into hyp_seq or seq).
struct BeamHyp { double score; const int* toks; int len; };
int beam_finalize(int nb, double length_penalty, int hyp_n, const double* hyp_score, const int* hyp_len, const int* hyp_slot,
                  const int* hyp_seq, int seq_ld, bool done, const float* bscore, const int* seq, int steps_done, BeamHyp* best,
                  int n_best = 1);      // n_best > 1: best [n_best], finalize's order -- best first, of equal scores the one added later first

// The rows an n-best read returns: row q of out [n][ld] = hypothesis q, then the stop token to the end of the row; lens[q] = the
// hypothesis and the stop token behind it where that fits under `cap`; scores[q] = its score (lens / scores may be null)
void beam_fill_rows(const BeamHyp* hyps, int n, int ld, int cap, int stop_token, long long* out, int* lens, float* scores);

}  // namespace idxtts
