// IndexTTS-2 semantic-to-mel stage on MI355X: gpt_layer + vq2emb + length regulator, and the CFM Euler
// solver over the DiT (13 adaLN-RMSNorm/rotary/SwiGLU blocks with U-ViT skips) + WaveNet estimator.
//
// Reference: infer_v2.py:835-856 (caller), commons.py:390-420 (MyModel), length_regulator.py:90-141,
// flow_matching.py:31-115, diffusion_transformer.py:186-257, gpt_fast/model.py:121-360, wavenet.py:138-166.
//
// Layout: everything is token-major [rows = (stacked batch, frame)][channels] so that every linear AND every
// convolution (WaveNet k=5 reflect-pad, length-regulator k=3) is the same fp32-MFMA GEMM (gemm.hip; the conv
// taps are shifted row reads inside the tile loader, no im2col, no transposes between the DiT and the WaveNet).
// Only the 80-channel ODE state x stays channels-first [B][80][T] (the boundary layout, flow_matching.py:52).
//
// What is hoisted out of the Euler loop (all of it depends on t only, not on the data):
//   timestep MLPs, all 27 adaLN modulation vectors, the FinalLayer shift/scale and the WaveNet conditioning
//   bias g_l (folded with the in_layer bias) are computed ONCE per call for all steps by five small GEMMs
//   with M = n_steps; cond_projection(mu) is computed once per call.  The reference recomputes all of them
//   in every step (diffusion_transformer.py:212-213, wavenet.py:142-152).
// CFG: the [cond | null] stacking of flow_matching.py:89-93 is kept (2B rows per step).
#include <algorithm>
#include <cmath>
#include <cstring>

#include <map>
#include <mutex>
#include <utility>

#include "model_util.h"
#include "s2mel.h"
#include "s2mel_buffers.h"

namespace idxtts {

S2MelModel::S2MelModel(const idxtts_s2mel_config& c) : cfg(c) {}

bool S2MelModel::accepts(const std::string& name) const {
  static const char* prefixes[] = {"cfm.estimator.", "length_regulator.", "gpt_layer.", "semantic_codec.", "rope_cache"};
  for (const char* p : prefixes)
    if (name.rfind(p, 0) == 0) return true;
  return false;
}

namespace {

// columns [k0, k1) of a [N][K] matrix
std::vector<float> col_slice(const std::vector<float>& w, int N, int K, int k0, int k1) {
  std::vector<float> o((size_t)N * (k1 - k0));
  for (int n = 0; n < N; ++n) std::memcpy(&o[(size_t)n * (k1 - k0)], &w[(size_t)n * K + k0], (k1 - k0) * sizeof(float));
  return o;
}

// interleave two [H][K] blocks as [32 of a | 32 of b] groups (SwiGLU / tanh-sigmoid gate packing)
std::vector<float> pair_pack(const float* a, const float* b, int H, int K) {
  std::vector<float> o((size_t)2 * H * K);
  for (int blk = 0; blk < H / 32; ++blk) {
    std::memcpy(&o[(size_t)(blk * 64) * K], a + (size_t)blk * 32 * K, (size_t)32 * K * sizeof(float));
    std::memcpy(&o[(size_t)(blk * 64 + 32) * K], b + (size_t)blk * 32 * K, (size_t)32 * K * sizeof(float));
  }
  return o;
}

// torch Conv1d weight [Cout][Cin][k] -> [Cout][k*Cin] (tap-major K, the order the conv-mode tile loader walks)
std::vector<float> conv_to_rows(const std::vector<float>& w, int Cout, int Cin, int k) {
  std::vector<float> o((size_t)Cout * Cin * k);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int kk = 0; kk < k; ++kk) o[((size_t)co * k + kk) * Cin + ci] = w[((size_t)co * Cin + ci) * k + kk];
  return o;
}

}  // namespace

int S2MelModel::finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) {
  const int D = cfg.hidden_dim, C = cfg.in_channels, Wh = cfg.wn_hidden, depth = cfg.depth;
  IDX_CHECK(D == cfg.num_heads * 64, "head_dim must be 64");
  IDX_CHECK(Wh == D, "the reference's FinalLayer requires wavenet.hidden_dim == DiT.hidden_dim");
  IDX_CHECK((D & 31) == 0 && (Wh & 31) == 0 && (cfg.lr_channels & 31) == 0, "channel counts must be multiples of 32");
  {
    const int nh = (int)(2 * (4 * D) / 3);
    ffn = (nh % 256 == 0) ? nh : nh + 256 - (nh % 256);
  }
  const std::string e = "cfm.estimator";
  // every linear of this stage: a split-bf16 pack for every shape, the LDS-DMA kernel on its 16x16x32 loop (model_util.h)
  auto lin_from = [&](const std::string& key, int N, int K, bool bias, LinearWeights* out) { return linear_from(t, arena, key, N, K, bias, WP16_ALWAYS_MF16, out); };
  auto mk_lin = [&](const float* w, const float* bias, int N, int K, LinearWeights* out) { return make_linear(arena, w, bias, N, K, {WP16_ALWAYS_MF16}, out); };
  blocks.resize(depth);
  std::vector<float> mod_w, mod_b;
  auto append_mod = [&](const std::string& name) -> int {
    HostTensor *w = nullptr, *b = nullptr;
    if (need(t, name + ".project_layer.weight", {2 * D, D}, &w) || need(t, name + ".project_layer.bias", {2 * D}, &b)) return 1;
    mod_w.insert(mod_w.end(), w->data.begin(), w->data.end());
    mod_b.insert(mod_b.end(), b->data.begin(), b->data.end());
    return 0;
  };
  for (int i = 0; i < depth; ++i) {
    DiTBlock& B = blocks[i];
    const std::string p = e + ".transformer.layers." + std::to_string(i);
    if (lin_from(p + ".attention.wqkv", 3 * D, D, false, &B.wqkv)) return 1;
    if (lin_from(p + ".attention.wo", D, D, false, &B.wo)) return 1;
    HostTensor *w1 = nullptr, *w3 = nullptr;
    if (need(t, p + ".feed_forward.w1.weight", {ffn, D}, &w1) || need(t, p + ".feed_forward.w3.weight", {ffn, D}, &w3)) return 1;
    if (mk_lin(pair_pack(w1->data.data(), w3->data.data(), ffn, D).data(), nullptr, 2 * ffn, D, &B.w13)) return 1;
    if (lin_from(p + ".feed_forward.w2", D, ffn, false, &B.w2)) return 1;
    HostTensor *g = nullptr;
    if (need(t, p + ".attention_norm.norm.weight", {D}, &g) || up(arena, g->data, &B.attn_g)) return 1;
    if (need(t, p + ".ffn_norm.norm.weight", {D}, &g) || up(arena, g->data, &B.ffn_g)) return 1;
    if (append_mod(p + ".attention_norm") || append_mod(p + ".ffn_norm")) return 1;
    if (i > depth / 2) {
      HostTensor *sw = nullptr, *sb = nullptr;
      if (need(t, p + ".skip_in_linear.weight", {D, 2 * D}, &sw) || need(t, p + ".skip_in_linear.bias", {D}, &sb)) return 1;
      if (mk_lin(col_slice(sw->data, D, 2 * D, 0, D).data(), sb->data.data(), D, D, &B.skip_a)) return 1;
      if (mk_lin(col_slice(sw->data, D, 2 * D, D, 2 * D).data(), nullptr, D, D, &B.skip_b)) return 1;
    }
  }
  {
    HostTensor* g = nullptr;
    if (need(t, e + ".transformer.norm.norm.weight", {D}, &g) || up(arena, g->data, &final_g)) return 1;
    if (append_mod(e + ".transformer.norm")) return 1;
    if (mk_lin(mod_w.data(), mod_b.data(), (2 * depth + 1) * 2 * D, D, &mod_all)) return 1;
  }
  const int Win = 2 * C + D + cfg.style_dim;
  if (lin_from(e + ".cond_projection", D, cfg.content_dim, true, &cond_proj)) return 1;
  if (lin_from(e + ".cond_x_merge_linear", D, Win, true, &merge)) return 1;
  if (lin_from(e + ".t_embedder.mlp.0", D, 256, true, &temb0) || lin_from(e + ".t_embedder.mlp.2", D, D, true, &temb2)) return 1;
  if (lin_from(e + ".t_embedder2.mlp.0", Wh, 256, true, &t2emb0) || lin_from(e + ".t_embedder2.mlp.2", Wh, Wh, true, &t2emb2)) return 1;
  {
    HostTensor *sw = nullptr, *sb = nullptr;
    if (need(t, e + ".skip_linear.weight", {D, D + C}, &sw) || need(t, e + ".skip_linear.bias", {D}, &sb)) return 1;
    if (mk_lin(col_slice(sw->data, D, D + C, 0, D).data(), sb->data.data(), D, D, &skiplin_a)) return 1;
    if (mk_lin(col_slice(sw->data, D, D + C, D, D + C).data(), nullptr, D, C, &skiplin_b)) return 1;
  }
  if (lin_from(e + ".conv1", Wh, D, true, &conv1)) return 1;
  if (lin_from(e + ".res_projection", Wh, D, true, &res_proj)) return 1;
  if (lin_from(e + ".final_layer.linear", Wh, Wh, true, &final_lin)) return 1;
  if (lin_from(e + ".final_layer.adaLN_modulation.1", 2 * Wh, Wh, true, &final_mod)) return 1;
  {
    HostTensor *w = nullptr, *b = nullptr;
    if (need(t, e + ".conv2.weight", {C, Wh, 1}, &w) || need(t, e + ".conv2.bias", {C}, &b)) return 1;
    if (mk_lin(w->data.data(), b->data.data(), C, Wh, &conv2)) return 1;      // (N = 80: the split-bf16 tile kernels)
  }
  // ---- WaveNet ----
  const int L = cfg.wn_layers, k = cfg.wn_kernel;
  wn.resize(L);
  {
    HostTensor *cw = nullptr, *cb = nullptr;
    if (need(t, e + ".wavenet.cond_layer.conv.conv.weight", {2 * Wh * L, Wh, 1}, &cw) ||
        need(t, e + ".wavenet.cond_layer.conv.conv.bias", {2 * Wh * L}, &cb)) return 1;
    std::vector<float> cw_perm, cb_perm;
    for (int l = 0; l < L; ++l) {
      WNLayer& W = wn[l];
      const std::string p = e + ".wavenet.in_layers." + std::to_string(l) + ".conv.conv";
      HostTensor *iw = nullptr, *ib = nullptr;
      if (need(t, p + ".weight", {2 * Wh, Wh, k}, &iw) || need(t, p + ".bias", {2 * Wh}, &ib)) return 1;
      const std::vector<float> rows = conv_to_rows(iw->data, 2 * Wh, Wh, k);
      if (mk_lin(pair_pack(rows.data(), rows.data() + (size_t)Wh * k * Wh, Wh, k * Wh).data(), nullptr, 2 * Wh, k * Wh, &W.in_gate)) return 1;
      // cond_layer slice of this layer, same gate packing; its bias absorbs the in_layer bias
      const float* cwl = cw->data.data() + (size_t)l * 2 * Wh * Wh;
      const std::vector<float> cwp = pair_pack(cwl, cwl + (size_t)Wh * Wh, Wh, Wh);
      cw_perm.insert(cw_perm.end(), cwp.begin(), cwp.end());
      std::vector<float> bsum(2 * Wh);
      for (int c = 0; c < 2 * Wh; ++c) bsum[c] = cb->data[(size_t)l * 2 * Wh + c] + ib->data[c];
      const std::vector<float> bp = pair_pack(bsum.data(), bsum.data() + Wh, Wh, 1);
      cb_perm.insert(cb_perm.end(), bp.begin(), bp.end());
      const std::string r = e + ".wavenet.res_skip_layers." + std::to_string(l) + ".conv.conv";
      const int rc = l < L - 1 ? 2 * Wh : Wh;
      HostTensor *rw = nullptr, *rb = nullptr;
      if (need(t, r + ".weight", {rc, Wh, 1}, &rw) || need(t, r + ".bias", {rc}, &rb)) return 1;
      if (l < L - 1) {
        std::vector<float> w_res(rw->data.begin(), rw->data.begin() + (size_t)Wh * Wh), b_res(rb->data.begin(), rb->data.begin() + Wh);
        std::vector<float> w_skip(rw->data.begin() + (size_t)Wh * Wh, rw->data.end()), b_skip(rb->data.begin() + Wh, rb->data.end());
        if (mk_lin(w_res.data(), b_res.data(), Wh, Wh, &W.res) || mk_lin(w_skip.data(), b_skip.data(), Wh, Wh, &W.skip)) return 1;
      } else {
        W.has_res = false;
        if (mk_lin(rw->data.data(), rb->data.data(), Wh, Wh, &W.skip)) return 1;
      }
    }
    if (mk_lin(cw_perm.data(), cb_perm.data(), 2 * Wh * L, Wh, &wn_cond)) return 1;
  }
  // ---- length regulator, gpt_layer, codec table ----
  const int LC = cfg.lr_channels;
  if (lin_from("length_regulator.content_in_proj", LC, cfg.lr_in_channels, true, &lr_in)) return 1;
  lr_conv.resize(cfg.lr_num_convs);
  lr_gn_g.resize(cfg.lr_num_convs);
  lr_gn_b.resize(cfg.lr_num_convs);
  for (int n = 0; n < cfg.lr_num_convs; ++n) {
    HostTensor *w = nullptr, *b = nullptr, *g = nullptr, *bb = nullptr;
    const std::string p = "length_regulator.model." + std::to_string(3 * n);
    if (need(t, p + ".weight", {LC, LC, 3}, &w) || need(t, p + ".bias", {LC}, &b)) return 1;
    if (mk_lin(conv_to_rows(w->data, LC, LC, 3).data(), b->data.data(), LC, 3 * LC, &lr_conv[n])) return 1;
    const std::string q = "length_regulator.model." + std::to_string(3 * n + 1);
    if (need(t, q + ".weight", {LC}, &g) || need(t, q + ".bias", {LC}, &bb)) return 1;
    if (up(arena, g->data, &lr_gn_g[n]) || up(arena, bb->data, &lr_gn_b[n])) return 1;
  }
  {
    HostTensor *w = nullptr, *b = nullptr;
    const std::string p = "length_regulator.model." + std::to_string(3 * cfg.lr_num_convs);
    if (need(t, p + ".weight", {LC, LC, 1}, &w) || need(t, p + ".bias", {LC}, &b)) return 1;
    if (mk_lin(w->data.data(), b->data.data(), LC, LC, &lr_out)) return 1;
  }
  {
    const int dims[4] = {cfg.gpt_dim, cfg.gpt_layer_dims[0], cfg.gpt_layer_dims[1], cfg.gpt_layer_dims[2]};
    for (int n = 0; n < 3; ++n)
      if (lin_from("gpt_layer." + std::to_string(n), dims[n + 1], dims[n], true, &gl[n])) return 1;
    IDX_CHECK(dims[3] == cfg.codec_hidden && cfg.codec_hidden == cfg.lr_in_channels, "gpt_layer / codec / length-regulator widths");
  }
  {
    // vq2emb table: out_project(codebook[v]) for every v (factorized_vector_quantize.py:123-127)
    HostTensor *cb = nullptr, *ow = nullptr, *ob = nullptr;
    const std::string q = "semantic_codec.quantizer.quantizers.0";
    if (need(t, q + ".codebook.weight", {cfg.codebook_size, cfg.codebook_dim}, &cb) ||
        need(t, q + ".out_project.weight", {cfg.codec_hidden, cfg.codebook_dim, 1}, &ow) ||
        need(t, q + ".out_project.bias", {cfg.codec_hidden}, &ob)) return 1;
    std::vector<float> table((size_t)cfg.codebook_size * cfg.codec_hidden);
    for (int v = 0; v < cfg.codebook_size; ++v)
      for (int h = 0; h < cfg.codec_hidden; ++h) {
        float acc = 0.0f;
        for (int c = 0; c < cfg.codebook_dim; ++c) acc = std::fmaf(cb->data[(size_t)v * cfg.codebook_dim + c], ow->data[(size_t)h * cfg.codebook_dim + c], acc);
        table[(size_t)v * cfg.codec_hidden + h] = acc + ob->data[h];
      }
    if (up(arena, table, &vq_table)) return 1;
  }
  {
    auto it = t.find("rope_cache");
    if (it == t.end()) IDX_FAIL("missing tensor 'rope_cache' ([T][32][2] cos/sin table, precompute_freqs_cis)");
    IDX_CHECK(it->second.shape.size() == 3 && it->second.shape[1] == 32 && it->second.shape[2] == 2, "rope_cache must be [T][32][2]");
    rope_len = (int)it->second.shape[0];
    if (up(arena, it->second.data, &rope)) return 1;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
size_t S2MelModel::cfm_workspace_bytes(int B, int T, int n_steps) const { return carve_cfm(cfg, ffn, nullptr, B, T, n_steps).bytes; }

// An operand of a launch: fp32 rows, split-bf16 planes of them (GemmArgs::x_planes / y_planes), or -- an output -- both.
// A launch given planes to read does not read the rows; one given only planes to write writes no fp32 output.
struct Src { const float* f; const void* p; Src(const float* rows, const void* planes = nullptr) : f(planes ? nullptr : rows), p(planes) {} };
struct Dst { float* f; void* p; Dst(float* rows, void* planes = nullptr) : f(rows), p(planes) {} };

static GemmArgs gemm_args(Src x, int ldx, Dst y, int ldy, int M, int act = ACT_NONE, const float* res = nullptr, int ldr = 0) {
  GemmArgs a;
  a.x = x.f; a.x_planes = x.p; a.ldx = ldx; a.y = y.f; a.y_planes = y.p; a.ldy = ldy; a.M = M; a.act = act; a.res = res; a.ldr = ldr;
  return a;
}
static int gemm(const LinearWeights& w, Src x, int ldx, Dst y, int ldy, int M, hipStream_t st, int act = ACT_NONE,
                const float* res = nullptr, int ldr = 0) {
  return gemm_forward(w, gemm_args(x, ldx, y, ldy, M, act, res, ldr), st);
}

// The rows a part of one evaluation runs on, and how its operands travel from launch to launch.  An evaluation has at most two
// row sets: ALL frames (nseq * T rows) and the TAIL, the frames t >= tail_t0 of every sequence compacted to nseq * (T - tail_t0)
// rows (tail_t0 == 0: the tail IS the set of all frames).
// Producer -> GEMM chaining: when the consumers run on the LDS-DMA split-bf16 kernel, hn / att / ff / wn_acts are written by
// their producers directly as bf16 hi/lo planes (same bytes as the fp32 row) and never exist in fp32; the operands that are also
// read as rows (h, the skips, xres, wn_x) get planes beside their rows.  A call site takes its operands from the accessors and
// never looks at the flags: planes of one row set handed to a launch on the other are wrong data with no error.
struct RowSet {
  const CfmBuffers* w = nullptr;
  int nseq = 0, seq = 0, rows = 0;      // rows = nseq * seq
  const int* lens = nullptr;            // [nseq] valid frames
  bool planes = false;                  // hn / att / ff / wn_acts / skips / h travel as planes
  bool planes_wn = false;               // and so do the long skip's and the WaveNet's operands (xres, wn_x)

  Src hn_in() const { return in(w->hn, w->hn_p, planes); }                  Dst hn_out() const { return instead(w->hn, w->hn_p, planes); }
  Src att_in() const { return in(w->att, w->att_p, planes); }               Dst att_out() const { return instead(w->att, w->att_p, planes); }
  Src ff_in() const { return in(w->ff, w->ff_p, planes); }                  Dst ff_out() const { return instead(w->ff, w->ff_p, planes); }
  Src acts_in() const { return in(w->wn_acts, w->acts_p, planes); }         Dst acts_out() const { return instead(w->wn_acts, w->acts_p, planes); }
  Src skip_in(int i) const { return in(w->skips[i], w->skips_p[i], planes); }   Dst skip_out(int i) const { return beside(w->skips[i], w->skips_p[i], planes); }
  Src xres_in() const { return in(w->xres, w->xres_p, planes_wn); }         Dst xres_out() const { return beside(w->xres, w->xres_p, planes_wn); }
  Src wnx_in() const { return in(w->wn_x, w->wnx_p, planes_wn); }           Dst wnx_out() const { return beside(w->wn_x, w->wnx_p, planes_wn); }
  // the residual stream (in ha or hb): its planes exist only where a skip-receive layer reads it next (reread)
  Src h_in(const float* h) const { return in(h, w->h_p, planes); }          Dst h_out(float* h, bool reread) const { return beside(h, w->h_p, planes && reread); }

 private:
  static Src in(const float* f, const void* p, bool on) { return on ? Src(f, p) : Src(f); }
  static Dst instead(float* f, void* p, bool on) { return on ? Dst(nullptr, p) : Dst(f); }      // planes INSTEAD of the rows
  static Dst beside(float* f, void* p, bool on) { return on ? Dst(f, p) : Dst(f); }             // planes BESIDE the rows
};

// The only place that asks gemm_uses_planes (and with it the 256-row rule) on behalf of the hand-offs: a row set is on planes when
// EVERY GEMM that reads or writes a chained operand on its rows runs on the LDS-DMA kernel.  within: the set of all frames when
// this one is its tail -- a tail is on planes only if all frames are (the last block hands planes from one to the other), and the
// K/V projection never runs on a tail.
static RowSet row_set(const S2MelModel& m, const CfmBuffers& w, int nseq, int seq, const int* lens, const RowSet* within) {
  RowSet r;
  r.w = &w; r.nseq = nseq; r.seq = seq; r.rows = nseq * seq; r.lens = lens;
  const DiTBlock& b0 = m.blocks[0];
  const WNLayer& wn0 = m.wn[0];
  GemmArgs pr;
  pr.M = r.rows;
  r.planes = within ? within->planes : gemm_uses_planes(b0.wqkv, pr);
  for (const LinearWeights* lw : {&b0.wo, &b0.w13, &b0.w2, &m.skiplin_a, &m.final_lin, &wn0.skip}) r.planes = r.planes && gemm_uses_planes(*lw, pr);
  r.planes_wn = r.planes && (!within || within->planes_wn);
  for (const LinearWeights* lw : {&m.skiplin_b, &m.conv1, &m.res_proj, &wn0.res}) r.planes_wn = r.planes_wn && gemm_uses_planes(*lw, pr);
  pr.taps = m.cfg.wn_kernel; pr.seq_len = seq;
  r.planes_wn = r.planes_wn && gemm_uses_planes(wn0.in_gate, pr);
  return r;
}

// The t-only constants of ONE estimator evaluation: the 2 * depth + 1 adaLN (weight, bias) pairs, the FinalLayer (shift, scale) and the
// WaveNet conditioning biases of all layers.  ld == 0: one step's vectors, shared by every sequence (the solver of one schedule);
// ld > 0: one row per sequence, [nseq][ld] tables (per-row schedules: cfm_sched gathers each live row's own step).
struct StepConsts { const float* mods; int ld_mods; const float* fmod; int ld_fmod; const float* wnb; int ld_wnb; };

// adaLN-RMSNorm of x into the set's hn; mod: the (weight, bias) pair of this norm and step, ld_mod apart from sequence to sequence
static int ada_norm(const S2MelModel& m, const float* x, const float* g, const float* mod, int ld_mod, const RowSet& r, hipStream_t st) {
  const int D = m.cfg.hidden_dim;
  const Dst hn = r.hn_out();
  RowsNormArgs n;
  n.x_in = x; n.ld_in = D; n.y = hn.f; n.y_planes = hn.p; n.ld_y = D; n.M = r.rows; n.d = D;
  n.mode = NORM_ADA_RMS; n.eps = m.cfg.norm_eps; n.g1 = g;
  n.mod_a = mod; n.mod_b = mod + D; n.ld_mod = ld_mod; n.rows_per_batch = ld_mod ? r.seq : 0;
  return rows_norm_forward(n, st);
}

// Attention of the queries [q0, q0 + Sq) of every sequence over the keys / values of all its frames.  w.qkv: the projection of
// all frames as fp32 rows, or (qkv_planes) as the split-bf16 planes the planes kernel reads.
static int attention(const S2MelModel& m, const RowSet& all, bool qkv_planes, int q0, int Sq, Dst o, hipStream_t st) {
  const int D = m.cfg.hidden_dim, T = all.seq;
  const float* qkv = all.w->qkv;
  if (qkv_planes) {
    AttnPlanesArgs ap;
    ap.planes = qkv; ap.Mrows = all.rows; ap.ncols = 3 * D; ap.q_col = 0; ap.k_col = D; ap.v_col = 2 * D; ap.T = T; ap.q_row0 = q0; ap.Sq = Sq;
    ap.B = all.nseq; ap.H = m.cfg.num_heads; ap.kend = all.lens; ap.scale = 0.125f;
    ap.o = o.f; ap.o_planes = o.p; ap.o_bs = (long)Sq * D; ap.o_ts = D;
    ap.split_bf16 = acoustic_bf16_active() ? 2 : 1;
    return flash_attn_planes_forward(ap, st);
  }
  AttnArgs a;
  a.q = qkv + (size_t)q0 * 3 * D; a.k = qkv + D; a.v = qkv + 2 * D; a.o = o.f; a.o_planes = o.p;
  a.q_bs = a.k_bs = a.v_bs = (long)T * 3 * D; a.o_bs = (long)Sq * D; a.q_ts = a.k_ts = a.v_ts = 3 * D; a.o_ts = D;
  a.B = all.nseq; a.H = m.cfg.num_heads; a.Sq = Sq; a.Sk = T; a.causal = 0; a.kend = all.lens; a.scale = 0.125f;
  a.split_bf16 = get_gemm_mode() == GEMM_BF16X3 ? (acoustic_bf16_active() ? 2 : 1) : 0;
  return flash_attn_forward(a, st);
}

// One DiT block: h (on the rows of `all`) -> out.  Norm and K/V projection run on all frames; everything behind them -- queries,
// attention output, wo, norm, w13, w2 -- on `post`: all frames again, or, in the last block of a compacted tail, whose keys and
// values cover every frame but whose output nothing attends to, the tail rows alone.  res: h on post's rows: h itself, or the
// buffer the block gathers h's tail rows into.  lag_event (optional) is recorded behind the attention.
static int dit_block(S2MelModel& m, int i, const float* mods, int ld_mods, const float* h, const RowSet& all, const RowSet& post, float* res, Dst out,
                     hipEvent_t lag_event, hipStream_t st) {
  const auto& c = m.cfg;
  const CfmBuffers& w = *all.w;
  const DiTBlock& B = m.blocks[i];
  const int D = c.hidden_dim, T = all.seq, q0 = T - post.seq;
  if (ada_norm(m, h, B.attn_g, mods + (size_t)(2 * i) * 2 * D, ld_mods, all, st)) return 1;
  bool qkv_planes = false;
  {     // qkv projection; the rotary embedding of q and k rides in its epilogue when the LDS-DMA kernel runs it
    GemmArgs g = gemm_args(all.hn_in(), D, w.qkv, 3 * D, all.rows);
    const bool fuse_rope = gemm_uses_planes(B.wqkv, g);
    // LDS-DMA GEMM: rotary embedding in its epilogue, and q / k / v leave it as split-bf16 planes (the same bytes as the fp32
    // rows they replace) for the planes attention kernel
    qkv_planes = fuse_rope && D == 64 * c.num_heads;
    if (fuse_rope) { g.rope = m.rope; g.rope_T = T; g.rope_cols = 2 * D; }
    if (qkv_planes) { g.y = nullptr; g.y_planes = w.qkv; }
    if (gemm_forward(B.wqkv, g, st)) return 1;
    if (!fuse_rope && rotary_qk(w.qkv, all.rows, c.num_heads, T, m.rope, st)) return 1;
  }
  if (attention(m, all, qkv_planes, q0, post.seq, post.att_out(), st)) return 1;
  if (lag_event) IDX_HIP(hipEventRecord(lag_event, st));
  if (res != h && gather_tail_rows(res, D, h, D, D, all.nseq, T, q0, st)) return 1;
  if (gemm(B.wo, post.att_in(), D, w.hmid, D, post.rows, st, ACT_NONE, res, D)) return 1;           // h + attention(...)
  if (ada_norm(m, w.hmid, B.ffn_g, mods + (size_t)(2 * i + 1) * 2 * D, ld_mods, post, st)) return 1;
  if (gemm(B.w13, post.hn_in(), D, post.ff_out(), m.ffn, post.rows, st, ACT_SWIGLU)) return 1;
  return gemm(B.w2, post.ff_in(), m.ffn, out, D, post.rows, st, ACT_NONE, w.hmid, D);               // out = h + ffn
}

// N2 sequences of T frames (one CFG half, or the stacked batch); lag_event (optional) is recorded behind the first attention
static int dit_eval(S2MelModel& m, CfmBuffers& w, int N2, int T, const StepConsts& sc, hipStream_t st, hipEvent_t lag_event) {
  const auto& c = m.cfg;
  const int D = c.hidden_dim, C = c.in_channels, Wh = c.wn_hidden, depth = c.depth, half = depth / 2;
  const int Win = 2 * C + D + c.style_dim;
  const float* mods = sc.mods;
  // The solver needs the estimate only on the frames t >= tail_t0 (see below): the post-transformer part and, in the LAST block,
  // everything after the K/V projection run on those frames alone, compacted to [N2][T - tail_t0] rows.
  const int t0 = w.tail_t0;
  const RowSet all = row_set(m, w, N2, T, w.lens2, nullptr);
  const RowSet tail = t0 > 0 ? row_set(m, w, N2, T - t0, w.lens2t, &all) : all;
  if (lag_event && depth < 2) IDX_HIP(hipEventRecord(lag_event, st));      // (a one-block model has no "behind the first attention")
  if (gemm(m.merge, w.x_in, Win, w.ha, D, all.rows, st)) return 1;
  float* h = w.ha;
  int pushed = 0;
  for (int i = 0; i < depth; ++i) {
    if (i > half) {     // U-ViT receive: skip_in_linear(cat[x, skip]) as two GEMMs (model.py:233-234)
      DiTBlock& B = m.blocks[i];
      --pushed;
      if (gemm(B.skip_a, all.h_in(h), D, w.hmid, D, all.rows, st)) return 1;
      float* dst = (h == w.ha) ? w.hb : w.ha;
      if (gemm(B.skip_b, all.skip_in(pushed), D, dst, D, all.rows, st, ACT_NONE, w.hmid, D)) return 1;
      h = dst;
    }
    // the first half's outputs are the skip tensors; a block's output is read again as a GEMM operand when it is a skip tensor
    // (skip_b later) or enters a skip-receive layer (skip_a)
    const Dst out = i < half ? all.skip_out(pushed) : all.h_out((h == w.ha) ? w.hb : w.ha, i + 1 < depth && i + 1 > half);
    // the last block of a compacted tail gathers its residual rows into xres (free here) and leaves h on the tail rows; it is
    // never a skip push (depth - 1 >= depth / 2), so with t0 > 0 h always leaves the loop compacted
    const bool cut = i == depth - 1 && t0 > 0;
    if (dit_block(m, i, mods, sc.ld_mods, h, all, cut ? tail : all, cut ? w.xres : h, out, i == 0 && !cut ? lag_event : nullptr, st)) return 1;
    if (i < half) ++pushed;
    h = out.f;
  }
  // ---- everything after the transformer is row-local or a short convolution (WaveNet: k = 5, 8 layers -> 16 frames of context),
  // and the Euler step discards the estimate on the prompt frames (x[..., :prompt_len] = 0, flow_matching.py:113): in the solver
  // only the frames t >= tail_t0 = prompt_len - halo are evaluated -- the prompt is 44 % of the frames at configs[2] -- on rows
  // compacted to [N2][T - tail_t0].  The frames t >= prompt_len come out bit-identical: the reflect padding at the cut only reaches
  // the halo.  tail_t0 = 0 (the stand-alone estimator entry point): every frame.
  const int Mt = tail.rows, Tt = tail.seq;
  const float* xin_t = w.x_in;
  int ld_xin = Win;
  if (t0 > 0) {
    if (gather_tail_rows(w.qkv, C, w.x_in, Win, C, N2, T, t0, st)) return 1;      // the x columns of x_in (qkv is free here)
    xin_t = w.qkv; ld_xin = C;
  }
  if (ada_norm(m, h, m.final_g, mods + (size_t)(2 * depth) * 2 * D, sc.ld_mods, tail, st)) return 1;
  // long skip: skip_linear(cat[x_res, x]) (diffusion_transformer.py:243-244); x rows live in x_in[:, :C]
  if (gemm(m.skiplin_a, tail.hn_in(), D, w.hmid, D, Mt, st)) return 1;
  if (gemm(m.skiplin_b, xin_t, ld_xin, tail.xres_out(), D, Mt, st, ACT_NONE, w.hmid, D)) return 1;
  if (gemm(m.conv1, tail.xres_in(), D, tail.wnx_out(), Wh, Mt, st)) return 1;
  // WaveNet (wavenet.py:138-166)
  const int L = c.wn_layers, k = c.wn_kernel;
  for (int l = 0; l < L; ++l) {
    WNLayer& W = m.wn[l];
    int dil = 1;
    for (int q = 0; q < l; ++q) dil *= c.wn_dilation_rate;
    LinearWeights in = W.in_gate;
    in.bias = sc.wnb + (size_t)l * 2 * Wh;     // in_layer bias + g_l of this step (of every sequence's own step), gate-packed
    GemmArgs g = gemm_args(tail.wnx_in(), Wh, tail.acts_out(), Wh, Mt, ACT_GATE);
    g.ld_bias = sc.ld_wnb;
    g.taps = k; g.seq_len = Tt; g.dil = dil; g.pad_left = (k - 1) / 2 * dil; g.pad_mode = 1; g.row_len = tail.lens;
    if (gemm_forward(in, g, st)) return 1;
    if (W.has_res) {   // x = (x + res) * mask
      GemmArgs r = gemm_args(tail.acts_in(), Wh, tail.wnx_out(), Wh, Mt, ACT_NONE, w.wn_x, Wh);
      r.seq_len = Tt; r.row_len = tail.lens;
      if (gemm_forward(W.res, r, st)) return 1;
    }
    GemmArgs sk = gemm_args(tail.acts_in(), Wh, w.wn_out, Wh, Mt);     // output += skip ; the last layer's epilogue applies "* x_mask" to the finished sum
    if (l > 0) { sk.res = w.wn_out; sk.ldr = Wh; }
    if (l == L - 1) { sk.seq_len = Tt; sk.row_len = tail.lens; }
    if (gemm_forward(W.skip, sk, st)) return 1;
  }
  if (gemm(m.res_proj, tail.xres_in(), D, w.hmid, Wh, Mt, st, ACT_NONE, w.wn_out, Wh)) return 1;
  {
    const Dst hn = tail.hn_out();
    RowsNormArgs n;     // FinalLayer (diffusion_transformer.py:96-101)
    n.x_in = w.hmid; n.ld_in = Wh; n.y = hn.f; n.y_planes = hn.p; n.ld_y = Wh; n.M = Mt; n.d = Wh; n.mode = NORM_MOD_LN; n.eps = 1e-6f;
    n.mod_a = sc.fmod; n.mod_b = n.mod_a + Wh; n.ld_mod = sc.ld_fmod; n.rows_per_batch = sc.ld_fmod ? Tt : 0;
    if (rows_norm_forward(n, st)) return 1;
  }
  if (gemm(m.final_lin, tail.hn_in(), Wh, w.att, Wh, Mt, st)) return 1;
  return gemm(m.conv2, w.att, Wh, w.vout, C, Mt, st);
}

// ---- the two CFG halves on two streams -------------------------------------------------------------------
// Every kernel of the estimator alternates an MFMA-bound phase with an HBM-bound one (a GEMM tile: 57 k cycles of main loop, then
// 22-39 k cycles in which all 256 CUs write their tiles at once at ~4.6 TB/s; in-kernel stamps, profiles/README.md "Round 3"), and
// all workgroups of one launch are in the same phase.  Two launches of DIFFERENT kernels side by side are not: with the null
// half of the batch a couple of kernels behind the conditional half, one half's epilogues drain while the other half multiplies
// (tools/two_stream_gemm.py: the four GEMMs of a DiT layer 1290 -> 1098 us).  The halves share nothing between cfm_pack and the
// Euler update.  Each half is a dit_eval of its own with N2 = B, so its row sets (row_set) are taken at B*T and B*Tt rows instead of 2B*T
// and 2B*Tt: results are bit-identical to the single-stream order (same kernels on the same rows) when both pairs are on the
// same side of the 256-row switch (and always in GEMM_F32 mode); otherwise a half runs the fp32-row kernels where the stacked
// batch runs planes, within the split-bf16 bounds (tests/test_s2mel_dispatch_gpu.py::test_solver_halves_on_two_streams).
struct HalfStreams { hipStream_t side = nullptr; hipEvent_t fork = nullptr, lag = nullptr, join = nullptr; };
static std::map<std::pair<int, hipStream_t>, HalfStreams> g_half_streams;   // per (device, caller stream)
static std::mutex g_half_mu;
// Off by default: alone on the device the solver takes 9 % less time with it (542 -> 491 ms at configs[2]), a sequential
// synthesize_batch 3 % less -- but in the serving pipeline the decode chains of the NEXT batches then run at less than half their
// speed (two of three lanes 2.65 s instead of 1.18 s per 512 tokens, also when decode and acoustic stages take strict turns; not
// understood: profiles/README.md "Round 3"), so the batch pipeline leaves it off.
static int g_s2mel_overlap = 0;
void set_s2mel_overlap(int on) { g_s2mel_overlap = on ? 1 : 0; }
int get_s2mel_overlap() { return g_s2mel_overlap; }

static int half_streams_for(hipStream_t st, HalfStreams* out) {
  int dev = 0;
  IDX_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_half_mu);
  HalfStreams& hs = g_half_streams[std::make_pair(dev, st)];
  if (!hs.side) {
    // same priority as the caller's stream: the halves are peers (a side stream of HIGHER priority than its caller starves the
    // caller's half -- measured: the solver took twice as long on a low-priority serving stream)
    int prio = 0;
    if (st) IDX_HIP(hipStreamGetPriority(st, &prio));
    IDX_HIP(hipStreamCreateWithPriority(&hs.side, hipStreamNonBlocking, prio));
    IDX_HIP(hipEventCreateWithFlags(&hs.fork, hipEventDisableTiming));
    IDX_HIP(hipEventCreateWithFlags(&hs.lag, hipEventDisableTiming));
    IDX_HIP(hipEventCreateWithFlags(&hs.join, hipEventDisableTiming));
  }
  *out = hs;
  return 0;
}

int s2mel_release_stream(hipStream_t st) {      // idxtts_release_stream: the side stream + events kept for a caller stream
  int dev = 0;
  IDX_HIP(hipGetDevice(&dev));
  HalfStreams hs;
  {
    std::lock_guard<std::mutex> lk(g_half_mu);
    auto it = g_half_streams.find(std::make_pair(dev, st));
    if (it == g_half_streams.end()) return 0;
    hs = it->second;
    g_half_streams.erase(it);
  }
  if (hs.side) { (void)hipStreamSynchronize(hs.side); (void)hipStreamDestroy(hs.side); }
  if (hs.fork) (void)hipEventDestroy(hs.fork);
  if (hs.lag) (void)hipEventDestroy(hs.lag);
  if (hs.join) (void)hipEventDestroy(hs.join);
  return 0;
}

// true: the two halves run as two chains on two streams (half_view buffers); false: ONE stacked evaluation of 2B sequences on the
// caller's stream (larger launches: 394 instead of 2 x 198 tiles for an N = 512 GEMM fill the second round of CUs better)
static bool halves_on_two_streams(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  return g_s2mel_overlap && !prof_enabled() && cap == hipStreamCaptureStatusNone;     // (per-launch event timing wants kernels alone)
}

// the constants of step `step` of the call's one schedule, shared by all sequences
static StepConsts shared_step(const S2MelModel& m, const CfmBuffers& w, int step) {
  const auto& c = m.cfg;
  return {w.mods + (size_t)step * (2 * c.depth + 1) * 2 * c.hidden_dim, 0, w.fmod + (size_t)step * 2 * c.wn_hidden, 0,
          w.wnb + (size_t)step * c.wn_layers * 2 * c.wn_hidden, 0};
}

// The two CFG halves as two evaluations of their own, N0 conditional and N1 null sequences (N1 may be 0: no row asks for guidance) in
// the half views v0 / v1: on two streams (two_streams), or one behind the other on the caller's.
static int dit_eval_two(S2MelModel& m, CfmBuffers& v0, int N0, const StepConsts& c0, CfmBuffers& v1, int N1, const StepConsts& c1, int T,
                        bool two_streams, hipStream_t st) {
  if (!two_streams || N1 == 0) {
    if (dit_eval(m, v0, N0, T, c0, st, nullptr)) return 1;
    return N1 ? dit_eval(m, v1, N1, T, c1, st, nullptr) : 0;
  }
  HalfStreams hs;
  if (half_streams_for(st, &hs)) return 1;
  IDX_HIP(hipEventRecord(hs.fork, st));
  IDX_HIP(hipStreamWaitEvent(hs.side, hs.fork, 0));
  // the null half starts when the conditional half has finished its first attention (a few kernels in): from then on the two
  // chains stay that far apart
  if (dit_eval(m, v0, N0, T, c0, st, hs.lag)) return 1;
  IDX_HIP(hipStreamWaitEvent(hs.side, hs.lag, 0));
  if (dit_eval(m, v1, N1, T, c1, hs.side, nullptr)) return 1;
  IDX_HIP(hipEventRecord(hs.join, hs.side));
  IDX_HIP(hipStreamWaitEvent(st, hs.join, 0));
  return 0;
}

// one estimator evaluation of the solver: both CFG halves, on two streams (two_streams) or stacked
static int dit_eval_halves(S2MelModel& m, CfmBuffers& w, int B, int T, int step, bool two_streams, hipStream_t st) {
  const StepConsts sc = shared_step(m, w, step);
  if (!two_streams) return dit_eval(m, w, 2 * B, T, sc, st, nullptr);
  CfmBuffers v0 = half_view(m.cfg, m.ffn, w, 0, B, T);
  CfmBuffers v1 = half_view(m.cfg, m.ffn, w, 1, B, T);
  return dit_eval_two(m, v0, B, sc, v1, B, sc, T, true, st);
}

int S2MelModel::cfm(const float* mu, const int* x_lens_host, const float* prompt, const int* prompt_lens_host, int Tp_max,
                    const float* style, const float* z, const float* t_emb, const float* dt_host, int n_steps, float cfg_rate,
                    float* out, int B, int T, void* ws, size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(mu && x_lens_host && prompt && prompt_lens_host && style && z && t_emb && dt_host && out, "null pointer");
  IDX_CHECK(B > 0 && T > 0 && n_steps > 0 && Tp_max > 0, "shape");
  IDX_CHECK(cfg_rate > 0.0f, "the stacked-CFG path needs inference_cfg_rate > 0 (reference default 0.7)");
  IDX_CHECK(T <= rope_len, "sequence longer than the rope cache");
  IDX_CHECK(ws && ws_bytes >= cfm_workspace_bytes(B, T, n_steps), "workspace too small");
  CfmBuffers w = carve_cfm(cfg, ffn, ws, B, T, n_steps);
  if (cfm_solve(w, mu, x_lens_host, prompt, prompt_lens_host, Tp_max, style, z, t_emb, dt_host, n_steps, cfg_rate, B, T, st)) return 1;
  IDX_HIP(hipMemcpyAsync(out, w.xstate, (size_t)B * cfg.in_channels * T * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- the per-call set-up the solver and the stand-alone estimator share -----------------------------------
// Lengths, checked and on the device when it returns: lens2 (both halves) and plen.  solver: a prompt lies inside its own row, and
// the tail cut is taken from the shortest prompt (w.tail_t0, lens2t = lens2 - tail_t0); the stand-alone estimator (prompt within T)
// evaluates every frame.
static int upload_lens(const S2MelModel& m, CfmBuffers& w, const int* x_lens_host, const int* prompt_lens_host, int Tp_max, int B, int T,
                       bool solver, hipStream_t st) {
  const auto& c = m.cfg;
  std::vector<int> lens2(2 * B), plen(B), lens2t(2 * B);
  for (int b = 0; b < B; ++b) {
    const int pmax = std::min(Tp_max, solver ? x_lens_host[b] : T);
    IDX_CHECK(x_lens_host[b] > 0 && x_lens_host[b] <= T && prompt_lens_host[b] >= 0 && prompt_lens_host[b] <= pmax, "lengths");
    lens2[b] = lens2[B + b] = x_lens_host[b];
    plen[b] = prompt_lens_host[b];
  }
  IDX_HIP(hipMemcpyAsync(w.lens2, lens2.data(), 2 * B * sizeof(int), hipMemcpyHostToDevice, st));
  if (solver) {
    // the post-transformer part runs on the frames from tail_t0 on: the shortest prompt minus the WaveNet's one-sided context
    int halo = 0, dil = 1, pmin = plen[0];
    for (int l = 0; l < c.wn_layers; ++l) { halo += (c.wn_kernel - 1) / 2 * dil; dil *= c.wn_dilation_rate; }
    for (int b = 0; b < B; ++b) pmin = std::min(pmin, plen[b]);
    w.tail_t0 = pmin - halo >= 64 ? pmin - halo : 0;
    for (int i = 0; i < 2 * B; ++i) lens2t[i] = lens2[i] - w.tail_t0;
    IDX_HIP(hipMemcpyAsync(w.lens2t, lens2t.data(), 2 * B * sizeof(int), hipMemcpyHostToDevice, st));
  }
  IDX_HIP(hipMemcpyAsync(w.plen, plen.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  return 0;
}

// per-call constants: every t-dependent vector for all steps at once (M = n_steps GEMMs)
static int step_constants(const S2MelModel& m, const CfmBuffers& w, const float* t_emb, int n_steps, hipStream_t st) {
  const int D = m.cfg.hidden_dim, Wh = m.cfg.wn_hidden;
  if (gemm(m.temb0, t_emb, 256, w.tmp_steps, D, n_steps, st, ACT_SILU) || gemm(m.temb2, w.tmp_steps, D, w.t1, D, n_steps, st)) return 1;
  if (gemm(m.mod_all, w.t1, D, w.mods, (2 * m.cfg.depth + 1) * 2 * D, n_steps, st)) return 1;
  if (silu_rows(w.t1s, w.t1, (size_t)n_steps * D, st) || gemm(m.final_mod, w.t1s, Wh, w.fmod, 2 * Wh, n_steps, st)) return 1;
  if (gemm(m.t2emb0, t_emb, 256, w.tmp_steps, Wh, n_steps, st, ACT_SILU) || gemm(m.t2emb2, w.tmp_steps, Wh, w.t2, Wh, n_steps, st)) return 1;
  return gemm(m.wn_cond, w.t2, Wh, w.wnb, m.cfg.wn_layers * 2 * Wh, n_steps, st);
}

// the stacked [cond | null] input rows from the state w.xstate (x_only: see CfmPackArgs)
static CfmPackArgs pack_args(const S2MelModel& m, const CfmBuffers& w, const float* prompt, const float* style, int B, int T, int Tp_max) {
  const auto& c = m.cfg;
  CfmPackArgs pk;
  pk.x_in = w.x_in; pk.ld = 2 * c.in_channels + c.hidden_dim + c.style_dim; pk.x = w.xstate; pk.prompt = prompt; pk.prompt_len = w.plen;
  pk.cond = w.condp; pk.cond_null = m.cond_proj.bias; pk.style = style;
  pk.B = B; pk.T = T; pk.C = c.in_channels; pk.D = c.hidden_dim; pk.S = c.style_dim; pk.Tp_max = Tp_max;
  return pk;
}

// The Euler solve shared by cfm and cfm_rows: leaves the final state x [B][C][T] in w.xstate.
int S2MelModel::cfm_solve(CfmBuffers& w, const float* mu, const int* x_lens_host, const float* prompt, const int* prompt_lens_host,
                          int Tp_max, const float* style, const float* z, const float* t_emb, const float* dt_host, int n_steps,
                          float cfg_rate, int B, int T, hipStream_t st) {
  const int D = cfg.hidden_dim, C = cfg.in_channels;
  if (upload_lens(*this, w, x_lens_host, prompt_lens_host, Tp_max, B, T, true, st)) return 1;
  if (step_constants(*this, w, t_emb, n_steps, st)) return 1;
  if (gemm(cond_proj, mu, cfg.content_dim, w.condp, D, B * T, st)) return 1;
  if (cfm_init_state(w.xstate, z, w.plen, B, C, T, st)) return 1;       // x[..., :prompt_len] = 0 (flow_matching.py:82)
  const bool two_streams = halves_on_two_streams(st);
  for (int s = 0; s < n_steps; ++s) {
    CfmPackArgs pk = pack_args(*this, w, prompt, style, B, T, Tp_max);
    pk.x_only = s > 0;      // x_in is read by the merge GEMM and the long skip only: its other 784 columns are packed once
    if (cfm_pack(pk, st)) return 1;
    if (dit_eval_halves(*this, w, B, T, s, two_streams, st)) return 1;
    CfmEulerArgs eu;      // (two streams: the null half's estimate lives in half_view's second block)
    eu.x = w.xstate; eu.v = w.vout; eu.v_null = two_streams ? w.vout + (size_t)B * T * C : nullptr; eu.ldv = C; eu.prompt_len = w.plen; eu.B = B; eu.T = T; eu.C = C; eu.dt = dt_host[s]; eu.cfg_rate = cfg_rate;
    eu.v_t0 = w.tail_t0; eu.v_T = T - w.tail_t0;
    if (cfm_euler(eu, st)) return 1;
  }
  return 0;
}

// ---- mixed-prompt batches: every row with its own speaker's prompt_condition / ref_mel (flow_matching.py:31-115, infer_v2.py:850-856) ----
// The extra workspace behind the solver's: the packed mu rows [B][T][content_dim], the packed prompt mel [B][C][Tp_max], the
// device copies of the two pointer tables and of the generated lengths.
struct CfmRowsBuffers { float *mu, *prompt; const float **pcond, **ref_mel; int* gen_len; size_t bytes; };

static CfmRowsBuffers carve_cfm_rows(const S2MelModel& m, void* ws, size_t base, int B, int T, int Tp_max) {
  const auto& c = m.cfg;
  CfmRowsBuffers b;
  Carver k(ws ? static_cast<char*>(ws) + base : nullptr);
  b.mu = k.take<float>((size_t)B * T * c.content_dim);
  b.prompt = k.take<float>((size_t)B * c.in_channels * Tp_max);
  b.pcond = k.take<const float*>(B);
  b.ref_mel = k.take<const float*>(B);
  b.gen_len = k.take<int>(B);
  b.bytes = base + ((k.off + 255) & ~(size_t)255);
  return b;
}

size_t S2MelModel::cfm_rows_workspace_bytes(int B, int T, int Tp_max, int n_steps) const {
  return carve_cfm_rows(*this, nullptr, cfm_workspace_bytes(B, T, n_steps), B, T, Tp_max).bytes;
}

int S2MelModel::cfm_rows(const float* gen_cond, const int* target_lens_host, int Tg_max, const float* const* prompt_cond_host,
                         const float* const* ref_mel_host, const int* prompt_lens_host, const float* style, const float* z,
                         const float* t_emb, const float* dt_host, int n_steps, float cfg_rate, float* out, int B, int T, void* ws,
                         size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(gen_cond && target_lens_host && prompt_cond_host && ref_mel_host && prompt_lens_host && style && z && t_emb && dt_host && out,
            "null pointer");
  IDX_CHECK(B > 0 && T > 0 && Tg_max > 0 && n_steps > 0, "shape");
  IDX_CHECK(cfg_rate > 0.0f, "the stacked-CFG path needs inference_cfg_rate > 0 (reference default 0.7)");
  IDX_CHECK(T <= rope_len, "sequence longer than the rope cache");
  IDX_CHECK(cfg.content_dim % 4 == 0 && ((uintptr_t)gen_cond & 15) == 0, "gen_cond must be 16-byte aligned (content_dim % 4 == 0)");
  std::vector<int> xl(B), tg(B);
  int Tp_max = 0, T_need = 0;
  for (int b = 0; b < B; ++b) {
    const int Tp = prompt_lens_host[b], Tg = target_lens_host[b];
    IDX_CHECK(Tp > 0 && Tg > 0 && Tg <= Tg_max, "prompt_lens / target_lens out of range");
    IDX_CHECK(prompt_cond_host[b] && ref_mel_host[b], "null prompt table entry");
    IDX_CHECK(((uintptr_t)prompt_cond_host[b] & 15) == 0, "prompt_condition rows must be 16-byte aligned");
    xl[b] = Tp + Tg;
    tg[b] = Tg;
    Tp_max = std::max(Tp_max, Tp);
    T_need = std::max(T_need, Tp + Tg);
  }
  IDX_CHECK(T == T_need, "T must be max_b(prompt_lens[b] + target_lens[b])");
  IDX_CHECK(ws && ws_bytes >= cfm_rows_workspace_bytes(B, T, Tp_max, n_steps), "workspace too small");
  CfmBuffers w = carve_cfm(cfg, ffn, ws, B, T, n_steps);
  CfmRowsBuffers r = carve_cfm_rows(*this, ws, w.bytes, B, T, Tp_max);
  IDX_HIP(hipMemcpyAsync(r.pcond, prompt_cond_host, B * sizeof(float*), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(r.ref_mel, ref_mel_host, B * sizeof(float*), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(r.gen_len, tg.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.plen, prompt_lens_host, B * sizeof(int), hipMemcpyHostToDevice, st));    // (cfm_solve writes it again)
  CfmRowsPackArgs pk;
  pk.mu = r.mu; pk.prompt = r.prompt; pk.pcond = r.pcond; pk.ref_mel = r.ref_mel; pk.gen = gen_cond; pk.prompt_len = w.plen;
  pk.gen_len = r.gen_len; pk.B = B; pk.T = T; pk.Dc = cfg.content_dim; pk.C = cfg.in_channels; pk.Tp_max = Tp_max; pk.Tg_max = Tg_max;
  if (cfm_rows_pack(pk, st)) return 1;
  // (the host tables above are consumed before cfm_solve returns: it synchronises the stream after its own uploads)
  if (cfm_solve(w, r.mu, xl.data(), r.prompt, prompt_lens_host, Tp_max, style, z, t_emb, dt_host, n_steps, cfg_rate, B, T, st)) return 1;
  return cfm_rows_emit(out, w.xstate, w.plen, r.gen_len, B, cfg.in_channels, T, Tg_max, st);
}

// ---- per-row schedules: every row with its own Euler steps and guidance rate (idxtts_s2mel_cfm_sched) ----------------------------
// The rows are kept in an order of the solver's own: by descending step count (stable), so that the rows still live at iteration s
// are the first n_live(s) slots, and the rows of the null half -- those with a rate > 0, in the same order -- the first n_null(s) of
// their list.  An iteration is cfm_solve's: pack, estimator, Euler update; each half is an evaluation of its own on its live rows
// (dit_eval_two), with the step constants of each row's own schedule gathered into [rows][cols] tables.  THIS routine is the one
// place that builds the row maps; the kernels that read them are cfm_rows_pack (gen_row), cfm_init_state_rows, cfm_pack_half,
// cfm_gather_consts, cfm_euler_rows and cfm_rows_emit_map.
size_t S2MelModel::cfm_sched_workspace_bytes(int B, int T, int Tp_max, int n_sched, const int* sched_steps) const {
  if (B <= 0 || T <= 0 || Tp_max <= 0 || n_sched < 1 || !sched_steps) return 0;
  long total = 0;
  int smax = 0;
  for (int d = 0; d < n_sched; ++d) {
    if (sched_steps[d] < 1) return 0;
    total += sched_steps[d];
    smax = std::max(smax, sched_steps[d]);
  }
  if (total > (1 << 20)) return 0;
  return carve_cfm_sched(cfg, nullptr, cfm_rows_workspace_bytes(B, T, Tp_max, (int)total), B, smax).bytes;
}

int S2MelModel::cfm_sched(const float* gen_cond, const int* target_lens_host, int Tg_max, const float* const* prompt_cond_host,
                          const float* const* ref_mel_host, const int* prompt_lens_host, const float* style, const float* z, int n_sched,
                          const int* sched_steps, const float* t_emb, const float* dt_host, const int* row_sched, const float* cfg_rates,
                          float* out, int B, int T, void* ws, size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(gen_cond && target_lens_host && prompt_cond_host && ref_mel_host && prompt_lens_host && style && z && sched_steps && t_emb &&
            dt_host && row_sched && cfg_rates && out, "null pointer");
  IDX_CHECK(B > 0 && T > 0 && Tg_max > 0, "shape");
  IDX_CHECK(n_sched >= 1, "n_sched must be at least 1");
  std::vector<int> first(n_sched);      // first row of schedule d in the concatenated tables
  int total = 0, smax = 0;
  for (int d = 0; d < n_sched; ++d) {
    IDX_CHECK(sched_steps[d] >= 1 && sched_steps[d] <= (1 << 20) - total, "a schedule needs at least 1 step");
    first[d] = total;
    total += sched_steps[d];
    smax = std::max(smax, sched_steps[d]);
  }
  for (int b = 0; b < B; ++b) {
    IDX_CHECK(row_sched[b] >= 0 && row_sched[b] < n_sched, "row_sched entry out of range");
    IDX_CHECK(std::isfinite(cfg_rates[b]) && cfg_rates[b] >= 0.0f, "cfg_rates must be finite and >= 0 (negative rates are refused)");
  }
  IDX_CHECK(T <= rope_len, "sequence longer than the rope cache");
  IDX_CHECK(cfg.content_dim % 4 == 0 && ((uintptr_t)gen_cond & 15) == 0, "gen_cond must be 16-byte aligned (content_dim % 4 == 0)");
  // slot i = the caller's row order[i]: descending steps, stable
  std::vector<int> order(B);
  for (int b = 0; b < B; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sched_steps[row_sched[a]] > sched_steps[row_sched[b]]; });
  std::vector<int> xl(B), tg(B), pl(B), steps(B);
  std::vector<const float*> pcond(B), refmel(B);
  int Tp_max = 0, T_need = 0, pmin = 0;
  for (int i = 0; i < B; ++i) {
    const int b = order[i], Tp = prompt_lens_host[b], Tg = target_lens_host[b];
    IDX_CHECK(Tp > 0 && Tg > 0 && Tg <= Tg_max, "prompt_lens / target_lens out of range");
    IDX_CHECK(prompt_cond_host[b] && ref_mel_host[b], "null prompt table entry");
    IDX_CHECK(((uintptr_t)prompt_cond_host[b] & 15) == 0, "prompt_condition rows must be 16-byte aligned");
    xl[i] = Tp + Tg; tg[i] = Tg; pl[i] = Tp; steps[i] = sched_steps[row_sched[b]];
    pcond[i] = prompt_cond_host[b]; refmel[i] = ref_mel_host[b];
    Tp_max = std::max(Tp_max, Tp);
    T_need = std::max(T_need, Tp + Tg);
    pmin = i ? std::min(pmin, Tp) : Tp;
  }
  IDX_CHECK(T == T_need, "T must be max_b(prompt_lens[b] + target_lens[b])");
  IDX_CHECK(ws && ws_bytes >= cfm_sched_workspace_bytes(B, T, Tp_max, n_sched, sched_steps), "workspace too small");
  CfmBuffers w = carve_cfm(cfg, ffn, ws, B, T, total);
  CfmRowsBuffers r = carve_cfm_rows(*this, ws, w.bytes, B, T, Tp_max);
  CfmSchedBuffers sb = carve_cfm_sched(cfg, ws, r.bytes, B, smax);
  // ---- the row maps and per-slot tables (host), uploaded once ----
  std::vector<int> null_slot(B, 0), null_row(B, -1), src0((size_t)smax * B, 0), src1((size_t)smax * B, 0), live0(smax, 0), live1(smax, 0);
  std::vector<float> dts((size_t)smax * B, 0.0f), rates(B);
  int n_null = 0;
  for (int i = 0; i < B; ++i) {
    rates[i] = cfg_rates[order[i]];
    if (rates[i] > 0.0f) { null_row[i] = n_null; null_slot[n_null++] = i; }
    const int f = first[row_sched[order[i]]];
    for (int s = 0; s < steps[i]; ++s) {
      ++live0[s];
      src0[(size_t)s * B + i] = f + s;
      dts[(size_t)s * B + i] = dt_host[f + s];
      if (null_row[i] >= 0) { ++live1[s]; src1[(size_t)s * B + null_row[i]] = f + s; }
    }
  }
  {     // tail cut: the shortest prompt of the whole batch minus the WaveNet's one-sided context (upload_lens)
    int halo = 0, dil = 1;
    for (int l = 0; l < cfg.wn_layers; ++l) { halo += (cfg.wn_kernel - 1) / 2 * dil; dil *= cfg.wn_dilation_rate; }
    w.tail_t0 = pmin - halo >= 64 ? pmin - halo : 0;
  }
  std::vector<int> lens2(2 * B), lens2t(2 * B);      // [conditional rows = slots | null rows (the unused tail repeats slot 0)]
  for (int i = 0; i < B; ++i) { lens2[i] = xl[i]; lens2[B + i] = xl[i < n_null ? null_slot[i] : 0]; }
  for (int i = 0; i < 2 * B; ++i) lens2t[i] = lens2[i] - w.tail_t0;
  auto upload = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
  IDX_HIP(upload(w.lens2, lens2.data(), 2 * B * sizeof(int)));
  IDX_HIP(upload(w.lens2t, lens2t.data(), 2 * B * sizeof(int)));
  IDX_HIP(upload(w.plen, pl.data(), B * sizeof(int)));
  IDX_HIP(upload(r.pcond, pcond.data(), B * sizeof(float*)));
  IDX_HIP(upload(r.ref_mel, refmel.data(), B * sizeof(float*)));
  IDX_HIP(upload(r.gen_len, tg.data(), B * sizeof(int)));
  IDX_HIP(upload(sb.order, order.data(), B * sizeof(int)));
  IDX_HIP(upload(sb.null_slot, null_slot.data(), B * sizeof(int)));
  IDX_HIP(upload(sb.null_row, null_row.data(), B * sizeof(int)));
  IDX_HIP(upload(sb.src_row[0], src0.data(), src0.size() * sizeof(int)));
  IDX_HIP(upload(sb.src_row[1], src1.data(), src1.size() * sizeof(int)));
  IDX_HIP(upload(sb.dt, dts.data(), dts.size() * sizeof(float)));
  IDX_HIP(upload(sb.cfg_rate, rates.data(), B * sizeof(float)));
  IDX_HIP(hipStreamSynchronize(st));      // (the host tables above may go)
  // ---- per-call set-up: cfm_rows' and cfm_solve's, one set of step constants per schedule ----
  const int D = cfg.hidden_dim, C = cfg.in_channels, Wh = cfg.wn_hidden;
  CfmRowsPackArgs rp;
  rp.mu = r.mu; rp.prompt = r.prompt; rp.pcond = r.pcond; rp.ref_mel = r.ref_mel; rp.gen = gen_cond; rp.prompt_len = w.plen;
  rp.gen_len = r.gen_len; rp.B = B; rp.T = T; rp.Dc = cfg.content_dim; rp.C = C; rp.Tp_max = Tp_max; rp.Tg_max = Tg_max; rp.gen_row = sb.order;
  if (cfm_rows_pack(rp, st)) return 1;
  for (int d = 0; d < n_sched; ++d)
    if (step_constants(*this, steps_view(cfg, ffn, w, first[d]), t_emb + (size_t)first[d] * 256, sched_steps[d], st)) return 1;
  if (gemm(cond_proj, r.mu, cfg.content_dim, w.condp, D, B * T, st)) return 1;
  if (cfm_init_state_rows(w.xstate, z, w.plen, sb.order, B, C, T, st)) return 1;
  const bool two_streams = halves_on_two_streams(st);
  CfmBuffers v[2] = {half_view(cfg, ffn, w, 0, B, T), half_view(cfg, ffn, w, 1, B, T)};
  const int cols[3] = {(2 * cfg.depth + 1) * 2 * D, 2 * Wh, cfg.wn_layers * 2 * Wh};
  StepConsts sc[2];
  for (int h = 0; h < 2; ++h) sc[h] = {sb.mods[h], cols[0], sb.fmod[h], cols[1], sb.wnb[h], cols[2]};
  for (int s = 0; s < smax; ++s) {
    const int live[2] = {live0[s], live1[s]};
    for (int h = 0; h < 2; ++h) {
      if (!live[h]) continue;
      CfmPackArgs pk = pack_args(*this, v[h], r.prompt, style, B, T, Tp_max);
      pk.x_only = s > 0;      // (a half's live rows are a prefix of its rows at s = 0: the other columns stand)
      if (cfm_pack_half(pk, h == 0, live[h], h ? sb.null_slot : nullptr, sb.order, st)) return 1;
      CfmGatherConstsArgs ga;
      ga.dst[0] = sb.mods[h]; ga.dst[1] = sb.fmod[h]; ga.dst[2] = sb.wnb[h];
      ga.src[0] = w.mods; ga.src[1] = w.fmod; ga.src[2] = w.wnb;
      for (int k = 0; k < 3; ++k) ga.cols[k] = cols[k];
      ga.src_row = sb.src_row[h] + (size_t)s * B; ga.N = live[h];
      if (cfm_gather_consts(ga, st)) return 1;
    }
    if (dit_eval_two(*this, v[0], live[0], sc[0], v[1], live[1], sc[1], T, two_streams, st)) return 1;
    CfmEulerRowsArgs eu;
    eu.x = w.xstate; eu.v = v[0].vout; eu.v_null = v[1].vout; eu.ldv = C; eu.prompt_len = w.plen; eu.dt = sb.dt + (size_t)s * B;
    eu.cfg_rate = sb.cfg_rate; eu.null_row = sb.null_row; eu.N = live[0]; eu.T = T; eu.C = C; eu.v_t0 = w.tail_t0; eu.v_T = T - w.tail_t0;
    if (cfm_euler_rows(eu, st)) return 1;
  }
  return cfm_rows_emit_map(out, w.xstate, w.plen, r.gen_len, sb.order, B, C, T, Tg_max, st);
}

// One evaluation of the CFM estimator = DiT.forward(x, prompt_x, x_lens, t, style, cond) (diffusion_transformer.py:186-257)
// on B rows: the conditional half of the stacked [cond | null] evaluation the Euler loop runs every step.
int S2MelModel::estimator(const float* x, const float* prompt, const int* prompt_lens_host, int Tp_max, const int* x_lens_host,
                          const float* t_emb, const float* style, const float* mu, float* out_tm, int B, int T, void* ws, size_t ws_bytes,
                          hipStream_t st) {
  IDX_CHECK(x && prompt && prompt_lens_host && x_lens_host && t_emb && style && mu && out_tm, "null pointer");
  IDX_CHECK(B > 0 && T > 0 && Tp_max > 0 && T <= rope_len, "shape");
  IDX_CHECK(ws && ws_bytes >= cfm_workspace_bytes(B, T, 1), "workspace too small");
  const int C = cfg.in_channels;
  CfmBuffers w = carve_cfm(cfg, ffn, ws, B, T, 1);
  if (upload_lens(*this, w, x_lens_host, prompt_lens_host, Tp_max, B, T, false, st)) return 1;
  if (step_constants(*this, w, t_emb, 1, st)) return 1;
  if (gemm(cond_proj, mu, cfg.content_dim, w.condp, cfg.hidden_dim, B * T, st)) return 1;
  IDX_HIP(hipMemcpyAsync(w.xstate, x, (size_t)B * C * T * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (cfm_pack(pack_args(*this, w, prompt, style, B, T, Tp_max), st)) return 1;
  {
    CfmBuffers v0 = half_view(cfg, ffn, w, 0, B, T);      // the conditional half alone
    if (dit_eval(*this, v0, B, T, shared_step(*this, w, 0), st, nullptr)) return 1;
  }
  IDX_HIP(hipMemcpyAsync(out_tm, w.vout, (size_t)B * T * C * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------

static CondBuffers carve_cond(const S2MelModel& m, void* ws, int B, int M, int Tg) {
  const auto& c = m.cfg;
  CondBuffers b;
  Carver k(ws);
  const size_t rows = (size_t)B * std::max(M, Tg);
  const int wide = std::max(std::max(c.codec_hidden, c.lr_channels), std::max(c.gpt_layer_dims[0], c.gpt_layer_dims[1]));
  b.a = k.take<float>(rows * wide);
  b.b = k.take<float>(rows * wide);
  b.s = k.take<float>(rows * wide);
  b.stats = k.take<float>(2 * B);
  b.idx_code = k.take<int>((size_t)B * M);
  b.idx_row = k.take<int>((size_t)B * M);
  b.idx_interp = k.take<int>((size_t)B * Tg);
  b.tlen = k.take<int>(B);
  b.bytes = (k.off + 255) & ~(size_t)255;
  return b;
}

size_t S2MelModel::cond_workspace_bytes(int B, int M, int Tg) const { return carve_cond(*this, nullptr, B, M, Tg).bytes; }

// torch's 'nearest' source row for the tb target frames of one sequence of mb rows that start at row0:
// F.interpolate(mode='nearest'): src = min(floor(dst * (float)in / out), in - 1), float32 arithmetic
static void nearest_rows(int* idx, int row0, int mb, int tb) {
  const float scale = (float)mb / (float)tb;
  for (int j = 0; j < tb; ++j) idx[j] = row0 + std::min((int)std::floor((float)j * scale), mb - 1);
}

int S2MelModel::prepare_cond(const float* latent, const long long* codes, const int* code_lens_host, const int* target_lens_host,
                             int B, int M, int Tg, float* cond_out, void* ws, size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(latent && codes && code_lens_host && target_lens_host && cond_out, "null pointer");
  IDX_CHECK(B > 0 && M > 0 && Tg > 0, "shape");
  IDX_CHECK(ws && ws_bytes >= cond_workspace_bytes(B, M, Tg), "workspace too small");
  const int Hc = cfg.codec_hidden;
  CondBuffers w = carve_cond(*this, ws, B, M, Tg);
  // host-side index tables: code ids, and torch's 'nearest' source row for every target frame
  std::vector<long long> hc((size_t)B * M);
  IDX_HIP(hipMemcpyAsync(hc.data(), codes, hc.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
  IDX_HIP(hipStreamSynchronize(st));
  std::vector<int> ic((size_t)B * M), ir((size_t)B * M), ii((size_t)B * Tg, -1), tl(B);
  for (int b = 0; b < B; ++b) {
    const int mb = code_lens_host[b], tb = target_lens_host[b];
    IDX_CHECK(mb > 0 && mb <= M && tb > 0 && tb <= Tg, "code_lens / target_lens out of range");
    tl[b] = tb;
    for (int i = 0; i < M; ++i) {
      const long long cde = hc[(size_t)b * M + i];
      IDX_CHECK(i >= mb || (cde >= 0 && cde < cfg.codebook_size), "semantic code out of the codebook");
      ic[(size_t)b * M + i] = i < mb ? (int)cde : -1;
      ir[(size_t)b * M + i] = i < mb ? b * M + i : -1;
    }
    nearest_rows(&ii[(size_t)b * Tg], b * M, mb, tb);
  }
  IDX_HIP(hipMemcpyAsync(w.idx_code, ic.data(), ic.size() * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.idx_row, ir.data(), ir.size() * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.idx_interp, ii.data(), ii.size() * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.tlen, tl.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  const int rowsM = B * M;
  // gpt_layer: 1280 -> 256 -> 128 -> 1024 (commons.py:413)
  if (gemm(gl[0], latent, cfg.gpt_dim, w.a, gl[0].N, rowsM, st) || gemm(gl[1], w.a, gl[0].N, w.b, gl[1].N, rowsM, st) ||
      gemm(gl[2], w.b, gl[1].N, w.a, Hc, rowsM, st)) return 1;
  // S_infer = vq2emb(codes) + latent (infer_v2.py:841-843)
  GatherArgs ga;
  ga.out = w.s; ga.ld_out = Hc; ga.d = Hc;
  ga.table[0] = vq_table; ga.idx[0] = w.idx_code;
  ga.table[1] = w.a; ga.idx[1] = w.idx_row;
  if (gather_sum_rows(ga, rowsM, st)) return 1;
  return regulate_rows(w.s, w, B, M, Tg, cond_out, st);
}

// InterpolateRegulator.forward on token-major rows s [B*M][lr_in_channels] (length_regulator.py:117-141): content_in_proj, nearest
// interpolation M_b -> Tg_b through the host-built index table w.idx_interp, 4 x (Conv1d k3 -> GroupNorm(1) -> Mish), Conv1d 1x1, mask
int S2MelModel::regulate_rows(const float* s_rows, const CondBuffers& w, int B, int M, int Tg, float* cond_out, hipStream_t st) {
  const int Hc = cfg.codec_hidden, LC = cfg.lr_channels;
  const int rowsM = B * M, rowsT = B * Tg;
  // content_in_proj, nearest interpolation M_b -> Tg_b (rows beyond Tg_b are zero)
  if (gemm(lr_in, s_rows, Hc, w.a, LC, rowsM, st)) return 1;
  GatherArgs gi;
  gi.out = w.b; gi.ld_out = LC; gi.d = LC; gi.table[0] = w.a; gi.idx[0] = w.idx_interp;
  if (gather_sum_rows(gi, rowsT, st)) return 1;
  float* cur = w.b;
  float* other = w.a;
  for (int n = 0; n < cfg.lr_num_convs; ++n) {
    GemmArgs g;
    g.x = cur; g.ldx = LC; g.y = other; g.ldy = LC; g.M = rowsT; g.taps = 3; g.seq_len = Tg; g.dil = 1; g.pad_left = 1; g.pad_mode = 0;
    if (gemm_forward(lr_conv[n], g, st)) return 1;
    if (groupnorm1_mish(cur, other, lr_gn_g[n], lr_gn_b[n], w.tlen, B, Tg, LC, 1e-5f, w.stats, st)) return 1;
  }
  GemmArgs o;
  o.x = cur; o.ldx = LC; o.y = cond_out; o.ldy = LC; o.M = rowsT; o.seq_len = Tg; o.row_len = w.tlen;    // * mask
  return gemm_forward(lr_out, o, st);
}

// length_regulator(S, ylens) alone = the prompt-side call of infer_v2.py:649-652 (S_ref -> prompt_condition)
int S2MelModel::regulate(const float* S, const int* in_lens_host, const int* target_lens_host, int B, int M, int Tg, float* cond_out,
                         void* ws, size_t ws_bytes, hipStream_t st) {
  IDX_CHECK(S && in_lens_host && target_lens_host && cond_out, "null pointer");
  IDX_CHECK(B > 0 && M > 0 && Tg > 0, "shape");
  IDX_CHECK(ws && ws_bytes >= cond_workspace_bytes(B, M, Tg), "workspace too small");
  CondBuffers w = carve_cond(*this, ws, B, M, Tg);
  std::vector<int> ii((size_t)B * Tg, -1), tl(B);
  for (int b = 0; b < B; ++b) {
    const int mb = in_lens_host[b], tb = target_lens_host[b];
    IDX_CHECK(mb > 0 && mb <= M && tb > 0 && tb <= Tg, "in_lens / target_lens out of range");
    tl[b] = tb;
    nearest_rows(&ii[(size_t)b * Tg], b * M, mb, tb);
  }
  IDX_HIP(hipMemcpyAsync(w.idx_interp, ii.data(), ii.size() * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipMemcpyAsync(w.tlen, tl.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  IDX_HIP(hipStreamSynchronize(st));
  return regulate_rows(S, w, B, M, Tg, cond_out, st);
}

}  // namespace idxtts
