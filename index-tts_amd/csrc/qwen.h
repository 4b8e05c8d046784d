// Qwen3 causal LM, B = 1 greedy generation: the emotion-from-text classifier of the reference (QwenEmotion, infer_v2.py:948-1063).
// RMSNorm, per-head q/k RMSNorm, rotary positions, grouped-query attention at head_dim 128, SwiGLU MLP, (tied) vocabulary head.
// fp32 arithmetic; linear weights stored fp32 or bf16 (exact for a bf16 checkpoint).  Kernels and host code: qwen.hip.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/idxtts.h"
#include "ctx.h"
#include "gemm.h"
#include "prof.h"

namespace idxtts {

enum QwenWeightFormat { QWEN_W_F32 = 0, QWEN_W_BF16 = 1 };

// step scalars of the generation in flight, device-resident: a captured decode step replays on them
struct QwenState {
  int pos;        // position of the token whose embedding is in xd (= keys in the cache before its step)
  int step;       // generated tokens so far
  int done;       // an end id has been fed (or the cap reached): later launches change nothing
  int argmax;     // the head's choice of the step in flight
  int n_out;      // valid entries of out_ids
  int pad[3];
};

struct QwenStream {      // a weight matrix [N][K] row-major in the decode format
  const void* w = nullptr;
  int N = 0, K = 0;
};

struct QwenLayer {
  const float *in_g = nullptr, *post_g = nullptr, *qn_g = nullptr, *kn_g = nullptr;
  LinearWeights qkv_l, o_l, gu_l, down_l;      // MFMA-packed fp32 (prefill)
  QwenStream qkv_s, o_s, gate_s, up_s, down_s; // decode streams
};

struct QwenModel : ModelBase {
  idxtts_qwen_config cfg;
  int fmt = QWEN_W_F32;
  std::vector<QwenLayer> layers;
  const float* norm_g = nullptr;
  QwenStream embed_s, head_s;      // head_s == embed_s when tied
  const float* rope = nullptr;     // [max_context][head_dim / 2][2] = (cos, sin)
  int qdim() const { return cfg.num_attention_heads * cfg.head_dim; }
  int kvdim() const { return cfg.num_key_value_heads * cfg.head_dim; }
  int qkvdim() const { return qdim() + 2 * kvdim(); }

  struct Buffers {
    float *x, *x2, *xn, *qkv, *att, *gu, *hmid;      // prefill activations, P rows
    float *kc, *vc; int Smax;                        // [L][Hkv][Smax][128] each
    float *xd, *qkvd, *attd, *hd, *logits;           // decode vectors
    float* head_val; int* head_idx; unsigned* head_cnt; int head_blocks;
    float* attn_part; unsigned* attn_cnt; int nsplit;
    QwenState* st;
    int *prompt, *eos, *forced, *cols, *out_ids;
    size_t bytes;
  };
  // one kept decode-step graph: nothing call-specific but these is baked into its launches
  struct GraphKey {
    void* ws = nullptr; size_t ws_bytes = 0; int P = 0, max_new = 0, n_eos = 0, n_cols = 0; bool forced = false, all_cols = false;
    float* out_logits = nullptr;
    bool operator==(const GraphKey& o) const {
      return ws == o.ws && ws_bytes == o.ws_bytes && P == o.P && max_new == o.max_new && n_eos == o.n_eos && n_cols == o.n_cols &&
             forced == o.forced && all_cols == o.all_cols && out_logits == o.out_logits;
    }
  };
  GraphKey graph_key;
  hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
  int graph_kernel_nodes = -1;
  hipStream_t own_stream = nullptr;

  explicit QwenModel(const idxtts_qwen_config& c) : cfg(c) {}
  ~QwenModel() override;
  void drop_graph();
  bool accepts(const std::string& name) const override;
  int finalize(std::map<std::string, HostTensor>& t, DeviceArena& arena) override;
  Buffers carve(void* ws, int P, int max_new, int n_eos, int n_cols) const;
  size_t workspace_bytes(int P, int max_new, int n_eos, int n_cols) const { return carve(nullptr, P, max_new, n_eos, n_cols).bytes; }
  int prefill(const Buffers& w, int P, hipStream_t st);
  // the step's tail: final norm + head + argmax, the logits hand-over, then record / next embedding / advance
  int head_tail(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st);
  int decode_step(const Buffers& w, int max_new, int n_eos, bool forced, float* out_logits, int n_cols, bool all_cols, hipStream_t st);
  int generate(const int* prompt_ids, int n_prompt, int max_new, const int* eos_ids, int n_eos, const int* forced_ids, int* out_ids,
               int* n_out, float* out_logits, const int* logit_cols, int n_logit_cols, void* ws, size_t ws_bytes, int use_graph,
               hipStream_t st);
};

}  // namespace idxtts
