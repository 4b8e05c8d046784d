/* libidxtts_hip -- C ABI of the MI355X-native IndexTTS-2 hot path (gfx950 only).
 *
 * Drop-in boundary.  Every entry point takes plain device pointers, explicit
 * shapes and a hipStream_t (passed as void*), returns 0 on success / non-zero on error (message via
 * idxtts_last_error(), thread-local) and never throws.  No ownership transfer: the caller's allocator
 * (torch) owns inputs, outputs and workspaces; the library owns only an opaque idxtts_ctx holding the
 * kernel-layout (packed) weights.  One ctx per (process, device); calls on one ctx are serialised by
 * the caller (same rule as the reference object, infer_v2.py:304-310 / serve_tars.py:139-140).
 * All tensors are float32, contiguous, unless a parameter says otherwise.
 *
 * Reference interfaces replaced (file:line relative to grantjr1842/index-tts):
 *   idxtts_aa_act_fwd      <- pybind `anti_alias_activation_cuda.forward(input, up_ftr, down_ftr, alpha, beta)`
 *                             indextts/s2mel/modules/bigvgan/alias_free_activation/cuda/anti_alias_activation.cpp:19-23,
 *                             `extern "C" fwd_cuda` anti_alias_activation_cuda.cu:212-246, used by
 *                             `FusedAntiAliasActivation.forward` activation1d.py:21-26
 *   idxtts_bigvgan_*       <- `BigVGAN.forward` indextts/s2mel/modules/bigvgan/bigvgan.py:360-386 as called at
 *                             indextts/infer_v2.py:860 (`self.bigvgan(vc_target.float())`)
 *   idxtts_conv1d_*        <- torch.nn.Conv1d / ConvTranspose1d call sites on the hot path
 *                             (bigvgan.py:136-139, 362, 367; wavenet.py:149, 161; length_regulator.py:51, 61)
 */
#ifndef IDXTTS_H
#define IDXTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct idxtts_ctx idxtts_ctx;

#define IDXTTS_DTYPE_F32 0
#define IDXTTS_DTYPE_F16 1
#define IDXTTS_DTYPE_BF16 2

int idxtts_version(void);
/* Last error message of the calling thread ("" if none). */
const char* idxtts_last_error(void);

/* ---- fused anti-aliased SnakeBeta activation (reference: fwd_cuda, .cu:212-246) -------------------
 * out/in: [B][C][T] of element type `dtype` (IDXTTS_DTYPE_F32 / F16 / BF16: the dispatch of .cu:232-244; 16-bit inputs are
 * widened on load, the arithmetic is float32 throughout, the result is rounded once on store); up_filter/down_filter: 12 float32
 * taps; log_alpha/log_beta: float32 [C] (log-scale, exp'd in-kernel, .cu:86-89).  T == 0 is a no-op (.cu:193).  out must not alias in. */
int idxtts_aa_act_fwd(void* out, const void* in, const float* up_filter, const float* down_filter,
                      const float* log_alpha, const float* log_beta, int B, int C, int T, int dtype,
                      void* stream);

/* ---- stand-alone Conv1d on the fp32 matrix core (used by the tests and by s2mel) -------------------
 * weight: torch layout [Cout][Cin][K] (or [Cin][Cout][Kt] when transposed_stride > 1), host or device.
 * The returned handle owns the packed copy; free with idxtts_conv1d_destroy. */
typedef struct idxtts_conv1d idxtts_conv1d;
int idxtts_conv1d_create(const float* weight, const float* bias /* may be NULL */, int Cout, int Cin, int K,
                         int transposed_stride /* 1 = Conv1d, u>1 = ConvTranspose1d(k=2u, stride u, pad u/2) */,
                         idxtts_conv1d** out);
/* y[b][co][t] = scale*(bias + sum x[..t + k*dil - pad_left..] + residual) (+ y if accumulate).
 * pad_mode: 0 zero, 1 reflect.  x: [B][Cin][T]; y/residual: [B][Cout][T*transposed_stride].
 * Follows idxtts_set_gemm_mode (split-bf16 for layers that carry the bf16 pack) and, in that mode, idxtts_set_acoustic_bf16 (one
 * bf16 MFMA per product on w and x rounded to nearest-even bf16; bias, residual, scale and the fp32 output unchanged). */
int idxtts_conv1d_fwd(const idxtts_conv1d* conv, const float* x, float* y, const float* residual /* may be NULL */,
                      int B, int T, int dilation, int pad_left, int pad_mode, float scale, int accumulate,
                      void* stream);
int idxtts_conv1d_destroy(idxtts_conv1d* conv);

/* ---- generic weight hand-over for model contexts -------------------------------------------------
 * `name` is the reference module's state_dict key (e.g. "resblocks.3.convs1.0.weight"); data may be a
 * host or a device pointer (copied during the call).  Unknown keys are rejected; buffers the kernels
 * derive themselves ("*.filter") are accepted and cross-checked. */
int idxtts_ctx_load_tensor(idxtts_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim);
/* Pack everything loaded so far into kernel layouts on the current device; fails if a tensor is missing. */
int idxtts_ctx_finalize(idxtts_ctx* ctx);
/* Read a staged tensor back (host fp32, `capacity` floats) before finalize: after idxtts_gpt_quantize_weights this is the
 * exact model every kernel will run, under the reference's own keys (what a parity check feeds the reference / oracle). */
int idxtts_ctx_get_tensor(idxtts_ctx* ctx, const char* name, float* host_out, size_t capacity);
int idxtts_ctx_destroy(idxtts_ctx* ctx);
/* OCP fp8 e4m3fn value of a code / nearest-even saturating code of a value (host helpers of the fp8 weight format). */
float idxtts_fp8_e4m3_decode(unsigned char code);
unsigned char idxtts_fp8_e4m3_encode(float v);
/* Instrument: the quantiser of the scaled-fp8 KV cache (IDXTTS_KV_FP8 below) on n_vectors device vectors x [n_vectors][64] ->
 * codes [n_vectors][64], scales [n_vectors] (device pointers).  The very device routine the cache's producers call; it plays for the
 * cache the role idxtts_fp8_e4m3_encode plays for the weights. */
int idxtts_kv_fp8_quantize(const float* x, int n_vectors, unsigned char* codes, float* scales, void* stream);

/* ---- BigVGAN-v2 vocoder (reference: BigVGAN.forward, bigvgan.py:360-386) ------------------------- */
typedef struct idxtts_bigvgan_config {
  int num_mels;                   /* 80 */
  int upsample_initial_channel;   /* 1536 */
  int num_upsamples;              /* 6 */
  int upsample_rates[8];          /* 4,4,2,2,2,2 */
  int upsample_kernel_sizes[8];   /* 8,8,4,4,4,4 */
  int num_kernels;                /* 3 */
  int resblock_kernel_sizes[4];   /* 3,7,11 */
  int resblock_dilations[4][3];   /* 1,3,5 each */
} idxtts_bigvgan_config;

int idxtts_bigvgan_create(const idxtts_bigvgan_config* cfg, idxtts_ctx** out);
/* Bytes of scratch idxtts_bigvgan_fwd needs for a [B][num_mels][Tm] input. */
size_t idxtts_bigvgan_workspace_bytes(const idxtts_ctx* ctx, int B, int Tm);
/* mel: [B][num_mels][Tm] -> wav: [B][1][Tm*prod(upsample_rates)], clamped to [-1,1] (bigvgan.py:384).
 * If stage_out != NULL the activation tensor after up-sampling stage `stage_idx` (1-based, after the
 * resblock average, [B][C_i][T_i]) is also copied there (parity tests).  If clamp == 0 the final clamp
 * is skipped (tests compare the pre-clamp waveform so saturation cannot hide an error). */
int idxtts_bigvgan_fwd(idxtts_ctx* ctx, const float* mel, float* wav, int B, int Tm, void* workspace,
                       size_t workspace_bytes, int clamp, int stage_idx, float* stage_out, void* stream);
/* Ragged batch: mel_lengths = device int32 [B], valid frames of each row (<= Tm; mel must be zero beyond them).  Row b of the
 * result equals idxtts_bigvgan_fwd on mel[b, :, :mel_lengths[b]] alone -- every layer pads (zeros for the convolutions,
 * replicate for the anti-alias filters) at the row's OWN end, as the reference's per-utterance call does (infer_v2.py:860);
 * samples beyond mel_lengths[b] * prod(upsample_rates) are not meaningful. */
int idxtts_bigvgan_fwd_ragged(idxtts_ctx* ctx, const float* mel, const int* mel_lengths, float* wav, int B, int Tm, void* workspace,
                              size_t workspace_bytes, int clamp, void* stream);

/* ---- token-major building blocks (also used stand-alone by the tests) ------------------------------
 * idxtts_linear: Y[M][N] = act(X[M][K] W^T + bias) (+ residual) on the fp32 matrix core.
 * weight: [N][K] (torch nn.Linear) or, if weight_is_kn, [K][N] (HF Conv1D: model_v2.py:290 GPT2Model).
 * act: 0 none, 1 gelu_new, 2 silu, 3 swiglu (rows packed [32 gate | 32 linear] blocks; Y is [M][N/2]), 4 mish. */
typedef struct idxtts_linear idxtts_linear;
int idxtts_linear_create(const float* weight, const float* bias /* may be NULL */, int N, int K, int weight_is_kn,
                         idxtts_linear** out);
int idxtts_linear_fwd(const idxtts_linear* lin, const float* x, int ldx, float* y, int ldy, const float* residual /* may be NULL */,
                      int ldr, int M, int act, int bf16x3 /* 0: exact fp32 MFMA, 1: split-bf16 (3 bf16 MFMAs per product), 2: split-bf16 with the LDS-DMA kernel's 32x32x16 main loop,
                                    3: bf16 -- x and w rounded to nearest-even bf16, ONE MFMA per product, fp32 accumulation in the k order of
                                    form 1, epilogue and fp32 output unchanged: the LDS-DMA kernel's 16x16x32 loop, whatever
                                    idxtts_set_acoustic_bf16 says; needs M >= 256, N >= 96, K % 16 == 0.  Forms 0..2 never read that switch. */,
                      void* stream);
/* Arithmetic of the compute-bound passes of the model contexts (s2mel GEMMs and DiT attention, GPT latent pass, vocoder
 * convolutions): 0 = exact fp32 MFMA, 1 (default) = split-bf16: x*w ~= hi*hi' + hi*lo' + lo*hi' on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation (relative product error ~2^-16; mel / waveform stay ~1e-5 from the fp32
 * reference).  The KV-cached greedy decode and its prefill are always exact fp32 (token indices are bit-exact in both modes). */
int idxtts_set_gemm_mode(int mode);
int idxtts_get_gemm_mode(void);
/* Opt-in bf16 arithmetic of the acoustic stage (s2mel and BigVGAN): process-wide, default 0, effective only while the GEMM mode is 1
 * (mode 0 stays exact).  With it on, the compute-bound kernels of those two models multiply the hi values of the split form alone --
 * every fp32 operand rounded once to nearest-even bf16, ONE bf16 MFMA per product, fp32 accumulation in the k order of the split
 * kernel replaced (rows stay independent of row count and tile place), epilogues and fp32 outputs unchanged:
 *   - GEMMs of 256 rows and more on the LDS-DMA kernel whose weights run its 16x16x32 loop (s2mel, idxtts_linear_create).  Launches
 *     below 256 rows, shapes without weight planes (N < 96 or K % 16 != 0) and the exact kernel keep their arithmetic, so results below
 *     and above 256 rows differ by bf16 rounding (~2^-9 relative per operand), not by ~1e-5;
 *   - the DiT attention: QK^T on bf16 q and k, P rounded once to bf16, PV on bf16 v;
 *   - the vocoder convolutions that carry the bf16 pack (and idxtts_conv1d_fwd).
 * The GPT (prefill, latent pass, decode), conditioning, semantic, CAMPPlus and Qwen3 contexts never read the switch: everything that
 * feeds a choice of discrete codes is bit-identical with it on.  Measured cost and gain: profiles/README.md "Acoustic bf16". */
int idxtts_set_acoustic_bf16(int on);
int idxtts_get_acoustic_bf16(void);
/* Geometry of the decode step's GEMVs (5..16 rows, bf16 / fp8 weight streams): 0 (default) = 1024-thread workgroups, the fastest form
 * for a decode that has the GPU to itself; 1 = 512-thread workgroups at <= 88 VGPRs, which fit into what ONE retiring workgroup of
 * an s2mel / vocoder kernel frees on a CU: 7 % slower alone, but a serving loop that decodes beside the acoustic stages of other
 * batches (indextts_amd/serving.py) gains 1.5 % (profiles/README.md "Round 3").  The two forms split K over a different number of
 * waves, so results differ in the last bits: choose once per process, before generating (cached decode graphs carry the choice). */
int idxtts_set_decode_geometry(int narrow);
int idxtts_get_decode_geometry(void);
/* From how many decode rows on (compact weight streams) the decode step runs on the plane GEMV (csrc/gemv_pl.hip: activations split
 * into three bf16 planes inside the kernel, bf16 MFMA with exact products, K split over waves and workgroups, one weight stream
 * for up to 64 rows -- the accel engine's one-graph-for-all-rows batching, accel/accel_engine.py:221-310) instead of the fp32-MFMA
 * GEMV.  Default 17: two or more 16-row tiles (merged requests, 16 utterances x 3 beams: 7 % faster at 48 rows); at <= 16 rows the
 * fp32-MFMA GEMV's single-round-trip launches win by 8 %.  5..64 selects a threshold, 65 turns the plane path off, 0 restores the
 * default.  A shape the plane GEMV has no kernel for (49..64 rows of a compact model wider than d = 1280, idxtts_gemv_pl_plan_query)
 * stays on the fp32-MFMA GEMV.  Rows of 17..64-row decodes do not depend on the batch they are in; the two kernel families differ in summation order
 * (last bits), so choose once per process, before generating (cached decode graphs carry the choice). */
int idxtts_set_decode_plane_rows(int min_rows);
int idxtts_get_decode_plane_rows(void);
/* What the library itself would launch for one decode GEMV (host only, no GPU work: the answers of the launchers' own plan
 * functions, for tests and diagnostics).
 *   fx: the fp32-MFMA GEMV (csrc/gemv_fx.hip) on an [K][N] weight stream of `format` (0 fp32, 1 bf16, 2 fp8) and `rows` rows;
 *       with_slab = the caller hands the K-split slab (mlp.c_proj in the decode step), narrow = idxtts_set_decode_geometry(1).
 *       (mt, ntw, single, r4, narrow) and the format name the kernel instantiation; kw, cps, ksb the split of K over waves,
 *       16-k chunks per wave and workgroups.
 *   pl: the plane GEMV (csrc/gemv_pl.hip): column tiles per workgroup, K parts across workgroups, and whether a kernel exists
 *       for that pair (where none does, the decode step stays on the fp32-MFMA GEMV). */
typedef struct idxtts_gemv_fx_plan {
  int mt, ntw, single, r4, narrow, kw, cps, ksb;
} idxtts_gemv_fx_plan;
int idxtts_gemv_fx_plan_query(int N, int K, int rows, int format, int with_slab, int narrow, idxtts_gemv_fx_plan* out);
int idxtts_gemv_pl_plan_query(int N, int K, int rows, int* ct, int* kparts, int* has_kernel);
/* The CFM solver (idxtts_s2mel_cfm) can evaluate the conditional and the null half of its stacked batch (flow_matching.py:91-103,
 * one DiT.forward on 2B rows there) as two chains of launches on two streams, the null half a few kernels behind: 9 % less time
 * for a solver that has the device to itself (one half's HBM-bound epilogues beside the other's MFMA-bound loops).  Each half is
 * an evaluation of its own on B sequences, and the split-bf16 mode picks its kernels by row count (256 rows, see
 * idxtts_set_gemm_mode): the results are bit-identical to the stacked form -- same kernels on the same rows -- when B*T and 2B*T
 * are on the same side of 256 rows, and likewise B*Tt and 2B*Tt for the Tt = T - (shortest prompt - WaveNet context) frames the
 * solver evaluates behind the transformer when that prompt is long enough; otherwise they differ as the two GEMM modes do.  The
 * exact fp32 mode picks its kernels regardless of the row count and is bit-identical always.  on = 0 (default): one stacked 2B batch on the caller's stream, as the
 * reference evaluates it -- serving loops with several decode chains in flight should leave it off (profiles/README.md "Round 3"). */
int idxtts_s2mel_set_overlap(int on);
int idxtts_s2mel_get_overlap(void);
int idxtts_linear_destroy(idxtts_linear* lin);
/* The library keeps a little state per caller STREAM (the split-plane scratch of the LDS-DMA GEMM; the side stream and events of
 * idxtts_s2mel_set_overlap): a caller that retires a stream (a serving loop shutting down its worker threads) hands it back here,
 * before destroying the stream.  Stream-ordered, no device-wide synchronisation.  No reference counterpart (torch's caching
 * allocator plays this role there). */
int idxtts_release_stream(void* stream);
/* Multi-head attention, head_dim 64, softmax(q k^T * scale + mask) v without materialising the scores.
 * q/k/v/o are read in place: element (b, t, h, e) at base + b*batch_stride + t*token_stride + 64*h + e.
 * causal: key <= query.  kstart/kend: optional device int32 [B], keys outside [kstart, kend) are masked
 * (left padding of GPT prompts, model_v2.py:766-779; key padding of the DiT, diffusion_transformer.py:235-237). */
int idxtts_attention_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream);
/* Same contract on the bf16 matrix core with split operands (x = hi + lo, three bf16 MFMAs per product, fp32
 * accumulation; relative error ~2^-16).  Used by the s2mel DiT and the GPT latent pass when the GEMM mode is
 * IDXTTS_GEMM_BF16X3; the KV-cache-building prefill always runs the exact-fp32 form above. */
int idxtts_attention_bf16x3_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream);
/* Same contract in bf16 (what the DiT attention runs under idxtts_set_acoustic_bf16): q, k and v rounded once to nearest-even bf16
 * (q unscaled; the softmax scale is applied in fp32), QK^T with one bf16 MFMA per product and fp32 accumulation, fp32 softmax, P
 * rounded once to bf16 (the denominator sums the unrounded P), PV with one MFMA per product; fp32 output.  Against float64 attention
 * on the rounded inputs the error stays below 2^-8 max|v| + 1e-5. */
int idxtts_attention_bf16_fwd(const float* q, const float* k, const float* v, float* o, long q_batch_stride, int q_token_stride,
                         long kv_batch_stride, int kv_token_stride, long o_batch_stride, int o_token_stride, int B, int H,
                         int Sq, int Sk, int causal, const int* kstart, const int* kend, float scale, void* stream);
/* Non-causal self-attention (head_dim 64) with the "relative_key" distance embedding of the w2v-bert-2.0 encoder the reference's prompt block
 * runs (indextts/infer_v2.py:633-638 get_emb -> transformers Wav2Vec2BertSelfAttention, position_embeddings_type="relative_key"):
 *   scores[i][j] = scale * (q_i . k_j + q_i . rel_key[clamp(j - i, -rel_left, rel_right) + rel_left]),   rel_key [rel_left + rel_right + 1][64]
 * (one table for every head, at most 96 rows), keys >= kend[b] masked.  q / k / v share one batch / token stride (a fused qkv buffer);
 * split_bf16 = 0: exact-fp32 MFMAs, 1: split-bf16 products. */
int idxtts_attention_relkey_fwd(const float* q, const float* k, const float* v, float* o, long batch_stride, int token_stride,
                                long o_batch_stride, int o_token_stride, int B, int H, int S, const int* kend, float scale,
                                const float* rel_key, int rel_left, int rel_right, int split_bf16, void* stream);
/* The DiT attention of the s2mel stage in split-bf16 mode (calls of 256 rows and more), as an instrument on the caller's buffers:
 * non-causal attention, head_dim 64, that reads q / k / v as SPLIT-BF16 PLANES of one [Mrows][ncols] projection output.
 * Plane layout: element (row, col) of a [rows][cols] matrix lies at bf16 index ((col / 16) * rows + row) * 16 + col % 16 of the hi
 * plane (16-column chunks, each [rows][16]); a plane has ceil(cols / 16) * rows * 16 elements and the lo plane follows the hi plane
 * directly; hi = bf16(x) (nearest even), lo = bf16(x - hi).  `planes` (16-byte aligned) holds B batch rows of T rows each
 * (B * T <= Mrows); q / k / v of head h are columns q_col / k_col / v_col + 64 h .. + 63 (each a multiple of 16, inside ncols).
 * Queries of batch row b are rows b * T + q_row0 + [0, Sq) (q_row0 + Sq <= T), its keys rows b * T + [0, min(kend[b], T)); kend is
 * a device int32 [B] or NULL (T keys everywhere); a batch row without keys gives zeros.
 *   out[b][q] = softmax(scale * q k^T over the visible keys) v
 * Contract on the data: the kernel loads whole 32-key tiles and masks afterwards, so the rows of `planes` behind a batch row's
 * kend -- up to row Mrows - 1, the rows of the next batch row and any padding rows included -- must hold FINITE values in the k and v
 * columns (a tile past row Mrows - 1 re-reads that last row).  Their values do not reach the output.
 * Outputs, either or both (not both NULL): o, fp32, element (b, q, h, e) at o + b * o_batch_stride + q * o_token_stride + 64 h + e;
 * o_planes, split-bf16 planes of the [B * Sq][64 H] output in the layout above (row b * Sq + q, column 64 h + e).
 * one_product = 0: three bf16 MFMAs per product on hi + lo (q, k, v and P; relative error ~2^-16); 1: the hi planes alone, P rounded
 * once to bf16, one MFMA per product (the lo planes of q / k / v are not read) -- whatever idxtts_set_acoustic_bf16 says: that switch
 * picks the form for the s2mel stage, this entry takes it as a parameter.  B, H or Sq = 0: nothing is launched. */
int idxtts_attention_planes_fwd(const void* planes, int Mrows, int ncols, int q_col, int k_col, int v_col, int T, int q_row0, int Sq, int B,
                                int H, const int* kend, float scale, float* o, long o_batch_stride, int o_token_stride, void* o_planes,
                                int one_product, void* stream);
/* y = LayerNorm(x) * gamma + beta over the last dim (eps), rows of length d. */
int idxtts_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, int M, int d, float eps, void* stream);

/* ---- GPT stage (reference: UnifiedVoice.inference_speech model_v2.py:796-895, .forward 673-723) -----
 * State-dict keys accepted by idxtts_ctx_load_tensor: gpt.h.{i}.{ln_1,ln_2}.{weight,bias},
 * gpt.h.{i}.attn.{c_attn,c_proj}.{weight,bias}, gpt.h.{i}.mlp.{c_fc,c_proj}.{weight,bias}, gpt.ln_f.*, final_norm.*,
 * mel_head.*, mel_embedding.weight, text_embedding.weight, mel_pos_embedding.emb.weight, text_pos_embedding.emb.weight,
 * speed_emb.weight (UnifiedVoice.state_dict(), model_v2.py:381-443). */
typedef struct idxtts_gpt_config {
  int model_dim, heads, layers;          /* 1280, 20, 24 */
  int number_mel_codes;                  /* 8194 */
  int number_text_tokens;                /* 12000 (table has +1 rows) */
  int start_mel_token, stop_mel_token;   /* 8192, 8193 */
  int mel_pos_len, text_pos_len;         /* 1818, 602 */
} idxtts_gpt_config;
int idxtts_gpt_create(const idxtts_gpt_config* cfg, idxtts_ctx** out);
/* Scratch for sequences of S tokens per row (prefill: P+1; latent pass: 34+L+2+M+2) and max_new_tokens of decode. */
/* Compact storage of the GPT's linear weights (call between the last idxtts_ctx_load_tensor and idxtts_ctx_finalize).
 * Replaces the reference's reduced-precision switch (`use_fp16` -> self.gpt.half(), infer_v2.py:109, 145-146) and is what
 * BASELINE.json configs[4] names ("fp8 GPT GEMMs"): the decode step is bound by the weight stream, so the format decides
 * the bytes per token; the arithmetic stays the fp32 MFMA.
 *   format 0: fp32 (default, no-op)   1: bf16 (nearest-even)   2: fp8 e4m3fn with a power-of-two scale per output channel
 * The staged tensors are rewritten IN PLACE into an ordinary fp32 GPT-2 state that the format holds exactly --
 *   c_attn / c_fc: (ln.weight, ln.bias, W, b) -> (1, 0, Q(diag(ln.weight) W), ln.bias . W + b);   c_proj, mlp.c_proj, mel_head: Q(W)
 * (mathematically the same network up to Q) -- and prefill, latent pass and decode are all packed from them, so the three
 * passes run one model and idxtts_ctx_get_tensor returns exactly that model for the reference / oracle to run. */
int idxtts_gpt_quantize_weights(idxtts_ctx* ctx, int format);
/* Storage of the KV cache of the cached generation (idxtts_gpt_generate / _sampled / _beam): 0 = fp32 (default), 1 = bf16.
 * The other half of the reference's reduced-precision switch: with `use_fp16` the whole GPT, its `past_key_values` included, is
 * half precision (infer_v2.py:145-146; model_v2.py:149-151).  Here a key / value is rounded to bf16 (nearest even) once, when it
 * is produced -- in the prefill (whose own attention then reads the rounded values) and in every decode step (the new token's own
 * k / v included) -- and every product and sum stays fp32; the decode attention streams half the bytes (the KV read is the largest
 * HBM stream of a batched decode step: 1.7 GB against 1.0 GB of bf16 weights at 16 utterances).  The latent pass has no cache and
 * is unchanged.  Call any time between generations on the context; idxtts_gpt_workspace_bytes follows the format.
 *
 * 2 = IDXTTS_KV_FP8, scaled fp8: opt-in, never selected implicitly (not with fp8 weights either).  The contract:
 *   unit    one vector: the 64 head dims of one (layer, row, head, position); a key vector and a value vector separately, same rule
 *   scale   amax = max |x_i| over the fp32 values; s = 2^ceil(log2(amax / 448)), exponent clamped to [-100, 100] (the weight columns'
 *           rule), s = 1 when amax == 0.  Computed exactly from amax's exponent and mantissa (448 = 1.75 * 2^8)
 *   code    the OCP e4m3fn encoding of x_i / s, nearest with ties to the even code; |x_i / s| <= 448, so nothing ever saturates
 *   value   decode(code_i) * s, an exact fp32 product; every product and sum of the attention stays fp32
 *   when    once, when the key / value is produced: in the prefill (the k / v columns are replaced by the cached values, so the
 *           prefill attention reads them) and in every decode step, the new token's own k / v included
 *   Non-finite inputs, and amax above 448 * 2^100, are outside the contract.
 * Storage: one byte per element in the bf16 cache's arrangement, plus one fp32 scale per cached vector ([layer][row][head][position],
 * for K and for V) in the same caller-owned workspace: 68 bytes per vector against 128 for bf16; every *_workspace_bytes entry counts
 * them.  (fp32 scales, not one-byte exponents: the reader multiplies a score or a probability by the scale as loaded.)  The call fails
 * on a device whose f32 <-> fp8 conversions are not OCP e4m3fn (checked against the host codec on every code and every midpoint).
 * The prefill of an fp8 cache runs on the exact fp32 GEMMs in every arithmetic mode, like that of an fp32 cache: the split-bf16 GEMM's
 * 2^-16 moves a key / value across an e4m3 rounding boundary 250 x as often as an fp32 summation order does (measured: max |dlogit|
 * against the oracle 5.5e-2 with the split prefill, 1.8e-2 with the exact one).  Everywhere else the format follows the bf16 cache's
 * rules.  Measured on MI355X (profiles/README.md "fp8 KV cache"): half the cache memory; the decode attention's time per step and
 * the logit noise are tabulated there. */
#define IDXTTS_KV_F32 0
#define IDXTTS_KV_BF16 1
#define IDXTTS_KV_FP8 2
int idxtts_gpt_set_kv_format(idxtts_ctx* ctx, int format);
int idxtts_gpt_get_kv_format(const idxtts_ctx* ctx);
/* Batch-invariant mode: opt-in, per context, default 0 (off: every path is bit for bit what it is without the call).  With the mode on,
 * everything that feeds the choice of a code is a function of the request alone.
 * Contract: a request's codes -- and with logits_out its logits -- equal BIT FOR BIT those of the B = 1 call (idxtts_gpt_generate,
 * _generate_forced, _generate_sampled or _generate_beam) on its own unpadded prompt, for the same weight format, KV format and GEMM
 * mode, wherever the request runs: any row of a one-shot call of any B <= 64 with any pad_left; any slot or group of a greedy, sampled
 * or beam session of any `slots`; any lane; after any _park and _resume, into a session of any slot count.  It holds whatever
 * idxtts_set_decode_geometry and idxtts_set_decode_plane_rows say: the mode reads neither switch.
 * Seeded draws (exp_noise NULL) carry no term in B or in the group count: row b of a one-shot call at step t draws id v (beam: flat
 * index v of num_beams * V) from exp1_draw(seed + b * 0xD6E8FEB86659FD93, t * V + v) (beam: t * num_beams * V + v).  Row 0's stream is
 * the B = 1 stream, and that is the stream a session request (slot, group) draws from.  exp_noise supplied by the caller is read as
 * without the mode.
 * What the mode launches (csrc/gpt.hip; idxtts_batch_invariant_plan_query answers for one shape):
 *   decode GEMVs    the fp32-MFMA GEMV at every row count, in its 16-row-tile forms only: K slices, chunks per slice and K pieces
 *                   follow (N, K) alone, and a row's products are added in one order at every number of row tiles.  The 4-row form,
 *                   the narrow geometry and the plane GEMV (other summation orders) are never taken.
 *   decode attention  a row with n keys is cut into ceil(n / 512) pieces (at most 16; ceil(n / pieces) keys each, rounded up to 16) and
 *                   the pieces are merged in piece order.  The batch size only decides how many workgroups share a row's pieces out
 *                   (one workgroup walks all of them from 7 rows x 20 heads on), never what is added to what.
 *   prefill         the exact fp32 GEMMs and fp32 attention for every KV format (a bf16 cache's prefill too, which otherwise follows
 *                   the GEMM mode from 256 rows), and the attention's 32-key tiles counted from each row's first real key, so a
 *                   left-padded row equals the unpadded one.
 * Rules: those of idxtts_gpt_set_kv_format -- callable between generations (refused while one is in flight); cached decode graphs
 * carry the mode in their key; a session keeps the mode it had at _init (every later call on it is refused while the context's mode
 * differs).  Cost: profiles/README.md "Batch-invariant decode".  The latent pass and the acoustic stage are outside the contract. */
int idxtts_gpt_set_batch_invariant(idxtts_ctx* ctx, int on);
int idxtts_gpt_get_batch_invariant(const idxtts_ctx* ctx);
/* What the batch-invariant mode would launch (host only, no GPU work; the launchers' own plan functions):
 *   one decode GEMV of an [K][N] weight stream in `format` on `rows` rows (with_slab as idxtts_gemv_fx_plan_query): family (0 = the
 *   fp32-MFMA GEMV), r4, narrow, kw, cps, ksb -- the summation order, a function of (N, K) alone -- and mt, ntw, single, which name
 *   the instantiation for that many rows (how many row / column tiles a wave carries; no part in the order);
 *   the decode attention of a row with n_keys keys in a B-row step of `heads` heads on a cache of smax positions: attn_pieces and
 *   attn_piece_keys -- functions of n_keys alone -- and attn_workgroups, how many workgroups share the pieces out at that B. */
typedef struct idxtts_batch_invariant_plan {
  int family, r4, narrow, kw, cps, ksb;
  int mt, ntw, single;
  int attn_pieces, attn_piece_keys, attn_workgroups;
} idxtts_batch_invariant_plan;
int idxtts_batch_invariant_plan_query(int N, int K, int rows, int format, int with_slab, int B, int heads, int smax, int n_keys,
                                      idxtts_batch_invariant_plan* out);
/* Instrument (no reference counterpart; tests/test_decode_attn_gpu.py): the library's own KV-cache store and ONE step of its decode
 * attention on caller-owned device buffers, so that a test knows every cached bit.  Two launches, then the stream is synchronised:
 *   store   S > 0: positions [0, S) of the plain prefill rows qkv [n][S][3d] (d = 64 * heads) go to the caches in `kv_format` --
 *           slot_ids NULL: kv_store_prefill, row b -> cache row b (n == rows); else kv_store_slots, positions [0, len[b]) of row b ->
 *           the `fan` >= 1 consecutive cache rows from slot_ids[b] (slot_ids, len: device int32 [n]).  As in the product, the k / v
 *           columns of qkv are rewritten to the cached values.  Cache sizes: kcache and vcache rows * heads * smax * 64 elements of
 *           4 / 2 / 1 bytes (layouts: idxtts_gpt_set_kv_format; csrc/decode.h), kscale and vscale rows * heads * smax floats (fp8 only).
 *   step    decode_attn_forward on step_qkv [rows][3d] with the arguments GPTModel::attn_args builds: one c_attn part, no bias, scale
 *           0.125, kstart (device int32 [rows], never NULL), partial results and arrival counters sized as the GPT workspace sizes
 *           them and the counters zero on entry.  slot_state NULL: every row at position `pos` (a DecodeState); else the session
 *           form, slot_state = device int32 [rows][5], a SlotState {pos, mel_pos, step, max_step, live} per row.  invariant: the
 *           batch-invariant kernels.  nsplit 0: the library's rule (decode_attn_nsplit, or decode_attn_inv_wgs under invariant),
 *           1..16: that many workgroups per (row, head).  out: fp32 rows [rows][d], or with out_frag the A-fragment image
 *           (ceil(rows / 16) * (d / 16) * 256 floats).  The step also writes the new token's k / v at its position.
 * workspace: idxtts_decode_attn_probe_workspace_bytes(heads, rows) device bytes, 256-byte aligned; the arrival counters are its first
 * rows * heads uint32 (0 after the call).  nsplit_used returns the workgroups per (row, head) the step was launched with. */
typedef struct idxtts_decode_attn_probe {
  int kv_format, heads, rows, smax;
  int n, S;                                       /* the store (S = 0: none) */
  float* qkv;
  const int* slot_ids; const int* len; int fan;
  void* kcache; void* vcache; float* kscale; float* vscale;
  const float* step_qkv;                          /* the step */
  int pos;
  const int* kstart;
  const int* slot_state;
  int invariant, nsplit, out_frag;
  float* out;
  void* workspace; size_t workspace_bytes;
  int nsplit_used;                                /* out */
} idxtts_decode_attn_probe;
size_t idxtts_decode_attn_probe_workspace_bytes(int heads, int rows);
int idxtts_decode_attn_probe_run(idxtts_decode_attn_probe* p, void* stream);
/* Greedy generations keep their instantiated decode-step hipGraph per (workspace address and size, B, prompt length, max_new_tokens,
 * penalty): the same shapes on the same workspace replay it without re-capturing (at most 8 are kept, least recently used first
 * out).  Returns how many are held (diagnostics / tests), -1 for a non-GPT context. */
int idxtts_gpt_graph_cache_entries(idxtts_ctx* ctx);
size_t idxtts_gpt_workspace_bytes(const idxtts_ctx* ctx, int B, int S, int max_new_tokens);
/* out[r] = text_emb[text_ids[r]] + text_pos[text_pos_idx[r]] + mel_emb[mel_ids[r]] + mel_pos[mel_pos_idx[r]] + extra[extra_idx[r]],
 * every term skipped where its index is < 0 (or its index array is NULL).  Index arrays are device int32 [rows].
 * Builds the [pad|cond|text] prompt of prepare_gpt_inputs (model_v2.py:749-779) and the latent-pass input (704-716). */
int idxtts_gpt_embed(idxtts_ctx* ctx, float* out, int rows, const int* text_ids, const int* text_pos_idx, const int* mel_ids,
                     const int* mel_pos_idx, const float* extra, const int* extra_idx, void* stream);
/* Greedy KV-cached generation = the accel_engine.generate plugin slot (model_v2.py:871-883) with the HF greedy
 * semantics of the fallback path (do_sample=False, num_beams=1; RepetitionPenalty over the fake prefix + generated ids;
 * finished rows emit stop_mel_token; stops when every row has stopped or at max_new_tokens).
 * inputs_embeds: [B][P][d] device (the `tts_embeddings` argument); pad_left: HOST int32 [B] = number of left-pad rows
 * (attention_mask zeros), may be NULL.  codes: device int64 [B][max_new_tokens]; *n_steps (host) = columns that are valid.
 * logits_out: optional device [max_new_tokens][B][V] raw (pre-penalty) logits per step (disables graph replay). */
int idxtts_gpt_generate(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                        float repetition_penalty, long long* codes, int* n_steps, float* logits_out, void* workspace,
                        size_t workspace_bytes, int use_graph, void* stream);
/* Parity instrument: the greedy loop above TEACHER-FORCED on forced_codes (device int64 [B][max_new_tokens]) -- at every step the
 * row's own argmax (after the repetition penalty) is written to `codes`, and forced_codes[b][step] is what continues the sequence
 * (input_ids of the next step, the penalty set, the finished flag: transformers_generation_utils.py:3252-3264 with next_tokens
 * replaced).  With logits_out it yields the logits of a GIVEN token sequence, i.e. what a test compares with the reference's logits on
 * the reference's own codes when two correct implementations may part at a near-tie of the argmax.  Eager launches, no graph.
 * *n_steps = steps run (stops early only when every forced row has emitted the stop token). */
int idxtts_gpt_generate_forced(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                               float repetition_penalty, const long long* forced_codes, long long* codes, int* n_steps, float* logits_out,
                               void* workspace, size_t workspace_bytes, void* stream);
/* The same generation loop with multinomial sampling instead of argmax (reference default do_sample=True,
 * infer_v2.py:714-722; HF _sample transformers_generation_utils.py:3196-3262 with the warpers of 1036-1044):
 *   mode 1: repetition penalty -> / temperature -> top-k -> top-p -> softmax -> torch.multinomial(probs, 1);
 *   mode 2: the accel engine's Sampler (accel/accel_engine.py:648-659): softmax(logits / temperature) / clamp_min(q, 1e-10), argmax.
 * torch.multinomial with one draw per row is argmax(probs / q), q ~ Exp(1) from ONE exponential_() call on a [B][V] tensor
 * per step: the caller supplies those draws (exp_noise, device fp32 [max_new_tokens][B][V]), so a seeded torch generator on
 * the host side reproduces the reference token for token.  Beam search (num_beams > 1) is not covered. */
typedef struct idxtts_sampling {
  int mode;              /* 0 greedy (as idxtts_gpt_generate), 1 HF multinomial with warpers, 2 accel-engine sampler */
  float temperature;     /* > 0 */
  int top_k;             /* 0 = off */
  float top_p;           /* >= 1 = off; < 1 needs 0 < top_k <= 1024 */
  const float* exp_noise;
  unsigned long long seed;  /* used when exp_noise is NULL: the draws come from a counter-based generator keyed by (seed, step, row, id) */
} idxtts_sampling;
int idxtts_gpt_generate_sampled(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps,
                                float* logits_out, void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* Several takes of every prompt in one call (HF's num_return_sequences, _expand_inputs_for_generation): idxtts_gpt_generate (sampling
 * NULL or mode 0) or idxtts_gpt_generate_sampled on B * takes decode rows, row b * takes + j being take j of prompt b -- codes
 * [B * takes][max_new_tokens], logits_out [max_new_tokens][B * takes][V], exp_noise [steps][B * takes][V], a seeded row draws the
 * stream of row b * takes + j, the workspace is idxtts_gpt_workspace_bytes(B * takes, P + 1, max_new_tokens), B * takes <= 64 -- while
 * inputs_embeds [B][P][d] and pad_left [B] hold one entry per prompt and the prefill runs on those B rows: each row's keys and values
 * are written to its takes' cache rows and its last position feeds all of their first tokens.  The result equals the plain call on
 * the caller-expanded batch wherever the two prefills (B * (P + 1) and B * takes * (P + 1) rows) choose the same kernels: always
 * with an fp32 or fp8 KV cache or in the batch-invariant mode; with a bf16 cache in split-bf16 GEMM mode when both row counts lie on
 * the same side of 256.  takes = 1 is the plain call. */
int idxtts_gpt_generate_takes(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                              float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps, float* logits_out,
                              void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* ---- Scores: the log-probability of every code ----
 * For decode row b at the step t that writes token tok to codes[b][t]:
 *   lp[b][t] = (l[tok] - m) - logf(S),  m = max_v l[v],  S = sum_v expf(l[v] - m)
 * where l is the row's raw fp32 logits, exactly the values logits_out records: before the repetition penalty, temperature, top-k and
 * top-p, in every mode (greedy, HF, accel).  It is what HF's generate(output_logits=True) + compute_transition_scores(
 * normalize_logits=True) give -- not output_scores: with repetition penalty 10 and top-k 30 the processed scores of two takes are not
 * comparable.  S is summed in an order that depends on V alone (each of 1024 threads its own ids ascending, the wave butterfly, the
 * waves ascending): never on B, the slot, the sampler mode.  lp is finite for every finite logit row.  Steps after a one-shot row has
 * finished (pad steps) record 0.  A teacher-forced call records the log-probability of the code it writes to `codes`.
 * Sequence score (host, HF's sum_logprobs / len ** length_penalty): (sum_{t<n} lp[t]) / n ** length_penalty over the n codes produced,
 * the stop token included.
 * idxtts_gpt_generate_scored: idxtts_gpt_generate_takes (same workspace size, same codes, bit for bit) that also writes logprobs,
 * device fp32 [B * takes][max_new_tokens] (columns from *n_steps on are not defined).  sampling NULL = greedy.  A kept decode-step graph
 * is keyed by the logprobs address as well: a call with another buffer captures anew, a stale address is never replayed.
 * Determinism: wherever this header says "codes equal, bit for bit", the log-probabilities do too. */
int idxtts_gpt_generate_scored(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                               float repetition_penalty, const idxtts_sampling* sampling, long long* codes, int* n_steps, float* logprobs,
                               float* logits_out, void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* idxtts_gpt_generate_forced with the log-probabilities of the codes it writes (the rows' own argmax, not the forced tokens). */
int idxtts_gpt_generate_forced_scored(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                      float repetition_penalty, const long long* forced_codes, long long* codes, int* n_steps,
                                      float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes, void* stream);
/* ---- Continuing from given codes ----
 * The reference's inference_speech(..., input_tokens=) (model_v2.py:838-856): mel codes appended to input_ids, generation goes on behind
 * them.  A prefix of k codes makes the prefill run on P + 1 + k positions -- the prompt, mel_emb[start] + mel_pos[0], then
 * mel_emb[prefix[j]] + mel_pos[pos0 + j] for j < k -- and the row start with pos = P + k, mel_pos = k + 1: the first new code is fed
 * at mel position k + 2.  Two layouts, differing in the prefix codes' positions only:
 *   prefix_pos0 = 1 ("hf"): code j at mel position j + 1, what the reference's first forward embeds (model_v2.py:163-165);
 *   prefix_pos0 = 2 ("resume"): code j at mel position j + 2, where the uninterrupted run fed it (that run never uses position 1:
 *   model_v2.py:175).  The reference's continuation is therefore not the continuation of its own uninterrupted run; sessions use 2.
 * The repetition penalty sees the prefix, as HF's processor reads the whole input_ids.
 * idxtts_gpt_generate_prefix: idxtts_gpt_generate_scored with prefix (device int64 [B][k], one row per prompt, shared by its takes), k
 * and prefix_pos0; sampling, logprobs and logits_out may each be NULL.  max_new_tokens, exp_noise [max_new_tokens][B * takes][V], the
 * seeded draw counter, codes, logprobs and logits_out count NEW tokens from 0.  Workspace: idxtts_gpt_workspace_bytes(B * takes,
 * P + 1 + k, max_new_tokens).  k = 0 (prefix ignored) is idxtts_gpt_generate_scored bit for bit (logprobs NULL: _generate_takes).  Takes
 * with a prefix equal the caller-expanded batch under _generate_takes' conditions, the two prefills counting P + 1 + k positions a row.
 * Refused, before anything runs: k < 0, a NULL prefix with k > 0, prefix_pos0 other than 1 or 2; a prefix code outside [0, V) or equal
 * to stop_mel_token ("prefix contains the stop token"); k + max_new_tokens + 1 >= the mel position table's rows ("prefix +
 * max_new_tokens exceed the mel position table"); a workspace smaller than the size above. */
int idxtts_gpt_generate_prefix(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int takes, int P, int max_new_tokens,
                               float repetition_penalty, const idxtts_sampling* sampling, const long long* prefix, int k, int prefix_pos0,
                               long long* codes, int* n_steps, float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes,
                               int use_graph, void* stream);
/* ---- Scoring given codes ----
 * The log-probabilities ("Scores") of codes the context did not just emit, from ONE prefill instead of one decode step per code.
 * Row b has n_b >= 1 codes c_0 .. c_{n_b - 1}; the last may be stop_mel_token, no other may; all lie in [0, V).  Its prefill input is
 *   [ prompt rows (P, left pad as pad_left says) | mel_emb[start] + mel_pos[0] | mel_emb[c_j] + mel_pos[prefix_pos0 + j], j = 0 .. n_b - 2 ]
 * in the layouts of "Continuing from given codes": prefix_pos0 = 2 ("resume": where an uninterrupted run fed the codes) or 1 ("hf":
 * what the reference's first forward with input_tokens embeds).  The rows go through the input kernels and the prefill of
 * idxtts_gpt_generate_prefix unchanged (the GEMMs and the key / value rounding that prefill runs for the context's KV format; nothing is
 * cached).  lp[b][j] is "Scores"'s formula on the raw logits of position P + j with tok = c_j, for j < n_b: position P (the start
 * token) predicts c_0, position P + j (code c_{j-1}) predicts c_j.  lp[b][j] = 0 for n_b <= j < n.  Rows shorter than n = max n_b are
 * right-padded with code 0's table rows; attention is causal, so the padding reaches no scored position.  No repetition penalty,
 * temperature or warper applies, as in "Scores".
 * Head: ln_f -> final_norm -> mel_head on the scored positions of all rows packed one behind the other, at most 64 at a time, through
 * the decode step's GEMVs (chosen by each chunk's row count as a decode step of that many rows chooses them), each chunk reduced by
 * one launch of 1024-thread workgroups, one per position, that sum as the samplers do.  The head weights are streamed
 * ceil(sum_b n_b / 64) times per call.  In the batch-invariant mode the head runs that mode's GEMV at every row count, so a position's
 * value does not depend on the chunk it falls into, nor on the other rows of the call.
 * codes: device int64 [B][n] (columns from n_b on are not read); lens: HOST int32 [B], or NULL = every row n codes; logprobs: device
 * fp32 [B][n]; logits_out: device fp32 [B][n][V] or NULL -- the raw logits of every scored position, 0 from n_b on.  1 <= B <= 64.
 * Workspace: idxtts_gpt_score_workspace_bytes(ctx, B, P, n), for the context's KV format at the time of the call.
 * Refused, before anything runs: a NULL ctx, inputs_embeds, codes, logprobs or workspace; B outside 1 .. 64, P < 1, n < 1; n_b < 1 or
 * n_b > n; a pad_left outside [0, P); a code outside [0, V) ("a code outside the mel code table"); stop_mel_token before a row's last
 * code ("a stop token before a row's last code"); prefix_pos0 other than 1 or 2; prefix_pos0 + n - 1 >= the mel position table's rows
 * ("the codes exceed the mel position table"); a workspace smaller than the size above. */
size_t idxtts_gpt_score_workspace_bytes(const idxtts_ctx* ctx, int B, int P, int n);
int idxtts_gpt_score(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, const long long* codes, const int* lens,
                     int n, int prefix_pos0, float* logprobs, float* logits_out, void* workspace, size_t workspace_bytes, void* stream);
/* Beam search / beam-sample = what `IndexTTS2.infer` runs by default (infer_v2.py:714-722, 767: do_sample=True, num_beams=3,
 * top_p .8, top_k 30, temperature .8, repetition_penalty 10, length_penalty 0) through HF `_beam_search`
 * (transformers_generation_utils.py:3325-3516) + BeamSearchScorer (transformers_beam_search.py:123-420): log_softmax before
 * the processors, warpers with min_tokens_to_keep = 2, 2 * num_beams candidates per utterance drawn without replacement
 * (torch.multinomial == top-(2 num_beams) of probs / q, q ~ Exp(1): exp_noise, device fp32 [max_new_tokens][B][num_beams * V],
 * one exponential_() per step on the [B][num_beams * V] tensor) or taken as the plain top-k (do_sample = 0), hypotheses kept
 * per utterance, the best one returned.  codes: device int64 [B][max_new_tokens] = best hypothesis, the stop token appended when
 * it fits, stop-token padded; *n_steps = valid columns.  B * num_beams <= 64, 2 <= num_beams <= 8. */
typedef struct idxtts_beam {
  int num_beams;
  int do_sample;
  float temperature;
  int top_k;
  float top_p;
  float length_penalty;
  int early_stopping;        /* 0 = False (heuristic, the default), 1 = True */
  const float* exp_noise;
  unsigned long long seed;   /* used when exp_noise is NULL (see idxtts_sampling) */
} idxtts_beam;
size_t idxtts_gpt_beam_workspace_bytes(const idxtts_ctx* ctx, int B, int num_beams, int S, int max_new_tokens);
int idxtts_gpt_generate_beam(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                             float repetition_penalty, const idxtts_beam* beam, long long* codes, int* n_steps, void* workspace,
                             size_t workspace_bytes, int use_graph, void* stream);
/* idxtts_gpt_generate_beam returning the scorer's n_best best hypotheses of every utterance (BeamSearchScorer with
 * num_beam_hyps_to_keep = n_best = HF's num_return_sequences), 1 <= n_best <= num_beams: codes device int64 [B][n_best][max_new_tokens],
 * lens HOST int32 [B][n_best], scores HOST fp32 [B][n_best] (sequences_scores).  Order: finalize's (transformers_beam_search.py:355-380)
 * -- the ascending stable sort of the utterance's list, popped from the end: best first, among equal scores the one added later
 * first.  Each row is the hypothesis, then the stop token where it fits under the cap (lens counts it), then stop-padded.  Fewer than
 * n_best hypotheses cannot occur: finalize tops the list up from the open beams to num_beams entries.  *n_steps: min(longest
 * hypothesis + 1, max_new_tokens).  n_best = 1 returns exactly what idxtts_gpt_generate_beam returns. */
int idxtts_gpt_generate_beam_nbest(idxtts_ctx* ctx, const float* inputs_embeds, const int* pad_left, int B, int P, int max_new_tokens,
                                   float repetition_penalty, const idxtts_beam* beam, int n_best, long long* codes, int* lens, float* scores,
                                   int* n_steps, void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* Instrument: the host routine behind every beam read -- BeamSearchScorer.finalize for one utterance on HOST copies of its state, then
 * the rows of an n-best read.  hyp_score / hyp_len / hyp_slot [hyp_n]: the finished hypotheses in the order they were added, hypothesis q's
 * tokens in row hyp_slot[q] (0 .. 8) of hyp_seq [9][seq_ld]; unless `done`, the num_beams open beams (beam_scores
 * [num_beams], seq [num_beams][seq_ld]) join at steps_done tokens under BeamHypotheses.add's rule.  Out: codes [n_best][seq_ld]
 * stop-padded, lens [n_best] = min(length + 1, cap), scores [n_best]. */
int idxtts_beam_finalize_host(int num_beams, double length_penalty, int hyp_n, const double* hyp_score, const int* hyp_len,
                              const int* hyp_slot, const int* hyp_seq, int seq_ld, int done, const float* beam_scores, const int* seq,
                              int steps_done, int cap, int stop_token, int n_best, long long* codes, int* lens, float* scores);
/* ---- GPT decode session (continuous batching) ----
 * Stands in for the accel engine's per-sequence bookkeeping -- `context_lens` per sequence in the decode step and a KV allocation per
 * sequence that is taken when a sequence is admitted and given back when it finishes (accel_engine.py:154-212,
 * KVCacheManager.allocate / remove_seq in kv_manager.py:130-202) -- with a fixed set of `slots` decode rows, one KV region each.
 * Greedy (the semantics of idxtts_gpt_generate) unless initialised with IDXTTS_SESSION_SAMPLED (see _admit_sampled).  A slot retires
 * when it samples stop_mel_token (recorded) or at its own cap;
 * rows keep stepping on their own, so requests can be admitted into free slots between steps.
 * Determinism: a request's codes equal, bit for bit, row 0 of idxtts_gpt_generate on `slots` copies of its prompt with no left
 * padding (for a bf16 KV cache in split-bf16 GEMM mode: a reference batch of slots * (P + 1) >= 256 prefill rows), whatever else is in
 * flight, whenever it was admitted and whichever slot it has.  Results can depend on `slots` (decode attention key split, decode GEMV).
 * The caller owns the workspace (idxtts_gpt_session_workspace_bytes); the session lives in it until _release or the next _init on
 * it.  The KV format and the GEMM mode must stay as they were at _init.
 * In the batch-invariant mode (idxtts_gpt_set_batch_invariant; the session keeps the mode of its _init) the rule is simpler: a
 * request's codes equal those of the B = 1 call on its own prompt, for every `slots`, and so do the sampled and beam rules below
 * (seeded draws: the B = 1 stream). */
size_t idxtts_gpt_session_workspace_bytes(const idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens);
/* Prepares the workspace: every slot free.  max_prompt: longest prompt (P, the `tts_embeddings` rows) a request may have;
 * max_new_tokens: largest per-request cap. */
int idxtts_gpt_session_init(idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, float repetition_penalty, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Admits n requests into the free slots slot_ids (HOST int32 [n]): inputs_embeds device [n][ld_rows][d], request b's prompt in its
 * first prompt_lens[b] rows (HOST int32 [n], 1 .. max_prompt); max_new_tokens: HOST int32 [n] caps (1 .. max_new_tokens of _init).
 * Runs their prefill and first token. */
int idxtts_gpt_session_admit(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                             const int* slot_ids, const int* max_new_tokens, void* workspace, void* stream);
/* Sampled sessions: _workspace_bytes_ex / _init_ex with flags = IDXTTS_SESSION_SAMPLED add a per-slot sampler table; flags = 0 is
 * exactly _workspace_bytes / _init.  A sampled session's step samples every slot with its own request's idxtts_sampling. */
#define IDXTTS_SESSION_SAMPLED 1
/* Scored sessions ("Scores" above): flags |= IDXTTS_SESSION_SCORES, alone or with IDXTTS_SESSION_SAMPLED, adds [slots][max_new_tokens]
 * fp32 behind everything else in the workspace (flags 0 and 1: exactly the sizes and layout of before); every sampler launch of the
 * session -- the step's, the admissions' and _fork's first-token pass -- then records the log-probability of the code it writes, and
 * _read_scored returns them.  _admit, _admit_sampled, _admit_takes (each take's first code with its own lp[0]), _fork (a destination
 * receives lp[0, at) of the source), _evict, _stop, _park, _park_bytes and _resume work as on any session.  Beam sessions have no such
 * flag: their hypotheses carry the scorer's scores. */
#define IDXTTS_SESSION_SCORES 2
/* Sessions that admit rows behind given codes (_admit_prefix below): flags |= IDXTTS_SESSION_PREFIX sizes the admission's prefill area
 * for at least one row of max_prompt + 1 + max_new_tokens positions (without it: slots rows of max_prompt + 1) and adds two [slots]
 * int32 arrays behind everything else; every other flag combination keeps its size and layout.  Not for beam sessions. */
#define IDXTTS_SESSION_PREFIX 8       /* (4 is not a flag: _workspace_bytes_ex returns 0 for it and _init_ex refuses it, as ever) */
/* Sessions whose prefixed admissions can fill lp[0, k) from their own prefill (_admit_prefix_scored below): flags |=
 * IDXTTS_SESSION_PREFIX_SCORES, valid only together with IDXTTS_SESSION_PREFIX | IDXTTS_SESSION_SCORES (_workspace_bytes_ex returns 0 and
 * _init_ex refuses it otherwise), adds the 64-row head buffers of "Scoring given codes" and a packed [slots * max_new_tokens] fp32
 * staging buffer behind everything else; every other flag combination keeps its size and layout. */
#define IDXTTS_SESSION_PREFIX_SCORES 16
size_t idxtts_gpt_session_workspace_bytes_ex(const idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, int flags);
int idxtts_gpt_session_init_ex(idxtts_ctx* ctx, int slots, int max_prompt, int max_new_tokens, float repetition_penalty, int flags,
                               void* workspace, size_t workspace_bytes, void* stream);
/* _admit on a sampled session with a sampler per row: per_row HOST [n] (idxtts_sampling; mode 0 = greedy, bit-identical to the same
 * row in a greedy session).  exp_noise: NULL, or device fp32 [max_new_tokens[b]][V] that the caller keeps alive until the slot is read
 * (row t = the draws of the request's step t); with NULL the draws come from `seed`, the stream row 0 of a `slots`-row
 * idxtts_gpt_generate_sampled uses.  Determinism: a sampled request's codes equal, bit for bit, row 0 of idxtts_gpt_generate_sampled
 * with the same sampler on `slots` copies of its prompt (exp_noise: whose row 0 of every step is the request's row), under the greedy
 * rule's conditions above.  Every row is checked first (mode 0 / 1 / 2, temperature > 0, top_p < 1 needs 0 < top_k <= 1024): a bad
 * row refuses the whole call, no slot taken.  Refused on a greedy session.  The repetition penalty is the session's (HF mode applies
 * it, the accel sampler does not). _admit on a sampled session admits greedy rows. */
int idxtts_gpt_session_admit_sampled(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                     const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_row, void* workspace,
                                     void* stream);
/* ---- Several takes of one request ----
 * What HF's num_return_sequences is to generate (_expand_inputs_for_generation, model_v2.py:796, infer_v2.py:718, 771): several
 * continuations of one prompt, each an ordinary row of the session -- its own slot, cache rows, sampler, cap; stepped, read, evicted,
 * stopped, parked and resumed like any other -- whose prompt was prefilled once.  Greedy and sampled sessions; a beam session returns its
 * scorer's list instead (_read_nbest below).
 * _admit_takes: _admit_sampled with takes[b] >= 1 slots for request b (HOST int32 [n]).  slot_ids, max_new_tokens and per_take then hold
 * one entry per take, request after request -- T = sum(takes) <= slots entries; the slots free, distinct, in any order and not necessarily
 * adjacent.  per_take: HOST [T] idxtts_sampling, or NULL = every take greedy (the only choice on a greedy session).  Each request's
 * prefill runs once; its keys and values for positions [0, P + 1) go to all of its takes' slots, and each take's first token is drawn
 * with its own sampler in the admission's one head-and-sample pass.  Every check happens before anything changes.
 * Determinism: take j's codes equal, bit for bit, those of the same prompt admitted alone with sampler j -- the session rules above
 * hold per take.  The zero-row padding of the bf16 cache's prefill in split-bf16 mode counts prefill rows: a request counts once. */
int idxtts_gpt_session_admit_takes(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* takes,
                                   const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take, void* workspace,
                                   void* stream);
/* _fork: n further takes of the request in src_slot, branching where it stood after `at` codes, in the free slots dst_slots (HOST int32
 * [n]; at = -1: after all the codes it has, the stop token left out).  The source may be decoding, or ended and not read yet; it is only read.  One launch on `stream`, the session's stream, between
 * steps, that loads every 16-byte vector of the source's rows once and stores it to all n destinations (no intermediate buffer): bytes
 * read are proportional to P + at, bytes written n times that; the captured step and the workspace layout are untouched.
 * Each destination receives the source's step scalars cut back to step = at (pos = P + at, mel_pos = at + 1), codes [0, at), the set
 * of seen ids rebuilt from the start token and those codes, the cached keys, values and fp8 scales of every layer for the positions a
 * row with `at` codes holds -- [0, P + max(at, 1)): the prefill's P + 1 and one per code fed back -- its own sampler samplers[j] (HOST
 * [n]; NULL = greedy takes; exp_noise device fp32 [cap][V], row t = the draws of step t, rows below `at` never read), its own cap
 * max_new_tokens[j] (HOST [n]; NULL = the source's cap), live = 1, and its next decode input rebuilt from codes[at - 1] as _resume
 * rebuilds it.  at = 0: the take starts in front of its first token, which is drawn at once with its sampler (the admission's
 * head-and-sample pass on the destinations, after the copy).
 * Refused, before anything changes: a beam session; a source that is free or out of range; at < 0 or at > the source's codes (a source
 * that ended on the stop token: > the codes in front of it, for nothing follows a stop token); at = 0 on a source that came in through
 * _resume (or a take of one): its prefill output is gone; a destination that is busy, repeated, out of range or the source; a sampled
 * take on a greedy session or a bad sampler; a cap above the session's max_new_tokens, one that is not above `at`, or P + 1 + cap
 * beyond the cache length.
 * Determinism: a take forked at `at` = k with explicit draws E', E'[t] equal to the source's draws for t < k, returns bit for bit the
 * codes of a fresh admission of the same prompt with E' into a session of the same configuration; its first k codes are the source's.
 * With a seed the take draws from its own seed from step k on (a slot's stream is keyed by seed and step).  Every other row's codes,
 * the source's included, are untouched. */
int idxtts_gpt_session_fork(idxtts_ctx* ctx, int src_slot, int at, int n, const int* dst_slots, const idxtts_sampling* samplers,
                            const int* max_new_tokens, void* workspace, void* stream);
/* _admit_prefix ("Continuing from given codes" above, layout prefix_pos0 = 2): _admit_takes -- takes NULL = one slot per request, slot_ids /
 * max_new_tokens / per_take then [n] -- where request b starts behind the prefix_lens[b] >= 0 codes (HOST int32 [n]) it is given:
 * prefix, device int64, the n prefixes packed one behind the other (request b's at the sum of the lengths before it);
 * prefix_logprobs, device fp32 packed likewise, or NULL.  A request's takes share its prefix and its one prefill row of
 * P + 1 + k positions.  Each slot starts as _fork leaves a take cut at k: SlotState {P + k, k + 1, k, cap, live}, codes[0, k) = the
 * prefix, seen = {1, start} and the prefix, and on a scored session lp[0, k) = prefix_logprobs (NULL: 0); its first new code is drawn in
 * the admission.  The cap counts prefix + new codes; exp_noise [cap][V] and the seeded draw counter are indexed by the absolute step
 * (rows below k are never read: _fork's rule); _read returns prefix + continuation.  _fork at any at >= 1, _park, _resume, _evict,
 * _stop and _read_scored treat the row as any other (at = 0 is refused on it as on a resumed row: x_last is not the prompt's).
 * Every k = 0: _admit_takes, kernel for kernel.
 * The prefill takes rows x S positions of the prefill area, S = max_b (P_b + 1 + k_b), rows = n (bf16 KV in split-bf16 mode:
 * max(n, ceil(256 / S))); an admission above the area is refused with the limit in the message: admit in smaller groups.
 * Refused, before anything changes: a beam session ("a beam session takes no prefix"); a session without IDXTTS_SESSION_PREFIX when
 * some k > 0 (the message names the flag); k < 0 or k >= the request's cap, for any of its takes ("prefix: k >= cap"; since cap <=
 * max_new_tokens and _init checks max_new_tokens + 1 against the mel position table, no position can lie beyond the table or the
 * cache); a code outside [0, V) or equal to stop_mel_token ("prefix contains the stop token"); and everything _admit_takes refuses.
 * Determinism: the row's codes equal, bit for bit, row 0 of idxtts_gpt_generate_prefix (prefix_pos0 = 2) on `slots` copies of its
 * prompt and prefix with the same sampler -- exp_noise rows offset by k, a seed's counter likewise absolute in the session -- under the
 * session rules above; whatever else is admitted with it, whichever slot it has. */
int idxtts_gpt_session_admit_prefix(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens, const int* takes,
                                    const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take, const int* prefix_lens,
                                    const long long* prefix, const float* prefix_logprobs, void* workspace, void* stream);
/* _admit_prefix_scored: _admit_prefix with from_model, HOST unsigned char [n].  from_model[b] = 1: lp[0, k_b) of every take's slot is
 * what "Scoring given codes" defines for the request's prefix in layout prefix_pos0 = 2 -- position P_b + j of the admission's own
 * prefill row, which predicts prefix code j, goes through the scoring head (packed with the other such requests' positions, 64 at a
 * time) into the session's staging buffer, which the slot reset then reads as it reads prefix_logprobs; request b's segment of
 * prefix_logprobs is not read.  from_model[b] = 0 keeps _admit_prefix's rule (the caller's values, or 0 with prefix_logprobs NULL).
 * The codes drawn are those of _admit_prefix, bit for bit: the prefill, the reset's other outputs and the first-token pass are the
 * same launches on the same data.  The values are those of idxtts_gpt_score on the same prompt and prefix wherever both prefills
 * choose the same kernels; in the batch-invariant mode always, bit for bit.  _fork, _park and _resume carry them as any lp.
 * Refused, before anything changes: a session without IDXTTS_SESSION_PREFIX_SCORES (the message names the flag); a NULL from_model or
 * prefix_lens; and everything _admit_prefix refuses. */
int idxtts_gpt_session_admit_prefix_scored(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                           const int* takes, const int* slot_ids, const int* max_new_tokens, const idxtts_sampling* per_take,
                                           const int* prefix_lens, const long long* prefix, const float* prefix_logprobs,
                                           const unsigned char* from_model, void* workspace, void* stream);
/* Beam sessions (beam search / beam-sample per request, idxtts_gpt_generate_beam's semantics): the `slots` rows form slots / num_beams
 * groups of num_beams consecutive slots (2 <= num_beams <= 8, slots % num_beams == 0, slots <= 64); each admitted request takes one
 * group and runs HF _beam_search + BeamSearchScorer with its own idxtts_beam.  A group retires when its scorer is done
 * (BeamHypotheses.is_done with the request's early_stopping / length_penalty) or at the request's cap; _step then reports the group's
 * FIRST slot, and _read on that slot returns the best hypothesis followed by the stop token if it fits under the cap (reading any other
 * slot of a group is refused) and frees the group.  _admit / _admit_sampled on a beam session are refused, as is _admit_beam on any
 * other session.  The repetition penalty is the session's.
 * Determinism: a beam request's codes equal, bit for bit, row 0 of idxtts_gpt_generate_beam (same num_beams, do_sample, temperature,
 * top_k, top_p, length_penalty, early_stopping, repetition penalty) on slots / num_beams copies of its prompt with no left padding and
 * max_new_tokens = its cap -- with the same seed, or with exp_noise whose [:, 0, :] is the request's noise -- cut after its first stop
 * token (or cap codes), whatever else is in flight, whenever it was admitted and whichever group it has, under the greedy rule's
 * conditions above (bf16 KV in split-bf16 mode: slots * (P + 1) >= 256). */
size_t idxtts_gpt_session_workspace_bytes_beam(const idxtts_ctx* ctx, int slots, int num_beams, int max_prompt, int max_new_tokens);
int idxtts_gpt_session_init_beam(idxtts_ctx* ctx, int slots, int num_beams, int max_prompt, int max_new_tokens, float repetition_penalty,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* Admits n requests into the free groups group_ids (HOST int32 [n], 0 .. slots / num_beams - 1); inputs_embeds, ld_rows, prompt_lens and
 * max_new_tokens as in _admit (one prompt row set per request, its prefill runs once).  per_request: HOST [n] idxtts_beam, num_beams equal
 * to the session's; exp_noise NULL or device fp32 [max_new_tokens[b]][num_beams * V], kept alive by the caller until the group is read
 * (row t = the draws of the request's step t); with NULL the draws come from `seed`, the stream row 0 of a slots / num_beams-utterance
 * idxtts_gpt_generate_beam uses.  Every request is checked first (generate_beam's rules, num_beams, the cap): a bad one refuses the
 * whole call, no group taken.  Runs their prefill and first beam step. */
int idxtts_gpt_session_admit_beam(idxtts_ctx* ctx, int n, const float* inputs_embeds, int ld_rows, const int* prompt_lens,
                                  const int* group_ids, const int* max_new_tokens, const idxtts_beam* per_request, void* workspace,
                                  void* stream);
/* Runs n_steps decode steps for every live slot (a captured hipGraph is replayed when use_graph), then reports the slots that hold a
 * finished request not read yet: finished_slots HOST int32 [slots] (may be NULL), *n_finished. */
int idxtts_gpt_session_step(idxtts_ctx* ctx, int n_steps, int use_graph, int* finished_slots, int* n_finished, void* workspace,
                            void* stream);
/* Copies a finished slot's codes (up to and including the stop token) to codes (device int64, >= *n_codes entries: at most
 * max_new_tokens), sets *n_codes (host) and frees the slot. */
int idxtts_gpt_session_read(idxtts_ctx* ctx, int slot, long long* codes, int* n_codes, void* workspace, void* stream);
/* _read on a scored session (IDXTTS_SESSION_SCORES), which also copies the slot's *n_codes log-probabilities to logprobs (device fp32,
 * >= *n_codes entries).  Frees the slot as _read does.  Refused on a session without the flag, before anything changes. */
int idxtts_gpt_session_read_scored(idxtts_ctx* ctx, int slot, long long* codes, float* logprobs, int* n_codes, void* workspace,
                                   void* stream);
/* _read on a beam session's group for the scorer's n_best best hypotheses, 1 <= n_best <= num_beams: codes device int64, lens and scores
 * HOST [n_best], in idxtts_gpt_generate_beam_nbest's order and padding.  n_best = 1: codes receives lens[0] entries, exactly what _read
 * returns; else codes is [n_best][max_new_tokens of _init_beam], every row stop-padded to the end.  Frees the group.  Refused on every
 * other kind of session. */
int idxtts_gpt_session_read_nbest(idxtts_ctx* ctx, int slot, int n_best, long long* codes, int* lens, float* scores, void* workspace,
                                  void* stream);
/* Ending requests from outside (a client that went away, a failed job): what KVCacheManager.remove_seq is to the accel engine
 * (kv_manager.py:130-202) -- a sequence's KV allocation given back before it finished.  slots: HOST int32 [n], every kind of session; a
 * beam session addresses a group by its FIRST slot, as _read does.  Every id is checked before anything changes -- in range, holding a
 * request (admitted and not read), a group's first slot: one bad id refuses the whole call and changes nothing.  Both are one small
 * launch on `stream`, the session's stream, between steps (the ids travel in its arguments): no copy, no synchronisation, the captured
 * step and the workspace layout are untouched.
 * _evict: the requests end and are free at once: admissible in the next _admit, never reported by a later _step, _read refused.
 *   Allowed on a request that is decoding and on one that has ended and was not read.  A sampled request's exp_noise may be freed
 *   once the call has returned and the work queued on `stream` before it has run (stream order).
 * _stop: the requests that are decoding end and are kept: the next _step reports them (n_steps = 0 included) and _read returns the k
 *   codes produced so far (a beam group: its best hypothesis at k steps).  A request that has already ended is left alone.
 * Determinism: with any sequence of _evict and _stop calls between steps every other request's codes stay those of the rules above; a
 * request admitted into an evicted slot or group meets them as in any other; a stopped request returns, bit for bit, what the same
 * request with max_new_tokens = k returns (greedy, sampled: the first k codes of its uninterrupted run; beam: row 0 of
 * idxtts_gpt_generate_beam with max_new_tokens = k and the same seed, or the first k rows of its exp_noise). */
int idxtts_gpt_session_evict(idxtts_ctx* ctx, int n, const int* slots, void* workspace, void* stream);
int idxtts_gpt_session_stop(idxtts_ctx* ctx, int n, const int* slots, void* workspace, void* stream);
/* Preempt and resume: a decoding request steps aside and keeps what it has computed.  _park gathers everything the request's slot
 * owns -- step scalars, sampler, the ids it has seen, its codes and positions [0, pos) of its keys and values in every layer -- into
 * one contiguous DEVICE buffer, the parked row, and frees the slot as _evict does; _resume scatters a parked row into any free slot of
 * any session that fits it, at any later time.  Both are one launch on `stream`, the session's stream, between steps: bytes moved are
 * proportional to pos, the captured step and the workspace layout are untouched.  The row's next decode input is not saved: _resume
 * rebuilds it from the last code and the mel position, so a parked row does not depend on which GEMV the step runs.
 * Determinism: a request parked and resumed any number of times, into any slots, returns bit for bit the codes of its uninterrupted
 * run; every other request's codes are untouched.  Greedy and sampled sessions; both calls fail on a beam session, where one row of
 * a group cannot leave it: a whole group is parked with _park_group / _resume_group below.
 * The parked row: idxtts_park_header, then segments that each start 16-byte aligned, padding written as zero (a parked row is a
 * function of the request's state alone, byte for byte).  With pad16(n) = (n + 15) & ~15, V = number_mel_codes, C = 16 key chunks
 * (fp32 cache) or 8 (bf16, fp8), g = 16 bytes of one key chunk per position (fp32, bf16) or 8 (fp8), e = 4 / 2 / 1 bytes per element:
 *   [header 128] [seen: pad16(V)] [codes int64: pad16(8 * step)]
 *   then for every layer, for every head:  C key runs of pad16(pos * g) | values pos * 64 * e | fp8 only: key scales pad16(4 * pos) |
 *   value scales pad16(4 * pos)
 *   bytes = 128 + pad16(V) + pad16(8 * step) + layers * heads * (C * pad16(pos * g) + pos * 64 * e + (fp8 ? 2 * pad16(4 * pos) : 0))
 * A row parked from a scored session (IDXTTS_SESSION_SCORES) carries one more segment behind the codes, announced by reserved[1] = 1:
 *   [header 128] [seen: pad16(V)] [codes int64: pad16(8 * step)] [logprobs fp32: pad16(4 * step)]  then the layers as above
 * and bytes grows by pad16(4 * step); a row from any other session is byte for byte what it always was.
 * exp_noise travels as the caller's pointer: the tensor must stay alive while the row is parked and until the resumed request ends. */
#define IDXTTS_PARK_MAGIC 0x4b525049u      /* "IPRK" */
#define IDXTTS_PARK_VERSION 1
typedef struct idxtts_park_header {      /* 128 bytes */
  unsigned magic, version;
  int layers, heads, model_dim, number_mel_codes;      /* the model the row belongs to */
  int slots, kv_format, gemm_mode, sampled;            /* of the session it left (sampled: IDXTTS_SESSION_SAMPLED) */
  int pos, mel_pos, step, max_step;                    /* keys cached, mel position, codes produced, the request's cap */
  int mode; float temperature; int top_k; float top_p; /* the request's sampler (idxtts_sampling; mode 0 = greedy) */
  unsigned long long seed;
  unsigned long long exp_noise;                        /* device pointer, or 0 */
  unsigned long long bytes;                            /* the whole parked row, header included */
  int reserved[8];                                /* [0]: 1 = parked in the batch-invariant mode; [1]: 1 = parked from a scored
                                                     session (the logprobs segment follows the codes); everything else zero */
} idxtts_park_header;
/* Exact size of slot's parked row now (one small device-to-host read of its state); 0 with idxtts_last_error set when the slot cannot
 * be parked (see _park). */
size_t idxtts_gpt_session_park_bytes(idxtts_ctx* ctx, int slot, void* workspace, void* stream);
/* slot must hold a request that is still decoding: one that has ended is to be read (_read), not parked.  dst: device, 16-byte aligned,
 * dst_bytes >= _park_bytes.  Sets *written (host, may be NULL) and frees the slot: admissible in the next call, never reported by a
 * later _step.  Every refusal happens before anything changes. */
int idxtts_gpt_session_park(idxtts_ctx* ctx, int slot, void* dst, size_t dst_bytes, size_t* written, void* workspace, void* stream);
/* src: a parked row in device memory (16-byte aligned), src_bytes of it.  Refused, before anything changes: a bad magic or version,
 * another model's dimensions, a session with other slots, KV format or GEMM mode (they select the key split and the GEMV: the
 * remaining codes would belong to another reference), a sampled request offered to a greedy session, a cap above the session's
 * max_new_tokens, pos + (max_step - step) + 1 beyond the session's cache length, a slot that is busy or out of range, src_bytes
 * shorter than the header says, a row whose batch-invariant flag (reserved[0]) or scores flag (reserved[1]) differs from the
 * session's.  When both are in the
 * batch-invariant mode the slot counts need not match: nothing on the row's path depends on them, and the row's codes stay those of
 * its uninterrupted B = 1 run.  On success the slot decodes on from the next _step; src may be freed once the work queued on `stream`
 * has run (stream order). */
int idxtts_gpt_session_resume(idxtts_ctx* ctx, int slot, const void* src, size_t src_bytes, void* workspace, void* stream);
/* Preempt and resume, beam sessions: a GROUP steps aside (one row of a group cannot leave it, so the slot-addressed calls above keep
 * refusing a beam session; these calls refuse every other session).  _park_group gathers everything a decoding group owns -- the step
 * scalars of its num_beams slots (all equal), the request's idxtts_beam values, per beam the ids it has seen, its tokens and its beam
 * score, the scorer's finished hypotheses, and the keys and values of its cached positions in every layer -- into one contiguous
 * DEVICE buffer, the parked group, and frees the group as _evict does; _resume_group scatters it into any free group of any beam
 * session that fits it.  One launch each on `stream`, the session's stream, between steps; the captured step and the workspace layout
 * are untouched.  The prompt positions [0, Ps), Ps = pos - step + 1, hold the same keys and values in every row of a group (the
 * admission writes them to all of its slots and the beam re-indexing never moves them): they are read from the group's first slot and
 * stored ONCE, and _resume_group writes them to all num_beams rows; only the T = step - 1 generated positions [Ps, pos) are stored
 * per beam.  Bytes moved are proportional to Ps + num_beams * T.  The rows' next decode inputs are rebuilt from each beam's last token
 * and the mel position, as _resume does.
 * Determinism: a group parked and resumed any number of times, into any groups, returns bit for bit the codes of its uninterrupted
 * run; every other request's codes are untouched.
 * The parked group: idxtts_park_group_header, then segments that each start 16-byte aligned, padding written as zero, and so are the
 * tails of each token row behind its length and the hypothesis rows behind hyp_n: a parked group is a function of the request's state
 * alone, byte for byte.  With pad16, V, C, g, e as for a parked row, nb = num_beams, and
 *   kv(n) = C * pad16(n * g) + n * 64 * e + (fp8 ? 2 * pad16(4 * n) : 0)
 * the bytes of n positions of one (layer, head) -- C key runs, the value run, fp8 only: key scales, value scales:
 *   [header 128] [seen: nb x pad16(V)] [tokens int32: nb x pad16(4 * step)] [beam scores fp32: pad16(4 * nb)]
 *   [hyp_worst fp64: 16] [hypothesis scores fp64: pad16(8 * nb)] [hypothesis lengths int32: pad16(4 * nb)]
 *   [hypothesis tokens int32: nb x pad16(4 * step), the scorer's list in its own order]
 *   then for every layer, for every head:  kv(Ps) of the shared positions | for every beam: kv(T) of its generated positions
 *   bytes = 128 + nb * pad16(V) + 2 * nb * pad16(4 * step) + 16 + pad16(8 * nb) + 2 * pad16(4 * nb)
 *           + layers * heads * (kv(Ps) + nb * kv(T))
 * exp_noise travels as the caller's pointer, under the same lifetime rule as a parked row's. */
#define IDXTTS_PARK_GROUP_MAGIC 0x4b524742u      /* "BGRK" */
#define IDXTTS_PARK_GROUP_VERSION 1
typedef struct idxtts_park_group_header {      /* 128 bytes */
  unsigned magic, version;
  int layers, heads, model_dim, number_mel_codes;      /* the model the group belongs to */
  int slots, num_beams, kv_format, gemm_mode;          /* of the session it left */
  int pos, mel_pos, step, max_step;                    /* keys cached, mel position, tokens per beam, the request's cap */
  int do_sample; float temperature; int top_k; float top_p;      /* the request's idxtts_beam values */
  double length_penalty;
  int early_stopping;
  int batch_invariant;                                 /* 1 = parked in the batch-invariant mode */
  unsigned long long seed;
  unsigned long long exp_noise;                        /* device pointer, or 0 */
  int hyp_n, done;                                     /* finished hypotheses the scorer holds (0 .. num_beams); its done flag */
  unsigned long long bytes;                            /* the whole parked group, header included */
  int reserved[2];                                     /* zero */
} idxtts_park_group_header;
/* Exact size of the parked group now (one small device-to-host read of its state); 0 with idxtts_last_error set when the group cannot
 * be parked (see _park_group).  group: 0 .. slots / num_beams - 1, as in _admit_beam. */
size_t idxtts_gpt_session_park_group_bytes(idxtts_ctx* ctx, int group, void* workspace, void* stream);
/* group must hold a request that is still decoding: one that has ended is to be read (_read).  dst: device, 16-byte aligned, dst_bytes
 * >= _park_group_bytes.  Sets *written (host, may be NULL) and frees the group: admissible in the next call, never reported by a later
 * _step.  Refused, before anything changes: a greedy or sampled session, a group that is free, out of range or has ended, dst_bytes
 * too small. */
int idxtts_gpt_session_park_group(idxtts_ctx* ctx, int group, void* dst, size_t dst_bytes, size_t* written, void* workspace,
                                  void* stream);
/* src: a parked group in device memory (16-byte aligned), src_bytes of it.  Refused, before anything changes: a greedy or sampled
 * session, a bad magic (a parked row's included) or version, another model's dimensions, a session with another num_beams, KV format
 * or GEMM mode, or other slots (seeded draws index with slots / num_beams, the key split and the GEMV follow the row count) unless
 * both sides are in the batch-invariant mode, a batch-invariant flag that differs from the session's, a cap above the session's
 * max_new_tokens, pos + (max_step - step) + 1 beyond the session's cache length, a group that is busy or out of range, src_bytes
 * shorter than the header says.  On success the group decodes on from the next _step; src may be freed once the work queued on
 * `stream` has run (stream order). */
int idxtts_gpt_session_resume_group(idxtts_ctx* ctx, int group, const void* src, size_t src_bytes, void* workspace, void* stream);
/* Forgets the session on this workspace (and its captured step); the caller may then free or reuse the workspace. */
int idxtts_gpt_session_release(idxtts_ctx* ctx, void* workspace);
/* Latent pass: full causal forward over emb [B][S][d]; latent[b][i] = final_norm(ln_f(h[b][mel_start + i])), i < M.
 * pad_left: optional HOST int32 [B], leading rows of each sequence that are padding (masked as keys), so rows with
 * shorter texts can share a batch and still reproduce the reference's per-utterance (B=1) result. */
int idxtts_gpt_latent(idxtts_ctx* ctx, const float* emb, const int* pad_left, int B, int S, int mel_start, int M, float* latent,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- prompt-conditioning encoders (reference: UnifiedVoice.get_conditioning model_v2.py:627-663, get_emo_conditioning
 * 665-671, get_emovec / merge_emovec 897-910; ConformerEncoder conformer_encoder.py:284-520; PerceiverResampler
 * perceiver.py:193-317).  One context per encoder pair:
 *   emotion = 0: keys "conditioning_encoder.*" + "perceiver_encoder.*"            -> latents [B][num_latents][perceiver_dim]
 *   emotion = 1: keys "emo_conditioning_encoder.*" + "emo_perceiver_encoder.*" + "emovec_layer.*" + "emo_layer.*"
 *                                                                                 -> emotion vector [B][model_dim] (get_emovec)
 * The sinusoid buffer "<encoder>.embed.pos_enc.pe" [1][max_len][output_size] of the reference's state_dict is a required
 * tensor (embedding.py:45-53). */
typedef struct idxtts_cond_config {
  int input_size;                                   /* 1024 (w2v-bert features) */
  int output_size, linear_units, attention_heads, num_blocks, cnn_kernel;   /* 512, 2048 | 1024, 8 | 4, 6 | 4, 15 */
  int perceiver_dim, num_latents, perceiver_depth, perceiver_dim_head, perceiver_mult;   /* 1280 | 1024, 32 | 1, 2, 64, 2 */
  int emotion;
  int model_dim;                                    /* 1280: width of emovec_layer / emo_layer (emotion = 1) */
} idxtts_cond_config;
int idxtts_cond_create(const idxtts_cond_config* cfg, idxtts_ctx** out);
size_t idxtts_cond_workspace_bytes(const idxtts_ctx* ctx, int B, int T);
/* feats: device [B][T][input_size]; lengths: HOST int32 [B] valid frames per prompt, or NULL = all T (values > T are
 * clamped: the reference passes the feature width 1024 as "length", infer_v2.py:751-752, i.e. no padding). */
int idxtts_cond_forward(idxtts_ctx* ctx, const float* feats, const int* lengths, int B, int T, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The same for several prompts of different lengths, right-padded into one batch, each row computing what its OWN unpadded call of
 * idxtts_cond_forward computes (the reference runs these encoders on one prompt at a time, infer_v2.py:748-754, model_v2.py:819; its
 * masks alone do not give that: a padded frame's pointwise-conv bias reaches the last valid frames through the depthwise taps).
 * extents: HOST int32 [B], the frames row b really holds (3 .. T); lengths: as above, what the row's own call would be given, or NULL. */
int idxtts_cond_forward_rows(idxtts_ctx* ctx, const float* feats, const int* lengths, const int* extents, int B, int T, float* out,
                             void* workspace, size_t workspace_bytes, void* stream);
/* out = base + alpha * (emo - base) over n floats (merge_emovec, model_v2.py:904-910). */
int idxtts_emovec_merge(float* out, const float* base, const float* emo, float alpha, size_t n, void* stream);

/* ---- semantic features of a prompt (reference: IndexTTS2.get_emb, infer_v2.py:381-408; build_semantic_model,
 * utils/maskgct_utils.py:87-93) -------------------------------------------------------------------------
 * The first `num_layers` conformer layers of w2v-bert-2.0 (third-party: transformers' Wav2Vec2BertModel, pinned 4.52.1 by the
 * reference; `hidden_states[17]` of `output_hidden_states=True` is the INPUT of layer 17, i.e. 17 layers run), then
 * (x - semantic_mean) / semantic_std.  State-dict keys: Wav2Vec2BertModel's own ("feature_projection.*",
 * "encoder.layers.{i}.*" for i < num_layers; later layers and "masked_spec_embed" are not consumed), plus the optional
 * vectors "semantic_mean" / "semantic_std" [hidden_size] (wav2vec2bert_stats.pt: mean, sqrt(var)). */
typedef struct idxtts_w2vbert_config {
  int input_dim, hidden_size, num_heads, intermediate_size;   /* 160, 1024, 16, 4096 */
  int num_layers;                                             /* 17 */
  int left_max, right_max, conv_kernel;                       /* 64, 8, 31 (relative_key distance embedding; causal depthwise conv) */
  float layer_norm_eps;                                       /* 1e-5 */
} idxtts_w2vbert_config;
int idxtts_w2vbert_create(const idxtts_w2vbert_config* cfg, idxtts_ctx** out);
size_t idxtts_w2vbert_workspace_bytes(const idxtts_ctx* ctx, int B, int T);
/* feats: device [B][T][input_dim] (SeamlessM4TFeatureExtractor's input_features); lengths: HOST int32 [B] valid frames
 * (attention_mask.sum(1)) or NULL = all T; out: device [B][T][hidden_size] (rows t >= lengths[b] are unspecified). */
int idxtts_w2vbert_forward(idxtts_ctx* ctx, const float* feats, const int* lengths, int B, int T, float* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- semantic codec, `quantize` (reference: `_, S_ref = self.semantic_codec.quantize(spk_cond_emb)`, infer_v2.py:637; RepCodec,
 * utils/maskgct/models/codec/kmeans/repcodec_model.py:179-199; build_semantic_codec, utils/maskgct_utils.py:96-99) ------
 * State-dict keys: RepCodec's own, "encoder.*" (VocosBackbone + Linear) and "quantizer.quantizers.0.{in_project,out_project,
 * codebook}.*" with the weight-norm pairs folded to plain ".weight"; "decoder.*" is not consumed. */
typedef struct idxtts_repcodec_config {
  int hidden_size, codebook_size, codebook_dim;                   /* 1024, 8192, 8 */
  int vocos_dim, vocos_intermediate_dim, vocos_num_layers;        /* 384, 2048, 12 */
} idxtts_repcodec_config;
int idxtts_repcodec_create(const idxtts_repcodec_config* cfg, idxtts_ctx** out);
size_t idxtts_repcodec_workspace_bytes(const idxtts_ctx* ctx, int B, int T);
/* x: device [B][T][hidden_size] (the normalised w2v-bert features); indices: device int64 [B][T]; quantized: device
 * [B][T][hidden_size] (= quantize(x)[1], already transposed back to token-major: the S_ref the length regulator takes). */
int idxtts_repcodec_quantize(idxtts_ctx* ctx, const float* x, int B, int T, long long* indices, float* quantized, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- log-mel spectrogram of the prompt (reference: `ref_mel = self.mel_fn(audio_22k)`, infer_v2.py:291-301, 640;
 * mel_spectrogram, s2mel/modules/audio.py:45-83) -----------------------------------------------------------------------
 * Tensors of the context: "mel_basis" [num_mels][n_fft/2+1] (the reference's librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax))
 * and "window" [win_size] (torch.hann_window(win_size)). */
typedef struct idxtts_melspec_config {
  int n_fft, hop_size, win_size, num_mels;          /* 1024, 256, 1024, 80 */
} idxtts_melspec_config;
int idxtts_melspec_create(const idxtts_melspec_config* cfg, idxtts_ctx** out);
int idxtts_melspec_frames(const idxtts_ctx* ctx, int n_samples);       /* (n_samples + 2 * ((n_fft - hop) / 2) - n_fft) / hop + 1 */
size_t idxtts_melspec_workspace_bytes(const idxtts_ctx* ctx, int B, int n_samples);
/* audio: device [B][n_samples] in [-1, 1]; mel: device [B][num_mels][frames] = log(clamp(mel_basis @ |STFT|, 1e-5)). */
int idxtts_melspec_forward(idxtts_ctx* ctx, const float* audio, int B, int n_samples, float* mel, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- Kaldi filter bank of the 16 kHz prompt audio, for a ragged batch of prompts (replaces the host numpy of
 * indextts_amd/features.py: `SeamlessM4TFeatureExtractor(audio_16k)`, infer_v2.py:633, 680, and `torchaudio.compliance.kaldi.fbank(
 * audio_16k, num_mel_bins=80, dither=0, sample_frequency=16000)` minus its mean over time, infer_v2.py:641-646) -------------
 * snip_edges framing, per frame: mean removal, pre-emphasis, window, power spectrum, mel filters, log(max(., 2^-23)).
 * Tensors of the context: "window" [frame_length] (povey) and "mel_filters" [num_mel_bins][fft_length/2+1] (Kaldi's get_mel_banks). */
typedef struct idxtts_fbank_config {
  int frame_length, hop_length, fft_length, num_mel_bins;      /* 400, 160, 512, 80 */
  float preemphasis;                                           /* 0.97 */
} idxtts_fbank_config;
#define IDXTTS_FBANK_RAW 0        /* the log-mel energies themselves (kaldi.fbank) */
#define IDXTTS_FBANK_CAMPPLUS 1   /* minus every bin's mean over the row's own frames (infer_v2.py:646) */
#define IDXTTS_FBANK_W2VBERT 2    /* every bin normalised over the row's own frames (mean, variance with ddof = 1, + 1e-7), frames stacked in pairs */
int idxtts_fbank_create(const idxtts_fbank_config* cfg, idxtts_ctx** out);
int idxtts_fbank_frames(const idxtts_ctx* ctx, int n_samples);       /* n_samples < frame_length ? 0 : 1 + (n_samples - frame_length) / hop_length */
/* n_samples: HOST int32 [B] */
size_t idxtts_fbank_workspace_bytes(const idxtts_ctx* ctx, const int* n_samples, int B);
/* audio: device [B][ld_audio], row b holds n_samples[b] (HOST int32 [B], each >= frame_length) samples, multiplied by `scale` before
 * anything else (2^15 for w2v-BERT, 1 for CAMPPlus).  out: device, zero at every padded position;
 *   RAW / CAMPPLUS: [B][T_out][num_mel_bins], T_out >= the longest row's frames;
 *   W2VBERT:        [B][T_out][2 * num_mel_bins], T_out >= ceil(longest row's frames / 2); every row needs two frames; an odd frame
 *                   count leaves a last row (frame | zeros), which the extractor's attention mask does not count (valid = frames / 2).
 * Both GEMMs are exact fp32 whatever the GEMM mode: a row's result does not depend on the rows beside it. */
int idxtts_fbank_forward(idxtts_ctx* ctx, const float* audio, int ld_audio, const int* n_samples, int B, float scale, int mode, float* out,
                         int T_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- polyphase windowed-sinc resampler for a ragged batch of one rate pair (replaces the host `audioio.sinc_resample`, i.e.
 * `torchaudio.transforms.Resample(orig, new)`, infer_v2.py:629-630; torchaudio/functional/functional.py::_apply_sinc_resample_kernel) ----
 * orig / new: the two rates divided by their gcd.  kernel_t: device [2 * width + orig][new], the TRANSPOSE of torchaudio's
 * `_get_sinc_resample_kernel` table (float32).  x: device [B][ldx], row b holds lengths[b] (HOST int32 [B], >= 0) samples.
 * out: device [B][ldo], ldo >= ceil(new * max length / orig): out[b][f * new + p] = sum_t padded_b[f * orig + t] * kernel[p][t] for the
 * first ceil(new * lengths[b] / orig) positions (padded_b = `width` zeros, the row, zeros), 0 behind them.  Products are summed in
 * float64 and rounded once.  No context: the table belongs to the caller. */
int idxtts_resample_forward(const float* kernel_t, int orig, int new_rate, int width, const float* x, int ldx, const int* lengths, int B,
                            float* out, int ldo, void* stream);

/* ---- CAMPPlus speaker encoder: the global style vector of the prompt (reference: `style = self.campplus_model(feat.unsqueeze(0))`,
 * infer_v2.py:251-257, 641-647; CAMPPlus, s2mel/modules/campplus/DTDNN.py:62-140, layers.py) ------------------------------
 * State-dict keys: CAMPPlus's own ("head.*", "xvector.*": campplus_cn_common.bin), BatchNorm running statistics included
 * (inference mode; "num_batches_tracked" entries are ignored). */
typedef struct idxtts_campplus_config {
  int feat_dim, embedding_size;                        /* 80, 192 */
  int m_channels, growth_rate, bn_size, init_channels; /* 32, 32, 4, 128 */
  int num_blocks;                                      /* 3 */
  int block_layers[4], block_dilation[4];              /* {12, 24, 16}, {1, 2, 2} (kernel 3) */
} idxtts_campplus_config;
int idxtts_campplus_create(const idxtts_campplus_config* cfg, idxtts_ctx** out);
size_t idxtts_campplus_workspace_bytes(const idxtts_ctx* ctx, int T);
/* feat: device [B][T][feat_dim] (Kaldi fbank minus its mean over time); style: device [B][embedding_size]. */
int idxtts_campplus_forward(idxtts_ctx* ctx, const float* feat, int B, int T, float* style, void* workspace, size_t workspace_bytes, void* stream);

/* ---- s2mel stage (reference: infer_v2.py:835-856; MyModel commons.py:390-420) -------------------------
 * State-dict keys: "cfm.estimator.*", "length_regulator.*", "gpt_layer.{0,1,2}.*" (s2mel.pth['net'][...], weight-norm
 * layers folded to plain ".weight"), "semantic_codec.quantizer.quantizers.0.{codebook.weight,out_project.weight,out_project.bias}",
 * plus one constant table "rope_cache" [T][32][2] = precompute_freqs_cis (gpt_fast/model.py:336-345). */
typedef struct idxtts_s2mel_config {
  int hidden_dim, num_heads, depth;      /* DiT: 512, 8, 13 */
  int in_channels, content_dim, style_dim;   /* 80, 512, 192 */
  int wn_hidden, wn_layers, wn_kernel, wn_dilation_rate;   /* 512, 8, 5, 1 */
  int lr_channels, lr_in_channels, lr_num_convs;           /* 512, 1024, 4 */
  int gpt_dim; int gpt_layer_dims[3];                      /* 1280; 256,128,1024 */
  int codebook_size, codebook_dim, codec_hidden;           /* 8192, 8, 1024 */
  float norm_eps;                                          /* 1e-5 */
} idxtts_s2mel_config;
int idxtts_s2mel_create(const idxtts_s2mel_config* cfg, idxtts_ctx** out);
/* cond = length_regulator(vq2emb(codes) + gpt_layer(latent)) (infer_v2.py:835-849).  latent [B][M][gpt_dim], codes int64
 * [B][M] (device); code_lens / target_lens: HOST int32 [B] (target = floor(1.72 * code_len), infer_v2.py:844);
 * cond_out [B][Tg][lr_channels], rows >= target_lens[b] are zero.  Statistics (GroupNorm) are per utterance. */
size_t idxtts_s2mel_cond_workspace_bytes(const idxtts_ctx* ctx, int B, int M, int Tg);
int idxtts_s2mel_prepare_cond(idxtts_ctx* ctx, const float* latent, const long long* codes, const int* code_lens,
                              const int* target_lens, int B, int M, int Tg, float* cond_out, void* workspace,
                              size_t workspace_bytes, void* stream);
/* length_regulator(S, ylens) alone (InterpolateRegulator.forward, length_regulator.py:117-141) = the prompt-side call of
 * infer_v2.py:649-652 that turns S_ref into prompt_condition: S [B][M][lr_in_channels]; in_lens / target_lens HOST int32 [B];
 * cond_out [B][Tg][lr_channels], rows >= target_lens[b] zero.  Workspace: idxtts_s2mel_cond_workspace_bytes(ctx, B, M, Tg). */
int idxtts_s2mel_regulate(idxtts_ctx* ctx, const float* S, const int* in_lens, const int* target_lens, int B, int M, int Tg, float* cond_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* CFM Euler solve with classifier-free guidance = cfm.inference (flow_matching.py:31-115) with the noise given:
 * mu [B][T][content_dim]; x_lens HOST [B]; prompt [B][in_channels][Tp_max] + prompt_lens HOST [B]; style [B][style_dim];
 * z [B][in_channels][T] (the randn of flow_matching.py:52); t_emb device [n_steps][256] sinusoidal timestep features and
 * dt HOST [n_steps] (both from torch.linspace as the reference does); out [B][in_channels][T] (caller slices off the prompt). */
size_t idxtts_s2mel_cfm_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int n_steps);
int idxtts_s2mel_cfm(idxtts_ctx* ctx, const float* mu, const int* x_lens, const float* prompt, const int* prompt_lens, int Tp_max,
                     const float* style, const float* z, const float* t_emb, const float* dt, int n_steps, float cfg_rate,
                     float* out, int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* The same solve on a batch whose rows come from DIFFERENT prompts (speakers): cfm.inference (flow_matching.py:31-115) on
 * mu_b = cat([prompt_condition_b, gen_cond_b]) with prompt ref_mel_b, then vc_target = mel[:, :, Tp_b:] (infer_v2.py:850-856),
 * for every row b at once.  gen_cond [B][Tg_max][content_dim] (the idxtts_s2mel_prepare_cond output) and target_lens HOST [B];
 * prompt_conditions / ref_mels: HOST tables of B DEVICE pointers, row b's prompt_condition [Tp_b][content_dim] (16-byte aligned)
 * and ref_mel [in_channels][Tp_b] -- rows of one speaker point at the same tensors --; prompt_lens HOST [B] = Tp_b;
 * style [B][style_dim]; z [B][in_channels][T] with T = max_b(Tp_b + Tg_b), row b's noise in its first Tp_b + Tg_b frames;
 * t_emb, dt, n_steps, cfg_rate as idxtts_s2mel_cfm.  out [B][in_channels][Tg_max]: row b's generated frames left-aligned,
 * zero from target_lens[b] on (the vocoder's input as it is).  A row's frames do not depend on the other rows' prompts (the
 * post-transformer part starts at the shortest prompt minus the WaveNet context: more frames, same values on this row's own).
 * Workspace: idxtts_s2mel_cfm_rows_workspace_bytes(ctx, B, T, max_b Tp_b, n_steps). */
size_t idxtts_s2mel_cfm_rows_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int Tp_max, int n_steps);
int idxtts_s2mel_cfm_rows(idxtts_ctx* ctx, const float* gen_cond, const int* target_lens, int Tg_max, const float* const* prompt_conditions,
                          const float* const* ref_mels, const int* prompt_lens, const float* style, const float* z, const float* t_emb,
                          const float* dt, int n_steps, float cfg_rate, float* out, int B, int T, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The mixed-prompt solve with an Euler schedule and a guidance rate PER ROW: a batch may hold rows of different quality tiers (say 8
 * and 25 steps, guidance 0 and 0.7).  Inputs, output and layout are idxtts_s2mel_cfm_rows' (rows of one speaker point at the same
 * tensors, so this entry serves single-prompt batches too).  The schedules:
 *   sched_steps  HOST int32 [n_sched], each >= 1: the step counts of the n_sched >= 1 distinct schedules;
 *   t_emb        device [sum of steps][256]: the schedules' timestep features one block after the other, in schedule order, each block
 *                exactly what idxtts_s2mel_cfm takes for that n_steps;   dt  HOST [sum of steps], concatenated the same way;
 *   row_sched    HOST int32 [B], each in [0, n_sched): row b's schedule;
 *   cfg_rates    HOST fp32 [B], finite and >= 0: row b's inference_cfg_rate.  NEGATIVE rates are refused here, whereas the reference
 *                treats them as 0 (flow_matching.py:87 tests `> 0`).
 * The library draws no timestep itself: the caller's tables define the schedules.  Row b with schedule d = row_sched[b], S_b =
 * sched_steps[d] steps and rate c_b: at iteration s < S_b the estimator evaluates the row with schedule d's step-s constants -- computed
 * per schedule by the launches a call of that schedule alone makes, so they are that call's values -- and
 *   c_b > 0:   x_b += dt[d][s] * ((1 + c_b) * v_cond - c_b * v_null)
 *   c_b == 0:  x_b += dt[d][s] * v_cond      (the reference's else-branch, flow_matching.py:105-106: no null evaluation of that row exists)
 * then x_b[..., :Tp_b] = 0.  From iteration S_b on the row is in no launch: iteration s runs on the rows with S_b > s, its null half on
 * those of them with c_b > 0 (a call whose rows all have c_b == 0 evaluates one half per step), all live rows of a half in ONE launch of
 * each kernel.  The two halves are two evaluations of their own, as under idxtts_s2mel_set_overlap(1) (and on two streams when it is on):
 * in the exact fp32 mode a row's result is bit-identical to idxtts_s2mel_cfm_rows on that row with its steps and rate (c_b > 0); in the
 * split-bf16 mode likewise while the row counts of the halves stay on the side of 256 rows the stacked batch is on.  The frames the
 * post-transformer part skips are taken once, from the shortest prompt of the whole batch.
 * Refused before anything is launched (idxtts_last_error names the cause; out is untouched): a null pointer; n_sched < 1 or a schedule with
 * fewer than 1 step; a row_sched entry out of range; a cfg_rates entry that is negative, NaN or infinite; everything
 * idxtts_s2mel_cfm_rows refuses; a workspace below idxtts_s2mel_cfm_sched_workspace_bytes(ctx, B, T, max_b Tp_b, n_sched, sched_steps)
 * (0 for arguments it refuses). */
size_t idxtts_s2mel_cfm_sched_workspace_bytes(const idxtts_ctx* ctx, int B, int T, int Tp_max, int n_sched, const int* sched_steps);
int idxtts_s2mel_cfm_sched(idxtts_ctx* ctx, const float* gen_cond, const int* target_lens, int Tg_max, const float* const* prompt_conditions,
                           const float* const* ref_mels, const int* prompt_lens, const float* style, const float* z, int n_sched,
                           const int* sched_steps, const float* t_emb, const float* dt, const int* row_sched, const float* cfg_rates,
                           float* out, int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* The noise `z` of either solve from a counter-based generator, one seed per utterance: row b's element (c, t) is a pure function of
 * (seeds[b], c, t) -- t counted from the row's column 0, prompt frames included -- whatever batch, padding, row position or stream it is
 * produced in, so a request's audio is reproducible alone and merged.  With idx = (c << 32) | t, in arithmetic mod 2^64:
 *   z = (seed ^ 0xD1B54A32D192ED03) + 0x9E3779B97F4A7C15 * (idx + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31;
 *   u1 = ((z >> 41) + 0.5) * 2^-23;  u2 = (((z >> 18) & 0x7FFFFF) + 0.5) * 2^-23;  n = sqrt(-2 ln u1) * cos(2 pi u2)
 * (23-bit uniforms: exact in fp32, never 0 or 1; the tail is cut at 5.77 sigma = 8e-9 of the mass per draw; the xor constant keeps
 * the stream apart from a sampler given the same seed).
 * z[b][c][t] = that draw for t < x_lens[b], 0.0f for x_lens[b] <= t < T.  seeds, x_lens: HOST [B].
 * z: device [B][C][T] fp32, any T >= max x_lens (rows need not be 16-byte aligned).  No workspace, no allocation,
 * no host-device copy, no synchronisation; seeds / x_lens may be reused as soon as the call returns.
 * Errors: a null pointer, B < 1, C < 1, T < 1 (or C * T beyond an int), an x_lens[b] outside 0..T. */
int idxtts_cfm_noise(const unsigned long long* seeds, const int* x_lens, int B, int C, int T, float* z, void* stream);

/* One evaluation of the CFM estimator = DiT.forward(x, prompt_x, x_lens, t, style, cond) (diffusion_transformer.py:186-257),
 * the function `cfm.inference` calls once per Euler step on the [cond | null] stack (flow_matching.py:96).  x [B][in_channels][T];
 * prompt [B][in_channels][Tp_max] with prompt_lens HOST [B] (prompt_x is zero beyond them); x_lens HOST [B]; t_emb device
 * [1][256] sinusoidal features of the (shared) timestep; style [B][style_dim]; mu [B][T][content_dim].
 * out: TOKEN-MAJOR [B][T][in_channels] (the reference returns [B][in_channels][T]).  Workspace: idxtts_s2mel_cfm_workspace_bytes(ctx, B, T, 1). */
int idxtts_s2mel_estimator(idxtts_ctx* ctx, const float* x, const float* prompt, const int* prompt_lens, int Tp_max, const int* x_lens,
                           const float* t_emb, const float* style, const float* mu, float* out, int B, int T, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- emotion-from-text classifier: Qwen3 causal LM, greedy generation for one prompt or a batch (reference: QwenEmotion.inference, infer_v2.py:948-1063:
 * AutoModelForCausalLM.from_pretrained(qwen_emo_path) + model.generate(max_new_tokens=32768) on a two-message chat prompt; third-party
 * model: transformers' Qwen3ForCausalLM) --------------------------------------------------------------------------------------
 * State-dict keys: the HF checkpoint's own -- "model.embed_tokens.weight", "model.layers.{i}.self_attn.{q,k,v,o}_proj.weight",
 * "model.layers.{i}.self_attn.{q,k}_norm.weight", "model.layers.{i}.mlp.{gate,up,down}_proj.weight",
 * "model.layers.{i}.{input,post_attention}_layernorm.weight", "model.norm.weight", "lm_head.weight" (required unless
 * tie_word_embeddings) -- plus the optional buffer "model.rotary_emb.inv_freq" [head_dim / 2] (absent: theta^(-2i/d) in fp32).
 * Arithmetic is fp32 throughout (the reference loads the model without a dtype). */
typedef struct idxtts_qwen_config {
  int vocab_size;                /* 151936 */
  int hidden_size;               /* 1024 */
  int intermediate_size;         /* 3072 */
  int num_hidden_layers;         /* 28 */
  int num_attention_heads;       /* 16 */
  int num_key_value_heads;       /* 8 */
  int head_dim;                  /* 128: the only value the kernels are built for, any other is refused */
  float rms_norm_eps;            /* 1e-6 */
  float rope_theta;              /* 1e6 */
  int tie_word_embeddings;       /* 1: the head reads model.embed_tokens.weight */
  int max_context;               /* prompt + generated tokens a call may reach (the rotary table's rows), e.g. 4096 */
} idxtts_qwen_config;
int idxtts_qwen_create(const idxtts_qwen_config* cfg, idxtts_ctx** out);
/* Storage of the linear weights and the embedding / head table (before idxtts_ctx_finalize): 0 = fp32 (default), 1 = bf16.  bf16 holds
 * a bf16 checkpoint widened to fp32 exactly and halves the bytes a token streams; finalize then FAILS, naming the first tensor, if a
 * weight is not on the bf16 grid (nothing is rounded).  Norm gains and the KV cache stay fp32.  Both formats give the same bits. */
int idxtts_qwen_set_weight_format(idxtts_ctx* ctx, int format);
size_t idxtts_qwen_workspace_bytes(const idxtts_ctx* ctx, int n_prompt, int max_new_tokens, int n_eos, int n_logit_cols /* 0 without out_logits; vocab_size for all columns */);
/* Prefill of prompt_ids (HOST int32 [n_prompt]) + greedy loop: out_ids (HOST int32 [max_new_tokens]) receives every step's argmax
 * (ties: the lowest id, as torch.argmax), *n_out the steps run; the loop ends after the step whose fed token is one of eos_ids (HOST
 * int32 [n_eos]; that token is the last entry) or at max_new_tokens.  forced_ids (HOST int32 [max_new_tokens], or NULL): the
 * teacher-forced parity instrument -- forced_ids[s] continues the sequence after step s (and is what ends it) while out_ids still
 * records the model's own choice.  out_logits (DEVICE fp32 [max_new_tokens][n], or NULL): the logits of every step that ran at the
 * columns logit_cols (HOST int32 [n_logit_cols], n = n_logit_cols), or at every column (logit_cols NULL, n = vocab_size).
 * use_graph: steps 2.. replay one captured hipGraph (kept for the next call with the same shapes on the same workspace); eager
 * launches and replay give the same bits.  The call returns after the stream has finished. */
int idxtts_qwen_generate(idxtts_ctx* ctx, const int* prompt_ids, int n_prompt, int max_new_tokens, const int* eos_ids, int n_eos,
                         const int* forced_ids /* may be NULL */, int* out_ids, int* n_out, float* out_logits /* may be NULL */,
                         const int* logit_cols /* may be NULL */, int n_logit_cols, void* workspace, size_t bytes, int use_graph,
                         void* stream);
/* Kernel launches in the kept decode-step graph (5 per layer + 2, + 1 with out_logits); -1 when no graph is held. */
int idxtts_qwen_step_graph_launches(const idxtts_ctx* ctx);
/* ---- batched generation: several prompts share every weight pass of a decode step (replaces B calls of idxtts_qwen_generate in series;
 * reference: QwenEmotion.inference once per text, infer_v2.py:1013-1063).  Row b of a batched call equals
 * idxtts_qwen_generate(prompt b, max_new_tokens[b], ...) bit for bit: ids, stop step and every logit, in both storage formats, eager or
 * replayed.  Rows the library passes through the weights together (replaces the fixed B = 1): a call with more rows is served in
 * consecutive tiles of this many inside the library. */
int idxtts_qwen_max_batch(const idxtts_ctx* ctx);
/* Workspace for a batched call (replaces idxtts_qwen_workspace_bytes; n_prompt, max_new_tokens: HOST int32 [B]); 0 on a bad shape
 * (B < 1, a null array, a length < 1). */
size_t idxtts_qwen_batch_workspace_bytes(const idxtts_ctx* ctx, int B, const int* n_prompt, const int* max_new_tokens, int n_eos,
                                         int n_logit_cols /* 0 without out_logits; vocab_size for all columns */);
/* idxtts_qwen_generate for B prompts (replaces B calls in series): prompt_ids HOST int32, the rows concatenated (n_prompt[b] each);
 * forced_ids / out_ids HOST int32, the rows concatenated by max_new_tokens[b]; n_out HOST int32 [B].  Every row stops at its own end id
 * (one of eos_ids, shared by the rows) or its own max_new_tokens[b].  out_logits (DEVICE fp32, or NULL): row b's steps start at row
 * (sum of max_new_tokens[0..b-1]) of a [sum max_new_tokens][n] matrix; rows of steps a row did not run are left untouched.
 * logit_cols / n_logit_cols / use_graph / stream: as idxtts_qwen_generate; the kept batched step graph is separate from the single one
 * and is reused by the next call with the same lengths on the same workspace.  Nothing runs when a row fails a check. */
int idxtts_qwen_generate_batch(idxtts_ctx* ctx, int B, const int* prompt_ids, const int* n_prompt, const int* max_new_tokens,
                               const int* eos_ids, int n_eos, const int* forced_ids /* may be NULL */, int* out_ids, int* n_out,
                               float* out_logits /* may be NULL */, const int* logit_cols /* may be NULL */, int n_logit_cols,
                               void* workspace, size_t bytes, int use_graph, void* stream);
/* Kernel launches in the kept batched decode-step graph (replaces idxtts_qwen_step_graph_launches: the same 5 per layer + 2, + 1 with
 * out_logits, whatever the rows); -1 when no graph is held.  A tile of one row runs idxtts_qwen_generate's path and its graph, not this one. */
int idxtts_qwen_batch_step_graph_launches(const idxtts_ctx* ctx);

/* ---- per-kernel timing for the benchmark's roofline report ------------------------------------------
 * When enabled, every kernel launch is bracketed by HIP events on its own stream and the library
 * accumulates, per kernel family, the launch count, elapsed milliseconds and the ALGORITHMIC flops /
 * bytes of the launches (DESIGN.md "work units").  Enabling resets the accumulators.  Not for use
 * inside a timed region (event records serialise nothing but add host work per launch). */
int idxtts_profile_enable(int on);
int idxtts_profile_num_kernels(void);
const char* idxtts_profile_kernel_name(int index);
int idxtts_profile_read(int index, double* total_ms, double* flops, double* bytes, long* launches);
/* Average reading of an event pair around one launch of an EMPTY 256-workgroup kernel on `stream`: the fixed per-launch cost
 * of this timing method (subtract launches * overhead before comparing kernel families by time). */
int idxtts_profile_event_overhead(void* stream, int launches, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* IDXTTS_H */
