#pragma once
#include "wstream.h"

namespace idxtts {

// Decode GEMV (gemv_fx.hip) on a weight stream of kdepth 16: activations as A-fragment images (frag_index, common.h), K split
// across the waves of one workgroup, LayerNorm folded into the weights + epilogue, bias / gelu_new / residual epilogue, final
// output (no combine launch).
struct GemvFXArgs {
  const float* xf = nullptr; int rows = 0;        // fragment images [ceil(rows/16)][ceil(K/16)][64][4], padding rows/k zero
  const float* bias = nullptr;                    // [N]; folded layers: c = ln_b . W + bias
  const float* colsum = nullptr; float ln_eps = 1e-5f;   // folded layers: colsum(diag(ln_g) W); weights = diag(ln_g) W
  int act = 0;                                    // 0 none, 1 gelu_new
  const float* res = nullptr;                     // residual in the layout of y (may alias y)
  float* y = nullptr; int y_frag = 0; int ldy = 0;   // y_frag: fragment images over N, else row-major [rows][ldy]
  float* slab = nullptr;                          // Both given: a shape with gemv_fx_ksb(N, K) > 1 also splits K across that many
  unsigned* ksb_counters = nullptr;               // workgroups per column tile (slab [ksb][rows][N]); the LAST of them to arrive adds
                                                  // the partial sums in slab order (fixed, whoever is last) and runs the normal
                                                  // epilogue into y; counters [ceil(N/16)] start at 0 and are left at 0
  int invariant = 0;                              // batch-invariant mode: one summation order per (N, K, format) for 1..64 rows (below)
  int dbg = 0;                                    // ablation mask for tools/gemv_probe.hip only
};
int gemv_fx_ksb(int N, int K);
// 0 (default): 16 waves x 5 chunks (1024 threads, 256 registers per SIMD); 1: the narrow form, 8 waves x 10 chunks (512 threads, <= 176
// registers per SIMD: what ONE retiring workgroup of the acoustic stage's kernels frees on a CU) for 5..16 rows on bf16 / fp8 streams.
// The two forms split K differently, so their results differ in the last bits: a process-wide choice, made before generating.
void set_decode_geometry(int narrow);
int get_decode_geometry();

// The launch geometry of one gemv_fx_forward: which instantiation of the kernel runs, and on what grid.
struct FxPlan {
  int MT, ntw;        // row tiles; column tiles per wave
  int kw, cps;        // K slices (waves) per workgroup; 16-k chunks per slice
  bool single;        // the one-batch kernel: a wave's whole K-slice in one register batch
  bool r4;            // <= 4 rows: the 16-block 4x4x1 MFMA
  bool narrow;        // 8 waves x 10 chunks in one batch (set_decode_geometry)
  int threads;
  size_t lds;
  int grid_x, grid_y; // column-tile groups; K pieces across workgroups (ksb)
};
// invariant: only the forms that sum a row's products in ONE order -- the 16x16x4 MFMA over the wave's chunks in turn, the K-slices
// in wave order, the K pieces in slab order: the one-batch and two-buffer kernels at every MT and ntw.  The 4-row form (its 4x4x1
// MFMA adds four k-groups by shuffles) and the narrow geometry (8 slices instead of 16) sum otherwise and are left out; kw, cps and
// ksb follow (N, K) alone, so a row's bits do not depend on how many rows the launch has.
FxPlan gemv_fx_make_plan(int N, int K, int rows, int fmt, int ksb, bool narrow_geom, bool invariant = false);
int gemv_fx_forward(const WeightStream& w, const GemvFXArgs& a, hipStream_t stream);

}  // namespace idxtts
