// Host side of a channels-first convolution launch, shared by the fp32 kernel (conv1d.hip) and the bf16 kernels (conv1d_bf16x3.hip):
// the checks, the parameters every kernel and conv_epilogue read, the tile grid, and what the profiler is told.  Header-only:
// conv1d_bf16x3.hip links without conv1d.hip (tools/gemv_stress.hip).
#pragma once
#include <string>
#include "conv1d.h"

namespace idxtts {

struct ConvGrid { int mblocks; unsigned blocks; };      // row blocks; workgroups = 8 XCDs x row blocks x time tiles per XCD

// Checks the launch and fills, for a BM x BN tile, *g and the fields that both kernels' parameter structs (ConvKP, ConvKP16) carry
// under the same names.  (Two structs, no common base: the kernels keep the argument layouts they were tuned with -- a base moved
// fields, and with them the kernels' scalar register counts.)
template <class P>
static inline int conv_launch_setup(const ConvWeights& w, const ConvArgs& a, int BM, int BN, P* p, ConvGrid* g) {
  IDX_CHECK(a.x && a.y, "null pointer");
  p->x = a.x; p->bias = w.bias; p->res = a.res; p->y = a.y;
  p->Cin = w.Cin; p->M = w.M; p->T = a.T;
  p->K = w.K; p->dil = a.dil; p->pad_left = a.pad_left; p->pad_mode = a.pad_mode;
  p->nchunk = w.nchunk; p->mt32 = cdiv(w.M, CONV_MT);
  int ul = 0;
  while ((1 << ul) < w.ups) ++ul;
  IDX_CHECK((1 << ul) == w.ups, "transposed-conv stride must be a power of two");
  p->ups_log2 = ul;
  const int halo = (w.K - 1) * a.dil;
  IDX_CHECK(halo <= CONV_MAX_HALO, "(K-1)*dil exceeds CONV_MAX_HALO");
  p->xt = BN + halo;
  p->ntiles_row = cdiv(a.T, BN);
  p->ntiles = p->ntiles_row * a.B;
  p->nt8 = cdiv(p->ntiles, 8);
  p->scale = a.scale; p->accum = a.accum; p->lens = a.lens; p->len_mul_out = a.len_mul_out;
  g->mblocks = cdiv(w.M, BM);
  const int64_t blocks = (int64_t)8 * g->mblocks * p->nt8;
  IDX_CHECK(blocks > 0 && blocks < (1ll << 31), "grid size");
  g->blocks = (unsigned)blocks;
  return 0;
}

// algorithmic work: 2*Cout*Cin*taps per output sample (a transposed conv has Kt/u = 2 live taps per output, not the 3 the
// packed form multiplies); bytes = x + y (+ residual / accumulate) + weights once
static inline void conv_work(const ConvWeights& w, const ConvArgs& a, double* flops, double* bytes) {
  const double cout = (double)(w.M / w.ups), tout = (double)a.T * w.ups * a.B;
  const double taps = w.ups > 1 ? 2.0 : (double)w.K;
  *flops = 2.0 * cout * w.Cin * taps * tout;
  *bytes = 4.0 * ((double)a.B * w.Cin * a.T + cout * tout * (1.0 + (a.res ? 1.0 : 0.0) + (a.accum ? 1.0 : 0.0)) +
                  cout * w.Cin * (w.ups > 1 ? 2.0 * w.ups : (double)w.K));
}

// profiler category (prof.h): the kernel instance as rocprofv3 prints it; `tail`: its template arguments behind the tile's
template <class Tile>
static inline std::string conv_category(const char* kernel, const char* tail = "") {
  return std::string(kernel) + "<" + std::to_string(Tile::TM) + ", " + std::to_string(Tile::TN) + ", " + std::to_string(Tile::WGM) + ", " +
         std::to_string(Tile::WGN) + tail + ">";
}

}  // namespace idxtts
