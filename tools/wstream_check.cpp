// Host-side checks of the decode weight streams and of the two GEMVs' launch plans, as a stand-alone program (no GPU needed: nothing
// is launched).  It supplies idxtts::fail itself, so it can be built with a host sanitizer:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iindex-tts_amd/csrc tools/wstream_check.cpp \
//         index-tts_amd/csrc/{wstream,gemv_fx,gemv_pl,prof}.hip -o tools/wstream_check && tools/wstream_check
//  1. pack_wstream against a plain restatement of the lane rule (wstream.h), every byte and every fp8 scale, padding zero;
//  2. gemv_fx_make_plan against the plans written out below;  3. gemv_pl_plan / gemv_pl_slab_floats likewise (IDXTTS_PL_CT unset).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gemv16.h"
#include "gemv_pl.h"

namespace idxtts {
int fail(const char* file, int line, const std::string& msg) {
  std::printf("%s:%d: %s\n", file, line, msg.c_str());
  return 1;
}
}  // namespace idxtts
using namespace idxtts;

static int failures = 0;
static void expect(bool ok, const char* what, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0) {
  if (ok) return;
  if (++failures <= 20) std::printf("FAILED %s (%d %d %d %d %d)\n", what, a, b, c, d, e);
}

// ---- 1. the packer ----
// smallest power of two s with maxabs / s <= 448 (1 for an all-zero column)
static float scale_of(float maxabs) {
  float s = 1.0f;
  if (!(maxabs > 0.0f)) return s;
  while (maxabs / s > 448.0f) s *= 2.0f;
  while (maxabs / (s * 0.5f) <= 448.0f) s *= 0.5f;
  return s;
}

static void check_pack(int N, int K, bool kn, int fmt, int kdepth) {
  std::vector<float> w((size_t)N * K);
  auto at = [&](int k, int n) -> float& { return kn ? w[(size_t)k * N + n] : w[(size_t)n * K + k]; };
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      const float r = (std::rand() / (float)RAND_MAX - 0.5f) * 0.2f;
      at(k, n) = n % 7 == 3 ? 0.0f : r * (n % 5 == 1 ? 300.0f : 1.0f);      // all-zero columns, and a spread of column scales
    }
  quantize_matrix(w.data(), K, N, kn, fmt);
  const int per = kdepth / 4, KC = cdiv(K, kdepth), eb = wfmt_bytes(fmt);
  const size_t elems = wstream_elems(N, K, kdepth);
  expect(elems == (size_t)cdiv(N, 16) * KC * 64 * per, "wstream_elems", N, K, kdepth);
  std::vector<unsigned char> want(elems * eb, 0), got(elems * eb, 0xAA);
  std::vector<float> sc_want(N, 1.0f), sc_got(N, -1.0f);
  for (int n = 0; n < N; ++n) {
    float mx = 0.0f;
    for (int k = 0; k < K; ++k) mx = std::fmax(mx, std::fabs(at(k, n)));
    if (fmt == WFMT_FP8) sc_want[n] = scale_of(mx);
    for (int k = 0; k < K; ++k) {
      const int t = n / 16, c = k / kdepth, lane = (n % 16) + 16 * ((k % kdepth) / per), j = k % per;
      const size_t i = (((size_t)t * KC + c) * 64 + lane) * per + j;
      const float v = at(k, n);
      if (fmt == WFMT_F32) {
        std::memcpy(&want[i * 4], &v, 4);
      } else if (fmt == WFMT_BF16) {
        uint32_t u; std::memcpy(&u, &v, 4);
        const uint16_t h = (uint16_t)(u >> 16);
        std::memcpy(&want[i * 2], &h, 2);
      } else {
        int code = -1;      // the e4m3 code whose value times the column scale IS v
        for (int q = 0; q < 256 && code < 0; ++q) {
          const float dq = fp8_e4m3_decode((unsigned char)q);
          if (sc_want[n] * dq == v && std::signbit(dq) == std::signbit(v)) code = q;
        }
        expect(code >= 0, "quantised value has an fp8 code", N, K, n, k);
        want[i] = (unsigned char)code;
      }
    }
  }
  const int rc = pack_wstream(got.data(), w.data(), N, K, kn, fmt, kdepth, sc_got.data());
  expect(rc == 0, "pack_wstream accepts a quantised matrix", N, K, kn, fmt, kdepth);
  expect(std::memcmp(want.data(), got.data(), want.size()) == 0, "stream bytes", N, K, kn, fmt, kdepth);
  if (fmt == WFMT_FP8) expect(std::memcmp(sc_want.data(), sc_got.data(), (size_t)N * 4) == 0, "fp8 column scales", N, K, kn, fmt, kdepth);
  if (fmt == WFMT_FP8) expect(pack_wstream(got.data(), w.data(), N, K, kn, fmt, kdepth, nullptr) == 0, "scale_out may be null", N, K, kn);
  // one value the format cannot hold
  float& bad = at(K - 1, N - 1);
  bad = fmt == WFMT_FP8 ? 0.3f * sc_want[N - 1] : 1.0f + 1.0f / 1048576.0f;      // 0.3 is no e4m3 value; 1 + 2^-20 is no bf16 value
  const int rb = pack_wstream(got.data(), w.data(), N, K, kn, fmt, kdepth, sc_got.data());
  if (fmt == WFMT_FP8) {
    float mx = 0.0f;
    for (int k = 0; k < K; ++k) mx = std::fmax(mx, std::fabs(at(k, N - 1)));
    expect(scale_of(mx) == sc_want[N - 1], "the bad value leaves its column's scale alone", N, K, kn, fmt, kdepth);
    expect(rb == 1, "unrepresentable fp8 value refused", N, K, kn, fmt, kdepth);
  } else {
    expect(rb == (fmt == WFMT_BF16 ? 1 : 0), "unrepresentable bf16 value refused (fp32 holds anything)", N, K, kn, fmt, kdepth);
  }
}

// ---- 2. gemv_fx plans, as the launcher before FxPlan chose them (its plan function, its fix-ups and its launch table, run on these
//         shapes): the GPT's c_attn, c_proj, c_fc, mlp.c_proj and mel_head, a toy shape, and one with more than 5 chunks per wave ----
struct FxWant {
  int N, K, ksb, rows_lo, rows_hi;
  unsigned combos;      // bit (3 * narrow geometry + format) for which this plan holds
  struct { int MT, ntw, kw, cps, single, r4, narrow, threads; size_t lds; int grid_x, grid_y; } p;
};
static const FxWant fx_want[] = {
    {3840, 1280, 1,  1,  4, 0x3f, {1, 1, 16,  5, 1, 1, 0, 1024,  18560, 240, 1}},
    {3840, 1280, 1,  5, 16, 0x0f, {1, 1, 16,  5, 1, 0, 0, 1024,  18560, 240, 1}},
    {3840, 1280, 1,  5, 16, 0x30, {1, 1,  8, 10, 1, 0, 1,  512,   9344, 240, 1}},
    {3840, 1280, 1, 17, 32, 0x3f, {2, 1, 16,  5, 1, 0, 0, 1024,  37120, 240, 1}},
    {3840, 1280, 1, 33, 48, 0x3f, {3, 1, 16,  5, 1, 0, 0, 1024,  55680, 240, 1}},
    {3840, 1280, 1, 49, 64, 0x3f, {4, 1, 16,  5, 0, 0, 0, 1024,  74240, 240, 1}},
    {1280, 1280, 1,  1,  4, 0x3f, {1, 1, 16,  5, 1, 1, 0, 1024,  18560,  80, 1}},
    {1280, 1280, 1,  5, 16, 0x0f, {1, 1, 16,  5, 1, 0, 0, 1024,  18560,  80, 1}},
    {1280, 1280, 1,  5, 16, 0x30, {1, 1,  8, 10, 1, 0, 1,  512,   9344,  80, 1}},
    {1280, 1280, 1, 17, 32, 0x3f, {2, 1, 16,  5, 1, 0, 0, 1024,  37120,  80, 1}},
    {1280, 1280, 1, 33, 48, 0x3f, {3, 1, 16,  5, 1, 0, 0, 1024,  55680,  80, 1}},
    {1280, 1280, 1, 49, 64, 0x3f, {4, 1, 16,  5, 0, 0, 0, 1024,  74240,  80, 1}},
    {1280, 1280, 4,  1,  4, 0x3f, {1, 1, 16,  2, 1, 1, 0, 1024,  18560,  80, 4}},
    {1280, 1280, 4,  5, 16, 0x3f, {1, 1, 16,  2, 1, 0, 0, 1024,  18560,  80, 4}},
    {1280, 1280, 4, 17, 32, 0x3f, {2, 1, 16,  2, 1, 0, 0, 1024,  37120,  80, 4}},
    {1280, 1280, 4, 33, 48, 0x3f, {3, 1, 16,  2, 1, 0, 0, 1024,  55680,  80, 4}},
    {1280, 1280, 4, 49, 64, 0x3f, {4, 1, 16,  2, 0, 0, 0, 1024,  74240,  80, 4}},
    {5120, 1280, 1,  1,  4, 0x3f, {1, 2, 16,  5, 1, 1, 0, 1024,  34944, 160, 1}},
    {5120, 1280, 1,  5, 16, 0x0f, {1, 2, 16,  5, 1, 0, 0, 1024,  34944, 160, 1}},
    {5120, 1280, 1,  5, 16, 0x30, {1, 1,  8, 10, 1, 0, 1,  512,   9344, 320, 1}},
    {5120, 1280, 1, 17, 32, 0x3f, {2, 2, 16,  5, 1, 0, 0, 1024,  69888, 160, 1}},
    {5120, 1280, 1, 33, 48, 0x3f, {3, 1, 16,  5, 1, 0, 0, 1024,  55680, 320, 1}},
    {5120, 1280, 1, 49, 64, 0x3f, {4, 1, 16,  5, 0, 0, 0, 1024,  74240, 320, 1}},
    {1280, 5120, 1,  1,  4, 0x3f, {1, 1, 16, 20, 0, 1, 0, 1024,  18560,  80, 1}},
    {1280, 5120, 1,  5, 16, 0x3f, {1, 1, 16, 20, 0, 0, 0, 1024,  18560,  80, 1}},
    {1280, 5120, 1, 17, 32, 0x3f, {2, 1, 16, 20, 0, 0, 0, 1024,  37120,  80, 1}},
    {1280, 5120, 1, 33, 48, 0x3f, {3, 1, 16, 20, 0, 0, 0, 1024,  55680,  80, 1}},
    {1280, 5120, 1, 49, 64, 0x3f, {4, 1, 16, 20, 0, 0, 0, 1024,  74240,  80, 1}},
    {1280, 5120, 4,  1,  4, 0x3f, {1, 1, 16,  5, 1, 1, 0, 1024,  18560,  80, 4}},
    {1280, 5120, 4,  5, 16, 0x0f, {1, 1, 16,  5, 1, 0, 0, 1024,  18560,  80, 4}},
    {1280, 5120, 4,  5, 16, 0x30, {1, 1,  8, 10, 1, 0, 1,  512,   9344,  80, 4}},
    {1280, 5120, 4, 17, 32, 0x3f, {2, 1, 16,  5, 1, 0, 0, 1024,  37120,  80, 4}},
    {1280, 5120, 4, 33, 48, 0x3f, {3, 1, 16,  5, 1, 0, 0, 1024,  55680,  80, 4}},
    {1280, 5120, 4, 49, 64, 0x3f, {4, 1, 16,  5, 0, 0, 0, 1024,  74240,  80, 4}},
    {8194, 1280, 1,  1,  4, 0x3f, {1, 1, 16,  5, 1, 1, 0, 1024,  18560, 513, 1}},
    {8194, 1280, 1,  5, 16, 0x0f, {1, 1, 16,  5, 1, 0, 0, 1024,  18560, 513, 1}},
    {8194, 1280, 1,  5, 16, 0x30, {1, 1,  8, 10, 1, 0, 1,  512,   9344, 513, 1}},
    {8194, 1280, 1, 17, 32, 0x3f, {2, 1, 16,  5, 1, 0, 0, 1024,  37120, 513, 1}},
    {8194, 1280, 1, 33, 48, 0x3f, {3, 1, 16,  5, 1, 0, 0, 1024,  55680, 513, 1}},
    {8194, 1280, 1, 49, 64, 0x3f, {4, 1, 16,  5, 0, 0, 0, 1024,  74240, 513, 1}},
    { 384,  128, 1,  1,  4, 0x3f, {1, 1,  8,  1, 1, 1, 0,  512,   9344,  24, 1}},
    { 384,  128, 1,  5, 16, 0x3f, {1, 1,  8,  1, 1, 0, 0,  512,   9344,  24, 1}},
    { 384,  128, 1, 17, 32, 0x3f, {2, 1,  8,  1, 1, 0, 0,  512,  18688,  24, 1}},
    { 384,  128, 1, 33, 48, 0x3f, {3, 1,  8,  1, 1, 0, 0,  768,  28032,  24, 1}},
    { 384,  128, 1, 49, 64, 0x3f, {4, 1,  8,  1, 0, 0, 0, 1024,  37376,  24, 1}},
    {4096, 2048, 1,  1,  4, 0x3f, {1, 1, 16,  8, 0, 1, 0, 1024,  18560, 256, 1}},
    {4096, 2048, 1,  5, 16, 0x3f, {1, 1, 16,  8, 0, 0, 0, 1024,  18560, 256, 1}},
    {4096, 2048, 1, 17, 32, 0x3f, {2, 1, 16,  8, 0, 0, 0, 1024,  37120, 256, 1}},
    {4096, 2048, 1, 33, 48, 0x3f, {3, 1, 16,  8, 0, 0, 0, 1024,  55680, 256, 1}},
    {4096, 2048, 1, 49, 64, 0x3f, {4, 1, 16,  8, 0, 0, 0, 1024,  74240, 256, 1}},
};
static const int plan_rows[10] = {1, 4, 5, 16, 17, 32, 33, 48, 49, 64};

static void check_fx_plans() {
  const int shapes[][3] = {{3840, 1280, 1}, {1280, 1280, 4}, {5120, 1280, 1}, {1280, 5120, 4}, {8194, 1280, 1}, {384, 128, 1}, {4096, 2048, 1}};      // N, K, gemv_fx_ksb
  for (const auto& sh : shapes) {
    const int N = sh[0], K = sh[1];
    expect(gemv_fx_ksb(N, K) == sh[2], "gemv_fx_ksb", N, K);
    for (int ksb : {1, sh[2]})
      for (int rows : plan_rows)
        for (int fmt : {WFMT_F32, WFMT_BF16, WFMT_FP8})
          for (int geom = 0; geom < 2; ++geom) {
            int found = 0;
            const FxPlan pl = gemv_fx_make_plan(N, K, rows, fmt, ksb, geom != 0);
            for (const FxWant& e : fx_want) {
              if (e.N != N || e.K != K || e.ksb != ksb || rows < e.rows_lo || rows > e.rows_hi || !(e.combos >> (3 * geom + fmt) & 1)) continue;
              ++found;
              expect(pl.MT == e.p.MT && pl.ntw == e.p.ntw && pl.kw == e.p.kw && pl.cps == e.p.cps && pl.single == (e.p.single != 0) &&
                         pl.r4 == (e.p.r4 != 0) && pl.narrow == (e.p.narrow != 0) && pl.threads == e.p.threads && pl.lds == e.p.lds &&
                         pl.grid_x == e.p.grid_x && pl.grid_y == e.p.grid_y,
                     "gemv_fx plan", N, K, rows, fmt, 10 * ksb + geom);
            }
            expect(found == 1, "one expected gemv_fx plan per case", N, K, rows, fmt, 10 * ksb + geom);
          }
  }
}

// ---- 3. gemv_pl plans: {column tiles per workgroup, K parts, slab floats} at plan_rows ----
struct PlWant { int N, K; struct { int ct, kparts; size_t slab; } r[10]; };
static const PlWant pl_want[] = {
    {3840, 1280, {{4,  4,  245760}, {4,  4,  245760}, {4,  4,  245760}, {4,  4,  245760}, {4,  4,  491520}, {4,  4,  491520}, {4,  4,  737280}, {4,  4,  737280}, {8,  8, 1966080}, {8,  8, 1966080}}},
    {1280, 1280, {{4,  4,   81920}, {4,  4,   81920}, {4,  4,   81920}, {4,  4,   81920}, {4,  4,  163840}, {4,  4,  163840}, {4,  4,  245760}, {4,  4,  245760}, {8,  8,  655360}, {8,  8,  655360}}},
    {5120, 1280, {{4,  4,  327680}, {4,  4,  327680}, {4,  4,  327680}, {4,  4,  327680}, {4,  4,  655360}, {4,  4,  655360}, {8,  8, 1966080}, {8,  8, 1966080}, {8,  8, 2621440}, {8,  8, 2621440}}},
    {1280, 5120, {{4, 16,  327680}, {4, 16,  327680}, {4, 16,  327680}, {4, 16,  327680}, {4, 16,  655360}, {4, 16,  655360}, {4, 16,  983040}, {4, 16,  983040}, {8, 32, 2621440}, {8, 32, 2621440}}},
    {8194, 1280, {{4,  4,  525312}, {4,  4,  525312}, {4,  4,  525312}, {4,  4,  525312}, {8,  8, 2101248}, {8,  8, 2101248}, {8,  8, 3151872}, {8,  8, 3151872}, {8,  8, 4202496}, {8,  8, 4202496}}},
    { 384,  128, {{4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {4,  1,       0}, {8,  1,       0}, {8,  1,       0}}},
    {4096, 2048, {{4,  7,  458752}, {4,  7,  458752}, {4,  7,  458752}, {4,  7,  458752}, {4,  7,  917504}, {4,  7,  917504}, {8, 13, 2555904}, {8, 13, 2555904}, {8, 13, 3407872}, {8, 13, 3407872}}},
};

static void check_pl_plans() {
  for (const PlWant& e : pl_want)
    for (int i = 0; i < 10; ++i) {
      int ct = 0, kparts = 0;
      gemv_pl_plan(e.N, e.K, plan_rows[i], &ct, &kparts);
      expect(ct == e.r[i].ct && kparts == e.r[i].kparts, "gemv_pl plan", e.N, e.K, plan_rows[i], ct, kparts);
      expect(gemv_pl_slab_floats(e.N, e.K, plan_rows[i]) == e.r[i].slab, "gemv_pl slab", e.N, e.K, plan_rows[i]);
    }
}

int main() {
  std::srand(3);
  const int shapes[][2] = {{16, 16}, {33, 48}, {129, 64}, {110, 160}, {40, 96}};      // N, K
  int packs = 0;
  for (const auto& sh : shapes)
    for (int kn = 0; kn < 2; ++kn)
      for (int fmt : {WFMT_F32, WFMT_BF16, WFMT_FP8})
        for (int kdepth : {16, 32}) { check_pack(sh[0], sh[1], kn != 0, fmt, kdepth); ++packs; }
  unsigned char one[64 * 16];
  const float v = 1.0f;
  expect(pack_wstream(one, &v, 1, 1, true, WFMT_F32, 8, nullptr) == 1, "kdepth other than 16 / 32 refused");
  expect(pack_wstream(one, &v, 1, 1, true, 3, 16, nullptr) == 1, "unknown format refused");
  check_fx_plans();
  check_pl_plans();
  if (failures) std::printf("FAILED: %d\n", failures);
  else std::printf("%d packs, %zu gemv_fx plans, %zu gemv_pl shapes: all as expected\n", packs, sizeof(fx_want) / sizeof(fx_want[0]), sizeof(pl_want) / sizeof(pl_want[0]));
  return failures ? 1 : 0;
}
