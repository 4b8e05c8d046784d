// Host-side check of the CFM solver's buffer table (index-tts_amd/csrc/s2mel_buffers.h), as a stand-alone program (no GPU needed:
// pointer arithmetic on a host allocation, nothing is launched), so it can be built with a host sanitizer:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iindex-tts_amd/csrc tools/s2mel_buffers_check.cpp \
//         -o tools/s2mel_buffers_check && tools/s2mel_buffers_check
// For S2MelConfig.tiny()'s and the full-size dimensions at (B, T, n_steps) = (1, 127, 3), (3, 200, 3), (16, 1200, 20):
//  1. carve_cfm's byte total against the literals below: the totals of the carve_cfm this table replaced (34 hand-written takes),
//     from a scratch program holding that function; the tiny ones are also what idxtts_s2mel_cfm_workspace_bytes returned;
//  2. every halved entry: half_view(0) is the stacked pointer, half_view(1) lies one half's block (B*T*cols elements, B ints) on;
//  3. every shared entry: both views are the stacked pointer;
//  4. the buffers follow each other without overlap, each 256-byte aligned, the last one ending inside the byte total.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s2mel_buffers.h"

using namespace idxtts;

static int failures = 0;
static void expect(bool ok, const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
  if (ok) return;
  if (++failures <= 20) std::printf("FAILED %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

struct Entry { const char* p; size_t cols; CfmKind kind; bool halved; };
static std::vector<Entry> entries(CfmBuffers& b, const idxtts_s2mel_config& c, int ffn) {
  std::vector<Entry> e;
  cfm_buffer_table(b, c, ffn, [&](auto*& p, size_t cols, CfmKind kind, bool halved) {
    e.push_back({reinterpret_cast<const char*>(p), cols, kind, halved});
  });
  return e;
}

struct Want { int B, T, n_steps; size_t bytes; };

static int check(const char* name, const idxtts_s2mel_config& c, int ffn, const Want& s) {
  const size_t bytes = carve_cfm(c, ffn, nullptr, s.B, s.T, s.n_steps).bytes;
  expect(bytes == s.bytes, "workspace bytes", s.B, s.T, (long)bytes, (long)s.bytes);
  // nothing is read or written through the pointers: the allocation only makes them real addresses for the sanitizer
  void* ws = std::aligned_alloc(256, bytes);
  CfmBuffers w = carve_cfm(c, ffn, ws, s.B, s.T, s.n_steps);
  CfmBuffers v0 = half_view(c, ffn, w, 0, s.B, s.T), v1 = half_view(c, ffn, w, 1, s.B, s.T);
  const std::vector<Entry> e = entries(w, c, ffn), e0 = entries(v0, c, ffn), e1 = entries(v1, c, ffn);
  const size_t n = 22 + 2 * (size_t)(c.depth / 2) + 7 + 3;      // 22 activation buffers, two per skip, 7 per-step constants, 3 int arrays
  expect(e.size() == n && e0.size() == n && e1.size() == n, "entries", (long)e.size(), (long)n);
  expect(w.bytes == bytes && v0.bytes == bytes && v0.tail_t0 == w.tail_t0, "views keep bytes / tail_t0");
  int halved = 0;
  const char* end = static_cast<const char*>(ws);
  for (size_t i = 0; i < e.size(); ++i) {
    const size_t block = 4 * cfm_block_elems(s.B, s.T, s.n_steps, e[i].kind, e[i].cols);      // 4 bytes per element of every kind
    expect(e0[i].p == e[i].p, "half 0 is the stacked pointer", (long)i);
    expect(e1[i].p == e[i].p + (e[i].halved ? block : 0), e[i].halved ? "half 1 lies one block on" : "a shared buffer is not moved", (long)i);
    expect(e[i].kind != CFM_STEPS || !e[i].halved, "per-step constants are shared", (long)i);
    expect(e[i].p >= end && e[i].p - end < 256 && ((uintptr_t)e[i].p & 255) == 0, "follows its predecessor, 256-byte aligned", (long)i);
    end = e[i].p + (e[i].halved ? 2 : 1) * block;
    halved += e[i].halved;
  }
  expect(end <= static_cast<const char*>(ws) + bytes && (size_t)(static_cast<const char*>(ws) + bytes - end) < 256, "the total ends the last buffer");
  expect(halved == (int)n - 10, "halved entries: all but condp, xstate, plen and the 7 per-step constants", halved);
  // the shared ones by name
  expect(v1.condp == w.condp && v1.xstate == w.xstate && v1.plen == w.plen && v1.mods == w.mods && v1.wnb == w.wnb, "shared by name");
  expect(v1.lens2 == w.lens2 + s.B && v1.lens2t == w.lens2t + s.B && v1.vout == w.vout + (size_t)s.B * s.T * c.in_channels, "halved by name");
  std::free(ws);
  std::printf("%s B = %d T = %d n_steps = %d: %zu bytes, %zu buffers, %d halved\n", name, s.B, s.T, s.n_steps, bytes, e.size(), halved);
  return 0;
}

int main() {
  idxtts_s2mel_config tiny{}, full{};      // S2MelConfig.tiny() and the defaults (indextts_amd/config.py); ffn = S2MelConfig.ffn_dim
  tiny.hidden_dim = 128; tiny.num_heads = 2; tiny.depth = 5; tiny.in_channels = 16; tiny.content_dim = 64; tiny.style_dim = 24;
  tiny.wn_hidden = 128; tiny.wn_layers = 3; tiny.wn_kernel = 5; tiny.wn_dilation_rate = 1;
  full.hidden_dim = 512; full.num_heads = 8; full.depth = 13; full.in_channels = 80; full.content_dim = 512; full.style_dim = 192;
  full.wn_hidden = 512; full.wn_layers = 8; full.wn_kernel = 5; full.wn_dilation_rate = 1;
  const Want tiny_want[] = {{1, 127, 3, 4231168}, {3, 200, 3, 19790592}, {16, 1200, 20, 631952128}};
  const Want full_want[] = {{1, 127, 3, 20454656}, {3, 200, 3, 94893312}, {16, 1200, 20, 3024732928}};
  for (const Want& s : tiny_want) check("tiny", tiny, 512, s);
  for (const Want& s : full_want) check("full", full, 1536, s);
  if (failures) std::printf("FAILED: %d\n", failures);
  else std::printf("6 workspaces: all as expected\n");
  return failures ? 1 : 0;
}
