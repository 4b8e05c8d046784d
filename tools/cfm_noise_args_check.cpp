// Host-side argument checking of idxtts_cfm_noise, as a stand-alone program (no GPU needed: every call below is refused before a
// launch).  It links csrc/cfm_noise.hip alone and supplies the two error hooks of capi.hip itself, so it can be built with a host
// sanitizer:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/cfm_noise_args_check.cpp \
//         index-tts_amd/csrc/cfm_noise.hip -o tools/cfm_noise_args_check && tools/cfm_noise_args_check
#include <cstdio>
#include <string>

#include "../include/idxtts.h"

namespace idxtts {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
int fail(const char* file, int line, const std::string& msg) {
  g_error = std::string(file) + ":" + std::to_string(line) + ": " + msg;
  return 1;
}
}  // namespace idxtts

static int failures = 0;

static void refused(const char* what, int rc) {
  const bool ok = rc != 0 && !idxtts::g_error.empty();
  std::printf("%-28s rc=%d  %s\n", what, rc, ok ? idxtts::g_error.c_str() : "NOT REFUSED");
  if (!ok) ++failures;
  idxtts::g_error.clear();
}

int main() {
  unsigned long long seeds[40] = {};
  int lens[40] = {};
  float* z = reinterpret_cast<float*>(0x1000);      // never dereferenced on the host, and no launch happens
  refused("null seeds", idxtts_cfm_noise(nullptr, lens, 1, 80, 8, z, nullptr));
  refused("null x_lens", idxtts_cfm_noise(seeds, nullptr, 1, 80, 8, z, nullptr));
  refused("null z", idxtts_cfm_noise(seeds, lens, 1, 80, 8, nullptr, nullptr));
  refused("B = 0", idxtts_cfm_noise(seeds, lens, 0, 80, 8, z, nullptr));
  refused("B < 0", idxtts_cfm_noise(seeds, lens, -3, 80, 8, z, nullptr));
  refused("C = 0", idxtts_cfm_noise(seeds, lens, 1, 0, 8, z, nullptr));
  refused("C * T > INT_MAX", idxtts_cfm_noise(seeds, lens, 1, 65536, 32768, z, nullptr));
  refused("T = 0", idxtts_cfm_noise(seeds, lens, 1, 80, 0, z, nullptr));
  lens[39] = 9;
  refused("x_lens[39] > T", idxtts_cfm_noise(seeds, lens, 40, 80, 8, z, nullptr));
  lens[39] = -1;
  refused("x_lens[39] < 0", idxtts_cfm_noise(seeds, lens, 40, 80, 8, z, nullptr));
  refused("misaligned z", idxtts_cfm_noise(seeds, lens, 1, 80, 8, reinterpret_cast<float*>(0x1002), nullptr));
  if (failures) std::printf("FAILED: %d\n", failures);
  else std::printf("all refused\n");
  return failures ? 1 : 0;
}
