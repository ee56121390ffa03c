// Print the network source ec_netgen.cpp generates for a matrix read from stdin, so it can be
// compiled offline (hipcc -c, resource usage) or compared between trees (tools/jit_sources.py):
//   "R K W" then R*K coefficients (W = 8, 16 or 32): the XOR / bit-sliced network;
//   "P R K W packet" then the R*W*K row masks [(r*W + l)*K + j] (W <= 32): the packet network,
//   its lane width and output groups from pkt_shape as bind_pkt takes them.
// Built by `make jit_src` in lstore_amd/csrc from this file and ec_netgen.cpp alone.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lstore_amd/csrc/ec_netgen.h"

static bool read_words(std::vector<uint32_t> &m) {
  for (auto &c : m) {
    unsigned long v = 0;
    if (scanf("%lu", &v) != 1) return false;
    c = static_cast<uint32_t>(v);
  }
  return true;
}

int main() {
  char first[16];
  if (scanf("%15s", first) != 1) return 2;
  if (!strcmp(first, "P")) {
    int R = 0, K = 0, W = 0, packet = 0, D = 0, S = 1;
    if (scanf("%d %d %d %d", &R, &K, &W, &packet) != 4 || R < 1 || K < 1 || W < 2 || W > 32) return 2;
    std::vector<uint32_t> masks(static_cast<size_t>(R) * W * K);
    if (!read_words(masks)) return 2;
    lsec::jit::pkt_shape(R, W, packet, &D, &S);
    if (D == 0) return 2;
    fputs(lsec::jit::pktnet_source(masks.data(), R, K, W, D, S).c_str(), stdout);
    return 0;
  }
  int R = 0, K = 0, W = 0;
  if (sscanf(first, "%d", &R) != 1 || scanf("%d %d", &K, &W) != 2 || R < 1 || K < 1 || (W != 8 && W != 16 && W != 32)) return 2;
  std::vector<uint32_t> m(static_cast<size_t>(R) * K);
  if (!read_words(m)) return 2;
  if (W == 8) {
    std::vector<uint8_t> m8(m.begin(), m.end());
    fputs(lsec::jit::xornet_source(m8.data(), R, K).c_str(), stdout);
  } else {
    fputs(lsec::jit::gfw_source(m.data(), R, K, W).c_str(), stdout);
  }
  return 0;
}
