// ec_netgen.h -- the source generator of the run-time compiled networks (ec_netgen.cpp): pure
// functions from a matrix to HIP text, over the C++ standard library alone.  ec_jit.cpp compiles
// and launches what they emit; tools/jit_src.cpp prints it.  Internal to liblstore_ec.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace lsec {
namespace jit {

constexpr int kMaxRows = 8;   // output rows one network computes
constexpr int kMaxCols = 32;  // input columns (registers: 8 slices per input per lane)

// LSEC_JIT=0: no networks
bool jit_on();
// whether an R x K bytewise matrix is served by a network (wide codes only; LSEC_JIT=0: never)
bool wants_xornet(int R, int K);
// whether an R x K GF(2^w) matrix (w = 16 / 32, word layout) is served by a network
bool wants_gfw_net(int R, int K, int w);
// whether an R-output bitmatrix code over K inputs at w is served by a packet network
bool wants_pktnet(int R, int K, int w);

// LSEC_JIT_VARIANT (code shape knobs for A/B runs; 0 = default), raw and decoded.  Round 2
// measured the w = 8 shapes on RS(20+6) encode within 70.6-74.3 % of 8 TB/s
// (profiles/r02_v15_jit_ab.txt); round 4 capped pairs (r04_v15_xornet_ab.txt); the w = 16 / 32
// knobs: profiles/r04_v7_gfw_w32_ab.md, r04_v9_gfw_w32_split.txt.
int jit_variant();
struct Variant {
  bool pairs_uncapped;    // bit 0      w = 8: uncapped common-pair elimination (default: capped by registers, xornet_source)
  bool doubling_by_sub;   // bit 1      w = 8: doubling by shift-and-subtract instead of a packed 16-bit multiply
  bool pairs_off;         // bit 3      w = 8: no common-pair elimination (the round-3 form)
  int dwords;             // bits 4-7   w = 8: dwords per lane (1, 2, 4; else xornet_dwords chooses)
  int slice_pair_cap;     // bits 8-15  w = 16 / 32 and packets: most shared pairs per input (0: the default 32, 255: none), decoded
  bool unfenced;          // bit 16     one wave: loads left to the compiler's scheduler (gfw_source)
  int ahead;              // bits 17-18 one wave: inputs loaded ahead of their use (0: the default 1)
  bool split_off;         // bit 19     no wave-pair split (gfw_rowsplit)
  bool split_no_prefetch; // bit 20     split: each step loads its own input at its top
  bool fold_flip;         // bit 21     the other XOR fold: serial in the one-wave form (default trees), trees in the split (default serial)
  int split_waves;        // bits 22-23 split: occupancy target (0: by rows, 1 none, 2 four, 3 two)
  bool split_w16_off;     // bit 24     no split at w = 16
  int pkt_groups;         // bits 25-26 packets: 1 / 2 / 4 output groups (0: one)
  bool cauchy8_pkt_off;   // bit 27     Cauchy w = 8 stays off the packet networks (bind_pkt_field)
  bool reload_on;         // bit 28     shard table re-read from the kernarg segment in every tile (default: from 24 shards)
  bool reload_off;        // bit 30     ... never
};
const Variant &variant();

// HIP source of the network for the row-major R x K matrix (exposed for tests and tools)
std::string xornet_source(const uint8_t *mat, int R, int K);
// HIP source of the bit-sliced network for an R x K GF(2^w) matrix, w = 16 / 32
std::string gfw_source(const uint32_t *mat, int R, int K, int w);
// HIP source of the packet network for bitmatrix row masks [(r*w + l)*K + j] (w <= 32), D dwords
// per lane (exposed for tests and tools)
std::string pktnet_source(const uint32_t *masks, int R, int K, int w, int D, int S = 1);
// bytes of a shard one block of an R-row w = 16 / 32 network covers per tile; it serves whole
// tiles only
int gfw_tile(int w, int R);
// whether the R-row network at w takes the wave-pair slice split (4 rows at w = 32; ec_netgen.cpp)
bool gfw_rowsplit(int w, int R);
// bytes of a shard one 256-lane block of the network covers per tile
int xornet_tile(int K, int R);
int xornet_dwords(int R, int K);
// lane width (dwords, 0: none) and output groups of the packet network for R outputs at w
void pkt_shape(int R, int w, int packet, int *D, int *S);
// c * x in GF(2^w), w = 8 / 16 / 32
uint32_t gfw_times_x(uint32_t c, int w);
// the bitmatrix row masks [(r*w + l)*K + j] of an R x K GF(2^w) coefficient matrix (w = 8 / 16 / 32)
std::vector<uint32_t> coef_masks(const uint32_t *coef, int R, int K, int w);

// One network: what the generator emits for it and what the launcher must know of it, so that
// the source's tile constant and the launch's tile count come from the same expression.
struct Net {
  enum Kind { kXor, kGfw, kPkt } kind;  // w = 8 XOR network, w = 16 / 32 bit-sliced, packet network
  int R, K, w;
  int D, S;  // packet networks: dwords per lane per packet (0: no network) and output groups
  static Net matrix(int R, int K, int w) { return {w == 8 ? kXor : kGfw, R, K, w, 0, 1}; }
  static Net packets(int R, int K, int w, int packet) {
    Net n{kPkt, R, K, w, 0, 1};
    pkt_shape(R, w, packet, &n.D, &n.S);
    return n;
  }
  // words of its matrix: R x K coefficients, or one mask word per (bit-row, input)
  size_t words() const { return static_cast<size_t>(R) * K * (kind == kPkt ? w : 1); }
  std::string source(const uint32_t *mat) const;
  // the identity of its source: shape and matrix
  std::vector<uint32_t> key(const uint32_t *mat) const;
  // bytes of a shard (packet networks: column bytes) a block covers per tile
  int tile_bytes() const;
  // tiles of a stripe of `size` bytes per shard: every byte at w = 8 and in packets, whole tiles
  // only at w = 16 / 32
  uint64_t tiles_per_stripe(int64_t size) const;
};

}  // namespace jit
}  // namespace lsec
