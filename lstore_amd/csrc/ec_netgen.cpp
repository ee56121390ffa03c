// ec_netgen.cpp -- the source of the per-matrix networks that ec_jit.cpp compiles at run time
// with hipRTC for gfx950 and launches.
//
// The bytewise kernel (ec_kernels_impl.h) multiplies by a coefficient with three v_perm_b32
// table lookups per 4 bytes, about 5 VALU ops per (output, input) pair and dword.  Wide codes
// are VALU-bound that way: RS(20+6) encode ran at 0.61-0.65 of 8 TB/s, 97 % VALU-busy
// (DESIGN.md §3).  With the matrix known when the kernel is compiled, output r is a fixed
// network evaluated in Horner form over the coefficient bits,
//     out_r = x(...x(x S_r7 + S_r6)...) + S_r0,   S_rt = XOR of the inputs j whose A[r][j] has
//     bit t set,
// on 4 packed bytes per dword: multiplying by x is a shift plus 0x1D times the bit-7 flags (a
// packed 16-bit multiply; 5 VALU ops), the S_rt are 3-input XORs (v_bitop3) -- straight-line
// code, no table lookups, no branches.  For RS(20+6), with the 6-op shift-and-subtract doubling
// (variant bit 1), that is 469 VALU instructions per dword column against 634 for the table
// kernel (SQ_INSTS_VALU per wave 1875 vs 2537, profiles/r02_v14_pmc_valu_rs206.txt); the
// packed multiply takes 7 % more off (offline count, tools/jit_variants.py).  Encode goes from
// 0.67 to 0.73-0.74 of 8 TB/s.
// (A bit-sliced form of the same Horner chains needs 8 x 8 bit transposes, 150 ops per dword,
// and 300 VGPRs; it lost: profiles/r02_kbench_jit_v1.txt.)  Used for R * K >= 96 only: on
// narrower codes the table kernel is already at the memory-bound rate.  The generated kernel
// computes the same GF(2^8) products as the table kernel, bit for bit; it is used once its
// compile has finished (in the background), and the table kernel serves until then.
// LSEC_JIT=0 turns it off.
//
// RS / r6 at w = 16 / 32 (Jerasure's word layout, galois.c:527-604, :730-810) get the same
// treatment in the bit-sliced domain of k_gfw_transposed: each lane transposes W words of an
// input so that word x holds bit x of 32 elements, and output slice b of row r is the XOR of the
// input slices x whose product c_rj * x^x has bit b set -- the 32 x 32 (16 x 16) bitmatrix block
// of the coefficient, known at compile time, so every slice is a straight chain of 3-input XORs
// (about w/4 per output slice per input) instead of the generic kernel's popcount(c) sweeps of
// w XORs plus w-1 doublings.  gfw_source below.
#include "ec_netgen.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sstream>

namespace lsec {
namespace jit {

bool jit_on() {
  static const bool on = [] {
    const char *s = getenv("LSEC_JIT");
    return !s || *s != '0';
  }();
  return on;
}

int jit_variant() {
  static const int v = [] {
    const char *s = getenv("LSEC_JIT_VARIANT");
    return s ? atoi(s) : 0;
  }();
  return v;
}

const Variant &variant() {
  static const Variant v = [] {
    const int x = jit_variant();
    auto bits = [x](int lo, int n) { return (x >> lo) & ((1 << n) - 1); };
    const int cap = bits(8, 8);
    return Variant{bits(0, 1) != 0, bits(1, 1) != 0, bits(3, 1) != 0, bits(4, 4), cap == 0 ? 32 : cap == 255 ? 0 : cap,
                   bits(16, 1) != 0, std::max(1, bits(17, 2)), bits(19, 1) != 0, bits(20, 1) != 0, bits(21, 1) != 0, bits(22, 2),
                   bits(24, 1) != 0, bits(25, 2), bits(27, 1) != 0, bits(28, 1) != 0, bits(30, 1) != 0};
  }();
  return v;
}

bool wants_gfw_net(int R, int K, int w) {
  // every non-trivial w = 16 / 32 matrix (XOR-only ones take the plain-XOR path); at w = 32 the
  // R x 32 accumulator slices limit the one-wave form to 4 rows, the wave-pair split (half the
  // slices per wave) to 6 (8 rows spill at 2 waves per SIMD)
  const int max_w32 = gfw_rowsplit(32, 4) ? 6 : 4;
  return jit_on() && (w == 16 || w == 32) && R >= 1 && R <= (w == 32 ? max_w32 : kMaxRows) && K >= 1 && K <= kMaxCols;
}

bool wants_pktnet(int R, int K, int w) {
  // liberation-family bitmatrices (one mask word per bit-row and input) of modest width, two
  // outputs (encodes, double erasures): single-erasure decodes measured 0.72 on a network against
  // 0.76 on k_bitmatrix (profiles/r04_v12_pktnet.txt).  R * w <= 128: the measured shapes (4 rows
  // at w = 32, Cauchy-good(10+4) 0.80, r04_v13_pktnet_cauchy.txt); 8 rows at w = 32 hold 256
  // accumulator dwords per lane, and hipRTC took 320 s over one such network on the build host
  // (6 s at 4 rows), so wider shapes stay on the generic kernels
  return jit_on() && w >= 2 && w <= 32 && R >= 2 && R <= kMaxRows && K >= 1 && K <= kMaxCols && R * w <= 128;
}

bool wants_xornet(int R, int K) {
  const bool on = jit_on();
  // R * K >= 96 only: narrower codes are memory-bound on the table kernel already (RS(16+4) /
  // RS(12+4) level within noise on a network, profiles/r02_v15_jit_ab.txt)
  return on && R >= 2 && R <= kMaxRows && K >= 2 && K <= kMaxCols && R * K >= 96;
}

// dwords per lane: 16 B loads by default, 8 B for many-row networks over few inputs (R >= 8,
// K <= 13, where 16 B would be two pieces per lane: RS(12+8) encode 0.67 -> 0.70,
// profiles/r04_v15_xornet_ab.txt); LSEC_JIT_VARIANT bits 4-7 force 1 / 2 / 4
int xornet_dwords(int R, int K) {
  const int v = variant().dwords;
  if (v == 1 || v == 2 || v == 4) return v;
  return R >= 8 && K * 8 <= 104 ? 2 : 4;
}

int xornet_tile(int K, int R) {
  const int D = xornet_dwords(R, K);
  const int IT = D == 4 && K * 8 <= 104 ? 2 : 1;  // 16 B pieces per lane per shard (D = 4)
  return 256 * 4 * D * IT;
}

bool gfw_rowsplit(int w, int R) {
  // the wave-pair split below for networks of 4+ rows at w = 32, where the one-wave form holds one
  // wave per SIMD (RS(10+4) encode 0.66 -> 0.76; at 3 rows the one-wave form holds two and the
  // split gains nothing: profiles/r04_v9_gfw_w32_split.txt).  LSEC_JIT_VARIANT bit 19 turns it off
  // and from 5 rows at w = 16 (RS(20+6) 0.68 -> 0.72; bit 24 turns that off)
  if (variant().split_off) return false;
  return (w == 32 && R >= 4) || (w == 16 && R >= 5 && !variant().split_w16_off);
}

int gfw_tile(int w, int R) { return gfw_rowsplit(w, R) ? 128 * 4 * w : 256 * 4 * w; }

void pkt_shape(int R, int w, int packet, int *D, int *S) {
  // 16 B per lane where the packet allows, fewer where the R*w accumulator packets would pass 64
  // dwords (w = 7 / 8 at R = 2: 4 dwords, ~120 registers).  One output group: Cauchy(10+4) at
  // w = 32 (128 accumulators, one wave per SIMD) encodes at 0.80 that way, 0.61 / 0.41 in 2 / 4
  // groups (profiles/r04_v13_pktnet_cauchy.txt); LSEC_JIT_VARIANT bits 25-26 force 1 / 2 / 4
  int d = packet % 16 == 0 ? 4 : packet % 8 == 0 ? 2 : packet % 4 == 0 ? 1 : 0;
  while (d > 1 && R * w * d > 64) d /= 2;
  const int fv = variant().pkt_groups;
  *D = d;
  *S = fv ? 1 << (fv - 1) : 1;
}

// c * x in GF(2^w), Jerasure's polynomials (galois.c:65-98: 0210013, 020000007)
uint32_t gfw_times_x(uint32_t c, int w) {
  if (w == 8) {  // Jerasure's GF(2^8), x^8 = x^4+x^3+x^2+1 (0x11D)
    c <<= 1;
    return (c & 0x100u) ? (c ^ 0x11Du) & 0xFFu : c;
  }
  if (w == 16) {
    c <<= 1;
    return (c & 0x10000u) ? (c ^ 0x1100Bu) & 0xFFFFu : c;
  }
  const bool top = c >> 31;
  return (c << 1) ^ (top ? 0x400007u : 0u);
}

// the bitmatrix of each GF(2^w) coefficient: output packet l takes input packet x where bit l
// of c * x^x is set (Cauchy's packet layout, k_gfw_bitsliced)
std::vector<uint32_t> coef_masks(const uint32_t *coef, int R, int K, int w) {
  std::vector<uint32_t> masks(static_cast<size_t>(R) * w * K, 0u);
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < K; ++j) {
      uint32_t cx = coef[r * K + j] & (w == 8 ? 0xFFu : w == 16 ? 0xFFFFu : 0xFFFFFFFFu);
      for (int x = 0; x < w && cx; ++x) {
        for (int l = 0; l < w; ++l)
          if ((cx >> l) & 1u) masks[(static_cast<size_t>(r) * w + l) * K + j] |= 1u << x;
        cx = gfw_times_x(cx, w);
      }
    }
  return masks;
}

int Net::tile_bytes() const { return kind == kXor ? xornet_tile(K, R) : kind == kGfw ? gfw_tile(w, R) : 256 * 4 * D; }

uint64_t Net::tiles_per_stripe(int64_t size) const {
  const int64_t tile = tile_bytes();
  if (kind == kGfw) return static_cast<uint64_t>(size / tile);
  if (kind == kXor) return static_cast<uint64_t>((size + tile - 1) / tile);
  const int64_t cols = size / w;  // column bytes of a stripe: nsuper * packet
  return static_cast<uint64_t>((cols + tile - 1) / tile) * S;
}

std::string Net::source(const uint32_t *mat) const {
  if (kind == kPkt) return pktnet_source(mat, R, K, w, D, S);
  if (kind == kGfw) return gfw_source(mat, R, K, w);
  std::vector<uint8_t> m8(mat, mat + words());
  return xornet_source(m8.data(), R, K);
}

std::vector<uint32_t> Net::key(const uint32_t *mat) const {
  std::vector<uint32_t> k = {static_cast<uint32_t>(R), static_cast<uint32_t>(K), static_cast<uint32_t>(w)};
  if (kind == kPkt) {
    k[2] += 1000u;
    k.push_back(static_cast<uint32_t>(D));
    k.push_back(static_cast<uint32_t>(S));
  }
  k.insert(k.end(), mat, mat + words());
  return k;
}

namespace {

// a balanced left fold of terms with 3-input XORs (ceil((n-1)/2) ops)
std::string xor_chain(std::vector<std::string> t) {
  if (t.empty()) return "0u";
  while (t.size() > 1) {
    std::vector<std::string> n;
    size_t i = 0;
    for (; i + 3 <= t.size(); i += 3) n.push_back("X3(" + t[i] + "," + t[i + 1] + "," + t[i + 2] + ")");
    if (t.size() - i == 2) n.push_back("(" + t[i] + "^" + t[i + 1] + ")");
    else if (t.size() - i == 1) n.push_back(t[i]);
    t.swap(n);
  }
  return t[0];
}

// Greedy common-pair elimination over XOR sets of symbols 0 .. nsym-1 (Paar's heuristic): the
// pair of symbols that occurs together in the most sets (the first such pair in lexicographic
// order) becomes a new symbol nsym, nsym + 1, ... while it occurs in at least 3 (one 2-input XOR
// then saves a term in each of them) and fewer than `cap` pairs are shared.
std::vector<std::pair<int, int>> share_pairs(std::vector<std::vector<int>> &sets, int nsym, int cap) {
  std::vector<std::pair<int, int>> pairs;
  for (; static_cast<int>(pairs.size()) < cap; ++nsym) {
    std::vector<int> count(static_cast<size_t>(nsym) * nsym, 0);
    for (auto &set : sets)
      for (size_t i = 0; i < set.size(); ++i)
        for (size_t j = i + 1; j < set.size(); ++j) ++count[static_cast<size_t>(std::min(set[i], set[j])) * nsym + std::max(set[i], set[j])];
    const auto best = std::max_element(count.begin(), count.end());  // the first maximum
    if (best == count.end() || *best < 3) break;
    const int a = static_cast<int>(best - count.begin()) / nsym, b = static_cast<int>(best - count.begin()) % nsym;
    pairs.push_back({a, b});
    for (auto &set : sets) {
      if (std::find(set.begin(), set.end(), a) == set.end() || std::find(set.begin(), set.end(), b) == set.end()) continue;
      set.erase(std::remove_if(set.begin(), set.end(), [&](int x) { return x == a || x == b; }), set.end());
      set.push_back(nsym);
    }
  }
  return pairs;
}

// The types, struct Args { ...; Ref in[K]; Ref out[R]; unsigned phase; } (ec_jit.cpp packs it),
// X3 and the global-pointer casts every network starts with.  `int2`: the name of Args' second
// int; `defs` / `funcs`: what a shape adds before / after X3; `casts`: (suffix, pointee) of its
// G<suffix> / GW<suffix> macros.
void prelude(std::ostringstream &s, int R, int K, const char *int2, bool u16x2, const std::string &defs, const std::string &funcs,
             std::initializer_list<std::pair<const char *, const char *>> casts) {
  s << "typedef unsigned int u32;\n"
    << (u16x2 ? "typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));\n" : "")
    << "typedef u32 u32x4 __attribute__((ext_vector_type(4)));\n"
       "typedef u32 u32x2 __attribute__((ext_vector_type(2)));\n"
       "struct Ref { unsigned long long base; long long stride; };\n"
    << "struct Args { long long size; int nstripes; int " << int2 << "; Ref in[" << K << "]; Ref out[" << R << "]; unsigned phase; };\n"
    << defs << "#define X3(a,b,c) __builtin_amdgcn_bitop3_b32((a),(b),(c),0x96)\n"
    << funcs;
  for (const auto &c : casts)
    s << "#define G" << c.first << "(a) ((const __attribute__((address_space(1))) " << c.second << " *)(a))\n"
      << "#define GW" << c.first << "(a) ((__attribute__((address_space(1))) " << c.second << " *)(a))\n";
}

// The head of the tile loop, down to the stripe s of tile t: tiles per stripe as
// Net::tiles_per_stripe counts them (a packet network's S groups of a column tile are tiles
// ct * S + g), and the first tile of a block (one tile per block, XCD x taking a contiguous
// eighth of the tiles in dispatch order).  Args::phase > 0 (the XCD tile phase,
// lsec::tile_phase_net_on, ec_kernels.h; off by default for the networks): XCD x starts its eighth
// x * phase tiles further on and wraps around inside it.
void loop_head(std::ostringstream &s, const Net &net) {
  const int tile = net.tile_bytes();
  const bool pkt = net.kind == Net::kPkt;
  if (pkt)
    s << "  const unsigned P = (unsigned)a.packet;\n"
      << "  const unsigned cols = (unsigned)(a.size / " << net.w << ");\n"
      << "  const unsigned tps = (cols + " << tile - 1 << ") / " << tile << ";\n"
      << "  const unsigned nt = tps * (unsigned)a.nstripes * " << net.S << "u;\n";
  else if (net.kind == Net::kXor)
    s << "  const long long C = a.size;\n"
      << "  const unsigned tps = (unsigned)((C + " << tile - 1 << ") / " << tile << ");\n"
      << "  const unsigned nt = tps * (unsigned)a.nstripes;\n";
  else
    s << "  const long long C = a.size;\n"
      << "  const unsigned tps = (unsigned)(C / " << tile << ");\n"
      << "  const unsigned nt = tps * (unsigned)a.nstripes;\n";
  s << "  const unsigned nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = blockIdx.x & 7;\n"
       "  const unsigned sz_ = per + (xcd < rem ? 1u : 0u);\n"
       "  const unsigned ph_ = (nb == nt && sz_) ? (xcd * a.phase) % sz_ : 0u;\n"
       "  const unsigned t0 = xcd * per + (xcd < rem ? xcd : rem) + (ph_ ? ((blockIdx.x >> 3) + ph_) % sz_ : (blockIdx.x >> 3));\n"
       "  for (unsigned t = t0; t < nt; t += nb) {\n";
  if (pkt) s << "    const unsigned g = t % " << net.S << "u, ct = t / " << net.S << "u;\n    const unsigned s = ct / tps;\n";
  else s << "    const unsigned s = t / tps;\n";
}

// How a network reads its shard table (struct Args { ...; Ref in[K]; Ref out[R]; }): "a." for the
// kernel argument, or -- from 24 shards -- "ap->", an opaque pointer to the kernarg segment
// re-read in every tile, so that the table's 4 (K + R) SGPRs are not hoisted out of the tile loop
// and spilled to VGPR lanes (RS(24+8): 65 SGPRs spilled, 2661 -> 2339 VALU ops a tile, encode
// 0.65 -> 0.71, 8-loss decode 0.62 -> 0.69; RS(12+8) spills 7 and loses 3 % with it:
// profiles/r04_v18_xornet_reload.txt).  LSEC_JIT_VARIANT bit 28 forces it on, bit 30 off
std::string shard_table(std::ostringstream &s, int K, int R, const char *ind) {
  if (variant().reload_off || !(variant().reload_on || K + R >= 24)) return "a.";
  s << ind << "const __attribute__((address_space(4))) Args *ap = (const __attribute__((address_space(4))) Args *)"
            "__builtin_amdgcn_kernarg_segment_ptr();\n"
    << ind << "asm volatile(\"\" : \"+s\"(ap));\n";
  return "ap->";
}

// the address of stripe s of shard i of table `tab` ("in" / "out") under the table prefix A
std::string shard(const std::string &A, const char *tab, int i) {
  const std::string ref = A + tab + "[" + std::to_string(i) + "]";
  return ref + ".base + (unsigned long long)s * " + ref + ".stride";
}

}  // namespace

std::string xornet_source(const uint8_t *mat, int R, int K) {
  const Net net = Net::matrix(R, K, 8);
  const int D = xornet_dwords(R, K), tile = net.tile_bytes();
  const int IT = tile / (256 * 4 * D);  // 16 B pieces per lane per shard (xornet_tile)
  const int DL = D * IT;                // dwords per lane per shard
  // the XOR sets of the Horner steps of every row (row r: sets first[r] .. first[r+1]-1, from its
  // top bit down; every step but a row's first doubles h first): the inputs, or shared pairs
  // K.., whose coefficient has bit t set
  std::vector<std::vector<int>> sets;
  std::vector<size_t> first(R + 1, 0);
  for (int r = 0; r < R; ++r) {
    first[r] = sets.size();
    int top = -1;
    for (int t = 7; t >= 0 && top < 0; --t)
      for (int j = 0; j < K; ++j)
        if ((mat[r * K + j] >> t) & 1) top = t;
    for (int t = top; t >= 0; --t) {
      sets.emplace_back();
      for (int j = 0; j < K; ++j)
        if ((mat[r * K + j] >> t) & 1) sets.back().push_back(j);
    }
  }
  first[R] = sets.size();
  // common-pair elimination, capped so that the inputs and the pairs (D*IT registers each) stay
  // within about 128 registers: RS(20+6) encode 0.70 -> 0.74 and its 6-loss decode 0.65 -> 0.73,
  // RS(24+8) encode 0.60 -> 0.66, RS(12+8) 0.68 -> 0.72 (profiles/r04_v15_xornet_ab.txt; uncapped,
  // the pairs cost occupancy).  LSEC_JIT_VARIANT bit 0: no cap; bit 3: no pairs (the round-3 form)
  const int cap = variant().pairs_uncapped ? 1 << 30 : variant().pairs_off ? 0 : std::max(0, (128 - K * DL) / DL);
  const std::vector<std::pair<int, int>> pairs = share_pairs(sets, K, cap);
  auto sym = [&](int x) { return (x < K ? "e" : "p") + std::to_string(x < K ? x : x - K) + "[d]"; };

  std::ostringstream s;
  prelude(s, R, K, "pad", true, "",
          !variant().doubling_by_sub
              // x * (4 packed GF(2^8) elements), polynomial 0x11D: shift, and 0x1D times the bit-7 flags
              // by a packed 16-bit multiply (each 16-bit half holds two flags, 0x1D1D at most)
              ? "__device__ static inline u32 XT(u32 a) {\n"
                "  const u16x2 f = __builtin_bit_cast(u16x2, (a >> 7) & 0x01010101u) * (u16x2){0x1D, 0x1D};\n"
                "  return ((a << 1) & 0xFEFEFEFEu) ^ __builtin_bit_cast(u32, f);\n"
                "}\n"
              // x * (4 packed GF(2^8) elements), polynomial 0x11D: shift the low 7 bits of every byte,
              // and XOR the taps 0x1D into the bytes whose bit 7 was set (t - (t >> 7) is 0x7F in exactly
              // those bytes, borrow-free).  A 24-bit multiply of the bit-7 flags by 0x1D would drop byte 3.
              : "__device__ static inline u32 XT(u32 a) {\n"
                "  const u32 t = a & 0x80808080u;\n"
                "  return ((a ^ t) << 1) ^ ((t - (t >> 7)) & 0x1D1D1D1Du);\n"
                "}\n",
          {{"", "u32x4"}, {"2", "u32x2"}, {"1", "u32"}});
  s << // a lane's D dwords at byte o of a shard of C bytes (C % 8 == 0: tails are whole 8 B)
       "__device__ static inline void ld4(u32 *e, unsigned long long p, long long o, long long C) {\n"
       "  if (o + 16 <= C) { const u32x4 v = __builtin_nontemporal_load(G(p + o)); e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; return; }\n"
       "  e[0] = e[1] = e[2] = e[3] = 0u;\n"
       "  if (o + 8 <= C) { const u32x2 h = *G2(p + o); e[0] = h.x; e[1] = h.y; }\n"
       "}\n"
       "__device__ static inline void st4(const u32 *h, unsigned long long p, long long o, long long C) {\n"
       "  if (o + 16 <= C) __builtin_nontemporal_store((u32x4){h[0], h[1], h[2], h[3]}, GW(p + o));\n"
       "  else if (o + 8 <= C) *GW2(p + o) = (u32x2){h[0], h[1]};\n"
       "}\n"
       "__device__ static inline void ld2(u32 *e, unsigned long long p, long long o, long long C) {\n"
       "  if (o + 8 <= C) { const u32x2 v = __builtin_nontemporal_load(G2(p + o)); e[0] = v.x; e[1] = v.y; return; }\n"
       "  e[0] = e[1] = 0u;\n"
       "}\n"
       "__device__ static inline void st2(const u32 *h, unsigned long long p, long long o, long long C) {\n"
       "  if (o + 8 <= C) __builtin_nontemporal_store((u32x2){h[0], h[1]}, GW2(p + o));\n"
       "}\n"
       // D = 1: a lane owns 4 B; a chunk ends on 8 B, so its last 4 B are in range too
       "__device__ static inline void ld1(u32 *e, unsigned long long p, long long o, long long C) {\n"
       "  e[0] = o + 4 <= C ? __builtin_nontemporal_load(G1(p + o)) : 0u;\n"
       "}\n"
       "__device__ static inline void st1(const u32 *h, unsigned long long p, long long o, long long C) {\n"
       "  if (o + 4 <= C) __builtin_nontemporal_store(h[0], GW1(p + o));\n"
       "}\n"
       "extern \"C\" __global__ __launch_bounds__(256) void lsec_xornet(Args a) {\n";
  loop_head(s, net);
  s << "    const long long o0 = (long long)(t - s * tps) * " << tile << " + threadIdx.x * " << 4 * D << ";\n";
  const std::string A = shard_table(s, K, R, "    ");
  for (int j = 0; j < K; ++j) {
    s << "    u32 e" << j << "[" << DL << "];\n    { const unsigned long long p = " << shard(A, "in", j) << ";\n";
    for (int it = 0; it < IT; ++it)
      s << "      ld" << D << "(e" << j << " + " << D * it << ", p, o0 + " << 256 * 4 * D * it << ", C);\n";
    s << "    }\n";
  }
  for (size_t i = 0; i < pairs.size(); ++i)
    s << "    u32 p" << i << "[" << DL << "];\n    for (int d = 0; d < " << DL << "; ++d) p" << i << "[d] = " << sym(pairs[i].first)
      << " ^ " << sym(pairs[i].second) << ";\n";
  for (int r = 0; r < R; ++r) {
    s << "    { u32 h[" << DL << "];\n";
    if (first[r] == first[r + 1]) s << "      for (int d = 0; d < " << DL << "; ++d) h[d] = 0u;\n";
    // Horner over the coefficient bits: h = x(...x(S_top) + ...) + S_0
    for (size_t i = first[r]; i < first[r + 1]; ++i) {
      s << "      for (int d = 0; d < " << DL << "; ++d) {\n";
      std::vector<std::string> terms;
      if (i != first[r]) {
        s << "        const u32 x = XT(h[d]);\n";
        terms.push_back("x");
      }
      for (int x : sets[i]) terms.push_back(sym(x));
      s << "        h[d] = " << xor_chain(terms) << ";\n      }\n";
    }
    s << "      const unsigned long long q = " << shard(A, "out", r) << ";\n";
    for (int it = 0; it < IT; ++it) s << "      st" << D << "(h + " << D * it << ", q, o0 + " << 256 * 4 * D * it << ", C);\n";
    s << "    }\n";
  }
  s << "  }\n}\n";
  return s.str();
}

// ---- GF(2^16) / GF(2^32): bit-sliced networks over Jerasure's word layout
namespace {

// Types, the bit transpose and the whole-tile loads / stores shared by both network shapes: a
// lane's W dwords of a shard are W/4 pieces of 16 B, `stride` bytes apart
void gfw_prelude(std::ostringstream &s, int R, int K, int W, int stride) {
  prelude(s, R, K, "pad", false, "#define W " + std::to_string(W) + "\n#define PIECE " + std::to_string(stride) + "\n", "",
          {{"", "u32x4"}});
  s << // the W x W bit transpose of k_gfw_transposed (ec_kernels_impl.h, transpose_units)
       "template <int d> __device__ static inline void tb(u32 (&D)[W], u32 m) {\n"
       "#pragma unroll\n"
       "  for (int r = 0; r < W; ++r) { if (r & d) continue; const u32 x = D[r], y = D[r + d];\n"
       "    D[r] = (x & m) | ((y << d) & ~m); D[r + d] = ((x >> d) & m) | (y & ~m); }\n"
       "}\n"
       "__device__ static inline void tr(u32 (&D)[W]) {\n"
       "#if W == 32\n"
       "#pragma unroll\n"
       "  for (int r = 0; r < 16; ++r) { const u32 x = D[r], y = D[r + 16];\n"
       "    D[r] = __builtin_amdgcn_perm(y, x, 0x05040100u); D[r + 16] = __builtin_amdgcn_perm(y, x, 0x07060302u); }\n"
       "#endif\n"
       "#pragma unroll\n"
       "  for (int r = 0; r < W; ++r) { if (r & 8) continue; const u32 x = D[r], y = D[r + 8];\n"
       "    D[r] = __builtin_amdgcn_perm(y, x, 0x06020400u); D[r + 8] = __builtin_amdgcn_perm(y, x, 0x07030501u); }\n"
       "  tb<4>(D, 0x0F0F0F0Fu); tb<2>(D, 0x33333333u); tb<1>(D, 0x55555555u);\n"
       "}\n"
       // whole tiles only: the launcher hands a ragged tail to the generic kernel, so loads are
       // unconditional and each tile is one basic block for the scheduler
       "__device__ static inline void ld(u32 (&e)[W], unsigned long long p) {\n"
       "#pragma unroll\n"
       "  for (int q = 0; q < W / 4; ++q) { const u32x4 v = __builtin_nontemporal_load(G(p + q * PIECE));\n"
       "    e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w; }\n"
       "}\n"
       "__device__ static inline void st(const u32 (&h)[W], unsigned long long p) {\n"
       "#pragma unroll\n"
       "  for (int q = 0; q < W / 4; ++q)\n"
       "    __builtin_nontemporal_store((u32x4){h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]}, GW(p + q * PIECE));\n"
       "}\n";
}

// Input j's contribution to the R output rows (accumulators h<r>): slice b of row r takes the
// input slices x (in array `e`, transposed) with bit b of c_rj * x^x set -- the bitmatrix block of
// the coefficient -- after common-pair elimination over those rows (at most variant's
// slice_pair_cap shared pairs, each used by at least 3 slices)
void gfw_net(std::ostringstream &s, const uint32_t *mat, int R, int K, int W, int j, std::vector<std::vector<bool>> &live,
             const std::string &e, const char *ind, bool linear, int b0 = 0, int b1 = -1) {
  // output slices b0 .. b1-1 only (accumulator element b - b0); linear: serial folds into the
  // accumulator instead of balanced 3-input XOR trees
  if (b1 < 0) b1 = W;
  std::vector<std::vector<int>> sl(static_cast<size_t>(R) * W);
  bool any = false;
  for (int r = 0; r < R; ++r) {
    uint32_t cx = mat[r * K + j];
    any |= cx != 0;
    for (int x = 0; x < W && cx; ++x) {
      for (int b = b0; b < b1; ++b)
        if ((cx >> b) & 1u) sl[r * W + b].push_back(x);
      cx = gfw_times_x(cx, W);
    }
  }
  if (!any) return;
  const std::vector<std::pair<int, int>> pairs = share_pairs(sl, W, variant().slice_pair_cap);
  auto nm = [&](int x) { return x < W ? e + "[" + std::to_string(x) + "]" : "p" + std::to_string(x - W); };
  s << ind << "{\n";
  for (size_t i = 0; i < pairs.size(); ++i)
    s << ind << "  const u32 p" << i << " = " << nm(pairs[i].first) << " ^ " << nm(pairs[i].second) << ";\n";
  for (int r = 0; r < R; ++r)
    for (int b = b0; b < b1; ++b) {
      const auto &row = sl[r * W + b];
      if (row.empty()) continue;
      std::vector<std::string> t;
      const std::string a = "h" + std::to_string(r) + "[" + std::to_string(b - b0) + "]";
      if (live[r][b - b0]) t.push_back(a);
      for (int x : row) t.push_back(nm(x));
      if (linear) {
        // a serial fold into the accumulator: no partial sums of the inputs alone for the
        // scheduler to hoist (each is a VGPR live until its fold)
        std::string v = t[0];
        size_t k = 1;
        for (; k + 2 <= t.size(); k += 2) {
          s << ind << "  " << a << " = X3(" << v << ", " << t[k] << ", " << t[k + 1] << ");\n";
          v = a;
        }
        if (k < t.size()) s << ind << "  " << a << " = " << v << " ^ " << t[k] << ";\n";
        else if (v != a) s << ind << "  " << a << " = " << v << ";\n";
      } else {
        s << ind << "  " << a << " = " << xor_chain(t) << ";\n";
      }
      live[r][b - b0] = true;
    }
  s << ind << "}\n";
}

// the inputs with a non-zero coefficient in some row
std::vector<int> gfw_used(const uint32_t *mat, int R, int K) {
  std::vector<int> used;
  for (int j = 0; j < K; ++j)
    for (int r = 0; r < R; ++r)
      if (mat[r * K + j]) {
        used.push_back(j);
        break;
      }
  return used;
}

// Wave-pair split of the w = 32 (4-6 rows) and w = 16 (5-8 rows) networks.  The one-wave form keeps R x 32
// accumulator slices per lane (128 VGPRs at 4 rows) plus two inputs' 32 slices: at 4 rows its code
// object takes 273 registers, one wave per SIMD.  Here the 4 waves of a block form 2 pairs; the two waves of a pair cover the same 64 lane
// columns and each computes half of every output row's bit slices (role 0 slices 0-15, role 1
// 16-31; balanced for any R).  Per step each wave loads and transposes one input (role 0 the even
// used inputs, role 1 the odd), writes its 32 slices to LDS, XORs them into its half slices, and
// after a barrier reads its partner's input slices from LDS into the same registers and XORs
// those in: every input is still loaded and transposed once and the accumulators halve (64 VGPRs
// at 4 rows).  At the end the halves meet through LDS: role 0 transposes and stores rows
// 0 .. ceil(R/2)-1, role 1 the rest.  Tile: 128 lane columns x 16 B x 8 pieces, 2 KiB apart
// (16 KiB per shard); LDS 2 pairs x 2 roles x 8 KiB (12 KiB at 5-6 rows).  The roles' code sits
// in two consecutive `if (role == r)` blocks, never in if / else: at an if / else join the
// compiler kept both branches' accumulators apart (294 registers at RS(10+4) even with identical
// branches; 139 as consecutive ifs, profiles/r04_v9_gfw_w32_split.txt).
std::string gfw_rowsplit_source(const uint32_t *mat, int R, int K, int W) {
  const Net net = Net::matrix(R, K, W);
  const int tile = net.tile_bytes(), HW = W / 2;
  const int n0 = (R + 1) / 2;  // output rows of role 0: 0 .. n0-1; role 1: n0 .. R-1
  // quads (64 lanes x 16 B) of a wave's LDS slot: one transposed input (W / 4), or the half
  // slices of the rows it hands its partner at the end (at most n0 rows of HW / 4)
  const int lq = std::max(W / 4, n0 * (HW / 4));
  // the roles' accumulator slices written so far
  std::vector<std::vector<bool>> live[2] = {std::vector<std::vector<bool>>(R, std::vector<bool>(HW, false)),
                                            std::vector<std::vector<bool>>(R, std::vector<bool>(HW, false))};
  const std::vector<int> used = gfw_used(mat, R, K);
  const int n = static_cast<int>(used.size()), steps = (n + 1) / 2;
  std::ostringstream s;
  // defaults measured best (profiles/r04_v9_gfw_w32_split.txt): serial folds (LSEC_JIT_VARIANT
  // bit 21: trees instead), one input prefetched (bit 20: none), and an occupancy target of 3
  // waves per SIMD for the register allocator (bits 22-23: 1 none, 2 four, 3 two), which RS(10+4)
  // meets at 167 registers without spills
  const bool linear = !variant().fold_flip;
  const int wv_opt = variant().split_waves, wpe = wv_opt == 0 ? (R <= 4 ? 3 : 2) : wv_opt == 1 ? 0 : wv_opt == 2 ? 4 : 2;
  gfw_prelude(s, R, K, W, 128 * 16);
  s << "extern \"C\" __global__ __launch_bounds__(256) ";
  if (wpe) s << "__attribute__((amdgpu_waves_per_eu(" << wpe << "))) ";
  s << "void lsec_xornet(Args a) {\n"
    << "  __shared__ u32x4 L[2][2][" << lq << "][64];\n"
       "  const unsigned wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;\n"
       "  const unsigned pair = wv >> 1, role = wv & 1;\n"
       "  u32x4 (*const mine)[64] = L[pair][role];\n"
       "  u32x4 (*const theirs)[64] = L[pair][role ^ 1];\n";
  loop_head(s, net);
  s << "    const long long base = (long long)(t - s * tps) * " << tile << " + (pair * 64 + lane) * 16;\n";
  const std::string A = shard_table(s, K, R, "    ");
  for (int r = 0; r < R; ++r) s << "    u32 h" << r << "[" << HW << "];\n";
  s << "    u32 e0[W], e1[W];\n";
  auto ptr = [&](int j) { return shard(A, "in", j) + " + base"; };
  // step u's own inputs into buffer b: used[2u] (role 0) and used[2u+1] (role 1)
  auto load = [&](int u, int b) {
    if (2 * u >= n) return;
    if (2 * u + 1 < n)
      s << "    ld(e" << b << ", role ? " << ptr(used[2 * u + 1]) << " : " << ptr(used[2 * u]) << ");\n";
    else
      s << "    if (role == 0) ld(e" << b << ", " << ptr(used[2 * u]) << ");\n";
  };
  // bit 20: no prefetch -- each step loads its own input at its top (32 fewer VGPRs live; the
  // other waves of the SIMD hide the latency)
  const bool ahead = !variant().split_no_prefetch;
  if (ahead) load(0, 0);
  for (int u = 0; u < steps; ++u) {
    const int b = ahead ? u & 1 : 0;
    const std::string e = "e" + std::to_string(b);
    // input j into role's half of every row's slices
    auto net_of = [&](int role, int j) { gfw_net(s, mat, R, K, W, j, live[role], e, "      ", linear, role * HW, role * HW + HW); };
    auto half = [&](int role, int j) {
      s << "    if (role == " << role << ") {\n";
      net_of(role, j);
      s << "    }\n";
    };
    const bool pairB = 2 * u + 1 < n;
    load(ahead ? u + 1 : u, ahead ? b ^ 1 : 0);
    // own input: transpose, publish, accumulate.  A lone last input (odd count) is role 0's:
    // role 1 then only reads it
    const char *own = pairB ? "" : "if (role == 0) ";
    s << "    " << own << "tr(" << e << ");\n"
      << "    " << own << "{\n"
      << "#pragma unroll\n      for (int q = 0; q < W / 4; ++q) mine[q][lane] = (u32x4){" << e << "[4 * q], " << e
      << "[4 * q + 1], " << e << "[4 * q + 2], " << e << "[4 * q + 3]};\n    }\n";
    half(0, used[2 * u]);
    if (pairB) half(1, used[2 * u + 1]);
    s << "    __builtin_amdgcn_sched_barrier(0);\n    __syncthreads();\n";
    // the partner's input from LDS, into the same registers
    const std::string rd = "#pragma unroll\n      for (int q = 0; q < W / 4; ++q) { const u32x4 v = theirs[q][lane]; " + e + "[4 * q] = v.x; " + e +
                           "[4 * q + 1] = v.y; " + e + "[4 * q + 2] = v.z; " + e + "[4 * q + 3] = v.w; }\n";
    if (pairB) {
      s << "    {\n" << rd << "    }\n";
      half(0, used[2 * u + 1]);
      half(1, used[2 * u]);
    } else {
      s << "    if (role == 1) {\n" << rd;
      net_of(1, used[2 * u]);
      s << "    }\n";
    }
    s << "    __builtin_amdgcn_sched_barrier(0);\n    __syncthreads();\n";
  }
  // the halves meet: each role publishes its slices of the rows the other stores (slot k = the
  // k-th of those rows, 4 quads each), then completes its own rows from the partner's slots
  auto zero = [&](const std::vector<std::vector<bool>> &lv) {
    for (int r = 0; r < R; ++r)
      for (int b = 0; b < HW; ++b)
        if (!lv[r][b]) s << "      h" << r << "[" << b << "] = 0u;\n";
  };
  auto publish = [&](int lo, int hi) {
    for (int r = lo; r < hi; ++r)
      for (int q = 0; q < HW / 4; ++q)
        s << "      mine[" << (r - lo) * (HW / 4) + q << "][lane] = (u32x4){h" << r << "[" << 4 * q << "], h" << r << "["
          << 4 * q + 1 << "], h" << r << "[" << 4 * q + 2 << "], h" << r << "[" << 4 * q + 3 << "]};\n";
  };
  auto complete = [&](int lo, int hi, bool low_half_mine) {
    for (int r = lo; r < hi; ++r) {
      s << "      { u32 f[W];\n";
      for (int q = 0; q < HW / 4; ++q) {
        const int mo = low_half_mine ? 4 * q : HW + 4 * q, po = low_half_mine ? HW + 4 * q : 4 * q;
        s << "        { const u32x4 v = theirs[" << (r - lo) * (HW / 4) + q << "][lane]; f[" << po << "] = v.x; f[" << po + 1
          << "] = v.y; f[" << po + 2 << "] = v.z; f[" << po + 3 << "] = v.w; }\n";
        for (int d = 0; d < 4; ++d) s << "        f[" << mo + d << "] = h" << r << "[" << 4 * q + d << "];\n";
      }
      s << "        tr(f);\n        st(f, " << shard(A, "out", r) << " + base);\n      }\n";
    }
  };
  s << "    if (role == 0) {\n";
  zero(live[0]);
  publish(n0, R);
  s << "    }\n    if (role == 1) {\n";
  zero(live[1]);
  publish(0, n0);
  s << "    }\n    __syncthreads();\n    if (role == 0) {\n";
  complete(0, n0, true);
  s << "    }\n    if (role == 1) {\n";
  complete(n0, R, false);
  s << "    }\n    __syncthreads();\n  }\n}\n";
  return s.str();
}

}  // namespace

std::string gfw_source(const uint32_t *mat, int R, int K, int W) {
  if (gfw_rowsplit(W, R)) return gfw_rowsplit_source(mat, R, K, W);
  // LSEC_JIT_VARIANT bits 8-15: most shared pairs per input (0: the default 32, 255: none);
  // bit 16: let the compiler schedule loads freely (no one-input-ahead prefetch fenced by sched
  // barriers: it then hoists every input's loads and spills at 10+4, w = 32)
  const bool fenced = !variant().unfenced;
  // bits 17-18: inputs loaded ahead of their use (0: the default 1); bit 21: serial XOR folds
  const int ahead = variant().ahead;
  const bool linear = variant().fold_flip;
  const Net net = Net::matrix(R, K, W);  // the launch covers whole tiles only
  std::ostringstream s;
  gfw_prelude(s, R, K, W, 4096);
  s << "extern \"C\" __global__ __launch_bounds__(256) void lsec_xornet(Args a) {\n";
  loop_head(s, net);
  s << "    const long long base = (long long)(t - s * tps) * " << net.tile_bytes() << " + threadIdx.x * 16;\n";
  const std::string A = shard_table(s, K, R, "    ");
  for (int r = 0; r < R; ++r) s << "    u32 h" << r << "[W];\n";
  std::vector<std::vector<bool>> live(R, std::vector<bool>(W, false));
  // inputs with a non-zero coefficient in some row, each loaded one input ahead of its use: the
  // scheduler would otherwise hoist every input's loads to the top (K x W registers live: spills
  // at 10+4, w = 32), so sched barriers fence each input's arithmetic
  const std::vector<int> used = gfw_used(mat, R, K);
  const size_t nbuf = static_cast<size_t>(ahead) + 1;
  auto load = [&](size_t u) { s << "    ld(e" << u % nbuf << ", " << shard(A, "in", used[u]) << " + base);\n"; };
  for (size_t b = 0; b < nbuf; ++b) s << "    u32 e" << b << "[W];\n";
  for (size_t u = 0; u < used.size() && u < static_cast<size_t>(ahead); ++u) load(u);
  for (size_t u = 0; u < used.size(); ++u) {
    if (u + ahead < used.size()) load(u + ahead);
    const std::string e = "e" + std::to_string(u % nbuf);
    s << "    tr(" << e << ");\n";
    gfw_net(s, mat, R, K, W, used[u], live, e, "    ", linear);
    if (fenced) s << "    __builtin_amdgcn_sched_barrier(0);\n";
  }
  for (int r = 0; r < R; ++r) {
    for (int b = 0; b < W; ++b)
      if (!live[r][b]) s << "    h" << r << "[" << b << "] = 0u;\n";
    s << "    tr(h" << r << ");\n    st(h" << r << ", " << shard(A, "out", r) << " + base);\n";
  }
  s << "  }\n}\n";
  return s.str();
}

// Packet networks for bitmatrix codes (liberation / blaum_roth / liber8tion; jerasure_bitmatrix_dotprod,
// jerasure.c:317-362) and for Cauchy codes at w = 16 / 32 (the bitmatrix of each GF(2^w)
// coefficient): a super-packet is w packets of P bytes per shard; packet l of output r is the XOR
// of the input packets (j, x) whose bit B[r*w+l][j*w+x] is set.  With the bitmatrix known when the
// kernel is compiled every output packet is a straight XOR chain (shared pairs per input, as
// gfw_net), where k_bitmatrix tests R*w*w mask bits per input under uniform branches and moves 4 B
// per lane, and k_gfw_bitsliced XORs w slices per set coefficient bit.  A lane owns D dwords (16 B
// at P % 16 == 0) of one packet column; it loads the packets of that column each input needs (one
// input ahead, fenced) and stores its output packets.  With S > 1 groups (an A/B knob; slower)
// the output packets (r, l) are split by l into S groups, tile t computing group t % S of column
// tile t / S: the groups of one column run side by side on one XCD and re-read the inputs from its
// L2.  Lanes past the last column redo the last column: no divergent branch.
// masks[((r*w + l)*K + j)] bit x = B[r*w+l][j*w+x] (w <= 32).
std::string pktnet_source(const uint32_t *masks, int R, int K, int W, int D, int S) {
  const Net net{Net::kPkt, R, K, W, D, S};
  const int tile = net.tile_bytes();
  const char *vt = D == 4 ? "u32x4" : D == 2 ? "u32x2" : "u32";
  std::ostringstream s;
  prelude(s, R, K, "packet", false, std::string("typedef ") + vt + " V;\n", "", {{"", "V"}});
  s << "#define D " << D << "\n"
       "__device__ static inline void ld(u32 (&e)[D], unsigned long long p) {\n"
       "  const V v = __builtin_nontemporal_load(G(p));\n"
    << (D == 1 ? "  e[0] = v;\n" : D == 2 ? "  e[0] = v.x; e[1] = v.y;\n" : "  e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;\n")
    << "}\n"
       "__device__ static inline void st(const u32 (&h)[D], unsigned long long p) {\n"
    << (D == 1 ? "  __builtin_nontemporal_store(h[0], GW(p));\n"
               : D == 2 ? "  __builtin_nontemporal_store((u32x2){h[0], h[1]}, GW(p));\n"
                        : "  __builtin_nontemporal_store((u32x4){h[0], h[1], h[2], h[3]}, GW(p));\n")
    << "}\n"
       "extern \"C\" __global__ __launch_bounds__(256) void lsec_xornet(Args a) {\n";
  loop_head(s, net);
  // lanes past the last column redo the last column (same loads, same bytes stored)
  s << "    const unsigned colb = min((ct - s * tps) * " << tile << " + threadIdx.x * " << 4 * D << ", cols - " << 4 * D << "u);\n"
       "    const unsigned sp = colb / P;\n"
    << "    const long long off = (long long)sp * " << W << " * P + (colb - sp * P);\n";
  const std::string A = shard_table(s, K, R, "    ");
  const int per_g = (W + S - 1) / S;
  // accumulators and input buffers declared once, shared by the groups' blocks (each group's
  // packet l uses slot l - l0): the compiler then gives the blocks the same registers
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < per_g; ++i) s << "    u32 h" << r << "_" << i << "[D];\n";
  for (int b2 = 0; b2 < 2; ++b2)
    for (int x = 0; x < W; ++x) s << "    u32 e" << b2 << "_" << x << "[D];\n";
  for (int grp = 0; grp < S; ++grp) {
    const int l0 = grp * per_g, l1 = std::min(W, l0 + per_g);
    if (l0 >= l1) continue;
    std::vector<int> rl_of;  // this group's output packets, as r*W + l
    for (int r = 0; r < R; ++r)
      for (int l = l0; l < l1; ++l) rl_of.push_back(r * W + l);
    s << "    if (g == " << grp << "u) {\n";
    std::vector<bool> live(static_cast<size_t>(R) * W, false);
    // inputs and their packets this group reads
    std::vector<int> used;
    std::vector<uint32_t> need;
    for (int j = 0; j < K; ++j) {
      uint32_t nm_ = 0;
      for (int rl : rl_of) nm_ |= masks[static_cast<size_t>(rl) * K + j];
      if (nm_) {
        used.push_back(j);
        need.push_back(nm_);
      }
    }
    auto load = [&](size_t u) {
      s << "      { const unsigned long long p = " << shard(A, "in", used[u]) << " + off;\n";
      for (int x = 0; x < W; ++x)
        if ((need[u] >> x) & 1u) s << "        ld(e" << u % 2 << "_" << x << ", p + " << x << "ull * P);\n";
      s << "      }\n";
    };
    if (!used.empty()) load(0);
    for (size_t u = 0; u < used.size(); ++u) {
      const int j = used[u];
      if (u + 1 < used.size()) load(u + 1);
      std::vector<std::vector<int>> rows(rl_of.size());
      for (size_t i = 0; i < rl_of.size(); ++i) {
        const uint32_t m = masks[static_cast<size_t>(rl_of[i]) * K + j];
        for (int x = 0; x < W; ++x)
          if ((m >> x) & 1u) rows[i].push_back(x);
      }
      const std::vector<std::pair<int, int>> pairs = share_pairs(rows, W, variant().slice_pair_cap);
      const std::string eb = "e" + std::to_string(u % 2) + "_";
      auto nm = [&](int x) { return x < W ? eb + std::to_string(x) + "[d]" : "p" + std::to_string(x - W); };
      s << "      for (int d = 0; d < D; ++d) {\n";
      for (size_t i = 0; i < pairs.size(); ++i)
        s << "        const u32 p" << i << " = " << nm(pairs[i].first) << " ^ " << nm(pairs[i].second) << ";\n";
      for (size_t i = 0; i < rl_of.size(); ++i) {
        if (rows[i].empty()) continue;
        const int rl = rl_of[i];
        const std::string acc = "h" + std::to_string(rl / W) + "_" + std::to_string(rl % W - l0) + "[d]";
        std::vector<std::string> t;
        if (live[rl]) t.push_back(acc);
        for (int x : rows[i]) t.push_back(nm(x));
        s << "        " << acc << " = " << xor_chain(t) << ";\n";
        live[rl] = true;
      }
      s << "      }\n      __builtin_amdgcn_sched_barrier(0);\n";
    }
    for (int r = 0; r < R; ++r) {
      s << "      { const unsigned long long q = " << shard(A, "out", r) << " + off;\n";
      for (int l = l0; l < l1; ++l) {
        if (!live[static_cast<size_t>(r) * W + l]) s << "        for (int d = 0; d < D; ++d) h" << r << "_" << l - l0 << "[d] = 0u;\n";
        s << "        st(h" << r << "_" << l - l0 << ", q + " << l << "ull * P);\n";
      }
      s << "      }\n";
    }
    s << "    }\n";
  }
  s << "  }\n}\n";
  return s.str();
}

}  // namespace jit
}  // namespace lsec
