// ec_kernels.h -- launch interface of the gfx950 erasure kernels (internal to liblstore_ec).
//
// Both kernels compute the same thing -- R output shards as GF(2^8)-linear combinations
// of K input shards, out_r = sum_j A[r][j] * in_j -- for every stripe of a batch.  They
// differ in how a shard's bytes map onto field elements:
//
//   gf8_bytewise   each byte is one element (Reed-Solomon "matrix" codes:
//                  jerasure_matrix_encode/_decode, jerasure.c:301, :169)
//   gf8_bitsliced  each shard is a sequence of super-packets of 8 packets of P bytes;
//                  bit b of byte t of packet x is bit x of element (t, b) (Cauchy
//                  "bitmatrix/schedule" codes: jerasure_schedule_encode, jerasure.c:1193,
//                  jerasure_schedule_decode_lazy, :953)
//
// Shard addressing per stripe s:  in_j = in[j].base + s * in[j].stride  (same for out),
// so a batch can describe LStore's layout (k data chunks back to back in one cache page,
// m parity chunks in a parity buffer) or any other strided layout without a pointer table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <type_traits>
#include <utility>

namespace lsec {

// Launches kernel k and returns the launch's own status (hipLaunchKernel's return value).  The
// engine never reads the runtime's per-thread last error to learn about its launches: that error
// is sticky until read, so a read would both take a caller's pending error for the engine's and
// clear it from under the caller.
template <typename T, size_t... I>
hipError_t launch_packed(const void *k, dim3 grid, dim3 block, hipStream_t st, T &args, std::index_sequence<I...>) {
  void *ptrs[] = {static_cast<void *>(&std::get<I>(args))..., nullptr};
  return hipLaunchKernel(k, grid, block, ptrs, 0, st);
}
template <typename... KArgs, typename... Args>
hipError_t launch_kernel(void (*k)(KArgs...), dim3 grid, dim3 block, hipStream_t st, const Args &...args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count");
  std::tuple<std::decay_t<KArgs>...> t(static_cast<std::decay_t<KArgs>>(args)...);
  return launch_packed(reinterpret_cast<const void *>(k), grid, block, st, t, std::index_sequence_for<KArgs...>{});
}

// Occupancy cap of the streaming launches (launch_tiled's kernels and the compiled networks), as
// unused dynamic LDS per workgroup: with it at most n workgroups share a CU's 160 KiB.  0 (the
// default, or n = 0): no cap.  n from LSEC_WGS_CAP for launches whose shards are at least
// LSEC_WGS_CAP_MIN_KB apart (A/B runs of the C = 8 MiB encode dip).
size_t occupancy_lds_bytes(int64_t shard_bytes);
template <typename T, size_t... I>
hipError_t launch_packed_shm(const void *k, dim3 grid, dim3 block, size_t shm, hipStream_t st, T &args,
                             std::index_sequence<I...>) {
  void *ptrs[] = {static_cast<void *>(&std::get<I>(args))..., nullptr};
  return hipLaunchKernel(k, grid, block, ptrs, shm, st);
}
template <typename... KArgs, typename... Args>
hipError_t launch_kernel_shm(void (*k)(KArgs...), dim3 grid, dim3 block, size_t shm, hipStream_t st, const Args &...args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count");
  std::tuple<std::decay_t<KArgs>...> t(static_cast<std::decay_t<KArgs>>(args)...);
  return launch_packed_shm(reinterpret_cast<const void *>(k), grid, block, shm, st, t, std::index_sequence_for<KArgs...>{});
}

constexpr int kMaxK = 64;   // input shards per launch (wider stripes: several launches, the later ones with
                            // ApplyArgs::accumulate, over images in the grouped layout below)
constexpr int kMaxR = 16;   // output shards per launch
constexpr int kMaxW = 257;  // bitmatrix word size w (packets per super-packet) the kernels accept:
                             // every liberation-family plan with k + m <= 256 (liberation k = 252..254
                             // gets w = 257, erasure_tools.c:756-757)

// Matrix images of stripes wider than kMaxK inputs are stored in groups of kMaxK input columns:
// group g (inputs g*kMaxK ..) holds every row's cells / masks / products for its columns, rows in
// order, so one launch per group reads a plain row-major image of its K_g columns.
__host__ __device__ inline int image_groups(int K) { return (K + kMaxK - 1) / kMaxK; }
// 32-bit words per bitmatrix mask: bit x of mask word q covers packet 32q + x of an input
__host__ __device__ inline int mask_words(int w) { return (w + 31) / 32; }

struct ShardRef {
  uint64_t base;    // device address of this shard in stripe 0
  int64_t stride;   // bytes between consecutive stripes
};

// One coefficient cell of the device "matrix image": 8 dwords, 32-byte aligned so a
// wave fetches it with one scalar load.  For bytewise kernels the three 8-entry
// product tables implement  c*v = Ta[v & 7] ^ Tb[(v >> 3) & 7] ^ Tc[v >> 6]  with one
// v_perm_b32 each (v_perm selects bytes from an 8-byte table).
constexpr uint32_t kCellXorRow = 1;  // CoefCell::pad of a row's first cell: every coefficient of the row is 1

struct CoefCell {
  uint32_t coef;        // A[r][j] (0..255)
  uint32_t pad;         // flags (kCellXorRow in the first cell of a row)
  uint32_t ta_lo, ta_hi;  // c * {0..7}
  uint32_t tb_lo, tb_hi;  // c * {0,8,..,56}
  uint32_t tc_lo, tc_hi;  // c * {0,64,128,192}, upper 4 bytes unused
};
static_assert(sizeof(CoefCell) == 32, "CoefCell must be 32 bytes");

struct ApplyArgs {
  const CoefCell *cells;  // R x K, row-major (device memory)
  int K, R;
  int nstripes;
  int packet;             // bitsliced / bitmatrix: packet size P (bytes)
  int64_t size;           // bytes per shard (chunk C)
  const uint32_t *masks;  // bitmatrix: (R*w) x K x mask_words(w) words, bit x of [((r*w+l)*K + j)*NW + q]
                          //   = B[r*w+l][j*w + 32q + x]
                          // wordwise: R x K x w products, [(r*K + j)*w + b] = c_rj * x^b
  int w;                  // bitmatrix: packets per super-packet; wordwise: field width (16 / 32)
  int accumulate;         // 1: out[r] ^= the result (the second and later input groups of a wide stripe)
  unsigned long long *magic_acc;  // encode only (bytewise, bitsliced): fused stripe magic over the K inputs then the
                                  // R outputs (2 x u64 per stripe, zeroed), see MagicArgs
  unsigned *tiles;        // work-sharing tile queue slot (tile_queue_slot), or null: each XCD its static eighth
  uint32_t tiles_pre;     // with a slot: the tiles of each eighth dealt statically before the sharing starts
  unsigned long long *stamps;  // measurement only (lsec_test_set_stamps): each workgroup's end time, or null
  uint32_t nstamps;
  uint32_t tile_phase;    // XCD tile phase (tile_phase_on): XCD x starts its eighth x * tile_phase tiles on, 0 = off
  ShardRef in[kMaxK];
  ShardRef out[kMaxR];
};

// Per-stripe erasure patterns (lsec_decode_dev_patterns / _rotated): one launch decodes stripes
// that do not share an erasure pattern.  A tile belongs to one stripe; the kernel looks the
// stripe's pattern up once per tile and takes the matrix, the input shards and the output shards
// from that pattern's record.  The table (records + one CoefCell[Rmax][K] image per pattern, Rmax
// the largest erasure count of the table, rows past a pattern's own count zero cells) lives in
// device memory and is read through the constant address space; the shard refs travel in the
// kernel arguments, indexed by the record's selection lists.
constexpr int kPatMaxOut = 8;        // erasures per pattern
constexpr int kPatMaxShards = 128;   // k + m of a patterned call (the shard refs are kernel arguments)
constexpr int kPatMaxPatterns = 256; // patterns per table (stripe_pattern holds bytes)

struct alignas(64) PatRecord {
  uint32_t nout;               // erasure count; 0: the stripe is neither read nor written
  uint32_t cells_off;          // first cell of the pattern's CoefCell[Rmax][K] image in PatternArgs::cells
  uint32_t pad[2];
  uint32_t in_sel[kMaxK];      // PatternArgs::sh index of input j (the pattern's j-th survivor; nout 0: data chunk j,
                               // which only the MG kernels look at)
  uint32_t out_sel[kPatMaxOut];  // PatternArgs::sh index of output r (its r-th erased chunk)
};
static_assert(sizeof(PatRecord) == 320, "PatRecord layout");

// An argument struct of its own: ApplyArgs, which every other launch passes by value, stays as it is.
struct PatternArgs {
  const PatRecord *recs;       // npat records (device memory)
  const CoefCell *cells;       // the patterns' images (device memory)
  const uint8_t *stripe_pattern;  // nstripes pattern ids (device memory), or null: the rotation below
  uint32_t npat;               // records in the table; a stripe whose id is >= npat is left alone
  uint32_t rot0, rot_step, rot_n;  // stripe_pattern null: stripe s has pattern (rot0 + s * rot_step) mod rot_n
  int K;
  int nstripes;
  int packet;                  // bit-sliced: packet size P (bytes)
  int nshards;                 // entries of sh in use
  int64_t size;                // bytes per shard (chunk C)
  unsigned *tiles;             // as ApplyArgs
  uint32_t tiles_pre;
  uint32_t tile_phase;
  ShardRef sh[kPatMaxShards];  // the call's shards
};

// rmax = the table's largest erasure count (1..kPatMaxOut): the kernel's output rows
hipError_t launch_pattern_bytewise(const PatternArgs &a, int rmax, hipStream_t stream);
hipError_t launch_pattern_bitsliced(const PatternArgs &a, int rmax, hipStream_t stream);

// The patterned decode that also leaves each stripe's adler32 magic (lsec_decode_magic_dev_patterns /
// _rotated): the paranoid read's "rebuild, then the checksum over all k+m chunks" in one pass.  A
// tile holds the K survivors it loads and the rows it forms in registers; the MG kernels
// (k_patmagic_*: the patterned tile bodies under `if constexpr (MG)`) sum those into one MagicLane at
// their LOGICAL chunk ids, load the survivors the decode does not read -- the pattern's PatUnused
// list, a device array parallel to recs and in in_sel's index space -- for the checksum alone, and
// commit once per tile into magic_acc[2s], [2s + 1] (zeroed before the first launch).  A record whose
// nout is 0 names the K data chunks in in_sel and the parity in its PatUnused: the checksum-only
// path, K + m reads and no write.  Logical ids: the selection itself with a stripe_pattern (the
// shards are logical chunks), (sel + p) mod nshards without one (the records of rotation p hold
// physical devices).  launch_pattern_magic_finalize folds the sums into the magic words.  The struct
// derives from PatternArgs, whose layout -- and PatRecord's, and with them every k_pat_* and
// k_patrot_* kernel -- stays as it is.
constexpr int kPatMaxUnused = 8;     // survivors a pattern's decode does not read: m - nout <= m <= 8
struct alignas(16) PatUnused {
  uint32_t n;                        // entries of sel in use
  uint32_t pad[3];
  uint32_t sel[kPatMaxUnused];       // PatternArgs::sh indices, ascending by logical id
};
static_assert(sizeof(PatUnused) == 48, "PatUnused layout");

struct PatternMagicArgs : PatternArgs {
  const PatUnused *unused;        // npat records (device memory)
  unsigned long long *magic_acc;  // 2 per stripe of this launch (8-byte aligned device memory)
};
static_assert(sizeof(PatternMagicArgs) == sizeof(PatternArgs) + 16, "PatternMagicArgs layout");
static_assert(sizeof(PatternMagicArgs) < 4096, "PatternMagicArgs: under the 4 KiB of kernel arguments");

// As launch_pattern_*, with unused and magic_acc != NULL and nshards - K <= kPatMaxUnused; rmax >= 1
// also for a table whose patterns are all empty (its tiles only checksum).  The launch shapes are the
// patterned kernels' own (patmagic_bytewise_form).
hipError_t launch_pattern_magic_bytewise(const PatternMagicArgs &a, int rmax, hipStream_t stream);
hipError_t launch_pattern_magic_bitsliced(const PatternMagicArgs &a, int rmax, hipStream_t stream);
// One launch per call, behind the tile launches, one thread per stripe of the whole call.  A stripe
// whose stripe_pattern id (stripe_pattern may be null: none is skipped) is >= npat: its magic word is
// neither read nor written and bad[s] = 0.  Every other: the 4 little-endian bytes at magic + 4s (no
// alignment) become A = (1 + acc[2s]) mod 65521, B = (total_len + acc[2s + 1]) mod 65521; with expect
// (may be null; 4 bytes per stripe, no alignment) bad[s] (may be null) = the words differ, and
// bad_count (may be null; zeroed by the caller) counts them.
hipError_t launch_pattern_magic_finalize(const unsigned long long *acc, const uint8_t *stripe_pattern, uint32_t npat,
                                         int nstripes, int64_t total_len, uint8_t *magic, const uint8_t *expect,
                                         uint8_t *bad, unsigned *bad_count, hipStream_t stream);

// The search for the erasure set that fits the quorum magic (lsec_search_dev_patterns / _rotated): LStore's
// jerase_brute_recovery over device-resident stripes, every candidate of every selected stripe tried in one
// pass.  A trial of candidate p on stripe s is the MG tile of pattern p with its stores left out: the
// survivors it loads, the rows it forms and the unused survivors it loads for the sum give the magic the
// stripe would have after that decode, and nothing is written.  The SR kernels (k_patsearch_*: the patterned
// tile bodies under `if constexpr (SR)`) take one tile per (stripe, candidate, piece of the chunk) -- p from
// the tile index, never from stripe_pattern, which stays null -- skip every stripe whose select byte is 0
// before any of its chunks is read, and commit into magic_acc[2(s * npat + p)], [.. + 1]: 16 bytes per
// (stripe, candidate), zeroed before the first launch.  cand_outer picks the tile order (0: the candidate
// innermost), plain_loads the load kind (0: non-temporal, as the decode's; 1: plain, which ships).  The table is the logical one of
// lsec_decode_dev_patterns for the same list; the rotated struct turns every selection into a physical
// device per stripe as PatternRotArgs does (rot0 / rot_step / rot_n), and the magic ids are the selections
// themselves.  launch_pattern_search_finalize folds the sums, writes trial and found and counts.  The
// structs derive from PatternMagicArgs, whose layout stays as it is.
struct PatternSearchArgs : PatternMagicArgs {
  const uint8_t *select;   // nstripes bytes (device memory), or null: every stripe is searched
  uint32_t cand_outer;     // tile order: 0 the candidate innermost, 1 the piece innermost
  uint32_t plain_loads;    // 0: non-temporal loads, 1: plain ones (host side: selects the kernel)
};
struct PatternSearchRotArgs : PatternSearchArgs {};  // the type only selects the kernels (PatShards)
static_assert(sizeof(PatternSearchArgs) == sizeof(PatternMagicArgs) + 16, "PatternSearchArgs layout");
static_assert(sizeof(PatternSearchRotArgs) < 4096, "PatternSearchArgs: under the 4 KiB of kernel arguments");

// The MG kernels over the k+m devices of a rotated LUN with a logical pattern per stripe
// (lsec_decode_magic_dev_patterns_rotated): the logical table of lsec_decode_dev_patterns, a stripe_pattern,
// and rot0 / rot_step / rot_n = nshards as PatternRotArgs has them, so that logical chunk c of stripe s is
// sh[(c - rot_s) mod nshards].  The magic ids are the selections themselves.  The type only selects the
// kernels (PatShards); the launch shapes are a constant of their own (patmagicrot_bytewise_form).
struct PatternMagicRotArgs : PatternMagicArgs {};
hipError_t launch_pattern_magic_rot_bytewise(const PatternMagicRotArgs &a, int rmax, hipStream_t stream);
hipError_t launch_pattern_magic_rot_bitsliced(const PatternMagicRotArgs &a, int rmax, hipStream_t stream);

// As launch_pattern_magic_*, over npat candidates per stripe: nstripes * npat * (tiles per chunk) < 2^31,
// stripe_pattern null; the rotated struct with rot_n = nshards.  The launch shapes are the MG forms' own
// (patsearch_bytewise_form).
template <typename Args>
hipError_t launch_pattern_search_bytewise(const Args &a, int rmax, hipStream_t stream);
template <typename Args>
hipError_t launch_pattern_search_bitsliced(const Args &a, int rmax, hipStream_t stream);
// One launch per call, behind the tile launches, one thread per stripe of the whole call.  A stripe with
// select[s] == 0 (select may be null): found[s] = kLocateClean and nothing else of it is touched.  Every
// other: for p = 0 .. npat - 1 the word A = (1 + acc[2q]) mod 65521, B = (total_len + acc[2q + 1]) mod 65521,
// q = s * npat + p, goes to the 4 little-endian bytes at trial + 4q (trial may be null; no alignment);
// found[s] = the first p whose word equals the 4 bytes at expect + 4s (no alignment), or kLocateMany.
// counts (may be null; two words, zeroed by the caller): [0] the stripes found, [1] the kLocateMany ones.
hipError_t launch_pattern_search_finalize(const unsigned long long *acc, const uint8_t *select, uint32_t npat, int nstripes,
                                          int64_t total_len, const uint8_t *expect, uint8_t *found, uint8_t *trial,
                                          unsigned *counts, hipStream_t stream);

// Parity check of device-resident stripes (lsec_check_dev): one streaming pass forms the R parity
// rows of every stripe in registers, as the encode kernels do, and compares them with the stored
// parity chunks instead of storing them.  Bit r of syndrome[s] is set when row r of stripe s
// differs anywhere; bad_count (may be null) counts the stripes whose word became nonzero.  Both
// are zeroed by the caller (scrub_dev's hipMemsetAsync, ahead of the kernel on the same stream):
// the kernels only ever OR bits in, one returning atomic per wave that found a difference, and
// the wave whose atomic returns 0 -- the first to make the word nonzero, so exactly one per bad
// stripe -- counts the stripe.  A clean wave writes nothing.  An argument struct of its own:
// ApplyArgs and PatternArgs stay as they are.
struct CheckArgs {
  const CoefCell *cells;  // the encode image, R x K, row-major (device memory)
  int K, R;
  int nstripes;
  int packet;             // bit-sliced: packet size P (bytes)
  int64_t size;           // bytes per shard (chunk C)
  unsigned *syndrome;     // nstripes words (device memory, zeroed)
  unsigned *bad_count;    // one word (device memory, zeroed), or null
  unsigned *tiles;        // as ApplyArgs
  uint32_t tiles_pre;
  uint32_t tile_phase;
  ShardRef in[kMaxK];     // the data chunks
  ShardRef par[kMaxR];    // the stored parity chunks (only read)
};

// Locating the corrupt chunk (lsec_locate_dev): the check's pass, whose per-row differences
// S_r = (row r re-formed from the stored data) ^ (stored parity r) are the stripe's syndromes.  One
// wrong data chunk j gives S_r = Q[r-1][j] * S_0 at every byte column, Q[r-1][j] = g[r][j] / g[0][j]
// (the ratio image); one wrong parity chunk r gives S_r alone.  A wave that saw a difference tests
// every j < K over its lanes' words, ORs its row mask into syndrome[s] and ANDs the k-bit mask of
// the hypotheses that held into hyp[s]; a clean wave issues nothing.  The caller has set syndrome
// to 0 and hyp to all ones on the stream ahead of the launch.  CheckArgs' fields mean what they
// mean to the check (bad_count is unused: the finalize launch counts).
struct LocateArgs : CheckArgs {
  const CoefCell *ratio;      // (R - 1) x K, row-major (device memory): Q
  unsigned long long *hyp;    // nstripes words (device memory, all ones)
};


constexpr unsigned kLocateClean = 0xFF, kLocateMany = 0xFE;  // LSEC_LOCATE_CLEAN / _MANY (lstore_ec.h)

// One thread per stripe, behind the accumulate launches: masks hyp[s] to K bits, writes located[s]
// (kLocateClean, K + r, j or kLocateMany: the rules of lsec_locate_dev) and, with counts, adds the
// located stripes to counts[0] and the kLocateMany ones to counts[1] (zeroed by the caller).
hipError_t launch_locate_finalize(const unsigned *syndrome, unsigned long long *hyp, unsigned char *located,
                                  unsigned *counts, int nstripes, int K, int R, hipStream_t stream);

// Check, locate and repair over the physical devices of a rotated LUN (lsec_check_dev_rotated /
// lsec_locate_dev_rotated).  The arithmetic, the tile loops and the launch shapes are the check's
// and the locate's; what differs is where a tile takes its shard refs from.  With
// rot_s = (rot0 + s * rot_step) mod rot_n the rotation of stripe s, logical chunk c (data chunk j:
// c = j, parity row r: c = K + r) is read from sh[(c - rot_s) mod rot_n].  s is uniform over the
// workgroup, so rot_s and the index stay scalar and the refs come by dynamic-offset scalar loads
// from the kernel arguments, as the patterned decode takes its refs.  Argument structs of their
// own: CheckArgs, LocateArgs and PatternArgs keep their layout.
constexpr int kRotMaxShards = kMaxK + 8;  // k <= kMaxK data chunks, m <= 8 parity rows
struct CheckRotArgs {
  const CoefCell *cells;  // as CheckArgs, up to tile_phase
  int K, R;
  int nstripes;
  int packet;
  int64_t size;
  unsigned *syndrome;
  unsigned *bad_count;
  unsigned *tiles;
  uint32_t tiles_pre;
  uint32_t tile_phase;
  uint32_t rot0, rot_step, rot_n;  // rot0, rot_step < rot_n = K + R
  ShardRef sh[kRotMaxShards];      // the K + R physical devices
};

struct LocateRotArgs : CheckRotArgs {
  const CoefCell *ratio;      // as LocateArgs
  unsigned long long *hyp;
};

// The check that also leaves each stripe's adler32 magic (lsec_check_magic_dev / _rotated): the scrub's
// "is the parity consistent" and "are these the bytes that were written" from one read of the k + m
// chunks.  A check tile holds every byte of its part of the stripe in registers -- the K data units
// as they are loaded and the R stored parity units -- so the MG kernels (k_chkmagic_*, k_chkmagicrot_*:
// the check's tile bodies under `if constexpr (MG)`) sum them into one MagicLane at their LOGICAL chunk
// ids (j, K + r; for the rotated struct whatever device ChkShards fetched them from) and commit once
// per tile into magic_acc[2s], [2s + 1] (zeroed before the first launch).  The syndrome words are the
// check's.  The tile launches are given no bad_count: launch_check_magic_finalize folds the sums into
// the magic words, compares and counts.  The structs derive from CheckArgs / CheckRotArgs, whose
// layouts -- and with them every k_chk_*, k_loc_* kernel -- stay as they are.
struct CheckMagicArgs : CheckArgs {
  unsigned long long *magic_acc;  // 2 per stripe of this launch (8-byte aligned device memory)
};
struct CheckMagicRotArgs : CheckRotArgs {
  unsigned long long *magic_acc;  // as CheckMagicArgs
};
static_assert(sizeof(CheckMagicArgs) == sizeof(CheckArgs) + 8, "CheckMagicArgs layout");
static_assert(sizeof(CheckMagicRotArgs) == sizeof(CheckRotArgs) + 8, "CheckMagicRotArgs layout");
static_assert(sizeof(CheckMagicArgs) < 4096 && sizeof(CheckMagicRotArgs) < 4096,
              "CheckMagicArgs / CheckMagicRotArgs: under the 4 KiB of kernel arguments");

// As launch_scrub_*, and magic_acc != NULL.  The launch shapes are chkmagic_bytewise_form and the
// check's lane dwords.
template <typename Args>
hipError_t launch_check_magic_bytewise(const Args &a, hipStream_t stream);
template <typename Args>
hipError_t launch_check_magic_bitsliced(const Args &a, hipStream_t stream, int dw_pref = 0);
constexpr unsigned kScrubBadParity = 1, kScrubBadMagic = 2;  // LSEC_SCRUB_BAD_PARITY / _MAGIC (lstore_ec.h)
// One launch per call, behind the tile launches, one thread per stripe of the whole call: the 4
// little-endian bytes at magic + 4s (no alignment) become A = (1 + acc[2s]) mod 65521,
// B = (total_len + acc[2s + 1]) mod 65521.  bad[s] (may be null; no alignment) = kScrubBadParity when
// syndrome[s] != 0, | kScrubBadMagic when expect (may be null; 4 bytes per stripe, no alignment) is
// given and differs from the word.  counts (may be null; two words, zeroed by the caller): [0] the
// stripes with a nonzero syndrome, [1] those whose magic differs from expect.
hipError_t launch_check_magic_finalize(const unsigned long long *acc, const unsigned *syndrome, int nstripes,
                                       int64_t total_len, uint8_t *magic, const uint8_t *expect, uint8_t *bad,
                                       unsigned *counts, hipStream_t stream);

// What tells the argument structs apart, to the host's launch path and to the kernels' tile
// bodies alike: a locate struct adds ratio and hyp, a rotated one takes its refs from sh.
template <typename Args>
constexpr bool kLocArgs = std::is_same<Args, LocateArgs>::value || std::is_same<Args, LocateRotArgs>::value;
struct EncodeRotArgs;
struct EncodeMagicRotArgs;
struct UpdateRotArgs;
template <typename Args>
constexpr bool kRotArgs = std::is_base_of<CheckRotArgs, Args>::value || std::is_same<Args, EncodeRotArgs>::value ||
                          std::is_same<Args, EncodeMagicRotArgs>::value || std::is_same<Args, UpdateRotArgs>::value;

// The accumulate launch of a check or locate, for each of CheckArgs, LocateArgs, CheckRotArgs and
// LocateRotArgs.  R <= 8 (a locate: 2 <= R); the launch shape is the encode's for the same K x R
// (bytewise_shape's automatic policy), and a locate's and a rotated form's are the check's.
template <typename Args>
hipError_t launch_scrub_bytewise(const Args &a, hipStream_t stream);
// dw_pref: dwords per lane (1, 2, 4; 0 = 1), as launch_bitsliced
template <typename Args>
hipError_t launch_scrub_bitsliced(const Args &a, hipStream_t stream, int dw_pref = 0);
// launch_locate_finalize's verdict, and with it the physical device of each located chunk:
// located_dev[s] (may be null) = (located[s] - rot_s) mod rot_n, both sentinels passed through, and
// one atomic add per located stripe into dev_faults[located_dev[s]] (may be null; rot_n words,
// zeroed by the caller).
hipError_t launch_locate_finalize_rot(const unsigned *syndrome, unsigned long long *hyp, unsigned char *located,
                                      unsigned char *located_dev, unsigned *counts, unsigned *dev_faults, int nstripes,
                                      int K, int R, uint32_t rot0, uint32_t rot_step, uint32_t rot_n, hipStream_t stream);

// The rotated single-erasure repair: the patterned decode over the k+m single-erasure table of
// logical chunks (record c rebuilds logical chunk c from its logical survivors), each stripe's
// pattern id read from stripe_pattern (the locate's `located`), and every selection of the record
// turned into a physical device per stripe: sh index = (sel - rot_s) mod rot_n, rot_s from rot0 /
// rot_step / rot_n as above.  So n records serve every rotation, where a table of (rotation x
// chunk) records would pass kPatMaxPatterns at RS(16+4).  The type only selects the kernels.
struct PatternRotArgs : PatternArgs {};
// one output row per pattern (single erasures)
hipError_t launch_pattern_rot_bytewise(const PatternRotArgs &a, hipStream_t stream);
hipError_t launch_pattern_rot_bitsliced(const PatternRotArgs &a, hipStream_t stream);
// The same kernels over any logical table with a stripe_pattern (the repair behind a rotated search, whose
// stripe_pattern is the search's `found`): rmax = the table's largest erasure count, 1..kPatMaxOut.
hipError_t launch_pattern_rot_rows_bytewise(const PatternRotArgs &a, int rmax, hipStream_t stream);
hipError_t launch_pattern_rot_rows_bitsliced(const PatternRotArgs &a, int rmax, hipStream_t stream);

// Parity update for partial-stripe writes (lsec_update_dev): c of a stripe's K data chunks change
// from old_i to fresh_i, and the code is linear, so every parity row r takes
//   par_r ^= sum_i cells[r][col[i]] * (old_i ^ fresh_i)
// (for Cauchy the bit-sliced product over packets, as the encode forms it).  One streaming pass
// reads 2c + R chunks of a stripe and writes R, or R + c with `store`, which also puts the fresh
// bytes over the old ones from the registers that hold them.  Only the changed chunks and the
// parity travel here: a data chunk that does not change has no ref in the struct, so no kernel can
// read it.  cells is the plan's cached encode image, indexed by column: nothing is uploaded per
// call.  An argument struct of its own: ApplyArgs, PatternArgs and the four scrub structs keep
// their layout.
struct UpdateArgs {
  const CoefCell *cells;  // the encode image, R x K, row-major (device memory)
  int K, R;
  int c;                  // changed chunks, 1..K
  int nstripes;
  int packet;             // bit-sliced: packet size P (bytes)
  int store;              // != 0: old[i] <- fresh[i] in the same pass
  int64_t size;           // bytes per shard (chunk C)
  unsigned *tiles;        // as ApplyArgs
  uint32_t tiles_pre;
  uint32_t tile_phase;
  alignas(4) uint8_t col[kMaxK];  // data chunk id of changed chunk i (distinct, < K)
  ShardRef old[kMaxK];    // the changed chunks as stored (read; written with store)
  ShardRef fresh[kMaxK];  // their new contents (only read)
  ShardRef par[8];        // the parity chunks (read and written)
};

// R <= 8, 1 <= c <= K <= kMaxK, every col[i] < K.  The launch shapes are the update's own
// (upd_bytewise_form: they depend on R alone, the columns being walked at run time).
hipError_t launch_update_bytewise(const UpdateArgs &a, hipStream_t stream);
// dw_pref: dwords per lane (1, 2, 4; 0 = 1), as launch_bitsliced
hipError_t launch_update_bitsliced(const UpdateArgs &a, hipStream_t stream, int dw_pref = 0);

// Encode and parity update over the physical devices of a rotated LUN (lsec_encode_dev_rotated /
// lsec_update_dev_rotated): the write side of what CheckRotArgs reads.  The refs are the K + R
// devices, and a tile finds logical chunk c of its stripe in sh[(c - rot_s) mod rot_n], rot_s from
// rot0 / rot_step / rot_n exactly as the rotated check works it out (rot_back, ChkShards): scalar
// arithmetic and dynamic-offset scalar loads from the kernel arguments.  Argument structs of their
// own: every other struct keeps its layout.
//
// The encode forms the R parity rows of every stripe from the K logical data chunks, as the check
// does, and stores them where the check would load and compare: to sh[(K + r - rot_s) mod rot_n].
// The data chunks are only read.
struct EncodeRotArgs {
  const CoefCell *cells;  // the encode image, R x K, row-major (device memory)
  int K, R;
  int nstripes;
  int packet;             // bit-sliced: packet size P (bytes)
  int64_t size;           // bytes per shard (chunk C)
  unsigned *tiles;        // as ApplyArgs
  uint32_t tiles_pre;
  uint32_t tile_phase;
  uint32_t rot0, rot_step, rot_n;  // rot0, rot_step < rot_n = K + R
  ShardRef sh[kRotMaxShards];      // the K + R physical devices
};

// UpdateArgs with old[] and par[] replaced by the devices: old_i is read from (and with `store`
// written to) sh[(col[i] - rot_s) mod rot_n], parity row r is sh[(K + r - rot_s) mod rot_n].  fresh is
// logical and not rotated.  The chunks that do not change have refs here -- under rotation every
// device holds a changed chunk in some stripe -- but no kernel forms an address from them in a
// stripe where they do not change.
struct UpdateRotArgs {
  const CoefCell *cells;  // as UpdateArgs, up to col
  int K, R;
  int c;
  int nstripes;
  int packet;
  int store;
  int64_t size;
  unsigned *tiles;
  uint32_t tiles_pre;
  uint32_t tile_phase;
  uint32_t rot0, rot_step, rot_n;  // rot0, rot_step < rot_n = K + R
  alignas(4) uint8_t col[kMaxK];
  ShardRef fresh[kMaxK];           // the new contents of the changed chunks (only read)
  ShardRef sh[kRotMaxShards];      // the K + R physical devices
};
static_assert(sizeof(UpdateRotArgs) == 2312, "UpdateRotArgs: well under the 4 KiB of kernel arguments");
static_assert(sizeof(EncodeRotArgs) == 1216, "EncodeRotArgs layout");

// R <= 8.  The encode's launch shape is the rotated check's for the same K x R (chk_bytewise_form,
// scrub_lane_dwords), the update's is the unrotated update's (upd_bytewise_form, update_lane_dwords).
hipError_t launch_encode_rot_bytewise(const EncodeRotArgs &a, hipStream_t stream);
hipError_t launch_encode_rot_bitsliced(const EncodeRotArgs &a, hipStream_t stream, int dw_pref = 0);
hipError_t launch_update_rot_bytewise(const UpdateRotArgs &a, hipStream_t stream);
hipError_t launch_update_rot_bitsliced(const UpdateRotArgs &a, hipStream_t stream, int dw_pref = 0);

// The rotated encode that also leaves each stripe's adler32 magic (lsec_encode_magic_dev_rotated): the
// full-stripe write of a rotated LUN and the word LStore stores in front of every chunk, from k chunk
// reads and m chunk writes.  An encode tile holds every byte of its part of the stripe in registers --
// the K data units as they are loaded and the R rows as they are formed -- so the MG kernels
// (k_encmagicrot_*: the rotated encode's tile bodies under `if constexpr (MG)`) sum them into one
// MagicLane at their LOGICAL chunk ids (j, K + r, whatever device ChkShards fetched or stores them at)
// and commit once per tile into magic_acc[2s], [2s + 1] (zeroed before the first launch);
// launch_magic_finalize folds the sums into the magic words.  The struct derives from EncodeRotArgs,
// whose layout -- and with it every k_encrot_* kernel -- stays as it is.
struct EncodeMagicRotArgs : EncodeRotArgs {
  unsigned long long *magic_acc;  // 2 per stripe of this launch (8-byte aligned device memory)
};
static_assert(sizeof(EncodeMagicRotArgs) == sizeof(EncodeRotArgs) + 8, "EncodeMagicRotArgs layout");
static_assert(sizeof(EncodeMagicRotArgs) < 4096, "EncodeMagicRotArgs: under the 4 KiB of kernel arguments");

// As launch_encode_rot_*, and magic_acc != NULL.  The launch shapes are encmagicrot_bytewise_form and
// encode_magic_rot_lane_dwords: the rotated encode's.
hipError_t launch_encode_magic_rot_bytewise(const EncodeMagicRotArgs &a, hipStream_t stream);
hipError_t launch_encode_magic_rot_bitsliced(const EncodeMagicRotArgs &a, hipStream_t stream, int dw_pref = 0);

// The parity update with a changed set per stripe (lsec_update_dev_masked / _masked_rotated): bit j of
// stripe_cols[s] says that data chunk j of stripe s changes.  One kernel family and one struct for
// both calls: the refs are the K + R devices as in UpdateRotArgs, and the unrotated call passes its
// logical chunks with rot_step = 0, which makes every rotation 0.  fresh is indexed by logical chunk
// id (fresh[j] goes with chunk j, not with a list position).  A tile reads its stripe's word through
// a uniform address, ANDs it with `allowed` -- the columns that have a fresh buffer, below K -- and
// on 0 touches nothing more; otherwise it walks the set bits, lowest first, as the update walks
// col[].  So no address is ever formed from fresh[j] or from a chunk's ref for a j outside
// `allowed`: those entries are zero here.  Argument struct of its own: every other struct keeps its
// layout.
struct UpdateMaskArgs {
  const CoefCell *cells;  // the encode image, R x K, row-major (device memory)
  int K, R;
  int nstripes;
  int packet;             // bit-sliced: packet size P (bytes)
  int store;              // != 0: old_j <- fresh_j in the same pass
  int64_t size;           // bytes per shard (chunk C)
  unsigned *tiles;        // as ApplyArgs
  uint32_t tiles_pre;
  uint32_t tile_phase;
  uint32_t rot0, rot_step, rot_n;  // rot0, rot_step < rot_n = K + R; the unrotated call: 0, 0
  unsigned long long allowed;      // bit j: fresh[j] is there and j < K
  const unsigned long long *stripe_cols;  // nstripes words (device memory, only read)
  ShardRef fresh[kMaxK];           // by logical chunk id (only read)
  ShardRef sh[kRotMaxShards];      // the K + R physical devices (unrotated: the logical chunks)
};
static_assert(sizeof(UpdateMaskArgs) == 2264, "UpdateMaskArgs layout");
static_assert(sizeof(UpdateMaskArgs) < 4096, "UpdateMaskArgs: under the 4 KiB of kernel arguments");

// R <= 8, K <= kMaxK, allowed != 0 with no bit at or above K.  The launch shapes are the masked
// update's own (updmask_bytewise_form, update_masked_lane_dwords): they depend on R alone.
hipError_t launch_update_masked_bytewise(const UpdateMaskArgs &a, hipStream_t stream);
hipError_t launch_update_masked_bitsliced(const UpdateMaskArgs &a, hipStream_t stream, int dw_pref = 0);

// The masked update that also keeps the stripes' adler32 magics current (lsec_update_magic_dev_masked /
// _masked_rotated).  A write changes the magic's two halves by sums over the changed positions alone,
//   dA = sum (new_p - old_p),  dB = sum (L - p)(new_p - old_p)   (mod 65521),
// and those positions are the changed data chunks and the R parity rows: the bytes the update's lanes
// hold on both sides anyway.  The MG kernels (k_updmagic_*: the masked update's tile bodies under
// `if constexpr (MG)`) add each tile's dA, dB, reduced into [0, 65521), to magic_acc[2s], [2s + 1]
// (zeroed before the first launch), at the positions of the LOGICAL stripe: chunk j at j * size, row r
// at (K + r) * size.  launch_update_magic_finalize folds them into the magic words.  The struct
// derives from UpdateMaskArgs, whose layout -- and with it every non-MG kernel -- stays as it is.
struct UpdateMaskMagicArgs : UpdateMaskArgs {
  unsigned long long *magic_acc;  // 2 per stripe of this launch (8-byte aligned device memory)
};
static_assert(sizeof(UpdateMaskMagicArgs) == sizeof(UpdateMaskArgs) + 8, "UpdateMaskMagicArgs layout");
static_assert(sizeof(UpdateMaskMagicArgs) < 4096, "UpdateMaskMagicArgs: under the 4 KiB of kernel arguments");

// As launch_update_masked_*, and magic_acc != NULL.  The launch shapes are updmagic_bytewise_form and
// update_magic_lane_dwords.
hipError_t launch_update_magic_bytewise(const UpdateMaskMagicArgs &a, hipStream_t stream);
hipError_t launch_update_magic_bitsliced(const UpdateMaskMagicArgs &a, hipStream_t stream, int dw_pref = 0);
// One launch per call, behind the tile launches: for every stripe s < nstripes of the whole call whose
// effective mask stripe_cols[s] & allowed is not 0, the 4 little-endian bytes at magic + 4s (no
// alignment) are read, each 16-bit half h becomes (h + acc) mod 65521 -- or 0xFFFF where h >= 65521,
// which no adler32 half can be: invalid stays invalid -- and 4 bytes are written.  The word of a
// stripe whose effective mask is 0 is neither read nor written.
hipError_t launch_update_magic_finalize(const unsigned long long *acc, const unsigned long long *stripe_cols,
                                        unsigned long long allowed, int nstripes, uint8_t *magic, hipStream_t stream);

// Which kernel ran (test hooks lsec_test_launch_record / lsec_test_predict_forms, ec_plan.cpp).  The
// check, locate, patterned, rotated and update calls are families of separately compiled kernels; a form
// names one of them by its template arguments: bytewise R, KC (0: K at run time), IT, VW, BF; or
// bit-sliced R, DW (the patterned bit-sliced kernels have one dword per lane).  The per-R dispatch
// functions record the form at the one place where the template arguments are known; the record
// is the calling thread's, holds the launches since launch_record_reset() in order (the engine
// resets it on entry to each of those calls) and costs a few host stores per launch.
enum LaunchFamily { kFormChk = 1, kFormLoc, kFormChkRot, kFormLocRot, kFormPat, kFormPatRot, kFormUpd, kFormEncRot, kFormUpdRot, kFormUpdMask, kFormUpdMaskMagic, kFormPatMagic, kFormChkMagic, kFormChkMagicRot, kFormEncMagicRot, kFormPatSearch, kFormPatSearchRot, kFormPatMagicRot };
struct LaunchForm {
  int family, sliced, R, KC, IT, VW, BF, DW;
};
constexpr int kLaunchRecordMax = 16;  // forms kept (the count goes on)
void record_launch(const LaunchForm &f);
void launch_record_reset();
int launch_record(LaunchForm *out, int max);  // -> launches recorded; out[0 .. min(that, max, kLaunchRecordMax))
// The form launch_*(family) takes for K x R (R: the table's rmax for the patterned families), from
// the functions the dispatch itself calls; dw_pref: as launch_*_bitsliced takes it.  No GPU is
// touched.  false: no such kernel (R or K out of range, a locate of one row, a packet no lane fits).
bool predict_launch(int family, bool sliced, int K, int R, int packet, int dw_pref, LaunchForm *out);
// the same for the masked update (kFormUpdMask), which predict_launch does not answer for
bool predict_masked_launch(bool sliced, int K, int R, int packet, int dw_pref, LaunchForm *out);
// and for the masked update with the magic (kFormUpdMaskMagic)
bool predict_masked_magic_launch(bool sliced, int K, int R, int packet, int dw_pref, LaunchForm *out);
// and for the patterned decode with the magic (kFormPatMagic; R: the table's rmax, at least 1)
bool predict_pattern_magic_launch(bool sliced, int K, int R, int packet, LaunchForm *out);
// and for that decode over rotating shards with a stripe_pattern (kFormPatMagicRot)
bool predict_pattern_magic_rot_launch(bool sliced, int K, int R, int packet, LaunchForm *out);
// and for the search (kFormPatSearch, or kFormPatSearchRot with `rotated`; R: the table's rmax, at least 1)
bool predict_pattern_search_launch(bool rotated, bool sliced, int K, int R, int packet, LaunchForm *out);
// and for the check with the magic (kFormChkMagic, or kFormChkMagicRot with `rotated`)
bool predict_check_magic_launch(bool rotated, bool sliced, int K, int R, int packet, int dw_pref, LaunchForm *out);
// and for the rotated encode with the magic (kFormEncMagicRot)
bool predict_encode_magic_launch(bool sliced, int K, int R, int packet, int dw_pref, LaunchForm *out);
// the K with fixed-K forms (LSEC_FIXED_K), ascending -> how many there are; out[0 .. min(that, max))
int fixed_k_list(int *out, int max);

// The apply family: what lsec_encode_dev, lsec_decode_dev and lsec_encode_magic_dev launch (test hooks
// lsec_test_apply_record / lsec_test_predict_apply, ec_plan.cpp).  Its kernels take more template arguments
// than a LaunchForm names, so it has a record of its own, kept apart from the one above:
//   kind   1 k_gf8_bytewise, 2 k_gf8_bitsliced, 3 k_bitmatrix / k_bitmatrix_any, 4 k_gfw_wordwise /
//          k_gfw_transposed, 5 k_gfw_bitsliced (the KernelKind of ec_engine.h)
//   R, KC, IT, VW, BF   bytewise, as in a LaunchForm;  DW  kind 2's dwords per lane;  w  kinds 3-5
//   acc    the ACC instantiation (a later input group of a stripe of more than kMaxK inputs)
//   magic  the MG instantiation (lsec_encode_magic_dev's fused pass)
//   sub    kind 3: 1 the kernel of its word size, 0 k_bitmatrix_any;  kind 4: 1 k_gfw_transposed,
//          0 the mask-per-bit k_gfw_wordwise;  else 0
//   loop   bytewise kernels that hold two whole tile loops (bw_dual_loops): 1 the plain-XOR first row's
//          (X0), 0 the other's, as the flag of the launch's first cell selects; -1: the kernel has one loop
// The per-R dispatch functions record the form where the template arguments are spelled out; `loop` comes
// from apply_record_first_row, which the engine sets from its host matrix before each launch (nothing is
// read back from the device).
struct ApplyForm {
  int kind, R, KC, IT, VW, BF, DW, w, acc, magic, sub, loop;
};
constexpr int kApplyFormInts = 12;
constexpr int kApplyRecordMax = 64;  // forms kept (the count goes on); RS(200+17): 4 input groups x 3 row launches
constexpr int kApplyCountMax = 1 << 20;  // where the launch count stops (record_apply)
void record_apply(const ApplyForm &f);  // nothing on a thread that never called apply_record_reset()
void apply_record_reset();
void apply_record_first_row(bool all_ones);  // of the launches that follow, until set again
int apply_record(ApplyForm *out, int max);   // -> launches recorded; out[0 .. min(that, max, kApplyRecordMax))
// The form one launch_bytewise / launch_bytewise_magic / launch_bitsliced / launch_bitmatrix /
// launch_wordwise / launch_gfw_bitsliced call takes for K x R, from the functions those call; bw_variant
// and bs_variant as lsec_set_kernel_variant takes them, dw_pref as launch_bitsliced does, first_row_ones
// as apply_record_first_row.  No GPU is touched.  false: the launch would be refused.
bool predict_apply_launch(int kind, int K, int R, int w, int packet, bool acc, bool magic, int dw_pref, int bw_variant,
                          int bs_variant, bool first_row_ones, ApplyForm *out);

// Work-sharing tiles.  The streaming kernels deal each XCD a contiguous eighth of the tiles
// (xcd_remap), but the XCDs do not run at one rate: on the headline's memory shape the odd ones
// take ~15 % longer per tile, every launch, so the even ones idle for the last 6-8 % of it
// (tools/probes/xcd_balance.hip, profiles/r05_v2_xcd_balance.jsonl).  With a queue slot the grid
// is persistent (the kernel's resident workgroups) and each workgroup takes tiles from its own
// XCD's eighth through an atomic counter, then from the other eighths once its own is done, so
// the XCDs finish within microseconds of each other.  A slot is kTileQueueWords counters on
// lines of their own: one per eighth, then a done counter; the launch's last workgroup zeroes
// them, and slots rotate over a ring per device; a slot is taken again only after an event
// recorded behind its last launch has completed.  LSEC_TILES=static turns it off (A/B).
constexpr int kTileQueueLine = 32;  // unsigned words per counter (a 128-B line each)
constexpr int kTileQueueWords = 9 * kTileQueueLine;
constexpr int kTileQueueRing = 4096;
// a slot on the device of stream st for a launch of ntiles tiles; null: tile sharing off, the
// launch small (fewer than kTileQueueMinTiles), or no slot available (the static eighths serve)
constexpr uint64_t kTileQueueMinTiles = 16384;
unsigned *tile_queue_slot(hipStream_t st, uint64_t ntiles);
// XCD tile phase: every XCD's eighth of the tiles starts 1/8 of a stripe later than the previous
// XCD's (wrapping around inside the eighth), so the eight XCDs stream from different column offsets
// of their stripes at any moment.  On for launch_tiled's kernels (tile_phase_on), off for the
// compiled networks (tile_phase_net_on); LSEC_TILE_PHASE = bit 0 | bit 1 << 1 overrides (default 1)
bool tile_phase_on();
bool tile_phase_net_on();
void set_tile_phase(int mode);  // (lsec_test_set_tile_phase: A/B runs in one process)
// after the launch that took `slot` is queued on st: records the slot's event and frees it for a
// later taker (who waits for that event first: a slot is never shared by two unfinished launches)
void tile_queue_release(hipStream_t st, unsigned *slot);
// with tile sharing on, the tiles of each eighth (of ntiles) dealt statically, one per block,
// before the sharing blocks take the rest (LSEC_TILES=shared: none; the default keeps 7/8)
uint32_t tiles_prefix(uint32_t ntiles);
// measurement hook: the buffer launch_tiled hands its kernels for per-workgroup end times
unsigned long long *launch_stamps(uint32_t *n);
void set_launch_stamps(unsigned long long *p, uint32_t n);
// the persistent grid of `kernel` on st's device (its resident workgroups of kBlock threads,
// times the CUs), at most `grid`; 0 when the runtime cannot say
int persistent_grid(const void *kernel, int grid, hipStream_t st);

// Per-stripe adler32 "magic" of LStore's erasure segment (je_cksum_calc,
// src/lio/segment/jerasure.c:169-182): zlib adler32 (RFC 1950) over the concatenation of all
// k+m chunks of a stripe, stored as 4 little-endian bytes.  Computed with position-weighted
// partial sums: over bytes b_i at positions i of a stream of length L,
//   A = 1 + sum b_i,  B = L + sum (L - i) b_i   (mod 65521)
// so any tile of any shard contributes independently (S = sum b, U = sum (i - p0) b via
// v_dot4_u32_u8), blocks add their reduced partials into 2 x u64 per stripe (acc), and a
// finalize kernel folds them into the magic.
constexpr int kMaxMagicShards = kMaxK + kMaxR;

struct MagicArgs {
  int nshards;            // shards of this launch, in checksum order (LStore: data 0..k-1, parity 0..m-1)
  int shard0;             // checksum index of sh[0] (wide stripes: one launch per kMaxMagicShards shards)
  int total_shards;       // shards per stripe (0: nshards)
  int nstripes;
  int64_t size;           // bytes of each shard covered by this launch
  int64_t col0;           // column offset of those bytes inside the chunk (column-block staging)
  int64_t chunk;          // full chunk size C (checksum positions are i*C + col0 + o)
  unsigned long long *acc;  // 2 per stripe: sum A, sum B (zeroed before the first launch)
  ShardRef sh[kMaxMagicShards];
};

hipError_t launch_stripe_magic(const MagicArgs &a, hipStream_t stream);
// magic[s*4 .. s*4+3] from acc (total_len = shards * C)
hipError_t launch_magic_finalize(const unsigned long long *acc, int nstripes, int64_t total_len, uint8_t *magic,
                                 hipStream_t stream);

// Chunk comparison for the control-chunk check of jerase_control_check (segment/jerasure.c:
// 202-269): flags[s] = 1 when any byte of a[p] and b[p] (p < npairs) differs in stripe s
// (flags zeroed by the caller).
struct DiffArgs {
  int npairs;
  int nstripes;
  int64_t size;
  int *flags;
  ShardRef a[kMaxR];
  ShardRef b[kMaxR];
};
hipError_t launch_chunk_diff(const DiffArgs &a, hipStream_t stream);

// Device-side gather of scattered byte ranges into one contiguous buffer (so a scattered
// device -> host transfer becomes one DMA): dst + dst_off[i] <- src[i], bytes[i] (multiples of
// 8, 8-byte aligned).  `list` is in device memory; one block per piece.
struct GatherPiece {
  uint64_t src;
  uint64_t dst_off;
  uint64_t bytes;
};
hipError_t launch_gather(const GatherPiece *list, int n, char *dst, hipStream_t stream);

// Host-memory transport by kernel: piece i copies bytes[i] (a multiple of 16, <= kPieceBytes)
// from src to dst, both 16-byte aligned, one block per piece.  Either side may be the device
// alias of page-locked host memory, so one launch moves many small host runs over PCIe
// without a DMA command per run.  `list` must be device-readable (page-locked host is).
constexpr uint32_t kPieceBytes = 16384;
struct CopyPiece {
  uint64_t src;
  uint64_t dst;
  uint64_t bytes;
};
hipError_t launch_copy_pieces(const CopyPiece *list, int n, hipStream_t stream);

// Completion signal of a zero-copy call: every block writes back its XCD's L2 at system scope
// (a call's kernel may have left dirty lines of page-locked host memory in any XCD's L2), the
// last block to arrive (agent-scope counter in device memory, reset by it) stores `value` to
// `flag` (page-locked host memory) with system-scope release.  Launched on the call's stream
// right after its coding kernel, so stream order puts every byte the call wrote before the flag.
hipError_t launch_signal(unsigned *counter, unsigned *flag, unsigned value, hipStream_t stream);

// HBM probe (measurement only): dst <- src, bytes a multiple of 16, both 16-byte aligned.
hipError_t launch_hbm_copy(void *dst, const void *src, uint64_t bytes, hipStream_t stream);
// HBM probe (measurement only): out[r] = XOR of the K inputs for every stripe (a.K, a.R <= kMaxR,
// a.in / a.out / a.nstripes / a.size): the encode's K-read : R-write traffic without its arithmetic.
hipError_t launch_hbm_mix(const ApplyArgs &a, hipStream_t stream);
// HBM probe (measurement only): out = XOR of the K inputs for every stripe, in a kernel that shares
// no code with the coding kernels (the decode's K-read : 1-write shape); variant = IT | G << 4 |
// REMAP << 8: IT 16-byte steps per lane, G tiles per block, XCD-contiguous grabs (ec_kernels.hip).
hipError_t launch_probe_xor(const ShardRef *in, int K, ShardRef out, int nstripes, int64_t size, int variant,
                            hipStream_t stream);

// Host helper: fill one cell for coefficient c.
void make_cell(uint8_t c, CoefCell &cell);

// Launchers (return hipError_t of the launch).  grid_blocks <= 0 picks a default.
hipError_t launch_bytewise(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0);
// encode + stripe magic in one pass (a.magic_acc != nullptr; checksum order = inputs, outputs)
hipError_t launch_bytewise_magic(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0);
// dw_pref: dwords per lane (1, 2, 4; 0 = 1) unless an A/B variant is set (lsec_set_kernel_variant)
hipError_t launch_bitsliced(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0, int dw_pref = 0);
// generic GF(2) bitmatrix codes (liberation / blaum_roth / liber8tion, liberation.c; Cauchy at
// w = 16 / 32): w in LSEC_BITMATRIX_W by a kernel per w, any other 2 <= w <= kMaxW by the
// LDS-staged kernel; R <= 2 per launch
hipError_t launch_bitmatrix(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0);
bool bitmatrix_w_supported(int w);
// matrix codes over GF(2^16) / GF(2^32) (a.w), little-endian words, R <= 8: bit-sliced after
// an in-register transpose (R <= 4 at w = 32), per-bit masks beyond that
hipError_t launch_wordwise(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0);
// Cauchy codes at w = 16 / 32 in the packet layout, bit-sliced over GF(2^w): the wordwise
// image supplies the coefficients; R <= 8 per launch at w = 16, <= 4 at w = 32
hipError_t launch_gfw_bitsliced(const ApplyArgs &a, hipStream_t stream, int grid_blocks = 0);
// host helper: the w products c * x^b (b = 0..w-1) of a wordwise cell, replicated for w = 16
void make_word_cell(uint32_t c, int w, uint32_t *out);

// Variant selection knobs for experiments: 0 = default
void set_kernel_variant(int bytewise_variant, int bitsliced_variant);
void set_tile_mode(int mode);  // lsec_set_tile_sharing: 0 static, 1 shared, 2 static prefix + shared tail
int tile_mode();
int bytewise_variant();  // != 0: a forced bytewise shape (also keeps wide codes off their XOR networks)
int bitsliced_variant();  // != 0: a forced bit-sliced / wordwise variant (also keeps w = 16 / 32 RS off its XOR network)

}  // namespace lsec
