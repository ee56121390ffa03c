/*
 * lstore_ec.h -- C ABI of liblstore_ec.so, the MI355X (gfx950) erasure-coding engine that
 * drops in behind LStore's erasure plan service.
 *
 * Part 1 is the reference interface, declaration for declaration: the plan struct layout,
 * method ids and et_* entry points of src/lio/erasure_tools.h:28-75.  LStore's segment
 * driver dereferences the struct's fields and function pointers directly
 * (src/lio/segment/jerasure.c:1231-1232, :1847, :2242-2243, :245), so the layout below IS
 * the ABI and must not change.  A binary built against the reference header links against
 * this library unchanged (INTEGRATION.md shows the build-line change).
 *
 * Part 2 adds batched and device-resident entry points (prefix lsec_ / et_*_stripes) that
 * the reference does not have; they let a caller hand over many stripes per call, which is
 * what a GPU needs (SURVEY.md §8b "recommended extension").
 *
 * Errors: every call that can fail returns a status (0 = success, negative = failure) and
 * records a message for lsec_last_error().  The two void fn-pointers inherited from the
 * reference (encode_block) cannot return a status; on failure they print the reason to
 * stderr and abort() -- the engine never silently skips or falls back to a CPU path.
 */
#ifndef LSTORE_EC_H
#define LSTORE_EC_H

#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================== Part 1: reference ABI */

typedef struct lio_erasure_plan_t lio_erasure_plan_t;   /* src/lio/lio/erasure_tools.h:31 */

/* method ids -- src/lio/erasure_tools.h:37-45 */
#define REED_SOL_VAN    0
#define REED_SOL_R6_OP  1
#define CAUCHY_ORIG     2
#define CAUCHY_GOOD     3
#define BLAUM_ROTH      4
#define LIBERATION      5
#define LIBER8TION      6
#define RAID4           7
#define N_JE_METHODS    8

/* method names -- src/lio/erasure_tools.c:35 */
extern const char *JE_method[N_JE_METHODS];

/* src/lio/erasure_tools.h:50-65 (layout-identical) */
struct lio_erasure_plan_t {
    long long int strip_size;   /* size of each data strip */
    int method;                 /* encoding/decoding method */
    int data_strips;            /* k */
    int parity_strips;          /* m */
    int w;                      /* word size */
    int packet_size;            /* bitmatrix packet size */
    int base_unit;              /* register size in bytes */
    int *encode_matrix;         /* m x k coding matrix (matrix / Cauchy methods) */
    int *encode_bitmatrix;      /* (m*w) x (k*w) 0/1 bitmatrix (bitmatrix methods) */
    int **encode_schedule;      /* smart XOR schedule, -1 terminated (bitmatrix methods) */
    int (*form_encoding_matrix)(lio_erasure_plan_t *plan);
    int (*form_decoding_matrix)(lio_erasure_plan_t *plan);
    void (*encode_block)(lio_erasure_plan_t *plan, char **ptr, int block_size);
    int (*decode_block)(lio_erasure_plan_t *plan, char **ptr, int block_size, int *erasures);
};

/* replaces nearest_prime, erasure_tools.c:50-77 */
int nearest_prime(int w, int which);
/* replaces et_method_type, erasure_tools.c:716-725 (case-insensitive name -> id, -1 if unknown) */
int et_method_type(char *meth);
/* replaces et_new_plan, erasure_tools.c:606-685 */
lio_erasure_plan_t *et_new_plan(int method, long long int strip_size,
                                int data_strips, int parity_strips, int w, int packet_size, int base_unit);
/* replaces et_generate_plan, erasure_tools.c:733-908 (same w / packet-size search) */
lio_erasure_plan_t *et_generate_plan(long long int file_size, int method,
                                     int data_strips, int parity_strips, int w, int packet_low, int packet_high);
/* replaces et_destroy_plan, erasure_tools.c:691-710 */
void et_destroy_plan(lio_erasure_plan_t *plan);
/* replace the file tools et_encode / et_decode, erasure_tools.c:339-436 / :476-600 */
int et_encode(lio_erasure_plan_t *plan, const char *fname, long long int foffset, const char *pname,
              long long int poffset, int buffer_size);
int et_decode(lio_erasure_plan_t *plan, long long int fsize, const char *fname, long long int foffset,
              const char *pname, long long int poffset, int buffer_size, int *erasures);

/*
 * Semantics of the plan's fn-pointers (unchanged from the reference):
 *   encode_block(plan, ptr, C)   ptr[0..k) data chunks, ptr[k..k+m) parity chunks, C bytes each;
 *                                writes only ptr[k..k+m).   (segment/jerasure.c:1847)
 *   decode_block(plan, ptr, C, erasures)  erasures = -1 terminated ids; rebuilds only the
 *                                erased slots; 0 on success, -1 if unrecoverable.  (:245)
 * ptr may hold host pointers (staged over PCIe) or device pointers (used in place).
 * C must be a multiple of 8 (matrix methods) or of w*packet_size (bitmatrix methods).
 */

/* ===================================================================== Part 2: extensions */

#define LSEC_ABI_VERSION 3   /* 3: + lsec_decode_dev_patterns, lsec_decode_dev_rotated (additive) */
/* lsec_check_dev came later and is purely additive: the version stays 3, and a caller detects
 * it by the symbol (dlsym). */

/* Stripe-batched host-memory calls.  ptrs holds nstripes*(k+m) pointers laid out exactly
 * like segjerase_write_func's ptr[] array (segment/jerasure.c:1647, :1812-1836): stripe s
 * uses ptrs[s*(k+m) .. s*(k+m)+k+m).  One erasure pattern for all stripes. */
int et_encode_stripes(lio_erasure_plan_t *plan, char **ptrs, int nstripes, int block_size);
int et_decode_stripes(lio_erasure_plan_t *plan, char **ptrs, int nstripes, int block_size, int *erasures);

/* Device-resident calls.  Shard i (0..k+m-1) of stripe s lives at
 *   (char *)shards[i].base + s * shards[i].stride        (device memory)
 * e.g. LStore's layout: data base = page + i*C, stride = k*C; parity base = par + i*C,
 * stride = m*C.  Work is enqueued on `stream` (a hipStream_t; NULL = legacy default stream)
 * and the call returns without synchronising.
 *
 * Layout rule, the same for every lsec_*_dev entry point that takes a plan: each base and each
 * stride is a multiple of 8 bytes (as block_size is); nothing more is required -- shards need
 * be neither 16-byte aligned nor contiguous, and each shard may have a stride of its own.  The
 * shards of one call must not overlap (a call reads its inputs while it writes its outputs).
 * A base that is not a multiple of 8, or such a stride with nstripes > 1, returns -1 with a
 * message naming this rule, and nothing is enqueued.  nstripes == 0 with NULL bases stays
 * valid (the calls that prepare ahead). */
typedef struct {
    void *base;
    long long stride;
} lsec_shard_t;

int lsec_encode_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                    long long block_size, void *stream);
int lsec_decode_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                    long long block_size, const int *erasures, void *stream);

/* Stripes that do not share an erasure pattern, one launch.  `patterns` holds npatterns
 * erasure lists back to back, each -1 terminated as decode_block takes them; an empty list
 * (just -1) is valid: nothing to rebuild.  stripe_pattern (device memory, nstripes bytes)
 * gives each stripe's index into them.  Shards are logical chunks, as for lsec_decode_dev.
 *
 * - The bytes written are exactly what lsec_decode_dev writes for that stripe with that
 *   pattern.  Only the erased slots of each stripe are written; survivors are only read.  A
 *   stripe whose pattern is empty is neither read nor written.
 * - A RAID4 pattern that loses only the parity counts as empty (raid4.c:48, as lsec_decode_dev).
 * - A stripe_pattern value >= npatterns makes that stripe behave as the empty pattern; the
 *   kernel never indexes past its tables.
 * - Patterns of one call may have different erasure counts, from 0 to m.
 * - 1 <= npatterns <= 256.
 * - nstripes == 0 validates the arguments and builds, uploads and caches the call's device
 *   tables (stripe_pattern may then be NULL), so a caller can prepare ahead; the tables are
 *   cached on the plan per device, keyed by the pattern lists in their order, until the plan is
 *   destroyed, and a repeated call does no matrix work and no upload.
 * - Plans: lsec_plan_kernel 1 (bytewise GF(2^8): RS, r6, raid4) and 2 (bit-sliced GF(2^8):
 *   Cauchy at w = 8).  Further limits: k <= 64, k + m <= 128, at most 8 erasures per pattern.
 * - Anything outside these limits -- plan kernels 3-5, wider stripes, an id out of range, more
 *   than m erasures, a NULL pointer -- returns -1 with a message for lsec_last_error that names
 *   the limit.  There is no fallback and no partial work.
 * - Alignment and block_size rules are those of lsec_decode_dev (lsec_shard_t, above).
 * Enqueued on `stream`; returns without synchronising.  0 / -1. */
int lsec_decode_dev_patterns(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                             long long block_size, const int *patterns, int npatterns,
                             const unsigned char *stripe_pattern, void *stream);

/* Degraded read of a rotated LUN.  devs[i] (i < k+m) is PHYSICAL device i: it holds, for
 * stripe s, logical chunk (i + (first_stripe + s) * n_shift) mod (k+m)  (lun.c:1178-1223).
 * `lost` lists unreadable physical devices (-1 terminated, at most m); their entries in devs
 * point at the memory that receives the rebuilt chunks.  Each stripe is decoded with the
 * pattern its rotation gives (the lost devices' logical chunks), under the semantics and limits
 * of lsec_decode_dev_patterns; n_shift < 0 and first_stripe < 0 return -1.  The tables are
 * cached by (lost, n_shift mod (k+m)) and do not depend on first_stripe; nstripes == 0
 * prepares them.  Enqueued on `stream`; returns without synchronising.  0 / -1. */
int lsec_decode_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                            long long block_size, const int *lost, int n_shift,
                            long long first_stripe, void *stream);

/* The patterned decode that also leaves every stripe's magic, one pass: lsec_decode_dev_patterns /
 * lsec_decode_dev_rotated, and magic[s] -- the adler32 over all k+m chunks of stripe s (the stripe
 * "magic", below) -- as lsec_stripe_magic_dev would write it behind the decode.  A degraded or
 * paranoid read is "rebuild the bad chunks, then the checksum over all k+m chunks must equal the
 * quorum magic" (jerase_control_check, segment/jerasure.c:244-249; je_cksum_compare, :188-194);
 * as two calls that is k reads + e writes and then k+m reads per stripe with e erasures.  Here the k
 * survivors the decode loads and the e chunks it forms are summed from registers, and only the
 * m - e survivors it does not use are loaded for the checksum alone: k+m-e reads and e writes.
 * Purely additive too: the version stays 3, a caller detects the calls by their symbols.
 *
 * - Bytes left in the shards: exactly those lsec_decode_dev_patterns / lsec_decode_dev_rotated
 *   leave for the same arguments.  Only erased slots are written; survivors are only read; a
 *   RAID4 pattern that loses only the parity writes nothing.
 * - `magic` is device memory, 4*nstripes bytes, no alignment requirement, pure output.  Word s is
 *   the 4 little-endian bytes of zlib's adler32 over the k+m chunks of stripe s in LOGICAL order
 *   (for the rotated call: after un-rotating), as they lie in memory after the decode.  A stripe
 *   whose stored bytes are inconsistent, or whose RAID4 parity is stale, gets the adler32 of
 *   exactly those bytes: the call judges nothing but `expect`.
 * - A stripe whose pattern is empty (just -1, or RAID4 parity-only) is checksummed without being
 *   written, k+m reads: the paranoid read's "verify every stripe".
 * - Patterned call: a stripe_pattern value >= npatterns skips the stripe entirely.  None of its
 *   chunks is read or written, its magic word is neither read nor written, and bad[s] is 0: the
 *   non-paranoid read, which verifies only stripes with bad chunks.  In the rotated call every
 *   stripe has a pattern (its rotation), so none is skipped.
 * - `expect`, `bad` and `bad_count` are optional (NULL).  expect: device memory, 4*nstripes bytes,
 *   no alignment requirement, only read: the quorum magics.  With it, bad (nstripes bytes, no
 *   alignment) receives 1 where magic[s] != expect[s] for a stripe that was not skipped, else 0,
 *   and bad_count (one 32-bit word, 4-byte aligned) the number of those.  The call sets both; it
 *   does not add to them.  Without expect a non-NULL bad or bad_count is refused.
 * - Scratch: the per-stripe accumulators, 16 bytes per stripe, come from the stream-ordered
 *   allocator (hipMallocAsync on `stream`), are zeroed there and go back to it on the stream,
 *   exactly as lsec_encode_magic_dev's do.
 * - Tables: the plain calls' own, cached on the plan per device under the same keys, together with
 *   what the magic form adds to a pattern's record (the survivors its decode does not read).  A
 *   repeated call does no matrix work and no upload.  nstripes == 0 validates the arguments and
 *   prepares the tables, as for the plain calls; magic and the other outputs may then be NULL.
 * - Plans: lsec_plan_kernel 1 and 2.  Limits: k <= 64, 1 <= m <= 8 (so a pattern has at most 8
 *   unused survivors), at most 8 erasures per pattern, 1 <= npatterns <= 256.  Layout, alignment
 *   and block_size rules are those of lsec_decode_dev.  magic, expect, bad and bad_count must not
 *   overlap one another or the shards.
 * - Every refusal -- plan kernels 3-5, k or m out of range, then anything the plain call refuses,
 *   in its order, then a NULL magic with nstripes > 0, bad or bad_count without expect, a
 *   misaligned bad_count -- returns -1 with a message for lsec_last_error that names this call and
 *   the limit, and nothing is enqueued: every argument check comes before the first HIP call.
 *   There is no fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
int lsec_decode_magic_dev_patterns(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                                   long long block_size, const int *patterns, int npatterns,
                                   const unsigned char *stripe_pattern, void *magic,
                                   const void *expect, unsigned char *bad, unsigned int *bad_count,
                                   void *stream);
int lsec_decode_magic_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                  long long block_size, const int *lost, int n_shift, long long first_stripe,
                                  void *magic, const void *expect, unsigned char *bad,
                                  unsigned int *bad_count, void *stream);

/* The patterned decodes over the physical devices of a rotated LUN: lsec_decode_dev_patterns and
 * lsec_decode_magic_dev_patterns for a caller who holds device images, not logical shards -- the layout
 * lsec_segment_write produces.  They are the middle step of the device-resident read of a rotated LUN:
 * the `ids` of lsec_vote_dev_rotated (or the `found` of lsec_search_dev_patterns_rotated, the `located`
 * of lsec_locate_dev_rotated) are their stripe_pattern, and the `bad` of the magic call is the `select`
 * of lsec_search_dev_patterns_rotated.  Purely additive too: the version stays 3, a caller detects the
 * calls by their symbols.
 *
 * Devices and patterns
 * - devs, n_shift and first_stripe mean exactly what they mean for lsec_check_dev_rotated: devs[i]
 *   (i < k+m) is PHYSICAL device i, rot_s = ((first_stripe + s) * n_shift) mod (k+m).  n_shift >= k+m is
 *   taken mod k+m; n_shift < 0 and first_stripe < 0 are refused; first_stripe may be anything up to
 *   2^63 - 1.
 * - `patterns`, npatterns and stripe_pattern are those of lsec_decode_dev_patterns: erasure lists of
 *   LOGICAL chunk ids back to back, each ended by -1, and one byte per stripe in device memory.
 * - Logical chunk c of stripe s is read from devs[(c - rot_s) mod (k+m)] and, if it is erased, rebuilt
 *   there.  The entry of an unreadable device points at memory that receives the rebuilt chunks, as for
 *   lsec_decode_dev_rotated.  All k+m entries of devs are validated.
 * Plain call
 * - The bytes left on the devices are exactly those lsec_decode_dev_patterns leaves for the logical view
 *   of each stripe with that stripe's pattern.  Only erased slots are written.  A stripe with an empty
 *   pattern, a RAID4 parity-only pattern or an id >= npatterns is neither read nor written.
 * - n_shift == 0 behaves exactly as lsec_decode_dev_patterns over devs.
 * - Limits: those of lsec_decode_dev_patterns -- plan kernels 1 and 2, k <= 64, k + m <= 128, at most 8
 *   erasures per pattern, 1 <= npatterns <= 256.
 * Magic call
 * - Everything lsec_decode_magic_dev_patterns specifies holds for the logical view: magic[s] is zlib's
 *   adler32 over the k+m chunks in LOGICAL order as they lie after the decode (the rotation never enters
 *   a position weight); an empty pattern checksums without writing, k+m reads; for an id >= npatterns no
 *   chunk is read or written, the magic word is neither read nor written and bad[s] = 0.
 * - expect, bad and bad_count behave as in lsec_decode_magic_dev_patterns.
 * - Scratch: 16 bytes per stripe from the stream-ordered allocator (hipMallocAsync on `stream`), zeroed
 *   there and freed there, also when a launch fails.
 * - Limits: those of lsec_decode_magic_dev_patterns -- k <= 64, 1 <= m <= 8.  n_shift == 0 behaves
 *   exactly as lsec_decode_magic_dev_patterns.
 * Tables
 * - Both calls use the cache entry lsec_decode_dev_patterns uses for the same list (the magic call adds
 *   the unused-survivor records), so vote, decode, search and repair over one list share one upload and
 *   a repeated call does no matrix work and no upload.  nstripes == 0 validates the arguments and
 *   prepares the tables as lsec_decode_dev_patterns does; all device pointers may then be NULL.
 * Refusals
 * - The ladder of lsec_decode_dev_patterns / lsec_decode_magic_dev_patterns in their order, with a
 *   negative n_shift and then a negative first_stripe directly behind a negative nstripes.  Each returns
 *   -1 with a message for lsec_last_error that names the call that was made, and nothing is enqueued:
 *   every argument check comes before the first HIP call.  There is no fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
int lsec_decode_dev_patterns_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                     long long block_size, int n_shift, long long first_stripe,
                                     const int *patterns, int npatterns,
                                     const unsigned char *stripe_pattern, void *stream);
int lsec_decode_magic_dev_patterns_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                           long long block_size, int n_shift, long long first_stripe,
                                           const int *patterns, int npatterns,
                                           const unsigned char *stripe_pattern, void *magic,
                                           const void *expect, unsigned char *bad,
                                           unsigned int *bad_count, void *stream);

/* The search for the erasure set that fits the magic, one pass: what LStore does when a stripe's magic
 * does not match and the first guess fails (jerase_brute_recovery / jerase_brute_recurse,
 * segment/jerasure.c:271-339).  That routine tries erasure combinations in order and stops at the
 * first whose rebuilt stripe sums to the quorum magic; it is the reference's only answer to silent
 * corruption, and it covers what lsec_locate_dev cannot: m = 1 plans (RAID4 among them), more than one
 * corrupt chunk, and m = 2 stripes where two corrupt chunks imitate a third.  Built from
 * lsec_decode_magic_dev_patterns, which writes in place, it is a copy of the stripes aside and one
 * launch and one restore per candidate.  Here every candidate is tried on every selected stripe in one
 * pass that writes no chunk.  Purely additive too: the version stays 3, a caller detects the calls by
 * their symbols.
 *
 * Candidates
 * - `patterns` / npatterns: the candidate list, in the format lsec_decode_dev_patterns takes -- erasure
 *   lists of LOGICAL chunk ids back to back, each ended by -1; an empty list is valid.  The order is
 *   the caller's.  The reference's order is the empty pattern (or its last successful guess) first,
 *   then sizes ascending, each size in lexicographic order.
 * - 1 <= npatterns <= 254 (both sentinels below stay past the table), at most min(m, 8) erasures per
 *   pattern, nstripes * npatterns < 2^31.
 * Trial magic
 * - T(s, p) is the word lsec_decode_magic_dev_patterns would write for stripe s if that stripe's
 *   pattern were p: zlib's adler32 over the k+m chunks in logical order with the erased chunks
 *   replaced by what the pattern's survivors rebuild.  A RAID4 pattern that loses only the parity
 *   rebuilds nothing, and T is the sum of the stored bytes.
 * Outputs
 * - `expect`: required with nstripes > 0; device memory, 4*nstripes bytes, no alignment requirement,
 *   only read: the quorum magics.
 * - `found`: required with nstripes > 0; nstripes bytes, no alignment requirement.  found[s] is the
 *   lowest p with T(s, p) == expect[s], LSEC_LOCATE_MANY if no candidate matches, and
 *   LSEC_LOCATE_CLEAN for a stripe that was not selected.  The call sets every byte itself.  found is
 *   directly usable as stripe_pattern of lsec_decode_dev_patterns or lsec_decode_magic_dev_patterns
 *   with the same list: both sentinels are >= npatterns.
 * - `select`: optional (NULL selects every stripe); nstripes bytes of device memory, only read.  A
 *   stripe with select[s] == 0 is not searched and none of its chunks is read.  The `bad` output of
 *   lsec_decode_magic_dev_patterns or lsec_check_magic_dev is a valid select.
 * - `trial`: optional; 4*nstripes*npatterns bytes, no alignment requirement, pure output.  Word
 *   s*npatterns + p receives T(s, p), little-endian.  Words of stripes not selected are neither read
 *   nor written.
 * - `counts`: optional; two 32-bit words, 4-byte aligned: stripes found, stripes marked
 *   LSEC_LOCATE_MANY.  The call sets them; it does not add to them.
 * Without LSEC_SEARCH_REPAIR the shards are only read: no byte of any chunk is written.
 * With LSEC_SEARCH_REPAIR, behind the search on the same stream, every found stripe is rebuilt in
 *   place: the bytes are those lsec_decode_dev_patterns writes for that stripe with pattern found[s].
 *   Stripes not found and stripes not selected are neither read again nor written.  Unknown flag bits
 *   are refused.
 * What the call can and cannot tell
 * - A stripe whose stored bytes already sum to expect[s] matches every candidate made of chunks that
 *   are intact, so found[s] is the first such entry of the list: a caller that wants "nothing to do"
 *   reported puts the empty pattern first.
 * - A candidate that is a superset of the corrupt set also matches; the order decides.
 * - adler32 is a weak sum: a false match is possible, exactly as in the reference.
 * Rotated call
 * - devs, n_shift and first_stripe mean what they mean for lsec_check_dev_rotated.  Patterns, found
 *   and trial are logical: logical chunk c of stripe s is read from devs[(c - rot_s) mod (k+m)] and,
 *   with the flag, rebuilt there.  n_shift == 0 behaves exactly as the unrotated call; n_shift < 0
 *   and first_stripe < 0 are refused.  found is the stripe_pattern of lsec_decode_dev_patterns_rotated
 *   and lsec_decode_magic_dev_patterns_rotated over the same devices and list.
 * Plans and limits
 * - lsec_plan_kernel 1 and 2, k <= 64, 1 <= m <= 8.  Layout, alignment and block_size rules are those
 *   of lsec_decode_dev.  The outputs must not overlap one another or the shards.
 * - Scratch: 16 bytes per (stripe, candidate) of accumulators from the stream-ordered allocator
 *   (hipMallocAsync on `stream`), zeroed there and freed there, also when a launch fails.
 * - Tables: the cache entry lsec_decode_dev_patterns uses for the same list, so the search, the repair
 *   and a later decode with found share one upload and a repeated call does no matrix work.
 *   nstripes == 0 validates the arguments and prepares the tables, as lsec_decode_dev_patterns does;
 *   all device pointers may then be NULL.
 * Refusals
 * - In this order: plan kernels 3-5; k or m out of range; whatever lsec_decode_dev_patterns refuses,
 *   in its order; npatterns > 254; nstripes * npatterns too large; a NULL expect or found with
 *   nstripes > 0; a misaligned counts; unknown flags.  Each returns -1 with a message for
 *   lsec_last_error that names this call and the limit, and nothing is enqueued: every argument check
 *   comes before the first HIP call.  There is no fallback to a launch per candidate.
 * Enqueued on `stream`; return without synchronising.  0 / -1.  (LSEC_LOCATE_CLEAN and
 * LSEC_LOCATE_MANY: with lsec_locate_dev, below.) */
#define LSEC_SEARCH_REPAIR 1   /* flags: rebuild every found stripe in place, behind the search */

int lsec_search_dev_patterns(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                             long long block_size, const int *patterns, int npatterns,
                             const unsigned char *select, const void *expect,
                             unsigned char *found, void *trial, unsigned int *counts,
                             int flags, void *stream);

int lsec_search_dev_patterns_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                     long long block_size, int n_shift, long long first_stripe,
                                     const int *patterns, int npatterns,
                                     const unsigned char *select, const void *expect,
                                     unsigned char *found, void *trial, unsigned int *counts,
                                     int flags, void *stream);

/* The read path's quorum vote, on the device: the first thing LStore does per stripe when it reads or scrubs
 * (segjerase_read_func, segment/jerasure.c:1383-1462) -- the majority vote over the k+m stored 4-byte magics and
 * the classification built on it -- for a caller whose images and magics already sit in device memory.  Its
 * `quorum` is directly the `expect`, and its `ids` the `stripe_pattern`, of lsec_decode_magic_dev_patterns,
 * lsec_check_magic_dev and lsec_search_dev_patterns, so a read or a scrub is one chain of calls on one stream
 * with no host step.  Purely additive too: the version stays 3, a caller detects the calls by their symbols.
 *
 * Inputs
 * - `stored`: k+m entries, required.  The stored magic of entry i for stripe s is the 4 bytes at
 *   base + s*stride: device memory, only read, no alignment requirement on base or stride (LStore's
 *   [magic | chunk] records: {image_i, C+4}).  base == NULL: that device is unreadable for the whole call.
 *   Plain call: entry i is logical chunk i.  Rotated call: entry i is physical device i, and logical chunk c of
 *   stripe s is entry (c - rot_s) mod (k+m), rot_s exactly as for lsec_check_dev_rotated; n_shift == 0 behaves
 *   as the plain call, n_shift < 0 and first_stripe < 0 are refused.
 * - `shards` / `devs`: optional (NULL).  The chunks, under the layout rule of lsec_check_dev /
 *   lsec_check_dev_rotated.  Only the blank scan reads them.  With NULL there is no scan: LSEC_VOTE_BLANK is
 *   never reported (such stripes are LSEC_VOTE_OK) and block_size is not looked at.  An entry whose `stored`
 *   base is NULL is not validated and never read.
 * - `patterns` / npatterns: optional (NULL / 0; with NULL patterns, ids must be NULL too).  The list format of
 *   lsec_decode_dev_patterns: erasure lists of LOGICAL chunk ids, each ended by -1.  1 <= npatterns <= 254 (as
 *   for the search: both sentinels stay past the table), at most min(m, 8) erasures per pattern.
 * Per stripe (all ids logical)
 * - The quorum is the largest group of readable chunks whose 4 stored bytes are equal; between groups of equal
 *   size the one whose first member has the lowest id wins (the reference's "first group with the largest
 *   count").  An unreadable chunk is in no group.
 * - `quorum`: required with nstripes > 0; 4*nstripes bytes, no alignment requirement.  The quorum's 4 bytes as
 *   stored; 0 when no chunk is readable.
 * - `outside`: optional; nstripes 64-bit words, 8-byte aligned.  Bit c is set when logical chunk c is outside
 *   the quorum (unreadable, or another magic).  Bits k+m and above are 0.
 * - `cls`: required with nstripes > 0; nstripes bytes.
 *     LSEC_VOTE_LOST      no chunk is readable, or the quorum has fewer than k members;
 *     LSEC_VOTE_BLANK     chunks were given, all k+m are in the quorum, its bytes are all 0 and every byte of
 *                         all k+m chunks is 0 (never written);
 *     LSEC_VOTE_OK        all k data chunks are in the quorum and the stripe is not BLANK;
 *     LSEC_VOTE_DEGRADED  otherwise.
 *   This is step 1 of lsec_segment_read, with one difference: an unreadable chunk never shadows a readable
 *   group of the same size (it matters only for k = 1).
 * - `ids`: optional; nstripes bytes, usable as stripe_pattern of the patterned calls with the same list
 *   (the rotated vote's: of lsec_decode_dev_patterns_rotated and lsec_decode_magic_dev_patterns_rotated).
 *     DEGRADED: the lowest p whose erasure set equals the outside set, LSEC_LOCATE_MANY if the list has none;
 *     OK with LSEC_VOTE_PARANOID: the same lookup (the outside set is then empty or parity-only: the paranoid
 *       read verifies the stripe and rebuilds the parity outside the quorum);
 *     OK without the flag, and BLANK: LSEC_LOCATE_CLEAN (the patterned calls skip the stripe);
 *     LOST: LSEC_LOCATE_MANY.
 * - `counts`: optional; five 32-bit words, 4-byte aligned: the stripes of class OK, DEGRADED, BLANK and LOST,
 *   then the stripes whose lookup found no pattern.  The call sets them; it does not add to them.
 * The call sets every output element itself.  Outputs must not overlap one another, `stored` or the chunks.
 * Cost
 * - The vote reads (k+m)*4 bytes per stripe.  The blank scan reads the k+m chunks of a stripe only when all its
 *   magics are zero and agree (a blank candidate), and stops launching loads for a stripe once a nonzero byte
 *   was seen; a stripe that is no candidate costs no chunk read.
 * - Scratch: 16 bytes per stripe from the stream-ordered allocator (hipMallocAsync on `stream`), zeroed there and
 *   freed there, also when a launch fails.
 * - Tables: the list's masks live in the cache entry lsec_decode_dev_patterns uses for the same list, so vote,
 *   decode, search and repair share one table and a repeated call does no matrix work and no upload.
 *   nstripes == 0 validates the arguments and, with patterns, prepares the tables as lsec_decode_dev_patterns
 *   does; all device pointers may then be NULL.
 * Plans and limits
 * - lsec_plan_kernel 1 and 2, 1 <= m <= 8, k + m <= 64 (the mask is one word, a stripe is one wavefront).
 * Refusals
 * - In this order: plan kernels 3-5; k, m or k+m out of range; a NULL stored; a negative nstripes; (rotated) a
 *   negative n_shift or first_stripe; whatever lsec_decode_dev_patterns refuses about the list, in its order;
 *   npatterns > 254; ids without patterns; with chunks, the layout and block_size refusals of lsec_check_dev;
 *   a NULL quorum or cls with nstripes > 0; a misaligned outside or counts; unknown flag bits.  Each returns -1
 *   with a message for lsec_last_error that names this call and the limit, and nothing is enqueued: every
 *   argument check comes before the first HIP call.  There is no host fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
#define LSEC_VOTE_OK        0  /* every data chunk is in the quorum (parity chunks may be outside it) */
#define LSEC_VOTE_DEGRADED  1  /* a data chunk is outside the quorum, and the quorum has >= k chunks */
#define LSEC_VOTE_BLANK     2  /* never written: all k+m magics zero and every byte of every chunk zero */
#define LSEC_VOTE_LOST      3  /* quorum smaller than k, or no device readable */
#define LSEC_VOTE_PARANOID  1  /* flags: OK stripes get a pattern id too (verify every stripe) */

int lsec_vote_dev(lio_erasure_plan_t *plan, const lsec_shard_t *stored, const lsec_shard_t *shards,
                  int nstripes, long long block_size, const int *patterns, int npatterns,
                  void *quorum, unsigned char *cls, unsigned char *ids,
                  unsigned long long *outside, unsigned int *counts, int flags, void *stream);
int lsec_vote_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *stored, const lsec_shard_t *devs,
                          int nstripes, long long block_size, int n_shift, long long first_stripe,
                          const int *patterns, int npatterns,
                          void *quorum, unsigned char *cls, unsigned char *ids,
                          unsigned long long *outside, unsigned int *counts, int flags, void *stream);

/* Parity check of device-resident stripes, one pass: are these stripes consistent, and if not,
 * which parity rows disagree?  `shards` are the k+m logical chunks as for lsec_encode_dev; all
 * of them are only read.  `syndrome` is device memory holding nstripes 32-bit words.
 *
 * - After the call, bit r (r < m) of syndrome[s] is set exactly when parity chunk r, as
 *   lsec_encode_dev would write it for the stored data chunks of stripe s, differs in at least
 *   one byte from the stored parity chunk r.  Bits m..31 are 0.
 * - The call sets every word itself (a hipMemsetAsync on `stream` ahead of the kernel): the
 *   caller does not pre-zero.
 * - bad_count is optional (may be NULL): one 32-bit word of device memory that receives the
 *   number of stripes with a nonzero syndrome.  The call sets it; it does not add to it.
 * - Nothing else is written, and nothing proportional to the data is allocated: the pass reads
 *   k + m chunks per stripe and writes only for inconsistent stripes.
 * - syndrome and bad_count must be 4-byte aligned and must not overlap the shards.
 * - Layout, alignment and block_size rules are those of lsec_encode_dev (lsec_shard_t, above;
 *   for Cauchy a multiple of 8 * packet_size).
 * - nstripes == 0 validates the arguments, returns 0 and touches no GPU (syndrome may then be
 *   NULL), so a caller can check a call shape ahead.
 * - Plans: lsec_plan_kernel 1 (bytewise GF(2^8): RS, r6, raid4) and 2 (bit-sliced GF(2^8):
 *   Cauchy at w = 8).  Further limits: k <= 64, m <= 8.
 * - Anything outside these limits -- plan kernels 3-5, wider stripes, a NULL shards, a NULL
 *   syndrome with nstripes > 0, a misaligned pointer -- returns -1 with a message for
 *   lsec_last_error that names the limit, and nothing is enqueued.  There is no fallback to
 *   encode-and-compare.
 * Enqueued on `stream`; returns without synchronising.  0 / -1. */
int lsec_check_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                   long long block_size, unsigned int *syndrome, unsigned int *bad_count,
                   void *stream);

/* Locating -- and with LSEC_LOCATE_REPAIR rebuilding -- the one corrupt chunk of device-resident
 * stripes, in the pass lsec_check_dev makes.  Purely additive too: the version stays 3, a caller
 * detects the call by its symbol.
 *
 * With S_r the difference between parity row r re-formed from the stored data and the stored
 * parity chunk r, one wrong data chunk j gives S_r = (g[r][j] / g[0][j]) * S_0 at every byte
 * column (g: the coding matrix), and one wrong parity chunk r gives S_r alone.  All four outputs
 * are device memory; the call sets every element itself (memsets on `stream` ahead of the
 * kernels), nothing is allocated per call and no scratch is shared between streams.
 *
 * - syndrome[s] (nstripes 32-bit words): exactly the word lsec_check_dev produces for stripe s.
 * - hyp[s] (nstripes 64-bit words): bit j (j < k) is set exactly when data chunk j is a
 *   single-chunk explanation of stripe s, that is, when replacing chunk j by what the other
 *   chunks rebuild makes the stripe consistent.  Bits k..63 are 0.  A consistent stripe has all k
 *   bits set (every hypothesis holds trivially); a stripe whose only fault is in parity has 0.
 * - located[s] (nstripes bytes):
 *     LSEC_LOCATE_CLEAN  when syndrome[s] == 0;
 *     k + r              when exactly bit r of syndrome[s] is set (parity chunk r);
 *     j                  when all m syndrome bits are set and hyp[s] has exactly the one bit j;
 *     LSEC_LOCATE_MANY   otherwise: inconsistent, and no single chunk explains it.
 *   located is directly usable as the stripe_pattern argument of lsec_decode_dev_patterns with
 *   the k+m single-erasure lists in chunk order ({0,-1}, {1,-1}, ..., {k+m-1,-1}): both sentinels
 *   are >= npatterns and so act as the empty pattern.
 * - counts is optional (may be NULL): two 32-bit words, the stripes located (a chunk id in
 *   located) and the stripes marked LSEC_LOCATE_MANY.
 * - flags & LSEC_LOCATE_REPAIR: behind the locate, on the same stream, every located chunk is
 *   rebuilt in place, with the bytes lsec_decode_dev writes for that stripe with that one erasure
 *   (it is that patterned decode, with located as stripe_pattern).  Clean and LSEC_LOCATE_MANY
 *   stripes are neither read again nor written.  Without the flag the shards are only read.
 * - What a code can tell apart: with m >= 3, corruption confined to two chunks is always
 *   reported LSEC_LOCATE_MANY.  With m = 2, two corrupt chunks can imitate a third one (two
 *   syndromes cannot tell two unknown chunks from one); this is a property of the code, not of
 *   the engine.  Corruption in more chunks than that can imitate a single chunk under any code.
 * - Plans: lsec_plan_kernel 1 and 2, k <= 64, 2 <= m <= 8 (one parity row cannot locate, so RAID4
 *   and every m = 1 plan is refused), and no zero coefficient in the coding matrix (none of the
 *   RS, r6 and Cauchy matrices has one).  LSEC_LOCATE_REPAIR adds the limits of
 *   lsec_decode_dev_patterns.
 * - syndrome and counts must be 4-byte aligned, hyp 8-byte aligned; located has no alignment
 *   requirement.  None of the outputs may overlap the shards.
 * - Layout, alignment and block_size rules are those of lsec_check_dev.
 * - nstripes == 0 validates the arguments, returns 0 and touches no GPU (the outputs may then be
 *   NULL); with LSEC_LOCATE_REPAIR it also prepares the pattern tables, as
 *   lsec_decode_dev_patterns with nstripes == 0 does.
 * - Every refusal returns -1 with a message for lsec_last_error that names the limit, and nothing
 *   is enqueued.  There is no fallback.
 * Enqueued on `stream`; returns without synchronising.  0 / -1. */
#define LSEC_LOCATE_CLEAN  0xFF   /* stripe is consistent */
#define LSEC_LOCATE_MANY   0xFE   /* inconsistent, and no single chunk explains it */
#define LSEC_LOCATE_REPAIR 1      /* flags: rebuild each located chunk in place */

int lsec_locate_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                    long long block_size, unsigned int *syndrome, unsigned long long *hyp,
                    unsigned char *located, unsigned int *counts, int flags, void *stream);

/* Check, locate and repair over the PHYSICAL devices of a rotated LUN, one pass: the scrub of a
 * LUN whose stripes do not share a chunk-to-device map, and the answer to its question, which
 * disk is going bad.  Purely additive too: the version stays 3, a caller detects the calls by
 * their symbols.
 *
 * - devs[i] (i < k+m) is physical device i, exactly as for lsec_decode_dev_rotated.  With
 *   rot_s = ((first_stripe + s) * n_shift) mod (k+m), logical chunk c of stripe s is read from
 *   devs[(c - rot_s) mod (k+m)].  n_shift >= k+m is taken mod k+m; n_shift < 0 and
 *   first_stripe < 0 return -1; first_stripe may be anything up to 2^63 - 1.
 * - syndrome, bad_count, hyp, located and counts are exactly what lsec_check_dev /
 *   lsec_locate_dev produce for the logical view of each stripe: bits and ids are logical (parity
 *   row r, data chunk j, k + r), the sentinels are the same, and n_shift == 0 behaves exactly as
 *   the unrotated calls.
 * - located_dev is optional (may be NULL): nstripes bytes, no alignment requirement.
 *   located_dev[s] is the physical device holding the located chunk, (located[s] - rot_s) mod
 *   (k+m); LSEC_LOCATE_CLEAN and LSEC_LOCATE_MANY pass through unchanged.
 * - dev_faults is optional (may be NULL): k+m 32-bit words, 4-byte aligned.  dev_faults[i] is the
 *   number of stripes of this call whose located chunk lives on device i; clean and
 *   LSEC_LOCATE_MANY stripes count nowhere.
 * - The calls set every output themselves (memsets on `stream` ahead of the kernels) and do not
 *   add to what was there.  Nothing is allocated per call and no scratch is shared between streams.
 * - flags & LSEC_LOCATE_REPAIR: behind the locate, on the same stream, every located chunk is
 *   rebuilt in place, with the bytes lsec_decode_dev_rotated writes for that stripe with
 *   lost = {located_dev[s]}.  Clean and LSEC_LOCATE_MANY stripes are neither read again nor
 *   written.  Without the flag the devices are only read.
 * - Plans and limits are those of lsec_check_dev / lsec_locate_dev: lsec_plan_kernel 1 and 2,
 *   k <= 64, m 1..8 for the check and 2..8 for the locate, no zero coefficient in the coding
 *   matrix.  LSEC_LOCATE_REPAIR adds no further limit: the repair works each stripe's rotation
 *   out in the kernel over one k+m single-erasure table, so RS(16+4) at n_shift = 1 repairs.
 * - Layout, alignment and block_size rules are those of lsec_check_dev; syndrome, counts and
 *   dev_faults must be 4-byte aligned, hyp 8-byte aligned.  None of the outputs may overlap the
 *   devices.
 * - nstripes == 0 validates the arguments, returns 0 and touches no GPU (the outputs may then be
 *   NULL); with LSEC_LOCATE_REPAIR it also prepares the single-erasure tables, as lsec_locate_dev
 *   does (on a host without a GPU the tables are built and dropped: there is nowhere to upload).
 * - Every refusal returns -1 with a message for lsec_last_error that names the limit, and nothing
 *   is enqueued.  There is no fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
int lsec_check_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                           long long block_size, int n_shift, long long first_stripe,
                           unsigned int *syndrome, unsigned int *bad_count, void *stream);

int lsec_locate_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                            long long block_size, int n_shift, long long first_stripe,
                            unsigned int *syndrome, unsigned long long *hyp,
                            unsigned char *located, unsigned char *located_dev,
                            unsigned int *counts, unsigned int *dev_faults,
                            int flags, void *stream);

/* The scrub's two questions in one pass: is the parity of each stripe consistent with its data
 * (lsec_check_dev's syndrome word), and are these the bytes that were written (the stripe's adler32
 * "magic", below, against the quorum magic stored in front of the chunks: jerase_control_check,
 * je_cksum_compare)?  The two do not catch the same faults -- a stale but self-consistent stripe (a
 * lost full-stripe write) has syndrome 0 and the wrong magic; with m = 2 two corrupt chunks can
 * imitate a third under the parity check -- and as lsec_check_dev followed by lsec_stripe_magic_dev
 * they cost 2(k+m) chunk reads per stripe.  Here the check's tiles, which hold every byte of the
 * stripe in registers, sum the magic too: k+m chunk reads.  The rotated call also gives the magics
 * of a rotated LUN on the device for stripes that are already stored (a full-stripe write gets them
 * from lsec_encode_magic_dev_rotated, below, in the pass that forms the parity).  Purely additive
 * too: the version stays 3, a caller detects the calls by their symbols.
 *
 * - shards, devs, n_shift and first_stripe mean exactly what they mean for lsec_check_dev /
 *   lsec_check_dev_rotated.  Every chunk is only read, exactly once; nothing proportional to the
 *   data is written.
 * - syndrome[s] (nstripes 32-bit words, 4-byte aligned, required with nstripes > 0): exactly the
 *   word lsec_check_dev / lsec_check_dev_rotated produces for stripe s.  The call sets it; it does
 *   not add to it.
 * - `magic` is device memory, 4*nstripes bytes, no alignment requirement, pure output, required
 *   with nstripes > 0.  Word s is the 4 little-endian bytes of zlib's adler32 over the k+m chunks of
 *   stripe s in LOGICAL order (for the rotated call: after un-rotating), exactly as
 *   lsec_stripe_magic_dev writes it.  An inconsistent stripe gets the adler32 of exactly the bytes
 *   stored: the call judges nothing but the syndrome and `expect`.
 * - `expect` is optional (NULL): device memory, 4*nstripes bytes, no alignment requirement, only
 *   read: the quorum magics.
 * - `bad` is optional (NULL), with or without expect: nstripes bytes, no alignment requirement.
 *   bad[s] = LSEC_SCRUB_BAD_PARITY when syndrome[s] != 0, OR'ed with LSEC_SCRUB_BAD_MAGIC when
 *   expect is given and magic[s] != expect[s].  Without expect only the parity bit can appear.
 * - `counts` is optional (NULL): two 32-bit words, 4-byte aligned.  counts[0] is the number of
 *   stripes with a nonzero syndrome, counts[1] the number whose magic differs from expect (0
 *   without expect).  The call sets both; it does not add to them.
 * - The outputs must not overlap one another or the shards.
 * - Scratch: the per-stripe accumulators, 16 bytes per stripe, come from the stream-ordered
 *   allocator (hipMallocAsync on `stream`), are zeroed there and go back to it on the stream,
 *   exactly as lsec_encode_magic_dev's do.  Nothing is uploaded: the kernels index the plan's
 *   cached encode image.
 * - n_shift == 0 behaves exactly as the unrotated call.
 * - nstripes == 0 validates the arguments, returns 0 and touches no GPU; all outputs may then be
 *   NULL.  Where lsec_check_dev accepts block_size == 0, every magic word comes out as 1 (adler32
 *   of nothing) and every syndrome as 0.
 * - Plans and limits are those of lsec_check_dev: lsec_plan_kernel 1 and 2, k <= 64, 1 <= m <= 8.
 *   Layout, alignment and block_size rules are those of lsec_check_dev.
 * - Everything lsec_check_dev / lsec_check_dev_rotated refuses is refused, in its order; behind
 *   those a NULL magic with nstripes > 0 and a misaligned counts.  Each returns -1 with a message
 *   for lsec_last_error that names this call and the limit, and nothing is enqueued: every
 *   argument check comes before the first HIP call.  There is no fallback to two passes.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
#define LSEC_SCRUB_BAD_PARITY 1   /* bad[s]: syndrome[s] != 0 */
#define LSEC_SCRUB_BAD_MAGIC  2   /* bad[s]: magic[s] != expect[s] */

int lsec_check_magic_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                         long long block_size, unsigned int *syndrome, void *magic,
                         const void *expect, unsigned char *bad, unsigned int *counts, void *stream);

int lsec_check_magic_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                 long long block_size, int n_shift, long long first_stripe,
                                 unsigned int *syndrome, void *magic, const void *expect,
                                 unsigned char *bad, unsigned int *counts, void *stream);

/* Parity update for a partial-stripe write, one pass: c of a stripe's k data chunks change, and the
 * parity follows without the other k - c chunks being read, or even being on the device.  Purely
 * additive too: the version stays 3, a caller detects the call by its symbol.
 *
 * - `shards` are the k+m logical chunks as for lsec_encode_dev, but only shards[cols[i]] (the old
 *   contents of the changed chunks) and shards[k .. k+m) (the parity) are used.  Every other data
 *   entry is ignored entirely: its base may be NULL or misaligned, it is not validated, and it
 *   never reaches the kernel, whose arguments carry only the c old, the c fresh and the m parity
 *   chunks.
 * - `cols` is a -1 terminated list of c distinct data chunk ids, 1 <= c <= k, each in 0..k-1, in
 *   any order; fresh[i] is the new content of chunk cols[i], under the layout rule of `shards`.
 * - Effect, per stripe and byte column: parity_r ^= sum_i g[r][cols[i]] * (old_i ^ fresh_i) for
 *   every r < m, g the plan's coding matrix (for Cauchy the bit-sliced product over packets, as the
 *   encode forms it).  Nothing else is computed.  So:
 *     1. a stripe that was consistent comes out with exactly the parity bytes lsec_encode_dev
 *        writes for the data with those chunks replaced;
 *     2. any stripe keeps its syndrome: lsec_check_dev over the stripe with the chunks replaced
 *        gives after the call the word it gave over the old stripe before it.  An inconsistent
 *        stripe is neither healed nor made worse.
 * - Without LSEC_UPDATE_STORE only the m parity chunks are written; shards[cols[i]] and fresh are
 *   only read.  With the flag shards[cols[i]] <- fresh[i] in the same pass, from the registers
 *   that hold the fresh bytes: one store more per unit and no further load.  fresh is never
 *   written.
 * - fresh must not overlap shards; the changed chunks and the parity must not overlap one another.
 * - Layout, alignment and block_size rules are those of lsec_encode_dev (lsec_shard_t, above; for
 *   Cauchy block_size is a multiple of 8 * packet_size), applied to the c old, the c fresh and the
 *   m parity chunks.
 * - Plans: lsec_plan_kernel 1 (bytewise GF(2^8): RS, r6, raid4) and 2 (bit-sliced GF(2^8): Cauchy
 *   at w = 8), k <= 64, 1 <= m <= 8.
 * - nstripes == 0 validates everything, returns 0 and touches no GPU; all bases may then be NULL,
 *   cols may not.
 * - Nothing is allocated and nothing is uploaded per call: the kernel indexes the plan's cached
 *   encode image by column.
 * - One column list per call.  Stripes that change in different chunks take
 *   lsec_update_dev_masked, below: one 64-bit word per stripe names its changed chunks, in one
 *   launch.  The form over the physical devices of a rotated LUN is lsec_update_dev_rotated, below.
 * - This call and lsec_update_dev_rotated leave the stripes' magics to the caller.  The masked
 *   calls have a form that keeps them current in the same pass (lsec_update_magic_dev_masked,
 *   below); one word repeated for every stripe expresses any column list.
 * - Every refusal -- plan kernels 3-5; k or m out of range; a NULL shards, cols or fresh; an empty
 *   list; an id < 0, an id >= k (a parity id) or a duplicate; more than k ids; unknown flag bits; a
 *   misaligned base, or a misaligned stride with nstripes > 1; a bad block_size; a negative
 *   nstripes -- returns -1 with a message for lsec_last_error that names the limit, and nothing is
 *   enqueued.  There is no fallback to re-encoding.
 * Enqueued on `stream`; returns without synchronising.  0 / -1. */
#define LSEC_UPDATE_STORE 1   /* flags: also write the fresh bytes over the old data chunks */

int lsec_update_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                    long long block_size, const int *cols, const lsec_shard_t *fresh,
                    int flags, void *stream);

/* Encode and parity update over the PHYSICAL devices of a rotated LUN, one pass each: the write
 * side of lsec_check_dev_rotated / lsec_locate_dev_rotated / lsec_decode_dev_rotated, so that a
 * caller that keeps device images on the GPU writes to them without splitting its stripes into
 * classes that share a chunk-to-device map.  Purely additive too: the version stays 3, a caller
 * detects the calls by their symbols.
 *
 * Both calls:
 * - devs[i] (i < k+m) is physical device i, exactly as for lsec_check_dev_rotated.  With
 *   rot_s = ((first_stripe + s) * n_shift) mod (k+m), logical chunk c of stripe s lives in
 *   devs[(c - rot_s) mod (k+m)].  n_shift >= k+m is taken mod k+m; n_shift < 0 and
 *   first_stripe < 0 return -1; first_stripe may be anything up to 2^63 - 1.
 * - Plans: lsec_plan_kernel 1 (bytewise GF(2^8): RS, r6, raid4) and 2 (bit-sliced GF(2^8): Cauchy
 *   at w = 8), k <= 64, 1 <= m <= 8.
 * - Layout, alignment and block_size rules are those of lsec_encode_dev (lsec_shard_t, above; for
 *   Cauchy block_size is a multiple of 8 * packet_size).  All k+m entries of devs are validated in
 *   every call: under rotation every device holds data in some stripes and parity in others.
 * - nstripes == 0 validates everything, returns 0 and touches no GPU; all bases may then be NULL,
 *   cols may not.
 * - Every refusal returns -1 with a message for lsec_last_error that names the limit, and nothing
 *   is enqueued.  There is no fallback.
 * - Nothing is allocated and nothing is uploaded per call: the kernels use the plan's cached
 *   encode image.
 * Enqueued on `stream`; return without synchronising.  0 / -1.
 *
 * lsec_encode_dev_rotated: for every stripe, reads the k logical data chunks from the devices that
 * hold them and writes the m parity chunks to the devices that hold them.
 * - The parity bytes are exactly what lsec_encode_dev writes for the logical view of the stripe;
 *   n_shift == 0 behaves exactly as lsec_encode_dev over devs.
 * - The data chunks are only read, and no byte outside the m parity chunks of each stripe is
 *   written.
 * - For Cauchy at w = 8 the bit-sliced table kernel runs even where lsec_encode_dev would run a
 *   compiled packet network, as for the check; the bytes are identical.
 * - The stripes' magics are not computed here.  A writer that stores [4-byte magic | chunk] on every
 *   device takes lsec_encode_magic_dev_rotated, below: the same bytes, and the magics from the same
 *   pass.
 *
 * lsec_update_dev_rotated: lsec_update_dev with the old chunks and the parity on the devices.
 * - `cols` is a -1 terminated list of c distinct LOGICAL data chunk ids, 1 <= c <= k, each in
 *   0..k-1, in any order, as for lsec_update_dev.  fresh[i] is the new content of logical chunk
 *   cols[i]: a logical buffer with its own base and stride, not rotated.
 * - Effect, per stripe and byte column: the parity chunk of row r, wherever the rotation puts it,
 *   takes ^= sum_i g[r][cols[i]] * (old_i ^ fresh_i), with old_i read from
 *   devs[(cols[i] - rot_s) mod (k+m)].  Both numbered guarantees of lsec_update_dev carry over:
 *   a consistent stripe comes out with the parity lsec_encode_dev_rotated writes for the data with
 *   those chunks replaced, and any stripe keeps its syndrome under lsec_check_dev_rotated.
 * - With LSEC_UPDATE_STORE fresh[i] also goes over the old chunk on its device, in the same pass,
 *   from the registers that hold the fresh bytes.  Without it only parity is written.
 * - The chunks that do not change are not read, although they live in devs.
 * - fresh must not overlap devs.
 * - Refused: everything lsec_update_dev refuses -- plan kernels 3-5; k or m out of range; a NULL
 *   devs, cols or fresh; an empty list; an id < 0, an id >= k or a duplicate; more than k ids;
 *   unknown flag bits; a misaligned base (on any of the k+m devices or of fresh), or a misaligned
 *   stride with nstripes > 1; a bad block_size; a negative nstripes -- and a negative n_shift or
 *   first_stripe. */
int lsec_encode_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                            long long block_size, int n_shift, long long first_stripe, void *stream);

int lsec_update_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                            long long block_size, int n_shift, long long first_stripe,
                            const int *cols, const lsec_shard_t *fresh, int flags, void *stream);

/* lsec_encode_dev_rotated that also leaves each stripe's adler32 magic, one pass: the full-stripe
 * write of a rotated LUN together with the word LStore stores in front of every chunk
 * ([4-byte magic | chunk] on every device, segjerase_write_func).  As lsec_encode_dev_rotated followed
 * by lsec_check_magic_dev_rotated the writer pays 2k+m chunk reads and m chunk writes per stripe and a
 * parity re-computation whose answer is known; here the encode's tiles, which hold every byte of the
 * stripe in registers -- the k inputs as loaded, the m rows as formed -- sum the magic too: k chunk
 * reads and m chunk writes.  Purely additive too: the version stays 3, a caller detects the call by
 * its symbol.
 *
 * - devs, n_shift and first_stripe mean exactly what they mean for lsec_encode_dev_rotated, and the
 *   bytes left on the devices are exactly those it leaves for the same arguments: the data chunks
 *   are only read, once each, and no byte outside the m parity chunks of each stripe is written.
 * - `magic` is device memory, 4*nstripes bytes, no alignment requirement, pure output, required with
 *   nstripes > 0.  Word s is the 4 little-endian bytes of zlib's adler32 over the k+m chunks of
 *   stripe s in LOGICAL order -- data 0..k-1, then the parity rows just formed -- exactly what
 *   lsec_check_magic_dev_rotated would write behind the encode, and what lsec_encode_magic_dev
 *   writes for the logical view.  Rotation moves where chunks live, never their position in the sum.
 * - magic must not overlap the devices.
 * - n_shift == 0 behaves exactly as lsec_encode_magic_dev over devs, in bytes and in magics.
 * - Scratch: the per-stripe accumulators, 16 bytes per stripe, come from the stream-ordered
 *   allocator (hipMallocAsync on `stream`), are zeroed there and go back to it on the stream,
 *   exactly as lsec_encode_magic_dev's and lsec_check_magic_dev's do; they are freed too when a
 *   launch fails.  Nothing is uploaded: the kernels use the plan's cached encode image.
 * - Plans and limits: lsec_plan_kernel 1 and 2, k <= 64, 1 <= m <= 8.  Layout, alignment and
 *   block_size rules are those of lsec_encode_dev_rotated; all k+m entries of devs are validated.
 *   For Cauchy at w = 8 the bit-sliced table kernel runs at every shape, as for
 *   lsec_encode_dev_rotated.
 * - nstripes == 0 validates everything, returns 0 and touches no GPU; magic and all bases may then
 *   be NULL.  Where lsec_encode_dev_rotated accepts block_size == 0 with nstripes > 0, every magic
 *   word comes out as 1 (adler32 of nothing) and no chunk is touched: the rule of
 *   lsec_check_magic_dev.
 * - Everything lsec_encode_dev_rotated refuses is refused, in its order; behind that a NULL magic
 *   with nstripes > 0.  Each returns -1 with a message for lsec_last_error that names this call and
 *   the limit, and nothing is enqueued: every argument check comes before the first HIP call.
 *   There is no fallback to two passes.
 * - No `expect`: a write has no quorum to compare with.
 * Enqueued on `stream`; returns without synchronising.  0 / -1. */
int lsec_encode_magic_dev_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                  long long block_size, int n_shift, long long first_stripe,
                                  void *magic, void *stream);

/* The parity update with a changed set PER STRIPE, one pass: lsec_update_dev and
 * lsec_update_dev_rotated for a batch whose stripes do not change in the same chunks -- the first
 * and the last stripe of a contiguous byte-range write, or a batch of small random writes -- without
 * sorting the stripes into classes and launching once per class.  Purely additive too: the version
 * stays 3, a caller detects the calls by their symbols.
 *
 * Both calls:
 * - `stripe_cols` is device memory: nstripes 64-bit words, 8-byte aligned.  Bit j (j < k) of
 *   stripe_cols[s] means "data chunk j of stripe s changes".  It is only read; the caller must not
 *   change it while the call is in flight; it must not overlap shards / devs or fresh.
 * - `fresh` has k entries INDEXED BY LOGICAL CHUNK ID: fresh[j] is the new content of chunk j, under
 *   the layout rule of lsec_shard_t.  (lsec_update_dev's fresh[i] goes with cols[i]; this one does
 *   not.)  The usual write buffer is fresh[j] = {wbuf + j*C, k*C}.  fresh is never written.
 * - Column j is ENABLED when fresh[j].base != NULL.  Only enabled columns are validated (base and
 *   stride alignment of fresh[j], and in the unrotated call of shards[j], whose base must not be
 *   NULL either); shards[j] of a column that is not enabled is ignored entirely, as lsec_update_dev
 *   ignores the chunks that do not change.  The m parity entries are always validated; in the
 *   rotated call all k+m devs are, as for lsec_update_dev_rotated.
 * - The effective mask of stripe s is stripe_cols[s] & enabled & (the k low bits).  Bits >= k and
 *   bits of columns that are not enabled are ignored: no address is ever formed from a ref the
 *   call was not given, and the coding matrix is never indexed past column k-1.
 * - Effect, per stripe and byte column: parity_r ^= sum over j in the effective mask of
 *   g[r][j] * (old_j ^ fresh_j) for every r < m (for Cauchy the bit-sliced product over packets, as
 *   the encode forms it).  The bytes left in a stripe are exactly those lsec_update_dev (or
 *   lsec_update_dev_rotated) leaves for that stripe with cols = the set bits, the changed chunks
 *   under LSEC_UPDATE_STORE included, and both numbered guarantees of lsec_update_dev carry over
 *   per stripe: a consistent stripe gets the reference's parity for the replaced data, and any
 *   stripe keeps its syndrome.
 * - A stripe whose effective mask is 0 is neither read nor written, apart from its mask word.
 *   Chunks outside the mask are not read.
 * - `flags` is LSEC_UPDATE_STORE or 0, uniform over the call.
 * - Plans, limits (k <= 64, 1 <= m <= 8, plan kernels 1 and 2), layout, alignment and block_size
 *   rules are those of lsec_update_dev.  nstripes == 0 validates everything, returns 0 and touches
 *   no GPU; all bases and stripe_cols may then be NULL (shards / devs and fresh themselves may not).
 * - Nothing is allocated and nothing is uploaded per call: the masks are read where they lie, and
 *   the kernel indexes the plan's cached encode image by column.
 * - Every refusal -- plan kernels 3-5; k or m out of range; a NULL shards / devs or fresh; unknown
 *   flag bits; a negative n_shift or first_stripe; with nstripes > 0 no enabled column; a
 *   misaligned base of an enabled column's fresh or shard, of a parity chunk or of a device, or
 *   such a stride with nstripes > 1; with nstripes > 0 an enabled column whose shards[j].base is
 *   NULL (unrotated call); a NULL or misaligned stripe_cols with nstripes > 0; a bad block_size; a
 *   negative nstripes -- returns -1 with a message for lsec_last_error that names the call and the
 *   limit, and nothing is enqueued.  There is no fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1.
 *
 * lsec_update_dev_masked_rotated: devs, n_shift and first_stripe mean what they mean for
 * lsec_update_dev_rotated; the masks and fresh are logical.  Old chunk j of stripe s is read from
 * devs[(j - rot_s) mod (k+m)], and with LSEC_UPDATE_STORE written there. */
int lsec_update_dev_masked(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                           long long block_size, const unsigned long long *stripe_cols,
                           const lsec_shard_t *fresh, int flags, void *stream);

int lsec_update_dev_masked_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                   long long block_size, int n_shift, long long first_stripe,
                                   const unsigned long long *stripe_cols,
                                   const lsec_shard_t *fresh, int flags, void *stream);

/* The masked parity update that also keeps the stripes' magics current, one pass:
 * lsec_update_dev_masked / lsec_update_dev_masked_rotated, and magic[s] -- the 4-byte adler32 LStore
 * stores in front of every chunk of stripe s (below) -- moved from the old stripe's to the new
 * stripe's.  A partial-stripe write changes the magic, and the only other way to the new one is
 * lsec_stripe_magic_dev over all k+m chunks behind the update: a second pass over exactly the chunks
 * the update does not read and that need not be on the device.  adler32's two halves are sums over
 * byte positions, so the write moves them by sums over the changed positions alone, and the update's
 * kernels hold those bytes -- old and fresh data, parity before and after -- in registers.  Purely
 * additive too: the version stays 3, a caller detects the calls by their symbols.
 *
 * Everything lsec_update_dev_masked and lsec_update_dev_masked_rotated specify holds unchanged: the
 * arguments, the enabled columns and the effective mask, LSEC_UPDATE_STORE, the bytes left in the
 * stripes, the layout rules and the limits (plan kernels 1 and 2, k <= 64, 1 <= m <= 8), and that
 * nstripes == 0 touches no GPU.
 * - `magic` is device memory, 4*nstripes bytes: word s is 4 little-endian bytes, as
 *   lsec_stripe_magic_dev writes them.  No alignment requirement, as for that call.  It is read and
 *   written; it must not overlap shards / devs, fresh or stripe_cols.  NULL with nstripes > 0 is
 *   refused, NULL with nstripes == 0 is fine.
 * - Effect, for a stripe whose effective mask is not 0, with A_in / B_in the low / high 16 bits of
 *   magic[s] on entry: each half comes out as (in + d) mod 65521, d taken over the changed data
 *   chunks and the m parity chunks: dA = sum (new_p - old_p), dB = sum (L - p)(new_p - old_p) over
 *   their byte positions p in the LOGICAL stripe -- chunk j at j*block_size, parity row r at
 *   (k+r)*block_size, L = (k+m)*block_size.  Rotation does not enter: the magic is over logical
 *   order, as lsec_segment_write computes it.  So if magic[s] was adler32(old stripe) it comes out
 *   as adler32(new stripe), bit-exact with zlib, whether or not the stripe is consistent; and a half
 *   that was off by d stays off by d: a wrong magic is neither healed nor hidden, the counterpart of
 *   "any stripe keeps its syndrome".
 * - A half of 65521 or more can never be an adler32 half.  It is not folded into a valid one: that
 *   half comes out as 0xFFFF.  Invalid stays invalid.
 * - The magic word of a stripe whose effective mask is 0 is neither read nor written, whatever it
 *   holds.
 * - With or without LSEC_UPDATE_STORE the magic is that of the stripe with the chunks replaced;
 *   without the flag the caller puts the fresh bytes in place itself, as for the plain calls.
 * - Scratch: the per-stripe accumulators, 16 bytes per stripe, come from the stream-ordered
 *   allocator (hipMallocAsync on `stream`) and go back to it on the stream, exactly as
 *   lsec_encode_magic_dev's do.  Nothing is uploaded: the masks are read where they lie.
 * - Only the masked family has this form.  A caller of lsec_update_dev / lsec_update_dev_rotated
 *   gets it by passing the same word for every stripe (bit cols[i] set, fresh[cols[i]] = its
 *   fresh[i]).
 * - Every refusal -- those of the masked calls, in their order, and a NULL magic with nstripes > 0,
 *   behind the stripe_cols ones -- returns -1 with a message for lsec_last_error that names this
 *   call and the limit, and nothing is enqueued.  There is no fallback.
 * Enqueued on `stream`; return without synchronising.  0 / -1. */
int lsec_update_magic_dev_masked(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                                 long long block_size, const unsigned long long *stripe_cols,
                                 const lsec_shard_t *fresh, int flags, void *magic, void *stream);

int lsec_update_magic_dev_masked_rotated(lio_erasure_plan_t *plan, const lsec_shard_t *devs, int nstripes,
                                         long long block_size, int n_shift, long long first_stripe,
                                         const unsigned long long *stripe_cols, const lsec_shard_t *fresh,
                                         int flags, void *magic, void *stream);

/* Per-stripe "magic": the 4-byte little-endian zlib adler32 over the concatenation of a
 * stripe's k+m chunks that LStore's erasure segment stores in front of every chunk
 * (je_cksum_calc, src/lio/segment/jerasure.c:169-182; checked by je_cksum_compare, :188-194).
 * Computed on the GPU.  magic receives 4*nstripes bytes (host memory for et_*, device memory
 * for lsec_*_dev).  The *_encode_* forms encode first and checksum data + fresh parity,
 * which is what segjerase_write_func does per stripe (:1847-1850). */
int et_encode_stripes_magic(lio_erasure_plan_t *plan, char **ptrs, int nstripes, int block_size, char *magic);
int et_stripes_magic(lio_erasure_plan_t *plan, char **ptrs, int nstripes, int block_size, char *magic);
int lsec_encode_magic_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                          long long block_size, void *magic, void *stream);
int lsec_stripe_magic_dev(lio_erasure_plan_t *plan, const lsec_shard_t *shards, int nstripes,
                          long long block_size, void *magic, void *stream);

/* Batched write side of LStore's erasure segment (segjerase_write_func,
 * src/lio/segment/jerasure.c:1640-1895, for whole-stripe-aligned writes) including the LUN
 * child's placement (lun_row_decompose, src/lio/segment/lun.c:1140-1246).
 * data: nstripes*k*C user bytes (host memory, stripe-major, as the cache page holds them).
 * dev[i] (i = 0..k+m-1, host memory, nstripes*(C+4) bytes each) receives, at offset
 * s*(C+4), the LUN chunk [4-byte stripe magic | chunk j] with
 * j = (i + (first_stripe + s)*n_shift) % (k+m) -- data chunk j for j < k, parity j-k else.
 * Parity and magics are computed on the GPU.  0 / -1. */
int lsec_segment_write(lio_erasure_plan_t *plan, const char *data, int nstripes, int chunk, int n_shift,
                       long long first_stripe, char **dev);
/* The same with the user data as a scatter list (the tbuf's iovecs, segment/jerasure.c:1786-1825):
 * stripe s covers bytes [s*k*C, (s+1)*k*C) of the concatenated pieces.  A stripe inside one
 * piece is read in place; a stripe straddling pieces is gathered into a contiguous copy first
 * (:1795-1811); a stripe whose first piece is an error page (iov_base NULL) is encoded and
 * written as zero data chunks (:1816, :1823-1831).  Error pages inside a straddling stripe read
 * as zeros (the reference would read through the NULL base).  0 / -1 (fewer than nstripes*k*C
 * bytes listed is an error). */
struct iovec;
int lsec_segment_write_iov(lio_erasure_plan_t *plan, const struct iovec *iov, int n_iov, int nstripes, int chunk,
                           int n_shift, long long first_stripe, char **dev);
/* segjerase_write_func's own hand-off, with no data copy (segment/jerasure.c:1780-1858): for
 * nstripes stripes of the scatter list `iov` (as lsec_segment_write_iov reads it), the parity
 * goes to `parity` (caller memory, nstripes*m*C bytes, stripe-major: parity chunk r of stripe s
 * at (s*m + r)*C, the reference's per-op parity buffer) and the stripe magics to `magic`
 * (nstripes*4 bytes), both computed on the GPU; `out` receives 2*(k+m)*nstripes iovecs
 * [4-byte magic | chunk] in logical chunk order (data 0..k-1 then parity 0..m-1 per stripe):
 * the tbuf the reference hands its LUN child (:1852-1853).  Data iovecs point into the caller's
 * pages; a stripe straddling scatter pieces is gathered into `straddle` (k*C bytes per such
 * stripe, lsec_segment_straddle_bytes tells how many bytes); a stripe starting in an error page
 * points at an engine-owned zero chunk.  Returns the number of iovecs, or -1. */
int lsec_segment_encode_iov(lio_erasure_plan_t *plan, const struct iovec *iov, int n_iov, int nstripes, int chunk,
                            char *parity, char *magic, char *straddle, long long straddle_bytes, struct iovec *out,
                            int out_cap);
long long lsec_segment_straddle_bytes(lio_erasure_plan_t *plan, const struct iovec *iov, int n_iov, int nstripes,
                                      int chunk);

/* Flags of the read / inspect entry points */
#define LSEC_READ_PARANOID 1   /* verify every stripe, not only those with bad chunks */
#define LSEC_MAGIC_LEGACY  2   /* segment magic_cksum == 0: magics are not adler32 sums, so
                                  stripes are verified with control chunks (jerasure.c:218-266) */
#define LSEC_INSPECT_FIX   4   /* inspect: repair in place (INSPECT_{QUICK,SCAN,FULL}_REPAIR) */
#define LSEC_MAX_DEVS      256  /* k + m of the segment paths, of w = 8 and of the bitmatrix codes;
                                  the GF(2^16) / GF(2^32) matrix codes (RS, r6, Cauchy) take up
                                  to LSEC_MAX_DEVS_WIDE through the et_* / lsec_*_dev calls */
#define LSEC_MAX_DEVS_WIDE 1024

/* Batched read side for whole stripes (segjerase_read_func, segment/jerasure.c:1255-1631):
 * dev[i] are device images laid out as lsec_segment_write writes them (NULL = device
 * unreadable).  Per stripe: majority vote over the stored magics (:1383-1438); stripes with
 * chunks outside the quorum are rebuilt (decode) and verified (jerase_control_check,
 * :202-269: against the quorum magic, or with control chunks under LSEC_MAGIC_LEGACY),
 * falling back to the brute-force search over erasure combinations (jerase_brute_recovery,
 * :321-339); with LSEC_READ_PARANOID every stripe is verified.  Checks and rebuilds run as
 * GPU batches.  User data (nstripes*k*C) goes to data_out; status[s] (optional) = 0 ok,
 * 1 recovered (a data chunk was rebuilt), 2 blank (zero-filled), -1 unrecoverable.  Returns the number of
 * unrecoverable stripes, or -1 on error. */
int lsec_segment_read(lio_erasure_plan_t *plan, char **dev, int nstripes, int chunk, int n_shift,
                      long long first_stripe, int flags, char *data_out, int *status);

/* Full byte-level inspection and optional repair (segjerase_inspect_full_func,
 * segment/jerasure.c:347-732).  buf holds nstripes stripes as the inspection reads them from
 * the LUN child: stripe-major, k+m records of [4-byte magic | chunk] each
 * (stripe_size_with_magic = (k+m)*(C+4)).  Every stripe is classified as the reference does:
 * stripe_status[s] = LSEC_STRIPE_*; badmap[s*(k+m)+j] = 1 for the devices the reference's
 * badmap holds after the stripe (what [DEVMAP] prints).  With LSEC_INSPECT_FIX the repaired
 * chunks and magics are written into buf and rewrite[s*(k+m)+j] = 1 marks every record the
 * reference writes back (all of them under LSEC_MAGIC_LEGACY, which converts the stripe to
 * adler32 magics).  `state` carries the counters and the brute-force guess between
 * consecutive calls of one inspection (zero it first).  Returns 0, or -1 on error. */
enum {
  LSEC_STRIPE_OK = 0,            /* every magic agrees and the stripe verifies */
  LSEC_STRIPE_EMPTY = 1,         /* never written: zero magics, zero data (skipped) */
  LSEC_STRIPE_BAD_MAGIC = 2,     /* some magics disagree; the rebuild of those devices verifies */
  LSEC_STRIPE_REPAIRED = 3,      /* silent corruption found by the brute-force search ("r-mismatch") */
  LSEC_STRIPE_LOST_MAGIC = 4,    /* too few matching magics to rebuild ("magic") */
  LSEC_STRIPE_LOST_MISMATCH = 5  /* data and parity disagree beyond repair ("u-mismatch") */
};
typedef struct {
  long long bad_stripes;      /* sf->bad_stripes (bad_count) */
  long long unrecoverable;    /* unrecoverable_count */
  long long silent_errors;    /* erasure_errors: stripes whose check failed */
  long long empty_stripes;    /* n_empty */
  int brute_used;             /* bm_brute_used */
  unsigned char brute_badmap[LSEC_MAX_DEVS];  /* badmap_brute */
} lsec_inspect_state_t;
int lsec_segment_inspect(lio_erasure_plan_t *plan, char *buf, int nstripes, int chunk, int flags,
                         int *stripe_status, unsigned char *badmap, unsigned char *rewrite,
                         lsec_inspect_state_t *state);

/* Pre-build (and cache on the current device) the decode matrix for one erasure pattern,
 * so the first lsec_decode_dev of that pattern does no host work.  0 / -1. */
int lsec_prepare_decode(lio_erasure_plan_t *plan, const int *erasures);
/* The same for the encode image.  For wide matrix codes (R*K >= 96 at w = 8) both also wait
 * for the plan's run-time compiled XOR network (ec_jit.cpp); until it is ready the table
 * kernel serves.  0 / -1. */
int lsec_prepare_encode(lio_erasure_plan_t *plan);
/* 1 when the encode (erasures == NULL) or the decode of that erasure pattern runs on a
 * compiled network on the current device (wide GF(2^8) RS codes; RS / r6 at w = 16 / 32; the
 * packet networks of the liberation family and of Cauchy at w = 16 / 32, and at w = 8 with more
 * than four outputs -- at the plan's strip_size), 0 otherwise. */
int lsec_plan_jit(lio_erasure_plan_t *plan, const int *erasures);

/* Devices that serve host-memory calls (et_*_stripes, et_*_magic, the plan's fn-pointers,
 * lsec_segment_write).  n = 0 (the default): the calling thread's current HIP device.  With a
 * set, a batch larger than the coalescing limit is split into contiguous stripe ranges, one
 * per listed device, each staged and computed on its own device and PCIe link in parallel;
 * smaller calls go to the listed devices in turn.  A device may be listed more than once.
 * 0 / -1 (unknown device). */
int lsec_set_host_devices(const int *devices, int n);
/* Host NUMA placement of device `dev`: its node (-1 if unknown) in *node and up
 * to max_cpus of that node's CPUs this process may use in cpus[].  The engine pins a device's
 * dispatcher thread, the threads running its share of a split host batch and the copy pool that
 * packs its page-locked staging to these CPUs (LSEC_NUMA=0: no pinning).  A caller that owns a
 * device (one process per GPU) can pin itself there before it allocates its host buffers.
 * Returns the number of CPUs (0: no placement known), or -1 (no such device). */
int lsec_device_numa(int dev, int *node, int *cpus, int max_cpus);

/* Engine information / control */
int lsec_abi_version(void);
int lsec_device_count(void);                 /* visible HIP devices, 0 if none */
const char *lsec_last_error(void);           /* thread-local message of the last failure */
/* kernel that applies the plan: 1 = bytewise GF(2^8) (RS, r6, raid4), 2 = bit-sliced GF(2^8)
 * (Cauchy w = 8), 3 = GF(2) bitmatrix (liberation family), 4 = wordwise GF(2^16) / GF(2^32)
 * (RS, r6 at w = 16/32), 5 = bit-sliced GF(2^16) / GF(2^32) (Cauchy at w = 16/32),
 * 0 = no GPU kernel (calls fail with -1) */
int lsec_plan_kernel(lio_erasure_plan_t *plan);
void lsec_set_kernel_variant(int bytewise_variant, int bitsliced_variant);  /* tuning experiments */
/* How the streaming kernels deal their tiles to the 8 XCDs (LSEC_TILES=static|shared|tail picks
 * the start value; default tail): 0 = each XCD its static eighth; 1 = persistent grid, each XCD
 * takes tiles from its own eighth through an atomic counter and then helps the others; 2 = the
 * first 7/8 of each eighth static, the rest shared.  For A/B runs; results are identical in every
 * mode. */
void lsec_set_tile_sharing(int mode);
int lsec_tile_sharing(void);
/* Pageable host chunks a call pins in place (hipHostRegister) are unregistered before the call
 * returns.  Opt-in (LSEC_DEFER_UNPIN_MB > 0, for a process where this library is the only HIP
 * user): while other calls hold registrations of their own, a background thread does it instead,
 * shortly after the call returns (hipHostUnregister waits until the whole device is idle).  With
 * that on, a caller that registers host memory with HIP itself, or hands memory it may have freed
 * and reallocated to another HIP user, calls this first: it returns when nothing is pending.  0. */
int lsec_host_unpin_drain(void);
/* Measurement probe, not part of the coding path: enqueue a streaming device copy dst <- src
 * (bytes a multiple of 16, 16-byte aligned device pointers) on `stream` with the coding kernels'
 * memory shape; bench.py times it as the box's practical HBM ceiling.  0 / -1. */
int lsec_hbm_copy_dev(void *dst, const void *src, unsigned long long bytes, void *stream);
/* Measurement probe: for every stripe, shards[k+r] <- XOR of shards[0..k) (r < m <= 16), with
 * the RS encode kernel's tiles: the encode's k-read : m-write HBM traffic without its GF
 * arithmetic, which bench.py times beside the encode.  0 / -1. */
int lsec_hbm_mix_dev(const lsec_shard_t *shards, int k, int m, int nstripes, long long block_size, void *stream);

/* Measurement probe: for every stripe, shards[k] <- XOR of shards[0..k), in a kernel that shares
 * no code with the coding kernels: the single-erasure decode's k-read : 1-write HBM traffic with
 * the plainest streaming code.  variant = IT | G << 4 | REMAP << 8: IT (1, 2, 4) 16-byte steps
 * per lane, G (1, 2, 4) tiles of 4096 * IT bytes per workgroup, REMAP 1 = XCD-contiguous grabs;
 * block_size a multiple of 4096 * IT.  bench.py times every variant beside the decode.  0 / -1. */
int lsec_hbm_decode_shape_dev(const lsec_shard_t *shards, int k, int nstripes, long long block_size, int variant,
                              void *stream);
#ifdef __cplusplus
}
#endif

#endif /* LSTORE_EC_H */
