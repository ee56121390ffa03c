// ec_vote.h -- launch interface of the quorum-vote kernels (lsec_vote_dev / lsec_vote_dev_rotated; internal to
// liblstore_ec, kernels in ec_vote_inst.hip).
//
// The head of LStore's read and scrub path, per stripe: the majority vote over the k+m stored 4-byte magics and the
// classification built on it (segjerase_read_func's first step, segment/jerasure.c:1383-1462).  Three launches on one
// stream over 16 bytes of scratch per stripe (VoteScratch, zeroed by the caller):
//
//   vote      one wave64 per stripe, kVoteWaves stripes per workgroup, no LDS and no barrier.  Lane c holds the stored
//             word of LOGICAL chunk c, loaded bytewise from stored[(c - rot_s) mod n] (rot_s from rot0 / rot_step /
//             rot_n exactly as CheckRotArgs works it out; rot_n = 0: the entries are the logical chunks).  A NULL base
//             is an unreadable chunk: in no group.  The groups come from a loop over the not-yet-grouped mask -- the
//             leader is its lowest set bit, its word is broadcast, the equal readable lanes ballot -- and the best is
//             replaced only by a strictly larger one, which is the reference's "first group with the largest count".
//             The wave writes the quorum's 4 bytes, the outside mask, a provisional class (kVoteBlank: a blank
//             CANDIDATE, all n chunks in a quorum of zero bytes, and only with `scan`) and the pattern whose erasure
//             mask equals the outside mask (masks: one 64-bit word per pattern, 64 per step of the wave).
//   scan      the blank scan, one workgroup per (stripe, chunk, piece of the chunk).  A tile reads its stripe's
//             provisional class before any chunk load and leaves unless it is kVoteBlank; a candidate's tile ORs
//             16-byte lanes, ballots once per wave, and a wave that saw a nonzero byte stores kVoteOk over the
//             class: one fixed value, so the store needs no atomic.  A stripe that is no candidate costs no chunk read.
//   finalize  one thread per stripe: the final cls, ids and counts.
#pragma once

#include "ec_kernels.h"

namespace lsec {

constexpr unsigned kVoteOk = 0, kVoteDegraded = 1, kVoteBlank = 2, kVoteLost = 3;  // LSEC_VOTE_* (lstore_ec.h)
constexpr int kVoteMaxShards = 64;  // one bit of the outside mask and one lane of the wave each
constexpr int kVoteWaves = 4;       // stripes per workgroup of the vote launch

struct alignas(16) VoteScratch {
  unsigned long long outside;  // bit c: logical chunk c is outside the quorum
  uint32_t cls;                // provisional class; the scan turns kVoteBlank into kVoteOk
  uint32_t id;                 // the lowest pattern whose mask equals `outside`, or kLocateMany
};
static_assert(sizeof(VoteScratch) == 16, "VoteScratch: the 16 bytes of scratch per stripe");

struct VoteArgs {
  const unsigned long long *masks;  // npat erasure masks (device memory), or null: no lookup
  uint32_t npat;
  uint32_t rot0, rot_step, rot_n;   // rot_n = n: rotated; 0: stored[] are the logical chunks
  int n, K;                         // k + m <= kVoteMaxShards, k
  int nstripes;
  int scan;                         // != 0: the chunks were given, blank candidates are marked
  uint8_t *quorum;                  // 4 bytes per stripe, no alignment
  unsigned long long *outside;      // nstripes words, or null
  VoteScratch *scratch;             // nstripes records
  ShardRef stored[kVoteMaxShards];  // the stored magics: 4 bytes at base + s * stride, no alignment; base 0: unreadable
};
static_assert(sizeof(VoteArgs) < 4096, "VoteArgs: under the 4 KiB of kernel arguments");

struct VoteScanArgs {
  VoteScratch *scratch;             // the vote's records: cls is read, and demoted
  int n;
  int nstripes;
  int64_t size;                     // bytes per chunk (a multiple of 8)
  ShardRef sh[kVoteMaxShards];      // the chunks, in any order: a candidate's are all looked at
};

hipError_t launch_vote(const VoteArgs &a, hipStream_t stream);
// plain_loads: 0 non-temporal loads, 1 plain ones; steps: 16-byte steps per lane of a tile (2 or 4).  nstripes * n *
// (tiles per chunk) < 2^31.
hipError_t launch_vote_scan(const VoteScanArgs &a, int plain_loads, int steps, hipStream_t stream);
constexpr int64_t vote_scan_tile_bytes(int steps) { return 256 * 16 * static_cast<int64_t>(steps); }
// cls: nstripes bytes; ids: nstripes bytes or null (paranoid: an OK stripe gets its lookup's id, else kLocateClean);
// counts: five words zeroed by the caller, or null; lookups: masks were given (else no stripe counts in counts[4]).
hipError_t launch_vote_finalize(const VoteScratch *scratch, int nstripes, int paranoid, int lookups, uint8_t *cls, uint8_t *ids,
                                unsigned *counts, hipStream_t stream);

}  // namespace lsec
