// ec_vote_inst.hip -- the quorum-vote kernels of lsec_vote_dev / lsec_vote_dev_rotated (ec_vote.h has the contract)
// and their launchers, in a translation unit of their own so that no other object changes.
#include "ec_kernels_impl.h"
#include "ec_vote.h"

namespace lsec {
namespace {

__device__ __forceinline__ unsigned long long low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// One wave64 per stripe; lane c is logical chunk c.  Every lane of a live wave stays active to the end, so each
// ballot covers the whole wave; lanes at or past n are never readable.
__global__ __launch_bounds__(kVoteWaves * 64) void k_vote(VoteArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kVoteWaves + (threadIdx.x >> 6);
  if (s >= a.nstripes) return;  // (the whole wave: s does not depend on the lane)
  const uint32_t n = static_cast<uint32_t>(a.n);
  uint32_t word = 0;
  bool readable = false;
  if (lane < n) {
    uint32_t i = lane;
    if (a.rot_n) {  // logical chunk c sits at entry (c - rot_s) mod n
      const uint32_t rot_s = static_cast<uint32_t>((a.rot0 + static_cast<uint64_t>(s % a.rot_n) * a.rot_step) % a.rot_n);
      i = (lane + n - rot_s) % n;
    }
    const ShardRef ref = a.stored[i];
    if (ref.base) {
      readable = true;
      const LSEC_GLOBAL uint8_t *b = gptr<uint8_t>(ref.base + static_cast<uint64_t>(s * ref.stride));
      word = b[0] | (b[1] << 8) | (b[2] << 16) | (static_cast<uint32_t>(b[3]) << 24);
    }
  }
  // the groups, in the order of their lowest members; the best is replaced only by a strictly larger one
  unsigned long long todo = __ballot(readable), best = 0;
  uint32_t best_count = 0, best_word = 0;
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t lw = __shfl(word, leader);
    const unsigned long long group = __ballot(readable && word == lw);
    const uint32_t count = __popcll(group);
    if (count > best_count) {
      best_count = count;
      best = group;
      best_word = lw;
    }
    todo &= ~group;
  }
  const unsigned long long outside = ~best & low_bits(a.n);
  uint32_t cls;
  if (best_count == 0 || best_count < static_cast<uint32_t>(a.K)) cls = kVoteLost;
  else if (outside & low_bits(a.K)) cls = kVoteDegraded;
  else cls = a.scan && outside == 0 && best_word == 0 ? kVoteBlank : kVoteOk;
  // the lowest pattern whose erasure set is the outside set: 64 masks per step
  uint32_t id = kLocateMany;
  if (a.masks) {
    for (uint32_t p0 = 0; p0 < a.npat; p0 += 64) {
      const uint32_t p = p0 + lane;
      const unsigned long long hit = __ballot(p < a.npat && a.masks[p < a.npat ? p : 0] == outside);
      if (hit) {
        id = p0 + static_cast<uint32_t>(__ffsll(hit) - 1);
        break;
      }
    }
  }
  if (lane < 4) a.quorum[4 * s + lane] = static_cast<uint8_t>(best_word >> (8 * lane));
  if (lane == 0) {
    if (a.outside) a.outside[s] = outside;
    VoteScratch r;
    r.outside = outside;
    r.cls = cls;
    r.id = id;
    a.scratch[s] = r;
  }
}

template <bool PLAIN>
__device__ __forceinline__ u32x4 scan_load(uint64_t addr) {
  if constexpr (PLAIN) return *gptr<u32x4>(addr);
  else return __builtin_nontemporal_load(gptr<u32x4>(addr));
}

// One workgroup per (stripe, chunk, piece of IT * 4 KiB): lane steps of 16 bytes, an 8-byte one at a ragged end
// (chunks are multiples of 8 bytes, 8-byte aligned).
template <bool PLAIN, int IT>
__global__ __launch_bounds__(kBlock) void k_vote_scan(VoteScanArgs a) {
  constexpr int64_t kTile = kBlock * 16 * IT;
  const int64_t C = a.size;
  const uint32_t tps = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t t = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t sc = t / tps;  // stripe * n + chunk
  const uint32_t s = sc / static_cast<uint32_t>(a.n), i = sc - s * static_cast<uint32_t>(a.n);
  if (s >= static_cast<uint32_t>(a.nstripes)) return;
  if (a.scratch[s].cls != kVoteBlank) return;  // no candidate (or one already demoted): none of its chunks is read
  const uint64_t base = a.sh[i].base + static_cast<uint64_t>(static_cast<int64_t>(s) * a.sh[i].stride);
  const int64_t off0 = static_cast<int64_t>(t - sc * tps) * kTile + threadIdx.x * 16;
  u32x4 acc = 0u;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int64_t o = off0 + static_cast<int64_t>(it) * kBlock * 16;
    if (o + 16 <= C) {
      acc |= scan_load<PLAIN>(base + o);
    } else if (o < C) {
      const u32x2 h = *gptr<u32x2>(base + o);
      acc.x |= h.x;
      acc.y |= h.y;
    }
  }
  const bool nonzero = (acc.x | acc.y | acc.z | acc.w) != 0;
  if (__ballot(nonzero) != 0 && (threadIdx.x & 63) == 0) a.scratch[s].cls = kVoteOk;  // a plain store of one fixed value
}

__global__ void k_vote_finalize(const VoteScratch *scratch, int nstripes, int paranoid, int lookups, uint8_t *cls, uint8_t *ids,
                                unsigned *counts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nstripes) return;
  const VoteScratch r = scratch[s];
  cls[s] = static_cast<uint8_t>(r.cls);
  const bool looked = lookups && (r.cls == kVoteDegraded || (r.cls == kVoteOk && paranoid));
  if (ids) ids[s] = static_cast<uint8_t>(looked ? r.id : r.cls == kVoteLost ? kLocateMany : kLocateClean);
  if (counts) {
    atomicAdd(counts + r.cls, 1u);
    if (looked && r.id == kLocateMany) atomicAdd(counts + 4, 1u);
  }
}

}  // namespace

hipError_t launch_vote(const VoteArgs &a, hipStream_t st) {
  if (a.nstripes <= 0) return hipSuccess;
  if (a.n < 2 || a.n > kVoteMaxShards || a.K < 1 || a.K >= a.n || !a.quorum || !a.scratch || (a.masks && (a.npat < 1 || a.npat > kLocateMany)) ||
      (a.rot_n && (a.rot_n != static_cast<uint32_t>(a.n) || a.rot0 >= a.rot_n || a.rot_step >= a.rot_n)))
    return hipErrorInvalidValue;
  return launch_kernel(&k_vote, dim3((a.nstripes + kVoteWaves - 1) / kVoteWaves), dim3(kVoteWaves * 64), st, a);
}

hipError_t launch_vote_scan(const VoteScanArgs &a, int plain_loads, int steps, hipStream_t st) {
  if (a.nstripes <= 0 || a.size == 0) return hipSuccess;
  if (a.n < 2 || a.n > kVoteMaxShards || a.size < 0 || a.size % 8 != 0 || !a.scratch || (steps != 2 && steps != 4))
    return hipErrorInvalidValue;
  const int64_t tile = vote_scan_tile_bytes(steps);
  const uint64_t ntiles = static_cast<uint64_t>((a.size + tile - 1) / tile) * static_cast<uint64_t>(a.n) * static_cast<uint64_t>(a.nstripes);
  if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
  if (steps == 2) return plain_loads ? launch_kernel(&k_vote_scan<true, 2>, grid, block, st, a) : launch_kernel(&k_vote_scan<false, 2>, grid, block, st, a);
  return plain_loads ? launch_kernel(&k_vote_scan<true, 4>, grid, block, st, a) : launch_kernel(&k_vote_scan<false, 4>, grid, block, st, a);
}

hipError_t launch_vote_finalize(const VoteScratch *scratch, int nstripes, int paranoid, int lookups, uint8_t *cls, uint8_t *ids,
                                unsigned *counts, hipStream_t st) {
  if (nstripes <= 0) return hipSuccess;
  if (!scratch || !cls || reinterpret_cast<uintptr_t>(counts) % 4 != 0) return hipErrorInvalidValue;
  return launch_kernel(&k_vote_finalize, dim3((nstripes + 255) / 256), dim3(256), st, scratch, nstripes, paranoid, lookups, cls, ids, counts);
}

}  // namespace lsec
