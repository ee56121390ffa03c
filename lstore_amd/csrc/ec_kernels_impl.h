// ec_kernels_impl.h -- gfx950 (CDNA4) erasure-coding kernels (device templates).
// Instantiated per output-row count R in ec_kernels_inst.hip (one translation unit per R, so
// the many (R, K, tile) specialisations compile in parallel); launched from ec_kernels.hip.
// See ec_kernels.h for the contract.
//
// The path is HBM-bound byte/bit arithmetic (no MFMA):
//   encode  reads K*C, writes R*C bytes per stripe
//   decode  reads K survivors, writes R = #erased shards
// Both kernels stream every input byte exactly once from HBM and write every output byte
// exactly once; all GF(2^8) work happens in VGPRs.
//
// gf8_bytewise (Reed-Solomon / matrix codes).  Multiply-by-constant c of a byte v is split
// over three bit fields of v:  c*v = c*(v & 7) ^ c*(v & 0x38) ^ c*(v & 0xC0).  Each field
// has at most 8 values, so each partial product is ONE v_perm_b32 that selects bytes out of
// an 8-byte table {c*0..c*7}, {c*0,c*8,..,c*56} or {c*0,c*64,c*128,c*192} -- four bytes of
// the word at once.  The three field extractions are shared by all R outputs of an input
// shard; per (output, input) pair a word costs 3 perms + 2 xors (one of them gfx950's
// 3-input v_bitop3), versus a 64 KiB table walk per byte on the CPU (galois.c:471-525).
//
// gf8_bitsliced (Cauchy / bitmatrix codes).  In Jerasure's packet layout the 8 bits of a
// field element live in 8 different packets, so a 32-bit lane word of each packet carries
// bit x of 32 independent elements.  Multiplying all of them by 2 is then a renaming of
// the 8 packet words plus 3 XORs (x^8 = x^4+x^3+x^2+1), and c*e = sum_{t: c_t=1} 2^t e.
// Per input shard: 7 doublings (21 xors per 8 words), then 8 xors per set coefficient bit,
// under wave-uniform branches.  Identical result to running the smart XOR schedule over
// the bitmatrix (jerasure.c:1168-1191), but every packet is read once and all
// intermediates stay in registers instead of streaming P-byte XORs through memory.
#pragma once
#include "ec_kernels.h"

#include <algorithm>
#include <type_traits>

namespace lsec {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int N> struct VecT;
template <> struct VecT<1> { typedef uint32_t type; };
template <> struct VecT<2> { typedef u32x2 type; };
template <> struct VecT<4> { typedef u32x4 type; };

constexpr int kBlock = 256;

// The coefficient image is read-only and every lane of a wave reads the same cell, so read
// it through the constant address space: uniform addresses there become s_load (SGPRs),
// leaving the VALU and the vector memory pipe to the shard bytes.
typedef const __attribute__((address_space(4))) CoefCell ConstCell;

__device__ __forceinline__ ConstCell *const_cells(const CoefCell *p) {
  return reinterpret_cast<ConstCell *>(reinterpret_cast<uintptr_t>(p));
}

// Shard addresses arrive as integers; give them the global address space explicitly so
// loads/stores are global_* (vmcnt only) rather than flat_* (vmcnt + lgkmcnt).
#define LSEC_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const LSEC_GLOBAL T *gptr(uint64_t addr) {
  return reinterpret_cast<const LSEC_GLOBAL T *>(addr);
}
template <typename T>
__device__ __forceinline__ LSEC_GLOBAL T *gptr_w(uint64_t addr) {
  return reinterpret_cast<LSEC_GLOBAL T *>(addr);
}

// Output stores.  ACC XORs the result into what the output holds: the second and later input
// groups of a stripe wider than kMaxK inputs (ApplyArgs::accumulate), launched on separate
// ACC instantiations -- a run-time branch at the stores cost the hot kernels registers (RS
// 10+4: 155 -> 268 VGPRs, occupancy 3 -> 1, 0.77 -> 0.55 of 8 TB/s).
template <bool ACC, typename V>
__device__ __forceinline__ void put_nt(uint64_t q, V v) {
  if constexpr (ACC) v ^= *gptr<V>(q);
  __builtin_nontemporal_store(v, gptr_w<V>(q));
}
template <bool ACC, typename V>
__device__ __forceinline__ void put(uint64_t q, V v) {
  if constexpr (ACC) v ^= *gptr<V>(q);
  *gptr_w<V>(q) = v;
}

// ------------------------------------------------------------------ bytewise
// 3-input XOR in one VALU op (gfx950 v_bitop3_b32, truth table 0x96)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// acc ^= c * word (4 bytes in parallel): 3 byte-permutes over the cell's tables + 2 xors
__device__ __forceinline__ uint32_t gf_mul_acc(uint32_t acc, uint32_t ia, uint32_t ib, uint32_t ic,
                                               const uint32_t (&t)[6]) {
  return xor3(acc, __builtin_amdgcn_perm(t[1], t[0], ia), __builtin_amdgcn_perm(t[3], t[2], ib)) ^
         __builtin_amdgcn_perm(t[5], t[4], ic);
}

// Spread the grid so that each XCD (blocks b, b+8, b+16, ... are dealt to one XCD) gets a
// contiguous run of tiles instead of every 8th tile: measured +2-3% HBM throughput on this
// streaming pattern (tools/kprobe.hip).  Bijective for any grid size; placement is only a
// speed hint, correctness never depends on it.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nb) {
  const uint32_t per = nb >> 3, rem = nb & 7, xcd = b & 7;
  return xcd * per + min(xcd, rem) + (b >> 3);
}

// Every tile t < ntiles to body(t) exactly once, body's t uniform over the workgroup.
//   q null: the grid strides over the tiles from its XCD-contiguous start (one tile per block
//   when the grid is the tile count): each XCD its static eighth.
//   q a tile queue slot (ec_kernels.h, "Work-sharing tiles"): each eighth's first `pre` tiles go
//   one per block to blocks 0 .. 8*pre-1 (block b on XCD b % 8, as the static form), and the
//   blocks after those share the rest: each takes G consecutive tiles at a time (a grab) from its
//   own XCD's remainder, then from the other eighths'.  pre = 0: all tiles are shared.  Thread 0
//   issues the atomic for the next grab as soon as it has the current one, so the counter's round
//   trip hides behind the grab's tiles; it posts the grab in one of two LDS words (never one a wave
//   has yet to read: that wave has not passed the barrier after its read), and readfirstlane keeps
//   the loop uniform.  One call site of body for every form: the kernels' code is not repeated.
//   phase > 0 (ApplyArgs::tile_phase): XCD / eighth x visits its tiles starting x * phase tiles in,
//   wrapping around inside its own range (a bijection; the static form only when the grid is the
//   tile count).
template <int G = 1, typename Body>
__device__ __forceinline__ void for_tiles(uint32_t ntiles, unsigned *q, uint32_t pre, Body &&body, uint32_t phase = 0) {
  __shared__ uint32_t next[2];
  const uint32_t per = (ntiles + 7) >> 3, xcd = blockIdx.x & 7;
  // the phase's map of a queue-form tile index: eighth e = t / per, rotated inside its own range
  const auto rot = [&](uint32_t t) -> uint32_t {
    const uint32_t e = t / per, base = e * per, size = min(per, ntiles - base);
    return base + ((t - base) + (e * phase) % size) % size;
  };
  const bool sharing = q != nullptr && blockIdx.x >= 8 * pre;  // block-uniform
  const uint32_t rest = per - pre, grabs = (rest + G - 1) / G;  // each eighth's shared tiles, grabs
  uint32_t k = 0, pend = 0, it = 0;  // thread 0: eighths done, the counter value in flight
  const auto take = [&]() -> uint32_t {  // thread 0: first tile of the grab `pend` names, or ntiles
    for (;;) {
      const uint32_t t = ((xcd + k) & 7) * per + pre + pend * G;
      if (pend < grabs && t < ntiles) return t;
      if (++k == 8) return ntiles;
      pend = atomicAdd(q + kTileQueueLine * ((xcd + k) & 7), 1u);
    }
  };
  uint32_t t, end, step = 1;
  if (q == nullptr) {
    t = xcd_remap(blockIdx.x, gridDim.x);
    if (phase && gridDim.x == ntiles) {  // one tile per block: rotate inside this XCD's contiguous run
      const uint32_t nb = gridDim.x, p8 = nb >> 3, rem = nb & 7;
      const uint32_t size = p8 + (xcd < rem ? 1u : 0u), start = xcd * p8 + min(xcd, rem);
      t = start + ((blockIdx.x >> 3) + (xcd * phase) % size) % size;
    }
    end = ntiles;
    step = gridDim.x;
  } else if (!sharing) {  // the static prefix: one tile
    t = xcd * per + (blockIdx.x >> 3);
    end = min(ntiles, t + 1);
  } else {
    t = end = 0;  // the first grab comes below
  }
  for (;;) {
    if (t >= end) {
      if (!sharing) break;
      if (threadIdx.x == 0) {
        if (it == 0) pend = atomicAdd(q + kTileQueueLine * xcd, 1u);
        next[it & 1] = take();
      }
      __syncthreads();
      t = __builtin_amdgcn_readfirstlane(next[it & 1]);
      ++it;
      if (t >= ntiles) break;
      end = min(min(ntiles, (t / per + 1) * per), t + G);  // a grab stays inside its eighth
      if (threadIdx.x == 0) pend = atomicAdd(q + kTileQueueLine * ((xcd + k) & 7), 1u);  // the next grab
    }
    body(q != nullptr && phase ? rot(t) : t);
    t += step;
  }
  // the launch's last sharing block leaves the slot zeroed for its next taker
  if (sharing && threadIdx.x == 0 && atomicAdd(q + kTileQueueLine * 8, 1u) == gridDim.x - 8 * pre - 1)
    for (int e = 0; e <= 8; ++e) atomicExch(q + kTileQueueLine * e, 0u);
}

// A tile-loop kernel over ApplyArgs, PatternArgs, CheckArgs, LocateArgs or a rotated form, launched with a
// work-sharing tile queue slot and its persistent grid when tile sharing is on (ec_kernels.h),
// else on `grid` blocks over static eighths.
template <typename Kern, typename Args>
hipError_t launch_tiled(Kern *k, int grid, hipStream_t st, Args a) {
  if constexpr (std::is_same<Args, ApplyArgs>::value) a.stamps = launch_stamps(&a.nstamps);
  // `grid` is the tile count here: tiles per stripe = grid / nstripes
  a.tile_phase = tile_phase_on() && a.nstripes > 0 && grid % a.nstripes == 0 ? static_cast<uint32_t>(grid / a.nstripes / 8) : 0;
  unsigned *slot = tile_queue_slot(st, static_cast<uint64_t>(grid));
  a.tiles = nullptr;
  a.tiles_pre = 0;
  if (slot) {
    const int pg = persistent_grid(reinterpret_cast<const void *>(k), grid, st);
    if (pg > 0) {
      // `grid` is the tile count here (one tile per block in the static form)
      a.tiles = slot;
      a.tiles_pre = tiles_prefix(static_cast<uint32_t>(grid));
      grid = static_cast<int>(8 * a.tiles_pre) + pg;
    }
  }
  const hipError_t e = launch_kernel_shm(k, dim3(grid), dim3(kBlock), occupancy_lds_bytes(a.size), st, a);
  tile_queue_release(st, slot);
  return e;
}

// ------------------------------------------------------------------ adler32 partial sums
constexpr uint32_t kAdlerMod = 65521;

template <typename V>
__device__ __forceinline__ void adler_add(V v, uint64_t len_minus_pos, uint64_t &a_sum, uint64_t &b_sum) {
  // S = sum of the 16 bytes, U = sum t*b_t (t = 0..15) via packed byte dot products
  constexpr int N = sizeof(V) / 4;
  uint32_t S = 0, U = 0;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const uint32_t x = reinterpret_cast<const uint32_t *>(&v)[e];
    S = __builtin_amdgcn_udot4(x, 0x01010101u, S, false);
    U = __builtin_amdgcn_udot4(x, 0x03020100u + 0x04040404u * e, U, false);
  }
  a_sum += S;
  b_sum += len_minus_pos * S - U;   // sum_t (L - p - t) b_t, every term >= 0
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kBlock / 64; ++w) t += lds[w];
  __syncthreads();
  return t;
}

// Per-lane work unit of the bytewise kernel: VW dwords (16 B for VW = 4, 8 B for VW = 2) per
// step, IT steps kBlock*4*VW bytes apart; a tile is kBlock*4*VW*IT bytes of every shard.
template <int IT, int VW>
struct BwTile {
  static constexpr int kStep = kBlock * 4 * VW;
  static constexpr int kBytes = kStep * IT;
};

// One lane unit of a ragged last tile, at byte o of a chunk of C bytes.  C is a multiple of 8,
// so a 16-byte unit may be half full: its two valid dwords are read (the rest is 0) or stored;
// a unit wholly past C reads as 0 and is not stored.
template <int VW>
__device__ __forceinline__ typename VecT<VW>::type load_ragged(uint64_t p, int64_t o, int64_t C) {
  typename VecT<VW>::type v = 0u;
  if (o + 4 * VW <= C) {
    v = *gptr<typename VecT<VW>::type>(p + o);
  } else if (o < C) {
    const u32x2 h = *gptr<u32x2>(p + o);
    v[0] = h.x;
    v[1] = h.y;
  }
  return v;
}
template <bool ACC, int VW>
__device__ __forceinline__ void store_ragged(uint64_t q, int64_t o, int64_t C, typename VecT<VW>::type v) {
  if (o + 4 * VW <= C) {
    put<ACC, typename VecT<VW>::type>(q + o, v);
  } else if (o < C) {
    u32x2 h;
    h.x = v[0];
    h.y = v[1];
    put<ACC, u32x2>(q + o, h);
  }
}

template <int R, int IT, int VW>
__device__ __forceinline__ void bw_accumulate(typename VecT<VW>::type (&acc)[IT][R],
                                              const typename VecT<VW>::type (&v)[IT], ConstCell *cells, int K,
                                              int j) {
  typedef typename VecT<VW>::type V;
  V ia[IT], ib[IT], ic[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    ia[it] = v[it] & 0x07070707u;
    ib[it] = (v[it] >> 3) & 0x07070707u;
    ic[it] = (v[it] >> 6) & 0x03030303u;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ConstCell *cell = cells + r * K + j;  // wave-uniform -> scalar loads
    const uint32_t c = cell->coef;
    if (c == 0) continue;
    if (c == 1) {
#pragma unroll
      for (int it = 0; it < IT; ++it) acc[it][r] ^= v[it];
      continue;
    }
    const uint32_t t[6] = {cell->ta_lo, cell->ta_hi, cell->tb_lo, cell->tb_hi, cell->tc_lo, cell->tc_hi};
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[it][r][e] = gf_mul_acc(acc[it][r][e], ia[it][e], ib[it][e], ic[it][e], t);
  }
}

// Branch-free variant: every coefficient takes the 3-perm path (the tables of 0 and 1 give 0
// and the identity), so there are no per-cell branches (whose merges cost register copies
// and serialise the cell loads), and inputs are taken two at a time so three 3-input XORs
// fold six partial products.  The c*(v>>6) table has 4 entries: one dword, so that perm
// takes an inline 0 as its high half and needs no VGPR copy of the table.
template <int IT, int VW>
__device__ __forceinline__ void bw_fields(const typename VecT<VW>::type (&v)[IT], typename VecT<VW>::type (&fa)[IT],
                                          typename VecT<VW>::type (&fb)[IT], typename VecT<VW>::type (&fc)[IT]) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    fa[it] = v[it] & 0x07070707u;
    fb[it] = (v[it] >> 3) & 0x07070707u;
    fc[it] = (v[it] >> 6) & 0x03030303u;
  }
}

//
// X0: output row 0 is the plain XOR of the inputs (every coefficient 1 -- P0 of RS / Cauchy
// encodes, and decode rows that re-encode P0), flagged by the host in the row's first cell.
// That row then costs one 3-input XOR per input pair instead of 6 perms + 3 XORs, which
// is what the VALU-bound wide codes pay for it otherwise (RS 20+6: 20 of 120 cells).
template <int R, int IT, int VW, bool TWO, bool X0 = false>
__device__ __forceinline__ void bw_accumulate_bf(typename VecT<VW>::type (&acc)[IT][R],
                                                 const typename VecT<VW>::type (&va)[IT],
                                                 const typename VecT<VW>::type (&vb)[IT], ConstCell *cells, int K, int j) {
  typedef typename VecT<VW>::type V;
  V ia[IT], ib[IT], ic[IT], ja[IT], jb[IT], jc[IT];
  bw_fields<IT, VW>(va, ia, ib, ic);
  if constexpr (TWO) bw_fields<IT, VW>(vb, ja, jb, jc);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if constexpr (X0) {
      if (r == 0) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[it][0][e] = TWO ? xor3(acc[it][0][e], va[it][e], vb[it][e]) : acc[it][0][e] ^ va[it][e];
        continue;
      }
    }
    ConstCell *ca = cells + r * K + j;  // wave-uniform -> scalar loads
    const uint32_t a0 = ca->ta_lo, a1 = ca->ta_hi, a2 = ca->tb_lo, a3 = ca->tb_hi, a4 = ca->tc_lo;
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    if constexpr (TWO) {
      ConstCell *cb = ca + 1;
      b0 = cb->ta_lo, b1 = cb->ta_hi, b2 = cb->tb_lo, b3 = cb->tb_hi, b4 = cb->tc_lo;
    }
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        uint32_t x = acc[it][r][e];
        const uint32_t p1 = __builtin_amdgcn_perm(a1, a0, ia[it][e]);
        const uint32_t p2 = __builtin_amdgcn_perm(a3, a2, ib[it][e]);
        const uint32_t p3 = __builtin_amdgcn_perm(0u, a4, ic[it][e]);
        if constexpr (TWO) {
          const uint32_t q1 = __builtin_amdgcn_perm(b1, b0, ja[it][e]);
          const uint32_t q2 = __builtin_amdgcn_perm(b3, b2, jb[it][e]);
          const uint32_t q3 = __builtin_amdgcn_perm(0u, b4, jc[it][e]);
          x = xor3(x, p1, p2);
          x = xor3(x, p3, q1);
          x = xor3(x, q2, q3);
        } else {
          x = xor3(x, p1, p2) ^ p3;
        }
        acc[it][r][e] = x;
      }
  }
}

// one input (BF = false: branchy per-cell path; true: branch-free)
template <int R, int IT, int VW, bool BF, bool X0>
__device__ __forceinline__ void bw_acc1(typename VecT<VW>::type (&acc)[IT][R], const typename VecT<VW>::type (&v)[IT],
                                       ConstCell *cells, int K, int j) {
  if constexpr (BF) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v, v, cells, K, j);
  else bw_accumulate<R, IT, VW>(acc, v, cells, K, j);
}

__device__ __forceinline__ void magic_commit(unsigned long long *acc, uint32_t s, uint64_t as, uint64_t bs, uint32_t *red) {
  const uint32_t am = block_sum(static_cast<uint32_t>(as % kAdlerMod), red);
  const uint32_t bm = block_sum(static_cast<uint32_t>(bs % kAdlerMod), red);
  if (threadIdx.x == 0) {
    atomicAdd(acc + 2 * s, static_cast<unsigned long long>(am));
    atomicAdd(acc + 2 * s + 1, static_cast<unsigned long long>(bm));
  }
}

// Per-lane partial sums of the fused stripe magic.  A lane's byte at stripe position
//   p = sh*C + off + x*X + 4d + t
// (shard sh, the lane's first byte `off`, its x-th word group X bytes further on -- the
// iteration of the bytewise kernel, the packet of the bit-sliced one -- dword d, byte t)
// contributes (L - p)*b to adler32's B, so over the lane's bytes
//   sum (L - p) b = L*A - (C*JS + off*A + X*XS + W)
// with A = sum b, JS = sum sh*b, XS = sum x*b, W = sum (4d+t)*b: 32-bit v_dot4 chains,
// no 64-bit arithmetic until the lane's tile is done.
struct MagicLane {
  uint32_t a = 0, js = 0, xs = 0, w = 0;
};

__device__ __forceinline__ void ml_commit(const MagicLane &m, unsigned long long *acc, uint32_t s, int nsh, uint64_t C,
                                          uint64_t off, uint64_t X, uint32_t *red) {
  const uint64_t A = m.a;
  const uint64_t B = static_cast<uint64_t>(nsh) * C * A - (C * m.js + off * A + X * m.xs + m.w);
  magic_commit(acc, s, A, B, red);
}

// one shard's words of a lane: e[x] = VW dwords, x = 0..NX-1
template <int NX, int VW>
__device__ __forceinline__ void ml_add(MagicLane &m, const typename VecT<VW>::type (&e)[NX], uint32_t sh) {
  uint32_t sum = 0;
#pragma unroll
  for (int x = 0; x < NX; ++x)
#pragma unroll
    for (int d = 0; d < VW; ++d) {
      const uint32_t v = reinterpret_cast<const uint32_t *>(&e[x])[d];
      sum = __builtin_amdgcn_udot4(v, 0x01010101u, sum, false);
      if (NX > 1) m.xs = __builtin_amdgcn_udot4(v, 0x01010101u * x, m.xs, false);
      m.w = __builtin_amdgcn_udot4(v, 0x03020100u + 0x04040404u * d, m.w, false);
    }
  m.a += sum;
  m.js += sh * sum;
}

// The same sums taken away: the bytes a write replaces (the masked update's magic, below).
template <int NX, int VW>
__device__ __forceinline__ void ml_sub(MagicLane &m, const typename VecT<VW>::type (&e)[NX], uint32_t sh) {
  MagicLane t;
  ml_add<NX, VW>(t, e, sh);
  m.a -= t.a;
  m.js -= t.js;
  m.xs -= t.xs;
  m.w -= t.w;
}

// A tile's change of a stripe magic that exists already (lsec_update_magic_dev_masked): the lane has added
// the bytes the write leaves (ml_add) and taken away the ones it replaces (ml_sub), in wrapping 32-bit
// arithmetic, so its four sums read back as signed are new minus old.  Their true magnitudes are far
// below 2^31: at most 72 shards x 128 bytes of a lane x 255, times a shard index of at most 71.  The
// signed tile sums go into [0, M) before the block sum, so the per-stripe accumulators only ever grow.
__device__ __forceinline__ void ml_commit_delta(const MagicLane &m, unsigned long long *acc, uint32_t s, int nsh, int64_t C,
                                                int64_t off, int64_t X, uint32_t *red) {
  const int64_t A = static_cast<int32_t>(m.a);
  const int64_t B = nsh * C * A - (C * static_cast<int32_t>(m.js) + off * A + X * static_cast<int32_t>(m.xs) +
                                   static_cast<int32_t>(m.w));
  int64_t am = A % static_cast<int64_t>(kAdlerMod), bm = B % static_cast<int64_t>(kAdlerMod);
  if (am < 0) am += kAdlerMod;
  if (bm < 0) bm += kAdlerMod;
  magic_commit(acc, s, static_cast<uint64_t>(am), static_cast<uint64_t>(bm), red);
}

// fused stripe magic (bytewise kernel): lane words are the IT steps kStep bytes apart
template <int R, int IT, int VW>
__device__ __forceinline__ void bw_magic(MagicLane &ml, const typename VecT<VW>::type (*v)[IT], int nv, int j0) {
  for (int jj = 0; jj < nv; ++jj) ml_add<IT, VW>(ml, v[jj], static_cast<uint32_t>(j0 + jj));
}

// (NEG: taken away, the stored rows an update is about to replace)
template <int R, int IT, int VW, bool NEG = false>
__device__ __forceinline__ void bw_magic_out(MagicLane &ml, int K, const typename VecT<VW>::type (&acc)[IT][R]) {
  typedef typename VecT<VW>::type V;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    V o[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) o[it] = acc[it][r];
    if constexpr (NEG) ml_sub<IT, VW>(ml, o, static_cast<uint32_t>(K + r));
    else ml_add<IT, VW>(ml, o, static_cast<uint32_t>(K + r));
  }
}

// (on a lambda: inlined before anything else is optimised, as a __forceinline__ function is)
#define LSEC_INLINE __attribute__((always_inline))

// The input stage of a full bytewise tile: acc[it][r] ^= cells[r][j] * (input j's IT lane units),
// j = 0 .. K-1.  addr(j) is the address of the lane's first unit of input j.  KC > 0: K fixed at
// compile time, all K*IT loads in flight before any arithmetic; else four inputs at a time.
// extra() issues the caller's own loads (the check's stored parity) where they overlap the
// inputs': behind the data loads with K fixed, ahead of the first group otherwise.
// BF, X0 as bw_accumulate_bf.  The patterned, check and locate kernels call it; the encode's
// bytewise_tiles keeps the same stage written out, with the fused stripe magic after each group.
template <int R, int KC, int IT, int VW, bool BF, bool X0, typename Addr, typename Extra>
__device__ __forceinline__ void bw_inputs(typename VecT<VW>::type (&acc)[IT][R], ConstCell *cells, int K, Addr &&addr,
                                          Extra &&extra) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  if constexpr (KC > 0) {
    V v[KC][IT];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const uint64_t p = addr(j);
#pragma unroll
      for (int it = 0; it < IT; ++it) v[j][it] = __builtin_nontemporal_load(gptr<V>(p + it * kStep));
    }
    extra();
    if constexpr (BF) {
#pragma unroll
      for (int j = 0; j + 1 < KC; j += 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[j], v[j + 1], cells, K, j);
      if constexpr (KC % 2) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[KC - 1], v[KC - 1], cells, K, KC - 1);
    } else {
#pragma unroll
      for (int j = 0; j < KC; ++j) bw_accumulate<R, IT, VW>(acc, v[j], cells, K, j);
    }
  } else {
    extra();
    for (int j0 = 0; j0 < K; j0 += 4) {
      V v[4][IT];
      const int nj = min(4, K - j0);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (jj < nj) {
          const uint64_t p = addr(j0 + jj);
#pragma unroll
          for (int it = 0; it < IT; ++it) v[jj][it] = __builtin_nontemporal_load(gptr<V>(p + it * kStep));
        }
      }
      if constexpr (BF) {
        if (nj >= 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[0], v[1], cells, K, j0);
        if (nj == 4) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[2], v[3], cells, K, j0 + 2);
        if (nj == 1 || nj == 3) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[nj - 1], v[nj - 1], cells, K, j0 + nj - 1);
      } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          if (jj < nj) bw_accumulate<R, IT, VW>(acc, v[jj], cells, K, j0 + jj);
      }
    }
  }
}

// extra() of a caller with no loads of its own
struct NoLoads {
  __device__ __forceinline__ void operator()() const {}
};

// BF = branch-free coefficient path (bw_accumulate_bf).
// MG = also accumulate the stripe magic of inputs + outputs (encode + je_cksum_calc fused).
// X0 = row 0 is a plain XOR (see bw_accumulate_bf).
template <int R, int KC, int IT, bool BF, int VW, bool MG, bool X0, bool ACC>
__device__ __forceinline__ void bytewise_tiles(const ApplyArgs &a) {
  typedef typename VecT<VW>::type V;
  __shared__ uint32_t red[MG ? kBlock / 64 : 1];
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = KC ? KC : a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  // grabs of about 8 KiB per shard (the single-erasure decode's 2 KiB tiles go 4 at a time)
  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform

    V acc[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[it][r] = 0u;
    MagicLane ml;  // fused magic partial sums (MG only)

    if (full) {
      // bw_inputs, load_ragged and store_ragged written out: called from here they moved the register
      // tables of this kernel's forms, 18 of them to a lower occupancy (the branchy forms of two or more
      // rows: <4, 4, 1, false, 2> 48 -> 86 VGPRs; profiles/tile_bodies_refactor_resources.txt)
      if constexpr (KC > 0) {
        V v[KC][IT];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          const uint64_t p = a.in[j].base + s * a.in[j].stride + off0;
#pragma unroll
          for (int it = 0; it < IT; ++it) v[j][it] = __builtin_nontemporal_load(gptr<V>(p + it * kStep));
        }
        if constexpr (BF) {
#pragma unroll
          for (int j = 0; j + 1 < KC; j += 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[j], v[j + 1], cells, K, j);
          if constexpr (KC % 2) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[KC - 1], v[KC - 1], cells, K, KC - 1);
        } else {
#pragma unroll
          for (int j = 0; j < KC; ++j) bw_accumulate<R, IT, VW>(acc, v[j], cells, K, j);
        }
        if constexpr (MG) bw_magic<R, IT, VW>(ml, v, KC, 0);
      } else {
        for (int j0 = 0; j0 < K; j0 += 4) {
          V v[4][IT];
          const int nj = min(4, K - j0);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            if (jj < nj) {
              const uint64_t p = a.in[j0 + jj].base + s * a.in[j0 + jj].stride + off0;
#pragma unroll
              for (int it = 0; it < IT; ++it) v[jj][it] = __builtin_nontemporal_load(gptr<V>(p + it * kStep));
            }
          }
          if constexpr (BF) {
            if (nj >= 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[0], v[1], cells, K, j0);
            if (nj == 4) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[2], v[3], cells, K, j0 + 2);
            if (nj == 1 || nj == 3) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[nj - 1], v[nj - 1], cells, K, j0 + nj - 1);
          } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
              if (jj < nj) bw_accumulate<R, IT, VW>(acc, v[jj], cells, K, j0 + jj);
          }
          if constexpr (MG) bw_magic<R, IT, VW>(ml, v, nj, j0);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.out[r].base + s * a.out[r].stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) put_nt<ACC, V>(q + it * kStep, acc[it][r]);
      }
    } else {
      for (int j = 0; j < K; ++j) {
        const uint64_t p = a.in[j].base + s * a.in[j].stride;
        V v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {  // (load_ragged, written out)
          const int64_t o = off0 + it * kStep;
          v[it] = 0u;
          if (o + kLane <= C) {
            v[it] = *gptr<V>(p + o);
          } else if (o < C) {
            const u32x2 h = *gptr<u32x2>(p + o);
            v[it][0] = h.x;
            v[it][1] = h.y;
          }
        }
        bw_acc1<R, IT, VW, BF, X0>(acc, v, cells, K, j);
        if constexpr (MG) {
          const V(*vv)[IT] = &v;
          bw_magic<R, IT, VW>(ml, vv, 1, j);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.out[r].base + s * a.out[r].stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) {  // (store_ragged, written out)
          const int64_t o = off0 + it * kStep;
          if (o + kLane <= C) {
            put<ACC, V>(q + o, acc[it][r]);
          } else if (o < C) {
            u32x2 h;
            h.x = acc[it][r][0];
            h.y = acc[it][r][1];
            put<ACC, u32x2>(q + o, h);
          }
        }
      }
    }
    if constexpr (MG) {
      bw_magic_out<R, IT, VW>(ml, K, acc);
      ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(a.size), static_cast<uint64_t>(off0), kStep, red);
    }
  }, a.tile_phase);
}

// The XOR-row flag (CoefCell::pad bit 0 of the launch's first cell) picks one of two whole
// instantiations once per wave: a uniform branch outside the tile loop, no merges inside it.
// Only codes with K*R >= 40 cells take the dual form: narrow codes are HBM-bound, and the
// second path would only raise the kernel's register allocation (RS 6+3: 56 -> 108 VGPRs).
constexpr bool bw_dual_loops(int R, int KC, bool BF) { return BF && R >= 2 && (KC == 0 || KC * R >= 40); }

template <int R, int KC, int IT, bool BF, int VW, bool MG = false, bool ACC = false>
__global__ __launch_bounds__(kBlock) void k_gf8_bytewise(ApplyArgs a) {
  if constexpr (bw_dual_loops(R, KC, BF)) {
    if (const_cells(a.cells)->pad & kCellXorRow) {
      bytewise_tiles<R, KC, IT, BF, VW, MG, true, ACC>(a);
      return;
    }
  }
  bytewise_tiles<R, KC, IT, BF, VW, MG, false, ACC>(a);
  if (a.stamps) {  // measurement only: when this workgroup finished (s_memrealtime, 100 MHz)
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < a.nstamps) a.stamps[blockIdx.x] = __builtin_amdgcn_s_memrealtime();
  }
}

// ------------------------------------------------------------------ bitsliced
// e <- 2*e on the 8 bit slices of GF(2^8) (word x of e = bit x of the lane's elements): a
// renaming of the slices, the top one XORed into the taps of x^8 = x^4+x^3+x^2+1.
template <typename V>
__device__ __forceinline__ void gf8_double_sliced(V (&e)[8]) {
  const V top = e[7];
  e[7] = e[6];
  e[6] = e[5];
  e[5] = e[4];
  e[4] = e[3] ^ top;
  e[3] = e[2] ^ top;
  e[2] = e[1] ^ top;
  e[1] = e[0];
  e[0] = top;
}

// acc[r] ^= c[r] * e for the rows r = R0 .. R-1, c*e = sum_{t: c_t = 1} 2^t e; e is used up.
// cm is the OR of those rows' coefficients: no doublings past its highest bit (e.g. the XOR
// rows of a single-erasure decode stop after bit 0).  The branches are wave-uniform.
template <int R0, int R, typename V>
__device__ __forceinline__ void gf8_sliced_mul_acc(V (&acc)[R][8], V (&e)[8], const uint32_t (&c)[R], uint32_t cm) {
#pragma unroll
  for (int b = 0; b < 8; ++b) {
#pragma unroll
    for (int r = R0; r < R; ++r)
      if ((c[r] >> b) & 1u) {
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[r][x] ^= e[x];
      }
    if ((cm >> (b + 1)) == 0) break;
    if (b < 7) gf8_double_sliced(e);
  }
}

// A lane owns DW consecutive dwords of packet-column space in one super-packet and reads
// the same columns of all 8 packets of every input shard.  MG: also the stripe magic of the
// inputs and outputs (encode + je_cksum_calc in one pass, as the bytewise kernel does).
template <int R, int KC, int DW, bool MG = false, bool ACC = false>
__global__ __launch_bounds__(kBlock) void k_gf8_bitsliced(ApplyArgs a) {
  typedef typename VecT<DW>::type V;
  __shared__ uint32_t red[MG ? kBlock / 64 : 1];
  const int K = KC ? KC : a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    // lanes past the end occur only in a ragged last tile (P % 16 == 0 keeps a lane's DW
    // dwords inside one packet); with MG they still join the block's magic reduction
    const bool valid = colb < col_bytes;
    if (!MG && !valid) return;
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);
    MagicLane ml;

    V acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[r][x] = 0u;

    for (int j = 0; j < K && valid; ++j) {
      const uint64_t p = a.in[j].base + s * a.in[j].stride + off;
      V e[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) e[x] = __builtin_nontemporal_load(gptr<V>(p + x * P));
      if constexpr (MG) ml_add<8, DW>(ml, e, static_cast<uint32_t>(j));
      uint32_t c[R];
      uint32_t cm = 0;  // bits used by any output: no doublings past the highest one
#pragma unroll
      for (int r = 0; r < R; ++r) {
        c[r] = cells[r * K + j].coef;
        cm |= c[r];
      }
      gf8_sliced_mul_acc<0>(acc, e, c, cm);
    }
    if (valid) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.out[r].base + s * a.out[r].stride + off;
#pragma unroll
        for (int x = 0; x < 8; ++x) put_nt<ACC, V>(q + x * P, acc[r][x]);
        if constexpr (MG) ml_add<8, DW>(ml, acc[r], static_cast<uint32_t>(K + r));
      }
    }
    if constexpr (MG) ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(a.size), static_cast<uint64_t>(off), P, red);
  }, a.tile_phase);
}

// ------------------------------------------------------------------ generic bitmatrix
// Bitmatrix codes that are not GF(2^8)-linear per byte (liberation / blaum_roth / liber8tion,
// vendor/jerasure/src/liberation.c): packet l of output r = XOR of the input packets (j, x)
// whose bit B[r*w+l][j*w+x] is set (jerasure_bitmatrix_dotprod, jerasure.c:317-362).  A lane
// owns one dword column of a super-packet and applies the bitmatrix under wave-uniform
// branches (the row masks live in the constant address space).
typedef const __attribute__((address_space(4))) uint32_t ConstU32;

template <int R, int W>
__global__ __launch_bounds__(kBlock) void k_bitmatrix(ApplyArgs a) {
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / W);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstU32 *masks = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  for (uint32_t t = xcd_remap(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {
    const uint32_t s = t / tiles_per_stripe;
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * 4;
    if (colb >= col_bytes) continue;
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * W * P + (colb - sp * P);
    uint32_t acc[R][W];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int l = 0; l < W; ++l) acc[r][l] = 0u;
    for (int j = 0; j < K; ++j) {
      const uint64_t p = a.in[j].base + s * a.in[j].stride + off;
      uint32_t e[W];
#pragma unroll
      for (int x = 0; x < W; ++x) e[x] = __builtin_nontemporal_load(gptr<uint32_t>(p + x * P));
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < W; ++l) {
          const uint32_t mask = masks[(r * W + l) * K + j];
          uint32_t v = 0;
#pragma unroll
          for (int x = 0; x < W; ++x)
            if ((mask >> x) & 1u) v ^= e[x];
          acc[r][l] ^= v;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t q = a.out[r].base + s * a.out[r].stride + off;
#pragma unroll
      for (int l = 0; l < W; ++l) put_nt<false, uint32_t>(q + l * P, acc[r][l]);
    }
  }
}

// ------------------------------------------------------------------ bitmatrix, any w
// Word sizes outside LSEC_BITMATRIX_W: a liberation plan with k > 31 gets the next prime w >= k
// (37, 41, ..; erasure_tools.c:756-757), blaum_roth w = p - 1.  Per-w register tiles do not
// scale there (acc[2][w] + e[w] registers), so a block stages its inputs in LDS instead.  A block
// owns 1 KiB of packet-column space (4 B per lane); for each input it stages the words of up to
// 64 packets of that column in LDS, and each of up to 64 output packets (registers) XORs the
// staged words its mask selects: a loop over the mask's set bits (wave-uniform scalar mask
// words), one LDS read per bit -- liberation rows have one or two bits per input block.  Output
// packets beyond 64 take another pass over the inputs (w <= 64: one pass).
template <int R>
__global__ __launch_bounds__(kBlock) void k_bitmatrix_any(ApplyArgs a) {
  constexpr int kChunk = 64;
  __shared__ uint32_t stage[kChunk][kBlock];  // 64 KiB
  const int K = a.K, W = a.w, NW = mask_words(a.w);
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / W);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstU32 *masks = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  for (uint32_t t = xcd_remap(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {  // block-uniform
    const uint32_t s = t / tiles_per_stripe;
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * 4;
    const bool valid = colb < col_bytes;  // lanes past the end still join the barriers
    const uint32_t sp = valid ? colb / P : 0;
    const int64_t off = static_cast<int64_t>(sp) * W * P + (colb - sp * P);
    for (int l0 = 0; l0 < W; l0 += kChunk) {
      const int nl = min(kChunk, W - l0);
      uint32_t acc[R][kChunk];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < kChunk; ++l) acc[r][l] = 0u;
      for (int j = 0; j < K; ++j) {
        const uint64_t p = a.in[j].base + s * a.in[j].stride + off;
        for (int x0 = 0; x0 < W; x0 += kChunk) {
          const int nx = min(kChunk, W - x0);
          __syncthreads();  // the previous chunk's readers are done
          for (int x = 0; x < nx; ++x)
            stage[x][threadIdx.x] = valid ? __builtin_nontemporal_load(gptr<uint32_t>(p + static_cast<uint64_t>(x0 + x) * P)) : 0u;
          __syncthreads();
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int l = 0; l < kChunk; ++l) {
              if (l >= nl) continue;  // uniform; `continue` keeps the loop fully unrolled (acc in VGPRs)
              const uint32_t mi = static_cast<uint32_t>(((r * W + l0 + l) * K + j) * NW + (x0 >> 5));
              uint64_t m = masks[mi];
              if (nx > 32) m |= static_cast<uint64_t>(masks[mi + 1]) << 32;
              uint32_t v = 0;
              while (m) {
                v ^= stage[__builtin_ctzll(m)][threadIdx.x];
                m &= m - 1;
              }
              acc[r][l] ^= v;
            }
        }
      }
      if (valid) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint64_t q = a.out[r].base + s * a.out[r].stride + off;
#pragma unroll
          for (int l = 0; l < kChunk; ++l) {
            if (l >= nl) continue;
            if (a.accumulate) put_nt<true, uint32_t>(q + static_cast<uint64_t>(l0 + l) * P, acc[r][l]);
            else put_nt<false, uint32_t>(q + static_cast<uint64_t>(l0 + l) * P, acc[r][l]);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------ wordwise GF(2^16) / GF(2^32)
// Reed-Solomon at w = 16 / 32 (jerasure_matrix_dotprod -> galois_w16/w32_region_multiply,
// galois.c:527-604, :730-810): element t of a shard is the little-endian uint16 / uint32 at
// byte 2t / 4t.  c*v = XOR_{b: v_b = 1} (c * x^b), so with the W products P_b = c*x^b of a
// cell in SGPRs (image [(r*K + j)*W + b], replicated into both halves of the dword for
// W = 16), each input dword yields W bit masks (bit b of each element smeared over the
// element: v_pk_lshlrev_b16 + v_pk_ashrrev_i16 for two uint16 elements, v_bfe_i32 for one
// uint32) shared by all R outputs, and each (output, input, bit) costs one v_bitop3_b32
// (acc ^ (mask & P_b), truth table 0x78).  VALU-bound by design at W ops per dword per
// (output, input) pair; these word sizes are off the headline configs.
typedef short s16x2 __attribute__((ext_vector_type(2)));

template <int W>
__device__ __forceinline__ uint32_t bit_smear(uint32_t x, int b) {
  if constexpr (W == 32) {
    return static_cast<uint32_t>(static_cast<int32_t>(x << (31 - b)) >> 31);
  } else {
    const s16x2 v = __builtin_bit_cast(s16x2, x);
    const s16x2 m = (v << static_cast<short>(15 - b)) >> static_cast<short>(15);
    return __builtin_bit_cast(uint32_t, m);
  }
}

template <int R, int W, bool ACC = false>
__global__ __launch_bounds__(kBlock) void k_gfw_wordwise(ApplyArgs a) {
  constexpr int VW = W == 16 ? 4 : 2;
  typedef typename VecT<VW>::type V;
  constexpr int kLane = 4 * VW;
  constexpr int kTile = kBlock * kLane;
  constexpr uint32_t kOne = W == 16 ? 0x00010001u : 1u;
  const int K = a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstU32 *prod = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  for (uint32_t t = xcd_remap(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {
    const uint32_t s = t / tiles_per_stripe;
    const int64_t off = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    if (off >= C) continue;
    const bool whole = off + kLane <= C;  // C % 8 == 0: otherwise exactly 8 bytes remain
    V acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0u;
    for (int j = 0; j < K; ++j) {
      const uint64_t p = a.in[j].base + s * a.in[j].stride + off;
      V v = 0u;
      if (whole) {
        v = __builtin_nontemporal_load(gptr<V>(p));
      } else {
        const u32x2 h = *gptr<u32x2>(p);
        v[0] = h.x;
        v[1] = h.y;
      }
      V mk[W];
#pragma unroll
      for (int b = 0; b < W; ++b)
#pragma unroll
        for (int e = 0; e < VW; ++e) mk[b][e] = bit_smear<W>(v[e], b);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        ConstU32 *pc = prod + (r * K + j) * W;  // wave-uniform -> scalar loads
        const uint32_t c0 = pc[0];
        if (c0 == 0) continue;
        if (c0 == kOne) {
          acc[r] ^= v;
          continue;
        }
#pragma unroll
        for (int b = 0; b < W; ++b) {
          const uint32_t pb = pc[b];
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[r][e] = __builtin_amdgcn_bitop3_b32(acc[r][e], mk[b][e], pb, 0x78);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t q = a.out[r].base + s * a.out[r].stride + off;
      if (whole) {
        put_nt<ACC, V>(q, acc[r]);
      } else {
        u32x2 h;
        h.x = acc[r][0];
        h.y = acc[r][1];
        put<ACC, u32x2>(q, h);
      }
    }
  }
}

// ------------------------------------------------------------------ bit-sliced GF(2^16) / GF(2^32)
// Cauchy codes at w = 16 / 32 in Jerasure's packet layout: a super-packet is W packets of P
// bytes, and bit x of element (t, b) is bit b of byte t of packet x, so a 32-bit word of each
// of the W packets holds bit x of 32 elements -- the w = 8 bit-sliced scheme with W slices.
// Multiplying all 32 elements by x renames the slices and XORs the top slice into the
// polynomial's taps (Jerasure's fields, galois.c:65-98: x^16 = x^12+x^3+x+1, x^32 =
// x^22+x^2+x+1), and c*e = sum_{t: c_t = 1} x^t e.  Identical bytes to the bitmatrix of the
// GF(2^W) coefficient matrix (what jerasure_bitmatrix_encode applies), in W XORs per set
// coefficient bit instead of one per set bitmatrix bit, under R*W uniform branches per input
// instead of R*W*W.  Coefficients come from the wordwise image (product b = 0 of a cell).
// (The bit loops below are gf8_sliced_mul_acc's at W slices.  They stay written out: folded
// into it, k_gfw_bitsliced<4, 32> went from 171 to 194 VGPRs.)
template <int W>
__device__ __forceinline__ void times_x_sliced(uint32_t (&e)[W]) {
  const uint32_t top = e[W - 1];
#pragma unroll
  for (int i = W - 1; i > 0; --i) e[i] = e[i - 1];
  e[0] = top;
  if constexpr (W == 16) {
    e[1] ^= top;
    e[3] ^= top;
    e[12] ^= top;
  } else {
    e[1] ^= top;
    e[2] ^= top;
    e[22] ^= top;
  }
}

template <int R, int W, bool ACC = false>
__global__ __launch_bounds__(kBlock) void k_gfw_bitsliced(ApplyArgs a) {
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / W);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4;
  constexpr uint32_t kCoefMask = W == 16 ? 0xFFFFu : 0xFFFFFFFFu;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstU32 *prod = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  for (uint32_t t = xcd_remap(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {
    const uint32_t s = t / tiles_per_stripe;
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * 4;
    if (colb >= col_bytes) continue;
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * W * P + (colb - sp * P);
    uint32_t acc[R][W];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int l = 0; l < W; ++l) acc[r][l] = 0u;
    for (int j = 0; j < K; ++j) {
      const uint64_t p = a.in[j].base + s * a.in[j].stride + off;
      uint32_t e[W];
#pragma unroll
      for (int x = 0; x < W; ++x) e[x] = __builtin_nontemporal_load(gptr<uint32_t>(p + x * P));
      uint32_t c[R], cm = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        c[r] = prod[(r * K + j) * W] & kCoefMask;  // wave-uniform -> scalar loads
        cm |= c[r];
      }
#pragma unroll
      for (int b = 0; b < W; ++b) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if ((c[r] >> b) & 1u) {
#pragma unroll
            for (int x = 0; x < W; ++x) acc[r][x] ^= e[x];
          }
        if (b == W - 1 || (cm >> (b + 1)) == 0) break;
        times_x_sliced<W>(e);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t q = a.out[r].base + s * a.out[r].stride + off;
#pragma unroll
      for (int l = 0; l < W; ++l) put_nt<ACC, uint32_t>(q + l * P, acc[r][l]);
    }
  }
}

// ------------------------------------------------------------------ transposed GF(2^16) / GF(2^32)
// RS / r6 at w = 16 / 32 keep Jerasure's word layout (element t = little-endian uint16/uint32
// at byte 2t / 4t, galois.c:527-604, :730-810).  Each lane loads W dwords of a shard (32
// elements: W/4 coalesced 16 B pieces), transposes the W x W bit blocks in registers so that
// word x holds bit x of all 32 elements, runs k_gfw_bitsliced's arithmetic (one XOR per slice
// per set coefficient bit), and transposes back.  A W x W transpose is log2(W) swap stages:
// byte and halfword stages are two v_perm_b32 per pair of words, bit stages two shifts and two
// v_bfi_b32.  Elements never mix, so a zero-filled tail produces zeros that are not stored.
template <int W, int d>
__device__ __forceinline__ void transpose_bits(uint32_t (&D)[W], uint32_t m) {
#pragma unroll
  for (int r = 0; r < W; ++r) {
    if (r & d) continue;
    const uint32_t x = D[r], y = D[r + d];
    D[r] = (x & m) | ((y << d) & ~m);
    D[r + d] = ((x >> d) & m) | (y & ~m);
  }
}

template <int W>
__device__ __forceinline__ void transpose_units(uint32_t (&D)[W]) {
  if constexpr (W == 32) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t x = D[r], y = D[r + 16];
      D[r] = __builtin_amdgcn_perm(y, x, 0x05040100u);       // (x.lo, y.lo)
      D[r + 16] = __builtin_amdgcn_perm(y, x, 0x07060302u);  // (x.hi, y.hi)
    }
  }
#pragma unroll
  for (int r = 0; r < W; ++r) {
    if (r & 8) continue;
    const uint32_t x = D[r], y = D[r + 8];
    D[r] = __builtin_amdgcn_perm(y, x, 0x06020400u);      // (x.b0, y.b0, x.b2, y.b2)
    D[r + 8] = __builtin_amdgcn_perm(y, x, 0x07030501u);  // (x.b1, y.b1, x.b3, y.b3)
  }
  transpose_bits<W, 4>(D, 0x0F0F0F0Fu);
  transpose_bits<W, 2>(D, 0x33333333u);
  transpose_bits<W, 1>(D, 0x55555555u);
}

template <int R, int W, bool xor_only, bool ACC>
__device__ __forceinline__ void gfw_transposed_tiles(const ApplyArgs &a) {
  constexpr int kPieces = W / 4;  // 16 B pieces per lane per shard
  constexpr uint32_t kTile = kBlock * 4 * W;
  constexpr uint32_t kCoefMask = W == 16 ? 0xFFFFu : 0xFFFFFFFFu;
  const int K = a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstU32 *prod = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  for (uint32_t t = xcd_remap(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {
    const uint32_t s = t / tiles_per_stripe;
    const int64_t base = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * 16;
    if (base >= C) continue;
    // whole tile in range: every piece is a full 16 B; otherwise per piece (C % 8 == 0)
    const bool whole = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + kTile <= C;
    uint32_t acc[R][W];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int l = 0; l < W; ++l) acc[r][l] = 0u;
    for (int j = 0; j < K; ++j) {
      const uint64_t p = a.in[j].base + s * a.in[j].stride;
      uint32_t e[W];
#pragma unroll
      for (int q = 0; q < kPieces; ++q) {
        const int64_t o = base + static_cast<int64_t>(q) * kBlock * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (whole || o + 16 <= C) {
          v = __builtin_nontemporal_load(gptr<u32x4>(p + o));
        } else if (o + 8 <= C) {
          const u32x2 h = *gptr<u32x2>(p + o);
          v.x = h.x;
          v.y = h.y;
        }
        e[4 * q] = v.x;
        e[4 * q + 1] = v.y;
        e[4 * q + 2] = v.z;
        e[4 * q + 3] = v.w;
      }
      uint32_t c[R], cm = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        c[r] = prod[(r * K + j) * W] & kCoefMask;  // wave-uniform -> scalar loads
        cm |= c[r];
      }
      if (cm == 0) continue;
      if constexpr (xor_only) {  // coefficients 0 / 1: plain XOR, no transposes
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (c[r])
#pragma unroll
            for (int x = 0; x < W; ++x) acc[r][x] ^= e[x];
        continue;
      }
      transpose_units<W>(e);
#pragma unroll
      for (int b = 0; b < W; ++b) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if ((c[r] >> b) & 1u) {
#pragma unroll
            for (int x = 0; x < W; ++x) acc[r][x] ^= e[x];
          }
        if (b == W - 1 || (cm >> (b + 1)) == 0) break;
        times_x_sliced<W>(e);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (!xor_only) transpose_units<W>(acc[r]);
      const uint64_t q0 = a.out[r].base + s * a.out[r].stride;
#pragma unroll
      for (int q = 0; q < kPieces; ++q) {
        const int64_t o = base + static_cast<int64_t>(q) * kBlock * 16;
        const u32x4 v = {acc[r][4 * q], acc[r][4 * q + 1], acc[r][4 * q + 2], acc[r][4 * q + 3]};
        if (whole || o + 16 <= C) {
          put_nt<ACC, u32x4>(q0 + o, v);
        } else if (o + 8 <= C) {
          u32x2 h;
          h.x = v.x;
          h.y = v.y;
          put<ACC, u32x2>(q0 + o, h);
        }
      }
    }
  }
}

// One kernel, two whole tile loops chosen by a uniform branch: a launch whose coefficients are
// all 0 / 1 (XOR-of-survivors decodes) is plain XOR and skips the bit slicing.
template <int R, int W, bool ACC = false>
__global__ __launch_bounds__(kBlock) void k_gfw_transposed(ApplyArgs a) {
  constexpr uint32_t kCoefMask = W == 16 ? 0xFFFFu : 0xFFFFFFFFu;
  ConstU32 *prod = reinterpret_cast<ConstU32 *>(reinterpret_cast<uintptr_t>(a.masks));
  bool xor_only = true;
  for (int i = 0; i < R * a.K && xor_only; ++i) xor_only = (prod[i * W] & kCoefMask) <= 1u;
  if (xor_only)
    gfw_transposed_tiles<R, W, true, ACC>(a);
  else
    gfw_transposed_tiles<R, W, false, ACC>(a);
}

// word sizes the liberation family can produce: primes (liberation), p-1 for prime p
// (blaum_roth), 8 (liber8tion); 16 and 32 for Cauchy at those word sizes
#define LSEC_BITMATRIX_W(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(10) X(11) X(12) X(13) X(16) X(17) \
                            X(18) X(19) X(22) X(23) X(28) X(29) X(30) X(31) X(32)

// ------------------------------------------------------------------ per-R dispatch
// the K with fixed-K forms of the bytewise kernels (the encode's, the check's and the locate's)
#define LSEC_FIXED_K(X) X(4) X(6) X(8) X(10) X(12) X(16) X(20)
constexpr bool has_fixed_k(int K) {
#define LSEC_IS_K(KK) \
  if (K == KK) return true;
  LSEC_FIXED_K(LSEC_IS_K)
#undef LSEC_IS_K
  return false;
}

// Bytewise launch shapes (tile per lane): IT steps of VW dwords, BF the coefficient path.  By code:
//   0 -> (2, 4) 32 B/lane, branch-free   1 -> (1, 4) 16 B/lane, branch-free
//   2 -> (2, 2) 16 B/lane in 8 B pieces, branch-free   3 -> (1, 2) 8 B/lane, branch-free
//   4 -> (1, 2) 8 B/lane, per-cell branches (single-output decodes: mostly XORs of
//        coefficient-1 inputs, which the branch turns into one v_xor instead of 3 perms)
struct BwShape {
  int it, vw;
  bool bf;
  constexpr uint64_t tile_bytes() const { return static_cast<uint64_t>(kBlock) * 4 * vw * it; }
};
constexpr int kBwShapes = 5;
constexpr BwShape bw_shape(int code) {
  return code == 0 ? BwShape{2, 4, true} : code == 1 ? BwShape{1, 4, true} : code == 2 ? BwShape{2, 2, true}
       : code == 3 ? BwShape{1, 2, true} : BwShape{1, 2, false};
}
// The automatic shape of a K x R launch, as a code (measured with tools/kbench.py:
// profiles/r01_v6_kbench_branchfree.txt, r01_v10_kbench_xorrow.txt); the encode, the patterned
// decode, the check and the locate all take it, so their tiles and vector widths agree:
//   R == 1 (single-erasure decode: XOR-heavy, read-bound)  8 B per lane, branchy cells
//   K >= 16 (VALU-bound wide codes)                          16 B per lane, branch-free: 2 x 16 B
//                                                            needs 256 VGPRs there (1 wave/SIMD);
//                                                            RS 20+6 67 %, 16+4 79 % vs 51 / 63 %
//   otherwise                                                2 x 16 B per lane, branch-free
constexpr int bw_auto_code(int K, int R) { return R == 1 ? 4 : K >= 16 ? 1 : 0; }
constexpr BwShape bw_auto(int K, int R) { return bw_shape(bw_auto_code(K, R)); }
// encode + magic is branch-free at 16 B units for every R: the rule's steps for two or more rows
constexpr int bytewise_magic_it(int K) { return bw_auto(K, 2).it; }

// the record of a k_gf8_bytewise<R, KC, IT, BF, VW, MG, ACC> launch (ec_kernels.h, ApplyForm); loop: 1 where the
// kernel holds the two loops, which record_apply and predict_apply_launch turn into the loop the first row selects
constexpr ApplyForm bw_apply_form(int R, int KC, int IT, bool BF, int VW, bool MG = false, bool ACC = false) {
  return ApplyForm{1, R, KC, IT, VW, BF ? 1 : 0, 0, 0, ACC ? 1 : 0, MG ? 1 : 0, 0, bw_dual_loops(R, KC, BF) ? 1 : -1};
}

template <int R, int IT, bool BF, int VW>
hipError_t bytewise_k(const ApplyArgs &a, hipStream_t st, int grid) {
  switch (a.K) {
#define LSEC_BW_K(KK)                                \
  case KK:                                           \
    record_apply(bw_apply_form(R, KK, IT, BF, VW)); \
    return launch_tiled(&k_gf8_bytewise<R, KK, IT, BF, VW>, grid, st, a);
    LSEC_FIXED_K(LSEC_BW_K)
#undef LSEC_BW_K
    default:
      record_apply(bw_apply_form(R, 0, IT, BF, VW));
      return launch_tiled(&k_gf8_bytewise<R, 0, IT, BF, VW>, grid, st, a);
  }
}

template <int R>
hipError_t dispatch_bytewise(const ApplyArgs &a, hipStream_t st, int grid, int shape) {
  if (a.accumulate) {  // a later input group of a wide stripe: generic K, 16 B per lane (shape 1)
    record_apply(bw_apply_form(R, 0, 1, true, 4, false, true));
    return launch_tiled(&k_gf8_bytewise<R, 0, 1, true, 4, false, true>, grid, st, a);
  }
  switch (shape) {
    case 1: return bytewise_k<R, 1, true, 4>(a, st, grid);
    case 2: return bytewise_k<R, 2, true, 2>(a, st, grid);
    case 3: return bytewise_k<R, 1, true, 2>(a, st, grid);
    case 4: return bytewise_k<R, 1, false, 2>(a, st, grid);
    default: return bytewise_k<R, 2, true, 4>(a, st, grid);
  }
}

// encode + magic: 2 x 16 B per lane, 16 B for K >= 16 (bytewise_magic_it)
template <int R>
hipError_t dispatch_bytewise_magic(const ApplyArgs &a, hipStream_t st, int grid) {
  switch (a.K) {
#define LSEC_BWM_K(KK)                                                           \
  case KK:                                                                      \
    record_apply(bw_apply_form(R, KK, bytewise_magic_it(KK), true, 4, true)); \
    return launch_tiled(&k_gf8_bytewise<R, KK, bytewise_magic_it(KK), true, 4, true>, grid, st, a);
    LSEC_FIXED_K(LSEC_BWM_K)
#undef LSEC_BWM_K
    default:
      if (bytewise_magic_it(a.K) == 1) {
        record_apply(bw_apply_form(R, 0, 1, true, 4, true));
        return launch_tiled(&k_gf8_bytewise<R, 0, 1, true, 4, true>, grid, st, a);
      }
      record_apply(bw_apply_form(R, 0, 2, true, 4, true));
      return launch_tiled(&k_gf8_bytewise<R, 0, 2, true, 4, true>, grid, st, a);
  }
}

// the records of the other apply kernels: k_gf8_bitsliced<R, 0, DW, MG, ACC>, k_bitmatrix<R, W> (per_w) or
// k_bitmatrix_any<R>, k_gfw_transposed<R, W, ACC> (transposed) or k_gfw_wordwise<R, W, ACC>, k_gfw_bitsliced<R, W, ACC>
constexpr ApplyForm bs_apply_form(int R, int DW, bool MG = false, bool ACC = false) {
  return ApplyForm{2, R, 0, 0, 0, 0, DW, 8, ACC ? 1 : 0, MG ? 1 : 0, 0, -1};
}
constexpr ApplyForm bm_apply_form(int R, int w, bool per_w, bool ACC) { return ApplyForm{3, R, 0, 0, 0, 0, 0, w, ACC ? 1 : 0, 0, per_w ? 1 : 0, -1}; }
constexpr ApplyForm gfw_apply_form(int kind, int R, int w, bool transposed, bool ACC) {
  return ApplyForm{kind, R, 0, 0, 0, 0, 0, w, ACC ? 1 : 0, 0, transposed ? 1 : 0, -1};
}

template <int R>
hipError_t dispatch_bitsliced(const ApplyArgs &a, hipStream_t st, int grid, int dw) {
  if (a.magic_acc) {  // encode + stripe magic, one lane dword wide
    record_apply(bs_apply_form(R, 1, true, false));
    return launch_tiled(&k_gf8_bitsliced<R, 0, 1, true>, grid, st, a);
  }
  if (a.accumulate) {  // a later input group of a wide stripe, one lane dword wide
    record_apply(bs_apply_form(R, 1, false, true));
    return launch_tiled(&k_gf8_bitsliced<R, 0, 1, false, true>, grid, st, a);
  }
  switch (dw) {
    case 4: record_apply(bs_apply_form(R, 4)); return launch_tiled(&k_gf8_bitsliced<R, 0, 4>, grid, st, a);
    case 2: record_apply(bs_apply_form(R, 2)); return launch_tiled(&k_gf8_bitsliced<R, 0, 2>, grid, st, a);
    default: record_apply(bs_apply_form(R, 1)); return launch_tiled(&k_gf8_bitsliced<R, 0, 1>, grid, st, a);
  }
}

template <int R>
hipError_t dispatch_bitmatrix(const ApplyArgs &a, hipStream_t st, int grid) {
  if constexpr (R <= 2) {
    if (a.accumulate) {  // wide stripes (k > 64) only occur at w > 64: the any-w kernel
      record_apply(bm_apply_form(R, a.w, false, true));
      return launch_kernel(&k_bitmatrix_any<R>, dim3(grid), dim3(kBlock), st, a);
    }
    switch (a.w) {
#define LSEC_BM_W(WW)                                 \
  case WW:                                            \
    record_apply(bm_apply_form(R, WW, true, false)); \
    return launch_kernel(&k_bitmatrix<R, WW>, dim3(grid), dim3(kBlock), st, a);
      LSEC_BITMATRIX_W(LSEC_BM_W)
#undef LSEC_BM_W
      default:
        record_apply(bm_apply_form(R, a.w, false, false));
        return launch_kernel(&k_bitmatrix_any<R>, dim3(grid), dim3(kBlock), st, a);
    }
  } else {
    return hipErrorInvalidValue;
  }
}

template <int R>
hipError_t dispatch_wordwise(const ApplyArgs &a, hipStream_t st, int grid) {
  switch (a.w * 2 + (a.accumulate ? 1 : 0)) {
    case 32: record_apply(gfw_apply_form(4, R, 16, false, false)); return launch_kernel(&k_gfw_wordwise<R, 16>, dim3(grid), dim3(kBlock), st, a);
    case 33: record_apply(gfw_apply_form(4, R, 16, false, true)); return launch_kernel(&k_gfw_wordwise<R, 16, true>, dim3(grid), dim3(kBlock), st, a);
    case 64: record_apply(gfw_apply_form(4, R, 32, false, false)); return launch_kernel(&k_gfw_wordwise<R, 32>, dim3(grid), dim3(kBlock), st, a);
    case 65: record_apply(gfw_apply_form(4, R, 32, false, true)); return launch_kernel(&k_gfw_wordwise<R, 32, true>, dim3(grid), dim3(kBlock), st, a);
    default: return hipErrorInvalidValue;
  }
}

// at most 8 rows per launch at w = 16, 4 at w = 32 (acc[R][W] lives in VGPRs)
template <int R>
hipError_t dispatch_gfw_transposed(const ApplyArgs &a, hipStream_t st, int grid) {
  if (a.w == 16) {
    if (a.accumulate) {
      record_apply(gfw_apply_form(4, R, 16, true, true));
      return launch_kernel(&k_gfw_transposed<R, 16, true>, dim3(grid), dim3(kBlock), st, a);
    }
    record_apply(gfw_apply_form(4, R, 16, true, false));
    return launch_kernel(&k_gfw_transposed<R, 16>, dim3(grid), dim3(kBlock), st, a);
  } else if constexpr (R <= 4) {
    if (a.w != 32) return hipErrorInvalidValue;
    if (a.accumulate) {
      record_apply(gfw_apply_form(4, R, 32, true, true));
      return launch_kernel(&k_gfw_transposed<R, 32, true>, dim3(grid), dim3(kBlock), st, a);
    }
    record_apply(gfw_apply_form(4, R, 32, true, false));
    return launch_kernel(&k_gfw_transposed<R, 32>, dim3(grid), dim3(kBlock), st, a);
  } else {
    return hipErrorInvalidValue;
  }
}

template <int R>
hipError_t dispatch_gfw_bitsliced(const ApplyArgs &a, hipStream_t st, int grid) {
  if (a.w == 16) {
    if (a.accumulate) {
      record_apply(gfw_apply_form(5, R, 16, false, true));
      return launch_kernel(&k_gfw_bitsliced<R, 16, true>, dim3(grid), dim3(kBlock), st, a);
    }
    record_apply(gfw_apply_form(5, R, 16, false, false));
    return launch_kernel(&k_gfw_bitsliced<R, 16>, dim3(grid), dim3(kBlock), st, a);
  } else if constexpr (R <= 4) {
    if (a.w != 32) return hipErrorInvalidValue;
    if (a.accumulate) {
      record_apply(gfw_apply_form(5, R, 32, false, true));
      return launch_kernel(&k_gfw_bitsliced<R, 32, true>, dim3(grid), dim3(kBlock), st, a);
    }
    record_apply(gfw_apply_form(5, R, 32, false, false));
    return launch_kernel(&k_gfw_bitsliced<R, 32>, dim3(grid), dim3(kBlock), st, a);
  } else {
    return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ per-stripe erasure patterns
// Decodes of stripes that do not share an erasure pattern, in one launch (ec_kernels.h,
// PatternArgs).  The arithmetic is that of k_gf8_bytewise / k_gf8_bitsliced; what differs is
// where a tile takes its matrix and its shards from: its stripe's pattern record, looked up once
// per tile.  Everything the lookup yields is wave-uniform (the tile index is, the pattern id is
// made so, the record and the cells come through the constant address space), so the selection
// costs scalar loads only.  R is the table's largest erasure count: a pattern with fewer
// erasures has zero cells in its remaining rows and its stores stop at its own count.
typedef const __attribute__((address_space(4))) PatRecord ConstRec;

// the pattern id of stripe s (s uniform over the workgroup)
__device__ __forceinline__ uint32_t stripe_pattern_id(const PatternArgs &a, uint32_t s) {
  if (a.stripe_pattern)
    return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(*gptr<uint8_t>(reinterpret_cast<uint64_t>(a.stripe_pattern) + s)));
  return (a.rot0 + (s % a.rot_n) * a.rot_step) % a.rot_n;  // rot0, rot_step < rot_n <= kPatMaxShards: 32 bits do
}

// (n - rot_s) of stripe s under the rotation fields of CheckRotArgs / PatternRotArgs, 1..n: logical
// chunk c of the stripe is shard (c + back) mod n.  s is uniform over the workgroup; readfirstlane
// says so to the compiler, and every index derived from it stays in scalar registers.
template <typename Args>
__device__ __forceinline__ uint32_t rot_back(const Args &a, uint32_t s) {
  return __builtin_amdgcn_readfirstlane(a.rot_n - (a.rot0 + (s % a.rot_n) * a.rot_step) % a.rot_n);
}

// Where a patterned tile takes a shard ref from: the record's selection itself (PatternArgs), or
// the physical device holding that logical chunk in stripe s (PatternRotArgs, PatternSearchRotArgs and
// PatternMagicRotArgs, ec_kernels.h).
template <typename Args>
struct PatShards {
  static constexpr bool kRot = std::is_same<Args, PatternRotArgs>::value || std::is_same<Args, PatternSearchRotArgs>::value ||
                               std::is_same<Args, PatternMagicRotArgs>::value;
  const Args &a;
  uint32_t back = 0;
  __device__ __forceinline__ PatShards(const Args &a_, uint32_t s) : a(a_) {
    if constexpr (kRot) back = rot_back(a, s);
  }
  __device__ __forceinline__ ShardRef at(uint32_t sel) const {
    if constexpr (kRot) {
      uint32_t i = sel + back;
      if (i >= a.rot_n) i -= a.rot_n;
      return a.sh[i];
    } else {
      return a.sh[sel];
    }
  }
};

// BF as k_gf8_bytewise: the branch-free coefficient path, or per-cell branches (R = 1).  KC > 0:
// K fixed at compile time, so a full tile has all its K*IT loads in flight before any arithmetic,
// as the single-pattern kernel's fixed-K forms have (with four inputs at a time the one-row
// kernel ran at 0.56 of 8 TB/s against their 0.75: profiles/patterns_kbench_runtime_k.txt).
// Instantiated for the one-row kernel only (dispatch_pat_bytewise).  Args: PatternArgs, or
// PatternRotArgs for the rotated single-erasure repair (the same tile body up to PatShards).
//
// MG (lsec_decode_magic_dev_patterns / _rotated / _patterns_rotated; Args: PatternMagicArgs, or PatternMagicRotArgs
// for logical patterns over rotating shards): the tile also sums the
// stripe's adler32 magic over all of its chunks as the decode leaves them.  One MagicLane takes every
// survivor the tile loads, every row it rebuilds (r < nout) and the pattern's unused survivors
// (PatUnused, loaded here for the checksum alone), each at its LOGICAL chunk id (pat_logical), and the
// tile commits once through block_sum into macc[2s], macc[2s + 1].  block_sum has barriers: every lane
// of the workgroup reaches it.  The one exit ahead of it, id >= npat, is uniform over the workgroup;
// nout == 0 no longer leaves but takes the checksum-only path (no image is read, nothing is
// stored), and units past the end of a ragged tile read as zero and add nothing.  red: kBlock / 64
// words of LDS.  Without MG un, macc and red are not looked at and the code is the plain decode's.
//
// SR (lsec_search_dev_patterns / _rotated; Args: PatternSearchArgs, PatternSearchRotArgs; with MG): the
// trial of a candidate.  A tile belongs to (stripe s, candidate p, piece of the chunk), all three from the
// tile index (pat_search_tile), and p is a record of the table, never a stripe_pattern id.  The tile reads
// select[s] first and leaves when it is 0 -- uniform over the workgroup, ahead of every shard access and
// of block_sum.  Then it is the MG tile with every store to a shard compiled out, and it commits into the
// accumulator pair of (s, p): macc[2(s * npat + p)], [.. + 1].  NT: pat_load's.
typedef const __attribute__((address_space(4))) PatUnused ConstUnused;

// the logical chunk id of selection sel in a stripe of pattern p: the records of a call without a
// stripe_pattern hold the physical devices of rotation p (wave-uniform scalar arithmetic); the search's
// records (SR) are logical whether its shards rotate or not
template <bool SR = false>
__device__ __forceinline__ uint32_t pat_logical(const PatternArgs &a, uint32_t p, uint32_t sel) {
  if (SR || a.stripe_pattern) return sel;
  const uint32_t c = sel + p;
  return c >= static_cast<uint32_t>(a.nshards) ? c - static_cast<uint32_t>(a.nshards) : c;
}

// A streaming load of the patterned tiles: non-temporal as everywhere else, or (the search's A/B form)
// a plain one, which leaves the line in the XCD's L2 for the candidates that read it next.
template <bool NT, typename V>
__device__ __forceinline__ V pat_load(uint64_t p) {
  if constexpr (NT) return __builtin_nontemporal_load(gptr<V>(p));
  else return *gptr<V>(p);
}

// bw_inputs for the MG tiles of a full tile: the same loads and arithmetic (`work`: the pattern has
// rows to form, wave-uniform), and every input's units handed to seen(j, units) once they are loaded.
// X0 and extra() as bw_inputs (the check's MG tiles: its stored parity loads, issued where bw_inputs
// issues them).  EARLY (K fixed; the caller always has work): an input is handed to seen() right
// ahead of its own arithmetic, not behind everybody's, so its registers die with its pair as in
// bw_inputs.  The patterned MG tiles leave all three at their defaults.  NT: pat_load's.
template <int R, int KC, int IT, int VW, bool BF, bool X0 = false, bool EARLY = false, bool NT = true, typename Addr,
          typename Seen, typename Extra = NoLoads>
__device__ __forceinline__ void bw_inputs_seen(typename VecT<VW>::type (&acc)[IT][R], ConstCell *cells, int K, bool work,
                                               Addr &&addr, Seen &&seen, Extra &&extra = Extra()) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  if constexpr (KC > 0) {
    V v[KC][IT];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const uint64_t p = addr(j);
#pragma unroll
      for (int it = 0; it < IT; ++it) v[j][it] = pat_load<NT, V>(p + it * kStep);
    }
    extra();
    if constexpr (EARLY) {
      if constexpr (BF) {
#pragma unroll
        for (int j = 0; j + 1 < KC; j += 2) {
          seen(j, v[j]);
          seen(j + 1, v[j + 1]);
          bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[j], v[j + 1], cells, K, j);
        }
        if constexpr (KC % 2) {
          seen(KC - 1, v[KC - 1]);
          bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[KC - 1], v[KC - 1], cells, K, KC - 1);
        }
      } else {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          seen(j, v[j]);
          bw_accumulate<R, IT, VW>(acc, v[j], cells, K, j);
        }
      }
    } else {
      if (work) {
        if constexpr (BF) {
#pragma unroll
          for (int j = 0; j + 1 < KC; j += 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[j], v[j + 1], cells, K, j);
          if constexpr (KC % 2) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[KC - 1], v[KC - 1], cells, K, KC - 1);
        } else {
#pragma unroll
          for (int j = 0; j < KC; ++j) bw_accumulate<R, IT, VW>(acc, v[j], cells, K, j);
        }
      }
#pragma unroll
      for (int j = 0; j < KC; ++j) seen(j, v[j]);
    }
  } else {
    extra();
    for (int j0 = 0; j0 < K; j0 += 4) {
      V v[4][IT];
      const int nj = min(4, K - j0);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (jj < nj) {
          const uint64_t p = addr(j0 + jj);
#pragma unroll
          for (int it = 0; it < IT; ++it) v[jj][it] = pat_load<NT, V>(p + it * kStep);
        }
      }
      if (work) {
        if constexpr (BF) {
          if (nj >= 2) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[0], v[1], cells, K, j0);
          if (nj == 4) bw_accumulate_bf<R, IT, VW, true, X0>(acc, v[2], v[3], cells, K, j0 + 2);
          if (nj == 1 || nj == 3) bw_accumulate_bf<R, IT, VW, false, X0>(acc, v[nj - 1], v[nj - 1], cells, K, j0 + nj - 1);
        } else {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            if (jj < nj) bw_accumulate<R, IT, VW>(acc, v[jj], cells, K, j0 + jj);
        }
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        if (jj < nj) seen(j0 + jj, v[jj]);
    }
  }
}

// The (stripe, candidate, piece) of search tile t, tps pieces per stripe.  cand_outer 0: the candidate runs
// innermost, so the tiles an XCD takes in a row read the same bytes of one stripe; 1: the piece does.
template <typename Args>
__device__ __forceinline__ void pat_search_tile(const Args &a, uint32_t t, uint32_t tps, uint32_t &s, uint32_t &p, uint32_t &piece) {
  if (a.cand_outer) {
    const uint32_t sp = t / tps;
    piece = t - sp * tps;
    s = sp / a.npat;
    p = sp - s * a.npat;
  } else {
    const uint32_t sq = t / a.npat;
    p = t - sq * a.npat;
    s = sq / tps;
    piece = sq - s * tps;
  }
}
// select[s] != 0, or no select (s uniform over the workgroup)
template <typename Args>
__device__ __forceinline__ bool pat_search_selected(const Args &a, uint32_t s) {
  if (!a.select) return true;
  return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(*gptr<uint8_t>(reinterpret_cast<uint64_t>(a.select) + s))) != 0;
}

template <int R, int KC, int IT, int VW, bool BF, bool MG = false, bool SR = false, bool NT = true, typename Args>
__device__ __forceinline__ void pat_bytewise_tiles(const Args &a, ConstUnused *un = nullptr, unsigned long long *macc = nullptr,
                                                   uint32_t *red = nullptr) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = KC ? KC : a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  if constexpr (SR) ntiles *= a.npat;
  ConstRec *recs = reinterpret_cast<ConstRec *>(reinterpret_cast<uintptr_t>(a.recs));
  ConstCell *images = const_cells(a.cells);

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    uint32_t s, p, piece;
    if constexpr (SR) {
      pat_search_tile(a, t, tiles_per_stripe, s, p, piece);
      if (!pat_search_selected(a, s)) return;  // not searched: none of its chunks is read
    } else {
      s = t / tiles_per_stripe;
      piece = t - s * tiles_per_stripe;
      p = stripe_pattern_id(a, s);
      if (p >= a.npat) return;  // no such pattern: the stripe is left alone
    }
    ConstRec *rec = recs + p;
    const uint32_t nout = rec->nout;
    if (!MG && nout == 0) return;  // nothing to rebuild
    ConstCell *cells = images + rec->cells_off;
    const PatShards<Args> sh(a, s);
    const int64_t off0 = static_cast<int64_t>(piece) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(piece) + 1) * kTile <= C;  // wave-uniform
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    V acc[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[it][r] = 0u;

    if (full) {
      if constexpr (MG) {
        bw_inputs_seen<R, KC, IT, VW, BF, false, false, NT>(
            acc, cells, K, nout != 0,
            [&](int j) LSEC_INLINE {
              const ShardRef in = sh.at(rec->in_sel[j]);
              return in.base + s * in.stride + off0;
            },
            [&](int j, const V(&v)[IT]) LSEC_INLINE { ml_add<IT, VW>(ml, v, pat_logical<SR>(a, p, rec->in_sel[j])); });
      } else {
        bw_inputs<R, KC, IT, VW, BF, false>(
            acc, cells, K,
            [&](int j) LSEC_INLINE {
              const ShardRef in = sh.at(rec->in_sel[j]);
              return in.base + s * in.stride + off0;
            },
            NoLoads());
      }
      if constexpr (!SR) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (static_cast<uint32_t>(r) < nout) {  // wave-uniform
            const ShardRef out = sh.at(rec->out_sel[r]);
            const uint64_t q = out.base + s * out.stride + off0;
#pragma unroll
            for (int it = 0; it < IT; ++it) put_nt<false, V>(q + it * kStep, acc[it][r]);
          }
        }
      }
    } else {
      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.at(rec->in_sel[j]);
        const uint64_t q = in.base + s * in.stride;
        V v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) v[it] = load_ragged<VW>(q, off0 + it * kStep, C);
        if constexpr (MG) {
          ml_add<IT, VW>(ml, v, pat_logical<SR>(a, p, rec->in_sel[j]));
          if (nout == 0) continue;  // checksum only: the record has no image
        }
        bw_acc1<R, IT, VW, BF, false>(acc, v, cells, K, j);
      }
      if constexpr (!SR) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (static_cast<uint32_t>(r) < nout) {
            const ShardRef out = sh.at(rec->out_sel[r]);
            const uint64_t q = out.base + s * out.stride;
#pragma unroll
            for (int it = 0; it < IT; ++it) store_ragged<false, VW>(q, off0 + it * kStep, C, acc[it][r]);
          }
        }
      }
    }
    if constexpr (MG) {
      // the rebuilt rows as stored (a ragged tile's units past C were formed from zeros and are zero)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (static_cast<uint32_t>(r) < nout) {
          V o[IT];
#pragma unroll
          for (int it = 0; it < IT; ++it) o[it] = acc[it][r];
          ml_add<IT, VW>(ml, o, pat_logical<SR>(a, p, rec->out_sel[r]));
        }
      }
      // the survivors the decode did not read, up to four in flight as the inputs are
      ConstUnused *ur = un + p;
      const uint32_t nu = min(ur->n, static_cast<uint32_t>(kPatMaxUnused));
      for (uint32_t u0 = 0; u0 < nu; u0 += 4) {
        V v[4][IT];
#pragma unroll
        for (uint32_t uu = 0; uu < 4; ++uu) {
          if (u0 + uu < nu) {
            const ShardRef in = sh.at(ur->sel[u0 + uu]);
            const uint64_t q = in.base + s * in.stride;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
              if (full) v[uu][it] = pat_load<NT, V>(q + off0 + it * kStep);
              else v[uu][it] = load_ragged<VW>(q, off0 + it * kStep, C);
            }
          }
        }
#pragma unroll
        for (uint32_t uu = 0; uu < 4; ++uu)
          if (u0 + uu < nu) ml_add<IT, VW>(ml, v[uu], pat_logical<SR>(a, p, ur->sel[u0 + uu]));
      }
      ml_commit(ml, macc, SR ? s * a.npat + p : s, a.nshards, static_cast<uint64_t>(C), static_cast<uint64_t>(off0), kStep, red);
    }
  }, a.tile_phase);
}

template <int R, int KC, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_pat_bytewise(PatternArgs a) {
  pat_bytewise_tiles<R, KC, IT, VW, BF>(a);
}

template <int R, int KC, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_patrot_bytewise(PatternRotArgs a) {
  pat_bytewise_tiles<R, KC, IT, VW, BF>(a);
}

template <int R, int KC, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_patmagic_bytewise(PatternMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bytewise_tiles<R, KC, IT, VW, BF, true>(
      a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc, red);
}

// The MG tile over the devices of a rotated LUN with a logical pattern per stripe
// (lsec_decode_magic_dev_patterns_rotated): every selection becomes a physical device through PatShards,
// whose rotation stays in scalar registers (rot_back), and the magic ids are the selections themselves
// (pat_logical with a stripe_pattern).  The stores are on.
template <int R, int KC, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_patmagicrot_bytewise(PatternMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bytewise_tiles<R, KC, IT, VW, BF, true>(
      a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc, red);
}

// k_gf8_bitsliced's lanes (one dword of packet-column space per lane) under a pattern record.
// MG as in pat_bytewise_tiles: the lanes past the end of a ragged last tile then skip the loads and
// the stores, but still join the tile's reduction (as k_gf8_bitsliced's do).  SR, NT as there.
template <int R, bool MG = false, bool SR = false, bool NT = true, typename Args>
__device__ __forceinline__ void pat_bitsliced_tiles(const Args &a, ConstUnused *un = nullptr, unsigned long long *macc = nullptr,
                                                    uint32_t *red = nullptr) {
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  if constexpr (SR) ntiles *= a.npat;
  ConstRec *recs = reinterpret_cast<ConstRec *>(reinterpret_cast<uintptr_t>(a.recs));
  ConstCell *images = const_cells(a.cells);

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    uint32_t s, p, piece;
    if constexpr (SR) {
      pat_search_tile(a, t, tiles_per_stripe, s, p, piece);
      if (!pat_search_selected(a, s)) return;
    } else {
      s = t / tiles_per_stripe;
      piece = t - s * tiles_per_stripe;
      p = stripe_pattern_id(a, s);
      if (p >= a.npat) return;
    }
    ConstRec *rec = recs + p;
    const uint32_t nout = rec->nout;
    if (!MG && nout == 0) return;
    ConstCell *cells = images + rec->cells_off;
    const PatShards<Args> sh(a, s);
    const uint32_t colb = piece * kTile + threadIdx.x * 4;
    const bool valid = colb < col_bytes;
    if (!MG && !valid) return;  // lanes past the end of a ragged last tile
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    if (!MG || valid) {
      uint32_t acc[R][8];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[r][x] = 0u;

      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.at(rec->in_sel[j]);
        const uint64_t q = in.base + s * in.stride + off;
        uint32_t e[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) e[x] = pat_load<NT, uint32_t>(q + x * P);
        if constexpr (MG) {
          ml_add<8, 1>(ml, e, pat_logical<SR>(a, p, rec->in_sel[j]));
          if (nout == 0) continue;  // checksum only: the record has no image
        }
        uint32_t c[R];
        uint32_t cm = 0;  // bits used by any output: no doublings past the highest one
#pragma unroll
        for (int r = 0; r < R; ++r) {
          c[r] = cells[r * K + j].coef;
          cm |= c[r];
        }
        gf8_sliced_mul_acc<0>(acc, e, c, cm);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (static_cast<uint32_t>(r) < nout) {  // wave-uniform
          if constexpr (!SR) {
            const ShardRef out = sh.at(rec->out_sel[r]);
            const uint64_t q = out.base + s * out.stride + off;
#pragma unroll
            for (int x = 0; x < 8; ++x) put_nt<false, uint32_t>(q + x * P, acc[r][x]);
          }
          if constexpr (MG) ml_add<8, 1>(ml, acc[r], pat_logical<SR>(a, p, rec->out_sel[r]));
        }
      }
      if constexpr (MG) {
        // the survivors the decode did not read
        ConstUnused *ur = un + p;
        const uint32_t nu = min(ur->n, static_cast<uint32_t>(kPatMaxUnused));
        for (uint32_t u = 0; u < nu; ++u) {
          const ShardRef in = sh.at(ur->sel[u]);
          const uint64_t q = in.base + s * in.stride + off;
          uint32_t e[8];
#pragma unroll
          for (int x = 0; x < 8; ++x) e[x] = pat_load<NT, uint32_t>(q + x * P);
          ml_add<8, 1>(ml, e, pat_logical<SR>(a, p, ur->sel[u]));
        }
      }
    }
    if constexpr (MG)
      ml_commit(ml, macc, SR ? s * a.npat + p : s, a.nshards, static_cast<uint64_t>(a.size), static_cast<uint64_t>(off), P, red);
  }, a.tile_phase);
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_pat_bitsliced(PatternArgs a) {
  pat_bitsliced_tiles<R>(a);
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_patrot_bitsliced(PatternRotArgs a) {
  pat_bitsliced_tiles<R>(a);
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_patmagic_bitsliced(PatternMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bitsliced_tiles<R, true>(a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc, red);
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_patmagicrot_bitsliced(PatternMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bitsliced_tiles<R, true>(a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc, red);
}

// The patterned bytewise kernel takes the automatic shape (bw_auto) of the table's row count and
// K.  The one-row kernel has fixed-K forms for K = 6 and 10; tables of two or more rows run with
// K at run time: their fixed-K forms, with every input's 2 x 16 B in flight on top of the
// accumulators, took 186 (K = 6) and 256 (K = 10) VGPRs and measured slower (RS(10+4), three
// erasures: 17.5 ms against 10.2; profiles/patterns_fixedk_ab.txt).
// K of the one-row kernel's form (0: K at run time), and a table's form by its row count
constexpr int pat_one_row_kc(int K) { return K == 6 || K == 10 ? K : 0; }
struct BwForm {
  int kc, it, vw;
  bool bf;
};
constexpr BwForm pat_bytewise_form(int K, int R) {
  const BwShape sh = bw_auto(R == 1 ? 0 : K, R);
  return BwForm{R == 1 ? pat_one_row_kc(K) : 0, sh.it, sh.vw, sh.bf};
}

template <int R, int KC, int IT, int VW, bool BF>
hipError_t pat_kernel(const PatternArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPat, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_pat_bytewise<R, KC, IT, VW, BF>, grid, st, a);
}

template <int R>
hipError_t dispatch_pat_bytewise(const PatternArgs &a, hipStream_t st, int grid) {
  const BwForm f = pat_bytewise_form(a.K, R);
  if constexpr (R == 1) {
    constexpr BwShape sh = bw_auto(0, 1);
    switch (f.kc) {
      case 6: return pat_kernel<1, 6, sh.it, sh.vw, sh.bf>(a, st, grid);
      case 10: return pat_kernel<1, 10, sh.it, sh.vw, sh.bf>(a, st, grid);
      default: return pat_kernel<1, 0, sh.it, sh.vw, sh.bf>(a, st, grid);
    }
  } else {
    if (f.it == 1) return pat_kernel<R, 0, 1, 4, true>(a, st, grid);
    return pat_kernel<R, 0, 2, 4, true>(a, st, grid);
  }
}

template <int R>
hipError_t dispatch_pat_bitsliced(const PatternArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPat, 1, R, 0, 0, 0, 0, 1});
  return launch_tiled(&k_pat_bitsliced<R>, grid, st, a);
}

// The rotated single-erasure repair: the one-row kernels in dispatch_pat_bytewise<1>'s shapes.
// Defined in ec_patterns_rot_inst.hip alone.
hipError_t dispatch_patrot_bytewise(const PatternRotArgs &a, hipStream_t st, int grid);
hipError_t dispatch_patrot_bitsliced(const PatternRotArgs &a, hipStream_t st, int grid);
#ifdef LSEC_INSTANTIATING_PATROT
template <int KC, int IT, int VW, bool BF>
hipError_t patrot_kernel(const PatternRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatRot, 0, 1, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_patrot_bytewise<1, KC, IT, VW, BF>, grid, st, a);
}

hipError_t dispatch_patrot_bytewise(const PatternRotArgs &a, hipStream_t st, int grid) {
  constexpr BwShape sh = bw_auto(0, 1);
  switch (pat_bytewise_form(a.K, 1).kc) {
    case 6: return patrot_kernel<6, sh.it, sh.vw, sh.bf>(a, st, grid);
    case 10: return patrot_kernel<10, sh.it, sh.vw, sh.bf>(a, st, grid);
    default: return patrot_kernel<0, sh.it, sh.vw, sh.bf>(a, st, grid);
  }
}

hipError_t dispatch_patrot_bitsliced(const PatternRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatRot, 1, 1, 0, 0, 0, 0, 1});
  return launch_tiled(&k_patrot_bitsliced<1>, grid, st, a);
}
#endif

// The MG forms (lsec_decode_magic_dev_patterns / _rotated; DESIGN.md 3.7 has their registers): the
// patterned kernels' own, through a constant of their own, so that one family can move without the other.
constexpr BwForm patmagic_bytewise_form(int K, int R) { return pat_bytewise_form(K, R); }

template <int R, int KC, int IT, int VW, bool BF>
hipError_t patmagic_kernel(const PatternMagicArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatMagic, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_patmagic_bytewise<R, KC, IT, VW, BF>, grid, st, a);
}

template <int R>
hipError_t dispatch_patmagic_bytewise(const PatternMagicArgs &a, hipStream_t st, int grid) {
  const BwForm f = patmagic_bytewise_form(a.K, R);
  if constexpr (R == 1) {
    constexpr BwShape sh = bw_auto(0, 1);
    switch (f.kc) {
      case 6: return patmagic_kernel<1, 6, sh.it, sh.vw, sh.bf>(a, st, grid);
      case 10: return patmagic_kernel<1, 10, sh.it, sh.vw, sh.bf>(a, st, grid);
      default: return patmagic_kernel<1, 0, sh.it, sh.vw, sh.bf>(a, st, grid);
    }
  } else {
    if (f.it == 1) return patmagic_kernel<R, 0, 1, 4, true>(a, st, grid);
    return patmagic_kernel<R, 0, 2, 4, true>(a, st, grid);
  }
}

template <int R>
hipError_t dispatch_patmagic_bitsliced(const PatternMagicArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatMagic, 1, R, 0, 0, 0, 0, 1});
  return launch_tiled(&k_patmagic_bitsliced<R>, grid, st, a);
}

// The MG forms over rotating shards (lsec_decode_magic_dev_patterns_rotated; DESIGN.md 3.7.3 has their
// registers beside the unrotated ones'): the MG forms' own shapes, through a constant of their own.
constexpr BwForm patmagicrot_bytewise_form(int K, int R) { return patmagic_bytewise_form(K, R); }

template <int R, int KC, int IT, int VW, bool BF>
hipError_t patmagicrot_kernel(const PatternMagicRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatMagicRot, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_patmagicrot_bytewise<R, KC, IT, VW, BF>, grid, st, a);
}

template <int R>
hipError_t dispatch_patmagicrot_bytewise(const PatternMagicRotArgs &a, hipStream_t st, int grid) {
  const BwForm f = patmagicrot_bytewise_form(a.K, R);
  if constexpr (R == 1) {
    constexpr BwShape sh = bw_auto(0, 1);
    switch (f.kc) {
      case 6: return patmagicrot_kernel<1, 6, sh.it, sh.vw, sh.bf>(a, st, grid);
      case 10: return patmagicrot_kernel<1, 10, sh.it, sh.vw, sh.bf>(a, st, grid);
      default: return patmagicrot_kernel<1, 0, sh.it, sh.vw, sh.bf>(a, st, grid);
    }
  } else {
    if (f.it == 1) return patmagicrot_kernel<R, 0, 1, 4, true>(a, st, grid);
    return patmagicrot_kernel<R, 0, 2, 4, true>(a, st, grid);
  }
}

template <int R>
hipError_t dispatch_patmagicrot_bitsliced(const PatternMagicRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatMagicRot, 1, R, 0, 0, 0, 0, 1});
  return launch_tiled(&k_patmagicrot_bitsliced<R>, grid, st, a);
}

// The search (lsec_search_dev_patterns / _rotated): the MG tile bodies in their SR mode, in the MG forms'
// own shapes (patsearch_bytewise_form), once per load kind (NT) and per argument struct.
constexpr BwForm patsearch_bytewise_form(int K, int R) { return patmagic_bytewise_form(K, R); }

template <int R, int KC, int IT, int VW, bool BF, bool NT, typename Args>
__global__ __launch_bounds__(kBlock) void k_patsearch_bytewise(Args a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bytewise_tiles<R, KC, IT, VW, BF, true, true, NT>(
      a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc, red);
}

template <int R, bool NT, typename Args>
__global__ __launch_bounds__(kBlock) void k_patsearch_bitsliced(Args a) {
  __shared__ uint32_t red[kBlock / 64];
  pat_bitsliced_tiles<R, true, true, NT>(a, reinterpret_cast<ConstUnused *>(reinterpret_cast<uintptr_t>(a.unused)), a.magic_acc,
                                         red);
}

template <typename Args>
constexpr int patsearch_family() {
  return std::is_same<Args, PatternSearchRotArgs>::value ? kFormPatSearchRot : kFormPatSearch;
}

template <int R, int KC, int IT, int VW, bool BF, typename Args>
hipError_t patsearch_kernel(const Args &a, hipStream_t st, int grid) {
  record_launch({patsearch_family<Args>(), 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  if (a.plain_loads) return launch_tiled(&k_patsearch_bytewise<R, KC, IT, VW, BF, false, Args>, grid, st, a);
  return launch_tiled(&k_patsearch_bytewise<R, KC, IT, VW, BF, true, Args>, grid, st, a);
}

// grid: the launch's tiles, one per (stripe, candidate, piece)
template <int R, typename Args>
hipError_t dispatch_patsearch_bytewise(const Args &a, hipStream_t st, int grid) {
  const BwForm f = patsearch_bytewise_form(a.K, R);
  if constexpr (R == 1) {
    constexpr BwShape sh = bw_auto(0, 1);
    switch (f.kc) {
      case 6: return patsearch_kernel<1, 6, sh.it, sh.vw, sh.bf>(a, st, grid);
      case 10: return patsearch_kernel<1, 10, sh.it, sh.vw, sh.bf>(a, st, grid);
      default: return patsearch_kernel<1, 0, sh.it, sh.vw, sh.bf>(a, st, grid);
    }
  } else {
    if (f.it == 1) return patsearch_kernel<R, 0, 1, 4, true>(a, st, grid);
    return patsearch_kernel<R, 0, 2, 4, true>(a, st, grid);
  }
}

template <int R, typename Args>
hipError_t dispatch_patsearch_bitsliced(const Args &a, hipStream_t st, int grid) {
  record_launch({patsearch_family<Args>(), 1, R, 0, 0, 0, 0, 1});
  if (a.plain_loads) return launch_tiled(&k_patsearch_bitsliced<R, false, Args>, grid, st, a);
  return launch_tiled(&k_patsearch_bitsliced<R, true, Args>, grid, st, a);
}

// instantiated per R in ec_patterns_search_inst.hip
#define LSEC_DECLARE_PATSEARCH_R(RR)                                                                                 \
  extern template hipError_t dispatch_patsearch_bytewise<RR, PatternSearchArgs>(const PatternSearchArgs &, hipStream_t, int);       \
  extern template hipError_t dispatch_patsearch_bitsliced<RR, PatternSearchArgs>(const PatternSearchArgs &, hipStream_t, int);      \
  extern template hipError_t dispatch_patsearch_bytewise<RR, PatternSearchRotArgs>(const PatternSearchRotArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_patsearch_bitsliced<RR, PatternSearchRotArgs>(const PatternSearchRotArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING_PATSEARCH
LSEC_DECLARE_PATSEARCH_R(1) LSEC_DECLARE_PATSEARCH_R(2) LSEC_DECLARE_PATSEARCH_R(3) LSEC_DECLARE_PATSEARCH_R(4)
LSEC_DECLARE_PATSEARCH_R(5) LSEC_DECLARE_PATSEARCH_R(6) LSEC_DECLARE_PATSEARCH_R(7) LSEC_DECLARE_PATSEARCH_R(8)
#endif

// The rotated repair behind a search: k_patrot_* for tables of up to R erasures per pattern, in the patterned
// decode's shapes (pat_bytewise_form), one unit per R (ec_patterns_rot_rows_inst.hip).  One row is the single-row
// unit's own kernels (dispatch_patrot_*), which no second unit instantiates.
template <int R, int IT>
hipError_t patrot_rows_kernel(const PatternRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormPatRot, 0, R, 0, IT, 4, 1, 0});
  return launch_tiled(&k_patrot_bytewise<R, 0, IT, 4, true>, grid, st, a);
}

template <int R>
hipError_t dispatch_patrot_rows_bytewise(const PatternRotArgs &a, hipStream_t st, int grid) {
  if constexpr (R == 1) {
    return dispatch_patrot_bytewise(a, st, grid);
  } else {
    if (pat_bytewise_form(a.K, R).it == 1) return patrot_rows_kernel<R, 1>(a, st, grid);
    return patrot_rows_kernel<R, 2>(a, st, grid);
  }
}

template <int R>
hipError_t dispatch_patrot_rows_bitsliced(const PatternRotArgs &a, hipStream_t st, int grid) {
  if constexpr (R == 1) {
    return dispatch_patrot_bitsliced(a, st, grid);
  } else {
    record_launch({kFormPatRot, 1, R, 0, 0, 0, 0, 1});
    return launch_tiled(&k_patrot_bitsliced<R>, grid, st, a);
  }
}

#define LSEC_DECLARE_PATROT_ROWS_R(RR)                                                                      \
  extern template hipError_t dispatch_patrot_rows_bytewise<RR>(const PatternRotArgs &, hipStream_t, int);  \
  extern template hipError_t dispatch_patrot_rows_bitsliced<RR>(const PatternRotArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING_PATROT_ROWS
LSEC_DECLARE_PATROT_ROWS_R(1) LSEC_DECLARE_PATROT_ROWS_R(2) LSEC_DECLARE_PATROT_ROWS_R(3) LSEC_DECLARE_PATROT_ROWS_R(4)
LSEC_DECLARE_PATROT_ROWS_R(5) LSEC_DECLARE_PATROT_ROWS_R(6) LSEC_DECLARE_PATROT_ROWS_R(7) LSEC_DECLARE_PATROT_ROWS_R(8)
#endif

// instantiated per R in ec_patterns_magic_inst.hip
#define LSEC_DECLARE_PATMAGIC_R(RR)                                                                    \
  extern template hipError_t dispatch_patmagic_bytewise<RR>(const PatternMagicArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_patmagic_bitsliced<RR>(const PatternMagicArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING_PATMAGIC
LSEC_DECLARE_PATMAGIC_R(1) LSEC_DECLARE_PATMAGIC_R(2) LSEC_DECLARE_PATMAGIC_R(3) LSEC_DECLARE_PATMAGIC_R(4)
LSEC_DECLARE_PATMAGIC_R(5) LSEC_DECLARE_PATMAGIC_R(6) LSEC_DECLARE_PATMAGIC_R(7) LSEC_DECLARE_PATMAGIC_R(8)
#endif

// instantiated per R in ec_patterns_magic_rot_inst.hip
#define LSEC_DECLARE_PATMAGICROT_R(RR)                                                                         \
  extern template hipError_t dispatch_patmagicrot_bytewise<RR>(const PatternMagicRotArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_patmagicrot_bitsliced<RR>(const PatternMagicRotArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING_PATMAGICROT
LSEC_DECLARE_PATMAGICROT_R(1) LSEC_DECLARE_PATMAGICROT_R(2) LSEC_DECLARE_PATMAGICROT_R(3) LSEC_DECLARE_PATMAGICROT_R(4)
LSEC_DECLARE_PATMAGICROT_R(5) LSEC_DECLARE_PATMAGICROT_R(6) LSEC_DECLARE_PATMAGICROT_R(7) LSEC_DECLARE_PATMAGICROT_R(8)
#endif

// instantiated per R in ec_patterns_inst.hip
#define LSEC_DECLARE_PAT_R(RR)                                                                  \
  extern template hipError_t dispatch_pat_bytewise<RR>(const PatternArgs &, hipStream_t, int);  \
  extern template hipError_t dispatch_pat_bitsliced<RR>(const PatternArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING_PAT
LSEC_DECLARE_PAT_R(1) LSEC_DECLARE_PAT_R(2) LSEC_DECLARE_PAT_R(3) LSEC_DECLARE_PAT_R(4)
LSEC_DECLARE_PAT_R(5) LSEC_DECLARE_PAT_R(6) LSEC_DECLARE_PAT_R(7) LSEC_DECLARE_PAT_R(8)
#endif

// ------------------------------------------------------------------ parity check
// lsec_check_dev (ec_kernels.h, CheckArgs): the encode kernels' tile loop, loads and arithmetic,
// with the stored parity chunks read alongside the data and compared in registers where the
// encode stores: k + m chunk reads per stripe and no writes unless a stripe is inconsistent.
// There is no barrier and no LDS in the tile body: a wave reduces its rows with a wave-wide vote
// and publishes on its own.

// d |= x ^ y in one VALU op (v_bitop3_b32, truth table (a ^ b) | c = 0xBE)
__device__ __forceinline__ uint32_t or_diff(uint32_t x, uint32_t y, uint32_t d) {
  return __builtin_amdgcn_bitop3_b32(x, y, d, 0xBE);
}

// A wave's finding for stripe s (s uniform over the wave): d[r] != 0 in any active lane sets bit
// r.  One vote decides the common case -- no lane of the wave saw a difference: nothing is issued
// -- and only a wave that did votes per row and has its first active lane publish.  The atomic's
// return value tells the one wave that made the word nonzero, which counts the stripe.
template <int R, typename Args>
__device__ __forceinline__ void chk_publish(const Args &a, uint32_t s, const uint32_t (&d)[R]) {
  uint32_t any = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= d[r];
  if (__ballot(any != 0) == 0) return;  // wave-uniform
  uint32_t mask = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) mask |= (__ballot(d[r] != 0) != 0 ? 1u : 0u) << r;
  const uint32_t first = static_cast<uint32_t>(__builtin_ctzll(__ballot(1)));
  if ((threadIdx.x & 63u) == first) {
    const uint32_t old = atomicOr(a.syndrome + s, mask);
    if (old == 0 && a.bad_count) atomicAdd(a.bad_count, 1u);
  }
}

// lsec_locate_dev (ec_kernels.h, LocateArgs).  The locate kernels are the check kernels over
// LocateArgs: the tile bodies below end in loc_*_wave instead of chk_publish.  The first vote is
// the check's, so a wave that saw no difference issues nothing; one that did takes the wave-uniform
// slow path: it forms the syndromes S_r = acc ^ stored parity in place (the tile's registers are
// dead after it), tests S_r == Q[r-1][j] * S_0 for every j < K over its lanes' words -- a
// run-time loop, so its code does not grow with K and its registers are the ones the inputs
// held -- and reduces each test with a vote into bit j of a mask that starts all ones.  A column
// with S_0 = 0 and some S_r != 0 fails every j by the same comparison.
template <typename Args>
__device__ __forceinline__ void loc_publish(const Args &a, uint32_t s, uint32_t rows, uint64_t hyp) {
  const uint32_t first = static_cast<uint32_t>(__builtin_ctzll(__ballot(1)));
  if ((threadIdx.x & 63u) == first) {
    atomicOr(a.syndrome + s, rows);
    if (hyp != ~0ull) atomicAnd(a.hyp + s, static_cast<unsigned long long>(hyp));  // (all ones: nothing to clear)
  }
}

template <int R>
__device__ __forceinline__ uint32_t loc_rows(const uint32_t (&d)[R]) {
  uint32_t rows = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) rows |= (__ballot(d[r] != 0) != 0 ? 1u : 0u) << r;
  return rows;
}

// bytewise: Q[r-1][j] * S_0 through the ratio cells' v_perm tables, as gf_mul_acc multiplies
template <int R, int IT, int VW, typename Args>
__device__ __forceinline__ void loc_bytewise_wave(const Args &a, uint32_t s, const uint32_t (&d)[R],
                                                  typename VecT<VW>::type (&acc)[IT][R],
                                                  const typename VecT<VW>::type (&pv)[R][IT]) {
  typedef typename VecT<VW>::type V;
  uint32_t any = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= d[r];
  if (__ballot(any != 0) == 0) return;  // wave-uniform
  const uint32_t rows = loc_rows<R>(d);
  V s0[IT], fa[IT], fb[IT], fc[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[it][r] ^= pv[r][it];
    s0[it] = acc[it][0];
  }
  bw_fields<IT, VW>(s0, fa, fb, fc);
  ConstCell *q = const_cells(a.ratio);
  const int K = a.K;
  uint64_t hyp = ~0ull;
#pragma unroll 1
  for (int j = 0; j < K; ++j) {
    uint32_t bad = 0;
#pragma unroll
    for (int r = 1; r < R; ++r) {
      ConstCell *c = q + (r - 1) * K + j;  // wave-uniform -> scalar loads
      const uint32_t t[6] = {c->ta_lo, c->ta_hi, c->tb_lo, c->tb_hi, c->tc_lo, c->tc_hi};
#pragma unroll
      for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int e = 0; e < VW; ++e) bad |= gf_mul_acc(acc[it][r][e], fa[it][e], fb[it][e], fc[it][e], t);
    }
    if (__ballot(bad != 0) != 0) hyp &= ~(1ull << j);
  }
  loc_publish(a, s, rows, hyp);
}

// bit-sliced: the kernel's doubling loop with S_0 as the input.  Rows r >= 1 hold
// T_r(j) = S_r ^ Q[r-1][j] * S_0 in place: T_r(j) = T_r(j-1) ^ (Q[r-1][j-1] ^ Q[r-1][j]) * S_0, with
// Q[r-1][-1] = 0, so a hypothesis costs one pass of the loop and no registers beside the doubled
// copy of S_0 -- the registers of the tile body's `e`.  AHEAD: the tile body kept the stored rows
// (pv) and acc holds the re-formed ones; else acc holds the syndromes already.
template <int R, int DW, bool AHEAD, typename Args>
__device__ __forceinline__ void loc_bitsliced_wave(const Args &a, uint32_t s, const uint32_t (&d)[R],
                                                   typename VecT<DW>::type (&acc)[R][8],
                                                   const typename VecT<DW>::type (&pv)[AHEAD ? R : 1][8]) {
  typedef typename VecT<DW>::type V;
  uint32_t any = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= d[r];
  if (__ballot(any != 0) == 0) return;  // wave-uniform
  const uint32_t rows = loc_rows<R>(d);
  if constexpr (AHEAD) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[r][x] ^= pv[r][x];
  }
  ConstCell *q = const_cells(a.ratio);
  const int K = a.K;
  uint64_t hyp = ~0ull;
  uint32_t prev[R];
#pragma unroll
  for (int r = 1; r < R; ++r) prev[r] = 0;
#pragma unroll 1
  for (int j = 0; j < K; ++j) {
    uint32_t c[R];
    uint32_t cm = 0;
#pragma unroll
    for (int r = 1; r < R; ++r) {
      const uint32_t cur = q[(r - 1) * K + j].coef;
      c[r] = prev[r] ^ cur;
      prev[r] = cur;
      cm |= c[r];
    }
    V e[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) e[x] = acc[0][x];
    gf8_sliced_mul_acc<1>(acc, e, c, cm);  // (c[0] is not read)
    V bad = 0u;
#pragma unroll
    for (int r = 1; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 8; ++x) bad |= acc[r][x];
    uint32_t b1 = 0;
#pragma unroll
    for (int w = 0; w < DW; ++w) b1 |= reinterpret_cast<const uint32_t *>(&bad)[w];
    if (__ballot(b1 != 0) != 0) hyp &= ~(1ull << j);
  }
  loc_publish(a, s, rows, hyp);
}

// The argument structs of the check's tile bodies: CheckArgs / LocateArgs, whose shards are the
// logical chunks, and CheckRotArgs / LocateRotArgs, whose shards are the physical devices of a
// rotated LUN; kLocArgs and kRotArgs tell them apart (ec_kernels.h).

// Where a tile of stripe s takes the ref of data chunk j / parity row r from: a.in[j] / a.par[r],
// or, rotated, sh[(j - rot_s) mod n] / sh[(K + r - rot_s) mod n] with rot_s worked out once per
// tile.  Everything here is uniform over the workgroup: scalar arithmetic and scalar loads only.
template <typename Args>
struct ChkShards {
  const Args &a;
  uint32_t back = 0;
  __device__ __forceinline__ ChkShards(const Args &a_, uint32_t s) : a(a_) {
    if constexpr (kRotArgs<Args>) back = rot_back(a, s);
  }
  __device__ __forceinline__ ShardRef in(int j) const {
    if constexpr (kRotArgs<Args>) return at(static_cast<uint32_t>(j));
    else return a.in[j];
  }
  __device__ __forceinline__ ShardRef par(int r) const {
    if constexpr (kRotArgs<Args>) return at(static_cast<uint32_t>(a.K + r));
    else return a.par[r];
  }

 private:
  __device__ __forceinline__ ShardRef at(uint32_t c) const {
    uint32_t i = c + back;
    if (i >= a.rot_n) i -= a.rot_n;
    return a.sh[i];
  }
};

// BF, X0, KC as bytewise_tiles.  A full tile with K fixed has its K*IT data loads and its R*IT
// parity loads in flight before any arithmetic (the parity rows cost R*IT*VW VGPRs more than the
// encode: 24 at RS(6+3)); with K at run time the parity loads go out ahead of the first four inputs.
// Args: CheckArgs, or LocateArgs for the locate kernels (the same tile body up to the last call);
// their rotated forms differ in ChkShards alone.
//
// MG (lsec_check_magic_dev / _rotated; Args: CheckMagicArgs, CheckMagicRotArgs): the tile also sums the
// stripe's adler32 magic over the k + m chunks it holds anyway.  One MagicLane takes every data unit
// as it is loaded and every stored parity unit pv[r], each at its LOGICAL chunk id (j, K + r: what
// ChkShards un-rotates), and the tile commits once through block_sum into a.magic_acc[2s], [2s + 1].
// block_sum has barriers: every lane of the workgroup reaches it, and there is no exit ahead of it
// (chk_publish's early return is its own).  Units past the end of a ragged tile read as zero and add
// nothing.  red: kBlock / 64 words of LDS.  Without MG red is not looked at and the code is the plain
// check's.
template <int R, int KC, int IT, bool BF, int VW, bool X0, bool MG = false, typename Args>
__device__ __forceinline__ void chk_bytewise_tiles(const Args &a, uint32_t *red = nullptr) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = KC ? KC : a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const ChkShards<Args> sh(a, s);
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform

    V acc[IT][R], pv[R][IT];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[it][r] = 0u;
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    if (full) {
      const auto addr = [&](int j) LSEC_INLINE {
        const ShardRef in = sh.in(j);
        return in.base + s * in.stride + off0;
      };
      const auto stored = [&]() LSEC_INLINE {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const ShardRef par = sh.par(r);
          const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
          for (int it = 0; it < IT; ++it) pv[r][it] = __builtin_nontemporal_load(gptr<V>(q + it * kStep));
        }
      };
      if constexpr (MG) {
        // by the registers of the fixed-K forms: summing an input ahead of its own pair
        // frees it early, which the wide forms need (R = 5, K = 20: 256 VGPRs and copies in AGPRs -> 168)
        // and the narrow two-step ones pay for (R = 3, K = 6: 123 -> 137, four waves per SIMD -> three)
        constexpr bool kEarly = BF && (R >= 4 || IT == 1);
        bw_inputs_seen<R, KC, IT, VW, BF, X0, kEarly>(
            acc, cells, K, true, addr,
            [&](int j, const V(&v)[IT]) LSEC_INLINE { ml_add<IT, VW>(ml, v, static_cast<uint32_t>(j)); }, stored);
      } else {
        bw_inputs<R, KC, IT, VW, BF, X0>(acc, cells, K, addr, stored);
      }
    } else {
      // ragged last tile: zero-filled inputs give zero parity there, and the stored parity is
      // zero-filled the same way, so bytes past C never show as a difference
      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.in(j);
        const uint64_t p = in.base + s * in.stride;
        V v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) v[it] = load_ragged<VW>(p, off0 + it * kStep, C);
        if constexpr (MG) ml_add<IT, VW>(ml, v, static_cast<uint32_t>(j));
        bw_acc1<R, IT, VW, BF, X0>(acc, v, cells, K, j);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) pv[r][it] = load_ragged<VW>(q, off0 + it * kStep, C);
      }
    }
    uint32_t d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      d[r] = 0;
#pragma unroll
      for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int e = 0; e < VW; ++e) d[r] = or_diff(acc[it][r][e], pv[r][it][e], d[r]);
    }
    if constexpr (kLocArgs<Args>) loc_bytewise_wave<R, IT, VW>(a, s, d, acc, pv);
    else chk_publish<R>(a, s, d);
    if constexpr (MG) {
      // the stored parity rows, as loaded (a ragged tile's units past C are zero)
#pragma unroll
      for (int r = 0; r < R; ++r) ml_add<IT, VW>(ml, pv[r], static_cast<uint32_t>(K + r));
      ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(C), static_cast<uint64_t>(off0), kStep, red);
    }
  }, a.tile_phase);
}

// the XOR-row flag picks one of two whole instantiations, by k_gf8_bytewise's rule
template <int R, int KC, int IT, bool BF, int VW, bool MG = false, typename Args>
__device__ __forceinline__ void chk_bytewise_body(const Args &a, uint32_t *red = nullptr) {
  if constexpr (BF && R >= 2 && (KC == 0 || KC * R >= 40)) {
    if (const_cells(a.cells)->pad & kCellXorRow) {
      chk_bytewise_tiles<R, KC, IT, BF, VW, true, MG>(a, red);
      return;
    }
  }
  chk_bytewise_tiles<R, KC, IT, BF, VW, false, MG>(a, red);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_chk_bytewise(CheckArgs a) {
  chk_bytewise_body<R, KC, IT, BF, VW>(a);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_loc_bytewise(LocateArgs a) {
  chk_bytewise_body<R, KC, IT, BF, VW>(a);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_chkrot_bytewise(CheckRotArgs a) {
  chk_bytewise_body<R, KC, IT, BF, VW>(a);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_locrot_bytewise(LocateRotArgs a) {
  chk_bytewise_body<R, KC, IT, BF, VW>(a);
}

// k_gf8_bitsliced's lanes and doubling loop.  The stored parity words are loaded ahead of the
// inputs while they fit beside the accumulators (R * DW <= 8: 8 * R * DW VGPRs), else row by row
// after them.  Lanes past the end of a ragged last tile leave the tile body (whole waves may).
// Args: as chk_bytewise_tiles.
// MG as in chk_bytewise_tiles: every e[x] of input j and every stored parity word go into the
// MagicLane (a row that shares pv[0] is summed before the next one overwrites it).  The lanes past
// the end of a ragged last tile then skip the loads and the vote under `valid`, but still join the
// tile's reduction (as pat_bitsliced_tiles' do).
template <int R, int DW, bool MG = false, typename Args>
__device__ __forceinline__ void chk_bitsliced_tiles(const Args &a, uint32_t *red = nullptr) {
  typedef typename VecT<DW>::type V;
  constexpr bool kAhead = R * DW <= 8;
  constexpr bool kLocate = kLocArgs<Args>;
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const ChkShards<Args> sh(a, s);
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    const bool valid = colb < col_bytes;
    if (!MG && !valid) return;  // (P % (4 * DW) == 0 keeps a lane's DW dwords inside one packet)
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    if (!MG || valid) {
      V acc[R][8], pv[kAhead ? R : 1][8];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[r][x] = 0u;
      if constexpr (kAhead) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const ShardRef par = sh.par(r);
          const uint64_t q = par.base + s * par.stride + off;
#pragma unroll
          for (int x = 0; x < 8; ++x) pv[r][x] = __builtin_nontemporal_load(gptr<V>(q + x * P));
        }
      }

      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.in(j);
        const uint64_t p = in.base + s * in.stride + off;
        V e[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) e[x] = __builtin_nontemporal_load(gptr<V>(p + x * P));
        if constexpr (MG) ml_add<8, DW>(ml, e, static_cast<uint32_t>(j));
        uint32_t c[R];
        uint32_t cm = 0;  // bits used by any output: no doublings past the highest one
#pragma unroll
        for (int r = 0; r < R; ++r) {
          c[r] = cells[r * K + j].coef;
          cm |= c[r];
        }
        gf8_sliced_mul_acc<0>(acc, e, c, cm);
      }
      uint32_t d[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if constexpr (!kAhead) {
          const ShardRef par = sh.par(r);
          const uint64_t q = par.base + s * par.stride + off;
#pragma unroll
          for (int x = 0; x < 8; ++x) pv[0][x] = __builtin_nontemporal_load(gptr<V>(q + x * P));
        }
        if constexpr (MG) ml_add<8, DW>(ml, pv[kAhead ? r : 0], static_cast<uint32_t>(K + r));  // (before pv[0] is loaded over)
        d[r] = 0;
        if constexpr (kLocate && !kAhead) {
          // the stored row is gone after this: keep the syndrome in the accumulator (one XOR and one
          // OR per word where the check has one v_bitop3)
#pragma unroll
          for (int x = 0; x < 8; ++x) {
            acc[r][x] ^= pv[0][x];
#pragma unroll
            for (int w = 0; w < DW; ++w) d[r] |= reinterpret_cast<const uint32_t *>(&acc[r][x])[w];
          }
        } else {
#pragma unroll
          for (int x = 0; x < 8; ++x)
#pragma unroll
            for (int w = 0; w < DW; ++w)
              d[r] = or_diff(reinterpret_cast<const uint32_t *>(&acc[r][x])[w],
                             reinterpret_cast<const uint32_t *>(&pv[kAhead ? r : 0][x])[w], d[r]);
        }
      }
      if constexpr (kLocate) loc_bitsliced_wave<R, DW, kAhead>(a, s, d, acc, pv);
      else chk_publish<R>(a, s, d);
    }
    if constexpr (MG) ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(a.size), static_cast<uint64_t>(off), P, red);
  }, a.tile_phase);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_chk_bitsliced(CheckArgs a) {
  chk_bitsliced_tiles<R, DW>(a);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_loc_bitsliced(LocateArgs a) {
  chk_bitsliced_tiles<R, DW>(a);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_chkrot_bitsliced(CheckRotArgs a) {
  chk_bitsliced_tiles<R, DW>(a);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_locrot_bitsliced(LocateRotArgs a) {
  chk_bitsliced_tiles<R, DW>(a);
}

// the MG kernels (lsec_check_magic_dev / _rotated): the same tile bodies, and the LDS of their reduction
template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_chkmagic_bytewise(CheckMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  chk_bytewise_body<R, KC, IT, BF, VW, true>(a, red);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_chkmagicrot_bytewise(CheckMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  chk_bytewise_body<R, KC, IT, BF, VW, true>(a, red);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_chkmagic_bitsliced(CheckMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  chk_bitsliced_tiles<R, DW, true>(a, red);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_chkmagicrot_bitsliced(CheckMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  chk_bitsliced_tiles<R, DW, true>(a, red);
}

// The check's launch shape is the encode's automatic one for the same K x R (bw_auto, without
// bytewise_shape's A/B variants), so tile sizes and vector widths match lsec_encode_dev's;
// fixed-K forms for the K the encode has them for.
// A fixed-K form holds K data units, R stored-parity units and R accumulators per step: past 160
// such dwords (RS(12+8) at 2 x 16 B: 224) it would fill the register file (256 VGPRs and copies in
// AGPRs), so those stripes run with K at run time, four inputs in flight at a time.
constexpr bool chk_fixed_k(int K, int R, int IT, int VW) { return (K + 2 * R) * IT * VW <= 160; }

// The bytewise form of a K x R check or locate: the fixed-K form where K has one and it fits, else
// K at run time in the automatic shape (R == 1: 8 B per lane, per-cell branches)
constexpr BwForm chk_bytewise_form(int K, int R) {
  const BwShape sh = bw_auto(K, R);
  if (has_fixed_k(K) && chk_fixed_k(K, R, sh.it, sh.vw)) return BwForm{K, sh.it, sh.vw, sh.bf};
  if (R == 1) return BwForm{0, 1, 2, false};
  return BwForm{0, sh.it == 1 ? 1 : 2, 4, true};
}

// The family and the __global__ functions of an argument struct: the check kernels of CheckArgs, the
// locate kernels of LocateArgs, the rotated forms of theirs.
template <typename Args>
struct ScrubKernels;
#define LSEC_SCRUB_KERNELS(ARGS, FAMILY, STEM)                      \
  template <>                                                       \
  struct ScrubKernels<ARGS> {                                       \
    static constexpr int family = FAMILY;                           \
    template <int R, int KC, int IT, bool BF, int VW>               \
    static auto bytewise() {                                        \
      return &k_##STEM##_bytewise<R, KC, IT, BF, VW>;               \
    }                                                               \
    template <int R, int DW>                                        \
    static auto bitsliced() {                                       \
      return &k_##STEM##_bitsliced<R, DW>;                          \
    }                                                               \
  };
LSEC_SCRUB_KERNELS(CheckArgs, kFormChk, chk)
LSEC_SCRUB_KERNELS(LocateArgs, kFormLoc, loc)
LSEC_SCRUB_KERNELS(CheckRotArgs, kFormChkRot, chkrot)
LSEC_SCRUB_KERNELS(LocateRotArgs, kFormLocRot, locrot)
LSEC_SCRUB_KERNELS(CheckMagicArgs, kFormChkMagic, chkmagic)
LSEC_SCRUB_KERNELS(CheckMagicRotArgs, kFormChkMagicRot, chkmagicrot)
#undef LSEC_SCRUB_KERNELS

// one kernel's launch, and its record (the template arguments are known here and nowhere later)
template <int R, int KC, int IT, bool BF, int VW, typename Args>
hipError_t scrub_bytewise_kernel(const Args &a, hipStream_t st, int grid) {
  record_launch({ScrubKernels<Args>::family, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(ScrubKernels<Args>::template bytewise<R, KC, IT, BF, VW>(), grid, st, a);
}

template <int R, int DW, typename Args>
hipError_t scrub_bitsliced_kernel(const Args &a, hipStream_t st, int grid) {
  record_launch({ScrubKernels<Args>::family, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(ScrubKernels<Args>::template bitsliced<R, DW>(), grid, st, a);
}

// The bytewise check or locate of R rows (a locate: R >= 2, one row cannot locate): decides the form
// (chk_bytewise_form), then switches on it.  A locate and the rotated forms take the check's shape.
template <int R, typename Args>
hipError_t dispatch_scrub_bytewise(const Args &a, hipStream_t st, int grid) {
  static_assert(!kLocArgs<Args> || R >= 2, "locating needs two parity rows");
  const BwForm f = chk_bytewise_form(a.K, R);
  switch (f.kc) {
#define LSEC_CHK_K(KK)                                                                          \
  case KK: {                                                                                    \
    constexpr BwForm ff = chk_bytewise_form(KK, R);                                             \
    if constexpr (ff.kc == KK)                                                                  \
      return scrub_bytewise_kernel<R, KK, ff.it, ff.bf, ff.vw>(a, st, grid);                   \
    break;                                                                                      \
  }
    LSEC_FIXED_K(LSEC_CHK_K)
#undef LSEC_CHK_K
    default: break;
  }
  if constexpr (R == 1) {
    return scrub_bytewise_kernel<1, 0, 1, false, 2>(a, st, grid);
  } else {
    if (f.it == 1) return scrub_bytewise_kernel<R, 0, 1, true, 4>(a, st, grid);
    return scrub_bytewise_kernel<R, 0, 2, true, 4>(a, st, grid);
  }
}

// Bit-sliced, dw dwords per lane.  A locate has more than one only up to kLocWideRows rows: the
// encode's policy asks for none wider (cauchy8_bitsliced_dw), and they would not fit the register
// file, so those forms do not exist.
constexpr int kLocWideRows = 4;
template <int R, typename Args>
hipError_t dispatch_scrub_bitsliced(const Args &a, hipStream_t st, int grid, int dw) {
  static_assert(!kLocArgs<Args> || R >= 2, "locating needs two parity rows");
  if constexpr (!kLocArgs<Args> || R <= kLocWideRows) {
    if (dw == 4) return scrub_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return scrub_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? scrub_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per argument struct and R in ec_scrub_inst.hip (the checks 1..8, the locates 2..8)
#define LSEC_DECLARE_SCRUB_R(ARGS, RR)                                                              \
  extern template hipError_t dispatch_scrub_bytewise<RR, ARGS>(const ARGS &, hipStream_t, int);     \
  extern template hipError_t dispatch_scrub_bitsliced<RR, ARGS>(const ARGS &, hipStream_t, int, int);
#define LSEC_DECLARE_SCRUB(ARGS)                                                                    \
  LSEC_DECLARE_SCRUB_R(ARGS, 2) LSEC_DECLARE_SCRUB_R(ARGS, 3) LSEC_DECLARE_SCRUB_R(ARGS, 4)        \
  LSEC_DECLARE_SCRUB_R(ARGS, 5) LSEC_DECLARE_SCRUB_R(ARGS, 6) LSEC_DECLARE_SCRUB_R(ARGS, 7) LSEC_DECLARE_SCRUB_R(ARGS, 8)
#ifndef LSEC_INSTANTIATING_SCRUB
LSEC_DECLARE_SCRUB_R(CheckArgs, 1) LSEC_DECLARE_SCRUB_R(CheckRotArgs, 1)
LSEC_DECLARE_SCRUB(CheckArgs) LSEC_DECLARE_SCRUB(LocateArgs) LSEC_DECLARE_SCRUB(CheckRotArgs) LSEC_DECLARE_SCRUB(LocateRotArgs)
#endif

// The MG forms (lsec_check_magic_dev / _rotated; DESIGN.md 3.8 has their registers): the check's own,
// through a constant of their own, so that one family can move without the other.
constexpr BwForm chkmagic_bytewise_form(int K, int R) { return chk_bytewise_form(K, R); }

// dispatch_scrub_bytewise over chkmagic_bytewise_form (Args: CheckMagicArgs or CheckMagicRotArgs)
template <int R, typename Args>
hipError_t dispatch_chkmagic_bytewise(const Args &a, hipStream_t st, int grid) {
  const BwForm f = chkmagic_bytewise_form(a.K, R);
  switch (f.kc) {
#define LSEC_CHKMAGIC_K(KK)                                                                     \
  case KK: {                                                                                    \
    constexpr BwForm ff = chkmagic_bytewise_form(KK, R);                                        \
    if constexpr (ff.kc == KK)                                                                  \
      return scrub_bytewise_kernel<R, KK, ff.it, ff.bf, ff.vw>(a, st, grid);                   \
    break;                                                                                      \
  }
    LSEC_FIXED_K(LSEC_CHKMAGIC_K)
#undef LSEC_CHKMAGIC_K
    default: break;
  }
  if constexpr (R == 1) {
    return scrub_bytewise_kernel<1, 0, 1, false, 2>(a, st, grid);
  } else {
    if (f.it == 1) return scrub_bytewise_kernel<R, 0, 1, true, 4>(a, st, grid);
    return scrub_bytewise_kernel<R, 0, 2, true, 4>(a, st, grid);
  }
}

// Bit-sliced, dw dwords per lane.  More than one only up to kChkMagicWideRows rows: the encode's policy
// asks for none wider (cauchy8_bitsliced_dw: R <= 4), and with the sums the 4-dword forms of 7 and 8 rows
// would pass the register file (8 bytes of scratch at R = 8), so those forms do not exist.
constexpr int kChkMagicWideRows = 6;
template <int R, typename Args>
hipError_t dispatch_chkmagic_bitsliced(const Args &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kChkMagicWideRows) {
    if (dw == 4) return scrub_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return scrub_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? scrub_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per argument struct and R in ec_scrub_magic_inst.hip
#define LSEC_DECLARE_CHKMAGIC_R(ARGS, RR)                                                              \
  extern template hipError_t dispatch_chkmagic_bytewise<RR, ARGS>(const ARGS &, hipStream_t, int);     \
  extern template hipError_t dispatch_chkmagic_bitsliced<RR, ARGS>(const ARGS &, hipStream_t, int, int);
#define LSEC_DECLARE_CHKMAGIC(ARGS)                                                                    \
  LSEC_DECLARE_CHKMAGIC_R(ARGS, 1) LSEC_DECLARE_CHKMAGIC_R(ARGS, 2) LSEC_DECLARE_CHKMAGIC_R(ARGS, 3)   \
  LSEC_DECLARE_CHKMAGIC_R(ARGS, 4) LSEC_DECLARE_CHKMAGIC_R(ARGS, 5) LSEC_DECLARE_CHKMAGIC_R(ARGS, 6)   \
  LSEC_DECLARE_CHKMAGIC_R(ARGS, 7) LSEC_DECLARE_CHKMAGIC_R(ARGS, 8)
#ifndef LSEC_INSTANTIATING_CHKMAGIC
LSEC_DECLARE_CHKMAGIC(CheckMagicArgs) LSEC_DECLARE_CHKMAGIC(CheckMagicRotArgs)
#endif

// ------------------------------------------------------------------ parity update
// lsec_update_dev (ec_kernels.h, UpdateArgs): parity_r ^= sum_i g[r][col[i]] * (old_i ^ fresh_i) over
// the c changed data chunks of a stripe.  The tile loop, the lanes and the arithmetic are the
// encode's; the accumulators start as the stored parity rows instead of zero, so those loads go out
// ahead of the columns' and nothing but the accumulators holds them.  old_i ^ fresh_i is formed once
// per column and multiplied once per row; its cell is cells[r * K + col[i]], col[i] from the kernel
// arguments and so uniform over the wave (a scalar load, as the patterned decode's cells).  With
// UpdateArgs::store the fresh units, already in registers, go over the old ones.  One lane reads
// and writes each byte of a tile: no atomics, no LDS, no cross-lane traffic.

// col[i] of the call (i uniform over the workgroup): the byte out of its aligned word of the arguments
__device__ __forceinline__ uint32_t upd_col(const UpdateArgs &a, int i) {
  uint32_t w;
  __builtin_memcpy(&w, a.col + (i & ~3), 4);
  return (w >> (8 * (i & 3))) & 0xFFu;
}

// BF as k_gf8_bytewise: the branch-free coefficient path, or per-cell branches (R = 1).  Row 0's
// all-ones flag is not used: the tables of coefficient 1 give the same bytes.
template <int R, int IT, int VW, bool BF>
__device__ __forceinline__ void upd_bytewise_tiles(const UpdateArgs &a) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform

    V acc[IT][R];
    if (full) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.par[r].base + s * a.par[r].stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = __builtin_nontemporal_load(gptr<V>(q + it * kStep));
      }
      for (int i = 0; i < a.c; ++i) {
        const ShardRef old = a.old[i], fresh = a.fresh[i];
        const uint64_t po = old.base + s * old.stride + off0, pf = fresh.base + s * fresh.stride + off0;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = __builtin_nontemporal_load(gptr<V>(po + it * kStep));
          f[it] = __builtin_nontemporal_load(gptr<V>(pf + it * kStep));
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) put_nt<false, V>(po + it * kStep, f[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(upd_col(a, i)));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.par[r].base + s * a.par[r].stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) put_nt<false, V>(q + it * kStep, acc[it][r]);
      }
    } else {
      // ragged last tile: units past C read as zero and are not stored, a half unit moves 8 bytes
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.par[r].base + s * a.par[r].stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = load_ragged<VW>(q, off0 + it * kStep, C);
      }
      for (int i = 0; i < a.c; ++i) {
        const ShardRef old = a.old[i], fresh = a.fresh[i];
        const uint64_t po = old.base + s * old.stride, pf = fresh.base + s * fresh.stride;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = load_ragged<VW>(po, off0 + it * kStep, C);
          f[it] = load_ragged<VW>(pf, off0 + it * kStep, C);
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) store_ragged<false, VW>(po, off0 + it * kStep, C, f[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(upd_col(a, i)));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t q = a.par[r].base + s * a.par[r].stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) store_ragged<false, VW>(q, off0 + it * kStep, C, acc[it][r]);
      }
    }
  }, a.tile_phase);
}

template <int R, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_upd_bytewise(UpdateArgs a) {
  upd_bytewise_tiles<R, IT, VW, BF>(a);
}

// k_gf8_bitsliced's lanes and doubling loop over old_i ^ fresh_i, the accumulators starting as the
// 8 * R stored parity words.  Lanes past the end of a ragged last tile leave the tile body.
template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_upd_bitsliced(UpdateArgs a) {
  typedef typename VecT<DW>::type V;
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    if (colb >= col_bytes) return;  // (P % (4 * DW) == 0 keeps a lane's DW dwords inside one packet)
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);

    V acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t q = a.par[r].base + s * a.par[r].stride + off;
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[r][x] = __builtin_nontemporal_load(gptr<V>(q + x * P));
    }
    for (int i = 0; i < a.c; ++i) {
      const ShardRef old = a.old[i], fresh = a.fresh[i];
      const uint64_t po = old.base + s * old.stride + off, pf = fresh.base + s * fresh.stride + off;
      V e[8], f[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        e[x] = __builtin_nontemporal_load(gptr<V>(po + x * P));
        f[x] = __builtin_nontemporal_load(gptr<V>(pf + x * P));
      }
      if (store) {
#pragma unroll
        for (int x = 0; x < 8; ++x) put_nt<false, V>(po + x * P, f[x]);
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) e[x] ^= f[x];
      const uint32_t j = upd_col(a, i);
      uint32_t c[R];
      uint32_t cm = 0;  // bits used by any row: no doublings past the highest one
#pragma unroll
      for (int r = 0; r < R; ++r) {
        c[r] = cells[r * K + j].coef;
        cm |= c[r];
      }
      gf8_sliced_mul_acc<0>(acc, e, c, cm);
    }
    // The stores go to the addresses the parity loads came from.  Kept from there to here they are
    // 16 * R VGPRs, more than the accumulators at one dword per lane (R = 8: 236 VGPRs, 2 waves per
    // SIMD); formed again from an offset the compiler cannot see through, they cost two adds each.
    int64_t off_st = off;
    asm volatile("" : "+v"(off_st));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t q = a.par[r].base + s * a.par[r].stride + off_st;
#pragma unroll
      for (int x = 0; x < 8; ++x) put_nt<false, V>(q + x * P, acc[r][x]);
    }
  }, a.tile_phase);
}

// The forms (DESIGN.md 3.6 has their registers).  Bytewise: one per R, the changed columns at run
// time -- one row in the one-row shape of the other kernels (8 B per lane, per-cell branches), two or
// more branch-free in 16-byte units, two per lane up to kUpdTwoStepRows rows and one beyond, where a
// second unit's accumulators would cost a wave of occupancy.  Bit-sliced: 1, 2 or 4 dwords per lane up
// to kUpdWideRows rows, as the locate (the encode's policy asks for none wider), else one.
constexpr int kUpdTwoStepRows = 4;
constexpr int kUpdWideRows = kLocWideRows;
constexpr BwForm upd_bytewise_form(int R) {
  if (R == 1) return BwForm{0, 1, 2, false};
  return BwForm{0, R <= kUpdTwoStepRows ? 2 : 1, 4, true};
}

template <int R>
hipError_t dispatch_upd_bytewise(const UpdateArgs &a, hipStream_t st, int grid) {
  constexpr BwForm f = upd_bytewise_form(R);
  record_launch({kFormUpd, 0, R, f.kc, f.it, f.vw, f.bf ? 1 : 0, 0});
  return launch_tiled(&k_upd_bytewise<R, f.it, f.vw, f.bf>, grid, st, a);
}

template <int R, int DW>
hipError_t upd_bitsliced_kernel(const UpdateArgs &a, hipStream_t st, int grid) {
  record_launch({kFormUpd, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_upd_bitsliced<R, DW>, grid, st, a);
}

template <int R>
hipError_t dispatch_upd_bitsliced(const UpdateArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kUpdWideRows) {
    if (dw == 4) return upd_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return upd_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? upd_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_update_inst.hip
#define LSEC_DECLARE_UPD_R(RR)                                                                \
  extern template hipError_t dispatch_upd_bytewise<RR>(const UpdateArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_upd_bitsliced<RR>(const UpdateArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_UPD
LSEC_DECLARE_UPD_R(1) LSEC_DECLARE_UPD_R(2) LSEC_DECLARE_UPD_R(3) LSEC_DECLARE_UPD_R(4)
LSEC_DECLARE_UPD_R(5) LSEC_DECLARE_UPD_R(6) LSEC_DECLARE_UPD_R(7) LSEC_DECLARE_UPD_R(8)
#endif

// lsec_update_dev_rotated (ec_kernels.h, UpdateRotArgs): the update over the K + R physical devices
// of a rotated LUN, in the update's own forms.
__device__ __forceinline__ uint32_t upd_col(const UpdateRotArgs &a, int i) {
  uint32_t w;
  __builtin_memcpy(&w, a.col + (i & ~3), 4);
  return (w >> (8 * (i & 3))) & 0xFFu;
}

// Where a tile of stripe s takes the ref of changed chunk i as stored / parity row r from:
// sh[(col[i] - rot_s) mod n] / sh[(K + r - rot_s) mod n], by the rotated check's ChkShards.
struct UpdShards {
  const UpdateRotArgs &a;
  const ChkShards<UpdateRotArgs> sh;
  __device__ __forceinline__ UpdShards(const UpdateRotArgs &a_, uint32_t s) : a(a_), sh(a_, s) {}
  __device__ __forceinline__ ShardRef old(int i) const { return sh.in(static_cast<int>(upd_col(a, i))); }
  __device__ __forceinline__ ShardRef par(int r) const { return sh.par(r); }
};

// upd_bytewise_tiles over the devices of a rotated LUN: a second body, differing in where a tile takes
// its refs from (UpdShards).  (Shared with the unrotated kernels through a template parameter, the
// body moved the code of some of their instantiations; their objects are to stay as they are.)
template <int R, int IT, int VW, bool BF>
__device__ __forceinline__ void updrot_bytewise_tiles(const UpdateRotArgs &a) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const UpdShards sh(a, s);
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform

    V acc[IT][R];
    if (full) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = __builtin_nontemporal_load(gptr<V>(q + it * kStep));
      }
      for (int i = 0; i < a.c; ++i) {
        const ShardRef old = sh.old(i), fresh = a.fresh[i];
        const uint64_t po = old.base + s * old.stride + off0, pf = fresh.base + s * fresh.stride + off0;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = __builtin_nontemporal_load(gptr<V>(po + it * kStep));
          f[it] = __builtin_nontemporal_load(gptr<V>(pf + it * kStep));
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) put_nt<false, V>(po + it * kStep, f[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(upd_col(a, i)));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) put_nt<false, V>(q + it * kStep, acc[it][r]);
      }
    } else {
      // ragged last tile: units past C read as zero and are not stored, a half unit moves 8 bytes
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = load_ragged<VW>(q, off0 + it * kStep, C);
      }
      for (int i = 0; i < a.c; ++i) {
        const ShardRef old = sh.old(i), fresh = a.fresh[i];
        const uint64_t po = old.base + s * old.stride, pf = fresh.base + s * fresh.stride;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = load_ragged<VW>(po, off0 + it * kStep, C);
          f[it] = load_ragged<VW>(pf, off0 + it * kStep, C);
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) store_ragged<false, VW>(po, off0 + it * kStep, C, f[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(upd_col(a, i)));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) store_ragged<false, VW>(q, off0 + it * kStep, C, acc[it][r]);
      }
    }
  }, a.tile_phase);
}

template <int R, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_updrot_bytewise(UpdateRotArgs a) {
  updrot_bytewise_tiles<R, IT, VW, BF>(a);
}

// k_upd_bitsliced over the devices of a rotated LUN, a second body as updrot_bytewise_tiles is.
template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_updrot_bitsliced(UpdateRotArgs a) {
  typedef typename VecT<DW>::type V;
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const UpdShards sh(a, s);
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    if (colb >= col_bytes) return;  // (P % (4 * DW) == 0 keeps a lane's DW dwords inside one packet)
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);

    V acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const ShardRef par = sh.par(r);
      const uint64_t q = par.base + s * par.stride + off;
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[r][x] = __builtin_nontemporal_load(gptr<V>(q + x * P));
    }
    for (int i = 0; i < a.c; ++i) {
      const ShardRef old = sh.old(i), fresh = a.fresh[i];
      const uint64_t po = old.base + s * old.stride + off, pf = fresh.base + s * fresh.stride + off;
      V e[8], f[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        e[x] = __builtin_nontemporal_load(gptr<V>(po + x * P));
        f[x] = __builtin_nontemporal_load(gptr<V>(pf + x * P));
      }
      if (store) {
#pragma unroll
        for (int x = 0; x < 8; ++x) put_nt<false, V>(po + x * P, f[x]);
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) e[x] ^= f[x];
      const uint32_t j = upd_col(a, i);
      uint32_t c[R];
      uint32_t cm = 0;  // bits used by any row: no doublings past the highest one
#pragma unroll
      for (int r = 0; r < R; ++r) {
        c[r] = cells[r * K + j].coef;
        cm |= c[r];
      }
      gf8_sliced_mul_acc<0>(acc, e, c, cm);
    }
    // The stores go to the addresses the parity loads came from.  Kept from there to here they are
    // 16 * R VGPRs, more than the accumulators at one dword per lane (R = 8: 236 VGPRs, 2 waves per
    // SIMD); formed again from an offset the compiler cannot see through, they cost two adds each.
    int64_t off_st = off;
    asm volatile("" : "+v"(off_st));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const ShardRef par = sh.par(r);
      const uint64_t q = par.base + s * par.stride + off_st;
#pragma unroll
      for (int x = 0; x < 8; ++x) put_nt<false, V>(q + x * P, acc[r][x]);
    }
  }, a.tile_phase);
}

template <int R>
hipError_t dispatch_updrot_bytewise(const UpdateRotArgs &a, hipStream_t st, int grid) {
  constexpr BwForm f = upd_bytewise_form(R);
  record_launch({kFormUpdRot, 0, R, f.kc, f.it, f.vw, f.bf ? 1 : 0, 0});
  return launch_tiled(&k_updrot_bytewise<R, f.it, f.vw, f.bf>, grid, st, a);
}

template <int R, int DW>
hipError_t updrot_bitsliced_kernel(const UpdateRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormUpdRot, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_updrot_bitsliced<R, DW>, grid, st, a);
}

template <int R>
hipError_t dispatch_updrot_bitsliced(const UpdateRotArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kUpdWideRows) {
    if (dw == 4) return updrot_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return updrot_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? updrot_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_update_rot_inst.hip
#define LSEC_DECLARE_UPDROT_R(RR)                                                                   \
  extern template hipError_t dispatch_updrot_bytewise<RR>(const UpdateRotArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_updrot_bitsliced<RR>(const UpdateRotArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_UPDROT
LSEC_DECLARE_UPDROT_R(1) LSEC_DECLARE_UPDROT_R(2) LSEC_DECLARE_UPDROT_R(3) LSEC_DECLARE_UPDROT_R(4)
LSEC_DECLARE_UPDROT_R(5) LSEC_DECLARE_UPDROT_R(6) LSEC_DECLARE_UPDROT_R(7) LSEC_DECLARE_UPDROT_R(8)
#endif

// ------------------------------------------------------------------ parity update, a changed set per stripe
// lsec_update_dev_masked / _masked_rotated (ec_kernels.h, UpdateMaskArgs): the update's tile bodies
// with the column loop replaced by a walk over the set bits of the stripe's mask word.  The stripe is
// uniform over the workgroup, so the word is read through a uniform address and made scalar; ANDed
// with `allowed` it is the stripe's effective mask.  A tile of a stripe whose effective mask is 0
// leaves the tile body before any other load.  Otherwise the bits are taken lowest first (find
// first set, clear it): bit j loads the lane's units of old_j and fresh_j, stores fresh over old
// under the launch-uniform flag, XORs the two once and multiplies once per row with
// cells[r * K + j], a scalar load.  The refs are the rotated update's (sh, rot_back once per tile);
// the unrotated call has rot_step = 0.  No atomics, no LDS, no cross-lane traffic.

// the effective mask of stripe s (s uniform over the workgroup): scalar
__device__ __forceinline__ uint64_t updmask_word(const UpdateMaskArgs &a, uint32_t s) {
  const uint64_t w = *gptr<uint64_t>(reinterpret_cast<uint64_t>(a.stripe_cols) + 8ull * s);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w >> 32));
  return ((static_cast<uint64_t>(hi) << 32) | lo) & a.allowed;
}

// Where a tile of stripe s takes the ref of data chunk j / parity row r from: sh[(j - rot_s) mod n] /
// sh[(K + r - rot_s) mod n], as ChkShards over a rotated struct.
struct UpdMaskShards {
  const UpdateMaskArgs &a;
  const uint32_t back;
  __device__ __forceinline__ UpdMaskShards(const UpdateMaskArgs &a_, uint32_t s) : a(a_), back(rot_back(a_, s)) {}
  __device__ __forceinline__ ShardRef old(uint32_t j) const { return at(j); }
  __device__ __forceinline__ ShardRef par(int r) const { return at(static_cast<uint32_t>(a.K + r)); }

 private:
  __device__ __forceinline__ ShardRef at(uint32_t c) const {
    uint32_t i = c + back;
    if (i >= a.rot_n) i -= a.rot_n;
    return a.sh[i];
  }
};

// BF as k_gf8_bytewise: the branch-free coefficient path, or per-cell branches (R = 1).
//
// MG (lsec_update_magic_dev_masked / _rotated): the tile also sums what the write does to the stripe's
// adler32 magic.  The changed positions are the changed data chunks and the R parity rows, and the lane
// holds both sides of every one of them: the stored parity units as loaded and the accumulators as
// stored, old_j and fresh_j before they are XORed.  One MagicLane takes new minus old (ml_add / ml_sub)
// at the LOGICAL shard index, j or K + r -- the rotation moves addresses, not positions -- and the
// tile commits once through block_sum into macc[2s], macc[2s + 1] (ml_commit_delta).  block_sum has
// barriers: every lane of the workgroup reaches it.  The mask == 0 exit is uniform; units past the end
// of a ragged tile read as zero and add nothing.  red: kBlock / 64 words of LDS.  Without MG macc and
// red are not looked at and the code is the plain masked update's.
template <int R, int IT, int VW, bool BF, bool MG = false>
__device__ __forceinline__ void updmask_bytewise_tiles(const UpdateMaskArgs &a, unsigned long long *macc = nullptr,
                                                       uint32_t *red = nullptr) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    uint64_t mask = updmask_word(a, s);
    if (mask == 0) return;  // nothing of this stripe changes: neither read nor written
    const UpdMaskShards sh(a, s);
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform
    MagicLane ml;  // new minus old of the stripe magic (MG only)

    V acc[IT][R];
    if (full) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = __builtin_nontemporal_load(gptr<V>(q + it * kStep));
      }
      if constexpr (MG) bw_magic_out<R, IT, VW, true>(ml, K, acc);
      do {
        const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(mask));
        mask &= mask - 1;
        const ShardRef old = sh.old(j), fresh = a.fresh[j];
        const uint64_t po = old.base + s * old.stride + off0, pf = fresh.base + s * fresh.stride + off0;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = __builtin_nontemporal_load(gptr<V>(po + it * kStep));
          f[it] = __builtin_nontemporal_load(gptr<V>(pf + it * kStep));
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) put_nt<false, V>(po + it * kStep, f[it]);
        }
        if constexpr (MG) {
          ml_sub<IT, VW>(ml, d, j);
          ml_add<IT, VW>(ml, f, j);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(j));
      } while (mask);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) put_nt<false, V>(q + it * kStep, acc[it][r]);
      }
    } else {
      // ragged last tile: units past C read as zero and are not stored, a half unit moves 8 bytes
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) acc[it][r] = load_ragged<VW>(q, off0 + it * kStep, C);
      }
      if constexpr (MG) bw_magic_out<R, IT, VW, true>(ml, K, acc);
      do {
        const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(mask));
        mask &= mask - 1;
        const ShardRef old = sh.old(j), fresh = a.fresh[j];
        const uint64_t po = old.base + s * old.stride, pf = fresh.base + s * fresh.stride;
        V d[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          d[it] = load_ragged<VW>(po, off0 + it * kStep, C);
          f[it] = load_ragged<VW>(pf, off0 + it * kStep, C);
        }
        if (store) {
#pragma unroll
          for (int it = 0; it < IT; ++it) store_ragged<false, VW>(po, off0 + it * kStep, C, f[it]);
        }
        if constexpr (MG) {
          ml_sub<IT, VW>(ml, d, j);
          ml_add<IT, VW>(ml, f, j);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) d[it] ^= f[it];
        bw_acc1<R, IT, VW, BF, false>(acc, d, cells, K, static_cast<int>(j));
      } while (mask);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) store_ragged<false, VW>(q, off0 + it * kStep, C, acc[it][r]);
      }
    }
    if constexpr (MG) {
      bw_magic_out<R, IT, VW>(ml, K, acc);
      ml_commit_delta(ml, macc, s, K + R, C, off0, kStep, red);
    }
  }, a.tile_phase);
}

template <int R, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_updmask_bytewise(UpdateMaskArgs a) {
  updmask_bytewise_tiles<R, IT, VW, BF>(a);
}

template <int R, int IT, int VW, bool BF>
__global__ __launch_bounds__(kBlock) void k_updmagic_bytewise(UpdateMaskMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  updmask_bytewise_tiles<R, IT, VW, BF, true>(a, a.magic_acc, red);
}

// k_upd_bitsliced's lanes and doubling loop under the stripe's mask.  The mask is looked at first;
// lanes past the end of a ragged last tile leave the tile body behind that.  MG as in
// updmask_bytewise_tiles: those lanes then skip the loads and stores, but still join the tile's
// reduction (as k_gf8_bitsliced's do).
template <int R, int DW, bool MG = false>
__device__ __forceinline__ void updmask_bitsliced_tiles(const UpdateMaskArgs &a, unsigned long long *macc = nullptr,
                                                        uint32_t *red = nullptr) {
  typedef typename VecT<DW>::type V;
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);
  const bool store = a.store != 0;  // uniform over the launch

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    uint64_t mask = updmask_word(a, s);
    if (mask == 0) return;  // nothing of this stripe changes: neither read nor written
    const UpdMaskShards sh(a, s);
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    const bool valid = colb < col_bytes;  // (P % (4 * DW) == 0 keeps a lane's DW dwords inside one packet)
    if (!MG && !valid) return;
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);
    MagicLane ml;  // new minus old of the stripe magic (MG only)

    if (!MG || valid) {
      V acc[R][8];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[r][x] = __builtin_nontemporal_load(gptr<V>(q + x * P));
        if constexpr (MG) ml_sub<8, DW>(ml, acc[r], static_cast<uint32_t>(K + r));
      }
      do {
        const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(mask));
        mask &= mask - 1;
        const ShardRef old = sh.old(j), fresh = a.fresh[j];
        const uint64_t po = old.base + s * old.stride + off, pf = fresh.base + s * fresh.stride + off;
        V e[8], f[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          e[x] = __builtin_nontemporal_load(gptr<V>(po + x * P));
          f[x] = __builtin_nontemporal_load(gptr<V>(pf + x * P));
        }
        if (store) {
#pragma unroll
          for (int x = 0; x < 8; ++x) put_nt<false, V>(po + x * P, f[x]);
        }
        if constexpr (MG) {
          ml_sub<8, DW>(ml, e, j);
          ml_add<8, DW>(ml, f, j);
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) e[x] ^= f[x];
        uint32_t c[R];
        uint32_t cm = 0;  // bits used by any row: no doublings past the highest one
#pragma unroll
        for (int r = 0; r < R; ++r) {
          c[r] = cells[r * K + j].coef;
          cm |= c[r];
        }
        gf8_sliced_mul_acc<0>(acc, e, c, cm);
      } while (mask);
      // the stores go to the addresses the parity loads came from, formed again (k_upd_bitsliced)
      int64_t off_st = off;
      asm volatile("" : "+v"(off_st));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off_st;
#pragma unroll
        for (int x = 0; x < 8; ++x) put_nt<false, V>(q + x * P, acc[r][x]);
        if constexpr (MG) ml_add<8, DW>(ml, acc[r], static_cast<uint32_t>(K + r));
      }
    }
    if constexpr (MG) ml_commit_delta(ml, macc, s, K + R, a.size, off, P, red);
  }, a.tile_phase);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_updmask_bitsliced(UpdateMaskArgs a) {
  updmask_bitsliced_tiles<R, DW>(a);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_updmagic_bitsliced(UpdateMaskMagicArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  updmask_bitsliced_tiles<R, DW, true>(a, a.magic_acc, red);
}

// The forms (DESIGN.md 3.6 has their registers): the update's, which depend on R alone.
constexpr BwForm updmask_bytewise_form(int R) { return upd_bytewise_form(R); }
constexpr int kUpdMaskWideRows = kUpdWideRows;

template <int R>
hipError_t dispatch_updmask_bytewise(const UpdateMaskArgs &a, hipStream_t st, int grid) {
  constexpr BwForm f = updmask_bytewise_form(R);
  record_launch({kFormUpdMask, 0, R, f.kc, f.it, f.vw, f.bf ? 1 : 0, 0});
  return launch_tiled(&k_updmask_bytewise<R, f.it, f.vw, f.bf>, grid, st, a);
}

template <int R, int DW>
hipError_t updmask_bitsliced_kernel(const UpdateMaskArgs &a, hipStream_t st, int grid) {
  record_launch({kFormUpdMask, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_updmask_bitsliced<R, DW>, grid, st, a);
}

template <int R>
hipError_t dispatch_updmask_bitsliced(const UpdateMaskArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kUpdMaskWideRows) {
    if (dw == 4) return updmask_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return updmask_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? updmask_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_update_masked_inst.hip
#define LSEC_DECLARE_UPDMASK_R(RR)                                                                    \
  extern template hipError_t dispatch_updmask_bytewise<RR>(const UpdateMaskArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_updmask_bitsliced<RR>(const UpdateMaskArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_UPDMASK
LSEC_DECLARE_UPDMASK_R(1) LSEC_DECLARE_UPDMASK_R(2) LSEC_DECLARE_UPDMASK_R(3) LSEC_DECLARE_UPDMASK_R(4)
LSEC_DECLARE_UPDMASK_R(5) LSEC_DECLARE_UPDMASK_R(6) LSEC_DECLARE_UPDMASK_R(7) LSEC_DECLARE_UPDMASK_R(8)
#endif

// The MG forms (lsec_update_magic_dev_masked / _rotated; DESIGN.md 3.6 has their registers): the masked
// update's own.  None of them uses scratch at those shapes -- the widest, <4, 4>, takes 244 VGPRs -- so
// they were kept; constants of their own, so that one family can move without the other.
constexpr BwForm updmagic_bytewise_form(int R) { return updmask_bytewise_form(R); }
constexpr int kUpdMagicWideRows = kUpdMaskWideRows;

template <int R>
hipError_t dispatch_updmagic_bytewise(const UpdateMaskMagicArgs &a, hipStream_t st, int grid) {
  constexpr BwForm f = updmagic_bytewise_form(R);
  record_launch({kFormUpdMaskMagic, 0, R, f.kc, f.it, f.vw, f.bf ? 1 : 0, 0});
  return launch_tiled(&k_updmagic_bytewise<R, f.it, f.vw, f.bf>, grid, st, a);
}

template <int R, int DW>
hipError_t updmagic_bitsliced_kernel(const UpdateMaskMagicArgs &a, hipStream_t st, int grid) {
  record_launch({kFormUpdMaskMagic, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_updmagic_bitsliced<R, DW>, grid, st, a);
}

template <int R>
hipError_t dispatch_updmagic_bitsliced(const UpdateMaskMagicArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kUpdMagicWideRows) {
    if (dw == 4) return updmagic_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return updmagic_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? updmagic_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_update_magic_inst.hip
#define LSEC_DECLARE_UPDMAGIC_R(RR)                                                                         \
  extern template hipError_t dispatch_updmagic_bytewise<RR>(const UpdateMaskMagicArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_updmagic_bitsliced<RR>(const UpdateMaskMagicArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_UPDMAGIC
LSEC_DECLARE_UPDMAGIC_R(1) LSEC_DECLARE_UPDMAGIC_R(2) LSEC_DECLARE_UPDMAGIC_R(3) LSEC_DECLARE_UPDMAGIC_R(4)
LSEC_DECLARE_UPDMAGIC_R(5) LSEC_DECLARE_UPDMAGIC_R(6) LSEC_DECLARE_UPDMAGIC_R(7) LSEC_DECLARE_UPDMAGIC_R(8)
#endif

// ------------------------------------------------------------------ encode over a rotated LUN
// lsec_encode_dev_rotated (ec_kernels.h, EncodeRotArgs): the rotated check's tile bodies -- its
// tile loop, its rotated input addresses (ChkShards), bw_inputs / bw_acc1, the bit-sliced lanes and
// doubling loop -- with the accumulators stored to the devices that hold the stripe's parity rows
// where the check loads the stored rows and compares.  No stored-parity registers (the check's pv),
// no votes, no atomics.
//
// MG (lsec_encode_magic_dev_rotated; Args: EncodeMagicRotArgs): the tile also sums the stripe's adler32
// magic over the k + m chunks it holds anyway.  One MagicLane takes every data unit as it is loaded and
// every row acc[.][r] as it is stored, each at its LOGICAL chunk id (j, K + r: what ChkShards
// un-rotates), and the tile commits once through block_sum into a.magic_acc[2s], [2s + 1].  block_sum
// has barriers: every lane of the workgroup reaches it, and the MG forms have no exit ahead of it.
// red: kBlock / 64 words of LDS.  Without MG red is not looked at and the code is the plain encode's.

// Whether a fixed-K MG tile sums an input ahead of its own pair's arithmetic (bw_inputs_seen's EARLY) or
// all of them behind everybody's: by the registers of the fixed-K forms.  With one step
// per lane the early order frees each input with its pair and never costs a wave (R = 3, K = 16: 96
// VGPRs against 121, five waves per SIMD against four); with two steps the late order is the smaller
// one (R = 5, K = 6: 157 against 215, three waves against two) at every form but R = 4 and 5 at K = 4,
// where it costs four VGPRs and no wave.  The encode has no stored rows beside its accumulators, so the
// MG check's R >= 4 rule does not carry over.  No form of either order spills.
constexpr bool encmagicrot_early(int IT, bool BF) { return BF && IT == 1; }

// BF, X0, KC as chk_bytewise_tiles.  Args: EncodeRotArgs, or EncodeMagicRotArgs with MG.
template <int R, int KC, int IT, bool BF, int VW, bool X0, bool MG = false, typename Args>
__device__ __forceinline__ void encrot_bytewise_tiles(const Args &a, uint32_t *red = nullptr) {
  typedef typename VecT<VW>::type V;
  constexpr int kStep = BwTile<IT, VW>::kStep;
  constexpr int kTile = BwTile<IT, VW>::kBytes;
  constexpr int kLane = 4 * VW;
  const int K = KC ? KC : a.K;
  const int64_t C = a.size;
  const uint32_t tiles_per_stripe = static_cast<uint32_t>((C + kTile - 1) / kTile);
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  for_tiles<(kTile >= 8192 ? 1 : 8192 / kTile)>(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const ChkShards<Args> sh(a, s);
    const int64_t off0 = static_cast<int64_t>(t - s * tiles_per_stripe) * kTile + threadIdx.x * kLane;
    const bool full = (static_cast<int64_t>(t - s * tiles_per_stripe) + 1) * kTile <= C;  // wave-uniform

    V acc[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[it][r] = 0u;
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    if (full) {
      const auto addr = [&](int j) LSEC_INLINE {
        const ShardRef in = sh.in(j);
        return in.base + s * in.stride + off0;
      };
      if constexpr (MG) {
        // early or late by the registers of the fixed-K forms, as the MG check picks
        bw_inputs_seen<R, KC, IT, VW, BF, X0, encmagicrot_early(IT, BF)>(
            acc, cells, K, true, addr,
            [&](int j, const V(&v)[IT]) LSEC_INLINE { ml_add<IT, VW>(ml, v, static_cast<uint32_t>(j)); });
      } else {
        bw_inputs<R, KC, IT, VW, BF, X0>(acc, cells, K, addr, NoLoads());
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off0;
#pragma unroll
        for (int it = 0; it < IT; ++it) put_nt<false, V>(q + it * kStep, acc[it][r]);
      }
    } else {
      // ragged last tile: units past C read as zero and are not stored, a half unit moves 8 bytes
      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.in(j);
        const uint64_t p = in.base + s * in.stride;
        V v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) v[it] = load_ragged<VW>(p, off0 + it * kStep, C);
        if constexpr (MG) ml_add<IT, VW>(ml, v, static_cast<uint32_t>(j));
        bw_acc1<R, IT, VW, BF, X0>(acc, v, cells, K, j);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride;
#pragma unroll
        for (int it = 0; it < IT; ++it) store_ragged<false, VW>(q, off0 + it * kStep, C, acc[it][r]);
      }
    }
    if constexpr (MG) {
      // The rows as formed.  Of a ragged tile only the units inside C are stored, and only those add to
      // the sums: a formed row is zero past C (and in the upper half of a half unit) because every input
      // read as zero there and the code is linear.  Nothing here may make a row nonzero past C.
      bw_magic_out<R, IT, VW>(ml, K, acc);
      ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(C), static_cast<uint64_t>(off0), kStep, red);
    }
  }, a.tile_phase);
}

// the XOR-row flag picks one of two whole instantiations, by k_gf8_bytewise's rule
template <int R, int KC, int IT, bool BF, int VW, bool MG = false, typename Args>
__device__ __forceinline__ void encrot_bytewise_body(const Args &a, uint32_t *red = nullptr) {
  if constexpr (BF && R >= 2 && (KC == 0 || KC * R >= 40)) {
    if (const_cells(a.cells)->pad & kCellXorRow) {
      encrot_bytewise_tiles<R, KC, IT, BF, VW, true, MG>(a, red);
      return;
    }
  }
  encrot_bytewise_tiles<R, KC, IT, BF, VW, false, MG>(a, red);
}

template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_encrot_bytewise(EncodeRotArgs a) {
  encrot_bytewise_body<R, KC, IT, BF, VW>(a);
}

// k_gf8_bitsliced's lanes and doubling loop.  Lanes past the end of a ragged last tile leave the tile body.
// MG as in encrot_bytewise_tiles: every e[x] of input j and every formed word acc[r][x] go into the
// MagicLane.  The lanes past the end of a ragged last tile then skip the loads and the stores under
// `valid`, but still join the tile's reduction with zero sums (as chk_bitsliced_tiles' do).
template <int R, int DW, bool MG = false, typename Args>
__device__ __forceinline__ void encrot_bitsliced_tiles(const Args &a, uint32_t *red = nullptr) {
  typedef typename VecT<DW>::type V;
  const int K = a.K;
  const uint32_t P = static_cast<uint32_t>(a.packet);
  const uint32_t col_bytes = static_cast<uint32_t>(a.size / 8);  // nsuper * P
  constexpr uint32_t kTile = kBlock * 4 * DW;
  const uint32_t tiles_per_stripe = (col_bytes + kTile - 1) / kTile;
  const uint32_t ntiles = tiles_per_stripe * static_cast<uint32_t>(a.nstripes);
  ConstCell *cells = const_cells(a.cells);

  for_tiles(ntiles, a.tiles, a.tiles_pre, [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe;
    const ChkShards<Args> sh(a, s);
    const uint32_t colb = (t - s * tiles_per_stripe) * kTile + threadIdx.x * (4 * DW);
    const bool valid = colb < col_bytes;
    if (!MG && !valid) return;  // (P % (4 * DW) == 0 keeps a lane's DW dwords inside one packet)
    const uint32_t sp = colb / P;
    const int64_t off = static_cast<int64_t>(sp) * 8 * P + (colb - sp * P);
    MagicLane ml;  // the stripe magic's partial sums (MG only)

    if (!MG || valid) {
      V acc[R][8];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[r][x] = 0u;

      for (int j = 0; j < K; ++j) {
        const ShardRef in = sh.in(j);
        const uint64_t p = in.base + s * in.stride + off;
        V e[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) e[x] = __builtin_nontemporal_load(gptr<V>(p + x * P));
        if constexpr (MG) ml_add<8, DW>(ml, e, static_cast<uint32_t>(j));
        uint32_t c[R];
        uint32_t cm = 0;  // bits used by any output: no doublings past the highest one
#pragma unroll
        for (int r = 0; r < R; ++r) {
          c[r] = cells[r * K + j].coef;
          cm |= c[r];
        }
        gf8_sliced_mul_acc<0>(acc, e, c, cm);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ShardRef par = sh.par(r);
        const uint64_t q = par.base + s * par.stride + off;
#pragma unroll
        for (int x = 0; x < 8; ++x) put_nt<false, V>(q + x * P, acc[r][x]);
        if constexpr (MG) ml_add<8, DW>(ml, acc[r], static_cast<uint32_t>(K + r));
      }
    }
    if constexpr (MG) ml_commit(ml, a.magic_acc, s, K + R, static_cast<uint64_t>(a.size), static_cast<uint64_t>(off), P, red);
  }, a.tile_phase);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_encrot_bitsliced(EncodeRotArgs a) {
  encrot_bitsliced_tiles<R, DW>(a);
}

// the MG kernels (lsec_encode_magic_dev_rotated): the same tile bodies, and the LDS of their reduction
template <int R, int KC, int IT, bool BF, int VW>
__global__ __launch_bounds__(kBlock) void k_encmagicrot_bytewise(EncodeMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  encrot_bytewise_body<R, KC, IT, BF, VW, true>(a, red);
}

template <int R, int DW>
__global__ __launch_bounds__(kBlock) void k_encmagicrot_bitsliced(EncodeMagicRotArgs a) {
  __shared__ uint32_t red[kBlock / 64];
  encrot_bitsliced_tiles<R, DW, true>(a, red);
}

template <int R, int KC, int IT, bool BF, int VW>
hipError_t encrot_bytewise_kernel(const EncodeRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormEncRot, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_encrot_bytewise<R, KC, IT, BF, VW>, grid, st, a);
}

template <int R, int DW>
hipError_t encrot_bitsliced_kernel(const EncodeRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormEncRot, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_encrot_bitsliced<R, DW>, grid, st, a);
}

template <int R, int KC, int IT, bool BF, int VW>
hipError_t encmagicrot_bytewise_kernel(const EncodeMagicRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormEncMagicRot, 0, R, KC, IT, VW, BF ? 1 : 0, 0});
  return launch_tiled(&k_encmagicrot_bytewise<R, KC, IT, BF, VW>, grid, st, a);
}

template <int R, int DW>
hipError_t encmagicrot_bitsliced_kernel(const EncodeMagicRotArgs &a, hipStream_t st, int grid) {
  record_launch({kFormEncMagicRot, 1, R, 0, 0, 0, 0, DW});
  return launch_tiled(&k_encmagicrot_bitsliced<R, DW>, grid, st, a);
}

// the form is the rotated check's for the same K x R (chk_bytewise_form), switched on as dispatch_scrub_bytewise does
template <int R>
hipError_t dispatch_encrot_bytewise(const EncodeRotArgs &a, hipStream_t st, int grid) {
  const BwForm f = chk_bytewise_form(a.K, R);
  switch (f.kc) {
#define LSEC_ENCROT_K(KK)                                                        \
  case KK: {                                                                     \
    constexpr BwForm ff = chk_bytewise_form(KK, R);                              \
    if constexpr (ff.kc == KK)                                                   \
      return encrot_bytewise_kernel<R, KK, ff.it, ff.bf, ff.vw>(a, st, grid);    \
    break;                                                                       \
  }
    LSEC_FIXED_K(LSEC_ENCROT_K)
#undef LSEC_ENCROT_K
    default: break;
  }
  if constexpr (R == 1) {
    return encrot_bytewise_kernel<1, 0, 1, false, 2>(a, st, grid);
  } else {
    if (f.it == 1) return encrot_bytewise_kernel<R, 0, 1, true, 4>(a, st, grid);
    return encrot_bytewise_kernel<R, 0, 2, true, 4>(a, st, grid);
  }
}

// dw dwords per lane, as the rotated check wherever the encode's policy sends it (cauchy8_bitsliced_dw
// asks for more than one dword up to kEncRotWideRows rows only; the wider forms beyond, 256 VGPRs of
// accumulators at eight rows, are not instantiated)
constexpr int kEncRotWideRows = kLocWideRows;
template <int R>
hipError_t dispatch_encrot_bitsliced(const EncodeRotArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kEncRotWideRows) {
    if (dw == 4) return encrot_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return encrot_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? encrot_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_encode_rot_inst.hip
#define LSEC_DECLARE_ENCROT_R(RR)                                                                   \
  extern template hipError_t dispatch_encrot_bytewise<RR>(const EncodeRotArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_encrot_bitsliced<RR>(const EncodeRotArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_ENCROT
LSEC_DECLARE_ENCROT_R(1) LSEC_DECLARE_ENCROT_R(2) LSEC_DECLARE_ENCROT_R(3) LSEC_DECLARE_ENCROT_R(4)
LSEC_DECLARE_ENCROT_R(5) LSEC_DECLARE_ENCROT_R(6) LSEC_DECLARE_ENCROT_R(7) LSEC_DECLARE_ENCROT_R(8)
#endif

// The MG forms (lsec_encode_magic_dev_rotated; DESIGN.md 3.9 has their registers): the rotated encode's
// own, through constants of their own, so that one family can move without the other.
constexpr BwForm encmagicrot_bytewise_form(int K, int R) { return chk_bytewise_form(K, R); }

// dispatch_encrot_bytewise over encmagicrot_bytewise_form
template <int R>
hipError_t dispatch_encmagicrot_bytewise(const EncodeMagicRotArgs &a, hipStream_t st, int grid) {
  const BwForm f = encmagicrot_bytewise_form(a.K, R);
  switch (f.kc) {
#define LSEC_ENCMAGICROT_K(KK)                                                        \
  case KK: {                                                                          \
    constexpr BwForm ff = encmagicrot_bytewise_form(KK, R);                           \
    if constexpr (ff.kc == KK)                                                        \
      return encmagicrot_bytewise_kernel<R, KK, ff.it, ff.bf, ff.vw>(a, st, grid);    \
    break;                                                                            \
  }
    LSEC_FIXED_K(LSEC_ENCMAGICROT_K)
#undef LSEC_ENCMAGICROT_K
    default: break;
  }
  if constexpr (R == 1) {
    return encmagicrot_bytewise_kernel<1, 0, 1, false, 2>(a, st, grid);
  } else {
    if (f.it == 1) return encmagicrot_bytewise_kernel<R, 0, 1, true, 4>(a, st, grid);
    return encmagicrot_bytewise_kernel<R, 0, 2, true, 4>(a, st, grid);
  }
}

// dw dwords per lane: the rotated encode's, more than one up to kEncMagicRotWideRows rows
constexpr int kEncMagicRotWideRows = kEncRotWideRows;
template <int R>
hipError_t dispatch_encmagicrot_bitsliced(const EncodeMagicRotArgs &a, hipStream_t st, int grid, int dw) {
  if constexpr (R <= kEncMagicRotWideRows) {
    if (dw == 4) return encmagicrot_bitsliced_kernel<R, 4>(a, st, grid);
    if (dw == 2) return encmagicrot_bitsliced_kernel<R, 2>(a, st, grid);
  }
  return dw == 1 ? encmagicrot_bitsliced_kernel<R, 1>(a, st, grid) : hipErrorInvalidValue;
}

// instantiated per R in ec_encode_magic_rot_inst.hip
#define LSEC_DECLARE_ENCMAGICROT_R(RR)                                                                        \
  extern template hipError_t dispatch_encmagicrot_bytewise<RR>(const EncodeMagicRotArgs &, hipStream_t, int); \
  extern template hipError_t dispatch_encmagicrot_bitsliced<RR>(const EncodeMagicRotArgs &, hipStream_t, int, int);
#ifndef LSEC_INSTANTIATING_ENCMAGICROT
LSEC_DECLARE_ENCMAGICROT_R(1) LSEC_DECLARE_ENCMAGICROT_R(2) LSEC_DECLARE_ENCMAGICROT_R(3) LSEC_DECLARE_ENCMAGICROT_R(4)
LSEC_DECLARE_ENCMAGICROT_R(5) LSEC_DECLARE_ENCMAGICROT_R(6) LSEC_DECLARE_ENCMAGICROT_R(7) LSEC_DECLARE_ENCMAGICROT_R(8)
#endif

#define LSEC_DECLARE_R(RR)                                                                         \
  extern template hipError_t dispatch_bytewise<RR>(const ApplyArgs &, hipStream_t, int, int);      \
  extern template hipError_t dispatch_bitsliced<RR>(const ApplyArgs &, hipStream_t, int, int);         \
  extern template hipError_t dispatch_bitmatrix<RR>(const ApplyArgs &, hipStream_t, int);           \
  extern template hipError_t dispatch_bytewise_magic<RR>(const ApplyArgs &, hipStream_t, int);          \
  extern template hipError_t dispatch_wordwise<RR>(const ApplyArgs &, hipStream_t, int);         \
  extern template hipError_t dispatch_gfw_bitsliced<RR>(const ApplyArgs &, hipStream_t, int);      \
  extern template hipError_t dispatch_gfw_transposed<RR>(const ApplyArgs &, hipStream_t, int);
#ifndef LSEC_INSTANTIATING
LSEC_DECLARE_R(1) LSEC_DECLARE_R(2) LSEC_DECLARE_R(3) LSEC_DECLARE_R(4)
LSEC_DECLARE_R(5) LSEC_DECLARE_R(6) LSEC_DECLARE_R(7) LSEC_DECLARE_R(8)
#endif

#undef LSEC_INLINE

}  // namespace lsec
