"""GPU: lsec_check_dev, the one-pass parity check of device-resident stripes.

Bar: bit-exact.  The yardstick is the reference: stripes are encoded by the real reference
(oracle/_ref) when it is built, else by the oracle restatement, and the expected syndrome of a
stripe is always computed on the CPU -- its data chunks as stored are re-encoded by the reference
and bit r is set where that parity row differs from the stored one.  It is never taken from the engine.

Shards live in the arenas of tests/layouts.py (canary gaps and guard bands).  After every call
  * the syndrome words and bad_count equal the expected ones (they were pre-filled with 0xFFFFFFFF
    and a non-zero value: the call sets them itself),
  * the canary words on either side of both are unchanged,
  * the whole arena is unchanged: the shards are only read.
"""
import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

import layouts as LY

pytestmark = pytest.mark.gpu

# code -> (method, k, m, packet): every bytewise launch shape and the bit-sliced kernel
CODES = {
    "rs63": (L.REED_SOL_VAN, 6, 3, 0),        # 2 x 16 B per lane, K fixed
    "rs164": (L.REED_SOL_VAN, 16, 4, 0),      # the K >= 16 shape: 16 B per lane
    "raid4_61": (L.RAID4, 6, 1, 0),           # R = 1: 8 B per lane, per-cell branches
    "r6_62": (L.REED_SOL_R6_OP, 6, 2, 0),
    "rs128": (L.REED_SOL_VAN, 12, 8, 0),      # bit 7 must be reachable; K at run time
    "rs52": (L.REED_SOL_VAN, 5, 2, 0),        # K at run time, odd: the four-at-a-time input loop ends in one input
    "rs73": (L.REED_SOL_VAN, 7, 3, 0),        # ... and in three
    "cg63": (L.CAUCHY_GOOD, 6, 3, 8),         # bit-sliced
    "co42": (L.CAUCHY_ORIG, 4, 2, 8),
    "cg164": (L.CAUCHY_GOOD, 16, 4, 8),       # bit-sliced at the encode's 4 (2 at packet 8) dwords per lane
}
BYTEWISE = ("rs63", "rs164", "raid4_61", "r6_62", "rs128", "rs52", "rs73")
SLICED = ("cg63", "co42", "cg164")
# a single half lane, one lane, one full 8 KiB tile, a tile + a half-lane tail, three tiles, three tiles + a tail
BYTEWISE_SIZES = (8, 16, 8192, 8200, 24576, 24584)
# (packet, C).  Packet 8 is the smallest the yardstick encodes (Jerasure takes multiples of
# sizeof(long)): one super-packet, and 161 super-packets = 1288 bytes of packet-column space, which is
# no multiple of the 1 KiB column tile; then packet 512 with three super-packets (1.5 tiles).
# K >= 16 runs 4 dwords per lane where the packet holds them (a 4 KiB tile: 65 super-packets of 64 make
# 4160 bytes) and 2 at packet 8.
SLICED_SIZES = ((8, 64), (8, 64 * 161), (512, 8 * 512 * 3))
SLICED_SIZES_K16 = ((8, 64), (8, 64 * 161), (64, 8 * 64 * 65))
LAYOUTS = ("packed", "off8", "mixed")
NSTRIPES, BAD = 5, 2
FLIP = 0x5A
CANARY_WORD, BAD_FILL = 0x5EED5EED, 0x7B7B7B7B

_plans, _stripes = {}, {}


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES, or the tuple itself (tests/scrub_forms.py's plans)"""
    return CODES[code] if isinstance(code, str) else tuple(code)


def ref_encode(code, packet, data):
    """the yardstick's parity [m, C] of data [k, C]"""
    method, k, m, _ = spec(code)
    if not O.ref_available():
        return O.encode(method, np.ascontiguousarray(data), m, packet, 8)
    key = (code, packet)
    if key not in _plans:
        _plans[key] = O.RefPlan(method, k, m, 8, packet)
    return _plans[key].encode(np.ascontiguousarray(data))


def stripes(code, packet, size, nstripes):
    """uint8 [N, k+m, C]: random data and the yardstick's parity; computed once per shape, never modified"""
    key = (code, packet, size, nstripes)
    if key not in _stripes:
        method, k, m, _ = spec(code)
        rng = np.random.default_rng(abs(hash(key)) % (1 << 32))
        full = np.empty((nstripes, k + m, size), np.uint8)
        full[:, :k] = rng.integers(0, 256, (nstripes, k, size), dtype=np.uint8)
        for s in range(nstripes):
            full[s, k:] = ref_encode(code, packet, full[s, :k])
        full.setflags(write=False)
        _stripes[key] = full
    return _stripes[key]


def expected_mask(code, packet, stripe):
    """stripe uint8 [k+m, C] as stored -> the syndrome word the call must produce"""
    _, k, m, _ = spec(code)
    par = ref_encode(code, packet, stripe[:k])
    return sum(1 << r for r in range(m) if not np.array_equal(par[r], stripe[k + r]))


def make_plan(code, packet, size):
    method, k, m, _ = spec(code)
    p = L.Plan.new(method, size, k, m, 8, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0
    return p


class Words:
    """[4 canaries | nstripes syndrome words | 4 canaries | bad_count | 4 canaries] in device memory"""

    def __init__(self, torch, n):
        self.n = n
        t = np.full(n + 13, CANARY_WORD, np.uint32)
        t[4:4 + n] = 0xFFFFFFFF
        t[8 + n] = BAD_FILL
        self.template = torch.from_numpy(t.view(np.int32)).cuda()
        self.dev = torch.empty_like(self.template)
        self.syndrome_ptr = self.dev.data_ptr() + 16
        self.bad_ptr = self.dev.data_ptr() + 4 * (8 + n)

    def arm(self):
        self.dev.copy_(self.template)

    def read(self):
        """(syndrome uint32 [n], bad_count) after checking the canaries; the caller has synchronised"""
        w = self.dev.cpu().numpy().view(np.uint32)
        n = self.n
        for lo, hi in ((0, 4), (4 + n, 8 + n), (9 + n, 13 + n)):
            assert (w[lo:hi] == CANARY_WORD).all(), f"canary words [{lo}, {hi}) changed: {w[lo:hi]}"
        return w[4:4 + n].copy(), int(w[8 + n])


class Rig:
    """one arena of consistent stripes on the device, a plan and the output words"""

    def __init__(self, torch, code, packet, size, layout, nstripes=NSTRIPES):
        self.torch, self.code, self.packet, self.size, self.nstripes = torch, code, packet, size, nstripes
        _, self.k, self.m, _ = spec(code)
        self.full = stripes(code, packet, size, nstripes)
        self.lay = LY.plan_layout(layout, self.k, self.m, nstripes, size, outputs=range(self.k, self.k + self.m))
        LY.check_layout(self.lay)
        before, _ = LY.images(self.lay, self.full, ())
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, before)
        self.orig = self.arena.clone()
        self.words = Words(torch, nstripes)
        self.plan = make_plan(code, packet, size)

    def close(self):
        self.plan.close()

    def pos(self, s, i, b):
        return self.lay.start(i, s) + b

    def flip(self, s, i, b):
        self.arena[self.pos(s, i, b):self.pos(s, i, b) + 1].bitwise_xor_(FLIP)

    def flip_chunk(self, s, i):
        a = self.lay.start(i, s)
        self.arena[a:a + self.size].bitwise_xor_(0xFF)

    def check(self):
        """one call over the arena as it is; returns (syndrome, bad_count) after the canary and arena checks"""
        torch = self.torch
        want_arena = self.arena.clone()
        self.words.arm()
        self.plan.check_dev_refs(self.refs, self.nstripes, self.size, self.words.syndrome_ptr, self.words.bad_ptr,
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(self.arena, want_arena), "the call wrote into the arena"
        return self.words.read()

    def expect(self, bad):
        """bad: {stripe: mask}; every other word must be 0"""
        syn, count = self.check()
        want = np.zeros(self.nstripes, np.uint32)
        for s, mask in bad.items():
            want[s] = mask
        assert np.array_equal(syn, want), f"{self.code} C={self.size} {self.lay.name}: syndrome {syn} != {want}"
        assert count == sum(1 for v in bad.values() if v), f"{self.code} C={self.size}: bad_count {count}, syndrome {syn}"

    def stored(self, s, flips=(), chunks=()):
        """stripe s as the arena holds it after the given byte flips (i, b) and whole-chunk flips i"""
        st = self.full[s].copy()
        for i, b in flips:
            st[i, b] ^= FLIP
        for i in chunks:
            st[i] ^= 0xFF
        return st


def positions(size):
    return sorted({b for b in (0, 15, 16, 1023, 1024, 8191, 8192, size - 9, size - 8, size - 1) if 0 <= b < size})


def shapes(code):
    if code in BYTEWISE:
        return [(0, c) for c in BYTEWISE_SIZES]
    return list(SLICED_SIZES_K16 if CODES[code][1] >= 16 else SLICED_SIZES)


# ---------------------------------------------------------------- consistent stripes, one corrupted byte
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", list(CODES))
def test_consistent_and_single_byte(cuda, code, layout):
    import torch

    _, k, m, _ = CODES[code]
    for packet, size in shapes(code):
        bench = Rig(torch, code, packet, size, layout)
        try:
            bench.expect({})  # consistent: every word 0, bad_count 0
            for b in positions(size):
                # a corruption in parity row r gives exactly 1 << r; the neighbours of stripe 2 stay 0
                for r in range(m):
                    bench.flip(BAD, k + r, b)
                    assert expected_mask(code, packet, bench.stored(BAD, [(k + r, b)])) == 1 << r
                    bench.expect({BAD: 1 << r})
                    bench.flip(BAD, k + r, b)
                # a corruption in a data chunk gives the reference-derived mask
                for j in sorted({0, k // 2, k - 1}):
                    bench.flip(BAD, j, b)
                    mask = expected_mask(code, packet, bench.stored(BAD, [(j, b)]))
                    assert mask != 0
                    bench.expect({BAD: mask})
                    bench.flip(BAD, j, b)
            assert torch.equal(bench.arena, bench.orig)
        finally:
            bench.close()


# ---------------------------------------------------------------- several rows, two stripes
@pytest.mark.parametrize("code", list(CODES))
def test_several_rows(cuda, code):
    import torch

    _, k, m, _ = CODES[code]
    for packet, size in shapes(code)[1:]:
        bench = Rig(torch, code, packet, size, "mixed")
        try:
            b0, b1 = size // 2, size - 1
            other = (m - 1) // 2 if m != 2 else 1  # a row of its own where the code has three
            bench.flip(1, k, b0)
            if m > 1:
                bench.flip(1, k + m - 1, b1)
            bench.flip(4, k + other, 0)
            want = {1: expected_mask(code, packet, bench.stored(1, [(k, b0)] + ([(k + m - 1, b1)] if m > 1 else []))),
                    4: expected_mask(code, packet, bench.stored(4, [(k + other, 0)]))}
            assert want == {1: 1 | 1 << (m - 1), 4: 1 << other}
            bench.expect(want)
        finally:
            bench.close()


# ---------------------------------------------------------------- exactly-once counting
@pytest.mark.parametrize("code", list(CODES))
def test_every_wave_publishes_each_stripe_counts_once(cuda, code):
    """every byte of a data chunk differs in 3 of 8 stripes, so every tile and wave of those stripes
    publishes; bad_count must still be 3"""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = (0, 24584) if code in BYTEWISE else (8, 64 * 385)  # 385 super-packets: three column tiles + 8 bytes
    bench = Rig(torch, code, packet, size, "off8", nstripes=8)
    try:
        want = {}
        for s, j in ((0, 0), (3, k - 1), (7, k // 2)):
            bench.flip_chunk(s, j)
            want[s] = expected_mask(code, packet, bench.stored(s, chunks=[j]))
            assert want[s] != 0
        bench.expect(want)
    finally:
        bench.close()


# ---------------------------------------------------------------- stream order
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_follows_a_write_on_its_stream(cuda, code):
    """a torch op on a non-default stream corrupts a byte and the check is queued straight behind
    it, no synchronisation in between: the corruption is seen"""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = shapes(code)[-1]
    bench = Rig(torch, code, packet, size, "packed")
    try:
        st = torch.cuda.Stream()
        bench.words.arm()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            bench.flip(3, k + 1, size - 1)
        bench.plan.check_dev_refs(bench.refs, bench.nstripes, size, bench.words.syndrome_ptr, bench.words.bad_ptr, st.cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        syn, count = bench.words.read()
        assert syn.tolist() == [0, 0, 0, 2, 0] and count == 1
    finally:
        bench.close()


def test_torch_form_and_no_bad_count(cuda):
    import torch

    code, size, nstr = "rs63", 4096, 8
    _, k, m, _ = CODES[code]
    full = stripes(code, 0, size, nstr)
    data, par = torch.from_numpy(full[:, :k].copy()).cuda(), torch.from_numpy(full[:, k:].copy()).cuda()
    par[5, 2, 77] ^= 1
    syn = torch.full((nstr,), -1, dtype=torch.int32, device="cuda")
    with make_plan(code, 0, size) as p:
        p.check_dev(data, par, syn)  # bad_count NULL
        torch.cuda.synchronize()
    assert syn.cpu().tolist() == [0, 0, 0, 0, 0, 4, 0, 0]


# ---------------------------------------------------------------- persistent-grid path
def test_persistent_grid_all_tile_modes(cuda):
    """16384 tiles (kTileQueueMinTiles): RS(6+3), C = 16 KiB, 8192 stripes, about 1.2 GB.  Data from
    torch.randint, parity from lsec_encode_dev (pinned bit-exact to the reference by the rest of the
    suite); a dozen stripes over the range are corrupted, their masks come from the reference."""
    import torch

    code, size, nstr = "rs63", 16384, 8192
    _, k, m, _ = CODES[code]
    data = torch.randint(0, 256, (nstr, k, size), dtype=torch.uint8, device="cuda")
    par = torch.empty((nstr, m, size), dtype=torch.uint8, device="cuda")
    words = Words(torch, nstr)
    hit = [0, 1, 700, 1023, 1024, 2049, 4095, 4096, 5555, 7000, 8190, 8191]
    mode0 = E.tile_sharing()
    try:
        with make_plan(code, 0, size) as p:
            p.encode_dev(data, par)
            torch.cuda.synchronize()
            want = np.zeros(nstr, np.uint32)
            for n, s in enumerate(hit):
                if n % 3 == 0:
                    par[s, n % m, (n * 1361) % size] ^= 0x10       # one parity row
                elif n % 3 == 1:
                    data[s, n % k, size - 1 - n] ^= 0x01           # a data byte
                else:
                    par[s, 0, n] ^= 0x80                           # two parity rows
                    par[s, m - 1, size - 1] ^= 0x80
                stored = np.concatenate([data[s].cpu().numpy(), par[s].cpu().numpy()])
                want[s] = expected_mask(code, 0, stored)
                assert want[s] != 0
            d0, p0 = data.clone(), par.clone()
            refs, _, _ = p.tensor_refs(data, par)
            for mode in (E.TILES_STATIC, E.TILES_SHARED, E.TILES_TAIL):
                E.set_tile_sharing(mode)
                words.arm()
                p.check_dev_refs(refs, nstr, size, words.syndrome_ptr, words.bad_ptr, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                syn, count = words.read()
                diff = np.flatnonzero(syn != want)
                assert diff.size == 0, f"tile mode {mode}: stripes {diff[:8]} got {syn[diff[:8]]} want {want[diff[:8]]}"
                assert count == len(hit), f"tile mode {mode}: bad_count {count}"
                assert torch.equal(data, d0) and torch.equal(par, p0), f"tile mode {mode}: the call wrote into the shards"
    finally:
        E.set_tile_sharing(mode0)
