"""GPU: lsec_locate_dev, finding (and with repair rebuilding) the corrupt chunk of device-resident stripes.

Bar: bit-exact.  The yardstick is the reference, never the engine: stripes are encoded by the real
reference (oracle/_ref) when it is built, else by the oracle restatement (test_gpu_check's stripes,
shared with it and computed once).  For a stripe as stored, chunk i is an explanation when, after the
reference's decode with erasure {i}, the reference's encode reproduces every parity row of the
stripe.  From the explanations and the reference-derived syndrome word the expected outputs follow
by the rules of include/lstore_ec.h:
  hyp      bit j for every data chunk j that is an explanation (a consistent stripe: all k bits)
  located  LOCATE_CLEAN when the syndrome is 0, k + r when it is 1 << r, j when it has all m bits and
           hyp is 1 << j, else LOCATE_MANY
The oracle runs only for corrupted stripes, once per distinct corruption (cached across layouts).

Shards live in the arenas of tests/layouts.py (canary gaps and guard bands); the four outputs sit in
one buffer between canary bytes, pre-filled with garbage, `located` at an odd address.  After every
call the canaries are unchanged and, without repair, so is the whole arena.
"""
import numpy as np
import pytest

import oracle as O
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC

pytestmark = pytest.mark.gpu

CODES = {c: TC.CODES[c] for c in ("rs63", "rs164", "r6_62", "rs128", "rs52", "rs73", "cg63", "co42", "cg164")}
BYTEWISE = ("rs63", "rs164", "r6_62", "rs128", "rs52", "rs73")
# test_gpu_check.py explains the shapes: a half lane, a lane, one 8 KiB tile, a tile + a half-lane tail,
# three tiles + a tail; bit-sliced one super-packet, a ragged column tile, 1.5 tiles (k >= 16: 4 dwords per lane)
BYTEWISE_SIZES = (8, 16, 8192, 8200, 24584)
SLICED_SIZES = ((8, 64), (8, 64 * 161), (512, 12288))
SLICED_SIZES_K16 = ((8, 64), (8, 64 * 161), (64, 8 * 64 * 65))
LAYOUTS = ("packed", "off8", "mixed")
NSTRIPES, BAD = 5, 2
FLIP, FLIP2 = TC.FLIP, 0x33
CANARY, FILL = 0x5E, 0x7B
CLEAN, MANY = E.LOCATE_CLEAN, E.LOCATE_MANY

_expect = {}


def shapes(code):
    if code in BYTEWISE:
        return [(0, c) for c in BYTEWISE_SIZES]
    return list(SLICED_SIZES_K16 if CODES[code][1] >= 16 else SLICED_SIZES)


def ref_decode(code, packet, shards, erased):
    """the yardstick's decode of one erased chunk (or of a list of them), in place"""
    method, k, m, _ = TC.spec(code)
    erased = [erased] if isinstance(erased, (int, np.integer)) else list(erased)
    if not O.ref_available():
        assert O.decode(method, shards, k, erased, packet, 8) == 0
        return
    if (code, packet) not in TC._plans:  # (shared with test_gpu_check's ref_encode)
        TC._plans[(code, packet)] = O.RefPlan(method, k, m, 8, packet)
    assert TC._plans[(code, packet)].decode(shards, erased) == 0


def explanations(code, packet, stripe):
    """the chunks i of stripe [k+m, C] whose replacement by what the others rebuild makes it consistent"""
    _, k, m, _ = TC.spec(code)
    out = []
    for i in range(k + m):
        sh = stripe.copy()
        sh[i] = 0
        ref_decode(code, packet, sh, i)
        if np.array_equal(TC.ref_encode(code, packet, sh[:k]), sh[k:]):
            out.append(i)
    return out


def expected(code, packet, stripe, key):
    """(syndrome, hyp, located) of a corrupted stripe as stored; key names the corruption for the cache (the
    rigs: the batch's stripe count, the stripe and what it holds, so the rotated rig shares the entries)"""
    _, k, m, _ = TC.spec(code)
    key = (code, packet, stripe.shape[1]) + key
    if key not in _expect:
        syn = TC.expected_mask(code, packet, stripe)
        ex = explanations(code, packet, stripe)
        hyp = sum(1 << i for i in ex if i < k)
        if syn == 0:
            loc = CLEAN
        elif bin(syn).count("1") == 1:
            loc = k + syn.bit_length() - 1
            assert loc in ex  # the rule and the yardstick agree
        elif syn == (1 << m) - 1 and bin(hyp).count("1") == 1:
            loc = hyp.bit_length() - 1
        else:
            loc = MANY
        _expect[key] = (syn, hyp, loc)
    return _expect[key]


class Outs:
    """[canary | syndrome | canary | hyp | canary | located (odd address) | canary | counts | canary], one
    device buffer of bytes; everything outside the four outputs is CANARY, the outputs start as FILL"""

    def __init__(self, torch, n):
        self.n = n
        self.syn_off = 16
        self.hyp_off = (self.syn_off + 4 * n + 16 + 7) // 8 * 8
        self.loc_off = (self.hyp_off + 8 * n + 16) | 1
        self.cnt_off = (self.loc_off + n + 16 + 3) // 4 * 4
        total = self.cnt_off + 8 + 16
        t = np.full(total, CANARY, np.uint8)
        self.spans = ((self.syn_off, 4 * n), (self.hyp_off, 8 * n), (self.loc_off, n), (self.cnt_off, 8))
        self.mask = np.ones(total, bool)
        for off, ln in self.spans:
            t[off:off + ln] = FILL
            self.mask[off:off + ln] = False
        self.template_np = t
        self.template = torch.from_numpy(t).cuda()
        self.dev = torch.empty_like(self.template)
        base = self.dev.data_ptr()
        assert base % 8 == 0
        self.syndrome_ptr, self.hyp_ptr = base + self.syn_off, base + self.hyp_off
        self.located_ptr, self.counts_ptr = base + self.loc_off, base + self.cnt_off
        assert self.located_ptr % 2 == 1

    def arm(self):
        self.dev.copy_(self.template)

    def read(self):
        """(syndrome uint32 [n], hyp uint64 [n], located uint8 [n], counts [2]) after checking the canaries"""
        b = self.dev.cpu().numpy()
        bad = np.flatnonzero((b != self.template_np) & self.mask)
        assert bad.size == 0, f"canary bytes changed at {bad[:8]}"
        n = self.n
        return (b[self.syn_off:self.syn_off + 4 * n].copy().view(np.uint32), b[self.hyp_off:self.hyp_off + 8 * n].copy().view(np.uint64),
                b[self.loc_off:self.loc_off + n].copy(), b[self.cnt_off:self.cnt_off + 8].copy().view(np.uint32))


class Rig:
    """one arena of consistent stripes on the device, a plan and the outputs"""

    def __init__(self, torch, code, packet, size, layout, nstripes=NSTRIPES):
        self.torch, self.code, self.packet, self.size, self.nstripes = torch, code, packet, size, nstripes
        _, self.k, self.m, _ = TC.spec(code)
        self.full = TC.stripes(code, packet, size, nstripes)
        self.lay = LY.plan_layout(layout, self.k, self.m, nstripes, size, outputs=range(self.k, self.k + self.m))
        LY.check_layout(self.lay)
        before, _ = LY.images(self.lay, self.full, ())
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, before)
        self.orig = self.arena.clone()
        self.outs = Outs(torch, nstripes)
        self.plan = TC.make_plan(code, packet, size)
        self.flips, self.chunks = {}, {}  # stripe -> what it holds beside the reference bytes
        self.written = {}                 # stripe -> (the whole stripe as stored, a name for the cache): write()

    def close(self):
        self.plan.close()

    def flip(self, s, i, b, v=FLIP):
        """XOR v into byte b of chunk i of stripe s (a second call with the same v undoes it)"""
        a = self.lay.start(i, s) + b
        self.arena[a:a + 1].bitwise_xor_(v)
        self.note(self.flips.setdefault(s, []), (i, b, v))

    def flip_chunk(self, s, i):
        a = self.lay.start(i, s)
        self.arena[a:a + self.size].bitwise_xor_(0xFF)
        self.note(self.chunks.setdefault(s, []), i)

    def write(self, s, stripe, name):
        """store `stripe` uint8 [k+m, C] as stripe s (the chunks that differ from what the arena holds)"""
        assert s not in self.flips and s not in self.chunks
        for i in range(self.k + self.m):
            a = self.lay.start(i, s)
            self.arena[a:a + self.size] = self.torch.from_numpy(np.ascontiguousarray(stripe[i])).to(self.arena.device)
        self.written[s] = (stripe.copy(), name)

    @staticmethod
    def note(cur, what):
        if what in cur:
            cur.remove(what)
        else:
            cur.append(what)

    def want(self):
        """expected (syndrome, hyp, located, counts) of the arena as it is, from the yardstick"""
        n, k = self.nstripes, self.k
        syn, hyp = np.zeros(n, np.uint32), np.full(n, (1 << k) - 1, np.uint64)
        loc = np.full(n, CLEAN, np.uint8)
        for s in range(n):
            fl, ch = sorted(self.flips.get(s, [])), sorted(self.chunks.get(s, []))
            if s in self.written:
                st, name = self.written[s]
                syn[s], hyp[s], loc[s] = expected(self.code, self.packet, st, (n, s, name))
                continue
            if not fl and not ch:
                continue
            st = self.full[s].copy()
            for i, b, v in fl:
                st[i, b] ^= v
            for i in ch:
                st[i] ^= 0xFF
            syn[s], hyp[s], loc[s] = expected(self.code, self.packet, st, (n, s, tuple(fl), tuple(ch)))
        counts = [int(((loc != CLEAN) & (loc != MANY)).sum()), int((loc == MANY).sum())]
        return syn, hyp, loc, counts

    def locate(self, repair=False, stream=None):
        torch = self.torch
        self.outs.arm()
        o = self.outs
        self.plan.locate_dev_refs(self.refs, self.nstripes, self.size, o.syndrome_ptr, o.hyp_ptr, o.located_ptr, o.counts_ptr,
                                  repair, stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return o.read()

    def expect(self, what=""):
        """one call without repair over the arena as it is: the outputs are the yardstick's and the arena
        is unchanged; returns the expected (syndrome, hyp, located, counts)"""
        before = self.arena.clone()
        got = self.locate()
        want = self.want()
        tag = f"{self.code} C={self.size} {self.lay.name} {what}"
        assert np.array_equal(got[0], want[0]), f"{tag}: syndrome {got[0]} != {want[0]}"
        assert np.array_equal(got[1], want[1]), f"{tag}: hyp {got[1]} != {want[1]}"
        assert np.array_equal(got[2], want[2]), f"{tag}: located {got[2]} != {want[2]}"
        assert got[3].tolist() == want[3], f"{tag}: counts {got[3]} != {want[3]}"
        assert self.torch.equal(self.arena, before), f"{tag}: the call wrote into the arena"
        return want


# ---------------------------------------------------------------- consistent stripes, one corrupted byte
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", list(CODES))
def test_consistent_and_single_byte(cuda, code, layout):
    import torch

    _, k, m, _ = CODES[code]
    for packet, size in shapes(code):
        rig = Rig(torch, code, packet, size, layout)
        try:
            syn, hyp, loc, counts = rig.expect("consistent")
            assert not syn.any() and (hyp == (1 << k) - 1).all() and (loc == CLEAN).all() and counts == [0, 0]
            for b in TC.positions(size):
                for i in list(range(k, k + m)) + sorted({0, k // 2, k - 1}):
                    rig.flip(BAD, i, b)
                    syn, hyp, loc, counts = rig.expect(f"chunk {i} byte {b}")
                    # the yardstick names exactly that chunk, and the neighbours are clean
                    assert loc.tolist() == [CLEAN, CLEAN, i, CLEAN, CLEAN] and counts == [1, 0]
                    assert hyp[BAD] == ((1 << i) if i < k else 0)
                    rig.flip(BAD, i, b)
            assert torch.equal(rig.arena, rig.orig)
        finally:
            rig.close()


# ---------------------------------------------------------------- one chunk seen by several waves
@pytest.mark.parametrize("code", list(CODES))
def test_one_chunk_in_several_tiles_counts_once(cuda, code):
    """the same chunk hit at byte 0 and at byte C-1 (different tiles and waves), and a whole chunk flipped so
    that every wave of the stripe publishes: still located, and counted once"""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "off8", nstripes=8)
    try:
        for s, i in ((0, k - 1), (5, k + m - 1)):
            rig.flip(s, i, 0)
            rig.flip(s, i, size - 1)
        for s, i in ((2, 0), (3, k // 2), (7, k)):
            rig.flip_chunk(s, i)
        _, _, loc, counts = rig.expect()
        assert loc.tolist() == [k - 1, CLEAN, 0, k // 2, CLEAN, k + m - 1, CLEAN, k] and counts == [5, 0]
    finally:
        rig.close()


# ---------------------------------------------------------------- two chunks
@pytest.mark.parametrize("code", list(CODES))
def test_two_corrupt_chunks(cuda, code):
    """two chunks hit in different tiles, and two chunks hit at one column: the verdict is the yardstick's
    (no single chunk explains them with these byte values, so LOCATE_MANY), and counts[1] follows"""
    import torch

    _, k, m, _ = CODES[code]
    for packet, size in shapes(code)[1:]:
        rig = Rig(torch, code, packet, size, "mixed")
        try:
            col = size // 2
            rig.flip(0, 0, 0)            # two data chunks, different tiles
            rig.flip(0, k - 1, size - 1)
            rig.flip(1, 1, col)          # two data chunks, one column (two values: equal ones cancel in an all-ones row)
            rig.flip(1, k // 2 + 1, col, FLIP2)
            rig.flip(3, k // 2, 0)       # a data chunk and a parity chunk, different tiles
            rig.flip(3, k + 1, size - 1)
            rig.flip(4, k // 2, col)     # a data chunk and a parity chunk, one column
            rig.flip(4, k + m - 1, col, FLIP2)
            _, _, loc, counts = rig.expect()
            assert loc.tolist() == [MANY, MANY, CLEAN, MANY, MANY] and counts == [0, 4]
        finally:
            rig.close()


# ---------------------------------------------------------------- hypotheses that hold in different places
ADVERSARIAL = ("rs63", "rs164", "r6_62", "cg63", "cg164")


def placements(code, packet, size):
    """{name: (b, b2)}: two chunk bytes in two columns that one dword, one lane unit, one lane, one wave, one
    tile and two tiles of the locate kernel of this shape hold; the kernel's shape from the engine's prediction"""
    _, k, m, _ = TC.spec(code)
    f = E.predict_form("loc", 2 if packet else 1, k, m, packet, size)
    if not f.sliced:
        lane, step = 4 * f.VW, 256 * 4 * f.VW
        tile, b = step * f.IT, 3 * 4 * f.VW  # lane 3 of the first tile
        out = {"one dword": (b, b + 1), "two dwords of a lane unit": (b, b + 4), "two lanes of a wave": (b, b + lane),
               "two waves of a tile": (b, b + 64 * lane), "two tiles": (b, b + tile),
               "one dword of the ragged tail": (size - 8, size - 7), "two dwords of the ragged tail": (size - 8, size - 4)}
        if f.IT == 2:
            out["the two steps of a lane"] = (b, b + step)
        assert size % tile == 8 and b + tile < size - 8  # the tail is a half lane behind whole tiles
    else:
        at = lambda col, x: (col // packet) * 8 * packet + x * packet + col % packet  # chunk byte of bit plane x of a column byte
        lane, c0 = 4 * f.DW, 2 * 4 * f.DW  # lane 2 of the first column tile
        tile = 256 * lane
        # two bit planes of one column byte: the flip values overlap in some bits only, so some elements are wrong
        # in one chunk, some in the other and some in both
        out = {"two bit-plane packets of a lane": (at(c0, 0), at(c0, 5)), "two lanes of a wave": (at(c0, 2), at(c0 + lane, 2)),
               "two waves of a tile": (at(c0, 7), at(c0 + 64 * lane, 7)), "two tiles": (at(c0, 1), at(c0 + tile, 1))}
        if f.DW > 1:
            out["two dwords of a lane"] = (at(c0, 3), at(c0 + 4, 3))
        assert c0 + tile < size // 8
    assert all(0 <= b < size and 0 <= b2 < size and b != b2 for b, b2 in out.values())
    return out


@pytest.mark.parametrize("code", ADVERSARIAL)
def test_hypotheses_in_different_places_intersect_to_nothing(cuda, code):
    """data chunk j1 wrong at byte b, data chunk j2 at byte b2: each column has its own single-chunk
    explanation, the stripe has none.  hyp is an AND over lanes (the vote), waves and tiles (atomicAnd): the
    two columns are put at every distance over which that reduction runs.  One stripe per placement."""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = shapes(code)[-1]
    places = placements(code, packet, size)
    j1, j2 = 1, k - 1
    rig = Rig(torch, code, packet, size, "off8", nstripes=len(places) + 1)
    try:
        for s, (b, b2) in enumerate(places.values()):
            rig.flip(s, j1, b)
            rig.flip(s, j2, b2, FLIP2)
        syn, hyp, loc, counts = rig.want()
        # the reference says so: every row differs, no chunk explains the stripe
        for s, name in enumerate(places):
            assert (syn[s], hyp[s], loc[s]) == ((1 << m) - 1, 0, MANY), (code, name, syn[s], hyp[s], loc[s])
        assert loc[-1] == CLEAN and counts == [0, len(places)]
        rig.expect("two columns")
    finally:
        rig.close()


# ---------------------------------------------------------------- two corrupt chunks that imitate a third
def imitation(code, packet, clean, c, a, b, pos):
    """(stored, consistent, rebuilt): a byte of data chunk c of the clean stripe flipped, and chunks a and b
    rebuilt from the others by the reference.  With m = 2 that gives a consistent stripe.  With more rows the
    reference's decode of two chunks leaves m - 2 parity rows out, and no stripe that differs from a consistent
    one in fewer than m chunks has another single-chunk explanation (the code's distance is m + 1), so the last
    parity chunks are rebuilt along with a and b, m chunks in all.  stored is the clean stripe with the rebuilt
    chunks of the consistent one: it differs from the clean stripe in those alone, and from the consistent one
    in chunk c alone."""
    _, k, m, _ = TC.spec(code)
    rebuilt = [a, b]
    rebuilt += [i for i in range(k + m - 1, k - 1, -1) if i not in rebuilt][:m - 2]
    y = clean.copy()
    y[c, pos] ^= FLIP
    y[rebuilt] = 0
    ref_decode(code, packet, y, sorted(rebuilt))
    assert np.array_equal(TC.ref_encode(code, packet, y[:k]), y[k:])
    stored = clean.copy()
    stored[rebuilt] = y[rebuilt]
    assert all(not np.array_equal(stored[i], clean[i]) for i in rebuilt) and c not in rebuilt
    return stored, y, sorted(rebuilt)


@pytest.mark.parametrize("code", ADVERSARIAL)
def test_two_corrupt_chunks_imitate_a_third(cuda, code):
    """include/lstore_ec.h: with m = 2 two corrupt chunks can be what a third, innocent one would explain (with
    m rows: m corrupt chunks, see imitation()).  Chunks a and b (two data chunks; a data and a parity chunk) hold
    what makes the stripe consistent with a wrong chunk c, in a column of a full tile and in one of the ragged
    tail: the call names c, and with repair rewrites it."""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = shapes(code)[-1]
    c = k // 2
    variants = [(a, b, pos) for a, b in ((0, k - 1), (1, k + m - 1)) for pos in (83, size - 3)]
    rig = Rig(torch, code, packet, size, "off8", nstripes=len(variants) + 1)
    try:
        consistent = {}
        for s, (a, b, pos) in enumerate(variants):
            stored, consistent[s], _ = imitation(code, packet, rig.full[s], c, a, b, pos)
            rig.write(s, stored, ("imitation", c, a, b, pos))
        syn, hyp, loc, counts = rig.want()
        # the reference says so: chunk c is the one explanation
        assert loc.tolist() == [c] * len(variants) + [CLEAN] and counts == [len(variants), 0]
        assert (hyp[:-1] == 1 << c).all() and (syn[:-1] == (1 << m) - 1).all()
        rig.expect("imitation")
        # repaired: chunk c holds the consistent stripe's bytes, nothing else changed
        after = rig.arena.clone()
        for s, y in consistent.items():
            a0 = rig.lay.start(c, s)
            after[a0:a0 + size] = torch.from_numpy(y[c].copy()).cuda()
        got = rig.locate(repair=True)
        for g, w, name in zip(got[:3], (syn, hyp, loc), ("syndrome", "hyp", "located")):
            assert np.array_equal(g, w), f"{code}: {name} {g} != {w}"
        assert got[3].tolist() == counts
        LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), after.cpu().numpy(), f"{code} imitation, repaired")
    finally:
        rig.close()


# ---------------------------------------------------------------- repair
def corrupt_mixed(rig):
    """stripe 0: a data byte; 1: clean; 2: a whole parity chunk; 3: two chunks (LOCATE_MANY); 4: the last
    data chunk at its first and last byte"""
    k, m, size = rig.k, rig.m, rig.size
    rig.flip(0, k // 2, size // 3)
    rig.flip_chunk(2, k + m - 1)
    rig.flip(3, 0, 0)
    rig.flip(3, k, size - 1)
    rig.flip(4, k - 1, 0)
    rig.flip(4, k - 1, size - 1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", list(CODES))
def test_repair(cuda, code, layout):
    import torch

    _, k, m, _ = CODES[code]
    for packet, size in shapes(code)[1:]:
        rig = Rig(torch, code, packet, size, layout)
        try:
            corrupt_mixed(rig)
            want = rig.want()
            assert want[2].tolist() == [k // 2, CLEAN, k + m - 1, MANY, k - 1]
            # after the repair: the located stripes hold the original bytes, the LOCATE_MANY stripe its
            # corrupted ones, and every other byte of the arena (guard bands, gaps) is as before
            after = rig.orig.clone()
            for i, b in ((0, 0), (k, size - 1)):
                a = rig.lay.start(i, 3) + b
                after[a:a + 1].bitwise_xor_(FLIP)
            corrupted = rig.arena.clone()
            got = rig.locate(repair=True)
            for g, w, name in zip(got[:3], want[:3], ("syndrome", "hyp", "located")):
                assert np.array_equal(g, w), f"{code} C={size} {layout}: {name} {g} != {w}"
            assert got[3].tolist() == want[3] == [3, 1]
            LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), after.cpu().numpy(), f"{code} C={size} repair")
            # a following lsec_check_dev reports the repaired stripes consistent
            words = TC.Words(torch, NSTRIPES)
            words.arm()
            rig.plan.check_dev_refs(rig.refs, NSTRIPES, size, words.syndrome_ptr, words.bad_ptr, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            syn, count = words.read()
            assert syn.tolist() == [0, 0, 0, int(want[0][3]), 0] and count == 1
            # located is a stripe_pattern: the patterned decode over the k+m single erasures gives the same bytes
            rig.arena.copy_(corrupted)
            rig.locate()
            assert torch.equal(rig.arena, corrupted)
            rig.plan.decode_dev_patterns_refs(rig.refs, NSTRIPES, size, [[i] for i in range(k + m)], rig.outs.located_ptr,
                                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), after.cpu().numpy(), f"{code} C={size} patterned decode")
            rig.outs.read()  # (the canaries)
        finally:
            rig.close()


# ---------------------------------------------------------------- stream order
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_follows_a_write_on_its_stream(cuda, code):
    """a torch op on a non-default stream corrupts a byte and the call, with repair, is queued straight
    behind it, no synchronisation in between: the corruption is seen and undone"""
    import torch

    _, k, m, _ = CODES[code]
    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "packed")
    try:
        st = torch.cuda.Stream()
        rig.outs.arm()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            rig.flip(3, 1, size - 1)
        o = rig.outs
        rig.plan.locate_dev_refs(rig.refs, NSTRIPES, size, o.syndrome_ptr, o.hyp_ptr, o.located_ptr, o.counts_ptr, True, st.cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        want = rig.want()
        syn, hyp, loc, counts = o.read()
        assert loc.tolist() == [CLEAN, CLEAN, CLEAN, 1, CLEAN] and counts.tolist() == [1, 0]
        assert np.array_equal(syn, want[0]) and np.array_equal(hyp, want[1]) and syn[3] == (1 << m) - 1
        assert torch.equal(rig.arena, rig.orig)
    finally:
        rig.close()


def test_torch_form_and_no_counts(cuda):
    import torch

    code, size, nstr = "rs63", 4096, 8
    _, k, m, _ = CODES[code]
    full = TC.stripes(code, 0, size, nstr)
    data, par = torch.from_numpy(full[:, :k].copy()).cuda(), torch.from_numpy(full[:, k:].copy()).cuda()
    par[5, 2, 77] ^= 1
    data[1, 4, 4095] ^= 0x80
    syn = torch.full((nstr,), -1, dtype=torch.int32, device="cuda")
    hyp = torch.full((nstr,), 0x7B7B, dtype=torch.int64, device="cuda")
    loc = torch.full((nstr,), 0x7B, dtype=torch.uint8, device="cuda")
    with TC.make_plan(code, 0, size) as p:
        p.locate_dev(data, par, syn, hyp, loc)  # counts NULL
        torch.cuda.synchronize()
        assert syn.cpu().tolist() == [0, 7, 0, 0, 0, 4, 0, 0]
        assert hyp.cpu().tolist() == [63, 1 << 4, 63, 63, 63, 0, 63, 63]
        assert loc.cpu().tolist() == [CLEAN, 4, CLEAN, CLEAN, CLEAN, k + 2, CLEAN, CLEAN]
        counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        p.locate_dev(data, par, syn, hyp, loc, counts, repair=True)
        torch.cuda.synchronize()
    assert counts.cpu().tolist() == [2, 0]
    assert np.array_equal(data.cpu().numpy(), full[:, :k]) and np.array_equal(par.cpu().numpy(), full[:, k:])


# ---------------------------------------------------------------- persistent-grid path
def test_persistent_grid_all_tile_modes(cuda):
    """16384 tiles (kTileQueueMinTiles): RS(6+3), C = 16 KiB, 8192 stripes, about 1.2 GB, as
    test_gpu_check's.  Data from torch.randint, parity from lsec_encode_dev (pinned bit-exact to the
    reference by the rest of the suite); a dozen stripes over the range are corrupted, their expected
    outputs come from the reference.  The last mode's call repairs."""
    import torch

    code, size, nstr = "rs63", 16384, 8192
    _, k, m, _ = CODES[code]
    data = torch.randint(0, 256, (nstr, k, size), dtype=torch.uint8, device="cuda")
    par = torch.empty((nstr, m, size), dtype=torch.uint8, device="cuda")
    outs = Outs(torch, nstr)
    hit = [0, 1, 700, 1023, 1024, 2049, 4095, 4096, 5555, 7000, 8190, 8191]
    mode0 = E.tile_sharing()
    try:
        with TC.make_plan(code, 0, size) as p:
            p.encode_dev(data, par)
            torch.cuda.synchronize()
            good_d, good_p = data.clone(), par.clone()
            syn_w, hyp_w = np.zeros(nstr, np.uint32), np.full(nstr, (1 << k) - 1, np.uint64)
            loc_w = np.full(nstr, CLEAN, np.uint8)
            for n, s in enumerate(hit):
                if n % 4 == 0:
                    par[s, n % m, (n * 1361) % size] ^= 0x10       # one parity chunk
                elif n % 4 == 1:
                    data[s, n % k, size - 1 - n] ^= 0x01           # a data byte
                elif n % 4 == 2:
                    data[s, n % k, n] ^= 0x80                      # a data chunk in its first and last tile
                    data[s, n % k, size - 1] ^= 0x80
                else:
                    data[s, 0, n] ^= 0x80                          # two chunks
                    par[s, m - 1, size - 1] ^= 0x80
                stored = np.concatenate([data[s].cpu().numpy(), par[s].cpu().numpy()])
                syn_w[s], hyp_w[s], loc_w[s] = expected(code, 0, stored, ("grid", s))
            counts_w = [int(((loc_w != CLEAN) & (loc_w != MANY)).sum()), int((loc_w == MANY).sum())]
            assert counts_w == [9, 3]
            d0, p0 = data.clone(), par.clone()
            refs, _, _ = p.tensor_refs(data, par)
            modes = (E.TILES_STATIC, E.TILES_SHARED, E.TILES_TAIL)
            for mode in modes:
                E.set_tile_sharing(mode)
                outs.arm()
                repair = mode == modes[-1]
                p.locate_dev_refs(refs, nstr, size, outs.syndrome_ptr, outs.hyp_ptr, outs.located_ptr, outs.counts_ptr, repair,
                                  torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                syn, hyp, loc, counts = outs.read()
                for got, want, name in ((syn, syn_w, "syndrome"), (hyp, hyp_w, "hyp"), (loc, loc_w, "located")):
                    diff = np.flatnonzero(got != want)
                    assert diff.size == 0, f"tile mode {mode}: {name} of stripes {diff[:8]} got {got[diff[:8]]} want {want[diff[:8]]}"
                assert counts.tolist() == counts_w, f"tile mode {mode}: counts {counts}"
                if not repair:
                    assert torch.equal(data, d0) and torch.equal(par, p0), f"tile mode {mode}: the call wrote into the shards"
            # repaired: the located stripes hold the encode's bytes again, the LOCATE_MANY ones are as they were
            many = torch.from_numpy(np.flatnonzero(loc_w == MANY)).cuda()
            good_d[many], good_p[many] = d0[many], p0[many]
            assert torch.equal(data, good_d) and torch.equal(par, good_p)
    finally:
        E.set_tile_sharing(mode0)
