"""Shard layouts for the device-resident calls: one arena holding all k+m shards of N stripes.

The C ABI takes every shard as lsec_shard_t {base, stride}; its only rule is that bases and
strides are multiples of 8 bytes.  ``plan_layout`` places the shards of one call in an arena by a
named layout, ``images`` gives the arena before the call and as it must be after it, and
``assert_arena`` compares the whole arena: outputs against the reference, and every input, every
gap and both guard bands unchanged.

Layouts (C = chunk size; a shard's region holds its N chunks `stride` bytes apart):

* ``packed``       LStore's own: data base = D + i*C, stride = k*C; parity base = P + i*C,
                   stride = m*C; no gaps inside a stripe.  With C % 16 == 8 every odd shard sits at
                   base % 16 == 8.
* ``off8``         every shard in a region of its own at base % 16 == 8, stride = C + 40 (with
                   C % 16 == 0 successive stripes alternate between 8 and 0 mod 16; with
                   C % 16 == 8 every stripe sits at 8).
* ``mixed``        inputs at base % 16 == 0, outputs at base % 16 == 8 (``mixed_swapped``: the other
                   way round); strides differ per shard: C + 8, C + 24, C + 4096 + 8, 2*C + 16.
* ``aligned_gap``  base % 256 == 0, stride = C + 4096 rounded up to 16: everything 16-byte aligned,
                   nothing contiguous.

At least GUARD bytes of canary precede the first chunk and follow the last, so an access a few
lanes too wide stays inside the allocation: these tests cannot fault.  Only numpy here; torch is
the caller's (``to_device``).
"""
import numpy as np

CANARY, GARBAGE = 0xC3, 0xA5
GUARD = 4096
LAYOUTS = ("packed", "off8", "mixed", "mixed_swapped", "aligned_gap")
MIXED_STRIDES = (lambda c: c + 8, lambda c: c + 24, lambda c: c + 4096 + 8, lambda c: 2 * c + 16)


def _up(x, a):
    return (x + a - 1) // a * a


class Layout:
    """offsets[i], strides[i]: shard i's chunk of stripe s is arena[offsets[i] + s*strides[i]:][:C];
    magic_off: offset of the 4*N magic bytes (None without one); total: arena bytes"""

    def __init__(self, name, k, m, nstripes, size, offsets, strides, total, magic_off):
        self.name, self.k, self.m, self.n, self.nstripes, self.size = name, k, m, k + m, nstripes, size
        self.offsets, self.strides, self.total, self.magic_off = list(offsets), list(strides), total, magic_off
        # chunk starts in arena order, for naming a byte's place
        at = [(self.start(i, s), s, i) for i in range(self.n) for s in range(nstripes)]
        at.sort()
        self._starts = np.array([a[0] for a in at], np.int64)
        self._slots = [(a[1], a[2]) for a in at]

    def start(self, i, s):
        return self.offsets[i] + s * self.strides[i]

    def refs(self, base_ptr):
        return [(base_ptr + o, st) for o, st in zip(self.offsets, self.strides)]

    def place(self, pos):
        """(stripe, shard, byte, in_gap): the chunk holding arena byte pos, or (in_gap) the last chunk
        that starts before it, `byte` then counting from that chunk's start (>= C); a byte before
        the first chunk: (-1, -1, pos, True)"""
        j = int(np.searchsorted(self._starts, pos, side="right")) - 1
        if j < 0:
            return -1, -1, int(pos), True
        s, i = self._slots[j]
        b = int(pos - self._starts[j])
        return s, i, b, b >= self.size


def plan_layout(name, k, m, nstripes, size, outputs=(), magic=False):
    """Place k+m shards of nstripes chunks of `size` bytes; `outputs`: the shard ids the call writes
    (only the mixed layouts look at them)."""
    n, cur = k + m, GUARD
    offsets, strides = [0] * n, [0] * n
    if name == "packed":
        for i in range(k):
            offsets[i], strides[i] = cur + i * size, k * size
        cur = _up(cur + nstripes * k * size, 256) + 256
        for i in range(m):
            offsets[k + i], strides[k + i] = cur + i * size, m * size
        cur += nstripes * m * size
    elif name in ("off8", "mixed", "mixed_swapped", "aligned_gap"):
        for i in range(n):
            cur = _up(cur, 256)
            if name == "off8":
                off, st = 8, size + 40
            elif name == "aligned_gap":
                off, st = 0, _up(size, 16) + 4096
            else:
                off = 8 if (i in outputs) != (name == "mixed_swapped") else 0
                st = MIXED_STRIDES[i % 4](size)
            offsets[i], strides[i] = cur + off, st
            cur = offsets[i] + (nstripes - 1) * st + size + 64
    else:
        raise ValueError(name)
    magic_off = None
    if magic:
        magic_off = _up(cur, 256) + 256
        cur = magic_off + 4 * nstripes
    return Layout(name, k, m, nstripes, size, offsets, strides, _up(cur, 256) + GUARD, magic_off)


def images(lay, chunks, outputs, keep=(), magic=None):
    """chunks uint8 [N, k+m, C]: every chunk as the reference has it.  Returns (before, want), both
    the whole arena: gaps hold CANARY; the slots of `outputs` hold GARBAGE in `before` and the
    reference bytes in `want`, except those of `keep` (outputs the call must leave alone), which
    keep their garbage; everything else is the same in both.  magic uint8 [N, 4]: the bytes `want`
    holds at magic_off (`before`: CANARY)."""
    assert chunks.shape == (lay.nstripes, lay.n, lay.size)
    want = np.full(lay.total, CANARY, np.uint8)
    for i in range(lay.n):
        for s in range(lay.nstripes):
            a = lay.start(i, s)
            want[a:a + lay.size] = chunks[s, i]
    before = want.copy()
    for i in outputs:
        for s in range(lay.nstripes):
            a = lay.start(i, s)
            before[a:a + lay.size] = GARBAGE
            if i in keep:
                want[a:a + lay.size] = GARBAGE
    if magic is not None:
        want[lay.magic_off:lay.magic_off + 4 * lay.nstripes] = np.asarray(magic, np.uint8).reshape(-1)
    return before, want


def check_layout(lay):
    """what every layout promises: 8-byte bases and strides, disjoint regions, guard bands"""
    spans = []
    for i in range(lay.n):
        assert lay.offsets[i] % 8 == 0 and lay.strides[i] % 8 == 0, (lay.name, i)
        assert lay.strides[i] >= lay.size
        for s in range(lay.nstripes):
            spans.append((lay.start(i, s), lay.start(i, s) + lay.size))
    if lay.magic_off is not None:
        spans.append((lay.magic_off - 64, lay.magic_off + 4 * lay.nstripes + 64))  # a canary region of its own
    spans.sort()
    assert spans[0][0] >= GUARD and spans[-1][1] + GUARD <= lay.total
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{lay.name}: regions overlap at {b0}"


def to_device(torch, lay, before):
    """(arena, refs, magic_ptr): `before` in device memory, the arena's first byte 256-byte aligned"""
    raw = torch.empty(lay.total + 256, dtype=torch.uint8, device="cuda")
    skip = -raw.data_ptr() % 256
    arena = raw[skip:skip + lay.total]
    arena.copy_(torch.from_numpy(before))
    base = arena.data_ptr()
    assert base % 256 == 0
    return arena, lay.refs(base), (None if lay.magic_off is None else base + lay.magic_off)


def assert_arena(lay, got, want, what):
    """the whole arena equals `want`, or an AssertionError naming where it does not: per chunk
    (stripe, shard, first and last differing byte), per gap the chunk it follows"""
    if np.array_equal(got, want):
        return
    d = np.flatnonzero(got != want)
    chunks, gaps = {}, {}
    for pos in d[:4096]:
        s, i, b, gap = lay.place(pos)
        if lay.magic_off is not None and lay.magic_off <= pos < lay.magic_off + 4 * lay.nstripes:
            key, tab, b = ("magic", int(pos - lay.magic_off) // 4), chunks, int(pos - lay.magic_off) % 4
        else:
            key, tab = (s, i), (gaps if gap else chunks)
        lo, hi = tab.get(key, (b, b))
        tab[key] = (min(lo, b), max(hi, b))
    parts = [f"stripe {k[0]} shard {k[1]} bytes [{lo}, {hi}]" if k[0] != "magic" else f"magic of stripe {k[1]} bytes [{lo}, {hi}]"
             for k, (lo, hi) in sorted(chunks.items(), key=str)[:8]]
    parts += [f"gap after stripe {s} shard {i}: bytes [{lo}, {hi}] from its start (chunk is {lay.size})" if s >= 0
              else f"gap before the first chunk: arena bytes [{lo}, {hi}]" for (s, i), (lo, hi) in sorted(gaps.items())[:8]]
    raise AssertionError(f"{what} ({lay.name}): {len(d)} bytes differ: " + "; ".join(parts))
