"""GPU: lsec_update_dev_masked / lsec_update_dev_masked_rotated, the parity update with a changed set per
stripe (one 64-bit word per stripe in device memory, fresh buffers by logical chunk id).

Bar: bit-exact.  The yardstick is the reference, never the engine: the expected stripes after a call are
test_gpu_check.ref_encode (oracle/_ref when it is built, else the oracle restatement) over the data with
the chunks of each stripe's effective mask replaced, computed on the CPU; for the rotated call the logical
stripes are put on the devices by the numpy permutation of test_gpu_rotated_scrub.physical.  Only the
n_shift = 0 test and the composition test also compare engine with engine, and say so.

Shards (devices) live in the arenas of tests/layouts.py (canary gaps and guard bands), the k fresh chunks
in a second arena of the same kind.  One column (DISABLED) has no fresh buffer: fresh[j].base = NULL.  In
the unrotated call its shard ref points into a third arena of random bytes, the decoys.  The masks sit in
a buffer of 64-bit words with canary words on both sides.  After every call
  * the whole shard arena equals the expected image: parity from the reference, the changed chunks fresh
    with LSEC_UPDATE_STORE and old without, every other chunk, gap and guard band unchanged,
  * the fresh arena, the decoys and the mask buffer are unchanged,
  * the launch record names the predicted form once per launch.

Seven stripes, whose masks are: bit 0; bit k-1; 0 (the stripe is left alone); all k bits (k = 64: the
all-ones word); two bits; one valid bit and garbage at and above bit k (k = 64: bits 3 and 63); one
enabled bit and the bit of the column that is not enabled.  Unsplit and in launches of 3, 3 and 1 stripes,
so the mask pointer and rot0 cross two launch boundaries.  Shapes as test_gpu_update.shapes derives them
from the form that runs.
"""
import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_rotated_scrub as TR

pytestmark = pytest.mark.gpu

CODES = dict(TC.CODES, rs642=(L.REED_SOL_VAN, 64, 2, 0))  # + the widest word: column 63
ALL = ("rs63", "rs164", "raid4_61", "r6_62", "rs128", "rs52", "rs642", "cg63", "co42", "cg164")
ROTATED = ("rs63", "rs164", "rs128", "cg63", "cg164")
LAYOUTS = ("packed", "off8", "mixed")
NSTRIPES, SPLIT = 7, 3  # split: launches of 3, 3 and 1 stripes
DISABLED = 1            # the column without a fresh buffer (every code here has k >= 4)
FIRST_BIG = 3_000_000_007
CANARY64 = 0x5EED5EED5EED5EED
ALL_ONES = (1 << 64) - 1

_after = {}


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES, or the tuple itself (tests/scrub_forms.py's plans)"""
    return CODES[code] if isinstance(code, str) else tuple(code)


def sliced(code):
    return spec(code)[3] != 0


def form_of(code, packet, size):
    _, k, m, _ = spec(code)
    return E.predict_masked_form(2 if sliced(code) else 1, k, m, packet, size)


def shapes(code):
    """(packet, C): the smallest sizes at which the form that runs can go wrong"""
    if not sliced(code):
        f = form_of(code, 0, 8192)
        tile = 256 * 4 * f.VW * f.IT  # bytes of a chunk per tile, from the form built
        return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]
    out = [(8, 64), (8, 64 * 161), (512, 8 * 512 * 3)]
    if form_of(code, 64, 8 * 64 * 65).DW == 4:
        out.append((64, 8 * 64 * 65))  # a 4 KiB tile: 65 super-packets make 4160 bytes
    return out


def masks_of(k):
    """the seven words"""
    low = (1 << k) - 1
    junk = ((0xDEADBEEFCAFF << k) | (1 << 63)) & ALL_ONES & ~low if k < 64 else 1 << 63
    m = [1, 1 << (k - 1), 0, ALL_ONES if k == 64 else low, 1 | 1 << (k - 2), 1 << 3 | junk, 1 << 2 | 1 << DISABLED]
    assert len(m) == NSTRIPES
    return m


def effective(k, masks, disabled=(DISABLED,)):
    """[[j, ...] per stripe]: the set bits below k of the enabled columns"""
    return [[j for j in range(k) if w >> j & 1 and j not in disabled] for w in masks]


def fresh_chunks(code, packet, size):
    _, k, _, _ = spec(code)
    rng = np.random.default_rng([k, packet, size, 77])
    return rng.integers(0, 256, (NSTRIPES, k, size), dtype=np.uint8)


def updated(code, packet, full, sets, fresh):
    """the logical stripes [N, k+m, C] the reference has after the write: each stripe's chunks `sets[s]` replaced,
    its encode; a stripe with an empty set as it was"""
    _, k, _, _ = spec(code)
    out = full.copy()
    for s, cols in enumerate(sets):
        if not cols:
            continue
        for j in cols:
            out[s, j] = fresh[s, j]
        out[s, k:] = TC.ref_encode(spec(code), packet, out[s, :k])
    return out


def after_write(code, packet, size):
    """(fresh, the reference's stripes after the masked write of the consistent stripes); once per shape, never modified"""
    key = (code, packet, size)
    if key not in _after:
        _, k, _, _ = spec(code)
        fresh = fresh_chunks(code, packet, size)
        u = updated(code, packet, TC.stripes(spec(code), packet, size, NSTRIPES), effective(k, masks_of(k)), fresh)
        fresh.setflags(write=False)
        u.setflags(write=False)
        _after[key] = (fresh, u)
    return _after[key]


class Masks:
    """[4 canaries | nstripes words | 4 canaries] of 64 bits in device memory"""

    def __init__(self, torch, words):
        self.n = len(words)
        self.host = np.array([CANARY64] * 4 + [int(w) for w in words] + [CANARY64] * 4, dtype=np.uint64)
        self.dev = torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        self.ptr = self.dev.data_ptr() + 32
        assert self.ptr % 8 == 0

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.host)


class Bench:
    """consistent stripes (rotated: on the devices of a rotated LUN) in an arena, the k fresh chunks in a second one,
    decoys behind the ref of the column that is not enabled (unrotated), the masks, a plan"""

    def __init__(self, torch, code, packet, size, layout, rotated=False, masks=None, fresh=None):
        self.torch, self.code, self.packet, self.size, self.rotated = torch, code, packet, size, rotated
        _, self.k, self.m, _ = spec(code)
        k, m = self.k, self.m
        self.n = k + m
        self.full = TC.stripes(spec(code), packet, size, NSTRIPES)
        self.words = masks_of(k) if masks is None else list(masks)
        self.fresh = after_write(code, packet, size)[0] if fresh is None else fresh
        self.lay = LY.plan_layout(layout, k, m, NSTRIPES, size, outputs=range(k, k + m))
        self.flay = LY.plan_layout(layout, k, 0, NSTRIPES, size)
        LY.check_layout(self.lay)
        LY.check_layout(self.flay)
        self.arena, self.real_refs, _ = LY.to_device(torch, self.lay, np.full(self.lay.total, LY.GARBAGE, np.uint8))
        self.fbefore = LY.images(self.flay, self.fresh, ())[0]
        self.farena, fresh_refs, _ = LY.to_device(torch, self.flay, self.fbefore)
        self.fresh_refs = [(0, 0) if j == DISABLED else fresh_refs[j] for j in range(k)]
        rng = np.random.default_rng(size + 7)
        self.dbefore = rng.integers(0, 256, self.lay.total, dtype=np.uint8)
        self.darena, decoys, _ = LY.to_device(torch, self.lay, self.dbefore)
        # rotated: every device is real; unrotated: the column that is not enabled has a decoy behind its ref
        self.refs = list(self.real_refs) if rotated else [decoys[i] if i == DISABLED else self.real_refs[i] for i in range(k + m)]
        self.masks = Masks(torch, self.words)
        self.plan = TC.make_plan(spec(code), packet, size)
        self.form = form_of(code, packet, size)
        self.tag = f"{code} packet={packet} C={size} {layout}" + (" rotated" if rotated else "")

    def close(self):
        self.plan.close()

    def image(self, logical, n_shift=0, first=0):
        """the arena holding the logical stripes [N, k+m, C] (rotated: on the devices of that rotation)"""
        return LY.images(self.lay, TR.physical(logical, n_shift, first) if self.rotated else logical, ())[0]

    def arm(self, image):
        self.arena.copy_(self.torch.from_numpy(image))

    def call(self, store, n_shift=0, first=0, masks=None, stream=None, refs=None):
        st = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        ptr = (self.masks if masks is None else masks).ptr
        refs = self.refs if refs is None else refs
        if self.rotated:
            self.plan.update_dev_masked_rotated_refs(refs, NSTRIPES, self.size, n_shift, first, ptr, self.fresh_refs, store, st)
        else:
            self.plan.update_dev_masked_refs(refs, NSTRIPES, self.size, ptr, self.fresh_refs, store, st)

    def got(self, masks=()):
        """the arena after the call; the fresh arena, the decoys and the masks must be as they were"""
        self.torch.cuda.synchronize()
        assert np.array_equal(self.farena.cpu().numpy(), self.fbefore), f"{self.tag}: the call wrote into the fresh chunks"
        assert np.array_equal(self.darena.cpu().numpy(), self.dbefore), f"{self.tag}: the call wrote into a decoy"
        for mk in (self.masks, *masks):
            assert mk.unchanged(), f"{self.tag}: the call wrote into the mask array"
        return self.arena.cpu().numpy()

    def want(self, store, after):
        """the logical stripes the arena must hold: the reference's after the write; without the flag the old data stay"""
        u = after.copy()
        if not store:
            u[:, :self.k] = self.full[:, :self.k]
        return u

    def run(self, store, after, n_shift=0, first=0, split=0, stream=None):
        what = f"{self.tag} store={store} n_shift={n_shift} first={first} split={split}"
        self.arm(self.image(self.full, n_shift, first))
        if stream is not None:
            self.torch.cuda.synchronize()
        E.set_pattern_split(split)
        try:
            self.call(store, n_shift, first, stream=stream)
        finally:
            E.set_pattern_split(0)
        forms = E.launch_record()
        got = self.got()
        LY.assert_arena(self.lay, got, self.image(self.want(store, after), n_shift, first), what)
        launches = 1 if not split else -(-NSTRIPES // split)
        assert forms == [self.form] * launches, (what, forms, self.form)
        return got


def test_the_masks_are_what_the_file_says():
    for k in (4, 6, 16, 64):
        w = masks_of(k)
        eff = effective(k, w)
        assert eff[0] == [0] and eff[1] == [k - 1] and eff[2] == []
        assert eff[3] == [j for j in range(k) if j != DISABLED]
        assert eff[4] == [0, k - 2] and eff[6] == [2]
        assert eff[5] == ([3] if k < 64 else [3, 63])
        assert all(0 <= x <= ALL_ONES for x in w)
        if k < 64:
            assert w[5] >> k != 0 and w[5] >> 63 == 1  # garbage at and above bit k
        else:
            assert w[3] == ALL_ONES and w[1] == 1 << 63


# ---------------------------------------------------------------- 1. the unrotated call
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", ALL)
def test_update_masked(cuda, code, layout):
    import torch

    for packet, size in shapes(code):
        _, after = after_write(code, packet, size)
        bench = Bench(torch, code, packet, size, layout)
        try:
            for store in (False, True):
                bench.run(store, after)
                bench.run(store, after, split=SPLIT)  # crosses two launch boundaries
        finally:
            bench.close()


# ---------------------------------------------------------------- 2. over the devices of a rotated LUN
def rotations(n):
    """n_shift 0, 1 and one beyond k+m (taken mod k+m), first stripes 5 and one beyond 32 bits"""
    return [(0, FIRST_BIG), (1, 5), (1, FIRST_BIG), (n + 1, FIRST_BIG)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", ROTATED)
def test_update_masked_rotated(cuda, code, layout):
    import torch

    for packet, size in shapes(code):
        _, after = after_write(code, packet, size)
        bench = Bench(torch, code, packet, size, layout, rotated=True)
        try:
            for n_shift, first in rotations(bench.n):
                for store in (False, True):
                    bench.run(store, after, n_shift, first)
            bench.run(True, after, 1, FIRST_BIG, split=SPLIT)
            bench.run(False, after, bench.n + 1, FIRST_BIG, split=SPLIT)
        finally:
            bench.close()


@pytest.mark.parametrize("code", ROTATED)
def test_unrotated_devices_are_the_unrotated_call(cuda, code):
    """engine against engine (and both against the reference): at n_shift = 0 the rotated call leaves the bytes the
    unrotated call leaves over the same refs"""
    import torch

    for packet, size in shapes(code)[-2:]:
        _, after = after_write(code, packet, size)
        rot = Bench(torch, code, packet, size, "off8", rotated=True)
        flat = Bench(torch, code, packet, size, "off8")
        try:
            for store in (False, True):
                a = rot.run(store, after, 0, FIRST_BIG)
                b = flat.run(store, after)
                assert np.array_equal(a, b), (rot.tag, store)
        finally:
            rot.close()
            flat.close()


# ---------------------------------------------------------------- 3. a stream of its own, the torch form
@pytest.mark.parametrize("code", ["rs63", "cg164"])
def test_on_a_stream_of_its_own(cuda, code):
    import torch

    packet, size = shapes(code)[-1]
    _, after = after_write(code, packet, size)
    for rotated in (False, True):
        bench = Bench(torch, code, packet, size, "off8", rotated=rotated)
        try:
            st = torch.cuda.Stream()
            bench.run(True, after, 1 if rotated else 0, FIRST_BIG if rotated else 0, stream=st.cuda_stream)
            bench.run(False, after, 1 if rotated else 0, FIRST_BIG if rotated else 0, split=SPLIT, stream=st.cuda_stream)
        finally:
            bench.close()


def test_torch_form(cuda):
    import torch

    code, size = "rs63", 4096
    _, k, m, _ = spec(code)
    full = TC.stripes(spec(code), 0, size, NSTRIPES)
    fresh = fresh_chunks(code, 0, size)
    words = masks_of(k)
    want = updated(code, 0, full, effective(k, words, disabled=()), fresh)  # every column has a fresh buffer here
    for store in (False, True):
        data, par = torch.from_numpy(full[:, :k].copy()).cuda(), torch.from_numpy(full[:, k:].copy()).cuda()
        f = torch.from_numpy(fresh.copy()).cuda()
        cols = torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).cuda()
        with TC.make_plan(spec(code), 0, size) as p:
            p.update_dev_masked(data, par, cols, f, store=store)
            torch.cuda.synchronize()
        assert np.array_equal(par.cpu().numpy(), want[:, k:])
        assert np.array_equal(data.cpu().numpy(), want[:, :k] if store else full[:, :k])
        assert np.array_equal(f.cpu().numpy(), fresh)
        assert np.array_equal(cols.cpu().numpy().view(np.uint64), np.array(words, dtype=np.uint64))


# ---------------------------------------------------------------- 4. syndrome preservation
SYNDROME_CASES = [(c, False) for c in ("rs63", "rs164", "raid4_61", "r6_62", "cg63", "cg164")] + \
                 [(c, True) for c in ("rs63", "rs164", "cg63", "cg164")]


@pytest.mark.parametrize("code,rotated", SYNDROME_CASES, ids=[c + ("-rotated" if r else "") for c, r in SYNDROME_CASES])
def test_keeps_the_syndrome_of_an_inconsistent_stripe(cuda, code, rotated):
    """two of the seven stripes are inconsistent before the write: a flipped byte in a parity row of stripe 1 (whose
    chunk k-1 changes) and in data chunk k-1 of stripe 4 (whose chunks 0 and k-2 change).  The check's words over the
    stripes with the chunks replaced are, after the update, the CPU-expected ones -- the reference's re-encode of
    the data as stored after the update against the stored parity -- and the words the check gave before it."""
    import torch

    _, k, m, _ = spec(code)
    n = k + m
    packet, size = shapes(code)[-1]
    n_shift, first = (1, FIRST_BIG) if rotated else (0, 0)
    bench = Bench(torch, code, packet, size, "mixed", rotated=rotated)
    words = TC.Words(torch, NSTRIPES)
    stream = torch.cuda.current_stream().cuda_stream
    sets = effective(k, bench.words)

    def check():
        words.arm()
        if rotated:
            bench.plan.check_dev_rotated_refs(bench.real_refs, NSTRIPES, size, n_shift, first, words.syndrome_ptr, words.bad_ptr, stream)
        else:
            bench.plan.check_dev_refs(bench.real_refs, NSTRIPES, size, words.syndrome_ptr, words.bad_ptr, stream)
        torch.cuda.synchronize()
        return words.read()[0]

    def logical_view(arena):
        """[N, k+m, C]: what the arena holds, as logical chunks"""
        out = np.empty_like(bench.full)
        for s in range(NSTRIPES):
            rot = TR.rot_of(n, n_shift, first, s) if rotated else 0
            for c in range(n):
                a = bench.lay.start((c - rot) % n, s)
                out[s, c] = arena[a:a + size]
        return out

    try:
        logical = bench.full.copy()
        logical[1, n - 1, size - 1] ^= TC.FLIP
        logical[4, k - 1, size // 2] ^= TC.FLIP
        for store in (True, False):
            bench.arm(bench.image(logical, n_shift, first))
            old = check()
            assert [int(w != 0) for w in old] == [0, 1, 0, 0, 1, 0, 0], old
            bench.call(store, n_shift, first)
            stored = logical_view(bench.got())
            if not store:  # the caller puts the fresh bytes in place itself
                assert np.array_equal(stored[:, :k], logical[:, :k])
                for s, cols in enumerate(sets):
                    for j in cols:
                        stored[s, j] = bench.fresh[s, j]
                bench.arm(bench.image(stored, n_shift, first))
            for s, cols in enumerate(sets):
                for j in range(k):
                    assert np.array_equal(stored[s, j], bench.fresh[s, j] if j in cols else logical[s, j]), (s, j)
            new = check()
            want = np.array([TC.expected_mask(spec(code), packet, stored[s]) for s in range(NSTRIPES)], np.uint32)
            assert np.array_equal(new, want), (store, new, want)
            assert np.array_equal(new, old), (store, new, old)
    finally:
        bench.close()


# ---------------------------------------------------------------- 5. composition
@pytest.mark.parametrize("code", ["rs63", "rs164", "rs642", "cg63"])
def test_two_calls_compose(cuda, code):
    """masks A, then masks B disjoint from A in every stripe, leave what one call with A | B leaves (engine against
    engine, and both against the reference): A the even bits of the seven words, B the odd ones"""
    import torch

    packet, size = shapes(code)[-1]
    _, after = after_write(code, packet, size)
    bench = Bench(torch, code, packet, size, "packed")
    even = 0x5555555555555555
    a = Masks(torch, [w & even for w in bench.words])
    b = Masks(torch, [w & ~even & ALL_ONES for w in bench.words])
    try:
        for store in (False, True):
            once = bench.run(store, after)
            bench.arm(bench.image(bench.full))
            bench.call(store, masks=a)
            bench.call(store, masks=b)
            got = bench.got((a, b))
            LY.assert_arena(bench.lay, got, bench.image(bench.want(store, after)), f"two calls {bench.tag} store={store}")
            assert np.array_equal(got, once)
    finally:
        bench.close()
