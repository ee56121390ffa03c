"""GPU: lsec_encode_dev_rotated / lsec_update_dev_rotated, the write side over the physical devices of a
rotated LUN.

Bar: bit-exact.  The yardstick is the reference, never the engine: logical stripes come from
test_gpu_check.stripes() (oracle/_ref when it is built, else the oracle restatement), the expected parity
of a stripe after a write is test_gpu_check.ref_encode of its data with the chunks replaced, computed on
the CPU, and the logical stripes are rotated onto the devices on the host by the numpy permutation of
test_gpu_rotated_scrub.physical.  Only test_unrotated_encode_is_encode_dev and the tile-sharing test
compare engine with engine, and say so.

Devices live in the arenas of tests/layouts.py (canary gaps and guard bands), shard i of the layout as
device i; the fresh chunks in a second arena of the same kind.  After every call the WHOLE device arena
equals the expected image -- parity at the rotated positions, the changed chunks fresh with
LSEC_UPDATE_STORE and old without, every other chunk, every gap and both guard bands unchanged -- the
fresh arena is unchanged, and the launch record names the predicted form once per launch.

Stripes per call: k + m + 2, so the rotation wraps.  Sizes: a single unit, a ragged tile, more than one
tile (test_gpu_rotated_scrub's); shifts 0, 1, one sharing a factor with k + m, k + m + 1; first stripes
5 and one beyond 32 bits.
"""
import numpy as np
import pytest

from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_rotated_scrub as TR

pytestmark = pytest.mark.gpu

BYTEWISE = ("rs63", "r6_62", "rs52", "rs128", "rs164", "raid4_61")  # raid4: one row, 8 B per lane, per-cell branches
SLICED = ("cg63", "cg164")
CODES = {c: TC.CODES[c] for c in BYTEWISE + SLICED}
BYTEWISE_SIZES = ((0, 8), (0, 8200), (0, 24584))
SLICED_SIZES = {"cg63": ((8, 64), (8, 64 * 161)), "cg164": ((8, 64), (8, 64 * 161), (64, 8 * 64 * 65))}
FIRSTS = (5, 3_000_000_007)
LAYOUTS = ("packed", "off8", "mixed")
SPLIT = 3
NOISE = 0x9D

_updated = {}


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES, or the tuple itself (tests/scrub_forms.py's plans)"""
    return CODES[code] if isinstance(code, str) else tuple(code)


def shapes(code):
    return list(SLICED_SIZES[code] if code in SLICED else BYTEWISE_SIZES)


def geometry(code):
    _, k, m, _ = spec(code)
    return k, m, k + m, k + m + 2


def shifts(n):
    """0: lsec_encode_dev's behaviour; 1: every rotation; the smallest divisor of n above 1 (n itself where n is
    prime: the shift that is 0 mod n); n + 1: taken mod n"""
    return (0, 1, next(d for d in range(2, n + 1) if n % d == 0), n + 1)


def rotations(n):
    return [(n_shift, first) for n_shift in shifts(n) for first in FIRSTS]


def col_lists(code):
    k = spec(code)[1]
    return [(0,), (k - 1,), (k - 2, 1), tuple(range(k))]


def form_of(family, code, packet, size):
    _, k, m, _ = spec(code)
    return E.predict_form(family, 2 if spec(code)[3] else 1, k, m, packet, size)


def fresh_chunks(code, packet, size, cols):
    k, _, _, nstripes = geometry(code)
    rng = np.random.default_rng([k, packet, size, *cols])
    return rng.integers(0, 256, (nstripes, len(cols), size), dtype=np.uint8)


def updated(code, packet, full, cols, fresh):
    """the logical stripes [N, k+m, C] the reference has after the write: data with the chunks replaced, its encode"""
    k = spec(code)[1]
    out = full.copy()
    for i, j in enumerate(cols):
        out[:, j] = fresh[:, i]
    for s in range(full.shape[0]):
        out[s, k:] = TC.ref_encode(spec(code), packet, out[s, :k])
    return out


def updated_consistent(code, packet, size, cols):
    """(fresh, the reference's stripes after the write) of the consistent stripes; computed once, never modified"""
    key = (code, packet, size, tuple(cols))
    if key not in _updated:
        nstripes = geometry(code)[3]
        fresh = fresh_chunks(code, packet, size, cols)
        u = updated(code, packet, TC.stripes(spec(code), packet, size, nstripes), cols, fresh)
        fresh.setflags(write=False)
        u.setflags(write=False)
        _updated[key] = (fresh, u)
    return _updated[key]


class Bench:
    """the devices of a rotated LUN in one arena, a plan, and (for the update) the fresh chunks in a second arena"""

    def __init__(self, torch, code, packet, size, layout, cols=None, fresh=None):
        self.torch, self.code, self.packet, self.size = torch, code, packet, size
        self.k, self.m, self.n, self.nstripes = geometry(code)
        self.full = TC.stripes(spec(code), packet, size, self.nstripes)
        self.lay = LY.plan_layout(layout, self.k, self.m, self.nstripes, size, outputs=range(self.k, self.n))
        LY.check_layout(self.lay)
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, np.full(self.lay.total, LY.GARBAGE, np.uint8))
        self.plan = TC.make_plan(spec(code), packet, size)
        self.tag = f"{code} packet={packet} C={size} {layout}"
        if cols is not None:
            self.cols = tuple(cols)
            self.fresh = fresh_chunks(code, packet, size, cols) if fresh is None else fresh
            self.flay = LY.plan_layout(layout, len(cols), 0, self.nstripes, size)
            LY.check_layout(self.flay)
            self.fbefore = LY.images(self.flay, self.fresh, ())[0]
            self.farena, self.fresh_refs, _ = LY.to_device(torch, self.flay, self.fbefore)

    def close(self):
        self.plan.close()

    def image(self, logical, n_shift, first):
        """the arena holding the logical stripes [N, k+m, C] on the devices of that rotation"""
        return LY.images(self.lay, TR.physical(logical, n_shift, first), ())[0]

    def arm(self, image):
        self.arena.copy_(self.torch.from_numpy(image))

    def stream(self, stream):
        return self.torch.cuda.current_stream().cuda_stream if stream is None else stream

    def encode(self, n_shift, first, stream=None):
        self.plan.encode_dev_rotated_refs(self.refs, self.nstripes, self.size, n_shift, first, self.stream(stream))

    def update(self, n_shift, first, store, idx=None, stream=None):
        idx = range(len(self.cols)) if idx is None else idx
        self.plan.update_dev_rotated_refs(self.refs, self.nstripes, self.size, n_shift, first, [self.cols[i] for i in idx],
                                          [self.fresh_refs[i] for i in idx], store, self.stream(stream))

    def got(self):
        self.torch.cuda.synchronize()
        if hasattr(self, "farena"):
            assert np.array_equal(self.farena.cpu().numpy(), self.fbefore), f"{self.tag}: the call wrote into the fresh chunks"
        return self.arena.cpu().numpy()

    def noisy(self):
        """the logical stripes with noise where the parity belongs"""
        v = self.full.copy()
        v[:, self.k:] = NOISE
        return v

    def launches(self, family, split=0):
        n = 1 if not split else -(-self.nstripes // split)
        return [form_of(family, self.code, self.packet, self.size)] * n

    def run_encode(self, n_shift, first, split=0, stream=None):
        what = f"encode {self.tag} n_shift={n_shift} first={first} split={split}"
        self.arm(self.image(self.noisy(), n_shift, first))
        E.set_pattern_split(split)
        try:
            self.encode(n_shift, first, stream)
        finally:
            E.set_pattern_split(0)
        forms = E.launch_record()
        got = self.got()
        LY.assert_arena(self.lay, got, self.image(self.full, n_shift, first), what)
        assert forms == self.launches("encrot", split), (what, forms)
        return got

    def want_update(self, store, after):
        u = after.copy()
        if not store:
            u[:, :self.k] = self.full[:, :self.k]
        return u

    def run_update(self, n_shift, first, store, after, split=0, stream=None):
        """`after`: the reference's logical stripes after the write"""
        what = f"update {self.tag} cols={self.cols} store={store} n_shift={n_shift} first={first} split={split}"
        self.arm(self.image(self.full, n_shift, first))
        E.set_pattern_split(split)
        try:
            self.update(n_shift, first, store, stream=stream)
        finally:
            E.set_pattern_split(0)
        forms = E.launch_record()
        got = self.got()
        LY.assert_arena(self.lay, got, self.image(self.want_update(store, after), n_shift, first), what)
        assert forms == self.launches("updrot", split), (what, forms)
        return got


# ---------------------------------------------------------------- 1. encode
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", list(CODES))
def test_encode(cuda, code, layout):
    """random logical data on the devices, noise where the parity belongs: one call leaves the reference's parity
    at the rotated positions and everything else as it was"""
    import torch

    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, layout)
        try:
            for n_shift, first in rotations(bench.n):
                bench.run_encode(n_shift, first)
        finally:
            bench.close()


# ---------------------------------------------------------------- 2. n_shift = 0
@pytest.mark.parametrize("code", ["rs63", "rs128", "raid4_61", "cg63", "cg164"])
def test_unrotated_encode_is_encode_dev(cuda, code):
    """engine against engine (and both against the reference): at n_shift = 0 the bytes are lsec_encode_dev's over
    the same refs -- for Cauchy whichever kernel or network that call picks"""
    import torch

    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, "off8")
        try:
            rotated = bench.run_encode(0, FIRSTS[1])
            bench.arm(bench.image(bench.noisy(), 0, 0))
            bench.plan.encode_dev_refs(bench.refs, bench.nstripes, size, torch.cuda.current_stream().cuda_stream)
            assert np.array_equal(bench.got(), rotated), bench.tag
        finally:
            bench.close()


# ---------------------------------------------------------------- 3. update on consistent stripes
@pytest.mark.parametrize("which", range(4), ids=("first", "last", "reverse_pair", "all"))
@pytest.mark.parametrize("code", list(CODES))
def test_update(cuda, code, which):
    import torch

    cols = col_lists(code)[which]
    for packet, size in shapes(code):
        fresh, after = updated_consistent(code, packet, size, cols)
        bench = Bench(torch, code, packet, size, "mixed", cols, fresh)
        try:
            for n_shift, first in rotations(bench.n):
                for store in (False, True):
                    bench.run_update(n_shift, first, store, after)
        finally:
            bench.close()


@pytest.mark.parametrize("layout", ("packed", "off8"))
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_update_in_the_other_layouts(cuda, code, layout):
    import torch

    cols = col_lists(code)[2]
    packet, size = shapes(code)[-1]
    fresh, after = updated_consistent(code, packet, size, cols)
    bench = Bench(torch, code, packet, size, layout, cols, fresh)
    try:
        for store in (False, True):
            bench.run_update(1, FIRSTS[1], store, after)
    finally:
        bench.close()


# ---------------------------------------------------------------- 4. the syndrome is kept
@pytest.mark.parametrize("code", ["rs63", "rs164", "raid4_61", "cg63", "cg164"])
def test_update_keeps_the_syndrome(cuda, code):
    """two stripes are inconsistent before the write: a flipped byte in a parity chunk of one, in a data chunk that
    does not change of the other.  lsec_check_dev_rotated over the devices with the chunks replaced gives after the
    update the CPU-expected words (the reference's re-encode of each stripe's logical view as stored against its
    stored parity), and those are the words it gave before"""
    import torch

    k, m, n, nstripes = geometry(code)
    cols = col_lists(code)[2]
    packet, size = shapes(code)[-1]
    n_shift, first = 1, FIRSTS[1]
    bench = Bench(torch, code, packet, size, "mixed", cols)
    words = TC.Words(torch, nstripes)
    stream = torch.cuda.current_stream().cuda_stream

    def check():
        words.arm()
        bench.plan.check_dev_rotated_refs(bench.refs, nstripes, size, n_shift, first, words.syndrome_ptr, words.bad_ptr, stream)
        torch.cuda.synchronize()
        return words.read()[0]

    try:
        untouched = [j for j in range(k) if j not in cols]
        logical = bench.full.copy()
        logical[1, n - 1, size - 1] ^= TC.FLIP
        logical[3, untouched[-1], size // 2] ^= TC.FLIP
        for store in (True, False):
            bench.arm(bench.image(logical, n_shift, first))
            old = check()
            assert [int(w != 0) for w in old] == [0, 1, 0, 1] + [0] * (nstripes - 4), old
            bench.update(n_shift, first, store)
            stored = logical.copy()
            for i, j in enumerate(cols):
                stored[:, j] = bench.fresh[:, i]
            got = bench.got()
            if not store:  # the caller puts the fresh bytes in place itself
                data = np.concatenate([stored[:, :k], np.zeros((nstripes, m, size), np.uint8)], axis=1)
                mask = np.concatenate([np.ones_like(stored[:, :k]), np.zeros((nstripes, m, size), np.uint8)], axis=1)
                sel = bench.image(mask, n_shift, first) == 1
                got = np.where(sel, bench.image(data, n_shift, first), got)
                bench.arm(got)
            # the logical view of what the devices hold now
            for s in range(nstripes):
                rot = TR.rot_of(n, n_shift, first, s)
                for c in range(k, n):
                    a = bench.lay.start((c - rot) % n, s)
                    stored[s, c] = got[a:a + size]
            assert np.array_equal(got, bench.image(stored, n_shift, first)), "a data chunk is not where the write put it"
            new = check()
            want = np.array([TC.expected_mask(spec(code), packet, stored[s]) for s in range(nstripes)], np.uint32)
            assert np.array_equal(new, want), (store, new, want)
            assert np.array_equal(new, old), (store, new, old)
    finally:
        bench.close()


# ---------------------------------------------------------------- 5. launch split
@pytest.mark.parametrize("code", ["rs63", "rs128", "cg164"])
def test_split_launches(cuda, code):
    """lsec_test_set_pattern_split(3) cuts both calls into launches of three stripes, each with its own rot0 and
    refs: the arenas are those of one launch, and the record names the predicted form once per launch"""
    import torch

    cols = col_lists(code)[2]
    packet, size = shapes(code)[-1]
    fresh, after = updated_consistent(code, packet, size, cols)
    bench = Bench(torch, code, packet, size, "off8", cols, fresh)
    try:
        for n_shift, first in ((1, FIRSTS[0]), (shifts(bench.n)[2], FIRSTS[1]), (bench.n + 1, FIRSTS[1])):
            assert np.array_equal(bench.run_encode(n_shift, first, split=SPLIT), bench.run_encode(n_shift, first))
            for store in (False, True):
                assert np.array_equal(bench.run_update(n_shift, first, store, after, split=SPLIT),
                                      bench.run_update(n_shift, first, store, after))
        assert E.launch_record() == bench.launches("updrot")  # the split is off again
    finally:
        E.set_pattern_split(0)
        bench.close()


# ---------------------------------------------------------------- 6. stream order
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_behind_a_copy_on_a_stream_of_its_own(cuda, code):
    """the calls are enqueued behind a copy_ of their inputs on a non-default stream, nothing waited for in between:
    they see the copied bytes"""
    import torch

    cols = col_lists(code)[2]
    packet, size = shapes(code)[-1]
    n_shift, first = 1, FIRSTS[1]
    fresh, after = updated_consistent(code, packet, size, cols)
    bench = Bench(torch, code, packet, size, "off8", cols, fresh)
    try:
        noisy = torch.from_numpy(bench.image(bench.noisy(), n_shift, first)).cuda()
        consistent = torch.from_numpy(bench.image(bench.full, n_shift, first)).cuda()
        fresh_src = bench.farena.clone()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            bench.arena.copy_(noisy, non_blocking=True)
            bench.encode(n_shift, first, stream=st.cuda_stream)
        LY.assert_arena(bench.lay, bench.got(), bench.image(bench.full, n_shift, first), f"encode on a stream {bench.tag}")
        bench.arena.fill_(LY.GARBAGE)
        bench.farena.fill_(LY.GARBAGE)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            bench.arena.copy_(consistent, non_blocking=True)
            bench.farena.copy_(fresh_src, non_blocking=True)
            bench.update(n_shift, first, True, stream=st.cuda_stream)
        LY.assert_arena(bench.lay, bench.got(), bench.image(after, n_shift, first), f"update on a stream {bench.tag}")
    finally:
        bench.close()


# ---------------------------------------------------------------- 7. round trip
@pytest.mark.parametrize("code", ["rs63", "r6_62", "rs164", "raid4_61", "cg63", "cg164"])
def test_round_trip(cuda, code):
    """lsec_encode_dev_rotated, lsec_update_dev_rotated with LSEC_UPDATE_STORE, lsec_check_dev_rotated: every
    syndrome word is 0 and bad_count is 0 (and the devices hold the reference's stripes after the write)"""
    import torch

    k, m, n, nstripes = geometry(code)
    cols = col_lists(code)[2]
    stream = torch.cuda.current_stream().cuda_stream
    for packet, size in shapes(code)[1:]:
        fresh, after = updated_consistent(code, packet, size, cols)
        bench = Bench(torch, code, packet, size, "mixed", cols, fresh)
        words = TC.Words(torch, nstripes)
        try:
            for n_shift, first in ((shifts(n)[2], FIRSTS[0]), (n + 1, FIRSTS[1])):
                bench.arm(bench.image(bench.noisy(), n_shift, first))
                words.arm()
                bench.encode(n_shift, first)
                bench.update(n_shift, first, True)
                bench.plan.check_dev_rotated_refs(bench.refs, nstripes, size, n_shift, first, words.syndrome_ptr, words.bad_ptr, stream)
                got = bench.got()
                syndrome, bad = words.read()
                assert not syndrome.any() and bad == 0, (bench.tag, n_shift, first, syndrome, bad)
                LY.assert_arena(bench.lay, got, bench.image(after, n_shift, first), f"round trip {bench.tag}")
        finally:
            bench.close()


# ---------------------------------------------------------------- 8. tile sharing
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_tile_sharing_modes(cuda, code):
    """engine against engine: static eighths, shared tiles and the static prefix with a shared tail leave
    identical arenas (each also compared with the reference's)"""
    import torch

    cols = col_lists(code)[2]
    packet, size = shapes(code)[-1]
    n_shift, first = 1, FIRSTS[1]
    fresh, after = updated_consistent(code, packet, size, cols)
    bench = Bench(torch, code, packet, size, "mixed", cols, fresh)
    mode = E.tile_sharing()
    try:
        enc, upd = [], []
        for m in (E.TILES_STATIC, E.TILES_SHARED, E.TILES_TAIL):
            E.set_tile_sharing(m)
            enc.append(bench.run_encode(n_shift, first))
            upd.append(bench.run_update(n_shift, first, True, after))
        for got in (enc, upd):
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    finally:
        E.set_tile_sharing(mode)
        bench.close()
