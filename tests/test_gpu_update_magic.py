"""GPU: lsec_update_magic_dev_masked / lsec_update_magic_dev_masked_rotated, the masked parity update that also
moves each stripe's 4-byte adler32 magic from the old stripe's to the new stripe's.

Bar: bit-exact.  The yardstick is never the engine: the expected magic is zlib.adler32 over the expected
LOGICAL stripe built on the CPU -- the data with each stripe's effective-mask chunks replaced, parity from
test_gpu_check.ref_encode -- and the magic on entry is zlib.adler32 of the old logical stripe.  For the
rotated call the stripes are put on the devices by test_gpu_rotated_scrub.physical; the expected magics are
those of the logical view, whatever the rotation.  Only the last test compares engine with engine, and
says so.

The seven-stripe batch, the mask words, the DISABLED column, the arenas and the canaries are those of
tests/test_gpu_update_masked.py (its Bench, with the call replaced).  The magic words sit in a byte buffer
with canary bytes on both sides.  After every call
  * the magic bytes, and the canaries around them, equal the expected bytes,
  * the shard arena equals the image lsec_update_dev_masked is specified to leave,
  * the fresh arena, the decoys and the masks are unchanged,
  * the launch record names the predicted form of the new family once per launch.
"""
import zlib

import numpy as np
import pytest

from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_rotated_scrub as TR
import test_gpu_update_masked as TM

pytestmark = pytest.mark.gpu

CODES, NSTRIPES, SPLIT, DISABLED, FIRST_BIG = TM.CODES, TM.NSTRIPES, TM.SPLIT, TM.DISABLED, TM.FIRST_BIG
ALL = ("rs63", "rs164", "rs128", "rs52", "raid4_61", "r6_62", "rs642", "cg63", "co42", "cg164")
ROTATED = ("rs63", "rs164", "rs128", "cg63", "cg164")
M = 65521
CANARY = 0xC5
PAD = 16  # canary bytes on each side of the magic words


def form_of(code, packet, size):
    _, k, m, _ = TM.spec(code)
    return E.predict_masked_magic_form(2 if TM.sliced(code) else 1, k, m, packet, size)


def shapes(code):
    """(packet, C).  Bytewise, from the form that runs: a half unit, one unit, one full tile, a ragged tile behind
    a full one, a ragged tile behind three -- the ragged tiles are where the position weights and the
    reduction's participation can be wrong.  Bit-sliced: test_gpu_update_masked.shapes."""
    if TM.sliced(code):
        return TM.shapes(code)
    f = form_of(code, 0, 8192)
    tile = 256 * 4 * f.VW * f.IT
    return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]


def adler(stripe):
    """zlib's adler32 over the logical stripe [k+m, C]: chunk 0, ..., chunk k-1, parity 0, ..., parity m-1"""
    return zlib.adler32(np.ascontiguousarray(stripe).tobytes()) & 0xFFFFFFFF


def adlers(stripes):
    return [adler(s) for s in stripes]


def halves(word):
    return word & 0xFFFF, word >> 16


def word_of(a, b):
    return (b << 16) | a


class Magics:
    """[PAD canary bytes (+1 when odd) | nstripes little-endian words | PAD canary bytes] in device memory"""

    def __init__(self, torch, words, odd=False):
        self.torch, self.n, self.lead = torch, len(words), PAD + (1 if odd else 0)
        body = np.array([int(w) for w in words], dtype="<u4").view(np.uint8)
        self.host = np.concatenate([np.full(self.lead, CANARY, np.uint8), body, np.full(PAD, CANARY, np.uint8)])
        raw = torch.empty(self.host.size + 256, dtype=torch.uint8, device="cuda")
        skip = -raw.data_ptr() % 256
        self.dev = raw[skip:skip + self.host.size]
        self.dev.copy_(torch.from_numpy(self.host))
        self.ptr = self.dev.data_ptr() + self.lead
        assert self.ptr % 2 == (1 if odd else 0)

    def assert_words(self, want, what):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[:self.lead], self.host[:self.lead]) and np.array_equal(got[-PAD:], self.host[-PAD:]), \
            f"{what}: the call wrote outside the magic words"
        words = [int(w) for w in got[self.lead:-PAD].view("<u4")]
        assert words == [int(w) for w in want], (what, [hex(w) for w in words], [hex(int(w)) for w in want])


class Bench(TM.Bench):
    """test_gpu_update_masked.Bench with the call replaced by the one that keeps the magics (self.magics), and the
    predicted form that of the new family.  every_column: the DISABLED column gets its fresh buffer and its real
    shard too, so that an all-ones mask changes all k chunks."""

    def __init__(self, torch, code, packet, size, layout, rotated=False, masks=None, fresh=None, every_column=False):
        super().__init__(torch, code, packet, size, layout, rotated, masks, fresh)
        self.form = form_of(code, packet, size)
        self.magics = None
        self.disabled = () if every_column else (DISABLED,)
        if every_column:
            self.farena, self.fresh_refs, _ = LY.to_device(torch, self.flay, self.fbefore)
            self.refs = list(self.real_refs)

    def sets(self):
        return TM.effective(self.k, self.words, self.disabled)

    def load_fresh(self, fresh):
        """other fresh chunks [N, k, C] into the fresh arena"""
        self.fresh = fresh
        self.fbefore = LY.images(self.flay, fresh, ())[0]
        self.farena.copy_(self.torch.from_numpy(self.fbefore))

    def call(self, store, n_shift=0, first=0, masks=None, stream=None, refs=None):
        st = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        ptr = (self.masks if masks is None else masks).ptr
        refs = self.refs if refs is None else refs
        if self.rotated:
            self.plan.update_magic_dev_masked_rotated_refs(refs, NSTRIPES, self.size, n_shift, first, ptr, self.fresh_refs,
                                                           self.magics.ptr, store, st)
        else:
            self.plan.update_magic_dev_masked_refs(refs, NSTRIPES, self.size, ptr, self.fresh_refs, self.magics.ptr, store, st)

    def check(self, store, after, n_shift=0, first=0, split=0, entry=None, want=None, odd=False):
        """one call over the armed consistent stripes self.full: the image and the rest as TM.Bench.run asserts them,
        then the magics.  entry: the words on entry (default: zlib's of the old stripes); want: the words expected
        (default: zlib's of `after` where the effective mask is not empty, the entry word where it is)."""
        entry = adlers(self.full) if entry is None else entry
        if want is None:
            want = [adler(after[s]) if cols else entry[s] for s, cols in enumerate(self.sets())]
        self.magics = Magics(self.torch, entry, odd)
        got = self.run(store, after, n_shift, first, split)
        self.magics.assert_words(want, f"{self.tag} store={store} n_shift={n_shift} first={first} split={split} odd={odd}")
        return got, want


def test_the_yardstick_is_zlib():
    """adler() is zlib's over the concatenation in logical order, and the halves are what the header says"""
    s = np.arange(3 * 8, dtype=np.uint8).reshape(3, 8)
    b = bytes(range(24))
    assert adler(s) == zlib.adler32(b)
    a_half, b_half = halves(adler(s))
    assert a_half == (1 + sum(b)) % M and b_half == (24 + sum((24 - p) * x for p, x in enumerate(b))) % M
    assert word_of(a_half, b_half) == adler(s)


# ---------------------------------------------------------------- 1. every form
@pytest.mark.parametrize("layout", ("packed", "mixed"))
@pytest.mark.parametrize("code", ALL)
def test_every_form(cuda, code, layout):
    import torch

    for packet, size in shapes(code):
        _, after = TM.after_write(code, packet, size)
        bench = Bench(torch, code, packet, size, layout)
        try:
            for store in (False, True):
                bench.check(store, after)
        finally:
            bench.close()


# ---------------------------------------------------------------- 2. over the devices of a rotated LUN
@pytest.mark.parametrize("code", ROTATED)
def test_rotated(cuda, code):
    """the same expected magics as the logical view: rotation does not enter the positions"""
    import torch

    for packet, size in shapes(code):
        _, after = TM.after_write(code, packet, size)
        bench = Bench(torch, code, packet, size, "off8", rotated=True)
        try:
            for n_shift, first in ((1, FIRST_BIG), (0, FIRST_BIG)):
                for store in (False, True):
                    bench.check(store, after, n_shift, first)
        finally:
            bench.close()


# ---------------------------------------------------------------- 3. split launches
@pytest.mark.parametrize("code", ("rs63", "rs642", "cg63", "cg164"))
def test_split_launches(cuda, code):
    """launches of 3, 3 and 1 stripes: the accumulators, the mask pointer and rot0 cross two launch boundaries, and
    the one finalize launch covers the whole call; magics and images are those of the unsplit call"""
    import torch

    for packet, size in shapes(code)[-2:]:
        _, after = TM.after_write(code, packet, size)
        for rotated in ((False, True) if code in ROTATED else (False,)):
            bench = Bench(torch, code, packet, size, "mixed", rotated=rotated)
            n_shift, first = (1, FIRST_BIG) if rotated else (0, 0)
            try:
                for store in (False, True):
                    one, want_one = bench.check(store, after, n_shift, first)
                    parts, want_parts = bench.check(store, after, n_shift, first, split=SPLIT)
                    assert np.array_equal(one, parts) and want_one == want_parts
            finally:
                bench.close()


# ---------------------------------------------------------------- 4. the extremes of the modular arithmetic
@pytest.mark.parametrize("old,new", ((0xFF, 0x00), (0x00, 0xFF)), ids=("ff_to_00", "00_to_ff"))
@pytest.mark.parametrize("code", ("rs642", "cg164"))
def test_extremes(cuda, code, old, new):
    """every data byte of every stripe goes from 0xFF to 0 (the largest negative change of both halves) or from 0 to
    0xFF (the largest positive one): all k columns enabled, the all-ones mask in every stripe"""
    import torch

    _, k, m, _ = TM.spec(code)
    packet, size = shapes(code)[-1]
    full = np.empty((NSTRIPES, k + m, size), np.uint8)
    full[:, :k] = old
    full[:, k:] = TC.ref_encode(TM.spec(code), packet, full[0, :k])
    fresh = np.full((NSTRIPES, k, size), new, np.uint8)
    words = [TM.ALL_ONES] * NSTRIPES
    after = TM.updated(code, packet, full, TM.effective(k, words, ()), fresh)
    assert np.all(after[:, :k] == new)
    for rotated in (False, True):
        bench = Bench(torch, code, packet, size, "packed", rotated=rotated, masks=words, fresh=fresh, every_column=True)
        bench.full = full
        try:
            for store in (False, True):
                bench.check(store, after, *((1, FIRST_BIG) if rotated else (0, 0)))
        finally:
            bench.close()


# ---------------------------------------------------------------- 5. an inconsistent stripe
@pytest.mark.parametrize("code", ("rs63", "rs642", "cg63", "cg164"))
def test_inconsistent_stripe(cuda, code):
    """one parity byte and one byte of a data chunk that does not change are flipped before the call, in every
    stripe that changes, and the magic on entry is zlib's of that corrupted stripe.  The codes are linear, so the
    stripe expected is the corrupted one with the chunks replaced and parity_old ^ ref_encode(old ^ fresh, zeros
    in the columns that do not change); its magic is zlib's over it"""
    import torch

    _, k, m, _ = TM.spec(code)
    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "mixed")
    sets = bench.sets()
    try:
        bad = bench.full.copy()
        for s, cols in enumerate(sets):
            if not cols:
                continue
            still = next(j for j in range(k) if j not in cols)  # (stripe 3 changes all but DISABLED: that one)
            bad[s, k + s % m, size - 1] ^= TC.FLIP
            bad[s, still, size // 2] ^= TC.FLIP
        want = bad.copy()
        for s, cols in enumerate(sets):
            if not cols:
                continue
            delta = np.zeros((k, size), np.uint8)
            for j in cols:
                delta[j] = bad[s, j] ^ bench.fresh[s, j]
                want[s, j] = bench.fresh[s, j]
            want[s, k:] = bad[s, k:] ^ TC.ref_encode(TM.spec(code), packet, delta)
        assert any(TC.expected_mask(TM.spec(code), packet, want[s]) for s in range(NSTRIPES))  # still inconsistent
        entry = adlers(bad)
        for store in (False, True):
            bench.magics = Magics(torch, entry)
            bench.arm(bench.image(bad))
            bench.call(store)
            forms = E.launch_record()
            stored = want.copy()
            if not store:
                stored[:, :k] = bad[:, :k]
            LY.assert_arena(bench.lay, bench.got(), bench.image(stored), f"{bench.tag} inconsistent store={store}")
            assert forms == [bench.form]
            bench.magics.assert_words([adler(want[s]) if cols else entry[s] for s, cols in enumerate(sets)],
                                      f"{bench.tag} inconsistent store={store}")
    finally:
        bench.close()


# ---------------------------------------------------------------- 6. / 7. wrong stays wrong, invalid stays invalid
@pytest.mark.parametrize("code", ("rs63", "cg164"))
def test_wrong_stays_wrong(cuda, code):
    """entry halves off by d from the true ones come out off by d from the true new ones"""
    import torch

    packet, size = shapes(code)[-1]
    _, after = TM.after_write(code, packet, size)
    bench = Bench(torch, code, packet, size, "packed")
    try:
        true_in, true_out = adlers(bench.full), adlers(after)
        for d in (1, 65520):
            off = lambda w: word_of(*((h + d) % M for h in halves(w)))  # noqa: E731
            entry = [off(w) for w in true_in]
            want = [off(true_out[s]) if cols else entry[s] for s, cols in enumerate(bench.sets())]
            assert all(w != t for w, t in zip(want, true_out))
            bench.check(True, after, entry=entry, want=want)
    finally:
        bench.close()


@pytest.mark.parametrize("code", ("rs63", "cg164"))
def test_poison(cuda, code):
    """a half of 65521 or more is no adler32 half: it comes out as 0xFFFF, and the other half follows its rule"""
    import torch

    packet, size = shapes(code)[-1]
    _, after = TM.after_write(code, packet, size)
    bench = Bench(torch, code, packet, size, "packed")
    try:
        true_in, true_out = adlers(bench.full), adlers(after)
        entry, want = [], []
        for s, cols in enumerate(bench.sets()):
            (a_in, b_in), (a_out, b_out) = halves(true_in[s]), halves(true_out[s])
            bad = (0xFFF1, 0xFFFF)[s // 2 % 2]
            if s % 2:
                entry.append(word_of(bad, b_in))
                want.append(word_of(0xFFFF, b_out) if cols else entry[-1])
            else:
                entry.append(word_of(a_in, bad))
                want.append(word_of(a_out, 0xFFFF) if cols else entry[-1])
        bench.check(True, after, entry=entry, want=want)
        # both halves
        entry = [0xFFF1FFFF] * NSTRIPES
        bench.check(False, after, entry=entry, want=[0xFFFFFFFF if cols else entry[s] for s, cols in enumerate(bench.sets())])
    finally:
        bench.close()


# ---------------------------------------------------------------- 8. untouched words
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_untouched_words(cuda, code):
    """the stripe whose mask is 0 and the stripe whose only set bit is the disabled column's: their words -- one
    0xFFFFFFFF, one random -- come out byte-identical, split or not"""
    import torch

    _, k, _, _ = TM.spec(code)
    packet, size = shapes(code)[-2]
    words = TM.masks_of(k)
    words[4] = 1 << DISABLED
    assert TM.effective(k, words)[2] == [] and TM.effective(k, words)[4] == []
    fresh, _ = TM.after_write(code, packet, size)
    full = TC.stripes(TM.spec(code), packet, size, NSTRIPES)
    after = TM.updated(code, packet, full, TM.effective(k, words), fresh)
    for rotated in (False, True):
        bench = Bench(torch, code, packet, size, "packed", rotated=rotated, masks=words)
        try:
            for a, b in ((0xFFFFFFFF, 0x9E3779B9), (0x12345678, 0xFFFFFFFF)):
                entry = adlers(full)
                entry[2], entry[4] = a, b
                for split in (0, SPLIT):
                    _, want = bench.check(True, after, *((1, FIRST_BIG) if rotated else (0, 0)), split=split, entry=entry)
                    assert want[2] == a and want[4] == b
        finally:
            bench.close()


# ---------------------------------------------------------------- 9. a misaligned magic buffer
@pytest.mark.parametrize("code", ("rs63", "rs128", "cg63"))
def test_misaligned_magic(cuda, code):
    import torch

    packet, size = shapes(code)[-1]
    _, after = TM.after_write(code, packet, size)
    for rotated in (False, True):
        bench = Bench(torch, code, packet, size, "mixed", rotated=rotated)
        try:
            bench.check(True, after, *((1, FIRST_BIG) if rotated else (0, 0)), odd=True)
            bench.check(False, after, *((1, FIRST_BIG) if rotated else (0, 0)), split=SPLIT, odd=True)
        finally:
            bench.close()


# ---------------------------------------------------------------- 10. composition
@pytest.mark.parametrize("code", ("rs63", "rs642", "cg164"))
def test_two_calls_compose(cuda, code):
    """two calls in a row with different masks and different fresh data, both storing: the second takes the magics
    the first left, and the result is zlib's over the final stripes"""
    import torch

    _, k, _, _ = TM.spec(code)
    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "packed")
    first_words = bench.words
    second_words = [w >> 1 | (w & 1) << (k - 1) for w in TM.masks_of(k)[::-1]]  # other sets, in other stripes
    fresh2 = np.random.default_rng([k, size, 78]).integers(0, 256, (NSTRIPES, k, size), dtype=np.uint8)
    second = TM.Masks(torch, second_words)
    try:
        mid = TM.updated(code, packet, bench.full, TM.effective(k, first_words), bench.fresh)
        end = TM.updated(code, packet, mid, TM.effective(k, second_words), fresh2)
        touched = [bool(a or b) for a, b in zip(TM.effective(k, first_words), TM.effective(k, second_words))]
        assert sum(touched) >= 6 and not np.array_equal(mid, end)
        entry = adlers(bench.full)
        bench.magics = Magics(torch, entry)
        bench.arm(bench.image(bench.full))
        bench.call(True)
        bench.got()
        bench.load_fresh(fresh2)
        bench.call(True, masks=second)
        LY.assert_arena(bench.lay, bench.got((second,)), bench.image(end), f"two calls {bench.tag}")
        bench.magics.assert_words([adler(end[s]) if touched[s] else entry[s] for s in range(NSTRIPES)], f"two calls {bench.tag}")
    finally:
        bench.close()


# ---------------------------------------------------------------- 11. engine against engine
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63", "cg164"))
def test_agrees_with_stripe_magic_dev(cuda, code):
    """ENGINE AGAINST ENGINE (the tests above are against zlib): lsec_stripe_magic_dev over the full stripes after a
    storing call gives the words the call left, for the stripes it touched"""
    import torch

    packet, size = shapes(code)[-1]
    _, after = TM.after_write(code, packet, size)
    bench = Bench(torch, code, packet, size, "packed")
    try:
        _, want = bench.check(True, after)
        again = Magics(torch, [0] * NSTRIPES)
        bench.plan.stripe_magic_dev_refs(bench.real_refs, NSTRIPES, size, again.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        again.assert_words(adlers(after), f"{bench.tag} lsec_stripe_magic_dev")
        assert [w for w, cols in zip(want, bench.sets()) if cols] == [w for w, cols in zip(adlers(after), bench.sets()) if cols]
    finally:
        bench.close()
