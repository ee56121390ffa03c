"""GPU: lsec_decode_magic_dev_patterns / lsec_decode_magic_dev_rotated, the patterned decode that also leaves
each stripe's 4-byte adler32 magic (and, with `expect`, compares it with the quorum magic).

Bar: bit-exact.  The yardstick is never the engine: the expected chunks are the reference's decode of the
stripe as it lies in memory before the call (oracle/_ref when it is built, else the oracle restatement, as
tests/test_gpu_patterns.py takes them), over stripes the reference encoded; the expected magic is zlib.adler32
over that expected LOGICAL stripe.  For the rotated call the stripes are put on the devices as
test_gpu_patterns.rotated_images puts them; the expected magics are those of the logical view, whatever the
rotation.  Only the last test compares engine with engine, and says so.

Seven stripes per case, in the arenas of tests/layouts.py (strided, offset, guard-banded), the magic words and
the bad bytes in byte buffers with canaries on both sides.  One call carries an empty pattern, one data chunk,
one parity chunk, two mixed, m erasures, for raid4 the parity alone, and a stripe whose id is past the table:
that stripe's chunks hold garbage that would change its magic if read, and its word must come out untouched.
After every call
  * the whole arena equals the image the plain call is specified to leave,
  * the magic words, and the canaries around them, equal the expected bytes,
  * the launch record names the predicted form of the new family once per launch.
"""
import zlib

import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_update_magic as TUM
import test_gpu_update_masked as TM

pytestmark = pytest.mark.gpu

CODES = {c: TUM.CODES[c] for c in ("rs63", "rs164", "raid4_61", "r6_62", "cg63", "co42")}
ROTATED = ("rs63", "rs164", "cg63")
NSTRIPES, SPLIT = 7, 3
SENTINEL, SKIPPED = 200, 4  # the id past every table, and the stripe that carries it
ENTRY = [0xDEAD0000 + 0x1111 * s for s in range(NSTRIPES)]  # the magic words on entry: the call only writes them
CANARY, BAD_FILL = 0xC5, 0x7B
FIRST_HUGE = (1 << 40) + 3

_ref_plans = {}


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES, or the tuple itself (tests/scrub_forms.py's plans)"""
    return CODES[code] if isinstance(code, str) else tuple(code)


def sliced(code):
    return spec(code)[3] != 0


def patterns_of(code):
    """empty, one data chunk, one parity chunk (raid4: the parity alone, which writes nothing), two mixed, m erasures"""
    _, k, m, _ = spec(code)
    pats = [[], [1], [k + m - 1]]
    if m >= 2:
        pats.append([2, k])
    if m >= 3:
        pats.append([0, 3] + list(range(k + 2, k + m)))
    assert max(len(p) for p in pats) == m
    return pats


def ids_of(npat):
    """every pattern at least once over the seven stripes, and the sentinel"""
    ids = [SENTINEL] * NSTRIPES
    for i, s in enumerate(s for s in range(NSTRIPES) if s != SKIPPED):
        ids[s] = i % npat
    assert set(ids) == set(range(npat)) | {SENTINEL}
    return ids


def form_of(code, packet, rmax=None):
    _, k, m, _ = spec(code)
    return E.predict_pattern_magic_form(2 if sliced(code) else 1, k, m if rmax is None else rmax, packet)


def shapes(code, rmax=None):
    """(packet, C).  Bytewise, from the form that runs: a half unit, one unit, one full tile, a ragged tile behind a
    full one, a ragged tile behind three -- the ragged tiles are where the position weights and the reduction's
    participation can be wrong.  Bit-sliced: test_gpu_update_masked.shapes."""
    if sliced(code):
        return TM.shapes(code)
    f = form_of(code, 0, rmax)
    tile = 256 * 4 * f.VW * f.IT
    return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]


def make_plan(code, packet, size):
    method, k, m, _ = spec(code)
    p = L.Plan.new(method, size, k, m, 8, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


def effective(code, pat):
    method, k, _, _ = spec(code)
    return [] if (method == L.RAID4 and pat and min(pat) >= k) else sorted(set(pat))


def ref_decode(code, packet, stripe, pat):
    """the reference's decode of stripe [k+m, C] as it lies in memory (the erased rows hold whatever they hold)"""
    method, k, m, _ = spec(code)
    out = np.ascontiguousarray(stripe).copy()
    pat = effective(code, pat)
    if not pat:
        return out
    if O.ref_available():
        key = (code, packet)
        if key not in _ref_plans:
            _ref_plans[key] = O.RefPlan(method, k, m, 8, packet)
        rc = _ref_plans[key].decode(out, pat)
    else:
        rc = O.decode(method, out, k, pat, packet, 8)
    assert rc == 0, (code, pat, rc)
    return out


adler, adlers = TUM.adler, TUM.adlers


class Bytes:
    """[16 canary bytes (+1 when odd) | body | 16 canary bytes] in device memory"""

    def __init__(self, torch, body, odd=False):
        self.lead = 16 + (1 if odd else 0)
        body = np.asarray(body, np.uint8)
        self.host = np.concatenate([np.full(self.lead, CANARY, np.uint8), body, np.full(16, CANARY, np.uint8)])
        raw = torch.empty(self.host.size + 256, dtype=torch.uint8, device="cuda")
        skip = -raw.data_ptr() % 256
        self.dev = raw[skip:skip + self.host.size]
        self.dev.copy_(torch.from_numpy(self.host))
        self.ptr = self.dev.data_ptr() + self.lead

    def body(self, what):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[:self.lead], self.host[:self.lead]) and np.array_equal(got[-16:], self.host[-16:]), \
            f"{what}: the call wrote outside its buffer"
        return got[self.lead:-16]


class Case:
    """One call over `before` [N, n, C] (each shard as the call finds it; for the rotated call the PHYSICAL devices),
    in an arena of the named layout."""

    def __init__(self, torch, code, packet, size, layout, before, outputs):
        self.torch, self.code, self.packet, self.size = torch, code, packet, size
        _, self.k, self.m, _ = spec(code)
        self.lay = LY.plan_layout(layout, self.k, self.m, NSTRIPES, size, outputs=tuple(outputs))
        LY.check_layout(self.lay)
        self.before = LY.images(self.lay, before, ())[0]
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, self.before)
        self.tag = f"{code} packet={packet} C={size} {layout}"

    def image(self, chunks):
        return LY.images(self.lay, chunks, ())[0]

    def arm(self, chunks=None):
        self.arena.copy_(self.torch.from_numpy(self.before if chunks is None else self.image(chunks)))

    def run(self, plan, want_chunks, want_words, pats=None, ids=None, lost=None, n_shift=0, first=0, rmax=None, odd=False,
            expect=None, split=0, stream=None, what=""):
        """the call, then every assertion of the module's docstring; with expect (words) also bad and bad_count.
        Returns (arena, words)."""
        torch, what = self.torch, f"{self.tag} {what}"
        if rmax is None and pats is not None:  # the table's largest erasure count (one row when it has none)
            rmax = max(1, max(len(effective(self.code, p)) for p in pats))
        magics = TUM.Magics(torch, ENTRY, odd)
        exp = bad = count = None
        if expect is not None:
            exp = Bytes(torch, np.array([int(w) for w in expect], "<u4").view(np.uint8), odd=True)
            bad = Bytes(torch, np.full(NSTRIPES, BAD_FILL, np.uint8), odd=True)
            count = torch.full((3,), 0x5EED5EED, dtype=torch.int32, device="cuda")
        ids_dev = None if ids is None else torch.from_numpy(np.asarray(ids, np.uint8)).cuda()
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        torch.cuda.synchronize()
        E.set_pattern_split(split)
        try:
            args = (magics.ptr, exp.ptr if exp else 0, bad.ptr if bad else 0, count[1:].data_ptr() if exp else 0, st)
            if ids is None:
                plan.decode_magic_dev_rotated_refs(self.refs, NSTRIPES, self.size, lost, n_shift, first, *args)
            else:
                plan.decode_magic_dev_patterns_refs(self.refs, NSTRIPES, self.size, pats, ids_dev.data_ptr(), *args)
            forms = E.launch_record()
        finally:
            E.set_pattern_split(0)
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        LY.assert_arena(self.lay, got, self.image(want_chunks), what)
        magics.assert_words(want_words, what)
        launches = -(-NSTRIPES // split) if split else 1
        assert forms == [form_of(self.code, self.packet, rmax)] * launches, (what, forms)
        if expect is not None:
            skipped = [] if ids is None else [s for s in range(NSTRIPES) if ids[s] >= len(pats)]
            want_bad = [int(s not in skipped and int(want_words[s]) != int(expect[s])) for s in range(NSTRIPES)]
            assert bad.body(what).tolist() == want_bad, (what, bad.body(what).tolist(), want_bad)
            assert exp.body(what).tolist() == exp.host[exp.lead:-16].tolist()  # only read
            c = count.cpu().numpy().view(np.uint32).tolist()
            assert c == [0x5EED5EED, sum(want_bad), 0x5EED5EED], (what, c)
        return got, [int(w) for w in want_words]


def patterned_inputs(code, packet, size, pats, ids, full=None):
    """(before, want, words): the stripes as the call finds them -- garbage in the erased slots, and in two chunks of
    the skipped stripe -- the reference's decode of each, and zlib's magics of those (the skipped stripe: its entry
    word)"""
    _, k, m, _ = spec(code)
    full = TC.stripes(spec(code), packet, size, NSTRIPES) if full is None else full
    before = np.array(full)
    want = np.empty_like(before)
    words = []
    for s in range(NSTRIPES):
        if ids[s] >= len(pats):
            before[s, 0] = LY.GARBAGE  # would change the magic if read; must stay as it is
            before[s, k] = LY.GARBAGE
            want[s] = before[s]
            words.append(ENTRY[s])
            continue
        before[s, pats[ids[s]]] = LY.GARBAGE
        want[s] = ref_decode(code, packet, before[s], pats[ids[s]])
        words.append(adler(want[s]))
    return before, want, words


def outputs_of(pats):
    return sorted({i for p in pats for i in p})


# ---------------------------------------------------------------- 0. the yardstick
def test_the_yardstick_decodes_what_the_reference_encoded(cuda):
    """ref_decode over a consistent stripe with garbage in the erased slots gives the stripe back, for every pattern
    used here; a raid4 parity-only pattern leaves the garbage.  (No GPU work, but shapes() asks the engine library
    for the form, and the `cuda` fixture has torch bring up its HIP runtime before that library is loaded: the
    order every GPU test here has.)"""
    for code in CODES:
        _, k, m, _ = spec(code)
        packet, size = shapes(code)[1]
        full = TC.stripes(spec(code), packet, size, NSTRIPES)
        for pat in patterns_of(code):
            broken = np.array(full[0])
            broken[pat] = LY.GARBAGE
            got = ref_decode(code, packet, broken, pat)
            if effective(code, pat) == sorted(pat):
                assert np.array_equal(got, full[0]), (code, pat)
            else:
                assert np.array_equal(got, broken), (code, pat)


# ---------------------------------------------------------------- 1. every form, every pattern kind in one call
@pytest.mark.parametrize("layout", ("packed", "off8", "mixed"))
@pytest.mark.parametrize("code", tuple(CODES))
def test_every_form(cuda, code, layout):
    import torch

    pats = patterns_of(code)
    ids = ids_of(len(pats))
    rmax = max(len(effective(code, p)) for p in pats)
    for i, (packet, size) in enumerate(shapes(code, rmax)):
        before, want, words = patterned_inputs(code, packet, size, pats, ids)
        case = Case(torch, code, packet, size, layout, before, outputs_of(pats))
        with make_plan(code, packet, size) as p:
            case.run(p, want, words, pats, ids, rmax=rmax, odd=(i % 2 == 1), what="every form")
            assert words[SKIPPED] == ENTRY[SKIPPED] and np.all(want[SKIPPED, 0] == LY.GARBAGE)


@pytest.mark.parametrize("code", ("rs63", "raid4_61", "cg63"))
def test_tables_of_one_row_and_of_none(cuda, code):
    """single erasures only: the one-row kernels (for K = 6 the fixed-K form); and a table with nothing to rebuild --
    the empty pattern, for raid4 the parity alone too -- whose tiles only checksum: the paranoid read's verify"""
    import torch

    _, k, m, _ = spec(code)
    for pats in ([[0], [k - 1], [k]] if m > 1 else [[0], [k - 1]], [[], [k]] if m == 1 else [[]]):
        ids = ids_of(len(pats))
        rmax = max(1, max(len(effective(code, p)) for p in pats))
        for packet, size in shapes(code, rmax)[-2:]:
            before, want, words = patterned_inputs(code, packet, size, pats, ids)
            case = Case(torch, code, packet, size, "aligned_gap", before, outputs_of(pats))
            with make_plan(code, packet, size) as p:
                case.run(p, want, words, pats, ids, rmax=rmax, what=f"table {pats}")


# ---------------------------------------------------------------- 2. corrupt survivors
@pytest.mark.parametrize("code", ("rs63", "r6_62", "cg63"))
def test_corruption_in_an_unused_survivor(cuda, code):
    """a byte of a survivor the decode does not read is flipped, at another place in every stripe: the rebuilt bytes
    are those of the clean stripe, and the magic is that of the corrupt stripe -- those chunks are read, at their own
    positions"""
    import torch

    _, k, m, _ = spec(code)
    pats = [[1], [0, 2]] if m > 2 else [[1]]  # the decode reads the first k survivors; the last parity chunk is unused
    ids = [s % len(pats) for s in range(NSTRIPES)]
    packet, size = shapes(code)[-1]
    full = np.array(TC.stripes(spec(code), packet, size, NSTRIPES))
    clean_before, clean_want, clean_words = patterned_inputs(code, packet, size, pats, ids)
    with make_plan(code, packet, size) as p:
        for s in range(NSTRIPES):
            _, in_sel, out_sel, unused = E.pattern_unused_entry(p, ids[s], patterns=pats)
            assert k + m - 1 in unused
            full[s, k + m - 1, (s * 977 + 5) % size] ^= TC.FLIP
        before, want, words = patterned_inputs(code, packet, size, pats, ids, full)
        for s in range(NSTRIPES):
            assert np.array_equal(want[s, pats[ids[s]]], clean_want[s, pats[ids[s]]]) and words[s] != clean_words[s]
        Case(torch, code, packet, size, "mixed", before, outputs_of(pats)).run(p, want, words, pats, ids, what="unused corrupt")


@pytest.mark.parametrize("code", ("rs63", "r6_62", "cg63"))
def test_corruption_in_a_used_survivor(cuda, code):
    """a byte of a survivor the decode reads is flipped: bytes and magic are those of the reference's decode of the
    corrupt stripe"""
    import torch

    _, k, m, _ = spec(code)
    pats = [[1], [0, k]]
    ids = [s % len(pats) for s in range(NSTRIPES)]
    packet, size = shapes(code)[-1]
    full = np.array(TC.stripes(spec(code), packet, size, NSTRIPES))
    _, clean_want, _ = patterned_inputs(code, packet, size, pats, ids)
    for s in range(NSTRIPES):
        full[s, 3, (s * 977 + 5) % size] ^= TC.FLIP
    before, want, words = patterned_inputs(code, packet, size, pats, ids, full)
    assert all(not np.array_equal(want[s, pats[ids[s]][0]], clean_want[s, pats[ids[s]][0]]) for s in range(NSTRIPES))
    with make_plan(code, packet, size) as p:
        Case(torch, code, packet, size, "off8", before, outputs_of(pats)).run(p, want, words, pats, ids, what="used corrupt")


# ---------------------------------------------------------------- 3. expect, bad, bad_count
@pytest.mark.parametrize("code", ("rs63", "raid4_61", "cg63"))
def test_expect_bad_and_bad_count(cuda, code):
    """expect holds the true magics with two words altered, and rubbish for the skipped stripe: bad flags exactly the
    two, bad_count is 2 (set, not added to), and the skipped stripe's bad byte is 0"""
    import torch

    pats = patterns_of(code)
    ids = ids_of(len(pats))
    for packet, size in shapes(code)[-2:]:
        before, want, words = patterned_inputs(code, packet, size, pats, ids)
        expect = list(words)
        expect[1] ^= 1            # the low half off by one
        expect[5] ^= 0x80000000   # the top bit of the high half
        expect[SKIPPED] = 0x0BADF00D
        case = Case(torch, code, packet, size, "packed", before, outputs_of(pats))
        with make_plan(code, packet, size) as p:
            case.run(p, want, words, pats, ids, expect=expect, what="expect")
            case.arm()
            case.run(p, want, words, pats, ids, expect=words[:SKIPPED] + [0] + words[SKIPPED + 1:], split=SPLIT, what="all good")


# ---------------------------------------------------------------- 4. split launches
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63"))
def test_split_launches(cuda, code):
    """launches of 3, 3 and 1 stripes: the accumulators, the ids and the refs cross two launch boundaries and the one
    finalize launch covers the whole call; outputs are those of the unsplit call"""
    import torch

    pats = patterns_of(code)
    ids = ids_of(len(pats))
    for packet, size in shapes(code)[-2:]:
        before, want, words = patterned_inputs(code, packet, size, pats, ids)
        case = Case(torch, code, packet, size, "mixed", before, outputs_of(pats))
        with make_plan(code, packet, size) as p:
            one, w1 = case.run(p, want, words, pats, ids, what="unsplit")
            case.arm()
            parts, w2 = case.run(p, want, words, pats, ids, split=SPLIT, odd=True, what="split")
            assert np.array_equal(one, parts) and w1 == w2


# ---------------------------------------------------------------- 5. over the devices of a rotated LUN
def rotated_inputs(code, packet, size, lost, n_shift, first):
    """(before, want, words): the PHYSICAL devices [N, n, C] -- device i holds logical chunk (i + rot_s) mod n, the lost
    devices garbage -- the devices after the reference's decode of each logical stripe, zlib's magics of the logical
    stripes"""
    _, k, m, _ = spec(code)
    n = k + m
    full = TC.stripes(spec(code), packet, size, NSTRIPES)
    before, want, words = np.empty_like(full), np.empty_like(full), []
    for s in range(NSTRIPES):
        rot = ((first + s) * n_shift) % n
        to_logical = (np.arange(n) + rot) % n  # device i holds logical chunk to_logical[i]
        phys = np.array(full[s][to_logical])
        phys[list(lost)] = LY.GARBAGE
        logical = np.empty_like(phys)
        logical[to_logical] = phys
        done = ref_decode(code, packet, logical, sorted((d + rot) % n for d in lost))
        before[s], want[s] = phys, done[to_logical]
        words.append(adler(done))
    return before, want, words


@pytest.mark.parametrize("lost", ([2], [2, 7]), ids=("one_lost", "two_lost"))
@pytest.mark.parametrize("code", ROTATED)
def test_rotated(cuda, code, lost):
    """the expected magics are those of the logical view, whatever the rotation; n_shift == 0 equals the patterned
    call with that one pattern for every stripe"""
    import torch

    rmax = len(lost)
    for packet, size in shapes(code, rmax)[-2:]:
        with make_plan(code, packet, size) as p:
            for n_shift in (0, 1, 5):
                for first in (0, 5, FIRST_HUGE):
                    before, want, words = rotated_inputs(code, packet, size, lost, n_shift, first)
                    case = Case(torch, code, packet, size, "off8", before, lost)
                    got, _ = case.run(p, want, words, lost=lost, n_shift=n_shift, first=first, rmax=rmax,
                                      odd=(first == 5), split=SPLIT if first == 5 else 0, what=f"rotated {lost} {n_shift} {first}")
                    if n_shift == 0:
                        case.arm()
                        same, _ = case.run(p, want, words, [lost], [0] * NSTRIPES, rmax=rmax, what="as one pattern")
                        assert np.array_equal(got, same)


def test_rotated_without_a_lost_device(cuda):
    """no device lost: nothing is written and every stripe is checksummed in logical order"""
    import torch

    code = "rs63"
    packet, size = shapes(code, 1)[-1]
    before, want, words = rotated_inputs(code, packet, size, [], 1, 5)
    assert np.array_equal(before, want)
    with make_plan(code, packet, size) as p:
        Case(torch, code, packet, size, "packed", before, ()).run(p, want, words, lost=[], n_shift=1, first=5, rmax=1, what="none lost")


# ---------------------------------------------------------------- 6. two streams
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_two_streams(cuda, code):
    """two calls on two streams over different data, queued back to back: each gets its own results -- the scratch is
    the call's own"""
    import torch

    pats = patterns_of(code)
    ids = ids_of(len(pats))
    packet, size = shapes(code)[-1]
    b1, w1, m1 = patterned_inputs(code, packet, size, pats, ids)
    other = np.array(TC.stripes(spec(code), packet, size, 2 * NSTRIPES)[NSTRIPES:])
    b2, w2, m2 = patterned_inputs(code, packet, size, pats, ids, other)
    assert m1 != m2
    c1 = Case(torch, code, packet, size, "packed", b1, outputs_of(pats))
    c2 = Case(torch, code, packet, size, "mixed", b2, outputs_of(pats))
    g1, g2 = TUM.Magics(torch, ENTRY), TUM.Magics(torch, ENTRY, odd=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ids_dev = torch.from_numpy(np.asarray(ids, np.uint8)).cuda()
    torch.cuda.synchronize()
    with make_plan(code, packet, size) as p:
        for _ in range(3):
            p.decode_magic_dev_patterns_refs(c1.refs, NSTRIPES, size, pats, ids_dev.data_ptr(), g1.ptr, stream=s1.cuda_stream)
            p.decode_magic_dev_patterns_refs(c2.refs, NSTRIPES, size, pats, ids_dev.data_ptr(), g2.ptr, stream=s2.cuda_stream)
        torch.cuda.synchronize()
    LY.assert_arena(c1.lay, c1.arena.cpu().numpy(), c1.image(w1), "stream 1")
    LY.assert_arena(c2.lay, c2.arena.cpu().numpy(), c2.image(w2), "stream 2")
    g1.assert_words(m1, "stream 1")
    g2.assert_words(m2, "stream 2")


# ---------------------------------------------------------------- 7. the torch form
def test_torch_form(cuda):
    import torch

    code, size = "rs63", 4096
    _, k, m, _ = spec(code)
    pats = [[0], [1, 7], []]
    ids = [s % 3 for s in range(NSTRIPES)]
    before, want, words = patterned_inputs(code, 0, size, pats, ids)
    data, par = torch.from_numpy(before[:, :k].copy()).cuda(), torch.from_numpy(before[:, k:].copy()).cuda()
    magic = torch.zeros(4 * NSTRIPES, dtype=torch.uint8, device="cuda")
    expect = torch.from_numpy(np.array(words[:-1] + [words[-1] ^ 2], "<u4").view(np.uint8).copy()).cuda()
    bad = torch.full((NSTRIPES,), 9, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    with make_plan(code, 0, size) as p:
        p.decode_magic_dev_patterns(data, par, pats, torch.from_numpy(np.asarray(ids, np.uint8)).cuda(), magic, expect, bad, count)
        torch.cuda.synchronize()
    assert np.array_equal(data.cpu().numpy(), want[:, :k]) and np.array_equal(par.cpu().numpy(), want[:, k:])
    assert magic.cpu().numpy().view("<u4").tolist() == words
    assert bad.cpu().tolist() == [0] * (NSTRIPES - 1) + [1] and count.item() == 1


# ---------------------------------------------------------------- 8. engine against engine
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63"))
def test_agrees_with_decode_then_stripe_magic_dev(cuda, code):
    """ENGINE AGAINST ENGINE (the tests above are against the reference and zlib): lsec_decode_dev_patterns and then
    lsec_stripe_magic_dev on a copy leave the bytes and, for the stripes that are not skipped, the words of the new
    call"""
    import torch

    pats = patterns_of(code)
    ids = ids_of(len(pats))
    packet, size = shapes(code)[-1]
    before, want, words = patterned_inputs(code, packet, size, pats, ids)
    case = Case(torch, code, packet, size, "packed", before, outputs_of(pats))
    copy = Case(torch, code, packet, size, "packed", before, outputs_of(pats))
    with make_plan(code, packet, size) as p:
        got, _ = case.run(p, want, words, pats, ids, what="fused")
        ids_dev = torch.from_numpy(np.asarray(ids, np.uint8)).cuda()
        again = TUM.Magics(torch, [0] * NSTRIPES)
        st = torch.cuda.current_stream().cuda_stream
        p.decode_dev_patterns_refs(copy.refs, NSTRIPES, size, pats, ids_dev.data_ptr(), st)
        p.stripe_magic_dev_refs(copy.refs, NSTRIPES, size, again.ptr, st)
        torch.cuda.synchronize()
    assert np.array_equal(copy.arena.cpu().numpy(), got)
    two_pass = [int(w) for w in again.dev.cpu().numpy()[again.lead:-TUM.PAD].view("<u4")]
    keep = [s for s in range(NSTRIPES) if s != SKIPPED]
    assert [two_pass[s] for s in keep] == [words[s] for s in keep]
