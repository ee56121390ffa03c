"""GPU: lsec_check_magic_dev / lsec_check_magic_dev_rotated, the parity check that also leaves each stripe's 4-byte
adler32 magic and, with `expect`, the scrub's verdict per stripe.

Bar: bit-exact.  The yardstick is never the engine: the stripes are the reference's encode (test_gpu_check.stripes:
oracle/_ref when it is built, else the oracle restatement), the expected syndrome of a stripe is
test_gpu_check.expected_mask over the stripe as stored, and the expected magic is zlib.adler32 over the LOGICAL stripe
as stored.  For the rotated call the stripes are put on the devices as test_gpu_decode_magic.rotated_inputs puts them
(no device lost); syndromes and magics are those of the logical view, whatever the rotation.  Only the last test
compares engine with engine, and says so.

Seven stripes per case, in the arenas of tests/layouts.py, all kinds in one call:
  0  clean
  1  one byte flipped in a data chunk: all m syndrome bits, the magic of the corrupt bytes
  2  one byte flipped in a parity row r: bit r alone
  3  the last byte of the last chunk flipped: the position of weight 1
  4  a STALE stripe -- another consistent stripe's bytes, as after a lost full-stripe write: syndrome 0, and a magic that
     differs from the quorum's.  The parity check alone cannot see it: its bad byte is exactly LSEC_SCRUB_BAD_MAGIC
  5, 6  clean
`expect` holds the magics of the bytes stored, but for stripe 4 the magic of the stripe that should be there, for stripe
1 the low half off by one and for stripe 5 the top bit of the high half flipped: bad = [0, 3, 1, 1, 2, 2, 0].

Magic, expect and bad live in byte buffers with canaries on both sides, at alternating odd addresses; syndrome and counts
between canary words, pre-filled with non-zero values.  After every call
  * the whole arena is unchanged (every chunk is only read),
  * the canaries are intact,
  * the launch record names the predicted form of the new family once per launch.
"""
import functools
import zlib

import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import scrub_forms as SF
import test_gpu_check as TC
import test_gpu_decode_magic as TDM
import test_gpu_update_magic as TUM
import test_gpu_update_masked as TM

pytestmark = pytest.mark.gpu

NAMES = ("rs63", "rs164", "raid4_61", "r6_62", "rs128", "rs52", "cg63", "co42", "cg164")
CODES = {c: TC.CODES[c] for c in NAMES}
# the tests/scrub_forms.py edges: shard index 71 carries the largest position weights of the lane sums
EDGES = {"rs648": (L.REED_SOL_VAN, 64, 8, 0), "cg648": (L.CAUCHY_GOOD, 64, 8, 8)}
ROTATED = ("rs63", "rs164", "cg63")
LAYOUTS = ("packed", "off8", "mixed")
NSTRIPES, SPLIT = 7, 3
DATA_BAD, ROW_BAD, LAST_BAD, STALE, LOW_OFF, TOP_OFF = 1, 2, 3, 4, 1, 5
ENTRY = [0xDEAD0000 + 0x1111 * s for s in range(NSTRIPES)]  # the magic words on entry: the call only writes them
CANARY_WORD, SYN_FILL, COUNT_FILL, BAD_FILL = 0x5EED5EED, 0xFFFFFFFF, 0x7B7B7B7B, 0x7B
FIRST_HUGE = (1 << 40) + 3
PARITY, MAGIC = E.SCRUB_BAD_PARITY, E.SCRUB_BAD_MAGIC


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES or EDGES, or the tuple itself (tests/scrub_forms.py's plans)"""
    if not isinstance(code, str):
        return tuple(code)
    return CODES[code] if code in CODES else EDGES[code]


def sliced(code):
    return spec(code)[3] != 0


def form_of(code, packet, size, rotated=False):
    _, k, m, _ = spec(code)
    return E.predict_check_magic_form(rotated, 2 if sliced(code) else 1, k, m, packet, size)


def shapes(code):
    """(packet, C), the smallest at which the sums can go wrong.  Bytewise, from the predicted form's tile: a half unit,
    one unit, one full tile, a ragged tile behind a full one, a ragged tile behind three.  Bit-sliced:
    test_gpu_update_masked.shapes, and for K >= 16 test_gpu_check's shapes of the wide lanes."""
    if not sliced(code):
        f = form_of(code, 0, 8192)
        tile = SF.tile_bytes(f)
        return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]
    out = list(TM.shapes(code))
    if spec(code)[1] >= 16:
        out += [s for s in TC.SLICED_SIZES_K16 if s not in out]
    return out


def edge_shape(code):
    """the one size of an edge code: a full tile and a ragged one behind it (scrub_forms.sizes' second size)"""
    _, _, _, packet = spec(code)
    tile = SF.tile_bytes(form_of(code, packet, 8 * packet if packet else 8))
    if not packet:
        return 0, tile + 8
    return packet, 8 * (-(-tile // packet) * packet + packet)


@functools.lru_cache(maxsize=None)
def scenario(code, packet, size, donor=0):
    """(stored, syndromes, words, expect, bad): the seven LOGICAL stripes [N, k+m, C] as the call finds them (read-only),
    the reference's syndrome words, zlib's magics of the bytes stored, the quorum magics handed in and the bad bytes that
    follow.  donor: which other set of consistent stripes the data comes from (two streams)."""
    _, k, m, _ = spec(code)
    n = k + m
    full = TC.stripes(spec(code), packet, size, 3 * NSTRIPES)[donor * NSTRIPES:]
    stored = np.array(full[:NSTRIPES])
    stored[DATA_BAD, k // 2, (5 * size // 7) % size] ^= TC.FLIP
    row = (m - 1) // 2
    stored[ROW_BAD, k + row, 0] ^= TC.FLIP
    stored[LAST_BAD, n - 1, size - 1] ^= TC.FLIP
    stored[STALE] = full[NSTRIPES + STALE]  # consistent, and not the stripe that was written
    syn = [TC.expected_mask(spec(code), packet, stored[s]) for s in range(NSTRIPES)]
    assert syn == [0, (1 << m) - 1, 1 << row, 1 << (m - 1), 0, 0, 0], (code, packet, size, syn)
    words = [zlib.adler32(stored[s].tobytes()) & 0xFFFFFFFF for s in range(NSTRIPES)]
    expect = list(words)
    expect[STALE] = zlib.adler32(full[STALE].tobytes()) & 0xFFFFFFFF
    assert expect[STALE] != words[STALE]
    expect[LOW_OFF] ^= 1             # the low half off by one
    expect[TOP_OFF] ^= 0x80000000    # the top bit of the high half
    bad = [(PARITY if syn[s] else 0) | (MAGIC if expect[s] != words[s] else 0) for s in range(NSTRIPES)]
    assert bad == [0, PARITY | MAGIC, PARITY, PARITY, MAGIC, MAGIC, 0]
    stored.setflags(write=False)
    return stored, syn, words, expect, bad


def rotate(stored, n_shift, first):
    """the PHYSICAL devices [N, n, C]: device i of stripe s holds logical chunk (i + rot_s) mod n"""
    n = stored.shape[1]
    phys = np.empty_like(stored)
    for s in range(stored.shape[0]):
        rot = ((first + s) * n_shift) % n
        phys[s] = stored[s][(np.arange(n) + rot) % n]
    return phys


def make_plan(code, packet, size):
    method, k, m, _ = spec(code)
    p = L.Plan.new(method, size, k, m, 8, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0
    return p


class Words:
    """[4 canaries | nstripes syndrome words | 4 canaries | counts[2] | 4 canaries] in device memory, pre-filled"""

    def __init__(self, torch, n):
        self.n = n
        t = np.full(n + 14, CANARY_WORD, np.uint32)
        t[4:4 + n] = SYN_FILL
        t[8 + n:10 + n] = COUNT_FILL
        self.dev = torch.from_numpy(t.view(np.int32)).cuda()
        self.syndrome_ptr = self.dev.data_ptr() + 16
        self.counts_ptr = self.dev.data_ptr() + 4 * (8 + n)

    def read(self, what):
        """(syndrome [n], counts [2]) after the canary check; the caller has synchronised"""
        w = self.dev.cpu().numpy().view(np.uint32)
        n = self.n
        for lo, hi in ((0, 4), (4 + n, 8 + n), (10 + n, 14 + n)):
            assert (w[lo:hi] == CANARY_WORD).all(), f"{what}: canary words [{lo}, {hi}) changed: {w[lo:hi]}"
        return w[4:4 + n].tolist(), w[8 + n:10 + n].tolist()


class Case:
    """One arena holding `chunks` [N, n, C] (the logical chunks, or the devices of a rotated LUN) and the calls over it."""

    def __init__(self, torch, code, packet, size, layout, chunks, rotated=False, n_shift=0, first=0):
        self.torch, self.code, self.packet, self.size = torch, code, packet, size
        self.rotated, self.n_shift, self.first = rotated, n_shift, first
        _, self.k, self.m, _ = spec(code)
        self.lay = LY.plan_layout(layout, self.k, self.m, NSTRIPES, size, outputs=range(self.k, self.k + self.m))
        LY.check_layout(self.lay)
        self.before = LY.images(self.lay, chunks, ())[0]
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, self.before)
        self.tag = f"{code} packet={packet} C={size} {layout}" + (f" rotated {n_shift} {first}" if rotated else "")

    def call(self, plan, syndrome_ptr, magic_ptr, expect_ptr=0, bad_ptr=0, counts_ptr=0, stream=None):
        st = self.torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        if self.rotated:
            plan.check_magic_dev_rotated_refs(self.refs, NSTRIPES, self.size, self.n_shift, self.first, syndrome_ptr, magic_ptr,
                                              expect_ptr, bad_ptr, counts_ptr, st)
        else:
            plan.check_magic_dev_refs(self.refs, NSTRIPES, self.size, syndrome_ptr, magic_ptr, expect_ptr, bad_ptr, counts_ptr, st)

    def run(self, plan, syn, words, expect=None, want_bad=None, outputs=True, odd=False, split=0, what=""):
        """the call, then every assertion of the module's docstring.  expect: the quorum magics (None: NULL); outputs:
        False hands in NULL for bad and counts too.  Returns (syndrome, magic words, bad, counts)."""
        torch, what = self.torch, f"{self.tag} {what}"
        magics = TUM.Magics(torch, ENTRY, odd)
        words_dev = Words(torch, NSTRIPES)
        exp = None if expect is None else TDM.Bytes(torch, np.array([int(w) for w in expect], "<u4").view(np.uint8), odd=not odd)
        bad = TDM.Bytes(torch, np.full(NSTRIPES, BAD_FILL, np.uint8), odd=odd) if outputs else None
        torch.cuda.synchronize()
        E.set_pattern_split(split)
        try:
            self.call(plan, words_dev.syndrome_ptr, magics.ptr, exp.ptr if exp else 0, bad.ptr if bad else 0,
                      words_dev.counts_ptr if outputs else 0)
            forms = E.launch_record()
        finally:
            E.set_pattern_split(0)
        torch.cuda.synchronize()
        LY.assert_arena(self.lay, self.arena.cpu().numpy(), self.before, what)  # only read
        got_syn, got_counts = words_dev.read(what)
        print(f"{what}: syndrome {got_syn} magic {[hex(w) for w in magics.dev.cpu().numpy()[magics.lead:-TUM.PAD].view('<u4')]}"
              f" counts {got_counts}")
        assert got_syn == list(syn), (what, got_syn, syn)
        magics.assert_words(words, what)
        launches = -(-NSTRIPES // split) if split else 1
        assert forms == [form_of(self.code, self.packet, self.size, self.rotated)] * launches, (what, forms)
        got_bad = None
        if exp is not None:
            assert exp.body(what).tolist() == exp.host[exp.lead:-16].tolist()  # only read
        if outputs:
            if want_bad is None:  # without expect only the parity bit can appear
                want_bad = [PARITY if v else 0 for v in syn]
            got_bad = bad.body(what).tolist()
            assert got_bad == list(want_bad), (what, got_bad, want_bad)
            assert got_counts == [sum(1 for b in want_bad if b & PARITY), sum(1 for b in want_bad if b & MAGIC)], (what, got_counts)
        else:
            assert got_counts == [COUNT_FILL] * 2, (what, got_counts)
        return got_syn, [int(w) for w in words], got_bad, got_counts


# ---------------------------------------------------------------- 0. the yardstick
def test_the_yardstick(cuda):
    """scenario()'s own assertions over every code at one shape: the reference's syndromes are the ones the kinds are
    named for, and the stale stripe is consistent.  (No GPU work; the `cuda` fixture brings torch's HIP runtime up before
    the engine library answers for the forms, the order every GPU test here has.)"""
    for code in NAMES:
        packet, size = shapes(code)[1]
        stored, syn, words, expect, bad = scenario(code, packet, size)
        assert syn[STALE] == 0 and bad[STALE] == MAGIC and words[STALE] != expect[STALE]
        assert zlib.adler32(b"") == 1


# ---------------------------------------------------------------- 1. every form, every stripe kind in one call
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", NAMES)
def test_every_form(cuda, code, layout):
    import torch

    for i, (packet, size) in enumerate(shapes(code)):
        stored, syn, words, expect, bad = scenario(code, packet, size)
        case = Case(torch, code, packet, size, layout, stored)
        with make_plan(code, packet, size) as p:
            got = case.run(p, syn, words, expect, bad, odd=(i % 2 == 1), what="every form")
            assert got[2][STALE] == MAGIC  # the stripe the parity check alone cannot see


@pytest.mark.parametrize("code", tuple(EDGES))
def test_widest_stripes(cuda, code):
    """RS(64+8) and Cauchy-good(64+8, packet 8): 72 chunks, shard index 71"""
    import torch

    packet, size = edge_shape(code)
    stored, syn, words, expect, bad = scenario(code, packet, size)
    with make_plan(code, packet, size) as p:
        Case(torch, code, packet, size, "off8", stored).run(p, syn, words, expect, bad, odd=True, what="widest")
        phys = rotate(stored, 5, 5)
        Case(torch, code, packet, size, "packed", phys, True, 5, 5).run(p, syn, words, expect, bad, what="widest")


# ---------------------------------------------------------------- 2. expect, bad, counts
@pytest.mark.parametrize("code", ("rs63", "raid4_61", "cg63"))
def test_optional_outputs(cuda, code):
    """without expect only the parity bit appears and counts[1] is 0; with all three NULL the call still writes
    syndrome and magic; with the true magics as expect no magic bit appears.  counts is set, not added to: the same
    buffers' fill values are non-zero on every call."""
    import torch

    for packet, size in shapes(code)[-2:]:
        stored, syn, words, expect, bad = scenario(code, packet, size)
        case = Case(torch, code, packet, size, "mixed", stored)
        with make_plan(code, packet, size) as p:
            got = case.run(p, syn, words, None, None, what="no expect")
            assert got[3][1] == 0 and all(b in (0, PARITY) for b in got[2])
            case.run(p, syn, words, None, None, outputs=False, odd=True, what="all NULL")
            case.run(p, syn, words, expect, None, outputs=False, what="expect alone")
            case.run(p, syn, words, words, [PARITY if v else 0 for v in syn], what="true magics")
            got = case.run(p, syn, words, expect, bad, odd=True, what="expect")
            assert got[3] == [3, 3]


def test_empty_chunks(cuda):
    """block_size == 0: every magic word is adler32 of nothing, every syndrome 0"""
    import torch

    code = "rs63"
    stored = scenario(code, 0, 8)[0]
    case = Case(torch, code, 0, 8, "packed", stored)
    case.size = 0
    with make_plan(code, 0, 4096) as p:
        magics, words = TUM.Magics(torch, ENTRY, True), Words(torch, NSTRIPES)
        case.call(p, words.syndrome_ptr, magics.ptr, 0, 0, words.counts_ptr)
        assert E.launch_record() == []
        torch.cuda.synchronize()
        magics.assert_words([1] * NSTRIPES, "empty")
        assert words.read("empty") == ([0] * NSTRIPES, [0, 0])


# ---------------------------------------------------------------- 3. over the devices of a rotated LUN
@pytest.mark.parametrize("code", ROTATED)
def test_rotated(cuda, code):
    """magics and syndromes are those of the logical view, whatever the rotation; n_shift == 0 gives the unrotated
    call's outputs"""
    import torch

    for packet, size in shapes(code)[-2:]:
        stored, syn, words, expect, bad = scenario(code, packet, size)
        with make_plan(code, packet, size) as p:
            plain = Case(torch, code, packet, size, "off8", stored).run(p, syn, words, expect, bad, what="unrotated")
            for n_shift in (0, 1, 5):
                for first in (0, 5, FIRST_HUGE):
                    case = Case(torch, code, packet, size, "off8", rotate(stored, n_shift, first), True, n_shift, first)
                    got = case.run(p, syn, words, expect, bad, odd=(first == 5), split=SPLIT if first == 5 else 0)
                    if n_shift == 0:
                        assert got == plain


# ---------------------------------------------------------------- 4. split launches
@pytest.mark.parametrize("rotated", (False, True), ids=("plain", "rotated"))
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63"))
def test_split_launches(cuda, code, rotated):
    """launches of 3, 3 and 1 stripes: the accumulators, the syndrome words, the refs and rot0 cross two launch
    boundaries and the one finalize launch covers the whole call; outputs are those of the unsplit call"""
    import torch

    for packet, size in shapes(code)[-2:]:
        stored, syn, words, expect, bad = scenario(code, packet, size)
        chunks = rotate(stored, 4, 6) if rotated else stored
        case = Case(torch, code, packet, size, "mixed", chunks, rotated, 4, 6)
        with make_plan(code, packet, size) as p:
            one = case.run(p, syn, words, expect, bad, what="unsplit")
            parts = case.run(p, syn, words, expect, bad, split=SPLIT, odd=True, what="split")
            assert one == parts


# ---------------------------------------------------------------- 5. two streams
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_two_streams(cuda, code):
    """two calls on two streams over different data, queued back to back three times: each gets its own results -- the
    scratch is the call's own"""
    import torch

    packet, size = shapes(code)[-1]
    s1, y1, w1, e1, b1 = scenario(code, packet, size)
    s2, y2, w2, e2, b2 = scenario(code, packet, size, donor=1)
    assert w1 != w2
    c1 = Case(torch, code, packet, size, "packed", s1)
    c2 = Case(torch, code, packet, size, "mixed", rotate(s2, 1, 5), True, 1, 5)
    g1, g2 = TUM.Magics(torch, ENTRY), TUM.Magics(torch, ENTRY, odd=True)
    o1, o2 = Words(torch, NSTRIPES), Words(torch, NSTRIPES)
    x1 = TDM.Bytes(torch, np.array(e1, "<u4").view(np.uint8), odd=True)
    x2 = TDM.Bytes(torch, np.array(e2, "<u4").view(np.uint8))
    d1 = TDM.Bytes(torch, np.full(NSTRIPES, BAD_FILL, np.uint8))
    d2 = TDM.Bytes(torch, np.full(NSTRIPES, BAD_FILL, np.uint8), odd=True)
    st1, st2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with make_plan(code, packet, size) as p:
        for _ in range(3):
            c1.call(p, o1.syndrome_ptr, g1.ptr, x1.ptr, d1.ptr, o1.counts_ptr, st1)
            c2.call(p, o2.syndrome_ptr, g2.ptr, x2.ptr, d2.ptr, o2.counts_ptr, st2)
        torch.cuda.synchronize()
    g1.assert_words(w1, "stream 1")
    g2.assert_words(w2, "stream 2")
    assert o1.read("stream 1") == (y1, [3, 3]) and o2.read("stream 2") == (y2, [3, 3])
    assert d1.body("stream 1").tolist() == b1 and d2.body("stream 2").tolist() == b2


# ---------------------------------------------------------------- 6. the torch forms
def test_torch_forms(cuda):
    import torch

    code, size = "rs63", 4096
    _, k, m, _ = spec(code)
    stored, syn, words, expect, bad = scenario(code, 0, size)
    data, par = torch.from_numpy(stored[:, :k].copy()).cuda(), torch.from_numpy(stored[:, k:].copy()).cuda()
    exp = torch.from_numpy(np.array(expect, "<u4").view(np.uint8).copy()).cuda()
    with make_plan(code, 0, size) as p:
        for rotated in (False, True):
            syn_t = torch.full((NSTRIPES,), -1, dtype=torch.int32, device="cuda")
            magic = torch.zeros(4 * NSTRIPES, dtype=torch.uint8, device="cuda")
            bad_t = torch.full((NSTRIPES,), 9, dtype=torch.uint8, device="cuda")
            counts = torch.full((2,), 77, dtype=torch.int32, device="cuda")
            if rotated:
                devs = torch.from_numpy(np.ascontiguousarray(rotate(stored, 2, 3).transpose(1, 0, 2))).cuda()
                p.check_magic_dev_rotated(devs, 2, 3, syn_t, magic, exp, bad_t, counts)
            else:
                p.check_magic_dev(data, par, syn_t, magic, exp, bad_t, counts)
            torch.cuda.synchronize()
            assert syn_t.cpu().tolist() == syn and magic.cpu().numpy().view("<u4").tolist() == words
            assert bad_t.cpu().tolist() == bad and counts.cpu().tolist() == [3, 3]
        with pytest.raises(ValueError):
            p.check_magic_dev(data, par, syn_t, magic[:-1])


# ---------------------------------------------------------------- 7. engine against engine
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63"))
def test_agrees_with_check_then_stripe_magic_dev(cuda, code):
    """ENGINE AGAINST ENGINE (the tests above are against the reference and zlib): lsec_check_dev and then
    lsec_stripe_magic_dev on a copy -- for the rotated call on the un-rotated copy -- give the words of the new call"""
    import torch

    packet, size = shapes(code)[-1]
    stored, syn, words, expect, bad = scenario(code, packet, size)
    with make_plan(code, packet, size) as p:
        fused = Case(torch, code, packet, size, "packed", stored).run(p, syn, words, expect, bad, what="fused")
        turned = Case(torch, code, packet, size, "packed", rotate(stored, 1, 5), True, 1, 5).run(p, syn, words, expect, bad)
        copy = Case(torch, code, packet, size, "packed", stored)
        two_syn = torch.full((NSTRIPES + 1,), -1, dtype=torch.int32, device="cuda")
        again = TUM.Magics(torch, [0] * NSTRIPES)
        st = torch.cuda.current_stream().cuda_stream
        p.check_dev_refs(copy.refs, NSTRIPES, size, two_syn.data_ptr(), two_syn[NSTRIPES:].data_ptr(), st)
        p.stripe_magic_dev_refs(copy.refs, NSTRIPES, size, again.ptr, st)
        torch.cuda.synchronize()
    two_pass = [int(w) for w in again.dev.cpu().numpy()[again.lead:-TUM.PAD].view("<u4")]
    two = two_syn.cpu().numpy().view(np.uint32).tolist()
    assert two[:NSTRIPES] == fused[0] == turned[0] and two[NSTRIPES] == fused[3][0] == turned[3][0]
    assert two_pass == fused[1] == turned[1]
