"""GPU: lsec_decode_dev_patterns_rotated / lsec_decode_magic_dev_patterns_rotated, the patterned decodes over the
physical devices of a rotated LUN -- a logical erasure pattern per stripe, plain and with the stripe magics.

Bar: bit-exact.  The yardstick is never the engine: the expected chunks are the reference's decode of the LOGICAL
stripe as it lies before the call (oracle/_ref when it is built, else the oracle restatement, exactly as
test_gpu_decode_magic.ref_decode takes them); the expected magics are zlib.adler32 over that expected logical stripe;
the physical images are a Python restatement of the rotation (test_gpu_search.rotate).  Two tests compare engine with
engine, and say so.

Seven stripes per case, in the arenas of tests/layouts.py (strided, offset, guard-banded), the magic words and the bad
bytes in byte buffers with canaries on both sides.  One call carries an empty pattern, one data chunk, one parity
chunk, two mixed, m erasures, for raid4 the parity alone, and a stripe whose id is past the table: that stripe's
chunks hold garbage, its magic word must come out untouched and its bad byte must be 0.  The split is set to 3
stripes in every other call, so that rot0, stripe_pattern and the accumulators advance across launches.
After every call
  * the whole arena equals the expected image,
  * the magic words, and the canaries around them, equal the expected bytes,
  * the launch record names the predicted form once per launch: family 18 ("patmagicrot") for the magic call, the
    "pat" form under the family "patrot" for the plain call.
"""
import itertools

import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_decode_magic as TDM
import test_gpu_search as TS
import test_gpu_update_magic as TUM
import test_gpu_vote as TV

pytestmark = pytest.mark.gpu

CODES = {c: TUM.CODES[c] for c in ("rs63", "rs164", "raid4_61", "r6_62", "cg63", "co42")}
NSTRIPES, SPLIT, SKIPPED, ENTRY = TDM.NSTRIPES, TDM.SPLIT, TDM.SKIPPED, TDM.ENTRY
FIRST_HUGE = (1 << 40) + 3

spec, sliced, adler, ref_decode, effective, rotate = TDM.spec, TDM.sliced, TDM.adler, TDM.ref_decode, TDM.effective, TS.rotate
_inputs = {}


def rotations(n):
    """(n_shift, first_stripe): step 1 from rotation 0, a step of -1 from stripe 5, a step taken mod n from a stripe
    past 2^40, and no rotation at all"""
    return ((1, 0), (n - 1, 5), (n + 2, FIRST_HUGE), (0, 3))


def rot_of(n, n_shift, first, s):
    return ((first + s) * n_shift) % n


def kernel_of(code):
    return 2 if sliced(code) else 1


def rmax_of(code, pats):
    return max(len(effective(code, p)) for p in pats)


def inputs(code, packet, size, pats, ids):
    """TDM.patterned_inputs, computed once per shape and never modified: the LOGICAL stripes as the call finds them, the
    reference's decode of each, zlib's magics of those"""
    key = (str(code), packet, size, str(pats), tuple(ids))
    if key not in _inputs:
        before, want, words = TDM.patterned_inputs(code, packet, size, pats, ids)
        before.setflags(write=False)
        want.setflags(write=False)
        _inputs[key] = (before, want, words)
    return _inputs[key]


def magic_form(code, packet, rmax):
    return E.predict_pattern_magic_rot_form(kernel_of(code), spec(code)[1], max(1, rmax), packet)


def plain_form(code, packet, size, rmax):
    return E.predict_form("pat", kernel_of(code), spec(code)[1], rmax, packet, size)._replace(family="patrot")


def shapes(code, rmax=None):
    """(packet, C).  Bytewise, from the form of family 18 that runs: a half unit, one unit, one full tile, a ragged tile
    behind a full one, a ragged tile behind three.  Bit-sliced: test_gpu_update_masked.shapes."""
    if sliced(code):
        return TDM.shapes(code)
    f = magic_form(code, 0, spec(code)[2] if rmax is None else rmax)
    tile = 256 * 4 * f.VW * f.IT
    return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]


def run(case, plan, rot, pats, ids, want_phys, want_words=None, expect=None, split=0, odd=False, what=""):
    """One call over case (the PHYSICAL devices) and every check of the module's docstring.  want_words None: the plain
    call; else the magic call, with expect (words) also bad and bad_count.  Returns (arena, words or None)."""
    torch, code = case.torch, case.code
    what = f"{case.tag} rot={rot} split={split} {'magic' if want_words is not None else 'plain'} {what}"
    rmax = rmax_of(code, pats)
    ids_dev = TDM.Bytes(torch, np.asarray(ids, np.uint8), odd=odd)  # stripe_pattern has no alignment rule
    magics = exp = bad = count = None
    if want_words is not None:
        magics = TUM.Magics(torch, ENTRY, odd)
    if expect is not None:
        exp = TDM.Bytes(torch, np.array([int(w) for w in expect], "<u4").view(np.uint8), odd=True)
        bad = TDM.Bytes(torch, np.full(NSTRIPES, TDM.BAD_FILL, np.uint8), odd=True)
        count = torch.full((3,), 0x5EED5EED, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    E.set_pattern_split(split)
    try:
        if want_words is None:
            plan.decode_dev_patterns_rotated_refs(case.refs, NSTRIPES, case.size, rot[0], rot[1], pats, ids_dev.ptr, st)
        else:
            plan.decode_magic_dev_patterns_rotated_refs(case.refs, NSTRIPES, case.size, rot[0], rot[1], pats, ids_dev.ptr,
                                                        magics.ptr, exp.ptr if exp else 0, bad.ptr if bad else 0,
                                                        count[1:].data_ptr() if exp else 0, st)
        forms = E.launch_record()
    finally:
        E.set_pattern_split(0)
    torch.cuda.synchronize()
    got = case.arena.cpu().numpy()
    LY.assert_arena(case.lay, got, case.image(want_phys), what)
    assert ids_dev.body(what).tolist() == list(ids)  # only read
    launches = -(-NSTRIPES // split) if split else 1
    if want_words is None:
        want_forms = [plain_form(code, case.packet, case.size, rmax)] * launches if rmax else []
    else:
        want_forms = [magic_form(code, case.packet, rmax)] * launches
        magics.assert_words(want_words, what)
    assert forms == want_forms, (what, forms, want_forms)
    if expect is not None:
        skipped = [s for s in range(NSTRIPES) if ids[s] >= len(pats)]
        want_bad = [int(s not in skipped and int(want_words[s]) != int(expect[s])) for s in range(NSTRIPES)]
        assert bad.body(what).tolist() == want_bad, (what, bad.body(what).tolist(), want_bad)
        assert exp.body(what).tolist() == exp.host[exp.lead:-16].tolist()  # only read
        c = count.cpu().numpy().view(np.uint32).tolist()
        assert c == [0x5EED5EED, sum(want_bad), 0x5EED5EED], (what, c)
    return got, None if want_words is None else [int(w) for w in want_words]


def both_calls(torch, plan, code, packet, size, layout, pats, ids, rot, split, odd, what=""):
    """the plain call, then the magic call over the same devices as they were"""
    n = spec(code)[1] + spec(code)[2]
    before, want, words = inputs(code, packet, size, pats, ids)
    case = TDM.Case(torch, code, packet, size, layout, rotate(before, *rot), range(n))
    want_phys = rotate(want, *rot)
    run(case, plan, rot, pats, ids, want_phys, split=split, odd=odd, what=what)
    case.arm()
    run(case, plan, rot, pats, ids, want_phys, words, split=split, odd=odd, what=what)


# ---------------------------------------------------------------- 0. the rotations
def test_the_rotations_are_what_they_are_meant_to_be(cuda):
    """over the four (n_shift, first_stripe) the seven stripes take at least four distinct rotations, (1, 0) starts at
    rotation 0, the step past n is taken mod n and (0, 3) never rotates; rotate() puts logical chunk c of stripe s on
    device (c - rot_s) mod n"""
    for code in CODES:
        _, k, m, _ = spec(code)
        n = k + m
        seen = [[rot_of(n, ns, first, s) for s in range(NSTRIPES)] for ns, first in rotations(n)]
        assert len(set(itertools.chain(*seen))) >= 4 and seen[0][0] == 0 and len(set(seen[0])) >= 4 and len(set(seen[1])) >= 4
        assert seen[2] == [((FIRST_HUGE + s) * 2) % n for s in range(NSTRIPES)] and set(seen[3]) == {0}
    logical = np.arange(3 * 9, dtype=np.uint8).reshape(3, 9, 1)
    phys = rotate(logical, 4, 7)
    for s in range(3):
        for c in range(9):
            assert phys[s, (c - rot_of(9, 4, 7, s)) % 9, 0] == logical[s, c, 0]


# ---------------------------------------------------------------- 1. every pattern kind, every shape, every rotation
@pytest.mark.parametrize("layout", ("packed", "off8", "mixed"))
@pytest.mark.parametrize("code", tuple(CODES))
def test_every_kind(cuda, code, layout):
    import torch

    _, k, m, _ = spec(code)
    pats = TDM.patterns_of(code)
    ids = TDM.ids_of(len(pats))
    rmax = rmax_of(code, pats)
    for i, (packet, size) in enumerate(shapes(code, rmax)):
        with TDM.make_plan(code, packet, size) as p:
            for j, rot in enumerate(rotations(k + m)):
                both_calls(torch, p, code, packet, size, layout, pats, ids, rot, SPLIT if (i + j) % 2 == 0 else 0, odd=(j % 2 == 1))
        _, want, words = inputs(code, packet, size, pats, ids)
        assert words[SKIPPED] == ENTRY[SKIPPED] and np.all(want[SKIPPED, 0] == LY.GARBAGE)


@pytest.mark.parametrize("code", ("rs63", "raid4_61", "cg63"))
def test_tables_with_nothing_to_rebuild(cuda, code):
    """the empty pattern, for raid4 the parity alone too: the plain call launches nothing and touches nothing, the magic
    call's one-row tiles only checksum, in LOGICAL order"""
    import torch

    _, k, m, _ = spec(code)
    pats = [[], [k]] if m == 1 else [[]]
    ids = TDM.ids_of(len(pats))
    packet, size = shapes(code, 1)[-1]
    with TDM.make_plan(code, packet, size) as p:
        for rot in rotations(k + m)[:2]:
            both_calls(torch, p, code, packet, size, "aligned_gap", pats, ids, rot, SPLIT, False, what="nothing to rebuild")


# ---------------------------------------------------------------- 2. one plan per form of family 18
def form_plans():
    """(plan kernel, k, m, rows, packet): a plan for every form of family 18, from the predictor -- per R the smallest K of
    each distinct form (R = 1 bytewise: K = 6, K = 10 and K at run time; R >= 2 bytewise: each IT the constant yields),
    bit-sliced R = 1..8.  tests/test_patterns_rotated_args.py asserts that the enumeration is closed."""
    out, seen = [], set()
    for kernel, packet in ((1, 0), (2, 8)):
        for rows in range(1, 9):
            for k in range(1, 65):
                f = E.predict_pattern_magic_rot_form(kernel, k, rows, packet)
                if f not in seen:
                    seen.add(f)
                    out.append((kernel, k, max(rows, 2), rows, packet))
    return out


class _FormPlans:
    """iterable at call time: the library is asked when a test runs, not when the module is collected"""

    def __iter__(self):
        return iter(form_plans())


FORM_PLANS = _FormPlans()


def test_every_form_of_family_18(cuda):
    import torch

    forms = set()
    for kernel, k, m, rows, packet in FORM_PLANS:
        code = (L.CAUCHY_GOOD if kernel == 2 else L.REED_SOL_VAN, k, m, packet)
        n = k + m
        data = list(range(min(k, rows // 2 + 1)))
        tall = sorted(data + list(range(n - (rows - len(data)), n)))  # `rows` erasures, data and parity mixed
        assert len(tall) == rows and len(set(tall)) == rows
        pats = [[], [0], tall, [n - 1]]
        ids = TDM.ids_of(len(pats))
        f = magic_form(code, packet, rows)
        forms.add(f)
        sizes = [(8, 64), (8, 64 * 161)] if kernel == 2 else [(0, 8), (0, 256 * 4 * f.VW * f.IT + 8)]
        for i, (pk, size) in enumerate(sizes):
            with TDM.make_plan(code, pk, size) as p:
                rot = rotations(n)[(i + rows) % 3]
                both_calls(torch, p, code, pk, size, "off8", pats, ids, rot, SPLIT if i else 0, odd=bool(i), what=f"form {f}")
    assert len(forms) == len(list(FORM_PLANS))
    assert {f.R for f in forms if f.sliced} == set(range(1, 9)) and {f.KC for f in forms if f.R == 1 and not f.sliced} == {0, 6, 10}


# ---------------------------------------------------------------- 3. expect, bad, bad_count
@pytest.mark.parametrize("code", ("rs63", "raid4_61", "cg63"))
def test_expect_bad_and_bad_count(cuda, code):
    """expect holds the true magics with two words altered, and rubbish for the skipped stripe: bad flags exactly the
    two, bad_count is 2 (set, not added to), and the skipped stripe's bad byte is 0"""
    import torch

    _, k, m, _ = spec(code)
    pats = TDM.patterns_of(code)
    ids = TDM.ids_of(len(pats))
    packet, size = shapes(code)[-1]
    before, want, words = inputs(code, packet, size, pats, ids)
    expect = list(words)
    expect[1] ^= 1            # the low half off by one
    expect[5] ^= 0x80000000   # the top bit of the high half
    expect[SKIPPED] = 0x0BADF00D
    rot = rotations(k + m)[1]
    case = TDM.Case(torch, code, packet, size, "packed", rotate(before, *rot), range(k + m))
    with TDM.make_plan(code, packet, size) as p:
        run(case, p, rot, pats, ids, rotate(want, *rot), words, expect=expect, what="expect")
        case.arm()
        run(case, p, rot, pats, ids, rotate(want, *rot), words, expect=words[:SKIPPED] + [0] + words[SKIPPED + 1:], split=SPLIT,
            what="all good")


def test_bad_without_expect_is_refused(cuda):
    """with real device pointers: refused by name, nothing enqueued, nothing written"""
    import torch

    code = "rs63"
    pats = TDM.patterns_of(code)
    ids = TDM.ids_of(len(pats))
    packet, size = shapes(code)[1]
    before, _, _ = inputs(code, packet, size, pats, ids)
    case = TDM.Case(torch, code, packet, size, "packed", rotate(before, 1, 0), range(9))
    ids_dev = torch.from_numpy(np.asarray(ids, np.uint8)).cuda()
    magics = TUM.Magics(torch, ENTRY)
    bad = TDM.Bytes(torch, np.full(NSTRIPES, TDM.BAD_FILL, np.uint8))
    with TDM.make_plan(code, packet, size) as p:
        with pytest.raises(E.ErasureError, match="lsec_decode_magic_dev_patterns_rotated: bad is given without expect"):
            p.decode_magic_dev_patterns_rotated_refs(case.refs, NSTRIPES, size, 1, 0, pats, ids_dev.data_ptr(), magics.ptr,
                                                     0, bad.ptr)
        assert E.launch_record() == []
    torch.cuda.synchronize()
    LY.assert_arena(case.lay, case.arena.cpu().numpy(), case.before, "refused")
    magics.assert_words(ENTRY, "refused")
    assert bad.body("refused").tolist() == [TDM.BAD_FILL] * NSTRIPES


# ---------------------------------------------------------------- 4. engine against engine
@pytest.mark.parametrize("code", ("rs63", "rs164", "cg63"))
def test_one_lost_device_is_the_lost_call(cuda, code):
    """ENGINE AGAINST ENGINE (each side is also held to the yardstick elsewhere): with stripe_pattern[s] the single
    erasure that lost device d gives stripe s, both new calls leave what lsec_decode_dev_rotated and
    lsec_decode_magic_dev_rotated leave with lost = {d}, bytes and magic words"""
    import torch

    _, k, m, _ = spec(code)
    n, d = k + m, 2
    pats = [[c] for c in range(n)]
    packet, size = shapes(code, 1)[-1]
    full = np.array(TC.stripes(spec(code), packet, size, NSTRIPES))
    st = torch.cuda.current_stream().cuda_stream
    with TDM.make_plan(code, packet, size) as p:
        for rot in rotations(n):
            ids = [(d + rot_of(n, rot[0], rot[1], s)) % n for s in range(NSTRIPES)]
            phys = rotate(full, *rot)
            phys[:, d] = LY.GARBAGE
            outs = []
            for magic in (False, True):
                a = TDM.Case(torch, code, packet, size, "packed", phys, [d])
                b = TDM.Case(torch, code, packet, size, "packed", phys, [d])
                ids_dev = torch.from_numpy(np.asarray(ids, np.uint8)).cuda()
                ma, mb = TUM.Magics(torch, ENTRY), TUM.Magics(torch, ENTRY)
                if magic:
                    p.decode_magic_dev_patterns_rotated_refs(a.refs, NSTRIPES, size, rot[0], rot[1], pats, ids_dev.data_ptr(),
                                                             ma.ptr, stream=st)
                    p.decode_magic_dev_rotated_refs(b.refs, NSTRIPES, size, [d], rot[0], rot[1], mb.ptr, stream=st)
                else:
                    p.decode_dev_patterns_rotated_refs(a.refs, NSTRIPES, size, rot[0], rot[1], pats, ids_dev.data_ptr(), st)
                    p.decode_dev_rotated_refs(b.refs, NSTRIPES, size, [d], rot[0], rot[1], st)
                torch.cuda.synchronize()
                got = a.arena.cpu().numpy()
                assert np.array_equal(got, b.arena.cpu().numpy()), (code, rot, magic)
                assert np.array_equal(ma.dev.cpu().numpy(), mb.dev.cpu().numpy()), (code, rot, magic)
                outs.append(got)
            assert np.array_equal(outs[0], outs[1])
            LY.assert_arena(a.lay, outs[0], a.image(rotate(full, *rot)), f"{code} {rot}")  # and both rebuilt the device


@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_found_of_a_search_is_a_stripe_pattern(cuda, code):
    """ENGINE AGAINST ENGINE for the arena, the yardstick for the image: after lsec_search_dev_patterns_rotated without
    the repair flag, lsec_decode_dev_patterns_rotated with `found` leaves what the flag leaves"""
    import torch

    _, k, m, _ = spec(code)
    n = k + m
    pats = TS.candidates(code)
    packet, size = TS.shapes(code)[-1]
    stored, expect, trial, found = TS.expectation(code, packet, size)
    fixed = TS.repaired(code, packet, stored, pats, found)
    rot = rotations(n)[2]
    st = torch.cuda.current_stream().cuda_stream
    with TDM.make_plan(code, packet, size) as p:
        a = TDM.Case(torch, code, packet, size, "off8", rotate(stored, *rot), range(n))
        b = TDM.Case(torch, code, packet, size, "off8", rotate(stored, *rot), range(n))
        exp = TDM.Bytes(torch, np.array(expect, "<u4").view(np.uint8))
        fa, fb = (TDM.Bytes(torch, np.full(NSTRIPES, 0x7B, np.uint8)) for _ in range(2))
        p.search_dev_patterns_rotated_refs(a.refs, NSTRIPES, size, rot[0], rot[1], pats, exp.ptr, fa.ptr, stream=st)
        E.set_pattern_split(SPLIT)
        try:
            p.decode_dev_patterns_rotated_refs(a.refs, NSTRIPES, size, rot[0], rot[1], pats, fa.ptr, st)
            forms = E.launch_record()
        finally:
            E.set_pattern_split(0)
        p.search_dev_patterns_rotated_refs(b.refs, NSTRIPES, size, rot[0], rot[1], pats, exp.ptr, fb.ptr, flags=E.SEARCH_REPAIR,
                                           stream=st)
        torch.cuda.synchronize()
        assert fa.body("found").tolist() == found == fb.body("found").tolist()
        assert forms == [plain_form(code, packet, size, rmax_of(code, pats))] * 3
        got = a.arena.cpu().numpy()
        assert np.array_equal(got, b.arena.cpu().numpy())
        LY.assert_arena(a.lay, got, a.image(rotate(fixed, *rot)), "found as stripe_pattern")


# ---------------------------------------------------------------- 5. nstripes == 0
def test_nstripes_zero_prepares_the_tables(cuda):
    """NULL device pointers; the table is the one of lsec_decode_dev_patterns for the same list, so the calls that
    follow -- the vote, the search, the decodes, rotated or not -- upload nothing"""
    import torch

    code = "rs63"
    pats = TS.candidates(code)
    packet, size = TS.shapes(code)[2]
    stored, expect, trial, found = TS.expectation(code, packet, size)
    with TDM.make_plan(code, packet, size) as p:
        assert E.plan_images(p) == 0
        p.decode_dev_patterns_rotated_refs([(0, 0)] * 9, 0, size, 1, 5, pats, 0)
        assert E.launch_record() == [] and E.plan_images(p) == 2  # records, cells
        p.decode_magic_dev_patterns_rotated_refs([(0, 0)] * 9, 0, size, 1, 5, pats, 0, 0)
        assert E.launch_record() == [] and E.plan_images(p) == 3  # and the unused survivors
        p.vote_dev_rotated_refs([(0, 0)] * 9, None, 0, 0, 1, 5, pats, 0, 0)
        assert E.plan_images(p) == 4                              # and the vote's masks
        p.search_dev_patterns_rotated_refs([(0, 0)] * 9, 0, size, 1, 5, pats, 0, 0)
        p.decode_dev_patterns_refs([(0, 0)] * 9, 0, size, pats, 0)
        assert E.plan_images(p) == 4
        rot = (1, 5)
        case = TDM.Case(torch, code, packet, size, "packed", rotate(stored, *rot), range(9))
        ids = torch.from_numpy(np.asarray(found, np.uint8)).cuda()
        magics = TUM.Magics(torch, ENTRY)
        p.decode_magic_dev_patterns_rotated_refs(case.refs, NSTRIPES, size, rot[0], rot[1], pats, ids.data_ptr(), magics.ptr)
        p.decode_dev_patterns_rotated_refs(case.refs, NSTRIPES, size, rot[0], rot[1], pats, ids.data_ptr())
        torch.cuda.synchronize()
        assert E.plan_images(p) == 4
        fixed = TS.repaired(code, packet, stored, pats, found)
        LY.assert_arena(case.lay, case.arena.cpu().numpy(), case.image(rotate(fixed, *rot)), "prepared")
        magics.assert_words([adler(fixed[s]) if found[s] < len(pats) else ENTRY[s] for s in range(NSTRIPES)], "prepared")


# ---------------------------------------------------------------- 6. the read, end to end
@pytest.mark.parametrize("missing", ((), (6,)))
@pytest.mark.parametrize("code", ("rs43", "cg43"))
def test_read_end_to_end(cuda, code, missing):
    """test_gpu_vote.test_read_end_to_end with the vote's ids used: vote (paranoid) -> the directed decode with the
    magics -> search and repair of what is still bad, on one stream with no host step.  Two damages are added, a stale
    data chunk and a stale parity chunk, each with other bytes and another magic on its one device: the vote names the
    chunk, the directed decode rebuilds it, and neither stripe reaches the search; the silently flipped byte does."""
    import torch

    method = L.REED_SOL_VAN if code == "rs43" else L.CAUCHY_GOOD
    k, m = 4, 3
    n, rec, READ_N, READ_C, N_SHIFT = k + m, TV.READ_C + 4, TV.READ_N, TV.READ_C, TV.N_SHIFT
    pats = [[]] + [list(c) for e in range(1, m + 1) for c in itertools.combinations(range(n), e)]
    with L.Plan.for_chunk(method, k, m, READ_C) as p:
        data, images, stripes = TV.damaged_images(p, k, m, missing)
        stale = {3: 1, 21: k + 1}  # stripe -> the logical chunk that is stale there (a data chunk, a parity chunk)
        assert not set(stale) & {2, 5, 8, 11, 12, 15, 19}
        rng = np.random.default_rng(77)
        for s, c in stale.items():
            d = (c - s * N_SHIFT) % n
            assert d not in missing
            images[d][s * rec:s * rec + 4] ^= 0xC3
            images[d][s * rec + 4:(s + 1) * rec] = rng.integers(0, 256, READ_C, dtype=np.uint8)
        want_data, status, lost = p.segment_read(images, READ_N, READ_C, n_shift=N_SHIFT, first_stripe=0, paranoid=True,
                                                 missing=missing)
        status = status.tolist()
        assert status[stripes["lost"]] == -1 and status[stripes["flip"]] == 1
        for s in stale:
            assert status[s] in (0, 1)
        for s in range(READ_N):
            if status[s] in (0, 1) and s not in stripes["blank"]:
                assert np.array_equal(want_data[s], data[s]), s
        mags = np.stack([images[d].reshape(READ_N, rec)[:, :4] for d in range(n)])
        chunks = np.stack([images[d].reshape(READ_N, rec)[:, 4:] for d in range(n)])
        for d in missing:
            mags[d], chunks[d] = 0xEE, 0xA5
        dmag = torch.from_numpy(np.ascontiguousarray(mags)).cuda()
        arena = torch.from_numpy(np.ascontiguousarray(chunks)).cuda()
        assert arena.data_ptr() % 8 == 0
        stored = [(0, 0) if d in missing else (dmag.data_ptr() + d * READ_N * 4, 4) for d in range(n)]
        refs = [(arena.data_ptr() + d * READ_N * READ_C, READ_C) for d in range(n)]
        quorum = torch.full((4 * READ_N,), TV.FILL, dtype=torch.uint8, device="cuda")
        cls, ids, bad, found = (torch.full((READ_N,), TV.FILL, dtype=torch.uint8, device="cuda") for _ in range(4))
        magic = torch.full((4 * READ_N,), TV.FILL, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            st = stream.cuda_stream
            p.vote_dev_rotated_refs(stored, refs, READ_N, READ_C, N_SHIFT, 0, pats, quorum.data_ptr(), cls.data_ptr(),
                                    ids.data_ptr(), 0, 0, E.VOTE_PARANOID, st)
            p.decode_magic_dev_patterns_rotated_refs(refs, READ_N, READ_C, N_SHIFT, 0, pats, ids.data_ptr(), magic.data_ptr(),
                                                     quorum.data_ptr(), bad.data_ptr(), 0, st)
            p.search_dev_patterns_rotated_refs(refs, READ_N, READ_C, N_SHIFT, 0, pats, quorum.data_ptr(), found.data_ptr(),
                                               bad.data_ptr(), 0, 0, E.SEARCH_REPAIR, st)
        stream.synchronize()
        cls, ids, bad, found = (t.cpu().tolist() for t in (cls, ids, bad, found))
        got = arena.cpu().numpy()
        view = [[None if (c - s * N_SHIFT) % n in missing else int(mags[(c - s * N_SHIFT) % n, s].view("<u4")[0]) for c in range(n)]
                for s in range(READ_N)]
        blank = [not chunks[:, s].any() for s in range(READ_N)]
        want = TV.expected(n, k, view, pats, True, blank)
        TV.same((quorum.cpu().numpy().view("<u4").tolist(), None, cls, ids, None), want, f"{code} read {missing}")
        for s in range(READ_N):
            what = (code, missing, s, status[s], cls[s], ids[s], bad[s], found[s])
            if status[s] == 2:
                assert cls[s] == E.VOTE_BLANK, what
            elif status[s] == -1:
                assert cls[s] == E.VOTE_LOST or (bad[s] and found[s] == E.LOCATE_MANY), what
            else:
                assert cls[s] in (E.VOTE_OK, E.VOTE_DEGRADED) and not (bad[s] and found[s] == E.LOCATE_MANY), what
                for c in range(k):
                    assert np.array_equal(got[(c - s * N_SHIFT) % n, s], want_data[s, c]), what + (c,)
        for s, c in stale.items():  # named by the vote, rebuilt by the directed decode, never searched
            lost_here = sorted({c} | {(d + s * N_SHIFT) % n for d in missing})
            assert ids[s] == pats.index(lost_here) and bad[s] == 0 and found[s] == E.LOCATE_CLEAN, (s, ids[s], bad[s], found[s])
        assert cls[stripes["lost"]] == E.VOTE_LOST and bad[stripes["flip"]] == 1 and found[stripes["flip"]] < len(pats)
