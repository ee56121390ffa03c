"""GPU: lsec_search_dev_patterns / lsec_search_dev_patterns_rotated, the search for the erasure set whose rebuilt
stripe sums to the quorum magic (LStore's jerase_brute_recovery over device-resident stripes, one pass).

Bar: bit-exact.  The yardstick is never the engine: the expected trial magic T(s, p) is zlib.adler32 over the
reference's decode of a copy of the stripe as stored, with candidate p as its erasures (oracle/_ref when it is built,
else the oracle restatement, exactly as test_gpu_decode_magic.ref_decode takes them); the expected found[s] is the
first p whose T equals expect[s].  Only the n_shift = 0 test compares engine with engine, and says so.

Seven stripes per case, all reference-encoded first, expect = the magic of the encoded stripe:
  0 untouched                                   -> found 0 (the empty pattern comes first)
  1 one data chunk, its last byte flipped       -> that single (the last byte of a ragged tile)
  2 one parity chunk corrupt                    -> that single (raid4: the parity-only candidate rebuilds nothing
                                                   and no other fits, so the yardstick says LOCATE_MANY)
  3 two chunks corrupt (m >= 2)                 -> that pair
  4 m chunks corrupt                            -> that set (rs164: outside its list of singles and pairs: MANY)
  5 m + 1 chunks corrupt                        -> LOCATE_MANY
  6 corrupt, select = 0                         -> LOCATE_CLEAN, its trial words keep their entry bytes
in the arenas of tests/layouts.py, the byte outputs in test_gpu_decode_magic's buffers with canaries on both sides.
After every call: found, counts and trial equal the expectation and the canaries are intact; without the flag the
whole arena is byte-identical to before the call, with it exactly the found stripes carry the reference's decode;
the launch record names the predicted form once per launch, and with the flag the decode's form follows it.
"""
import itertools

import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_decode_magic as TDM
import test_gpu_update_magic as TUM

pytestmark = pytest.mark.gpu

CODES = {c: TUM.CODES[c] for c in ("rs63", "cg63", "r6_62", "raid4_61", "rs164")}
LIST_SIZES = {"rs63": 130, "cg63": 130, "r6_62": 37, "raid4_61": 8, "rs164": 211}
ROTATED = ("rs63", "rs164", "cg63")
NSTRIPES, SPLIT, UNSELECTED = 7, 3, 6
FOUND_FILL, TRIAL_FILL, COUNT_CANARY = 0x7B, 0xE7, 0x5EED5EED
FIRST_HUGE = (1 << 40) + 3

spec, sliced, adler, ref_decode, effective = TDM.spec, TDM.sliced, TDM.adler, TDM.ref_decode, TDM.effective
_cases = {}


def candidates(code):
    """the reference's order: the empty pattern, then sizes ascending, each size in lexicographic order; rs164 stops
    at the pairs"""
    _, k, m, _ = spec(code)
    top = 2 if code == "rs164" else m
    pats = [[]] + [list(c) for e in range(1, top + 1) for c in itertools.combinations(range(k + m), e)]
    assert len(pats) == LIST_SIZES[code]
    return pats


def rmax_of(code, pats):
    return max(1, max(len(effective(code, p)) for p in pats))


def corrupt_sets(code):
    """the chunks corrupted in each of the seven stripes"""
    _, k, m, _ = spec(code)
    many = ([0, 3] + list(range(k + 2, k + m)))[:m] if m >= 2 else [0]
    assert len(many) == m
    return [[], [1], [k + m - 1], [2, k] if m >= 2 else [], many, sorted(set(many) | {1, 2})[:m + 1], [4]]


def shapes(code):
    """test_gpu_decode_magic.shapes: bytewise 8, 16, one tile, tile + 8, 3 tiles + 8; sliced: the masked update's.
    rs164: the two smallest and one ragged one"""
    all_ = TDM.shapes(code, rmax_of(code, candidates(code)))
    return [all_[0], all_[1], all_[3]] if code == "rs164" else all_


def expectation(code, packet, size):
    """(stored [N, n, C], expect words, T [N][npat], found [N] with every stripe selected), computed once per shape
    and never modified"""
    key = (code, packet, size)
    if key in _cases:
        return _cases[key]
    _, k, m, _ = spec(code)
    pats = candidates(code)
    full = TC.stripes(spec(code), packet, size, NSTRIPES)
    expect = [adler(full[s]) for s in range(NSTRIPES)]
    stored = np.array(full)
    sets = corrupt_sets(code)
    assert len(sets[5]) == m + 1
    for s, chunks in enumerate(sets):
        for c in chunks:
            at = size - 1 if s == 1 else (s * 977 + c * 131 + 5) % size
            stored[s, c, at] ^= TC.FLIP
    trial = [[adler(ref_decode(code, packet, stored[s], p)) for p in pats] for s in range(NSTRIPES)]
    found = [next((i for i, t in enumerate(trial[s]) if t == expect[s]), E.LOCATE_MANY) for s in range(NSTRIPES)]
    # the preconditions, on the CPU: the first fit is the true corrupt set wherever the list holds it and it can be
    # rebuilt; nothing fits the stripe with m + 1 corrupt chunks
    assert found[0] == 0
    for s in (1, 2, 3, 4, 6):
        if sets[s] in pats and effective(code, sets[s]) == sets[s]:
            assert found[s] == pats.index(sets[s]), (code, s, found[s])
        else:  # raid4's parity, rs164's four chunks
            assert found[s] == E.LOCATE_MANY, (code, s, found[s])
    assert found[5] == E.LOCATE_MANY and expect[5] not in trial[5]
    stored.setflags(write=False)
    _cases[key] = (stored, expect, trial, found)
    return _cases[key]


def repaired(code, packet, stored, pats, found):
    """the image in which exactly the found stripes carry the reference's decode"""
    want = np.array(stored)
    for s, f in enumerate(found):
        if f < len(pats):
            want[s] = ref_decode(code, packet, stored[s], pats[f])
    return want


def rotate(logical, n_shift, first):
    """the physical devices [N, n, C] of logical stripes, placed as test_gpu_patterns.rotated_images places them:
    device i holds, for stripe s, logical chunk (i + (first + s) * n_shift) mod n"""
    n = logical.shape[1]
    phys = np.empty_like(logical)
    for s in range(logical.shape[0]):
        phys[s] = logical[s][(np.arange(n) + ((first + s) * n_shift) % n) % n]
    return phys


def search(torch, case, plan, pats, expect, want_trial, want_found, select, want_arena, rotated=None, repair=False, split=0,
           odd=True, what=""):
    """one call and every check of the module's docstring; want_found: with every stripe selected (the stripes that
    `select` leaves out are expected CLEAN here).  Returns (found, trial bytes, counts, arena)."""
    code, npat = case.code, len(pats)
    what = f"{case.tag} {what} split={split} repair={repair}"
    chosen = [s for s in range(NSTRIPES) if select is None or select[s]]
    found_want = [want_found[s] if s in chosen else E.LOCATE_CLEAN for s in range(NSTRIPES)]
    exp = TDM.Bytes(torch, np.array(expect, "<u4").view(np.uint8), odd=odd)
    found = TDM.Bytes(torch, np.full(NSTRIPES, FOUND_FILL, np.uint8), odd=odd)
    trial = TDM.Bytes(torch, np.full(4 * NSTRIPES * npat, TRIAL_FILL, np.uint8), odd=odd)
    sel = None if select is None else TDM.Bytes(torch, np.asarray(select, np.uint8), odd=odd)
    counts = torch.full((4,), COUNT_CANARY, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    E.set_pattern_split(split)
    try:
        args = (pats, exp.ptr, found.ptr, 0 if sel is None else sel.ptr, trial.ptr, counts[1:].data_ptr(),
                E.SEARCH_REPAIR if repair else 0, st)
        if rotated is None:
            plan.search_dev_patterns_refs(case.refs, NSTRIPES, case.size, *args)
        else:
            plan.search_dev_patterns_rotated_refs(case.refs, NSTRIPES, case.size, rotated[0], rotated[1], *args)
        forms = E.launch_record()
    finally:
        E.set_pattern_split(0)
    torch.cuda.synchronize()
    got_found = found.body(what).tolist()
    assert got_found == found_want, (what, got_found, found_want)
    c = counts.cpu().numpy().view(np.uint32).tolist()
    n_found = sum(1 for s in chosen if found_want[s] < npat)
    assert c == [COUNT_CANARY, n_found, len(chosen) - n_found, COUNT_CANARY], (what, c)
    want_bytes = np.full((NSTRIPES, 4 * npat), TRIAL_FILL, np.uint8)
    for s in chosen:
        want_bytes[s] = np.array(want_trial[s], "<u4").view(np.uint8)
    got_trial = trial.body(what).reshape(NSTRIPES, 4 * npat)
    for s in range(NSTRIPES):
        assert np.array_equal(got_trial[s], want_bytes[s]), \
            (what, s, np.flatnonzero(got_trial[s].view("<u4") != want_bytes[s].view("<u4"))[:8].tolist())
    assert exp.body(what).tolist() == exp.host[exp.lead:-16].tolist()  # only read
    if sel is not None:
        assert sel.body(what).tolist() == list(select)
    arena = case.arena.cpu().numpy()
    LY.assert_arena(case.lay, arena, case.image(want_arena), what)
    _, k, _, _ = spec(code)
    kernel, rmax = (2 if sliced(code) else 1), rmax_of(code, pats)
    launches = -(-NSTRIPES // split) if split else 1
    want_forms = [E.predict_search_form(rotated is not None, kernel, k, rmax, case.packet)] * launches
    if repair:
        decode = E.predict_form("pat", kernel, k, rmax, case.packet, case.size)
        if rotated is not None:
            decode = decode._replace(family="patrot")
        want_forms += [decode] * launches
    assert forms == want_forms, (what, forms, want_forms)
    return got_found, got_trial, c, arena


SELECT = [1] * UNSELECTED + [0]


# ---------------------------------------------------------------- 1. every form, every stripe kind in one call
@pytest.mark.parametrize("layout", ("packed", "off8", "mixed"))
@pytest.mark.parametrize("code", tuple(CODES))
def test_search(cuda, code, layout):
    import torch

    pats = candidates(code)
    outputs = sorted({i for p in pats for i in p})
    for i, (packet, size) in enumerate(shapes(code)):
        stored, expect, trial, found = expectation(code, packet, size)
        case = TDM.Case(torch, code, packet, size, layout, stored, outputs)
        found_sel = [found[s] if SELECT[s] else E.LOCATE_CLEAN for s in range(NSTRIPES)]
        fixed = repaired(code, packet, stored, pats, found_sel)
        with TDM.make_plan(code, packet, size) as p:
            for split in (0, SPLIT):
                search(torch, case, p, pats, expect, trial, found, SELECT, stored, split=split, odd=(i % 2 == 0))
                search(torch, case, p, pats, expect, trial, found, SELECT, fixed, repair=True, split=split, odd=(i % 2 == 1))
                case.arm()
        for s in (1, 3, 4):
            if found[s] < len(pats):  # what the repair leaves is the stripe that was encoded
                assert np.array_equal(fixed[s], TC.stripes(spec(code), packet, size, NSTRIPES)[s])


def test_without_select_and_without_the_optional_outputs(cuda):
    """select NULL searches every stripe, the seventh too; trial and counts may be NULL"""
    import torch

    code = "rs63"
    pats = candidates(code)
    packet, size = shapes(code)[-1]
    stored, expect, trial, found = expectation(code, packet, size)
    assert found[UNSELECTED] == pats.index([4])
    case = TDM.Case(torch, code, packet, size, "aligned_gap", stored, range(9))
    with TDM.make_plan(code, packet, size) as p:
        search(torch, case, p, pats, expect, trial, found, None, stored, what="no select")
        exp = TDM.Bytes(torch, np.array(expect, "<u4").view(np.uint8))
        out = TDM.Bytes(torch, np.full(NSTRIPES, FOUND_FILL, np.uint8))
        p.search_dev_patterns_refs(case.refs, NSTRIPES, size, pats, exp.ptr, out.ptr)
        torch.cuda.synchronize()
        assert out.body("bare").tolist() == found
        LY.assert_arena(case.lay, case.arena.cpu().numpy(), case.image(stored), "bare")


# ---------------------------------------------------------------- 2. two corrupt chunks that imitate a third
def test_imitation_r6(cuda):
    """X consistent; chunk c replaced by random bytes and a, b rebuilt from that: the stored stripe is X with only a
    and b taken from the rebuild, one chunk (c) away from a codeword and two (a, b) away from X.  A locate names c
    and leaves a consistent stripe with the wrong bytes; only the magic tells: found is the index of [a, b], and no
    single-chunk candidate fits."""
    import torch

    code = "r6_62"
    _, k, m, _ = spec(code)
    pats = candidates(code)
    packet, size = shapes(code)[-1]
    full = TC.stripes(spec(code), packet, size, NSTRIPES)
    rng = np.random.default_rng(62)
    triples = [(1, 4, 2), (0, 6, 3), (2, 7, 5), (6, 7, 0), (3, 5, 7), (0, 1, 6), (4, 7, 1)]
    stored, expect, found = np.array(full), [adler(x) for x in full], []
    for s, (a, b, c) in enumerate(triples):
        y = np.array(full[s])
        y[c] = rng.integers(0, 256, size, dtype=np.uint8)
        d = ref_decode(code, packet, y, [a, b])
        stored[s, [a, b]] = d[[a, b]]
        found.append(pats.index([a, b]))
    trial = [[adler(ref_decode(code, packet, stored[s], p)) for p in pats] for s in range(NSTRIPES)]
    for s in range(NSTRIPES):
        fits = [i for i, t in enumerate(trial[s]) if t == expect[s]]
        assert fits and fits[0] == found[s] and all(len(pats[i]) == 2 for i in fits), (s, fits)
    case = TDM.Case(torch, code, packet, size, "mixed", stored, range(k + m))
    with TDM.make_plan(code, packet, size) as p:
        search(torch, case, p, pats, expect, trial, found, None, stored, what="imitation")
        search(torch, case, p, pats, expect, trial, found, None, np.array(full), repair=True, split=SPLIT, what="imitation")


# ---------------------------------------------------------------- 3. over the devices of a rotated LUN
@pytest.mark.parametrize("code", ROTATED)
def test_rotated(cuda, code):
    """the expectations are those of the logical view, whatever the rotation; with the flag the un-rotated arena
    equals the reference's decode"""
    import torch

    _, k, m, _ = spec(code)
    n = k + m
    pats = candidates(code)
    packet, size = shapes(code)[-1]
    stored, expect, trial, found = expectation(code, packet, size)
    found_sel = [found[s] if SELECT[s] else E.LOCATE_CLEAN for s in range(NSTRIPES)]
    fixed = repaired(code, packet, stored, pats, found_sel)
    with TDM.make_plan(code, packet, size) as p:
        for n_shift, first, split in ((1, 0, 0), (1, FIRST_HUGE, SPLIT), (n + 2, 0, SPLIT), (n + 2, FIRST_HUGE, 0)):
            rot = (n_shift, first)
            case = TDM.Case(torch, code, packet, size, "off8", rotate(stored, *rot), range(n))
            search(torch, case, p, pats, expect, trial, found, SELECT, rotate(stored, *rot), rotated=rot, split=split,
                   what=f"rotated {rot}")
            search(torch, case, p, pats, expect, trial, found, SELECT, rotate(fixed, *rot), rotated=rot, repair=True,
                   split=split, what=f"rotated {rot}")


@pytest.mark.parametrize("code", ROTATED)
def test_unrotated_devices_are_the_unrotated_call(cuda, code):
    """ENGINE AGAINST ENGINE (the one such comparison here; each side is also held to the yardstick): n_shift = 0
    gives the unrotated call's outputs byte for byte, with and without the flag"""
    import torch

    _, k, m, _ = spec(code)
    pats = candidates(code)
    packet, size = shapes(code)[-1]
    stored, expect, trial, found = expectation(code, packet, size)
    found_sel = [found[s] if SELECT[s] else E.LOCATE_CLEAN for s in range(NSTRIPES)]
    fixed = repaired(code, packet, stored, pats, found_sel)
    with TDM.make_plan(code, packet, size) as p:
        for repair, want in ((False, stored), (True, fixed)):
            a = TDM.Case(torch, code, packet, size, "packed", stored, range(k + m))
            b = TDM.Case(torch, code, packet, size, "packed", stored, range(k + m))
            plain = search(torch, a, p, pats, expect, trial, found, SELECT, want, repair=repair, what="plain")
            twin = search(torch, b, p, pats, expect, trial, found, SELECT, want, rotated=(0, FIRST_HUGE), repair=repair,
                          what="n_shift 0")
            assert plain[0] == twin[0] and np.array_equal(plain[1], twin[1]) and plain[2] == twin[2]
            assert np.array_equal(plain[3], twin[3])


# ---------------------------------------------------------------- 4. found as the stripe_pattern of a later decode
def test_found_is_a_stripe_pattern(cuda):
    """found goes straight into lsec_decode_magic_dev_patterns with the same list: the found stripes are rebuilt and
    their magics equal expect, both sentinels skip their stripes; and the decode's `bad` is a valid select"""
    import torch

    code = "rs63"
    pats = candidates(code)
    packet, size = shapes(code)[-1]
    stored, expect, trial, found = expectation(code, packet, size)
    case = TDM.Case(torch, code, packet, size, "packed", stored, range(9))
    with TDM.make_plan(code, packet, size) as p:
        st = torch.cuda.current_stream().cuda_stream
        # the read path's three steps: verify every stripe (the empty pattern), search the bad ones, repair
        exp = TDM.Bytes(torch, np.array(expect, "<u4").view(np.uint8))
        magic = TDM.Bytes(torch, np.zeros(4 * NSTRIPES, np.uint8))
        bad = TDM.Bytes(torch, np.full(NSTRIPES, FOUND_FILL, np.uint8))
        zeros = torch.zeros(NSTRIPES, dtype=torch.uint8, device="cuda")
        p.decode_magic_dev_patterns_refs(case.refs, NSTRIPES, size, pats, zeros.data_ptr(), magic.ptr, exp.ptr, bad.ptr, 0, st)
        out = TDM.Bytes(torch, np.full(NSTRIPES, FOUND_FILL, np.uint8))
        p.search_dev_patterns_refs(case.refs, NSTRIPES, size, pats, exp.ptr, out.ptr, bad.ptr, 0, 0, 0, st)
        p.decode_magic_dev_patterns_refs(case.refs, NSTRIPES, size, pats, out.ptr, magic.ptr, exp.ptr, 0, 0, st)
        torch.cuda.synchronize()
        assert bad.body("bad").tolist() == [0] + [1] * (NSTRIPES - 1)
        want_found = [E.LOCATE_CLEAN] + found[1:]  # stripe 0 is not bad, so it is not searched
        assert out.body("found").tolist() == want_found
        LY.assert_arena(case.lay, case.arena.cpu().numpy(), case.image(repaired(code, packet, stored, pats, want_found)), "decode")
        words = magic.body("magic").view("<u4").tolist()
        assert all(words[s] == expect[s] for s in range(NSTRIPES) if want_found[s] < len(pats))


# ---------------------------------------------------------------- 5. nstripes == 0, and the torch form
def test_nstripes_zero_prepares_the_tables(cuda):
    """NULL device pointers, the table uploaded (records, cells, unused survivors); the calls that follow -- the search,
    the rotated search and a decode with the same list -- upload nothing"""
    import torch

    code = "rs63"
    pats = candidates(code)
    packet, size = shapes(code)[2]
    stored, expect, trial, found = expectation(code, packet, size)
    with TDM.make_plan(code, packet, size) as p:
        assert E.plan_images(p) == 0
        p.search_dev_patterns_refs([(0, 0)] * 9, 0, size, pats, 0, 0)
        assert E.launch_record() == [] and E.plan_images(p) == 3
        p.search_dev_patterns_rotated_refs([(0, 0)] * 9, 0, size, 1, 5, pats, 0, 0)
        assert E.plan_images(p) == 3
        case = TDM.Case(torch, code, packet, size, "packed", stored, range(9))
        search(torch, case, p, pats, expect, trial, found, SELECT, stored, what="prepared")
        assert E.plan_images(p) == 3
        ids = torch.full((NSTRIPES,), E.LOCATE_MANY, dtype=torch.uint8, device="cuda")
        p.decode_dev_patterns_refs(case.refs, NSTRIPES, size, pats, ids.data_ptr())
        torch.cuda.synchronize()
        assert E.plan_images(p) == 3


def test_torch_form(cuda):
    import torch

    code = "rs63"
    _, k, m, _ = spec(code)
    pats = candidates(code)
    packet, size = shapes(code)[2]
    stored, expect, trial, found = expectation(code, packet, size)
    data, par = torch.from_numpy(stored[:, :k].copy()).cuda(), torch.from_numpy(stored[:, k:].copy()).cuda()
    exp = torch.from_numpy(np.array(expect, "<u4").view(np.uint8).copy()).cuda()
    out = torch.full((NSTRIPES,), FOUND_FILL, dtype=torch.uint8, device="cuda")
    sel = torch.tensor(SELECT, dtype=torch.uint8, device="cuda")
    words = torch.zeros(4 * NSTRIPES * len(pats), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    found_sel = [found[s] if SELECT[s] else E.LOCATE_CLEAN for s in range(NSTRIPES)]
    with TDM.make_plan(code, packet, size) as p:
        p.search_dev_patterns(data, par, pats, exp, out, select=sel, trial=words, counts=counts, repair=True)
        torch.cuda.synchronize()
    assert out.cpu().tolist() == found_sel
    n_found = sum(1 for f in found_sel[:UNSELECTED] if f < len(pats))
    assert counts.cpu().tolist() == [n_found, UNSELECTED - n_found]
    got = words.cpu().numpy().view("<u4").reshape(NSTRIPES, len(pats))
    assert got[:UNSELECTED].tolist() == trial[:UNSELECTED] and not got[UNSELECTED].any()
    fixed = repaired(code, packet, stored, pats, found_sel)
    assert np.array_equal(data.cpu().numpy(), fixed[:, :k]) and np.array_equal(par.cpu().numpy(), fixed[:, k:])
