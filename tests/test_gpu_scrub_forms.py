"""GPU: every kernel form of lsec_check_dev, lsec_locate_dev, their _rotated twins and
lsec_decode_dev_patterns against the reference.

Each of these calls is a family of separately compiled kernels (tests/scrub_forms.py); the tables of codes
in test_gpu_check.py, test_gpu_locate.py, test_gpu_rotated_scrub.py and test_gpu_patterns.py run a corner of
them.  Here one representative plan per form, and the edge plans of scrub_forms.py, run through the rigs of
those files, so the bars are theirs: bit-exact, the expected values from the reference (oracle/_ref when it
is built, else the restatement) and never from the engine, canary words around the outputs, the outputs
pre-filled and set by the call itself, the whole arena compared.  After every call the launch record
(E.launch_record) equals the prediction for the plan and is the form the case was generated for: which
kernel ran is asserted, not assumed.

Sizes are the smallest at which a form can still go wrong (scrub_forms.sizes): a single half lane, which only
the ragged path sees, and one full tile of that form plus a half-lane tail; bit-sliced one super-packet, and
one tile of column space plus a packet.  Five stripes in the "off8" layout, every shard at 8 mod 16.
"""
import numpy as np
import pytest
import torch  # before the engine library, which the enumeration below loads while pytest collects:
#               the rest of the suite loads it behind torch, inside its tests

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import scrub_forms as SF
import test_gpu_check as TC
import test_gpu_locate as TL
import test_gpu_patterns as TP
import test_gpu_rotated_scrub as TR

pytestmark = pytest.mark.gpu

NSTRIPES, BAD = 5, 2
N_SHIFT, FIRST = 1, 3_000_000_007
CLEAN, MANY = E.LOCATE_CLEAN, E.LOCATE_MANY
LAYOUT = "off8"

SCRUB_CASES = [c for call in ("chk", "loc", "chkrot", "locrot") for c in SF.cases(call)]
# The reference's verdict on one corrupted stripe costs k + m decodes.  At k = 64 a locate item is therefore one
# corruption at one size, not all of a plan's, and the bit-sliced plan (whose reference decode is the slowest)
# runs at its one-super-packet size alone; the mixed arena of the repair holds three damaged stripes, not four.
# From k = 16 a locate item is one size.
HEAVY_K, PER_SIZE_K = 64, 16


def heavy(c):
    return c.k >= HEAVY_K and c.call in ("loc", "locrot")


def case_sizes(c):
    return SF.sizes(c)[:1] if heavy(c) and c.form.sliced else SF.sizes(c)


def code_of(c):
    return (c.method, c.k, c.m, c.packet)


def assert_forms(c, size, repair=False, rows=None):
    """the calling thread's last call launched the predicted kernels, and the first is the case's form"""
    rows = c.rows if rows is None else rows
    got = E.launch_record()
    want = E.predict_forms(c.call, SF.plan_kernel(c.method), c.k, rows, c.packet, size, repair)
    assert got == want, f"{SF.case_id(c)} C={size}: launched {got}, predicted {want}"
    assert got[0] == c.form, f"{SF.case_id(c)} C={size}: launched {got[0]}, the case stands for {c.form}"


def positions(c, size):
    """chunk bytes: the first, the last of the full tile, the first of the tail, the last (bit-sliced: of the
    column tile, in the last and the first bit-plane packet)"""
    tile = SF.tile_bytes(c.form)
    if not c.form.sliced:
        pos = [0, tile - 1, tile, size - 1]
    else:
        P = c.packet
        at = lambda col, x: (col // P) * 8 * P + x * P + col % P
        pos = [0, at(tile - 1, 7), at(tile, 0), size - 1]
    return sorted({b for b in pos if 0 <= b < size})


def data_chunks(k):
    """the first, the middle, the last four (the tail of the four-at-a-time input loop), and 31, 32 and 63:
    the hypothesis bits around a 32-bit shift and the last one"""
    return sorted({j for j in (0, k // 2, k - 4, k - 3, k - 2, k - 1, 31, 32, 63) if 0 <= j < k})


def corruptions(c, size):
    """(chunk, byte): every parity row and each of data_chunks once, the positions dealt round; then
    chunk 0 at whatever position is still unused"""
    pos = positions(c, size)
    chunks = [c.k + r for r in range(c.m)] + data_chunks(c.k)
    out = [(i, pos[n % len(pos)]) for n, i in enumerate(chunks)]
    out += [(0, b) for b in pos if b not in {x[1] for x in out}]
    return out


class Logical:
    """a rig of either kind under flips in LOGICAL chunks (the rotated rig flips by device); what it holds
    beside the reference bytes is noted per stripe, for the calls whose rig does not keep it"""

    def __init__(self, rig, rotated):
        self.rig, self.rotated, self.noted = rig, rotated, {}

    def __getattr__(self, name):
        return getattr(self.rig, name)

    def flip(self, s, i, b):
        self.rig.flip(s, self.rig.dev_of(s, i) if self.rotated else i, b)
        TL.Rig.note(self.noted.setdefault(s, []), (i, b))

    def flip_chunk(self, s, i):
        self.rig.flip_chunk(s, self.rig.dev_of(s, i) if self.rotated else i)

    def masks(self, c):
        """the reference's syndrome word of every stripe as stored (the check calls' expectation)"""
        want = np.zeros(NSTRIPES, np.uint32)
        for s, flips in self.noted.items():
            st = self.rig.full[s].copy()
            for i, b in flips:
                st[i, b] ^= TC.FLIP
            want[s] = TC.expected_mask(code_of(c), c.packet, st)
        return want


def make_rig(torch, c, size):
    code = code_of(c)
    if c.call == "chk":
        rig = TC.Rig(torch, code, c.packet, size, LAYOUT, NSTRIPES)
    elif c.call == "loc":
        rig = TL.Rig(torch, code, c.packet, size, LAYOUT, NSTRIPES)
    else:
        rig = TR.Rig(torch, code, c.packet, size, LAYOUT, N_SHIFT, FIRST, NSTRIPES)
    return Logical(rig, c.call in ("chkrot", "locrot"))


def run(c, rig, size, what):
    """one call of the case's kind over the arena as it is, compared with the reference in every output, the
    arena unchanged, the kernel the predicted one; returns the expected outputs by name"""
    torch = rig.torch
    if c.call == "chk":
        want = rig.masks(c)
        rig.expect({s: int(v) for s, v in enumerate(want) if v})  # (syndrome, bad_count, canaries, the arena)
        assert_forms(c, size)
        return {"syndrome": want}
    if c.call == "loc":
        syn, hyp, loc, counts = rig.expect(what)  # (every output, canaries, the arena)
        assert_forms(c, size)
        return {"syndrome": syn, "hyp": hyp, "located": loc, "counts": counts}
    before = rig.arena.clone()
    if c.call == "chkrot":
        want = {"syndrome": rig.masks(c)}
        want["bad_count"] = np.array([np.count_nonzero(want["syndrome"])], np.uint32)
        got = rig.check()
        assert_forms(c, size)
        rig.same(got, want, ("syndrome", "bad_count"), what)
        rig.untouched(got, ("hyp", "located", "located_dev", "counts", "dev_faults"))
    else:
        want = rig.want()
        got = rig.locate()
        assert_forms(c, size)
        rig.same(got, want, TR.NAMES, what)
        rig.untouched(got, ("bad_count",))
    assert torch.equal(rig.arena, before), f"{rig.tag} {what}: the call wrote into the arena"
    return want


# ---------------------------------------------------------------- check / locate, plain and rotated
def one_byte_items():
    """(case, size, which corruption): None for all of a case's"""
    out = []
    for c in SCRUB_CASES:
        if not heavy(c) and not (c.k >= PER_SIZE_K and c.call in ("loc", "locrot")):
            out.append((c, None, None))
        elif not heavy(c):
            out += [(c, size, None) for size in case_sizes(c)]
        else:
            out += [(c, size, n) for size in case_sizes(c) for n in range(len(corruptions(c, size)))]
    return out


def one_byte_id(item):
    c, size, n = item
    return SF.case_id(c) + ("" if size is None else f"-C{size}") + ("" if n is None else f"-{n}")


@pytest.mark.parametrize("item", one_byte_items(), ids=one_byte_id)
def test_consistent_then_one_byte(cuda, item):
    c, only_size, only = item
    k, m, n = c.k, c.m, c.k + c.m
    locating = c.call in ("loc", "locrot")
    for size in case_sizes(c) if only_size is None else (only_size,):
        rig = make_rig(torch, c, size)
        try:
            want = run(c, rig, size, "consistent")
            assert not want["syndrome"].any()
            if locating:
                assert (want["hyp"] == (1 << k) - 1).all() and (want["located"] == CLEAN).all()
                assert list(want["counts"]) == [0, 0]
            for i, b in corruptions(c, size) if only is None else corruptions(c, size)[only:only + 1]:
                rig.flip(BAD, i, b)
                want = run(c, rig, size, f"chunk {i} byte {b}")
                # what the reference said: that stripe alone; a parity row r shows as bit r alone
                assert [s for s in range(NSTRIPES) if want["syndrome"][s]] == [BAD], (SF.case_id(c), i, b, want)
                if i >= k:
                    assert want["syndrome"][BAD] == 1 << (i - k)
                if locating:
                    assert want["located"][BAD] == i and want["hyp"][BAD] == ((1 << i) if i < k else 0), (SF.case_id(c), i, b, want)
                if c.call == "locrot":
                    assert want["located_dev"][BAD] == (i - (FIRST + BAD) * N_SHIFT) % n
                    assert want["dev_faults"].sum() == 1 and want["dev_faults"][want["located_dev"][BAD]] == 1
                rig.flip(BAD, i, b)
            assert torch.equal(rig.arena, rig.orig)
        finally:
            rig.close()


def repair_items():
    out = []
    for c in SCRUB_CASES:
        if c.call in ("loc", "locrot"):
            out += [(c, size) for size in case_sizes(c)] if heavy(c) else [(c, None)]
    return out


@pytest.mark.parametrize("item", repair_items(), ids=lambda item: SF.case_id(item[0]) + (f"-C{item[1]}" if item[1] else ""))
def test_repair(cuda, item):
    """a data byte, a clean stripe, a whole parity chunk, a two-chunk stripe, a data chunk hit in its first and
    last byte (test_gpu_locate's corrupt_mixed; a heavy case leaves the last one clean): afterwards the arena holds
    what the reference's decode of each located chunk gives, and the LOCATE_MANY and the clean stripes byte for
    byte what they held"""
    c, only_size = item
    k, m = c.k, c.m
    code = code_of(c)
    for size in case_sizes(c) if only_size is None else (only_size,):
        rig = make_rig(torch, c, size)
        try:
            TL.corrupt_mixed(rig)
            located = [k // 2, CLEAN, k + m - 1, MANY, k - 1]
            if heavy(c):
                rig.flip(4, k - 1, 0)
                rig.flip(4, k - 1, size - 1)
                located[4] = CLEAN
            want = rig.want()
            if c.call == "loc":
                want = dict(zip(("syndrome", "hyp", "located", "counts"), want))
            nloc = sum(1 for x in located if x not in (CLEAN, MANY))
            assert want["located"].tolist() == located and list(want["counts"]) == [nloc, 1]
            # the reference's decode of each located chunk from the stripe as stored gives the encoded bytes back
            for s in (s for s in range(NSTRIPES) if located[s] not in (CLEAN, MANY)):
                st = rig.full[s].copy()
                for i, b, v in rig.flips.get(s, []):
                    st[i, b] ^= v
                for i in rig.chunks.get(s, []):
                    st[i] ^= 0xFF
                TL.ref_decode(code, c.packet, st, located[s])
                assert np.array_equal(st, rig.full[s])
            after = rig.orig.clone()
            for i, b in ((0, 0), (k, size - 1)):
                a = rig.lay.start(rig.dev_of(3, i) if c.call == "locrot" else i, 3) + b
                after[a:a + 1].bitwise_xor_(TC.FLIP)
            got = rig.locate(repair=True)
            assert_forms(c, size, repair=True)
            if c.call == "loc":
                got = dict(zip(("syndrome", "hyp", "located", "counts"), got))
            for name in want:
                if name != "bad_count":
                    assert np.array_equal(got[name], want[name]), f"{SF.case_id(c)} C={size}: {name} {got[name]} != {want[name]}"
            LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), after.cpu().numpy(), f"{SF.case_id(c)} C={size} repair")
        finally:
            rig.close()


# ---------------------------------------------------------------- patterned decode
def pat_cases():
    """(method, k, m, packet, rmax): a plan below and one from K = 16 for every table height, bit-sliced at both
    packets that hold no lane of four dwords, the limit plans, and whatever scrub_forms yields beside them"""
    out = [(L.REED_SOL_VAN, k, 8, 0, r) for k in (12, 16) for r in range(1, 9)]
    out += [(L.CAUCHY_GOOD, 6, 8, p, r) for p in (8, 24) for r in range(1, 9)]
    out += [(L.CAUCHY_GOOD, 16, 8, p, r) for p in (8, 24) for r in (1, 4, 8)]
    out += [(L.REED_SOL_VAN, 64, 8, 0, 8), (L.REED_SOL_VAN, 64, 64, 0, 8)]
    for c in SF.cases("pat"):
        if (c.method, c.k, c.m, c.packet, c.rows) not in out:
            out.append((c.method, c.k, c.m, c.packet, c.rows))
    return out


def pat_id(p):
    method, k, m, packet, rmax = p
    return f"{L.JE_METHOD_NAMES[method]}_{k}+{m}" + (f"_p{packet}" if packet else "") + f"-rmax{rmax}"


def pattern_table(k, m, rmax):
    """patterns of exactly rmax erasures (data only while k has that many, parity only, mixed with the last
    chunk id), of fewer, and the empty one"""
    n = k + m
    mixed = [x for pair in zip(range(k), range(k, n)) for x in pair]  # 0, k, 1, k + 1, ...
    pats = []
    for p in (range(min(rmax, k)), range(k, k + rmax), mixed[:rmax - 1] + [n - 1], [k // 2] if rmax > 1 else [],
              [min(1, k - 1), n - 2] if rmax > 2 else [], []):
        p = sorted(set(p))
        if p not in pats:
            pats.append(p)
    assert max(len(p) for p in pats) == rmax and [] in pats and all(len(p) <= m for p in pats)
    return pats


@pytest.mark.parametrize("plan", pat_cases(), ids=pat_id)
def test_patterned_decode(cuda, plan):
    method, k, m, packet, rmax = plan
    form = SF.predict("pat", method, k, rmax, packet)
    c = SF.Case("pat", "rep", method, k, m, packet, rmax, form, "")
    pats = pattern_table(k, m, rmax)
    # every pattern once, a stripe without one (an id past the table), and the first pattern again
    sp = np.random.default_rng(rmax).permutation(np.array(list(range(len(pats))) + [255, 0], np.uint8))
    for size in SF.sizes(c):
        full = TP.reference_stripes(method, k, m, size, len(sp), packet)
        with TP.make_plan(method, k, m, size, packet) as p:
            assert p.kernel == SF.plan_kernel(method)
            # lsec_decode_dev compiles a network per pattern for these shapes (in the background): the reference alone
            networks = rmax > 4 if form.sliced else rmax * k >= 96
            TP.run_patterned(torch, p, full, pats, sp, cross_check=not networks)
            # (run_patterned's per-pattern lsec_decode_dev runs are not among the recorded calls)
            assert_forms(c, size)
