"""GPU: every kernel form of the calls that leave the stripe magics beside a scrub, a decode or a rotated encode,
against the reference: lsec_check_magic_dev(_rotated), lsec_decode_magic_dev_patterns, lsec_decode_magic_dev_rotated
and lsec_encode_magic_dev_rotated.

Each of these calls is a family of separately compiled kernels (tests/scrub_forms.py: MAGIC_FORM_CALLS); the tables
of codes in test_gpu_check_magic.py, test_gpu_decode_magic.py and test_gpu_encode_magic_rotated.py run a corner of
them.  Here one representative plan per form, and the edge plans of scrub_forms.py (among them the two 72-chunk
plans; the decodes take m <= 8, so RS(64+64) is none of theirs), run through the rigs of those files, so the bars are
theirs: bit-exact, the stripes
and the expected syndromes from the reference's encode, the rebuilt chunks from the reference's decode (oracle/_ref
when it is built, else the restatement), the magics from zlib's adler32 over the logical stripe, nothing expected
ever taken from the engine, the whole arena compared, every output between canaries and pre-filled.  After every
call the launch record (E.launch_record) equals the prediction, once per launch -- the rigs assert that -- and the
predicted form is the form the case was generated for: which kernel ran is asserted, not assumed.

Sizes are the smallest at which a form can still go wrong (scrub_forms.sizes): a single half lane, which only the
ragged path sees, and one full tile of that form plus a half-lane tail; bit-sliced one super-packet, and one tile of
column space plus a packet.  The "off8" layout, every shard at 8 mod 16; the stripe counts are the rigs' own.
"""
import pytest
import torch  # before the engine library, which the enumeration below loads while pytest collects:
#               the rest of the suite loads it behind torch, inside its tests

from lstore_amd import erasure as E

import scrub_forms as SF
import test_gpu_check_magic as TCM
import test_gpu_decode_magic as TDM
import test_gpu_encode_magic_rotated as TEM

pytestmark = pytest.mark.gpu

N_SHIFT, FIRST = 1, 3_000_000_007
LAYOUT = "off8"
# The reference's decode of a stripe of 64 data chunks is the one large piece of host work here.  As in
# test_gpu_scrub_forms.py such a case runs at one size -- the full tile with the ragged one behind it -- never at
# fewer forms.
HEAVY_K = 64
WRONG, JUNK = 1, 0x0BADF00D  # the stripe whose quorum magic is planted wrong; the skipped stripe's quorum word


def code_of(c):
    return (c.method, c.k, c.m, c.packet)


def cases(*calls):
    return [c for call in calls for c in SF.cases(call)]


def decode_sizes(c):
    return SF.sizes(c)[1:] if c.k >= HEAVY_K else SF.sizes(c)


def is_the_case(c, size, form):
    """the form the rig predicts (and compares the launch record with) is the one the case stands for, and the
    calling thread's last call launched it"""
    assert form == c.form, f"{SF.case_id(c)} C={size}: predicted {form}, the case stands for {c.form}"
    got = E.launch_record()
    assert got and set(got) == {c.form}, f"{SF.case_id(c)} C={size}: launched {got}"


# ---------------------------------------------------------------- lsec_check_magic_dev, lsec_check_magic_dev_rotated
@pytest.mark.parametrize("c", cases("chkmagic", "chkmagicrot"), ids=SF.case_id)
def test_check_magic(cuda, c):
    """the rig's scenario -- a bad data byte, a bad parity row, a bad last byte, a stale stripe -- with `expect`"""
    code, rotated = code_of(c), c.call == "chkmagicrot"
    for i, size in enumerate(SF.sizes(c)):
        stored, syn, words, expect, bad = TCM.scenario(code, c.packet, size)
        if rotated:
            case = TCM.Case(torch, code, c.packet, size, LAYOUT, TCM.rotate(stored, N_SHIFT, FIRST), True, N_SHIFT, FIRST)
        else:
            case = TCM.Case(torch, code, c.packet, size, LAYOUT, stored)
        with TCM.make_plan(code, c.packet, size) as p:
            got = case.run(p, syn, words, expect, bad, odd=(i % 2 == 1), what=SF.case_id(c))
            is_the_case(c, size, TCM.form_of(code, c.packet, size, rotated))
            assert got[2][TCM.STALE] == TCM.MAGIC  # the stripe the parity check alone cannot see


# ---------------------------------------------------------------- lsec_decode_magic_dev_patterns
def pattern_table(k, m, rows):
    """patterns over k + m chunks: `rows` erasures, data from the front and parity from the back with the last chunk
    id among them (one row: that parity chunk alone); a parity chunk alone; one data chunk, which leaves a survivor
    unused wherever m >= 2; a data chunk beside the last parity chunk but one; and the empty one"""
    n = k + m
    data = min(k, rows // 2)
    pats = []
    for p in (list(range(data)) + [n - 1 - i for i in range(rows - data)], [k], [k // 2],
              [min(1, k - 1), n - 2] if rows > 2 else [], []):
        p = sorted(set(p))
        if p not in pats:
            pats.append(p)
    assert max(len(p) for p in pats) == rows and [] in pats and all(len(p) <= m for p in pats)
    assert any(p and min(p) >= k for p in pats) and any(0 < len(p) < m for p in pats) == (m >= 2)
    return pats


@pytest.mark.parametrize("c", cases("patmagic"), ids=SF.case_id)
def test_decode_magic_patterns(cuda, c):
    """a table with `rows` erasures in one pattern and fewer in the others, a stripe without a pattern, `expect` with
    one quorum magic planted wrong"""
    code = code_of(c)
    pats = pattern_table(c.k, c.m, c.rows)
    ids = TDM.ids_of(len(pats))
    for i, size in enumerate(decode_sizes(c)):
        before, want, words = TDM.patterned_inputs(code, c.packet, size, pats, ids)
        expect = list(words)
        expect[WRONG] ^= 1 << 16
        expect[TDM.SKIPPED] = JUNK
        case = TDM.Case(torch, code, c.packet, size, LAYOUT, before, TDM.outputs_of(pats))
        with TDM.make_plan(code, c.packet, size) as p:
            case.run(p, want, words, pats, ids, odd=(i % 2 == 1), expect=expect, what=SF.case_id(c))
            rmax = max(1, max(len(TDM.effective(code, pat)) for pat in pats))
            is_the_case(c, size, TDM.form_of(code, c.packet, rmax))


# ---------------------------------------------------------------- lsec_decode_magic_dev_rotated
def lost_devices(n, rows):
    """`rows` devices, the first and the last among them where there are two: over the seven stripes the rotation
    turns them into runs of logical chunks that hold data, parity and both"""
    return sorted(set(range(rows - 1)) | {n - 1})


@pytest.mark.parametrize("c", cases("patmagicrot"), ids=SF.case_id)
def test_decode_magic_rotated(cuda, c):
    code = code_of(c)
    lost = lost_devices(c.k + c.m, c.rows)
    assert len(lost) == c.rows
    for i, size in enumerate(decode_sizes(c)):
        before, want, words = TDM.rotated_inputs(code, c.packet, size, lost, N_SHIFT, FIRST)
        expect = list(words)
        expect[WRONG] ^= 1 << 16
        case = TDM.Case(torch, code, c.packet, size, LAYOUT, before, lost)
        with TDM.make_plan(code, c.packet, size) as p:
            case.run(p, want, words, lost=lost, n_shift=N_SHIFT, first=FIRST, rmax=c.rows, odd=(i % 2 == 1), expect=expect,
                     what=SF.case_id(c))
            is_the_case(c, size, TDM.form_of(code, c.packet, c.rows))


# ---------------------------------------------------------------- lsec_encode_magic_dev_rotated
@pytest.mark.parametrize("c", cases("encmagicrot"), ids=SF.case_id)
def test_encode_magic_rotated(cuda, c):
    """noise where the parity belongs: the reference's parity bytes at the rotated positions, and zlib's magics"""
    code = code_of(c)
    for size in SF.sizes(c):
        bench = TEM.Bench(torch, code, c.packet, size, LAYOUT)
        try:
            bench.run(N_SHIFT, FIRST)
            is_the_case(c, size, bench.form)
        finally:
            bench.close()
