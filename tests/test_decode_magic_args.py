"""Host side of lsec_decode_magic_dev_patterns and lsec_decode_magic_dev_rotated (the patterned decode that also
leaves every stripe's adler32 magic): the symbols, the header, the Python mirror, the argument validation,
the unused-survivor lists the magic form adds to a pattern's record, and the form prediction, checked
without a GPU.  Every refusal comes before the first HIP call, so the fake pointers handed in (the fakes of
tests/test_update_masked_args.py) are never dereferenced; the calls that would reach a device (nstripes == 0
prepares the tables there) are left to tests/test_gpu_decode_magic.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {False: "lsec_decode_magic_dev_patterns", True: "lsec_decode_magic_dev_rotated"}
BOTH = (False, True)
IDS = FAKE + (1 << 20)      # stripe_pattern
MAGIC = FAKE + (2 << 20) + 1  # magic and expect have no alignment rule
EXPECT = FAKE + (3 << 20) + 3
BAD = FAKE + (4 << 20) + 1
COUNT = FAKE + (5 << 20)
PATS = ([], [2], [1, 7])


def pattern_array(pats):
    return None if pats is None else E._pattern_array(pats)


def call(rotated, p, sh, nstripes, size, pats=PATS, ids=IDS, lost=(1,), n_shift=1, first=5, magic=MAGIC, expect=None,
         bad=None, count=None, npat=None):
    lib = L.lib()
    if rotated:
        return lib.lsec_decode_magic_dev_rotated(p.ptr, sh, nstripes, size, None if lost is None else E._erasure_array(lost),
                                                 n_shift, first, magic, expect, bad, count, None)
    return lib.lsec_decode_magic_dev_patterns(p.ptr, sh, nstripes, size, pattern_array(pats),
                                              (0 if pats is None else len(pats)) if npat is None else npat, ids, magic,
                                              expect, bad, count, None)


def refused(rotated, words, *args, **kw):
    assert call(rotated, *args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)
    assert NAMES[rotated] + ":" in msg or NAMES[rotated] + " " in msg, msg  # the message names the call


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbols_header_mirror_and_abi_version(built):
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "lstore_ec.h")) as f:
        header = f.read()
    for name in NAMES.values():
        assert name in E.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M)
    # declared behind lsec_decode_dev_rotated
    assert header.index("int lsec_decode_dev_rotated(") < header.index("int lsec_decode_magic_dev_patterns(") \
        < header.index("int lsec_decode_magic_dev_rotated(") < header.index("int lsec_check_dev(")
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    for name in ("decode_magic_dev_patterns_refs", "decode_magic_dev_rotated_refs", "decode_magic_dev_patterns"):
        assert callable(getattr(L.Plan, name))
    for hook in ("lsec_test_predict_pattern_magic_form", "lsec_test_pattern_unused"):
        assert hasattr(lib, hook)
    # the existing family tuples are as they were; the new family sits in a tuple of its own, behind them
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",)


# ---------------------------------------------------------------- the refusal ladder
def test_refuses_other_plan_kernels(built):
    for rot in BOTH:
        with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:  # a liberation plan
            p.form_encoding_matrix()
            assert p.kernel == 3
            refused(rot, "plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
            assert p.kernel == 4
            refused(rot, "plan kernel 4", p, shards_of(9), 0, 4096)
        with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 5
            refused(rot, "plan kernel 5", p, shards_of(9), 0, 16 * 64)


def test_refuses_wide_and_parityless_stripes(built):
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
            refused(rot, "m=9", p, shards_of(15), 0, 4096)
            assert "1..8" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
            refused(rot, "k=65", p, shards_of(68), 0, 4096)
            assert "1..64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
            refused(rot, "m=0", p, shards_of(6), 0, 4096)


def test_refuses_what_the_plain_calls_refuse(rs63):
    refused(False, "shards is NULL", rs63, None, 0, 4096)
    refused(True, "devs is NULL", rs63, None, 0, 4096)
    for rot in BOTH:
        sh = shards_of(9)
        sh[4].base = FAKE + 4 * 4096 + 4
        refused(rot, "shard 4: base", rs63, sh, 0, 4096)
        assert "multiple of 8 bytes" in E.last_error()
        sh = shards_of(9)
        sh[7].stride = 8196
        refused(rot, "shard 7: stride 8196", rs63, sh, 2, 4096)
        refused(rot, "nstripes -1 is negative", rs63, shards_of(9), -1, 4096)
        refused(rot, "multiple of 8", rs63, shards_of(9), 0, 4100)
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(rot, "w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)
    # the patterned call's own
    refused(False, "patterns is NULL", rs63, shards_of(9), 0, 4096, pats=None)
    refused(False, "stripe_pattern is NULL", rs63, shards_of(9), 1, 4096, ids=None)
    refused(False, "npatterns=0", rs63, shards_of(9), 0, 4096, pats=[])
    refused(False, "npatterns=257", rs63, shards_of(9), 0, 4096, pats=[[0]] * 257)
    refused(False, "out of range", rs63, shards_of(9), 0, 4096, pats=[[0], [9]])
    assert call(False, rs63, shards_of(9), 0, 4096, pats=[[0, 1, 2, 3]]) == -1  # more than m erasures
    assert NAMES[False] in E.last_error()
    # the rotated call's own
    refused(True, "lost is NULL", rs63, shards_of(9), 0, 4096, lost=None)
    refused(True, "n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
    refused(True, "first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)
    refused(True, "lost device 9 out of range", rs63, shards_of(9), 0, 4096, lost=(9,))
    refused(True, "exceed m=3", rs63, shards_of(9), 0, 4096, lost=(0, 1, 2, 3))


def test_refuses_the_magic_arguments(rs63):
    for rot in BOTH:
        refused(rot, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None)
        refused(rot, "magic is NULL", rs63, shards_of(9), 7, 4096, magic=None, expect=EXPECT)
        refused(rot, "bad is given without expect", rs63, shards_of(9), 1, 4096, bad=BAD)
        refused(rot, "bad is given without expect", rs63, shards_of(9), 0, 4096, bad=BAD, count=COUNT)
        refused(rot, "bad_count is given without expect", rs63, shards_of(9), 1, 4096, count=COUNT)
        for off in (1, 2, 3):
            refused(rot, "bad_count", rs63, shards_of(9), 1, 4096, expect=EXPECT, count=COUNT + off)
            assert "multiple of 4 bytes" in E.last_error()


def test_ladder_order(rs63):
    """the call's own limits, then the plain call's refusals in its order, then the magic's"""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
        refused(False, "m=9", wide, None, -1, 4100, pats=None, magic=None, bad=BAD)
        refused(True, "m=9", wide, None, -1, 4100, lost=None, n_shift=-1, magic=None, bad=BAD)
    refused(False, "shards is NULL", rs63, None, -1, 4100, pats=None, magic=None, bad=BAD)
    refused(False, "shard 0: base", rs63, bad_sh, -1, 4100, pats=None, magic=None, bad=BAD)
    refused(False, "patterns is NULL", rs63, shards_of(9), -1, 4100, pats=None, magic=None, bad=BAD)
    refused(False, "nstripes -1", rs63, shards_of(9), -1, 4100, magic=None, bad=BAD)
    refused(False, "stripe_pattern is NULL", rs63, shards_of(9), 1, 4100, ids=None, magic=None, bad=BAD)
    refused(False, "multiple of 8", rs63, shards_of(9), 1, 4100, pats=[[9]], magic=None, bad=BAD)
    refused(False, "out of range", rs63, shards_of(9), 1, 4096, pats=[[9]], magic=None, bad=BAD)
    refused(False, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None, bad=BAD, count=COUNT + 1)
    refused(False, "bad is given", rs63, shards_of(9), 1, 4096, bad=BAD, count=COUNT + 1)
    refused(False, "bad_count is given", rs63, shards_of(9), 1, 4096, count=COUNT + 1)
    refused(False, "multiple of 4 bytes", rs63, shards_of(9), 1, 4096, expect=EXPECT, count=COUNT + 1)
    refused(True, "devs is NULL", rs63, None, -1, 4100, lost=None, n_shift=-1, first=-1, magic=None, bad=BAD)
    refused(True, "lost is NULL", rs63, shards_of(9), -1, 4100, lost=None, n_shift=-1, first=-1, magic=None, bad=BAD)
    refused(True, "nstripes -1", rs63, shards_of(9), -1, 4100, n_shift=-1, first=-1, magic=None, bad=BAD)
    refused(True, "n_shift -1", rs63, shards_of(9), 1, 4100, n_shift=-1, first=-1, magic=None, bad=BAD)
    refused(True, "first_stripe -1", rs63, shards_of(9), 1, 4100, first=-1, magic=None, bad=BAD)
    refused(True, "multiple of 8", rs63, shards_of(9), 1, 4100, lost=(9,), magic=None, bad=BAD)
    refused(True, "lost device 9", rs63, shards_of(9), 1, 4096, lost=(9,), magic=None, bad=BAD)
    refused(True, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None, bad=BAD)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    lib = L.lib()
    assert lib.lsec_decode_magic_dev_patterns(fake, shards_of(9), 0, 4096, pattern_array(PATS), 3, IDS, MAGIC, None, None, None,
                                              None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert lib.lsec_decode_magic_dev_rotated(fake, shards_of(9), 0, 4096, E._erasure_array((1,)), 1, 0, MAGIC, None, None, None,
                                             None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# ---------------------------------------------------------------- the unused-survivor lists
def test_unused_survivors_rs63(rs63):
    pats = [[], [2], [1, 7], [0, 3, 8]]
    for pid, (pat, count) in enumerate(zip(pats, (3, 2, 1, 0))):
        nout, in_sel, out_sel, unused = E.pattern_unused_entry(rs63, pid, patterns=pats)
        assert nout == len(pat) and out_sel == pat
        assert len(unused) == count and unused == sorted(unused)
        assert sorted(in_sel + out_sel + unused) == list(range(9)), (pat, in_sel, out_sel, unused)
        if pat:  # the inputs and outputs are the plain table's own
            nout0, in0, out0, _ = E.pattern_table_entry(rs63, pid, patterns=pats)
            assert (nout0, in0, out0) == (nout, in_sel, out_sel)
    # the empty pattern: the checksum-only path reads the data chunks as its inputs and the parity as unused
    assert E.pattern_unused_entry(rs63, 0, patterns=pats) == (0, [0, 1, 2, 3, 4, 5], [], [6, 7, 8])
    # the plain hook shows an empty entry as it did
    assert E.pattern_table_entry(rs63, 0, patterns=pats)[:3] == (0, [-1] * 6, [])


def test_unused_survivors_raid4_parity_only(built):
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        p.form_encoding_matrix()
        nout, in_sel, out_sel, unused = E.pattern_unused_entry(p, 0, patterns=[[6], [2]])
        assert (nout, in_sel, out_sel, unused) == (0, [0, 1, 2, 3, 4, 5], [], [6])  # all 7 chunks summed, none written
        nout, in_sel, out_sel, unused = E.pattern_unused_entry(p, 1, patterns=[[6], [2]])
        assert nout == 1 and out_sel == [2] and unused == [] and sorted(in_sel + out_sel) == list(range(7))


def test_unused_survivors_rotated(rs63):
    """lost = {1}, n_shift = 1: every rotation occurs; the record of rotation p holds PHYSICAL devices, and
    (device + p) mod n are the logical chunks: all nine, once each, the lost device the one rebuilt"""
    n = 9
    for rot in range(n):
        nout, in_sel, out_sel, unused = E.pattern_unused_entry(rs63, rot, lost=[1], n_shift=1)
        assert nout == 1 and out_sel == [1] and len(unused) == 2
        assert sorted(in_sel + out_sel + unused) == list(range(n))
        logical = lambda devs: [(d + rot) % n for d in devs]  # noqa: E731
        assert logical(unused) == sorted(logical(unused))  # ascending by logical id
        lost_logical = (1 + rot) % n
        # the decode reads the first k logical survivors; the unused ones are the last two
        survivors = [c for c in range(n) if c != lost_logical]
        assert sorted(logical(in_sel)) == survivors[:6] and logical(unused) == survivors[6:]
    # n_shift = 3: rotations 0, 3, 6 only; an unreachable one is the checksum-only record of its rotation
    nout, in_sel, out_sel, unused = E.pattern_unused_entry(rs63, 1, lost=[1], n_shift=3)
    assert nout == -1 and out_sel == []
    assert [(d + 1) % n for d in in_sel] == list(range(6)) and [(d + 1) % n for d in unused] == [6, 7, 8]
    # no lost device: every stripe is only checksummed
    for rot in range(n):
        nout, in_sel, out_sel, unused = E.pattern_unused_entry(rs63, rot, lost=[], n_shift=1)
        assert nout == 0 and [(d + rot) % n for d in in_sel + unused] == list(range(n))


def test_unused_hook_refuses_wide_parity(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        with pytest.raises(L.ErasureError, match="m=9"):
            E.pattern_unused_entry(p, 0, patterns=[[0]])


# ---------------------------------------------------------------- the predictor
def test_predicted_forms(built):
    out = (C.c_int * 8)()
    for k in (1, 4, 6, 10, 16, 64):
        for rows in range(1, 9):
            f = E.predict_pattern_magic_form(1, k, rows)
            # the patterned kernels' own shapes
            assert f == E.predict_form("pat", 1, k, rows)._replace(family="patmagic"), (k, rows, f)
            g = E.predict_pattern_magic_form(2, k, rows, 64)
            assert g == E.Form("patmagic", True, rows, 0, 0, 0, 0, 1)
    # one row: the fixed-K forms at K = 6 and 10, 8 bytes per lane, per-cell branches
    assert E.predict_pattern_magic_form(1, 6, 1) == E.Form("patmagic", False, 1, 6, 1, 2, 0, 0)
    assert E.predict_pattern_magic_form(1, 7, 1).KC == 0
    lib = L.lib()
    for kernel, packet in ((1, 0), (2, 64)):
        assert lib.lsec_test_predict_pattern_magic_form(kernel, 10, 9, packet, out) == -1
        assert "no kernel" in E.last_error() and "R=9" in E.last_error()
        assert lib.lsec_test_predict_pattern_magic_form(kernel, 10, 0, packet, out) == -1
        assert lib.lsec_test_predict_pattern_magic_form(kernel, 65, 3, packet, out) == -1
        assert "K=65" in E.last_error()
        assert lib.lsec_test_predict_pattern_magic_form(kernel, 0, 3, packet, out) == -1
        assert lib.lsec_test_predict_pattern_magic_form(kernel, 64, 8, packet, out) == 0, E.last_error()
    assert lib.lsec_test_predict_pattern_magic_form(2, 6, 3, 6, out) == -1  # a packet no lane fits
    assert lib.lsec_test_predict_pattern_magic_form(3, 6, 3, 0, out) == -1  # plan kernels 1 and 2 only
    # the existing hooks still answer for their own families alone
    assert lib.lsec_test_predict_form(12, 1, 6, 3, 0, 4096, out) == -1
