"""Host side of lsec_decode_dev_patterns_rotated and lsec_decode_magic_dev_patterns_rotated (the patterned decodes
over the physical devices of a rotated LUN, plain and with the stripe magics): the symbols, the header, the Python
mirror, each call's refusal ladder rung by rung and in its order, and the form prediction, checked without a GPU.
Every refusal comes before the first HIP call, so the fake pointers handed in (the fakes of
tests/test_update_masked_args.py) are never dereferenced; the calls that would reach a device (nstripes == 0
prepares the tables there) are left to tests/test_gpu_patterns_rotated.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# keyed by "with the magics"
NAMES = {False: "lsec_decode_dev_patterns_rotated", True: "lsec_decode_magic_dev_patterns_rotated"}
BOTH = (False, True)
IDS = FAKE + (1 << 20) + 1    # stripe_pattern, magic, expect and bad have no alignment rule
MAGIC = FAKE + (2 << 20) + 1
EXPECT = FAKE + (3 << 20) + 3
BAD = FAKE + (4 << 20) + 1
COUNT = FAKE + (5 << 20)
PATS = ([], [2], [1, 7])


def pattern_array(pats):
    return None if pats is None else E._pattern_array(pats)


def call(magics, p, sh, nstripes, size, pats=PATS, ids=IDS, n_shift=1, first=5, magic=MAGIC, expect=None, bad=None,
         count=None, npat=None):
    lib = L.lib()
    npat = (0 if pats is None else len(pats)) if npat is None else npat
    if magics:
        return lib.lsec_decode_magic_dev_patterns_rotated(p.ptr, sh, nstripes, size, n_shift, first, pattern_array(pats), npat,
                                                          ids, magic, expect, bad, count, None)
    return lib.lsec_decode_dev_patterns_rotated(p.ptr, sh, nstripes, size, n_shift, first, pattern_array(pats), npat, ids, None)


def refused(magics, words, *args, **kw):
    assert call(magics, *args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)
    assert NAMES[magics] + ":" in msg or NAMES[magics] + " " in msg, msg  # the message names the call that was made


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
    # the argument order of lsec_search_dev_patterns_rotated: the rotation ahead of the list
    for name in NAMES.values():
        decl = header[header.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        order = [decl.index(w) for w in ("*plan", "*devs", "nstripes", "block_size", "n_shift", "first_stripe", "*patterns",
                                         "npatterns", "*stripe_pattern", "*stream")]
        assert order == sorted(order), decl
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    for name in ("decode_dev_patterns_rotated_refs", "decode_magic_dev_patterns_rotated_refs"):
        assert callable(getattr(L.Plan, name))
    assert hasattr(lib, "lsec_test_predict_pattern_magic_rot_form") and callable(E.predict_pattern_magic_rot_form)
    # the existing family tuples are as they were; the new family sits in a tuple of its own, behind them
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",) and E.CHKMAGIC_FAMILIES == ("chkmagic", "chkmagicrot")
    assert E.ENCMAGIC_FAMILIES == ("encmagicrot",) and E.SEARCH_FAMILIES == ("patsearch", "patsearchrot")
    assert E.PATMAGICROT_FAMILIES == ("patmagicrot",)
    assert E._form([18, 0, 3, 0, 1, 4, 1, 0]).family == "patmagicrot" and E._form([17, 1, 3, 0, 0, 0, 0, 1]).family == "patsearchrot"
    # the vote's and the search's comments name the takers of ids and found
    vote = header[header.index("The read path's quorum vote"):header.index("int lsec_vote_dev(")]
    search = header[header.index("The search for the erasure set"):header.index("int lsec_search_dev_patterns(")]
    for text in (vote, search):
        assert all(name in text for name in NAMES.values())


# ---------------------------------------------------------------- the refusal ladder
def test_refuses_other_plan_kernels(built):
    for mg in BOTH:
        with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:  # a liberation plan
            p.form_encoding_matrix()
            assert p.kernel == 3
            refused(mg, "kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
            assert p.kernel == 4
            refused(mg, "kernel 4", p, shards_of(9), 0, 4096)
        with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 5
            refused(mg, "kernel 5", p, shards_of(9), 0, 16 * 64)


def test_refuses_k_and_m_out_of_range(built):
    for mg in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
            refused(mg, "k=65", p, shards_of(68), 0, 4096)
            assert "1..64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
            assert call(mg, p, shards_of(6), 0, 4096) == -1  # no parity
            assert NAMES[mg] in E.last_error()
    # the magic call: 1 <= m <= 8; the plain call: k + m <= 128
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused(True, "m=9", p, shards_of(15), 0, 4096)
        assert "1..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 64, 65, 8, 0, 8) as p:
        refused(False, "k+m=129", p, shards_of(129), 0, 4096)


def test_refuses_null_pointers_and_negative_counts(rs63):
    for mg in BOTH:
        refused(mg, "devs is NULL", rs63, None, 0, 4096)
        refused(mg, "patterns is NULL", rs63, shards_of(9), 0, 4096, pats=None)
        refused(mg, "stripe_pattern is NULL", rs63, shards_of(9), 1, 4096, ids=None)
        assert call(mg, rs63, shards_of(9), -1, 4096) == -1  # (nstripes == 0 with a NULL stripe_pattern would reach the device)
        refused(mg, "nstripes -1 is negative", rs63, shards_of(9), -1, 4096)
        refused(mg, "n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
        refused(mg, "first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)
        refused(mg, "first_stripe -9223372036854775808 is negative", rs63, shards_of(9), 0, 4096, first=-(1 << 63))


def test_refuses_the_lists(rs63):
    for mg in BOTH:
        refused(mg, "npatterns=0", rs63, shards_of(9), 0, 4096, pats=[])
        refused(mg, "npatterns=257", rs63, shards_of(9), 0, 4096, pats=[[0]] * 257)
        assert "1..256" in E.last_error()
        refused(mg, "out of range", rs63, shards_of(9), 0, 4096, pats=[[0], [9]])  # an id out of range
        assert call(mg, rs63, shards_of(9), 0, 4096, pats=[[0, 1, 2, 3]]) == -1  # more than m erasures
        assert NAMES[mg] in E.last_error()


def test_refuses_a_misaligned_device_any_of_them(rs63):
    for mg in BOTH:
        for dev in range(9):  # all k+m entries are validated, whatever the patterns touch
            sh = shards_of(9)
            sh[dev].base = FAKE + dev * 4096 + 4
            refused(mg, f"shard {dev}: base", rs63, sh, 0, 4096, pats=[[]])
            assert "multiple of 8 bytes" in E.last_error()
            sh = shards_of(9)
            sh[dev].stride = 8196
            refused(mg, f"shard {dev}: stride 8196", rs63, sh, 2, 4096, pats=[[]])


def test_refuses_a_bad_block_size(rs63):
    for mg in BOTH:
        refused(mg, "multiple of 8", rs63, shards_of(9), 0, 4100)
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(mg, "w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)


def test_refuses_the_magic_arguments(rs63):
    refused(True, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None)
    refused(True, "magic is NULL", rs63, shards_of(9), 7, 4096, magic=None, expect=EXPECT)
    refused(True, "bad is given without expect", rs63, shards_of(9), 1, 4096, bad=BAD)
    refused(True, "bad is given without expect", rs63, shards_of(9), 0, 4096, bad=BAD, count=COUNT)
    refused(True, "bad_count is given without expect", rs63, shards_of(9), 1, 4096, count=COUNT)
    for off in (1, 2, 3):
        refused(True, "bad_count", rs63, shards_of(9), 1, 4096, expect=EXPECT, count=COUNT + off)
        assert "multiple of 4 bytes" in E.last_error()


def test_ladder_order(rs63):
    """The unrotated calls' ladders in their order, n_shift and first_stripe directly behind nstripes: each call below
    carries every later fault as well."""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    late = dict(magic=None, bad=BAD, count=COUNT + 1)
    every = dict(pats=None, ids=None, n_shift=-1, first=-1, **late)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as other:  # the magic call's own limits come first
        refused(True, "plan kernel 4", other, None, -1, 4100, **every)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
        refused(True, "m=9", wide, None, -1, 4100, **every)
    for mg in BOTH:
        refused(mg, "devs is NULL", rs63, None, -1, 4100, **every)
        refused(mg, "shard 0: base", rs63, bad_sh, -1, 4100, **every)
        refused(mg, "patterns is NULL", rs63, shards_of(9), -1, 4100, **every)
        refused(mg, "nstripes -1", rs63, shards_of(9), -1, 4100, **dict(every, pats=[[9]]))
        refused(mg, "n_shift -1", rs63, shards_of(9), 1, 4100, **dict(every, pats=[[9]]))
        refused(mg, "first_stripe -1", rs63, shards_of(9), 1, 4100, **dict(every, pats=[[9]], n_shift=1))
        refused(mg, "stripe_pattern is NULL", rs63, shards_of(9), 1, 4100, pats=[[9]], ids=None, **late)
        refused(mg, "multiple of 8", rs63, shards_of(9), 1, 4100, pats=[[9]], **late)
        refused(mg, "out of range", rs63, shards_of(9), 1, 4096, pats=[[9]], **late)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as other:  # the plain call: the plan kernel behind stripe_pattern
            if not mg:
                refused(mg, "stripe_pattern is NULL", other, shards_of(9), 1, 4100, pats=[[9]], ids=None)
                refused(mg, "kernel 4", other, shards_of(9), 1, 4100, pats=[[9]])
    refused(True, "magic is NULL", rs63, shards_of(9), 1, 4096, **late)
    refused(True, "bad is given", rs63, shards_of(9), 1, 4096, bad=BAD, count=COUNT + 1)
    refused(True, "bad_count is given", rs63, shards_of(9), 1, 4096, count=COUNT + 1)
    refused(True, "multiple of 4 bytes", rs63, shards_of(9), 1, 4096, expect=EXPECT, count=COUNT + 1)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    lib = L.lib()
    assert lib.lsec_decode_dev_patterns_rotated(fake, shards_of(9), 0, 4096, 1, 0, pattern_array(PATS), 3, IDS, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert lib.lsec_decode_magic_dev_patterns_rotated(fake, shards_of(9), 0, 4096, 1, 0, pattern_array(PATS), 3, IDS, MAGIC,
                                                      None, None, None, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# ---------------------------------------------------------------- the predictor
def test_predicted_forms(built):
    out = (C.c_int * 8)()
    for k in (1, 4, 6, 10, 16, 64):
        for rows in range(1, 9):
            # the shapes of the patterned decode with the magics, under the new family
            assert E.predict_pattern_magic_rot_form(1, k, rows) == \
                E.predict_pattern_magic_form(1, k, rows)._replace(family="patmagicrot"), (k, rows)
            assert E.predict_pattern_magic_rot_form(2, k, rows, 64) == \
                E.predict_pattern_magic_form(2, k, rows, 64)._replace(family="patmagicrot")
    assert E.predict_pattern_magic_rot_form(1, 6, 1) == E.Form("patmagicrot", False, 1, 6, 1, 2, 0, 0)
    lib = L.lib()
    for kernel, packet in ((1, 0), (2, 64)):
        assert lib.lsec_test_predict_pattern_magic_rot_form(kernel, 10, 9, packet, out) == -1
        assert "no kernel" in E.last_error() and "R=9" in E.last_error()
        assert lib.lsec_test_predict_pattern_magic_rot_form(kernel, 10, 0, packet, out) == -1
        assert lib.lsec_test_predict_pattern_magic_rot_form(kernel, 65, 3, packet, out) == -1
        assert "K=65" in E.last_error()
        assert lib.lsec_test_predict_pattern_magic_rot_form(kernel, 0, 3, packet, out) == -1
        assert lib.lsec_test_predict_pattern_magic_rot_form(kernel, 64, 8, packet, out) == 0, E.last_error()
        assert list(out)[:3] == [18, kernel - 1, 8]
    assert lib.lsec_test_predict_pattern_magic_rot_form(2, 6, 3, 6, out) == -1  # a packet no lane fits
    assert lib.lsec_test_predict_pattern_magic_rot_form(3, 6, 3, 0, out) == -1  # plan kernels 1 and 2 only
    # the existing hook still answers for its own families alone
    assert lib.lsec_test_predict_form(18, 1, 6, 3, 0, 4096, out) == -1


def family18_forms():
    """Every form of family 18 the dispatch can take, from the predictor: K 1..64 x R 1..8 bytewise, R 1..8 bit-sliced."""
    bytewise = {E.predict_pattern_magic_rot_form(1, k, rows) for k in range(1, 65) for rows in range(1, 9)}
    sliced = {E.predict_pattern_magic_rot_form(2, k, rows, 64) for k in range(1, 65) for rows in range(1, 9)}
    return bytewise, sliced


def test_form_enumeration_is_closed(built):
    """The plans of tests/test_gpu_patterns_rotated.py (FORM_PLANS there) reach every form of family 18: the three one-row
    bytewise forms (K = 6, K = 10, K at run time), for R >= 2 every IT form the constant yields, and R = 1..8 bit-sliced."""
    from test_gpu_patterns_rotated import FORM_PLANS
    bytewise, sliced = family18_forms()
    assert {f for f in bytewise if f.R == 1} == {E.Form("patmagicrot", False, 1, kc, 1, 2, 0, 0) for kc in (0, 6, 10)}
    for rows in range(2, 9):
        assert {(f.KC, f.VW, f.BF) for f in bytewise if f.R == rows} == {(0, 4, 1)}
        assert {f.IT for f in bytewise if f.R == rows} <= {1, 2}
    assert sliced == {E.Form("patmagicrot", True, rows, 0, 0, 0, 0, 1) for rows in range(1, 9)}
    covered = set()
    for kernel, k, m, rows, packet in FORM_PLANS:
        assert 1 <= rows <= min(m, 8)
        covered.add(E.predict_pattern_magic_rot_form(kernel, k, rows, packet))
    assert covered == bytewise | sliced, (bytewise | sliced) ^ covered
