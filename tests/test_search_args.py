"""Host side of lsec_search_dev_patterns and lsec_search_dev_patterns_rotated (the search for the erasure set that
fits a stripe's quorum magic): the symbols, the header, the Python mirror, the whole refusal ladder in its order,
and the form prediction, checked without a GPU.  Every refusal comes before the first HIP call, so the fake
pointers handed in (the fakes of tests/test_update_masked_args.py) are never dereferenced; the calls that would
reach a device (nstripes == 0 prepares the tables there) are left to tests/test_gpu_search.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {False: "lsec_search_dev_patterns", True: "lsec_search_dev_patterns_rotated"}
BOTH = (False, True)
SELECT = FAKE + (1 << 20) + 1  # select, expect, found and trial have no alignment rule
EXPECT = FAKE + (2 << 20) + 3
FOUND = FAKE + (3 << 20) + 1
TRIAL = FAKE + (4 << 20) + 1
COUNTS = FAKE + (5 << 20)
PATS = ([], [2], [1, 7])


def pattern_array(pats):
    return None if pats is None else E._pattern_array(pats)


def call(rotated, p, sh, nstripes, size, pats=PATS, n_shift=1, first=5, select=SELECT, expect=EXPECT, found=FOUND,
         trial=TRIAL, counts=COUNTS, flags=0, npat=None):
    lib = L.lib()
    npat = (0 if pats is None else len(pats)) if npat is None else npat
    if rotated:
        return lib.lsec_search_dev_patterns_rotated(p.ptr, sh, nstripes, size, n_shift, first, pattern_array(pats), npat,
                                                    select, expect, found, trial, counts, flags, None)
    return lib.lsec_search_dev_patterns(p.ptr, sh, nstripes, size, pattern_array(pats), npat, select, expect, found, trial,
                                        counts, flags, None)


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
    # declared behind lsec_decode_magic_dev_rotated
    assert header.index("int lsec_decode_magic_dev_rotated(") < header.index("int lsec_search_dev_patterns(") \
        < header.index("int lsec_search_dev_patterns_rotated(") < header.index("int lsec_check_dev(")
    assert re.search(r"^#define\s+LSEC_SEARCH_REPAIR\s+1\b", header, re.M) and E.SEARCH_REPAIR == 1
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    for name in ("search_dev_patterns_refs", "search_dev_patterns_rotated_refs", "search_dev_patterns"):
        assert callable(getattr(L.Plan, name))
    for hook in ("lsec_test_predict_search_form", "lsec_test_set_search_form"):
        assert hasattr(lib, hook)
    # the existing family tuples are as they were; the new families sit in a tuple of their own, behind them
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",) and E.CHKMAGIC_FAMILIES == ("chkmagic", "chkmagicrot")
    assert E.ENCMAGIC_FAMILIES == ("encmagicrot",)
    assert E.SEARCH_FAMILIES == ("patsearch", "patsearchrot")
    assert E._form([16, 0, 3, 0, 1, 4, 1, 0]).family == "patsearch" and E._form([17, 1, 3, 0, 0, 0, 0, 1]).family == "patsearchrot"


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


def test_refuses_what_the_patterned_decode_refuses(rs63):
    refused(False, "shards is NULL", rs63, None, 0, 4096)
    refused(True, "devs is NULL", rs63, None, 0, 4096)
    for rot in BOTH:
        sh = shards_of(9)
        sh[4].base = FAKE + 4 * 4096 + 4  # a misaligned base
        refused(rot, "shard 4: base", rs63, sh, 0, 4096)
        assert "multiple of 8 bytes" in E.last_error()
        sh = shards_of(9)
        sh[7].stride = 8196
        refused(rot, "shard 7: stride 8196", rs63, sh, 2, 4096)
        refused(rot, "patterns is NULL", rs63, shards_of(9), 0, 4096, pats=None)
        refused(rot, "nstripes -1 is negative", rs63, shards_of(9), -1, 4096)
        refused(rot, "multiple of 8", rs63, shards_of(9), 0, 4100)
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(rot, "w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)
        refused(rot, "npatterns=0", rs63, shards_of(9), 0, 4096, pats=[])
        refused(rot, "out of range", rs63, shards_of(9), 0, 4096, pats=[[0], [9]])  # an id out of range
        assert call(rot, rs63, shards_of(9), 0, 4096, pats=[[0, 1, 2, 3]]) == -1  # m + 1 erasures
        assert NAMES[rot] in E.last_error()
    refused(True, "n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
    refused(True, "first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)


def test_refuses_the_search_arguments(rs63):
    for rot in BOTH:
        refused(rot, "npatterns=255", rs63, shards_of(9), 0, 4096, pats=[[0]] * 255)
        assert "1..254" in E.last_error()
        refused(rot, "npatterns=256", rs63, shards_of(9), 0, 4096, pats=[[0]] * 256)
        refused(rot, "nstripes * npatterns", rs63, shards_of(9), (1 << 30), 4096, pats=[[0], [1]])
        assert "2^31" in E.last_error()
        refused(rot, "expect is NULL", rs63, shards_of(9), 1, 4096, expect=None)
        refused(rot, "found is NULL", rs63, shards_of(9), 7, 4096, found=None)
        for off in (1, 2, 3):
            refused(rot, "counts", rs63, shards_of(9), 1, 4096, counts=COUNTS + off)
            assert "multiple of 4 bytes" in E.last_error()
        refused(rot, "unknown flags 0x2", rs63, shards_of(9), 1, 4096, flags=2)
        refused(rot, "unknown flags 0x3", rs63, shards_of(9), 1, 4096, flags=3)
        refused(rot, "unknown flags", rs63, shards_of(9), 0, 4096, flags=-2)


def test_ladder_order(rs63):
    """plan kernel, k and m, then the patterned decode's refusals in its order, then npatterns > 254, the pair count,
    expect and found, counts, flags: each call below carries every later fault as well"""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    many = [[0]] * 255
    late = dict(expect=None, found=None, counts=COUNTS + 1, flags=2)
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as other:
            refused(rot, "plan kernel 4", other, None, -1, 4100, pats=None, n_shift=-1, first=-1, **late)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
            refused(rot, "m=9", wide, None, -1, 4100, pats=None, n_shift=-1, first=-1, **late)
        refused(rot, "devs is NULL" if rot else "shards is NULL", rs63, None, -1, 4100, pats=None, n_shift=-1, first=-1, **late)
        refused(rot, "shard 0: base", rs63, bad_sh, -1, 4100, pats=None, n_shift=-1, first=-1, **late)
        refused(rot, "patterns is NULL", rs63, shards_of(9), -1, 4100, pats=None, n_shift=-1, first=-1, **late)
        refused(rot, "nstripes -1", rs63, shards_of(9), -1, 4100, pats=many, n_shift=-1, first=-1, **late)
        if rot:
            refused(rot, "n_shift -1", rs63, shards_of(9), 1 << 30, 4100, pats=many, n_shift=-1, first=-1, **late)
            refused(rot, "first_stripe -1", rs63, shards_of(9), 1 << 30, 4100, pats=many, first=-1, **late)
        refused(rot, "multiple of 8", rs63, shards_of(9), 1 << 30, 4100, pats=[[9]] + many[1:], **late)
        refused(rot, "out of range", rs63, shards_of(9), 1 << 30, 4096, pats=[[9]] + many[1:], **late)
        refused(rot, "npatterns=255", rs63, shards_of(9), 1 << 30, 4096, pats=many, **late)
        refused(rot, "nstripes * npatterns", rs63, shards_of(9), 1 << 30, 4096, pats=many[:2], **late)
        refused(rot, "expect is NULL", rs63, shards_of(9), 1, 4096, **late)
        refused(rot, "found is NULL", rs63, shards_of(9), 1, 4096, **dict(late, expect=EXPECT))
        refused(rot, "multiple of 4 bytes", rs63, shards_of(9), 1, 4096, counts=COUNTS + 1, flags=2)
        refused(rot, "unknown flags", rs63, shards_of(9), 1, 4096, flags=2)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    lib = L.lib()
    assert lib.lsec_search_dev_patterns(fake, shards_of(9), 0, 4096, pattern_array(PATS), 3, None, EXPECT, FOUND, None, None, 0,
                                        None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert lib.lsec_search_dev_patterns_rotated(fake, shards_of(9), 0, 4096, 1, 0, pattern_array(PATS), 3, None, EXPECT, FOUND,
                                                None, None, 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# ---------------------------------------------------------------- the predictor
def test_predicted_forms(built):
    out = (C.c_int * 8)()
    for rot, family in ((False, "patsearch"), (True, "patsearchrot")):
        for k in (1, 4, 6, 10, 16, 64):
            for rows in range(1, 9):
                # the shapes of the patterned decode with the magics, under the new family
                assert E.predict_search_form(rot, 1, k, rows) == \
                    E.predict_pattern_magic_form(1, k, rows)._replace(family=family), (k, rows)
                assert E.predict_search_form(rot, 2, k, rows, 64) == \
                    E.predict_pattern_magic_form(2, k, rows, 64)._replace(family=family)
        assert E.predict_search_form(rot, 1, 6, 1) == E.Form(family, False, 1, 6, 1, 2, 0, 0)
    lib = L.lib()
    for kernel, packet in ((1, 0), (2, 64)):
        assert lib.lsec_test_predict_search_form(0, kernel, 10, 9, packet, out) == -1
        assert "no kernel" in E.last_error() and "R=9" in E.last_error()
        assert lib.lsec_test_predict_search_form(1, kernel, 10, 0, packet, out) == -1
        assert lib.lsec_test_predict_search_form(0, kernel, 65, 3, packet, out) == -1
        assert "K=65" in E.last_error()
        assert lib.lsec_test_predict_search_form(1, kernel, 64, 8, packet, out) == 0, E.last_error()
        assert list(out)[:3] == [17, kernel - 1, 8]
    assert lib.lsec_test_predict_search_form(0, 2, 6, 3, 6, out) == -1  # a packet no lane fits
    assert lib.lsec_test_predict_search_form(0, 3, 6, 3, 0, out) == -1  # plan kernels 1 and 2 only
    # the existing hooks still answer for their own families alone
    assert lib.lsec_test_predict_form(16, 1, 6, 3, 0, 4096, out) == -1
    assert lib.lsec_test_predict_form(17, 1, 6, 3, 0, 4096, out) == -1
