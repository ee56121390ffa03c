"""Host side of lsec_vote_dev and lsec_vote_dev_rotated (the quorum vote over a stripe's stored magics): the symbols,
the header, the Python mirror and the whole refusal ladder in its order, checked without a GPU.  Every refusal comes
before the first HIP call, so the fake pointers handed in (the fakes of tests/test_update_masked_args.py) are never
dereferenced; the calls that reach a device are left to tests/test_gpu_vote.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {False: "lsec_vote_dev", True: "lsec_vote_dev_rotated"}
BOTH = (False, True)
QUORUM = FAKE + (1 << 20) + 1  # quorum, cls and ids have no alignment rule
CLS = FAKE + (2 << 20) + 3
IDS = FAKE + (3 << 20) + 1
OUTSIDE = FAKE + (4 << 20)
COUNTS = FAKE + (5 << 20) + 4
PATS = ([], [2], [1, 7])
CHUNKS = "chunks"  # the default: fake chunks for the plan's k+m


def stored_of(n, base=FAKE + (1 << 30) + 1, stride=4101):
    """k+m stored-magic entries at odd addresses with an odd stride: neither has an alignment rule"""
    st = (E.ShardRef * n)()
    for i in range(n):
        st[i].base, st[i].stride = base + i * (1 << 16), stride
    return st


def pattern_array(pats):
    return None if pats is None else E._pattern_array(pats)


def call(rotated, p, stored, nstripes, size, sh=CHUNKS, pats=PATS, n_shift=1, first=5, quorum=QUORUM, cls=CLS, ids=IDS,
         outside=OUTSIDE, counts=COUNTS, flags=0, npat=None):
    lib = L.lib()
    n = p.k + p.m
    if stored == "stored":
        stored = stored_of(n)
    if sh == CHUNKS:
        sh = shards_of(n)
    npat = (0 if pats is None else len(pats)) if npat is None else npat
    if rotated:
        return lib.lsec_vote_dev_rotated(p.ptr, stored, sh, nstripes, size, n_shift, first, pattern_array(pats), npat, quorum,
                                         cls, ids, outside, counts, flags, None)
    return lib.lsec_vote_dev(p.ptr, stored, sh, nstripes, size, pattern_array(pats), npat, quorum, cls, ids, outside, counts,
                             flags, None)


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
    # declared directly behind the search pair
    assert header.index("int lsec_search_dev_patterns_rotated(") < header.index("int lsec_vote_dev(") \
        < header.index("int lsec_vote_dev_rotated(") < header.index("int lsec_check_dev(")
    between = header[header.index("int lsec_search_dev_patterns_rotated("):header.index("int lsec_vote_dev(")]
    assert not re.search(r"^int\s+\w+\s*\(", between[4:], re.M)
    for name, value in (("OK", 0), ("DEGRADED", 1), ("BLANK", 2), ("LOST", 3), ("PARANOID", 1)):
        assert re.search(r"^#define\s+LSEC_VOTE_" + name + r"\s+" + str(value) + r"\b", header, re.M), name
        assert getattr(E, "VOTE_" + name) == value
    assert (E.LOCATE_CLEAN, E.LOCATE_MANY) == (0xFF, 0xFE)
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    for name in ("vote_dev_refs", "vote_dev_rotated_refs"):
        assert callable(getattr(L.Plan, name))
    assert hasattr(lib, "lsec_test_set_vote_form")
    # the launch record gained no family: every tuple is as it was
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",) and E.CHKMAGIC_FAMILIES == ("chkmagic", "chkmagicrot")
    assert E.ENCMAGIC_FAMILIES == ("encmagicrot",)
    assert E.SEARCH_FAMILIES == ("patsearch", "patsearchrot")


def test_validates_without_stripes(rs63):
    """nstripes == 0 without patterns validates and touches no device: every device pointer may be NULL"""
    for rot in BOTH:
        assert call(rot, rs63, "stored", 0, 4096, pats=None, ids=None) == 0, E.last_error()
        assert call(rot, rs63, "stored", 0, 0, sh=None, pats=None, quorum=None, cls=None, ids=None, outside=None,
                    counts=None) == 0, E.last_error()
        # without chunks block_size is not looked at
        assert call(rot, rs63, "stored", 0, 4100, sh=None, pats=None, ids=None) == 0, E.last_error()
        # an entry whose stored base is NULL is not validated
        st, sh = stored_of(9), shards_of(9)
        st[4].base = 0
        sh[4].base = FAKE + 3
        assert call(rot, rs63, st, 0, 4096, sh=sh, pats=None, ids=None) == 0, E.last_error()


# ---------------------------------------------------------------- the refusal ladder
def test_refuses_other_plan_kernels(built):
    for rot in BOTH:
        with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:  # a liberation plan
            p.form_encoding_matrix()
            assert p.kernel == 3
            refused(rot, "plan kernel 3", p, "stored", 0, 7 * 32 * 4)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
            assert p.kernel == 4
            refused(rot, "plan kernel 4", p, "stored", 0, 4096)
        with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 5
            refused(rot, "plan kernel 5", p, "stored", 0, 16 * 64)


def test_refuses_stripes_out_of_range(built):
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
            refused(rot, "m=9", p, "stored", 0, 4096)
            assert "1..8" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
            refused(rot, "k=65", p, "stored", 0, 4096)
            assert "1..64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
            refused(rot, "m=0", p, "stored", 0, 4096)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 57, 8, 8, 0, 8) as p:  # k and m in range, k + m = 65
            refused(rot, "k+m=65", p, "stored", 0, 4096)
            assert "64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 56, 8, 8, 0, 8) as p:  # k + m = 64 is taken
            assert call(rot, p, "stored", 0, 4096, pats=None, ids=None) == 0, E.last_error()


def test_refuses_the_arguments(rs63):
    for rot in BOTH:
        refused(rot, "stored is NULL", rs63, None, 0, 4096)
        refused(rot, "nstripes -1 is negative", rs63, "stored", -1, 4096)
        # the list: what the patterned decode refuses, then the search's limit
        refused(rot, "npatterns=0", rs63, "stored", 0, 4096, pats=[])
        refused(rot, "out of range", rs63, "stored", 0, 4096, pats=[[0], [9]])
        assert call(rot, rs63, "stored", 0, 4096, pats=[[0, 1, 2, 3]]) == -1  # m + 1 erasures
        assert NAMES[rot] in E.last_error()
        refused(rot, "npatterns=255", rs63, "stored", 0, 4096, pats=[[0]] * 255)
        assert "1..254" in E.last_error()
        refused(rot, "npatterns=257", rs63, "stored", 0, 4096, pats=[[0]] * 257)
        refused(rot, "ids is given without patterns", rs63, "stored", 0, 4096, pats=None)
        # the chunks: lsec_check_dev's layout and block_size rules
        sh = shards_of(9)
        sh[4].base = FAKE + 4 * 4096 + 4
        refused(rot, "shard 4: base", rs63, "stored", 0, 4096, sh=sh)
        assert "multiple of 8 bytes" in E.last_error()
        sh = shards_of(9)
        sh[7].stride = 8196
        refused(rot, "shard 7: stride 8196", rs63, "stored", 2, 4096, sh=sh)
        assert call(rot, rs63, "stored", 0, 4096, sh=sh, pats=None, ids=None) == 0  # one stripe uses no stride
        refused(rot, "multiple of 8", rs63, "stored", 0, 4100)
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(rot, "w*packet_size = 512", p, "stored", 0, 8 * 64 * 2 + 64)
        # the outputs
        refused(rot, "quorum is NULL", rs63, "stored", 1, 4096, quorum=None)
        refused(rot, "cls is NULL", rs63, "stored", 7, 4096, cls=None)
        for off in range(1, 8):
            refused(rot, "outside", rs63, "stored", 1, 4096, outside=OUTSIDE + off)
            assert "multiple of 8 bytes" in E.last_error()
        for off in (1, 2, 3):
            refused(rot, "counts", rs63, "stored", 1, 4096, counts=COUNTS + off)
            assert "multiple of 4 bytes" in E.last_error()
        refused(rot, "unknown flags 0x2", rs63, "stored", 1, 4096, flags=2)
        refused(rot, "unknown flags 0x3", rs63, "stored", 1, 4096, flags=3)
        refused(rot, "unknown flags", rs63, "stored", 0, 4096, flags=-2)
    refused(True, "n_shift -1 is negative", rs63, "stored", 0, 4096, n_shift=-1)
    refused(True, "first_stripe -1 is negative", rs63, "stored", 0, 4096, first=-1)


def test_ladder_order(rs63):
    """plan kernel; k, m, k+m; stored; nstripes; n_shift and first_stripe; the list's own refusals; npatterns > 254; ids
    without patterns; the chunks' layout and block_size; quorum and cls; outside and counts; flags: each call below
    carries every later fault as well"""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    many = [[0]] * 255
    late = dict(quorum=None, cls=None, outside=OUTSIDE + 4, counts=COUNTS + 1, flags=2)
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as other:
            refused(rot, "plan kernel 4", other, None, -1, 4100, pats=[[9]], n_shift=-1, first=-1, **late)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
            refused(rot, "m=9", wide, None, -1, 4100, pats=[[9]], n_shift=-1, first=-1, **late)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 57, 8, 8, 0, 8) as wide:
            refused(rot, "k+m=65", wide, None, -1, 4100, pats=[[99]], n_shift=-1, first=-1, **late)
        refused(rot, "stored is NULL", rs63, None, -1, 4100, sh=bad_sh, pats=[[9]], n_shift=-1, first=-1, **late)
        refused(rot, "nstripes -1", rs63, "stored", -1, 4100, sh=bad_sh, pats=[[9]], n_shift=-1, first=-1, **late)
        if rot:
            refused(rot, "n_shift -1", rs63, "stored", 2, 4100, sh=bad_sh, pats=[[9]], n_shift=-1, first=-1, **late)
            refused(rot, "first_stripe -1", rs63, "stored", 2, 4100, sh=bad_sh, pats=[[9]], first=-1, **late)
        refused(rot, "out of range", rs63, "stored", 2, 4100, sh=bad_sh, pats=[[9]] + many[1:], **late)
        refused(rot, "npatterns=255", rs63, "stored", 2, 4100, sh=bad_sh, pats=many, **late)
        refused(rot, "ids is given without patterns", rs63, "stored", 2, 4100, sh=bad_sh, pats=None, **late)
        refused(rot, "shard 0: base", rs63, "stored", 2, 4100, sh=bad_sh, **late)
        refused(rot, "multiple of 8", rs63, "stored", 2, 4100, **late)
        refused(rot, "quorum is NULL", rs63, "stored", 2, 4096, **late)
        refused(rot, "cls is NULL", rs63, "stored", 2, 4096, **dict(late, quorum=QUORUM))
        refused(rot, "outside", rs63, "stored", 2, 4096, outside=OUTSIDE + 4, counts=COUNTS + 1, flags=2)
        refused(rot, "counts", rs63, "stored", 2, 4096, counts=COUNTS + 1, flags=2)
        refused(rot, "unknown flags", rs63, "stored", 2, 4096, flags=2)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    lib = L.lib()
    assert lib.lsec_vote_dev(fake, stored_of(9), None, 0, 4096, None, 0, None, None, None, None, None, 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert lib.lsec_vote_dev_rotated(fake, stored_of(9), None, 0, 4096, 1, 0, None, 0, None, None, None, None, None, 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
