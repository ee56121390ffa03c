"""Host side of lsec_check_magic_dev and lsec_check_magic_dev_rotated (the parity check that also leaves every
stripe's adler32 magic): the symbols, the header, the Python mirror, the whole refusal ladder in its order
and the form prediction, checked without a GPU.  Every refusal comes before the first HIP call, so the fake
pointers handed in (the fakes of tests/test_update_masked_args.py) are never dereferenced, and nstripes == 0
validates and touches no GPU.  What reaches a device is left to tests/test_gpu_check_magic.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {False: "lsec_check_magic_dev", True: "lsec_check_magic_dev_rotated"}
BOTH = (False, True)
SYN = FAKE + (1 << 20)
MAGIC = FAKE + (2 << 20) + 1   # magic, expect and bad have no alignment rule
EXPECT = FAKE + (3 << 20) + 3
BAD = FAKE + (4 << 20) + 1
COUNTS = FAKE + (5 << 20)


def call(rotated, p, sh, nstripes, size, n_shift=1, first=5, syn=SYN, magic=MAGIC, expect=None, bad=None, counts=None):
    lib = L.lib()
    if rotated:
        return lib.lsec_check_magic_dev_rotated(p.ptr, sh, nstripes, size, n_shift, first, syn, magic, expect, bad, counts, None)
    return lib.lsec_check_magic_dev(p.ptr, sh, nstripes, size, syn, magic, expect, bad, counts, None)


def refused(rotated, words, *args, **kw):
    assert call(rotated, *args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)
    assert NAMES[rotated] + ":" in msg or NAMES[rotated] + " " in msg, msg  # the message names the call
    if not rotated:
        assert NAMES[True] not in msg, msg


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
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    assert re.search(r"^#define\s+LSEC_SCRUB_BAD_PARITY\s+1\b", header, re.M) and E.SCRUB_BAD_PARITY == 1
    assert re.search(r"^#define\s+LSEC_SCRUB_BAD_MAGIC\s+2\b", header, re.M) and E.SCRUB_BAD_MAGIC == 2
    doc = header[header.index("The scrub's two questions in one pass"):header.index("int lsec_check_magic_dev(")]
    assert "stream-ordered" in doc and "16 bytes per stripe" in doc and "no fallback to two passes" in doc
    for name in ("check_magic_dev_refs", "check_magic_dev_rotated_refs", "check_magic_dev", "check_magic_dev_rotated"):
        assert callable(getattr(L.Plan, name))
    assert hasattr(lib, "lsec_test_predict_check_magic_form")
    # the existing family tuples are as they were; the new families sit in a tuple of their own, behind them
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",)
    assert E.CHKMAGIC_FAMILIES == ("chkmagic", "chkmagicrot")
    assert E._form([13, 0, 3, 6, 2, 4, 1, 0]).family == "chkmagic" and E._form([14, 1, 3, 0, 0, 0, 0, 2]).family == "chkmagicrot"


def test_zero_stripes_validate_only(rs63):
    """nstripes == 0: everything is validated, nothing is touched; all outputs may be NULL"""
    for rot in BOTH:
        assert call(rot, rs63, shards_of(9), 0, 4096, syn=None, magic=None) == 0, E.last_error()
        assert call(rot, rs63, shards_of(9), 0, 4096, expect=EXPECT, bad=BAD, counts=COUNTS) == 0, E.last_error()
        assert call(rot, rs63, shards_of(9), 0, 4096, bad=BAD, counts=COUNTS) == 0, E.last_error()  # bad without expect
        assert call(rot, rs63, shards_of(9), 0, 0, syn=None, magic=None) == 0, E.last_error()
    assert call(True, rs63, shards_of(9), 0, 4096, n_shift=0, first=(1 << 63) - 1, syn=None, magic=None) == 0
    assert call(True, rs63, shards_of(9), 0, 4096, n_shift=9 * 7 + 2, syn=None, magic=None) == 0  # taken mod k+m


# ---------------------------------------------------------------- the refusal ladder, one rung at a time
def test_refuses_other_plan_kernels(built):
    for rot in BOTH:
        with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:  # a liberation plan
            p.form_encoding_matrix()
            assert p.kernel == 3
            refused(rot, "plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
            assert "plan kernel 1" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
            assert p.kernel == 4
            refused(rot, "plan kernel 4", p, shards_of(9), 0, 4096)
        with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 5
            refused(rot, "plan kernel 5", p, shards_of(9), 0, 16 * 64)


def test_refuses_k_and_m_out_of_range(built):
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
            refused(rot, "k=65", p, shards_of(68), 0, 4096)
            assert "1..64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
            refused(rot, "m=9", p, shards_of(15), 0, 4096)
            assert "1..8" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
            refused(rot, "m=0", p, shards_of(6), 0, 4096)
            assert "1..8" in E.last_error()


def test_refuses_negative_counts_and_offsets(rs63):
    for rot in BOTH:
        refused(rot, "nstripes -1 is negative", rs63, shards_of(9), -1, 4096)
    refused(True, "n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
    refused(True, "first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)


def test_refuses_bad_block_size(rs63):
    for rot in BOTH:
        refused(rot, "multiple of 8", rs63, shards_of(9), 0, 4100)
        refused(rot, "multiple of 8", rs63, shards_of(9), 1, 4)
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(rot, "w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)


def test_refuses_null_pointers(rs63):
    refused(False, "shards is NULL", rs63, None, 0, 4096)
    refused(True, "devs is NULL", rs63, None, 0, 4096)
    for rot in BOTH:
        refused(rot, "syndrome is NULL", rs63, shards_of(9), 1, 4096, syn=None)
        refused(rot, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None)
        refused(rot, "magic is NULL", rs63, shards_of(9), 7, 4096, magic=None, expect=EXPECT, bad=BAD, counts=COUNTS)
        assert "nstripes > 0" in E.last_error()


def test_refuses_misaligned_pointers(rs63):
    for rot in BOTH:
        for off in (1, 2, 3):
            refused(rot, "syndrome", rs63, shards_of(9), 1, 4096, syn=SYN + off)
            assert "multiple of 4 bytes" in E.last_error()
            refused(rot, "counts", rs63, shards_of(9), 1, 4096, expect=EXPECT, counts=COUNTS + off)
            assert "multiple of 4 bytes" in E.last_error()
            refused(rot, "counts", rs63, shards_of(9), 0, 4096, counts=COUNTS + off)  # without stripes and without expect too
        sh = shards_of(9)
        sh[4].base = FAKE + 4 * 4096 + 4
        refused(rot, "shard 4: base", rs63, sh, 0, 4096)
        assert "multiple of 8 bytes" in E.last_error()
        sh = shards_of(9)
        sh[7].stride = 8196
        refused(rot, "shard 7: stride 8196", rs63, sh, 2, 4096)
        assert call(rot, rs63, sh, 0, 4096) == 0  # (the stride matters once a second stripe uses it)
        # magic, expect and bad have no alignment rule: every odd address passes
        for off in (0, 1, 2, 3):
            assert call(rot, rs63, shards_of(9), 0, 4096, magic=MAGIC + off, expect=EXPECT + off, bad=BAD + off) == 0


def test_ladder_order(rs63):
    """lsec_check_dev's refusals in its order -- shards, their alignment, plan kernel, k, m, nstripes, n_shift,
    first_stripe, block_size, a NULL syndrome, its alignment -- then a NULL magic, then counts: every call has
    everything behind the rung under test wrong as well"""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    wrong = dict(syn=None, magic=None, counts=COUNTS + 1)
    for rot in BOTH:
        refused(rot, "devs is NULL" if rot else "shards is NULL", rs63, None, -1, 4100, n_shift=-1, first=-1, **wrong)
        refused(rot, "shard 0: base", rs63, bad_sh, -1, 4100, n_shift=-1, first=-1, **wrong)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p16:
            refused(rot, "plan kernel 4", p16, shards_of(9), -1, 4100, n_shift=-1, first=-1, **wrong)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 9, 8, 0, 8) as wide:
            refused(rot, "k=65", wide, shards_of(74), -1, 4100, n_shift=-1, first=-1, **wrong)
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
            refused(rot, "m=9", wide, shards_of(15), -1, 4100, n_shift=-1, first=-1, **wrong)
        refused(rot, "nstripes -1", rs63, shards_of(9), -1, 4100, n_shift=-1, first=-1, **wrong)
        if rot:
            refused(rot, "n_shift -1", rs63, shards_of(9), 1, 4100, n_shift=-1, first=-1, **wrong)
            refused(rot, "first_stripe -1", rs63, shards_of(9), 1, 4100, first=-1, **wrong)
        refused(rot, "multiple of 8", rs63, shards_of(9), 1, 4100, **wrong)
        refused(rot, "syndrome is NULL", rs63, shards_of(9), 1, 4096, **wrong)
        refused(rot, "syndrome", rs63, shards_of(9), 1, 4096, syn=SYN + 2, magic=None, counts=COUNTS + 1)
        assert "multiple of 4 bytes" in E.last_error()
        refused(rot, "magic is NULL", rs63, shards_of(9), 1, 4096, magic=None, counts=COUNTS + 1)
        refused(rot, "counts", rs63, shards_of(9), 1, 4096, counts=COUNTS + 1)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    lib = L.lib()
    assert lib.lsec_check_magic_dev(fake, shards_of(9), 0, 4096, SYN, MAGIC, None, None, None, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert lib.lsec_check_magic_dev_rotated(fake, shards_of(9), 0, 4096, 1, 0, SYN, MAGIC, None, None, None, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


def test_plain_check_messages_are_as_they_were(rs63):
    """the plain calls share the ladder: their messages carry no new prefix"""
    lib = L.lib()
    assert lib.lsec_check_dev(rs63.ptr, shards_of(9), -1, 4096, SYN, None, None) == -1
    assert E.last_error() == "nstripes -1 is negative"
    assert lib.lsec_check_dev_rotated(rs63.ptr, shards_of(9), 1, 4096, 1, 0, None, None, None) == -1
    assert E.last_error() == "syndrome is NULL"


# ---------------------------------------------------------------- the predictor
def test_predicted_forms(built):
    """The rule the code implements: the check's own form for the same K x R, packet and chunk size
    (chk_bytewise_form through chkmagic_bytewise_form; the check's lane dwords), with the family replaced.
    The one register-driven deviation is out of this rule's reach: the bit-sliced forms of 2 and 4 dwords per lane
    stop at six rows (the 4-dword form of eight rows would use scratch), and the policy that feeds the dispatch and
    this hook alike (cauchy8_bitsliced_dw) asks for one dword per lane above four rows.  Every form that exists fits
    the register file without scratch."""
    for rot, old, new in ((False, "chk", "chkmagic"), (True, "chkrot", "chkmagicrot")):
        for k in range(1, 65):
            for rows in range(1, 9):
                f = E.predict_check_magic_form(rot, 1, k, rows, 0, 4096)
                assert f == E.predict_form(old, 1, k, rows, 0, 4096)._replace(family=new), (k, rows, f)
                assert not f.sliced and f.DW == 0 and f.KC in (0, k)
                for packet in (8, 24, 64):
                    for size in (8 * packet, 8 * packet * 64, 1 << 20):
                        g = E.predict_check_magic_form(rot, 2, k, rows, packet, size - size % (8 * packet))
                        assert g == E.predict_form(old, 2, k, rows, packet, size - size % (8 * packet))._replace(family=new)
                        assert g.sliced and g.DW in (1, 2, 4) and packet % (4 * g.DW) == 0 and (g.KC, g.IT, g.VW, g.BF) == (0,) * 4
    assert E.predict_check_magic_form(False, 1, 6, 3) == E.Form("chkmagic", False, 3, 6, 2, 4, 1, 0)
    out = (C.c_int * 8)()
    lib = L.lib()
    for rot in (0, 1):
        for kernel, packet in ((1, 0), (2, 64)):
            assert lib.lsec_test_predict_check_magic_form(rot, kernel, 10, 9, packet, 4096, out) == -1
            assert "no kernel" in E.last_error() and "R=9" in E.last_error()
            assert lib.lsec_test_predict_check_magic_form(rot, kernel, 10, 0, packet, 4096, out) == -1
            assert lib.lsec_test_predict_check_magic_form(rot, kernel, 65, 3, packet, 4096, out) == -1
            assert "K=65" in E.last_error()
            assert lib.lsec_test_predict_check_magic_form(rot, kernel, 0, 3, packet, 4096, out) == -1
            assert lib.lsec_test_predict_check_magic_form(rot, kernel, 64, 8, packet, 4096, out) == 0, E.last_error()
        assert lib.lsec_test_predict_check_magic_form(rot, 2, 6, 3, 6, 4096, out) == -1  # a packet no lane fits
        assert lib.lsec_test_predict_check_magic_form(rot, 3, 6, 3, 0, 4096, out) == -1  # plan kernels 1 and 2 only
        assert lib.lsec_test_predict_check_magic_form(rot, 1, 6, 3, 0, 4096, None) == -1


def test_old_hooks_answer_as_before(built):
    """E.predict_form answers for the nine old families, under their own names, and for no new one"""
    for i, fam in enumerate(E.FORM_FAMILIES):
        rows = 1 if fam == "patrot" else 3
        for kernel, packet in ((1, 0), (2, 64)):
            f = E.predict_form(fam, kernel, 6, rows, packet, 1 << 16)
            assert f.family == fam and f.R == rows and f.sliced == (kernel == 2)
    assert E.predict_form("chk", 1, 6, 3) == E.Form("chk", False, 3, 6, 2, 4, 1, 0)
    out = (C.c_int * 8)()
    for family in (13, 14):
        assert L.lib().lsec_test_predict_form(family, 1, 6, 3, 0, 4096, out) == -1
