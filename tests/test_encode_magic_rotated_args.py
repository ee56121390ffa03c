"""Host side of lsec_encode_magic_dev_rotated (the full-stripe write over the physical devices of a rotated LUN
that also leaves every stripe's adler32 magic): the symbol, the header, the Python mirror, the whole refusal ladder
in its order and the form prediction, checked without a GPU.  Every refusal comes before the first HIP call, so the
fake pointers handed in (the fakes of tests/test_update_masked_args.py) are never dereferenced, and nstripes == 0
validates and touches no GPU: that these tests pass on a machine without one is the proof.  The stride rule only
applies once a second stripe uses the stride, so it is checked at nstripes == 2: the ladder refuses before it
reaches a device.  What reaches a device is left to tests/test_gpu_encode_magic_rotated.py.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import FAKE, shards_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lsec_encode_magic_dev_rotated"
MAGIC = FAKE + (2 << 20) + 1   # magic has no alignment rule
FIRST_MAX = (1 << 63) - 1


def call(p, devs, nstripes, size, n_shift=1, first=5, magic=MAGIC):
    return L.lib().lsec_encode_magic_dev_rotated(p.ptr, devs, nstripes, size, n_shift, first, magic, None)


def refused(words, *args, **kw):
    assert call(*args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)
    assert NAME + ":" in msg or NAME + " " in msg, msg  # the message names the call


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbol_header_mirror_and_abi_version(built):
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "lstore_ec.h")) as f:
        header = f.read()
    assert NAME in E.EXPORTS and hasattr(lib, NAME)
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M)
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the call by its symbol
    assert re.search(r"^#define\s+LSEC_ABI_VERSION\s+3\b", header, re.M)
    doc = header[header.index("lsec_encode_dev_rotated that also leaves"):header.index("int " + NAME + "(")]
    assert "stream-ordered" in doc and "16 bytes per stripe" in doc and "no fallback to two passes" in doc
    assert "LOGICAL order" in doc and "adler32 of nothing" in doc
    # lsec_encode_dev_rotated's own comment points to the call
    rotated_doc = header[header.index("lsec_encode_dev_rotated: for every stripe"):header.index("lsec_update_dev_rotated: lsec_update_dev with")]
    assert NAME in rotated_doc
    for name in ("encode_magic_dev_rotated_refs", "encode_magic_dev_rotated"):
        assert callable(getattr(L.Plan, name))
    assert hasattr(lib, "lsec_test_predict_encode_magic_form") and callable(E.predict_encode_magic_form)
    # the existing family tuples are as they were; the new family sits in a tuple of its own, behind them
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",) and E.MAGIC_FAMILIES == ("updmaskmagic",)
    assert E.PATMAGIC_FAMILIES == ("patmagic",) and E.CHKMAGIC_FAMILIES == ("chkmagic", "chkmagicrot")
    assert E.ENCMAGIC_FAMILIES == ("encmagicrot",)
    assert E._form([15, 0, 3, 6, 2, 4, 1, 0]).family == "encmagicrot" and E._form([14, 1, 3, 0, 0, 0, 0, 2]).family == "chkmagicrot"


def test_zero_stripes_validate_only(rs63):
    """nstripes == 0: everything is validated, nothing is touched; magic and all bases may be NULL"""
    null = shards_of(9, base=0, stride=0)
    assert call(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    assert call(rs63, shards_of(9), 0, 4096, magic=None) == 0, E.last_error()
    assert call(rs63, null, 0, 4096, magic=None) == 0, E.last_error()  # NULL bases: the prepare-ahead convention
    assert call(rs63, shards_of(9), 0, 0, magic=None) == 0, E.last_error()
    assert call(rs63, shards_of(9), 0, 4096, n_shift=0, first=0) == 0, E.last_error()
    assert call(rs63, shards_of(9), 0, 4096, n_shift=10, first=FIRST_MAX) == 0, E.last_error()  # taken mod k+m
    for off in (0, 1, 2, 3):  # every odd address passes
        assert call(rs63, shards_of(9), 0, 4096, magic=MAGIC + off) == 0, E.last_error()
    # the mirror
    refs = [(FAKE + i * 4096, 8192) for i in range(9)]
    rs63.encode_magic_dev_rotated_refs(refs, 0, 4096, 1, 5, 0)
    rs63.encode_magic_dev_rotated_refs(refs, 0, 4096, 1, 5, MAGIC)
    # RAID4 (m = 1)
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        p.form_encoding_matrix()
        assert p.kernel == 1
        assert call(p, shards_of(7), 0, 4096, magic=None) == 0, E.last_error()
    # Cauchy
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert call(p, shards_of(9), 0, 8 * 64 * 2, magic=None) == 0, E.last_error()


# ---------------------------------------------------------------- the refusal ladder, one rung at a time
def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        refused("plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
        assert "plan kernel 1" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        refused("plan kernel 4", p, shards_of(9), 0, 4096)
    with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 5
        refused("plan kernel 5", p, shards_of(9), 0, 16 * 64)


def test_refuses_k_and_m_out_of_range(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        refused("k=65", p, shards_of(68), 0, 4096)
        assert "1..64" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused("m=9", p, shards_of(15), 0, 4096)
        assert "1..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
        refused("m=0", p, shards_of(6), 0, 4096)
        assert "1..8" in E.last_error()


def test_refuses_negative_counts_and_offsets(rs63):
    refused("nstripes -1 is negative", rs63, shards_of(9), -1, 4096)
    refused("n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
    refused("first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)


def test_refuses_bad_block_size(rs63):
    refused("multiple of 8", rs63, shards_of(9), 0, 4100)
    refused("multiple of 8", rs63, shards_of(9), 1, 4)
    refused("multiple of 8", rs63, shards_of(9), 0, -8)
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        refused("w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)


def test_refuses_misaligned_refs_on_every_device(rs63):
    """all k+m devices are validated: under rotation every one holds data in some stripes and parity in others"""
    for d in range(9):  # 0..5 hold data at rotation 0, 6..8 parity
        sh = shards_of(9)
        sh[d].base = FAKE + d * 4096 + 4
        refused(f"{d}: base", rs63, sh, 0, 4096)
        assert "multiple of 8 bytes" in E.last_error()
    for d in (0, 4, 8):
        sh = shards_of(9)
        sh[d].stride = 8196
        assert call(rs63, sh, 0, 4096) == 0, E.last_error()  # (the stride matters once a second stripe uses it)
        assert call(rs63, sh, 1, 4100) == -1 and "block_size" in E.last_error()  # past the stride rule
        refused(f"{d}: stride 8196", rs63, sh, 2, 4096)
        assert "multiple of 8 bytes" in E.last_error()


def test_refuses_null_pointers(rs63):
    refused("devs is NULL", rs63, None, 0, 4096)
    refused("magic is NULL", rs63, shards_of(9), 1, 4096, magic=None)
    assert "nstripes > 0" in E.last_error()
    refused("magic is NULL", rs63, shards_of(9), 7, 0, magic=None)  # an empty chunk still gets its words


def test_ladder_order(rs63):
    """lsec_encode_dev_rotated's refusals in its order -- devs, their alignment, plan kernel, k, m, nstripes, n_shift,
    first_stripe, block_size -- then a NULL magic: every call has everything behind the rung under test wrong as well"""
    bad_sh = shards_of(9)
    bad_sh[0].base = FAKE + 4
    wrong = dict(n_shift=-1, first=-1, magic=None)
    refused("devs is NULL", rs63, None, -1, 4100, **wrong)
    refused("shard 0: base", rs63, bad_sh, -1, 4100, **wrong)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p16:
        refused("plan kernel 4", p16, shards_of(9), -1, 4100, **wrong)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 9, 8, 0, 8) as wide:
        refused("k=65", wide, shards_of(74), -1, 4100, **wrong)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as wide:
        refused("m=9", wide, shards_of(15), -1, 4100, **wrong)
    refused("nstripes -1", rs63, shards_of(9), -1, 4100, **wrong)
    refused("n_shift -1", rs63, shards_of(9), 1, 4100, **wrong)
    refused("first_stripe -1", rs63, shards_of(9), 1, 4100, first=-1, magic=None)
    refused("multiple of 8", rs63, shards_of(9), 1, 4100, magic=None)
    refused("magic is NULL", rs63, shards_of(9), 1, 4096, magic=None)


def test_the_same_order_as_the_plain_call(rs63):
    """with the same wrong arguments lsec_encode_dev_rotated stops at the same rung, and its message is this call's
    without the name in front (or, where the plain message carries its own name, with that name replaced)"""
    lib = L.lib()
    bad_sh = shards_of(9)
    bad_sh[3].base = FAKE + 4
    cases = [(rs63, None, -1, 4100, -1, -1), (rs63, bad_sh, -1, 4100, -1, -1), (rs63, shards_of(9), -1, 4100, -1, -1),
             (rs63, shards_of(9), 1, 4100, -1, -1), (rs63, shards_of(9), 1, 4100, 1, -1), (rs63, shards_of(9), 1, 4100, 1, 5)]
    for p, devs, nstripes, size, n_shift, first in cases:
        assert lib.lsec_encode_dev_rotated(p.ptr, devs, nstripes, size, n_shift, first, None) == -1
        plain = E.last_error()
        assert call(p, devs, nstripes, size, n_shift, first, None) == -1
        assert E.last_error() == NAME + ": " + plain, (plain, E.last_error())
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 9, 8, 0, 8) as p:
        assert lib.lsec_encode_dev_rotated(p.ptr, shards_of(74), -1, 4100, -1, -1, None) == -1
        plain = E.last_error()
        assert call(p, shards_of(74), -1, 4100, -1, -1, None) == -1
        assert E.last_error() == plain.replace("lsec_encode_dev_rotated", NAME)


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    assert L.lib().lsec_encode_magic_dev_rotated(fake, shards_of(9), 0, 4096, 1, 0, MAGIC, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


def test_plain_call_messages_are_as_they_were(rs63):
    """the plain call shares the path: its messages carry no new prefix"""
    lib = L.lib()
    assert lib.lsec_encode_dev_rotated(rs63.ptr, shards_of(9), -1, 4096, 1, 0, None) == -1
    assert E.last_error() == "nstripes -1 is negative"
    assert lib.lsec_encode_dev_rotated(rs63.ptr, shards_of(9), 0, 4096, -1, 0, None) == -1
    assert E.last_error() == "n_shift -1 is negative"
    assert lib.lsec_encode_dev_rotated(rs63.ptr, shards_of(9), 0, 4100, 1, 0, None) == -1
    assert E.last_error() == "block_size 4100 is not a multiple of 8"
    assert lib.lsec_encode_dev_rotated(rs63.ptr, None, 0, 4096, 1, 0, None) == -1
    assert E.last_error() == "devs is NULL"


# ---------------------------------------------------------------- the predictor
def test_predicted_forms(built):
    """The rule the code implements: the rotated encode's own form for the same K x R, packet and chunk size
    (chk_bytewise_form through encmagicrot_bytewise_form; the rotated encode's lane dwords), with the family replaced:
    no form is narrowed, every one fits the register file without scratch."""
    for k in range(1, 65):
        for rows in range(1, 9):
            f = E.predict_encode_magic_form(1, k, rows, 0, 4096)
            assert f == E.predict_form("encrot", 1, k, rows, 0, 4096)._replace(family="encmagicrot"), (k, rows, f)
            assert not f.sliced and f.DW == 0 and f.KC in (0, k)
            for packet in (8, 24, 64):
                for size in (8 * packet, 8 * packet * 64, 1 << 20):
                    size -= size % (8 * packet)
                    g = E.predict_encode_magic_form(2, k, rows, packet, size)
                    assert g == E.predict_form("encrot", 2, k, rows, packet, size)._replace(family="encmagicrot")
                    assert g.sliced and g.DW in (1, 2, 4) and packet % (4 * g.DW) == 0 and (g.KC, g.IT, g.VW, g.BF) == (0,) * 4
    assert E.predict_encode_magic_form(1, 6, 3) == E.Form("encmagicrot", False, 3, 6, 2, 4, 1, 0)
    assert E.predict_encode_magic_form(2, 16, 4, 64, 8 * 64 * 65) == E.Form("encmagicrot", True, 4, 0, 0, 0, 0, 4)
    out = (C.c_int * 8)()
    lib = L.lib()
    for kernel, packet in ((1, 0), (2, 64)):
        assert lib.lsec_test_predict_encode_magic_form(kernel, 10, 9, packet, 4096, out) == -1
        assert "no kernel" in E.last_error() and "R=9" in E.last_error()
        assert lib.lsec_test_predict_encode_magic_form(kernel, 10, 0, packet, 4096, out) == -1
        assert lib.lsec_test_predict_encode_magic_form(kernel, 65, 3, packet, 4096, out) == -1
        assert "K=65" in E.last_error()
        assert lib.lsec_test_predict_encode_magic_form(kernel, 0, 3, packet, 4096, out) == -1
        assert lib.lsec_test_predict_encode_magic_form(kernel, 64, 8, packet, 4096, out) == 0, E.last_error()
    assert lib.lsec_test_predict_encode_magic_form(2, 6, 3, 6, 4096, out) == -1  # a packet no lane fits
    assert lib.lsec_test_predict_encode_magic_form(3, 6, 3, 0, 4096, out) == -1  # plan kernels 1 and 2 only
    assert lib.lsec_test_predict_encode_magic_form(1, 6, 3, 0, 4096, None) == -1
    assert lib.lsec_test_predict_form(15, 1, 6, 3, 0, 4096, out) == -1  # the old hook answers for no new family
