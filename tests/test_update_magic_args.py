"""Host side of lsec_update_magic_dev_masked and lsec_update_magic_dev_masked_rotated (the masked parity update
that also keeps the stripes' adler32 magics current): the symbols, the header, the Python mirror, the
argument validation and the form prediction, checked without a GPU.  Everything the masked calls refuse
these refuse too, in the same order and with THIS call's name in the message; a NULL magic with stripes is
refused behind the mask array.  As in tests/test_update_masked_args.py the ladder refuses before it
reaches a device, so the pointers handed in are never dereferenced.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

from test_update_masked_args import CODES, FAKE, FIRST_MAX, MASKED_FORMS, MASKS, ROOT, fresh_of, shards_of

MAGIC = FAKE + (1 << 22) + 1  # odd: the magic words have no alignment rule
NAMES = {False: "lsec_update_magic_dev_masked", True: "lsec_update_magic_dev_masked_rotated"}
BOTH = (False, True)


def update(rotated, p, sh, nstripes, size, masks, fresh, flags=0, n_shift=1, first=5, magic=MAGIC):
    if rotated:
        return L.lib().lsec_update_magic_dev_masked_rotated(p.ptr, sh, nstripes, size, n_shift, first, masks, fresh, flags,
                                                            magic, None)
    return L.lib().lsec_update_magic_dev_masked(p.ptr, sh, nstripes, size, masks, fresh, flags, magic, None)


def refused(rotated, words, *args, **kw):
    assert update(rotated, *args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)
    assert NAMES[rotated] + ":" in msg or NAMES[rotated] + " " in msg, msg  # the message names THIS call


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
    # the scratch is said to come from the stream-ordered allocator; the plain update's sentence is not copied
    doc = header[header.index("The masked parity update that also keeps"):header.index("int lsec_update_magic_dev_masked(")]
    assert "stream-ordered" in doc and "16 bytes per stripe" in doc
    assert "Nothing is allocated" not in doc
    for name in ("update_magic_dev_masked_refs", "update_magic_dev_masked_rotated_refs", "update_magic_dev_masked"):
        assert callable(getattr(L.Plan, name))
    assert hasattr(lib, "lsec_test_predict_masked_magic_form")
    # the families of the existing hooks are as they were; the new one sits in a tuple of its own
    assert E.FORM_FAMILIES == ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
    assert E.MASKED_FAMILIES == ("updmask",)
    assert E.MAGIC_FAMILIES == ("updmaskmagic",)


def test_accepted_with_no_stripes(rs63, built):
    """no GPU is touched: this machine may have none"""
    null = shards_of(9, base=0, stride=0)
    for rot in BOTH:
        assert update(rot, rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6)) == 0, E.last_error()
        assert update(rot, rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), E.UPDATE_STORE) == 0, E.last_error()
        # NULL bases everywhere, a NULL mask array and a NULL magic
        assert update(rot, rs63, null, 0, 4096, None, fresh_of(6, base=0), magic=None) == 0, E.last_error()
        assert update(rot, rs63, shards_of(9), 0, 4096, None, fresh_of(6, enabled=(2,)), magic=None) == 0, E.last_error()
    assert update(True, rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), n_shift=10, first=FIRST_MAX) == 0, E.last_error()
    assert update(True, rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), n_shift=0, first=0) == 0, E.last_error()
    # the mirror
    refs = [(FAKE + i * 4096, 8192) for i in range(9)]
    fresh = [(0, 0)] * 6
    fresh[4] = (FAKE + 65536, 4096)
    rs63.update_magic_dev_masked_refs(refs, 0, 4096, MASKS, fresh, MAGIC)
    rs63.update_magic_dev_masked_refs(refs, 0, 4096, 0, fresh, 0, store=True)
    rs63.update_magic_dev_masked_rotated_refs(refs, 0, 4096, 1, 5, MASKS, fresh, MAGIC)
    rs63.update_magic_dev_masked_rotated_refs(refs, 0, 4096, 1, 5, 0, fresh, 0, store=True)
    # RAID4 (m = 1), Cauchy, and k = 64 (every bit of the word a column)
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        p.form_encoding_matrix()
        for rot in BOTH:
            assert update(rot, p, shards_of(7), 0, 4096, MASKS, fresh_of(6)) == 0, E.last_error()
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        for rot in BOTH:
            assert update(rot, p, shards_of(9), 0, 8 * 64 * 2, MASKS, fresh_of(6, enabled=(5, 2))) == 0, E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 64, 2, 8, 0, 8) as p:
        for rot in BOTH:
            assert update(rot, p, shards_of(66), 0, 4096, MASKS, fresh_of(64)) == 0, E.last_error()
            assert update(rot, p, shards_of(66), 0, 4096, MASKS, fresh_of(64, enabled=(63,)), magic=None) == 0, E.last_error()


def test_refuses_a_null_magic_with_stripes(rs63):
    for rot in BOTH:
        for n in (1, 3):
            refused(rot, "magic is NULL", rs63, shards_of(9), n, 4096, MASKS, fresh_of(6), magic=None)
    # behind the mask array's rungs, in front of the block size's
    for rot in BOTH:
        refused(rot, "stripe_cols is NULL", rs63, shards_of(9), 1, 4096, None, fresh_of(6), magic=None)
        refused(rot, "stripe_cols", rs63, shards_of(9), 1, 4096, MASKS + 4, fresh_of(6), magic=None)
        refused(rot, "magic is NULL", rs63, shards_of(9), 1, 4100, MASKS, fresh_of(6), magic=None)
        refused(rot, "multiple of 8", rs63, shards_of(9), 1, 4100, MASKS, fresh_of(6))


def test_columns_that_are_not_enabled_are_ignored(rs63):
    sh = shards_of(9)
    sh[0].base, sh[0].stride = 0, 0
    sh[3].base, sh[3].stride = FAKE + 3, 4097
    assert update(False, rs63, sh, 0, 4096, MASKS, fresh_of(6, enabled=(1, 5))) == 0, E.last_error()
    refused(False, "stripe_cols", rs63, sh, 2, 4096, MASKS + 4, fresh_of(6, enabled=(1, 5)))
    refused(True, "device 3: base", rs63, sh, 0, 4096, MASKS, fresh_of(6, enabled=(1, 5)))


def test_refuses_other_plan_kernels(built):
    for rot in BOTH:
        with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 3
            refused(rot, "plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4, MASKS, fresh_of(5))
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
            assert p.kernel == 4
            refused(rot, "plan kernel 4", p, shards_of(9), 0, 4096, MASKS, fresh_of(6))
        with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
            p.form_encoding_matrix()
            assert p.kernel == 5
            refused(rot, "plan kernel 5", p, shards_of(9), 0, 16 * 64, MASKS, fresh_of(6))


def test_refuses_wide_and_parityless_stripes(built):
    for rot in BOTH:
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
            refused(rot, "m=9", p, shards_of(15), 0, 4096, MASKS, fresh_of(6))
            assert "1..8" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
            refused(rot, "k=65", p, shards_of(68), 0, 4096, MASKS, fresh_of(65))
            assert "1..64" in E.last_error()
        with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
            refused(rot, "m=0", p, shards_of(6), 0, 4096, MASKS, fresh_of(6))


def test_refuses_null_pointers(rs63):
    refused(False, "shards is NULL", rs63, None, 0, 4096, MASKS, fresh_of(6))
    refused(True, "devs is NULL", rs63, None, 0, 4096, MASKS, fresh_of(6))
    for rot in BOTH:
        refused(rot, "fresh is NULL", rs63, shards_of(9), 0, 4096, MASKS, None)
        refused(rot, "stripe_cols is NULL", rs63, shards_of(9), 1, 4096, None, fresh_of(6))
        refused(rot, "stripe_cols is NULL", rs63, shards_of(9), 3, 4096, None, fresh_of(6, enabled=(0,)))


def test_refuses_a_misaligned_mask_array(rs63):
    for rot in BOTH:
        for off in (1, 4):
            refused(rot, "stripe_cols", rs63, shards_of(9), 1, 4096, MASKS + off, fresh_of(6))
            assert "multiple of 8 bytes" in E.last_error()
        assert update(rot, rs63, shards_of(9), 0, 4096, MASKS + 4, fresh_of(6)) == 0, E.last_error()  # not used


def test_refuses_a_call_without_an_enabled_column(rs63):
    for rot in BOTH:
        refused(rot, "no enabled column", rs63, shards_of(9), 1, 4096, MASKS, fresh_of(6, base=0))
        assert "k=6" in E.last_error()
        refused(rot, "no enabled column", rs63, shards_of(9), 2, 4096, MASKS, fresh_of(9, enabled=(6, 8)))


def test_refuses_a_null_shard_of_an_enabled_column(rs63):
    sh = shards_of(9)
    sh[2].base = 0
    refused(False, "shard 2: base is NULL", rs63, sh, 1, 4096, MASKS, fresh_of(6, enabled=(2, 4)))
    refused(False, "shard 2: base is NULL", rs63, sh, 1, 4096, MASKS, fresh_of(6))
    refused(False, "stripe_cols is NULL", rs63, sh, 1, 4096, None, fresh_of(6, enabled=(4,)))


def test_refuses_unknown_flags(rs63):
    for rot in BOTH:
        refused(rot, "bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), flags=2)
        refused(rot, "bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6),
                flags=E.UPDATE_STORE | 4)


def test_refuses_negative_rotation_and_stripes(rs63):
    refused(True, "n_shift -1 is negative", rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), n_shift=-1)
    refused(True, "first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, MASKS, fresh_of(6), first=-1)
    for rot in BOTH:
        refused(rot, "nstripes -1 is negative", rs63, shards_of(9), -1, 4096, MASKS, fresh_of(6))


def test_refuses_misaligned_refs(rs63):
    for i in (1, 5, 6, 8):
        sh = shards_of(9)
        sh[i].base = FAKE + i * 4096 + 4
        refused(False, f"shard {i}: base", rs63, sh, 0, 4096, MASKS, fresh_of(6, enabled=(1, 5)))
        assert "multiple of 8 bytes" in E.last_error()
    for d in range(9):
        sh = shards_of(9)
        sh[d].base = FAKE + d * 4096 + 4
        refused(True, f"device {d}: base", rs63, sh, 0, 4096, MASKS, fresh_of(6, enabled=(2,)))
        assert "multiple of 8 bytes" in E.last_error()
    for rot in BOTH:
        fr = fresh_of(6, enabled=(0, 3))
        fr[3].base += 12
        refused(rot, "fresh 3: base", rs63, shards_of(9), 0, 4096, MASKS, fr)
        sh = shards_of(9)
        sh[7].stride = 8196
        assert update(rot, rs63, sh, 0, 4096, MASKS, fresh_of(6)) == 0, E.last_error()
        refused(rot, "7: stride 8196", rs63, sh, 2, 4096, MASKS, fresh_of(6))
        fr = fresh_of(6)
        fr[1].stride = 4100
        assert update(rot, rs63, shards_of(9), 0, 4096, MASKS, fr) == 0, E.last_error()
        refused(rot, "fresh 1: stride 4100", rs63, shards_of(9), 2, 4096, MASKS, fr)


def test_refuses_block_sizes(rs63):
    for rot in BOTH:
        refused(rot, "multiple of 8", rs63, shards_of(9), 0, 4100, MASKS, fresh_of(6))
        refused(rot, "multiple of 8", rs63, shards_of(9), 0, -8, MASKS, fresh_of(6))
        with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
            p.form_encoding_matrix()
            refused(rot, "w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64, MASKS, fresh_of(6))


def test_ladder_order(rs63):
    """the refusals come in the order of the masked calls' list, the magic behind the mask array"""
    bad = shards_of(9)
    bad[0].base = FAKE + 4
    kw = dict(n_shift=-1, first=-1, magic=None)
    for rot in BOTH:
        refused(rot, "fresh is NULL", rs63, bad, -1, 4100, None, None, flags=8, **kw)
        refused(rot, "bits other than", rs63, bad, -1, 4100, None, fresh_of(6, base=0), flags=8, **kw)
    refused(True, "n_shift -1", rs63, bad, -1, 4100, None, fresh_of(6, base=0), **kw)
    refused(True, "first_stripe -1", rs63, bad, -1, 4100, None, fresh_of(6, base=0), first=-1, magic=None)
    for rot in BOTH:
        refused(rot, "no enabled column", rs63, bad, 1, 4100, None, fresh_of(6, base=0), magic=None)
        refused(rot, "0: base", rs63, bad, 1, 4100, None, fresh_of(6), magic=None)
        refused(rot, "stripe_cols is NULL", rs63, shards_of(9), 1, 4100, None, fresh_of(6), magic=None)
        refused(rot, "magic is NULL", rs63, shards_of(9), 1, 4100, MASKS, fresh_of(6), magic=None)
        refused(rot, "multiple of 8", rs63, shards_of(9), -1, 4100, MASKS, fresh_of(6))
        assert "block_size" in E.last_error()


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    assert L.lib().lsec_update_magic_dev_masked(fake, shards_of(9), 0, 4096, MASKS, fresh_of(6), 0, MAGIC, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert L.lib().lsec_update_magic_dev_masked_rotated(fake, shards_of(9), 0, 4096, 1, 0, MASKS, fresh_of(6), 0, MAGIC,
                                                        None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# The forms of the new family, (sliced, R, KC, IT, VW, BF, DW).  No form of it spills at the masked update's own
# launch shapes, so they are those: two 16-byte units per lane up to four rows and one beyond,
# branch-free; bit-sliced one dword per lane below K = 16, four from there where the packet holds them.
MAGIC_FORMS = {"rs63": (False, 3, 0, 2, 4, 1, 0), "rs128": (False, 8, 0, 1, 4, 1, 0), "cg63": (True, 3, 0, 0, 0, 0, 1),
               "cg164": (True, 4, 0, 0, 0, 0, 4)}


def test_predicted_forms(built):
    """the new family answers without a GPU, and the existing families answer what they answered"""
    for code, (kernel, k, m, packet, size) in CODES.items():
        f = E.predict_masked_magic_form(kernel, k, m, packet, size)
        assert f == E.Form("updmaskmagic", *MAGIC_FORMS[code]), (code, f)
    assert E.predict_masked_magic_form(1, 6, 1) == E.Form("updmaskmagic", False, 1, 0, 1, 2, 0, 0)
    for m in range(1, 9):
        f = E.predict_masked_magic_form(1, 10, m)
        assert f.family == "updmaskmagic" and f.R == m and not f.sliced
        f = E.predict_masked_magic_form(2, 10, m, 64, 8 * 64)
        assert f.R == m and f.sliced and f.DW in (1, 2, 4)
    out = (C.c_int * 8)()
    for kernel, packet in ((1, 0), (2, 64)):
        assert L.lib().lsec_test_predict_masked_magic_form(kernel, 10, 9, packet, 8 * 64, out) == -1
        assert "no kernel" in E.last_error() and "R=9" in E.last_error()
        assert L.lib().lsec_test_predict_masked_magic_form(kernel, 65, 3, packet, 8 * 64, out) == -1
        assert "K=65" in E.last_error()
        assert L.lib().lsec_test_predict_masked_magic_form(kernel, 64, 8, packet, 8 * 64, out) == 0, E.last_error()
        assert out[0] == 11  # appended behind the ten: every existing family keeps its number
    assert L.lib().lsec_test_predict_masked_magic_form(3, 6, 3, 0, 4096, out) == -1  # plan kernels 1 and 2 only
    # the existing families' predictions: the values predict_masked_form gave before this family existed
    for code in ("rs63", "rs128", "cg164"):
        kernel, k, m, packet, size = CODES[code]
        assert E.predict_masked_form(kernel, k, m, packet, size) == E.Form("updmask", *MASKED_FORMS[code]), code
    # and the older hook still has nine families
    assert L.lib().lsec_test_predict_form(10, 1, 6, 3, 0, 4096, out) == -1
    assert L.lib().lsec_test_predict_form(11, 1, 6, 3, 0, 4096, out) == -1
