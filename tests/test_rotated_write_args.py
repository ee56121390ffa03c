"""Host side of lsec_encode_dev_rotated and lsec_update_dev_rotated (the write side over the physical
devices of a rotated LUN): the symbols, the header, the Python mirror, the argument validation and the
form prediction, checked without a GPU.  nstripes == 0 validates everything and touches no GPU, so
every refusal here is reached before anything could be enqueued; the pointers handed in are never
dereferenced.  The stride rule only applies once a second stripe uses the stride, so it is checked at
nstripes == 2: the ladder refuses before it reaches a device.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # an address that is a multiple of 8: only its alignment is looked at
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_MAX = (1 << 63) - 1


def shards_of(n, base=FAKE, stride=8192):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = (base + i * 4096 if base else 0), stride
    return sh


def ids(*cols):
    return (C.c_int * (len(cols) + 1))(*cols, -1)


def encode(p, devs, nstripes, size, n_shift=1, first=5):
    return L.lib().lsec_encode_dev_rotated(p.ptr, devs, nstripes, size, n_shift, first, None)


def update(p, devs, nstripes, size, cols, fresh, flags=0, n_shift=1, first=5):
    return L.lib().lsec_update_dev_rotated(p.ptr, devs, nstripes, size, n_shift, first, cols, fresh, flags, None)


def refused(call, words, *args, **kw):
    assert call(*args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)


def both_refused(words, p, devs, nstripes, size, **kw):
    """the refusals the two calls share: the update with one valid column"""
    refused(encode, words, p, devs, nstripes, size, **kw)
    refused(update, words, p, devs, nstripes, size, ids(0), shards_of(1), **kw)


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbols_header_mirror_and_abi_version(built):
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "lstore_ec.h")) as f:
        header = f.read()
    for name in ("lsec_encode_dev_rotated", "lsec_update_dev_rotated"):
        assert name in E.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M)
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    assert "there is no form over the physical devices" not in header
    for name in ("encode_dev_rotated_refs", "update_dev_rotated_refs"):
        assert callable(getattr(L.Plan, name))
    assert E.FORM_FAMILIES[7:] == ("encrot", "updrot")


def test_accepted_with_no_stripes(rs63, built):
    null = shards_of(9, base=0, stride=0)
    assert encode(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    assert encode(rs63, null, 0, 4096) == 0, E.last_error()  # NULL bases: the prepare-ahead convention
    assert update(rs63, shards_of(9), 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
    assert update(rs63, shards_of(9), 0, 4096, ids(2), shards_of(1), E.UPDATE_STORE) == 0, E.last_error()
    assert update(rs63, null, 0, 4096, ids(0, 1), shards_of(2, base=0, stride=0)) == 0, E.last_error()
    # c = k, a descending list, n_shift beyond k+m, the largest first_stripe
    assert update(rs63, shards_of(9), 0, 4096, ids(0, 1, 2, 3, 4, 5), shards_of(6)) == 0, E.last_error()
    assert update(rs63, shards_of(9), 0, 4096, ids(5, 3, 0), shards_of(3), n_shift=10, first=FIRST_MAX) == 0, E.last_error()
    assert encode(rs63, shards_of(9), 0, 4096, n_shift=10, first=FIRST_MAX) == 0, E.last_error()
    assert encode(rs63, shards_of(9), 0, 4096, n_shift=0, first=0) == 0, E.last_error()
    # the mirror
    refs = [(FAKE + i * 4096, 8192) for i in range(9)]
    rs63.encode_dev_rotated_refs(refs, 0, 4096, 1, 5)
    rs63.update_dev_rotated_refs(refs, 0, 4096, 1, 5, [4], [(FAKE + 65536, 4096)])
    rs63.update_dev_rotated_refs(refs, 0, 4096, 1, 5, [4], [(FAKE + 65536, 4096)], store=True)
    # RAID4 (m = 1)
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        p.form_encoding_matrix()
        assert p.kernel == 1
        assert encode(p, shards_of(7), 0, 4096) == 0, E.last_error()
        assert update(p, shards_of(7), 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
    # Cauchy
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert encode(p, shards_of(9), 0, 8 * 64 * 2) == 0, E.last_error()
        assert update(p, shards_of(9), 0, 8 * 64 * 2, ids(5, 2), shards_of(2)) == 0, E.last_error()


def test_refuses_negative_rotation_and_stripes(rs63):
    both_refused("n_shift -1 is negative", rs63, shards_of(9), 0, 4096, n_shift=-1)
    both_refused("first_stripe -1 is negative", rs63, shards_of(9), 0, 4096, first=-1)
    both_refused("nstripes -1 is negative", rs63, shards_of(9), -1, 4096)


def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        both_refused("plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        both_refused("plan kernel 4", p, shards_of(9), 0, 4096)
    with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 5
        both_refused("plan kernel 5", p, shards_of(9), 0, 16 * 64)


def test_refuses_wide_and_parityless_stripes(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        both_refused("m=9", p, shards_of(15), 0, 4096)
        assert "1..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        both_refused("k=65", p, shards_of(68), 0, 4096)
        assert "1..64" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 0, 8, 0, 8) as p:
        both_refused("m=0", p, shards_of(6), 0, 4096)
        assert "1..8" in E.last_error()


def test_refuses_null_pointers(rs63):
    refused(encode, "devs is NULL", rs63, None, 0, 4096)
    refused(update, "devs is NULL", rs63, None, 0, 4096, ids(0), shards_of(1))
    refused(update, "cols is NULL", rs63, shards_of(9), 0, 4096, None, shards_of(1))
    refused(update, "fresh is NULL", rs63, shards_of(9), 0, 4096, ids(0), None)
    # cols may not be NULL with no stripes either, where every base may
    refused(update, "cols is NULL", rs63, shards_of(9, base=0, stride=0), 0, 4096, None, shards_of(1, base=0, stride=0))


def test_refuses_bad_column_lists(rs63):
    sh = shards_of(9)
    refused(update, "cols is empty", rs63, sh, 0, 4096, ids(), shards_of(1))
    refused(update, "cols[1] = -2 is negative", rs63, sh, 0, 4096, ids(0, -2), shards_of(2))
    refused(update, "cols[0] = 6 is not a data chunk", rs63, sh, 0, 4096, ids(6), shards_of(1))  # parity row 0
    assert "0..5" in E.last_error()
    refused(update, "cols[1] = 8 is not a data chunk", rs63, sh, 0, 4096, ids(1, 8), shards_of(2))
    refused(update, "cols[0] = 9 is not a data chunk", rs63, sh, 0, 4096, ids(9), shards_of(1))
    refused(update, "chunk 3 twice", rs63, sh, 0, 4096, ids(3, 1, 3), shards_of(3))
    assert "distinct" in E.last_error()
    refused(update, "more than k=6", rs63, sh, 0, 4096, ids(0, 1, 2, 3, 4, 5, 0), shards_of(7))
    assert "lsec_update_dev_rotated" in E.last_error()  # the messages name the call


def test_refuses_unknown_flags(rs63):
    refused(update, "bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, ids(0), shards_of(1), flags=2)
    refused(update, "bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, ids(0), shards_of(1),
            flags=E.UPDATE_STORE | 4)


def test_refuses_misaligned_refs_on_every_device(rs63):
    """all k+m devices are validated in every call: under n_shift = 1, first_stripe = 5 device 3 holds logical chunk
    (3 + 5) mod 9 = 8 at stripe 0, and with cols = (2,) the changed chunk sits on device 6 -- a misaligned base on a
    device that holds no changed chunk (and, device 0, no parity either) at stripe 0 is refused all the same"""
    for d in range(9):
        sh = shards_of(9)
        sh[d].base = FAKE + d * 4096 + 4
        refused(update, f"device {d}: base", rs63, sh, 0, 4096, ids(2), shards_of(1))
        assert "multiple of 8 bytes" in E.last_error()
        refused(encode, f"{d}: base", rs63, sh, 0, 4096)
        assert "multiple of 8 bytes" in E.last_error()
    refused(update, "fresh 0: base", rs63, shards_of(9), 0, 4096, ids(2), shards_of(1, base=FAKE + 12))
    # strides: only once a second stripe uses them
    for d in (0, 4, 8):
        sh = shards_of(9)
        sh[d].stride = 8196
        assert update(rs63, sh, 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
        assert update(rs63, sh, 1, 4100, ids(2), shards_of(1)) == -1 and "block_size" in E.last_error()  # past the stride rule
        refused(update, f"device {d}: stride 8196", rs63, sh, 2, 4096, ids(2), shards_of(1))
        assert "multiple of 8 bytes" in E.last_error()
        assert encode(rs63, sh, 0, 4096) == 0, E.last_error()
        refused(encode, f"{d}: stride 8196", rs63, sh, 2, 4096)
    fr = shards_of(2)
    fr[1].stride = 4100
    refused(update, "fresh 1: stride 4100", rs63, shards_of(9), 2, 4096, ids(2, 0), fr)


def test_refuses_block_sizes(rs63):
    both_refused("multiple of 8", rs63, shards_of(9), 0, 4100)
    both_refused("multiple of 8", rs63, shards_of(9), 0, -8)
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        both_refused("w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)


def test_update_ladder_order(rs63):
    """the refusals come in lsec_update_dev's order, the two rotation arguments behind the flags"""
    bad = shards_of(9)
    bad[0].base = FAKE + 4
    kw = dict(n_shift=-1, first=-1)
    refused(update, "cols is NULL", rs63, bad, -1, 4100, None, None, flags=8, **kw)
    refused(update, "fresh is NULL", rs63, bad, -1, 4100, ids(0, 0), None, flags=8, **kw)
    refused(update, "chunk 0 twice", rs63, bad, -1, 4100, ids(0, 0), shards_of(2), flags=8, **kw)
    refused(update, "bits other than", rs63, bad, -1, 4100, ids(0), shards_of(1), flags=8, **kw)
    refused(update, "n_shift -1", rs63, bad, -1, 4100, ids(0), shards_of(1), **kw)
    refused(update, "first_stripe -1", rs63, bad, -1, 4100, ids(0), shards_of(1), first=-1)
    refused(update, "device 0: base", rs63, bad, -1, 4100, ids(3), shards_of(1))
    refused(update, "multiple of 8", rs63, shards_of(9), -1, 4100, ids(0), shards_of(1))
    assert "block_size" in E.last_error()


def test_not_a_plan(built):
    fake = C.cast((C.c_char * 512)(), C.POINTER(E.PlanStruct))
    assert L.lib().lsec_encode_dev_rotated(fake, shards_of(9), 0, 4096, 1, 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert L.lib().lsec_update_dev_rotated(fake, shards_of(9), 0, 4096, 1, 0, ids(0), shards_of(1), 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# the codes tests/test_gpu_rotated_write.py runs: (plan kernel, k, m, packet, block_size)
CODES = {"rs63": (1, 6, 3, 0, 8200), "rs128": (1, 12, 8, 0, 8200), "cg63": (2, 6, 3, 8, 64 * 161),
         "cg164": (2, 16, 4, 64, 8 * 64 * 65)}
# the rotated encode takes the rotated check's form for K x R: K fixed at 6 with 2 x 16 B per lane; RS(12+8)'s
# fixed-K form would pass the check's register bound, so K at run time, 2 x 16 B; one dword per lane below
# K = 16, four from there where the packet holds them
ENC_FORMS = {"rs63": (False, 3, 6, 2, 4, 1, 0), "rs128": (False, 8, 0, 2, 4, 1, 0), "cg63": (True, 3, 0, 0, 0, 0, 1),
             "cg164": (True, 4, 0, 0, 0, 0, 4)}
# the rotated update takes the update's: K at run time, two 16-byte units per lane up to four rows and one beyond;
# the update's dwords-per-lane rule
UPD_FORMS = {"rs63": (False, 3, 0, 2, 4, 1, 0), "rs128": (False, 8, 0, 1, 4, 1, 0), "cg63": (True, 3, 0, 0, 0, 0, 1),
             "cg164": (True, 4, 0, 0, 0, 0, 4)}


def test_predicted_forms(built):
    for code, (kernel, k, m, packet, size) in CODES.items():
        enc = E.predict_form("encrot", kernel, k, m, packet, size)
        assert enc == E.Form("encrot", *ENC_FORMS[code]), (code, enc)
        assert enc[1:] == E.predict_form("chkrot", kernel, k, m, packet, size)[1:], code  # the rotated check's shape
        upd = E.predict_form("updrot", kernel, k, m, packet, size)
        assert upd == E.Form("updrot", *UPD_FORMS[code]), (code, upd)
        assert upd[1:] == E.predict_form("upd", kernel, k, m, packet, size)[1:], code  # the unrotated update's
    # every row count has a form; nine rows have none
    for family, number in (("encrot", 8), ("updrot", 9)):
        for m in range(1, 9):
            assert E.predict_form(family, 1, 10, m).R == m and E.predict_form(family, 2, 10, m, 64, 8 * 64).R == m
        for kernel, packet in ((1, 0), (2, 64)):
            out = (C.c_int * 8)()
            assert L.lib().lsec_test_predict_form(number, kernel, 10, 9, packet, 8 * 64, out) == -1
            assert "no kernel" in E.last_error() and "R=9" in E.last_error()
            assert L.lib().lsec_test_predict_form(number, kernel, 65, 3, packet, 8 * 64, out) == -1
    out = (C.c_int * 8)()
    assert L.lib().lsec_test_predict_form(10, 1, 6, 3, 0, 4096, out) == -1  # no tenth family
