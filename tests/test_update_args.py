"""Host side of lsec_update_dev (the parity update for partial-stripe writes): the symbol, the header,
the Python mirror, the argument validation and the form prediction, checked without a GPU.
nstripes == 0 validates everything and touches no GPU, so every refusal here is reached before
anything could be enqueued; the pointers handed in are never dereferenced.  The stride rule only
applies once a second stripe uses the stride, so it is checked at nstripes == 2: the ladder refuses
before it reaches a device.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # an address that is a multiple of 8: only its alignment is looked at
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shards_of(n, base=FAKE, stride=8192):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = (base + i * 4096 if base else 0), stride
    return sh


def ids(*cols):
    return (C.c_int * (len(cols) + 1))(*cols, -1)


def update(p, sh, nstripes, size, cols, fresh, flags=0):
    return L.lib().lsec_update_dev(p.ptr, sh, nstripes, size, cols, fresh, flags, None)


def refused(words, *args, **kw):
    assert update(*args, **kw) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbol_header_mirror_and_abi_version(built):
    lib = L.lib()
    assert "lsec_update_dev" in E.EXPORTS and hasattr(lib, "lsec_update_dev")
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the call by its symbol
    with open(os.path.join(ROOT, "include", "lstore_ec.h")) as f:
        header = f.read()
    assert re.search(r"^int\s+lsec_update_dev\s*\(", header, re.M)
    assert re.search(r"^#define\s+LSEC_UPDATE_STORE\s+1\b", header, re.M) and E.UPDATE_STORE == 1
    for name in ("update_dev_refs", "update_dev"):
        assert callable(getattr(L.Plan, name))


def test_accepted_with_no_stripes(rs63, built):
    assert update(rs63, shards_of(9), 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
    assert update(rs63, shards_of(9), 0, 4096, ids(2), shards_of(1), E.UPDATE_STORE) == 0, E.last_error()
    # NULL bases everywhere (the prepare-ahead convention of the *_dev calls)
    assert update(rs63, shards_of(9, base=0, stride=0), 0, 4096, ids(0, 1), shards_of(2, base=0, stride=0)) == 0, E.last_error()
    # an untouched data entry is ignored entirely: (0, 0), or a base and a stride no call would take
    sh = shards_of(9)
    sh[0].base, sh[0].stride = 0, 0
    sh[3].base, sh[3].stride = FAKE + 3, 4097
    assert update(rs63, sh, 0, 4096, ids(1, 5), shards_of(2)) == 0, E.last_error()
    # c = k, and a descending list
    assert update(rs63, shards_of(9), 0, 4096, ids(0, 1, 2, 3, 4, 5), shards_of(6)) == 0, E.last_error()
    assert update(rs63, shards_of(9), 0, 4096, ids(5, 3, 0), shards_of(3)) == 0, E.last_error()
    # the mirror: (0, 0) for the untouched chunks
    refs = [(0, 0)] * 9
    for i in (4, 6, 7, 8):
        refs[i] = (FAKE + i * 4096, 8192)
    rs63.update_dev_refs(refs, 0, 4096, [4], [(FAKE + 65536, 4096)])
    rs63.update_dev_refs(refs, 0, 4096, [4], [(FAKE + 65536, 4096)], store=True)
    # RAID4 (m = 1)
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        p.form_encoding_matrix()
        assert p.kernel == 1
        assert update(p, shards_of(7), 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
    # Cauchy
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert update(p, shards_of(9), 0, 8 * 64 * 2, ids(5, 2), shards_of(2)) == 0, E.last_error()


def test_untouched_entries_are_not_validated_with_two_stripes(rs63):
    """a misaligned base and stride in an untouched entry pass the ladder at nstripes == 2 as well: the refusal
    that ends this call (so that it never reaches a device) names the fresh chunk behind it, not that entry"""
    sh = shards_of(9)
    sh[3].base, sh[3].stride = FAKE + 3, 4097
    refused("fresh 0: stride 8196", rs63, sh, 2, 4096, ids(1), shards_of(1, stride=8196))


def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        refused("plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4, ids(0), shards_of(1))
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        refused("plan kernel 4", p, shards_of(9), 0, 4096, ids(0), shards_of(1))
    with L.Plan.new(L.CAUCHY_GOOD, 16 * 64, 6, 3, 16, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 5
        refused("plan kernel 5", p, shards_of(9), 0, 16 * 64, ids(0), shards_of(1))


def test_refuses_wide_stripes(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused("m=9", p, shards_of(15), 0, 4096, ids(0), shards_of(1))
        assert "1..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        refused("k=65", p, shards_of(68), 0, 4096, ids(0), shards_of(1))
        assert "1..64" in E.last_error()


def test_refuses_null_pointers(rs63):
    refused("shards is NULL", rs63, None, 0, 4096, ids(0), shards_of(1))
    refused("cols is NULL", rs63, shards_of(9), 0, 4096, None, shards_of(1))
    refused("fresh is NULL", rs63, shards_of(9), 0, 4096, ids(0), None)


def test_refuses_bad_column_lists(rs63):
    refused("cols is empty", rs63, shards_of(9), 0, 4096, ids(), shards_of(1))
    refused("cols[1] = -2 is negative", rs63, shards_of(9), 0, 4096, ids(0, -2), shards_of(2))
    refused("cols[0] = 6 is not a data chunk", rs63, shards_of(9), 0, 4096, ids(6), shards_of(1))  # parity row 0
    assert "0..5" in E.last_error()
    refused("cols[1] = 8 is not a data chunk", rs63, shards_of(9), 0, 4096, ids(1, 8), shards_of(2))
    refused("cols[0] = 9 is not a data chunk", rs63, shards_of(9), 0, 4096, ids(9), shards_of(1))
    refused("chunk 3 twice", rs63, shards_of(9), 0, 4096, ids(3, 1, 3), shards_of(3))
    assert "distinct" in E.last_error()
    refused("more than k=6", rs63, shards_of(9), 0, 4096, ids(0, 1, 2, 3, 4, 5, 0), shards_of(7))


def test_refuses_unknown_flags(rs63):
    refused("bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, ids(0), shards_of(1), flags=2)
    refused("bits other than LSEC_UPDATE_STORE", rs63, shards_of(9), 0, 4096, ids(0), shards_of(1), flags=E.UPDATE_STORE | 4)


def test_refuses_misaligned_refs(rs63):
    sh = shards_of(9)
    sh[2].base = FAKE + 4
    refused("shard 2: base", rs63, sh, 0, 4096, ids(2), shards_of(1))  # a changed chunk
    assert "multiple of 8 bytes" in E.last_error()
    sh = shards_of(9)
    sh[7].base = FAKE + 4
    refused("shard 7: base", rs63, sh, 0, 4096, ids(2), shards_of(1))  # a parity chunk
    refused("fresh 0: base", rs63, shards_of(9), 0, 4096, ids(2), shards_of(1, base=FAKE + 12))
    assert "multiple of 8 bytes" in E.last_error()
    # strides: only once a second stripe uses them
    sh = shards_of(9)
    sh[2].stride = 8196
    assert update(rs63, sh, 0, 4096, ids(2), shards_of(1)) == 0, E.last_error()
    refused("shard 2: stride 8196", rs63, sh, 2, 4096, ids(2), shards_of(1))
    assert "multiple of 8 bytes" in E.last_error()
    sh = shards_of(9)
    sh[8].stride = 8196
    refused("shard 8: stride 8196", rs63, sh, 2, 4096, ids(2), shards_of(1))
    fr = shards_of(2)
    fr[1].stride = 4100
    refused("fresh 1: stride 4100", rs63, shards_of(9), 2, 4096, ids(2, 0), fr)


def test_refuses_block_sizes_and_negative_stripes(rs63):
    refused("multiple of 8", rs63, shards_of(9), 0, 4100, ids(0), shards_of(1))
    refused("multiple of 8", rs63, shards_of(9), 0, -8, ids(0), shards_of(1))
    refused("nstripes -1 is negative", rs63, shards_of(9), -1, 4096, ids(0), shards_of(1))
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        refused("w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64, ids(0), shards_of(1))


def test_ladder_order(rs63):
    """the refusals come in the order the header lists them"""
    bad = shards_of(9)
    bad[0].base = FAKE + 4
    refused("cols is NULL", rs63, bad, -1, 4100, None, None, flags=8)
    refused("fresh is NULL", rs63, bad, -1, 4100, ids(0, 0), None, flags=8)
    refused("chunk 0 twice", rs63, bad, -1, 4100, ids(0, 0), shards_of(2), flags=8)
    refused("bits other than", rs63, bad, -1, 4100, ids(0), shards_of(1), flags=8)
    refused("shard 0: base", rs63, bad, -1, 4100, ids(0), shards_of(1))
    refused("multiple of 8", rs63, shards_of(9), -1, 4100, ids(0), shards_of(1))
    assert "block_size" in E.last_error()


def test_not_a_plan(built):
    fake = (C.c_char * 512)()
    assert L.lib().lsec_update_dev(C.cast(fake, C.POINTER(E.PlanStruct)), shards_of(9), 0, 4096, ids(0), shards_of(1), 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# the shapes tests/test_gpu_update.py runs: (plan kernel, k, m, packet, block_size) -> (IT, VW, BF) or DW
BYTEWISE_FORMS = {(6, 3): (2, 4, 1), (16, 4): (2, 4, 1), (6, 1): (1, 2, 0), (6, 2): (2, 4, 1), (12, 8): (1, 4, 1),
                  (5, 2): (2, 4, 1), (64, 2): (2, 4, 1)}
SLICED_FORMS = {(6, 3, 8, 64): 1, (6, 3, 8, 64 * 161): 1, (6, 3, 512, 8 * 512 * 3): 1, (4, 2, 8, 64): 1,
                (16, 4, 8, 64): 2, (16, 4, 8, 64 * 161): 2, (16, 4, 512, 8 * 512 * 3): 4, (16, 4, 64, 8 * 64 * 65): 4}


def test_predicted_forms(built):
    for (k, m), (it, vw, bf) in BYTEWISE_FORMS.items():
        f = E.predict_form("upd", 1, k, m, 0, 8192)
        assert f == E.Form("upd", False, m, 0, it, vw, bf, 0), (k, m, f)
    for (k, m, packet, size), dw in SLICED_FORMS.items():
        f = E.predict_form("upd", 2, k, m, packet, size)
        assert f == E.Form("upd", True, m, 0, 0, 0, 0, dw), (k, m, packet, size, f)
    # every row count has a form; nine rows have none
    for m in range(1, 9):
        assert E.predict_form("upd", 1, 10, m).R == m and E.predict_form("upd", 2, 10, m, 64, 8 * 64).R == m
    for kernel, packet in ((1, 0), (2, 64)):
        out = (C.c_int * 8)()
        assert L.lib().lsec_test_predict_form(7, kernel, 10, 9, packet, 8 * 64, out) == -1
        assert "R=9" in E.last_error()
        assert L.lib().lsec_test_predict_form(7, kernel, 65, 3, packet, 8 * 64, out) == -1
