"""The refusals of lsec_check_dev, lsec_locate_dev and their _rotated forms, word for word and in
order, checked without a GPU.  Every case here fails in the validation ladder, before any device
could be touched; the pointers handed in are fixed fake addresses that are never dereferenced.
Each message is compared as a whole, and the cases with two faults at once pin which check comes
first, so the ladder the four calls share cannot move a rung or reword one unnoticed.
"""
import ctypes as C

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # a multiple of 8: only its alignment is looked at
CALLS = ("lsec_check_dev", "lsec_locate_dev", "lsec_check_dev_rotated", "lsec_locate_dev_rotated")
CHECKS = tuple(c for c in CALLS if "check" in c)
LOCATES = tuple(c for c in CALLS if "locate" in c)
ROTATED = tuple(c for c in CALLS if c.endswith("_rotated"))

KERNELS = "%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s is plan kernel %d"
K_RANGE = {c: "%s: k=65 outside 1..64 (one launch's inputs%s)" % (c, ", one bit of hyp each" if c in LOCATES else "")
           for c in CALLS}
M_RANGE = {c: "%s: m=%%d outside " % c + ("2..8 (one parity row cannot locate; one launch's parity rows)" if c in LOCATES
                                        else "1..8 (one launch's parity rows)") for c in CALLS}
FLAGS = "%s: flags 0x6 has bits other than LSEC_LOCATE_REPAIR"
ZERO = ("lsec_locate_dev: coding matrix coefficient [1][2] is zero: a data chunk that leaves a parity row "
        "untouched cannot be told from that row's own corruption")  # the ratio image's one message, either locate


def misaligned(what, addr, unit):
    return "%s 0x%x is not a multiple of %d bytes" % (what, addr, unit)


def shards_of(n):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = FAKE + i * 4096, 8192
    return sh


def run(name, p, nstripes=0, size=4096, n_shift=1, first=5, syndrome=None, bad_count=None, hyp=None, located=None,
        located_dev=None, counts=None, dev_faults=None, flags=0):
    """One of the four calls over the plan's k+m shards; arguments a call does not take are dropped."""
    sh = shards_of(p.k + p.m)
    rot = (n_shift, first) if name in ROTATED else ()
    if name in CHECKS:
        args = (syndrome, bad_count)
    elif name in ROTATED:
        args = (syndrome, hyp, located, located_dev, counts, dev_faults, flags)
    else:
        args = (syndrome, hyp, located, counts, flags)
    return getattr(L.lib(), name)(p.ptr, sh, nstripes, size, *rot, *args, None)


def says(name, text, p, **kw):
    assert run(name, p, **kw) == -1, (name, text)
    assert E.last_error() == text, (name, kw)


@pytest.fixture(scope="module")
def plans(built):
    made = dict(
        rs63=L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096),
        liberation=L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8),   # plan kernel 3
        rs_w16=L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8),          # plan kernel 4
        k65=L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8),
        k65m9=L.Plan.new(L.REED_SOL_VAN, 4096, 65, 9, 8, 0, 8),
        m9=L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8),
        m1=L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1),
        cauchy=L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8),     # plan kernel 2, w * packet = 512
        zero=L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 8, 0, 8),
    )
    made["liberation"].form_encoding_matrix()
    made["cauchy"].form_encoding_matrix()
    # a caller's own coding matrix (the plan struct's public field, freed with the plan): all ones but one zero
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    mat = C.cast(libc.malloc(C.sizeof(C.c_int) * 18), C.POINTER(C.c_int))
    for i in range(18):
        mat[i] = 0 if i == 1 * 6 + 2 else 1 + i
    made["zero"].s.encode_matrix = mat
    assert (made["liberation"].kernel, made["rs_w16"].kernel, made["cauchy"].kernel, made["zero"].kernel) == (3, 4, 2, 1)
    yield made
    for p in made.values():
        p.close()


@pytest.mark.parametrize("name", CALLS)
def test_every_refusal(plans, name):
    rs63 = plans["rs63"]
    loc = name in LOCATES
    says(name, KERNELS % (name, "liberation (w=7)", 3), plans["liberation"], size=7 * 32 * 4)
    says(name, KERNELS % (name, "reed_sol_van (w=16)", 4), plans["rs_w16"])
    says(name, K_RANGE[name], plans["k65"])
    says(name, M_RANGE[name] % 9, plans["m9"])
    if loc:
        says(name, M_RANGE[name] % 1, plans["m1"])
        says(name, FLAGS % name, rs63, flags=6)
    says(name, "nstripes -1 is negative", rs63, nstripes=-1)
    if name in ROTATED:
        says(name, "n_shift -1 is negative", rs63, n_shift=-1)
        says(name, "first_stripe -1 is negative", rs63, first=-1)
    says(name, "block_size 12 is not a multiple of 8", rs63, size=12)
    says(name, "block_size 1088 is not a multiple of w*packet_size = 512", plans["cauchy"], size=8 * 64 * 2 + 64)
    says(name, "syndrome is NULL", rs63, nstripes=1, hyp=FAKE, located=FAKE)
    if loc:
        says(name, "hyp is NULL", rs63, nstripes=1, syndrome=FAKE, located=FAKE)
        says(name, "located is NULL", rs63, nstripes=1, syndrome=FAKE, hyp=FAKE)
    says(name, misaligned("syndrome", FAKE + 2, 4), rs63, syndrome=FAKE + 2)
    if loc:
        says(name, misaligned("hyp", FAKE + 4, 8), rs63, syndrome=FAKE, hyp=FAKE + 4)
        says(name, misaligned("counts", FAKE + 6, 4), rs63, syndrome=FAKE, hyp=FAKE, located=FAKE + 1, counts=FAKE + 6)
        if name in ROTATED:
            says(name, misaligned("dev_faults", FAKE + 2, 4), rs63, syndrome=FAKE, hyp=FAKE, located=FAKE + 1,
                 located_dev=FAKE + 3, counts=FAKE + 8, dev_faults=FAKE + 2)
        says(name, ZERO, plans["zero"])
        says(name, ZERO, plans["zero"], nstripes=1, syndrome=FAKE, hyp=FAKE, located=FAKE + 1)  # before any device is touched
    else:
        says(name, misaligned("bad_count", FAKE + 2, 4), rs63, syndrome=FAKE, bad_count=FAKE + 2)


@pytest.mark.parametrize("name", CALLS)
def test_which_refusal_wins(plans, name):
    """two faults at once: the earlier rung of the ladder answers"""
    rs63 = plans["rs63"]
    loc = name in LOCATES
    says(name, KERNELS % (name, "reed_sol_van (w=16)", 4), plans["rs_w16"], nstripes=-1)     # kernel < nstripes
    says(name, K_RANGE[name], plans["k65m9"])                                                # k < m
    says(name, M_RANGE[name] % 9, plans["m9"], nstripes=-1, flags=6)                         # m < flags, nstripes
    says(name, "nstripes -1 is negative", rs63, nstripes=-1, n_shift=-1, size=12)            # nstripes < n_shift, block_size
    says(name, "block_size 12 is not a multiple of 8", rs63, nstripes=1, size=12)            # block_size < NULL syndrome
    says(name, "syndrome is NULL", rs63, nstripes=1, hyp=FAKE + 4, bad_count=FAKE + 2)       # NULL < any alignment
    if loc:
        says(name, M_RANGE[name] % 1, plans["m1"], flags=6)                                  # m < flags
        says(name, FLAGS % name, rs63, flags=6, nstripes=-1)                                 # flags < nstripes
        says(name, "hyp is NULL", rs63, nstripes=1, syndrome=FAKE + 2)                       # hyp NULL < located NULL, alignment
        says(name, "located is NULL", rs63, nstripes=1, syndrome=FAKE + 2, hyp=FAKE)         # every NULL < any alignment
        says(name, misaligned("syndrome", FAKE + 2, 4), rs63, syndrome=FAKE + 2, hyp=FAKE + 4)
        says(name, misaligned("hyp", FAKE + 4, 8), rs63, hyp=FAKE + 4, counts=FAKE + 6)
        says(name, misaligned("counts", FAKE + 6, 4), plans["zero"], counts=FAKE + 6, dev_faults=FAKE + 2)  # < dev_faults, matrix
    else:
        says(name, misaligned("syndrome", FAKE + 2, 4), rs63, syndrome=FAKE + 2, bad_count=FAKE + 2)
    if name in ROTATED:
        says(name, "n_shift -1 is negative", rs63, n_shift=-1, first=-1)                     # n_shift < first_stripe
        says(name, "n_shift -1 is negative", rs63, n_shift=-1, size=12)                      # n_shift < block_size
        says(name, "first_stripe -1 is negative", rs63, first=-1, size=12)                   # first_stripe < block_size
    if name == "lsec_locate_dev_rotated":
        says(name, misaligned("dev_faults", FAKE + 2, 4), plans["zero"], dev_faults=FAKE + 2)  # dev_faults < matrix
