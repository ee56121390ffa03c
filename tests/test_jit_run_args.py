"""CPU tests of the hooks that run a compiled network on any matrix (lsec_test_jit_run,
lsec_test_jit_tile; ec_jit.cpp) and of the reference tests/test_gpu_jit_nets.py compares them with
(tests/netref.py): every refusal by its message -- all come before the first HIP call, so no GPU is
needed -- the tile sizes, and the oracle's matrix and bitmatrix products against independent numpy
restatements for every matrix class, so that the reference stands on the CPU alone."""
import ctypes as C

import numpy as np
import pytest

import netref as NR
import oracle as O
from lstore_amd import erasure as E
from test_jit_shapes import SHAPES

RUN = "lsec_test_jit_run"


def hooks():
    lib = E.lib()
    lib.lsec_test_jit_run.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(E.ShardRef), C.POINTER(E.ShardRef), C.c_int,
                                                      C.c_longlong, C.c_void_p]
    lib.lsec_test_jit_run.restype = C.c_int
    lib.lsec_test_jit_tile.argtypes = [C.c_int] * 5
    lib.lsec_test_jit_tile.restype = C.c_int
    return lib


def refs(n, base=0x10000, stride=0x1000):
    arr = (E.ShardRef * n)()
    for i in range(n):
        arr[i].base, arr[i].stride = base + i * 0x100000, stride
    return arr


def refused(shape, R, K, w, packet, mat="ok", inp="ok", out="ok", nstripes=1, size=None):
    """one call that must be refused: the message"""
    lib = hooks()
    m = np.ones(max(1, R * K * (w if shape == 2 else 1)), np.uint32) if isinstance(mat, str) else mat
    if size is None:
        size = 8 if shape < 2 else w * packet
    rc = lib.lsec_test_jit_run(shape, R, K, w, packet, None if mat is None else m.ctypes.data,
                               None if inp is None else (refs(max(K, 1)) if isinstance(inp, str) else inp),
                               None if out is None else (refs(max(R, 1)) if isinstance(out, str) else out), nstripes, size, None)
    assert rc == -1
    msg = E.last_error()
    assert msg.startswith(RUN + ":"), msg
    return msg


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("args,limit", [
    ((-1, 4, 6, 8, 0), "shape -1: 0 .. 3"),
    ((4, 4, 6, 8, 0), "shape 4: 0 .. 3"),
    ((0, 0, 6, 8, 0), "R 0: 1 .. 8 rows"),
    ((1, 9, 6, 16, 0), "R 9: 1 .. 8 rows"),
    ((0, 4, 0, 8, 0), "K 0: 1 .. 32 inputs"),
    ((2, 2, 33, 7, 32), "K 33: 1 .. 32 inputs"),
    ((0, 4, 6, 16, 0), "w 16: shape 0 takes 8"),
    ((1, 4, 6, 8, 0), "w 8: shape 1 takes 16 or 32"),
    ((1, 4, 6, 24, 0), "w 24: shape 1 takes 16 or 32"),
    ((2, 2, 6, 1, 32), "w 1: shape 2 takes 2 .. 32"),
    ((2, 2, 6, 33, 32), "w 33: shape 2 takes 2 .. 32"),
    ((3, 2, 6, 7, 32), "w 7: shape 3 takes 8, 16 or 32"),
    ((2, 2, 6, 7, 0), "packet 0: 4 .. 1048576 bytes"),
    ((3, 4, 5, 32, -8), "packet -8: 4 .. 1048576 bytes"),
    ((2, 2, 6, 7, 1 << 21), "packet 2097152: 4 .. 1048576 bytes"),
    ((2, 2, 6, 7, 6), "packet 6: no lane width (pkt_shape: a multiple of 4 bytes)"),
    ((3, 4, 6, 16, 30), "packet 30: no lane width (pkt_shape: a multiple of 4 bytes)"),
])
def test_shape_limits(built, args, limit):
    assert limit in refused(*args)
    # the same checks, and the same words, behind lsec_test_jit_tile
    assert hooks().lsec_test_jit_tile(*args) == -1
    assert E.last_error() == "lsec_test_jit_tile: " + limit, E.last_error()


def test_null_pointers(built):
    assert "NULL mat" in refused(0, 4, 6, 8, 0, mat=None)
    assert "NULL in" in refused(1, 4, 6, 16, 0, inp=None)
    assert "NULL out" in refused(2, 2, 6, 7, 32, out=None)


def test_negative_nstripes(built):
    assert "nstripes -1: negative" in refused(0, 4, 6, 8, 0, nstripes=-1)
    assert "nstripes -3: negative" in refused(3, 4, 5, 32, 64, nstripes=-3)


@pytest.mark.parametrize("shape,w,packet", [(0, 8, 0), (1, 16, 0), (3, 8, 32), (3, 16, 32)])
def test_coefficient_above_the_field(built, shape, w, packet):
    R, K = 4, 6
    m = np.ones(R * K, np.uint32)
    m[7] = 1 << w
    assert f"coefficient 7 is {1 << w}: above {(1 << w) - 1} at w = {w}" in refused(shape, R, K, w, packet, mat=m)
    m[7] = 0xFFFFFFFF
    assert f"coefficient 7 is {0xFFFFFFFF}" in refused(shape, R, K, w, packet, mat=m)


def test_masks_are_not_coefficients(built):
    """shape 2's words are row masks: bits above w are not a coefficient's, and the refusal that
    follows is the next check's (here the size), not the coefficient bound"""
    m = np.full(2 * 7 * 6, 0xFFFFFFFF, np.uint32)
    assert "size 100" in refused(2, 2, 6, 7, 32, mat=m, size=100)


@pytest.mark.parametrize("shape,w,packet,size,unit", [
    (0, 8, 0, 12, 8), (0, 8, 0, -8, 8), (1, 32, 0, 32772, 8), (1, 16, 0, 4, 8),
    (2, 7, 32, 7 * 32 + 8, 7 * 32), (2, 7, 32, 32, 7 * 32), (3, 32, 64, 1024, 32 * 64), (3, 16, 32, -512, 16 * 32),
])
def test_size_not_a_multiple(built, shape, w, packet, size, unit):
    R = 2 if shape == 2 else 4
    msg = refused(shape, R, 6, w, packet, size=size)
    assert f"size {size}: not a multiple of {unit} bytes" in msg
    assert ("(w * packet)" if shape >= 2 else "(8)") in msg


@pytest.mark.parametrize("which", ["in base", "in stride", "out base", "out stride"])
def test_packet_alignment(built, which):
    """(2, 6, 7, 32) has 16-byte lanes (pkt_shape: 2 * 7 * 4 <= 64): one base or stride at 8 mod 16
    fails pkt_aligned; with one stripe the stride still counts, as in pkt_aligned itself"""
    R, K, w, packet = 2, 6, 7, 32
    assert hooks().lsec_test_jit_tile(2, R, K, w, packet) == 4096
    inp, out = refs(K), refs(R)
    arr, field = (inp if which.startswith("in") else out), which.split()[1]
    setattr(arr[len(arr) - 1], field, getattr(arr[len(arr) - 1], field) + 8)
    msg = refused(2, R, K, w, packet, inp=inp, out=out, nstripes=2)
    assert "not a multiple of the lane width, 16 bytes (pkt_aligned)" in msg
    # 4-byte lanes (4 rows at w = 32) take the same shards
    inp4 = refs(5)
    inp4[4].base += 8
    lib = hooks()
    m = np.ones(4 * 5, np.uint32)
    # ... up to the next refusal: here the size
    rc = lib.lsec_test_jit_run(3, 4, 5, 32, 64, m.ctypes.data, inp4, refs(4), 1, 100, None)
    assert rc == -1 and "size 100" in E.last_error()


# ------------------------------------------------------------------ tile sizes
# 256 lanes x bytes per lane and piece; the wave-pair split covers 128 lane columns.  (1, 3, 6, 32):
# the 32 KiB that tests/test_gpu_layouts.py's docstring states for the three-row network, and the
# transposed kernels' 256 x 4 x w = 16 KiB / 32 KiB it states are the one-wave tiles here.
TILES = {
    (0, 6, 20, 8, 0): 256 * 16,        # 16 B lanes, one piece (K * 8 > 104)
    (0, 8, 12, 8, 0): 256 * 8,         # 8 B lanes
    (0, 8, 32, 8, 0): 256 * 16,
    (1, 3, 6, 32, 0): 256 * 4 * 32,    # one wave: 32 KiB
    (1, 4, 10, 32, 0): 128 * 4 * 32,   # split
    (1, 6, 10, 32, 0): 128 * 4 * 32,
    (1, 4, 10, 16, 0): 256 * 4 * 16,   # one wave: 16 KiB
    (1, 6, 20, 16, 0): 128 * 4 * 16,   # split at w = 16
    (2, 2, 6, 7, 32): 256 * 16,        # column bytes: 16 B lanes
    (2, 2, 16, 16, 32): 256 * 8,       # 8 B by the register cap
    (2, 2, 8, 8, 40): 256 * 8,         # 8 B by the packet
    (3, 4, 10, 32, 64): 256 * 4,       # 4 B lanes
    (3, 4, 10, 16, 32): 256 * 4,
}


def test_tiles_of_the_compile_shapes(built):
    assert set(TILES) == set(SHAPES)
    lib = hooks()
    for s in SHAPES:
        assert lib.lsec_test_jit_tile(*s) == TILES[s], s
    # two pieces of 16 B per lane while K * 8 <= 104: the 8 KiB bytewise tile
    assert lib.lsec_test_jit_tile(0, 6, 13, 8, 0) == 256 * 32
    assert lib.lsec_test_jit_tile(0, 6, 14, 8, 0) == 256 * 16


# ------------------------------------------------------------------ the reference, on the CPU
@pytest.mark.parametrize("cls", NR.CLASSES)
@pytest.mark.parametrize("w", [8, 16, 32])
def test_expected_is_the_gf_product(built, cls, w):
    R, K, size = 4, 6, 104
    shape = 0 if w == 8 else 1
    M = NR.matrix(cls, shape, R, K, w)
    data = NR.stripes(shape, R, K, w, size)
    want = NR.expected(shape, R, K, w, 0, M, data)
    for s in range(NR.NSTRIPES):
        assert np.array_equal(want[s], NR.gf_product(M, data[s], w)), (cls, w, s)
    # the classes are what they say
    zero_cols = [j for j in range(K) if not M[:, j].any()]
    zero_rows = [r for r in range(R) if not M[r].any()]
    assert (zero_cols, zero_rows) == {"dense": ([], []), "edges": ([], []), "holes_odd": ([1], [1]),
                                      "holes_even": ([0, K - 2], [R - 1])}.get(cls, (zero_cols, []))
    if cls == "single":
        assert len(zero_cols) == K - 1 and M.any(axis=1).all()
    if cls == "edges":
        assert (M[0] == 1).all() and (M[1] < 16).all() and M[1].all()
        assert set(M[2:].flatten().tolist()) <= {1, 2, 1 << (w - 1), (1 << w) - 1}


def test_gf_product_known_answers():
    """x * x^(w-1) wraps by the polynomial; the all-ones element times itself"""
    for w, poly in NR.POLY.items():
        data = np.zeros((1, 8), np.uint8)
        data[0, w // 8 - 1] = 0x80  # the element x^(w-1), little-endian
        got = NR.gf_product(np.array([[2]]), data, w)[0]
        assert int.from_bytes(got[:w // 8].tobytes(), "little") == poly & ((1 << w) - 1)
        assert not got[w // 8:].any()


@pytest.mark.parametrize("cls", NR.CLASSES)
@pytest.mark.parametrize("R,K,w,packet", [(2, 6, 7, 8), (2, 5, 16, 4), (3, 4, 32, 4)])
def test_expected_masks_are_the_packet_xor(built, cls, R, K, w, packet):
    M = NR.matrix(cls, 2, R, K, w)
    assert M.shape == (R * w, K) and int(M.max()) >> w == 0
    data = NR.stripes(2, R, K, w, 3 * w * packet)
    want = NR.expected(2, R, K, w, packet, M, data)
    for s in range(NR.NSTRIPES):
        assert np.array_equal(want[s], NR.packet_xor(M, data[s], w, packet)), (cls, s)
    if cls == "holes_odd":
        assert not M[:, 1].any() and not M[1].any() and not want[:, 0].reshape(3, 3, w, packet)[:, :, 1].any()
    if cls == "holes_even":
        assert not M[:, 0].any() and not M[:, K - 2].any() and not want[:, R - 1].any()
    if cls == "edges":
        assert int(M[:, 2].max()) == 1  # input 2: packet 0 alone is read
        plain = np.bitwise_xor.reduce(np.delete(data[0], 2, axis=0), axis=0).reshape(3, w, packet)
        plain[:, 0] ^= data[0, 2].reshape(3, w, packet)[:, 0]
        assert np.array_equal(want[0, 0], plain.reshape(-1))  # output 0: identity blocks
    if cls == "single":
        assert np.count_nonzero(M.any(axis=0)) == 1 and M.any(axis=1).all()


@pytest.mark.parametrize("cls", NR.CLASSES)
@pytest.mark.parametrize("w", [8, 16, 32])
def test_expected_coefficient_packets(built, cls, w):
    """shape 3: the oracle's bitmatrix of the coefficients against the numpy coef_masks, and the
    packet product against the plain packet XOR"""
    R, K, packet = 3, 4, 4
    M = NR.matrix(cls, 3, R, K, w)
    masks = NR.coef_masks(M, w)
    assert np.array_equal(O.bitmatrix(M.view(np.int32), w), NR.mask_bits(masks, R, K, w))
    data = NR.stripes(3, R, K, w, 2 * w * packet)
    want = NR.expected(3, R, K, w, packet, M, data)
    for s in range(NR.NSTRIPES):
        assert np.array_equal(want[s], NR.packet_xor(masks, data[s], w, packet)), (cls, s)


@pytest.mark.parametrize("k,m,w", [(6, 3, 8), (20, 6, 8), (6, 3, 16), (6, 4, 32)])
def test_expected_of_a_stock_matrix_is_the_oracle_encode(built, k, m, w):
    M = O.coding_matrix(O.REED_SOL_VAN, k, m, w)
    shape = 0 if w == 8 else 1
    data = NR.stripes(shape, m, k, w, 136)
    want = NR.expected(shape, m, k, w, 0, M.astype(np.uint32), data)
    for s in range(NR.NSTRIPES):
        assert np.array_equal(want[s], O.encode(O.REED_SOL_VAN, data[s], m, 0, w))


def test_stripes_are_as_stated():
    d = NR.stripes(1, 4, 6, 32, 64)
    assert d.shape == (3, 6, 64) and (d[1] == 0xFF).all()
    assert d[2, 5, 63] == 0x80 and np.count_nonzero(d[2]) == 1
    assert np.array_equal(d, NR.stripes(1, 4, 6, 32, 64)) and len(np.unique(d[0])) > 64
