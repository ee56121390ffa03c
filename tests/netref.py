"""Matrices, data and reference bytes for running the compiled networks on arbitrary matrices
(lsec_test_jit_run; tests/test_jit_run_args.py and tests/test_gpu_jit_nets.py).

The networks' source depends on the matrix (ec_netgen.cpp): which inputs are read at all, which
accumulator slices are ever written, where a row's top coefficient bit lies.  The matrices of stock
plans are MDS -- no zero coefficient anywhere -- so the classes here hold what those never do.

Shapes are those of lsec_test_jit_compile: 0 = w = 8 XOR network and 1 = w = 16 / 32 network over
R x K coefficients, 2 = packet network over R*w x K row masks (bit x of mask [r*w + l][j]: output
packet l of row r takes packet x of input j), 3 = packet network over R x K coefficients.

``expected`` is the oracle restatement's (oracle/ec_oracle.c, pinned to the reference fixtures by
tests/test_oracle.py); ``gf_product`` and ``packet_xor`` restate the two operations in numpy,
independently of it.  Only numpy and the oracle here.
"""
import ctypes as C
import zlib

import numpy as np

import oracle as O

CLASSES = ("dense", "holes_odd", "holes_even", "edges", "single")
POLY = {8: 0x11D, 16: 0x1100B, 32: 0x100400007}  # Jerasure's primitive polynomials
NSTRIPES = 3


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _coefficients(cls, rng, R, K, w):
    """R x K GF(2^w) coefficients of a class"""
    top = (1 << w) - 1
    M = rng.integers(1, top, (R, K), dtype=np.uint64, endpoint=True)  # dense: non-zero, full width
    if cls == "holes_odd":  # an odd count of used inputs where K is even; a zero row
        M[:, 1] = 0
        M[1, :] = 0
    elif cls == "holes_even":  # gaps in `used` on both sides; the last row zero
        M[:, 0] = 0
        M[:, K - 2] = 0
        M[R - 1, :] = 0
    elif cls == "edges":
        M = rng.choice(np.array([1, 2, 1 << (w - 1), top], dtype=np.uint64), (R, K))
        M[0, :] = 1
        M[1, :] = rng.integers(1, 16, K, dtype=np.uint64)  # a low top bit
    elif cls == "single":
        col = int(rng.integers(0, K))
        keep = M[:, col].copy()
        M[:, :] = 0
        M[:, col] = keep
    elif cls != "dense":
        raise ValueError(cls)
    return M.astype(np.uint32)


def _masks(cls, rng, R, K, w):
    """R*w x K row masks of a class: the counterparts for a packet network"""
    top = (1 << w) - 1

    def sparse(shape):
        return rng.integers(0, top, shape, dtype=np.uint64, endpoint=True) & rng.integers(0, top, shape, dtype=np.uint64,
                                                                                         endpoint=True)

    M = sparse((R * w, K))
    if cls == "holes_odd":  # an input no row uses; an output packet with no bit set
        M[:, 1] = 0
        M[1, :] = 0
    elif cls == "holes_even":  # unused inputs on both sides; every packet of the last output empty
        M[:, 0] = 0
        M[:, K - 2] = 0
        M[(R - 1) * w:, :] = 0
    elif cls == "edges":
        for l in range(w):  # output 0: identity blocks, the plain XOR of the inputs
            M[l, :] = 1 << l
        M[:, 2] &= 1  # an input of which only packet 0 is read
        M[w, 2] = 1
    elif cls == "single":
        col = int(rng.integers(0, K))
        keep = M[:, col] | (1 << (np.arange(R * w, dtype=np.uint64) % np.uint64(w)))  # no empty row
        M[:, :] = 0
        M[:, col] = keep
    elif cls != "dense":
        raise ValueError(cls)
    return M.astype(np.uint32)


def matrix(cls, shape, R, K, w):
    """the matrix of a class as lsec_test_jit_run takes it (uint32, C order): R x K coefficients, or
    for shape 2 R*w x K row masks; seeded by (class, shape, R, K, w)"""
    rng = _rng(cls, shape, R, K, w)
    return np.ascontiguousarray(_masks(cls, rng, R, K, w) if shape == 2 else _coefficients(cls, rng, R, K, w))


def stripes(shape, R, K, w, size):
    """uint8 [3, K, size]: stripe 0 seeded random, stripe 1 all 0xFF, stripe 2 zero but for 0x80 in
    the last byte of the last input"""
    d = np.empty((NSTRIPES, K, size), np.uint8)
    d[0] = _rng("data", shape, R, K, w, size).integers(0, 256, (K, size), dtype=np.uint8)
    d[1] = 0xFF
    d[2] = 0
    d[2, K - 1, size - 1] = 0x80
    return d


def _ptrs(rows):
    return (C.c_char_p * len(rows))(*[r.ctypes.data_as(C.c_char_p) for r in rows])


def mask_bits(masks, R, K, w):
    """the 0 / 1 bitmatrix B[r*w + l][j*w + x] = (mask[r*w + l][j] >> x) & 1 of row masks"""
    m = np.asarray(masks, np.uint32).reshape(R * w, K)
    return np.ascontiguousarray(((m[:, :, None] >> np.arange(w, dtype=np.uint32)) & 1).reshape(R * w, K * w).astype(np.int32))


def expected(shape, R, K, w, packet, mat, data):
    """the reference's output bytes, uint8 [N, R, size], of the network of `mat` over data uint8
    [N, K, size]"""
    lib = O.oracle()
    data = np.ascontiguousarray(data, np.uint8)
    n, k, size = data.shape
    assert k == K
    out = np.zeros((n, R, size), np.uint8)
    if shape in (0, 1):
        M = np.ascontiguousarray(np.asarray(mat, np.uint32).reshape(R, K)).view(np.int32)
    elif shape == 2:
        M = mask_bits(mat, R, K, w)
    else:
        M = np.ascontiguousarray(O.bitmatrix(np.asarray(mat, np.uint32).reshape(R, K).view(np.int32), w))
    for s in range(n):
        d, p = _ptrs([data[s, j] for j in range(K)]), _ptrs([out[s, r] for r in range(R)])
        if shape in (0, 1):
            assert size % (w // 8) == 0
            lib.eco_matrix_encode(K, R, w, M.ctypes.data_as(C.c_void_p), d, p, size)
        else:
            rc = lib.eco_bitmatrix_encode(K, R, w, M.ctypes.data_as(C.c_void_p), d, p, size, packet)
            assert rc == 0, "size must be a multiple of w * packet"
    return out


# ------------------------------------------------------------------ independent restatements
def times_x(v, w):
    """v * x in GF(2^w), v a uint64 array (or int) of elements below 2^w"""
    return ((v << 1) & ((1 << w) - 1)) ^ ((v >> (w - 1)) * (POLY[w] & ((1 << w) - 1)))


def gf_product(M, data, w):
    """out[r] = sum_j M[r][j] * data[j] over GF(2^w) by shift and xor: data uint8 [K, size] read as
    little-endian w-bit words; uint8 [R, size]"""
    M = np.asarray(M, np.uint64)
    R, K = M.shape
    word = {8: np.uint8, 16: "<u2", 32: "<u4"}[w]
    v = np.ascontiguousarray(data, np.uint8).view(word).astype(np.uint64)  # [K, words]
    out = np.zeros((R, v.shape[1]), np.uint64)
    for x in range(w):  # v holds data * x^x
        for r in range(R):
            for j in range(K):
                if (int(M[r, j]) >> x) & 1:
                    out[r] ^= v[j]
        v = times_x(v, w)
    return np.ascontiguousarray(out.astype(word)).view(np.uint8).reshape(R, -1)


def coef_masks(coef, w):
    """row masks [r*w + l][j] of R x K coefficients: bit x = bit l of c * x^x (the orientation of
    the engine's coef_masks and of eco_matrix_to_bitmatrix)"""
    coef = np.asarray(coef, np.uint64)
    R, K = coef.shape
    masks = np.zeros((R * w, K), np.uint64)
    for r in range(R):
        for j in range(K):
            cx = int(coef[r, j])
            for x in range(w):
                for l in range(w):
                    if (cx >> l) & 1:
                        masks[r * w + l, j] |= 1 << x
                cx = int(times_x(cx, w))
    return masks.astype(np.uint32)


def packet_xor(masks, data, w, packet):
    """the plain packet XOR of row masks [R*w][K] over data uint8 [K, size]: per super-packet of w
    packets, output packet l of row r = XOR of the input packets (j, x) whose mask bit is set"""
    masks = np.asarray(masks, np.uint64)
    K, size = data.shape
    R = masks.shape[0] // w
    d = data.reshape(K, size // (w * packet), w, packet)
    out = np.zeros((R, size // (w * packet), w, packet), np.uint8)
    for r in range(R):
        for l in range(w):
            for j in range(K):
                m = int(masks[r * w + l, j])
                for x in range(w):
                    if (m >> x) & 1:
                        out[r, :, l] ^= d[j, :, x]
    return out.reshape(R, size)
