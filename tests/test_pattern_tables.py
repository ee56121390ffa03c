"""Host side of the per-stripe-pattern decodes (lsec_decode_dev_patterns / lsec_decode_dev_rotated):
the pattern tables the engine builds, checked without a GPU through lsec_test_pattern_table.

The selection lists are checked against a restatement of the LUN rotation (lun.c:1178-1223) and of
Jerasure's survivor choice (the first k surviving ids, jerasure.c:100-128); the coefficient rows by
applying them in numpy, over a GF(2^8) product table built here from polynomial 0x11D, to stripes
the oracle encoded.
"""
import ctypes as C
import math

import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E


# ---------------------------------------------------------------- GF(2^8), polynomial 0x11D
def _gf_table():
    exp, log = [0] * 512, [0] * 256
    x = 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    for i in range(255, 512):
        exp[i] = exp[i - 255]
    t = np.zeros((256, 256), np.uint8)
    for a in range(1, 256):
        for b in range(1, 256):
            t[a, b] = exp[log[a] + log[b]]
    return t


GF = _gf_table()


def apply_rows(rows, inputs):
    """rows [e, k] over GF(2^8), inputs [k, ...] uint8 -> [e, ...]"""
    out = np.zeros((rows.shape[0],) + inputs.shape[1:], np.uint8)
    for r in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            out[r] ^= GF[int(rows[r, j])][inputs[j]]
    return out


def packet_elements(chunk, P):
    """Jerasure's packet layout at w = 8 -> field elements: bit b of byte t of packet x of a
    super-packet is bit x of element (t, b).  [C] -> [C / (8P), P, 8] (a bijection)."""
    sp = chunk.reshape(-1, 8, P)
    bits = np.unpackbits(sp, axis=-1, bitorder="little").reshape(sp.shape[0], 8, P, 8)  # [sp, x, t, b]
    el = np.zeros((sp.shape[0], P, 8), np.uint8)
    for x in range(8):
        el |= bits[:, x] << x
    return el


# ---------------------------------------------------------------- restatement of the table
def survivors_of(k, n, erased):
    return [i for i in range(n) if i not in erased][:k]


def rotated_entry(k, n, lost, rot):
    """(nout, in_sel, out_sel) of rotation `rot`: physical device i holds logical chunk (i + rot) mod n"""
    erased = sorted((d + rot) % n for d in set(lost))
    return (len(erased), [(c - rot) % n for c in survivors_of(k, n, erased)], [(c - rot) % n for c in erased])


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


# ---------------------------------------------------------------- selection arithmetic
@pytest.mark.parametrize("lost", [[2], [2, 7]])
@pytest.mark.parametrize("n_shift", [0, 1, 2, 3, 9, 10])
def test_rotated_selection_lists(rs63, lost, n_shift):
    k, n = 6, 9
    reachable = {((f + s) * n_shift) % n for f in (0, 5) for s in range(2 * n)}
    assert len(reachable) == n // math.gcd(n, n_shift % n if n_shift % n else n)
    if n_shift == 3:
        assert reachable == {0, 3, 6}
    for rot in range(n):
        nout, in_sel, out_sel, rows = E.pattern_table_entry(rs63, rot, lost=lost, n_shift=n_shift)
        if rot not in reachable:
            assert nout == -1, (rot, nout)
            continue
        want = rotated_entry(k, n, lost, rot)
        assert (nout, in_sel, out_sel) == want, (rot, nout, in_sel, out_sel, want)
        assert rows.shape == (len(lost), k)
        # no shard is both read and written, and every index is a device of the call
        assert not set(in_sel) & set(out_sel) and set(out_sel) == set(lost)
        assert all(0 <= i < n for i in in_sel + out_sel)


def test_patterned_selection_lists(rs63):
    k, n = 6, 9
    pats = [[], [0], [5], [6], [8], [0, 5], [7, 1], [6, 8], [0, 3, 5], [2, 6, 7]]
    for i, pat in enumerate(pats):
        nout, in_sel, out_sel, rows = E.pattern_table_entry(rs63, i, patterns=pats)
        erased = sorted(pat)
        assert nout == len(erased) and out_sel == erased
        assert in_sel == (survivors_of(k, n, erased) if erased else [-1] * k)


def test_rot0_is_64_bit(built):
    f = 3_000_000_007
    for n, n_shift in ((9, 1), (9, 2), (9, 3), (9, 10), (14, 5), (9, 0), (128, 2_000_000_011)):
        assert E.pattern_rot0(n, n_shift, f) == (f * n_shift) % n, (n, n_shift)
    assert E.pattern_rot0(9, 1, 5) == 5


# ---------------------------------------------------------------- coefficient rows
CODES = [
    ("rs63", L.REED_SOL_VAN, 6, 3, [[0], [5], [6], [8], [0, 5], [1, 7], [6, 8], [0, 3, 5], [2, 6, 7]]),
    ("rs104", L.REED_SOL_VAN, 10, 4, [[3], [11], [0, 9], [2, 10, 13], [0, 1, 2, 3], [4, 10, 11, 12], [10, 11, 12, 13]]),
    ("r6", L.REED_SOL_R6_OP, 6, 2, [[0], [6], [7], [0, 5], [2, 6], [3, 7], [6, 7]]),
    ("raid4", L.RAID4, 4, 1, [[0], [3], [4]]),
]


@pytest.mark.parametrize("name,method,k,m,pats", CODES, ids=[c[0] for c in CODES])
def test_rows_rebuild_reference_stripes(built, name, method, k, m, pats):
    size, n = 512, k + m
    rng = np.random.default_rng(k * 100 + m)
    data = rng.integers(0, 256, (k, size), dtype=np.uint8)
    full = np.vstack([data, O.encode(method, data, m)])
    with L.Plan.new(method, size, k, m, 8, 0, 1 if method == L.RAID4 else 8) as p:
        p.form_encoding_matrix()
        p.form_decoding_matrix()
        # as a rotated call sees them too: rotation 4 with the devices that hold these chunks lost
        for i, pat in enumerate(pats):
            for rot, entry in ((0, E.pattern_table_entry(p, i, patterns=pats)),
                               (4, E.pattern_table_entry(p, 4, lost=[(c - 4) % n for c in pat], n_shift=1))):
                nout, in_sel, out_sel, rows = entry
                if method == L.RAID4 and pat[0] >= k:
                    assert nout == 0  # raid4.c:48 leaves lost parity alone
                    continue
                assert nout == len(pat)
                inputs = np.stack([full[(s + rot) % n] for s in in_sel])
                got = apply_rows(rows, inputs)
                want = np.stack([full[(s + rot) % n] for s in out_sel])
                assert sorted((s + rot) % n for s in out_sel) == sorted(pat)
                assert np.array_equal(got, want), (pat, rot)


def test_cauchy_rows_rebuild_reference_stripes(built):
    """Cauchy-good(6+3) at w = 8: the rows act on field elements, which Jerasure's packet layout
    spreads over the 8 packets of a super-packet."""
    k, m, P = 6, 3, 16
    size = 8 * P * 3
    pats = [[0], [5], [6], [8], [0, 5], [1, 7], [6, 8], [0, 3, 5], [2, 6, 7]]
    rng = np.random.default_rng(63)
    data = rng.integers(0, 256, (k, size), dtype=np.uint8)
    full = np.vstack([data, O.encode(L.CAUCHY_GOOD, data, m, P, 8)])
    elems = np.stack([packet_elements(full[i], P) for i in range(k + m)])
    with L.Plan.new(L.CAUCHY_GOOD, size, k, m, 8, P, 8) as p:
        p.form_encoding_matrix()
        p.form_decoding_matrix()
        assert p.kernel == 2
        for i, pat in enumerate(pats):
            nout, in_sel, out_sel, rows = E.pattern_table_entry(p, i, patterns=pats)
            assert nout == len(pat) and out_sel == sorted(pat)
            assert np.array_equal(apply_rows(rows, elems[in_sel]), elems[out_sel]), pat
        # the single-data-loss rows are the 0 / 1 rows the single-pattern path hands the XOR kernel
        _, _, _, rows = E.pattern_table_entry(p, 0, patterns=pats)
        assert set(rows.ravel().tolist()) <= {0, 1}


# ---------------------------------------------------------------- rejections (no GPU call: this runs without one)
def _call_patterns(p, pats_flat, npatterns, nstripes=0):
    n = p.k + p.m
    sh = (E.ShardRef * n)()
    arr = (C.c_int * len(pats_flat))(*pats_flat)
    return L.lib().lsec_decode_dev_patterns(p.ptr, sh, nstripes, 4096, arr, npatterns, None, None)


def _call_rotated(p, lost, n_shift, first_stripe=0):
    n = p.k + p.m
    sh = (E.ShardRef * n)()
    arr = (C.c_int * (len(lost) + 1))(*(list(lost) + [-1]))
    return L.lib().lsec_decode_dev_rotated(p.ptr, sh, 0, 4096, arr, n_shift, first_stripe, None)


REJECTED = [
    ("npatterns 0", lambda p: _call_patterns(p, [-1], 0), "npatterns"),
    ("npatterns 257", lambda p: _call_patterns(p, [0, -1] * 257, 257), "npatterns"),
    ("id out of range", lambda p: _call_patterns(p, [0, -1, 9, -1], 2), "out of range"),
    ("m+1 erasures", lambda p: _call_patterns(p, [0, -1, 0, 1, 2, 3, -1], 2), "exceed m=3"),
    ("more than m lost", lambda p: _call_rotated(p, [0, 1, 2, 3], 1), "exceed m=3"),
    ("lost out of range", lambda p: _call_rotated(p, [9], 1), "out of range"),
    ("n_shift < 0", lambda p: _call_rotated(p, [2], -1), "n_shift"),
    ("first_stripe < 0", lambda p: _call_rotated(p, [2], 1, -5), "first_stripe"),
]


@pytest.mark.parametrize("what,call,words", REJECTED, ids=[r[0].replace(" ", "_") for r in REJECTED])
def test_rejections(rs63, what, call, words):
    assert call(rs63) == -1, what
    msg = E.last_error()
    assert msg and words in msg, (what, msg)


def test_rejects_null_pointers_and_other_kernels(rs63, built):
    lib = L.lib()
    sh = (E.ShardRef * 9)()
    one = (C.c_int * 2)(0, -1)
    assert lib.lsec_decode_dev_patterns(rs63.ptr, None, 0, 4096, one, 1, None, None) == -1 and "NULL" in E.last_error()
    assert lib.lsec_decode_dev_patterns(rs63.ptr, sh, 0, 4096, None, 1, None, None) == -1 and "NULL" in E.last_error()
    assert lib.lsec_decode_dev_patterns(rs63.ptr, sh, 4, 4096, one, 1, None, None) == -1 and "stripe_pattern" in E.last_error()
    assert lib.lsec_decode_dev_rotated(rs63.ptr, sh, 0, 4096, None, 1, 0, None) == -1 and "NULL" in E.last_error()
    assert lib.lsec_decode_dev_patterns(rs63.ptr, sh, 0, 4100, one, 1, None, None) == -1 and "multiple of 8" in E.last_error()
    # a liberation plan (kernel 3), RS at w = 16 (kernel 4), and a stripe wider than 64 data chunks
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        assert _call_patterns(p, [0, -1], 1) == -1 and "kernel 3" in E.last_error()
        assert _call_rotated(p, [0], 1) == -1 and "kernel 3" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert _call_patterns(p, [0, -1], 1) == -1 and "kernel 4" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 70, 4, 8, 0, 8) as p:
        assert _call_patterns(p, [0, -1], 1) == -1 and "k=70" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 60, 70, 8, 0, 8) as p:
        assert _call_patterns(p, [0, -1], 1) == -1 and "128" in E.last_error()


def test_abi_version_and_python_mirror(built):
    assert L.lib().lsec_abi_version() == 3
    for name in ("decode_dev_patterns_refs", "decode_dev_patterns", "decode_dev_rotated_refs"):
        assert callable(getattr(L.Plan, name))
