#!/usr/bin/env python3
"""Generate the network source of a fixed list of matrices for a fixed list of LSEC_JIT_VARIANT
values with build/jit_src (tools/jit_src.cpp; `make jit_src` in lstore_amd/csrc) and write a
manifest, one line per (case, variant): name, variant, sha256 of the source, its length.  Two
trees whose generators emit the same text give the same manifest (the matrices come from a fixed
seed), and identical text means identical code objects: profiles/netgen_refactor.txt.

  python tools/jit_sources.py --out manifest.txt [--jit-src PATH] [--keep DIR] [--jobs N]
"""
import argparse
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = [0, 0x1, 0x2, 0x8, 0x9, 0x10, 0x20, 0x28, 0x40, 0x100, 0xFF00, 0x10000, 0x20000, 0x40000, 0x60000, 0x80000,
            0x100000, 0x200000, 0x380000, 0x400000, 0x800000, 0xC00000, 0x1000000, 0x2000000, 0x4000000, 0x6000000,
            0x10000000, 0x40000000]


def times_x(c, w):
    """c * x in GF(2^w), Jerasure's polynomials"""
    c <<= 1
    if c >> w:
        c = (c ^ {8: 0x11D, 16: 0x1100B, 32: 0x100400007}[w]) & ((1 << w) - 1)
    return c


def coef_masks(coef, w):
    """row masks [(r*w + l)*K + j] of an R x K GF(2^w) matrix: bit x = bit l of c * x^x"""
    R, K = coef.shape
    masks = np.zeros((R * w, K), dtype=np.uint64)
    for r in range(R):
        for j in range(K):
            cx = int(coef[r, j])
            for x in range(w):
                for l in range(w):
                    if (cx >> l) & 1:
                        masks[r * w + l, j] |= 1 << x
                cx = times_x(cx, w)
    return masks


def cases():
    """(name, stdin text of jit_src) for every case, from one seeded generator in a fixed order"""
    rng = np.random.default_rng(20250607)
    out = []

    def coef(R, K, w):
        return rng.integers(1, 1 << w, size=(R, K), dtype=np.uint64)

    def matrix(name, M, w):
        out.append((name, f"{M.shape[0]} {M.shape[1]} {w} " + " ".join(str(int(v)) for v in M.flatten())))

    def packets(name, masks, R, K, w, packet):
        assert masks.shape == (R * w, K)
        out.append((name, f"P {R} {K} {w} {packet} " + " ".join(str(int(v)) for v in masks.flatten())))

    # w = 8: both sides of the piece count (K * 8 <= 104), the 8 B lanes (R >= 8), the kernarg
    # reload (K + R >= 24); an all-zero row
    for R, K in ((6, 20), (8, 12), (8, 32), (6, 13), (6, 14), (3, 20), (4, 20)):
        matrix(f"w8_{R}x{K}", coef(R, K, 8), 8)
    M = coef(2, 10, 8)
    M[0, :] = 0
    matrix("w8_2x10_zero_row0", M, 8)
    # w = 32: one wave; the split with rows dividing unevenly and 12 KiB slots; an even and an odd
    # count of used inputs
    for R, K in ((3, 6), (4, 10), (5, 9), (6, 10)):
        matrix(f"w32_{R}x{K}", coef(R, K, 32), 32)
    M = coef(4, 7, 32)
    full = M.copy()
    M[:, 3] = 0
    matrix("w32_4x7_zero_col3", M, 32)
    matrix("w32_4x7_odd_inputs", full, 32)
    # w = 16: one wave, the split, 8 rows, a zero row, coefficients 1
    for R, K in ((4, 10), (5, 11), (6, 20), (8, 20)):
        matrix(f"w16_{R}x{K}", coef(R, K, 16), 16)
    M = coef(5, 9, 16)
    M[2, :] = 0
    matrix("w16_5x9_zero_row2", M, 16)
    M = coef(4, 9, 16)
    M[1, :] = 0
    matrix("w16_4x9_zero_row1", M, 16)
    M = coef(6, 12, 16)
    M[0, :] = 1
    M[3, ::2] = 1
    matrix("w16_6x12_ones", M, 16)
    M = coef(3, 8, 32)
    M[0, :] = 1
    matrix("w32_3x8_ones", M, 32)

    # packet networks: sparse random masks, then coefficient bitmatrices, then the empty corners
    def sparse(R, K, w):
        return rng.integers(0, 1 << w, size=(R * w, K), dtype=np.uint64) & rng.integers(0, 1 << w, size=(R * w, K), dtype=np.uint64)

    for R, K, w, packet in ((2, 6, 7, 32), (2, 16, 16, 32), (2, 8, 8, 40), (2, 5, 3, 16)):
        packets(f"pkt_{R}x{K}_w{w}_p{packet}", sparse(R, K, w), R, K, w, packet)
    for R, K, w, packet in ((4, 10, 32, 64), (4, 10, 16, 32), (3, 6, 8, 32)):
        packets(f"pkt_coef_{R}x{K}_w{w}_p{packet}", coef_masks(coef(R, K, w), w), R, K, w, packet)
    m = sparse(2, 6, 8)
    m[3, :] = 0
    packets("pkt_2x6_w8_zero_output_row3", m, 2, 6, 8, 32)
    m = sparse(2, 7, 5)
    m[:, 4] = 0
    packets("pkt_2x7_w5_unread_input4", m, 2, 7, 5, 24)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--jit-src", default=os.path.join(ROOT, "build", "jit_src"))
    ap.add_argument("--out", default="-", help="manifest file (default: stdout)")
    ap.add_argument("--keep", metavar="DIR", help="also write every source into DIR")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)

    def one(job):
        name, text, v = job
        r = subprocess.run([a.jit_src], input=text.encode(), capture_output=True, env=dict(os.environ, LSEC_JIT_VARIANT=str(v)))
        if r.returncode:
            return f"{name} {v:#x} failed rc={r.returncode}"
        if a.keep:
            with open(os.path.join(a.keep, f"{name}_v{v:#x}.hip"), "wb") as f:
                f.write(r.stdout)
        return f"{name} {v:#x} {hashlib.sha256(r.stdout).hexdigest()} {len(r.stdout)}"

    jobs = [(name, text, v) for name, text in cases() for v in VARIANTS]
    with ThreadPoolExecutor(a.jobs) as pool:
        lines = list(pool.map(one, jobs))
    body = "".join(line + "\n" for line in lines)
    if a.out == "-":
        sys.stdout.write(body)
    else:
        with open(a.out, "w") as f:
            f.write(body)
    bad = sum(" failed " in line for line in lines)
    print(f"{len(lines)} sources, {bad} failed, manifest sha256 {hashlib.sha256(body.encode()).hexdigest()}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
