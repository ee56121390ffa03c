#!/usr/bin/env python3
"""A/B of the directed decode of a rotated LUN with its checksum, on one set of device buffers in one
process:
  (a) lsec_decode_magic_dev_patterns_rotated, one pass: k+m-1 chunk reads and 1 write per stripe;
  (b) lsec_decode_dev_patterns_rotated followed by lsec_check_magic_dev_rotated on the same buffers, the two passes a
      caller of a rotated LUN had to string together: k reads and 1 write, then k+m reads;
  (c) lsec_decode_magic_dev_patterns over the unrotated layout of the same logical stripes: what the rotation's
      scalar work is measured against.
RS(6+3) and Cauchy-good(6+3), C = 1 MiB, 1024 stripes, n_shift = 1, one erased data chunk per stripe (the ids cycle
over the k single-erasure patterns).  The results are checked first at the timed size: every case rebuilds the
chunks that were overwritten, and the three leave the same magics.  The three cases alternate; each repetition is one
call (pair) between two device events, after a warm-up of all three.  One JSON line per code: median, min and max ms
of each over REPS repetitions, the ratios of the medians a / b and a / c, and the counted chunk traffic over each
median.  Run from the repository root on a GPU."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402

C = 1 << 20
N = 1024
N_SHIFT, FIRST = 1, 0
REPS, WARM = 25, 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for name, method, k, m in (("rs63", L.REED_SOL_VAN, 6, 3), ("cg63", L.CAUCHY_GOOD, 6, 3)):
    n = k + m
    with L.Plan.for_chunk(method, k, m, C) as p:
        st = torch.cuda.current_stream().cuda_stream
        flat = torch.randint(0, 256, (n, N, C), dtype=torch.uint8, device="cuda")   # logical chunk c: flat[c]
        frefs = [(flat[i].data_ptr(), C) for i in range(n)]
        p.encode_dev_refs(frefs, N, C, st)
        rot = torch.empty_like(flat)                                                # physical device i: rot[i]
        for r in range(n):  # the stripes of rotation r: device i holds logical chunk (i + r) mod n
            for i in range(n):
                rot[i, r::n] = flat[(i + r) % n, r::n]
        rrefs = [(rot[i].data_ptr(), C) for i in range(n)]
        clean_flat, clean_rot = flat.clone(), rot.clone()
        pats = [[j] for j in range(k)]
        stripe = torch.arange(N, device="cuda")
        ids = (stripe % k).to(torch.uint8)
        erased_dev = (stripe % k - (FIRST + stripe) * N_SHIFT) % n                  # where that chunk lies, per stripe
        magic = {c: torch.zeros(4 * N, dtype=torch.uint8, device="cuda") for c in "abc"}
        syndrome = torch.zeros(N, dtype=torch.int32, device="cuda")

        def erase():
            for j in range(k):
                flat[j, j::k].fill_(0xA5)
            rot[erased_dev, stripe] = 0xA5

        def one_pass():
            p.decode_magic_dev_patterns_rotated_refs(rrefs, N, C, N_SHIFT, FIRST, pats, ids.data_ptr(), magic["a"].data_ptr(),
                                                     stream=st)

        def two_pass():
            p.decode_dev_patterns_rotated_refs(rrefs, N, C, N_SHIFT, FIRST, pats, ids.data_ptr(), st)
            p.check_magic_dev_rotated_refs(rrefs, N, C, N_SHIFT, FIRST, syndrome.data_ptr(), magic["b"].data_ptr(), stream=st)

        def unrotated():
            p.decode_magic_dev_patterns_refs(frefs, N, C, pats, ids.data_ptr(), magic["c"].data_ptr(), stream=st)

        cases = {"a": one_pass, "b": two_pass, "c": unrotated}
        # correctness at the timed size
        for c, fn in cases.items():
            erase()
            assert not torch.equal(rot, clean_rot) and not torch.equal(flat, clean_flat)
            fn()
            torch.cuda.synchronize()
            assert torch.equal(flat if c == "c" else rot, clean_flat if c == "c" else clean_rot), (name, c)
        assert torch.equal(magic["a"], magic["b"]) and torch.equal(magic["a"], magic["c"]) and not syndrome.any().item(), name
        del clean_flat, clean_rot
        for _ in range(WARM):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(REPS):
            for c, fn in cases.items():
                ms[c].append(timed(fn))
        med = {c: statistics.median(v) for c, v in ms.items()}
        chunks = {"a": n, "b": k + 1 + n, "c": n}  # reads + writes, in chunks per stripe
        row = dict(code=name, N=N, C=C, n_shift=N_SHIFT, reps=REPS, ratio_a_over_b=round(med["a"] / med["b"], 4),
                   ratio_a_over_c=round(med["a"] / med["c"], 4))
        for c in cases:
            row[c] = dict(ms=round(med[c], 4), lo=round(min(ms[c]), 4), hi=round(max(ms[c]), 4),
                          TB_s=round(chunks[c] * N * C / med[c] / 1e9, 3))
        print(json.dumps(row), flush=True)
        del flat, rot
        torch.cuda.empty_cache()
