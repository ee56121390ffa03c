#!/usr/bin/env python3
"""A/B of the degraded read with its checksum: (a) lsec_decode_dev_patterns followed by
lsec_stripe_magic_dev, the two passes a caller had before, against (b) lsec_decode_magic_dev_patterns, on one set
of device buffers in one process.  RS(6+3) and Cauchy-good(6+3), C = 1 MiB, 1024 stripes, one erased data chunk
per stripe (the chunk differs from stripe to stripe: six patterns).  The results are checked first at the timed
size: (b) leaves the bytes and the magics of (a), and the rebuilt chunks are the ones that were overwritten.
The two cases alternate; each repetition is one call (pair) between two device events, after a warm-up of both.
One JSON line per code: median, min and max ms of both over REPS repetitions, the ratio of the medians b / a, and
the counted chunk traffic over each median (a: k + 1 + k + m chunks per stripe, b: k + m).  Run from the
repository root on a GPU."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402

C = 1 << 20
N = 1024
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
        dev = torch.randint(0, 256, (n, N, C), dtype=torch.uint8, device="cuda")
        refs = [(dev[i].data_ptr(), C) for i in range(n)]
        st = torch.cuda.current_stream().cuda_stream
        pats = [[j] for j in range(k)]
        ids = (torch.arange(N, dtype=torch.int32, device="cuda") % k).to(torch.uint8)
        magic_a = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        magic_b = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        p.encode_dev_refs(refs, N, C, st)
        clean = dev.clone()

        def erase():
            for j in range(k):
                dev[j, j::k].fill_(0xA5)

        def two_pass():
            p.decode_dev_patterns_refs(refs, N, C, pats, ids.data_ptr(), st)
            p.stripe_magic_dev_refs(refs, N, C, magic_a.data_ptr(), st)

        def fused():
            p.decode_magic_dev_patterns_refs(refs, N, C, pats, ids.data_ptr(), magic_b.data_ptr(), stream=st)

        # correctness at the timed size
        erase()
        two_pass()
        torch.cuda.synchronize()
        assert torch.equal(dev, clean), name
        erase()
        fused()
        torch.cuda.synchronize()
        assert torch.equal(dev, clean) and torch.equal(magic_a, magic_b), name
        del clean
        cases = {"a": two_pass, "b": fused}
        for _ in range(WARM):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(REPS):
            for c, fn in cases.items():
                ms[c].append(timed(fn))
        med = {c: statistics.median(v) for c, v in ms.items()}
        chunks = {"a": k + 1 + n, "b": n}  # reads + writes, in chunks per stripe
        row = dict(code=name, N=N, C=C, reps=REPS, ratio_b_over_a=round(med["b"] / med["a"], 4))
        for c in cases:
            row[c] = dict(ms=round(med[c], 4), lo=round(min(ms[c]), 4), hi=round(max(ms[c]), 4),
                          TB_s=round(chunks[c] * N * C / med[c] / 1e9, 3))
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
