#!/usr/bin/env python3
"""A/B of the scrub with its checksum: (a) lsec_check_dev followed by lsec_stripe_magic_dev, the two
passes a caller had before, against (b) lsec_check_magic_dev, on one set of device buffers in one process.  RS(6+3) and
Cauchy-good(6+3), C = 1 MiB, 1024 stripes, one stripe in 64 with a flipped parity byte.  The results are checked first
at the timed size: (b) leaves the syndrome words, the count and the magics of (a), and the flipped stripes are the ones
reported.  The two cases alternate; each repetition is one call (pair) between two device events, after a warm-up of
both.  One JSON line per code: median, min and max ms of both over REPS repetitions, the ratio of the medians b / a,
and the counted chunk traffic over each median (a: 2 (k + m) chunk reads per stripe, b: k + m).  Run from the
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
        p.encode_dev_refs(refs, N, C, st)
        dev[k + 1, ::64, 4097] ^= 1  # parity row 1 of every 64th stripe
        syn_a = torch.full((N + 1,), -1, dtype=torch.int32, device="cuda")  # the words, then bad_count
        syn_b = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        counts_b = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        magic_a = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        magic_b = torch.ones(4 * N, dtype=torch.uint8, device="cuda")
        bad_b = torch.full((N,), 9, dtype=torch.uint8, device="cuda")

        def two_pass():
            p.check_dev_refs(refs, N, C, syn_a.data_ptr(), syn_a[N:].data_ptr(), st)
            p.stripe_magic_dev_refs(refs, N, C, magic_a.data_ptr(), st)

        def fused():
            p.check_magic_dev_refs(refs, N, C, syn_b.data_ptr(), magic_b.data_ptr(), magic_a.data_ptr(), bad_b.data_ptr(),
                                   counts_b.data_ptr(), st)

        # correctness at the timed size ((b) takes (a)'s magics as its expect: no magic bit may appear)
        two_pass()
        fused()
        torch.cuda.synchronize()
        want = torch.zeros(N, dtype=torch.int32, device="cuda")
        want[::64] = 2
        assert torch.equal(syn_a[:N], want) and torch.equal(syn_b, want) and syn_a[N].item() == N // 64, name
        assert torch.equal(magic_a, magic_b), name
        assert counts_b.tolist() == [N // 64, 0] and torch.equal(bad_b, (want != 0).to(torch.uint8)), name
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
        chunks = {"a": 2 * n, "b": n}  # chunk reads per stripe
        row = dict(code=name, N=N, C=C, reps=REPS, ratio_b_over_a=round(med["b"] / med["a"], 4))
        for c in cases:
            row[c] = dict(ms=round(med[c], 4), lo=round(min(ms[c]), 4), hi=round(max(ms[c]), 4),
                          TB_s=round(chunks[c] * N * C / med[c] / 1e9, 3))
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
