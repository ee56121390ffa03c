#!/usr/bin/env python3
"""Time of lsec_encode_magic_dev_rotated beside the two-call sequence it replaces (lsec_encode_dev_rotated, then
lsec_check_magic_dev_rotated) and beside lsec_encode_dev_rotated alone, in one process on the same buffers
(DESIGN.md 3.9): C = 1 MiB, n_shift 1, RS(6+3) and Cauchy-good(6+3) at 1024 stripes (9 GiB of chunks: far past the
caches).  Results are checked first at the timed size: the fused call's parity is the plain rotated encode's and its
magics are the rotated check's own, with every syndrome zero.  Every case is warmed, the cases alternate inside each
round, and each sample is one call between two device events; one JSON line per case: median, min and max ms over
ROUNDS samples, the counted chunk traffic (reads + writes) over the median, and the median's ratio to the fused
call's.  Run from the repository root on a GPU."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402

C = 1 << 20
N = 1024
ROUNDS = 12
SHIFT, FIRST = 1, 7


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
        syn = torch.zeros(N, dtype=torch.int32, device="cuda")
        magic = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        again = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def plain():
            p.encode_dev_rotated_refs(refs, N, C, SHIFT, FIRST, st)

        def two_calls():
            p.encode_dev_rotated_refs(refs, N, C, SHIFT, FIRST, st)
            p.check_magic_dev_rotated_refs(refs, N, C, SHIFT, FIRST, syn.data_ptr(), again.data_ptr(), 0, 0, 0, st)

        def fused():
            p.encode_magic_dev_rotated_refs(refs, N, C, SHIFT, FIRST, magic.data_ptr(), st)

        # correctness at the timed size
        two_calls()
        want = dev.clone()
        fused()
        torch.cuda.synchronize()
        assert torch.equal(dev, want) and torch.equal(magic, again) and not bool(syn.any()), name
        del want
        cases = {"encode_rot": (plain, n), "encode_rot + check_magic_rot": (two_calls, 2 * n), "encode_magic_rot": (fused, n)}
        for fn, _ in cases.values():  # warm every shape
            fn()
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(ROUNDS):
            for c, (fn, _) in cases.items():
                ms[c].append(timed(fn))
        base = statistics.median(ms["encode_magic_rot"])
        for c, v in ms.items():
            med = statistics.median(v)
            row = dict(code=name, case=c, N=N, C=C, ms=round(med, 4), lo=round(min(v), 4), hi=round(max(v), 4),
                       TB_s=round(cases[c][1] * N * C / med / 1e9, 3), over_fused=round(med / base, 3))
            print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
