#!/usr/bin/env python3
"""Rate of lsec_encode_dev_rotated / lsec_update_dev_rotated beside the unrotated calls on the same
buffers: C = 1 MiB, RS(6+3) and Cauchy-good(6+3) at 1024 stripes, RS(16+4) at 512.
Results are checked first at the timed size (n_shift = 0 against lsec_encode_dev / lsec_update_dev,
n_shift = 1 and 3 by lsec_check_dev_rotated).  The cases alternate inside each round; one JSON line per
case: median, min and max ms per launch over 7 rounds of 5 launches (device events), and the counted
chunk traffic (reads + writes) over the median.  Run from the repository root on a GPU."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402

C = 1 << 20
ROUNDS, PER = 7, 5


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(PER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / PER


for name, method, k, m, N in (("rs63", L.REED_SOL_VAN, 6, 3, 1024), ("rs164", L.REED_SOL_VAN, 16, 4, 512),
                              ("cg63", L.CAUCHY_GOOD, 6, 3, 1024)):
    n = k + m
    with L.Plan.for_chunk(method, k, m, C) as p:
        dev = torch.randint(0, 256, (n, N, C), dtype=torch.uint8, device="cuda")
        fresh = torch.randint(0, 256, (1, N, C), dtype=torch.uint8, device="cuda")
        refs = [(dev[i].data_ptr(), C) for i in range(n)]
        frefs = [(fresh[0].data_ptr(), C)]
        syn = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        cols = [3]
        # correctness at the timed size: n_shift = 0 is encode_dev; n_shift = 1 checks clean, also after an update
        p.encode_dev_refs(refs, N, C, st)
        want = dev[k:].clone()
        dev[k:].fill_(0x5A)
        p.encode_dev_rotated_refs(refs, N, C, 0, 7, st)
        assert torch.equal(dev[k:], want), name
        p.update_dev_refs(refs, N, C, cols, frefs, True, st)
        want = dev.clone()
        dev[3].copy_(torch.randint(0, 256, (N, C), dtype=torch.uint8, device="cuda"))
        p.encode_dev_rotated_refs(refs, N, C, 0, 7, st)
        p.update_dev_rotated_refs(refs, N, C, 0, 7, cols, frefs, True, st)
        assert torch.equal(dev, want), name
        for shift in (1, 3):
            p.encode_dev_rotated_refs(refs, N, C, shift, 3_000_000_007, st)
            p.update_dev_rotated_refs(refs, N, C, shift, 3_000_000_007, cols, frefs, True, st)
            p.check_dev_rotated_refs(refs, N, C, shift, 3_000_000_007, syn.data_ptr(), syn[N:].data_ptr(), st)
            torch.cuda.synchronize()
            assert int(syn[N]) == 0 and not bool(syn[:N].any()), (name, shift)
        cases = {
            "encode_dev": lambda: p.encode_dev_refs(refs, N, C, st),
            "encode_rot shift0": lambda: p.encode_dev_rotated_refs(refs, N, C, 0, 7, st),
            "encode_rot shift1": lambda: p.encode_dev_rotated_refs(refs, N, C, 1, 7, st),
            "check_rot shift1": lambda: p.check_dev_rotated_refs(refs, N, C, 1, 7, syn.data_ptr(), 0, st),
            "update_dev store": lambda: p.update_dev_refs(refs, N, C, cols, frefs, True, st),
            "update_rot shift0 store": lambda: p.update_dev_rotated_refs(refs, N, C, 0, 7, cols, frefs, True, st),
            "update_rot shift1 store": lambda: p.update_dev_rotated_refs(refs, N, C, 1, 7, cols, frefs, True, st),
        }
        for fn in cases.values():  # warm every shape
            fn()
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(ROUNDS):
            for c, fn in cases.items():
                ms[c].append(timed(fn))
        for c, v in ms.items():
            chunks = (2 + 2 * m + 1) if c.startswith("update") else n  # reads + writes, in chunks per stripe
            med = statistics.median(v)
            row = dict(code=name, case=c, N=N, ms=round(med, 4), lo=round(min(v), 4), hi=round(max(v), 4),
                       TB_s=round(chunks * N * C / med / 1e9, 3))
            print(json.dumps(row), flush=True)
        del dev, fresh
        torch.cuda.empty_cache()
