#!/usr/bin/env python3
"""A/B of the search for the erasure set that fits the magic: (a) what a device-resident caller did
before -- per candidate, lsec_decode_magic_dev_patterns with `expect` over the failing stripes and then the erased
chunks put back from a saved copy, 130 launches and 130 restores -- against (b) one lsec_search_dev_patterns call,
in its four forms: the candidate or the piece of the chunk innermost in the tile order, non-temporal or plain
loads.  RS(6+3) and Cauchy-good(6+3), C = 1 MiB, 64 corrupt stripes (one, two or three chunks with a flipped byte
each), the full list of 130 candidates in the reference's order.  The results are checked first at the timed size:
every form finds each stripe's true corrupt set, (a) agrees, and no chunk has changed.  The cases alternate; each
repetition is one whole search between two device events, after a warm-up of all.  One JSON line per code and case:
median, min and max ms over REPS repetitions, the ratio of the median to (a)'s, and the counted chunk reads over
the median.  Run from the repository root on a GPU."""
import itertools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402
from lstore_amd import erasure as E  # noqa: E402

C = 1 << 20
N = 64
REPS, WARM = 15, 2
FORMS = {"b_cand_inner_nt": (False, False), "b_cand_inner_plain": (False, True),
         "b_cand_outer_nt": (True, False), "b_cand_outer_plain": (True, True)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for name, method, k, m in (("rs63", L.REED_SOL_VAN, 6, 3), ("cg63", L.CAUCHY_GOOD, 6, 3)):
    n = k + m
    pats = [[]] + [list(c) for e in range(1, m + 1) for c in itertools.combinations(range(n), e)]
    npat = len(pats)
    with L.Plan.for_chunk(method, k, m, C) as p:
        dev = torch.randint(0, 256, (n, N, C), dtype=torch.uint8, device="cuda")
        refs = [(dev[i].data_ptr(), C) for i in range(n)]
        st = torch.cuda.current_stream().cuda_stream
        p.encode_dev_refs(refs, N, C, st)
        expect = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        p.stripe_magic_dev_refs(refs, N, C, expect.data_ptr(), st)
        # corrupt sets of one, two and three chunks, a flipped byte in each
        gen = torch.Generator().manual_seed(63)
        truth = []
        for s in range(N):
            chunks = sorted(torch.randperm(n, generator=gen)[:1 + s % 3].tolist())
            truth.append(pats.index(chunks))
            for c in chunks:
                dev[c, s, (s * 977 + c * 131 + 5) % C] ^= 0x5A
        torch.cuda.synchronize()
        saved = dev.clone()
        found = torch.zeros(N, dtype=torch.uint8, device="cuda")
        magic = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
        bad = torch.zeros((npat, N), dtype=torch.uint8, device="cuda")
        ids = [torch.full((N,), q, dtype=torch.uint8, device="cuda") for q in range(npat)]

        def per_candidate():
            for q in range(npat):
                p.decode_magic_dev_patterns_refs(refs, N, C, pats, ids[q].data_ptr(), magic.data_ptr(), expect.data_ptr(),
                                                 bad[q].data_ptr(), 0, st)
                for c in pats[q]:
                    dev[c].copy_(saved[c])

        def one_call():
            p.search_dev_patterns_refs(refs, N, C, pats, expect.data_ptr(), found.data_ptr(), stream=st)

        def form(cand_outer, plain):
            def run():
                E.set_search_form(cand_outer, plain)
                one_call()
            return run

        cases = {"a_per_candidate": per_candidate}
        cases.update({c: form(*f) for c, f in FORMS.items()})
        # correctness at the timed size
        per_candidate()
        torch.cuda.synchronize()
        first_fit = (bad == 0).to(torch.int32).argmax(dim=0).tolist()
        assert first_fit == truth and torch.equal(dev, saved), name
        for c in FORMS:
            found.fill_(0x7B)
            cases[c]()
            torch.cuda.synchronize()
            assert found.tolist() == truth and torch.equal(dev, saved), (name, c)
        for _ in range(WARM):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(REPS):
            for c, fn in cases.items():
                ms[c].append(timed(fn))
        E.set_search_form()  # back to the form that ships
        med = {c: statistics.median(v) for c, v in ms.items()}
        reads = sum(n - len(q) for q in pats)  # chunk reads per stripe: k + m - e per candidate
        for c in cases:
            print(json.dumps(dict(code=name, case=c, N=N, C=C, candidates=npat, reps=REPS, ms=round(med[c], 4),
                                  lo=round(min(ms[c]), 4), hi=round(max(ms[c]), 4),
                                  ratio_to_a=round(med[c] / med["a_per_candidate"], 4),
                                  read_TB_s=round(reads * N * C / med[c] / 1e9, 3))), flush=True)
        del dev, saved
        torch.cuda.empty_cache()
