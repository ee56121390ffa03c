#!/usr/bin/env python3
"""A/B of the read path's quorum vote on the device.

vote   4096 RS(6+3) stripes, magics at record stride 4, one stripe in four with one or two dissenting chunks and no
       blank candidate, the list of all 130 erasure sets.  (a) the round trip a device-resident caller made before:
       the (k+m)*4 bytes per stripe copied to page-locked host memory, the vote there -- a NUMPY restatement of the
       rules, vectorised over the stripes, not the engine's C++ -- then ids and quorum copied back, and a
       synchronise; (b) one lsec_vote_dev call and a synchronise.  Both are wall-clock times around the same
       synchronise, since (a) has host work in it; (b) is also given between two device events.
scan   4096 all-zero stripes of 1 MiB chunks (36 GiB), zero magics: every stripe is a blank candidate and the scan
       reads every chunk.  (c) lsec_stripe_magic_dev over the same arena, the only call that read all k+m chunks on
       the device before; (d) lsec_vote_dev in the scan's four forms: plain or non-temporal loads, tiles of 2 or 4
       16-byte steps per lane.  Between two device events.
The results are checked first at the timed size.  The cases alternate; medians over REPS repetitions after a warm-up of
all.  One JSON line per case.  Run from the repository root on a GPU."""
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lstore_amd as L  # noqa: E402
from lstore_amd import erasure as E  # noqa: E402

K, M, N = 6, 3, 4096
C = 1 << 20
REPS, WARM = 15, 2
FORMS = {"d_plain_2": (True, 2), "d_nt_2": (False, 2), "d_plain_4": (True, 4), "d_nt_4": (False, 4)}
n = K + M
pats = [[]] + [list(c) for e in range(1, M + 1) for c in itertools.combinations(range(n), e)]


def device_timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_vote(words, masks_sorted, masks_order):
    """words uint32 [N, n] -> (quorum uint32 [N], ids uint8 [N]) by the rules of lsec_vote_dev with LSEC_VOTE_PARANOID:
    the largest group of equal words, the lowest first member on a tie; LOST below k members; else the lowest pattern
    whose set is the outside set"""
    eq = words[:, :, None] == words[:, None, :]
    count = eq.sum(axis=2)
    best = count.argmax(axis=1)  # the first of the largest: its lowest member
    rows = np.arange(words.shape[0])
    member = eq[rows, best]
    outside = ((~member).astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(axis=1)
    at = np.minimum(np.searchsorted(masks_sorted, outside), len(masks_sorted) - 1)
    ids = np.where(masks_sorted[at] == outside, masks_order[at], E.LOCATE_MANY).astype(np.uint8)
    ids[count[rows, best] < K] = E.LOCATE_MANY
    return words[rows, best], ids


def report(case, ms, base, **extra):
    med = statistics.median(ms[case])
    print(json.dumps(dict(case=case, N=N, reps=REPS, ms=round(med, 4), lo=round(min(ms[case]), 4), hi=round(max(ms[case]), 4),
                          ratio=round(med / statistics.median(ms[base]), 4), ratio_to=base, **extra)), flush=True)


with L.Plan.for_chunk(L.REED_SOL_VAN, K, M, C) as p:
    st = torch.cuda.current_stream().cuda_stream
    # ---------------------------------------------------------------- the vote
    rng = np.random.default_rng(63)
    words = np.repeat(rng.integers(1, 1 << 32, (N, 1), dtype=np.uint32), n, axis=1)
    for s in range(0, N, 4):
        for c in rng.permutation(n)[:1 + (s // 4) % 2]:
            words[s, c] ^= 0x5A5A
    mags = torch.from_numpy(np.ascontiguousarray(words.T).view(np.uint8)).cuda()  # [n, 4N] bytes: record stride 4
    stored = [(mags[i].data_ptr(), 4) for i in range(n)]
    host_mags = torch.empty((n, N * 4), dtype=torch.uint8, pin_memory=True)
    host_ids = torch.empty(N, dtype=torch.uint8, pin_memory=True)
    host_quorum = torch.empty(4 * N, dtype=torch.uint8, pin_memory=True)
    quorum = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
    cls, ids = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    ids_a, quorum_a = torch.zeros_like(ids), torch.zeros_like(quorum)
    mask_of = np.array([sum(1 << c for c in q) for q in pats], np.uint64)
    order = np.argsort(mask_of, kind="stable")
    masks_sorted, masks_order = mask_of[order], order

    def round_trip():
        host_mags.copy_(mags, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        w = host_mags.numpy().view("<u4").T
        q, i = host_vote(w, masks_sorted, masks_order)
        host_quorum.numpy()[:] = q.astype("<u4").view(np.uint8)
        host_ids.numpy()[:] = i
        quorum_a.copy_(host_quorum, non_blocking=True)
        ids_a.copy_(host_ids, non_blocking=True)

    def vote():
        p.vote_dev_refs(stored, None, N, 0, pats, quorum.data_ptr(), cls.data_ptr(), ids.data_ptr(), 0, 0, E.VOTE_PARANOID, st)

    round_trip()
    vote()
    torch.cuda.synchronize()
    assert torch.equal(quorum, quorum_a) and torch.equal(ids, ids_a), "the device vote and the host restatement differ"
    assert set(cls.tolist()) <= {E.VOTE_OK, E.VOTE_DEGRADED} and E.LOCATE_MANY not in ids.tolist()
    for _ in range(WARM):
        round_trip()
        vote()
    ms = {"a_round_trip_numpy": [], "b_vote_dev": [], "b_vote_dev_device_time": []}
    for _ in range(REPS):
        ms["a_round_trip_numpy"].append(wall_timed(round_trip))
        ms["b_vote_dev"].append(wall_timed(vote))
        ms["b_vote_dev_device_time"].append(device_timed(vote))
    for case in ms:
        report(case, ms, "a_round_trip_numpy", part="vote", code="rs63", candidates=len(pats))

    # ---------------------------------------------------------------- the blank scan
    arena = torch.zeros((n, N, C), dtype=torch.uint8, device="cuda")
    refs = [(arena[i].data_ptr(), C) for i in range(n)]
    zmags = torch.zeros((n, N), dtype=torch.int32, device="cuda")
    zstored = [(zmags[i].data_ptr(), 4) for i in range(n)]
    magic = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(5, dtype=torch.int32, device="cuda")

    def stripe_magic():
        p.stripe_magic_dev_refs(refs, N, C, magic.data_ptr(), st)

    def scan(plain, steps):
        def run():
            E.set_vote_form(plain, steps)
            p.vote_dev_refs(zstored, refs, N, C, None, quorum.data_ptr(), cls.data_ptr(), 0, 0, counts.data_ptr(), 0, st)
        return run

    cases = {"c_stripe_magic_dev": stripe_magic}
    cases.update({c: scan(*f) for c, f in FORMS.items()})
    for c in FORMS:
        cls.fill_(0x7B)
        cases[c]()
        torch.cuda.synchronize()
        assert counts.tolist() == [0, 0, N, 0, 0] and set(cls.tolist()) == {E.VOTE_BLANK}, c
    arena[n - 1, N - 1, C - 1] = 1  # one nonzero byte, the very last: that stripe alone is demoted
    cases["d_nt_2"]()
    torch.cuda.synchronize()
    assert counts.tolist() == [1, 0, N - 1, 0, 0] and cls[N - 1].item() == E.VOTE_OK
    arena[n - 1, N - 1, C - 1] = 0
    for _ in range(WARM):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {c: [] for c in cases}
    for _ in range(REPS):
        for c, fn in cases.items():
            ms[c].append(device_timed(fn))
    E.set_vote_form()  # back to the form that ships
    for c in cases:
        report(c, ms, "c_stripe_magic_dev", part="scan", code="rs63", C=C,
               read_TB_s=round(n * N * C / statistics.median(ms[c]) / 1e9, 3))
