#!/usr/bin/env python3
"""Kernel A/B bench (development tool): interleaved rounds of encode/decode per kernel variant.

python tools/kbench.py [--stripes N] [--rounds R] [--configs rs63,cg104,cg63,cg:K:M:C_KiB,...]
Prints HBM GB/s (algorithmic bytes / launch time, HIP events on the launch stream).

python tools/kbench.py --patterns [--nine] [--rounds R] [--reps N]
The per-stripe-pattern decodes against the single-pattern decode, interleaved on the same buffers
(RS(6+3) and Cauchy-good(6+3), C = 1 MiB, 4095 stripes): see patterns_bench.

python tools/kbench.py --check [--rounds R] [--reps N]
lsec_check_dev against lsec_encode_dev and against encode-and-compare, on the same shapes: see check_bench.

python tools/kbench.py --locate [--rounds R] [--reps N]
lsec_locate_dev against lsec_check_dev on the same shapes, clean, corrupt and repairing: see locate_bench.

python tools/kbench.py --update [--rounds R] [--reps N] [--pattern-codes rs63,rs164,cg63]
lsec_update_dev against a device copy of the fresh chunk followed by lsec_encode_dev: see update_bench.

python tools/kbench.py --update-masked [--rounds R] [--reps N] [--pattern-codes rs63,rs164,cg63]
lsec_update_dev_masked against lsec_update_dev and the per-class calls it replaces: see update_masked_bench.

python tools/kbench.py --update-magic [--rounds R] [--reps N] [--pattern-codes rs63,cg63]
lsec_update_magic_dev_masked against lsec_update_dev_masked alone and followed by lsec_stripe_magic_dev, which is
what keeping the magics current costs without it: see update_magic_bench.

python tools/kbench.py --rotated-scrub [--rounds R] [--reps N]
lsec_check_dev_rotated / lsec_locate_dev_rotated over the devices of a rotated LUN against the unrotated
calls over the same bytes: see rotated_scrub_bench.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import lstore_amd as L  # noqa: E402
from lstore_amd import erasure as E  # noqa: E402

CONFIGS = {
    "rs63": (L.REED_SOL_VAN, 6, 3, 1 << 20),
    "rs104": (L.REED_SOL_VAN, 10, 4, 1 << 20),
    "cg63": (L.CAUCHY_GOOD, 6, 3, 1 << 20),
    "cg104": (L.CAUCHY_GOOD, 10, 4, 4 << 20),
    "rs206": (L.REED_SOL_VAN, 20, 6, 256 << 10),
    "rs128": (L.REED_SOL_VAN, 12, 8, 512 << 10),
    "rs166": (L.REED_SOL_VAN, 16, 6, 512 << 10),
    "rs248": (L.REED_SOL_VAN, 24, 8, 256 << 10),
    "rs104c4": (L.REED_SOL_VAN, 10, 4, 4 << 20),
    "rs104c8": (L.REED_SOL_VAN, 10, 4, 8 << 20),
    "cg104s": (L.CAUCHY_GOOD, 10, 4, 256 << 10),
    "cg104m": (L.CAUCHY_GOOD, 10, 4, 512 << 10),
    "cg104l": (L.CAUCHY_GOOD, 10, 4, 2 << 20),
    "cg164c8": (L.CAUCHY_GOOD, 16, 4, 8 << 20),
    "cg164c1": (L.CAUCHY_GOOD, 16, 4, 1 << 20),
    "rs84c4": (L.REED_SOL_VAN, 8, 4, 4 << 20),
    "cg206c4": (L.CAUCHY_GOOD, 20, 6, 4 << 20),
    "cg42c4": (L.CAUCHY_GOOD, 4, 2, 4 << 20),
    "rs83c8": (L.REED_SOL_VAN, 8, 3, 8 << 20),
    "rs164c8": (L.REED_SOL_VAN, 16, 4, 8 << 20),
    "rs63c8": (L.REED_SOL_VAN, 6, 3, 8 << 20),
    "cg206c1": (L.CAUCHY_GOOD, 20, 6, 1 << 20),
    "cg206c8": (L.CAUCHY_GOOD, 20, 6, 8 << 20),
    "cg124c4": (L.CAUCHY_GOOD, 12, 4, 4 << 20),
    "cg124c8": (L.CAUCHY_GOOD, 12, 4, 8 << 20),
    "rs164": (L.REED_SOL_VAN, 16, 4, 1 << 20),
    "rs124": (L.REED_SOL_VAN, 12, 4, 1 << 20),
    "rs84": (L.REED_SOL_VAN, 8, 4, 1 << 20),
    "cg206": (L.CAUCHY_GOOD, 20, 6, 256 << 10),
    # the c5 points under 0.70 in round 4 (r04_v15_sweep_c5.jsonl)
    "rs84c8": (L.REED_SOL_VAN, 8, 4, 8 << 20),
    "rs124c4": (L.REED_SOL_VAN, 12, 4, 4 << 20),
    "cg206c2": (L.CAUCHY_GOOD, 20, 6, 2 << 20),
    # wide fields (w = 16 / 32): transposed bit-sliced RS, bit-sliced Cauchy
    "rs63w16": (L.REED_SOL_VAN, 6, 3, 1 << 20, 16),
    "rs63w32": (L.REED_SOL_VAN, 6, 3, 1 << 20, 32),
    "rs104w16": (L.REED_SOL_VAN, 10, 4, 1 << 20, 16),
    "rs104w32": (L.REED_SOL_VAN, 10, 4, 1 << 20, 32),
    "rs106w32": (L.REED_SOL_VAN, 10, 6, 1 << 20, 32),
    "rs105w32": (L.REED_SOL_VAN, 10, 5, 1 << 20, 32),
    "rs206w16": (L.REED_SOL_VAN, 20, 6, 256 << 10, 16),
    "rs208w16": (L.REED_SOL_VAN, 20, 8, 256 << 10, 16),
    "rs165w16": (L.REED_SOL_VAN, 16, 5, 1 << 20, 16),
    "cg63w16": (L.CAUCHY_GOOD, 6, 3, 1 << 20, 16),
    "cg104w16": (L.CAUCHY_GOOD, 10, 4, 1 << 20, 16),
    "cg104w32": (L.CAUCHY_GOOD, 10, 4, 1 << 20, 32),
    # bitmatrix codes (K3): liberation w = 7, Blaum-Roth w = 6, liber8tion w = 8, raid4, r6
    "lib62": (L.LIBERATION, 6, 2, 7 << 17, 7),
    "br62": (L.BLAUM_ROTH, 6, 2, 6 << 17, 6),
    "l8t62": (L.LIBER8TION, 6, 2, 1 << 20, 8),
    "raid4_6": (L.RAID4, 6, 1, 1 << 20),
    "r6_62": (L.REED_SOL_R6_OP, 6, 2, 1 << 20),
    "cg63w32": (L.CAUCHY_GOOD, 6, 3, 1 << 20, 32),
}


def patterns_bench(a):
    """Degraded decodes four ways, interleaved round by round on the same k+m buffers (one per
    chunk / device, C = 1 MiB; rebuilt chunks go to scratch buffers, so the inputs stay as they are):
      (a) lsec_decode_dev, erasures --pattern-lost ([0])    the yardstick: code the patterned calls do not touch
      (b) lsec_decode_dev_patterns, every stripe on that    (a)'s traffic: isolates the table indirection
          one pattern
      (c) lsec_decode_dev_rotated, device 0 lost, n_shift 1 the rotated degraded read: k+m patterns in turn
      (d) --nine: k+m whole-stage lsec_decode_dev launches, one per rotation: (c)'s cost without the call
    (a)'s own min-max over the rounds is the margin (b) and (c) are judged by (with the default
    --pattern-lost; (c) always rebuilds one chunk per stripe).  Results are checked before timing."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    C, N = 1 << 20, a.pattern_stripes
    lost = sorted({int(x) for x in a.pattern_lost.split(",")})  # (a) and (b): these logical chunks; (c), (d): device 0
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        outs = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in lost]
        out, out2 = outs[0], torch.empty((N, C), dtype=torch.uint8, device=dev)
        refs = [(b.data_ptr(), C) for b in bufs]
        plan.encode_dev_refs(refs, N, C, stream.cuda_stream)  # consistent parity in buffers k..n-1
        into = lambda o: [(o.data_ptr(), C)] + refs[1:]  # shard / device 0 is the lost one
        scratch = list(refs)  # the lost chunks' refs point at the scratch outputs
        for o, e in zip(outs, lost):
            scratch[e] = (o.data_ptr(), C)
        ids = torch.zeros(N, dtype=torch.uint8, device=dev)
        sh = stream.cuda_stream
        plan.prepare_decode(lost)
        plan.decode_dev_patterns_refs(refs, 0, C, [lost], 0)
        plan.decode_dev_rotated_refs(refs, 0, C, [0], 1, 0)

        def nine(o):
            for rot in range(n):  # logical chunk c of a rotation-rot stripe is on device (c - rot) mod n
                plan.decode_dev_refs([into(o)[(c - rot) % n] for c in range(n)], N, C, [rot], sh)

        runs = {"a": lambda: plan.decode_dev_refs(scratch, N, C, lost, sh),
                "b": lambda: plan.decode_dev_patterns_refs(scratch, N, C, [lost], ids.data_ptr(), sh),
                "c": lambda: plan.decode_dev_rotated_refs(into(out), N, C, [0], 1, 0, sh)}
        if a.nine:
            runs["d"] = lambda: nine(out2)
        # results first: (a) rebuilds the lost chunks, (b) writes the same bytes, (c) equals per-rotation decodes
        for key in "ab":
            for o in outs:
                o.zero_()
            runs[key]()
            torch.cuda.synchronize()
            for o, e in zip(outs, lost):
                assert torch.equal(o, bufs[e]), f"({key}) did not rebuild chunk {e}"
        runs["c"]()
        torch.cuda.synchronize()
        for rot in range(n):
            plan.decode_dev_refs([into(out2)[(c - rot) % n] for c in range(n)], N, C, [rot], sh)
            torch.cuda.synchronize()
            assert torch.equal(out[rot::n], out2[rot::n]), f"(c) differs from lsec_decode_dev at rotation {rot}"
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        lo, hi = min(times["a"]), max(times["a"])
        what = {"a": f"lsec_decode_dev {lost}", "b": f"patterns, all stripes {lost}", "c": "rotated, 1 lost, n_shift 1",
                "d": f"{n} whole-stage lsec_decode_dev"}
        for key, ts in times.items():
            med = sorted(ts)[len(ts) // 2]
            db = (k + (len(lost) if key in "ab" else 1)) * C * N  # bytes the stripes' decodes have to move
            band = "" if key in "ad" else ("  inside (a)'s band" if lo <= med <= hi else
                                          f"  {'below' if med < lo else 'above'} (a)'s band by {abs(med - (lo if med < lo else hi)) / med:.2%}")
            print(f"{name} N={N} C={C} ({key}) {what[key]:34s} median {med:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{db / med / 1e6:7.1f} GB/s ({db / med / 8e9:5.1%} of 8 TB/s){band}", flush=True)
        print(f"{name} (a) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches", flush=True)
        del bufs, outs, out, out2, ids
        plan.close()
        torch.cuda.empty_cache()


def check_bench(a):
    """The parity check four ways, interleaved round by round on the same k+m buffers (one per chunk,
    C = 1 MiB; nothing timed writes into them):
      (a) lsec_encode_dev into scratch parity           the yardstick: the same k+m chunks of traffic, in
                                                        code the check does not touch
      (b) lsec_check_dev on consistent stripes          k+m reads, no writes past the memset
      (c) lsec_check_dev, every byte of data chunk 0    every wave publishes: the atomics' worst case
          of every stripe corrupted
      (d) lsec_encode_dev into scratch parity + a       what a device caller does without the call
          per-stripe torch comparison with the stored
    (a)'s own min-max over the rounds is the margin (b) is judged by.  Results are checked before timing."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        scratch = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in range(m)]
        refs = [(b.data_ptr(), C) for b in bufs]
        plan.encode_dev_refs(refs, N, C, sh)  # consistent parity in buffers k..n-1
        bad0 = bufs[0] ^ 0xFF  # every byte of data chunk 0 differs
        bad_refs = [(bad0.data_ptr(), C)] + refs[1:]
        to_scratch = lambda r: r[:k] + [(s.data_ptr(), C) for s in scratch]
        syn = torch.full((N,), -1, dtype=torch.int32, device=dev)
        count = torch.full((1,), -1, dtype=torch.int32, device=dev)

        def compare(r):  # (d): the syndrome words by encode-and-compare
            plan.encode_dev_refs(to_scratch(r), N, C, sh)
            out = torch.zeros(N, dtype=torch.int32, device=dev)
            for i in range(m):
                out |= (scratch[i] != bufs[k + i]).any(dim=1).to(torch.int32) << i
            return out

        runs = {"a": lambda: plan.encode_dev_refs(to_scratch(refs), N, C, sh),
                "b": lambda: plan.check_dev_refs(refs, N, C, syn.data_ptr(), count.data_ptr(), sh),
                "c": lambda: plan.check_dev_refs(bad_refs, N, C, syn.data_ptr(), count.data_ptr(), sh),
                "d": lambda: compare(refs)}
        # results first
        runs["b"]()
        torch.cuda.synchronize()
        assert int(syn.count_nonzero()) == 0 and int(count) == 0, "(b) found a difference in consistent stripes"
        want = compare(bad_refs)
        runs["c"]()
        torch.cuda.synchronize()
        assert int(want.min()) > 0 and torch.equal(syn, want) and int(count) == N, "(c) differs from encode-and-compare"
        assert int(compare(refs).count_nonzero()) == 0
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        lo, hi = min(times["a"]), max(times["a"])
        what = {"a": "lsec_encode_dev", "b": "lsec_check_dev, consistent", "c": "lsec_check_dev, all corrupt",
                "d": "encode + torch compare"}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = n * C * N  # the k+m chunks a check has to move
            band = "" if key != "b" else ("  inside (a)'s band" if lo <= med[key] <= hi else
                                          f"  {'below' if med[key] < lo else 'above'} (a)'s band by "
                                          f"{abs(med[key] - (lo if med[key] < lo else hi)) / med[key]:.2%}")
            print(f"{name} N={N} C={C} ({key}) {what[key]:28s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s){band}", flush=True)
        print(f"{name} (a) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches; "
              f"(b)/(d) = {med['b'] / med['d']:.3f}, (c)/(b) = {med['c'] / med['b']:.3f}", flush=True)
        del bufs, scratch, bad0, syn, count, want
        plan.close()
        torch.cuda.empty_cache()


def locate_bench(a):
    """The locate five ways, interleaved round by round on the same k+m buffers (one per chunk, C = 1 MiB):
      (a) lsec_check_dev on consistent stripes          the yardstick: the pass the locate kernels share
      (b) lsec_locate_dev on consistent stripes         (a) plus the two extra memsets and the finalize launch
      (c) lsec_locate_dev, every byte of data chunk 0   every wave takes the slow path and publishes
          of every stripe corrupted
      (d) lsec_locate_dev with repair, one byte of a    the scrub: each launch is preceded by the torch op that
          data chunk corrupt in 1 % of the stripes      corrupts those bytes again (inside the timed window)
      (e) lsec_locate_dev at block_size 0               the memsets and the finalize launch alone
    (a)'s own min-max over the rounds is the margin (b) is judged by, widened by (e).  Results are checked
    before timing."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        refs = [(b.data_ptr(), C) for b in bufs]
        plan.encode_dev_refs(refs, N, C, sh)  # consistent parity in buffers k..n-1
        bad0 = bufs[0] ^ 0xFF  # every byte of data chunk 0 differs
        bad_refs = [(bad0.data_ptr(), C)] + refs[1:]
        syn = torch.full((N,), -1, dtype=torch.int32, device=dev)
        hyp = torch.full((N,), -1, dtype=torch.int64, device=dev)
        loc = torch.full((N,), 0x7B, dtype=torch.uint8, device=dev)
        counts = torch.full((2,), -1, dtype=torch.int32, device=dev)
        one = torch.full((1,), -1, dtype=torch.int32, device=dev)
        hit = torch.arange(0, N, 100, device=dev)  # 1 % of the stripes
        jd, col = k // 2, 4097
        good = bufs[jd][hit, col].clone()
        outs = (syn.data_ptr(), hyp.data_ptr(), loc.data_ptr(), counts.data_ptr())

        def scrub():
            bufs[jd][hit, col] = good ^ 0x5A
            plan.locate_dev_refs(refs, N, C, *outs, True, sh)

        runs = {"a": lambda: plan.check_dev_refs(refs, N, C, syn.data_ptr(), one.data_ptr(), sh),
                "b": lambda: plan.locate_dev_refs(refs, N, C, *outs, False, sh),
                "c": lambda: plan.locate_dev_refs(bad_refs, N, C, *outs, False, sh),
                "d": scrub,
                "e": lambda: plan.locate_dev_refs(refs, N, 0, *outs, False, sh)}
        # results first
        full = (1 << k) - 1
        runs["b"]()
        torch.cuda.synchronize()
        assert int(syn.count_nonzero()) == 0 and bool((hyp == full).all()) and bool((loc == E.LOCATE_CLEAN).all()) \
            and counts.tolist() == [0, 0], "(b) found a difference in consistent stripes"
        runs["c"]()
        torch.cuda.synchronize()
        assert bool((syn == (1 << m) - 1).all()) and bool((hyp == 1).all()) and bool((loc == 0).all()) \
            and counts.tolist() == [N, 0], "(c) did not locate chunk 0 everywhere"
        runs["d"]()
        torch.cuda.synchronize()
        assert int(loc[hit].ne(jd).sum()) == 0 and counts.tolist() == [hit.numel(), 0] \
            and torch.equal(bufs[jd][hit, col], good), "(d) did not repair"
        runs["a"]()
        torch.cuda.synchronize()
        assert int(syn.count_nonzero()) == 0 and int(one) == 0, "(d) left an inconsistent stripe"
        runs["e"]()
        torch.cuda.synchronize()
        assert bool((loc == E.LOCATE_CLEAN).all()) and bool((hyp == full).all())
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        lo, hi = min(times["a"]), max(times["a"])
        what = {"a": "lsec_check_dev, consistent", "b": "lsec_locate_dev, consistent", "c": "lsec_locate_dev, all corrupt",
                "d": "corrupt 1 % + locate + repair", "e": "memsets + finalize alone"}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = n * C * N  # the k+m chunks a pass has to move
            band = ""
            if key == "b":
                top = hi + med["e"]
                band = ("  inside (a)'s band + (e)" if lo <= med[key] <= top else
                        f"  {'below' if med[key] < lo else 'above'} (a)'s band + (e) by "
                        f"{abs(med[key] - (lo if med[key] < lo else top)) / med[key]:.2%}")
            rate = "" if key == "e" else f"  {db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s)"
            print(f"{name} N={N} C={C} ({key}) {what[key]:30s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}"
                  f"{rate}{band}", flush=True)
        print(f"{name} (a) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches; "
              f"(b) - (a) = {med['b'] - med['a']:+.3f} ms, (c)/(b) = {med['c'] / med['b']:.3f}, (d)/(b) = {med['d'] / med['b']:.3f}",
              flush=True)
        del bufs, bad0, syn, hyp, loc, counts
        plan.close()
        torch.cuda.empty_cache()


def rotated_scrub_bench(a):
    """The scrub of a rotated LUN against the unrotated calls, interleaved round by round (C = 1 MiB).  One
    set of k+m buffers holds consistent logical stripes, a second one the same bytes as the devices of a LUN
    with n_shift = 1 hold them (device i: logical chunk (i + first_stripe + s) mod n of stripe s):
      (a) lsec_check_dev on the logical stripes         the yardstick of (b): code the rotated calls do not touch
      (b) lsec_check_dev_rotated on the devices         (a) plus the rotation's scalar work per tile
      (c) lsec_locate_dev on the logical stripes        the yardstick of (d)
      (d) lsec_locate_dev_rotated on the devices
      (e) lsec_locate_dev_rotated with repair, one      each launch is preceded by the torch op that corrupts those
          byte of one device corrupt in every stripe    bytes again (inside the timed window); k+m chunks to locate
      (f) lsec_locate_dev with repair, one byte of      (e)'s yardstick: one chunk to locate
          one chunk corrupt in every stripe
    (a)'s and (c)'s own min-max over the rounds are the margins (b) and (d) are judged by.  Results are checked
    before timing."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    n_shift, first = 1, 3_000_000_007
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        refs = [(b.data_ptr(), C) for b in bufs]
        plan.encode_dev_refs(refs, N, C, sh)  # consistent parity in buffers k..n-1
        rots = (first + torch.arange(N, device=dev)) * n_shift % n
        devs = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        for r in range(n):
            rows = torch.nonzero(rots == r).flatten()
            for i in range(n):
                devs[i][rows] = bufs[(i + r) % n][rows]
        dev_refs = [(b.data_ptr(), C) for b in devs]
        syn = torch.full((N,), -1, dtype=torch.int32, device=dev)
        hyp = torch.full((N,), -1, dtype=torch.int64, device=dev)
        loc = torch.full((N,), 0x7B, dtype=torch.uint8, device=dev)
        loc_dev = torch.full((N,), 0x7B, dtype=torch.uint8, device=dev)
        counts = torch.full((2,), -1, dtype=torch.int32, device=dev)
        faults = torch.full((n,), -1, dtype=torch.int32, device=dev)
        one = torch.full((1,), -1, dtype=torch.int32, device=dev)
        jd, col = k // 2, 4097
        good, good_dev = bufs[jd][:, col].clone(), devs[jd][:, col].clone()
        outs = (syn.data_ptr(), hyp.data_ptr(), loc.data_ptr())
        rot_outs = outs + (loc_dev.data_ptr(), counts.data_ptr(), faults.data_ptr())

        def scrub_rotated():
            devs[jd][:, col] = good_dev ^ 0x5A
            plan.locate_dev_rotated_refs(dev_refs, N, C, n_shift, first, *rot_outs, True, sh)

        def scrub():
            bufs[jd][:, col] = good ^ 0x5A
            plan.locate_dev_refs(refs, N, C, *outs, counts.data_ptr(), True, sh)

        runs = {"a": lambda: plan.check_dev_refs(refs, N, C, syn.data_ptr(), one.data_ptr(), sh),
                "b": lambda: plan.check_dev_rotated_refs(dev_refs, N, C, n_shift, first, syn.data_ptr(), one.data_ptr(), sh),
                "c": lambda: plan.locate_dev_refs(refs, N, C, *outs, counts.data_ptr(), False, sh),
                "d": lambda: plan.locate_dev_rotated_refs(dev_refs, N, C, n_shift, first, *rot_outs, False, sh),
                "e": scrub_rotated,
                "f": scrub}
        # results first
        full = (1 << k) - 1
        for key in ("a", "b"):
            runs[key]()
            torch.cuda.synchronize()
            assert int(syn.count_nonzero()) == 0 and int(one) == 0, f"({key}) found a difference in consistent stripes"
        for key in ("c", "d"):
            runs[key]()
            torch.cuda.synchronize()
            assert int(syn.count_nonzero()) == 0 and bool((hyp == full).all()) and bool((loc == E.LOCATE_CLEAN).all()) \
                and counts.tolist() == [0, 0], f"({key}) found a difference in consistent stripes"
        assert bool((loc_dev == E.LOCATE_CLEAN).all()) and faults.tolist() == [0] * n
        runs["e"]()
        torch.cuda.synchronize()
        assert torch.equal(loc.to(torch.int64), (jd + rots) % n) and bool((loc_dev == jd).all()) and counts.tolist() == [N, 0] \
            and faults.tolist() == [N if i == jd else 0 for i in range(n)] and torch.equal(devs[jd][:, col], good_dev), \
            "(e) did not locate and repair device %d" % jd
        runs["b"]()
        torch.cuda.synchronize()
        assert int(syn.count_nonzero()) == 0 and int(one) == 0, "(e) left an inconsistent stripe"
        runs["f"]()
        torch.cuda.synchronize()
        assert bool((loc == jd).all()) and counts.tolist() == [N, 0] and torch.equal(bufs[jd][:, col], good), "(f) did not repair"
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        what = {"a": "lsec_check_dev", "b": "lsec_check_dev_rotated", "c": "lsec_locate_dev", "d": "lsec_locate_dev_rotated",
                "e": "corrupt + rotated locate + repair", "f": "corrupt + locate + repair"}
        twin = {"b": "a", "d": "c"}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = n * C * N  # the k+m chunks a pass has to move
            band = ""
            if key in twin:
                lo, hi = min(times[twin[key]]), max(times[twin[key]])
                band = (f"  inside ({twin[key]})'s band" if lo <= med[key] <= hi else
                        f"  {'below' if med[key] < lo else 'above'} ({twin[key]})'s band by "
                        f"{abs(med[key] - (lo if med[key] < lo else hi)) / med[key]:.2%}")
            print(f"{name} N={N} C={C} ({key}) {what[key]:34s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s){band}", flush=True)
        for key in ("a", "c"):
            lo, hi = min(times[key]), max(times[key])
            print(f"{name} ({key}) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches",
                  flush=True)
        print(f"{name} (b)/(a) = {med['b'] / med['a']:.3f}, (d)/(c) = {med['d'] / med['c']:.3f}, (e)/(f) = {med['e'] / med['f']:.3f}",
              flush=True)
        del bufs, devs, syn, hyp, loc, loc_dev, counts, faults
        plan.close()
        torch.cuda.empty_cache()


def update_bench(a):
    """The partial-stripe write four ways, interleaved round by round on the same k+m buffers (one per
    chunk, C = 1 MiB) and two buffers of fresh bytes:
      (a) a device copy of the fresh chunk over data chunk 0,  what a device caller does without the call: c + k
          then lsec_encode_dev                                 chunk reads and c + m chunk writes
      (b) lsec_update_dev, LSEC_UPDATE_STORE, cols = {0}       2c + m reads, m + c writes
      (c) lsec_update_dev without the flag, cols = {0}         2c + m reads, m writes
      (d) lsec_update_dev, LSEC_UPDATE_STORE, cols = {0, k-1}  c = 2
    (a)'s own min-max over the rounds is the margin (b) is judged by.  Every case is checked before timing: the
    parity after (b), (c) and (d) is lsec_encode_dev's for the data with the chunks replaced."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        fresh = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(2)]
        refs = [(b.data_ptr(), C) for b in bufs]
        fresh_refs = [(f.data_ptr(), C) for f in fresh]
        # the untouched data chunks are not handed to the update at all
        only = lambda cols: [refs[i] if i in cols or i >= k else (0, 0) for i in range(n)]
        one, two = only((0,)), only((0, k - 1))

        def copy_encode():
            bufs[0].copy_(fresh[0])
            plan.encode_dev_refs(refs, N, C, sh)

        runs = {"a": copy_encode,
                "b": lambda: plan.update_dev_refs(one, N, C, [0], fresh_refs[:1], True, sh),
                "c": lambda: plan.update_dev_refs(one, N, C, [0], fresh_refs[:1], False, sh),
                "d": lambda: plan.update_dev_refs(two, N, C, [0, k - 1], fresh_refs, True, sh)}
        # results first: each update against a re-encode of the data with the chunks replaced
        want = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in range(m)]
        for key, cols in (("b", (0,)), ("c", (0,)), ("d", (0, k - 1))):
            old = {j: bufs[j].clone() for j in cols}
            plan.encode_dev_refs(refs, N, C, sh)  # consistent stripes
            runs[key]()
            torch.cuda.synchronize()
            for i, j in enumerate(cols):
                assert torch.equal(bufs[j], fresh[i] if key != "c" else old[j]), f"({key}) data chunk {j}"
                bufs[j].copy_(fresh[i])
            plan.encode_dev_refs(refs[:k] + [(w.data_ptr(), C) for w in want], N, C, sh)
            torch.cuda.synchronize()
            for r in range(m):
                assert torch.equal(bufs[k + r], want[r]), f"({key}) parity row {r} differs from the re-encode"
            for j in cols:
                bufs[j].copy_(old[j])
            del old
        del want
        torch.cuda.empty_cache()
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        lo, hi = min(times["a"]), max(times["a"])
        what = {"a": "copy + lsec_encode_dev", "b": "lsec_update_dev, store, c = 1", "c": "lsec_update_dev, c = 1",
                "d": "lsec_update_dev, store, c = 2"}
        chunks = {"a": 1 + k + 1 + m, "b": 2 + m + m + 1, "c": 2 + m + m, "d": 4 + m + m + 2}  # chunk transfers per stripe
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = chunks[key] * C * N
            band = "" if key != "b" else ("  inside (a)'s band" if lo <= med[key] <= hi else
                                          f"  {'below' if med[key] < lo else 'above'} (a)'s band by "
                                          f"{abs(med[key] - (lo if med[key] < lo else hi)) / med[key]:.2%}")
            print(f"{name} N={N} C={C} ({key}) {what[key]:30s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{chunks[key]:2d} chunks {db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s){band}", flush=True)
        print(f"{name} (a) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches; "
              f"(b)/(a) = {med['b'] / med['a']:.3f}, (c)/(b) = {med['c'] / med['b']:.3f}, (d)/(b) = {med['d'] / med['b']:.3f}", flush=True)
        del bufs, fresh
        plan.close()
        torch.cuda.empty_cache()


def update_masked_bench(a):
    """The per-stripe-mask update beside lsec_update_dev, interleaved round by round on the same k+m buffers (one
    per chunk, C = 1 MiB) and two buffers of fresh bytes that the k fresh refs alternate between:
      (a) lsec_update_dev, LSEC_UPDATE_STORE, cols = {0}              its own min-max over the rounds is the band
      (b) lsec_update_dev_masked, the same single bit in every stripe the cost of the per-tile mask read
      (c) lsec_update_dev_masked, masks 1 << (s mod k), one launch    a different chunk in every stripe
      (d) what a caller does today for (c): k lsec_update_dev calls over stride-stretched refs
      (e) lsec_update_dev_masked, bit 0 in 1 % of the stripes         the cost of visiting tiles only to skip them
    All with the store flag.  Every case is checked before timing: the data chunks named by the masks hold the fresh
    bytes and the parity is lsec_encode_dev's for the data as it then stands."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        fresh = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(2)]
        refs = [(b.data_ptr(), C) for b in bufs]
        fresh_refs = [(fresh[j % 2].data_ptr(), C) for j in range(k)]
        one = [refs[i] if i == 0 or i >= k else (0, 0) for i in range(n)]
        s_idx = torch.arange(N, dtype=torch.int64, device=dev)
        masks = {"b": torch.ones(N, dtype=torch.int64, device=dev),
                 "c": torch.ones(N, dtype=torch.int64, device=dev) << (s_idx % k),
                 "e": (s_idx % 100 == 0).to(torch.int64)}

        def classes():
            for j in range(k):  # the stripes s = j mod k: chunk j changes
                cnt = (N - j + k - 1) // k
                if cnt > 0:
                    cls = [(refs[i][0] + j * C, k * C) if i == j or i >= k else (0, 0) for i in range(n)]
                    plan.update_dev_refs(cls, cnt, C, [j], [(fresh_refs[j][0] + j * C, k * C)], True, sh)

        runs = {"a": lambda: plan.update_dev_refs(one, N, C, [0], fresh_refs[:1], True, sh),
                "b": lambda: plan.update_dev_masked_refs(refs, N, C, masks["b"].data_ptr(), fresh_refs, True, sh),
                "c": lambda: plan.update_dev_masked_refs(refs, N, C, masks["c"].data_ptr(), fresh_refs, True, sh),
                "d": classes,
                "e": lambda: plan.update_dev_masked_refs(refs, N, C, masks["e"].data_ptr(), fresh_refs, True, sh)}
        # results first: the changed chunks hold the fresh bytes, the parity is the re-encode's
        want = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in range(m)]
        for key in runs:
            for b in bufs[:k]:
                b.add_(1)  # old bytes that differ from the fresh ones again (five cases: no byte comes back round)
            plan.encode_dev_refs(refs, N, C, sh)  # consistent stripes
            runs[key]()
            torch.cuda.synchronize()
            word = masks["c" if key == "d" else "b" if key == "a" else key]
            for j in range(k):
                hit = (word >> j & 1).bool()
                assert torch.equal(bufs[j][hit], fresh[j % 2][hit]), f"({key}) data chunk {j}"
                if not hit.all():  # every stripe outside the mask still differs from the fresh bytes
                    assert (bufs[j][~hit] != fresh[j % 2][~hit]).any(dim=1).all(), f"({key}) data chunk {j} was stored"
            plan.encode_dev_refs(refs[:k] + [(w.data_ptr(), C) for w in want], N, C, sh)
            torch.cuda.synchronize()
            for r in range(m):
                assert torch.equal(bufs[k + r], want[r]), f"({key}) parity row {r} differs from the re-encode"
        del want
        torch.cuda.empty_cache()
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        lo, hi = min(times["a"]), max(times["a"])
        what = {"a": "lsec_update_dev, store, c = 1", "b": "masked, bit 0 in every stripe", "c": "masked, 1 << (s mod k)",
                "d": f"{k} lsec_update_dev calls for (c)", "e": "masked, bit 0 in 1 % of stripes"}
        per = 2 + m + m + 1  # chunk transfers of a stripe that changes in one chunk
        touched = {key: N for key in runs}
        touched["e"] = int(masks["e"].sum().item())
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = per * C * touched[key]
            band = "" if key == "a" else ("  inside (a)'s band" if lo <= med[key] <= hi else
                                          f"  {'below' if med[key] < lo else 'above'} (a)'s band by "
                                          f"{abs(med[key] - (lo if med[key] < lo else hi)) / med[key]:.2%}")
            print(f"{name} N={N} C={C} ({key}) {what[key]:32s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{touched[key]:5d} stripes {db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s){band}", flush=True)
        print(f"{name} (a) band: {lo:.3f} .. {hi:.3f} ms ({(hi - lo) / lo:.2%}) over {a.rounds} rounds of {a.reps} launches; "
              f"(b)/(a) = {med['b'] / med['a']:.3f}, (c)/(a) = {med['c'] / med['a']:.3f}, (d)/(c) = {med['d'] / med['c']:.3f}, "
              f"(e)/(a) = {med['e'] / med['a']:.3f}", flush=True)
        del bufs, fresh, masks
        plan.close()
        torch.cuda.empty_cache()


def update_magic_bench(a):
    """The masked update that keeps the stripe magics beside what a caller does without it, interleaved round by
    round in one process on the same k+m buffers (one per chunk, C = 1 MiB), one changed chunk per stripe (masks
    1 << (s mod k)), LSEC_UPDATE_STORE:
      (a) lsec_update_dev_masked                                        the update alone; its min-max is the band
      (b) (a), then lsec_stripe_magic_dev over the k+m chunks           what a caller does today for the new magics
      (c) lsec_update_magic_dev_masked                                  the new call
    Chunk-sized units moved per stripe with c changed chunks: (a) (2c+m)+(m+c), (b) that + (k+m), (c) as (a).
    Every case is checked before timing: the parity is lsec_encode_dev's for the data as it then stands, and the
    magics (c) leaves, entered as lsec_stripe_magic_dev's of the old stripes, are lsec_stripe_magic_dev's of the new."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    C, N = 1 << 20, a.pattern_stripes
    for name in a.pattern_codes.split(","):
        meth, k, m = CONFIGS[name][:3]
        n = k + m
        plan = L.Plan.for_chunk(meth, k, m, C)
        bufs = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(n)]
        fresh = [torch.randint(0, 256, (N, C), dtype=torch.uint8, device=dev) for _ in range(2)]
        refs = [(b.data_ptr(), C) for b in bufs]
        fresh_refs = [(fresh[j % 2].data_ptr(), C) for j in range(k)]
        s_idx = torch.arange(N, dtype=torch.int64, device=dev)
        mask = torch.ones(N, dtype=torch.int64, device=dev) << (s_idx % k)
        magic = torch.zeros((N, 4), dtype=torch.uint8, device=dev)
        magic_b = torch.zeros((N, 4), dtype=torch.uint8, device=dev)

        def today():
            plan.update_dev_masked_refs(refs, N, C, mask.data_ptr(), fresh_refs, True, sh)
            plan.stripe_magic_dev_refs(refs, N, C, magic_b.data_ptr(), sh)

        runs = {"a": lambda: plan.update_dev_masked_refs(refs, N, C, mask.data_ptr(), fresh_refs, True, sh),
                "b": today,
                "c": lambda: plan.update_magic_dev_masked_refs(refs, N, C, mask.data_ptr(), fresh_refs, magic.data_ptr(), True, sh)}
        want = [torch.empty((N, C), dtype=torch.uint8, device=dev) for _ in range(m)]
        for key in runs:
            for b in bufs[:k]:
                b.add_(1)  # old bytes that differ from the fresh ones again
            plan.encode_dev_refs(refs, N, C, sh)  # consistent stripes
            plan.stripe_magic_dev_refs(refs, N, C, magic.data_ptr(), sh)  # and their magics
            runs[key]()
            torch.cuda.synchronize()
            for j in range(k):
                hit = (mask >> j & 1).bool()
                assert torch.equal(bufs[j][hit], fresh[j % 2][hit]), f"({key}) data chunk {j}"
            plan.encode_dev_refs(refs[:k] + [(w.data_ptr(), C) for w in want], N, C, sh)
            torch.cuda.synchronize()
            for r in range(m):
                assert torch.equal(bufs[k + r], want[r]), f"({key}) parity row {r} differs from the re-encode"
            if key == "c":
                plan.stripe_magic_dev_refs(refs, N, C, magic_b.data_ptr(), sh)
                torch.cuda.synchronize()
                assert torch.equal(magic, magic_b), "(c) the magics differ from lsec_stripe_magic_dev's over the new stripes"
        del want
        torch.cuda.empty_cache()
        times = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, fn in runs.items():
                fn()  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / a.reps)
        what = {"a": "lsec_update_dev_masked", "b": "(a) + lsec_stripe_magic_dev", "c": "lsec_update_magic_dev_masked"}
        units = {"a": 2 + m + m + 1, "b": 2 + m + m + 1 + n, "c": 2 + m + m + 1}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
        for key, ts in times.items():
            db = units[key] * C * N
            print(f"{name} N={N} C={C} ({key}) {what[key]:30s} median {med[key]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
                  f"{units[key]:2d} chunks per stripe {db / med[key] / 1e6:7.1f} GB/s ({db / med[key] / 8e9:5.1%} of 8 TB/s)", flush=True)
        print(f"{name} over {a.rounds} rounds of {a.reps} launches: (c)/(b) = {med['c'] / med['b']:.3f} "
              f"({'below' if med['c'] < med['b'] else 'NOT below'} today's two calls), (c)/(a) = {med['c'] / med['a']:.3f} "
              f"(the price of the fused sums)", flush=True)
        del bufs, fresh, mask, magic, magic_b
        plan.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data-gib", type=float, default=24.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="rs63,cg104,cg63")
    ap.add_argument("--variants", default="0,0;1,0;0,2;0,4")
    ap.add_argument("--magic", action="store_true", help="also time fused encode+magic and standalone magic")
    ap.add_argument("--pad", type=int, default=0, help="bytes of padding after every shard (HBM channel spread)")
    ap.add_argument("--no-wait", action="store_true", help="do not wait for a network (A/B runs with it off)")
    ap.add_argument("--lost", default="0", help="erasures of the timed decode, e.g. 0,1,k+1 as ids (default: D0)")
    ap.add_argument("--mix", action="store_true",
                    help="also time lsec_hbm_mix_dev over the same shards: the encode's traffic, XOR only")
    ap.add_argument("--patterns", action="store_true",
                    help="time the per-stripe-pattern decodes against lsec_decode_dev (patterns_bench) and exit")
    ap.add_argument("--nine", action="store_true", help="--patterns: also nine whole-stage lsec_decode_dev launches")
    ap.add_argument("--pattern-stripes", type=int, default=4095)
    ap.add_argument("--pattern-codes", default="rs63,cg63", help="--patterns: names from CONFIGS (their k and m; C = 1 MiB)")
    ap.add_argument("--pattern-lost", default="0", help="--patterns: the erasure list of (a) and (b)")
    ap.add_argument("--check", action="store_true",
                    help="time lsec_check_dev against lsec_encode_dev and encode-and-compare (check_bench; "
                         "--pattern-stripes, --pattern-codes) and exit")
    ap.add_argument("--locate", action="store_true",
                    help="time lsec_locate_dev against lsec_check_dev, clean, corrupt and repairing (locate_bench; "
                         "--pattern-stripes, --pattern-codes) and exit")
    ap.add_argument("--rotated-scrub", action="store_true",
                    help="time lsec_check_dev_rotated / lsec_locate_dev_rotated against the unrotated calls "
                         "(rotated_scrub_bench; --pattern-stripes, --pattern-codes) and exit")
    ap.add_argument("--update", action="store_true",
                    help="time lsec_update_dev against a device copy + lsec_encode_dev (update_bench; "
                         "--pattern-stripes, --pattern-codes) and exit")
    ap.add_argument("--update-masked", action="store_true",
                    help="time lsec_update_dev_masked against lsec_update_dev and the per-class calls it replaces "
                         "(update_masked_bench; --pattern-stripes, --pattern-codes) and exit")
    ap.add_argument("--update-magic", action="store_true",
                    help="time lsec_update_magic_dev_masked against lsec_update_dev_masked alone and followed by "
                         "lsec_stripe_magic_dev (update_magic_bench; --pattern-stripes, --pattern-codes) and exit")
    a = ap.parse_args()
    if a.update_magic:
        update_magic_bench(a)
        return
    if a.update_masked:
        update_masked_bench(a)
        return
    if a.update:
        update_bench(a)
        return
    if a.rotated_scrub:
        rotated_scrub_bench(a)
        return
    if a.locate:
        locate_bench(a)
        return
    if a.patterns:
        patterns_bench(a)
        return
    if a.check:
        check_bench(a)
        return
    dev = torch.device("cuda:0")
    variants = [tuple(int(x) for x in v.split(",")) for v in a.variants.split(";")]
    for name in a.configs.split(","):
        if name not in CONFIGS:  # "rs:K:M:C_KiB" / "cg:K:M:C_KiB"
            t, kk, mm, ck = name.split(":")
            CONFIGS[name] = ({"rs": L.REED_SOL_VAN, "cg": L.CAUCHY_GOOD}[t], int(kk), int(mm), int(ck) << 10)
        meth, k, m, C = CONFIGS[name][:4]
        w = CONFIGS[name][4] if len(CONFIGS[name]) > 4 else -1
        N = max(8, int(a.data_gib * 2**30 / (k * C)))
        plan = L.Plan.for_chunk(meth, k, m, C, w)
        data = torch.randint(0, 256, (N, k, C + a.pad), dtype=torch.uint8, device=dev)[:, :, :C]
        par = torch.empty((N, m, C + a.pad), dtype=torch.uint8, device=dev)[:, :, :C]
        lost = sorted({int(x) for x in a.lost.split(",")})
        out = torch.empty((N, len(lost), C), dtype=torch.uint8, device=dev)
        plan.prepare_encode()  # wide codes: wait for the compiled XOR network (variant 0,0 uses it)
        plan.prepare_decode(lost)
        import time
        # heavy networks can take longer than prepare's 30 s wait; only codes that get one
        # (ec_netgen.cpp wants_xornet / wants_gfw_net / wants_pktnet)
        has_net = (w in (16, 32) and meth == L.REED_SOL_VAN) or (meth in (L.CAUCHY_GOOD, L.CAUCHY_ORIG) and k <= 32) or \
            (meth == L.REED_SOL_VAN and m * k >= 96) or meth in (L.LIBERATION, L.BLAUM_ROTH, L.LIBER8TION)
        t_end = time.time() + (90 if has_net and not a.no_wait else 0)
        while time.time() < t_end and not plan.jit():
            time.sleep(5)
            print(f"{name}: waiting for the encode network", flush=True)
        print(f"{name}: encode network {'ready' if plan.jit() else 'NOT ready'}", flush=True)
        plan.encode_dev(data, par)
        ref_par = par.clone()
        stream = torch.cuda.current_stream()
        res = {v: ([], []) for v in variants}
        tmix = []
        if a.mix:
            lib = E.lib()
            mrefs = L.Plan.shard_refs(plan.tensor_refs(data, par)[0])

            def mix():
                assert lib.lsec_hbm_mix_dev(mrefs, k, m, N, C, stream.cuda_stream) == 0
        for _ in range(a.rounds):
            if a.mix:
                mix()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    mix()
                e1.record(stream)
                torch.cuda.synchronize()
                tmix.append(e0.elapsed_time(e1) / a.reps)
                plan.encode_dev(data, par)  # restore the parity the variants are checked against
            for v in variants:
                E.set_kernel_variant(v[0], v[1])
                if len(v) > 2:  # a third field: the XCD tile phase (lsec_test_set_tile_phase)
                    E.lib().lsec_test_set_tile_phase(v[2])
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                plan.encode_dev(data, par)
                e0.record(stream)
                for _ in range(a.reps):
                    plan.encode_dev(data, par)
                e1.record(stream)
                for _ in range(a.reps):
                    plan.decode_dev(data, par, lost, out=out)
                e2.record(stream)
                torch.cuda.synchronize()
                res[v][0].append(e0.elapsed_time(e1) / a.reps)
                res[v][1].append(e1.elapsed_time(e2) / a.reps)
                assert torch.equal(par, ref_par), f"variant {v} changed parity"
                for i, e in enumerate(lost):
                    want = data[:, e] if e < k else ref_par[:, e - k]
                    assert torch.equal(out[:, i], want), f"variant {v} decode mismatch (shard {e})"
        E.set_kernel_variant(0, 0)
        net = int(plan.jit())
        for v in variants:
            te = sorted(res[v][0])[len(res[v][0]) // 2]
            td = sorted(res[v][1])[len(res[v][1]) // 2]
            eb = (k + m) * C * N
            db = (k + len(lost)) * C * N
            print(f"{name:6s} N={N:5d} variant={v} jit={net if v[:2] == (0, 0) else 0}  encode {te:8.3f} ms {eb / te / 1e6:7.1f} GB/s "
                  f"({eb / te / 8e9:5.1%})   decode {td:8.3f} ms {db / td / 1e6:7.1f} GB/s ({db / td / 8e9:5.1%})",
                  flush=True)
        if tmix:
            tm = sorted(tmix)[len(tmix) // 2]
            eb = (k + m) * C * N
            print(f"{name:6s} N={N:5d} mix probe (XOR of k to m, no GF)  {tm:8.3f} ms {eb / tm / 1e6:7.1f} GB/s ({eb / tm / 8e9:5.1%})",
                  flush=True)
        E.set_kernel_variant(0, 0)
        E.lib().lsec_test_set_tile_phase(1)  # the default
        if a.magic:
            mg = torch.zeros((N, 4), dtype=torch.uint8, device=dev)
            tm = []
            for fn in (lambda: plan.encode_magic_dev(data, par, mg), lambda: plan.stripe_magic_dev(data, par, mg)):
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                tm.append(e0.elapsed_time(e1) / a.reps)
            eb = (k + m) * C * N
            print(f"{name:6s} encode+magic fused {tm[0]:8.3f} ms {eb / tm[0] / 1e6:7.1f} GB/s ({eb / tm[0] / 8e9:5.1%})   "
                  f"magic alone {tm[1]:8.3f} ms {eb / tm[1] / 1e6:7.1f} GB/s ({eb / tm[1] / 8e9:5.1%})", flush=True)
            del mg
        del data, par, out, ref_par
        plan.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
