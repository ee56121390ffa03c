"""GPU: stripes that do not share an erasure pattern, decoded in one launch
(lsec_decode_dev_patterns) and the degraded read of a rotated LUN (lsec_decode_dev_rotated).

Bar: bit-exact.  The yardstick is the reference: every stripe is encoded by the real reference
(oracle/_ref) when it is built, else by the oracle restatement, and the rebuilt chunks must equal
the encoded ones.  Every shard lives in a buffer of its own with a stride larger than the chunk,
a canary in the gaps and 0xA5 garbage in the erased slots; after each call
  * the erased slots equal the reference,
  * every survivor, every gap and every chunk of an empty-pattern stripe is unchanged
    (both: the whole image equals the expected one),
  * the image equals what per-pattern lsec_decode_dev runs leave on copies.
"""
import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

pytestmark = pytest.mark.gpu

CANARY, GARBAGE = 0xC3, 0xA5
PATTERNS_63 = [[], [0], [5], [6], [8], [0, 5], [1, 7], [6, 8], [0, 3, 5], [2, 6, 7]]

_ref_cache = {}


def reference_stripes(method, k, m, size, nstripes, packet=0):
    """uint8 [N, k+m, C]: random data and the reference's parity; computed once per shape, never modified"""
    key = (method, k, m, size, nstripes, packet)
    if key not in _ref_cache:
        rng = np.random.default_rng(abs(hash(key)) % (1 << 32))
        full = np.empty((nstripes, k + m, size), np.uint8)
        full[:, :k] = rng.integers(0, 256, (nstripes, k, size), dtype=np.uint8)
        rp = O.RefPlan(method, k, m, 8, packet) if O.ref_available() else None
        for s in range(nstripes):
            full[s, k:] = rp.encode(full[s, :k]) if rp else O.encode(method, full[s, :k], m, packet, 8)
        full.setflags(write=False)
        _ref_cache[key] = full
    return _ref_cache[key]


def make_plan(method, k, m, size, packet=0):
    p = L.Plan.new(method, size, k, m, 8, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


def images(chunks, erased_slots, pad=40):
    """chunks [N, n, C] as the shards hold them -> (want, before) uint8 [n, N, C + pad]: shard i in
    row i, canary gaps; `before` has garbage in the slots (stripe, shard) of erased_slots"""
    nstr, n, size = chunks.shape
    want = np.full((n, nstr, size + pad), CANARY, np.uint8)
    want[:, :, :size] = chunks.transpose(1, 0, 2)
    before = want.copy()
    for s, i in erased_slots:
        before[i, s, :size] = GARBAGE
    return want, before


def refs_of(t):
    """shard refs of a device image [n, N, stride]"""
    return [(t[i].data_ptr(), t.stride(1)) for i in range(t.shape[0])]


def assert_same(got, want, what):
    if np.array_equal(got, want):
        return
    d = np.argwhere(got != want)
    slots = sorted({(int(s), int(i)) for i, s, _ in d})[:8]
    raise AssertionError(f"{what}: {len(d)} bytes differ, first (stripe, shard) slots {slots}, "
                         f"bytes [{d[:, 2].min()}, {d[:, 2].max()}]")


def effective(p, pat):
    """the slots a pattern rebuilds (a raid4 pattern that loses only the parity rebuilds nothing)"""
    if p.method == L.RAID4 and pat and min(pat) >= p.k:
        return []
    return sorted(set(pat))


def run_patterned(torch, p, full, patterns, sp, stream=None, queue_ids=None, cross_check=True):
    """One patterned call over images of `full` with stripe pattern ids sp (a value >= len(patterns):
    no pattern); returns the device image as numpy after checking it three ways.  queue_ids, when
    given, puts the ids into device memory right before the call and returns that tensor.
    cross_check=False leaves out the third way, the engine's own lsec_decode_dev (test_gpu_scrub_forms:
    shapes whose lsec_decode_dev would start a network compile per pattern)."""
    nstr, n, size = full.shape
    at = lambda s: patterns[sp[s]] if sp[s] < len(patterns) else []
    want, before = images(full, [(s, i) for s in range(nstr) for i in at(s)])
    # slots a call must not touch keep their garbage: those of a raid4 parity-only pattern
    for s in range(nstr):
        for i in set(at(s)) - set(effective(p, at(s))):
            want[i, s, :size] = GARBAGE
    dev = torch.from_numpy(before).cuda()
    sp_dev = None if queue_ids else torch.from_numpy(np.asarray(sp, np.uint8)).cuda()
    torch.cuda.synchronize()
    if queue_ids:
        sp_dev = queue_ids()
    p.decode_dev_patterns_refs(refs_of(dev), nstr, size, patterns, sp_dev.data_ptr(),
                               0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert_same(got, want, "against the reference")
    if not cross_check:
        return got
    # per-pattern lsec_decode_dev runs over all stripes of a copy; each stripe taken from its pattern's run
    single = before.copy()
    for pi, pat in enumerate(patterns):
        mine = [s for s in range(nstr) if sp[s] == pi]
        if not mine or not pat:
            continue
        cp = torch.from_numpy(before).cuda()
        p.decode_dev_refs(refs_of(cp), nstr, size, pat)
        torch.cuda.synchronize()
        single[:, mine] = cp.cpu().numpy()[:, mine]
    assert_same(got, single, "against per-pattern lsec_decode_dev")
    return got


def seeded_ids(nstr, npat, seed, none_at=None):
    sp = np.random.default_rng(seed).permutation(np.arange(nstr) % npat).astype(np.uint8)
    if none_at is not None:
        sp[none_at] = 255
    return sp


# ---------------------------------------------------------------- 1, 6: RS(6+3), ragged tile with a half-filled lane
def test_rs63_mixed_patterns_and_reordered_table(cuda):
    import torch

    k, m, size, nstr = 6, 3, 24584, 37  # three 8 KiB tiles + 8 bytes
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    sp = seeded_ids(nstr, len(PATTERNS_63), 1, none_at=11)
    assert set(sp.tolist()) == set(range(len(PATTERNS_63))) | {255}
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        run_patterned(torch, p, full, PATTERNS_63, sp)
        # the same patterns in another order: a table of its own, not the first call's
        order = [3, 0, 9, 1, 8, 2, 7, 4, 6, 5]
        pats2 = [PATTERNS_63[i] for i in order]
        sp2 = np.array([order.index(x) if x != 255 else 255 for x in sp], np.uint8)
        run_patterned(torch, p, full, pats2, sp2)
        run_patterned(torch, p, full, PATTERNS_63, sp)  # and the first one again, from the cache


def test_rs63_split_launches(cuda):
    import torch

    k, m, size, nstr = 6, 3, 24584, 37
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    sp = seeded_ids(nstr, len(PATTERNS_63), 1, none_at=11)
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        whole = run_patterned(torch, p, full, PATTERNS_63, sp)
        E.set_pattern_split(16)
        try:
            split = run_patterned(torch, p, full, PATTERNS_63, sp)
            want, before = rotated_images(full, [2], 1, 5)
            dev = torch.from_numpy(before).cuda()
            p.decode_dev_rotated_refs(refs_of(dev), nstr, size, [2], 1, 5)
            torch.cuda.synchronize()
            assert_same(dev.cpu().numpy(), want, "rotated, split")
        finally:
            E.set_pattern_split(0)
        assert np.array_equal(whole, split)


# ---------------------------------------------------------------- 2: RS(10+4), runtime K, 0-4 erasures
def test_rs104_zero_to_four_erasures(cuda):
    import torch

    k, m, size, nstr = 10, 4, 8200, 19
    pats = [[], [3], [11], [0, 9], [2, 10, 13], [0, 1, 2, 3], [4, 10, 11, 12], [10, 11, 12, 13]]
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        run_patterned(torch, p, full, pats, seeded_ids(nstr, len(pats), 2))
        # a table of single erasures only: the one-row kernel
        ones = [[3], [11], [0], [13]]
        run_patterned(torch, p, full, ones, seeded_ids(nstr, len(ones), 3))


# ---------------------------------------------------------------- 2b: odd K, the tail of the run-time-K input loop
@pytest.mark.parametrize("k,m", [(5, 2), (7, 3)])
def test_odd_k_runtime_input_tail(cuda, k, m):
    """K = 5 and 7 at run time: the full tiles' four-at-a-time input loop ends in a group of one and
    of three inputs.  C = 8200 is one full 8 KiB tile plus a half-filled lane for the tables of up to
    two erasures, and four full 2 KiB tiles plus 8 bytes for the one-row kernel."""
    import torch

    size, nstr, n = 8200, 19, k + m
    pats = [[], [0], [k - 1], [k], [n - 1], [0, k - 1], [1, k], [k, n - 1]]
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        run_patterned(torch, p, full, pats, seeded_ids(nstr, len(pats), 10))
        # a table of single erasures only: the one-row branchy kernel
        ones = [[0], [k // 2], [k - 1], [k]]
        run_patterned(torch, p, full, ones, seeded_ids(nstr, len(ones), 11))


# ---------------------------------------------------------------- 3: r6 and raid4
def test_r6_and_raid4(cuda):
    import torch

    size, nstr = 4104, 19
    full = reference_stripes(L.REED_SOL_R6_OP, 6, 2, size, nstr)
    pats = [[], [0], [6], [7], [0, 5], [2, 6], [6, 7]]
    with make_plan(L.REED_SOL_R6_OP, 6, 2, size) as p:
        run_patterned(torch, p, full, pats, seeded_ids(nstr, len(pats), 4))
    full = reference_stripes(L.RAID4, 4, 1, size, nstr)
    pats = [[4], [0], [3], []]  # [4]: only the parity lost, which raid4 leaves alone: the slot keeps its garbage
    with make_plan(L.RAID4, 4, 1, size) as p:
        run_patterned(torch, p, full, pats, seeded_ids(nstr, len(pats), 5))
        run_patterned(torch, p, full, [[4], []], seeded_ids(nstr, 2, 6))  # a table with nothing to rebuild


# ---------------------------------------------------------------- 4: Cauchy-good(6+3) at w = 8
@pytest.mark.parametrize("packet,size", [(64, 16896), (24, 9600)])  # 33 super-packets: a ragged column tile
def test_cauchy63_bit_sliced(cuda, packet, size):
    import torch

    k, m, nstr = 6, 3, 21
    full = reference_stripes(L.CAUCHY_GOOD, k, m, size, nstr, packet)
    with make_plan(L.CAUCHY_GOOD, k, m, size, packet) as p:
        assert p.kernel == 2
        run_patterned(torch, p, full, PATTERNS_63, seeded_ids(nstr, len(PATTERNS_63), 7, none_at=4))
        # single data losses only: the 0 / 1 rows the single-pattern path sends to the XOR kernel
        run_patterned(torch, p, full, [[0], [5], [3]], seeded_ids(nstr, 3, 8))


# ---------------------------------------------------------------- 5: rotated LUN
def rotated_images(full, lost, n_shift, first_stripe):
    """the physical devices' images: device i holds, for stripe s, logical chunk (i + (first + s) * n_shift) mod n"""
    nstr, n, size = full.shape
    phys = np.empty_like(full)
    for s in range(nstr):
        rot = ((first_stripe + s) * n_shift) % n
        phys[s] = full[s][(np.arange(n) + rot) % n]
    return images(phys, [(s, d) for s in range(nstr) for d in lost])


@pytest.mark.parametrize("code", ["rs63", "cauchy63"])
@pytest.mark.parametrize("lost", [[2], [2, 7]])
def test_rotated_degraded_read(cuda, code, lost):
    import torch

    k, m, nstr, n = 6, 3, 37, 9
    method, packet, size = (L.REED_SOL_VAN, 0, 24584) if code == "rs63" else (L.CAUCHY_GOOD, 64, 16896)
    full = reference_stripes(method, k, m, size, nstr, packet)
    with make_plan(method, k, m, size, packet) as p:
        for n_shift in (0, 1, 2, 3):
            for first in (5, 3_000_000_007):
                want, before = rotated_images(full, lost, n_shift, first)
                dev = torch.from_numpy(before).cuda()
                p.decode_dev_rotated_refs(refs_of(dev), nstr, size, lost, n_shift, first)
                torch.cuda.synchronize()
                got = dev.cpu().numpy()
                assert_same(got, want, f"rotated n_shift={n_shift} first={first}")
        # per-rotation lsec_decode_dev runs on copies (n_shift 1: every rotation occurs), logical refs
        n_shift, first = 1, 3_000_000_007
        want, before = rotated_images(full, lost, n_shift, first)
        single = before.copy()
        for rot in range(n):
            mine = [s for s in range(nstr) if ((first + s) * n_shift) % n == rot]
            cp = torch.from_numpy(before).cuda()
            phys_refs = refs_of(cp)
            p.decode_dev_refs([phys_refs[(c - rot) % n] for c in range(n)], nstr, size, [(d + rot) % n for d in lost])
            torch.cuda.synchronize()
            single[:, mine] = cp.cpu().numpy()[:, mine]
        assert_same(single, want, "per-rotation lsec_decode_dev")


# ---------------------------------------------------------------- 7: stream order
def test_stripe_pattern_written_on_the_calls_stream(cuda):
    """stripe_pattern arrives by an asynchronous copy queued on a non-default stream and the call is
    queued straight behind it: one synchronisation, at the end."""
    import torch

    k, m, size, nstr = 6, 3, 24584, 37
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    sp = seeded_ids(nstr, len(PATTERNS_63), 9)
    host = torch.from_numpy(sp.copy()).pin_memory()
    sp_dev = torch.full((nstr,), 255, dtype=torch.uint8, device="cuda")  # stale ids: every stripe "no pattern"
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        p.decode_dev_patterns_refs([(0, 0)] * (k + m), 0, size, PATTERNS_63, 0)  # prepare ahead: tables only

        def queue_ids():
            with torch.cuda.stream(st):
                sp_dev.copy_(host, non_blocking=True)
            return sp_dev

        run_patterned(torch, p, full, PATTERNS_63, sp, stream=st, queue_ids=queue_ids)


def test_torch_form(cuda):
    import torch

    k, m, size, nstr = 6, 3, 4096, 8
    full = reference_stripes(L.REED_SOL_VAN, k, m, size, nstr)
    pats = [[0], [1, 7], []]
    sp = np.arange(nstr, dtype=np.uint8) % 3
    broken = full.copy()
    for s in range(nstr):
        broken[s, pats[sp[s]]] = GARBAGE
    data, par = torch.from_numpy(broken[:, :k].copy()).cuda(), torch.from_numpy(broken[:, k:].copy()).cuda()
    with make_plan(L.REED_SOL_VAN, k, m, size) as p:
        p.decode_dev_patterns(data, par, pats, torch.from_numpy(sp).cuda())
        torch.cuda.synchronize()
    assert np.array_equal(data.cpu().numpy(), full[:, :k]) and np.array_equal(par.cpu().numpy(), full[:, k:])
