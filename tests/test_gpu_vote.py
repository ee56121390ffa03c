"""GPU: lsec_vote_dev / lsec_vote_dev_rotated, the read path's quorum vote over a stripe's stored magics, its blank
scan and the lookup of the outside set in a pattern list.

Bar: exact.  The yardstick is never the engine:
  (a) `model` below restates the rules of include/lstore_ec.h in plain Python (the largest group of equal readable
      words, the lowest first member on a tie; the classes; the lookup), over hand-made magic tables;
  (b) the blank scan's verdicts follow from where the test put its nonzero bytes;
  (c) the end-to-end read compares with lsec_segment_read(..., LSEC_READ_PARANOID) over the same host images.
Every output is pre-filled with garbage and sits between canaries; the stored magics and the chunks are compared
whole after each call: the vote only reads them.
"""
import itertools

import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_decode_magic as TDM

pytestmark = pytest.mark.gpu

A, B, CC = 0x11223344, 0xA1B2C3D4, 0x0F0E0D0C  # three magics; UNIQ + c: one that no other chunk holds
UNIQ = 0x70000000
FILL = 0x7B
COUNT_CANARY = 0x5EED5EED
FIRST_HUGE = (1 << 40) + 3
PLANS = {"rs32": (L.REED_SOL_VAN, 3, 2, 0), "cg43": (L.CAUCHY_GOOD, 4, 3, 8), "raid4_31": (L.RAID4, 3, 1, 0),
         "rs568": (L.REED_SOL_VAN, 56, 8, 0)}
NSTRIPES = 53  # thirteen workgroups of four waves and one wave more


def make_plan(code, size=4096):
    method, k, m, packet = PLANS[code]
    return TDM.make_plan((method, k, m, packet), packet, size)


# ---------------------------------------------------------------- the rules, restated
def model(n, k, words, pats, paranoid, blank=None):
    """words[c]: logical chunk c's stored magic, None: unreadable.  blank: None without chunks, else whether every byte
    of the stripe's chunks is zero.  -> (quorum word, outside mask, class, id or None without a list, looked-up)"""
    best, best_word = [], 0
    seen = []
    for c in range(n):  # groups in the order of their lowest members
        if words[c] is None or words[c] in seen:
            continue
        seen.append(words[c])
        group = [j for j in range(n) if words[j] == words[c]]
        if len(group) > len(best):  # strictly greater: the first of the largest groups stays
            best, best_word = group, words[c]
    outside = sum(1 << c for c in range(n) if c not in best)
    if not best or len(best) < k:
        cls = E.VOTE_LOST
    elif blank and len(best) == n and best_word == 0:
        cls = E.VOTE_BLANK
    elif all(c in best for c in range(k)):
        cls = E.VOTE_OK
    else:
        cls = E.VOTE_DEGRADED
    ident, looked = None, False
    if pats is not None:
        looked = cls == E.VOTE_DEGRADED or (cls == E.VOTE_OK and paranoid)
        if looked:
            want = {c for c in range(n) if c not in best}
            ident = next((p for p, pat in enumerate(pats) if set(pat) == want), E.LOCATE_MANY)
        else:
            ident = E.LOCATE_MANY if cls == E.VOTE_LOST else E.LOCATE_CLEAN
    return best_word, outside, cls, ident, looked


def table(n, k, m, nstripes=NSTRIPES):
    """hand-made magics [N][n]; the kind of stripe s is s mod 13, the dissenting chunks move with s"""
    rows = []
    for s in range(nstripes):
        kind, d = s % 13, (s * 7 + 1) % k
        w = [A] * n
        if kind == 1:  # one dissenter, a data chunk
            w[d] = B
        elif kind == 2:  # two dissenters with different magics, a data and a parity chunk
            w[d], w[k + s % m] = B, CC
        elif kind == 3:  # a parity-only dissenter
            w[k + s % m] = B
        elif kind == 4:  # the tie A,B,A,B (an odd chunk left over holds a third magic): A wins
            w = [A if c % 2 == 0 else B for c in range(n)]
            if n % 2:
                w[n - 1] = CC
        elif kind == 5:  # a tie in all but one: the later group is larger by one, and wins
            a = (n - 1) // 2
            w = [CC] * n
            for c in range(2 * a + 1):
                w[c] = B if c % 2 else A
            w[2 * a] = B  # a - ... A's at even places below 2a, B's at the odd ones and at 2a
            assert w.count(B) == w.count(A) + 1 and w[0] == A
        elif kind == 6:  # a quorum of k - 1: every other chunk holds a magic of its own
            w = [A if c < k - 1 else UNIQ + c for c in range(n)]
        elif kind == 7:  # zero magics with dissent
            w = [0] * n
            w[d] = B
        elif kind == 8:  # zero magics, all agreeing (without chunks: OK)
            w = [0] * n
        elif kind == 9:  # zero magics, a parity chunk dissenting
            w = [0] * n
            w[n - 1] = B
        elif kind == 10:  # two data chunks that agree with each other
            w[d], w[(d + 1) % k] = B, B
        elif kind == 11:  # m + 1 dissenters
            for c in range(m + 1):
                w[(d + c) % n] = UNIQ + c
        elif kind == 12:  # the quorum is not the first group: chunk 0 dissents
            w[0] = B
        rows.append(w)
    return rows


def lists(n, k, m):
    """name -> pattern list; None: no list"""
    full = [[]] + [list(c) for e in range(1, min(m, 2) + 1) for c in itertools.combinations(range(n), e)]
    full = full[:254]
    lacking = [p for p in full if 1 not in p and p != []]  # no set with chunk 1, and no empty set
    dup = [[k]] + ([[0, 1]] if m >= 2 else []) + [[1], [], [1], []] + [[c] for c in range(n)]  # duplicates; [] not first
    return {"none": None, "full": full, "lacking": lacking, "dup": dup}


class Stored:
    """the stored magics of n entries in one device arena: entry i at an odd address with an odd stride of its own"""

    def __init__(self, torch, rows, n, unreadable=()):
        self.n, N = n, len(rows)
        strides = [5 + 2 * (i % 3) for i in range(n)]
        offs, cur = [], 33
        for i in range(n):
            offs.append(cur)
            cur += N * strides[i] + 8
            cur += 1 - cur % 2  # every offset odd
        assert all(o % 2 == 1 for o in offs)
        self.host = np.full(cur + 64, 0xC3, np.uint8)
        for i in range(n):
            for s in range(N):
                at = offs[i] + s * strides[i]
                self.host[at:at + 4] = np.array([rows[s][i]], "<u4").view(np.uint8)
        self.dev = TDM.Bytes(torch, self.host, odd=False)  # (its body starts 16 bytes into a 256-byte line)
        self.refs = [(0, 0) if i in unreadable else (self.dev.ptr + offs[i], strides[i]) for i in range(n)]
        assert all(b % 2 == 1 for b, _ in self.refs if b)

    def unchanged(self, what):
        assert np.array_equal(self.dev.body(what), self.host), f"{what}: the stored magics were written"


def rotate_rows(rows, n, n_shift, first):
    """physical device i holds, for stripe s, logical chunk (i + (first + s) * n_shift) mod n"""
    return [[rows[s][(i + (first + s) * n_shift) % n] for i in range(n)] for s in range(len(rows))]


def run_vote(torch, plan, n, stored, chunk_refs, size, pats, paranoid, rotated=None, outputs="all", what=""):
    """one call -> (quorum words, outside, cls, ids, counts), each None where the output was not asked for"""
    N = NSTRIPES if chunk_refs is None else chunk_refs[1]
    refs = None if chunk_refs is None else chunk_refs[0]
    quorum = TDM.Bytes(torch, np.full(4 * N, FILL, np.uint8), odd=True)
    cls = TDM.Bytes(torch, np.full(N, FILL, np.uint8), odd=True)
    want_ids = pats is not None and outputs == "all"
    ids = TDM.Bytes(torch, np.full(N, FILL, np.uint8), odd=True) if want_ids else None
    outside = TDM.Bytes(torch, np.full(8 * N, FILL, np.uint8)) if outputs == "all" else None
    counts = torch.full((7,), COUNT_CANARY, dtype=torch.int32, device="cuda") if outputs == "all" else None
    st = torch.cuda.current_stream().cuda_stream
    args = (pats, quorum.ptr, cls.ptr, ids.ptr if ids else 0, outside.ptr if outside else 0,
            counts[1:].data_ptr() if counts is not None else 0, E.VOTE_PARANOID if paranoid else 0, st)
    if rotated is None:
        plan.vote_dev_refs(stored.refs, refs, N, size, *args)
    else:
        plan.vote_dev_rotated_refs(stored.refs, refs, N, size, rotated[0], rotated[1], *args)
    torch.cuda.synchronize()
    stored.unchanged(what)
    c = None
    if counts is not None:
        c = counts.cpu().numpy().view(np.uint32).tolist()
        assert c[0] == COUNT_CANARY and c[6] == COUNT_CANARY, (what, c)
        c = c[1:6]
    return (quorum.body(what).view("<u4").tolist(), None if outside is None else outside.body(what).view("<u8").tolist(),
            cls.body(what).tolist(), None if ids is None else ids.body(what).tolist(), c)


def expected(n, k, rows, pats, paranoid, blank=None):
    """the model over every stripe -> the tuple run_vote returns"""
    res = [model(n, k, rows[s], pats, paranoid, None if blank is None else blank[s]) for s in range(len(rows))]
    counts = [sum(1 for r in res if r[2] == c) for c in range(4)] + [sum(1 for r in res if r[4] and r[3] == E.LOCATE_MANY)]
    return ([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], None if pats is None else [r[3] for r in res], counts)


def same(got, want, what):
    names = ("quorum", "outside", "cls", "ids", "counts")
    for name, g, w in zip(names, got, want):
        if g is not None:
            assert g == w, (what, name, [(s, a, b) for s, (a, b) in enumerate(zip(g, w)) if a != b][:6])


# ---------------------------------------------------------------- (a) the vote
@pytest.mark.parametrize("code", tuple(PLANS))
def test_vote_against_the_rules(cuda, code):
    import torch

    _, k, m, _ = PLANS[code]
    n = k + m
    rows = table(n, k, m)
    all_pats = lists(n, k, m)
    # the table holds what it is meant to hold (full list, paranoid): every class, a lookup that fails, both ties
    probe = expected(n, k, rows, all_pats["full"], True)
    assert set(probe[2]) == {E.VOTE_OK, E.VOTE_DEGRADED, E.VOTE_LOST}
    assert probe[0][4] == A and probe[0][5] == B and probe[0][12] == A and probe[1][12] == 1
    assert probe[2][6] == E.VOTE_LOST and probe[2][11] == E.VOTE_LOST and probe[2][8] == E.VOTE_OK
    with make_plan(code) as p:
        for name, pats in all_pats.items():
            for paranoid in (False, True):
                what = f"{code} {name} paranoid={paranoid}"
                want = expected(n, k, rows, pats, paranoid)
                plain = run_vote(torch, p, n, Stored(torch, rows, n), None, 0, pats, paranoid, what=what)
                same(plain, want, what)
                if name == "lacking":
                    assert want[4][4] > 0 and E.LOCATE_MANY in [i for i, c in zip(want[3], want[2]) if c == E.VOTE_DEGRADED]
                if name == "dup":  # the lowest index of a duplicate set, and the empty set behind the first place
                    one = 1 + (m >= 2)  # [1] sits at `one` and at one + 2, [] at one + 1 and one + 3
                    assert one in want[3] and one + 2 not in want[3] and one + 3 not in want[3]
                    assert (one + 1 in want[3]) == paranoid
                for n_shift, first in ((1, 0), (n + 1, FIRST_HUGE), (0, 7)):
                    phys = rotate_rows(rows, n, n_shift, first)
                    got = run_vote(torch, p, n, Stored(torch, phys, n), None, 0, pats, paranoid, rotated=(n_shift, first),
                                   what=f"{what} rotated {n_shift} {first}")
                    same(got, plain, f"{what} rotated {n_shift} {first}")  # the plain outputs of the un-rotated table
        # only the required outputs
        bare = run_vote(torch, p, n, Stored(torch, rows, n), None, 0, None, False, outputs="bare", what=f"{code} bare")
        same(bare, expected(n, k, rows, None, False), f"{code} bare")


@pytest.mark.parametrize("code", ("rs32", "cg43", "rs568"))
def test_unreadable_entries(cuda, code):
    """a NULL base is in no group: the lowest id, a parity entry, m + 1 entries, every entry; under rotation the
    unreadable device holds another logical chunk in every stripe"""
    import torch

    _, k, m, _ = PLANS[code]
    n = k + m
    rows = table(n, k, m)
    pats = lists(n, k, m)["full"]
    with make_plan(code) as p:
        for gone in ((0,), (n - 1,), (0, n - 1), tuple(range(m + 1)), tuple(range(n))):
            logical = [[None if c in gone else w for c, w in enumerate(r)] for r in rows]
            what = f"{code} unreadable {gone}"
            got = run_vote(torch, p, n, Stored(torch, rows, n, gone), None, 0, pats, True, what=what)
            want = expected(n, k, logical, pats, True)
            same(got, want, what)
            if len(gone) == n:
                assert set(want[2]) == {E.VOTE_LOST} and not any(want[0]) and set(want[1]) == {(1 << n) - 1 if n < 64 else 2**64 - 1}
            for n_shift, first in ((1, 0), (n + 1, FIRST_HUGE)):
                phys = rotate_rows(rows, n, n_shift, first)
                view = [[None if (c - (first + s) * n_shift) % n in gone else rows[s][c] for c in range(n)] for s in range(len(rows))]
                got = run_vote(torch, p, n, Stored(torch, phys, n, gone), None, 0, pats, True, rotated=(n_shift, first), what=what)
                same(got, expected(n, k, view, pats, True), f"{what} rotated {n_shift}")


# ---------------------------------------------------------------- (b) the blank scan
SCAN_N = 8
TILE = 8192  # the scan's tile as shipped (lsec_test_set_vote_form: 2 steps of 16 bytes per lane, 256 lanes)


def scan_case(n, k, size):
    """(magics [N][n], chunks [N, n, C], blank [N]): zero magics that agree except stripes 4 (another magic) and 5 (a
    dissenter), whose chunks hold nonzero bytes throughout; stripes 0 and 6 all zero; one nonzero byte in the others"""
    rows = [[0] * n for _ in range(SCAN_N)]
    rows[4] = [A] * n
    rows[5][1] = B
    chunks = np.zeros((SCAN_N, n, size), np.uint8)
    chunks[1, 0, 0] = 1                     # the first byte of chunk 0
    chunks[2, n - 1, size - 1] = 0x80       # the last byte of the last parity chunk
    chunks[3, k, size - 3] = 2              # the ragged tail, and for Cauchy the last packet
    chunks[7, k // 2, size // 2 + 1] = 0xFF  # the middle of a middle chunk
    chunks[4], chunks[5] = 0xC3, 0xC3       # no candidates: their chunks are never read
    blank = [not chunks[s].any() for s in range(SCAN_N)]
    assert blank == [True, False, False, False, False, False, True, False]
    return rows, chunks, blank


@pytest.mark.parametrize("layout", ("packed", "off8", "mixed"))
@pytest.mark.parametrize("code", ("rs32", "cg43"))
def test_blank_scan(cuda, code, layout):
    import torch

    _, k, m, packet = PLANS[code]
    n = k + m
    unit = 8 * packet if packet else 8
    sizes = (unit, TILE + unit, 3 * TILE + 3 * unit)  # the smallest chunk, a ragged second tile, several tiles
    assert sizes[1] % TILE and sizes[2] % TILE
    pats = lists(n, k, m)["full"]
    for size in sizes:
        rows, chunks, blank = scan_case(n, k, size)
        assert not packet or (size - 3) // packet == size // packet - 1
        lay = LY.plan_layout(layout, k, m, SCAN_N, size)
        before, _ = LY.images(lay, chunks, ())
        arena, refs, _ = LY.to_device(torch, lay, before)
        with make_plan(code, size) as p:
            want = expected(n, k, rows, pats, True, blank)
            assert [want[2][s] for s in (0, 1, 4, 5, 6)] == [E.VOTE_BLANK, E.VOTE_OK, E.VOTE_OK, E.VOTE_DEGRADED, E.VOTE_BLANK]
            forms = ((False, 2), (True, 2), (False, 4), (True, 4)) if layout == "off8" else ((False, 2),)
            try:
                for plain_loads, steps in forms:
                    E.set_vote_form(plain_loads, steps)
                    what = f"{code} {layout} C={size} plain={plain_loads} steps={steps}"
                    got = run_vote(torch, p, n, Stored(torch, rows, n), (refs, SCAN_N), size, pats, True, what=what)
                    same(got, want, what)
                    LY.assert_arena(lay, arena.cpu().numpy(), before, what)
            finally:
                E.set_vote_form()
            # several launches of the scan
            E.set_pattern_split(3)
            try:
                same(run_vote(torch, p, n, Stored(torch, rows, n), (refs, SCAN_N), size, pats, False, what="split"),
                     expected(n, k, rows, pats, False, blank), f"{code} {layout} C={size} split")
            finally:
                E.set_pattern_split(0)
            # without the chunks there is no scan and no BLANK
            none = run_vote(torch, p, n, Stored(torch, rows, n), (None, SCAN_N), size, pats, True, what="no chunks")
            same(none, expected(n, k, rows, pats, True), f"{code} {layout} C={size} no chunks")
            assert E.VOTE_BLANK not in none[2]
            # the rotated call over the rotated devices: the logical view's verdicts
            if layout == "off8":
                rot = (1, FIRST_HUGE)
                phys_rows = rotate_rows(rows, n, *rot)
                phys = np.stack([chunks[s][(np.arange(n) + ((rot[1] + s) * rot[0]) % n) % n] for s in range(SCAN_N)])
                pb, _ = LY.images(lay, phys, ())
                parena, prefs, _ = LY.to_device(torch, lay, pb)
                got = run_vote(torch, p, n, Stored(torch, phys_rows, n), (prefs, SCAN_N), size, pats, True, rotated=rot, what="rotated")
                same(got, want, f"{code} C={size} rotated scan")
                LY.assert_arena(lay, parena.cpu().numpy(), pb, "rotated scan")


def test_nstripes_zero_prepares_the_tables(cuda):
    """NULL device pointers; with a list the table is uploaded with its masks, and the vote, a decode and a search with
    the same list then upload nothing more than the search's own records"""
    import torch

    n, k, m = 5, 3, 2
    pats = lists(n, k, m)["full"]
    rows = table(n, k, m)
    with make_plan("rs32") as p:
        assert E.plan_images(p) == 0
        p.vote_dev_refs([(0, 0)] * n, None, 0, 0, None, 0, 0)
        assert E.plan_images(p) == 0
        p.vote_dev_refs([(0, 0)] * n, None, 0, 0, pats, 0, 0)
        assert E.plan_images(p) == 3  # records, cells, masks
        p.vote_dev_rotated_refs([(0, 0)] * n, None, 0, 0, 1, 5, pats, 0, 0)
        assert E.plan_images(p) == 3
        same(run_vote(torch, p, n, Stored(torch, rows, n), None, 0, pats, True, what="prepared"),
             expected(n, k, rows, pats, True), "prepared")
        assert E.plan_images(p) == 3
        ids = torch.full((NSTRIPES,), E.LOCATE_MANY, dtype=torch.uint8, device="cuda")
        p.decode_dev_patterns_refs([(0, 0)] * n, 0, 4096, pats, ids.data_ptr())
        assert E.plan_images(p) == 3  # the decode's table is the vote's


# ---------------------------------------------------------------- (c) the read, end to end
READ_N, READ_C, N_SHIFT = 24, 4096, 1


def damaged_images(p, k, m, missing):
    """host images of READ_N stripes written by lsec_segment_write, then damaged; -> (images, the stripes by damage)"""
    n, rec = k + m, READ_C + 4
    rng = np.random.default_rng(43 + len(missing))
    data = rng.integers(0, 256, (READ_N, k, READ_C), dtype=np.uint8)
    images = p.segment_write(data, n_shift=N_SHIFT, first_stripe=0)
    dev_of = lambda s, c: (c - s * N_SHIFT) % n  # noqa: E731
    ok_devs = [d for d in range(n) if d not in missing]

    def magic(s, d):
        return images[d][s * rec:s * rec + 4]

    stripes = dict(one=2, two=5, flip=8, blank=(11, 12), lost=15, parity=19)
    magic(stripes["one"], ok_devs[1])[:] ^= 0x5A                 # a wrong magic on one device
    for d in ok_devs[2:4]:                                       # and on two
        magic(stripes["two"], d)[:] ^= 0x33
    c = 1                                                        # a silently flipped byte in data chunk 1
    images[dev_of(stripes["flip"], c)][stripes["flip"] * rec + 4 + 1234] ^= 0x40
    for s in stripes["blank"]:                                   # never written
        for d in range(n):
            images[d][s * rec:(s + 1) * rec] = 0
    for i, d in enumerate(ok_devs[:n - len(missing) - (k - 1)]):  # only k - 1 magics agree
        magic(stripes["lost"], d)[:] = np.array([UNIQ + i], "<u4").view(np.uint8)
    magic(stripes["parity"], dev_of(stripes["parity"], k))[:] ^= 0x0F  # a wrong magic on a parity chunk alone
    return data, images, stripes


@pytest.mark.parametrize("missing", ((), (6,)))
@pytest.mark.parametrize("code", ("rs43", "cg43"))
def test_read_end_to_end(cuda, code, missing):
    """vote -> decode with the magics -> search and repair, on one stream with no host step between the calls, gives
    the user data lsec_segment_read gives and its statuses"""
    import torch

    method = L.REED_SOL_VAN if code == "rs43" else L.CAUCHY_GOOD
    k, m = 4, 3
    n, rec = k + m, READ_C + 4
    pats = [[]] + [list(c) for e in range(1, m + 1) for c in itertools.combinations(range(n), e)]
    with L.Plan.for_chunk(method, k, m, READ_C) as p:
        data, images, stripes = damaged_images(p, k, m, missing)
        want_data, status, lost = p.segment_read(images, READ_N, READ_C, n_shift=N_SHIFT, first_stripe=0, paranoid=True,
                                                 missing=missing)
        status = status.tolist()
        # the damage does what it is meant to do, on the host: every stripe's answer is the written data, the k - 1
        # stripe is lost, and without a missing device the blank stripes are reported blank
        assert status[stripes["lost"]] == -1 and lost >= 1
        if not missing:
            assert status.count(-1) == 1 and all(status[s] == 2 for s in stripes["blank"])
        assert status[stripes["flip"]] == 1 and status[stripes["one"]] in (0, 1) and status[stripes["two"]] in (0, 1)
        for s in range(READ_N):
            if status[s] in (0, 1) and s not in stripes["blank"]:
                assert np.array_equal(want_data[s], data[s]), s
        # upload: the magics with record stride 4, the chunks in an 8-aligned arena (a missing device's hold garbage)
        mags = np.stack([images[d].reshape(READ_N, rec)[:, :4] for d in range(n)])
        chunks = np.stack([images[d].reshape(READ_N, rec)[:, 4:] for d in range(n)])
        for d in missing:
            mags[d], chunks[d] = 0xEE, 0xA5
        dmag = torch.from_numpy(np.ascontiguousarray(mags)).cuda()
        arena = torch.from_numpy(np.ascontiguousarray(chunks)).cuda()
        assert arena.data_ptr() % 8 == 0
        stored = [(0, 0) if d in missing else (dmag.data_ptr() + d * READ_N * 4, 4) for d in range(n)]
        refs = [(arena.data_ptr() + d * READ_N * READ_C, READ_C) for d in range(n)]
        quorum = torch.full((4 * READ_N,), FILL, dtype=torch.uint8, device="cuda")
        cls, ids, bad, found = (torch.full((READ_N,), FILL, dtype=torch.uint8, device="cuda") for _ in range(4))
        magic = torch.full((4 * READ_N,), FILL, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            st = stream.cuda_stream
            p.vote_dev_rotated_refs(stored, refs, READ_N, READ_C, N_SHIFT, 0, pats, quorum.data_ptr(), cls.data_ptr(),
                                    ids.data_ptr(), 0, 0, E.VOTE_PARANOID, st)
            p.decode_magic_dev_rotated_refs(refs, READ_N, READ_C, list(missing), N_SHIFT, 0, magic.data_ptr(), quorum.data_ptr(),
                                            bad.data_ptr(), 0, st)
            p.search_dev_patterns_rotated_refs(refs, READ_N, READ_C, N_SHIFT, 0, pats, quorum.data_ptr(), found.data_ptr(),
                                               bad.data_ptr(), 0, 0, E.SEARCH_REPAIR, st)
        stream.synchronize()
        cls, ids, bad, found = (t.cpu().tolist() for t in (cls, ids, bad, found))
        got = arena.cpu().numpy()
        # the vote's verdicts are the model's over the logical view of the images
        view = [[None if (c - s * N_SHIFT) % n in missing else int(mags[(c - s * N_SHIFT) % n, s].view("<u4")[0]) for c in range(n)]
                for s in range(READ_N)]
        blank = [not chunks[:, s].any() for s in range(READ_N)]
        want = expected(n, k, view, pats, True, blank)
        same((quorum.cpu().numpy().view("<u4").tolist(), None, cls, ids, None), want, f"{code} read {missing}")
        for s in range(READ_N):
            what = (code, missing, s, status[s], cls[s], ids[s], bad[s], found[s])
            if status[s] == 2:
                assert cls[s] == E.VOTE_BLANK, what
            elif status[s] == -1:
                assert cls[s] == E.VOTE_LOST or (bad[s] and found[s] == E.LOCATE_MANY), what
            else:
                assert cls[s] in (E.VOTE_OK, E.VOTE_DEGRADED) and not (bad[s] and found[s] == E.LOCATE_MANY), what
                for c in range(k):
                    assert np.array_equal(got[(c - s * N_SHIFT) % n, s], want_data[s, c]), what + (c,)
        assert cls[stripes["lost"]] == E.VOTE_LOST and bad[stripes["flip"]] == 1 and found[stripes["flip"]] < len(pats)
        if not missing:
            assert [cls[s] for s in stripes["blank"]] == [E.VOTE_BLANK] * 2
            assert ids[stripes["one"]] == pats.index([(1 + stripes["one"] * N_SHIFT) % n])  # device 1's chunk of that stripe
