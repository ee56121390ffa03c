"""GPU: lsec_update_dev, the parity update for partial-stripe writes.

Bar: bit-exact.  The yardstick is the reference: the expected parity is always the reference's encode
(oracle/_ref when it is built, else the oracle restatement; test_gpu_check.ref_encode) of the data with
the changed chunks replaced, computed on the CPU.  It is never taken from the engine.

Shards live in the arenas of tests/layouts.py (canary gaps and guard bands), the fresh chunks in a
second arena of the same kind.  The refs of the data chunks that do not change point into a third
buffer of random bytes, so a kernel that read them would get the parity wrong (NULL there is the CPU
test's case).  After every call
  * the whole shard arena equals the expected image: the parity chunks hold the reference's bytes,
    the changed chunks hold the fresh bytes with LSEC_UPDATE_STORE and the old ones without, and
    every other chunk, every canary gap and both guard bands are unchanged,
  * the fresh arena and the decoy buffer are unchanged,
  * the launch record names the predicted form, once per launch.
"""
import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC

pytestmark = pytest.mark.gpu

CODES = dict(TC.CODES, rs642=(L.REED_SOL_VAN, 64, 2, 0))  # + the widest launch: column id 63
CASES = [("rs63", (0,)), ("rs63", (5,)), ("rs63", (4, 1)), ("rs63", (0, 1, 2, 3, 4, 5)),
         ("rs164", (15,)), ("rs164", (3, 9, 12)),
         ("raid4_61", (2,)),
         ("r6_62", (0, 5)),
         ("rs128", (11,)),
         ("rs52", (4,)),
         ("rs642", (63,)),
         ("cg63", (0,)), ("cg63", (5, 2)),
         ("co42", (3,)),
         ("cg164", (15,))]
LAYOUTS = ("packed", "off8", "mixed")
NSTRIPES, SPLIT = 5, 2  # split: three launches of 2, 2 and 1 stripes

_fresh, _parity = {}, {}


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES, or the tuple itself (tests/scrub_forms.py's plans)"""
    return CODES[code] if isinstance(code, str) else tuple(code)


def case_id(case):
    name = case[0] if isinstance(case[0], str) else "_".join(str(x) for x in case[0])
    return name + "-" + "_".join(str(j) for j in case[1])


def sliced(code):
    return spec(code)[3] != 0


def form_of(code, packet, size):
    _, k, m, _ = spec(code)
    return E.predict_form("upd", 2 if sliced(code) else 1, k, m, packet, size)


def shapes(code):
    """(packet, C): the smallest sizes at which the form that runs can go wrong"""
    if not sliced(code):
        f = form_of(code, 0, 8192)
        tile = 256 * 4 * f.VW * f.IT  # bytes of a chunk per tile, from the form built
        return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]
    # one super-packet; 161 super-packets of packet 8 (1288 bytes of column space: no multiple of a
    # tile); three super-packets of packet 512 (1.5 tiles at one dword per lane)
    out = [(8, 64), (8, 64 * 161), (512, 8 * 512 * 3)]
    if form_of(code, 64, 8 * 64 * 65).DW == 4:
        out.append((64, 8 * 64 * 65))  # a 4 KiB tile: 65 super-packets make 4160 bytes
    return out


def fresh_chunks(code, packet, size, cols):
    """uint8 [N, c, C], random; computed once per shape, never modified"""
    key = (code, packet, size, tuple(cols))
    if key not in _fresh:
        rng = np.random.default_rng([spec(code)[1], packet, size, *cols])
        f = rng.integers(0, 256, (NSTRIPES, len(cols), size), dtype=np.uint8)
        f.setflags(write=False)
        _fresh[key] = f
    return _fresh[key]


def updated(code, packet, full, cols, fresh):
    """the stripes [N, k+m, C] the reference has after the write: data with the chunks replaced, its encode"""
    _, k, m, _ = spec(code)
    out = full.copy()
    for i, j in enumerate(cols):
        out[:, j] = fresh[:, i]
    for s in range(full.shape[0]):
        out[s, k:] = TC.ref_encode(spec(code), packet, out[s, :k])
    return out


def updated_consistent(code, packet, size, cols):
    key = (code, packet, size, tuple(cols))
    if key not in _parity:
        full = TC.stripes(spec(code), packet, size, NSTRIPES)
        u = updated(code, packet, full, cols, fresh_chunks(code, packet, size, cols))
        u.setflags(write=False)
        _parity[key] = u
    return _parity[key]


class Bench:
    """consistent stripes in an arena, fresh chunks in a second one, decoys behind the untouched refs"""

    def __init__(self, torch, code, packet, size, layout, cols, fresh=None):
        self.torch, self.code, self.packet, self.size, self.cols = torch, code, packet, size, tuple(cols)
        _, self.k, self.m, _ = spec(code)
        k, m, c = self.k, self.m, len(cols)
        self.full = TC.stripes(spec(code), packet, size, NSTRIPES)
        self.fresh = fresh_chunks(code, packet, size, cols) if fresh is None else fresh
        self.lay = LY.plan_layout(layout, k, m, NSTRIPES, size, outputs=range(k, k + m))
        self.flay = LY.plan_layout(layout, c, 0, NSTRIPES, size)
        LY.check_layout(self.lay)
        LY.check_layout(self.flay)
        self.before = LY.images(self.lay, self.full, ())[0]
        self.arena, self.real_refs, _ = LY.to_device(torch, self.lay, self.before)
        self.fbefore = LY.images(self.flay, self.fresh, ())[0]
        self.farena, self.fresh_refs, _ = LY.to_device(torch, self.flay, self.fbefore)
        rng = np.random.default_rng(size + 7)
        self.dbefore = rng.integers(0, 256, self.lay.total, dtype=np.uint8)
        self.darena, decoys, _ = LY.to_device(torch, self.lay, self.dbefore)
        self.refs = [self.real_refs[i] if i in cols or i >= k else decoys[i] for i in range(k + m)]
        self.plan = TC.make_plan(spec(code), packet, size)
        self.form = form_of(code, packet, size)

    def close(self):
        self.plan.close()

    def arm(self, image=None):
        self.arena.copy_(self.torch.from_numpy(self.before if image is None else image))

    def call(self, store, idx=None, stream=None):
        """one call over the arena as it is, for the changed chunks idx (positions in cols; None: all)"""
        idx = range(len(self.cols)) if idx is None else idx
        st = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.plan.update_dev_refs(self.refs, NSTRIPES, self.size, [self.cols[i] for i in idx],
                                  [self.fresh_refs[i] for i in idx], store, st)

    def got(self):
        """the arena after the call; the fresh arena and the decoys must be as they were"""
        self.torch.cuda.synchronize()
        assert np.array_equal(self.farena.cpu().numpy(), self.fbefore), "the call wrote into the fresh chunks"
        assert np.array_equal(self.darena.cpu().numpy(), self.dbefore), "the call wrote into an untouched chunk's ref"
        return self.arena.cpu().numpy()

    def want(self, store, chunks=None):
        """the expected arena: the reference's stripes after the write; without the flag the old data stay"""
        u = (updated_consistent(self.code, self.packet, self.size, self.cols) if chunks is None else chunks).copy()
        if not store:
            u[:, :self.k] = self.full[:, :self.k]
        return LY.images(self.lay, u, ())[0]

    def run(self, store, split=0, stream=None):
        what = f"{case_id((self.code, self.cols))} packet={self.packet} C={self.size} store={store} split={split}"
        self.arm()
        if stream is not None:
            self.torch.cuda.synchronize()
        E.set_pattern_split(split)
        try:
            self.call(store, stream=stream)
        finally:
            E.set_pattern_split(0)
        forms = E.launch_record()
        LY.assert_arena(self.lay, self.got(), self.want(store), what)
        launches = 1 if not split else -(-NSTRIPES // split)
        assert forms == [self.form] * launches, (what, forms, self.form)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_update(cuda, case, layout):
    import torch

    code, cols = case
    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, layout, cols)
        try:
            for store in (False, True):
                bench.run(store)
                bench.run(store, split=SPLIT)  # crosses two launch boundaries
        finally:
            bench.close()


@pytest.mark.parametrize("code", ["rs63", "cg164"])
def test_on_a_stream_of_its_own(cuda, code):
    import torch

    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "off8", (spec(code)[1] - 1,))
    try:
        st = torch.cuda.Stream()
        bench.run(True, stream=st.cuda_stream)
        bench.run(False, split=SPLIT, stream=st.cuda_stream)
    finally:
        bench.close()


def test_torch_form(cuda):
    import torch

    code, size, cols = "rs63", 4096, (3, 0)
    _, k, m, _ = spec(code)
    full = TC.stripes(spec(code), 0, size, NSTRIPES)
    fresh = fresh_chunks(code, 0, size, cols)
    want = updated(code, 0, full, cols, fresh)
    for store in (False, True):
        data, par = torch.from_numpy(full[:, :k].copy()).cuda(), torch.from_numpy(full[:, k:].copy()).cuda()
        f = torch.from_numpy(fresh.copy()).cuda()
        with TC.make_plan(spec(code), 0, size) as p:
            p.update_dev(data, par, cols, f, store=store)
            torch.cuda.synchronize()
        assert np.array_equal(par.cpu().numpy(), want[:, k:])
        assert np.array_equal(data.cpu().numpy(), want[:, :k] if store else full[:, :k])
        assert np.array_equal(f.cpu().numpy(), fresh)


# ---------------------------------------------------------------- syndrome preservation
@pytest.mark.parametrize("case", [("rs63", (4, 1)), ("rs63", (0, 1, 2, 3, 4, 5)), ("rs164", (3, 9, 12)), ("raid4_61", (2,)),
                                  ("r6_62", (0, 5)), ("cg63", (5, 2)), ("cg164", (15,))], ids=case_id)
def test_keeps_the_syndrome_of_an_inconsistent_stripe(cuda, case):
    """2 of the 5 stripes are inconsistent before the write: a flipped byte in a parity row of one and
    in a data chunk that does not change (a parity row where every chunk changes) of the other.  The
    check's words over the stripes with the chunks replaced are, after the update, the CPU-expected
    ones -- the reference's re-encode of the data as stored after the update against the stored parity
    -- and the words the check gave over the old stripes before it."""
    import torch

    code, cols = case
    _, k, m, _ = spec(code)
    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "mixed", cols)
    words = TC.Words(torch, NSTRIPES)
    stream = torch.cuda.current_stream().cuda_stream

    def check():
        words.arm()
        bench.plan.check_dev_refs(bench.real_refs, NSTRIPES, size, words.syndrome_ptr, words.bad_ptr, stream)
        torch.cuda.synchronize()
        return words.read()[0]

    def stored():
        a = bench.arena.cpu().numpy()
        return np.stack([np.stack([a[bench.lay.start(i, s):][:size] for i in range(k + m)]) for s in range(NSTRIPES)])

    try:
        untouched = [j for j in range(k) if j not in cols]
        hits = [(1, k + m - 1, size - 1), (3, untouched[-1] if untouched else k, size // 2)]
        image = bench.before.copy()
        for s, i, b in hits:
            image[bench.lay.start(i, s) + b] ^= TC.FLIP
        for store in (True, False):
            bench.arm(image)
            old = check()
            assert [int(w != 0) for w in old] == [0, 1, 0, 1, 0], old
            bench.call(store)
            if not store:  # the caller puts the fresh bytes in place itself
                torch.cuda.synchronize()
                for i, j in enumerate(cols):
                    for s in range(NSTRIPES):
                        a, f = bench.lay.start(j, s), bench.flay.start(i, s)
                        bench.arena[a:a + size].copy_(bench.farena[f:f + size])
            new = check()
            st = stored()
            for i, j in enumerate(cols):
                assert np.array_equal(st[:, j], bench.fresh[:, i])
            want = np.array([TC.expected_mask(spec(code), packet, st[s]) for s in range(NSTRIPES)], np.uint32)
            assert np.array_equal(new, want), (store, new, want)
            assert np.array_equal(new, old), (store, new, old)
    finally:
        bench.close()


# ---------------------------------------------------------------- identity, order, composition
@pytest.mark.parametrize("case", [("rs63", (4, 1)), ("raid4_61", (2,)), ("rs128", (11,)), ("cg63", (5, 2)), ("cg164", (15,))],
                         ids=case_id)
def test_identity(cuda, case):
    """fresh equal to the old bytes leaves the whole arena bit-identical, with and without the flag"""
    import torch

    code, cols = case
    for packet, size in shapes(code)[-2:]:
        full = TC.stripes(spec(code), packet, size, NSTRIPES)
        bench = Bench(torch, code, packet, size, "off8", cols, fresh=np.ascontiguousarray(full[:, list(cols)]))
        try:
            for store in (False, True):
                bench.arm()
                bench.call(store)
                LY.assert_arena(bench.lay, bench.got(), bench.before, f"identity {case_id(case)} C={size} store={store}")
        finally:
            bench.close()


@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_order_of_the_list(cuda, code):
    """{4, 1} with the fresh chunks in that order gives the bytes of {1, 4} with them swapped"""
    import torch

    packet, size = shapes(code)[-1]
    fresh = fresh_chunks(code, packet, size, (4, 1))
    a = Bench(torch, code, packet, size, "mixed", (4, 1), fresh=fresh)
    b = Bench(torch, code, packet, size, "mixed", (1, 4), fresh=np.ascontiguousarray(fresh[:, ::-1]))
    try:
        want = updated(code, packet, a.full, (4, 1), fresh)
        for store in (False, True):
            got = []
            for bench in (a, b):
                bench.arm()
                bench.call(store)
                got.append(bench.got())
                LY.assert_arena(bench.lay, got[-1], bench.want(store, want), f"order {bench.cols} store={store}")
            assert np.array_equal(got[0], got[1])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("code", ["rs63", "rs164", "cg63"])
def test_two_calls_compose(cuda, code):
    """{1} then {4} on the same stripes equals one call on {1, 4}"""
    import torch

    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "packed", (1, 4))
    try:
        for store in (False, True):
            bench.arm()
            bench.call(store)
            once = bench.got()
            LY.assert_arena(bench.lay, once, bench.want(store), f"one call, store={store}")
            bench.arm()
            bench.call(store, idx=[0])
            bench.call(store, idx=[1])
            LY.assert_arena(bench.lay, bench.got(), once, f"two calls, store={store}")
    finally:
        bench.close()
