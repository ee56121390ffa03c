"""GPU: lsec_check_dev_rotated / lsec_locate_dev_rotated, the scrub of a rotated LUN over its physical devices.

Bar: bit-exact.  The yardstick is the reference, never the engine: logical stripes come from
test_gpu_check.stripes() (oracle/_ref when it is built, else the oracle restatement), they are rotated
onto the devices on the host by the numpy permutation of test_gpu_patterns.rotated_images, and the
expected outputs of a corrupted stripe come from test_gpu_locate.expected() on its LOGICAL view.  From
those follow
  located_dev  (located - rot_s) mod n, rot_s = ((first_stripe + s) * n_shift) mod n; the sentinels as they are
  dev_faults   numpy's bincount of the located_dev values below n
Only test_consistent_with_the_unrotated_calls compares engine with engine, and says so.

Devices live in the arenas of tests/layouts.py, shard i of the layout as device i.  Every output sits in
one buffer between canary bytes, pre-filled with garbage, `located` and `located_dev` at odd addresses.
After every call the canaries are unchanged and, without repair, so is the whole arena.
"""
import numpy as np
import pytest

from lstore_amd import erasure as E

import layouts as LY
import test_gpu_check as TC
import test_gpu_locate as TL
import test_gpu_patterns as TP

pytestmark = pytest.mark.gpu

CODES = {c: TC.CODES[c] for c in ("rs63", "r6_62", "rs52", "rs128", "rs164", "cg63", "cg164")}
BYTEWISE = ("rs63", "r6_62", "rs52", "rs128", "rs164")  # fixed K; an XOR row, n = 8; run-time odd K; 8 rows; n = 20
# a half lane (ragged only), one tile + a ragged tail, three tiles + a tail
BYTEWISE_SIZES = ((0, 8), (0, 8200), (0, 24584))
# (packet, C): one super-packet, a ragged column tile; k = 16: 4 dwords per lane
SLICED_SIZES = {"cg63": ((8, 64), (8, 64 * 161)), "cg164": ((64, 8 * 64 * 65),)}
FIRSTS = (5, 3_000_000_007)  # a small value and one beyond 32 bits
FLIP, FLIP2 = TC.FLIP, 0x33
CANARY, FILL = 0x5E, 0x7B
CLEAN, MANY = E.LOCATE_CLEAN, E.LOCATE_MANY
NAMES = ("syndrome", "hyp", "located", "located_dev", "counts", "dev_faults")


def shapes(code):
    return list(BYTEWISE_SIZES if code in BYTEWISE else SLICED_SIZES[code])


def shifts(n):
    """0: the unrotated behaviour; 1: every rotation; 3: shares a factor with n = 9; n + 2: taken mod n"""
    return (0, 1, 3, n + 2)


def rot_of(n, n_shift, first, s):
    return ((first + s) * n_shift) % n


def physical(full, n_shift, first):
    """[N, n, C] as the devices hold the logical stripes `full`: test_gpu_patterns' permutation"""
    size = full.shape[2]
    want, _ = TP.rotated_images(full, [], n_shift, first)  # [n, N, C + pad]
    return np.ascontiguousarray(want[:, :, :size].transpose(1, 0, 2))


class Outs:
    """[syndrome | hyp | located (odd) | located_dev (odd) | counts | dev_faults | bad_count], one device
    buffer of bytes with 16 or more canary bytes around each; the outputs start as FILL"""

    def __init__(self, torch, nstripes, n):
        self.nstripes, self.n = nstripes, n
        off, self.off = 16, {}
        for name, length, align in (("syndrome", 4 * nstripes, 4), ("hyp", 8 * nstripes, 8), ("located", nstripes, 0),
                                    ("located_dev", nstripes, 0), ("counts", 8, 4), ("dev_faults", 4 * n, 4), ("bad_count", 4, 4)):
            off = (off + align - 1) // align * align if align else off | 1
            self.off[name] = (off, length)
            off += length + 16
        t = np.full(off, CANARY, np.uint8)
        self.mask = np.ones(off, bool)
        for o, ln in self.off.values():
            t[o:o + ln] = FILL
            self.mask[o:o + ln] = False
        self.template_np = t
        self.template = torch.from_numpy(t).cuda()
        self.dev = torch.empty_like(self.template)
        assert self.dev.data_ptr() % 8 == 0
        assert self.ptr("located") % 2 == 1 and self.ptr("located_dev") % 2 == 1

    def ptr(self, name):
        return self.dev.data_ptr() + self.off[name][0]

    def arm(self):
        self.dev.copy_(self.template)

    def read(self):
        """{name: array} after checking the canaries; the caller has synchronised"""
        b = self.dev.cpu().numpy()
        bad = np.flatnonzero((b != self.template_np) & self.mask)
        assert bad.size == 0, f"canary bytes changed at {bad[:8]}"
        kinds = {"syndrome": np.uint32, "hyp": np.uint64, "counts": np.uint32, "dev_faults": np.uint32, "bad_count": np.uint32}
        return {name: b[o:o + ln].copy().view(kinds.get(name, np.uint8)) for name, (o, ln) in self.off.items()}


class Rig:
    """one arena of consistent stripes rotated onto its devices, a plan and the outputs"""

    def __init__(self, torch, code, packet, size, layout, n_shift, first, nstripes=None):
        self.torch, self.code, self.packet, self.size = torch, code, packet, size
        _, self.k, self.m, _ = TC.spec(code)
        self.n = self.k + self.m
        self.nstripes = nstripes = nstripes or 2 * self.n + 1  # every rotation class at least twice, no multiple of n
        self.n_shift, self.first = n_shift, first
        self.full = TC.stripes(code, packet, size, nstripes)
        self.lay = LY.plan_layout(layout, self.k, self.m, nstripes, size, outputs=range(self.k, self.n))
        LY.check_layout(self.lay)
        before, _ = LY.images(self.lay, physical(self.full, n_shift, first), ())
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, before)
        self.orig = self.arena.clone()
        self.outs = Outs(torch, nstripes, self.n)
        self.plan = TC.make_plan(code, packet, size)
        self.flips, self.chunks = {}, {}  # stripe -> what its LOGICAL view holds beside the reference bytes
        self.tag = f"{code} C={size} {layout} n_shift={n_shift} first={first}"

    def close(self):
        self.plan.close()

    def rot(self, s):
        return rot_of(self.n, self.n_shift, self.first, s)

    def chunk_on(self, s, d):
        return (d + self.rot(s)) % self.n

    def dev_of(self, s, c):
        return (c - self.rot(s)) % self.n

    def flip(self, s, d, b, v=FLIP):
        """XOR v into byte b of what DEVICE d holds for stripe s (a second call with the same v undoes it)"""
        a = self.lay.start(d, s) + b
        self.arena[a:a + 1].bitwise_xor_(v)
        TL.Rig.note(self.flips.setdefault(s, []), (self.chunk_on(s, d), b, v))

    def flip_chunk(self, s, d):
        a = self.lay.start(d, s)
        self.arena[a:a + self.size].bitwise_xor_(0xFF)
        TL.Rig.note(self.chunks.setdefault(s, []), self.chunk_on(s, d))

    def want(self):
        """the expected outputs of the arena as it is, from the yardstick on each stripe's logical view"""
        n, k, N = self.n, self.k, self.nstripes
        syn, hyp = np.zeros(N, np.uint32), np.full(N, (1 << k) - 1, np.uint64)
        loc = np.full(N, CLEAN, np.uint8)
        for s in range(N):
            fl, ch = sorted(self.flips.get(s, [])), sorted(self.chunks.get(s, []))
            if not fl and not ch:
                continue
            st = self.full[s].copy()
            for i, b, v in fl:
                st[i, b] ^= v
            for i in ch:
                st[i] ^= 0xFF
            syn[s], hyp[s], loc[s] = TL.expected(self.code, self.packet, st, (N, s, tuple(fl), tuple(ch)))
        dev = loc.copy()
        for s in np.flatnonzero(loc < n):
            dev[s] = self.dev_of(int(s), int(loc[s]))
        return {"syndrome": syn, "hyp": hyp, "located": loc, "located_dev": dev,
                "counts": np.array([(loc < n).sum(), (loc == MANY).sum()], np.uint32),
                "dev_faults": np.bincount(dev[dev < n], minlength=n).astype(np.uint32),
                "bad_count": np.array([(syn != 0).sum()], np.uint32)}

    def locate(self, repair=False, stream=None, null=()):
        """one locate call; `null`: the optional outputs passed as NULL"""
        torch, o = self.torch, self.outs
        o.arm()
        ptr = lambda name: 0 if name in null else o.ptr(name)
        self.plan.locate_dev_rotated_refs(self.refs, self.nstripes, self.size, self.n_shift, self.first, o.ptr("syndrome"),
                                          o.ptr("hyp"), o.ptr("located"), ptr("located_dev"), ptr("counts"), ptr("dev_faults"),
                                          repair, stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return o.read()

    def check(self, null=()):
        torch, o = self.torch, self.outs
        o.arm()
        self.plan.check_dev_rotated_refs(self.refs, self.nstripes, self.size, self.n_shift, self.first, o.ptr("syndrome"),
                                         0 if "bad_count" in null else o.ptr("bad_count"), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return o.read()

    def same(self, got, want, names, what=""):
        for name in names:
            assert np.array_equal(got[name], want[name]), f"{self.tag} {what}: {name} {got[name]} != {want[name]}"

    def untouched(self, got, names):
        for name in names:
            assert (got[name].view(np.uint8) == FILL).all(), f"{self.tag}: {name} was written"

    def expect(self, what=""):
        """a locate and a check call, neither repairing, over the arena as it is: the outputs are the yardstick's
        and the arena is unchanged; returns the expected outputs"""
        before = self.arena.clone()
        want = self.want()
        got = self.locate()
        self.same(got, want, NAMES, what)
        self.untouched(got, ("bad_count",))
        got = self.check()
        self.same(got, want, ("syndrome", "bad_count"), what + " (check)")
        self.untouched(got, ("hyp", "located", "located_dev", "counts", "dev_faults"))
        assert self.torch.equal(self.arena, before), f"{self.tag} {what}: a call wrote into the arena"
        return want


# ---------------------------------------------------------------- 1, 2: consistent, then one byte per device
@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("code", list(CODES))
def test_consistent_then_one_byte_per_device(cuda, code, shift):
    import torch

    _, k, m, _ = CODES[code]
    n = k + m
    n_shift = shifts(n)[shift]
    for packet, size in shapes(code):
        for first in FIRSTS:
            rig = Rig(torch, code, packet, size, "off8", n_shift, first)
            try:
                want = rig.expect("consistent")
                assert not want["syndrome"].any() and (want["hyp"] == (1 << k) - 1).all() and (want["located"] == CLEAN).all()
                assert want["counts"].tolist() == [0, 0] and not want["dev_faults"].any()
                # device d corrupted in stripe d + 1: n consecutive stripes, so each of another rotation class
                # wherever the rotation has more than one; stripe 0 and the n stripes behind them stay clean
                pos = TC.positions(size)
                for d in range(n):
                    rig.flip(d + 1, d, pos[d % len(pos)])
                want = rig.expect("one byte per device")
                for d in range(n):
                    s = d + 1
                    assert want["located_dev"][s] == d and want["located"][s] == rig.chunk_on(s, d), (rig.tag, d, want)
                assert want["dev_faults"].tolist() == [1] * n and want["counts"].tolist() == [n, 0]
                assert want["located"][0] == CLEAN and (want["located"][n + 1:] == CLEAN).all() and int(want["bad_count"][0]) == n
            finally:
                rig.close()


@pytest.mark.parametrize("code", ["rs63", "rs164", "cg63"])
def test_whole_chunk_counts_once(cuda, code):
    """a whole chunk flipped, so that every wave of the stripe publishes, and a chunk hit in its first and last
    tile: the stripe is counted once by the check and by the locate, and the device once"""
    import torch

    _, k, m, _ = CODES[code]
    n = k + m
    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "mixed", 1, FIRSTS[1])
    try:
        rig.flip_chunk(2, 0)
        rig.flip_chunk(n + 2, 0)  # the same device and rotation, n stripes on
        rig.flip_chunk(5, n - 1)
        rig.flip(7, 3, 0)
        rig.flip(7, 3, size - 1)
        want = rig.expect()
        assert want["located_dev"][[2, n + 2, 5, 7]].tolist() == [0, 0, n - 1, 3]
        assert want["counts"].tolist() == [4, 0] and int(want["bad_count"][0]) == 4
        assert want["dev_faults"][[0, 3, n - 1]].tolist() == [2, 1, 1] and want["dev_faults"].sum() == 4
    finally:
        rig.close()


# ---------------------------------------------------------------- 3: LOCATE_MANY and parity alone
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_many_and_parity_only(cuda, code):
    import torch

    _, k, m, _ = CODES[code]
    n = k + m
    packet, size = shapes(code)[-1]
    for n_shift in (1, 3):
        rig = Rig(torch, code, packet, size, "packed", n_shift, FIRSTS[0])
        try:
            rig.flip(4, 1, 0)                 # two devices of one stripe: m = 3 reports LOCATE_MANY
            rig.flip(4, 6, size - 1, FLIP2)
            par = []
            for r in range(m):                # one byte of parity row r, on whichever device holds it in stripe 6 + r
                s = 6 + r
                par.append(rig.dev_of(s, k + r))
                rig.flip(s, par[-1], size // 2)
            want = rig.expect("many and parity")
            assert want["located"][4] == MANY and want["located_dev"][4] == MANY
            for r in range(m):
                s = 6 + r
                assert want["located"][s] == k + r and want["hyp"][s] == 0 and want["located_dev"][s] == par[r]
            assert want["counts"].tolist() == [m, 1] and want["dev_faults"].sum() == m
            assert want["dev_faults"].tolist() == np.bincount(par, minlength=n).tolist()
        finally:
            rig.close()


# ---------------------------------------------------------------- 5: repair
def corrupt_mixed(rig):
    """stripe 0: a byte on device n // 2; 1: clean; 2: a whole chunk on the last device; 3: two devices
    (LOCATE_MANY); 4: device 0 at its first and last byte; n + 1: a byte on device 1 -- and the located devices
    by stripe"""
    n, size = rig.n, rig.size
    rig.flip(0, n // 2, size // 3)
    rig.flip_chunk(2, n - 1)
    rig.flip(3, 0, 0)
    rig.flip(3, rig.k, size - 1)
    rig.flip(4, 0, 0)
    rig.flip(4, 0, size - 1)
    rig.flip(n + 1, 1, size - 1)
    return {0: n // 2, 2: n - 1, 4: 0, n + 1: 1}


def many_image(rig):
    """the arena after a repair of corrupt_mixed's damage: the original bytes, but stripe 3 as corrupted"""
    after = rig.orig.clone()
    for d, b in ((0, 0), (rig.k, rig.size - 1)):
        a = rig.lay.start(d, 3) + b
        after[a:a + 1].bitwise_xor_(FLIP)
    return after


@pytest.mark.parametrize("layout", ["packed", "off8", "mixed"])
@pytest.mark.parametrize("code", ["rs63", "r6_62", "rs164", "cg63"])
def test_repair(cuda, code, layout):
    """rs164 at n_shift 1: 20 chunks x 20 rotations = 400, past any table of (rotation, chunk) records"""
    import torch

    _, k, m, _ = CODES[code]
    n = k + m
    for packet, size in shapes(code)[1:] if len(shapes(code)) > 1 else shapes(code):
        rig = Rig(torch, code, packet, size, layout, 1, FIRSTS[1])
        try:
            devs = corrupt_mixed(rig)
            want = rig.want()
            assert {int(s): int(want["located_dev"][s]) for s in devs} == devs and want["located"][3] == MANY
            assert want["counts"].tolist() == [4, 1]
            corrupted = rig.arena.clone()
            after = many_image(rig)
            got = rig.locate(repair=True)
            rig.same(got, want, NAMES, "repair")
            # the located stripes hold the reference bytes again; the clean and the LOCATE_MANY stripes, the
            # gaps and the guard bands are byte for byte as before the call
            LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), after.cpu().numpy(), f"{rig.tag} repair")
            repaired = rig.arena.clone()
            # a second locate, not repairing, reports those stripes clean
            rig.flips = {3: rig.flips[3]}
            rig.chunks = {}
            again = rig.expect("after the repair")
            assert again["counts"].tolist() == [0, 1] and not again["dev_faults"].any()
            # the rebuilt bytes are those of lsec_decode_dev_rotated with that one device lost
            for s, d in devs.items():
                cp = corrupted.clone()
                rig.plan.decode_dev_rotated_refs(rig.lay.refs(cp.data_ptr()), rig.nstripes, size, [d], 1, FIRSTS[1],
                                                 torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                a = rig.lay.start(d, s)
                assert torch.equal(cp[a:a + size], repaired[a:a + size]), f"{rig.tag}: stripe {s} device {d}"
        finally:
            rig.close()


# ---------------------------------------------------------------- 4: launches split
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_launch_split(cuda, code):
    """four stripes per launch (the test hook), n_shift 1: 4 is no divisor of n, so every launch starts at
    another rotation.  Outputs and repaired bytes equal the unsplit run's and the yardstick's."""
    import torch

    packet, size = shapes(code)[-1]
    runs = []
    try:
        for split in (0, 4):
            E.set_pattern_split(split)
            rig = Rig(torch, code, packet, size, "off8", 1, FIRSTS[1])
            try:
                corrupt_mixed(rig)
                rig.flip(rig.nstripes - 1, 2, 1)  # the last launch's last stripe
                want = rig.expect(f"split {split}")
                got = rig.locate(repair=True)
                rig.same(got, want, NAMES, f"split {split}, repair")
                LY.assert_arena(rig.lay, rig.arena.cpu().numpy(), many_image(rig).cpu().numpy(), f"{rig.tag} split {split}")
                runs.append((got, rig.arena.cpu().numpy()))
            finally:
                rig.close()
    finally:
        E.set_pattern_split(0)
    for name in NAMES:
        assert np.array_equal(runs[0][0][name], runs[1][0][name]), name
    assert np.array_equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------- 6: the unrotated calls (engine against engine)
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_consistent_with_the_unrotated_calls(cuda, code):
    """ENGINE AGAINST ENGINE: lsec_locate_dev once per rotation class, over refs permuted into the logical
    order of that class (the way test_rotated_degraded_read cross-checks the decode), gives on the stripes of
    the class what the one rotated call gives"""
    import torch

    _, k, m, _ = CODES[code]
    n = k + m
    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "mixed", 1, FIRSTS[1])
    try:
        corrupt_mixed(rig)
        rig.flip(9, 5, 3)
        got = rig.locate()
        plain = TL.Outs(torch, rig.nstripes)
        for rot in range(n):
            mine = [s for s in range(rig.nstripes) if rig.rot(s) == rot]
            assert len(mine) >= 2
            plain.arm()
            rig.plan.locate_dev_refs([rig.refs[(c - rot) % n] for c in range(n)], rig.nstripes, size, plain.syndrome_ptr,
                                     plain.hyp_ptr, plain.located_ptr, 0, False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            syn, hyp, loc, _ = plain.read()
            for name, arr in (("syndrome", syn), ("hyp", hyp), ("located", loc)):
                assert np.array_equal(arr[mine], got[name][mine]), f"{rig.tag} rotation {rot}: {name}"
    finally:
        rig.close()


# ---------------------------------------------------------------- 7: stream order
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_follows_a_write_on_its_stream(cuda, code):
    """a torch op on a non-default stream corrupts a byte and the call, with repair, is queued straight
    behind it, no synchronisation in between: the corruption is seen and undone"""
    import torch

    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "packed", 1, FIRSTS[0])
    try:
        st = torch.cuda.Stream()
        rig.outs.arm()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            rig.flip(3, 1, size - 1)
        o = rig.outs
        rig.plan.locate_dev_rotated_refs(rig.refs, rig.nstripes, size, 1, FIRSTS[0], o.ptr("syndrome"), o.ptr("hyp"),
                                         o.ptr("located"), o.ptr("located_dev"), o.ptr("counts"), o.ptr("dev_faults"), True,
                                         st.cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        want = rig.want()
        got = o.read()
        rig.same(got, want, NAMES, "behind a write on its stream")
        assert got["located_dev"][3] == 1 and got["counts"].tolist() == [1, 0] and got["dev_faults"][1] == 1
        assert torch.equal(rig.arena, rig.orig)
    finally:
        rig.close()


# ---------------------------------------------------------------- 8: optional outputs
@pytest.mark.parametrize("code", ["rs63", "cg63"])
def test_optional_outputs_null(cuda, code):
    import torch

    packet, size = shapes(code)[-1]
    rig = Rig(torch, code, packet, size, "off8", 3, FIRSTS[1])
    try:
        corrupt_mixed(rig)
        want = rig.want()
        for skip in ("located_dev", "counts", "dev_faults"):
            got = rig.locate(null=(skip,))
            rig.same(got, want, [name for name in NAMES if name != skip], f"{skip} NULL")
            rig.untouched(got, (skip, "bad_count"))
        got = rig.locate(null=("located_dev", "counts", "dev_faults"))
        rig.same(got, want, ("syndrome", "hyp", "located"), "all three NULL")
        got = rig.check(null=("bad_count",))
        rig.same(got, want, ("syndrome",), "bad_count NULL")
        rig.untouched(got, ("bad_count", "hyp", "located", "located_dev", "counts", "dev_faults"))
    finally:
        rig.close()


# ---------------------------------------------------------------- 9: persistent-grid path
def test_persistent_grid_all_tile_modes(cuda):
    """16384 tiles (kTileQueueMinTiles): RS(6+3), C = 16 KiB, 8192 stripes, as test_gpu_locate's.  Data from
    torch.randint, parity from lsec_encode_dev (pinned bit-exact to the reference by the rest of the suite), the
    stripes rotated onto their devices by a gather; a dozen stripes over the range are corrupted, their expected
    outputs come from the reference on their logical views.  Static, shared and tail tiles give the same outputs,
    from the check too; the last mode's call repairs."""
    import torch

    code, size, nstr, n_shift, first = "rs63", 16384, 8192, 1, FIRSTS[1]
    _, k, m, _ = CODES[code]
    n = k + m
    rots = (first + np.arange(nstr)) * n_shift % n
    outs = Outs(torch, nstr, n)
    hit = [0, 1, 700, 1023, 1024, 2049, 4095, 4096, 5555, 7000, 8190, 8191]
    mode0 = E.tile_sharing()
    try:
        with TC.make_plan(code, 0, size) as p:
            logical = torch.empty((nstr, n, size), dtype=torch.uint8, device="cuda")
            logical[:, :k] = torch.randint(0, 256, (nstr, k, size), dtype=torch.uint8, device="cuda")
            p.encode_dev_refs([(logical.data_ptr() + i * size, n * size) for i in range(n)], nstr, size,
                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            # device i holds logical chunk (i + rot_s) mod n of stripe s
            idx = torch.from_numpy((np.arange(n)[None, :] + rots[:, None]) % n).cuda()
            phys = logical[torch.arange(nstr, device="cuda")[:, None], idx].contiguous()
            del logical, idx
            good = phys.clone()
            syn_w, hyp_w = np.zeros(nstr, np.uint32), np.full(nstr, (1 << k) - 1, np.uint64)
            loc_w = np.full(nstr, CLEAN, np.uint8)
            for j, s in enumerate(hit):
                if j % 4 == 0:
                    phys[s, j % n, (j * 1361) % size] ^= 0x10     # one byte of one device
                elif j % 4 == 1:
                    phys[s, (j + 3) % n, size - 1 - j] ^= 0x01
                elif j % 4 == 2:
                    phys[s, j % n, j] ^= 0x80                     # one device in its first and last tile
                    phys[s, j % n, size - 1] ^= 0x80
                else:
                    phys[s, 0, j] ^= 0x80                         # two devices
                    phys[s, n - 1, size - 1] ^= 0x80
                stored = phys[s].cpu().numpy()[(np.arange(n) - rots[s]) % n]  # the logical view: chunk c from device c - rot
                syn_w[s], hyp_w[s], loc_w[s] = TL.expected(code, 0, stored, ("rotated grid", s))
            dev_w = loc_w.copy()
            dev_w[loc_w < n] = (loc_w[loc_w < n].astype(np.int64) - rots[loc_w < n]) % n
            want = {"syndrome": syn_w, "hyp": hyp_w, "located": loc_w, "located_dev": dev_w,
                    "counts": np.array([(loc_w < n).sum(), (loc_w == MANY).sum()], np.uint32),
                    "dev_faults": np.bincount(dev_w[dev_w < n], minlength=n).astype(np.uint32),
                    "bad_count": np.array([len(hit)], np.uint32)}
            assert want["counts"].tolist() == [9, 3]
            p0 = phys.clone()
            refs = [(phys.data_ptr() + i * size, n * size) for i in range(n)]
            stream = torch.cuda.current_stream().cuda_stream
            modes = (E.TILES_STATIC, E.TILES_SHARED, E.TILES_TAIL)
            for mode in modes:
                E.set_tile_sharing(mode)
                outs.arm()
                p.check_dev_rotated_refs(refs, nstr, size, n_shift, first, outs.ptr("syndrome"), outs.ptr("bad_count"), stream)
                torch.cuda.synchronize()
                got = outs.read()
                for name in ("syndrome", "bad_count"):
                    assert np.array_equal(got[name], want[name]), f"tile mode {mode}: check {name}"
                outs.arm()
                repair = mode == modes[-1]
                p.locate_dev_rotated_refs(refs, nstr, size, n_shift, first, outs.ptr("syndrome"), outs.ptr("hyp"),
                                          outs.ptr("located"), outs.ptr("located_dev"), outs.ptr("counts"),
                                          outs.ptr("dev_faults"), repair, stream)
                torch.cuda.synchronize()
                got = outs.read()
                for name in NAMES:
                    diff = np.flatnonzero(got[name] != want[name])
                    assert diff.size == 0, f"tile mode {mode}: {name} at {diff[:8]} got {got[name][diff[:8]]} want {want[name][diff[:8]]}"
                if not repair:
                    assert torch.equal(phys, p0), f"tile mode {mode}: the call wrote into the devices"
            # repaired: the located stripes hold the encode's bytes again, the LOCATE_MANY ones are as they were
            many = torch.from_numpy(np.flatnonzero(loc_w == MANY)).cuda()
            good[many] = p0[many]
            assert torch.equal(phys, good)
    finally:
        E.set_tile_sharing(mode0)
