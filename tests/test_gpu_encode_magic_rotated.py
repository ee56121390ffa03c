"""GPU: lsec_encode_magic_dev_rotated, the full-stripe write over the physical devices of a rotated LUN that also
leaves each stripe's 4-byte adler32 magic.

Bar: bit-exact.  The yardstick is never the engine: logical stripes come from test_gpu_check.stripes (oracle/_ref when
it is built, else the oracle restatement), so the expected parity is test_gpu_check.ref_encode's, computed on the CPU;
the expected magic is zlib.adler32 over the LOGICAL reference stripe -- data 0..k-1, then the parity rows -- whatever
the rotation; the logical stripes are rotated onto the devices on the host by test_gpu_rotated_scrub.physical.  Only
test_unrotated_is_encode_magic_dev and the tile-sharing test compare engine with engine, and say so.

Devices live in the arenas of tests/layouts.py (canary gaps and guard bands), shard i of the layout as device i.
Before each call the parity positions hold noise and the magic words a non-zero fill, in a byte buffer at an odd
address between canary bytes.  After each call
  * the WHOLE device arena equals the reference image: parity at the rotated positions, every data chunk, every gap
    and both guard bands unchanged,
  * every magic word equals zlib's, and the canaries are intact,
  * the launch record names the predicted form of the new family once per launch.

Stripes per call: k + m + 2, so the rotation wraps.  Sizes: the smallest at which the sums or the stores can go wrong,
from the predicted form's tile (a half unit, one unit, one full tile, a ragged tile behind a full one, a ragged tile
behind three); bit-sliced test_gpu_update_masked.shapes, and for K >= 16 test_gpu_check's shapes of the wide lanes.
"""
import functools
import zlib

import numpy as np
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import layouts as LY
import scrub_forms as SF
import test_gpu_check as TC
import test_gpu_check_magic as TCM
import test_gpu_decode_magic as TDM
import test_gpu_rotated_scrub as TR
import test_gpu_rotated_write as TRW
import test_gpu_update_magic as TUM
import test_gpu_update_masked as TM

pytestmark = pytest.mark.gpu

NAMES = ("rs63", "r6_62", "rs52", "rs128", "rs164", "raid4_61", "cg63", "co42", "cg164")
CODES = {c: TC.CODES[c] for c in NAMES}
EDGES = TCM.EDGES  # rs648 / cg648: chunk ids up to 71, the largest position weights of the lane sums
LAYOUTS = ("packed", "off8", "mixed")
FIRSTS, NOISE, SPLIT = TRW.FIRSTS, TRW.NOISE, 3


def spec(code):
    """(method, k, m, packet) of a code: a name of CODES or EDGES, or the tuple itself (tests/scrub_forms.py's plans)"""
    if not isinstance(code, str):
        return tuple(code)
    return CODES[code] if code in CODES else EDGES[code]


def sliced(code):
    return spec(code)[3] != 0


def form_of(code, packet, size):
    _, k, m, _ = spec(code)
    return E.predict_encode_magic_form(2 if sliced(code) else 1, k, m, packet, size)


def shapes(code):
    """(packet, C), chosen as test_gpu_check_magic.shapes chooses them, from the new family's predicted form"""
    if not sliced(code):
        tile = SF.tile_bytes(form_of(code, 0, 8192))
        return [(0, c) for c in (8, 16, tile, tile + 8, 3 * tile + 8)]
    out = list(TM.shapes(code))
    if spec(code)[1] >= 16:
        out += [s for s in TC.SLICED_SIZES_K16 if s not in out]
    return out


def edge_shape(code):
    """the one size of an edge code: a full tile and a ragged one behind it"""
    _, _, _, packet = spec(code)
    tile = SF.tile_bytes(form_of(code, packet, 8 * packet if packet else 8))
    if not packet:
        return 0, tile + 8
    return packet, 8 * (-(-tile // packet) * packet + packet)


@functools.lru_cache(maxsize=None)
def reference(code, packet, size):
    """(the reference's logical stripes [N, k+m, C], zlib's magic of each): computed once, never modified"""
    _, k, m, _ = spec(code)
    full = TC.stripes(spec(code), packet, size, k + m + 2)
    return full, tuple(zlib.adler32(full[s].tobytes()) & 0xFFFFFFFF for s in range(full.shape[0]))


class Bench:
    """the devices of a rotated LUN in one arena, a plan, and the call over them"""

    def __init__(self, torch, code, packet, size, layout):
        self.torch, self.code, self.packet, self.size = torch, code, packet, size
        _, self.k, self.m, _ = spec(code)
        self.n, self.nstripes = self.k + self.m, self.k + self.m + 2
        self.full, self.words = reference(code, packet, size)
        self.lay = LY.plan_layout(layout, self.k, self.m, self.nstripes, size, outputs=range(self.k, self.n))
        LY.check_layout(self.lay)
        self.arena, self.refs, _ = LY.to_device(torch, self.lay, np.full(self.lay.total, LY.GARBAGE, np.uint8))
        self.plan = TC.make_plan(spec(code), packet, size)
        self.form = form_of(code, packet, size)
        self.entry = [0xDEAD0000 + 0x1111 * s for s in range(self.nstripes)]  # the words on entry: pure output
        self.tag = f"{code} packet={packet} C={size} {layout}"

    def close(self):
        self.plan.close()

    def image(self, logical, n_shift, first):
        """the arena holding the logical stripes [N, k+m, C] on the devices of that rotation"""
        return LY.images(self.lay, TR.physical(logical, n_shift, first), ())[0]

    def noisy(self):
        """the logical stripes with noise where the parity belongs"""
        v = self.full.copy()
        v[:, self.k:] = NOISE
        return v

    def arm(self, image):
        self.arena.copy_(self.torch.from_numpy(image))

    def call(self, n_shift, first, magic_ptr, stream=None, size=None):
        st = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.plan.encode_magic_dev_rotated_refs(self.refs, self.nstripes, self.size if size is None else size, n_shift, first,
                                                magic_ptr, st)

    def run(self, n_shift, first, split=0):
        """the call, then every assertion of the module's docstring -> (arena, magic words)"""
        torch = self.torch
        what = f"{self.tag} n_shift={n_shift} first={first} split={split}"
        self.arm(self.image(self.noisy(), n_shift, first))
        magics = TUM.Magics(torch, self.entry, odd=True)
        torch.cuda.synchronize()
        E.set_pattern_split(split)
        try:
            self.call(n_shift, first, magics.ptr)
            forms = E.launch_record()
        finally:
            E.set_pattern_split(0)
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        LY.assert_arena(self.lay, got, self.image(self.full, n_shift, first), what)
        magics.assert_words(self.words, what)
        launches = -(-self.nstripes // split) if split else 1
        assert forms == [self.form] * launches, (what, forms)
        assert self.form.family == "encmagicrot"
        return got, [int(w) for w in magics.dev.cpu().numpy()[magics.lead:-TUM.PAD].view("<u4")]


# ---------------------------------------------------------------- 1. every form, every rotation
@pytest.mark.parametrize("code", NAMES)
def test_every_form_and_rotation(cuda, code):
    """random logical data on the devices, noise where the parity belongs: one call leaves the reference's parity at
    the rotated positions, everything else as it was, and zlib's magic of every logical stripe.  n_shift = 0 is among
    the shifts: bytes and magics equal the reference, which is therefore what lsec_encode_magic_dev gives"""
    import torch

    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, "packed")
        try:
            for n_shift in TRW.shifts(bench.n):
                for first in FIRSTS:
                    bench.run(n_shift, first)
        finally:
            bench.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("code", NAMES)
def test_layouts(cuda, code, layout):
    import torch

    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, layout)
        try:
            bench.run(1, FIRSTS[1])
        finally:
            bench.close()


@pytest.mark.parametrize("code", tuple(EDGES))
def test_widest_stripes(cuda, code):
    """RS(64+8) and Cauchy-good(64+8, packet 8): 72 chunks, chunk id 71"""
    import torch

    packet, size = edge_shape(code)
    bench = Bench(torch, code, packet, size, "off8")
    try:
        bench.run(5, FIRSTS[0])
        bench.run(1, FIRSTS[1], split=SPLIT * 8)
    finally:
        bench.close()


# ---------------------------------------------------------------- 2. split launches
@pytest.mark.parametrize("code", ("rs63", "rs128", "rs164", "cg63", "cg164"))
def test_split_launches(cuda, code):
    """lsec_test_set_pattern_split(3) cuts the call into launches of three stripes, each with its own rot0, refs and
    accumulator offset, and the one finalize launch covers the whole call: the same bytes and magics, and
    ceil(N / 3) launch records"""
    import torch

    for packet, size in shapes(code)[-2:]:
        bench = Bench(torch, code, packet, size, "mixed")
        try:
            for n_shift, first in ((1, FIRSTS[0]), (TRW.shifts(bench.n)[2], FIRSTS[1]), (bench.n + 1, FIRSTS[1])):
                one, parts = bench.run(n_shift, first), bench.run(n_shift, first, split=SPLIT)
                assert np.array_equal(one[0], parts[0]) and one[1] == parts[1]
        finally:
            E.set_pattern_split(0)
            bench.close()


# ---------------------------------------------------------------- 3. n_shift = 0
@pytest.mark.parametrize("code", ("rs63", "rs128", "raid4_61", "cg63", "cg164"))
def test_unrotated_is_encode_magic_dev(cuda, code):
    """ENGINE AGAINST ENGINE (and both against the reference and zlib): at n_shift = 0 the bytes and the magics are
    lsec_encode_magic_dev's over the same refs -- for Cauchy whichever kernel or network that call picks"""
    import torch

    for packet, size in shapes(code):
        bench = Bench(torch, code, packet, size, "off8")
        try:
            arena, words = bench.run(0, FIRSTS[1])
            bench.arm(bench.image(bench.noisy(), 0, 0))
            magics = TUM.Magics(torch, bench.entry, odd=True)
            bench.plan.encode_magic_dev_refs(bench.refs, bench.nstripes, size, magics.ptr, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(bench.arena.cpu().numpy(), arena), bench.tag
            magics.assert_words(words, bench.tag)
        finally:
            bench.close()


# ---------------------------------------------------------------- 4. block_size = 0
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_empty_chunks(cuda, code):
    """block_size == 0: every magic word is adler32 of nothing, no chunk is touched, nothing but the finalize launches"""
    import torch

    packet, size = shapes(code)[0]
    bench = Bench(torch, code, packet, size, "packed")
    try:
        before = bench.image(bench.noisy(), 1, FIRSTS[0])
        bench.arm(before)
        magics = TUM.Magics(torch, bench.entry, odd=True)
        torch.cuda.synchronize()
        bench.call(1, FIRSTS[0], magics.ptr, size=0)
        assert E.launch_record() == []
        torch.cuda.synchronize()
        assert zlib.adler32(b"") == 1
        magics.assert_words([1] * bench.nstripes, "empty")
        LY.assert_arena(bench.lay, bench.arena.cpu().numpy(), before, "empty")
    finally:
        bench.close()


# ---------------------------------------------------------------- 5. stream order
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_on_a_stream_of_its_own_then_checked(cuda, code):
    """the call behind a copy_ of its inputs on a non-default stream, and behind it on that stream
    lsec_check_magic_dev_rotated with `expect` set to the call's own magics, nothing waited for in between: syndromes 0,
    bad all 0, counts (0, 0) -- the expected values come from the contract, not from the engine -- and the check's own
    magics are zlib's too"""
    import torch

    packet, size = shapes(code)[-1]
    n_shift, first = 1, FIRSTS[1]
    bench = Bench(torch, code, packet, size, "off8")
    try:
        noisy = torch.from_numpy(bench.image(bench.noisy(), n_shift, first)).cuda()
        magics = TUM.Magics(torch, bench.entry, odd=True)
        again = TUM.Magics(torch, bench.entry)
        words = TCM.Words(torch, bench.nstripes)
        bad = TDM.Bytes(torch, np.full(bench.nstripes, TCM.BAD_FILL, np.uint8), odd=True)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            bench.arena.copy_(noisy, non_blocking=True)
            bench.call(n_shift, first, magics.ptr, stream=st.cuda_stream)
            bench.plan.check_magic_dev_rotated_refs(bench.refs, bench.nstripes, size, n_shift, first, words.syndrome_ptr, again.ptr,
                                                    magics.ptr, bad.ptr, words.counts_ptr, st.cuda_stream)
        torch.cuda.synchronize()
        what = f"on a stream {bench.tag}"
        LY.assert_arena(bench.lay, bench.arena.cpu().numpy(), bench.image(bench.full, n_shift, first), what)
        magics.assert_words(bench.words, what)
        again.assert_words(bench.words, what)
        assert words.read(what) == ([0] * bench.nstripes, [0, 0])
        assert bad.body(what).tolist() == [0] * bench.nstripes
    finally:
        bench.close()


# ---------------------------------------------------------------- 6. the torch form
def test_torch_form(cuda):
    import torch

    code, size, n_shift, first = "rs63", 4096, 2, 3
    full, words = reference(code, 0, size)
    k = spec(code)[1]
    noisy = full.copy()
    noisy[:, k:] = NOISE
    with TC.make_plan(spec(code), 0, size) as p:
        devs = torch.from_numpy(np.ascontiguousarray(TR.physical(noisy, n_shift, first).transpose(1, 0, 2))).cuda()
        magic = torch.zeros(4 * full.shape[0], dtype=torch.uint8, device="cuda")
        p.encode_magic_dev_rotated(devs, n_shift, first, magic)
        torch.cuda.synchronize()
        assert np.array_equal(devs.cpu().numpy().transpose(1, 0, 2), TR.physical(full, n_shift, first))
        assert magic.cpu().numpy().view("<u4").tolist() == list(words)
        with pytest.raises(ValueError):
            p.encode_magic_dev_rotated(devs, n_shift, first, magic[:-1])


# ---------------------------------------------------------------- 7. tile sharing
@pytest.mark.parametrize("code", ("rs63", "cg63"))
def test_tile_sharing_modes(cuda, code):
    """engine against engine: static eighths, shared tiles and the static prefix with a shared tail leave identical
    arenas and magics (each also compared with the reference's and zlib's)"""
    import torch

    packet, size = shapes(code)[-1]
    bench = Bench(torch, code, packet, size, "mixed")
    mode = E.tile_sharing()
    try:
        got = []
        for m in (E.TILES_STATIC, E.TILES_SHARED, E.TILES_TAIL):
            E.set_tile_sharing(m)
            got.append(bench.run(1, FIRSTS[1]))
        assert all(np.array_equal(got[0][0], g[0]) and got[0][1] == g[1] for g in got[1:])
    finally:
        E.set_tile_sharing(mode)
        bench.close()
