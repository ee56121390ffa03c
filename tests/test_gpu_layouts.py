"""GPU: the device-resident calls on strided, offset, guard-banded shards (tests/layouts.py).

lsec_encode_dev, lsec_decode_dev, lsec_encode_magic_dev and lsec_stripe_magic_dev take every shard
as {base, stride} with one rule: multiples of 8 bytes.  Each kernel family, each path the dispatch
picks by alignment, and the stripe magic run here on layouts a caller may pass -- LStore's packed
one, which misaligns odd shards when C % 16 == 8; every shard at 8 mod 16; inputs and outputs
aligned differently with a stride per shard; aligned but not contiguous -- and the WHOLE arena is
compared: outputs bit-exact against the reference (oracle/_ref when built, else the oracle
restatement), every survivor, every gap and both guard bands untouched.

Which path ran is asserted, not assumed (E.apply_path): a case with a compiled network is prepared
first, so the path is fixed and no race with the background compile; the generic kernel of the same
shape is reached by alignment (pkt_aligned false) or through E.set_kernel_variant.

Sizes: the smallest with two tiles of the family's widest tile and a ragged last lane.  Tile sizes
read from the code: bytewise 256 lanes x 32 B (2 x 16 B) = 8 KiB, 4 KiB at 16 B per lane; bit-sliced
256 x 4 x dw column bytes; k_bitmatrix / k_gfw_bitsliced 1 KiB of column bytes; GF(2^16) / GF(2^32)
transposed 256 x 4 x w = 16 KiB / 32 KiB, and gfw_tile(32, 3) = 32 KiB for the three-row network:
all as the sizes below assume.
"""
import zlib
from collections import namedtuple

import numpy as np
import pytest

import layouts as LY
import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

pytestmark = pytest.mark.gpu

NSTRIPES = 5
GENERIC, NET, PKT = E.PATH_GENERIC, E.PATH_NETWORK, E.PATH_PACKET_NETWORK

# path: "auto" = no network exists for the shape's calls, the default dispatch is fixed;
#       "variant" = wants_xornet / wants_gfw_net / wants_pktnet holds but the kernel under test is the
#                   generic one: run under set_kernel_variant(0, 1), which turns networks off;
#       "net" = prepared, the network asserted (expected_path)
Case = namedtuple("Case", "id family method k m w packet size erasures path")
CASES = [
    Case("rs63", "bytewise", L.REED_SOL_VAN, 6, 3, 8, 0, 16392, ([0], [7], [1, 7], [0, 3, 5]), "auto"),
    Case("rs164", "bytewise", L.REED_SOL_VAN, 16, 4, 8, 0, 8200, ([16], [0, 16], [1, 2, 3, 17]), "auto"),
    Case("rs1210", "bytewise", L.REED_SOL_VAN, 12, 10, 8, 0, 8200, (list(range(10)),), "auto"),
    Case("rs704", "bytewise", L.REED_SOL_VAN, 70, 4, 8, 0, 4104, ([0, 65, 70],), "auto"),
    Case("r6", "r6raid4", L.REED_SOL_R6_OP, 6, 2, 8, 0, 16392, ([0, 6], [6, 7]), "auto"),
    Case("raid4", "r6raid4", L.RAID4, 4, 1, 8, 0, 4104, ([0], [4]), "auto"),
    Case("cauchy63", "bitsliced", L.CAUCHY_GOOD, 6, 3, 8, 24, 8 * 24 * 43, ([0], [1, 7], [2, 6, 7]), "auto"),
    Case("cauchy164", "bitsliced", L.CAUCHY_GOOD, 16, 4, 8, 64, 8 * 64 * 65, ([0, 16],), "auto"),
    Case("cauchy206", "cauchy8net", L.CAUCHY_GOOD, 20, 6, 8, 32, 8 * 32 * 33, ([0, 20],), "net"),
    Case("liberation7", "bitmatrix", L.LIBERATION, 7, 2, 7, 40, 7 * 40 * 33, ([0], [7], [0, 6], [7, 8]), "variant"),
    Case("blaumroth6", "bitmatrix", L.BLAUM_ROTH, 6, 2, 6, 24, 6 * 24 * 50, ([0], [6], [0, 5], [6, 7]), "variant"),
    Case("liber8tion8", "bitmatrix", L.LIBER8TION, 8, 2, 8, 64, 8 * 64 * 24, ([0], [8], [0, 7], [8, 9]), "net"),
    Case("rs63w16", "gf16", L.REED_SOL_VAN, 6, 3, 16, 0, 2 * 16384 + 8, ([0, 1, 2],), "variant"),
    Case("rs129w32", "gf32", L.REED_SOL_VAN, 12, 9, 32, 0, 4104, ([0, 12],), "variant"),
    Case("rs53w32", "gf32net", L.REED_SOL_VAN, 5, 3, 32, 0, 32768 + 4104, ([0, 2, 4],), "net"),
    Case("cauchy63w16", "gfwbitsliced", L.CAUCHY_GOOD, 6, 3, 16, 64, 16 * 64 * 17, ([1, 6],), "variant"),
    Case("cauchy104w32", "gfwbitsliced", L.CAUCHY_GOOD, 10, 4, 32, 32, 32 * 32 * 33, ([1, 10],), "variant"),
]
BY_ID = {c.id: c for c in CASES}
LIBERATION_FAMILY = (L.LIBERATION, L.BLAUM_ROTH, L.LIBER8TION)


def case_layouts():
    """every case on packed and off8; the mixed layouts and aligned_gap on the first case of each
    family and on every case with a network"""
    seen, out = set(), []
    for c in CASES:
        wide = c.family not in seen or c.path == "net"
        seen.add(c.family)
        for name in LY.LAYOUTS if wide else ("packed", "off8"):
            out.append(pytest.param(c.id, name, id=f"{c.id}-{name}"))
    return out


_ref_cache = {}


def reference_chunks(method, k, m, w, packet, size, nstripes=NSTRIPES, fill=None):
    """uint8 [N, k+m, C], computed once per shape, never modified: seeded random data, stripe 1 all
    0xFF, stripe 2 zero but for one set bit in the last byte of the last data chunk (fill: every
    data byte that value instead), and the reference's parity"""
    key = (method, k, m, w, packet, size, nstripes, fill)
    if key not in _ref_cache:
        if method in LIBERATION_FAMILY and not O.ref_available():
            pytest.skip("oracle/_ref not built")  # O.encode has no matrix for the liberation family
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        full = np.empty((nstripes, k + m, size), np.uint8)
        full[:, :k] = rng.integers(0, 256, (nstripes, k, size), dtype=np.uint8)
        if fill is not None:
            full[:, :k] = fill
        elif nstripes >= 3:
            full[1, :k] = 0xFF
            full[2, :k] = 0
            full[2, k - 1, size - 1] = 0x80
        rp = O.RefPlan(method, k, m, w, packet) if O.ref_available() else None
        for s in range(nstripes):
            full[s, k:] = rp.encode(full[s, :k]) if rp else O.encode(method, full[s, :k], m, packet, w)
        if rp:
            rp.close()
        full.setflags(write=False)
        _ref_cache[key] = full
    return _ref_cache[key]


def reference_of(c):
    return reference_chunks(c.method, c.k, c.m, c.w, c.packet, c.size)


def make_plan(c):
    p = L.Plan.new(c.method, c.size, c.k, c.m, c.w, c.packet, 1 if c.method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


def je_magic(full):
    """je_cksum_calc: adler32 over the k+m chunks in order, 4 bytes little-endian (zlib)"""
    a = 1
    for row in full:
        a = zlib.adler32(row.tobytes(), a)
    return np.frombuffer(np.uint32(a).tobytes(), dtype=np.uint8)


def aligned16(lay, ids):
    return all(lay.offsets[i] % 16 == 0 and lay.strides[i] % 16 == 0 for i in ids)


def expected_path(c, lay, nout, forced_generic):
    """PATH_* bits of one call that writes nout shards"""
    if c.path != "net" or forced_generic:
        return GENERIC
    if c.id == "rs53w32":
        return NET | GENERIC  # whole 32 KiB tiles on the network, the 4104-byte tail at base + 32768 generic
    if c.id == "cauchy206":
        # six outputs: the packet network (4-byte lanes: R * w * d <= 64 leaves d = 1, so every 8-byte
        # layout is aligned for it); up to four: the bit-sliced kernel (cauchy8_bitsliced_dw)
        return PKT if nout > 4 else GENERIC
    # liber8tion: two outputs on the packet network with 16-byte lanes (pkt_shape: 2 * 8 * 4 = 64),
    # which pkt_aligned grants only where every base and stride is 16-byte aligned; one output: k_bitmatrix
    return (PKT if aligned16(lay, range(lay.n)) else GENERIC) if nout == 2 else GENERIC


def run_call(torch, p, c, lay, full, outputs, call, what, keep=(), path=None):
    before, want = LY.images(lay, full, outputs, keep=keep)
    arena, refs, _ = LY.to_device(torch, lay, before)
    torch.cuda.synchronize()
    call(refs)
    torch.cuda.synchronize()
    LY.assert_arena(lay, arena.cpu().numpy(), want, f"{c.id} {what}")
    if path is not None:
        assert E.apply_path() == path, f"{c.id} {what} ({lay.name}): path {E.apply_path()}, expected {path}"


def effective(c, er):
    """the slots a pattern rebuilds (a raid4 pattern that loses only the parity rebuilds nothing)"""
    return [] if c.method == L.RAID4 and min(er) >= c.k else sorted(er)


def encode_and_decode(torch, c, layout, forced_generic):
    full = reference_of(c)
    n, size = NSTRIPES, c.size
    parity = list(range(c.k, c.k + c.m))
    with make_plan(c) as p:
        if c.path == "net" and not forced_generic:
            p.prepare_encode()
        lay = LY.plan_layout(layout, c.k, c.m, n, size, parity)
        path = expected_path(c, lay, c.m, forced_generic)
        if c.path == "net" and not forced_generic and path != GENERIC:
            assert p.jit() == 1, "network not compiled"
        run_call(torch, p, c, lay, full, parity, lambda refs: p.encode_dev_refs(refs, n, size), "encode", path=path)
        for er in c.erasures:
            if c.path == "net" and not forced_generic:
                p.prepare_decode(er)
            eff = effective(c, er)
            lay = LY.plan_layout(layout, c.k, c.m, n, size, er)
            path = expected_path(c, lay, len(er), forced_generic) if eff else None  # nothing rebuilt: nothing launched
            if path is not None and path != GENERIC:
                assert p.jit(er) == 1, f"network of {er} not compiled"
            run_call(torch, p, c, lay, full, er, lambda refs: p.decode_dev_refs(refs, n, size, er), f"decode {er}",
                     keep=set(er) - set(eff), path=path)


# ---------------------------------------------------------------- every family x layout
@pytest.mark.parametrize("case_id,layout", case_layouts())
def test_encode_decode_whole_arena(cuda, case_id, layout):
    import torch

    c = BY_ID[case_id]
    # cauchy206 on the 8-mod-16 layouts: its network takes them (4-byte lanes), so the generic
    # kernel of the shape is reached through the variant there and must give the same bytes
    forced = c.path == "variant" or (c.id == "cauchy206" and layout in ("off8", "mixed", "mixed_swapped"))
    if forced:
        E.set_kernel_variant(0, 1)
    try:
        encode_and_decode(torch, c, layout, forced)
    finally:
        E.set_kernel_variant(0, 0)


# ---------------------------------------------------------------- variant sweep
@pytest.mark.parametrize("b", [1, 2, 3, 4, 5])
def test_bytewise_launch_shapes(cuda, b):
    """all five bytewise launch shapes -- (2,4) (1,4) (2,2) (1,2) branch-free and (1,2) branchy; the
    automatic policy never picks (2,2) or branch-free (1,2) -- on RS(6+3) with every shard at 8 mod 16"""
    import torch

    E.set_kernel_variant(b, 0)
    try:
        encode_and_decode(torch, BY_ID["rs63"], "off8", True)
    finally:
        E.set_kernel_variant(0, 0)


@pytest.mark.parametrize("case_id,bs", [("cauchy63p64", 2), ("cauchy63p64", 4), ("rs129w32", 10)])
def test_bitsliced_variants(cuda, case_id, bs):
    """Cauchy-good(6+3) at 2 and 4 dwords per lane (P = 64: the packet must hold a lane's 16 bytes;
    two 4 KiB column tiles, the second ragged), and RS(12+9) at w = 32 on the mask-per-bit
    k_gfw_wordwise, which the automatic policy picks only past 4 rows"""
    import torch

    c = BY_ID.get(case_id) or Case("cauchy63p64", "bitsliced", L.CAUCHY_GOOD, 6, 3, 8, 64, 8 * 64 * 65,
                                  ([0], [1, 7], [2, 6, 7]), "auto")
    E.set_kernel_variant(0, bs)
    try:
        encode_and_decode(torch, c, "off8", True)
    finally:
        E.set_kernel_variant(0, 0)


# ---------------------------------------------------------------- stripe magic
MAGIC_CASES = [
    Case("rs63", "fused bytewise, IT = 2", L.REED_SOL_VAN, 6, 3, 8, 0, 16392, (), ""),
    Case("rs164", "fused bytewise, IT = 1", L.REED_SOL_VAN, 16, 4, 8, 0, 8200, (), ""),
    Case("cauchy63", "fused bit-sliced", L.CAUCHY_GOOD, 6, 3, 8, 24, 8256, (), ""),
    Case("rs1210", "two passes: m > 8", L.REED_SOL_VAN, 12, 10, 8, 0, 8200, (), ""),
    Case("liberation7", "two passes: bitmatrix", L.LIBERATION, 7, 2, 7, 40, 7 * 40 * 33, (), ""),
    Case("rs63w16", "two passes: w = 16", L.REED_SOL_VAN, 6, 3, 16, 0, 2 * 16384 + 8, (), ""),
]


def test_oracle_adler32_is_zlib():
    buf = np.random.default_rng(3).integers(0, 256, 70001, dtype=np.uint8)
    assert O.adler32(buf) == zlib.adler32(buf.tobytes())
    assert O.adler32(np.full(70001, 0xFF, np.uint8)) == zlib.adler32(b"\xff" * 70001)


def run_magic(torch, p, what, lay, chunks, outputs, call):
    """one magic call: outputs against the reference, the magics against zlib, exactly 4*N magic
    bytes and nothing else changed"""
    magic = np.stack([je_magic(chunks[s]) for s in range(lay.nstripes)])
    before, want = LY.images(lay, chunks, outputs, magic=magic)
    arena, refs, magic_ptr = LY.to_device(torch, lay, before)
    torch.cuda.synchronize()
    call(refs, magic_ptr)
    torch.cuda.synchronize()
    LY.assert_arena(lay, arena.cpu().numpy(), want, what)


@pytest.mark.parametrize("layout", ["packed", "off8", "mixed"])
@pytest.mark.parametrize("c", MAGIC_CASES, ids=[c.id for c in MAGIC_CASES])
def test_encode_magic_whole_arena(cuda, c, layout):
    import torch

    full = reference_of(c)
    parity = list(range(c.k, c.k + c.m))
    lay = LY.plan_layout(layout, c.k, c.m, NSTRIPES, c.size, parity, magic=True)
    with make_plan(c) as p:
        run_magic(torch, p, f"{c.id} encode + magic", lay, full, parity,
                  lambda refs, mp: p.encode_magic_dev_refs(refs, NSTRIPES, c.size, mp))


@pytest.mark.parametrize("layout", ["off8", "mixed"])
@pytest.mark.parametrize("n,size", [(9, 8), (9, 16), (9, 24), (9, 8200), (9, 65536), (72, 8200), (128, 8200)])
def test_stripe_magic_of_chunks_no_encode_produced(cuda, n, size, layout):
    """lsec_stripe_magic_dev over chunks as they are: stripe 0 every byte of all k+m chunks 0xFF (the
    modular sums' true maximum, which no encode produces: the parity of 0xFF data is not 0xFF),
    stripes 1 and 3 random, stripe 2 one set bit in the stripe's last byte.  72 shards: one launch of
    kMaxMagicShards; 128: two, the second with shard0 = 72."""
    import torch

    k, m, w = (n - 3, 3, 8) if n == 9 else (n - 8, 8, 8 if n == 72 else 16)
    nstr = 4
    chunks = np.random.default_rng(n * size).integers(0, 256, (nstr, n, size), dtype=np.uint8)
    chunks[0] = 0xFF
    chunks[2] = 0
    chunks[2, n - 1, size - 1] = 0x01
    lay = LY.plan_layout(layout, k, m, nstr, size, (), magic=True)
    with L.Plan.new(L.REED_SOL_VAN, size, k, m, w, 0, 8) as p:
        run_magic(torch, p, f"stripe magic of {n} x {size}", lay, chunks, (),
                  lambda refs, mp: p.stripe_magic_dev_refs(refs, nstr, size, mp))


@pytest.mark.parametrize("layout", ["packed", "off8", "mixed"])
@pytest.mark.parametrize("size", [8, 16392, 65536])
def test_all_ff_stripe_through_the_fused_kernel(cuda, size, layout):
    """RAID4(1+1): the parity equals the data, so with 0xFF data every byte of the stripe is 0xFF --
    inputs and outputs -- and the fused kernel's 32-bit MagicLane chains carry their largest
    per-byte terms (the plan service accepts k = m = 1)."""
    import torch

    c = Case("raid4_11", "", L.RAID4, 1, 1, 8, 0, size, (), "")
    full = reference_chunks(c.method, 1, 1, 8, 0, size, 3, fill=0xFF)
    assert (full == 0xFF).all()
    lay = LY.plan_layout(layout, 1, 1, 3, size, [1], magic=True)
    with make_plan(c) as p:
        assert p.kernel == 1
        run_magic(torch, p, f"all-0xFF RAID4(1+1) C={size}", lay, full, [1],
                  lambda refs, mp: p.encode_magic_dev_refs(refs, 3, size, mp))


# ---------------------------------------------------------------- the contract of lsec_shard_t
def test_bases_and_strides_must_be_multiples_of_8(cuda):
    """every lsec_*_dev entry point refuses a base that is not a multiple of 8, and such a stride
    once nstripes > 1, with a message naming the rule; nothing is enqueued: the arena is unchanged.
    nstripes == 0 with null refs stays valid (the calls that prepare ahead)."""
    import torch

    c = BY_ID["rs63"]
    n, size, km = NSTRIPES, c.size, c.k + c.m
    full = reference_of(c)
    lay = LY.plan_layout("off8", c.k, c.m, n, size, [0], magic=True)
    before, _ = LY.images(lay, full, [0])
    arena, refs, magic_ptr = LY.to_device(torch, lay, before)
    ids = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with make_plan(c) as p:
        calls = {
            "lsec_encode_dev": lambda r, ns: p.encode_dev_refs(r, ns, size),
            "lsec_decode_dev": lambda r, ns: p.decode_dev_refs(r, ns, size, [0]),
            "lsec_decode_dev_patterns": lambda r, ns: p.decode_dev_patterns_refs(r, ns, size, [[0]], ids.data_ptr()),
            "lsec_decode_dev_rotated": lambda r, ns: p.decode_dev_rotated_refs(r, ns, size, [0], 1, 0),
            "lsec_encode_magic_dev": lambda r, ns: p.encode_magic_dev_refs(r, ns, size, magic_ptr),
            "lsec_stripe_magic_dev": lambda r, ns: p.stripe_magic_dev_refs(r, ns, size, magic_ptr),
        }
        for name, call in calls.items():
            for shard in (0, 4, km - 1):
                bad = list(refs)
                bad[shard] = (refs[shard][0] + 4, refs[shard][1])
                for ns in (1, n):
                    with pytest.raises(L.ErasureError, match=rf"shard {shard}: base .* multiple of 8 bytes"):
                        call(bad, ns)
                bad[shard] = (refs[shard][0], refs[shard][1] + 4)
                with pytest.raises(L.ErasureError, match=rf"shard {shard}: stride .* multiple of 8 bytes"):
                    call(bad, n)
            call([(0, 0)] * km, 0)  # prepare ahead: null refs, no stripes
        torch.cuda.synchronize()
        assert np.array_equal(arena.cpu().numpy(), before), "a refused call wrote to the arena"
        # one stripe never uses the stride: any value is accepted, and the decode is right
        lay1 = LY.plan_layout("off8", c.k, c.m, 1, size, [0])
        before1, want1 = LY.images(lay1, full[:1], [0])
        arena1, refs1, _ = LY.to_device(torch, lay1, before1)
        p.decode_dev_refs([(b, s + 4) for b, s in refs1], 1, size, [0])
        torch.cuda.synchronize()
        LY.assert_arena(lay1, arena1.cpu().numpy(), want1, "one stripe, odd strides")
