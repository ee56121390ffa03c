"""GPU: a plan's per-device images (DevImage) -- every device-resident call of one plan of each
kernel kind, bit-exact against the yardstick, with the number of device allocations the plan owns
(lsec_test_plan_images) asserted after each step: a repeated call adds none, a new erasure pattern
or the locate's ratio image one, a new pattern table two (records and cells), and the check and the
update none (they read the encode image).  Then the plan is destroyed and made again, and the first
encode and decode must equal the yardstick again: the new plan's images may land on the freed
addresses, where a network still bound to the old image would be launched over the new one.
"""
import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

pytestmark = pytest.mark.gpu

NSTRIPES = 3
# name: (method, k, m, w, packet, chunk).  Chunks: 4096 = one bytewise tile; the packet codes' a few super-packets
KINDS = {
    "rs8": (L.REED_SOL_VAN, 6, 3, 8, 0, 4096),          # bytewise GF(2^8): cells
    "cauchy8": (L.CAUCHY_GOOD, 6, 3, 8, 64, 4096),      # bit-sliced GF(2^8): cells
    "rs16": (L.REED_SOL_VAN, 6, 3, 16, 0, 4096),        # wordwise GF(2^16): word products
    "cauchy16": (L.CAUCHY_GOOD, 4, 2, 16, 32, 2048),    # bit-sliced GF(2^16): word products
    "liberation": (L.LIBERATION, 5, 2, 5, 64, 5 * 64 * 4),  # bitmatrix: row masks
    "raid4": (L.RAID4, 6, 1, 8, 0, 4096),               # XOR: cells
}
GF8 = ("rs8", "cauchy8")  # the kinds the check, locate, patterned decode and update serve

_ref = {}


def ref_encode(kind, data):
    """the yardstick's parity [m, C] of data [k, C]"""
    method, k, m, w, packet, _ = KINDS[kind]
    if not O.ref_available():
        if method in (L.LIBERATION, L.RAID4):
            pytest.skip("oracle/_ref not built")
        return O.encode(method, np.ascontiguousarray(data), m, packet, w)
    if kind not in _ref:
        _ref[kind] = O.RefPlan(method, k, m, w, packet)
    return _ref[kind].encode(np.ascontiguousarray(data))


def ref_stripes(kind, seed):
    """uint8 [N, k+m, C]: random data and the yardstick's parity; computed once, never modified"""
    key = (kind, seed)
    if key not in _ref:
        _, k, m, _, _, chunk = KINDS[kind]
        full = np.empty((NSTRIPES, k + m, chunk), np.uint8)
        full[:, :k] = np.random.default_rng(seed).integers(0, 256, (NSTRIPES, k, chunk), dtype=np.uint8)
        for s in range(NSTRIPES):
            full[s, k:] = ref_encode(kind, full[s, :k])
        full.setflags(write=False)
        _ref[key] = full
    return _ref[key]


def make_plan(kind):
    method, k, m, w, packet, chunk = KINDS[kind]
    p = L.Plan.new(method, chunk, k, m, w, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


def patterns_of(kind):
    """two erasure patterns: data chunk 0 alone (rebuilt from P0 by XOR for every matrix code here: a u32 kind's
    plan then takes its cell image), and one that needs the kind's own coefficients"""
    _, k, m, _, _, _ = KINDS[kind]
    return [0], ([1, k] if m > 1 else [2])


def encode_and_decode(torch, p, kind, dev, want, counted):
    """the first two steps and the decodes of the sequence on `dev`; counted(step, added) asserts the image count"""
    _, k, m, _, _, _ = KINDS[kind]
    full = torch.from_numpy(want.copy()).to(dev)
    data, par = full[:, :k], full[:, k:]
    for again in (False, True):
        par.fill_(0xA5)
        p.encode_dev(data, par)
        torch.cuda.synchronize(dev)
        assert np.array_equal(full.cpu().numpy(), want), f"{kind}: encode{' again' if again else ''}"
        counted("encode again" if again else "encode", 0 if again else 1)
    first, second = patterns_of(kind)
    for er, added, what in ((first, 1, "decode"), (first, 0, "decode again"), (second, 1, "decode, second pattern")):
        full[:, er] = 0x5C
        p.decode_dev(data, par, er)
        torch.cuda.synchronize(dev)
        assert np.array_equal(full.cpu().numpy(), want), f"{kind}: {what} {er}"
        counted(what, added)
    return full


def sequence(torch, p, kind, dev, base=0):
    """every step on `dev`, whose images come on top of `base`; returns the images added"""
    _, k, m, _, _, chunk = KINDS[kind]
    count = [base]

    def counted(step, added):
        count[0] += added
        assert E.plan_images(p) == count[0], f"{kind}: after {step}"

    want = ref_stripes(kind, 1)
    full = encode_and_decode(torch, p, kind, dev, want, counted)
    if kind not in GF8:
        return count[0] - base
    data, par = full[:, :k], full[:, k:]
    syndrome = torch.full((NSTRIPES,), -1, dtype=torch.int32, device=dev)
    bad = torch.full((1,), -1, dtype=torch.int32, device=dev)
    p.check_dev(data, par, syndrome, bad)
    torch.cuda.synchronize(dev)
    assert syndrome.cpu().tolist() == [0] * NSTRIPES and bad.item() == 0, f"{kind}: check"
    counted("check", 0)  # the encode image
    # locate with repair: the ratio image and the table of the k+m single erasures
    hyp = torch.zeros((NSTRIPES,), dtype=torch.int64, device=dev)
    located = torch.zeros((NSTRIPES,), dtype=torch.uint8, device=dev)
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    full[1, 2, 17] ^= 0x40
    for again in (False, True):
        p.locate_dev(data, par, syndrome, hyp, located, counts, repair=True)
        torch.cuda.synchronize(dev)
        assert located.cpu().tolist() == ([E.LOCATE_CLEAN] * NSTRIPES if again else [E.LOCATE_CLEAN, 2, E.LOCATE_CLEAN]), kind
        assert np.array_equal(full.cpu().numpy(), want), f"{kind}: locate and repair"
        counted("locate again" if again else "locate with repair", 0 if again else 3)
    # patterned decode: a table of its own
    pats = [list(x) for x in patterns_of(kind)]
    which = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    for again in (False, True):
        for s, w in enumerate((0, 1, 0)):
            full[s, pats[w]] = 0x5C
        p.decode_dev_patterns(data, par, pats, which)
        torch.cuda.synchronize(dev)
        assert np.array_equal(full.cpu().numpy(), want), f"{kind}: patterned decode"
        counted("patterned decode again" if again else "patterned decode", 0 if again else 2)
    # update: chunks 1 and 4 change to those of another set of stripes, whose parity the yardstick gives
    cols = [1, 4]
    other = ref_stripes(kind, 2)
    after = want.copy()
    after[:, cols] = other[:, cols]
    for s in range(NSTRIPES):
        after[s, k:] = ref_encode(kind, after[s, :k])
    fresh = torch.from_numpy(np.ascontiguousarray(other[:, cols])).to(dev)
    p.update_dev(data, par, cols, fresh, store=True)
    torch.cuda.synchronize(dev)
    assert np.array_equal(full.cpu().numpy(), after), f"{kind}: update"
    counted("update", 0)  # the encode image
    return count[0] - base


@pytest.mark.parametrize("kind", list(KINDS))
def test_images_per_step_and_after_a_new_plan(cuda, kind):
    import torch

    p = make_plan(kind)
    try:
        assert E.plan_images(p) == 0, "forming the matrices touches no device"
        # encode 1, two patterns 2; the GF(2^8) kinds: ratio 1, two tables 4
        assert sequence(torch, p, kind, cuda) == (8 if kind in GF8 else 3)
    finally:
        p.close()
    # the same plan again, after the first one's images were freed
    p = make_plan(kind)
    try:
        count = [0]

        def counted(step, added):
            count[0] += added
            assert E.plan_images(p) == count[0], f"{kind}: new plan, after {step}"

        encode_and_decode(torch, p, kind, cuda, ref_stripes(kind, 1), counted)
    finally:
        p.close()


def test_xor_only_pattern_of_a_mask_kind_takes_cells(cuda):
    """Cauchy at w = 16 is a u32-image kind; data chunk 0 rebuilt from P0 only XORs survivors, so that entry's one
    image is the cell image and the bytewise kernel applies it (apply_path: a generic kernel, no network)"""
    import torch

    kind = "cauchy16"
    _, k, m, _, _, _ = KINDS[kind]
    want = ref_stripes(kind, 1)
    with make_plan(kind) as p:
        full = torch.from_numpy(want.copy()).to(cuda)
        full[:, 0] = 0
        p.decode_dev(full[:, :k], full[:, k:], [0])
        torch.cuda.synchronize(cuda)
        assert E.apply_path() == 4
        assert np.array_equal(full.cpu().numpy(), want)
        assert E.plan_images(p) == 1  # no encode image yet: the entry's alone


def test_second_device_doubles_the_images(cuda):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    p = make_plan("rs8")
    try:
        n0 = sequence(torch, p, "rs8", cuda)
        with torch.cuda.device(1):
            n1 = sequence(torch, p, "rs8", torch.device("cuda:1"), base=n0)
        assert n0 == n1 == 8 and E.plan_images(p) == 2 * n0
    finally:
        p.close()
