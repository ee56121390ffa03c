"""The layout helper of the device-resident tests (tests/layouts.py), checked without a GPU: every
layout keeps its promises, and the whole-arena comparison notices one wrong byte wherever it
lands -- in an output, in the gap right behind a chunk, in a survivor -- and names the place."""
import numpy as np
import pytest

import layouts as LY

SHAPES = [(6, 3, 5, 16392, (6, 7, 8)), (6, 3, 5, 8256, (1, 7)), (4, 1, 3, 4104, (0,)), (70, 4, 2, 520, (0, 65, 70))]


def chunks_of(k, m, nstr, size):
    return np.random.default_rng(k * size + m).integers(0, 256, (nstr, k + m, size), dtype=np.uint8)


@pytest.mark.parametrize("name", LY.LAYOUTS)
@pytest.mark.parametrize("k,m,nstr,size,outputs", SHAPES)
def test_layout_promises(name, k, m, nstr, size, outputs):
    lay = LY.plan_layout(name, k, m, nstr, size, outputs, magic=True)
    LY.check_layout(lay)
    b16 = [o % 16 for o in lay.offsets]
    if name == "packed":
        assert lay.strides == [k * size] * k + [m * size] * m
        assert [lay.offsets[i] - lay.offsets[0] for i in range(k)] == [i * size for i in range(k)]
        assert lay.offsets[0] % 16 == 0 and lay.offsets[k] % 16 == 0
        if size % 16 == 8 and k > 1:
            assert b16[1] == 8
    elif name == "off8":
        assert set(b16) == {8} and set(lay.strides) == {size + 40}
    elif name in ("mixed", "mixed_swapped"):
        out_at = 8 if name == "mixed" else 0
        assert all(b16[i] == (out_at if i in outputs else 8 - out_at) for i in range(k + m))
        assert len(set(lay.strides)) == min(4, k + m)
    else:
        assert all(o % 256 == 0 for o in lay.offsets) and all(s % 16 == 0 and s >= size + 4096 for s in lay.strides)
    # the images: outputs garbage before and reference after, everything else equal, gaps canary
    full = chunks_of(k, m, nstr, size)
    keep = outputs[:1]
    before, want = LY.images(lay, full, outputs, keep=keep, magic=np.arange(4 * nstr, dtype=np.uint8))
    owner = np.zeros(lay.total, bool)
    for i in range(k + m):
        for s in range(nstr):
            a = lay.start(i, s)
            owner[a:a + size] = True
            assert np.array_equal(want[a:a + size], np.full(size, LY.GARBAGE, np.uint8) if i in keep else full[s, i])
            assert np.array_equal(before[a:a + size], np.full(size, LY.GARBAGE, np.uint8) if i in outputs else full[s, i])
    assert (before[~owner] == LY.CANARY).all()
    owner[lay.magic_off:lay.magic_off + 4 * nstr] = True
    assert (want[~owner] == LY.CANARY).all() and (want[:LY.GUARD] == LY.CANARY).all() and (want[-LY.GUARD:] == LY.CANARY).all()
    assert np.array_equal(want[lay.magic_off:lay.magic_off + 4 * nstr], np.arange(4 * nstr, dtype=np.uint8))


@pytest.mark.parametrize("name", LY.LAYOUTS)
@pytest.mark.parametrize("k,m,nstr,size,outputs", SHAPES[:3])
def test_comparison_names_the_planted_byte(name, k, m, nstr, size, outputs):
    lay = LY.plan_layout(name, k, m, nstr, size, outputs, magic=True)
    full = chunks_of(k, m, nstr, size)
    _, want = LY.images(lay, full, outputs, magic=np.zeros(4 * nstr, np.uint8))
    LY.assert_arena(lay, want.copy(), want, "clean")
    s, out = nstr - 1, outputs[-1]
    survivor = next(i for i in range(k + m) if i not in outputs)

    def planted(pos):
        got = want.copy()
        got[pos] ^= 0x10
        return got

    # one wrong byte in an output
    with pytest.raises(AssertionError, match=rf"1 bytes differ: stripe {s} shard {out} bytes \[{size - 3}, {size - 3}\]$"):
        LY.assert_arena(lay, planted(lay.start(out, s) + size - 3), want, "output")
    # one byte written directly behind a chunk: a gap wherever the layout leaves one there, else
    # (packed: the next chunk starts right there) the neighbour's first byte
    pos = lay.start(out, s) + size
    ps, pi, pb, gap = lay.place(pos)
    if gap:
        assert (ps, pi, pb) == (s, out, size)
        expect = rf"gap after stripe {s} shard {out}: bytes \[{size}, {size}\] from its start"
    else:
        assert name == "packed" and pb == 0 and (ps, pi) != (s, out)
        expect = rf"stripe {ps} shard {pi} bytes \[0, 0\]$"
    with pytest.raises(AssertionError, match=expect):
        LY.assert_arena(lay, planted(pos), want, "overrun")
    # the last chunk of the arena is followed by canary in every layout
    last = max((lay.start(i, nstr - 1), i) for i in range(k + m))
    with pytest.raises(AssertionError, match=rf"gap after stripe {nstr - 1} shard {last[1]}: bytes \[{size + 8}, {size + 8}\]"):
        LY.assert_arena(lay, planted(last[0] + size + 8), want, "overrun of the last chunk")
    # one byte changed in a survivor
    with pytest.raises(AssertionError, match=rf"1 bytes differ: stripe 0 shard {survivor} bytes \[7, 7\]$"):
        LY.assert_arena(lay, planted(lay.start(survivor, 0) + 7), want, "survivor")
    # the guard band in front, and a fifth magic byte
    with pytest.raises(AssertionError, match=r"gap before the first chunk: arena bytes \[4000, 4000\]"):
        LY.assert_arena(lay, planted(4000), want, "front guard")
    with pytest.raises(AssertionError, match="gap after"):
        LY.assert_arena(lay, planted(lay.magic_off + 4 * nstr), want, "past the magics")
    with pytest.raises(AssertionError, match=r"magic of stripe 1 bytes \[2, 2\]"):
        LY.assert_arena(lay, planted(lay.magic_off + 6), want, "magic")
