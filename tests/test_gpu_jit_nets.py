"""GPU: the run-time compiled networks (ec_netgen.cpp) on matrices no stock plan produces, against
the oracle (tests/netref.py).

The other GPU tests run a network only for the Vandermonde / Cauchy matrices of stock plans and
their inverses: no zero coefficient, no zero row, no unused input.  Here every generator form --
the w = 8 XOR network, the one-wave and the wave-pair-split w = 16 / 32 networks, the packet
networks over row masks and over coefficients -- runs alone (lsec_test_jit_run: bound, compiled,
fetched and launched by the production route) on the matrix classes of netref: inputs that no row
reads, so that `used` has holes and an odd count; rows and slices that are never written and must
be stored as zeros; rows whose top coefficient bit is low; an input of which one packet is read.

Each test is one compile and a few tiny launches over a whole arena (tests/layouts.py): outputs
bit-exact, every input, gap and guard band untouched.  Sizes come from lsec_test_jit_tile:
  XOR networks      8 bytes, and one tile plus 24 bytes (a ragged second tile);
  w = 16 / 32       two tiles plus 40 bytes: the network covers whole tiles only, so the last 40
                    bytes of every output keep the arena's garbage; below one tile nothing is written;
  packet networks   one super-packet, and the fewest super-packets whose column bytes exceed one
                    tile and are no multiple of it.
The LSEC_JIT_VARIANT forms of tests/test_jit_shapes.py run the same way, each in a child process.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import layouts as LY
import netref as NR
from lstore_amd import erasure as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# form -> (shape, R, K, w, packet), all inside the wants_* gates; K small where the source is long
FORMS = {
    "xor": [(0, 6, 20, 8, 0), (0, 8, 12, 8, 0), (0, 8, 32, 8, 0), (0, 3, 32, 8, 0)],
    "wave": [(1, 3, 6, 32, 0), (1, 4, 6, 16, 0)],
    "split": [(1, 4, 6, 32, 0), (1, 6, 5, 32, 0), (1, 5, 6, 16, 0), (1, 8, 5, 16, 0)],
    "pktmask": [(2, 2, 6, 7, 32), (2, 2, 16, 16, 32), (2, 2, 8, 8, 40)],
    "pktcoef": [(3, 4, 5, 32, 64), (3, 4, 6, 16, 32), (3, 6, 8, 8, 32)],
}
EVERY_CLASS = [cases[0] for cases in FORMS.values()] + [(1, 5, 6, 16, 0)]


def case_id(c):
    return "s%d_%dx%d_w%d" % c[:4] + ("_p%d" % c[4] if c[0] >= 2 else "")


def params():
    """every shape case on dense and holes_odd; holes_even, edges and single on the first case of
    each form and on (5, 6, 16); matrix shapes on packed and off8, packet shapes on packed and
    aligned_gap"""
    out = []
    for cases in FORMS.values():
        for c in cases:
            for cls in NR.CLASSES if c in EVERY_CLASS else ("dense", "holes_odd"):
                for layout in ("packed", "off8") if c[0] < 2 else ("packed", "aligned_gap"):
                    out.append(pytest.param(c, cls, layout, id=f"{case_id(c)}-{cls}-{layout}"))
    return out


def hooks():
    lib = E.lib()
    lib.lsec_test_jit_run.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(E.ShardRef), C.POINTER(E.ShardRef), C.c_int,
                                                      C.c_longlong, C.c_void_p]
    lib.lsec_test_jit_run.restype = C.c_int
    lib.lsec_test_jit_tile.argtypes = [C.c_int] * 5
    lib.lsec_test_jit_tile.restype = C.c_int
    return lib


def tile_of(c):
    t = hooks().lsec_test_jit_tile(*c)
    assert t > 0, E.last_error()
    return t


def sizes_of(c):
    """[(chunk size, bytes of it the network covers)] of a case"""
    shape, R, K, w, packet = c
    tile = tile_of(c)
    if shape == 0:
        return [(8, 8), (tile + 24, tile + 24)]
    if shape == 1:
        return [(2 * tile + 40, 2 * tile), (tile - 8, 0)]
    n = tile // packet + 1
    while n * packet % tile == 0:
        n += 1
    return [(w * packet, w * packet), (w * packet * n, w * packet * n)]


_want = {}


def reference(c, cls, size, covered):
    """(matrix, chunks uint8 [3, K+R, size]): computed once per (case, class, size), never modified.
    The outputs hold the reference over the first `covered` bytes and zeros after them."""
    key = (c, cls, size)
    if key not in _want:
        shape, R, K, w, packet = c
        M = NR.matrix(cls, shape, R, K, w)
        full = np.zeros((NR.NSTRIPES, K + R, size), np.uint8)
        full[:, :K] = NR.stripes(shape, R, K, w, size)
        if covered:
            full[:, K:, :covered] = NR.expected(shape, R, K, w, packet, M, full[:, :K, :covered])
        full.setflags(write=False)
        _want[key] = (M, full)
    return _want[key]


def shard_array(refs):
    arr = (E.ShardRef * len(refs))()
    for i, (b, st) in enumerate(refs):
        arr[i].base, arr[i].stride = b, st
    return arr


def run_net(torch, c, cls, layout, size, covered, refuse=False):
    """one launch of the case's network over a fresh arena, the whole arena compared"""
    shape, R, K, w, packet = c
    M, full = reference(c, cls, size, covered)
    outputs = list(range(K, K + R))
    lay = LY.plan_layout(layout, K, R, NR.NSTRIPES, size, outputs=outputs)
    before, want = LY.images(lay, full, outputs)
    for i in outputs:  # what the network does not cover keeps the arena's garbage
        for s in range(NR.NSTRIPES):
            want[lay.start(i, s) + covered:lay.start(i, s) + size] = LY.GARBAGE
    if refuse:
        want = before
    arena, refs, _ = LY.to_device(torch, lay, before)
    torch.cuda.synchronize()
    rc = hooks().lsec_test_jit_run(shape, R, K, w, packet, M.ctypes.data, shard_array(refs[:K]), shard_array(refs[K:]),
                                   NR.NSTRIPES, size, None)
    what = f"{case_id(c)} {cls} C={size}"
    if rc != 0 and "launch failed" in E.last_error():
        # the launch or its synchronisation failed: the device may be in error, run nothing after it
        pytest.exit(f"{what} ({layout}): {E.last_error()}", returncode=3)
    if refuse:
        assert rc == -1 and "pkt_aligned" in E.last_error(), (what, rc, E.last_error())
    else:
        assert rc == 0, (what, E.last_error())
    torch.cuda.synchronize()
    LY.assert_arena(lay, arena.cpu().numpy(), want, what)


def run_case(torch, c, cls, layout):
    for size, covered in sizes_of(c):
        run_net(torch, c, cls, layout, size, covered)


@pytest.mark.parametrize("c,cls,layout", params())
def test_network_of_any_matrix(cuda, c, cls, layout):
    import torch

    run_case(torch, c, cls, layout)
    # 16-byte lanes: shards at 8 mod 16 are refused, and nothing is written
    if c[0] >= 2 and tile_of(c) == 256 * 16 and layout == "packed":
        size, covered = sizes_of(c)[0]
        run_net(torch, c, cls, "off8", size, covered, refuse=True)


# ------------------------------------------------------------------ the LSEC_JIT_VARIANT forms
def knob_sets():
    from test_jit_shapes import test_knob_shapes_compile

    mark = next(m for m in test_knob_shapes_compile.pytestmark if m.name == "parametrize")
    return list(mark.args[1])


def knob_cases(pick):
    """the first case of every form that `pick` selects"""
    return [next(c for c in cases if pick(c)) for cases in FORMS.values() if any(pick(c) for c in cases)]


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_jit_nets as T
assert torch.cuda.is_available()
for c in {cases!r}:
    for layout in (("packed", "off8") if c[0] < 2 else ("packed", "aligned_gap")):
        T.run_case(torch, c, "holes_odd", layout)
        print("ok", c, layout, flush=True)
"""


def test_knob_forms_run(cuda):
    """every LSEC_JIT_VARIANT set of test_jit_shapes.test_knob_shapes_compile, each in a fresh child
    process (the variant is read once per process): holes_odd on the first case of every form the
    set's pick selects, compared as above.  Stops at the first child that does not exit 0."""
    sets = knob_sets()
    assert len(sets) >= 6
    for variant, pick in sets:
        cases = knob_cases(pick)
        assert cases, hex(variant)
        script = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), cases=cases)
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, LSEC_JIT_VARIANT=str(variant)))
        print(f"LSEC_JIT_VARIANT={variant:#x} {cases}: exit {r.returncode} after {time.monotonic() - t0:.1f} s")
        assert r.returncode == 0, (hex(variant), r.returncode, r.stdout[-1500:], r.stderr[-3000:])
