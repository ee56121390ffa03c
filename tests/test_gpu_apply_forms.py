"""GPU: every kernel form behind lsec_encode_dev, lsec_decode_dev and lsec_encode_magic_dev, one plan per form.

tests/apply_forms.py enumerates the forms through the engine's prediction hooks and yields one plan per form and the
edge plans; tests/test_apply_forms.py shows on the CPU that the enumeration is closed.  Here each case runs through
the whole-arena rig of tests/layouts.py and tests/test_gpu_layouts.py (run_call, run_magic): the arena byte for byte,
guard bands included, against the reference -- oracle/_ref where built, else the oracle restatement, zlib.adler32 for
the magics -- and after every call E.apply_record() equals the prediction, so a case that ran another kernel than
the one it is there for fails.

The compiled networks are held off (E.hold_networks) and the variants set in try / finally: what runs is the table
dispatch, deterministically, as on a plan's first calls.

Shapes: the smallest at which these kernels can go wrong (AF.sizes) -- bytewise 8 bytes (the ragged path alone) and
one tile plus 8; the packet kernels one super-packet, and the whole packets that cover one tile of column space plus
one packet -- on 3 stripes, so that the one-row shape's four-tile grabs cross a stripe boundary, on the layouts
packed and off8.  Data: seeded random, stripe 1 all 0xFF (the modular sums' maximum), stripe 2 zero but for the top
bit of the last data byte (test_gpu_layouts.reference_chunks).
"""
import collections

import pytest
import torch  # before the engine library, which the enumeration below loads while pytest collects:
#               the rest of the suite loads it behind torch, inside its tests

import apply_forms as AF
import layouts as LY
import test_gpu_layouts as TL
from lstore_amd import erasure as E

pytestmark = pytest.mark.gpu

NSTRIPES = 3
LAYOUTS = ("packed", "off8")
Id = collections.namedtuple("Id", "id")


def params(tier):
    return [pytest.param(c, id=AF.case_id(c)) for c in AF.cases(tier)]


def run_case(torch, c):
    name, n = Id(AF.case_id(c)), NSTRIPES
    parity = list(range(c.k, c.k + c.m))
    E.hold_networks(True)
    E.set_kernel_variant(*c.variants)
    try:
        for size in AF.sizes(c):
            full = TL.reference_chunks(c.method, c.k, c.m, c.w, c.packet, size, n)
            with AF.make_plan(c.method, c.k, c.m, c.w, c.packet, size) as p:
                want = E.predict_apply_plan(p, list(c.erasures) if c.op == "dec" else None, size, magic=c.op == "magic")
                assert tuple(want) == c.forms, f"{name.id} C={size}: predicted {want}"

                def recorded(what):
                    got = E.apply_record()
                    assert got == want, f"{name.id} C={size} {what}: launched {got}, predicted {want}"

                for layout in LAYOUTS:
                    if c.op == "enc":
                        lay = LY.plan_layout(layout, c.k, c.m, n, size, parity)
                        TL.run_call(torch, p, name, lay, full, parity,
                                    lambda refs: (p.encode_dev_refs(refs, n, size), recorded("encode")), f"encode C={size}",
                                    path=TL.GENERIC)
                    elif c.op == "dec":
                        er = list(c.erasures)
                        lay = LY.plan_layout(layout, c.k, c.m, n, size, er)
                        TL.run_call(torch, p, name, lay, full, er,
                                    lambda refs: (p.decode_dev_refs(refs, n, size, er), recorded(f"decode {er}")),
                                    f"decode {er} C={size}", path=TL.GENERIC)
                    else:
                        lay = LY.plan_layout(layout, c.k, c.m, n, size, parity, magic=True)
                        TL.run_magic(torch, p, f"{name.id} encode + magic C={size} ({layout})", lay, full, parity,
                                     lambda refs, mp: (p.encode_magic_dev_refs(refs, n, size, mp), recorded("encode + magic")))
    finally:
        E.set_kernel_variant(0, 0)
        E.hold_networks(False)


@pytest.mark.parametrize("c", params("auto"))
def test_automatic_policy_forms(cuda, c):
    """kinds 1 and 2 under the automatic policy with no network ready: every plain, accumulate and fused-magic
    kernel, both loops of the two-loop kernels, the edge plans and the decodes of fewer chunks than m"""
    run_case(torch, c)


@pytest.mark.parametrize("c", params("variant"))
def test_variant_forms(cuda, c):
    """the kernels only lsec_set_kernel_variant reaches: the five bytewise shapes x R x KC with both loops, the
    bit-sliced kernels at 2 and 4 dwords per lane for every R"""
    run_case(torch, c)


@pytest.mark.parametrize("c", params("wide"))
def test_wide_kind_forms(cuda, c):
    """kinds 3-5: k_bitmatrix per word size and k_bitmatrix_any, k_gfw_transposed, the mask-per-bit k_gfw_wordwise and
    k_gfw_bitsliced, each R they take, plain and accumulating"""
    run_case(torch, c)
