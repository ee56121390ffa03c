"""GPU: every kernel form of the parity updates and of the rotated encode against the reference:
lsec_update_dev, lsec_update_dev_rotated, lsec_encode_dev_rotated, lsec_update_dev_masked(_rotated) and
lsec_update_magic_dev_masked(_rotated).

Each of these calls is a family of separately compiled kernels (tests/scrub_forms.py: WRITE_CALLS); the tables of
codes in test_gpu_update.py, test_gpu_rotated_write.py, test_gpu_update_masked.py and test_gpu_update_magic.py run a
corner of them.  Here one representative plan per form, and the edge plans of scrub_forms.py, run through the rigs of
those files, so the bars are theirs: bit-exact, the expected parity from test_gpu_check.ref_encode (oracle/_ref when
it is built, else the restatement), the expected magics from zlib's adler32, nothing expected ever taken from the
engine, canary gaps and guard bands compared over the whole arena, and the fresh, decoy and mask buffers unchanged.
After every call the launch record (E.launch_record) equals the prediction, once per launch -- the rigs assert that
-- and the predicted form is the form the case was generated for: which kernel ran is asserted, not assumed.

Sizes are the smallest at which a form can still go wrong (scrub_forms.sizes): a single half lane, which only the
ragged path sees, and one full tile of that form plus a half-lane tail; bit-sliced one super-packet, and one tile of
column space plus a packet.  The "off8" layout, every shard at 8 mod 16; the stripe counts are the rigs' own.
"""
import pytest
import torch  # before the engine library, which the enumeration below loads while pytest collects:
#               the rest of the suite loads it behind torch, inside its tests

from lstore_amd import erasure as E

import scrub_forms as SF
import test_gpu_rotated_write as TRW
import test_gpu_update as TU
import test_gpu_update_magic as TUM
import test_gpu_update_masked as TM

pytestmark = pytest.mark.gpu

N_SHIFT, FIRST = 1, 3_000_000_007
LAYOUT = "off8"
HEAVY_K = 64


def code_of(c):
    return (c.method, c.k, c.m, c.packet)


def col_sets(k):
    """the changed sets of an update: column k-1 alone, and {0, k//2, k-1} (all k columns where k <= 3)"""
    out = [(k - 1,), tuple(sorted({0, k // 2, k - 1}))]
    return out[:1] if out[0] == out[1] else out


def cases(*calls):
    return [c for call in calls for c in SF.cases(call)]


def is_the_case(c, size, form):
    """the form the rig predicts (and compares the launch record with) is the one the case stands for, and the
    calling thread's last call launched it"""
    assert form == c.form, f"{SF.case_id(c)} C={size}: predicted {form}, the case stands for {c.form}"
    got = E.launch_record()
    assert got and set(got) == {c.form}, f"{SF.case_id(c)} C={size}: launched {got}"


# ---------------------------------------------------------------- lsec_update_dev
@pytest.mark.parametrize("c", cases("upd"), ids=SF.case_id)
def test_update(cuda, c):
    for size in SF.sizes(c):
        for cols in col_sets(c.k):
            bench = TU.Bench(torch, code_of(c), c.packet, size, LAYOUT, cols)
            try:
                for store in (False, True):
                    bench.run(store)  # (the whole arena, the fresh arena, the decoys, the launch record)
                    is_the_case(c, size, bench.form)
            finally:
                bench.close()


# ---------------------------------------------------------------- lsec_update_dev_rotated, lsec_encode_dev_rotated
def rotated_update_items():
    """(case, size, changed set): None for both of a case's sizes and sets.  The rotated rig holds k + m + 2 stripes,
    so that the rotation wraps, and the reference encodes each of them once per size and changed set: at k = 64 an
    item is one size and one set."""
    out = []
    for c in cases("updrot"):
        if c.k >= HEAVY_K:
            out += [(c, size, cols) for size in SF.sizes(c) for cols in col_sets(c.k)]
        else:
            out.append((c, None, None))
    return out


def rotated_update_id(item):
    c, size, cols = item
    return SF.case_id(c) + ("" if size is None else f"-C{size}-" + "_".join(str(j) for j in cols))


@pytest.mark.parametrize("item", rotated_update_items(), ids=rotated_update_id)
def test_update_rotated(cuda, item):
    c, only_size, only_cols = item
    code = code_of(c)
    for size in SF.sizes(c) if only_size is None else (only_size,):
        for cols in col_sets(c.k) if only_cols is None else (only_cols,):
            fresh, after = TRW.updated_consistent(code, c.packet, size, cols)
            bench = TRW.Bench(torch, code, c.packet, size, LAYOUT, cols, fresh)
            try:
                for store in (False, True):
                    bench.run_update(N_SHIFT, FIRST, store, after)
                    is_the_case(c, size, TRW.form_of("updrot", code, c.packet, size))
            finally:
                bench.close()


@pytest.mark.parametrize("c", cases("encrot"), ids=SF.case_id)
def test_encode_rotated(cuda, c):
    code = code_of(c)
    for size in SF.sizes(c):
        bench = TRW.Bench(torch, code, c.packet, size, LAYOUT)
        try:
            bench.run_encode(N_SHIFT, FIRST)
            is_the_case(c, size, TRW.form_of("encrot", code, c.packet, size))
        finally:
            bench.close()


# ---------------------------------------------------------------- the masked updates, with and without the magics
@pytest.mark.parametrize("c", cases("updmask", "updmaskrot"), ids=SF.case_id)
def test_update_masked(cuda, c):
    """the rig's seven mask words, unsplit and in launches of 3, 3 and 1 stripes"""
    code, rotated = code_of(c), c.call == "updmaskrot"
    rotation = (N_SHIFT, FIRST) if rotated else (0, 0)
    for size in SF.sizes(c):
        _, after = TM.after_write(code, c.packet, size)
        bench = TM.Bench(torch, code, c.packet, size, LAYOUT, rotated=rotated)
        try:
            for store in (False, True):
                for split in (0, TM.SPLIT):
                    bench.run(store, after, *rotation, split=split)
                    is_the_case(c, size, bench.form)
        finally:
            bench.close()


@pytest.mark.parametrize("c", cases("updmagic", "updmagicrot"), ids=SF.case_id)
def test_update_magic(cuda, c):
    """as above, and every stripe's magic moved from zlib's of the old stripe to zlib's of the new one"""
    code, rotated = code_of(c), c.call == "updmagicrot"
    rotation = (N_SHIFT, FIRST) if rotated else (0, 0)
    for size in SF.sizes(c):
        _, after = TM.after_write(code, c.packet, size)
        bench = TUM.Bench(torch, code, c.packet, size, LAYOUT, rotated=rotated)
        try:
            for store in (False, True):
                for split in (0, TUM.SPLIT):
                    bench.check(store, after, *rotation, split=split, odd=store)
                    is_the_case(c, size, bench.form)
        finally:
            bench.close()
