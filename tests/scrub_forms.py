"""Which plans run which kernel of the check / locate / patterned-decode families (a helper, not a test).

Each of lsec_check_dev, lsec_locate_dev, their _rotated twins and lsec_decode_dev_patterns is a family
of separately compiled kernels: per parity-row count R, and bytewise per input count (fixed-K forms,
K at run time at 2 x 16 B and at 16 B per lane, the 8 B shape of R == 1), bit-sliced per dwords per
lane.  ``E.predict_form`` asks the engine -- the functions its dispatch calls, no GPU -- which form
a plan takes.  ``cases(call)`` enumerates K = 1..64 x R x packet through it and yields

* one representative plan per distinct form, at the smallest K that produces the form, and
* the edge plans: no new form, but the boundaries of the input loop, of the 64-bit hypothesis mask
  and of the documented limits.

Nothing here is a count or a list of forms: both come from the engine at import time of the caller.
"""
import collections

import lstore_amd as L
from lstore_amd import erasure as E

CALLS = ("chk", "loc", "chkrot", "locrot", "pat")
KS = range(1, 65)
SLICED_PACKETS = (8, 24, 64)  # 8 and 24 hold no lane of 4 dwords (DW falls to 2 where 4 is wanted), 64 does

# call, kind ("rep" / "edge"), the plan (method, k, m, packet), rows (m; pat: the table's largest erasure
# count), the predicted Form and a word on why the case is there
Case = collections.namedtuple("Case", "call kind method k m packet rows form why")


def rows_of(call):
    return range(2, 9) if call in ("loc", "locrot") else range(1, 9)


def plan_kernel(method):
    return 2 if method in (L.CAUCHY_GOOD, L.CAUCHY_ORIG) else 1


def small_size(packet):
    """a chunk size far below the 4 MiB at which the bit-sliced policy widens its lanes for K >= 10"""
    return 8 * packet if packet else 8


def predict(call, method, k, rows, packet, size=None):
    return E.predict_form(call, plan_kernel(method), k, rows, packet, small_size(packet) if size is None else size)


def _plan_for(call, sliced, k, rows):
    """the plan of a representative: RS, RAID4 where one row is wanted (bytewise), Cauchy-good (bit-sliced);
    a patterned table of `rows` erasures needs m >= rows, and two rows so that there is parity to lose"""
    m = max(rows, 2) if call == "pat" else rows
    if sliced:
        return L.CAUCHY_GOOD, k, m
    return (L.RAID4 if m == 1 else L.REED_SOL_VAN), k, m


def representatives(call):
    """one Case per distinct predicted form of `call`, at the smallest K (then the first packet) giving it"""
    seen, out = set(), []
    for sliced in (False, True):
        for rows in rows_of(call):
            for k in KS:
                for packet in (SLICED_PACKETS if sliced else (0,)):
                    method, _, m = _plan_for(call, sliced, k, rows)
                    form = predict(call, method, k, rows, packet)
                    if form not in seen:
                        seen.add(form)
                        out.append(Case(call, "rep", method, k, m, packet, rows, form, "smallest K of its form"))
    return out


# (method, k, m, packet, why); RS(64+64) is for the patterned decode alone
EDGES = (
    (L.REED_SOL_VAN, 1, 2, 0, "K < 4: one input"),
    (L.REED_SOL_VAN, 2, 7, 0, "K < 4: two inputs, seven rows"),
    (L.REED_SOL_VAN, 3, 6, 0, "K < 4: three inputs, six rows"),
    (L.REED_SOL_VAN, 17, 2, 0, "run-time K at 16 B per lane, the four-at-a-time loop ends in one input"),
    (L.REED_SOL_VAN, 18, 3, 0, "... in two"),
    (L.REED_SOL_VAN, 19, 5, 0, "... in three"),
    (L.REED_SOL_VAN, 33, 5, 0, "hyp bit 32"),
    (L.REED_SOL_VAN, 64, 8, 0, "k = 64: hyp bit 63, the finalize's K >= 64 branch"),
    (L.CAUCHY_GOOD, 64, 8, 8, "k = 64, bit-sliced"),
    (L.RAID4, 5, 1, 0, "R == 1 with K at run time"),
    (L.CAUCHY_GOOD, 3, 1, 8, "bit-sliced R == 1"),
    (L.CAUCHY_GOOD, 16, 4, 24, "a packet of 24: two dwords per lane where four are wanted"),
)
PAT_ONLY_EDGES = ((L.REED_SOL_VAN, 64, 64, 0, "k + m = 128: the shard-reference limit"),)


def edges(call):
    out = []
    for method, k, m, packet, why in EDGES + (PAT_ONLY_EDGES if call == "pat" else ()):
        if m not in rows_of(call) and call != "pat":
            continue  # one row cannot locate
        rows = min(m, 8)
        out.append(Case(call, "edge", method, k, m, packet, rows, predict(call, method, k, rows, packet), why))
    return out


def cases(call):
    """the representatives, then the edge plans that are not representatives already"""
    reps = representatives(call)
    have = {(c.method, c.k, c.m, c.packet) for c in reps}
    return reps + [c for c in edges(call) if (c.method, c.k, c.m, c.packet) not in have]


def case_id(c):
    f = c.form
    shape = f"dw{f.DW}" if f.sliced else f"kc{f.KC}_it{f.IT}_vw{f.VW}{'' if f.BF else '_br'}"
    return f"{c.call}-{c.kind}-{L.JE_METHOD_NAMES[c.method]}_{c.k}+{c.m}" + (f"_p{c.packet}" if c.packet else "") + f"-r{f.R}_{shape}"


def tile_bytes(form):
    """bytes of chunk (bytewise) or of packet-column space (bit-sliced) that one workgroup's tile covers"""
    return 1024 * form.DW if form.sliced else 256 * 4 * form.VW * form.IT


def sizes(c):
    """the two chunk sizes of a case.  Bytewise: 8 (a half lane, the ragged path alone) and one full tile plus
    a half-lane ragged tail.  Bit-sliced: one super-packet, and the whole packets that cover one tile of
    column space plus one more packet."""
    tile = tile_bytes(c.form)
    if not c.form.sliced:
        return (8, tile + 8)
    cols = -(-tile // c.packet) * c.packet + c.packet
    return (8 * c.packet, 8 * cols)


def make_plan(method, k, m, packet, size):
    p = L.Plan.new(method, size, k, m, 8, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


def distinct_forms(call, plans):
    """the forms `call` takes over plans (method, k, m, packet): what a table of codes reaches"""
    out = set()
    for method, k, m, packet in plans:
        if m in rows_of(call):
            out.add(predict(call, method, k, m, packet))
    return out
