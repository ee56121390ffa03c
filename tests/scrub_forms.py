"""Which plans run which kernel of the check / locate / patterned-decode families (a helper, not a test).

Each of lsec_check_dev, lsec_locate_dev, their _rotated twins and lsec_decode_dev_patterns is a family
of separately compiled kernels: per parity-row count R, and bytewise per input count (fixed-K forms,
K at run time at 2 x 16 B and at 16 B per lane, the 8 B shape of R == 1), bit-sliced per dwords per
lane.  ``E.predict_form`` asks the engine -- the functions its dispatch calls, no GPU -- which form
a plan takes.  ``cases(call)`` enumerates K = 1..64 x R x packet through it and yields

* one representative plan per distinct form, at the smallest K that produces the form, and
* the edge plans: no new form, but the boundaries of the input loop, of the 64-bit hypothesis mask
  and of the documented limits.

The nine families added since -- the parity updates (plain, rotated, masked, masked with the magics), the
rotated encodes and the magic scrubs and decodes -- are the twelve call names of NEW_CALLS, each asked of
the prediction hook its own test file asks (_HOOKS).  Their cases are built the same way, with two
differences: an update's form does not depend on K bytewise, so its representatives start at K = 5, and the
magic calls carry the two 72-chunk plans whose last chunk id has the largest position weight.

Nothing here is a count or a list of forms: both come from the engine at import time of the caller.
"""
import collections

import lstore_amd as L
from lstore_amd import erasure as E

CALLS = ("chk", "loc", "chkrot", "locrot", "pat")
# the calls added since, by what tests/test_gpu_write_forms.py and tests/test_gpu_magic_forms.py run
WRITE_CALLS = ("upd", "updrot", "encrot", "updmask", "updmaskrot", "updmagic", "updmagicrot")
MAGIC_FORM_CALLS = ("chkmagic", "chkmagicrot", "patmagic", "patmagicrot", "encmagicrot")
NEW_CALLS = WRITE_CALLS + MAGIC_FORM_CALLS
UPDATES = ("upd", "updrot", "updmask", "updmaskrot", "updmagic", "updmagicrot")
MASKED = ("updmask", "updmaskrot", "updmagic", "updmagicrot")
PATTERNED = ("pat", "patmagic", "patmagicrot")
WITH_MAGICS = ("updmagic", "updmagicrot", "chkmagic", "chkmagicrot", "patmagic", "patmagicrot", "encmagicrot")
ROTATED = ("chkrot", "locrot", "updrot", "encrot", "updmaskrot", "updmagicrot", "chkmagicrot", "patmagicrot", "encmagicrot")
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


# call -> its prediction hook as f(plan kernel, k, rows, packet, chunk size); a rotated twin of a masked, a
# masked-magic or a patterned-magic call launches its plain twin's family
_HOOKS = {
    "upd": lambda *a: E.predict_form("upd", *a),
    "updrot": lambda *a: E.predict_form("updrot", *a),
    "encrot": lambda *a: E.predict_form("encrot", *a),
    "updmask": lambda *a: E.predict_masked_form(*a),
    "updmaskrot": lambda *a: E.predict_masked_form(*a),
    "updmagic": lambda *a: E.predict_masked_magic_form(*a),
    "updmagicrot": lambda *a: E.predict_masked_magic_form(*a),
    "patmagic": lambda kernel, k, rows, packet, size: E.predict_pattern_magic_form(kernel, k, rows, packet),
    "patmagicrot": lambda kernel, k, rows, packet, size: E.predict_pattern_magic_form(kernel, k, rows, packet),
    "chkmagic": lambda *a: E.predict_check_magic_form(False, *a),
    "chkmagicrot": lambda *a: E.predict_check_magic_form(True, *a),
    "encmagicrot": lambda *a: E.predict_encode_magic_form(*a),
}
assert set(_HOOKS) == set(NEW_CALLS)


def predict(call, method, k, rows, packet, size=None):
    size = small_size(packet) if size is None else size
    if call in _HOOKS:
        return _HOOKS[call](plan_kernel(method), k, rows, packet, size)
    return E.predict_form(call, plan_kernel(method), k, rows, packet, size)


def ks_of(call):
    """the order in which representatives() walks K.  An update's bytewise form depends on R alone and its
    bit-sliced one on K only through the dwords per lane, so the smallest K of a form would be 1, which the masked
    rigs cannot express: K = 5 first (odd, no fixed K, the k >= 4 the masked rigs document), then upwards, then
    the K below 5"""
    return tuple(range(5, 65)) + tuple(range(1, 5)) if call in UPDATES else tuple(KS)


def _plan_for(call, sliced, k, rows):
    """the plan of a representative: RS, RAID4 where one row is wanted (bytewise), Cauchy-good (bit-sliced);
    a patterned table of `rows` erasures needs m >= rows, and two rows so that there is parity to lose"""
    m = max(rows, 2) if call in PATTERNED else rows
    if sliced:
        return L.CAUCHY_GOOD, k, m
    return (L.RAID4 if m == 1 else L.REED_SOL_VAN), k, m


def representatives(call):
    """one Case per distinct predicted form of `call`, at the smallest K (an update: ks_of; then the first
    packet) giving it"""
    seen, out = set(), []
    why = "K = 5, or the first K from there of its form" if call in UPDATES else "smallest K of its form"
    for sliced in (False, True):
        for rows in rows_of(call):
            for k in ks_of(call):
                for packet in (SLICED_PACKETS if sliced else (0,)):
                    method, _, m = _plan_for(call, sliced, k, rows)
                    form = predict(call, method, k, rows, packet)
                    if form not in seen:
                        seen.add(form)
                        out.append(Case(call, "rep", method, k, m, packet, rows, form, why))
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
# test_gpu_check_magic.EDGES: the calls that sum magics weigh chunk id 71 heaviest.  (Both plans are in EDGES
# already, for their k = 64; they are named here so that they stay if EDGES moves.)
MAGIC_EDGES = (
    (L.REED_SOL_VAN, 64, 8, 0, "72 chunks: chunk id 71, the largest position weight"),
    (L.CAUCHY_GOOD, 64, 8, 8, "72 chunks, bit-sliced"),
)


def edges(call):
    out, have = [], set()
    # (RS(64+64) is the plain patterned decode's alone: the decodes that leave the magics take m <= 8, as the other
    # magic calls do -- include/lstore_ec.h; tests/test_scrub_forms.py has the refusal)
    more = (PAT_ONLY_EDGES if call == "pat" else ()) + (MAGIC_EDGES if call in WITH_MAGICS else ())
    for method, k, m, packet, why in EDGES + more:
        if m not in rows_of(call) and call not in PATTERNED:
            continue  # one row cannot locate
        if (method, k, m, packet) in have:
            continue
        if call in MASKED and k < 4:
            # the masked rigs' seven mask words need four columns (bits 0, k-2, 2, 3 and the disabled column 1), and
            # the masked kernels walk the set bits of a word: they have no path that depends on K < 4
            continue
        have.add((method, k, m, packet))
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


# ---------------------------------------------------------------- what the tables of codes reached
def table_plans(call):
    """(method, k, m, packet, rows, size) of every plan and chunk size the family's own test file runs `call` at:
    its table of codes at its own shapes (the patterned decodes: at the table heights its tests build)"""
    import test_gpu_check_magic as TCM
    import test_gpu_decode_magic as TDM
    import test_gpu_encode_magic_rotated as TEM
    import test_gpu_rotated_write as TRW
    import test_gpu_update as TU
    import test_gpu_update_magic as TUM
    import test_gpu_update_masked as TM

    def plans(mod, codes, shapes=None, rows=None):
        out = []
        for code in codes:
            method, k, m, _ = mod.spec(code)
            for packet, size in (shapes or mod.shapes)(code):
                out += [(method, k, m, packet, r, size) for r in (rows(code) if rows else (m,))]
        return out

    edge = lambda mod: (lambda code: [mod.edge_shape(code)])  # noqa: E731
    if call == "upd":
        return plans(TU, sorted({code for code, _ in TU.CASES}))
    if call in ("updrot", "encrot"):
        return plans(TRW, TRW.CODES)
    if call in ("updmask", "updmaskrot"):
        return plans(TM, TM.ALL if call == "updmask" else TM.ROTATED)
    if call in ("updmagic", "updmagicrot"):
        return plans(TM, TUM.ALL if call == "updmagic" else TUM.ROTATED, TUM.shapes)
    if call in ("chkmagic", "chkmagicrot"):
        return plans(TCM, TCM.NAMES if call == "chkmagic" else TCM.ROTATED) + plans(TCM, TCM.EDGES, edge(TCM))
    if call == "encmagicrot":
        return plans(TEM, TEM.NAMES) + plans(TEM, TEM.EDGES, edge(TEM))
    if call == "patmagic":
        # every code at its m erasures; one-row tables, and the two-erasure tables of the corrupt-survivor tests
        heights = {"rs63": (1, 2, 3), "raid4_61": (1,), "r6_62": (1, 2), "cg63": (1, 2, 3)}
        return plans(TDM, TDM.CODES, rows=lambda code: heights.get(code, (TDM.spec(code)[2],)))
    if call == "patmagicrot":
        return plans(TDM, TDM.ROTATED, rows=lambda code: (1, 2))
    raise KeyError(call)


def coverage(call):
    """(forms in the domain of tests/test_scrub_forms.py's closure test, of those the family's own table of codes
    reaches, of those cases(call) runs)"""
    every = set()
    for method, packets in ((L.REED_SOL_VAN, (0,)), (L.CAUCHY_GOOD, SLICED_PACKETS)):
        for r in rows_of(call):
            for k in KS:
                for packet in packets:
                    big = (4 << 20) // (8 * packet) * 8 * packet + 8 * packet if packet else 4 << 20
                    every |= {predict(call, method, k, r, packet, size) for size in (small_size(packet), big)}
    table = {predict(call, method, k, rows, packet, size) for method, k, m, packet, rows, size in table_plans(call)}
    return len(every), len(table & every), len({c.form for c in cases(call)} & every)


if __name__ == "__main__":
    # the figures of DESIGN.md 3.5: PYTHONPATH=. python tests/scrub_forms.py
    for name in NEW_CALLS:
        print("%-12s %3d forms, %2d reached by its table of codes, %3d run by tests/scrub_forms.py's cases" % ((name,) + coverage(name)))
