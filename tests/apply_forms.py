"""Which plans run which kernel behind encode_dev, decode_dev and encode_magic_dev (a helper, not a test).

The oldest calls of the engine dispatch to several hundred separately compiled kernels: k_gf8_bytewise per row
count R, fixed or run-time input count KC, launch shape (IT steps of VW dwords, branch-free or not), with the
accumulate and the fused-magic instantiations, and -- where a kernel holds two whole tile loops -- the loop that
the flag of the launch's first cell selects; k_gf8_bitsliced per R and dwords per lane; the bitmatrix kernels per
word size; the GF(2^16) / GF(2^32) kernels per R, w and data layout.  ``E.predict_apply`` asks the engine -- the
functions its launches go through, no GPU -- what a K x R call launches, ``E.predict_apply_plan`` asks the same
of a plan's own matrices, and ``E.apply_record`` tells what a call did launch.

``cases(tier)`` yields, per tier,

* one representative per distinct form at the smallest K that gives it: the encode of a plan with m = R where the
  encode takes the form, a decode of a plan with m = R + 1 where only a decode does (the loop of a first row that
  is not all ones), and for the two-loop forms of the automatic policy a second decode that takes the first loop;
* the edge plans: no new form, but the ends of the input loop, the input groups of k > 64, the row launches of
  m > 8, both together, the 72-chunk plans of the fused magic and its two-pass fallback;
* decodes of fewer chunks than m on one plan per launch shape: data only, parity only and mixed losses.

Tiers: "auto" is the automatic policy with the compiled networks held off (E.hold_networks), which is what a
plan's first calls run; "variant" the kernels that only lsec_set_kernel_variant reaches (bytewise 1..5, bit-sliced
2 and 4); "wide" the kernels of kinds 3-5 (bitmatrix, GF(2^w) wordwise / transposed, GF(2^w) bit-sliced), under
the automatic policy and under bit-sliced variant 10 (the mask-per-bit kernel).

Nothing here is a count or a list of forms: both come from the engine at import time of the caller.  That time is
pytest's collection, so a GPU test file that calls cases() at import imports torch first, as the other form files do:
the engine library then shares torch's HIP runtime instead of loading a second one.
"""
import collections
import contextlib

import lstore_amd as L
from lstore_amd import erasure as E

KS = range(1, 65)
RS = range(1, 9)
SLICED_PACKETS = (8, 24, 64)  # 8 and 24 hold no lane of 4 dwords (DW falls to 2 where 4 is wanted), 64 does
BW_VARIANTS = (1, 2, 3, 4, 5)
BS_VARIANTS = (2, 4)
MASK_PER_BIT = 10  # lsec_set_kernel_variant's second value that picks k_gfw_wordwise
TIERS = ("auto", "variant", "wide")
BYTEWISE, BITSLICED, BITMATRIX, WORDWISE, BITSLICEDW = 1, 2, 3, 4, 5
LIBERATION_FAMILY = (L.LIBERATION, L.BLAUM_ROTH, L.LIBER8TION)

# tier, kind ("rep" / "edge" / "dec"), op ("enc" / "dec" / "magic"), the plan (method, k, m, w, packet), the two
# kernel-variant values, the erasures of a decode, the predicted forms of one unsplit call (a tuple, in launch
# order) and a word on why the case is there
Case = collections.namedtuple("Case", "tier kind op method k m w packet variants erasures forms why")


def small_size(packet, w=8):
    """a chunk size far below the 4 MiB at which the bit-sliced policy widens its lanes for K >= 10"""
    return w * packet if packet else 8


def big_size(packet):
    """just past 4 MiB (the prediction alone takes it: no GPU case does)"""
    return (4 << 20) // (8 * packet) * 8 * packet + 8 * packet if packet else (4 << 20) + 8


@contextlib.contextmanager
def variants(bw, bs):
    E.set_kernel_variant(bw, bs)
    try:
        yield
    finally:
        E.set_kernel_variant(0, 0)


def make_plan(method, k, m, w, packet, size):
    p = L.Plan.new(method, size, k, m, w, packet, 1 if method == L.RAID4 else 8)
    assert p.form_encoding_matrix() == 0 and p.form_decoding_matrix() == 0
    return p


_plan_forms = {}


def plan_forms(method, k, m, w, packet, vs, op, erasures=()):
    """what one unsplit call of the plan launches, from the plan's own matrices (no GPU)"""
    key = (method, k, m, w, packet, vs, op, tuple(erasures))
    if key not in _plan_forms:
        with make_plan(method, k, m, w, packet, small_size(packet, w)) as p, variants(*vs):
            _plan_forms[key] = tuple(E.predict_apply_plan(p, list(erasures) if op == "dec" else None,
                                                          small_size(packet, w), magic=op == "magic"))
    return _plan_forms[key]


def kernel_of(form):
    """the compiled kernel a form names: the any-w bitmatrix kernel takes its word size at run time"""
    return form._replace(w=0) if form.kind == BITMATRIX and not form.sub else form


# ---------------------------------------------------------------- the domains, from the prediction hook
def domain(tier):
    """every form the dispatch takes over the tier's domain, as {kernel_of(form)}: bytewise K x R x the first
    row's flag, bit-sliced K x R x packet x chunk size, each with and without the fused magic ("auto"), under
    every variant value ("variant")"""
    out = set()
    if tier == "auto":
        vss = ((0, 0),)
    elif tier == "variant":
        vss = tuple((b, 0) for b in BW_VARIANTS) + tuple((0, b) for b in BS_VARIANTS)
    else:
        return wide_domain()
    for vs in vss:
        for r in RS:
            for k in KS:
                for magic in ((False, True) if tier == "auto" else (False,)):
                    if vs[1] == 0:
                        for ones in (False, True):
                            out |= set(E.predict_apply(BYTEWISE, k, r, magic=magic, variants=vs, row_ones=[ones] + [False] * (r - 1)))
                    if vs[0] == 0:
                        for packet in SLICED_PACKETS:
                            for size in (small_size(packet), big_size(packet)):
                                out |= set(E.predict_apply(BITSLICED, k, r, 8, packet, size, magic, vs))
    if tier == "auto":  # the accumulate kernels of later input groups: k > 64
        for r in RS:
            out |= set(E.predict_apply(BYTEWISE, 65, r, row_ones=[True] + [False] * (r - 1)))
            out |= set(E.predict_apply(BITSLICED, 65, r, 8, 8, small_size(8)))
    return {kernel_of(f) for f in out}


def wide_domain():
    """kinds 3-5: every kernel the dispatch can launch for some K x R x w, K <= 64 and K = 65 (the accumulate
    kernels), under the automatic policy and the mask-per-bit variant; and every kernel a single launch of R = 1..8
    rows names (E.predict_apply_launch), whether or not the row split of a call ever hands a launch that many"""
    out = set()
    for r in RS:
        for w in (16, 32):
            for acc in (False, True):
                for kind, vss in ((WORDWISE, ((0, 0), (0, MASK_PER_BIT))), (BITSLICEDW, ((0, 0),))):
                    for vs in vss:
                        try:
                            out.add(E.predict_apply_launch(kind, 5, r, w, 8, acc=acc, variants=vs))
                        except E.ErasureError:
                            pass  # no kernel: the transposed and the bit-sliced kernels stop at 4 rows at w = 32
    for r in RS:
        for k in (1, 65):
            for w in range(2, 65):
                if r <= 2:
                    out |= set(E.predict_apply(BITMATRIX, k, r, w, 8))
                if w in (16, 32):
                    for bs in (0, MASK_PER_BIT):
                        out |= set(E.predict_apply(WORDWISE, k, r, w, variants=(0, bs)))
                    out |= set(E.predict_apply(BITSLICEDW, k, r, w, 8))
    return {kernel_of(f) for f in out}


# ---------------------------------------------------------------- representatives
def _enc_plan(kind, k, r):
    """the encode plan of a K x R form: RS, RAID4 where one row is wanted (bytewise), Cauchy-good (bit-sliced)"""
    if kind == BITSLICED:
        return L.CAUCHY_GOOD, k, r
    return (L.RAID4 if r == 1 else L.REED_SOL_VAN), k, r


def _loop_decodes(k, r):
    """erasure sets of r chunks on RS(k + (r+1)), by what they are meant to select: a data chunk lost together with
    parities other than row 0 leaves the all-ones row to the first output (loop 1); losing parity row 0 with it
    takes that row away, and so does a loss of parities other than row 0 alone (loop 0)"""
    return (
        (1, [0] + list(range(k + 1, k + r)), "data chunk 0 and parities other than row 0: the first row is all ones"),
        (0, [0] + list(range(k, k + r - 1)), "data chunk 0 and parity row 0: the all-ones row is gone"),
        (0, list(range(k + 1, k + r + 1)), "parities other than row 0"),
    )


def representatives(tier):
    if tier == "wide":
        return wide_cases()
    seen, out = set(), []
    vss = ((0, 0),) if tier == "auto" else tuple((b, 0) for b in BW_VARIANTS) + tuple((0, b) for b in BS_VARIANTS)

    def add(op, method, k, m, packet, vs, erasures, why, want_loop=None, again=False):
        forms = plan_forms(method, k, m, 8, packet, vs, op, erasures)
        if len(forms) != 1 or (want_loop is not None and forms[0].loop != want_loop):
            return False
        if forms[0] in seen and not again:
            return False
        seen.add(forms[0])
        out.append(Case(tier, "rep", op, method, k, m, 8, packet, vs, tuple(erasures), forms, why))
        return True

    for vs in vss:
        for kind in ((BYTEWISE,) if vs[0] else (BITSLICED,) if vs[1] else (BYTEWISE, BITSLICED)):
            for r in RS:
                for k in KS:
                    for packet in (SLICED_PACKETS if kind == BITSLICED else (0,)):
                        method, _, m = _enc_plan(kind, k, r)
                        for op in (("enc", "magic") if tier == "auto" else ("enc",)):
                            add(op, method, k, m, packet, vs, (), "smallest K of its form")
                        if kind == BYTEWISE and r >= 2:
                            # the loops only a decode selects, on a plan with m > R
                            for loop, er, why in _loop_decodes(k, r):
                                first = add("dec", L.REED_SOL_VAN, k, r + 1, 0, vs, er, why, want_loop=loop)
                                if first and loop == 0 and tier == "auto":
                                    # ... and with it the set that gives the other loop of the same kernel
                                    l1, er1, why1 = _loop_decodes(k, r)[0]
                                    add("dec", L.REED_SOL_VAN, k, r + 1, 0, vs, er1, why1, want_loop=l1, again=True)
    if tier == "auto":  # the accumulate kernels: the second input group of k = 65, one per row count
        for kind in (BYTEWISE, BITSLICED):
            for r in RS:
                method, k, m = _enc_plan(kind, 65, r)
                forms = plan_forms(method, k, m, 8, 8 if kind == BITSLICED else 0, (0, 0), "enc")
                if not set(forms) <= seen:
                    seen.update(forms)
                    out.append(Case(tier, "rep", "enc", method, k, m, 8, 8 if kind == BITSLICED else 0, (0, 0), (), forms,
                                    "k = 65: the accumulate kernel of its row count"))
    return out


def never_reached(tier):
    """the forms of domain(tier) that no plan's own matrices reach, by the reason (a predicate on the form):
    * the fused magic runs encodes alone, and the first row of every encode matrix the plan service builds for a
      bytewise code (RS, r6) is all ones: a two-loop fused-magic kernel never takes its other loop;
    * k_bitmatrix<R, 32>: no liberation-family plan has w = 32 (32 is not prime, 33 is not, liber8tion has w = 8),
      and Cauchy at w = 32 runs k_gfw_bitsliced;
    * the mask-per-bit k_gfw_wordwise<R, 32> of five to eight rows, plain and accumulating: a call's launches get at
      most four rows at w = 32 (E.predict_apply never hands a launch more), under the automatic policy and under
      variant 10 alike."""
    if tier == "auto":
        return {f for f in domain(tier) if f.kind == BYTEWISE and f.magic and f.loop == 0}
    if tier == "wide":
        return {f for f in domain(tier) if (f.kind == BITMATRIX and f.sub and f.w == 32) or
                (f.kind == WORDWISE and not f.sub and f.w == 32 and f.R > max(x.R for x in E.predict_apply(WORDWISE, 5, 8, 32)))}
    return set()


# ---------------------------------------------------------------- edge plans
# (op, method, k, m, packet, why)
EDGES = (
    ("enc", L.RAID4, 1, 1, 0, "K = 1, one row"),
    ("enc", L.REED_SOL_VAN, 1, 2, 0, "K < 4: one input"),
    ("enc", L.REED_SOL_VAN, 2, 7, 0, "K < 4: two inputs, seven rows"),
    ("enc", L.REED_SOL_VAN, 3, 6, 0, "K < 4: three inputs, six rows"),
    ("enc", L.REED_SOL_VAN, 17, 2, 0, "run-time K at 16 B per lane, the four-at-a-time loop ends in one input"),
    ("enc", L.REED_SOL_VAN, 18, 3, 0, "... in two"),
    ("enc", L.REED_SOL_VAN, 19, 5, 0, "... in three"),
    ("enc", L.REED_SOL_VAN, 64, 8, 0, "k = 64: one full input group, eight rows"),
    ("enc", L.CAUCHY_GOOD, 64, 8, 8, "k = 64, bit-sliced"),
    ("enc", L.REED_SOL_VAN, 65, 4, 0, "k = 65: an accumulate group of one input"),
    ("enc", L.REED_SOL_VAN, 128, 4, 0, "k = 128: an accumulate group of 64 inputs"),
    ("enc", L.REED_SOL_VAN, 200, 4, 0, "k = 200: three accumulate groups, the last of 8 inputs"),
    ("enc", L.CAUCHY_GOOD, 65, 4, 8, "k = 65, bit-sliced"),
    ("enc", L.CAUCHY_GOOD, 128, 4, 8, "k = 128, bit-sliced"),
    ("enc", L.CAUCHY_GOOD, 200, 4, 8, "k = 200, bit-sliced"),
    ("enc", L.REED_SOL_VAN, 10, 9, 0, "m = 9: row launches 8 + 1, the ninth row on the one-row shape"),
    ("enc", L.REED_SOL_VAN, 10, 16, 0, "m = 16: row launches 8 + 8"),
    ("enc", L.REED_SOL_VAN, 10, 17, 0, "m = 17: row launches 8 + 8 + 1"),
    ("enc", L.CAUCHY_GOOD, 10, 9, 8, "m = 9, bit-sliced"),
    ("enc", L.REED_SOL_VAN, 70, 10, 0, "k = 70, m = 10: input groups and row launches together"),
    ("magic", L.REED_SOL_VAN, 64, 8, 0, "72 chunks: chunk id 71, the largest position weight"),
    ("magic", L.CAUCHY_GOOD, 64, 8, 8, "72 chunks, bit-sliced"),
    ("magic", L.REED_SOL_VAN, 12, 10, 0, "the two-pass magic: m > 8"),
    ("magic", L.REED_SOL_VAN, 65, 3, 0, "the two-pass magic: k > 64"),
    ("magic", L.REED_SOL_VAN, 17, 2, 0, "fused magic, run-time K ends in one input"),
    ("magic", L.REED_SOL_VAN, 3, 6, 0, "fused magic, K < 4"),
)
WIDE_PLANS = ((L.REED_SOL_VAN, 200, 4, 0), (L.CAUCHY_GOOD, 200, 4, 8), (L.REED_SOL_VAN, 64, 8, 0), (L.CAUCHY_GOOD, 64, 8, 8),
              (L.REED_SOL_VAN, 128, 4, 0), (L.CAUCHY_GOOD, 128, 4, 8))  # these run one chunk size


def edges():
    out = []
    for op, method, k, m, packet, why in EDGES:
        out.append(Case("auto", "edge", op, method, k, m, 8, packet, (0, 0), (), plan_forms(method, k, m, 8, packet, (0, 0), op), why))
    return out


# decodes of fewer chunks than m, one plan per launch shape of the automatic policy: (method, k, m, packet)
PARTIAL_PLANS = (
    (L.REED_SOL_VAN, 10, 8, 0),   # 2 x 16 B per lane
    (L.REED_SOL_VAN, 21, 8, 0),   # 16 B per lane
    (L.CAUCHY_GOOD, 6, 4, 8),     # one dword per lane
    (L.CAUCHY_GOOD, 16, 4, 64),   # four
)


def partial_decodes():
    out = []
    for method, k, m, packet in PARTIAL_PLANS:
        for r in range(1, m):
            sets = (("data only", list(range(r))), ("parity only", list(range(k, k + r))),
                    ("parity only, without row 0", list(range(k + 1, k + 1 + r))))
            if r >= 2:
                sets += (("mixed", [1] + list(range(k + m - r + 1, k + m))), ("mixed, with parity row 0", [1, k] + list(range(2, r))))
            for what, er in sets:
                er = sorted(er)
                forms = plan_forms(method, k, m, 8, packet, (0, 0), "dec", er)
                out.append(Case("auto", "dec", "dec", method, k, m, 8, packet, (0, 0), tuple(er), forms, f"{r} of {m} lost: {what}"))
    return out


# ---------------------------------------------------------------- kinds 3-5
def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def bitmatrix_plans():
    """(method, k, w) of the liberation family over the word sizes it can have up to 64: liberation w prime (and
    k <= w), blaum_roth w + 1 prime, liber8tion w = 8; the smallest w past 64 for a plan of k > 64"""
    out = []
    for w in range(2, 65):
        if _is_prime(w):
            out.append((L.LIBERATION, min(w, 3), w))
        if _is_prime(w + 1):
            out.append((L.BLAUM_ROTH, min(w, 3), w))
        if w == 8:
            out.append((L.LIBER8TION, 3, w))
    out.append((L.LIBERATION, 65, 67))
    return out


def _try_forms(method, k, m, w, packet, vs, op, er=()):
    try:
        return plan_forms(method, k, m, w, packet, vs, op, er)
    except (E.ErasureError, AssertionError):
        return None  # the plan service refuses the shape


def wide_cases():
    """one case per kernel of kinds 3-5 that a plan reaches, at the first plan that gives it"""
    seen, out = set(), []

    def add(op, method, k, m, w, packet, vs, er, why):
        forms = _try_forms(method, k, m, w, packet, vs, op, er)
        if not forms or {kernel_of(f) for f in forms} <= seen:
            return
        seen.update(kernel_of(f) for f in forms)
        out.append(Case("wide", "rep", op, method, k, m, w, packet, vs, tuple(er), forms, why))

    for method, k, w in bitmatrix_plans():
        name = L.JE_METHOD_NAMES[method]
        add("enc", method, k, 2, w, 8, (0, 0), (), f"{name} w = {w}: two rows")
        add("dec", method, k, 2, w, 8, (0, 0), (0,), f"{name} w = {w}: one row, a single loss")
        if k > 64:
            add("dec", method, k, 2, w, 8, (0, 0), (0, 1), f"{name} w = {w}: a double loss of k > 64")
    for w in (16, 32):
        for bs in (0, MASK_PER_BIT):
            what = "mask-per-bit" if bs else "transposed"
            for r in RS:
                add("enc", L.REED_SOL_VAN, 5, r, w, 0, (0, bs), (), f"RS w = {w}, {what}: {r} rows")
            for r in RS:
                add("enc", L.REED_SOL_VAN, 65, r, w, 0, (0, bs), (), f"RS w = {w}, {what}: an accumulate group, {r} rows")
            add("enc", L.REED_SOL_VAN, 5, 9, w, 0, (0, bs), (), f"RS w = {w}, {what}: nine rows, the row launches")
        for r in RS:
            add("enc", L.CAUCHY_GOOD, 5, r, w, 8, (0, 0), (), f"Cauchy w = {w}: {r} rows")
        for r in RS:
            add("enc", L.CAUCHY_GOOD, 65, r, w, 8, (0, 0), (), f"Cauchy w = {w}: an accumulate group, {r} rows")
    return out


# ---------------------------------------------------------------- all of a tier
def cases(tier):
    """the representatives, then (auto) the edge plans and the partial decodes"""
    out = list(representatives(tier))
    if tier == "auto":
        have = {(c.op, c.method, c.k, c.m, c.packet, c.erasures) for c in out}
        out += [c for c in edges() + partial_decodes() if (c.op, c.method, c.k, c.m, c.packet, c.erasures) not in have]
    return out


def forms_run(tier):
    return {kernel_of(f) for c in cases(tier) for f in c.forms}


def form_id(f):
    if f.kind == BYTEWISE:
        s = f"r{f.R}_kc{f.KC}_it{f.IT}_vw{f.VW}{'' if f.BF else '_br'}" + ("" if f.loop < 0 else f"_loop{f.loop}")
    elif f.kind == BITSLICED:
        s = f"r{f.R}_dw{f.DW}"
    else:
        s = f"kind{f.kind}_r{f.R}_w{f.w}_{'ab'[f.sub]}"
    return s + ("_acc" if f.acc else "") + ("_mg" if f.magic else "")


def case_id(c):
    plan = f"{L.JE_METHOD_NAMES[c.method]}_{c.k}+{c.m}" + (f"_w{c.w}" if c.w != 8 else "") + (f"_p{c.packet}" if c.packet else "")
    vs = f"-v{c.variants[0]}.{c.variants[1]}" if c.variants != (0, 0) else ""
    er = "-lost" + ".".join(map(str, c.erasures)) if c.op == "dec" else ""
    forms = form_id(c.forms[0]) + (f"_x{len(c.forms)}" if len(c.forms) != 1 else "") if c.forms else "none"
    return f"{c.tier}-{c.kind}-{c.op}-{plan}{vs}{er}-{forms}"


def tile_bytes(c):
    """bytes of chunk (column space for the packet kinds) that one workgroup's tile of the case's widest launch covers"""
    f = max(c.forms, key=lambda f: (f.IT * f.VW, f.DW)) if c.forms else None
    if f is None or f.kind == BYTEWISE:
        return 256 * 4 * (f.VW * f.IT if f else 8)
    if f.kind == BITSLICED:
        return 1024 * f.DW
    if f.kind == WORDWISE:
        return 256 * (4 * f.w if f.sub else 16 if f.w == 16 else 8)
    return 1024  # k_bitmatrix, k_gfw_bitsliced: 256 lanes of one dword of column space


def sizes(c):
    """the chunk sizes of a case.  Byte kernels: 8 (a half lane, the ragged path alone) and one full tile plus a
    half-lane ragged tail.  Packet kernels: one super-packet, and the whole packets that cover one tile of column
    space plus one more packet.  The wide plans run the larger size alone."""
    tile = tile_bytes(c)
    if not c.packet:
        both = (8, tile + 8)
    else:
        cols = -(-tile // c.packet) * c.packet + c.packet
        both = (c.w * c.packet, c.w * cols)
    return both[1:] if (c.method, c.k, c.m, c.packet) in WIDE_PLANS else both


# ---------------------------------------------------------------- what the tables of codes reached
def table_forms():
    """{kernel_of(form)} that the tables of codes of tests/test_gpu_layouts.py and tests/test_gpu_parity.py reach at
    their own shapes: every encode and decode of theirs, and the fused magics, as the automatic policy with no network
    ready launches them, and their variant sweeps (a table that runs with a network ready reaches less)"""
    import test_gpu_layouts as TL
    import test_gpu_parity as TP

    out = set()

    def plan(method, k, m, w, packet, erasure_sets, vs=(0, 0), magic=False):
        f = _try_forms(method, k, m, w, packet, vs, "magic" if magic else "enc")
        out.update(kernel_of(x) for x in f or ())
        for er in erasure_sets:
            out.update(kernel_of(x) for x in _try_forms(method, k, m, w, packet, vs, "dec", sorted(er)) or ())

    for c in TL.CASES:
        plan(c.method, c.k, c.m, c.w, c.packet, c.erasures, (0, 1) if c.path == "variant" else (0, 0))
    for c in TL.MAGIC_CASES:
        plan(c.method, c.k, c.m, c.w, c.packet, (), magic=True)
    plan(L.RAID4, 1, 1, 8, 0, (), magic=True)
    rs63 = TL.BY_ID["rs63"]
    for b in BW_VARIANTS:
        plan(rs63.method, rs63.k, rs63.m, 8, 0, rs63.erasures, (b, 0))
    for b in BS_VARIANTS:
        plan(L.CAUCHY_GOOD, 6, 3, 8, 64, ([0], [1, 7], [2, 6, 7]), (0, b))
    for method, k, m, w, packet, er in randomized_plans(TP):
        plan(method, k, m, w, packet, er)
    return out


def randomized_plans(TP):
    """(method, k, m, w, packet, erasure sets) of test_gpu_parity.test_randomized_plans_vs_oracle: its seeded draws,
    replayed in its order (its decode goes through the host path, which launches by the same dispatch).  A snapshot
    of that test as it stands: it feeds the "older tables reached" figure of coverage() alone, no assertion"""
    import numpy as np

    assert hasattr(TP, "test_randomized_plans_vs_oracle")
    rng = np.random.default_rng(20261016)
    out = []
    for case in range(48):
        method = int(rng.choice([L.REED_SOL_VAN, L.REED_SOL_R6_OP, L.CAUCHY_ORIG, L.CAUCHY_GOOD, L.RAID4]))
        w = 8 if method == L.RAID4 or case % 4 else int(rng.choice([16, 32]))
        k = int(rng.integers(1, 25))
        m = 2 if method == L.REED_SOL_R6_OP else 1 if method == L.RAID4 else int(rng.integers(1, 9))
        if method in (L.CAUCHY_ORIG, L.CAUCHY_GOOD):
            packet = 8 * int(rng.integers(1, 17))
            size = w * packet * int(rng.integers(1, 5))
        else:
            packet = 0
            size = 8 * int(rng.integers(1, 1025))
        n = int(rng.integers(1, 4))
        rng.integers(0, 256, (n, k, size), dtype=np.uint8)
        e = int(rng.integers(1, m + 1))
        lost = sorted(rng.choice(k + m, size=e, replace=False).tolist())
        out.append((method, k, m, w, packet, () if method == L.RAID4 and lost[0] >= k else (lost,)))
    return out


def coverage(tier):
    """(forms of the tier's domain, of those the older tables reach, of those cases(tier) runs)"""
    every = domain(tier)
    return len(every), len(table_forms() & every), len(forms_run(tier) & every), len(never_reached(tier))


if __name__ == "__main__":
    # the figures of DESIGN.md 3.5: PYTHONPATH=. python tests/apply_forms.py
    for t in TIERS:
        print("%-8s %3d forms, %3d reached by the older tables of codes, %3d run by tests/apply_forms.py's cases, %2d that no plan reaches"
              % ((t,) + coverage(t)))
