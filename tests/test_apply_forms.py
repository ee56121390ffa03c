"""CPU: the enumeration of tests/apply_forms.py reaches every kernel form behind lsec_encode_dev, lsec_decode_dev and
lsec_encode_magic_dev, and every plan it yields is one the calls accept.  No GPU: the forms come from
E.predict_apply (what one K x R call launches, asked of the functions the launches go through) and
E.predict_apply_plan (the same from a plan's own matrices: its kernel kind, its row count and which of its rows are
all ones), the validation from the calls with nstripes == 0.

Nothing here is a count of forms.  The expectations are properties of the dispatch: the launch split it shares with
enqueue_apply, every K of LSEC_FIXED_K (E.fixed_k()) a fixed form and no other K, five launch shapes under the
variants, and a form being a function of what the dispatch looks at, so that an enumeration over the domain finds it.
The kernels that no plan reaches are named by a reason (AF.never_reached) and printed, not skipped.
"""
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import apply_forms as AF

FAKE = 0x7F0000000000


@pytest.fixture(scope="module")
def all_cases(built):
    return {tier: AF.cases(tier) for tier in AF.TIERS}


@pytest.fixture(scope="module")
def domains(built):
    return {tier: AF.domain(tier) for tier in AF.TIERS}


# ---------------------------------------------------------------- the closure
@pytest.mark.parametrize("tier", AF.TIERS)
def test_closure(all_cases, domains, tier):
    """THE completeness condition: every form the hook predicts anywhere in the tier's domain is launched by some
    case, but for the forms that no plan of the library's own matrices reaches, which are exactly the ones
    AF.never_reached names by reason; ids are unique"""
    every, have = domains[tier], {AF.kernel_of(f) for c in all_cases[tier] for f in c.forms}
    never = AF.never_reached(tier)
    assert never <= every
    assert every - have == never, f"{tier}: no case for {sorted(map(AF.form_id, every - have - never))}; reached after all: " \
                                  f"{sorted(map(AF.form_id, never & have))}"
    ids = [AF.case_id(c) for c in all_cases[tier]]
    assert len(ids) == len(set(ids))
    if never:
        print(f"\n{tier}: compiled, launched by no plan: " + " ".join(sorted(map(AF.form_id, never))))
    # the two tiers of kinds 1 and 2 run nothing outside their domains but the launches of the edge plans
    if tier == "variant":
        assert have == every
    rep = [c for c in all_cases[tier] if c.kind == "rep"]
    assert {AF.kernel_of(f) for c in rep for f in c.forms} >= every - never  # the representatives alone close it


def test_the_tiers_do_not_hide_in_each_other(domains):
    """the automatic policy reaches a part of the bytewise kernels and the variants the rest: together the five shapes
    x R x KC, each K of LSEC_FIXED_K and run-time K"""
    plain = lambda forms: {(f.R, f.KC, f.IT, f.VW, f.BF) for f in forms if f.kind == AF.BYTEWISE and not f.acc and not f.magic}  # noqa: E731
    auto, var = plain(domains["auto"]), plain(domains["variant"])
    assert auto < var
    shapes = {(it, vw, bf) for _, _, it, vw, bf in var}
    assert shapes == {(2, 4, 1), (1, 4, 1), (2, 2, 1), (1, 2, 1), (1, 2, 0)}
    assert var == {(r, kc) + sh for r in AF.RS for kc in (0,) + E.fixed_k() for sh in shapes}
    # the automatic policy: the branchy 8 B shape for one row, 2 x 16 B below K = 16 and 16 B from there for more
    assert {(it, vw, bf) for r, _, it, vw, bf in auto if r == 1} == {(1, 2, 0)}
    for r in range(2, 9):
        assert {(kc, it) for rr, kc, it, vw, bf in auto if rr == r} == \
            {(kc, 2) for kc in (0,) + E.fixed_k() if kc < 16} | {(kc, 1) for kc in (0,) + E.fixed_k() if kc == 0 or kc >= 16}
    sliced = lambda forms: {(f.R, f.DW) for f in forms if f.kind == AF.BITSLICED and not f.acc and not f.magic}  # noqa: E731
    assert sliced(domains["auto"]) == {(r, dw) for r in AF.RS for dw in ((1, 2, 4) if r <= 4 else (1,))}
    assert sliced(domains["variant"]) == {(r, dw) for r in AF.RS for dw in (2, 4)}


def test_fused_magic_and_accumulate_forms(domains):
    magic = {f for f in domains["auto"] if f.magic}
    assert {(f.R, f.KC, f.IT) for f in magic if f.kind == AF.BYTEWISE} == \
        {(r, kc, 1 if kc >= 16 else 2) for r in AF.RS for kc in E.fixed_k()} | {(r, 0, it) for r in AF.RS for it in (1, 2)}
    assert all((f.VW, f.BF) == (4, 1) for f in magic if f.kind == AF.BYTEWISE)
    assert {(f.R, f.DW) for f in magic if f.kind == AF.BITSLICED} == {(r, 1) for r in AF.RS}
    acc = {f for f in domains["auto"] if f.acc}
    assert {(f.kind, f.R) for f in acc} == {(kind, r) for kind in (AF.BYTEWISE, AF.BITSLICED) for r in AF.RS}
    assert all(f.loop <= 0 for f in acc)  # a later group's first cell never carries the flag


def test_two_loop_forms_take_both_loops_in_decodes(all_cases):
    """every two-loop kernel of the automatic policy (R >= 2) has a decode of R chunks on a plan with m > R for each of
    its loops, and the prediction from the plan's own decode rows says that each set selects the loop it is meant to"""
    decs = [c for c in all_cases["auto"] if c.kind == "rep" and c.op == "dec"]
    assert decs and all(c.m > len(c.erasures) and len(c.forms) == 1 for c in decs)
    by_kernel = {}
    for c in decs:
        by_kernel.setdefault(c.forms[0]._replace(loop=0), set()).add(c.forms[0].loop)
    two_loop = {f._replace(loop=0) for f in AF.domain("auto") if f.kind == AF.BYTEWISE and f.loop >= 0 and not f.magic and not f.acc}
    assert set(by_kernel) == two_loop
    assert all(loops == {0, 1} for loops in by_kernel.values()), {AF.form_id(k): v for k, v in by_kernel.items() if v != {0, 1}}
    for c in decs:
        if c.forms[0].loop == 1:
            assert c.k not in c.erasures and c.erasures[0] < c.k, AF.case_id(c)  # parity row 0 survives, a data chunk comes first
    # the same kernels' loops under the variants: the encode gives the first, one decode the other
    for kern in {f._replace(loop=0) for f in AF.domain("variant") if f.loop >= 0}:
        got = {c.op for c in all_cases["variant"] if c.forms[0]._replace(loop=0) == kern}
        assert got == {"enc", "dec"}, AF.form_id(kern)


# ---------------------------------------------------------------- the launch split
def test_launch_split_of_wide_and_tall_plans(built):
    """input groups of 64 (the later ones accumulate, at 16 B per lane), row launches of 8 -- 2 for the bitmatrix
    kernels, 4 at w = 32 -- in the order enqueue_apply walks: groups outside, rows inside"""
    def split(kind, k, r, w=8, packet=0, **kw):
        return [(f.R, f.acc) for f in E.predict_apply(kind, k, r, w, packet, AF.small_size(packet, w), **kw)]

    assert split(1, 10, 9) == [(8, 0), (1, 0)]
    assert split(1, 10, 16) == [(8, 0), (8, 0)]
    assert split(1, 10, 17) == [(8, 0), (8, 0), (1, 0)]
    assert split(1, 65, 4) == [(4, 0), (4, 1)] and split(1, 128, 4) == [(4, 0), (4, 1)]
    assert split(1, 200, 4) == [(4, 0)] + [(4, 1)] * 3
    assert split(1, 70, 10) == [(8, 0), (2, 0), (8, 1), (2, 1)]
    assert split(1, 200, 17) == ([(8, 0)] * 2 + [(1, 0)]) + ([(8, 1)] * 2 + [(1, 1)]) * 3
    assert len(split(1, 200, 17)) <= E.APPLY_RECORD_MAX
    assert split(2, 70, 10, 8, 8) == [(8, 0), (2, 0), (8, 1), (2, 1)]
    assert split(4, 5, 9, 32) == [(4, 0), (4, 0), (1, 0)] and split(4, 5, 9, 16) == [(8, 0), (1, 0)]
    assert split(5, 5, 6, 32, 8) == [(4, 0), (2, 0)]
    # RS(k+9): the ninth row runs alone, on the one-row shape with per-cell branches
    ninth = E.predict_apply(1, 10, 9)[1]
    assert (ninth.R, ninth.KC, ninth.IT, ninth.VW, ninth.BF, ninth.loop) == (1, 10, 1, 2, 0, -1)
    # an accumulate launch is generic-K at 16 B per lane whatever the shape of the first group
    for v in (0,) + AF.BW_VARIANTS:
        a = E.predict_apply(1, 70, 3, variants=(v, 0))[1]
        assert (a.KC, a.IT, a.VW, a.BF, a.acc) == (0, 1, 4, 1, 1)
    # the fused magic is one launch where it fuses, the encode's launches where it does not
    assert [f.magic for f in E.predict_apply(1, 64, 8, magic=True)] == [1]
    assert E.predict_apply(1, 12, 10, magic=True) == E.predict_apply(1, 12, 10)
    assert E.predict_apply(1, 65, 3, magic=True) == E.predict_apply(1, 65, 3)
    assert E.predict_apply(4, 6, 3, 16, magic=True) == E.predict_apply(4, 6, 3, 16)
    assert [f.R for f in E.predict_apply(3, 5, 3, 7, 8)] == [2, 1] and [f.R for f in E.predict_apply(3, 5, 4, 7, 8)] == [2, 2]
    with pytest.raises(E.ErasureError):
        E.predict_apply(3, 5, 2, 7, 6)  # a packet that is no multiple of 4: the launch would be refused


def test_the_first_rows_flag_selects_the_loop(built):
    """loop follows the flag of the launch's first row in the first input group, and only there"""
    for ones in (False, True):
        f = E.predict_apply(1, 17, 5, row_ones=[ones, False, False, False, False])
        assert [x.loop for x in f] == [1 if ones else 0]
    got = E.predict_apply(1, 70, 10, row_ones=[True] + [False] * 7 + [True, False])
    assert [x.loop for x in got] == [1, 1, 0, 0]
    assert [x.loop for x in E.predict_apply(1, 6, 3, row_ones=[True, False, False])] == [-1]  # 18 cells: one loop
    assert [x.loop for x in E.predict_apply(1, 5, 1, row_ones=[True])] == [-1]


# ---------------------------------------------------------------- every plan is one the calls accept
def shards_of(n):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = FAKE + i * (1 << 20), 1 << 24
    return sh


@pytest.mark.parametrize("tier", AF.TIERS)
def test_every_plan_passes_the_calls_validation(all_cases, tier):
    lib = L.lib()
    for c in all_cases[tier]:
        for size in AF.sizes(c):
            try:
                p = AF.make_plan(c.method, c.k, c.m, c.w, c.packet, size)
            except E.ErasureError:
                raise AssertionError(f"{AF.case_id(c)} C={size}: {E.last_error()}")
            with p, AF.variants(*c.variants):
                n = c.k + c.m
                if c.op == "enc":
                    rc = lib.lsec_encode_dev(p.ptr, shards_of(n), 0, size, None)
                elif c.op == "magic":
                    rc = lib.lsec_encode_magic_dev(p.ptr, shards_of(n), 0, size, FAKE, None)
                else:
                    rc = lib.lsec_decode_dev(p.ptr, shards_of(n), 0, size, E._erasure_array(c.erasures), None)
                assert rc == 0, f"{AF.case_id(c)} C={size}: {E.last_error()}"
                # the forms do not depend on which of the case's sizes runs
                got = tuple(E.predict_apply_plan(p, list(c.erasures) if c.op == "dec" else None, size, magic=c.op == "magic"))
                assert got == c.forms, AF.case_id(c)
                # and the plan's answer is the shape's answer, given the plan's kernel kind and rows of ones
                if c.forms and c.op != "dec":
                    kind = c.forms[0].kind
                    ones = [f.loop == 1 for f in c.forms if not f.acc] if kind == AF.BYTEWISE else None
                    rows = sum(f.R for f in c.forms if not f.acc) if not c.forms[0].magic else c.forms[0].R
                    if ones is not None and len(c.forms) == 1:
                        ones = ones + [False] * (rows - 1)
                        assert tuple(E.predict_apply(kind, c.k, rows, c.w, c.packet, size, c.op == "magic", c.variants, ones)) == c.forms


def test_sizes_are_the_smallest_that_cover_a_tile(all_cases):
    for tier in AF.TIERS:
        for c in all_cases[tier]:
            sz = AF.sizes(c)
            assert 1 <= len(sz) <= 2 and all(s % 8 == 0 for s in sz)
            if c.packet:
                assert all(s % (c.w * c.packet) == 0 for s in sz)
                assert sz[-1] // c.w > AF.tile_bytes(c) and sz[-1] // c.w - c.packet <= -(-AF.tile_bytes(c) // c.packet) * c.packet
            else:
                assert sz[-1] == AF.tile_bytes(c) + 8 and AF.tile_bytes(c) <= max(8192, 256 * 4 * c.w)


def test_edge_plans_present(all_cases):
    have = {(c.op, c.method, c.k, c.m, c.packet) for c in all_cases["auto"]}
    want = {("enc", L.REED_SOL_VAN, k, m, 0) for k, m in ((1, 2), (2, 7), (3, 6), (17, 2), (18, 3), (19, 5), (64, 8), (65, 4), (128, 4),
                                                         (200, 4), (10, 9), (10, 16), (10, 17), (70, 10))}
    want |= {("enc", L.CAUCHY_GOOD, k, 4, 8) for k in (65, 128, 200)}
    want |= {("magic", L.REED_SOL_VAN, 64, 8, 0), ("magic", L.CAUCHY_GOOD, 64, 8, 8), ("magic", L.REED_SOL_VAN, 12, 10, 0),
             ("magic", L.REED_SOL_VAN, 65, 3, 0)}
    assert want <= have, sorted(want - have)
    # the partial decodes: every R < m on each plan, with data-only, parity-only and mixed losses
    for method, k, m, packet in AF.PARTIAL_PLANS:
        decs = [c for c in all_cases["auto"] if c.kind == "dec" and (c.method, c.k, c.m, c.packet) == (method, k, m, packet)]
        assert {len(c.erasures) for c in decs} == set(range(1, m))
        for r in range(2, m):
            kinds = {(min(c.erasures) < k, max(c.erasures) >= k) for c in decs if len(c.erasures) == r}
            assert kinds == {(True, False), (False, True), (True, True)}


def test_wide_kinds_cases(all_cases, domains):
    """kinds 3-5: both bitmatrix row counts at every word size the liberation family has among the per-w kernels, the
    any-w kernel with and without accumulate, and for the GF(2^w) kernels each R they take, plain and accumulating"""
    run = {AF.kernel_of(f) for c in all_cases["wide"] for f in c.forms}
    assert {(f.R, f.acc) for f in run if f.kind == AF.BITMATRIX and not f.sub} == {(1, 0), (2, 0), (1, 1), (2, 1)}
    per_w = {f.w for f in domains["wide"] if f.kind == AF.BITMATRIX and f.sub}
    assert all(E.predict_apply(AF.BITMATRIX, 3, 2, w, 8)[0].sub == (1 if w in per_w else 0) for w in range(2, 65))
    assert {(f.R, f.w) for f in run if f.kind == AF.BITMATRIX and f.sub} == {(r, w) for r in (1, 2) for w in per_w - {32}}
    for kind, subs in ((AF.WORDWISE, (0, 1)), (AF.BITSLICEDW, (0,))):
        for sub in subs:
            got = {(f.R, f.w, f.acc) for f in run if f.kind == kind and f.sub == sub}
            assert got == {(r, w, acc) for w in (16, 32) for r in (AF.RS if w == 16 else range(1, 5)) for acc in (0, 1)}, (kind, sub)
    # what a single launch names beyond that is the mask-per-bit kernel of more rows than a launch gets at w = 32
    assert {(f.kind, f.sub, f.w, f.R, f.acc) for f in domains["wide"] - run if f.kind != AF.BITMATRIX} == \
        {(AF.WORDWISE, 0, 32, r, acc) for r in range(5, 9) for acc in (0, 1)}


# ---------------------------------------------------------------- the figures of DESIGN.md 3.5
def test_coverage_figures(all_cases, capsys):
    """forms per tier, forms the tables of tests/test_gpu_layouts.py and tests/test_gpu_parity.py reach at their own
    shapes, forms run now (printed with -s; DESIGN.md 3.5 has them)"""
    for tier in AF.TIERS:
        forms, table, run, never = AF.coverage(tier)
        with capsys.disabled():
            print(f"\napply forms, {tier}: {forms} forms, {table} reached by the older tables, {run} run now, {never} that no plan reaches")
        assert run == forms - never and table < run
