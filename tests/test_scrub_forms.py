"""CPU: the enumeration of tests/scrub_forms.py reaches every kernel form of the check, locate, rotated and
patterned calls, and every plan it yields is one the call accepts.  No GPU: the forms come from
E.predict_form (the dispatch's own decision functions), the validation from the calls with nstripes == 0
(include/lstore_ec.h: validates, returns 0, touches no GPU) and, for the patterned decode, whose
nstripes == 0 uploads its tables, from the host table hook.

Nothing here is a count of forms.  The expectations are properties of the dispatch: every R has its
kernels, every K of LSEC_FIXED_K (E.fixed_k()) is a fixed form somewhere and no other K is, both run-time
shapes exist, and a form is a function of what the dispatch looks at, so an enumeration over all K finds it.
"""
import pytest

import lstore_amd as L
from lstore_amd import erasure as E

import scrub_forms as SF

SCRUB = ("chk", "loc", "chkrot", "locrot")
FAKE = 0x7F0000000000


@pytest.fixture(scope="module")
def all_cases(built):
    return {call: SF.cases(call) for call in SF.CALLS}


def reps(all_cases, call, sliced):
    return [c for c in all_cases[call] if c.kind == "rep" and c.form.sliced == sliced]


# ---------------------------------------------------------------- the enumeration covers the dispatch
@pytest.mark.parametrize("call", SF.CALLS)
def test_every_row_count_bytewise_and_bit_sliced(all_cases, call):
    for sliced in (False, True):
        assert {c.form.R for c in reps(all_cases, call, sliced)} == set(SF.rows_of(call)), (call, sliced)


@pytest.mark.parametrize("call", SCRUB)
def test_fixed_k_forms_and_run_time_shapes(all_cases, call):
    fixed = set(E.fixed_k())
    assert fixed and all(1 <= k <= 64 for k in fixed)
    forms = [c.form for c in reps(all_cases, call, False)]
    # every K of LSEC_FIXED_K is a fixed form for some R, at that very K, and nothing else is
    assert {f.KC for f in forms} - {0} == fixed, f"{call}: fixed-K forms {sorted({f.KC for f in forms})}, LSEC_FIXED_K {sorted(fixed)}"
    for c in reps(all_cases, call, False):
        assert c.form.KC in (0, c.k)
    for r in SF.rows_of(call):
        run_time = {(f.IT, f.VW, f.BF) for f in forms if f.R == r and f.KC == 0}
        if r == 1:
            assert run_time == {(1, 2, 0)}, f"{call}: R == 1 runs 8 B per lane with per-cell branches, got {run_time}"
        else:
            assert run_time == {(2, 4, 1), (1, 4, 1)}, f"{call} R={r}: the two run-time-K shapes, got {run_time}"
        # a fixed form has the shape that K x R has at run time too (one policy: bw_auto)
        for f in forms:
            if f.R == r and f.KC:
                assert (f.IT, f.VW, f.BF) in (run_time | {(1, 2, 0)}), f


def test_patterned_one_row_forms(all_cases):
    """the one-row kernel has fixed forms (for K of LSEC_FIXED_K only) and a run-time form; tables of two or
    more rows run with K at run time in both shapes"""
    forms = [c.form for c in reps(all_cases, "pat", False)]
    one = {f.KC for f in forms if f.R == 1}
    assert 0 in one and len(one) > 1 and one - {0} <= set(E.fixed_k())
    for r in range(2, 9):
        assert {(f.KC, f.IT, f.VW, f.BF) for f in forms if f.R == r} == {(0, 2, 4, 1), (0, 1, 4, 1)}


@pytest.mark.parametrize("call", SF.CALLS)
def test_bit_sliced_forms(all_cases, call):
    """every (R, DW) the dispatch reaches over K x packet x chunk size (4 MiB widens K >= 10) has a
    representative; the check and the locate have kernels on both sides of R * DW <= 8"""
    reach = set()
    for r in SF.rows_of(call):
        for k in SF.KS:
            for packet in SF.SLICED_PACKETS + (4, 16, 512):
                for size in (8 * packet, (4 << 20) // (8 * packet) * 8 * packet + 8 * packet):
                    f = E.predict_form(call, 2, k, r, packet, size)
                    reach.add((f.R, f.DW))
    got = {(c.form.R, c.form.DW) for c in reps(all_cases, call, True)}
    assert got == reach, f"{call}: representatives {sorted(got)}, reachable {sorted(reach)}"
    if call != "pat":
        assert {r * dw <= 8 for r, dw in got} == {True, False}
        assert {dw for _, dw in got} == {1, 2, 4}


@pytest.mark.parametrize("call", SF.CALLS)
def test_one_representative_per_form(all_cases, call):
    every = set()
    for kernel, packets in ((1, (0,)), (2, SF.SLICED_PACKETS)):
        for r in SF.rows_of(call):
            for k in SF.KS:
                for packet in packets:
                    every.add(E.predict_form(call, kernel, k, r, packet, SF.small_size(packet)))
    rep_forms = [c.form for c in all_cases[call] if c.kind == "rep"]
    assert len(rep_forms) == len(set(rep_forms)) and set(rep_forms) == every
    # the smallest K: no smaller K of the same row count has the form
    for c in all_cases[call]:
        if c.kind == "rep":
            for k in range(1, c.k):
                for packet in (SF.SLICED_PACKETS if c.form.sliced else (0,)):
                    assert SF.predict(call, c.method, k, c.rows, packet) != c.form, (SF.case_id(c), k)
    # an edge plan defines no form of its own
    assert {c.form for c in all_cases[call] if c.kind == "edge"} <= every


@pytest.mark.parametrize("call", SF.CALLS)
def test_edge_plans_present(all_cases, call):
    have = {(c.method, c.k, c.m, c.packet) for c in all_cases[call]}  # (an edge plan may be a representative already)
    assert any(c.kind == "edge" for c in all_cases[call])
    want = {(L.REED_SOL_VAN, 1, 2, 0), (L.REED_SOL_VAN, 2, 7, 0), (L.REED_SOL_VAN, 3, 6, 0), (L.REED_SOL_VAN, 17, 2, 0),
            (L.REED_SOL_VAN, 18, 3, 0), (L.REED_SOL_VAN, 19, 5, 0), (L.REED_SOL_VAN, 33, 5, 0), (L.REED_SOL_VAN, 64, 8, 0),
            (L.CAUCHY_GOOD, 64, 8, 8)}
    if call in ("chk", "chkrot", "pat"):
        want |= {(L.RAID4, 5, 1, 0), (L.CAUCHY_GOOD, 3, 1, 8)}
    if call == "pat":
        want.add((L.REED_SOL_VAN, 64, 64, 0))
    assert want <= have, sorted(want - have)
    if call != "pat":
        assert (L.REED_SOL_VAN, 64, 64, 0) not in have
    ids = [SF.case_id(c) for c in all_cases[call]]
    assert len(ids) == len(set(ids))


def test_the_rotated_twins_take_their_unrotated_shapes(all_cases):
    for plain, rot in (("chk", "chkrot"), ("loc", "locrot")):
        assert [c._replace(call=rot, form=c.form._replace(family=rot)) for c in all_cases[plain]] == all_cases[rot]


def test_rotated_repair_forms(built):
    """the rotated repair is the one-row patterned decode: the same forms under its own family"""
    for kernel, packet in ((1, 0), (2, 8)):
        for k in SF.KS:
            assert E.predict_form("patrot", kernel, k, 1, packet, 64) == \
                E.predict_form("pat", kernel, k, 1, packet, 64)._replace(family="patrot")
    with pytest.raises(E.ErasureError):
        E.predict_form("patrot", 1, 6, 2)
    with pytest.raises(E.ErasureError):
        E.predict_form("loc", 1, 6, 1)
    assert E.predict_forms("locrot", 1, 10, 3, repair=True)[1] == E.predict_form("patrot", 1, 10, 1)
    assert E.launch_record() == [] or all(isinstance(f, E.Form) for f in E.launch_record())


# ---------------------------------------------------------------- every plan is one the call accepts
def shards_of(n):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = FAKE + i * (1 << 20), 1 << 24
    return sh


def validate(c, p, size):
    """the call's own argument validation for case c: 0, or -1 with lsec_last_error set"""
    lib, n = L.lib(), p.k + p.m
    if c.call == "chk":
        return lib.lsec_check_dev(p.ptr, shards_of(n), 0, size, None, None, None)
    if c.call == "loc":
        return lib.lsec_locate_dev(p.ptr, shards_of(n), 0, size, None, None, None, None, 0, None)
    if c.call == "chkrot":
        return lib.lsec_check_dev_rotated(p.ptr, shards_of(n), 0, size, 1, 3_000_000_007, None, None, None)
    if c.call == "locrot":
        return lib.lsec_locate_dev_rotated(p.ptr, shards_of(n), 0, size, 1, 3_000_000_007, None, None, None, None, None, None,
                                           E.LOCATE_REPAIR, None)
    # pat: the host table of a pattern of `rows` erasures, the last chunk among them, and of a single one
    pats = [list(range(c.rows - 1)) + [n - 1], [0]]
    try:
        nout, _, out_sel, _ = E.pattern_table_entry(p, 0, patterns=pats)
    except E.ErasureError:
        return -1
    lost_only_parity = p.method == L.RAID4 and c.rows == 1
    assert (nout, out_sel[-1:]) == ((0, []) if lost_only_parity else (c.rows, [n - 1])), (SF.case_id(c), nout, out_sel)
    return 0


@pytest.mark.parametrize("call", SF.CALLS)
def test_every_plan_passes_the_calls_validation(all_cases, call):
    for c in all_cases[call]:
        for size in SF.sizes(c):
            with SF.make_plan(c.method, c.k, c.m, c.packet, size) as p:
                assert p.kernel == SF.plan_kernel(c.method), SF.case_id(c)
                assert validate(c, p, size) == 0, f"{SF.case_id(c)} C={size}: {E.last_error()}"
                # the form does not depend on which of the case's sizes runs
                assert SF.predict(call, c.method, c.k, c.rows, c.packet, size) == c.form


# ---------------------------------------------------------------- just outside the limits
def test_patterned_limits(built):
    """k = 65, a pattern of nine erasures, k + m = 129: refused with the limit named.  (k = 65 and m = 9 of the
    check and the locate calls: test_check_args.py, test_locate_args.py, test_rotated_scrub_args.py.)"""
    lib = L.lib()

    def call(p, pats):
        n = p.k + p.m
        flat = E._pattern_array(pats)
        return lib.lsec_decode_dev_patterns(p.ptr, shards_of(n), 0, 4096, flat, len(pats), None, None)

    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        assert call(p, [[0]]) == -1 and "k=65 outside 1..64" in E.last_error(), E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        assert call(p, [[0], list(range(9))]) == -1 and "9 erasures in one pattern exceed 8" in E.last_error(), E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 64, 65, 8, 0, 8) as p:
        assert call(p, [[0]]) == -1 and "k+m=129 exceeds 128" in E.last_error(), E.last_error()
    # at the limits the same calls get as far as the host table (RS(64+64), eight erasures)
    with SF.make_plan(L.REED_SOL_VAN, 64, 64, 0, 4096) as p:
        nout, in_sel, out_sel, rows = E.pattern_table_entry(p, 0, patterns=[[0, 1, 2, 3, 64, 100, 126, 127]])
        assert nout == 8 and out_sel == [0, 1, 2, 3, 64, 100, 126, 127] and len(in_sel) == 64 and rows.shape == (8, 64)
        assert (rows != 0).any(axis=1).all()
