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


# ---------------------------------------------------------------- the families added since: SF.NEW_CALLS
@pytest.fixture(scope="module")
def new_cases(built):
    return {call: SF.cases(call) for call in SF.NEW_CALLS}


def big_size(packet):
    """a chunk of 4 MiB (bit-sliced: the whole super-packets past it), where cauchy8_bitsliced_dw widens K >= 10"""
    return (4 << 20) // (8 * packet) * 8 * packet + 8 * packet if packet else 4 << 20


def domain_forms(call, sizes=(SF.small_size, big_size)):
    """every form the call's hook predicts over K = 1..64 x its rows x bytewise and SLICED_PACKETS x the chunk sizes"""
    every = set()
    for method, packets in ((L.REED_SOL_VAN, (0,)), (L.CAUCHY_GOOD, SF.SLICED_PACKETS)):
        for r in SF.rows_of(call):
            for k in SF.KS:
                for packet in packets:
                    for size in sizes:
                        every.add(SF.predict(call, method, k, r, packet, size(packet)))
    return every


def test_the_new_calls_are_the_twelve():
    assert len(SF.NEW_CALLS) == len(set(SF.NEW_CALLS)) == 12 and not set(SF.NEW_CALLS) & set(SF.CALLS)
    assert set(SF.UPDATES) | set(SF.MASKED) | set(SF.WITH_MAGICS) | set(SF.PATTERNED) | set(SF.ROTATED) <= set(SF.NEW_CALLS) | set(SF.CALLS)
    assert set(SF.MASKED) <= set(SF.UPDATES)


@pytest.mark.parametrize("call", SF.NEW_CALLS)
def test_closure(new_cases, call):
    """THE completeness condition: every form the hook predicts anywhere in the domain, at either chunk-size regime,
    is the form of some case of cases(call); ids are unique; an edge plan defines no form of its own"""
    every = domain_forms(call)
    have = {c.form for c in new_cases[call]}
    assert every <= have, f"{call}: no case for {sorted(every - have)}"
    rep_forms = [c.form for c in new_cases[call] if c.kind == "rep"]
    assert len(rep_forms) == len(set(rep_forms)) and set(rep_forms) == domain_forms(call, (SF.small_size,))
    assert every == set(rep_forms)  # (4 MiB gives K = 10..15 the forms K >= 16 has at any size, no further one)
    assert have == set(rep_forms)
    ids = [SF.case_id(c) for c in new_cases[call]]
    assert len(ids) == len(set(ids))
    for sliced in (False, True):
        assert {c.form.R for c in new_cases[call] if c.kind == "rep" and c.form.sliced == sliced} == set(range(1, 9)), (call, sliced)


@pytest.mark.parametrize("call", SF.NEW_CALLS)
def test_representatives_sit_at_the_first_k_of_their_form(new_cases, call):
    for c in new_cases[call]:
        if c.kind != "rep":
            continue
        walked = SF.ks_of(call)
        for k in walked[:walked.index(c.k)]:
            for packet in (SF.SLICED_PACKETS if c.form.sliced else (0,)):
                assert SF.predict(call, c.method, k, c.rows, packet) != c.form, (SF.case_id(c), k)
        if call in SF.UPDATES:
            assert c.k >= 5 and (c.k == 5 or c.form.sliced), SF.case_id(c)
            assert c.m == c.rows and c.method == (L.CAUCHY_GOOD if c.form.sliced else L.RAID4 if c.m == 1 else L.REED_SOL_VAN)
        if call in SF.PATTERNED:
            assert c.m == max(c.rows, 2)


@pytest.mark.parametrize("call", SF.UPDATES)
def test_update_forms(new_cases, call):
    """bytewise one kernel per R, K at run time: 8 B per lane with branches at R = 1, two 16-byte steps per lane up to
    four rows (kUpdTwoStepRows) and one above; bit-sliced 1, 2 and 4 dwords per lane up to four rows, one above"""
    forms = [c.form for c in new_cases[call] if c.kind == "rep"]
    assert {(f.R, f.KC, f.IT, f.VW, f.BF) for f in forms if not f.sliced} == \
        {(1, 0, 1, 2, 0)} | {(r, 0, 2 if r <= 4 else 1, 4, 1) for r in range(2, 9)}
    assert {(f.R, f.DW) for f in forms if f.sliced} == {(r, dw) for r in range(1, 9) for dw in ((1, 2, 4) if r <= 4 else (1,))}
    # no form depends on K bytewise: every edge plan runs a representative's kernel
    assert all(c.form.KC == 0 for c in new_cases[call])


@pytest.mark.parametrize("call", ("encrot", "chkmagic", "chkmagicrot", "encmagicrot"))
def test_check_shaped_forms(new_cases, call):
    """the families shaped by chk_bytewise_form: every K of LSEC_FIXED_K is a fixed form somewhere, at that very K,
    both run-time shapes exist for every R >= 2, and the forms the tables of codes never reached are there: fixed K
    with two steps per lane at four rows and more (the magic check's early order at IT == 2), and R = 5 at K = 20"""
    reps = [c for c in new_cases[call] if c.kind == "rep" and not c.form.sliced]
    forms = [c.form for c in reps]
    assert {f.KC for f in forms} - {0} == set(E.fixed_k())
    assert all(c.form.KC in (0, c.k) for c in reps)
    for r in range(2, 9):
        assert {(f.IT, f.VW, f.BF) for f in forms if f.R == r and f.KC == 0} == {(2, 4, 1), (1, 4, 1)}, (call, r)
    assert {(f.IT, f.VW, f.BF) for f in forms if f.R == 1 and f.KC == 0} == {(1, 2, 0)}
    assert any(f.KC and f.IT == 2 and f.BF and f.R >= 4 for f in forms)
    assert any(f.KC and f.IT == 2 and f.BF and f.R < 4 for f in forms)
    assert any((f.R, f.KC, f.IT) == (5, 20, 1) for f in forms)
    sliced = {(c.form.R, c.form.DW) for c in new_cases[call] if c.kind == "rep" and c.form.sliced}
    assert sliced == {(r, dw) for r in range(1, 9) for dw in ((1, 2, 4) if r <= 4 else (1,))}


@pytest.mark.parametrize("call", ("patmagic", "patmagicrot"))
def test_patterned_magic_forms(new_cases, call):
    """the plain patterned decode's shapes under the family of their own: fixed forms for one row alone"""
    assert [c._replace(call="pat", form=c.form._replace(family="pat")) for c in new_cases[call]] == \
        [c for c in SF.cases("pat") if c.m <= 8]
    assert {c.form.family for c in new_cases[call]} == {"patmagic"}


def test_patterned_magic_limit(built):
    """RS(64+64), the plain patterned decode's k + m = 128 plan, is no plan of the decodes that leave the magics: they
    take m <= 8 and say so before the first HIP call (the fake pointers are never dereferenced)"""
    lib = L.lib()
    with SF.make_plan(L.REED_SOL_VAN, 64, 64, 0, 4096) as p:
        flat = E._pattern_array([[0]])
        assert lib.lsec_decode_magic_dev_patterns(p.ptr, shards_of(128), 0, 4096, flat, 1, FAKE, FAKE + 1, None, None, None, None) == -1
        assert "m=64 outside 1..8" in E.last_error(), E.last_error()
        assert lib.lsec_decode_magic_dev_rotated(p.ptr, shards_of(128), 0, 4096, E._erasure_array([1]), 1, 5, FAKE + 1, None, None,
                                                 None, None) == -1
        assert "m=64 outside 1..8" in E.last_error(), E.last_error()


def test_the_new_rotated_twins_take_their_unrotated_shapes(new_cases):
    for plain, rot, family in (("upd", "updrot", "updrot"), ("updmask", "updmaskrot", "updmask"),
                               ("updmagic", "updmagicrot", "updmaskmagic"), ("chkmagic", "chkmagicrot", "chkmagicrot"),
                               ("patmagic", "patmagicrot", "patmagic")):
        assert [c._replace(call=rot, form=c.form._replace(family=family)) for c in new_cases[plain]] == new_cases[rot]
    # the rotated encodes take the check's shape for the same K x R, bytewise and bit-sliced
    chk = [c.form._replace(family="") for c in SF.cases("chk") if c.kind == "rep"]
    for call in ("encrot", "encmagicrot", "chkmagic"):
        assert [c.form._replace(family="") for c in new_cases[call] if c.kind == "rep"] == chk, call


@pytest.mark.parametrize("call", SF.NEW_CALLS)
def test_new_edge_plans(new_cases, call):
    import test_gpu_check_magic as TCM

    have = {(c.method, c.k, c.m, c.packet) for c in new_cases[call]}
    want = {e[:4] for e in SF.EDGES}
    if call in SF.WITH_MAGICS:
        assert {e[:4] for e in SF.MAGIC_EDGES} == set(TCM.EDGES.values())
        want |= set(TCM.EDGES.values())
    if call in SF.MASKED:
        # the seven mask words of the masked rigs need four columns
        assert {p for p in want if p[1] < 4} and all(c.k >= 4 for c in new_cases[call])
        want = {p for p in want if p[1] >= 4}
    assert want <= have, sorted(want - have)
    assert (L.REED_SOL_VAN, 64, 64, 0) not in have and all(c.k <= 64 and c.m <= 8 for c in new_cases[call])
    assert (L.REED_SOL_VAN, 64, 8, 0) in have and (L.CAUCHY_GOOD, 64, 8, 8) in have  # chunk id 71


def refs_of(n):
    return [(FAKE + i * (1 << 20), 1 << 24) for i in range(n)]


def validate_new(c, p, size):
    """the call's own argument validation for case c (nstripes == 0: validates, touches no GPU): 0, or -1 with
    lsec_last_error set.  The patterned decodes, whose nstripes == 0 uploads their tables: the limits their header
    documents (test_patterned_magic_limit has the refusal) and the host table hook."""
    k, n, call = p.k, p.k + p.m, c.call
    assert 1 <= p.k <= 64 and 1 <= p.m <= 8, SF.case_id(c)
    rot = (1, 3_000_000_007)
    try:
        if call == "upd":
            p.update_dev_refs(refs_of(n), 0, size, [0, k // 2, k - 1][:k], refs_of(min(k, 3)), True)
        elif call == "updrot":
            p.update_dev_rotated_refs(refs_of(n), 0, size, *rot, [0, k // 2, k - 1][:k], refs_of(min(k, 3)), True)
        elif call == "encrot":
            p.encode_dev_rotated_refs(refs_of(n), 0, size, *rot)
        elif call == "updmask":
            p.update_dev_masked_refs(refs_of(n), 0, size, FAKE, refs_of(k), True)
        elif call == "updmaskrot":
            p.update_dev_masked_rotated_refs(refs_of(n), 0, size, *rot, FAKE, refs_of(k), True)
        elif call == "updmagic":
            p.update_magic_dev_masked_refs(refs_of(n), 0, size, FAKE, refs_of(k), FAKE + 1, True)
        elif call == "updmagicrot":
            p.update_magic_dev_masked_rotated_refs(refs_of(n), 0, size, *rot, FAKE, refs_of(k), FAKE + 1, True)
        elif call == "chkmagic":
            p.check_magic_dev_refs(refs_of(n), 0, size, FAKE, FAKE + 1, FAKE + 3, FAKE + 5, FAKE + 8)
        elif call == "chkmagicrot":
            p.check_magic_dev_rotated_refs(refs_of(n), 0, size, *rot, FAKE, FAKE + 1, FAKE + 3, FAKE + 5, FAKE + 8)
        elif call == "encmagicrot":
            p.encode_magic_dev_rotated_refs(refs_of(n), 0, size, *rot, FAKE + 1)
        elif call == "patmagic":
            nout, _, out_sel, _ = E.pattern_table_entry(p, 0, patterns=[list(range(c.rows - 1)) + [n - 1], [0]])
            lost_only_parity = p.method == L.RAID4 and c.rows == 1
            assert (nout, out_sel[-1:]) == ((0, []) if lost_only_parity else (c.rows, [n - 1])), (SF.case_id(c), nout, out_sel)
        else:  # patmagicrot: the table entry of every rotation that occurs
            lost = sorted(set(range(c.rows - 1)) | {n - 1})
            for r in range(n):
                nout, _, out_sel, _ = E.pattern_table_entry(p, r, lost=lost, n_shift=1)
                assert nout in (0, c.rows) and len(out_sel) == nout, (SF.case_id(c), r, nout)
    except E.ErasureError:
        return -1
    return 0


@pytest.mark.parametrize("call", SF.NEW_CALLS)
def test_every_new_plan_passes_the_calls_validation(new_cases, call):
    for c in new_cases[call]:
        for size in SF.sizes(c):
            with SF.make_plan(c.method, c.k, c.m, c.packet, size) as p:
                assert p.kernel == SF.plan_kernel(c.method), SF.case_id(c)
                assert validate_new(c, p, size) == 0, f"{SF.case_id(c)} C={size}: {E.last_error()}"
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
